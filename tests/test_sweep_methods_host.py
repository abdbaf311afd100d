"""Host side of the lock-step `linear_probing` / `adapter_reg` sweeps, no GPU: the argument checks of the two C entries of
csrc/linear_sweep.hip on host pointers -- nothing is launched on these paths -- and their workspace functions; the routing of
trainer.train_sweep; the per-replica random streams, the reference's result table and file name for both methods.
tests/golden/sweep_wb_{linear_probing,adapter_reg}.npz hold what the reference's own sweep driver
(run_multiple/final_main_iteration_wb.py, its seed loop and table code unmodified; tools/make_golden_sweep_methods.py) produced."""
import ctypes
import json
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from dbmm_amd import _lib, adapter, synth, trainer

SHAPE, ALIGN, WORKSPACE, ARG = -1, -2, -3, -4


@pytest.fixture(scope="module")
def L():
    _lib.build()
    return _lib.lib()


def test_linear_sweep_entries_refuse_bad_arguments_without_a_gpu(L):
    buf = (ctypes.c_float * 4096)()
    p = ctypes.c_void_p((ctypes.addressof(buf) + 15) // 16 * 16)      # a 16-B aligned host address
    off = ctypes.c_void_p(p.value + 4)
    lr = (ctypes.c_float * 16)(*[0.1] * 16)

    def step(R=2, B=8, D=512, C=2, G=4, idx_R=None, idx_B=None, ws_bytes=None, table=p, idx=p, w=p, mw=p, ws=p, lrs=lr, n_rows=100):
        need = L.dbmm_workspace_bytes_linear_sweep_step(R, B, D, C)
        return L.dbmm_linear_sweep_step(table, n_rows, idx, R if idx_R is None else idx_R, B if idx_B is None else idx_B, p, p, w, p, mw, p, lrs,
                                        0.9, 0.0, 1, p, p, p, p, p, G, 1, R, B, D, C, ws, need if ws_bytes is None else ws_bytes, None)

    def evaluate(R=2, B=8, D=512, C=2, G=4, row0=0, ws_bytes=None, table=p, w=p, ws=p, idx=None, n_rows=100):
        need = L.dbmm_workspace_bytes_linear_sweep_eval(R, B)
        return L.dbmm_linear_sweep_eval(table, n_rows, idx, row0, p, p, w, p, p, p, p, p, G, R, B, D, C, ws, need if ws_bytes is None else ws_bytes,
                                        None)
    assert step(R=0) == SHAPE and step(R=17) == SHAPE and evaluate(R=0) == SHAPE and evaluate(R=17) == SHAPE
    assert step(idx_R=3) == SHAPE and step(idx_B=9) == SHAPE                      # idx is not [R, B]
    assert step(C=0) == SHAPE and step(C=9) == SHAPE and evaluate(C=0) == SHAPE and evaluate(C=9) == SHAPE
    assert step(D=510) == SHAPE and step(D=1028) == SHAPE and evaluate(D=6) == SHAPE and evaluate(D=2048) == SHAPE
    assert step(G=65) == SHAPE and evaluate(G=65) == SHAPE and step(G=0) == SHAPE
    assert step(B=0) == SHAPE and evaluate(B=0) == SHAPE
    assert evaluate(row0=95) == SHAPE and evaluate(row0=-1) == SHAPE              # rows 95 .. 102 of a 100-row table
    # rows 92 .. 99 fit, and with an index list row0 is not used: shown by the LATER workspace check refusing the call, so that no
    # call of this test passes validation
    assert evaluate(row0=92, ws_bytes=0) == WORKSPACE and evaluate(row0=95, idx=p, ws_bytes=0) == WORKSPACE
    assert step(table=None) == ARG and step(idx=None) == ARG and step(w=None) == ARG and step(mw=None) == ARG and step(ws=None) == ARG
    assert step(lrs=None) == ARG and evaluate(table=None) == ARG and evaluate(w=None) == ARG and evaluate(ws=None) == ARG
    assert step(table=off) == ALIGN and step(w=off) == ALIGN and step(mw=off) == ALIGN and step(ws=off) == ALIGN
    assert evaluate(table=off) == ALIGN and evaluate(w=off) == ALIGN and evaluate(ws=off) == ALIGN
    assert step(ws_bytes=L.dbmm_workspace_bytes_linear_sweep_step(2, 8, 512, 2) - 4) == WORKSPACE
    assert evaluate(ws_bytes=L.dbmm_workspace_bytes_linear_sweep_eval(2, 8) - 4) == WORKSPACE
    assert step(R=17, table=None) == ARG                                          # null pointers are reported first


def test_linear_sweep_workspace_is_linear_in_the_replicas(L):
    for B, D, C in ((1, 4, 1), (8, 512, 2), (512, 1024, 8), (513, 768, 4), (4100, 1024, 2)):
        one = L.dbmm_workspace_bytes_linear_sweep_step(1, B, D, C)
        assert one > 0 and one % 16 == 0
        assert one >= L.dbmm_workspace_bytes_linear_train_step(B, D, C)          # a replica's share holds the single step's workspace
        for R in (2, 3, 8, 16):
            assert L.dbmm_workspace_bytes_linear_sweep_step(R, B, D, C) == R * one
        e1 = L.dbmm_workspace_bytes_linear_sweep_eval(1, B)
        assert e1 > 0 and e1 % 16 == 0 and all(L.dbmm_workspace_bytes_linear_sweep_eval(R, B) == R * e1 for R in (2, 5, 16))
    for R, B, D, C in ((0, 8, 512, 2), (17, 8, 512, 2), (2, 0, 512, 2), (2, 8, 510, 2), (2, 8, 1028, 2), (2, 8, 512, 0), (2, 8, 512, 9)):
        assert L.dbmm_workspace_bytes_linear_sweep_step(R, B, D, C) == 0, (R, B, D, C)
    assert L.dbmm_workspace_bytes_linear_sweep_eval(0, 8) == 0 and L.dbmm_workspace_bytes_linear_sweep_eval(17, 8) == 0
    assert L.dbmm_workspace_bytes_linear_sweep_eval(2, 0) == 0


def test_train_sweep_routes_the_two_methods_to_their_lock_step_schedules(monkeypatch):
    """eligibility: linear_probing with R >= 2, n_cls <= 8, D % 4 == 0, D <= 1024; adapter_reg under the adapter path's conditions;
    everything else replica by replica; more than 16 replicas in groups of 16.  Observed where train_sweep hands a group to the
    schedule: which executor, which method, how many replicas"""
    import torch
    calls = []

    def schedule(ex, opts, *a, **k):
        assert type(ex) is trainer._LockStep and ex.R == len(opts) == len(ex.streams.states)
        calls.append((opts[0].tl_method, len(opts)))
        return [None] * len(opts)
    monkeypatch.setattr(trainer, "_run_schedule", schedule)
    monkeypatch.setattr(trainer, "train_all_epochs", lambda o, *a, **k: calls.append(("sequential", 1)))
    monkeypatch.setattr(trainer.ops, "get_option", lambda name: 1)

    def run(method, D, seeds, **kw):
        calls.clear()
        opt = SimpleNamespace(tl_method=method, n_cls=2, adapter_feat_dim=128, learning_rate=0.1, **kw)
        table = SimpleNamespace(embeddings=torch.zeros(4, D))
        out = trainer.train_sweep(opt, table, table, table, seeds)
        assert len(out) == len(seeds)
        return list(calls)
    assert run("linear_probing", 1024, range(3)) == [("linear_probing", 3)]
    assert run("linear_probing", 20, range(18)) == [("linear_probing", 16), ("linear_probing", 2)]
    assert run("linear_probing", 1028, range(2)) == [("sequential", 1)] * 2
    assert run("linear_probing", 1022, range(2)) == [("sequential", 1)] * 2
    assert run("linear_probing", 512, [7]) == [("sequential", 1)]
    calls.clear()
    opt = SimpleNamespace(tl_method="linear_probing", n_cls=9, adapter_feat_dim=128, learning_rate=0.1)
    table = SimpleNamespace(embeddings=torch.zeros(4, 512))
    trainer.train_sweep(opt, table, table, table, [0, 1])
    assert calls == [("sequential", 1)] * 2
    assert run("adapter_reg", 512, range(17)) == [("adapter_reg", 16), ("adapter_reg", 1)]
    assert run("adapter_reg", 500, range(2)) == [("sequential", 1)] * 2
    assert run("adapter_reg_seq", 512, range(2)) == [("adapter_reg_seq", 2)]
    with pytest.raises(ValueError):
        run("contrastive_adapter", 512, range(2))


# ---- against the reference's own sweep driver ---------------------------------------------------------------------------------

METHODS = ("linear_probing", "adapter_reg")


@pytest.fixture(scope="module", params=METHODS)
def g(request):
    return np.load(os.path.join(GOLDEN, f"sweep_wb_{request.param}.npz"), allow_pickle=False)


def _sample(t, n=256):
    f = t.detach().double().flatten()
    return f[::max(1, f.numel() // n)][:n].float().numpy()


def test_interleaved_replica_streams_draw_what_separate_runs_draw(g):
    """the host-side draws of both schedules (initialisations, shuffle orders, balanced subsets, the base-seed draws of un-shuffled
    and evaluation passes), taken replica by replica WITHIN every epoch through ReplicaStreams, are the ones the reference drew in
    three separate set_seed(s) runs"""
    cfg, o = json.loads(str(g["config"])), json.loads(str(g["opt"]))
    seeds = [int(s) for s in g["seeds"]]
    R = len(seeds)
    linear = o["tl_method"] == "linear_probing"
    _, y, c = synth.embedding_dataset(cfg["seed"], "val", cfg["n_val"], cfg["dim"])
    group_array = adapter.group_index(y.numpy(), c.numpy())[2]
    reg_idx, _ = adapter.stratified_split_indices(group_array, 0.5)
    streams = trainer.ReplicaStreams(seeds)
    draw = lambda: torch.empty((), dtype=torch.int64).random_()
    orders = [[] for _ in range(R)]
    balanced = [[] for _ in range(R)]
    if linear:
        inits = [streams.run(r, adapter.LinearClassifier, cfg["dim"], o["n_cls"]).state_dict() for r in range(R)]
    else:
        inits = [streams.run(r, adapter.Adapter, cfg["dim"], o["adapter_feat_dim"]).state_dict() for r in range(R)]
    for epoch in range(1, o["epochs"] + 1):
        if not linear:
            for r in range(R):
                balanced[r].append(streams.run(r, adapter.balance_val_indices, group_array[reg_idx], 4, o["batch_size_reg"]))
        for r in range(R):
            orders[r].append(streams.run(r, trainer.dataloader_shuffle_order, cfg["n_train"]).numpy())
        if not linear:
            for r in range(R):
                streams.run(r, draw)                          # the un-shuffled loader over the balanced subset
                orders[r][-1] = np.concatenate([orders[r][-1], reg_idx[balanced[r][-1][0]]])
        for _ in range(2):                                    # the val and the test pass
            for r in range(R):
                streams.run(r, draw)
    for r in range(R):
        train = [i for i in range(int(g[f"s{r}/n_phases"])) if str(g[f"s{r}/p{i}/kind"]) in ("train1", "train_reg")]
        assert len(train) == len(orders[r]) == o["epochs"]
        for e, (i, mine) in enumerate(zip(train, orders[r])):
            assert np.array_equal(np.asarray(mine, dtype=np.int64), g[f"s{r}/p{i}/idx"].astype(np.int64)), (r, e)
            if not linear:
                assert int(g[f"s{r}/p{i}/n_train"]) == cfg["n_train"]
        for e, (bi, bs) in enumerate(balanced[r]):
            assert np.array_equal(bi, g[f"s{r}/balanced{e}/indices"]) and bs == int(g[f"s{r}/balanced{e}/batch_size"]), (r, e)
        for k, v in inits[r].items():
            assert np.array_equal(_sample(v), g[f"s{r}/init0/{k}_sample"]), (r, k)


def _fixture_results(g):
    out = []
    for s in range(int(g["n_seeds"])):
        d = {tag: {str(k): float(v) for k, v in zip(g[f"s{s}/final/{tag}_keys"], g[f"s{s}/final/{tag}"])} for tag in ("tr", "val", "test", "zs_tg", "zs_spu")}
        out.append(((d["tr"], d["val"], d["test"]), (d["zs_tg"], d["zs_spu"])))
    return out


def test_sweep_frame_and_result_name_are_the_references(g):
    frame = trainer.sweep_frame(_fixture_results(g))
    assert [str(i) for i in frame.index] == [str(i) for i in g["table/index"]]
    assert [str(c) for c in frame.columns] == [str(c) for c in g["table/columns"]]
    assert np.array_equal(frame.to_numpy(dtype=np.float64), g["table/values"], equal_nan=True)
    assert trainer.sweep_result_name(SimpleNamespace(**json.loads(str(g["opt"])))) == str(g["table/name"])
