"""Host side of the seed sweep (trainer.train_sweep), no GPU: the per-replica random streams, the reference's result table and file
name, and the argument checks of the replica-batched C entries.  tests/golden/sweep_wb.npz holds what the reference's own sweep
driver (run_multiple/final_main_iteration_wb.py, its seed loop and table code unmodified; tools/make_golden_sweep.py) produced."""
import ctypes
import json
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from dbmm_amd import _lib, adapter, optim, trainer


@pytest.fixture(scope="module")
def g():
    return np.load(os.path.join(GOLDEN, "sweep_wb.npz"), allow_pickle=False)


def _sample(t, n=256):
    f = t.detach().double().flatten()
    return f[::max(1, f.numel() // n)][:n].float().numpy()


def _passes(g, s):
    return [{k: g[f"s{s}/p{i}/{k}"] for k in ("kind", "idx") if f"s{s}/p{i}/{k}" in g.files} for i in range(int(g[f"s{s}/n_phases"]))]


def test_interleaved_replica_streams_draw_what_separate_runs_draw(g):
    """the host-side draws of the fixture's schedule (adapter initialisations, shuffle orders, balanced subsets, the base-seed draws
    of un-shuffled passes), taken replica by replica WITHIN every epoch through ReplicaStreams, are the ones the reference drew in
    three separate set_seed(s) runs"""
    cfg, o = json.loads(str(g["config"])), json.loads(str(g["opt"]))
    seeds = [int(s) for s in g["seeds"]]
    R = len(seeds)
    D, Hd = cfg["dim"], o["adapter_feat_dim"]
    from dbmm_amd import synth
    _, y, c = synth.embedding_dataset(cfg["seed"], "val", cfg["n_val"], cfg["dim"])
    group_array = adapter.group_index(y.numpy(), c.numpy())[2]
    reg_idx, _ = adapter.stratified_split_indices(group_array, 0.5)
    streams = trainer.ReplicaStreams(seeds)
    draw = lambda: torch.empty((), dtype=torch.int64).random_()
    inits = [[] for _ in range(R)]
    orders = [[] for _ in range(R)]
    balanced = [[] for _ in range(R)]
    for r in range(R):
        inits[r].append(streams.run(r, adapter.Adapter, D, Hd).state_dict())
    for epoch in range(1, o["epochs"] + 1):
        for r in range(R):
            balanced[r].append(streams.run(r, adapter.balance_val_indices, group_array[reg_idx], 4, o["batch_size_reg"]))
        if epoch == o["epochs_feature_learning"] + 1:
            for r in range(R):
                inits[r].append(streams.run(r, adapter.Adapter, D, Hd).state_dict())
        for r in range(R):
            if epoch <= o["epochs_feature_learning"]:
                orders[r].append(streams.run(r, trainer.dataloader_shuffle_order, cfg["n_train"]).numpy())
            else:
                streams.run(r, draw)
                orders[r].append(reg_idx[balanced[r][-1][0]])
        for _ in range(2):                                    # the val and the test pass
            for r in range(R):
                streams.run(r, draw)
    for r in range(R):
        train = [p for p in _passes(g, r) if str(p["kind"]) in ("train1", "train2")]
        assert len(train) == len(orders[r]) == o["epochs"]
        for e, (p, mine) in enumerate(zip(train, orders[r])):
            assert np.array_equal(np.asarray(mine, dtype=np.int64), p["idx"].astype(np.int64)), (r, e)
        for e, (bi, bs) in enumerate(balanced[r]):
            assert np.array_equal(bi, g[f"s{r}/balanced{e}/indices"]) and bs == int(g[f"s{r}/balanced{e}/batch_size"]), (r, e)
        for i, sd in enumerate(inits[r]):
            for k, v in sd.items():
                assert np.array_equal(_sample(v), g[f"s{r}/init{i}/{k}_sample"]), (r, i, k)


def _results(g):
    out = []
    for s in range(int(g["n_seeds"])):
        d = {tag: {str(k): float(v) for k, v in zip(g[f"s{s}/final/{tag}_keys"], g[f"s{s}/final/{tag}"])} for tag in ("tr", "val", "test", "zs_tg", "zs_spu")}
        out.append(((d["tr"], d["val"], d["test"]), (d["zs_tg"], d["zs_spu"])))
    return out


def test_sweep_frame_is_the_references_table(g):
    frame = trainer.sweep_frame(_results(g))
    assert [str(i) for i in frame.index] == [str(i) for i in g["table/index"]]
    assert [str(c) for c in frame.columns] == [str(c) for c in g["table/columns"]]
    assert np.array_equal(frame.to_numpy(dtype=np.float64), g["table/values"], equal_nan=True)


def test_sweep_result_name_is_the_references(g):
    opt = SimpleNamespace(**json.loads(str(g["opt"])))
    assert trainer.sweep_result_name(opt) == str(g["table/name"])
    base = dict(dataset="waterbirds", batch_size=128, learning_rate=0.1, learning_rate_reg=0.01, batch_size_reg=4, balance_val=False,
                use_cls_prompt_in_reg=False, add_adapter=False, init_near_identity=False, continue_from_best=False, resample_ce=False)
    name = lambda **kw: trainer.sweep_result_name(SimpleNamespace(**{**base, **kw}))
    assert name(tl_method="adapter") == "ds_waterbirds_tl_adapter_bs_128_lr_0.1"
    assert name(tl_method="adapter", resample_ce=True, balance_val=True) == "ds_waterbirds_tl_adapter_bs_128_lr_0.1_rs"
    assert name(tl_method="adapter_reg", use_cls_prompt_in_reg=True) == "ds_waterbirds_tl_adapter_reg_bs_128_lr_0.1_lrr0.01_bsr4_CP"
    assert name(tl_method="adapter_reg", continue_from_best=True) == "ds_waterbirds_tl_adapter_reg_bs_128_lr_0.1_lrr0.01_bsr4_GP"
    assert (name(tl_method="adapter_reg_seq", balance_val=True, add_adapter=True, init_near_identity=True, continue_from_best=True)
            == "ds_waterbirds_tl_adapter_reg_seq_bs_128_lr_0.1_lrr0.01_bsr4_balval_GP_MA+ni_cont")


def test_replicas_are_learning_rate_major():
    opt = SimpleNamespace(learning_rate=1.0, learning_rate_reg=2.0, lr_multiple=0.5)
    reps = trainer._sweep_replicas(opt, [7, 8], [0.1, 0.2])
    assert [(o.learning_rate, o.learning_rate_reg, s) for o, s in reps] == [(0.1, 0.05, 7), (0.1, 0.05, 8), (0.2, 0.1, 7), (0.2, 0.1, 8)]
    assert opt.learning_rate == 1.0
    assert [(o is opt, s) for o, s in trainer._sweep_replicas(opt, [7, 8], None)] == [(True, 7), (True, 8)]


def test_sweep_entries_refuse_bad_arguments_without_a_gpu():
    _lib.build()
    L = _lib.lib()
    buf = (ctypes.c_float * 4096)()
    base = ctypes.addressof(buf)
    p = ctypes.c_void_p((base + 15) // 16 * 16)               # a 16-B aligned host address: nothing is launched on these paths
    P9, P6 = (ctypes.c_void_p * 9)(*[p.value] * 9), (ctypes.c_void_p * 6)(*[p.value] * 6)
    lr = (ctypes.c_float * 16)(*[0.1] * 16)

    def step(R=2, B=8, D=512, H=128, C=2, G=4, idx_R=None, idx_B=None, ws_bytes=None, table=p, params=P9, ws=p):
        need = L.dbmm_workspace_bytes_adapter_sweep_step(R, B, D, H, 0)
        return L.dbmm_adapter_sweep_step(table, 100, p, R if idx_R is None else idx_R, B if idx_B is None else idx_B, p, p, params, P6, None, 0.5, p,
                                         0.01, lr, 0.9, 0.0, 1, p, p, p, p, p, G, 1, R, B, D, H, C, ws, need if ws_bytes is None else ws_bytes, None)

    def evaluate(R=2, B=8, D=512, H=128, C=2, G=4, row0=0, ws_bytes=None, ws=p, idx=None):
        need = L.dbmm_workspace_bytes_adapter_sweep_eval(R, B, D, H, 0)
        return L.dbmm_adapter_sweep_eval(p, 100, idx, row0, p, p, P9, None, 0.5, p, 0.01, p, p, p, p, G, R, B, D, H, C, ws,
                                         need if ws_bytes is None else ws_bytes, None)
    SHAPE, ALIGN, WORKSPACE, ARG, UNSUPPORTED = -1, -2, -3, -4, -5
    assert step(R=0) == SHAPE and step(R=17) == SHAPE and evaluate(R=0) == SHAPE and evaluate(R=17) == SHAPE
    assert step(idx_R=3) == SHAPE and step(idx_B=9) == SHAPE                      # idx is not [R, B]
    assert step(B=1) == SHAPE                                                     # train-mode BatchNorm1d over one row
    assert step(C=9) == SHAPE and evaluate(C=0) == SHAPE and step(G=65) == SHAPE
    assert step(D=500) == UNSUPPORTED and step(H=64) == UNSUPPORTED and evaluate(D=192) == UNSUPPORTED      # not the fast shape
    assert step(ws_bytes=L.dbmm_workspace_bytes_adapter_sweep_step(2, 8, 512, 128, 0) - 4) == WORKSPACE
    assert evaluate(ws_bytes=L.dbmm_workspace_bytes_adapter_sweep_eval(2, 8, 512, 128, 0) - 4) == WORKSPACE
    assert evaluate(row0=95) == SHAPE                                             # rows 95 .. 102 of a 100-row table
    off = ctypes.c_void_p(p.value + 4)
    assert step(ws=off) == ALIGN and step(table=off) == ALIGN and evaluate(ws=off) == ALIGN
    assert step(params=(ctypes.c_void_p * 9)(*([p.value] * 8 + [off.value]))) == ALIGN
    assert step(params=None) == ARG and step(table=None) == ARG and evaluate(ws=None) == ARG
    assert L.dbmm_workspace_bytes_adapter_sweep_step(2, 8, 512, 128, 1) > L.dbmm_workspace_bytes_adapter_sweep_step(2, 8, 512, 128, 0) > 0
    assert L.dbmm_workspace_bytes_adapter_sweep_step(4, 8, 512, 128, 0) == 2 * L.dbmm_workspace_bytes_adapter_sweep_step(2, 8, 512, 128, 0)
    assert L.dbmm_workspace_bytes_adapter_sweep_eval(2, 1, 512, 128, 0) > 0 and L.dbmm_workspace_bytes_adapter_sweep_step(2, 1, 512, 128, 0) == 0
