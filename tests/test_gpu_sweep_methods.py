"""The replica-batched linear-probe step and evaluation forward (csrc/linear_sweep.hip, adapter.SweepLinear) and the lock-step
`linear_probing` / `adapter_reg` schedules of trainer.train_sweep on the MI355X.

  * step == single step: replica r of one batched call equals, bit for bit, LinearClassifier.train_step run for r alone on
    table.batch(idx[r]) -- logits, per-row CE, loss, fc.weight, fc.bias, both momentum buffers -- over three consecutive steps with
    distinct per-replica rows (with repeats) and learning rates, on both sides of the one-launch switch and of the slab caps; the
    in-step group counters equal adapter.group_counts and the float64 loss sums equal the trainer's accumulation exactly.  Same for
    the evaluation entry against LinearClassifier.loss, with an index list and with row0.
  * guard zones around every stacked tensor, output and the workspace; a repeat of a call gives identical bits.
  * sweep == sequential: train_sweep against set_seed(s); train_all_epochs(...) per replica, records included.
  * the batched path is taken: with the single-run step / loss methods patched to raise, the sweeps still complete.
  * against the reference's own sweep driver (tests/golden/sweep_wb_{linear_probing,adapter_reg}.npz,
    tools/make_golden_sweep_methods.py): passes, best epochs and the result table."""
import ctypes
import json
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from dbmm_amd import _lib, adapter, ops, optim, synth, trainer

pytestmark = pytest.mark.gpu
G, N_ROWS = 4, 1500
GUARD = 2048


@pytest.fixture(scope="module")
def table_by_dim():
    cache = {}

    def get(D, n=N_ROWS):
        if (D, n) not in cache:
            g = torch.Generator().manual_seed(17 + D + n)
            x = torch.randn(n, D, generator=g) * 0.5
            y = torch.randint(0, 2, (n,), generator=g)
            c = torch.randint(0, 2, (n,), generator=g)
            t = trainer.EmbeddingTable(x.numpy(), y.numpy(), c.numpy(), device="cuda")
            t.labels8 = (t.targets_group * 2 + torch.randint(0, 2, (n,), generator=g).cuda()).contiguous()
            cache[(D, n)] = t
        return cache[(D, n)]
    return get


def _labels(table, C):
    return {2: table.targets, 4: table.targets_group, 8: table.labels8}[C]


def _modules(R, D, C, seed=100):
    mods = []
    for r in range(R):
        torch.manual_seed(seed + r)
        mods.append(adapter.LinearClassifier(D, C).cuda().train())
    return mods


def _idx(R, B, step, seed=5):
    g = torch.Generator().manual_seed(seed * 7919 + 31 * step + B)
    idx = torch.randint(0, N_ROWS, (R, B), generator=g)
    if B > 1:
        idx[:, 1] = idx[:, 0]                                # a repeated row within every replica
    if R > 1 and B > 2:
        idx[1, 2] = idx[0, 2]                                # and one shared by two replicas
    return idx.cuda()


@pytest.mark.parametrize("C", [2, 4, 8])
@pytest.mark.parametrize("D", [512, 768, 1024, 20])
@pytest.mark.parametrize("B", [1, 4, 37, 256, 512, 513, 1025, 4100])
@pytest.mark.parametrize("R", [1, 3, 8, 16])
def test_step_equals_single_step(R, B, D, C, table_by_dim):
    table = table_by_dim(D)
    labels_tab = _labels(table, C)
    mods = _modules(R, D, C)
    sweep = adapter.SweepLinear.from_modules(mods, "cuda")
    lrs = [0.05 + 0.01 * r for r in range(R)]
    opts = [optim.SGD(m.parameters(), lr=lrs[r], momentum=0.9, weight_decay=5e-5) for r, m in enumerate(mods)]
    counts = torch.zeros((R, G, 2), dtype=torch.int64, device="cuda")
    loss_sum = torch.zeros((R,), dtype=torch.float64, device="cuda")
    ref_counts = torch.zeros((R, G, 2), dtype=torch.int64, device="cuda")
    ref_sum = [torch.zeros((), dtype=torch.float64, device="cuda") for _ in range(R)]
    for step in range(3):
        idx = _idx(R, B, step)
        counted = step != 1                                   # the middle step is an uncounted pass: metrics must not move
        loss, logits, rows = sweep.step(table.embeddings, idx, labels_tab, table.targets_group, lrs, 0.9, 5e-5, counts, loss_sum, counted=counted)
        assert logits.shape == (R, B, C) and rows.shape == (R, B) and loss.shape == (R,)
        for r, m in enumerate(mods):
            emb, _, grp = table.batch(idx[r])
            lab = labels_tab[idx[r]]
            l1, lg1, rw1 = m.train_step(emb, lab, opts[r])
            assert torch.equal(logits[r], lg1), (step, r, "logits")
            assert torch.equal(rows[r], rw1), (step, r, "loss_rows")
            assert torch.equal(loss[r], l1), (step, r, "loss")
            if counted:
                ref_sum[r] += l1.double() * idx[r].numel()
                adapter.group_counts(lg1, lab, grp, G, ref_counts[r])
            assert torch.equal(sweep.w[r], m.fc.weight.detach()), (step, r, "fc.weight")
            assert torch.equal(sweep.b[r], m.fc.bias.detach()), (step, r, "fc.bias")
            assert torch.equal(sweep.mom_w[r], opts[r].state[m.fc.weight]["momentum_buffer"]), (step, r, "momentum of fc.weight")
            assert torch.equal(sweep.mom_b[r], opts[r].state[m.fc.bias]["momentum_buffer"]), (step, r, "momentum of fc.bias")
        assert torch.equal(counts, ref_counts), step
        assert torch.equal(loss_sum, torch.stack(ref_sum)), step


@pytest.mark.parametrize("C", [2, 4, 8])
@pytest.mark.parametrize("D", [512, 768, 1024, 20])
@pytest.mark.parametrize("B", [1, 4, 37, 256, 512, 513, 1025, 4100])
@pytest.mark.parametrize("R", [1, 3, 8, 16])
def test_eval_equals_single_loss(R, B, D, C, table_by_dim):
    table = table_by_dim(D)
    labels_tab = _labels(table, C)
    mods = _modules(R, D, C, seed=300)
    for m in mods:
        m.eval()
    sweep = adapter.SweepLinear.from_modules(mods, "cuda")
    big = table_by_dim(D, 4200) if B > N_ROWS - 77 else table           # row0 .. row0 + B - 1 must fit: 4100 rows need a longer table
    for table, idx, r0, n in ((table, _idx(1, B, 3)[0].contiguous(), 0, B), (big, None, 77, B)):
        labels_tab = _labels(table, C)
        counts = torch.zeros((R, G, 2), dtype=torch.int64, device="cuda")
        loss_sum = torch.zeros((R,), dtype=torch.float64, device="cuda")
        logits, rows = sweep.evaluate(table.embeddings, idx, labels_tab, table.targets_group, counts, loss_sum, row0=r0, n=n)
        rows_idx = idx if idx is not None else torch.arange(r0, r0 + n, device="cuda")
        emb = ops.gather_rows(table.embeddings, rows_idx)
        lab, grp = labels_tab[rows_idx], table.targets_group[rows_idx]
        for r, m in enumerate(mods):
            _, lg1, rw1 = m.loss(emb, lab)
            assert torch.equal(logits[r], lg1), (r, "logits")
            assert torch.equal(rows[r], rw1), (r, "loss_rows")
            assert torch.equal(counts[r], adapter.group_counts(lg1, lab, grp, G)), r
            ref = rw1.double().sum().item()
            assert abs(loss_sum[r].item() - ref) <= 1e-12 * max(1.0, abs(ref)), r      # float64 sums of the same terms, another order
        c2, s2 = torch.zeros_like(counts), torch.zeros_like(loss_sum)
        l2, r2 = sweep.evaluate(table.embeddings, idx, labels_tab, table.targets_group, c2, s2, row0=r0, n=n)
        assert torch.equal(l2, logits) and torch.equal(r2, rows) and torch.equal(c2, counts) and torch.equal(s2, loss_sum), "repeat differs"


def _guarded(n, dtype=torch.float32, fill=7):
    buf = torch.full((n + 2 * GUARD,), fill, device="cuda", dtype=dtype)
    return buf, buf[GUARD:GUARD + n]


def _guards_intact(buf, n, fill=7):
    return bool((buf[:GUARD] == fill).all() and (buf[GUARD + n:] == fill).all())


@pytest.mark.parametrize("R,B,D,C", [(3, 37, 512, 4), (16, 4, 768, 2), (8, 1025, 1024, 8), (2, 512, 1024, 2), (16, 4100, 20, 8), (5, 1, 512, 2)])
def test_guard_zones_and_repeat(R, B, D, C, table_by_dim):
    """every stacked tensor, every output and the workspace sit between guard zones; the call is run twice from the same state"""
    table = table_by_dim(D)
    labels_tab = _labels(table, C)
    src = adapter.SweepLinear.from_modules(_modules(R, D, C, seed=500), "cuda")
    L = _lib.lib()
    idx = _idx(R, B, 1)
    lrs = (ctypes.c_float * R)(*[0.05 + 0.01 * r for r in range(R)])
    results = []
    for rep in range(2):
        held = []

        def place(t, n=None, dtype=torch.float32, fill=7):
            buf, v = _guarded(t.numel() if t is not None else n, dtype, fill)
            if t is not None:
                v.copy_(t.flatten())
            elif fill == 0:
                v.zero_()
            held.append((buf, v.numel(), fill))
            return v
        w, b = place(src.w), place(src.b)
        mw, mb = place(torch.zeros_like(src.w)), place(torch.zeros_like(src.b))
        logits, rows, mean = place(None, R * B * C), place(None, R * B), place(None, R)
        counts, loss_sum = place(None, R * G * 2, torch.int64, 0), place(None, R, torch.float64, 0)
        nbytes = L.dbmm_workspace_bytes_linear_sweep_step(R, B, D, C)
        assert nbytes > 0 and nbytes % 16 == 0
        ws = place(None, nbytes // 4)
        rc = L.dbmm_linear_sweep_step(table.embeddings.data_ptr(), N_ROWS, idx.data_ptr(), R, B, labels_tab.data_ptr(), table.targets_group.data_ptr(),
                                      w.data_ptr(), b.data_ptr(), mw.data_ptr(), mb.data_ptr(), lrs, 0.9, 5e-5, 1, logits.data_ptr(), rows.data_ptr(),
                                      mean.data_ptr(), counts.data_ptr(), loss_sum.data_ptr(), G, 1, R, B, D, C, ws.data_ptr(), nbytes, ops.stream())
        assert rc == 0, rc
        torch.cuda.synchronize()
        for buf, n, fill in held:
            assert _guards_intact(buf, n, fill), "a guard zone was written"
        assert int(counts.view(R, G, 2)[:, :, 0].sum()) == R * B
        results.append([t.clone() for t in (w, b, mw, mb, logits, rows, mean, counts, loss_sum)])
        # the evaluation entry on the same guarded stacks
        nb = L.dbmm_workspace_bytes_linear_sweep_eval(R, B)
        assert nb > 0 and nb % 16 == 0
        ews, lg, rw = place(None, nb // 4), place(None, R * B * C), place(None, R * B)
        cn, sm = place(None, R * G * 2, torch.int64, 0), place(None, R, torch.float64, 0)
        rc = L.dbmm_linear_sweep_eval(table.embeddings.data_ptr(), N_ROWS, idx[0].contiguous().data_ptr(), 0, labels_tab.data_ptr(),
                                      table.targets_group.data_ptr(), w.data_ptr(), b.data_ptr(), lg.data_ptr(), rw.data_ptr(), cn.data_ptr(),
                                      sm.data_ptr(), G, R, B, D, C, ews.data_ptr(), nb, ops.stream())
        assert rc == 0, rc
        torch.cuda.synchronize()
        for buf, n, fill in held:
            assert _guards_intact(buf, n, fill), "a guard zone was written (eval)"
        assert int(cn.view(R, G, 2)[:, :, 0].sum()) == R * B
        results[-1] += [lg.clone(), rw.clone(), cn.clone(), sm.clone()]
    for a, b in zip(*results):
        assert torch.equal(a, b), "two runs from the same state differ"


def test_wrapper_shape_checks(table_by_dim):
    table = table_by_dim(512)
    sweep = adapter.SweepLinear.from_modules(_modules(2, 512, 2), "cuda")
    counts = torch.zeros((2, G, 2), dtype=torch.int64, device="cuda")
    loss_sum = torch.zeros((2,), dtype=torch.float64, device="cuda")
    with pytest.raises(_lib.DbmmError):                       # three index rows for two replicas
        sweep.step(table.embeddings, _idx(3, 8, 0), table.targets, table.targets_group, [0.1, 0.1], 0.9, 0.0, counts, loss_sum)
    with pytest.raises(_lib.DbmmError):                       # one learning rate short
        sweep.step(table.embeddings, _idx(2, 8, 0), table.targets, table.targets_group, [0.1], 0.9, 0.0, counts, loss_sum)
    with pytest.raises(RuntimeError):                         # labels of another table
        sweep.step(table.embeddings, _idx(2, 8, 0), table.targets[:100].contiguous(), table.targets_group, [0.1, 0.1], 0.9, 0.0, counts, loss_sum)
    with pytest.raises(_lib.DbmmError):                       # counters of another replica count
        sweep.step(table.embeddings, _idx(2, 8, 0), table.targets, table.targets_group, [0.1, 0.1], 0.9, 0.0, counts[:1].contiguous(), loss_sum)
    with pytest.raises(_lib.DbmmError):                       # a table of another width
        sweep.evaluate(table_by_dim(768).embeddings, None, table.targets, table.targets_group, counts, loss_sum)
    with pytest.raises(_lib.DbmmError):                       # rows 1495 .. 1502 of a 1500-row table
        sweep.evaluate(table.embeddings, None, table.targets, table.targets_group, counts, loss_sum, row0=N_ROWS - 5, n=8)


def test_replica_is_an_ordinary_module_and_leaves_the_random_stream_alone(table_by_dim):
    mods = _modules(3, 512, 2)
    sweep = adapter.SweepLinear.from_modules(mods, "cuda")
    assert sweep.replica(1, best=True) is None
    sweep.snapshot([False, True, False])
    torch.manual_seed(9)
    before = torch.get_rng_state()
    m = sweep.replica(1, best=True)
    assert torch.equal(torch.get_rng_state(), before)
    assert isinstance(m, adapter.LinearClassifier) and not m.training and list(m.state_dict()) == ["fc.weight", "fc.bias"]
    assert torch.equal(m.fc.weight.detach(), mods[1].fc.weight.detach()) and torch.equal(m.fc.bias.detach(), mods[1].fc.bias.detach())
    assert sweep.replica(0, best=True) is None and sweep.replica(0) is not None


# ---- the sweep driver --------------------------------------------------------------------------------------------------------

CFG = dict(seed=3, dim=512, n_train=1000, n_val=600, n_test=700)
SEEDS = (0, 1, 2)


def _opt(d, **kw):
    tcls, tspu, tgrp = synth.embedding_text(CFG["seed"], CFG["dim"])
    o = dict(tl_method="linear_probing", dataset="waterbirds", epochs=5, epochs_feature_learning=3, batch_size=256, batch_size_reg=64,
             learning_rate=0.05, learning_rate_reg=0.02, lr_multiple=0.5, momentum=0.9, weight_decay=5e-5, cosine=False, lr_decay_epochs=[4],
             lr_decay_rate=0.5, warm=False, warm_reg=False, adapter_feat_dim=128, zs_temperature=0.01, train_target="class", balance_val=False,
             add_adapter=False, continue_from_best=False, init_near_identity=False, use_cls_prompt_in_reg=False, resample_ce=False, n_cls=2)
    o.update(kw)
    for key, m, cols in (("text_embedding_dir", tcls, ["c0", "c1"]), ("text_spurious_embedding_dir", tspu, ["s0", "s1"]),
                         ("text_group_embedding_dir", tgrp, ["g0", "g1", "g2", "g3"])):
        o[key] = os.path.join(d, key + ".json")
        if not os.path.exists(o[key]):
            json.dump({n: m[:, i].numpy().tolist() for i, n in enumerate(cols)}, open(o[key], "w"))
    return SimpleNamespace(**o)


@pytest.fixture(scope="module")
def tables():
    out = []
    for split, n in (("train", CFG["n_train"]), ("val", CFG["n_val"]), ("test", CFG["n_test"])):
        x, y, c = synth.embedding_dataset(CFG["seed"], split, n, CFG["dim"])
        out.append(trainer.EmbeddingTable(x.numpy(), y.numpy(), c.numpy(), device="cuda"))
    return out


def _sequential(opt, tables, seeds, learning_rates=None):
    out, logs = [], []
    for o, s in trainer._sweep_replicas(opt, list(seeds), learning_rates):
        optim.set_seed(s)
        lg = []
        out.append(trainer.train_all_epochs(o, *tables, log=lg))
        logs.append(lg)
    return out, logs


def _assert_same_runs(got, glog, want, wlog):
    assert len(got) == len(want) == len(glog) == len(wlog)
    for r in range(len(want)):
        assert got[r] == want[r], (r, "returned dicts")
        assert [e["kind"] for e in glog[r]] == [e["kind"] for e in wlog[r]], r
        for a, b in zip(glog[r], wlog[r]):
            assert set(a) == set(b), (r, a["kind"], "fields of the record")
            if a["kind"] == "init":
                assert list(a["state"]) == list(b["state"]) and all(torch.equal(a["state"][k], b["state"][k]) for k in b["state"]), (r, "init")
            elif a["kind"] == "final":
                assert a["best_epoch"] == b["best_epoch"], (r, "best epoch")
                assert type(a["best_model"]) is type(b["best_model"]), (r, "kind of the best model")
                if b["best_model"] is None:                   # worst-group accuracy never above 0: no best model in either run
                    continue
                assert a["best_model"].training == b["best_model"].training
                sa, sb = a["best_model"].state_dict(), b["best_model"].state_dict()
                assert list(sa) == list(sb), (r, "state-dict keys")
                for k in sb:
                    assert torch.equal(sa[k], sb[k]), (r, k)
            else:
                assert np.array_equal(a["counts"], b["counts"]), (r, a["kind"], a.get("epoch"))
                assert a["group_acc"] == b["group_acc"] and a["acc"] == b["acc"], (r, a["kind"], a.get("epoch"))
                assert abs(a["loss"] - b["loss"]) <= 1e-12 * max(1.0, abs(b["loss"])), (r, a["kind"], a.get("epoch"), a["loss"], b["loss"])
                for k in ("epoch", "split", "target", "use_group", "n_train_rows"):
                    assert a.get(k) == b.get(k), (r, a["kind"], k)
                if "order" in b:
                    assert np.array_equal(a["order"], b["order"]), (r, a["kind"], a.get("epoch"))


WARM = dict(warm=True, warm_epochs=2, warmup_from=0.01, warmup_to=0.05)
SCHEDULES = {
    "linear_probing": dict(tl_method="linear_probing"),
    "linear_probing_warm_small_batches": dict(tl_method="linear_probing", batch_size=37, **WARM),
    "linear_probing_two_launch_batches": dict(tl_method="linear_probing", batch_size=600),
    "adapter_reg_gp_balval": dict(tl_method="adapter_reg", balance_val=True),
    "adapter_reg_cls_prompt": dict(tl_method="adapter_reg", use_cls_prompt_in_reg=True),
    "adapter_reg_warm": dict(tl_method="adapter_reg", balance_val=True, **WARM),
}


@pytest.mark.parametrize("name", list(SCHEDULES))
@pytest.mark.parametrize("grid", ["seeds", "lr_x_seeds"])
def test_sweep_equals_sequential(name, grid, tables, tmp_path_factory):
    opt = _opt(str(tmp_path_factory.mktemp("sweep")), **SCHEDULES[name])
    seeds, lrs = (SEEDS, None) if grid == "seeds" else (SEEDS[:2], [0.05, 0.02])
    want, wlog = _sequential(opt, tables, seeds, lrs)
    glog = []
    got = trainer.train_sweep(opt, *tables, seeds, learning_rates=lrs, log=glog)
    _assert_same_runs(got, glog, want, wlog)


def test_more_than_sixteen_linear_probes_are_split_into_groups(tables, tmp_path_factory):
    """18 seeds: one group of 16 replicas and one of 2, results in seed order"""
    opt = _opt(str(tmp_path_factory.mktemp("sweep")), tl_method="linear_probing", epochs=3)
    seeds = list(range(18))
    want, wlog = _sequential(opt, tables, seeds)
    glog = []
    got = trainer.train_sweep(opt, *tables, seeds, log=glog)
    _assert_same_runs(got, glog, want, wlog)


def _raiser(name):
    def f(*a, **k):
        raise AssertionError(f"{name} was called: the sweep went replica by replica")
    return f


def test_linear_probing_sweep_does_not_go_through_the_single_run_step(tables, tmp_path_factory, monkeypatch):
    opt = _opt(str(tmp_path_factory.mktemp("sweep")), tl_method="linear_probing", epochs=3)
    want, _ = _sequential(opt, tables, SEEDS)
    monkeypatch.setattr(adapter.LinearClassifier, "train_step", _raiser("LinearClassifier.train_step"))
    monkeypatch.setattr(adapter.LinearClassifier, "loss", _raiser("LinearClassifier.loss"))
    assert trainer.train_sweep(opt, *tables, SEEDS) == want


def test_adapter_reg_sweep_does_not_go_through_the_single_run_step(tables, tmp_path_factory, monkeypatch):
    opt = _opt(str(tmp_path_factory.mktemp("sweep")), tl_method="adapter_reg", epochs=3, balance_val=True)
    want, _ = _sequential(opt, tables, SEEDS)
    monkeypatch.setattr(adapter.CustomCLIP, "train_step", _raiser("CustomCLIP.train_step"))
    monkeypatch.setattr(adapter.CustomCLIP, "loss", _raiser("CustomCLIP.loss"))
    assert trainer.train_sweep(opt, *tables, SEEDS) == want


def test_ineligible_shapes_keep_the_sequential_path(tables, tmp_path_factory):
    """a single replica runs through train_all_epochs as before"""
    opt = _opt(str(tmp_path_factory.mktemp("sweep")), tl_method="linear_probing", epochs=2)
    want, wlog = _sequential(opt, tables, SEEDS[:1])
    glog = []
    got = trainer.train_sweep(opt, *tables, SEEDS[:1], log=glog)
    _assert_same_runs(got, glog, want, wlog)


# ---- against the reference's own sweep driver (tests/golden/sweep_wb_<method>.npz, tools/make_golden_sweep_methods.py) --------

@pytest.fixture(scope="module", params=["linear_probing", "adapter_reg"])
def wb_run(request, tmp_path_factory):
    from conftest import GOLDEN
    g = np.load(os.path.join(GOLDEN, f"sweep_wb_{request.param}.npz"), allow_pickle=False)
    cfg, o = json.loads(str(g["config"])), json.loads(str(g["opt"]))
    d = tmp_path_factory.mktemp("sweep_wb")
    tcls, tspu, tgrp = synth.embedding_text(cfg["seed"], cfg["dim"])
    for key, m, cols in (("text_embedding_dir", tcls, ["c0", "c1"]), ("text_spurious_embedding_dir", tspu, ["s0", "s1"]),
                         ("text_group_embedding_dir", tgrp, ["g0", "g1", "g2", "g3"])):
        o[key] = os.path.join(d, key + ".json")
        json.dump({n: m[:, i].numpy().tolist() for i, n in enumerate(cols)}, open(o[key], "w"))
    opt = SimpleNamespace(**o)
    tabs = []
    for split, n in (("train", cfg["n_train"]), ("val", cfg["n_val"]), ("test", cfg["n_test"])):
        x, y, c = synth.embedding_dataset(cfg["seed"], split, n, cfg["dim"])
        tabs.append(trainer.EmbeddingTable(x.numpy(), y.numpy(), c.numpy(), device="cuda"))
    log = []
    results = trainer.train_sweep(opt, *tabs, [int(s) for s in g["seeds"]], log=log)
    return g, opt, log, results


def test_sweep_passes_against_the_references_driver(wb_run):
    """per pass and seed: row orders equal; (n) counters equal, `correct` counters within the fixture's own 1-ulp / 8-ulp sensitivity
    + 1; losses within 2e-3 max(1, |loss|) + 4 x the reference's own perturbation distance; best epoch per seed equal (the bounds of
    test_gpu_sweep.py::test_sweep_passes_against_the_references_driver)"""
    g, opt, log, _ = wb_run
    assert len(log) == int(g["n_seeds"])
    for s, lg in enumerate(log):
        passes = [e for e in lg if e["kind"] in ("train1", "train_reg", "validate", "validate_zs")]
        assert len(passes) == int(g[f"s{s}/n_phases"])
        flips = 0
        for i, e in enumerate(passes):
            k = f"s{s}/p{i}/"
            assert e["kind"] == str(g[k + "kind"]), (s, i)
            if e["kind"] in ("train1", "train_reg"):
                assert np.array_equal(e["order"], g[k + "idx"].astype(np.int64)), (s, i)
            if e["kind"] == "train_reg":
                assert e["use_group"] == bool(g[k + "use_group"]) and e["n_train_rows"] == int(g[k + "n_train"]), (s, i)
            ref = g[k + "counts"]
            assert np.array_equal(e["counts"][:, 0], ref[:, 0]), (s, i)
            sens = np.maximum(np.abs(g[k + "counts_1ulp"] - ref), np.abs(g[k + "counts_8ulp"] - ref))[:, 1]
            dcnt = np.abs(e["counts"][:, 1] - ref[:, 1])
            flips += int(dcnt.sum())
            lref = float(g[k + "loss"])
            ltol = 2e-3 * max(1.0, abs(lref)) + 4 * max(abs(float(g[k + "loss_1ulp"]) - lref), abs(float(g[k + "loss_8ulp"]) - lref))
            print(f"seed {s} p{i:02d} {e['kind']:11s} correct {e['counts'][:, 1].tolist()} ref {ref[:, 1].tolist()} sens {sens.tolist()} "
                  f"loss {e['loss']:.6f} ref {lref:.6f} tol {ltol:.2e}")
            assert (dcnt <= sens + 1).all(), (s, i, e["kind"], e["counts"][:, 1].tolist(), ref[:, 1].tolist())
            assert abs(e["loss"] - lref) <= ltol, (s, i, e["kind"], e["loss"], lref)
        best = [e for e in lg if e["kind"] == "final"][0]["best_epoch"]
        print(f"seed {s}: {flips} flipped predictions, best epoch {best} (reference {int(g[f's{s}/best_epoch'])})")
        assert best == int(g[f"s{s}/best_epoch"]), s


def test_sweep_table_against_the_references_driver(wb_run):
    """every *_mean row of sweep_frame within 0.002 of the reference's table (the project's +-0.2 pp criterion).  *_std rows: the
    sample std is the norm of the centred values over sqrt(n - 1), so moving each of n values by at most eps moves it by at most
    eps sqrt(n / (n - 1)); n = 3, eps = 0.002: 0.00245, plus 1e-4 for the two round(4)"""
    g, opt, _, results = wb_run
    frame = trainer.sweep_frame(results)
    index = [str(i) for i in g["table/index"]]
    assert [str(i) for i in frame.index] == index and [str(c) for c in frame.columns] == [str(c) for c in g["table/columns"]]
    assert trainer.sweep_result_name(opt) == str(g["table/name"])
    got, ref = frame.to_numpy(dtype=np.float64), g["table/values"]
    assert np.array_equal(np.isnan(got), np.isnan(ref))
    for i, name in enumerate(index):
        if name.endswith("_mean") or name.endswith("_std"):
            d = np.nanmax(np.abs(got[i] - ref[i]))
            bound = 0.002 + 1e-9 if name.endswith("_mean") else 0.002 * np.sqrt(3 / 2) + 1e-4
            print(f"{name:12s} max |diff| {d:.5f} (bound {bound:.5f})")
            assert d <= bound, (name, got[i].tolist(), ref[i].tolist())
