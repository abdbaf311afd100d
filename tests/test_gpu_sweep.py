"""The replica-batched adapter step and evaluation forward (csrc/adapter_sweep.hip, adapter.SweepAdapters) and the sweep driver
(trainer.train_sweep) on the MI355X.

  * step == single step: replica r of one batched call equals, bit for bit, classifier.train_step run for r alone on
    table.batch(idx[r]) -- logits, per-row CE, loss, parameters, momentum buffers, running statistics, num_batches_tracked -- over
    three consecutive steps with distinct per-replica rows (with repeats) and learning rates; the in-step group counters equal
    adapter.group_counts and the float64 loss sums equal the trainer's accumulation exactly.  Same for the evaluation entry against
    classifier.loss.
  * guard zones around every stacked tensor, output and the workspace; a repeat of a call gives identical bits.
  * sweep == sequential: train_sweep against set_seed(s); train_all_epochs(...) per replica.
  * the fallback methods through train_sweep return what the sequential loop returns."""
import copy
import ctypes
import json
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from dbmm_amd import _lib, adapter, ops, optim, synth, trainer

pytestmark = pytest.mark.gpu
H, G, N_ROWS = 128, 4, 1500
GUARD = 2048


def _text_paths(tmp_path_factory, D):
    d = tmp_path_factory.mktemp(f"text{D}")
    paths = []
    for name, kind, cols in (("class", "class", ["c0", "c1"]), ("spurious", "spurious", ["s0", "s1"]), ("group", "group", ["g0", "g1", "g2", "g3"])):
        m = synth.text_matrix(1, D, len(cols), kind)
        p = os.path.join(d, name + ".json")
        json.dump({n: m[:, i].numpy().tolist() for i, n in enumerate(cols)}, open(p, "w"))
        paths.append(p)
    return paths


@pytest.fixture(scope="module")
def text_paths_by_dim(tmp_path_factory):
    cache = {}

    def get(D):
        if D not in cache:
            cache[D] = _text_paths(tmp_path_factory, D)
        return cache[D]
    return get


@pytest.fixture(scope="module")
def table_by_dim():
    cache = {}

    def get(D):
        if D not in cache:
            g = torch.Generator().manual_seed(11 + D)
            x = torch.randn(N_ROWS, D, generator=g) * 0.5
            y = torch.randint(0, 2, (N_ROWS,), generator=g)
            c = torch.randint(0, 2, (N_ROWS,), generator=g)
            cache[D] = trainer.EmbeddingTable(x.numpy(), y.numpy(), c.numpy(), device="cuda")
        return cache[D]
    return get


def _modules(R, D, paths, with_old, seed=100):
    mods = []
    for r in range(R):
        torch.manual_seed(seed + r)
        m = adapter.CustomCLIP(adapter.Adapter(D, H), *paths)
        if with_old:
            m = adapter.MultipleAdapter(m, adapter.Adapter(D, H), init_near_identity=False, ebd_weight=0.5)
        mods.append(m.cuda().train())
    return mods


def _trainable(m):
    return m.new_adapter if isinstance(m, adapter.MultipleAdapter) else m.adapter


def _idx(R, B, step, seed=5):
    g = torch.Generator().manual_seed(seed * 7919 + 31 * step + B)
    idx = torch.randint(0, N_ROWS, (R, B), generator=g)
    idx[:, 1] = idx[:, 0]                                    # a repeated row within every replica
    if R > 1:
        idx[1, 2] = idx[0, 2]                                # and one shared by two replicas
    return idx.cuda()


def _assert_stack_equals_modules(sweep, mods, opts=None):
    for r, m in enumerate(mods):
        for name, got, want in zip(("w1", "b1", "gamma", "beta", "running_mean", "running_var", "nbt", "w2", "b2"), sweep.new,
                                   adapter._adapter_tensors(_trainable(m))):
            assert torch.equal(got[r], want.detach()), (r, name)
        if sweep.old is not None:
            for name, got, want in zip(("w1", "b1", "gamma", "beta", "running_mean", "running_var", "nbt", "w2", "b2"), sweep.old,
                                       adapter._adapter_tensors(m.old_cls.adapter)):
                assert torch.equal(got[r], want.detach()), (r, "old." + name)
        if opts is not None:
            ts = adapter._adapter_tensors(_trainable(m))
            for k, i in enumerate(adapter._TRAINABLE):
                assert torch.equal(sweep.mom[k][r], opts[r].state[ts[i]]["momentum_buffer"]), (r, "momentum", i)


@pytest.mark.parametrize("with_old", [False, True])
@pytest.mark.parametrize("C", [2, 4])
@pytest.mark.parametrize("D", [512, 768, 1024])
@pytest.mark.parametrize("B", [4, 37, 256, 1025])
@pytest.mark.parametrize("R", [1, 3, 8, 16])
def test_step_equals_single_step(R, B, D, C, with_old, text_paths_by_dim, table_by_dim):
    table = table_by_dim(D)
    mods = _modules(R, D, text_paths_by_dim(D), with_old)
    sweep = adapter.SweepAdapters.from_modules(copy.deepcopy(mods), "cuda")
    lrs = [0.05 + 0.01 * r for r in range(R)]
    opts = [optim.SGD([p for n, p in m.named_parameters() if "old_cls" not in n], lr=lrs[r], momentum=0.9, weight_decay=5e-5)
            for r, m in enumerate(mods)]
    use_group = C == 4
    which = "group" if use_group else "class"
    labels_tab = table.targets_group if use_group else table.targets
    counts = torch.zeros((R, G, 2), dtype=torch.int64, device="cuda")
    loss_sum = torch.zeros((R,), dtype=torch.float64, device="cuda")
    ref_counts = torch.zeros((R, G, 2), dtype=torch.int64, device="cuda")
    ref_sum = [torch.zeros((), dtype=torch.float64, device="cuda") for _ in range(R)]
    for step in range(3):
        idx = _idx(R, B, step)
        counted = step != 1                                   # the middle step is an uncounted pass: metrics must not move
        loss, logits, rows = sweep.step(table.embeddings, idx, labels_tab, table.targets_group, which, lrs, 0.9, 5e-5, counts, loss_sum,
                                        counted=counted)
        assert logits.shape == (R, B, C) and rows.shape == (R, B) and loss.shape == (R,)
        for r, m in enumerate(mods):
            emb, lab, grp = table.batch(idx[r])
            if use_group:
                lab = grp
            l1, lg1, rw1 = m.train_step(emb, lab, opts[r], use_group)
            assert torch.equal(logits[r], lg1), (step, r, "logits")
            assert torch.equal(rows[r], rw1), (step, r, "loss_rows")
            assert torch.equal(loss[r], l1), (step, r, "loss")
            if counted:
                ref_sum[r] += l1.double() * idx[r].numel()
                adapter.group_counts(lg1, lab, grp, G, ref_counts[r])
        _assert_stack_equals_modules(sweep, mods, opts)
        assert torch.equal(counts, ref_counts), step
        assert torch.equal(loss_sum, torch.stack(ref_sum)), step


@pytest.mark.parametrize("with_old", [False, True])
@pytest.mark.parametrize("which", ["class", "group", "spurious"])
@pytest.mark.parametrize("D", [512, 1024])
@pytest.mark.parametrize("B,R", [(4, 3), (37, 16), (1025, 8), (256, 1)])
def test_eval_equals_single_loss(B, R, D, which, with_old, text_paths_by_dim, table_by_dim):
    table = table_by_dim(D)
    mods = _modules(R, D, text_paths_by_dim(D), with_old, seed=300)
    # running statistics that are not the initial ones: one training step each
    opts = [optim.SGD([p for n, p in m.named_parameters() if "old_cls" not in n], lr=0.1, momentum=0.9, weight_decay=5e-5) for m in mods]
    for r, m in enumerate(mods):
        emb, lab, _ = table.batch(_idx(R, 64, 9)[r])
        m.train_step(emb, lab, opts[r])
        m.eval()
    sweep = adapter.SweepAdapters.from_modules(mods, "cuda")
    labels_tab = {"class": table.targets, "group": table.targets_group, "spurious": table.targets_spurious}[which]
    for idx, row0 in ((_idx(1, B, 3)[0].contiguous(), 0), (None, 77)):
        counts = torch.zeros((R, G, 2), dtype=torch.int64, device="cuda")
        loss_sum = torch.zeros((R,), dtype=torch.float64, device="cuda")
        logits, rows = sweep.evaluate(table.embeddings, idx, labels_tab, table.targets_group, which, counts, loss_sum, row0=row0, n=B)
        rows_idx = idx if idx is not None else torch.arange(row0, row0 + B, device="cuda")
        emb = ops.gather_rows(table.embeddings, rows_idx)
        lab, grp = labels_tab[rows_idx], table.targets_group[rows_idx]
        for r, m in enumerate(mods):
            with torch.no_grad():
                _, lg1, rw1 = m.loss(emb, lab, use_group=which == "group", spurious=which == "spurious")
            assert torch.equal(logits[r], lg1), (r, "logits")
            assert torch.equal(rows[r], rw1), (r, "loss_rows")
            assert torch.equal(counts[r], adapter.group_counts(lg1, lab, grp, G)), r
            ref = rw1.double().sum().item()
            assert abs(loss_sum[r].item() - ref) <= 1e-12 * max(1.0, abs(ref)), r      # float64 sums of the same terms, another order
        c2, s2 = torch.zeros_like(counts), torch.zeros_like(loss_sum)
        l2, r2 = sweep.evaluate(table.embeddings, idx, labels_tab, table.targets_group, which, c2, s2, row0=row0, n=B)
        assert torch.equal(l2, logits) and torch.equal(r2, rows) and torch.equal(c2, counts) and torch.equal(s2, loss_sum), "repeat differs"


def _guarded(n, dtype=torch.float32, fill=7):
    buf = torch.full((n + 2 * GUARD,), fill, device="cuda", dtype=dtype)
    return buf, buf[GUARD:GUARD + n]


def _guards_intact(buf, n, fill=7):
    return bool((buf[:GUARD] == fill).all() and (buf[GUARD + n:] == fill).all())


@pytest.mark.parametrize("with_old", [False, True])
@pytest.mark.parametrize("R,B,D,C", [(3, 37, 512, 4), (16, 4, 768, 2), (8, 1025, 1024, 2), (2, 256, 1024, 4)])
def test_guard_zones_and_repeat(R, B, D, C, with_old, text_paths_by_dim, table_by_dim):
    """every stacked tensor, every output and the workspace sit between guard zones; the call is run twice from the same state"""
    table = table_by_dim(D)
    mods = _modules(R, D, text_paths_by_dim(D), with_old, seed=500)
    src = adapter.SweepAdapters.from_modules(mods, "cuda")
    L = _lib.lib()
    tn = src.text("group" if C == 4 else "class")
    labels_tab = table.targets_group if C == 4 else table.targets
    idx = _idx(R, B, 1)
    lrs = (ctypes.c_float * R)(*[0.05 + 0.01 * r for r in range(R)])
    results = []
    for rep in range(2):
        held = []

        def place(t):
            fill = 7 if t.dtype == torch.float32 else 123456789
            buf, v = _guarded(t.numel(), t.dtype, fill)
            v.copy_(t.flatten())
            held.append((buf, t.numel(), fill))
            return v.view(t.shape)
        new = [place(t) for t in src.new]
        mom = [place(torch.zeros_like(src.new[i])) for i in adapter._TRAINABLE]
        old = [place(t) for t in src.old] if with_old else None
        args = ops.adapter_sweep_args(R, D, H, new, mom, old)
        outs = {}
        for name, n, dt in (("logits", R * B * C, torch.float32), ("rows", R * B, torch.float32), ("mean", R, torch.float32),
                            ("counts", R * G * 2, torch.int64), ("loss_sum", R, torch.float64)):
            fill = 0 if dt != torch.float32 else 7
            buf, v = _guarded(n, dt, fill)
            if dt == torch.float32:
                held.append((buf, n, fill))
            else:
                v.zero_()
                held.append((buf, n, fill))
            outs[name] = v
        nbytes = L.dbmm_workspace_bytes_adapter_sweep_step(R, B, D, H, int(with_old))
        assert nbytes > 0 and nbytes % 16 == 0
        wbuf, ws = _guarded(nbytes // 4)
        held.append((wbuf, nbytes // 4, 7))
        rc = L.dbmm_adapter_sweep_step(table.embeddings.data_ptr(), N_ROWS, idx.data_ptr(), R, B, labels_tab.data_ptr(), table.targets_group.data_ptr(),
                                       args["P"], args["Bf"], args["O"], 0.5, tn.data_ptr(), 0.01, lrs, 0.9, 5e-5, 1, outs["logits"].data_ptr(),
                                       outs["rows"].data_ptr(), outs["mean"].data_ptr(), outs["counts"].data_ptr(), outs["loss_sum"].data_ptr(), G, 1,
                                       R, B, D, H, C, ws.data_ptr(), nbytes, ops.stream())
        assert rc == 0, rc
        torch.cuda.synchronize()
        for buf, n, fill in held:
            assert _guards_intact(buf, n, fill), "a guard zone was written"
        assert int(outs["counts"].view(R, G, 2)[:, :, 0].sum()) == R * B
        results.append([t.clone() for t in new + mom + (old or []) + list(outs.values())])
        # the evaluation entry on the same guarded stacks
        nb = L.dbmm_workspace_bytes_adapter_sweep_eval(R, B, D, H, int(with_old))
        ebuf, ews = _guarded(nb // 4)
        lbuf, lg = _guarded(R * B * C)
        rbuf, rw = _guarded(R * B)
        cbuf, cn = _guarded(R * G * 2, torch.int64, 0)
        sbuf, sm = _guarded(R, torch.float64, 0)
        rc = L.dbmm_adapter_sweep_eval(table.embeddings.data_ptr(), N_ROWS, idx[0].contiguous().data_ptr(), 0, labels_tab.data_ptr(),
                                       table.targets_group.data_ptr(), args["P"], args["O"], 0.5, tn.data_ptr(), 0.01, lg.data_ptr(), rw.data_ptr(),
                                       cn.data_ptr(), sm.data_ptr(), G, R, B, D, H, C, ews.data_ptr(), nb, ops.stream())
        assert rc == 0, rc
        torch.cuda.synchronize()
        for buf, n, fill in ((ebuf, nb // 4, 7), (lbuf, R * B * C, 7), (rbuf, R * B, 7), (cbuf, R * G * 2, 0), (sbuf, R, 0)):
            assert _guards_intact(buf, n, fill), "a guard zone was written (eval)"
        for buf, n, fill in held:
            assert _guards_intact(buf, n, fill), "a guard zone was written (eval)"
        results[-1] += [lg.clone(), rw.clone(), cn.clone(), sm.clone()]
    for a, b in zip(*results):
        assert torch.equal(a, b), "two runs from the same state differ"


def test_wrapper_shape_checks(text_paths_by_dim, table_by_dim):
    table = table_by_dim(512)
    sweep = adapter.SweepAdapters.from_modules(_modules(2, 512, text_paths_by_dim(512), False), "cuda")
    counts = torch.zeros((2, G, 2), dtype=torch.int64, device="cuda")
    loss_sum = torch.zeros((2,), dtype=torch.float64, device="cuda")
    with pytest.raises(_lib.DbmmError):                       # three index rows for two replicas
        sweep.step(table.embeddings, _idx(3, 8, 0), table.targets, table.targets_group, "class", [0.1, 0.1], 0.9, 0.0, counts, loss_sum)
    with pytest.raises(_lib.DbmmError):                       # one row: train-mode BatchNorm1d
        sweep.step(table.embeddings, _idx(2, 4, 0)[:, :1].contiguous(), table.targets, table.targets_group, "class", [0.1, 0.1], 0.9, 0.0, counts,
                   loss_sum)
    with pytest.raises(_lib.DbmmError):                       # one learning rate short
        sweep.step(table.embeddings, _idx(2, 8, 0), table.targets, table.targets_group, "class", [0.1], 0.9, 0.0, counts, loss_sum)
    with pytest.raises(RuntimeError):                         # labels of another table
        sweep.step(table.embeddings, _idx(2, 8, 0), table.targets[:100].contiguous(), table.targets_group, "class", [0.1, 0.1], 0.9, 0.0, counts,
                   loss_sum)
    with pytest.raises(_lib.DbmmError):                       # counters of another replica count
        sweep.step(table.embeddings, _idx(2, 8, 0), table.targets, table.targets_group, "class", [0.1, 0.1], 0.9, 0.0, counts[:1].contiguous(),
                   loss_sum)


# ---- the sweep driver --------------------------------------------------------------------------------------------------------

CFG = dict(seed=3, dim=512, n_train=1000, n_val=600, n_test=700)
SEEDS = (0, 1, 2)


def _opt(d, **kw):
    tcls, tspu, tgrp = synth.embedding_text(CFG["seed"], CFG["dim"])
    o = dict(tl_method="adapter_reg_seq_alter", dataset="waterbirds", epochs=6, epochs_feature_learning=3, batch_size=256, batch_size_reg=64,
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
            if a["kind"] == "init":
                assert all(torch.equal(a["state"][k], b["state"][k]) for k in b["state"]), (r, "init")
            elif a["kind"] == "final":
                assert a["best_epoch"] == b["best_epoch"], (r, "best epoch")
                sa, sb = a["best_model"].state_dict(), b["best_model"].state_dict()
                assert list(sa) == list(sb), (r, "state-dict keys")
                for k in sb:
                    assert torch.equal(sa[k], sb[k]), (r, k)
            else:
                assert np.array_equal(a["counts"], b["counts"]), (r, a["kind"], a.get("epoch"))
                assert a["group_acc"] == b["group_acc"] and a["acc"] == b["acc"], (r, a["kind"], a.get("epoch"))
                assert abs(a["loss"] - b["loss"]) <= 1e-12 * max(1.0, abs(b["loss"])), (r, a["kind"], a.get("epoch"), a["loss"], b["loss"])
                if "order" in b:
                    assert np.array_equal(a["order"], b["order"]), (r, a["kind"], a.get("epoch"))
                if "use_group" in b:
                    assert a["use_group"] == b["use_group"]


SCHEDULES = {
    "adapter": dict(tl_method="adapter"),
    "adapter_reg_seq": dict(tl_method="adapter_reg_seq"),
    "adapter_reg_seq_cls_warm": dict(tl_method="adapter_reg_seq", use_cls_prompt_in_reg=True, warm=True, warm_epochs=2, warmup_from=0.01,
                                     warmup_to=0.05, warm_reg=True, warm_epochs_reg=2, warmup_from_reg=0.005, warmup_to_reg=0.02),
    "alter_full_ni": dict(tl_method="adapter_reg_seq_alter", add_adapter=True, balance_val=True, continue_from_best=True, init_near_identity=True),
    "alter_full_rn": dict(tl_method="adapter_reg_seq_alter", add_adapter=True, balance_val=True, continue_from_best=True, init_near_identity=False),
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


def test_more_than_sixteen_replicas_are_split_into_groups(tables, tmp_path_factory):
    """18 seeds: one group of 16 replicas and one of 2, results in seed order"""
    opt = _opt(str(tmp_path_factory.mktemp("sweep")), tl_method="adapter_reg_seq")
    seeds = list(range(18))
    want, _ = _sequential(opt, tables, seeds)
    got = trainer.train_sweep(opt, *tables, seeds)
    assert got == want


@pytest.mark.parametrize("method", ["adapter_reg", "linear_probing"])
def test_fallback_methods_return_the_sequential_results(method, tables, tmp_path_factory):
    opt = _opt(str(tmp_path_factory.mktemp("sweep")), tl_method=method, epochs=3, balance_val=True)
    want, _ = _sequential(opt, tables, SEEDS[:2])
    got = trainer.train_sweep(opt, *tables, SEEDS[:2])
    assert got == want


def test_contrastive_adapter_keeps_raising(tables, tmp_path_factory):
    opt = _opt(str(tmp_path_factory.mktemp("sweep")), tl_method="contrastive_adapter")
    with pytest.raises(ValueError):
        trainer.train_sweep(opt, *tables, SEEDS)


# ---- against the reference's own sweep driver (tests/golden/sweep_wb.npz, tools/make_golden_sweep.py) ------------------------

@pytest.fixture(scope="module")
def wb_run(tmp_path_factory):
    from conftest import GOLDEN
    g = np.load(os.path.join(GOLDEN, "sweep_wb.npz"), allow_pickle=False)
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
    """per pass and seed: row orders equal; counters within the fixture's own 1-ulp / 8-ulp sensitivity + 1; losses within
    2e-3 max(1, |loss|) + 4 x the reference's own perturbation distance (the schedule tests' bound); best epoch per seed equal"""
    g, opt, log, _ = wb_run
    assert len(log) == int(g["n_seeds"])
    for s, lg in enumerate(log):
        passes = [e for e in lg if e["kind"] in ("train1", "train2", "validate", "validate_zs")]
        assert len(passes) == int(g[f"s{s}/n_phases"])
        flips = 0
        for i, e in enumerate(passes):
            k = f"s{s}/p{i}/"
            assert e["kind"] == str(g[k + "kind"]), (s, i)
            if e["kind"] in ("train1", "train2"):
                assert np.array_equal(e["order"], g[k + "idx"].astype(np.int64)), (s, i)
            if e["kind"] == "train2":
                assert e["use_group"] == bool(g[k + "use_group"]), (s, i)
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
