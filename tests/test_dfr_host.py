"""Deep feature reweighting without a GPU: the float64 reference of the L1-probe iteration (dfr.prox_fit_reference), the pieces of
DFR-Val that need no launch, train_dfr on its solver="reference" path, the C-level refusals of dbmm_linear_prox_fit through the built
library, and the CPU-side facts the GPU tests (tests/test_gpu_dfr.py) rely on: the band cap of their cases, the tuning margin."""
import ctypes
import math
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import dfr_cases as K
from dbmm_amd import _lib, adapter, analysis, dfr, ops, synth, trainer


def _small(n=64, D=16, C=3, seed=5):
    x = synth.normal(seed, "x", (n, D)).contiguous()
    y = (synth.uniform(seed, "y", (n,)) * C).long().clamp(0, C - 1)
    return x, y, torch.arange(n)[None]


def _run(x, y, idx, lam, iters, C, accelerate=True, dtype=torch.float64):
    step = dfr.prox_steps(x, idx)
    return dfr.prox_fit_reference(x, idx, y, [lam], step, None, iters, accelerate, dtype=dtype, n_classes=C)


# ---- the iteration ----------------------------------------------------------------------------------------------------------------
def test_reference_reaches_its_own_long_run():
    """n = 64, D = 16, C = 3: 1500 iterations are no worse than 5000 by 1e-9 relative"""
    x, y, idx = _small()
    for lam in (0.0, 0.01, 0.05):
        f = {}
        for k in (1500, 5000):
            st, _ = _run(x, y, idx, lam, k, 3)
            f[k] = dfr.objective(x, idx, y, st.w, st.b, [lam])[0].item()
        print(f"lam {lam}: F_1500 {f[1500]:.12f} F_5000 {f[5000]:.12f} rel {(f[1500] - f[5000]) / f[5000]:.2e}")
        assert f[1500] <= f[5000] * (1 + 1e-9)


def test_objective_is_sklearns_at_lam_equal_one_over_c_n():
    """the lam <-> C mapping: no worse than saga's objective at C_sk by the slack saga's own tol leaves"""
    lm = pytest.importorskip("sklearn.linear_model")
    x, y, idx = _small()
    n = x.shape[0]
    for c_sk in (1.0, 0.1):
        lam = 1.0 / (c_sk * n)
        st, _ = _run(x, y, idx, lam, 3000, 3)
        ours = dfr.objective(x, idx, y, st.w, st.b, [lam])[0].item()
        tol = 1e-6
        sk = lm.LogisticRegression(penalty="l1", solver="saga", C=c_sk, tol=tol, max_iter=20000, fit_intercept=True, random_state=0).fit(x.numpy(), y.numpy())
        W, b = torch.from_numpy(sk.coef_)[None], torch.from_numpy(sk.intercept_)[None]
        theirs = dfr.objective(x, idx, y, W, b, [lam])[0].item()
        # saga stops when max |dw| <= tol max |w|: its iterate is within that of a fixed point, the objective within first order of it
        slack = tol * max(1.0, abs(theirs))
        print(f"C {c_sk}: ours {ours:.10f} saga {theirs:.10f}")
        assert ours <= theirs + slack
        # and the mapping is not off by a factor: the penalty term is a tenth of the objective here, so the optimum under lam / 2 or
        # 2 lam is percents away from saga's
        assert abs(ours - theirs) <= 1e-3 * abs(theirs)


def test_exact_zeros_and_a_moving_intercept():
    x, y, idx = _small()
    C = 3
    p0 = torch.full((x.shape[0], C), 1.0 / C, dtype=torch.float64)
    p0[torch.arange(x.shape[0]), y] -= 1
    g0 = (p0.t() @ x.double() / x.shape[0]).abs().max().item()
    for dtype in (torch.float64, torch.float32):
        st, stats = _run(x, y, idx, g0 * 1.0001, 20, C, dtype=dtype)
        assert bool((st.w == 0).all()) and bool((st.v == 0).all()) and stats["nnz"][0] == 0
        assert st.b.abs().max() > 1e-3
    st, _ = _run(x, y, idx, g0 * 0.5, 50, C)
    z = (st.w == 0)
    assert 0 < int(z.sum()) < z.numel()                    # some exact zeros, not all


def test_beta_sequence_is_the_float64_recurrence():
    betas, t_end = dfr.beta_sequence(12)
    t = np.float64(1.0)
    for k in range(12):
        t1 = (np.float64(1.0) + np.sqrt(np.float64(1.0) + np.float64(4.0) * t * t)) / np.float64(2.0)
        assert betas[k] == float(np.float32((t - 1.0) / t1))
        t = t1
    assert t_end == float(t) and betas[0] == 0.0
    # the reference applies them: V_k - W_k = beta_k (W_k - W_{k-1}), and t round-trips through the state
    x, y, idx = _small()
    s2, _ = _run(x, y, idx, 0.01, 2, 3)
    s3, _ = dfr.prox_fit_reference(x, idx, y, [0.01], dfr.prox_steps(x, idx), s2, 1, True, n_classes=3)
    assert torch.allclose(s3.v - s3.w, betas[2] * (s3.w - s2.w), rtol=0, atol=1e-15)
    assert s3.t.item() == dfr.beta_sequence(3)[1]
    s3b, _ = _run(x, y, idx, 0.01, 3, 3)
    assert all(torch.equal(a, b) for a, b in zip(s3, s3b))
    ista, _ = _run(x, y, idx, 0.01, 3, 3, accelerate=False)
    assert torch.equal(ista.v, ista.w) and not torch.equal(ista.w, s3.w)


# ---- the pieces of DFR-Val --------------------------------------------------------------------------------------------------------
def test_folded_weights_on_raw_rows_are_the_weights_on_standardised_rows():
    x = synth.normal(2, "rows", (50, 12)).double() * 3 + 1.5
    x[:, 4] = 2.0                                           # a constant column: sigma = 0 -> 1
    mean, std = dfr.column_moments(x.float())
    assert std[4] == 1.0 and mean[4] == 2.0
    assert torch.allclose(std[:4], x.float().double().std(0, unbiased=False)[:4], rtol=1e-12)
    W, b = synth.normal(2, "W", (3, 12)).double(), synth.normal(2, "b", (3,)).double()
    Wf, bf = dfr.fold_standardisation(W, b, mean, std)
    xr = x.float().double()
    a = ((xr - mean) / std) @ W.t() + b
    f = xr @ Wf.t() + bf
    assert (a - f).abs().max().item() <= 1e-12 * max(1.0, a.abs().max().item())
    z = dfr.standardised(x.float(), mean, std)
    assert z.dtype == torch.float32 and bool((z[:, 4] == 0).all()) and bool(torch.isfinite(z).all())


def test_draws_are_deterministic_and_private():
    g = np.array([0] * 50 + [1] * 9 + [2] * 5 + [3] * 30)
    s0 = (torch.get_rng_state().clone(), np.random.get_state()[1].copy())
    ha, hb = dfr.val_halves(len(g), 7)
    sub = dfr.balanced_subsets(g, ha, [8, 9])
    assert torch.equal(s0[0], torch.get_rng_state()) and (s0[1] == np.random.get_state()[1]).all()
    ha2, hb2 = dfr.val_halves(len(g), 7)
    assert (ha == ha2).all() and (hb == hb2).all() and (sub == dfr.balanced_subsets(g, ha, [8, 9])).all()
    assert len(ha) == 47 and len(hb) == 47 and not set(ha) & set(hb) and sorted(set(ha) | set(hb)) == list(range(len(g)))
    m = np.bincount(g[ha]).min()
    assert sub.shape == (2, 4 * m) and set(sub[0]) <= set(ha) and (sub[0] != sub[1]).any()
    assert (np.bincount(g[sub[0]]) == m).all()
    assert (sub[0] == ha[analysis.balanced_rows(g[ha], seed=8)]).all()          # balanced_rows' drawing rule
    assert (dfr.val_halves(len(g), 8)[0] != ha).any()


def test_ties_go_to_the_smaller_c():
    assert dfr.pick_c([1.0, 0.7, 0.3], [0.5, 0.5, 0.4]) == 1
    assert dfr.pick_c([0.3, 0.7, 1.0], [0.5, 0.5, 0.4]) == 0
    assert dfr.pick_c([1.0, 0.7, 0.3], [0.5, 0.6, 0.6]) == 2
    assert dfr.pick_c([1.0, 0.7, 0.3], [0.7, 0.6, 0.6]) == 0


def test_launch_iters_caps_row_visits():
    assert dfr.launch_iters(188, 32, 1000) == 32 and dfr.launch_iters(188, 32, 5) == 5
    assert dfr.launch_iters(3000, 32, 1000) == dfr.MAX_ROW_VISITS // 3000 < 32
    assert dfr.launch_iters(10 ** 7, 32, 1000) == 1


def _tiny_tables(n_val=80, groups_missing=None, device="cpu"):
    out = []
    for split, n in (("train", 120), ("val", n_val), ("test", 60)):
        x, y, c = synth.embedding_dataset(4, split, n, dim=16, p_y=0.5, p_agree=0.7)
        if split == "val" and groups_missing is not None:
            keep = (2 * y + c) != groups_missing
            x, y, c = x[keep], y[keep], c[keep]
        out.append(trainer.EmbeddingTable(x, y, c, device=device))
    return out


def test_every_refusal_precedes_a_model_and_a_launch(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("reached past the refusals")
    monkeypatch.setattr(adapter, "LinearClassifier", boom)
    monkeypatch.setattr(dfr, "fit_l1_probes", boom)
    monkeypatch.setattr(ops, "linear_prox_fit", boom)
    monkeypatch.setattr(ops, "linear_sweep_eval", boom)
    tr, va, te = _tiny_tables()
    base = dict(dfr_solver="reference", n_cls=2, batch_size=64)
    for bad, what in ((dict(dfr_c_grid=[]), "empty"), (dict(dfr_c_grid=[1.0, 0.0]), "positive"), (dict(dfr_c_grid=[-1.0]), "positive"),
                      (dict(dfr_c_grid=[float("nan")]), "positive"), (dict(n_cls=9), "8 classes"), (dict(n_cls=1), "outside"),
                      (dict(dfr_solver="sklearn"), "dfr_solver"), (dict(dfr_retrains=0), "dfr_retrains")):
        with pytest.raises(ValueError, match=what):
            trainer.train_dfr(SimpleNamespace(**{**base, **bad}), tr, va, te)
    _, va3, _ = _tiny_tables(groups_missing=2)
    with pytest.raises(ValueError, match="absent from the validation split"):
        trainer.train_dfr(SimpleNamespace(**base), tr, va3, te)
    # a group that the split has but one half has not: one row of it
    x, y, c = synth.embedding_dataset(4, "val", 80, dim=16, p_y=0.5, p_agree=0.7)
    g = (2 * y + c).numpy()
    keep = np.ones(len(g), dtype=bool)
    keep[np.flatnonzero(g == 1)[1:]] = False
    va1 = trainer.EmbeddingTable(x[keep], y[keep], c[keep], device="cpu")
    with pytest.raises(ValueError, match="half"):
        trainer.train_dfr(SimpleNamespace(**base), tr, va1, te)
    monkeypatch.undo()
    with pytest.raises(ValueError, match="solver"):
        dfr.fit_l1_probes(va.embeddings, np.arange(8)[None], va.targets, [0.1], solver="torch")
    with pytest.raises(ValueError, match="label outside"):
        dfr.fit_l1_probes(va.embeddings, np.arange(len(va))[None], va.targets_group, [0.1], solver="reference", n_classes=2)


# ---- DFR-Val on the reference solver ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def split():
    return K.dfr_split()


def test_dfr_beats_erm_on_the_worst_group(split):
    """synth.embedding_dataset(3, ..., dim=64), 4000 / 1200 / 4000 rows: the ERM optimum (the same solver at lam = 0 on train) against
    DFR-Val, worst-group test accuracy.  A float64 prototype gave 0.14 and 0.55 - 0.57."""
    tr, va, te = split
    erm = dfr.fit_l1_probes(tr.embeddings, np.arange(len(tr))[None], tr.targets, [0.0], solver="reference", max_iter=3000)
    assert bool(erm.converged.all())
    c, _ = trainer._probe_counts(te.embeddings, te.targets, te.targets_group, 4, erm.weights, erm.intercepts)
    erm_worst = trainer._worst_group_acc(c[0])
    log = []
    s0 = (torch.get_rng_state().clone(), np.random.get_state()[1].copy())
    clf, scores, record = trainer.train_dfr(SimpleNamespace(dfr_solver="reference", n_cls=2, batch_size=128), tr, va, te, log=log)
    assert torch.equal(s0[0], torch.get_rng_state()) and (s0[1] == np.random.get_state()[1]).all()
    worst = scores[2][2]["worst_acc"]
    print(f"ERM worst-group test accuracy {erm_worst:.4f}, DFR {worst:.4f} at C = {record['C']}")
    assert worst - erm_worst >= 0.2
    assert [r["kind"] for r in log] == ["dfr_tune", "dfr_fit", "dfr_eval", "dfr_eval", "dfr_eval"]
    assert record["C"] in dfr.DEFAULT_C_GRID and len(record["tuning"]) == 7 and all(record["converged"]) and len(record["nnz"]) == 10
    assert isinstance(clf, adapter.LinearClassifier) and tuple(clf.fc.weight.shape) == (2, 64)
    # the classifier on raw rows is the averaged probe on standardised rows
    fit = log[1]
    W, b = fit["weights"].double().mean(0), fit["intercepts"].double().mean(0)
    z = (va.embeddings.double() - record["mean"]) / record["std"]
    raw = va.embeddings.double() @ clf.fc.weight.detach().double().t() + clf.fc.bias.detach().double()
    assert (z @ W.t() + b - raw).abs().max().item() < 1e-5               # float32 weights in the classifier
    # with equal tuning scores the smaller C is taken (seed 0: C = 1 and C = 0.7 tie)
    t = {r["C"]: r["mean"] for r in record["tuning"]}
    assert t[1.0] == t[0.7] == max(t.values()) and record["C"] == 0.7


def test_the_full_grid_seed_has_a_clear_margin(split):
    """what test_gpu_dfr.py's chosen-C test relies on: at dfr_seed = TUNE_SEED the reference's best and second-best tuning scores are
    at least two rows of the held-out half's smallest group apart"""
    tr, va, te = split
    log = []
    _, _, record = trainer.train_dfr(SimpleNamespace(dfr_solver="reference", n_cls=2, dfr_seed=K.TUNE_SEED, dfr_retrains=1), tr, va, te, log=log)
    margin, need = K.tuning_margin(record, va, log[0]["halves"])
    print(f"margin {margin:.4f}, two rows of the smallest group {need:.4f}, C = {record['C']}")
    assert margin >= need and record["C"] == 0.1


# ---- what the GPU cases rely on ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", K.SHAPES)
def test_gpu_cases_stay_inside_the_band_cap(shape):
    for iters in K.ITERS:
        for acc in (True, False):
            m = K.band_mask(*shape, iters, acc)
            out = 1.0 - m.double().mean().item()
            assert out <= K.BAND_CAP, (shape, iters, acc, out)
            s64 = K.references(*shape, iters, acc)[0]
            assert bool(torch.isfinite(s64.w).all())
    R = shape[3]
    w = K.references(*shape, 8, True)[0].w
    if R >= 3:
        assert bool((w[2] == 0).all())                     # LAM_BIG zeroes everything
    if R >= 2:
        assert bool((w[1] != 0).all())                     # lam = 0: no zero
    assert 0 < int((w[0] == 0).sum()) < w[0].numel() or shape[0] == 1


# ---- the C entry's refusals, through the built library ----------------------------------------------------------------------------------
def test_c_entry_refusals_without_gpu():
    L = _lib.lib() if _lib.build() else None
    raw = (ctypes.c_float * 4200)()
    base = ctypes.addressof(raw)
    p = base + (-base) % 16                                # 16-byte aligned host memory: nothing is launched on a refusal
    args = lambda **k: [k.get(a, p) for a in ("table",)] + [k.get("n_rows", 8)] + [k.get(a, p) for a in
                       ("idx", "labels", "lam", "step", "w", "b", "v", "c", "t", "stats")] + \
                      [k.get("R", 2), k.get("n", 8), k.get("D", 16), k.get("C", 2), k.get("iters", 1), 1, None]
    for name in ("table", "idx", "labels", "lam", "step", "w", "b", "v", "c", "t", "stats"):
        assert L.dbmm_linear_prox_fit(*args(**{name: None})) == -4, name
    for bad in (dict(R=0), dict(R=257), dict(n=0), dict(D=2), dict(D=18), dict(D=1028), dict(C=0), dict(C=9), dict(iters=0), dict(iters=-3),
                dict(iters=(1 << 20) + 1), dict(n_rows=0)):
        assert L.dbmm_linear_prox_fit(*args(**bad)) == -1, bad
    for name in ("table", "w", "v", "stats"):
        assert L.dbmm_linear_prox_fit(*args(**{name: p + 4})) == -2, name
    for name in ("idx", "labels", "t"):
        assert L.dbmm_linear_prox_fit(*args(**{name: p + 4})) == -2, name
    assert L.dbmm_linear_prox_fit(*args(w=None, R=0)) == -4              # a null pointer is named first


def test_wrapper_refuses_host_tensors():
    st = ops.ProxState(torch.zeros(1, 2, 8), torch.zeros(1, 2), torch.zeros(1, 2, 8), torch.zeros(1, 2), torch.ones(1, dtype=torch.float64))
    with pytest.raises(_lib.DbmmError):
        ops.linear_prox_fit(torch.zeros(4, 8), torch.zeros(1, 4, dtype=torch.int64), torch.zeros(4, dtype=torch.int64), torch.zeros(1),
                            torch.ones(1), st, 1)
    assert math.isfinite(dfr.MAX_ROW_VISITS)
