"""The kernel ridge probe on the MI355X: the matrix-free RBF kernel product (ops.pairdist_rbf_matvec) and analysis.kernel_ridge_fit /
kernel_ridge_predict / kernel_ridge_probe / ridge_report against dense float64: torch.cdist(xd, xd) ** 2 -> exp, diagonal zeroed,
times the weights.

The bound of an entry R[i, c] is 1e-4 * sum_{j != i} k_ij |v_jc|: the per-term bound of test_gpu_kernel_probe.py's header (the 22-bit
split, the fp32 coefficient and product, the hardware exp2: under 6e-5 on every kernel value under the two preconditions
gamma * max_ij (|a|^2 + |b|^2) <= 64 and gamma * max d^2 <= 80), plus the weight product w0 k0 + w1 k1 (a multiply and a fused
multiply-add in fp32: 2 * 2^-24), plus the fp32 tree over a wave's 64 columns (6 * 2^-24) -- relative to the sum of the ABSOLUTE terms,
because the weights are signed and the terms may cancel.  An entry whose sum of absolute terms is 0 must be exactly 0.  Both
preconditions are asserted on every test's own inputs in float64; the generators, the ladders and check_preconditions are
pairdist_cases.py's, and every test prints its figures before it asserts.

The fit is checked backward (the dense float64 residual of the returned coefficients, valid at any conditioning) and, at lam = 1
only, forward: ||alpha^ - alpha|| <= kappa (1e-4 + tol) ||alpha|| with kappa = cond(K + lam I) from eigvalsh -- the operator's error is
entrywise relative on non-negative entries, so its 2-norm is at most 1e-4 ||K||_2; at lam = 0.1 kappa reaches the thousands on these
inputs and the bound says nothing."""
import functools

import numpy as np
import pytest
import torch

from pairdist_cases import DEV, GuardedAlloc, check_preconditions, clustered_rows, ladder, rows, sq_dists

pytestmark = pytest.mark.gpu

RTOL = 1e-4
TOL = 1e-5                                 # kernel_ridge_fit's default stopping residual


def kernel_f64(d2, gam):
    """the float64 kernel matrix of square squared distances, diagonal zeroed"""
    K = torch.exp(-gam * d2)
    K.fill_diagonal_(0.0)
    return K


def check_product(R, K, v, what, factor=1.0):
    """|R - K v| <= factor * 1e-4 * K |v| on every entry, an exact 0 where K |v| is 0; returns the worst ratio to the bound's unit"""
    ref, unit = K @ v.double(), K @ v.double().abs()
    assert R.shape == ref.shape and R.dtype == torch.float64 and R.device == ref.device
    assert torch.isfinite(R).all()
    live = unit > 0
    ratio = ((R - ref).abs() / unit.clamp_min(1e-300)).where(live, torch.zeros_like(ref))
    worst = ratio.max().item() if ratio.numel() else 0.0
    print(f"{what}: worst |R - R64| / sum k|v| = {worst:.3e} over {int(live.sum())} entries with a term")
    assert (ratio <= factor * RTOL).all(), f"{what}: an entry is off by more than {factor * RTOL} of its sum of absolute terms"
    assert (R[~live] == 0).all(), f"{what}: an entry without a term is not exactly 0"
    return worst


def weight_cases(n, C, seed):
    g = torch.Generator().manual_seed(seed)
    normal = torch.randn(n, C, generator=g)
    onehot = torch.nn.functional.one_hot(torch.randint(0, C, (n,), generator=g), C).float()
    block = torch.zeros(n, C)
    block[256:512] = normal[256:512]                                    # one whole row block carries weight: every other tile is skipped
    head = torch.zeros(n, C)
    head[:100] = normal[:100]
    return {"normal": normal, "onehot": onehot, "rows_256_511": block, "first_100": head}


# ---- the product against float64 --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("d", [64, 192, 1024])
@pytest.mark.parametrize("n", [1, 2, 255, 256, 257, 513, 1000])
def test_product_shapes_columns_and_weights(n, d):
    from dbmm_amd import ops
    worst = 0.0
    for kind in ("iso", "clustered"):
        seed = 1000 * n + d
        x = rows(n, d, seed) if kind == "iso" else clustered_rows(n, d, seed)[0]
        lad = ladder(kind, d)
        d2 = sq_dists(x)
        check_preconditions(x, d2, lad, f"N={n} D={d} {kind}")
        center = x.mean(0)
        for gam in (lad[0], lad[-1]):
            K = kernel_f64(d2, gam)
            for C in (1, 3, 16):
                for name, v in weight_cases(n, C, seed + C).items():
                    v = v.to(DEV).contiguous()
                    R = ops.pairdist_rbf_matvec(x, v, center, gam)
                    assert R.shape == (n, C)
                    worst = max(worst, check_product(R, K, v, f"N={n} D={d} {kind} gamma={gam:.3e} C={C} {name}"))
    print(f"N={n} D={d}: worst ratio of the case {worst:.3e} (bound {RTOL})")


def test_product_more_than_sixteen_row_blocks():
    """N = 4353: 18 row blocks, the last of one row; a unit of the schedule holds several column blocks"""
    from dbmm_amd import ops
    n, d = 4353, 64
    x, _ = clustered_rows(n, d, 16)
    lad = ladder("clustered", d)
    d2 = sq_dists(x)
    check_preconditions(x, d2, lad, "N=4353")
    for gam in (lad[0], lad[-1]):
        K = kernel_f64(d2, gam)
        for name, v in weight_cases(n, 3, 17).items():
            v = v.to(DEV).contiguous()
            check_product(ops.pairdist_rbf_matvec(x, v, x.mean(0), gam), K, v, f"N=4353 gamma={gam:.3e} {name}")


# ---- further properties of the product --------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def property_case():
    n, d = 1000, 192
    x = rows(n, d, 31)
    lad = ladder("iso", d)
    d2 = sq_dists(x)
    check_preconditions(x, d2, lad, "properties N=1000 D=192")
    g = torch.Generator().manual_seed(32)
    return x, x.mean(0), lad[1], kernel_f64(d2, lad[1]), torch.randn(n, 16, generator=g).to(DEV), torch.randn(n, 16, generator=g).to(DEV)


def test_a_column_does_not_depend_on_the_others_and_calls_repeat():
    from dbmm_amd import ops
    x, c, gam, K, v, _ = property_case()
    v = v.clone()
    v[300:600, 5] = 0                                                   # a column with a skipped block of its own
    R = ops.pairdist_rbf_matvec(x, v, c, gam)
    assert torch.equal(R, ops.pairdist_rbf_matvec(x, v, c, gam)), "two calls on the same input differ"
    for col in range(16):
        R1 = ops.pairdist_rbf_matvec(x, v[:, col:col + 1].contiguous(), c, gam)
        assert torch.equal(R1[:, 0], R[:, col]), f"column {col}: C = 1 and C = 16 differ in bits"
    check_product(R, K, v, "C=16 with a partly zero column")


def test_one_hot_weights_agree_with_the_row_sum_kernel():
    from dbmm_amd import ops
    x, c, gam, K, _, _ = property_case()
    n = x.shape[0]
    for name, g in (("shuffled", torch.randint(0, 4, (n,), generator=torch.Generator().manual_seed(33))),
                    ("sorted", torch.sort(torch.randint(0, 4, (n,), generator=torch.Generator().manual_seed(33))).values)):
        g = g.to(DEV)
        oh = torch.nn.functional.one_hot(g, 4).float().contiguous()
        A = ops.pairdist_rbf_matvec(x, oh, c, gam)
        B = ops.pairdist_rbf_row_group_sums(x, g, 4, c, [gam])[0]
        ref = K @ oh.double()
        ra, rb, rel = ((A - ref).abs() / ref).max().item(), ((B - ref).abs() / ref).max().item(), ((A - B).abs() / B).max().item()
        print(f"one-hot {name}: product vs float64 {ra:.3e}, row sums vs float64 {rb:.3e}, product vs row sums {rel:.3e}, bit-equal {torch.equal(A, B)}")
        assert ra <= RTOL and rb <= RTOL and rel <= 2e-4


def test_permuted_rows_give_the_permuted_product():
    from dbmm_amd import ops
    x, c, gam, K, v, _ = property_case()
    v = v[:, :4].contiguous()
    perm = torch.randperm(x.shape[0], generator=torch.Generator().manual_seed(34)).to(DEV)
    R = ops.pairdist_rbf_matvec(x, v, c, gam)
    Rp = ops.pairdist_rbf_matvec(ops.gather_rows(x, perm), v[perm].contiguous(), c, gam)
    unit = K @ v.double().abs()
    ratio = ((Rp - R[perm]).abs() / unit[perm]).max().item()
    print(f"permutation: worst |R_perm - R[perm]| / sum k|v| = {ratio:.3e} (<= 2e-4)")
    assert ratio <= 2e-4


def test_the_product_is_symmetric_within_its_bound():
    """u^T (K v) against v^T (K u): conjugate gradients rest on this near-symmetry"""
    from dbmm_amd import ops
    x, c, gam, K, v, u = property_case()
    Kv, Ku = ops.pairdist_rbf_matvec(x, v, c, gam), ops.pairdist_rbf_matvec(x, u, c, gam)
    a, b = (u.double() * Kv).sum(0), (v.double() * Ku).sum(0)
    unit = (u.double().abs() * (K @ v.double().abs())).sum(0)
    ratio = ((a - b).abs() / unit).max().item()
    print(f"symmetry: worst |u^T K v - v^T K u| / |u|^T K |v| = {ratio:.3e} (<= 2e-4) over 16 column pairs")
    assert ratio <= 2e-4


def test_nothing_is_written_outside_the_product_and_the_workspace(monkeypatch):
    """a ragged last block, three columns: the last partial and the last entry are the edges"""
    from dbmm_amd import ops
    n, d = 257, 192
    x = rows(n, d, 25)
    v = torch.randn(n, 3, generator=torch.Generator().manual_seed(26)).to(DEV)
    lad = ladder("iso", d)
    d2 = sq_dists(x)
    check_preconditions(x, d2, lad, "guarded")
    ga = GuardedAlloc()
    monkeypatch.setattr(ops, "_empty", ga)
    R = ops.pairdist_rbf_matvec(x, v, x.mean(0), lad[1])
    torch.cuda.synchronize()
    assert len(ga.bufs) == 2                                                    # workspace, product
    ga.check()
    check_product(R, kernel_f64(d2, lad[1]), v, "guarded N=257 C=3")


# ---- the fit -----------------------------------------------------------------------------------------------------------------------------

FIT_SHAPES = [(257, 100, 64), (513, 256, 64), (700, 300, 192), (700, 300, 1024)]
FIT_LAMS = (0.1, 1.0)


@functools.lru_cache(maxsize=None)
def fitted(n, m, d):
    """one draw of n + m clustered rows, the first n fitted; the fit, its predictions of the other m, and the dense float64 side"""
    from dbmm_amd import analysis
    x, cluster = clustered_rows(n + m, d, 1000 * (n + m) + d)
    labels = cluster.numpy()
    fit = analysis.kernel_ridge_fit(x[:n].contiguous(), labels[:n], scales=(1.0, 4.0), lams=FIT_LAMS)
    pred = analysis.kernel_ridge_predict(fit, x[n:].contiguous())
    d2 = sq_dists(x)
    check_preconditions(x, d2, fit["gammas"].tolist(), f"fit n={n} m={m} D={d}")
    uniq, dense = np.unique(labels[:n], return_inverse=True)
    G = len(uniq)
    freq = torch.as_tensor(np.bincount(dense, minlength=G) / n, device=DEV)
    T = torch.nn.functional.one_hot(torch.as_tensor(dense, device=DEV), G).double() - freq
    return {"fit": fit, "pred": pred, "d2": d2, "T": T, "freq": freq, "G": G, "labels": labels, "uniq": uniq}


@pytest.mark.parametrize("n,m,d", FIT_SHAPES)
def test_fit_backward_error(n, m, d):
    """the dense float64 residual of every column is at most its reported residual plus the product's bound, at any conditioning"""
    s = fitted(n, m, d)
    fit, T = s["fit"], s["T"]
    assert fit["alpha"].shape == (2, 2, n, s["G"]) and fit["alpha"].dtype == torch.float64 and fit["alpha"].is_cuda
    assert fit["iterations"].shape == (2,) and fit["residual"].shape == (2, 2, s["G"]) and fit["converged"].shape == (2, 2, s["G"])
    print(f"n={n} D={d}: iterations {fit['iterations'].tolist()}, converged {fit['converged'].all()}")
    assert fit["converged"].all(), "a column did not converge within max_iter"
    eye = torch.eye(n, dtype=torch.float64, device=DEV)
    for l, gam in enumerate(fit["gammas"]):
        K0 = kernel_f64(s["d2"][:n, :n].clone(), gam)
        for a, lam in enumerate(FIT_LAMS):
            al = fit["alpha"][l, a]
            dense = ((K0 + (1.0 + lam) * eye) @ al - T).norm(dim=0) / T.norm(dim=0)
            slack = RTOL * (K0 @ al.abs()).norm(dim=0) / T.norm(dim=0)
            rep = torch.as_tensor(fit["residual"][l, a], device=DEV)
            print(f"n={n} D={d} gamma={gam:.3e} lam={lam}: dense residual {dense.tolist()}, reported {rep.tolist()}, product's bound {slack.tolist()}")
            assert (dense <= rep + slack).all()


@pytest.mark.parametrize("n,m,d", FIT_SHAPES)
def test_fit_forward_error_at_lam_one(n, m, d):
    s = fitted(n, m, d)
    fit, T = s["fit"], s["T"]
    a = FIT_LAMS.index(1.0)
    eye = torch.eye(n, dtype=torch.float64, device=DEV)
    for l, gam in enumerate(fit["gammas"]):
        A = kernel_f64(s["d2"][:n, :n].clone(), gam) + 2.0 * eye
        ev = torch.linalg.eigvalsh(A)
        kappa = (ev[-1] / ev[0]).item()
        want = torch.linalg.solve(A, T)
        err = (fit["alpha"][l, a] - want).norm(dim=0)
        bound = kappa * (RTOL + TOL) * want.norm(dim=0)
        print(f"n={n} D={d} gamma={gam:.3e}: kappa {kappa:.1f}, ||alpha^ - alpha|| {err.tolist()}, bound {bound.tolist()}, "
              f"smallest bound / error {(bound / err.clamp_min(1e-300)).min().item():.1f}")
        assert (err <= bound).all()


def decided_rows(Kq, A, T, freq):
    """float64 scores of the query rows, and per row the bound of a score and whether its top-two gap exceeds four times that"""
    ev = torch.linalg.eigvalsh(A)
    kappa = (ev[-1] / ev[0]).item()
    alpha = torch.linalg.solve(A, T)
    scores = Kq @ alpha + freq
    per_class = Kq.norm(dim=1, keepdim=True) * kappa * (RTOL + TOL) * alpha.norm(dim=0).max() + RTOL * (Kq @ alpha.abs())      # [M, G]
    top = torch.sort(scores, dim=1).values
    gap = top[:, -1] - top[:, -2]
    return scores, per_class, gap > 4.0 * per_class.max(dim=1).values, kappa, gap


@pytest.mark.parametrize("n,m,d", FIT_SHAPES)
def test_predictions_at_lam_one(n, m, d):
    s = fitted(n, m, d)
    fit, pred = s["fit"], s["pred"]
    a = FIT_LAMS.index(1.0)
    assert pred["scores"].shape == (2, 2, m, s["G"]) and pred["pred"].shape == (2, 2, m) and pred["margin"].shape == (2, 2, m)
    eye = torch.eye(n, dtype=torch.float64, device=DEV)
    for l, gam in enumerate(fit["gammas"]):
        Kall = torch.exp(-gam * s["d2"])
        scores, bound, decided, kappa, gap = decided_rows(Kall[n:, :n], kernel_f64(s["d2"][:n, :n].clone(), gam) + 2.0 * eye, s["T"], s["freq"])
        got = torch.as_tensor(pred["scores"][l, a], device=DEV)
        want_pred = s["uniq"][scores.argmax(1).cpu().numpy()]
        left_out = int((~decided).sum())
        acc = (pred["pred"][l, a] == s["labels"][n:]).mean()
        print(f"n={n} m={m} D={d} gamma={gam:.3e}: kappa {kappa:.1f}, {left_out} of {m} rows left out, smallest gap {gap.min().item():.3f}, "
              f"worst score error / bound {((got - scores).abs() / bound)[decided].max().item():.3e}, accuracy {acc:.3f}")
        assert left_out <= 0.1 * m
        dn = decided.cpu().numpy()
        assert np.array_equal(pred["pred"][l, a][dn], want_pred[dn])
        assert ((got - scores).abs() <= bound)[decided].all()


# ---- the feature's point: a ring's radius -----------------------------------------------------------------------------------------------

def ring(n, d, g):
    x = 0.5 * torch.randn(n, d, generator=g, dtype=torch.float64) + 0.1
    y = torch.randint(0, 3, (n,), generator=g)
    th = 2 * np.pi * torch.rand(n, generator=g, dtype=torch.float64)
    r = 0.5 + 1.5 * y
    x[:, 0] += r * torch.cos(th); x[:, 1] += r * torch.sin(th)
    return x.float(), y


def test_ridge_reads_the_radius_of_a_ring():
    from dbmm_amd import analysis
    n, m, d = 257, 100, 64
    g = torch.Generator().manual_seed(n + d)
    xt, yt = ring(n, d, g)
    xq, yq = ring(m, d, g)
    xt, xq = xt.to(DEV), xq.to(DEV)
    res = analysis.kernel_ridge_probe(xt, yt.numpy(), query=xq, query_labels=yq.numpy(), scales=(4.0,), lams=(1.0,))
    gam = float(res["gammas"][0])
    xa = torch.cat([xt, xq])
    d2 = sq_dists(xa)
    check_preconditions(xa, d2, [gam], "ring")
    freq = torch.as_tensor(np.bincount(yt.numpy(), minlength=3) / n, device=DEV)
    T = torch.nn.functional.one_hot(yt.to(DEV), 3).double() - freq
    A = kernel_f64(d2[:n, :n].clone(), gam) + 2.0 * torch.eye(n, dtype=torch.float64, device=DEV)
    scores, bound, decided, kappa, gap = decided_rows(torch.exp(-gam * d2)[n:, :n], A, T, freq)
    want = scores.argmax(1).cpu().numpy()
    acc64 = (want == yq.numpy()).mean()
    left_out = int((~decided).sum())
    parzen = analysis.kernel_probe(xt, yt.numpy(), gammas=[gam], query=xq, query_labels=yq.numpy())
    print(f"ring: kappa {kappa:.1f}, {left_out} of {m} rows left out, ridge accuracy {res['accuracy'][0, 0]:.3f} (float64 {acc64:.3f}), "
          f"iterations {res['iterations'].tolist()}, Parzen probe accuracy on the same rows {parzen['accuracy'][0]:.3f}")
    assert res["converged"].all() and left_out <= 0.1 * m
    dn = decided.cpu().numpy()
    assert np.array_equal(res["pred"][0, 0][dn], want[dn])
    assert abs(res["accuracy"][0, 0] - acc64) <= left_out / m + 1e-12
    assert res["best"]["index"] == (0, 0) and res["held_out"] is None


# ---- kernel_ridge_probe without a query, ridge_report ----------------------------------------------------------------------------------

def test_probe_without_a_query_is_made_of_the_direct_calls():
    from dbmm_amd import analysis, ops
    n, d = 400, 64
    x, cluster = clustered_rows(n, d, 41)
    labels = 10 + 3 * cluster.numpy()                                   # any integers
    res = analysis.kernel_ridge_probe(x, labels, holdout=0.25, seed=5, scales=(1.0, 4.0))
    uniq, dense = np.unique(labels, return_inverse=True)
    keep, held = analysis.stratified_holdout(dense, 0.25, 5)
    assert np.array_equal(res["held_out"], held) and len(np.intersect1d(keep, held)) == 0
    fit = analysis.kernel_ridge_fit(ops.gather_rows(x, torch.from_numpy(keep).to(DEV)), labels[keep], scales=(1.0, 4.0))
    pr = analysis.kernel_ridge_predict(fit, ops.gather_rows(x, torch.from_numpy(held).to(DEV)))
    assert np.array_equal(res["pred"], pr["pred"]) and np.array_equal(res["scores"], pr["scores"]) and np.array_equal(res["margin"], pr["margin"])
    assert np.array_equal(res["residual"], fit["residual"]) and np.array_equal(res["iterations"], fit["iterations"])
    acc = (pr["pred"] == labels[held]).mean(axis=2)
    print(f"hold-out of {len(held)} rows: accuracy\n{res['accuracy']}\nbest {res['best']}")
    assert res["accuracy"].shape == (2, 2) and np.array_equal(res["accuracy"], acc)
    assert res["recall"].shape == (2, 2, 4) and res["balanced_accuracy"].shape == (2, 2)
    assert res["best"] == analysis._ridge_best(res["balanced_accuracy"], res["gammas"], res["lams"])
    again = analysis.kernel_ridge_probe(x, labels, holdout=0.25, seed=5, scales=(1.0, 4.0))
    assert np.array_equal(again["scores"], res["scores"]), "two runs differ in bits"


def test_ridge_report_is_made_of_the_direct_calls():
    from dbmm_amd import analysis, ops, synth, trainer
    D, seed = 256, 21
    tables = []
    for split, n in (("train", 700), ("val", 400), ("test", 500)):
        x, y, c = synth.embedding_dataset(seed, split, n, D)
        tables.append(trainer.EmbeddingTable(x, y.numpy(), c.numpy()))
    kw = dict(scales=(1.0,), lams=(1.0,))
    rep = analysis.ridge_report(*tables, **kw)
    assert list(rep) == ["val", "test"]
    train = tables[0]
    xt, yt, ct = train.embeddings.float().contiguous(), train.targets.cpu().numpy(), train.targets_spurious.cpu().numpy()
    for split, table in zip(rep, tables[1:]):
        r = rep[split]
        assert set(r) == {"spurious", "spurious_within_class", "best"} and sorted(r["spurious_within_class"]) == [0, 1]
        xq, yq, cq = table.embeddings.float().contiguous(), table.targets.cpu().numpy(), table.targets_spurious.cpu().numpy()
        direct = analysis.kernel_ridge_probe(xt, ct, query=xq, query_labels=cq, **kw)
        print(f"{split}: spurious {r['spurious'].tolist()}, within class {[(k, v.tolist()) for k, v in r['spurious_within_class'].items()]}")
        assert r["spurious"].shape == (1, 1) and np.array_equal(r["spurious"], direct["balanced_accuracy"]) and r["best"] == direct["best"]
        for cls in (0, 1):
            it, iq = np.flatnonzero(yt == cls), np.flatnonzero(yq == cls)
            sub = lambda rows_, idx: ops.gather_rows(rows_, torch.from_numpy(idx).to(DEV))
            direct = analysis.kernel_ridge_probe(sub(xt, it), ct[it], query=sub(xq, iq), query_labels=cq[iq], **kw)
            assert np.array_equal(r["spurious_within_class"][cls], direct["balanced_accuracy"])
        assert ((r["spurious"] >= 0) & (r["spurious"] <= 1)).all()
    scaled = analysis.ridge_report(*tables, transform=lambda r: 3.0 * r, **kw)
    assert scaled["val"]["spurious"].shape == (1, 1)
    # a class with one place only in train: nan, nothing raised
    x, y, c = synth.embedding_dataset(seed, "train", 300, D)
    c = torch.where(y == 1, torch.ones_like(c), c)
    one = trainer.EmbeddingTable(x, y.numpy(), c.numpy())
    r = analysis.ridge_report(one, one, one, **kw)["val"]
    assert np.isnan(r["spurious_within_class"][1]).all() and np.isfinite(r["spurious_within_class"][0]).all()


# ---- scale ------------------------------------------------------------------------------------------------------------------------------

def test_scale_without_an_n_by_n_buffer():
    from dbmm_amd import ops
    n, d, C = 20000, 64, 4
    x = rows(n, d, 80)
    v = torch.randn(n, C, generator=torch.Generator().manual_seed(81)).to(DEV)
    gam = ladder("iso", d)[1]
    center = x.mean(0)
    inputs = x.numel() * 4 + v.numel() * 4
    workspace = n * 2 * 128 * 2 + n * 8 + 16 * n * C * 8               # the documented rule: planes (Dp = 128), 8 bytes per row, 16 partials
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    R = ops.pairdist_rbf_matvec(x, v, center, gam)
    torch.cuda.synchronize()
    extra = torch.cuda.max_memory_allocated() - base
    print(f"N={n}: peak extra memory {extra / 2**20:.1f} MB for {inputs / 2**20:.1f} MB of inputs and {workspace / 2**20:.1f} MB of workspace "
          f"(N x N fp32 would be {n * n * 4 / 2**20:.0f} MB)")
    assert extra < workspace + n * C * 8 + (16 << 20) < n * n * 4 / 8
    xc = x.double() - x.double().mean(0)
    worst = 2.0 * (xc ** 2).sum(1).max().item()
    print(f"N={n}: gamma * max(|a|^2 + |b|^2) = {gam * worst:.2f} (<= 64), so gamma * max d^2 <= {2 * gam * worst:.2f} (<= 80)")
    assert gam * worst <= 64.0 and 2.0 * gam * worst <= 80.0           # d^2 <= 2 (|a|^2 + |b|^2)
    sample = torch.randperm(n, generator=torch.Generator().manual_seed(82))[:512].to(DEV)
    K = torch.exp(-gam * sq_dists(x[sample], x))
    K[torch.arange(512, device=DEV), sample] = 0.0
    check_product(R[sample], K, v, f"N={n} C={C}, 512 sampled rows")
