"""Linear concept erasure, the host half: analysis.erasure_from_moments against a float64 restatement of the formulas (written here,
numpy only), with the moments taken in numpy from synth.embedding_dataset, and analysis.balanced_rows.  No GPU.

The restatement.  Rows x_i, dense labels z_i in G classes, mu the mean, Sxx = (1/N) sum (x - mu)(x - mu)^T, Sxz [D, G] with column
g = (1/N) sum_{i: z_i = g} (x_i - mu).
  leace  W = Sxx^(-1/2), Wp = Sxx^(1/2) from one eigh (eigenvalues below D eps lambda_max dropped); U = the left singular vectors of
         W Sxz above 1e-10 sigma_max; A = (W U)^T, B = (Wp U)^T.
  orth   U = the left singular vectors of Sxz above 1e-10 sigma_max; A = B = U^T.
Both erase by r(x) = x - sum_k ((x - mu) . A_k) B_k = x - P (x - mu) with P = B^T A, which does not depend on the basis U chosen."""
import numpy as np
import pytest

from dbmm_amd import analysis, synth

# (D, N, seed): N = 259 and 1027 are odd and above D, N = 40 is below D (the pseudo-inverse); the seeds give every group two rows
SHAPES = [(64, 259, 4), (512, 1027, 4), (128, 40, 4)]
CASES = [(D, N, seed, G, method) for D, N, seed in SHAPES for G in (2, 4) for method in ("leace", "orth")]
IDS = [f"d{D}_n{N}_g{G}_{m}" for D, N, _, G, m in CASES]


def dataset(D, N, seed, G):
    """(rows float64 [N, D] holding fp32 values, dense labels int64 [N]): the spurious attribute (G = 2) or the groups (G = 4)"""
    x, y, c = synth.embedding_dataset(seed, "train", N, D)
    labels = (c if G == 2 else 2 * y + c).numpy().astype(np.int64)
    assert (np.bincount(labels, minlength=G) >= 2).all()
    return x.numpy().astype(np.float64), labels


def moments64(x, labels, center=None):
    """(scatter about `center` (default: the mean), center, mean, n, label_sums, counts) in numpy float64"""
    n = x.shape[0]
    mean = x.sum(0) / n
    center = mean if center is None else np.asarray(center, dtype=np.float64)
    xc = x - center
    G = int(labels.max()) + 1
    sums = np.stack([x[labels == g].sum(0) for g in range(G)])
    return xc.T @ xc, center, mean, n, sums, np.bincount(labels, minlength=G)


def restated_fit(x, labels, method):
    """(mu, A, B, r, singular values) by the formulas of the module docstring, float64"""
    n, D = x.shape
    G = int(labels.max()) + 1
    mu = x.mean(0)
    xc = x - mu
    Sxx = xc.T @ xc / n
    Sxz = np.stack([xc[labels == g].sum(0) / n for g in range(G)], axis=1)
    if method == "leace":
        lam, V = np.linalg.eigh(Sxx)
        keep = lam > D * np.finfo(np.float64).eps * lam.max()
        lam, V = lam[keep], V[:, keep]
        W, Wp = V @ np.diag(lam ** -0.5) @ V.T, V @ np.diag(lam ** 0.5) @ V.T
        U, s, _ = np.linalg.svd(W @ Sxz, full_matrices=False)
        r = int((s > 1e-10 * s.max()).sum())
        return mu, (W @ U[:, :r]).T, (Wp @ U[:, :r]).T, r, s
    U, s, _ = np.linalg.svd(Sxz, full_matrices=False)
    r = int((s > 1e-10 * s.max()).sum())
    return mu, U[:, :r].T, U[:, :r].T, r, s


def apply64(x, mu, A, B):
    """r(x) in float64 on whatever vectors are given (fp32 ones are promoted exactly)"""
    mu, A, B = (np.asarray(v, dtype=np.float64) for v in (mu, A, B))
    return x - ((x - mu) @ A.T) @ B


def mean_gap(x, labels):
    """the largest |entry| of (a label's mean - the overall mean), float64"""
    mu = x.mean(0)
    return max(np.abs(x[labels == g].mean(0) - mu).max() for g in np.unique(labels))


@pytest.fixture(scope="module")
def fitted():
    """per case: the rows, labels, the restatement and the code's float64 vectors and public fit, computed once"""
    cache = {}

    def get(D, N, seed, G, method):
        key = (D, N, seed, G, method)
        if key not in cache:
            x, labels = dataset(D, N, seed, G)
            m = moments64(x, labels)
            cache[key] = (x, labels, restated_fit(x, labels, method), analysis._erasure_vectors64(*m, method),
                          analysis.erasure_from_moments(*m, method=method))
        return cache[key]
    return get


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_fit_matches_the_restatement(case, fitted):
    D, N, seed, G, method = case
    x, labels, (mu, A, B, r, s), (mean64, A64, B64, sv64), fit = fitted(*case)
    assert r == G - 1 and fit["rank"] == G - 1 and fit["method"] == method
    assert fit["A"].shape == (r, D) and fit["B"].shape == (r, D) and fit["mean"].shape == (D,)
    assert fit["A"].dtype == np.float32 and fit["B"].dtype == np.float32 and fit["mean"].dtype == np.float32
    assert fit["singular_values"].shape == (G,) and fit["singular_values"].dtype == np.float64
    # the public fit is the float32 rounding of the float64 vectors
    assert (fit["A"] == A64.astype(np.float32)).all() and (fit["B"] == B64.astype(np.float32)).all()
    assert (fit["mean"] == mean64.astype(np.float32)).all()
    # the eraser x -> x - P (x - mu) is the restatement's: P = B^T A does not depend on the basis of the column space.  Two float64
    # evaluations of the same formulas differ by the conditioning of the whitening: cond(W) eps, with a factor 1e3 for the products
    P, P64 = B.T @ A, B64.T @ A64
    lam = np.linalg.eigvalsh(np.cov(x.T, bias=True))
    lam = lam[lam > D * np.finfo(np.float64).eps * lam.max()]
    tol = 1e3 * np.finfo(np.float64).eps * (np.sqrt(lam.max() / lam.min()) if method == "leace" else 1.0) * np.abs(P).max()
    print(case, "max |P - P_restated|", np.abs(P64 - P).max(), "allowed", tol, "singular values", sv64)
    assert np.abs(P64 - P).max() <= tol
    assert np.allclose(sv64[:r], s[:r], rtol=1e-9, atol=0) and np.abs(mean64 - mu).max() <= 1e-15 * np.abs(x).max() * 4
    assert (sv64[r:] <= 1e-10 * sv64[0]).all()


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_erased_rows_carry_no_linear_trace_of_the_labels(case, fitted):
    D, N, seed, G, method = case
    x, labels, _, (mean64, A64, B64, _), fit = fitted(*case)
    big = np.abs(x).max()
    before = mean_gap(x, labels)
    e = apply64(x, mean64, A64, B64)
    after = mean_gap(e, labels)
    rounded = mean_gap(apply64(x, fit["mean"], fit["A"], fit["B"]), labels)
    print(case, f"label-mean gap {before:.3e} -> {after:.3e} (float64 vectors), {rounded:.3e} (the fit's fp32 vectors); largest entry {big:.3f}")
    assert before > 1e-2
    assert after <= 1e-12 * big                                      # every label's mean is the overall mean
    assert rounded <= 1e-6 * big                                     # (fp32 vectors: 2^-24 of the entries, with D terms' room)
    assert np.abs(e.mean(0) - x.mean(0)).max() <= 1e-12 * big        # the overall mean stays
    # least squares of the one-hot labels on the erased rows with an intercept: the minimum-norm weights solve S w = g with
    # S = Ec^T Ec and g = Ec^T Zc, whose column for label h is n_h (mean_h - mean) of the erased rows: |g| <= n 1e-12 big per entry,
    # so ||w||_2 <= sqrt(D) n 1e-12 big / (the smallest eigenvalue of S that lstsq keeps)
    ec = e - e.mean(0)
    Z = np.eye(G)[labels]
    w, _, rank, sing = np.linalg.lstsq(ec, Z - Z.mean(0), rcond=None)
    kept = sing[sing > np.finfo(np.float64).eps * max(N, D) * sing.max()]
    allowed = np.sqrt(D) * N * 1e-12 * big / kept.min() ** 2
    print(case, "largest regression weight", np.abs(w).max(), "allowed", allowed, "rank", rank)
    assert np.linalg.norm(w, axis=0).max() <= allowed
    w0 = np.linalg.lstsq(x - x.mean(0), Z - Z.mean(0), rcond=None)[0]
    assert np.abs(w0).max() > 1e6 * allowed                          # the rows before had plenty


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_refit_on_erased_rows_has_rank_zero(case, fitted):
    D, N, seed, G, method = case
    x, labels, _, (mean64, A64, B64, _), fit = fitted(*case)
    for vectors in ((mean64, A64, B64), (fit["mean"], fit["A"], fit["B"])):       # float64 vectors; the fit's own fp32 vectors
        e = apply64(x, *vectors)
        again = analysis.erasure_from_moments(*moments64(e, labels), method=method)
        print(case, "refit singular values", again["singular_values"])
        assert again["rank"] == 0 and again["A"].shape == (0, D) and again["B"].shape == (0, D)
        assert (apply64(e, again["mean"], again["A"], again["B"]) == e).all()


@pytest.mark.parametrize("method", ["leace", "orth"])
def test_scatter_about_another_centre_gives_the_same_fit(method):
    x, labels = dataset(64, 259, 4, 4)
    at_mean = analysis.erasure_from_moments(*moments64(x, labels), method=method)
    away = x.mean(0) + 0.05 * np.linspace(-1.0, 1.0, 64)
    moved = analysis.erasure_from_moments(*moments64(x, labels, center=away), method=method)
    assert moved["rank"] == at_mean["rank"] == 3
    P0 = at_mean["B"].astype(np.float64).T @ at_mean["A"].astype(np.float64)
    P1 = moved["B"].astype(np.float64).T @ moved["A"].astype(np.float64)
    print(method, "max |P difference|", np.abs(P0 - P1).max())
    assert np.abs(P0 - P1).max() <= 2.0 ** -20 * np.abs(P0).max()            # two fp32 roundings of vectors that agree to 1e-12
    assert (moved["mean"] == at_mean["mean"]).all()
    assert np.allclose(moved["singular_values"][:3], at_mean["singular_values"][:3], rtol=1e-9, atol=0)   # (the fourth is rounding)


def test_one_label_and_coinciding_means_are_rank_zero():
    x, labels = dataset(64, 259, 4, 2)
    one = analysis.erasure_from_moments(*moments64(x, np.zeros_like(labels)))
    assert one["rank"] == 0 and one["A"].shape == (0, 64) and one["singular_values"].shape == (1,)
    twice = np.concatenate([x, x])                                           # every row under both labels: the means coincide
    both = np.concatenate([np.zeros(259, dtype=np.int64), np.ones(259, dtype=np.int64)])
    for method in ("leace", "orth"):
        assert analysis.erasure_from_moments(*moments64(twice, both), method=method)["rank"] == 0


@pytest.mark.parametrize("shape", SHAPES, ids=[f"d{D}_n{N}" for D, N, _ in SHAPES])
def test_a_ridge_keeps_the_erasure_exact_and_bounds_the_whitening(shape):
    """with the ridge erasure_fit passes for its fp32-accurate scatter matrix: Wp W is still the identity"""
    D, N, seed = shape
    x, labels = dataset(D, N, seed, 4)
    m = moments64(x, labels)
    ridge = D * analysis.ERASURE_FP32_RIDGE
    mean64, A64, B64, _ = analysis._erasure_vectors64(*m, "leace", ridge)
    plain = analysis._erasure_vectors64(*m, "leace")
    assert A64.shape == (3, D)
    assert mean_gap(apply64(x, mean64, A64, B64), labels) <= 1e-12 * np.abs(x).max()
    top = np.linalg.eigvalsh(np.cov(x.T, bias=True)).max()
    assert np.linalg.norm(A64, axis=1).max() <= (ridge * top) ** -0.5        # rows of (W U)^T: ||W|| ||u||
    change = np.abs(B64.T @ A64 - plain[2].T @ plain[1]).max() / np.abs(plain[2].T @ plain[1]).max()
    print(shape, "relative change of the eraser under the ridge", change)
    assert change <= 0.05                                                    # D 2^-24 lambda_max is far below every kept eigenvalue here
    with pytest.raises(ValueError):
        analysis.erasure_from_moments(*m, ridge=-1.0)


def test_balanced_rows():
    _, labels = dataset(512, 1027, 4, 4)
    counts = np.bincount(labels)
    np.random.seed(5)
    before = np.random.get_state()[1].copy()
    rows = analysis.balanced_rows(labels, seed=3)
    assert (np.random.get_state()[1] == before).all()                        # the global stream is left alone
    assert rows.dtype == np.int64 and (np.diff(rows) > 0).all() and rows.min() >= 0 and rows.max() < 1027
    assert np.bincount(labels[rows], minlength=4).tolist() == [counts.min()] * 4
    assert rows.tolist() == analysis.balanced_rows(labels, seed=3).tolist()
    assert rows.tolist() != analysis.balanced_rows(labels, seed=4).tolist()
    assert rows.tolist() == analysis.balanced_rows(labels + 7, seed=3).tolist()       # any integers: np.unique order
    import torch
    assert rows.tolist() == analysis.balanced_rows(torch.from_numpy(labels), seed=3).tolist()


def test_what_raises():
    x, labels = dataset(64, 259, 4, 2)
    m = moments64(x, labels)
    with pytest.raises(ValueError):
        analysis.erasure_from_moments(*m, method="inlp")
    with pytest.raises(ValueError):                                          # an empty label
        analysis.erasure_from_moments(m[0], m[1], m[2], m[3], np.concatenate([m[4], np.zeros((1, 64))]), np.append(m[5], 0))
    with pytest.raises(ValueError):                                          # n < 2
        analysis.erasure_from_moments(np.zeros((64, 64)), x[0], x[0], 1, x[:1], np.array([1]))
    wide = np.arange(259) % 17                                               # more than 16 labels
    with pytest.raises(ValueError):
        analysis.erasure_from_moments(*moments64(x, wide))
    with pytest.raises(ValueError):
        analysis.erasure_fit(object(), wide, method="inlp")                  # refused before the rows are looked at


# ---- the device's order of the per-label column sums (csrc/label_sums.h), restated ------------------------------------------------------------
def sums_ranges(N, D):
    """(P, rows): the row ranges of the sums kernels from (N, D) alone -- 2048 (range, slab of 256 columns) units aimed at, no range
    below 64 rows, at least one"""
    slabs = -(-D // 256)
    P = max(1, min(-(-2048 // slabs), -(-N // 64)))
    return P, -(-N // P)


def _butterfly(a):
    """lane 0 of the wave's xor butterfly over the last axis (64 lanes)"""
    lanes = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        a = a + a[..., lanes ^ o]
    return a[..., 0]


def fixed_order_sums(x, labels, G):
    """(sums float64 [G, D], counts int64 [G]) of the fp32 rows x added in the device's order: inside a range every label's rows in row
    order (fp32 values are exact in float64; fma(1, v, acc) is acc + v and fma(0, v, acc) leaves acc, so another label's row adds
    + 0 v), each quarter of the ranges in range order, then ((q0 + q1) + q2) + q3.  Vectorised over the ranges; labels outside
    [0, G) are in no sum and no count."""
    N, D = x.shape
    P, rows = sums_ranges(N, D)
    xp = np.zeros((P * rows, D))
    xp[:N] = x
    lp = np.full(P * rows, -1, dtype=np.int64)
    lp[:N] = labels
    xp, lp = xp.reshape(P, rows, D), lp.reshape(P, rows)
    part = np.zeros((P, G, D))
    for i in range(rows):
        w = (lp[:, i, None] == np.arange(G)).astype(np.float64)                  # [P, G]: 1 under label == j, else 0
        part = w[:, :, None] * xp[:, i, None, :] + part
    pq = -(-P // 4)
    quarter = np.zeros((4, G, D))
    for q in range(4):
        for p in range(min(q * pq, P), min(q * pq + pq, P)):
            quarter[q] = quarter[q] + part[p]
    inside = labels[(labels >= 0) & (labels < G)]
    return ((quarter[0] + quarter[1]) + quarter[2]) + quarter[3], np.bincount(inside, minlength=G).astype(np.int64)


def fixed_order_inertia(dmin, D):
    """the float64 sum of the fp32 dmin [N] in the k-means kernels' order: per range a lane adds every 64th row in row order and the
    wave's butterfly folds the lanes; then a lane adds a contiguous run of the ranges in range order and a butterfly folds those"""
    N = dmin.shape[0]
    P, rows = sums_ranges(N, D)
    steps = -(-rows // 64)
    dp = np.zeros((P, steps * 64))
    for p in range(P):
        r0 = min(p * rows, N)
        r1 = min(r0 + rows, N)
        dp[p, :r1 - r0] = dmin[r0:r1]
    lanes = np.zeros((P, 64))
    for k in range(steps):
        lanes = lanes + dp[:, 64 * k:64 * k + 64]
    inert = _butterfly(lanes)
    run = -(-P // 64)
    total = np.zeros(64)
    for lane in range(64):
        for p in range(lane * run, min((lane + 1) * run, P)):
            total[lane] = total[lane] + inert[p]
    return float(_butterfly(total))


@pytest.mark.parametrize("N,D,G", [(1, 64, 1), (259, 64, 3), (1027, 512, 16), (20001, 64, 3)])
def test_fixed_order_sums_are_sums(N, D, G):
    """the restated order against long double, within the bound of the device test: a label's column adds n_g float64 numbers, at
    most n_g - 1 additions round, each by 2^-53 of a partial sum that is at most sum |x|"""
    assert sums_ranges(N, D) == {1: (1, 1), 259: (5, 52), 1027: (17, 61), 20001: (313, 64)}[N]
    rng = np.random.RandomState(N + D)
    x = (rng.standard_normal((N, D)) * 2.0 ** rng.randint(-20, 21, size=(N, 1))).astype(np.float32)   # scales apart: the additions round
    labels = rng.randint(-1, G, size=N).astype(np.int64)                         # -1: in no sum
    sums, counts = fixed_order_sums(x, labels, G)
    chain = np.stack([np.add.reduce(x[labels == g].astype(np.float64), axis=0) for g in range(G)])
    assert N == 1 or (sums != chain).any()                                       # the order shows in the bits: one row-order chain differs
    assert counts.tolist() == [int((labels == g).sum()) for g in range(G)]
    for g in range(G):
        sel = x[labels == g].astype(np.longdouble)
        err = np.abs(sums[g].astype(np.longdouble) - sel.sum(0)).astype(np.float64)
        assert (err <= (counts[g] * 2.0 ** -52 * np.abs(sel).sum(0)).astype(np.float64)).all()
    dmin = np.abs(x[:, 0])
    total = fixed_order_inertia(dmin, D)
    assert abs(total - float(dmin.astype(np.longdouble).sum())) <= N * 2.0 ** -52 * float(dmin.astype(np.float64).sum())
