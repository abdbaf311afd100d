"""The kernel probe, the MMD witness function and the kernel alignment on the MI355X: the fused RBF row-sum kernel
(ops.pairdist_rbf_row_group_sums) and analysis.kernel_probe / mmd_witness / kernel_alignment / probe_report against dense float64:
torch.cdist(xd, xd) ** 2 -> exp, diagonal zeroed, times a one-hot matrix.

The 1e-4 relative bound of an entry R[l, i, g] is test_gpu_mmd.py's, term by term: the operands are split into 22 bits under a common
scale, so a squared distance is off by about 3 * 2^-22 = 7e-7 of the centred squared norms |a|^2 + |b|^2 of its two rows, and
exp(-gamma d^2) RELATIVELY by gamma times that: <= 4.5e-5 under the precondition gamma_max * max_ij (|a|^2 + |b|^2) <= 64.  The
coefficient and the product c d^2 are rounded to fp32 and the hardware exp2 is good to an ulp: with |c d^2| <= 116 (the second
precondition, gamma_max * max d^2 <= 80, which also keeps every kernel value a normal fp32 number) 1e-5 relative.  The fp32 tree over
a wave's 64 columns adds 6 * 2^-24 = 4e-7.  Together < 6e-5 on every term; the terms are non-negative, so a sum is no worse than its
worst term, however few terms it has.  An entry with no term (an empty label; a label's only row, for its own label; nothing at all
for N = 1) must be exactly 0.  Both preconditions are asserted on every test's own inputs in float64, the generators and ladders
are pairdist_cases.py's, and every test prints its figures before it asserts.

A density is an entry over a count: 1e-4 relative.  A witness value is a difference of two densities: 1e-4 * (density_a +
density_b) absolute.  An MMD^2 is a difference of three kernel means: 1e-4 * (k_aa + k_bb + 2 k_ab) absolute."""
import numpy as np
import pytest
import torch

from pairdist_cases import DEV, GuardedAlloc, ISO_SCALES, SPREAD, check_preconditions, clustered_rows, ladder, onehot, rows, sq_dists

pytestmark = pytest.mark.gpu

RTOL = 1e-4


def row_sums_f64(d2, g, G, gammas):
    """(R [L, N, G], number of terms [N, G]) from square float64 squared distances: the diagonal left out"""
    oh = onehot(g, G)
    off = 1.0 - torch.eye(d2.shape[0], dtype=torch.float64, device=d2.device)
    own = g.unsqueeze(1) == torch.arange(G, device=g.device).unsqueeze(0)
    return torch.stack([(torch.exp(-gam * d2) * off) @ oh for gam in gammas]), oh.sum(0).unsqueeze(0) - own.double()


def check_rows(R, ref, terms, what):
    assert R.shape == ref.shape and R.dtype == torch.float64 and R.device == ref.device
    assert torch.isfinite(R).all()
    live = (terms > 0).unsqueeze(0).expand_as(ref)
    rel = ((R - ref).abs() / ref.clamp_min(1e-300)).where(live, torch.zeros_like(ref))
    worst = rel.max().item() if rel.numel() else 0.0
    print(f"{what}: worst entry rel err {worst:.3e} over {int(live.sum())} entries with a term, smallest such entry {ref[live].min().item() if live.any() else 0.0:.3e}")
    assert (rel <= RTOL).all(), f"{what}: an entry is off by more than {RTOL}"
    assert (R[~live] == 0).all(), f"{what}: an entry without a term is not exactly 0"
    return worst


def layouts(n, seed):
    g = torch.Generator().manual_seed(seed)
    r = torch.randint(0, 3, (n,), generator=g)
    empty = torch.tensor([0, 1, 3])[r]                                  # label 2 has no rows
    one = r.clone()
    one[n // 2] = 3                                                     # label 3 has one row
    return {"empty_label": empty, "one_row_label": one, "single_label": torch.ones(n, dtype=torch.int64)}


# ---- the kernel against float64 -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["iso", "clustered"])
@pytest.mark.parametrize("d", [64, 192, 1024])
@pytest.mark.parametrize("n", [1, 2, 255, 256, 257, 513, 1000])
def test_shapes_layouts_and_bandwidth_counts(n, d, kind):
    """every shape x label layout, rows as drawn (unsorted: predicated tiles) and sorted by label (the fast path); L = 4 in one call
    against float64, and against four L = 1 calls bit for bit; two calls bit-equal"""
    from dbmm_amd import ops
    seed = 1000 * n + d
    if kind == "iso":
        x, cluster = rows(n, d, seed), None
    else:
        x, cluster = clustered_rows(n, d, seed)
    gammas = ladder(kind, d)
    d2 = sq_dists(x)
    check_preconditions(x, d2, gammas, f"N={n} D={d} {kind}")
    center = x.mean(0)
    cases = layouts(n, n + d)
    if cluster is not None:
        cases["by_cluster"] = cluster                                   # whole entries of between-cluster pairs: tiny values only
    worst = 0.0
    for name, g in cases.items():
        g = g.to(DEV)
        for tag, order in (("unsorted", None), ("sorted", torch.argsort(g, stable=True))):
            xs, gs, dd = (x, g, d2) if order is None else (ops.gather_rows(x, order), g[order].contiguous(), d2[order][:, order])
            R = ops.pairdist_rbf_row_group_sums(xs, gs, 4, center, gammas)
            assert R.shape == (4, n, 4)
            ref, terms = row_sums_f64(dd, gs, 4, gammas)
            worst = max(worst, check_rows(R, ref, terms, f"N={n} D={d} {kind} {name} {tag}"))
            assert torch.equal(R, ops.pairdist_rbf_row_group_sums(xs, gs, 4, center, gammas)), "two calls on the same input differ"
            for l, gam in enumerate(gammas):
                R1 = ops.pairdist_rbf_row_group_sums(xs, gs, 4, center, [gam])
                assert R1.shape == (1, n, 4)
                assert torch.equal(R1[0], R[l]), f"bandwidth {l}: L = 1 and L = 4 differ in bits"
    print(f"N={n} D={d} {kind}: worst entry rel err of the case {worst:.3e}")


def test_sixteen_labels():
    from dbmm_amd import ops
    n, d = 1000, 64
    x, _ = clustered_rows(n, d, 11)
    gammas = ladder("clustered", d)
    d2 = sq_dists(x)
    check_preconditions(x, d2, gammas, "G=16")
    for name, g in (("shuffled", torch.randint(0, 16, (n,), generator=torch.Generator().manual_seed(12))),
                    ("sorted", torch.sort(torch.randint(0, 16, (n,), generator=torch.Generator().manual_seed(13))).values),
                    ("label 15 and outside", torch.tensor([15, 16, 3, -1])[torch.arange(n) % 4])):
        g = g.to(DEV)
        R = ops.pairdist_rbf_row_group_sums(x, g, 16, x.mean(0), gammas)
        ref, terms = row_sums_f64(d2, g, 16, gammas)
        check_rows(R, ref, terms, f"G=16 {name}")


def test_labels_outside_are_in_nobodys_sum_and_keep_their_own():
    """-1 and 2^32 + 1 (which is 1 in 32 bits) on every fifth row: those rows' own sums are present, and they are in nobody's"""
    from dbmm_amd import ops
    n, d = 513, 192
    x = rows(n, d, 14)
    gammas = ladder("iso", d)
    d2 = sq_dists(x)
    check_preconditions(x, d2, gammas, "labels outside")
    g = torch.randint(0, 4, (n,), generator=torch.Generator().manual_seed(15))
    out = torch.zeros(n, dtype=torch.bool)
    out[::5] = True
    g[::5] = torch.tensor([-1, (1 << 32) + 1])[torch.arange(len(g[::5])) % 2]
    for tag, order in (("as drawn", torch.arange(n)), ("outside rows last", torch.argsort(torch.where(out, 99, g), stable=True))):
        gs, o = g[order].to(DEV), order.to(DEV)
        xs = ops.gather_rows(x, o)
        R = ops.pairdist_rbf_row_group_sums(xs, gs, 4, x.mean(0), gammas)
        ref, terms = row_sums_f64(d2[o][:, o], gs, 4, gammas)
        check_rows(R, ref, terms, f"labels outside, {tag}")
        outside = out[order].to(DEV)
        assert (R[:, outside].sum(2) > 0).all(), "a row with a label outside lost its own sums"


def test_more_than_sixteen_row_blocks():
    """N = 4500: 18 row blocks, so a unit of the schedule holds several column blocks"""
    from dbmm_amd import ops
    n, d = 4500, 64
    x, cluster = clustered_rows(n, d, 16)
    gammas = ladder("clustered", d)
    d2 = sq_dists(x)
    check_preconditions(x, d2, gammas, "N=4500")
    cluster = cluster.to(DEV)
    for tag, order in (("unsorted", torch.arange(n, device=DEV)), ("sorted", torch.argsort(cluster, stable=True))):
        g = cluster[order].contiguous()
        R = ops.pairdist_rbf_row_group_sums(ops.gather_rows(x, order), g, 4, x.mean(0), gammas)
        ref, terms = row_sums_f64(d2[order][:, order], g, 4, gammas)
        check_rows(R, ref, terms, f"N=4500 by cluster, {tag}")


def test_agrees_with_the_bucket_kernel():
    """the same planes, the same fp32 squared distances, another order of summation: the sum over the rows of label a of R[l, i, b] is
    K[l, a, b], and twice K[l, a, a] on the diagonal (every unordered pair is seen from both ends)"""
    from dbmm_amd import ops
    n, d = 1000, 192
    x = rows(n, d, 21)
    c = x.mean(0)
    gammas = ladder("iso", d)
    r = torch.randint(0, 4, (n,), generator=torch.Generator().manual_seed(22))
    for name, g in (("shuffled", r), ("sorted", torch.sort(r).values)):
        g = g.to(DEV)
        K = ops.pairdist_rbf_group_sums(x, g, 4, c, gammas)
        R = ops.pairdist_rbf_row_group_sums(x, g, 4, c, gammas)
        T = torch.einsum("na,lnb->lab", onehot(g, 4), R)
        want = K + torch.diag_embed(torch.diagonal(K, dim1=1, dim2=2))
        rel = ((T - want).abs() / want).max().item()
        print(f"rows kernel against bucket kernel, {name}: max rel diff {rel:.3e}")
        assert rel <= 1e-6


def test_sorted_and_unsorted_rows_agree():
    from dbmm_amd import ops
    n, d = 1000, 192
    x = rows(n, d, 79)
    g = torch.randint(0, 4, (n,), generator=torch.Generator().manual_seed(5)).to(DEV)
    c = x.mean(0)
    gammas = ladder("iso", d)
    R1 = ops.pairdist_rbf_row_group_sums(x, g, 4, c, gammas)
    order = torch.argsort(g, stable=True)
    R3 = torch.empty_like(R1)
    R3[:, order] = ops.pairdist_rbf_row_group_sums(ops.gather_rows(x, order), g[order].contiguous(), 4, c, gammas)
    rel = ((R3 - R1).abs() / R1).max().item()
    print(f"sorted vs unsorted: max entry rel diff {rel:.3e}")
    assert rel <= 1e-6


def test_translation_by_fifty_spreads():
    """the same rows plus a constant vector 50 x their spread: the bound holds because the centre is subtracted first"""
    from dbmm_amd import ops
    n, d = 1000, 1024
    x, _ = clustered_rows(n, d, 77)
    g = torch.randint(0, 4, (n,), generator=torch.Generator().manual_seed(3)).to(DEV)
    shifted = (x + 50 * SPREAD * torch.ones(d, device=DEV)).contiguous()
    gammas = ladder("clustered", d)
    d2 = sq_dists(shifted)
    check_preconditions(shifted, d2, gammas, "translated")
    R = ops.pairdist_rbf_row_group_sums(shifted, g, 4, shifted.mean(0), gammas)
    ref, terms = row_sums_f64(d2, g, 4, gammas)
    check_rows(R, ref, terms, "translated")


def test_duplicated_rows():
    """1 % duplicated rows: an exact-zero pair has d^2 = the accumulation's rounding (clamped at 0) and a kernel value within gamma
    times that of 1 -- finite, and the whole sums (over the rows, per bandwidth and label) stay within the bound"""
    from dbmm_amd import ops
    n, d = 1000, 1024
    x = rows(n, d, 78)
    x[n - 10:] = x[:10]
    g = torch.randint(0, 4, (n,), generator=torch.Generator().manual_seed(4)).to(DEV)
    gammas = ladder("iso", d)
    d2 = sq_dists(x)
    check_preconditions(x, d2, gammas, "duplicates")
    R = ops.pairdist_rbf_row_group_sums(x, g, 4, x.mean(0), gammas)
    ref, _ = row_sums_f64(d2, g, 4, gammas)
    assert torch.isfinite(R).all()
    rel = ((R.sum(1) - ref.sum(1)).abs() / ref.sum(1))
    print(f"duplicates: whole-sum rel err per (bandwidth, label)\n{rel}")
    assert (rel <= RTOL).all()


def test_nothing_is_written_outside_the_sums_and_the_workspace(monkeypatch):
    """a ragged last block, three labels for a width of three, four bandwidths: the last partial and the last sum are the edges"""
    from dbmm_amd import ops
    n, d = 257, 192
    x = rows(n, d, 25)
    g = torch.randint(0, 3, (n,), generator=torch.Generator().manual_seed(26)).to(DEV)
    c = x.mean(0)
    gammas = ladder("iso", d)
    d2 = sq_dists(x)
    ga = GuardedAlloc()
    monkeypatch.setattr(ops, "_empty", ga)
    R = ops.pairdist_rbf_row_group_sums(x, g, 3, c, gammas)
    torch.cuda.synchronize()
    assert len(ga.bufs) == 2                                                    # workspace, sums
    ga.check()
    ref, terms = row_sums_f64(d2, g, 3, gammas)
    check_rows(R, ref, terms, "guarded N=257 G=3")


def test_the_distance_rows_kernel_is_left_alone():
    """the other instantiation of the templated tile kernel, on one shape of test_gpu_silhouette.py and within its bound (RTOL of
    every entry: d^2 > 1 % of the mean centred squared norm on these rows); bits against the parent build are bench_kernel_probe's"""
    from dbmm_amd import ops
    n, d = 513, 192
    x = rows(n, d, 1000 * n + d)
    g = torch.randint(0, 4, (n,), generator=torch.Generator().manual_seed(n + d)).to(DEV)
    dist = sq_dists(x).sqrt()
    R = ops.pairdist_row_group_sums(x, g, 4, x.mean(0))
    ref = dist @ onehot(g, 4)
    rel = ((R - ref).abs() / ref).max().item()
    print(f"distance rows kernel N={n} D={d}: worst entry rel err {rel:.3e}")
    assert R.shape == (n, 4) and rel <= RTOL
    assert torch.equal(R, ops.pairdist_row_group_sums(x, g, 4, x.mean(0)))


# ---- kernel_probe ---------------------------------------------------------------------------------------------------------------------

def probe_f64(x, dense, G, gammas, prior="uniform", q=None):
    """analysis.parzen_from_sums (tested against the definition in test_kernel_probe_host.py) on float64 sums: leave-one-out over
    the rows x, or the rows q against x"""
    from dbmm_amd import analysis
    g = torch.from_numpy(dense).to(DEV)
    counts = np.bincount(dense, minlength=G)
    if q is None:
        R, _ = row_sums_f64(sq_dists(x), g, G, gammas)
        return analysis.parzen_from_sums(R.cpu().numpy(), dense, counts, prior), counts
    R = torch.stack([torch.exp(-gam * sq_dists(q, x)) @ onehot(g, G) for gam in gammas])
    return analysis.parzen_from_sums(R.cpu().numpy(), np.full(q.shape[0], -1), counts, prior), counts


def scores_f64(pred, true, G):
    hit = pred == true[None]
    recall = np.stack([hit[:, true == g].mean(1) for g in range(G)], axis=1)
    return hit.mean(1), recall, recall.mean(1)


PROBE_LABELS = {"by_cluster": np.array([3, 5, 7, 11]), "three_labels": np.array([10, 20, 30, 30])}     # 30 holds two clusters


@pytest.mark.parametrize("labelling", list(PROBE_LABELS))
@pytest.mark.parametrize("n,d", [(513, 64), (900, 192), (1000, 1024)])
def test_kernel_probe_matches_float64_on_every_row(n, d, labelling):
    from dbmm_amd import analysis
    x, cluster = clustered_rows(n, d, 31 + n)
    labels = PROBE_LABELS[labelling][cluster.numpy()]
    uniq, dense = np.unique(labels, return_inverse=True)
    G = len(uniq)
    for prior in ("uniform", "empirical"):
        out = analysis.kernel_probe(x, labels, prior=prior)
        gammas = out["gammas"].tolist()
        d2 = sq_dists(x)
        check_preconditions(x, d2, gammas, f"kernel_probe N={n} D={d}")
        np.testing.assert_allclose(out["gammas"], np.array([0.25, 1.0, 4.0]) * (n * (n - 1.0)) / d2.sum().item(), rtol=1e-9)
        want, counts = probe_f64(x, dense, G, gammas, prior)
        assert np.array_equal(out["labels"], uniq) and np.array_equal(out["counts"], counts)
        rel = np.abs(out["density"] - want["density"]) / want["density"]
        print(f"kernel_probe N={n} D={d} {labelling} {prior}: smallest float64 margin {np.nanmin(want['margin']):.3e}, worst density rel err {rel.max():.3e}, "
              f"accuracy {out['accuracy']}, balanced {out['balanced_accuracy']}")
        assert np.nanmin(want["margin"]) > 1e-2, "a float64 prediction is a near-tie: the comparison of EVERY row would hinge on rounding"
        assert out["pred"].shape == (3, n) and np.array_equal(out["pred"], uniq[want["pred"]]), "a row's prediction differs from float64's"
        assert (rel <= RTOL).all()
        np.testing.assert_allclose(out["margin"], want["margin"], atol=2.1 * RTOL)      # 1 - top2 / top1, each within RTOL, top2 <= top1
        acc, recall, bal = scores_f64(want["pred"], dense, G)
        assert np.array_equal(out["accuracy"], acc) and np.array_equal(out["recall"], recall) and np.array_equal(out["balanced_accuracy"], bal)
    f = lambda r: 2.0 * r + 1.0
    a, b = analysis.kernel_probe(x, labels, transform=f), analysis.kernel_probe(f(x), labels)
    for key in ("density", "pred", "margin", "gammas", "accuracy", "recall", "balanced_accuracy"):
        assert np.array_equal(a[key], b[key], equal_nan=True), key


def test_query_rows_are_scored_against_the_reference_rows_only():
    from dbmm_amd import analysis, ops
    n, m, d = 700, 300, 192
    x, cluster = clustered_rows(n + m, d, 41)
    labels = PROBE_LABELS["three_labels"][cluster.numpy()]
    ref_x, q = x[:n].contiguous(), x[n:].contiguous()
    uniq, dense = np.unique(labels[:n], return_inverse=True)
    out = analysis.kernel_probe(ref_x, labels[:n], query=q, query_labels=labels[n:])
    gammas = out["gammas"].tolist()
    d2 = sq_dists(x)
    check_preconditions(x, d2, gammas, "query")
    np.testing.assert_allclose(out["gammas"], np.array([0.25, 1.0, 4.0]) * (n * (n - 1.0)) / d2[:n, :n].sum().item(), rtol=1e-9)     # the reference rows' own
    want, counts = probe_f64(ref_x, dense, 3, gammas, q=q)
    rel = np.abs(out["density"] - want["density"]) / want["density"]
    print(f"query: smallest float64 margin {np.nanmin(want['margin']):.3e}, worst density rel err {rel.max():.3e}, accuracy {out['accuracy']}")
    assert np.nanmin(want["margin"]) > 1e-2
    assert out["density"].shape == (3, m, 3) and (rel <= RTOL).all()
    assert np.array_equal(out["pred"], uniq[want["pred"]])
    acc, recall, bal = scores_f64(want["pred"], np.searchsorted(uniq, labels[n:]), 3)
    assert np.array_equal(out["accuracy"], acc) and np.array_equal(out["recall"], recall) and np.array_equal(out["balanced_accuracy"], bal)
    assert "accuracy" not in analysis.kernel_probe(ref_x, labels[:n], query=q)
    # the reference rows' own sums with and without the query rows behind them: not equal in bits by construction (the centre is the
    # mean of what is passed, and the schedule's chunks follow the number of row blocks), so 1e-6
    order = np.argsort(dense, kind="stable")
    xs = ops.gather_rows(ref_x, torch.from_numpy(order).to(DEV))
    gs = torch.from_numpy(dense[order]).to(DEV)
    alone = ops.pairdist_rbf_row_group_sums(xs, gs, 3, xs.mean(0), gammas)
    both = torch.cat([xs, q])
    with_q = ops.pairdist_rbf_row_group_sums(both, torch.cat([gs, torch.full((m,), -1, dtype=torch.int64, device=DEV)]), 3, both.mean(0), gammas)
    diff = ((with_q[:, :n] - alone).abs() / alone).max().item()
    print(f"reference rows with and without queries: max entry rel diff {diff:.3e}")
    assert diff <= 1e-6


# ---- mmd_witness ------------------------------------------------------------------------------------------------------------------------

def test_mmd_witness_matches_float64():
    from dbmm_amd import analysis
    # the draw was chosen in float64 on the CPU among fifteen seeds: here the 8-th and 9-th witness values of every bandwidth and
    # side are more than 5 bounds apart (most draws have a pair within one bound somewhere; the test re-checks its own)
    n, d, k = 400, 64, 8
    x, cluster = clustered_rows(n, d, 63)
    labels = PROBE_LABELS["three_labels"][cluster.numpy()]
    out = analysis.mmd_witness(x, labels, (30, 10), top_k=k)
    idx = np.flatnonzero((labels == 30) | (labels == 10))
    assert np.array_equal(out["rows"], idx) and out["witness"].shape == (3, len(idx))
    xp = x[torch.from_numpy(idx).to(DEV)].contiguous()
    lab = (labels[idx] == 10).astype(np.int64)
    gammas = out["gammas"].tolist()
    d2 = sq_dists(xp)
    check_preconditions(xp, d2, gammas, "witness")
    want, counts = probe_f64(xp, lab, 2, gammas)
    dens = want["density"]
    w64, bound = dens[:, :, 0] - dens[:, :, 1], RTOL * (dens[:, :, 0] + dens[:, :, 1])
    err = np.abs(out["witness"] - w64)
    print(f"witness: max err / bound {(err / bound).max():.3e}")
    assert (err <= bound).all()
    both = analysis.mmd(xp, lab, gammas=gammas)
    a_rows, b_rows = lab == 0, lab == 1                                 # the kernel means of float64: the MMD bound's three terms
    k_aa, k_bb, k_ab = dens[:, a_rows, 0].mean(1), dens[:, b_rows, 1].mean(1), dens[:, a_rows, 1].mean(1)
    mbound = RTOL * (k_aa + k_bb + 2 * k_ab)
    m64 = w64[:, a_rows].mean(1) - w64[:, b_rows].mean(1)
    print(f"witness mmd2 {out['mmd2']} against mmd's {both['mmd2'][:, 0, 1]} and float64's {m64}, bound {mbound}")
    np.testing.assert_allclose(m64, k_aa + k_bb - 2 * k_ab, rtol=1e-9)  # the identity, in float64
    assert (np.abs(out["mmd2"] - both["mmd2"][:, 0, 1]) <= mbound).all()
    assert (np.abs(out["mmd2"] - m64) <= mbound).all()
    for l in range(3):
        for key, sign in (("largest", -1.0), ("smallest", 1.0)):
            o = np.argsort(sign * w64[l], kind="stable")
            gap = abs(w64[l][o[k]] - w64[l][o[k - 1]])
            print(f"witness l={l} {key}: the {k}-th and {k + 1}-th values are {gap:.3e} apart, bounds {bound[l][o[k - 1]]:.3e} + {bound[l][o[k]]:.3e}")
            assert gap > bound[l][o[k - 1]] + bound[l][o[k]], "float64 does not separate the top k from the rest: choose another draw"
            assert np.array_equal(np.sort(out["top"][key][l]), np.sort(idx[o[:k]])), f"top {key} rows of bandwidth {l} differ from float64's"
    with pytest.raises(ValueError):
        analysis.mmd_witness(x, labels, (10, 10))


# ---- kernel_alignment -----------------------------------------------------------------------------------------------------------------

def alignment_f64(d2, dense, G, gammas):
    """(alignment, rel_bound) per bandwidth from dense float64 matrices: the traces, and the first-order propagation of the
    kernels' 1e-4 through them, term by term"""
    n = d2.shape[0]
    oh = onehot(torch.from_numpy(dense).to(d2.device), G)
    H = torch.eye(n, dtype=torch.float64, device=d2.device) - 1.0 / n
    Lm = oh @ oh.T
    p = oh.sum(0) / n
    wabs = (torch.eye(G, dtype=torch.float64, device=d2.device) - p[:, None] - p[None, :] + (p * p).sum()).abs()
    ll = torch.trace(Lm @ H @ Lm @ H).item()
    al, rb = [], []
    for gam in gammas:
        Kd = torch.exp(-gam * d2)
        kl, kk = torch.trace(Kd @ H @ Lm @ H).item(), torch.trace(Kd @ H @ Kd @ H).item()
        al.append(kl / np.sqrt(kk * ll))
        A, B, C = (Kd ** 2).sum().item(), (Kd.sum(1) ** 2).sum().item(), Kd.sum().item()
        b_kl = RTOL * ((oh.T @ Kd @ oh) * wabs).sum().item()
        b_kk = RTOL * (A + 4 * B / n + 2 * C * C / n ** 2)
        rb.append(b_kl / abs(kl) + 0.5 * b_kk / kk)
    return np.array(al), np.array(rb)


def test_kernel_alignment_matches_float64_within_its_own_bound():
    from dbmm_amd import analysis
    n, d = 900, 192
    x, cluster = clustered_rows(n, d, 61)
    labels = PROBE_LABELS["three_labels"][cluster.numpy()]
    out = analysis.kernel_alignment(x, labels)
    assert {"alignment", "hsic", "hsic_kk", "hsic_ll", "rel_bound", "gammas", "labels", "counts"} <= set(out)
    gammas = out["gammas"].tolist()
    d2 = sq_dists(x)
    check_preconditions(x, d2, [2.0 * g for g in gammas], "alignment (the second pass runs at 2 gamma)")
    al64, rb64 = alignment_f64(d2, np.unique(labels, return_inverse=True)[1], 3, gammas)
    print(f"alignment {out['alignment']} against float64 {al64}; rel_bound {out['rel_bound']} against float64 {rb64}")
    assert (rb64 <= 0.05).all()
    assert (np.abs(out["alignment"] - al64) <= rb64 * (1 + rb64) * al64).all()
    assert (np.abs(out["rel_bound"] - rb64) <= 0.01 * rb64).all()
    assert (out["alignment"] > 0.75).all(), "the clusters' labels are not aligned with the kernel"
    rand = np.random.RandomState(62).randint(0, 3, n)
    r = analysis.kernel_alignment(x, rand, gammas=gammas)
    print(f"random labels: alignment {r['alignment']}, rel_bound {r['rel_bound']}")
    assert (r["alignment"] < 0.05).all()
    # more than 8 labels: the row sums serve 16
    many = analysis.kernel_alignment(x, np.arange(n) % 12, gammas=gammas)
    assert many["alignment"].shape == (3,) and (many["alignment"] < 0.05).all()


# ---- probe_report ---------------------------------------------------------------------------------------------------------------------

def test_probe_report_is_made_of_the_direct_calls():
    from dbmm_amd import analysis, ops, synth, trainer
    D, seed = 256, 21
    tables = []
    for split, n in (("train", 700), ("val", 400), ("test", 500)):
        x, y, c = synth.embedding_dataset(seed, split, n, D)
        tables.append(trainer.EmbeddingTable(x, y.numpy(), c.numpy()))
    rep = analysis.probe_report(*tables)
    assert list(rep) == ["train", "val", "test"]
    train = tables[0]
    for split, table in zip(rep, tables):
        r = rep[split]
        assert set(r) == {"group", "spurious_within_class", "spurious_alignment"} | (set() if split == "train" else {"spurious_from_train"})
        assert r["group"].shape == (3,) and r["spurious_alignment"].shape == (3,) and sorted(r["spurious_within_class"]) == [0, 1]
        y, c = table.targets.cpu().numpy(), table.targets_spurious.cpu().numpy()
        rows_ = table.embeddings.float().contiguous()
        for cls in (0, 1):
            idx = np.flatnonzero(y == cls)
            direct = analysis.kernel_probe(ops.gather_rows(rows_, torch.from_numpy(idx).to(DEV)), c[idx])
            assert np.array_equal(r["spurious_within_class"][cls], direct["balanced_accuracy"])
        assert np.array_equal(r["group"], analysis.kernel_probe(table)["balanced_accuracy"])
        assert np.array_equal(r["spurious_alignment"], analysis.kernel_alignment(table, c)["alignment"])
        if split != "train":
            direct = analysis.kernel_probe(train.embeddings, train.targets_spurious.cpu().numpy(), query=rows_, query_labels=c)
            assert np.array_equal(r["spurious_from_train"], direct["balanced_accuracy"])
            assert ((r["spurious_from_train"] >= 0) & (r["spurious_from_train"] <= 1)).all()
    scaled = analysis.probe_report(*tables, transform=lambda r: 3.0 * r, scales=(1.0,))
    assert scaled["val"]["group"].shape == (1,) and scaled["test"]["spurious_from_train"].shape == (1,)
    fit = analysis.erasure_fit(tables[0])                               # the spurious attribute, fitted on train
    erased = analysis.probe_report(*[analysis.erased_table(t, fit) for t in tables])
    for split in rep:                                                   # printed, not asserted: nobody has measured what LEACE does to a Parzen probe here
        print(f"{split}: spurious_alignment {rep[split]['spurious_alignment']} -> {erased[split]['spurious_alignment']} after erasure; "
              f"within-class {rep[split]['spurious_within_class']} -> {erased[split]['spurious_within_class']}; "
              f"from train {rep[split].get('spurious_from_train')} -> {erased[split].get('spurious_from_train')}")
    # a class with one place only: nan, nothing raised
    x, y, c = synth.embedding_dataset(seed, "train", 300, D)
    c = torch.where(y == 1, torch.ones_like(c), c)
    one = trainer.EmbeddingTable(x, y.numpy(), c.numpy())
    r = analysis.probe_report(one, one, one)["train"]
    assert np.isnan(r["spurious_within_class"][1]).all() and np.isfinite(r["spurious_within_class"][0]).all()


# ---- scale ----------------------------------------------------------------------------------------------------------------------------

def test_scale_without_an_n_by_n_buffer():
    from dbmm_amd import analysis
    n, d, G = 20000, 1024, 4
    x = rows(n, d, 80)
    g = torch.randint(0, G, (n,), generator=torch.Generator().manual_seed(6))
    x[(g == 1).to(DEV)] += 0.05
    m = 2.0 * SPREAD ** 2 * d
    gammas = [s / m for s in ISO_SCALES]                                # L = 4
    inputs = x.numel() * 4 + n * 8
    partials = 16 * len(gammas) * n * G * 8                             # the documented workspace rule: sized for 16 chunks, times L
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    out = analysis.kernel_probe(x, g.numpy(), gammas=gammas)
    torch.cuda.synchronize()
    extra = torch.cuda.max_memory_allocated() - base
    print(f"N={n}: peak extra memory {extra / 2**20:.1f} MB for {inputs / 2**20:.1f} MB of inputs and {partials / 2**20:.1f} MB of partials "
          f"(N x N fp32 would be {n * n * 4 / 2**20:.0f} MB)")
    assert extra < 3 * inputs + (64 << 20) + partials
    # float64 reference in row chunks, on centred rows (the Gram form in float64: 1e-16 of the norms)
    gd = g.to(DEV)
    xd = x.double() - x.double().mean(0)
    sq = (xd ** 2).sum(1)
    assert max(gammas) * 2 * sq.max().item() <= 64.0
    oh = onehot(gd, G)
    cnt = oh.sum(0)
    den = cnt.unsqueeze(0) - oh                                          # [N, G]: leave-one-out
    dens = torch.from_numpy(out["density"]).to(DEV)
    dmax, worst = 0.0, 0.0
    for i in range(0, n, 2000):
        d2 = (sq[i:i + 2000, None] + sq[None, :] - 2.0 * xd[i:i + 2000] @ xd.T).clamp_min(0)
        dmax = max(dmax, d2.max().item())
        for l, gam in enumerate(gammas):
            Kd = torch.exp(-gam * d2)
            Kd[torch.arange(Kd.shape[0]), i + torch.arange(Kd.shape[0])] = 0.0
            want = (Kd @ oh) / den[i:i + 2000]
            worst = max(worst, ((dens[l, i:i + 2000] - want).abs() / want).max().item())
    assert max(gammas) * dmax <= 80.0
    print(f"N={n}: worst density rel err {worst:.3e}, accuracy {out['accuracy']}")
    assert worst <= RTOL
