"""Kernel two-sample (MMD) and HSIC scores on the MI355X: the fused RBF bucket kernel (ops.pairdist_rbf_group_sums) and the statistics
of analysis.mmd / mmd_permutation_test / dependence_report against dense float64: torch.cdist(xd, xd) ** 2 -> exp -> one-hot products.

The 1e-4 relative bound of a bucket sum.  The operands are split into 22 bits under a common scale, so a squared distance is off by
about 3 * 2^-22 = 7e-7 of the centred squared norms |a|^2 + |b|^2 of its two rows.  exp(-gamma d^2) is then off RELATIVELY by gamma
times that, whatever its size; under the precondition gamma_max * max_ij (|a|^2 + |b|^2) <= 64 (centred rows) that is <= 4.5e-5.  What
the exponential adds: c = -gamma log2(e) 2^-2s and the product c d^2 are rounded to fp32 (2^-24 relative each) and the hardware exp2
is good to an ulp, so with |c d^2| = log2(e) gamma d^2 <= 116 (second precondition below) the argument is off by <= 2 * 116 * 2^-24
= 1.4e-5, the value by ln 2 of that, 1e-5 relative.  Together < 6e-5, and a sum of non-negative terms cannot be worse than its worst
term.  The second precondition, gamma_max * max d^2 <= 80, keeps every kernel value above fp32's smallest normal number (e^-80 =
2^-115): below it the hardware exponential returns 0 -- the right answer for a sum that holds anything larger, but not to 1e-4 of a
bucket that holds nothing else.  Both preconditions are asserted on every test's own inputs, in float64; the ladders below are chosen
so that they hold.  Buckets of fewer than 1000 pairs are measured against the whole sum.  Every test prints its figures before it asserts.

An MMD^2 is a difference of three kernel means, each good to 1e-4 relative: the bound there is 1e-4 * (k_aa + k_bb + 2 k_ab) absolute."""
import numpy as np
import pytest
import torch

from pairdist_cases import ISO_SCALES, SPREAD, check_preconditions, clustered_rows, ladder, rows, sq_dists

pytestmark = pytest.mark.gpu

RTOL = 1e-4


def bucket_sums_f64(d2, groups, G, gammas):
    """K [L, G, G] from float64 squared distances: (K, number of pairs per bucket)"""
    n = d2.shape[0]
    onehot = (groups.unsqueeze(0) == torch.arange(G, device=d2.device).unsqueeze(1)).double()      # [G, N]
    upper = torch.triu(torch.ones(n, n, dtype=torch.float64, device=d2.device), 1)
    out = []
    for gam in gammas:
        T = onehot @ (torch.exp(-gam * d2) * upper) @ onehot.T
        out.append(T + T.T - torch.diag(torch.diag(T)))
    cnt = onehot.sum(1)
    pairs = torch.outer(cnt, cnt)
    pairs[torch.arange(G), torch.arange(G)] = cnt * (cnt - 1) / 2
    return torch.stack(out), pairs


def check_buckets(K, ref, pairs, what):
    worst_all = 0.0
    for l in range(ref.shape[0]):
        S, R = K[l], ref[l]
        total = torch.triu(R).sum()
        err = (S - R).abs()
        tol = torch.where(pairs >= 1000, RTOL * R, RTOL * total)
        worst = (err / R.clamp_min(1e-300)).where(pairs >= 1000, torch.zeros_like(err)).max().item()
        worst_all = max(worst_all, worst)
        print(f"{what} l={l}: worst bucket rel err {worst:.3e}, whole-sum rel err "
              f"{(torch.triu(S).sum() - total).abs().item() / max(total.item(), 1e-300):.3e}, max abs err / total {err.max().item() / max(total.item(), 1e-300):.3e}")
        assert torch.equal(S, S.T), f"{what}: K[{l}] is not symmetric"
        assert (err <= tol).all(), f"{what}: bucket sums of bandwidth {l} off by more than {RTOL}"
        assert (S[pairs == 0] == 0).all(), f"{what}: an empty bucket is not zero"
    return worst_all


def layouts(n, seed):
    g = torch.Generator().manual_seed(seed)
    r = torch.randint(0, 3, (n,), generator=g)
    empty = torch.tensor([0, 1, 3])[r]                                  # group 2 has no rows
    one = r.clone()
    one[n // 2] = 3                                                     # group 3 has one row
    return {"empty_group": empty, "one_row_group": one, "single_group": torch.ones(n, dtype=torch.int64)}


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
        cases["by_cluster"] = cluster                                   # whole buckets of between-cluster pairs: tiny values only
    for name, g in cases.items():
        g = g.cuda()
        for tag, order in (("unsorted", None), ("sorted", torch.argsort(g, stable=True))):
            xs, gs, dd = (x, g, d2) if order is None else (ops.gather_rows(x, order), g[order].contiguous(), d2[order][:, order])
            K = ops.pairdist_rbf_group_sums(xs, gs, 4, center, gammas)
            assert K.shape == (4, 4, 4) and K.dtype == torch.float64 and K.device == x.device
            ref, pairs = bucket_sums_f64(dd, gs, 4, gammas)
            check_buckets(K, ref, pairs, f"N={n} D={d} {kind} {name} {tag}")
            assert torch.equal(K, ops.pairdist_rbf_group_sums(xs, gs, 4, center, gammas)), "two calls on the same input differ"
            for l, gam in enumerate(gammas):
                K1 = ops.pairdist_rbf_group_sums(xs, gs, 4, center, [gam])
                assert K1.shape == (1, 4, 4)
                assert torch.equal(K1[0], K[l]), f"bandwidth {l}: L = 1 and L = 4 differ in bits"


def test_sorted_and_unsorted_rows_agree():
    from dbmm_amd import ops
    n, d = 1000, 192
    x = rows(n, d, 79)
    g = torch.randint(0, 4, (n,), generator=torch.Generator().manual_seed(5)).cuda()
    c = x.mean(0)
    gammas = ladder("iso", d)
    K1 = ops.pairdist_rbf_group_sums(x, g, 4, c, gammas)
    order = torch.argsort(g, stable=True)
    K3 = ops.pairdist_rbf_group_sums(ops.gather_rows(x, order), g[order].contiguous(), 4, c, gammas)
    rel = ((K3 - K1).abs() / K1).max().item()
    print(f"sorted vs unsorted: max bucket rel diff {rel:.3e}")
    assert rel <= 1e-6


def test_translation_by_fifty_spreads():
    """the same rows plus a constant vector 50 x their spread: the bound holds because the centre is subtracted first"""
    from dbmm_amd import ops
    n, d = 1000, 1024
    x, _ = clustered_rows(n, d, 77)
    g = torch.randint(0, 4, (n,), generator=torch.Generator().manual_seed(3)).cuda()
    shifted = (x + 50 * SPREAD * torch.ones(d, device="cuda")).contiguous()
    gammas = ladder("clustered", d)
    d2 = sq_dists(shifted)
    check_preconditions(shifted, d2, gammas, "translated")
    K = ops.pairdist_rbf_group_sums(shifted, g, 4, shifted.mean(0), gammas)
    ref, pairs = bucket_sums_f64(d2, g, 4, gammas)
    check_buckets(K, ref, pairs, "translated")


def test_duplicated_rows():
    """1 % duplicated rows: an exact-zero pair has d^2 = the accumulation's rounding and a kernel value within that times gamma
    of 1 -- finite, and the whole sum stays within the bound"""
    from dbmm_amd import ops
    n, d = 1000, 1024
    x = rows(n, d, 78)
    x[n - 10:] = x[:10]
    g = torch.randint(0, 4, (n,), generator=torch.Generator().manual_seed(4)).cuda()
    gammas = ladder("iso", d)
    d2 = sq_dists(x)
    check_preconditions(x, d2, gammas, "duplicates")
    K = ops.pairdist_rbf_group_sums(x, g, 4, x.mean(0), gammas)
    ref, _ = bucket_sums_f64(d2, g, 4, gammas)
    assert torch.isfinite(K).all()
    for l in range(4):
        tot, want = torch.triu(K[l]).sum().item(), torch.triu(ref[l]).sum().item()
        print(f"duplicates l={l}: whole-sum rel err {abs(tot - want) / want:.3e}")
        assert abs(tot - want) <= RTOL * want


# ---- the statistics -------------------------------------------------------------------------------------------------------------

def dense_mmd(d2, labels, gammas, unbiased=True):
    """(mmd2_sum [G, G], its bound [G, G], hsic [L], its bound [L]) in float64 from dense kernels; labels dense in [0, G).  HSIC is
    sum_ab S_ab w_ab / N^2 with S the bucket sums and w = delta_ab - p_a - p_b + sum p^2: its bound is 1e-4 sum_ab S_ab |w_ab| / N^2"""
    n = d2.shape[0]
    G = int(labels.max().item()) + 1
    onehot = (labels.unsqueeze(0) == torch.arange(G, device=d2.device).unsqueeze(1)).double()
    cnt = onehot.sum(1)
    H = torch.eye(n, dtype=torch.float64, device=d2.device) - 1.0 / n
    Lm = onehot.T @ onehot
    total, bound, hsic, hbound = 0.0, 0.0, [], []
    pr = cnt / n
    wabs = (torch.eye(G, dtype=torch.float64, device=d2.device) - pr[:, None] - pr[None, :] + (pr * pr).sum()).abs()
    for gam in gammas:
        Kd = torch.exp(-gam * d2)
        S = onehot @ Kd @ onehot.T                                      # ordered pairs, the diagonal (ones) included
        mean = S / torch.outer(cnt, cnt)
        if unbiased:
            mean[torch.arange(G), torch.arange(G)] = (torch.diag(S) - cnt) / (cnt * (cnt - 1))
        w = torch.diag(mean)
        m2 = w[:, None] + w[None, :] - 2 * mean
        m2[torch.arange(G), torch.arange(G)] = 0.0
        total = total + m2
        bound = bound + RTOL * (w[:, None] + w[None, :] + 2 * mean)
        hsic.append((torch.trace(Kd @ H @ Lm @ H) / n ** 2).item())
        hbound.append(RTOL * (S * wabs).sum().item() / n ** 2)
    return total.cpu().numpy(), bound.cpu().numpy(), np.array(hsic), np.array(hbound)


def test_mmd_matches_the_dense_statistic_and_takes_a_transform():
    from dbmm_amd import analysis
    n, d = 900, 192
    x, cluster = clustered_rows(n, d, 31)
    labels = np.array([10, 20, 30, 30])[cluster.numpy()]                # three labels, any integers; 30 holds two clusters
    for unbiased in (True, False):
        out = analysis.mmd(x, labels, unbiased=unbiased)
        assert out["labels"].tolist() == [10, 20, 30] and out["counts"].sum() == n and out["gammas"].shape == (3,) and out["hsic"].shape == (3,)
        d2 = sq_dists(x)
        check_preconditions(x, d2, out["gammas"].tolist(), "mmd")
        m = d2.sum().item() / (n * (n - 1.0))
        np.testing.assert_allclose(out["gammas"], np.array([0.25, 1.0, 4.0]) / m, rtol=1e-9)
        dense = torch.from_numpy(np.searchsorted(out["labels"], labels)).cuda()
        want, bound, hsic, hbound = dense_mmd(d2, dense, out["gammas"].tolist(), unbiased)
        err = np.abs(out["mmd2_sum"] - want)
        print(f"mmd unbiased={unbiased}: mmd2_sum\n{out['mmd2_sum']}\nmax err {err.max():.3e}, smallest bound {bound.min():.3e}; hsic {out['hsic']} vs {hsic}")
        assert (err <= bound).all()
        assert out["mmd2"].shape == (3, 3, 3) and out["kernel_mean"].shape == (3, 3, 3)
        assert (np.abs(out["hsic"] - hsic) <= hbound).all()
        assert (out["mmd2_sum"][~np.eye(3, dtype=bool)] > 10 * bound.max()).all(), "the clusters are not told apart"
    f = lambda r: 2.0 * r + 1.0
    a, b = analysis.mmd(x, labels, transform=f), analysis.mmd(f(x), labels)
    for key in ("mmd2", "kernel_mean", "mmd2_sum", "hsic", "gammas"):
        assert np.array_equal(a[key], b[key]), key
    with pytest.raises(ValueError):
        analysis.mmd(x, np.zeros(n, dtype=np.int64))
    from dbmm_amd import ops
    with pytest.raises(ops.DbmmUnsupported):
        analysis.mmd(x, np.arange(n) % 9)


# (pooled rows, seed) of the two permutation tests: chosen so that no relabelling's statistic lies within 1e-3 relative of the
# observed one in float64 (the test re-checks it), so p cannot hinge on the kernel's 1e-4
PERM_CASES = {"same": (0.0, 2), "shifted": (0.5, 4)}


@pytest.mark.parametrize("case", list(PERM_CASES))
def test_permutation_test_matches_float64(case):
    """two labels drawn from one distribution, and two whose means differ by half a spread in every coordinate; a third label is
    in the split and is left out of the pool"""
    from dbmm_amd import analysis
    shift, seed = PERM_CASES[case]
    n, d, n_perm = 360, 64, 20
    x = rows(n, d, 500 + seed)
    g = np.arange(n) % 3 + 5                                            # labels 5, 6, 7 interleaved
    x[torch.from_numpy(g == 7).cuda()] += shift * SPREAD
    got = analysis.mmd_permutation_test(x, g, (5, 7), n_perm=n_perm, seed=seed)
    assert set(got) == {"stat", "null", "p"} and got["null"].shape == (n_perm,) and got["null"].dtype == np.float64
    idx = np.flatnonzero((g == 5) | (g == 7))
    xp = x[torch.from_numpy(idx).cuda()]
    labels = (g[idx] == 7).astype(np.int64)
    d2 = sq_dists(xp)
    m = d2.sum().item() / (len(idx) * (len(idx) - 1.0))
    gammas = [s / m for s in (0.25, 1.0, 4.0)]
    check_preconditions(xp, d2, gammas, f"permutation {case}")
    stat, bound, _, _ = dense_mmd(d2, torch.from_numpy(labels).cuda(), gammas)
    rng = np.random.default_rng(seed)
    null, nbound = [], []
    for _ in range(n_perm):
        v, b, _, _ = dense_mmd(d2, torch.from_numpy(labels[rng.permutation(len(labels))]).cuda(), gammas)
        null.append(v[0, 1]); nbound.append(b[0, 1])
    null, nbound = np.array(null), np.array(nbound)
    p = (1.0 + (null >= stat[0, 1]).sum()) / (1.0 + n_perm)
    margin = np.abs(null - stat[0, 1]).min() / abs(stat[0, 1])
    print(f"{case}: stat {got['stat']:.6e} (float64 {stat[0, 1]:.6e}), p {got['p']:.4f} (float64 {p:.4f}), nearest null at {margin:.3e} relative, "
          f"max null err {np.abs(got['null'] - null).max():.3e}, bound {bound[0, 1]:.3e}")
    assert margin > 1e-3, "a relabelling's statistic is a near-tie with the observed one: choose another seed"
    assert abs(got["stat"] - stat[0, 1]) <= bound[0, 1]
    assert (np.abs(got["null"] - null) <= nbound).all()
    assert got["p"] == p
    assert (p == 1.0 / (1.0 + n_perm)) if case == "shifted" else (p > 0.05)
    # fixed bandwidths come through **mmd_kw
    again = analysis.mmd_permutation_test(x, g, (5, 7), n_perm=2, seed=seed, gammas=gammas)
    assert abs(again["stat"] - stat[0, 1]) <= bound[0, 1] and (np.abs(again["null"] - null[:2]) <= nbound[:2]).all()


def test_dependence_report_and_erasure():
    from dbmm_amd import analysis, ops, synth, trainer
    D, seed = 256, 21
    tables = []
    for split, n in (("train", 700), ("val", 400), ("test", 500)):
        x, y, c = synth.embedding_dataset(seed, split, n, D)
        tables.append(trainer.EmbeddingTable(x, y.numpy(), c.numpy()))
    rep = analysis.dependence_report(*tables)
    assert list(rep) == ["train", "val", "test"]
    for split, table in zip(rep, tables):
        r = rep[split]
        assert set(r) == {"group", "spurious_within_class", "hsic_spurious"}
        G = len(np.unique(table.targets_group.cpu().numpy()))
        assert r["group"].shape == (G, G) and r["hsic_spurious"].shape == (3,) and sorted(r["spurious_within_class"]) == [0, 1]
        y, c = table.targets.cpu().numpy(), table.targets_spurious.cpu().numpy()
        for cls in (0, 1):
            idx = np.flatnonzero(y == cls)
            direct = analysis.mmd(ops.gather_rows(table.embeddings.float().contiguous(), torch.from_numpy(idx).cuda()), c[idx])
            assert r["spurious_within_class"][cls] == direct["mmd2_sum"][0, 1]
        assert np.array_equal(r["group"], analysis.mmd(table)["mmd2_sum"])
        assert np.array_equal(r["hsic_spurious"], analysis.mmd(table, c)["hsic"])
    scaled = analysis.dependence_report(*tables, transform=lambda r: 3.0 * r, scales=(1.0,))
    assert scaled["val"]["hsic_spurious"].shape == (1,)
    fit = analysis.erasure_fit(tables[0])                               # the spurious attribute, fitted on train
    erased = analysis.dependence_report(*[analysis.erased_table(t, fit) for t in tables])
    for split in rep:
        before, after = rep[split]["hsic_spurious"][0], erased[split]["hsic_spurious"][0]
        print(f"{split}: hsic_spurious at the widest bandwidth {before:.6e} -> {after:.6e} after erasure; within-class "
              f"{rep[split]['spurious_within_class']} -> {erased[split]['spurious_within_class']}")
    for split in rep:
        assert erased[split]["hsic_spurious"][0] < rep[split]["hsic_spurious"][0]
    # a class with one place only: nan, nothing raised
    x, y, c = synth.embedding_dataset(seed, "train", 300, D)
    c = torch.where(y == 1, torch.ones_like(c), c)
    one = trainer.EmbeddingTable(x, y.numpy(), c.numpy())
    r = analysis.dependence_report(one, one, one)["train"]
    assert np.isnan(r["spurious_within_class"][1]) and np.isfinite(r["spurious_within_class"][0])


def test_scale_without_an_n_by_n_buffer():
    from dbmm_amd import analysis
    n, d = 20000, 1024
    x = rows(n, d, 80)
    g = torch.randint(0, 4, (n,), generator=torch.Generator().manual_seed(6))
    x[(g == 1).cuda()] += 0.05
    m = 2.0 * SPREAD ** 2 * d
    gammas = [s / m for s in ISO_SCALES]                                # L = 4
    inputs = x.numel() * 4 + n * 8
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    out = analysis.mmd(x, g.numpy(), gammas=gammas)
    torch.cuda.synchronize()
    extra = torch.cuda.max_memory_allocated() - base
    print(f"N={n}: peak extra memory {extra / 2**20:.1f} MB for {inputs / 2**20:.1f} MB of inputs (N x N fp32 would be {n * n * 4 / 2**20:.0f} MB)")
    assert extra < 3 * inputs + (64 << 20)
    torch.cuda.reset_peak_memory_stats()
    analysis.mmd(x, g.numpy())                                          # the default ladder: rbf_gammas' two reads on top
    torch.cuda.synchronize()
    extra = torch.cuda.max_memory_allocated() - base
    print(f"N={n}: peak extra memory with the default bandwidths {extra / 2**20:.1f} MB")
    assert extra < 3 * inputs + (64 << 20)
    # float64 reference in row chunks, on centred rows (the Gram form in float64: 1e-16 of the norms)
    gd = g.cuda()
    xd = x.double() - x.double().mean(0)
    sq = (xd ** 2).sum(1)
    assert max(gammas) * 2 * sq.max().item() <= 64.0
    onehot = (gd.unsqueeze(0) == torch.arange(4, device="cuda").unsqueeze(1)).double()
    cnt = onehot.sum(1)
    total, bound, dmax = 0.0, 0.0, 0.0
    for gam in gammas:
        S = torch.zeros(4, 4, dtype=torch.float64, device="cuda")
        for i in range(0, n, 2000):
            d2 = (sq[i:i + 2000, None] + sq[None, :] - 2.0 * xd[i:i + 2000] @ xd.T).clamp_min(0)
            dmax = max(dmax, d2.max().item())
            S += onehot[:, i:i + 2000] @ torch.exp(-gam * d2) @ onehot.T                              # ordered pairs with the diagonal
        mean = S / torch.outer(cnt, cnt)
        mean[torch.arange(4), torch.arange(4)] = (torch.diag(S) - cnt) / (cnt * (cnt - 1))
        w = torch.diag(mean)
        total = total + (w[:, None] + w[None, :] - 2 * mean)
        bound = bound + RTOL * (w[:, None] + w[None, :] + 2 * mean)
    assert max(gammas) * dmax <= 80.0
    err = (torch.from_numpy(out["mmd2_sum"]).cuda() - total).abs()
    err.fill_diagonal_(0)
    print(f"N={n}: mmd2_sum max err {err.max().item():.3e}, smallest bound {bound.min().item():.3e}, mmd2_sum[0, 1] {out['mmd2_sum'][0, 1]:.4e}")
    assert (err <= bound).all()
