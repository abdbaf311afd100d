"""PCA maps of embedding splits on the MI355X: the fused scatter kernel and the projection kernel against float64, and the
analysis module (pca, pca_project, projection_report) on top of them.

The bounds come from the float64 reference alone.
  scatter      |S - S_ref|[a][b] <= 1e-4 sqrt(S_ref[a][a] S_ref[b][b]): an fp32 chain of at most 1024 products is off by at most
               1024 * 2^-24 = 6.1e-5 of sum |d_a d_b| <= sqrt(S_aa S_bb) (Cauchy-Schwarz); the float64 folds and the 2^-24 roundings of
               the centred inputs are far below that.
  eigenvalues  |l^_j - l_j| <= 1e-4 trace(S_ref): Weyl with ||E||_2 <= ||E||_F <= 1e-4 trace.
  components   sin angle(v^_j, v_j) <= 2e-4 trace(S_ref) / gap_j (Davis-Kahan in the Yu-Wang-Samworth form); the generator keeps
               gap_j >= 0.03 trace for the three planted directions (tests/test_pca_host.py asserts it at every shape used here).
  projection   |y - y_ref| <= (D + 8) 2^-24 ||x_i - c|| ||v_k|| per entry.
Every test prints its figures before it asserts."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from test_pca_host import SHAPES, eig_desc, gaps, planted, scatter_f64

pytestmark = pytest.mark.gpu

SCATTER_TOL, EIG_TOL, ANGLE_TOL = 1e-4, 1e-4, 2e-4
EPS = 2.0 ** -24


def spread(D):
    return 4 / np.sqrt(D)


_cache = {}


def case(N, D, offset=2.0):
    """(x float32 numpy, x on the device, float64 mean), made once per shape and left unchanged"""
    key = (N, D, offset)
    if key not in _cache:
        x = planted(N, D, offset) if N >= 3 else planted(37, D, offset)[:N].copy()
        _cache[key] = (x, torch.from_numpy(x).cuda(), x.astype(np.float64).mean(0))
    return _cache[key]


def centers(x, mean, D):
    off = (mean + 0.1 * spread(D) * np.random.RandomState(D).randn(D)).astype(np.float32)
    return {"mean": mean.astype(np.float32), "off_by_0.1_spreads": off}


def check_scatter(S, x, c, what):
    ref = scatter_f64(x, c)
    dg = np.sqrt(np.diag(ref))
    scale = np.outer(dg, dg)
    err = np.abs(S - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        rel = np.where(scale > 0, err / scale, np.where(err > 0, np.inf, 0.0))
    print(f"{what}: worst |S - S_ref| / sqrt(S_aa S_bb) = {rel.max():.3e} (bound {SCATTER_TOL:.0e})")
    assert np.array_equal(S, S.T), f"{what}: scatter is not symmetric to the bit"
    assert (err <= SCATTER_TOL * scale).all(), f"{what}: scatter off by more than the bound"
    return ref


def check_projection(y, x, c, V, what):
    d = x.astype(np.float64) - c.astype(np.float64)
    ref = d @ V.astype(np.float64).T
    D = x.shape[1]
    bound = (D + 8) * EPS * np.outer(np.linalg.norm(d, axis=1), np.linalg.norm(V.astype(np.float64), axis=1))
    err = np.abs(y.astype(np.float64) - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        worst = np.where(bound > 0, err / bound, np.where(err > 0, np.inf, 0.0)).max()
    print(f"{what}: worst |y - y_ref| / bound = {worst:.3e}")
    assert (err <= bound).all(), f"{what}: projection off by more than the bound"


# ---- 1. the scatter kernel against float64 ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("N,D", [(1, 64), (2, 64), (37, 64), (300, 128), (1025, 192), (2085, 192), (20000, 64), (3000, 1024)])
def test_scatter_matches_float64(N, D):
    from dbmm_amd import ops
    if N == 1:
        x = np.zeros((1, D), dtype=np.float32)
        xd, mean = torch.from_numpy(x).cuda(), np.zeros(D)
    else:
        x, xd, mean = case(N, D)
    for name, c in centers(x, mean, D).items():
        cd = torch.from_numpy(c).cuda()
        S = ops.covariance(xd, cd)
        assert S.dtype == torch.float64 and tuple(S.shape) == (D, D)
        check_scatter(S.cpu().numpy(), x, c, f"N={N} D={D} center={name}")
        assert torch.equal(S, ops.covariance(xd, cd)), "two calls on the same input differ"
    if N == 1:
        assert (ops.covariance(xd, torch.zeros(D, device="cuda")) == 0).all()


# ---- 2. centring happens before the products -------------------------------------------------------------------------------------------

def test_translation_by_fifty_spreads():
    """rows 50 spreads away from the origin: uncentred, an fp32 product carries 2500 spreads^2 and loses 2^-24 of THAT, and
    S - N mu mu^T cancels ~2500 to 1; centred on load, the bound holds as it does at the origin"""
    from dbmm_amd import ops
    N, D = 3000, 1024
    x, xd, mean = case(N, D, 50 * spread(D))
    print(f"|mean| / spread = {np.linalg.norm(mean) / spread(D):.1f}")
    for name, c in centers(x, mean, D).items():
        S = ops.covariance(xd, torch.from_numpy(c).cuda())
        check_scatter(S.cpu().numpy(), x, c, f"translated, center={name}")


# ---- 3. guard zones ----------------------------------------------------------------------------------------------------------------------

class GuardedAlloc:
    """stand-in for ops._empty: every output and workspace sits between two sentinel-filled zones"""
    S = -7.0

    def __init__(self):
        self.bufs = []

    def __call__(self, shape, device=None, dtype=torch.float32, **kw):
        shape = (shape,) if isinstance(shape, int) else tuple(shape)
        n = int(np.prod(shape))
        pad = 1 << 16                                                       # elements: a multiple of 16 bytes for every dtype used
        raw = torch.full((n + 2 * pad,), self.S, device=device, dtype=dtype)
        self.bufs.append((raw, pad, n))
        return raw[pad:pad + n].view(shape)

    def check(self):
        assert self.bufs
        for raw, pad, n in self.bufs:
            lo, hi = raw[:pad], raw[pad + n:]
            assert bool((lo == self.S).all()) and bool((hi == self.S).all()), \
                f"guard zone of a {n}-element {raw.dtype} buffer was written: {(lo != self.S).sum().item()} before, {(hi != self.S).sum().item()} after"


@pytest.mark.parametrize("N,D", [(37, 64), (2085, 192)])
def test_nothing_is_written_outside_the_outputs_and_the_workspace(N, D, monkeypatch):
    from dbmm_amd import ops
    x, xd, mean = case(N, D)
    c = mean.astype(np.float32)
    cd = torch.from_numpy(c).cuda()
    ga = GuardedAlloc()
    monkeypatch.setattr(ops, "_empty", ga)
    S = ops.covariance(xd, cd)
    V = np.linalg.qr(np.random.RandomState(1).randn(D, 8))[0].T.astype(np.float32).copy()
    ys = [ops.project_rows(xd, cd, torch.from_numpy(V[:k].copy()).cuda()) for k in (1, 3, 8)]
    torch.cuda.synchronize()
    assert len(ga.bufs) == 5                                                   # workspace, scatter, three y
    ga.check()
    check_scatter(S.cpu().numpy(), x, c, f"guarded N={N} D={D}")
    for k, y in zip((1, 3, 8), ys):
        check_projection(y.cpu().numpy(), x, c, V[:k], f"guarded N={N} D={D} K={k}")


# ---- 4. the projection kernel against float64 ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("K", [1, 2, 3, 8])
@pytest.mark.parametrize("N,D", [(37, 64), (2085, 192), (3000, 1024)])
def test_projection_matches_float64(N, D, K):
    from dbmm_amd import ops
    x, xd, mean = case(N, D)
    c = mean.astype(np.float32)
    V = np.linalg.qr(np.random.RandomState(K).randn(D, K))[0].T.astype(np.float32).copy()
    V[0] *= 3.0                                                              # not unit norm: the bound scales with ||v||
    cd, Vd = torch.from_numpy(c).cuda(), torch.from_numpy(V).cuda()
    y = ops.project_rows(xd, cd, Vd)
    assert y.dtype == torch.float32 and tuple(y.shape) == (N, K)
    check_projection(y.cpu().numpy(), x, c, V, f"N={N} D={D} K={K}")
    # a row's coordinates do not depend on its neighbours: any slice, ragged against the four rows of a wave
    for lo, hi in ((0, 1), (1, N), (5, 18)):
        assert torch.equal(ops.project_rows(xd[lo:hi], cd, Vd), y[lo:hi])


# ---- 5. analysis.pca end to end --------------------------------------------------------------------------------------------------------

def _groups(N, seed=0):
    g = np.random.RandomState(seed).randint(0, 4, N) * 2 + 1                   # labels 1, 3, 5, 7: np.unique order, not dense
    g[0] = 9                                                                    # a one-row group
    return g


@pytest.mark.parametrize("k", [2, 3])
@pytest.mark.parametrize("N,D", SHAPES)
def test_pca_end_to_end(N, D, k):
    from dbmm_amd import analysis
    x, xd, mean = case(N, D)
    g = _groups(N)
    fit = analysis.pca(xd, g, k=k)
    ref = scatter_f64(x, mean)
    w, V = eig_desc(ref)
    trace, gap = w.sum(), gaps(w)
    assert gap[:3].min() >= 0.03 * trace
    e_val = np.abs(fit["explained_variance"] * (N - 1) - w[:k]).max() / trace
    comp = fit["components"].astype(np.float64)
    cosang = np.abs((comp * V[:k]).sum(1)) / np.linalg.norm(comp, axis=1)
    sin = np.sqrt(np.maximum(0.0, 1 - cosang ** 2))
    print(f"N={N} D={D} k={k}: eigenvalue err / trace {e_val:.3e} (bound {EIG_TOL:.0e}); sin angle {sin} (bounds {ANGLE_TOL * trace / gap[:k]})")
    assert e_val <= EIG_TOL
    assert (sin <= ANGLE_TOL * trace / gap[:k]).all()
    assert fit["components"].dtype == np.float32 and fit["components"].shape == (k, D) and fit["mean"].dtype == np.float32
    # the mean: fp32 column sums over blocks of at most 512 rows added in float64, then one rounding to float32
    e_mean = np.abs(fit["mean"].astype(np.float64) - mean)
    mean_bound = 513 * EPS * np.abs(x.astype(np.float64)).mean(0)
    print(f"  mean: worst err / bound {(e_mean / mean_bound).max():.3e}")
    assert (e_mean <= mean_bound).all()
    top = np.abs(fit["components"]).argmax(1)
    assert (fit["components"][np.arange(k), top] > 0).all(), "sign rule"
    # a ratio carries the eigenvalue's error and the trace's (the diagonal's: at most 1e-4 of the trace as well)
    assert np.abs(fit["explained_variance_ratio"] - w[:k] / trace).max() <= 2 * EIG_TOL and fit["explained_variance_ratio"].sum() <= 1 + 1e-12
    assert abs(fit["total_variance"] * (N - 1) - trace) <= EIG_TOL * trace
    coords = fit["coords"]
    assert coords.is_cuda and coords.dtype == torch.float32 and tuple(coords.shape) == (N, k)
    y = coords.cpu().numpy()
    check_projection(y, x, fit["mean"], fit["components"], f"coords N={N} D={D} k={k}")
    # centroids: the per-group means of the coordinates, within the projection bound of the group's rows
    assert list(fit["centroids"]) == ["full"] + sorted(set(g.tolist())) and (fit["centroids"]["full"] == 0).all()
    d = x.astype(np.float64) - fit["mean"].astype(np.float64)
    row_bound = (D + 8) * EPS * np.outer(np.linalg.norm(d, axis=1), np.linalg.norm(comp, axis=1))
    for gv in sorted(set(g.tolist())):
        m = g == gv
        err = np.abs(fit["centroids"][gv] - y[m].astype(np.float64).mean(0))
        print(f"  group {gv} ({m.sum()} rows): centroid vs mean of coords {err.max():.3e} (bound {row_bound[m].mean(0).min():.3e})")
        assert (err <= row_bound[m].mean(0)).all()
    assert torch.equal(analysis.pca_project(fit, xd), coords), "pca_project(fit, x) is not coords bit for bit"


def test_pca_takes_a_table_and_a_groups_override():
    from dbmm_amd import analysis, synth, trainer
    x, y, c = synth.embedding_dataset(21, "train", 500, 512)
    table = trainer.EmbeddingTable(x, y.numpy(), c.numpy())
    fit = analysis.pca(table, k=2)
    assert list(fit["centroids"]) == ["full"] + sorted(set(table.group_array.tolist()))
    same = analysis.pca(table.embeddings, table.group_array, k=2)
    assert torch.equal(fit["coords"], same["coords"]) and np.array_equal(fit["components"], same["components"])
    over = analysis.pca(table, groups=table.targets.cpu().numpy(), k=2)          # coloured by target instead
    assert list(over["centroids"]) == ["full", 0, 1] and torch.equal(over["coords"], fit["coords"])
    assert torch.equal(analysis.pca_project(fit, table), fit["coords"])
    with pytest.raises(ValueError):
        analysis.pca(table.embeddings)                                          # a bare tensor needs its groups
    for bad_k in (0, 9):                                                        # refused before anything is launched
        with pytest.raises(ValueError):
            analysis.pca(table, k=bad_k)
    with pytest.raises(ValueError):
        analysis.pca(table.embeddings[:1], table.group_array[:1])


def test_centroids_under_translation():
    """rows 50 spreads from the origin: the group means are taken of the CENTRED gathered rows, so a centroid keeps the bound of
    the coordinates it averages (a sum of raw rows in fp32 would lose 2^-24 of the offset, ~50 x more)"""
    from dbmm_amd import analysis
    N, D = 3000, 1024
    x, xd, mean = case(N, D, 50 * spread(D))
    g = _groups(N)
    fit = analysis.pca(xd, g, k=3)
    comp = fit["components"].astype(np.float64)
    d = x.astype(np.float64) - fit["mean"].astype(np.float64)
    row_bound = (D + 8) * EPS * np.outer(np.linalg.norm(d, axis=1), np.linalg.norm(comp, axis=1))
    for gv in sorted(set(g.tolist())):
        m = g == gv
        want = d[m].mean(0) @ comp.T                                             # float64: (mean_g - mean) . components^T
        err = np.abs(fit["centroids"][gv] - want)
        print(f"translated, group {gv} ({m.sum()} rows): centroid err {err.max():.3e} (bound {row_bound[m].mean(0).min():.3e})")
        assert (err <= row_bound[m].mean(0)).all()


# ---- 6. the report ----------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def tables():
    from dbmm_amd import synth, trainer
    out = []
    for split, n in (("train", 900), ("val", 500), ("test", 600)):
        x, y, c = synth.embedding_dataset(21, split, n, 512)
        out.append(trainer.EmbeddingTable(x, y.numpy(), c.numpy()))
    return out


def test_projection_report_puts_every_split_in_trains_frame(tables):
    from dbmm_amd import adapter, analysis, synth
    opt = SimpleNamespace(batch_size=256)
    rep, fit = analysis.projection_report(opt, *tables, k=3, num_data=400, seed=7)
    assert list(rep) == ["train", "val", "test"]
    for split, table in zip(rep, tables):
        s = rep[split]
        rows = analysis.sample_rows(len(table), 400, 7)
        assert np.array_equal(s["rows"], rows) and s["coords"].shape == (400, 3) and isinstance(s["coords"], np.ndarray)
        assert np.array_equal(s["groups"], table.group_array[rows])
        assert np.array_equal(s["targets"], table.targets.cpu().numpy()[rows]) and np.array_equal(s["spurious"], table.targets_spurious.cpu().numpy()[rows])
        assert np.array_equal(s["groups"], 2 * s["targets"] + s["spurious"])
        # in train's frame: the split's sampled rows through train's fit
        want = analysis.pca_project(fit, table.embeddings[torch.from_numpy(rows).cuda()].contiguous())
        assert np.array_equal(s["coords"], want.cpu().numpy())
    # the fit is the PCA of exactly the sampled train rows
    rows = analysis.sample_rows(len(tables[0]), 400, 7)
    own = analysis.pca(tables[0].embeddings[torch.from_numpy(rows).cuda()].contiguous(), tables[0].group_array[rows], k=3)
    assert np.array_equal(own["components"], fit["components"]) and np.array_equal(own["mean"], fit["mean"])
    assert np.array_equal(rep["train"]["coords"], fit["coords"].cpu().numpy())
    val_own = analysis.pca(tables[1], k=3)
    assert not np.array_equal(val_own["mean"], fit["mean"])
    # all rows (num_data None), after a transform
    ad = adapter.Adapter(512, 128)
    ad.load_state_dict(synth.adapter_state_dict(3, 512, 128))
    ad = ad.cuda().eval()
    rep_t, fit_t = analysis.projection_report(opt, *tables, transform=ad, k=2)
    for split, table in zip(rep_t, tables):
        with torch.no_grad():
            z = ad(table.embeddings)
        assert np.array_equal(rep_t[split]["rows"], np.arange(len(table)))
        assert np.array_equal(rep_t[split]["coords"], analysis.pca_project(fit_t, z).cpu().numpy())
    rep_0, fit_0 = analysis.projection_report(opt, *tables, k=2)
    assert not np.array_equal(fit_0["mean"], fit_t["mean"]), "the transform was not applied"
    assert not ad.training


# ---- 7. memory ----------------------------------------------------------------------------------------------------------------------------

def test_pca_allocates_no_copy_of_the_rows():
    from dbmm_amd import analysis
    n, d = 40000, 1024
    g = torch.Generator().manual_seed(81)
    x = (0.5 * torch.randn(n, d, generator=g) + 0.1 * torch.randn(1, d, generator=g)).cuda()
    groups = torch.randint(0, 4, (n,), generator=g).numpy()
    inputs = x.numel() * 4

    def peak(fn):
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        out = fn()
        torch.cuda.synchronize()
        return out, torch.cuda.max_memory_allocated() - base

    def composed():
        xc = x - x.mean(0)
        S = xc.T @ xc
        return S

    fit, extra = peak(lambda: analysis.pca(x, groups, k=2))
    _, extra_torch = peak(composed)
    print(f"N={n} D={d}: peak extra device memory {extra / 2**20:.1f} MB (pca) vs {extra_torch / 2**20:.1f} MB (torch composition) for "
          f"{inputs / 2**20:.1f} MB of rows")
    assert extra <= 0.5 * inputs
    assert extra_torch >= inputs
    assert np.isfinite(fit["explained_variance"]).all() and torch.isfinite(fit["coords"]).all()


# ---- 8. the wrappers check their operands -------------------------------------------------------------------------------------------------

def test_wrappers_check_their_operands():
    from dbmm_amd import ops
    x, xd, mean = case(37, 64)
    c = torch.from_numpy(mean.astype(np.float32))
    V = torch.zeros(2, 64)
    with pytest.raises(RuntimeError):
        ops.covariance(torch.from_numpy(x), c)                                  # CPU tensors
    with pytest.raises(RuntimeError):
        ops.project_rows(torch.from_numpy(x), c, V)
    with pytest.raises(RuntimeError):
        ops.covariance(xd, c.cuda()[:-1].contiguous())
    with pytest.raises(RuntimeError):
        ops.covariance(xd.double(), c.cuda())
    with pytest.raises(RuntimeError):
        ops.covariance(xd.t(), c.cuda())                                        # not contiguous
    with pytest.raises(RuntimeError):
        ops.project_rows(xd, c.cuda(), torch.zeros(9, 64, device="cuda"))
    with pytest.raises(RuntimeError):
        ops.project_rows(xd, c.cuda(), torch.zeros(2, 128, device="cuda"))
    with pytest.raises(RuntimeError):
        ops.project_rows(xd, c.cuda(), V)                                       # basis on the CPU
    with pytest.raises(ops.DbmmUnsupported):
        ops.covariance(torch.zeros(10, 96, device="cuda"), torch.zeros(96, device="cuda"))
    with pytest.raises(ops.DbmmUnsupported):
        ops.project_rows(torch.zeros(10, 4160, device="cuda"), torch.zeros(4160, device="cuda"), torch.zeros(2, 4160, device="cuda"))
