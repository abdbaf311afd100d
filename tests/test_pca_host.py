"""PCA maps of embedding splits, the parts that need no GPU: the planted-spectrum generator the GPU tests use keeps the eigengap
their angle bound needs; sample_rows draws the reference's rows (plot_umap, demo/visualizer.py:321-334); the numpy eigen step
(order, sign rule, mean correction, ratios); the C entries are declared, exported and bound and refuse bad arguments before they
touch a device; analysis.pca has no CPU path."""
import ctypes

import numpy as np
import pytest
import torch

from dbmm_amd import _lib

# every (N, D) the GPU tests draw from `planted` with N >= 37 (tests/test_gpu_pca.py)
SHAPES = [(37, 64), (300, 128), (1025, 192), (2085, 192), (20000, 64), (3000, 1024)]
GAP_MIN = 0.03                     # eigengap of the three planted directions, as a share of the trace


def planted(N, D, offset=2.0):
    """float32 [N, D]: isotropic noise of spread 4 / sqrt(D), three planted directions of spread 4, 3, 2 and a constant vector"""
    r = np.random.RandomState(N + D)
    Q, _ = np.linalg.qr(r.randn(D, D))
    x = (4 / np.sqrt(D)) * r.randn(N, D) + (r.randn(N, 3) * np.array([4.0, 3.0, 2.0])) @ Q[:3] + offset * r.randn(1, D)
    return x.astype(np.float32)


def scatter_f64(x, center):
    d = x.astype(np.float64) - np.asarray(center, dtype=np.float64)
    return d.T @ d


def eig_desc(S):
    w, V = np.linalg.eigh(S)
    return w[::-1], V[:, ::-1].T


def gaps(w):
    """gap_j = distance from eigenvalue j to its nearest neighbour (descending w)"""
    up = np.concatenate([[np.inf], w[:-1] - w[1:]])
    down = np.concatenate([w[:-1] - w[1:], [np.inf]])
    return np.minimum(up, down)


@pytest.fixture(scope="module")
def built():
    _lib.build()
    return _lib.lib()


@pytest.mark.parametrize("N,D", SHAPES)
@pytest.mark.parametrize("scale", [1.0, 50.0], ids=["offset2", "offset50spreads"])
def test_generator_keeps_the_eigengap(N, D, scale):
    offset = 2.0 if scale == 1.0 else 50 * 4 / np.sqrt(D)
    x = planted(N, D, offset)
    w, _ = eig_desc(scatter_f64(x, x.astype(np.float64).mean(0)))
    ratio = gaps(w)[:3] / w.sum()
    print(f"N={N} D={D} offset={offset:.3g}: gap / trace of the three planted directions {ratio}")
    assert (ratio >= GAP_MIN).all()


@pytest.mark.parametrize("n,num_data,seed", [(100, 10, 42), (4795, 1000, 42), (4795, 1000, 7), (50, 50, 0), (30, 100, 42), (1, 5, 3)])
def test_sample_rows_draws_the_reference_rows(n, num_data, seed):
    from dbmm_amd import analysis
    state = np.random.get_state()
    np.random.seed(seed)
    num = np.min((num_data, n))
    want = np.random.choice(np.arange(n), size=num, replace=False)           # the reference's statements
    np.random.set_state(state)
    before = np.random.get_state()[1].copy()
    got = analysis.sample_rows(n, num_data, seed)
    assert np.array_equal(got, want) and len(got) == min(n, num_data)
    assert np.array_equal(np.random.get_state()[1], before), "sample_rows moved the global numpy stream"


def test_sample_rows_slice_and_all():
    from dbmm_amd import analysis
    emb = np.arange(100)
    assert np.array_equal(analysis.sample_rows(100, None), emb)
    assert np.array_equal(analysis.sample_rows(100, 10, offset=25), emb[25:35])
    assert np.array_equal(analysis.sample_rows(100, 10, offset=95), emb[95:105])
    assert np.array_equal(analysis.sample_rows(100, 10, seed=1, offset=5), emb[5:15])


@pytest.mark.parametrize("k", [1, 2, 3, 8])
def test_eigen_step_order_sign_and_mean_correction(k):
    from dbmm_amd import analysis
    N, D = 300, 128
    x = planted(N, D).astype(np.float64)
    mean = x.mean(0)
    spread = 4 / np.sqrt(D)
    center = (mean + 0.1 * spread * np.random.RandomState(5).randn(D)).astype(np.float32)      # 0.1 spreads off the mean
    comp, var, ratio, total = analysis.pca_from_scatter(scatter_f64(x, center), center, mean, N, k)
    w, V = eig_desc(scatter_f64(x, mean))
    assert comp.shape == (k, D) and comp.dtype == np.float32 and var.dtype == np.float64
    e_var = np.abs(var * (N - 1) - w[:k]).max() / w.sum()
    print(f"k={k}: eigenvalue err / trace {e_var:.3e}, total variance {total:.6f} (numpy {x.var(0, ddof=1).sum():.6f}), ratios {ratio}")
    assert e_var <= 1e-12
    assert (np.diff(var) <= 0).all(), "descending variance"
    assert abs(total - x.var(0, ddof=1).sum()) <= 1e-10 * total
    assert np.allclose(ratio, w[:k] / w.sum(), rtol=1e-10) and ratio.sum() <= 1 + 1e-12
    for j in range(min(k, 3)):                                                   # the planted directions have a gap: the vector is pinned
        cosang = abs(float(comp[j].astype(np.float64) @ V[j]))
        assert 1 - cosang <= 1e-6
    top = np.abs(comp).argmax(1)
    assert (comp[np.arange(k), top] > 0).all(), "each component's largest-magnitude entry is positive"
    # without the correction the same call is visibly off: the test would notice a dropped term
    _, var0, _, _ = analysis.pca_from_scatter(scatter_f64(x, center), mean, mean, N, k)
    assert np.abs(var0 * (N - 1) - w[:k]).max() / w.sum() > 1e-9
    with pytest.raises(ValueError):
        analysis.pca_from_scatter(scatter_f64(x, center), center, mean, N, 9)
    with pytest.raises(ValueError):
        analysis.pca_from_scatter(scatter_f64(x, center), center, mean, 1, k)


def test_symbols_exported_and_bound(built):
    for name in ("dbmm_workspace_bytes_covariance", "dbmm_covariance", "dbmm_project_rows"):
        assert name in _lib.EXPORTS
        assert hasattr(ctypes.CDLL(_lib.LIB_PATH), name)
    assert _lib.kernel_source_hash("covariance_tile_kernel") is not None and _lib.kernel_source_hash("project_rows_kernel<2>") is not None


def _aligned(buf):
    return (ctypes.addressof(buf) + 15) & ~15


def test_argument_validation_without_gpu(built):
    """every refusal returns before a device is touched (there is none here)"""
    buf = (ctypes.c_float * 4096)()
    p = _aligned(buf)
    big = 1 << 30
    cov, proj = built.dbmm_covariance, built.dbmm_project_rows
    assert cov(None, p, p, 10, 128, p, big, None) == -4 and cov(p, None, p, 10, 128, p, big, None) == -4
    assert cov(p, p, None, 10, 128, p, big, None) == -4 and cov(p, p, p, 10, 128, None, big, None) == -4
    assert cov(p, p, p, 10, 96, p, big, None) == -5                              # D % 64 != 0
    assert cov(p, p, p, 10, 4160, p, big, None) == -5                            # D > 4096
    assert cov(p, p, p, 0, 128, p, big, None) == -1 and cov(p, p, p, (1 << 23) + 1, 128, p, big, None) == -1
    assert cov(p + 4, p, p, 10, 128, p, big, None) == -2 and cov(p, p + 4, p, 10, 128, p, big, None) == -2
    assert cov(p, p, p, 10, 128, p + 8, big, None) == -2
    need = built.dbmm_workspace_bytes_covariance(10, 128)
    assert need > 0 and cov(p, p, p, 10, 128, p, need - 1, None) == -3
    assert proj(None, p, p, p, 10, 128, 2, None) == -4 and proj(p, p, None, p, 10, 128, 2, None) == -4
    assert proj(p, p, p, None, 10, 128, 2, None) == -4 and proj(p, None, p, p, 10, 128, 2, None) == -4
    assert proj(p, p, p, p, 10, 96, 2, None) == -5 and proj(p, p, p, p, 10, 4160, 2, None) == -5
    assert proj(p, p, p, p, 0, 128, 2, None) == -1
    assert proj(p, p, p, p, 10, 128, 0, None) == -1 and proj(p, p, p, p, 10, 128, 9, None) == -1
    assert proj(p + 4, p, p, p, 10, 128, 2, None) == -2 and proj(p, p, p + 4, p, 10, 128, 2, None) == -2


def test_workspace_is_partial_tiles_only(built):
    """P row ranges x tiles of the upper triangle x 32 KB: P from (N, D) alone, about 3 x 256 units, never N x anything"""
    for n, d in ((1, 64), (37, 64), (4795, 1024), (162770, 1024), (1 << 23, 1024), (162770, 4096), (1 << 23, 64)):
        b = built.dbmm_workspace_bytes_covariance(n, d)
        tiles = (d // 64) * (d // 64 + 1) // 2
        units = b // (64 * 64 * 8)
        print(f"N={n} D={d}: {units} units ({units // tiles} ranges x {tiles} tiles), {b / 2**20:.1f} MB")
        assert b % (64 * 64 * 8) == 0 and units % tiles == 0 and tiles <= units <= tiles + 3 * 256
    assert built.dbmm_workspace_bytes_covariance(162770, 1024) == built.dbmm_workspace_bytes_covariance(1 << 23, 1024)
    assert 2 * 256 <= built.dbmm_workspace_bytes_covariance(162770, 1024) // (64 * 64 * 8) <= 4 * 256
    assert built.dbmm_workspace_bytes_covariance(10, 96) == 0 and built.dbmm_workspace_bytes_covariance(0, 128) == 0


def test_pca_has_no_cpu_path():
    from dbmm_amd import analysis
    x = torch.from_numpy(planted(37, 64))
    with pytest.raises(_lib.DbmmError):
        analysis.pca(x, np.zeros(37, dtype=np.int64))
    with pytest.raises(_lib.DbmmError):
        analysis.pca_project({"mean": np.zeros(64, np.float32), "components": np.zeros((2, 64), np.float32)}, x)
