"""Kernel two-sample (MMD) and HSIC scores, the parts that need no GPU: the numpy statistics against the textbook formulas written
out on dense float64 kernel matrices, the bandwidth heuristic against the mean of the dense squared distances, and the refusals of
the C entry and of the op, with host pointers and host tensors."""
import ctypes

import numpy as np
import pytest
import torch

from dbmm_amd import _lib, analysis, ops

N, D, G = 60, 16, 3
GAMMAS = (0.02, 0.08, 0.3)


def dense_case():
    """rows, labels (label 1 is empty, label 2 has one row), the dense kernels [L, N, N] and the bucket sums [L, G, G] as the op
    defines them: unordered pairs i < j"""
    rng = np.random.default_rng(11)
    x = rng.normal(size=(N, D)) + 0.3 * rng.normal(size=(1, D))
    g = np.zeros(N, dtype=np.int64)
    g[17] = 2
    x[g == 2] += 0.8
    d2 = ((x[:, None, :] - x[None, :, :]) ** 2).sum(-1)
    Kd = np.exp(-np.asarray(GAMMAS)[:, None, None] * d2[None])
    onehot = (g[None, :] == np.arange(G)[:, None]).astype(np.float64)                # [G, N]
    upper = np.triu(np.ones((N, N)), 1)
    T = np.einsum("an,lnm,bm->lab", onehot, Kd * upper[None], onehot)
    K = T + T.transpose(0, 2, 1)
    K[:, np.arange(G), np.arange(G)] = T[:, np.arange(G), np.arange(G)]
    return x, g, Kd, K, onehot.sum(1)


def dense_case_three():
    """three labels with rows, for the finite values"""
    x, g, Kd, _, _ = dense_case()
    g = np.arange(N) % 3
    g[:7] = 0
    onehot = (g[None, :] == np.arange(G)[:, None]).astype(np.float64)
    T = np.einsum("an,lnm,bm->lab", onehot, Kd * np.triu(np.ones((N, N)), 1)[None], onehot)
    K = T + T.transpose(0, 2, 1)
    K[:, np.arange(G), np.arange(G)] = T[:, np.arange(G), np.arange(G)]
    return g, Kd, K, onehot.sum(1)


def textbook_mmd2(Kl, ia, ib, unbiased):
    """MMD^2 between the rows ia and ib of one dense kernel matrix (Gretton et al. 2012, eq. 3 / its V-statistic form)"""
    Kaa, Kbb, Kab = Kl[np.ix_(ia, ia)], Kl[np.ix_(ib, ib)], Kl[np.ix_(ia, ib)]
    m, n = len(ia), len(ib)
    if unbiased:
        aa = (Kaa.sum() - np.trace(Kaa)) / (m * (m - 1))
        bb = (Kbb.sum() - np.trace(Kbb)) / (n * (n - 1))
    else:
        aa, bb = Kaa.mean(), Kbb.mean()
    return aa + bb - 2 * Kab.mean()


@pytest.mark.parametrize("unbiased", [True, False])
def test_mmd_from_sums_is_the_textbook_statistic(unbiased):
    g, Kd, K, counts = dense_case_three()
    out = analysis.mmd_from_sums(K, counts, unbiased=unbiased)
    assert out["kernel_mean"].shape == (3, G, G) and out["mmd2"].shape == (3, G, G) and out["mmd2_sum"].shape == (G, G)
    for l in range(3):
        for a in range(G):
            assert out["mmd2"][l, a, a] == 0.0
            for b in range(G):
                ia, ib = np.flatnonzero(g == a), np.flatnonzero(g == b)
                if a != b:
                    want = textbook_mmd2(Kd[l], ia, ib, unbiased)
                    np.testing.assert_allclose(out["mmd2"][l, a, b], want, rtol=1e-12)
                    np.testing.assert_allclose(out["kernel_mean"][l, a, b], Kd[l][np.ix_(ia, ib)].mean(), rtol=1e-12)
    np.testing.assert_allclose(out["mmd2_sum"], out["mmd2"].sum(0), rtol=1e-12, atol=0)
    assert np.array_equal(out["mmd2"], out["mmd2"].transpose(0, 2, 1))


def test_mmd_from_sums_nan_exactly_where_a_label_is_too_small():
    x, g, Kd, K, counts = dense_case()
    assert counts.tolist() == [N - 1, 0, 1]
    u = analysis.mmd_from_sums(K, counts)
    # unbiased: label 0 alone has two rows; every mmd2 off the diagonal involves label 1 (empty) or 2 (one row)
    assert np.isfinite(u["kernel_mean"][:, 0, 0]).all() and np.isfinite(u["kernel_mean"][:, 0, 2]).all()
    assert np.isnan(u["kernel_mean"][:, 1, :]).all() and np.isnan(u["kernel_mean"][:, :, 1]).all() and np.isnan(u["kernel_mean"][:, 2, 2]).all()
    off = ~np.eye(G, dtype=bool)
    assert np.isnan(u["mmd2"][:, off]).all() and (u["mmd2"][:, 0, 0] == 0).all() and np.isnan(u["mmd2_sum"][off]).all()
    ia = np.flatnonzero(g == 0)
    for l in range(3):
        Kaa = Kd[l][np.ix_(ia, ia)]
        np.testing.assert_allclose(u["kernel_mean"][l, 0, 0], (Kaa.sum() - np.trace(Kaa)) / (len(ia) * (len(ia) - 1)), rtol=1e-12)
    # the V-statistic needs one row only: labels 0 and 2 are finite and equal the dense statistic, label 1 stays nan
    v = analysis.mmd_from_sums(K, counts, unbiased=False)
    ib = np.flatnonzero(g == 2)
    for l in range(3):
        np.testing.assert_allclose(v["mmd2"][l, 0, 2], textbook_mmd2(Kd[l], ia, ib, False), rtol=1e-12)
        assert v["kernel_mean"][l, 2, 2] == 1.0
    assert np.isnan(v["mmd2"][:, 1, :]).all() and np.isnan(v["mmd2"][:, :, 1]).all() and (v["mmd2"][:, 2, 2] == 0).all()


def test_hsic_from_sums_is_trace_khlh():
    for g, Kd, K, counts in (dense_case_three(), dense_case()[1:]):
        H = np.eye(N) - np.ones((N, N)) / N
        Lm = (g[:, None] == g[None, :]).astype(np.float64)
        got = analysis.hsic_from_sums(K, counts)
        assert got.shape == (3,) and got.dtype == np.float64
        for l in range(3):
            np.testing.assert_allclose(got[l], np.trace(Kd[l] @ H @ Lm @ H) / N ** 2, rtol=1e-12)
    with pytest.raises(ValueError):
        analysis.hsic_from_sums(np.zeros((2, 3, 2)), [1, 2, 3])
    with pytest.raises(ValueError):
        analysis.mmd_from_sums(np.zeros((2, 3, 3)), [1, 2])


def test_rbf_gammas_is_scale_over_the_mean_squared_distance():
    x = dense_case()[0]
    d2 = ((x[:, None, :] - x[None, :, :]) ** 2).sum(-1)
    m = d2.sum() / (N * (N - 1))
    got = analysis.rbf_gammas(torch.from_numpy(x).float(), scales=(0.25, 1.0, 4.0))
    assert got.dtype == np.float64 and got.shape == (3,)
    np.testing.assert_allclose(got, np.array([0.25, 1.0, 4.0]) / m, rtol=1e-6)           # the rows were rounded to fp32
    x32 = torch.from_numpy(x).float()
    d2 = torch.cdist(x32.double(), x32.double()) ** 2
    np.testing.assert_allclose(analysis.rbf_gammas(x32, scales=(1.0,)), [1.0 / (d2.sum().item() / (N * (N - 1)))], rtol=1e-12)
    np.testing.assert_allclose(analysis.rbf_gammas(x32, transform=lambda r: 2 * r), got / 4, rtol=1e-6)
    for bad in ((), (0.0,), (-1.0, 1.0), (float("nan"),)):
        with pytest.raises(ValueError):
            analysis.rbf_gammas(x32, scales=bad)
    with pytest.raises(ValueError):
        analysis.rbf_gammas(x32[:1])
    with pytest.raises(ValueError):
        analysis.rbf_gammas(torch.ones(5, 8))


@pytest.fixture(scope="module")
def built():
    _lib.build()
    return _lib.lib()


def test_symbols_exported_and_bound(built):
    for name in ("dbmm_pairdist_rbf_group_sums", "dbmm_workspace_bytes_pairdist_rbf"):
        assert name in _lib.EXPORTS
        assert hasattr(ctypes.CDLL(_lib.LIB_PATH), name)
    assert ops.PAIRDIST_RBF_MAX_L == 4


def test_argument_validation_without_gpu(built):
    buf = (ctypes.c_float * 1024)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    big = 1 << 30
    f = built.dbmm_pairdist_rbf_group_sums
    gam = lambda *v: ctypes.cast((ctypes.c_double * len(v))(*v), ctypes.c_void_p)
    ok = gam(0.5, 1.0, 2.0, 4.0, 8.0)
    assert f(p, p, p, ok, 0, p, 10, 128, 4, p, big, None) == -1                     # L = 0
    assert f(p, p, p, ok, 5, p, 10, 128, 4, p, big, None) == -1                     # L = 5
    assert f(p, p, p, ok, 4, p, 10, 128, 9, p, big, None) == -1                     # G = 9
    assert f(p, p, p, ok, 4, p, 0, 128, 4, p, big, None) == -1
    assert f(p, p, p, ok, 4, p, (1 << 23) + 1, 128, 4, p, big, None) == -1
    assert f(p, p, p, ok, 4, p, 10, 96, 4, p, big, None) == -5                      # D % 64: no kernel
    assert f(p, p, p, ok, 4, p, 10, 8192, 4, p, big, None) == -5
    assert f(p, p, p, ok, 0, p, 10, 96, 4, p, big, None) == -1                      # the shape is named before the width
    assert f(p, p, p, None, 4, p, 10, 128, 4, p, big, None) == -4                   # null gammas
    assert f(None, p, p, ok, 4, p, 10, 128, 4, p, big, None) == -4
    assert f(p, p, p, ok, 4, p, 10, 128, 4, None, big, None) == -4
    for bad in (float("nan"), 0.0, -1.0, float("inf")):
        assert f(p, p, p, gam(1.0, bad), 2, p, 10, 128, 4, p, big, None) == -4, bad
        assert f(p, p, p, gam(1.0, bad), 1, p, 10, 128, 4, p, 16, None) in (-2, -3)  # only the first L are read
    assert f(p, p, p, ok, 4, p, 10, 128, 4, p, 16, None) in (-2, -3)                # workspace too small (or the ctypes buffer unaligned)


def test_workspace_is_linear_in_rows_and_bandwidths(built):
    w, w1 = built.dbmm_workspace_bytes_pairdist_rbf, built.dbmm_workspace_bytes_pairdist
    for n, d in ((4795, 1024), (162770, 1024), (40000, 640)):
        assert w(n, d, 1) == w1(n, d)
        for L in (2, 3, 4):
            assert w(n, d, L) - w(n, d, L - 1) == w(n, d, 2) - w(n, d, 1) <= 1 << 18   # 512 bytes per workgroup and bandwidth
    assert w(10, 128, 0) == 0 and w(10, 128, 5) == 0 and w(0, 128, 1) == 0


def test_op_refuses_bad_gammas_before_touching_the_device():
    x, g, c = torch.zeros(4, 64), torch.zeros(4, dtype=torch.int64), torch.zeros(64)    # host tensors: the gammas are named first
    for bad, word in (((), "0 gammas"), ((1.0,) * 5, "5 gammas"), ((1.0, float("nan")), "nan"), ((0.0,), "0.0"), ((-2.5, 1.0), "-2.5"),
                      ((float("inf"),), "inf"), (None, "None"), (("a",), "'a'")):
        with pytest.raises(_lib.DbmmError) as e:
            ops.pairdist_rbf_group_sums(x, g, 1, c, bad)
        assert word in str(e.value), (bad, str(e.value))
    with pytest.raises(_lib.DbmmError) as e:                                            # good gammas (numpy numbers too): the host tensor is next
        ops.pairdist_rbf_group_sums(x, g, 1, c, np.array([0.5, 1.0], dtype=np.float32))
    assert "CPU tensor" in str(e.value)
