"""The device eigen-solver of `analysis.pca` (csrc/sym_eig.hip), the parts that need no GPU: a numpy float64 restatement of the
blocked subspace iteration (same start block, same stopping rule), the generators the GPU tests draw from and the conditions those
tests lean on (eigengaps, iteration counts, a case that must NOT converge early), the three C entries (declared, exported, bound,
refusing bad arguments before a device is touched), the workspace size, and the host tail both solvers share."""
import ctypes

import numpy as np
import pytest

from dbmm_amd import _lib
from test_pca_host import SHAPES, eig_desc, gaps, planted, scatter_f64

BLOCK = 16
START_SEED = 0x5EED
EIGHT_SHAPES = [(100, 64), (300, 128), (1025, 192), (3000, 1024)]
EIGHT_SPREADS = np.array([8.0, 7.0, 6.0, 5.0, 4.0, 3.5, 3.0, 2.5])
EIGHT_GAP_MIN = 0.029              # smallest eigengap of the eight planted directions over lambda_1
EIGHT_ITER_MAX = 11


def start_block(D, seed=START_SEED):
    """the start block of ops.sym_eig_topk: a private stream, never the global one"""
    return np.random.RandomState(seed).standard_normal((D, BLOCK))


def subspace_iteration(C, k, tol=1e-10, max_iter=256, seed=START_SEED):
    """Blocked subspace iteration with a Rayleigh-Ritz step in every iteration, numpy float64: what csrc/sym_eig.hip computes.
    Returns (theta [k], vectors [k, D], iterations done, converged, max_{j < k} r_j / theta_1 of the last iteration)."""
    Q = np.linalg.qr(start_block(C.shape[0], seed))[0]
    for it in range(1, max_iter + 1):
        Z = C @ Q
        T = Q.T @ Z
        th, W = np.linalg.eigh((T + T.T) / 2)
        th, W = th[::-1], W[:, ::-1]
        X, Y = Q @ W, Z @ W
        res = np.linalg.norm(Y - X * th, axis=0)[:k].max()                       # from the vectors
        if res <= tol * abs(th[0]):
            return th[:k], X[:, :k].T, it, True, res / th[0]
        L = np.linalg.cholesky(Y.T @ Y)
        Q = np.linalg.solve(L, Y.T).T
    return th[:k], X[:, :k].T, max_iter, False, res / th[0]


def eight_planted(N, D):
    """float32 [N, D]: isotropic noise of spread 4 / sqrt(D) plus eight orthogonal directions of spread 8, 7, 6, 5, 4, 3.5, 3, 2.5"""
    r = np.random.RandomState(7 + N + D)
    Q, _ = np.linalg.qr(r.randn(D, 8))
    return ((4 / np.sqrt(D)) * r.randn(N, D) + (r.randn(N, 8) * EIGHT_SPREADS) @ Q.T).astype(np.float32)


def powerlaw(D, p):
    """float64 [D, D], symmetric to the bit: U diag(j^-p) U^T in a random orthogonal frame"""
    U, _ = np.linalg.qr(np.random.RandomState(3 + D).randn(D, D))
    C = (U * np.arange(1, D + 1.0) ** -p) @ U.T
    return (C + C.T) / 2


def centred_scatter(x):
    x = x.astype(np.float64)
    return scatter_f64(x, x.mean(0))


_ref = {}


def restated(name, C, k, tol, max_iter=256):
    """the restatement's answer for a named matrix, computed once (the GPU tests compare iteration counts against it)"""
    key = (name, k, tol, max_iter)
    if key not in _ref:
        _ref[key] = subspace_iteration(C, k, tol, max_iter)
    return _ref[key]


@pytest.fixture(scope="module")
def built():
    _lib.build()
    return _lib.lib()


# ---- the conditions the GPU tests lean on ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("N,D", EIGHT_SHAPES)
def test_eight_planted_converges_fast_and_keeps_its_gaps(N, D):
    C = centred_scatter(eight_planted(N, D))
    w, U = eig_desc(C)
    gap = gaps(w)[:8].min() / w[0]
    print(f"N={N} D={D}: min gap / lambda_1 of the eight planted directions {gap:.4f}, lambda_17 / lambda_8 = {w[16] / w[7]:.3f}")
    assert gap >= EIGHT_GAP_MIN
    for k in (1, 2, 8):
        th, V, it, conv, res = subspace_iteration(C, k, tol=1e-12)
        sin = max(np.linalg.norm(V[j] - (V[j] @ U[j]) * U[j]) for j in range(k))
        print(f"  k={k}: {it} iterations, residual {res:.2e}, eigenvalue err {np.abs(th - w[:k]).max() / w[0]:.2e}, worst sin angle {sin:.2e}")
        assert conv and it <= EIGHT_ITER_MAX
        assert np.abs(th - w[:k]).max() <= (2e-12 + D * 2.0 ** -52) * w[0]


def test_powerlaw_iteration_counts():
    C = powerlaw(256, 0.5)
    assert np.array_equal(C, C.T)
    for k, cap in ((8, 68), (2, 27)):
        th, V, it, conv, res = subspace_iteration(C, k, tol=1e-12)
        print(f"powerlaw(256, 0.5) k={k}: {it} iterations (lambda_17 / lambda_k = {(k / 17) ** 0.5:.3f}), residual {res:.2e}")
        assert conv and it <= cap


def test_flat_bulk_does_not_converge_early():
    """three planted directions, k = 8: eigenvalues 4 .. 8 sit in the noise bulk, the factor lambda_17 / lambda_8 is close to 1.
    The count depends on the start block: from RandomState(0) the restatement is not converged after 24 iterations (residual 2e-5)
    and converged after 82; from the solver's block (0x5EED), which the GPU tests compare against, residual 4.8e-5 and 87."""
    C = centred_scatter(planted(300, 128))
    for seed, res24, cap in ((0, 2e-5, 82), (START_SEED, 4.8e-5, 90)):
        th, V, it, conv, res = subspace_iteration(C, 8, tol=1e-10, max_iter=24, seed=seed)
        print(f"planted(300, 128) k=8, start seed {seed:#x}, after 24 iterations: converged {conv}, residual {res:.2e}")
        assert not conv and it == 24 and 0.5 * res24 <= res <= 2 * res24
        th, V, it, conv, res = subspace_iteration(C, 8, tol=1e-10, max_iter=256, seed=seed)
        print(f"planted(300, 128) k=8, start seed {seed:#x}: converged {conv} after {it} iterations, residual {res:.2e}")
        assert conv and it <= cap                                                # with it // 4 of margin the GPU test stays inside 256


@pytest.mark.parametrize("N,D", SHAPES)
def test_planted_shapes_converge_for_small_k(N, D):
    C = centred_scatter(planted(N, D))
    for k in (1, 2, 3):
        th, V, it, conv, res = subspace_iteration(C, k, tol=1e-10)
        print(f"planted({N}, {D}) k={k}: {it} iterations, residual {res:.2e}")
        assert conv and it <= 15


def test_restatement_leaves_the_global_stream_alone():
    before = np.random.get_state()[1].copy()
    start_block(64)
    assert np.array_equal(np.random.get_state()[1], before)


# ---- the C entries -----------------------------------------------------------------------------------------------------------------------

ENTRIES = ("dbmm_workspace_bytes_sym_eig", "dbmm_sym_eig_begin", "dbmm_sym_eig_iterate")


def test_symbols_declared_exported_and_bound(built):
    header = open(_lib.INCLUDE + "/dbmm.h").read()
    for name in ENTRIES:
        assert name + "(" in header
        assert name in _lib.EXPORTS
        assert hasattr(ctypes.CDLL(_lib.LIB_PATH), name)
        assert getattr(built, name).argtypes is not None
    assert built.dbmm_workspace_bytes_sym_eig.restype is ctypes.c_size_t
    for kernel in ("sym_eig_begin_kernel", "sym_eig_matvec_kernel", "sym_eig_ritz_kernel", "sym_eig_rotate_kernel", "sym_eig_finish_kernel"):
        assert _lib.kernel_source_hash(kernel) is not None


def _aligned(buf):
    return (ctypes.addressof(buf) + 15) & ~15


def test_argument_validation_without_gpu(built):
    """every refusal returns before a device is touched (there is none here)"""
    buf = (ctypes.c_double * 4096)()
    p = _aligned(buf)
    big = 1 << 30
    begin, iterate = built.dbmm_sym_eig_begin, built.dbmm_sym_eig_iterate
    for D in (96, 4160, 0, -64):                                                 # D % 64 != 0, D > 4096, nothing to do
        assert begin(p, D, 2, 1e-10, p, big, None) == -5 and iterate(p, D, 1, p, big, None) == -5
    for k in (0, 9, -1):
        assert begin(p, 128, k, 1e-10, p, big, None) == -1
    for tol in (0.0, -1e-10, float("inf"), float("nan")):
        assert begin(p, 128, 2, tol, p, big, None) == -1
    assert iterate(p, 128, -1, p, big, None) == -1
    assert begin(None, 128, 2, 1e-10, p, big, None) == -4 and begin(p, 128, 2, 1e-10, None, big, None) == -4
    assert iterate(None, 128, 1, p, big, None) == -4 and iterate(p, 128, 1, None, big, None) == -4
    need = built.dbmm_workspace_bytes_sym_eig(128)
    assert need > 0 and begin(p, 128, 2, 1e-10, p, need - 1, None) == -3 and iterate(p, 128, 1, p, need - 1, None) == -3
    assert begin(p + 8, 128, 2, 1e-10, p, big, None) == -2 and begin(p, 128, 2, 1e-10, p + 8, big, None) == -2
    assert iterate(p + 8, 128, 1, p, big, None) == -2 and iterate(p, 128, 1, p + 8, big, None) == -2
    assert iterate(None, 128, 0, p, big, None) == -4                             # the checks come first even when nothing would be launched


def test_workspace_covers_the_documented_layout(built):
    """status block of 64 doubles, the Ritz vectors [16][D], Q and Z [D][16], the 16 x 16 partials of T and G and the 16 residual
    partials per 16 rows, W and M: (64 + 81 D + 512) doubles"""
    for D in (64, 128, 192, 1024, 4096):
        b = built.dbmm_workspace_bytes_sym_eig(D)
        nb = D // 16
        want = 64 + 16 * D + 2 * 16 * D + 2 * nb * 256 + nb * 16 + 2 * 256
        print(f"D={D}: {b} bytes = {b // 8} doubles ({b / 2**20:.2f} MB)")
        assert b == 8 * want == 8 * (64 + 81 * D + 512)
        assert b >= 8 * (64 + 16 * D)                                            # what Python reads views of
    for D in (0, 96, 4160):
        assert built.dbmm_workspace_bytes_sym_eig(D) == 0


# ---- analysis ------------------------------------------------------------------------------------------------------------------------------

def test_unknown_solver_is_refused_before_anything_else():
    import torch
    from dbmm_amd import analysis
    x = torch.from_numpy(planted(37, 64))                                        # a CPU tensor: a launch would raise DbmmError instead
    with pytest.raises(ValueError):
        analysis.pca(x, np.zeros(37, dtype=np.int64), solver="bogus")
    with pytest.raises(ValueError):
        analysis.pca(x, np.zeros(37, dtype=np.int64), k=2, solver="Device")
    assert analysis.SOLVERS == ("host", "device")


@pytest.mark.parametrize("k", [1, 2, 3, 8])
def test_shared_tail_gives_pca_from_scatter_bits(k):
    from dbmm_amd import analysis
    N, D = 300, 128
    x = planted(N, D).astype(np.float64)
    mean = x.mean(0)
    center = mean.astype(np.float32)
    S = scatter_f64(x, center)
    want = analysis.pca_from_scatter(S, center, mean, N, k)
    d = mean - center.astype(np.float64)
    C = S - np.float64(N) * np.outer(d, d)
    w, V = np.linalg.eigh(C)
    got = analysis._components_and_variances(w[::-1][:k], V[:, ::-1][:, :k].T, np.trace(C), N)
    for a, b in zip(got, want):
        assert np.array_equal(a, b) and np.asarray(a).dtype == np.asarray(b).dtype
    # the rules themselves, on an answer with the wrong signs: float32, largest-magnitude entry positive, / (n - 1), ratio
    comp, var, ratio, total = analysis._components_and_variances(w[::-1][:k], -V[:, ::-1][:, :k].T, np.trace(C), N)
    assert np.array_equal(comp, want[0]) and comp.dtype == np.float32
    assert np.array_equal(var, w[::-1][:k] / (N - 1.0)) and total == np.trace(C) / (N - 1.0)
