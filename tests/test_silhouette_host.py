"""Silhouettes, the parts that need no GPU: the float64 restatement every other silhouette test is measured against (checked by
hand and, where sklearn imports, against sklearn), analysis.silhouette_from_sums and its conventions, the C entries' argument
checks, and the conditions on the planted-group rows under which the GPU tests' per-row comparisons are decidable."""
import ctypes

import numpy as np
import pytest

from dbmm_amd import _lib, synth

E_SHAPE, E_ALIGN, E_WORKSPACE, E_ARG, E_UNSUPPORTED = -1, -2, -3, -4, -5


# ---- the yardstick ---------------------------------------------------------------------------------------------------------------

def row_group_sums_f64(x, dense, G, chunk=16):
    """R float64 [N, G]: R[i, g] = sum over j != i with dense[j] == g of ||x_i - x_j||, from direct differences (never the Gram
    form) in float64; labels outside [0, G) are in no sum"""
    x = np.asarray(x, dtype=np.float64)
    dense = np.asarray(dense)
    N = x.shape[0]
    onehot = (dense[:, None] == np.arange(G)[None, :]).astype(np.float64)                 # [N, G]
    R = np.empty((N, G))
    for i in range(0, N, chunk):
        d = np.sqrt(((x[i:i + chunk, None, :] - x[None, :, :]) ** 2).sum(-1))             # [chunk, N]; d[i, i] is exactly 0
        R[i:i + chunk] = d @ onehot
    return R


def silhouette_f64(x, labels):
    """The restatement: {'samples', 'a', 'b' float64 [N], 'nearest' (a label per row), 'second' (the second smallest mean distance
    to another label, inf with two labels), 'score', 'per_label', 'R', 'labels', 'counts'}, written row by row from the definition"""
    uniq, dense, counts = np.unique(np.asarray(labels), return_inverse=True, return_counts=True)
    dense = dense.reshape(-1)
    G, N = len(uniq), len(dense)
    if G < 2:
        raise ValueError("one label")
    R = row_group_sums_f64(x, dense, G)
    a, b, s, second = np.zeros(N), np.zeros(N), np.zeros(N), np.full(N, np.inf)
    nearest = np.zeros(N, dtype=np.int64)
    for i in range(N):
        others = sorted((R[i, g] / counts[g], g) for g in range(G) if g != dense[i])      # ties: the lowest index first
        b[i], nearest[i] = others[0]
        if len(others) > 1:
            second[i] = others[1][0]
        if counts[dense[i]] > 1:
            a[i] = R[i, dense[i]] / (counts[dense[i]] - 1)
            s[i] = (b[i] - a[i]) / max(a[i], b[i]) if max(a[i], b[i]) > 0 else 0.0
    return {"samples": s, "a": a, "b": b, "nearest": uniq[nearest], "second": second, "score": s.mean(),
            "per_label": {lab: s[dense == k].mean() for k, lab in enumerate(uniq)}, "R": R, "labels": uniq, "counts": counts}


def test_restatement_on_four_points_of_a_line():
    """x = 0, 1, 4, 6 on a line, labels A A B B.
    row 0: a = 1, b = (4 + 6) / 2 = 5, s = 4 / 5        row 1: a = 1, b = (3 + 5) / 2 = 4, s = 3 / 4
    row 2: a = 2, b = (4 + 3) / 2 = 3.5, s = 1.5 / 3.5  row 3: a = 2, b = (6 + 5) / 2 = 5.5, s = 3.5 / 5.5"""
    x = np.array([[0.0], [1.0], [4.0], [6.0]])
    ref = silhouette_f64(x, np.array([7, 7, 9, 9]))
    assert np.array_equal(ref["a"], [1, 1, 2, 2]) and np.array_equal(ref["b"], [5, 4, 3.5, 5.5])
    assert np.allclose(ref["samples"], [4 / 5, 3 / 4, 1.5 / 3.5, 3.5 / 5.5], rtol=1e-15, atol=0)
    assert ref["nearest"].tolist() == [9, 9, 7, 7]
    assert np.array_equal(ref["R"], [[1, 10], [1, 8], [7, 2], [11, 2]])
    assert abs(ref["score"] - (4 / 5 + 3 / 4 + 1.5 / 3.5 + 3.5 / 5.5) / 4) < 1e-15


def test_restatement_matches_sklearn():
    metrics = pytest.importorskip("sklearn.metrics")
    x = synth.normal(5, "sil/sk", (300, 24)).double().numpy()
    labels = (synth.uniform(5, "sil/sk/l", (300,)).numpy() * 5).astype(np.int64)
    labels[17] = 11                                                                       # a label with one row
    ref = silhouette_f64(x, labels)
    want = metrics.silhouette_samples(x, labels, metric="euclidean")
    assert np.abs(ref["samples"] - want).max() <= 1e-12
    assert ref["samples"][17] == 0.0


# ---- silhouette_from_sums ---------------------------------------------------------------------------------------------------------

def _from_sums(x, labels):
    from dbmm_amd import analysis
    uniq, dense, counts = np.unique(labels, return_inverse=True, return_counts=True)
    dense = dense.reshape(-1)
    return analysis.silhouette_from_sums(row_group_sums_f64(x, dense, len(uniq)), dense, counts), uniq


def test_from_sums_matches_the_restatement_in_input_order():
    x = synth.normal(6, "sil/fs", (240, 16)).double().numpy()
    labels = (synth.uniform(6, "sil/fs/l", (240,)).numpy() * 4).astype(np.int64) * 3 + 1  # shuffled: 1, 4, 7, 10
    got, uniq = _from_sums(x, labels)
    ref = silhouette_f64(x, labels)
    for key in ("a", "b", "samples"):
        assert np.abs(got[key] - ref[key]).max() <= 1e-13, key
    assert np.array_equal(uniq[got["nearest"]], ref["nearest"])
    # another order of the same rows: every row keeps its value
    perm = np.random.RandomState(0).permutation(240)
    got_p, _ = _from_sums(x[perm], labels[perm])
    assert np.abs(got_p["samples"] - got["samples"][perm]).max() <= 1e-13
    assert np.array_equal(got_p["nearest"], got["nearest"][perm])


def test_from_sums_conventions():
    from dbmm_amd import analysis
    x = synth.normal(7, "sil/conv", (60, 8)).double().numpy()
    labels = np.arange(60) % 3
    labels[5] = 3                                                                         # a singleton
    got, _ = _from_sums(x, labels)
    ref = silhouette_f64(x, labels)
    assert got["samples"][5] == 0.0 and got["a"][5] == 0.0 and ref["samples"][5] == 0.0
    assert np.abs(got["samples"] - ref["samples"]).max() <= 1e-13
    # an empty label (index 2 of 5, index 4 too) is ignored: the same values as without it
    dense = np.where(labels >= 2, labels + 1, labels)                                     # 0, 1, 3, 4 of 0..5
    counts = np.bincount(dense, minlength=6)
    assert counts[2] == 0 and counts[5] == 0
    wide = analysis.silhouette_from_sums(row_group_sums_f64(x, dense, 6), dense, counts)
    assert np.abs(wide["samples"] - got["samples"]).max() <= 1e-13 and not np.isin(wide["nearest"], (2, 5)).any()
    # identical rows: a = b = 0 gives 0, not nan
    same = analysis.silhouette_from_sums(np.zeros((6, 2)), np.array([0, 0, 0, 1, 1, 1]), np.array([3, 3]))
    assert np.array_equal(same["samples"], np.zeros(6)) and np.array_equal(same["a"], np.zeros(6)) and np.array_equal(same["b"], np.zeros(6))
    # a tie for the nearest label goes to the lowest index
    R = np.array([[0.0, 6.0, 3.0, 9.0], [6.0, 0.0, 1.0, 1.0], [3.0, 2.0, 0.0, 1.0], [9.0, 2.0, 1.0, 0.0]])
    tie = analysis.silhouette_from_sums(R, np.array([0, 1, 1, 2]), np.array([1, 2, 1, 0]))
    assert tie["nearest"][0] == 1 and tie["b"][0] == 3.0                                  # 6 / 2 == 3 / 1: label 1, not 2
    # one label
    with pytest.raises(ValueError):
        analysis.silhouette_from_sums(np.zeros((4, 3)), np.array([1, 1, 1, 1]), np.array([0, 4, 0]))
    with pytest.raises(ValueError):
        analysis.silhouette_from_sums(np.zeros((4, 2)), np.array([0, 0, 1, 1]), np.array([3, 1]))   # not the labels' counts


# ---- the C entries without a GPU ------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def built():
    _lib.build()
    return _lib.lib()


def test_symbols_exported_and_bound(built):
    for name in ("dbmm_pairdist_row_group_sums", "dbmm_workspace_bytes_pairdist_rows"):
        assert name in _lib.EXPORTS
        assert hasattr(ctypes.CDLL(_lib.LIB_PATH), name)
    assert _lib.kernel_source_hash("pairdist_rows_tile_kernel") == _lib.kernel_source_hash("pairdist_tile_kernel") is not None
    from dbmm_amd import ops
    assert ops.PAIRDIST_ROWS_MAX_G == 16 == ops.KMEANS_MAX_K
    header = open(_lib.INCLUDE + "/dbmm.h").read()
    assert "dbmm_pairdist_row_group_sums(" in header and "dbmm_workspace_bytes_pairdist_rows(" in header


def test_argument_validation_without_gpu(built):
    buf = (ctypes.c_float * 4096)()
    base = (ctypes.addressof(buf) + 15) & ~15                                             # 16-byte aligned inside the buffer
    p = ctypes.c_void_p(base)
    f = built.dbmm_pairdist_row_group_sums
    big = 1 << 30
    assert f(p, p, p, p, 0, 128, 4, p, big, None) == E_SHAPE
    assert f(p, p, p, p, 10, 128, 17, p, big, None) == E_SHAPE
    assert f(p, p, p, p, 10, 128, 0, p, big, None) == E_SHAPE
    assert f(p, p, p, p, (1 << 23) + 1, 128, 4, p, big, None) == E_SHAPE
    assert f(p, p, p, p, 10, 100, 4, p, big, None) == E_UNSUPPORTED
    assert f(p, p, p, p, 10, 8192, 4, p, big, None) == E_UNSUPPORTED
    assert f(p, p, p, p, 0, 100, 4, None, big, None) == E_SHAPE                           # the order: shape first
    for k in range(4):
        args = [p, p, p, p]
        args[k] = None
        assert f(*args, 10, 128, 4, p, big, None) == E_ARG
    assert f(p, p, p, p, 10, 128, 4, None, big, None) == E_ARG
    off = ctypes.c_void_p(base + 4)
    assert f(off, p, p, p, 10, 128, 4, p, big, None) == E_ALIGN
    assert f(p, p, off, p, 10, 128, 4, p, big, None) == E_ALIGN
    assert f(p, p, p, p, 10, 128, 4, off, big, None) == E_ALIGN
    need = built.dbmm_workspace_bytes_pairdist_rows(10, 128, 4)
    assert need > 0
    assert f(p, p, p, p, 10, 128, 4, p, need - 1, None) == E_WORKSPACE
    assert f(p, p, p, p, 10, 128, 16, p, need, None) == E_WORKSPACE                       # 16 labels need more than 4 do
    assert _lib.E_UNSUPPORTED == E_UNSUPPORTED and _lib.E_ALIGN == E_ALIGN


def test_workspace_grows_with_the_call_and_is_never_n_by_n(built):
    w = built.dbmm_workspace_bytes_pairdist_rows
    assert w(0, 128, 4) == 0 and w(10, 128, 17) == 0
    ns = (1, 2, 255, 256, 257, 1000, 4095, 4096, 4097, 4352, 4608, 4795, 40000, 65536, 65537, 162770, 1 << 23)
    for d in (64, 128, 192, 1024, 4096):
        for g in (1, 2, 4, 16):
            sizes = [w(n, d, g) for n in ns]
            assert all(a <= b for a, b in zip(sizes, sizes[1:])), (d, g)
            dp = (d + 127) // 128 * 128
            for n, b in zip(ns, sizes):
                assert n * dp * 4 <= b <= n * dp * 4 + n * 8 + 256 + 16 * n * g * 8 + 4096, (n, d, g)
    for n in (4795, 162770):
        assert [w(n, d, 4) for d in (64, 128, 192, 256, 1024, 4096)] == sorted(w(n, d, 4) for d in (64, 128, 192, 256, 1024, 4096))
        assert [w(n, 1024, g) for g in range(1, 17)] == sorted(w(n, 1024, g) for g in range(1, 17))


# ---- the planted-group rows of the GPU tests ----------------------------------------------------------------------------------------

PLANTED_OFFSETS = (0.0, 8.0, 20.0, 36.0)      # the groups' centres along one direction: squared centre distances 64, 144, 256, 400, 784, 1296
PLANTED_N, PLANTED_D = 600, 512


def planted_rows(n=PLANTED_N, d=PLANTED_D, seed=31):
    """(x float32 [n, d], labels int64 [n] in shuffled order) of four planted groups: isotropic noise with 2 sigma^2 d = 256 at every
    d, taken off the centres' direction, plus the group's centre PLANTED_OFFSETS[g] along that direction and a common shift.  A
    squared distance between groups a and b is then |noise_i - noise_j|^2 + (offset_a - offset_b)^2: the mean distances of a row to
    the other groups differ by several per cent (sqrt(256 + 64) : sqrt(256 + 144) : sqrt(256 + 256)), so which group is nearest is
    decided far above the kernel's error.  (Isotropic rows with one small common shift would not do: every group equally far, b a
    coin toss.)"""
    u = synth.normal(seed, "planted/dir", (d,)).double().numpy()
    u /= np.linalg.norm(u)
    noise = np.sqrt(128.0 / d) * synth.normal(seed, "planted/noise", (n, d)).double().numpy()
    noise -= np.outer(noise @ u, u)
    labels = np.minimum((synth.uniform(seed, "planted/labels", (n,)).numpy().astype(np.float64) * 4).astype(np.int64), 3)
    x = noise + np.outer(np.asarray(PLANTED_OFFSETS)[labels], u) + 0.1 * synth.normal(seed, "planted/shift", (1, d)).double().numpy()
    return x.astype(np.float32), labels


@pytest.fixture(scope="module")
def planted():
    x, labels = planted_rows()
    return x, labels, silhouette_f64(x, labels)


def test_planted_rows_are_decidable(planted):
    """what the GPU tests rely on: no row's nearest other group is within 4e-4 relative of the runner-up (the kernel's 1e-4 on each of
    the two means cannot swap them), and every squared distance exceeds 1 % of the mean centred squared norm (the condition behind
    that 1e-4, tests/test_gpu_group_stats.py).  The cap on undecided rows is zero."""
    x, labels, ref = planted
    assert np.bincount(labels).min() >= 100 and not np.array_equal(labels, np.sort(labels))
    gap = (ref["second"] - ref["b"]) / ref["b"]
    print(f"planted: smallest relative gap between the two nearest other groups {gap.min():.3e}, score {ref['score']:.4f}")
    assert int((gap <= 4e-4).sum()) == 0
    assert gap.min() > 0.03                                                               # several per cent, as designed
    xd = x.astype(np.float64)
    xc = xd - xd.mean(0)
    sq = (xc ** 2).sum(1)
    d2 = sq[:, None] + sq[None, :] - 2 * xc @ xc.T                                        # float64 Gram form on centred rows: fine for a 1 % check
    np.fill_diagonal(d2, np.inf)
    print(f"planted: smallest squared distance {d2.min():.2f} against a mean centred squared norm of {sq.mean():.2f}")
    assert d2.min() > 0.01 * sq.mean()
    # the design: every row's nearest other group is the neighbour along the line
    want = np.array([1, 0, 1, 2])[labels]
    assert np.array_equal(ref["nearest"], want)
    assert 0.0 < ref["score"] < 1.0 and all(v > 0 for v in ref["per_label"].values())
