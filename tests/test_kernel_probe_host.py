"""The host steps of the kernel probe, the MMD witness function and the kernel alignment (analysis.parzen_from_sums, witness_from_sums,
alignment_from_sums) against dense float64 numpy on a few dozen rows, and the refusals that must come before anything touches a
device.  No GPU: the per-row kernel sums R are formed here from the dense kernel matrix."""
import numpy as np
import pytest
import torch

from dbmm_amd import analysis, ops

GAMMAS = (0.05, 0.4, 2.0)


def planted(n, d, seed, G=3):
    rng = np.random.RandomState(seed)
    labels = rng.randint(0, G, n)
    x = rng.randn(n, d) + 1.5 * rng.randn(G, d)[labels]
    return x, labels


def dense_kernels(x, gammas=GAMMAS):
    d2 = ((x[:, None, :] - x[None, :, :]) ** 2).sum(2)
    return np.stack([np.exp(-g * d2) for g in gammas])                   # [L, N, N], ones on the diagonal


def row_sums(Kd, labels, G):
    """R [L, N, G]: the kernel's definition, the row itself left out, labels outside [0, G) in nobody's sum"""
    off = Kd * (1.0 - np.eye(Kd.shape[1]))[None]
    onehot = (labels[:, None] == np.arange(G)[None, :]).astype(np.float64)
    return off @ onehot


def parzen_by_rows(R, labels, counts, prior):
    """the restatement, row by row from the definition"""
    L, N, G = R.shape
    density, pred, margin = np.full((L, N, G), np.nan), np.full((L, N), -1, dtype=np.int64), np.full((L, N), np.nan)
    for l in range(L):
        for i in range(N):
            scores = []
            for g in range(G):
                den = counts[g] - (1 if labels[i] == g else 0)
                if den > 0:
                    density[l, i, g] = R[l, i, g] / den
                    scores.append((density[l, i, g] if prior == "uniform" else R[l, i, g], g))
            if not scores:
                continue
            best = max(s for s, _ in scores)
            if best > 0:
                pred[l, i] = min(g for s, g in scores if s == best)
                if len(scores) >= 2:
                    rest = sorted((s for s, _ in scores), reverse=True)
                    margin[l, i] = (rest[0] - rest[1]) / rest[0]
    return density, pred, margin


@pytest.mark.parametrize("prior", ["uniform", "empirical"])
def test_parzen_matches_the_definition(prior):
    x, labels = planted(57, 6, 1, G=4)
    labels[labels == 2] = 0                                              # label 2 is empty
    labels[labels == 3] = 0
    labels[11] = 3                                                       # label 3 has one row
    labels[50:] = -1                                                     # seven query rows
    G = 4
    counts = np.bincount(labels[labels >= 0], minlength=G)
    assert counts[2] == 0 and counts[3] == 1
    R = row_sums(dense_kernels(x), labels, G)
    got = analysis.parzen_from_sums(R, labels, counts, prior=prior)
    density, pred, margin = parzen_by_rows(R, labels, counts, prior)
    assert got["density"].shape == (3, 57, 4) and got["pred"].dtype == np.int64
    np.testing.assert_allclose(got["density"], density, rtol=1e-14, equal_nan=True)
    assert np.array_equal(got["pred"], pred)
    np.testing.assert_allclose(got["margin"], margin, rtol=1e-12, equal_nan=True)
    assert np.isnan(got["density"][:, :, 2]).all()                       # the empty label
    assert np.isnan(got["density"][:, 11, 3]).all() and (got["pred"][:, 11] != 3).all()      # the singleton's own label: never its prediction
    assert np.isfinite(got["density"][:, 50:, 3]).all()                  # ... but a query row can be scored against it
    assert (got["pred"] != 2).all()
    want_score = density if prior == "uniform" else np.where(np.isnan(density), np.nan, R)
    np.testing.assert_allclose(got["score"], want_score, rtol=1e-14, equal_nan=True)


def test_parzen_ties_zero_rows_and_refusals():
    # an exact tie: 6 / 2 == 3 / 1, the lowest label wins; margin 0
    R = np.array([[[6.0, 3.0, 1.0], [0.0, 0.0, 0.0], [2.0, 2.0, 8.0]]])
    labels, counts = np.array([-1, -1, -1]), np.array([2, 1, 4])
    got = analysis.parzen_from_sums(R, labels, counts)
    assert got["pred"][0, 0] == 0 and got["margin"][0, 0] == 0.0
    assert got["pred"][0, 1] == -1 and np.isnan(got["margin"][0, 1])     # an all-zero row
    assert got["pred"][0, 2] == 1 and got["margin"][0, 2] == 0.0         # 2 / 1 == 8 / 4 > 2 / 2: label 1, not 2
    emp = analysis.parzen_from_sums(R, labels, counts, prior="empirical")
    assert emp["pred"].tolist() == [[0, -1, 2]] and emp["margin"][0, 0] == 0.5
    # one scorable label: a prediction, no margin
    one = analysis.parzen_from_sums(np.array([[[0.5, 0.0]]]), np.array([-1]), np.array([3, 0]))
    assert one["pred"][0, 0] == 0 and np.isnan(one["margin"][0, 0])
    with pytest.raises(ValueError):
        analysis.parzen_from_sums(R, labels, counts, prior="flat")
    with pytest.raises(ValueError):
        analysis.parzen_from_sums(R[0], labels, counts)                  # not [L, N, G]
    with pytest.raises(ValueError):
        analysis.parzen_from_sums(R, labels[:2], counts)
    with pytest.raises(ValueError):
        analysis.parzen_from_sums(R, labels, counts[:2])
    with pytest.raises(ValueError):
        analysis.parzen_from_sums(R, np.array([0, 1, 3]), counts)        # a label outside [-1, G)
    with pytest.raises(ValueError):
        analysis.witness_from_sums(R, labels, counts, 0, 0)
    with pytest.raises(ValueError):
        analysis.witness_from_sums(R, labels, counts, 0, 3)


def test_witness_and_its_identity_with_mmd():
    x, labels = planted(60, 5, 2)
    G = 3
    counts = np.bincount(labels, minlength=G)
    Kd = dense_kernels(x)
    R = row_sums(Kd, labels, G)
    onehot = (labels[:, None] == np.arange(G)[None, :]).astype(np.float64)
    ordered = np.einsum("ia,lij,jb->lab", onehot, Kd * (1.0 - np.eye(60))[None], onehot)
    K = ordered.copy()
    K[:, np.arange(G), np.arange(G)] /= 2.0                              # unordered pairs, as the bucket kernel returns them
    mmd2 = analysis.mmd_from_sums(K, counts)["mmd2"]
    for a, b in ((0, 1), (2, 0), (1, 2)):
        w = analysis.witness_from_sums(R, labels, counts, a, b)
        assert w.shape == (3, 60)
        for i in (0, 17, 59):
            for l in range(3):
                da = sum(Kd[l, i, j] for j in range(60) if j != i and labels[j] == a) / (counts[a] - (labels[i] == a))
                db = sum(Kd[l, i, j] for j in range(60) if j != i and labels[j] == b) / (counts[b] - (labels[i] == b))
                assert abs(w[l, i] - (da - db)) <= 1e-14
        ident = w[:, labels == a].mean(1) - w[:, labels == b].mean(1)
        np.testing.assert_allclose(ident, mmd2[:, a, b], rtol=1e-11, atol=1e-15)


def test_alignment_matches_the_dense_traces():
    x, labels = planted(60, 5, 3, G=4)
    labels[labels == 3] = 1                                              # an empty label among the four
    G, N = 4, 60
    counts = np.bincount(labels, minlength=G)
    Kd = dense_kernels(x)
    R = row_sums(Kd, labels, G)
    onehot = (labels[:, None] == np.arange(G)[None, :]).astype(np.float64)
    S = np.einsum("ia,lig->lag", onehot, R)
    K = 0.5 * (S + S.transpose(0, 2, 1))
    K[:, np.arange(G), np.arange(G)] = 0.5 * S[:, np.arange(G), np.arange(G)]
    K2 = np.array([np.triu(k * k, 1).sum() for k in Kd])
    rows = 1.0 + R.sum(2)
    got = analysis.alignment_from_sums(K, K2, (rows * rows).sum(1), counts)
    H = np.eye(N) - 1.0 / N
    Lm = onehot @ onehot.T
    for l in range(3):
        kl, kk, ll = np.trace(Kd[l] @ H @ Lm @ H), np.trace(Kd[l] @ H @ Kd[l] @ H), np.trace(Lm @ H @ Lm @ H)
        assert abs(got["alignment"][l] - kl / np.sqrt(kk * ll)) <= 1e-12
        assert abs(got["hsic"][l] - kl / N ** 2) <= 1e-14 and abs(got["hsic_kk"][l] - kk / N ** 2) <= 1e-14
        assert abs(got["hsic_ll"] - ll / N ** 2) <= 1e-14
        # the bound, term by term from the dense matrices
        p = counts / N
        w = np.eye(G) - p[:, None] - p[None, :] + (p * p).sum()
        full = onehot.T @ Kd[l] @ onehot
        b_kl = 1e-4 * (full * np.abs(w)).sum() / N ** 2
        A, B, C = (Kd[l] ** 2).sum(), (Kd[l].sum(1) ** 2).sum(), Kd[l].sum()
        b_kk = 1e-4 * (A + 4 * B / N + 2 * C * C / N ** 2) / N ** 2
        want = b_kl / abs(kl / N ** 2) + 0.5 * b_kk / (kk / N ** 2)
        assert abs(got["rel_bound"][l] - want) <= 1e-10 * want
    assert set(got) == {"alignment", "hsic", "hsic_kk", "hsic_ll", "rel_bound"}
    assert (got["alignment"] > 0).all() and (got["alignment"] < 1).all()
    with pytest.raises(ValueError):
        analysis.alignment_from_sums(K, K2[:2], (rows * rows).sum(1), counts)
    with pytest.raises(ValueError):
        analysis.alignment_from_sums(K, K2, (rows * rows).sum(1), counts[:3])


def test_refusals_come_before_a_device_is_touched():
    """host tensors throughout: a refusal that needed the device would raise DbmmError (there is no CPU path) instead"""
    x = torch.zeros(40, 64)
    with pytest.raises(ValueError):
        analysis.kernel_probe(x, np.zeros(40, dtype=np.int64))           # one label
    with pytest.raises(ops.DbmmUnsupported):
        analysis.kernel_probe(x, np.arange(40) % 17)
    with pytest.raises(ValueError):
        analysis.kernel_alignment(x, np.zeros(40, dtype=np.int64))
    with pytest.raises(ops.DbmmUnsupported):
        analysis.kernel_alignment(x, np.arange(40) % 17)
    with pytest.raises(ValueError):
        analysis.kernel_probe(x, query=torch.zeros(3, 64))               # query rows without reference labels
    with pytest.raises(ValueError):
        analysis.kernel_probe(x, np.arange(40) % 2, prior="flat")
    with pytest.raises(ValueError):
        analysis.kernel_probe(x, np.arange(39) % 2)                      # one label short
    with pytest.raises(ops._lib.DbmmError):
        ops.pairdist_rbf_row_group_sums(x, torch.zeros(40, dtype=torch.int64), 2, torch.zeros(64), [0.0])      # gammas first, on the host
    with pytest.raises(ops._lib.DbmmError):
        ops.pairdist_rbf_row_group_sums(x, torch.zeros(40, dtype=torch.int64), 2, torch.zeros(64), [1.0] * 5)


def test_entry_refuses_its_operands_without_a_device():
    """the C entry's own checks, with host pointers: nothing is launched"""
    import ctypes
    from dbmm_amd import _lib
    L = _lib.lib()
    assert L.dbmm_workspace_bytes_pairdist_rbf_rows(1000, 64, 4, 1) == L.dbmm_workspace_bytes_pairdist_rows(1000, 64, 4)
    assert (L.dbmm_workspace_bytes_pairdist_rbf_rows(1000, 64, 4, 4) - L.dbmm_workspace_bytes_pairdist_rbf_rows(1000, 64, 4, 1)
            == 3 * 16 * 1000 * 4 * 8)
    partials = 16 * 4 * 162770 * 4 * 8                                   # CelebA's train split, 4 labels, 4 bandwidths: 333 MB
    assert L.dbmm_workspace_bytes_pairdist_rbf_rows(162770, 1024, 4, 4) - L.dbmm_workspace_bytes_pairdist_rows(162770, 1024, 4) == partials * 3 // 4
    for bad in ((1000, 64, 17, 1), (1000, 64, 0, 1), (1000, 64, 4, 5), (1000, 64, 4, 0), (0, 64, 4, 1)):
        assert L.dbmm_workspace_bytes_pairdist_rbf_rows(*bad) == 0, bad
    buf = (ctypes.c_double * 64)()
    p = (ctypes.addressof(buf) + 15) // 16 * 16
    gam = (ctypes.c_double * 4)(1.0, 2.0, 3.0, 4.0)
    call = lambda N, D, G, Lb, g=gam, ws=1 << 40, x=p: L.dbmm_pairdist_rbf_row_group_sums(x, p, p, ctypes.addressof(g), Lb, p, N, D, G, p, ws, None)
    assert call(1000, 64, 17, 1) == -1 and call(1000, 64, 4, 5) == -1 and call(0, 64, 4, 1) == -1 and call((1 << 23) + 1, 64, 4, 1) == -1
    assert call(1000, 96, 4, 1) == -5 and call(1000, 8192, 4, 1) == -5
    assert call(1000, 64, 4, 2, g=(ctypes.c_double * 2)(1.0, 0.0)) == -4
    assert call(1000, 64, 4, 2, g=(ctypes.c_double * 2)(1.0, float("inf"))) == -4
    assert call(1000, 64, 4, 2, g=(ctypes.c_double * 2)(float("nan"), 1.0)) == -4
    assert call(1000, 64, 4, 1, x=p + 4) == -2
    assert call(1000, 64, 4, 4, ws=L.dbmm_workspace_bytes_pairdist_rbf_rows(1000, 64, 4, 4) - 1) != 0


# What the pairwise-kernel family shares on the Python side: one driver in ops.py, one labelled-rows front end, one
# sorted-by-label pass and one spelling of each refusal in analysis.py.  A wrapper or report that carries its own copy again fails here
# (source scan with the comments stripped, no compute), as tests/test_csrc_shared_helpers.py does for the library.
def _python_source(name, section=None):
    import os
    import re
    txt = open(os.path.join(os.path.dirname(os.path.abspath(ops.__file__)), name)).read()
    if section is not None:
        txt = txt[txt.index(section[0]):txt.index(section[1])]
    return re.sub(r"#[^\n]*", "", txt)


@pytest.mark.parametrize("name,section,statement", [
    ("ops.py", ("PAIRDIST_RBF_MAX_L = 4", "def covariance("), "ws.numel() * 4"),                        # the C call of _pairdist
    ("analysis.py", None, 'np.argsort(dense, kind="stable")'),                                         # _sorted_pass
    ("analysis.py", None, "is None else np.asarray(gammas, dtype=np.float64).ravel()"),                # _resolved_gammas
    ("analysis.py", None, "there is no CPU path"),                                                     # _need_device
])
def test_pairwise_family_statement_stated_once(name, section, statement):
    assert _python_source(name, section).count(statement) == 1
