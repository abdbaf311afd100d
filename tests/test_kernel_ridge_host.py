"""The host half of the kernel ridge probe, without a GPU: analysis.cg_solve against torch.linalg.solve, the fit's and the
prediction's host steps on a dense float64 operator against the closed form (K + lam I)^-1 T, the stratified hold-out, every
refusal before any call into the library, and, for include/dbmm_kernel_ops.h, what test_abi.py and the operand audit do for
include/dbmm.h: the names it declares are the ones _lib._SIGS_KERNEL_OPS binds, the built library exports them, the entry answers
its error codes in the documented order, and the pointers ops.pairdist_rbf_matvec hands it resolve to tensors of the dtypes and
element counts the header implies.  Every test prints its figures before it asserts."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT
from dbmm_amd import _lib, analysis, ops
from ops_audit import Registry

F64 = torch.float64


# ---- cg_solve -------------------------------------------------------------------------------------------------------------------------

def spd(n, seed, cond=None):
    g = torch.Generator().manual_seed(seed)
    Q, _ = torch.linalg.qr(torch.randn(n, n, generator=g, dtype=F64))
    w = torch.rand(n, generator=g, dtype=F64) + 0.05 if cond is None else torch.logspace(0, -np.log10(cond), n, dtype=F64)
    return (Q * w) @ Q.T


def dense_solve(M, B, shifts):
    eye = torch.eye(M.shape[0], dtype=F64)
    return torch.stack([torch.linalg.solve(M + s * eye, B[:, c]) for c, s in enumerate(shifts)], 1)


@pytest.mark.parametrize("C", [1, 5, 16])
def test_cg_solve_matches_the_dense_solve_within_kappa_tol(C):
    n, tol = 40, 1e-8
    M = spd(n, 100 + C)
    g = torch.Generator().manual_seed(C)
    B = torch.randn(n, C, generator=g, dtype=F64)
    shifts = np.linspace(0.05, 2.0, C)                                  # a different shift per column
    calls = []

    def matvec(V):
        calls.append(1)
        return M @ V
    sol = analysis.cg_solve(matvec, B, shifts, tol=tol, max_iter=200)
    X = dense_solve(M, B, shifts)
    assert sol["x"].dtype == F64 and sol["x"].shape == (n, C)
    assert len(calls) == sol["iterations"] + 1, "one product per iteration for all columns, and one for the true residual"
    ev = torch.linalg.eigvalsh(M)
    for c, s in enumerate(shifts):
        kappa = ((ev[-1] + s) / (ev[0] + s)).item()
        err = ((sol["x"][:, c] - X[:, c]).norm() / X[:, c].norm()).item()
        print(f"C={C} column {c}: shift {s:.3f} kappa {kappa:.1f} rel err {err:.3e} (bound {kappa * tol:.3e}) residual {sol['residual'][c].item():.3e}")
        assert err <= kappa * tol
        assert sol["residual"][c].item() <= 2 * tol
    assert bool(sol["converged"].all())


def test_cg_solve_zero_column_frozen_columns_and_bits():
    n = 40
    M = spd(n, 7)
    B = torch.randn(n, 4, generator=torch.Generator().manual_seed(8), dtype=F64)
    B[:, 2] = 0
    shifts = [0.1, 1.0, 0.5, 50.0]
    seen = []

    def matvec(V):
        seen.append((V != 0).any(0).clone())
        return M @ V
    a = analysis.cg_solve(matvec, B, shifts, tol=1e-9, max_iter=200)
    b = analysis.cg_solve(lambda V: M @ V, B, shifts, tol=1e-9, max_iter=200)
    assert (a["x"][:, 2] == 0).all() and a["residual"][2].item() == 0 and bool(a["converged"][2]), "a zero right-hand side gives exact zeros"
    assert not any(bool(s[2]) for s in seen[:-1]), "the zero column's direction is handed over as zeros"
    # the column with the large shift converges first and is handed over as zeros from then on
    first_zero = [i for i, s in enumerate(seen[:-1]) if not bool(s[3])]
    print(f"iterations {a['iterations']}; column 3 frozen from product {first_zero[0] if first_zero else None}")
    assert first_zero and first_zero[0] < a["iterations"] - 1 and all(not bool(s[3]) for s in seen[first_zero[0]:-1])
    assert torch.equal(a["x"], b["x"]) and torch.equal(a["residual"], b["residual"]) and a["iterations"] == b["iterations"], "two runs differ in bits"


def test_cg_solve_reports_non_convergence_with_the_true_residual():
    n = 40
    M = spd(n, 9, cond=1e8)
    B = torch.randn(n, 3, generator=torch.Generator().manual_seed(10), dtype=F64)
    shifts = [1e-9, 1e-8, 1e-7]
    sol = analysis.cg_solve(lambda V: M @ V, B, shifts, tol=1e-10, max_iter=2)
    eye = torch.eye(n, dtype=F64)
    dense = torch.stack([(B[:, c] - (M + s * eye) @ sol["x"][:, c]).norm() / B[:, c].norm() for c, s in enumerate(shifts)])
    print(f"max_iter = 2: iterations {sol['iterations']}, converged {sol['converged'].tolist()}, residual {sol['residual'].tolist()}, dense {dense.tolist()}")
    assert sol["iterations"] == 2 and not bool(sol["converged"].any())
    assert (sol["residual"] - dense).abs().max().item() <= 1e-12
    assert (sol["residual"] > 1e-3).all()


# ---- the fit's and the prediction's host steps on a dense operator ---------------------------------------------------------------------

def ridge_case():
    g = torch.Generator().manual_seed(3)
    N, M, D = 60, 25, 8
    x = torch.randn(N + M, D, generator=g, dtype=F64)
    dense = np.concatenate([np.zeros(31, dtype=np.int64), np.ones(28, dtype=np.int64), [2]])      # label 2 has a single row
    x[:N] += torch.as_tensor(dense, dtype=F64).unsqueeze(1)
    gammas = [0.02, 0.08]
    lams = np.array([0.1, 1.0])
    d2 = torch.cdist(x, x) ** 2
    K0 = {gam: torch.exp(-gam * d2) * (1.0 - torch.eye(N + M, dtype=F64)) for gam in gammas}
    return x, dense, gammas, lams, K0, N, M


def test_ridge_host_steps_match_the_closed_form():
    x, dense, gammas, lams, K0, N, M = ridge_case()
    G, tol = 3, 1e-10
    calls = []

    def fit_product(gam, V):
        calls.append(V.shape)
        return K0[gam][:N, :N] @ V
    alpha, its, res, conv, freq = analysis._ridge_from_operator(fit_product, dense, G, gammas, lams, tol, 256, "cpu")
    assert alpha.shape == (2, 2, N, G) and alpha.dtype == F64 and its.shape == (2,) and res.shape == (2, 2, G) and conv.shape == (2, 2, G)
    assert all(s == (N, 2 * G) for s in calls) and len(calls) == int(its.sum()) + 2, "one product per iteration carries every (lam, label) column"
    counts = np.bincount(dense, minlength=G)
    assert np.array_equal(freq, counts / N)
    T = torch.nn.functional.one_hot(torch.as_tensor(dense), G).double() - torch.as_tensor(freq)
    eye = torch.eye(N, dtype=F64)
    for l, gam in enumerate(gammas):
        for a, lam in enumerate(lams):
            A = K0[gam][:N, :N] + (1.0 + lam) * eye                     # K + lam I, K with its unit diagonal
            want = torch.linalg.solve(A, T)
            ev = torch.linalg.eigvalsh(A)
            kappa = (ev[-1] / ev[0]).item()
            err = ((alpha[l, a] - want).norm(dim=0) / want.norm(dim=0)).max().item()
            print(f"gamma {gam} lam {lam}: kappa {kappa:.1f}, {its[l]} iterations, rel err {err:.3e} (bound {kappa * tol:.3e}), residual {res[l, a]}")
            assert err <= kappa * tol and conv[l, a].all() and (res[l, a] <= 2 * tol).all()
    # predictions: the rows [train; query] with the weights [alpha; 0]
    seen = []

    def predict_product(gam, W):
        seen.append(W)
        return K0[gam] @ W
    scores, pred, margin = analysis._ridge_scores(predict_product, alpha, freq, gammas, M)
    assert scores.shape == (2, 2, M, G) and pred.shape == (2, 2, M) and margin.shape == (2, 2, M)
    assert all(W.shape == (N + M, 2 * G) and (W[N:] == 0).all() for W in seen) and len(seen) == 2
    for l, gam in enumerate(gammas):
        for a, lam in enumerate(lams):
            want = (K0[gam][N:, :N] @ torch.linalg.solve(K0[gam][:N, :N] + (1.0 + lam) * eye, T)).numpy() + freq
            diff = np.abs(scores[l, a] - want).max()
            print(f"gamma {gam} lam {lam}: max score diff {diff:.3e}")
            assert diff <= 1e-7
            assert np.array_equal(pred[l, a], want.argmax(1))
            top = np.sort(want, axis=1)
            assert np.allclose(margin[l, a], top[:, -1] - top[:, -2], atol=1e-7)


def test_ridge_best_breaks_ties_toward_the_smaller_gamma_then_the_larger_lam():
    gammas, lams = np.array([0.4, 0.1, 0.2]), np.array([0.1, 1.0])
    bal = np.array([[0.9, 0.9], [0.9, 0.9], [0.5, 0.9]])
    best = analysis._ridge_best(bal, gammas, lams)
    assert best["index"] == (1, 1) and best["gamma"] == 0.1 and best["lam"] == 1.0 and best["balanced_accuracy"] == 0.9
    bal[0, 0] = 0.95
    assert analysis._ridge_best(bal, gammas, lams)["index"] == (0, 0)


# ---- the stratified hold-out -----------------------------------------------------------------------------------------------------------

def test_stratified_holdout():
    rng = np.random.RandomState(0)
    dense = rng.randint(0, 5, 400)
    dense[:2] = 5                                                       # a label with two rows: one on each side
    keep, held = analysis.stratified_holdout(dense, 0.25, seed=3)
    keep2, held2 = analysis.stratified_holdout(dense, 0.25, seed=3)
    _, other = analysis.stratified_holdout(dense, 0.25, seed=4)
    assert np.array_equal(keep, keep2) and np.array_equal(held, held2) and not np.array_equal(held, other), "deterministic in the seed"
    assert len(np.intersect1d(keep, held)) == 0 and np.array_equal(np.sort(np.concatenate([keep, held])), np.arange(400))
    for g in range(6):
        n, k = (dense == g).sum(), (dense[held] == g).sum()
        print(f"label {g}: {k} of {n} rows held out")
        assert 1 <= k <= n - 1 and abs(k - 0.25 * n) <= 1
    state = np.random.get_state()[1].copy()
    analysis.stratified_holdout(dense, 0.25, seed=3)
    assert np.array_equal(np.random.get_state()[1], state), "the draw must come from a private generator"
    # a label's only row stays with the fit
    keep, held = analysis.stratified_holdout(np.array([0, 0, 0, 0, 1, 1, 1, 2]), 0.25, 0)
    assert 7 in keep and 7 not in held


# ---- refusals, before anything reaches the library ------------------------------------------------------------------------------------

class Untouched:
    """stand-in for _lib.lib: any use of the library is recorded"""

    def __init__(self):
        self.used = []

    def __call__(self):
        self.used.append("lib()")
        return self

    def __getattr__(self, name):
        self.used.append(name)
        raise AssertionError(f"the library was reached: {name}")


def test_refusals_come_before_any_call(monkeypatch):
    stub = Untouched()
    monkeypatch.setattr(_lib, "lib", stub)
    x = torch.randn(40, 64)
    two = np.arange(40) % 2
    with pytest.raises(ops.DbmmUnsupported):
        analysis.kernel_ridge_fit(x, np.arange(40) % 17)                # 17 labels
    with pytest.raises(ops.DbmmUnsupported):
        analysis.kernel_ridge_fit(x, np.arange(40) % 6, lams=(0.1, 1.0, 10.0))   # 3 x 6 = 18 columns
    with pytest.raises(ops.DbmmUnsupported):
        analysis.kernel_ridge_probe(x, np.arange(40) % 6, lams=(0.1, 1.0, 10.0))
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            analysis.kernel_ridge_fit(x, two, lams=(1.0, bad))
    with pytest.raises(ValueError):
        analysis.kernel_ridge_fit(x, np.zeros(40, dtype=np.int64))      # one label
    for bad in (0.0, 1.0, -0.1, 1.5):
        with pytest.raises(ValueError):
            analysis.kernel_ridge_probe(x, two, holdout=bad)
    with pytest.raises(_lib.DbmmError) as e:
        analysis.kernel_ridge_fit(x, two)                               # a CPU tensor
    assert not isinstance(e.value, ops.DbmmUnsupported)
    with pytest.raises(_lib.DbmmError):
        analysis.kernel_ridge_probe(x, two)
    with pytest.raises(_lib.DbmmError):
        analysis.kernel_ridge_probe(x, two, query=x, query_labels=two)
    with pytest.raises(_lib.DbmmError):
        ops.pairdist_rbf_matvec(x, torch.randn(40, 2), x.mean(0), 0.1)  # CPU tensors
    for bad in (0.0, -1.0, float("nan"), float("inf"), "wide", [0.1, 0.2]):
        with pytest.raises(_lib.DbmmError):
            ops.pairdist_rbf_matvec(x, torch.randn(40, 2), x.mean(0), bad)
    with pytest.raises(ValueError):
        analysis.cg_solve(lambda V: V, torch.zeros(4, 2, dtype=F64), [1.0])
    print(f"library uses: {stub.used}")
    assert stub.used == []


# ---- include/dbmm_kernel_ops.h --------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def built():
    return _lib.build()


def _declared(header):
    txt = open(os.path.join(ROOT, "include", header)).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(dbmm_[a-z0-9_]+)\s*\(", txt)))


def test_the_new_header_and_its_binding_table(built):
    names = _declared("dbmm_kernel_ops.h")
    print(f"declared: {names}")
    assert names == sorted(_lib._SIGS_KERNEL_OPS) == ["dbmm_pairdist_rbf_matvec", "dbmm_workspace_bytes_pairdist_rbf_matvec"]
    assert not set(names) & set(_declared("dbmm.h")) and not set(names) & set(_lib.EXPORTS) and not set(names) & set(_lib._SIGS)
    raw = ctypes.CDLL(built)
    for n in names:
        assert hasattr(raw, n), f"{n} declared in include/dbmm_kernel_ops.h but not exported"
    L = _lib.lib()
    P, I, Z = ctypes.c_void_p, ctypes.c_int64, ctypes.c_size_t
    assert L.dbmm_pairdist_rbf_matvec.argtypes == [P, P, P, ctypes.c_double, P, I, I, I, P, Z, P] and L.dbmm_pairdist_rbf_matvec.restype is ctypes.c_int
    assert L.dbmm_workspace_bytes_pairdist_rbf_matvec.argtypes == [I, I, I] and L.dbmm_workspace_bytes_pairdist_rbf_matvec.restype is Z
    for n in _lib.EXPORTS:                                              # the first table is still bound beside it
        assert getattr(L, n).argtypes == _lib._SIGS[n]
    # the header's text: C linkage, the error codes of dbmm.h, and the note on folding it in
    txt = open(os.path.join(ROOT, "include", "dbmm_kernel_ops.h")).read()
    assert 'extern "C"' in txt and '#include "dbmm.h"' in txt and "folds this header into dbmm.h" in txt


def test_the_entry_refuses_in_the_documented_order(built):
    """host pointers: every refusal comes before anything touches a device"""
    L = _lib.lib()
    SHAPE, ALIGN, WORKSPACE, ARG, UNSUPPORTED = -1, -2, -3, -4, -5
    buf = (ctypes.c_char * 4096)()
    base = ctypes.addressof(buf)
    al = base + (-base) % 16                                            # a 16-byte aligned host address, and one that is not
    off = al + 4
    size = L.dbmm_workspace_bytes_pairdist_rbf_matvec
    assert [size(0, 64, 1), size(-1, 64, 1), size(8, 0, 1), size(8, 64, 0), size(8, 64, 17)] == [0] * 5
    need = size(300, 64, 3)
    print(f"workspace of (300, 64, 3): {need} bytes; dbmm_workspace_bytes_pairdist_rows: {L.dbmm_workspace_bytes_pairdist_rows(300, 64, 3)}")
    assert need == L.dbmm_workspace_bytes_pairdist_rows(300, 64, 3) and need >= 16 * 300 * 3 * 8 + 300 * 128 * 4
    call = lambda x=al, v=al, c=al, gamma=0.5, out=al, N=300, D=64, C=3, ws=al, wsb=need: L.dbmm_pairdist_rbf_matvec(x, v, c, gamma, out, N, D, C, ws, wsb, None)
    # shape first: whatever else is wrong
    for kw in (dict(N=0), dict(N=-5), dict(N=(1 << 23) + 1), dict(C=0), dict(C=17), dict(D=0)):
        assert call(x=None, gamma=0.0, ws=off, wsb=0, **dict(dict(D=65), **kw)) == SHAPE, kw
    # then the widths the kernel serves
    for D in (65, 32, 4160):
        assert call(x=None, gamma=0.0, ws=off, wsb=0, D=D) == UNSUPPORTED, D
    # then null pointers, then gamma
    for name in ("x", "v", "c", "out", "ws"):
        assert call(gamma=float("nan"), wsb=0, **{name: None}) == ARG, name
    for gamma in (0.0, -1.0, float("nan"), float("inf")):
        assert call(gamma=gamma, x=off, wsb=0) == ARG, gamma
    # then alignment, then the workspace size
    for name in ("x", "v", "c", "ws"):
        assert call(wsb=0, **{name: off}) == ALIGN, name
    assert call(wsb=need - 1) == WORKSPACE and call(wsb=0) == WORKSPACE
    assert call(N=1 << 23, wsb=0) == WORKSPACE                          # the largest N is a shape the entry takes


class RecordingStub:
    """stand-in for the loaded library for the entries of include/dbmm_kernel_ops.h: the size query is answered, the call recorded"""
    WS_BYTES = 4096 + 4                                                 # not a multiple of 16: the wrapper must round up, not down

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        if name not in _lib._SIGS_KERNEL_OPS:
            raise AttributeError(name)

        def entry(*args):
            assert len(args) == len(_lib._SIGS_KERNEL_OPS[name])
            if "_bytes" in name:
                return self.WS_BYTES
            self.calls.append((name, args))
            return 0
        return entry


def test_the_wrapper_hands_the_entry_operands_of_the_implied_extents(monkeypatch):
    """the operand audit of tests/ops_audit.py for this entry: x N D fp32, v N C fp32, center D fp32, out N C float64, a workspace of
    workspace_bytes bytes -- each pointer resolved to a registered tensor"""
    stub, reg = RecordingStub(), Registry()
    monkeypatch.setattr(_lib, "lib", lambda: stub)
    monkeypatch.setattr(ops, "require_cuda", lambda *t: None)
    monkeypatch.setattr(ops, "stream", lambda: None)
    monkeypatch.setattr(ops, "_empty", reg.empty)
    N, D, C = 37, 128, 5
    x, v, center = reg.add(torch.randn(N, D)), reg.add(torch.randn(N, C)), reg.add(torch.randn(D))
    out = ops.pairdist_rbf_matvec(x, v, center, 0.25)
    assert out.shape == (N, C) and out.dtype == F64 and len(stub.calls) == 1
    name, a = stub.calls[0]
    px, pv, pc, gamma, pout, n, d, c, pws, wsb, stream = a
    assert name == "dbmm_pairdist_rbf_matvec" and (n, d, c) == (N, D, C) and gamma == 0.25 and stream is None
    for what, address, dtype, count in (("x", px, torch.float32, N * D), ("v", pv, torch.float32, N * C), ("center", pc, torch.float32, D),
                                        ("out", pout, F64, N * C)):
        t = reg.find(address)
        assert t is not None, f"{what}: pointer {address} is no registered tensor"
        left = (t.data_ptr() + t.numel() * t.element_size() - address) // t.element_size()
        print(f"{what}: {t.dtype} {tuple(t.shape)}, {left} elements from the pointer, the entry indexes {count}")
        assert t.dtype == dtype and t.is_contiguous() and left >= count
    assert pout == out.data_ptr()
    ws = reg.find(pws)
    assert ws is not None and wsb >= RecordingStub.WS_BYTES and ws.data_ptr() + ws.numel() * ws.element_size() - pws >= wsb
    # operands the wrapper must refuse: nothing more is recorded
    bad = [dict(x=x.double()), dict(x=x[:, ::2]), dict(x=torch.randn(N, 96)), dict(v=v.double()), dict(v=v.t().contiguous().t()),
           dict(v=torch.randn(N - 1, C)), dict(v=torch.randn(N, 17)), dict(v=torch.randn(N)), dict(v=torch.randn(N, 0)),
           dict(center=torch.randn(D - 1)), dict(center=center.double()), dict(v=v.numpy())]
    for kw in bad:
        args = dict(x=x, v=v, center=center)
        args.update(kw)
        with pytest.raises(_lib.DbmmError):
            ops.pairdist_rbf_matvec(args["x"], args["v"], args["center"], 0.25)
    assert len(stub.calls) == 1
