"""The device eigen-solver of `analysis.pca` on the MI355X: ops.sym_eig_topk (csrc/sym_eig.hip) against numpy.linalg.eigh, against
an independent float64 residual and against the numpy restatement's iteration count; determinism and the no-op rule; the cases
that do not converge or break down; analysis.pca(solver="device") end to end; the default path unchanged; guard zones.

The bounds, with tol the solver's tolerance, D the order, lambda_1 the largest eigenvalue:
  eigenvalues   |theta_j - lambda_j| <= (2 tol + D 2^-52) lambda_1
  vectors       sin angle(v_j, u_j)  <= (2 tol + D 2^-52) lambda_1 / gap_j   (Davis-Kahan for a Ritz pair of residual tol lambda_1; the
                second term is LAPACK's own backward error), the sine as ||v - (v . u) u||
  residual      ||C v_j - theta_j v_j|| <= (2 tol + D 2^-52) theta_1 in numpy float64 from the returned pairs
  orthogonality |v_i . v_j| <= (r_i + r_j) / |theta_i - theta_j|, | ||v_j|| - 1 | <= D 2^-52
  iterations    <= it_ref + max(2, it_ref // 4) of the restatement on the same matrix
Every test prints its figures before it asserts."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from test_gpu_pca import GuardedAlloc, case, check_projection
from test_pca_eig_host import EIGHT_SHAPES, centred_scatter, eight_planted, powerlaw, restated
from test_pca_host import SHAPES, eig_desc, gaps, planted

pytestmark = pytest.mark.gpu

TOL = 1e-12
EPS52 = 2.0 ** -52

_mats = {}


def matrix(name):
    """(C float64 numpy symmetric to the bit, C on the device), made once per name and left unchanged"""
    if name not in _mats:
        kind, a, b = name
        if kind == "eight":
            C = centred_scatter(eight_planted(a, b))
        elif kind == "planted":
            C = centred_scatter(planted(a, b))
        else:
            C = powerlaw(a, b)
        C = (C + C.T) / 2
        _mats[name] = (C, torch.from_numpy(C).cuda())
    return _mats[name]


_eigh = {}


def eigh_of(name):
    if name not in _eigh:
        _eigh[name] = eig_desc(matrix(name)[0])
    return _eigh[name]


def bound(D, tol=TOL):
    return 2 * tol + D * EPS52


def solve(name, k, tol=TOL, **kw):
    from dbmm_amd import ops
    C, Cd = matrix(name)
    vals, vecs, info = ops.sym_eig_topk(Cd, k, tol=tol, **kw)
    assert vals.is_cuda and vecs.is_cuda and vals.dtype == torch.float64 and vecs.dtype == torch.float64
    assert tuple(vals.shape) == (k,) and tuple(vecs.shape) == (k, C.shape[0])
    assert set(info) == {"iterations", "converged", "state", "residual"}
    return vals.cpu().numpy(), vecs.cpu().numpy(), info


def check_residual(C, th, V, tol, what):
    """check 2: the independent residual, orthogonality and unit norm, from the returned pairs and the input matrix alone"""
    D, k = C.shape[0], len(th)
    R = C @ V.T - V.T * th
    r = np.linalg.norm(R, axis=0)
    norms = np.linalg.norm(V, axis=1)
    print(f"{what}: ||C v - theta v|| / theta_1 {r / th[0]} (bound {bound(D, tol):.3e}); | ||v|| - 1 | max {np.abs(norms - 1).max():.3e} "
          f"(bound {D * EPS52:.3e})")
    worst = 0.0
    for i in range(k):
        for j in range(i + 1, k):
            dot, lim = abs(V[i] @ V[j]), (r[i] + r[j]) / abs(th[i] - th[j])
            worst = max(worst, dot / lim if lim > 0 else np.inf)
    print(f"{what}: worst |v_i . v_j| / ((r_i + r_j) / |theta_i - theta_j|) = {worst:.3e}")
    assert np.isfinite(V).all() and np.isfinite(th).all()
    assert (r <= bound(D, tol) * th[0]).all()
    assert (np.abs(norms - 1) <= D * EPS52).all()
    assert worst <= 1.0


def check_against_eigh(name, th, V, tol, what):
    C = matrix(name)[0]
    D, k = C.shape[0], len(th)
    w, U = eigh_of(name)
    gap = gaps(w)[:k]
    e_val = np.abs(th - w[:k])
    sin = np.array([np.linalg.norm(V[j] - (V[j] @ U[j]) * U[j]) for j in range(k)])
    print(f"{what}: |theta - lambda| / lambda_1 {e_val / w[0]} (bound {bound(D, tol):.3e}); sin angle / bound {sin / (bound(D, tol) * w[0] / gap)}")
    assert (e_val <= bound(D, tol) * w[0]).all()
    assert (sin <= bound(D, tol) * w[0] / gap).all()


def check_iterations(name, C, k, tol, info, max_iter=256):
    it_ref = restated(name, C, k, tol, max_iter)[2]
    print(f"{name} k={k}: {info['iterations']} iterations on the device, {it_ref} in the restatement, residual {info['residual']:.3e}")
    assert info["iterations"] <= it_ref + max(2, it_ref // 4)


# ---- 1, 2, 3. against eigh, the independent residual, the iteration count ------------------------------------------------------------------

@pytest.mark.parametrize("k", [1, 2, 8])
@pytest.mark.parametrize("N,D", EIGHT_SHAPES)
def test_eight_planted_against_eigh(N, D, k):
    name = ("eight", N, D)
    th, V, info = solve(name, k)
    print(f"N={N} D={D} k={k}: {info}")
    assert info["converged"] and info["state"] == "converged" and info["residual"] <= TOL
    assert (np.diff(th) <= 0).all()
    check_against_eigh(name, th, V, TOL, f"N={N} D={D} k={k}")
    check_residual(matrix(name)[0], th, V, TOL, f"N={N} D={D} k={k}")
    check_iterations(name, matrix(name)[0], k, TOL, info)


def test_powerlaw_residual_and_iterations():
    name = ("powerlaw", 256, 0.5)
    th, V, info = solve(name, 8)
    print(f"powerlaw(256, 0.5) k=8: {info}")
    assert info["converged"]
    check_residual(matrix(name)[0], th, V, TOL, "powerlaw(256, 0.5) k=8")
    check_iterations(name, matrix(name)[0], 8, TOL, info)


def test_largest_order_residual():
    """D = 4096, the largest order served: no eigh here, the independent residual only"""
    name = ("eight", 600, 4096)
    th, V, info = solve(name, 8)
    print(f"eight_planted(600, 4096) k=8: {info}")
    assert info["converged"]
    check_residual(matrix(name)[0], th, V, TOL, "eight_planted(600, 4096) k=8")
    check_iterations(name, matrix(name)[0], 8, TOL, info)


# ---- 4. determinism and the no-op rule ------------------------------------------------------------------------------------------------------

def test_two_calls_and_every_check_interval_give_the_same_bits():
    from dbmm_amd import ops
    name = ("eight", 300, 128)
    Cd = matrix(name)[1]
    state = np.random.get_state()[1].copy()
    vals, vecs, info = ops.sym_eig_topk(Cd, 8, tol=TOL)
    vals2, vecs2, info2 = ops.sym_eig_topk(Cd, 8, tol=TOL)
    print(f"default: {info}")
    assert torch.equal(vals, vals2) and torch.equal(vecs, vecs2) and info == info2
    for every in (1, 4, 32):
        v, x, i = ops.sym_eig_topk(Cd, 8, tol=TOL, check_every=every)
        print(f"check_every={every}: {i}")
        assert torch.equal(v, vals) and torch.equal(x, vecs), f"check_every={every} changed the result"
        assert i == info
    assert np.array_equal(np.random.get_state()[1], state), "sym_eig_topk moved the global numpy stream"


# ---- 5. not converged ------------------------------------------------------------------------------------------------------------------------

def test_flat_bulk_is_reported_and_pca_falls_back():
    from dbmm_amd import analysis
    name = ("planted", 300, 128)
    th, V, info = solve(name, 8, tol=1e-10, max_iter=24)
    print(f"planted(300, 128) k=8 max_iter=24: {info}")
    assert not info["converged"] and info["iterations"] == 24 and info["state"] == "running"
    assert np.isfinite(th).all() and np.isfinite(V).all()
    x, xd, _ = case(300, 128)
    g = np.arange(300) % 4
    host = analysis.pca(xd, g, k=8, solver="host")
    dev = analysis.pca(xd, g, k=8, solver="device", max_iter=24)
    print(f"pca(solver='device', max_iter=24): eig {dev['eig']}")
    assert dev["eig"]["used"] == "host" and not dev["eig"]["converged"] and dev["eig"]["iterations"] == 24
    assert np.array_equal(dev["components"], host["components"]) and np.array_equal(dev["explained_variance"], host["explained_variance"])
    assert torch.equal(dev["coords"], host["coords"])
    th, V, info = solve(name, 8, tol=1e-10, max_iter=256)
    print(f"planted(300, 128) k=8 max_iter=256: {info}")
    assert info["converged"]
    check_residual(matrix(name)[0], th, V, 1e-10, "planted(300, 128) k=8")
    check_iterations(name, matrix(name)[0], 8, 1e-10, info)


# ---- 6. breakdown ------------------------------------------------------------------------------------------------------------------------------

def _agrees_with_host(dev, host, x, k, what):
    """bit for bit after a fall-back, within the bounds of check 1 (plus the float32 rounding of the components) otherwise"""
    if dev["eig"]["used"] == "host":
        assert np.array_equal(dev["components"], host["components"]) and np.array_equal(dev["explained_variance"], host["explained_variance"])
        return
    N, D = x.shape
    C = centred_scatter(x)
    w, _ = eig_desc(C)
    gap = gaps(w)[:k]
    b = bound(D, 1e-10)
    a, c = dev["components"].astype(np.float64), host["components"].astype(np.float64)
    sin = np.array([np.linalg.norm(a[j] - (a[j] @ c[j]) * c[j]) for j in range(k)])
    print(f"{what}: sin angle {sin} (bound {b * w[0] / gap + 2.0 ** -23})")
    assert (sin <= b * w[0] / gap + 2.0 ** -23).all()
    assert (np.abs(dev["explained_variance"] - host["explained_variance"]) <= b * w[0] / (N - 1)).all()


def test_zero_matrix_breaks_down_and_ends():
    from dbmm_amd import analysis, ops
    D = 64
    xd = torch.zeros(1, D, device="cuda")
    S = ops.covariance(xd, torch.zeros(D, device="cuda"))
    vals, vecs, info = ops.sym_eig_topk(S, 2)
    print(f"zero matrix: {info}")
    assert info["state"] == "breakdown" and not info["converged"]
    assert torch.isfinite(vals).all() and torch.isfinite(vecs).all()
    x2 = torch.zeros(2, D, device="cuda")
    g = np.zeros(2, dtype=np.int64)
    host, dev = analysis.pca(x2, g, k=2), analysis.pca(x2, g, k=2, solver="device")
    print(f"pca of two zero rows: eig {dev['eig']}")
    assert dev["eig"]["used"] == "host" and dev["eig"]["state"] == "breakdown"
    assert np.array_equal(dev["components"], host["components"]) and np.array_equal(dev["explained_variance"], host["explained_variance"])
    assert np.isfinite(dev["components"]).all() and torch.isfinite(dev["coords"]).all()


def test_rank_below_the_block_ends():
    from dbmm_amd import analysis, ops
    x = planted(37, 64)[:5].copy()
    xd = torch.from_numpy(x).cuda()
    mean = x.astype(np.float64).mean(0)
    S = ops.covariance(xd, torch.from_numpy(mean.astype(np.float32)).cuda())
    vals, vecs, info = ops.sym_eig_topk(S, 2)
    print(f"five rows, D = 64 (rank 4 < 16): {info}")
    assert info["state"] in ("converged", "breakdown")
    assert torch.isfinite(vals).all() and torch.isfinite(vecs).all()
    g = np.arange(5) % 2
    host, dev = analysis.pca(xd, g, k=2), analysis.pca(xd, g, k=2, solver="device")
    print(f"pca of five rows: eig {dev['eig']}")
    assert np.isfinite(dev["components"]).all() and np.isfinite(dev["explained_variance"]).all() and torch.isfinite(dev["coords"]).all()
    _agrees_with_host(dev, host, x, 2, "five rows")


# ---- 7. analysis.pca(solver="device") end to end ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", [1, 2, 3])
@pytest.mark.parametrize("N,D", SHAPES)
def test_pca_device_solver_end_to_end(N, D, k):
    from dbmm_amd import analysis
    x, xd, mean = case(N, D)
    g = np.random.RandomState(1).randint(0, 4, N)
    host = analysis.pca(xd, g, k=k, solver="host")
    dev = analysis.pca(xd, g, k=k, solver="device")
    print(f"N={N} D={D} k={k}: eig {dev['eig']}")
    assert dev["eig"]["used"] == "device" and dev["eig"]["converged"]
    assert np.array_equal(dev["mean"], host["mean"])
    _agrees_with_host(dev, host, x, k, f"N={N} D={D} k={k}")
    assert dev["components"].dtype == np.float32 and dev["components"].shape == (k, D)
    top = np.abs(dev["components"]).argmax(1)
    assert (dev["components"][np.arange(k), top] > 0).all(), "sign rule"
    assert (np.diff(dev["explained_variance"]) <= 0).all()
    assert abs(dev["total_variance"] - host["total_variance"]) <= 1e-12 * host["total_variance"]
    check_projection(dev["coords"].cpu().numpy(), x, dev["mean"], dev["components"], f"coords N={N} D={D} k={k}")
    other, od, _ = case(53 if N == 37 else 37, D)                               # another split: other rows of the same width
    check_projection(analysis.pca_project(dev, od).cpu().numpy(), other, dev["mean"], dev["components"], f"another split N={N} D={D} k={k}")
    assert list(dev["centroids"]) == list(host["centroids"])


def test_projection_report_with_the_device_solver():
    from dbmm_amd import analysis, synth, trainer
    tables = []
    for split, n in (("train", 900), ("val", 500), ("test", 600)):
        x, y, c = synth.embedding_dataset(21, split, n, 512)
        tables.append(trainer.EmbeddingTable(x, y.numpy(), c.numpy()))
    opt = SimpleNamespace(batch_size=256)
    rep_h, fit_h = analysis.projection_report(opt, *tables, k=2)
    rep_d, fit_d = analysis.projection_report(opt, *tables, k=2, solver="device")
    print(f"projection_report: eig {fit_d['eig']}")
    assert "eig" not in fit_h
    if fit_d["eig"]["used"] == "host":
        for split in rep_h:
            assert np.array_equal(rep_d[split]["coords"], rep_h[split]["coords"])
        return
    xt = tables[0].embeddings.cpu().numpy()
    _agrees_with_host(fit_d, fit_h, xt, 2, "projection_report fit")
    for split, table in zip(rep_d, tables):
        check_projection(rep_d[split]["coords"], table.embeddings.cpu().numpy(), fit_d["mean"], fit_d["components"], f"projection_report {split}")


# ---- 8. the default is unchanged ------------------------------------------------------------------------------------------------------------------

def test_default_is_the_host_path_and_never_calls_the_solver(monkeypatch):
    from dbmm_amd import analysis, ops
    x, xd, _ = case(300, 128)
    g = np.arange(300) % 3
    calls = []
    real = ops.sym_eig_topk

    def counted(*a, **kw):
        calls.append(a)
        return real(*a, **kw)

    monkeypatch.setattr(ops, "sym_eig_topk", counted)
    default = analysis.pca(xd, g, 2)
    host = analysis.pca(xd, g, 2, solver="host")
    assert calls == [], "the default path called the device solver"
    assert "eig" not in default and "eig" not in host
    for key in ("mean", "components", "explained_variance", "explained_variance_ratio"):
        assert np.array_equal(default[key], host[key])
    assert default["total_variance"] == host["total_variance"] and torch.equal(default["coords"], host["coords"])
    dev = analysis.pca(xd, g, 2, solver="device")
    assert len(calls) == 1 and "eig" in dev


# ---- 9. guard zones --------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("N,D,k", [(100, 64, 2), (1025, 192, 8)])
def test_nothing_is_written_outside_the_workspace_and_the_start_block(N, D, k, monkeypatch):
    from dbmm_amd import ops
    name = ("eight", N, D)
    C, Cd = matrix(name)
    want_vals, want_vecs, want_info = ops.sym_eig_topk(Cd, k, tol=TOL)
    ga = GuardedAlloc()
    monkeypatch.setattr(ops, "_empty", ga)
    vals, vecs, info = ops.sym_eig_topk(Cd, k, tol=TOL)
    torch.cuda.synchronize()
    assert len(ga.bufs) == 2                                                   # the workspace (the outputs are views of it) and the start block
    ga.check()
    assert torch.equal(Cd, torch.from_numpy(C).cuda()), "the input matrix was written"
    print(f"guarded N={N} D={D} k={k}: {info}")
    assert torch.equal(vals, want_vals) and torch.equal(vecs, want_vecs) and info == want_info
