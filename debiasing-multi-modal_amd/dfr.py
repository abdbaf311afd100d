"""Deep feature reweighting (Kirichenko, Izmailov, Wilson 2023: "Last layer re-training is sufficient for robustness to spurious
correlations"): L1-penalised logistic probes on small group-balanced subsets of the validation split.  The reference has no
counterpart (it leaves `--lr_linear_probing` commented out with "tuning needed"); DFR needs no learning rate.

One fit ("replica") minimises, over rows idx[0..n) of a shared fp32 table [N, D] with int64 labels and C classes,

    F(W, b) = (1 / n) sum_i CE(softmax(W x_i + b), y_i) + lam ||W||_1          (the intercept is not penalised)

which is sklearn's LogisticRegression(penalty="l1", C=C_sk) at lam = 1 / (C_sk n).  The solver is FISTA with the constant step
eta = 1 / L, L = (1 / 2) lambda_max((1 / n) [X, 1]^T [X, 1]) (Boehning's bound on the softmax Hessian); one iteration from the iterate
(W, b), the extrapolated point (V, c) and the scalar t:

    G, g = gradient of the CE mean at (V, c)
    W'   = soft(V - eta G, eta lam)        soft(z, tau) = sign(z) max(|z| - tau, 0): exact zeros
    b'   = c - eta g
    t'   = (1 + sqrt(1 + 4 t^2)) / 2       in float64;   beta = fp32((t - 1) / t')     (accelerate=False: beta = 0, plain ISTA)
    V'   = W' + beta (W' - W),  c' = b' + beta (b' - b)

from t = 1, V = W, zero weights.  `prox_fit_reference` is that iteration in torch (float64 by default, any device, replica by
replica): the oracle of the kernel's tests and the solver="reference" path, which runs without a GPU.  The device path is
ops.linear_prox_fit (csrc/linear_prox.hip): one workgroup per fit, the iterate in LDS, many iterations per launch.
`fit_l1_probes` computes the steps and runs launch groups until every fit has converged; trainer.train_dfr is DFR-Val as one call.
"""
import math
import time
from collections import namedtuple

import numpy as np
import torch

from . import ops

DEFAULT_C_GRID = (1.0, 0.7, 0.3, 0.1, 0.07, 0.03, 0.01)
TINY = 1e-30

# Row visits (rows x iterations) of one workgroup per launch.  Measured on an MI355X at D = 1024: one row
# visit costs a workgroup 0.14 us at C = 2 (DFR's shape), 0.22 us at C = 4 and 0.65 us at C = 8, whatever the number of workgroups.
# 2^15 of them are 4.6 ms a launch at C = 2 and 21 ms at C = 8: a launch stays short next to anything else the device is asked to
# do, the host looks at convergence every few milliseconds, and DFR's own subsets (200 - 1000 rows) keep check_every = 32.
MAX_ROW_VISITS = 1 << 15

ProxFit = namedtuple("ProxFit", "weights intercepts iterations nnz converged steps setup_seconds solver")


def soft(z, tau):
    """sign(z) max(|z| - tau, 0); exact zeros inside the threshold"""
    return torch.sign(z) * torch.clamp(z.abs() - tau, min=0)


def beta_sequence(k, t=1.0):
    """(betas fp32-rounded as Python floats, t after k iterations) of the FISTA recurrence from t, in float64"""
    out = []
    for _ in range(k):
        t1 = (1.0 + math.sqrt(1.0 + 4.0 * t * t)) / 2.0
        out.append(float(np.float32((t - 1.0) / t1)))
        t = t1
    return out, t


def _clamped(idx, n_rows):
    return idx.clamp(0, n_rows - 1)


def _as_idx(idx, device):
    idx = torch.as_tensor(np.asarray(idx) if not torch.is_tensor(idx) else idx, dtype=torch.int64)
    if idx.dim() == 1:
        idx = idx.unsqueeze(0)
    if idx.dim() != 2 or idx.shape[1] < 1 or idx.shape[0] < 1:
        raise ValueError(f"index lists [R, n] with n >= 1 expected, got {tuple(idx.shape)}")
    return idx.to(device).contiguous()


def _as_vec(v, R, device, dtype, what):
    v = torch.as_tensor(v, dtype=dtype).reshape(-1).to(device)
    if v.numel() == 1 and R > 1:
        v = v.expand(R)
    if v.numel() != R:
        raise ValueError(f"{what}: {v.numel()} values for {R} fits")
    return v.contiguous()


def ce_mean_and_grad(X, y, V, c, want_grad=True):
    """(CE mean, dV [C, D], dc [C]) of the rows X [n, D] with labels y at (V, c), in X's dtype"""
    logits = X @ V.t() + c
    lse = torch.logsumexp(logits, dim=1)
    ce = (lse - logits.gather(1, y.unsqueeze(1)).squeeze(1)).mean()
    if not want_grad:
        return ce, None, None
    p = torch.softmax(logits, dim=1)
    p.scatter_add_(1, y.unsqueeze(1), -torch.ones_like(p[:, :1]))
    n = X.shape[0]
    return ce, p.t() @ X / n, p.sum(0) / n


def objective(table, idx, labels, W, b, lam):
    """F(W, b) of every fit in float64: float64 [R] on the host.  idx [R, n]; W [R, C, D]; b [R, C]; lam [R]"""
    idx = _as_idx(idx, table.device)
    R = idx.shape[0]
    lam = _as_vec(lam, R, "cpu", torch.float64, "lam")
    out = torch.zeros(R, dtype=torch.float64)
    for r in range(R):
        rows = _clamped(idx[r], table.shape[0])
        X, y = table[rows].double(), labels[rows]
        Wr, br = W[r].to(table.device).double(), b[r].to(table.device).double()
        out[r] = ce_mean_and_grad(X, y, Wr, br, want_grad=False)[0].item() + lam[r].item() * Wr.abs().sum().item()
    return out


def reference_state(R, C, D, device="cpu", dtype=torch.float64):
    """the start of R fits for prox_fit_reference: zero weights, V = W, t = 1 (an ops.ProxState of `dtype` tensors, t float64)"""
    z = lambda *s: torch.zeros(s, dtype=dtype, device=device)
    return ops.ProxState(z(R, C, D), z(R, C), z(R, C, D), z(R, C), torch.ones(R, dtype=torch.float64, device=device))


def prox_fit_reference(table, idx, labels, lam, step, state=None, iters=1, accelerate=True, dtype=torch.float64, n_classes=2):
    """`iters` iterations of the module docstring's iteration for every fit, replica by replica, in `dtype` on the table's device:
    the oracle of ops.linear_prox_fit and the solver="reference" path.  Rows are clamped into the table as the kernel clamps them;
    beta is rounded to fp32 as the kernel rounds it; t advances in float64.  `state` (reference_state starts one) is left alone: the
    new state is returned.  Returns (state, stats): stats a dict of float64 [R] host tensors `delta` (max |W' - W|), `wmax`, `nnz`,
    `ce` (CE mean at the last extrapolated point) of the last iteration, and `z` [R, C, D]: that iteration's V - eta G, the value
    the threshold is applied to."""
    dev = table.device
    idx = _as_idx(idx, dev)
    R = idx.shape[0]
    D = table.shape[1]
    if state is None:
        state = reference_state(R, n_classes, D, dev, dtype)
    lam = _as_vec(lam, R, dev, torch.float64, "lam").to(dtype)
    step = _as_vec(step, R, dev, torch.float64, "step").to(dtype)
    W, b, V, c = (s.to(dev, dtype).clone() for s in state[:4])
    t = state.t.to("cpu", torch.float64).clone()
    stats = {k: torch.zeros(R, dtype=torch.float64) for k in ("delta", "wmax", "nnz", "ce")}
    stats["z"] = torch.zeros(W.shape, dtype=torch.float64)
    for r in range(R):
        rows = _clamped(idx[r], table.shape[0])
        X, y = table[rows].to(dtype), labels[rows]
        eta, thr = step[r], step[r] * lam[r]
        betas, t_end = beta_sequence(iters, float(t[r]))
        Wr, br, Vr, cr = W[r], b[r], V[r], c[r]
        for k in range(iters):
            ce, G, g = ce_mean_and_grad(X, y, Vr, cr)
            z = Vr - eta * G
            Wn = soft(z, thr)
            bn = cr - eta * g
            beta = betas[k] if accelerate else 0.0
            Vr, cr = Wn + beta * (Wn - Wr), bn + beta * (bn - br)
            if k == iters - 1:
                stats["delta"][r] = (Wn - Wr).abs().max().item()
                stats["wmax"][r] = Wn.abs().max().item()
                stats["nnz"][r] = int((Wn != 0).sum())
                stats["ce"][r] = ce.item()
                stats["z"][r] = z.double().cpu()
            Wr, br = Wn, bn
        W[r], b[r], V[r], c[r] = Wr, br, Vr, cr
        t[r] = t_end
    return ops.ProxState(W, b, V, c, t.to(dev)), stats


def prox_steps(table, idx):
    """eta = 1 / L per fit, L = (1 / 2) lambda_max((1 / n) [X, 1]^T [X, 1]) over the fit's (clamped) rows: float64 [R] on the host.
    The Gram matrix of the smaller side ([X, 1] [X, 1]^T when n <= D: the same nonzero eigenvalues) is formed in float64 on the
    table's device; its largest eigenvalue is a host eigvalsh."""
    idx = _as_idx(idx, table.device)
    out = torch.zeros(idx.shape[0], dtype=torch.float64)
    for r in range(idx.shape[0]):
        X = table[_clamped(idx[r], table.shape[0])].double()
        A = torch.cat([X, torch.ones_like(X[:, :1])], dim=1)
        n = A.shape[0]
        M = (A @ A.t() if n <= A.shape[1] else A.t() @ A) / n
        out[r] = 2.0 / float(np.linalg.eigvalsh(M.cpu().numpy())[-1])
    return out


def launch_iters(n, check_every, left):
    """iterations of the next launch: at most `check_every`, at most what is left, and few enough that rows x iterations stays
    under MAX_ROW_VISITS (at least one)"""
    return max(1, min(int(check_every), int(left), MAX_ROW_VISITS // max(1, int(n))))


def fit_l1_probes(table, idx, labels, lam, solver="device", tol=1e-4, max_iter=1000, check_every=32, n_classes=2, accelerate=True,
                  steps=None):
    """R L1-penalised logistic probes on rows idx [R, n] of `table` ([N, D] fp32, labels int64 [N]) at penalties lam [R]
    (lam = 1 / (C_sk n) for sklearn's C_sk).  solver="device": ops.linear_prox_fit, launch groups of `launch_iters` iterations, up
    to 256 fits a launch; solver="reference": prox_fit_reference in float64 at the same cadence.  A group of fits stops when every one
    has max |W' - W| <= tol max(max |W'|, tiny) (tol: sklearn's coefficient-change default) or at max_iter; fits that have converged
    keep iterating with their group.  Returns a ProxFit: weights [R, C, D], intercepts [R, C] (float32 from the device, float64
    from the reference), iterations / nnz int64 [R], converged bool [R] (host tensors), the steps [R] and the seconds their set-up
    took."""
    if solver not in ("device", "reference"):
        raise ValueError(f"fit_l1_probes: solver 'device' or 'reference' expected, got {solver!r}")
    if not (1 <= n_classes <= 8):
        raise ValueError(f"fit_l1_probes: 1..8 classes are served, got {n_classes}")
    if max_iter < 1 or check_every < 1 or not tol > 0:
        raise ValueError(f"fit_l1_probes: max_iter >= 1, check_every >= 1 and tol > 0 expected, got {max_iter}, {check_every}, {tol}")
    dev = table.device
    idx = _as_idx(idx, dev)
    R, n = idx.shape
    D = table.shape[1]
    lam64 = _as_vec(lam, R, "cpu", torch.float64, "lam")
    if not bool((lam64 >= 0).all()) or not bool(torch.isfinite(lam64).all()):
        raise ValueError("fit_l1_probes: finite penalties lam >= 0 expected")
    seen = labels[_clamped(idx, table.shape[0])]
    if int(seen.min()) < 0 or int(seen.max()) >= n_classes:
        raise ValueError(f"fit_l1_probes: a label outside [0, {n_classes}) among the indexed rows")
    t0 = time.perf_counter()
    steps = prox_steps(table, idx) if steps is None else _as_vec(steps, R, "cpu", torch.float64, "steps")
    setup = time.perf_counter() - t0
    Ws, bs = [], []
    its = torch.zeros(R, dtype=torch.int64)
    nnz = torch.zeros(R, dtype=torch.int64)
    conv = torch.zeros(R, dtype=torch.bool)
    for r0 in range(0, R, ops.PROX_MAX_R):
        sl = slice(r0, min(R, r0 + ops.PROX_MAX_R))
        Rg = sl.stop - sl.start
        gidx = idx[sl].contiguous()
        if solver == "device":
            state = ops.linear_prox_state(Rg, n_classes, D, dev)
            glam, gstep = lam64[sl].float().to(dev), steps[sl].float().to(dev)
        else:
            state = reference_state(Rg, n_classes, D, dev)
            glam, gstep = lam64[sl], steps[sl]
        done = 0
        while done < max_iter:
            k = launch_iters(n, check_every, max_iter - done)
            if solver == "device":
                st = ops.linear_prox_fit(table, gidx, labels, glam, gstep, state, k, accelerate=accelerate).double().cpu()
                delta, wmax, nz = st[:, 0], st[:, 1], st[:, 2]
            else:
                state, st = prox_fit_reference(table, gidx, labels, glam, gstep, state, k, accelerate=accelerate)
                delta, wmax, nz = st["delta"], st["wmax"], st["nnz"]
            done += k
            ok = delta <= tol * wmax.clamp_min(TINY)
            if bool(ok.all()):
                break
        its[sl], nnz[sl], conv[sl] = done, nz.round().long(), ok
        Ws.append(state.w)
        bs.append(state.b)
    return ProxFit(torch.cat(Ws), torch.cat(bs), its, nnz, conv, steps, setup, solver)


# ---- the pieces of DFR-Val (trainer.train_dfr) that need neither a model nor a launch ----

def column_moments(x, chunk=1 << 16):
    """(mean, std) float64 [D] of the rows x, from float64 sums (two passes: the mean, then the centred squares); the population
    standard deviation, as sklearn's StandardScaler; a constant column's 0 becomes 1"""
    n = x.shape[0]
    s = torch.zeros(x.shape[1], dtype=torch.float64, device=x.device)
    for i in range(0, n, chunk):
        s += x[i:i + chunk].double().sum(0)
    mean = s / n
    q = torch.zeros_like(s)
    for i in range(0, n, chunk):
        q += ((x[i:i + chunk].double() - mean) ** 2).sum(0)
    std = (q / n).sqrt()
    return mean, torch.where(std == 0, torch.ones_like(std), std)


def standardised(x, mean, std, chunk=1 << 16):
    """(x - mean) / std in float64, rounded to a new float32 tensor"""
    out = torch.empty_like(x)
    for i in range(0, x.shape[0], chunk):
        out[i:i + chunk] = ((x[i:i + chunk].double() - mean) / std).float()
    return out


def fold_standardisation(W, b, mean, std):
    """(W / std, b - sum W mean / std) in float64: the probe on raw rows that equals (W, b) on standardised rows"""
    W, b = W.double(), b.double()
    Wf = W / std
    return Wf, b - (Wf * mean).sum(1)


def val_halves(n, seed):
    """two disjoint sorted halves of range(n) (the first takes the odd row) from a private np.random.RandomState(seed)"""
    perm = np.random.RandomState(seed).permutation(n)
    h = (n + 1) // 2
    return np.sort(perm[:h]).astype(np.int64), np.sort(perm[h:]).astype(np.int64)


def balanced_subsets(groups, rows, seeds):
    """[len(seeds), m] int64: for every seed the rows of `rows` (indices into `groups`) that analysis.balanced_rows draws over their
    groups -- min-count rows of every group, without replacement, from a private stream"""
    from . import analysis                     # analysis imports trainer, which imports this module
    rows = np.asarray(rows, dtype=np.int64)
    g = np.asarray(groups)[rows]
    return np.stack([rows[analysis.balanced_rows(g, seed=int(s))] for s in seeds])


def pick_c(c_grid, scores):
    """index of the best mean score; ties go to the smaller C"""
    best = None
    for i, (c, s) in enumerate(zip(c_grid, scores)):
        if best is None or s > scores[best] or (s == scores[best] and c < c_grid[best]):
            best = i
    return best


def check_options(c_grid, n_cls, labels, groups, n_groups, halves):
    """train_dfr's refusals (ValueError), before a model or a launch"""
    if len(c_grid) == 0:
        raise ValueError("train_dfr: opt.dfr_c_grid is empty")
    if any(not np.isfinite(c) or c <= 0 for c in c_grid):
        raise ValueError(f"train_dfr: every C of opt.dfr_c_grid must be a finite positive number, got {list(c_grid)}")
    if not (1 <= n_cls <= 8):
        raise ValueError(f"train_dfr: the probe kernels serve at most 8 classes, got n_cls={n_cls}")
    labels = np.asarray(labels)
    if labels.size == 0 or labels.min() < 0 or labels.max() >= n_cls:
        raise ValueError(f"train_dfr: a validation label outside [0, {n_cls})")
    groups = np.asarray(groups)
    for what, rows in (("the validation split", np.arange(len(groups))), ("the tuning half", halves[0]), ("the held-out half", halves[1])):
        missing = sorted(set(range(n_groups)) - set(groups[rows].tolist()))
        if missing:
            raise ValueError(f"train_dfr: group(s) {missing} absent from {what}: a group-balanced subset cannot be drawn / scored")
