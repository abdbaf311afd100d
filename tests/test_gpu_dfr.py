"""The fused L1 proximal probe kernel (csrc/linear_prox.hip, ops.linear_prox_fit) and DFR on it, on the MI355X.

(a) The kernel against dfr.prox_fit_reference in float64 on the cases of tests/dfr_cases.py, iterations 1, 2 and 8, accelerated and
    plain.  Bound, the project's rule (test_gpu_adapter_generic.py): err <= 4 * e32 + 2^-23 * max|ref| per tensor, err = max|kernel -
    ref64|, e32 = max|ref32 - ref64| for the same iterations in torch float32; both references read the float32 lam / step the kernel
    reads.  Values are compared everywhere (the prox is 1-Lipschitz); the zero pattern is asserted exactly where the float64
    pre-threshold magnitude is outside eta lam (1 +- 1e-3) -- at most 5 % of a case's entries are inside, which
    tests/test_dfr_host.py checks on the CPU.  The launch's figures: nnz is the kernel's own count of nonzeros exactly; max |W|
    and max |dW| are 1- and 2-Lipschitz in W and take W's bound (twice it); the CE mean is ONE number, whose own e32 is one sample
    of a rounding error, so it also gets the fp32 chain's (n + 16) * 2^-24 relative (n / waves adds a wave, the waves in order).
(b) Bits: the same call twice; a replica alone against itself among five, in any position; 8 iterations in one launch against 3 + 5
    and 8 x 1; the state through a copy.
(c) Guard zones around the state and the figures through the C entry; the wrapper's refusals leave the state alone.  The entry has
    no workspace, so there is none to size.
(d) fit_l1_probes and train_dfr, solver="device" against solver="reference".

Measured on an MI355X: (a) the largest err / allowed over the issue's five shapes is 0.58 (an intercept), the
typical one 0.1 - 0.3, and no case leaves more than 0.2 % of its entries out of the zero pattern; (d) the objectives of the seven fits
differ by at most 1.6e-11 relative from the reference's with the same iteration counts and nnz, the averaged weights of train_dfr by
3.1e-07 after 64 iterations where 7.0e-05 is allowed, and the full grid's tuning table equals the reference's in every entry.
"""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import dfr_cases as K
from dbmm_amd import _lib, dfr, ops, trainer

gpu = pytest.mark.gpu
FLOOR = 2.0 ** -23


def _cuda(*ts):
    return [t.cuda() for t in ts]


def _launch(shape, chunks, accelerate, reps=None):
    """the kernel on case `shape` from the zero start, one launch per entry of `chunks`; `reps`: these replicas only, in this order"""
    n, D, C, R = shape
    table, labels, idx, lam, step = K.operands(*shape)
    if reps is not None:
        sel = torch.tensor(reps)
        idx, lam, step = idx[sel].contiguous(), lam[sel].contiguous(), step[sel].contiguous()
    table, labels, idx, lam, step = _cuda(table, labels, idx, lam, step)
    state = ops.linear_prox_state(idx.shape[0], C, D, "cuda")
    for k in chunks:
        stats = ops.linear_prox_fit(table, idx, labels, lam, step, state, k, accelerate=accelerate)
    torch.cuda.synchronize()
    return state, stats


def _same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


# ---- (a) ----------------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("accelerate", (True, False), ids=("fista", "ista"))
@pytest.mark.parametrize("iters", K.ITERS)
@pytest.mark.parametrize("shape", K.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_kernel_against_float64(shape, iters, accelerate):
    n, D, C, R = shape
    s64, st64, s32, st32 = K.references(*shape, iters, accelerate)
    state, stats = _launch(shape, (iters,), accelerate)
    stats = stats.double().cpu()
    worst = {}
    for name in ("w", "b", "v", "c"):
        k, r64, r32 = getattr(state, name).double().cpu(), getattr(s64, name), getattr(s32, name).double()
        err, e32, top = (k - r64).abs().max().item(), (r32 - r64).abs().max().item(), r64.abs().max().item()
        allowed = 4 * e32 + FLOOR * top
        worst[name] = allowed
        print(f"  {name}: err {err:.3e} e32 {e32:.3e} max|ref| {top:.3e} allowed {allowed:.3e} ratio {err / allowed if allowed else 0.0:.3f}")
        assert err <= allowed, name
    assert torch.equal(state.t.cpu(), s64.t.cpu())
    for j, (name, lip) in enumerate((("delta", 2.0), ("wmax", 1.0))):
        err = (stats[:, j] - st64[name]).abs().max().item()
        print(f"  {name}: err {err:.3e} allowed {lip * worst['w']:.3e}")
        assert err <= lip * worst["w"], name
    ce_err, ce_e32 = (stats[:, 3] - st64["ce"]).abs().max().item(), (st32["ce"] - st64["ce"]).abs().max().item()
    ce_allowed = max(4 * ce_e32 + FLOOR * st64["ce"].max().item(), (n + 16) * 2.0 ** -24 * st64["ce"].max().item())
    print(f"  ce: err {ce_err:.3e} e32 {ce_e32:.3e} allowed {ce_allowed:.3e}")
    assert ce_err <= ce_allowed
    kw = state.w.cpu()
    assert torch.equal(stats[:, 2].long(), (kw != 0).sum((1, 2)))
    mask = K.band_mask(*shape, iters, accelerate)
    left_out = 1.0 - mask.double().mean().item()
    print(f"  zero pattern: {left_out:.4f} of the entries inside the band, {int((kw == 0).sum())} zeros of {kw.numel()}")
    assert left_out <= K.BAND_CAP
    assert torch.equal((kw == 0)[mask], (s64.w == 0)[mask])
    assert not bool(torch.signbit(kw[kw == 0]).any())                    # the exact zero is +0


# ---- (b) ----------------------------------------------------------------------------------------------------------------------------
BITS_SHAPE = K.SHAPES[2]                                                   # (300, 1024, 2, 5)


@gpu
def test_same_call_same_bits():
    for shape in (BITS_SHAPE, K.SHAPES[3]):
        a, sa = _launch(shape, (8,), True)
        b, sb = _launch(shape, (8,), True)
        assert _same(a, b) and torch.equal(sa, sb)


@gpu
def test_replica_bits_do_not_depend_on_the_grid():
    full, sfull = _launch(BITS_SHAPE, (8,), True)
    for r in range(5):
        alone, salone = _launch(BITS_SHAPE, (8,), True, reps=[r])
        assert all(torch.equal(x[0], y[r]) for x, y in zip(alone, full)) and torch.equal(salone[0], sfull[r])
    order = [3, 0, 4, 2, 1]
    perm, sperm = _launch(BITS_SHAPE, (8,), True, reps=order)
    for j, r in enumerate(order):
        assert all(torch.equal(x[j], y[r]) for x, y in zip(perm, full)) and torch.equal(sperm[j], sfull[r])


@gpu
@pytest.mark.parametrize("accelerate", (True, False), ids=("fista", "ista"))
def test_split_launches_are_one_launch(accelerate):
    one, s1 = _launch(BITS_SHAPE, (8,), accelerate)
    for chunks in ((3, 5), (1,) * 8):
        many, sm = _launch(BITS_SHAPE, chunks, accelerate)
        assert _same(one, many) and torch.equal(s1, sm), chunks


@gpu
def test_state_round_trips_through_a_copy():
    n, D, C, R = shape = K.SHAPES[1]
    table, labels, idx, lam, step = _cuda(*K.operands(*shape))
    a = ops.linear_prox_state(R, C, D, "cuda")
    ops.linear_prox_fit(table, idx, labels, lam, step, a, 3)
    b = ops.ProxState(*(t.cpu().clone().cuda() for t in a))               # through the host and back
    sa = ops.linear_prox_fit(table, idx, labels, lam, step, a, 5)
    sb = ops.linear_prox_fit(table, idx, labels, lam, step, b, 5)
    one, s1 = _launch(shape, (8,), True)
    assert _same(a, b) and _same(a, one) and torch.equal(sa, sb) and torch.equal(sa, s1)
    warm = ops.linear_prox_state(R, C, D, "cuda", w=a.w, b=a.b)
    assert torch.equal(warm.v, a.w) and torch.equal(warm.c, a.b) and bool((warm.t == 1).all())


# ---- (c) ----------------------------------------------------------------------------------------------------------------------------
class _Zone:
    """n 4-byte words between two guard zones of PAD sentinel words"""
    PAD, S = 4096, 0x7FA5A5A5

    def __init__(self, n, dtype=torch.float32, fill=0.0):
        words = n * (2 if dtype == torch.float64 else 1)
        self.words = words
        self.raw = torch.full((words + 2 * self.PAD,), self.S, dtype=torch.int32, device="cuda")
        self.t = self.raw[self.PAD:self.PAD + words].view(dtype)
        self.t.fill_(fill)
        self.ptr = self.t.data_ptr()

    def intact(self):
        return bool((self.raw[:self.PAD] == self.S).all()) and bool((self.raw[self.PAD + self.words:] == self.S).all())


@gpu
@pytest.mark.parametrize("shape", (K.SHAPES[1], K.SHAPES[3], K.SHAPES[4]), ids=lambda s: "x".join(map(str, s)))
def test_entry_stays_inside_state_and_figures(shape):
    n, D, C, R = shape
    table, labels, idx, lam, step = _cuda(*K.operands(*shape))
    w, b, v, c = _Zone(R * C * D), _Zone(R * C), _Zone(R * C * D), _Zone(R * C)
    t, stats = _Zone(R, torch.float64, 1.0), _Zone(R * 4, fill=float("nan"))
    rc = _lib.lib().dbmm_linear_prox_fit(table.data_ptr(), table.shape[0], idx.data_ptr(), labels.data_ptr(), lam.data_ptr(), step.data_ptr(),
                                         w.ptr, b.ptr, v.ptr, c.ptr, t.ptr, stats.ptr, R, n, D, C, 8, 1, _lib.stream())
    torch.cuda.synchronize()
    assert rc == 0
    assert all(z.intact() for z in (w, b, v, c, t, stats))
    state, st = _launch(shape, (8,), True)
    got = (w.t.view(R, C, D), b.t.view(R, C), v.t.view(R, C, D), c.t.view(R, C), t.t)
    assert _same(got, state) and torch.equal(stats.t.view(R, 4), st) and not bool(torch.isnan(stats.t).any())


@gpu
def test_refused_arguments_launch_nothing():
    n, D, C, R = shape = K.SHAPES[1]
    table, labels, idx, lam, step = _cuda(*K.operands(*shape))
    state = ops.linear_prox_state(R, C, D, "cuda")
    ops.linear_prox_fit(table, idx, labels, lam, step, state, 2)
    before = [t.clone() for t in state]
    bad = [
        dict(iters=0), dict(iters=-1), dict(iters=(1 << 20) + 1),
        dict(idx=idx[:2].contiguous()), dict(idx=idx.int()), dict(idx=idx.t()), dict(idx=idx[:, :0]), dict(idx=idx.cpu()),
        dict(labels=labels.int()), dict(labels=labels[:-1].contiguous()),
        dict(lam=lam.double()), dict(lam=lam[:2].contiguous()), dict(step=step[:1].contiguous()),
        dict(table=table[:, :D - 4]), dict(table=table.double()), dict(table=table[:, :D - 4].contiguous()),
        dict(state=state._replace(t=state.t.float())), dict(state=state._replace(v=state.v[:, :, :D - 4].contiguous())),
        dict(state=state._replace(c=state.c[:2].contiguous())), dict(state=state._replace(b=state.b.cpu())),
    ]
    for k in bad:
        a = dict(table=table, idx=idx, labels=labels, lam=lam, step=step, state=state, iters=1)
        a.update(k)
        with pytest.raises((_lib.DbmmError, RuntimeError)):
            ops.linear_prox_fit(a["table"], a["idx"], a["labels"], a["lam"], a["step"], a["state"], a["iters"])
    big = ops.linear_prox_state(257, 2, 8, "cuda")
    with pytest.raises(_lib.DbmmError):
        ops.linear_prox_fit(torch.zeros(4, 8, device="cuda"), torch.zeros(257, 4, dtype=torch.int64, device="cuda"),
                            torch.zeros(4, dtype=torch.int64, device="cuda"), torch.zeros(257, device="cuda"), torch.ones(257, device="cuda"), big, 1)
    nine = ops.ProxState(*(torch.zeros(s, device="cuda") for s in ((1, 9, 8), (1, 9), (1, 9, 8), (1, 9))), torch.ones(1, dtype=torch.float64, device="cuda"))
    with pytest.raises(_lib.DbmmError):
        ops.linear_prox_fit(torch.zeros(4, 8, device="cuda"), torch.zeros(1, 4, dtype=torch.int64, device="cuda"),
                            torch.zeros(4, dtype=torch.int64, device="cuda"), torch.zeros(1, device="cuda"), torch.ones(1, device="cuda"), nine, 1)
    # the C entry itself, with device pointers: a misaligned w, a bad R and iters = 0 come back before any launch
    L, s = _lib.lib(), state
    call = lambda wp, R_, it: L.dbmm_linear_prox_fit(table.data_ptr(), table.shape[0], idx.data_ptr(), labels.data_ptr(), lam.data_ptr(),
                                                     step.data_ptr(), wp, s.b.data_ptr(), s.v.data_ptr(), s.c.data_ptr(), s.t.data_ptr(),
                                                     torch.empty(R * 4, device="cuda").data_ptr(), R_, n, D, C, it, 1, _lib.stream())
    assert call(s.w.data_ptr() + 4, R, 1) == -2 and call(s.w.data_ptr(), 0, 1) == -1 and call(s.w.data_ptr(), R, 0) == -1
    torch.cuda.synchronize()
    assert _same(before, state)


# ---- (d) ----------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def split():
    yield K.make_split("cuda")                       # released with the module: nothing stays allocated for the files that follow


def _standardised_val(split):
    tr, va, _ = split
    mean, std = dfr.column_moments(tr.embeddings)
    return dfr.standardised(va.embeddings, mean, std)


@gpu
def test_fit_l1_probes_device_against_reference(split):
    """188 rows (a balanced subset of the synthetic val split), D = 64, C = 2, the seven penalties of the default grid"""
    va = split[1]
    zv = _standardised_val(split)
    rows = dfr.balanced_subsets(va.group_array, np.arange(len(va)), [1])
    assert rows.shape == (1, 188)
    idx = np.repeat(rows, 7, axis=0)
    lam = [1.0 / (c * 188) for c in dfr.DEFAULT_C_GRID]
    dev = dfr.fit_l1_probes(zv, idx, va.targets, lam, solver="device")
    ref = dfr.fit_l1_probes(zv, idx, va.targets, lam, solver="reference")
    assert bool(dev.converged.all()) and bool(ref.converged.all())
    assert dev.weights.dtype == torch.float32 and dev.weights.is_cuda
    fd = dfr.objective(zv, idx, va.targets, dev.weights, dev.intercepts, lam)
    fr = dfr.objective(zv, idx, va.targets, ref.weights, ref.intercepts, lam)
    rel = ((fd - fr).abs() / fr.abs())
    print(f"  iterations device {dev.iterations.tolist()} reference {ref.iterations.tolist()}; nnz {dev.nnz.tolist()} / {ref.nnz.tolist()}")
    print(f"  objective relative difference {[f'{v:.2e}' for v in rel.tolist()]}")
    assert bool((rel <= 1e-5).all())


@gpu
def test_train_dfr_one_c_against_the_reference(split):
    """a one-value grid: the device run and the reference pick the same subsets, and the averaged weights are within the kernel bound
    (4 e32 + 2^-23 max|ref|, e32 from the same iterations in torch float32) times the number of iterations run"""
    tr, va, te = split
    logs = {}
    for solver in ("device", "reference"):
        logs[solver] = []
        opt = SimpleNamespace(dfr_solver=solver, n_cls=2, dfr_c_grid=[0.3], dfr_retrains=4, batch_size=128)
        clf, scores, record = trainer.train_dfr(opt, tr, va, te, log=logs[solver])
        assert record["C"] == 0.3 and all(record["converged"])
    d, r = logs["device"], logs["reference"]
    assert (d[0]["subsets"] == r[0]["subsets"]).all() and (d[1]["subsets"] == r[1]["subsets"]).all()
    assert (d[2]["counts"][:, 0].sum() == len(tr)) and d[4]["group_acc"]["worst_acc"] > 0.4
    k = int(d[1]["iterations"][0])
    zv = _standardised_val(split)
    sub = d[1]["subsets"]
    lam = torch.full((4,), 1.0 / (0.3 * sub.shape[1]), dtype=torch.float32)
    step = dfr.prox_steps(zv, sub).float()
    w64 = dfr.prox_fit_reference(zv, sub, va.targets, lam.double(), step.double(), None, k)[0].w.mean(0).cpu()
    w32 = dfr.prox_fit_reference(zv, sub, va.targets, lam.double(), step.double(), None, k, dtype=torch.float32)[0].w.double().mean(0).cpu()
    got = d[1]["weights"].double().mean(0)
    dist, e32, top = (got - w64).abs().max().item(), (w32 - w64).abs().max().item(), w64.abs().max().item()
    allowed = k * (4 * e32 + FLOOR * top)
    print(f"  {k} iterations: averaged weights differ by {dist:.3e} (e32 {e32:.3e}, max|ref| {top:.3e}); allowed {allowed:.3e}")
    assert dist <= allowed


@gpu
def test_train_dfr_full_grid_picks_the_references_c(split):
    """dfr_seed = TUNE_SEED: the reference's best and second-best C are more than two rows of the smallest held-out group apart
    (tests/test_dfr_host.py checks that on the CPU: 0.0888 against 0.08), so the kernel's rounding cannot move the choice"""
    tr, va, te = split
    log = []
    clf, scores, record = trainer.train_dfr(SimpleNamespace(dfr_seed=K.TUNE_SEED, n_cls=2, batch_size=128), tr, va, te, log=log)
    ref = trainer.train_dfr(SimpleNamespace(dfr_seed=K.TUNE_SEED, n_cls=2, dfr_solver="reference", dfr_retrains=1), *K.dfr_split())[2]
    print(f"  device C {record['C']} tuning {[round(t['mean'], 4) for t in record['tuning']]}")
    print(f"  reference C {ref['C']} tuning {[round(t['mean'], 4) for t in ref['tuning']]}")
    assert record["C"] == ref["C"] == 0.1
    assert record["solver"] == "device" and all(record["converged"]) and all(record["tune_converged"])
    assert scores[2][2]["worst_acc"] > 0.45
