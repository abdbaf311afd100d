"""The adapter step OFF its fast shape (csrc/adapter_ops.hip: dbmm_gemm_bias_act -> bn1d_stats -> bn1d_relu -> dbmm_gemm_bias_act
forward; two K-major weight-gradient GEMMs over the batch, colsum, bn1d_bwd_reduce, bn1d_bwd_apply backward; the one-call steps
through the stand-alone heads and sgd_impl) against float64, and at the fast shape both implementations against the same float64.

Reference: a torch restatement on the CPU of Linear -> BatchNorm1d -> ReLU -> Linear and of the step (adapter_ref, eval_ref and
step_ref below; the heads are those of test_gpu_row_weights.py, test_gpu_group_dro.py and test_gpu_supcon.py), evaluated in
float64 and -- the same statements -- in float32.  Bound, the project's rule (test_gpu_head_shapes.py): err <= 4 * e32 + 2^-23,
err = max|kernel - ref64| / max|ref64| and e32 = max|ref32 - ref64| / max|ref64|, per tensor.  layers.0.bias' gradient is
analytically zero (a bias in front of train-mode BatchNorm) and is bounded absolutely, 1e-5, as test_gpu_adapter.py has it.

ReLU ties: an entry whose pre-ReLU value lies within 1e-5 of zero in the float64 run may take the other branch in float32.  Such
entries of r and dh, the rows of dx that hold one, and the tied unit's row / element of the layer-0 and BatchNorm gradients are
left out (of err and of e32 alike), and at most 5 % of a case's hidden units may be tied: asserted in every case, and for all
cases at once on the CPU by test_float64_references_stay_within_the_tie_cap.  With the seeds used here NO entry of any case is
tied (that test prints the counts), so nothing is in fact left out.

Inputs: rows N(0, 0.5^2), the adapter of synth.adapter_state_dict, dz N(0, 1 / B^2) (the cosine head's dz at T = 0.01 is of that
order), running statistics that start away from (0, 1)."""
import functools

import pytest
import torch
import torch.nn.functional as F

from dbmm_amd import _lib, adapter, ops, optim, synth
from test_gpu_row_weights import KEYS, LR, MU, T, WD, _make, _momenta, _ns, _text_paths, _trainable, _weights
from test_gpu_supcon import _torch_supcon

gpu = pytest.mark.gpu
F64, F32 = torch.float64, torch.float32
FLOOR = 2.0 ** -23
TIE, TIE_CAP = 1e-5, 0.05
EPS, MOM = 1e-5, 0.1
ETA, G, LAM, TAU = 0.01, 4, 0.5, 0.1
W1, B1, GA, BE, W2, B2 = KEYS

# (B, D, H): one row-tile and K = 4 / 8; K = B = 3, 5 in the batch-reduced GEMMs; D % 16 != 0 (the register-staged loader) at
# 132 and 1020; more than one 64-row / 128-row tile (129, 301); H > 128; H = 128 with D % 128 != 0 (1020, 64): the widths of
# the fast shape on the generic path
SHAPES = [(2, 4, 4), (3, 8, 12), (5, 64, 16), (37, 132, 20), (129, 512, 64), (64, 768, 192), (128, 1024, 256), (301, 1024, 132),
          (37, 1020, 128), (33, 64, 128)]
FAST = [(37, 1024, 128), (256, 1024, 128)]
# (B, D, H, adapter_step_fused or None = the library's default)
CASES = [(B, D, H, None) for B, D, H in SHAPES] + [(B, D, H, f) for B, D, H in FAST for f in (0, 1)]
EVAL_CASES = CASES + [(1, 1024, 128, None), (1, 512, 64, None), (1, 4, 4, None)]
_id = lambda c: f"B{c[0]}_D{c[1]}_H{c[2]}" + ("" if c[3] is None else f"_fused{c[3]}")
STEP_SHAPES = [(37, 1024, 256, None), (10, 132, 20, None), (37, 1024, 128, 0)]
HEADS = ("erm", "weighted", "gdro", "supcon")
# seeds of the rows where seed 5 puts a pre-ReLU value within 1e-5 of zero in the float64 run (in a step of (d): at any of the three
# steps of any head); with these no case has a tied entry
X_SEED = {(128, 1024, 256): 6}
STEP_SEED = {(37, 1024, 256): 10, (37, 1024, 128): 6}


# ---- inputs -----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _inputs(B, D, H):
    sd = synth.adapter_state_dict(3, D, H)
    x = synth.normal(X_SEED.get((B, D, H), 5), f"ag_x{B}_{D}", (B, D), 0.5)
    dz = synth.normal(7, f"ag_dz{B}_{D}", (B, D), 1.0 / B)
    rm = synth.normal(8, f"ag_rm{H}", (H,), 0.1)
    rv = synth.uniform(9, f"ag_rv{H}", (H,), 0.5, 1.5)
    # eval mode: running variances spread over 1e-6 ... 1e3, the two ends present
    e = synth.uniform(10, f"ag_ev{H}", (H,), -6.0, 3.0).double()
    e[0], e[H - 1] = -6.0, 3.0
    return sd, x, dz, rm, rv, (10.0 ** e).float()


# ---- the references, in `dtype` on the CPU ------------------------------------------------------------------------------------------
def _fwd(p, x, rm=None, rv=None):
    """Linear -> BatchNorm1d -> ReLU -> Linear; train mode without (rm, rv), else eval mode on those running statistics"""
    h = x @ p[W1].t() + p[B1]
    if rm is None:
        mean, var = h.mean(0), h.var(0, unbiased=False)
    else:
        mean, var = rm, rv
    invstd = (var + EPS).rsqrt()
    pre = (h - mean) * invstd * p[GA] + p[BE]
    r = torch.relu(pre)
    return dict(h=h, mean=mean, var=var, invstd=invstd, pre=pre, r=r, z=r @ p[W2].t() + p[B2])


@functools.lru_cache(maxsize=None)
def adapter_ref(B, D, H, dtype):
    """forward in train mode, backward from dz, the running statistics after the call"""
    sd, x, dz, rm, rv, _ = _inputs(B, D, H)
    p = {k: sd[k].to(dtype).clone().requires_grad_() for k in KEYS}
    x = x.to(dtype).clone().requires_grad_()
    f = _fwd(p, x)
    f["h"].retain_grad()
    f["z"].backward(dz.to(dtype))
    out = {k: v.detach() for k, v in f.items()}
    out.update({k: p[k].grad for k in KEYS})
    out.update(dh=f["h"].grad, dx=x.grad, rm=(1 - MOM) * rm.to(dtype) + MOM * out["mean"],
               rv=(1 - MOM) * rv.to(dtype) + MOM * out["var"] * B / (B - 1))
    return out


@functools.lru_cache(maxsize=None)
def eval_ref(B, D, H, dtype):
    sd, x, _, rm, _, rv = _inputs(B, D, H)
    with torch.no_grad():
        return _fwd({k: sd[k].to(dtype) for k in KEYS}, x.to(dtype), rm.to(dtype), rv.to(dtype))


def _ties(pre64):
    """[B, H] mask of the float64 pre-ReLU values within TIE of zero; the share of hidden units that hold one stays under the cap"""
    tie = pre64.abs() < TIE
    assert tie.any(0).double().mean().item() <= TIE_CAP
    return tie


def _keep(name, tie):
    """mask of the entries of tensor `name` that are compared (None: all)"""
    if not tie.any():
        return None
    unit = ~tie.any(0)
    if name in ("r", "dh"):
        return ~tie
    if name == "dx":
        return (~tie.any(1))[:, None]
    if name in (W1,):
        return unit[:, None]
    if name in (B1, GA, BE):
        return unit
    return None


def errs(got, r64, r32, keep=None):
    got, r64, r32 = got.detach().double().cpu(), r64.double(), r32.double()
    assert got.shape == r64.shape and bool(torch.isfinite(got).all())
    if keep is not None:
        keep = keep.expand_as(r64)
        got, r64, r32 = got[keep], r64[keep], r32[keep]
    scale = r64.abs().max().item()
    return ((got - r64).abs().max() / scale).item(), ((r32 - r64).abs().max() / scale).item()


def hold(name, got, r64, r32, keep=None):
    ek, et = errs(got, r64, r32, keep)
    print(f"  {name}: err {ek:.3e} e32 {et:.3e} allowed {4 * et + FLOOR:.3e}")
    assert ek <= 4 * et + FLOOR, (name, ek, et)


# ---- (a) / (b) on the device --------------------------------------------------------------------------------------------------------
def _dev(B, D, H):
    sd, x, dz, rm, rv, ev = _inputs(B, D, H)
    return {k: sd[k].cuda() for k in KEYS}, x.cuda(), dz.cuda(), rm.cuda(), rv.cuda(), ev.cuda()


def _gemm_tag(M, N, K, ta, tw):
    """the kernel dbmm_gemm_bias_act (no workspace: the adapter's composition passes none) picks for op(a) [M, K] x op(w) [N, K]^T"""
    a, w, c = (torch.zeros(n, device="cuda") for n in (M * K, N * K, M * N))
    rc = _lib.lib().dbmm_gemm_bias_act(a.data_ptr(), M if ta else K, ta, w.data_ptr(), N if tw else K, tw, None, None, 0, c.data_ptr(), N, M, N, K,
                                       1.0, 0, _lib.stream())
    assert rc == 0
    return ops._last_igemm_tag()


def _routes(B, D, H):
    """the GEMM kernels of the generic composition at (B, D, H): fc1, fc2, dW2, dr, dW1, dx"""
    return {_gemm_tag(*g) for g in ((B, H, D, 0, 0), (B, D, H, 0, 0), (D, H, B, 1, 1), (B, H, D, 0, 1), (H, D, B, 1, 1), (B, D, H, 0, 1))}


@gpu
@pytest.mark.parametrize("case", CASES, ids=_id)
def test_forward_backward_train_mode_against_float64(case, option):
    """(a) ops.adapter_fwd / ops.adapter_bwd called directly in train mode: z, h, mean, invstd, r, the six gradients, dh, dx =
    ops.gemm(dh, w1, trans_w=True), the updated running_mean / running_var (unbiased, momentum 0.1) and num_batches_tracked.  At the
    two fast shapes once per implementation (adapter_step_fused = 0: this file's subject; 1: csrc/adapter_step.hip): the same bound
    for both.
    Measured on an MI355X: see MEASURED at the end of this file."""
    B, D, H, fused = case
    if fused is not None:
        option("adapter_step_fused", fused)
    r64, r32 = adapter_ref(B, D, H, F64), adapter_ref(B, D, H, F32)
    tie = _ties(r64["pre"])
    p, x, dz, rm, rv, _ = _dev(B, D, H)
    nbt = torch.tensor(7, dtype=torch.int64, device="cuda")
    composed = not (H == 128 and D % 128 == 0 and fused != 0)
    sentinel = _gemm_tag(4, 4, 4, 1, 1)                 # a launch with both operands K-major, which no forward issues
    z, h, mean, invstd, r = ops.adapter_fwd(x, p[W1], p[B1], p[GA], p[BE], rm, rv, nbt, p[W2], p[B2], True)
    fwd_tag = ops._last_igemm_tag()
    # the implementation this case is about did run: the composition ends in fc2 on the general GEMM, the fast kernels launch none
    assert (fwd_tag != sentinel) == composed, (fwd_tag, sentinel)
    sentinel = _gemm_tag(4, 4, 4, 0, 0)                 # and the backward's last GEMM is dW1, K-major
    grads = ops.adapter_bwd(x, dz, h, mean, invstd, r, p[GA], p[BE], p[W2])
    assert (ops._last_igemm_tag() != sentinel) == composed
    dh = grads[6]
    dx = ops.gemm(dh, p[W1], trans_w=True)
    torch.cuda.synchronize()
    print(f"B={B} D={D} H={H} fused={fused}: tied entries {int(tie.sum())}; last forward GEMM {fwd_tag if composed else 'none'}")
    if composed:
        print("  GEMM kernels of the composition: " + "; ".join(sorted(_routes(B, D, H))))
    got = dict(z=z, h=h, mean=mean, invstd=invstd, r=r, dh=dh, dx=dx, rm=rm, rv=rv)
    got.update(zip(KEYS, grads[:6]))
    for name, t in got.items():
        if name == B1:
            a = t.abs().max().item()
            print(f"  {name}: max |db1| {a:.3e} (analytically zero; float64 {r64[name].abs().max().item():.1e})")
            assert a <= 1e-5
            continue
        hold(name, t, r64[name], r32[name], _keep(name, tie))
    assert nbt.item() == 8


@gpu
@pytest.mark.parametrize("case", EVAL_CASES, ids=_id)
def test_forward_eval_mode_against_float64(case, option):
    """(b) eval mode, one row included (which never matches the fast shape), running variances from 1e-6 to 1e3: z and r against
    float64 (ReLU is continuous, so no entry is left out of a forward), the running statistics and num_batches_tracked bit-unchanged.
    Measured on an MI355X: see MEASURED."""
    B, D, H, fused = case
    if fused is not None:
        option("adapter_step_fused", fused)
    r64, r32 = eval_ref(B, D, H, F64), eval_ref(B, D, H, F32)
    p, x, _, rm, _, ev = _dev(B, D, H)
    nbt = torch.tensor(7, dtype=torch.int64, device="cuda")
    rm0, ev0 = rm.clone(), ev.clone()
    assert ev.min().item() <= 1.01e-6 and ev.max().item() >= 0.99e3
    z, h, mean, invstd, r = ops.adapter_fwd(x, p[W1], p[B1], p[GA], p[BE], rm, ev, nbt, p[W2], p[B2], False)
    torch.cuda.synchronize()
    print(f"B={B} D={D} H={H} fused={fused} eval")
    assert mean is None and invstd is None
    hold("h", h, r64["h"], r32["h"])
    hold("r", r, r64["r"], r32["r"])
    hold("z", z, r64["z"], r32["z"])
    assert torch.equal(rm, rm0) and torch.equal(ev, ev0) and nbt.item() == 7


@gpu
def test_reference_batches_take_the_pinned_gemm_kernels():
    """the reference's default batch (128) and ragged last batches (59: Waterbirds' 4795 rows; 82: CelebA's 162770) at D in {512,
    768, 1024}, H in {64, 256} launch no GEMM instantiation that the shapes of (a) do not launch"""
    pinned = set().union(*(_routes(B, D, H) for B, D, H in SHAPES + FAST))
    print("pinned: " + "; ".join(sorted(pinned)))
    for B in (128, 59, 82):
        for D in (512, 768, 1024):
            for H in (64, 256):
                extra = _routes(B, D, H) - pinned
                assert not extra, (B, D, H, extra)


LONG_K = [(128, 256, 1024, 0, 1), (64, 128, 1001, 1, 1), (64, 64, 2048, 1, 0), (64, 64, 1020, 0, 0), (128, 32, 1024, 0, 1), (130, 64, 1024, 0, 1)]


@gpu
@pytest.mark.parametrize("M,N,K,ta,tw", LONG_K, ids=[f"M{m}_N{n}_K{k}_trans{a}{w}" for m, n, k, a, w in LONG_K])
def test_generic_loader_gemm_long_reductions(M, N, K, ta, tw):
    """What the first run of (a) found: the GEMM modes of the generic loader (a K-major operand, or K % 16 != 0) summed all of K in
    one float32 chain.  dr = dz W2 of (B, D, H) = (128, 1024, 256) -- the first case here, on those very operands -- measured 1.72e-06
    against 3.06e-07 for the same product on the buffer-descriptor loader and 3.19e-07 for torch's float32 matmul, and dh missed the
    file's bound (1.95e-06 against 1.49e-06 allowed).  On one chain the six cases measured 1.72e-06, 8.8e-07, 1.30e-06, 1.27e-06,
    1.30e-06, 1.10e-06 -- 2.9 ... 5.4 x torch's -- and the first and the fourth (K = 1020, mode 00) failed here; the other four sat
    just inside 4 x e32 + 2^-23.
    Those modes now move their running sums into a second accumulator set every 128 products, as the buffer-descriptor loader's
    tiles do (csrc/igemm_f32.hip, TWO_LEVEL).  One case per mode and per tile with at most two accumulator blocks a wave, K > 128,
    against float64 under the file's bound, e32 = torch's float32 matmul.  Measured on an MI355X: see MEASURED."""
    if (M, N, K, ta, tw) == (128, 256, 1024, 0, 1):
        sd, _, a, _, _, _ = _inputs(128, 1024, 256)                       # dz [B, D] and W2 [D, H]: K-major along D
        w = sd[W2]
    else:
        a = synth.normal(21, f"lk_a{M}_{K}", (K, M) if ta else (M, K))
        w = synth.normal(22, f"lk_w{N}_{K}", (K, N) if tw else (N, K), K ** -0.5)
    am, wm = (a.t() if ta else a), (w.t() if tw else w)
    got = ops.gemm(a.cuda(), w.cuda(), trans_a=bool(ta), trans_w=bool(tw))
    print(f"M={M} N={N} K={K} trans {ta}{tw}: {ops._last_igemm_tag()}")
    hold("c", got, am.double() @ wm.double().t(), am @ wm.t())


# ---- (c) the input gradient through the module ----------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("B,D,H", [(37, 1024, 128), (37, 1024, 256)], ids=["fast", "generic"])
def test_input_gradient_through_the_module(B, D, H):
    """(c) features.grad of adapter.Adapter(D, H) in train mode (_AdapterFn.backward: ops.gemm(dh, w1, trans_w=True)) against
    float64 autograd of the restatement -- with (a), the only pin of dx on either path.  Measured on an MI355X: see MEASURED."""
    r64, r32 = adapter_ref(B, D, H, F64), adapter_ref(B, D, H, F32)
    tie = _ties(r64["pre"])
    sd, x, dz, _, _, _ = _inputs(B, D, H)
    ad = adapter.Adapter(D, H)
    ad.load_state_dict(sd)
    ad = ad.cuda().train()
    feats = x.cuda().requires_grad_(True)
    z = ad(feats)
    z.backward(dz.cuda())
    torch.cuda.synchronize()
    print(f"B={B} D={D} H={H} module")
    hold("z", z, r64["z"], r32["z"])
    hold("dx", feats.grad, r64["dx"], r32["dx"], _keep("dx", tie))
    hold(W1, ad.layers[0].weight.grad, r64[W1], r32[W1], _keep(W1, tie))


# ---- (d) the one-call steps ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def text_paths_by_dim(tmp_path_factory):
    cache = {}

    def get(D):
        if D not in cache:
            cache[D] = _text_paths(tmp_path_factory, D)
        return cache[D]
    return get


def _batch(B, D, H):
    x = synth.normal(STEP_SEED.get((B, D, H), 5), f"ag_sx{B}_{D}", (B, D), 0.5)
    y = synth.labels(6, B)[0]
    g = torch.arange(B) % (G - 1)
    g[5] = G - 1                                                       # a one-row group
    return x, y, g


def _gdro(rows, g, q, dtype):
    """one online group-DRO update (tests/test_group_dro_host.py gdro_update) in `dtype`: -> (new q, row weights, robust loss)"""
    n = torch.stack([(g == k).sum() for k in range(G)])
    L = torch.stack([rows[g == k].sum() / n[k] if n[k] else torch.zeros((), dtype=dtype) for k in range(G)])
    qn = q * torch.exp(ETA * (L - L[n > 0].max()))
    qn = qn / qn.sum()
    w = torch.where(n > 0, qn / n.clamp(min=1), torch.zeros((), dtype=dtype))
    return qn, w[g], (qn * L).sum()


@functools.lru_cache(maxsize=None)
def step_ref(B, D, H, multiple, head, dtype, steps=3):
    """`steps` SGD-momentum steps from the states _make() loads, in `dtype`: the total update of the six trainable tensors, both
    adapters' running statistics, q, each step's loss / logits / L_con, and the largest share of tied hidden units of any step"""
    x, y, g = _batch(B, D, H)
    x = x.to(dtype)
    text = synth.text_matrix(1, D, 2, "class").to(dtype)
    tn = text / text.norm(dim=0, keepdim=True)
    w = _weights(B).to(dtype)
    new = {k: v.to(dtype) for k, v in synth.adapter_state_dict(4 if multiple else 3, D, H).items()}
    old = {k: v.to(dtype) for k, v in synth.adapter_state_dict(3, D, H).items()} if multiple else None
    start = {k: new[k].clone() for k in KEYS}
    stats = {"new": [new["layers.1.running_mean"], new["layers.1.running_var"]]}
    if multiple:
        stats["old"] = [old["layers.1.running_mean"], old["layers.1.running_var"]]
    q = torch.full((G,), 1.0 / G, dtype=dtype)
    bufs, out, tied = {}, dict(loss=[], losses=[], logits=[], con=[]), 0.0

    def track(which, f):
        rm, rv = stats[which]
        stats[which] = [(1 - MOM) * rm + MOM * f["mean"].detach(), (1 - MOM) * rv + MOM * f["var"].detach() * B / (B - 1)]

    for _ in range(steps):
        ps = {k: new[k].clone().requires_grad_() for k in KEYS}
        f = _fwd(ps, x)
        track("new", f)
        tied = max(tied, (f["pre"].detach().abs() < TIE).any(0).double().mean().item())
        z = f["z"]
        feat = z / z.norm(dim=1, keepdim=True)
        if multiple:
            with torch.no_grad():
                fo = _fwd(old, x)
            track("old", fo)
            feat = 0.5 * fo["z"] / fo["z"].norm(dim=1, keepdim=True) + 0.5 * feat
        logits = feat @ tn / T
        rows = F.cross_entropy(logits, y, reduction="none")
        if head == "erm":
            loss = rows.mean()
        elif head == "weighted":
            loss = (rows * w).mean()
        elif head == "gdro":
            q, wrow, _ = _gdro(rows.detach(), g, q, dtype)
            loss = (wrow * rows).sum()
        else:
            con = _torch_supcon(z, y, TAU)
            out["con"].append(con.detach())
            loss = (1 - LAM) * rows.mean() + LAM * con
        loss.backward()
        out["loss"].append(loss.detach())
        out["losses"].append(torch.cat([rows.detach(), loss.detach()[None]]))
        out["logits"].append(logits.detach())
        for k in KEYS:
            gr = ps[k].grad + WD * new[k]
            bufs[k] = gr if k not in bufs else MU * bufs[k] + gr
            new[k] = new[k] - LR * bufs[k]
    out.update({k: new[k] - start[k] for k in KEYS})
    out.update(q=q, tied=tied)
    for which, (rm, rv) in stats.items():
        out[which + "_rm"], out[which + "_rv"] = rm, rv
    return out


def _head_kw(head, B, gd):
    if head == "weighted":
        return dict(row_weights=_weights(B).cuda())
    if head == "gdro":
        return dict(robust=(adapter.GroupDRO(G, ETA, "cuda"), gd))
    if head == "supcon":
        return dict(contrastive=(LAM, TAU))
    return {}


def _gpu_steps(B, D, H, multiple, head, paths, one_call, steps=3):
    clf, opt = _make(D, H, paths, multiple)
    start = {k: v.detach().clone() for k, v in _trainable(clf).state_dict().items() if k in KEYS}
    x, y, g = (t.cuda() for t in _batch(B, D, H))
    kw = _head_kw(head, B, g)
    outs = []
    for _ in range(steps):
        if one_call:
            o = clf.train_step(x, y, opt, **kw)
        else:
            o = clf.loss(x, y, **kw)
            opt.zero_grad(); o[0].backward(); opt.step()
        outs.append([t.detach().clone() for t in o] + ([kw["robust"][0].q.clone()] if head == "gdro" else []))
    torch.cuda.synchronize()
    return clf, opt, start, kw, outs


def _bn(ad):
    return ad.layers[1]


def _loss_of_own_rows(head, o, B, g):
    """the step's loss recombined in float64 from the kernel's OWN float32 per-row CE (and its own q / L_con)"""
    rows = o[2].double().cpu()
    if head == "weighted":
        return (rows * _weights(B).double()).mean()
    if head == "gdro":
        L = torch.stack([rows[g == k].mean() if bool((g == k).any()) else torch.zeros((), dtype=F64) for k in range(G)])
        return (o[-1].double().cpu() * L).sum()
    if head == "supcon":
        return (1 - LAM) * rows.mean() + LAM * o[3].double().cpu()
    return rows.mean()


@gpu
@pytest.mark.parametrize("multiple", [False, True], ids=["alone", "old_adapter"])
@pytest.mark.parametrize("head", HEADS)
@pytest.mark.parametrize("shape", STEP_SHAPES, ids=_id)
def test_one_call_steps_off_the_fast_shape(shape, head, multiple, text_paths_by_dim, option):
    """(d) dbmm_adapter_train_step, _weighted, _gdro and _supcon through CustomCLIP.train_step / MultipleAdapter.train_step, three
    consecutive steps (the momentum carries over), with and without the frozen old adapter (whose BatchNorm runs in train mode: its
    running statistics move, and are compared).  Against step_ref in float64 under the file's bound: the total update of every
    trainable tensor, the running statistics and num_batches_tracked of both adapters, q, and each step's loss, logits and L_con.
    layers.0.bias: every step's gradient is held to 1e-5 absolutely, so its total update to 1e-5 * lr * (1 + 1.9 + 2.71).
    Then what train_step's docstring promises: three loss(...).backward(); optimizer.step() steps from the same start leave
    torch.equal parameters, buffers, momentum buffers, logits and losses.  Measured on an MI355X: see MEASURED."""
    B, D, H, fused = shape
    if fused is not None:
        option("adapter_step_fused", fused)
    r64, r32 = step_ref(B, D, H, multiple, head, F64), step_ref(B, D, H, multiple, head, F32)
    assert r64["tied"] <= TIE_CAP
    paths = text_paths_by_dim(D)
    clf, opt, start, kw, outs = _gpu_steps(B, D, H, multiple, head, paths, True)
    print(f"B={B} D={D} H={H} fused={fused} head={head} old={multiple}: tied units {r64['tied']:.3f}")
    ad = _trainable(clf)
    sd = ad.state_dict()
    for k in KEYS:
        upd = sd[k].double() - start[k].double()
        if k == B1:
            a = (upd.cpu() - r64[k]).abs().max().item()
            print(f"  {k}: |update - ref| {a:.3e}, |ref| {r64[k].abs().max().item():.3e}")
            assert a <= 1e-5 * LR * (1 + 1.9 + 2.71)
        else:
            hold(k, upd, r64[k], r32[k])
    hold("new running_mean", _bn(ad).running_mean, r64["new_rm"], r32["new_rm"])
    hold("new running_var", _bn(ad).running_var, r64["new_rv"], r32["new_rv"])
    assert _bn(ad).num_batches_tracked.item() == 3
    if multiple:
        oad = clf.old_cls.adapter
        hold("old running_mean", _bn(oad).running_mean, r64["old_rm"], r32["old_rm"])
        hold("old running_var", _bn(oad).running_var, r64["old_rv"], r32["old_rv"])
        assert _bn(oad).num_batches_tracked.item() == 3
    if head == "gdro":
        hold("q", kw["robust"][0].q, r64["q"], r32["q"])
    g = _batch(B, D, H)[2]
    for s, o in enumerate(outs):
        # the loss is ONE number: its own e32 is one sample of a rounding error and says nothing (B = 10, gdro: the float32 restatement
        # landed 1.2e-09 from float64 at the first step, the kernel two ulps, 1.5e-07).  It is a convex combination (mean, weighted
        # mean, sum_g q_g L_g) of the per-row CE the step returns beside it, so it is held as the last element of that tensor, [B + 1]
        # as the library lays it out; and, as tests/test_gpu_row_weights.py holds the weighted mean, to the float64 recombination of
        # the kernel's own rows: B same-sign terms summed in float32, in any order, plus the weights' products and the division
        # stay within (B + 16) * 2^-24 of the sum.  The bare figures are printed.
        e, e32 = errs(o[0], r64["loss"][s], r32["loss"][s])
        own = _loss_of_own_rows(head, o, B, g)
        e_own = abs(o[0].item() - own.item()) / abs(own.item())
        print(f"  loss[{s}] {o[0].item():.6e} alone: err {e:.3e} e32 {e32:.3e}; against its own rows {e_own:.3e}, allowed {(B + 16) * 2.0 ** -24:.3e}")
        assert e_own <= (B + 16) * 2.0 ** -24
        hold(f"rows | loss[{s}]", torch.cat([o[2], o[0][None]]), r64["losses"][s], r32["losses"][s])
        hold(f"logits[{s}]", o[1], r64["logits"][s], r32["logits"][s])
        if head == "supcon":
            hold(f"L_con[{s}]", o[3], r64["con"][s], r32["con"][s])
    # the autograd path from the same start: the same bits
    clf2, opt2, _, kw2, outs2 = _gpu_steps(B, D, H, multiple, head, paths, False)
    for s, (o, o2) in enumerate(zip(outs, outs2)):
        assert len(o) == len(o2)
        for i, (a, b) in enumerate(zip(o, o2)):
            assert torch.equal(a, b), (s, i)
    for (k, va), (_, vb) in zip(clf.state_dict().items(), clf2.state_dict().items()):
        assert torch.equal(va, vb), k
    for ma, mb in zip(_momenta(clf, opt), _momenta(clf2, opt2)):
        assert torch.equal(ma, mb)
    if head == "gdro":
        assert torch.equal(kw["robust"][0].q, kw2["robust"][0].q)


def test_float64_references_stay_within_the_tie_cap():
    """no GPU: every float64 reference of (a), (c) and (d) keeps its tied hidden units within the 5 % cap -- with these seeds, at 0"""
    worst = 0.0
    for B, D, H in sorted(set(c[:3] for c in CASES) | {(37, 1024, 256)}):
        pre = adapter_ref(B, D, H, F64)["pre"]
        tie = pre.abs() < TIE
        share = tie.any(0).double().mean().item()
        print(f"(a) B={B} D={D} H={H}: {int(tie.sum())} tied entries, {share:.4f} of the units; smallest |pre| {pre.abs().min().item():.2e}")
        worst = max(worst, share)
    for B, D, H, _ in STEP_SHAPES:
        for head in HEADS:
            for multiple in (False, True):
                share = step_ref(B, D, H, multiple, head, F64)["tied"]
                print(f"(d) B={B} D={D} H={H} {head} old={multiple}: {share:.4f} of the units tied")
                worst = max(worst, share)
    assert worst <= TIE_CAP
    assert worst == 0.0                  # what the module docstring says: with these seeds the tie masks leave nothing out


# ---- (e) buffers ----------------------------------------------------------------------------------------------------------------------
class _Zone:
    """n float32 between two guard zones of PAD sentinel words; `fill` is what the n floats start as"""
    PAD, S = 4096, 0x7FA5A5A5

    def __init__(self, n, fill=0.0):
        self.n = n
        self.raw = torch.full((n + 2 * self.PAD,), self.S, dtype=torch.int32, device="cuda")
        self.t = self.raw[self.PAD:self.PAD + n].view(torch.float32)
        self.t.fill_(fill)
        self.ptr = self.t.data_ptr()

    def intact(self):
        return bool((self.raw[:self.PAD] == self.S).all()) and bool((self.raw[self.PAD + self.n:] == self.S).all())


@gpu
def test_direct_entries_stay_inside_outputs_and_an_exact_workspace(text_paths_by_dim):
    """(e) dbmm_adapter_fwd, dbmm_adapter_bwd and dbmm_adapter_train_step (with the old adapter) called through the C entries at
    (B, D, H) = (37, 132, 20) -- odd B, H = 4 * 5, D % 16 != 0: a shape of (a), and (d)'s (10, 132, 20) at an odd batch, none of
    (d)'s own shapes having both an odd B and H = 4 x odd -- with every output and a NaN-filled workspace of exactly
    dbmm_workspace_bytes_adapter_bwd / dbmm_workspace_bytes_adapter_train_step bytes between guard zones: the zones intact, every
    output finite and equal to the wrappers' result; one byte less of workspace: DBMM_E_WORKSPACE, nothing written"""
    B, D, H, C = 37, 132, 20, 2
    L, st = _lib.lib(), _lib.stream()
    nan = float("nan")
    p, x, dz, rm, rv, _ = _dev(B, D, H)
    rm2, rv2 = rm.clone(), rv.clone()
    nbt, nbt2 = (torch.tensor(0, dtype=torch.int64, device="cuda") for _ in range(2))
    want = ops.adapter_fwd(x, p[W1], p[B1], p[GA], p[BE], rm2, rv2, nbt2, p[W2], p[B2], True)
    wgrads = ops.adapter_bwd(x, dz, want[1], want[2], want[3], want[4], p[GA], p[BE], p[W2])
    zs = dict(h=_Zone(B * H, nan), mean=_Zone(H, nan), invstd=_Zone(H, nan), r=_Zone(B * H, nan), z=_Zone(B * D, nan))
    rc = L.dbmm_adapter_fwd(x.data_ptr(), p[W1].data_ptr(), p[B1].data_ptr(), p[GA].data_ptr(), p[BE].data_ptr(), rm.data_ptr(), rv.data_ptr(),
                            nbt.data_ptr(), p[W2].data_ptr(), p[B2].data_ptr(), zs["h"].ptr, zs["mean"].ptr, zs["invstd"].ptr, zs["r"].ptr,
                            zs["z"].ptr, B, D, H, 1, EPS, MOM, st)
    assert rc == 0
    torch.cuda.synchronize()
    for (name, zone), w in zip(zs.items(), (want[1], want[2], want[3], want[4], want[0])):
        assert zone.intact(), name
        assert torch.equal(zone.t, w.flatten()) and bool(torch.isfinite(zone.t).all()), name
    nbytes = L.dbmm_workspace_bytes_adapter_bwd(B, D, H)
    assert nbytes == 2 * B * H * 4
    gz = [_Zone(n, nan) for n in (H * D, H, H, H, D * H, D)]
    ws = _Zone(nbytes // 4, nan)
    args = (x.data_ptr(), dz.data_ptr(), zs["h"].ptr, zs["mean"].ptr, zs["invstd"].ptr, zs["r"].ptr, p[GA].data_ptr(), p[BE].data_ptr(),
            p[W2].data_ptr(), *(g.ptr for g in gz), B, D, H, ws.ptr)
    assert L.dbmm_adapter_bwd(*args, nbytes - 1, st) == -3                       # DBMM_E_WORKSPACE
    torch.cuda.synchronize()
    assert all(bool(torch.isnan(g.t).all()) for g in gz) and bool(torch.isnan(ws.t).all())
    assert L.dbmm_adapter_bwd(*args, nbytes, st) == 0
    torch.cuda.synchronize()
    assert ws.intact() and all(g.intact() for g in gz)
    for g, w in zip(gz, wgrads[:6]):
        assert torch.equal(g.t, w.flatten()) and bool(torch.isfinite(g.t).all())
    assert bool(torch.isfinite(ws.t).all())                                      # dr | dh: the whole workspace is written

    # the one-call step with the old adapter
    paths = text_paths_by_dim(D)
    xs, ys, _ = (t.cuda() for t in _batch(B, D, H))
    ref, oref = _make(D, H, paths, True)
    wl, wlogits, wrows = ref.train_step(xs, ys, oref)
    clf, opt = _make(D, H, paths, True)
    plan, first = clf._plan(opt, "train_step")
    sbytes = L.dbmm_workspace_bytes_adapter_train_step(B, D, H, 1)
    lg, ls, sws = _Zone(B * C, nan), _Zone(B + 1, nan), _Zone(sbytes // 4, nan)
    tn = clf._text("class", xs.device)
    call = lambda nb: L.dbmm_adapter_train_step(xs.data_ptr(), ys.data_ptr(), *plan["args"], 0.5, tn.data_ptr(), T, LR, MU, WD, int(first), lg.ptr,
                                                ls.ptr, ls.ptr + 4 * B, B, D, H, C, sws.ptr, nb, st)
    before = {k: v.clone() for k, v in clf.state_dict().items()}
    assert call(sbytes - 1) == -3
    torch.cuda.synchronize()
    assert bool(torch.isnan(sws.t).all()) and bool(torch.isnan(lg.t).all())
    for k, v in clf.state_dict().items():
        assert torch.equal(v, before[k]), k
    assert call(sbytes) == 0
    torch.cuda.synchronize()
    assert lg.intact() and ls.intact() and sws.intact()
    assert torch.equal(lg.t.view(B, C), wlogits) and torch.equal(ls.t[:B], wrows) and torch.equal(ls.t[B], wl)
    for (k, va), (_, vb) in zip(clf.state_dict().items(), ref.state_dict().items()):
        assert torch.equal(va, vb) and bool(torch.isfinite(va.double()).all()), k
    for ma, mb in zip(_momenta(clf, opt), _momenta(ref, oref)):
        assert torch.equal(ma, mb)


# ---- (f) refusals ---------------------------------------------------------------------------------------------------------------------
REFUSED = [(8, 1024, 30), (8, 1022, 128), (8, 1022, 30), (1, 1024, 128), (1, 1024, 256)]


@gpu
@pytest.mark.parametrize("B,D,H", REFUSED, ids=["H30", "D1022", "D1022_H30", "one_row_H128", "one_row_H256"])
def test_refused_shapes_leave_the_state_alone(B, D, H, tmp_path_factory):
    """(f) H % 4 != 0 (Adapter(1024, 30), which the reference accepts), D % 4 != 0 and one row in train mode, through ops.adapter_fwd,
    Adapter.forward and train_step: each raises, and each leaves every parameter, running_mean, running_var and num_batches_tracked
    with the bits it had.  Before dbmm_adapter_fwd checked its shape first, H = 30 got as far as the BatchNorm statistics kernel,
    which advanced the three buffers before dbmm_bn1d_relu refused."""
    ad = adapter.Adapter(D, H)
    ad.load_state_dict(synth.adapter_state_dict(3, D, H))
    with torch.no_grad():
        ad.layers[1].running_mean.copy_(synth.normal(8, f"ag_rm{H}", (H,), 0.1))
        ad.layers[1].running_var.copy_(synth.uniform(9, f"ag_rv{H}", (H,), 0.5, 1.5))
    clf = adapter.CustomCLIP(ad, *_text_paths(tmp_path_factory, D), temperature=T).cuda().train()
    opt = optim.set_optimizer(_ns(), clf)
    x = synth.normal(5, f"ag_x{B}_{D}", (B, D), 0.5).cuda()
    y = synth.labels(6, B)[0].cuda()
    before = {k: v.clone() for k, v in clf.state_dict().items()}
    assert sum(k.endswith(s) for k in before for s in ("running_mean", "running_var", "num_batches_tracked")) == 3

    def unchanged(what):
        torch.cuda.synchronize()
        for k, v in clf.state_dict().items():
            assert torch.equal(v, before[k]), (what, k)

    l0, bn, l3 = ad.layers[0], ad.layers[1], ad.layers[3]
    with pytest.raises(_lib.DbmmError, match="multiples of 4" if B > 1 else "at least 2 rows"):
        ops.adapter_fwd(x, l0.weight.detach(), l0.bias.detach(), bn.weight.detach(), bn.bias.detach(), bn.running_mean, bn.running_var,
                        bn.num_batches_tracked, l3.weight.detach(), l3.bias.detach(), True)
    unchanged("ops.adapter_fwd")
    # the library itself, without the wrapper's check in front of it: DBMM_E_SHAPE before any launch
    scratch = torch.full((2 * B * (D + H) + 2 * H + 16,), float("nan"), device="cuda")
    sp = scratch.data_ptr()
    rc = _lib.lib().dbmm_adapter_fwd(x.data_ptr(), l0.weight.data_ptr(), l0.bias.data_ptr(), bn.weight.data_ptr(), bn.bias.data_ptr(),
                                     bn.running_mean.data_ptr(), bn.running_var.data_ptr(), bn.num_batches_tracked.data_ptr(),
                                     l3.weight.data_ptr(), l3.bias.data_ptr(), sp, sp, sp, sp, sp, B, D, H, 1, EPS, MOM, _lib.stream())
    assert rc == -1
    unchanged("dbmm_adapter_fwd")
    assert bool(torch.isnan(scratch).all())
    with pytest.raises((RuntimeError, ValueError)):
        ad(x)
    unchanged("Adapter.forward")
    with pytest.raises((RuntimeError, ValueError)):
        clf.loss(x, y)
    unchanged("CustomCLIP.loss")
    with pytest.raises((RuntimeError, ValueError)):
        clf.train_step(x, y, opt)
    unchanged("train_step")
    if B > 1:
        ad.eval()
        with pytest.raises((RuntimeError, ValueError)):                          # eval mode refuses the widths too
            ad(x)
        unchanged("Adapter.forward (eval)")


MEASURED = """On an MI355X, largest err (largest e32) per tensor; the bound is err <= 4 * e32 + 2^-23 case by case.
(a) the composition, B >= 3 (eleven cases, the two fast shapes with adapter_step_fused = 0 among them): z 4.7e-07 (4.3e-07), h 3.7e-07
    (4.0e-07), mean 2.7e-07 (4.5e-07), invstd 2.4e-07 (1.8e-07), r 3.9e-07 (3.7e-07), dh 4.5e-07 (6.3e-07), dx 6.0e-07 (5.8e-07),
    layers.0.weight 4.8e-07 (4.9e-07), layers.1.weight 4.5e-07 (4.6e-07), layers.1.bias 2.7e-07 (3.1e-07), layers.3.weight 4.0e-07
    (4.3e-07), layers.3.bias 1.2e-07 (1.7e-07), running_mean 7.1e-08 (7.1e-08), running_var 9.7e-08 (9.7e-08); max |db1| 4.1e-07.
    B = 2 (dh is (1 - xhat^2) (d1 - d2) / 2, 1e-4 of dr): dh 2.4e-05 (4.7e-04), dx 1.8e-05 (4.0e-04), layers.0.weight 2.4e-05 (4.4e-04),
    invstd 2.5e-07 (1.1e-07), the rest below 2.2e-07.  Closest to its bound: invstd and r at 0.44 of it.
    the fast kernels at (37, 1024, 128), (256, 1024, 128): z 3.2e-07, h 2.6e-07, mean 2.6e-07, invstd 1.3e-07, r 2.7e-07, dh 2.8e-07,
    dx 6.0e-07, the gradients 1.7e-07 ... 2.7e-07, max |db1| 2.5e-07 (e32 as in the composition's rows: same references).
    Before the generic loader's GEMM modes summed K in blocks of 128: dh 7.1e-07 ... 1.95e-06 at every D >= 512 (e32 3.1e-07 ... 6.3e-07),
    1.95e-06 against 1.49e-06 allowed at (128, 1024, 256), which failed.
    GEMM kernels of the composition, igemm_f32_kernel<BM, BN, WAVES_M, WAVES_N, AMODE, WMODE, BK, MINB, FAST, SK, DMA>:
      <128, 32, 4, 1, 0, 0, 16, 5, 0, 0, 0>, <128, 32, 4, 1, 0, 0, 16, 6, 1, 0, 1>, <128, 32, 4, 1, 0, 1, 16, 5, 0, 0, 0>,
      <128, 32, 4, 1, 2, 1, 16, 5, 0, 0, 0>, <128, 64, 2, 2, 0, 0, 16, 5, 1, 0, 1>, <128, 64, 2, 2, 0, 1, 16, 4, 0, 0, 0>,
      <128, 64, 2, 2, 2, 1, 16, 4, 0, 0, 0>, <64, 64, 2, 2, 0, 0, 16, 5, 0, 0, 0>, <64, 64, 2, 2, 0, 0, 16, 6, 1, 0, 1>,
      <64, 64, 2, 2, 0, 1, 16, 5, 0, 0, 0>, <64, 64, 2, 2, 2, 1, 16, 5, 0, 0, 0>
    (fc1 / fc2: modes 00 on the buffer-descriptor loader, FAST = 1, or the generic one where K % 16 != 0; dr and dx: 01; dW1, dW2: 21).
    The reference's batches (128, 59, 82) at D in {512, 768, 1024}, H in {64, 256} launch none but these (asserted).
(b) eval, 17 cases, one row included: h 3.7e-07 (4.0e-07), r 3.3e-07 (4.0e-07), z 4.1e-07 (4.8e-07).
(c) through the module: dx 4.1e-07 (4.6e-07) fast, 3.7e-07 (3.7e-07) generic; z 3.6e-07 (4.3e-07); layers.0.weight 3.2e-07 (3.7e-07).
(d) 24 cases of three steps: updates of layers.0.weight 1.1e-06 (2.3e-06), layers.1.weight 9.4e-06 (9.4e-06), layers.1.bias 1.1e-06
    (2.5e-06), layers.3.weight 1.1e-06 (2.2e-06), layers.3.bias 3.2e-06 (6.0e-06); layers.0.bias |update - ref| <= 3.9e-07 of 5.6e-06
    allowed; running_mean 2.4e-06 (2.1e-06; one case, err 2.37e-06 e32 6.3e-07, at 0.90 of its bound: the closest of the file),
    running_var 1.5e-06 (2.3e-06), the old adapter's 3.2e-07 (3.6e-07) and 2.3e-07 (2.3e-07); logits 9.4e-07 (1.8e-05); rows | loss
    4.6e-06 (4.9e-05); q 8.0e-08 (1.0e-06); L_con 1.6e-07 (1.7e-07).  The loss alone: err up to 3.8e-05 (a loss of 0.002), above
    4 * e32 + 2^-23 of its own in 1 of 72; against the float64 recombination of the kernel's rows <= 0.07 of (B + 16) * 2^-24.
    Steps and autograd path: torch.equal in all 24.
long reductions: err 3.1e-07, 2.4e-07, 2.3e-07, 2.6e-07, 2.4e-07, 2.4e-07 (e32 3.2e-07, 3.1e-07, 3.2e-07, 2.7e-07, 3.0e-07, 3.8e-07).
The 70 GPU cases take 3.8 - 4.3 s together, the slowest 1.2 s (the first one, which loads the library)."""
