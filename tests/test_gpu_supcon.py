"""The supervised-contrastive head on the MI355X: the Gram / reduction / backward kernels against the reference's own
SupervisedContrastiveLoss (tests/golden/supcon.npz) and the float64 restatement of tests/test_supcon_host.py, the one-call mixed
step against a float64 torch-CPU restatement (the oracle pattern of tests/test_gpu_group_dro.py plus the contrastive term), the
autograd path, and the schedule.

Bound on l_i and L_con: 2e-5 / tau absolute.  The project bounds a cosine by 1e-5 (1e-3 on a logit at T = 0.01); a shift of at most
eps in every S_ij moves the logsumexp and the positive mean by at most eps each."""
import os
import re

import numpy as np
import pytest
import torch

from dbmm_amd import _lib, adapter, ops, optim, synth, trainer
from test_gpu_group_dro import (KEYS, LR, MU, T, WD, _batch, _make, _momenta, _oracle_adapter, _same_records, _schedule_opt, _trainable,
                                schedule_data, text_paths_by_dim)  # noqa: F401  (the last two are fixtures)
from test_supcon_host import golden_cases, supcon_ref

pytestmark = pytest.mark.gpu
LAM, TAU = 0.5, 0.1
RAGGED = ((130, 192), (257, 1024))             # one past two tiles of a 64-wide and of a 128-wide tiling


def _bound(tau):
    return 2e-5 / tau


def _ragged_case(B, D):
    """rows of uneven length; five labels in turn, one row with a label of its own"""
    z = synth.normal(11, f"supcon_z{B}_{D}", (B, D), 1.0) * synth.uniform(11, f"supcon_s{B}", (B, 1), 0.5, 2.0)
    y = (torch.arange(B) % 5) * 1000 - 7
    y[B // 2] = 123456789
    return z.contiguous(), y


def _fwd(z, y, tau):
    con, rows, stats, n_anchors, ws, _ = ops.supcon_fwd(z.cuda(), y.cuda(), tau)
    return con, rows, stats, n_anchors, ws


def _torch_supcon(z, y, tau):
    """the loss composed from torch ops (matmul, logsumexp; autograd for the gradient) in z's dtype, on z's device"""
    zn = z / z.norm(dim=1, keepdim=True)
    S = zn @ zn.t() / tau
    eye = torch.eye(len(y), dtype=torch.bool, device=z.device)
    pos = (y[:, None] == y[None, :]) & ~eye
    n_pos = pos.sum(1)
    l = torch.logsumexp(S.masked_fill(eye, float("-inf")), dim=1) - (S * pos).sum(1) / n_pos.clamp(min=1)
    anchors = n_pos > 0
    return (l * anchors).sum() / anchors.sum().clamp(min=1)


# ---- 1. forward against the reference golden ------------------------------------------------------------------------------------------
def test_forward_against_the_reference_class():
    """every golden case: l_i of the anchors and L_con against the reference class's float64 numbers; the one row without positives
    (not scored by the reference) has l = 0 and is not counted: A = B - 1.
    Measured on an MI355X: max |l_i - ref| 6.2e-07 (tau 0.1) and 1.1e-06 (tau 0.05) against bounds of 2e-4 and 4e-4; |L_con - ref|
    <= 3.7e-07."""
    n = 0
    for c, z, y, tau, rows_ref, mean_ref, _, _ in golden_cases():
        con, rows, stats, n_anchors, _ = _fwd(torch.from_numpy(z), torch.from_numpy(y), tau)
        rows = rows.double().cpu().numpy()
        anchors = rows_ref != 0
        e_rows, e_mean = np.abs(rows - rows_ref)[anchors].max(), abs(con.item() - mean_ref)
        print(f"{c}: max |l - ref| {e_rows:.3e}, |L_con - ref| {e_mean:.3e}, bound {_bound(tau):.1e}")
        assert anchors.sum() == len(y) - 1 and n_anchors.item() == len(y) - 1
        assert (rows[~anchors] == 0).all() and (stats[2].cpu().numpy()[~anchors] == 0).all()
        assert e_rows <= _bound(tau) and e_mean <= _bound(tau), c
        n += 1
    assert n == 8


# ---- 2. ragged multi-tile shapes ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,D", RAGGED)
def test_ragged_multi_tile_forward(B, D):
    """Measured on an MI355X: max |l - ref| 7.2e-07 at (130, 192) and 9.1e-07 at (257, 1024); bound 2e-4."""
    z, y = _ragged_case(B, D)
    l, L, _, A = supcon_ref(z.numpy(), y.numpy(), TAU)
    con, rows, stats, n_anchors, _ = _fwd(z, y, TAU)
    e_rows, e_mean = np.abs(rows.double().cpu().numpy() - l).max(), abs(con.item() - L)
    print(f"B={B} D={D}: max |l - ref| {e_rows:.3e}, |L_con - ref| {e_mean:.3e}, bound {_bound(TAU):.1e}")
    assert A == B - 1 and n_anchors.item() == A
    assert e_rows <= _bound(TAU) and e_mean <= _bound(TAU)
    inv = 1.0 / np.linalg.norm(z.double().numpy(), axis=1)
    assert np.abs(stats[3].double().cpu().numpy() - inv).max() <= 1e-6 * inv.max()


# ---- 3. backward ---------------------------------------------------------------------------------------------------------------------
def _backward_cases():
    for c, z, y, tau, _, _, _, _ in golden_cases():
        yield c, torch.from_numpy(z), torch.from_numpy(y), tau
    for B, D in RAGGED:
        yield f"ragged_b{B}_d{D}", *_ragged_case(B, D), TAU


def test_backward_against_float64():
    """err = max|dz - ref| / max|ref| against the float64 restatement, for the golden shapes and the ragged ones.  Allowed: 4 x the
    same error of the loss composed from fp32 torch ops on the GPU (matmul, logsumexp, autograd), measured here -- the margin
    tests/test_gpu_group_dro.py grants a differently ordered fixed-order reduction.  The output is weight * dL_con/dz alone, or
    fma(dz_in_scale, dz_in, weight * dL_con/dz), the documented expression.
    Measured on an MI355X, kernel err (ratio to the torch composition's): the eight golden cases 1.6e-07 (1.06), 2.0e-07 (1.25),
    1.9e-07 (0.70), 3.2e-07 (1.63), 3.4e-07 (1.49), 2.4e-07 (1.29), 7.2e-07 (1.56), 5.0e-07 (1.22); (130, 192) 4.3e-07 (1.05);
    (257, 1024) 5.5e-07 (1.08)."""
    for c, z, y, tau in _backward_cases():
        ref = torch.from_numpy(supcon_ref(z.numpy(), y.numpy(), tau)[2])
        zd, yd = z.cuda(), y.cuda()
        _, _, stats, n_anchors, ws = _fwd(z, y, tau)
        dz = ops.supcon_bwd(zd, yd, tau, stats, n_anchors, ws)
        zt = zd.clone().requires_grad_()
        _torch_supcon(zt, yd, tau).backward()
        err = lambda a: ((a.double().cpu() - ref).abs().max() / ref.abs().max()).item()
        e_k, e_t = err(dz), err(zt.grad)
        print(f"{c}: kernel err {e_k:.3e}, torch fp32 err {e_t:.3e}, ratio {e_k / e_t:.2f} (allowed 4)")
        assert e_k <= 4 * e_t, c
        dz_in = synth.normal(12, "supcon_dzin" + c, tuple(z.shape), 0.01).cuda()
        mixed = ops.supcon_bwd(zd, yd, tau, stats, n_anchors, ws, 0.3, dz_in=dz_in, dz_in_scale=0.7)
        # fma(s, dz_in, fl32(lam * dz)): the float64 sum of the exact product and the rounded one, within one float32 rounding
        lam, s = np.float32(0.3), np.float32(0.7)
        want = float(s) * dz_in.double().cpu() + torch.from_numpy(lam * dz.cpu().numpy()).double()
        assert torch.allclose(mixed.double().cpu(), want, rtol=2.0 ** -23, atol=0.0), c


# ---- 4. edge cases ---------------------------------------------------------------------------------------------------------------------
def _run_edge(z, y, tau):
    con, rows, stats, n_anchors, ws = _fwd(z, y, tau)
    dz = ops.supcon_bwd(z.cuda(), y.cuda(), tau, stats, n_anchors, ws)
    for t in (con, rows, stats, dz):
        assert torch.isfinite(t).all()
    return con.item(), rows.double().cpu().numpy(), dz.double().cpu().numpy(), n_anchors.item()


def _check_edge(z, y, tau, what):
    l, L, d, A = supcon_ref(z.numpy(), y.numpy(), tau)
    con, rows, dz, n_anchors = _run_edge(z, y, tau)
    print(f"{what}: |L_con - ref| {abs(con - L):.3e}, max |l - ref| {np.abs(rows - l).max():.3e}, bound {_bound(tau):.1e}")
    assert n_anchors == A and abs(con - L) <= _bound(tau) and np.abs(rows - l).max() <= _bound(tau), what
    # dz (its own check is test 3): a logit within eps = 1e-5 / tau (the project's bound on a cosine) moves every softmax weight by a
    # factor within e^(+-2 eps), and G is a signed sum of such weights: 2 eps relative to max|dz|, doubled
    assert np.abs(dz - d).max() <= 4e-5 / tau * np.abs(d).max() + 1e-12, what
    return con, rows, dz


def test_edge_cases():
    z = synth.normal(13, "supcon_edge", (37, 128), 1.0)
    _check_edge(z, torch.full((37,), 3, dtype=torch.int64), TAU, "all labels equal")         # A = B, no negatives
    con, rows, dz, A = _run_edge(z, torch.arange(37), TAU)                                   # all labels distinct: A = 0
    assert A == 0 and con == 0.0 and not rows.any() and not dz.any()
    con, rows, dz = _check_edge(z[:2].contiguous(), torch.tensor([5, 5]), TAU, "B = 2")
    assert np.abs(rows).max() <= 1e-6                                                        # one other row: lse == the positive mean
    _check_edge(z[:2].contiguous(), torch.tensor([5, 6]), TAU, "B = 2, two labels")
    z2 = z.clone()
    z2[9] = z2[4]                                                                            # two identical rows: S_ij = 1 / tau
    y2 = torch.arange(37) % 3
    _check_edge(z2, y2, TAU, "identical rows")
    _check_edge(z, y2, 0.01, "tau = 0.01")                                                   # logits up to 100
    _check_edge(z2, y2, 0.01, "identical rows at tau = 0.01")
    big = torch.tensor([2 ** 62 + 1, -(2 ** 62), 2 ** 40 + 3])[y2]                           # labels that differ in the high word only
    a, b = _check_edge(z, big, TAU, "large labels"), _check_edge(z, y2, TAU, "small labels")
    assert a[0] == b[0] and np.array_equal(a[2], b[2])


def test_no_anchor_mixed_step_is_the_weighted_ce_step(text_paths_by_dim):
    """four rows with the four group ids on the group prompts: no row has a positive, so con == 0 and the mixed loss is
    (1 - weight) * mean CE to the bit (weight 0.5; the reduction takes the CE mean with mean_reduce_kernel's statements)"""
    x = _batch(4, 128, 1)[0].cuda()
    y = torch.arange(4).cuda()
    a, _ = _make(128, 128, text_paths_by_dim(128), False)
    b, _ = _make(128, 128, text_paths_by_dim(128), False)
    ce, logits_a, rows_a = a.loss(x, y, use_group=True)
    mixed, logits_b, rows_b, con = b.loss(x, y, use_group=True, contrastive=(LAM, TAU))
    assert con.item() == 0.0 and torch.equal(logits_a, logits_b) and torch.equal(rows_a, rows_b)
    assert mixed.item() == (1 - LAM) * ce.item()
    ce.backward(); mixed.backward()
    for pa, pb in zip(a.adapter.parameters(), b.adapter.parameters()):
        assert torch.allclose(pb.grad, (1 - LAM) * pa.grad, rtol=1e-5, atol=1e-9)


def test_no_anchor_mixed_loss_is_the_weighted_ce():
    """all labels distinct: con == 0, dz_con == 0 exactly, mixed loss == (1 - weight) * mean CE, through the head's own entries"""
    B, D = 37, 128
    z = synth.normal(13, "supcon_edge", (B, D), 1.0).cuda()
    y = torch.arange(B).cuda()
    ce_rows = synth.uniform(14, "supcon_ce", (B,), 0.0, 5.0).cuda()
    con, _, stats, n_anchors, ws, mixed = ops.supcon_fwd(z, y, TAU, ce_rows=ce_rows, weight=LAM)
    ce = ops.supcon_fwd(z, y, TAU, ce_rows=ce_rows, weight=0.0)[5]                           # weight 0: the mean CE itself
    assert con.item() == 0.0 and n_anchors.item() == 0.0
    assert abs(ce.item() - ce_rows.double().mean().item()) <= 1e-6 * ce.item()
    assert mixed.item() == (1 - LAM) * ce.item()
    dz_in = synth.normal(12, "supcon_dzin_a0", (B, D), 0.01).cuda()
    dz = ops.supcon_bwd(z, y, TAU, stats, n_anchors, ws, LAM, dz_in=dz_in, dz_in_scale=1 - LAM)
    assert torch.equal(dz, dz_in * (1 - LAM))
    assert not ops.supcon_bwd(z, y, TAU, stats, n_anchors, ws, LAM).any()


# ---- 5. guard zones --------------------------------------------------------------------------------------------------------------------
class _Guarded:
    """stand-in for ops._empty: every tensor sits between two sentinel-filled zones of 4096 elements"""
    G, S = 4096, 777

    def __init__(self):
        self.bufs = []

    def __call__(self, shape, device=None, dtype=torch.float32):
        n = int(np.prod(shape)) if not isinstance(shape, int) else shape
        buf = torch.full((n + 2 * self.G,), self.S, device=device, dtype=dtype)
        self.bufs.append((buf, n))
        return buf[self.G:self.G + n].view(shape)

    def check(self):
        assert self.bufs
        for buf, n in self.bufs:
            assert (buf[:self.G] == self.S).all() and (buf[self.G + n:] == self.S).all(), f"guard zone of a {n}-element tensor was written"


@pytest.mark.parametrize("B,D", [(37, 128), (130, 192)])
def test_guard_zones(B, D, monkeypatch):
    """dz, the per-row outputs (statistics, l, the scalars: one allocation) and the workspace sit between guard zones"""
    z, y = _ragged_case(B, D)
    zd, yd = z.cuda(), y.cuda()
    ce_rows = synth.uniform(14, "supcon_ce", (B,), 0.0, 5.0).cuda()
    ga = _Guarded()
    monkeypatch.setattr(ops, "_empty", ga)
    con, rows, stats, n_anchors, ws, mixed = ops.supcon_fwd(zd, yd, TAU, ce_rows=ce_rows, weight=LAM)
    dz = ops.supcon_bwd(zd, yd, TAU, stats, n_anchors, ws, LAM)
    dz2 = ops.supcon_bwd(zd, yd, TAU, stats, n_anchors, ws, LAM, dz_in=dz, dz_in_scale=0.5)
    torch.cuda.synchronize()
    assert len(ga.bufs) == 4
    ga.check()
    assert torch.isfinite(dz).all() and torch.isfinite(dz2).all() and torch.isfinite(mixed)
    assert ws.numel() * 4 == _lib.lib().dbmm_supcon_workspace_bytes(B, D)


# ---- 6. three mixed steps against float64 ----------------------------------------------------------------------------------------------
def _oracle_run(D, H, x, y, text, multiple, contrastive, steps=3):
    """`steps` SGD-momentum steps in float64 from the states _make() loads -> {key: update of the trainable tensor}; `contrastive` =
    (weight, tau) adds the contrastive term on the trainable adapter's z, None is the ERM step"""
    x, text = x.double(), text.double()
    new = {k: v.double() for k, v in synth.adapter_state_dict(4 if multiple else 3, D, H).items()}
    old = {k: v.double() for k, v in synth.adapter_state_dict(3, D, H).items()} if multiple else None
    start = {k: new[k].clone() for k in KEYS}
    bufs = {}
    tn = text / text.norm(dim=0, keepdim=True)
    for _ in range(steps):
        ps = {k: new[k].clone().requires_grad_() for k in KEYS}
        z, _, _ = _oracle_adapter(ps, x)
        f = z / z.norm(dim=1, keepdim=True)
        if multiple:
            with torch.no_grad():
                zo, _, _ = _oracle_adapter(old, x)
            f = 0.5 * zo / zo.norm(dim=1, keepdim=True) + 0.5 * f
        loss = torch.nn.functional.cross_entropy(f @ tn / T, y)
        if contrastive is not None:
            loss = (1 - contrastive[0]) * loss + contrastive[0] * _torch_supcon(z, y, contrastive[1])
        loss.backward()
        for k in KEYS:
            gr = ps[k].grad + WD * new[k]
            bufs[k] = gr if k not in bufs else MU * bufs[k] + gr
            new[k] = new[k] - LR * bufs[k]
    return {k: new[k] - start[k] for k in KEYS}


def _gpu_run(D, H, x, y, paths, multiple, contrastive, steps=3):
    clf, opt = _make(D, H, paths, multiple)
    ad = _trainable(clf)
    start = {k: v.detach().clone() for k, v in ad.state_dict().items() if k in KEYS}
    xd, yd = x.cuda(), y.cuda()
    for _ in range(steps):
        out = clf.train_step(xd, yd, opt, contrastive=contrastive)
        assert len(out) == (3 if contrastive is None else 4) and torch.isfinite(out[0])
    sd = ad.state_dict()
    return {k: (sd[k].double() - start[k].double()).cpu() for k in KEYS}


@pytest.mark.parametrize("B,D,H,multiple", [(37, 128, 128, False), (10, 64, 16, False), (37, 128, 128, True)],
                         ids=["fast", "generic", "old_adapter"])
def test_mixed_step_against_float64_oracle(B, D, H, multiple, text_paths_by_dim):
    """Three consecutive mixed steps at weight 0.5, tau 0.1 (the momentum carries over): per trainable tensor, err = max|update -
    update_ref| / max|update_ref| of the three steps' total update; allowed 4 x the same quantity of the ERM train_step against its
    float64 restatement on the same inputs, measured here.  layers.0.bias as in tests/test_gpu_group_dro.py: its gradient is
    analytically zero (a bias in front of train-mode BatchNorm), so its update is bounded absolutely, 4 x 1e-5 on the gradient through
    three momentum steps.
    Measured on an MI355X, worst tensor by mixed / ERM ratio (ERM err -> mixed err): fast layers.1.weight 4.5e-07 -> 7.7e-07
    (1.69 x), generic layers.1.weight 2.3e-07 -> 4.4e-07 (1.96 x), old adapter layers.3.bias 2.0e-07 -> 4.3e-07 (2.15 x); every mixed
    err <= 2.3e-06.  layers.0.bias: 0.7e-02 ... 4.5e-02 of its own tiny update."""
    x, y, _ = _batch(B, D)
    paths = text_paths_by_dim(D)
    text = synth.text_matrix(1, D, 2, "class")
    erm_ref, erm = _oracle_run(D, H, x, y, text, multiple, None), _gpu_run(D, H, x, y, paths, multiple, None)
    mix_ref, mix = _oracle_run(D, H, x, y, text, multiple, (LAM, TAU)), _gpu_run(D, H, x, y, paths, multiple, (LAM, TAU))
    err = lambda a, b: ((a - b).abs().max() / b.abs().max()).item()
    for k in KEYS:
        e_erm, e_mix = err(erm[k], erm_ref[k]), err(mix[k], mix_ref[k])
        print(f"B={B} D={D} H={H} old={multiple} {k}: ERM err {e_erm:.3e}, mixed err {e_mix:.3e}, allowed {4 * e_erm:.3e}")
    for k in KEYS:
        if k == "layers.0.bias":
            assert (mix[k] - mix_ref[k]).abs().max().item() <= 4 * 1e-5 * LR * (1 + 1.9 + 2.71), k
        else:
            assert err(mix[k], mix_ref[k]) <= 4 * err(erm[k], erm_ref[k]), k
    assert err(mix["layers.3.weight"], erm["layers.3.weight"]) > 1e-3                      # the contrastive term did change the update


# ---- 7. bit identity -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,D,H,multiple", [(37, 128, 128, False), (37, 128, 128, True), (10, 64, 16, False)])
def test_one_call_step_equals_autograd_path_and_repeats(B, D, H, multiple, text_paths_by_dim):
    x, y, _ = (t.cuda() for t in _batch(B, D))
    a, oa = _make(D, H, text_paths_by_dim(D), multiple)
    b, ob = _make(D, H, text_paths_by_dim(D), multiple)
    c, oc = _make(D, H, text_paths_by_dim(D), multiple)
    for step in range(3):
        la, logits_a, rows_a, con_a = a.loss(x, y, contrastive=(LAM, TAU))
        oa.zero_grad(); la.backward(); oa.step()
        lb, logits_b, rows_b, con_b = b.train_step(x, y, ob, contrastive=(LAM, TAU))
        lc, logits_c, rows_c, con_c = c.train_step(x, y, oc, contrastive=(LAM, TAU))
        assert con_a.dim() == 0 and con_b.dim() == 0 and con_b.is_cuda and con_b.item() > 0
        for u, v, w in ((la.detach(), lb, lc), (logits_a, logits_b, logits_c), (rows_a, rows_b, rows_c), (con_a, con_b, con_c)):
            assert torch.equal(u, v) and torch.equal(v, w), step
    for (k, va), (_, vb), (_, vc) in zip(a.state_dict().items(), b.state_dict().items(), c.state_dict().items()):
        assert torch.equal(va, vb) and torch.equal(vb, vc), k                              # parameters and running statistics
    for ma, mb, mc in zip(_momenta(a, oa), _momenta(b, ob), _momenta(c, oc)):
        assert torch.equal(ma, mb) and torch.equal(mb, mc)
    # without contrastive= nothing changes: the 3-tuple, and a mixed module can go on with plain steps
    out = b.train_step(x, y, ob)
    assert len(out) == 3
    with pytest.raises(ops.DbmmUnsupported):
        b.train_step(x, y, ob, contrastive=(LAM, TAU), robust=(adapter.GroupDRO(4, 0.01, "cuda"), y))
    with pytest.raises(ops.DbmmUnsupported):
        b.loss(x, y, contrastive=(LAM, TAU), robust=(adapter.GroupDRO(4, 0.01, "cuda"), y))


# ---- 8. launch count -------------------------------------------------------------------------------------------------------------------
def test_launch_count_is_the_documented_one():
    h = open(os.path.join(_lib.INCLUDE, "dbmm.h")).read()
    doc = h[:h.index("int dbmm_adapter_train_step_supcon(")]
    doc = doc[doc.rindex("/*"):]
    plain, with_old = (int(v) for v in re.search(r"\((\d+) / (\d+) on the fast shape\)", doc).groups())
    assert ops.adapter_step_launches(256, 1024, 128, contrastive=True) == plain == ops.adapter_step_launches(256, 1024, 128) + 3
    assert ops.adapter_step_launches(256, 1024, 128, with_old=True, contrastive=True) == with_old
    assert ops.adapter_step_launches(10, 64, 16, contrastive=True) is None


def test_wrappers_check_their_operands():
    z, y = _ragged_case(37, 128)
    with pytest.raises(RuntimeError):
        ops.supcon_fwd(z, y, TAU)                                                            # CPU tensors
    with pytest.raises(RuntimeError):
        ops.supcon_fwd(z.cuda(), y.cuda()[:-1].contiguous(), TAU)
    with pytest.raises(RuntimeError):
        ops.supcon_fwd(z.cuda(), y.cuda().int(), TAU)
    with pytest.raises(ops.DbmmUnsupported):
        ops.supcon_fwd(torch.zeros(2049, 8, device="cuda"), torch.zeros(2049, dtype=torch.int64, device="cuda"), TAU)


# ---- 9. the schedule -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method,extra", [("adapter", {}), ("adapter_reg_seq_alter", {"add_adapter": True})], ids=["adapter", "seq_alter_add_adapter"])
def test_schedule_runs_contrastive(method, extra, schedule_data):
    paths, tables = schedule_data
    opt = _schedule_opt(method, paths, contrastive_weight=0.5, **extra)
    optim.set_seed(42)
    log = []
    trainer.train_all_epochs(opt, *tables, log=log)
    trains = [e for e in log if e["kind"] in ("train1", "train2")]
    assert len(trains) == 2 and all(np.isfinite(e["loss"]) and np.isfinite(e["con"]) and e["con"] > 0 for e in trains)
    # without the option (absent, or 0) the records are the plain run's, the same whichever way the option is off, and carry no con
    logs0 = []
    for off in ({}, {"contrastive_weight": 0.0}):
        optim.set_seed(42)
        log0 = []
        trainer.train_all_epochs(_schedule_opt(method, paths, **off, **extra), *tables, log=log0)
        assert all("con" not in e for e in log0)
        logs0.append(log0)
    _same_records(*logs0)
    assert [e["loss"] for e in logs0[0] if e["kind"] in ("train1", "train2")] != [e["loss"] for e in trains]


def test_schedule_refusals(schedule_data):
    paths, tables = schedule_data
    with pytest.raises(ops.DbmmUnsupported):
        trainer.train_all_epochs(_schedule_opt("linear_probing", paths, contrastive_weight=0.5), *tables)
    with pytest.raises(ops.DbmmUnsupported):
        trainer.train_all_epochs(_schedule_opt("adapter", paths, contrastive_weight=0.5, robust=True), *tables)
    with pytest.raises(ops.DbmmUnsupported):
        trainer.train_sweep(_schedule_opt("adapter", paths, contrastive_weight=0.5), *tables, [42, 43])
