"""The fused linear-probe step (csrc/linear_step.hip, LinearClassifier.train_step) and its eval forward (LinearClassifier.loss) on the
MI355X: three consecutive steps against an fp64 restatement, bit-identical repeats, equality with the autograd path
(`loss.backward(); optimizer.step()`) and alternation with it, guard zones around every output and parameter, deepcopy independence,
and the wrappers' shape checks.  B covers one row, ragged rows, both the one-launch and the two-launch reductions."""
import copy

import pytest
import torch
import torch.nn.functional as F

from dbmm_amd import _lib, adapter, ops, optim

pytestmark = pytest.mark.gpu

TOL = 1e-5


def _rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-30)).item()


def _data(B, D, C, seed=0):
    g = torch.Generator().manual_seed(seed * 1000 + B + 7 * D + C)
    x = (torch.randn(B, D, generator=g) * 0.5).cuda()
    y = torch.randint(0, C, (B,), generator=g).cuda()
    return x, y


def _classifier(D, C, seed=1):
    torch.manual_seed(seed)
    return adapter.LinearClassifier(D, C).cuda().train()


def _ref_step(x, y, W, b, mW, mb, lr, mu, wd, first):
    """fp64 restatement of one step (torch.optim.SGD semantics, dampening 0)"""
    x, W, b = x.double().cpu(), W.double().cpu(), b.double().cpu()
    y = y.cpu()
    B = x.shape[0]
    logits = x @ W.T + b
    rows = torch.logsumexp(logits, 1) - logits[torch.arange(B), y]
    d = (torch.softmax(logits, 1) - F.one_hot(y, W.shape[0]).double()) / B
    gW, gb = d.T @ x + wd * W, d.sum(0) + wd * b
    mW = gW if first else mu * mW.double().cpu() + gW
    mb = gb if first else mu * mb.double().cpu() + gb
    return logits, rows, rows.mean(), W - lr * mW, b - lr * mb, mW, mb


@pytest.mark.parametrize("B", [1, 3, 128, 255, 1024, 4097, 8192])
@pytest.mark.parametrize("C", [2, 4])
@pytest.mark.parametrize("D", [512, 768, 1024])
def test_three_steps_against_fp64_and_repeatable(D, C, B):
    x, y = _data(B, D, C)
    clf = _classifier(D, C)
    opt = optim.SGD(clf.parameters(), lr=0.1, momentum=0.9, weight_decay=5e-5)
    w, b = clf.fc.weight, clf.fc.bias
    for step, wd in enumerate((5e-5, 5e-5, 0.0)):
        opt.param_groups[0]["weight_decay"] = wd
        first = step == 0
        before = [t.detach().clone() for t in (w, b)]
        bufs = [None, None] if first else [opt.state[p]["momentum_buffer"].clone() for p in (w, b)]
        # a bit-identical repeat from the same state first (on copies), then the real step
        if not first:
            cw, cb, cmw, cmb = (t.clone() for t in (before[0], before[1], bufs[0], bufs[1]))
            r1 = ops.linear_train_step(x, y, cw, cb, cmw, cmb, 0.1, 0.9, wd, False)
            dw, db, dmw, dmb = (t.clone() for t in (before[0], before[1], bufs[0], bufs[1]))
            r2 = ops.linear_train_step(x, y, dw, db, dmw, dmb, 0.1, 0.9, wd, False)
            for u, v in zip(r1 + (cw, cb, cmw, cmb), r2 + (dw, db, dmw, dmb)):
                assert torch.equal(u, v), "two runs on identical inputs differ"
        loss, logits, rows = clf.train_step(x, y, opt)
        rl, rr, rm, rW, rb, rmW, rmb = _ref_step(x, y, before[0], before[1], bufs[0], bufs[1], 0.1, 0.9, wd, first)
        assert logits.shape == (B, C) and rows.shape == (B,) and loss.dim() == 0
        # per-row CE to 1e-5 of max(1, CE): a well-separated row's CE (1e-12 after a step at B = 1) is far below the logits' rounding
        assert (rows.double().cpu() - rr).abs().max().item() <= TOL * max(1.0, rr.abs().max().item()), (step, "loss_rows")
        for name, got, ref in (("logits", logits, rl), ("W", w, rW), ("b", b, rb),
                               ("m_w", opt.state[w]["momentum_buffer"], rmW), ("m_b", opt.state[b]["momentum_buffer"], rmb)):
            assert _rel(got, ref) < TOL, (step, name, _rel(got, ref))
        assert abs(loss.item() - rm.item()) <= TOL * max(1.0, abs(rm.item())), (step, loss.item(), rm.item())


@pytest.mark.parametrize("B", [3, 255, 4097])
def test_fused_step_equals_the_autograd_path_and_alternates_with_it(B):
    D, C = 1024, 2
    x, y = _data(B, D, C, seed=2)
    a = _classifier(D, C, seed=3)
    b = copy.deepcopy(a)
    oa = optim.SGD(a.parameters(), lr=0.05, momentum=0.9, weight_decay=5e-5)
    ob = optim.SGD(b.parameters(), lr=0.05, momentum=0.9, weight_decay=5e-5)

    def autograd_step(clf, opt):
        out = clf(x)
        loss = F.cross_entropy(out, y)
        opt.zero_grad(); loss.backward(); opt.step()
        return loss

    for rnd in range(4):                               # fused on a / autograd on b, then the other way round
        if rnd % 2 == 0:
            la, _, _ = a.train_step(x, y, oa)
            lb = autograd_step(b, ob)
        else:
            la = autograd_step(a, oa)
            lb, _, _ = b.train_step(x, y, ob)
        assert abs(la.item() - lb.item()) <= TOL * max(1.0, abs(lb.item())), rnd
        for pa, pb in zip(a.parameters(), b.parameters()):
            assert _rel(pa, pb) < TOL, rnd
            assert _rel(oa.state[pa]["momentum_buffer"], ob.state[pb]["momentum_buffer"]) < TOL, rnd


@pytest.mark.parametrize("B", [255, 4097])
def test_both_reductions_agree(B, option):
    D, C = 768, 4
    x, y = _data(B, D, C, seed=4)
    clf = _classifier(D, C, seed=5)
    outs = []
    for max_b in (1 << 30, 0):                        # everything in one launch / everything in two
        option("linear_step_one_launch_max_b", max_b)
        w, b = clf.fc.weight.detach().clone(), clf.fc.bias.detach().clone()
        mw, mb = torch.zeros_like(w), torch.zeros_like(b)
        loss, logits, rows = ops.linear_train_step(x, y, w, b, mw, mb, 0.1, 0.9, 5e-5, True)
        outs.append((loss, logits, rows, w, b, mw, mb))
    for u, v in zip(*outs):
        assert _rel(u, v) < 1e-6


@pytest.mark.parametrize("B", [1, 255, 4096])
def test_eval_loss_equals_the_forward(B):
    D, C = 1024, 4
    x, y = _data(B, D, C, seed=6)
    clf = _classifier(D, C, seed=7).eval()
    mean, logits, rows = clf.loss(x, y)
    with torch.no_grad():
        ref = clf(x)
    ref_rows = F.cross_entropy(ref, y, reduction="none")
    assert _rel(logits, ref) < TOL and (rows - ref_rows).abs().max().item() <= TOL * max(1.0, ref_rows.abs().max().item())
    assert abs(mean.item() - ref_rows.double().mean().item()) <= TOL * max(1.0, ref_rows.double().mean().abs().item())
    m2, l2, r2 = clf.loss(x, y)
    assert torch.equal(m2, mean) and torch.equal(l2, logits) and torch.equal(r2, rows)


class _Guarded:
    S = -7.0

    def __init__(self):
        self.bufs = []

    def __call__(self, shape, device=None, dtype=torch.float32, **kw):
        shape = (shape,) if isinstance(shape, int) else tuple(shape)
        n = 1
        for s in shape:
            n *= s
        pad = 4096
        raw = torch.empty(n + 2 * pad, device=device, dtype=dtype)
        raw[:pad] = self.S; raw[pad + n:] = self.S
        self.bufs.append((raw, pad, n))
        return raw[pad:pad + n].view(shape)

    def like(self, t):
        out = self(tuple(t.shape), device=t.device, dtype=t.dtype)
        out.copy_(t)
        return out

    def check(self):
        for raw, pad, n in self.bufs:
            assert bool((raw[:pad] == self.S).all()) and bool((raw[pad + n:] == self.S).all()), f"guard zone of a {n}-element tensor written"


@pytest.mark.parametrize("B", [1, 77, 1024, 4097])
@pytest.mark.parametrize("D,C", [(512, 3), (1024, 8)])
def test_guard_zones_around_outputs_and_parameters(B, D, C, monkeypatch):
    x, y = _data(B, D, C, seed=8)
    ga = _Guarded()
    monkeypatch.setattr(ops, "_empty", ga)
    monkeypatch.setattr(ops, "_linear_ws", {})                   # the workspace between guard zones too
    g = torch.Generator().manual_seed(9)
    w, b = ga.like(torch.randn(C, D, generator=g).cuda() * 0.03), ga.like(torch.randn(C, generator=g).cuda() * 0.03)
    mw, mb = ga.like(torch.zeros(C, D, device="cuda")), ga.like(torch.zeros(C, device="cuda"))
    xg, yg = ga.like(x), ga.like(y)
    for step in range(2):
        loss, logits, rows = ops.linear_train_step(xg, yg, w, b, mw, mb, 0.1, 0.9, 5e-5, step == 0)
    assert torch.isfinite(logits).all() and torch.isfinite(w).all()
    ops.linear_ce_fwd(xg, yg, w, b)
    torch.cuda.synchronize()
    ga.check()


def test_deepcopy_after_a_fused_step_is_independent():
    D, C, B = 512, 2, 64
    x, y = _data(B, D, C, seed=10)
    clf = _classifier(D, C, seed=11)
    opt = optim.SGD(clf.parameters(), lr=0.1, momentum=0.9, weight_decay=5e-5)
    clf.train_step(x, y, opt)
    snap = copy.deepcopy(clf)
    frozen = [p.detach().clone() for p in snap.parameters()]
    clf.train_step(x, y, opt)
    for p, f in zip(snap.parameters(), frozen):
        assert torch.equal(p, f)                                 # the original's step left the copy alone
    assert not torch.equal(clf.fc.weight, snap.fc.weight)
    before = [p.detach().clone() for p in clf.parameters()]
    opt2 = optim.SGD(snap.parameters(), lr=0.1, momentum=0.9, weight_decay=5e-5)
    snap.train_step(x, y, opt2)
    for p, f in zip(clf.parameters(), before):
        assert torch.equal(p, f)                                 # and the copy's step leaves the original alone
    assert not torch.equal(snap.fc.weight, frozen[0])


def test_wrappers_refuse_bad_operands_before_launching():
    D, C, B = 512, 2, 16
    x, y = _data(B, D, C, seed=12)
    clf = _classifier(D, C, seed=13)
    w, b = clf.fc.weight.detach(), clf.fc.bias.detach()
    mw, mb = torch.zeros_like(w), torch.zeros_like(b)
    w0 = w.clone()
    bad = [
        (x[:, :D - 4].contiguous(), y, w, b, mw, mb),                 # D mismatch
        (x, y[:-1], w, b, mw, mb),                                     # labels length
        (x, y.int(), w, b, mw, mb),                                    # labels dtype
        (x.t(), y, w, b, mw, mb),                                      # non-contiguous
        (x.cpu(), y, w, b, mw, mb),                                    # device
        (x, y, w, b, mw[:1], mb),                                      # momentum buffer shape
        (x, y, w, b[:1].contiguous(), mw, mb),                         # bias size
        (x.double(), y, w, b, mw, mb),                                 # dtype
    ]
    for args in bad:
        with pytest.raises((_lib.DbmmError, RuntimeError)):
            ops.linear_train_step(*args, 0.1, 0.9, 0.0, True)
    w9 = torch.zeros(9, D, device="cuda")                              # C > 8
    with pytest.raises(_lib.DbmmError):
        ops.linear_ce_fwd(x, y, w9, torch.zeros(9, device="cuda"))
    w_big = torch.zeros(C, 1028, device="cuda")                        # D > 1024
    with pytest.raises(_lib.DbmmError):
        ops.linear_ce_fwd(torch.zeros(B, 1028, device="cuda"), y, w_big, b)
    torch.cuda.synchronize()
    assert torch.equal(w, w0) and not mw.any()
    opt = optim.SGD(clf.parameters(), lr=0.1, momentum=0.9)
    with pytest.raises(ValueError):
        clf.train_step(x, y, opt, use_group=True)
    other = torch.nn.Parameter(torch.zeros(3, device="cuda"))
    with pytest.raises(RuntimeError):
        clf.train_step(x, y, optim.SGD(list(clf.parameters()) + [other], lr=0.1, momentum=0.9))
    with pytest.raises(RuntimeError):
        clf.eval().train_step(x, y, opt)
    assert torch.equal(clf.fc.weight, w0)
