"""Developer tool (GPU box): the adapter train step with the supervised-contrastive head -- us/step, in one
process, of
    erm_one_call      the ERM one-call step (dbmm_adapter_train_step)
    mixed_one_call    the mixed one-call step (dbmm_adapter_train_step_supcon)
    mixed_autograd    the mixed step through the autograd path on the same kernels (loss(contrastive=).backward(); optimizer.step())
    mixed_torch       the mixed step with the contrastive term composed from torch ops (matmul, logsumexp, autograd) on the adapter's z
    head_only         dbmm_supcon_fwd + dbmm_supcon_bwd alone on a fixed z (the three added launches)
    empty_launches    three launches of a one-element fill: the box's floor for three launches
over `repeats` alternating windows of `steps` steps each; prints every window and the medians.
    python tools/bench_supcon_step.py [B] [D] [steps] [repeats]        (defaults 256 1024 500 7; H = 128, weight 0.5, tau 0.1)"""
import json
import os
import statistics
import sys
import tempfile
import time
from types import SimpleNamespace

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import dbmm_amd  # noqa: E402,F401
from dbmm_amd import adapter, ops, optim, synth  # noqa: E402

B = int(sys.argv[1]) if len(sys.argv) > 1 else 256
D = int(sys.argv[2]) if len(sys.argv) > 2 else 1024
steps = int(sys.argv[3]) if len(sys.argv) > 3 else 500
repeats = int(sys.argv[4]) if len(sys.argv) > 4 else 7
LAM, TAU, T = 0.5, 0.1, 0.01
d = tempfile.mkdtemp()
paths = []
for nm, C in (("c", 2), ("s", 2), ("g", 4)):
    m = synth.text_matrix(1, D, C, nm); p = os.path.join(d, nm + ".json")
    json.dump({f"{nm}{i}": m[:, i].tolist() for i in range(C)}, open(p, "w")); paths.append(p)
ad = adapter.Adapter(D, 128); ad.load_state_dict(synth.adapter_state_dict(3, D, 128))
clf = adapter.CustomCLIP(ad, *paths, temperature=T).cuda().train()
opt = optim.set_optimizer(SimpleNamespace(learning_rate=0.1, momentum=0.9, weight_decay=5e-5), clf)
x = synth.normal(5, f"x{B}", (B, D), 0.5).cuda()
y = synth.labels(6, B)[0].cuda()
z0 = synth.normal(7, f"z{B}", (B, D), 1.0).cuda()
one = torch.zeros(1, device="cuda")


def torch_supcon(z, y, tau):
    zn = z / z.norm(dim=1, keepdim=True)
    S = zn @ zn.t() / tau
    eye = torch.eye(len(y), dtype=torch.bool, device=z.device)
    pos = (y[:, None] == y[None, :]) & ~eye
    n_pos = pos.sum(1)
    l = torch.logsumexp(S.masked_fill(eye, float("-inf")), dim=1) - (S * pos).sum(1) / n_pos.clamp(min=1)
    anchors = n_pos > 0
    return (l * anchors).sum() / anchors.sum().clamp(min=1)


def erm():
    clf.train_step(x, y, opt)


def mixed_one_call():
    clf.train_step(x, y, opt, contrastive=(LAM, TAU))


def mixed_autograd():
    loss = clf.loss(x, y, contrastive=(LAM, TAU))[0]
    opt.zero_grad(); loss.backward(); opt.step()


def mixed_torch():
    z, z_old = clf._features(x)
    ce = adapter._SimCEFn.apply(z, z_old, clf._text("class", x.device), T, 0.5, y)[0]
    loss = (1 - LAM) * ce + LAM * torch_supcon(z, y, TAU)
    opt.zero_grad(); loss.backward(); opt.step()


def head_only():
    _, _, stats, n_anchors, ws, _ = ops.supcon_fwd(z0, y, TAU)
    ops.supcon_bwd(z0, y, TAU, stats, n_anchors, ws, LAM)


def empty_launches():
    one.fill_(1.0); one.fill_(2.0); one.fill_(3.0)


modes = (("erm_one_call", erm), ("mixed_one_call", mixed_one_call), ("mixed_autograd", mixed_autograd), ("mixed_torch", mixed_torch),
         ("head_only", head_only), ("empty_launches", empty_launches))
for _, fn in modes:
    for _ in range(20):
        fn()
times = {name: [] for name, _ in modes}
for rep in range(repeats):
    for name, fn in modes:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            fn()
        torch.cuda.synchronize()
        times[name].append((time.perf_counter() - t0) / steps * 1e6)
for name, _ in modes:
    print(f"B={B} D={D} {name}: median {statistics.median(times[name]):.1f} us/step of {repeats} windows x {steps} steps: "
          + " ".join(f"{t:.1f}" for t in times[name]))
print(f"launches: ERM {ops.adapter_step_launches(B, D, 128)}, mixed {ops.adapter_step_launches(B, D, 128, contrastive=True)}")
