"""Developer tool (GPU box): the contrastive adapter's step on sampled sets -- us/step, in one process, of
    head_only         dbmm_supcon_sets_fwd + dbmm_supcon_sets_bwd alone on a fixed z (the four launches), with the achieved bytes/s
                      taken as 12 T S D bytes (z read twice, dz written once) over the time
    head_torch        the head composed from torch ops on the same z (normalise, bmm against the gathered anchors, logsumexp,
                      autograd)
    step_one_call     the one-call step (dbmm_adapter_train_step_sets)
    step_autograd     the same step through the autograd path on the same kernels (sets_loss(...).backward(); optimizer.step())
    step_torch        the same step with the head composed from torch ops on the adapter's z
over `repeats` alternating windows of `steps` steps each; prints every window and the medians.
    python tools/bench_contrastive_sets.py [T] [P] [N] [steps] [repeats]        (defaults 32 2048 2048 20 7; D = 1024, H = 128, A = 1)"""
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

T = int(sys.argv[1]) if len(sys.argv) > 1 else 32
P = int(sys.argv[2]) if len(sys.argv) > 2 else 2048
N = int(sys.argv[3]) if len(sys.argv) > 3 else 2048
steps = int(sys.argv[4]) if len(sys.argv) > 4 else 20
repeats = int(sys.argv[5]) if len(sys.argv) > 5 else 7
D, H, A, TAU = 1024, 128, 1, 0.1
S = A + P + N
SETS, SCALE = (T, A, P, N), 1.0 / T
COPY_RATE = 6.29e12                            # measured copy rate of the MI355X, bytes/s
d = tempfile.mkdtemp()
paths = []
for nm, C in (("c", 2), ("s", 2), ("g", 4)):
    m = synth.text_matrix(1, D, C, nm); p = os.path.join(d, nm + ".json")
    json.dump({f"{nm}{i}": m[:, i].tolist() for i in range(C)}, open(p, "w")); paths.append(p)
ad = adapter.Adapter(D, H); ad.load_state_dict(synth.adapter_state_dict(3, D, H))
clf = adapter.CustomCLIP(ad, *paths, temperature=0.01).cuda().train()
opt = optim.set_optimizer(SimpleNamespace(learning_rate=0.01, momentum=0.9, weight_decay=5e-5), clf)
gen = torch.Generator(device="cuda"); gen.manual_seed(5)
x = torch.randn((T * S, D), device="cuda", generator=gen) * 0.5
z0 = torch.randn((T * S, D), device="cuda", generator=gen)


def torch_sets(z):
    zn = torch.nn.functional.normalize(z, dim=1).view(T, S, D)
    s = torch.bmm(zn[:, A:], zn[:, :1].transpose(1, 2)).squeeze(2) / TAU
    return SCALE * (torch.logsumexp(s, dim=1) - s[:, :P].mean(1)).sum()


def head_only():
    _, _, ws = ops.supcon_sets_fwd(z0, SETS, SCALE, TAU)
    ops.supcon_sets_bwd(z0, SETS, SCALE, TAU, ws)


def head_torch():
    z = z0.detach().requires_grad_()
    torch_sets(z).backward()


def step_one_call():
    clf.sets_step(x, opt, sets=SETS, contrastive=(SCALE, TAU))


def step_autograd():
    loss = clf.sets_loss(x, sets=SETS, contrastive=(SCALE, TAU))[0]
    opt.zero_grad(); loss.backward(); opt.step()


def step_torch():
    loss = torch_sets(clf.adapter(x))
    opt.zero_grad(); loss.backward(); opt.step()


modes = (("head_only", head_only), ("head_torch", head_torch), ("step_one_call", step_one_call), ("step_autograd", step_autograd),
         ("step_torch", step_torch))
for _, fn in modes:
    for _ in range(3):
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
med = {name: statistics.median(times[name]) for name, _ in modes}
for name, _ in modes:
    print(f"T={T} P={P} N={N} D={D} {name}: median {med[name]:.1f} us/step of {repeats} windows x {steps} steps: "
          + " ".join(f"{t:.1f}" for t in times[name]))
nbytes = 12 * T * S * D
rate = nbytes / (med["head_only"] * 1e-6)
print(f"T={T} P={P} N={N} D={D} head_only: {nbytes / 1e6:.1f} MB at {rate / 1e12:.2f} TB/s = {100 * rate / COPY_RATE:.0f} % of the {COPY_RATE / 1e12:.2f} TB/s "
      f"copy rate; head_torch / head_only = {med['head_torch'] / med['head_only']:.2f}")
