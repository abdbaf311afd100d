"""Developer tool (GPU box): what per-row loss weights cost a training step -- us/step, in ONE process, medians of alternating windows.
    python tools/bench_weighted_step.py [steps] [repeats]        (defaults 200 steps x 7 windows)
Adapter step at D = 1024, H = 128, batch 256 and 1024, and the linear probe at D = 1024, C = 2, batch 128, each in four forms:
    erm_one_call        classifier.train_step(x, y, opt)
    weighted_one_call   classifier.train_step(x, y, opt, row_weights=w)
    weighted_autograd   loss(..., row_weights=w) / the module's forward, backward, optimizer.step()
    weighted_torch      the same loss composed from torch ops: (w * cross_entropy(forward(x), y, reduction="none")).mean()
and one replica-batched adapter step and linear step at R = 8, batch 256 / 128, unweighted against weighted ([R, N] weights).
Prints every window, the medians, the windows' spread (max - min over the median) and the weighted / ERM ratio."""
import json
import os
import statistics
import sys
import tempfile
import time
from types import SimpleNamespace

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn.functional as F
import dbmm_amd  # noqa
from dbmm_amd import adapter, optim, synth

steps = int(sys.argv[1]) if len(sys.argv) > 1 else 200
repeats = int(sys.argv[2]) if len(sys.argv) > 2 else 7
D, H = 1024, 128
NS = SimpleNamespace(learning_rate=0.01, momentum=0.9, weight_decay=5e-5)


def weights(n):
    w = torch.ones(n, dtype=torch.float64)
    w[1::5] = 0.0
    w[3::17] = 5.0
    return (w * n / w.sum()).float().cuda()


def windows(title, modes):
    for _, fn in modes:
        for _ in range(20):
            fn()
    times = {name: [] for name, _ in modes}
    for _ in range(repeats):
        for name, fn in modes:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                fn()
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) / steps * 1e6)
    med = {name: statistics.median(t) for name, t in times.items()}
    base = med[modes[0][0]]
    for name, _ in modes:
        t = times[name]
        print(f"{title} {name}: median {med[name]:.1f} us/step ({med[name] / base:.3f} x {modes[0][0]}), spread {(max(t) - min(t)) / med[name] * 100:.1f}% "
              f"of {repeats} windows x {steps} steps: " + " ".join(f"{v:.1f}" for v in t), flush=True)


d = tempfile.mkdtemp()
paths = []
for nm, C in (("c", 2), ("s", 2), ("g", 4)):
    m = synth.text_matrix(1, D, C, nm); p = os.path.join(d, nm + ".json")
    json.dump({f"{nm}{i}": m[:, i].tolist() for i in range(C)}, open(p, "w")); paths.append(p)

for B in (256, 1024):
    ad = adapter.Adapter(D, H); ad.load_state_dict(synth.adapter_state_dict(3, D, H))
    clf = adapter.CustomCLIP(ad, *paths, temperature=0.01).cuda().train()
    opt = optim.set_optimizer(NS, clf)
    x = synth.normal(5, f"x{B}", (B, D), 0.5).cuda()
    y = synth.labels(6, B)[0].cuda()
    w = weights(B)

    def autograd():
        loss, _, _ = clf.loss(x, y, row_weights=w)
        opt.zero_grad(); loss.backward(); opt.step()

    def composed():
        loss = (w * F.cross_entropy(clf(x), y, reduction="none")).mean()
        opt.zero_grad(); loss.backward(); opt.step()
    windows(f"adapter B={B} D={D}", (("erm_one_call", lambda: clf.train_step(x, y, opt)),
                                     ("weighted_one_call", lambda: clf.train_step(x, y, opt, row_weights=w)),
                                     ("weighted_autograd", autograd), ("weighted_torch", composed)))

B = 128
lin = adapter.LinearClassifier(D, 2).cuda().train()
lopt = optim.set_optimizer(NS, lin)
x = synth.normal(5, f"lx{B}", (B, D), 0.5).cuda()
y = synth.labels(6, B)[0].cuda()
w = weights(B)


def lin_composed():
    loss = (w * F.cross_entropy(lin(x), y, reduction="none")).mean()
    lopt.zero_grad(); loss.backward(); lopt.step()


# (the linear probe has no fused weighted loss on the autograd path: its autograd form IS the composition from torch ops)
windows(f"linear B={B} D={D}", (("erm_one_call", lambda: lin.train_step(x, y, lopt)),
                                ("weighted_one_call", lambda: lin.train_step(x, y, lopt, row_weights=w)),
                                ("weighted_torch", lin_composed)))

R, N = 8, 4096
table = synth.normal(7, "table", (N, D), 0.5).cuda()
labels = synth.labels(8, N)[0].cuda()
groups = synth.labels(8, N)[2].cuda()
wtab = torch.stack([weights(N).roll(r) for r in range(R)]).contiguous()
for kind, B in (("adapter", 256), ("linear", 128)):
    idx = torch.stack([torch.randperm(N, generator=torch.Generator().manual_seed(r))[:B] for r in range(R)]).cuda()
    counts = torch.zeros((R, 4, 2), dtype=torch.int64, device="cuda")
    loss_sum = torch.zeros((R,), dtype=torch.float64, device="cuda")
    if kind == "adapter":
        mods = [adapter.CustomCLIP(adapter.Adapter(D, H), *paths, temperature=0.01) for _ in range(R)]
        sweep = adapter.SweepAdapters.from_modules(mods, "cuda")
        step = lambda **k: sweep.step(table, idx, labels, groups, "class", [0.01] * R, 0.9, 5e-5, counts, loss_sum, **k)
    else:
        sweep = adapter.SweepLinear.from_modules([adapter.LinearClassifier(D, 2) for _ in range(R)], "cuda")
        step = lambda **k: sweep.step(table, idx, labels, groups, [0.01] * R, 0.9, 5e-5, counts, loss_sum, **k)
    windows(f"{kind} sweep R={R} B={B} D={D}", (("erm_sweep_step", lambda: step()), ("weighted_sweep_step", lambda: step(row_weights=wtab))))
