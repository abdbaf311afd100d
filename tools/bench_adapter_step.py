"""Developer tool (GPU box): the adapter-only train step (BASELINE configs[0] shape) -- us/step for the fused C step, at a batch.
    python tools/bench_adapter_step.py [B] [D] [steps]          (run under rocprofv3 --kernel-trace --stats for the per-kernel split)
    python tools/bench_adapter_step.py [B] [D] [steps] --robust [repeats]
        the group-DRO step: the ERM one-call step, the robust one-call step and the robust step through the autograd path in one
        process, `repeats` (default 7) alternating windows of `steps` steps each; prints every window and the medians"""
import os, sys, time, json, tempfile
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import dbmm_amd  # noqa
from dbmm_amd import adapter, optim, synth
from types import SimpleNamespace

robust = "--robust" in sys.argv
if robust:
    k = sys.argv.index("--robust")
    repeats = int(sys.argv[k + 1]) if len(sys.argv) > k + 1 else 7
    del sys.argv[k:]
B = int(sys.argv[1]) if len(sys.argv) > 1 else 256
D = int(sys.argv[2]) if len(sys.argv) > 2 else 1024
steps = int(sys.argv[3]) if len(sys.argv) > 3 else 200
d = tempfile.mkdtemp()
paths = []
for nm, C in (("c", 2), ("s", 2), ("g", 4)):
    m = synth.text_matrix(1, D, C, nm); p = os.path.join(d, nm + ".json")
    json.dump({f"{nm}{i}": m[:, i].tolist() for i in range(C)}, open(p, "w")); paths.append(p)
ad = adapter.Adapter(D, 128); ad.load_state_dict(synth.adapter_state_dict(3, D, 128))
clf = adapter.CustomCLIP(ad, *paths, temperature=0.01).cuda().train()
opt = optim.set_optimizer(SimpleNamespace(learning_rate=0.1, momentum=0.9, weight_decay=5e-5), clf)
x = synth.normal(5, f"x{B}", (B, D), 0.5).cuda()
y, c, g = (t.cuda() for t in synth.labels(6, B))
if robust:
    import statistics
    from dbmm_amd import ops
    state = adapter.GroupDRO(4, 0.01, "cuda")

    def erm():
        clf.train_step(x, y, opt)

    def one_call():
        clf.train_step(x, y, opt, robust=(state, g))

    def autograd():
        loss, _, _ = clf.loss(x, y, robust=(state, g))
        opt.zero_grad(); loss.backward(); opt.step()
    modes = (("erm_one_call", erm), ("robust_one_call", one_call), ("robust_autograd", autograd))
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
    print(f"launches: ERM {ops.adapter_step_launches(B, D, 128)}, robust {ops.adapter_step_launches(B, D, 128, robust=True)}; q = {state.q.tolist()}")
    sys.exit(0)
for _ in range(20):
    clf.train_step(x, y, opt)
torch.cuda.synchronize()
t0 = time.perf_counter()
for _ in range(steps):
    loss, logits, rows = clf.train_step(x, y, opt)
torch.cuda.synchronize()
print(f"B={B} D={D}: {(time.perf_counter() - t0) / steps * 1e6:.1f} us/step, loss {loss.item():.5f}")
