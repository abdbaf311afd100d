"""Developer tool (GPU box): the linear-probe training step -- us per step of the fused LinearClassifier.train_step (csrc/linear_step.hip)
against the autograd path (`logits = clf(x); F.cross_entropy; loss.backward(); optimizer.step()`), timed with HIP events on one stream.

    python tools/bench_linear_step.py [B[,B...]] [D] [iters]          default: 128,256,1024,8192  1024  300
    python tools/bench_linear_step.py --paths [B[,B...]] [D] [iters]  the fused step with the one-launch and the two-launch reduction
                                                                      forced in turn (where the option linear_step_one_launch_max_b belongs)
Run under `rocprofv3 --kernel-trace --stats -- python ...` for the launches per step."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

import dbmm_amd  # noqa: E402,F401
from dbmm_amd import adapter, ops, optim  # noqa: E402

args = [a for a in sys.argv[1:] if not a.startswith("--")]
paths = "--paths" in sys.argv
Bs = [int(b) for b in (args[0] if args else "128,256,1024,8192").split(",")]
D = int(args[1]) if len(args) > 1 else 1024
iters = int(args[2]) if len(args) > 2 else 300
C = 2


def timed(fn, n):
    for _ in range(20):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / n


for B in Bs:
    g = torch.Generator().manual_seed(B)
    x = (torch.randn(B, D, generator=g) * 0.5).cuda()
    y = torch.randint(0, C, (B,), generator=g).cuda()
    torch.manual_seed(0)
    clf = adapter.LinearClassifier(D, C).cuda().train()
    opt = optim.SGD(clf.parameters(), lr=1e-3, momentum=0.9, weight_decay=5e-5)

    def fused():
        clf.train_step(x, y, opt)

    def autograd():
        loss = F.cross_entropy(clf(x), y)
        opt.zero_grad()
        loss.backward()
        opt.step()

    if paths:
        old = ops.get_option("linear_step_one_launch_max_b")
        ops.set_option("linear_step_one_launch_max_b", 1 << 30)
        one = timed(fused, iters)
        ops.set_option("linear_step_one_launch_max_b", 0)
        two = timed(fused, iters)
        ops.set_option("linear_step_one_launch_max_b", old)
        print(f"B={B:5d} D={D}: one launch {one:7.2f} us/step   two launches {two:7.2f} us/step", flush=True)
    else:
        f, a = timed(fused, iters), timed(autograd, iters)
        print(f"B={B:5d} D={D} C={C}: fused {f:7.2f} us/step   autograd {a:7.2f} us/step   speedup {a / f:5.2f}x", flush=True)
