"""Time the group-wise distance statistics (analysis.group_stats on the fused pairwise-distance kernel) against what a user had to
write before it existed: chunked torch.cdist in fp32 on the same GPU, summed, once for the whole split and once per group.

Two sizes, D = 1024: Waterbirds-like (4,795 rows in groups of 3,498 / 184 / 56 / 1,057) and CelebA-like (162,770 rows in groups of
71,629 / 66,874 / 22,880 / 1,387).  Three repeats, alternating the two methods; medians.  One JSON line per size.

    python tools/bench_group_stats.py [--sizes waterbirds,celeba] [--repeats 3]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import dbmm_amd  # noqa: E402,F401
from dbmm_amd import analysis, ops  # noqa: E402

SIZES = {"waterbirds": (3498, 184, 56, 1057), "celeba": (71629, 66874, 22880, 1387)}
D = 1024


def timed(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t, out


def cdist_baseline(x, groups, chunk=4096):
    """mean pairwise distance of the whole split and of every group: torch.cdist fp32 in row chunks, summed in float64"""
    def mean_dist(rows):
        n = rows.shape[0]
        tot = torch.zeros((), dtype=torch.float64, device=rows.device)
        for i in range(0, n, chunk):
            tot += torch.cdist(rows[i:i + chunk], rows).sum(dtype=torch.float64)
        return (tot / (n * (n - 1.0))).item()
    out = {"full": mean_dist(x)}
    for g in np.unique(groups):
        out[int(g)] = mean_dist(x[torch.from_numpy(np.where(groups == g)[0]).to(x.device)])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="waterbirds,celeba")
    ap.add_argument("--repeats", type=int, default=3)
    a = ap.parse_args()
    for name in a.sizes.split(","):
        counts = SIZES[name]
        n = sum(counts)
        gen = torch.Generator().manual_seed(11)
        groups = np.repeat(np.arange(4), counts)[torch.randperm(n, generator=gen).numpy()]
        x = (0.5 * torch.randn(n, D, generator=gen) + 0.1 * torch.randn(1, D, generator=gen)).cuda()
        x += torch.from_numpy(groups).float().cuda().unsqueeze(1) * 0.05
        gd = torch.from_numpy(groups).cuda()
        center = x.mean(0)
        analysis.group_stats(x[:2048], groups[:2048])                # warm-up: library load, allocator
        torch.cdist(x[:2048], x[:2048]).sum()
        t_ours, t_kernel, t_base = [], [], []
        for _ in range(a.repeats):
            t, st = timed(lambda: analysis.group_stats(x, groups))
            t_ours.append(t)
            t_kernel.append(timed(lambda: ops.pairdist_group_sums(x, gd, 4, center))[0])
            t, base = timed(lambda: cdist_baseline(x, groups))
            t_base.append(t)
        rel = max(abs(st["pairwise_distance"][k] / base[k] - 1) for k in base)
        pairs = n * (n - 1) / 2
        med = statistics.median
        print(json.dumps({"size": name, "rows": n, "dim": D, "group_stats_s": round(med(t_ours), 4), "kernel_only_unsorted_s": round(med(t_kernel), 4),
                          "cdist_fp32_baseline_s": round(med(t_base), 4), "speedup": round(med(t_base) / med(t_ours), 2),
                          "kernel_fp16_tflops": round(pairs * 2 * 3 * D / med(t_kernel) / 1e12, 1),
                          "max_rel_diff_vs_baseline": float(f"{rel:.3e}"), "repeats": a.repeats,
                          "all_group_stats_s": [round(t, 4) for t in t_ours], "all_baseline_s": [round(t, 4) for t in t_base]}), flush=True)
        del x


if __name__ == "__main__":
    main()
