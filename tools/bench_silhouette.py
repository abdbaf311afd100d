"""Time the per-row, per-group distance sums behind analysis.silhouette (ops.pairdist_row_group_sums) against two comparisons on the
same GPU and the same label-sorted rows:
  1. what a user had to write before it existed: torch.cdist in fp32 over row chunks, times a one-hot matrix, summed in float64;
  2. its sibling ops.pairdist_group_sums, which walks the upper triangle only and reduces into (group, group) buckets: the rows
     kernel does 2 nb / (nb + 1) times its tile work (nb = row blocks of 256) plus a heavier epilogue.

Two sizes, D = 1024: Waterbirds-like (4,795 rows) and CelebA-like (162,770 rows), each with 2, 4 and 16 labels.  Medians of seven
windows in one process, the methods alternating inside every window; peak extra device memory of one call of each.  One JSON line
per (size, labels).

    python tools/bench_silhouette.py [--sizes waterbirds,celeba] [--labels 2,4,16] [--windows 7]
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


def label_counts(counts, G):
    """the split's four group sizes as 2 labels (the classes), 4 (the groups) or 16 (every group in four parts)"""
    if G == 2:
        return [counts[0] + counts[1], counts[2] + counts[3]]
    if G == 4:
        return list(counts)
    return [c // 4 + (1 if q < c % 4 else 0) for c in counts for q in range(4)]


def timed(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t, out


def peak_extra(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    out = fn()
    torch.cuda.synchronize()
    extra = torch.cuda.max_memory_allocated() - base
    del out
    return extra


def cdist_onehot(x, onehot, chunk=4096):
    """R [N, G]: torch.cdist fp32 in row chunks times the one-hot matrix, in float64 (cdist's own zero diagonal adds nothing)"""
    return torch.cat([torch.cdist(x[i:i + chunk], x).double() @ onehot for i in range(0, x.shape[0], chunk)])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="waterbirds,celeba")
    ap.add_argument("--labels", default="2,4,16")
    ap.add_argument("--windows", type=int, default=7)
    a = ap.parse_args()
    med = statistics.median
    for name in a.sizes.split(","):
        n = sum(SIZES[name])
        gen = torch.Generator().manual_seed(11)
        x = (0.5 * torch.randn(n, D, generator=gen) + 0.1 * torch.randn(1, D, generator=gen)).cuda()
        for G in (int(v) for v in a.labels.split(",")):
            labels = np.repeat(np.arange(G), label_counts(SIZES[name], G))                    # sorted, as analysis.silhouette hands them over
            gd = torch.from_numpy(labels).cuda()
            xs = (x + gd.float().unsqueeze(1) * 0.05).contiguous()
            center = xs.mean(0)
            onehot = (gd.unsqueeze(1) == torch.arange(G, device="cuda").unsqueeze(0)).double()
            g8 = (gd // 2).contiguous() if G > 8 else gd                                        # the bucket kernel takes 8 groups at most
            G8 = min(G, 8)
            ops.pairdist_row_group_sums(xs[:2048].contiguous(), gd[:2048].contiguous(), G, center)   # warm-up: library load, allocator
            ops.pairdist_group_sums(xs[:2048].contiguous(), g8[:2048].contiguous(), G8, center)
            cdist_onehot(xs[:2048], onehot[:2048])
            t_rows, t_sil, t_torch, t_bucket = [], [], [], []
            for _ in range(a.windows):
                t, R = timed(lambda: ops.pairdist_row_group_sums(xs, gd, G, center))
                t_rows.append(t)
                t, ref = timed(lambda: cdist_onehot(xs, onehot))
                t_torch.append(t)
                t_bucket.append(timed(lambda: ops.pairdist_group_sums(xs, g8, G8, center))[0])
                t_sil.append(timed(lambda: analysis.silhouette(xs, labels))[0])        # with the sort, the gather and the host step
            rel = ((R - ref).abs() / ref.clamp_min(1e-30)).where(ref > 0, torch.zeros_like(ref)).max().item()
            del R, ref
            mem_rows = peak_extra(lambda: ops.pairdist_row_group_sums(xs, gd, G, center))
            mem_torch = peak_extra(lambda: cdist_onehot(xs, onehot))
            mem_bucket = peak_extra(lambda: ops.pairdist_group_sums(xs, g8, G8, center))
            nb = (n + 255) // 256
            print(json.dumps({"size": name, "rows": n, "dim": D, "labels": G,
                              "rows_kernel_s": round(med(t_rows), 6), "silhouette_end_to_end_s": round(med(t_sil), 6),
                              "torch_cdist_onehot_s": round(med(t_torch), 6), "bucket_kernel_s": round(med(t_bucket), 6),
                              "speedup_vs_torch": round(med(t_torch) / med(t_rows), 2),
                              "ratio_to_bucket_kernel": round(med(t_rows) / med(t_bucket), 2), "tile_ratio": round(2 * nb / (nb + 1), 3),
                              "rows_kernel_fp16_tflops": round(nb * nb * 256.0 * 256.0 * 2 * 3 * D / med(t_rows) / 1e12, 1),
                              "peak_extra_mb": {"rows_kernel": round(mem_rows / 2**20, 1), "torch": round(mem_torch / 2**20, 1),
                                                "bucket_kernel": round(mem_bucket / 2**20, 1)},
                              "max_rel_diff_vs_torch": float(f"{rel:.3e}"), "windows": a.windows,
                              "all_rows_kernel_s": [round(t, 6) for t in t_rows], "all_torch_s": [round(t, 6) for t in t_torch],
                              "all_bucket_kernel_s": [round(t, 6) for t in t_bucket]}), flush=True)
            del xs, onehot
        del x


if __name__ == "__main__":
    main()
