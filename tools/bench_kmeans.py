"""Time Lloyd's k-means on the fused kernels (ops.kmeans_fit: assign + sums + merge per iteration) against the composition a user
writes from torch ops on the same GPU: chunked torch.cdist + argmin + index_add_ (+ bincount), one host sync per iteration for the
stopping test.

Two sizes, D = 1024: Waterbirds-like (4,795 rows) and CelebA-like (162,770 rows); k = 2 and k = 8.  Medians of 7 alternating windows
in one process.  Reported: one Lloyd iteration from a fixed start (ours: dbmm_kmeans_begin + one dbmm_kmeans_iterate, four launches;
the first iteration, in which every label changes), the assignment kernel alone (ops.kmeans_assign), a whole fit from the same fixed
start under the same cap on the iterations (with the iterations both took), the peak extra device memory of both fits, and the HBM
rate of the iteration: 2 N D 4 bytes over its time against the 6.29 TB/s copy rate.

    python tools/bench_kmeans.py [--sizes waterbirds,celeba] [--ks 2,8] [--windows 7] [--max-iter 30]
"""
import argparse
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import dbmm_amd  # noqa: E402,F401
from dbmm_amd import _lib, ops  # noqa: E402

SIZES = {"waterbirds": 4795, "celeba": 162770}
D = 1024
PLANTED = 8                         # planted clusters of the rows, whatever k is fitted
COPY_TBS = 6.29                     # the copy rate README.md records
CHUNK = 16384                       # rows per cdist of the torch composition: a [CHUNK, k] distance block at a time


def window(fn, steps):
    """seconds per call over `steps` calls ending in a device synchronise"""
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(steps):
        out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) / steps, out


def peak_extra(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    out = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    del out
    return peak


def torch_iteration(x, centers):
    """one Lloyd iteration of the composition -> (new centres, labels); an empty cluster keeps its centre"""
    k = centers.shape[0]
    sums = torch.zeros_like(centers)
    counts = torch.zeros(k, dtype=torch.int64, device=x.device)
    labels = torch.empty(x.shape[0], dtype=torch.int64, device=x.device)
    for i in range(0, x.shape[0], CHUNK):
        rows = x[i:i + CHUNK]
        lab = torch.cdist(rows, centers).argmin(1)
        labels[i:i + CHUNK] = lab
        sums.index_add_(0, lab, rows)
        counts += torch.bincount(lab, minlength=k)
    return torch.where((counts > 0).unsqueeze(1), sums / counts.clamp(min=1).unsqueeze(1), centers), labels


def torch_fit(x, start, max_iter):
    centers, labels, it = start, None, 0
    while it < max_iter:
        new, lab = torch_iteration(x, centers)
        it += 1
        if labels is not None and torch.equal(lab, labels):                     # (a host sync per iteration)
            break
        centers, labels = new, lab
    return centers, labels, it


def one_iteration(x, start, ws):
    """dbmm_kmeans_begin + one iteration on a workspace that is reused: the four launches, no allocation, no status read"""
    L, (n, d), k = _lib.lib(), x.shape, start.shape[0]
    _lib.check(L.dbmm_kmeans_begin(start.data_ptr(), n, d, k, ws.data_ptr(), ws.numel(), _lib.stream()), "kmeans_begin")
    _lib.check(L.dbmm_kmeans_iterate(x.data_ptr(), n, d, k, 1, ws.data_ptr(), ws.numel(), _lib.stream()), "kmeans_iterate")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="waterbirds,celeba")
    ap.add_argument("--ks", default="2,8")
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--max-iter", type=int, default=30)
    a = ap.parse_args()
    med = statistics.median
    for name in a.sizes.split(","):
        n = SIZES[name]
        gen = torch.Generator().manual_seed(11)
        base = 3.0 * torch.randn(1, D, generator=gen)
        cent = torch.randn(PLANTED, D, generator=gen) / D ** 0.5                # separation 1: overlapping clusters, far from zero
        x = (torch.randn(n, D, generator=gen) / D ** 0.5 + base).cuda()
        x += cent.cuda()[torch.randint(0, PLANTED, (n,), generator=gen).cuda()]
        for k in (int(v) for v in a.ks.split(",")):
            start = x[torch.randperm(n, generator=gen)[:k].cuda()].contiguous()  # a fixed start: k rows
            ws = torch.empty(_lib.lib().dbmm_workspace_bytes_kmeans(n, D, k), dtype=torch.uint8, device="cuda")
            centers, labels, info = ops.kmeans_fit(x, start, max_iter=a.max_iter)          # warm-up of every shape timed below
            tc, tl, tit = torch_fit(x, start, a.max_iter)
            one_iteration(x, start, ws)
            same = (labels.long() == tl).float().mean().item()
            tag = f"{name} N={n} D={D} k={k}"
            print(f"{tag} fit: ours {info['iterations']} iterations (converged {info['converged']}, inertia {info['inertia']:.6g}), torch composition "
                  f"{tit} iterations; {100 * same:.3f} % of the labels agree; max |centre difference| {(centers - tc).abs().max().item():.3e}", flush=True)
            steps = 50 if n < 20000 else 10
            legs = {
                "iteration": (lambda: one_iteration(x, start, ws), steps),
                "torch_iteration": (lambda: torch_iteration(x, start), steps),
                "assign_kernel": (lambda: ops.kmeans_assign(x, start), steps),
                "fit": (lambda: ops.kmeans_fit(x, start, max_iter=a.max_iter), 1),
                "torch_fit": (lambda: torch_fit(x, start, a.max_iter), 1),
            }
            times = {leg: [] for leg in legs}
            for _ in range(a.windows):                                           # alternating: one window of every leg per round
                for leg, (fn, st) in legs.items():
                    times[leg].append(window(fn, st)[0])
            for leg, (fn, st) in legs.items():
                ts = times[leg]
                print(f"{tag} {leg}: median {med(ts) * 1e3:.3f} ms/call of {a.windows} windows x {st} calls: " + " ".join(f"{t * 1e3:.3f}" for t in ts),
                      flush=True)
            t_it, t_as = med(times["iteration"]), med(times["assign_kernel"])
            byt = 2.0 * n * D * 4
            print(f"{tag} iteration: {byt / 1e6:.1f} MB (two reads of the rows) at {byt / t_it / 1e12:.2f} TB/s = {100 * byt / t_it / 1e12 / COPY_TBS:.0f} % of the "
                  f"{COPY_TBS} TB/s copy rate; the assignment alone reads {byt / 2e6:.1f} MB at {byt / 2 / t_as / 1e12:.2f} TB/s; "
                  f"torch_iteration / iteration = {med(times['torch_iteration']) / t_it:.2f}", flush=True)
            print(f"{tag} fit: torch_fit / fit = {med(times['torch_fit']) / med(times['fit']):.2f} ({tit} against {info['iterations']} iterations)", flush=True)
            m_ours = peak_extra(lambda: ops.kmeans_fit(x, start, max_iter=a.max_iter))
            m_torch = peak_extra(lambda: torch_fit(x, start, a.max_iter))
            print(f"{tag} peak extra device memory: kmeans_fit {m_ours / 2**20:.1f} MB, torch composition {m_torch / 2**20:.1f} MB, rows {n * D * 4 / 2**20:.1f} MB",
                  flush=True)
            del ws
        del x


if __name__ == "__main__":
    main()
