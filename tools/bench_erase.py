"""Time linear concept erasure on the fused kernels against the compositions a user writes from torch ops on the same GPU:

  label_column_sums   ops.label_column_sums (two launches, float64 from the first add) against a float64 index_add_ of the rows
                      (sums.index_add_(0, labels, x.double()) plus torch.bincount): that makes a float64 copy of the rows first;
  erase_rows          ops.erase_rows at R = 1, 3 and 15, out of place and in place, against x - ((x - c) @ A.T) @ B;
  erasure_fit         analysis.erasure_fit end to end (column sums, scatter matrix, label sums, the host's eigh and SVD).

Two sizes, D = 1024: Waterbirds-like (4,795 rows) and CelebA-like (162,770 rows).  Medians of 7 alternating windows in one process.
Reported: the time per call, the achieved bytes per second against the 6.29 TB/s copy rate (label sums: one read of the rows; erase:
one read and one write), and the peak extra device memory of both paths.

    python tools/bench_erase.py [--sizes waterbirds,celeba] [--ranks 1,3,15] [--windows 7]
"""
import argparse
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import dbmm_amd  # noqa: E402,F401
from dbmm_amd import analysis, ops  # noqa: E402

SIZES = {"waterbirds": 4795, "celeba": 162770}
D = 1024
G = 4                               # labels of the sums: the groups
COPY_TBS = 6.29                     # the copy rate README.md records


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


def torch_label_sums(x, labels):
    sums = torch.zeros((G, x.shape[1]), dtype=torch.float64, device=x.device)
    sums.index_add_(0, labels, x.double())
    return sums, torch.bincount(labels, minlength=G)


def torch_erase(x, c, A, B):
    return x - ((x - c) @ A.T) @ B


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="waterbirds,celeba")
    ap.add_argument("--ranks", default="1,3,15")
    ap.add_argument("--windows", type=int, default=7)
    a = ap.parse_args()
    med = statistics.median
    for name in a.sizes.split(","):
        n = SIZES[name]
        gen = torch.Generator().manual_seed(11)
        base = 3.0 * torch.randn(1, D, generator=gen)
        shift = torch.randn(G, D, generator=gen) / D ** 0.5                       # a label shifts the rows: far from zero, close together
        labels = torch.randint(0, G, (n,), generator=gen).cuda()
        x = (torch.randn(n, D, generator=gen) / D ** 0.5 + base).cuda() + shift.cuda()[labels]
        c = x.mean(0).contiguous()
        tag = f"{name} N={n} D={D}"
        steps = 50 if n < 20000 else 10
        legs = {"label_sums": (lambda: ops.label_column_sums(x, labels, G), steps),
                "torch_label_sums": (lambda: torch_label_sums(x, labels), steps),
                "erasure_fit": (lambda: analysis.erasure_fit(x, labels), 1)}
        ranks = [int(v) for v in a.ranks.split(",")]
        bases = {}
        for r in ranks:
            A = (torch.randn(r, D, generator=gen) / D ** 0.5).cuda()
            B = (torch.randn(r, D, generator=gen) / D ** 0.5).cuda()
            bases[r] = (A, B)
            target = x.clone()
            legs[f"erase_r{r}"] = (lambda A=A, B=B: ops.erase_rows(x, c, A, B), steps)
            legs[f"erase_r{r}_in_place"] = (lambda A=A, B=B, t=target: ops.erase_rows(t, c, A, B, out=t), steps)
            legs[f"torch_erase_r{r}"] = (lambda A=A, B=B: torch_erase(x, c, A, B), steps)
            diff = (ops.erase_rows(x, c, A, B) - torch_erase(x, c, A, B)).abs().max().item()
            print(f"{tag} R={r}: max |erase_rows - torch composition| {diff:.3e}", flush=True)
        ours, theirs = ops.label_column_sums(x, labels, G), torch_label_sums(x, labels)
        print(f"{tag} label sums: max |ours - index_add_| {(ours[0] - theirs[0]).abs().max().item():.3e}, counts equal {torch.equal(ours[1], theirs[1])}",
              flush=True)
        fit = analysis.erasure_fit(x, labels)                                        # warm-up of the fit's shapes
        print(f"{tag} erasure_fit: rank {fit['rank']}, singular values {fit['singular_values']}", flush=True)
        times = {leg: [] for leg in legs}
        for _ in range(a.windows):                                                   # alternating: one window of every leg per round
            for leg, (fn, st) in legs.items():
                times[leg].append(window(fn, st)[0])
        for leg, (fn, st) in legs.items():
            ts = times[leg]
            print(f"{tag} {leg}: median {med(ts) * 1e3:.3f} ms/call of {a.windows} windows x {st} calls: " + " ".join(f"{t * 1e3:.3f}" for t in ts),
                  flush=True)
        byt = n * D * 4.0
        t = med(times["label_sums"])
        print(f"{tag} label_sums: {byt / 1e6:.1f} MB (one read of the rows) at {byt / t / 1e12:.2f} TB/s = {100 * byt / t / 1e12 / COPY_TBS:.0f} % of the "
              f"{COPY_TBS} TB/s copy rate; torch_label_sums / label_sums = {med(times['torch_label_sums']) / t:.2f}", flush=True)
        for r in ranks:
            t, ti = med(times[f"erase_r{r}"]), med(times[f"erase_r{r}_in_place"])
            print(f"{tag} erase R={r}: {2 * byt / 1e6:.1f} MB (one read, one write) at {2 * byt / t / 1e12:.2f} TB/s = "
                  f"{100 * 2 * byt / t / 1e12 / COPY_TBS:.0f} % of the copy rate (in place {2 * byt / ti / 1e12:.2f} TB/s); "
                  f"torch_erase / erase_rows = {med(times[f'torch_erase_r{r}']) / t:.2f}", flush=True)
        A, B = bases[ranks[-1]]
        target = x.clone()
        mem = {"label_column_sums": peak_extra(lambda: ops.label_column_sums(x, labels, G)),
               "torch label sums": peak_extra(lambda: torch_label_sums(x, labels)),
               f"erase_rows R={ranks[-1]}": peak_extra(lambda: ops.erase_rows(x, c, A, B)),
               f"erase_rows R={ranks[-1]} in place": peak_extra(lambda: ops.erase_rows(target, c, A, B, out=target)),
               f"torch erase R={ranks[-1]}": peak_extra(lambda: torch_erase(x, c, A, B)),
               "erasure_fit": peak_extra(lambda: analysis.erasure_fit(x, labels))}
        print(f"{tag} peak extra device memory (rows {byt / 2**20:.1f} MB): " + ", ".join(f"{k} {v / 2**20:.1f} MB" for k, v in mem.items()), flush=True)
        del x, target


if __name__ == "__main__":
    main()
