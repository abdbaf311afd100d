"""Time the matrix-free RBF kernel product behind analysis.kernel_ridge_fit / kernel_ridge_predict (ops.pairdist_rbf_matvec) against
its neighbours on the same GPU:
  1. itself at C = 1, 4 and 16 dense weight columns: the ratios are the price of a column;
  2. ops.pairdist_rbf_row_group_sums at one bandwidth and four labels, in the same process and rotating with the others: the rows pass
     the product is built on (unchanged code), so product / rows pass is the cost of the weighted epilogue;
  3. itself with one-hot weights (the first CG product) and with weights that are zero past the first quarter of the rows (a
     prediction pass): what skipping the all-zero (tile, column) pairs buys;
  4. what a user had to write before: chunked fp32 torch.cdist -> exp -> matmul with the weights;
then analysis.kernel_ridge_fit and kernel_ridge_predict end to end with their iteration counts, and each path's peak extra device
memory.

Two sizes, D = 1024, 4 labels, rows sorted by label: Waterbirds-like (4,795 rows) and CelebA-like (162,770).  The order of the
contenders rotates with the repeat; medians, with every repeat listed so the spread can be read.  One JSON line per size.

    python tools/bench_kernel_ridge.py [--sizes waterbirds,celeba] [--repeats 5] [--no-fit]
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


def peak_extra(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


def torch_baseline(x, v, gam, chunk=4096):
    """[N, C] WITH the diagonal's ones (K v + v): fp32 cdist in row chunks, exp, a matmul with the weights"""
    out = torch.empty(x.shape[0], v.shape[1], dtype=torch.float32, device=x.device)
    for i in range(0, x.shape[0], chunk):
        out[i:i + chunk] = torch.exp(-gam * torch.cdist(x[i:i + chunk], x) ** 2) @ v
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="waterbirds,celeba")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--no-fit", action="store_true", help="skip the end-to-end fit and predict")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_kernel_ridge needs the GPU: there is nothing to time without it"
    assert a.repeats >= 5, "medians of at least five windows"
    med = statistics.median
    r4 = lambda ts: [round(t, 6) for t in ts]
    for name in a.sizes.split(","):
        counts = SIZES[name]
        n = sum(counts)
        gen = torch.Generator().manual_seed(11)
        groups = np.repeat(np.arange(4), counts)
        x = (0.5 * torch.randn(n, D, generator=gen) + 0.1 * torch.randn(1, D, generator=gen)).cuda()
        x += torch.from_numpy(groups).float().cuda().unsqueeze(1) * 0.05
        gd = torch.from_numpy(groups).cuda()
        center = x.mean(0)
        gam = float(analysis.rbf_gammas(x, (1.0,))[0])
        v16 = torch.randn(n, 16, generator=gen).cuda()
        v = {c: v16[:, :c].contiguous() for c in (1, 4, 16)}
        onehot = (gd.unsqueeze(1) == torch.arange(4, device="cuda").unsqueeze(0)).float().contiguous()
        quarter = v[4].clone()
        quarter[n // 4:] = 0
        small = slice(0, 2048)                                           # warm-up: library load, code objects, allocator
        xs_ = x[small].contiguous()
        ops.pairdist_rbf_row_group_sums(xs_, gd[small].contiguous(), 4, center, [gam])
        ops.pairdist_rbf_matvec(xs_, v[4][small].contiguous(), center, gam)
        torch_baseline(xs_, v[4][small], gam)
        times = {k: [] for k in ("rows", "c1", "c4", "c16", "onehot", "quarter")}

        def runner(key, fn):
            def run():
                t, out = timed(fn)
                times[key].append(t)
                return out
            return key, run

        methods = [runner("rows", lambda: ops.pairdist_rbf_row_group_sums(x, gd, 4, center, [gam])),
                   runner("c1", lambda: ops.pairdist_rbf_matvec(x, v[1], center, gam)),
                   runner("c4", lambda: ops.pairdist_rbf_matvec(x, v[4], center, gam)),
                   runner("c16", lambda: ops.pairdist_rbf_matvec(x, v[16], center, gam)),
                   runner("onehot", lambda: ops.pairdist_rbf_matvec(x, onehot, center, gam)),
                   runner("quarter", lambda: ops.pairdist_rbf_matvec(x, quarter, center, gam))]
        res = {}
        for r in range(a.repeats):                                       # the order rotates with the repeat
            k = r % len(methods)
            for nm, fn in methods[k:] + methods[:k]:
                res[nm] = fn()
        t_base = []
        for _ in range(min(a.repeats, 3)):
            t, base = timed(lambda: torch_baseline(x, v[4], gam))
            t_base.append(t)
        scale = torch_baseline(x, v[4].abs(), gam)
        rel = ((res["c4"] - (base - v[4]).double()).abs() / scale.double()).max().item()
        one_hot_equal = bool(torch.equal(res["onehot"], res["rows"][0]))
        mem = {"matvec_c4": peak_extra(lambda: ops.pairdist_rbf_matvec(x, v[4], center, gam)),
               "matvec_c16": peak_extra(lambda: ops.pairdist_rbf_matvec(x, v[16], center, gam)),
               "rbf_rows_l1": peak_extra(lambda: ops.pairdist_rbf_row_group_sums(x, gd, 4, center, [gam])),
               "torch_c4": peak_extra(lambda: torch_baseline(x, v[4], gam))}
        t = {k: med(ts) for k, ts in times.items()}
        pairs = float(n) * (n - 1)
        line = {"size": name, "rows": n, "dim": D, "repeats": a.repeats, "gamma": float(f"{gam:.6e}"),
                "rbf_rows_l1_g4_s": round(t["rows"], 6), "matvec_c1_s": round(t["c1"], 6), "matvec_c4_s": round(t["c4"], 6),
                "matvec_c16_s": round(t["c16"], 6), "matvec_onehot_c4_s": round(t["onehot"], 6), "matvec_quarter_nonzero_c4_s": round(t["quarter"], 6),
                "c1_over_rows_pass": round(t["c1"] / t["rows"], 3), "c4_over_rows_pass": round(t["c4"] / t["rows"], 3),
                "c16_over_rows_pass": round(t["c16"] / t["rows"], 3), "per_extra_column_of_c1": round((t["c16"] / t["c1"] - 1.0) / 15.0, 4),
                "torch_cdist_exp_matmul_c4_s": round(med(t_base), 6), "torch_over_matvec_c4": round(med(t_base) / t["c4"], 2),
                "matvec_c4_fp16_tflops": round(pairs * 2 * 3 * D / t["c4"] / 1e12, 1),
                "max_diff_vs_torch_fp32_over_sum_k_abs_v": float(f"{rel:.3e}"), "onehot_bits_equal_rows_pass": one_hot_equal,
                "peak_extra_mb": {k: round(val / 2 ** 20, 1) for k, val in mem.items()},
                "all_s": {k: r4(ts) for k, ts in times.items()}, "all_torch_s": r4(t_base)}
        if not a.no_fit:
            q = x[: max(n // 8, 1)].contiguous()                         # a query set an eighth of the split
            t_fit, fit = timed(lambda: analysis.kernel_ridge_fit(x, groups, scales=(1.0,)))
            t_pred, _ = timed(lambda: analysis.kernel_ridge_predict(fit, q))
            line.update(fit_1_bandwidth_2_ridges_s=round(t_fit, 6), fit_iterations=fit["iterations"].tolist(),
                        fit_converged=bool(fit["converged"].all()), fit_worst_residual=float(f"{fit['residual'].max():.3e}"),
                        predict_eighth_s=round(t_pred, 6),
                        fit_peak_extra_mb=round(peak_extra(lambda: analysis.kernel_ridge_fit(x, groups, scales=(1.0,), max_iter=2)) / 2 ** 20, 1))
        print(json.dumps(line), flush=True)
        del x, base, scale, res, v16, v


if __name__ == "__main__":
    main()
