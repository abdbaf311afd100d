"""Time the RBF row sums behind analysis.kernel_probe / mmd_witness / kernel_alignment (ops.pairdist_rbf_row_group_sums) against their
neighbours on the same GPU:
  1. itself at L = 1 and L = 4: the ratio is the price of a bandwidth;
  2. ops.pairdist_row_group_sums, the same tile kernel with the square root for the exponential: L = 1 over it is exp against sqrt;
  3. the distance rows entry of a library built from the PARENT commit (--parent-lib), in the same process and rotating with the
     others: templating the tile kernel must leave the distance instantiation's bits alone and its time within the spread of its
     own repeats;
  4. what a user had to write before: chunked fp32 torch.cdist -> exp -> one-hot matmul, once per bandwidth;
then analysis.kernel_probe and analysis.kernel_alignment end to end, and each path's peak extra device memory.

Two sizes, D = 1024, 4 labels, rows sorted by label as the analysis functions pass them: Waterbirds-like (4,795 rows) and CelebA-like
(162,770).  The order of the contenders rotates with the repeat; medians, with every repeat listed so the spread can be read.  One
JSON line per size.

    python tools/bench_kernel_probe.py [--sizes waterbirds,celeba] [--repeats 5] [--parent-lib PATH]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import dbmm_amd  # noqa: E402,F401
from dbmm_amd import _lib, analysis, ops  # noqa: E402

SIZES = {"waterbirds": (3498, 184, 56, 1057), "celeba": (71629, 66874, 22880, 1387)}
D = 1024
SCALES4 = (0.25, 1.0, 4.0, 16.0)


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


def torch_baseline(x, onehot, gam, chunk=4096):
    """[N, G] row sums WITH the diagonal's ones: fp32 cdist in row chunks, exp, a one-hot product, one pass over the pairs per
    bandwidth, as a user without the fused kernel would write it"""
    out = torch.empty(x.shape[0], onehot.shape[1], dtype=torch.float32, device=x.device)
    for i in range(0, x.shape[0], chunk):
        out[i:i + chunk] = torch.exp(-gam * torch.cdist(x[i:i + chunk], x) ** 2) @ onehot
    return out


def parent_distance_rows_entry(path):
    """dbmm_pairdist_row_group_sums and its workspace size from another build of the library (the parent commit's)"""
    L = ctypes.CDLL(path)
    L.dbmm_workspace_bytes_pairdist_rows.argtypes = _lib._SIGS["dbmm_workspace_bytes_pairdist_rows"]
    L.dbmm_workspace_bytes_pairdist_rows.restype = ctypes.c_size_t
    L.dbmm_pairdist_row_group_sums.argtypes = _lib._SIGS["dbmm_pairdist_row_group_sums"]

    def call(x, g, G, center):
        n, d = x.shape
        nbytes = L.dbmm_workspace_bytes_pairdist_rows(n, d, G)
        ws = torch.empty((nbytes + 3) // 4, device=x.device, dtype=torch.float32)
        out = torch.empty((n, G), device=x.device, dtype=torch.float64)
        rc = L.dbmm_pairdist_row_group_sums(x.data_ptr(), g.data_ptr(), center.data_ptr(), out.data_ptr(), n, d, G, ws.data_ptr(), ws.numel() * 4,
                                            _lib.stream())
        assert rc == 0, rc
        return out
    return call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="waterbirds,celeba")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--parent-lib", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_kernel_probe needs the GPU: there is nothing to time without it"
    assert a.repeats >= 5, "medians of at least five windows"
    parent = parent_distance_rows_entry(a.parent_lib) if a.parent_lib else None
    med = statistics.median
    r4 = lambda ts: [round(t, 6) for t in ts]
    for name in a.sizes.split(","):
        counts = SIZES[name]
        n = sum(counts)
        gen = torch.Generator().manual_seed(11)
        groups = np.repeat(np.arange(4), counts)                         # sorted by label: what the analysis functions hand the kernel
        x = (0.5 * torch.randn(n, D, generator=gen) + 0.1 * torch.randn(1, D, generator=gen)).cuda()
        x += torch.from_numpy(groups).float().cuda().unsqueeze(1) * 0.05
        gd = torch.from_numpy(groups).cuda()
        center = x.mean(0)
        onehot = (gd.unsqueeze(1) == torch.arange(4, device="cuda").unsqueeze(0)).float()          # [N, G]
        gammas = analysis.rbf_gammas(x, SCALES4).tolist()
        g1 = gammas[1:2]
        small = slice(0, 2048)                                           # warm-up: library load, code objects, allocator
        xs_, gs_ = x[small].contiguous(), gd[small].contiguous()
        ops.pairdist_rbf_row_group_sums(xs_, gs_, 4, center, gammas)
        ops.pairdist_row_group_sums(xs_, gs_, 4, center)
        if parent:
            parent(xs_, gs_, 4, center)
        torch_baseline(xs_, onehot[small], g1[0])
        times = {"l1": [], "l4": [], "dist": [], "parent": []}

        def runner(key, fn):
            def run():
                t, out = timed(fn)
                times[key].append(t)
                return out
            return key, run

        methods = [runner("l1", lambda: ops.pairdist_rbf_row_group_sums(x, gd, 4, center, g1)),
                   runner("l4", lambda: ops.pairdist_rbf_row_group_sums(x, gd, 4, center, gammas)),
                   runner("dist", lambda: ops.pairdist_row_group_sums(x, gd, 4, center))]
        if parent:
            methods.append(runner("parent", lambda: parent(x, gd, 4, center)))
        # the order rotates with the repeat, so that no method always follows the same neighbour
        res = {}
        for r in range(a.repeats):
            k = r % len(methods)
            for nm, fn in methods[k:] + methods[:k]:
                res[nm] = fn()
        R1, R4, Rd, Rp = res["l1"], res["l4"], res["dist"], res.get("parent")
        t_base = []
        for _ in range(min(a.repeats, 3)):
            t, base = timed(lambda: torch_baseline(x, onehot, g1[0]))
            t_base.append(t)
        own = torch.zeros_like(base)
        own[torch.arange(n, device="cuda"), gd] = 1.0                    # the baseline counts k(x, x) = 1 in the row's own label
        rel = ((R1[0] - (base - own).double()).abs() / R1[0]).max().item()
        assert torch.equal(R1[0], R4[1]), "a bandwidth's sums depend on the others in the call"
        mem = {"rbf_rows_l4": peak_extra(lambda: ops.pairdist_rbf_row_group_sums(x, gd, 4, center, gammas)),
               "rbf_rows_l1": peak_extra(lambda: ops.pairdist_rbf_row_group_sums(x, gd, 4, center, g1)),
               "distance_rows": peak_extra(lambda: ops.pairdist_row_group_sums(x, gd, 4, center)),
               "torch_per_bandwidth": peak_extra(lambda: torch_baseline(x, onehot, g1[0]))}
        t_probe = [timed(lambda: analysis.kernel_probe(x, groups))[0] for _ in range(min(a.repeats, 3))]
        t_align = [timed(lambda: analysis.kernel_alignment(x, groups))[0] for _ in range(min(a.repeats, 3))]
        probe, align = analysis.kernel_probe(x, groups), analysis.kernel_alignment(x, groups)
        pairs = float(n) * (n - 1)                                       # the rows kernel walks the full square
        t1, t4, td = med(times["l1"]), med(times["l4"]), med(times["dist"])
        line = {"size": name, "rows": n, "dim": D, "repeats": a.repeats,
                "rbf_rows_l1_s": round(t1, 6), "rbf_rows_l4_s": round(t4, 6), "distance_rows_s": round(td, 6),
                "l4_over_l1": round(t4 / t1, 3), "per_extra_bandwidth": round((t4 / t1 - 1.0) / 3.0, 4), "l1_over_distance": round(t1 / td, 3),
                "torch_cdist_exp_onehot_per_bandwidth_s": round(med(t_base), 6), "torch_x4_over_rbf_rows_l4": round(4 * med(t_base) / t4, 2),
                "rbf_rows_l1_fp16_tflops": round(pairs * 2 * 3 * D / t1 / 1e12, 1),
                "max_rel_diff_vs_torch_fp32": float(f"{rel:.3e}"),
                "peak_extra_mb": {k: round(v / 2 ** 20, 1) for k, v in mem.items()},
                "kernel_probe_3_bandwidths_end_to_end_s": round(med(t_probe), 6), "kernel_alignment_3_bandwidths_end_to_end_s": round(med(t_align), 6),
                "probe_balanced_accuracy": [round(float(v), 4) for v in probe["balanced_accuracy"]],
                "alignment": [float(f"{v:.4e}") for v in align["alignment"]], "alignment_rel_bound": [float(f"{v:.3e}") for v in align["rel_bound"]],
                "all_rbf_rows_l1_s": r4(times["l1"]), "all_rbf_rows_l4_s": r4(times["l4"]), "all_distance_rows_s": r4(times["dist"]),
                "all_torch_s": r4(t_base), "all_kernel_probe_s": r4(t_probe), "all_kernel_alignment_s": r4(t_align)}
        if parent:
            tp = med(times["parent"])
            spread = (max(times["dist"]) - min(times["dist"])) / td
            line.update(distance_rows_parent_s=round(tp, 6), all_distance_rows_parent_s=r4(times["parent"]),
                        distance_rows_over_parent=round(td / tp, 4), distance_rows_own_spread=round(spread, 4),
                        distance_rows_bits_equal_parent=bool(torch.equal(Rd, Rp)))
        print(json.dumps(line), flush=True)
        del x, base, own, R1, R4, Rd, Rp, res


if __name__ == "__main__":
    main()
