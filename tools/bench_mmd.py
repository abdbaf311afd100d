"""Time the RBF bucket sums behind analysis.mmd (ops.pairdist_rbf_group_sums) against its neighbours on the same GPU:
  1. itself at L = 1 and L = 4: the ratio is the price of a bandwidth;
  2. ops.pairdist_group_sums, the same tile kernel with the square root for the exponential: L = 1 over it is exp against sqrt;
  3. the distance entry of a library built from the PARENT commit (--parent-lib), in the same process and alternating with 2:
     templating the tile kernel must leave the distance kernel within the spread of its own repeats;
  4. what a user had to write before: chunked fp32 torch.cdist -> exp -> one-hot matmul, once per bandwidth;
then analysis.mmd end to end and mmd_permutation_test at n_perm = 20, and each path's peak extra device memory.

Two sizes, D = 1024, 4 groups, rows sorted by group as analysis.mmd passes them: Waterbirds-like (4,795 rows) and CelebA-like (162,770).
Repeats alternate the methods; medians, with every repeat listed so the spread can be read.  One JSON line per size.

    python tools/bench_mmd.py [--sizes waterbirds,celeba] [--repeats 5] [--parent-lib PATH] [--n-perm 20]
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


def torch_baseline(x, onehot, gammas, chunk=4096):
    """[L, G, G] sums over ORDERED pairs with the diagonal: fp32 cdist in row chunks, exp, one-hot products, float64 totals; one
    pass over the pairs per bandwidth, as a user without the fused kernel would write it"""
    out = []
    for gam in gammas:
        S = torch.zeros(onehot.shape[0], onehot.shape[0], dtype=torch.float64, device=x.device)
        for i in range(0, x.shape[0], chunk):
            k = torch.exp(-gam * torch.cdist(x[i:i + chunk], x) ** 2)
            S += (onehot[:, i:i + chunk] @ k @ onehot.T).double()
        out.append(S)
    return torch.stack(out)


def parent_distance_entry(path):
    """dbmm_pairdist_group_sums and its workspace size from another build of the library (the parent commit's)"""
    L = ctypes.CDLL(path)
    L.dbmm_workspace_bytes_pairdist.argtypes = _lib._SIGS["dbmm_workspace_bytes_pairdist"]
    L.dbmm_workspace_bytes_pairdist.restype = ctypes.c_size_t
    L.dbmm_pairdist_group_sums.argtypes = _lib._SIGS["dbmm_pairdist_group_sums"]

    def call(x, g, G, center):
        n, d = x.shape
        nbytes = L.dbmm_workspace_bytes_pairdist(n, d)
        ws = torch.empty((nbytes + 3) // 4, device=x.device, dtype=torch.float32)
        out = torch.empty((G, G), device=x.device, dtype=torch.float64)
        rc = L.dbmm_pairdist_group_sums(x.data_ptr(), g.data_ptr(), center.data_ptr(), out.data_ptr(), n, d, G, ws.data_ptr(), ws.numel() * 4,
                                        _lib.stream())
        assert rc == 0, rc
        return out
    return call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="waterbirds,celeba")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--n-perm", type=int, default=20)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_mmd needs the GPU: there is nothing to time without it"
    parent = parent_distance_entry(a.parent_lib) if a.parent_lib else None
    med = statistics.median
    r4 = lambda ts: [round(t, 6) for t in ts]                          # microseconds: the small size runs in a fraction of a millisecond
    for name in a.sizes.split(","):
        counts = SIZES[name]
        n = sum(counts)
        gen = torch.Generator().manual_seed(11)
        groups = np.repeat(np.arange(4), counts)                         # sorted by group: what analysis.mmd hands the kernel
        x = (0.5 * torch.randn(n, D, generator=gen) + 0.1 * torch.randn(1, D, generator=gen)).cuda()
        x += torch.from_numpy(groups).float().cuda().unsqueeze(1) * 0.05
        gd = torch.from_numpy(groups).cuda()
        center = x.mean(0)
        onehot = (gd.unsqueeze(0) == torch.arange(4, device="cuda").unsqueeze(1)).float()
        gammas = analysis.rbf_gammas(x, SCALES4).tolist()
        g1 = gammas[1:2]
        small = slice(0, 2048)                                           # warm-up: library load, code objects, allocator
        ops.pairdist_rbf_group_sums(x[small].contiguous(), gd[small].contiguous(), 4, center, gammas)
        ops.pairdist_group_sums(x[small].contiguous(), gd[small].contiguous(), 4, center)
        if parent:
            parent(x[small].contiguous(), gd[small].contiguous(), 4, center)
        torch_baseline(x[small], onehot[:, small], g1)
        t_l1, t_l4, t_dist, t_par, t_base = [], [], [], [], []

        def run_l1():
            t, K = timed(lambda: ops.pairdist_rbf_group_sums(x, gd, 4, center, g1))
            t_l1.append(t)
            return K

        def run_l4():
            t, K = timed(lambda: ops.pairdist_rbf_group_sums(x, gd, 4, center, gammas))
            t_l4.append(t)
            return K

        def run_dist():
            t, S = timed(lambda: ops.pairdist_group_sums(x, gd, 4, center))
            t_dist.append(t)
            return S

        def run_parent():
            t, S = timed(lambda: parent(x, gd, 4, center))
            t_par.append(t)
            return S

        # the order rotates with the repeat, so that no method always follows the same neighbour
        methods = [("l1", run_l1), ("l4", run_l4), ("dist", run_dist)] + ([("parent", run_parent)] if parent else [])
        res = {}
        for r in range(a.repeats):
            k = r % len(methods)
            for nm, fn in methods[k:] + methods[:k]:
                res[nm] = fn()
        K1, K4, S, Sp = res["l1"], res["l4"], res["dist"], res.get("parent")
        for _ in range(min(a.repeats, 3)):
            t, base = timed(lambda: torch_baseline(x, onehot, g1))
            t_base.append(t)
        full = K1[0].clone()                                             # -> ordered pairs with the diagonal of ones, as the baseline sums them
        full[torch.arange(4), torch.arange(4)] = 2.0 * torch.diag(K1[0]) + torch.tensor(counts, dtype=torch.float64, device="cuda")
        rel = ((full - base[0]).abs() / base[0]).max().item()
        assert torch.equal(K1[0], K4[1]), "a bandwidth's sums depend on the others in the call"
        mem = {"rbf_l4": peak_extra(lambda: ops.pairdist_rbf_group_sums(x, gd, 4, center, gammas)),
               "distance": peak_extra(lambda: ops.pairdist_group_sums(x, gd, 4, center)),
               "torch_per_bandwidth": peak_extra(lambda: torch_baseline(x, onehot, g1))}
        t_mmd = [timed(lambda: analysis.mmd(x, groups))[0] for _ in range(min(a.repeats, 3))]
        t_perm, perm = timed(lambda: analysis.mmd_permutation_test(x, groups, (1, 2), n_perm=a.n_perm, seed=0))
        pairs = n * (n - 1) / 2
        line = {"size": name, "rows": n, "dim": D, "repeats": a.repeats,
                "rbf_l1_s": round(med(t_l1), 6), "rbf_l4_s": round(med(t_l4), 6), "distance_s": round(med(t_dist), 6),
                "l4_over_l1": round(med(t_l4) / med(t_l1), 3), "l1_over_distance": round(med(t_l1) / med(t_dist), 3),
                "torch_cdist_exp_onehot_per_bandwidth_s": round(med(t_base), 6), "torch_x4_over_rbf_l4": round(4 * med(t_base) / med(t_l4), 2),
                "rbf_l1_fp16_tflops": round(pairs * 2 * 3 * D / med(t_l1) / 1e12, 1),
                "max_rel_diff_vs_torch_fp32": float(f"{rel:.3e}"),
                "peak_extra_mb": {k: round(v / 2 ** 20, 1) for k, v in mem.items()},
                "mmd_3_bandwidths_end_to_end_s": round(med(t_mmd), 6),
                "mmd_permutation_test_s": round(t_perm, 3), "n_perm": a.n_perm, "perm_rows": int(counts[1] + counts[2]), "perm_p": perm["p"],
                "all_rbf_l1_s": r4(t_l1), "all_rbf_l4_s": r4(t_l4), "all_distance_s": r4(t_dist), "all_torch_s": r4(t_base), "all_mmd_s": r4(t_mmd)}
        if parent:
            same = bool(torch.equal(S, Sp))
            line.update(distance_parent_s=round(med(t_par), 6), all_distance_parent_s=r4(t_par),
                        distance_over_parent=round(med(t_dist) / med(t_par), 4), distance_bits_equal_parent=same)
        print(json.dumps(line), flush=True)
        del x


if __name__ == "__main__":
    main()
