"""Time the PCA map (analysis.pca on the fused scatter kernel and the streaming projection) against the same result composed from
torch ops on the same GPU: xc = x - mean (a centred copy), fp32 xc.T @ xc, the same host eigen-solve, xc @ V.T.

Two sizes, D = 1024: Waterbirds-like (4,795 rows) and CelebA-like (162,770 rows).  Medians of 7 alternating windows.  Reported
separately: the covariance launch pair, the projection kernel, the host eigen-solve, end to end (analysis.pca with its column sums
and group centroids; the torch composition with its mean, centred copy and centroids), the peak extra device memory of both paths,
and the worst error of BOTH scatter matrices against float64 on a 20,000-row sample, as |S - S_ref| / sqrt(S_aa S_bb).

Beside host_eigh and pca_end_to_end, in the same alternating windows: device_eig (ops.sym_eig_topk alone on the resident scatter
matrix) and pca_end_to_end_device (analysis.pca(solver="device")), with the iterations, `converged` and the path `pca` used.
--spectrum iso (the default) draws isotropic noise plus one group direction: the second eigenvalue sits in the noise bulk and the
device solver is expected NOT to converge (what the failed attempt plus the fall-back costs is printed).  --spectrum powerlaw gives
the rows a covariance with eigenvalues proportional to 1 / j in a random orthogonal frame: a stand-in for real embeddings, whose
spectrum has not been measured here.

    python tools/bench_pca.py [--sizes waterbirds,celeba] [--windows 7] [--spectrum iso|powerlaw]
"""
import argparse
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
D, K = 1024, 2
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


def torch_pca(x, groups_dev, n_groups, k):
    """the composition a user writes without the kernels"""
    mean = x.mean(0)
    xc = x - mean
    S = xc.T @ xc
    comp, var, ratio, total = analysis.pca_from_scatter(S.double().cpu().numpy(), mean.cpu().numpy(), mean.double().cpu().numpy(), x.shape[0], k)
    coords = xc @ torch.from_numpy(comp).to(x.device).T
    cent = torch.zeros(n_groups, k, device=x.device).index_add_(0, groups_dev, coords) / torch.bincount(groups_dev, minlength=n_groups).unsqueeze(1)
    return S, coords, cent.cpu()


def scatter_errors(x, n_sample=20000):
    """worst |S - S_ref| / sqrt(S_aa S_bb) of the kernel's and of torch's fp32 scatter matrix on the first rows, float64 reference"""
    xs = x[:n_sample].contiguous()
    mean = xs.double().mean(0)
    c = mean.float()
    xd = xs.double() - c.double()
    ref = xd.T @ xd
    dg = ref.diagonal().sqrt()
    scale = torch.outer(dg, dg)
    ours = ops.covariance(xs, c)
    xc = xs - c
    theirs = (xc.T @ xc).double()
    return ((ours - ref).abs() / scale).max().item(), ((theirs - ref).abs() / scale).max().item(), xs.shape[0]


def powerlaw_mixer(gen):
    """[D, D] on the device: diag(j^-1/2) U^T for a random orthogonal U, so that rows z @ mixer of white z have a covariance with
    eigenvalues proportional to 1 / j in a random frame"""
    U, _ = torch.linalg.qr(torch.randn(D, D, generator=gen, dtype=torch.float64))
    return ((torch.arange(1, D + 1, dtype=torch.float64) ** -0.5).unsqueeze(1) * U.T).float().cuda()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="waterbirds,celeba")
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--spectrum", choices=("iso", "powerlaw"), default="iso",
                    help="iso: isotropic noise plus one group direction; powerlaw: covariance eigenvalues proportional to 1 / j")
    a = ap.parse_args()
    med = statistics.median
    if a.spectrum == "powerlaw":
        print("spectrum powerlaw: a STAND-IN for real embeddings, whose spectrum has not been measured here", flush=True)
    for name in a.sizes.split(","):
        counts = SIZES[name]
        n = sum(counts)
        gen = torch.Generator().manual_seed(11)
        groups = np.repeat(np.arange(4), counts)[torch.randperm(n, generator=gen).numpy()]
        x = (0.5 * torch.randn(n, D, generator=gen) + 0.1 * torch.randn(1, D, generator=gen)).cuda()
        if a.spectrum == "powerlaw":
            mixer = powerlaw_mixer(gen)
            for i in range(0, n, 16384):                                 # in place, block by block: no second copy of the rows
                x[i:i + 16384] = (x[i:i + 16384] @ mixer) * 8.0
            del mixer
        x += torch.from_numpy(groups).float().cuda().unsqueeze(1) * 0.05
        gd = torch.from_numpy(groups).cuda()
        name = f"{name}/{a.spectrum}"
        fit = analysis.pca(x, groups, K)                                 # warm-up of every shape timed below
        c = torch.from_numpy(fit["mean"]).cuda()
        V = torch.from_numpy(fit["components"]).cuda()
        scatter_dev = ops.covariance(x, c)
        scatter = scatter_dev.cpu().numpy()
        mean64 = fit["mean"].astype(np.float64)
        torch_pca(x, gd, 4, K)
        vals, vecs, info = ops.sym_eig_topk(scatter_dev, K)              # float32(mean) is the centre here: nothing to correct
        fit_dev = analysis.pca(x, groups, K, solver="device")
        w_host = np.linalg.eigvalsh(scatter)[::-1]
        print(f"{name} N={n} D={D} k={K} device_eig: iterations {info['iterations']}, converged {info['converged']}, state {info['state']}, "
              f"residual {info['residual']:.3e}; lambda_17 / lambda_k = {w_host[16] / w_host[K - 1]:.4f}; "
              f"|theta - lambda| / lambda_1 = {np.abs(vals.cpu().numpy() - w_host[:K]).max() / w_host[0]:.3e}", flush=True)
        print(f"{name} N={n} D={D} k={K} pca(solver='device'): used {fit_dev['eig']['used']}, iterations {fit_dev['eig']['iterations']}, "
              f"converged {fit_dev['eig']['converged']}", flush=True)
        steps = 20 if n < 20000 else 5
        legs = {
            "covariance_pair": (lambda: ops.covariance(x, c), steps),
            "torch_center_gemm": (lambda: (lambda xc: xc.T @ xc)(x - c), steps),
            "project_rows": (lambda: ops.project_rows(x, c, V), steps),
            "torch_center_project": (lambda: (x - c) @ V.T, steps),
            "host_eigh": (lambda: analysis.pca_from_scatter(scatter, fit["mean"], mean64, n, K), 1),
            "device_eig": (lambda: ops.sym_eig_topk(scatter_dev, K), 1),
            "pca_end_to_end": (lambda: analysis.pca(x, groups, K), 1),
            "pca_end_to_end_device": (lambda: analysis.pca(x, groups, K, solver="device"), 1),
            "torch_end_to_end": (lambda: torch_pca(x, gd, 4, K), 1),
        }
        times = {k: [] for k in legs}
        for _ in range(a.windows):                                       # alternating: one window of every leg per round
            for leg, (fn, st) in legs.items():
                times[leg].append(window(fn, st)[0])
        for leg, (fn, st) in legs.items():
            ts = times[leg]
            print(f"{name} N={n} D={D} k={K} {leg}: median {med(ts) * 1e3:.3f} ms/call of {a.windows} windows x {st} calls: "
                  + " ".join(f"{t * 1e3:.3f}" for t in ts), flush=True)
        t_cov, t_proj = med(times["covariance_pair"]), med(times["project_rows"])
        nt = D // 64
        flop = 2.0 * n * (nt * (nt + 1) // 2) * 64 * 64
        print(f"{name} N={n} covariance_pair: {flop / 1e9:.1f} GFLOP of the upper triangle at {flop / t_cov / 1e12:.1f} TF (fp32 MFMA peak 155); "
              f"torch_center_gemm / covariance_pair = {med(times['torch_center_gemm']) / t_cov:.2f}", flush=True)
        print(f"{name} N={n} project_rows: {n * D * 4 / 1e6:.1f} MB at {n * D * 4 / t_proj / 1e12:.2f} TB/s = {100 * n * D * 4 / t_proj / 1e12 / COPY_TBS:.0f} % of the "
              f"{COPY_TBS} TB/s copy rate; torch_center_project / project_rows = {med(times['torch_center_project']) / t_proj:.2f}", flush=True)
        print(f"{name} N={n} end to end: torch_end_to_end / pca_end_to_end = {med(times['torch_end_to_end']) / med(times['pca_end_to_end']):.2f}", flush=True)
        t_host, t_dev = med(times["host_eigh"]), med(times["device_eig"])
        e2e, e2e_dev = med(times["pca_end_to_end"]), med(times["pca_end_to_end_device"])
        print(f"{name} N={n} eigen step: host_eigh / device_eig = {t_host / t_dev:.2f} ({'converged' if info['converged'] else 'NOT converged'} "
              f"after {info['iterations']} iterations, {t_dev / max(info['iterations'], 1) * 1e6:.1f} us per iteration with the status reads)", flush=True)
        print(f"{name} N={n} end to end with solver='device' (used {fit_dev['eig']['used']}): pca_end_to_end / pca_end_to_end_device = "
              f"{e2e / e2e_dev:.2f}; the device attempt adds {(e2e_dev - e2e) * 1e3:+.3f} ms to the host path's {e2e * 1e3:.3f} ms", flush=True)
        m_ours = peak_extra(lambda: analysis.pca(x, groups, K))
        m_torch = peak_extra(lambda: torch_pca(x, gd, 4, K))
        print(f"{name} N={n} peak extra device memory: pca {m_ours / 2**20:.1f} MB, torch composition {m_torch / 2**20:.1f} MB, rows {n * D * 4 / 2**20:.1f} MB",
              flush=True)
        e_ours, e_torch, ns = scatter_errors(x)
        print(f"{name} N={n} worst |S - S_ref| / sqrt(S_aa S_bb) against float64 on {ns} rows: covariance kernel {e_ours:.3e}, torch fp32 GEMM {e_torch:.3e}",
              flush=True)
        del x, fit, scatter


if __name__ == "__main__":
    main()
