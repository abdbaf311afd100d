"""Time deep feature reweighting (trainer.train_dfr) on the fused L1 proximal probe kernel against what a user would otherwise run:

  iteration     one FISTA iteration of R probes: ops.linear_prox_fit (32 iterations a launch, one workgroup per probe) against the
                same iteration batched over the probes with torch ops on the same GPU (baddbmm / softmax / bmm on a gathered
                [R, n, D] copy of the rows: the honest competitor), at R = the tuning call's and the refit's probe counts;
  row visit     seconds per (row x iteration) of ONE workgroup, R = 1: what dfr.MAX_ROW_VISITS is derived from;
  train_dfr     DFR-Val end to end (7 C x 1 tuning subset, 10 refits) with solver="device", and with the torch composition put in
                fit_l1_probes' place at the same convergence cadence;
  saga          sklearn's LogisticRegression(penalty="l1", solver="saga") on the host for ONE probe of the refit's size, where
                sklearn imports (train_dfr fits 17 of them);
  set-up        dfr.prox_steps (the Gram matrix in float64 on the device, a host eigvalsh per probe), separately.

Two val sizes, D = 1024, two classes: Waterbirds-like (val 1,199 rows, groups 467 / 466 / 133 / 133: 532-row subsets, 264-row tuning
subsets) and CelebA-like (val 19,867 rows, groups 8,535 / 8,276 / 2,874 / 182: 728 and 364).  Medians of 7 alternating windows in one
process.

    python tools/bench_dfr.py [--sizes waterbirds,celeba] [--windows 7]
"""
import argparse
import os
import statistics
import sys
import time
from types import SimpleNamespace

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import dbmm_amd  # noqa: E402,F401
from dbmm_amd import dfr, ops, trainer  # noqa: E402

# split -> (train rows, val group counts, test rows); groups are 2 y + c
SIZES = {"waterbirds": (4795, (467, 466, 133, 133), 5794), "celeba": (162770, (8535, 8276, 2874, 182), 19962)}
D = 1024


def window(fn, steps):
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(steps):
        out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) / steps, out


def make_table(gen, counts):
    """a table with these group counts, built as synth.embedding_dataset builds its rows (class and spurious directions in noise)"""
    g = torch.cat([torch.full((k,), i) for i, k in enumerate(counts)])
    g = g[torch.randperm(len(g), generator=gen)]
    y, c = g // 2, g % 2
    u_y, u_c = make_table.dirs
    x = 0.5 * torch.randn(len(g), D, generator=gen) + 0.025 * (2 * y.float()[:, None] - 1) * u_y + 0.045 * (2 * c.float()[:, None] - 1) * u_c
    return trainer.EmbeddingTable(x, y.numpy(), c.numpy(), device="cuda")


def split_counts(n, like):
    p = np.array(like, dtype=np.float64) / sum(like)
    k = np.floor(p * n).astype(int)
    k[0] += n - k.sum()
    return tuple(int(v) for v in k)


def torch_iterations(X, onehot, lam, step, W, b, V, c, betas):
    """len(betas) iterations of the module's iteration, batched over the probes: X [R, n, D], onehot [R, n, C], lam / step [R, 1, 1]"""
    n = X.shape[1]
    thr = step * lam
    for beta in betas:
        p = torch.softmax(torch.baddbmm(c.unsqueeze(1), X, V.transpose(1, 2)), dim=2) - onehot
        G = torch.bmm(p.transpose(1, 2), X) / n
        z = V - step * G
        Wn = torch.sign(z) * torch.clamp(z.abs() - thr, min=0)
        bn = c - step[:, :, 0] * (p.sum(1) / n)
        V, c = Wn + beta * (Wn - W), bn + beta * (bn - b)
        delta, W, b = (Wn - W).abs().amax((1, 2)), Wn, bn
    return W, b, V, c, delta


def fit_torch(table, idx, labels, lam, solver="device", tol=1e-4, max_iter=1000, check_every=32, n_classes=2, accelerate=True, steps=None):
    """dfr.fit_l1_probes with the torch composition in the kernel's place: the same steps, cadence and stopping rule"""
    dev = table.device
    idx = torch.as_tensor(np.asarray(idx)).to(dev)
    R, n = idx.shape
    t0 = time.perf_counter()
    steps = dfr.prox_steps(table, idx)
    setup = time.perf_counter() - t0
    X = table[idx]
    onehot = torch.nn.functional.one_hot(labels[idx], n_classes).float()
    lam_d = torch.as_tensor(lam, dtype=torch.float32).to(dev).view(R, 1, 1)
    step_d = steps.float().to(dev).view(R, 1, 1)
    W = torch.zeros(R, n_classes, table.shape[1], device=dev)
    b = torch.zeros(R, n_classes, device=dev)
    V, c, t, done = W.clone(), b.clone(), 1.0, 0
    while done < max_iter:
        k = dfr.launch_iters(n, check_every, max_iter - done)
        betas, t = dfr.beta_sequence(k, t)
        W, b, V, c, delta = torch_iterations(X, onehot, lam_d, step_d, W, b, V, c, betas)
        done += k
        ok = (delta <= tol * W.abs().amax((1, 2)).clamp_min(dfr.TINY)).cpu()
        if bool(ok.all()):
            break
    return dfr.ProxFit(W, b, torch.full((R,), done), (W != 0).sum((1, 2)).cpu(), ok, steps, setup, "torch")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="waterbirds,celeba")
    ap.add_argument("--windows", type=int, default=7)
    a = ap.parse_args()
    med = statistics.median
    try:
        from sklearn.linear_model import LogisticRegression
    except ImportError:
        LogisticRegression = None
        print("sklearn does not import here: no saga leg", flush=True)
    for name in a.sizes.split(","):
        n_train, val_counts, n_test = SIZES[name]
        gen = torch.Generator().manual_seed(7)
        make_table.dirs = (torch.randn(D, generator=gen), torch.randn(D, generator=gen))
        tr, va, te = make_table(gen, split_counts(n_train, val_counts)), make_table(gen, val_counts), make_table(gen, split_counts(n_test, (1, 1, 1, 1)))
        mean, std = dfr.column_moments(tr.embeddings)
        zv = dfr.standardised(va.embeddings, mean, std)
        labels = va.targets
        halves = dfr.val_halves(len(va), 0)
        tune = dfr.balanced_subsets(va.group_array, halves[0], [1])
        refit = dfr.balanced_subsets(va.group_array, np.arange(len(va)), range(2, 12))
        tag = f"{name} val={len(va)} D={D}"
        print(f"{tag}: tuning subsets of {tune.shape[1]} rows, refit subsets of {refit.shape[1]} rows", flush=True)

        # ---- per iteration: the kernel against the torch composition, at the two calls' shapes and at 70 probes
        legs, per = {}, {}
        K = 32
        betas = dfr.beta_sequence(K)[0]
        for what, idx_np, C_list in (("tune R=7", np.repeat(tune, 7, 0), dfr.DEFAULT_C_GRID), ("refit R=10", refit, [0.1] * 10),
                                     ("sweep R=70", np.concatenate([refit] * 7), list(dfr.DEFAULT_C_GRID) * 10)):
            idx = torch.from_numpy(idx_np).cuda()
            R, n = idx.shape
            lam = torch.tensor([1.0 / (c * n) for c in C_list], dtype=torch.float32, device="cuda")
            t0 = time.perf_counter()
            steps = dfr.prox_steps(zv, idx[:10])
            setup = (time.perf_counter() - t0) / min(R, 10)
            print(f"{tag} {what}: step set-up {setup * 1e3:.1f} ms per probe (n = {n}: Gram matrix of {min(n, D + 1)} x {min(n, D + 1)}, host eigvalsh)", flush=True)
            step = steps.float().cuda().repeat((R + 9) // 10)[:R].contiguous()
            state = ops.linear_prox_state(R, 2, D, "cuda")
            X, onehot = zv[idx], torch.nn.functional.one_hot(labels[idx], 2).float()
            ts = [torch.zeros(R, 2, D, device="cuda"), torch.zeros(R, 2, device="cuda")]
            ts = ts + [t.clone() for t in ts]
            legs[f"{what} kernel"] = (lambda idx=idx, lam=lam, step=step, state=state: ops.linear_prox_fit(zv, idx, labels, lam, step, state, K), 10)
            legs[f"{what} torch"] = (lambda X=X, onehot=onehot, lam=lam, step=step, ts=ts:
                                     torch_iterations(X, onehot, lam.view(-1, 1, 1), step.view(-1, 1, 1), *ts, betas), 3)
            per[what] = (R, n)
        one = torch.from_numpy(refit[:1]).cuda()
        n1 = one.shape[1]
        lam1, step1 = torch.tensor([1.0 / (0.1 * n1)], device="cuda"), dfr.prox_steps(zv, one).float().cuda()
        st1 = ops.linear_prox_state(1, 2, D, "cuda")
        legs["row visit R=1 kernel"] = (lambda: ops.linear_prox_fit(zv, one, labels, lam1, step1, st1, K), 10)

        # ---- DFR-Val end to end
        opt = SimpleNamespace(n_cls=2, batch_size=128)
        real_fit = dfr.fit_l1_probes

        def run_dfr(fit):
            dfr.fit_l1_probes = fit
            try:
                return trainer.train_dfr(opt, tr, va, te)
            finally:
                dfr.fit_l1_probes = real_fit
        for leg, fit in (("train_dfr kernel", real_fit), ("train_dfr torch", fit_torch)):
            _, scores, rec = run_dfr(fit)                                            # warm-up, and what was computed
            print(f"{tag} {leg}: C = {rec['C']}, worst-group test accuracy {scores[2][2]['worst_acc']}, refit iterations {rec['iterations'][0]}, "
                  f"tuning iterations {rec['tune_iterations'][0]}, converged {all(rec['converged']) and all(rec['tune_converged'])}, "
                  f"nnz {min(rec['nnz'])} .. {max(rec['nnz'])} of {2 * D}; step set-up {rec['setup_seconds'] * 1e3:.0f} ms, tune {rec['tune_seconds'] * 1e3:.0f} ms, "
                  f"refit {rec['fit_seconds'] * 1e3:.0f} ms (both include their set-up)", flush=True)
            legs[leg] = (lambda fit=fit: run_dfr(fit), 1)
        legs["step set-up, 17 probes"] = (lambda: (dfr.prox_steps(zv, np.repeat(tune, 7, 0)), dfr.prox_steps(zv, refit)), 1)

        for fn, _ in legs.values():                                                 # warm-up of every leg
            fn()
        times = {leg: [] for leg in legs}
        for _ in range(a.windows):                                                   # alternating: one window of every leg per round
            for leg, (fn, st) in legs.items():
                times[leg].append(window(fn, st)[0])
        for leg, (fn, st) in legs.items():
            ts = times[leg]
            print(f"{tag} {leg}: median {med(ts) * 1e3:.3f} ms/call of {a.windows} windows x {st} calls: " + " ".join(f"{t * 1e3:.3f}" for t in ts),
                  flush=True)
        for what, (R, n) in per.items():
            k, t = med(times[f"{what} kernel"]) / K, med(times[f"{what} torch"]) / K
            print(f"{tag} {what}, n = {n}: kernel {k * 1e6:.1f} us / iteration ({k / n * 1e9:.1f} ns per row visit of a workgroup), torch composition "
                  f"{t * 1e6:.1f} us / iteration; torch / kernel = {t / k:.2f}", flush=True)
        k1 = med(times["row visit R=1 kernel"]) / K
        print(f"{tag} ONE workgroup, n = {n1}: {k1 * 1e6:.1f} us / iteration = {k1 / n1 * 1e9:.1f} ns per row visit; dfr.MAX_ROW_VISITS = {dfr.MAX_ROW_VISITS} "
              f"row visits are {dfr.MAX_ROW_VISITS * k1 / n1 * 1e3:.2f} ms a launch", flush=True)
        dk, dt = med(times["train_dfr kernel"]), med(times["train_dfr torch"])
        print(f"{tag} train_dfr: kernel {dk * 1e3:.0f} ms, torch composition {dt * 1e3:.0f} ms (torch / kernel = {dt / dk:.2f}); the step set-up of the 17 "
              f"probes is {med(times['step set-up, 17 probes']) * 1e3:.0f} ms of either", flush=True)

        if LogisticRegression is not None:
            rows = refit[0]
            Xh, yh = zv[torch.from_numpy(rows).cuda()].cpu().numpy(), labels[torch.from_numpy(rows).cuda()].cpu().numpy()
            for C in (1.0, 0.1):
                ts = []
                for _ in range(3):
                    t0 = time.perf_counter()
                    sk = LogisticRegression(penalty="l1", solver="saga", C=C, tol=1e-4, max_iter=1000).fit(Xh, yh)
                    ts.append(time.perf_counter() - t0)
                print(f"{tag} saga (host, sklearn), ONE probe of {len(rows)} rows at C = {C}: median {med(ts) * 1e3:.0f} ms of 3 ({int(sk.n_iter_[0])} epochs, "
                      f"{int((sk.coef_ != 0).sum())} nonzeros); train_dfr fits 17", flush=True)
        del tr, va, te, zv


if __name__ == "__main__":
    main()
