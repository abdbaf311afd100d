"""Wall time of a seed sweep in lock-step (trainer.train_sweep) against the same runs in sequence (set_seed + train_all_epochs per
replica: the path every run took before the sweep driver existed), on one device, in one process, alternating.

Two synthetic configurations at the published sizes, D = 1024, `--method` (default adapter_reg_seq_alter) with --add_adapter
--balance_val where the method has them (linear_probing: neither; adapter_reg: --balance_val):
  wb   Waterbirds-like: 4,795 / 1,199 / 5,794 rows, batch 1024, batch_size_reg 256
  ca   CelebA-like:     162,770 / 19,867 / 19,962 rows, batch 1024, batch_size_reg 4
For R in {2, 4, 8, 16}: one warm-up run of each path, then `--repeats` (>= 3) alternating pairs; host clock, every measurement ends
in a device synchronise.  Reported per R: median, min .. max of both paths and the ratio of the medians.

    python tools/bench_sweep.py                    # both configurations, one child process each under its own time limit
    python tools/bench_sweep.py --config wb        # one configuration in this process
    python tools/bench_sweep.py --method linear_probing
Prints one JSON line per (configuration, R) and a summary table; --log FILE appends them to a file."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time
from types import SimpleNamespace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CONFIGS = {
    "wb": dict(n_train=4795, n_val=1199, n_test=5794, batch_size=1024, batch_size_reg=256, epochs=6, efl=3, limit=600),
    "ca": dict(n_train=162770, n_val=19867, n_test=19962, batch_size=1024, batch_size_reg=4, epochs=4, efl=2, limit=1100),
}
D = 1024


def _dataset(seed, n, u_y, u_c, common):
    """synth.embedding_dataset's model (a class direction, a stronger spurious direction, isotropic noise) from torch's generator:
    the bench needs 200 k rows quickly, not a fixture"""
    import torch
    g = torch.Generator().manual_seed(seed)
    y = (torch.rand(n, generator=g) < 0.25).long()
    c = y ^ (torch.rand(n, generator=g) < 0.15).long()
    x = 0.5 * torch.randn(n, D, generator=g) + 0.1 * common
    x += 0.025 * (2 * y.float().unsqueeze(1) - 1) * u_y + 0.045 * (2 * c.float().unsqueeze(1) - 1) * u_c
    return x.contiguous(), y, c


def run_config(name, repeats, rs, log, method="adapter_reg_seq_alter"):
    import torch
    import dbmm_amd  # noqa: F401
    from dbmm_amd import optim, synth, trainer
    cfg = CONFIGS[name]
    tmp = tempfile.mkdtemp()
    tcls, tspu, tgrp = synth.embedding_text(7, D)
    o = dict(tl_method=method, dataset="waterbirds" if name == "wb" else "celeba", epochs=cfg["epochs"],
             epochs_feature_learning=cfg["efl"], batch_size=cfg["batch_size"], batch_size_reg=cfg["batch_size_reg"], learning_rate=0.05,
             learning_rate_reg=0.01, momentum=0.9, weight_decay=5e-5, cosine=False, lr_decay_epochs=[1000], lr_decay_rate=0.1, warm=False,
             warm_reg=False, adapter_feat_dim=128, zs_temperature=0.01, train_target="class", balance_val=method != "linear_probing",
             add_adapter="seq" in method, continue_from_best=False, init_near_identity=False, use_cls_prompt_in_reg=False, resample_ce=False, n_cls=2)
    for key, m, cols in (("text_embedding_dir", tcls, ["c0", "c1"]), ("text_spurious_embedding_dir", tspu, ["s0", "s1"]),
                         ("text_group_embedding_dir", tgrp, ["g0", "g1", "g2", "g3"])):
        o[key] = os.path.join(tmp, key + ".json")
        json.dump({n: m[:, i].numpy().tolist() for i, n in enumerate(cols)}, open(o[key], "w"))
    opt = SimpleNamespace(**o)
    u_y, u_c, common = synth.normal(7, "dir_class", (D,)), synth.normal(7, "dir_spur", (D,)), synth.normal(7, "common", (1, D))
    tables = []
    for k, split in enumerate(("n_train", "n_val", "n_test")):
        x, y, c = _dataset(100 + k, cfg[split], u_y, u_c, common)
        tables.append(trainer.EmbeddingTable(x.numpy(), y.numpy(), c.numpy(), device="cuda"))

    def sweep(seeds):
        t = time.perf_counter()
        out = trainer.train_sweep(opt, *tables, seeds)
        torch.cuda.synchronize()
        return time.perf_counter() - t, out

    def sequential(seeds):
        t = time.perf_counter()
        out = []
        for s in seeds:
            optim.set_seed(s)
            out.append(trainer.train_all_epochs(opt, *tables))
        torch.cuda.synchronize()
        return time.perf_counter() - t, out
    import contextlib
    import io
    lines = []
    for R in rs:
        seeds = list(range(40, 40 + R))
        with contextlib.redirect_stdout(io.StringIO()):
            _, a = sweep(seeds)                                 # warm-up of each path (allocator, workspaces, text matrices)
            _, b = sequential(seeds)
        same = a == b
        ts, tq = [], []
        for _ in range(repeats):
            with contextlib.redirect_stdout(io.StringIO()):
                ts.append(sweep(seeds)[0])
                tq.append(sequential(seeds)[0])
        rec = dict(config=name, method=method, R=R, repeats=repeats, epochs=cfg["epochs"], sweep_s=[round(t, 4) for t in ts], sequential_s=[round(t, 4) for t in tq],
                   sweep_median_s=round(statistics.median(ts), 4), sequential_median_s=round(statistics.median(tq), 4),
                   speedup=round(statistics.median(tq) / statistics.median(ts), 3), same_results=bool(same),
                   device=torch.cuda.get_device_name(0))
        line = json.dumps(rec)
        print(line, flush=True)
        lines.append(line)
        if log:
            with open(log, "a") as f:
                f.write(line + "\n")
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", choices=list(CONFIGS))
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--R", type=str, default="2,4,8,16")
    ap.add_argument("--log", type=str, default=None)
    ap.add_argument("--method", default="adapter_reg_seq_alter",
                    choices=["adapter", "adapter_reg", "adapter_reg_seq", "adapter_reg_seq_alter", "linear_probing"])
    a = ap.parse_args()
    if a.repeats < 3:
        ap.error("--repeats must be at least 3 (the spread is part of the result)")
    rs = [int(r) for r in a.R.split(",")]
    if a.config:
        run_config(a.config, a.repeats, rs, a.log, a.method)
        return 0
    # both configurations: a fresh child process each, under its own time limit; nothing more is started after a failure
    for name in CONFIGS:
        cmd = ["timeout", "-k", "10", str(CONFIGS[name]["limit"]), sys.executable, os.path.abspath(__file__), "--config", name, "--repeats",
               str(a.repeats), "--R", a.R, "--method", a.method] + (["--log", a.log] if a.log else [])
        rc = subprocess.run(cmd).returncode
        if rc != 0:
            print(f"bench_sweep: configuration {name} ended with status {rc}; stopping", file=sys.stderr)
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
