"""Kernel launches per training step of the replica-batched sweep, for a rocprofv3 kernel trace.

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o s -- python tools/sweep_launch_count.py --R 8
    python tools/sweep_launch_count.py --summarise R2_kernel_stats.csv R8_kernel_stats.csv        # the table under profiles/
    python tools/sweep_launch_count.py --summarise-linear R2_kernel_stats.csv R8_kernel_stats.csv # for --method linear_probing runs

The run: Waterbirds-like sizes (1,199 validation rows, D = 1024), R MultipleAdapter replicas, stage-2 passes of the sweep driver
(trainer._sweep_train_pass: balanced reg subset, group prompts) at batch_size_reg 256 and 16, nothing else on the device afterwards.
Prints the number of steps taken; every sweep_* kernel in the trace comes from those steps, everything else from the set-up.
`--method linear_probing`: R LinearClassifier replicas instead, two shuffled training passes over the table at batch 256 (one
launch per step) and 600 (two launches per step) and one evaluation pass (trainer._sweep_validate) in batches of 512: every
linear_sweep_* kernel and every memset in the trace comes from those."""
import csv
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def run(R):
    import json
    import tempfile

    import numpy as np
    import torch
    import dbmm_amd  # noqa: F401
    from dbmm_amd import adapter, synth, trainer
    D = 1024
    tmp = tempfile.mkdtemp()
    paths = []
    for nm, m, cols in zip(("c", "s", "g"), synth.embedding_text(7, D), (["c0", "c1"], ["s0", "s1"], ["g0", "g1", "g2", "g3"])):
        p = os.path.join(tmp, nm + ".json")
        json.dump({n: m[:, i].numpy().tolist() for i, n in enumerate(cols)}, open(p, "w"))
        paths.append(p)
    x, y, c = synth.embedding_dataset(7, "val", 1199, D)
    table = trainer.EmbeddingTable(x.numpy(), y.numpy(), c.numpy(), device="cuda")
    reg_idx, _ = adapter.stratified_split_indices(table.group_array, 0.5)
    seeds = list(range(R))
    streams = trainer.ReplicaStreams(seeds)
    mods = [streams.run(r, lambda: adapter.MultipleAdapter(adapter.CustomCLIP(adapter.Adapter(D, 128), *paths), adapter.Adapter(D, 128),
                                                           init_near_identity=False)) for r in range(R)]
    sweep = adapter.SweepAdapters.from_modules(mods, "cuda")
    steps = 0
    for bsr in (256, 16):
        bal = [streams.run(r, adapter.balance_val_indices, table.group_array[reg_idx], 4, bsr) for r in range(R)]

        def order(r):
            torch.empty((), dtype=torch.int64).random_()
            return torch.as_tensor(np.asarray(reg_idx[bal[r][0]]), dtype=torch.int64)
        c, ls, orders, _ = trainer._sweep_train_pass(streams, sweep, table, order, bal[0][1], "class", True, lambda i, n: [0.01] * R, 0.9, 5e-5)
        steps += -(-len(orders[0]) // bal[0][1])
    torch.cuda.synchronize()
    print(f"R={R} steps={steps} rows_per_pass={len(orders[0])}")


LINEAR_ROWS, LINEAR_BATCHES, LINEAR_EVAL_BATCH = 1199, (256, 600), 512


def linear_expected():
    """what run_linear must leave in a trace, whatever R is: (one-launch steps, two-launch steps, evaluation batches)"""
    one = sum(-(-LINEAR_ROWS // b) for b in LINEAR_BATCHES if b <= 512)
    two = sum(-(-LINEAR_ROWS // b) for b in LINEAR_BATCHES if b > 512)
    return one, two, -(-LINEAR_ROWS // LINEAR_EVAL_BATCH)


def run_linear(R):
    import torch
    import dbmm_amd  # noqa: F401
    from dbmm_amd import adapter, synth, trainer
    D = 1024
    x, y, c = synth.embedding_dataset(7, "val", LINEAR_ROWS, D)
    table = trainer.EmbeddingTable(x.numpy(), y.numpy(), c.numpy(), device="cuda")
    streams = trainer.ReplicaStreams(list(range(R)))
    sweep = adapter.SweepLinear.from_modules([streams.run(r, adapter.LinearClassifier, D, 2) for r in range(R)], "cuda")
    for bs in LINEAR_BATCHES:
        trainer._sweep_train_pass(streams, sweep, table, lambda r: trainer.dataloader_shuffle_order(len(table)), bs, "class", False,
                                  lambda i, n: [0.01] * R, 0.9, 5e-5)
    trainer._sweep_validate(streams, sweep, table, LINEAR_EVAL_BATCH, "class", None, len(table))
    torch.cuda.synchronize()
    one, two, ev = linear_expected()
    print(f"R={R} steps at batch 256 (1 kernel + 1 memset each)={one} steps at batch 600 (2 kernels each)={two} "
          f"evaluation batches (1 kernel + 1 memset each)={ev}")


def summarise_linear(files):
    """per trace: linear_sweep_rows_kernel launches split by their MODE template argument (0 evaluation, 1 one-launch step, 2 first
    launch of a two-launch step), the reduce launches, and the memsets, against what run_linear does.  hipMemsetAsync on device
    memory runs as a fill kernel of the runtime (a name with `fillBuffer`), so the memsets are in the kernel trace too; the
    library issues one per one-launch step and per evaluation batch, torch may add its own, so the count is a lower-bound check
    here and exact in the hipMemsetAsync row of a `rocprofv3 --hip-trace --stats` run of its own."""
    one, two, ev = linear_expected()
    want = {"step (MODE 1)": one, "partial (MODE 2)": two, "reduce": two, "evaluation (MODE 0)": ev}
    ok = True
    for f in files:
        got = {k: 0 for k in want}
        fills, bad = 0, []
        for r in csv.DictReader(open(f)):
            name, calls = r["Name"], int(r["Calls"])
            m = re.search(r"linear_sweep_rows_kernel<\s*\d+\s*,\s*\d+\s*,\s*(\d)\s*>", name)
            if m:
                got[{"0": "evaluation (MODE 0)", "1": "step (MODE 1)", "2": "partial (MODE 2)"}[m.group(1)]] += calls
            elif "linear_sweep_reduce_sgd_kernel" in name:
                got["reduce"] += calls
            elif "fillBuffer" in name:
                fills += calls
            elif "gather_rows" in name or "group_count" in name or "index" in name.lower():
                bad.append(name.split("(")[0][:70])
        print(f"{os.path.basename(f)}: " + ", ".join(f"{k} {got[k]} (expected {want[k]})" for k in want)
              + f"; runtime fill kernels (memsets) {fills} (the library's: {one + ev}); gather / group_count / index kernels: {bad or 'none'}")
        ok = ok and got == want and fills >= one + ev and not bad
    print("launch counts as expected in every trace" if ok else "LAUNCH COUNTS DIFFER FROM WHAT WAS EXPECTED")
    return ok


def summarise(files):
    short = lambda n: re.sub(r"\(anonymous namespace\)::|void ", "", n).split("(")[0][:70]
    tables = []
    for f in files:
        rows = list(csv.DictReader(open(f)))
        tables.append({short(r["Name"]): int(r["Calls"]) for r in rows})
    names = sorted(set().union(*tables), key=lambda n: (not n.startswith("sweep_"), n))
    print(f"{'kernel':72s}" + "".join(f"{os.path.basename(f)[:18]:>20s}" for f in files))
    for n in names:
        print(f"{n:72s}" + "".join(f"{t.get(n, 0):20d}" for t in tables))
    for f, t in zip(files, tables):
        sw = sum(v for k, v in t.items() if k.startswith("sweep_"))
        steps = t.get("sweep_sgd_kernel", 0)
        bad = [k for k in t if "gather_rows" in k or "index" in k.lower()]
        print(f"{os.path.basename(f)}: {sw} sweep_* launches over {steps} steps = {sw / max(steps, 1):.2f} per step; gather / index kernels: {bad or 'none'}")


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--summarise-linear":
        sys.exit(0 if summarise_linear(sys.argv[2:]) else 1)
    elif len(sys.argv) > 1 and sys.argv[1] == "--summarise":
        summarise(sys.argv[2:])
    else:
        method = sys.argv[sys.argv.index("--method") + 1] if "--method" in sys.argv else "adapter_reg_seq_alter"
        (run_linear if method == "linear_probing" else run)(int(sys.argv[sys.argv.index("--R") + 1]) if "--R" in sys.argv else 8)
