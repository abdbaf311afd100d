"""Kernel launches per training step of the replica-batched sweep, for a rocprofv3 kernel trace.

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o s -- python tools/sweep_launch_count.py --R 8
    python tools/sweep_launch_count.py --summarise R2_kernel_stats.csv R8_kernel_stats.csv        # the table under profiles/

The run: Waterbirds-like sizes (1,199 validation rows, D = 1024), R MultipleAdapter replicas, stage-2 passes of the sweep driver
(trainer._sweep_train_pass: balanced reg subset, group prompts) at batch_size_reg 256 and 16, nothing else on the device afterwards.
Prints the number of steps taken; every sweep_* kernel in the trace comes from those steps, everything else from the set-up."""
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
        c, ls, orders = trainer._sweep_train_pass(streams, sweep, table, order, bal[0][1], "class", True, lambda i, n: [0.01] * R, 0.9, 5e-5)
        steps += -(-len(orders[0]) // bal[0][1])
    torch.cuda.synchronize()
    print(f"R={R} steps={steps} rows_per_pass={len(orders[0])}")


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
    if len(sys.argv) > 1 and sys.argv[1] == "--summarise":
        summarise(sys.argv[2:])
    else:
        run(int(sys.argv[sys.argv.index("--R") + 1]) if "--R" in sys.argv else 8)
