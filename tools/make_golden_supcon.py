"""Generate tests/golden/supcon.npz from the REFERENCE's own SupervisedContrastiveLoss (demo/visualizer_supcon.py).

Same method as tools/make_golden_group_stats.py: nothing of the reference is copied.  Its module cannot be imported here, so the
class definition is compiled from the file in place (needs the reference tree, read-only) and run unmodified on the CPU in float64.
The class scores ONE anchor per call on a batch [anchor; its positives; its negatives] through `model.forward_ca`, which its
CustomCLIP has commented out; forward_ca is "adapter, then row-normalise", so the model handed to it row-normalises its input and
the input rows are the adapter outputs z.  Per case the class is called once per anchor that has a positive; the case's loss is the
mean over those anchors, dL/dz its gradient (torch autograd through the reference's own statements).

The class cannot score an anchor without negatives (its slice [-0:] takes the whole batch) and is not called for an anchor without
positives; asserted before anything is written:
  * exactly one row of every case has a label of its own (no positives: not an anchor, A = B - 1);
  * every other row has at least one positive and at least one negative.

Only numbers are saved: z (float32, one matrix per shape, shared by that shape's cases), labels, tau, the per-anchor losses (0 for
the row that is no anchor), their mean and dL/dz in float64 -- for B = 37 every fourth column of dL/dz, to keep the file small.

    python tools/make_golden_supcon.py
"""
import ast
import os
import sys
from types import SimpleNamespace

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))

import make_golden as MG  # noqa: E402  (path setup, the reference's location)

SRC = os.path.join(MG.REF, "demo", "visualizer_supcon.py")
OUT = os.path.join(ROOT, "tests", "golden", "supcon.npz")
SHAPES = ((12, 64), (37, 128))
TAUS = (0.1, 0.05)
N_LABELS = (2, 4)
DZ_STRIDE = {12: 1, 37: 4}                     # columns of dL/dz recorded


def case_name(B, D, tau, k):
    return f"b{B}_d{D}_t{tau}_k{k}"


def make_z(B, D):
    """adapter outputs of a batch: seeded normal rows of uneven length"""
    rng = np.random.default_rng(1000 * B + D)
    return (rng.standard_normal((B, D)) * rng.uniform(0.5, 2.0, (B, 1))).astype(np.float32)


def make_labels(B, k, seed):
    """k labels shared by B - 1 rows in turn plus one row with a label of its own, shuffled; arbitrary integer values"""
    rng = np.random.default_rng(seed)
    values = rng.choice(np.arange(-50, 50), size=k + 1, replace=False).astype(np.int64)
    y = np.concatenate([[values[k]], values[np.arange(B - 1) % k]])
    return y[rng.permutation(B)]


def check_labels(y):
    same = (y[:, None] == y[None, :]) & ~np.eye(len(y), dtype=bool)
    n_pos, n_neg = same.sum(1), len(y) - 1 - same.sum(1)
    assert (n_pos == 0).sum() == 1, "exactly one row without positives"
    assert (n_neg[n_pos > 0] >= 1).all() and (n_pos[n_pos > 0] >= 1).all(), "every anchor needs a positive and a negative"
    return n_pos


def reference_class():
    """the reference's SupervisedContrastiveLoss, compiled from its file"""
    tree = ast.parse(open(SRC).read(), SRC)
    defs = [n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == "SupervisedContrastiveLoss"]
    assert len(defs) == 1, "the reference's SupervisedContrastiveLoss moved"
    ns = {"torch": torch, "nn": torch.nn}
    exec(compile(ast.Module(body=defs, type_ignores=[]), SRC, "exec"), ns)
    return ns["SupervisedContrastiveLoss"]


class _RowNormalise:
    """forward_ca of the reference's CustomCLIP (commented out there) with the adapter already applied"""
    @staticmethod
    def forward_ca(features):
        return features / features.norm(dim=-1, keepdim=True)


def run_case(Loss, z32, y, tau):
    z = torch.tensor(z32, dtype=torch.float64, requires_grad=True)
    n_pos = check_labels(y)
    rows = torch.zeros(len(y), dtype=torch.float64)
    total = 0.0
    for i in np.flatnonzero(n_pos > 0):
        pos = np.flatnonzero((y == y[i]) & (np.arange(len(y)) != i))
        neg = np.flatnonzero(y != y[i])
        args = SimpleNamespace(cl_temperature=tau, num_positive=len(pos), num_negative=len(neg), tl_method="contrastive_adapter")
        loss = Loss(args)(_RowNormalise, z[np.concatenate([[i], pos, neg])])[0]
        rows[i] = loss.detach()
        total = total + loss
    mean = total / int((n_pos > 0).sum())
    mean.backward()
    return rows.numpy(), float(mean.detach()), z.grad.numpy()


def main():
    Loss = reference_class()
    out = {}
    for B, D in SHAPES:
        z = make_z(B, D)
        out[f"z_b{B}_d{D}"] = z
        for tau in TAUS:
            for k in N_LABELS:
                y = make_labels(B, k, seed=100 * B + k)
                rows, mean, dz = run_case(Loss, z, y, tau)
                c = case_name(B, D, tau, k)
                out[c + "/labels"], out[c + "/tau"] = y, np.float64(tau)
                out[c + "/loss_rows"], out[c + "/mean"], out[c + "/dz"] = rows, np.float64(mean), dz[:, ::DZ_STRIDE[B]].copy()
                print(f"{c}: L_con = {mean:.6f}, max |dz| = {np.abs(dz).max():.3e}")
    np.savez(OUT, **out)
    print(f"wrote {OUT}: {os.path.getsize(OUT)} bytes")


if __name__ == "__main__":
    main()
