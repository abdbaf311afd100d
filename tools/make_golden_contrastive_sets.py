"""Generate tests/golden/contrastive_sets.npz from the REFERENCE's own contrastive-adapter statements (demo/visualizer_supcon.py).

Same method as tools/make_golden_supcon.py: nothing of the reference is copied.  Its module cannot be imported here, so the
definitions of prepare_contrastive_points, construct_contrastive_data and SupervisedContrastiveLoss are compiled from the file in
place (needs the reference tree, read-only) and run unmodified on the CPU; only numbers are saved.

Sampler cases: seeded synthetic (y, confounder, y_pred) triples whose two zero-shot slices have the SAME size -- the reference's
`np.array(sliced_data_incorrect)` builds a ragged array otherwise, which numpy >= 1.24 refuses; asserted here.  The slices are the
statements of compute_slice_indices on arrays (np.unique / np.where; that function itself reads a pandas frame).  After
np.random.seed(k) the reference builds the points and the two index matrices; one np.random.random() drawn afterwards records where
it leaves the stream.  One case draws more negatives than its pool holds (replace=True), one has num_anchor = 2.

Head cases: explicit sets [anchor; P positives; N negatives] of seeded rows of uneven length, two sets per case; the reference
class scores one set per call through `model.forward_ca` ("adapter, then row-normalise"; commented out in its CustomCLIP), so the
model handed to it row-normalises and the rows are the adapter outputs z.  Saved: z (float32), the class's float64 loss per set and
the autograd gradient of every set's loss with respect to its own rows.

    python tools/make_golden_contrastive_sets.py
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
OUT = os.path.join(ROOT, "tests", "golden", "contrastive_sets.npz")
# (rows, data seed, numpy seed, num_anchor, num_positive, num_negative)
SAMPLER_CASES = ((140, 11, 3, 1, 4, 80), (400, 12, 7, 2, 6, 9))
# (D, P, N)
HEAD_SHAPES = ((64, 1, 1), (64, 5, 7), (128, 3, 40))
TAUS = (0.1, 0.05)
HEAD_SETS = 2


def reference_defs():
    """the reference's two sampler functions and its loss class, compiled from its file"""
    tree = ast.parse(open(SRC).read(), SRC)
    want = ("prepare_contrastive_points", "construct_contrastive_data", "SupervisedContrastiveLoss")
    defs = [n for n in tree.body if isinstance(n, (ast.FunctionDef, ast.ClassDef)) and n.name in want]
    assert sorted(n.name for n in defs) == sorted(want), "the reference's contrastive definitions moved"
    ns = {"np": np, "torch": torch, "nn": torch.nn, "tqdm": lambda it, **k: it, "print": lambda *a, **k: None}
    exec(compile(ast.Module(body=defs, type_ignores=[]), SRC, "exec"), ns)
    return [ns[n] for n in want]


def make_triple(n, seed):
    """(y, confounder, y_pred): half the rows predicted 0 and half 1 (equal slices), about a fifth of each slice predicted wrong"""
    rng = np.random.default_rng(seed)
    y_pred = rng.permutation(np.arange(n) % 2).astype(np.int64)
    wrong = rng.random(n) < 0.2
    y = np.where(wrong, 1 - y_pred, y_pred).astype(np.int64)
    confounder = rng.integers(0, 2, n).astype(np.int64)
    return y, confounder, y_pred


def slices_of(y, y_pred):
    """compute_slice_indices' statements (:1132-1145) on arrays"""
    correct = y_pred == y
    groups = [np.where(y_pred == label)[0] for label in np.unique(y_pred)]
    return groups, [correct[g] for g in groups]


class _RowNormalise:
    """forward_ca of the reference's CustomCLIP (commented out there) with the adapter already applied"""
    @staticmethod
    def forward_ca(features):
        return features / features.norm(dim=-1, keepdim=True)


def make_z(D, P, N):
    rng = np.random.default_rng(7000 + 100 * D + 10 * P + N)
    S = 1 + P + N
    return (rng.standard_normal((HEAD_SETS, S, D)) * rng.uniform(0.5, 2.0, (HEAD_SETS, S, 1))).astype(np.float32)


def main():
    prepare, construct, Loss = reference_defs()
    out = {}
    for k, (n, data_seed, seed, A, P, N) in enumerate(SAMPLER_CASES):
        y, c, y_pred = make_triple(n, data_seed)
        slices, correct = slices_of(y, y_pred)
        assert len(slices) == 2 and len(slices[0]) == len(slices[1]), "the reference needs two slices of equal size"
        assert all((~ok).sum() >= 2 and ok.sum() >= 2 for ok in correct)
        np.random.seed(seed)
        anchors, negatives, positives, _ = prepare(SimpleNamespace(y_array=y, confounder_array=c), slices, correct)
        args = SimpleNamespace(n_cls=2, num_anchor=A, num_positive=P, num_negative=N)
        batches = construct(anchors, negatives, positives, args)
        after = np.random.random()
        pools = [len(neg["ix"]) for neg in negatives]
        assert k != 0 or N > max(pools), "the first case draws with replacement"
        out[f"sampler{k}/y"], out[f"sampler{k}/confounder"], out[f"sampler{k}/y_pred"] = y, c, y_pred
        out[f"sampler{k}/params"] = np.array([seed, A, P, N], dtype=np.int64)
        for s, b in enumerate(batches):
            out[f"sampler{k}/batch{s}"] = np.array(b, dtype=np.int64)
        out[f"sampler{k}/after"] = np.float64(after)
        print(f"sampler{k}: {n} rows, anchors {[len(b) for b in batches]}, negative pools {pools}, N = {N}")
    for D, P, N in HEAD_SHAPES:
        z32 = make_z(D, P, N)
        out[f"head_d{D}_p{P}_n{N}/z"] = z32
        for tau in TAUS:
            args = SimpleNamespace(cl_temperature=tau, num_positive=P, num_negative=N, tl_method="contrastive_adapter")
            losses, grads = [], []
            for t in range(HEAD_SETS):
                z = torch.tensor(z32[t], dtype=torch.float64, requires_grad=True)
                loss = Loss(args)(_RowNormalise, z)[0]
                loss.backward()
                losses.append(float(loss.detach()))
                grads.append(z.grad.numpy())
            name = f"head_d{D}_p{P}_n{N}/t{tau}"
            out[name + "/loss"], out[name + "/dz"] = np.array(losses), np.stack(grads)
            print(f"{name}: l = {losses}")
    np.savez(OUT, **out)
    print(f"wrote {OUT}: {os.path.getsize(OUT)} bytes")


if __name__ == "__main__":
    main()
