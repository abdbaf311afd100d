"""Anchor sets of the contrastive adapter (Zhang & Re 2022, "Contrastive Adapters for Foundation Model Group Robustness"): the host
side of the reference's dead contrastive path (demo/visualizer_supcon.py:1100-1484) on arrays.

The method needs no group labels.  Its anchors are the rows CLIP's zero-shot prediction got wrong; per anchor it draws positives of
the anchor's class that zero-shot got right, and negatives of the other class: the correctly predicted rows that share the anchor's
zero-shot prediction, followed by the other slice's failures (the reference's "easy negatives").  A slice is the set of rows with
one predicted label.

    slices, correct = zero_shot_slices(y, y_pred)
    points = contrastive_points(y, confounder, slices, correct)
    batches = contrastive_batches(points, num_anchor, num_positive, num_negative)      # per slice [n_anchors, A + P + N] int64
    order = contrastive_order(batches)                                                 # [n_sets, A + P + N]

Every draw comes from the global numpy stream with the reference's own calls in the reference's order, so the same seed gives the
reference's index matrices.  Two classes and two slices, like the reference's `abs(slice_ix - 1)`.  Unlike the reference, slices of
unequal size work: its `np.array(sliced_data_incorrect)` (:1162) builds a ragged array, which numpy >= 1.24 refuses.
"""
from collections import namedtuple

import numpy as np

# anchors[s] / negatives[s]: dicts of arrays per slice ('ix' the row indices, 'target', 'source' the slice a row came from,
# 'spurious'; anchors also 'ix_by_class' {class: row indices}); positives_by_class {class: dict with 'ix', 'target', 'source',
# 'spurious'}
ContrastivePoints = namedtuple("ContrastivePoints", "anchors negatives positives_by_class")


def zero_shot_slices(y, y_pred):
    """compute_slice_indices (:1126-1145) on arrays: (one index array per predicted label in np.unique order, per slice the
    `y_pred == y` flags of its rows)"""
    y, y_pred = np.asarray(y), np.asarray(y_pred)
    if y.shape != y_pred.shape or y.ndim != 1:
        raise ValueError(f"zero_shot_slices: y {y.shape} and y_pred {y_pred.shape} must be vectors of one length")
    correct = y_pred == y
    slices = [np.where(y_pred == label)[0] for label in np.unique(y_pred)]
    return slices, [correct[s] for s in slices]


def contrastive_points(y, confounder, slices, correct):
    """prepare_contrastive_points (:1181-1300) on arrays: the anchors per slice (the slice's zero-shot failures, also by class), the
    negatives per slice (the slice's correct rows, then the OTHER slice's failures) and the positives by class (the correct rows of
    class c from every slice, in slice order).  Raises ValueError unless there are exactly two slices, and when a class that has
    anchors has no positives."""
    y, confounder = np.asarray(y), np.asarray(confounder)
    if len(slices) != 2 or len(correct) != 2:
        raise ValueError(f"contrastive_points: two zero-shot slices expected (two predicted labels), got {len(slices)}")
    anchors, negatives, positives = [], [], {}
    for s, (rows, ok) in enumerate(zip(slices, correct)):
        rows, ok = np.asarray(rows), np.asarray(ok, dtype=bool)
        wrong, right = rows[~ok], rows[ok]                                 # boolean masks keep the slice's row order, like np.where / np.setdiff1d
        anchors.append({"ix": wrong, "target": y[wrong], "source": np.full(len(wrong), s, dtype=int), "spurious": confounder[wrong],
                        "ix_by_class": {c: wrong[y[wrong] == c] for c in np.unique(y[wrong])}})
        negatives.append({"ix": right, "target": y[right], "source": np.full(len(right), s, dtype=int), "spurious": confounder[right]})
        for c in np.unique(y[right]):
            pos = right[y[right] == c]
            new = {"ix": pos, "target": y[pos], "source": np.full(len(pos), s, dtype=int), "spurious": confounder[pos]}
            positives[c] = new if c not in positives else {k: np.concatenate([positives[c][k], v]) for k, v in new.items()}
    for s in range(2):                                                     # the easy negatives: the other slice's failures
        other = abs(s - 1)
        negatives[other] = {k: np.concatenate([negatives[other][k], anchors[s][k]]) for k in negatives[other]}
    for s in range(2):
        for c in anchors[s]["ix_by_class"]:
            if c not in positives or not len(positives[c]["ix"]):
                raise ValueError(f"contrastive_points: class {c} has anchors in slice {s} but no correctly predicted row to draw positives from")
        if len(anchors[s]["ix"]) and not len(negatives[s]["ix"]):
            raise ValueError(f"contrastive_points: slice {s} has anchors but no negatives")
    return ContrastivePoints(anchors, negatives, positives)


def _choice(pool, num_samples):
    return np.random.choice(pool, size=num_samples, replace=num_samples > len(pool), p=None)


def contrastive_batches(points, num_anchor, num_positive, num_negative):
    """construct_contrastive_data (:1342-1435): per slice an int64 matrix [n_anchors of the slice, num_anchor + P + N] of row
    indices [anchor, extra anchors; positives; negatives].  Per anchor, in this order, np.random.choice draws the num_anchor - 1
    extra anchors of its class, the positives of its class, the negatives of its slice (with replacement exactly when the pool is
    smaller than the draw); then one np.random.shuffle of the slice's rows.  All from the global numpy stream."""
    if num_anchor < 1 or num_positive < 1 or num_negative < 1:
        raise ValueError("contrastive_batches: num_anchor, num_positive and num_negative must be at least 1")
    out = []
    for s, anchor in enumerate(points.anchors):
        rows = []
        for aix, anchor_ix in enumerate(anchor["ix"]):
            c = anchor["target"][aix]
            extra = _choice(anchor["ix_by_class"][c], num_anchor - 1)
            pos = points.positives_by_class[c]
            pos_ix = pos["ix"][_choice(np.arange(len(pos["ix"])), num_positive)]
            neg_ix = _choice(points.negatives[s]["ix"], num_negative)
            rows.append(np.concatenate([[anchor_ix], extra, pos_ix, neg_ix]))
        np.random.shuffle(rows)                                            # the reference shuffles the LIST of rows
        S = num_anchor + num_positive + num_negative
        out.append(np.array(rows, dtype=np.int64).reshape(len(rows), S))
    return out


def contrastive_order(batches, balance_by_zs_pred=False, re_shuffle=True, maintain_alternative_ordering=False):
    """The ordering statements of load_contrastive_loader (:1448-1468): [n_sets, S] int64.  Without `balance_by_zs_pred` the slices'
    sets are concatenated and, with `re_shuffle`, shuffled.  With it, every slice is shuffled first (`re_shuffle`), the slices are
    zipped -- the longer one is cut to the shorter one's length, the sets alternate between the slices -- and, with `re_shuffle`
    and without `maintain_alternative_ordering`, shuffled again.  Draws from the global numpy stream."""
    batches = [np.asarray(b) for b in batches]
    if balance_by_zs_pred:
        if re_shuffle:
            for b in batches:
                np.random.shuffle(b)
        n = min(len(b) for b in batches)
        out = np.stack([b[:n] for b in batches], axis=1)
        out = out.reshape(-1, out.shape[-1])
        if not maintain_alternative_ordering and re_shuffle:
            np.random.shuffle(out)
    else:
        out = np.concatenate(batches)
        if re_shuffle:
            np.random.shuffle(out)
    return np.ascontiguousarray(out, dtype=np.int64)
