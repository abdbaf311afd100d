"""Device-resident stage-2 data path: the adapter training /
validation loops of the reference (final_main.py:426-496, 571-653, 655-719) without its host
bottlenecks.

Reference loop per step: DataLoader workers do pandas column lookups per item
(data/celeba_embeddings_reg.py:63-84), `.cuda()` copies, `loss.item()`, and `update_dict` pulls
`g` to the host and loops over `np.unique` (final_main.py:383-391).  Here the whole embedding
table lives in HBM, a batch is one row-gather kernel, the step body is one C call
(`classifier.train_step`), the group counters stay on the device, and the host synchronises once
per epoch.  Batch composition follows the reference exactly: `dataloader_shuffle_order`
reproduces `DataLoader(shuffle=True)`'s index stream from the global torch RNG, and
adapter's balance_val draw the per-epoch group balancing from the global numpy RNG.
"""
import os
import time
from collections import namedtuple
from copy import copy, deepcopy
from functools import partial

import numpy as np
import torch

from . import adapter, contrastive, dfr, ops
from . import optim as O

NEW_ORDER_FOR_PRINT = ["weighted_mean_acc", "worst_acc", "acc_0_0", "acc_0_1", "acc_1_0", "acc_1_1", "mean_acc"]


class EmbeddingTable:
    """[N, D] fp32 embeddings + int64 labels resident on one device.

    Mirrors the attributes the reference datasets expose (data/celeba_embeddings_reg.py:40-57):
    n_classes, n_groups, n_places, group_array, group_counts, group_ratio."""

    def __init__(self, embeddings, y, confounder, y_pred=None, filenames=None, device="cuda"):
        y_np, c_np, g_np = adapter.group_index(np.asarray(y), np.asarray(confounder))
        self.device = torch.device(device)
        self.embeddings = torch.as_tensor(embeddings, dtype=torch.float32).contiguous().to(self.device)
        self.targets = torch.from_numpy(y_np).to(self.device)
        self.targets_spurious = torch.from_numpy(c_np).to(self.device)
        self.targets_group = torch.from_numpy(g_np).to(self.device)
        self.y_pred = None if y_pred is None else torch.as_tensor(np.asarray(y_pred), dtype=torch.int64).to(self.device)
        self.filenames = filenames
        self.group_array = g_np
        self.n_classes, self.n_groups, self.n_places = 2, 4, 2
        self.group_counts = (torch.arange(self.n_groups).unsqueeze(1) == torch.from_numpy(g_np)).sum(1).float()
        self.group_ratio = self.group_counts / len(self)

    def __len__(self):
        return self.embeddings.shape[0]

    def labels(self, target):
        return {"class": self.targets, "group": self.targets_group, "spurious": self.targets_spurious}[target]

    def batch(self, idx, target="class"):
        """(embeddings[idx], labels[idx], groups[idx]) -- idx int64 on the table's device"""
        return ops.gather_rows(self.embeddings, idx), self.labels(target)[idx], self.targets_group[idx]


def dataloader_shuffle_order(n):
    """Index order of one `DataLoader(dataset, shuffle=True)` epoch, drawn from the global torch
    RNG like torch.utils.data does: one int64 for the iterator's base seed, one for the
    RandomSampler's generator seed, then randperm with that generator."""
    _loader_base_seed()
    seed = int(torch.empty((), dtype=torch.int64).random_().item())   # RandomSampler.__iter__
    g = torch.Generator()
    g.manual_seed(seed)
    return torch.randperm(n, generator=g)


def _loader_base_seed():
    """every DataLoader iterator draws its base seed (_BaseDataLoaderIter._base_seed), shuffled or not: a pass over a loader
    advances the global torch RNG like the reference's loops do"""
    torch.empty((), dtype=torch.int64).random_()


def weighted_sampler_order(weights):
    """Index order of one `DataLoader(dataset, sampler=WeightedRandomSampler(weights, len(weights), replacement=True))` epoch, drawn
    from the global torch RNG like torch.utils.data does: the iterator's base seed, then torch.multinomial over the float64 weights
    (WeightedRandomSampler.__iter__ with no generator of its own)."""
    w = torch.as_tensor(np.asarray(weights, dtype=np.float64), dtype=torch.double)
    _loader_base_seed()
    return torch.multinomial(w, len(w), True)


def failure_weights(y, wrong, correct_class_bias=True, reweighting_by_class=False):
    """The reference's GetResampledWeightsCE (demo/visualizer_supcon.py:1642-1703) restated: float64 [N] sampling weights that
    up-sample, per class, the rows predicted wrong (`wrong` bool [N]; its "negatives") to the number predicted right (its
    "positives") -- weight n_right / n_wrong on the wrong rows of a class unless it has more wrong than right rows --, then correct
    the class imbalance the up-sampling introduced: with imbal = n_major / n_minor and reweighted = right_major / right_minor, the
    minority class's rows are multiplied by reweighted / imbal when imbal < reweighted (`correct_class_bias`), or by reweighted itself
    (`reweighting_by_class`, whatever the comparison says).  The defaults are what final_main.py:870-871 sets.  Two departures, where
    the reference divides by zero: a class without wrong rows keeps weight 1, and the correction is skipped when a class has no
    right rows.  Binary labels {0, 1} with both classes present, else ValueError."""
    y = np.asarray(y).astype(np.int64).ravel()
    wrong = np.asarray(wrong).astype(bool).ravel()
    if y.shape != wrong.shape:
        raise ValueError(f"failure_weights: {y.shape[0]} labels for {wrong.shape[0]} flags")
    if not np.array_equal(np.unique(y), [0, 1]):
        raise ValueError(f"failure_weights covers two classes (labels 0 and 1, both present), got {np.unique(y).tolist()}")
    weights = np.ones(len(y))
    num_cls, num_pos = {}, {}
    for c in (0, 1):
        n_pos, n_neg = int((~wrong & (y == c)).sum()), int((wrong & (y == c)).sum())
        num_cls[c], num_pos[c] = n_pos + n_neg, n_pos
        if n_neg and n_pos >= n_neg:
            weights[wrong & (y == c)] = n_pos / n_neg
    if (correct_class_bias or reweighting_by_class) and num_pos[0] and num_pos[1]:
        major, minor = (1, 0) if num_cls[0] < num_cls[1] else (0, 1)
        imbal = num_cls[major] / num_cls[minor]
        reweighted = num_pos[major] / num_pos[minor]
        if reweighting_by_class:
            weights[y == minor] = weights[y == minor] * (reweighted / 1)
        elif imbal < reweighted:
            weights[y == minor] = weights[y == minor] * (reweighted / imbal)
    return weights


def jtt_weights(wrong, lambda_up):
    """JTT's second-stage weights (Liu et al. 2021): `lambda_up` on the rows of the error set, 1 elsewhere; float64 [N]"""
    return np.where(np.asarray(wrong).astype(bool).ravel(), float(lambda_up), 1.0)


def zero_shot_failures(table, text_embedding_dir, temperature):
    """bool [N] (numpy): the rows of `table` CLIP's zero-shot prediction gets wrong -- `table.y_pred != targets` when the table
    carries y_pred, else the argmax of the fused kernel's logits of the raw embeddings against the class prompts"""
    if table.y_pred is not None:
        return (table.y_pred != table.targets).cpu().numpy()
    tn = ops.text_colnorm(adapter.get_text_embedding(text_embedding_dir).to(table.device).float().contiguous())
    pred = ops.l2norm_sim_ce_fwd(table.embeddings, tn, temperature, want_loss=False, want_pred=True)[3]
    return (pred != table.targets).cpu().numpy()


def normalise_row_weights(weights, n_rows, replicas=1):
    """given per-row weights -> float64 [Rw, n_rows] of mean 1 per row of weights (w * N / sum(w), on the host), Rw = 1 or `replicas`.
    Non-finite, negative, all-zero weights or a wrong shape raise ValueError."""
    w = np.asarray(weights, dtype=np.float64)
    if w.ndim == 1:
        w = w[None]
    if w.ndim != 2 or w.shape[1] != n_rows or w.shape[0] not in (1, replicas):
        want = f"[{n_rows}]" if replicas == 1 else f"[{n_rows}] or [{replicas}, {n_rows}]"
        raise ValueError(f"row_weights: {want} weights over the train table expected, got shape {np.shape(weights)}")
    if not np.isfinite(w).all():
        raise ValueError("row_weights: non-finite weights")
    if (w < 0).any():
        raise ValueError("row_weights: negative weights")
    tot = w.sum(axis=1, keepdims=True)
    if (tot <= 0).any():
        raise ValueError("row_weights: all weights are zero")
    return w * n_rows / tot


class _RowWeights:
    """the schedule's per-row weights over the train table: `mode` "loss" / "sample", `host` float64 [Rw, N] of mean 1, and -- once
    `upload`ed, in "loss" mode -- `dev` float32 [Rw, N] on the table's device"""

    def __init__(self, mode, host):
        self.mode, self.host, self.dev = mode, host, None

    def upload(self, device):
        if self.mode == "loss":
            self.dev = torch.from_numpy(self.host.astype(np.float32)).contiguous().to(device)
        return self

    def of(self, r):
        """replica r's float64 weights"""
        return self.host[r if self.host.shape[0] > 1 else 0]


def _row_weight_option(opt, n_train, replicas=1, zs_failures=None):
    """opt.row_weights / opt.row_weight_mode (read with getattr) as a _RowWeights over a train table of `n_train` rows, or None when
    off.  Runs on the host: `zs_failures()` -> (y, wrong) is only called for the string "zs_failures".  Raises DbmmUnsupported beside
    opt.robust / opt.contrastive_weight and ValueError for a bad mode or bad weights; opt.resample_ce plays no part (a no-op, as in
    the reference)."""
    given = getattr(opt, "row_weights", None)
    if given is None:
        return None
    mode = getattr(opt, "row_weight_mode", "loss") or "loss"
    if mode not in ("loss", "sample"):
        raise ValueError(f"row_weight_mode must be 'loss' or 'sample', got {mode!r}")
    if bool(getattr(opt, "robust", False)):
        raise ops.DbmmUnsupported("opt.row_weights and opt.robust do not combine: the group-DRO head has no per-row weighted form")
    if _contrastive_option(opt) is not None:
        raise ops.DbmmUnsupported("opt.row_weights and opt.contrastive_weight do not combine: the contrastive head has no per-row weighted form")
    if isinstance(given, str):
        if given != "zs_failures":
            raise ValueError(f"row_weights must be None, 'zs_failures' or an array over the train table, got {given!r}")
        if zs_failures is None:
            raise ValueError("row_weights='zs_failures' needs the train table")
        given = failure_weights(*zs_failures())
    return _RowWeights(mode, normalise_row_weights(given, n_train, replicas))


def _epoch_order(n, shuffle, indices):
    """row order of one loader pass over `indices` (n of them; None: rows 0 .. n-1), int64"""
    if shuffle:
        order = dataloader_shuffle_order(n)
    else:
        _loader_base_seed()
        order = torch.arange(n)
    if indices is not None:
        order = torch.as_tensor(np.asarray(indices), dtype=torch.int64)[order]
    return order


def _epoch_batches(n, batch_size, shuffle, indices):
    order = _epoch_order(n, shuffle, indices)
    return [order[i:i + batch_size] for i in range(0, n, batch_size)]


def _scores(table, c, loss_sum, n, ratio=None):
    """(loss average, accuracy, rounded group-accuracy dict) of one pass from its integer (n, correct) counters [G, 2] and its loss
    sum over n rows: get_results (final_main.py:395-406).  With `ratio`, the train split's group ratio, the evaluation form: the
    ratio-weighted mean as well."""
    meters = {}
    for g in range(c.shape[0]):
        meters[g] = adapter.AverageMeter()
        if c[g, 0]:
            meters[g].update(int(c[g, 1]) / int(c[g, 0]), int(c[g, 0]))
    res = adapter.get_results(meters, partial(adapter.get_y_p, n_places=table.n_places))
    keys = NEW_ORDER_FOR_PRINT[1:]
    if ratio is not None:
        indiv = [res[f"acc_{g // table.n_places}_{g % table.n_places}"] for g in range(table.n_groups)]
        res["weighted_mean_acc"] = (np.array(indiv) * np.array(ratio)).sum()
        keys = NEW_ORDER_FOR_PRINT
    return loss_sum / n, int(c[:, 1].sum()) / int(c[:, 0].sum()), {k: np.round(res[k], 4) for k in keys}


# One loader pass of an epoch, as the schedule describes it to an executor.  `rows`: per replica the row subset of `table` the pass
# runs over (None: the whole table); `counted`: the pass adds to the epoch's loss sum and group counters.
# `weights`: a _RowWeights over `table` (train-table passes of a schedule with opt.row_weights), else None.
_Pass = namedtuple("_Pass", "table rows shuffle batch_size use_group counted weights", defaults=(None,))


def _pass_rows(p, r=0):
    return len(p.table) if p.rows is None else len(p.rows[r])


def _contrastive_option(opt):
    """(weight, temperature) of opt.contrastive_weight / opt.cl_temperature (the reference's option names; read with getattr, default
    0 = off and 0.1), or None when the weight is 0"""
    weight = float(getattr(opt, "contrastive_weight", 0) or 0)
    return (weight, float(getattr(opt, "cl_temperature", 0.1))) if weight > 0 else None


def _train_passes(classifier, optimizer, target, passes, lr_hook, robust=None, q_log=None, contrastive=None, con_log=None):
    """The loader passes of one epoch of one run, on one pair of device accumulators with ONE host sync at the end.
    `lr_hook(step, n_steps)` runs before every step and restarts with each pass.  Returns (counters [G, 2] numpy, loss sum, the
    epoch's row order).  `robust` (an adapter.GroupDRO state): every step is a group-DRO step over the table's group ids -- also on
    the group-prompt passes --, the loss summed is the robust loss; `q_log` (a list) receives q after each pass.  `contrastive` = (weight,
    temperature): every step is the mixed step (CustomCLIP.train_step(contrastive=)) under the labels its CE uses, the loss summed is
    the mixed loss; `con_log` (a list) receives the sum of L_con x rows over the counted passes.  A pass with `weights` (whole-table
    passes only): in "loss" mode every step is the weighted step under the weights of its rows and the loss summed is L * B; in
    "sample" mode the row order is weighted_sampler_order's draw and the steps are plain."""
    classifier.train()
    dev = passes[0].table.device
    counts = torch.zeros((passes[0].table.n_groups, 2), dtype=torch.int64, device=dev)
    loss_sum = torch.zeros((), dtype=torch.float64, device=dev)
    con_sum = torch.zeros((), dtype=torch.float64, device=dev) if contrastive is not None else None
    order, qs = [], []
    for p in passes:
        wdev = None
        if p.weights is not None and p.weights.mode == "sample":
            drawn = weighted_sampler_order(p.weights.of(0))
            batches = [drawn[i:i + p.batch_size] for i in range(0, len(drawn), p.batch_size)]
        else:
            batches = _epoch_batches(_pass_rows(p), p.batch_size, p.shuffle, None if p.rows is None else p.rows[0])
            if p.weights is not None:
                wdev = p.weights.dev[0]
        for step, idx in enumerate(batches):
            idx = idx.to(dev, non_blocking=True)
            emb, labels, groups = p.table.batch(idx, target)
            if p.use_group:
                labels = groups
            if lr_hook is not None:
                lr_hook(step, len(batches))
            if robust is not None:
                loss, logits, _ = classifier.train_step(emb, labels, optimizer, p.use_group, robust=(robust, groups))
            elif contrastive is not None:
                loss, logits, _, con = classifier.train_step(emb, labels, optimizer, p.use_group, contrastive=contrastive)
                if p.counted:
                    con_sum += con.double() * idx.numel()
            elif wdev is not None:
                loss, logits, _ = classifier.train_step(emb, labels, optimizer, p.use_group, row_weights=wdev[idx])
            else:
                loss, logits, _ = classifier.train_step(emb, labels, optimizer, p.use_group)
            if p.counted:
                loss_sum += loss.double() * idx.numel()                  # losses.update(loss.item(), bsz)
                adapter.group_counts(logits, labels, groups, p.table.n_groups, counts)
        order += batches
        if robust is not None:
            qs.append(robust.q.clone())
    c = counts.cpu().numpy()
    if q_log is not None:
        q_log.extend(q.cpu().numpy() for q in qs)
    if con_log is not None and con_sum is not None:
        con_log.append(con_sum.item())
    return c, loss_sum.item(), torch.cat(order).numpy()


def train_epoch(table, classifier, optimizer, batch_size, target="class", use_group=False, indices=None,
                shuffle=True, lr_hook=None, stats=None, robust=None):
    """One epoch of train_one_epoch / train_reg_seq_one_epoch.  `indices` restricts the epoch to a
    subset (reg split, balanced indices); `lr_hook(step, n_steps)` runs before every step (the
    warm-up helpers).  Returns (loss average, accuracy, group accuracy dict) like the reference,
    computed from device-side accumulators with ONE host sync at the end.  `stats` (a dict) receives
    the integer (n, correct) counters [G, 2] and the row order of the epoch.  `robust`: an adapter.GroupDRO state -- the epoch
    takes group-DRO steps and the loss average is that of the robust loss."""
    p = _Pass(table, None if indices is None else [indices], shuffle, batch_size, use_group, True)
    c, loss_sum, order = _train_passes(classifier, optimizer, target, [p], lr_hook, robust)
    if stats is not None:
        stats.update(counts=c, order=order)
    return _scores(table, c, loss_sum, _pass_rows(p))


def train_reg_epoch(train_table, reg_table, classifier, optimizer, batch_size, reg_rows, reg_batch_size, reg_shuffle, target="class",
                    group_prompt=True, lr_hook=None, stats=None):
    """One epoch of train_reg_one_epoch (final_main.py:498-569): the shuffled train split on the class prompts, then -- same
    optimiser, same epoch -- the reg loader (`reg_rows` of `reg_table`, shuffled or not), on the group prompts with group labels
    when `group_prompt`.  `lr_hook(step, n_steps)` restarts with each loader like the reference's warmup_learning_rate(opt, epoch,
    idx, len(dataloader)).  Loss, accuracy and group counters accumulate over the batches scored on the class prompts only (the
    train loader, and the reg loader when not `group_prompt`); one host sync per epoch.  `stats` receives the counters, the row
    order (train rows, then the reg loop's rows) and the number of train rows."""
    passes = [_Pass(train_table, None, True, batch_size, False, True),
              _Pass(reg_table, [reg_rows], reg_shuffle, reg_batch_size, group_prompt, not group_prompt)]
    c, loss_sum, order = _train_passes(classifier, optimizer, target, passes, lr_hook)
    if stats is not None:
        stats.update(counts=c, order=order, n_train_rows=len(train_table))
    return _scores(train_table, c, loss_sum, sum(_pass_rows(p) for p in passes if p.counted))


@torch.no_grad()
def _eval_pass(table, batch_size, target, indices, score):
    """one un-shuffled loader pass in large batches: `score(emb, labels)` -> (logits, per-row CE).  Returns (counters [G, 2] numpy,
    loss sum)"""
    n = len(table) if indices is None else len(indices)
    dev = table.device
    counts = torch.zeros((table.n_groups, 2), dtype=torch.int64, device=dev)
    loss_sum = torch.zeros((), dtype=torch.float64, device=dev)
    for idx in _epoch_batches(n, batch_size, False, indices):
        idx = idx.to(dev, non_blocking=True)
        emb, labels, groups = table.batch(idx, target)
        logits, rows = score(emb, labels)
        loss_sum += rows.double().sum()
        adapter.group_counts(logits, labels, groups, table.n_groups, counts)
    return counts.cpu().numpy(), loss_sum.item()


def _validate_counts(table, classifier, batch_size, target, indices, spurious):
    classifier.eval()
    return _eval_pass(table, batch_size, target, indices,
                      lambda emb, labels: classifier.loss(emb, labels, spurious=spurious)[1:])   # fused normalise + logits + CE kernel


def validate(table, classifier, batch_size, train_group_ratio, target="class", indices=None, spurious=False, stats=None):
    """validate / validate_zs (final_main.py:655-803): eval-mode forward, CE, group accuracies and
    the train-ratio-weighted mean.  A LinearClassifier is scored through its own head (LinearClassifier.loss); its
    zero-shot scores are validate_zs's own branch, validate_zs_linear_probing below."""
    c, loss_sum = _validate_counts(table, classifier, batch_size, target, indices, spurious)
    if stats is not None:
        stats.update(counts=c)
    return _scores(table, c, loss_sum, len(table) if indices is None else len(indices), train_group_ratio)


def validate_zs_linear_probing(table, text_embedding_dir, temperature, batch_size, train_group_ratio, target="class", stats=None):
    """validate_zs's `linear_probing` branch (final_main.py:730-761): no classifier -- raw embeddings, row-normalised, against the
    column-normalised prompt matrix / T (the CLIP zero-shot baseline), CE and group accuracies.  One fused launch per batch."""
    tn = ops.text_colnorm(adapter.get_text_embedding(text_embedding_dir).to(table.device).float().contiguous())
    c, loss_sum = _eval_pass(table, batch_size, target, None,
                             lambda emb, labels: ops.l2norm_sim_ce_fwd(emb, tn, temperature, labels=labels)[:2])
    if stats is not None:
        stats.update(counts=c)
    return _scores(table, c, loss_sum, len(table), train_group_ratio)


# ---------------------------------------------------------------------------------------------------------------------
# the training schedule, written once; the two executors of a pass: one run on ordinary modules, R runs in lock-step
# ---------------------------------------------------------------------------------------------------------------------

_METHODS = ("linear_probing", "adapter", "adapter_reg", "adapter_reg_seq", "adapter_reg_seq_alter")


def _run_schedule(ex, opts, train_table, val_table, test_table, input_dim=None, log=None):
    """The training schedule of the reference's driver (final_main.py:805-1046) for the R runs of `opts` (one namespace of the
    reference's parse_option per run; they differ in their learning rates only), every pass executed by `ex` -- _SingleRun: one run
    on ordinary modules; _LockStep: up to 16 runs, every step one replica-batched call.  Whatever is not the execution of a pass is
    stated here, once, so a run of a sweep is scheduled like the run alone by construction:

      linear_probing: set_model's LinearClassifier (:306-308), train_one_epoch on the plain loaders, validated on the WHOLE val
          split; the zero-shot pair is validate_zs's linear_probing branch (the CLIP baseline, independent of the trained head);
      adapter: CustomCLIP(Adapter), train_one_epoch on the train split (:935), lr by adjust_learning_rate + warm-up;
      adapter_reg: every epoch is train_reg_one_epoch (:498-569, called at :924-931): the train split on the class prompts, then
          -- same optimiser; the warm-up's batch index and count restart with each loader -- the reg half of the val split on the
          group prompts with group labels, or on the class prompts and counted under --use_cls_prompt_in_reg;
      adapter_reg_seq, adapter_reg_seq_alter: stage 1 (epoch <= epochs_feature_learning) like `adapter`; switch (epoch == efl + 1):
          restart from the best model so far (--continue_from_best, :941-943), MultipleAdapter over it with a fresh Adapter
          (--add_adapter) and set_optimizer_reg (fresh momentum) (:945-950); stage 2: train_reg_seq_one_epoch on the reg half,
          `_alter`: odd epochs on the class prompts, even epochs on the group prompts (:954-968), warm-up from the stage's own
          epoch count (:607);
      the reg half: re-balanced per epoch by --balance_val from the global numpy RNG (also in stage 1, :920-921) and read by an
          un-shuffled loader with the adjusted batch size, else the reg loader itself (shuffled, batch_size_reg);
      every epoch: validate on the other half of the val split, keep the best worst-group model (strict `>`, :1001-1008), validate
          on the test split (:1013-1016); finally the zero-shot class / spurious scores of the best model (:1037-1045);
      opt.robust (a build-side addition; read with getattr, default off; step size opt.robust_step_size, default 0.01): every training
          step of the adapter methods is a group-DRO step (Sagawa et al. 2020; adapter.GroupDRO) over the table's
          group ids -- also on the group-prompt passes; q is per run, starts at 1 / G, starts over at the switch with the momentum, is
          not part of the best model; a pass counts the robust loss; the train records carry q after each pass; linear_probing raises.
      opt.contrastive_weight > 0 (the reference's option, dead there; read with getattr, default 0 = off; opt.cl_temperature, default
          0.1): every training step of the adapter methods of a single run minimises (1 - weight) * CE + weight * L_con, L_con the
          supervised-contrastive loss of the trainable adapter's output under the labels the pass's CE uses (group ids on a
          group-prompt pass); a pass counts the mixed loss; the train records carry `con`, the row-weighted
          average of L_con; linear_probing, a sweep and opt.robust raise.
      opt.row_weights (a build-side addition; read with getattr, default None = off): per-row weights over the TRAIN table -- an
          array [N] (a sweep also takes [R, N]) or the string "zs_failures" = failure_weights of zero_shot_failures of the train
          table, the reference's dead --resample_ce weights (:868-884).  Rescaled once, on the host in float64, to mean 1 over the
          table, then cast to fp32.  opt.row_weight_mode "loss" (default): every step of a train-table pass minimises (1 / B) sum_b
          w_b CE_b, a pass counts L * B, the group counters stay unweighted; "sample": every train-table pass
          draws weighted_sampler_order (a WeightedRandomSampler loader) in place of the shuffle and takes plain steps.  The reg
          passes on the val half (adapter_reg, stage 2 of the seq methods) stay unweighted.  All methods, single runs and sweeps;
          with opt.robust or opt.contrastive_weight it raises DbmmUnsupported, bad weights raise ValueError, both before a model is
          built.  opt.resample_ce alone stays the no-op it is in the reference.

    Random streams are consumed like the reference does (global torch RNG: parameter initialisation and DataLoader orders; global
    numpy RNG: balance_val) through ex.streams.run(r, ...), so the same seeds give the same initial weights and batches.  Returns per
    run ((best train, best val, best test group-accuracy dicts), (zero-shot class, zero-shot spurious)); `log` (a list) receives one
    list of records per run, one record per initialisation and per train / validate pass."""
    opt, R = opts[0], len(opts)
    method = opt.tl_method
    if method not in _METHODS:
        raise ValueError(f"the training schedule covers linear_probing and the adapter methods, not tl_method={method!r}")
    linear, seq, has_reg = method == "linear_probing", method.startswith("adapter_reg_seq"), method.startswith("adapter_reg")
    robust = bool(getattr(opt, "robust", False))
    if robust and linear:
        raise ops.DbmmUnsupported("group DRO (opt.robust) covers the adapter methods; the linear probe's fused step has no weighted form")
    contrastive = _contrastive_option(opt)
    if contrastive is not None:
        if linear:
            raise ops.DbmmUnsupported("the contrastive term (opt.contrastive_weight) covers the adapter methods; the linear probe has no adapter output")
        if robust:
            raise ops.DbmmUnsupported("opt.contrastive_weight and opt.robust do not combine: the group-DRO head has no contrastive form")
        if not isinstance(ex, _SingleRun):
            raise ops.DbmmUnsupported("the contrastive term (opt.contrastive_weight) covers single runs; the replica-batched step has no contrastive head")
        ex.contrastive = contrastive
    streams = ex.streams
    dev = train_table.device
    row_w = _row_weight_option(opt, len(train_table), R, lambda: (train_table.targets.cpu().numpy(),
                                                                   zero_shot_failures(train_table, opt.text_embedding_dir, opt.zs_temperature)))
    if row_w is not None:
        row_w.upload(dev)
    D = input_dim or train_table.embeddings.shape[1]
    reg_idx = val_idx = None
    if has_reg:                                                           # load_*_embeddings: stratified 50/50 split of the val split
        reg_idx, val_idx = adapter.stratified_split_indices(val_table.group_array, 0.5)
    n_val = len(val_table) if val_idx is None else len(val_idx)
    ratio = train_table.group_ratio.numpy()
    logs = [[] for _ in range(R)]
    rec = (lambda r, **k: logs[r].append(k)) if log is not None else (lambda r, **k: None)

    def each(fn):
        for r in range(R):
            fn(r)

    def new_model():
        if linear:
            return adapter.LinearClassifier(D, opt.n_cls)
        return adapter.CustomCLIP(adapter.Adapter(D, opt.adapter_feat_dim), opt.text_embedding_dir, opt.text_spurious_embedding_dir,
                                  opt.text_group_embedding_dir, temperature=opt.zs_temperature)

    def record_init(r, module):
        rec(r, kind="init", state={k: v.clone() for k, v in module.state_dict().items()})
    models = [streams.run(r, new_model) for r in range(R)]
    each(lambda r: record_init(r, models[r] if linear else models[r].adapter))
    lr1 = ex.start(models, dev)                                           # per run an optimiser, or what optim.py's helpers need of one
    if robust:                                                            # per run a group distribution q = 1 / G; every training step is a group-DRO step
        ex.start_robust(train_table.n_groups, getattr(opt, "robust_step_size", 0.01), dev)
    lr2 = None
    best_acc, best_epoch = [0] * R, [0] * R
    train_accs, val_accs, test_accs = [[] for _ in range(R)], [[] for _ in range(R)], [[] for _ in range(R)]
    # the reference evaluates in batches of batch_size_reg (as few as 4 rows: load_*_embeddings' bs_val); eval-mode scores do not
    # depend on the batch size, so evaluation runs in large batches -- one pass still advances the random stream once, like a loader
    bs_eval = max(opt.batch_size_reg if has_reg else opt.batch_size, 4096)
    efl = getattr(opt, "epochs_feature_learning", None) if seq else None
    for epoch in range(1, opt.epochs + 1):
        each(lambda r: O.adjust_learning_rate(opts[r], lr1[r], epoch))
        balanced = None
        if has_reg and opt.balance_val:                                   # a fresh balanced subset every epoch, also in stage 1
            balanced = [streams.run(r, adapter.balance_val_indices, val_table.group_array[reg_idx], val_table.n_groups, opt.batch_size_reg)
                        for r in range(R)]
        stage2 = seq and epoch > efl
        if stage2 and epoch == efl + 1:
            if opt.continue_from_best:
                ex.restore()
            fresh = None
            if opt.add_adapter:
                fresh = [streams.run(r, adapter.Adapter, D, opt.adapter_feat_dim) for r in range(R)]
                each(lambda r: record_init(r, fresh[r]))
            lr2 = ex.switch(fresh)
            if robust:                                                    # a fresh optimiser: q starts over with the momentum
                ex.dro.reset()
        if stage2:
            each(lambda r: O.adjust_learning_rate_reg(opts[r], lr2[r], epoch))
        lrs, warmup, warm_epoch = (lr2, O.warmup_learning_rate_reg, epoch - efl) if stage2 else (lr1, O.warmup_learning_rate, epoch)
        hook = lambda i, n: each(lambda r: warmup(opts[r], warm_epoch, i, n, lrs[r]))     # restarts with each loader of the epoch
        passes, extra = [], {}
        if not stage2:
            passes.append(_Pass(train_table, None, True, opt.batch_size, False, True, row_w))
        if stage2 or method == "adapter_reg":
            use_group = (epoch % 2) == 0 if method == "adapter_reg_seq_alter" else not opt.use_cls_prompt_in_reg
            if balanced is not None:                                     # DataLoader(balanced_subset, shuffle=False, batch_size=adjusted)
                rows, shuffle, bs = [reg_idx[b] for b, _ in balanced], False, balanced[0][1]
            else:                                                        # the reg loader itself: shuffle=True
                rows, shuffle, bs = [reg_idx] * R, True, opt.batch_size_reg
            passes.append(_Pass(val_table, rows, shuffle, bs, use_group, stage2 or not use_group))
            extra = {"use_group": use_group} if stage2 else {"use_group": use_group, "n_train_rows": len(train_table)}
        kind = "train2" if stage2 else "train_reg" if method == "adapter_reg" else "train1"
        c, ls, orders = ex.train(passes, lrs, hook)
        n_rows = sum(_pass_rows(p) for p in passes if p.counted)
        for r in range(R):
            loss, acc, gacc = _scores(train_table, c[r], ls[r], n_rows)
            if robust:                                                    # q after each pass of the epoch
                extra = dict(extra, q=ex.q_log[r])
            if contrastive is not None:                                   # row-weighted average of L_con over the counted passes
                extra = dict(extra, con=ex.con_log[r] / n_rows)
            rec(r, kind=kind, epoch=epoch, loss=loss, acc=acc, group_acc=gacc, counts=c[r], order=orders[r], **extra)
            train_accs[r].append(gacc)
        vc, vl = ex.evaluate(val_table, bs_eval, opt.train_target, val_idx)
        better = [False] * R
        for r in range(R):
            vloss, vacc, vg = _scores(val_table, vc[r], vl[r], n_val, ratio)
            rec(r, kind="validate", epoch=epoch, split="val", loss=vloss, acc=vacc, group_acc=vg, counts=vc[r])
            val_accs[r].append(vg)
            if vg["worst_acc"] > best_acc[r]:
                best_acc[r], best_epoch[r], better[r] = vg["worst_acc"], epoch, True
        ex.snapshot(better)
        tc, tl = ex.evaluate(test_table, bs_eval, "class", None)
        for r in range(R):
            tloss, tacc, tg = _scores(test_table, tc[r], tl[r], len(test_table), ratio)
            rec(r, kind="validate", epoch=epoch, split="test", loss=tloss, acc=tacc, group_acc=tg, counts=tc[r])
            test_accs[r].append(tg)
    zero_shot = []
    for target, text_dir in (("class", opt.text_embedding_dir), ("spurious", opt.text_spurious_embedding_dir)):
        if linear:
            # validate_zs's linear_probing branch scores the raw embeddings against the prompts: no trained head in it, so one
            # computation serves every run; every run's stream still advances by the loader pass its own run makes
            st = {}
            z = streams.run(0, validate_zs_linear_probing, test_table, text_dir, opt.zs_temperature, bs_eval, ratio, target=target, stats=st)
            for r in range(1, R):
                streams.run(r, _loader_base_seed)
            zero_shot.append([z + (st["counts"],)] * R)
        else:
            cc, ll = ex.evaluate(test_table, bs_eval, target, None, spurious=target == "spurious", best=True)
            zero_shot.append([_scores(test_table, cc[r], ll[r], len(test_table), ratio) + (cc[r],) for r in range(R)])
    out = []
    for r in range(R):
        for target, z in zip(("class", "spurious"), zero_shot):
            rec(r, kind="validate_zs", target=target, loss=z[r][0], acc=z[r][1], group_acc=z[r][2], counts=z[r][3])
        # a linear_probing run whose worst-group accuracy never rose above 0 has best_epoch 0 and no best model; the best model as
        # an ordinary module is only built for a caller who asked for the records
        rec(r, kind="final", best_epoch=best_epoch[r], best_model=ex.best_model(r) if log is not None else None)
        e = best_epoch[r] - 1
        out.append(((train_accs[r][e], val_accs[r][e], test_accs[r][e]), (zero_shot[0][r][2], zero_shot[1][r][2])))
    if log is not None:
        log.extend(logs)
    return out


class _AmbientStreams:
    """the streams of a run that owns the global torch and numpy random streams: draws go straight to them"""
    @staticmethod
    def run(r, fn, *args, **kwargs):
        return fn(*args, **kwargs)


class _SingleRun:
    """Executor of one run on ordinary modules: CustomCLIP / MultipleAdapter / LinearClassifier, the optimisers of optim.py, a
    deepcopy as the best model."""
    streams = _AmbientStreams

    def __init__(self, opt):
        self.opt = opt
        self.model = self.best = self.device = None
        self.dro, self.q_log = None, None                                # group DRO: the run's state (not part of the best model)
        self.contrastive, self.con_log = None, None                      # (weight, temperature) of the contrastive term; sum of L_con x rows

    def start(self, models, device):
        self.model, self.device = models[0].to(device), device
        return [O.set_optimizer(self.opt, self.model)]

    def start_robust(self, n_groups, step_size, device):
        self.dro = adapter.GroupDRO(n_groups, step_size, device)

    def restore(self):
        self.model = deepcopy(self.best)

    def switch(self, fresh):
        if fresh is not None:
            self.model = adapter.MultipleAdapter(self.model, fresh[0], init_near_identity=self.opt.init_near_identity,
                                                 ebd_weight=0.5).to(self.device)
        return [O.set_optimizer_reg(self.opt, self.model)]

    def train(self, passes, optimizers, hook):
        qs, cs = [], []
        c, loss_sum, order = _train_passes(self.model, optimizers[0], self.opt.train_target, passes, hook, self.dro, qs, self.contrastive, cs)
        self.q_log, self.con_log = [qs], cs
        return [c], [loss_sum], [order]

    def evaluate(self, table, batch_size, target, indices, spurious=False, best=False):
        c, loss_sum = _validate_counts(table, self.best if best else self.model, batch_size, target, indices, spurious)
        return [c], [loss_sum]

    def snapshot(self, better):
        if better[0]:
            self.best = deepcopy(self.model)

    def best_model(self, r):
        return self.best


# ---------------------------------------------------------------------------------------------------------------------
# the contrastive adapter (demo/visualizer_supcon.py: train_one_epoch_cl :412-508 inside train_all_epochs :720-772)
# ---------------------------------------------------------------------------------------------------------------------

def _contrastive_sets(opt, table):
    """the anchor sets of a run, built once: zero-shot slices of the train table, contrastive points, batches, order -- [n_sets, A + P +
    N] int64 row indices into `table`; draws from the global numpy stream (contrastive.py)"""
    if table.y_pred is None:
        raise ValueError("train_contrastive_adapter: the train table carries no y_pred (CLIP's zero-shot predictions)")
    y, c = table.targets.cpu().numpy(), table.targets_spurious.cpu().numpy()
    slices, correct = contrastive.zero_shot_slices(y, table.y_pred.cpu().numpy())
    points = contrastive.contrastive_points(y, c, slices, correct)
    batches = contrastive.contrastive_batches(points, int(getattr(opt, "num_anchor", 1)), int(opt.num_positive), int(opt.num_negative))
    return contrastive.contrastive_order(batches, bool(getattr(opt, "balance_by_zs_pred", False)), bool(getattr(opt, "re_shuffle_ca_loader", True)),
                                         bool(getattr(opt, "maintain_alternative_ordering", False)))


def _contrastive_epoch(opt, table, classifier, optimizer, epoch, order_dev, sets, contrastive_weight, tau):
    """train_one_epoch_cl (:412-508): step idx takes the next batch_factor sets of the order (the last step may hold fewer, at the
    same scale = contrastive_weight / batch_factor); one gather of the step's T * S rows, one sets_step, warmup_learning_rate before
    it; steps at idx >= opt.ca_update are skipped.  The pass advances the torch stream once, like a loader; ONE host sync.  Returns
    (mean over the epoch's sets of scale * l_t, sets trained on, steps taken)."""
    classifier.train()
    A, P, N = sets
    bf = int(getattr(opt, "batch_factor", 32))
    cap = getattr(opt, "ca_update", None)
    scale = contrastive_weight / bf
    _loader_base_seed()
    n_steps = -(-order_dev.shape[0] // bf)
    loss_sum = torch.zeros((), dtype=torch.float64, device=table.device)
    n_sets = taken = 0
    for idx in range(n_steps):
        if cap is not None and idx >= cap:
            continue
        rows = order_dev[idx * bf:(idx + 1) * bf]
        O.warmup_learning_rate(opt, epoch, idx, n_steps, optimizer)
        loss, _ = classifier.sets_step(ops.gather_sets(table.embeddings, rows), optimizer, sets=(rows.shape[0], A, P, N), contrastive=(scale, tau))
        loss_sum += loss.double()
        n_sets += rows.shape[0]
        taken += 1
    return (loss_sum.item() / n_sets if n_sets else 0.0), n_sets, taken


def train_contrastive_adapter(opt, train_table, val_table, test_table, log=None):
    """One run of the contrastive adapter (Zhang & Re 2022), the reference's one debiasing method that needs no group labels
    (demo/visualizer_supcon.py; dead there because its forward_ca is commented out): the anchors are the train rows CLIP's zero-shot
    prediction (`train_table.y_pred`) got wrong, each scored against sampled positives (same class, predicted right) and negatives
    (other class) of its own -- contrastive.py -- and the adapter is trained on scale * sum_t l_t alone (CustomCLIP.sets_step).

    The epoch loop is the reference's train_all_epochs (:720-772): adjust_learning_rate, one contrastive epoch (train_one_epoch_cl),
    validate the class prompts on the val split, keep the best worst-group model (strict `>`), validate on test; at the end the
    zero-shot class / spurious pair of the best model.  The sets are built once, after the model is created: slices, points, batches,
    order, from the global numpy stream.  Options (the reference's names, read with getattr): num_anchor (1), num_positive,
    num_negative (required), batch_factor (32), ca_update (no cap), contrastive_weight (1), cl_temperature (0.1), balance_by_zs_pred
    (False), re_shuffle_ca_loader (True), maintain_alternative_ordering (False).

    Departures from the dead reference path: a step's T * S rows are ONE train-mode BatchNorm batch; no
    ca_pre_norm and no ca_head (the adapter is fed raw embeddings, like the model that is validated and selected); the max subtracted
    in the loss is over positives and negatives.  Two classes; single run; CustomCLIP on the adapter's fast shape.

    Returns ((best train, best val, best test), (zero-shot class, zero-shot spurious)) like train_all_epochs; the train entry of a
    contrastive epoch is {"loss": its loss average} (the reference's contrastive epoch scores no accuracy).  `log` (a list) receives
    one record per initialisation, the sets (`kind="sets"`) and per train / validate pass; a train record carries `loss` = the mean
    over the epoch's sets of scale * l_t, `n_sets`, `n_steps` and `order` (the sets trained on, [n_sets, S])."""
    rec = (lambda **k: log.append(k)) if log is not None else (lambda **k: None)
    dev = train_table.device
    D = train_table.embeddings.shape[1]
    classifier = adapter.CustomCLIP(adapter.Adapter(D, opt.adapter_feat_dim), opt.text_embedding_dir, opt.text_spurious_embedding_dir,
                                    opt.text_group_embedding_dir, temperature=opt.zs_temperature)
    rec(kind="init", state={k: v.clone() for k, v in classifier.adapter.state_dict().items()})
    classifier = classifier.to(dev)
    optimizer = O.set_optimizer(opt, classifier)
    order = _contrastive_sets(opt, train_table)
    A, P, N = int(getattr(opt, "num_anchor", 1)), int(opt.num_positive), int(opt.num_negative)
    weight, tau = float(getattr(opt, "contrastive_weight", 1.0)), float(getattr(opt, "cl_temperature", 0.1))
    rec(kind="sets", order=order, sets=(A, P, N))
    order_dev = torch.from_numpy(order).to(dev)
    ratio = train_table.group_ratio.numpy()
    bs_eval = max(opt.batch_size, 4096)
    best_acc, best_epoch, best = 0, 0, None
    train_accs, val_accs, test_accs = [], [], []
    for epoch in range(1, opt.epochs + 1):
        O.adjust_learning_rate(opt, optimizer, epoch)
        loss, n_sets, n_steps = _contrastive_epoch(opt, train_table, classifier, optimizer, epoch, order_dev, (A, P, N), weight, tau)
        rec(kind="train_cl", epoch=epoch, loss=loss, n_sets=n_sets, n_steps=n_steps, order=order[:n_sets])
        train_accs.append({"loss": loss})
        for split, table, target, accs in (("val", val_table, opt.train_target, val_accs), ("test", test_table, "class", test_accs)):
            st = {}
            vloss, vacc, vg = validate(table, classifier, bs_eval, ratio, target=target, stats=st)
            rec(kind="validate", epoch=epoch, split=split, loss=vloss, acc=vacc, group_acc=vg, counts=st["counts"])
            accs.append(vg)
            if split == "val" and vg["worst_acc"] > best_acc:
                best_acc, best_epoch, best = vg["worst_acc"], epoch, deepcopy(classifier)
    if best is None:
        raise RuntimeError("train_contrastive_adapter: the worst-group accuracy never rose above 0, so there is no best model")
    zero_shot = []
    for target in ("class", "spurious"):
        st = {}
        zl, za, zg = validate(test_table, best, bs_eval, ratio, target=target, spurious=target == "spurious", stats=st)
        rec(kind="validate_zs", target=target, loss=zl, acc=za, group_acc=zg, counts=st["counts"])
        zero_shot.append(zg)
    rec(kind="final", best_epoch=best_epoch, best_model=best)
    e = best_epoch - 1
    return (train_accs[e], val_accs[e], test_accs[e]), (zero_shot[0], zero_shot[1])


def train_all_epochs(opt, train_table, val_table, test_table, input_dim=None, log=None):
    """One run of the training schedule (_run_schedule: `linear_probing`, `adapter`, `adapter_reg`, `adapter_reg_seq`,
    `adapter_reg_seq_alter`, with or without `--add_adapter`, `--balance_val`, `--continue_from_best`) on device-resident tables,
    every step one fused C call.  `opt` = the namespace of the reference's parse_option (same field names).  The run draws from the
    global random streams as they are (the caller seeds them: optim.set_seed).  Returns ((best train, best val, best test
    group-accuracy dicts), (zero-shot class, zero-shot spurious)) like the reference; `log` (a list) receives one record per
    initialisation and per train / validate pass."""
    logs = [] if log is not None else None
    out = _run_schedule(_SingleRun(opt), [opt], train_table, val_table, test_table, input_dim, logs)
    if log is not None:
        log.extend(logs[0])
    return out[0]


def train_jtt(opt, train_table, val_table, test_table, log=None):
    """Just Train Twice (Liu et al. 2021), the label-free baseline, as one run: an identification model of the method's own kind
    (`linear_probing`: LinearClassifier; the adapter methods: CustomCLIP(Adapter)) takes opt.jtt_epochs (T, default 1) plain
    train_epochs on the train table under the schedule's learning-rate rule (adjust_learning_rate per epoch, warm-up per step); its
    eval-mode predictions on the whole train table give the error set (no random draw); then train_all_epochs runs on a copy of `opt`
    with row_weights = jtt_weights(error set, opt.jtt_lambda (default 5)) -- in opt.row_weight_mode, "loss" by default.  The global
    random streams are consumed in that order (identification model's initialisation, its T loader orders, then the second stage's
    own draws), so a seed fixes the run.  opt.row_weights must be unset; opt.robust / opt.contrastive_weight raise as in the
    schedule, before a model is built.  Single runs only (a JTT sweep: train_sweep with [R, N] weights).

    Returns train_all_epochs' result plus the error set (bool [N] numpy): ((best train, best val, best test), (zero-shot class,
    zero-shot spurious), wrong).  `log` (a list) receives the identification model's records first (`init`, one `jtt_identify` per
    epoch, then `jtt_errors` with `wrong`, `n_wrong` and `rng_state` = the (torch, numpy) stream states the second stage starts
    from), then train_all_epochs' records."""
    if opt.tl_method not in _METHODS:
        raise ValueError(f"train_jtt covers linear_probing and the adapter methods, not tl_method={opt.tl_method!r}")
    if getattr(opt, "row_weights", None) is not None:
        raise ValueError("train_jtt sets opt.row_weights itself (jtt_weights of the error set); leave it unset")
    T, lam = int(getattr(opt, "jtt_epochs", 1)), float(getattr(opt, "jtt_lambda", 5.0))
    if T < 1 or not np.isfinite(lam) or lam <= 0:
        raise ValueError(f"train_jtt: jtt_epochs >= 1 and a finite jtt_lambda > 0 expected, got {T}, {lam}")
    probe = copy(opt)
    probe.row_weights = np.ones(len(train_table))
    _row_weight_option(probe, len(train_table))                            # the schedule's refusals, before a model is built
    rec = (lambda **k: log.append(k)) if log is not None else (lambda **k: None)
    dev = train_table.device
    D = train_table.embeddings.shape[1]
    linear = opt.tl_method == "linear_probing"
    if linear:
        model = adapter.LinearClassifier(D, opt.n_cls)
    else:
        model = adapter.CustomCLIP(adapter.Adapter(D, opt.adapter_feat_dim), opt.text_embedding_dir, opt.text_spurious_embedding_dir,
                                   opt.text_group_embedding_dir, temperature=opt.zs_temperature)
    rec(kind="init", state={k: v.clone() for k, v in (model if linear else model.adapter).state_dict().items()})
    model = model.to(dev)
    optimizer = O.set_optimizer(opt, model)
    for epoch in range(1, T + 1):
        O.adjust_learning_rate(opt, optimizer, epoch)
        st = {}
        loss, acc, gacc = train_epoch(train_table, model, optimizer, opt.batch_size, target=opt.train_target,
                                      lr_hook=lambda i, n: O.warmup_learning_rate(opt, epoch, i, n, optimizer), stats=st)
        rec(kind="jtt_identify", epoch=epoch, loss=loss, acc=acc, group_acc=gacc, counts=st["counts"], order=st["order"])
    wrong = prediction_errors(train_table, model, target=opt.train_target)
    rec(kind="jtt_errors", wrong=wrong, n_wrong=int(wrong.sum()), rng_state=(torch.get_rng_state(), np.random.get_state()))
    second = copy(opt)
    second.row_weights = jtt_weights(wrong, lam)
    out = train_all_epochs(second, train_table, val_table, test_table, log=log)
    return out + (wrong,)


@torch.no_grad()
def prediction_errors(table, classifier, target="class", batch_size=4096):
    """bool [N] (numpy): the rows of `table` whose eval-mode prediction (argmax of the logits, the first maximum) differs from the
    `target` label; in-order batches, no random draw.  Leaves the classifier in eval mode."""
    classifier.eval()
    labels = table.labels(target)
    wrong = []
    for i in range(0, len(table), batch_size):
        idx = torch.arange(i, min(i + batch_size, len(table)), device=table.device)
        emb, y, _ = table.batch(idx, target)
        logits = classifier.loss(emb, y)[1]
        wrong.append(logits.argmax(1) != y)
    return torch.cat(wrong).cpu().numpy()


@torch.no_grad()
def _probe_counts(emb, labels, groups, n_groups, W, b, rows=None):
    """(n, correct) counters [R, G, 2] and CE sums [R] (numpy) of R linear probes W [R, C, D], b [R, C] over the rows `rows` (int64
    numpy; None: all) of the embeddings `emb`.  On the device: ops.linear_sweep_eval in chunks of 16 probes; embeddings on the host
    (the solver="reference" path of train_dfr, which runs without a GPU) are scored in torch."""
    R, dev = W.shape[0], emb.device
    counts = torch.zeros((R, n_groups, 2), dtype=torch.int64, device=dev)
    loss = torch.zeros(R, dtype=torch.float64, device=dev)
    idx = None if rows is None else torch.as_tensor(rows, dtype=torch.int64).to(dev)
    W, b = W.to(dev, torch.float32).contiguous(), b.to(dev, torch.float32).contiguous()
    if dev.type == "cuda":
        for r0 in range(0, R, 16):
            ops.linear_sweep_eval(emb, idx, labels, groups, W[r0:r0 + 16], b[r0:r0 + 16], counts[r0:r0 + 16], loss[r0:r0 + 16])
    else:
        x, y, g = (emb, labels, groups) if idx is None else (emb[idx], labels[idx], groups[idx])
        for r in range(R):
            logits = x @ W[r].t() + b[r]
            loss[r] = torch.nn.functional.cross_entropy(logits.double(), y, reduction="sum")
            hit = logits.argmax(1) == y
            counts[r, :, 0] = torch.bincount(g, minlength=n_groups)[:n_groups]
            counts[r, :, 1] = torch.bincount(g[hit], minlength=n_groups)[:n_groups]
    return counts.cpu().numpy(), loss.cpu().numpy()


def _worst_group_acc(c):
    """smallest correct / n over the groups of one probe's counters [G, 2]"""
    return float((c[:, 1] / np.maximum(c[:, 0], 1)).min())


def train_dfr(opt, train_table, val_table, test_table, transform=None, log=None):
    """Deep feature reweighting, DFR-Val (Kirichenko et al. 2023), as one call: L1-penalised logistic probes (dfr.fit_l1_probes)
    on group-balanced subsets of the VALIDATION split, on frozen embeddings.  No learning rate is involved.

    Standardise (opt.dfr_preprocess, default True): column mean and population standard deviation of the TRAIN table from float64
    sums (a constant column's 0 becomes 1); the probes see a standardised copy of the val table.  `transform` (a stage-1 adapter, any
    callable on [B, D] rows) is applied first, batch by batch in eval mode, to all three tables.
    Tune: val is split into two halves by a private RandomState(opt.dfr_seed, default 0); for every C of opt.dfr_c_grid (sklearn's C:
    lam = 1 / (C n); default dfr.DEFAULT_C_GRID) and each of opt.dfr_tune_retrains (default 1) balanced subsets of the first half
    (analysis.balanced_rows' rule over group_array, private streams) one probe is fitted -- all of them in ONE fit_l1_probes call --
    and scored by its worst-group accuracy on the second half.  The best mean score wins, ties go to the smaller C.
    Refit: opt.dfr_retrains (default 10) balanced subsets of the whole val split at the chosen C; weights and intercepts are
    averaged, the standardisation is folded into them in float64 (W / sigma, b - sum W mu / sigma) and they are loaded into an
    adapter.LinearClassifier that works on the (transformed) raw embeddings, which every evaluation path takes unchanged.
    opt.dfr_solver: "device" (default; the fused kernel) or "reference" (dfr.prox_fit_reference in float64: runs on host tables,
    without a GPU); opt.dfr_tol (1e-4), opt.dfr_max_iter (1000), opt.dfr_check_every (32).  The global random streams are untouched.

    Refused with ValueError before a model is built or anything is launched: a group absent from val or from one of its halves, more
    than 8 classes, a val label outside [0, n_cls), an empty grid, a non-positive C.

    Returns (classifier, ((train), (val), (test)) scores as `validate` gives them, record).  The val score is on rows the probe was
    TRAINED on (every refit subset is drawn from val): only the test score is held out.  The record holds the chosen C, the tuning
    table (C, per-subset worst-group accuracies, their mean), per-retrain nnz / iterations / convergence, and the step set-up and
    fit seconds.  `log` (a list) receives `dfr_tune`, `dfr_fit` and `dfr_eval` records."""
    c_grid = [float(c) for c in getattr(opt, "dfr_c_grid", dfr.DEFAULT_C_GRID)]
    n_cls = int(getattr(opt, "n_cls", val_table.n_classes))
    seed = int(getattr(opt, "dfr_seed", 0))
    n_tune, n_fit = int(getattr(opt, "dfr_tune_retrains", 1)), int(getattr(opt, "dfr_retrains", 10))
    solver = getattr(opt, "dfr_solver", "device")
    kw = dict(solver=solver, tol=float(getattr(opt, "dfr_tol", 1e-4)), max_iter=int(getattr(opt, "dfr_max_iter", 1000)),
              check_every=int(getattr(opt, "dfr_check_every", 32)), n_classes=n_cls)
    target = getattr(opt, "train_target", "class")
    if solver not in ("device", "reference"):
        raise ValueError(f"train_dfr: opt.dfr_solver 'device' or 'reference' expected, got {solver!r}")
    if n_tune < 1 or n_fit < 1:
        raise ValueError(f"train_dfr: dfr_tune_retrains >= 1 and dfr_retrains >= 1 expected, got {n_tune}, {n_fit}")
    groups = np.asarray(val_table.group_array)
    halves = dfr.val_halves(len(val_table), seed)
    dfr.check_options(c_grid, n_cls, val_table.labels(target).cpu().numpy(), groups, val_table.n_groups, halves)
    rec = (lambda **k: log.append(k)) if log is not None else (lambda **k: None)
    dev = val_table.device
    bs_eval = max(int(getattr(opt, "batch_size", 4096)), 4096)

    def rows_of(table):
        if transform is None:
            return table.embeddings
        from . import analysis
        return analysis._transformed_rows(table.embeddings, transform, bs_eval)

    xt, xv = rows_of(train_table), rows_of(val_table)
    D = xv.shape[1]
    if bool(getattr(opt, "dfr_preprocess", True)):
        mean, std = dfr.column_moments(xt)
        zv = dfr.standardised(xv, mean.to(dev), std.to(dev))
    else:
        mean, std = torch.zeros(D, dtype=torch.float64, device=dev), torch.ones(D, dtype=torch.float64, device=dev)
        zv = xv
    labels, gdev = val_table.labels(target), val_table.targets_group

    # tune: every (C, subset) of half A is one fit of one call; scored on half B
    subsets = dfr.balanced_subsets(groups, halves[0], [seed + 1 + j for j in range(n_tune)])
    n = subsets.shape[1]
    idx = np.concatenate([subsets] * len(c_grid))                          # C-major: fit i * n_tune + j is (c_grid[i], subset j)
    lam = np.repeat([1.0 / (c * n) for c in c_grid], n_tune)
    t0 = time.perf_counter()
    fit = dfr.fit_l1_probes(zv, idx, labels, lam, **kw)
    counts, _ = _probe_counts(zv, labels, gdev, val_table.n_groups, fit.weights, fit.intercepts, rows=halves[1])
    tune_seconds = time.perf_counter() - t0
    worst = np.array([_worst_group_acc(c) for c in counts]).reshape(len(c_grid), n_tune)
    table = [dict(C=c, worst_acc=worst[i].tolist(), mean=float(worst[i].mean())) for i, c in enumerate(c_grid)]
    best = dfr.pick_c(c_grid, [t["mean"] for t in table])
    C = c_grid[best]
    rec(kind="dfr_tune", C=C, table=table, subsets=subsets, halves=halves, counts=counts, iterations=fit.iterations.numpy(),
        converged=fit.converged.numpy(), nnz=fit.nnz.numpy(), setup_seconds=fit.setup_seconds, seconds=tune_seconds)

    # refit on balanced subsets of the whole val split at the chosen C; average; fold the standardisation in
    subsets = dfr.balanced_subsets(groups, np.arange(len(val_table)), [seed + 1 + n_tune + j for j in range(n_fit)])
    t0 = time.perf_counter()
    refit = dfr.fit_l1_probes(zv, subsets, labels, [1.0 / (C * subsets.shape[1])] * n_fit, **kw)
    fit_seconds = time.perf_counter() - t0
    W, b = dfr.fold_standardisation(refit.weights.double().mean(0), refit.intercepts.double().mean(0), mean.to(dev), std.to(dev))
    rec(kind="dfr_fit", C=C, subsets=subsets, iterations=refit.iterations.numpy(), converged=refit.converged.numpy(),
        nnz=refit.nnz.numpy(), weights=refit.weights.cpu(), intercepts=refit.intercepts.cpu(), setup_seconds=refit.setup_seconds,
        seconds=fit_seconds)
    with torch.random.fork_rng(devices=[]):                                # nn.Linear's initialisation draws; the weights are replaced
        classifier = adapter.LinearClassifier(D, n_cls)
    with torch.no_grad():
        classifier.fc.weight.copy_(W.float())
        classifier.fc.bias.copy_(b.float())
    classifier = classifier.to(dev).eval()

    ratio = train_table.group_ratio.numpy()
    scores = []
    for split, table_, x in (("train", train_table, xt), ("val", val_table, xv), ("test", test_table, None)):
        x = rows_of(table_) if x is None else x
        if dev.type == "cuda":
            scored = table_
            if transform is not None:
                scored = copy(table_)
                scored.embeddings = x
            st = {}
            res = validate(scored, classifier, bs_eval, ratio, target="class" if split == "test" else target, stats=st)
            c = st["counts"]
        else:
            tg = "class" if split == "test" else target
            cs, ls = _probe_counts(x, table_.labels(tg), table_.targets_group, table_.n_groups, classifier.fc.weight.detach()[None],
                                   classifier.fc.bias.detach()[None])
            c = cs[0]
            res = _scores(table_, c, float(ls[0]), len(table_), ratio)
        rec(kind="dfr_eval", split=split, loss=res[0], acc=res[1], group_acc=res[2], counts=c)
        scores.append(res)
    record = dict(C=C, tuning=table, nnz=refit.nnz.tolist(), iterations=refit.iterations.tolist(), converged=refit.converged.tolist(),
                  tune_iterations=fit.iterations.tolist(), tune_converged=fit.converged.tolist(), solver=solver,
                  setup_seconds=fit.setup_seconds + refit.setup_seconds, tune_seconds=tune_seconds, fit_seconds=fit_seconds,
                  mean=mean.cpu(), std=std.cpu())
    return classifier, tuple(scores), record


# ---------------------------------------------------------------------------------------------------------------------
# seed sweeps (run_multiple/final_main_iteration_wb.py, final_main_iteration_ca.py): R runs in lock-step, one launch for all
# ---------------------------------------------------------------------------------------------------------------------

class ReplicaStreams:
    """The global torch and numpy random streams of R runs that advance in lock-step.  In the reference each seed's run owns the
    two global streams from set_seed to its end; here every replica keeps its own saved pair of states, swapped in around each
    host-side draw: `run(r, fn, *args)` calls fn with replica r's streams installed and saves them again.  The draws themselves
    are the ordinary functions (module constructors, dataloader_shuffle_order, the balance_val draw), unchanged."""

    def __init__(self, seeds):
        self.states = []
        for s in seeds:
            O.set_seed(s)
            self.states.append((torch.get_rng_state(), np.random.get_state()))

    def run(self, r, fn, *args, **kwargs):
        t, n = self.states[r]
        torch.set_rng_state(t)
        np.random.set_state(n)
        try:
            return fn(*args, **kwargs)
        finally:
            self.states[r] = (torch.get_rng_state(), np.random.get_state())


def _with_replica_weights(opts, n_replicas, first):
    """`opts`, the namespaces of replicas first, first + 1, ... of a sweep of `n_replicas`, with per-replica weights cut to their own
    rows: opt.row_weights of shape [n_replicas, N] becomes rows first : first + len(opts) on copies of the namespaces (one row,
    [N], for a replica that runs alone).  Anything else -- unset, "zs_failures", [N], [1, N] -- is shared: `opts` as they are."""
    given = getattr(opts[0], "row_weights", None)
    if given is None or isinstance(given, str) or np.ndim(given) != 2 or n_replicas < 2 or np.shape(given)[0] != n_replicas:
        return list(opts)
    rows = np.asarray(given)[first:first + len(opts)]
    out = [copy(o) for o in opts]
    for o in out:
        o.row_weights = rows[0] if len(opts) == 1 else rows
    return out


def _sweep_replicas(opt, seeds, learning_rates):
    """(opt of the replica, seed) pairs, learning-rate-major like final_main_iteration_ca.py's loops"""
    if learning_rates is None:
        return [(opt, s) for s in seeds]
    out = []
    for lr in learning_rates:
        o = copy(opt)
        o.learning_rate = lr
        o.learning_rate_reg = lr * getattr(opt, "lr_multiple", 1.0)
        out += [(o, s) for s in seeds]
    return out


class _Lr:
    """what the schedule helpers of optim.py need of an optimiser: param_groups with an 'lr'"""
    def __init__(self, lr):
        self.param_groups = [{"lr": lr}]

    @property
    def lr(self):
        return self.param_groups[0]["lr"]


def _sweep_train_pass(streams, sweep, table, orders_fn, batch_size, target, use_group, lr_fn, momentum, weight_decay, counted=True, acc=None,
                      sync=True, robust=None, row_weights=None):
    """one loader pass of every replica: `orders_fn(r)` draws replica r's row order (under its own streams), all orders go to the
    device in ONE upload, then n_steps batched steps; lr_fn(step, n_steps) -> the R learning rates.  `sweep`: SweepAdapters (scored on
    the group prompts when `use_group`, else the class prompts) or SweepLinear.  `counted`: the pass adds to the loss sums and group
    counters; `acc` = (counts, loss sums) device tensors of an epoch made of several passes (fresh ones if None).  Returns (counts
    [R, G, 2] numpy, loss sums [R] numpy, orders, acc) after the pass's one host sync; the two arrays are None without `sync`.
    `robust`: an adapter.GroupDRO state with q [R, G] -- every step is a group-DRO step over the table's group ids.  `row_weights`:
    float32 [Rw, N] on the device over the table's rows -- every step is the weighted step."""
    R, dev = sweep.R, table.device
    linear = isinstance(sweep, adapter.SweepLinear)
    orders = [streams.run(r, orders_fn, r) for r in range(R)]
    n = len(orders[0])
    if any(len(o) != n for o in orders):
        raise RuntimeError("sweep: replicas of one group must have passes of equal length")
    idx = torch.stack(orders).to(dev, non_blocking=True)                          # [R, n]: the pass's one index upload
    n_full, rem = divmod(n, batch_size)
    steps = []
    if n_full:
        full = idx[:, :n_full * batch_size].view(R, n_full, batch_size).permute(1, 0, 2).contiguous()       # [n_steps, R, B]
        steps += [full[i] for i in range(n_full)]
    if rem:
        if rem < 2 and not linear:
            raise ValueError("Expected more than 1 value per channel when training (BatchNorm1d)")
        steps.append(idx[:, n_full * batch_size:].contiguous())
    if acc is None:
        acc = (torch.zeros((R, table.n_groups, 2), dtype=torch.int64, device=dev), torch.zeros((R,), dtype=torch.float64, device=dev))
    counts, loss_sum = acc
    labels = table.targets_group if use_group else table.labels(target)
    prompts = () if linear else ("group" if use_group else "class",)
    extra = {} if robust is None else {"robust": robust}
    if row_weights is not None:
        extra["row_weights"] = row_weights
    for i, b in enumerate(steps):
        sweep.step(table.embeddings, b, labels, table.targets_group, *prompts, lr_fn(i, len(steps)), momentum, weight_decay, counts, loss_sum,
                   counted=counted, **extra)
    orders = [o.numpy() for o in orders]
    if not sync:
        return None, None, orders, acc
    return counts.cpu().numpy(), loss_sum.cpu().numpy(), orders, acc


def _sweep_validate(streams, sweep, table, batch_size, target, indices_dev, n, spurious=False, best=False, draw=True):
    """validate() for every replica: every replica's stream advances by the one draw a loader pass makes; the rows are the same
    for all replicas.  Returns (counts [R, G, 2], loss sums [R]) as numpy arrays."""
    R, dev = sweep.R, table.device
    if draw:
        for r in range(R):
            streams.run(r, _loader_base_seed)
    counts = torch.zeros((R, table.n_groups, 2), dtype=torch.int64, device=dev)
    loss_sum = torch.zeros((R,), dtype=torch.float64, device=dev)
    labels = table.labels(target)
    prompts = () if isinstance(sweep, adapter.SweepLinear) else ("spurious" if spurious else "class",)
    for i in range(0, n, batch_size):
        m = min(batch_size, n - i)
        if indices_dev is not None:
            sweep.evaluate(table.embeddings, indices_dev[i:i + m], labels, table.targets_group, *prompts, counts, loss_sum, best=best)
        else:
            sweep.evaluate(table.embeddings, None, labels, table.targets_group, *prompts, counts, loss_sum, row0=i, n=m, best=best)
    return counts.cpu().numpy(), loss_sum.cpu().numpy()


class _LockStep:
    """Executor of up to 16 runs in lock-step on stacked parameters (adapter.SweepAdapters / adapter.SweepLinear): every training
    step and every evaluation batch is one replica-batched call, every pass uploads its row orders once and an epoch's training
    synchronises with the host once.  Every run keeps its own pair of random streams (ReplicaStreams); its optimiser is the momentum
    buffers inside the stacked set plus an _Lr the schedule's learning-rate helpers write to."""

    def __init__(self, opts, seeds):
        self.opts, self.R = opts, len(opts)
        self.streams = ReplicaStreams(seeds)
        self.sweep = None
        self._dev_rows = None
        self.dro, self.q_log = None, None                                # group DRO: q [R, G] (not part of the best models)

    def start(self, models, device):
        linear = isinstance(models[0], adapter.LinearClassifier)
        self.sweep = (adapter.SweepLinear if linear else adapter.SweepAdapters).from_modules(models, device)
        return [_Lr(o.learning_rate) for o in self.opts]

    def start_robust(self, n_groups, step_size, device):
        self.dro = adapter.GroupDRO(n_groups, step_size, device, replicas=self.R)

    def restore(self):
        self.sweep.restore([True] * self.R)

    def switch(self, fresh):
        if fresh is not None:
            self.sweep.add_adapters(fresh, self.opts[0].init_near_identity)
        else:
            self.sweep.reset_optimizer()
        return [_Lr(o.learning_rate_reg) for o in self.opts]

    def train(self, passes, lrs, hook):
        opt = self.opts[0]

        def lr_fn(i, n):
            hook(i, n)
            return [l.lr for l in lrs]
        acc, orders, qs = None, [], []
        for k, p in enumerate(passes):                                   # the passes of an epoch share the accumulators: one host sync
            order_fn = lambda r, p=p: _epoch_order(_pass_rows(p, r), p.shuffle, None if p.rows is None else p.rows[r])
            wdev = None
            if p.weights is not None and p.weights.mode == "sample":     # the replica's own WeightedRandomSampler loader, under its streams
                order_fn = lambda r, p=p: weighted_sampler_order(p.weights.of(r))
            elif p.weights is not None:
                wdev = p.weights.dev
            c, ls, o, acc = _sweep_train_pass(self.streams, self.sweep, p.table, order_fn, p.batch_size, opt.train_target, p.use_group, lr_fn,
                                              opt.momentum, opt.weight_decay, counted=p.counted, acc=acc, sync=k == len(passes) - 1, robust=self.dro,
                                              row_weights=wdev)
            orders.append(o)
            if self.dro is not None:
                qs.append(self.dro.q.clone())
        if self.dro is not None:
            qs = [q.cpu().numpy() for q in qs]
            self.q_log = [[q[r] for q in qs] for r in range(self.R)]
        return c, [float(x) for x in ls], [np.concatenate(o) for o in zip(*orders)]

    def evaluate(self, table, batch_size, target, indices, spurious=False, best=False):
        n = len(table) if indices is None else len(indices)
        idx = None
        if indices is not None:                                          # the val half: uploaded once for the whole run
            if self._dev_rows is None or self._dev_rows[0] is not indices:
                self._dev_rows = (indices, torch.as_tensor(indices, dtype=torch.int64).to(table.device))
            idx = self._dev_rows[1]
        sweep = self.sweep
        if not best:
            c, ls = _sweep_validate(self.streams, sweep, table, batch_size, target, idx, n, spurious=spurious)
            return c, [float(x) for x in ls]
        if not all(sweep.has_best):
            raise RuntimeError("train_sweep: a replica never had a worst-group accuracy above 0, so it has no best model")
        for r in range(self.R):                                          # one loader pass: every replica's stream advances once
            self.streams.run(r, _loader_base_seed)
        # both kinds of best model may occur in one sweep (a best epoch before / after the adapters were added): one call per kind
        counts, loss_sums = [None] * self.R, [None] * self.R
        for kind in (False, True):
            rs = [r for r in range(self.R) if sweep.best_has_old[r] == kind]
            if not rs:
                continue
            whole = len(rs) == self.R
            c, ls = _sweep_validate(self.streams, sweep if whole else sweep.subset(rs, best=True), table, batch_size, target, idx, n,
                                    spurious=spurious, best=whole, draw=False)
            for k, r in enumerate(rs):
                counts[r], loss_sums[r] = c[k], float(ls[k])
        return counts, loss_sums

    def snapshot(self, better):
        self.sweep.snapshot(better)

    def best_model(self, r):
        return self.sweep.replica(r, best=True)


def train_sweep(opt, train_table, val_table, test_table, seeds, learning_rates=None, log=None):
    """A seed sweep as one batched run: returns, per replica, exactly what `train_all_epochs` returns for that replica run alone
    after `optim.set_seed(seed)`.  Replicas are (learning rate, seed) pairs, learning-rate-major; with `learning_rates` given,
    replica (lr, seed) runs with learning_rate = lr and learning_rate_reg = lr * opt.lr_multiple, like final_main_iteration_ca.py.

    Batched path -- at least two replicas and
      * tl_method `adapter`, `adapter_reg_seq`, `adapter_reg_seq_alter`, with or without --add_adapter, --balance_val,
        --continue_from_best, --init_near_identity, and `adapter_reg` (with or without --balance_val, --use_cls_prompt_in_reg), on
        the adapter's fast shape (hidden width 128, D % 128 == 0): adapter.SweepAdapters;
      * tl_method `linear_probing` with n_cls <= 8, D % 4 == 0 and D <= 1024: adapter.SweepLinear.
    The schedule is train_all_epochs' own (_run_schedule) with the lock-step executor: all replicas advance together, every training
    step and every evaluation batch is one replica-batched call (up to 16 replicas per group of launches, more are split into
    groups), each pass uploads its row orders once and synchronises with the host once, best-model selection runs per replica on the
    host.
    Sequential path -- other shapes and a single replica: replica by replica through train_all_epochs on the same tables.
    `contrastive_adapter` raises like train_all_epochs.

    Each replica keeps its own pair of global random streams (ReplicaStreams), so its initial weights, batch orders and balanced
    subsets are those of its own sequential run.  `log` (a list) receives one list of records per replica (train_all_epochs' records)."""
    if _contrastive_option(opt) is not None:
        raise ops.DbmmUnsupported("train_sweep: the contrastive term (opt.contrastive_weight) covers single runs (train_all_epochs)")
    replicas = _sweep_replicas(opt, list(seeds), learning_rates)
    D = train_table.embeddings.shape[1]
    if opt.tl_method not in _METHODS:
        raise ValueError(f"train_sweep covers linear_probing and the adapter methods, not tl_method={opt.tl_method!r}")
    if opt.tl_method == "linear_probing":
        batched = len(replicas) >= 2 and 1 <= opt.n_cls <= 8 and D % 4 == 0 and D <= 1024
    else:
        batched = len(replicas) >= 2 and opt.adapter_feat_dim == 128 and D % 128 == 0 and bool(ops.get_option("adapter_step_fused"))
    out = []
    if not batched:
        for k, (o, s) in enumerate(replicas):
            O.set_seed(s)
            lg = [] if log is not None else None
            out.append(train_all_epochs(_with_replica_weights([o], len(replicas), k)[0], train_table, val_table, test_table, log=lg))
            if log is not None:
                log.append(lg)
        return out
    for i in range(0, len(replicas), 16):
        opts, group_seeds = zip(*replicas[i:i + 16])
        opts = _with_replica_weights(opts, len(replicas), i)
        out += _run_schedule(_LockStep(opts, group_seeds), opts, train_table, val_table, test_table, log=log)
    return out


def sweep_frame(results):
    """The table of the reference's sweep drivers (final_main_iteration_wb.py:1136-1161, :1193) from the per-seed results of
    train_sweep / train_all_epochs, in run order: per block the per-seed rows 1 .. n, `<block>_mean`, `<block>_std`; blocks in the
    order test, spurious zero-shot, train, val, target zero-shot; rounded to 4 places.  Built with the reference's own pandas
    statements, so it has its property that a block's std row is taken after the mean row was appended (the sample standard deviation
    of the n values and their mean)."""
    import pandas as pd

    def block(dicts, tag):
        df = pd.concat([pd.DataFrame(d, index=[i + 1]) for i, d in enumerate(dicts)])
        df = pd.concat([df, pd.DataFrame(df.mean().to_dict(), index=[tag + "_mean"])])
        return pd.concat([df, pd.DataFrame(df.std().to_dict(), index=[tag + "_std"])])
    tr = block([r[0][0] for r in results], "tr")
    val = block([r[0][1] for r in results], "val")
    test = block([r[0][2] for r in results], "test")
    zt = block([r[1][0] for r in results], "zs_tg")
    zsp = block([r[1][1] for r in results], "zs_spu")
    return pd.concat([test, zsp, tr, val, zt]).round(4)


def sweep_result_name(opt):
    """file name (without .csv) of the reference's sweep drivers (final_main_iteration_wb.py:1166-1191)"""
    name = f"ds_{opt.dataset}_tl_{opt.tl_method}_bs_{opt.batch_size}_lr_{opt.learning_rate}"
    if "reg" in opt.tl_method:
        name += f"_lrr{opt.learning_rate_reg}_bsr{opt.batch_size_reg}"
        if opt.balance_val:
            name += "_balval"
        if opt.tl_method != "adapter_reg_seq_alter":
            name += "_CP" if opt.use_cls_prompt_in_reg else "_GP"
        if opt.add_adapter:
            name += "_MA" + ("+ni" if opt.init_near_identity else "+rn")
        if opt.continue_from_best and "seq" in opt.tl_method:
            name += "_cont"
    if getattr(opt, "resample_ce", False):
        name += "_rs"
    if getattr(opt, "robust", False):
        name += "_gdro"
    return name


def run_sweep(opt, tables, out_dir):
    """The two sweep drivers of the reference on device-resident tables (`tables` = (train, val, test) EmbeddingTables).
    With opt.lr_list / opt.bs_list / opt.bsr_list (comma-separated strings or sequences; final_main_iteration_ca.py:1167-1186) the
    (batch size, reg batch size) groups run one after the other and every group trains all lr_list x opt.random_seeds replicas as
    one batched sweep; without them it is final_main_iteration_wb.py: opt.random_seeds at opt's own settings.  Writes one CSV per
    (lr, bs, bsr) under `out_dir`, named like the reference's, and returns {file path: frame}."""
    def as_list(v, conv):
        if v is None:
            return None
        return [conv(x) for x in (v.split(",") if isinstance(v, str) else v)]
    seeds = list(opt.random_seeds)[:getattr(opt, "num_iter", len(opt.random_seeds))]
    lrs = as_list(getattr(opt, "lr_list", None), float)
    bss = as_list(getattr(opt, "bs_list", None), int) or [opt.batch_size]
    bsrs = as_list(getattr(opt, "bsr_list", None), int) or [opt.batch_size_reg]
    if lrs is not None and opt.tl_method == "adapter":
        bsrs = [128]
    os.makedirs(out_dir, exist_ok=True)
    written = {}
    for bs in bss:
        for bsr in bsrs:
            o = copy(opt)
            o.batch_size, o.batch_size_reg = bs, bsr
            results = train_sweep(o, *tables, seeds, learning_rates=lrs)
            for k, lr in enumerate(lrs if lrs is not None else [None]):
                if lr is not None:
                    o.learning_rate, o.learning_rate_reg = lr, lr * getattr(opt, "lr_multiple", 1.0)
                frame = sweep_frame(results[k * len(seeds):(k + 1) * len(seeds)])
                path = os.path.join(out_dir, sweep_result_name(o) + ".csv")
                frame.to_csv(path)
                written[path] = frame
    return written
