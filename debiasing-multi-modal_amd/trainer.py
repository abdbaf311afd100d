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
`adapter.balance_val_indices` the per-epoch group balancing from the global numpy RNG.
"""
from functools import partial

import numpy as np
import torch

from . import adapter, ops

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
    torch.empty((), dtype=torch.int64).random_()                       # _BaseDataLoaderIter._base_seed
    seed = int(torch.empty((), dtype=torch.int64).random_().item())   # RandomSampler.__iter__
    g = torch.Generator()
    g.manual_seed(seed)
    return torch.randperm(n, generator=g)


def _epoch_batches(n, batch_size, shuffle, indices):
    if shuffle:
        order = dataloader_shuffle_order(n)
    else:
        torch.empty((), dtype=torch.int64).random_()                   # every DataLoader iterator draws its base seed, shuffled or not:
        order = torch.arange(n)                                        # the global torch RNG advances like the reference's loops
    if indices is not None:
        order = torch.as_tensor(np.asarray(indices), dtype=torch.int64)[order]
    return [order[i:i + batch_size] for i in range(0, n, batch_size)]


def _results(counts, n_places=2):
    """get_results (final_main.py:395-406) from integer (n, correct) counters."""
    meters = {}
    for g in range(counts.shape[0]):
        m = adapter.AverageMeter()
        n, corr = int(counts[g, 0]), int(counts[g, 1])
        if n:
            m.update(corr / n, n)
        meters[g] = m
    return adapter.get_results(meters, partial(adapter.get_y_p, n_places=n_places))


def _train_pass(table, classifier, optimizer, batch_size, target, use_group, indices, shuffle, lr_hook, counts, loss_sum, counted=True):
    """one loader pass of steps; `counted`: the pass adds to the epoch's loss sum and group counters.  Returns the pass's batches."""
    n = len(table) if indices is None else len(indices)
    batches = _epoch_batches(n, batch_size, shuffle, indices)
    dev = table.device
    for step, idx in enumerate(batches):
        idx = idx.to(dev, non_blocking=True)
        emb, labels, groups = table.batch(idx, target)
        if use_group:
            labels = groups
        if lr_hook is not None:
            lr_hook(step, len(batches))
        loss, logits, _ = classifier.train_step(emb, labels, optimizer, use_group)
        if counted:
            loss_sum += loss.double() * idx.numel()                  # losses.update(loss.item(), bsz)
            adapter.group_counts(logits, labels, groups, table.n_groups, counts)
    return batches


def _train_results(table, counts, loss_sum, n):
    c = counts.cpu().numpy()
    total = int(c[:, 0].sum())
    res = _results(c, table.n_places)
    group_acc = {k: np.round(res[k], 4) for k in NEW_ORDER_FOR_PRINT[1:]}
    return c, (loss_sum.item() / n, int(c[:, 1].sum()) / total, group_acc)


def train_epoch(table, classifier, optimizer, batch_size, target="class", use_group=False, indices=None,
                shuffle=True, lr_hook=None, stats=None):
    """One epoch of train_one_epoch / train_reg_seq_one_epoch.  `indices` restricts the epoch to a
    subset (reg split, balanced indices); `lr_hook(step, n_steps)` runs before every step (the
    warm-up helpers).  Returns (loss average, accuracy, group accuracy dict) like the reference,
    computed from device-side accumulators with ONE host sync at the end.  `stats` (a dict) receives
    the integer (n, correct) counters [G, 2] and the row order of the epoch."""
    classifier.train()
    n = len(table) if indices is None else len(indices)
    dev = table.device
    counts = torch.zeros((table.n_groups, 2), dtype=torch.int64, device=dev)
    loss_sum = torch.zeros((), dtype=torch.float64, device=dev)
    batches = _train_pass(table, classifier, optimizer, batch_size, target, use_group, indices, shuffle, lr_hook, counts, loss_sum)
    c, out = _train_results(table, counts, loss_sum, n)
    if stats is not None:
        stats.update(counts=c, order=torch.cat(batches).numpy())
    return out


def train_reg_epoch(train_table, reg_table, classifier, optimizer, batch_size, reg_rows, reg_batch_size, reg_shuffle, target="class",
                    group_prompt=True, lr_hook=None, stats=None):
    """One epoch of train_reg_one_epoch (final_main.py:498-569): the shuffled train split on the class prompts, then -- same
    optimiser, same epoch -- the reg loader (`reg_rows` of `reg_table`, shuffled or not), on the group prompts with group labels
    when `group_prompt`.  `lr_hook(step, n_steps)` restarts with each loader like the reference's warmup_learning_rate(opt, epoch,
    idx, len(dataloader)).  Loss, accuracy and group counters accumulate over the batches scored on the class prompts only (the
    train loader, and the reg loader when not `group_prompt`); one host sync per epoch.  `stats` receives the counters, the row
    order (train rows, then the reg loop's rows) and the number of train rows."""
    classifier.train()
    dev = train_table.device
    counts = torch.zeros((train_table.n_groups, 2), dtype=torch.int64, device=dev)
    loss_sum = torch.zeros((), dtype=torch.float64, device=dev)
    b1 = _train_pass(train_table, classifier, optimizer, batch_size, target, False, None, True, lr_hook, counts, loss_sum)
    b2 = _train_pass(reg_table, classifier, optimizer, reg_batch_size, target, group_prompt, reg_rows, reg_shuffle, lr_hook, counts, loss_sum,
                     counted=not group_prompt)
    n = len(train_table) + (0 if group_prompt else len(reg_rows))
    c, out = _train_results(train_table, counts, loss_sum, n)
    if stats is not None:
        stats.update(counts=c, order=torch.cat(b1 + b2).numpy(), n_train_rows=len(train_table))
    return out


@torch.no_grad()
def validate(table, classifier, batch_size, train_group_ratio, target="class", indices=None, spurious=False, stats=None):
    """validate / validate_zs (final_main.py:655-803): eval-mode forward, CE, group accuracies and
    the train-ratio-weighted mean.  A LinearClassifier is scored through its own head (LinearClassifier.loss); its
    zero-shot scores are validate_zs's own branch, validate_zs_linear_probing below."""
    classifier.eval()
    n = len(table) if indices is None else len(indices)
    dev = table.device
    counts = torch.zeros((table.n_groups, 2), dtype=torch.int64, device=dev)
    loss_sum = torch.zeros((), dtype=torch.float64, device=dev)
    for idx in _epoch_batches(n, batch_size, False, indices):
        idx = idx.to(dev, non_blocking=True)
        emb, labels, groups = table.batch(idx, target)
        _, logits, rows = classifier.loss(emb, labels, spurious=spurious)   # fused normalise + logits + CE kernel
        loss_sum += rows.double().sum()
        adapter.group_counts(logits, labels, groups, table.n_groups, counts)
    c = counts.cpu().numpy()
    if stats is not None:
        stats.update(counts=c)
    res = _results(c, table.n_places)
    indiv = [res[f"acc_{g // table.n_places}_{g % table.n_places}"] for g in range(table.n_groups)]
    res["weighted_mean_acc"] = (np.array(indiv) * np.array(train_group_ratio)).sum()
    group_acc = {k: np.round(res[k], 4) for k in NEW_ORDER_FOR_PRINT}
    return loss_sum.item() / n, int(c[:, 1].sum()) / int(c[:, 0].sum()), group_acc


@torch.no_grad()
def validate_zs_linear_probing(table, text_embedding_dir, temperature, batch_size, train_group_ratio, target="class", stats=None):
    """validate_zs's `linear_probing` branch (final_main.py:730-761): no classifier -- raw embeddings, row-normalised, against the
    column-normalised prompt matrix / T (the CLIP zero-shot baseline), CE and group accuracies.  One fused launch per batch."""
    dev = table.device
    tn = ops.text_colnorm(adapter.get_text_embedding(text_embedding_dir).to(dev).float().contiguous())
    counts = torch.zeros((table.n_groups, 2), dtype=torch.int64, device=dev)
    loss_sum = torch.zeros((), dtype=torch.float64, device=dev)
    n = len(table)
    for idx in _epoch_batches(n, batch_size, False, None):
        idx = idx.to(dev, non_blocking=True)
        emb, labels, groups = table.batch(idx, target)
        logits, rows, _, _, _ = ops.l2norm_sim_ce_fwd(emb, tn, temperature, labels=labels)
        loss_sum += rows.double().sum()
        adapter.group_counts(logits, labels, groups, table.n_groups, counts)
    c = counts.cpu().numpy()
    if stats is not None:
        stats.update(counts=c)
    res = _results(c, table.n_places)
    indiv = [res[f"acc_{g // table.n_places}_{g % table.n_places}"] for g in range(table.n_groups)]
    res["weighted_mean_acc"] = (np.array(indiv) * np.array(train_group_ratio)).sum()
    return loss_sum.item() / n, int(c[:, 1].sum()) / int(c[:, 0].sum()), {k: np.round(res[k], 4) for k in NEW_ORDER_FOR_PRINT}


def train_all_epochs(opt, train_table, val_table, test_table, input_dim=None, log=None):
    """The training schedule of the reference's driver (final_main.py:805-1046) -- `linear_probing` and `adapter_reg`
    (_train_linear_probing / _train_adapter_reg below), and the adapter methods `adapter`, `adapter_reg_seq`, `adapter_reg_seq_alter`,
    with or without `--add_adapter`, `--balance_val`, `--continue_from_best` -- on device-resident tables, every step one fused C call:

      stage 1 (epoch <= epochs_feature_learning): train_one_epoch on the train split (:935), lr by adjust_learning_rate + warm-up;
      switch (epoch == efl + 1): restart from the best model so far (:941-943), MultipleAdapter over it with a fresh Adapter and
          set_optimizer_reg (fresh momentum) (:945-950);
      stage 2: train_reg_seq_one_epoch on the reg half of the validation split -- re-balanced per epoch by balance_val (:920-921)
          from the global numpy RNG, else shuffled like its DataLoader -- odd epochs on the class prompts, even epochs on the group
          prompts with group labels (`_alter`, :954-968), warm-up from the stage's own epoch count (:607);
      every epoch: validate on the other half of the validation split, keep a deepcopy of the best worst-group model (:1001-1008),
          validate on the test split (:1013-1016); finally zero-shot class / spurious scores of the best model (:1037-1045).

    `opt` = the namespace of the reference's parse_option (same field names).  Random streams are consumed like the reference does
    (global torch RNG: parameter initialisation and DataLoader orders; global numpy RNG: balance_val), so the same seeds give the same
    initial weights and batches.  Returns ((best train, best val, best test group-accuracy dicts), (zero-shot class, zero-shot
    spurious)) like the reference; `log` (a list) receives one record per train / validate pass."""
    from copy import deepcopy

    from . import optim as O
    if opt.tl_method == "linear_probing":
        return _train_linear_probing(opt, train_table, val_table, test_table, input_dim, log)
    if opt.tl_method == "adapter_reg":
        return _train_adapter_reg(opt, train_table, val_table, test_table, input_dim, log)
    if opt.tl_method not in ("adapter", "adapter_reg_seq", "adapter_reg_seq_alter"):
        raise ValueError(f"train_all_epochs covers linear_probing and the adapter methods, not tl_method={opt.tl_method!r}")
    two_stage = opt.tl_method != "adapter"
    dev = train_table.device
    D = input_dim or train_table.embeddings.shape[1]
    reg_idx = val_idx = None
    if two_stage:                                                         # load_*_embeddings: stratified 50/50 split of the val split
        reg_idx, val_idx = adapter.stratified_split_indices(val_table.group_array, 0.5)
    ratio = train_table.group_ratio.numpy()
    rec = (lambda **k: log.append(k)) if log is not None else (lambda **k: None)

    classifier = adapter.CustomCLIP(adapter.Adapter(D, opt.adapter_feat_dim), opt.text_embedding_dir, opt.text_spurious_embedding_dir,
                                    opt.text_group_embedding_dir, temperature=opt.zs_temperature)
    rec(kind="init", state={k: v.clone() for k, v in classifier.adapter.state_dict().items()})
    classifier = classifier.to(dev)
    optimizer = O.set_optimizer(opt, classifier)
    multiple_adapter = optimizer_reg = best_model = None
    best_acc, best_epoch = 0, 0
    train_accs, val_accs, test_accs = [], [], []
    # the reference evaluates in batches of batch_size_reg (as few as 4 rows: load_*_embeddings' bs_val); eval-mode scores do not
    # depend on the batch size, so evaluation runs in large batches -- one pass still advances the random stream once, like a loader
    bs_eval = max(opt.batch_size_reg if two_stage else opt.batch_size, 4096)
    efl = getattr(opt, "epochs_feature_learning", None) if two_stage else None
    for epoch in range(1, opt.epochs + 1):
        O.adjust_learning_rate(opt, optimizer, epoch)
        balanced = None
        if two_stage and opt.balance_val:                                # a fresh balanced subset every epoch, also in stage 1 (:920-921)
            balanced, bs_reg = adapter.balance_val_indices(val_table.group_array[reg_idx], val_table.n_groups, opt.batch_size_reg)
        st = {}
        stage2 = two_stage and epoch > efl
        if not stage2:
            hook = lambda i, n, e=epoch: O.warmup_learning_rate(opt, e, i, n, optimizer)
            loss, acc, gacc = train_epoch(train_table, classifier, optimizer, opt.batch_size, target=opt.train_target, lr_hook=hook, stats=st)
            rec(kind="train1", epoch=epoch, loss=loss, acc=acc, group_acc=gacc, **st)
        else:
            if epoch == efl + 1:
                if opt.continue_from_best:
                    classifier = deepcopy(best_model)
                if opt.add_adapter:
                    new_adapter = adapter.Adapter(D, opt.adapter_feat_dim)
                    rec(kind="init", state={k: v.clone() for k, v in new_adapter.state_dict().items()})
                    multiple_adapter = adapter.MultipleAdapter(classifier, new_adapter, init_near_identity=opt.init_near_identity,
                                                               ebd_weight=0.5).to(dev)
                    optimizer_reg = O.set_optimizer_reg(opt, multiple_adapter)
                else:
                    optimizer_reg = O.set_optimizer_reg(opt, classifier)
            O.adjust_learning_rate_reg(opt, optimizer_reg, epoch)
            model = multiple_adapter if opt.add_adapter else classifier
            if opt.tl_method == "adapter_reg_seq_alter":
                use_group = (epoch % 2) == 0
            else:
                use_group = not opt.use_cls_prompt_in_reg
            hook = lambda i, n, e=epoch: O.warmup_learning_rate_reg(opt, e - efl, i, n, optimizer_reg)
            if balanced is not None:                                     # DataLoader(balanced_subset, shuffle=False, batch_size=adjusted)
                rows, shuffle, bs = reg_idx[balanced], False, bs_reg
            else:                                                        # the reg loader itself: shuffle=True
                rows, shuffle, bs = reg_idx, True, opt.batch_size_reg
            loss, acc, gacc = train_epoch(val_table, model, optimizer_reg, bs, target=opt.train_target, use_group=use_group, indices=rows,
                                          shuffle=shuffle, lr_hook=hook, stats=st)
            rec(kind="train2", epoch=epoch, use_group=use_group, loss=loss, acc=acc, group_acc=gacc, **st)
        train_accs.append(gacc)
        model = multiple_adapter if (stage2 and opt.add_adapter) else classifier
        st = {}
        vloss, vacc, vg = validate(val_table, model, bs_eval, ratio, target=opt.train_target, indices=val_idx, stats=st)
        rec(kind="validate", epoch=epoch, split="val", loss=vloss, acc=vacc, group_acc=vg, **st)
        val_accs.append(vg)
        if vg["worst_acc"] > best_acc:
            best_acc, best_epoch, best_model = vg["worst_acc"], epoch, deepcopy(model)
        st = {}
        tloss, tacc, tg = validate(test_table, model, bs_eval, ratio, target="class", stats=st)
        rec(kind="validate", epoch=epoch, split="test", loss=tloss, acc=tacc, group_acc=tg, **st)
        test_accs.append(tg)
    st = {}
    zs = validate(test_table, best_model, bs_eval, ratio, target="class", stats=st)
    rec(kind="validate_zs", target="class", loss=zs[0], acc=zs[1], group_acc=zs[2], **st)
    st = {}
    zss = validate(test_table, best_model, bs_eval, ratio, target="spurious", spurious=True, stats=st)
    rec(kind="validate_zs", target="spurious", loss=zss[0], acc=zss[1], group_acc=zss[2], **st)
    rec(kind="final", best_epoch=best_epoch, best_model=best_model)
    return (train_accs[best_epoch - 1], val_accs[best_epoch - 1], test_accs[best_epoch - 1]), (zs[2], zss[2])


def _select_and_finish(rec, train_accs, val_accs, test_accs, best_epoch, best_model, zs, zss):
    """records the zero-shot pair ((loss, acc, group acc, stats) each) and returns what train_all_epochs returns"""
    rec(kind="validate_zs", target="class", loss=zs[0], acc=zs[1], group_acc=zs[2], **zs[3])
    rec(kind="validate_zs", target="spurious", loss=zss[0], acc=zss[1], group_acc=zss[2], **zss[3])
    rec(kind="final", best_epoch=best_epoch, best_model=best_model)
    return (train_accs[best_epoch - 1], val_accs[best_epoch - 1], test_accs[best_epoch - 1]), (zs[2], zss[2])


def _train_linear_probing(opt, train_table, val_table, test_table, input_dim, log):
    """tl_method linear_probing (the reference's default): set_model's LinearClassifier(D, n_cls) (final_main.py:306-308), drawn on
    the CPU from the global torch RNG, trained by train_one_epoch on the plain loaders (no reg split), validated on the WHOLE val
    split, the best worst-group model kept; the zero-shot pair is validate_zs's linear_probing branch (raw embeddings against the
    class / spurious prompts: the CLIP baseline, independent of the trained head)."""
    from copy import deepcopy

    from . import optim as O
    dev = train_table.device
    D = input_dim or train_table.embeddings.shape[1]
    ratio = train_table.group_ratio.numpy()
    rec = (lambda **k: log.append(k)) if log is not None else (lambda **k: None)
    classifier = adapter.LinearClassifier(D, opt.n_cls)
    rec(kind="init", state={k: v.clone() for k, v in classifier.state_dict().items()})
    classifier = classifier.to(dev)
    optimizer = O.set_optimizer(opt, classifier)
    best_acc, best_epoch, best_model = 0, 0, None
    train_accs, val_accs, test_accs = [], [], []
    bs_eval = max(opt.batch_size, 4096)
    for epoch in range(1, opt.epochs + 1):
        O.adjust_learning_rate(opt, optimizer, epoch)
        st = {}
        hook = lambda i, n, e=epoch: O.warmup_learning_rate(opt, e, i, n, optimizer)
        loss, acc, gacc = train_epoch(train_table, classifier, optimizer, opt.batch_size, target=opt.train_target, lr_hook=hook, stats=st)
        rec(kind="train1", epoch=epoch, loss=loss, acc=acc, group_acc=gacc, **st)
        train_accs.append(gacc)
        st = {}
        vloss, vacc, vg = validate(val_table, classifier, bs_eval, ratio, target=opt.train_target, stats=st)
        rec(kind="validate", epoch=epoch, split="val", loss=vloss, acc=vacc, group_acc=vg, **st)
        val_accs.append(vg)
        if vg["worst_acc"] > best_acc:
            best_acc, best_epoch, best_model = vg["worst_acc"], epoch, deepcopy(classifier)
        st = {}
        tloss, tacc, tg = validate(test_table, classifier, bs_eval, ratio, target="class", stats=st)
        rec(kind="validate", epoch=epoch, split="test", loss=tloss, acc=tacc, group_acc=tg, **st)
        test_accs.append(tg)
    st, sts = {}, {}
    zs = validate_zs_linear_probing(test_table, opt.text_embedding_dir, opt.zs_temperature, bs_eval, ratio, target="class", stats=st)
    zss = validate_zs_linear_probing(test_table, opt.text_spurious_embedding_dir, opt.zs_temperature, bs_eval, ratio, target="spurious",
                                     stats=sts)
    return _select_and_finish(rec, train_accs, val_accs, test_accs, best_epoch, best_model, zs + (st,), zss + (sts,))


def _train_adapter_reg(opt, train_table, val_table, test_table, input_dim, log):
    """tl_method adapter_reg: one CustomCLIP(Adapter) and one optimiser for the whole run; every epoch is train_reg_one_epoch
    (final_main.py:498-569, called at :924-931): the train split on the class prompts, then the reg half of the val split -- re-balanced
    per epoch by balance_val (global numpy RNG; DataLoader(shuffle=False) with the adjusted batch) or the reg loader itself (shuffled,
    batch_size_reg) -- on the group prompts with group labels, or on the class prompts under --use_cls_prompt_in_reg.  lr by
    adjust_learning_rate and warmup_learning_rate, whose batch index and count restart with each loader.  Validation on the other half."""
    from copy import deepcopy

    from . import optim as O
    dev = train_table.device
    D = input_dim or train_table.embeddings.shape[1]
    reg_idx, val_idx = adapter.stratified_split_indices(val_table.group_array, 0.5)
    ratio = train_table.group_ratio.numpy()
    rec = (lambda **k: log.append(k)) if log is not None else (lambda **k: None)
    classifier = adapter.CustomCLIP(adapter.Adapter(D, opt.adapter_feat_dim), opt.text_embedding_dir, opt.text_spurious_embedding_dir,
                                    opt.text_group_embedding_dir, temperature=opt.zs_temperature)
    rec(kind="init", state={k: v.clone() for k, v in classifier.adapter.state_dict().items()})
    classifier = classifier.to(dev)
    optimizer = O.set_optimizer(opt, classifier)
    best_acc, best_epoch, best_model = 0, 0, None
    train_accs, val_accs, test_accs = [], [], []
    bs_eval = max(opt.batch_size_reg, 4096)
    use_group = not opt.use_cls_prompt_in_reg
    for epoch in range(1, opt.epochs + 1):
        O.adjust_learning_rate(opt, optimizer, epoch)
        if opt.balance_val:                                              # DataLoader(balanced_subset, shuffle=False, batch_size=adjusted)
            balanced, bs_reg = adapter.balance_val_indices(val_table.group_array[reg_idx], val_table.n_groups, opt.batch_size_reg)
            rows, shuffle, bs = reg_idx[balanced], False, bs_reg
        else:                                                            # the reg loader itself: shuffle=True
            rows, shuffle, bs = reg_idx, True, opt.batch_size_reg
        st = {}
        hook = lambda i, n, e=epoch: O.warmup_learning_rate(opt, e, i, n, optimizer)
        loss, acc, gacc = train_reg_epoch(train_table, val_table, classifier, optimizer, opt.batch_size, rows, bs, shuffle,
                                          target=opt.train_target, group_prompt=use_group, lr_hook=hook, stats=st)
        rec(kind="train_reg", epoch=epoch, use_group=use_group, loss=loss, acc=acc, group_acc=gacc, **st)
        train_accs.append(gacc)
        st = {}
        vloss, vacc, vg = validate(val_table, classifier, bs_eval, ratio, target=opt.train_target, indices=val_idx, stats=st)
        rec(kind="validate", epoch=epoch, split="val", loss=vloss, acc=vacc, group_acc=vg, **st)
        val_accs.append(vg)
        if vg["worst_acc"] > best_acc:
            best_acc, best_epoch, best_model = vg["worst_acc"], epoch, deepcopy(classifier)
        st = {}
        tloss, tacc, tg = validate(test_table, classifier, bs_eval, ratio, target="class", stats=st)
        rec(kind="validate", epoch=epoch, split="test", loss=tloss, acc=tacc, group_acc=tg, **st)
        test_accs.append(tg)
    st, sts = {}, {}
    zs = validate(test_table, best_model, bs_eval, ratio, target="class", stats=st)
    zss = validate(test_table, best_model, bs_eval, ratio, target="spurious", spurious=True, stats=sts)
    return _select_and_finish(rec, train_accs, val_accs, test_accs, best_epoch, best_model, zs + (st,), zss + (sts,))


# ---------------------------------------------------------------------------------------------------------------------
# seed sweeps (run_multiple/final_main_iteration_wb.py, final_main_iteration_ca.py): R runs in lock-step, one launch for all
# ---------------------------------------------------------------------------------------------------------------------

class ReplicaStreams:
    """The global torch and numpy random streams of R runs that advance in lock-step.  In the reference each seed's run owns the
    two global streams from set_seed to its end; here every replica keeps its own saved pair of states, swapped in around each
    host-side draw: `run(r, fn, *args)` calls fn with replica r's streams installed and saves them again.  The draws themselves
    are the ordinary functions (module constructors, dataloader_shuffle_order, balance_val_indices), unchanged."""

    def __init__(self, seeds):
        from . import optim as O
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


def _sweep_replicas(opt, seeds, learning_rates):
    """(opt of the replica, seed) pairs, learning-rate-major like final_main_iteration_ca.py's loops"""
    from copy import copy
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


def _eval_results(table, c, loss_sum, n, ratio):
    """the tail of validate() from the counters of one replica"""
    res = _results(c, table.n_places)
    indiv = [res[f"acc_{g // table.n_places}_{g % table.n_places}"] for g in range(table.n_groups)]
    res["weighted_mean_acc"] = (np.array(indiv) * np.array(ratio)).sum()
    group_acc = {k: np.round(res[k], 4) for k in NEW_ORDER_FOR_PRINT}
    return loss_sum / n, int(c[:, 1].sum()) / int(c[:, 0].sum()), group_acc


def _sweep_train_pass(streams, sweep, table, orders_fn, batch_size, target, use_group, lr_fn, momentum, weight_decay, counted=True, acc=None,
                      sync=True):
    """one loader pass of every replica: `orders_fn(r)` draws replica r's row order (under its own streams), all orders go to the
    device in ONE upload, then n_steps batched steps; lr_fn(step, n_steps) -> the R learning rates.  `sweep`: SweepAdapters (scored on
    the group prompts when `use_group`, else the class prompts) or SweepLinear.  `counted`: the pass adds to the loss sums and group
    counters; `acc` = (counts, loss sums) device tensors of an epoch made of several passes (fresh ones if None).  Returns (counts
    [R, G, 2] numpy, loss sums [R] numpy, orders, acc) after the pass's one host sync; the two arrays are None without `sync`."""
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
    for i, b in enumerate(steps):
        sweep.step(table.embeddings, b, labels, table.targets_group, *prompts, lr_fn(i, len(steps)), momentum, weight_decay, counts, loss_sum,
                   counted=counted)
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
            streams.run(r, lambda: torch.empty((), dtype=torch.int64).random_())
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


def train_sweep(opt, train_table, val_table, test_table, seeds, learning_rates=None, log=None):
    """A seed sweep as one batched run: returns, per replica, exactly what `train_all_epochs` returns for that replica run alone
    after `optim.set_seed(seed)`.  Replicas are (learning rate, seed) pairs, learning-rate-major; with `learning_rates` given,
    replica (lr, seed) runs with learning_rate = lr and learning_rate_reg = lr * opt.lr_multiple, like final_main_iteration_ca.py.

    Batched path -- at least two replicas and
      * tl_method `adapter`, `adapter_reg_seq`, `adapter_reg_seq_alter`, with or without --add_adapter, --balance_val,
        --continue_from_best, --init_near_identity (the main branch of train_all_epochs), and `adapter_reg` (with or without
        --balance_val, --use_cls_prompt_in_reg), on the adapter's fast shape (hidden width 128, D % 128 == 0): adapter.SweepAdapters;
      * tl_method `linear_probing` with n_cls <= 8, D % 4 == 0 and D <= 1024: adapter.SweepLinear.
    All replicas advance in lock-step, every training step and every evaluation batch is one replica-batched call (up to 16 replicas
    per group of launches, more are split into groups), each pass uploads its row orders once and synchronises with the host once,
    best-model selection runs per replica on the host.
    Sequential path -- other shapes and a single replica: replica by replica through train_all_epochs on the same tables.
    `contrastive_adapter` raises like train_all_epochs.

    Each replica keeps its own pair of global random streams (ReplicaStreams), so its initial weights, batch orders and balanced
    subsets are those of its own sequential run.  `log` (a list) receives one list of records per replica (train_all_epochs' records)."""
    from . import optim as O
    replicas = _sweep_replicas(opt, list(seeds), learning_rates)
    D = train_table.embeddings.shape[1]
    if opt.tl_method == "linear_probing":
        group, batched = _train_linear_sweep_group, len(replicas) >= 2 and 1 <= opt.n_cls <= 8 and D % 4 == 0 and D <= 1024
    else:
        group = _train_adapter_reg_sweep_group if opt.tl_method == "adapter_reg" else _train_sweep_group
        batched = (opt.tl_method in ("adapter", "adapter_reg", "adapter_reg_seq", "adapter_reg_seq_alter") and len(replicas) >= 2
                   and opt.adapter_feat_dim == 128 and D % 128 == 0 and bool(ops.get_option("adapter_step_fused")))
    if opt.tl_method not in ("adapter", "adapter_reg_seq", "adapter_reg_seq_alter", "adapter_reg", "linear_probing"):
        raise ValueError(f"train_sweep covers linear_probing and the adapter methods, not tl_method={opt.tl_method!r}")
    if not batched:
        out = []
        for o, s in replicas:
            O.set_seed(s)
            lg = [] if log is not None else None
            out.append(train_all_epochs(o, train_table, val_table, test_table, log=lg))
            if log is not None:
                log.append(lg)
        return out
    out = []
    for i in range(0, len(replicas), 16):
        out += group(replicas[i:i + 16], train_table, val_table, test_table, log)
    return out


def _train_sweep_group(replicas, train_table, val_table, test_table, log):
    """train_all_epochs' main branch for up to 16 replicas in lock-step; statement for statement the sequential schedule, with
    every per-replica host decision (learning rate, best model) taken per replica"""
    from . import optim as O
    opts = [o for o, _ in replicas]
    opt = opts[0]
    R = len(replicas)
    two_stage = opt.tl_method != "adapter"
    dev = train_table.device
    D = train_table.embeddings.shape[1]
    reg_idx = val_idx = val_idx_dev = None
    if two_stage:
        reg_idx, val_idx = adapter.stratified_split_indices(val_table.group_array, 0.5)
        val_idx_dev = torch.as_tensor(val_idx, dtype=torch.int64).to(dev)
    n_val = len(val_table) if val_idx is None else len(val_idx)
    ratio = train_table.group_ratio.numpy()
    logs = [[] for _ in range(R)]
    rec = lambda r, **k: logs[r].append(k)
    streams = ReplicaStreams([s for _, s in replicas])

    def new_clip():
        return adapter.CustomCLIP(adapter.Adapter(D, opt.adapter_feat_dim), opt.text_embedding_dir, opt.text_spurious_embedding_dir,
                                  opt.text_group_embedding_dir, temperature=opt.zs_temperature)
    mods = [streams.run(r, new_clip) for r in range(R)]
    for r in range(R):
        rec(r, kind="init", state={k: v.clone() for k, v in mods[r].adapter.state_dict().items()})
    sweep = adapter.SweepAdapters.from_modules(mods, dev)
    lr1 = [_Lr(o.learning_rate) for o in opts]
    lr2 = None
    best_acc, best_epoch = [0] * R, [0] * R
    train_accs, val_accs, test_accs = [[] for _ in range(R)], [[] for _ in range(R)], [[] for _ in range(R)]
    bs_eval = max(opt.batch_size_reg if two_stage else opt.batch_size, 4096)
    efl = getattr(opt, "epochs_feature_learning", None) if two_stage else None
    for epoch in range(1, opt.epochs + 1):
        for r in range(R):
            O.adjust_learning_rate(opts[r], lr1[r], epoch)
        balanced = None
        if two_stage and opt.balance_val:
            balanced = [streams.run(r, adapter.balance_val_indices, val_table.group_array[reg_idx], val_table.n_groups, opt.batch_size_reg)
                        for r in range(R)]
        stage2 = two_stage and epoch > efl
        if not stage2:
            def lrs(i, n, e=epoch):
                for r in range(R):
                    O.warmup_learning_rate(opts[r], e, i, n, lr1[r])
                return [l.lr for l in lr1]
            n_train = len(train_table)
            c, ls, orders, _ = _sweep_train_pass(streams, sweep, train_table, lambda r: dataloader_shuffle_order(n_train), opt.batch_size,
                                                 opt.train_target, False, lrs, opt.momentum, opt.weight_decay)
            kind, extra, n_rows = "train1", {}, n_train
        else:
            if epoch == efl + 1:
                if opt.continue_from_best:
                    sweep.restore([True] * R)
                if opt.add_adapter:
                    fresh = [streams.run(r, adapter.Adapter, D, opt.adapter_feat_dim) for r in range(R)]
                    for r in range(R):
                        rec(r, kind="init", state={k: v.clone() for k, v in fresh[r].state_dict().items()})
                    sweep.add_adapters(fresh, opt.init_near_identity)
                else:
                    sweep.reset_optimizer()
                lr2 = [_Lr(o.learning_rate_reg) for o in opts]
            for r in range(R):
                O.adjust_learning_rate_reg(opts[r], lr2[r], epoch)
            if opt.tl_method == "adapter_reg_seq_alter":
                use_group = (epoch % 2) == 0
            else:
                use_group = not opt.use_cls_prompt_in_reg

            def lrs(i, n, e=epoch):
                for r in range(R):
                    O.warmup_learning_rate_reg(opts[r], e - efl, i, n, lr2[r])
                return [l.lr for l in lr2]
            if balanced is not None:
                bs = balanced[0][1]

                def order(r):
                    torch.empty((), dtype=torch.int64).random_()             # the un-shuffled loader's base-seed draw
                    return torch.as_tensor(np.asarray(reg_idx[balanced[r][0]]), dtype=torch.int64)
            else:
                bs = opt.batch_size_reg

                def order(r):
                    return torch.as_tensor(np.asarray(reg_idx), dtype=torch.int64)[dataloader_shuffle_order(len(reg_idx))]
            c, ls, orders, _ = _sweep_train_pass(streams, sweep, val_table, order, bs, opt.train_target, use_group, lrs, opt.momentum,
                                                 opt.weight_decay)
            kind, extra, n_rows = "train2", {"use_group": use_group}, len(orders[0])
        for r in range(R):
            total = int(c[r][:, 0].sum())
            res = _results(c[r], train_table.n_places)
            gacc = {k: np.round(res[k], 4) for k in NEW_ORDER_FOR_PRINT[1:]}
            rec(r, kind=kind, epoch=epoch, loss=float(ls[r]) / n_rows, acc=int(c[r][:, 1].sum()) / total, group_acc=gacc, counts=c[r],
                order=orders[r], **extra)
            train_accs[r].append(gacc)
        vc, vl = _sweep_validate(streams, sweep, val_table, bs_eval, opt.train_target, val_idx_dev, n_val)
        better = [False] * R
        for r in range(R):
            vloss, vacc, vg = _eval_results(val_table, vc[r], float(vl[r]), n_val, ratio)
            rec(r, kind="validate", epoch=epoch, split="val", loss=vloss, acc=vacc, group_acc=vg, counts=vc[r])
            val_accs[r].append(vg)
            if vg["worst_acc"] > best_acc[r]:
                best_acc[r], best_epoch[r], better[r] = vg["worst_acc"], epoch, True
        sweep.snapshot(better)
        tc, tl = _sweep_validate(streams, sweep, test_table, bs_eval, "class", None, len(test_table))
        for r in range(R):
            tloss, tacc, tg = _eval_results(test_table, tc[r], float(tl[r]), len(test_table), ratio)
            rec(r, kind="validate", epoch=epoch, split="test", loss=tloss, acc=tacc, group_acc=tg, counts=tc[r])
            test_accs[r].append(tg)
    if not all(sweep.has_best):
        raise RuntimeError("train_sweep: a replica never had a worst-group accuracy above 0, so it has no best model")
    # zero-shot scores of the best models: both kinds may occur in one sweep (a best epoch before / after the adapters were added)
    zs, zss = [None] * R, [None] * R
    for _ in range(2):                                                        # two validate passes: every replica's stream advances twice
        for r in range(R):
            streams.run(r, lambda: torch.empty((), dtype=torch.int64).random_())
    for kind in (False, True):
        rs = [r for r in range(R) if sweep.best_has_old[r] == kind]
        if not rs:
            continue
        whole = len(rs) == R
        sub = sweep if whole else sweep.subset(rs, best=True)
        for spurious, dst in ((False, zs), (True, zss)):
            cc, ll = _sweep_validate(streams, sub, test_table, bs_eval, "spurious" if spurious else "class", None, len(test_table),
                                     spurious=spurious, best=whole, draw=False)
            for k, r in enumerate(rs):
                dst[r] = _eval_results(test_table, cc[k], float(ll[k]), len(test_table), ratio) + (cc[k],)
    out = []
    for r in range(R):
        rec(r, kind="validate_zs", target="class", loss=zs[r][0], acc=zs[r][1], group_acc=zs[r][2], counts=zs[r][3])
        rec(r, kind="validate_zs", target="spurious", loss=zss[r][0], acc=zss[r][1], group_acc=zss[r][2], counts=zss[r][3])
        # the best model as an ordinary module is only built for a caller who asked for the records (a host-side copy per replica)
        rec(r, kind="final", best_epoch=best_epoch[r], best_model=sweep.replica(r, best=True) if log is not None else None)
        e = best_epoch[r] - 1
        out.append(((train_accs[r][e], val_accs[r][e], test_accs[r][e]), (zs[r][2], zss[r][2])))
    if log is not None:
        log.extend(logs)
    return out


def _sweep_finish(R, logs, log, best_epoch, best_model_fn, train_accs, val_accs, test_accs, zs, zss):
    """the tail of a lock-step schedule: the zero-shot pair ((loss, acc, group acc, counts) per replica) and the final record of every
    replica, and what train_all_epochs returns for each"""
    out = []
    for r in range(R):
        logs[r].append(dict(kind="validate_zs", target="class", loss=zs[r][0], acc=zs[r][1], group_acc=zs[r][2], counts=zs[r][3]))
        logs[r].append(dict(kind="validate_zs", target="spurious", loss=zss[r][0], acc=zss[r][1], group_acc=zss[r][2], counts=zss[r][3]))
        # the best model as an ordinary module is only built for a caller who asked for the records (a host-side copy per replica)
        logs[r].append(dict(kind="final", best_epoch=best_epoch[r], best_model=best_model_fn(r) if log is not None else None))
        e = best_epoch[r] - 1
        out.append(((train_accs[r][e], val_accs[r][e], test_accs[r][e]), (zs[r][2], zss[r][2])))
    if log is not None:
        log.extend(logs)
    return out


def _sweep_epoch_tail(streams, sweep, epoch, rec, val_table, test_table, bs_eval, target, val_idx_dev, n_val, ratio, best_acc, best_epoch,
                      val_accs, test_accs):
    """what every schedule does after an epoch's training: validate, strict `>` best-model selection per replica, test"""
    R = sweep.R
    vc, vl = _sweep_validate(streams, sweep, val_table, bs_eval, target, val_idx_dev, n_val)
    better = [False] * R
    for r in range(R):
        vloss, vacc, vg = _eval_results(val_table, vc[r], float(vl[r]), n_val, ratio)
        rec(r, kind="validate", epoch=epoch, split="val", loss=vloss, acc=vacc, group_acc=vg, counts=vc[r])
        val_accs[r].append(vg)
        if vg["worst_acc"] > best_acc[r]:
            best_acc[r], best_epoch[r], better[r] = vg["worst_acc"], epoch, True
    sweep.snapshot(better)
    tc, tl = _sweep_validate(streams, sweep, test_table, bs_eval, "class", None, len(test_table))
    for r in range(R):
        tloss, tacc, tg = _eval_results(test_table, tc[r], float(tl[r]), len(test_table), ratio)
        rec(r, kind="validate", epoch=epoch, split="test", loss=tloss, acc=tacc, group_acc=tg, counts=tc[r])
        test_accs[r].append(tg)


def _train_linear_sweep_group(replicas, train_table, val_table, test_table, log):
    """_train_linear_probing for up to 16 replicas in lock-step: statement for statement the sequential schedule, every per-replica
    host decision (initial weights, shuffle order, learning rate, best model) taken per replica"""
    from . import optim as O
    opts = [o for o, _ in replicas]
    opt = opts[0]
    R = len(replicas)
    dev = train_table.device
    D = train_table.embeddings.shape[1]
    ratio = train_table.group_ratio.numpy()
    logs = [[] for _ in range(R)]
    rec = lambda r, **k: logs[r].append(k)
    streams = ReplicaStreams([s for _, s in replicas])
    mods = [streams.run(r, adapter.LinearClassifier, D, opt.n_cls) for r in range(R)]
    for r in range(R):
        rec(r, kind="init", state={k: v.clone() for k, v in mods[r].state_dict().items()})
    sweep = adapter.SweepLinear.from_modules(mods, dev)
    lr1 = [_Lr(o.learning_rate) for o in opts]
    best_acc, best_epoch = [0] * R, [0] * R
    train_accs, val_accs, test_accs = [[] for _ in range(R)], [[] for _ in range(R)], [[] for _ in range(R)]
    bs_eval = max(opt.batch_size, 4096)
    n_train = len(train_table)
    for epoch in range(1, opt.epochs + 1):
        for r in range(R):
            O.adjust_learning_rate(opts[r], lr1[r], epoch)

        def lrs(i, n, e=epoch):
            for r in range(R):
                O.warmup_learning_rate(opts[r], e, i, n, lr1[r])
            return [l.lr for l in lr1]
        c, ls, orders, _ = _sweep_train_pass(streams, sweep, train_table, lambda r: dataloader_shuffle_order(n_train), opt.batch_size,
                                             opt.train_target, False, lrs, opt.momentum, opt.weight_decay)
        for r in range(R):
            res = _results(c[r], train_table.n_places)
            gacc = {k: np.round(res[k], 4) for k in NEW_ORDER_FOR_PRINT[1:]}
            rec(r, kind="train1", epoch=epoch, loss=float(ls[r]) / n_train, acc=int(c[r][:, 1].sum()) / int(c[r][:, 0].sum()), group_acc=gacc,
                counts=c[r], order=orders[r])
            train_accs[r].append(gacc)
        _sweep_epoch_tail(streams, sweep, epoch, rec, val_table, test_table, bs_eval, opt.train_target, None, len(val_table), ratio, best_acc,
                          best_epoch, val_accs, test_accs)
    # a replica whose worst-group accuracy never rose above 0 has best_epoch 0 and no best model, like its sequential run
    # validate_zs's linear_probing branch scores the raw embeddings against the prompts: no trained head in it, so one computation
    # serves every replica; every replica's stream still advances by the two loader passes its own run would make
    st, sts = {}, {}
    zs = streams.run(0, validate_zs_linear_probing, test_table, opt.text_embedding_dir, opt.zs_temperature, bs_eval, ratio, target="class",
                     stats=st)
    zss = streams.run(0, validate_zs_linear_probing, test_table, opt.text_spurious_embedding_dir, opt.zs_temperature, bs_eval, ratio,
                      target="spurious", stats=sts)
    for _ in range(2):
        for r in range(1, R):
            streams.run(r, lambda: torch.empty((), dtype=torch.int64).random_())
    return _sweep_finish(R, logs, log, best_epoch, lambda r: sweep.replica(r, best=True), train_accs, val_accs, test_accs,
                         [zs + (st["counts"],)] * R, [zss + (sts["counts"],)] * R)


def _train_adapter_reg_sweep_group(replicas, train_table, val_table, test_table, log):
    """_train_adapter_reg for up to 16 replicas in lock-step on SweepAdapters: per epoch the train pass on the class prompts, then the
    reg pass with the same momentum buffers -- the warm-up step index and count restart with each pass -- counted only when it runs
    on the class prompts; one sync per epoch"""
    from . import optim as O
    opts = [o for o, _ in replicas]
    opt = opts[0]
    R = len(replicas)
    dev = train_table.device
    D = train_table.embeddings.shape[1]
    reg_idx, val_idx = adapter.stratified_split_indices(val_table.group_array, 0.5)
    val_idx_dev = torch.as_tensor(val_idx, dtype=torch.int64).to(dev)
    ratio = train_table.group_ratio.numpy()
    logs = [[] for _ in range(R)]
    rec = lambda r, **k: logs[r].append(k)
    streams = ReplicaStreams([s for _, s in replicas])

    def new_clip():
        return adapter.CustomCLIP(adapter.Adapter(D, opt.adapter_feat_dim), opt.text_embedding_dir, opt.text_spurious_embedding_dir,
                                  opt.text_group_embedding_dir, temperature=opt.zs_temperature)
    mods = [streams.run(r, new_clip) for r in range(R)]
    for r in range(R):
        rec(r, kind="init", state={k: v.clone() for k, v in mods[r].adapter.state_dict().items()})
    sweep = adapter.SweepAdapters.from_modules(mods, dev)
    lr1 = [_Lr(o.learning_rate) for o in opts]
    best_acc, best_epoch = [0] * R, [0] * R
    train_accs, val_accs, test_accs = [[] for _ in range(R)], [[] for _ in range(R)], [[] for _ in range(R)]
    bs_eval = max(opt.batch_size_reg, 4096)
    use_group = not opt.use_cls_prompt_in_reg
    n_train = len(train_table)
    reg_rows = torch.as_tensor(np.asarray(reg_idx), dtype=torch.int64)
    for epoch in range(1, opt.epochs + 1):
        for r in range(R):
            O.adjust_learning_rate(opts[r], lr1[r], epoch)
        if opt.balance_val:                                              # DataLoader(balanced_subset, shuffle=False, batch_size=adjusted)
            balanced = [streams.run(r, adapter.balance_val_indices, val_table.group_array[reg_idx], val_table.n_groups, opt.batch_size_reg)
                        for r in range(R)]
            bs = balanced[0][1]

            def order(r):
                torch.empty((), dtype=torch.int64).random_()             # the un-shuffled loader's base-seed draw
                return torch.as_tensor(np.asarray(reg_idx[balanced[r][0]]), dtype=torch.int64)
        else:                                                            # the reg loader itself: shuffle=True
            bs = opt.batch_size_reg

            def order(r):
                return reg_rows[dataloader_shuffle_order(len(reg_idx))]

        def lrs(i, n, e=epoch):
            for r in range(R):
                O.warmup_learning_rate(opts[r], e, i, n, lr1[r])
            return [l.lr for l in lr1]
        _, _, o1, acc = _sweep_train_pass(streams, sweep, train_table, lambda r: dataloader_shuffle_order(n_train), opt.batch_size,
                                          opt.train_target, False, lrs, opt.momentum, opt.weight_decay, sync=False)
        c, ls, o2, _ = _sweep_train_pass(streams, sweep, val_table, order, bs, opt.train_target, use_group, lrs, opt.momentum,
                                         opt.weight_decay, counted=not use_group, acc=acc)
        n_rows = n_train + (0 if use_group else len(o2[0]))
        for r in range(R):
            res = _results(c[r], train_table.n_places)
            gacc = {k: np.round(res[k], 4) for k in NEW_ORDER_FOR_PRINT[1:]}
            rec(r, kind="train_reg", epoch=epoch, use_group=use_group, loss=float(ls[r]) / n_rows, acc=int(c[r][:, 1].sum()) / int(c[r][:, 0].sum()),
                group_acc=gacc, counts=c[r], order=np.concatenate([o1[r], o2[r]]), n_train_rows=n_train)
            train_accs[r].append(gacc)
        _sweep_epoch_tail(streams, sweep, epoch, rec, val_table, test_table, bs_eval, opt.train_target, val_idx_dev, len(val_idx), ratio, best_acc,
                          best_epoch, val_accs, test_accs)
    if not all(sweep.has_best):
        raise RuntimeError("train_sweep: a replica never had a worst-group accuracy above 0, so it has no best model")
    zs, zss = [None] * R, [None] * R
    for spurious, dst in ((False, zs), (True, zss)):
        cc, ll = _sweep_validate(streams, sweep, test_table, bs_eval, "spurious" if spurious else "class", None, len(test_table),
                                 spurious=spurious, best=True)
        for r in range(R):
            dst[r] = _eval_results(test_table, cc[r], float(ll[r]), len(test_table), ratio) + (cc[r],)
    return _sweep_finish(R, logs, log, best_epoch, lambda r: sweep.replica(r, best=True), train_accs, val_accs, test_accs, zs, zss)


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
    return name


def run_sweep(opt, tables, out_dir):
    """The two sweep drivers of the reference on device-resident tables (`tables` = (train, val, test) EmbeddingTables).
    With opt.lr_list / opt.bs_list / opt.bsr_list (comma-separated strings or sequences; final_main_iteration_ca.py:1167-1186) the
    (batch size, reg batch size) groups run one after the other and every group trains all lr_list x opt.random_seeds replicas as
    one batched sweep; without them it is final_main_iteration_wb.py: opt.random_seeds at opt's own settings.  Writes one CSV per
    (lr, bs, bsr) under `out_dir`, named like the reference's, and returns {file path: frame}."""
    import os
    from copy import copy

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
