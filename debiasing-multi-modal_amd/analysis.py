"""The numerical half of the reference's representation report (VisHandler.VisRepAll, demo/visualizer.py:182-222) on the device:
group-wise embedding statistics (GetGroupWiseStatEbd :657-690), group-wise confidences (GetGroupWiseStatConf :692-708), the
rows nearest to a prompt embedding (find_closest_sample :19-27), the 3 x 6 table per split, and the report's map (plot_umap :311-408)
as a PCA: the coordinates of every row, without the drawing (matplotlib) and without UMAP.

The reference's `Div.` row is scipy.cdist(X, X) summed: an N x N float64 matrix per split and per group, which its own notebook
switches off (return_dist=False) at CelebA's size.  Here it is one pass of the fused Gram-and-distance kernel
(ops.pairdist_group_sums): every pair is visited once and lands in its (group, group) bucket, nothing N x N is stored, and the
between-group mean distances come with it.
"""
import numpy as np
import torch

from . import ops, trainer

TABLE_INDEX = ["Acc.", "Div.", "Centr. Norm."]
TABLE_COLUMNS = ["Avg.", "Worst", "group0", "group1", "group2", "group3"]


def _need_device(x):
    if not torch.is_tensor(x) or not x.is_cuda:
        raise ops._lib.DbmmError("analysis works on device-resident embeddings (an EmbeddingTable or a HIP tensor); there is no CPU path")


def _labelled_rows(what, embeddings, labels, max_labels=None, min_labels=2, device="first"):
    """(x, unique labels, dense ids int64 [N], counts) of an EmbeddingTable (its targets_group unless `labels` is given) or a tensor
    [N, D] with `labels` [N]: any integers, through np.unique.  More than `max_labels` of them raise DbmmUnsupported, fewer than
    `min_labels` ValueError.  `device` says where the refusal of rows that are not device-resident falls: "first" -- before the
    labels are looked at, and the labels must then be one-dimensional --, "last" -- after every refusal of the labels --, or None:
    left to a caller that has refusals of its own to make first (_need_device)."""
    if isinstance(embeddings, trainer.EmbeddingTable):
        x = embeddings.embeddings
        labels = embeddings.targets_group if labels is None else labels
    else:
        x = embeddings
    if labels is None:
        raise ValueError(f"{what}: a device tensor of embeddings needs its labels array")
    if device == "first":
        _need_device(x)
    elif not torch.is_tensor(x) or x.dim() != 2:
        raise ValueError(f"{what}: the rows must be an EmbeddingTable or a tensor [N, D]")
    l_np = labels.detach().cpu().numpy() if torch.is_tensor(labels) else np.asarray(labels)
    if device != "first":
        l_np = l_np.ravel()
    if l_np.ndim != 1 or l_np.shape[0] != x.shape[0]:
        raise ValueError(f"{what}: labels of shape {l_np.shape} for {x.shape[0]} rows")
    uniq, dense, counts = np.unique(l_np, return_inverse=True, return_counts=True)
    if max_labels is not None and len(uniq) > max_labels:
        raise ops.DbmmUnsupported(f"{what}: {len(uniq)} labels; the kernel takes at most {max_labels}")
    if len(uniq) < min_labels:
        raise ValueError(f"{what} needs at least {min_labels} labels with rows, got {len(uniq)}")
    if device == "last":
        _need_device(x)
    return x, uniq, dense.reshape(-1).astype(np.int64), counts


TRANSFORM_ROWS = 4096     # rows per batch of `transform`


def _prepared(x, transform=None):
    """the rows as the kernels take them: fp32, contiguous, after `transform` (a callable emb -> emb, batch by batch in eval mode)"""
    x = x.float().contiguous()
    return x if transform is None else _transformed_rows(x, transform, TRANSFORM_ROWS)


def _resolved_gammas(x, gammas, scales):
    """the bandwidths of a call, float64 [L]: the caller's, or rbf_gammas(scales) of the prepared rows"""
    return rbf_gammas(x, scales) if gammas is None else np.asarray(gammas, dtype=np.float64).ravel()


SUM_ROWS = 512


def _column_sums(rows):
    """float64 [D] on the host: ops.colsum (fp32, fixed order) over blocks of SUM_ROWS rows, the blocks' sums added in float64 in
    block order.  A block's fp32 sum is good to ~1e-6 of it, and nothing the size of the rows is allocated: a float64 reduction in
    torch would first make a float64 copy of them."""
    acc = torch.zeros(rows.shape[1], dtype=torch.float64, device=rows.device)
    for i in range(0, rows.shape[0], SUM_ROWS):
        acc += ops.colsum(rows[i:i + SUM_ROWS])
    return acc.cpu().numpy()


def _sorted_pass(x, dense, kernel, per_row=False, extra=None, counts=None):
    """One pass of a pairwise kernel over the rows x sorted by their dense label (a stable sort and ONE gather: nearly every tile
    then holds one label), followed by the rows `extra` with label -1.  kernel(xs, ids, center) -> a device tensor; the centre is the
    fp32 mean of what is passed, from _column_sums of it -- with `counts`, of each label's slice, and those sums [G, D] are returned
    beside the result (group_stats' means).  The result comes back on the host, per_row: [..., N (+ M), G] in the INPUT's row order,
    x's rows first.  kernel None: the gather and the sums only."""
    order = np.argsort(dense, kind="stable")
    ids = dense[order]
    if extra is not None:
        order = np.concatenate([order, x.shape[0] + np.arange(extra.shape[0], dtype=np.int64)])
        ids = np.concatenate([ids, np.full(extra.shape[0], -1, dtype=np.int64)])
        x = torch.cat([x, extra])
    xs = ops.gather_rows(x, torch.from_numpy(order).to(x.device))
    if counts is None:
        sums = total = _column_sums(xs)
    else:
        bounds = np.concatenate([[0], np.cumsum(counts)])
        sums = np.stack([_column_sums(xs[bounds[k]:bounds[k + 1]]) for k in range(len(counts))])        # [G, D] float64, fixed order
        total = sums.sum(0)
    if kernel is None:
        return None, sums
    center = torch.from_numpy((total / xs.shape[0]).astype(np.float32)).to(x.device)
    out = kernel(xs, torch.from_numpy(ids.astype(np.int64)).to(x.device), center).cpu().numpy()
    if per_row:
        sorted_out, out = out, np.empty_like(out)
        out[..., order, :] = sorted_out
    return out, sums


def group_stats(embeddings, groups=None, return_dist=True):
    """GetGroupWiseStatEbd: {'mean_vector': {'full': v, g: v, ...}, 'mean_vector_norm': {...}, 'pairwise_distance': {...}} with the
    groups in np.unique order and numpy values; 'pairwise_distance' is sum over ordered pairs / (n (n - 1)) of the Euclidean distance
    (nan for a one-row group, the reference's 0 / 0) and stays empty with return_dist=False, which skips the kernel.  One more key
    than the reference: 'between_distance', float64 [G, G], the mean distance between a row of group a and a row of group b (the
    diagonal repeats 'pairwise_distance').

    `embeddings`: an EmbeddingTable (its targets_group unless `groups` is given) or a device tensor [N, D] with `groups` [N].
    The rows are sorted by group first (one gather), so that a group's mean is a slice's column sum and nearly every tile of the
    distance kernel holds one bucket."""
    x, uniq, dense, counts = _labelled_rows("group_stats", embeddings, groups, 8 if return_dist else None, min_labels=1)
    G, N = len(uniq), x.shape[0]
    kernel = (lambda xs, ids, center: ops.pairdist_group_sums(xs, ids, G, center)) if return_dist else None
    S, sums = _sorted_pass(_prepared(x), dense, kernel, counts=counts)
    mean_full = sums.sum(0) / N
    means = sums / counts.astype(np.float64)[:, None]
    norms = np.linalg.norm(np.concatenate([mean_full[None], means]), axis=1)
    stats = {"mean_vector": {"full": mean_full.astype(np.float32)}, "mean_vector_norm": {"full": np.float32(norms[0])},
             "pairwise_distance": {}}
    means_np = means.astype(np.float32)
    for k, g in enumerate(uniq):
        stats["mean_vector"][g] = means_np[k]
        stats["mean_vector_norm"][g] = np.float32(norms[k + 1])
    if not return_dist:
        return stats
    n = counts.astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        stats["pairwise_distance"]["full"] = 2.0 * np.triu(S).sum() / np.float64(N * (N - 1.0))
        within = 2.0 * np.diag(S) / (n * (n - 1.0))
        between = S / np.outer(n, n)
    for k, g in enumerate(uniq):
        stats["pairwise_distance"][g] = within[k]
    between[np.arange(G), np.arange(G)] = within
    stats["between_distance"] = between
    return stats


def group_conf_stats(confidences, groups):
    """GetGroupWiseStatConf: {'full': mean confidence, g: group g's mean, ...} in np.unique order, summed on the device in float64"""
    g_np = groups.detach().cpu().numpy() if torch.is_tensor(groups) else np.asarray(groups)
    conf = confidences if torch.is_tensor(confidences) else torch.as_tensor(np.asarray(confidences))
    if not conf.is_cuda:
        conf = conf.cuda()
    conf = conf.flatten()
    uniq, dense = np.unique(g_np, return_inverse=True)
    gd = torch.from_numpy(dense.astype(np.int64)).to(conf.device)
    onehot = gd.unsqueeze(0) == torch.arange(len(uniq), device=conf.device).unsqueeze(1)                 # [G, N]
    sums = torch.where(onehot, conf.double().unsqueeze(0), 0.0).sum(1)
    cnt = onehot.sum(1)
    out = {"full": np.float32((sums.sum() / conf.numel()).item())}
    for g, m in zip(uniq, (sums / cnt).cpu().numpy()):
        out[g] = np.float32(m)
    return out


def closest_samples(embeddings, anchor, top_k=1):
    """find_closest_sample: indices (numpy int64 [top_k], most similar first) of the rows whose normalised embedding has the
    largest dot product with the normalised anchor.  The fused normalise-and-similarity kernel, then torch.topk."""
    x = embeddings.embeddings if isinstance(embeddings, trainer.EmbeddingTable) else embeddings
    a = torch.as_tensor(np.asarray(anchor) if not torch.is_tensor(anchor) else anchor, dtype=torch.float32).to(x.device).reshape(-1, 1)
    tn = ops.text_colnorm(a.contiguous())                                                               # [1, D], unit norm
    scores = ops.l2norm_sim_ce_fwd(x.float().contiguous(), tn, 1.0, want_loss=False)[0][:, 0]
    return torch.topk(scores, min(int(top_k), scores.numel())).indices.cpu().numpy()


def representation_table(stats, zs_group_acc):
    """One split's table of VisRepAll (demo/visualizer.py:204-222): rows Acc. / Div. / Centr. Norm., columns Avg., Worst, group0 ..
    group3, rounded to 3 places.  `stats`: group_stats' dict (with distances); `zs_group_acc`: the group-accuracy dict of validate /
    validate_zs_linear_probing (its last entry, mean_acc, is dropped like the reference does)."""
    import pandas as pd
    values = [list(zs_group_acc.values())[:-1],
              [list(stats["pairwise_distance"].values())[0]] + [0] + list(stats["pairwise_distance"].values())[1:],
              [list(stats["mean_vector_norm"].values())[0]] + [0] + list(stats["mean_vector_norm"].values())[1:]]
    df = pd.DataFrame(values, index=TABLE_INDEX, columns=TABLE_COLUMNS)
    return df.round(3)


@torch.no_grad()
def _transformed_rows(x, transform, batch_size):
    was_training = getattr(transform, "training", False)
    if hasattr(transform, "eval"):
        transform.eval()
    out = torch.empty_like(x)
    for i in range(0, x.shape[0], batch_size):
        out[i:i + batch_size] = transform(x[i:i + batch_size])
    if was_training:
        transform.train()
    return out


def _transformed(table, transform, batch_size):
    return _transformed_rows(table.embeddings, transform, batch_size)


def representation_report(opt, train_table, val_table, test_table, classifier=None, transform=None):
    """The three tables of VisRepAll (train, val, test) and the group_stats dicts they were built from:
    ([frame_train, frame_val, frame_test], {'train': stats, 'val': stats, 'test': stats}).

    The `Acc.` row is the split's zero-shot group accuracies: validate() of `classifier` on the class prompts, or -- for
    linear_probing and without a classifier -- validate_zs_linear_probing, the raw embeddings against opt.text_embedding_dir.
    `transform` (a callable emb -> emb, e.g. classifier.adapter) is applied batch by batch in eval mode before the statistics: the
    report after the trained adapter (the reference's note 1.1)."""
    bs = max(int(getattr(opt, "batch_size", 0) or 0), 4096)
    ratio = train_table.group_ratio.numpy()
    zero_shot = classifier is None or getattr(opt, "tl_method", None) == "linear_probing"
    frames, all_stats = [], {}
    for split, table in (("train", train_table), ("val", val_table), ("test", test_table)):
        if zero_shot:
            acc = trainer.validate_zs_linear_probing(table, opt.text_embedding_dir, opt.zs_temperature, bs, ratio)[2]
        else:
            acc = trainer.validate(table, classifier, bs, ratio)[2]
        emb = table.embeddings if transform is None else _transformed(table, transform, bs)
        all_stats[split] = group_stats(emb, table.targets_group)
        frames.append(representation_table(all_stats[split], acc))
    return frames, all_stats


# ---- the map: PCA in place of plot_umap's UMAP / MDS (demo/visualizer.py:311-408) -----------------------------------------------
# PCA of the rows is classical (Torgerson) MDS of the Euclidean distances group_stats reports, it is deterministic, and a fit can
# place other rows (val and test in train's map; the embeddings after the adapter in the map of those before).

GATHER_ROWS = 4096        # rows of one group gathered at a time for its mean: a multiple of SUM_ROWS, 16 MB at D = 1024


def pca_from_scatter(scatter, center, mean, n, k):
    """The host step of `pca`, numpy only.  scatter float64 [D, D]: sum_i (x_i - center)(x_i - center)^T about `center` (any
    vector near the mean); mean float64 [D]: the rows' mean; n rows.  Since sum_i (x_i - center) = n (mean - center), the scatter
    about the mean is scatter - n (mean - center)(mean - center)^T.  Returns (components float32 [k, D] in descending variance, each
    signed so that its entry of largest magnitude is positive; explained_variance float64 [k] = eigenvalue / (n - 1);
    explained_variance_ratio float64 [k]; total_variance = trace / (n - 1))."""
    scatter = np.asarray(scatter, dtype=np.float64)
    D = scatter.shape[0]
    if scatter.shape != (D, D) or not 1 <= k <= min(D, 8):
        raise ValueError(f"pca: scatter {scatter.shape}, k = {k} (1..8)")
    if n < 2:
        raise ValueError(f"pca needs at least two rows, got {n}")
    d = np.asarray(mean, dtype=np.float64) - np.asarray(center).astype(np.float64)
    C = scatter - np.float64(n) * np.outer(d, d)
    w, V = np.linalg.eigh(C)                                        # ascending
    return _components_and_variances(w[::-1][:k], V[:, ::-1][:, :k].T, np.trace(C), n)


def _components_and_variances(w, V, trace, n):
    """The rules every eigen-solver's answer goes through, numpy only.  w float64 [k] descending eigenvalues of the scatter matrix
    about the mean, V float64 [k, D] their unit vectors as rows, trace of that matrix, n rows.  Returns pca_from_scatter's tuple:
    float32 components, each signed so that its entry of largest magnitude is positive; eigenvalue / (n - 1); ratio; total variance."""
    k = len(w)
    comp = np.ascontiguousarray(V, dtype=np.float32)
    top = np.abs(comp).argmax(axis=1)
    comp *= np.where(comp[np.arange(k), top] < 0, np.float32(-1), np.float32(1))[:, None]
    ratio = w / trace if trace > 0 else np.zeros(k)
    return comp, w / (n - 1.0), ratio, trace / (n - 1.0)


def _group_means(x, dense, counts, center):
    """float64 [G, D]: the groups' mean rows MINUS `center` (device fp32 [D]), GATHER_ROWS gathered rows at a time (never a sorted
    copy of x), fixed order.  The centre is subtracted from the gathered rows before they are summed, so the fp32 block sums lose
    2^-24 of the rows' spread, not of their distance from the origin."""
    means = np.zeros((len(counts), x.shape[1]), dtype=np.float64)
    for g in range(len(counts)):
        idx = torch.from_numpy(np.flatnonzero(dense == g)).to(x.device)
        for i in range(0, idx.numel(), GATHER_ROWS):
            means[g] += _column_sums(ops.gather_rows(x, idx[i:i + GATHER_ROWS].contiguous()).sub_(center))
        means[g] /= counts[g]
    return means


SOLVERS = ("host", "device")


def _device_eigen_step(scatter, center, mean, n, k, tol, max_iter):
    """`pca`'s eigen step without the D x D copy to the host.  scatter: ops.covariance's device tensor about float32 `center`.  The
    n (mean - center)(mean - center)^T correction and the trace are float64 torch ops on the device (torch.outer(d, d) is symmetric
    to the bit, so the corrected matrix is too), ops.sym_eig_topk solves, and only the [k, D] vectors and k values come back.
    Returns (pca_from_scatter's tuple or None when the solver did not converge, info)."""
    d = torch.from_numpy(np.asarray(mean, dtype=np.float64) - np.asarray(center).astype(np.float64)).to(scatter.device)
    C = scatter - float(n) * torch.outer(d, d)
    values, vectors, info = ops.sym_eig_topk(C, k, tol=tol, max_iter=max_iter)
    if not info["converged"]:
        return None, info
    trace = torch.trace(C).item()
    return _components_and_variances(values.cpu().numpy(), vectors.cpu().numpy(), np.float64(trace), n), info


def pca(embeddings, groups=None, k=2, solver="host", tol=1e-10, max_iter=256):
    """Principal components of a split and its rows' coordinates in them: the deterministic map of the reference's
    representation report (plot_umap draws UMAP or MDS; PCA is classical MDS of the distances of group_stats).

    `embeddings`: an EmbeddingTable (its targets_group unless `groups` is given) or a device tensor [N, D] with `groups` [N].
    Returns {'mean' float32 [D], 'components' float32 [k, D] (descending variance, largest-magnitude entry positive),
    'explained_variance' float64 [k] (eigenvalue / (N - 1)), 'explained_variance_ratio' [k], 'total_variance',
    'coords' device tensor [N, k] = (x - mean) components^T, 'centroids' {'full': zeros, g: (mean_g - mean) components^T}} with
    the groups in np.unique order.

    The scatter matrix comes from the fused kernel (ops.covariance) about float32(mean) -- nothing N x D is allocated --, the
    difference between that vector and the float64 mean is removed on the host, numpy.linalg.eigh solves the D x D float64
    problem there, and ops.project_rows reads the rows once more for the coordinates.  The group means behind the centroids are
    sums of gathered rows minus that centre, so they too lose precision relative to the rows' spread, wherever the split lies.
    k outside 1..8 and fewer than two rows raise ValueError before anything is launched.

    `solver`: "host" (the default) is the path above.  "device" keeps the scatter matrix on the device and finds the top k
    eigenpairs there (ops.sym_eig_topk: blocked subspace iteration on 16 vectors, stopped at a residual of `tol` theta_1 or after
    `max_iter` iterations); only k vectors and values come to the host, where the same rules apply (order, float32, sign,
    / (n - 1), ratio).  The fit then has one more key, 'eig': the solver's info (iterations, converged, state, residual) and
    'used', "device" or "host".  Known limit: the iteration converges by lambda_17 / lambda_k per step; when the k-th eigenvalue
    sits in a flat noise bulk (isotropic noise plus fewer than k directions) it does not get there in max_iter iterations.
    Then, and after a breakdown (a zero or rank-deficient matrix), `pca` silently solves the same scatter matrix on the host, so
    the answer is as good as the default's; the attempt is wasted time.  Any other solver name raises ValueError before anything
    is launched."""
    if solver not in SOLVERS:
        raise ValueError(f"pca: solver = {solver!r}; one of {SOLVERS}")
    x, uniq, dense, counts = _labelled_rows("pca", embeddings, groups, min_labels=1)
    x = _prepared(x)
    n = x.shape[0]
    if not 1 <= k <= min(x.shape[1], 8):
        raise ValueError(f"pca: k = {k} (1..8)")
    if n < 2:
        raise ValueError(f"pca needs at least two rows, got {n}")
    mean = _column_sums(x) / n
    center = mean.astype(np.float32)
    c_dev = torch.from_numpy(center).to(x.device)
    scatter = ops.covariance(x, c_dev)
    solved, eig = None, None
    if solver == "device":
        solved, eig = _device_eigen_step(scatter, center, mean, n, k, tol, max_iter)
        eig = dict(eig, used="device" if solved is not None else "host")
    if solved is None:
        solved = pca_from_scatter(scatter.cpu().numpy(), center, mean, n, k)
    comp, var, ratio, total = solved
    fit = {"mean": center, "components": comp, "explained_variance": var, "explained_variance_ratio": ratio, "total_variance": total}
    if eig is not None:
        fit["eig"] = eig
    fit["coords"] = ops.project_rows(x, c_dev, torch.from_numpy(comp).to(x.device))
    cent = _group_means(x, dense, counts, c_dev) @ comp.astype(np.float64).T
    fit["centroids"] = {"full": np.zeros(k, dtype=np.float64)}
    for i, g in enumerate(uniq):
        fit["centroids"][g] = cent[i]
    return fit


def pca_project(fit, embeddings):
    """coordinates (device tensor [N, k]) of another split, or of transformed embeddings, in the frame of an existing `pca` fit"""
    x = embeddings.embeddings if isinstance(embeddings, trainer.EmbeddingTable) else embeddings
    _need_device(x)
    return ops.project_rows(_prepared(x), torch.from_numpy(fit["mean"]).to(x.device), torch.from_numpy(fit["components"]).to(x.device))


def sample_rows(n, num_data, seed=42, offset=0):
    """The rows plot_umap draws (demo/visualizer.py:321-334), int64 indices: all n with num_data None; with offset == 0 the
    reference's np.random.seed(seed); np.random.choice(np.arange(n), size=min(num_data, n), replace=False) -- the same stream from a
    private RandomState, the global one is left alone --; with offset > 0 the slice offset .. offset + num_data."""
    if num_data is None:
        return np.arange(n)
    if offset == 0:
        return np.random.RandomState(seed).choice(np.arange(n), size=min(int(num_data), n), replace=False)
    return np.arange(n)[offset:offset + num_data]


def projection_report(opt, train_table, val_table, test_table, transform=None, k=2, num_data=None, seed=42, solver="host", tol=1e-10,
                      max_iter=256):
    """VisRepAll's map without matplotlib: a PCA fitted on train's rows (`sample_rows(len(train), num_data, seed)` of them; after
    `transform`, a callable emb -> emb such as classifier.adapter, applied batch by batch in eval mode) and all three splits in that
    one frame.  Returns ({'train': s, 'val': s, 'test': s}, fit) with s = {'coords' numpy [n, k], 'rows' (indices into the table),
    'groups', 'targets', 'spurious'} and fit = `pca`'s dict of the train rows.  `solver`, `tol`, `max_iter`: `pca`'s."""
    bs = max(int(getattr(opt, "batch_size", 0) or 0), 4096)
    out, fit = {}, None
    for split, table in (("train", train_table), ("val", val_table), ("test", test_table)):
        rows = sample_rows(len(table), num_data, seed)
        emb = table.embeddings if transform is None else _transformed(table, transform, bs)
        if num_data is not None:
            emb = ops.gather_rows(emb, torch.from_numpy(rows.astype(np.int64)).to(emb.device))
        groups = table.group_array[rows]
        if fit is None:
            fit = pca(emb, groups, k, solver=solver, tol=tol, max_iter=max_iter)
            coords = fit["coords"]
        else:
            coords = pca_project(fit, emb)
        out[split] = {"coords": coords.cpu().numpy(), "rows": rows, "groups": groups,
                      "targets": table.targets.cpu().numpy()[rows], "spurious": table.targets_spurious.cpu().numpy()[rows]}
    return out, fit


# ---- k-means pseudo-groups: the label-free route to group DRO (Sohoni et al. 2020, "GEORGE") ------------------------------------
# Cluster the embeddings of each class, train on the clusters as groups; and the report's open question in one number: does a
# representation, before or after the adapter, separate the spurious attribute at all (cluster_agreement)?

def kmeans_pp_rows(x, k, rng):
    """k-means++ (Arthur & Vassilvitskii 2007): the indices (numpy int64 [k]) of k rows of the device tensor x as start centres,
    drawn from `rng` (a numpy RandomState).  The first uniformly; each further one by D^2 sampling from dmin of ops.kmeans_assign
    against the rows chosen so far: one N-float copy to the host, a float64 cumulative sum and searchsorted.  A chosen row has
    dmin == 0 exactly and is never drawn again; when every row coincides with a chosen one the draw is uniform."""
    n = x.shape[0]
    rows = [int(rng.randint(n))]
    while len(rows) < k:
        centers = ops.gather_rows(x, torch.tensor(rows, dtype=torch.int64, device=x.device))
        cum = np.cumsum(ops.kmeans_assign(x, centers)[1].cpu().numpy().astype(np.float64))
        if not cum[-1] > 0:
            rows.append(int(rng.randint(n)))
            continue
        rows.append(min(int(np.searchsorted(cum, rng.random_sample() * cum[-1], side="right")), n - 1))
    return np.asarray(rows, dtype=np.int64)


def size_order(counts):
    """the renumbering rule of `kmeans`: the clusters' old indices by size, descending; the lower old index first on a tie"""
    return np.argsort(-np.asarray(counts, dtype=np.int64), kind="stable")


def kmeans(embeddings, k, init="k-means++", seed=0, n_init=1, max_iter=100, transform=None):
    """Lloyd's k-means of a split's rows into k <= 16 clusters on the device (ops.kmeans_fit: two reads of the rows per iteration,
    fixed-order float64 sums, the same bits on every call).

    `embeddings`: an EmbeddingTable or a device tensor [N, D].  `transform` (a callable emb -> emb, e.g. the stage-1 adapter) is
    applied batch by batch in eval mode first, as in representation_report.  `init`: "k-means++" -- `kmeans_pp_rows` drawn from a
    private np.random.RandomState(seed), the global stream is left alone -- or an fp32 [k, D] array of start centres.  With
    n_init > 1 (k-means++ only) the restarts continue the same stream and the fit of lowest inertia wins, the lowest restart index
    on a tie.  Returns {'labels' device int64 [N], 'centers' numpy fp32 [k, D], 'inertia' float, 'counts' numpy int64 [k],
    'iterations', 'converged'}; the clusters are renumbered by size, descending (size_order), so cluster 0 is the majority.  A fit
    that reaches max_iter reports converged False; nothing is raised."""
    x = embeddings.embeddings if isinstance(embeddings, trainer.EmbeddingTable) else embeddings
    _need_device(x)
    k, n_init = int(k), int(n_init)
    if not 1 <= k <= ops.KMEANS_MAX_K:
        raise ValueError(f"kmeans: k = {k} (1..{ops.KMEANS_MAX_K})")
    if x.shape[0] < k:
        raise ValueError(f"kmeans: {x.shape[0]} rows for {k} clusters")
    x = _prepared(x, transform)
    best = None
    if isinstance(init, str):
        if init != "k-means++" or n_init < 1:
            raise ValueError(f"kmeans: init = {init!r}, n_init = {n_init}; 'k-means++' with n_init >= 1, or an array of start centres")
        rng = np.random.RandomState(seed)
        for _ in range(n_init):
            start = ops.gather_rows(x, torch.from_numpy(kmeans_pp_rows(x, k, rng)).to(x.device))
            fit = ops.kmeans_fit(x, start, max_iter=max_iter)
            if best is None or fit[2]["inertia"] < best[2]["inertia"]:
                best = fit
    else:
        start = np.ascontiguousarray(init, dtype=np.float32)
        if start.shape != (k, x.shape[1]):
            raise ValueError(f"kmeans: init has shape {start.shape}, not {(k, x.shape[1])}")
        best = ops.kmeans_fit(x, torch.from_numpy(start).to(x.device), max_iter=max_iter)
    centers, labels, info = best
    order = size_order(info["counts"])
    rank = np.empty(k, dtype=np.int64)
    rank[order] = np.arange(k)
    return {"labels": torch.from_numpy(rank).to(x.device)[labels.long()], "centers": centers.cpu().numpy()[order],
            "inertia": info["inertia"], "counts": info["counts"][order], "iterations": info["iterations"], "converged": info["converged"]}


def pseudo_groups(table, k=2, **kw):
    """GEORGE's groups: `kmeans` (its keywords in `kw`) within every class of an EmbeddingTable.  The rows are sorted by class with
    one gather, as group_stats sorts them by group, and each class is a slice.  Returns (clusters numpy int64 [N]: the cluster id,
    0 .. k-1 and 0 the class's largest, of every row in the table's order; {class: that class's `kmeans` dict without its labels})."""
    y = table.targets.cpu().numpy()
    uniq, counts = np.unique(y, return_counts=True)
    order = np.argsort(y, kind="stable")
    xs = ops.gather_rows(table.embeddings.float().contiguous(), torch.from_numpy(order).to(table.embeddings.device))
    bounds = np.concatenate([[0], np.cumsum(counts)])
    clusters, fits = np.empty(len(y), dtype=np.int64), {}
    for i, cls in enumerate(uniq):
        fit = kmeans(xs[bounds[i]:bounds[i + 1]], k, **kw)
        clusters[order[bounds[i]:bounds[i + 1]]] = fit.pop("labels").cpu().numpy()
        fits[int(cls)] = fit
    return clusters, fits


def cluster_agreement(clusters, groups):
    """How well a partition recovers another, on the host: {'table': the contingency table int64 [clusters, groups] in np.unique
    order of both, 'purity': sum over clusters of their largest cell / N, 'ari': the adjusted Rand index (Hubert & Arabie 1985): 1
    for the same partition up to a renaming, about 0 for independent ones; 1 when both are one block}."""
    a, b = np.asarray(clusters).ravel(), np.asarray(groups).ravel()
    if a.shape != b.shape or a.size == 0:
        raise ValueError(f"cluster_agreement: {a.shape} cluster ids for {b.shape} group ids")
    ua, ia = np.unique(a, return_inverse=True)
    ub, ib = np.unique(b, return_inverse=True)
    table = np.zeros((len(ua), len(ub)), dtype=np.int64)
    np.add.at(table, (ia, ib), 1)
    pairs = lambda m: (m.astype(np.float64) * (m - 1.0) / 2.0).sum()
    cells, rows, cols, total = pairs(table), pairs(table.sum(1)), pairs(table.sum(0)), pairs(np.array([a.size]))
    expected = rows * cols / total if total > 0 else 0.0
    ceiling = 0.5 * (rows + cols)
    ari = 1.0 if ceiling == expected else (cells - expected) / (ceiling - expected)
    return {"table": table, "purity": float(table.max(1).sum() / a.size), "ari": float(ari)}


def pseudo_group_table(table, clusters):
    """An EmbeddingTable over the SAME embedding storage (no copy) whose confounder is the cluster id, so that targets_group =
    2 y + cluster: given as `train_table` to train_all_epochs / train_sweep with opt.robust it is group DRO without group labels.
    Val and test keep their true groups, so model selection and the reported worst-group accuracy do not change.  The tables have
    two places per class: cluster ids outside {0, 1} raise ValueError."""
    c = np.asarray(clusters)
    if c.shape != (len(table),) or not np.isin(c, (0, 1)).all():
        raise ValueError(f"pseudo_group_table: cluster ids must be {len(table)} values in {{0, 1}} (n_places = {table.n_places})")
    out = trainer.EmbeddingTable(table.embeddings, table.targets.cpu().numpy(), c.astype(np.int64), y_pred=None, filenames=table.filenames,
                                 device=table.device)
    out.y_pred = table.y_pred
    return out


# ---- silhouettes: how well a labelling is separated in a representation (Rousseeuw 1987) -----------------------------------------
# Exact, O(N^2 D), and without the N x N matrix: ops.pairdist_row_group_sums gives every row its summed distance to every label in
# one pass.  Per row, so it names the rows whose own group is not their nearest one; per labelling, so it needs no second partition
# (cluster_agreement does) and exists before and after `transform`; and it is the criterion kmeans_select_k chooses k by.

def silhouette_from_sums(R, dense_labels, counts):
    """The host step of `silhouette`, numpy only.  R float64 [N, G]: R[i, g] = sum over j != i with label g of ||x_i - x_j||;
    dense_labels int [N] in [0, G); counts [G]: the rows per label (they must be dense_labels' own counts).  The conventions:
    a_i = R[i, g_i] / (n_{g_i} - 1); b_i = min over g != g_i with n_g > 0 of R[i, g] / n_g; s_i = (b_i - a_i) / max(a_i, b_i);
    s_i = 0 (and a_i = 0) for a row alone in its label (Rousseeuw's and sklearn's convention) and where max(a_i, b_i) == 0 (all
    rows identical); empty labels are ignored; fewer than two labels with rows raise ValueError.  Returns {'a', 'b', 'samples':
    float64 [N], 'nearest': int64 [N], the label index that attains b_i, the lowest index on a tie}."""
    R = np.asarray(R, dtype=np.float64)
    g = np.asarray(dense_labels).astype(np.int64).ravel()
    n = np.asarray(counts).astype(np.int64).ravel()
    if R.ndim != 2 or g.shape != (R.shape[0],) or n.shape != (R.shape[1],):
        raise ValueError(f"silhouette_from_sums: R {R.shape}, {g.shape[0]} labels, {n.shape[0]} counts")
    N, G = R.shape
    if N and (g.min() < 0 or g.max() >= G) or not np.array_equal(np.bincount(g, minlength=G), n):
        raise ValueError("silhouette_from_sums: counts are not the counts of dense_labels")
    present = n > 0
    if present.sum() < 2:
        raise ValueError(f"a silhouette needs at least two labels with rows, got {int(present.sum())}")
    rows = np.arange(N)
    own = n[g]
    a = np.where(own > 1, R[rows, g] / np.maximum(own - 1, 1), 0.0)
    M = R / np.where(present, n, 1).astype(np.float64)[None, :]
    M[:, ~present] = np.inf
    M[rows, g] = np.inf
    nearest = M.argmin(axis=1)                                      # the first minimum: the lowest index on a tie
    b = M[rows, nearest]
    top = np.maximum(a, b)
    s = np.where((own > 1) & (top > 0), (b - a) / np.where(top > 0, top, 1.0), 0.0)
    return {"a": a, "b": b, "samples": s, "nearest": nearest.astype(np.int64)}


def silhouette(embeddings, labels=None, transform=None):
    """The exact silhouette of a labelling of a split's rows, Euclidean distances, on the device (ops.pairdist_row_group_sums: one
    pass over the 256 x 256 tiles of the Gram matrix, nothing N x N is stored).

    `embeddings`: an EmbeddingTable (its targets_group unless `labels` is given) or a device tensor [N, D] with `labels` [N] (any
    integers; they go through np.unique, at most 16 of them: more raise DbmmUnsupported, fewer than two ValueError, both before
    anything is launched).  `transform` (a callable emb -> emb, e.g. the stage-1 adapter) is applied batch by batch in eval mode
    first, as in `kmeans`.  The rows are sorted by label with one gather, as group_stats sorts them by group (nearly every tile of
    the kernel then holds one label), the centre is that copy's mean, and everything is returned in the INPUT's row order:
    {'samples': float64 [N], 'score': their mean, 'per_label': {label: mean of its rows}, 'a', 'b': float64 [N] (the mean distance
    to the row's own label and to the nearest other one), 'nearest': [N], the nearest other label of every row (a value of
    `labels`), 'labels': the unique labels, 'counts'}.  The conventions are silhouette_from_sums'."""
    x, uniq, dense, counts = _labelled_rows("silhouette", embeddings, labels, ops.PAIRDIST_ROWS_MAX_G)
    G = len(uniq)
    R, _ = _sorted_pass(_prepared(x, transform), dense, lambda xs, ids, center: ops.pairdist_row_group_sums(xs, ids, G, center), per_row=True)
    out = silhouette_from_sums(R, dense, counts)
    s = out["samples"]
    return {"samples": s, "score": float(s.mean()), "per_label": {lab: float(s[dense == i].mean()) for i, lab in enumerate(uniq)},
            "a": out["a"], "b": out["b"], "nearest": uniq[out["nearest"]], "labels": uniq, "counts": counts}


def _device_rows(embeddings, transform):
    x = embeddings.embeddings if isinstance(embeddings, trainer.EmbeddingTable) else embeddings
    _need_device(x)
    return _prepared(x, transform)


def kmeans_select_k(embeddings, ks=(2, 3, 4, 5, 6, 7, 8), transform=None, **kmeans_kw):
    """The number of clusters by the silhouette: one `kmeans` fit (its keywords in `kmeans_kw`) and one `silhouette` of that fit's
    labels per k in `ks` (each in 2..16), on the same rows -- `transform` is applied once, before the first fit.  Returns {'k': the
    k of the largest score, the smaller k on a tie, 'scores': {k: score}, 'fits': {k: `kmeans`' dict}}; a fit that left fewer than
    two clusters with rows scores nan and is never chosen.  It REPORTS k: pseudo_group_table still takes two clusters per class,
    the tables are not widened."""
    ks = sorted({int(k) for k in ks})
    if not ks or ks[0] < 2 or ks[-1] > ops.KMEANS_MAX_K:
        raise ValueError(f"kmeans_select_k: ks = {ks}; values in 2..{ops.KMEANS_MAX_K}")
    x = _device_rows(embeddings, transform)
    scores, fits, best = {}, {}, None
    for k in ks:
        fit = kmeans(x, k, **kmeans_kw)
        fits[k] = fit
        scores[k] = silhouette(x, fit["labels"])["score"] if (fit["counts"] > 0).sum() >= 2 else float("nan")
        if scores[k] == scores[k] and (best is None or scores[k] > scores[best]):
            best = k
    if best is None:
        raise ValueError("kmeans_select_k: no fit has two clusters with rows")
    return {"k": best, "scores": scores, "fits": fits}


def _score_or_nan(x, labels):
    if len(np.unique(labels)) < 2:
        return {"score": float("nan"), "per_label": {}}
    fit = silhouette(x, labels)
    return {"score": fit["score"], "per_label": fit["per_label"]}


def separation_report(train_table, val_table, test_table, transform=None):
    """How separable the groups, and within each class the spurious attribute, are in a representation: {'train': r, 'val': r,
    'test': r} with r = {'group': {'score', 'per_label'} of `silhouette` on targets_group, 'spurious_within_class': {class: the
    silhouette score of the confounder among that class's rows}}.  A class in which only one place is present gets nan; nothing is
    raised.  `transform` (a callable emb -> emb) is applied once per split, as in `kmeans`: run it once raw and once with the
    stage-1 or stage-2 adapter, the within-class scores should fall when the debiasing works."""
    out = {}
    for split, table in (("train", train_table), ("val", val_table), ("test", test_table)):
        x = _device_rows(table, transform)
        y, c = table.targets.cpu().numpy(), table.targets_spurious.cpu().numpy()
        within = {}
        for cls in np.unique(y):
            idx = np.flatnonzero(y == cls)
            if len(np.unique(c[idx])) < 2:
                within[int(cls)] = float("nan")
                continue
            within[int(cls)] = silhouette(ops.gather_rows(x, torch.from_numpy(idx).to(x.device)), c[idx])["score"]
        out[split] = {"group": _score_or_nan(x, table.targets_group.cpu().numpy()), "spurious_within_class": within}
    return out


# ---- kernel two-sample (MMD^2) and dependence (HSIC) scores: is a labelling still in the rows, beyond what a linear map sees? --------------
# Gretton et al. 2012 (MMD) and 2005 (HSIC) with the RBF kernel exp(-gamma ||x - y||^2) at a ladder of bandwidths.  Both are sums of kernel
# values over all pairs, bucketed by (label, label): ops.pairdist_rbf_group_sums gives the L x G x G bucket sums in one pass, nothing
# N x N is stored, and everything after it is numpy on L G^2 numbers.  Zero in the limit exactly when the groups' distributions coincide
# (MMD) or the labelling is independent of the rows (HSIC); the null comes from relabelling (mmd_permutation_test).

RBF_SCALES = (0.25, 1.0, 4.0)


def _variance_sum(x, chunk=1 << 12):
    """sum over the columns of the population variance of the rows x (any torch tensor [N, D]), from float64 sums in two passes over
    row chunks -- dfr.column_moments' arithmetic without its replacement of a constant column's 0 by 1, which would count here"""
    n = x.shape[0]
    s = torch.zeros(x.shape[1], dtype=torch.float64, device=x.device)
    for i in range(0, n, chunk):
        s += x[i:i + chunk].double().sum(0)
    mean, q = s / n, 0.0
    for i in range(0, n, chunk):
        q += ((x[i:i + chunk].double() - mean) ** 2).sum().item()
    return q / n


def rbf_gammas(embeddings, scales=RBF_SCALES, transform=None):
    """The bandwidth ladder gamma_k = scales[k] / m, float64 [len(scales)], with m the mean squared distance between two different
    rows, 2 N / (N - 1) * sum_d var_d: the "mean heuristic".  Deterministic, two reads of the rows and no N^2 work.  In D = 1024 the
    squared distances of a split concentrate, so m sits close to the median the usual heuristic takes; how close on real CLIP rows
    has not been measured here.  `embeddings`: an EmbeddingTable or a tensor [N, D] (a host tensor works too); `transform` as in
    `silhouette`.  Fewer than two rows, rows that are all equal or a scale <= 0 raise ValueError."""
    x = embeddings.embeddings if isinstance(embeddings, trainer.EmbeddingTable) else embeddings
    if not torch.is_tensor(x) or x.dim() != 2:
        raise ValueError("rbf_gammas: the rows must be an EmbeddingTable or a tensor [N, D]")
    x = x.float()
    if transform is not None:
        x = _transformed_rows(x.contiguous(), transform, TRANSFORM_ROWS)
    n = x.shape[0]
    scales = np.asarray(scales, dtype=np.float64).ravel()
    if n < 2 or scales.size == 0 or not (np.isfinite(scales).all() and (scales > 0).all()):
        raise ValueError(f"rbf_gammas: {n} rows, scales = {scales.tolist()}; at least two rows and finite scales > 0")
    m = 2.0 * n / (n - 1.0) * _variance_sum(x)
    if not (m > 0 and np.isfinite(m)):
        raise ValueError(f"rbf_gammas: the mean squared distance of the rows is {m}")
    return scales / m


def _kernel_sums(K, counts):
    K = np.asarray(K, dtype=np.float64)
    n = np.asarray(counts).astype(np.float64).ravel()
    if K.ndim != 3 or K.shape[1] != K.shape[2] or n.shape != (K.shape[1],):
        raise ValueError(f"K {K.shape} is not [L, G, G] for {n.shape[0]} counts")
    return K, n


def mmd_from_sums(K, counts, unbiased=True):
    """The host step of `mmd`, numpy only.  K float64 [L, G, G] as ops.pairdist_rbf_group_sums returns it (sums over unordered pairs,
    the diagonal i = j left out), counts [G]: the rows per label.  Returns {'kernel_mean': [L, G, G], 'mmd2': [L, G, G], 'mmd2_sum':
    [G, G]}: kernel_mean[l, a, b] is the mean kernel value between a row of a and a row of b -- K / (n_a n_b) off the diagonal, on it
    2 K / (n_a (n_a - 1)) (the U-statistic: pairs of different rows) or, with unbiased=False, (2 K + n_a) / n_a^2 (the V-statistic:
    k(x, x) = 1 counted); mmd2[l, a, b] = kernel_mean[l, a, a] + kernel_mean[l, b, b] - 2 kernel_mean[l, a, b] with a zero
    diagonal; mmd2_sum is the equal-weight multi-kernel statistic, the sum over l.  nan wherever a label has fewer than two rows
    (unbiased) or none; nothing is raised.  The unbiased estimate can be slightly negative."""
    K, n = _kernel_sums(K, counts)
    G = n.shape[0]
    with np.errstate(divide="ignore", invalid="ignore"):
        mean = K / np.outer(n, n)[None]
        d = np.arange(G)
        kd = K[:, d, d]
        mean[:, d, d] = 2.0 * kd / (n * (n - 1.0)) if unbiased else (2.0 * kd + n) / (n * n)
        mean[:, d, d] = np.where(n >= (2 if unbiased else 1), mean[:, d, d], np.nan)
        mean[:, n == 0, :] = np.nan
        mean[:, :, n == 0] = np.nan
        within = mean[:, d, d]
        mmd2 = within[:, :, None] + within[:, None, :] - 2.0 * mean
    bad = np.isnan(mmd2[:, d, d])
    mmd2[:, d, d] = np.where(bad, np.nan, 0.0)
    return {"kernel_mean": mean, "mmd2": mmd2, "mmd2_sum": mmd2.sum(0)}


def hsic_from_sums(K, counts):
    """The biased HSIC tr(K H L H) / N^2 of the rows against their labels, delta kernel on the labels, per bandwidth: float64 [L],
    numpy only.  K, counts as in mmd_from_sums.  With p = counts / N and Kfull[a][b] the sum over ORDERED pairs with the diagonal
    (K off the diagonal, 2 K + n_a on it) it is sum_ab Kfull[a][b] (delta_ab - p_a - p_b + sum p^2) / N^2."""
    K, n = _kernel_sums(K, counts)
    N = n.sum()
    G = n.shape[0]
    p = n / N
    full = K.copy()
    d = np.arange(G)
    full[:, d, d] = 2.0 * K[:, d, d] + n
    w = np.eye(G) - p[:, None] - p[None, :] + (p * p).sum()
    return (full * w[None]).sum((1, 2)) / (N * N)


def mmd(embeddings, groups=None, gammas=None, scales=RBF_SCALES, transform=None, unbiased=True):
    """RBF-kernel MMD^2 between every two groups of a split's rows, and the HSIC of the rows against the grouping, at up to four
    bandwidths from ONE pass of the fused Gram kernel (ops.pairdist_rbf_group_sums; nothing N x N is stored).

    `embeddings`: an EmbeddingTable (its targets_group unless `groups` is given) or a device tensor [N, D] with `groups` [N] (any
    integers; they go through np.unique, at most 8 of them: more raise DbmmUnsupported, fewer than two ValueError, both before
    anything is launched).  `transform` as in `silhouette`.  `gammas`: 1..4 bandwidths; by default rbf_gammas(scales) of the same
    (transformed) rows.  The rows are sorted by label with one gather, as group_stats sorts them; the centre is that copy's mean.
    Returns mmd_from_sums' dict (indexed by the labels in np.unique order) plus 'hsic': [L] (hsic_from_sums), 'gammas', 'labels',
    'counts'.  The kernel's precondition for its 1e-4 bound is gamma (|a|^2 + |b|^2) <= 64 for centred rows a, b: the default
    ladder's largest gamma, 4 / m, keeps it as long as no row lies more than 4 root-mean-square radii from the centre (m is twice the mean squared radius)."""
    x, uniq, dense, counts = _labelled_rows("mmd", embeddings, groups, 8)
    G = len(uniq)
    x = _prepared(x, transform)
    gammas = _resolved_gammas(x, gammas, scales)
    K, _ = _sorted_pass(x, dense, lambda xs, ids, center: ops.pairdist_rbf_group_sums(xs, ids, G, center, gammas.tolist()))
    out = mmd_from_sums(K, counts, unbiased=unbiased)
    out.update(hsic=hsic_from_sums(K, counts), gammas=gammas, labels=uniq, counts=counts)
    return out


def _pooled_pair(what, embeddings, groups, pair, transform):
    """The rows of the two labels in `pair`, pooled: (their indices in the input, the rows -- one gather, `transform` applied once --,
    their labels 0 / 1 for pair[0] / pair[1] in row order).  One label named twice, or fewer than two rows of either: ValueError."""
    x, uniq, dense, _ = _labelled_rows(what, embeddings, groups, min_labels=1)
    g_np = uniq[dense]
    a, b = pair
    if a == b:
        raise ValueError(f"{what}: pair = {pair!r} names one label twice")
    idx = np.flatnonzero((g_np == a) | (g_np == b))
    labels = (g_np[idx] == b).astype(np.int64)
    if labels.sum() < 2 or (1 - labels).sum() < 2:
        raise ValueError(f"{what}: labels {a!r} and {b!r} need at least two rows each")
    xp = ops.gather_rows(_prepared(x), torch.from_numpy(idx).to(x.device))
    return idx, xp if transform is None else _transformed_rows(xp, transform, TRANSFORM_ROWS), labels


def mmd_permutation_test(embeddings, groups, pair, n_perm=20, seed=0, **mmd_kw):
    """The kernel two-sample test between the two labels in `pair`: their rows are pooled (one gather, `transform` applied once),
    the bandwidths are fixed from the pooled rows once (`gammas`, else rbf_gammas of `scales`), and the observed mmd2_sum is compared
    with `n_perm` relabellings.  Relabelling k is labels[rng.permutation(n)] with rng = np.random.default_rng(seed), one draw per
    permutation in order, labels the pooled rows' 0 / 1 (pair[0] / pair[1]) in row order; each is one `mmd` call (rows re-sorted by
    the new labels, so the kernel's fast path holds).  Returns {'stat', 'null': float64 [n_perm], 'p': (1 + #{null >= stat}) /
    (1 + n_perm)}.  The cost is n_perm + 1 passes of the kernel over the pooled rows."""
    _, xp, labels = _pooled_pair("mmd_permutation_test", embeddings, groups, pair, mmd_kw.pop("transform", None))
    gammas = _resolved_gammas(xp, mmd_kw.pop("gammas", None), mmd_kw.pop("scales", RBF_SCALES))
    stat = float(mmd(xp, labels, gammas=gammas, **mmd_kw)["mmd2_sum"][0, 1])
    rng = np.random.default_rng(seed)
    null = np.array([mmd(xp, labels[rng.permutation(len(labels))], gammas=gammas, **mmd_kw)["mmd2_sum"][0, 1] for _ in range(n_perm)],
                    dtype=np.float64).reshape(n_perm)
    return {"stat": stat, "null": null, "p": (1.0 + float((null >= stat).sum())) / (1.0 + n_perm)}


def dependence_report(train_table, val_table, test_table, transform=None, scales=RBF_SCALES):
    """How much of the groups, and within each class of the spurious attribute, is left in a representation, by kernel scores:
    {'train': r, 'val': r, 'test': r} with r = {'group': `mmd`'s mmd2_sum [G, G] over targets_group, 'spurious_within_class': {class:
    the mmd2_sum between the two places among that class's rows, nan if only one is present}, 'hsic_spurious': the [L] HSIC of the
    rows against targets_spurious (nan if only one place is present)}; every call takes its bandwidths from its own rows
    (rbf_gammas of `scales`).  `transform` is applied once per split, as in separation_report: run it raw, with an adapter, and on
    erased_table's rows -- the within-class numbers are the ones that should fall."""
    out = {}
    for split, table in (("train", train_table), ("val", val_table), ("test", test_table)):
        x = _device_rows(table, transform)
        y, c = table.targets.cpu().numpy(), table.targets_spurious.cpu().numpy()
        within = {}
        for cls in np.unique(y):
            idx = np.flatnonzero(y == cls)
            if len(np.unique(c[idx])) < 2:
                within[int(cls)] = float("nan")
                continue
            within[int(cls)] = float(mmd(ops.gather_rows(x, torch.from_numpy(idx).to(x.device)), c[idx], scales=scales)["mmd2_sum"][0, 1])
        hsic = mmd(x, c, scales=scales)["hsic"] if len(np.unique(c)) >= 2 else np.full(len(scales), np.nan)
        out[split] = {"group": mmd(x, table.targets_group.cpu().numpy(), scales=scales)["mmd2_sum"], "spurious_within_class": within,
                      "hsic_spurious": hsic}
    return out


# ---- per-row kernel sums: a kernel probe, the MMD witness function and a normalised HSIC (CKA) --------------------------------------------
# All three are made of R[l, i, g] = sum over j != i with label g of exp(-gamma_l ||x_i - x_j||^2), which ops.pairdist_rbf_row_group_sums gives
# in one pass with nothing N x N stored.  The probe is the leave-one-out Parzen-window classifier (no training, no learning rate): whether
# a labelling is still readable NON-linearly, as an accuracy, where after an erasure every linear probe is at chance by construction.  The
# witness function (Gretton et al. 2012, section 2.3) names the rows that make two groups differ.  The alignment (Cortes et al. 2012;
# the CKA of Kornblith et al. 2019 with the labels' delta kernel) is HSIC on a scale that can be compared across representations.

KERNEL_REL = 1e-4   # the kernels' relative bound on a kernel value under their preconditions (csrc/pairdist.hip)


def _sums_operands(what, R, labels, counts):
    R = np.asarray(R, dtype=np.float64)
    g = np.asarray(labels).astype(np.int64).ravel()
    n = np.asarray(counts).astype(np.int64).ravel()
    if R.ndim != 3 or g.shape != (R.shape[1],) or n.shape != (R.shape[2],):
        raise ValueError(f"{what}: R {R.shape} is not [L, N, G] for {g.shape[0]} labels and {n.shape[0]} counts")
    if g.size and (g.min() < -1 or g.max() >= R.shape[2]):
        raise ValueError(f"{what}: labels must lie in [0, {R.shape[2]}) or be -1 (a query row)")
    return R, g, n


def _densities(R, g, n):
    """(density [L, N, G], denominators [N, G]): R / (counts[g] - [labels[i] == g]), nan where that is 0"""
    den = np.broadcast_to(n[None, :], (g.shape[0], n.shape[0])).copy()
    own = np.flatnonzero(g >= 0)
    den[own, g[own]] -= 1
    with np.errstate(divide="ignore", invalid="ignore"):
        density = np.where(den[None] > 0, R / np.where(den > 0, den, 1)[None].astype(np.float64), np.nan)
    return density, den


def parzen_from_sums(R, labels, counts, prior="uniform"):
    """The host step of `kernel_probe`, numpy only.  R float64 [L, N, G] as ops.pairdist_rbf_row_group_sums returns it (the row itself
    left out); labels int [N]: dense labels in [0, G), or -1 for a query row (in no label's sum); counts [G]: the REFERENCE rows per
    label.  density[l, i, g] = R[l, i, g] / (counts[g] - [labels[i] == g]): the leave-one-out Parzen-window estimate of label g's
    density at row i, up to the kernel's normalising constant, which is common to all labels; nan where that denominator is 0 (an
    empty label; a label's only row, for its own label).  score is density for prior="uniform" (every label equally likely: the
    balanced classifier) and R itself for prior="empirical" (the label frequencies as prior: the Nadaraya-Watson vote).  pred[l, i]
    is the argmax of score over the labels with a denominator > 0, the lowest label on a tie, -1 for a row whose scores are all 0
    (or that has no scorable label); margin[l, i] = (top1 - top2) / top1 of those scores, nan if top1 == 0 or fewer than two
    labels are scorable.  Returns {'density', 'score': [L, N, G], 'pred': int64 [L, N], 'margin': [L, N]}.  Another `prior`,
    shapes that do not match and labels outside [-1, G) raise ValueError."""
    if prior not in ("uniform", "empirical"):
        raise ValueError(f"parzen_from_sums: prior = {prior!r}; 'uniform' or 'empirical'")
    R, g, n = _sums_operands("parzen_from_sums", R, labels, counts)
    density, den = _densities(R, g, n)
    ok = den > 0
    score = density if prior == "uniform" else np.where(ok[None], R, np.nan)
    s = np.where(ok[None], score, -np.inf)                             # scores are >= 0: -inf never wins against a scorable label
    L, N, G = R.shape
    pred = s.argmax(axis=2) if G else np.zeros((L, N), dtype=np.int64)  # the first maximum: the lowest label on a tie
    top = np.sort(s, axis=2)[:, :, ::-1]
    top1 = top[:, :, 0] if G else np.full((L, N), -np.inf)
    pred = np.where(top1 > 0, pred, -1).astype(np.int64)
    if G >= 2:
        top2 = top[:, :, 1]
        with np.errstate(divide="ignore", invalid="ignore"):
            margin = np.where((top1 > 0) & (ok.sum(1) >= 2)[None], (top1 - np.where(np.isfinite(top2), top2, 0.0)) / np.where(top1 > 0, top1, 1.0), np.nan)
    else:
        margin = np.full((L, N), np.nan)
    return {"density": density, "score": score, "pred": pred, "margin": margin}


def witness_from_sums(R, labels, counts, a, b):
    """The empirical MMD witness function between the labels a and b at every row, float64 [L, N], numpy only: density[:, :, a] -
    density[:, :, b] with parzen_from_sums' leave-one-out densities (R, labels, counts as there; a, b dense label indices).  Positive
    where a's rows are denser than b's.  The identity that ties it to `mmd`: its mean over the rows of a minus its mean over the
    rows of b is the unbiased mmd2[l, a, b] of mmd_from_sums.  nan where a label has no row (or only the row itself)."""
    R, g, n = _sums_operands("witness_from_sums", R, labels, counts)
    G = n.shape[0]
    if not (0 <= a < G and 0 <= b < G) or a == b:
        raise ValueError(f"witness_from_sums: a = {a!r}, b = {b!r}; two different labels in [0, {G})")
    density, _ = _densities(R, g, n)
    return density[:, :, a] - density[:, :, b]


def alignment_from_sums(K, K2_total, row_sq, counts):
    """The host step of `kernel_alignment`, numpy only: the normalised HSIC (centred kernel alignment) of the RBF kernel against the
    delta kernel of the labels, per bandwidth.  Ordered pairs, the diagonal k(x, x) = 1 included, p = counts / N:
      hsic    = tr(K H L H) / N^2 = hsic_from_sums(K, counts);
      hsic_kk = tr(K H K H) / N^2 = (A - 2 B / N + C^2 / N^2) / N^2, A = sum_ij k_ij^2 = N + 2 K2_total (k^2 is the kernel at 2 gamma),
                B = sum_i (row sum of k)^2 = row_sq, C = sum_ij k_ij (K's own total);
      hsic_ll = tr(L H L H) / N^2 = sum p^2 - 2 sum p^3 + (sum p^2)^2;
      alignment = hsic / sqrt(hsic_kk hsic_ll), in [0, 1] up to rounding.
    K float64 [L, G, G] as ops.pairdist_rbf_group_sums returns it at gamma (unordered pairs, the diagonal left out); K2_total [L]:
    the sum over all unordered pairs at 2 gamma; row_sq [L]: sum_i (1 + sum_g R[l, i, g])^2; counts [G].
    rel_bound [L] is the first-order propagation of the kernels' 1e-4 on every kernel value into the alignment:
    b_kl / |hsic| + b_kk / (2 hsic_kk), b_kl = 1e-4 sum_ab Kfull_ab |w_ab| / N^2 (w as in hsic_from_sums), b_kk = 1e-4 (A + 4 B / N +
    2 C^2 / N^2) / N^2.  It is part of the result on purpose: the centred quantities are differences of sums that nearly cancel when
    the kernel is nearly constant (wide bandwidths in high D), and a bound above 1 says the alignment has no digits left.
    Returns {'alignment', 'hsic', 'hsic_kk', 'hsic_ll' (a number), 'rel_bound'}: float64 [L]."""
    K, n = _kernel_sums(K, counts)
    L, G = K.shape[0], n.shape[0]
    K2 = np.asarray(K2_total, dtype=np.float64).ravel()
    B = np.asarray(row_sq, dtype=np.float64).ravel()
    if K2.shape != (L,) or B.shape != (L,):
        raise ValueError(f"alignment_from_sums: K {K.shape}, K2_total {K2.shape}, row_sq {B.shape}")
    N = n.sum()
    if not N > 0:
        raise ValueError("alignment_from_sums: no rows")
    p = n / N
    d = np.arange(G)
    full = K.copy()
    full[:, d, d] = 2.0 * K[:, d, d] + n
    w = np.eye(G) - p[:, None] - p[None, :] + (p * p).sum()
    hsic = hsic_from_sums(K, counts)
    A, C = N + 2.0 * K2, full.sum((1, 2))
    hsic_kk = (A - 2.0 * B / N + C * C / (N * N)) / (N * N)
    hsic_ll = (p ** 2).sum() - 2.0 * (p ** 3).sum() + (p ** 2).sum() ** 2
    b_kl = KERNEL_REL * (full * np.abs(w)[None]).sum((1, 2)) / (N * N)
    b_kk = KERNEL_REL * (A + 4.0 * B / N + 2.0 * C * C / (N * N)) / (N * N)
    with np.errstate(divide="ignore", invalid="ignore"):
        alignment = hsic / np.sqrt(hsic_kk * hsic_ll)
        rel_bound = b_kl / np.abs(hsic) + 0.5 * b_kk / hsic_kk
    return {"alignment": alignment, "hsic": hsic, "hsic_kk": hsic_kk, "hsic_ll": float(hsic_ll), "rel_bound": rel_bound}


def _sorted_row_sums(x, dense, G, gammas, extra=None):
    """_sorted_pass of ops.pairdist_rbf_row_group_sums: R float64 [L, N (+ M), G] on the host in the INPUT's row order, x's rows first"""
    return _sorted_pass(x, dense, lambda xs, ids, center: ops.pairdist_rbf_row_group_sums(xs, ids, G, center, np.asarray(gammas, dtype=np.float64).tolist()),
                        per_row=True, extra=extra)[0]


def _probe_scores(pred, true, G):
    """accuracy [L], recall [L, G] (nan for a label without rows), balanced accuracy [L] (the mean of the non-nan recalls) of the
    dense predictions pred [L, n] against the dense labels true [n]"""
    hit = pred == true[None, :]
    recall = np.full((pred.shape[0], G), np.nan)
    for g in range(G):
        rows = true == g
        if rows.any():
            recall[:, g] = hit[:, rows].mean(1)
    return {"accuracy": hit.mean(1), "recall": recall, "balanced_accuracy": np.nanmean(recall, axis=1)}


def kernel_probe(embeddings, labels=None, gammas=None, scales=RBF_SCALES, transform=None, prior="uniform", query=None, query_labels=None):
    """The kernel probe: a Parzen-window (kernel density) classifier of a labelling on a split's rows, RBF kernel, at up to four
    bandwidths from ONE pass of the fused Gram kernel (ops.pairdist_rbf_row_group_sums; nothing N x N is stored).  No training and
    no learning rate: it answers "is the attribute still readable non-linearly, and from which rows" as an accuracy.

    `embeddings`: an EmbeddingTable (its targets_group unless `labels` is given) or a device tensor [N, D] with `labels` [N] (any
    integers; they go through np.unique, at most 16 of them: more raise DbmmUnsupported, fewer than two ValueError, both before
    anything is launched).  `transform` and the default bandwidths as in `mmd` (rbf_gammas(scales) of the transformed rows).  The
    rows are sorted by label with one gather, the centre is the mean of what is passed to the kernel, and everything is returned
    in the input's row order.

    Without `query` every row is scored leave-one-out against the other rows of the split.  With `query`, a device tensor [M, D]
    that gets the same `transform`, the query rows are appended with label -1 and scored against the reference rows only (a row
    with label -1 is in nobody's sums); the bandwidths come from the reference rows, and the per-row outputs are those of the M
    query rows.  `prior`: parzen_from_sums'.

    Returns {'density': float64 [L, n, G], 'pred': [L, n] (values of `labels`; -1 for a row whose scores are all 0), 'margin':
    [L, n], 'gammas', 'labels': the unique labels, 'counts'} and, where the true labels are known (leave-one-out, or `query_labels`
    [M], values of `labels`), 'accuracy' [L], 'recall' [L, G] (nan for a label without scored rows) and 'balanced_accuracy' [L],
    the mean of the non-nan recalls.

    Read `margin` beside `pred`.  A kernel value is good to 1e-4 relative, and in high D at wide bandwidths the kernel is nearly
    constant, so the densities of different labels differ by less than that for many rows: in the float64 CPU study of this
    function 57 % of isotropic rows in D = 1024 at scale 0.25 had a margin below 1e-3, and 3 - 27 % of the rows of the synthetic
    embedding tables at the default ladder.  A prediction with such a margin is decided by rounding."""
    if prior not in ("uniform", "empirical"):
        raise ValueError(f"kernel_probe: prior = {prior!r}; 'uniform' or 'empirical'")
    if query is not None and labels is None and not isinstance(embeddings, trainer.EmbeddingTable):
        raise ValueError("kernel_probe: `query` rows are scored against labelled reference rows; give `labels`")
    x, uniq, dense, counts = _labelled_rows("kernel_probe", embeddings, labels, ops.PAIRDIST_ROWS_MAX_G, device="last")
    G, N = len(uniq), x.shape[0]
    true = dense
    if query is not None:
        if not torch.is_tensor(query) or not query.is_cuda or query.dim() != 2 or query.shape[1] != x.shape[1] or query.shape[0] < 1:
            raise ValueError(f"kernel_probe: query must be a device tensor [M, {x.shape[1]}]")
        true = None
        if query_labels is not None:
            q_np = (query_labels.detach().cpu().numpy() if torch.is_tensor(query_labels) else np.asarray(query_labels)).ravel()
            pos = np.minimum(np.searchsorted(uniq, q_np), G - 1)
            if q_np.shape[0] != query.shape[0] or not np.array_equal(uniq[pos], q_np):
                raise ValueError("kernel_probe: query_labels must be one value of `labels` per query row")
            true = pos.astype(np.int64)
    x = _prepared(x, transform)
    q = None if query is None else _prepared(query, transform)
    gammas = _resolved_gammas(x, gammas, scales)
    R = _sorted_row_sums(x, dense, G, gammas, extra=q)
    if q is None:
        fit = parzen_from_sums(R, dense, counts, prior)
    else:
        fit = parzen_from_sums(R[:, N:], np.full(q.shape[0], -1, dtype=np.int64), counts, prior)
    pred = fit["pred"]
    out = {"density": fit["density"], "pred": np.where(pred >= 0, uniq[np.maximum(pred, 0)], -1), "margin": fit["margin"], "gammas": gammas,
           "labels": uniq, "counts": counts}
    if true is not None:
        out.update(_probe_scores(pred, true, G))
    return out


def mmd_witness(embeddings, groups, pair, top_k=8, gammas=None, scales=RBF_SCALES, transform=None):
    """Which rows make two groups different: the MMD witness function between the two labels in `pair`, evaluated at every one of
    their rows (witness_from_sums; one pass of ops.pairdist_rbf_row_group_sums).  The rows of the two labels are pooled as
    mmd_permutation_test pools them (one gather, `transform` applied once, the bandwidths from the pooled rows unless `gammas` is
    given).  Returns {'witness': float64 [L, n] in pooled order, positive where pair[0]'s rows are denser, 'rows': int64 [n], the
    pooled rows' indices in the input, 'top': {'largest', 'smallest': int64 [L, top_k]}, per bandwidth the input indices of the
    top_k rows with the largest and with the smallest witness (the most typical rows of pair[0] and of pair[1]; the lower index
    first on a tie), 'mmd2': [L], the unbiased MMD^2 by the identity mean over pair[0]'s rows - mean over pair[1]'s rows,
    'gammas'}."""
    idx, xp, lab = _pooled_pair("mmd_witness", embeddings, groups, pair, transform)
    gammas = _resolved_gammas(xp, gammas, scales)
    counts = np.bincount(lab, minlength=2)
    w = witness_from_sums(_sorted_row_sums(xp, lab, 2, gammas), lab, counts, 0, 1)
    k = max(0, min(int(top_k), len(idx)))
    top = {"largest": np.stack([idx[np.argsort(-wl, kind="stable")[:k]] for wl in w]),
           "smallest": np.stack([idx[np.argsort(wl, kind="stable")[:k]] for wl in w])}
    return {"witness": w, "rows": idx, "top": top, "mmd2": w[:, lab == 0].mean(1) - w[:, lab == 1].mean(1), "gammas": gammas}


def kernel_alignment(embeddings, labels=None, gammas=None, scales=RBF_SCALES, transform=None):
    """The normalised HSIC (centred kernel alignment, CKA) between the RBF kernel of a split's rows and the delta kernel of a
    labelling, per bandwidth: `mmd`'s 'hsic' on a scale in [0, 1] that does not move with the bandwidth or the representation, so
    that raw, adapter and erased rows can be put side by side.  `embeddings`, `labels` (at most 16), `transform` and the default
    bandwidths as in `kernel_probe`.

    Two passes: ops.pairdist_rbf_row_group_sums at gamma -- the bucket sums K are segment sums of R by the rows' label (ordered
    pairs; the diagonal buckets are halved to unordered pairs), the row sums give B --, and one ops.pairdist_rbf_group_sums call at
    2 gamma with a single label (only the total of k^2 is needed; that pass walks half the tiles).  Returns alignment_from_sums'
    dict plus 'gammas', 'labels', 'counts'.  Because the second pass runs at 2 gamma the kernels' preconditions are halved:
    2 gamma_max max d^2 <= 80 and 2 gamma_max (|a|^2 + |b|^2) <= 64 for centred rows a, b.  Read 'rel_bound' with 'alignment'."""
    x, uniq, dense, counts = _labelled_rows("kernel_alignment", embeddings, labels, ops.PAIRDIST_ROWS_MAX_G, device="last")
    G, N = len(uniq), x.shape[0]
    x = _prepared(x, transform)
    gammas = _resolved_gammas(x, gammas, scales)
    R = _sorted_row_sums(x, dense, G, gammas)
    S = np.stack([R[:, dense == a].sum(1) for a in range(G)], axis=1)            # [L, G, G]: ordered pairs, row in a, column in b
    K = 0.5 * (S + S.transpose(0, 2, 1))
    d = np.arange(G)
    K[:, d, d] = 0.5 * S[:, d, d]
    rows = 1.0 + R.sum(2)
    center = torch.from_numpy((_column_sums(x) / N).astype(np.float32)).to(x.device)
    K2 = ops.pairdist_rbf_group_sums(x, torch.zeros(N, dtype=torch.int64, device=x.device), 1, center, (2.0 * gammas).tolist()).cpu().numpy()
    out = alignment_from_sums(K, K2[:, 0, 0], (rows * rows).sum(1), counts)
    out.update(gammas=gammas, labels=uniq, counts=counts)
    return out


def probe_report(train_table, val_table, test_table, transform=None, scales=RBF_SCALES):
    """How readable the groups, and within each class the spurious attribute, are NON-linearly in a representation: {'train': r,
    'val': r, 'test': r} with r = {'group': the leave-one-out balanced accuracy [L] of `kernel_probe` over targets_group,
    'spurious_within_class': {class: the leave-one-out balanced accuracy [L] of targets_spurious among that class's rows, nan if
    only one place is present}, 'spurious_alignment': `kernel_alignment`'s [L] against targets_spurious (nan if only one place is
    present)} and, for val and test, 'spurious_from_train': the balanced accuracy [L] of the split's rows as queries against train's
    rows and targets_spurious.  Every call takes its bandwidths from its own (reference) rows.  `transform` is applied once per
    split, as in dependence_report: run it raw, with an adapter, and on erased_table's rows."""
    out, nan = {}, np.full(len(scales), np.nan)
    train_x, train_c = None, None
    for split, table in (("train", train_table), ("val", val_table), ("test", test_table)):
        x = _device_rows(table, transform)
        y, c = table.targets.cpu().numpy(), table.targets_spurious.cpu().numpy()
        within = {}
        for cls in np.unique(y):
            idx = np.flatnonzero(y == cls)
            if len(np.unique(c[idx])) < 2:
                within[int(cls)] = nan.copy()
                continue
            within[int(cls)] = kernel_probe(ops.gather_rows(x, torch.from_numpy(idx).to(x.device)), c[idx], scales=scales)["balanced_accuracy"]
        both = len(np.unique(c)) >= 2
        out[split] = {"group": kernel_probe(x, table.targets_group.cpu().numpy(), scales=scales)["balanced_accuracy"],
                      "spurious_within_class": within,
                      "spurious_alignment": kernel_alignment(x, c, scales=scales)["alignment"] if both else nan.copy()}
        if split == "train":
            train_x, train_c = x, c
        else:
            ok = len(np.unique(train_c)) >= 2 and np.isin(c, train_c).all()
            out[split]["spurious_from_train"] = (kernel_probe(train_x, train_c, scales=scales, query=x, query_labels=c)["balanced_accuracy"]
                                                 if ok else nan.copy())
    return out


# ---- kernel ridge regression: the trained non-linear probe ------------------------------------------------------------------------------
# The Parzen probe above sees kernel densities only, and misses a labelling whose classes share their means and their density scale (the
# radius of a ring, an XOR of two coordinates).  Kernel ridge regression on the same RBF kernel reads those: alpha = (K + lam I)^-1 T for
# the centred one-hot targets T, convex and exact, no learning rate, stopped at a residual.  The one primitive it needs of the device is the
# product of the kernel matrix with a few dense columns without the N x N matrix (ops.pairdist_rbf_matvec); the solver is conjugate
# gradients on the host's side of that product, in float64 torch on the device.  Every step but the product runs anywhere.

RIDGE_LAMS = (0.1, 1.0)
RIDGE_MAX_COLUMNS = 16    # ops.PAIRDIST_MATVEC_MAX_C: the (lam, label) pairs of one fit are the columns of one product


def cg_solve(matvec, B, shifts, tol=1e-5, max_iter=256):
    """Conjugate gradients on (M + shifts[c] I) X[:, c] = B[:, c] for all columns together, M symmetric positive semi-definite and
    known only through matvec(V) -> M V (float64 [n, C] in, float64 [n, C] out).  Float64 torch on B's device; ONE product per
    iteration, shared by all columns; every column has its own step lengths and stops on its own: once its recurrence residual is
    at most tol ||B[:, c]|| the column is frozen -- its iterate stays, its search direction is handed to matvec as zeros (which
    ops.pairdist_rbf_matvec skips).  A zero right-hand side gives exact zeros, a zero curvature freezes the column.  After the
    loop the TRUE residual B - (M + shift) X is formed with one more product.  Returns {'x': float64 [n, C], 'iterations': the
    products of the loop, 'residual': float64 [C], the true residual's norm over ||B[:, c]|| (0 for a zero column), 'converged':
    bool [C], the recurrence residual reached tol within max_iter}.  No random numbers, no atomics: the same bits on every call
    if matvec gives the same bits."""
    if not torch.is_tensor(B) or B.dim() != 2:
        raise ValueError("cg_solve: B must be a tensor [n, C]")
    B = B.double()
    shifts = torch.as_tensor(np.asarray(shifts, dtype=np.float64).ravel(), device=B.device)
    if shifts.shape[0] != B.shape[1]:
        raise ValueError(f"cg_solve: {shifts.shape[0]} shifts for {B.shape[1]} columns")
    if not (tol > 0 and max_iter >= 0):
        raise ValueError(f"cg_solve: tol = {tol!r}, max_iter = {max_iter!r}")
    apply = lambda V: matvec(V).double() + shifts * V
    bnorm = B.norm(dim=0)
    X = torch.zeros_like(B)
    R = B.clone()
    rs = (R * R).sum(0)
    active = rs.sqrt() > tol * bnorm                                   # a zero column is converged at the start
    P = torch.where(active, R, torch.zeros_like(R))
    it = 0
    while it < max_iter and bool(active.any()):
        Q = apply(P)
        pq = (P * Q).sum(0)
        step = active & (pq > 0)
        a = torch.where(step, rs / torch.where(step, pq, torch.ones_like(pq)), torch.zeros_like(pq))
        X += a * P
        R -= a * Q
        rs_new = (R * R).sum(0)
        go = step & (rs_new.sqrt() > tol * bnorm)
        beta = torch.where(go, rs_new / torch.where(go, rs, torch.ones_like(rs)), torch.zeros_like(rs))
        P = torch.where(go, R + beta * P, torch.zeros_like(R))
        rs = torch.where(active, rs_new, rs)
        active = go
        it += 1
    converged = rs.sqrt() <= tol * bnorm
    true = (B - apply(X)).norm(dim=0)
    residual = torch.where(bnorm > 0, true / torch.where(bnorm > 0, bnorm, torch.ones_like(bnorm)), torch.zeros_like(bnorm))
    return {"x": X, "iterations": it, "residual": residual, "converged": converged}


def _ridge_lams(what, lams, G):
    """float64 [n_lam], every value finite and > 0 (else ValueError), n_lam * G columns at most RIDGE_MAX_COLUMNS (else DbmmUnsupported)"""
    lams = np.asarray(lams, dtype=np.float64).ravel()
    if lams.size == 0 or not (np.isfinite(lams).all() and (lams > 0).all()):
        raise ValueError(f"{what}: lams = {lams.tolist()}; at least one ridge, every one finite and > 0")
    if G is not None and lams.size * G > RIDGE_MAX_COLUMNS:
        raise ops.DbmmUnsupported(f"{what}: {lams.size} ridges x {G} labels = {lams.size * G} columns; one product carries at most {RIDGE_MAX_COLUMNS}")
    return lams


def _ridge_from_operator(product, dense, G, gammas, lams, tol, max_iter, device):
    """The host step of `kernel_ridge_fit`: product(gamma, V) -> K0 V, float64 [N, C], for the kernel matrix with a ZERO diagonal (what
    ops.pairdist_rbf_matvec gives; a dense float64 matrix serves as well).  Targets: the one-hot columns of the dense labels minus
    the label frequencies; one cg_solve per bandwidth on (K0 + (1 + lam) I) alpha = T with the (lam, label) pairs as columns.
    Returns (alpha float64 [L, n_lam, N, G], iterations int64 [L], residual [L, n_lam, G], converged bool [L, n_lam, G], frequencies
    float64 [G])."""
    dense_t = torch.as_tensor(dense, device=device)
    N, n_lam = dense_t.shape[0], len(lams)
    freq = np.bincount(dense, minlength=G).astype(np.float64) / N
    T = (dense_t.unsqueeze(1) == torch.arange(G, device=device).unsqueeze(0)).double() - torch.as_tensor(freq, device=device)
    B = T.repeat(1, n_lam)                                              # column a * G + g: ridge a, label g
    shifts = np.repeat(1.0 + np.asarray(lams, dtype=np.float64), G)
    alpha, its, res, conv = [], [], [], []
    for gam in gammas:
        sol = cg_solve(lambda V: product(float(gam), V), B, shifts, tol, max_iter)
        alpha.append(sol["x"].reshape(N, n_lam, G).permute(1, 0, 2))
        its.append(sol["iterations"])
        res.append(sol["residual"].reshape(n_lam, G).cpu().numpy())
        conv.append(sol["converged"].reshape(n_lam, G).cpu().numpy())
    return torch.stack(alpha).contiguous(), np.asarray(its, dtype=np.int64), np.stack(res), np.stack(conv), freq


def _ridge_product(x, center):
    """product(gamma, V) on the device: the float64 iterate rounded to fp32, one pass of ops.pairdist_rbf_matvec"""
    return lambda gam, V: ops.pairdist_rbf_matvec(x, V.float().contiguous(), center, gam)


def kernel_ridge_fit(embeddings, labels=None, gammas=None, scales=RBF_SCALES, lams=RIDGE_LAMS, transform=None, tol=1e-5, max_iter=256):
    """Kernel ridge regression of a labelling on a split's rows, RBF kernel: alpha = (K + lam I)^-1 T per bandwidth and ridge, K the
    kernel matrix with its unit diagonal, T the one-hot label columns minus the label frequencies (the frequencies are the
    intercept of the scores).  Nothing N x N is stored: conjugate gradients (`cg_solve`) on ops.pairdist_rbf_matvec, one product
    per iteration for all (lam, label) columns of a bandwidth, the weights handed to the kernel being the float64 iterate rounded to
    fp32.  `embeddings`, `labels`, `transform` and the default bandwidths as in `kernel_probe` (at most 16 labels: more raise
    DbmmUnsupported, fewer than two ValueError); every `lam` > 0 (else ValueError) and len(lams) * labels <= 16 (else
    DbmmUnsupported) -- all of it before anything is launched.  The rows keep the input's order; the centre is their mean.

    Returns {'alpha': float64 [L, n_lam, N, G] on the device, 'rows': the fp32 rows as given to the kernel, 'center', 'gammas',
    'lams', 'labels': the unique labels, 'counts', 'intercept': float64 [G], 'iterations': int64 [L], 'residual' and 'converged':
    [L, n_lam, G] -- the TRUE relative residual ||(K + lam I) alpha - T|| / ||T|| formed with one more product, and whether the
    recurrence reached `tol` within `max_iter`; non-convergence is reported, never raised --, 'transform', 'tol'}.  In the
    float64 study of this function CG took 5 - 50 iterations at lam in {0.1, 1} and up to 210 at lam = 1e-3."""
    lams = _ridge_lams("kernel_ridge_fit", lams, None)
    x, uniq, dense, counts = _labelled_rows("kernel_ridge_fit", embeddings, labels, RIDGE_MAX_COLUMNS, device=None)
    G = len(uniq)
    _ridge_lams("kernel_ridge_fit", lams, G)
    _need_device(x)
    x = _prepared(x, transform)
    gammas = _resolved_gammas(x, gammas, scales)
    if gammas.size == 0 or not (np.isfinite(gammas).all() and (gammas > 0).all()):
        raise ValueError(f"kernel_ridge_fit: gammas = {gammas.tolist()}; at least one bandwidth, every one finite and > 0")
    center = torch.from_numpy((_column_sums(x) / x.shape[0]).astype(np.float32)).to(x.device)
    alpha, its, res, conv, freq = _ridge_from_operator(_ridge_product(x, center), dense, G, gammas, lams, tol, max_iter, x.device)
    return {"alpha": alpha, "rows": x, "center": center, "gammas": gammas, "lams": lams, "labels": uniq, "counts": counts, "intercept": freq,
            "iterations": its, "residual": res, "converged": conv, "transform": transform, "tol": tol}


def _ridge_scores(product, alpha, intercept, gammas, M):
    """The host step of `kernel_ridge_predict`: product(gamma, W) on the rows [train; query] with the weights W = [alpha; 0], the query
    rows of the result plus the intercept.  scores float64 [L, n_lam, M, G] (host), pred int64 [L, n_lam, M] (dense: the first
    maximum), margin [L, n_lam, M]: the gap between the two highest scores."""
    L, n_lam, N, G = alpha.shape
    scores = []
    for l, gam in enumerate(gammas):
        W = torch.cat([alpha[l].permute(1, 0, 2).reshape(N, n_lam * G), torch.zeros(M, n_lam * G, dtype=alpha.dtype, device=alpha.device)])
        scores.append(product(float(gam), W)[N:].reshape(M, n_lam, G).permute(1, 0, 2))
    scores = torch.stack(scores).cpu().numpy() + np.asarray(intercept, dtype=np.float64)
    top = np.sort(scores, axis=3)
    return scores, scores.argmax(axis=3).astype(np.int64), top[..., -1] - top[..., -2]


def kernel_ridge_predict(fit, query):
    """The scores of the query rows under a `kernel_ridge_fit`: s[l, a, q, g] = sum_j k_l(query[q], x_j) alpha[l, a, j, g] +
    intercept[g].  `query`: a device tensor [M, D]; the fit's `transform` is applied.  One product per bandwidth on the rows
    [train; query] with the weights [alpha; 0]: the query rows carry zero weights, so their column blocks are skipped, and the
    query rows of the result are the scores.  The train-against-train tiles of that pass are wasted work (N / (N + M) of the
    tiles that carry weight); a rectangular pass is a later change.  Returns {'scores': float64 [L, n_lam, M, G], 'pred':
    [L, n_lam, M] as values of the fit's `labels`, 'pred_dense': the same as indices into `labels`, 'margin': [L, n_lam, M], the
    gap between the two highest scores}."""
    x = fit["rows"]
    if not torch.is_tensor(query) or not query.is_cuda or query.dim() != 2 or query.shape[0] < 1:
        raise ValueError("kernel_ridge_predict: query must be a device tensor [M, D]")
    q = _prepared(query, fit["transform"])
    if q.shape[1] != x.shape[1]:
        raise ValueError(f"kernel_ridge_predict: query rows have {q.shape[1]} columns, the fit's {x.shape[1]}")
    rows = torch.cat([x, q])
    scores, pred, margin = _ridge_scores(_ridge_product(rows, fit["center"]), fit["alpha"], fit["intercept"], fit["gammas"], q.shape[0])
    return {"scores": scores, "pred": fit["labels"][pred], "pred_dense": pred, "margin": margin}


def stratified_holdout(dense, holdout, seed):
    """(fit rows, held-out rows), both sorted int64: a `holdout` share of every label's rows, rounded to the nearest count but at
    least one row of the label on each side (a label's only row stays with the fit), drawn label by label from a private
    np.random.RandomState(seed).  `holdout` outside (0, 1) raises ValueError."""
    if not (isinstance(holdout, (int, float)) and 0.0 < holdout < 1.0):
        raise ValueError(f"holdout = {holdout!r}; a share in (0, 1)")
    dense = np.asarray(dense).ravel()
    rng = np.random.RandomState(seed)
    held = []
    for g in np.unique(dense):
        idx = np.flatnonzero(dense == g)
        k = min(max(int(round(holdout * len(idx))), 1), len(idx) - 1)
        held.append(idx[rng.permutation(len(idx))[:k]])
    held = np.sort(np.concatenate(held)).astype(np.int64)
    return np.setdiff1d(np.arange(len(dense), dtype=np.int64), held), held


def _ridge_best(bal, gammas, lams):
    """the (bandwidth, ridge) of highest balanced accuracy, ties toward the smaller gamma and then the larger lam"""
    best = None
    for l in np.argsort(gammas, kind="stable"):
        for a in np.argsort(-np.asarray(lams), kind="stable"):
            if best is None or bal[l, a] > bal[best]:
                best = (int(l), int(a))
    return {"index": best, "gamma": float(gammas[best[0]]), "lam": float(lams[best[1]]), "balanced_accuracy": float(bal[best])}


def kernel_ridge_probe(embeddings, labels=None, query=None, query_labels=None, holdout=0.25, seed=0, **fit_kw):
    """The kernel ridge probe: how well a labelling is read off a split's rows by kernel ridge regression, as held-out accuracy.
    With `query` (a device tensor [M, D]) and `query_labels` [M] (values of `labels`): fit on the rows, score the query rows.
    Without: a stratified `holdout` share of every label is held out (`stratified_holdout`, deterministic in `seed`), the fit
    runs on the rest and the held-out rows are scored.  `fit_kw`: kernel_ridge_fit's gammas, scales, lams, transform, tol, max_iter.

    Returns {'accuracy', 'balanced_accuracy': [L, n_lam], 'recall': [L, n_lam, G] (nan for a label without scored rows), 'best':
    {'index': (l, a), 'gamma', 'lam', 'balanced_accuracy'}, the (bandwidth, ridge) of highest balanced accuracy, ties toward the
    smaller gamma and then the larger lam, 'pred': [L, n_lam, M] (values of `labels`), 'scores', 'margin', 'held_out': the
    held-out rows' indices (None with `query`), and the fit's 'gammas', 'lams', 'labels', 'counts', 'iterations', 'residual',
    'converged'}.  Read 'converged' and 'residual' beside the accuracies."""
    if query is None:
        if not (isinstance(holdout, (int, float)) and 0.0 < holdout < 1.0):
            raise ValueError(f"kernel_ridge_probe: holdout = {holdout!r}; a share in (0, 1)")
        x, uniq, dense, _ = _labelled_rows("kernel_ridge_probe", embeddings, labels, RIDGE_MAX_COLUMNS, device=None)
        l_np = uniq[dense]
        _ridge_lams("kernel_ridge_probe", fit_kw.get("lams", RIDGE_LAMS), len(uniq))
        _need_device(x)
        keep, held = stratified_holdout(dense, holdout, seed)
        x = _prepared(x)
        fit = kernel_ridge_fit(ops.gather_rows(x, torch.from_numpy(keep).to(x.device)), l_np[keep], **fit_kw)
        query, query_labels = ops.gather_rows(x, torch.from_numpy(held).to(x.device)), l_np[held]
    else:
        if query_labels is None:
            raise ValueError("kernel_ridge_probe: `query` rows need their `query_labels`")
        held = None
        fit = kernel_ridge_fit(embeddings, labels, **fit_kw)
    uniq, G = fit["labels"], len(fit["labels"])
    q_np = (query_labels.detach().cpu().numpy() if torch.is_tensor(query_labels) else np.asarray(query_labels)).ravel()
    pos = np.minimum(np.searchsorted(uniq, q_np), G - 1)
    if q_np.shape[0] != query.shape[0] or not np.array_equal(uniq[pos], q_np):
        raise ValueError("kernel_ridge_probe: query_labels must be one value of `labels` per query row")
    out = kernel_ridge_predict(fit, query)
    L, n_lam = len(fit["gammas"]), len(fit["lams"])
    sc = _probe_scores(out["pred_dense"].reshape(L * n_lam, -1), pos.astype(np.int64), G)
    res = {"accuracy": sc["accuracy"].reshape(L, n_lam), "recall": sc["recall"].reshape(L, n_lam, G),
           "balanced_accuracy": sc["balanced_accuracy"].reshape(L, n_lam)}
    res["best"] = _ridge_best(res["balanced_accuracy"], fit["gammas"], fit["lams"])
    res.update(pred=out["pred"], scores=out["scores"], margin=out["margin"], held_out=held)
    res.update({k: fit[k] for k in ("gammas", "lams", "labels", "counts", "iterations", "residual", "converged")})
    return res


def ridge_report(train_table, val_table, test_table, transform=None, **kw):
    """How readable the spurious attribute is to a TRAINED non-linear probe: `kernel_ridge_fit` on train's rows for targets_spurious,
    and for targets_spurious among each class's rows, scored on val and on test (`kernel_ridge_predict`).  {'val': r, 'test': r}
    with r = {'spurious': the balanced accuracy [L, n_lam] of the split's rows, 'spurious_within_class': {class: the same among
    that class's rows}, 'best': kernel_ridge_probe's 'best' for 'spurious'}; nan where train has one place only (or none of the
    class) or the split has a place train has not.  `transform` is applied once per split, `kw` goes to kernel_ridge_fit: run it
    raw, with an adapter as `transform=`, and on erased_table's rows."""
    xs = [_device_rows(t, transform) for t in (train_table, val_table, test_table)]
    ys = [t.targets.cpu().numpy() for t in (train_table, val_table, test_table)]
    cs = [t.targets_spurious.cpu().numpy() for t in (train_table, val_table, test_table)]
    L = len(kw["gammas"]) if kw.get("gammas") is not None else len(kw.get("scales", RBF_SCALES))
    nan = np.full((L, len(np.asarray(kw.get("lams", RIDGE_LAMS)).ravel())), np.nan)
    out = {"val": {"spurious_within_class": {}}, "test": {"spurious_within_class": {}}}

    def scored(rows_of):
        """per split the balanced accuracy (and best) of a fit on train's selected rows"""
        tr = rows_of(0)
        res = {}
        for k, split in ((1, "val"), (2, "test")):
            q = rows_of(k)
            ok = len(tr) and len(q) and len(np.unique(cs[0][tr])) >= 2 and np.isin(cs[k][q], cs[0][tr]).all()
            if not ok:
                res[split] = None
                continue
            sub = lambda j, idx: ops.gather_rows(xs[j], torch.from_numpy(idx).to(xs[j].device))
            res[split] = kernel_ridge_probe(sub(0, tr), cs[0][tr], query=sub(k, q), query_labels=cs[k][q], **kw)
        return res

    whole = scored(lambda k: np.arange(len(ys[k]), dtype=np.int64))
    for split in out:
        out[split]["spurious"] = nan.copy() if whole[split] is None else whole[split]["balanced_accuracy"]
        out[split]["best"] = None if whole[split] is None else whole[split]["best"]
    for cls in np.unique(ys[0]):
        within = scored(lambda k: np.flatnonzero(ys[k] == cls))
        for split in out:
            out[split]["spurious_within_class"][int(cls)] = nan.copy() if within[split] is None else within[split]["balanced_accuracy"]
    return out


# ---- linear concept erasure: the rows changed so that no linear classifier reads a labelling (Belrose et al. 2023, "LEACE") ---------------
# Post-hoc debiasing of frozen embeddings, in closed form from three moments: the column sums, the scatter matrix (ops.covariance) and
# the per-label column sums (ops.label_column_sums), each one read of the rows.  The eraser is x -> x - sum_k ((x - mean) . A_k) B_k with
# r <= G - 1 vector pairs; ops.erase_rows applies it in one read and one write.  separation_report and cluster_agreement measure what it
# destroys; every training path runs unchanged on erased_table's rows.

ERASURE_METHODS = ("leace", "orth")
ERASURE_MAX_LABELS = 16   # ops.LABEL_SUMS_MAX_G
ERASURE_RANK_RTOL = 1e-10  # a singular value of the decomposed matrix counts above this fraction of the largest ...
ERASURE_RANK_FLOOR = 1e-5  # ... as long as the cross-covariance itself has that many above this fraction of sqrt(lambda_max)
ERASURE_FP32_RIDGE = 2.0 ** -24  # erasure_fit's ridge per dimension: its scatter matrix is fp32-accurate


def erasure_from_moments(scatter, center, mean, n, label_sums, counts, method="leace", ridge=0.0):
    """The host step of `erasure_fit`, numpy only.  scatter float64 [D, D]: sum_i (x_i - center)(x_i - center)^T about `center` (any
    vector near the mean, as pca_from_scatter takes it); mean float64 [D]: the rows' mean; n rows; label_sums float64 [G, D]: the RAW
    per-label sums of the rows; counts [G]: the rows per label (they add up to n).

    With Sxx = (scatter - n (mean - center)(mean - center)^T) / n and Sxz [D, G], column g = (label_sums[g] - counts[g] mean) / n:
      "leace"  W = Sxx^(-1/2), Wp = Sxx^(1/2) from one eigh, eigenvalues below D eps lambda_max dropped (a pseudo-inverse: n < D works);
               U = an orthonormal basis of the column space of W Sxz (SVD); A = (W U)^T, B = (Wp U)^T: the least change of the rows,
               in the norm Sxx^-1 induces, after which every label's mean is the overall mean (Belrose et al. 2023, theorem 4.3).
      "orth"   U = a basis of the column space of Sxz; A = B = U^T: the mean projection (Haghighatkhah et al. 2022).
    Both erase by x -> x - sum_k ((x - mean) . A_k) B_k.

    The rank r is the number of singular values of the decomposed matrix above 1e-10 of the largest, but no more than the number of
    singular values of Sxz ITSELF above 1e-5 sqrt(lambda_max): the columns add up to zero, so r <= G - 1, and what a previous
    erasure left behind -- the rounding of float32 rows, 2^-24 of their entries -- is rank 0, not G - 1 directions of noise.  That
    floor is taken on Sxz because the whitening multiplies noise along a direction of small variance by 1 / its deviation.

    `ridge` (a fraction of lambda_max, "leace" only) is added to every kept eigenvalue before the two roots are taken: Wp W stays
    the identity on the kept directions, so the erasure stays exact, it is least in the norm (Sxx + ridge lambda_max I)^-1, and W
    is bounded by (ridge lambda_max)^(-1/2).  For a scatter matrix that is itself rounded (erasure_fit's comes from fp32 products):
    its null directions (n < D) come out with eigenvalues of either sign at the rounding level, and without a ridge the positive
    ones are whitened by 1 / sqrt(noise).

    Returns {'mean' float32 [D], 'A' float32 [r, D], 'B' float32 [r, D], 'rank', 'method', 'singular_values' float64 [G] (of the
    decomposed matrix)}.  Rank 0 (one label, or labels whose means coincide) is a valid fit with empty A and B.  An unknown
    method, a label with count 0, n < 2 and a negative ridge raise ValueError."""
    mean, A, B, sv = _erasure_vectors64(scatter, center, mean, n, label_sums, counts, method, ridge)
    r, D = A.shape
    return {"mean": mean.astype(np.float32), "A": np.ascontiguousarray(A, dtype=np.float32).reshape(r, D),
            "B": np.ascontiguousarray(B, dtype=np.float32).reshape(r, D), "rank": r, "method": method, "singular_values": sv}


def _erasure_vectors64(scatter, center, mean, n, label_sums, counts, method, ridge=0.0):
    """erasure_from_moments before its float32 rounding: (mean [D], A [r, D], B [r, D], singular values [G]), float64"""
    if method not in ERASURE_METHODS:
        raise ValueError(f"erasure: method = {method!r}; one of {ERASURE_METHODS}")
    if not ridge >= 0.0:
        raise ValueError(f"erasure: ridge = {ridge}; a fraction of the largest eigenvalue, not negative")
    scatter = np.asarray(scatter, dtype=np.float64)
    sums = np.asarray(label_sums, dtype=np.float64)
    cnt = np.asarray(counts).astype(np.int64).ravel()
    D = scatter.shape[0]
    if scatter.shape != (D, D) or sums.ndim != 2 or sums.shape[1] != D or cnt.shape != (sums.shape[0],):
        raise ValueError(f"erasure: scatter {scatter.shape}, label_sums {sums.shape}, counts {cnt.shape}")
    G = sums.shape[0]
    if not 1 <= G <= ERASURE_MAX_LABELS:
        raise ValueError(f"erasure: {G} labels (1..{ERASURE_MAX_LABELS})")
    if n < 2:
        raise ValueError(f"erasure needs at least two rows, got {n}")
    if (cnt <= 0).any() or cnt.sum() != n:
        raise ValueError(f"erasure: counts {cnt.tolist()} for {n} rows; every label needs a row and every row a label")
    mean = np.asarray(mean, dtype=np.float64)
    d = mean - np.asarray(center).astype(np.float64)
    Sxx = (scatter - np.float64(n) * np.outer(d, d)) / np.float64(n)
    Sxz = (sums - cnt.astype(np.float64)[:, None] * mean[None, :]).T / np.float64(n)          # [D, G]
    w, V = np.linalg.eigh(Sxx)                                                                   # ascending
    top = max(w[-1], 0.0)
    raw = np.linalg.svd(Sxz, compute_uv=False)
    above = int((raw > ERASURE_RANK_FLOOR * np.sqrt(top)).sum())                                 # what stands above the rows' own rounding
    if method == "leace":
        keep = w > D * np.finfo(np.float64).eps * top
        w, V = w[keep] + ridge * top, V[:, keep]
        root = np.sqrt(w)
        W, Wp = (V / root) @ V.T, (V * root) @ V.T
        M = W @ Sxz
    else:
        W = Wp = None
        M = Sxz
    U, s, _ = np.linalg.svd(M, full_matrices=False)                                              # s descending, [min(D, G)]
    r = min(int((s > ERASURE_RANK_RTOL * s[0]).sum()), above) if s[0] > 0 else 0
    U = U[:, :r]
    A, B = (U.T, U.T) if method == "orth" else ((W @ U).T, (Wp @ U).T)
    sv = np.zeros(G, dtype=np.float64)
    sv[:len(s)] = s
    return mean, np.asarray(A).reshape(r, D), np.asarray(B).reshape(r, D), sv


def balanced_rows(labels, seed=0):
    """Sorted int64 indices of min-count rows of every label (np.unique order), drawn without replacement from a private
    np.random.RandomState(seed): the global stream is left alone.  Fitting an eraser on the group-balanced rows
    (balanced_rows(table.group_array)) makes the erased attribute independent of the class there, so that erasing it does not take
    the class with it: on a confounded split the spurious attribute's direction IS partly the class's."""
    l = labels.detach().cpu().numpy() if torch.is_tensor(labels) else np.asarray(labels)
    l = l.ravel()
    if l.size == 0:
        raise ValueError("balanced_rows: no labels")
    uniq, dense, counts = np.unique(l, return_inverse=True, return_counts=True)
    rng, m = np.random.RandomState(seed), int(counts.min())
    picks = [rng.choice(np.flatnonzero(dense == g), size=m, replace=False) for g in range(len(uniq))]
    return np.sort(np.concatenate(picks)).astype(np.int64)


def erasure_fit(embeddings, labels=None, method="leace", rows=None, transform=None):
    """The eraser of a labelling of a split's rows (`erasure_from_moments`' dict plus 'labels': the unique labels, 'counts' and 'n').

    `embeddings`: an EmbeddingTable (its targets_spurious unless `labels` is given) or a device tensor [N, D] with `labels` [N]: any
    integers -- the spurious attribute, the groups, `pseudo_groups`' clusters --, mapped to dense ids by np.unique; more than 16
    raise ValueError before anything is launched, like an unknown method.  `rows`: an int64 index set (`balanced_rows`): the fit
    uses ops.gather_rows of those rows and their labels only.  `transform` (a callable emb -> emb) is applied batch by batch in
    eval mode first, as in `kmeans` / `silhouette`.

    Three reads of the rows and nothing N x D allocated apart from the gathered or transformed rows when they are asked for:
    _column_sums for the centre (float32 of the fp32-block mean), ops.covariance for the scatter about it, ops.label_column_sums
    for the float64 per-label sums -- whose total over n is the float64 mean the fit centres on, so that the cross-covariance's
    columns add up to zero to the last bit's worth and the rank is G - 1, not G.  The scatter matrix is fp32-accurate (exact fp32
    products of rows centred in fp32), so "leace" whitens with erasure_from_moments' ridge = D 2^-24: the erasure stays exact, and
    the vectors stay bounded where the rows leave directions empty (n < D)."""
    if method not in ERASURE_METHODS:
        raise ValueError(f"erasure: method = {method!r}; one of {ERASURE_METHODS}")
    if isinstance(embeddings, trainer.EmbeddingTable) and labels is None:
        labels = embeddings.targets_spurious
    x, uniq, dense, _ = _labelled_rows("erasure_fit", embeddings, labels, min_labels=1)
    l_np = uniq[dense]
    if rows is not None:
        rows = np.asarray(rows.detach().cpu().numpy() if torch.is_tensor(rows) else rows).astype(np.int64).ravel()
        if rows.size == 0 or rows.min() < 0 or rows.max() >= x.shape[0]:
            raise ValueError(f"erasure_fit: rows must index the {x.shape[0]} rows")
        l_np = l_np[rows]
    uniq, dense = np.unique(l_np, return_inverse=True)
    G = len(uniq)
    if G > ERASURE_MAX_LABELS:
        raise ValueError(f"erasure_fit: {G} labels; at most {ERASURE_MAX_LABELS}")
    if l_np.shape[0] < 2:
        raise ValueError(f"erasure needs at least two rows, got {l_np.shape[0]}")
    x = _prepared(x)
    if rows is not None:
        x = ops.gather_rows(x, torch.from_numpy(rows).to(x.device))
    if transform is not None:
        x = _transformed_rows(x, transform, TRANSFORM_ROWS)
    n = x.shape[0]
    center = (_column_sums(x) / n).astype(np.float32)
    scatter = ops.covariance(x, torch.from_numpy(center).to(x.device))
    sums, counts = ops.label_column_sums(x, torch.from_numpy(dense.reshape(-1).astype(np.int64)).to(x.device), G)
    sums, counts = sums.cpu().numpy(), counts.cpu().numpy()
    fit = erasure_from_moments(scatter.cpu().numpy(), center, sums.sum(0) / n, n, sums, counts, method, ridge=x.shape[1] * ERASURE_FP32_RIDGE)
    fit.update(labels=uniq, counts=counts, n=n)
    return fit


def erase(fit, embeddings, out=None):
    """The rows of `embeddings` (an EmbeddingTable or a device tensor [N, D]) after the eraser `fit` (erasure_fit's dict), on the fused
    kernel (ops.erase_rows: one read, one write, nothing else allocated): a device tensor [N, D], or `out` -- which may be the
    input tensor itself: in place.  Rank 0 returns a copy (or `out` filled with the rows) and launches no kernel of ours."""
    x = embeddings.embeddings if isinstance(embeddings, trainer.EmbeddingTable) else embeddings
    _need_device(x)
    x = _prepared(x)
    if fit["rank"] == 0:
        if out is None:
            return x.clone()
        if out.data_ptr() != x.data_ptr():
            out.copy_(x)
        return out
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(x.device)
    return ops.erase_rows(x, dev(fit["mean"]), dev(fit["A"]), dev(fit["B"]), out=out)


def erased_table(table, fit):
    """An EmbeddingTable with the erased rows (a new tensor; the source is left alone) and the table's own labels, y_pred and
    filenames, built as pseudo_group_table builds its table: what train_all_epochs, train_sweep, train_jtt and the reports take."""
    out = trainer.EmbeddingTable(erase(fit, table), table.targets.cpu().numpy(), table.targets_spurious.cpu().numpy(), y_pred=None,
                                 filenames=table.filenames, device=table.device)
    out.y_pred = table.y_pred
    return out


def label_mean_gap(x, labels):
    """The largest |entry| of (a label's mean - the overall mean) over the labels of the rows x (device [N, D]), in float64 from
    ops.label_column_sums: what an eraser of that labelling brings to rounding level."""
    l_np = labels.detach().cpu().numpy() if torch.is_tensor(labels) else np.asarray(labels)
    uniq, dense = np.unique(l_np, return_inverse=True)
    sums, counts = ops.label_column_sums(x, torch.from_numpy(dense.reshape(-1).astype(np.int64)).to(x.device), len(uniq))
    sums, counts = sums.cpu().numpy(), counts.cpu().numpy().astype(np.float64)
    return float(np.abs(sums / counts[:, None] - sums.sum(0) / counts.sum()).max())


def erasure_report(opt, fit, train_table, val_table, test_table):
    """What an eraser does to the three splits: {'train': r, 'val': r, 'test': r} with r = {'before': m, 'after': m,
    'relative_change': ||r(X) - X||_F / ||X - mean||_F} and m = {'class': the class prompts' group accuracies
    (validate_zs_linear_probing on opt.text_embedding_dir), 'spurious_acc': the accuracy of the spurious prompts on the spurious
    attribute (the same function on opt.text_spurious_embedding_dir, target="spurious"), 'gap': label_mean_gap of the fit's
    labelling where the split carries it (the table's spurious attribute or groups; else None)}."""
    bs = max(int(getattr(opt, "batch_size", 0) or 0), 4096)
    ratio = train_table.group_ratio.numpy()
    mean = torch.from_numpy(fit["mean"])

    def measures(table, labels):
        return {"class": trainer.validate_zs_linear_probing(table, opt.text_embedding_dir, opt.zs_temperature, bs, ratio)[2],
                "spurious_acc": trainer.validate_zs_linear_probing(table, opt.text_spurious_embedding_dir, opt.zs_temperature, bs, ratio,
                                                                   target="spurious")[1],
                "gap": None if labels is None else label_mean_gap(table.embeddings, labels)}

    out = {}
    for split, table in (("train", train_table), ("val", val_table), ("test", test_table)):
        labels = None
        for cand in (table.targets_spurious, table.targets_group, table.targets):
            if np.array_equal(np.unique(cand.cpu().numpy()), np.asarray(fit["labels"])):
                labels = cand
                break
        after = erased_table(table, fit)
        m_dev, diff, spread = mean.to(table.device), 0.0, 0.0
        for i in range(0, len(table), bs):                                           # batch by batch: no second copy of the split in float64
            a, b = after.embeddings[i:i + bs].double(), table.embeddings[i:i + bs].double()
            diff += (a - b).pow(2).sum().item()
            spread += (b - m_dev).pow(2).sum().item()
        diff, spread = diff ** 0.5, spread ** 0.5
        out[split] = {"before": measures(table, labels), "after": measures(after, labels),
                      "relative_change": diff / spread if spread > 0 else 0.0}
    return out
