"""k-means pseudo-groups without a device: the C ABI's argument checks, the host functions of dbmm_amd.analysis (cluster_agreement,
the renumbering rule, pseudo_group_table), the schedule on a pseudo-group table with the step stood in for, and the float64
restatement of Lloyd's algorithm that tests/test_gpu_kmeans.py compares the kernels with -- the generator and the helpers are
defined here, once."""
import ctypes

import numpy as np
import pytest
import torch

from dbmm_amd import _lib, adapter, analysis, optim, trainer
from test_supcon_host import _setup, _stand_ins

# (N, D, K, sep, seed): the trajectory cases of tests/test_gpu_kmeans.py
TRAJECTORY_CASES = [(257, 64, 2, 6.0, 0), (70, 8, 16, 8.0, 0), (1000, 132, 3, 1.5, 0)]


# ---- the generator and the three helpers ------------------------------------------------------------------------------------------
def planted(N, D, K, sep, seed):
    """K planted clusters far from zero and close to each other -> (x fp32 [N, D], planted labels [N])"""
    r = np.random.RandomState(seed)
    base = 3 * r.standard_normal(D)
    cent = base + sep * r.standard_normal((K, D)) / np.sqrt(D)
    lab = r.randint(0, K, N)
    lab[:K] = np.arange(K)
    return np.float32(cent[lab] + r.standard_normal((N, D)) / np.sqrt(D)), lab


def distances64(x, centers):
    """float64 [N, K] squared distances, taken from the fp32 values"""
    x64 = np.asarray(x, dtype=np.float64)
    return np.stack([((x64 - np.asarray(c, dtype=np.float64)) ** 2).sum(1) for c in centers], axis=1)


def undecided(d2, D):
    """(mask [N] of the rows whose two smallest float64 distances have a relative gap <= 4 (D + 8) 2^-24 -- twice the worst-case
    bound of two fp32 sums of D squares --, the smallest relative gap); with one centre every row is decided"""
    if d2.shape[1] < 2:
        return np.zeros(d2.shape[0], dtype=bool), np.inf
    two = np.partition(d2, 1, axis=1)[:, :2]
    with np.errstate(divide="ignore", invalid="ignore"):
        gap = np.where(two[:, 1] > 0, (two[:, 1] - two[:, 0]) / two[:, 1], 0.0)
    return gap <= 4 * (D + 8) * 2.0 ** -24, float(gap.min())


def restatement(x, centers0, max_iter=100):
    """Plain Lloyd in numpy: float64 distances, argmin (the lowest index on a tie), float64 means rounded to fp32, an empty cluster
    keeps its centre, stop when no label changes -- the assignment that changes nothing is the last iteration and leaves the
    centres alone.  -> {'centers' fp32, 'labels', 'counts', 'iterations', 'converged', 'undecided': rows per iteration, 'gap': the
    smallest relative gap met}"""
    c = np.array(centers0, dtype=np.float32)
    K, D = c.shape
    labels = np.full(x.shape[0], -1)
    out = {"undecided": [], "gap": np.inf, "converged": False}
    x64 = x.astype(np.float64)
    for it in range(1, max_iter + 1):
        d2 = distances64(x, c)
        mask, gap = undecided(d2, D)
        out["undecided"].append(int(mask.sum()))
        out["gap"] = min(out["gap"], gap)
        new = d2.argmin(1)
        changed = int((new != labels).sum())
        labels = new
        if changed == 0:
            out["converged"] = True
            break
        for j in range(K):
            if (labels == j).any():
                c[j] = x64[labels == j].mean(0).astype(np.float32)
    out.update(centers=c, labels=labels, counts=np.bincount(labels, minlength=K), iterations=it)
    return out


def kmeans_pp_restated(x, k, seed):
    """the restatement's own k-means++: row indices, float64 distances, a private stream"""
    r = np.random.RandomState(seed)
    rows = [int(r.randint(x.shape[0]))]
    while len(rows) < k:
        cum = np.cumsum(distances64(x, x[rows]).min(1))
        rows.append(min(int(np.searchsorted(cum, r.random_sample() * cum[-1], side="right")), x.shape[0] - 1))
    return np.asarray(rows)


# ---- the restatement on the trajectory cases ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,iterations", zip(TRAJECTORY_CASES, (2, 2, 4)), ids=["k2", "k16", "k3_d132"])
def test_restatement_converges_with_every_row_decided(case, iterations):
    N, D, K, sep, seed = case
    x, _ = planted(N, D, K, sep, seed)
    ref = restatement(x, x[kmeans_pp_restated(x, K, seed)])
    print(case, "iterations", ref["iterations"], "undecided", ref["undecided"], "smallest gap", ref["gap"], "margin", 4 * (D + 8) * 2.0 ** -24)
    assert ref["converged"] and ref["iterations"] == iterations
    assert not any(ref["undecided"])
    assert ref["counts"].sum() == N


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def built():
    return _lib.lib()


def test_symbols_are_exported_and_bound(built):
    for name in ("dbmm_workspace_bytes_kmeans", "dbmm_kmeans_begin", "dbmm_kmeans_iterate", "dbmm_kmeans_assign"):
        assert name in _lib.EXPORTS and getattr(built, name).argtypes == _lib._SIGS[name]
    assert built.dbmm_workspace_bytes_kmeans.restype is ctypes.c_size_t
    assert _lib.kernel_source_hash("kmeans_assign_kernel") is not None


def test_workspace_bytes(built):
    W = built.dbmm_workspace_bytes_kmeans
    for N, D, K in ((1, 64, 2), (100, 0, 2), (100, 66, 2), (100, 64, 0), (100, 64, 17), (100, 4100, 2), (1 << 31, 64, 2)):
        assert W(N, D, K) == 0, (N, D, K)
    # status | centres | labels, dmin (padded to 16 bytes) | P (K D + 16 + 1) 8-byte words (+ padding)
    N, D, K = 257, 64, 2
    P = 5                                                            # min(2048 / 1 column slab, ceil(257 / 64))
    assert W(N, D, K) == 256 + K * D * 4 + 2 * 1040 + P * (K * D + 16) * 8 + 48
    N, D, K = 162770, 1024, 8
    P = 512                                                          # 2048 / 4 column slabs
    assert W(N, D, K) == 256 + K * D * 4 + 2 * 651088 + P * (K * D + 16 + 1) * 8
    assert W(N, D, K) < N * 16 + P * K * D * 8 + (1 << 17)           # O(N) + O(P K D), nothing N x D


def test_argument_checks_precede_any_launch(built):
    """no device is touched: the process has none, and every refusal comes back as a code"""
    p = ctypes.c_void_p(4096)
    odd = ctypes.c_void_p(4096 + 4)
    big = 1 << 30
    B, I, A = built.dbmm_kmeans_begin, built.dbmm_kmeans_iterate, built.dbmm_kmeans_assign

    def begin(c=p, N=100, D=64, K=4, ws=p, nbytes=big):
        return B(c, N, D, K, ws, nbytes, None)

    def iterate(x=p, N=100, D=64, K=4, n=1, ws=p, nbytes=big):
        return I(x, N, D, K, n, ws, nbytes, None)

    def assign(x=p, c=p, labels=p, dmin=p, N=100, D=64, K=4):
        return A(x, c, labels, dmin, N, D, K, None)
    for call in (begin, iterate, assign):
        assert call(K=0) == -1 and call(D=0) == -1 and call(D=66) == -1 and call(D=-4) == -1
        assert call(K=17) == -5 and call(D=4100) == -5
    assert begin(N=3) == -1 and iterate(N=3) == -1 and iterate(n=-1) == -1
    assert assign(N=0) == -1                                         # (N below K is served there: rows are placed at fitted centres)
    assert begin(c=None) == -4 and begin(ws=None) == -4 and iterate(x=None) == -4 and iterate(ws=None) == -4
    for k in ("x", "c", "labels", "dmin"):
        assert assign(**{k: None}) == -4, k
    need = built.dbmm_workspace_bytes_kmeans(100, 64, 4)
    assert need > 0 and begin(nbytes=need - 1) == -3 and iterate(nbytes=need - 1) == -3
    assert begin(c=odd) == -2 and begin(ws=odd) == -2 and iterate(x=odd) == -2 and iterate(ws=odd) == -2
    assert assign(x=odd) == -2 and assign(c=odd) == -2 and assign(labels=ctypes.c_void_p(4098)) == -2 and assign(dmin=ctypes.c_void_p(4097)) == -2
    assert iterate(n=0) == 0                                         # nothing to enqueue


# ---- cluster_agreement -------------------------------------------------------------------------------------------------------------------
def test_cluster_agreement_on_hand_computed_tables():
    a = np.array([0, 0, 0, 1, 1, 1, 1, 2, 2, 2])
    same = analysis.cluster_agreement(np.array([5, 5, 5, 2, 2, 2, 2, 9, 9, 9]), a)      # a renaming: rows in np.unique order (2, 5, 9)
    assert same["table"].tolist() == [[0, 4, 0], [3, 0, 0], [0, 0, 3]]
    assert same["purity"] == 1.0 and same["ari"] == 1.0
    # clusters (0 0 1 1 2 2) against groups (0 0 0 1 1 1): cells (2 0 | 1 1 | 0 2): sum C(n_ij, 2) = 2, rows 3, columns 6, all 15
    r = analysis.cluster_agreement([0, 0, 1, 1, 2, 2], [0, 0, 0, 1, 1, 1])
    assert r["table"].tolist() == [[2, 0], [1, 1], [0, 2]]
    assert r["purity"] == 5 / 6
    assert abs(r["ari"] - (2 - 3 * 6 / 15) / (0.5 * (3 + 6) - 3 * 6 / 15)) < 1e-15
    # independent partitions: a full 2 x 2 design with equal cells has ARI -1 / (2 n - 3) exactly (n rows per cell ... here 4 n = 400)
    g = np.repeat([0, 1], 200)
    c = np.tile([0, 1], 200)
    ind = analysis.cluster_agreement(c, g)
    assert ind["table"].tolist() == [[100, 100], [100, 100]] and ind["purity"] == 0.5
    assert abs(ind["ari"]) < 0.01
    rs = np.random.RandomState(3)
    assert abs(analysis.cluster_agreement(rs.randint(0, 3, 5000), rs.randint(0, 2, 5000))["ari"]) < 0.01
    assert analysis.cluster_agreement([0, 0, 0], [7, 7, 7])["ari"] == 1.0                  # one block each
    with pytest.raises(ValueError):
        analysis.cluster_agreement([0, 1], [0, 1, 1])


def test_renumbering_rule():
    """by size, descending; the lower original index first on a tie"""
    assert analysis.size_order([3, 9, 3, 12]).tolist() == [3, 1, 0, 2]
    assert analysis.size_order([5, 5]).tolist() == [0, 1]
    assert analysis.size_order([0, 0, 1]).tolist() == [2, 0, 1]


# ---- pseudo_group_table and the schedule -----------------------------------------------------------------------------------------------
def test_pseudo_group_table_shares_storage_and_recodes_groups():
    rs = np.random.RandomState(0)
    y, conf = rs.randint(0, 2, 50), rs.randint(0, 2, 50)
    table = trainer.EmbeddingTable(rs.standard_normal((50, 8)).astype(np.float32), y, conf, device="cpu")
    clusters = rs.randint(0, 2, 50)
    pseudo = analysis.pseudo_group_table(table, clusters)
    assert pseudo.embeddings.data_ptr() == table.embeddings.data_ptr()
    assert torch.equal(pseudo.targets, table.targets)
    assert pseudo.targets_group.tolist() == (2 * y + clusters).tolist() and pseudo.group_array.tolist() == (2 * y + clusters).tolist()
    assert pseudo.targets_spurious.tolist() == clusters.tolist()
    assert (pseudo.n_classes, pseudo.n_groups, pseudo.n_places) == (2, 4, 2)
    assert pseudo.group_counts.tolist() == np.bincount(2 * y + clusters, minlength=4).tolist()
    assert table.targets_group.tolist() == (2 * y + conf).tolist()                        # the source table is left alone
    for bad in (np.where(clusters == 1, 2, clusters), np.where(clusters == 0, -1, clusters), clusters[:-1]):
        with pytest.raises(ValueError):
            analysis.pseudo_group_table(table, bad)


def test_schedule_trains_on_pseudo_groups_and_validates_on_true_ones(tmp_path, monkeypatch):
    """opt.robust on a pseudo-group table: every training step of train_all_epochs gets the pseudo group ids of its rows, and the
    counters of the validation passes are filled from the true group ids of val and test"""
    steps = []
    _stand_ins(monkeypatch, steps)
    seen = {"train": [], "eval": []}

    def fake_step(self, features, labels, optimizer, use_group=False, robust=None, contrastive=None):
        state, groups = robust
        seen["train"].append(groups.clone())
        return torch.full((), 2.0), torch.nn.functional.one_hot(labels, 2).float(), torch.zeros(labels.shape[0])
    counts = adapter.group_counts                                                         # (the stand-in: a bincount of the group ids)

    def spy_counts(logits, y, g_, n_groups, counts_=None):
        if not torch.is_grad_enabled():                                                   # an evaluation pass
            seen["eval"].append(g_.clone())
        return counts(logits, y, g_, n_groups, counts_)
    monkeypatch.setattr(adapter.CustomCLIP, "train_step", fake_step)
    monkeypatch.setattr(adapter, "group_counts", spy_counts)
    opt, (train, val, test) = _setup(tmp_path, tl_method="adapter", robust=True)
    clusters = 1 - train.targets_spurious.numpy()                                         # pseudo ids that differ from the true ones everywhere
    pseudo = analysis.pseudo_group_table(train, clusters)
    want = 2 * train.targets.numpy() + clusters
    optim.set_seed(opt.random_seed)
    log = []
    trainer.train_all_epochs(opt, pseudo, val, test, log=log)
    trains = [e for e in log if e["kind"] == "train1"]
    assert len(trains) == opt.epochs and seen["train"]
    batches = [len(b) for b in seen["train"]]
    assert sum(batches) == opt.epochs * len(train)
    at = 0
    for e in trains:                                                                      # the records carry each epoch's row order
        for row0 in range(0, len(train), opt.batch_size):
            rows = e["order"][row0:row0 + opt.batch_size]
            assert seen["train"][at].tolist() == want[rows].tolist()
            at += 1
        assert e["counts"][:, 0].tolist() == np.bincount(want, minlength=4).tolist()      # the train counters are per PSEUDO group
        assert len(e["q"]) == 1
    evals = torch.cat(seen["eval"]).numpy()
    per_epoch = np.concatenate([val.group_array, test.group_array])
    assert evals[:opt.epochs * len(per_epoch)].tolist() == np.tile(per_epoch, opt.epochs).tolist()
    vals = [e for e in log if e["kind"] == "validate"]
    assert [e["counts"][:, 0].tolist() for e in vals if e["split"] == "val"] == [np.bincount(val.group_array, minlength=4).tolist()] * opt.epochs
    assert [e["counts"][:, 0].tolist() for e in vals if e["split"] == "test"] == [np.bincount(test.group_array, minlength=4).tolist()] * opt.epochs
