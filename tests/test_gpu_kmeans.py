"""k-means pseudo-groups on the MI355X: the assign / sums / merge kernels behind ops.kmeans_fit and ops.kmeans_assign against the
float64 restatement of tests/test_kmeans_host.py (its trajectory where every row is decided, otherwise the fixed point the device
reached), ragged and edge shapes, determinism, and the analysis layer up to group DRO on pseudo-groups."""
import numpy as np
import pytest
import torch

from dbmm_amd import analysis, ops, optim, trainer
from test_gpu_group_dro import _same_records, _schedule_opt, schedule_data  # noqa: F401  (schedule_data: a fixture)
from test_gpu_supcon import _Guarded
from test_kmeans_host import TRAJECTORY_CASES, distances64, kmeans_pp_restated, planted, restatement, undecided

pytestmark = pytest.mark.gpu


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _fit(x, init, **kw):
    centers, labels, info = ops.kmeans_fit(_dev(x), _dev(init), **kw)
    return centers.cpu().numpy(), labels.cpu().numpy(), info


@pytest.fixture(scope="module")
def case():
    """planted(...) and the restatement's k-means++ start of a case, computed once"""
    cache = {}

    def get(N, D, K, sep, seed=0):
        key = (N, D, K, sep, seed)
        if key not in cache:
            x, lab = planted(*key)
            cache[key] = (x, lab, x[kmeans_pp_restated(x, K, seed)].copy())
        return cache[key]
    return get


def _check_fixed_point(x, centers, labels, info):
    """the device's own result against float64, no trajectory followed"""
    N, D = x.shape
    K = centers.shape[0]
    d2 = distances64(x, centers)
    mask, gap = undecided(d2, D)
    ref_inertia = d2[np.arange(N), labels].sum()
    print(f"N={N} D={D} K={K}: {info['iterations']} iterations, undecided {int(mask.sum())}, smallest gap {gap:.3e}, inertia rel err "
          f"{abs(info['inertia'] - ref_inertia) / max(ref_inertia, 1e-300):.3e} (allowed {(D + 8) * 2.0 ** -24:.3e})")
    assert np.isfinite(centers).all() and labels.min() >= 0 and labels.max() < K
    assert mask.sum() <= max(1, N // 1000)
    assert (labels[~mask] == d2.argmin(1)[~mask]).all()
    assert info["counts"].tolist() == np.bincount(labels, minlength=K).tolist()
    worst = 0.0
    for j in range(K):
        if info["counts"][j]:
            want = x[labels == j].astype(np.float64).mean(0).astype(np.float32)
            ulps = np.abs(centers[j].astype(np.float64) - want) / np.spacing(np.maximum(np.abs(want), np.abs(centers[j])))
            worst = max(worst, float(ulps.max()))
    print(f"    centres: at most {worst:.2f} ulp from the rounded float64 means")
    assert worst <= 1.0
    assert abs(info["inertia"] - ref_inertia) <= (D + 8) * 2.0 ** -24 * ref_inertia
    assert info["converged"]


# ---- 1. the trajectory ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", TRAJECTORY_CASES, ids=["k2", "k16", "k3_d132"])
def test_trajectory_equals_the_restatement(shape, case):
    N, D, K, sep, seed = shape
    x, _, init = case(*shape)
    ref = restatement(x, init)
    assert ref["converged"] and not any(ref["undecided"])                        # the condition under which fp32 distances must agree
    centers, labels, info = _fit(x, init)
    rel = np.abs(centers.astype(np.float64) - ref["centers"]) / np.abs(ref["centers"].astype(np.float64))
    print(shape, "iterations", info["iterations"], "restatement", ref["iterations"], "centres rel err", rel.max(), "smallest gap", ref["gap"])
    assert info["converged"] and info["iterations"] == ref["iterations"]
    assert (labels == ref["labels"]).all()
    assert info["counts"].tolist() == ref["counts"].tolist()
    assert (rel <= 2.0 ** -23).all()


# ---- 2. the fixed point ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(4099, 1024, 8, 1.0), (2048, 256, 4, 0.7), (5000, 64, 5, 1.0)], ids=["d1024_k8", "d256_k4", "d64_k5"])
def test_fixed_point_against_float64(shape, case):
    x, _, init = case(*shape)
    centers, labels, info = _fit(x, init)
    _check_fixed_point(x, centers, labels, info)


# ---- 3. ragged and edge shapes ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(261, 4, 3, 6.0), (257, 132, 2, 6.0), (67, 4096, 3, 6.0), (140001, 8, 3, 6.0), (300, 64, 1, 1.0),
                                   (16, 132, 16, 6.0)],
                         ids=["d4", "n_1_plus_4m_d132", "d4096", "ranges_above_64_rows", "k1", "k_equals_n"])
def test_ragged_and_edge_shapes(shape, case):
    """N = 1 + 4 m (the last wave step holds one row), N no multiple of the row range (257 rows: 5 ranges of 52; 140001 rows at D = 8:
    2048 ranges of 69), D = 4 (one lane), 132 (a ragged column slab), 4096 (16 slabs), K = 1 and K = N"""
    N, D, K, sep = shape
    x, _, init = case(*shape)
    if K == N:
        init = x.copy()                                                          # every row its own centre: the fixed point at once
    centers, labels, info = _fit(x, init)
    _check_fixed_point(x, centers, labels, info)
    if K == 1:
        assert info["iterations"] == 2 and (labels == 0).all()
    if K == N:
        assert info["iterations"] == 2 and labels.tolist() == list(range(N)) and info["inertia"] == 0.0 and (centers == x).all()


def test_empty_cluster_keeps_its_centre(case):
    """a far-away start centre wins no row: count 0, the centre unchanged, no NaN"""
    x, _, init = case(257, 64, 2, 6.0)
    far = np.full((1, 64), 1.0e3, dtype=np.float32)
    start = np.concatenate([init[:1], far, init[1:]])
    centers, labels, info = _fit(x, start)
    assert info["converged"] and info["counts"][1] == 0 and (centers[1] == far[0]).all()
    assert set(labels.tolist()) == {0, 2}
    _check_fixed_point(x, centers, labels, info)
    ref = restatement(x, init)
    assert (labels == np.where(ref["labels"] == 1, 2, 0)).all()


def test_exact_tie_goes_to_the_lower_index(case):
    x, _, init = case(257, 64, 2, 6.0)
    rows = np.concatenate([x[:40], x[:40]])                                      # duplicate rows
    labels, dmin = ops.kmeans_assign(_dev(rows), _dev(np.stack([init[1], init[0], init[1], init[0]])))
    labels, dmin = labels.cpu().numpy(), dmin.cpu().numpy()
    assert set(labels.tolist()) == {0, 1}                                        # never the equal centres 2 and 3
    assert (labels[:40] == labels[40:]).all() and (dmin[:40] == dmin[40:]).all()
    own = ops.kmeans_assign(_dev(x[:5]), _dev(x[:5]))                            # a row that is a centre: distance 0 exactly
    assert own[0].tolist() == [0, 1, 2, 3, 4] and (own[1] == 0).all()


def test_guard_zones(case, monkeypatch):
    """labels, dmin and the workspace sit between guard zones"""
    x, _, init = case(257, 132, 2, 6.0)
    xd, cd = _dev(x), _dev(init)
    ga = _Guarded()
    monkeypatch.setattr(ops, "_empty", ga)
    centers, labels, info = ops.kmeans_fit(xd, cd)
    alabels, admin = ops.kmeans_assign(xd, centers)
    torch.cuda.synchronize()
    assert len(ga.bufs) == 3
    ga.check()
    assert info["converged"] and torch.equal(alabels, labels) and torch.isfinite(admin).all()


# ---- 4. determinism and cutting ---------------------------------------------------------------------------------------------------------------
def test_determinism_and_cutting(case):
    x, _, init = case(2048, 256, 4, 0.7)                                         # 23 iterations in the restatement: overlapping clusters
    xd, cd = _dev(x), _dev(init)
    runs = [ops.kmeans_fit(xd, cd, check_every=ce) for ce in (8, 8, 1, 4, 32)]
    c0, l0, i0 = runs[0]
    print("iterations", i0["iterations"], "inertia", i0["inertia"])
    assert i0["converged"] and i0["iterations"] > 8
    for c, l, i in runs[1:]:
        assert torch.equal(c, c0) and torch.equal(l, l0)
        assert i["iterations"] == i0["iterations"] and i["inertia"] == i0["inertia"] and i["counts"].tolist() == i0["counts"].tolist()
    # a slice assigns to the bits of the slice of the assignment; fewer rows than centres are served
    labels, dmin = ops.kmeans_assign(xd, c0)
    ls, ds = ops.kmeans_assign(xd[101:358], c0)
    assert torch.equal(ls, labels[101:358]) and torch.equal(ds, dmin[101:358]) and torch.equal(labels, l0)
    l2, d2 = ops.kmeans_assign(xd[7:9], c0)
    assert torch.equal(l2, labels[7:9]) and torch.equal(d2, dmin[7:9])
    # max_iter reached: reported, not raised
    c, l, i = ops.kmeans_fit(xd, cd, max_iter=3)
    assert i["iterations"] == 3 and not i["converged"] and torch.isfinite(c).all()
    c, l, i = ops.kmeans_fit(xd, cd, max_iter=i0["iterations"])                  # exactly enough
    assert i["converged"] and torch.equal(c, c0)


def test_wrappers_check_their_operands(case):
    x, _, init = case(257, 64, 2, 6.0)
    xd, cd = _dev(x), _dev(init)
    with pytest.raises(RuntimeError):
        ops.kmeans_fit(torch.from_numpy(x), torch.from_numpy(init))              # host tensors
    with pytest.raises(RuntimeError):
        ops.kmeans_fit(xd, cd[:, :32].contiguous())
    with pytest.raises(RuntimeError):
        ops.kmeans_fit(xd[:1], cd)                                               # fewer rows than centres
    with pytest.raises(ops.DbmmUnsupported):
        ops.kmeans_assign(xd, _dev(np.zeros((17, 64), dtype=np.float32)))
    with pytest.raises(ops.DbmmUnsupported):
        ops.kmeans_assign(xd[:, :6].contiguous(), cd[:, :6].contiguous())
    with pytest.raises(ValueError):
        analysis.kmeans(xd, 17)
    with pytest.raises(ValueError):
        analysis.kmeans(xd, 2, init="random")


# ---- 5. the analysis layer ----------------------------------------------------------------------------------------------------------------------
def test_kmeans_pp_rows(case):
    x, _, _ = case(1000, 132, 3, 1.5)
    xd = _dev(x)
    np.random.seed(5)
    before = np.random.get_state()[1].copy()
    a = analysis.kmeans_pp_rows(xd, 8, np.random.RandomState(3))
    b = analysis.kmeans_pp_rows(xd, 8, np.random.RandomState(3))
    c = analysis.kmeans_pp_rows(xd, 8, np.random.RandomState(4))
    fit = analysis.kmeans(xd, 3, seed=3)
    assert (np.random.get_state()[1] == before).all()                            # the global stream is left alone
    assert a.tolist() == b.tolist() and a.tolist() != c.tolist()
    assert len(set(a.tolist())) == 8 and a.min() >= 0 and a.max() < 1000
    assert a[:3].tolist() == analysis.kmeans_pp_rows(xd, 3, np.random.RandomState(3)).tolist()
    again = analysis.kmeans(xd, 3, seed=3)
    assert torch.equal(fit["labels"], again["labels"]) and (fit["centers"] == again["centers"]).all()
    dup = _dev(np.repeat(x[:2], 5, axis=0))                                      # two distinct rows only: the third draw is uniform
    assert len(analysis.kmeans_pp_rows(dup, 3, np.random.RandomState(0))) == 3


def test_restarts_keep_the_lowest_inertia_and_clusters_are_numbered_by_size(case):
    x, _, _ = case(2048, 256, 4, 0.7)
    xd = _dev(x)
    rng = np.random.RandomState(11)
    singles = []
    for _ in range(3):
        rows = analysis.kmeans_pp_rows(xd, 4, rng)
        singles.append(ops.kmeans_fit(xd, xd[torch.from_numpy(rows).cuda()].contiguous())[2]["inertia"])
    fit = analysis.kmeans(xd, 4, seed=11, n_init=3)
    print("restarts", singles, "kept", fit["inertia"])
    assert fit["inertia"] == min(singles) and all(fit["inertia"] <= s for s in singles)
    assert fit["labels"].dtype == torch.int64 and fit["labels"].is_cuda and fit["centers"].dtype == np.float32
    counts = np.bincount(fit["labels"].cpu().numpy(), minlength=4)
    assert counts.tolist() == fit["counts"].tolist() and (np.diff(counts) <= 0).all()
    _check_fixed_point(x, fit["centers"], fit["labels"].cpu().numpy(), dict(fit))
    explicit = analysis.kmeans(xd, 4, init=fit["centers"])                       # an array as the start: already the fixed point
    assert explicit["iterations"] <= 2 and torch.equal(explicit["labels"], fit["labels"])


def test_planted_clusters_are_recovered(case):
    x, lab, _ = case(257, 64, 2, 6.0)
    fit = analysis.kmeans(_dev(x), 2)
    agreement = analysis.cluster_agreement(fit["labels"].cpu().numpy(), lab)
    assert agreement["ari"] == 1.0 and agreement["purity"] == 1.0 and fit["converged"]


def test_pseudo_groups_recover_a_confounder_that_shifts_the_embedding():
    """four planted clusters = (class, confounder): within each class the two clusters are the confounder's two values"""
    x, g = planted(300, 64, 4, 6.0, 1)
    y, conf = g // 2, g % 2
    table = trainer.EmbeddingTable(x, y, conf, device="cuda")
    clusters, fits = analysis.pseudo_groups(table, k=2, seed=0)
    assert clusters.dtype == np.int64 and clusters.shape == (300,) and set(fits) == {0, 1}
    for cls in (0, 1):
        rows = y == cls
        ref = restatement(x[rows], x[rows][kmeans_pp_restated(x[rows], 2, 0)])
        assert analysis.cluster_agreement(ref["labels"], conf[rows])["ari"] == 1.0          # the float64 restatement does ...
        assert analysis.cluster_agreement(clusters[rows], conf[rows])["ari"] == 1.0         # ... and so does the device
        assert fits[cls]["converged"] and fits[cls]["counts"].tolist() == np.bincount(clusters[rows], minlength=2).tolist()
        assert fits[cls]["counts"][0] >= fits[cls]["counts"][1]
    pseudo = analysis.pseudo_group_table(table, clusters)
    assert pseudo.embeddings.data_ptr() == table.embeddings.data_ptr()
    assert torch.equal(pseudo.targets_group.cpu(), torch.from_numpy(2 * y + clusters))


class _Doubling(torch.nn.Module):
    """x -> 2 x in eval mode (exact in fp32), x -> 0 in train mode; records the mode it was called in"""

    def __init__(self):
        super().__init__()
        self.modes = []

    def forward(self, x):
        self.modes.append(self.training)
        return x * (0.0 if self.training else 2.0)


def test_transform_is_applied_in_eval_mode(case):
    x, _, init = case(257, 64, 2, 6.0)
    xd = _dev(x)
    plain = analysis.kmeans(xd, 2, init=init)
    for training in (True, False):
        t = _Doubling().train(training)
        fit = analysis.kmeans(xd, 2, init=2 * init, transform=t)
        assert t.modes and not any(t.modes) and t.training == training          # eval inside, the mode as found afterwards
        assert torch.equal(fit["labels"], plain["labels"]) and (fit["centers"] == 2 * plain["centers"]).all()
        assert fit["inertia"] == 4 * plain["inertia"]


# ---- 6. end to end: group DRO without group labels ------------------------------------------------------------------------------------------
def test_group_dro_on_pseudo_groups_end_to_end(schedule_data):
    paths, (train, val, test) = schedule_data
    clusters, fits = analysis.pseudo_groups(train, k=2)
    assert set(np.unique(clusters).tolist()) == {0, 1} and all(f["converged"] for f in fits.values())
    pseudo = analysis.pseudo_group_table(train, clusters)
    opt = _schedule_opt("adapter", paths, robust=True, robust_step_size=0.05)
    logs = []
    for _ in range(2):
        optim.set_seed(42)
        log = []
        trainer.train_all_epochs(opt, pseudo, val, test, log=log)
        logs.append(log)
    trains = [e for e in logs[0] if e["kind"] == "train1"]
    assert len(trains) == 2 and all(np.isfinite(e["loss"]) and np.isfinite(e["q"][0]).all() for e in trains)
    assert all(np.isfinite(e["loss"]) for e in logs[0] if e["kind"] in ("validate", "validate_zs"))
    assert trains[0]["counts"][:, 0].tolist() == np.bincount(2 * train.targets.cpu().numpy() + clusters, minlength=4).tolist()
    _same_records(logs[0], logs[1])
