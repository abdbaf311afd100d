"""Silhouettes on the MI355X: the per-row, per-group distance-sum kernel against float64, against its sibling and against itself,
and analysis.silhouette / kmeans_select_k / separation_report against the float64 restatement of test_silhouette_host.

RTOL = 1e-4 is the bound tests/test_gpu_group_stats.py derives for this split and this arithmetic: 22-bit operands under a common
scale put a squared distance off by about 7e-7 of the centred squared norms of its rows; where every squared distance exceeds 1 % of
the mean centred squared norm (the random rows here are further apart still, d^2 ~ 2 |x|^2; test_silhouette_host asserts it for the
planted rows) a distance is within 4e-5 relative, and a sum of distances is no worse than its worst term.  The fp32 tree over a
wave's 64 columns adds at most 6 * 2^-24 = 4e-7.  With s = 1 - a / b (or b / a - 1) and a relative error e on each of a and b, s is
off by at most 2 e: the silhouettes are compared at 2 RTOL absolute.  Every test prints its figures before it asserts."""
import numpy as np
import pytest
import torch

from pairdist_cases import GuardedAlloc, onehot, rows
from test_silhouette_host import planted_rows, silhouette_f64

pytestmark = pytest.mark.gpu

RTOL = 1e-4


def distances_f64(x, chunk=1024):
    """the N x N float64 distance matrix from direct differences (small N only), its diagonal exactly 0.  cdist's direct kernel
    launches one block per pair: chunk * N stays under 2^24 blocks."""
    xd = x.double()
    return torch.cat([torch.cdist(xd[i:i + chunk], xd, compute_mode="donot_use_mm_for_euclid_dist") for i in range(0, xd.shape[0], chunk)])


def check_sums(R, ref, g, G, what):
    cnt = onehot(g, G).sum(0)
    own = (g.unsqueeze(1) == torch.arange(G, device=g.device).unsqueeze(0))
    alone = own & (cnt == 1).unsqueeze(0)                                                             # a singleton's own entry
    live = (cnt > 0).unsqueeze(0) & ~alone
    rel = ((R - ref).abs() / ref.clamp_min(1e-300)).where(live & (ref > 0), torch.zeros_like(R))
    print(f"{what}: worst entry rel err {rel.max().item():.3e} over {int(live.sum())} entries, counts {cnt.long().tolist()}")
    assert R.shape == ref.shape and R.dtype == torch.float64
    assert torch.isfinite(R).all()
    assert (rel <= RTOL).all(), f"{what}: an entry is off by more than {RTOL}"
    assert (R[:, cnt == 0] == 0).all(), f"{what}: an empty group's column is not exactly 0"
    assert (R[alone] == 0).all(), f"{what}: a singleton's own entry is not exactly 0"


def layouts(n, seed, G=4):
    gen = torch.Generator().manual_seed(seed)
    r = torch.randint(0, G, (n,), generator=gen)
    three = torch.randint(0, 3, (n,), generator=gen)
    one = three.clone()
    one[n // 2] = 3                                                     # group 3 has one row
    outside = r.clone()
    outside[::5] = torch.tensor([-1, G, 7, 255, -(1 << 40)])[torch.arange(len(outside[::5])) % 5]      # in no group; their rows still get sums
    return {"sorted": torch.sort(r).values, "shuffled": r, "empty_group": torch.tensor([0, 1, 3])[three], "one_row_group": one,
            "single_group": torch.ones(n, dtype=torch.int64), "labels_outside": outside}


# ---- the kernel against float64 ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("d", [64, 192, 1024])
@pytest.mark.parametrize("n", [2, 255, 256, 257, 513, 1000, 4099])
def test_shapes_and_label_layouts(n, d):
    """one tile, ragged tiles, the diagonal block next to a ragged one, several column chunks, D padded to 128"""
    from dbmm_amd import ops
    x = rows(n, d, 1000 * n + d)
    center = x.mean(0)
    dist = distances_f64(x)
    for name, g in layouts(n, n + d).items():
        g = g.cuda()
        R = ops.pairdist_row_group_sums(x, g, 4, center)
        check_sums(R, dist @ onehot(g, 4), g, 4, f"N={n} D={d} {name}")


def test_sixteen_labels():
    from dbmm_amd import ops
    n, d = 1000, 192
    x = rows(n, d, 11)
    dist = distances_f64(x)
    for name, g in (("shuffled", torch.randint(0, 16, (n,), generator=torch.Generator().manual_seed(12))),
                    ("sorted", torch.sort(torch.randint(0, 16, (n,), generator=torch.Generator().manual_seed(13))).values),
                    ("label 15 and outside", torch.tensor([15, 16, 3, -1])[torch.arange(n) % 4])):
        g = g.cuda()
        R = ops.pairdist_row_group_sums(x, g, 16, x.mean(0))
        check_sums(R, dist @ onehot(g, 16), g, 16, f"G=16 {name}")


def test_agrees_with_the_bucket_kernel():
    """the same planes, the same fp32 distances, another order of summation: sum over the rows of group a of R[i, b] is S[a, b], and
    twice S[a, a] on the diagonal (every unordered pair is seen from both ends)"""
    from dbmm_amd import ops
    n, d = 1000, 192
    x = rows(n, d, 21)
    c = x.mean(0)
    r = torch.randint(0, 4, (n,), generator=torch.Generator().manual_seed(22))
    for name, g in (("shuffled", r), ("sorted", torch.sort(r).values)):
        g = g.cuda()
        S = ops.pairdist_group_sums(x, g, 4, c)
        T = onehot(g, 4).T @ ops.pairdist_row_group_sums(x, g, 4, c)
        want = S + torch.diag(torch.diag(S))
        rel = ((T - want).abs() / want).max().item()
        print(f"rows kernel against bucket kernel, {name}: max rel diff {rel:.3e}")
        assert rel <= 1e-6


def test_deterministic_and_order_independent():
    from dbmm_amd import ops
    n, d = 3000, 192
    x = rows(n, d, 23)
    g = torch.randint(0, 4, (n,), generator=torch.Generator().manual_seed(24)).cuda()
    c = x.mean(0)
    R1 = ops.pairdist_row_group_sums(x, g, 4, c)
    R2 = ops.pairdist_row_group_sums(x, g, 4, c)
    assert torch.equal(R1, R2), "two calls on the same input differ"
    order = torch.argsort(g, stable=True)
    R3 = torch.empty_like(R1)
    R3[order] = ops.pairdist_row_group_sums(ops.gather_rows(x, order), g[order].contiguous(), 4, c)
    rel = ((R3 - R1).abs() / R1).max().item()
    print(f"sorted vs unsorted: max entry rel diff {rel:.3e}")
    assert rel <= 1e-6


def test_nothing_is_written_outside_the_sums_and_the_workspace(monkeypatch):
    from dbmm_amd import ops
    n, d = 257, 64
    x = rows(n, d, 25)
    g = torch.randint(0, 3, (n,), generator=torch.Generator().manual_seed(26)).cuda()
    c = x.mean(0)
    dist = distances_f64(x)
    ga = GuardedAlloc()
    monkeypatch.setattr(ops, "_empty", ga)
    R = ops.pairdist_row_group_sums(x, g, 3, c)
    torch.cuda.synchronize()
    assert len(ga.bufs) == 2                                                    # workspace, sums
    ga.check()
    check_sums(R, dist @ onehot(g, 3), g, 3, "guarded N=257 G=3")


def test_translation_by_fifty_spreads():
    """the sibling's case: the same rows plus a constant vector 50 x their spread; the centre is subtracted first"""
    from dbmm_amd import ops
    n, d = 2000, 1024
    x = rows(n, d, 77)
    g = torch.randint(0, 4, (n,), generator=torch.Generator().manual_seed(3)).cuda()
    shifted = (x + 50 * 0.5 * torch.ones(d, device="cuda")).contiguous()
    R = ops.pairdist_row_group_sums(shifted, g, 4, shifted.mean(0))
    check_sums(R, distances_f64(shifted) @ onehot(g, 4), g, 4, "translated")


def _silhouette_of_sums(R, g, G):
    from dbmm_amd import analysis
    dense = g.cpu().numpy()
    return analysis.silhouette_from_sums(R.cpu().numpy(), dense, np.bincount(dense, minlength=G))


def test_duplicated_rows():
    """1 % duplicated rows: an exact-zero pair comes out as sqrt of the accumulation's rounding, at most ~1e-3 of a centred norm, on
    1e-4 of the pairs -- nothing is nan (the clamp), and the score stays within the bound"""
    from dbmm_amd import ops
    n, d = 3000, 1024
    x = rows(n, d, 78)
    x[n - 30:] = x[:30]
    g = torch.randint(0, 4, (n,), generator=torch.Generator().manual_seed(4)).cuda()
    R = ops.pairdist_row_group_sums(x, g, 4, x.mean(0))
    assert torch.isfinite(R).all() and (R >= 0).all()
    got, want = _silhouette_of_sums(R, g, 4), _silhouette_of_sums(distances_f64(x) @ onehot(g, 4), g, 4)
    err = abs(got["samples"].mean() - want["samples"].mean())
    print(f"duplicates: score {got['samples'].mean():.6f}, abs err {err:.3e}, worst row {np.abs(got['samples'] - want['samples']).max():.3e}")
    assert np.isfinite(got["samples"]).all() and np.isfinite(got["a"]).all() and np.isfinite(got["b"]).all()
    assert err <= 2 * RTOL


# ---- analysis.silhouette against the restatement ---------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def planted():
    x, labels = planted_rows()
    return x, labels, silhouette_f64(x, labels)


def check_fit(fit, ref, what):
    e_s = np.abs(fit["samples"] - ref["samples"]).max()
    e_a, e_b = np.abs(fit["a"] / ref["a"] - 1).max(), np.abs(fit["b"] / ref["b"] - 1).max()
    e_l = max(abs(fit["per_label"][k] - ref["per_label"][k]) for k in ref["per_label"])
    print(f"{what}: max |s - ref| {e_s:.3e}, a rel {e_a:.3e}, b rel {e_b:.3e}, per_label {e_l:.3e}, score {fit['score']:.6f} (ref {ref['score']:.6f})")
    assert fit["samples"].dtype == np.float64 and fit["samples"].shape == ref["samples"].shape
    assert e_s <= 2 * RTOL and e_a <= RTOL and e_b <= RTOL
    assert np.array_equal(fit["nearest"], ref["nearest"])
    assert list(fit["per_label"]) == list(ref["per_label"]) and e_l <= 2 * RTOL
    assert abs(fit["score"] - ref["score"]) <= 2 * RTOL
    assert np.array_equal(fit["labels"], ref["labels"]) and np.array_equal(fit["counts"], ref["counts"])


def test_silhouette_matches_the_restatement_in_input_order(planted):
    from dbmm_amd import analysis, trainer
    x, labels, ref = planted
    xd = torch.from_numpy(x).cuda()
    fit = analysis.silhouette(xd, labels)
    check_fit(fit, ref, "tensor")
    assert fit["score"] == fit["samples"].mean()
    table = trainer.EmbeddingTable(torch.from_numpy(x), labels // 2, labels % 2)                      # targets_group = 2 y + c = labels
    fit_t = analysis.silhouette(table)
    check_fit(fit_t, ref, "EmbeddingTable")
    assert np.array_equal(fit_t["samples"], fit["samples"])
    # other labels for the same partition, given explicitly, and a device tensor of labels
    named = analysis.silhouette(table, labels=torch.from_numpy(10 * labels + 3).cuda())
    assert np.array_equal(named["samples"], fit["samples"]) and np.array_equal(named["nearest"], 10 * fit["nearest"] + 3)
    assert list(named["per_label"]) == [3, 13, 23, 33]
    with pytest.raises(ValueError):
        analysis.silhouette(xd, np.zeros(len(labels), dtype=np.int64))
    with pytest.raises(ops_unsupported()):
        analysis.silhouette(xd, np.arange(len(labels)) % 17)


def ops_unsupported():
    from dbmm_amd import ops
    return ops.DbmmUnsupported


def synth_adapter(D, H=128):
    from dbmm_amd import adapter, synth
    ad = adapter.Adapter(D, H)
    ad.load_state_dict(synth.adapter_state_dict(3, D, H))
    return ad.cuda().eval()


def test_silhouette_transform_is_the_silhouette_of_the_transformed_rows(planted):
    from dbmm_amd import analysis
    x, labels, _ = planted
    xd = torch.from_numpy(x).cuda()
    ad = synth_adapter(x.shape[1])
    with torch.no_grad():
        z = ad(xd)
    a, b = analysis.silhouette(xd, labels, transform=ad), analysis.silhouette(z, labels)
    for key in ("samples", "a", "b", "nearest"):
        assert np.array_equal(a[key], b[key]), key
    assert a["score"] == b["score"] and a["per_label"] == b["per_label"]
    assert a["score"] != analysis.silhouette(xd, labels)["score"]
    ref = silhouette_f64(z.double().cpu().numpy(), labels)
    print(f"transformed: score {a['score']:.6f} (ref {ref['score']:.6f}), max |s - ref| {np.abs(a['samples'] - ref['samples']).max():.3e}")
    assert np.abs(a["samples"] - ref["samples"]).max() <= 2 * RTOL


# ---- choosing k -----------------------------------------------------------------------------------------------------------------

def blobs(n=600, d=64, seed=41):
    """three blobs: 2 sigma^2 d = 64 inside, squared centre distances 256 -- apart enough that k = 3 wins, close enough that every
    squared distance stays above 1 % of the mean centred squared norm (about 32 + 85)"""
    from dbmm_amd import synth
    centres = synth.normal(seed, "blobs/centres", (3, d)).double().numpy()
    q = np.linalg.qr(centres.T)[0].T                                                                  # three orthonormal directions
    which = np.minimum((synth.uniform(seed, "blobs/which", (n,)).numpy().astype(np.float64) * 3).astype(np.int64), 2)
    x = np.sqrt(32.0 / d) * synth.normal(seed, "blobs/noise", (n, d)).double().numpy() + np.sqrt(128.0) * q[which]
    return x.astype(np.float32), which


def test_kmeans_select_k_picks_the_planted_three():
    from dbmm_amd import analysis
    x, which = blobs()
    xd = torch.from_numpy(x).cuda()
    out = analysis.kmeans_select_k(xd, ks=(2, 3, 4, 5), seed=1)
    print("kmeans_select_k scores:", {k: round(v, 5) for k, v in out["scores"].items()})
    assert list(out["scores"]) == [2, 3, 4, 5] and list(out["fits"]) == [2, 3, 4, 5]
    for k, fit in out["fits"].items():
        ref = silhouette_f64(x, fit["labels"].cpu().numpy())
        print(f"k={k}: score {out['scores'][k]:.6f}, restatement {ref['score']:.6f}")
        assert abs(out["scores"][k] - ref["score"]) <= 2 * RTOL
        assert fit["centers"].shape == (k, x.shape[1])
    assert out["k"] == 3 and out["scores"][3] == max(out["scores"].values())
    assert analysis.cluster_agreement(out["fits"][3]["labels"].cpu().numpy(), which)["ari"] == 1.0
    again = analysis.kmeans_select_k(xd, ks=(2, 3, 4, 5), seed=1)
    assert again["k"] == out["k"] and again["scores"] == out["scores"]
    with pytest.raises(ValueError):
        analysis.kmeans_select_k(xd, ks=(1, 2))


# ---- the report -------------------------------------------------------------------------------------------------------------------

def test_separation_report_with_adapter_transform():
    from dbmm_amd import analysis, ops, synth, trainer
    D, seed = 512, 21
    tables = []
    for split, n in (("train", 900), ("val", 500), ("test", 600)):
        x, y, c = synth.embedding_dataset(seed, split, n, D)
        tables.append(trainer.EmbeddingTable(x, y.numpy(), c.numpy()))
    ad = synth_adapter(D)
    raw, after = analysis.separation_report(*tables), analysis.separation_report(*tables, transform=ad)
    for rep, transform in ((raw, None), (after, ad)):
        assert list(rep) == ["train", "val", "test"]
        for split, table in zip(rep, tables):
            r = rep[split]
            assert sorted(r) == ["group", "spurious_within_class"] and sorted(r["group"]) == ["per_label", "score"]
            want = analysis.silhouette(table, transform=transform)
            assert r["group"]["score"] == want["score"] and r["group"]["per_label"] == want["per_label"]
            assert list(r["group"]["per_label"]) == [0, 1, 2, 3] and list(r["spurious_within_class"]) == [0, 1]
            y, c = table.targets.cpu().numpy(), table.targets_spurious.cpu().numpy()
            x = table.embeddings
            if transform is not None:
                with torch.no_grad():
                    x = transform(x)
            for cls in (0, 1):
                idx = torch.from_numpy(np.flatnonzero(y == cls)).cuda()
                direct = analysis.silhouette(ops.gather_rows(x.float().contiguous(), idx), c[y == cls])["score"]
                assert r["spurious_within_class"][cls] == direct and -1.0 <= direct <= 1.0
    for split in raw:
        assert raw[split]["group"]["score"] != after[split]["group"]["score"]
        assert raw[split]["spurious_within_class"] != after[split]["spurious_within_class"]
    print("separation, raw:", {s: (round(r["group"]["score"], 5), {k: round(v, 5) for k, v in r["spurious_within_class"].items()}) for s, r in raw.items()})
    print("separation, adapter:", {s: (round(r["group"]["score"], 5), {k: round(v, 5) for k, v in r["spurious_within_class"].items()}) for s, r in after.items()})
    # a class with one place only: nan, nothing raised
    x, y, c = synth.embedding_dataset(seed, "train", 300, D)
    c = torch.where(y == 1, torch.ones_like(c), c)
    one_place = trainer.EmbeddingTable(x, y.numpy(), c.numpy())
    rep = analysis.separation_report(one_place, one_place, one_place)
    assert np.isnan(rep["train"]["spurious_within_class"][1]) and np.isfinite(rep["train"]["spurious_within_class"][0])


# ---- memory -----------------------------------------------------------------------------------------------------------------------

def test_scale_without_an_n_by_n_buffer():
    from dbmm_amd import analysis
    n, d = 40000, 1024
    x = rows(n, d, 80)
    g = torch.randint(0, 4, (n,), generator=torch.Generator().manual_seed(6))
    inputs = x.numel() * 4 + n * 8
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fit = analysis.silhouette(x, g.numpy())
    torch.cuda.synchronize()
    extra = torch.cuda.max_memory_allocated() - base
    print(f"N={n}: peak extra memory {extra / 2**20:.1f} MB for {inputs / 2**20:.1f} MB of inputs (N x N fp32 would be {n * n * 4 / 2**20:.0f} MB)")
    assert extra < 3 * inputs + (64 << 20)
    # float64 reference in row chunks, on centred rows (the Gram form in float64: 1e-16 of the norms)
    gd = g.cuda()
    xd = x.double() - x.double().mean(0)
    oh = onehot(gd, 4)
    R = torch.cat([torch.cdist(xd[i:i + 2000], xd) @ oh for i in range(0, n, 2000)]).cpu().numpy()      # the zero diagonal adds nothing
    dense, cnt = g.numpy(), np.bincount(g.numpy(), minlength=4).astype(np.float64)
    idx = np.arange(n)
    a = R[idx, dense] / (cnt[dense] - 1)
    M = R / cnt[None, :]
    M[idx, dense] = np.inf
    b = M.min(1)
    want = ((b - a) / np.maximum(a, b)).mean()
    print(f"N={n}: score {fit['score']:.3e}, reference {want:.3e}, abs err {abs(fit['score'] - want):.3e}")
    assert abs(fit["score"] - want) <= 2 * RTOL
