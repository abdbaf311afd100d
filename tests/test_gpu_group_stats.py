"""Group-wise embedding statistics on the MI355X: the fused pairwise-distance kernel against float64 torch.cdist, and the analysis
module against the values the reference's own code recorded in tests/golden/group_stats.npz.

The 1e-4 relative bound.  The operands are split into 22 bits under a common scale, so a squared distance is off by about
2^-22 * 3 = 7e-7 of the centred squared norms of its two rows.  The fixture generator asserts (and test_group_stats_host re-checks)
that every off-diagonal squared distance exceeds 1 % of the mean centred squared norm; the random rows of the shape tests are
further apart still (d^2 ~ 2 |x|^2).  A distance is then within 7e-7 / 0.01 / 2 < 4e-5 relative, and a sum of distances cannot be
worse than its worst term.  Every test prints its figures before it asserts."""
import json
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from pairdist_cases import rows
from test_group_stats_host import SPLITS, regenerate

pytestmark = pytest.mark.gpu

RTOL = 1e-4


@pytest.fixture(scope="module")
def fx(golden):
    return golden("group_stats.npz")


def bucket_sums_f64(x, groups, G, chunk=1024):
    """S [G, G] from float64 distances, in row chunks: (S, number of pairs per bucket).  The chunks are small because cdist's direct
    (non-matmul) kernel launches one block per pair: chunk * N must stay under 2^24 blocks of 256 threads, the 2^32-thread limit of a
    launch (4096 x 4099 is past it and does not compute the distances)."""
    xd = x.double()
    n = xd.shape[0]
    onehot = (groups.unsqueeze(0) == torch.arange(G, device=x.device).unsqueeze(1)).double()      # [G, N]
    T = torch.zeros(G, G, dtype=torch.float64, device=x.device)
    col = torch.arange(n, device=x.device)
    for i in range(0, n, chunk):
        d = torch.cdist(xd[i:i + chunk], xd, compute_mode="donot_use_mm_for_euclid_dist")
        d = d * (col.unsqueeze(0) > torch.arange(i, min(i + chunk, n), device=x.device).unsqueeze(1))
        T += onehot[:, i:i + chunk] @ d @ onehot.T
    cnt = onehot.sum(1)
    pairs = torch.outer(cnt, cnt)
    pairs[torch.arange(G), torch.arange(G)] = cnt * (cnt - 1) / 2
    return T + T.T - torch.diag(torch.diag(T)), pairs


def check_buckets(S, ref, pairs, what):
    total = torch.triu(ref).sum()
    err = (S - ref).abs()
    # a bucket of fewer than 1000 pairs is "near-empty": measured against the whole sum
    tol = torch.where(pairs >= 1000, RTOL * ref, RTOL * total)
    worst = (err / ref.clamp_min(1e-300)).where(pairs >= 1000, torch.zeros_like(err)).max().item()
    print(f"{what}: worst bucket rel err {worst:.3e}, whole-sum rel err "
          f"{(torch.triu(S).sum() - total).abs().item() / max(total.item(), 1e-300):.3e}, max abs err / total {err.max().item() / max(total.item(), 1e-300):.3e}")
    assert torch.equal(S, S.T), f"{what}: S is not symmetric"
    assert (err <= tol).all(), f"{what}: bucket sums off by more than {RTOL}"
    assert (S[pairs == 0] == 0).all(), f"{what}: an empty bucket is not zero"


def layouts(n, seed):
    g = torch.Generator().manual_seed(seed)
    r = torch.randint(0, 3, (n,), generator=g)
    empty = torch.tensor([0, 1, 3])[r]                                  # group 2 has no rows
    one = r.clone()
    one[n // 2] = 3                                                     # group 3 has one row
    return {"empty_group": empty, "one_row_group": one, "single_group": torch.ones(n, dtype=torch.int64)}


# ---- fixture parity: the reference's recorded values ----------------------------------------------------------------------------

def test_group_stats_match_reference(fx):
    from dbmm_amd import analysis
    for split in SPLITS:
        x, g, _ = regenerate(fx, split)
        st = analysis.group_stats(x.cuda(), g.numpy())
        keys = ["full"] + [int(k) for k in fx[f"{split}/groups"]]
        for name in ("mean_vector", "mean_vector_norm", "pairwise_distance"):
            assert [k if k == "full" else int(k) for k in st[name]] == keys
        pd_ = np.array([st["pairwise_distance"][k] for k in st["pairwise_distance"]])
        nm = np.array([st["mean_vector_norm"][k] for k in st["mean_vector_norm"]], dtype=np.float64)
        mv = np.stack([st["mean_vector"][k][::int(fx["sample_stride"])] for k in st["mean_vector"]])
        e_pd = np.abs(pd_ / fx[f"{split}/pairwise_distance"] - 1).max()
        e_nm = np.abs(nm / fx[f"{split}/mean_vector_norm"] - 1).max()
        e_mv = np.abs(mv - fx[f"{split}/mean_vector_samples"]).max()
        print(f"{split}: pairwise_distance rel err {e_pd:.3e}, mean_vector_norm rel err {e_nm:.3e}, mean_vector abs err {e_mv:.3e}")
        assert e_pd <= RTOL and e_nm <= RTOL and e_mv <= 1e-5
        assert isinstance(st["mean_vector"]["full"], np.ndarray) and st["mean_vector"]["full"].shape == (int(fx["dim"]),)
        G = len(keys) - 1
        assert st["between_distance"].shape == (G, G) and np.array_equal(st["between_distance"], st["between_distance"].T)
        assert np.array_equal(np.diag(st["between_distance"]), pd_[1:])
        # the tables, equal after rounding
        df = analysis.representation_table(st, dict(zip([str(k) for k in fx["acc_keys"]], fx[f"{split}/zs_acc"])))
        assert np.array_equal(df.to_numpy(dtype=np.float64), fx[f"{split}/table"])
        assert list(df.index) == [str(s) for s in fx[f"{split}/table_index"]] and list(df.columns) == [str(s) for s in fx[f"{split}/table_columns"]]
        nd = analysis.group_stats(x.cuda(), g.numpy(), return_dist=False)
        assert nd["pairwise_distance"] == {} and "between_distance" not in nd
        assert np.array_equal(nd["mean_vector"]["full"], st["mean_vector"]["full"])


def test_conf_stats_and_closest_samples_match_reference(fx):
    from dbmm_amd import analysis
    anchor = synth_anchor(fx)
    for split in SPLITS:
        x, g, conf = regenerate(fx, split)
        cs = analysis.group_conf_stats(conf.cuda(), g.numpy())
        assert [k if k == "full" else int(k) for k in cs] == ["full"] + [int(k) for k in fx[f"{split}/groups"]]
        assert np.abs(np.array(list(cs.values()), dtype=np.float64) - fx[f"{split}/conf"]).max() <= 1e-6
        idx = analysis.closest_samples(x.cuda(), anchor, top_k=int(fx["top_k"]))
        assert idx.tolist() == fx[f"{split}/closest"].tolist()


def synth_anchor(fx):
    from dbmm_amd import synth
    return synth.embedding_text(int(fx["seed"]), int(fx["dim"]))[0][:, 1].contiguous()


# ---- the kernel against float64 cdist -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("d", [512, 640, 768, 1024])
@pytest.mark.parametrize("n", [1, 2, 255, 256, 257, 1000, 4099])
def test_shapes_and_group_layouts(n, d):
    from dbmm_amd import ops
    x = rows(n, d, 1000 * n + d)
    center = x.mean(0)
    for name, g in layouts(n, n + d).items():
        g = g.cuda()
        S = ops.pairdist_group_sums(x, g, 4, center)
        ref, pairs = bucket_sums_f64(x, g, 4)
        check_buckets(S, ref, pairs, f"N={n} D={d} {name}")


def test_one_row_group_is_nan_like_the_reference():
    from dbmm_amd import analysis
    x = rows(10, 512, 5)
    g = np.array([0, 0, 0, 1, 0, 2, 2, 0, 2, 0])
    st = analysis.group_stats(x, g)
    assert np.isnan(st["pairwise_distance"][1]) and np.isfinite(st["pairwise_distance"][0]) and np.isfinite(st["pairwise_distance"]["full"])
    assert list(st["pairwise_distance"]) == ["full", 0, 1, 2]


def test_translation_by_fifty_spreads():
    """the same rows plus a constant vector 50 x their spread: the bound holds because the centre is subtracted first (the planes
    then hold the same values; uncentred, 22 bits of a coordinate ~ 50 spreads leave 1e-5 of the spread per coordinate and
    |a|^2 + |b|^2 - 2 a.b cancels 5000 to 1)"""
    from dbmm_amd import ops
    n, d = 3000, 1024
    x = rows(n, d, 77)
    g = torch.randint(0, 4, (n,), generator=torch.Generator().manual_seed(3)).cuda()
    shifted = (x + 50 * 0.5 * torch.ones(d, device="cuda")).contiguous()
    S = ops.pairdist_group_sums(shifted, g, 4, shifted.mean(0))
    ref, pairs = bucket_sums_f64(shifted, g, 4)
    check_buckets(S, ref, pairs, "translated")


def test_duplicated_rows():
    """1 % duplicated rows: an exact-zero pair comes out as sqrt of the accumulation's rounding, at most ~1e-3 of a centred norm, on
    1e-4 of the pairs -- the whole sum stays within the bound"""
    from dbmm_amd import ops
    n, d = 4000, 1024
    x = rows(n, d, 78)
    x[n - 40:] = x[:40]
    g = torch.randint(0, 4, (n,), generator=torch.Generator().manual_seed(4)).cuda()
    S = ops.pairdist_group_sums(x, g, 4, x.mean(0))
    ref, _ = bucket_sums_f64(x, g, 4)
    tot, want = torch.triu(S).sum().item(), torch.triu(ref).sum().item()
    print(f"duplicates: whole-sum rel err {abs(tot - want) / want:.3e}")
    assert abs(tot - want) <= RTOL * want
    assert torch.isfinite(S).all()


def test_deterministic_and_order_independent():
    from dbmm_amd import ops
    n, d = 5000, 768
    x = rows(n, d, 79)
    g = torch.randint(0, 4, (n,), generator=torch.Generator().manual_seed(5)).cuda()
    c = x.mean(0)
    S1 = ops.pairdist_group_sums(x, g, 4, c)
    S2 = ops.pairdist_group_sums(x, g, 4, c)
    assert torch.equal(S1, S2), "two calls on the same input differ"
    order = torch.argsort(g, stable=True)
    S3 = ops.pairdist_group_sums(ops.gather_rows(x, order), g[order].contiguous(), 4, c)
    rel = ((S3 - S1).abs() / S1).max().item()
    print(f"sorted vs unsorted: max bucket rel diff {rel:.3e}")
    assert rel <= 1e-6


def test_scale_without_an_n_by_n_buffer():
    from dbmm_amd import analysis
    n, d = 40000, 1024
    x = rows(n, d, 80)
    g = torch.randint(0, 4, (n,), generator=torch.Generator().manual_seed(6))
    g[g == 3] = torch.where(torch.rand(int((g == 3).sum()), generator=torch.Generator().manual_seed(7)) < 0.1, 3, 0)   # a small group
    inputs = x.numel() * 4 + n * 8
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    st = analysis.group_stats(x, g.numpy())
    torch.cuda.synchronize()
    extra = torch.cuda.max_memory_allocated() - base
    print(f"N={n}: peak extra memory {extra / 2**20:.1f} MB for {inputs / 2**20:.1f} MB of inputs (N x N fp32 would be {n * n * 4 / 2**20:.0f} MB)")
    assert extra < 3 * inputs + (64 << 20)
    # float64 reference in row chunks, on centred rows (the Gram form in float64: 1e-16 of the norms)
    gd = g.cuda()
    xd = (x.double() - x.double().mean(0))
    onehot = (gd.unsqueeze(0) == torch.arange(4, device="cuda").unsqueeze(1)).double()
    T = torch.zeros(4, 4, dtype=torch.float64, device="cuda")
    for i in range(0, n, 2000):
        T += onehot[:, i:i + 2000] @ torch.cdist(xd[i:i + 2000], xd) @ onehot.T                     # ordered pairs, zero diagonal
    cnt = onehot.sum(1)
    want = [T.sum().item() / (n * (n - 1.0))] + [(T[k, k] / (cnt[k] * (cnt[k] - 1))).item() for k in range(4)]
    got = [st["pairwise_distance"][k] for k in ("full", 0, 1, 2, 3)]
    rel = max(abs(a / b - 1) for a, b in zip(got, want))
    print(f"N={n}: pairwise_distance rel err {rel:.3e}")
    assert rel <= RTOL
    btw = (T / torch.outer(cnt, cnt)).cpu().numpy()
    off = ~np.eye(4, dtype=bool)
    assert np.abs(st["between_distance"][off] / btw[off] - 1).max() <= RTOL


# ---- the report ---------------------------------------------------------------------------------------------------------------

def r3(values):
    return np.round(np.array(values, dtype=np.float64), 3).tolist()


def test_representation_report_with_adapter_transform(tmp_path):
    from dbmm_amd import adapter, analysis, synth, trainer
    D, H, seed = 512, 128, 21
    tables = []
    for split, n in (("train", 900), ("val", 500), ("test", 600)):
        x, y, c = synth.embedding_dataset(seed, split, n, D)
        tables.append(trainer.EmbeddingTable(x, y.numpy(), c.numpy()))
    paths = []
    for nm, m in zip(("class", "spurious", "group"), synth.embedding_text(seed, D)):
        p = str(tmp_path / (nm + ".json"))
        json.dump({f"{nm}{i}": m[:, i].tolist() for i in range(m.shape[1])}, open(p, "w"))
        paths.append(p)
    ad = adapter.Adapter(D, H)
    ad.load_state_dict(synth.adapter_state_dict(3, D, H))
    clf = adapter.CustomCLIP(ad, *paths, temperature=0.01).cuda().eval()
    opt = SimpleNamespace(batch_size=256, tl_method="adapter", text_embedding_dir=paths[0], zs_temperature=0.01)
    frames, stats = analysis.representation_report(opt, *tables, classifier=clf, transform=clf.adapter)
    ratio = tables[0].group_ratio.numpy()
    assert len(frames) == 3 and list(stats) == ["train", "val", "test"]
    for df, table, split in zip(frames, tables, stats):
        acc = trainer.validate(table, clf, 4096, ratio)[2]
        assert list(df.index) == ["Acc.", "Div.", "Centr. Norm."] and list(df.columns) == ["Avg.", "Worst", "group0", "group1", "group2", "group3"]
        assert df.loc["Acc."].tolist() == r3(list(acc.values())[:-1])
        with torch.no_grad():
            z = clf.adapter(table.embeddings)
        want = analysis.group_stats(z, table.targets_group)
        assert want["pairwise_distance"] == stats[split]["pairwise_distance"]          # the statistics are of the TRANSFORMED rows
        assert df.loc["Div."].tolist() == r3([want["pairwise_distance"]["full"], 0.0] + [want["pairwise_distance"][k] for k in range(4)])
        raw = analysis.group_stats(table)
        assert raw["pairwise_distance"]["full"] != want["pairwise_distance"]["full"]
    # without a classifier: the zero-shot baseline of the raw embeddings
    frames0, _ = analysis.representation_report(opt, *tables)
    for df, table in zip(frames0, tables):
        acc = trainer.validate_zs_linear_probing(table, paths[0], 0.01, 4096, ratio)[2]
        assert df.loc["Acc."].tolist() == r3(list(acc.values())[:-1])
