"""Linear concept erasure on the MI355X: the kernels behind ops.label_column_sums and ops.erase_rows against float64 with bounds
derived from their own arithmetic, and the analysis layer (erasure_fit, erase, erased_table, balanced_rows) end to end against the
float64 restatement of tests/test_erasure_host.py."""
import json
import os

import numpy as np
import pytest
import torch

from dbmm_amd import _lib, analysis, ops, optim, synth, trainer
from test_erasure_host import apply64, dataset, mean_gap
from test_gpu_group_dro import _schedule_opt, schedule_data  # noqa: F401  (schedule_data: a fixture)
from test_gpu_supcon import _Guarded

pytestmark = pytest.mark.gpu

U32 = 2.0 ** -24                     # the unit roundoff of fp32


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _rows(seed, N, D):
    """fp32 rows far from zero and close to each other, as CLIP rows are"""
    rng = np.random.RandomState(seed)
    return (0.5 * rng.standard_normal((N, D)) + 2.0 * rng.standard_normal((1, D))).astype(np.float32)


# ---- 1. label_column_sums --------------------------------------------------------------------------------------------------------------------
def _check_label_sums(x, labels, G, sums, counts):
    """A label's column is a sum of n_g float64 numbers (fp32 values are exact in float64; adding the +0 of another label's row or
    of a range without the label changes no bit), so at most n_g - 1 additions round, each by 2^-53 of a partial sum that is at
    most sum |x|: the column differs from the exact sum by at most n_g 2^-52 sum |x| (with a factor two of room).  The reference
    is summed in long double."""
    want_counts = np.array([(labels == g).sum() for g in range(G)])
    assert counts.tolist() == want_counts.tolist()
    worst = 0.0
    for g in range(G):
        rows = x[labels == g].astype(np.longdouble)
        want, mag = rows.sum(0), np.abs(rows).sum(0)
        err = np.abs(sums[g].astype(np.longdouble) - want).astype(np.float64)
        allowed = (want_counts[g] * 2.0 ** -52 * mag).astype(np.float64)
        worst = max(worst, float((err / np.maximum(allowed, 1e-300)).max()) if want_counts[g] else 0.0)
        assert (err <= allowed).all(), f"label {g}: error {err.max():.3e}"
        if want_counts[g] == 0:
            assert (sums[g] == 0).all()
    return worst


@pytest.mark.parametrize("D", [64, 512, 1024, 4096])
@pytest.mark.parametrize("N", [1, 3, 63, 64, 65, 1027])
def test_label_column_sums_against_float64(N, D):
    """N around the 64-row range cut (63, 64, 65: one range, one, two), 1027 rows: 17 ranges of 61; D = 64 (16 lanes of one slab), 512,
    1024 (4 slabs), 4096 (16 slabs); G = 1, 2, 16 (the accumulator arrays of 2 and 16); the last label of G >= 2 has no row"""
    x = _rows(N + D, N, D)
    xd = _dev(x)
    for G in (1, 2, 16):
        labels = np.random.RandomState(G).randint(0, max(G - 1, 1), size=N).astype(np.int64)
        sums, counts = ops.label_column_sums(xd, _dev(labels), G)
        assert sums.dtype == torch.float64 and tuple(sums.shape) == (G, D) and counts.dtype == torch.int64 and tuple(counts.shape) == (G,)
        worst = _check_label_sums(x, labels, G, sums.cpu().numpy(), counts.cpu().numpy())
        print(f"N={N} D={D} G={G}: largest error / allowed {worst:.3f}")
        if G >= 2:
            assert counts[G - 1].item() == 0 and (sums[G - 1] == 0).all()                   # the label that no row carries
        again = ops.label_column_sums(xd, _dev(labels), G)
        assert torch.equal(again[0], sums) and torch.equal(again[1], counts)             # the same bits


def test_labels_are_compared_as_64_bit():
    """-1, G, 2^32 (label 0 if it were cut to 32 bits) and 2^32 + 1 (label 1) are in no sum and no count"""
    N, D, G = 1027, 512, 3
    x = _rows(5, N, D)
    labels = np.random.RandomState(6).randint(0, G, size=N).astype(np.int64)
    outside = np.array([-1, G, 2 ** 32, 2 ** 32 + 1, -(2 ** 32), 2 ** 63 - 1], dtype=np.int64)
    where = np.arange(0, N, 7)
    labels[where] = outside[np.arange(len(where)) % len(outside)]
    sums, counts = ops.label_column_sums(_dev(x), _dev(labels), G)
    inside = (labels >= 0) & (labels < G)
    assert counts.sum().item() == inside.sum() < N
    _check_label_sums(x, labels, G, sums.cpu().numpy(), counts.cpu().numpy())
    only = ops.label_column_sums(_dev(x[inside]), _dev(labels[inside]), G)               # the rows inside alone: other ranges, the same sums
    assert torch.equal(only[1], counts)
    _check_label_sums(x[inside], labels[inside], G, only[0].cpu().numpy(), only[1].cpu().numpy())


# ---- 2. erase_rows ---------------------------------------------------------------------------------------------------------------------------
def _erase_case(N, D, R, seed=0):
    rng = np.random.RandomState(1000 * R + seed)
    x = _rows(N + D + R, N, D)
    c = (x.astype(np.float64).mean(0) + 0.01 * rng.standard_normal(D)).astype(np.float32)
    A = (rng.standard_normal((R, D)) / np.sqrt(D)).astype(np.float32)
    B = (rng.standard_normal((R, D)) / np.sqrt(D)).astype(np.float32)
    return x, c, A, B


def erase_bound(x, c, A, B):
    """(float64 result, entrywise bound) of y = x - sum_k ((x - c) . A_k) B_k as the kernel rounds it, operands fp32, u = 2^-24:
      x_j - c_j               one rounding;
      the lane's fmaf chain   L = 4 ceil(D / 256) terms (a lane owns a float4 of every 256 columns), one rounding each;
      the butterfly           6 additions on the path of every term;
      t = sum_k s_k B_kd      R fmaf, one rounding each;
      y = x - t               one rounding, of t's part and of x's.
    A product of n factors (1 + d), |d| <= u, is within gamma_n = n u / (1 - n u) of 1, so with n = 1 + L + 6 + R + 1
      |y_kernel - y| <= gamma_n sum_k (sum_j |x_j - c_j| |A_kj|) |B_kd| + 2^-23 |x_d|
    (2^-23 where one rounding of x's part would give 2^-24: the room the issue leaves)."""
    x64, c64, A64, B64 = (v.astype(np.float64) for v in (x, c, A, B))
    D, R = x.shape[1], A.shape[0]
    n = 1 + 4 * ((D + 255) // 256) + 6 + R + 1
    gamma = n * U32 / (1.0 - n * U32)
    y = x64 - ((x64 - c64) @ A64.T) @ B64
    S = (np.abs(x64 - c64) @ np.abs(A64).T) @ np.abs(B64)
    return y, gamma * S + 2.0 ** -23 * np.abs(x64)


@pytest.mark.parametrize("R", [1, 3, 8, 15])
@pytest.mark.parametrize("D", [64, 512, 1024, 4096])
def test_erase_rows_against_float64(D, R):
    """every N of {1, 3, 5, 257, 1027} per case: one row, a ragged last wave at 4 / 2 / 1 rows per wave, several workgroups; D = 64 (one
    chunk, 16 lanes), 512, 1024 (four rows per wave), 4096 (one row per wave, 16 chunks); R = 1, 3, 8, 15 (padded to 1, 4, 8, 16)"""
    for N in (1, 3, 5, 257, 1027):
        x, c, A, B = _erase_case(N, D, R)
        want, bound = erase_bound(x, c, A, B)
        xd, cd, Ad, Bd = _dev(x), _dev(c), _dev(A), _dev(B)
        y = ops.erase_rows(xd, cd, Ad, Bd)
        err = np.abs(y.cpu().numpy().astype(np.float64) - want)
        print(f"N={N} D={D} R={R}: largest error / bound {(err / bound).max():.3f}, largest |change| {np.abs(want - x).max():.3f}")
        assert (err <= bound).all()
        assert torch.equal(xd, _dev(x))                                                  # the input is left alone
        assert torch.equal(ops.erase_rows(xd, cd, Ad, Bd), y)                            # the same bits
        inplace = xd.clone()
        assert ops.erase_rows(inplace, cd, Ad, Bd, out=inplace) is inplace and torch.equal(inplace, y)
        if N >= 257:                                                                     # a slice that starts inside a wave's rows
            assert torch.equal(ops.erase_rows(xd[101:230], cd, Ad, Bd), y[101:230])
            assert torch.equal(ops.erase_rows(xd[7:8], cd, Ad, Bd), y[7:8])


def test_guard_zones(monkeypatch):
    """the erased rows, the label sums, the counts and the partials' workspace sit between guard zones; so does an in-place target"""
    x, c, A, B = _erase_case(259, 320, 3)                                                # D = 320: a ragged second chunk
    labels = _dev(np.random.RandomState(0).randint(0, 5, size=259).astype(np.int64))
    xd, cd, Ad, Bd = _dev(x), _dev(c), _dev(A), _dev(B)
    ga = _Guarded()
    monkeypatch.setattr(ops, "_empty", ga)
    y = ops.erase_rows(xd, cd, Ad, Bd)
    sums, counts = ops.label_column_sums(xd, labels, 5)
    target = ga((259, 320), device="cuda", dtype=torch.float32)
    target.copy_(xd)
    ops.erase_rows(target, cd, Ad, Bd, out=target)
    torch.cuda.synchronize()
    assert len(ga.bufs) == 5
    ga.check()
    want, bound = erase_bound(x, c, A, B)
    assert (np.abs(y.cpu().numpy() - want) <= bound).all() and torch.equal(target, y) and counts.sum().item() == 259
    assert ga.bufs[1][1] * 8 == _lib.lib().dbmm_workspace_bytes_label_colsums(259, 320, 5)


def test_wrappers_check_their_operands(monkeypatch):
    x, c, A, B = _erase_case(65, 64, 3)
    xd, cd, Ad, Bd = _dev(x), _dev(c), _dev(A), _dev(B)
    labels = _dev(np.zeros(65, dtype=np.int64))
    launched = []
    real = _lib.lib

    class _Spy:
        def __getattr__(self, name):
            if name in ("dbmm_erase_rows", "dbmm_label_colsums"):
                launched.append(name)
            return getattr(real(), name)
    monkeypatch.setattr(_lib, "lib", _Spy)
    with pytest.raises(_lib.DbmmError):
        ops.erase_rows(torch.from_numpy(x), cd, Ad, Bd)                               # a CPU tensor
    with pytest.raises(_lib.DbmmError):
        ops.erase_rows(xd, cd, torch.from_numpy(A), Bd)
    with pytest.raises(_lib.DbmmError):
        ops.erase_rows(xd.double(), cd, Ad, Bd)                                      # float64
    with pytest.raises(_lib.DbmmError):
        ops.erase_rows(xd, cd, Ad.double(), Bd)
    with pytest.raises(ops.DbmmUnsupported):
        ops.erase_rows(_dev(np.zeros((65, 100), dtype=np.float32)), _dev(np.zeros(100, dtype=np.float32)),
                       _dev(np.zeros((3, 100), dtype=np.float32)), _dev(np.zeros((3, 100), dtype=np.float32)))   # D = 100
    with pytest.raises(_lib.DbmmError):
        ops.erase_rows(xd, cd, Ad[:0], Bd[:0])                                       # R = 0
    wide = _dev(np.zeros((16, 64), dtype=np.float32))
    with pytest.raises(_lib.DbmmError):
        ops.erase_rows(xd, cd, wide, wide)                                           # R = 16
    with pytest.raises(_lib.DbmmError):
        ops.erase_rows(xd, cd, _dev(np.zeros((3, 128), dtype=np.float32)), Bd)       # a basis of the wrong width
    with pytest.raises(_lib.DbmmError):
        ops.erase_rows(xd, cd, Ad, Bd[:2])                                           # A and B of different ranks
    with pytest.raises(_lib.DbmmError):
        ops.erase_rows(xd, cd[:32], Ad, Bd)
    with pytest.raises(_lib.DbmmError):
        ops.erase_rows(xd, cd, Ad, Bd, out=xd[1:])                                   # a target of another shape
    both = torch.empty(66 * 64, device="cuda")
    with pytest.raises(_lib.DbmmError):
        ops.erase_rows(both[:65 * 64].view(65, 64), cd, Ad, Bd, out=both[64:].view(65, 64))     # overlapping, not the same
    with pytest.raises(_lib.DbmmError):
        ops.erase_rows(xd.t().contiguous().t(), cd, Ad, Bd)                          # not contiguous
    with pytest.raises(_lib.DbmmError):
        ops.label_column_sums(xd, labels, 17)                                        # G = 17
    with pytest.raises(_lib.DbmmError):
        ops.label_column_sums(xd, labels, 0)
    with pytest.raises(_lib.DbmmError):
        ops.label_column_sums(xd, labels.int(), 2)                                   # int32 labels
    with pytest.raises(_lib.DbmmError):
        ops.label_column_sums(xd, labels[:64], 2)
    with pytest.raises(_lib.DbmmError):
        ops.label_column_sums(xd, labels.cpu(), 2)
    with pytest.raises(_lib.DbmmError):
        ops.label_column_sums(torch.from_numpy(x), labels, 2)
    with pytest.raises(ops.DbmmUnsupported):
        ops.label_column_sums(_dev(np.zeros((65, 100), dtype=np.float32)), labels, 2)
    with pytest.raises(ValueError):
        analysis.erasure_fit(xd, np.arange(65) % 17)                                 # more than 16 labels
    with pytest.raises(ValueError):
        analysis.erasure_fit(xd, np.arange(65) % 2, method="inlp")
    with pytest.raises(ValueError):
        analysis.erasure_fit(xd)                                                     # a tensor needs its labels
    with pytest.raises(_lib.DbmmError):
        analysis.erasure_fit(torch.from_numpy(x), np.arange(65) % 2)
    assert launched == []                                                                # every refusal came before a launch


# ---- 3. end to end ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", ["leace", "orth"])
@pytest.mark.parametrize("G", [2, 4])
@pytest.mark.parametrize("D,N", [(64, 259), (1024, 600), (1024, 1027)])
def test_erase_after_fit_end_to_end(D, N, G, method):
    x64, labels = dataset(D, N, 4, G)
    x = x64.astype(np.float32)
    xd = _dev(x)
    fit = analysis.erasure_fit(xd, labels + 3, method=method)                            # any integers: np.unique order
    assert fit["rank"] == G - 1 and fit["labels"].tolist() == list(range(3, 3 + G)) and fit["n"] == N
    assert fit["counts"].tolist() == np.bincount(labels, minlength=G).tolist()
    out = analysis.erase(fit, xd)
    got = out.cpu().numpy().astype(np.float64)
    # Every label's mean and the overall mean of the kernel's rows are within the largest entry error of those of the float64
    # application of the same fp32 vectors, so the gap is within twice that of the reference's gap
    _, bound = erase_bound(x, fit["mean"], fit["A"], fit["B"])
    reference = mean_gap(apply64(x64, fit["mean"], fit["A"], fit["B"]), labels)
    before, after = mean_gap(x64, labels), mean_gap(got, labels)
    print(f"D={D} N={N} G={G} {method}: gap {before:.3e} -> {after:.3e}; float64 application of the fit {reference:.3e}, entry bound {bound.max():.3e}")
    assert before > 1e-2 and after <= reference + 2.0 * bound.max()
    assert abs(analysis.label_mean_gap(out, labels) - after) <= 1e-12
    again = analysis.erasure_fit(out, labels, method=method)
    print("    refit singular values", again["singular_values"])
    assert again["rank"] == 0 and again["A"].shape == (0, D)
    copy = analysis.erase(again, out)
    assert torch.equal(copy, out) and copy.data_ptr() != out.data_ptr()
    inplace = xd.clone()
    assert analysis.erase(fit, inplace, out=inplace) is inplace and torch.equal(inplace, out)


@pytest.fixture(scope="module")
def confounded(tmp_path_factory):
    """a confounded split as Waterbirds': (class prompts' path, spurious prompts' path, the table)"""
    D, N, seed = 1024, 4795, 7
    d = tmp_path_factory.mktemp("erase_prompts")
    paths = []
    for name, m in zip(("c", "s"), synth.embedding_text(seed, D)[:2]):
        paths.append(os.path.join(d, name + ".json"))
        json.dump({f"{name}{i}": m[:, i].numpy().tolist() for i in range(2)}, open(paths[-1], "w"))
    x, y, c = synth.embedding_dataset(seed, "train", N, D)
    return paths[0], paths[1], trainer.EmbeddingTable(x.numpy(), y.numpy(), c.numpy(), device="cuda")


def test_fit_on_balanced_rows_erases_the_attribute_and_keeps_the_class(confounded):
    cls, spu, table = confounded
    ratio = table.group_ratio.numpy()

    def scores(t):
        groups = trainer.validate_zs_linear_probing(t, cls, 0.01, 4096, ratio)[2]
        return groups["worst_acc"], trainer.validate_zs_linear_probing(t, spu, 0.01, 4096, ratio, target="spurious")[1]
    rows = analysis.balanced_rows(table.group_array, seed=0)
    assert np.bincount(table.group_array[rows]).tolist() == [int(table.group_counts.min())] * 4
    fit = analysis.erasure_fit(table, rows=rows)                                         # a table: its spurious attribute
    assert fit["rank"] == 1 and fit["n"] == len(rows) and fit["labels"].tolist() == [0, 1]
    erased = analysis.erased_table(table, fit)
    (worst0, spur0), (worst1, spur1) = scores(table), scores(erased)
    print(f"spurious prompts' accuracy {spur0:.4f} -> {spur1:.4f}; class prompts' worst group {worst0:.4f} -> {worst1:.4f}")
    assert spur0 > 0.95
    assert abs(spur1 - 0.5) < abs(spur1 - spur0)                                         # nearer to chance than to where it was
    assert abs(worst1 - worst0) <= 0.02
    # fitted on the confounded rows as they are, the same eraser takes class information along: the minority groups pay
    plain = analysis.erased_table(table, analysis.erasure_fit(table))
    assert scores(plain)[0] < worst0 - 0.1


def test_erased_table_and_report(schedule_data):
    paths, (train, val, test) = schedule_data
    fit = analysis.erasure_fit(train, rows=analysis.balanced_rows(train.group_array))
    before = train.embeddings.clone()
    erased = analysis.erased_table(train, fit)
    assert torch.equal(train.embeddings, before) and erased.embeddings.data_ptr() != train.embeddings.data_ptr()
    assert torch.equal(erased.embeddings, analysis.erase(fit, train))
    for name in ("targets", "targets_spurious", "targets_group", "group_counts", "group_ratio"):
        assert torch.equal(getattr(erased, name), getattr(train, name)), name
    assert (erased.group_array == train.group_array).all() and erased.filenames is train.filenames and erased.y_pred is train.y_pred
    opt = _schedule_opt("linear_probing", paths, epochs=1)
    optim.set_seed(42)
    log = []
    trainer.train_all_epochs(opt, erased, analysis.erased_table(val, fit), analysis.erased_table(test, fit), log=log)
    trains = [e for e in log if e["kind"] == "train1"]
    assert len(trains) == 1 and np.isfinite(trains[0]["loss"])
    assert trains[0]["counts"][:, 0].tolist() == train.group_counts.long().tolist()       # the source's groups and counts
    everything = analysis.erasure_fit(train)                                             # on all of train: its gap goes to rounding level
    report = analysis.erasure_report(opt, everything, train, val, test)
    assert set(report) == {"train", "val", "test"}
    for split, r in report.items():
        print(split, "gap", r["before"]["gap"], "->", r["after"]["gap"], "spurious", r["before"]["spurious_acc"], "->", r["after"]["spurious_acc"],
              "relative change", r["relative_change"])
        assert 0.0 < r["relative_change"] < 1.0 and set(r["before"]) == set(r["after"]) == {"class", "spurious_acc", "gap"}
        assert np.isfinite(r["after"]["gap"]) and "worst_acc" in r["after"]["class"]
    assert report["train"]["before"]["gap"] > 1e-2 and report["train"]["after"]["gap"] <= 1e-5
    assert report["train"]["after"]["spurious_acc"] <= report["train"]["before"]["spurious_acc"]


class _Doubling(torch.nn.Module):
    """x -> 2 x in eval mode (exact in fp32), x -> 0 in train mode; records the mode it was called in"""

    def __init__(self):
        super().__init__()
        self.modes = []

    def forward(self, x):
        self.modes.append(self.training)
        return x * (0.0 if self.training else 2.0)


def test_rows_and_transform():
    x64, labels = dataset(64, 259, 4, 2)
    xd = _dev(x64.astype(np.float32))
    rows = analysis.balanced_rows(labels, seed=1)
    picked = analysis.erasure_fit(xd, labels, rows=rows)
    alone = analysis.erasure_fit(xd[torch.from_numpy(rows).cuda()].contiguous(), labels[rows])       # the same rows in the same order
    assert picked["n"] == len(rows) and picked["counts"].tolist() == [len(rows) // 2] * 2
    for key in ("mean", "A", "B", "singular_values"):
        assert (picked[key] == alone[key]).all(), key
    with pytest.raises(ValueError):
        analysis.erasure_fit(xd, labels, rows=np.array([0, 259]))
    plain = analysis.erasure_fit(xd, labels)
    P = plain["B"].astype(np.float64).T @ plain["A"].astype(np.float64)
    for training in (True, False):
        t = _Doubling().train(training)
        fit = analysis.erasure_fit(xd, labels, transform=t)
        assert t.modes and not any(t.modes) and t.training == training                # eval inside, the mode as found afterwards
        assert (fit["mean"] == 2 * plain["mean"]).all() and fit["rank"] == 1          # doubling is exact in every moment
        Pt = fit["B"].astype(np.float64).T @ fit["A"].astype(np.float64)              # the eraser of 2 x is the eraser of x
        assert np.abs(Pt - P).max() <= 2.0 ** -20 * np.abs(P).max()
