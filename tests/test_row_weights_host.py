"""Per-row loss weights, the host side (no device): failure_weights against weights recorded from the reference's own
GetResampledWeightsCE (tests/golden/resample_weights.npz; HISTORY.md says how they were recorded), weighted_sampler_order against the
real DataLoader + WeightedRandomSampler, jtt_weights, the mean-1 normalisation and the option parsing's refusals."""
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch
from torch.utils.data import DataLoader, TensorDataset, WeightedRandomSampler

from conftest import ROOT
from dbmm_amd import ops, trainer

CASES = ("minor1_corrected", "minor0_corrected", "more_wrong_than_right", "not_corrected")


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "resample_weights.npz"))


def _counts(y, wrong):
    """per class (rows, rows predicted right)"""
    return {c: (int((y == c).sum()), int(((y == c) & ~wrong).sum())) for c in (0, 1)}


def _branch(y, wrong):
    """(minority class, imbal, reweighted) of the class-bias correction, from the counts alone"""
    n = _counts(y, wrong)
    major, minor = (1, 0) if n[0][0] < n[1][0] else (0, 1)
    return minor, n[major][0] / n[minor][0], n[major][1] / n[minor][1]


@pytest.mark.parametrize("name", CASES)
def test_failure_weights_equal_the_reference(name, golden):
    y, wrong, want = golden[name + "_y"].astype(np.int64), golden[name + "_wrong"], golden[name + "_w"]
    assert 900 <= len(y) <= 1100 and want.dtype == np.float64
    n = _counts(y, wrong)
    minor, imbal, reweighted = _branch(y, wrong)
    # each case takes the branch its name says, asserted from the counts
    if name == "minor1_corrected":
        assert minor == 1 and imbal < reweighted and all(2 * n[c][1] >= n[c][0] for c in (0, 1))
    elif name == "minor0_corrected":
        assert minor == 0 and imbal < reweighted and all(2 * n[c][1] >= n[c][0] for c in (0, 1))
    elif name == "more_wrong_than_right":
        assert 2 * n[1][1] < n[1][0]                                       # class 1: fewer right than wrong rows, no up-sampling
        assert np.unique(want[(y == 1)]).size == 1                         # ... so its wrong and right rows weigh the same
    else:
        assert imbal >= reweighted                                         # no correction: the minority class's right rows keep 1
        assert (want[(y == minor) & ~wrong] == 1.0).all()
    got = trainer.failure_weights(y, wrong)
    assert got.dtype == np.float64 and got.shape == want.shape
    assert (np.abs(got - want) <= 1e-12 * np.abs(want)).all()
    assert np.array_equal(got, trainer.failure_weights(y, wrong, correct_class_bias=True, reweighting_by_class=False))


def test_failure_weights_departures_and_refusals():
    y = np.array([0] * 6 + [1] * 4)
    # class 0 has no wrong rows (the reference divides by zero): weight 1; class 1: 3 right, 1 wrong -> 3 on the wrong row
    wrong = np.zeros(10, bool); wrong[9] = True
    w = trainer.failure_weights(y, wrong, correct_class_bias=False)
    assert w[:9].tolist() == [1.0] * 9 and w[9] == 3.0
    # with the correction: imbal = 6 / 4, reweighted = 6 / 3 -> class 1 times (2 / 1.5)
    w = trainer.failure_weights(y, wrong)
    assert np.allclose(w[:6], 1.0) and np.allclose(w[6:9], 2.0 / 1.5, rtol=1e-15) and np.isclose(w[9], 3.0 * 2.0 / 1.5, rtol=1e-15)
    # class 1 has no right rows (the reference divides by zero in the correction): the correction is skipped
    wrong = np.zeros(10, bool); wrong[6:] = True; wrong[0] = True
    w = trainer.failure_weights(y, wrong)
    assert w[0] == 5.0 and (w[1:] == 1.0).all()
    # reweighting_by_class multiplies the minority class by reweighted itself
    wrong = np.zeros(10, bool); wrong[9] = True
    assert np.allclose(trainer.failure_weights(y, wrong, reweighting_by_class=True)[6:9], 2.0)
    for bad in (np.array([0, 1, 2, 1]), np.zeros(4, np.int64), np.array([1, 1, 1, 1])):
        with pytest.raises(ValueError):
            trainer.failure_weights(bad, np.zeros(4, bool))
    with pytest.raises(ValueError):
        trainer.failure_weights(y, np.zeros(9, bool))


def test_weighted_sampler_order_is_the_dataloaders():
    n = 257
    w = np.random.default_rng(3).uniform(0.0, 4.0, n)
    w[::7] = 0.0
    for seed in (0, 42):
        torch.manual_seed(seed)
        ds = TensorDataset(torch.arange(n))
        loader = DataLoader(ds, sampler=WeightedRandomSampler(w, n, replacement=True), batch_size=64)
        want = torch.cat([b[0] for b in loader])
        after_loader = torch.rand(3)
        torch.manual_seed(seed)
        got = trainer.weighted_sampler_order(w)
        assert got.dtype == torch.int64 and torch.equal(got, want)
        assert torch.equal(torch.rand(3), after_loader)                   # the global stream is left where the loader leaves it
        assert (w[got.numpy()] > 0).all() and len(set(got.tolist())) < n  # rows of weight 0 never drawn; rows repeat


def test_jtt_weights_and_normalisation():
    wrong = np.array([True, False, False, True, False])
    w = trainer.jtt_weights(wrong, 5)
    assert w.dtype == np.float64 and w.tolist() == [5.0, 1.0, 1.0, 5.0, 1.0]
    nw = trainer.normalise_row_weights(w, 5)
    assert nw.dtype == np.float64 and nw.shape == (1, 5)
    assert np.array_equal(nw[0], w * 5 / w.sum()) and abs(nw.mean() - 1.0) <= 1e-15
    # float64 on the host: weights whose sum fp32 cannot hold still come out at mean 1
    big = np.ones(1 << 20); big[0] = 1e9
    assert abs(trainer.normalise_row_weights(big, len(big)).mean() - 1.0) <= 1e-12
    per = trainer.normalise_row_weights(np.stack([w, 2 * w, np.ones(5)]), 5, replicas=3)
    assert per.shape == (3, 5) and np.allclose(per[0], per[1], rtol=1e-15) and np.allclose(per.mean(1), 1.0, rtol=1e-15)
    assert trainer.normalise_row_weights(w[None], 5, replicas=3).shape == (1, 5)


def _opt(**k):
    return SimpleNamespace(tl_method="adapter", **k)


def test_option_parsing_without_a_device():
    N = 6
    w = np.arange(1.0, N + 1)
    assert trainer._row_weight_option(_opt(), N) is None
    assert trainer._row_weight_option(_opt(row_weights=None, resample_ce=True), N) is None      # resample_ce alone: the reference's no-op
    rw = trainer._row_weight_option(_opt(row_weights=w), N)
    assert rw.mode == "loss" and rw.dev is None and np.array_equal(rw.host[0], w * N / w.sum())
    assert trainer._row_weight_option(_opt(row_weights=w.tolist(), row_weight_mode="sample"), N).mode == "sample"
    rw = trainer._row_weight_option(_opt(row_weights=np.stack([w, w[::-1]])), N, replicas=2)
    assert rw.host.shape == (2, N) and np.array_equal(rw.of(1), w[::-1] * N / w.sum()) and np.array_equal(rw.of(0), rw.host[0])
    # "zs_failures": failure_weights of what the callback returns, called only then
    y, wrong = np.array([0, 0, 0, 1, 1, 1]), np.array([False, False, True, False, False, False])
    rw = trainer._row_weight_option(_opt(row_weights="zs_failures"), N, zs_failures=lambda: (y, wrong))
    fw = trainer.failure_weights(y, wrong)
    assert np.array_equal(rw.host[0], fw * N / fw.sum())
    for bad in (w[:-1], np.stack([w, w, w]), np.full(N, np.nan), np.r_[w[:-1], np.inf], -w, np.zeros(N), np.ones((2, 2, N))):
        with pytest.raises(ValueError):
            trainer._row_weight_option(_opt(row_weights=bad), N, replicas=2)
    with pytest.raises(ValueError):
        trainer._row_weight_option(_opt(row_weights=np.stack([w, w])), N)                       # [2, N] for a single run
    with pytest.raises(ValueError):
        trainer._row_weight_option(_opt(row_weights=w, row_weight_mode="both"), N)
    with pytest.raises(ValueError):
        trainer._row_weight_option(_opt(row_weights="failures"), N)
    with pytest.raises(ops.DbmmUnsupported):
        trainer._row_weight_option(_opt(row_weights=w, robust=True), N)
    with pytest.raises(ops.DbmmUnsupported):
        trainer._row_weight_option(_opt(row_weights=w, contrastive_weight=0.5), N)


def test_pass_keeps_its_positional_form():
    p = trainer._Pass("table", None, True, 64, False, True)
    assert p.weights is None and trainer._Pass("t", None, True, 64, False, True, "w").weights == "w"


def test_train_jtt_refuses_before_building_a_model():
    table = [0] * 8                                                       # never touched: the refusals come first
    with pytest.raises(ValueError):
        trainer.train_jtt(_opt(row_weights=np.ones(8)), table, None, None)
    with pytest.raises(ValueError):
        trainer.train_jtt(_opt(jtt_epochs=0), table, None, None)
    with pytest.raises(ops.DbmmUnsupported):
        trainer.train_jtt(_opt(robust=True), table, None, None)
    with pytest.raises(ValueError):
        trainer.train_jtt(SimpleNamespace(tl_method="contrastive_adapter"), table, None, None)


def test_sweep_cuts_per_replica_weights_to_each_group():
    """train_sweep's [R, N] weights reach a lock-step group as its own rows, a replica that runs alone as its one row; shared forms
    pass through untouched"""
    N, R = 5, 19
    w = np.arange(R * N, dtype=np.float64).reshape(R, N) + 1.0
    opts = [SimpleNamespace(tl_method="adapter", learning_rate=0.1 * (r + 1), row_weights=w) for r in range(R)]
    first = trainer._with_replica_weights(opts[:16], R, 0)                  # more than 16 replicas: groups of 16
    rest = trainer._with_replica_weights(opts[16:], R, 16)
    assert len(first) == 16 and all(np.array_equal(o.row_weights, w[:16]) for o in first)
    assert len(rest) == 3 and all(np.array_equal(o.row_weights, w[16:]) for o in rest)
    assert [o.learning_rate for o in rest] == [o.learning_rate for o in opts[16:]] and all(a is not b for a, b in zip(rest, opts[16:]))
    assert opts[0].row_weights is w                                         # the caller's namespaces are left alone
    trainer.normalise_row_weights(rest[0].row_weights, N, replicas=3)       # what the schedule then makes of a group's rows
    for k in (0, 7, 18):                                                    # replica by replica (the sequential path): one row, [N]
        alone = trainer._with_replica_weights([opts[k]], R, k)
        assert len(alone) == 1 and np.array_equal(alone[0].row_weights, w[k]) and alone[0].row_weights.ndim == 1
    # one group of all replicas: the whole array
    three = [SimpleNamespace(row_weights=w[:3]) for _ in range(3)]
    assert all(np.array_equal(o.row_weights, w[:3]) for o in trainer._with_replica_weights(three, 3, 0))
    # shared forms and a single replica: the same objects back
    for given in (None, "zs_failures", w[0], w[:1], w[:4]):
        shared = [SimpleNamespace(row_weights=given) for _ in range(3)]
        assert all(a is b for a, b in zip(trainer._with_replica_weights(shared, 3, 0), shared))
    solo = [SimpleNamespace(row_weights=w[:1])]
    assert trainer._with_replica_weights(solo, 1, 0)[0] is solo[0]
    assert trainer._with_replica_weights([SimpleNamespace()], 4, 2)[0].__dict__ == {}
