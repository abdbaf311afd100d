"""The order of the per-label column sums and of their merge (csrc/label_sums.h), to the bit: ops.label_column_sums and one iteration of
ops.kmeans_fit against the host restatement of tests/test_erasure_host.py.  A float64 error bound holds for any order; the order is
fully specified -- P from (N, D) alone, row order within a range, each quarter of the ranges in range order, ((q0 + q1) + q2) + q3 --,
so numpy reproduces it exactly and a reordered walk, merge or partition fails here."""
import numpy as np
import pytest
import torch

from dbmm_amd import ops
from test_erasure_host import fixed_order_inertia, fixed_order_sums, sums_ranges

pytestmark = pytest.mark.gpu

# (N, D, labels): the smallest shapes at which each branch of the order exists
CASES = [
    (1, 64, 1),              # P = 1; three quarters empty
    (65, 64, 2),             # P = 2, rows 33
    (259, 64, 3),            # P = 5; quarters of 2, 2, 1, 0; four accumulators, one of them padding
    (1027, 512, 16),         # two slabs; P = 17; quarters of 5, 5, 5, 2
    (1200, 4096, 4),         # sixteen slabs; P = 19; last range 48 rows
    (140001, 64, 3),         # P = 2048 capped by the units; rows 69; ranges 2029 and up are empty (k-means: D = 8)
]
RANGES = [(1, 1), (2, 33), (5, 52), (17, 61), (19, 64), (2048, 69)]
IDS = [f"n{N}_d{D}_g{G}" for N, D, G in CASES]


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _rows(seed, N, D):
    """fp32 rows whose scales spread over 2^-20 .. 2^20: sums of rows that are close to each other (as CLIP rows are) are exact in
    float64 up to thousands of rows, and exact sums have the same bits in any order.  With 40 binary places between the rows nearly
    every addition rounds, so the order shows in the bits"""
    rng = np.random.RandomState(seed)
    return (rng.standard_normal((N, D)) * 2.0 ** rng.randint(-20, 21, size=(N, 1))).astype(np.float32)


def _one_chain(x, labels, G):
    """every label's rows in one row-order float64 chain: no ranges, no quarters"""
    return np.stack([np.add.reduce(x[labels == g].astype(np.float64), axis=0) for g in range(G)])


def test_the_cases_have_the_ranges_they_are_chosen_for():
    assert [sums_ranges(N, D) for N, D, _ in CASES] == RANGES
    assert sums_ranges(140001, 8) == (2048, 69) and 2029 * 69 >= 140001 > 2028 * 69


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_label_column_sums_to_the_bit(case):
    N, D, G = case
    x = _rows(N + D, N, D)
    labels = np.random.RandomState(G).randint(0, G, size=N).astype(np.int64)
    if N == 1027:                                                                # ids outside [0, G): as 32 bits 2^32 + 1 would be label 1
        labels[::7] = np.array([-1, 2 ** 32 + 1], dtype=np.int64)[np.arange(len(labels[::7])) % 2]
    want_sums, want_counts = fixed_order_sums(x, labels, G)
    assert N < 65 or (want_sums != _one_chain(x, labels, G)).any()                # from two ranges on, another order gives other bits
    sums, counts = ops.label_column_sums(_dev(x), _dev(labels), G)
    differ = int((sums.cpu().numpy() != want_sums).sum())
    print(f"N={N} D={D} G={G}: {differ} of {G * D} entries differ from the restated order; counts {counts.tolist()}")
    assert torch.equal(counts.cpu(), torch.from_numpy(want_counts))
    assert torch.equal(sums.cpu(), torch.from_numpy(want_sums))


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_one_kmeans_iteration_to_the_bit(case):
    N, D, K = case
    D = 8 if N == 140001 else D                                                  # as the ragged case of the k-means tests
    x = _rows(N + D + 1, N, D)
    start = x[:: max(N // K, 1)][:K].copy()                                      # K rows of x: every cluster keeps at least its own
    xd, cd = _dev(x), _dev(start)
    centers, labels, info = ops.kmeans_fit(xd, cd, max_iter=1)
    assert info["iterations"] == 1
    labels = labels.cpu().numpy()
    sums, counts = fixed_order_sums(x, labels.astype(np.int64), K)
    assert info["counts"].tolist() == counts.tolist() and (counts > 0).all()
    assert N < 65 or (sums != _one_chain(x, labels, K)).any()
    want = (sums / counts[:, None].astype(np.float64)).astype(np.float32)
    got = centers.cpu().numpy()
    assigned, dmin = ops.kmeans_assign(xd, cd)                                   # the assignment the iteration made, on the start centres
    inertia = fixed_order_inertia(dmin.cpu().numpy(), D)
    print(f"N={N} D={D} K={K}: {int((got != want).sum())} of {K * D} centre entries differ; inertia {info['inertia']!r}, restated {inertia!r}")
    assert (assigned.cpu().numpy() == labels).all()
    assert torch.equal(centers.cpu(), torch.from_numpy(want))
    assert info["inertia"] == inertia
