"""Group DRO, the parts that need no GPU: the C entries are declared, exported and bound and refuse bad arguments before touching a
device; and the float64 restatement of one online group-DRO update (the oracle of tests/test_gpu_group_dro.py) gives the
hand-computed numbers of a 5-row, 3-group batch with one absent group."""
import ctypes
import math
from types import SimpleNamespace

import numpy as np
import pytest

from dbmm_amd import _lib

ENTRIES = ("dbmm_group_dro_weights", "dbmm_l2norm_sim_ce_bwd_weighted", "dbmm_adapter_train_step_gdro", "dbmm_adapter_sweep_step_gdro")


def gdro_update(loss_rows, groups, q, eta, G):
    """One online group-DRO update in float64 (Sagawa et al. 2020, Algorithm 1, shifted by the largest group loss):
    -> (n_g, L_g, new q, row weights q_g / n_g, robust loss).  A group id outside [0, G) belongs to no bucket."""
    l, g, q = np.asarray(loss_rows, dtype=np.float64), np.asarray(groups), np.asarray(q, dtype=np.float64)
    n = np.array([(g == k).sum() for k in range(G)], dtype=np.int64)
    L = np.array([l[g == k].sum() / n[k] if n[k] else 0.0 for k in range(G)])
    m = L[n > 0].max() if (n > 0).any() else 0.0
    qn = q * np.exp(eta * (L - m))                 # absent groups: L = 0
    qn = qn / qn.sum()
    w = np.where(n > 0, qn / np.maximum(n, 1), 0.0)
    return n, L, qn, w, float((qn * L).sum())


@pytest.fixture(scope="module")
def built():
    _lib.build()
    return _lib.lib()


def test_symbols_exported_and_bound(built):
    for name in ENTRIES:
        assert name in _lib.EXPORTS
        assert hasattr(ctypes.CDLL(_lib.LIB_PATH), name)


def test_argument_validation_without_gpu(built):
    buf = (ctypes.c_float * 1024)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    W = built.dbmm_group_dro_weights
    assert W(None, p, p, p, p, p, 8, 4, 0.01, None) == -4
    assert W(p, None, p, p, p, p, 8, 4, 0.01, None) == -4
    assert W(p, p, None, p, p, p, 8, 4, 0.01, None) == -4
    assert W(p, p, p, None, p, p, 8, 4, 0.01, None) == -4
    assert W(p, p, p, p, None, p, 8, 4, 0.01, None) == -4
    assert W(p, p, p, p, p, None, 8, 4, 0.01, None) == -4
    assert W(p, p, p, p, p, p, 8, 9, 0.01, None) == -1
    assert W(p, p, p, p, p, p, 8, 0, 0.01, None) == -1
    assert W(p, p, p, p, p, p, 1, 4, 0.01, None) == -1
    Bw = built.dbmm_l2norm_sim_ce_bwd_weighted
    assert Bw(p, p, 0.5, 0, p, p, p, None, p, 4, 0.01, p, 8, 128, 2, None) == -4       # groups
    assert Bw(p, p, 0.5, 0, p, p, p, p, None, 4, 0.01, p, 8, 128, 2, None) == -4       # weights
    assert Bw(p, p, 0.5, 0, p, p, p, p, p, 9, 0.01, p, 8, 128, 2, None) == -1
    assert Bw(p, p, 0.5, 0, p, p, p, p, p, 4, 0.01, p, 1, 128, 2, None) == -1
    S = built.dbmm_adapter_train_step_gdro
    ps = [p] * 26

    def step(groups, q, G, B, x=p):
        return S(x, p, *ps[2:], 0.5, p, 0.01, 0.1, 0.9, 0.0, 1, p, p, p, groups, q, 0.01, G, B, 128, 128, 2, p, 1 << 30, None)
    assert step(None, p, 4, 8) == -4
    assert step(p, None, 4, 8) == -4
    assert step(p, p, 4, 8, x=None) == -4
    assert step(p, p, 9, 8) == -1
    assert step(p, p, 4, 1) == -1
    Sw = built.dbmm_adapter_sweep_step_gdro
    nine, six = (ctypes.c_void_p * 9)(*[p.value] * 9), (ctypes.c_void_p * 6)(*[p.value] * 6)

    def sweep(q, G, B, table=p):
        return Sw(table, 100, p, 2, B, p, p, nine, six, None, 0.5, p, 0.01, p, 0.9, 0.0, 1, p, p, p, p, p, G, 1, q, 0.01, 2, B, 128, 128, 2, p,
                  1 << 30, None)
    assert sweep(None, 4, 8) == -4
    assert sweep(p, 4, 8, table=None) == -4
    assert sweep(p, 9, 8) == -1
    assert sweep(p, 4, 1) == -1


def test_restatement_on_a_hand_computed_batch():
    """losses (1, 3 | 2, 4, 3) in groups (0, 0 | 2, 2, 2), group 1 absent, q = 1/3 each, eta = ln 2:
    L = (2, 0, 3), m = 3, q' = (2^-1, 2^-3, 1) / 3, so q = (4, 1, 8) / 13; weights (4/13 / 2, 0, 8/13 / 3); loss (4 * 2 + 8 * 3) / 13."""
    n, L, q, w, loss = gdro_update([1.0, 3.0, 2.0, 4.0, 3.0], [0, 0, 2, 2, 2], [1 / 3] * 3, math.log(2.0), 3)
    assert n.tolist() == [2, 0, 3]
    assert L.tolist() == [2.0, 0.0, 3.0]
    assert np.abs(q - np.array([4.0, 1.0, 8.0]) / 13).max() < 1e-15
    assert np.abs(w - np.array([2.0 / 13, 0.0, 8.0 / 39])).max() < 1e-15
    assert abs(loss - 32.0 / 13) < 1e-14
    assert abs(q.sum() - 1.0) < 1e-15
    # a group id outside [0, G) belongs to no bucket; a huge step size stays finite and puts the mass on the worst group
    n2, L2, q2, w2, _ = gdro_update([1.0, 3.0, 2.0, 4.0, 3.0, 100.0], [0, 0, 2, 2, 2, 7], [1 / 3] * 3, 1000.0, 3)
    assert n2.tolist() == [2, 0, 3] and L2.tolist() == [2.0, 0.0, 3.0]
    assert np.isfinite(q2).all() and q2[2] == 1.0 and q2[0] == 0.0


def test_sweep_result_name_suffix_only_with_the_flag():
    from dbmm_amd import trainer
    o = SimpleNamespace(dataset="waterbirds", tl_method="adapter", batch_size=128, learning_rate=0.1)
    plain = trainer.sweep_result_name(o)
    o.robust = False
    assert trainer.sweep_result_name(o) == plain
    o.robust = True
    assert trainer.sweep_result_name(o) == plain + "_gdro"
