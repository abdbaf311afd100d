"""Group-wise embedding statistics, the parts that need no GPU: the C entries are declared, exported and bound and refuse bad
arguments before touching a device; representation_table reproduces the reference's recorded frames; and the fixture's recorded
distances are what a float64 recomputation from the regenerated inputs gives (which pins tools/make_golden_group_stats.py)."""
import ctypes

import numpy as np
import pytest
import torch

from dbmm_amd import _lib, synth

SPLITS = ("train", "val", "test")


def regenerate(fx, split):
    """(embeddings, groups, confidences) of a fixture split from its seed, as tools/make_golden_group_stats.py builds them"""
    n = int(fx["sizes"][list(fx["splits"]).index(split)])
    seed = int(fx["seed"])
    x, y, c = synth.embedding_dataset(seed, split, n, int(fx["dim"]), p_y=float(fx["p_y"]), p_agree=float(fx["p_agree"]))
    conf = synth.uniform(seed, split + "/conf", (n,), 0.5, 1.0)
    return (x * float(fx["scale"])).contiguous(), 2 * y + c, conf


@pytest.fixture(scope="module")
def fx(golden):
    return golden("group_stats.npz")


@pytest.fixture(scope="module")
def built():
    _lib.build()
    return _lib.lib()


def test_symbols_exported_and_bound(built):
    for name in ("dbmm_pairdist_group_sums", "dbmm_workspace_bytes_pairdist"):
        assert name in _lib.EXPORTS
        assert hasattr(ctypes.CDLL(_lib.LIB_PATH), name)
    assert _lib.kernel_source_hash("pairdist_tile_kernel") is not None


def test_argument_validation_without_gpu(built):
    buf = (ctypes.c_float * 1024)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    big = 1 << 30
    assert built.dbmm_pairdist_group_sums(p, p, p, p, 10, 100, 4, p, big, None) == -5       # D % 64 != 0: no kernel
    assert built.dbmm_pairdist_group_sums(p, p, p, p, 10, 8192, 4, p, big, None) == -5      # D > 4096
    assert built.dbmm_pairdist_group_sums(p, p, p, p, 10, 128, 9, p, big, None) == -1       # G > 8
    assert built.dbmm_pairdist_group_sums(p, p, p, p, 0, 128, 4, p, big, None) == -1
    assert built.dbmm_pairdist_group_sums(p, p, p, p, 10, 128, 4, None, big, None) == -4    # null workspace
    assert built.dbmm_pairdist_group_sums(None, p, p, p, 10, 128, 4, p, big, None) == -4
    assert built.dbmm_pairdist_group_sums(p, p, p, p, 10, 128, 4, p, 16, None) in (-2, -3)  # workspace too small (or the ctypes buffer unaligned)


def test_workspace_is_linear_in_rows(built):
    """the planes and 8 bytes per row, 128 KB of workgroup sums: nothing N x N"""
    for n, d in ((4795, 1024), (162770, 1024), (40000, 640)):
        b = built.dbmm_workspace_bytes_pairdist(n, d)
        dp = (d + 127) // 128 * 128
        assert n * dp * 4 <= b <= n * (dp * 4 + 8) + (1 << 18)


def test_representation_table_reproduces_reference_frames(fx):
    from dbmm_amd import analysis
    keys = [str(k) for k in fx["acc_keys"]]
    for split in SPLITS:
        groups = [int(g) for g in fx[f"{split}/groups"]]
        names = ["full"] + groups
        stats = {"pairwise_distance": dict(zip(names, fx[f"{split}/pairwise_distance"])),
                 "mean_vector_norm": dict(zip(names, fx[f"{split}/mean_vector_norm"].astype(np.float32)))}
        df = analysis.representation_table(stats, dict(zip(keys, fx[f"{split}/zs_acc"])))
        assert list(df.index) == [str(s) for s in fx[f"{split}/table_index"]]
        assert list(df.columns) == [str(s) for s in fx[f"{split}/table_columns"]]
        assert np.array_equal(df.to_numpy(dtype=np.float64), fx[f"{split}/table"])


def test_recorded_distances_are_the_float64_recomputation(fx):
    for split in SPLITS:
        x, g, conf = regenerate(fx, split)
        xd = x.double()
        d = torch.cdist(xd, xd, compute_mode="donot_use_mm_for_euclid_dist")
        n = x.shape[0]
        rec = fx[f"{split}/pairwise_distance"]
        assert abs(d.sum().item() / (n * (n - 1)) - rec[0]) <= 1e-9 * rec[0]
        groups = [int(k) for k in fx[f"{split}/groups"]]
        assert groups == sorted(set(g.tolist()))
        for i, k in enumerate(groups):
            m = g == k
            nk = int(m.sum())
            want = d[m][:, m].sum().item() / (nk * (nk - 1))
            assert abs(want - rec[1 + i]) <= 1e-9 * rec[1 + i]
            mv = xd[m].mean(0)
            assert abs(mv.norm().item() - fx[f"{split}/mean_vector_norm"][1 + i]) <= 1e-5 * mv.norm().item()
            assert np.abs(mv.numpy()[::int(fx["sample_stride"])] - fx[f"{split}/mean_vector_samples"][1 + i]).max() <= 1e-6
        # the generator's condition behind the GPU test's 1e-4 bound: no squared distance below 1 % of the mean centred squared norm
        xc = xd - xd.mean(0)
        d2 = d ** 2
        d2.fill_diagonal_(float("inf"))
        assert d2.min().item() > 0.01 * (xc ** 2).sum(1).mean().item()
