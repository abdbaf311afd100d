"""The kernel cases of the L1-probe tests, shared by tests/test_dfr_host.py (which checks on the CPU what the GPU tests rely on) and
tests/test_gpu_dfr.py: operands, the float64 / float32 references (computed once per case and cached) and the synthetic DFR split."""
import functools

import numpy as np
import torch

from dbmm_amd import dfr, synth

# (n, D, C, R): one row (fewer rows than the 16 waves); a ragged quad group at three classes; DFR's shape with more than one replica
# (8 waves); eight classes at full width (the 4-wave instantiation); five classes (CM = 8) on a ragged width; and, past the issue's
# list, the 16-wave instantiation at its register limit (two classes, three quad groups, the last one ragged)
SHAPES = ((1, 4, 2, 1), (17, 252, 3, 3), (300, 1024, 2, 5), (64, 1024, 8, 2), (33, 132, 5, 1), (40, 520, 2, 2))
ITERS = (1, 2, 8)
BAND = 1e-3                 # entries whose float64 pre-threshold magnitude is within eta lam (1 +- BAND) are left out of the zero pattern
BAND_CAP = 0.05
LAM_BIG = 50.0              # zeroes everything: |dCE/dW| <= max |x| < 50 on these operands
LAMS = (0.02, 0.0, LAM_BIG, 0.006, 0.06)


@functools.lru_cache(maxsize=None)
def operands(n, D, C, R):
    """table [n + 7, D], labels, idx [R, n] (repeated rows, rows outside the table), lam / step float32 [R]: host tensors"""
    seed = 1000 * n + D + C + R
    N = n + 7
    table = synth.normal(seed, "dfr/table", (N, D)).contiguous()
    labels = (synth.uniform(seed, "dfr/labels", (N,)) * C).long().clamp(0, C - 1)
    idx = (synth.uniform(seed, "dfr/idx", (R, n)) * N).long().clamp(0, N - 1)
    if n >= 4:
        idx[:, 1] = idx[:, 0]                       # a repeated row
        idx[:, 2] = -3                              # clamped to row 0
        idx[:, 3] = N + 5                           # clamped to the last row
    lam = torch.tensor(LAMS[:R], dtype=torch.float32)
    step = dfr.prox_steps(table, idx).float()
    return table, labels, idx.contiguous(), lam, step


@functools.lru_cache(maxsize=None)
def references(n, D, C, R, iters, accelerate):
    """(state64, stats64, state32, stats32) of `iters` iterations from the zero start, on the float32 operands the kernel reads"""
    table, labels, idx, lam, step = operands(n, D, C, R)
    out = []
    for dt in (torch.float64, torch.float32):
        out += list(dfr.prox_fit_reference(table, idx, labels, lam.double(), step.double(), None, iters, accelerate, dtype=dt, n_classes=C))
    return tuple(out)


def band_mask(n, D, C, R, iters, accelerate):
    """bool [R, C, D]: True where the zero pattern is asserted (the float64 pre-threshold magnitude is outside eta lam (1 +- BAND))"""
    _, _, _, lam, step = operands(n, D, C, R)
    z = references(n, D, C, R, iters, accelerate)[1]["z"].abs()
    thr = (lam.double() * step.double()).view(R, 1, 1)
    return (z - thr).abs() > BAND * thr


def make_split(device):
    """the synthetic split of the end-to-end tests: synth.embedding_dataset(3, ..., dim=64), 4000 / 1200 / 4000 rows"""
    from dbmm_amd import trainer
    out = []
    for split, n in (("train", 4000), ("val", 1200), ("test", 4000)):
        x, y, c = synth.embedding_dataset(3, split, n, dim=64)
        out.append(trainer.EmbeddingTable(x, y, c, device=device))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def dfr_split():
    """the split on the host, built once for the session (device tables are built per module by make_split and released with it:
    nothing of these tests stays allocated on the GPU while later files run)"""
    return make_split("cpu")


TUNE_SEED = 32              # dfr_seed of the full-grid test: the reference's best and second-best C are 0.0888 apart in worst-group
                            # accuracy on the held-out half, whose smallest group has 25 rows (two rows: 0.08).  Checked on the CPU


def tuning_margin(record, val_table, halves):
    """(best - second best mean tuning score, two rows of the smallest group of the held-out half)"""
    m = sorted((t["mean"] for t in record["tuning"]), reverse=True)
    small = np.bincount(np.asarray(val_table.group_array)[halves[1]]).min()
    return m[0] - m[1], 2.0 / small
