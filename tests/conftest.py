import glob
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle")):
    if p not in sys.path:
        sys.path.insert(0, p)

import dbmm_amd  # noqa: E402,F401  (root shim -> debiasing-multi-modal_amd/)

GOLDEN = os.path.join(ROOT, "tests", "golden")


def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: needs a real MI355X (run with -m gpu on the GPU box)")


def pytest_collection_modifyitems(config, items):
    if torch.cuda.is_available():
        return
    skip = pytest.mark.skip(reason="no GPU in this container")
    for item in items:
        if "gpu" in item.keywords:
            item.add_marker(skip)


class _JoinedNpz:
    """one fixture stored as <name>.npz plus <name>.part*.npz (each committed file stays under 1 MiB): the NpzFile
    interface the tests use, `files` and item lookup"""

    def __init__(self, parts):
        self._by_key = {k: p for p in parts for k in p.files}
        self.files = list(self._by_key)

    def __getitem__(self, key):
        return self._by_key[key][key]

    def __contains__(self, key):
        return key in self._by_key


@pytest.fixture(scope="session")
def golden():
    def load(name):
        path = os.path.join(GOLDEN, name)
        parts = sorted(glob.glob(path[:-len(".npz")] + ".part*.npz")) if name.endswith(".npz") else []
        if not parts:
            return np.load(path, allow_pickle=False)
        return _JoinedNpz([np.load(p, allow_pickle=False) for p in [path] + parts])
    return load


def relerr(a, b):
    a, b = torch.as_tensor(a).double(), torch.as_tensor(b).double()
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-30)).item()


def summary(t, nsample=256):
    f = t.detach().double().flatten().cpu()
    step = max(1, f.numel() // nsample)
    return np.array([f.sum().item(), f.abs().sum().item()]), f[::step][:nsample].float().numpy()


@pytest.fixture
def option():
    """set a library option (dbmm_set_option) for the duration of a test: option("igemm_halo", 0)"""
    from dbmm_amd import ops
    saved = {}

    def set_(name, value):
        old = ops.set_option(name, int(value))
        saved.setdefault(name, old)
    yield set_
    for name, old in saved.items():
        ops.set_option(name, old)
