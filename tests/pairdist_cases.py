"""The inputs and float64 preliminaries shared by the GPU tests of the pairwise-kernel family (csrc/pairdist.hip): test_gpu_group_stats,
test_gpu_silhouette, test_gpu_mmd, test_gpu_kernel_probe and test_gpu_kernel_ridge.  No tests here; every generator is seeded, draws on
the host and moves the result to DEV, so the same call gives the same rows in every file."""
import numpy as np
import torch

DEV = "cuda" if torch.cuda.is_available() else "cpu"   # the float64 side of every test runs anywhere
SPREAD = 0.5
ISO_SCALES = (0.25, 1.0, 4.0, 16.0)        # gamma = scale / (2 SPREAD^2 D): the mean squared distance of the isotropic rows
CLU_SCALES = (0.5, 2.0, 8.0, 24.0)         # gamma = scale / (15.5 SPREAD^2 D): that of the clustered rows (2 within + 18 * 3/4 between)


def rows(n, d, seed, spread=SPREAD):
    """isotropic rows about a small common offset: d^2 is nearly constant in high D"""
    g = torch.Generator().manual_seed(seed)
    return (spread * torch.randn(n, d, generator=g) + 0.1 * torch.randn(1, d, generator=g)).to(DEV)


def clustered_rows(n, d, seed, spread=SPREAD):
    """four centres three spreads apart per coordinate plus noise: d^2 is 2 spread^2 D within a cluster and about 20 spread^2 D
    between two, so kernel values span orders of magnitude and a wrong exponent scale cannot hide.  (rows, cluster of every row)"""
    g = torch.Generator().manual_seed(seed)
    centres = 3.0 * spread * torch.randn(4, d, generator=g)
    which = torch.randint(0, 4, (n,), generator=g)
    return (centres[which] + spread * torch.randn(n, d, generator=g) + 0.1 * torch.randn(1, d, generator=g)).to(DEV), which


def ladder(kind, d):
    return [s / ((2.0 if kind == "iso" else 15.5) * SPREAD ** 2 * d) for s in (ISO_SCALES if kind == "iso" else CLU_SCALES)]


def sq_dists(x, y=None, chunk=1024):
    """float64 squared distances from direct differences, row chunks of x against y (x itself by default).  cdist's direct kernel
    launches one block per pair: chunk * N stays under 2^24 blocks"""
    xd = x.double()
    yd = xd if y is None else y.double()
    return torch.cat([torch.cdist(xd[i:i + chunk], yd, compute_mode="donot_use_mm_for_euclid_dist") for i in range(0, xd.shape[0], chunk)]) ** 2


def check_preconditions(x, d2, gammas, what):
    xc = x.double() - x.double().mean(0)
    worst = 2.0 * (xc ** 2).sum(1).max().item()                          # max_ij (|a|^2 + |b|^2), centred
    gmax = max(gammas)
    print(f"{what}: gamma_max * max(|a|^2 + |b|^2) = {gmax * worst:.2f} (<= 64), gamma_max * max d^2 = {gmax * d2.max().item():.2f} (<= 80)")
    assert gmax * worst <= 64.0 and gmax * d2.max().item() <= 80.0, f"{what}: the test's own inputs break the bound's preconditions"


def onehot(g, G):
    return (g.unsqueeze(1) == torch.arange(G, device=g.device).unsqueeze(0)).double()                  # [N, G]; labels outside: no column


class GuardedAlloc:
    """stand-in for ops._empty: every output and workspace sits between two sentinel-filled zones"""
    S = -7.0

    def __init__(self):
        self.bufs = []

    def __call__(self, shape, device=None, dtype=torch.float32, **kw):
        shape = (shape,) if isinstance(shape, int) else tuple(shape)
        n = int(np.prod(shape))
        pad = 1 << 16                                                       # elements: a multiple of 16 bytes for every dtype used
        raw = torch.full((n + 2 * pad,), self.S, device=device, dtype=dtype)
        self.bufs.append((raw, pad, n))
        return raw[pad:pad + n].view(shape)

    def check(self):
        assert self.bufs
        for raw, pad, n in self.bufs:
            lo, hi = raw[:pad], raw[pad + n:]
            assert bool((lo == self.S).all()) and bool((hi == self.S).all()), \
                f"guard zone of a {n}-element {raw.dtype} buffer was written: {(lo != self.S).sum().item()} before, {(hi != self.S).sum().item()} after"
