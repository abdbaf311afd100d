"""The attention pool (dbmm_attnpool / dbmm_attnpool_x) and the batched GEMM under it (dbmm_gemm_batched) against float64, black box:
nothing here looks at the workspace, so a rewrite of the operator's internal layout keeps these tests.

Operator.  Reference = clip_oracle.attention_pool on .double() tensors (the reference's formulation: every k and v projection, nothing
collapsed).  err = max|out - ref64| / max|ref64| (conftest.relerr).  Bound: err <= 4 x the err of the same oracle in fp32 on the CPU on
the same inputs, and err < 1e-5 (the bound of test_gpu_kernels.py::test_attnpool) always.  4 is the margin this suite grants a
fixed-order fp32 reduction in another order (test_gpu_supcon.py::test_backward_against_float64, test_gpu_group_dro.py); on the CPU the
kernel's collapsed algebra in fp32 sits at 0.3 - 1.1 x the oracle's err.  The figures in the docstrings are one run's; the oracle's err
depends on the CPU's BLAS, so the ratios move a little between machines.

dbmm_gemm_batched.  Reference = float64 einsum; bound: err <= 4 x the err of torch.matmul in fp32 (with the same epilogue in fp32) on the
same operands.  Every operand is a strided view inside a NaN-filled buffer and the output a view inside a sentinel-filled one: a read
outside an operand's extent that reaches an accumulator shows as NaN, a write outside the M x N outputs as a changed sentinel."""
import functools
import math

import pytest
import torch

import clip_oracle as CO
from conftest import relerr
from dbmm_amd import _lib, ops, synth

pytestmark = pytest.mark.gpu
DEV = "cuda"
E_SHAPE, E_ALIGN, E_WORKSPACE, E_ARG = -1, -2, -3, -4          # include/dbmm.h
P = "a."

# (C, H, W, heads, Dout, B)
ARCH = {
    "RN50": (2048, 7, 7, 32, 1024, 3),
    "RN101": (2048, 7, 7, 32, 512, 3),
    "RN50x4": (2560, 9, 9, 40, 640, 2),
    "RN50x16": (3072, 12, 12, 48, 768, 2),
    "RN50x64": (4096, 14, 14, 64, 1024, 1),
}
# token-count edges: (HW + 1) % 4 takes all four values, L lands on Lp (HW = 3, 15, 63, 127), L crosses the softmax kernel's 64 lanes
# both ways (63 / 64, 127 / 128), HW = 1 is the map whose mean is its only pixel
EDGE_HW = {1: (1, 1), 3: (1, 3), 4: (2, 2), 5: (1, 5), 6: (2, 3), 15: (3, 5), 63: (7, 9), 64: (4, 16), 127: (1, 127), 128: (8, 16)}


def _edge(hw):
    return (128,) + EDGE_HW[hw] + (2, 36, 3)


def _batch_edge(B):
    return (64, 1, 3, 1, 10, B)                # Dout = 10: the last GEMM leaves through the per-element epilogue


def _weights(C, L, Dout):
    """synth weights scaled as in test_gpu_kernels.py::test_attnpool"""
    sd = {P + "positional_embedding": synth.normal(1, "pos", (L, C), C ** -0.5)}
    for nm, o in (("q_proj", C), ("k_proj", C), ("v_proj", C), ("c_proj", Dout)):
        sd[P + nm + ".weight"] = synth.normal(2, nm, (o, C), C ** -0.5)
        sd[P + nm + ".bias"] = synth.normal(3, nm + "b", (o,), 0.1)
    return sd


class _Case:
    """one set of inputs with its float64 reference and the fp32 oracle's own err, computed once and never changed"""

    def __init__(self, shape, scale, f16, randn):
        C, H, W, heads, Dout, B = shape
        self.shape, self.heads = shape, heads
        self.sd = _weights(C, H * W + 1, Dout)
        if randn:
            x = torch.randn((B, C, H, W), generator=torch.Generator().manual_seed(4))
        else:
            x = synth.normal(4, "x", (B, C, H, W))
        x = x * scale
        if f16:
            x = x.half().float()
        self.x = x.permute(0, 2, 3, 1).contiguous()            # NHWC, what the kernel reads
        with torch.no_grad():
            self.ref = CO.attention_pool(x.double(), {k: v.double() for k, v in self.sd.items()}, P, heads)
            self.e32 = relerr(CO.attention_pool(x, self.sd, P, heads), self.ref)

    def args(self):
        d = {k: v.to(DEV) for k, v in self.sd.items()}
        return (d[P + "positional_embedding"], d[P + "q_proj.weight"], d[P + "q_proj.bias"],
                torch.cat([d[P + "k_proj.weight"], d[P + "v_proj.weight"]]).contiguous(),
                torch.cat([d[P + "k_proj.bias"], d[P + "v_proj.bias"]]).contiguous(), d[P + "c_proj.weight"], d[P + "c_proj.bias"], self.heads)

    def check(self, out, what):
        err = relerr(out.cpu(), self.ref)
        print(f"attnpool {what} {self.shape}: err {err:.2e}, fp32 oracle {self.e32:.2e}, ratio {err / max(self.e32, 1e-30):.2f}")
        assert out.shape == self.ref.shape and bool(torch.isfinite(out).all()), what
        assert err <= 4 * self.e32 and err < 1e-5, (what, err, self.e32)
        return err


@functools.lru_cache(maxsize=8)
def _case(shape, scale=1.0, f16=False, randn=False):
    return _Case(shape, scale, f16, randn)


def _run(case, x=None):
    return ops.attnpool(case.x.to(DEV) if x is None else x, *case.args())


class _Poisoned:
    """stand-in for ops._empty in the style of test_gpu_headline.GuardedAlloc / test_gpu_supcon._Guarded: every tensor sits between two
    sentinel-filled zones (2^18 elements: 128 rows of the widest row here, what a ragged tile that ignored M would write), and the
    payload, which torch.empty leaves as it finds it, is filled with `fill`"""
    G, S = 1 << 18, -7.0

    def __init__(self, fill):
        self.fill, self.bufs = fill, []

    def __call__(self, shape, device=None, dtype=torch.float32, **kw):
        shape = (shape,) if isinstance(shape, int) else tuple(shape)
        n = math.prod(shape)
        raw = torch.full((n + 2 * self.G,), self.S, device=device, dtype=dtype)
        raw[self.G:self.G + n] = self.fill
        self.bufs.append((raw, n))
        return raw[self.G:self.G + n].view(shape)

    def payload(self, i):
        raw, n = self.bufs[i]
        return raw[self.G:self.G + n]

    def check(self):
        assert self.bufs
        for raw, n in self.bufs:
            assert bool((raw[:self.G] == self.S).all()) and bool((raw[self.G + n:] == self.S).all()), \
                f"guard zone of a {n}-element tensor was written"


# ---- 1. the operator against float64 ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("arch", list(ARCH))
def test_head_shapes_of_every_architecture(arch):
    """The real head shapes: 32 / 40 / 48 / 64 heads (the 32 x 128 tile and the tiles the wider towers are routed to, batched), L = 50,
    82, 145, 197 (the softmax rows past 64 lanes), Lp - L = 2, 2, 3, 3 padded rows.
    Measured on an MI355X: err (ratio to the fp32 oracle's) RN50 2.35e-07 (0.53), RN101 2.76e-07 (0.51), RN50x4 2.22e-07 (0.52), RN50x16
    2.21e-07 (0.41), RN50x64 2.64e-07 (0.40).  The first run of this test, with the score product (K = C) summed in one fp32 chain,
    measured 1.10e-06 (2.49), 1.34e-06 (2.49), 1.34e-06 (3.15), 1.41e-06 (2.63), 1.77e-06 (2.64)."""
    case = _case(ARCH[arch])
    case.check(_run(case), arch)


@pytest.mark.parametrize("hw", list(EDGE_HW))
def test_token_count_edges(hw):
    """C = 128, 2 heads, Dout = 36, B = 3 on non-square maps of 1 .. 128 pixels.
    Measured on an MI355X: err (ratio) HW 1: 4.23e-07 (2.89), 3: 3.78e-07 (1.59), 4: 2.79e-07 (1.35), 5: 4.13e-07 (2.40), 6: 3.00e-07 (1.45),
    15: 2.57e-07 (1.16), 63: 2.74e-07 (1.07), 64: 3.32e-07 (1.51), 127: 4.54e-07 (1.55), 128: 3.03e-07 (1.12)."""
    case = _case(_edge(hw))
    case.check(_run(case), f"HW = {hw}")


@pytest.mark.parametrize("B", [1, 33, 130])
def test_batch_edges(B):
    """B is M in four of the GEMMs: 1 row, one row past the 32-row tile, two rows past the 128-row tile (C = 64, 1 head, HW = 3).
    Measured on an MI355X: err (ratio) B 1: 1.69e-07 (0.98), 33: 3.15e-07 (1.73), 130: 2.68e-07 (1.49)."""
    case = _case(_batch_edge(B))
    case.check(_run(case), f"B = {B}")


def test_batch_at_the_grid_limit():
    """B = 65535, the largest batch the entry takes (one grid row per image in the token kernel and per problem in two of the batched
    GEMMs); torch.randn inputs.
    Measured on an MI355X: err 4.94e-07, ratio 1.59; 0.25 s."""
    case = _case(_batch_edge(65535), randn=True)
    case.check(_run(case), "B = 65535")


def test_batch_past_the_grid_limit_raises(monkeypatch):
    """B = 65536 raises through ops.attnpool and launches nothing: the output and the workspace keep what they were filled with"""
    C, H, W, heads, Dout, B = _batch_edge(65536)
    case = _case(_batch_edge(1))
    x = torch.zeros((B, H, W, C), device=DEV)
    ga = _Poisoned(5.0)
    monkeypatch.setattr(ops, "_empty", ga)
    with pytest.raises(_lib.DbmmError):
        ops.attnpool(x, *case.args())
    torch.cuda.synchronize()
    assert len(ga.bufs) == 2
    ga.check()
    assert bool((ga.payload(0) == 5.0).all()) and bool((ga.payload(1) == 5.0).all())


PEAKED = [("RN50", ARCH["RN50"], 4.0), ("RN50", ARCH["RN50"], 12.0), ("HW = 128", _edge(128), 4.0), ("HW = 128", _edge(128), 30.0)]


@pytest.mark.parametrize("name,shape,scale", PEAKED)
def test_peaked_and_saturated_attention(name, shape, scale):
    """The feature map times 4 (largest attention weight 0.92 at the RN50 shape, against 0.036 for unit-scale inputs) and scaled until
    the weights saturate and expf underflows: an error in one score is no longer averaged away over near-uniform weights.
    The saturated RN50 case runs at x 12, not x 30.  At x 30 the scores reach 10^3, one fp32 rounding of a score is 1e-4 in the
    exponent, and the fp32 oracle itself measured 1.25e-5 from float64 on the test machine's CPU: no fp32 evaluation meets the 1e-5
    cap on those inputs (this operator measured 4.0e-5, ratio 3.19).  That is a property of the inputs.  At x 12, 45 of the 96 rows
    have a weight above 0.999, 54 of the 4800 exponentials underflow to zero and 219 more are denormal, and the oracle leaves room
    under the cap; x 30 stays on the small shape, whose scores are smaller.
    Measured on an MI355X: err (ratio) RN50 x 4: 8.29e-07 (0.72; 2.93e-06 (2.54) with the score product in one chain), RN50 x 12: 2.09e-06
    (0.70, the oracle 3.00e-06), HW = 128 x 4: 9.74e-07 (1.62), HW = 128 x 30: 9.58e-07 (1.21)."""
    case = _case(shape, scale=scale)
    case.check(_run(case), f"{name} x {scale:g}")


@pytest.mark.parametrize("name,shape", [("RN50", ARCH["RN50"])] + [(f"HW = {hw}", _edge(hw)) for hw in EDGE_HW])
def test_poisoned_workspace(name, shape, monkeypatch):
    """The workspace and the output arrive filled with NaN instead of whatever torch.empty finds: a padded token row that is not written,
    or a padded probability that is not zero, then contributes 0 * NaN.  The result is finite, within the bound and bit-equal to a run
    on a zero-filled workspace; the guard zones around both tensors are intact; the workspace is dbmm_workspace_bytes_attnpool long.
    Measured on an MI355X: the errs of test_head_shapes_of_every_architecture[RN50] and test_token_count_edges, digit for digit."""
    C, H, W, heads, Dout, B = shape
    case = _case(shape)
    x, args = case.x.to(DEV), case.args()
    outs = []
    for fill in (float("nan"), 0.0):
        ga = _Poisoned(fill)
        monkeypatch.setattr(ops, "_empty", ga)
        outs.append(ops.attnpool(x, *args))
        torch.cuda.synchronize()
        assert len(ga.bufs) == 2
        ga.check()
        assert ga.bufs[0][1] * 4 == _lib.lib().dbmm_workspace_bytes_attnpool(B, H * W, C)
    case.check(outs[0], f"{name}, NaN-filled workspace")
    assert torch.equal(outs[0], outs[1])


@pytest.mark.parametrize("name,shape", [("RN50", ARCH["RN50"]), ("HW = 6", _edge(6))])
def test_f16_feature_map(name, shape):
    """dbmm_attnpool_x with x_is_f16 = 1 reads the fp16 map directly: bit-equal to the same call on xh.float(), both within the bound of
    the float64 result on xh.
    Measured on an MI355X: err (ratio) RN50 2.56e-07 (0.48), HW = 6 3.17e-07 (1.29), the same for both calls."""
    case = _case(shape, f16=True)
    xh = case.x.to(DEV).half()
    assert torch.equal(xh.float().cpu(), case.x)
    out_h, out_f = _run(case, xh), _run(case, xh.float())
    case.check(out_h, f"{name}, fp16 map")
    case.check(out_f, f"{name}, the fp16 map cast to fp32")
    assert torch.equal(out_h, out_f)


@pytest.mark.parametrize("name,shape", [("RN50", ARCH["RN50"]), ("HW = 128", _edge(128))])
def test_two_calls_same_bits(name, shape):
    case = _case(shape)
    assert torch.equal(_run(case), _run(case))


def test_refusals_launch_nothing():
    """each refusal returns the code include/dbmm.h names; the output keeps its sentinel"""
    C, H, W, heads, Dout, B = shape = _edge(5)
    HW = H * W
    case = _case(shape)
    pos, wq, bq, wkv, bkv, wc, bc, _ = case.args()
    x = case.x.to(DEV)
    L = _lib.lib()
    nbytes = L.dbmm_workspace_bytes_attnpool(B, HW, C)
    ws = torch.zeros(nbytes // 4, device=DEV)
    out = torch.full((B, Dout), 9.0, device=DEV)
    pos_off = torch.zeros(pos.numel() + 4, device=DEV)          # the same table 4 bytes past a 16-byte boundary
    pos_off[1:1 + pos.numel()] = pos.flatten()

    def call(x=x.data_ptr(), pos=pos.data_ptr(), heads=heads, nbytes=nbytes):
        return L.dbmm_attnpool(x, pos, wq.data_ptr(), bq.data_ptr(), wkv.data_ptr(), bkv.data_ptr(), wc.data_ptr(), bc.data_ptr(),
                               out.data_ptr(), B, HW, C, heads, Dout, ws.data_ptr(), nbytes, _lib.stream())

    assert call(nbytes=nbytes - 1) == E_WORKSPACE
    assert call(heads=heads + 1) == E_SHAPE                     # C != heads * 64
    assert call(x=None) == E_ARG
    assert call(pos=pos_off.data_ptr() + 4) == E_ALIGN
    torch.cuda.synchronize()
    assert bool((out == 9.0).all())
    assert call() == 0                                          # the same arguments unaltered are served
    case.check(out, "raw entry")


# ---- 2. dbmm_gemm_batched directly -----------------------------------------------------------------------------------------------------
SENT = -7.0
PAD = 4096                                                       # NaN / sentinel elements before and after every view


def _act(v, act):
    return {0: v, 1: torch.relu(v), 2: v * torch.sigmoid(1.702 * v)}[act]


def _place(data, strides, fill):
    """data [nb][rows][cols] as a strided view (element strides) inside a buffer of `fill`, PAD elements from either end; a stride of 0
    along the batch places problem 0 once.  Returns (buffer, view)."""
    if strides[0] == 0:
        data = data[:1]
    extent = sum((n - 1) * s for n, s in zip(data.shape, strides)) + 1
    buf = torch.full((extent + 2 * PAD,), fill, device=DEV)
    view = buf.as_strided(tuple(data.shape), strides, PAD)
    view.copy_(data.to(DEV))
    return buf, view


def _batched(M, N, K, nb, ta=0, tw=0, *, lda=None, sa=None, ldw=None, sw=None, ldc=None, sc=None, bias=False, sbias=None, alpha=1.0,
             act=0, seed=0, what=""):
    """one dbmm_gemm_batched call between moats, checked against float64; returns (err, fp32 matmul's err, igemm tag).
    Default strides leave NaN between the rows of an operand and between problems."""
    a = synth.normal(10 + seed, "gb_a", (nb, M, K))
    w = synth.normal(20 + seed, "gb_w", (1 if sw == 0 else nb, N, K), K ** -0.5)
    b = synth.normal(30 + seed, "gb_b", (1 if sbias == 0 else nb, N), 0.5) if bias else None
    ar, ac = (K, M) if ta else (M, K)
    wr, wc = (K, N) if tw else (N, K)
    lda = ac + 8 if lda is None else lda
    ldw = wc + 4 if ldw is None else ldw
    ldc = (N + 4) // 4 * 4 + 4 if ldc is None else ldc
    sa = ar * lda + 12 if sa is None else sa
    sw = wr * ldw + 8 if sw is None else sw
    sc = M * ldc + 4 if sc is None else sc
    sbias = (N + 7) // 4 * 4 if sbias is None else sbias
    abuf, _ = _place(a.transpose(1, 2) if ta else a, (sa, lda, 1), float("nan"))
    wbuf, _ = _place(w.transpose(1, 2) if tw else w, (sw, ldw, 1), float("nan"))
    bbuf = _place(b[:, None, :], (sbias, 0, 1), float("nan"))[0] if bias else None
    cbuf, cview = _place(torch.full((nb, M, N), SENT), (sc, ldc, 1), SENT)
    el = 4
    rc = _lib.lib().dbmm_gemm_batched(abuf.data_ptr() + PAD * el, lda, sa, ta, wbuf.data_ptr() + PAD * el, ldw, sw, tw,
                                      bbuf.data_ptr() + PAD * el if bias else None, sbias if bias else 0, cbuf.data_ptr() + PAD * el, ldc, sc,
                                      M, N, K, nb, alpha, act, _lib.stream())
    assert rc == 0, (what, rc)
    tag = ops._last_igemm_tag()
    torch.cuda.synchronize()
    out = cview.clone().cpu()
    cview.fill_(SENT)
    assert bool((cbuf == SENT).all()), f"{what}: written outside the {nb} x {M} x {N} outputs"
    ref = torch.einsum("bmk,bnk->bmn", a.double(), w.double().expand(nb, N, K))
    f32 = torch.matmul(a, w.expand(nb, N, K).transpose(1, 2))
    if bias:
        ref = ref + b.double().expand(nb, N)[:, None, :]
        f32 = f32 + b.expand(nb, N)[:, None, :]
    ref, f32 = _act(ref * alpha, act), _act(f32 * alpha, act)
    err, e32 = relerr(out, ref), relerr(f32, ref)
    print(f"gemm_batched {what} (M {M}, N {N}, K {K}, batch {nb}, trans {ta}{tw}) {tag}: err {err:.2e}, fp32 matmul {e32:.2e}, "
          f"ratio {err / max(e32, 1e-30):.2f}")
    assert bool(torch.isfinite(out).all()), f"{what}: NaN from outside an operand reached an output"
    assert err <= 4 * e32, (what, err, e32)
    return err, e32, tag


def _tile(tag):
    """(BM, BN, FAST) of an igemm_f32_kernel<BM, BN, WAVES_M, WAVES_N, AMODE, WMODE, BK, MINB, FAST, SK, DMA> tag"""
    assert tag.startswith("igemm_f32_kernel<"), tag
    v = [int(t) for t in tag[len("igemm_f32_kernel<"):-1].split(", ")]
    return v[0], v[1], v[8]


def test_the_four_products_of_the_attention_pool():
    """the four dbmm_gemm_batched calls of dbmm_attnpool_x at RN50 size (C = 2048, 32 heads, HW = 49, Lp = 52) and B = 3, with the strides
    of csrc/resnet_ops.hip: the slices and interleaved outputs leave no gap between rows there, the moats are past the ends.
    Measured on an MI355X: err (ratio to fp32 matmul's) U 3.06e-07 (2.17), S 2.80e-07 (0.99), Sx 3.28e-07 (1.18), o 2.08e-07 (0.47); all four
    on the 32 x 128 tile.  With one fp32 chain over K = 2048 the score product S measured 1.51e-06 (5.33) and failed here."""
    C, heads, B, Lp = 2048, 32, 3, 52
    # U[b][h][:] = Wk_h^T q_h: A a 64-column slice of a row of q, W the k rows of head h K-major, C interleaved by head
    _batched(B, C, 64, heads, 0, 1, lda=C, sa=64, ldw=C, sw=64 * C, ldc=heads * C, sc=C, what="U = Wk^T q")
    # S[b][h][j] = U[b][h] . t[b][j]
    _batched(heads, Lp, C, B, 0, 0, lda=C, sa=heads * C, ldw=C, sw=Lp * C, ldc=Lp, sc=heads * Lp, what="S = U t^T")
    # Sx[b][h][:] = sum_j p[b][h][j] t[b][j][:]: K = 52 is no multiple of the 16-deep chunk
    _batched(heads, C, Lp, B, 0, 1, lda=Lp, sa=heads * Lp, ldw=C, sw=Lp * C, ldc=C, sc=heads * C, what="Sx = P t")
    # o[:, 64h:64h+64] = Sx[:, h, :] Wv_h^T + bv_h
    _batched(B, 64, C, heads, 0, 0, lda=heads * C, sa=C, ldw=C, sw=64 * C, ldc=C, sc=64, bias=True, sbias=64, what="o = Sx Wv^T + bv")


def test_every_tile_route_and_both_loaders():
    """one batched case per tile route of launch_modes; K % 16 != 0 takes the generic loader, the others the buffer-descriptor one.
    A routing change that empties this matrix fails here.
    Measured on an MI355X: err (ratio) 32 x 128: 1.23e-07 (1.64), 128 x 32: 1.84e-07 (1.00), 128 x 64: 2.20e-07 (1.00), 64 x 64: 2.57e-07 (0.85),
    128 x 128: 2.93e-07 (1.08).  With one fp32 chain over K = 2560 the 64 x 64 case measured 1.82e-06 (6.04) and failed here."""
    routes = [((32, 33, 16, 2), (32, 128)),            # N tail, N % 4 != 0: per-element epilogue
              ((130, 24, 36, 3), (128, 32)),           # K % 16 != 0: the generic loader
              ((130, 64, 48, 5), (128, 64)),
              ((40, 84, 2560, 2), (64, 64)),           # RN50x4's score product
              ((40, 200, 64, 96), (128, 128))]         # 192 tiles
    seen, loaders = set(), set()
    for i, ((M, N, K, nb), want) in enumerate(routes):
        _, _, tag = _batched(M, N, K, nb, seed=i, what=f"tile {want[0]} x {want[1]}")
        bm, bn, fast = _tile(tag)
        assert (bm, bn) == want, tag
        seen.add((bm, bn)); loaders.add(fast)
    assert seen == {(32, 128), (128, 32), (128, 64), (64, 64), (128, 128)}
    assert loaders == {0, 1}


@pytest.mark.parametrize("M,N,K,nb,ta,tw", [(64, 100, 20, 4, 1, 0), (32, 128, 12, 7, 1, 1)])
def test_trans_a_modes(M, N, K, nb, ta, tw):
    """the two modes with a K-major A, which no caller in the library reaches.
    Measured on an MI355X: err (ratio) 1.42e-07 (1.00) and 9.18e-08 (0.74)."""
    _batched(M, N, K, nb, ta, tw, bias=True, what="K-major A")


@pytest.mark.parametrize("act", [0, 1, 2])
def test_epilogue_alpha_bias_activation(act):
    """act(alpha * (a w^T + bias)) with alpha = 0.125, through the 16-byte (N = 64) and the per-element (N = 50) epilogue.
    Measured on an MI355X: err (ratio), N = 64 / N = 50: none 1.84e-07 (1.00) / 1.96e-07 (1.00), ReLU 1.84e-07 (1.00) / 1.48e-07 (1.00), QuickGELU
    1.65e-07 (0.91) / 1.86e-07 (1.07)."""
    _batched(70, 64, 32, 3, alpha=0.125, bias=True, act=act, what=f"act {act}, N % 4 == 0")
    _batched(70, 50, 32, 3, alpha=0.125, bias=True, act=act, seed=1, what=f"act {act}, N % 4 != 0")


def test_shared_weight_and_bias():
    """stride_w = 0 and stride_bias = 0: one weight and one bias for every problem.
    Measured on an MI355X: err 1.82e-07, ratio 1.17."""
    _batched(36, 72, 32, 6, sw=0, bias=True, sbias=0, what="stride_w = stride_bias = 0")


def test_batch_of_65535():
    """the largest batch the entry takes, of 4 x 4 x 4 problems.
    Measured on an MI355X: err 9.89e-08, ratio 0.93."""
    _batched(4, 4, 4, 65535, bias=True, what="batch 65535")


def test_gemm_batched_refusals_launch_nothing():
    """each refusal returns the code include/dbmm.h names and the output keeps its sentinel.  Every batch stride is 0 and the buffers are
    far larger than the problem, so the arguments are harmless even to an entry that did not refuse them."""
    L = _lib.lib()
    a = torch.ones(4096, device=DEV); w = torch.ones(4096, device=DEV); b = torch.ones(4096, device=DEV)
    c = torch.full((4096,), SENT, device=DEV)
    base = dict(a=a.data_ptr(), lda=8, sa=0, ta=0, w=w.data_ptr(), ldw=8, sw=0, tw=0, bias=b.data_ptr(), sbias=0, c=c.data_ptr(), ldc=8,
                sc=0, M=8, N=8, K=8, batch=2, alpha=1.0, act=0)

    def call(**over):
        v = dict(base, **over)
        return L.dbmm_gemm_batched(v["a"], v["lda"], v["sa"], v["ta"], v["w"], v["ldw"], v["sw"], v["tw"], v["bias"], v["sbias"], v["c"],
                                   v["ldc"], v["sc"], v["M"], v["N"], v["K"], v["batch"], v["alpha"], v["act"], _lib.stream())

    assert call(batch=0) == E_SHAPE
    assert call(batch=65536) == E_SHAPE
    assert call(lda=6) == E_ALIGN
    assert call(K=6) == E_SHAPE                                  # K % 4 != 0 without trans_a
    assert call(ta=1, M=6) == E_SHAPE                            # M % 4 != 0 with trans_a
    assert call(act=3) == E_ARG
    for name in ("a", "w", "c"):
        assert call(**{name: None}) == E_ARG
    # the epilogue stores C and loads the bias 16 bytes at a time when N and ldc are multiples of 4: every problem's c and bias start on
    # a 16-byte boundary, as the header's "multiples of 4" asks of all four strides
    assert call(sc=6) == E_ALIGN
    assert call(sbias=2) == E_ALIGN
    assert call(c=c.data_ptr() + 4) == E_ALIGN
    assert call(bias=b.data_ptr() + 8) == E_ALIGN
    assert call(ldc=4) == E_SHAPE                                # ldc < N: rows would overlap
    torch.cuda.synchronize()
    assert bool((c == SENT).all())
    assert call() == 0
    torch.cuda.synchronize()
    assert bool((c[:64].view(8, 8) == 9.0).all()) and bool((c[64:] == SENT).all())
