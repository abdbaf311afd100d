"""The layout and reduction kernels between the GEMMs, each against a plain reference of its own: the fp16 / fp32 patch gather, token
assembly, embedding gather and EOT gather of the ViT and text towers (csrc/f16_ops.hip, csrc/transformer_ops.hip), avgpool2_f16
(csrc/conv_f16.hip), cast_f32_f16, and gather_rows / colsum / l2norm_rows / group_loss_sum / group_count (csrc/adapter_ops.hip).

These kernels copy, or round once, or sum small integers: wherever the operation is exact the comparison is torch.equal.  The two float
reductions (colsum on random floats, l2norm_rows) are held to the error of the same expression evaluated by torch in float32, both
measured against float64: e_kernel <= 4 * e_torch + 2^-23 (another, equally valid summation order; the floor is for an exact torch).

A "guard zone": the C entry is called through _lib.lib() on a buffer pre-filled with 7.0 that is 4096 elements longer than the output,
and the tail must still be 7.0.  "Past the block cap": the launchers' grid_for() stops at 16384 blocks of 256 threads (8192 in
adapter_ops.hip), so more than 16384 * 256 work items -- VEC-pixel vectors, float4s or elements, as the launcher counts them -- is
what makes the grid-stride loops take a second trip.  Each such case states and asserts its count."""
import pytest
import torch
import torch.nn.functional as F

from conftest import relerr
from dbmm_amd import _lib, ops, synth

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD, FILL = 4096, 7.0
CAP = 16384 * 256                                              # work items one pass of a capped grid covers (grid_for, 256 threads per block)
F32, F16, I32, I64 = torch.float32, torch.float16, torch.int32, torch.int64


def gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


def randn(seed, *shape, dtype=F32):
    return torch.randn(shape, device=DEV, generator=gen(seed)).to(dtype)


def randint(seed, lo, hi, *shape, dtype=I64):
    return torch.randint(lo, hi, shape, device=DEV, generator=gen(seed)).to(dtype)


def guarded(n, dtype):
    return torch.full((n + GUARD,), FILL, device=DEV, dtype=dtype)


def guard_intact(buf, n):
    return bool((buf[n:] == FILL).all()) and buf.numel() == n + GUARD


def call(name, *args):
    """a C entry on the current stream; its return code must be DBMM_OK"""
    rc = getattr(_lib.lib(), name)(*[a.data_ptr() if isinstance(a, torch.Tensor) else a for a in args], _lib.stream())
    assert rc == 0, (name, rc)


def bits(t):
    """fp16 payloads as integers: tells -0 from +0, which torch.equal on the floats does not"""
    return t.contiguous().view(torch.int16)


# ---- patch gather --------------------------------------------------------------------------------------------------------------------

def patch_ref(x, P):
    """[B, 3, R, R] -> [B * g * g, 3 * P * P] float32 rows in (channel, kh, kw) order, patches row-major (as test_im2col_patch_and_tokens)"""
    B, _, R, _ = x.shape
    g = R // P
    return F.unfold(x.float(), P, stride=P).transpose(1, 2).reshape(B * g * g, 3 * P * P)


def im2col_f16_raw(x, P, Kp):
    B, _, R, _ = x.shape
    rows = B * (R // P) ** 2
    buf = guarded(rows * Kp, F16)
    call("dbmm_im2col_patch_f16", x, int(x.dtype == F16), buf, B, R, P, Kp)
    return buf, rows


@pytest.mark.parametrize("pad", ["K", "K_up_to_64", "K_plus_64"])
@pytest.mark.parametrize("R,P,vec", [(64, 32, 4), (28, 14, 2), (21, 7, 1)])
@pytest.mark.parametrize("dtype", [F32, F16], ids=["x_f32", "x_f16"])
def test_im2col_patch_f16(dtype, R, P, vec, pad):
    """every VEC instantiation (P % 4 == 0, P % 2 == 0, odd P) for both input types: columns [:K] are the image rounded once to fp16,
    columns [K:] exactly zero (on a buffer that held 7.0 there: the wrapper's allocation could hold zeros by luck), nothing behind"""
    B, K = 3, 3 * P * P
    assert vec == (4 if P % 4 == 0 else 2 if P % 2 == 0 else 1)
    Kp = {"K": K, "K_up_to_64": (K + 63) // 64 * 64, "K_plus_64": K + 64}[pad]
    x = randn(R + P, B, 3, R, R, dtype=dtype)
    buf, rows = im2col_f16_raw(x, P, Kp)
    out = buf[:rows * Kp].view(rows, Kp)
    assert torch.equal(out[:, :K], patch_ref(x.half(), P).half())
    assert bool((bits(out[:, K:]) == 0).all()), "pad columns must be +0"
    assert guard_intact(buf, rows * Kp)
    if Kp % 8 == 0:                                            # what the wrapper accepts: the same bytes
        assert torch.equal(ops.im2col_patch_f16(x, P, Kp), out)


def test_im2col_patch_f16_past_the_block_cap():
    B, R, P, VEC = 112, 224, 32, 4
    n_vec = B * 3 * R * (R // VEC)                             # 4,214,784 four-pixel vectors
    assert n_vec == 4214784 and n_vec > CAP
    K = Kp = 3 * P * P
    x = randn(1, B, 3, R, R, dtype=F16)
    buf, rows = im2col_f16_raw(x, P, Kp)
    assert torch.equal(buf[:rows * Kp].view(rows, Kp), patch_ref(x, P).half()) and guard_intact(buf, rows * Kp)


@pytest.mark.parametrize("B,R,P,n_vec", [(3, 21, 7, 3 * 3 * 21 * 21), (112, 224, 32, 4214784)], ids=["vec1", "past_cap"])
def test_im2col_patch_f32(B, R, P, n_vec):
    """the VEC == 1 instantiation (odd P) and a second trip of the grid-stride loop: an exact copy, and max|x| beside it"""
    vec = 4 if P % 4 == 0 else 2 if P % 2 == 0 else 1
    assert n_vec == B * 3 * R * (R // vec) and (n_vec > CAP) == (B == 112)
    x = randn(2, B, 3, R, R)
    rows, K = B * (R // P) ** 2, 3 * P * P
    buf = guarded(rows * K, F32)
    am = torch.zeros(1, device=DEV)
    call("dbmm_im2col_patch", x, buf, am, B, R, P)
    ref = patch_ref(x, P)
    assert torch.equal(buf[:rows * K].view(rows, K), ref) and guard_intact(buf, rows * K)
    assert am.item() == x.abs().max().item()
    assert torch.equal(ops.im2col_patch(x, P), ref)


def test_im2col_patch_absmax():
    """out_absmax is a running maximum of |x|: a negative extreme counts, a larger value already there stays, a smaller one rises"""
    x = randn(3, 2, 3, 28, 28)
    x[1, 2, 27, 26] = -50.0
    assert x.abs().max().item() == 50.0 and x.max().item() < 50.0
    for start, want in ((0.0, 50.0), (100.0, 100.0), (1.0, 50.0)):
        am = torch.full((1,), start, device=DEV)
        ops.im2col_patch(x, 14, out_absmax=am)
        assert am.item() == want, (start, am.item())


# ---- token assembly --------------------------------------------------------------------------------------------------------------------

def tokens_ref(patches, cls, pos, B):
    L, W = pos.shape
    t = torch.cat([cls.expand(B, 1, W), patches.float().view(B, L - 1, W)], 1)
    return t + pos


def vit_tokens_case(seed, B, L, W, f16):
    patches = randn(seed, B * (L - 1), W, dtype=F16 if f16 else F32)
    cls, pos = randn(seed + 1, W), randn(seed + 2, L, W)
    ref = tokens_ref(patches, cls, pos, B)
    return patches, cls, pos, (ref.half() if f16 else ref)


@pytest.mark.parametrize("B,L,W", [(1, 2, 64), (3, 17, 128), (2, 50, 100)])
@pytest.mark.parametrize("f16", [True, False], ids=["f16", "f32"])
def test_vit_tokens(f16, B, L, W):
    """(class token | patches) + positional table, in fp32; the f16 kernel rounds once.  Every image gets the same `pos`, row l to row l."""
    patches, cls, pos, ref = vit_tokens_case(10, B, L, W, f16)
    buf = guarded(B * L * W, F16 if f16 else F32)
    call("dbmm_vit_tokens_f16" if f16 else "dbmm_vit_tokens", patches, cls, pos, buf, B, L, W)
    assert torch.equal(buf[:B * L * W].view(B, L, W), ref) and guard_intact(buf, B * L * W)
    assert torch.equal((ops.vit_tokens_f16 if f16 else ops.vit_tokens)(patches, cls, pos, B), ref)


@pytest.mark.parametrize("f16,B", [(True, 8), (False, 32)], ids=["f16", "f32"])
def test_vit_tokens_past_the_block_cap(f16, B):
    L, W = 577, 1024
    items = B * L * W if f16 else B * L * (W // 4)             # f16: one element per thread; fp32: one float4
    assert items == 4726784 and items > CAP
    patches, cls, pos, ref = vit_tokens_case(11, B, L, W, f16)
    assert torch.equal((ops.vit_tokens_f16 if f16 else ops.vit_tokens)(patches, cls, pos, B), ref)


# ---- embedding gather --------------------------------------------------------------------------------------------------------------------

VOCAB = 100


def embed_case(seed, n, L, W):
    tok = randint(seed, 0, VOCAB, n, L, dtype=I32)
    tok[0, 3], tok[n - 1, L - 1], tok[0, 0], tok[n - 1, 7] = -5, VOCAB + 7, 0, VOCAB - 1
    table, pos = randn(seed + 1, VOCAB, W), randn(seed + 2, L, W)
    ref = table[tok.long().clamp(0, VOCAB - 1)] + pos          # ids outside the table take its first / last row, never a stray read
    assert torch.equal(ref[0, 3], table[0] + pos[3]) and torch.equal(ref[n - 1, L - 1], table[VOCAB - 1] + pos[L - 1])
    return tok, table, pos, ref


@pytest.mark.parametrize("n,L,W,f16,items", [(1, 77, 64, True, None), (5, 77, 512, True, None), (1, 77, 64, False, None),
                                             (5, 77, 512, False, None), (128, 77, 512, True, 128 * 77 * 512),
                                             (512, 77, 512, False, 512 * 77 * 128)])
def test_embed_gather(n, L, W, f16, items):
    """table[token] + pos in fp32 (the f16 kernel rounds once), ids -5 and vocab + 7 clamped into the table; the last two shapes are
    past the block cap: 5,046,272 elements (f16) / float4s (fp32)"""
    if items is not None:
        assert items == 5046272 and items > CAP
    tok, table, pos, ref = embed_case(20, n, L, W)
    out, tok_back = (ops.embed_gather_f16 if f16 else ops.embed_gather)(tok, table, pos)
    assert out.dtype == (F16 if f16 else F32) and torch.equal(out, ref.half() if f16 else ref)
    assert torch.equal(tok_back, tok)
    if items is None:
        buf = guarded(n * L * W, out.dtype)
        call("dbmm_embed_gather_f16" if f16 else "dbmm_embed_gather", tok, table, pos, buf, n, L, W, VOCAB)
        assert torch.equal(buf[:n * L * W].view(n, L, W), out) and guard_intact(buf, n * L * W)


# ---- EOT gather ------------------------------------------------------------------------------------------------------------------------

def first_argmax(tok):
    """index of the first occurrence of each row's maximum, spelled out (no reliance on a library's tie rule)"""
    L = tok.shape[1]
    is_max = tok == tok.max(1, keepdim=True).values
    return torch.where(is_max, torch.arange(L, device=tok.device), L).min(1).values


def eot_rows_77():
    """L = 77 is two candidates for lanes 0..12 and one for the rest: (tokens, expected index, what the row is about)"""
    L = 77
    rows = []
    for p in (0, 63, 64, 76):
        t = randint(30 + p, 0, 100, L); t[p] = 1000
        rows.append((t, p, f"maximum at {p}"))
    for a, b, want in ((5, 69, 5), (10, 40, 10), (70, 3, 3)):
        t = randint(40 + a, 0, 100, L); t[a] = 1000; t[b] = 1000
        rows.append((t, want, f"maximum at {a} and {b}"))
    rows.append((torch.full((L,), 49407, device=DEV), 0, "all ids equal"))
    t = randint(50, -1000, -1, L); t[33] = -1
    rows.append((t, 33, "all ids negative"))
    return rows


@pytest.mark.parametrize("W", [8, 64, 100])
@pytest.mark.parametrize("f16", [True, False], ids=["f16", "f32"])
def test_gather_eot(f16, W):
    """out[i] = x[i, first index of max(tokens[i])], bit for bit: hand-placed maxima and ties at L = 77 (within a lane, across lanes,
    the later lane holding the earlier index), L = 1, L = 200, and 300 rows of ids drawn from ten values (ties everywhere)"""
    dtype = F16 if f16 else F32
    entry, wrapper = ("dbmm_gather_eot_f16", ops.gather_eot_f16) if f16 else ("dbmm_gather_eot", ops.gather_eot)
    hand = eot_rows_77()
    cases = [(torch.stack([t for t, _, _ in hand]).to(I32), torch.tensor([w for _, w, _ in hand], device=DEV), [s for _, _, s in hand])]
    for n, L, hi in ((4, 1, 100), (9, 200, 100000), (9, 200, 10), (300, 77, 10)):
        cases.append((randint(60 + L + hi, 0, hi, n, L, dtype=I32), None, None))
    for tok, want, names in cases:
        n, L = tok.shape
        idx = first_argmax(tok)
        if want is not None:
            assert torch.equal(idx, want)                      # the reference itself, on the rows whose answer is known by construction
        x = randn(70 + L, n, L, W, dtype=dtype)
        ref = x[torch.arange(n, device=DEV), idx]
        buf = guarded(n * W, dtype)
        call(entry, tok, x, buf, n, L, W)
        got = buf[:n * W].view(n, W)
        bad = (got != ref).any(1).nonzero().flatten().tolist()
        assert not bad, [(names[i] if names else f"row {i} of {n} x {L}") for i in bad]
        assert guard_intact(buf, n * W)
        assert torch.equal(wrapper(tok, x), ref)


# ---- avgpool2_f16 ------------------------------------------------------------------------------------------------------------------------

def avgpool_ref(x):
    """fp32 sum of the window in (dy, dx) order, times 0.25, one rounding: sequential IEEE adds, so exact"""
    f = x.float()
    s = f[:, 0::2, 0::2] + f[:, 0::2, 1::2]
    s = s + f[:, 1::2, 0::2]
    s = s + f[:, 1::2, 1::2]
    return (s * 0.25).half()


def avgpool_check(x):
    B, H, W, C = x.shape
    n = B * (H // 2) * (W // 2) * C
    buf = guarded(n, F16)
    call("dbmm_avgpool2_f16", x, buf, B, H, W, C)
    ref = avgpool_ref(x)
    assert torch.equal(bits(buf[:n].view(ref.shape)), bits(ref)) and guard_intact(buf, n)
    assert torch.equal(ops.avgpool2_f16(x), ref)
    return ref


@pytest.mark.parametrize("B,H,W,C", [(1, 2, 2, 8), (3, 6, 10, 24), (2, 14, 14, 2048), (5, 4, 2, 64)])
def test_avgpool2_f16(B, H, W, C):
    """the kernel the pooled chain and streaming kernels are held bit-equal to, itself bit-equal to its definition, and within the
    suite's bound (test_stem_and_avgpool_f16) of float64 avg_pool2d"""
    x = randn(80 + C, B, H, W, C, dtype=F16)
    ref = avgpool_check(x)
    ref64 = F.avg_pool2d(x.double().permute(0, 3, 1, 2), 2).permute(0, 2, 3, 1)
    assert relerr(ref, ref64) < 1e-3


def test_avgpool2_f16_sums_in_fp32_in_window_order():
    # four inputs of 60000: an fp16 sum overflows, the fp32 sum of 240000 comes back as 60000
    x = torch.full((2, 4, 6, 16), 60000.0, device=DEV, dtype=F16)
    ref = avgpool_check(x)
    assert bool((ref == 60000.0).all())
    # magnitudes 2^14 apart inside a window: x00 ~ 2^14, x11 ~ -x00, the other two ~ 1.  The fp32 sum rounds at 2^-9 while the big terms
    # are in it, so the order of the adds decides the last bits of a result of about 0.5 (fp16 ulp 2^-11 after the 0.25)
    B, H, W, C = 2, 8, 8, 64
    x = randn(90, B, H, W, C, dtype=F16)
    big = (torch.rand((B, H // 2, W // 2, C), device=DEV, generator=gen(91)) + 1.0) * 2.0 ** 14       # [2^14, 2^15): finite in fp16
    x[:, 0::2, 0::2] = big.half()
    x[:, 1::2, 1::2] = -big.half()
    ref = avgpool_check(x)
    f = x.float()
    other = (((f[:, 1::2, 1::2] + f[:, 0::2, 0::2]) + f[:, 0::2, 1::2]) + f[:, 1::2, 0::2]) * 0.25
    assert bool((other.half() != ref).any()), "this input must tell the (dy, dx) order from another one"


def test_avgpool2_f16_refusals():
    z = lambda *s: torch.zeros(s, device=DEV, dtype=F16)
    for shape in ((1, 3, 4, 8), (1, 4, 3, 8), (1, 4, 4, 12), (1, 4, 4, 4)):
        with pytest.raises(RuntimeError, match="avgpool2_f16"):
            ops.avgpool2_f16(z(*shape))
    torch.cuda.synchronize()


# ---- cast --------------------------------------------------------------------------------------------------------------------------------

def test_cast_f32_f16():
    """x.half() bit for bit: round to nearest even into inf, into the fp16 subnormals and to signed zeros; past the block cap"""
    n = CAP + 77
    assert n == 4194381 and n > CAP
    x = randn(100, n) * torch.pow(10.0, torch.rand(n, device=DEV, generator=gen(101)) * 14 - 9)      # 1e-9 .. 1e5: subnormals to overflow
    edge = [0.0, -0.0, 65504.0, 65519.99, 65520.0, -65520.0, 1e5, -1e5, float("inf"), float("-inf"), 2.0 ** -24, 2.0 ** -25, -2.0 ** -25,
            2.0 ** -25 * 1.0001, 3 * 2.0 ** -25, 2.0 ** -14, 2.0 ** -14 - 2.0 ** -26, 1023.5 * 2.0 ** -24, 1e-40, -1e-40, 1.0 + 2.0 ** -11,
            1.0 + 3 * 2.0 ** -11, 2049.0, 2051.0]
    x[:len(edge)] = torch.tensor(edge, device=DEV)
    x[-len(edge):] = torch.tensor(edge, device=DEV)            # the same values in the loop's second trip
    ref = x.half()
    assert bool(ref.isinf().sum() > 8) and bool(((ref != 0) & (ref.abs() < 2.0 ** -14)).sum() > 1000)
    buf = guarded(n, F16)
    call("dbmm_cast_f32_f16", x, buf, n)
    assert torch.equal(bits(buf[:n]), bits(ref)) and guard_intact(buf, n)


# ---- gather_rows -------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n_idx,D", [(9, 4), (1000, 68), (20000, 1024)])
def test_gather_rows(n_idx, D):
    """duplicates, the first and the last row, indices outside the table (clamped into it); 20000 x 1024 is 5,120,000 float4s, past the
    block cap (this file's own cap is half of it)"""
    n = 1000
    if D == 1024:
        assert n_idx * (D // 4) == 5120000 > CAP
    table = randn(110, n, D)
    idx = randint(111, 0, n, n_idx)
    idx[:9] = torch.tensor([0, n - 1, 5, 5, -3, n + 5, -2 ** 40, 2 ** 40, n], device=DEV)
    idx[-2:] = torch.tensor([n - 1, 0], device=DEV)
    out = ops.gather_rows(table, idx)
    assert torch.equal(out, table[idx.clamp(0, n - 1)])


# ---- colsum ------------------------------------------------------------------------------------------------------------------------------

def colsum_raw(x):
    B, N = x.shape
    buf = guarded(N, F32)
    call("dbmm_colsum", x, buf, B, N)
    assert guard_intact(buf, N)
    return buf[:N].clone()


@pytest.mark.parametrize("B", [1, 63, 64, 65, 1000])
def test_colsum_integers_exact(B):
    """small integers: every partial sum is exact in fp32 whatever the order, so a dropped or doubled row or column shows as an
    integer difference.  N = 12 and 20 leave column groups of the last block idle; 64 is the row-lane count"""
    for N in (4, 12, 16, 20, 1024):
        x = randint(120 + N, -8, 9, B, N).float()
        want = x.long().sum(0)
        got = colsum_raw(x)
        assert torch.equal(got.long(), want) and torch.equal(got, got.round()), (B, N)
        assert torch.equal(ops.colsum(x), got)


def test_colsum_floats():
    x = randn(130, 1000, 1024)
    ref = x.double().sum(0)
    e_t, e_k = relerr(x.sum(0), ref), relerr(ops.colsum(x), ref)
    print(f"colsum (1000, 1024): kernel error {e_k:.3e}, torch float32 error {e_t:.3e}")
    assert e_k <= 4 * e_t + 2.0 ** -23
    assert torch.equal(ops.colsum(x), ops.colsum(x))           # a fixed order: two calls agree bit for bit
    with pytest.raises(RuntimeError, match="colsum"):
        ops.colsum(torch.zeros(8, 6, device=DEV))
    torch.cuda.synchronize()


# ---- l2norm_rows -------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("B,D", [(1, 4), (3, 512), (5, 1024), (1001, 68), (7, 4096)])
def test_l2norm_rows(B, D):
    """D / 4 below, at and above the 64 lanes of a row's wave; B off the 4 rows of a block; rows of 1e3 and 1e-3 times the others"""
    x = randn(140 + D, B, D)
    x = x * torch.tensor([1.0, 1e3, 1e-3], device=DEV)[torch.arange(B, device=DEV) % 3].unsqueeze(1)
    ref = x.double() / x.double().norm(dim=1, keepdim=True)
    y = ops.l2norm_rows(x)
    e_t, e_k = relerr(x / x.norm(dim=1, keepdim=True), ref), relerr(y, ref)
    print(f"l2norm_rows ({B}, {D}): kernel error {e_k:.3e}, torch float32 error {e_t:.3e}")
    assert e_k <= 4 * e_t + 2.0 ** -23
    assert ((y.double().norm(dim=1) - 1.0).abs().max().item()) < 1e-6
    buf = guarded(B * D, F32)
    call("dbmm_l2norm_rows", x, buf, B, D)
    assert torch.equal(buf[:B * D].view(B, D), y) and guard_intact(buf, B * D)


# ---- per-group sums and counters ---------------------------------------------------------------------------------------------------------

def group_ids(seed, B, G):
    """ids in [-1, G]: both neighbours of the valid range occur; a few far outside it whose low 32 bits look like valid ids"""
    g = randint(seed, -1, G + 1, B)
    far = torch.tensor([2 ** 32, 2 ** 32 + 1, -2 ** 32, 2 ** 33 + G - 1, 2 ** 31], device=DEV)
    if B >= 255:
        g[7:7 + len(far)] = far
    return g


def per_group(values, g, G):
    """int64 sum of `values` over the rows of each group; rows whose id is outside [0, G) belong to none"""
    ok = (g >= 0) & (g < G)
    return torch.zeros(G, device=DEV, dtype=I64).index_add_(0, g[ok], values[ok].long())


@pytest.mark.parametrize("G", [1, 4, 64])
def test_group_loss_sum(G):
    """integer-valued losses: exact sums.  Ids outside [0, G) are skipped -- as 64-bit values; a second call adds to the first"""
    for B in (1, 255, 256, 257, 1000):
        loss = randint(150 + B, 0, 9, B).float()
        g = group_ids(151 + B, B, G)
        want = per_group(loss, g, G)
        start = torch.arange(G, device=DEV, dtype=F32)
        buf = guarded(G, F32)
        buf[:G] = start
        call("dbmm_group_loss_sum", loss, g, buf, B, G)
        assert torch.equal(buf[:G].long(), start.long() + want) and guard_intact(buf, G), (B, G)
        sums = start.clone()
        ops.group_loss_sum(loss, g, sums); ops.group_loss_sum(loss, g, sums)
        assert torch.equal(sums.long(), start.long() + 2 * want), (B, G)


@pytest.mark.parametrize("C", [2, 7])
@pytest.mark.parametrize("G", [1, 4, 64])
def test_group_count(G, C):
    """(rows, rows whose first-maximum logit is the label) per group; logits drawn from three values, so most rows hold a tie"""
    for B in (1, 255, 256, 257, 1000):
        logits = randint(160 + B, 0, 3, B, C).float()
        pred = first_argmax(logits)
        assert B == 1 or bool(((logits == logits.max(1, keepdim=True).values).sum(1) > 1).any())
        y = randint(161 + B, 0, C, B)
        g = group_ids(162 + B, B, G)
        want = torch.stack([per_group(torch.ones_like(y), g, G), per_group((pred == y).long(), g, G)], 1)
        buf = guarded(2 * G, I64)
        buf[:2 * G] = 0
        call("dbmm_group_count", logits, y, g, buf, B, C, G)
        assert torch.equal(buf[:2 * G].view(G, 2), want) and guard_intact(buf, 2 * G), (B, C, G)
        counts = torch.zeros(G, 2, device=DEV, dtype=I64)
        ops.group_count(logits, y, g, counts); ops.group_count(logits, y, g, counts)
        assert torch.equal(counts, 2 * want), (B, C, G)


# ---- the wrappers refuse what the kernels would misread ------------------------------------------------------------------------------------

def test_wrappers_refuse_misshapen_operands_before_launching():
    """these wrappers hand the library raw pointers and a few sizes: an operand of another shape, dtype or layout is a read or write
    outside a buffer, or one type read as another.  Zero tensors; every call raises before anything is launched."""
    z = lambda *s, dt=F32: torch.zeros(s, device=DEV, dtype=dt)
    for fn, kw in ((ops.im2col_patch, {}), (ops.im2col_patch_f16, {"Kp": 3 * 16 * 16})):
        for shape in ((2, 3, 64, 32), (2, 1, 64, 64), (2, 3, 32, 64), (2, 4, 64, 64), (3, 64, 64), (2, 3, 40, 40)):
            with pytest.raises(RuntimeError, match=r"image batch of shape \(" + ", ".join(map(str, shape))):
                fn(z(*shape), 16, **kw)
    for Kp in (3 * 16 * 16 - 8, 3 * 16 * 16 + 4, 3 * 7 * 7 + 1):
        with pytest.raises(RuntimeError, match=f"Kp = {Kp}"):
            ops.im2col_patch_f16(z(2, 3, 112, 112), 16 if Kp > 200 else 7, Kp)
    with pytest.raises(RuntimeError, match="out_absmax"):
        ops.im2col_patch(z(2, 3, 64, 64), 16, out_absmax=z(1, dt=F16))

    B, L, W = 2, 5, 64
    good = dict(patches=z(B * (L - 1), W), cls=z(W), pos=z(L, W))
    for f16, fn in ((False, ops.vit_tokens), (True, ops.vit_tokens_f16)):
        ok = dict(good, patches=good["patches"].half()) if f16 else good
        wrong = F32 if f16 else F16
        for name, bad in (("patches", ok["patches"].to(wrong)), ("patches", z(W, B * (L - 1), dt=ok["patches"].dtype).t()),
                          ("cls", z(W, dt=F16)), ("cls", z(W, 2)[:, 0]), ("pos", z(L, W, dt=F16)), ("pos", z(W, L).t())):
            with pytest.raises(RuntimeError, match=f"vit_tokens {name}"):
                fn(**dict(ok, **{name: bad}), B=B)
        with pytest.raises(RuntimeError, match="positional embedding"):
            fn(ok["patches"], ok["cls"], z(L + 1, W), B)

    tok = z(2, 77, dt=I32)
    for fn in (ops.embed_gather, ops.embed_gather_f16):
        name = fn.__name__
        for what, args in (("table", (tok, z(100, 64, dt=F16), z(77, 64))), ("table", (tok, z(64, 100).t(), z(77, 64))),
                           ("pos", (tok, z(100, 64), z(77, 64, dt=F16))), ("pos", (tok, z(100, 64), z(64, 77).t()))):
            with pytest.raises(RuntimeError, match=f"{name} {what}"):
                fn(*args)
        with pytest.raises(RuntimeError, match="tokens per prompt"):
            fn(z(2, 9, dt=I32), z(100, 64), z(77, 64))

    for fn, dt, wrong in ((ops.gather_eot, F32, F16), (ops.gather_eot_f16, F16, F32)):
        name = fn.__name__
        x = z(3, 77, 64, dt=dt)
        for bad in (z(3, 77, dt=I64), z(3, 76, dt=I32), z(2, 77, dt=I32), z(77, 3, dt=I32).t(), z(3 * 77, dt=I32)):
            with pytest.raises(RuntimeError, match=f"{name} tokens"):
                fn(bad, x)
        for bad in (z(3, 77, 64, dt=wrong), z(3, 64, 77, dt=dt).transpose(1, 2), z(3 * 77, 64, dt=dt)):
            with pytest.raises(RuntimeError, match=f"{name} x"):
                fn(z(3, 77, dt=I32), bad)

    B, C, G = 6, 2, 4
    ok = dict(logits=z(B, C), y=z(B, dt=I64), g=z(B, dt=I64), counts=z(G, 2, dt=I64))
    for name, bad in (("y", z(B, dt=I32)), ("y", z(B - 1, dt=I64)), ("g", z(B, dt=I32)), ("g", z(B + 1, dt=I64)), ("g", z(B, 2, dt=I64)[:, 0]),
                      ("counts", z(G, 2, dt=I32)), ("counts", z(G, 3, dt=I64)), ("counts", z(2, G, dt=I64).t()), ("logits", z(B, C, dt=F16)),
                      ("logits", z(C, B).t())):
        with pytest.raises(RuntimeError, match=f"group_count {name}"):
            ops.group_count(**dict(ok, **{name: bad}))
    with pytest.raises(RuntimeError, match="G <= 64"):
        ops.group_count(**dict(ok, counts=z(65, 2, dt=I64)))
    ok = dict(loss_rows=z(B), g=z(B, dt=I64), sums=z(G))
    for name, bad in (("g", z(B, dt=I32)), ("g", z(B - 1, dt=I64)), ("g", z(B, 2, dt=I64)[:, 0]), ("loss_rows", z(B, dt=F16)),
                      ("loss_rows", z(B, 2)[:, 0]), ("sums", z(G, dt=torch.float64)), ("sums", z(G, 2)[:, 0]), ("sums", z(65))):
        with pytest.raises(RuntimeError, match=f"group_loss_sum {name}"):
            ops.group_loss_sum(**dict(ok, **{name: bad}))
    torch.cuda.synchronize()


@pytest.mark.parametrize("shape", [(2, 3, 64, 32), (2, 1, 64, 64)], ids=["half_width", "one_channel"])
def test_vit_tower_refuses_misshapen_images(shape):
    """a [B, 3, 64, 32] batch has the patch count the positional table expects when only the height is looked at, a [B, 1, 64, 64]
    batch a third of the pixels the gather reads: the reference raises for both (conv1 on the channels, `x + positional_embedding` on
    the patch count, clip/model.py:224-229), and so do both modes here, before a kernel sees the batch"""
    from dbmm_amd.clip.model import build_model, convert_weights
    sd = synth.clip_state_dict(3, "tiny-ViT")
    img = torch.zeros(shape, device=DEV)
    with pytest.raises(RuntimeError, match="image batch of shape"):
        build_model(sd).cuda().encode_image(img)
    with pytest.raises(RuntimeError, match="image batch of shape"):
        convert_weights(build_model(sd).cuda()).encode_image(img)
    torch.cuda.synchronize()
