"""Tensor-level wrappers over the C ABI (include/dbmm.h).  Plumbing only: allocate outputs
with torch's caching allocator, pass raw pointers + the current HIP stream, raise on error.
Every function requires HIP tensors -- there is no CPU path here.
"""
import ctypes
import math
import os
import weakref
from collections import namedtuple

import numpy as np
import torch

from . import _lib
from ._lib import check, ptr, require_cuda, stream

ACT_NONE, ACT_RELU, ACT_QUICKGELU = 0, 1, 2


class DbmmUnsupported(_lib.DbmmError):
    """a wrapper's C entry answered DBMM_E_UNSUPPORTED (no kernel for this valid request)"""


def set_option(name, value):
    """library option by name (include/dbmm.h dbmm_set_option; names in csrc/options.hip); returns the previous value"""
    old = get_option(name)
    check(_lib.lib().dbmm_set_option(name.encode(), int(value)), f"set_option({name})")
    return old


def get_option(name):
    v = ctypes.c_int()
    check(_lib.lib().dbmm_get_option(name.encode(), ctypes.byref(v)), f"get_option({name})")
    return v.value


# every output / workspace of this module comes from here (torch's caching allocator); tests swap in an allocator
# that surrounds each tensor with guard zones to catch writes outside the tensor (tests/test_gpu_headline.py)
_empty = torch.empty

# ---- optional per-launch timing of the MFMA kernel family (bench.py roofline leg) ----------
_prof = None
_prof_conv_only = False
_prof_paused = False


def profile_begin(conv_only=False):
    """start collecting (kernel tag, flops, start event, end event) for every igemm launch --
    with conv_only, just the KxK convolutions (the event pairs are stream work themselves, ~4 us
    per launch, so a bench that only needs the dominant kernel should not pay for all)."""
    global _prof, _prof_conv_only, _prof_paused
    _prof, _prof_conv_only, _prof_paused = [], bool(conv_only), False


def profile_sample(on):
    """inside a profile_begin() ... profile_end() window: switch the per-launch events off / on again (bench.py times the launches of
    every k-th step only: an event pair is ~4 us of stream time, ~60 launches per RN50 step)"""
    global _prof_paused
    _prof_paused = not on


def profile_end():
    """stop collecting; returns {tag: (launches, total_flops, total_ms, total_algorithmic_bytes)} (synchronises)."""
    global _prof
    rec, _prof = _prof or [], None
    torch.cuda.synchronize()
    out = {}
    for tag, flops, nbytes, e0, e1 in rec:
        n, f, ms, by = out.get(tag, (0, 0.0, 0.0, 0.0))
        out[tag] = (n + 1, f + flops, ms + e0.elapsed_time(e1), by + nbytes)
    return out


def _last_igemm_tag():
    """exact instantiation of the igemm launch just issued, spelled like rocprofv3's kernel name"""
    cfg = (ctypes.c_int * 11)()
    _lib.lib().dbmm_debug_last_igemm(cfg)
    if cfg[8] == 5:        # conv3 + downsample dual-source GEMM: the x3 kernel with TWO = 1
        return f"igemm_x3_kernel<{cfg[0]}, {cfg[1]}, {cfg[2]}, {cfg[3]}, 0, {cfg[7]}, {cfg[9]}, 2, 1, 32, 1>"
    if cfg[8] == 8:        # the dual-source GEMM on the deep-pipelined kernel: <ACT, RES, TWO = 1>
        return "gemm_pair_8ph_kernel<dual>"
    if cfg[8] == 9:        # conv3 + residual, short K into many channels (conv1x1_res_stream.hip): <K, POOL>
        return f"conv1x1_res_stream_kernel<{cfg[0]}, {cfg[5]}>"
    if cfg[8] == 6:        # deep-pipelined parity GEMM (gemm_pair_8ph.hip): <ACT, RES> are not reported
        return "gemm_pair_8ph_kernel"
    if cfg[8] == 7:        # eight-phase 3x3 halo kernel (conv3x3_halo8.hip): <POOL, ACT>, ACT not reported
        return f"conv3x3_halo8{'n' if cfg[1] == 128 else ''}_kernel<{cfg[5]}>"
    if cfg[8] == 4:        # 3x3 halo kernel: <BN, WAVES_M, WAVES_N, MINB, SK, POOL>
        return f"igemm_halo_kernel<{cfg[1]}, {cfg[2]}, {cfg[3]}, {cfg[7]}, {cfg[9]}, {cfg[5]}>"
    if cfg[8] in (2, 3):   # split-precision kernels: <BM, BN, WAVES_M, WAVES_N, AMODE, MINB, SK, NP, NW, BK, TWO>
        return (f"igemm_x3_kernel<{cfg[0]}, {cfg[1]}, {cfg[2]}, {cfg[3]}, {cfg[4]}, {cfg[7]}, {cfg[9]}, {cfg[8]}, "
                f"{cfg[10]}, {cfg[6]}, 0>")
    return "igemm_f32_kernel<" + ", ".join(str(v) for v in cfg) + ">"


class _Timed:
    """HIP events (on the launch stream = torch's current stream) around one igemm launch.  nbytes = the launch's
    ALGORITHMIC bytes: every operand read once, every output written once."""
    def __init__(self, M, N, K, amode, wmode, nbytes=0):
        self.args = (M, N, K, amode, wmode)
        self.nbytes = float(nbytes)

    def __enter__(self):
        if _TRACE_LAUNCHES:
            with open(_TRACE_LAUNCHES, "a") as f:
                f.write(f"igemm {self.args} ... ")
        self.on = _prof is not None and not _prof_paused and (self.args[3] == 1 or not _prof_conv_only)
        if self.on:
            self.e0 = torch.cuda.Event(enable_timing=True)
            self.e0.record()

    def __exit__(self, *exc):
        if _TRACE_LAUNCHES:
            torch.cuda.synchronize()
            with open(_TRACE_LAUNCHES, "a") as f:
                f.write("ok\n")
        if self.on and _prof is not None and exc[0] is None:
            M, N, K, amode, wmode = self.args
            e1 = torch.cuda.Event(enable_timing=True)
            e1.record()
            tag = _chain_tag if amode == -1 else _last_igemm_tag()
            _prof.append((tag, 2.0 * M * N * K, self.nbytes, self.e0, e1))


_ws_cache = {}


def igemm_workspace(device):
    """per-device scratch for the stream-K work split (allocated once, reused by every launch on
    the stream; launches on one stream are ordered, so sharing it is safe)."""
    key = (device.type, device.index)
    ws = _ws_cache.get(key)
    if ws is None:
        ws = _empty(_lib.lib().dbmm_workspace_bytes_igemm() // 4, device=device, dtype=torch.float32)
        _ws_cache[key] = ws
    return ws


def _sized(name, t, n):
    """an optional per-channel / per-row operand the library will index as n elements (it only sees the pointer)"""
    if t is not None and t.numel() != n:
        raise RuntimeError(f"{name}: {t.numel()} elements where the kernels will index {n}")


def _f32c(t, name=None):
    if t.dtype != torch.float32 or not t.is_contiguous():
        what = f"{name} {tuple(t.shape)}: " if name else ""
        raise _lib.DbmmError(f"{what}expected a contiguous float32 tensor, got {t.dtype} contiguous={t.is_contiguous()}")
    return t


# id(tensor) -> (weak reference, dtype, shape, element count) of the operands a compiled plan keeps for its lifetime (mark_static)
_static = {}


def mark_static(*tensors):
    """A plan builder (clip/model.py) hands over the tensors its plan owns and never replaces -- planes, packed weights, BatchNorm scales,
    biases, ratios, positional tables: device and contiguity are checked here, once, and their dtype and shape recorded, so that the
    wrappers compare only those two per launch (about 60 launches per RN50 step read the same few hundred tensors).  Only tensors that
    pass are recorded; anything else, and every tensor not handed over, gets the whole check at each launch.  An entry goes when its
    tensor does.  Not for module parameters: `.data` of a parameter can be replaced under the same object."""
    for t in tensors:
        if t is None:
            continue
        try:
            require_cuda(t)
        except _lib.DbmmError:
            continue
        if t.is_contiguous():
            key = id(t)
            _static[key] = (weakref.ref(t, lambda _, key=key: _static.pop(key, None)), t.dtype, tuple(t.shape), t.numel())


def _name(name):
    """operand names are put together only when an error needs them: a string or a tuple of parts"""
    return name if isinstance(name, str) else " ".join(name)


def _operand(name, t, dtype, shape):
    """an operand the library only sees as a pointer: on the device, contiguous, of the dtype the kernel reads and of exactly the
    shape (a tuple) or element count (an int) it will index -- an int32 tensor read as int64, or a short one, is a stray read,
    not an error the library can see"""
    m = _static.get(id(t))
    if m is not None and m[1] == dtype and (m[3] if shape.__class__ is int else m[2]) == shape and m[0]() is t:
        return t
    if t is None:
        raise _lib.DbmmError(f"{_name(name)}: the kernel reads this operand, got None")
    require_cuda(t)
    fits = t.numel() == shape if isinstance(shape, int) else tuple(t.shape) == tuple(shape)
    if t.dtype != dtype or not t.is_contiguous() or not fits:
        want = f"{shape} elements" if isinstance(shape, int) else f"shape {tuple(shape)}"
        raise _lib.DbmmError(f"{_name(name)}: expected a contiguous {dtype} tensor of {want}, got {t.dtype} {tuple(t.shape)} "
                             f"contiguous={t.is_contiguous()}")
    return t


def _optional(name, t, dtype, shape):
    """_operand for an argument the entry takes as NULL when it is None"""
    return None if t is None else _operand(name, t, dtype, shape)


def _absmax(name, t, required=False):
    """a one-element float32 device scalar (the *_absmax arguments; one element is always contiguous); None is NULL unless the entry
    needs the scalar"""
    if t is None and required:
        raise _lib.DbmmError(f"{_name(name)}: the kernel reads this scalar, got None")
    if t is not None:
        require_cuda(t)
        if t.dtype != torch.float32 or t.numel() != 1:
            raise _lib.DbmmError(f"{_name(name)}: expected one float32 element, got {t.dtype} {tuple(t.shape)}")
    return t


def _spans(name, t, dtype, n):
    """an operand addressed through a leading dimension: on the device, contiguous, of the dtype the kernel reads, and at least the
    n elements the entry will index from its first one"""
    require_cuda(t)
    if t.dtype != dtype or not t.is_contiguous() or t.numel() < n:
        raise _lib.DbmmError(f"{name}: expected a contiguous {dtype} tensor of at least {n} elements, got {t.dtype} {tuple(t.shape)} "
                             f"contiguous={t.is_contiguous()}")
    return t


def _rank(name, t, nd):
    """the shape of `t` is about to be read by index: it has nd dimensions"""
    if t.dim() != nd:
        raise _lib.DbmmError(f"{name}: a tensor of {nd} dimensions is expected, got shape {tuple(t.shape)}")
    return t


def _plane(name, c, N, K):
    """the operands of a plan entry (clip/model.py _pack_conv) the chain kernels read: one exact fp16 plane [1][N][K] and the
    BatchNorm scale / bias per output channel"""
    _operand((name, "plane"), c["ph"], torch.float16, (1, N, K))
    _operand((name, "scale"), c["sc"], torch.float32, N)
    _operand((name, "bias"), c["b"], torch.float32, N)


def _conv_f16(name, c, N, K):
    """the (w f16 [N][K], scale f32 [N], bias f32 [N]) triple of an fp16-mode 1x1 conv"""
    w, s, b = c
    _operand((name, "weight"), w, torch.float16, (N, K))
    _operand((name, "scale"), s, torch.float32, N)
    _operand((name, "bias"), b, torch.float32, N)


def _patch_image_check(name, x, P, Kp=None):
    # the library gets B, R, P and a pointer and reads B * 3 * R * R elements: another channel count or a non-square image
    # fails here like the reference's conv1 / `x + self.positional_embedding` (clip/model.py:224-229), not as a read past the batch
    if x.dim() != 4 or x.shape[1] != 3 or x.shape[2] != x.shape[3] or P <= 0 or x.shape[2] % P:
        raise RuntimeError(f"{name}: image batch of shape {tuple(x.shape)} where the patch kernel reads [B, 3, R, R] with R a multiple "
                           f"of the patch size {P}")
    if Kp is not None and (Kp < 3 * P * P or Kp % 8):
        raise RuntimeError(f"{name}: padded patch length Kp = {Kp} for images of shape {tuple(x.shape)}: it must be a multiple of 8 "
                           f"(aligned vector stores) and at least 3 * {P} * {P} = {3 * P * P}")


def split_planes(w):
    """fp32 [N][K] weight -> three bf16 planes [3][N][K] (hi, mid, lo) for the split-precision kernels"""
    require_cuda(w)
    _f32c(w)
    if w.dim() < 2:
        raise _lib.DbmmError(f"split planes of a weight [N][K] (or [Cout][Cin][kh][kw]), got shape {tuple(w.shape)}")
    N, K = w.shape[0], w.numel() // w.shape[0]
    planes = _empty((3, N, K), device=w.device, dtype=torch.bfloat16)
    check(_lib.lib().dbmm_split_weight_planes(ptr(w), ptr(planes), N, K, stream()), "split_weight_planes")
    return planes


def split_planes_f16(w, allow_single=False):
    """fp32 [N][K] weight -> (fp16 planes [n][N][K] of w * 2^w_exp, w_exp, n) for the fp16-pair
    kernel; w_exp puts max|w| just below 2^14 (one host read of the maximum, at plan time).
    n = 2 (hi, lo) in general.  With allow_single, n = 1 when the scaled weight is exactly
    representable in fp16 -- the case for every conv / linear weight that went through the
    reference's build_model, which stores them in fp16 -- and K is a multiple of 32."""
    require_cuda(w)
    _f32c(w)
    if w.dim() < 2:
        raise _lib.DbmmError(f"split planes of a weight [N][K] (or [Cout][Cin][kh][kw]), got shape {tuple(w.shape)}")
    N, K = w.shape[0], w.numel() // w.shape[0]
    m = float(w.abs().max())
    w_exp = 0 if not (m > 0.0 and math.isfinite(m)) else max(-40, min(40, 13 - math.frexp(m)[1] + 1))
    if allow_single and K % 32 == 0:
        ws = w.reshape(N, K) * (2.0 ** w_exp)
        h = ws.half()
        if torch.equal(h.float(), ws):
            return h.reshape(1, N, K).contiguous(), w_exp, 1
    planes = _empty((2, N, K), device=w.device, dtype=torch.float16)
    check(_lib.lib().dbmm_split_weight_planes_f16(ptr(w), ptr(planes), N, K, w_exp, stream()), "split_weight_planes_f16")
    return planes, w_exp, 2


def gemm(a, w, bias=None, residual=None, act=ACT_NONE, alpha=1.0, trans_a=False, trans_w=False,
         M=None, N=None, K=None, lda=None, out=None, w_planes=None, w_planes_f16=None, w_exp=0, a_absmax=None,
         c_absmax=None):
    """c = act(alpha * (op(a) @ op(w)^T + bias) + residual); see dbmm_gemm_bias_act.
    w_planes: bf16 triple; w_planes_f16 / w_exp + a_absmax: fp16-pair kernel (split_planes_f16);
    c_absmax (1-element device tensor, zeroed by the caller) receives max|c|."""
    require_cuda(a, w)
    _f32c(_rank("gemm w", w, 2))
    if a.dtype != torch.float32:
        raise _lib.DbmmError("gemm needs float32")
    _f32c(a, "gemm a")
    if lda is None:
        lda = a.shape[-1]
    if M is None:
        M = a.shape[-1] if trans_a else a.numel() // a.shape[-1]
    if K is None:
        K = a.numel() // a.shape[-1] if trans_a else a.shape[-1]
    if N is None:
        N = w.shape[1] if trans_w else w.shape[0]
    if out is None:
        out = _empty((M, N), device=a.device, dtype=torch.float32)
    else:
        require_cuda(out)
        _f32c(out, "gemm out")
    ldr = residual.shape[-1] if residual is not None else 0
    # the library sees raw pointers and leading dimensions: what it will index must be there (a [K][lda] with trans_a, else [M][lda])
    a_span = (K - 1) * lda + M if trans_a else (M - 1) * lda + K
    if w.numel() != N * K or a.numel() < a_span or out.shape[-1] < N or out.numel() < (M - 1) * out.shape[-1] + N:
        raise RuntimeError(f"gemm: operands {tuple(a.shape)}, {tuple(w.shape)}, out {tuple(out.shape)} do not hold an M = {M}, N = {N}, K = {K} product")
    _optional("gemm bias", bias, torch.float32, N)
    if residual is not None:
        if ldr < N:
            raise RuntimeError(f"gemm: residual {tuple(residual.shape)} for an [{M}, {N}] output")
        _spans("gemm residual", residual, torch.float32, (M - 1) * ldr + N)
    if w_planes_f16 is not None:
        if w_planes_f16.dim() != 3 or w_planes_f16.shape[0] not in (1, 2):
            raise RuntimeError(f"gemm: weight planes {tuple(w_planes_f16.shape)} for a [{N}, {K}] weight")
        _operand("gemm w_planes_f16", w_planes_f16, torch.float16, (w_planes_f16.shape[0], N, K))
    _optional("gemm w_planes", w_planes, torch.bfloat16, (3, N, K))
    _absmax("gemm a_absmax", a_absmax); _absmax("gemm c_absmax", c_absmax)
    ws = igemm_workspace(a.device)
    # algorithmic bytes: A and the residual read once, C written once, W once in the form the kernel reads it
    nby = 4 * (M * K + M * N * (2 if residual is not None else 1)) + \
        (w_planes_f16.numel() * 2 if w_planes_f16 is not None else (w_planes.numel() * 2 if w_planes is not None else 4 * N * K))
    if (w_planes_f16 is not None or c_absmax is not None) and not trans_a and not trans_w:
        nw = 2 if w_planes_f16 is None else int(w_planes_f16.shape[0])
        with _Timed(M, N, K, 0, 0, nby):
            check(_lib.lib().dbmm_gemm_bias_act_x2(ptr(a), lda, ptr(a_absmax), ptr(w), ptr(w_planes_f16), nw, int(w_exp),
                                                   w.shape[-1], None, ptr(bias), ptr(residual), ldr, ptr(out),
                                                   out.shape[-1], ptr(c_absmax), M, N, K, float(alpha), act, ptr(ws),
                                                   ws.numel() * 4, stream()), "gemm_bias_act_x2")
        return out
    if w_planes is not None and not trans_a and not trans_w:
        with _Timed(M, N, K, 0, 0, nby):
            check(_lib.lib().dbmm_gemm_bias_act_x3(ptr(a), lda, ptr(w), ptr(w_planes), w.shape[-1], ptr(bias),
                                                   ptr(residual), ldr, ptr(out), out.shape[-1], M, N, K, float(alpha),
                                                   act, ptr(ws), ws.numel() * 4, stream()), "gemm_bias_act_x3")
        return out
    with _Timed(M, N, K, 2 if trans_a else 0, int(trans_w), nby):
        check(_lib.lib().dbmm_gemm_bias_act_ws(ptr(a), lda, int(trans_a), ptr(w), w.shape[-1], int(trans_w), ptr(bias),
                                               ptr(residual), ldr, ptr(out), out.shape[-1], M, N, K, float(alpha), act,
                                               ptr(ws), ws.numel() * 4, stream()), "gemm_bias_act")
    return out


WL_TAP_MAJOR, WL_CHUNK_MAJOR, WL_CHUNK32_MAJOR = 0, 1, 2


def pack_conv_weight(w_oihw, chunk_major=False):
    """[Cout][Cin][kh][kw] -> (packed fp32 [Cout][K], layout id).

    Default K order (kh, kw, cin).  chunk_major=True packs (cin/16, kh, kw, 16), chunk_major=32
    packs (cin/32, kh, kw, 32) -- the taps of a
    channel slab adjacent along K -- which cuts the fabric re-reads of the 3x3 gather (each
    input pixel is read by 9 taps) but measured 1-5 % *slower* on MI355X at B = 512: the
    Infinity Cache already absorbs the re-reads and tap-major uses both halves of every 128-B
    line back to back.  Kept as an option (needs Cin % 16 == 0)."""
    Cout, Cin, kh, kw = w_oihw.shape
    slab = 32 if chunk_major == 32 else 16
    if chunk_major and kh * kw > 1 and Cin % slab == 0:
        w = w_oihw.reshape(Cout, Cin // slab, slab, kh, kw).permute(0, 1, 3, 4, 2)
        return w.contiguous().float().reshape(Cout, kh * kw * Cin), (WL_CHUNK32_MAJOR if slab == 32 else WL_CHUNK_MAJOR)
    return w_oihw.permute(0, 2, 3, 1).contiguous().float().reshape(Cout, kh * kw * Cin), WL_TAP_MAJOR


def conv_bn_act(x, w, bias, residual, kh, kw, stride, pad, act, w_layout=WL_TAP_MAJOR, w_planes=None,
                w_planes_f16=None, w_exp=0, x_absmax=None, y_absmax=None, out_scale=None, pool=1, keep_full=False):
    """x NHWC [B,H,W,Cin]; w packed [Cout][K] (BN folded) in `w_layout` order (default
    [Cout][kh][kw][Cin]; see pack_conv_weight); returns NHWC.
    w_planes: bf16 triple (split_planes) -> split-precision kernel.
    w_planes_f16 / w_exp (split_planes_f16) + x_absmax (1-element device tensor >= max|x|) ->
    fp16-pair kernel; y_absmax (1-element device tensor, zeroed by the caller) receives max|y|.
    out_scale ([Cout], x2 entry only): per-channel scale of the accumulator before the bias.
    pool = 2: followed by AvgPool2d(2) (returns the pooled tensor); fused into the conv epilogue
    when the library has a kernel for it, otherwise the two calls are composed here.
    keep_full (with pool = 2): returns (pooled, un-pooled) -- both written by the one launch."""
    require_cuda(x, w)
    _f32c(x); _f32c(w)
    B, H, W, Cin = x.shape
    Cout = w.shape[0]
    Ho = (H + 2 * pad - kh) // stride + 1
    Wo = (W + 2 * pad - kw) // stride + 1
    if pool not in (1, 2):
        raise _lib.DbmmError("conv_bn_act: pool must be 1 or 2")
    if w.numel() != Cout * kh * kw * Cin:
        raise RuntimeError(f"conv_bn_act: packed weight {tuple(w.shape)} for a {kh} x {kw} conv over {Cin} channels")
    _optional("conv_bn_act bias", bias, torch.float32, Cout); _optional("conv_bn_act out_scale", out_scale, torch.float32, Cout)
    _optional("conv_bn_act residual", residual, torch.float32, (B, Ho, Wo, Cout))
    if w_planes_f16 is not None:
        if w_planes_f16.dim() < 2 or w_planes_f16.shape[0] not in (1, 2):
            raise RuntimeError(f"conv_bn_act: weight planes {tuple(w_planes_f16.shape)} for a packed weight {tuple(w.shape)}")
        _operand("conv_bn_act w_planes_f16", w_planes_f16, torch.float16, w_planes_f16.shape[0] * w.numel())
    _optional("conv_bn_act w_planes", w_planes, torch.bfloat16, 3 * w.numel())
    _absmax("conv_bn_act x_absmax", x_absmax); _absmax("conv_bn_act y_absmax", y_absmax)
    plain = kh == 1 and kw == 1 and stride == 1 and pad == 0
    split = w_planes_f16 is not None or y_absmax is not None or out_scale is not None
    # algorithmic bytes: input map and residual read once, output(s) written once, weights once
    wby = w_planes_f16.numel() * 2 if w_planes_f16 is not None else (w_planes.numel() * 2 if w_planes is not None else w.numel() * 4)
    oel = B * Ho * Wo * Cout
    nby_pool = 4 * (x.numel() + (residual.numel() if residual is not None else 0) + oel // 4 + (oel if keep_full else 0)) + wby
    nby = 4 * (x.numel() + (residual.numel() if residual is not None else 0) + oel) + wby
    # the 32-channel stem convs: persistent patch kernel (csrc/conv_patch.hip); option conv_patch = 0 disables
    if (Cin == 32 and kh == 3 and kw == 3 and stride == 1 and pad == 1 and act == ACT_RELU and residual is None and not keep_full
            and w_planes_f16 is not None and w_planes_f16.shape[0] == 1 and out_scale is not None and x_absmax is not None and bias is not None
            and Cout in (32, 64) and H % 4 == 0 and W % 28 == 0 and (pool == 1 or (H % 2 == 0 and W % 2 == 0))
            and w_layout in (WL_TAP_MAJOR, WL_CHUNK32_MAJOR) and get_option("conv_patch")):
        y = _empty((B, H // pool, W // pool, Cout), device=x.device, dtype=torch.float32)
        global _chain_tag
        _chain_tag = f"conv3x3_c32_kernel<{Cout}, {int(pool == 2)}>"
        t = _Timed(B * H * W, Cout, 9 * Cin, -1, 0, 4 * (x.numel() + y.numel()) + 2 * Cout * 9 * Cin)
        t.__enter__()
        rc = _lib.lib().dbmm_conv3x3_c32_bn_relu_x2(ptr(x), ptr(x_absmax), ptr(w_planes_f16), int(w_exp), ptr(out_scale), ptr(bias),
                                                   ptr(y), ptr(y_absmax), B, H, W, Cin, Cout, 2 if pool == 2 else 0, stream())
        if rc == 0:
            t.__exit__(None, None, None)
            return y
        if rc not in (_lib.E_UNSUPPORTED, _lib.E_ALIGN):      # a shape / alignment the patch kernel does not serve: the general kernels below do
            check(rc, "conv3x3_c32_bn_relu_x2")
        del y
    if pool == 2 and split and Ho % 2 == 0 and Wo % 2 == 0:
        y = _empty((B, Ho // 2, Wo // 2, Cout), device=x.device, dtype=torch.float32)
        yf = _empty((B, Ho, Wo, Cout), device=x.device, dtype=torch.float32) if keep_full else None
        t = _Timed(B * Ho * Wo, Cout, kh * kw * Cin, 0 if plain else 1, 0, nby_pool)
        t.__enter__()
        rc = _conv_x2(x, w, bias, residual, y, kh, kw, stride, pad, act, w_layout, w_planes_f16, w_exp, x_absmax,
                      y_absmax, out_scale, 2, yf)
        if rc == 0:
            t.__exit__(None, None, None)
            return (y, yf) if keep_full else y
        if rc != _lib.E_UNSUPPORTED:
            check(rc, "conv_bn_act_x2(pool)")
    y = _empty((B, Ho, Wo, Cout), device=x.device, dtype=torch.float32)
    with _Timed(B * Ho * Wo, Cout, kh * kw * Cin, 0 if plain else 1, 0, nby):
        ws = igemm_workspace(x.device)
        if split:
            check(_conv_x2(x, w, bias, residual, y, kh, kw, stride, pad, act, w_layout, w_planes_f16, w_exp, x_absmax,
                           y_absmax, out_scale, 0, None), "conv_bn_act_x2")
        elif w_planes is not None:
            check(_lib.lib().dbmm_conv_bn_act_x3(ptr(x), ptr(w), ptr(w_planes), ptr(bias), ptr(residual), ptr(y), B, H, W,
                                                 Cin, Cout, kh, kw, stride, pad, act, int(w_layout), ptr(ws),
                                                 ws.numel() * 4, stream()), "conv_bn_act_x3")
        else:
            check(_lib.lib().dbmm_conv_bn_act_ws(ptr(x), ptr(w), ptr(bias), ptr(residual), ptr(y), B, H, W, Cin, Cout, kh,
                                                 kw, stride, pad, act, int(w_layout), ptr(ws), ws.numel() * 4, stream()),
                  "conv_bn_act")
    if pool == 2:      # (y_absmax of the unpooled map bounds the pooled one)
        return (avgpool2d(y, 2), y) if keep_full else avgpool2d(y, 2)
    return y


def _conv_x2(x, w, bias, residual, y, kh, kw, stride, pad, act, w_layout, w_planes_f16, w_exp, x_absmax, y_absmax,
             out_scale, pool, y_full):
    B, H, W, Cin = x.shape
    ws = igemm_workspace(x.device)
    nw = 2 if w_planes_f16 is None else int(w_planes_f16.shape[0])
    return _lib.lib().dbmm_conv_bn_act_x2(ptr(x), ptr(x_absmax), ptr(w), ptr(w_planes_f16), nw, int(w_exp), ptr(out_scale),
                                          ptr(bias), ptr(residual), ptr(y), ptr(y_full), ptr(y_absmax), B, H, W, Cin,
                                          w.shape[0], kh,
                                          kw, stride, pad, act, pool, int(w_layout), ptr(ws), ws.numel() * 4, stream())


def gemm_dual(a, a_absmax, w_plane, w_exp, out_scale, a2, a2_absmax, w2_plane, ratio, bias, act=ACT_RELU, c_absmax=None):
    """c = act((a @ w^T) * out_scale + (a2 @ w2^T) * out_scale2 + bias) as one launch -- conv3 and the
    downsample branch of a bottleneck's first block (see dbmm_gemm_dual_bn_act_x2).  a [.., K],
    a2 [.., K2] with the same leading shape; planes [1][N][K] / [1][N][K2].  Returns None when the
    library has no kernel for the shape (the caller then runs the two convs)."""
    require_cuda(a, a2)
    _f32c(a); _f32c(a2)
    K, K2 = a.shape[-1], a2.shape[-1]
    M, N = a.numel() // K, _rank("gemm_dual w_plane", w_plane, 3).shape[1]
    if a2.numel() // K2 != M:
        raise _lib.DbmmError("gemm_dual: operand row counts differ")
    _operand("gemm_dual w_plane", w_plane, torch.float16, (1, N, K)); _operand("gemm_dual w2_plane", w2_plane, torch.float16, (1, N, K2))
    _operand("gemm_dual out_scale", out_scale, torch.float32, N); _operand("gemm_dual ratio", ratio, torch.float32, N)
    _operand("gemm_dual bias", bias, torch.float32, N)
    _absmax("gemm_dual a_absmax", a_absmax, True); _absmax("gemm_dual a2_absmax", a2_absmax, True); _absmax("gemm_dual c_absmax", c_absmax)
    c = _empty(tuple(a.shape[:-1]) + (N,), device=a.device, dtype=torch.float32)
    ws = igemm_workspace(a.device)
    t = _Timed(M, N, K + K2, 0, 0, 4 * (M * K + M * K2 + M * N) + 2 * (N * K + N * K2))
    t.__enter__()
    rc = _lib.lib().dbmm_gemm_dual_bn_act_x2(ptr(a), K, ptr(a_absmax), ptr(w_plane), int(w_exp), K, K, ptr(out_scale),
                                             ptr(a2), K2, ptr(a2_absmax), ptr(w2_plane), K2, K2, ptr(ratio), ptr(bias),
                                             ptr(c), N, ptr(c_absmax), M, N, act, ptr(ws), ws.numel() * 4, stream())
    if rc == _lib.E_UNSUPPORTED:
        return None
    check(rc, "gemm_dual_bn_act_x2")
    t.__exit__(None, None, None)
    return c


def bottleneck_chain(y2, y2_absmax, c3, residual, c1, x_absmax=None, y1_absmax=None, pooled=False, keep_full=True):
    """x' = relu(bn3(conv3(y2)) + residual); y1' = relu(bn1'(conv1'(x'))) in ONE launch (dbmm_bottleneck_chain_x2);
    c3 / c1 = plan entries of the two 1x1 convs (single exact fp16 plane `ph`, `we`, `sc`, `b`).  y2 NHWC [B,H,W,K].
    Returns (x', y1') or (x', x'_pooled, y1') with pooled=True -- x' is None with keep_full=False (pooled only: the un-pooled
    tensor is not written); None when the library has no kernel for the shape (the caller then runs the two convs)."""
    require_cuda(y2, residual)
    _f32c(y2); _f32c(residual)
    B, H, W, K = y2.shape
    N, P = _rank("bottleneck_chain c3 plane", c3["ph"], 3).shape[1], _rank("bottleneck_chain c1 plane", c1["ph"], 3).shape[1]
    if c3["ph"].shape[0] != 1 or c1["ph"].shape[0] != 1 or tuple(residual.shape) != (B, H, W, N):
        return None
    chain8 = K == 256 and P == 256 and not pooled and get_option("chain8")       # the layer-3 geometry: eight-wave kernel
    if not chain8 and (K not in (64, 128) or P not in (64, 128)):                 # shapes the library serves
        return None
    if N % 64 or (pooled and (H % 2 or W % 2)):
        return None
    _plane("bottleneck_chain c3", c3, N, K); _plane("bottleneck_chain c1", c1, P, N)
    _absmax("bottleneck_chain y2_absmax", y2_absmax, True); _absmax("bottleneck_chain x_absmax", x_absmax)
    _absmax("bottleneck_chain y1_absmax", y1_absmax)
    dev = y2.device
    full = keep_full or not pooled
    x = _empty((B, H, W, N), device=dev, dtype=torch.float32) if full else None
    y1 = _empty((B, H, W, P), device=dev, dtype=torch.float32)
    xp = _empty((B, H // 2, W // 2, N), device=dev, dtype=torch.float32) if pooled else None
    M = B * H * W
    # tagged like an igemm launch for bench.py's per-kernel table: FLOPs of both GEMMs, algorithmic bytes
    global _chain_tag
    _chain_tag = "bottleneck_chain8_kernel" if chain8 else f"bottleneck_chain_kernel<{K}, {P}, {int(pooled) + int(not full)}, 0>"
    t = _Timed(M, N, K + P, -1, 0, 4 * (M * K + (2 if full else 1) * M * N + M * P + (M // 4 * N if pooled else 0)) + 2 * (N * K + P * N))
    t.__enter__()
    rc = _lib.lib().dbmm_bottleneck_chain_x2(ptr(y2), ptr(y2_absmax), ptr(c3["ph"]), int(c3["we"]), ptr(c3["sc"]), ptr(c3["b"]),
                                            ptr(residual), ptr(x), ptr(xp), ptr(x_absmax), ptr(c1["ph"]), int(c1["we"]),
                                            ptr(c1["sc"]), ptr(c1["b"]), ptr(y1), ptr(y1_absmax), B, H, W, K, N, P, stream())
    if rc == _lib.E_UNSUPPORTED:
        return None
    check(rc, "bottleneck_chain_x2")
    t.__exit__(None, None, None)
    return (x, xp, y1) if pooled else (x, y1)


_chain_tag = None


def bottleneck_block_chain(y1, y1_absmax, c2, c3, c1, residual=None, dual=None, x_absmax=None, y1n_absmax=None):
    """one stride-1 bottleneck block from its conv1 output on, continued into the next block's conv1, ONE launch
    (dbmm_bottleneck_block_chain_x2): y1 -> conv2 3x3 -> conv3 + residual (or, dual = dict(a2, a2_absmax, ds, ratio, bias):
    + downsample branch) -> x' -> conv1' -> y1'.  c2 / c3 / c1 = plan entries (c2 in the chunk32-major K order).
    Returns (x', y1') or None when the library has no kernel for the shape."""
    require_cuda(y1)
    _f32c(y1)
    B, H, W, K = y1.shape
    N, P = _rank("bottleneck_block_chain c3 plane", c3["ph"], 3).shape[1], _rank("bottleneck_block_chain c1 plane", c1["ph"], 3).shape[1]
    M = B * H * W
    if (c2["ph"] is None or c2["ph"].shape[0] != 1 or c2["wl"] != WL_CHUNK32_MAJOR or tuple(c2["ph"].shape[1:]) != (K, 9 * K)
            or c3["ph"].shape[0] != 1 or c1["ph"].shape[0] != 1 or N % 64 or M % 4):
        return None
    if dual is None:
        if (K, P) not in ((64, 64), (128, 128)) or residual is None or tuple(residual.shape) != (B, H, W, N):
            return None
    elif (K, P) != (64, 64) or dual["ds"]["ph"].shape[0] != 1 or tuple(dual["a2"].shape) != (B, H, W, 64):
        return None
    _plane("bottleneck_block_chain c2", c2, K, 9 * K); _plane("bottleneck_block_chain c1", c1, P, N)
    _absmax("bottleneck_block_chain y1_absmax", y1_absmax, True); _absmax("bottleneck_block_chain x_absmax", x_absmax)
    _absmax("bottleneck_block_chain y1n_absmax", y1n_absmax)
    if dual is None:
        _plane("bottleneck_block_chain c3", c3, N, K)
        _operand("bottleneck_block_chain residual", residual, torch.float32, (B, H, W, N))
    else:
        _operand("bottleneck_block_chain c3 plane", c3["ph"], torch.float16, (1, N, K))
        _operand("bottleneck_block_chain c3 scale", c3["sc"], torch.float32, N)
        _operand("bottleneck_block_chain dual a2", dual["a2"], torch.float32, (B, H, W, 64))
        _absmax("bottleneck_block_chain dual a2_absmax", dual["a2_absmax"], True)
        _operand("bottleneck_block_chain dual ds plane", dual["ds"]["ph"], torch.float16, (1, N, 64))
        _operand("bottleneck_block_chain dual ratio", dual["ratio"], torch.float32, N)
        _operand("bottleneck_block_chain dual bias", dual["bias"], torch.float32, N)
    x = _empty((B, H, W, N), device=y1.device, dtype=torch.float32)
    y1n = _empty((B, H, W, P), device=y1.device, dtype=torch.float32)
    global _chain_tag
    _chain_tag = f"bottleneck_chain_kernel<{K}, {P}, 0, {int(dual is not None)}, 1>"
    K2 = 64 if dual is not None else 0
    nby = 4 * (M * K + M * N * (1 if dual is not None else 2) + M * K2 + M * P) + 2 * (K * 9 * K + N * K + N * K2 + P * N)
    t = _Timed(M, 1, 9 * K * K + N * (K + K2 + P), -1, 0, nby)
    t.__enter__()
    d = dual or {}
    bias3 = d["bias"] if dual is not None else c3["b"]
    rc = _lib.lib().dbmm_bottleneck_block_chain_x2(
        ptr(y1), ptr(y1_absmax), ptr(c2["ph"]), int(c2["we"]), ptr(c2["sc"]), ptr(c2["b"]), ptr(c3["ph"]), int(c3["we"]),
        ptr(c3["sc"]), ptr(bias3), ptr(residual) if dual is None else None, ptr(d.get("a2")), ptr(d.get("a2_absmax")),
        ptr(d["ds"]["ph"]) if dual is not None else None, ptr(d.get("ratio")), ptr(x), ptr(x_absmax), ptr(c1["ph"]), int(c1["we"]),
        ptr(c1["sc"]), ptr(c1["b"]), ptr(y1n), ptr(y1n_absmax), B, H, W, K, N, P, stream())
    if rc == _lib.E_UNSUPPORTED:
        return None
    check(rc, "bottleneck_block_chain_x2")
    t.__exit__(None, None, None)
    return x, y1n


def bottleneck_chain_dual(y2, y2_absmax, c3, a2, a2_absmax, ds, ratio, bias, c1, x_absmax=None, y1_absmax=None):
    """first block of a stage at unchanged resolution: x' = relu(bn3(conv3(y2)) + bn_d(conv_d(a2))), then the next
    block's y1' = relu(bn1'(conv1'(x'))), one launch (dbmm_bottleneck_chain_dual_x2).  Returns (x', y1') or None."""
    require_cuda(y2, a2)
    _f32c(y2); _f32c(a2)
    K, K2 = y2.shape[-1], a2.shape[-1]
    N, P = _rank("bottleneck_chain_dual c3 plane", c3["ph"], 3).shape[1], _rank("bottleneck_chain_dual c1 plane", c1["ph"], 3).shape[1]
    M = y2.numel() // K
    if (c3["ph"].shape[0] != 1 or ds["ph"].shape[0] != 1 or c1["ph"].shape[0] != 1 or a2.numel() // K2 != M
            or K != 64 or K2 != 64 or N % 64 or P not in (64, 128) or M % 4):
        return None
    _operand("bottleneck_chain_dual c3 plane", c3["ph"], torch.float16, (1, N, K))
    _operand("bottleneck_chain_dual c3 scale", c3["sc"], torch.float32, N)
    _operand("bottleneck_chain_dual ds plane", ds["ph"], torch.float16, (1, N, K2))
    _operand("bottleneck_chain_dual ratio", ratio, torch.float32, N); _operand("bottleneck_chain_dual bias", bias, torch.float32, N)
    _plane("bottleneck_chain_dual c1", c1, P, N)
    _absmax("bottleneck_chain_dual y2_absmax", y2_absmax, True); _absmax("bottleneck_chain_dual a2_absmax", a2_absmax, True)
    _absmax("bottleneck_chain_dual x_absmax", x_absmax); _absmax("bottleneck_chain_dual y1_absmax", y1_absmax)
    x = _empty(tuple(y2.shape[:-1]) + (N,), device=y2.device, dtype=torch.float32)
    y1 = _empty(tuple(y2.shape[:-1]) + (P,), device=y2.device, dtype=torch.float32)
    global _chain_tag
    _chain_tag = f"bottleneck_chain_kernel<{K}, {P}, 0, 1>"
    t = _Timed(M, N, K + K2 + P, -1, 0, 4 * (M * K + M * K2 + M * N + M * P) + 2 * (N * K + N * K2 + P * N))
    t.__enter__()
    rc = _lib.lib().dbmm_bottleneck_chain_dual_x2(ptr(y2), ptr(y2_absmax), ptr(c3["ph"]), int(c3["we"]), ptr(c3["sc"]), ptr(bias),
                                                 ptr(a2), ptr(a2_absmax), ptr(ds["ph"]), ptr(ratio), ptr(x), ptr(x_absmax),
                                                 ptr(c1["ph"]), int(c1["we"]), ptr(c1["sc"]), ptr(c1["b"]), ptr(y1),
                                                 ptr(y1_absmax), M, K, K2, N, P, stream())
    if rc == _lib.E_UNSUPPORTED:
        return None
    check(rc, "bottleneck_chain_dual_x2")
    t.__exit__(None, None, None)
    return x, y1


def conv_stem_s2(x_nchw, w, bias, y_absmax=None):
    require_cuda(x_nchw, w)
    _f32c(x_nchw); _f32c(w)
    B, C, H, W = x_nchw.shape
    if C != 3:
        raise _lib.DbmmError("stem conv expects 3 input channels")
    Cout = w.shape[-1]
    _operand("conv_stem_s2 weight", w, torch.float32, (3, 3, 3, Cout)); _operand("conv_stem_s2 bias", bias, torch.float32, Cout)
    _absmax("conv_stem_s2 y_absmax", y_absmax)
    y = _empty((B, (H - 1) // 2 + 1, (W - 1) // 2 + 1, Cout), device=x_nchw.device, dtype=torch.float32)
    check(_lib.lib().dbmm_conv_stem_s2(ptr(x_nchw), ptr(w), ptr(bias), ptr(y), ptr(y_absmax), B, H, W, Cout, stream()),
          "conv_stem_s2")
    return y


def avgpool2d(x, k):
    require_cuda(x)
    _f32c(x)
    B, H, W, C = x.shape
    y = _empty((B, H // k, W // k, C), device=x.device, dtype=torch.float32)
    check(_lib.lib().dbmm_avgpool2d(ptr(x), ptr(y), B, H, W, C, k, stream()), "avgpool2d")
    return y


def attnpool(x, pos, wq, bq, wkv, bkv, wc, bc, heads):
    """x NHWC [B,h,w,C] feature map, fp32 or (fp16 mode) fp16 -> fp32 [B, Dout]."""
    require_cuda(x)
    if x.dtype != torch.float16:
        _f32c(x)
    elif not x.is_contiguous():
        raise _lib.DbmmError("attnpool: expected a contiguous tensor")
    B, H, W, C = x.shape
    HW = H * W
    Dout = _rank("attnpool wc", wc, 2).shape[0]
    # the library sees raw pointers: the operand shapes are checked here.  A feature map of another resolution than the positional table
    # was built for fails like the reference's `x + self.positional_embedding[:, None, :]` (clip/model.py:72), not as a stray read
    if tuple(pos.shape) != (HW + 1, C):
        raise RuntimeError(f"attnpool: positional embedding {tuple(pos.shape)} does not match a {H} x {W} x {C} feature map "
                           f"(expected ({HW + 1}, {C})): the input resolution differs from the one the model was built for")
    if (tuple(wq.shape) != (C, C) or tuple(wkv.shape) != (2 * C, C) or wc.shape[1] != C or bq.numel() != C or bkv.numel() != 2 * C
            or bc.numel() != Dout):
        raise RuntimeError(f"attnpool: projection shapes {tuple(wq.shape)}, {tuple(wkv.shape)}, {tuple(wc.shape)} do not match C = {C}")
    for t in (pos, wq, bq, wkv, bkv, wc, bc):
        require_cuda(t)
        _f32c(t)
    nbytes = _lib.lib().dbmm_workspace_bytes_attnpool(B, HW, C)
    ws = _empty(nbytes // 4, device=x.device, dtype=torch.float32)
    out = _empty((B, Dout), device=x.device, dtype=torch.float32)
    check(_lib.lib().dbmm_attnpool_x(ptr(x), int(x.dtype == torch.float16), ptr(pos), ptr(wq), ptr(bq), ptr(wkv), ptr(bkv), ptr(wc), ptr(bc),
                                     ptr(out), B, HW, C, heads, Dout, ptr(ws), nbytes, stream()), "attnpool")
    return out


def layernorm(x, gamma, beta, rows=None, ldx=None, eps=1e-5, y_absmax=None):
    E = gamma.numel()
    if rows is None:
        rows = x.numel() // E
    if ldx is None:
        ldx = E
    _operand("layernorm gamma", gamma, torch.float32, E); _operand("layernorm beta", beta, torch.float32, E)
    if ldx < E:
        raise RuntimeError(f"layernorm: input {tuple(x.shape)} for {rows} rows of {E} at pitch {ldx}")
    _spans("layernorm input", x, torch.float32, (rows - 1) * ldx + E)
    _absmax("layernorm y_absmax", y_absmax)
    y = _empty((rows, E), device=x.device, dtype=torch.float32)
    check(_lib.lib().dbmm_layernorm(ptr(x), ldx, ptr(gamma), ptr(beta), ptr(y), E, rows, E, eps, ptr(y_absmax), stream()),
          "layernorm")
    return y


def mha_core(qkv, B, L, E, heads, causal, qkv_absmax=None):
    """softmax(q k^T / 8) v per (image, head).  With qkv_absmax (device scalar >= max|qkv|, the qkv GEMM's c_absmax) the
    fp16-pair kernel runs (16-bit matrix cores, three partial products, fp32 accuracy); without it, or with
    option mha_x2 = 0, the fp32-input-MFMA kernel."""
    require_cuda(qkv)
    _f32c(qkv, "mha_core qkv"); _absmax("mha_core qkv_absmax", qkv_absmax)
    if qkv.numel() != B * L * 3 * E or E != heads * 64:
        raise RuntimeError(f"mha_core: qkv {tuple(qkv.shape)} for B = {B}, L = {L}, E = {E}, {heads} heads of 64")
    out = _empty((B * L, E), device=qkv.device, dtype=torch.float32)
    if qkv_absmax is not None and get_option("mha_x2"):
        with _TimedTag("mha_pair_kernel", 4.0 * B * heads * L * L * 64, 4 * (B * L * 4 * E)):
            check(_lib.lib().dbmm_mha_core_x2(ptr(qkv), ptr(qkv_absmax), ptr(out), B, L, E, heads, int(causal), stream()),
                  "mha_core_x2")
        return out
    with _TimedTag("mha_mfma_kernel", 4.0 * B * heads * L * L * 64, 4 * (B * L * 4 * E)):
        check(_lib.lib().dbmm_mha_core(ptr(qkv), ptr(out), B, L, E, heads, int(causal), stream()), "mha_core")
    return out


def _embed_gather_check(name, tokens, table, pos):
    require_cuda(tokens, table, pos)
    _f32c(table, f"{name} table"); _f32c(pos, f"{name} pos")
    if tokens.dim() != 2 or table.dim() != 2:
        raise RuntimeError(f"{name}: tokens {tuple(tokens.shape)} and table {tuple(table.shape)} where [n, L] ids and a [vocab, W] table are expected")
    if tokens.dtype != torch.int32:
        tokens = tokens.to(torch.int32)
    return tokens.contiguous()


def embed_gather(tokens, table, pos):
    tokens = _embed_gather_check("embed_gather", tokens, table, pos)
    n, L = tokens.shape
    W = table.shape[1]
    if tuple(pos.shape) != (L, W):          # (clip/model.py:346: `x + self.positional_embedding` needs context_length tokens)
        raise RuntimeError(f"embed_gather: {L} tokens per prompt against a positional embedding of shape {tuple(pos.shape)}")
    out = _empty((n, L, W), device=table.device, dtype=torch.float32)
    check(_lib.lib().dbmm_embed_gather(ptr(tokens), ptr(table), ptr(pos), ptr(out), n, L, W, table.shape[0], stream()),
          "embed_gather")
    return out, tokens


def im2col_patch(x_nchw, P, out_absmax=None):
    """[B,3,R,R] -> patch rows [B*g*g, 3*P*P]; out_absmax (1-element device tensor, zeroed by the caller) receives max|x|"""
    require_cuda(x_nchw, out_absmax)
    _f32c(x_nchw, "im2col_patch image batch")
    _patch_image_check("im2col_patch", x_nchw, P)
    if out_absmax is not None and (out_absmax.dtype != torch.float32 or out_absmax.numel() != 1):
        raise RuntimeError(f"im2col_patch out_absmax: one float32 element expected, got {out_absmax.dtype} {tuple(out_absmax.shape)}")
    B, C, R, _ = x_nchw.shape
    g = R // P
    out = _empty((B * g * g, 3 * P * P), device=x_nchw.device, dtype=torch.float32)
    check(_lib.lib().dbmm_im2col_patch(ptr(x_nchw), ptr(out), ptr(out_absmax), B, R, P, stream()), "im2col_patch")
    return out


def _vit_tokens_check(patches, cls, pos, B, patch_dtype=torch.float32):
    # raw pointers below: a patch count other than the positional table's (another input resolution) fails like the reference's
    # `x + self.positional_embedding` (clip/model.py:229), not as a stray read
    require_cuda(patches, cls, pos)
    if pos.dim() != 2:
        raise RuntimeError(f"vit_tokens: positional embedding of shape {tuple(pos.shape)} where [L, W] is expected")
    L, W = pos.shape
    if patches.numel() != B * (L - 1) * W or cls.numel() != W:
        raise RuntimeError(f"vit_tokens: {patches.numel() // max(1, B * W)} patches of width {W} per image do not match a positional embedding of "
                           f"{L} rows: the input resolution differs from the one the model was built for")
    _f32c(cls, "vit_tokens cls"); _f32c(pos, "vit_tokens pos")
    if patches.dtype != patch_dtype or not patches.is_contiguous():
        raise _lib.DbmmError(f"vit_tokens patches {tuple(patches.shape)}: expected a contiguous {patch_dtype} tensor, got {patches.dtype} "
                             f"contiguous={patches.is_contiguous()}")


def vit_tokens(patches, cls, pos, B):
    _vit_tokens_check(patches, cls, pos, B)
    L, W = pos.shape
    out = _empty((B, L, W), device=patches.device, dtype=torch.float32)
    check(_lib.lib().dbmm_vit_tokens(ptr(patches), ptr(cls), ptr(pos), ptr(out), B, L, W, stream()), "vit_tokens")
    return out


def _gather_eot_check(name, tokens_i32, x, dtype):
    require_cuda(tokens_i32, x)
    if x.dim() != 3 or x.dtype != dtype or not x.is_contiguous():
        raise _lib.DbmmError(f"{name} x: expected a contiguous {dtype} tensor [n, L, W], got {x.dtype} {tuple(x.shape)} "
                             f"contiguous={x.is_contiguous()}")
    _operand((name, "tokens"), tokens_i32, torch.int32, x.shape[:2])


def gather_eot(tokens_i32, x):
    _gather_eot_check("gather_eot", tokens_i32, x, torch.float32)
    n, L, W = x.shape
    out = _empty((n, W), device=x.device, dtype=torch.float32)
    check(_lib.lib().dbmm_gather_eot(ptr(tokens_i32), ptr(x), ptr(out), n, L, W, stream()), "gather_eot")
    return out


def text_colnorm(text):
    """[D, C] -> normalised, transposed [C, D]."""
    require_cuda(text)
    _f32c(text)
    D, C = text.shape
    tn = _empty((C, D), device=text.device, dtype=torch.float32)
    check(_lib.lib().dbmm_text_colnorm(ptr(text), ptr(tn), D, C, stream()), "text_colnorm")
    return tn


def l2norm_rows(x):
    """x / x.norm(dim=1, keepdim=True) for fp32 [B, D] (CLIP.forward, clip/model.py:362-363)"""
    require_cuda(x)
    _f32c(x)
    B, D = x.shape
    y = _empty((B, D), device=x.device, dtype=torch.float32)
    check(_lib.lib().dbmm_l2norm_rows(ptr(x), ptr(y), B, D, stream()), "l2norm_rows")
    return y


def colsum(x):
    """x.sum(0) of fp32 [B, N] (N % 4 == 0) in a fixed order"""
    require_cuda(x)
    _f32c(x)
    B, N = x.shape
    out = _empty((N,), device=x.device, dtype=torch.float32)
    check(_lib.lib().dbmm_colsum(ptr(x), ptr(out), B, N, stream()), "colsum")
    return out


def l2norm_sim_ce_fwd(z, tn, temperature, labels=None, z_old=None, ebd_weight=0.5, want_loss=True, want_pred=False, want_mean=True):
    require_cuda(z, tn)
    _f32c(z)
    B, D = z.shape
    C = tn.shape[0]
    dev = z.device
    logits = _empty((B, C), device=dev, dtype=torch.float32)
    inv_norm = _empty((B,), device=dev, dtype=torch.float32)
    loss_rows = loss_mean = pred = None
    if labels is not None and want_loss:
        loss_rows = _empty((B,), device=dev, dtype=torch.float32)
        loss_mean = _empty((), device=dev, dtype=torch.float32) if want_mean else None      # (the mean is a launch of its own)
    if want_pred:
        pred = _empty((B,), device=dev, dtype=torch.int64)
    check(_lib.lib().dbmm_l2norm_sim_ce_fwd(ptr(z), ptr(z_old), float(ebd_weight), ptr(tn), ptr(labels),
                                            float(temperature), ptr(logits), ptr(loss_rows), ptr(loss_mean), ptr(pred),
                                            ptr(inv_norm), B, D, C, stream()), "l2norm_sim_ce_fwd")
    return logits, loss_rows, loss_mean, pred, inv_norm


def l2norm_sim_ce_bwd(z, inv_norm, tn, temperature, logits=None, labels=None, dlogits=None, blended=False,
                      ebd_weight=0.5, grad_scale=1.0):
    B, D = z.shape
    C = tn.shape[0]
    dz = _empty(tuple(z.shape), device=z.device, dtype=z.dtype)
    check(_lib.lib().dbmm_l2norm_sim_ce_bwd(ptr(z), ptr(inv_norm), float(ebd_weight), int(blended), ptr(tn), ptr(logits),
                                            ptr(labels), ptr(dlogits), float(temperature), float(grad_scale), ptr(dz),
                                            B, D, C, stream()), "l2norm_sim_ce_bwd")
    return dz


GDRO_MAX_GROUPS = 8


def _gdro_operands(groups, q, B, R=None):
    """the group ids of a batch and the group-DRO state q ([G], or [R, G] for R replicas) as the library will index them"""
    require_cuda(groups, q)
    if groups.dtype != torch.int64 or not groups.is_contiguous():
        raise _lib.DbmmError("group DRO: groups must be a contiguous int64 tensor")
    if B is not None:
        _sized("group DRO groups", groups, B)
    _f32c(q)
    if q.dim() != (1 if R is None else 2) or (R is not None and q.shape[0] != R) or not 1 <= q.shape[-1] <= GDRO_MAX_GROUPS:
        want = "[G]" if R is None else f"[{R}, G]"
        raise _lib.DbmmError(f"group DRO: q must be a float32 {want} tensor with 1 <= G <= {GDRO_MAX_GROUPS}, got {tuple(q.shape)}")
    return q.shape[-1]


def group_dro_weights(loss_rows, groups, q, eta, q_out=None):
    """one online group-DRO update on a batch's per-row CE (dbmm_group_dro_weights): `q` [G] is updated in place, or left alone and
    the new state written to `q_out`.  Returns (robust loss (0-dim), stats [3, G]: row weights q_g / n_g | group means L_g | n_g)."""
    require_cuda(loss_rows)
    _f32c(loss_rows)
    B = loss_rows.shape[0]
    G = _gdro_operands(groups, q, B)
    if q_out is None:
        q_out = q
    else:
        require_cuda(q_out)
        _f32c(q_out)
        _sized("group DRO q_out", q_out, G)
    stats = _empty((3, G), device=loss_rows.device, dtype=torch.float32)
    robust = _empty((), device=loss_rows.device, dtype=torch.float32)
    check(_lib.lib().dbmm_group_dro_weights(ptr(loss_rows), ptr(groups), ptr(q), ptr(q_out), ptr(stats), ptr(robust), B, G, float(eta),
                                            stream()), "group_dro_weights")
    return robust, stats


def l2norm_sim_ce_bwd_weighted(z, inv_norm, tn, temperature, logits, labels, groups, weights, blended=False, ebd_weight=0.5):
    """dz of sum_b weights[groups[b]] CE_b (dbmm_l2norm_sim_ce_bwd_weighted); `weights` [G] = row 0 of group_dro_weights' stats"""
    require_cuda(z, inv_norm, tn, logits, labels, groups, weights)
    _f32c(z); _f32c(weights)
    B, D = z.shape
    C = tn.shape[0]
    _sized("l2norm_sim_ce_bwd_weighted inv_norm", inv_norm, B)
    _sized("l2norm_sim_ce_bwd_weighted logits", logits, B * C)
    _sized("l2norm_sim_ce_bwd_weighted labels", labels, B)
    G = _gdro_operands(groups, weights, B)
    dz = _empty(tuple(z.shape), device=z.device, dtype=z.dtype)
    check(_lib.lib().dbmm_l2norm_sim_ce_bwd_weighted(ptr(z), ptr(inv_norm), float(ebd_weight), int(blended), ptr(tn), ptr(logits), ptr(labels),
                                                     ptr(groups), ptr(weights), G, float(temperature), ptr(dz), B, D, C, stream()),
          "l2norm_sim_ce_bwd_weighted")
    return dz


def _row_weights(what, w, dev, n, R=None):
    """per-row loss weights as the library will index them: float32, contiguous, on the rows' device; `n` elements for a single
    step, or with `R` (a sweep) [n] / [1, n] (shared by the replicas) or [R, n] over the table's rows.  Returns Rw (1 or R).  No sync."""
    if not isinstance(w, torch.Tensor):
        raise _lib.DbmmError(f"{what}: row_weights must be a float32 tensor on the device, got {type(w).__name__}")
    require_cuda(w)
    if w.device != dev:
        raise _lib.DbmmError(f"{what}: row_weights are on {w.device}, the rows on {dev}")
    _f32c(w)
    if R is None:
        if w.dim() != 1:
            raise _lib.DbmmError(f"{what}: row_weights must be [B], got {tuple(w.shape)}")
        _sized(f"{what} row_weights", w, n)
        return 1
    if w.dim() == 1:
        _sized(f"{what} row_weights", w, n)
        return 1
    if w.dim() != 2 or w.shape[1] != n or w.shape[0] not in (1, R):
        raise _lib.DbmmError(f"{what}: row_weights must be [{n}], [1, {n}] or [{R}, {n}] over the table's rows, got {tuple(w.shape)}")
    return w.shape[0]


def weighted_mean(x, row_w):
    """(sum_i x[i] row_w[i]) / n in the order of l2norm_sim_ce_fwd's loss mean (dbmm_weighted_mean); 0-dim"""
    require_cuda(x)
    _f32c(x)
    _row_weights("weighted_mean", row_w, x.device, x.numel())
    out = _empty((), device=x.device, dtype=torch.float32)
    check(_lib.lib().dbmm_weighted_mean(ptr(x), ptr(row_w), ptr(out), x.numel(), stream()), "weighted_mean")
    return out


def l2norm_sim_ce_bwd_rows(z, inv_norm, tn, temperature, logits, labels, row_w, blended=False, ebd_weight=0.5, grad_scale=1.0):
    """dz of (1 / B) sum_b row_w[b] CE_b (dbmm_l2norm_sim_ce_bwd_rows): l2norm_sim_ce_bwd's fused path under per-row weights [B]"""
    require_cuda(z, inv_norm, tn, logits, labels)
    _f32c(z)
    B, D = z.shape
    C = tn.shape[0]
    _sized("l2norm_sim_ce_bwd_rows inv_norm", inv_norm, B)
    _sized("l2norm_sim_ce_bwd_rows logits", logits, B * C)
    _sized("l2norm_sim_ce_bwd_rows labels", labels, B)
    _row_weights("l2norm_sim_ce_bwd_rows", row_w, z.device, B)
    dz = _empty(tuple(z.shape), device=z.device, dtype=z.dtype)
    check(_lib.lib().dbmm_l2norm_sim_ce_bwd_rows(ptr(z), ptr(inv_norm), float(ebd_weight), int(blended), ptr(tn), ptr(logits), ptr(labels),
                                                 ptr(row_w), float(temperature), float(grad_scale), ptr(dz), B, D, C, stream()),
          "l2norm_sim_ce_bwd_rows")
    return dz


SUPCON_MAX_B = 2048


def _f32(v):
    """v rounded to float32, as the C ABI's float arguments are"""
    return ctypes.c_float(v).value


def supcon_ce_weight(weight):
    """1 - weight in float32: the CE term's weight exactly as the library forms it from a float32 `weight`"""
    return _f32(1.0 - _f32(weight))


def _supcon_operands(z, labels, what):
    require_cuda(z, labels)
    _f32c(z)
    B, D = z.shape
    if labels.dtype != torch.int64 or not labels.is_contiguous():
        raise _lib.DbmmError(f"{what}: labels must be a contiguous int64 tensor")
    _sized(f"{what} labels", labels, B)
    if B > SUPCON_MAX_B:
        raise DbmmUnsupported(f"{what}: B = {B}; the contrastive head serves 2 <= B <= {SUPCON_MAX_B}")
    return B, D


def supcon_fwd(z, labels, tau, ce_rows=None, weight=0.0):
    """supervised-contrastive loss of the rows of z [B, D] under `labels` at temperature `tau` (dbmm_supcon_fwd, 2 launches).
    Returns (L_con (0-dim), per-row l [B], stats [4, B], A (0-dim float), workspace, mixed): stats, A and the workspace (it holds the
    similarity matrix) are what supcon_bwd needs; `mixed` = (1 - weight) * mean(ce_rows) + weight * L_con when the per-row CE of the
    batch is given, else None."""
    B, D = _supcon_operands(z, labels, "supcon_fwd")
    dev = z.device
    if ce_rows is not None:
        require_cuda(ce_rows)
        _f32c(ce_rows)
        _sized("supcon_fwd ce_rows", ce_rows, B)
    nbytes = _lib.lib().dbmm_supcon_workspace_bytes(B, D)
    ws = _empty(max(nbytes // 4, 4), device=dev, dtype=torch.float32)
    out = _empty((5 * B + 3,), device=dev, dtype=torch.float32)         # stats [4][B] | l [B] | L_con, A, mixed: one allocation
    base = out.data_ptr()
    check(_lib.lib().dbmm_supcon_fwd(ptr(z), ptr(labels), float(tau), ptr(ce_rows), float(weight), base + 20 * B,
                                     base + 20 * B + 8 if ce_rows is not None else None, base + 16 * B, base, base + 20 * B + 4, B, D,
                                     ptr(ws), nbytes, stream()), "supcon_fwd")
    return out[5 * B], out[4 * B:5 * B], out[:4 * B].view(4, B), out[5 * B + 1], ws, (out[5 * B + 2] if ce_rows is not None else None)


def supcon_bwd(z, labels, tau, stats, n_anchors, ws, weight=1.0, dz_in=None, dz_in_scale=1.0):
    """dz = dz_in_scale * dz_in + weight * dL_con/dz (dbmm_supcon_bwd, 1 launch) from supcon_fwd's stats, A and workspace"""
    B, D = _supcon_operands(z, labels, "supcon_bwd")
    require_cuda(stats, n_anchors, ws)
    _f32c(stats)
    _sized("supcon_bwd stats", stats, 4 * B)
    if dz_in is not None:
        require_cuda(dz_in)
        _f32c(dz_in)
        _sized("supcon_bwd dz_in", dz_in, B * D)
    dz = _empty((B, D), device=z.device, dtype=torch.float32)
    check(_lib.lib().dbmm_supcon_bwd(ptr(z), ptr(labels), float(tau), ptr(stats), ptr(n_anchors), float(weight), ptr(dz_in),
                                     float(dz_in_scale), ptr(dz), B, D, ptr(ws), ws.numel() * 4, stream()), "supcon_bwd")
    return dz


SETS_CHUNK_ROWS = 32        # rows of a set one workgroup of the sets head takes (csrc/supcon_sets.hip: SETS_ROWS)
SETS_MAX_D = 8192


def _sets_operands(z, sets, what):
    """(T, A, P, N, D) of z [T * (A + P + N), D] under `sets` = (T, A, P, N)"""
    require_cuda(z)
    _f32c(z)
    T, A, P, N = (int(v) for v in sets)
    if min(T, A, P, N) < 1:
        raise ValueError(f"{what}: sets=(T, A, P, N) must all be at least 1, got {tuple(sets)!r}")
    if z.dim() != 2 or z.shape[0] != T * (A + P + N):
        raise RuntimeError(f"{what}: {tuple(z.shape)} rows where sets={tuple(sets)!r} means {T * (A + P + N)} rows of one width")
    if z.shape[1] > SETS_MAX_D:
        raise DbmmUnsupported(f"{what}: D = {z.shape[1]}; the sets head serves D <= {SETS_MAX_D}")
    return T, A, P, N, z.shape[1]


def supcon_sets_fwd(z, sets, scale, tau):
    """contrastive loss of T sampled sets (dbmm_supcon_sets_fwd, 2 launches): z [T * S, D], `sets` = (T, A, P, N), S = A + P + N; row 0
    of a set is the anchor, rows A .. A+P-1 the positives, the last N rows the negatives.  Returns (L = scale * sum_t l_t (0-dim),
    l_t [T], workspace); the workspace is what supcon_sets_bwd needs."""
    T, A, P, N, D = _sets_operands(z, sets, "supcon_sets_fwd")
    nbytes = _lib.lib().dbmm_supcon_sets_workspace_bytes(T, A + P + N, D)
    ws = _empty(max(nbytes // 4, 4), device=z.device, dtype=torch.float32)
    out = _empty((T + 1,), device=z.device, dtype=torch.float32)          # l_t, then L: one allocation
    check(_lib.lib().dbmm_supcon_sets_fwd(ptr(z), float(scale), float(tau), out.data_ptr() + 4 * T, ptr(out), T, A, P, N, D, ptr(ws), nbytes,
                                          stream()), "supcon_sets_fwd")
    return out[T], out[:T], ws


def supcon_sets_bwd(z, sets, scale, tau, ws):
    """dz = dL/dz (dbmm_supcon_sets_bwd, 2 launches) from supcon_sets_fwd's workspace; the rows of extra anchors are zero"""
    T, A, P, N, D = _sets_operands(z, sets, "supcon_sets_bwd")
    require_cuda(ws)
    _f32c(ws)
    dz = _empty((z.shape[0], D), device=z.device, dtype=torch.float32)
    check(_lib.lib().dbmm_supcon_sets_bwd(ptr(z), float(scale), float(tau), ptr(dz), T, A, P, N, D, ptr(ws), ws.numel() * 4, stream()),
          "supcon_sets_bwd")
    return dz


def gather_sets(table, idx):
    """the rows of T sampled sets as one batch: out[t * S + j] = table[idx[t, j]] for int64 idx [T, S] on the table's device"""
    require_cuda(table, idx)
    if idx.dtype != torch.int64 or idx.dim() != 2:
        raise _lib.DbmmError(f"gather_sets: idx must be an int64 tensor [T, S], got {idx.dtype} {tuple(idx.shape)}")
    return gather_rows(table, idx.reshape(-1))


_step_ws, _sets_ws = {}, {}


def _cached_ws(cache, limit, key, dev, nbytes):
    """the workspace of the one-call steps of shape `key`: from `cache`, or allocated with nbytes(*key[1:]) bytes and kept there; a
    cache that already holds more than `limit` workspaces is emptied first"""
    ws = cache.get(key)
    if ws is None:
        ws = _empty(max(nbytes(*key[1:]) // 4, 4), device=dev, dtype=torch.float32)      # 0 bytes: a shape the library refuses by name
        if len(cache) > limit:
            cache.clear()
        cache[key] = ws
    return ws


def _step_ws_bytes(B, D, H, with_old, contrastive):
    L = _lib.lib()
    return L.dbmm_workspace_bytes_adapter_train_step(B, D, H, int(with_old)) + (L.dbmm_supcon_workspace_bytes(B, D) if contrastive else 0)


def adapter_train_step_sets(x, args, H, sets, scale, tau, lr, momentum, weight_decay, first_step):
    """one step of the contrastive adapter on T sampled sets in one call (dbmm_adapter_train_step_sets): adapter forward with
    train-mode BatchNorm over the T * S rows as one batch, the sets head forward and backward, adapter backward, SGD.  `args`: the
    first 15 pointers of adapter_step_args().  Returns (L, l_t [T]).  Raises DbmmUnsupported off the adapter's fast shape."""
    T, A, P, N, D = _sets_operands(x, sets, "adapter_train_step_sets")
    S = A + P + N
    dev = x.device
    ws = _cached_ws(_sets_ws, 4, (dev.index, T, S, D, H), dev, _lib.lib().dbmm_workspace_bytes_adapter_train_step_sets)
    out = _empty((T + 1,), device=dev, dtype=torch.float32)
    rc = _lib.lib().dbmm_adapter_train_step_sets(x.data_ptr(), *args[:15], float(lr), float(momentum), float(weight_decay), int(first_step),
                                                 float(scale), float(tau), out.data_ptr() + 4 * T, out.data_ptr(), T, A, P, N, D, H,
                                                 ws.data_ptr(), ws.numel() * 4, stream())
    if rc == _lib.E_UNSUPPORTED:
        raise DbmmUnsupported(f"adapter_train_step_sets: no one-call step for D = {D}, H = {H}, {T * S} rows (the adapter's fast shape: "
                              "H == 128, D % 128 == 0); use sets_loss(...).backward() and optimizer.step()")
    if rc:
        check(rc, "adapter_train_step_sets")
    return out[T], out[:T]


def adapter_fwd(x, w1, b1, gamma, beta, running_mean, running_var, nbt, w2, b2, train, eps=1e-5, momentum=0.1):
    require_cuda(x, w1)
    _f32c(x)
    B, D = x.shape
    H = w1.shape[0]
    # the library refuses these too (DBMM_E_SHAPE, before its first launch); here the message can name the limit
    if D % 4 or H % 4:
        raise _lib.DbmmError(f"adapter_fwd: input width {D} and hidden width {H}: both must be multiples of 4 (the kernels read and "
                             "write rows in 16-byte pieces)")
    if train and B < 2:
        raise _lib.DbmmError(f"adapter_fwd: train-mode BatchNorm1d needs at least 2 rows, got {B}")
    dev = x.device
    h = _empty((B, H), device=dev, dtype=torch.float32)
    r = _empty((B, H), device=dev, dtype=torch.float32)
    z = _empty((B, D), device=dev, dtype=torch.float32)
    mean = _empty((H,), device=dev, dtype=torch.float32) if train else None
    invstd = _empty((H,), device=dev, dtype=torch.float32) if train else None
    check(_lib.lib().dbmm_adapter_fwd(ptr(x), ptr(w1), ptr(b1), ptr(gamma), ptr(beta), ptr(running_mean),
                                      ptr(running_var), ptr(nbt), ptr(w2), ptr(b2), ptr(h), ptr(mean), ptr(invstd),
                                      ptr(r), ptr(z), B, D, H, int(train), eps, momentum, stream()), "adapter_fwd")
    return z, h, mean, invstd, r


def adapter_bwd(x, dz, h, mean, invstd, r, gamma, beta, w2):
    B, D = x.shape
    H = h.shape[1]
    dev = x.device
    f = dict(device=dev, dtype=torch.float32)
    dw1, db1 = _empty((H, D), **f), _empty((H,), **f)
    dgamma, dbeta = _empty((H,), **f), _empty((H,), **f)
    dw2, db2 = _empty((D, H), **f), _empty((D,), **f)
    nbytes = _lib.lib().dbmm_workspace_bytes_adapter_bwd(B, D, H)
    ws = _empty(nbytes // 4, **f)
    check(_lib.lib().dbmm_adapter_bwd(ptr(x), ptr(dz), ptr(h), ptr(mean), ptr(invstd), ptr(r), ptr(gamma), ptr(beta),
                                      ptr(w2), ptr(dw1), ptr(db1), ptr(dgamma), ptr(dbeta), ptr(dw2), ptr(db2), B, D, H,
                                      ptr(ws), nbytes, stream()), "adapter_bwd")
    return dw1, db1, dgamma, dbeta, dw2, db2, ws[B * H:2 * B * H].view(B, H)   # last = dh (for an optional dx)


def sgd_momentum(params, grads, bufs, lr, momentum, weight_decay, first_step):
    n = len(params)
    for i in range(0, n, 16):
        ps, gs, bs = params[i:i + 16], grads[i:i + 16], bufs[i:i + 16]
        m = len(ps)
        P = (ctypes.c_void_p * m)(*[p.data_ptr() for p in ps])
        G = (ctypes.c_void_p * m)(*[g.data_ptr() for g in gs])
        Bf = (ctypes.c_void_p * m)(*[b.data_ptr() for b in bs])
        S = (ctypes.c_int64 * m)(*[p.numel() for p in ps])
        check(_lib.lib().dbmm_sgd_momentum(m, P, G, Bf, S, float(lr), float(momentum), float(weight_decay),
                                           int(first_step), stream()), "sgd_momentum")


def group_count(logits, y, g, counts):
    """counts int64 [G,2] accumulated in place: (n, correct) per group."""
    require_cuda(logits)
    _f32c(logits, "group_count logits")
    if logits.dim() != 2 or counts.dim() != 2 or counts.shape[0] > 64:
        raise RuntimeError(f"group_count: logits {tuple(logits.shape)} and counts {tuple(counts.shape)} where [B, C] and [G, 2] with "
                           f"G <= 64 are expected")
    B, C = logits.shape
    _operand("group_count y", y, torch.int64, B)
    _operand("group_count g", g, torch.int64, B)
    _operand("group_count counts", counts, torch.int64, (counts.shape[0], 2))
    check(_lib.lib().dbmm_group_count(ptr(logits), ptr(y), ptr(g), ptr(counts), B, C, counts.shape[0], stream()),
          "group_count")
    return counts


def group_loss_sum(loss_rows, g, sums):
    """sums float32 [G] accumulated in place: the sum of loss_rows over the rows of each group."""
    require_cuda(loss_rows, sums)
    _f32c(loss_rows, "group_loss_sum loss_rows"); _f32c(sums, "group_loss_sum sums")
    B, G = loss_rows.numel(), sums.numel()
    if G > 64:
        raise RuntimeError(f"group_loss_sum sums {tuple(sums.shape)}: the kernel takes at most 64 groups")
    _operand("group_loss_sum g", g, torch.int64, B)
    check(_lib.lib().dbmm_group_loss_sum(ptr(loss_rows), ptr(g), ptr(sums), B, G, stream()), "group_loss_sum")
    return sums


def adapter_step_launches(B, D, H, with_old=False, robust=False, contrastive=False, weighted=False):
    """kernel launches of one dbmm_adapter_train_step call on the purpose-built kernels (csrc/adapter_step.hip): forward 3
    (K-split fc1, BatchNorm statistics, BatchNorm + ReLU + fc2; 3 more for a frozen old adapter), cosine logits + CE forward
    and backward in one, backward 3 (dW2 / dr + the loss mean, BatchNorm backward + dW2 sums, dW1), SGD (+ dW1 sums); None for
    shapes that take the general GEMM kernel (H != 128 or D % 128 != 0).  `robust` (dbmm_adapter_train_step_gdro): 2 more -- the
    head is forward rows, group reduction + q update, weighted backward rows, and the loss needs no launch of the backward.
    `contrastive` (dbmm_adapter_train_step_supcon): 3 more -- Gram tiles, the reduction + the mixed loss, the contrastive backward.
    `weighted` (dbmm_adapter_train_step_weighted): none more -- fixed per-row weights need no batch reduction, the head and the
    backward's spare block read them in the launches ERM has"""
    if H != 128 or D % 128 or not get_option("adapter_step_fused"):
        return None
    if weighted and (robust or contrastive):
        raise DbmmUnsupported("adapter_step_launches: per-row weights do not combine with group DRO or the contrastive head")
    return 8 + (3 if with_old else 0) + (2 if robust else 0) + (3 if contrastive else 0)


def adapter_step_args(new, bufs, old):
    """the 24 parameter / buffer pointers of dbmm_adapter_train_step, converted once: `new` / `old` are tuples
    (w1, b1, gamma, beta, running_mean, running_var, nbt, w2, b2); `bufs` the six momentum buffers in the order
    (w1, b1, gamma, beta, w2, b2); `old` may be None.  Valid while those tensors keep their storage."""
    require_cuda(*new)
    return tuple(ptr(t) for t in list(new) + list(bufs)) + (tuple(ptr(t) for t in old) if old is not None else (None,) * 9)


def adapter_train_step(x, labels, args, H, with_old, ebd_weight, tn, temperature, lr, momentum, weight_decay, first_step, robust=None,
                       contrastive=None, row_weights=None):
    """one fused training-step body (dbmm_adapter_train_step); `args` from adapter_step_args().  `robust` = (groups int64 [B], q
    float32 [G], eta): the group-DRO step (dbmm_adapter_train_step_gdro) -- q is updated in place, the returned loss is the robust
    loss.  `contrastive` = (weight, tau): the step with the supervised-contrastive head (dbmm_adapter_train_step_supcon); returns
    (mixed loss, logits, per-row CE, L_con).  `row_weights` float32 [B]: the step under per-row loss weights
    (dbmm_adapter_train_step_weighted) -- the returned loss is (1 / B) sum_b w_b CE_b, logits and per-row CE are the unweighted ones."""
    if not (x.is_cuda and labels.is_cuda and tn.is_cuda):
        require_cuda(x, labels, tn)
    _f32c(x)
    B, D = x.shape
    C = tn.shape[0]
    dev = x.device
    if contrastive is not None:
        if robust is not None:
            raise DbmmUnsupported("adapter_train_step: the contrastive head and group DRO do not combine")
        if B > SUPCON_MAX_B:
            raise DbmmUnsupported(f"adapter_train_step: B = {B}; the contrastive head serves 2 <= B <= {SUPCON_MAX_B}")
    if row_weights is not None:
        if robust is not None or contrastive is not None:
            raise DbmmUnsupported("adapter_train_step: per-row weights do not combine with group DRO or the contrastive head")
        _row_weights("adapter_train_step", row_weights, dev, B)
    L = _lib.lib()
    ws = _cached_ws(_step_ws, 8, (dev.index, B, D, H, with_old, contrastive is not None), dev, _step_ws_bytes)
    logits = _empty((B, C), device=dev, dtype=torch.float32)
    # per-row losses, then their mean (the robust / the mixed loss), then L_con of the contrastive head: one allocation
    loss = _empty((B + (1 if contrastive is None else 2),), device=dev, dtype=torch.float32)
    if contrastive is not None:
        weight, tau = contrastive
        step, name = L.dbmm_adapter_train_step_supcon, "adapter_train_step_supcon"
        head = (float(weight), float(tau), loss.data_ptr() + 4 * B + 4)
    elif robust is not None:
        groups, q, eta = robust
        step, name = L.dbmm_adapter_train_step_gdro, "adapter_train_step_gdro"
        head = (groups.data_ptr(), q.data_ptr(), float(eta), _gdro_operands(groups, q, B))
    elif row_weights is not None:
        step, name, head = L.dbmm_adapter_train_step_weighted, "adapter_train_step_weighted", (row_weights.data_ptr(),)
    else:
        step, name, head = L.dbmm_adapter_train_step, "adapter_train_step", ()
    # the 36 arguments every head shares, the head's own, the shape and the workspace
    rc = step(x.data_ptr(), labels.data_ptr(), *args, float(ebd_weight), tn.data_ptr(), float(temperature), float(lr), float(momentum),
              float(weight_decay), int(first_step), logits.data_ptr(), loss.data_ptr(), loss.data_ptr() + 4 * B, *head, B, D, H, C, ws.data_ptr(),
              ws.numel() * 4, stream())
    if rc:
        check(rc, name)
    return (loss[B], logits, loss[:B]) if contrastive is None else (loss[B], logits, loss[:B], loss[B + 1])


_sweep_ws = {}


def _sweep_workspace(dev, nbytes):
    ws = _sweep_ws.get(dev.index)
    if ws is None or ws.numel() * 4 < nbytes:
        ws = _empty(max((nbytes + 3) // 4, 4), device=dev, dtype=torch.float32)     # 0 bytes: a shape the library will refuse by name
        _sweep_ws[dev.index] = ws
    return ws


def adapter_sweep_args(R, D, H, new, bufs, old=None):
    """the pointer arrays of dbmm_adapter_sweep_step / _eval, built and shape-checked once: `new` / `old` are the nine stacked tensors
    (w1 [R, H, D], b1, gamma, beta, running_mean, running_var [R, H], nbt int64 [R], w2 [R, D, H], b2 [R, D]) of R adapters, `bufs`
    the six stacked momentum buffers in the order (w1, b1, gamma, beta, w2, b2), or None (evaluation only); `old` may be None.
    Valid while those tensors keep their storage (the arrays hold raw addresses, the tuple keeps the tensors alive)."""
    sizes = (R * H * D, R * H, R * H, R * H, R * H, R * H, R, R * D * H, R * D)
    names = ("w1", "b1", "gamma", "beta", "running_mean", "running_var", "num_batches_tracked", "w2", "b2")

    def stack(ts, what):
        ts = list(ts)
        if len(ts) != 9:
            raise _lib.DbmmError(f"adapter sweep: {what} must be the nine stacked tensors, got {len(ts)}")
        require_cuda(*ts)
        for i, (t, n, nm) in enumerate(zip(ts, sizes, names)):
            _sized(f"adapter sweep {what}.{nm}", t, n)
            want = torch.int64 if i == 6 else torch.float32
            if t.dtype != want or not t.is_contiguous():
                raise _lib.DbmmError(f"adapter sweep {what}.{nm}: expected a contiguous {want} tensor")
        return (ctypes.c_void_p * 9)(*[t.data_ptr() for t in ts]), ts

    P, keep = stack(new, "params")
    Bf = None
    if bufs is not None:
        bufs = list(bufs)
        if len(bufs) != 6:
            raise _lib.DbmmError("adapter sweep: six momentum buffers expected")
        require_cuda(*bufs)
        for t, i in zip(bufs, (0, 1, 2, 3, 7, 8)):
            _sized(f"adapter sweep momentum.{names[i]}", t, sizes[i])
            _f32c(t)
        Bf = (ctypes.c_void_p * 6)(*[t.data_ptr() for t in bufs])
        keep = keep + bufs
    O = None
    if old is not None:
        O, k2 = stack(old, "old")
        keep = keep + k2
    return dict(P=P, Bf=Bf, O=O, R=R, D=D, H=H, keep=keep)


def _sweep_tables(table, labels, groups, args):
    require_cuda(table, labels, groups)
    _f32c(table)
    if table.dim() != 2 or table.shape[1] != args["D"]:
        raise _lib.DbmmError(f"adapter sweep: table {tuple(table.shape)} for adapters of width {args['D']}")
    for nm, t in (("labels", labels), ("groups", groups)):
        if t.dtype != torch.int64 or not t.is_contiguous():
            raise _lib.DbmmError(f"adapter sweep: {nm} must be a contiguous int64 tensor")
        _sized(f"adapter sweep {nm}", t, table.shape[0])


def _sweep_metrics(counts, loss_sum, R):
    require_cuda(counts, loss_sum)
    if counts.dtype != torch.int64 or not counts.is_contiguous() or counts.dim() != 3 or counts.shape[0] != R or counts.shape[2] != 2:
        raise _lib.DbmmError(f"adapter sweep: counts must be a contiguous int64 [R, G, 2] tensor, got {tuple(counts.shape)} {counts.dtype}")
    if loss_sum.dtype != torch.float64 or not loss_sum.is_contiguous():
        raise _lib.DbmmError("adapter sweep: loss_sum must be a contiguous float64 tensor")
    _sized("adapter sweep loss_sum", loss_sum, R)
    return counts.shape[1]


def adapter_sweep_step(table, idx, labels, groups, args, ebd_weight, tn, temperature, lrs, momentum, weight_decay, first_step, counts, loss_sum,
                       counted=True, robust=None, row_weights=None):
    """one training step of R replicas in the launches of one (dbmm_adapter_sweep_step): replica r trains on rows idx[r] of `table`
    ([N, D] fp32; labels / groups int64 [N]); `args` from adapter_sweep_args(); `lrs` R host floats; counts int64 [R, G, 2] and
    loss_sum float64 [R] are accumulated in place when `counted`.  Returns (mean CE [R], logits [R, B, C], per-row CE [R, B]).
    `robust` = (q float32 [R, G], eta): the group-DRO step of every replica (dbmm_adapter_sweep_step_gdro) over the groups of
    `groups` (G = counts.shape[1] <= 8) -- q is updated in place, the robust losses take the means' place.  `row_weights` float32
    [N] / [1, N] (shared) or [R, N] over the TABLE's rows: the step under per-row loss weights (dbmm_adapter_sweep_step_weighted) --
    the losses returned and counted are (1 / B) sum_b w CE_b, the counters and per-row CE stay unweighted."""
    R, D, H = args["R"], args["D"], args["H"]
    if args["Bf"] is None:
        raise _lib.DbmmError("adapter sweep step: adapter_sweep_args() was built without momentum buffers")
    _sweep_tables(table, labels, groups, args)
    require_cuda(idx, tn)
    if idx.dtype != torch.int64 or not idx.is_contiguous() or idx.dim() != 2:
        raise _lib.DbmmError("adapter sweep step: idx must be a contiguous int64 [R, B] tensor")
    _f32c(tn)
    if tn.dim() != 2 or tn.shape[1] != D:
        raise _lib.DbmmError(f"adapter sweep: prompt matrix {tuple(tn.shape)} for width {D}")
    G = _sweep_metrics(counts, loss_sum, R)
    if len(lrs) != R:
        raise _lib.DbmmError(f"adapter sweep step: {len(lrs)} learning rates for {R} replicas")
    B, C = idx.shape[1], tn.shape[0]
    dev = table.device
    L = _lib.lib()
    ws = _sweep_workspace(dev, L.dbmm_workspace_bytes_adapter_sweep_step(R, B, D, H, int(args["O"] is not None)))
    logits = _empty((R, B, C), device=dev, dtype=torch.float32)
    loss = _empty((R, B + 1), device=dev, dtype=torch.float32)          # [:, :B] would not be contiguous: rows first, then the R means
    loss = loss.view(-1)
    LR = (ctypes.c_float * R)(*[float(v) for v in lrs])
    step, name, head = L.dbmm_adapter_sweep_step, "adapter_sweep_step", ()
    if robust is not None:
        q, eta = robust
        if _gdro_operands(groups, q, None, R) != G:
            raise _lib.DbmmError(f"adapter sweep step: q {tuple(q.shape)} for counters of {G} groups")
        step, name, head = L.dbmm_adapter_sweep_step_gdro, "adapter_sweep_step_gdro", (q.data_ptr(), float(eta))
    if row_weights is not None:
        if robust is not None:
            raise DbmmUnsupported("adapter sweep step: per-row weights do not combine with group DRO")
        Rw = _row_weights("adapter sweep step", row_weights, dev, table.shape[0], R)
        step, name, head = L.dbmm_adapter_sweep_step_weighted, "adapter_sweep_step_weighted", (row_weights.data_ptr(), Rw)
    rc = step(table.data_ptr(), table.shape[0], idx.data_ptr(), idx.shape[0], B, labels.data_ptr(), groups.data_ptr(), args["P"], args["Bf"], args["O"],
              float(ebd_weight), tn.data_ptr(), float(temperature), LR, float(momentum), float(weight_decay), int(first_step), logits.data_ptr(),
              loss.data_ptr(), loss.data_ptr() + 4 * R * B, counts.data_ptr(), loss_sum.data_ptr(), G, int(counted), *head, R, B, D, H, C,
              ws.data_ptr(), ws.numel() * 4, stream())
    if rc:
        check(rc, name)
    return loss[R * B:], logits, loss[:R * B].view(R, B)


def adapter_sweep_eval(table, idx, labels, groups, args, ebd_weight, tn, temperature, counts, loss_sum, row0=0, n=None):
    """the eval-mode forward of R replicas over the same rows (dbmm_adapter_sweep_eval): rows idx (int64 [B]) of `table`, or
    idx None: rows row0 .. row0 + n - 1.  counts int64 [R, G, 2] and loss_sum float64 [R] are accumulated in place.  Returns
    (logits [R, B, C], per-row CE [R, B])."""
    R, D, H = args["R"], args["D"], args["H"]
    _sweep_tables(table, labels, groups, args)
    require_cuda(tn)
    _f32c(tn)
    if tn.dim() != 2 or tn.shape[1] != D:
        raise _lib.DbmmError(f"adapter sweep: prompt matrix {tuple(tn.shape)} for width {D}")
    if idx is not None:
        require_cuda(idx)
        if idx.dtype != torch.int64 or not idx.is_contiguous() or idx.dim() != 1:
            raise _lib.DbmmError("adapter sweep eval: idx must be a contiguous int64 [B] tensor")
        B = idx.shape[0]
    else:
        B = table.shape[0] - row0 if n is None else n
    G = _sweep_metrics(counts, loss_sum, R)
    C = tn.shape[0]
    dev = table.device
    L = _lib.lib()
    ws = _sweep_workspace(dev, L.dbmm_workspace_bytes_adapter_sweep_eval(R, B, D, H, int(args["O"] is not None)))
    logits = _empty((R, B, C), device=dev, dtype=torch.float32)
    rows = _empty((R, B), device=dev, dtype=torch.float32)
    rc = L.dbmm_adapter_sweep_eval(table.data_ptr(), table.shape[0], ptr(idx), row0, labels.data_ptr(), groups.data_ptr(), args["P"], args["O"],
                                   float(ebd_weight), tn.data_ptr(), float(temperature), logits.data_ptr(), rows.data_ptr(), counts.data_ptr(),
                                   loss_sum.data_ptr(), G, R, B, D, H, C, ws.data_ptr(), ws.numel() * 4, stream())
    if rc:
        check(rc, "adapter_sweep_eval")
    return logits, rows


_linear_ws = {}


def _linear_workspace(dev, nbytes):
    ws = _linear_ws.get(dev.index)
    if ws is None or ws.numel() * 4 < nbytes:
        ws = _empty((nbytes + 3) // 4, device=dev, dtype=torch.float32)
        _linear_ws[dev.index] = ws
    return ws


def _linear_operands(x, labels, w, b, extra=()):
    """the shapes, dtypes and devices the linear-probe kernels assume, checked before anything launches"""
    require_cuda(x, labels, w, b, *extra)
    if x.dim() != 2 or w.dim() != 2 or b.dim() != 1 or labels.dim() != 1:
        raise _lib.DbmmError(f"linear probe: x [B, D], labels [B], w [C, D], b [C] expected; got {tuple(x.shape)}, {tuple(labels.shape)}, "
                             f"{tuple(w.shape)}, {tuple(b.shape)}")
    B, D = x.shape
    C = w.shape[0]
    for t in (x, w, b) + tuple(extra):
        _f32c(t)
    if labels.dtype != torch.int64 or not labels.is_contiguous():
        raise _lib.DbmmError("linear probe: labels must be a contiguous int64 tensor")
    if w.shape[1] != D or b.numel() != C or labels.numel() != B:
        raise _lib.DbmmError(f"linear probe: x [{B}, {D}] against w {tuple(w.shape)}, b {tuple(b.shape)}, labels {tuple(labels.shape)}")
    if B < 1 or not (1 <= C <= 8) or D % 4 or not (4 <= D <= 1024):
        raise _lib.DbmmError(f"linear probe kernels serve B >= 1, C <= 8 classes, D % 4 == 0 and D <= 1024; got B={B} C={C} D={D}")
    if any(t.device != x.device for t in (labels, w, b) + tuple(extra)):
        raise _lib.DbmmError("linear probe: all operands must be on one device")
    return B, D, C


def linear_train_step(x, labels, w, b, m_w, m_b, lr, momentum, weight_decay, first_step, row_weights=None):
    """one fused linear-probe training step (dbmm_linear_train_step): w, b, m_w, m_b updated in place.
    Returns (mean CE 0-dim, logits [B, C], per-row CE [B]), all on the device.  `row_weights` float32 [B]: the step under per-row
    loss weights (dbmm_linear_train_step_weighted) -- the loss is (1 / B) sum_b w_b CE_b, logits and per-row CE stay unweighted."""
    B, D, C = _linear_operands(x, labels, w, b, (m_w, m_b))
    if m_w.shape != w.shape or m_b.shape != b.shape:
        raise _lib.DbmmError(f"linear probe: momentum buffers {tuple(m_w.shape)}, {tuple(m_b.shape)} for w {tuple(w.shape)}, b {tuple(b.shape)}")
    dev = x.device
    L = _lib.lib()
    step, name, head = L.dbmm_linear_train_step, "linear_train_step", ()
    if row_weights is not None:
        _row_weights("linear_train_step", row_weights, dev, B)
        step, name, head = L.dbmm_linear_train_step_weighted, "linear_train_step_weighted", (row_weights.data_ptr(),)
    ws = _linear_workspace(dev, L.dbmm_workspace_bytes_linear_train_step(B, D, C))
    logits = _empty((B, C), device=dev, dtype=torch.float32)
    loss = _empty((B + 1,), device=dev, dtype=torch.float32)        # per-row losses, then their mean: one allocation
    rc = step(x.data_ptr(), labels.data_ptr(), w.data_ptr(), b.data_ptr(), m_w.data_ptr(), m_b.data_ptr(),
              float(lr), float(momentum), float(weight_decay), int(first_step), logits.data_ptr(),
              loss.data_ptr(), loss.data_ptr() + 4 * B, *head, B, D, C, ws.data_ptr(), ws.numel() * 4, stream())
    if rc:
        check(rc, name)
    return loss[B], logits, loss[:B]


def linear_ce_fwd(x, labels, w, b):
    """the linear probe's eval forward (dbmm_linear_ce_fwd): (mean CE 0-dim, logits [B, C], per-row CE [B])"""
    B, D, C = _linear_operands(x, labels, w, b)
    dev = x.device
    L = _lib.lib()
    ws = _linear_workspace(dev, L.dbmm_workspace_bytes_linear_ce_fwd(B))
    logits = _empty((B, C), device=dev, dtype=torch.float32)
    loss = _empty((B + 1,), device=dev, dtype=torch.float32)
    rc = L.dbmm_linear_ce_fwd(x.data_ptr(), w.data_ptr(), b.data_ptr(), labels.data_ptr(), logits.data_ptr(), loss.data_ptr(),
                              loss.data_ptr() + 4 * B, B, D, C, ws.data_ptr(), ws.numel() * 4, stream())
    if rc:
        check(rc, "linear_ce_fwd")
    return loss[B], logits, loss[:B]


def _linear_sweep_operands(table, labels, groups, w, b, extra=()):
    """the stacked operands of the replica-batched linear-probe calls: table [N, D], labels / groups int64 [N], w [R, C, D], b [R, C]
    (and momentum buffers of the same shapes), all contiguous on one device.  Returns (R, C, D)."""
    require_cuda(table, labels, groups, w, b, *extra)
    if table.dim() != 2 or w.dim() != 3 or b.dim() != 2:
        raise _lib.DbmmError(f"linear sweep: table [N, D], w [R, C, D], b [R, C] expected; got {tuple(table.shape)}, {tuple(w.shape)}, "
                             f"{tuple(b.shape)}")
    R, C, D = w.shape
    for t in (table, w, b) + tuple(extra):
        _f32c(t)
    if table.shape[1] != D or tuple(b.shape) != (R, C):
        raise _lib.DbmmError(f"linear sweep: table {tuple(table.shape)} and b {tuple(b.shape)} against w {tuple(w.shape)}")
    if not (1 <= R <= 16) or not (1 <= C <= 8) or D % 4 or not (4 <= D <= 1024):
        raise _lib.DbmmError(f"linear sweep kernels serve 1..16 replicas, C <= 8 classes, D % 4 == 0 and D <= 1024; got R={R} C={C} D={D}")
    for nm, t in (("labels", labels), ("groups", groups)):
        if t.dtype != torch.int64 or not t.is_contiguous():
            raise _lib.DbmmError(f"linear sweep: {nm} must be a contiguous int64 tensor")
        _sized(f"linear sweep {nm}", t, table.shape[0])
    if any(t.device != table.device for t in (labels, groups, w, b) + tuple(extra)):
        raise _lib.DbmmError("linear sweep: all operands must be on one device")
    return R, C, D


def linear_sweep_step(table, idx, labels, groups, w, b, m_w, m_b, lrs, momentum, weight_decay, first_step, counts, loss_sum, counted=True,
                      row_weights=None):
    """one training step of R linear probes in the launches of one (dbmm_linear_sweep_step): replica r trains on rows idx[r] of
    `table` ([N, D] fp32; labels / groups int64 [N]); w / m_w [R, C, D] and b / m_b [R, C] are updated in place; `lrs` R host floats;
    counts int64 [R, G, 2] and loss_sum float64 [R] are accumulated in place when `counted`.  Returns (mean CE [R], logits
    [R, B, C], per-row CE [R, B]).  `row_weights` float32 [N] / [1, N] (shared) or [R, N] over the TABLE's rows: the step under
    per-row loss weights (dbmm_linear_sweep_step_weighted)."""
    R, C, D = _linear_sweep_operands(table, labels, groups, w, b, (m_w, m_b))
    if m_w.shape != w.shape or m_b.shape != b.shape:
        raise _lib.DbmmError(f"linear sweep: momentum buffers {tuple(m_w.shape)}, {tuple(m_b.shape)} for w {tuple(w.shape)}, b {tuple(b.shape)}")
    require_cuda(idx)
    if idx.dtype != torch.int64 or not idx.is_contiguous() or idx.dim() != 2 or idx.shape[0] != R or idx.shape[1] < 1:
        raise _lib.DbmmError("linear sweep step: idx must be a contiguous int64 [R, B] tensor")
    if idx.device != table.device:
        raise _lib.DbmmError(f"linear sweep step: idx is on {idx.device}, the table on {table.device}")
    G = _sweep_metrics(counts, loss_sum, R)
    if len(lrs) != R:
        raise _lib.DbmmError(f"linear sweep step: {len(lrs)} learning rates for {R} replicas")
    B = idx.shape[1]
    dev = table.device
    L = _lib.lib()
    ws = _sweep_workspace(dev, L.dbmm_workspace_bytes_linear_sweep_step(R, B, D, C))
    logits = _empty((R, B, C), device=dev, dtype=torch.float32)
    loss = _empty((R * (B + 1),), device=dev, dtype=torch.float32)      # the R x B per-row losses, then the R means: one allocation
    LR = (ctypes.c_float * R)(*[float(v) for v in lrs])
    step, name, head = L.dbmm_linear_sweep_step, "linear_sweep_step", ()
    if row_weights is not None:
        Rw = _row_weights("linear sweep step", row_weights, dev, table.shape[0], R)
        step, name, head = L.dbmm_linear_sweep_step_weighted, "linear_sweep_step_weighted", (row_weights.data_ptr(), Rw)
    rc = step(table.data_ptr(), table.shape[0], idx.data_ptr(), idx.shape[0], B, labels.data_ptr(), groups.data_ptr(),
              w.data_ptr(), b.data_ptr(), m_w.data_ptr(), m_b.data_ptr(), LR, float(momentum), float(weight_decay),
              int(first_step), logits.data_ptr(), loss.data_ptr(), loss.data_ptr() + 4 * R * B, counts.data_ptr(),
              loss_sum.data_ptr(), G, int(counted), *head, R, B, D, C, ws.data_ptr(), ws.numel() * 4, stream())
    if rc:
        check(rc, name)
    return loss[R * B:], logits, loss[:R * B].view(R, B)


def linear_sweep_eval(table, idx, labels, groups, w, b, counts, loss_sum, row0=0, n=None):
    """the eval forward of R linear probes over the same rows (dbmm_linear_sweep_eval): rows idx (int64 [B]) of `table`, or idx
    None: rows row0 .. row0 + n - 1.  counts int64 [R, G, 2] and loss_sum float64 [R] are accumulated in place.  Returns (logits
    [R, B, C], per-row CE [R, B])."""
    R, C, D = _linear_sweep_operands(table, labels, groups, w, b)
    if idx is not None:
        require_cuda(idx)
        if idx.dtype != torch.int64 or not idx.is_contiguous() or idx.dim() != 1 or idx.shape[0] < 1:
            raise _lib.DbmmError("linear sweep eval: idx must be a contiguous int64 [B] tensor")
        if idx.device != table.device:
            raise _lib.DbmmError(f"linear sweep eval: idx is on {idx.device}, the table on {table.device}")
        B = idx.shape[0]
    else:
        B = table.shape[0] - row0 if n is None else n
        if row0 < 0 or B < 1 or row0 + B > table.shape[0]:
            raise _lib.DbmmError(f"linear sweep eval: rows row0={row0} .. row0 + n - 1 (n={B}) are not inside the table of {table.shape[0]} rows")
    G = _sweep_metrics(counts, loss_sum, R)
    dev = table.device
    L = _lib.lib()
    ws = _sweep_workspace(dev, L.dbmm_workspace_bytes_linear_sweep_eval(R, B))
    logits = _empty((R, B, C), device=dev, dtype=torch.float32)
    rows = _empty((R, B), device=dev, dtype=torch.float32)
    rc = L.dbmm_linear_sweep_eval(table.data_ptr(), table.shape[0], ptr(idx), row0, labels.data_ptr(), groups.data_ptr(), w.data_ptr(),
                                  b.data_ptr(), logits.data_ptr(), rows.data_ptr(), counts.data_ptr(), loss_sum.data_ptr(), G, R, B, D, C,
                                  ws.data_ptr(), ws.numel() * 4, stream())
    if rc:
        check(rc, "linear_sweep_eval")
    return logits, rows


PROX_MAX_R = 256                    # fits of one dbmm_linear_prox_fit launch (csrc/linear_prox.hip: one workgroup each)

# the state of R L1-probe fits between launches: iterate w [R, C, D] / b [R, C], extrapolated point v / c (float32), t float64 [R]
ProxState = namedtuple("ProxState", "w b v c t")


def linear_prox_state(R, C, D, device, w=None, b=None):
    """the start of R fits: t = 1 and V = W (zero weights unless `w` [R, C, D] / `b` [R, C] are given)"""
    w = torch.zeros((R, C, D), dtype=torch.float32, device=device) if w is None else w.to(device, torch.float32).contiguous().clone()
    b = torch.zeros((R, C), dtype=torch.float32, device=device) if b is None else b.to(device, torch.float32).contiguous().clone()
    if tuple(w.shape) != (R, C, D) or tuple(b.shape) != (R, C):
        raise _lib.DbmmError(f"linear prox state: w {tuple(w.shape)}, b {tuple(b.shape)} for R={R} C={C} D={D}")
    return ProxState(w, b, w.clone(), b.clone(), torch.ones((R,), dtype=torch.float64, device=device))


def linear_prox_fit(table, idx, labels, lam, step, state, iters, accelerate=True):
    """`iters` FISTA iterations of R L1-penalised logistic probes in ONE launch (dbmm_linear_prox_fit, one workgroup per fit): fit r
    minimises (1 / n) sum CE + lam[r] ||W||_1 over rows idx[r] (int64 [R, n], clamped into the table) of `table` ([N, D] fp32; labels
    int64 [N]) with step[r] = 1 / L; lam, step float32 [R] on the device.  `state` (a ProxState; linear_prox_state starts one) is
    advanced in place, so a fit may be split over any number of calls.  accelerate=False: plain ISTA (beta = 0).  Returns stats
    float32 [R, 4] of the call's last iteration: max |dW|, max |W|, nonzeros of W, CE mean at the extrapolated point."""
    require_cuda(table, idx, labels, lam, step, *state)
    w, b, v, c, t = state
    if table.dim() != 2 or w.dim() != 3 or b.dim() != 2:
        raise _lib.DbmmError(f"linear prox: table [N, D], w [R, C, D], b [R, C] expected; got {tuple(table.shape)}, {tuple(w.shape)}, "
                             f"{tuple(b.shape)}")
    R, C, D = w.shape
    for nm, x in (("table", table), ("w", w), ("b", b), ("v", v), ("c", c), ("lam", lam), ("step", step)):
        _f32c(x, "linear prox " + nm)
    if table.shape[1] != D or tuple(b.shape) != (R, C) or v.shape != w.shape or c.shape != b.shape:
        raise _lib.DbmmError(f"linear prox: table {tuple(table.shape)}, b {tuple(b.shape)}, v {tuple(v.shape)}, c {tuple(c.shape)} against "
                             f"w {tuple(w.shape)}")
    if not (1 <= R <= PROX_MAX_R) or not (1 <= C <= 8) or D % 4 or not (4 <= D <= 1024) or table.shape[0] < 1:
        raise _lib.DbmmError(f"linear prox serves 1..{PROX_MAX_R} fits, C <= 8 classes, D % 4 == 0 and D <= 1024; got R={R} C={C} D={D}")
    if labels.dtype != torch.int64 or not labels.is_contiguous():
        raise _lib.DbmmError("linear prox: labels must be a contiguous int64 tensor")
    _sized("linear prox labels", labels, table.shape[0])
    if idx.dtype != torch.int64 or not idx.is_contiguous() or idx.dim() != 2 or idx.shape[0] != R or idx.shape[1] < 1:
        raise _lib.DbmmError("linear prox: idx must be a contiguous int64 [R, n] tensor with n >= 1")
    _operand("linear prox t", t, torch.float64, (R,))
    _sized("linear prox lam", lam, R)
    _sized("linear prox step", step, R)
    if any(x.device != table.device for x in (idx, labels, lam, step, w, b, v, c, t)):
        raise _lib.DbmmError("linear prox: all operands must be on one device")
    iters = int(iters)
    if not (1 <= iters <= 1 << 20):
        raise _lib.DbmmError(f"linear prox: iters in 1..2^20 expected, got {iters}")
    stats = _empty((R, 4), device=table.device, dtype=torch.float32)
    rc = _lib.lib().dbmm_linear_prox_fit(table.data_ptr(), table.shape[0], idx.data_ptr(), labels.data_ptr(), lam.data_ptr(), step.data_ptr(),
                                         w.data_ptr(), b.data_ptr(), v.data_ptr(), c.data_ptr(), t.data_ptr(), stats.data_ptr(), R,
                                         idx.shape[1], D, C, iters, int(bool(accelerate)), stream())
    if rc:
        check(rc, "linear_prox_fit")
    return stats


def gather_rows(table, idx):
    """out[i] = table[idx[i]] for a device-resident [N, D] fp32 table and int64 indices."""
    require_cuda(table, idx)
    _f32c(table)
    idx = idx.contiguous()
    out = _empty((idx.numel(), table.shape[1]), device=table.device, dtype=torch.float32)
    check(_lib.lib().dbmm_gather_rows(ptr(table), ptr(idx), ptr(out), table.shape[0], idx.numel(), table.shape[1],
                                      stream()), "gather_rows")
    return out


# ---- the analysis kernels (pairdist, covariance, k-means, label sums, erasure): every operand is refused here, before any allocation or launch
def _rows_operand(what, x, mult=64, max_n=1 << 23):
    """(N, D) of the rows x: an fp32 contiguous 16-byte aligned [N, D] device tensor with N in 1..max_n (None: any N >= 1), else
    DbmmError; D a positive multiple of `mult` up to 4096 -- the widths the kernels serve --, else DbmmUnsupported"""
    require_cuda(x)
    _f32c(x, f"{what}: x")
    if x.dim() != 2 or x.shape[0] < 1 or (max_n is not None and x.shape[0] > max_n):
        raise _lib.DbmmError(f"{what}: x must be [N, D] with N {'>= 1' if max_n is None else f'in 1..{max_n}'}, got {tuple(x.shape)}")
    N, D = x.shape
    if D % mult or D > 4096 or D == 0:
        raise DbmmUnsupported(f"{what}: D = {D}; the kernel serves D % {mult} == 0, D <= 4096")
    if x.data_ptr() % 16:
        raise _lib.DbmmError(f"{what}: x is not 16-byte aligned")
    return N, D


def _ids_operand(what, name, ids, x):
    """ids (`name`: groups, labels): a contiguous int64 [N] tensor on x's device, one id per row of x"""
    if not torch.is_tensor(ids):
        raise _lib.DbmmError(f"{what}: {name} must be a contiguous int64 [N] device tensor, got {type(ids).__name__}")
    require_cuda(ids)
    if ids.dtype != torch.int64 or not ids.is_contiguous() or ids.dim() != 1:
        raise _lib.DbmmError(f"{what}: {name} must be a contiguous int64 [N] tensor, got {ids.dtype} {tuple(ids.shape)}")
    if ids.numel() != x.shape[0]:
        raise _lib.DbmmError(f"{what}: {ids.numel()} {name} for {x.shape[0]} rows")
    if ids.device != x.device:
        raise _lib.DbmmError(f"{what}: {name} is on {ids.device}, x on {x.device}")


def _f32_operand(what, name, t, x, n=None):
    """an fp32 contiguous 16-byte aligned operand on x's device; n: the elements the kernels will index (a [D] vector as `center`)"""
    if not torch.is_tensor(t):
        raise _lib.DbmmError(f"{what}: {name} must be a device tensor, got {type(t).__name__}")
    require_cuda(t)
    _f32c(t, f"{what}: {name}")
    if n is not None and t.numel() != n:
        raise _lib.DbmmError(f"{what}: {name} has {t.numel()} elements where the kernels will index {n}")
    if t.device != x.device:
        raise _lib.DbmmError(f"{what}: {name} is on {t.device}, x on {x.device}")
    if t.data_ptr() % 16:
        raise _lib.DbmmError(f"{what}: {name} is not 16-byte aligned")


def _served(rc, what, request):
    """a C entry's return code: DBMM_E_UNSUPPORTED is DbmmUnsupported (no kernel for this valid request), any other failure DbmmError"""
    if rc == _lib.E_UNSUPPORTED:
        raise DbmmUnsupported(f"{what}: no kernel for {request}")
    check(rc, what)


PAIRDIST_RBF_MAX_L = 4               # bandwidths of one RBF bucket pass (csrc/pairdist.hip: RBF_MAX_L)


def _rbf_gammas(what, gammas):
    """1..PAIRDIST_RBF_MAX_L finite numbers > 0 as a ctypes double array, else DbmmError naming the value"""
    try:
        vals = [float(g) for g in gammas]
    except (TypeError, ValueError):
        raise _lib.DbmmError(f"{what}: gammas must be a sequence of 1..{PAIRDIST_RBF_MAX_L} positive numbers, got {gammas!r}") from None
    if not 1 <= len(vals) <= PAIRDIST_RBF_MAX_L:
        raise _lib.DbmmError(f"{what}: {len(vals)} gammas; the kernel sums 1..{PAIRDIST_RBF_MAX_L} bandwidths in one pass")
    for v in vals:
        if not (v > 0 and math.isfinite(v)):
            raise _lib.DbmmError(f"{what}: gamma = {v!r}; every bandwidth must be finite and > 0")
    return (ctypes.c_double * len(vals))(*vals)


_NO_GAMMAS = object()                # a distance entry: it takes no bandwidths (None is a refused value of `gammas`)


def _pairdist(what, sizer, x, center, cap, groups=None, n_groups=None, v=None, per_row=False, gammas=_NO_GAMMAS):
    """The one frame of the five pairwise-kernel wrappers below (csrc/pairdist.hip); each says what is its own.  In this order: the
    gammas, host values, refused before any device is touched; x; the ids `groups` (n_groups labels, at most `cap`) or the weights
    `v` [N, C <= cap]; center; the workspace, sized by the library's `sizer`, then the result -- the call's two allocations --;
    the C entry dbmm_<what>; _served.  The result is float64: [G, G] of a bucket pass, [N, G] with per_row, under a leading [L]
    where the entry takes a ladder of bandwidths (with `v` it takes one, by value)."""
    gam = None if gammas is _NO_GAMMAS else _rbf_gammas(what, gammas)
    N, D = _rows_operand(what, x)
    if v is None:
        _ids_operand(what, "groups", groups, x)
        _f32_operand(what, "center", center, x, D)
        if not 1 <= n_groups <= cap:
            raise _lib.DbmmError(f"{what}: n_groups = {n_groups} outside 1..{cap}")
        second, n = groups, n_groups
        lead, mid = ((), ()) if gam is None else ((len(gam),), (ctypes.addressof(gam), len(gam)))
    else:
        _f32_operand(what, "v", v, x)
        if v.dim() != 2 or v.shape[0] != N or not 1 <= v.shape[1] <= cap:
            raise _lib.DbmmError(f"{what}: v must be [{N}, C] with C in 1..{cap}, got {tuple(v.shape)}")
        _f32_operand(what, "center", center, x, D)
        second, n, lead, mid = v, v.shape[1], (), (gam[0],)
    L = _lib.lib()
    nbytes = getattr(L, sizer)(N, D, *((n,) if per_row else ()), *lead)
    ws = _empty((nbytes + 3) // 4, device=x.device, dtype=torch.float32)           # planes and partials: sized by the call, not cached
    out = _empty(lead + ((N, n) if per_row else (n, n)), device=x.device, dtype=torch.float64)
    rc = getattr(L, "dbmm_" + what)(x.data_ptr(), second.data_ptr(), center.data_ptr(), *mid, out.data_ptr(), N, D, n, ws.data_ptr(),
                                    ws.numel() * 4, stream())
    _served(rc, what, f"N = {N}, D = {D}")
    return out


def pairdist_group_sums(x, groups, n_groups, center):
    """S float64 [G, G], symmetric: S[a, b] = sum over unordered pairs i < j with {groups[i], groups[j]} = {a, b} of
    ||x[i] - x[j]||_2, on the fused Gram-and-distance kernel (dbmm_pairdist_group_sums): no N x N matrix, float64 sums in a fixed
    order.  x fp32 [N, D] (D % 64 == 0, D <= 4096), groups int64 [N] in [0, n_groups) (n_groups <= 8), center fp32 [D]: a vector
    near the rows' mean (the split's mean vector), subtracted before the products are formed.  The whole split's sum is
    S.triu().sum(); group a's own is S[a, a]."""
    return _pairdist("pairdist_group_sums", "dbmm_workspace_bytes_pairdist", x, center, groups=groups, n_groups=n_groups, cap=8)


def pairdist_rbf_group_sums(x, groups, n_groups, center, gammas):
    """K float64 [L, G, G], symmetric in its last two axes: K[l, a, b] = sum over unordered pairs i < j with {groups[i], groups[j]} =
    {a, b} of exp(-gammas[l] ||x[i] - x[j]||^2), on the fused Gram kernel (dbmm_pairdist_rbf_group_sums): pairdist_group_sums'
    pass with the exponential for the square root, L bandwidths from one Gram product, no N x N matrix, float64 sums in a fixed
    order -- the same bits on every call, and a bandwidth's sums do not depend on the others in the call.  Operands as
    pairdist_group_sums; gammas: 1..4 finite numbers > 0 (host values).  The diagonal is left out by index: a V-statistic adds the
    group's row count to K[l, a, a]."""
    return _pairdist("pairdist_rbf_group_sums", "dbmm_workspace_bytes_pairdist_rbf", x, center, groups=groups, n_groups=n_groups, cap=8, gammas=gammas)


PAIRDIST_ROWS_MAX_G = 16            # labels of the per-row distance sums (csrc/pairdist.hip); the value of KMEANS_MAX_K


def pairdist_row_group_sums(x, groups, n_groups, center):
    """R float64 [N, G]: R[i, g] = sum over j != i with groups[j] == g of ||x[i] - x[j]||_2, on the fused Gram-and-distance kernel
    (dbmm_pairdist_row_group_sums): no N x N matrix, float64 sums in a fixed order, the same bits on every call.  x fp32 [N, D]
    (D % 64 == 0, D <= 4096), groups int64 [N] (n_groups <= 16; a row with a label outside [0, n_groups) is in nobody's sums and
    still gets its own), center fp32 [D]: a vector near the rows' mean (the split's mean vector), subtracted before the products
    are formed.  The diagonal is left out by index: R[i, groups[i]] of a group's only row and the column of an empty group are
    exactly 0.  Rows sorted by group take the kernel's fast path; any order gives the same sums to 1e-6."""
    return _pairdist("pairdist_row_group_sums", "dbmm_workspace_bytes_pairdist_rows", x, center, groups=groups, n_groups=n_groups, cap=PAIRDIST_ROWS_MAX_G,
                     per_row=True)


def pairdist_rbf_row_group_sums(x, groups, n_groups, center, gammas):
    """R float64 [L, N, G]: R[l, i, g] = sum over j != i with groups[j] == g of exp(-gammas[l] ||x[i] - x[j]||^2), on the fused Gram
    kernel (dbmm_pairdist_rbf_row_group_sums): pairdist_row_group_sums' pass with pairdist_rbf_group_sums' element map, L bandwidths
    from one Gram product, no N x N matrix, float64 sums in a fixed order -- the same bits on every call, and a bandwidth's sums do
    not depend on the others in the call.  Operands as pairdist_row_group_sums (n_groups <= 16; a row with a label outside
    [0, n_groups) is in nobody's sums and still gets its own: a query row); gammas: 1..4 finite numbers > 0 (host values).  The
    diagonal is left out by index: R[l, i, groups[i]] of a label's only row and the column of an empty label are exactly 0."""
    return _pairdist("pairdist_rbf_row_group_sums", "dbmm_workspace_bytes_pairdist_rbf_rows", x, center, groups=groups, n_groups=n_groups,
                     cap=PAIRDIST_ROWS_MAX_G, per_row=True, gammas=gammas)


PAIRDIST_MATVEC_MAX_C = 16          # weight columns of one kernel-matrix product (csrc/pairdist.hip: ROWS_MAX_G)


def pairdist_rbf_matvec(x, v, center, gamma):
    """R float64 [N, C]: R[i, c] = sum over j != i of exp(-gamma ||x[i] - x[j]||^2) v[j, c], the product of the RBF kernel matrix of
    the rows (zero diagonal) with C dense columns, on the fused Gram kernel (dbmm_pairdist_rbf_matvec): pairdist_rbf_row_group_sums'
    pass with the weights v in place of the labels -- no N x N matrix, the kernel values formed once per tile and a further column
    one multiply-add per pair, float64 sums in a fixed order, the same bits on every call, and a column's result does not depend on
    the other columns of the call.  x, center as pairdist_row_group_sums; v fp32 [N, C] contiguous, 1 <= C <= 16, signed; gamma:
    one finite number > 0 (a host value).  A 256-row block of v that is zero in a column costs that column nothing: one-hot
    columns and zero weights on appended query rows are cheap.  An entry is good to 1e-4 sum_j k_ij |v_jc|; the kernel matrix with
    its unit diagonal is R + v."""
    return _pairdist("pairdist_rbf_matvec", "dbmm_workspace_bytes_pairdist_rbf_matvec", x, center, v=v, cap=PAIRDIST_MATVEC_MAX_C, per_row=True, gammas=[gamma])


def covariance(x, center):
    """S float64 [D, D]: S[a, b] = sum_i (x[i, a] - center[a]) (x[i, b] - center[b]), about the given center exactly, on the fused
    scatter kernel (dbmm_covariance): no centred copy of x, exact fp32 products, no fp32 chain longer than 1024 rows, float64 sums
    in a fixed order; symmetric to the bit and the same bits on every call.  x fp32 [N, D] (D % 64 == 0, D <= 4096), center fp32
    [D]: a vector near the rows' mean."""
    N, D = _rows_operand("covariance", x)
    _f32_operand("covariance", "center", center, x, D)
    L = _lib.lib()
    nbytes = L.dbmm_workspace_bytes_covariance(N, D)
    ws = _empty((nbytes + 7) // 8, device=x.device, dtype=torch.float64)            # the partial tiles: sized by (N, D), not cached
    out = _empty((D, D), device=x.device, dtype=torch.float64)
    rc = L.dbmm_covariance(x.data_ptr(), center.data_ptr(), out.data_ptr(), N, D, ws.data_ptr(), ws.numel() * 8, stream())
    _served(rc, "covariance", f"N = {N}, D = {D}")
    return out


def project_rows(x, center, basis):
    """y fp32 [N, K] = (x - center) @ basis.T in one read of x (dbmm_project_rows): basis fp32 [K, D], K in 1..8.  A row's
    coordinates do not depend on the other rows: projecting a slice gives the bits of the slice of the projection."""
    N, D = _rows_operand("project_rows", x)
    _f32_operand("project_rows", "center", center, x, D)
    _f32_operand("project_rows", "basis", basis, x)
    if basis.dim() != 2 or basis.shape[1] != D or not 1 <= basis.shape[0] <= 8:
        raise _lib.DbmmError(f"project_rows: basis must be [K, {D}] with K in 1..8, got {tuple(basis.shape)}")
    K = basis.shape[0]
    out = _empty((N, K), device=x.device, dtype=torch.float32)
    rc = _lib.lib().dbmm_project_rows(x.data_ptr(), center.data_ptr(), basis.data_ptr(), out.data_ptr(), N, D, K, stream())
    _served(rc, "project_rows", f"N = {N}, D = {D}")
    return out


SYM_EIG_BLOCK = 16                  # vectors of the subspace iteration's block (csrc/sym_eig.hip)
SYM_EIG_STATES = ("running", "converged", "breakdown")
_SYM_EIG_STATUS = 64                # doubles of the status block at the head of the workspace (include/dbmm.h)


def sym_eig_topk(C, k, tol=1e-10, max_iter=256, check_every=8):
    """The top k eigenpairs of a symmetric positive semi-definite float64 matrix C [D, D] (D % 64 == 0, D <= 4096; symmetric to
    the bit, as `covariance` returns it) on the device: blocked subspace iteration on 16 vectors with a Rayleigh-Ritz step per
    iteration (dbmm_sym_eig_begin / dbmm_sym_eig_iterate).  Returns (values float64 [k] descending, vectors float64 [k, D] of unit
    norm, info): device tensors, views of the call's workspace, and info = {'iterations', 'converged', 'state' ('running' |
    'converged' | 'breakdown'), 'residual': max_j ||C v_j - theta_j v_j|| / theta_1 as the device reports it}.

    The start block is np.random.RandomState(0x5EED).standard_normal((D, 16)) (a private stream), so two calls give the same bits.
    The loop enqueues min(check_every, remaining) iterations, reads the status block (one small copy to the host) and stops on
    'converged', 'breakdown' or max_iter; iterations enqueued after convergence are no-ops on the device, so the result does not
    depend on check_every.  Non-convergence is reported, never raised: the iteration converges by lambda_17 / lambda_k per step and
    does not get there when the k-th eigenvalue sits in a flat bulk."""
    require_cuda(C)
    if C.dtype != torch.float64 or not C.is_contiguous() or C.dim() != 2 or C.shape[0] != C.shape[1]:
        raise _lib.DbmmError(f"sym_eig_topk: C must be a contiguous float64 [D, D] tensor, got {C.dtype} {tuple(C.shape)}")
    D = C.shape[0]
    k, max_iter, check_every = int(k), int(max_iter), int(check_every)
    if not 1 <= k <= 8:
        raise _lib.DbmmError(f"sym_eig_topk: k = {k} outside 1..8")
    if max_iter < 1 or check_every < 1:
        raise _lib.DbmmError(f"sym_eig_topk: max_iter = {max_iter}, check_every = {check_every}; both at least 1")
    if not (tol > 0 and math.isfinite(tol)):
        raise _lib.DbmmError(f"sym_eig_topk: tol = {tol} is not a positive finite number")
    if D % 64 or D > 4096 or D == 0:
        raise DbmmUnsupported(f"sym_eig_topk: D = {D}; the kernels serve D % 64 == 0, D <= 4096")
    L = _lib.lib()
    nbytes = L.dbmm_workspace_bytes_sym_eig(D)
    ws = _empty(nbytes // 8, device=C.device, dtype=torch.float64)
    q0 = _empty((D, SYM_EIG_BLOCK), device=C.device, dtype=torch.float64)
    q0.copy_(torch.from_numpy(np.random.RandomState(0x5EED).standard_normal((D, SYM_EIG_BLOCK))))
    check(L.dbmm_sym_eig_begin(q0.data_ptr(), D, k, float(tol), ws.data_ptr(), nbytes, stream()), "sym_eig_begin")
    done = 0
    while True:
        n = min(check_every, max_iter - done)
        check(L.dbmm_sym_eig_iterate(C.data_ptr(), D, n, ws.data_ptr(), nbytes, stream()), "sym_eig_iterate")
        done += n
        status = ws[:_SYM_EIG_STATUS].cpu().numpy()
        state = int(status[1])
        if state != 0 or done >= max_iter:
            break
    theta1 = status[2]
    info = {"iterations": int(status[0]), "converged": state == 1, "state": SYM_EIG_STATES[state],
            "residual": float(status[18:18 + k].max() / theta1) if theta1 > 0 else float("inf")}
    vectors = ws[_SYM_EIG_STATUS:_SYM_EIG_STATUS + SYM_EIG_BLOCK * D].view(SYM_EIG_BLOCK, D)[:k]
    return ws[2:2 + k], vectors, info


KMEANS_MAX_K = 16                   # centres of the k-means kernels (csrc/kmeans.hip); more wants an MFMA tile kernel
_KMEANS_STATUS = 256                # bytes of the status block at the head of the workspace (include/dbmm.h)


def _kmeans_operands(what, x, centers):
    N, D = _rows_operand(what, x, mult=4, max_n=None)
    _f32_operand(what, "centers", centers, x)
    if centers.dim() != 2 or centers.shape[1] != D or centers.shape[0] < 1:
        raise _lib.DbmmError(f"{what}: centers must be [K, {D}] with K >= 1, got {tuple(centers.shape)}")
    K = centers.shape[0]
    if K > KMEANS_MAX_K:
        raise DbmmUnsupported(f"{what}: K = {K}; the kernels serve K <= {KMEANS_MAX_K}")
    return N, D, K


def kmeans_assign(x, centers):
    """(labels int32 [N], dmin fp32 [N]): the nearest of the centres fp32 [K, D] (K <= 16; the lowest index on an exact tie) and the
    squared distance to it, for every row of x fp32 [N, D] (D % 4 == 0, D <= 4096), in one read of x (dbmm_kmeans_assign).  The
    distances are sums of squared differences in fp32, and a row's result does not depend on the other rows: assigning a slice gives
    the bits of the slice of the assignment."""
    N, D, K = _kmeans_operands("kmeans_assign", x, centers)
    labels = _empty((N,), device=x.device, dtype=torch.int32)
    dmin = _empty((N,), device=x.device, dtype=torch.float32)
    rc = _lib.lib().dbmm_kmeans_assign(x.data_ptr(), centers.data_ptr(), labels.data_ptr(), dmin.data_ptr(), N, D, K, stream())
    _served(rc, "kmeans_assign", f"N = {N}, D = {D}, K = {K}")
    return labels, dmin


def kmeans_fit(x, centers0, max_iter=100, check_every=8):
    """Lloyd's k-means of the rows x fp32 [N, D] from the start centres centers0 fp32 [K, D] (K <= 16, N >= K, D % 4 == 0,
    D <= 4096) on the device (dbmm_kmeans_begin / dbmm_kmeans_iterate): per iteration one assignment, the per-cluster sums in a fixed
    order and the float64 merge; a cluster that loses all its rows keeps its centre.  Returns (centers fp32 [K, D], labels int32
    [N], info): device tensors, views of the call's workspace, and info = {'iterations', 'converged', 'inertia': the float64 sum of the
    squared distances of the last assignment, 'counts': numpy int64 [K] of that assignment}.  Converged means that an assignment
    changed no label; labels, inertia and counts then belong to the returned centres.

    The loop enqueues min(check_every, remaining) iterations, reads the status block (one small copy to the host) and stops on
    'converged' or max_iter; iterations enqueued after convergence are no-ops on the device, so the result does not depend on
    check_every, and two calls give the same bits.  Non-convergence is reported, never raised."""
    N, D, K = _kmeans_operands("kmeans_fit", x, centers0)
    max_iter, check_every = int(max_iter), int(check_every)
    if max_iter < 1 or check_every < 1:
        raise _lib.DbmmError(f"kmeans_fit: max_iter = {max_iter}, check_every = {check_every}; both at least 1")
    if N < K:
        raise _lib.DbmmError(f"kmeans_fit: {N} rows for {K} centres")
    L = _lib.lib()
    nbytes = L.dbmm_workspace_bytes_kmeans(N, D, K)
    if nbytes == 0:
        raise DbmmUnsupported(f"kmeans_fit: no kernel for N = {N}, D = {D}, K = {K}")
    ws = _empty((nbytes // 4,), device=x.device, dtype=torch.float32).view(torch.uint8)       # (the layout is in bytes, a multiple of 16)
    check(L.dbmm_kmeans_begin(centers0.data_ptr(), N, D, K, ws.data_ptr(), nbytes, stream()), "kmeans_begin")
    done = 0
    while True:
        n = min(check_every, max_iter - done)
        check(L.dbmm_kmeans_iterate(x.data_ptr(), N, D, K, n, ws.data_ptr(), nbytes, stream()), "kmeans_iterate")
        done += n
        status = ws[:_KMEANS_STATUS].cpu().numpy()
        words = status.view(np.int64)
        if words[1] != 0 or done >= max_iter:
            break
    info = {"iterations": int(words[0]), "converged": bool(words[1] == 1), "inertia": float(status.view(np.float64)[3]),
            "counts": words[4:4 + K].copy()}
    c0 = _KMEANS_STATUS
    l0 = c0 + K * D * 4
    centers = ws[c0:c0 + K * D * 4].view(torch.float32).view(K, D)
    labels = ws[l0:l0 + N * 4].view(torch.int32)
    return centers, labels, info


LABEL_SUMS_MAX_G = 16               # labels of the per-label column sums (csrc/erase.hip); the value of KMEANS_MAX_K
ERASE_MAX_R = 15                    # rank of the update of erase_rows: at most 16 labels, whose centred means have rank <= 15


def label_column_sums(x, labels, n_labels):
    """(sums float64 [G, D], counts int64 [G]): the RAW per-label column sums of the rows x fp32 [N, D] (D % 64 == 0, D <= 4096,
    N <= 2^23) and the rows per label, from one read of x (dbmm_label_colsums).  labels int64 [N], compared as 64-bit: a value
    outside [0, n_labels) is in no sum and no count.  n_labels in 1..16.  float64 from the first add, row order inside a range,
    the ranges merged in a fixed order: the same bits on every call."""
    N, D = _rows_operand("label_column_sums", x)
    _ids_operand("label_column_sums", "labels", labels, x)
    G = int(n_labels)
    if not 1 <= G <= LABEL_SUMS_MAX_G:
        raise _lib.DbmmError(f"label_column_sums: n_labels = {G} outside 1..{LABEL_SUMS_MAX_G}")
    L = _lib.lib()
    nbytes = L.dbmm_workspace_bytes_label_colsums(N, D, G)
    if nbytes == 0:
        raise DbmmUnsupported(f"label_column_sums: no kernel for N = {N}, D = {D}, G = {G}")
    ws = _empty((nbytes // 8,), device=x.device, dtype=torch.float64)                # the partials: sized by (N, D, G), not cached
    sums = _empty((G, D), device=x.device, dtype=torch.float64)
    counts = _empty((G,), device=x.device, dtype=torch.int64)
    rc = L.dbmm_label_colsums(x.data_ptr(), labels.data_ptr(), sums.data_ptr(), counts.data_ptr(), N, D, G, ws.data_ptr(), nbytes, stream())
    _served(rc, "label_column_sums", f"N = {N}, D = {D}")
    return sums, counts


def erase_rows(x, center, A, B, out=None):
    """y fp32 [N, D] = x - ((x - center) @ A.T) @ B in one read and one write of the rows (dbmm_erase_rows): A, B fp32 [R, D] with R
    in 1..15, center fp32 [D], x fp32 [N, D] (D % 64 == 0, D <= 4096, N <= 2^23).  `out`: None (a new tensor), x itself (in place:
    a row is read completely before it is written) or a tensor of x's shape that does not overlap x.  Nothing N x D is allocated
    beyond the result.  A row's result depends on that row only: erasing a slice gives the bits of the slice, and in place gives
    the bits of out of place."""
    N, D = _rows_operand("erase_rows", x)
    for name, t in (("center", center), ("A", A), ("B", B)):
        _f32_operand("erase_rows", name, t, x)
    if center.dim() != 1 or center.shape[0] != D:
        raise _lib.DbmmError(f"erase_rows: center must be [{D}], got {tuple(center.shape)}")
    if A.dim() != 2 or B.dim() != 2 or A.shape[1] != D or tuple(B.shape) != tuple(A.shape) or not 1 <= A.shape[0] <= ERASE_MAX_R:
        raise _lib.DbmmError(f"erase_rows: A and B must both be [R, {D}] with R in 1..{ERASE_MAX_R}, got {tuple(A.shape)} and {tuple(B.shape)}")
    R = A.shape[0]
    if out is None:
        out = _empty((N, D), device=x.device, dtype=torch.float32)
    else:
        _f32_operand("erase_rows", "out", out, x)
        if tuple(out.shape) != (N, D):
            raise _lib.DbmmError(f"erase_rows: out must be a 16-byte aligned [{N}, {D}] tensor on {x.device}, got {tuple(out.shape)} on {out.device}")
        lo, hi = out.data_ptr(), out.data_ptr() + N * D * 4
        if out.data_ptr() != x.data_ptr() and lo < x.data_ptr() + N * D * 4 and x.data_ptr() < hi:
            raise _lib.DbmmError("erase_rows: out overlaps x without being x; rows would be read after they were written")
    rc = _lib.lib().dbmm_erase_rows(x.data_ptr(), center.data_ptr(), A.data_ptr(), B.data_ptr(), out.data_ptr(), N, D, R, stream())
    _served(rc, "erase_rows", f"N = {N}, D = {D}")
    return out


# ---- fp16 mode of the transformer towers (csrc/f16_ops.hip) -------------------------------------------------------

def _f16c(t):
    if t.dtype != torch.float16 or not t.is_contiguous():
        raise _lib.DbmmError(f"expected a contiguous float16 tensor, got {t.dtype} contiguous={t.is_contiguous()}")
    return t


def _gemm_f16_tag(M, N):
    """instantiation dbmm_gemm_f16 picks for a shape the deep-pipelined kernel does not take (its own rule), as rocprofv3 prints it"""
    wide = get_option("f16_bn256") and N >= 768 and N % 256 == 0 and M >= 32768
    return "gemm_f16_kernel<32, 256, 2>" if wide else "gemm_f16_kernel<64, 128, 2>"


def gemm_f16(a, w, bias=None, residual=None, act=ACT_NONE, M=None, lda=None):
    """c f16 = act(a @ w^T + bias) + residual; a f16 [M][K] (row pitch lda), w f16 [N][K], bias f32, residual f16."""
    require_cuda(a, w)
    _f16c(w)
    if a.dtype != torch.float16:
        raise _lib.DbmmError("gemm_f16 needs float16 activations")
    N, K = w.shape
    _f16c(a)
    if lda is None:
        lda = a.shape[-1]
    if M is None:
        M = a.numel() // a.shape[-1]
    if a.numel() < (M - 1) * lda + K or lda < K:
        raise RuntimeError(f"gemm_f16: activations {tuple(a.shape)} (row pitch {lda}) for M = {M}, K = {K}")
    _optional("gemm_f16 bias", bias, torch.float32, N); _optional("gemm_f16 residual", residual, torch.float16, M * N)
    c = _empty((M, N), device=a.device, dtype=torch.float16)
    deep = N % 256 == 0 and K % 128 == 0 and M >= 16384 and get_option("f16_8ph")   # dbmm_gemm_f16's own rule
    with _TimedTag(f"gemm_f16_8ph_kernel<{act}, {int(residual is not None)}>" if deep else _gemm_f16_tag(M, N), 2.0 * M * N * K,
                   2 * (M * K + N * K + M * N * (2 if residual is not None else 1))):
        ws = igemm_workspace(a.device)
        check(_lib.lib().dbmm_gemm_f16_ws(ptr(a), lda, ptr(w), K, ptr(bias), ptr(residual), N if residual is not None else 0, ptr(c), N,
                                          M, N, K, act, ptr(ws), ws.numel() * 4, stream()), "gemm_f16")
    return c


def mha_core_f16(qkv, B, L, E, heads, causal):
    require_cuda(qkv)
    _f16c(qkv)
    if qkv.numel() != B * L * 3 * E or E != heads * 64:
        raise RuntimeError(f"mha_core_f16: qkv {tuple(qkv.shape)} for B = {B}, L = {L}, E = {E}, {heads} heads of 64")
    out = _empty((B * L, E), device=qkv.device, dtype=torch.float16)
    with _TimedTag("mha_f16_kernel", 4.0 * B * heads * L * L * 64, 2 * (B * L * 4 * E)):
        check(_lib.lib().dbmm_mha_core_f16(ptr(qkv), ptr(out), B, L, E, heads, int(causal), stream()), "mha_core_f16")
    return out


def layernorm_f16(x, gamma, beta, rows=None, ldx=None, eps=1e-5):
    E = gamma.numel()
    if rows is None:
        rows = x.numel() // E
    if ldx is None:
        ldx = E
    _operand("layernorm_f16 gamma", gamma, torch.float32, E); _operand("layernorm_f16 beta", beta, torch.float32, E)
    if ldx < E:
        raise RuntimeError(f"layernorm_f16: input {tuple(x.shape)} for {rows} rows of {E} at pitch {ldx}")
    _spans("layernorm_f16 input", x, torch.float16, (rows - 1) * ldx + E)
    y = _empty((rows, E), device=x.device, dtype=torch.float16)
    check(_lib.lib().dbmm_layernorm_f16(ptr(x), ldx, ptr(gamma), ptr(beta), ptr(y), E, rows, E, eps, stream()), "layernorm_f16")
    return y


def im2col_patch_f16(x_nchw, P, Kp):
    require_cuda(x_nchw)
    if x_nchw.dtype not in (torch.float16, torch.float32) or not x_nchw.is_contiguous():
        raise _lib.DbmmError(f"im2col_patch_f16 needs a contiguous float16 / float32 image batch, got {x_nchw.dtype} {tuple(x_nchw.shape)} "
                             f"contiguous={x_nchw.is_contiguous()}")
    _patch_image_check("im2col_patch_f16", x_nchw, P, Kp)
    B, C, R, _ = x_nchw.shape
    g = R // P
    out = _empty((B * g * g, Kp), device=x_nchw.device, dtype=torch.float16)
    check(_lib.lib().dbmm_im2col_patch_f16(ptr(x_nchw), int(x_nchw.dtype == torch.float16), ptr(out), B, R, P, Kp, stream()),
          "im2col_patch_f16")
    return out


def vit_tokens_f16(patches, cls, pos, B):
    _vit_tokens_check(patches, cls, pos, B, torch.float16)
    L, W = pos.shape
    out = _empty((B, L, W), device=patches.device, dtype=torch.float16)
    check(_lib.lib().dbmm_vit_tokens_f16(ptr(patches), ptr(cls), ptr(pos), ptr(out), B, L, W, stream()), "vit_tokens_f16")
    return out


def embed_gather_f16(tokens, table, pos):
    tokens = _embed_gather_check("embed_gather_f16", tokens, table, pos)
    n, L = tokens.shape
    W = table.shape[1]
    if tuple(pos.shape) != (L, W):
        raise RuntimeError(f"embed_gather_f16: {L} tokens per prompt against a positional embedding of shape {tuple(pos.shape)}")
    out = _empty((n, L, W), device=table.device, dtype=torch.float16)
    check(_lib.lib().dbmm_embed_gather_f16(ptr(tokens), ptr(table), ptr(pos), ptr(out), n, L, W, table.shape[0], stream()),
          "embed_gather_f16")
    return out, tokens


def gather_eot_f16(tokens_i32, x):
    _gather_eot_check("gather_eot_f16", tokens_i32, x, torch.float16)
    n, L, W = x.shape
    out = _empty((n, W), device=x.device, dtype=torch.float16)
    check(_lib.lib().dbmm_gather_eot_f16(ptr(tokens_i32), ptr(x), ptr(out), n, L, W, stream()), "gather_eot_f16")
    return out


# ---- fp16 mode of the ModifiedResNet towers (csrc/conv_f16.hip, csrc/f16_ops.hip) ------------------------------------------

def conv1x1_f16(x, w, scale, bias, residual=None, act=ACT_RELU):
    """y f16 NHWC = act(conv1x1(x) * scale + bias + residual); x f16 [..., Cin], w f16 [Cout][Cin]; None when the library has no
    kernel for the shape (Cin % 64, Cout % 8)."""
    require_cuda(x, w)
    _f16c(x); _f16c(w)
    Cout, Cin = w.shape
    if x.shape[-1] != Cin:
        raise RuntimeError(f"conv1x1_f16: {x.shape[-1]} input channels against a weight {tuple(w.shape)}")
    M = x.numel() // Cin
    _operand("conv1x1_f16 scale", scale, torch.float32, Cout); _operand("conv1x1_f16 bias", bias, torch.float32, Cout)
    _optional("conv1x1_f16 residual", residual, torch.float16, M * Cout)
    y = _empty(tuple(x.shape[:-1]) + (Cout,), device=x.device, dtype=torch.float16)
    deep = Cout % 256 == 0 and Cin % 128 == 0 and M >= 16384                            # what dbmm_gemm_f16 gives the eight-phase kernel
    mode = get_option("conv1x1_stream")
    # dbmm_conv1x1_bn_act_f16's own routing rule: the streaming kernel where the GEMM is not deep-pipelined, and for conv3 + residual with K <= 256
    stream_k = ((mode == 2 or (mode == 1 and not (deep and not (residual is not None and Cin <= 256))) or (mode == 3 and not deep))
                and act in (ACT_NONE, ACT_RELU) and Cin % 32 == 0)           # (mode 3: round 3's rule, without the conv3 + residual exception)
    res = int(residual is not None)
    tag = (f"conv1x1_f16_kernel<{'4, 1, 2' if Cout <= 64 else '2, 2, 4'}, {res}>" if stream_k
           else (f"gemm_f16_8ph_kernel<{act}, {res}>" if deep and get_option("f16_8ph") else _gemm_f16_tag(M, Cout)))
    if residual is not None and act == ACT_RELU and Cin == 256 and Cout >= 1024 and Cout % 64 == 0 and M >= 131072 and get_option("conv1x1_res_stream"):
        tag = "conv1x1_res_stream_f16_kernel<256, 0>"            # layer 3's conv3 + residual: the row-owning streaming kernel
    t = _TimedTag(tag, 2.0 * M * Cout * Cin,
                  2 * (M * Cin + Cout * Cin + M * Cout * (2 if residual is not None else 1)))
    t.__enter__()
    ws = igemm_workspace(x.device)
    rc = _lib.lib().dbmm_conv1x1_bn_act_f16_ws(ptr(x), ptr(w), ptr(scale), ptr(bias), ptr(residual), ptr(y), M, Cin, Cout, act, ptr(ws),
                                               ws.numel() * 4, stream())
    t.__exit__(None if rc == 0 else DbmmUnsupported, None, None)      # nothing is recorded for a launch that did not happen
    if rc == _lib.E_UNSUPPORTED:
        return None
    check(rc, "conv1x1_bn_act_f16")
    return y


def conv1x1_res_pool_f16(x, c3, residual):
    """fp16 mode, the last block of a stage: (y, AvgPool2d(2) of y) with y = relu(conv1x1(x) * scale + bias + residual) in one launch
    (dbmm_conv1x1_res_pool_f16); x NHWC f16 [B,H,W,128 | 256]; None when the library has no kernel for the shape."""
    require_cuda(x, residual)
    _f16c(x); _f16c(residual)
    w, scale, bias = c3
    Cout, Cin = _rank("conv1x1_res_pool_f16 weight", w, 2).shape
    if x.dim() != 4 or x.shape[1] % 2 or x.shape[2] % 2:
        return None
    B, H, W = x.shape[:3]
    M = B * H * W
    if x.shape[3] != Cin:
        raise RuntimeError(f"conv1x1_res_pool_f16: {x.shape[3]} input channels against a weight {tuple(w.shape)}")
    _conv_f16("conv1x1_res_pool_f16 c3", c3, Cout, Cin)
    _operand("conv1x1_res_pool_f16 residual", residual, torch.float16, M * Cout)
    y = _empty((B, H, W, Cout), device=x.device, dtype=torch.float16)
    yp = _empty((B, H // 2, W // 2, Cout), device=x.device, dtype=torch.float16)
    t = _TimedTag(f"conv1x1_res_stream_f16_kernel<{Cin}, 1>", 2.0 * M * Cout * Cin, 2 * (M * Cin + Cout * Cin + 2 * M * Cout + M // 4 * Cout))
    t.__enter__()
    rc = _lib.lib().dbmm_conv1x1_res_pool_f16(ptr(x), ptr(w), ptr(scale), ptr(bias), ptr(residual), ptr(y), ptr(yp), B, H, W, Cin, Cout, stream())
    t.__exit__(None if rc == 0 else DbmmUnsupported, None, None)
    if rc == _lib.E_UNSUPPORTED:
        return None
    check(rc, "conv1x1_res_pool_f16")
    return y, yp


def chain_f16(y2, c3, residual, c1, pooled=False, keep_full=True):
    """fp16 mode: x' = relu(conv3(y2) * s3 + b3 + residual) and y1' = relu(conv1'(x') * s1 + b1) in one launch (dbmm_bottleneck_chain_f16);
    c3 / c1 = (w f16, scale f32, bias f32).  Returns (x', y1'), or with pooled=True (y2 NHWC [B,H,W,K], a stage seam) (x', AvgPool2d(2) of x',
    y1') where x' is None with keep_full=False (not written); None when the library has no kernel for the shape."""
    require_cuda(y2, residual)
    _f16c(y2); _f16c(residual)
    (w3, s3, b3), (w1, s1, b1) = c3, c1
    N, K = _rank("chain_f16 c3 weight", w3, 2).shape
    P = _rank("chain_f16 c1 weight", w1, 2).shape[0]
    M = y2.numel() // K
    full = keep_full or not pooled
    if pooled and (y2.dim() != 4 or y2.shape[1] % 2 or y2.shape[2] % 2):
        return None
    if y2.shape[-1] != K:
        raise RuntimeError(f"chain_f16: {y2.shape[-1]} input channels against a conv3 weight {tuple(w3.shape)}")
    _conv_f16("chain_f16 c3", c3, N, K); _conv_f16("chain_f16 c1", c1, P, N)
    _operand("chain_f16 residual", residual, torch.float16, M * N)
    x = _empty(tuple(y2.shape[:-1]) + (N,), device=y2.device, dtype=torch.float16) if full else None
    y1 = _empty(tuple(y2.shape[:-1]) + (P,), device=y2.device, dtype=torch.float16)
    xp = _empty((y2.shape[0], y2.shape[1] // 2, y2.shape[2] // 2, N), device=y2.device, dtype=torch.float16) if pooled else None
    tag = f"chain_f16_kernel<{K}, {P}, 0, {int(pooled) + int(not full)}>" if pooled else f"chain_f16_kernel<{K}, {P}>"
    t = _TimedTag(tag, 2.0 * M * N * (K + P), 2 * (M * (K + (2 if full else 1) * N + P) + (M // 4 * N if pooled else 0) + N * (K + P)))
    t.__enter__()
    if pooled:
        B, H, W = y2.shape[:3]
        rc = _lib.lib().dbmm_bottleneck_chain_pool_f16(ptr(y2), ptr(w3), ptr(s3), ptr(b3), ptr(residual), ptr(x), ptr(xp), ptr(w1), ptr(s1), ptr(b1),
                                                       ptr(y1), B, H, W, K, N, P, stream())
    else:
        rc = _lib.lib().dbmm_bottleneck_chain_f16(ptr(y2), ptr(w3), ptr(s3), ptr(b3), ptr(residual), ptr(x), ptr(w1), ptr(s1), ptr(b1), ptr(y1),
                                                  M, K, N, P, stream())
    t.__exit__(None if rc == 0 else DbmmUnsupported, None, None)
    if rc == _lib.E_UNSUPPORTED:
        return None
    check(rc, "bottleneck_chain_f16")
    return (x, xp, y1) if pooled else (x, y1)


def _dual_f16(name, y2, w3, scale3, xp, wd, ratio, bias, M, N, K, K2):
    """the operands of the fp16 dual-source 1x1 conv: y2 [M][K] and xp [M][K2] against w3 [N][K] and wd [N][K2], three [N] vectors"""
    if y2.shape[-1] != K or xp.shape[-1] != K2 or xp.numel() != M * K2:
        raise RuntimeError(f"{name}: inputs {tuple(y2.shape)}, {tuple(xp.shape)} against weights {tuple(w3.shape)}, {tuple(wd.shape)}")
    require_cuda(w3)
    _operand((name, "wd"), wd, torch.float16, (N, K2))
    _operand((name, "scale3"), scale3, torch.float32, N); _operand((name, "ratio"), ratio, torch.float32, N)
    _operand((name, "bias"), bias, torch.float32, N)


def chain_dual_f16(y2, w3, scale3, xp, wd, ratio, bias, c1):
    """fp16 mode: the first block of a stage -- x' = relu(conv3(y2) * scale3 + conv_d(xp) * scale_d + bias) (conv1x1_dual_f16's arguments) and
    y1' = relu(conv1'(x') * s1 + b1) in one launch (dbmm_bottleneck_chain_dual_f16).  Returns (x', y1') or None."""
    require_cuda(y2, xp)
    _f16c(y2); _f16c(xp); _f16c(w3); _f16c(wd)
    w1, s1, b1 = c1
    N, K = _rank("chain_dual_f16 w3", w3, 2).shape
    K2 = _rank("chain_dual_f16 wd", wd, 2).shape[1]
    P = _rank("chain_dual_f16 c1 weight", w1, 2).shape[0]
    M = y2.numel() // K
    _dual_f16("chain_dual_f16", y2, w3, scale3, xp, wd, ratio, bias, M, N, K, K2)
    _conv_f16("chain_dual_f16 c1", c1, P, N)
    x = _empty(tuple(y2.shape[:-1]) + (N,), device=y2.device, dtype=torch.float16)
    y1 = _empty(tuple(y2.shape[:-1]) + (P,), device=y2.device, dtype=torch.float16)
    t = _TimedTag(f"chain_f16_kernel<{K}, {P}, 1>", 2.0 * M * N * (K + K2 + P), 2 * (M * (K + K2 + N + P) + N * (K + K2 + P)))
    t.__enter__()
    rc = _lib.lib().dbmm_bottleneck_chain_dual_f16(ptr(y2), ptr(w3), ptr(scale3), ptr(xp), ptr(wd), ptr(ratio), ptr(bias), ptr(x), ptr(w1), ptr(s1),
                                                   ptr(b1), ptr(y1), M, K, K2, N, P, stream())
    t.__exit__(None if rc == 0 else DbmmUnsupported, None, None)
    if rc == _lib.E_UNSUPPORTED:
        return None
    check(rc, "bottleneck_chain_dual_f16")
    return x, y1


def conv1x1_dual_f16(y2, w3, scale3, xp, wd, ratio, bias, act=ACT_RELU):
    """fp16 mode: act(conv3(y2) * scale3 + conv_d(xp) * scale_d + bias) as one dual-source GEMM (dbmm_conv1x1_dual_bn_act_f16);
    ratio = scale_d / scale3, bias = both BatchNorm biases.  None when the library has no kernel for the shape."""
    require_cuda(y2, xp)
    _f16c(y2); _f16c(xp); _f16c(w3); _f16c(wd)
    Cout, K = _rank("conv1x1_dual_f16 w3", w3, 2).shape
    K2 = _rank("conv1x1_dual_f16 wd", wd, 2).shape[1]
    M = y2.numel() // K
    _dual_f16("conv1x1_dual_f16", y2, w3, scale3, xp, wd, ratio, bias, M, Cout, K, K2)
    out = _empty(tuple(y2.shape[:-1]) + (Cout,), device=y2.device, dtype=torch.float16)
    t = _TimedTag("gemm_f16_8ph_kernel<dual>", 2.0 * M * Cout * (K + K2), 2 * (M * (K + K2) + Cout * (K + K2) + M * Cout))
    t.__enter__()
    rc = _lib.lib().dbmm_conv1x1_dual_bn_act_f16(ptr(y2), ptr(w3), ptr(scale3), ptr(xp), ptr(wd), ptr(ratio), ptr(bias), ptr(out), M, K, K2, Cout,
                                                 act, stream())
    t.__exit__(None if rc == 0 else DbmmUnsupported, None, None)
    if rc == _lib.E_UNSUPPORTED:
        return None
    check(rc, "conv1x1_dual_bn_act_f16")
    return out


def conv3x3_f16(x, w, scale, bias, pool=1):
    """y f16 NHWC = [AvgPool2d(2)] relu(conv3x3(x, stride 1, pad 1) * scale + bias); x f16 [B,H,W,Cin], w f16 [Cout][(cin/32, kh, kw, 32)];
    None when the library has no kernel for the shape."""
    require_cuda(x, w)
    _f16c(x); _f16c(w)
    B, H, W, Cin = x.shape
    Cout = w.shape[0]
    if w.numel() != Cout * 9 * Cin:
        raise RuntimeError(f"conv3x3_f16: packed weight {tuple(w.shape)} for a 3 x 3 conv over {Cin} channels")
    _operand("conv3x3_f16 scale", scale, torch.float32, Cout); _operand("conv3x3_f16 bias", bias, torch.float32, Cout)
    y = _empty((B, H // pool, W // pool, Cout), device=x.device, dtype=torch.float16)
    geo = "2, 2, 2" if Cout > 64 else ("4, 1, 2" if Cout > 32 else "4, 1, 1")
    deep = Cout % 256 == 0 and B * H * W >= 16384 and get_option("f16_conv_8ph")     # dbmm_conv3x3_bn_relu_f16's own routing rule
    tag = f"conv3x3_f16_8ph_kernel<{int(pool == 2)}>" if deep else f"conv3x3_f16_kernel<{geo}, {int(pool == 2)}>"
    if Cin == 32 and Cout in (32, 64) and H % 4 == 0 and W % 28 == 0 and get_option("conv_patch"):      # the stem convs: persistent patch kernel
        tag = f"conv3x3_c32_f16_kernel<{Cout}, {int(pool == 2)}>"
    t = _TimedTag(tag, 2.0 * B * H * W * Cout * 9 * Cin, 2 * (x.numel() + y.numel() + w.numel()))
    t.__enter__()
    rc = _lib.lib().dbmm_conv3x3_bn_relu_f16(ptr(x), ptr(w), ptr(scale), ptr(bias), ptr(y), B, H, W, Cin, Cout, 2 if pool == 2 else 0, stream())
    t.__exit__(None if rc == 0 else DbmmUnsupported, None, None)
    if rc == _lib.E_UNSUPPORTED:
        return None
    check(rc, "conv3x3_bn_relu_f16")
    return y


def conv_stem_s2_f16(x_nchw, w, bias, scale=None):
    """stem conv1 (3x3, stride 2, BatchNorm, ReLU): NCHW f32 / f16 image -> f16 NHWC.  w fp32 [kh][kw][cin][cout].  Without `scale`: w carries
    the folded BatchNorm and is used as it is (FMA kernel); with it: w = the model's fp16 conv weights, BatchNorm = scale / bias on the fp32
    accumulator (dbmm_conv_stem_s2_bn_f16, MFMA gather kernel)."""
    require_cuda(x_nchw, w)
    if x_nchw.dtype not in (torch.float16, torch.float32) or not x_nchw.is_contiguous():
        raise _lib.DbmmError("conv_stem_s2_f16 needs a contiguous float16 / float32 image batch")
    B, C, H, W = x_nchw.shape
    if C != 3:
        raise _lib.DbmmError("stem conv expects 3 input channels")
    Cout = w.shape[-1]
    _operand("conv_stem_s2_f16 weight", w, torch.float32, (3, 3, 3, Cout)); _operand("conv_stem_s2_f16 bias", bias, torch.float32, Cout)
    _optional("conv_stem_s2_f16 scale", scale, torch.float32, Cout)
    y = _empty((B, (H - 1) // 2 + 1, (W - 1) // 2 + 1, Cout), device=x_nchw.device, dtype=torch.float16)
    mfma = scale is not None and get_option("stem_mfma")
    with _TimedTag("stem_s2_f16_mfma_kernel" if mfma else "stem_s2_f16_kernel", 2.0 * y.numel() * 27,
                   x_nchw.numel() * x_nchw.element_size() + 2 * y.numel()):
        if scale is None:
            check(_lib.lib().dbmm_conv_stem_s2_f16(ptr(x_nchw), int(x_nchw.dtype == torch.float16), ptr(w), ptr(bias), ptr(y), B, H, W, Cout,
                                                   stream()), "conv_stem_s2_f16")
        else:
            check(_lib.lib().dbmm_conv_stem_s2_bn_f16(ptr(x_nchw), int(x_nchw.dtype == torch.float16), ptr(w), ptr(scale), ptr(bias), ptr(y), B, H, W,
                                                      Cout, stream()), "conv_stem_s2_bn_f16")
    return y


def avgpool2_f16(x):
    require_cuda(x)
    _f16c(x)
    B, H, W, C = x.shape
    y = _empty((B, H // 2, W // 2, C), device=x.device, dtype=torch.float16)
    with _TimedTag("avgpool2_f16_kernel", 0.0, 2 * (x.numel() + y.numel())):
        check(_lib.lib().dbmm_avgpool2_f16(ptr(x), ptr(y), B, H, W, C, stream()), "avgpool2_f16")
    return y


_TRACE_LAUNCHES = os.environ.get("DBMM_TRACE_LAUNCHES")


class _TimedTag:
    """profile hook for kernels outside the igemm family: fixed tag, caller-supplied FLOPs and algorithmic bytes"""
    def __init__(self, tag, flops, nbytes):
        self.tag, self.flops, self.nbytes = tag, float(flops), float(nbytes)

    def __enter__(self):
        if _TRACE_LAUNCHES:                 # developer aid (DBMM_TRACE_LAUNCHES=<file>): tag before the launch, "ok" after a device sync
            with open(_TRACE_LAUNCHES, "a") as f:
                f.write(self.tag + " ... ")
        self.on = _prof is not None and not _prof_paused and not _prof_conv_only
        if self.on:
            self.e0 = torch.cuda.Event(enable_timing=True)
            self.e0.record()

    def __exit__(self, *exc):
        if _TRACE_LAUNCHES:
            torch.cuda.synchronize()
            with open(_TRACE_LAUNCHES, "a") as f:
                f.write("ok\n")
        if self.on and _prof is not None and exc[0] is None:
            e1 = torch.cuda.Event(enable_timing=True)
            e1.record()
            _prof.append((self.tag, self.flops, self.nbytes, self.e0, e1))
