// Shared helpers for the gfx950 kernels of libdbmm_hip.so, each defined ONCE here:
//   - the vector typedefs of the MFMA fragments and 8 / 16-byte accesses (f16x8, u32x4, ...);
//   - DBMM_N_CU and dbmm_cut_slices: persistent-grid sizing;
//   - wave_sum / wave_sum_f64 / wave_max, xcd_first / xcd_remap: wave reductions, the split of tile ids over the XCDs and the tile -> workgroup map;
//   - desc / glds16 with OOR and EXT_LIM: rebased buffer descriptors and LDS-DMA loads;
//   - scale_exp / pow2f / split2h_pair / frag / pack2: the fp16 (hi, lo) split under an exact power-of-two scale, the
//     library's precision contract.  Every parity kernel splits with THESE functions.
// plus the internal C entries that one kernel file calls in another.
// What only the persistent 256-tile kernels share is defined once in persistent_tiles.h (tile_walk, work_item, slice_store / slice_sum,
// absmax_fold, ring_rows, plan_tiles), the fp16 ring of two of them in fp16_ring.inc, the per-label column sums of k-means and the label sums
// and their fixed-order merge in label_sums.h, and the epilogues that a main kernel and its fixup kernel both run in gemm_f16_8ph_epilogue.inc, gemm_pair_8ph_epilogue.inc and conv3x3_halo8_epilogue.inc.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>
#include "../../include/dbmm.h"

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
typedef unsigned short u16;
typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

constexpr int DBMM_N_CU = 256;                   // compute units of the MI355X: a persistent grid is one workgroup (or a multiple) per CU

#define DBMM_CHECK_LAUNCH()                      \
    do {                                         \
        hipError_t e__ = hipGetLastError();      \
        if (e__ != hipSuccess) return (int)e__;  \
    } while (0)

// library options (csrc/options.hip; set by name through dbmm_set_option, seeded once from DBMM_<NAME> at load time)
enum DbmmOpt {
    OPT_IGEMM_EPI_DIRECT, OPT_IGEMM_FAST, OPT_IGEMM_STREAMK, OPT_IGEMM_X3, OPT_IGEMM_X2, OPT_IGEMM_X2_BK, OPT_IGEMM_BK,
    OPT_IGEMM_HALO, OPT_IGEMM_HALO_POOL, OPT_IGEMM_BN256, OPT_IGEMM_BN256_KXK, OPT_GEMM_8PH, OPT_F16_8PH, OPT_F16_BN256,
    OPT_STEM_MFMA, OPT_MHA_VALU, OPT_CONV_PATCH, OPT_MHA_X2, OPT_ADAPTER_STEP_FUSED, OPT_CONV1X1_STREAM, OPT_CONV1X1_8PH, OPT_CHAIN8, OPT_CONV1X1_BN256, OPT_TAIL_SPLIT, OPT_HALO8, OPT_DUAL_8PH, OPT_MHA_SHORT, OPT_F16_CONV_8PH, OPT_CONV1X1_RES_STREAM, OPT_LINEAR_STEP_ONE_LAUNCH_MAX_B, DBMM_OPT_COUNT
};
int dbmm_opt(int id);

// conv3x3_halo8.hip: parity-mode 3x3 / stride 1 / pad 1 conv (+ scale / bias / ReLU, pool = 2: fused 2x2 average pool) on the eight-phase
// 256 x 256 structure; x NHWC fp32, w ONE fp16 plane [Cout][9 Cin] in the 32-channel-slab K order.  split != 0 + a workspace: the tiles of a short
// last round are cut along K over the idle CUs.  DBMM_E_UNSUPPORTED: not this kernel's shape.
int dbmm_conv3x3_halo8(const float* x, const float* x_absmax, const void* w_plane_f16, int w_exp, const float* out_scale, const float* bias,
                       float* y, float* y_absmax, int64_t B, int64_t H, int64_t W, int64_t Cin, int64_t Cout, int act, int pool, int split,
                       void* workspace, size_t workspace_bytes, void* stream);

// gemm_pair_8ph.hip: dbmm_gemm_pair_8ph (include/dbmm.h) with a workspace: the tiles of a short last round are cut along K over the idle CUs
int dbmm_gemm_pair_8ph_ws(const float* a, int64_t lda, const float* a_absmax, const void* w_plane_f16, int w_exp, int64_t ldw,
                          const float* out_scale, const float* bias, const float* residual, int64_t ldr, float* c, int64_t ldc,
                          float* c_absmax, int64_t M, int64_t N, int64_t K, float alpha, int act, void* workspace, size_t workspace_bytes, void* stream);
// gemm_pair_8ph.hip: dbmm_gemm_dual_bn_act_x2's GEMM on the eight-phase 256 x 256 kernel (arguments checked by the caller)
int dbmm_gemm_dual_pair_8ph(const float* a, int64_t lda, const float* a_absmax, const void* w_plane_f16, int w_exp, int64_t ldw, int64_t K,
                            const float* out_scale, const float* a2, int64_t lda2, const float* a2_absmax, const void* w2_plane_f16, int64_t ldw2,
                            int64_t K2, const float* ratio, const float* bias, float* c, int64_t ldc, float* c_absmax, int64_t M, int64_t N, int act,
                            void* stream);

// K cut of a short last round of the 256-tile persistent kernels: `rem` tiles left for DBMM_N_CU workgroups, `trips` loop trips per tile -> slices
// per tile (0: no cut).  One slice per workgroup at most: a slice costs ~0.3 of a layer-3 tile on top of its share of the loop (prologue,
// 256 KB of partial sums) and the summing launch reads rem x S x 256 KB, so a second slice per workgroup (rem > 128) never paid
// (HISTORY.md, round 4); with rem = 64 and S = 4 the cut is already neutral.
static inline int dbmm_cut_slices(int rem, int trips) {
    if (rem <= 0 || rem > DBMM_N_CU / 2) return 0;
    int S = DBMM_N_CU / rem;
    S = S < trips ? S : trips;
    S = S < 16 ? S : 16;
    return S >= 2 ? S : 0;
}

// conv1x1_res_stream.hip: y = relu((a @ W^T) * scale + bias + residual) (+ y_pooled = AvgPool2d(2) of y), K = 256, N % 32 == 0, M % 4 == 0
int dbmm_conv1x1_res_stream(const float* a, const float* a_absmax, const void* w_plane_f16, int w_exp, const float* scale, const float* bias,
                            const float* residual, float* y, float* y_pooled, float* y_absmax, int64_t M, int64_t Ho, int64_t Wo, int64_t K,
                            int64_t N, void* stream);

// conv1x1_res_stream_f16.hip: the fp16 twin (K = 256, Cout % 64 == 0; y_pooled: also AvgPool2d(2) of y, rows = pixels of [B][Ho][Wo] maps)
int dbmm_conv1x1_res_stream_f16(const void* x, const void* w, const float* scale, const float* bias, const void* residual, void* y, void* y_pooled,
                                int64_t M, int64_t Ho, int64_t Wo, int64_t Cin, int64_t Cout, void* stream);

// supcon.hip: the 5 B + 4 spare floats at the end of a dbmm_supcon_workspace_bytes workspace (the one-call step's stats | l | A)
float* dbmm_supcon_spare(void* workspace, int64_t B);

static inline bool dbmm_aligned16(const void* p) { return (((uintptr_t)p) & 15u) == 0; }

// fp32 rows [N][D] of the analysis kernels that give a lane whole float4s of 64-column groups (covariance.hip, erase.hip)
static inline int dbmm_rows_shape(int64_t N, int64_t D) {
    if (D <= 0 || (D % 64) || D > 4096) return DBMM_E_UNSUPPORTED;
    if (N < 1 || N > (1 << 23)) return DBMM_E_SHAPE;
    return DBMM_OK;
}

// wave64 butterfly sum / max (all lanes get the result)
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}

// The split of n tile ids over the 8 XCDs: XCD x owns the contiguous range [xcd_first(x, n), xcd_first(x + 1, n)), the first
// n % 8 ranges one longer (neighbouring tiles share operand panels in that XCD's L2).  Speed only, never correctness.
__device__ __forceinline__ int xcd_first(int xcd, int n) {
    const int tq = n >> 3, trm = n & 7;
    return xcd < trm ? xcd * (tq + 1) : trm * (tq + 1) + (xcd - trm) * tq;
}
// Bijective XCD-aware remap of a linear workgroup id: blocks are dealt round-robin over the 8 XCDs, block bid is the (bid >> 3)-th
// of XCD bid & 7 and takes that tile of the XCD's range.  (The persistent kernels walk the same ranges: tile_walk, persistent_tiles.h.)
__device__ __forceinline__ int xcd_remap(int bid, int nwg) { return xcd_first(bid & 7, nwg) + (bid >> 3); }

// Buffer addressing.  OOR: a voffset that is out of range for every descriptor (>= any accepted extent, and OOR + (K offset)
// cannot wrap): the hardware drops the store / returns 0 for the load, so ragged edges need no branch.
constexpr unsigned OOR = 0x80000000u;
constexpr long long EXT_LIM = 0x7FFFFFF0LL;

// Buffer descriptor of a tensor of `total` bytes rebased to `shift` bytes (wave-uniform) past its start: extent = what is left
// of the tensor, capped below 2 GiB.  Offsets are then relative to the tile's first row / image, a few MB at most, while the
// tensor itself may be any size.
__device__ __forceinline__ __amdgpu_buffer_rsrc_t desc(const void* base, long long total, long long shift) {
    long long ext = total - shift;
    ext = ext < 0 ? 0 : (ext > EXT_LIM ? EXT_LIM : ext);
    return __builtin_amdgcn_make_buffer_rsrc((void*)((const char*)base + shift), 0, (int)ext, 0x00020000);
}
// LDS-DMA: 16 B per lane from a buffer straight into LDS at (wave-uniform dst) + 16 * lane.
// (The builtin only exists in the device pass, hence the guard; the host pass never calls it.)
__device__ __forceinline__ void glds16(__amdgpu_buffer_rsrc_t r, unsigned char* lds_dst, unsigned voff, unsigned soff) {
#if defined(__HIP_DEVICE_COMPILE__)
    __builtin_amdgcn_raw_ptr_buffer_load_lds(r, (__attribute__((address_space(3))) void*)lds_dst, 16, voff, soff, 0, 0);
#else
    (void)r; (void)lds_dst; (void)voff; (void)soff;
#endif
}

// The fp16-pair split.  Contract: s with amax * 2^s in [2^13, 2^14), clamped to +-60; hi = fp16(x * sc), lo = fp16(x * sc - hi).
// fp16 tops out at 65504 and hi + lo keep 22 bits; the fp32 accumulator is rescaled by 2^-(s + w_exp) in the epilogue --
// powers of two, so the scaling itself is exact.
__device__ __forceinline__ int scale_exp(float amax) {
    const unsigned b = __float_as_uint(amax) & 0x7fffffffu;
    int s = b ? 13 - ((int)(b >> 23) - 127) : 0;
    return s < -60 ? -60 : (s > 60 ? 60 : s);
}
__device__ __forceinline__ float pow2f(int e) { return __uint_as_float((unsigned)(e + 127) << 23); }
// (hi, lo) fp16 pairs of x0 * sc and x1 * sc, packed {x0 | x1 << 16}, on v_fma_mix{lo,hi}_f16
__device__ __forceinline__ void split2h_pair(float x0, float x1, float sc, unsigned& hi, unsigned& lo) {
#if defined(__HIP_DEVICE_COMPILE__)
    asm("v_fma_mixlo_f16 %0, %1, %2, 0" : "=v"(hi) : "v"(x0), "v"(sc));
    asm("v_fma_mixhi_f16 %0, %1, %2, 0" : "+v"(hi) : "v"(x1), "v"(sc));
    asm("v_fma_mixlo_f16 %0, %1, %2, -%3 op_sel_hi:[0,0,1]" : "=v"(lo) : "v"(x0), "v"(sc), "v"(hi));
    asm("v_fma_mixhi_f16 %0, %1, %2, -%3 op_sel:[0,0,1] op_sel_hi:[0,0,1]" : "+v"(lo) : "v"(x1), "v"(sc), "v"(hi));
#else
    (void)x0; (void)x1; (void)sc; hi = lo = 0;
#endif
}
// fp16-mode twin of the packing: {fp16(a) | fp16(b) << 16}
__device__ __forceinline__ unsigned pack2(float a, float b) {
    const f16x2 v = {(_Float16)a, (_Float16)b};
    return __builtin_bit_cast(unsigned, v);
}
// four packed fp16 pairs as one MFMA operand
__device__ __forceinline__ f16x8 frag(const unsigned (&v)[4]) { return __builtin_bit_cast(f16x8, (u32x4){v[0], v[1], v[2], v[3]}); }
