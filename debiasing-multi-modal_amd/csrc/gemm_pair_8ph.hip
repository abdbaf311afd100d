// Parity-mode GEMM of the transformer towers on the deep-pipelined structure of gemm_f16_8ph_kernel (f16_ops.hip):
//   c = act(alpha * ((a @ w^T) * out_scale + bias) + residual),  a fp32 [M][K],  w exact in ONE fp16 plane (w * 2^w_exp),
// at fp32 accuracy: a = (hi + lo) * 2^-s, two fp16 MFMA products per fp32 product, fp32 accumulation (the fp16-pair
// split of common.h; clip/model.py:171-240 are the GEMMs it serves in the parity mode).
//
// What differs from the fp16 kernel: the activations are fp32 in HBM, so LDS-DMA brings them in as fp32 and the split into
// (hi, lo) happens when a wave READS its fragments -- 16 VALU per 32 x 16 fragment, placed in the "load" half of a phase,
// i.e. while the other wave group of the SIMD owns the matrix pipe (VALU and MFMA of different waves overlap).  Every
// wave that shares an A row block repeats that split, so the waves are laid out 4 x 2 (64 x 128 of output each; with
// 2 x 4 the four waves of a row quadrupled the split and the kernel ran BELOW the two-barrier one: 337 vs 506 TF-eq at
// K = 4096): two waves per row block = as many split instructions as splitting once on the way into LDS.  To keep two
// buffers of four half-tiles inside LDS a K tile is 32 deep: A half-tile 128 rows x 32 k fp32 = 16 KB (2 DMA instructions
// per thread), W half-tile 128 rows x 32 k fp16 = 8 KB (1), 96 KB in all.  A phase is one 32 x 64 quadrant x 32 k =
// 2 column blocks x 2 k-steps x 2 products = 8 MFMAs, as in the fp16 kernel, and the stage / wait / read distances are the same
// (stage five phases ahead, retire three stages back, read one phase after the wait); only the vmcnt constants differ
// because the stages issue 2 / 1 / 1 / 2 instructions: outstanding after the wait = the last three stages = 5 / 4 / 4 / 5.
// Persistent workgroups, next tile's first five half-tiles issued before the epilogue, epilogue straight from the
// accumulator layout (one register = two 128-B fp32 row segments), branch-free buffer accesses, activation / residual
// compile-time.  Needs N % 256 == 0, K % 64 == 0.
#include <stdlib.h>
#include "persistent_tiles.h"

namespace {

constexpr int A_HALF = 128 * 32 * 4, W_HALF = 128 * 32 * 2;        // bytes of the half-tiles
constexpr int BUF = 2 * A_HALF + 2 * W_HALF;                       // one buffer: Ah0, Bh0, Bh1, Ah1
constexpr int OFF_AH0 = 0, OFF_BH0 = A_HALF, OFF_BH1 = A_HALF + W_HALF, OFF_AH1 = A_HALF + 2 * W_HALF;

struct PairP {
    const float* a; const float* a_absmax; const unsigned short* w; const float* oscale; const float* bias; const float* res;
    float* c; float* c_absmax;
    long long lda, ldw, ldr, ldc, a_total, w_total;
    int M, N, K, w_exp, tiles_n, n_tiles;
    float alpha;
    // TWO: a second operand pair whose K2 / 32 tiles run FIRST (conv3 + downsample branch of a stage's first block as one GEMM, see
    // dbmm_gemm_dual_bn_act_x2): then the accumulators are multiplied per output channel by ratio[n] * 2^(s - s2) and the main pair continues
    const float* a2; const float* a2_absmax; const unsigned short* w2; const float* ratio;
    long long lda2, ldw2, a2_total, w2_total;
    int K2;
    // the tiles of a short last round, cut along K (see pair_8ph_launch): tiles [0, n_full) are computed whole; tile n_full + l (l < n_cut) by
    // n_slices workgroups over a share of the loop trips each, which leave their accumulators in ws[(l * n_slices + s)][32][512][4] for
    // gemm_pair_8ph_fixup_kernel.  Not with TWO.
    int n_full, n_cut, n_slices;
    float* ws;
};

template <int ACT, int RES, int TWO = 0>
__global__ __launch_bounds__(512, 1) void gemm_pair_8ph_kernel(const PairP p) {
    __shared__ __attribute__((aligned(1024))) unsigned char lds[2 * BUF + (TWO ? 8192 : 0)];   // 96 KB (+ TWO: this thread's four column ratios)
    const int tid = threadIdx.x, lane = tid & 63;
    const int wid = __builtin_amdgcn_readfirstlane(tid >> 6), wr = wid >> 1, wc = wid & 1, grp = wid >> 2;   // 4 x 2 waves, two groups of four
    const int fr = lane & 31, fh = lane >> 5;
    const int nwg = gridDim.x;
    const TileWalk walk = tile_walk(blockIdx.x, nwg, p.n_full);
    const __amdgpu_buffer_rsrc_t rsA0 = __builtin_amdgcn_make_buffer_rsrc((void*)p.a, 0, 0, 0x00020000);
    const __amdgpu_buffer_rsrc_t rsW0 = __builtin_amdgcn_make_buffer_rsrc((void*)p.w, 0, 0, 0x00020000);
    __amdgpu_buffer_rsrc_t rsA = rsA0, rsW = rsW0, rsA2 = rsA0, rsW2 = rsW0;
    int m0 = 0, n0 = 0;
    // A half-tile h (128 rows x 32 k): thread -> (local row tid >> 2, k group tid & 3 of 8 k = 32 B of fp32).  Local row lr is
    // tile row (lr >> 5) * 64 + h * 32 + (lr & 31): the h-th 32 rows of every wave row's 64.  W half-tile h by LDS-DMA: chunk
    // tid = local row tid >> 2, slot tid & 3 of a 64-B row, source chunk slot ^ ((row >> 2) & 3); local row lr is tile column
    // (lr >> 6) * 128 + h * 64 + (lr & 63).
    // (TWO: the per-lane offsets of BOTH operand pairs are recomputed where they are used and the ratios wait in LDS -- kept in registers they
    //  pushed the loop over the budget, and every spill reload inside it is a vector-memory load the counted waits then drain behind)
    unsigned voffA[2], voffW[2];
    const int nT2 = TWO ? p.K2 / 32 : 0, nT = nT2 + p.K / 32;         // K tiles of the second pair (they run first) / in all
    const int s_a = scale_exp(*p.a_absmax), s_a2 = TWO ? scale_exp(*p.a2_absmax) : 0;
    const float a_sc = pow2f(s_a), acc_scale = pow2f(-s_a - p.w_exp), a_sc2 = pow2f(s_a2);
    auto set_tile = [&](int tile) {
        m0 = (tile / p.tiles_n) * 256; n0 = (tile % p.tiles_n) * 256;
        rsA = desc(p.a, p.a_total, (long long)m0 * p.lda * 4);
        rsW = desc(p.w, p.w_total, (long long)n0 * p.ldw * 2);
        if constexpr (TWO) {
            rsA2 = desc(p.a2, p.a2_total, (long long)m0 * p.lda2 * 4);
            rsW2 = desc(p.w2, p.w2_total, (long long)n0 * p.ldw2 * 2);
        }
        const int lr = tid >> 2;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int ra = (lr >> 5) * 64 + h * 32 + (lr & 31);
            const unsigned wrow = (unsigned)((lr >> 6) * 128 + h * 64 + (lr & 63)), wsl = (unsigned)(((tid & 3) ^ ((lr >> 2) & 3)) << 4);
            voffA[h] = m0 + ra < p.M ? (unsigned)ra * (unsigned)(p.lda * 4) + (tid & 3) * 32u : OOR;
            voffW[h] = wrow * (unsigned)(p.ldw * 2) + wsl;
        }
        if constexpr (TWO) {                                          // ratio[n] * 2^(s - s2) of this lane's four columns
            f32x4 rr;
#pragma unroll
            for (int j = 0; j < 4; ++j) rr[j] = p.ratio[n0 + (wid & 1) * 128 + 32 * j + (lane & 31)] * pow2f(s_a - s_a2);
            *(f32x4*)(lds + 2 * BUF + tid * 16) = rr;
        }
    };
    auto voff_a = [&](int h, bool second) -> unsigned {               // TWO: the A offset of load_a, from scratch
        const int lr = tid >> 2, ra = (lr >> 5) * 64 + h * 32 + (lr & 31);
        const unsigned ld4 = (unsigned)((second ? p.lda2 : p.lda) * 4);
        return m0 + ra < p.M ? (unsigned)ra * ld4 + (tid & 3) * 32u : OOR;
    };
    auto voff_w = [&](int h, bool second) -> unsigned {
        const int lr = tid >> 2;
        const unsigned ld2 = (unsigned)((second ? p.ldw2 : p.ldw) * 2);
        return (unsigned)((lr >> 6) * 128 + h * 64 + (lr & 63)) * ld2 + (((tid & 3) ^ ((lr >> 2) & 3)) << 4);
    };
    // this thread's 16-B slot inside an fp16 plane of an A half-tile (its 8 k values), and the fragment addresses: A rows
    // wr * 32 + fr, W rows wc * 64 + cb * 32 + fr, chunk 2 ks + fh, 64-B rows swizzled by (row >> 2) & 3
    const int cv_off = (tid >> 2) * 64 + (((tid & 3) ^ (((tid >> 2) >> 2) & 3)) << 4);
    int aoff[2], boff[2][2];
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
        const int r = wr * 32 + fr;
        aoff[ks] = r * 64 + (((2 * ks + fh) ^ ((r >> 2) & 3)) << 4);
#pragma unroll
        for (int cb = 0; cb < 2; ++cb) {
            const int rw = wc * 64 + cb * 32 + fr;
            boff[cb][ks] = rw * 64 + (((2 * ks + fh) ^ ((rw >> 2) & 3)) << 4);
        }
    }
    // A in flight in registers: [half][tile parity][2 x 16 B]
    f32x4 ar[2][2][2];
    auto load_a = [&](int h, int t, int set) {
        const bool second = TWO && t < nT2;                           // (selects, not branches: the phases stay straight-line code)
        // (K tiles past the last one -- the final trip's look-ahead -- fetch whatever follows: split, stored, never multiplied)
        const __amdgpu_buffer_rsrc_t rs = second ? rsA2 : rsA;
        const unsigned vo = TWO ? voff_a(h, second) : voffA[h], so = (unsigned)(second ? t : t - nT2) * 128u;
#pragma unroll
        for (int i = 0; i < 2; ++i)
            ar[h][set][i] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rs, vo, so + i * 16u, 0));
    };
    // split this thread's 8 values ONCE and store them into the (hi, lo) planes of the half-tile's slot
    auto convert_a = [&](int h, int set, int buf, int t = 0) {         // t: the K tile the values belong to (TWO: which operand's scale)
        unsigned hi[4], lo[4];
        const float sc = (TWO && t < nT2) ? a_sc2 : a_sc;
        split2h_pair(ar[h][set][0][0], ar[h][set][0][1], sc, hi[0], lo[0]);
        split2h_pair(ar[h][set][0][2], ar[h][set][0][3], sc, hi[1], lo[1]);
        split2h_pair(ar[h][set][1][0], ar[h][set][1][1], sc, hi[2], lo[2]);
        split2h_pair(ar[h][set][1][2], ar[h][set][1][3], sc, hi[3], lo[3]);
        unsigned char* slot = lds + buf * BUF + (h ? OFF_AH1 : OFF_AH0) + cv_off;
        *(u32x4*)slot = (u32x4){hi[0], hi[1], hi[2], hi[3]};
        *(u32x4*)(slot + A_HALF / 2) = (u32x4){lo[0], lo[1], lo[2], lo[3]};
    };
    auto dma_w = [&](int h, int t, int buf) {
        const bool second = TWO && t < nT2;
        glds16(second ? rsW2 : rsW, lds + buf * BUF + (h ? OFF_BH1 : OFF_BH0) + wid * 1024, TWO ? voff_w(h, second) : voffW[h],
               (unsigned)(second ? t : t - nT2) * 64u);
    };
    f32x16 acc[2][4];                                                 // [A half (32 rows)][W half * 2 + column block]
    u32x4 fah[2], fal[2];                                             // [ks]
    u32x4 fb0[2][2], fb1[2][2];                                       // [column block][ks]

    // One phase.  j = phase within the loop trip (static), t2 = the trip's first K tile (even).  Tile t = t2 + (j >> 2) lives
    // in buffer (j >> 2) & 1; the wave walks its 64 x 128 block as quadrants (A0,B0) (A0,B1) (A1,B1) (A1,B0).  Besides its
    // fragment reads a phase does one piece of staging for later tiles:
    //   p0: convert Ah1(t) -> LDS (read at p2);  DMA Bh1(t + 1) (read at its tile's p1, five phases on)
    //   p1: load Ah0(t + 2) into registers (converted at p2 of t + 1)
    //   p2: convert Ah0(t + 1) -> LDS (read at its p0);  load Ah1(t + 2) into registers (converted at p0 of t + 2);
    //       vmcnt(5) retires the DMA of the last p3
    //   p3: DMA Bh0(t + 2);  vmcnt(5) retires the DMA of this tile's p0
    // (5 = the vector-memory instructions issued after the DMA being retired: 1 + 2 + 2 or 2 + 2 + 1.)  Converted data is
    // read TWO phases after it is stored: the storing wave's lgkmcnt(0) sits behind its first barrier, and the other wave
    // group runs one barrier behind (storing one phase ahead and waiting before the barrier stretched every other interval).
    auto phase = [&](int j, int t2) {
        const int ph = j & 3, buf = (j >> 2) & 1, t = t2 + (j >> 2);
        const unsigned char* base = lds + buf * BUF;
        if (ph == 0) {
#pragma unroll
            for (int cb = 0; cb < 2; ++cb)
#pragma unroll
                for (int ks = 0; ks < 2; ++ks) fb0[cb][ks] = *(const u32x4*)(base + OFF_BH0 + boff[cb][ks]);
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                fah[ks] = *(const u32x4*)(base + OFF_AH0 + aoff[ks]);
                fal[ks] = *(const u32x4*)(base + OFF_AH0 + A_HALF / 2 + aoff[ks]);
            }
            convert_a(1, buf, buf, t);
            __builtin_amdgcn_sched_barrier(0);
            dma_w(1, t + 1, buf ^ 1);
        } else if (ph == 1) {
#pragma unroll
            for (int cb = 0; cb < 2; ++cb)
#pragma unroll
                for (int ks = 0; ks < 2; ++ks) fb1[cb][ks] = *(const u32x4*)(base + OFF_BH1 + boff[cb][ks]);
            __builtin_amdgcn_sched_barrier(0);
            load_a(0, t + 2, buf);
        } else if (ph == 2) {
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                fah[ks] = *(const u32x4*)(base + OFF_AH1 + aoff[ks]);
                fal[ks] = *(const u32x4*)(base + OFF_AH1 + A_HALF / 2 + aoff[ks]);
            }
            convert_a(0, buf ^ 1, buf ^ 1, t + 1);
            __builtin_amdgcn_sched_barrier(0);
            load_a(1, t + 2, buf);
        } else {
            dma_w(0, t + 2, buf);
        }
        __builtin_amdgcn_sched_barrier(0);
        if (ph >= 2) asm volatile("s_waitcnt vmcnt(5)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_sched_barrier(0);
        __builtin_amdgcn_s_setprio(1);
        const int ai = (ph >= 2) ? 1 : 0, bj = (ph == 1 || ph == 2) ? 1 : 0;
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
#pragma unroll
            for (int cb = 0; cb < 2; ++cb)                            // (lo, w) first, then (hi, w)
                acc[ai][2 * bj + cb] = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, fal[ks]), __builtin_bit_cast(f16x8, bj ? fb1[cb][ks] : fb0[cb][ks]),
                                                                              acc[ai][2 * bj + cb], 0, 0, 0);
#pragma unroll
            for (int cb = 0; cb < 2; ++cb)
                acc[ai][2 * bj + cb] = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, fah[ks]), __builtin_bit_cast(f16x8, bj ? fb1[cb][ks] : fb0[cb][ks]),
                                                                              acc[ai][2 * bj + cb], 0, 0, 0);
        }
        __builtin_amdgcn_s_setprio(0);
        __builtin_amdgcn_sched_barrier(0);
        __builtin_amdgcn_s_barrier();
    };
    float out_amax = 0.f;

    // Work items of this workgroup (work_item, persistent_tiles.h): its whole tiles, then its slices of the cut tiles; a loop trip is two K tiles
    const int n_items = walk.n_whole + work_slices(blockIdx.x, nwg, TWO ? 0 : p.n_cut * p.n_slices);
    int tb = 0, te = nT, slice_id = 0;                                // the current item's K tiles [tb, te), both even; its slice number
    auto set_item = [&](int k) {
        const WorkItem it = work_item(walk, k, blockIdx.x, nwg, p.n_full, p.n_slices, nT >> 1);
        tb = 2 * it.trip_lo; te = 2 * it.trip_hi; slice_id = it.slice;
        set_tile(it.tile);
    };
    // the W half-tiles an item needs before its first phases: Bh0, Bh1 of its first K tile into buffer 0, Bh0 of the second into buffer 1
    auto prologue_w = [&]() { dma_w(0, tb, 0); dma_w(1, tb, 0); dma_w(0, tb + 1, 1); };
    if (n_items > 0) { set_item(0); prologue_w(); }
    for (int k = 0; k < n_items; ++k) {
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
        // the activations of the first K tiles go through registers: Ah0 of the first is converted here, its Ah1 and the second tile's halves
        // wait in their register sets for the phases that convert them (p0 / p2 of the first tile, p0 of the second)
        load_a(0, tb, 0); load_a(1, tb, 0); load_a(0, tb + 1, 1); load_a(1, tb + 1, 1);
        convert_a(0, 0, 0, tb);
        // everything older than those loads (the W prologue issued before the previous item's epilogue, that epilogue's loads and
        // stores) has been retired by the wait the conversion needed; the LDS stores are waited for before the barrier
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        if (grp == 1) __builtin_amdgcn_s_barrier();                   // the second wave group runs one barrier behind
        for (int t2 = tb; t2 < te; t2 += 2) {
            if (TWO && t2 == nT2) {                                   // the second pair's sums -> the main pair's scale (both K2 / 32 and t2 are even)
                const f32x4 rr = *(const f32x4*)(lds + 2 * BUF + tid * 16);
#pragma unroll
                for (int i = 0; i < 2; ++i)
#pragma unroll
                    for (int j = 0; j < 4; ++j)
#pragma unroll
                        for (int r = 0; r < 16; ++r) acc[i][j][r] *= rr[j];
            }
#pragma unroll
            for (int j = 0; j < 8; ++j) phase(j, t2);
        }
        if (grp == 0) __builtin_amdgcn_s_barrier();
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");              // the look-ahead loads / DMA past this item's last K tile
        __builtin_amdgcn_s_barrier();                                 // every wave is done with the ring
        const int em0 = m0, en0 = n0, e_slice = slice_id;
        const bool whole = k < walk.n_whole;
        if (k + 1 < n_items) { set_item(k + 1); prologue_w(); }       // in flight during the epilogue below
        if (!whole) { slice_store(acc, p.ws, e_slice, tid); continue; }
        {
            constexpr int EP_NI = 2, EP_NJ = 4, EP_I0 = 0, EP_J0 = 0;
            constexpr bool EP_FULL = true;
#include "gemm_pair_8ph_epilogue.inc"
        }
    }
    absmax_fold(p.c_absmax, out_amax, (float*)lds, tid, lane, wid);              // (its first barrier: all DMA drained at loop exit, the ring is free)
}

}  // namespace

namespace {
// The cut tiles: sum the slices' accumulators in slice order (same thread <-> element mapping as the main kernel), then the main kernel's
// epilogue for ONE 32 x 32 block (i, j) of every wave's 64 x 128 per workgroup -- grid (n_cut, 8).
template <int ACT, int RES>
__global__ __launch_bounds__(512) void gemm_pair_8ph_fixup_kernel(const PairP p) {
    __shared__ float red[8];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, wr = wid >> 1, wc = wid & 1, fr = lane & 31, fh = lane >> 5;
    const int tile = p.n_full + blockIdx.x, em0 = (tile / p.tiles_n) * 256, en0 = (tile % p.tiles_n) * 256;
    f32x16 acc[1][1];
    slice_sum(acc[0], p.ws, blockIdx.x, p.n_slices, blockIdx.y, tid);
    const float acc_scale = pow2f(-scale_exp(*p.a_absmax) - p.w_exp);
    float out_amax = 0.f;
    const int EP_I0 = blockIdx.y >> 2, EP_J0 = blockIdx.y & 3;
    constexpr int EP_NI = 1, EP_NJ = 1;
    constexpr bool EP_FULL = false;
#include "gemm_pair_8ph_epilogue.inc"
    absmax_fold(p.c_absmax, out_amax, red, tid, lane, wid);
}

// Tile quantisation: the persistent grid works in rounds of DBMM_N_CU tiles.  With a workspace the tiles of a short last round are cut along K into
// S slices (dbmm_cut_slices, common.h) dealt over the workgroups, and a small second launch sums the slices and runs the epilogue (as
// conv3x3_halo8.hip does).
int pair_8ph_launch(PairP& p, int act, bool two, void* workspace, size_t workspace_bytes, void* stream) {
    p.tiles_n = p.N / 256;
    p.n_tiles = ((p.M + 255) / 256) * p.tiles_n;
    const int grid = plan_tiles(p, two ? 0 : dbmm_cut_slices(p.n_tiles % DBMM_N_CU, p.K / 64), workspace, workspace_bytes);
    hipStream_t s = (hipStream_t)stream;
#define DBMM_P8(A, R, T) hipLaunchKernelGGL((gemm_pair_8ph_kernel<A, R, T>), dim3(grid), dim3(512), 0, s, p)
    if (two) { if (act == 0) DBMM_P8(0, 0, 1); else if (act == 1) DBMM_P8(1, 0, 1); else return DBMM_E_UNSUPPORTED; }
    else if (p.res) { if (act == 0) DBMM_P8(0, 1, 0); else if (act == 1) DBMM_P8(1, 1, 0); else DBMM_P8(2, 1, 0); }
    else { if (act == 0) DBMM_P8(0, 0, 0); else if (act == 1) DBMM_P8(1, 0, 0); else DBMM_P8(2, 0, 0); }
#undef DBMM_P8
    DBMM_CHECK_LAUNCH();
    if (p.n_cut) {
#define DBMM_P8F(A, R) hipLaunchKernelGGL((gemm_pair_8ph_fixup_kernel<A, R>), dim3(p.n_cut, 8), dim3(512), 0, s, p)
        if (p.res) { if (act == 0) DBMM_P8F(0, 1); else if (act == 1) DBMM_P8F(1, 1); else DBMM_P8F(2, 1); }
        else { if (act == 0) DBMM_P8F(0, 0); else if (act == 1) DBMM_P8F(1, 0); else DBMM_P8F(2, 0); }
#undef DBMM_P8F
        DBMM_CHECK_LAUNCH();
    }
    return DBMM_OK;
}
}  // namespace

// common.h: dbmm_gemm_pair_8ph with a workspace for the K cut of a short last round (null: one launch)
int dbmm_gemm_pair_8ph_ws(const float* a, int64_t lda, const float* a_absmax, const void* w_plane_f16, int w_exp, int64_t ldw,
                          const float* out_scale, const float* bias, const float* residual, int64_t ldr, float* c, int64_t ldc,
                          float* c_absmax, int64_t M, int64_t N, int64_t K, float alpha, int act, void* workspace, size_t workspace_bytes, void* stream) {
    if (!a || !a_absmax || !w_plane_f16 || !c) return DBMM_E_ARG;
    if (M <= 0 || N <= 0 || K <= 0 || M > INT32_MAX || N > INT32_MAX || K > INT32_MAX) return DBMM_E_SHAPE;
    if (act < 0 || act > 2) return DBMM_E_ARG;
    if ((N % 256) || (K % 64) || w_exp < -40 || w_exp > 40) return DBMM_E_UNSUPPORTED;
    if ((lda & 3) || (ldw & 7) || !dbmm_aligned16(a) || !dbmm_aligned16(w_plane_f16) || !dbmm_aligned16(c) ||
        (residual && !dbmm_aligned16(residual)))
        return DBMM_E_ALIGN;
    const long long wb = ((N - 1) * ldw + K) * 2;
    if (wb >= EXT_LIM || 256 * lda * 4 >= EXT_LIM || 256 * ldc * 4 >= EXT_LIM || (residual && 256 * ldr * 4 >= EXT_LIM)) return DBMM_E_UNSUPPORTED;
    PairP p{};
    p.a = a; p.a_absmax = a_absmax; p.w = (const unsigned short*)w_plane_f16; p.oscale = out_scale; p.bias = bias; p.res = residual;
    p.c = c; p.c_absmax = c_absmax;
    p.lda = lda; p.ldw = ldw; p.ldr = ldr; p.ldc = ldc; p.a_total = ((M - 1) * lda + K) * 4; p.w_total = wb;
    p.M = (int)M; p.N = (int)N; p.K = (int)K; p.w_exp = w_exp; p.alpha = alpha;
    return pair_8ph_launch(p, act, false, workspace, workspace_bytes, stream);
}

// see include/dbmm.h
extern "C" int dbmm_gemm_pair_8ph(const float* a, int64_t lda, const float* a_absmax, const void* w_plane_f16, int w_exp, int64_t ldw,
                                  const float* out_scale, const float* bias, const float* residual, int64_t ldr, float* c, int64_t ldc,
                                  float* c_absmax, int64_t M, int64_t N, int64_t K, float alpha, int act, void* stream) {
    return dbmm_gemm_pair_8ph_ws(a, lda, a_absmax, w_plane_f16, w_exp, ldw, out_scale, bias, residual, ldr, c, ldc, c_absmax, M, N, K, alpha, act, nullptr, 0,
                                 stream);
}

// common.h: the dual-source GEMM of dbmm_gemm_dual_bn_act_x2 on this kernel (TWO = 1).  DBMM_E_UNSUPPORTED: not this kernel's shape.
int dbmm_gemm_dual_pair_8ph(const float* a, int64_t lda, const float* a_absmax, const void* w_plane_f16, int w_exp, int64_t ldw, int64_t K,
                            const float* out_scale, const float* a2, int64_t lda2, const float* a2_absmax, const void* w2_plane_f16, int64_t ldw2,
                            int64_t K2, const float* ratio, const float* bias, float* c, int64_t ldc, float* c_absmax, int64_t M, int64_t N, int act,
                            void* stream) {
    if ((N % 256) || (K % 64) || (K2 % 64) || M < 16384 || (act != 0 && act != 1)) return DBMM_E_UNSUPPORTED;
    const long long wb = ((N - 1) * ldw + K) * 2, wb2 = ((N - 1) * ldw2 + K2) * 2;
    if (wb >= EXT_LIM || wb2 >= EXT_LIM || 256 * lda * 4 >= EXT_LIM || 256 * lda2 * 4 >= EXT_LIM || 256 * ldc * 4 >= EXT_LIM) return DBMM_E_UNSUPPORTED;
    PairP p{};
    p.a = a; p.a_absmax = a_absmax; p.w = (const unsigned short*)w_plane_f16; p.oscale = out_scale; p.bias = bias; p.res = nullptr;
    p.c = c; p.c_absmax = c_absmax;
    p.lda = lda; p.ldw = ldw; p.ldr = 0; p.ldc = ldc; p.a_total = ((M - 1) * lda + K) * 4; p.w_total = wb;
    p.M = (int)M; p.N = (int)N; p.K = (int)K; p.w_exp = w_exp; p.alpha = 1.f;
    p.a2 = a2; p.a2_absmax = a2_absmax; p.w2 = (const unsigned short*)w2_plane_f16; p.ratio = ratio;
    p.lda2 = lda2; p.ldw2 = ldw2; p.a2_total = ((M - 1) * lda2 + K2) * 4; p.w2_total = wb2; p.K2 = (int)K2;
    return pair_8ph_launch(p, act, true, nullptr, 0, stream);
}
