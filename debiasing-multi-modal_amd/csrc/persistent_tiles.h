// What the persistent 256-tile ("eight-phase") kernels share, each stated ONCE:
//   gemm_f16_8ph_kernel (f16_ops.hip), pairdist_tile_kernel (pairdist.hip), gemm_pair_8ph_kernel (gemm_pair_8ph.hip),
//   conv3x3_halo8_kernel / conv3x3_halo8n_kernel (conv3x3_halo8.hip), conv3x3_f16_8ph_kernel (conv_f16.hip) and the three fixup kernels.
//   - tile_walk: a workgroup's tiles -- its XCD's contiguous range (xcd_first, common.h), walked with the stride of the XCD's workgroups;
//   - work_item: whole tiles, then this workgroup's slices of the cut tiles, each a range of loop trips (the K cut of a short last round);
//   - slice_store / slice_sum: the slices' raw accumulators in ws[slice][32][512][4] and their sum in slice order;
//   - absmax_fold: one filtered atomic per workgroup for the output's absmax;
//   - ring_rows: the stager's row / swizzle map of the fp16 ring (fp16_ring.inc holds the ring itself: LDS layout, stage, phase, prologue);
//   - plan_tiles: the host's K-cut plan and persistent grid.
// Phase bodies other than the fp16 ring's stay in their kernels: their staging differs in kind (fp32 through registers, halo strips, taps).
#pragma once
#include "common.h"

constexpr int PH_HALF = 128 * 64 * 2;                              // fp16 ring: bytes of a half-tile (128 rows x 64 k)
constexpr int SLICE_FLOATS = 128 * 512;                            // a slice's accumulators: 128 registers of 512 threads

// This workgroup's whole tiles of [0, n_tiles): number k is tile first + k * stride, k < n_whole; span = tiles of its XCD's range.
struct TileWalk { int first, stride, n_whole, span; };
__device__ __forceinline__ TileWalk tile_walk(int bid, int nwg, int n_tiles) {
    const int xcd = bid & 7, slot_in_xcd = bid >> 3, wg_per_xcd = (nwg - xcd + 7) >> 3;
    const int t_lo = xcd_first(xcd, n_tiles), t_hi = xcd_first(xcd + 1, n_tiles);
    const int n_whole = t_lo + slot_in_xcd < t_hi ? (t_hi - t_lo - slot_in_xcd + wg_per_xcd - 1) / wg_per_xcd : 0;
    return TileWalk{t_lo + slot_in_xcd, wg_per_xcd, n_whole, t_hi - t_lo};
}

// Work items of a workgroup: its n_whole whole tiles (all `trips` loop trips), then its share of the n_sl_all = n_cut * n_slices slices, dealt
// round-robin: slice number bid + j * nwg goes to workgroup bid.  Slice i is cut tile n_full + i / S, loop trips [s T / S, (s + 1) T / S) with
// s = i % S.  (One slice per workgroup at most -- n_sl_all <= nwg, what gemm_f16_impl plans -- is the case j = 0: slice number = bid.)
__device__ __forceinline__ int work_slices(int bid, int nwg, int n_sl_all) { return bid < n_sl_all ? (n_sl_all - 1 - bid) / nwg + 1 : 0; }
struct WorkItem { int tile, slice, trip_lo, trip_hi; };
__device__ __forceinline__ WorkItem work_item(const TileWalk& w, int k, int bid, int nwg, int n_full, int n_slices, int trips) {
    if (k < w.n_whole) return WorkItem{w.first + k * w.stride, 0, 0, trips};
    const int slice = bid + (k - w.n_whole) * nwg;
    const int l = slice / n_slices, sl = slice - l * n_slices;
    return WorkItem{n_full + l, slice, sl * trips / n_slices, (sl + 1) * trips / n_slices};
}

// A slice's raw accumulators: 16 B per thread and store, [register quad][thread][4] (8 KB per workgroup instruction).
// (buffer stores with the register's offset in soffset: 128 flat addresses would be hoisted out of the item loop and spilled)
template <int NI, int NJ>
__device__ __forceinline__ void slice_store(const f32x16 (&acc)[NI][NJ], float* ws, int slice, int tid) {
    const __amdgpu_buffer_rsrc_t rsP = __builtin_amdgcn_make_buffer_rsrc((void*)(ws + (size_t)slice * SLICE_FLOATS), 0, SLICE_FLOATS * 4, 0x00020000);
#pragma unroll
    for (int i = 0; i < NI; ++i)
#pragma unroll
        for (int j = 0; j < NJ; ++j)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const u32x4 v = {__float_as_uint(acc[i][j][4 * q]), __float_as_uint(acc[i][j][4 * q + 1]), __float_as_uint(acc[i][j][4 * q + 2]),
                                 __float_as_uint(acc[i][j][4 * q + 3])};
                __builtin_amdgcn_raw_buffer_store_b128(v, rsP, (unsigned)tid * 16u, (unsigned)(((i * NJ + j) * 4 + q) * 8192), 0);
            }
}
// Cut tile `cut`: accumulator blocks b0 .. b0 + NB - 1 (block = i * NJ + j of the main kernel) summed over the slices in slice order, with the
// main kernel's thread <-> element map.
template <int NB>
__device__ __forceinline__ void slice_sum(f32x16 (&a)[NB], const float* ws, int cut, int n_slices, int b0, int tid) {
    const f32x4* src = (const f32x4*)(ws + (size_t)cut * n_slices * SLICE_FLOATS) + (size_t)b0 * 4 * 512 + tid;
#pragma unroll
    for (int b = 0; b < NB; ++b)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const f32x4 v = src[(4 * b + q) * 512];
#pragma unroll
            for (int e = 0; e < 4; ++e) a[b][4 * q + e] = v[e];
        }
    for (int sl = 1; sl < n_slices; ++sl) {
        src += 32 * 512;
#pragma unroll
        for (int b = 0; b < NB; ++b)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const f32x4 v = src[(4 * b + q) * 512];
#pragma unroll
                for (int e = 0; e < 4; ++e) a[b][4 * q + e] += v[e];
            }
    }
}

// The output's absmax: one (filtered) atomic per workgroup of 512 threads -- all launches of a layer hit ONE address.  red: 8 floats of LDS.
__device__ __forceinline__ void absmax_fold(float* c_absmax, float out_amax, float* red, int tid, int lane, int wid) {
    if (!c_absmax) return;
    out_amax = wave_max(out_amax);
    __syncthreads();
    if (lane == 0) red[wid] = out_amax;
    __syncthreads();
    if (tid == 0) {
        float m = red[0];
#pragma unroll
        for (int i = 1; i < 8; ++i) m = fmaxf(m, red[i]);
        if (m > *(volatile const float*)c_absmax) atomicMax((unsigned*)c_absmax, __float_as_uint(m));
    }
}

// fp16 ring, stager: thread -> LDS chunk (tid + 512 i) of a half-tile = local row lr = (tid >> 3) + 64 i, slot tid & 7; it fetches source
// chunk slot ^ swz(row) (the XOR swizzle that keeps ds_read_b128 conflict-free, applied to the SOURCE chunk index).  Operand rows of half h:
//   A: tile row ra = (lr >> 6) * 128 + h * 64 + (lr & 63);   B: tile column rw = (lr >> 5) * 64 + 2 * (lr & 31) + h
//   (B half 0 = the EVEN columns of every wave column's 64, half 1 = the odd ones: accumulator blocks j = 0 / 1 of a lane are then two
//    ADJACENT output columns -- one packed dword in an epilogue)
// cb = byte offset of the source chunk inside the row's 128-B K tile.
__device__ __forceinline__ void ring_rows(int tid, int i, int h, int& ra, int& rw, unsigned& cb) {
    const int lr = (tid >> 3) + 64 * i, c = (tid & 7) ^ ((lr >> 1) & 7);
    ra = (lr >> 6) * 128 + h * 64 + (lr & 63); rw = (lr >> 5) * 64 + 2 * (lr & 31) + h;
    cb = c * 16u;
}

// Host: the K cut of a short last round and the persistent grid.  p.n_tiles is set; S = slices per cut tile the caller chose (< 2: no cut).
// The rem = n_tiles % DBMM_N_CU tiles of the last round are cut when there is more than one round, the last one is short and the 16-B aligned
// workspace holds rem * S slices; fills p.n_full, p.n_cut, p.n_slices, p.ws and returns the grid (one workgroup per CU).
constexpr size_t SLICE_BYTES = SLICE_FLOATS * sizeof(float);
template <class P>
inline int plan_tiles(P& p, int S, void* workspace, size_t workspace_bytes) {
    p.n_full = p.n_tiles; p.n_cut = 0; p.n_slices = 1; p.ws = nullptr;
    const int rem = p.n_tiles % DBMM_N_CU;
    if (S >= 2 && p.n_tiles > DBMM_N_CU && rem != 0 && workspace && dbmm_aligned16(workspace) && (size_t)rem * S * SLICE_BYTES <= workspace_bytes) {
        p.n_full = p.n_tiles - rem; p.n_cut = rem; p.n_slices = S; p.ws = (float*)workspace;
    }
    return p.n_tiles < DBMM_N_CU ? p.n_tiles : DBMM_N_CU;
}
