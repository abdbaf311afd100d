// Group-wise sums of pairwise Euclidean distances (the numbers behind the reference's representation report,
// demo/visualizer.py:650-690: scipy.cdist(X, X) summed, for the whole split and once per group) WITHOUT the N x N matrix:
//   S[a][b] = sum over unordered pairs i < j with {g_i, g_j} = {a, b} of ||x_i - x_j||_2,   float64 [G][G], symmetric.
// Every pair is visited once: d^2 = |a|^2 + |b|^2 - 2 a.b over 256 x 256 tiles of the UPPER TRIANGLE of the Gram matrix, sqrt and
// the bucket reduction in the epilogue, straight from the accumulator layout.
//
// Arithmetic.  The rows are centred first (x - centre: distances do not change, the cancellation in |a|^2 + |b|^2 - 2 a.b mostly
// goes), scaled by an exact power of two so that the largest centred magnitude lies in [2^13, 2^14), and split into two fp16
// planes hi = fp16(v), lo = fp16(v - hi) (22 bits).  The Gram product is hi.hi + hi.lo + lo.hi, three fp16 MFMA products with
// fp32 accumulation (lo.lo is below 2^-22 of |a||b|); the row norms are taken from the same rounded values hi + lo, so a pair of
// identical rows differs from zero only by the accumulation's rounding, and d^2 is clamped at 0.  The diagonal is excluded by
// index, not by value.
//
// Structure.  pairdist_split_kernel writes the planes as ONE fp16 matrix P [N][2 Dp] (row = hi | lo, Dp = D rounded up to 128,
// zero padded) plus {norm, group} per row.  The tile product runs on the shared fp16 ring (fp16_ring.inc, the one gemm_f16_8ph_kernel
// uses: 256 x 256 x 64 tiles, LDS-DMA half-tiles staged five phases ahead, two wave rows one barrier apart) under persistent workgroups
// (tile_walk, persistent_tiles.h; the next tile's prologue in flight during the epilogue).  What is this kernel's own is the source map
// (ring_src), the range check of the B rows and the epilogue.  K is 3 Dp: K tile t reads A from plane columns (t < T ? t : t - T)
// and B from (t < 2 T ? t : t - 2 T), T = Dp / 64, i.e. the segments hi.hi, hi.lo, lo.hi.  Both operands are row blocks of P.
//
// Determinism.  No floating-point atomics: a lane sums its 128 distances in float64, a wave folds them by butterfly, eight wave
// slots are added in wave order, a workgroup keeps one float64 running sum per (row group, column group) over ITS tiles (the tile ->
// workgroup map is static), and pairdist_fold_kernel adds the workgroups' 64 sums in workgroup order.  Rows sorted by group make
// nearly every tile single-bucket (the fast path: no predicates); mixed, ragged and diagonal tiles take the predicated path.
// Workspace: the planes (4 Dp bytes per row), 8 bytes per row, 512 bytes per workgroup -- O(N D), never O(N^2).
//
// Element maps.  The tile kernel is a template on what a pair adds to its bucket: DistanceMap (sqrt(d^2), one sum: the kernel above) and
// RbfMap (exp(-gamma_l d^2) for L <= 4 bandwidths: the bucket sums MMD^2 and HSIC are made of, dbmm_pairdist_rbf_group_sums).  For RbfMap
// d^2 stays in the accumulator registers and the reduction above runs once per l, l OUTSIDE the lane's 128 elements: a runtime loop, so
// the instructions that form a bandwidth's sums are the same whatever L is (L = 4 in one call equals four L = 1 calls bit for bit).
// k = exp2(c_l d^2) on the hardware exponential, c_l = -gamma_l log2(e) 2^(-2s) with the split's scale exponent s read on the device.
// Everything else -- planes, RowInfo, ring, walk, clamp, masks, wave slots, the workgroup's running sums (thread 64 l + b), the fold -- is
// one text; the workspace grows by 512 bytes per workgroup and bandwidth.
#include <stdlib.h>
#include "persistent_tiles.h"
#include "../../include/dbmm_kernel_ops.h"

namespace {

constexpr int MAX_WG = DBMM_N_CU;                                  // persistent grid: one workgroup per CU
constexpr int NO_GROUP = 15;                                       // rows past N / labels outside [0, G): in no bucket
constexpr size_t HEAD_BYTES = 256;                                 // workspace head: the centred absmax (uint bits)

struct RowInfo { float norm; int group; };                         // |hi + lo|^2 in scaled units, group label or NO_GROUP

// max |x - centre| over the split (an integer max of the float bits: the order of the atomics does not matter)
__global__ __launch_bounds__(256) void pairdist_absmax_kernel(const float* __restrict__ x, const float* __restrict__ c, long long n4, int D4,
                                                              unsigned* __restrict__ amax_bits) {
    __shared__ float red[4];
    float m = 0.f;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long long)gridDim.x * 256) {
        const f32x4 v = ((const f32x4*)x)[i], cc = ((const f32x4*)c)[i % D4];
#pragma unroll
        for (int e = 0; e < 4; ++e) m = fmaxf(m, fabsf(v[e] - cc[e]));
    }
    m = wave_max(m);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        m = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
        if (m == m && m < 3.0e38f) atomicMax(amax_bits, __float_as_uint(m));
    }
}

// one wave per row: centre, scale, split; P[row] = hi[0 .. Dp) | lo[0 .. Dp), info[row] = {sum (hi + lo)^2, group}; without LABELS g is
// not read and every row is in no group (the weighted rows pass has no labels)
template <bool LABELS>
__global__ __launch_bounds__(256) void pairdist_split_kernel(const float* __restrict__ x, const float* __restrict__ c, const int64_t* __restrict__ g,
                                                             const unsigned* __restrict__ amax_bits, u16* __restrict__ P, RowInfo* __restrict__ info,
                                                             int N, int D, int Dp, int G) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= N) return;
    const float sc = pow2f(scale_exp(__uint_as_float(*amax_bits)));
    const float* xr = x + (size_t)row * D;
    unsigned* ph = (unsigned*)(P + (size_t)row * 2 * Dp);
    unsigned* pl = ph + Dp / 2;
    float nrm = 0.f;
    for (int k = 2 * lane; k < Dp; k += 128) {
        unsigned hb = 0, lb = 0;
        if (k < D) {                                               // D is even: a pair is inside or outside
            const float v0 = (xr[k] - c[k]) * sc, v1 = (xr[k + 1] - c[k + 1]) * sc;
            const _Float16 h0 = (_Float16)v0, h1 = (_Float16)v1;
            const _Float16 l0 = (_Float16)(v0 - (float)h0), l1 = (_Float16)(v1 - (float)h1);
            const float r0 = (float)h0 + (float)l0, r1 = (float)h1 + (float)l1;
            nrm = fmaf(r0, r0, nrm); nrm = fmaf(r1, r1, nrm);
            hb = __builtin_bit_cast(unsigned, (f16x2){h0, h1});
            lb = __builtin_bit_cast(unsigned, (f16x2){l0, l1});
        }
        ph[k >> 1] = hb; pl[k >> 1] = lb;
    }
    nrm = wave_sum(nrm);
    if (lane == 0) {
        const int64_t gv = LABELS ? g[row] : -1;
        info[row] = RowInfo{nrm, (gv >= 0 && gv < G) ? (int)gv : NO_GROUP};
    }
}

constexpr int RBF_MAX_L = 4;                                      // bandwidths of one RBF pass: e_wsum [4][8][64] is 16 KB beside the ring

struct PairDistP {
    const u16* P; const RowInfo* info; double* part;               // part [MAX_WG][L][64]: a workgroup's sums per (l, row group * 8 + column group)
    long long ldp, p_total;                                        // halves per row of P (2 Dp), bytes of P
    int N, T, nb, n_tiles;                                         // T = Dp / 64 K tiles per plane, nb = row blocks of 256
    const unsigned* amax_bits; double gamma[RBF_MAX_L]; int L;     // RbfMap only: the split's absmax (its scale exponent), the L bandwidths
};

struct PairRowsP;                                                  // the rows kernel's parameters, below: each map names its own
struct PairRowsRbfP;
struct PairRowsMatvecP;

// The element maps of the tile kernel: what a pair adds to its bucket, from its d^2 >= 0 in scaled units (2^-2s of the rows' own).
// pre() is applied once to every accumulator element, in place; val(a, coef(p, l)) is summed, once per l < n_sums(p).
struct DistanceMap {                                               // ||x_i - x_j||: one sum per bucket, in units of 2^-s
    static constexpr int MAX_L = 1;
    static constexpr bool SCALED = true;
    static constexpr bool WEIGHTED = false;
    using RowsP = PairRowsP;
    template <class Params> static __device__ __forceinline__ int n_sums(const Params&) { return 1; }
    static __device__ __forceinline__ float pre(float d2) { return __builtin_sqrtf(d2); }
    template <class Params> static __device__ __forceinline__ float coef(const Params&, int) { return 0.f; }
    static __device__ __forceinline__ float val(float a, float) { return a; }
    static __device__ __forceinline__ float per_group(float c) { return c; }
    static __device__ __forceinline__ float self_pair() { return 0.f; }      // the rows kernel's (i, i): a distance of 0 adds nothing
    static __device__ __forceinline__ float self_coef(float c) { return c; }
};
struct RbfMap {                                                    // exp(-gamma_l ||x_i - x_j||^2), l < L: d^2 stays in the registers, L sums per bucket
    static constexpr int MAX_L = RBF_MAX_L;
    static constexpr bool SCALED = false;
    static constexpr bool WEIGHTED = false;
    using RowsP = PairRowsRbfP;
    template <class Params> static __device__ __forceinline__ int n_sums(const Params& p) { return p.L; }
    static __device__ __forceinline__ float pre(float d2) { return d2; }
    // c_l = -gamma_l log2(e) 2^(-2s), formed in float64 (|s| <= 60: either factor alone may leave fp32's range) and rounded once
    template <class Params> static __device__ __forceinline__ float coef(const Params& p, int l) {
        const double u = (double)pow2f(-scale_exp(__uint_as_float(*p.amax_bits)));
        return (float)(-p.gamma[l] * 1.4426950408889634 * u * u);
    }
    // the hardware exponential on a non-positive argument: underflow to 0 is the answer
    static __device__ __forceinline__ float val(float a, float c) { return __builtin_amdgcn_exp2f(c * a); }
    // the predicated path's coefficient, opaque per row group: hoisted out of that loop the 128 float64 kernel values of a lane would
    // have to live across it, and the registers go to them instead of d^2
    static __device__ __forceinline__ float per_group(float c) { asm volatile("" : "+v"(c)); return c; }
    // the rows kernel's (i, i): d^2 = +inf, whose kernel value exp2(-inf) is an exact 0 at every bandwidth -- for a coefficient that is not
    // a zero (0 x inf is nan): self_coef keeps it at or below the largest negative normal number, which changes no kernel value
    // (|c d^2| < 2^-96 there: exp2 gives 1 either way)
    static __device__ __forceinline__ float self_pair() { return __builtin_inff(); }
    static __device__ __forceinline__ float self_coef(float c) { return fminf(c, -1.17549435e-38f); }
};
// The rows kernel only: RbfMap's kernel values at ONE bandwidth, each column j weighted by v[j][c] for c < G weight columns instead of
// being bucketed by a label: R[i][c] = sum over j != i of exp(-gamma ||x_i - x_j||^2) v[j][c], the kernel-matrix product
struct RbfMatvecMap : RbfMap {
    static constexpr bool WEIGHTED = true;
    using RowsP = PairRowsMatvecP;
};

// Two statements of both tile kernels, stated once -- as text, not as functions: each was tried as a lambda and as a __forceinline__
// helper, and every form moved the register allocation around the ring (the rows kernel has two registers to spare there).
// The stager's lane offsets of thread t for the tile at (m0, n0), per half-tile kind (Ah0, Bh0, Bh1, Ah1); rows >= N masked.  In scope: voff,
// m0, n0, p
#define PAIRDIST_LANE_OFFSETS(t)                                                                                    \
    _Pragma("unroll") for (int i = 0; i < 2; ++i) {                                                                 \
        _Pragma("unroll") for (int h = 0; h < 2; ++h) {                                                             \
            int ra, rw;                                                                                             \
            unsigned cb;                                                                                            \
            ring_rows(t, i, h, ra, rw, cb);                                                                         \
            voff[h ? 3 : 0][i] = m0 + ra < p.N ? (unsigned)ra * (unsigned)(p.ldp * 2) + cb : OOR;                   \
            voff[h ? 2 : 1][i] = n0 + rw < p.N ? (unsigned)rw * (unsigned)(p.ldp * 2) + cb : OOR;                   \
        }                                                                                                           \
    }
// The accumulators -> Map::pre(d^2) in place, d^2 = |a|^2 + |b|^2 - 2 a.b clamped at 0.  In scope: acc, e_norm (the tile's row norms, then
// its column norms), wm0, c0 (the lane's first column), fh; defines cn0, cn1
#define PAIRDIST_ACC_TO_D2()                                                                                        \
    const float cn0 = e_norm[256 + c0], cn1 = e_norm[256 + c0 + 1];                                                 \
    _Pragma("unroll") for (int i = 0; i < 4; ++i)                                                                   \
        _Pragma("unroll") for (int r = 0; r < 16; ++r) {                                                            \
            const float rn = e_norm[wm0 + 32 * i + (r & 3) + 8 * (r >> 2) + 4 * fh];                                \
            acc[i][0][r] = Map::pre(fmaxf(fmaf(-2.f, acc[i][0][r], rn + cn0), 0.f));                                \
            acc[i][1][r] = Map::pre(fmaxf(fmaf(-2.f, acc[i][1][r], rn + cn1), 0.f));                                \
        }

template <class Map>
__global__ __launch_bounds__(512, 1) void pairdist_tile_kernel(const PairDistP p) {
    __shared__ __attribute__((aligned(1024))) unsigned char lds[8 * PH_HALF];      // [buffer 2][Ah0, Bh0, Bh1, Ah1] = 128 KB
    __shared__ float e_norm[512];                                  // epilogue: norms of the tile's 256 rows, then of its 256 columns
    __shared__ unsigned char e_grp[512];
    __shared__ unsigned e_mask[2];                                 // groups present among the rows / the columns
    __shared__ double e_wsum[Map::MAX_L][8][64];                   // per sum l, per wave, per bucket
    const int tid = threadIdx.x, lane = tid & 63;
    const int wid = __builtin_amdgcn_readfirstlane(tid >> 6), wr = wid >> 2, wc = wid & 3;
    const int fr = lane & 31, fh = lane >> 5;
    const TileWalk walk = tile_walk(blockIdx.x, gridDim.x, p.n_tiles);
    const __amdgpu_buffer_rsrc_t rs0 = __builtin_amdgcn_make_buffer_rsrc((void*)p.P, 0, 0, 0x00020000);
    __amdgpu_buffer_rsrc_t rsA = rs0, rsW = rs0;
    int m0 = 0, n0 = 0;
    unsigned voff[4][2];                                           // the stager's lane offsets per half-tile kind (Ah0, Bh0, Bh1, Ah1); rows >= N masked
    // tile number -> (row block bi <= column block bj) of the upper triangle, row-major: row bi starts at bi * nb - bi (bi - 1) / 2
    auto set_tile = [&](int tile) {
        const double w = 2.0 * p.nb + 1.0;
        int bi = (int)((w - sqrt(w * w - 8.0 * tile)) * 0.5);
        bi = bi < 0 ? 0 : (bi > p.nb - 1 ? p.nb - 1 : bi);
        auto start = [&](int b) { return (long long)b * p.nb - (long long)b * (b - 1) / 2; };
        while (bi > 0 && start(bi) > tile) --bi;
        while (bi + 1 < p.nb && start(bi + 1) <= tile) ++bi;
        const int bj = bi + (int)(tile - start(bi));
        m0 = bi * 256; n0 = bj * 256;
        rsA = desc(p.P, p.p_total, (long long)m0 * p.ldp * 2);
        rsW = desc(p.P, p.p_total, (long long)n0 * p.ldp * 2);
        PAIRDIST_LANE_OFFSETS(tid);
    };
#include "pairdist_ring.inc"

    const int n_items = walk.n_whole;
    const int wm0 = wr * 128, wn0 = wc * 64;
    const int nl = Map::n_sums(p);
    double total = 0.0;                                               // thread 64 l + b, l < nl: this workgroup's sum l of bucket b
    if (tid < 2) e_mask[tid] = 0u;
    if (n_items > 0) { set_tile(walk.first); ring_prologue(0); }
    for (int k = 0; k < n_items; ++k) {
        ring_item(0, nT, true, [](int) {});                           // (no epilogue stores: every item waits for all of its prologue)
        const int em0 = m0, en0 = n0;
        if (k + 1 < n_items) { set_tile(walk.first + (k + 1) * walk.stride); ring_prologue(0); }   // in flight during the epilogue

        // ---- epilogue: distances and bucket sums straight from the accumulators -------------------------------------------
        // lane (fr, fh) holds columns wn0 + 2 fr + j (blocks j = 0 / 1: the B halves are the even / odd columns) of rows
        // wm0 + 32 i + (r & 3) + 8 (r >> 2) + 4 fh.
        {
            const int src = (tid < 256 ? em0 : en0 - 256) + tid;      // threads 0 .. 255: the tile's rows, 256 .. 511: its columns
            RowInfo ri{0.f, NO_GROUP};
            if (src < p.N) ri = p.info[src];
            e_norm[tid] = ri.norm;
            e_grp[tid] = (unsigned char)ri.group;
            if (ri.group != NO_GROUP) atomicOr(&e_mask[tid >> 8], 1u << ri.group);   // integer, order-free
        }
        __syncthreads();
        const unsigned mA = e_mask[0], mB = e_mask[1];
        const bool diag = em0 == en0;
        const bool fast = !diag && em0 + 256 <= p.N && en0 + 256 <= p.N && __builtin_popcount(mA) == 1 && __builtin_popcount(mB) == 1;
        const int c0 = wn0 + 2 * fr;
        PAIRDIST_ACC_TO_D2();
        // one reduction per sum l, the same whatever nl is: l outside the lane's 128 elements, no second copy of the tile
#pragma unroll 1
        for (int l = 0; l < nl; ++l) {
            const float cf = Map::coef(p, l);
            if (fast) {
                double s = 0.0;
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int r = 0; r < 16; ++r) s += (double)Map::val(acc[i][0][r], cf) + (double)Map::val(acc[i][1][r], cf);
                s = wave_sum_f64(s);
                if (lane == 0) e_wsum[l][wid][(__builtin_ctz(mA) << 3) + __builtin_ctz(mB)] = s;
            } else {
                const int gb0 = e_grp[256 + c0], gb1 = e_grp[256 + c0 + 1];
                for (unsigned ma = mA; ma; ma &= ma - 1) {
                    const int ga = __builtin_ctz(ma);
                    const float cg = Map::per_group(cf);
                    double v0 = 0.0, v1 = 0.0;
#pragma unroll
                    for (int i = 0; i < 4; ++i)
#pragma unroll
                        for (int r = 0; r < 16; ++r) {
                            const int lr = wm0 + 32 * i + (r & 3) + 8 * (r >> 2) + 4 * fh;
                            const bool in = e_grp[lr] == ga;
                            v0 += (in && (!diag || lr < c0)) ? (double)Map::val(acc[i][0][r], cg) : 0.0;
                            v1 += (in && (!diag || lr < c0 + 1)) ? (double)Map::val(acc[i][1][r], cg) : 0.0;
                        }
                    for (unsigned mb = mB; mb; mb &= mb - 1) {
                        const int gb = __builtin_ctz(mb);
                        const double s = wave_sum_f64((gb0 == gb ? v0 : 0.0) + (gb1 == gb ? v1 : 0.0));
                        if (lane == 0) e_wsum[l][wid][(ga << 3) + gb] = s;
                    }
                }
            }
        }
        __syncthreads();
        if (tid < 64 * nl && ((mA >> ((tid & 63) >> 3)) & 1u) && ((mB >> (tid & 7)) & 1u)) {
            double s = 0.0;
#pragma unroll
            for (int w = 0; w < 8; ++w) s += e_wsum[tid >> 6][w][tid & 63];
            total += s;
        }
        __syncthreads();
        if (tid < 2) e_mask[tid] = 0u;                                // for the next tile: its atomics come after that tile's ring barriers
    }
    if (tid < 64 * nl) p.part[(size_t)blockIdx.x * (64 * nl) + tid] = total;
}

// workgroup sums -> S [L][G][G], block l folds sum l: bucket (a, b) of the kernel is "row in group a, column in group b"; unordered pairs
// fold (a, b) and (b, a).  amax_bits: distances were taken in units of 2^-s and are rescaled; null for kernel values, which have no unit
__global__ __launch_bounds__(64) void pairdist_fold_kernel(const double* __restrict__ part, int n_wg, const unsigned* __restrict__ amax_bits, int G,
                                                           double* __restrict__ S) {
    __shared__ double tot[64];
    const int b = threadIdx.x, l = blockIdx.x, nl = gridDim.x;
    double s = 0.0;
    for (int w = 0; w < n_wg; ++w) s += part[((size_t)w * nl + l) * 64 + b];
    tot[b] = s;
    __syncthreads();
    const int ga = b >> 3, gb = b & 7;
    if (ga < G && gb < G) {
        const int e = amax_bits ? -scale_exp(__uint_as_float(*amax_bits)) : 0;
        const double v = ga == gb ? tot[b] : tot[(ga << 3) + gb] + tot[(gb << 3) + ga];
        S[(l * G + ga) * G + gb] = ldexp(v, e);
    }
}

inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }
inline long long padded_dim(long long D) { return (D + 127) / 128 * 128; }

// The workspace of every pass: the head, RowInfo, the planes, then the pass's partials (part_bytes of them); byte offsets and the total
struct Layout { size_t info, planes, part, total; };
inline Layout layout(int64_t N, int64_t D, size_t part_bytes) {
    Layout w;
    w.info = HEAD_BYTES;
    w.planes = w.info + align_up((size_t)N * sizeof(RowInfo), 256);
    w.part = w.planes + align_up((size_t)N * 2 * (size_t)padded_dim(D) * 2, 256);
    w.total = w.part + part_bytes;
    return w;
}

// the partials of a bucket pass with L sums per bucket: 64 buckets per workgroup and sum
inline size_t bucket_workspace_bytes(int64_t N, int64_t D, int64_t L) { return layout(N, D, (size_t)MAX_WG * (size_t)L * 64 * sizeof(double)).total; }

// The operand check of every public entry, in the order the callers rely on: shape, unsupported width, null, gamma, alignment, workspace.
// cap: the entry's most labels or weight columns G; groups / gammas / v: checked where the entry takes them (`takes`), gammas being L host
// values; required: the entry's workspace size for this request
enum : unsigned { TAKES_GROUPS = 1, TAKES_GAMMAS = 2, TAKES_V = 4 };
int check_operands(unsigned takes, int64_t cap, const float* x, const int64_t* groups, const float* v, const float* center, const double* gammas, int64_t L,
                   const double* sums, int64_t N, int64_t D, int64_t G, const void* workspace, size_t workspace_bytes, size_t required) {
    if (N <= 0 || D <= 0 || N > (1 << 23) || G < 1 || G > cap || L < 1 || L > RBF_MAX_L) return DBMM_E_SHAPE;
    if ((D % 64) || D > 4096) return DBMM_E_UNSUPPORTED;
    if (!x || !center || !sums || !workspace) return DBMM_E_ARG;
    if (((takes & TAKES_GROUPS) && !groups) || ((takes & TAKES_GAMMAS) && !gammas) || ((takes & TAKES_V) && !v)) return DBMM_E_ARG;
    for (int l = 0; (takes & TAKES_GAMMAS) && l < L; ++l)
        if (!(gammas[l] > 0.0) || !(gammas[l] <= 1.79769313486231570e308)) return DBMM_E_ARG;      // finite and positive
    if (!dbmm_aligned16(x) || !dbmm_aligned16(center) || !dbmm_aligned16(workspace) || ((takes & TAKES_V) && !dbmm_aligned16(v))) return DBMM_E_ALIGN;
    if (workspace_bytes < required) return DBMM_E_WORKSPACE;
    return DBMM_OK;
}

// The start of every pass; the operands have been checked.  The head of the workspace zeroed, absmax, split (LABELS: it records groups[row],
// the bucket kernel's labels), and the parameter fields both tile kernels have; amax: the head, the split's centred absmax
template <bool LABELS, class Params>
int prepare(Params& p, unsigned*& amax, const float* x, const int64_t* groups, const float* center, int64_t N, int64_t D, int64_t G, void* workspace,
            hipStream_t s) {
    const long long Dp = padded_dim(D);
    const Layout w = layout(N, D, 0);
    char* ws = (char*)workspace;
    amax = (unsigned*)ws;
    RowInfo* info = (RowInfo*)(ws + w.info);
    u16* P = (u16*)(ws + w.planes);
    hipError_t e = hipMemsetAsync(amax, 0, HEAD_BYTES, s);
    if (e != hipSuccess) return (int)e;
    const long long n4 = N * D / 4;
    const int g1 = (int)((n4 + 255) / 256 < 2048 ? (n4 + 255) / 256 : 2048);
    hipLaunchKernelGGL(pairdist_absmax_kernel, dim3(g1), dim3(256), 0, s, x, center, n4, (int)(D / 4), amax);
    DBMM_CHECK_LAUNCH();
    hipLaunchKernelGGL(pairdist_split_kernel<LABELS>, dim3((unsigned)((N + 3) / 4)), dim3(256), 0, s, x, center, groups, amax, P, info, (int)N, (int)D, (int)Dp,
                       (int)G);
    DBMM_CHECK_LAUNCH();
    p.P = P; p.info = info; p.part = (double*)(ws + w.part);
    p.ldp = 2 * Dp; p.p_total = (long long)N * 2 * Dp * 2;
    p.N = (int)N; p.T = (int)(Dp / 64); p.nb = (int)((N + 255) / 256);
    return DBMM_OK;
}

// prepare, tiles, fold for one element map; the operands have been checked.  gammas: RbfMap's L bandwidths (host), else null and L = 1
template <class Map>
int bucket_sums(const float* x, const int64_t* groups, const float* center, const double* gammas, int64_t L, double* sums, int64_t N, int64_t D, int64_t G,
                void* workspace, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    PairDistP p{};
    unsigned* amax;
    const int rc = prepare<true>(p, amax, x, groups, center, N, D, G, workspace, s);
    if (rc != DBMM_OK) return rc;
    p.amax_bits = amax; p.L = (int)L;
    for (int l = 0; gammas && l < L; ++l) p.gamma[l] = gammas[l];
    const long long nt = (long long)p.nb * (p.nb + 1) / 2;
    p.n_tiles = (int)nt;
    const int grid = nt < MAX_WG ? (int)nt : MAX_WG;
    hipLaunchKernelGGL(pairdist_tile_kernel<Map>, dim3(grid), dim3(512), 0, s, p);
    DBMM_CHECK_LAUNCH();
    hipLaunchKernelGGL(pairdist_fold_kernel, dim3((unsigned)L), dim3(64), 0, s, p.part, grid, Map::SCALED ? amax : (const unsigned*)nullptr, (int)G, sums);
    DBMM_CHECK_LAUNCH();
    return DBMM_OK;
}

}  // namespace

// see include/dbmm.h
extern "C" size_t dbmm_workspace_bytes_pairdist(int64_t N, int64_t D) {
    if (N <= 0 || D <= 0) return 0;
    return bucket_workspace_bytes(N, D, 1);
}

// see include/dbmm.h
extern "C" int dbmm_pairdist_group_sums(const float* x, const int64_t* groups, const float* center, double* sums, int64_t N, int64_t D,
                                        int64_t G, void* workspace, size_t workspace_bytes, void* stream) {
    const int rc = check_operands(TAKES_GROUPS, 8, x, groups, nullptr, center, nullptr, 1, sums, N, D, G, workspace, workspace_bytes,
                                  bucket_workspace_bytes(N, D, 1));
    return rc != DBMM_OK ? rc : bucket_sums<DistanceMap>(x, groups, center, nullptr, 1, sums, N, D, G, workspace, stream);
}

// see include/dbmm.h
extern "C" size_t dbmm_workspace_bytes_pairdist_rbf(int64_t N, int64_t D, int64_t L) {
    if (N <= 0 || D <= 0 || L < 1 || L > RBF_MAX_L) return 0;
    return bucket_workspace_bytes(N, D, L);
}

// see include/dbmm.h
extern "C" int dbmm_pairdist_rbf_group_sums(const float* x, const int64_t* groups, const float* center, const double* gammas, int64_t L, double* sums,
                                            int64_t N, int64_t D, int64_t G, void* workspace, size_t workspace_bytes, void* stream) {
    const int rc = check_operands(TAKES_GROUPS | TAKES_GAMMAS, 8, x, groups, nullptr, center, gammas, L, sums, N, D, G, workspace, workspace_bytes,
                                  bucket_workspace_bytes(N, D, L));
    return rc != DBMM_OK ? rc : bucket_sums<RbfMap>(x, groups, center, gammas, L, sums, N, D, G, workspace, stream);
}

// ---- per-row, per-group sums: R[i][g] = sum over j != i with group[j] == g of ||x_i - x_j||_2, float64 [N][G] (the silhouette's input) -------
// The same planes, ring and distance arithmetic; the epilogue reduces ALONG THE COLUMNS of a tile per row instead of into (group, group)
// buckets, so the kernel walks the full square of 256 x 256 blocks (the triangle's column sums would need an (other block) x N x G buffer to
// fold deterministically).  A work unit is one row block and a run of consecutive column blocks (a "column chunk", C of them per row block,
// chosen on the host); units are numbered chunk-major, so the workgroups of an XCD walk the same column blocks at about the same time.  A
// workgroup handles its unit's column blocks in order and keeps one float64 running sum per (row, group) IN PLACE in the unit's [256][G]
// block of part [C][N][G] (zeroed by a memset; thread t < 256 owns row t, nobody else touches the block): the ring leaves neither sixteen
// registers per thread nor 32 KB of LDS for them.  pairdist_rows_fold_kernel adds the C partials in chunk order and rescales.
// Order of a sum: a lane's two columns and the 32 fr lanes by a fixed fp32 tree (depth 6: 6 x 2^-24 relative, the terms are non-negative),
// then float64: the four column waves in wave order, the unit's tiles in walk order, the chunks in chunk order.  No floating-point atomics.
// A column takes its label from `groups` directly (RowInfo's NO_GROUP = 15 is a label here): labels outside [0, G) and columns >= N are in
// no sum.  The fast path is a tile off the diagonal whose 256 columns all carry one label; every other tile takes the predicated path, once
// per label present among its columns.
//
// Element maps, as for the bucket kernel: DistanceMap (the sums above) and RbfMap, R[l][i][g] = sum over j != i with group[j] == g of
// exp(-gamma_l ||x_i - x_j||^2) for L <= 4 bandwidths (dbmm_pairdist_rbf_row_group_sums: a Parzen-window probe, the MMD witness function, the
// row sums of a centred kernel alignment).  d^2 stays in the accumulators, the diagonal's is set to +inf (exp2(-inf) is an exact 0), and the
// reduction above runs once per l in a runtime loop: the partials are part [C][L][N][G], the owner thread's update runs once per (l, label
// present).  The predicated path forms the exponentials again for every label (the ring leaves no registers to keep L x 128 values), with
// the coefficient opaque per label so that they are not hoisted and d^2 is not spilled; neither instantiation uses scratch.
//
// A third map, RbfMatvecMap (dbmm_pairdist_rbf_matvec, include/dbmm_kernel_ops.h): the kernel matrix times C <= 16 dense columns,
// R[i][c] = sum over j != i of exp(-gamma ||x_i - x_j||^2) v[j][c], what conjugate gradients on (K + lambda I) alpha = T need.  No labels: the
// tile's weights (v fp32 [N][C], zero for a column past N) go to LDS, 16 KB beside the ring, and e_mask holds the weight columns with a
// non-zero weight in the tile -- the others are skipped, which adds nothing and changes no value (one-hot columns, frozen CG columns and
// the zero weights of appended query rows cost nothing).  ONE bandwidth: the kernel values are formed once, in place in the accumulators,
// and a weight column is w0 k0 + w1 k1 per lane, then the same tree, e_rsum, barrier and owner update as a label's sum, in a runtime loop:
// a column's sums are formed by the same instructions whatever C is.  part is [chunk][N][C]; no scratch, 157,700 bytes of LDS.
namespace {

constexpr int ROWS_MAX_G = 16;                                     // labels live in a byte; 16 = the k-means kernels' K
constexpr int ROWS_NO_GROUP = 255;                                 // columns past N / labels outside [0, G): in no sum
constexpr int ROWS_MAX_CHUNKS = 16;

struct PairRowsP {
    const u16* P; const RowInfo* info; const int64_t* groups; double* part;      // part [C][L][N][G]
    long long ldp, p_total;                                        // halves per row of P (2 Dp), bytes of P
    int N, T, nb, G, C, n_units;                                   // T = Dp / 64 K tiles per plane, nb = row blocks of 256, units = nb * C
};
struct PairRowsRbfP : PairRowsP {                                  // RbfMap's: the distance instantiation keeps its kernel arguments
    const unsigned* amax_bits; double gamma[RBF_MAX_L]; int L;     // as in PairDistP
};
struct PairRowsMatvecP : PairRowsRbfP {                            // RbfMatvecMap's: L = 1, groups is null, G counts the weight columns
    const float* v;                                                // the weights [N][G], row-major
};

// v[16 ii + r] (ii = 0 / 1, r < 16) of the 32 lanes with the same fh -> the sums over those lanes, one per lane: afterwards lane fr holds in
// v[0] the sum of value number fr.  Step s pairs lane fr with fr ^ (16 >> s); the lane whose bit is set keeps the upper half of what is left.
__device__ __forceinline__ void fold_fr_lanes(float (&v)[32], int fr) {
#pragma unroll
    for (int s = 0; s < 5; ++s) {
        const int h = 16 >> s;
        const bool up = (fr >> (4 - s)) & 1;
#pragma unroll
        for (int k = 0; k < h; ++k) {
            const float lo = v[k], hi = v[k + h];
            v[k] = (up ? hi : lo) + __shfl_xor(up ? lo : hi, 16 >> s, 64);
        }
    }
}

template <class Map>
__global__ __launch_bounds__(512, 1) void pairdist_rows_tile_kernel(const typename Map::RowsP p) {
    __shared__ __attribute__((aligned(1024))) unsigned char lds[8 * PH_HALF];      // [buffer 2][Ah0, Bh0, Bh1, Ah1] = 128 KB
    __shared__ float e_norm[512];                                  // epilogue: norms of the tile's 256 rows, then of its 256 columns
    __shared__ unsigned char e_grp[256];                           // labels of the tile's columns
    __shared__ unsigned e_mask;                                    // labels present among the columns; bit 16: a column in no group
    __shared__ float e_rsum[2][4][256];                            // [parity][column wave][row]: a wave's sums over its 64 columns
    // RbfMatvecMap: [weight column][tile column], 16 KB: 154.3 KB of LDS with the ring and the arrays above, under the CU's 160 KB.  The other
    // maps never name it and their instantiations do not allocate it (138.3 KB, as before)
    __shared__ float e_w[Map::WEIGHTED ? ROWS_MAX_G : 1][256];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wid = __builtin_amdgcn_readfirstlane(tid >> 6), wr = wid >> 2, wc = wid & 3;
    const int fr = lane & 31, fh = lane >> 5;
    const TileWalk walk = tile_walk(blockIdx.x, gridDim.x, p.n_units);
    const __amdgpu_buffer_rsrc_t rs0 = __builtin_amdgcn_make_buffer_rsrc((void*)p.P, 0, 0, 0x00020000);
    __amdgpu_buffer_rsrc_t rsA = rs0, rsW = rs0;
    int m0 = 0, n0 = 0;
    unsigned voff[4][2];                                           // the stager's lane offsets per half-tile kind (Ah0, Bh0, Bh1, Ah1); rows >= N masked
    auto set_tile = [&](int t, int bi, int bj) {
        m0 = bi * 256; n0 = bj * 256;
        rsA = desc(p.P, p.p_total, (long long)m0 * p.ldp * 2);
        rsW = desc(p.P, p.p_total, (long long)n0 * p.ldp * 2);
        PAIRDIST_LANE_OFFSETS(t);
    };
    // unit number k of this workgroup -> its row block, chunk and column blocks [lo, hi)
    auto unit = [&](int k, int& bi, int& c, int& lo, int& hi) {
        const int u = walk.first + k * walk.stride;
        c = u / p.nb; bi = u - c * p.nb;
        lo = (int)((long long)c * p.nb / p.C); hi = (int)((long long)(c + 1) * p.nb / p.C);
    };
#include "pairdist_ring.inc"

    const int wm0 = wr * 128, wn0 = wc * 64;
    int k = 0, bi = 0, ch = 0, bj = 0, hi = 0, par = 0;
    if (tid == 0) e_mask = 0u;
    if (walk.n_whole > 0) { unit(0, bi, ch, bj, hi); set_tile(tid, bi, bj); ring_prologue(0); }
    while (k < walk.n_whole) {
        ring_item(0, nT, true, [](int) {});                           // (every item waits for all of its prologue and the epilogue's stores)
        const int em0 = m0, en0 = n0, ech = ch;
        // everything per-lane below is recomputed from an opaque copy of tid: hoisted out of the item loop it would live across the ring's
        // phases, which leave two registers free, and be spilled
        int te = tid;
        asm volatile("" : "+v"(te));
        const int fr = te & 31, fh = (te >> 5) & 1;
        if (bj + 1 == hi) { if (++k < walk.n_whole) unit(k, bi, ch, bj, hi); } else ++bj;
        if (k < walk.n_whole) { set_tile(te, bi, bj); ring_prologue(0); }    // in flight during the epilogue

        // ---- epilogue: distances and per-row sums straight from the accumulators ------------------------------------------------
        // lane (fr, fh) holds columns wn0 + 2 fr + j (blocks j = 0 / 1: the B halves are the even / odd columns) of rows
        // wm0 + 32 i + (r & 3) + 8 (r >> 2) + 4 fh.
        {
            const int src = (te < 256 ? em0 : en0 - 256) + te;      // threads 0 .. 255: the tile's rows, 256 .. 511: its columns
            e_norm[te] = src < p.N ? p.info[src].norm : 0.f;
            if constexpr (Map::WEIGHTED) {
                // the tile's weights, zero for a column past N (its kernel value is some finite number); e_mask: the weight columns that
                // have a non-zero weight in this tile.  The others are skipped below, which adds nothing and so changes no value
                if (te >= 256) {
                    unsigned nz = 0u;
                    for (int c = 0; c < p.G; ++c) {
                        const float w = src < p.N ? p.v[(size_t)src * p.G + c] : 0.f;
                        e_w[c][te - 256] = w;
                        nz |= w != 0.f ? 1u << c : 0u;
                    }
                    if (nz) atomicOr(&e_mask, nz);                    // integer, order-free
                }
            } else if (te >= 256) {
                int g = ROWS_NO_GROUP;
                if (src < p.N) {
                    const int64_t gv = p.groups[src];
                    if (gv >= 0 && gv < p.G) g = (int)gv;
                }
                e_grp[te - 256] = (unsigned char)g;
                atomicOr(&e_mask, g == ROWS_NO_GROUP ? 0x10000u : 1u << g);        // integer, order-free
            }
        }
        __syncthreads();
        const unsigned mB = e_mask;
        const bool diag = em0 == en0;
        const bool fast = !diag && __builtin_popcount(mB) == 1 && mB < 0x10000u;
        const int c0 = wn0 + 2 * fr;
        PAIRDIST_ACC_TO_D2();
        if (diag) {                                                   // the pair (i, i) is in no sum: by index, whatever its value
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int lr = wm0 + 32 * i + (r & 3) + 8 * (r >> 2) + 4 * fh;
                    acc[i][0][r] = lr == c0 ? Map::self_pair() : acc[i][0][r];
                    acc[i][1][r] = lr == c0 + 1 ? Map::self_pair() : acc[i][1][r];
                }
        }
        const int gb0 = e_grp[c0], gb1 = e_grp[c0 + 1];
        // after the fold of row blocks 2 hh, 2 hh + 1 lane fr holds value fr: i = 2 hh + (fr >> 4), r = fr & 15
        const int out_row = wm0 + 32 * (fr >> 4) + (fr & 3) + 8 * ((fr & 15) >> 2) + 4 * fh;
        // this tile's running sums: thread t < 256 owns row em0 + t of the unit's block of part, for every label (in place: sixteen float64
        // sums per row held across the ring's phases do not fit its register budget, and [256][16] float64 does not fit beside the ring in LDS)
        const bool owner = te < 256 && em0 + te < p.N;
        auto fold_store = [&](float (&v)[32], int hh) {
            fold_fr_lanes(v, fr);
            e_rsum[par][wc][out_row + 64 * hh] = v[0];
        };
        // sum l of chunk ech is matrix ech * L + l of part (a one-sum map: the chunk's own number, as before there was an l)
        auto slot = [&](int l) {
            if constexpr (Map::MAX_L == 1) return (size_t)ech; else return (size_t)ech * Map::n_sums(p) + l;
        };
        auto add_label = [&](int l, int g) {                          // the four column waves in wave order, onto the running sum
            __syncthreads();
            if (owner)
                p.part[(slot(l) * p.N + em0 + te) * p.G + g] += (double)e_rsum[par][0][te] + (double)e_rsum[par][1][te] + (double)e_rsum[par][2][te] + (double)e_rsum[par][3][te];
            par ^= 1;                                                 // the next label's sums go to the other half: one barrier per label
        };
        // one reduction per sum l, the same whatever L is (a runtime loop, never unrolled: L bandwidths in one call equal L calls bit for bit);
        // the element values are formed from the accumulators on the way into the fold, so the tile is never held twice.  A do-while whose
        // condition is a constant for a one-sum map: written so, and with slot() above, DistanceMap's instantiation compiles to the listing the
        // kernel had before it was a template, instruction for instruction (a for loop, or this body in a lambda, did not: other registers)
        int l = 0;
#pragma unroll 1
        do {
            const float cf = Map::self_coef(Map::coef(p, l));
            if constexpr (Map::WEIGHTED) {
                // the kernel values once, in place (the diagonal's +inf gives an exact 0); a weight column then costs one multiply-add per
                // element and no second exponential.  One bandwidth: this body runs once
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        acc[i][0][r] = Map::val(acc[i][0][r], cf);
                        acc[i][1][r] = Map::val(acc[i][1][r], cf);
                    }
                // once per weight column with a non-zero weight in this tile: a runtime loop, never unrolled, so a column's sums are formed
                // by the same instructions whatever the other columns of the call are
#pragma unroll 1
                for (unsigned mb = mB & 0xffffu; mb; mb &= mb - 1) {
                    const int c = __builtin_ctz(mb);
                    const float w0 = e_w[c][c0], w1 = e_w[c][c0 + 1];
#pragma unroll
                    for (int hh = 0; hh < 2; ++hh) {
                        float v[32];
#pragma unroll
                        for (int ii = 0; ii < 2; ++ii)
#pragma unroll
                            for (int r = 0; r < 16; ++r) v[16 * ii + r] = fmaf(w1, acc[2 * hh + ii][1][r], w0 * acc[2 * hh + ii][0][r]);
                        fold_store(v, hh);
                    }
                    add_label(l, c);
                }
            } else if (fast) {                                        // one label, all 256 columns: no predicates
#pragma unroll
                for (int hh = 0; hh < 2; ++hh) {
                    float v[32];
#pragma unroll
                    for (int ii = 0; ii < 2; ++ii)
#pragma unroll
                        for (int r = 0; r < 16; ++r) v[16 * ii + r] = Map::val(acc[2 * hh + ii][0][r], cf) + Map::val(acc[2 * hh + ii][1][r], cf);
                    fold_store(v, hh);
                }
                add_label(l, __builtin_ctz(mB));
            } else {
                for (unsigned mb = mB & 0xffffu; mb; mb &= mb - 1) {  // once per label present among the columns
                    const int g = __builtin_ctz(mb);
                    const bool in0 = gb0 == g, in1 = gb1 == g;
                    const float cg = Map::per_group(cf);              // (RbfMap: the kernel values are formed again per label, not kept across)
#pragma unroll
                    for (int hh = 0; hh < 2; ++hh) {
                        float v[32];
#pragma unroll
                        for (int ii = 0; ii < 2; ++ii)
#pragma unroll
                            for (int r = 0; r < 16; ++r)
                                v[16 * ii + r] = (in0 ? Map::val(acc[2 * hh + ii][0][r], cg) : 0.f) + (in1 ? Map::val(acc[2 * hh + ii][1][r], cg) : 0.f);
                        fold_store(v, hh);
                    }
                    add_label(l, g);
                }
            }
        } while (Map::MAX_L > 1 && ++l < Map::n_sums(p));
        __syncthreads();
        if (tid == 0) e_mask = 0u;                                    // for the next tile: its atomics come after that tile's ring barriers
    }
}

// chunk partials -> R [L][N][G] (n_out = L N G values), in chunk order; amax_bits: distances were taken in units of 2^-s and are rescaled, null
// for kernel values, which have no unit
__global__ __launch_bounds__(256) void pairdist_rows_fold_kernel(const double* __restrict__ part, int C, long long n_out, const unsigned* __restrict__ amax_bits,
                                                                 double* __restrict__ R) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n_out) return;
    double s = 0.0;
    for (int c = 0; c < C; ++c) s += part[(size_t)c * n_out + i];
    R[i] = ldexp(s, amax_bits ? -scale_exp(__uint_as_float(*amax_bits)) : 0);
}

// Column chunks per row block: 1 .. min(16, nb), the count whose schedule is shortest -- rounds of the persistent grid times the tiles of the
// longest unit --, the smaller count on a tie.  Few row blocks want many chunks to fill the grid; many row blocks still gain when
// nb / MAX_WG is just above a whole number (636 row blocks: 3 rounds of 636 tiles with one chunk, 5 rounds of 318 with two).
inline int rows_chunks(long long nb) {
    long long best = 0;
    int C = 1;
    for (int c = 1; c <= ROWS_MAX_CHUNKS && c <= nb; ++c) {
        const long long units = nb * c, grid = units < MAX_WG ? units : MAX_WG;
        const long long cost = ((units + grid - 1) / grid) * ((nb + c - 1) / c);
        if (c == 1 || cost < best) { best = cost; C = c; }
    }
    return C;
}

// the partials of a rows pass with L sums per (row, label): sized for 16 chunks whatever rows_chunks picks: the size then grows with N
inline size_t rows_workspace_bytes(int64_t N, int64_t D, int64_t G, int64_t L) {
    return layout(N, D, (size_t)ROWS_MAX_CHUNKS * (size_t)L * (size_t)N * (size_t)G * sizeof(double)).total;
}

// prepare, tiles, fold for one element map; the operands have been checked.  gammas: RbfMap's L bandwidths (host), else null and L = 1;
// v: RbfMatvecMap's weights [N][G], with groups null and L = 1
template <class Map>
int row_sums(const float* x, const int64_t* groups, const float* center, const double* gammas, int64_t L, double* sums, int64_t N, int64_t D, int64_t G,
             void* workspace, void* stream, const float* v = nullptr) {
    hipStream_t s = (hipStream_t)stream;
    typename Map::RowsP p{};
    unsigned* amax;
    // (the split's own group column is not read here: the tile kernel takes the labels from `groups`)
    const int rc = prepare<!Map::WEIGHTED>(p, amax, x, groups, center, N, D, G, workspace, s);
    if (rc != DBMM_OK) return rc;
    p.groups = groups; p.G = (int)G;
    p.C = rows_chunks(p.nb);
    p.n_units = p.nb * p.C;
    if constexpr (!Map::SCALED) {
        p.amax_bits = amax; p.L = (int)L;
        for (int l = 0; l < L; ++l) p.gamma[l] = gammas[l];
    }
    if constexpr (Map::WEIGHTED) p.v = v;
    const long long n_out = L * N * G;
    hipError_t e = hipMemsetAsync(p.part, 0, (size_t)p.C * (size_t)n_out * sizeof(double), s);  // the units' running sums start at zero
    if (e != hipSuccess) return (int)e;
    const int grid = p.n_units < MAX_WG ? p.n_units : MAX_WG;
    hipLaunchKernelGGL(pairdist_rows_tile_kernel<Map>, dim3(grid), dim3(512), 0, s, p);
    DBMM_CHECK_LAUNCH();
    hipLaunchKernelGGL(pairdist_rows_fold_kernel, dim3((unsigned)((n_out + 255) / 256)), dim3(256), 0, s, p.part, p.C, n_out,
                       Map::SCALED ? amax : (const unsigned*)nullptr, sums);
    DBMM_CHECK_LAUNCH();
    return DBMM_OK;
}

}  // namespace

// see include/dbmm.h
extern "C" size_t dbmm_workspace_bytes_pairdist_rows(int64_t N, int64_t D, int64_t G) {
    if (N <= 0 || D <= 0 || G < 1 || G > ROWS_MAX_G) return 0;
    return rows_workspace_bytes(N, D, G, 1);
}

// see include/dbmm.h
extern "C" int dbmm_pairdist_row_group_sums(const float* x, const int64_t* groups, const float* center, double* sums, int64_t N, int64_t D,
                                            int64_t G, void* workspace, size_t workspace_bytes, void* stream) {
    const int rc = check_operands(TAKES_GROUPS, ROWS_MAX_G, x, groups, nullptr, center, nullptr, 1, sums, N, D, G, workspace, workspace_bytes,
                                  rows_workspace_bytes(N, D, G, 1));
    return rc != DBMM_OK ? rc : row_sums<DistanceMap>(x, groups, center, nullptr, 1, sums, N, D, G, workspace, stream);
}

// see include/dbmm.h
extern "C" size_t dbmm_workspace_bytes_pairdist_rbf_rows(int64_t N, int64_t D, int64_t G, int64_t L) {
    if (N <= 0 || D <= 0 || G < 1 || G > ROWS_MAX_G || L < 1 || L > RBF_MAX_L) return 0;
    return rows_workspace_bytes(N, D, G, L);
}

// see include/dbmm.h
extern "C" int dbmm_pairdist_rbf_row_group_sums(const float* x, const int64_t* groups, const float* center, const double* gammas, int64_t L, double* sums,
                                                int64_t N, int64_t D, int64_t G, void* workspace, size_t workspace_bytes, void* stream) {
    const int rc = check_operands(TAKES_GROUPS | TAKES_GAMMAS, ROWS_MAX_G, x, groups, nullptr, center, gammas, L, sums, N, D, G, workspace, workspace_bytes,
                                  rows_workspace_bytes(N, D, G, L));
    return rc != DBMM_OK ? rc : row_sums<RbfMap>(x, groups, center, gammas, L, sums, N, D, G, workspace, stream);
}

// see include/dbmm_kernel_ops.h
extern "C" size_t dbmm_workspace_bytes_pairdist_rbf_matvec(int64_t N, int64_t D, int64_t C) {
    if (N <= 0 || D <= 0 || C < 1 || C > ROWS_MAX_G) return 0;
    return rows_workspace_bytes(N, D, C, 1);
}

// see include/dbmm_kernel_ops.h
extern "C" int dbmm_pairdist_rbf_matvec(const float* x, const float* v, const float* center, double gamma, double* out, int64_t N, int64_t D, int64_t C,
                                        void* workspace, size_t workspace_bytes, void* stream) {
    const int rc = check_operands(TAKES_GAMMAS | TAKES_V, ROWS_MAX_G, x, nullptr, v, center, &gamma, 1, out, N, D, C, workspace, workspace_bytes,
                                  rows_workspace_bytes(N, D, C, 1));
    return rc != DBMM_OK ? rc : row_sums<RbfMatvecMap>(x, nullptr, center, &gamma, 1, out, N, D, C, workspace, stream, v);
}
