// Lloyd's k-means on fp32 rows, K <= 16 centres (include/dbmm.h: dbmm_kmeans_begin / dbmm_kmeans_iterate / dbmm_kmeans_assign;
// DESIGN.md section 6c).  A streaming problem: x is read twice per iteration, nothing N x D or N x K is stored.
//
// One iteration is three launches on the given stream:
//   kmeans_assign_kernel<KP>  one read of x: a wave takes four rows at a time (float4 loads), the centres fp32 [K][D] are read once per
//                             four rows.  d2_ij = sum_d (x_id - c_jd)^2 FROM THE DIFFERENCES, one fmaf chain per (row, centre) over the
//                             lane's columns in column order and a fixed butterfly: CLIP rows sit far from zero and close to each
//                             other, and the differences have no cancellation to manage (the |x|^2 + |c|^2 - 2 x.c form does).  A row's
//                             result depends on that row and the centres only.  Writes label[i] (lowest index on an exact tie) and
//                             dmin[i], and counts the rows whose label changed: one integer atomic per workgroup of 64 rows.
//   kmeans_sums_kernel<KP>    per-cluster column sums IN FLOAT64 FROM THE FIRST ADD, per (one of P row ranges, slab of 256 columns): the unit
//                             body of label_sums.h on the int labels of the assignment.  The first slab's wave also writes the range's
//                             float64 sum of dmin (lane-strided, a fixed butterfly).  The very first wave latches the changed-label
//                             counter for the merge and resets it with plain stores.
//   kmeans_merge_kernel       adds the P partials in label_sums.h's fixed order, c_j <- fp32(sum_j / n_j) in float64, unless the latched
//                             counter is 0: then no label moved, the state becomes `converged` and the centres stay the ones the labels,
//                             dmin and the inertia were computed against.  A cluster with no rows keeps its centre and reports count 0.
//                             One workgroup writes the status: iterations, changed rows, inertia (a fixed order too), counts.
// P depends on (N, D) only (label_sums::ranges), so two runs add the same numbers in the same order: no floating-point atomics, no memset.
//
// The state word lives in the workspace: every kernel reads it first and returns at once unless it is `running`, so iterations enqueued
// after convergence are no-ops and the result does not depend on how the host cuts the iterations into calls.  Inside one launch nobody
// reads a word that another workgroup of that launch writes, except the state itself in the merge, which only ever moves to
// `converged` there -- when no workgroup of the merge has anything left to write.  That is why the counter is latched by the sums
// kernel: a merge workgroup that reset it could be overtaken by one that has yet to read it.
#include "label_sums.h"

namespace {

using namespace label_sums;

constexpr int PR = 4;                      // rows per wave step of the assignment
constexpr int WG_STEPS = 4;                // steps per wave: a workgroup assigns 4 waves x 4 steps x 4 rows
constexpr int WG_ROWS = 4 * WG_STEPS * PR;

// status block, 8-byte words at offset 0 of the workspace (include/dbmm.h documents it: Python reads it)
constexpr int ST_ITER = 0, ST_STATE = 1, ST_CHANGED = 2, ST_INERTIA = 3, ST_COUNTS = 4, ST_COUNTER = 20, ST_LATCH = 21;
constexpr int ST_WORDS = 32;
constexpr long long RUNNING = 0, CONVERGED = 1;

inline size_t pad16(size_t b) { return (b + 15) & ~(size_t)15; }
// workspace, in bytes: status | centres fp32 [K][D] | labels int32 [N] | dmin fp32 [N] | partial sums float64 [P][K][D] |
// partial counts int64 [P][16] | partial inertia float64 [P]; every part starts 16-byte aligned
struct Layout {
    size_t c, lab, dmin, part, cnt, inert, total;
    int P, rows;
};
inline Layout layout(int64_t N, int64_t D, int64_t K) {
    Layout l;
    ranges(N, D, l.P, l.rows);
    l.c = ST_WORDS * 8;
    l.lab = l.c + (size_t)K * D * 4;
    l.dmin = l.lab + pad16((size_t)N * 4);
    l.part = l.dmin + pad16((size_t)N * 4);
    l.cnt = l.part + part_bytes(l.P, K, D);
    l.inert = l.cnt + count_bytes(l.P);
    l.total = l.inert + pad16((size_t)l.P * 8);
    return l;
}

// ---- begin: the start centres, labels = -1 (every row changes in the first assignment), a cleared status ----------------------------
__global__ __launch_bounds__(256) void kmeans_begin_kernel(const float* __restrict__ c0, float* __restrict__ c, int* __restrict__ labels,
                                                           float* __restrict__ dmin, long long* __restrict__ st, int N, int KD) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i < ST_WORDS) st[i] = 0;                                                 // (the inertia word: +0.0)
    if (i < KD) c[i] = c0[i];
    if (i < N) {
        labels[i] = -1;
        dmin[i] = 0.f;
    }
}

// ---- assignment: labels and squared distances of 64 rows per workgroup ------------------------------------------------------------------
// st == nullptr: the stand-alone assignment (dbmm_kmeans_assign): no state, nothing counted
template <int KP>
__global__ __launch_bounds__(256) void kmeans_assign_kernel(const float* __restrict__ x, const float* __restrict__ c, int* __restrict__ labels,
                                                            float* __restrict__ dmin, long long* __restrict__ st, int N, int D, int K) {
    if (st && st[ST_STATE] != RUNNING) return;
    __shared__ int ch[4];
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    int changed = 0;                                                             // lane 0 counts for its wave
    for (int g = 0; g < WG_STEPS; ++g) {
        const long long row0 = (long long)blockIdx.x * WG_ROWS + (wid * WG_STEPS + g) * PR;
        if (row0 >= N) break;                                                    // wave-uniform
        const int nr = (int)(N - row0 < PR ? N - row0 : PR);
        float acc[PR][KP];
#pragma unroll
        for (int r = 0; r < PR; ++r)
#pragma unroll
            for (int j = 0; j < KP; ++j) acc[r][j] = 0.f;
        for (int d = lane * 4; d < D; d += 256) {
            f32x4 xv[PR];
#pragma unroll
            for (int r = 0; r < PR; ++r) xv[r] = *(const f32x4*)(x + (size_t)(row0 + min(r, nr - 1)) * D + d);     // past N: the last row again
#pragma unroll
            for (int j = 0; j < KP; ++j) {
                if (j >= K) continue;
                const f32x4 cv = *(const f32x4*)(c + (size_t)j * D + d);
#pragma unroll
                for (int r = 0; r < PR; ++r) {
                    const f32x4 df = xv[r] - cv;
#pragma unroll
                    for (int e = 0; e < 4; ++e) acc[r][j] = fmaf(df[e], df[e], acc[r][j]);
                }
            }
        }
#pragma unroll
        for (int r = 0; r < PR; ++r) {
            float best = wave_sum(acc[r][0]);
            int bj = 0;
#pragma unroll
            for (int j = 1; j < KP; ++j) {
                if (j >= K) continue;
                const float s = wave_sum(acc[r][j]);
                if (s < best) { best = s; bj = j; }                              // strict: the lowest index wins an exact tie
            }
            if (lane == 0 && r < nr) {
                if (st) changed += labels[row0 + r] != bj ? 1 : 0;
                labels[row0 + r] = bj;
                dmin[row0 + r] = best;
            }
        }
    }
    if (!st) return;
    if (lane == 0) ch[wid] = changed;
    __syncthreads();
    if (threadIdx.x == 0) {
        const int n = ch[0] + ch[1] + ch[2] + ch[3];
        if (n) atomicAdd((unsigned long long*)(st + ST_COUNTER), (unsigned long long)n);   // an integer count: its order does not matter
    }
}

// ---- per-cluster column sums, per (row range, column slab) ----------------------------------------------------------------------------------
template <int KP>
__global__ __launch_bounds__(256) void kmeans_sums_kernel(const float* __restrict__ x, const int* __restrict__ labels, const float* __restrict__ dmin,
                                                          double* __restrict__ part, long long* __restrict__ cntp, double* __restrict__ inert,
                                                          long long* __restrict__ st, int N, int D, int K, int P, int rows, int slabs) {
    if (st[ST_STATE] != RUNNING) return;
    const int lane = threadIdx.x & 63, unit = wave_unit();
    if (unit == 0 && lane == 0) {                                                // this iteration's assignment is complete: latch its count
        st[ST_LATCH] = st[ST_COUNTER];
        st[ST_COUNTER] = 0;
    }
    if (unit >= P * slabs) return;
    const Unit u = unit_sums<KP, int>(unit, x, labels, part, cntp, N, D, K, rows, slabs);
    if (u.s != 0) return;
    // the first column slab: the range's sum of dmin
    double a = 0.0;
    for (int i = u.r0 + lane; i < u.r1; i += 64) a += (double)dmin[i];
    a = wave_sum_f64(a);
    if (lane == 0) inert[u.p] = a;
}

// ---- merge: new centres, the status ------------------------------------------------------------------------------------------------------------
// grid (ceil(D / 64), K), 256 threads: a lane owns one entry of one centre, the four waves a quarter of the ranges each
__global__ __launch_bounds__(256) void kmeans_merge_kernel(float* __restrict__ c, const double* __restrict__ part, const long long* __restrict__ cntp,
                                                           const double* __restrict__ inert, long long* __restrict__ st, int D, int K, int P) {
    if (st[ST_STATE] != RUNNING) return;
    __shared__ long long red[4];
    __shared__ double quarter[4][64];
    const long long changed = st[ST_LATCH];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, j = blockIdx.y, d = blockIdx.x * 64 + lane;
    if (changed != 0) {
        const long long n = merge_count(cntp, j, P, red);
        quarter_sums(part + (size_t)j * D + (d < D ? d : 0), (size_t)K * D, P, quarter);
        if (w == 0 && n > 0 && d < D) c[(size_t)j * D + d] = (float)(merge_sum(quarter, lane) / (double)n);
    }
    if (blockIdx.x != 0 || j != 0) return;
    for (int k = 0; k < K; ++k) {
        const long long n = merge_count(cntp, k, P, red);
        if (threadIdx.x == 0) st[ST_COUNTS + k] = n;
    }
    if (w != 0) return;
    // the inertia: every lane a contiguous run of the ranges in range order, then a fixed butterfly
    const int run = (P + 63) / 64;
    double total = 0.0;
    for (int p = lane * run; p < min((lane + 1) * run, P); ++p) total += inert[p];
    total = wave_sum_f64(total);
    if (lane == 0) {
        st[ST_INERTIA] = __double_as_longlong(total);
        st[ST_CHANGED] = changed;
        st[ST_ITER] += 1;
        if (changed == 0) st[ST_STATE] = CONVERGED;
    }
}

inline int km_shape(int64_t N, int64_t D, int64_t K) {
    if (K < 1 || N < K || D <= 0 || (D & 3)) return DBMM_E_SHAPE;
    if (K > MAX_LABELS || D > 4096 || N > 0x7fffffffLL) return DBMM_E_UNSUPPORTED;
    return DBMM_OK;
}

template <int KP>
void launch_assign(const float* x, const float* c, int* labels, float* dmin, long long* st, int N, int D, int K, hipStream_t s) {
    hipLaunchKernelGGL(kmeans_assign_kernel<KP>, dim3((unsigned)(((long long)N + WG_ROWS - 1) / WG_ROWS)), dim3(256), 0, s, x, c, labels, dmin, st, N, D, K);
}
template <int KP>
void launch_sums(const float* x, char* ws, const Layout& l, int N, int D, int K, hipStream_t s) {
    hipLaunchKernelGGL(kmeans_sums_kernel<KP>, dim3(sums_grid(l.P, D)), dim3(256), 0, s, x, (const int*)(ws + l.lab),
                       (const float*)(ws + l.dmin), (double*)(ws + l.part), (long long*)(ws + l.cnt), (double*)(ws + l.inert), (long long*)ws, N, D,
                       K, l.P, l.rows, slabs(D));
}

// K padded to 2 / 4 / 8 / 16: the kernels' register arrays
#define KM_DISPATCH(K, CALL)              \
    do {                                  \
        if ((K) <= 2) { CALL(2); }        \
        else if ((K) <= 4) { CALL(4); }   \
        else if ((K) <= 8) { CALL(8); }   \
        else { CALL(16); }                \
    } while (0)

}  // namespace

// see include/dbmm.h
extern "C" size_t dbmm_workspace_bytes_kmeans(int64_t N, int64_t D, int64_t K) {
    if (km_shape(N, D, K) != DBMM_OK) return 0;
    return layout(N, D, K).total;
}

// see include/dbmm.h
extern "C" int dbmm_kmeans_begin(const float* centers0, int64_t N, int64_t D, int64_t K, void* workspace, size_t workspace_bytes, void* stream) {
    const int rc = km_shape(N, D, K);
    if (rc != DBMM_OK) return rc;
    if (!centers0 || !workspace) return DBMM_E_ARG;
    if (workspace_bytes < dbmm_workspace_bytes_kmeans(N, D, K)) return DBMM_E_WORKSPACE;
    if (!dbmm_aligned16(centers0) || !dbmm_aligned16(workspace)) return DBMM_E_ALIGN;
    const Layout l = layout(N, D, K);
    char* ws = (char*)workspace;
    const long long n = N > K * D ? N : K * D;
    hipLaunchKernelGGL(kmeans_begin_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, centers0, (float*)(ws + l.c),
                       (int*)(ws + l.lab), (float*)(ws + l.dmin), (long long*)ws, (int)N, (int)(K * D));
    DBMM_CHECK_LAUNCH();
    return DBMM_OK;
}

// see include/dbmm.h
extern "C" int dbmm_kmeans_iterate(const float* x, int64_t N, int64_t D, int64_t K, int64_t n_iter, void* workspace, size_t workspace_bytes,
                                   void* stream) {
    const int rc = km_shape(N, D, K);
    if (rc != DBMM_OK) return rc;
    if (n_iter < 0) return DBMM_E_SHAPE;
    if (!x || !workspace) return DBMM_E_ARG;
    if (workspace_bytes < dbmm_workspace_bytes_kmeans(N, D, K)) return DBMM_E_WORKSPACE;
    if (!dbmm_aligned16(x) || !dbmm_aligned16(workspace)) return DBMM_E_ALIGN;
    const Layout l = layout(N, D, K);
    char* ws = (char*)workspace;
    hipStream_t s = (hipStream_t)stream;
    for (int64_t it = 0; it < n_iter; ++it) {
#define KM_ASSIGN(KP) launch_assign<KP>(x, (const float*)(ws + l.c), (int*)(ws + l.lab), (float*)(ws + l.dmin), (long long*)ws, (int)N, (int)D, (int)K, s)
        KM_DISPATCH(K, KM_ASSIGN);
#undef KM_ASSIGN
        DBMM_CHECK_LAUNCH();
#define KM_SUMS(KP) launch_sums<KP>(x, ws, l, (int)N, (int)D, (int)K, s)
        KM_DISPATCH(K, KM_SUMS);
#undef KM_SUMS
        DBMM_CHECK_LAUNCH();
        hipLaunchKernelGGL(kmeans_merge_kernel, dim3((unsigned)((D + 63) / 64), (unsigned)K), dim3(256), 0, s, (float*)(ws + l.c),
                           (const double*)(ws + l.part), (const long long*)(ws + l.cnt), (const double*)(ws + l.inert), (long long*)ws, (int)D,
                           (int)K, l.P);
        DBMM_CHECK_LAUNCH();
    }
    return DBMM_OK;
}

// see include/dbmm.h
extern "C" int dbmm_kmeans_assign(const float* x, const float* centers, int32_t* labels, float* dmin, int64_t N, int64_t D, int64_t K, void* stream) {
    // (rows are placed at fitted centres: any N >= 1, also below K)
    const int rc = km_shape(N < K ? K : N, D, K);
    if (rc != DBMM_OK) return rc;
    if (N < 1) return DBMM_E_SHAPE;
    if (!x || !centers || !labels || !dmin) return DBMM_E_ARG;
    if (!dbmm_aligned16(x) || !dbmm_aligned16(centers) || (((uintptr_t)labels) & 3u) || (((uintptr_t)dmin) & 3u)) return DBMM_E_ALIGN;
    hipStream_t s = (hipStream_t)stream;
#define KM_ASSIGN(KP) launch_assign<KP>(x, centers, labels, dmin, nullptr, (int)N, (int)D, (int)K, s)
    KM_DISPATCH(K, KM_ASSIGN);
#undef KM_ASSIGN
    DBMM_CHECK_LAUNCH();
    return DBMM_OK;
}
