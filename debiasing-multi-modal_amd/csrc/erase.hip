// Linear concept erasure of fp32 rows (include/dbmm.h: dbmm_label_colsums / dbmm_erase_rows).
//
//   sums[g][d]  = sum over i with labels[i] == g of x[i][d],   double [G][D], and counts[g], int64 [G]: one read of x
//   y[i][d]     = x[i][d] - sum_k ((x[i] - c) . A[k]) B[k][d],  float [N][D], R = 1..15: one read and one write of x, y may be x
//
// Label sums: label_sums_kernel<KP> and label_merge_kernel are the unit body and the fixed-order merge of label_sums.h on int64 labels that
// nobody fitted, compared AS 64 BITS: a label outside [0, G) (-1, G, 2^32 + 1) is in no sum and no count.  The merge writes the RAW sums
// and the counts; the caller divides.
//
// Erasure: erase_rows_kernel<RP, PR, NCH>, one launch.  It starts from project_rows_kernel (covariance.hip): a wave per group of PR
// rows, float4 loads, one fp32 fmaf chain per (row, k) over the lane's columns in column order, a fixed butterfly.  The lane KEEPS
// its columns of the rows in registers (NCH float4 per row: NCH = chunks of 256 columns, padded to a power of two), so the update
// y = x - sum_k s_k B_k is formed from the registers: x is read once, and a row is read completely before any of it is written --
// y may alias x.  A and B (up to 30 x D floats) are read from the caches once per PR rows; PR is the largest of 4, 2, 1 at which
// the PR x NCH float4 of the rows fit a lane (PR NCH <= 16), so it depends on D alone and a row's arithmetic does not depend on
// its neighbours, on N or on where the row sits: erasing a slice gives the bits of the slice.  The R projections are padded to
// RP = 1 / 2 / 4 / 8 / 16 accumulators per row, as k-means pads K.
#include "label_sums.h"

namespace {

using namespace label_sums;

constexpr int RMAX = 15;

// workspace, in bytes: partial sums float64 [P][G][D] | partial counts int64 [P][16]
inline size_t ls_bytes(int64_t N, int64_t D, int64_t G) {
    int P, rows;
    ranges(N, D, P, rows);
    return part_bytes(P, G, D) + count_bytes(P);
}

// ---- per-label column sums, per (row range, column slab) ------------------------------------------------------------------------------------
template <int KP>
__global__ __launch_bounds__(256) void label_sums_kernel(const float* __restrict__ x, const long long* __restrict__ labels, double* __restrict__ part,
                                                         long long* __restrict__ cntp, int N, int D, int G, int P, int rows, int slabs) {
    const int unit = wave_unit();
    if (unit < P * slabs) unit_sums<KP, long long>(unit, x, labels, part, cntp, N, D, G, rows, slabs);
}

// ---- merge: the raw sums and the counts ---------------------------------------------------------------------------------------------------------
// grid (D / 64, G), 256 threads: a lane owns one entry of one label's sum, the four waves a quarter of the ranges each
__global__ __launch_bounds__(256) void label_merge_kernel(double* __restrict__ sums, long long* __restrict__ counts, const double* __restrict__ part,
                                                          const long long* __restrict__ cntp, int D, int G, int P) {
    __shared__ long long red[4];
    __shared__ double quarter[4][64];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, j = blockIdx.y, d = blockIdx.x * 64 + lane;
    quarter_sums(part + (size_t)j * D + (d < D ? d : 0), (size_t)G * D, P, quarter);
    if (w == 0 && d < D) sums[(size_t)j * D + d] = merge_sum(quarter, lane);
    if (blockIdx.x != 0) return;
    const long long n = merge_count(cntp, j, P, red);
    if (threadIdx.x == 0) counts[j] = n;
}

template <int KP>
void launch_label_sums(const float* x, const int64_t* labels, char* ws, int N, int D, int G, hipStream_t s) {
    int P, rows;
    ranges(N, D, P, rows);
    hipLaunchKernelGGL(label_sums_kernel<KP>, dim3(sums_grid(P, D)), dim3(256), 0, s, x, (const long long*)labels, (double*)ws,
                       (long long*)(ws + part_bytes(P, G, D)), N, D, G, P, rows, slabs(D));
}

// ---- erasure: y = x - sum_k ((x - c) . A_k) B_k -------------------------------------------------------------------------------------------------
// x and y carry no __restrict__: they may be the same rows
template <int RP, int PR, int NCH>
__global__ __launch_bounds__(256) void erase_rows_kernel(const float* x, const float* __restrict__ c, const float* __restrict__ A,
                                                         const float* __restrict__ B, float* y, int N, int D, int R) {
    const int lane = threadIdx.x & 63;
    const long long row0 = ((long long)blockIdx.x * 4 + (threadIdx.x >> 6)) * PR;
    if (row0 >= N) return;
    const int nr = (int)(N - row0 < PR ? N - row0 : PR);                         // wave-uniform
    f32x4 xv[PR][NCH];                                                           // the lane's columns of the rows, as loaded
    float acc[PR][RP];
#pragma unroll
    for (int r = 0; r < PR; ++r)
#pragma unroll
        for (int k = 0; k < RP; ++k) acc[r][k] = 0.f;
    // 1. the R projections of every row: one fmaf chain per (row, k) over the lane's columns in column order
#pragma unroll
    for (int ch = 0; ch < NCH; ++ch) {
        const int d = ch * SLAB_COLS + lane * 4;
        const bool active = d < D;                                               // (D % 64 == 0: a lane's float4 is inside or outside)
        const int ld = active ? d : 0;
        const f32x4 cc = *(const f32x4*)(c + ld);
        f32x4 df[PR];
#pragma unroll
        for (int r = 0; r < PR; ++r) {
            xv[r][ch] = *(const f32x4*)(x + (size_t)(row0 + min(r, nr - 1)) * D + ld);                             // past N: the last row again
            df[r] = active ? xv[r][ch] - cc : (f32x4){0.f, 0.f, 0.f, 0.f};       // a lane past the last column adds + 0 x a: no bit changes
        }
#pragma unroll
        for (int k = 0; k < RP; ++k) {
            if (k >= R) continue;
            const f32x4 av = *(const f32x4*)(A + (size_t)k * D + ld);
#pragma unroll
            for (int r = 0; r < PR; ++r)
#pragma unroll
                for (int e = 0; e < 4; ++e) acc[r][k] = fmaf(df[r][e], av[e], acc[r][k]);
        }
    }
#pragma unroll
    for (int r = 0; r < PR; ++r)
#pragma unroll
        for (int k = 0; k < RP; ++k)
            if (k < R) acc[r][k] = wave_sum(acc[r][k]);                          // a fixed butterfly: every lane gets the sum
    // 2. the update from the registers that still hold the rows: t = sum_k s_k B_k as one fmaf chain in k order, then y = x - t
#pragma unroll
    for (int ch = 0; ch < NCH; ++ch) {
        const int d = ch * SLAB_COLS + lane * 4;
        if (d >= D) continue;
        f32x4 t[PR];
#pragma unroll
        for (int r = 0; r < PR; ++r) t[r] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int k = 0; k < RP; ++k) {
            if (k >= R) continue;
            const f32x4 bv = *(const f32x4*)(B + (size_t)k * D + d);
#pragma unroll
            for (int r = 0; r < PR; ++r)
#pragma unroll
                for (int e = 0; e < 4; ++e) t[r][e] = fmaf(acc[r][k], bv[e], t[r][e]);
        }
#pragma unroll
        for (int r = 0; r < PR; ++r)
            if (r < nr) *(f32x4*)(y + (size_t)(row0 + r) * D + d) = xv[r][ch] - t[r];
    }
}

template <int RP, int PR, int NCH>
void launch_erase(const float* x, const float* c, const float* A, const float* B, float* y, int N, int D, int R, hipStream_t s) {
    const unsigned grid = (unsigned)(((long long)N + 4 * PR - 1) / (4 * PR));
    hipLaunchKernelGGL((erase_rows_kernel<RP, PR, NCH>), dim3(grid), dim3(256), 0, s, x, c, A, B, y, N, D, R);
}

// chunks of 256 columns padded to 1 / 2 / 4 / 8 / 16 and the rows per wave that go with them (PR NCH <= 16 float4 per lane)
template <int RP>
void dispatch_erase(const float* x, const float* c, const float* A, const float* B, float* y, int N, int D, int R, hipStream_t s) {
    const int chunks = (D + SLAB_COLS - 1) / SLAB_COLS;
    if (chunks <= 1) launch_erase<RP, 4, 1>(x, c, A, B, y, N, D, R, s);
    else if (chunks <= 2) launch_erase<RP, 4, 2>(x, c, A, B, y, N, D, R, s);
    else if (chunks <= 4) launch_erase<RP, 4, 4>(x, c, A, B, y, N, D, R, s);
    else if (chunks <= 8) launch_erase<RP, 2, 8>(x, c, A, B, y, N, D, R, s);
    else launch_erase<RP, 1, 16>(x, c, A, B, y, N, D, R, s);
}

}  // namespace

// see include/dbmm.h
extern "C" size_t dbmm_workspace_bytes_label_colsums(int64_t N, int64_t D, int64_t G) {
    if (dbmm_rows_shape(N, D) != DBMM_OK || G < 1 || G > MAX_LABELS) return 0;
    return ls_bytes(N, D, G);
}

// see include/dbmm.h
extern "C" int dbmm_label_colsums(const float* x, const int64_t* labels, double* sums, int64_t* counts, int64_t N, int64_t D, int64_t G,
                                  void* workspace, size_t workspace_bytes, void* stream) {
    const int rc = dbmm_rows_shape(N, D);
    if (rc != DBMM_OK) return rc;
    if (G < 1 || G > MAX_LABELS) return DBMM_E_SHAPE;
    if (!x || !labels || !sums || !counts || !workspace) return DBMM_E_ARG;
    if (workspace_bytes < ls_bytes(N, D, G)) return DBMM_E_WORKSPACE;
    if (!dbmm_aligned16(x) || !dbmm_aligned16(workspace) || (((uintptr_t)labels) & 7u) || (((uintptr_t)sums) & 7u) || (((uintptr_t)counts) & 7u))
        return DBMM_E_ALIGN;
    hipStream_t s = (hipStream_t)stream;
    char* ws = (char*)workspace;
    if (G <= 2) launch_label_sums<2>(x, labels, ws, (int)N, (int)D, (int)G, s);
    else if (G <= 4) launch_label_sums<4>(x, labels, ws, (int)N, (int)D, (int)G, s);
    else if (G <= 8) launch_label_sums<8>(x, labels, ws, (int)N, (int)D, (int)G, s);
    else launch_label_sums<16>(x, labels, ws, (int)N, (int)D, (int)G, s);
    DBMM_CHECK_LAUNCH();
    int P, rows;
    ranges(N, D, P, rows);
    hipLaunchKernelGGL(label_merge_kernel, dim3((unsigned)(D / 64), (unsigned)G), dim3(256), 0, s, sums, (long long*)counts, (const double*)ws,
                       (const long long*)(ws + part_bytes(P, G, D)), (int)D, (int)G, P);
    DBMM_CHECK_LAUNCH();
    return DBMM_OK;
}

// see include/dbmm.h
extern "C" int dbmm_erase_rows(const float* x, const float* center, const float* A, const float* B, float* y, int64_t N, int64_t D, int64_t R,
                               void* stream) {
    const int rc = dbmm_rows_shape(N, D);
    if (rc != DBMM_OK) return rc;
    if (R < 1 || R > RMAX) return DBMM_E_SHAPE;
    if (!x || !center || !A || !B || !y) return DBMM_E_ARG;
    if (!dbmm_aligned16(x) || !dbmm_aligned16(center) || !dbmm_aligned16(A) || !dbmm_aligned16(B) || !dbmm_aligned16(y)) return DBMM_E_ALIGN;
    hipStream_t s = (hipStream_t)stream;
    if (R <= 1) dispatch_erase<1>(x, center, A, B, y, (int)N, (int)D, (int)R, s);
    else if (R <= 2) dispatch_erase<2>(x, center, A, B, y, (int)N, (int)D, (int)R, s);
    else if (R <= 4) dispatch_erase<4>(x, center, A, B, y, (int)N, (int)D, (int)R, s);
    else if (R <= 8) dispatch_erase<8>(x, center, A, B, y, (int)N, (int)D, (int)R, s);
    else dispatch_erase<16>(x, center, A, B, y, (int)N, (int)D, (int)R, s);
    DBMM_CHECK_LAUNCH();
    return DBMM_OK;
}
