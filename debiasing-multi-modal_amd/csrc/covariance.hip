// PCA of an embedding split (include/dbmm.h: dbmm_covariance / dbmm_project_rows).
//
//   scatter[a][b] = sum_i (x[i][a] - c[a]) (x[i][b] - c[b]),  double [D][D], about the GIVEN centre c (any vector near the mean)
//   y[i][k]       = (x[i] - c) . basis[k],                      float [N][K], K <= 8
//
// Covariance, two launches, no memset, no floating-point atomics:
//   covariance_tile_kernel   a workgroup owns one unit = (64 x 64 tile of the UPPER TRIANGLE of the scatter matrix, row range p of P).
//                            The rows are centred on load and go through LDS 32 at a time; the products are exact fp32
//                            (v_mfma_f32_32x32x2_f32: a row-ordered fmaf chain, four waves, one 32 x 32 block each).  NO fp32 CHAIN IS
//                            LONGER THAN 1024 ROWS: after every slab of 1024 rows the 16 fp32 accumulators of a lane are added to 16
//                            float64 running sums (32 VGPRs) and cleared.  The unit's float64 tile goes to the workspace in the
//                            accumulator layout (coalesced).
//   covariance_merge_kernel  one workgroup per tile adds the P partial tiles in range order and writes the tile and its mirror image:
//                            scatter is symmetric to the bit (a diagonal tile is written from its upper half).  On a diagonal tile the
//                            wave of the block below the diagonal issues no MFMA: nobody reads that block.
// P depends on (N, D) only (cov_ranges), never on the device, so two calls -- on any gfx950 -- add the same numbers in the same order.
//
// Projection: project_rows_kernel, one wave per group of four rows: float4 loads, one fp32 fmaf chain per (row, component) over the
// lane's columns in column order, a fixed butterfly; all K outputs from one read of the row, the basis read once per four rows.
#include "common.h"

namespace {

constexpr int CT = 64;                     // columns of a scatter tile (both ways)
constexpr int KC = 32;                     // rows staged in LDS at a time
constexpr int SLAB = 1024;                 // rows per fp32 accumulation chain, at most
constexpr int UNITS = 3 * DBMM_N_CU;       // units aimed at: 2 - 4 workgroups per CU
constexpr int MIN_RANGE = 2 * SLAB;        // a row range is not cut below two slabs
constexpr int PR = 4;                      // rows per wave of the projection

inline long long cov_tiles(long long D) { const long long nt = D / CT; return nt * (nt + 1) / 2; }
// row ranges P and rows per range, from (N, D) alone
inline void cov_ranges(long long N, long long D, int& P, int& rows) {
    const long long T = cov_tiles(D);
    long long p = (UNITS + T - 1) / T, cap = (N + MIN_RANGE - 1) / MIN_RANGE;
    p = p < cap ? p : cap;
    p = p < 1 ? 1 : p;
    P = (int)p;
    rows = (int)((N + p - 1) / p);
}
constexpr size_t TILE_BYTES = (size_t)CT * CT * sizeof(double);

__global__ __launch_bounds__(256) void covariance_tile_kernel(const float* __restrict__ x, const float* __restrict__ c, double* __restrict__ part,
                                                              int N, int D, int T, int rows) {
    __shared__ float as[KC * CT], bs[KC * CT];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, wr = wid >> 1, wc = wid & 1;
    // tile number -> (ta <= tb), row-major over the upper triangle
    int ta = 0, rem = blockIdx.x;
    const int nt = D / CT;
    while (rem >= nt - ta) { rem -= nt - ta; ++ta; }
    const int a0 = ta * CT, b0 = (ta + rem) * CT;
    const bool diag = rem == 0;
    const int r0 = min((long long)blockIdx.y * rows, (long long)N), r1 = min((long long)r0 + rows, (long long)N);
    // loader: thread -> row (tid >> 4) + 16 h of the chunk, columns 4 (tid & 15) .. + 3 of both panels
    const int lr = tid >> 4, lc = (tid & 15) * 4;
    const f32x4 ca = *(const f32x4*)(c + a0 + lc), cb = *(const f32x4*)(c + b0 + lc);
    f32x4 ra[2], rb[2];
    auto fetch = [&](int k0) {
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int row = k0 + lr + 16 * h;
            ra[h] = (f32x4){0.f, 0.f, 0.f, 0.f}; rb[h] = ra[h];           // a row past the range adds nothing: zero AFTER centring
            if (row < r1) {
                const float* xr = x + (size_t)row * D;
                ra[h] = *(const f32x4*)(xr + a0 + lc) - ca;
                if (!diag) rb[h] = *(const f32x4*)(xr + b0 + lc) - cb;
            }
        }
    };
    f32x16 acc;
    double sum[16];
#pragma unroll
    for (int v = 0; v < 16; ++v) { acc[v] = 0.f; sum[v] = 0.0; }
    // operands of the 32x32x2 product: A[i = lane & 31][k = lane >> 5], B[k = lane >> 5][j = lane & 31]; k is the row of x
    const float* bp = diag ? as : bs;
    const bool active = !(diag && wr > wc);                               // the block below the diagonal of a diagonal tile is the mirror's
    const int ao = (lane >> 5) * CT + wr * 32 + (lane & 31), bo = (lane >> 5) * CT + wc * 32 + (lane & 31);
    int chunks = 0;
    if (r0 < r1) fetch(r0);
    for (int k0 = r0; k0 < r1; k0 += KC) {
        __syncthreads();                                                   // the previous chunk has been read
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            *(f32x4*)(as + (lr + 16 * h) * CT + lc) = ra[h];
            if (!diag) *(f32x4*)(bs + (lr + 16 * h) * CT + lc) = rb[h];
        }
        __syncthreads();
        if (k0 + KC < r1) fetch(k0 + KC);                                  // the next chunk's loads fly over this chunk's MFMAs
        if (active) {                                                      // an idle wave still loads, stores and waits at the barriers
#pragma unroll
            for (int kk = 0; kk < KC / 2; ++kk)
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(as[ao + 2 * kk * CT], bp[bo + 2 * kk * CT], acc, 0, 0, 0);
        }
        if (++chunks == SLAB / KC) {                                       // a slab is done: fold the fp32 chain into float64
#pragma unroll
            for (int v = 0; v < 16; ++v) { sum[v] += (double)acc[v]; acc[v] = 0.f; }
            chunks = 0;
        }
    }
#pragma unroll
    for (int v = 0; v < 16; ++v) sum[v] += (double)acc[v];
    // unit (range, tile): [wave][register][lane]
    double* out = part + ((size_t)blockIdx.y * T + blockIdx.x) * (CT * CT) + (size_t)wid * 16 * 64 + lane;
#pragma unroll
    for (int v = 0; v < 16; ++v) out[v * 64] = sum[v];
}

__global__ __launch_bounds__(256) void covariance_merge_kernel(const double* __restrict__ part, double* __restrict__ scatter, int D, int T, int P) {
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, wr = wid >> 1, wc = wid & 1;
    int ta = 0, rem = blockIdx.x;
    const int nt = D / CT;
    while (rem >= nt - ta) { rem -= nt - ta; ++ta; }
    const int a0 = ta * CT, b0 = (ta + rem) * CT;
    const bool diag = rem == 0;
    const double* in = part + (size_t)blockIdx.x * (CT * CT) + (size_t)wid * 16 * 64 + lane;
#pragma unroll
    for (int v = 0; v < 16; ++v) {
        double s = 0.0;
        for (int p = 0; p < P; ++p) s += in[(size_t)p * T * (CT * CT) + v * 64];       // range order
        // accumulator layout: row (v & 3) + 8 (v >> 2) + 4 (lane >> 5), column lane & 31 of the wave's 32 x 32 block
        const int i = wr * 32 + (v & 3) + 8 * (v >> 2) + 4 * (lane >> 5), j = wc * 32 + (lane & 31);
        if (diag && i > j) continue;
        scatter[(size_t)(a0 + i) * D + b0 + j] = s;
        scatter[(size_t)(b0 + j) * D + a0 + i] = s;
    }
}

template <int K>
__global__ __launch_bounds__(256) void project_rows_kernel(const float* __restrict__ x, const float* __restrict__ c, const float* __restrict__ basis,
                                                           float* __restrict__ y, int N, int D) {
    const int lane = threadIdx.x & 63;
    const long long row0 = ((long long)blockIdx.x * 4 + (threadIdx.x >> 6)) * PR;
    if (row0 >= N) return;
    const int nr = (int)(N - row0 < PR ? N - row0 : PR);                  // wave-uniform
    float acc[PR][K];
#pragma unroll
    for (int r = 0; r < PR; ++r)
#pragma unroll
        for (int k = 0; k < K; ++k) acc[r][k] = 0.f;
    for (int d = lane * 4; d < D; d += 256) {
        const f32x4 cc = *(const f32x4*)(c + d);
        f32x4 xv[PR];
#pragma unroll
        for (int r = 0; r < PR; ++r) xv[r] = r < nr ? *(const f32x4*)(x + (size_t)(row0 + r) * D + d) - cc : (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const f32x4 bv = *(const f32x4*)(basis + (size_t)k * D + d);
#pragma unroll
            for (int r = 0; r < PR; ++r)
#pragma unroll
                for (int e = 0; e < 4; ++e) acc[r][k] = fmaf(xv[r][e], bv[e], acc[r][k]);
        }
    }
#pragma unroll
    for (int r = 0; r < PR; ++r)
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const float s = wave_sum(acc[r][k]);
            if (lane == 0 && r < nr) y[(size_t)(row0 + r) * K + k] = s;
        }
}

template <int K>
void launch_project(const float* x, const float* c, const float* basis, float* y, int N, int D, hipStream_t s) {
    const unsigned grid = (unsigned)((N + 4 * PR - 1) / (4 * PR));
    hipLaunchKernelGGL(project_rows_kernel<K>, dim3(grid), dim3(256), 0, s, x, c, basis, y, N, D);
}

}  // namespace

// see include/dbmm.h
extern "C" size_t dbmm_workspace_bytes_covariance(int64_t N, int64_t D) {
    if (dbmm_rows_shape(N, D) != DBMM_OK) return 0;
    int P, rows;
    cov_ranges(N, D, P, rows);
    return (size_t)P * (size_t)cov_tiles(D) * TILE_BYTES;
}

// see include/dbmm.h
extern "C" int dbmm_covariance(const float* x, const float* center, double* scatter, int64_t N, int64_t D, void* workspace, size_t workspace_bytes,
                               void* stream) {
    const int rc = dbmm_rows_shape(N, D);
    if (rc != DBMM_OK) return rc;
    if (!x || !center || !scatter || !workspace) return DBMM_E_ARG;
    if (workspace_bytes < dbmm_workspace_bytes_covariance(N, D)) return DBMM_E_WORKSPACE;
    if (!dbmm_aligned16(x) || !dbmm_aligned16(center) || !dbmm_aligned16(workspace) || (((uintptr_t)scatter) & 7u)) return DBMM_E_ALIGN;
    int P, rows;
    cov_ranges(N, D, P, rows);
    const int T = (int)cov_tiles(D);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(covariance_tile_kernel, dim3(T, P), dim3(256), 0, s, x, center, (double*)workspace, (int)N, (int)D, T, rows);
    DBMM_CHECK_LAUNCH();
    hipLaunchKernelGGL(covariance_merge_kernel, dim3(T), dim3(256), 0, s, (const double*)workspace, scatter, (int)D, T, P);
    DBMM_CHECK_LAUNCH();
    return DBMM_OK;
}

// see include/dbmm.h
extern "C" int dbmm_project_rows(const float* x, const float* center, const float* basis, float* y, int64_t N, int64_t D, int64_t K, void* stream) {
    const int rc = dbmm_rows_shape(N, D);
    if (rc != DBMM_OK) return rc;
    if (K < 1 || K > 8) return DBMM_E_SHAPE;
    if (!x || !center || !basis || !y) return DBMM_E_ARG;
    if (!dbmm_aligned16(x) || !dbmm_aligned16(center) || !dbmm_aligned16(basis) || (((uintptr_t)y) & 3u)) return DBMM_E_ALIGN;
    hipStream_t s = (hipStream_t)stream;
    switch (K) {
        case 1: launch_project<1>(x, center, basis, y, (int)N, (int)D, s); break;
        case 2: launch_project<2>(x, center, basis, y, (int)N, (int)D, s); break;
        case 3: launch_project<3>(x, center, basis, y, (int)N, (int)D, s); break;
        case 4: launch_project<4>(x, center, basis, y, (int)N, (int)D, s); break;
        case 5: launch_project<5>(x, center, basis, y, (int)N, (int)D, s); break;
        case 6: launch_project<6>(x, center, basis, y, (int)N, (int)D, s); break;
        case 7: launch_project<7>(x, center, basis, y, (int)N, (int)D, s); break;
        default: launch_project<8>(x, center, basis, y, (int)N, (int)D, s); break;
    }
    DBMM_CHECK_LAUNCH();
    return DBMM_OK;
}
