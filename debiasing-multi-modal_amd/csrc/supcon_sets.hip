// Contrastive head over sampled sets (include/dbmm.h: dbmm_supcon_sets_fwd / dbmm_supcon_sets_bwd).
//
// z [T S][D]: T sets of S = A + P + N rows; row 0 of a set is the anchor, rows A .. A+P-1 its positives, the last N rows its
// negatives, rows 1 .. A-1 (extra anchors) take no loss.
//   zn = z / ||z||,  c_j = zn_a . zn_j,  s_j = c_j / tau  (j in P u N),
//   l_t = log sum_{P u N} exp(s_j) - (1 / P) sum_P s_p,  L = scale * sum_t l_t.
// One anchor against S rows: nothing for the matrix cores, the work is two streaming passes over z and one over dz.  Four
// launches, no floating-point atomics, every sum in a fixed order:
//   sets_fwd_rows_kernel   one workgroup per (set, chunk of SETS_ROWS rows): normalises the anchor itself into LDS (every chunk: the same
//                          statements, the same bits), a wave takes zn_a . z_j and ||z_j||^2 of two rows at a time from one pass of 16-byte
//                          loads, writes c_j and 1 / ||z_j||, and leaves the chunk's partials (max, sum of exp, sum over positives)
//   sets_reduce_kernel     one wave per set merges the partials (a lane its chunks in chunk order, then the butterfly): l_t, the
//                          set's max m_t and sum se_t; L in float64 in set order
//   sets_bwd_rows_kernel   dz_j of its chunk -- a thread owns 16-byte columns and walks the chunk's rows, so the anchor sums
//                          sum_j g_j zn_j of the chunk accumulate in registers in row order -- and the chunk's partial [D] of them
//   sets_anchor_kernel     adds the chunk partials (a wave every fourth chunk in chunk order, then the four sums) and writes dz_a
#include "common.h"
#include <math.h>

namespace {

constexpr int SETS_ROWS = 32;              // rows of a chunk (ops.SETS_CHUNK_ROWS)
constexpr int SETS_MAXD = 8192;            // the normalised anchor lives in LDS: 32 KB

inline size_t up4(size_t n) { return (n + 3) / 4 * 4; }
inline int64_t sets_chunks(int64_t S) { return (S + SETS_ROWS - 1) / SETS_ROWS; }
// workspace (floats): c [T S] | 1 / ||z|| [T S] | partials [T nC][4] | stats [T][4] (m, se, 1 / ||z_a||, -) | sum g c [T nC] | anchor partials [T nC][D]
struct SetsLayout {
    size_t cosv, inv, part, stats, gc, apart, total;
};
inline SetsLayout sets_layout(int64_t T, int64_t S, int64_t D) {
    const size_t nC = (size_t)sets_chunks(S);
    SetsLayout L;
    size_t f = 0;
    L.cosv = f;  f += up4((size_t)T * S);
    L.inv = f;   f += up4((size_t)T * S);
    L.part = f;  f += (size_t)T * nC * 4;
    L.stats = f; f += (size_t)T * 4;
    L.gc = f;    f += up4((size_t)T * nC);
    L.apart = f; f += (size_t)T * nC * D;
    L.total = f;
    return L;
}

// merge of two (max, sum of exp relative to it) pairs; an empty side has max -inf and sum 0
__device__ __forceinline__ void lse_merge(float& m, float& se, float mo, float seo) {
    const float mn = fmaxf(m, mo);
    const float x0 = m > -INFINITY ? se * expf(m - mn) : 0.f, x1 = mo > -INFINITY ? seo * expf(mo - mn) : 0.f;
    se = x0 + x1;
    m = mn;
}

__global__ __launch_bounds__(256) void sets_fwd_rows_kernel(const float* __restrict__ z, float invT, float* __restrict__ cosv,
                                                            float* __restrict__ inv_norm, float* __restrict__ part, float* __restrict__ stats,
                                                            int S, int A, int P, int D) {
    extern __shared__ __attribute__((aligned(16))) float an[];                 // zn_a [D]
    __shared__ float red[4], wm[4], wse[4], wps[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, D4 = D >> 2;
    const int t = blockIdx.y, k = blockIdx.x, nC = gridDim.x, j0 = k * SETS_ROWS;
    const long long base = (long long)t * S;
    const float* za = z + base * D;
    float ss = 0.f;
    for (int q = tid; q < D4; q += 256) {
        const f32x4 v = *(const f32x4*)(za + 4 * q);
        ss = fmaf(v[0], v[0], ss); ss = fmaf(v[1], v[1], ss); ss = fmaf(v[2], v[2], ss); ss = fmaf(v[3], v[3], ss);
    }
    ss = wave_sum(ss);
    if (lane == 0) red[wave] = ss;
    __syncthreads();
    const float inva = 1.f / sqrtf((red[0] + red[1]) + (red[2] + red[3]));
    for (int q = tid; q < D4; q += 256) *(f32x4*)(an + 4 * q) = *(const f32x4*)(za + 4 * q) * inva;
    if (k == 0 && tid == 0) stats[4 * t + 2] = inva;
    __syncthreads();
    float m = -INFINITY, se = 0.f, ps = 0.f;                                   // this wave's rows, in row order (wave-uniform)
    for (int r = wave; r < SETS_ROWS; r += 8) {                                // rows r and r + 4 of the chunk: two rows' loads in flight
        const int ja = j0 + r, jb = ja + 4;
        if (ja >= S) break;
        const bool vb = jb < S;
        const float* za_ = z + (base + ja) * D;
        const float* zb_ = z + (base + (vb ? jb : ja)) * D;
        float dot[2] = {0.f, 0.f}, sq[2] = {0.f, 0.f};
#pragma unroll 2
        for (int q = lane; q < D4; q += 64) {
            const f32x4 a = *(const f32x4*)(an + 4 * q), v0 = *(const f32x4*)(za_ + 4 * q), v1 = *(const f32x4*)(zb_ + 4 * q);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                dot[0] = fmaf(a[e], v0[e], dot[0]); sq[0] = fmaf(v0[e], v0[e], sq[0]);
                dot[1] = fmaf(a[e], v1[e], dot[1]); sq[1] = fmaf(v1[e], v1[e], sq[1]);
            }
        }
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int j = h ? jb : ja;
            if (h && !vb) break;
            const float d = wave_sum(dot[h]), ij = 1.f / sqrtf(wave_sum(sq[h])), c = d * ij;
            if (lane == 0) { cosv[base + j] = c; inv_norm[base + j] = ij; }
            if (j >= A) {
                const float s = c * invT;
                lse_merge(m, se, s, 1.f);
                if (j < A + P) ps += s;
            }
        }
    }
    if (lane == 0) { wm[wave] = m; wse[wave] = se; wps[wave] = ps; }
    __syncthreads();
    if (tid == 0) {                                                            // the four waves in wave order
        float M = wm[0], SE = wse[0], PS = wps[0];
        for (int w = 1; w < 4; ++w) { lse_merge(M, SE, wm[w], wse[w]); PS += wps[w]; }
        float* p = part + ((long long)t * nC + k) * 4;
        p[0] = M; p[1] = SE; p[2] = PS; p[3] = 0.f;
    }
}

// one wave per set: lane i merges chunks i, i + 64, ... in chunk order, then the 64 lanes merge in butterfly order
__global__ __launch_bounds__(1024) void sets_reduce_kernel(const float* __restrict__ part, float scale, float* __restrict__ stats,
                                                           float* __restrict__ loss_sets, float* __restrict__ loss, int T, int nC, int P) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int t = wave; t < T; t += 16) {
        const float* p = part + (long long)t * nC * 4;
        float m = -INFINITY, se = 0.f, ps = 0.f;
        for (int k = lane; k < nC; k += 64) {
            const f32x4 v = *(const f32x4*)(p + 4 * k);
            lse_merge(m, se, v[0], v[1]);
            ps += v[2];
        }
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const float mo = __shfl_xor(m, o, 64), seo = __shfl_xor(se, o, 64);
            lse_merge(m, se, mo, seo);
            ps += __shfl_xor(ps, o, 64);
        }
        if (lane == 0) {
            stats[4 * t] = m; stats[4 * t + 1] = se;
            loss_sets[t] = (m + logf(se)) - ps / (float)P;
        }
    }
    __syncthreads();                                                           // loss_sets of this (only) workgroup is written
    if (threadIdx.x == 0) {
        double acc = 0.0;
        for (int t = 0; t < T; ++t) acc += (double)loss_sets[t];
        *loss = (float)((double)scale * acc);
    }
}

// dz rows 1 .. S-1 of the set (row 0 is sets_anchor_kernel's); apart [D], gcpart [1]: this chunk's sum_j g_j zn_j and sum_j g_j c_j
__global__ __launch_bounds__(256) void sets_bwd_rows_kernel(const float* __restrict__ z, const float* __restrict__ cosv,
                                                            const float* __restrict__ inv_norm, const float* __restrict__ stats, float scale,
                                                            float invT, float* __restrict__ dz, float* __restrict__ apart,
                                                            float* __restrict__ gcpart, int S, int A, int P, int D) {
    __shared__ float ca[SETS_ROWS], cb[SETS_ROWS], cz[SETS_ROWS], cg[SETS_ROWS];
    const int tid = threadIdx.x, D4 = D >> 2;
    const int t = blockIdx.y, k = blockIdx.x, nC = gridDim.x, j0 = k * SETS_ROWS;
    const long long base = (long long)t * S;
    const int n = S - j0 < SETS_ROWS ? S - j0 : SETS_ROWS;                     // rows of this chunk
    const int r0 = A - j0 < 0 ? 0 : (A - j0 < n ? A - j0 : n);                 // its rows before r0 are anchors
    const float inva = stats[4 * t + 2];
    if (tid < SETS_ROWS) {
        float a = 0.f, b = 0.f, zc = 0.f, gc = 0.f;
        const int j = j0 + tid;
        if (tid >= r0 && tid < n) {
            const float c = cosv[base + j], ij = inv_norm[base + j];
            const float e = expf(c * invT - stats[4 * t]) / stats[4 * t + 1];
            const float g = scale * (j < A + P ? e - 1.f / (float)P : e);
            a = g * invT * ij;                                                 // dz_j = a zn_a + b z_j
            b = -(a * c * ij);
            zc = g * ij;                                                       // g_j zn_j = zc z_j
            gc = g * c;
        }
        ca[tid] = a; cb[tid] = b; cz[tid] = zc; cg[tid] = gc;
    }
    __syncthreads();
    const float* zs = z + base * D;
    float* dzs = dz + base * D;
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    for (int q = tid; q < D4; q += 256) {
        const f32x4 a4 = *(const f32x4*)(zs + 4 * q) * inva;
        for (int r = (j0 == 0 ? 1 : 0); r < r0; ++r) *(f32x4*)(dzs + (long long)(j0 + r) * D + 4 * q) = zero;   // extra anchors
        f32x4 acc = zero;
#pragma unroll 8
        for (int r = r0; r < n; ++r) {
            const long long o = (long long)(j0 + r) * D + 4 * q;
            const f32x4 v = *(const f32x4*)(zs + o);
            const float a = ca[r], b = cb[r], zc = cz[r];
            f32x4 out;
#pragma unroll
            for (int e = 0; e < 4; ++e) { acc[e] = fmaf(zc, v[e], acc[e]); out[e] = fmaf(b, v[e], a * a4[e]); }
            *(f32x4*)(dzs + o) = out;
        }
        *(f32x4*)(apart + ((long long)t * nC + k) * D + 4 * q) = acc;
    }
    if (tid == 0) {
        float gc = 0.f;
        for (int r = 0; r < n; ++r) gc += cg[r];
        gcpart[(long long)t * nC + k] = gc;
    }
}

// dz_a = (sum_j g_j zn_j - (sum_j g_j c_j) zn_a) / (tau ||z_a||).  A workgroup owns 64 16-byte columns of one set: wave w adds the
// chunk partials w, w + 4, ... in chunk order, the four sums are added in the order (0 + 1) + (2 + 3); sum_j g_j c_j likewise over the
// lanes of wave 0, then the butterfly
__global__ __launch_bounds__(256) void sets_anchor_kernel(const float* __restrict__ z, const float* __restrict__ stats,
                                                          const float* __restrict__ apart, const float* __restrict__ gcpart, float invT,
                                                          float* __restrict__ dz, int S, int nC, int D) {
    __shared__ __attribute__((aligned(16))) float wacc[4][64][4];
    __shared__ float gcs;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int q = blockIdx.x * 64 + lane, t = blockIdx.y;
    const bool valid = q < (D >> 2);
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    if (valid) {
#pragma unroll 4
        for (int k = wave; k < nC; k += 4) acc += *(const f32x4*)(apart + ((long long)t * nC + k) * D + 4 * q);
    }
    *(f32x4*)wacc[wave][lane] = acc;
    if (wave == 0) {
        float gc = 0.f;
        for (int k = lane; k < nC; k += 64) gc += gcpart[(long long)t * nC + k];
        gc = wave_sum(gc);
        if (lane == 0) gcs = gc;
    }
    __syncthreads();
    if (wave != 0 || !valid) return;
    acc = (*(const f32x4*)wacc[0][lane] + *(const f32x4*)wacc[1][lane]) + (*(const f32x4*)wacc[2][lane] + *(const f32x4*)wacc[3][lane]);
    const float inva = stats[4 * t + 2], gc = gcs, w = invT * inva;
    const long long o = (long long)t * S * D + 4 * q;
    const f32x4 a4 = *(const f32x4*)(z + o) * inva;
    f32x4 out;
#pragma unroll
    for (int e = 0; e < 4; ++e) out[e] = fmaf(-gc, a4[e], acc[e]) * w;
    *(f32x4*)(dz + o) = out;
}

int sets_check(const void* z, const void* out0, const void* out1, const void* workspace, float temperature, int64_t T, int64_t A, int64_t P,
               int64_t N, int64_t D, size_t workspace_bytes) {
    if (!z || !out0 || !out1 || !workspace) return DBMM_E_ARG;
    if (T < 1 || A < 1 || P < 1 || N < 1 || D <= 0 || (D & 3) || !(temperature > 0.f)) return DBMM_E_SHAPE;
    if (T > 65535 || A > INT32_MAX || P > INT32_MAX || N > INT32_MAX || A + P + N > INT32_MAX || T * (A + P + N) > INT32_MAX) return DBMM_E_SHAPE;
    if (D > SETS_MAXD) return DBMM_E_UNSUPPORTED;
    if (workspace_bytes < dbmm_supcon_sets_workspace_bytes(T, A + P + N, D)) return DBMM_E_WORKSPACE;
    if (!dbmm_aligned16(z) || !dbmm_aligned16(workspace)) return DBMM_E_ALIGN;
    return DBMM_OK;
}

}  // namespace

extern "C" size_t dbmm_supcon_sets_workspace_bytes(int64_t T, int64_t S, int64_t D) {
    if (T < 1 || T > 65535 || S < 3 || S > INT32_MAX || T * S > INT32_MAX || D <= 0 || (D & 3) || D > SETS_MAXD) return 0;
    return sets_layout(T, S, D).total * sizeof(float);
}

extern "C" int dbmm_supcon_sets_fwd(const float* z, float scale, float temperature, float* loss, float* loss_sets, int64_t T, int64_t A,
                                    int64_t P, int64_t N, int64_t D, void* workspace, size_t workspace_bytes, void* stream) {
    const int rc = sets_check(z, loss, loss_sets, workspace, temperature, T, A, P, N, D, workspace_bytes);
    if (rc) return rc;
    const int64_t S = A + P + N;
    const SetsLayout L = sets_layout(T, S, D);
    float* f = (float*)workspace;
    const int nC = (int)sets_chunks(S);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(sets_fwd_rows_kernel, dim3(nC, (unsigned)T), dim3(256), (size_t)D * sizeof(float), s, z, 1.f / temperature, f + L.cosv,
                       f + L.inv, f + L.part, f + L.stats, (int)S, (int)A, (int)P, (int)D);
    DBMM_CHECK_LAUNCH();
    hipLaunchKernelGGL(sets_reduce_kernel, dim3(1), dim3(1024), 0, s, f + L.part, scale, f + L.stats, loss_sets, loss, (int)T, nC, (int)P);
    DBMM_CHECK_LAUNCH();
    return DBMM_OK;
}

extern "C" int dbmm_supcon_sets_bwd(const float* z, float scale, float temperature, float* dz, int64_t T, int64_t A, int64_t P, int64_t N,
                                    int64_t D, void* workspace, size_t workspace_bytes, void* stream) {
    const int rc = sets_check(z, dz, dz, workspace, temperature, T, A, P, N, D, workspace_bytes);
    if (rc) return rc;
    if (!dbmm_aligned16(dz)) return DBMM_E_ALIGN;
    const int64_t S = A + P + N;
    const SetsLayout L = sets_layout(T, S, D);
    float* f = (float*)workspace;
    const int nC = (int)sets_chunks(S);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(sets_bwd_rows_kernel, dim3(nC, (unsigned)T), dim3(256), 0, s, z, f + L.cosv, f + L.inv, f + L.stats, scale,
                       1.f / temperature, dz, f + L.apart, f + L.gc, (int)S, (int)A, (int)P, (int)D);
    DBMM_CHECK_LAUNCH();
    hipLaunchKernelGGL(sets_anchor_kernel, dim3((unsigned)((D / 4 + 63) / 64), (unsigned)T), dim3(256), 0, s, z, f + L.stats, f + L.apart,
                       f + L.gc, 1.f / temperature, dz, (int)S, nC, (int)D);
    DBMM_CHECK_LAUNCH();
    return DBMM_OK;
}
