// Supervised-contrastive head on a fused Gram kernel (include/dbmm.h: dbmm_supcon_fwd / dbmm_supcon_bwd).
//
//   zn_i = z_i / ||z_i||,  S_ij = zn_i . zn_j / tau (j != i),  P(i) = { j != i : y_j == y_i },
//   l_i = logsumexp_{j != i} S_ij - mean_{j in P(i)} S_ij,  L_con = mean of l_i over the A rows with a positive.
//
// Three launches, no floating-point atomics, every sum in a fixed order:
//   supcon_gram_kernel    64 x 64 tiles of S on the exact-fp32 MFMA (v_mfma_f32_32x32x2_f32: a k-ordered fmaf chain, so S_ij and
//                         S_ji are the same bits); the row norms come out of the same loads; S goes to the workspace, each tile
//                         leaves per-row partials (max, sum of exp, sum over positives, positive count) of its 64 columns
//   supcon_reduce_kernel  one workgroup merges the partials in column-tile order, forms l_i, A and L_con (float64, row order) and,
//                         when the per-row CE is given, the mixed loss (1 - lambda) mean CE + lambda L_con
//   supcon_bwd_kernel     dz = s_in dz_in + lambda dz_con: G = dS + dS^T is an elementwise function of S_ij, the labels and four
//                         per-row numbers, built 64 x 32 at a time in LDS as the A operand of G zn; zn_i . dzn_i = sum_j G_ij S_ij
//                         rides along, so the projection and 1 / ||z|| are the epilogue
// The diagonal is excluded by index everywhere: it never enters a max or a sum.
#include "common.h"
#include <math.h>

namespace {

constexpr int SC_MAXB = 2048;
constexpr int TS = 64;                     // rows / columns of a Gram tile, rows of a backward tile
constexpr int KC = 32;                     // reduction depth staged in LDS at a time
constexpr int KP = KC + 1;                 // LDS pitch of a [64][KC] operand
constexpr int SP = TS + 1;                 // LDS pitch of the S tile
constexpr int BD = 64;                     // dz columns of a backward tile
constexpr int ZP = BD + 4;                 // LDS pitch of the [KC][BD] zn chunk (float4 stores)

inline size_t up4(size_t n) { return (n + 3) / 4 * 4; }
inline int sc_tiles(int64_t B) { return (int)((B + TS - 1) / TS); }
// workspace (floats): S [B][B] | partials [tiles][4][B] | 5 B + 4 spare (the one-call step keeps the head's outputs there)
inline size_t sc_part_off(int64_t B) { return up4((size_t)B * B); }
inline size_t sc_spare_off(int64_t B) { return sc_part_off(B) + up4((size_t)sc_tiles(B) * 4 * B); }
inline size_t sc_floats(int64_t B) { return sc_spare_off(B) + up4(5 * (size_t)B + 4); }

__global__ __launch_bounds__(256) void supcon_gram_kernel(const float* __restrict__ z, const long long* __restrict__ labels, float invT,
                                                          float* __restrict__ S, float* __restrict__ part, float* __restrict__ inv_norm,
                                                          int B, int D) {
    __shared__ __attribute__((aligned(16))) float lds[2 * TS * KP];            // rows i | rows j of the chunk; then the S tile [64][SP]
    __shared__ float inva[TS], invb[TS];
    __shared__ long long ya[TS], yb[TS];
    float* as = lds;
    float* bs = lds + TS * KP;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wr = wave >> 1, wc = wave & 1;
    const int i0 = blockIdx.y * TS, j0 = blockIdx.x * TS;
    const int lr = tid >> 3, lc = (tid & 7) * 4;                               // loader: one float4 of rows lr and lr + 32 of either operand
    bool va[2], vb[2];
    const float *za[2], *zb[2];
    f32x4 ra[2], rb[2];
    float ssa[2] = {0.f, 0.f}, ssb[2] = {0.f, 0.f};
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        va[h] = i0 + lr + 32 * h < B; vb[h] = j0 + lr + 32 * h < B;
        za[h] = z + (long long)(va[h] ? i0 + lr + 32 * h : 0) * D;
        zb[h] = z + (long long)(vb[h] ? j0 + lr + 32 * h : 0) * D;
        ra[h] = (f32x4){0.f, 0.f, 0.f, 0.f}; rb[h] = ra[h];
        if (lc < D) {
            if (va[h]) ra[h] = *(const f32x4*)(za[h] + lc);
            if (vb[h]) rb[h] = *(const f32x4*)(zb[h] + lc);
        }
    }
    f32x16 acc;
#pragma unroll
    for (int v = 0; v < 16; ++v) acc[v] = 0.f;
    const int ar = (wr * 32 + (lane & 31)) * KP + (lane >> 5), br = (wc * 32 + (lane & 31)) * KP + (lane >> 5);
    for (int k0 = 0; k0 < D; k0 += KC) {
        __syncthreads();                                                       // the previous chunk has been read
#pragma unroll
        for (int h = 0; h < 2; ++h) {
#pragma unroll
            for (int e = 0; e < 4; ++e) { as[(lr + 32 * h) * KP + lc + e] = ra[h][e]; bs[(lr + 32 * h) * KP + lc + e] = rb[h][e]; }
            ssa[h] += (ra[h][0] * ra[h][0] + ra[h][1] * ra[h][1]) + (ra[h][2] * ra[h][2] + ra[h][3] * ra[h][3]);
            ssb[h] += (rb[h][0] * rb[h][0] + rb[h][1] * rb[h][1]) + (rb[h][2] * rb[h][2] + rb[h][3] * rb[h][3]);
        }
        __syncthreads();
#pragma unroll
        for (int h = 0; h < 2; ++h) {                                          // the next chunk's loads fly over this chunk's MFMAs
            ra[h] = (f32x4){0.f, 0.f, 0.f, 0.f}; rb[h] = ra[h];
            if (k0 + KC + lc < D) {
                if (va[h]) ra[h] = *(const f32x4*)(za[h] + k0 + KC + lc);
                if (vb[h]) rb[h] = *(const f32x4*)(zb[h] + k0 + KC + lc);
            }
        }
#pragma unroll
        for (int kk = 0; kk < KC / 2; ++kk)
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(as[ar + 2 * kk], bs[br + 2 * kk], acc, 0, 0, 0);
    }
    // row norms: the eight loader threads of a row are neighbouring lanes
#pragma unroll
    for (int h = 0; h < 2; ++h) {
#pragma unroll
        for (int o = 1; o < 8; o <<= 1) { ssa[h] += __shfl_xor(ssa[h], o, 64); ssb[h] += __shfl_xor(ssb[h], o, 64); }
        if ((tid & 7) == 0) {
            inva[lr + 32 * h] = va[h] ? 1.f / sqrtf(ssa[h]) : 0.f;
            invb[lr + 32 * h] = vb[h] ? 1.f / sqrtf(ssb[h]) : 0.f;
        }
    }
    if (tid < TS) ya[tid] = i0 + tid < B ? labels[i0 + tid] : 0;
    else if (tid < 2 * TS) yb[tid - TS] = j0 + tid - TS < B ? labels[j0 + tid - TS] : 0;
    __syncthreads();                                                           // also: every wave is done with the operand chunk
    float* st = lds;
#pragma unroll
    for (int v = 0; v < 16; ++v) {
        const int li = wr * 32 + (v >> 2) * 8 + (lane >> 5) * 4 + (v & 3), lj = wc * 32 + (lane & 31);
        const float s = acc[v] * (inva[li] * invb[lj]) * invT;                  // inv_i inv_j first: S stays symmetric to the bit
        st[li * SP + lj] = s;
        if (i0 + li < B && j0 + lj < B) S[(long long)(i0 + li) * B + j0 + lj] = s;
    }
    if (blockIdx.x == 0 && tid < TS && i0 + tid < B) inv_norm[i0 + tid] = inva[tid];
    __syncthreads();
    // per-row partials over this tile's columns: four threads a row, 16 columns each, merged in lane order
    const int r = tid >> 2, q4 = tid & 3, gi = i0 + r;
    float m = -INFINITY;
#pragma unroll
    for (int c = 0; c < 16; ++c) {
        const int gj = j0 + q4 * 16 + c;
        if (gj < B && gj != gi) m = fmaxf(m, st[r * SP + q4 * 16 + c]);
    }
    float se = 0.f, ps = 0.f, np = 0.f;
    const long long yi = ya[r];
#pragma unroll
    for (int c = 0; c < 16; ++c) {
        const int lj = q4 * 16 + c, gj = j0 + lj;
        if (gj < B && gj != gi) {
            const float s = st[r * SP + lj];
            se += expf(s - m);
            if (yb[lj] == yi) { ps += s; np += 1.f; }
        }
    }
#pragma unroll
    for (int o = 1; o < 4; o <<= 1) {
        const float mo = __shfl_xor(m, o, 64), seo = __shfl_xor(se, o, 64);
        const float mn = fmaxf(m, mo);
        const float x0 = m > -INFINITY ? se * expf(m - mn) : 0.f, x1 = mo > -INFINITY ? seo * expf(mo - mn) : 0.f;
        se = x0 + x1;                                                          // (lane q4 == 0 holds the result that is kept)
        m = mn;
        ps += __shfl_xor(ps, o, 64);
        np += __shfl_xor(np, o, 64);
    }
    if (q4 == 0 && gi < B) {
        float* p = part + (long long)blockIdx.x * 4 * B + gi;
        p[0] = m; p[B] = se; p[2 * (long long)B] = ps; p[3 * (long long)B] = np;
    }
}

// stats [4][B]: row max | sum of exp(S - max) | |P(i)| | 1 / ||z_i|| (the last one written by the Gram kernel)
__global__ __launch_bounds__(256) void supcon_reduce_kernel(const float* __restrict__ part, const float* __restrict__ ce_rows, float lam,
                                                            float* __restrict__ stats, float* __restrict__ l_rows, float* __restrict__ con_loss,
                                                            float* __restrict__ mixed, float* __restrict__ n_anchors, int B, int nT) {
    __shared__ double sred[256];
    __shared__ int nred[256];
    __shared__ float s0[4];
    const int t = threadIdx.x;
    double acc = 0.0;
    int na = 0;
    for (int i = t; i < B; i += 256) {
        float m = -INFINITY;
        for (int tj = 0; tj < nT; ++tj) m = fmaxf(m, part[(long long)tj * 4 * B + i]);
        float se = 0.f, ps = 0.f, np = 0.f;
        for (int tj = 0; tj < nT; ++tj) {
            const float* p = part + (long long)tj * 4 * B + i;
            const float mt = p[0];
            if (mt > -INFINITY) se += p[B] * expf(mt - m);
            ps += p[2 * (long long)B];
            np += p[3 * (long long)B];
        }
        stats[i] = m; stats[B + i] = se; stats[2 * (long long)B + i] = np;
        float l = 0.f;
        if (np > 0.f) { l = (m + logf(se)) - ps / np; acc += (double)l; na += 1; }
        l_rows[i] = l;
    }
    sred[t] = acc; nred[t] = na;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (t < o) { sred[t] += sred[t + o]; nred[t] += nred[t + o]; }
        __syncthreads();
    }
    float ce = 0.f;
    if (ce_rows) {                                                             // the batch mean of the CE rows (mean_reduce_kernel's statements)
        float s = 0.f;
        for (int i = t; i < B; i += 256) s += ce_rows[i];
        s = wave_sum(s);
        if ((t & 63) == 0) s0[t >> 6] = s;
        __syncthreads();
        ce = ((s0[0] + s0[1]) + (s0[2] + s0[3])) / (float)B;
    }
    if (t != 0) return;
    const int A = nred[0];
    const float con = A ? (float)(sred[0] / (double)A) : 0.f;
    *con_loss = con;
    *n_anchors = (float)A;
    if (mixed) *mixed = ce_rows ? fmaf(1.f - lam, ce, lam * con) : con;
}

// dz may be dz_in (every element is read, then written, by one thread)
__global__ __launch_bounds__(256) void supcon_bwd_kernel(const float* __restrict__ z, const long long* __restrict__ labels, const float* __restrict__ S,
                                                         const float* __restrict__ stats, const float* __restrict__ n_anchors, float invT, float lam,
                                                         const float* dz_in, float s_in, float* dz, int B, int D) {
    __shared__ float gs[TS * KP];                                              // G chunk [64 i][KC j]
    __shared__ __attribute__((aligned(16))) float zs[KC * ZP];                 // zn chunk [KC j][BD d]
    __shared__ float rm[TS], re[TS], rp[TS], rinv[TS], proj[TS];
    __shared__ long long ry[TS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wr = wave >> 1, wc = wave & 1;
    const int i0 = blockIdx.y * TS, d0 = blockIdx.x * BD;
    const float A = *n_anchors, c = A > 0.f ? 1.f / A : 0.f;
    if (tid < TS) {
        const int gi = i0 + tid;
        float m = 0.f, e = 0.f, p = 0.f, iv = 0.f;
        long long y = 0;
        if (gi < B) {
            const float np = stats[2 * (long long)B + gi];
            m = stats[gi]; iv = stats[3 * (long long)B + gi]; y = labels[gi];
            if (np > 0.f) { e = c / stats[B + gi]; p = c / np; }
        }
        rm[tid] = m; re[tid] = e; rp[tid] = p; rinv[tid] = iv; ry[tid] = y;
    }
    // G build: thread = column jj of the chunk, rows rb + 8 e;  zn chunk: thread = float4 zc of rows zr, zr + 16
    const int jj = tid & 31, rb = tid >> 5, zr = tid >> 4, zc = (tid & 15) * 4;
    float sv[8], cm = 0.f, ce = 0.f, cp = 0.f, pj[8];
    long long cy = 0;
    f32x4 zv[2];
    bool vj = false;
    int gj = 0;
    auto fetch = [&](int j0) {
        gj = j0 + jj; vj = gj < B;
        cm = ce = cp = 0.f; cy = 0;
        if (vj) {
            const float np = stats[2 * (long long)B + gj];
            cm = stats[gj]; cy = labels[gj];
            if (np > 0.f) { ce = c / stats[B + gj]; cp = c / np; }
        }
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int gi = i0 + rb + 8 * e;
            sv[e] = (vj && gi < B) ? S[(long long)gi * B + gj] : 0.f;
        }
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            const int j = j0 + zr + 16 * e;
            zv[e] = (f32x4){0.f, 0.f, 0.f, 0.f};
            if (j < B && d0 + zc < D) zv[e] = *(const f32x4*)(z + (long long)j * D + d0 + zc) * stats[3 * (long long)B + j];
        }
    };
#pragma unroll
    for (int e = 0; e < 8; ++e) pj[e] = 0.f;
    f32x16 acc;
#pragma unroll
    for (int v = 0; v < 16; ++v) acc[v] = 0.f;
    const int ar = (wr * 32 + (lane & 31)) * KP + (lane >> 5), br = (lane >> 5) * ZP + wc * 32 + (lane & 31);
    fetch(0);
    __syncthreads();                                                           // the row statistics are in LDS
    for (int j0 = 0; j0 < B; j0 += KC) {
        if (j0) __syncthreads();                                               // the previous chunk has been read
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int li = rb + 8 * e, gi = i0 + li;
            float g = 0.f;
            if (vj && gi < B && gi != gj) {
                const float s = sv[e];
                g = expf(s - rm[li]) * re[li] + expf(s - cm) * ce;
                if (ry[li] == cy) g -= rp[li] + cp;
                pj[e] = fmaf(g, s, pj[e]);
            }
            gs[li * KP + jj] = g;
        }
        *(f32x4*)(zs + zr * ZP + zc) = zv[0];
        *(f32x4*)(zs + (zr + 16) * ZP + zc) = zv[1];
        __syncthreads();
        if (j0 + KC < B) fetch(j0 + KC);                                       // the next chunk's loads fly over this chunk's MFMAs
#pragma unroll
        for (int kk = 0; kk < KC / 2; ++kk)
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(gs[ar + 2 * kk], zs[br + 2 * kk * ZP], acc, 0, 0, 0);
    }
    // zn_i . dzn_i = sum_j G_ij S_ij: the 32 column threads of a row group are one half of a wave
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        float v = pj[e];
#pragma unroll
        for (int o = 16; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
        if (jj == 0) proj[rb + 8 * e] = v;
    }
    __syncthreads();
    const int d = d0 + wc * 32 + (lane & 31);
#pragma unroll
    for (int v = 0; v < 16; ++v) {
        const int li = wr * 32 + (v >> 2) * 8 + (lane >> 5) * 4 + (v & 3), gi = i0 + li;
        if (gi < B && d < D) {
            const long long o = (long long)gi * D + d;
            const float iv = rinv[li];
            const float con = (acc[v] * invT - proj[li] * (z[o] * iv)) * iv;
            const float out = lam * con;
            dz[o] = dz_in ? fmaf(s_in, dz_in[o], out) : out;                   // the fma written out: not left to the contraction setting
        }
    }
}

}  // namespace

extern "C" size_t dbmm_supcon_workspace_bytes(int64_t B, int64_t D) {
    (void)D;
    if (B < 2 || B > SC_MAXB) return 0;
    return sc_floats(B) * sizeof(float);
}

extern "C" int dbmm_supcon_fwd(const float* z, const int64_t* labels, float temperature, const float* ce_rows, float weight, float* con_loss,
                               float* mixed_loss, float* loss_rows, float* stats, float* n_anchors, int64_t B, int64_t D, void* workspace,
                               size_t workspace_bytes, void* stream) {
    if (!z || !labels || !con_loss || !loss_rows || !stats || !n_anchors || !workspace) return DBMM_E_ARG;
    if (ce_rows && !mixed_loss) return DBMM_E_ARG;
    if (B < 2 || D <= 0 || (D & 3) || D > INT32_MAX || !(temperature > 0.f)) return DBMM_E_SHAPE;
    if (B > SC_MAXB) return DBMM_E_UNSUPPORTED;
    if (workspace_bytes < dbmm_supcon_workspace_bytes(B, D)) return DBMM_E_WORKSPACE;
    if (!dbmm_aligned16(z) || !dbmm_aligned16(workspace)) return DBMM_E_ALIGN;
    float* S = (float*)workspace;
    float* part = S + sc_part_off(B);
    const int nT = sc_tiles(B);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(supcon_gram_kernel, dim3(nT, nT), dim3(256), 0, s, z, (const long long*)labels, 1.f / temperature, S, part,
                       stats + 3 * B, (int)B, (int)D);
    DBMM_CHECK_LAUNCH();
    hipLaunchKernelGGL(supcon_reduce_kernel, dim3(1), dim3(256), 0, s, part, ce_rows, weight, stats, loss_rows, con_loss, mixed_loss, n_anchors,
                       (int)B, nT);
    DBMM_CHECK_LAUNCH();
    return DBMM_OK;
}

extern "C" int dbmm_supcon_bwd(const float* z, const int64_t* labels, float temperature, const float* stats, const float* n_anchors, float weight,
                               const float* dz_in, float dz_in_scale, float* dz, int64_t B, int64_t D, const void* workspace,
                               size_t workspace_bytes, void* stream) {
    if (!z || !labels || !stats || !n_anchors || !dz || !workspace) return DBMM_E_ARG;
    if (B < 2 || D <= 0 || (D & 3) || D > INT32_MAX || !(temperature > 0.f)) return DBMM_E_SHAPE;
    if (B > SC_MAXB) return DBMM_E_UNSUPPORTED;
    if (workspace_bytes < dbmm_supcon_workspace_bytes(B, D)) return DBMM_E_WORKSPACE;
    if (!dbmm_aligned16(z) || !dbmm_aligned16(workspace)) return DBMM_E_ALIGN;
    hipLaunchKernelGGL(supcon_bwd_kernel, dim3((unsigned)((D + BD - 1) / BD), sc_tiles(B)), dim3(256), 0, (hipStream_t)stream, z,
                       (const long long*)labels, (const float*)workspace, stats, n_anchors, 1.f / temperature, weight, dz_in, dz_in_scale, dz,
                       (int)B, (int)D);
    DBMM_CHECK_LAUNCH();
    return DBMM_OK;
}

// the spare floats at the end of the workspace (the one-call step: stats [4][B] | l [B] | A, L_con)
float* dbmm_supcon_spare(void* workspace, int64_t B) { return (float*)workspace + sc_spare_off(B); }
