// Debiasing-adapter step kernels (final_main.py:53-174, 426-496; demo/util.py:118-136):
// BatchNorm1d batch statistics / apply / backward, fused row-L2-norm + image x text logits +
// cross-entropy forward and backward, column reductions for bias gradients, a multi-tensor
// SGD-momentum update and the per-group accuracy counters.  These are HBM/launch-bound
// (arithmetic intensity ~1 FLOP/B); the four GEMM-shaped products go through
// dbmm_gemm_bias_act (fp32 MFMA).
#include "adapter_step.h"

namespace {

#include "adapter_bodies.inc"

// ---- BatchNorm1d(H) statistics over the batch: 8 columns x 32 row-lanes per block ---------
__global__ __launch_bounds__(256) void bn1d_stats_kernel(const float* __restrict__ h, int B, int H, float eps,
                                                         float momentum, float* __restrict__ mean_o,
                                                         float* __restrict__ invstd_o, float* __restrict__ rmean,
                                                         float* __restrict__ rvar, long long* __restrict__ nbt) {
    __shared__ float red[32][9];
    const int cl = threadIdx.x & 7, rl = threadIdx.x >> 3;
    const int j = blockIdx.x * 8 + cl;
    const bool ok = j < H;
    float s = 0.f;
    if (ok) for (int b = rl; b < B; b += 32) s += h[(long long)b * H + j];
    red[rl][cl] = s;
    __syncthreads();
    float mean = 0.f;
    for (int r = 0; r < 32; ++r) mean += red[r][cl];
    mean /= (float)B;
    __syncthreads();
    float q = 0.f;
    if (ok) for (int b = rl; b < B; b += 32) { const float d = h[(long long)b * H + j] - mean; q = fmaf(d, d, q); }
    red[rl][cl] = q;
    __syncthreads();
    if (rl == 0 && ok) {
        float var = 0.f;
        for (int r = 0; r < 32; ++r) var += red[r][cl];
        var /= (float)B;
        mean_o[j] = mean;
        invstd_o[j] = rsqrtf(var + eps);
        if (rmean) rmean[j] = (1.f - momentum) * rmean[j] + momentum * mean;
        if (rvar) rvar[j] = (1.f - momentum) * rvar[j] + momentum * (var * (float)B / (float)(B - 1));
    }
    if (nbt && blockIdx.x == 0 && threadIdx.x == 0) *nbt += 1;
}

__global__ __launch_bounds__(256) void bn1d_relu_kernel(const float* __restrict__ h, const float* __restrict__ mean,
                                                        const float* __restrict__ invstd,
                                                        const float* __restrict__ gamma,
                                                        const float* __restrict__ beta, float* __restrict__ r,
                                                        int H4, int var_mode, float eps, long long total) {
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total;
         i += (long long)gridDim.x * blockDim.x) {
        const int c = (int)(i % H4);
        f32x4 is = ((const f32x4*)invstd)[c];
        if (var_mode) {
#pragma unroll
            for (int k = 0; k < 4; ++k) is[k] = rsqrtf(is[k] + eps);
        }
        f32x4 v = (((const f32x4*)h)[i] - ((const f32x4*)mean)[c]) * is * ((const f32x4*)gamma)[c] +
                  ((const f32x4*)beta)[c];
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = fmaxf(v[k], 0.f);
        ((f32x4*)r)[i] = v;
    }
}

// dhn = dr * (hn > 0);  dbeta_j = sum_b dhn;  dgamma_j = sum_b dhn * xhat
__global__ __launch_bounds__(256) void bn1d_bwd_reduce_kernel(const float* __restrict__ dr,
                                                              const float* __restrict__ h,
                                                              const float* __restrict__ mean,
                                                              const float* __restrict__ invstd,
                                                              const float* __restrict__ gamma,
                                                              const float* __restrict__ beta, int B, int H,
                                                              float* __restrict__ dgamma, float* __restrict__ dbeta) {
    __shared__ float red[2][32][9];
    const int cl = threadIdx.x & 7, rl = threadIdx.x >> 3;
    const int j = blockIdx.x * 8 + cl;
    const bool ok = j < H;
    float sb = 0.f, sg = 0.f;
    if (ok) {
        const float mu = mean[j], is = invstd[j], ga = gamma[j], be = beta[j];
        for (int b = rl; b < B; b += 32) {
            const float xh = (h[(long long)b * H + j] - mu) * is;
            const float d = (fmaf(ga, xh, be) > 0.f) ? dr[(long long)b * H + j] : 0.f;
            sb += d;
            sg = fmaf(d, xh, sg);
        }
    }
    red[0][rl][cl] = sb; red[1][rl][cl] = sg;
    __syncthreads();
    if (rl == 0 && ok) {
        float a = 0.f, g = 0.f;
        for (int r = 0; r < 32; ++r) { a += red[0][r][cl]; g += red[1][r][cl]; }
        dbeta[j] = a; dgamma[j] = g;
    }
}

// dh = gamma * invstd * (dhn - dbeta/B - xhat * dgamma/B)      (train-mode BN backward)
__global__ __launch_bounds__(256) void bn1d_bwd_apply_kernel(const float* __restrict__ dr,
                                                             const float* __restrict__ h,
                                                             const float* __restrict__ mean,
                                                             const float* __restrict__ invstd,
                                                             const float* __restrict__ gamma,
                                                             const float* __restrict__ beta,
                                                             const float* __restrict__ dgamma,
                                                             const float* __restrict__ dbeta, float* __restrict__ dh,
                                                             int H, float invB, long long total) {
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total;
         i += (long long)gridDim.x * blockDim.x) {
        const int j = (int)(i % H);
        const float is = invstd[j], ga = gamma[j];
        const float xh = (h[i] - mean[j]) * is;
        const float d = (fmaf(ga, xh, beta[j]) > 0.f) ? dr[i] : 0.f;
        dh[i] = ga * is * (d - dbeta[j] * invB - xh * dgamma[j] * invB);
    }
}

// out[j] = sum_b x[b][j]: 16 columns (4 float4 lanes) x 64 row-lanes per block, fixed summation
// order (row-lane partial sums, then an LDS tree) => deterministic.  N % 4 == 0.
__global__ __launch_bounds__(256) void colsum_kernel(const float* __restrict__ x, int B, int N,
                                                     float* __restrict__ out) {
    __shared__ f32x4 red[64][4];
    const int cg = threadIdx.x & 3, rl = threadIdx.x >> 2;
    const int j = blockIdx.x * 16 + cg * 4;
    f32x4 s = {0.f, 0.f, 0.f, 0.f};
    if (j < N) for (int b = rl; b < B; b += 64) s += *(const f32x4*)(x + (long long)b * N + j);
    red[rl][cg] = s;
    __syncthreads();
    for (int o = 32; o > 0; o >>= 1) {
        if (rl < o) red[rl][cg] += red[rl + o][cg];
        __syncthreads();
    }
    if (rl == 0 && j < N) *(f32x4*)(out + j) = red[0][cg];
}

// y[r][:] = x[r][:] / ||x[r][:]||: one wave per row, the row read twice (the second pass hits L2), no epsilon (clip/model.py:362-363)
__global__ __launch_bounds__(256) void l2norm_rows_kernel(const float* __restrict__ x, float* __restrict__ y, int B, int D4) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= B) return;
    const f32x4* xr = (const f32x4*)x + (long long)row * D4;
    f32x4* yr = (f32x4*)y + (long long)row * D4;
    float s = 0.f;
    for (int i = lane; i < D4; i += 64) { const f32x4 v = xr[i]; s = fmaf(v.x, v.x, s); s = fmaf(v.y, v.y, s); s = fmaf(v.z, v.z, s); s = fmaf(v.w, v.w, s); }
    const float inv = 1.f / sqrtf(wave_sum(s));
    for (int i = lane; i < D4; i += 64) yr[i] = xr[i] * inv;
}

// tn[c][:] = text[:, c] / ||text[:, c]||
__global__ __launch_bounds__(256) void text_colnorm_kernel(const float* __restrict__ text, float* __restrict__ tn,
                                                           int D, int C) {
    __shared__ float red[4];
    const int c = blockIdx.x;
    float s = 0.f;
    for (int i = threadIdx.x; i < D; i += 256) { const float v = text[(long long)i * C + c]; s = fmaf(v, v, s); }
    s = wave_sum(s);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    const float inv = 1.f / sqrtf((red[0] + red[1]) + (red[2] + red[3]));
    for (int i = threadIdx.x; i < D; i += 256) tn[(long long)c * D + i] = text[(long long)i * C + c] * inv;
}

// ---- fused row L2-norm + logits + CE: one wave per row (ce_fwd_row / ce_bwd_row: adapter_bodies.inc) ----------------
template <int CMAX>
__global__ __launch_bounds__(256) void l2norm_sim_ce_fwd_kernel(
    const float* __restrict__ z, const float* __restrict__ z_old, float w_old, const float* __restrict__ tn,
    const long long* __restrict__ labels, float invT, float* __restrict__ logits, float* __restrict__ loss_rows,
    long long* __restrict__ pred, float* __restrict__ inv_norm, int B, int D4, int C) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= B) return;
    float lg[CMAX], inv;
    ce_fwd_row<CMAX>(z, z_old, w_old, tn, labels, invT, logits, loss_rows, pred, inv_norm, row, lane, D4, C, lg, inv, row);
}

__global__ __launch_bounds__(256) void mean_reduce_kernel(const float* __restrict__ x, int n, float* __restrict__ out) {
    __shared__ float red[4];
    float s = 0.f;
    for (int i = threadIdx.x; i < n; i += 256) s += x[i];
    s = wave_sum(s);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) *out = ((red[0] + red[1]) + (red[2] + red[3])) / (float)n;
}

template <int CMAX>
__global__ __launch_bounds__(256) void l2norm_sim_ce_bwd_kernel(
    const float* __restrict__ z, const float* __restrict__ inv_norm, float w_new, const float* __restrict__ tn,
    const float* __restrict__ logits, const long long* __restrict__ labels, const float* __restrict__ dlogits,
    float invT, float gscale, float* __restrict__ dz, int B, int D4, int C) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= B) return;
    float lgv[CMAX];
#pragma unroll
    for (int c = 0; c < CMAX; ++c) lgv[c] = (logits && c < C) ? logits[(long long)row * C + c] : -INFINITY;
    ce_bwd_row<CMAX>(z, inv_norm[row], w_new, tn, lgv, labels, dlogits, invT, gscale, dz, row, lane, D4, C, row);
}

// group DRO: the row's weight is its group's entry of the weight vector (gdro_weights_body), 0 for a group id outside [0, G)
template <int CMAX>
__global__ __launch_bounds__(256) void l2norm_sim_ce_bwd_w_kernel(
    const float* __restrict__ z, const float* __restrict__ inv_norm, float w_new, const float* __restrict__ tn,
    const float* __restrict__ logits, const long long* __restrict__ labels, const long long* __restrict__ groups,
    const float* __restrict__ weights, int G, float invT, float* __restrict__ dz, int B, int D4, int C) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= B) return;
    float lgv[CMAX];
#pragma unroll
    for (int c = 0; c < CMAX; ++c) lgv[c] = (c < C) ? logits[(long long)row * C + c] : -INFINITY;
    const int g = gdro_group(groups, nullptr, 0, row, G);
    ce_bwd_row<CMAX>(z, inv_norm[row], w_new, tn, lgv, labels, nullptr, invT, g >= 0 ? weights[g] : 0.f, dz, row, lane, D4, C, row);
}

__global__ __launch_bounds__(256) void gdro_weights_kernel(const float* __restrict__ loss_rows, const long long* __restrict__ groups,
                                                           const float* q_in, float* q_out, float* __restrict__ stats,
                                                           float* __restrict__ robust_loss, int B, int G, float eta) {
    gdro_weights_body(loss_rows, groups, nullptr, 0, q_in, q_out, stats, robust_loss, B, G, eta);
}

// the one-call step: forward and backward of a row in ONE launch (both are row-local; the logits stay in registers).  Same
// statements as the two kernels above, so the results are the same bits.
template <int CMAX>
__global__ __launch_bounds__(256) void l2norm_sim_ce_fwdbwd_kernel(
    const float* __restrict__ z, const float* __restrict__ z_old, float w_old, float w_new, const float* __restrict__ tn,
    const long long* __restrict__ labels, float invT, float gscale, float* __restrict__ logits, float* __restrict__ loss_rows,
    float* __restrict__ dz, int B, int D4, int C) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= B) return;
    float lg[CMAX], inv;
    ce_fwd_row<CMAX>(z, z_old, w_old, tn, labels, invT, logits, loss_rows, nullptr, nullptr, row, lane, D4, C, lg, inv, row);
    ce_bwd_row<CMAX>(z, inv, w_new, tn, lg, labels, nullptr, invT, gscale, dz, row, lane, D4, C, row);
}

// ---- per-row loss weights: L = (1 / B) sum_b row_w[b] CE_b (fixed weights: no batch reduction, so ERM's launch count) -------------
// The siblings of the three kernels above and of mean_reduce_kernel; the only new arithmetic is gscale * row_w[row] and
// loss_rows[b] * row_w[b], so all-ones weights give the unweighted kernels' bits.  logits / loss_rows stay unweighted.
template <int CMAX>
__global__ __launch_bounds__(256) void l2norm_sim_ce_bwd_rows_kernel(
    const float* __restrict__ z, const float* __restrict__ inv_norm, float w_new, const float* __restrict__ tn,
    const float* __restrict__ logits, const long long* __restrict__ labels, const float* __restrict__ row_w, float invT, float gscale,
    float* __restrict__ dz, int B, int D4, int C) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= B) return;
    float lgv[CMAX];
#pragma unroll
    for (int c = 0; c < CMAX; ++c) lgv[c] = (c < C) ? logits[(long long)row * C + c] : -INFINITY;
    ce_bwd_row<CMAX>(z, inv_norm[row], w_new, tn, lgv, labels, nullptr, invT, gscale * row_w[row], dz, row, lane, D4, C, row);
}

template <int CMAX>
__global__ __launch_bounds__(256) void l2norm_sim_ce_fwdbwd_rows_kernel(
    const float* __restrict__ z, const float* __restrict__ z_old, float w_old, float w_new, const float* __restrict__ tn,
    const long long* __restrict__ labels, const float* __restrict__ row_w, float invT, float gscale, float* __restrict__ logits,
    float* __restrict__ loss_rows, float* __restrict__ dz, int B, int D4, int C) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= B) return;
    float lg[CMAX], inv;
    ce_fwd_row<CMAX>(z, z_old, w_old, tn, labels, invT, logits, loss_rows, nullptr, nullptr, row, lane, D4, C, lg, inv, row);
    ce_bwd_row<CMAX>(z, inv, w_new, tn, lg, labels, nullptr, invT, gscale * row_w[row], dz, row, lane, D4, C, row);
}

__global__ __launch_bounds__(256) void mean_reduce_rows_kernel(const float* __restrict__ x, const float* __restrict__ row_w, int n,
                                                               float* __restrict__ out) {
    __shared__ float red[4];
    weighted_mean_body(x, row_w, nullptr, 0, n, red, out);
}

// ---- multi-tensor SGD with momentum ---------------------------------------------------------
struct SgdArgs {
    float* p[16];
    const float* g[16];
    float* m[16];
    long long n[16];
    int ns[16];            // > 1: g[t] holds ns[t] partial gradients n[t] apart, summed here in order (grad_reduce_kernel's order)
};
__global__ __launch_bounds__(256) void sgd_kernel(const SgdArgs a, float lr, float mu, float wd, int first) {
    const int t = blockIdx.y;
    sgd_body(blockIdx, gridDim, a.p[t], a.g[t], a.m[t], a.n[t], a.ns[t], lr, mu, wd, first);
}

// ---- update_dict counters --------------------------------------------------------------------
__global__ __launch_bounds__(256) void group_count_kernel(const float* __restrict__ logits,
                                                          const long long* __restrict__ y,
                                                          const long long* __restrict__ g,
                                                          unsigned long long* __restrict__ counts, int B, int C, int G) {
    __shared__ unsigned int sc[64][2];
    if (threadIdx.x < 64) { sc[threadIdx.x][0] = 0; sc[threadIdx.x][1] = 0; }
    __syncthreads();
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b < B) {
        int am = 0; float mx = logits[(long long)b * C];
        for (int c = 1; c < C; ++c) { const float v = logits[(long long)b * C + c]; if (v > mx) { mx = v; am = c; } }
        const long long gi = g[b];                 // compared as 64 bits: an id of 2^32 + 1 is outside [0, G), not group 1
        if (gi >= 0 && gi < G) {
            atomicAdd(&sc[gi][0], 1u);
            if ((long long)am == y[b]) atomicAdd(&sc[gi][1], 1u);
        }
    }
    __syncthreads();
    if (threadIdx.x < G) {
        if (sc[threadIdx.x][0]) atomicAdd(&counts[threadIdx.x * 2], (unsigned long long)sc[threadIdx.x][0]);
        if (sc[threadIdx.x][1]) atomicAdd(&counts[threadIdx.x * 2 + 1], (unsigned long long)sc[threadIdx.x][1]);
    }
}

// sums[g] += sum of loss_rows over group g; single block, fixed order => deterministic
__global__ __launch_bounds__(256) void group_loss_sum_kernel(const float* __restrict__ loss,
                                                             const long long* __restrict__ g,
                                                             float* __restrict__ sums, int B, int G) {
    __shared__ float red[256];
    for (int gi = 0; gi < G; ++gi) {
        float s = 0.f;
        for (int b = threadIdx.x; b < B; b += 256) if (g[b] == (long long)gi) s += loss[b];
        red[threadIdx.x] = s;
        __syncthreads();
        for (int o = 128; o > 0; o >>= 1) { if (threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o]; __syncthreads(); }
        if (threadIdx.x == 0) sums[gi] += red[0];
        __syncthreads();
    }
}

// out[i][:] = table[idx[i]][:]  (float4 lanes; indices clamped into the table)
__global__ __launch_bounds__(256) void gather_rows_kernel(const float* __restrict__ table,
                                                          const long long* __restrict__ idx, float* __restrict__ out,
                                                          int D4, long long n_rows, long long total) {
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total;
         i += (long long)gridDim.x * blockDim.x) {
        const long long r = i / D4;
        const int c = (int)(i - r * D4);
        long long src = idx[r];
        src = src < 0 ? 0 : (src >= n_rows ? n_rows - 1 : src);
        ((f32x4*)out)[i] = ((const f32x4*)table)[src * D4 + c];
    }
}

inline unsigned grid_for(long long total) {
    const long long blocks = (total + 255) / 256;
    return (unsigned)(blocks < 8192 ? (blocks > 0 ? blocks : 1) : 8192);
}

}  // namespace

extern "C" int dbmm_bn1d_stats(const float* h, int64_t B, int64_t H, float eps, float momentum, float* mean,
                               float* invstd, float* running_mean, float* running_var, int64_t* nbt, void* stream) {
    if (!h || !mean || !invstd) return DBMM_E_ARG;
    if (B < 2 || H <= 0 || B > INT32_MAX || H > INT32_MAX) return DBMM_E_SHAPE;  // torch raises for B == 1 too
    hipLaunchKernelGGL(bn1d_stats_kernel, dim3((unsigned)((H + 7) / 8)), dim3(256), 0, (hipStream_t)stream, h, (int)B,
                       (int)H, eps, momentum, mean, invstd, running_mean, running_var, (long long*)nbt);
    DBMM_CHECK_LAUNCH();
    return DBMM_OK;
}

extern "C" int dbmm_bn1d_relu(const float* h, const float* mean, const float* invstd, const float* gamma,
                              const float* beta, float* r, int64_t B, int64_t H, int var_mode, float eps,
                              void* stream) {
    if (!h || !mean || !invstd || !gamma || !beta || !r) return DBMM_E_ARG;
    if (B <= 0 || H <= 0 || (H & 3)) return DBMM_E_SHAPE;
    if (!dbmm_aligned16(h) || !dbmm_aligned16(r) || !dbmm_aligned16(mean) || !dbmm_aligned16(invstd) ||
        !dbmm_aligned16(gamma) || !dbmm_aligned16(beta))
        return DBMM_E_ALIGN;
    const long long total = (long long)B * (H / 4);
    hipLaunchKernelGGL(bn1d_relu_kernel, dim3(grid_for(total)), dim3(256), 0, (hipStream_t)stream, h, mean, invstd,
                       gamma, beta, r, (int)(H / 4), var_mode, eps, total);
    DBMM_CHECK_LAUNCH();
    return DBMM_OK;
}

extern "C" int dbmm_adapter_fwd(const float* x, const float* w1, const float* b1, const float* gamma,
                                const float* beta, float* running_mean, float* running_var, int64_t* nbt,
                                const float* w2, const float* b2, float* h, float* mean, float* invstd, float* r,
                                float* z, int64_t B, int64_t D, int64_t H, int train, float eps, float momentum,
                                void* stream) {
    if (!x || !w1 || !b1 || !gamma || !beta || !w2 || !b2 || !h || !r || !z) return DBMM_E_ARG;
    if (!running_mean || !running_var) return DBMM_E_ARG;
    if (train && (!mean || !invstd)) return DBMM_E_ARG;
    // before the first launch, as dbmm_adapter_bwd has it: the BatchNorm statistics kernel takes any H and updates the running
    // statistics, so a width only dbmm_bn1d_relu refuses must not get that far
    if (B <= 0 || D <= 0 || H <= 0 || (D & 3) || (H & 3) || (train && B < 2)) return DBMM_E_SHAPE;
    if (dbmm_adapter_fast_shape(B, D, H) && (!train || B >= 2) && dbmm_aligned16(x) && dbmm_aligned16(w1) && dbmm_aligned16(w2) && dbmm_aligned16(h) &&
        dbmm_aligned16(r) && dbmm_aligned16(z) && dbmm_aligned16(gamma) && dbmm_aligned16(beta) &&
        dbmm_aligned16(train ? mean : running_mean) && dbmm_aligned16(train ? invstd : running_var) && dbmm_opt(OPT_ADAPTER_STEP_FUSED))
        return dbmm_adapter_fwd_fast(x, w1, b1, gamma, beta, running_mean, running_var, nbt, w2, b2, h, mean, invstd, r, z, B, D, train, eps,
                                     momentum, (hipStream_t)stream);
    int rc = dbmm_gemm_bias_act(x, D, 0, w1, D, 0, b1, nullptr, 0, h, H, B, H, D, 1.f, DBMM_ACT_NONE, stream);
    if (rc) return rc;
    if (train) {
        rc = dbmm_bn1d_stats(h, B, H, eps, momentum, mean, invstd, running_mean, running_var, nbt, stream);
        if (rc) return rc;
        rc = dbmm_bn1d_relu(h, mean, invstd, gamma, beta, r, B, H, 0, eps, stream);
    } else {
        rc = dbmm_bn1d_relu(h, running_mean, running_var, gamma, beta, r, B, H, 1, eps, stream);
    }
    if (rc) return rc;
    return dbmm_gemm_bias_act(r, H, 0, w2, H, 0, b2, nullptr, 0, z, D, B, D, H, 1.f, DBMM_ACT_NONE, stream);
}

// dr [B][H] | dh [B][H] | the fast path's partial sums (adapter_step.hip)
extern "C" size_t dbmm_workspace_bytes_adapter_bwd(int64_t B, int64_t D, int64_t H) {
    return ((size_t)(2 * B * H) + (dbmm_adapter_fast_shape(B, D, H) ? dbmm_adapter_bwd_scratch(B, D).total : 0)) * sizeof(float);
}

extern "C" int dbmm_adapter_bwd(const float* x, const float* dz, const float* h, const float* mean,
                                const float* invstd, const float* r, const float* gamma, const float* beta,
                                const float* w2, float* dw1, float* db1, float* dgamma, float* dbeta, float* dw2,
                                float* db2, int64_t B, int64_t D, int64_t H, void* workspace, size_t workspace_bytes,
                                void* stream) {
    if (!x || !dz || !h || !mean || !invstd || !r || !gamma || !beta || !w2 || !dw1 || !db1 || !dgamma || !dbeta ||
        !dw2 || !db2 || !workspace)
        return DBMM_E_ARG;
    if (B < 2 || D <= 0 || H <= 0 || (D & 3) || (H & 3)) return DBMM_E_SHAPE;
    if (workspace_bytes < dbmm_workspace_bytes_adapter_bwd(B, D, H)) return DBMM_E_WORKSPACE;
    if (!dbmm_aligned16(workspace)) return DBMM_E_ALIGN;
    hipStream_t s = (hipStream_t)stream;
    float* dr = (float*)workspace;
    float* dh = dr + B * H;
    if (dbmm_adapter_fast_shape(B, D, H) && dbmm_aligned16(x) && dbmm_aligned16(dz) && dbmm_aligned16(r) && dbmm_aligned16(w2) && dbmm_aligned16(dw1) &&
        dbmm_aligned16(dw2) && dbmm_aligned16(db1) && dbmm_aligned16(db2) && dbmm_opt(OPT_ADAPTER_STEP_FUSED))
        return dbmm_adapter_bwd_fast(x, dz, h, mean, invstd, r, gamma, beta, w2, dw1, db1, dgamma, dbeta, dw2, db2, dh, dh + B * H, B, D, s, true, nullptr, nullptr);
    int rc;
    // dW2[D][H] = dz^T r   (reduction over the batch: both operands K-major)
    rc = dbmm_gemm_bias_act(dz, D, 1, r, H, 1, nullptr, nullptr, 0, dw2, H, D, H, B, 1.f, DBMM_ACT_NONE, stream);
    if (rc) return rc;
    hipLaunchKernelGGL(colsum_kernel, dim3((unsigned)((D + 15) / 16)), dim3(256), 0, s, dz, (int)B, (int)D, db2);
    DBMM_CHECK_LAUNCH();
    // dr[B][H] = dz W2   (W2 is [D][H]: K-major weight operand)
    rc = dbmm_gemm_bias_act(dz, D, 0, w2, H, 1, nullptr, nullptr, 0, dr, H, B, H, D, 1.f, DBMM_ACT_NONE, stream);
    if (rc) return rc;
    hipLaunchKernelGGL(bn1d_bwd_reduce_kernel, dim3((unsigned)((H + 7) / 8)), dim3(256), 0, s, dr, h, mean, invstd,
                       gamma, beta, (int)B, (int)H, dgamma, dbeta);
    DBMM_CHECK_LAUNCH();
    const long long total = (long long)B * H;
    hipLaunchKernelGGL(bn1d_bwd_apply_kernel, dim3(grid_for(total)), dim3(256), 0, s, dr, h, mean, invstd, gamma, beta,
                       dgamma, dbeta, dh, (int)H, 1.f / (float)B, total);
    DBMM_CHECK_LAUNCH();
    // dW1[H][D] = dh^T x
    rc = dbmm_gemm_bias_act(dh, H, 1, x, D, 1, nullptr, nullptr, 0, dw1, D, H, D, B, 1.f, DBMM_ACT_NONE, stream);
    if (rc) return rc;
    hipLaunchKernelGGL(colsum_kernel, dim3((unsigned)((H + 15) / 16)), dim3(256), 0, s, dh, (int)B, (int)H, db1);
    DBMM_CHECK_LAUNCH();
    return DBMM_OK;
}

extern "C" int dbmm_l2norm_rows(const float* x, float* y, int64_t B, int64_t D, void* stream) {
    if (!x || !y) return DBMM_E_ARG;
    if (B <= 0 || D <= 0 || (D & 3) || B > INT32_MAX) return DBMM_E_SHAPE;
    if (!dbmm_aligned16(x) || !dbmm_aligned16(y)) return DBMM_E_ALIGN;
    hipLaunchKernelGGL(l2norm_rows_kernel, dim3((unsigned)((B + 3) / 4)), dim3(256), 0, (hipStream_t)stream, x, y, (int)B, (int)(D / 4));
    DBMM_CHECK_LAUNCH();
    return DBMM_OK;
}

extern "C" int dbmm_colsum(const float* x, float* out, int64_t B, int64_t N, void* stream) {
    if (!x || !out) return DBMM_E_ARG;
    if (B <= 0 || N <= 0 || (N & 3) || B > INT32_MAX) return DBMM_E_SHAPE;
    if (!dbmm_aligned16(x) || !dbmm_aligned16(out)) return DBMM_E_ALIGN;
    hipLaunchKernelGGL(colsum_kernel, dim3((unsigned)((N + 15) / 16)), dim3(256), 0, (hipStream_t)stream, x, (int)B, (int)N, out);
    DBMM_CHECK_LAUNCH();
    return DBMM_OK;
}

extern "C" int dbmm_text_colnorm(const float* text, float* tn, int64_t D, int64_t C, void* stream) {
    if (!text || !tn) return DBMM_E_ARG;
    if (D <= 0 || C <= 0 || C > 65535) return DBMM_E_SHAPE;
    hipLaunchKernelGGL(text_colnorm_kernel, dim3((unsigned)C), dim3(256), 0, (hipStream_t)stream, text, tn, (int)D, (int)C);
    DBMM_CHECK_LAUNCH();
    return DBMM_OK;
}

extern "C" int dbmm_l2norm_sim_ce_fwd(const float* z, const float* z_old, float ebd_weight, const float* tn,
                                      const int64_t* labels, float temperature, float* logits, float* loss_rows,
                                      float* loss_mean, int64_t* pred, float* inv_norm, int64_t B, int64_t D,
                                      int64_t C, void* stream) {
    if (!z || !tn) return DBMM_E_ARG;
    if (B <= 0 || D <= 0 || (D & 3) || C <= 0 || C > 8 || B > INT32_MAX) return DBMM_E_SHAPE;
    if (loss_mean && !(loss_rows && labels)) return DBMM_E_ARG;
    if (!dbmm_aligned16(z) || !dbmm_aligned16(tn) || (z_old && !dbmm_aligned16(z_old))) return DBMM_E_ALIGN;
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid((unsigned)((B + 3) / 4));
    dbmm_with_cmax(C, [&](auto cm) {
        hipLaunchKernelGGL(l2norm_sim_ce_fwd_kernel<decltype(cm)::value>, grid, dim3(256), 0, s, z, z_old, ebd_weight, tn,
                           (const long long*)labels, 1.f / temperature, logits, loss_rows, (long long*)pred, inv_norm,
                           (int)B, (int)(D / 4), (int)C);
    });
    DBMM_CHECK_LAUNCH();
    if (loss_mean) {
        hipLaunchKernelGGL(mean_reduce_kernel, dim3(1), dim3(256), 0, s, loss_rows, (int)B, loss_mean);
        DBMM_CHECK_LAUNCH();
    }
    return DBMM_OK;
}

extern "C" int dbmm_l2norm_sim_ce_bwd(const float* z, const float* inv_norm, float ebd_weight, int blended,
                                      const float* tn, const float* logits, const int64_t* labels,
                                      const float* dlogits, float temperature, float grad_scale, float* dz,
                                      int64_t B, int64_t D, int64_t C, void* stream) {
    if (!z || !inv_norm || !tn || !dz) return DBMM_E_ARG;
    if (!dlogits && (!logits || !labels)) return DBMM_E_ARG;
    if (B <= 0 || D <= 0 || (D & 3) || C <= 0 || C > 8 || B > INT32_MAX) return DBMM_E_SHAPE;
    if (!dbmm_aligned16(z) || !dbmm_aligned16(tn) || !dbmm_aligned16(dz)) return DBMM_E_ALIGN;
    const float w_new = blended ? (1.f - ebd_weight) : 1.f;
    const float gs = grad_scale / (float)B;
    const dim3 grid((unsigned)((B + 3) / 4));
    hipStream_t s = (hipStream_t)stream;
    dbmm_with_cmax(C, [&](auto cm) {
        hipLaunchKernelGGL(l2norm_sim_ce_bwd_kernel<decltype(cm)::value>, grid, dim3(256), 0, s, z, inv_norm, w_new, tn, logits,
                           (const long long*)labels, dlogits, 1.f / temperature, gs, dz, (int)B, (int)(D / 4), (int)C);
    });
    DBMM_CHECK_LAUNCH();
    return DBMM_OK;
}

extern "C" int dbmm_group_dro_weights(const float* loss_rows, const int64_t* groups, const float* q_in, float* q_out, float* weights,
                                      float* robust_loss, int64_t B, int64_t G, float eta, void* stream) {
    if (!loss_rows || !groups || !q_in || !q_out || !weights || !robust_loss) return DBMM_E_ARG;
    if (G < 1 || G > GDRO_MAXG || B < 2 || B > INT32_MAX) return DBMM_E_SHAPE;
    hipLaunchKernelGGL(gdro_weights_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, loss_rows, (const long long*)groups, q_in, q_out, weights,
                       robust_loss, (int)B, (int)G, eta);
    DBMM_CHECK_LAUNCH();
    return DBMM_OK;
}

extern "C" int dbmm_l2norm_sim_ce_bwd_weighted(const float* z, const float* inv_norm, float ebd_weight, int blended, const float* tn,
                                               const float* logits, const int64_t* labels, const int64_t* groups, const float* weights,
                                               int64_t G, float temperature, float* dz, int64_t B, int64_t D, int64_t C, void* stream) {
    if (!z || !inv_norm || !tn || !dz || !logits || !labels || !groups || !weights) return DBMM_E_ARG;
    if (G < 1 || G > GDRO_MAXG || B < 2 || D <= 0 || (D & 3) || C <= 0 || C > 8 || B > INT32_MAX) return DBMM_E_SHAPE;
    if (!dbmm_aligned16(z) || !dbmm_aligned16(tn) || !dbmm_aligned16(dz)) return DBMM_E_ALIGN;
    const float w_new = blended ? (1.f - ebd_weight) : 1.f;
    const dim3 grid((unsigned)((B + 3) / 4));
    hipStream_t s = (hipStream_t)stream;
    dbmm_with_cmax(C, [&](auto cm) {
        hipLaunchKernelGGL(l2norm_sim_ce_bwd_w_kernel<decltype(cm)::value>, grid, dim3(256), 0, s, z, inv_norm, w_new, tn, logits,
                           (const long long*)labels, (const long long*)groups, weights, (int)G, 1.f / temperature, dz, (int)B, (int)(D / 4), (int)C);
    });
    DBMM_CHECK_LAUNCH();
    return DBMM_OK;
}

extern "C" int dbmm_weighted_mean(const float* x, const float* row_w, float* out, int64_t n, void* stream) {
    if (!x || !row_w || !out) return DBMM_E_ARG;
    if (n <= 0 || n > INT32_MAX) return DBMM_E_SHAPE;
    hipLaunchKernelGGL(mean_reduce_rows_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, x, row_w, (int)n, out);
    DBMM_CHECK_LAUNCH();
    return DBMM_OK;
}

extern "C" int dbmm_l2norm_sim_ce_bwd_rows(const float* z, const float* inv_norm, float ebd_weight, int blended, const float* tn,
                                           const float* logits, const int64_t* labels, const float* row_w, float temperature, float grad_scale,
                                           float* dz, int64_t B, int64_t D, int64_t C, void* stream) {
    if (!z || !inv_norm || !tn || !dz || !logits || !labels || !row_w) return DBMM_E_ARG;
    if (B <= 0 || D <= 0 || (D & 3) || C <= 0 || C > 8 || B > INT32_MAX) return DBMM_E_SHAPE;
    if (!dbmm_aligned16(z) || !dbmm_aligned16(tn) || !dbmm_aligned16(dz)) return DBMM_E_ALIGN;
    const float w_new = blended ? (1.f - ebd_weight) : 1.f;
    const float gs = grad_scale / (float)B;
    const dim3 grid((unsigned)((B + 3) / 4));
    hipStream_t s = (hipStream_t)stream;
    dbmm_with_cmax(C, [&](auto cm) {
        hipLaunchKernelGGL(l2norm_sim_ce_bwd_rows_kernel<decltype(cm)::value>, grid, dim3(256), 0, s, z, inv_norm, w_new, tn, logits,
                           (const long long*)labels, row_w, 1.f / temperature, gs, dz, (int)B, (int)(D / 4), (int)C);
    });
    DBMM_CHECK_LAUNCH();
    return DBMM_OK;
}

static int sgd_impl(int64_t n, float* const* params, const float* const* grads, float* const* bufs, const int64_t* sizes, const int* nsplit,
                    float lr, float momentum, float weight_decay, int first_step, void* stream) {
    if (!params || !grads || !bufs || !sizes) return DBMM_E_ARG;
    if (n <= 0 || n > 16) return DBMM_E_SHAPE;
    SgdArgs a{};
    long long mx = 0;
    for (int i = 0; i < n; ++i) {
        if (!params[i] || !grads[i] || !bufs[i] || sizes[i] <= 0) return DBMM_E_ARG;
        a.p[i] = params[i]; a.g[i] = grads[i]; a.m[i] = bufs[i]; a.n[i] = sizes[i]; a.ns[i] = nsplit ? nsplit[i] : 1;
        if (sizes[i] > mx) mx = sizes[i];
    }
    long long bx = (mx + 1023) / 1024;
    if (bx > 1024) bx = 1024;
    hipLaunchKernelGGL(sgd_kernel, dim3((unsigned)bx, (unsigned)n), dim3(256), 0, (hipStream_t)stream, a, lr, momentum,
                       weight_decay, first_step);
    DBMM_CHECK_LAUNCH();
    return DBMM_OK;
}

extern "C" int dbmm_sgd_momentum(int64_t n, float* const* params, const float* const* grads, float* const* bufs,
                                 const int64_t* sizes, float lr, float momentum, float weight_decay, int first_step,
                                 void* stream) {
    return sgd_impl(n, params, grads, bufs, sizes, nullptr, lr, momentum, weight_decay, first_step, stream);
}

extern "C" int dbmm_group_count(const float* logits, const int64_t* y, const int64_t* g, int64_t* counts, int64_t B,
                                int64_t C, int64_t G, void* stream) {
    if (!logits || !y || !g || !counts) return DBMM_E_ARG;
    if (B <= 0 || C <= 0 || G <= 0 || G > 64 || B > INT32_MAX) return DBMM_E_SHAPE;
    hipLaunchKernelGGL(group_count_kernel, dim3((unsigned)((B + 255) / 256)), dim3(256), 0, (hipStream_t)stream, logits,
                       (const long long*)y, (const long long*)g, (unsigned long long*)counts, (int)B, (int)C, (int)G);
    DBMM_CHECK_LAUNCH();
    return DBMM_OK;
}

extern "C" int dbmm_group_loss_sum(const float* loss_rows, const int64_t* g, float* sums, int64_t B, int64_t G,
                                   void* stream) {
    if (!loss_rows || !g || !sums) return DBMM_E_ARG;
    if (B <= 0 || G <= 0 || G > 64 || B > INT32_MAX) return DBMM_E_SHAPE;
    hipLaunchKernelGGL(group_loss_sum_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, loss_rows,
                       (const long long*)g, sums, (int)B, (int)G);
    DBMM_CHECK_LAUNCH();
    return DBMM_OK;
}

extern "C" int dbmm_gather_rows(const float* table, const int64_t* idx, float* out, int64_t n_rows, int64_t n_idx,
                                int64_t D, void* stream) {
    if (!table || !idx || !out) return DBMM_E_ARG;
    if (n_rows <= 0 || n_idx <= 0 || D <= 0 || (D & 3)) return DBMM_E_SHAPE;
    if (!dbmm_aligned16(table) || !dbmm_aligned16(out)) return DBMM_E_ALIGN;
    const long long total = (long long)n_idx * (D / 4);
    hipLaunchKernelGGL(gather_rows_kernel, dim3(grid_for(total)), dim3(256), 0, (hipStream_t)stream, table,
                       (const long long*)idx, out, (int)(D / 4), (long long)n_rows, total);
    DBMM_CHECK_LAUNCH();
    return DBMM_OK;
}

// ---- one call = one training step body (final_main.py:455-466 / :610-623) ----------------------
namespace {

// the step's workspace, as offsets in floats: h, r [B*H]x2 | z [B*D] | mean, invstd [H]x2 | (old: the same five) | (inv_norm [B])
// | dz [B*D] | dw1 [H*D] db1 dgamma dbeta [H]x3 dw2 [D*H] db2 [D] | bwd scratch (dbmm_workspace_bytes_adapter_bwd).  Every region
// is a multiple of 4 floats (16-B aligned) and so is `total`: a head's workspace follows the step's, 64 floats off its grid.
struct ActOffsets {
    size_t h, r, z, mean, invstd;
};
struct StepWs {
    ActOffsets a, o;
    size_t inv_norm, dz, g[6], bws, total;
    int64_t gn[6];          // sizes of the six gradients (dw1, db1, dgamma, dbeta, dw2, db2), the order of AdapterMomentum
};
StepWs step_ws(int64_t B, int64_t D, int64_t H, bool with_old, bool with_inv_norm) {
    StepWs L{};
    const int64_t gn[6] = {H * D, H, H, H, D * H, D};
    size_t f = 0;
    auto take = [&](size_t n) { const size_t o = f; f += (n + 3) / 4 * 4; return o; };
    auto acts = [&] { return ActOffsets{take(B * H), take(B * H), take(B * D), take(H), take(H)}; };      // braces: evaluated in order
    L.a = acts();
    if (with_old) L.o = acts();
    if (with_inv_norm) L.inv_norm = take(B);
    L.dz = take(B * D);
    for (int i = 0; i < 6; ++i) {
        L.gn[i] = gn[i];
        L.g[i] = take(gn[i]);
    }
    L.bws = take(dbmm_workspace_bytes_adapter_bwd(B, D, H) / sizeof(float));
    // 64 floats between the step's regions and a head's workspace: every region above is a multiple of 512 bytes at the reference's shapes, and
    // the contrastive head's Gram tiles on that same grid cost the mixed step 0.6 us of 141 (HISTORY.md); sizes equal the earlier ones
    L.total = f + 64;
    return L;
}

// nbt (num_batches_tracked) is optional
bool complete(const FrozenAdapter& p) { return p.w1 && p.b1 && p.gamma && p.beta && p.rmean && p.rvar && p.w2 && p.b2; }
bool complete(const AdapterMomentum& m) { return m.w1 && m.b1 && m.gamma && m.beta && m.w2 && m.b2; }

// forward of one adapter with train-mode BatchNorm1d (its defaults: eps 1e-5, momentum 0.1) into its activations
int fwd_train(const float* x, const FrozenAdapter& p, float* f, const ActOffsets& a, int64_t B, int64_t D, int64_t H, void* stream) {
    return dbmm_adapter_fwd(x, p.w1, p.b1, p.gamma, p.beta, p.rmean, p.rvar, (int64_t*)p.nbt, p.w2, p.b2, f + a.h, f + a.mean, f + a.invstd, f + a.r,
                            f + a.z, B, D, H, 1, 1e-5f, 0.1f, stream);
}

// what the cosine-logits heads read and write: z of the trainable branch and of the frozen one (or null), the prompts; logits,
// per-row losses, 1 / ||z|| and dz.  `fast`: the step runs on the purpose-built kernels (adapter_step.hip)
struct HeadIo {
    const float *z, *oz, *tn;
    const int64_t* labels;
    float ebd_weight, temperature;
    float *logits, *loss_rows, *inv_norm, *dz;
    int64_t B, D, C;
    bool fast;
    void* stream;
};
struct GdroHead {
    const int64_t* groups;
    float* q;
    float eta;
    int64_t G;
};
struct SupconHead {
    float weight, tau;
    float* loss;
};

// plain CE.  fast: forward AND backward of a row are one launch (row-local) and the batch mean of the losses rides in a spare block
// of the backward's first launch (*spare); else the two stand-alone calls, the first one followed by the mean's launch -- the same
// statements, hence the same bits.  `loss_mean` null: a head on top of this one writes the loss
int head_ce(const HeadIo& io, float* loss_mean, bool* spare) {
    *spare = io.fast && loss_mean;
    if (io.fast) {
        const float w_new = io.oz ? (1.f - io.ebd_weight) : 1.f;
        dbmm_with_cmax(io.C, [&](auto cm) {
            hipLaunchKernelGGL(l2norm_sim_ce_fwdbwd_kernel<decltype(cm)::value>, dim3((unsigned)((io.B + 3) / 4)), dim3(256), 0,
                               (hipStream_t)io.stream, io.z, io.oz, io.ebd_weight, w_new, io.tn, (const long long*)io.labels, 1.f / io.temperature,
                               1.f / (float)io.B, io.logits, io.loss_rows, io.dz, (int)io.B, (int)(io.D / 4), (int)io.C);
        });
        DBMM_CHECK_LAUNCH();
        return DBMM_OK;
    }
    const int rc = dbmm_l2norm_sim_ce_fwd(io.z, io.oz, io.ebd_weight, io.tn, io.labels, io.temperature, io.logits, io.loss_rows, loss_mean, nullptr,
                                          io.inv_norm, io.B, io.D, io.C, io.stream);
    if (rc) return rc;
    return dbmm_l2norm_sim_ce_bwd(io.z, io.inv_norm, io.ebd_weight, io.oz != nullptr, io.tn, io.logits, io.labels, nullptr, io.temperature, 1.f,
                                  io.dz, io.B, io.D, io.C, io.stream);
}

// CE under fixed per-row weights `row_w` [B]: head_ce's launches with the row's gradient scale (1 / B) row_w[b] and the mean of
// loss_rows[b] row_w[b] (fast: by the backward's spare block, which then reads the weights too -- *spare).  logits and loss_rows
// are ERM's; a row of weight 0 still takes part in the BatchNorm statistics, which ran before the head
int head_ce_weighted(const HeadIo& io, const float* row_w, float* loss_mean, bool* spare) {
    *spare = io.fast;
    const float w_new = io.oz ? (1.f - io.ebd_weight) : 1.f;
    if (io.fast) {
        dbmm_with_cmax(io.C, [&](auto cm) {
            hipLaunchKernelGGL(l2norm_sim_ce_fwdbwd_rows_kernel<decltype(cm)::value>, dim3((unsigned)((io.B + 3) / 4)), dim3(256), 0,
                               (hipStream_t)io.stream, io.z, io.oz, io.ebd_weight, w_new, io.tn, (const long long*)io.labels, row_w,
                               1.f / io.temperature, 1.f / (float)io.B, io.logits, io.loss_rows, io.dz, (int)io.B, (int)(io.D / 4), (int)io.C);
        });
        DBMM_CHECK_LAUNCH();
        return DBMM_OK;
    }
    int rc = dbmm_l2norm_sim_ce_fwd(io.z, io.oz, io.ebd_weight, io.tn, io.labels, io.temperature, io.logits, io.loss_rows, nullptr, nullptr,
                                    io.inv_norm, io.B, io.D, io.C, io.stream);
    if (rc) return rc;
    rc = dbmm_weighted_mean(io.loss_rows, row_w, loss_mean, io.B, io.stream);
    if (rc) return rc;
    return dbmm_l2norm_sim_ce_bwd_rows(io.z, io.inv_norm, io.ebd_weight, io.oz != nullptr, io.tn, io.logits, io.labels, row_w, io.temperature, 1.f,
                                       io.dz, io.B, io.D, io.C, io.stream);
}

// group DRO: a row's weight needs the whole batch's losses, so the head is three launches -- forward rows, the group reduction + q
// update (one workgroup), weighted backward rows; the robust loss is written by the second.  The [3][G] statistics live in `stats`
// (the start of the backward scratch, unused until then).
int head_gdro(const HeadIo& io, const GdroHead& g, float* stats, float* robust_loss) {
    int rc = dbmm_l2norm_sim_ce_fwd(io.z, io.oz, io.ebd_weight, io.tn, io.labels, io.temperature, io.logits, io.loss_rows, nullptr, nullptr,
                                    io.inv_norm, io.B, io.D, io.C, io.stream);
    if (rc) return rc;
    rc = dbmm_group_dro_weights(io.loss_rows, g.groups, g.q, g.q, stats, robust_loss, io.B, g.G, g.eta, io.stream);
    if (rc) return rc;
    return dbmm_l2norm_sim_ce_bwd_weighted(io.z, io.inv_norm, io.ebd_weight, io.oz != nullptr, io.tn, io.logits, io.labels, g.groups, stats, g.G,
                                           io.temperature, io.dz, io.B, io.D, io.C, io.stream);
}

// CE + the supervised-contrastive head (supcon.hip), which reads the trainable branch's z against itself: Gram tiles, the reduction
// (which also takes the mean of the CE rows and writes the mixed loss), and the backward onto the CE head's dz in place.  The
// statistics live in the spare floats of the contrastive workspace `cws`.
int head_ce_supcon(const HeadIo& io, const SupconHead& c, float* mixed_loss, void* cws, size_t cbytes) {
    bool spare;
    int rc = head_ce(io, nullptr, &spare);
    if (rc) return rc;
    float* sp = dbmm_supcon_spare(cws, io.B);
    rc = dbmm_supcon_fwd(io.z, io.labels, c.tau, io.loss_rows, c.weight, c.loss, mixed_loss, sp + 4 * io.B, sp, sp + 5 * io.B, io.B, io.D, cws,
                         cbytes, io.stream);
    if (rc) return rc;
    return dbmm_supcon_bwd(io.z, io.labels, c.tau, sp, sp + 5 * io.B, c.weight, io.dz, 1.f - c.weight, io.dz, io.B, io.D, cws, cbytes, io.stream);
}

// the contrastive loss of T sampled sets (supcon_sets.hip) and its gradient
int head_sets(const float* z, float* dz, float scale, float tau, float* loss, float* loss_sets, int64_t T, int64_t A, int64_t P, int64_t N, int64_t D,
              void* hws, size_t hbytes, void* stream) {
    const int rc = dbmm_supcon_sets_fwd(z, scale, tau, loss, loss_sets, T, A, P, N, D, hws, hbytes, stream);
    if (rc) return rc;
    return dbmm_supcon_sets_bwd(z, scale, tau, dz, T, A, P, N, D, hws, hbytes, stream);
}

// the tail of every step: adapter backward from dz, then SGD.  fast: the batch-split dW1 / db1 partial sums stay in the backward's
// scratch and are summed inside the SGD launch, and `loss_mean` given has the backward's spare block write the mean of loss_rows
// (of loss_rows[b] row_w[b] with `row_w`)
int bwd_sgd(const float* x, const AdapterParams& p, const AdapterMomentum& m, const SgdScalars& sc, float* f, const StepWs& L, bool fast,
            const float* loss_rows, float* loss_mean, int64_t B, int64_t D, int64_t H, void* stream, const float* row_w = nullptr) {
    float* ps[6] = {p.w1, p.b1, p.gamma, p.beta, p.w2, p.b2};
    float* ms[6] = {m.w1, m.b1, m.gamma, m.beta, m.w2, m.b2};
    float* gs[6];
    for (int i = 0; i < 6; ++i) gs[i] = f + L.g[i];
    const float *dz = f + L.dz, *h = f + L.a.h, *mean = f + L.a.mean, *invstd = f + L.a.invstd, *r = f + L.a.r;
    float* bws = f + L.bws;                                               // dr [B*H] | dh [B*H] | the fast path's scratch
    if (!fast) {
        const int rc = dbmm_adapter_bwd(x, dz, h, mean, invstd, r, p.gamma, p.beta, p.w2, gs[0], gs[1], gs[2], gs[3], gs[4], gs[5], B, D, H, bws,
                                        dbmm_workspace_bytes_adapter_bwd(B, D, H), stream);
        if (rc) return rc;
        return sgd_impl(6, ps, gs, ms, L.gn, nullptr, sc.lr, sc.momentum, sc.weight_decay, sc.first_step, stream);
    }
    const BwdScratch S = dbmm_adapter_bwd_scratch(B, D);
    float* scratch = bws + 2 * B * H;
    const int rc = dbmm_adapter_bwd_fast(x, dz, h, mean, invstd, r, p.gamma, p.beta, p.w2, gs[0], gs[1], gs[2], gs[3], gs[4], gs[5], bws + B * H,
                                         scratch, B, D, (hipStream_t)stream, false, loss_rows, loss_mean, row_w);
    if (rc) return rc;
    gs[0] = scratch + S.dw1part;
    gs[1] = scratch + S.db1part;
    const int nsp[6] = {S.NS, S.NS, 1, 1, 1, 1};
    return sgd_impl(6, ps, gs, ms, L.gn, nsp, sc.lr, sc.momentum, sc.weight_decay, sc.first_step, stream);
}

// `gdro.groups` given: the group-DRO step (q [G] updated in place, loss_mean = the robust loss); `con.loss` given: the ERM step with the
// supervised-contrastive head on top (loss_mean = the mixed loss); `row_w` given: the step under fixed per-row loss weights (loss_mean =
// (1 / B) sum_b row_w[b] CE_b); else the ERM step.  `old`: the frozen adapter, or none (w1 null)
int train_step_impl(const float* x, const int64_t* labels, const AdapterParams& p, const AdapterMomentum& m, const FrozenAdapter& old,
                    float ebd_weight, const float* tn, float temperature, const SgdScalars& sc, float* logits, float* loss_rows, float* loss_mean,
                    const GdroHead& gdro, const SupconHead& con, int64_t B, int64_t D, int64_t H, int64_t C, void* workspace, size_t workspace_bytes,
                    void* stream, const float* row_w = nullptr) {
    if (!x || !labels || !complete(p.forward_only()) || !complete(m) || !tn || !logits || !loss_rows || !loss_mean || !workspace)
        return DBMM_E_ARG;
    const bool with_old = old.w1 != nullptr, with_con = con.loss != nullptr;
    if (with_old && !complete(old)) return DBMM_E_ARG;
    if (B < 2 || D <= 0 || H <= 0 || (D & 3) || (H & 3) || C <= 0 || C > 8) return DBMM_E_SHAPE;
    const StepWs L = step_ws(B, D, H, with_old, true);
    const size_t step_bytes = L.total * sizeof(float), cbytes = with_con ? dbmm_supcon_workspace_bytes(B, D) : 0;
    if (with_con) {
        if (!(con.tau > 0.f)) return DBMM_E_SHAPE;
        if (!cbytes) return DBMM_E_UNSUPPORTED;                                  // B > 2048: nothing has been launched
        if (workspace_bytes < step_bytes + cbytes) return DBMM_E_WORKSPACE;
    }
    if (workspace_bytes < step_bytes) return DBMM_E_WORKSPACE;
    if (!dbmm_aligned16(workspace)) return DBMM_E_ALIGN;
    float* f = (float*)workspace;
    int rc = fwd_train(x, p.forward_only(), f, L.a, B, D, H, stream);
    if (rc) return rc;
    if (with_old) {   // frozen branch: forward only, but BatchNorm still in train mode
        rc = fwd_train(x, old, f, L.o, B, D, H, stream);
        if (rc) return rc;
    }
    const bool fast = dbmm_adapter_fast_shape(B, D, H) && dbmm_opt(OPT_ADAPTER_STEP_FUSED) && dbmm_aligned16(x);
    const HeadIo io{f + L.a.z, with_old ? f + L.o.z : nullptr, tn, labels, ebd_weight, temperature, logits, loss_rows, f + L.inv_norm, f + L.dz,
                    B, D, C, fast, stream};
    bool spare = false;                      // the loss mean is still to be written, by the backward's spare block
    if (gdro.groups) rc = head_gdro(io, gdro, f + L.bws, loss_mean);
    else if (with_con) rc = head_ce_supcon(io, con, loss_mean, (char*)workspace + step_bytes, cbytes);
    else if (row_w) rc = head_ce_weighted(io, row_w, loss_mean, &spare);
    else rc = head_ce(io, loss_mean, &spare);
    if (rc) return rc;
    return bwd_sgd(x, p, m, sc, f, L, fast, spare ? loss_rows : nullptr, spare ? loss_mean : nullptr, B, D, H, stream, spare ? row_w : nullptr);
}

}  // namespace

extern "C" size_t dbmm_workspace_bytes_adapter_train_step(int64_t B, int64_t D, int64_t H, int with_old) {
    return step_ws(B, D, H, with_old != 0, true).total * sizeof(float);
}

extern "C" int dbmm_adapter_train_step(const float* x, const int64_t* labels, float* w1, float* b1, float* gamma,
                                       float* beta, float* rmean, float* rvar, int64_t* nbt, float* w2, float* b2,
                                       float* m_w1, float* m_b1, float* m_gamma, float* m_beta, float* m_w2,
                                       float* m_b2, const float* o_w1, const float* o_b1, const float* o_gamma,
                                       const float* o_beta, float* o_rmean, float* o_rvar, int64_t* o_nbt,
                                       const float* o_w2, const float* o_b2, float ebd_weight, const float* tn,
                                       float temperature, float lr, float momentum, float weight_decay,
                                       int first_step, float* logits, float* loss_rows, float* loss_mean, int64_t B,
                                       int64_t D, int64_t H, int64_t C, void* workspace, size_t workspace_bytes,
                                       void* stream) {
    return train_step_impl(x, labels, {w1, b1, gamma, beta, rmean, rvar, (long long*)nbt, w2, b2}, {m_w1, m_b1, m_gamma, m_beta, m_w2, m_b2},
                           {o_w1, o_b1, o_gamma, o_beta, o_rmean, o_rvar, (long long*)o_nbt, o_w2, o_b2}, ebd_weight, tn, temperature,
                           {lr, momentum, weight_decay, first_step}, logits, loss_rows, loss_mean, {}, {}, B, D, H, C, workspace,
                           workspace_bytes, stream);
}

// the ERM step under per-row loss weights row_w [B] (fp32, taken as they are): L = (1 / B) sum_b row_w[b] CE_b.  Same workspace and
// launch count as dbmm_adapter_train_step; logits / loss_rows are the unweighted ones; all-ones weights give that step's bits
extern "C" int dbmm_adapter_train_step_weighted(const float* x, const int64_t* labels, float* w1, float* b1, float* gamma,
                                                float* beta, float* rmean, float* rvar, int64_t* nbt, float* w2, float* b2,
                                                float* m_w1, float* m_b1, float* m_gamma, float* m_beta, float* m_w2,
                                                float* m_b2, const float* o_w1, const float* o_b1, const float* o_gamma,
                                                const float* o_beta, float* o_rmean, float* o_rvar, int64_t* o_nbt,
                                                const float* o_w2, const float* o_b2, float ebd_weight, const float* tn,
                                                float temperature, float lr, float momentum, float weight_decay,
                                                int first_step, float* logits, float* loss_rows, float* loss_mean,
                                                const float* row_w, int64_t B, int64_t D, int64_t H, int64_t C, void* workspace,
                                                size_t workspace_bytes, void* stream) {
    if (!row_w) return DBMM_E_ARG;
    return train_step_impl(x, labels, {w1, b1, gamma, beta, rmean, rvar, (long long*)nbt, w2, b2}, {m_w1, m_b1, m_gamma, m_beta, m_w2, m_b2},
                           {o_w1, o_b1, o_gamma, o_beta, o_rmean, o_rvar, (long long*)o_nbt, o_w2, o_b2}, ebd_weight, tn, temperature,
                           {lr, momentum, weight_decay, first_step}, logits, loss_rows, loss_mean, {}, {}, B, D, H, C, workspace,
                           workspace_bytes, stream, row_w);
}

extern "C" int dbmm_adapter_train_step_gdro(const float* x, const int64_t* labels, float* w1, float* b1, float* gamma,
                                            float* beta, float* rmean, float* rvar, int64_t* nbt, float* w2, float* b2,
                                            float* m_w1, float* m_b1, float* m_gamma, float* m_beta, float* m_w2,
                                            float* m_b2, const float* o_w1, const float* o_b1, const float* o_gamma,
                                            const float* o_beta, float* o_rmean, float* o_rvar, int64_t* o_nbt,
                                            const float* o_w2, const float* o_b2, float ebd_weight, const float* tn,
                                            float temperature, float lr, float momentum, float weight_decay,
                                            int first_step, float* logits, float* loss_rows, float* robust_loss,
                                            const int64_t* groups, float* q, float eta, int64_t G, int64_t B,
                                            int64_t D, int64_t H, int64_t C, void* workspace, size_t workspace_bytes,
                                            void* stream) {
    if (!groups || !q) return DBMM_E_ARG;
    if (G < 1 || G > GDRO_MAXG) return DBMM_E_SHAPE;
    return train_step_impl(x, labels, {w1, b1, gamma, beta, rmean, rvar, (long long*)nbt, w2, b2}, {m_w1, m_b1, m_gamma, m_beta, m_w2, m_b2},
                           {o_w1, o_b1, o_gamma, o_beta, o_rmean, o_rvar, (long long*)o_nbt, o_w2, o_b2}, ebd_weight, tn, temperature,
                           {lr, momentum, weight_decay, first_step}, logits, loss_rows, robust_loss, {groups, q, eta, G}, {}, B, D, H, C, workspace,
                           workspace_bytes, stream);
}

extern "C" int dbmm_adapter_train_step_supcon(const float* x, const int64_t* labels, float* w1, float* b1, float* gamma,
                                              float* beta, float* rmean, float* rvar, int64_t* nbt, float* w2, float* b2,
                                              float* m_w1, float* m_b1, float* m_gamma, float* m_beta, float* m_w2,
                                              float* m_b2, const float* o_w1, const float* o_b1, const float* o_gamma,
                                              const float* o_beta, float* o_rmean, float* o_rvar, int64_t* o_nbt,
                                              const float* o_w2, const float* o_b2, float ebd_weight, const float* tn,
                                              float temperature, float lr, float momentum, float weight_decay,
                                              int first_step, float* logits, float* loss_rows, float* loss_mean,
                                              float weight, float tau, float* con_loss, int64_t B,
                                              int64_t D, int64_t H, int64_t C, void* workspace, size_t workspace_bytes,
                                              void* stream) {
    if (!con_loss) return DBMM_E_ARG;
    return train_step_impl(x, labels, {w1, b1, gamma, beta, rmean, rvar, (long long*)nbt, w2, b2}, {m_w1, m_b1, m_gamma, m_beta, m_w2, m_b2},
                           {o_w1, o_b1, o_gamma, o_beta, o_rmean, o_rvar, (long long*)o_nbt, o_w2, o_b2}, ebd_weight, tn, temperature,
                           {lr, momentum, weight_decay, first_step}, logits, loss_rows, loss_mean, {}, {weight, tau, con_loss}, B, D, H, C, workspace,
                           workspace_bytes, stream);
}

// ---- one call = one step of the contrastive adapter on sampled sets (supcon_sets.hip) ----------------------------
// workspace: the step's (no frozen adapter, no inv_norm) | the head's, B = T*S
extern "C" size_t dbmm_workspace_bytes_adapter_train_step_sets(int64_t T, int64_t S, int64_t D, int64_t H) {
    const size_t head = dbmm_supcon_sets_workspace_bytes(T, S, D);
    if (!head || H <= 0 || (H & 3)) return 0;
    return step_ws(T * S, D, H, false, false).total * sizeof(float) + head;
}

extern "C" int dbmm_adapter_train_step_sets(const float* x, float* w1, float* b1, float* gamma, float* beta, float* rmean, float* rvar,
                                            int64_t* nbt, float* w2, float* b2, float* m_w1, float* m_b1, float* m_gamma, float* m_beta,
                                            float* m_w2, float* m_b2, float lr, float momentum, float weight_decay, int first_step,
                                            float scale, float tau, float* loss, float* loss_sets, int64_t T, int64_t A, int64_t P,
                                            int64_t N, int64_t D, int64_t H, void* workspace, size_t workspace_bytes, void* stream) {
    const AdapterParams p{w1, b1, gamma, beta, rmean, rvar, (long long*)nbt, w2, b2};
    const AdapterMomentum m{m_w1, m_b1, m_gamma, m_beta, m_w2, m_b2};
    if (!x || !complete(p.forward_only()) || !complete(m) || !loss || !loss_sets || !workspace) return DBMM_E_ARG;
    if (T < 1 || A < 1 || P < 1 || N < 1 || D <= 0 || H <= 0 || (D & 3) || (H & 3) || !(tau > 0.f) || T > 65535 || A > INT32_MAX ||
        P > INT32_MAX || N > INT32_MAX || T * (A + P + N) > INT32_MAX)
        return DBMM_E_SHAPE;
    const int64_t S = A + P + N, B = T * S;
    if (!dbmm_adapter_fast_shape(B, D, H) || !dbmm_opt(OPT_ADAPTER_STEP_FUSED) || !dbmm_aligned16(x)) return DBMM_E_UNSUPPORTED;
    const size_t head_bytes = dbmm_supcon_sets_workspace_bytes(T, S, D);
    if (!head_bytes) return DBMM_E_UNSUPPORTED;
    const StepWs L = step_ws(B, D, H, false, false);
    const size_t step_bytes = L.total * sizeof(float);
    if (workspace_bytes < step_bytes + head_bytes) return DBMM_E_WORKSPACE;
    if (!dbmm_aligned16(workspace)) return DBMM_E_ALIGN;
    float* f = (float*)workspace;
    int rc = fwd_train(x, p.forward_only(), f, L.a, B, D, H, stream);
    if (rc) return rc;
    rc = head_sets(f + L.a.z, f + L.dz, scale, tau, loss, loss_sets, T, A, P, N, D, (char*)workspace + step_bytes, head_bytes, stream);
    if (rc) return rc;
    return bwd_sgd(x, p, m, {lr, momentum, weight_decay, first_step}, f, L, true, nullptr, nullptr, B, D, H, stream);
}

extern "C" int dbmm_version(void) { return 101; }

extern "C" const char* dbmm_error_string(int code) {
    switch (code) {
        case DBMM_OK: return "ok";
        case DBMM_E_SHAPE: return "unsupported or inconsistent dimensions";
        case DBMM_E_ALIGN: return "pointer or leading dimension not 16-byte aligned";
        case DBMM_E_WORKSPACE: return "workspace too small";
        case DBMM_E_ARG: return "null pointer or bad enum";
        case DBMM_E_UNSUPPORTED: return "no kernel for this (valid) request; use the unfused calls";
        default: return code > 0 ? hipGetErrorString((hipError_t)code) : "unknown dbmm error";
    }
}
