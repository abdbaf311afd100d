// The GEMM-shaped parts of the debiasing-adapter step (final_main.py:160-174 forward, its backward, 455-466 step body)
// for the reference's shapes: hidden width H = 128 (final_main.py:241), D = 512 / 768 / 1024, a batch of 4 ... 8192 rows.
//
// At B = 256 the whole step is 0.34 GFLOP and 7 MB: nothing in it is throughput-bound, the step is latency- and launch-
// bound.  Through the general implicit-GEMM kernel its five products ran as grids of 8 - 64 tiles with K loops of up to
// 64 barrier-separated chunks: 95 of the step's 135 us (rocprofv3, tools/bench_adapter_step.py).  These kernels cut every
// product so that >= 64 workgroups work on it, fuse what is elementwise into the product that consumes it, and keep
// every sum in a fixed order (no atomics): results do not depend on the launch geometry's timing and the one-call step
// equals the autograd path bit for bit (both run these kernels).
//
//   fc1_partial      hpart[ks][b][:] = x[b][128 ks : 128 ks + 128] . W1[:, same]^T     grid (B / 32, 2, D / 128); the partials
//                    live in the z buffer (B x D floats = D / 128 slices of B x 128), which is written later
//   bn_stats         h = b1 + sum_ks hpart (fixed order), column mean / biased variance over the batch (two passes),
//                    running statistics with the unbiased variance, num_batches_tracked          grid H / 4
//   fc2              r = relu(bn(h)) (stored for the backward), z = r . W2^T + b2                grid (B / 32, D / 64)
//   bwd2             dW2 = dz^T r, db2 = colsum dz (blocks < D / 32) and drpart[ks] = dz[:, slice ks] . W2[slice ks]
//                    (the other blocks) in ONE launch: both only need dz, r and W2
//   bn_bwd           dr = sum_ks drpart, dhn = dr * (bn(h) > 0), dbeta / dgamma column sums, dh                  grid H / 4
//   bwd1             dW1 = dh^T x, db1 = colsum dh                                                 grid D / 32
//
// All fp32 on the vector ALUs (exact fp32 products, like the fp32-input MFMA the general kernel uses): a 32 x 128 output
// tile per workgroup, 4 x 4 register tiles, operands through LDS rows padded to 132 floats (16-B aligned, conflict-free
// ds_read_b128 for 16 consecutive rows).  Bound: launch latency (1.2 us of HBM time at B = 256).
//
// The kernels' bodies live in adapter_bodies.inc (device functions shared with the replica-batched kernels of adapter_sweep.hip); the
// __global__ kernels below keep their names and grids and call them with their own blockIdx / gridDim.
#include "adapter_step.h"

namespace {

#include "adapter_bodies.inc"

__global__ __launch_bounds__(256) void fc1_partial_kernel(const float* __restrict__ x, const float* __restrict__ w1, float* __restrict__ part,
                                                          int B, int D) {
    fc1_partial_body<false>(blockIdx, gridDim, x, nullptr, 0, w1, part, B, D);
}

__global__ __launch_bounds__(256) void bn_stats_kernel(const float* __restrict__ part, int KS, const float* __restrict__ b1, float* __restrict__ h,
                                                       int B, float eps, float momentum, float* __restrict__ mean_o, float* __restrict__ invstd_o,
                                                       float* __restrict__ rmean, float* __restrict__ rvar, long long* __restrict__ nbt) {
    bn_stats_body(blockIdx, gridDim, part, KS, b1, h, B, eps, momentum, mean_o, invstd_o, rmean, rvar, nbt);
}

__global__ __launch_bounds__(256) void fc1_reduce_kernel(const float* __restrict__ part, int KS, const float* __restrict__ b1, float* __restrict__ h,
                                                         long long total, int B) {
    fc1_reduce_body(blockIdx, gridDim, part, KS, b1, h, total, B);
}

__global__ __launch_bounds__(256) void fc2_kernel(const float* __restrict__ h, const float* __restrict__ mean, const float* __restrict__ invstd,
                                                  int var_mode, float eps, const float* __restrict__ gamma, const float* __restrict__ beta,
                                                  const float* __restrict__ w2, const float* __restrict__ b2, float* __restrict__ r,
                                                  float* __restrict__ z, int B, int D) {
    fc2_body(blockIdx, gridDim, h, mean, invstd, var_mode, eps, gamma, beta, w2, b2, r, z, B, D);
}

__global__ __launch_bounds__(256) void bwd2_kernel(const float* __restrict__ dz, const float* __restrict__ r, const float* __restrict__ w2,
                                                   float* __restrict__ dw2part, float* __restrict__ db2part, float* __restrict__ drpart, int B, int D,
                                                   int NS, int RB, const float* __restrict__ loss_rows, float* __restrict__ loss_mean) {
    bwd2_body(blockIdx, gridDim, dz, r, w2, dw2part, db2part, drpart, B, D, NS, RB, loss_rows, loss_mean);
}

// the weighted step's first backward launch: bwd2_kernel's blocks, and the spare block writes the WEIGHTED mean of loss_rows
__global__ __launch_bounds__(256) void bwd2_rows_kernel(const float* __restrict__ dz, const float* __restrict__ r, const float* __restrict__ w2,
                                                        float* __restrict__ dw2part, float* __restrict__ db2part, float* __restrict__ drpart, int B, int D,
                                                        int NS, int RB, const float* __restrict__ loss_rows, const float* __restrict__ row_w,
                                                        float* __restrict__ loss_mean) {
    __shared__ float red[4];
    if (blockIdx.x == gridDim.x - 1) {
        weighted_mean_body(loss_rows, row_w, nullptr, 0, B, red, loss_mean);
        return;
    }
    bwd2_body(blockIdx, gridDim, dz, r, w2, dw2part, db2part, drpart, B, D, NS, RB, nullptr, nullptr);
}

__global__ __launch_bounds__(256) void bn_bwd_kernel(const float* __restrict__ drpart, int KS, const float* __restrict__ h, const float* __restrict__ mean,
                                                     const float* __restrict__ invstd, const float* __restrict__ gamma, const float* __restrict__ beta,
                                                     float* __restrict__ dgamma, float* __restrict__ dbeta, float* __restrict__ dh, int B,
                                                     const float* __restrict__ dw2part, float* __restrict__ dw2, long long nw4,
                                                     const float* __restrict__ db2part, float* __restrict__ db2, long long nb4, int NS) {
    bn_bwd_body(blockIdx, gridDim, drpart, KS, h, mean, invstd, gamma, beta, dgamma, dbeta, dh, B, dw2part, dw2, nw4, db2part, db2, nb4, NS);
}

__global__ __launch_bounds__(256) void bwd1_kernel(const float* __restrict__ dh, const float* __restrict__ x, float* __restrict__ dw1part,
                                                   float* __restrict__ db1part, int B, int D, int RB) {
    bwd1_body<false>(blockIdx, gridDim, dh, x, nullptr, 0, dw1part, db1part, B, D, RB);
}

__global__ __launch_bounds__(256) void grad_reduce_kernel(const float* __restrict__ pa, float* __restrict__ oa, long long na4,
                                                          const float* __restrict__ pb, float* __restrict__ ob, long long nb4, int NS) {
    grad_reduce_body(blockIdx, gridDim, pa, oa, na4, pb, ob, nb4, NS);
}

}  // namespace

// ---- launchers (adapter_ops.hip composes dbmm_adapter_fwd / dbmm_adapter_bwd from them) -----------------------------------
bool dbmm_adapter_fast_shape(int64_t B, int64_t D, int64_t H) { return H == 128 && D >= 128 && (D % 128) == 0 && B >= 2 && B <= (1 << 20); }

int dbmm_adapter_fwd_fast(const float* x, const float* w1, const float* b1, const float* gamma, const float* beta, float* running_mean,
                          float* running_var, int64_t* nbt, const float* w2, const float* b2, float* h, float* mean, float* invstd, float* r,
                          float* z, int64_t B, int64_t D, int train, float eps, float momentum, hipStream_t s) {
    const int KS = (int)(D / 128), nb = (int)((B + 31) / 32);
    hipLaunchKernelGGL(fc1_partial_kernel, dim3(nb, 2, KS), dim3(256), 0, s, x, w1, z, (int)B, (int)D);
    DBMM_CHECK_LAUNCH();
    if (train) {
        hipLaunchKernelGGL(bn_stats_kernel, dim3(32), dim3(256), 0, s, (const float*)z, KS, b1, h, (int)B, eps, momentum, mean, invstd, running_mean,
                           running_var, (long long*)nbt);
    } else {
        const long long total = B * 128;
        hipLaunchKernelGGL(fc1_reduce_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, (const float*)z, KS, b1, h, total, (int)B);
    }
    DBMM_CHECK_LAUNCH();
    hipLaunchKernelGGL(fc2_kernel, dim3(nb, (unsigned)(D / 64)), dim3(256), 0, s, (const float*)h, train ? (const float*)mean : (const float*)running_mean,
                       train ? (const float*)invstd : (const float*)running_var, train ? 0 : 1, eps, gamma, beta, w2, b2, r, z, (int)B, (int)D);
    DBMM_CHECK_LAUNCH();
    return DBMM_OK;
}

int dbmm_adapter_bwd_fast(const float* x, const float* dz, const float* h, const float* mean, const float* invstd, const float* r, const float* gamma,
                          const float* beta, const float* w2, float* dw1, float* db1, float* dgamma, float* dbeta, float* dw2, float* db2,
                          float* dh, float* scratch, int64_t B, int64_t D, hipStream_t s, bool sum_dw1, const float* loss_rows, float* loss_mean,
                          const float* row_w) {
    const int KS = (int)(D / 128), nb = (int)((B + TB - 1) / TB);
    const BwdScratch L = dbmm_adapter_bwd_scratch(B, D);
    const int NS = L.NS, RB = L.RB;
    float *drpart = scratch + L.drpart, *dw2part = scratch + L.dw2part, *db2part = scratch + L.db2part, *dw1part = scratch + L.dw1part,
          *db1part = scratch + L.db1part;
    if (row_w && loss_mean)
        hipLaunchKernelGGL(bwd2_rows_kernel, dim3((unsigned)(D / 32 * NS + nb * KS + 1)), dim3(256), 0, s, dz, r, w2, dw2part, db2part, drpart, (int)B,
                           (int)D, NS, RB, loss_rows, row_w, loss_mean);
    else
        hipLaunchKernelGGL(bwd2_kernel, dim3((unsigned)(D / 32 * NS + nb * KS + (loss_mean ? 1 : 0))), dim3(256), 0, s, dz, r, w2, dw2part, db2part, drpart,
                           (int)B, (int)D, NS, RB, loss_rows, loss_mean);
    DBMM_CHECK_LAUNCH();
    const long long nw4 = D * 128 / 4, nb4 = D / 4;
    hipLaunchKernelGGL(bn_bwd_kernel, dim3((unsigned)(32 + (nw4 + nb4 + 255) / 256)), dim3(256), 0, s, (const float*)drpart, KS, h, mean, invstd, gamma,
                       beta, dgamma, dbeta, dh, (int)B, (const float*)dw2part, dw2, nw4, (const float*)db2part, db2, nb4, NS);
    DBMM_CHECK_LAUNCH();
    hipLaunchKernelGGL(bwd1_kernel, dim3((unsigned)(D / 32), NS), dim3(256), 0, s, (const float*)dh, x, dw1part, db1part, (int)B, (int)D, RB);
    DBMM_CHECK_LAUNCH();
    if (!sum_dw1) return DBMM_OK;
    hipLaunchKernelGGL(grad_reduce_kernel, dim3((unsigned)((nw4 + 32 + 255) / 256)), dim3(256), 0, s, (const float*)dw1part, dw1, nw4,
                       (const float*)db1part, db1, 32LL, NS);
    DBMM_CHECK_LAUNCH();
    return DBMM_OK;
}
