// Replica-batched adapter step and evaluation forward: R independent runs of one sweep group (same schedule, different seed and
// possibly learning rate) advance in lock-step and share every launch.  The step is launch-bound (adapter_step.hip: the same 8
// launches take 65 us at 256 rows and 45 us at 4), so R replicas in one launch cost about what one costs: the replica is one more
// grid dimension and every operand is `base + r * stride` into stacked tensors ([R, ...] contiguous) and a per-replica workspace.
//
// Every kernel here is a wrapper around a device body of adapter_bodies.inc -- the bodies the single-run kernels call -- with the
// block coordinates of the single-run launch, so replica r gets the bits dbmm_adapter_train_step gives for r alone.  What is new:
//   * the batch of replica r is rows idx[r][b] of ONE shared embedding table, read in place by fc1 and bwd1 (rows are 16-B aligned:
//     D % 4 == 0), labels / groups are read as labels[idx[r][b]]: no gathered [R, B, D] copy exists;
//   * the CE launch also adds the (n, correct) group counters (integer atomics: order-free), the launch that computes the batch
//     loss mean adds `(double)loss_mean * B` to the replica's float64 epoch loss sum (one thread, one add per step);
//   * the per-replica learning rates reach the SGD launch by value.
// Launches of a step: fc1 partials, BN statistics, fc2 [the same three for a frozen old adapter], CE forward + backward, bwd2,
// BN backward, bwd1, SGD = 8 (11), whatever R is; the group-DRO step (dbmm_adapter_sweep_step_gdro) has CE forward, group weights +
// q update, weighted CE backward in place of the one CE launch = 10 (13); the step under per-row loss weights
// (dbmm_adapter_sweep_step_weighted) has the ERM step's 8 (11).  Evaluation: fc1 partials, reduce, fc2 [x 2], CE forward, loss sum = 5 (8).
// No float atomics, no order that depends on timing.
#include "adapter_step.h"

namespace {

#include "adapter_bodies.inc"

constexpr int MAXR = 16;

template <bool GATHER>
__global__ __launch_bounds__(256) void sweep_fc1_kernel(const float* __restrict__ x, const long long* __restrict__ idx, long long idx_stride,
                                                        long long n_tab, const float* __restrict__ w1, float* __restrict__ ws, long long ws_stride,
                                                        long long zoff, int B, int D, int KS) {
    const int r = blockIdx.z / KS;
    fc1_partial_body<GATHER>(dim3(blockIdx.x, blockIdx.y, blockIdx.z % KS), dim3(gridDim.x, gridDim.y, KS), x, GATHER ? idx + r * idx_stride : nullptr,
                             n_tab, w1 + (long long)r * 128 * D, ws + r * ws_stride + zoff, B, D);
}

__global__ __launch_bounds__(256) void sweep_bn_stats_kernel(float* __restrict__ ws, long long ws_stride, long long zoff, long long hoff, long long moff,
                                                             long long ioff, int KS, const float* __restrict__ b1, int B, float eps, float momentum,
                                                             float* __restrict__ rmean, float* __restrict__ rvar, long long* __restrict__ nbt) {
    const int r = blockIdx.y;
    float* w = ws + r * ws_stride;
    bn_stats_body(dim3(blockIdx.x, 0, 0), dim3(gridDim.x, 1, 1), w + zoff, KS, b1 + r * 128, w + hoff, B, eps, momentum, w + moff, w + ioff,
                  rmean + r * 128, rvar + r * 128, nbt + r);
}

__global__ __launch_bounds__(256) void sweep_fc1_reduce_kernel(float* __restrict__ ws, long long ws_stride, long long zoff, long long hoff, int KS,
                                                               const float* __restrict__ b1, long long total, int B) {
    const int r = blockIdx.y;
    float* w = ws + r * ws_stride;
    fc1_reduce_body(dim3(blockIdx.x, 0, 0), dim3(gridDim.x, 1, 1), w + zoff, KS, b1 + r * 128, w + hoff, total, B);
}

// mean / invstd: the batch statistics in the workspace (train) or the stacked running statistics (eval, var_mode 1)
__global__ __launch_bounds__(256) void sweep_fc2_kernel(float* __restrict__ ws, long long ws_stride, long long hoff, const float* __restrict__ mean,
                                                        const float* __restrict__ invstd, long long stat_stride, int var_mode, float eps,
                                                        const float* __restrict__ gamma, const float* __restrict__ beta, const float* __restrict__ w2,
                                                        const float* __restrict__ b2, long long roff, long long zoff, int B, int D) {
    const int r = blockIdx.z;
    float* w = ws + r * ws_stride;
    fc2_body(dim3(blockIdx.x, blockIdx.y, 0), dim3(gridDim.x, gridDim.y, 1), w + hoff, mean + r * stat_stride, invstd + r * stat_stride, var_mode, eps,
             gamma + r * 128, beta + r * 128, w2 + (long long)r * D * 128, b2 + (long long)r * D, w + roff, w + zoff, B, D);
}

// update_dict of one row (group_count_kernel's argmax and comparison) into the block's LDS counters
template <int CMAX>
__device__ __forceinline__ void count_row(const float (&lg)[CMAX], int C, long long y, long long g, int G, unsigned int (*sc)[2]) {
    int am = 0;
    float mx = lg[0];
#pragma unroll
    for (int c = 1; c < CMAX; ++c)
        if (c < C && lg[c] > mx) { mx = lg[c]; am = c; }
    if (g >= 0 && g < (long long)G) {                    // the int64 id is compared: 2^32 + k is no group
        atomicAdd(&sc[g][0], 1u);
        if ((long long)am == y) atomicAdd(&sc[g][1], 1u);
    }
}
__device__ __forceinline__ void flush_counts(unsigned int (*sc)[2], unsigned long long* __restrict__ counts, int G) {
    if ((int)threadIdx.x < G) {
        if (sc[threadIdx.x][0]) atomicAdd(&counts[threadIdx.x * 2], (unsigned long long)sc[threadIdx.x][0]);
        if (sc[threadIdx.x][1]) atomicAdd(&counts[threadIdx.x * 2 + 1], (unsigned long long)sc[threadIdx.x][1]);
    }
}

// train: forward + backward of the head for row b of replica r (l2norm_sim_ce_fwdbwd_kernel's two calls) + the group counters
template <int CMAX>
__global__ __launch_bounds__(256) void sweep_ce_fwdbwd_kernel(float* __restrict__ ws, long long ws_stride, long long zoff, long long ozoff, long long dzoff,
                                                              float w_old, float w_new, const float* __restrict__ tn,
                                                              const long long* __restrict__ labels, const long long* __restrict__ groups,
                                                              const long long* __restrict__ idx, long long n_tab, float invT, float gscale,
                                                              float* __restrict__ logits, float* __restrict__ loss_rows,
                                                              unsigned long long* __restrict__ counts, int G, int B, int D4, int C) {
    __shared__ unsigned int sc[64][2];
    const int r = blockIdx.y;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (counts) {
        if (threadIdx.x < 64) { sc[threadIdx.x][0] = 0; sc[threadIdx.x][1] = 0; }
        __syncthreads();
    }
    if (row < B) {
        float* w = ws + r * ws_stride;
        const long long lrow = table_row(idx + (long long)r * B, row, n_tab);
        float lg[CMAX], inv;
        ce_fwd_row<CMAX>(w + zoff, ozoff >= 0 ? w + ozoff : nullptr, w_old, tn, labels, invT, logits + (long long)r * B * C, loss_rows + (long long)r * B,
                         nullptr, nullptr, row, lane, D4, C, lg, inv, lrow);
        ce_bwd_row<CMAX>(w + zoff, inv, w_new, tn, lg, labels, nullptr, invT, gscale, w + dzoff, row, lane, D4, C, lrow);
        if (counts && lane == 0) count_row<CMAX>(lg, C, labels[lrow], groups[lrow], G, sc);
    }
    if (counts) {
        __syncthreads();
        flush_counts(sc, counts + (long long)r * G * 2, G);
    }
}

// per-row loss weights: sweep_ce_fwdbwd_kernel with the gradient scale of row b of replica r times row_w[r * w_stride + table row of b]
// (l2norm_sim_ce_fwdbwd_rows_kernel's two calls); w_stride = 0: one weight vector shared by the replicas, else the table's rows
template <int CMAX>
__global__ __launch_bounds__(256) void sweep_ce_fwdbwd_rows_kernel(float* __restrict__ ws, long long ws_stride, long long zoff, long long ozoff,
                                                                   long long dzoff, float w_old, float w_new, const float* __restrict__ tn,
                                                                   const long long* __restrict__ labels, const long long* __restrict__ groups,
                                                                   const long long* __restrict__ idx, long long n_tab, const float* __restrict__ row_w,
                                                                   long long w_stride, float invT, float gscale, float* __restrict__ logits,
                                                                   float* __restrict__ loss_rows, unsigned long long* __restrict__ counts, int G, int B,
                                                                   int D4, int C) {
    __shared__ unsigned int sc[64][2];
    const int r = blockIdx.y;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (counts) {
        if (threadIdx.x < 64) { sc[threadIdx.x][0] = 0; sc[threadIdx.x][1] = 0; }
        __syncthreads();
    }
    if (row < B) {
        float* w = ws + r * ws_stride;
        const long long lrow = table_row(idx + (long long)r * B, row, n_tab);
        float lg[CMAX], inv;
        ce_fwd_row<CMAX>(w + zoff, ozoff >= 0 ? w + ozoff : nullptr, w_old, tn, labels, invT, logits + (long long)r * B * C, loss_rows + (long long)r * B,
                         nullptr, nullptr, row, lane, D4, C, lg, inv, lrow);
        ce_bwd_row<CMAX>(w + zoff, inv, w_new, tn, lg, labels, nullptr, invT, gscale * row_w[r * w_stride + lrow], w + dzoff, row, lane, D4, C, lrow);
        if (counts && lane == 0) count_row<CMAX>(lg, C, labels[lrow], groups[lrow], G, sc);
    }
    if (counts) {
        __syncthreads();
        flush_counts(sc, counts + (long long)r * G * 2, G);
    }
}

// group-DRO train step, first of the head's three launches: forward of row b of replica r (l2norm_sim_ce_fwd_kernel's call, 1 / ||z||
// kept for the backward) + the group counters
template <int CMAX>
__global__ __launch_bounds__(256) void sweep_ce_fwd_train_kernel(float* __restrict__ ws, long long ws_stride, long long zoff, long long ozoff,
                                                                 long long invoff, float w_old, const float* __restrict__ tn,
                                                                 const long long* __restrict__ labels, const long long* __restrict__ groups,
                                                                 const long long* __restrict__ idx, long long n_tab, float invT,
                                                                 float* __restrict__ logits, float* __restrict__ loss_rows,
                                                                 unsigned long long* __restrict__ counts, int G, int B, int D4, int C) {
    __shared__ unsigned int sc[64][2];
    const int r = blockIdx.y;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (counts) {
        if (threadIdx.x < 64) { sc[threadIdx.x][0] = 0; sc[threadIdx.x][1] = 0; }
        __syncthreads();
    }
    if (row < B) {
        float* w = ws + r * ws_stride;
        const long long lrow = table_row(idx + (long long)r * B, row, n_tab);
        float lg[CMAX], inv;
        ce_fwd_row<CMAX>(w + zoff, ozoff >= 0 ? w + ozoff : nullptr, w_old, tn, labels, invT, logits + (long long)r * B * C, loss_rows + (long long)r * B,
                         nullptr, w + invoff, row, lane, D4, C, lg, inv, lrow);
        if (counts && lane == 0) count_row<CMAX>(lg, C, labels[lrow], groups[lrow], G, sc);
    }
    if (counts) {
        __syncthreads();
        flush_counts(sc, counts + (long long)r * G * 2, G);
    }
}

// second: replica r's group reduction and q update (gdro_weights_kernel's call); loss_mean[r] = the robust loss, and the thread
// that wrote it adds it, as a double times the batch rows, to the epoch's loss sum
__global__ __launch_bounds__(256) void sweep_gdro_weights_kernel(float* __restrict__ ws, long long ws_stride, long long gwoff,
                                                                 const float* __restrict__ loss_rows, const long long* __restrict__ groups,
                                                                 const long long* __restrict__ idx, long long n_tab, float* q,
                                                                 float* __restrict__ loss_mean, double* __restrict__ loss_sum, int B, int G, float eta) {
    const int r = blockIdx.x;
    gdro_weights_body(loss_rows + (long long)r * B, groups, idx + (long long)r * B, n_tab, q + r * G, q + r * G, ws + r * ws_stride + gwoff, loss_mean + r,
                      B, G, eta);
    if (loss_sum && threadIdx.x == 0) loss_sum[r] += (double)loss_mean[r] * (double)B;
}

// third: weighted backward of row b of replica r (l2norm_sim_ce_bwd_w_kernel's call)
template <int CMAX>
__global__ __launch_bounds__(256) void sweep_ce_bwd_w_kernel(float* __restrict__ ws, long long ws_stride, long long zoff, long long invoff, long long gwoff,
                                                             long long dzoff, float w_new, const float* __restrict__ tn,
                                                             const float* __restrict__ logits, const long long* __restrict__ labels,
                                                             const long long* __restrict__ groups, const long long* __restrict__ idx, long long n_tab,
                                                             int G, float invT, int B, int D4, int C) {
    const int r = blockIdx.y;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= B) return;
    float* w = ws + r * ws_stride;
    const long long* idr = idx + (long long)r * B;
    float lgv[CMAX];
#pragma unroll
    for (int c = 0; c < CMAX; ++c) lgv[c] = (c < C) ? logits[((long long)r * B + row) * C + c] : -INFINITY;
    const int g = gdro_group(groups, idr, n_tab, row, G);
    ce_bwd_row<CMAX>(w + zoff, (w + invoff)[row], w_new, tn, lgv, labels, nullptr, invT, g >= 0 ? (w + gwoff)[g] : 0.f, w + dzoff, row, lane, D4, C,
                     table_row(idr, row, n_tab));
}

// eval: l2norm_sim_ce_fwd_kernel's call for row b of replica r + the group counters; every replica scores the same rows
template <int CMAX>
__global__ __launch_bounds__(256) void sweep_ce_fwd_kernel(float* __restrict__ ws, long long ws_stride, long long zoff, long long ozoff, float w_old,
                                                           const float* __restrict__ tn, const long long* __restrict__ labels,
                                                           const long long* __restrict__ groups, const long long* __restrict__ idx, long long n_tab,
                                                           float invT, float* __restrict__ logits, float* __restrict__ loss_rows,
                                                           unsigned long long* __restrict__ counts, int G, int B, int D4, int C) {
    __shared__ unsigned int sc[64][2];
    const int r = blockIdx.y;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (threadIdx.x < 64) { sc[threadIdx.x][0] = 0; sc[threadIdx.x][1] = 0; }
    __syncthreads();
    if (row < B) {
        float* w = ws + r * ws_stride;
        const long long lrow = idx ? table_row(idx, row, n_tab) : (long long)row;
        float lg[CMAX], inv;
        ce_fwd_row<CMAX>(w + zoff, ozoff >= 0 ? w + ozoff : nullptr, w_old, tn, labels, invT, logits + (long long)r * B * C, loss_rows + (long long)r * B,
                         nullptr, nullptr, row, lane, D4, C, lg, inv, lrow);
        if (lane == 0) count_row<CMAX>(lg, C, labels[lrow], groups[lrow], G, sc);
    }
    __syncthreads();
    flush_counts(sc, counts + (long long)r * G * 2, G);
}

// eval: loss_sum[r] += sum_b (double)loss_rows[r][b], in a fixed order (thread-strided partial sums, then an LDS tree)
__global__ __launch_bounds__(256) void sweep_loss_sum_kernel(const float* __restrict__ loss_rows, double* __restrict__ loss_sum, int B) {
    __shared__ double red[256];
    const int r = blockIdx.x;
    double s = 0.0;
    for (int b = threadIdx.x; b < B; b += 256) s += (double)loss_rows[(long long)r * B + b];
    red[threadIdx.x] = s;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) loss_sum[r] += red[0];
}

__global__ __launch_bounds__(256) void sweep_bwd2_kernel(float* __restrict__ ws, long long ws_stride, long long dzoff, long long roff,
                                                         const float* __restrict__ w2, long long dw2p, long long db2p, long long drp, int B, int D, int NS,
                                                         int RB, const float* __restrict__ loss_rows, float* __restrict__ loss_mean,
                                                         double* __restrict__ loss_sum) {
    const int r = blockIdx.y;
    float* w = ws + r * ws_stride;
    bwd2_body(dim3(blockIdx.x, 0, 0), dim3(gridDim.x, 1, 1), w + dzoff, w + roff, w2 + (long long)r * D * 128, w + dw2p, w + db2p, w + drp, B, D, NS, RB,
              loss_rows + (long long)r * B, loss_mean ? loss_mean + r : nullptr);
    // losses.update(loss.item(), bsz) on the device: the thread that wrote the mean adds it, as a double times the batch rows
    if (loss_sum && blockIdx.x == gridDim.x - 1 && threadIdx.x == 0) loss_sum[r] += (double)loss_mean[r] * (double)B;
}

// per-row loss weights: sweep_bwd2_kernel whose spare block writes replica r's WEIGHTED loss mean (bwd2_rows_kernel's statements, the
// weight of batch row b read at its table row) and counts it as sweep_bwd2_kernel counts the mean
__global__ __launch_bounds__(256) void sweep_bwd2_rows_kernel(float* __restrict__ ws, long long ws_stride, long long dzoff, long long roff,
                                                              const float* __restrict__ w2, long long dw2p, long long db2p, long long drp, int B, int D,
                                                              int NS, int RB, const float* __restrict__ loss_rows, const float* __restrict__ row_w,
                                                              long long w_stride, const long long* __restrict__ idx, long long n_tab,
                                                              float* __restrict__ loss_mean, double* __restrict__ loss_sum) {
    __shared__ float red[4];
    const int r = blockIdx.y;
    if (blockIdx.x == gridDim.x - 1) {
        weighted_mean_body(loss_rows + (long long)r * B, row_w + r * w_stride, idx + (long long)r * B, n_tab, B, red, loss_mean + r);
        if (loss_sum && threadIdx.x == 0) loss_sum[r] += (double)loss_mean[r] * (double)B;
        return;
    }
    float* w = ws + r * ws_stride;
    bwd2_body(dim3(blockIdx.x, 0, 0), dim3(gridDim.x, 1, 1), w + dzoff, w + roff, w2 + (long long)r * D * 128, w + dw2p, w + db2p, w + drp, B, D, NS, RB,
              nullptr, nullptr);
}

__global__ __launch_bounds__(256) void sweep_bn_bwd_kernel(float* __restrict__ ws, long long ws_stride, long long drp, int KS, long long hoff,
                                                           long long moff, long long ioff, const float* __restrict__ gamma,
                                                           const float* __restrict__ beta, long long dgoff, long long dboff, long long dhoff, int B,
                                                           long long dw2p, long long dw2off, long long nw4, long long db2p, long long db2off,
                                                           long long nb4, int NS) {
    const int r = blockIdx.y;
    float* w = ws + r * ws_stride;
    bn_bwd_body(dim3(blockIdx.x, 0, 0), dim3(gridDim.x, 1, 1), w + drp, KS, w + hoff, w + moff, w + ioff, gamma + r * 128, beta + r * 128, w + dgoff,
                w + dboff, w + dhoff, B, w + dw2p, w + dw2off, nw4, w + db2p, w + db2off, nb4, NS);
}

__global__ __launch_bounds__(256) void sweep_bwd1_kernel(float* __restrict__ ws, long long ws_stride, long long dhoff, const float* __restrict__ x,
                                                         const long long* __restrict__ idx, long long n_tab, long long dw1p, long long db1p, int B, int D,
                                                         int RB) {
    const int r = blockIdx.z;
    float* w = ws + r * ws_stride;
    bwd1_body<true>(dim3(blockIdx.x, blockIdx.y, 0), dim3(gridDim.x, gridDim.y, 1), w + dhoff, x, idx + (long long)r * B, n_tab, w + dw1p, w + db1p, B, D,
                    RB);
}

// tensor t = blockIdx.y of replica r = blockIdx.z: stacked parameter / momentum tensors, gradients in the replica's workspace
struct SweepSgdArgs {
    float* p[6];
    float* m[6];
    long long g[6];        // offset of the gradient (or of its partial sums) in a replica's workspace
    long long n[6];
    int ns[6];
    float lr[MAXR];
};
__global__ __launch_bounds__(256) void sweep_sgd_kernel(const SweepSgdArgs a, const float* __restrict__ ws, long long ws_stride, float mu, float wd,
                                                        int first) {
    const int t = blockIdx.y, r = blockIdx.z;
    const long long n = a.n[t];
    float lr = a.lr[0];
#pragma unroll
    for (int i = 1; i < MAXR; ++i)
        if (i == r) lr = a.lr[i];                 // by-value array, selected without indexing it dynamically (keeps it out of scratch memory)
    sgd_body(dim3(blockIdx.x, 0, 0), dim3(gridDim.x, 1, 1), a.p[t] + r * n, ws + r * ws_stride + a.g[t], a.m[t] + r * n, n, a.ns[t], lr, mu, wd, first);
}

inline size_t up4(size_t n) { return (n + 3) / 4 * 4; }

// per-replica workspace of a step, in floats (every region a multiple of 4 floats: 16-B aligned)
struct StepLayout {
    long long h, r, z, mean, invstd, oh, orr, oz, omean, oinv, dz, dgamma, dbeta, dw2, db2, dh, scratch, total;
};
StepLayout step_layout(int64_t B, int64_t D, int with_old) {
    StepLayout L{};
    long long f = 0;
    auto take = [&](size_t n) { const long long o = f; f += (long long)up4(n); return o; };
    L.h = take(B * 128); L.r = take(B * 128); L.z = take(B * D); L.mean = take(128); L.invstd = take(128);
    L.oh = L.orr = L.oz = L.omean = L.oinv = -1;
    if (with_old) { L.oh = take(B * 128); L.orr = take(B * 128); L.oz = take(B * D); L.omean = take(128); L.oinv = take(128); }
    L.dz = take(B * D); L.dgamma = take(128); L.dbeta = take(128); L.dw2 = take(D * 128); L.db2 = take(D); L.dh = take(B * 128);
    L.scratch = take(dbmm_adapter_bwd_scratch(B, D).total);
    L.total = f;
    return L;
}
struct EvalLayout {
    long long h, r, z, oh, orr, oz, total;
};
EvalLayout eval_layout(int64_t B, int64_t D, int with_old) {
    EvalLayout L{};
    long long f = 0;
    auto take = [&](size_t n) { const long long o = f; f += (long long)up4(n); return o; };
    L.h = take(B * 128); L.r = take(B * 128); L.z = take(B * D);
    L.oh = L.orr = L.oz = -1;
    if (with_old) { L.oh = take(B * 128); L.orr = take(B * 128); L.oz = take(B * D); }
    L.total = f;
    return L;
}

bool stack_ok(void* const* p) {
    if (!p) return false;
    for (int i = 0; i < 9; ++i)
        if (!p[i]) return false;
    return true;
}
bool stack_aligned(void* const* p) {
    for (int i = 0; i < 9; ++i)
        if (i != 6 && !dbmm_aligned16(p[i])) return false;
    return true;
}
AdapterParams stack_of(void* const* p) {                 // the nine stacked tensors of R adapters
    return AdapterParams{(float*)p[0], (float*)p[1], (float*)p[2], (float*)p[3], (float*)p[4], (float*)p[5], (long long*)p[6], (float*)p[7], (float*)p[8]};
}

// shapes the replica-batched kernels serve: the fast shape of the single step, R replicas on the grid
int sweep_shape(int64_t R, int64_t B, int64_t D, int64_t H, int64_t C, int64_t G, int64_t n_rows, int64_t min_B) {
    if (R < 1 || R > MAXR) return DBMM_E_SHAPE;
    if (B < min_B || D <= 0 || H <= 0 || (D & 3) || (H & 3) || C <= 0 || C > 8 || G <= 0 || G > 64 || n_rows <= 0) return DBMM_E_SHAPE;
    if (!dbmm_adapter_fast_shape(B < 2 ? 2 : B, D, H)) return DBMM_E_UNSUPPORTED;
    if ((D / 128) * R > 65535 || (D / 64) > 65535) return DBMM_E_SHAPE;
    return DBMM_OK;
}

}  // namespace

extern "C" size_t dbmm_workspace_bytes_adapter_sweep_step(int64_t R, int64_t B, int64_t D, int64_t H, int with_old) {
    if (R < 1 || R > MAXR || B < 2 || !dbmm_adapter_fast_shape(B, D, H)) return 0;
    return (size_t)R * (size_t)step_layout(B, D, with_old).total * sizeof(float);
}

extern "C" size_t dbmm_workspace_bytes_adapter_sweep_eval(int64_t R, int64_t B, int64_t D, int64_t H, int with_old) {
    if (R < 1 || R > MAXR || B < 1 || !dbmm_adapter_fast_shape(B < 2 ? 2 : B, D, H)) return 0;
    return (size_t)R * (size_t)eval_layout(B, D, with_old).total * sizeof(float);
}

// `q` given: the group-DRO step of every replica (q [R][G] updated in place, loss_mean = the robust losses); `row_w` given: the step
// under per-row loss weights [Rw][n_rows] over the table's rows, Rw = 1 (shared) or R; else the ERM step
static int sweep_step_impl(const float* table, int64_t n_rows, const int64_t* idx, int64_t idx_R, int64_t idx_B, const int64_t* labels,
                           const int64_t* groups, void* const* params, float* const* bufs, void* const* old, float ebd_weight,
                           const float* tn, float temperature, const float* lr, float momentum, float weight_decay, int first_step,
                           float* logits, float* loss_rows, float* loss_mean, int64_t* counts, double* loss_sum, int64_t G, int counted,
                           float* q, float eta, int64_t R, int64_t B, int64_t D, int64_t H, int64_t C, void* workspace, size_t workspace_bytes,
                           void* stream, const float* row_w = nullptr, int64_t Rw = 0) {
    if (!table || !idx || !labels || !groups || !tn || !lr || !logits || !loss_rows || !loss_mean || !counts || !loss_sum || !workspace || !bufs)
        return DBMM_E_ARG;
    if (!stack_ok(params) || (old && !stack_ok(old))) return DBMM_E_ARG;
    for (int i = 0; i < 6; ++i)
        if (!bufs[i]) return DBMM_E_ARG;
    int rc = sweep_shape(R, B, D, H, C, G, n_rows, 2);               // B < 2: train-mode BatchNorm1d has no statistics, as in the single step
    if (rc) return rc;
    if (idx_R != R || idx_B != B) return DBMM_E_SHAPE;
    if (row_w && Rw != 1 && Rw != R) return DBMM_E_SHAPE;
    const long long w_stride = (row_w && Rw != 1) ? (long long)n_rows : 0;
    const int with_old = old != nullptr;
    if (workspace_bytes < dbmm_workspace_bytes_adapter_sweep_step(R, B, D, H, with_old)) return DBMM_E_WORKSPACE;
    if (!dbmm_aligned16(workspace) || !dbmm_aligned16(table) || !dbmm_aligned16(tn) || !stack_aligned(params) || (old && !stack_aligned(old)))
        return DBMM_E_ALIGN;
    for (int i = 0; i < 6; ++i)
        if (!dbmm_aligned16(bufs[i])) return DBMM_E_ALIGN;
    hipStream_t s = (hipStream_t)stream;
    const StepLayout L = step_layout(B, D, with_old);
    float* ws = (float*)workspace;
    const long long wst = L.total;
    const AdapterParams P = stack_of(params);
    const int KS = (int)(D / 128), nb = (int)((B + 31) / 32), iR = (int)R, iB = (int)B, iD = (int)D;
    const float eps = 1e-5f, bn_momentum = 0.1f;
    const long long* idxl = (const long long*)idx;

    for (int pass = 0; pass < 1 + with_old; ++pass) {                 // the trainable adapter, then the frozen one (train-mode BatchNorm too)
        const AdapterParams A = pass ? stack_of(old) : P;
        const long long zo = pass ? L.oz : L.z, ho = pass ? L.oh : L.h, mo = pass ? L.omean : L.mean, io = pass ? L.oinv : L.invstd,
                        ro = pass ? L.orr : L.r;
        hipLaunchKernelGGL(sweep_fc1_kernel<true>, dim3(nb, 2, KS * iR), dim3(256), 0, s, table, idxl, (long long)B, (long long)n_rows,
                           (const float*)A.w1, ws, wst, zo, iB, iD, KS);
        DBMM_CHECK_LAUNCH();
        hipLaunchKernelGGL(sweep_bn_stats_kernel, dim3(32, iR), dim3(256), 0, s, ws, wst, zo, ho, mo, io, KS, (const float*)A.b1, iB, eps, bn_momentum,
                           A.rmean, A.rvar, A.nbt);
        DBMM_CHECK_LAUNCH();
        hipLaunchKernelGGL(sweep_fc2_kernel, dim3(nb, (unsigned)(D / 64), iR), dim3(256), 0, s, ws, wst, ho, (const float*)(ws + mo),
                           (const float*)(ws + io), wst, 0, eps, (const float*)A.gamma, (const float*)A.beta, (const float*)A.w2, (const float*)A.b2, ro, zo,
                           iB, iD);
        DBMM_CHECK_LAUNCH();
    }
    const float w_new = with_old ? (1.f - ebd_weight) : 1.f, invT = 1.f / temperature;
    unsigned long long* cnt = counted ? (unsigned long long*)counts : nullptr;
    const dim3 grid((unsigned)((B + 3) / 4), iR);
    const long long* lab = (const long long*)labels;
    const long long* grp = (const long long*)groups;
    if (q) {
        // group DRO: forward rows, group reduction + q update (one workgroup per replica), weighted backward rows.  1 / ||z|| and the
        // [3][G] statistics live in the dh region, which nothing uses before the BatchNorm backward
        const long long invoff = L.dh, gwoff = L.dh + (long long)up4(B);
        dbmm_with_cmax(C, [&](auto cm) {
            hipLaunchKernelGGL(sweep_ce_fwd_train_kernel<decltype(cm)::value>, grid, dim3(256), 0, s, ws, wst, L.z, L.oz, invoff, ebd_weight, tn, lab,
                               grp, idxl, (long long)n_rows, invT, logits, loss_rows, cnt, (int)G, iB, (int)(D / 4), (int)C);
        });
        DBMM_CHECK_LAUNCH();
        hipLaunchKernelGGL(sweep_gdro_weights_kernel, dim3(iR), dim3(256), 0, s, ws, wst, gwoff, (const float*)loss_rows, grp, idxl, (long long)n_rows, q,
                           loss_mean, counted ? loss_sum : nullptr, iB, (int)G, eta);
        DBMM_CHECK_LAUNCH();
        dbmm_with_cmax(C, [&](auto cm) {
            hipLaunchKernelGGL(sweep_ce_bwd_w_kernel<decltype(cm)::value>, grid, dim3(256), 0, s, ws, wst, L.z, invoff, gwoff, L.dz, w_new, tn,
                               (const float*)logits, lab, grp, idxl, (long long)n_rows, (int)G, invT, iB, (int)(D / 4), (int)C);
        });
        DBMM_CHECK_LAUNCH();
    } else if (row_w) {
        dbmm_with_cmax(C, [&](auto cm) {
            hipLaunchKernelGGL(sweep_ce_fwdbwd_rows_kernel<decltype(cm)::value>, grid, dim3(256), 0, s, ws, wst, L.z, L.oz, L.dz, ebd_weight, w_new, tn,
                               lab, grp, idxl, (long long)n_rows, row_w, w_stride, invT, 1.f / (float)B, logits, loss_rows, cnt, (int)G, iB, (int)(D / 4),
                               (int)C);
        });
        DBMM_CHECK_LAUNCH();
    } else {
        dbmm_with_cmax(C, [&](auto cm) {
            hipLaunchKernelGGL(sweep_ce_fwdbwd_kernel<decltype(cm)::value>, grid, dim3(256), 0, s, ws, wst, L.z, L.oz, L.dz, ebd_weight, w_new, tn, lab,
                               grp, idxl, (long long)n_rows, invT, 1.f / (float)B, logits, loss_rows, cnt, (int)G, iB, (int)(D / 4), (int)C);
        });
        DBMM_CHECK_LAUNCH();
    }
    // the single step's backward (dbmm_adapter_bwd_fast) with its scratch at L.scratch: dr partials | dW2, db2, dW1, db1 partials
    const BwdScratch S = dbmm_adapter_bwd_scratch(B, D);
    const int NS = S.NS, RB = S.RB;
    const long long drp = L.scratch + S.drpart, dw2p = L.scratch + S.dw2part, db2p = L.scratch + S.db2part, dw1p = L.scratch + S.dw1part,
                    db1p = L.scratch + S.db1part;
    const int nbT = (int)((B + TB - 1) / TB);
    // (group DRO: the robust loss is already written and counted, so the spare loss-mean block is not launched)
    if (row_w)
        hipLaunchKernelGGL(sweep_bwd2_rows_kernel, dim3((unsigned)(D / 32 * NS + nbT * KS + 1), iR), dim3(256), 0, s, ws, wst, L.dz, L.r, (const float*)P.w2,
                           dw2p, db2p, drp, iB, iD, NS, RB, (const float*)loss_rows, row_w, w_stride, idxl, (long long)n_rows, loss_mean,
                           counted ? loss_sum : nullptr);
    else
        hipLaunchKernelGGL(sweep_bwd2_kernel, dim3((unsigned)(D / 32 * NS + nbT * KS + (q ? 0 : 1)), iR), dim3(256), 0, s, ws, wst, L.dz, L.r,
                           (const float*)P.w2, dw2p, db2p, drp, iB, iD, NS, RB, (const float*)loss_rows, q ? nullptr : loss_mean,
                           (counted && !q) ? loss_sum : nullptr);
    DBMM_CHECK_LAUNCH();
    const long long nw4 = D * 128 / 4, nb4 = D / 4;
    hipLaunchKernelGGL(sweep_bn_bwd_kernel, dim3((unsigned)(32 + (nw4 + nb4 + 255) / 256), iR), dim3(256), 0, s, ws, wst, drp, KS, L.h, L.mean, L.invstd,
                       (const float*)P.gamma, (const float*)P.beta, L.dgamma, L.dbeta, L.dh, iB, dw2p, L.dw2, nw4, db2p, L.db2, nb4, NS);
    DBMM_CHECK_LAUNCH();
    hipLaunchKernelGGL(sweep_bwd1_kernel, dim3((unsigned)(D / 32), NS, iR), dim3(256), 0, s, ws, wst, L.dh, table, idxl, (long long)n_rows, dw1p, db1p, iB,
                       iD, RB);
    DBMM_CHECK_LAUNCH();
    SweepSgdArgs a{};
    float* ps[6] = {P.w1, P.b1, P.gamma, P.beta, P.w2, P.b2};
    const long long go[6] = {dw1p, db1p, L.dgamma, L.dbeta, L.dw2, L.db2};
    const long long ns[6] = {128 * D, 128, 128, 128, D * 128, D};
    long long mx = 0;
    for (int i = 0; i < 6; ++i) {
        a.p[i] = ps[i]; a.m[i] = bufs[i]; a.g[i] = go[i]; a.n[i] = ns[i]; a.ns[i] = i < 2 ? NS : 1;
        if (ns[i] > mx) mx = ns[i];
    }
    for (int i = 0; i < MAXR; ++i) a.lr[i] = i < R ? lr[i] : 0.f;
    long long bx = (mx + 1023) / 1024;                                // sgd_impl's grid: the elements a thread updates are the same
    if (bx > 1024) bx = 1024;
    hipLaunchKernelGGL(sweep_sgd_kernel, dim3((unsigned)bx, 6, iR), dim3(256), 0, s, a, (const float*)ws, wst, momentum, weight_decay, first_step);
    DBMM_CHECK_LAUNCH();
    return DBMM_OK;
}

extern "C" int dbmm_adapter_sweep_step(const float* table, int64_t n_rows, const int64_t* idx, int64_t idx_R, int64_t idx_B, const int64_t* labels,
                                       const int64_t* groups, void* const* params, float* const* bufs, void* const* old, float ebd_weight,
                                       const float* tn, float temperature, const float* lr, float momentum, float weight_decay, int first_step,
                                       float* logits, float* loss_rows, float* loss_mean, int64_t* counts, double* loss_sum, int64_t G, int counted,
                                       int64_t R, int64_t B, int64_t D, int64_t H, int64_t C, void* workspace, size_t workspace_bytes, void* stream) {
    return sweep_step_impl(table, n_rows, idx, idx_R, idx_B, labels, groups, params, bufs, old, ebd_weight, tn, temperature, lr, momentum, weight_decay,
                           first_step, logits, loss_rows, loss_mean, counts, loss_sum, G, counted, nullptr, 0.f, R, B, D, H, C, workspace, workspace_bytes,
                           stream);
}

// the ERM step of every replica under per-row loss weights row_w [Rw][n_rows] (fp32, over the TABLE's rows; Rw = 1: shared by the
// replicas, Rw = R: one vector each): batch row b of replica r weighs row_w[(Rw == 1 ? 0 : r) * n_rows + idx[r][b] clamped].  The
// workspace and launches of dbmm_adapter_sweep_step; the counters stay unweighted, the counted loss sum adds L * B
extern "C" int dbmm_adapter_sweep_step_weighted(const float* table, int64_t n_rows, const int64_t* idx, int64_t idx_R, int64_t idx_B,
                                                const int64_t* labels, const int64_t* groups, void* const* params, float* const* bufs,
                                                void* const* old, float ebd_weight, const float* tn, float temperature, const float* lr,
                                                float momentum, float weight_decay, int first_step, float* logits, float* loss_rows,
                                                float* loss_mean, int64_t* counts, double* loss_sum, int64_t G, int counted, const float* row_w,
                                                int64_t Rw, int64_t R, int64_t B, int64_t D, int64_t H, int64_t C, void* workspace,
                                                size_t workspace_bytes, void* stream) {
    if (!row_w) return DBMM_E_ARG;
    return sweep_step_impl(table, n_rows, idx, idx_R, idx_B, labels, groups, params, bufs, old, ebd_weight, tn, temperature, lr, momentum, weight_decay,
                           first_step, logits, loss_rows, loss_mean, counts, loss_sum, G, counted, nullptr, 0.f, R, B, D, H, C, workspace, workspace_bytes,
                           stream, row_w, Rw);
}

extern "C" int dbmm_adapter_sweep_step_gdro(const float* table, int64_t n_rows, const int64_t* idx, int64_t idx_R, int64_t idx_B, const int64_t* labels,
                                            const int64_t* groups, void* const* params, float* const* bufs, void* const* old, float ebd_weight,
                                            const float* tn, float temperature, const float* lr, float momentum, float weight_decay, int first_step,
                                            float* logits, float* loss_rows, float* robust_loss, int64_t* counts, double* loss_sum, int64_t G,
                                            int counted, float* q, float eta, int64_t R, int64_t B, int64_t D, int64_t H, int64_t C, void* workspace,
                                            size_t workspace_bytes, void* stream) {
    if (!q) return DBMM_E_ARG;
    if (G < 1 || G > GDRO_MAXG) return DBMM_E_SHAPE;
    return sweep_step_impl(table, n_rows, idx, idx_R, idx_B, labels, groups, params, bufs, old, ebd_weight, tn, temperature, lr, momentum, weight_decay,
                           first_step, logits, loss_rows, robust_loss, counts, loss_sum, G, counted, q, eta, R, B, D, H, C, workspace, workspace_bytes,
                           stream);
}

extern "C" int dbmm_adapter_sweep_eval(const float* table, int64_t n_rows, const int64_t* idx, int64_t row0, const int64_t* labels,
                                       const int64_t* groups, void* const* params, void* const* old, float ebd_weight, const float* tn,
                                       float temperature, float* logits, float* loss_rows, int64_t* counts, double* loss_sum, int64_t G, int64_t R,
                                       int64_t B, int64_t D, int64_t H, int64_t C, void* workspace, size_t workspace_bytes, void* stream) {
    if (!table || !labels || !groups || !tn || !logits || !loss_rows || !counts || !loss_sum || !workspace) return DBMM_E_ARG;
    if (!stack_ok(params) || (old && !stack_ok(old))) return DBMM_E_ARG;
    int rc = sweep_shape(R, B, D, H, C, G, n_rows, 1);
    if (rc) return rc;
    if (!idx && (row0 < 0 || row0 + B > n_rows)) return DBMM_E_SHAPE;
    const int with_old = old != nullptr;
    if (workspace_bytes < dbmm_workspace_bytes_adapter_sweep_eval(R, B, D, H, with_old)) return DBMM_E_WORKSPACE;
    if (!dbmm_aligned16(workspace) || !dbmm_aligned16(table) || !dbmm_aligned16(tn) || !stack_aligned(params) || (old && !stack_aligned(old)))
        return DBMM_E_ALIGN;
    hipStream_t s = (hipStream_t)stream;
    const EvalLayout L = eval_layout(B, D, with_old);
    float* ws = (float*)workspace;
    const long long wst = L.total;
    const int KS = (int)(D / 128), nb = (int)((B + 31) / 32), iR = (int)R, iB = (int)B, iD = (int)D;
    const float eps = 1e-5f;
    const long long* idxl = (const long long*)idx;
    const float* x = idx ? table : table + row0 * D;                  // no index list: rows row0 .. row0 + B - 1 in place
    const long long* lab = (const long long*)(idx ? labels : labels + row0);
    const long long* grp = (const long long*)(idx ? groups : groups + row0);
    for (int pass = 0; pass < 1 + with_old; ++pass) {
        const AdapterParams A = stack_of(pass ? old : params);
        const long long zo = pass ? L.oz : L.z, ho = pass ? L.oh : L.h, ro = pass ? L.orr : L.r;
        const auto fc1 = idx ? sweep_fc1_kernel<true> : sweep_fc1_kernel<false>;       // rows idx[b] of the table, or rows in place
        hipLaunchKernelGGL(fc1, dim3(nb, 2, KS * iR), dim3(256), 0, s, x, idxl, 0LL, (long long)n_rows, (const float*)A.w1, ws, wst, zo, iB, iD, KS);
        DBMM_CHECK_LAUNCH();
        const long long total = B * 128;
        hipLaunchKernelGGL(sweep_fc1_reduce_kernel, dim3((unsigned)((total + 255) / 256), iR), dim3(256), 0, s, ws, wst, zo, ho, KS, (const float*)A.b1,
                           total, iB);
        DBMM_CHECK_LAUNCH();
        hipLaunchKernelGGL(sweep_fc2_kernel, dim3(nb, (unsigned)(D / 64), iR), dim3(256), 0, s, ws, wst, ho, (const float*)A.rmean, (const float*)A.rvar,
                           128LL, 1, eps, (const float*)A.gamma, (const float*)A.beta, (const float*)A.w2, (const float*)A.b2, ro, zo, iB, iD);
        DBMM_CHECK_LAUNCH();
    }
    const dim3 grid((unsigned)((B + 3) / 4), iR);
    dbmm_with_cmax(C, [&](auto cm) {
        hipLaunchKernelGGL(sweep_ce_fwd_kernel<decltype(cm)::value>, grid, dim3(256), 0, s, ws, wst, L.z, L.oz, ebd_weight, tn, lab, grp, idxl,
                           (long long)n_rows, 1.f / temperature, logits, loss_rows, (unsigned long long*)counts, (int)G, iB, (int)(D / 4), (int)C);
    });
    DBMM_CHECK_LAUNCH();
    hipLaunchKernelGGL(sweep_loss_sum_kernel, dim3(iR), dim3(256), 0, s, (const float*)loss_rows, loss_sum, iB);
    DBMM_CHECK_LAUNCH();
    return DBMM_OK;
}
