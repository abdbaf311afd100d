// What adapter_step.hip defines for adapter_ops.hip (the single step) and adapter_sweep.hip (the replica-batched step), and the
// values all three pass around: one adapter, its momentum buffers, the SGD scalars, the layout of the fast backward's scratch.
#pragma once
#include "common.h"

// the nine tensors of an adapter that only runs forward: weights read-only, the running statistics still written (train-mode BatchNorm)
struct FrozenAdapter {
    const float *w1, *b1, *gamma, *beta;
    float *rmean, *rvar;
    long long* nbt;
    const float *w2, *b2;
};
// one trainable adapter's nine tensors; in the sweep each is the stack of R adapters ([R, ...] contiguous, H = 128)
struct AdapterParams {
    float *w1, *b1, *gamma, *beta, *rmean, *rvar;
    long long* nbt;
    float *w2, *b2;
    FrozenAdapter forward_only() const { return {w1, b1, gamma, beta, rmean, rvar, nbt, w2, b2}; }
};
// the six SGD momentum buffers, in the order of the gradients
struct AdapterMomentum {
    float *w1, *b1, *gamma, *beta, *w2, *b2;
};
// the scalars of the SGD update that ends a single step
struct SgdScalars {
    float lr, momentum, weight_decay;
    int first_step;
};

// the fast backward's scratch, in floats: K-split partial sums of dr [D / 128][B][128] | batch-split partial sums of dW2 [NS][D][128],
// db2 [NS][D], dW1 [NS][128][D], db1 [NS][128].  NS batch splits (at most 16) of RB rows each (a multiple of 32)
struct BwdScratch {
    int NS, RB;
    long long drpart, dw2part, db2part, dw1part, db1part, total;
};
static inline BwdScratch dbmm_adapter_bwd_scratch(int64_t B, int64_t D) {
    BwdScratch S{};
    const int nb = (int)((B + 31) / 32);
    S.NS = nb < 16 ? nb : 16;
    S.RB = ((nb + S.NS - 1) / S.NS) * 32;
    S.NS = (int)((B + S.RB - 1) / S.RB);
    S.drpart = 0;
    S.dw2part = S.drpart + B * D;
    S.db2part = S.dw2part + (long long)S.NS * D * 128;
    S.dw1part = S.db2part + (long long)S.NS * D;
    S.db1part = S.dw1part + (long long)S.NS * 128 * D;
    S.total = S.db1part + (long long)S.NS * 128;
    return S;
}

// the cosine-logits kernels exist for up to 4 and up to 8 classes: calls f(std::integral_constant<int, CMAX>) with the one that holds C
template <class F>
static inline void dbmm_with_cmax(int64_t C, F&& f) {
    if (C <= 4) f(std::integral_constant<int, 4>{});
    else f(std::integral_constant<int, 8>{});
}

// the shapes the kernels of adapter_step.hip serve (the reference's: H = 128, D % 128 == 0)
bool dbmm_adapter_fast_shape(int64_t B, int64_t D, int64_t H);
// forward: h (pre-BatchNorm), mean / invstd (train), r, z.  `z` doubles as the scratch of the K-split partial sums.
int dbmm_adapter_fwd_fast(const float* x, const float* w1, const float* b1, const float* gamma, const float* beta, float* running_mean,
                          float* running_var, int64_t* nbt, const float* w2, const float* b2, float* h, float* mean, float* invstd, float* r,
                          float* z, int64_t B, int64_t D, int train, float eps, float momentum, hipStream_t s);
// backward: dW2, db2, dgamma, dbeta, dh (left in `dh`) and, with `sum_dw1`, dW1, db1; `scratch` = dbmm_adapter_bwd_scratch(B, D).total floats.
// !sum_dw1: the batch splits of dW1 / db1 stay in the scratch and the caller (the one-call step) sums them inside its SGD launch, in the
// same order.  `loss_mean` given: a spare block of the first launch writes the mean of loss_rows [B] to it; with `row_w` [B] (per-row
// loss weights) that block writes (1 / B) sum_b loss_rows[b] row_w[b] instead.
int dbmm_adapter_bwd_fast(const float* x, const float* dz, const float* h, const float* mean, const float* invstd, const float* r, const float* gamma,
                          const float* beta, const float* w2, float* dw1, float* db1, float* dgamma, float* dbeta, float* dw2, float* db2,
                          float* dh, float* scratch, int64_t B, int64_t D, hipStream_t s, bool sum_dw1, const float* loss_rows, float* loss_mean,
                          const float* row_w = nullptr);
