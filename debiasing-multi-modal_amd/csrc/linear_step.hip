// The linear-probe step (final_main.py:43-49 LinearClassifier, trained by train_one_epoch :426-496) and its eval forward.
//
// One training step is  logits = x W^T + b;  CE per row and its batch mean;  dlogits = (softmax - onehot) / B;
// dW = dlogits^T x, db = colsum dlogits;  SGD with momentum and weight decay in place (dbmm_sgd_momentum's expression:
// g' = g + wd p; buf = first ? g' : mu buf + g'; p -= lr buf).  With C <= 8 classes and D <= 1024 the whole step reads
// B x D floats of x and a C x D weight: through the autograd path it is ~ten launches of launch overhead, here it is one.
// All arithmetic is exact fp32 FMAs on the vector ALUs; the shapes are far too small for MFMA to matter.
//
// The device code is in linear_bodies.inc (linear_rows_body, linear_reduce_sgd_body; the replica-batched kernels of
// linear_sweep.hip call the same bodies); the kernels here are those bodies on their own grid.
//
// Determinism: every sum runs in a fixed order (row order inside a wave, wave order inside a block, slab order across blocks), so
// two calls on the same inputs give identical bits whatever the block timing; no float atomics.  The in-launch hand-off is the
// split-K recipe: each block stores its slab with plain stores, drains them, and one lane issues an agent-scope release before
// taking its ticket (relaxed agent-scope fetch_add on a counter the host zeroes with hipMemsetAsync ahead of every launch); the block
// that draws the last ticket issues an agent-scope acquire before any wave reads a slab.  That is correct for any placement of the
// blocks over the XCDs, whose L2s are not coherent with each other.
//
// Updating W and b in place is safe: every block copies W and b into LDS / registers before its first row, and the reducer only
// runs after every block has taken its ticket, i.e. after every block is done reading them (in the two-launch path the update is a
// later launch).  x is never written.
#include "common.h"

namespace {

#include "linear_bodies.inc"

template <int NQ, int CM, int MODE, bool WEIGHTED = false>
__global__ __launch_bounds__(256) void linear_rows_kernel(const LinArgs a) {
    __shared__ __attribute__((aligned(16))) float lds[CM * NQ * 256 + 16];
    __shared__ int flag;
    linear_rows_body<NQ, CM, MODE, false, WEIGHTED>(a, LinSweepRows{}, blockIdx.x, gridDim.x, lds, &flag, nullptr, nullptr);
}

__global__ __launch_bounds__(256) void linear_reduce_sgd_kernel(const LinArgs a, int NS) {
    linear_reduce_sgd_body<false>(a, nullptr, NS, blockIdx.x);
}

template <int MODE, bool WEIGHTED = false>
int launch_rows(const LinArgs& a, int NS, hipStream_t s) {
    const int NQ = (a.D / 4 + 63) / 64, CM = a.C <= 2 ? 2 : a.C <= 4 ? 4 : 8;
#define DBMM_LIN_CASE(nq, cm)                                                                                    \
    if (NQ == nq && CM == cm) {                                                                                  \
        hipLaunchKernelGGL((linear_rows_kernel<nq, cm, MODE, WEIGHTED>), dim3((unsigned)NS), dim3(256), 0, s, a); \
        DBMM_CHECK_LAUNCH();                                                                                     \
        return DBMM_OK;                                                                                          \
    }
#define DBMM_LIN_CM(nq) DBMM_LIN_CASE(nq, 2) DBMM_LIN_CASE(nq, 4) DBMM_LIN_CASE(nq, 8)
    DBMM_LIN_CM(1) DBMM_LIN_CM(2) DBMM_LIN_CM(3) DBMM_LIN_CM(4)
#undef DBMM_LIN_CM
#undef DBMM_LIN_CASE
    return DBMM_E_SHAPE;
}

}  // namespace

extern "C" size_t dbmm_workspace_bytes_linear_train_step(int64_t B, int64_t D, int64_t C) {
    if (!lin_shape_ok(B, D, C)) return 0;
    int n1, n2, rb;
    split_step1(B, &n1, &rb);
    split_step2(B, &n2, &rb);
    return 16 + (size_t)(n1 > n2 ? n1 : n2) * (size_t)slab_pitch((int)C, (int)D) * sizeof(float);
}

extern "C" size_t dbmm_workspace_bytes_linear_ce_fwd(int64_t B) {
    if (B < 1 || B > INT32_MAX / 8) return 0;
    int ns, rb;
    split_eval(B, &ns, &rb);
    return 16 + (size_t)ns * sizeof(float);
}

// `row_w` given: the step under per-row loss weights [B] (the WEIGHTED kernels), else the ERM step
static int linear_step_impl(const float* x, const int64_t* labels, float* w, float* b, float* m_w, float* m_b, float lr, float momentum,
                            float weight_decay, int first_step, float* logits, float* loss_rows, float* loss_mean, const float* row_w, int64_t B,
                            int64_t D, int64_t C, void* workspace, size_t workspace_bytes, void* stream) {
    if (!x || !labels || !w || !b || !m_w || !m_b || !logits || !loss_rows || !loss_mean || !workspace) return DBMM_E_ARG;
    if (!lin_shape_ok(B, D, C)) return DBMM_E_SHAPE;
    if (!dbmm_aligned16(x) || !dbmm_aligned16(w) || !dbmm_aligned16(m_w) || !dbmm_aligned16(workspace)) return DBMM_E_ALIGN;
    if (workspace_bytes < dbmm_workspace_bytes_linear_train_step(B, D, C)) return DBMM_E_WORKSPACE;
    const hipStream_t s = (hipStream_t)stream;
    LinArgs a{x, (const long long*)labels, w, b, m_w, m_b, lr, momentum, weight_decay, first_step, logits, loss_rows, loss_mean,
              (float*)((char*)workspace + 16), (unsigned*)workspace, (int)B, (int)D, (int)C, 0, row_w};
    int NS;
    if (B <= dbmm_opt(OPT_LINEAR_STEP_ONE_LAUNCH_MAX_B)) {
        split_step1(B, &NS, &a.RB);
        const hipError_t e = hipMemsetAsync(workspace, 0, sizeof(unsigned), s);       // the ticket counter, per call, ahead of the launch
        if (e != hipSuccess) return (int)e;
        return row_w ? launch_rows<MODE_STEP, true>(a, NS, s) : launch_rows<MODE_STEP>(a, NS, s);
    }
    split_step2(B, &NS, &a.RB);
    const int rc = row_w ? launch_rows<MODE_PARTIAL, true>(a, NS, s) : launch_rows<MODE_PARTIAL>(a, NS, s);
    if (rc != DBMM_OK) return rc;
    const int items = (int)(C * D / 4) + 1;
    hipLaunchKernelGGL(linear_reduce_sgd_kernel, dim3((unsigned)((items + 255) / 256)), dim3(256), 0, s, a, NS);
    DBMM_CHECK_LAUNCH();
    return DBMM_OK;
}

extern "C" int dbmm_linear_train_step(const float* x, const int64_t* labels, float* w, float* b, float* m_w, float* m_b, float lr,
                                      float momentum, float weight_decay, int first_step, float* logits, float* loss_rows, float* loss_mean,
                                      int64_t B, int64_t D, int64_t C, void* workspace, size_t workspace_bytes, void* stream) {
    return linear_step_impl(x, labels, w, b, m_w, m_b, lr, momentum, weight_decay, first_step, logits, loss_rows, loss_mean, nullptr, B, D, C,
                            workspace, workspace_bytes, stream);
}

// the step under per-row loss weights row_w [B] (fp32, taken as they are): L = (1 / B) sum_b row_w[b] CE_b.  Same workspace and launches
// as dbmm_linear_train_step; logits / loss_rows are the unweighted ones; all-ones weights give that step's bits
extern "C" int dbmm_linear_train_step_weighted(const float* x, const int64_t* labels, float* w, float* b, float* m_w, float* m_b, float lr,
                                               float momentum, float weight_decay, int first_step, float* logits, float* loss_rows,
                                               float* loss_mean, const float* row_w, int64_t B, int64_t D, int64_t C, void* workspace,
                                               size_t workspace_bytes, void* stream) {
    if (!row_w) return DBMM_E_ARG;
    return linear_step_impl(x, labels, w, b, m_w, m_b, lr, momentum, weight_decay, first_step, logits, loss_rows, loss_mean, row_w, B, D, C,
                            workspace, workspace_bytes, stream);
}

extern "C" int dbmm_linear_ce_fwd(const float* x, const float* w, const float* b, const int64_t* labels, float* logits, float* loss_rows,
                                  float* loss_mean, int64_t B, int64_t D, int64_t C, void* workspace, size_t workspace_bytes, void* stream) {
    if (!x || !w || !b || !labels || !logits || !loss_rows || !loss_mean || !workspace) return DBMM_E_ARG;
    if (!lin_shape_ok(B, D, C)) return DBMM_E_SHAPE;
    if (!dbmm_aligned16(x) || !dbmm_aligned16(w) || !dbmm_aligned16(workspace)) return DBMM_E_ALIGN;
    if (workspace_bytes < dbmm_workspace_bytes_linear_ce_fwd(B)) return DBMM_E_WORKSPACE;
    const hipStream_t s = (hipStream_t)stream;
    LinArgs a{x, (const long long*)labels, (float*)w, (float*)b, nullptr, nullptr, 0.f, 0.f, 0.f, 0, logits, loss_rows, loss_mean,
              (float*)((char*)workspace + 16), (unsigned*)workspace, (int)B, (int)D, (int)C, 0};
    int NS;
    split_eval(B, &NS, &a.RB);
    const hipError_t e = hipMemsetAsync(workspace, 0, sizeof(unsigned), s);
    if (e != hipSuccess) return (int)e;
    return launch_rows<MODE_EVAL>(a, NS, s);
}
