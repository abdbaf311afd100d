// Replica-batched linear-probe step and evaluation forward: R independent runs of one sweep group (same schedule, different seed and
// possibly learning rate) advance in lock-step and share every launch.  The single step (linear_step.hip) is ONE kernel of at most
// 16 workgroups on a 256-CU chip, so R replicas in one launch cost about what one costs: the replica is grid dimension y and every
// operand is `base + r * stride` into stacked tensors (w [R][C][D], b [R][C], their momentum buffers) and a per-replica slab region.
//
// Every kernel here is a wrapper around a device body of linear_bodies.inc -- the bodies the single-run kernels call -- with the
// block coordinates of the single-run launch (the same row split, switched at the option linear_step_one_launch_max_b), so replica r
// gets the bits dbmm_linear_train_step / dbmm_linear_ce_fwd give for r alone.  What is new (SWEEP in the bodies):
//   * the batch of replica r is rows idx[r][b] of ONE shared embedding table, read in place (rows are 16-B aligned: D % 4 == 0),
//     labels / groups are read as labels[idx[r][b]]: no gathered [R, B, D] copy exists;
//   * the rows kernel also adds the (n, correct) group counters (integer atomics: order-free); the thread that writes the batch loss
//     mean adds `(double)loss_mean * B` to the replica's float64 epoch loss sum (one thread, one add per step); in the evaluation the
//     last block of a replica to arrive sums (double)loss_rows[r][:] in a fixed order;
//   * the per-replica learning rates reach the kernels by value;
//   * one ticket counter per replica (R of them at the head of the workspace, zeroed by ONE memset): the hand-off stays the
//     non-blocking last-arriver ticket of the single step, the last block of ITS replica reduces that replica's slabs.  No block
//     waits for another.
// Launches: step = 1 memset + 1 kernel up to linear_step_one_launch_max_b rows, 2 kernels above; evaluation = 1 memset + 1 kernel;
// whatever R is.  The evaluation keeps the replica as a grid dimension too (a row is read once per replica, from L2 / MALL after the
// first): the forward of one replica is the single-run body unchanged, and 16 x 4096 rows x 4 KB is far below what the caches feed.
#include "common.h"

namespace {

#include "linear_bodies.inc"

constexpr int MAXR = 16;

// Null in the evaluation call, which neither updates nor writes a mean or a slab: mw, mb, loss_mean, slabs (replica_args() keeps
// them null per replica); idx is null when the rows are row0 .. row0 + B - 1; counts and loss_sum are null in an uncounted step.
struct LinSweepArgs {
    const float* x;                       // the table, or its row row0 (evaluation without an index list)
    const long long* idx; long long idx_stride; long long n_tab;
    const long long* labels; const long long* groups;
    float *w, *b, *mw, *mb;               // stacked [R][C][D] / [R][C]
    float lr[MAXR];
    float mu, wd; int first;
    float *logits, *loss_rows, *loss_mean;
    float* slabs; long long slab_stride;  // replica r's slabs at slabs + r * slab_stride
    unsigned* counter;                    // R ticket counters
    unsigned long long* counts; double* loss_sum; int G;
    int B, D, C, RB;
    const float* row_w; long long w_stride;   // per-row loss weights over the table's rows (null: none); replica r's at row_w + r * w_stride
};

__device__ __forceinline__ LinArgs replica_args(const LinSweepArgs& s, int r) {
    float lr = s.lr[0];
#pragma unroll
    for (int i = 1; i < MAXR; ++i)
        if (i == r) lr = s.lr[i];                 // by-value array, selected without indexing it dynamically (keeps it out of scratch memory)
    const long long CD = (long long)s.C * s.D;
    return LinArgs{s.x, s.labels, s.w + r * CD, s.b + r * s.C, s.mw ? s.mw + r * CD : nullptr, s.mb ? s.mb + r * s.C : nullptr,
                   lr, s.mu, s.wd, s.first,
                   s.logits + (long long)r * s.B * s.C, s.loss_rows + (long long)r * s.B, s.loss_mean ? s.loss_mean + r : nullptr,
                   s.slabs ? s.slabs + r * s.slab_stride : nullptr, s.counter + r, s.B, s.D, s.C, s.RB,
                   s.row_w ? s.row_w + r * s.w_stride : nullptr};
}
__device__ __forceinline__ LinSweepRows replica_rows(const LinSweepArgs& s, int r) {
    return LinSweepRows{s.idx ? s.idx + r * s.idx_stride : nullptr, s.n_tab, s.groups,
                        s.counts ? s.counts + (long long)r * s.G * 2 : nullptr, s.G, s.loss_sum ? s.loss_sum + r : nullptr};
}

template <int NQ, int CM, int MODE, bool WEIGHTED = false>
__global__ __launch_bounds__(256) void linear_sweep_rows_kernel(const LinSweepArgs s) {
    __shared__ __attribute__((aligned(16))) float lds[CM * NQ * 256 + 16];
    __shared__ int flag;
    __shared__ unsigned int sc[64][2];
    __shared__ double red[MODE == MODE_EVAL ? 256 : 1];
    const int r = blockIdx.y;
    linear_rows_body<NQ, CM, MODE, true, WEIGHTED>(replica_args(s, r), replica_rows(s, r), blockIdx.x, gridDim.x, lds, &flag, sc, red);
}

__global__ __launch_bounds__(256) void linear_sweep_reduce_sgd_kernel(const LinSweepArgs s, int NS) {
    const int r = blockIdx.y;
    linear_reduce_sgd_body<true>(replica_args(s, r), s.loss_sum ? s.loss_sum + r : nullptr, NS, blockIdx.x);
}

template <int MODE, bool WEIGHTED = false>
int launch_sweep_rows(const LinSweepArgs& a, int NS, int R, hipStream_t s) {
    const int NQ = (a.D / 4 + 63) / 64, CM = a.C <= 2 ? 2 : a.C <= 4 ? 4 : 8;
#define DBMM_LIN_CASE(nq, cm)                                                                                               \
    if (NQ == nq && CM == cm) {                                                                                             \
        hipLaunchKernelGGL((linear_sweep_rows_kernel<nq, cm, MODE, WEIGHTED>), dim3((unsigned)NS, (unsigned)R), dim3(256), 0, s, a); \
        DBMM_CHECK_LAUNCH();                                                                                                \
        return DBMM_OK;                                                                                                     \
    }
#define DBMM_LIN_CM(nq) DBMM_LIN_CASE(nq, 2) DBMM_LIN_CASE(nq, 4) DBMM_LIN_CASE(nq, 8)
    DBMM_LIN_CM(1) DBMM_LIN_CM(2) DBMM_LIN_CM(3) DBMM_LIN_CM(4)
#undef DBMM_LIN_CM
#undef DBMM_LIN_CASE
    return DBMM_E_SHAPE;
}

// per replica: 16 bytes of the counter region, then (step) the slabs of the larger of the two row splits
size_t step_slab_floats(int64_t B, int64_t D, int64_t C) {
    int n1, n2, rb;
    split_step1(B, &n1, &rb);
    split_step2(B, &n2, &rb);
    return (size_t)(n1 > n2 ? n1 : n2) * (size_t)slab_pitch((int)C, (int)D);
}

int sweep_shape(int64_t R, int64_t B, int64_t D, int64_t C, int64_t G, int64_t n_rows) {
    if (R < 1 || R > MAXR || !lin_shape_ok(B, D, C) || G < 1 || G > 64 || n_rows < 1) return DBMM_E_SHAPE;
    return DBMM_OK;
}

}  // namespace

extern "C" size_t dbmm_workspace_bytes_linear_sweep_step(int64_t R, int64_t B, int64_t D, int64_t C) {
    if (R < 1 || R > MAXR || !lin_shape_ok(B, D, C)) return 0;
    return (size_t)R * (16 + step_slab_floats(B, D, C) * sizeof(float));
}

extern "C" size_t dbmm_workspace_bytes_linear_sweep_eval(int64_t R, int64_t B) {
    if (R < 1 || R > MAXR || B < 1 || B > INT32_MAX / 8) return 0;
    return (size_t)R * 16;
}

// `row_w` given: the step under per-row loss weights [Rw][n_rows] over the table's rows, Rw = 1 (shared) or R; else the ERM step
static int linear_sweep_step_impl(const float* table, int64_t n_rows, const int64_t* idx, int64_t idx_R, int64_t idx_B, const int64_t* labels,
                                  const int64_t* groups, float* w, float* b, float* m_w, float* m_b, const float* lr, float momentum,
                                  float weight_decay, int first_step, float* logits, float* loss_rows, float* loss_mean, int64_t* counts,
                                  double* loss_sum, int64_t G, int counted, const float* row_w, int64_t Rw, int64_t R, int64_t B, int64_t D,
                                  int64_t C, void* workspace, size_t workspace_bytes, void* stream) {
    if (!table || !idx || !labels || !groups || !w || !b || !m_w || !m_b || !lr || !logits || !loss_rows || !loss_mean || !counts || !loss_sum ||
        !workspace)
        return DBMM_E_ARG;
    const int rc = sweep_shape(R, B, D, C, G, n_rows);
    if (rc) return rc;
    if (idx_R != R || idx_B != B) return DBMM_E_SHAPE;
    if (row_w && Rw != 1 && Rw != R) return DBMM_E_SHAPE;
    if (!dbmm_aligned16(table) || !dbmm_aligned16(w) || !dbmm_aligned16(m_w) || !dbmm_aligned16(workspace)) return DBMM_E_ALIGN;
    if (workspace_bytes < dbmm_workspace_bytes_linear_sweep_step(R, B, D, C)) return DBMM_E_WORKSPACE;
    const hipStream_t s = (hipStream_t)stream;
    LinSweepArgs a{};
    a.x = table; a.idx = (const long long*)idx; a.idx_stride = B; a.n_tab = n_rows;
    a.labels = (const long long*)labels; a.groups = (const long long*)groups;
    a.w = w; a.b = b; a.mw = m_w; a.mb = m_b;
    for (int i = 0; i < MAXR; ++i) a.lr[i] = i < R ? lr[i] : 0.f;
    a.mu = momentum; a.wd = weight_decay; a.first = first_step;
    a.logits = logits; a.loss_rows = loss_rows; a.loss_mean = loss_mean;
    a.slabs = (float*)((char*)workspace + R * 16); a.slab_stride = (long long)step_slab_floats(B, D, C);
    a.counter = (unsigned*)workspace;
    a.counts = counted ? (unsigned long long*)counts : nullptr; a.loss_sum = counted ? loss_sum : nullptr; a.G = (int)G;
    a.B = (int)B; a.D = (int)D; a.C = (int)C;
    a.row_w = row_w; a.w_stride = (row_w && Rw != 1) ? (long long)n_rows : 0;
    int NS;
    if (B <= dbmm_opt(OPT_LINEAR_STEP_ONE_LAUNCH_MAX_B)) {
        split_step1(B, &NS, &a.RB);
        const hipError_t e = hipMemsetAsync(workspace, 0, (size_t)R * sizeof(unsigned), s);      // the R ticket counters, per call
        if (e != hipSuccess) return (int)e;
        return row_w ? launch_sweep_rows<MODE_STEP, true>(a, NS, (int)R, s) : launch_sweep_rows<MODE_STEP>(a, NS, (int)R, s);
    }
    split_step2(B, &NS, &a.RB);
    const int rc2 = row_w ? launch_sweep_rows<MODE_PARTIAL, true>(a, NS, (int)R, s) : launch_sweep_rows<MODE_PARTIAL>(a, NS, (int)R, s);
    if (rc2 != DBMM_OK) return rc2;
    const int items = (int)(C * D / 4) + 1;
    hipLaunchKernelGGL(linear_sweep_reduce_sgd_kernel, dim3((unsigned)((items + 255) / 256), (unsigned)R), dim3(256), 0, s, a, NS);
    DBMM_CHECK_LAUNCH();
    return DBMM_OK;
}

extern "C" int dbmm_linear_sweep_step(const float* table, int64_t n_rows, const int64_t* idx, int64_t idx_R, int64_t idx_B, const int64_t* labels,
                                      const int64_t* groups, float* w, float* b, float* m_w, float* m_b, const float* lr, float momentum,
                                      float weight_decay, int first_step, float* logits, float* loss_rows, float* loss_mean, int64_t* counts,
                                      double* loss_sum, int64_t G, int counted, int64_t R, int64_t B, int64_t D, int64_t C, void* workspace,
                                      size_t workspace_bytes, void* stream) {
    return linear_sweep_step_impl(table, n_rows, idx, idx_R, idx_B, labels, groups, w, b, m_w, m_b, lr, momentum, weight_decay, first_step, logits,
                                  loss_rows, loss_mean, counts, loss_sum, G, counted, nullptr, 0, R, B, D, C, workspace, workspace_bytes, stream);
}

// every replica's step under per-row loss weights row_w [Rw][n_rows] (fp32, over the TABLE's rows; Rw = 1: shared, Rw = R: one vector
// each), indexed like the labels: batch row b of replica r weighs row_w[(Rw == 1 ? 0 : r) * n_rows + idx[r][b] clamped].  The workspace
// and launches of dbmm_linear_sweep_step; the counters stay unweighted, the counted loss sum adds L * B
extern "C" int dbmm_linear_sweep_step_weighted(const float* table, int64_t n_rows, const int64_t* idx, int64_t idx_R, int64_t idx_B,
                                               const int64_t* labels, const int64_t* groups, float* w, float* b, float* m_w, float* m_b,
                                               const float* lr, float momentum, float weight_decay, int first_step, float* logits,
                                               float* loss_rows, float* loss_mean, int64_t* counts, double* loss_sum, int64_t G, int counted,
                                               const float* row_w, int64_t Rw, int64_t R, int64_t B, int64_t D, int64_t C, void* workspace,
                                               size_t workspace_bytes, void* stream) {
    if (!row_w) return DBMM_E_ARG;
    return linear_sweep_step_impl(table, n_rows, idx, idx_R, idx_B, labels, groups, w, b, m_w, m_b, lr, momentum, weight_decay, first_step, logits,
                                  loss_rows, loss_mean, counts, loss_sum, G, counted, row_w, Rw, R, B, D, C, workspace, workspace_bytes, stream);
}

extern "C" int dbmm_linear_sweep_eval(const float* table, int64_t n_rows, const int64_t* idx, int64_t row0, const int64_t* labels,
                                      const int64_t* groups, const float* w, const float* b, float* logits, float* loss_rows, int64_t* counts,
                                      double* loss_sum, int64_t G, int64_t R, int64_t B, int64_t D, int64_t C, void* workspace,
                                      size_t workspace_bytes, void* stream) {
    if (!table || !labels || !groups || !w || !b || !logits || !loss_rows || !counts || !loss_sum || !workspace) return DBMM_E_ARG;
    const int rc = sweep_shape(R, B, D, C, G, n_rows);
    if (rc) return rc;
    if (!idx && (row0 < 0 || row0 + B > n_rows)) return DBMM_E_SHAPE;
    if (!dbmm_aligned16(table) || !dbmm_aligned16(w) || !dbmm_aligned16(workspace)) return DBMM_E_ALIGN;
    if (workspace_bytes < dbmm_workspace_bytes_linear_sweep_eval(R, B)) return DBMM_E_WORKSPACE;
    const hipStream_t s = (hipStream_t)stream;
    LinSweepArgs a{};
    a.x = idx ? table : table + row0 * D;                                 // no index list: rows row0 .. row0 + B - 1 in place
    a.idx = (const long long*)idx; a.idx_stride = 0; a.n_tab = n_rows;   // every replica scores the same rows
    a.labels = (const long long*)(idx ? labels : labels + row0); a.groups = (const long long*)(idx ? groups : groups + row0);
    a.w = (float*)w; a.b = (float*)b;
    a.logits = logits; a.loss_rows = loss_rows;
    a.counter = (unsigned*)workspace;
    a.counts = (unsigned long long*)counts; a.loss_sum = loss_sum; a.G = (int)G;
    a.B = (int)B; a.D = (int)D; a.C = (int)C;
    int NS;
    split_eval(B, &NS, &a.RB);
    const hipError_t e = hipMemsetAsync(workspace, 0, (size_t)R * sizeof(unsigned), s);
    if (e != hipSuccess) return (int)e;
    return launch_sweep_rows<MODE_EVAL>(a, NS, (int)R, s);
}
