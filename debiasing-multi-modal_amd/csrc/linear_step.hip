// The linear-probe step (final_main.py:43-49 LinearClassifier, trained by train_one_epoch :426-496) and its eval forward.
//
// One training step is  logits = x W^T + b;  CE per row and its batch mean;  dlogits = (softmax - onehot) / B;
// dW = dlogits^T x, db = colsum dlogits;  SGD with momentum and weight decay in place (dbmm_sgd_momentum's expression:
// g' = g + wd p; buf = first ? g' : mu buf + g'; p -= lr buf).  With C <= 8 classes and D <= 1024 the whole step reads
// B x D floats of x and a C x D weight: through the autograd path it is ~ten launches of launch overhead, here it is one.
// All arithmetic is exact fp32 FMAs on the vector ALUs; the shapes are far too small for MFMA to matter.
//
//   linear_rows_kernel<NQ, CM, MODE>   one wave per row (rows wave, wave + 4, ... of the block's row slice): the lane owns the
//                                      column quads lane, lane + 64, ... (NQ of them, D <= 256 NQ); logits by a butterfly wave sum
//                                      (every lane ends with the same bits), softmax / CE in registers; the wave accumulates dW
//                                      [CM][NQ] quads, db and the loss sum in registers.  The four waves are summed into LDS in wave
//                                      order and the block writes one slab: dW [C][D] | db [8] | loss sum, pad (pitch C D + 16).
//     MODE_STEP     at most 16 slabs; the last block to arrive sums the slabs in slab order and applies the update (one launch)
//     MODE_PARTIAL  up to 128 slabs, no update: linear_reduce_sgd_kernel does it, gridded over the C x D quads (two launches)
//     MODE_EVAL     no gradient: the slab is the block's loss sum, the last arriver writes the mean
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

constexpr int MODE_EVAL = 0, MODE_STEP = 1, MODE_PARTIAL = 2;
constexpr int LS_MAX_SLABS = 16;          // one-launch step: what the last arriver sums
constexpr int LS_MAX_SLABS2 = 128;        // two-launch step
constexpr int LS_MAX_SLABS_EVAL = 256;    // eval: one float per slab

struct LinArgs {
    const float* x; const long long* labels; float* w; float* b; float* mw; float* mb;
    float lr, mu, wd; int first;
    float* logits; float* loss_rows; float* loss_mean;
    float* slabs; unsigned* counter;
    int B, D, C, RB;
};

inline long long slab_pitch(int C, int D) { return (long long)C * D + 16; }

__device__ __forceinline__ void sgd4(f32x4& p, f32x4& m, f32x4 g, float lr, float mu, float wd, int first) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const float gi = fmaf(wd, p[k], g[k]);
        const float bv = first ? gi : fmaf(mu, m[k], gi);
        m[k] = bv;
        p[k] = p[k] - lr * bv;
    }
}
__device__ __forceinline__ void sgd1(float* p, float* m, float g, float lr, float mu, float wd, int first) {
    const float w = *p;
    const float gi = fmaf(wd, w, g);
    const float bv = first ? gi : fmaf(mu, *m, gi);
    *m = bv;
    *p = w - lr * bv;
}

template <int NQ>
__device__ __forceinline__ void load_row(const float* __restrict__ x, int row, int D4, int lane, f32x4 (&v)[NQ]) {
    const f32x4* xr = (const f32x4*)(x + (long long)row * (D4 * 4));
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
        v[q] = (f32x4){0.f, 0.f, 0.f, 0.f};
        if (q * 64 + lane < D4) v[q] = xr[q * 64 + lane];
    }
}

// takes the block's ticket after its slab is stored; true in the block that arrived last (all its waves may then read every slab)
__device__ __forceinline__ bool arrive_last(unsigned* counter, int* flag) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (threadIdx.x == 0) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const unsigned t = __hip_atomic_fetch_add(counter, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const int last = t == gridDim.x - 1;
        if (last) {
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
        *flag = last;
    }
    __syncthreads();
    return *flag != 0;
}

template <int NQ, int CM, int MODE>
__global__ __launch_bounds__(256) void linear_rows_kernel(const LinArgs a) {
    // W [C][D] while rows run; afterwards the block's dW [C][D] | db [8] | loss, pad (MODE_EVAL: the four wave loss sums)
    __shared__ __attribute__((aligned(16))) float lds[CM * NQ * 256 + 16];
    __shared__ int flag;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int D = a.D, D4 = D >> 2, C = a.C, B = a.B;
    const int r0 = blockIdx.x * a.RB, r1 = min(B, r0 + a.RB);
    for (int i = threadIdx.x; i < C * D4; i += 256) ((f32x4*)lds)[i] = ((const f32x4*)a.w)[i];
    float bias[CM];
#pragma unroll
    for (int c = 0; c < CM; ++c) bias[c] = c < C ? a.b[c] : 0.f;
    __syncthreads();

    f32x4 dw[CM][NQ];
    float db[CM];
#pragma unroll
    for (int c = 0; c < CM; ++c) {
        db[c] = 0.f;
#pragma unroll
        for (int q = 0; q < NQ; ++q) dw[c][q] = (f32x4){0.f, 0.f, 0.f, 0.f};
    }
    float lsum = 0.f;
    const float invB = 1.f / (float)B;
    f32x4 xv[NQ];
    int r = r0 + wave;
    if (r < r1) load_row<NQ>(a.x, r, D4, lane, xv);
    for (; r < r1; r += 4) {
        f32x4 xn[NQ];
        if (r + 4 < r1) load_row<NQ>(a.x, r + 4, D4, lane, xn);      // next row in flight while this one is scored
        const int y = (int)a.labels[r];
        float l[CM];
#pragma unroll
        for (int c = 0; c < CM; ++c) {
            float s = 0.f;
            if (c < C) {
#pragma unroll
                for (int q = 0; q < NQ; ++q)
                    if (q * 64 + lane < D4) {
                        const f32x4 wv = ((const f32x4*)lds)[c * D4 + q * 64 + lane];
                        s = fmaf(xv[q][0], wv[0], s);
                        s = fmaf(xv[q][1], wv[1], s);
                        s = fmaf(xv[q][2], wv[2], s);
                        s = fmaf(xv[q][3], wv[3], s);
                    }
            }
            l[c] = wave_sum(s) + bias[c];
        }
        // CE = (max - l_y) + log1p(sum of the other classes' exp(l - max)): accurate also when the row is well separated (CE << 1),
        // where m + log(sum) - l_y would lose it to cancellation
        float m = l[0];
        int cm = 0;
#pragma unroll
        for (int c = 1; c < CM; ++c) if (c < C && l[c] > m) { m = l[c]; cm = c; }
        float e[CM], so = 0.f, ly = __builtin_nanf("");                 // a label outside [0, C) scores NaN
#pragma unroll
        for (int c = 0; c < CM; ++c) {
            e[c] = c < C ? expf(l[c] - m) : 0.f;
            if (c != cm) so += e[c];
            if (c == y) ly = l[c];
        }
        const float se = 1.f + so;
        const float ce = (m - ly) + log1pf(so);
        lsum += ce;
        if (lane == 0) a.loss_rows[r] = ce;
        float lo = l[0];
#pragma unroll
        for (int c = 1; c < CM; ++c) if (lane == c) lo = l[c];
        if (lane < C) a.logits[(long long)r * C + lane] = lo;
        if (MODE != MODE_EVAL) {
            const float inv = 1.f / se;
#pragma unroll
            for (int c = 0; c < CM; ++c) {
                const float d = (e[c] * inv - (c == y ? 1.f : 0.f)) * invB;
                db[c] += d;
#pragma unroll
                for (int q = 0; q < NQ; ++q) {
                    dw[c][q][0] = fmaf(d, xv[q][0], dw[c][q][0]);
                    dw[c][q][1] = fmaf(d, xv[q][1], dw[c][q][1]);
                    dw[c][q][2] = fmaf(d, xv[q][2], dw[c][q][2]);
                    dw[c][q][3] = fmaf(d, xv[q][3], dw[c][q][3]);
                }
            }
        }
#pragma unroll
        for (int q = 0; q < NQ; ++q) xv[q] = xn[q];
    }
    __syncthreads();                                                     // every wave is done with W in LDS

    if (MODE == MODE_EVAL) {
        if (lane == 0) lds[wave] = lsum;
        __syncthreads();
        if (threadIdx.x == 0) a.slabs[blockIdx.x] = ((lds[0] + lds[1]) + lds[2]) + lds[3];
        if (!arrive_last(a.counter, &flag)) return;
        if (threadIdx.x == 0) {
            float s = 0.f;
            for (int i = 0; i < (int)gridDim.x; ++i) s += a.slabs[i];
            *a.loss_mean = s * invB;
            *a.counter = 0u;
        }
        return;
    }

    // the block's sums, waves in order: dW quads, then db / loss (wave-uniform scalars)
    const int CD = C * D;
    for (int w = 0; w < 4; ++w) {
        if (wave == w) {
#pragma unroll
            for (int c = 0; c < CM; ++c)
                if (c < C)
#pragma unroll
                    for (int q = 0; q < NQ; ++q)
                        if (q * 64 + lane < D4) {
                            f32x4* p = (f32x4*)lds + c * D4 + q * 64 + lane;
                            *p = w == 0 ? dw[c][q] : *p + dw[c][q];
                        }
            if (lane < 16) {
                float v = lane == 8 ? lsum : 0.f;
#pragma unroll
                for (int c = 0; c < CM; ++c) if (lane == c) v = db[c];
                lds[CD + lane] = w == 0 ? v : lds[CD + lane] + v;
            }
        }
        __syncthreads();
    }
    const long long pitch = (long long)CD + 16;
    f32x4* slab = (f32x4*)(a.slabs + blockIdx.x * pitch);
    for (int i = threadIdx.x; i < (CD + 16) / 4; i += 256) slab[i] = ((const f32x4*)lds)[i];
    if (MODE == MODE_PARTIAL) return;
    if (!arrive_last(a.counter, &flag)) return;

    // the last arriver: slab sums in slab order, then the update
    const int NS = gridDim.x;
    for (int i = threadIdx.x; i < CD / 4; i += 256) {
        f32x4 g = ((const f32x4*)a.slabs)[i];
        for (int s = 1; s < NS; ++s) g += ((const f32x4*)(a.slabs + s * pitch))[i];
        f32x4 p = ((const f32x4*)a.w)[i], mv = ((const f32x4*)a.mw)[i];
        sgd4(p, mv, g, a.lr, a.mu, a.wd, a.first);
        ((f32x4*)a.w)[i] = p;
        ((f32x4*)a.mw)[i] = mv;
    }
    if (threadIdx.x < C) {
        const int c = threadIdx.x;
        float g = a.slabs[CD + c];
        for (int s = 1; s < NS; ++s) g += a.slabs[s * pitch + CD + c];
        sgd1(a.b + c, a.mb + c, g, a.lr, a.mu, a.wd, a.first);
    } else if (threadIdx.x == 64) {
        float s = a.slabs[CD + 8];
        for (int k = 1; k < NS; ++k) s += a.slabs[k * pitch + CD + 8];
        *a.loss_mean = s * invB;
    } else if (threadIdx.x == 128) {
        *a.counter = 0u;
    }
}

// two-launch path: thread i < C D / 4 sums the dW quad i over the NS slabs (slab order) and updates W / its momentum; the thread after
// them does db, b and the loss mean
__global__ __launch_bounds__(256) void linear_reduce_sgd_kernel(const LinArgs a, int NS) {
    const int CD = a.C * a.D;
    const long long pitch = (long long)CD + 16;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < CD / 4) {
        f32x4 g = ((const f32x4*)a.slabs)[i];
        for (int s = 1; s < NS; ++s) g += ((const f32x4*)(a.slabs + s * pitch))[i];
        f32x4 p = ((const f32x4*)a.w)[i], mv = ((const f32x4*)a.mw)[i];
        sgd4(p, mv, g, a.lr, a.mu, a.wd, a.first);
        ((f32x4*)a.w)[i] = p;
        ((f32x4*)a.mw)[i] = mv;
    } else if (i == CD / 4) {
        for (int c = 0; c < a.C; ++c) {
            float g = a.slabs[CD + c];
            for (int s = 1; s < NS; ++s) g += a.slabs[s * pitch + CD + c];
            sgd1(a.b + c, a.mb + c, g, a.lr, a.mu, a.wd, a.first);
        }
        float s = a.slabs[CD + 8];
        for (int k = 1; k < NS; ++k) s += a.slabs[k * pitch + CD + 8];
        *a.loss_mean = s / (float)a.B;
    }
}

// row slices: at least `min_rows` rows per block, at most `max_slabs` blocks
void row_split(int64_t B, int min_rows, int max_slabs, int* NS, int* RB) {
    int64_t ns = (B + min_rows - 1) / min_rows;
    if (ns > max_slabs) ns = max_slabs;
    const int64_t rb = (B + ns - 1) / ns;
    *RB = (int)rb;
    *NS = (int)((B + rb - 1) / rb);
}
void split_step1(int64_t B, int* NS, int* RB) { row_split(B, 16, LS_MAX_SLABS, NS, RB); }
void split_step2(int64_t B, int* NS, int* RB) { row_split(B, 64, LS_MAX_SLABS2, NS, RB); }
void split_eval(int64_t B, int* NS, int* RB) { row_split(B, 16, LS_MAX_SLABS_EVAL, NS, RB); }

template <int MODE>
int launch_rows(const LinArgs& a, int NS, hipStream_t s) {
    const int NQ = (a.D / 4 + 63) / 64, CM = a.C <= 2 ? 2 : a.C <= 4 ? 4 : 8;
#define DBMM_LIN_CASE(nq, cm)                                                                                    \
    if (NQ == nq && CM == cm) {                                                                                  \
        hipLaunchKernelGGL((linear_rows_kernel<nq, cm, MODE>), dim3((unsigned)NS), dim3(256), 0, s, a);         \
        DBMM_CHECK_LAUNCH();                                                                                     \
        return DBMM_OK;                                                                                          \
    }
#define DBMM_LIN_CM(nq) DBMM_LIN_CASE(nq, 2) DBMM_LIN_CASE(nq, 4) DBMM_LIN_CASE(nq, 8)
    DBMM_LIN_CM(1) DBMM_LIN_CM(2) DBMM_LIN_CM(3) DBMM_LIN_CM(4)
#undef DBMM_LIN_CM
#undef DBMM_LIN_CASE
    return DBMM_E_SHAPE;
}

bool lin_shape_ok(int64_t B, int64_t D, int64_t C) {
    return B >= 1 && B <= INT32_MAX / 8 && D >= 4 && D <= 1024 && (D % 4) == 0 && C >= 1 && C <= 8;
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

extern "C" int dbmm_linear_train_step(const float* x, const int64_t* labels, float* w, float* b, float* m_w, float* m_b, float lr,
                                      float momentum, float weight_decay, int first_step, float* logits, float* loss_rows, float* loss_mean,
                                      int64_t B, int64_t D, int64_t C, void* workspace, size_t workspace_bytes, void* stream) {
    if (!x || !labels || !w || !b || !m_w || !m_b || !logits || !loss_rows || !loss_mean || !workspace) return DBMM_E_ARG;
    if (!lin_shape_ok(B, D, C)) return DBMM_E_SHAPE;
    if (!dbmm_aligned16(x) || !dbmm_aligned16(w) || !dbmm_aligned16(m_w) || !dbmm_aligned16(workspace)) return DBMM_E_ALIGN;
    if (workspace_bytes < dbmm_workspace_bytes_linear_train_step(B, D, C)) return DBMM_E_WORKSPACE;
    const hipStream_t s = (hipStream_t)stream;
    LinArgs a{x, (const long long*)labels, w, b, m_w, m_b, lr, momentum, weight_decay, first_step, logits, loss_rows, loss_mean,
              (float*)((char*)workspace + 16), (unsigned*)workspace, (int)B, (int)D, (int)C, 0};
    int NS;
    if (B <= dbmm_opt(OPT_LINEAR_STEP_ONE_LAUNCH_MAX_B)) {
        split_step1(B, &NS, &a.RB);
        const hipError_t e = hipMemsetAsync(workspace, 0, sizeof(unsigned), s);       // the ticket counter, per call, ahead of the launch
        if (e != hipSuccess) return (int)e;
        return launch_rows<MODE_STEP>(a, NS, s);
    }
    split_step2(B, &NS, &a.RB);
    const int rc = launch_rows<MODE_PARTIAL>(a, NS, s);
    if (rc != DBMM_OK) return rc;
    const int items = (int)(C * D / 4) + 1;
    hipLaunchKernelGGL(linear_reduce_sgd_kernel, dim3((unsigned)((items + 255) / 256)), dim3(256), 0, s, a, NS);
    DBMM_CHECK_LAUNCH();
    return DBMM_OK;
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
