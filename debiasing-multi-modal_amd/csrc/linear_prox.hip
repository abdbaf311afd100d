// L1-penalised logistic probes by FISTA, many iterations per launch: ONE workgroup per fit ("replica"), the iterate resident in LDS.
//
// Deep feature reweighting fits dozens of tiny full-batch problems (200 - 3000 rows x 1024 columns, 2 classes) that each need hundreds
// of DEPENDENT iterations.  Through the step kernels that is one launch per iteration, every one of them on the launch floor; here
// replica r is workgroup r and runs `iters` iterations of
//     G, g    = gradient of (1 / n) sum_i CE(softmax(V x_i + c), y_i)           over the rows idx[r][0 .. n) of a shared table
//     W'      = soft(V - eta G, eta lam)          soft(z, tau) = sign(z) max(|z| - tau, 0), an exact +0 inside the threshold
//     b'      = c - eta g                         (the intercept is not penalised)
//     t'      = (1 + sqrt(1 + 4 t^2)) / 2         in float64;  beta = fp32((t - 1) / t')   (accelerate == 0: beta = 0, plain ISTA)
//     V'      = W' + beta (W' - W),  c' = b' + beta (b' - b)
// with no communication between workgroups: no ticket, no atomics, no spinning.  Per iteration every wave walks the rows wave, wave +
// NW, ... of the replica's index list (clamped into the table, the next row in flight), scores a row against V in LDS and adds to dW
// [CM][NQ] quads in registers -- the arithmetic of linear_rows_body (linear_bodies.inc): lane ownership of the column quads, fmaf chains,
// butterfly wave sums, the CE by its log1p form, labels compared as 64 bits.  The waves are then summed through LDS in wave order and
// every thread applies the prox and the extrapolation to the quads tid, tid + NT, ...  W, V and the reduction buffer stay in LDS
// across the iterations (3 x 32 KB at C = 8, D = 1024); only the state at the end of the launch goes back to memory.
//
// Every sum has a fixed order that depends on (n, D, C) only: two calls give the same bits, a replica's bits depend neither on R nor
// on its place in the grid, and K iterations in one launch are the K iterations of several launches (the state W, b, V, c, t
// round-trips exactly: nothing else is carried from one iteration to the next).
//
// Workgroup size per (CM, NQ): the dW accumulators are CM x NQ x 4 VGPRs a lane.  16 waves (4 per SIMD, <= 128 VGPRs) where the
// kernel fits that, else 8 (<= 256) or 4 (<= 512): prox_waves below; no instantiation uses scratch.
#include "common.h"

namespace {

#include "linear_bodies.inc"

constexpr int PROX_MAX_R = 256;
constexpr int PROX_MAX_ITERS = 1 << 20;

struct ProxArgs {
    const float* x; const long long* idx; long long n_tab; const long long* labels;
    const float* lam; const float* step;
    float *w, *b, *v, *c; double* t;
    float* stats;                          // [R][4]: delta, wmax, nnz, CE mean of the launch's last iteration
    int n, D, C, iters, accelerate;
};

// Waves of the workgroup, from the register counts of the compiled instantiations (tools/isa_regs.py; the table is in DESIGN.md,
// section 6f): 16 waves (4 per SIMD, 128 VGPRs) where the kernel fits that without scratch (two classes up to D = 768), 4 waves
// (512 VGPRs) for the one instantiation that needs more than 256 (C > 4 at D > 768: 128 accumulator registers), else 8 waves (256).
constexpr int prox_waves(int CM, int NQ) {
    return (CM == 2 && NQ <= 3) ? 16 : CM * NQ == 32 ? 4 : 8;
}

// t' = (1 + sqrt(1 + 4 t^2)) / 2 as the float64 statements read, uncontracted: the host's recurrence gives the same bits
__device__ __forceinline__ double prox_next_t(double t) {
#pragma clang fp contract(off)
    const double q = 4.0 * t * t;
    return (1.0 + sqrt(1.0 + q)) * 0.5;
}

// Row `i` of the replica's index list as a table row, clamped into the table, and the lane's quads of a table row: written without a
// branch (the ragged last quad reads a clamped address and is zeroed by a select), so that the loads of the NEXT row stay in flight
// while this one is scored -- a load under a divergent branch is waited for where it is issued.  D4 > 64 (NQ - 1): only the last quad
// of a lane can lie past the row's end.
__device__ __forceinline__ long long prox_row(const long long* idx, long long n_tab, int i) {
    const long long s = idx[i];
    return s < 0 ? 0 : (s >= n_tab ? n_tab - 1 : s);
}
template <int NQ>
__device__ __forceinline__ void prox_load_row(const float* __restrict__ x, long long row, int D4, int lane, f32x4 (&v)[NQ]) {
    const f32x4* xr = (const f32x4*)(x + row * (D4 * 4));
#pragma unroll
    for (int q = 0; q < NQ - 1; ++q) v[q] = xr[q * 64 + lane];
    const int last = (NQ - 1) * 64 + lane;
    const f32x4 t = xr[min(last, D4 - 1)];
    v[NQ - 1] = last < D4 ? t : (f32x4){0.f, 0.f, 0.f, 0.f};
}

template <int NQ, int CM, int NW>
__global__ __launch_bounds__(NW * 64) void linear_prox_kernel(const ProxArgs a) {
    constexpr int NT = NW * 64, CDM = CM * NQ * 256;
    __shared__ __attribute__((aligned(16))) float sV[CDM];               // the extrapolated point V [C][D]
    __shared__ __attribute__((aligned(16))) float sW[CDM];               // the iterate W [C][D]
    __shared__ __attribute__((aligned(16))) float red[CDM + 16];         // dW [C][D] | db [8] | loss sum, pad
    __shared__ float sb[8], sc[8];                                       // b, c
    __shared__ float sstat[NW][4];
    const int rep = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int D = a.D, D4 = D >> 2, C = a.C, n = a.n, CD = C * D, CD4 = C * D4;
    const long long* idx = a.idx + (long long)rep * n;
    {
        const f32x4* gw = (const f32x4*)(a.w + (long long)rep * CD);
        const f32x4* gv = (const f32x4*)(a.v + (long long)rep * CD);
        for (int i = tid; i < CD4; i += NT) {
            ((f32x4*)sW)[i] = gw[i];
            ((f32x4*)sV)[i] = gv[i];
        }
        if (tid < 8) {
            sb[tid] = tid < C ? a.b[rep * C + tid] : 0.f;
            sc[tid] = tid < C ? a.c[rep * C + tid] : 0.f;
        }
    }
    double t = a.t[rep];
    const float eta = a.step[rep], thr = eta * a.lam[rep];
    const float invn = 1.f / (float)n;
    float s_delta = 0.f, s_wmax = 0.f, s_nnz = 0.f;
    __syncthreads();

    for (int it = 0; it < a.iters; ++it) {
        float bias[CM];
#pragma unroll
        for (int c = 0; c < CM; ++c) bias[c] = c < C ? sc[c] : 0.f;
        f32x4 dw[CM][NQ];
        float db[CM];
#pragma unroll
        for (int c = 0; c < CM; ++c) {
            db[c] = 0.f;
#pragma unroll
            for (int q = 0; q < NQ; ++q) dw[c][q] = (f32x4){0.f, 0.f, 0.f, 0.f};
        }
        float lsum = 0.f;
        // one row against V: logits, CE, and the row's term of dW / db in the wave's registers
        auto score = [&](const f32x4 (&xv)[NQ], const long long yl) {
            const int y = (yl >= 0 && yl < (long long)C) ? (int)yl : -1; // the int64 label is compared: 2^32 + 1 is no class
            float l[CM];
#pragma unroll
            for (int c = 0; c < CM; ++c) {
                float s = 0.f;
                if (c < C) {
#pragma unroll
                    for (int q = 0; q < NQ; ++q)
                        if (q < NQ - 1 || q * 64 + lane < D4) {
                            const f32x4 wv = ((const f32x4*)sV)[c * D4 + q * 64 + lane];
                            s = fmaf(xv[q][0], wv[0], s);
                            s = fmaf(xv[q][1], wv[1], s);
                            s = fmaf(xv[q][2], wv[2], s);
                            s = fmaf(xv[q][3], wv[3], s);
                        }
                }
                l[c] = s;
            }
            // wave_sum's butterfly for every class, the classes side by side (their shuffles overlap): every lane ends with the same bits
#pragma unroll
            for (int o = 32; o > 0; o >>= 1)
#pragma unroll
                for (int c = 0; c < CM; ++c) l[c] += __shfl_xor(l[c], o, 64);
#pragma unroll
            for (int c = 0; c < CM; ++c) l[c] += bias[c];
            // CE = (max - l_y) + log1p(sum of the other classes' exp(l - max)), as in linear_rows_body
            float m = l[0];
            int cm = 0;
#pragma unroll
            for (int c = 1; c < CM; ++c) if (c < C && l[c] > m) { m = l[c]; cm = c; }
            float e[CM], so = 0.f, ly = __builtin_nanf("");             // a label outside [0, C) scores NaN
#pragma unroll
            for (int c = 0; c < CM; ++c) {
                e[c] = c < C ? expf(l[c] - m) : 0.f;
                if (c != cm) so += e[c];
                if (c == y) ly = l[c];
            }
            lsum += (m - ly) + log1pf(so);
            const float inv = 1.f / (1.f + so);
#pragma unroll
            for (int c = 0; c < CM; ++c) {
                const float d = (e[c] * inv - (c == y ? 1.f : 0.f)) * invn;
                db[c] += d;
#pragma unroll
                for (int q = 0; q < NQ; ++q) {
                    dw[c][q][0] = fmaf(d, xv[q][0], dw[c][q][0]);
                    dw[c][q][1] = fmaf(d, xv[q][1], dw[c][q][1]);
                    dw[c][q][2] = fmaf(d, xv[q][2], dw[c][q][2]);
                    dw[c][q][3] = fmaf(d, xv[q][3], dw[c][q][3]);
                }
            }
        };
        // Rows wave, wave + NW, ... in that order, two to a trip on two register buffers: while a row is scored the next row, its label
        // and the list entry three rows on are in flight (past the wave's last row the list's last row is read again and dropped).
        // Loads return in order, so nothing a half-trip needs was issued in that half-trip, and no buffer is copied (a copy waits
        // for its load): `snext` is the table row of the row after this one, `sraw` the list entry of the one after that.
        f32x4 xa[NQ], xb[NQ];
        long long ya = 0, yb = 0, snext = 0, sraw = 0;
        int r = wave;
        if (r < n) {
            const long long srow = prox_row(idx, a.n_tab, r);
            snext = prox_row(idx, a.n_tab, min(r + NW, n - 1));
            sraw = idx[min(r + 2 * NW, n - 1)];
            prox_load_row<NQ>(a.x, srow, D4, lane, xa);
            ya = a.labels[srow];
        }
        for (; r < n; r += 2 * NW) {
            prox_load_row<NQ>(a.x, snext, D4, lane, xb);
            yb = a.labels[snext];
            const long long sraw3 = idx[min(r + 3 * NW, n - 1)];
            score(xa, ya);
            if (r + NW >= n) break;
            const long long s2 = sraw < 0 ? 0 : (sraw >= a.n_tab ? a.n_tab - 1 : sraw);
            prox_load_row<NQ>(a.x, s2, D4, lane, xa);
            ya = a.labels[s2];
            sraw = idx[min(r + 4 * NW, n - 1)];
            score(xb, yb);
            snext = sraw3 < 0 ? 0 : (sraw3 >= a.n_tab ? a.n_tab - 1 : sraw3);
        }

        // the replica's sums, waves in order: dW quads, then db / loss (wave-uniform scalars).  The barrier that closed the previous
        // iteration's update freed `red`
        for (int w = 0; w < NW; ++w) {
            if (wave == w) {
#pragma unroll
                for (int c = 0; c < CM; ++c)
                    if (c < C)
#pragma unroll
                        for (int q = 0; q < NQ; ++q)
                            if (q < NQ - 1 || q * 64 + lane < D4) {
                                f32x4* p = (f32x4*)red + c * D4 + q * 64 + lane;
                                *p = w == 0 ? dw[c][q] : *p + dw[c][q];
                            }
                if (lane < 16) {
                    float v = lane == 8 ? lsum : 0.f;
#pragma unroll
                    for (int c = 0; c < CM; ++c) if (lane == c) v = db[c];
                    red[CD + lane] = w == 0 ? v : red[CD + lane] + v;
                }
            }
            __syncthreads();
        }

        const double t1 = prox_next_t(t);
        const float beta = a.accelerate ? (float)((t - 1.0) / t1) : 0.f;
        t = t1;
        const bool last = it == a.iters - 1;
        for (int i = tid; i < CD4; i += NT) {
            const f32x4 g = ((const f32x4*)red)[i], vo = ((const f32x4*)sV)[i], wo = ((const f32x4*)sW)[i];
            f32x4 wn, vn;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const float z = fmaf(-eta, g[k], vo[k]);
                const float az = fabsf(z) - thr;
                wn[k] = az > 0.f ? copysignf(az, z) : 0.f;
                const float dk = wn[k] - wo[k];
                vn[k] = fmaf(beta, dk, wn[k]);
                if (last) {
                    s_delta = fmaxf(s_delta, fabsf(dk));
                    s_wmax = fmaxf(s_wmax, fabsf(wn[k]));
                    s_nnz += wn[k] != 0.f ? 1.f : 0.f;
                }
            }
            ((f32x4*)sW)[i] = wn;
            ((f32x4*)sV)[i] = vn;
        }
        if (tid < C) {
            const float bo = sb[tid];
            const float bn = fmaf(-eta, red[CD + tid], sc[tid]);
            sb[tid] = bn;
            sc[tid] = fmaf(beta, bn - bo, bn);
        }
        __syncthreads();
    }

    // the state at the end of the launch, and the last iteration's figures (maxima are order-free, the count is an integer below 2^24)
    {
        f32x4* gw = (f32x4*)(a.w + (long long)rep * CD);
        f32x4* gv = (f32x4*)(a.v + (long long)rep * CD);
        for (int i = tid; i < CD4; i += NT) {
            gw[i] = ((const f32x4*)sW)[i];
            gv[i] = ((const f32x4*)sV)[i];
        }
        if (tid < C) {
            a.b[rep * C + tid] = sb[tid];
            a.c[rep * C + tid] = sc[tid];
        }
    }
    s_delta = wave_max(s_delta);
    s_wmax = wave_max(s_wmax);
    s_nnz = wave_sum(s_nnz);
    if (lane == 0) { sstat[wave][0] = s_delta; sstat[wave][1] = s_wmax; sstat[wave][2] = s_nnz; }
    __syncthreads();
    if (tid == 0) {
        float d = sstat[0][0], m = sstat[0][1], z = sstat[0][2];
        for (int w = 1; w < NW; ++w) { d = fmaxf(d, sstat[w][0]); m = fmaxf(m, sstat[w][1]); z += sstat[w][2]; }
        float* st = a.stats + (long long)rep * 4;
        st[0] = d; st[1] = m; st[2] = z; st[3] = red[CD + 8] * invn;
        a.t[rep] = t;
    }
}

int launch_prox(const ProxArgs& a, int R, hipStream_t s) {
    const int NQ = (a.D / 4 + 63) / 64, CM = a.C <= 2 ? 2 : a.C <= 4 ? 4 : 8;
#define DBMM_PROX_CASE(nq, cm)                                                                                              \
    if (NQ == nq && CM == cm) {                                                                                             \
        constexpr int NW = prox_waves(cm, nq);                                                                              \
        hipLaunchKernelGGL((linear_prox_kernel<nq, cm, NW>), dim3((unsigned)R), dim3(NW * 64), 0, s, a);                    \
        DBMM_CHECK_LAUNCH();                                                                                                \
        return DBMM_OK;                                                                                                     \
    }
#define DBMM_PROX_CM(nq) DBMM_PROX_CASE(nq, 2) DBMM_PROX_CASE(nq, 4) DBMM_PROX_CASE(nq, 8)
    DBMM_PROX_CM(1) DBMM_PROX_CM(2) DBMM_PROX_CM(3) DBMM_PROX_CM(4)
#undef DBMM_PROX_CM
#undef DBMM_PROX_CASE
    return DBMM_E_SHAPE;
}

}  // namespace

extern "C" int dbmm_linear_prox_fit(const float* table, int64_t n_rows, const int64_t* idx, const int64_t* labels, const float* lam,
                                    const float* step, float* w, float* b, float* v, float* c, double* t, float* stats, int64_t R,
                                    int64_t n, int64_t D, int64_t C, int64_t iters, int accelerate, void* stream) {
    if (!table || !idx || !labels || !lam || !step || !w || !b || !v || !c || !t || !stats) return DBMM_E_ARG;
    if (R < 1 || R > PROX_MAX_R || !lin_shape_ok(n, D, C) || n_rows < 1 || iters < 1 || iters > PROX_MAX_ITERS) return DBMM_E_SHAPE;
    if (!dbmm_aligned16(table) || !dbmm_aligned16(w) || !dbmm_aligned16(v) || !dbmm_aligned16(stats)) return DBMM_E_ALIGN;
    if ((((uintptr_t)idx) & 7u) || (((uintptr_t)labels) & 7u) || (((uintptr_t)t) & 7u)) return DBMM_E_ALIGN;
    ProxArgs a{};
    a.x = table; a.idx = (const long long*)idx; a.n_tab = n_rows; a.labels = (const long long*)labels;
    a.lam = lam; a.step = step;
    a.w = w; a.b = b; a.v = v; a.c = c; a.t = t; a.stats = stats;
    a.n = (int)n; a.D = (int)D; a.C = (int)C; a.iters = (int)iters; a.accelerate = accelerate != 0;
    return launch_prox(a, (int)R, (hipStream_t)stream);
}
