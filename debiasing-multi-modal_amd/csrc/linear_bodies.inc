// Device bodies of the linear-probe step and its eval forward, shared by the single-run kernels (linear_step.hip) and the
// replica-batched ones (linear_sweep.hip).  A body takes the block coordinates it works for (`bid` of `nblk` row slices) instead of
// reading blockIdx / gridDim, so a replica-batched kernel is a wrapper that passes the coordinates of the single-run launch and the
// replica's operands: replica r gets the arithmetic -- lane ownership of the column quads, fmaf chains, butterfly wave sums, wave
// order inside a block, slab order across blocks -- and so the bits of the single run.  Included inside an anonymous namespace.
//
//   linear_rows_body<NQ, CM, MODE, SWEEP>   one wave per row (rows wave, wave + 4, ... of the block's row slice): the lane owns the
//                                      column quads lane, lane + 64, ... (NQ of them, D <= 256 NQ); logits by a butterfly wave sum
//                                      (every lane ends with the same bits), softmax / CE in registers; the wave accumulates dW
//                                      [CM][NQ] quads, db and the loss sum in registers.  The four waves are summed into LDS in wave
//                                      order and the block writes one slab: dW [C][D] | db [8] | loss sum, pad (pitch C D + 16).
//     MODE_STEP     at most 16 slabs; the last block to arrive sums the slabs in slab order and applies the update (one launch)
//     MODE_PARTIAL  up to 128 slabs, no update: linear_reduce_sgd_body does it, gridded over the C x D quads (two launches)
//     MODE_EVAL     no gradient: the slab is the block's loss sum, the last arriver writes the mean
//   WEIGHTED (MODE_STEP / MODE_PARTIAL): per-row loss weights a.row_w, indexed like the labels (batch row, or table row in a sweep): the
//   softmax-minus-one-hot term is scaled by invB * w where the unweighted form has invB, the loss sums take ce * w; logits and
//   loss_rows stay unweighted.  All-ones weights give the unweighted bits; the unweighted instantiation has no new operation.
//   SWEEP adds what a lock-step sweep needs and changes no float operation: batch row b is row idx[b] of a shared table (clamped
//   into it), read in place, with labels[idx[b]] / groups[idx[b]]; the (n, correct) group counters of the block's rows go to LDS and
//   from there to the replica's int64 counters (integer atomics: order-free); the thread that writes the loss mean adds
//   (double)mean * B to the float64 epoch loss sum; in MODE_EVAL the last arriver sums (double)loss_rows over the B rows in a fixed
//   order (thread-strided partial sums, then an LDS tree) and no float slab or mean is written.

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
    const float* row_w;                   // WEIGHTED: the weights of the rows `labels` indexes; else unused (null)
};

// what SWEEP adds, per replica: idx == nullptr: batch row b is row b of x / labels / groups (already offset to the first row)
struct LinSweepRows {
    const long long* idx; long long n_tab;
    const long long* groups; unsigned long long* counts; int G;
    double* loss_sum;
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
__device__ __forceinline__ void load_row(const float* __restrict__ x, long long row, int D4, int lane, f32x4 (&v)[NQ]) {
    const f32x4* xr = (const f32x4*)(x + row * (D4 * 4));
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
        v[q] = (f32x4){0.f, 0.f, 0.f, 0.f};
        if (q * 64 + lane < D4) v[q] = xr[q * 64 + lane];
    }
}

// batch row b -> row of x (and of labels / groups): the table row idx[b], clamped into the table, in a sweep with an index list
template <bool SWEEP>
__device__ __forceinline__ long long lin_row(const LinSweepRows& sw, int b) {
    if (SWEEP && sw.idx) {
        const long long s = sw.idx[b];
        return s < 0 ? 0 : (s >= sw.n_tab ? sw.n_tab - 1 : s);
    }
    return (long long)b;
}

// takes the block's ticket after its slab is stored; true in the block that arrived last of `nblk` (all its waves may then read
// every slab)
__device__ __forceinline__ bool arrive_last(unsigned* counter, int* flag, int nblk) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (threadIdx.x == 0) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const unsigned t = __hip_atomic_fetch_add(counter, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const int last = t == (unsigned)nblk - 1;
        if (last) {
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
        *flag = last;
    }
    __syncthreads();
    return *flag != 0;
}

// lds: W [C][D] while rows run; afterwards the block's dW [C][D] | db [8] | loss, pad (MODE_EVAL: the four wave loss sums)
//      (CM * NQ * 256 + 16 floats, 16-B aligned); sc: the block's group counters (SWEEP); red: 256 doubles (SWEEP, MODE_EVAL)
template <int NQ, int CM, int MODE, bool SWEEP, bool WEIGHTED = false>
__device__ __forceinline__ void linear_rows_body(const LinArgs& a, const LinSweepRows& sw, const int bid, const int nblk, float* lds, int* flag,
                                                 unsigned int (*sc)[2], double* red) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int D = a.D, D4 = D >> 2, C = a.C, B = a.B;
    const int r0 = bid * a.RB, r1 = min(B, r0 + a.RB);
    const bool count = SWEEP && sw.counts != nullptr;
    for (int i = threadIdx.x; i < C * D4; i += 256) ((f32x4*)lds)[i] = ((const f32x4*)a.w)[i];
    if (SWEEP && threadIdx.x < 64) { sc[threadIdx.x][0] = 0; sc[threadIdx.x][1] = 0; }
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
    long long srow = 0, srown = 0;                                       // SWEEP: the table rows of batch rows r and r + 4
    if (r < r1) {
        srow = lin_row<SWEEP>(sw, r);
        load_row<NQ>(a.x, SWEEP ? srow : (long long)r, D4, lane, xv);
    }
    for (; r < r1; r += 4) {
        f32x4 xn[NQ];
        if (r + 4 < r1) {                                                // next row in flight while this one is scored
            srown = lin_row<SWEEP>(sw, r + 4);
            load_row<NQ>(a.x, SWEEP ? srown : (long long)(r + 4), D4, lane, xn);
        }
        const long long row = SWEEP ? srow : (long long)r;
        const long long yl = a.labels[row];
        const int y = (yl >= 0 && yl < (long long)C) ? (int)yl : -1;     // the int64 label is compared: 2^32 + 1 is no class
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
        const float rw = WEIGHTED ? a.row_w[row] : 1.f;
        if (WEIGHTED) {
#pragma clang fp contract(off)
            lsum += ce * rw;                                             // the rounded term ce * w, in every instantiation
        } else {
            lsum += ce;
        }
        if (lane == 0) a.loss_rows[r] = ce;
        float lo = l[0];
#pragma unroll
        for (int c = 1; c < CM; ++c) if (lane == c) lo = l[c];
        if (lane < C) a.logits[(long long)r * C + lane] = lo;
        if (SWEEP) {
            // update_dict of the row: cm is group_count_kernel's argmax (the first maximum), compared with the int64 label
            if (count && lane == 0) {
                const long long gl = sw.groups[row];              // the int64 id is compared: 2^32 + k is no group
                if (gl >= 0 && gl < (long long)sw.G) {
                    atomicAdd(&sc[gl][0], 1u);
                    if ((long long)cm == yl) atomicAdd(&sc[gl][1], 1u);
                }
            }
        }
        if (MODE != MODE_EVAL) {
            const float inv = 1.f / se;
            if (WEIGHTED) {
                // The unweighted statements (the else branch) with invB * w for invB, written as the operations the compiler makes
                // of them -- e * inv - onehot is ONE fma, db += t * invB is ONE fma, d itself is the rounded product -- and with
                // contraction off, so that this instantiation cannot be contracted (or packed) into other roundings: all-ones
                // weights give the unweighted step's bits, which tests/test_gpu_row_weights.py holds on both launch paths.
#pragma clang fp contract(off)
                const float gs = invB * rw;
#pragma unroll
                for (int c = 0; c < CM; ++c) {
                    const float t = fmaf(e[c], inv, -(c == y ? 1.f : 0.f));
                    const float d = t * gs;
                    db[c] = fmaf(t, gs, db[c]);
#pragma unroll
                    for (int q = 0; q < NQ; ++q) {
                        dw[c][q][0] = fmaf(d, xv[q][0], dw[c][q][0]);
                        dw[c][q][1] = fmaf(d, xv[q][1], dw[c][q][1]);
                        dw[c][q][2] = fmaf(d, xv[q][2], dw[c][q][2]);
                        dw[c][q][3] = fmaf(d, xv[q][3], dw[c][q][3]);
                    }
                }
            } else {
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
        }
#pragma unroll
        for (int q = 0; q < NQ; ++q) xv[q] = xn[q];
        srow = srown;
    }
    __syncthreads();                                                     // every wave is done with W in LDS
    if (SWEEP) {
        if (count && (int)threadIdx.x < sw.G) {
            if (sc[threadIdx.x][0]) atomicAdd(&sw.counts[threadIdx.x * 2], (unsigned long long)sc[threadIdx.x][0]);
            if (sc[threadIdx.x][1]) atomicAdd(&sw.counts[threadIdx.x * 2 + 1], (unsigned long long)sc[threadIdx.x][1]);
        }
    }

    if (MODE == MODE_EVAL) {
        if (SWEEP) {
            // validate()'s loss_sum += rows.double().sum(): the last arriver sums the B per-row losses of the replica
            if (!arrive_last(a.counter, flag, nblk)) return;
            double s = 0.0;
            for (int b = threadIdx.x; b < B; b += 256) s += (double)a.loss_rows[b];
            red[threadIdx.x] = s;
            __syncthreads();
            for (int o = 128; o > 0; o >>= 1) {
                if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
                __syncthreads();
            }
            if (threadIdx.x == 0) {
                *sw.loss_sum += red[0];
                *a.counter = 0u;
            }
            return;
        }
        if (lane == 0) lds[wave] = lsum;
        __syncthreads();
        if (threadIdx.x == 0) a.slabs[bid] = ((lds[0] + lds[1]) + lds[2]) + lds[3];
        if (!arrive_last(a.counter, flag, nblk)) return;
        if (threadIdx.x == 0) {
            float s = 0.f;
            for (int i = 0; i < nblk; ++i) s += a.slabs[i];
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
    f32x4* slab = (f32x4*)(a.slabs + bid * pitch);
    for (int i = threadIdx.x; i < (CD + 16) / 4; i += 256) slab[i] = ((const f32x4*)lds)[i];
    if (MODE == MODE_PARTIAL) return;
    if (!arrive_last(a.counter, flag, nblk)) return;

    // the last arriver: slab sums in slab order, then the update
    const int NS = nblk;
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
        const float mean = s * invB;
        *a.loss_mean = mean;
        if (SWEEP && sw.loss_sum) *sw.loss_sum += (double)mean * (double)B;      // losses.update(loss.item(), bsz) on the device
    } else if (threadIdx.x == 128) {
        *a.counter = 0u;
    }
}

// two-launch path: thread i < C D / 4 (i = bid * 256 + threadIdx.x) sums the dW quad i over the NS slabs (slab order) and updates
// W / its momentum; the thread after them does db, b and the loss mean
template <bool SWEEP>
__device__ __forceinline__ void linear_reduce_sgd_body(const LinArgs& a, double* loss_sum, int NS, int bid) {
    const int CD = a.C * a.D;
    const long long pitch = (long long)CD + 16;
    const int i = bid * 256 + threadIdx.x;
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
        const float mean = s / (float)a.B;
        *a.loss_mean = mean;
        if (SWEEP && loss_sum) *loss_sum += (double)mean * (double)a.B;
    }
}

// row slices: at least `min_rows` rows per block, at most `max_slabs` blocks
inline void row_split(int64_t B, int min_rows, int max_slabs, int* NS, int* RB) {
    int64_t ns = (B + min_rows - 1) / min_rows;
    if (ns > max_slabs) ns = max_slabs;
    const int64_t rb = (B + ns - 1) / ns;
    *RB = (int)rb;
    *NS = (int)((B + rb - 1) / rb);
}
inline void split_step1(int64_t B, int* NS, int* RB) { row_split(B, 16, LS_MAX_SLABS, NS, RB); }
inline void split_step2(int64_t B, int* NS, int* RB) { row_split(B, 64, LS_MAX_SLABS2, NS, RB); }
inline void split_eval(int64_t B, int* NS, int* RB) { row_split(B, 16, LS_MAX_SLABS_EVAL, NS, RB); }

inline bool lin_shape_ok(int64_t B, int64_t D, int64_t C) {
    return B >= 1 && B <= INT32_MAX / 8 && D >= 4 && D <= 1024 && (D % 4) == 0 && C >= 1 && C <= 8;
}
