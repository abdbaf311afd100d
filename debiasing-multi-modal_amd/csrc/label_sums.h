// Per-label column sums of fp32 rows in float64 and their fixed-order merge, each stated ONCE for
//   kmeans_sums_kernel / kmeans_merge_kernel (kmeans.hip: int labels that the assignment wrote, a state gate, the dmin sum, the division) and
//   label_sums_kernel / label_merge_kernel   (erase.hip: int64 labels that nobody fitted, the raw sums).
// Two launches, no memset, no floating-point atomics:
//   - ranges: the partition.  P row ranges of `rows` rows from (N, D) ALONE, so two calls add the same numbers in the same order; a unit is
//     (range, slab of 256 columns), a wave takes one unit, a workgroup four.
//   - unit_sums<KP, LabelT>: a lane owns a float4 of the slab's columns and walks the range's rows in order, sixteen loads in flight.  FLOAT64
//     FROM THE FIRST ADD.  A row's label is wave-uniform and is compared IN LabelT with every j < KP: the row goes into acc[j] as
//     fma(w_j, x, acc[j]) with the scalar w_j = 1 under label == j and 0 otherwise -- 1 x v is v and + 0 x v changes no bit --, so these are KP
//     predicated adds on register-resident accumulators at one v_fma_f64 each: no dynamic register index, no branch in the loop.  (A row that
//     is not finite therefore reaches every label, not one.)  A label outside [0, G) matches no j < G: it is in no sum and no count.  There
//     is no fp32 chain, so covariance.hip's rule (none longer than 1024 rows) holds with nothing to fold.  fp32 accumulators, centred or
//     not, miss an entry near zero by many of ITS ulps when the rows' entries cancel; float64 ones give the rounding of the sum.
//     Writes the partials float64 [P][G][D] and, from lane 0 of the first slab's wave, the range's counts int64 [P][16].
//   - quarter_sums / merge_sum: a merge workgroup (256 threads, a lane per entry of one label's sum) adds the P partials in a fixed order:
//     each quarter of the ranges in range order by one wave, sixteen loads in flight, then the quarters in order.
//   - merge_count: a label's rows over all ranges (integers: the order does not matter).
#pragma once
#include "common.h"

namespace label_sums {

constexpr int SLAB_COLS = 256;             // columns of a wave: a float4 per lane
constexpr int UNITS = 2048;                // (range, column slab) units aimed at: eight waves per CU
constexpr int MIN_RANGE = 64;              // a row range is not cut below 64 rows
constexpr int DEPTH = 16;                  // rows in flight per wave of the sums, partials in flight per thread of the merge
constexpr int MAX_LABELS = 16;             // the count words of a range; KP = labels padded to 2 / 4 / 8 / 16 accumulators

typedef double f64x2 __attribute__((ext_vector_type(2)));

inline int slabs(long long D) { return (int)((D + SLAB_COLS - 1) / SLAB_COLS); }
// row ranges P and rows per range, from (N, D) alone
inline void ranges(long long N, long long D, int& P, int& rows) {
    const long long sl = slabs(D);
    long long p = (UNITS + sl - 1) / sl, cap = (N + MIN_RANGE - 1) / MIN_RANGE;
    p = p < cap ? p : cap;
    p = p < 1 ? 1 : p;
    P = (int)p;
    rows = (int)((N + p - 1) / p);
}
// bytes of the partial sums float64 [P][G][D] and of the partial counts int64 [P][16] that follow them
inline size_t part_bytes(int P, long long G, long long D) { return (size_t)P * G * D * 8; }
inline size_t count_bytes(int P) { return (size_t)P * MAX_LABELS * 8; }
inline unsigned sums_grid(int P, long long D) { return (unsigned)((P * slabs(D) + 3) / 4); }

// the unit of this wave (wave-uniform); units past P * slabs(D) have nothing to do
__device__ __forceinline__ int wave_unit() { return __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + (threadIdx.x >> 6)); }

struct Unit { int p, s, r0, r1; };         // range, column slab, the range's rows [r0, r1)

// unit < P * slabs: its partial sums of the G labels and, from the first slab, the range's counts
template <int KP, typename LabelT>
__device__ __forceinline__ Unit unit_sums(int unit, const float* __restrict__ x, const LabelT* __restrict__ labels, double* __restrict__ part,
                                          long long* __restrict__ cntp, int N, int D, int G, int rows, int n_slabs) {
    const int lane = threadIdx.x & 63;
    const int p = unit / n_slabs, s = unit - p * n_slabs;
    const int col = s * SLAB_COLS + lane * 4;
    const bool active = col < D;
    const int lcol = active ? col : 0;                                           // a lane past the last column loads column 0 and stores nothing
    const int r0 = (int)min((long long)p * rows, (long long)N), r1 = (int)min((long long)r0 + rows, (long long)N);
    double acc[KP][4];
    int cnt[KP];
#pragma unroll
    for (int j = 0; j < KP; ++j) {
        cnt[j] = 0;
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[j][e] = 0.0;
    }
    for (int r = r0; r < r1; r += DEPTH) {
        LabelT lab[DEPTH];
        f32x4 xv[DEPTH];
#pragma unroll
        for (int u = 0; u < DEPTH; ++u) {
            const int row = min(r + u, r1 - 1);                                  // past the end: a row read again and added nowhere
            lab[u] = r + u < r1 ? labels[row] : (LabelT)-1;                      // wave-uniform
            xv[u] = *(const f32x4*)(x + (size_t)row * D + lcol);
        }
#pragma unroll
        for (int u = 0; u < DEPTH; ++u) {
            const double v[4] = {(double)xv[u][0], (double)xv[u][1], (double)xv[u][2], (double)xv[u][3]};
#pragma unroll
            for (int j = 0; j < KP; ++j) {                                       // row order within every accumulator
                const bool hit = lab[u] == (LabelT)j;                            // in LabelT: as 64 bits, 2^32 + 1 is not label 1
                const double w = hit ? 1.0 : 0.0;                                // a scalar: 1 x v is v, and + 0 x v changes no bit
                cnt[j] += hit ? 1 : 0;
#pragma unroll
                for (int e = 0; e < 4; ++e) acc[j][e] = fma(w, v[e], acc[j][e]);
            }
        }
    }
    if (active) {
#pragma unroll
        for (int j = 0; j < KP; ++j) {
            if (j >= G) continue;
            f64x2* o = (f64x2*)(part + ((size_t)p * G + j) * D + col);           // (16-byte stores: the workspace's alignment)
            o[0] = (f64x2){acc[j][0], acc[j][1]};
            o[1] = (f64x2){acc[j][2], acc[j][3]};
        }
    }
    if (s == 0 && lane == 0) {
#pragma unroll
        for (int j = 0; j < KP; ++j) cntp[(size_t)p * MAX_LABELS + j] = cnt[j];  // the first column slab: the range's row counts (KP <= 16 words)
    }
    return Unit{p, s, r0, r1};
}

// The merge, in a workgroup of 256 threads whose lane owns entry `in` = part + j D + d of label j ([P] partials, `stride` = G D apart):
// wave w adds its quarter of the ranges in range order into quarter[w][lane]; ends in a barrier.
__device__ __forceinline__ void quarter_sums(const double* __restrict__ in, size_t stride, int P, double (&quarter)[4][64]) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int pq = (P + 3) / 4, p0 = min(w * pq, P), p1 = min(p0 + pq, P);
    double sum = 0.0;
    for (int b = p0; b < p1; b += DEPTH) {
        double v[DEPTH];
#pragma unroll
        for (int u = 0; u < DEPTH; ++u) v[u] = in[(size_t)min(b + u, p1 - 1) * stride];
#pragma unroll
        for (int u = 0; u < DEPTH; ++u)
            if (b + u < p1) sum += v[u];
    }
    quarter[w][lane] = sum;
    __syncthreads();
}
// ... and the quarters in order
__device__ __forceinline__ double merge_sum(const double (&quarter)[4][64], int lane) {
    return ((quarter[0][lane] + quarter[1][lane]) + quarter[2][lane]) + quarter[3][lane];
}

// rows of label j over all ranges: every thread of the workgroup gets the sum.  May be called in a loop with the same `red`.
__device__ __forceinline__ long long merge_count(const long long* __restrict__ cntp, int j, int P, long long (&red)[4]) {
    long long n = 0;
    for (int p = threadIdx.x; p < P; p += 256) n += cntp[(size_t)p * MAX_LABELS + j];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) n += __shfl_xor(n, o, 64);
    __syncthreads();                                                             // the previous call's sums have been read
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = n;
    __syncthreads();
    return red[0] + red[1] + red[2] + red[3];
}

}  // namespace label_sums
