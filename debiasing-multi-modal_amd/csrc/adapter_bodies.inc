// Device bodies of the adapter-step kernels, shared by the single-run kernels (adapter_step.hip, adapter_ops.hip) and the
// replica-batched ones (adapter_sweep.hip): a kernel of either family is a thin __global__ wrapper that picks its operands and its
// block coordinates (`bi` / `gd` stand for blockIdx / gridDim of the single-run launch) and calls the body, so both families run
// the same statements in the same order and give the same bits.  Include inside an anonymous namespace, after common.h.
//
// GATHER bodies read batch row b from `x + idx[b] * D` (rows of an embedding table) instead of `x + b * D`.

constexpr int LP = 132;                    // LDS row pitch in floats

constexpr int TB = 16, TI = TB / 8;        // rows of a tile product's output tile, rows per thread

// acc[i][j] += sum_k a[row_i][k] * w[col_j][k] over 128 k, both operands as [rows][LP] in LDS; rows ty + 8 i, cols tx + 32 j
template <int RI, int CJ>
__device__ __forceinline__ void tile_kk(const float* __restrict__ as, const float* __restrict__ ws, int tx, int ty, float (&acc)[RI][CJ]) {
#pragma unroll 4
    for (int k4 = 0; k4 < 32; ++k4) {
        f32x4 a[RI], w[CJ];
#pragma unroll
        for (int i = 0; i < RI; ++i) a[i] = *(const f32x4*)(as + (ty + 8 * i) * LP + 4 * k4);
#pragma unroll
        for (int j = 0; j < CJ; ++j) w[j] = *(const f32x4*)(ws + (tx + 32 * j) * LP + 4 * k4);
#pragma unroll
        for (int i = 0; i < RI; ++i)
#pragma unroll
            for (int j = 0; j < CJ; ++j) {
                acc[i][j] = fmaf(a[i][0], w[j][0], acc[i][j]);
                acc[i][j] = fmaf(a[i][1], w[j][1], acc[i][j]);
                acc[i][j] = fmaf(a[i][2], w[j][2], acc[i][j]);
                acc[i][j] = fmaf(a[i][3], w[j][3], acc[i][j]);
            }
    }
}

// rows [r0, r0 + TB) x columns [c0, c0 + 128) of a row-major [n_rows][ld] matrix -> LDS [TB][LP] (rows past n_rows: zeros)
__device__ __forceinline__ void load_tileTB(const float* __restrict__ src, long long ld, int r0, int n_rows, int c0, float* __restrict__ dst, int tid) {
#pragma unroll
    for (int i = 0; i < TB / 8; ++i) {
        const int q = tid + 256 * i, r = q >> 5, c = q & 31;
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (r0 + r < n_rows) v = *(const f32x4*)(src + (long long)(r0 + r) * ld + c0 + 4 * c);
        *(f32x4*)(dst + r * LP + 4 * c) = v;
    }
}
// rows [r0, r0 + 32) x columns [c0, c0 + 128) of a row-major [n_rows][ld] matrix -> LDS [32][LP] (rows past n_rows: zeros)
__device__ __forceinline__ void load_tile32(const float* __restrict__ src, long long ld, int r0, int n_rows, int c0, float* __restrict__ dst, int tid) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int q = tid + 256 * i, r = q >> 5, c = q & 31;
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (r0 + r < n_rows) v = *(const f32x4*)(src + (long long)(r0 + r) * ld + c0 + 4 * c);
        *(f32x4*)(dst + r * LP + 4 * c) = v;
    }
}
// row idx[b] of a table of n_tab rows, clamped into the table like gather_rows_kernel does (a bad index never reads out of bounds)
__device__ __forceinline__ long long table_row(const long long* __restrict__ idx, int b, long long n_tab) {
    const long long s = idx[b];
    return s < 0 ? 0 : (s >= n_tab ? n_tab - 1 : s);
}
// load_tile32 of the rows idx[r0 ..] of a table (the replica-batched step reads its batch straight from the embedding table)
__device__ __forceinline__ void gather_tile32(const float* __restrict__ src, const long long* __restrict__ idx, long long n_tab, long long ld, int r0,
                                              int n_rows, int c0,
                                              float* __restrict__ dst, int tid) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int q = tid + 256 * i, r = q >> 5, c = q & 31;
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (r0 + r < n_rows) v = *(const f32x4*)(src + table_row(idx, r0 + r, n_tab) * ld + c0 + 4 * c);
        *(f32x4*)(dst + r * LP + 4 * c) = v;
    }
}
// rows [r0, r0 + 64) x columns [c0, c0 + 128) -> LDS [64][LP]
__device__ __forceinline__ void load_tile64(const float* __restrict__ src, long long ld, int r0, int c0, float* __restrict__ dst, int tid) {
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int q = tid + 256 * i, r = q >> 5, c = q & 31;
        *(f32x4*)(dst + r * LP + 4 * c) = *(const f32x4*)(src + (long long)(r0 + r) * ld + c0 + 4 * c);
    }
}
// rows [r0, r0 + 128) x columns [c0, c0 + 128) -> LDS [128][LP]
__device__ __forceinline__ void load_tile128(const float* __restrict__ src, long long ld, int r0, int c0, float* __restrict__ dst, int tid) {
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const int q = tid + 256 * i, r = q >> 5, c = q & 31;
        *(f32x4*)(dst + r * LP + 4 * c) = *(const f32x4*)(src + (long long)(r0 + r) * ld + c0 + 4 * c);
    }
}

template <bool GATHER>
__device__ __forceinline__ void fc1_partial_body(const dim3 bi, const dim3 gd, const float* __restrict__ x, const long long* __restrict__ idx, long long n_tab, const float* __restrict__ w1, float* __restrict__ part,
                                                          int B, int D) {
    // tile = 32 rows x 64 hidden units over a 128-deep K slice (24 KB + 32 KB of operands per workgroup)
    __shared__ __attribute__((aligned(16))) float as[32 * LP];
    __shared__ __attribute__((aligned(16))) float ws[64 * LP];
    const int tid = threadIdx.x, tx = tid & 31, ty = tid >> 5;
    const int b0 = bi.x * 32, h0 = bi.y * 64, ks = bi.z;
    if (GATHER) gather_tile32(x, idx, n_tab, D, b0, B, ks * 128, as, tid);
    else load_tile32(x, D, b0, B, ks * 128, as, tid);
    load_tile64(w1, D, h0, ks * 128, ws, tid);
    __syncthreads();
    float acc[4][2] = {};
    tile_kk<4, 2>(as, ws, tx, ty, acc);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int b = b0 + ty + 8 * i;
        if (b < B)
#pragma unroll
            for (int j = 0; j < 2; ++j) part[((long long)ks * B + b) * 128 + h0 + tx + 32 * j] = acc[i][j];
    }
}

// 4 columns x 64 row-lanes per workgroup (thread = column tid & 3, row-lane tid >> 2); sums over the batch: per row-lane
// sequentially, then a fixed butterfly over the 16 row-lanes of a wave (lane bits 2 .. 5), then the 4 waves in order
__device__ __forceinline__ float lanes64_sum(float (*red)[4], int c, int rl, float v) {
#pragma unroll
    for (int o = 4; o < 64; o <<= 1) v += __shfl_xor(v, o, 64);
    __syncthreads();
    if ((threadIdx.x & 63) < 4) red[threadIdx.x >> 6][c] = v;
    __syncthreads();
    (void)rl;
    return ((red[0][c] + red[1][c]) + red[2][c]) + red[3][c];
}

// v[u] += sum_ks part[ks][b + 64 u][j] (ks in order) for the four rows of a row-lane: the loads of eight slices x four rows are
// issued together (a loop that adds each load before issuing the next pays one memory round trip per slice)
__device__ __forceinline__ void ksum4(const float* __restrict__ part, int KS, int B, int b, int j, float (&v)[4]) {
    long long off[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) off[u] = (long long)(b + 64 * u < B ? b + 64 * u : B - 1) * 128 + j;       // clamped: branch-free loads
    for (int k0 = 0; k0 < KS; k0 += 8) {
        float t[8][4];
#pragma unroll
        for (int kk = 0; kk < 8; ++kk) {
            const long long base = (long long)(k0 + kk < KS ? k0 + kk : KS - 1) * B * 128;
#pragma unroll
            for (int u = 0; u < 4; ++u) t[kk][u] = part[base + off[u]];
        }
#pragma unroll
        for (int kk = 0; kk < 8; ++kk)
            if (k0 + kk < KS)
#pragma unroll
                for (int u = 0; u < 4; ++u) v[u] += t[kk][u];
    }
}

__device__ __forceinline__ void bn_stats_body(const dim3 bi, const dim3 gd, const float* __restrict__ part, int KS, const float* __restrict__ b1, float* __restrict__ h,
                                                       int B, float eps, float momentum, float* __restrict__ mean_o, float* __restrict__ invstd_o,
                                                       float* __restrict__ rmean, float* __restrict__ rvar, long long* __restrict__ nbt) {
    __shared__ float red[64][4];
    const int c = threadIdx.x & 3, rl = threadIdx.x >> 2, j = bi.x * 4 + c;
    const float bj = b1[j];
    float s = 0.f;
    float v[4];
    // four rows of this row-lane at a time: 4 KS independent loads in flight (the loop is latency-bound, not bandwidth-bound)
    for (int b = rl; b < B; b += 256) {
        v[0] = v[1] = v[2] = v[3] = bj;
        ksum4(part, KS, B, b, j, v);
#pragma unroll
        for (int u = 0; u < 4; ++u)
            if (b + 64 * u < B) { h[(long long)(b + 64 * u) * 128 + j] = v[u]; s += v[u]; }
    }
    const float mean = lanes64_sum(red, c, rl, s) / (float)B;
    float q = 0.f;
    if (B <= 256) {                                          // the only row group is still in registers
#pragma unroll
        for (int u = 0; u < 4; ++u)
            if (rl + 64 * u < B) { const float d = v[u] - mean; q = fmaf(d, d, q); }
    } else {
#pragma unroll 4
        for (int b = rl; b < B; b += 64) { const float d = h[(long long)b * 128 + j] - mean; q = fmaf(d, d, q); }
    }
    const float var = lanes64_sum(red, c, rl, q) / (float)B;
    if (rl == 0) {
        mean_o[j] = mean;
        invstd_o[j] = rsqrtf(var + eps);
        if (rmean) rmean[j] = (1.f - momentum) * rmean[j] + momentum * mean;
        if (rvar) rvar[j] = (1.f - momentum) * rvar[j] + momentum * (var * (float)B / (float)(B - 1));
    }
    if (nbt && bi.x == 0 && threadIdx.x == 0) *nbt += 1;
}

// eval mode: h = b1 + sum_ks part (no statistics)
__device__ __forceinline__ void fc1_reduce_body(const dim3 bi, const dim3 gd, const float* __restrict__ part, int KS, const float* __restrict__ b1, float* __restrict__ h,
                                                         long long total, int B) {
    const long long i = (long long)bi.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int j = (int)(i & 127);
    const long long b = i >> 7;
    float v = b1[j];
    for (int ks = 0; ks < KS; ++ks) v += part[((long long)ks * B + b) * 128 + j];
    h[i] = v;
}

__device__ __forceinline__ void fc2_body(const dim3 bi, const dim3 gd, const float* __restrict__ h, const float* __restrict__ mean, const float* __restrict__ invstd,
                                                  int var_mode, float eps, const float* __restrict__ gamma, const float* __restrict__ beta,
                                                  const float* __restrict__ w2, const float* __restrict__ b2, float* __restrict__ r,
                                                  float* __restrict__ z, int B, int D) {
    // tile = 32 rows x 64 output columns, K = H = 128 (the whole reduction)
    __shared__ __attribute__((aligned(16))) float as[32 * LP];
    __shared__ __attribute__((aligned(16))) float ws[64 * LP];
    const int tid = threadIdx.x, tx = tid & 31, ty = tid >> 5;
    const int b0 = bi.x * 32, d0 = bi.y * 64;
    // r tile = relu(bn(h tile)): the expression of the stand-alone BatchNorm + ReLU kernel (bn1d_relu_kernel)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int q = tid + 256 * i, rr = q >> 5, c = q & 31;
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (b0 + rr < B) {
            f32x4 is = ((const f32x4*)invstd)[c];
            if (var_mode) {
#pragma unroll
                for (int k = 0; k < 4; ++k) is[k] = rsqrtf(is[k] + eps);
            }
            v = (*(const f32x4*)(h + (long long)(b0 + rr) * 128 + 4 * c) - ((const f32x4*)mean)[c]) * is * ((const f32x4*)gamma)[c] + ((const f32x4*)beta)[c];
#pragma unroll
            for (int k = 0; k < 4; ++k) v[k] = fmaxf(v[k], 0.f);
            if (bi.y == 0) *(f32x4*)(r + (long long)(b0 + rr) * 128 + 4 * c) = v;
        }
        *(f32x4*)(as + rr * LP + 4 * c) = v;
    }
    load_tile64(w2, 128, d0, 0, ws, tid);                  // W2 [D][128]: rows d0 .. d0 + 63
    __syncthreads();
    float acc[4][2] = {};
    tile_kk<4, 2>(as, ws, tx, ty, acc);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int b = b0 + ty + 8 * i;
        if (b < B)
#pragma unroll
            for (int j = 0; j < 2; ++j) z[(long long)b * D + d0 + tx + 32 * j] = acc[i][j] + b2[d0 + tx + 32 * j];
    }
}

// blocks [0, NS D / 32): split s = bid / (D / 32) of the batch: dw2part[s][d0 .. d0 + 31][:] = sum_{b in split} dz[b][d] r[b][:],
//                         db2part[s][d] = sum_{b in split} dz[b][d]           (summed over s, in order, by grad_reduce blocks)
// the other blocks:       drpart[ks][b0 .. b0 + 31][:] = dz[b][128 ks ..] . W2[128 ks ..][:]
// one more block, when loss_mean is given: the batch mean of the per-row losses (mean_reduce_kernel's statements)
__device__ __forceinline__ void bwd2_body(const dim3 bi, const dim3 gd, const float* __restrict__ dz, const float* __restrict__ r, const float* __restrict__ w2,
                                                   float* __restrict__ dw2part, float* __restrict__ db2part, float* __restrict__ drpart, int B, int D,
                                                   int NS, int RB, const float* __restrict__ loss_rows, float* __restrict__ loss_mean) {
    __shared__ __attribute__((aligned(16))) float s0[32 * LP];
    __shared__ __attribute__((aligned(16))) float s1[128 * LP];
    const int tid = threadIdx.x;
    const int nd = D / 32;
    if (loss_mean && bi.x == gd.x - 1) {
        float s = 0.f;
        for (int i = threadIdx.x; i < B; i += 256) s += loss_rows[i];
        s = wave_sum(s);
        if ((threadIdx.x & 63) == 0) s0[threadIdx.x >> 6] = s;
        __syncthreads();
        if (threadIdx.x == 0) *loss_mean = ((s0[0] + s0[1]) + (s0[2] + s0[3])) / (float)B;
        return;
    }
    if ((int)bi.x < nd * NS) {
        const int sp = bi.x / nd, d0 = (bi.x % nd) * 32, td = tid & 7, th = tid >> 3;   // register tile: d = 4 td .., h = 4 th ..
        const int bb = sp * RB, be = bb + RB < B ? bb + RB : B;
        float acc[4][4] = {};
        f32x4 cs = {0.f, 0.f, 0.f, 0.f};
        float* dzs = s1;                                                         // [32 b][36]
        for (int bc = bb; bc < be; bc += 32) {
            __syncthreads();
            {   // dz chunk [32 b][32 d]: one float4 per thread
                const int rr = tid >> 3, c = tid & 7;
                f32x4 v = {0.f, 0.f, 0.f, 0.f};
                if (bc + rr < be) v = *(const f32x4*)(dz + (long long)(bc + rr) * D + d0 + 4 * c);
                *(f32x4*)(dzs + rr * 36 + 4 * c) = v;
            }
            load_tile32(r, 128, bc, be, 0, s0, tid);                             // r chunk [32 b][128 h]
            __syncthreads();
#pragma unroll 8
            for (int b = 0; b < 32; ++b) {
                const f32x4 dv = *(const f32x4*)(dzs + b * 36 + 4 * td), rv = *(const f32x4*)(s0 + b * LP + 4 * th);
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int j = 0; j < 4; ++j) acc[i][j] = fmaf(dv[i], rv[j], acc[i][j]);
                cs += dv;
            }
        }
        float* o = dw2part + (long long)sp * D * 128;
#pragma unroll
        for (int i = 0; i < 4; ++i)
            *(f32x4*)(o + (long long)(d0 + 4 * td + i) * 128 + 4 * th) = (f32x4){acc[i][0], acc[i][1], acc[i][2], acc[i][3]};
        if (th == 0) *(f32x4*)(db2part + (long long)sp * D + d0 + 4 * td) = cs;
    } else {
        const int bid = bi.x - nd * NS, nbt = (B + TB - 1) / TB, ks = bid / nbt, b0 = (bid % nbt) * TB;
        const int tx = tid & 31, ty = tid >> 5;
        load_tileTB(dz, D, b0, B, ks * 128, s0, tid);                            // dz[b][d slice]
        load_tile128(w2, 128, ks * 128, 0, s1, tid);                             // W2[d slice][h]: rows are the REDUCTION index
        __syncthreads();
        // dr[b][h] = sum_d dz[b][d] W2[d][h]; rows ty + 8 i, columns 4 tx .. 4 tx + 3
        float acc[TI][4] = {};
#pragma unroll 4
        for (int k4 = 0; k4 < 32; ++k4) {
            f32x4 a[TI], w[4];
#pragma unroll
            for (int i = 0; i < TI; ++i) a[i] = *(const f32x4*)(s0 + (ty + 8 * i) * LP + 4 * k4);
#pragma unroll
            for (int kk = 0; kk < 4; ++kk) w[kk] = *(const f32x4*)(s1 + (4 * k4 + kk) * LP + 4 * tx);
#pragma unroll
            for (int i = 0; i < TI; ++i)
#pragma unroll
                for (int kk = 0; kk < 4; ++kk)
#pragma unroll
                    for (int j = 0; j < 4; ++j) acc[i][j] = fmaf(a[i][kk], w[kk][j], acc[i][j]);
        }
#pragma unroll
        for (int i = 0; i < TI; ++i) {
            const int b = b0 + ty + 8 * i;
            if (b < B) *(f32x4*)(drpart + ((long long)ks * B + b) * 128 + 4 * tx) = (f32x4){acc[i][0], acc[i][1], acc[i][2], acc[i][3]};
        }
    }
}

// per-row loss weights: one workgroup writes L = (1 / B) sum_b loss_rows[b] * row_w[row(b)] -- mean_reduce_kernel's statements (and
// those of bwd2_body's spare block) over the weighted terms, so all-ones weights give the ERM mean's bits.  row(b) = b, or with `idx`
// the table row idx[b] clamped into a table of n_tab rows (the sweep's weights are per table row).  `red`: 4 floats of LDS
__device__ __forceinline__ void weighted_mean_body(const float* __restrict__ loss_rows, const float* __restrict__ row_w, const long long* __restrict__ idx,
                                                   long long n_tab, int B, float* red, float* __restrict__ loss_mean) {
#pragma clang fp contract(off)                                           // the rounded terms loss_rows[b] * w, in every kernel that calls this
    float s = 0.f;
    for (int i = threadIdx.x; i < B; i += 256) s += loss_rows[i] * row_w[idx ? table_row(idx, i, n_tab) : (long long)i];
    s = wave_sum(s);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) *loss_mean = ((red[0] + red[1]) + (red[2] + red[3])) / (float)B;
}

// train-mode BatchNorm backward, 4 columns x 64 row-lanes per workgroup:
// dr = sum_ks drpart; dhn = dr * (gamma xhat + beta > 0); dbeta = sum_b dhn; dgamma = sum_b dhn xhat;
// dh = gamma invstd (dhn - dbeta / B - xhat dgamma / B)
// (blocks >= 32 of the same launch sum the batch splits of dW2 / db2, which only bwd2 precedes)
__device__ __forceinline__ void bn_bwd_body(const dim3 bi, const dim3 gd, const float* __restrict__ drpart, int KS, const float* __restrict__ h, const float* __restrict__ mean,
                                                     const float* __restrict__ invstd, const float* __restrict__ gamma, const float* __restrict__ beta,
                                                     float* __restrict__ dgamma, float* __restrict__ dbeta, float* __restrict__ dh, int B,
                                                     const float* __restrict__ dw2part, float* __restrict__ dw2, long long nw4,
                                                     const float* __restrict__ db2part, float* __restrict__ db2, long long nb4, int NS) {
    __shared__ float red[64][4];
    if (bi.x >= 32) {
        const long long i = (long long)(bi.x - 32) * 256 + threadIdx.x;
        const float* p; float* o; long long n4, k;
        if (i < nw4) { p = dw2part; o = dw2; n4 = nw4; k = i; }
        else if (i < nw4 + nb4) { p = db2part; o = db2; n4 = nb4; k = i - nw4; }
        else return;
        f32x4 v = ((const f32x4*)p)[k];
        for (int sidx = 1; sidx < NS; ++sidx) v += ((const f32x4*)p)[(long long)sidx * n4 + k];
        ((f32x4*)o)[k] = v;
        return;
    }
    const int c = threadIdx.x & 3, rl = threadIdx.x >> 2, j = bi.x * 4 + c;
    const float mu = mean[j], is = invstd[j], ga = gamma[j], be = beta[j];
    float sb = 0.f, sg = 0.f;
    float dn[4] = {0.f, 0.f, 0.f, 0.f}, xh[4] = {0.f, 0.f, 0.f, 0.f};
    for (int b = rl; b < B; b += 256) {
        float d[4] = {0.f, 0.f, 0.f, 0.f}, hv[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int u = 0; u < 4; ++u)
            if (b + 64 * u < B) hv[u] = h[(long long)(b + 64 * u) * 128 + j];
        ksum4(drpart, KS, B, b, j, d);
#pragma unroll
        for (int u = 0; u < 4; ++u)
            if (b + 64 * u < B) {
                xh[u] = (hv[u] - mu) * is;
                dn[u] = (fmaf(ga, xh[u], be) > 0.f) ? d[u] : 0.f;
                if (B > 256) dh[(long long)(b + 64 * u) * 128 + j] = dn[u];   // dhn for now; finished below by the same thread
                sb += dn[u];
                sg = fmaf(dn[u], xh[u], sg);
            }
    }
    const float db = lanes64_sum(red, c, rl, sb), dg = lanes64_sum(red, c, rl, sg);
    if (rl == 0) { dbeta[j] = db; dgamma[j] = dg; }
    const float invB = 1.f / (float)B;
    if (B <= 256) {                                          // the only row group is still in registers
#pragma unroll
        for (int u = 0; u < 4; ++u)
            if (rl + 64 * u < B) dh[(long long)(rl + 64 * u) * 128 + j] = ga * is * (dn[u] - db * invB - xh[u] * dg * invB);
    } else {
        for (int b = rl; b < B; b += 64) {
            const float xhb = (h[(long long)b * 128 + j] - mu) * is;
            const float d = dh[(long long)b * 128 + j];
            dh[(long long)b * 128 + j] = ga * is * (d - db * invB - xhb * dg * invB);
        }
    }
}

// split s = blockIdx.y of the batch: dw1part[s][:, d0 .. d0 + 31] = sum_{b in split} dh[b][:]^T x[b][d0 ..]; blockIdx.x == 0 also
// db1part[s] = sum_{b in split} dh[b][:]
template <bool GATHER>
__device__ __forceinline__ void bwd1_body(const dim3 bi, const dim3 gd, const float* __restrict__ dh, const float* __restrict__ x, const long long* __restrict__ idx, long long n_tab, float* __restrict__ dw1part,
                                                   float* __restrict__ db1part, int B, int D, int RB) {
    __shared__ __attribute__((aligned(16))) float dhs[32 * LP];
    __shared__ __attribute__((aligned(16))) float xs[32 * 36];
    const int tid = threadIdx.x, td = tid & 7, th = tid >> 3;                    // register tile: h = 4 th .., d = 4 td ..
    const int d0 = bi.x * 32, sp = bi.y;
    const int bb = sp * RB, be = bb + RB < B ? bb + RB : B;
    float acc[4][4] = {};
    f32x4 cs = {0.f, 0.f, 0.f, 0.f};
    for (int bc = bb; bc < be; bc += 32) {
        __syncthreads();
        {
            const int rr = tid >> 3, c = tid & 7;
            f32x4 v = {0.f, 0.f, 0.f, 0.f};
            if (bc + rr < be) v = *(const f32x4*)(x + (GATHER ? table_row(idx, bc + rr, n_tab) : (long long)(bc + rr)) * D + d0 + 4 * c);
            *(f32x4*)(xs + rr * 36 + 4 * c) = v;
        }
        load_tile32(dh, 128, bc, be, 0, dhs, tid);
        __syncthreads();
#pragma unroll 8
        for (int b = 0; b < 32; ++b) {
            const f32x4 hv = *(const f32x4*)(dhs + b * LP + 4 * th), xv = *(const f32x4*)(xs + b * 36 + 4 * td);
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[i][j] = fmaf(hv[i], xv[j], acc[i][j]);
            cs += hv;
        }
    }
    float* o = dw1part + (long long)sp * 128 * D;
#pragma unroll
    for (int i = 0; i < 4; ++i)
        *(f32x4*)(o + (long long)(4 * th + i) * D + d0 + 4 * td) = (f32x4){acc[i][0], acc[i][1], acc[i][2], acc[i][3]};
    if (bi.x == 0 && td == 0) *(f32x4*)(db1part + (long long)sp * 128 + 4 * th) = cs;
}

// out[i] = sum_s part[s][i] in the order s = 0, 1, ...: two tensors per launch (a weight gradient and its bias gradient)
__device__ __forceinline__ void grad_reduce_body(const dim3 bi, const dim3 gd, const float* __restrict__ pa, float* __restrict__ oa, long long na4,
                                                          const float* __restrict__ pb, float* __restrict__ ob, long long nb4, int NS) {
    const long long i = (long long)bi.x * 256 + threadIdx.x;
    const float* p; float* o; long long n4, k;
    if (i < na4) { p = pa; o = oa; n4 = na4; k = i; }
    else if (i < na4 + nb4) { p = pb; o = ob; n4 = nb4; k = i - na4; }
    else return;
    f32x4 v = ((const f32x4*)p)[k];
    for (int sidx = 1; sidx < NS; ++sidx) v += ((const f32x4*)p)[(long long)sidx * n4 + k];
    ((f32x4*)o)[k] = v;
}


// ---- fused row L2-norm + logits + CE: one wave per row -------------------------------------
// forward of one row by one wave (every lane ends up with the row's logits lg[] and 1 / ||z||); lane 0 writes the outputs
template <int CMAX>
__device__ __forceinline__ void ce_fwd_row(const float* __restrict__ z, const float* __restrict__ z_old, float w_old, const float* __restrict__ tn,
                                           const long long* __restrict__ labels, float invT, float* __restrict__ logits,
                                           float* __restrict__ loss_rows, long long* __restrict__ pred, float* __restrict__ inv_norm, int row,
                                           int lane, int D4, int C, float (&lg)[CMAX], float& inv, long long lrow) {
    const f32x4* zr = (const f32x4*)z + (long long)row * D4;
    const f32x4* zo = z_old ? (const f32x4*)z_old + (long long)row * D4 : nullptr;
    float ss = 0.f, sso = 0.f, dot[CMAX], doto[CMAX];
#pragma unroll
    for (int c = 0; c < CMAX; ++c) { dot[c] = 0.f; doto[c] = 0.f; }
    for (int i = lane; i < D4; i += 64) {
        const f32x4 v = zr[i];
        ss += (v[0] * v[0] + v[1] * v[1]) + (v[2] * v[2] + v[3] * v[3]);
        f32x4 vo = {0.f, 0.f, 0.f, 0.f};
        if (zo) { vo = zo[i]; sso += (vo[0] * vo[0] + vo[1] * vo[1]) + (vo[2] * vo[2] + vo[3] * vo[3]); }
#pragma unroll
        for (int c = 0; c < CMAX; ++c) {
            if (c < C) {
                const f32x4 t = ((const f32x4*)tn)[(long long)c * D4 + i];
                dot[c] += (v[0] * t[0] + v[1] * t[1]) + (v[2] * t[2] + v[3] * t[3]);
                if (zo) doto[c] += (vo[0] * t[0] + vo[1] * t[1]) + (vo[2] * t[2] + vo[3] * t[3]);
            }
        }
    }
    ss = wave_sum(ss);
    inv = 1.f / sqrtf(ss);
    float invo = 0.f;
    if (zo) invo = 1.f / sqrtf(wave_sum(sso));
    float mx = -INFINITY;
    int am = 0;
#pragma unroll
    for (int c = 0; c < CMAX; ++c) {
        lg[c] = -INFINITY;
        if (c < C) {
            const float d = wave_sum(dot[c]) * inv;
            float f = d;
            if (zo) f = w_old * (wave_sum(doto[c]) * invo) + (1.f - w_old) * d;
            lg[c] = f * invT;
            if (lg[c] > mx) { mx = lg[c]; am = c; }
        }
    }
    if (lane == 0) {
        if (inv_norm) inv_norm[row] = inv;
        if (logits) for (int c = 0; c < C; ++c) logits[(long long)row * C + c] = lg[c];
        if (pred) pred[row] = am;
        if (loss_rows && labels) {
            float se = 0.f;
#pragma unroll
            for (int c = 0; c < CMAX; ++c) if (c < C) se += expf(lg[c] - mx);
            const long long yl = labels[lrow];
            const int y = (yl >= 0 && yl < (long long)C) ? (int)yl : -1;     // the int64 label is compared: 2^32 + 1 is no class
            float ly = __builtin_nanf("");                                   // a label outside [0, C) scores NaN
#pragma unroll
            for (int c = 0; c < CMAX; ++c) if (c == y) ly = lg[c];
            loss_rows[row] = (mx + logf(se)) - ly;
        }
    }
}

// backward of one row by one wave: dz from the row's logits `lgv` (read back or still in registers), its label and 1 / ||z||
template <int CMAX>
__device__ __forceinline__ void ce_bwd_row(const float* __restrict__ z, float inv, float w_new, const float* __restrict__ tn, const float (&lgv)[CMAX],
                                           const long long* __restrict__ labels, const float* __restrict__ dlogits, float invT, float gscale,
                                           float* __restrict__ dz, int row, int lane, int D4, int C, long long lrow) {
    float dl[CMAX];
    if (dlogits) {   // upstream gradient given (autograd path): dl = dlogits / T * blend weight
#pragma unroll
        for (int c = 0; c < CMAX; ++c) dl[c] = (c < C) ? dlogits[(long long)row * C + c] * invT * w_new : 0.f;
    } else {
        float mx = -INFINITY;
#pragma unroll
        for (int c = 0; c < CMAX; ++c) { dl[c] = (c < C) ? lgv[c] : -INFINITY; mx = fmaxf(mx, dl[c]); }
        float se = 0.f;
#pragma unroll
        for (int c = 0; c < CMAX; ++c) { dl[c] = (c < C) ? expf(dl[c] - mx) : 0.f; se += dl[c]; }
        const long long yl = labels[lrow];
        const int y = (yl >= 0 && yl < (long long)C) ? (int)yl : -1;         // as ce_fwd_row: no one-hot for a label outside [0, C)
        const float k = gscale * invT * w_new;   // d loss / d (feat . tn[c]) incl. blend weight
#pragma unroll
        for (int c = 0; c < CMAX; ++c) dl[c] = (dl[c] / se - (c == y ? 1.f : 0.f)) * k;
    }
    const f32x4* zr = (const f32x4*)z + (long long)row * D4;
    float fd = 0.f;
    for (int i = lane; i < D4; i += 64) {
        f32x4 df = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int c = 0; c < CMAX; ++c) if (c < C) df += dl[c] * ((const f32x4*)tn)[(long long)c * D4 + i];
        const f32x4 f = zr[i] * inv;
        fd += (f[0] * df[0] + f[1] * df[1]) + (f[2] * df[2] + f[3] * df[3]);
    }
    fd = wave_sum(fd);
    f32x4* dzr = (f32x4*)dz + (long long)row * D4;
    for (int i = lane; i < D4; i += 64) {
        f32x4 df = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int c = 0; c < CMAX; ++c) if (c < C) df += dl[c] * ((const f32x4*)tn)[(long long)c * D4 + i];
        const f32x4 f = zr[i] * inv;
        dzr[i] = (df - f * fd) * inv;
    }
}

// ---- online group DRO (Sagawa et al. 2020): the group reduction and the update of q, one workgroup of 256 threads -------------
// Row b belongs to group groups[row], row = b, or idx[b] clamped into a table of n_tab rows when `idx` is given; a group id
// outside [0, G) belongs to no bucket (-1).
constexpr int GDRO_MAXG = 8;

__device__ __forceinline__ int gdro_group(const long long* __restrict__ groups, const long long* __restrict__ idx, long long n_tab, int b, int G) {
    const long long g = groups[idx ? table_row(idx, b, n_tab) : (long long)b];
    return (g >= 0 && g < G) ? (int)g : -1;
}

// n_g, L_g = mean of loss_rows over group g (0 for an absent group), m = max L_g over the groups present,
// q'_g = q_g exp(eta (L_g - m)), q = q' / sum q', weight of a row of group g = q_g / n_g (0 for an absent group), robust loss =
// sum_g q_g L_g.  Sums in float64 in a fixed order: thread t adds rows t, t + 256, ... in row order, then an LDS tree over the
// 256 threads; the G-element arithmetic is thread 0's, in float64.  stats [3][G]: the row weights | L_g | n_g.  q_in may be q_out
// (every q_in is read before any q_out is written, by the same thread).
__device__ __forceinline__ void gdro_weights_body(const float* __restrict__ loss_rows, const long long* __restrict__ groups,
                                                  const long long* __restrict__ idx, long long n_tab, const float* q_in, float* q_out,
                                                  float* __restrict__ stats, float* __restrict__ robust_loss, int B, int G, float eta) {
    __shared__ double sred[GDRO_MAXG][256];
    __shared__ int nred[GDRO_MAXG][256];
    const int t = threadIdx.x;
    double s[GDRO_MAXG];
    int n[GDRO_MAXG];
#pragma unroll
    for (int k = 0; k < GDRO_MAXG; ++k) { s[k] = 0.0; n[k] = 0; }
    for (int b = t; b < B; b += 256) {
        const int g = gdro_group(groups, idx, n_tab, b, G);
        const double l = (double)loss_rows[b];
#pragma unroll
        for (int k = 0; k < GDRO_MAXG; ++k)
            if (k == g) { s[k] += l; n[k] += 1; }
    }
#pragma unroll
    for (int k = 0; k < GDRO_MAXG; ++k) { sred[k][t] = s[k]; nred[k][t] = n[k]; }
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (t < o) {
#pragma unroll
            for (int k = 0; k < GDRO_MAXG; ++k) { sred[k][t] += sred[k][t + o]; nred[k][t] += nred[k][t + o]; }
        }
        __syncthreads();
    }
    if (t != 0) return;
    double L[GDRO_MAXG], qn[GDRO_MAXG];
    double m = 0.0, sum = 0.0, rl = 0.0;
    bool any = false;
#pragma unroll
    for (int k = 0; k < GDRO_MAXG; ++k) {
        const int nk = k < G ? nred[k][0] : 0;
        n[k] = nk;
        L[k] = nk ? sred[k][0] / (double)nk : 0.0;
        if (nk && (!any || L[k] > m)) { m = L[k]; any = true; }
    }
#pragma unroll
    for (int k = 0; k < GDRO_MAXG; ++k) {
        qn[k] = k < G ? (double)q_in[k] * exp((double)eta * (L[k] - m)) : 0.0;
        sum += qn[k];
    }
#pragma unroll
    for (int k = 0; k < GDRO_MAXG; ++k)
        if (k < G) {
            const float qf = (float)(qn[k] / sum);
            q_out[k] = qf;
            stats[k] = n[k] ? qf / (float)n[k] : 0.f;
            stats[G + k] = (float)L[k];
            stats[2 * G + k] = (float)n[k];
            rl += (double)qf * L[k];
        }
    *robust_loss = (float)rl;
}

// ---- multi-tensor SGD with momentum: one tensor's update (n elements; ns > 1: g holds ns partial gradients n apart, summed here
// in order, grad_reduce_body's order) -------------------------------------------------------------------------------------
__device__ __forceinline__ void sgd_body(const dim3 bi, const dim3 gd, float* p, const float* g, float* m, const long long n, const int ns, float lr,
                                         float mu, float wd, int first) {
    for (long long i = (long long)bi.x * blockDim.x + threadIdx.x; i < n; i += (long long)gd.x * blockDim.x) {
        const float w = p[i];
        float gv = g[i];
        for (int sidx = 1; sidx < ns; ++sidx) gv += g[(long long)sidx * n + i];
        const float gi = fmaf(wd, w, gv);
        const float b = first ? gi : fmaf(mu, m[i], gi);
        m[i] = b;
        p[i] = w - lr * b;
    }
}
