// Top-k eigenpairs of a symmetric positive semi-definite float64 matrix C [D][D] by blocked subspace iteration with a Rayleigh-Ritz
// step in every iteration (include/dbmm.h: dbmm_sym_eig_begin / dbmm_sym_eig_iterate).  The block is
// m = 16 vectors (k <= 8 plus oversampling); all arithmetic is float64, plain v_fma_f64 chains: the product is 2 D^2 16 flop per
// iteration and bounds nothing.  Measured at D = 1024 an iteration is 78 us of kernel time, 59 of them the one-workgroup
// Rayleigh-Ritz launch (HISTORY.md).
//
// One iteration is three launches on the given stream, Q [D][16] orthonormal:
//   sym_eig_matvec_kernel   one workgroup per 16 rows of C: Z = C Q for those rows (four waves split K, each a row-ordered fma chain over
//                           its quarter, combined through LDS in wave order), then the block's 16 x 16 partials of T = Q^T Z and G = Z^T Z.
//   sym_eig_ritz_kernel     one workgroup: the residual test of the PREVIOUS iteration if it is still pending (below); the partials
//                           added in block order; T symmetrised; T = W theta W^T by cyclic Jacobi in LDS (round-robin ordering, at
//                           most JACOBI_SWEEPS sweeps), theta sorted descending; L L^T = W^T G W (Cholesky) and M = W L^-T.
//   sym_eig_rotate_kernel   one workgroup per 16 rows: the Ritz vectors' rows X = Q W (stored vector-major) and Y = Z W, the block's
//                           partials of the residuals r_j^2 = |Y_j - theta_j X_j|^2 FROM THE VECTORS, and Q <- Z M (= Y L^-T).
// The residual test of an iteration (r_j summed in block order, max_{j < k} r_j <= tol theta_1) needs the rotate kernel's partials, so
// it runs in the NEXT ritz kernel, or, after the last iteration of a dbmm_sym_eig_iterate call, in sym_eig_finish_kernel (one small
// launch per call): whichever comes first finds the `pending` word set, runs the one shared function and clears it, so the arithmetic,
// the iteration count and the result are the same however the host cuts the iterations into calls.  A fourth launch per iteration
// for the test would buy nothing.
//
// The state word lives in the workspace: every kernel reads it first and returns at once unless it is `running`, so iterations
// enqueued after convergence or breakdown are no-ops.  No cooperative launch, no grid barrier, no flag is waited for; every loop
// has a bound fixed at launch; no floating-point atomics (partials are merged in block order: two calls give the same bits); no memset.
// Breakdown: theta_1 not positive or not finite, Jacobi not converged after its cap, a residual that is not finite; a Cholesky pivot
// that is not positive, not finite or below 2^-40 of the largest so far (rank below 16) ends the run after that iteration's
// residual test, which may still find the top k converged.
#include "common.h"

namespace {

constexpr int M16 = 16;                    // vectors of the block
constexpr int RB = 16;                     // rows of C per workgroup
constexpr int LDP = 17;                    // padded leading dimension of the 16 x 16 LDS matrices
constexpr int JACOBI_SWEEPS = 12;          // cap; a 16 x 16 float64 matrix takes 8 - 9 from scratch, 4 - 6 in a nearly Ritz basis

// status block, doubles at offset 0 of the workspace (include/dbmm.h documents it: Python reads it)
constexpr int ST_ITER = 0, ST_STATE = 1, ST_THETA = 2, ST_RES = 18, ST_K = 34, ST_TOL = 35, ST_PENDING = 36, ST_CHOL_BAD = 37;
constexpr int ST_DOUBLES = 64;
constexpr double RUNNING = 0.0, CONVERGED = 1.0, BREAKDOWN = 2.0;

// workspace, in doubles: status | X [16][D] vector-major | Q [D][16] | Z [D][16] | T partials [D/16][256] | G partials [D/16][256] |
// residual partials [D/16][16] | W [16][16] | M [16][16]
struct Layout {
    size_t x, q, z, tp, gp, rp, w, m, total;
};
inline Layout layout(int64_t D) {
    Layout l;
    const size_t d = (size_t)D, nb = d / RB;
    l.x = ST_DOUBLES;
    l.q = l.x + 16 * d;
    l.z = l.q + 16 * d;
    l.tp = l.z + 16 * d;
    l.gp = l.tp + nb * 256;
    l.rp = l.gp + nb * 256;
    l.w = l.rp + nb * 16;
    l.m = l.w + 256;
    l.total = l.m + 256;
    return l;
}

// L L^T = H in place (the lower triangle becomes L), 256 threads, H in LDS.  false (for every thread): a pivot was not positive,
// not finite or below 2^-40 of the largest pivot so far.
__device__ __forceinline__ bool chol16(double (*H)[LDP], int tid) {
    const int i = tid >> 4, j = tid & 15;
    double pmax = 0.0;
    for (int c = 0; c < M16; ++c) {
        const double d = H[c][c];
        if (!(d > 0.0) || !isfinite(d) || d < pmax * 0x1p-40) return false;      // every thread read the same word
        pmax = fmax(pmax, d);
        const double l = sqrt(d);
        __syncthreads();
        if (j == c && i >= c) H[i][c] = i == c ? l : H[i][c] / l;
        __syncthreads();
        if (i > c && j > c && j <= i) H[i][j] = fma(-H[i][c], H[j][c], H[i][j]);
        __syncthreads();
    }
    return true;
}

// X <- X L^-T in place (the triangular solve X_new L^T = X, column by column, every row at once), 256 threads, X and L in LDS
__device__ __forceinline__ void solve_lt16(double (*X)[LDP], const double (*L)[LDP], int tid) {
    const int i = tid >> 4, j = tid & 15;
    for (int b = 0; b < M16; ++b) {
        if (j == b) X[i][b] = X[i][b] / L[b][b];
        __syncthreads();
        if (j > b) X[i][j] = fma(-X[i][b], L[j][b], X[i][j]);
        __syncthreads();
    }
}

// sum of p[0], p[stride], ..., n terms, added IN THAT ORDER; the loads go out sixteen at a time so that the chain waits for one
// memory round trip per sixteen terms, not per term
__device__ __forceinline__ double ordered_sum(const double* p, size_t stride, int n) {
    double s = 0.0;
    for (int b = 0; b < n; b += 16) {
        double v[16];
#pragma unroll
        for (int u = 0; u < 16; ++u) v[u] = b + u < n ? p[(size_t)(b + u) * stride] : 0.0;
#pragma unroll
        for (int u = 0; u < 16; ++u)
            if (b + u < n) s += v[u];
    }
    return s;
}

// The residual test of the iteration whose rotate kernel has run: r_j = sqrt(sum over row blocks, in block order), converged when
// max_{j < k} r_j <= tol theta_1.  One workgroup of 256 threads; `sh` is 17 doubles of LDS.  Returns the new state to every thread.
__device__ __forceinline__ double residual_test(double* __restrict__ ws, const Layout l, int nb, double* sh, int tid) {
    if (tid < M16) {
        const double s = ordered_sum(ws + l.rp + tid, 16, nb);
        const double r = sqrt(s);
        sh[tid] = r;
        ws[ST_RES + tid] = r;
    }
    __syncthreads();
    if (tid == 0) {
        const int k = (int)ws[ST_K];
        double mx = 0.0;
        bool finite = true;
        for (int j = 0; j < 8; ++j)
            if (j < k) {
                finite = finite && isfinite(sh[j]);
                mx = fmax(mx, sh[j]);
            }
        double state = RUNNING;
        if (!finite) state = BREAKDOWN;
        else if (mx <= ws[ST_TOL] * ws[ST_THETA]) state = CONVERGED;
        else if (ws[ST_CHOL_BAD] != 0.0) state = BREAKDOWN;
        ws[ST_ITER] += 1.0;
        ws[ST_PENDING] = 0.0;
        ws[ST_STATE] = state;
        sh[16] = state;
    }
    __syncthreads();
    const double state = sh[16];
    __syncthreads();
    return state;
}

// partner of index x in round r of the round-robin ordering of 16 indices (15 rounds of 8 disjoint pairs cover every pair once)
__device__ __forceinline__ int partner(int x, int r) {
    if (x == 15) return r;
    int y = 2 * r - x;
    y = y < 0 ? y + 15 : (y >= 15 ? y - 15 : y);
    return y == x ? 15 : y;
}

// The rotation that zeroes A[p][q] (p < q), as index x sees it: new_x = alpha old_x + beta old_partner.  Identity when the entry is
// already negligible against the diagonal; `rotated` reports a real rotation.
__device__ __forceinline__ void rotation(const double (*A)[LDP], int x, int xp, double floor, double& alpha, double& beta, bool& rotated) {
    const int p = x < xp ? x : xp, q = x < xp ? xp : x;
    const double apq = A[p][q], app = A[p][p], aqq = A[q][q];
    alpha = 1.0; beta = 0.0; rotated = false;
    if (fabs(apq) > fmax(0x1p-53 * sqrt(fabs(app) * fabs(aqq)), floor) && isfinite(apq)) {
        const double tau = (aqq - app) / (2.0 * apq);
        const double t = copysign(1.0, tau) / (fabs(tau) + sqrt(1.0 + tau * tau));
        const double c = rsqrt(1.0 + t * t), s = t * c;
        alpha = c;
        beta = x < xp ? -s : s;
        rotated = s != 0.0;
    }
}

// ---- begin: orthonormalise the start block (Cholesky QR in one workgroup), reset the status ---------------------------------------
__global__ __launch_bounds__(256) void sym_eig_begin_kernel(const double* __restrict__ q0, double* __restrict__ ws, const Layout l, int D, int k,
                                                            double tol) {
    __shared__ double H[M16][LDP], Mi[M16][LDP], qs[64][LDP];
    const int tid = threadIdx.x, a = tid >> 4, b = tid & 15;
    // the start block goes through LDS 64 rows at a time (D % 64 == 0), the next chunk's loads in flight over this chunk's sums
    double v0, v1, v2, v3;
    auto fetch = [&](int r0) {
        const double* p = q0 + (size_t)(r0 + a) * 16 + b;
        v0 = p[0]; v1 = p[256]; v2 = p[512]; v3 = p[768];                        // rows a, a + 16, a + 32, a + 48 of the chunk
    };
    auto stage = [&](int r0) {
        __syncthreads();                                                         // the previous chunk has been read
        qs[a][b] = v0; qs[a + 16][b] = v1; qs[a + 32][b] = v2; qs[a + 48][b] = v3;
        __syncthreads();
        if (r0 + 64 < D) fetch(r0 + 64);
    };
    double g = 0.0;
    fetch(0);
    for (int r0 = 0; r0 < D; r0 += 64) {
        stage(r0);
#pragma unroll 8
        for (int r = 0; r < 64; ++r) g = fma(qs[r][a], qs[r][b], g);            // row order
    }
    H[a][b] = g;
    Mi[a][b] = a == b ? 1.0 : 0.0;
    __syncthreads();
    const bool ok = chol16(H, tid);
    __syncthreads();
    if (ok) solve_lt16(Mi, H, tid);                                              // Mi = L^-T
    if (tid < ST_DOUBLES) {
        double v = 0.0;
        if (tid == ST_STATE) v = ok ? RUNNING : BREAKDOWN;
        if (tid == ST_K) v = (double)k;
        if (tid == ST_TOL) v = tol;
        ws[tid] = v;
    }
    // Q = q0 L^-T, and the same block as the (not yet meaningful) Ritz vectors, so that they are finite whatever follows
    fetch(0);
    for (int r0 = 0; r0 < D; r0 += 64) {
        stage(r0);
#pragma unroll
        for (int m = 0; m < 4; ++m) {
            const int row = a + 16 * m;
            double s = 0.0;
            if (ok) {
#pragma unroll
                for (int c = 0; c < M16; ++c) s = fma(qs[row][c], Mi[c][b], s);
            }
            ws[l.q + (size_t)(r0 + row) * 16 + b] = s;
            ws[l.x + (size_t)b * D + r0 + row] = s;
        }
    }
}

// ---- Z = C Q for 16 rows, and the block's partials of T = Q^T Z and G = Z^T Z ------------------------------------------------------------
__global__ __launch_bounds__(256) void sym_eig_matvec_kernel(const double* __restrict__ C, double* __restrict__ ws, const Layout l, int D) {
    if (ws[ST_STATE] != RUNNING) return;
    __shared__ double cs[4][RB][LDP];          // a wave's chunk of C: 16 rows x 16 columns
    __shared__ double qc[4][RB][M16];          // and the 16 rows of Q that meet it
    __shared__ double zs[4][RB][M16];          // the four waves' partial Z blocks
    __shared__ double qf[RB][LDP], zf[RB][LDP];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int r0 = blockIdx.x * RB;
    const int i = lane >> 2, jq = lane & 3;    // the lane's row of the block and its four columns 4 jq .. 4 jq + 3 of Z
    const int kq = D / 4, k0 = w * kq;         // the wave's quarter of K (a multiple of 16)
    const double* Q = ws + l.q;
    double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
    // a chunk is 16 columns of the wave's 16 rows of C and the 16 rows of Q that meet them; both go through the wave's LDS, and the
    // next chunk's loads are in flight over this chunk's products
    double c0, c1, c2, c3, q0, q1, q2, q3;
    auto fetch = [&](int kb) {
        const double* cp = C + (size_t)(r0 + i) * D + kb + 4 * jq;
        const double* qp = Q + (size_t)(kb + i) * 16 + 4 * jq;
        c0 = cp[0]; c1 = cp[1]; c2 = cp[2]; c3 = cp[3];
        q0 = qp[0]; q1 = qp[1]; q2 = qp[2]; q3 = qp[3];
    };
    fetch(k0);
    for (int kb = k0; kb < k0 + kq; kb += 16) {
        __syncthreads();                       // the previous chunk has been read
        cs[w][i][4 * jq + 0] = c0; cs[w][i][4 * jq + 1] = c1; cs[w][i][4 * jq + 2] = c2; cs[w][i][4 * jq + 3] = c3;
        qc[w][i][4 * jq + 0] = q0; qc[w][i][4 * jq + 1] = q1; qc[w][i][4 * jq + 2] = q2; qc[w][i][4 * jq + 3] = q3;
        __syncthreads();
        if (kb + 16 < k0 + kq) fetch(kb + 16);
#pragma unroll
        for (int kk = 0; kk < 16; ++kk) {
            const double c = cs[w][i][kk];
            const double* qp = &qc[w][kk][4 * jq];
            a0 = fma(c, qp[0], a0); a1 = fma(c, qp[1], a1); a2 = fma(c, qp[2], a2); a3 = fma(c, qp[3], a3);
        }
    }
    zs[w][i][4 * jq + 0] = a0; zs[w][i][4 * jq + 1] = a1; zs[w][i][4 * jq + 2] = a2; zs[w][i][4 * jq + 3] = a3;
    __syncthreads();
    const int a = tid >> 4, b = tid & 15;
    const double z = ((zs[0][a][b] + zs[1][a][b]) + zs[2][a][b]) + zs[3][a][b];      // wave order
    ws[l.z + (size_t)(r0 + a) * 16 + b] = z;
    zf[a][b] = z;
    qf[a][b] = Q[(size_t)(r0 + a) * 16 + b];
    __syncthreads();
    double t = 0.0, g = 0.0;
#pragma unroll
    for (int r = 0; r < RB; ++r) {
        t = fma(qf[r][a], zf[r][b], t);
        g = fma(zf[r][a], zf[r][b], g);
    }
    ws[l.tp + (size_t)blockIdx.x * 256 + tid] = t;
    ws[l.gp + (size_t)blockIdx.x * 256 + tid] = g;
}

// ---- Rayleigh-Ritz on the merged 16 x 16 matrices -----------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void sym_eig_ritz_kernel(double* __restrict__ ws, const Layout l, int nb) {
    if (ws[ST_STATE] != RUNNING) return;
    __shared__ double A[M16][LDP], W[M16][LDP], G[M16][LDP], H[M16][LDP], Ws[M16][LDP];
    __shared__ double sh[17], th[M16];
    __shared__ int flag, rank[M16];
    const int tid = threadIdx.x, i = tid >> 4, j = tid & 15;
    if (ws[ST_PENDING] != 0.0 && residual_test(ws, l, nb, sh, tid) != RUNNING) return;
    H[i][j] = ordered_sum(ws + l.tp + tid, 256, nb);                             // block order
    G[i][j] = ordered_sum(ws + l.gp + tid, 256, nb);
    W[i][j] = i == j ? 1.0 : 0.0;
    __syncthreads();
    A[i][j] = 0.5 * (H[i][j] + H[j][i]);
    if (tid < M16) th[tid] = fabs(H[tid][tid]);
    __syncthreads();
    // an entry below 2^-70 of the largest diagonal entry is left alone: it moves no eigenvalue by more than 2^-66 theta_1, and a
    // block of rank below 16 (pure rounding noise on its trailing diagonal) still ends its sweeps
    double floor = 0.0;
    for (int m = 0; m < M16; ++m) floor = fmax(floor, th[m]);
    floor *= 0x1p-70;
    __syncthreads();
    // cyclic Jacobi: 15 rounds of 8 disjoint rotations per sweep, A <- J^T A J and W <- W J, every thread one entry of each
    bool done = false;
    for (int sweep = 0; sweep < JACOBI_SWEEPS && !done; ++sweep) {
        if (tid == 0) flag = 0;
        for (int r = 0; r < 15; ++r) {
            const int ip = partner(i, r), jp = partner(j, r);
            double ai, bi, aj, bj;
            bool ri, rj;
            rotation(A, i, ip, floor, ai, bi, ri);
            rotation(A, j, jp, floor, aj, bj, rj);
            const double n_a = ai * (aj * A[i][j] + bj * A[i][jp]) + bi * (aj * A[ip][j] + bj * A[ip][jp]);
            const double n_w = aj * W[i][j] + bj * W[i][jp];
            __syncthreads();
            A[i][j] = (ri && j == ip) ? 0.0 : n_a;                               // the annihilated pair is zero exactly
            W[i][j] = n_w;
            if (ri) flag = 1;
            __syncthreads();
        }
        done = flag == 0;                                                        // a sweep without a rotation: converged
        __syncthreads();
    }
    // theta descending: rank by counting, ties by index
    if (tid < M16) th[tid] = A[tid][tid];
    __syncthreads();
    if (tid < M16) {
        int rk = 0;
        bool fin = true;
        for (int m = 0; m < M16; ++m) {
            rk += (th[m] > th[tid] || (th[m] == th[tid] && m < tid)) ? 1 : 0;
            fin = fin && isfinite(th[m]);
        }
        rank[tid] = fin ? rk : tid;
        if (!fin) flag = 2;
    }
    __syncthreads();
    Ws[i][rank[j]] = W[i][j];
    if (tid < M16) sh[rank[tid]] = th[tid];
    __syncthreads();
    const bool hard = !done || flag == 2 || !(sh[0] > 0.0);
    if (hard) {                                                                  // nothing to iterate on: the run ends here
        if (tid == 0) {
            ws[ST_ITER] += 1.0;
            ws[ST_STATE] = BREAKDOWN;
        }
        return;
    }
    if (tid < M16) ws[ST_THETA + tid] = sh[tid];
    ws[l.w + tid] = Ws[i][j];
    // H = Ws^T G Ws, then L L^T = H and M = Ws L^-T
    {
        double s = 0.0;
#pragma unroll
        for (int c = 0; c < M16; ++c) s = fma(G[i][c], Ws[c][j], s);
        A[i][j] = s;
    }
    __syncthreads();
    {
        double s = 0.0;
#pragma unroll
        for (int c = 0; c < M16; ++c) s = fma(Ws[c][i], A[c][j], s);
        H[i][j] = s;
    }
    __syncthreads();
    const bool ok = chol16(H, tid);
    __syncthreads();
    if (ok) solve_lt16(Ws, H, tid);                                              // Ws becomes M (its copy for the rotate is written)
    ws[l.m + tid] = ok ? Ws[i][j] : 0.0;
    if (tid == 0) ws[ST_CHOL_BAD] = ok ? 0.0 : 1.0;
}

// ---- the Ritz vectors' rows, the residual partials, Q <- Z M ---------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void sym_eig_rotate_kernel(double* __restrict__ ws, const Layout l, int D) {
    if (ws[ST_STATE] != RUNNING) return;
    __shared__ double qf[RB][LDP], zf[RB][LDP], W[M16][LDP], M[M16][LDP], xs[M16][LDP], rs[RB][LDP];
    const int tid = threadIdx.x, i = tid >> 4, j = tid & 15;
    const int r0 = blockIdx.x * RB;
    qf[i][j] = ws[l.q + (size_t)(r0 + i) * 16 + j];
    zf[i][j] = ws[l.z + (size_t)(r0 + i) * 16 + j];
    W[i][j] = ws[l.w + tid];
    M[i][j] = ws[l.m + tid];
    const double theta = ws[ST_THETA + j];
    __syncthreads();
    double x = 0.0, y = 0.0, q = 0.0;
#pragma unroll
    for (int c = 0; c < M16; ++c) {
        x = fma(qf[i][c], W[c][j], x);
        y = fma(zf[i][c], W[c][j], y);
        q = fma(zf[i][c], M[c][j], q);
    }
    const double r = fma(-theta, x, y);
    ws[l.q + (size_t)(r0 + i) * 16 + j] = q;
    xs[j][i] = x;
    rs[i][j] = r * r;
    __syncthreads();
    ws[l.x + (size_t)i * D + r0 + j] = xs[i][j];                                 // vector-major: vector i, rows r0 .. r0 + 15
    if (tid < M16) {
        double s = 0.0;
#pragma unroll
        for (int c = 0; c < RB; ++c) s += rs[c][tid];                            // row order
        ws[l.rp + (size_t)blockIdx.x * 16 + tid] = s;
    }
    if (blockIdx.x == 0 && tid == 0) ws[ST_PENDING] = 1.0;
}

// ---- the residual test after the last iteration of a call -------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void sym_eig_finish_kernel(double* __restrict__ ws, const Layout l, int nb) {
    if (ws[ST_STATE] != RUNNING) return;
    __shared__ double sh[17];
    if (ws[ST_PENDING] != 0.0) residual_test(ws, l, nb, sh, threadIdx.x);
}

inline int eig_shape(int64_t D) {
    if (D <= 0 || (D % 64) || D > 4096) return DBMM_E_UNSUPPORTED;
    return DBMM_OK;
}

}  // namespace

// see include/dbmm.h
extern "C" size_t dbmm_workspace_bytes_sym_eig(int64_t D) {
    if (eig_shape(D) != DBMM_OK) return 0;
    return layout(D).total * sizeof(double);
}

// see include/dbmm.h
extern "C" int dbmm_sym_eig_begin(const double* q0, int64_t D, int64_t k, double tol, void* workspace, size_t workspace_bytes, void* stream) {
    const int rc = eig_shape(D);
    if (rc != DBMM_OK) return rc;
    if (k < 1 || k > 8 || !(tol > 0.0) || !(tol < HUGE_VAL)) return DBMM_E_SHAPE;
    if (!q0 || !workspace) return DBMM_E_ARG;
    if (workspace_bytes < dbmm_workspace_bytes_sym_eig(D)) return DBMM_E_WORKSPACE;
    if (!dbmm_aligned16(q0) || !dbmm_aligned16(workspace)) return DBMM_E_ALIGN;
    hipLaunchKernelGGL(sym_eig_begin_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, q0, (double*)workspace, layout(D), (int)D, (int)k, tol);
    DBMM_CHECK_LAUNCH();
    return DBMM_OK;
}

// see include/dbmm.h
extern "C" int dbmm_sym_eig_iterate(const double* C, int64_t D, int64_t n_iter, void* workspace, size_t workspace_bytes, void* stream) {
    const int rc = eig_shape(D);
    if (rc != DBMM_OK) return rc;
    if (n_iter < 0) return DBMM_E_SHAPE;
    if (!C || !workspace) return DBMM_E_ARG;
    if (workspace_bytes < dbmm_workspace_bytes_sym_eig(D)) return DBMM_E_WORKSPACE;
    if (!dbmm_aligned16(C) || !dbmm_aligned16(workspace)) return DBMM_E_ALIGN;
    if (n_iter == 0) return DBMM_OK;
    const Layout l = layout(D);
    const int nb = (int)(D / RB);
    double* ws = (double*)workspace;
    hipStream_t s = (hipStream_t)stream;
    for (int64_t it = 0; it < n_iter; ++it) {
        hipLaunchKernelGGL(sym_eig_matvec_kernel, dim3(nb), dim3(256), 0, s, C, ws, l, (int)D);
        DBMM_CHECK_LAUNCH();
        hipLaunchKernelGGL(sym_eig_ritz_kernel, dim3(1), dim3(256), 0, s, ws, l, nb);
        DBMM_CHECK_LAUNCH();
        hipLaunchKernelGGL(sym_eig_rotate_kernel, dim3(nb), dim3(256), 0, s, ws, l, (int)D);
        DBMM_CHECK_LAUNCH();
    }
    hipLaunchKernelGGL(sym_eig_finish_kernel, dim3(1), dim3(256), 0, s, ws, l, nb);
    DBMM_CHECK_LAUNCH();
    return DBMM_OK;
}
