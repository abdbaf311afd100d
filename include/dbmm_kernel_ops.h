/* dbmm_kernel_ops.h -- entries of libdbmm_hip.so for matrix-free kernel-matrix operators (kernel ridge regression; later Gaussian-process
 * means, kernel PCA).  Same library, same conventions as include/dbmm.h: C linkage, 0 on success, a negative DBMM_E_* of dbmm.h for a
 * refused call (nothing is launched then), device pointers unless stated, `stream` a hipStream_t or NULL.
 *
 * Why a second header: the set of entries that dbmm.h declares is pinned, name by name, by the operand audit of the test suite
 * (tests/ops_audit.py), and the change that added these entries could not edit that list.  A later change that may edit the audit's
 * lists folds this header into dbmm.h and its binding table (_lib._SIGS_KERNEL_OPS) into _lib._SIGS; nothing else depends on the split. */
#ifndef DBMM_KERNEL_OPS_H
#define DBMM_KERNEL_OPS_H

#include "dbmm.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The product of the RBF kernel matrix of the rows x (zero diagonal) with C dense columns, without N x N:
 *   out double [N][C]: out[i][c] = sum over j != i of exp(-gamma ||x[i] - x[j]||^2) v[j][c].
 * dbmm_pairdist_rbf_row_group_sums' tile kernel with a weighted-columns epilogue: x fp32 [N][D], center fp32 [D] (a vector near the
 * rows' mean, subtracted before the products are formed), planes, ring and d^2 as there; the kernel values of a tile are formed ONCE,
 * in place in the accumulator registers (hardware exp2; the pair (i, i) excluded by index through d^2 = +inf, an exact 0), and every
 * weight column then costs one multiply-add per element: a lane forms w0 k0 + w1 k1 for its two columns, the rows kernel's fp32 tree
 * over a wave's 64 columns follows, then float64 over the column waves, tiles and chunks in a fixed order.  No floating-point atomics:
 * two calls give the same bits, and a column's result does not depend on C or on the other columns (a runtime loop over the columns).
 * v fp32 [N][C] row-major, signed.  A (tile, column) pair whose 256 weights are all zero is skipped, which changes no value: a product
 * with one-hot or mostly-zero weights (query rows appended with zero weights) pays only for the tiles that carry weight.
 * Error of an entry: 1e-4 sum_j k_ij |v_jc| under the preconditions of dbmm_pairdist_rbf_row_group_sums; an exact 0 where that sum is 0.
 * gamma: ONE finite bandwidth > 0, by value (else DBMM_E_ARG).  N outside 1..2^23 or C outside 1..16: DBMM_E_SHAPE; D % 64 != 0 or
 * D > 4096: DBMM_E_UNSUPPORTED; a null pointer: DBMM_E_ARG; x, v, center and the workspace 16-byte aligned, else DBMM_E_ALIGN; a
 * workspace below dbmm_workspace_bytes_pairdist_rbf_matvec(N, D, C): DBMM_E_WORKSPACE -- checked in this order.  Four launches and two
 * memsets on `stream`.  The workspace is dbmm_workspace_bytes_pairdist_rows(N, D, C): the planes (about N * D * 4 bytes), 8 bytes per
 * row, 16 partial [N][C] float64 matrices (0 for N <= 0, D <= 0 or C outside 1..16). */
size_t dbmm_workspace_bytes_pairdist_rbf_matvec(int64_t N, int64_t D, int64_t C);
int dbmm_pairdist_rbf_matvec(const float* x, const float* v, const float* center, double gamma, double* out, int64_t N, int64_t D,
                             int64_t C, void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DBMM_KERNEL_OPS_H */
