/*
 * dbmm.h -- C ABI of libdbmm_hip.so: the MI355X (gfx950) kernels under the reference's
 * CLIP-embedding + debiasing-adapter hot path.
 *
 * The reference (Lainshower/debiasing-multi-modal) is pure PyTorch: it has no native
 * boundary of its own.  Each entry point below replaces the ATen operator sequence at the
 * cited reference site (paths relative to /root/reference); the Python mirror of the
 * reference classes in debiasing-multi-modal_amd/ binds them through ctypes
 * (INTEGRATION.md shows the stub a maintainer would add).
 *
 * Conventions
 *   - plain pointers + int64 sizes; no torch / hip types in signatures (`stream` is a
 *     hipStream_t passed as void*; NULL = the null stream).
 *   - the caller owns every buffer, including workspaces; the library never allocates,
 *     frees, retains pointers or synchronises.  All work is enqueued on `stream`.
 *   - return 0 on success, a negative DBMM_E_* for shape/alignment violations, or the
 *     positive hipError_t of a failed launch.  Never throws, never aborts.
 *   - activations are fp32, channels-last (NHWC) inside the library; image input is the
 *     reference's NCHW and is converted by the first kernel that touches it.
 *   - all float pointers must be 16-byte aligned; leading dimensions multiples of 4.
 */
#ifndef DBMM_H
#define DBMM_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DBMM_OK 0
#define DBMM_E_SHAPE (-1)     /* unsupported / inconsistent dimensions            */
#define DBMM_E_ALIGN (-2)     /* pointer or leading dimension not 16-byte aligned */
#define DBMM_E_WORKSPACE (-3) /* workspace too small                              */
#define DBMM_E_ARG (-4)       /* null pointer / bad enum                          */
#define DBMM_E_UNSUPPORTED (-5) /* valid request this build has no kernel for (caller falls back) */

/* K order of a packed conv weight [Cout][K], K = KH*KW*Cin */
#define DBMM_WL_TAP_MAJOR 0   /* (kh, kw, cin)                                              */
#define DBMM_WL_CHUNK_MAJOR 1 /* (cin/16, kh, kw, 16): needs Cin % 16 == 0; the taps of one
                                 16-channel slab are adjacent along K, so the KH*KW re-reads
                                 of an input pixel hit L1/L2 instead of HBM                  */
#define DBMM_WL_CHUNK32_MAJOR 2 /* (cin/32, kh, kw, 32): the same with 32-channel slabs (Cin % 32
                                 == 0) -- the order the 32-deep fp16-pair kernels can step     */

#define DBMM_ACT_NONE 0
#define DBMM_ACT_RELU 1
#define DBMM_ACT_QUICKGELU 2 /* x * sigmoid(1.702 x), clip/model.py:166-168 */

int dbmm_version(void);
const char* dbmm_error_string(int code);

/* Library options: the switches the launchers consult (which kernel family serves a shape; every setting gives the same
 * results up to fp32 rounding).  Names are listed in csrc/options.hip ("igemm_halo", "gemm_8ph", "f16_8ph",
 * "adapter_step_fused", ...).  Defaults are the measured best; each option is seeded once, at load time, from the
 * environment variable DBMM_<NAME IN UPPER CASE> when that is set -- no launch path reads the environment.
 * Returns DBMM_E_ARG for an unknown name.  The reference has no counterpart (it has no native code). */
int dbmm_set_option(const char* name, int value);
int dbmm_get_option(const char* name, int* value);

/* ---------------------------------------------------------------------------------------
 * Dense contractions on fp32 MFMA (v_mfma_f32_32x32x2_f32), LDS-tiled implicit GEMM.
 * ------------------------------------------------------------------------------------ */

/* y[B,Ho,Wo,Cout] = act( conv(x[B,H,W,Cin], w) + bias + residual ), NHWC, BatchNorm already
 * folded into (w, bias) by the caller.  w is [Cout][KH][KW][Cin].  Cin % 4 == 0.
 * Replaces conv->bn->relu(->add) of Bottleneck.forward (clip/model.py:45-54) and the stem
 * convs 2/3 (clip/model.py:141-142).  residual may be NULL; it has y's shape. */
int dbmm_conv_bn_act(const float* x, const float* w, const float* bias, const float* residual,
                     float* y, int64_t B, int64_t H, int64_t W, int64_t Cin, int64_t Cout,
                     int64_t KH, int64_t KW, int64_t stride, int64_t pad, int act, void* stream);
/* named specialisations of the above */
int dbmm_conv1x1_bn_act(const float* x, const float* w, const float* bias, const float* residual,
                        float* y, int64_t B, int64_t H, int64_t W, int64_t Cin, int64_t Cout,
                        int act, void* stream);
int dbmm_conv3x3_bn_act(const float* x, const float* w, const float* bias, const float* residual,
                        float* y, int64_t B, int64_t H, int64_t W, int64_t Cin, int64_t Cout,
                        int act, void* stream);

/* c[M,N] = act( alpha * (op(a) @ op(w)^T + bias) + residual )
 *   trans_a = 0: a is [M][lda] (K contiguous);  1: a is [K][lda] (M contiguous)
 *   trans_w = 0: w is [N][ldw] (K contiguous, i.e. nn.Linear.weight); 1: w is [K][ldw]
 * Replaces F.linear / addmm at clip/model.py:72-90 (attention-pool projections), :185-191
 * (QKV / out_proj / c_fc+QuickGELU / c_proj with residual), :238, :354 (projections) and the
 * adapter Linear layers and their weight/input gradients (final_main.py:167-172). */
int dbmm_gemm_bias_act(const float* a, int64_t lda, int trans_a, const float* w, int64_t ldw,
                       int trans_w, const float* bias, const float* residual, int64_t ldr,
                       float* c, int64_t ldc, int64_t M, int64_t N, int64_t K, float alpha,
                       int act, void* stream);

/* Variants with a caller-provided scratch buffer (dbmm_workspace_bytes_igemm() bytes, 16-B
 * aligned).  With it the library may pick the stream-K work split when whole tiles would
 * leave part of the 256 CUs idle (e.g. 784 tiles); results are deterministic either way. */
size_t dbmm_workspace_bytes_igemm(void);
int dbmm_conv_bn_act_ws(const float* x, const float* w, const float* bias, const float* residual,
                        float* y, int64_t B, int64_t H, int64_t W, int64_t Cin, int64_t Cout,
                        int64_t KH, int64_t KW, int64_t stride, int64_t pad, int act, int w_layout,
                        void* workspace, size_t workspace_bytes, void* stream);
int dbmm_gemm_bias_act_ws(const float* a, int64_t lda, int trans_a, const float* w, int64_t ldw,
                          int trans_w, const float* bias, const float* residual, int64_t ldr,
                          float* c, int64_t ldc, int64_t M, int64_t N, int64_t K, float alpha,
                          int act, void* workspace, size_t workspace_bytes, void* stream);

/* Split-precision variants ("x3"): each fp32 operand value is the exact sum of three bf16 values
 * and a product is accumulated as its six largest bf16 x bf16 partial products on the bf16
 * matrix cores (2.67x the fp32-MFMA rate, dropped terms <= 2^-24 relative = fp32-level accuracy).
 * w_planes = the weight split once by dbmm_split_weight_planes ([3][N][K] bf16,
 * dbmm_split_planes_bytes(N, K) bytes); activations stay fp32 and are split on the fly.  `w`
 * (fp32, same K order as the planes, see w_layout) is still required: shapes the split kernel does not cover (K or Cin
 * not a multiple of 16, N <= 32, operands >= 2 GiB) run on the fp32-MFMA kernel. */
size_t dbmm_split_planes_bytes(int64_t N, int64_t K);
int dbmm_split_weight_planes(const float* w, void* planes, int64_t N, int64_t K, void* stream);
int dbmm_conv_bn_act_x3(const float* x, const float* w, const void* w_planes, const float* bias,
                        const float* residual, float* y, int64_t B, int64_t H, int64_t W, int64_t Cin,
                        int64_t Cout, int64_t KH, int64_t KW, int64_t stride, int64_t pad, int act,
                        int w_layout, void* workspace, size_t workspace_bytes, void* stream);
int dbmm_gemm_bias_act_x3(const float* a, int64_t lda, const float* w, const void* w_planes, int64_t ldw,
                          const float* bias, const float* residual, int64_t ldr, float* c, int64_t ldc,
                          int64_t M, int64_t N, int64_t K, float alpha, int act, void* workspace,
                          size_t workspace_bytes, void* stream);

/* fp16-pair variant ("x2"): with a per-tensor power-of-two scale an fp32 value is hi + lo of two
 * fp16 values to 2^-22 relative, so three fp16 x fp16 partial products (hl, lh, hh) give
 * fp32-level accuracy at HALF the matrix-core work of the bf16 triple.  The scale of the
 * activations comes from a device scalar x_absmax >= max|x| that the producing launch wrote
 * through its y_absmax argument (atomic max over |y|; the caller zeroes the scalar beforehand;
 * an average pool may reuse its input's scalar: any upper bound works, a bound 2^k too large
 * costs k bits of the 2^-39 absolute floor).  w_planes_f16 = w * 2^w_exp split by
 * dbmm_split_weight_planes_f16 ([2][N][K] fp16); choose w_exp so that max|w| * 2^w_exp < 2^15.
 * x_absmax or w_planes_f16 may be NULL (fp32-MFMA kernel, y_absmax still honoured).
 * w_planes = 2: hi and lo plane.  w_planes = 1: the scaled weight is EXACTLY representable in
 * fp16 (true for every conv / linear weight the reference's build_model loads: it stores them
 * in fp16, clip/model.py:375-396,433) and only that plane is given -> two partial products; the
 * 32-deep K chunk is required (K % 32 == 0, and Cin % 32 == 0 for KxK convs), otherwise the
 * fp32-MFMA kernel runs.  out_scale (optional, [Cout]) multiplies the accumulator per output
 * channel before the bias: y = act((acc * out_scale + bias) + residual) -- it carries the
 * BatchNorm scale so that the weights themselves can stay the stored fp16 values.
 * pool = 2 fuses the AvgPool2d(2) that follows the conv in the reference's stem and stride-2
 * bottlenecks (clip/model.py:25,48,117,145) into the epilogue: the kernel walks the output
 * pixels 2x2-window-major, averages each window after the activation and writes only the pooled
 * tensor y[B][Ho/2][Wo/2][Cout] (same summation order as dbmm_avgpool2d: bit-identical result).
 * With pool = 2, y_full (optional, [B][Ho][Wo][Cout]) additionally receives the un-pooled output:
 * the last conv3 of a stage needs both -- the next block's conv1 reads the full map, its
 * downsample branch the pooled one (clip/model.py:36-38).  The residual, if any, is un-pooled.
 * Needs the fp16-pair kernel and even Ho and Wo; otherwise DBMM_E_UNSUPPORTED is returned and
 * nothing is launched (run the conv and the pool separately).  y_full must be NULL when pool = 0. */
size_t dbmm_split_planes_f16_bytes(int64_t N, int64_t K);
int dbmm_split_weight_planes_f16(const float* w, void* planes, int64_t N, int64_t K, int w_exp, void* stream);
int dbmm_conv_bn_act_x2(const float* x, const float* x_absmax, const float* w, const void* w_planes_f16,
                        int w_planes, int w_exp, const float* out_scale, const float* bias,
                        const float* residual, float* y, float* y_full, float* y_absmax,
                        int64_t B, int64_t H, int64_t W, int64_t Cin, int64_t Cout, int64_t KH, int64_t KW,
                        int64_t stride, int64_t pad, int act, int pool, int w_layout, void* workspace,
                        size_t workspace_bytes, void* stream);

/* GEMM on the fp16-pair path (see dbmm_conv_bn_act_x2 for the operands): c = act(alpha *
 * (a @ w^T * out_scale + bias) + residual), a row-major [M][K] with a device scalar a_absmax >=
 * max|a|, w [N][K] plus its fp16 planes (w_planes = 1 when w * 2^w_exp is exact in fp16 -- every
 * nn.Linear / attention projection weight of a model loaded like the reference does; needs
 * K % 32 == 0), c_absmax (optional) receives max|c|.  The attention core's output is a convex
 * combination of V rows, so the qkv GEMM's c_absmax also bounds it. */
int dbmm_gemm_bias_act_x2(const float* a, int64_t lda, const float* a_absmax, const float* w,
                          const void* w_planes_f16, int w_planes, int w_exp, int64_t ldw,
                          const float* out_scale, const float* bias, const float* residual, int64_t ldr,
                          float* c, int64_t ldc, float* c_absmax, int64_t M, int64_t N, int64_t K, float alpha,
                          int act, void* workspace, size_t workspace_bytes, void* stream);

/* First block of a ResNet stage (clip/model.py:36-38,42-55): out = relu(bn3(conv3(y)) +
 * bn_d(conv_d(avgpool(x)))).  Both convs are 1x1, so the sum is ONE GEMM over the concatenated
 * K = K + K2 -- the downsample branch's output is never written or re-read:
 *   c = act((a @ w^T) * 2^-(s+w_exp) * out_scale[n] + (a2 @ w2^T) * 2^-(s2+w2_exp) * out_scale2[n] + bias[n])
 * a [M][K] (lda) = conv2 output, a2 [M][K2] (lda2) = (pooled) block input, both with device scalars
 * a_absmax / a2_absmax; w_plane_f16 / w2_plane_f16 = single exact fp16 planes [N][K] / [N][K2] of
 * the stored weights times 2^w_exp / 2^w2_exp.  The kernel accumulates the second pair first,
 * multiplies the accumulators by ratio[n] * 2^(s - s2) and continues with the first pair;
 * ratio[n] = out_scale2[n] / out_scale[n] * 2^(w_exp - w2_exp) is supplied by the caller (out_scale
 * must be non-zero), bias = both BatchNorm biases added.  K, K2 multiples of 32.
 * DBMM_E_UNSUPPORTED (nothing launched) when the shape does not suit the 128x128 fp16-pair tile. */
int dbmm_gemm_dual_bn_act_x2(const float* a, int64_t lda, const float* a_absmax, const void* w_plane_f16,
                             int w_exp, int64_t ldw, int64_t K, const float* out_scale, const float* a2,
                             int64_t lda2, const float* a2_absmax, const void* w2_plane_f16, int64_t ldw2,
                             int64_t K2, const float* ratio, const float* bias, float* c, int64_t ldc,
                             float* c_absmax, int64_t M, int64_t N, int act, void* workspace,
                             size_t workspace_bytes, void* stream);

/* The two wide stem convolutions of ModifiedResNet (clip/model.py:108-116): 3x3 / stride 1 / pad 1 over Cin = 32
 * channels, eval-mode BatchNorm scale / bias, ReLU, optional AvgPool2d(2) (pool = 2), one launch of a persistent kernel
 * that keeps the whole weight in LDS and forms the nine taps from one 6 x 30 input patch per 4 x 28 output tile.
 * x NHWC [B][H][W][32] with device scalar x_absmax; w_plane_f16 [Cout][kh][kw][32] = stored weight * 2^w_exp as one
 * exact fp16 plane; y NHWC [B][H][W][Cout] or, pooled, [B][H/2][W/2][Cout]; y_absmax optional.  Same fp16-pair
 * arithmetic as dbmm_conv_bn_act_x2.  Served: Cin = 32, Cout in {32, 64}, H % 4 == 0, W % 28 == 0; DBMM_E_UNSUPPORTED
 * otherwise (nothing launched). */
int dbmm_conv3x3_c32_bn_relu_x2(const float* x, const float* x_absmax, const void* w_plane_f16, int w_exp,
                                const float* scale, const float* bias, float* y, float* y_absmax, int64_t B, int64_t H,
                                int64_t W, int64_t Cin, int64_t Cout, int pool, void* stream);

/* conv3 + residual of one bottleneck block chained with conv1 of the NEXT block (clip/model.py:42-55, two
 * consecutive Bottleneck.forward bodies) in one launch:
 *   x_out  = relu((y2 @ w3^T) * scale3 + bias3 + residual)        [B*Ho*Wo][N]
 *   y1_out = relu((x_out @ w1^T) * scale1 + bias1)                [B*Ho*Wo][P]
 *   x_pooled (optional) = AvgPool2d(2) of x_out                   [B*Ho/2*Wo/2][N]  (next stage's downsample input)
 * With x_pooled given, x_out may be NULL: the un-pooled tensor is then not written at all (at a stage seam its only other reader is
 * conv1 of the next block, which this launch has already computed).
 * The wide tensor x_out is written once and not read back for conv1.  y2 [B*Ho*Wo][K] fp32 with its device scalar
 * y2_absmax >= max|y2|; w3_plane_f16 [N][K] / w1_plane_f16 [P][N] = the stored (fp16-exact) weights times
 * 2^w3_exp / 2^w1_exp as single fp16 planes; scale / bias = eval-mode BatchNorm per channel.  x_absmax / y1_absmax
 * (optional, zeroed by the caller) receive the maxima for the consumers' fp16 scales.  Same fp16-pair arithmetic
 * as dbmm_conv_bn_act_x2.  Shapes served: K in {64, 128}, N % 64 == 0, P in {64, 128}, B*Ho*Wo % 4 == 0; DBMM_E_UNSUPPORTED (nothing
 * launched) otherwise -- the caller then issues the two convs separately. */
int dbmm_bottleneck_chain_x2(const float* y2, const float* y2_absmax, const void* w3_plane_f16, int w3_exp,
                             const float* scale3, const float* bias3, const float* residual, float* x_out,
                             float* x_pooled, float* x_absmax, const void* w1_plane_f16, int w1_exp,
                             const float* scale1, const float* bias1, float* y1_out, float* y1_absmax,
                             int64_t B, int64_t Ho, int64_t Wo, int64_t K, int64_t N, int64_t P, void* stream);

/* The same chain for the FIRST block of a stage whose input has the output's resolution (layer 1): the block adds
 * its downsample branch instead of a residual (clip/model.py:36-38,52), as in dbmm_gemm_dual_bn_act_x2:
 *   x_out  = relu((y2 @ w3^T) * scale3 + (a2 @ wd^T) * scale_d + bias)   with ratio[n] = scale_d[n] / scale3[n] * 2^(w3_exp - wd_exp),
 *   y1_out = relu((x_out @ w1^T) * scale1 + bias1).
 * y2 [M][K], a2 [M][K2] (the block input) with device scalars; bias = both BatchNorm biases added.  Served: K = K2 = 64,
 * N % 64 == 0, P in {64, 128}, M % 4 == 0; DBMM_E_UNSUPPORTED otherwise. */
int dbmm_bottleneck_chain_dual_x2(const float* y2, const float* y2_absmax, const void* w3_plane_f16, int w3_exp,
                                  const float* scale3, const float* bias, const float* a2, const float* a2_absmax,
                                  const void* wd_plane_f16, const float* ratio, float* x_out, float* x_absmax,
                                  const void* w1_plane_f16, int w1_exp, const float* scale1, const float* bias1,
                                  float* y1_out, float* y1_absmax, int64_t M, int64_t K, int64_t K2, int64_t N,
                                  int64_t P, void* stream);

/* The same chains started one conv earlier: conv2 (3x3, pad 1) + BatchNorm + ReLU of the block is computed inside the
 * launch from the block's conv1 output y1 (NHWC [B][H][W][K], device scalar y1_absmax), so neither y2 nor -- for conv1' --
 * x_out is read back from HBM:  y1 -> conv2 -> conv3 + (residual | downsample branch) -> x_out -> next conv1 -> y1_out.
 * w2_plane_f16 [K][(cin/32, kh, kw, 32)] = the stored 3x3 weight times 2^w2_exp as one exact fp16 plane in the
 * DBMM_WL_CHUNK32_MAJOR K order.  Pass `residual` for an ordinary block, or (a2, a2_absmax, wd_plane_f16, ratio) with
 * residual = NULL for a stage's first block at unchanged resolution (see dbmm_bottleneck_chain_dual_x2).
 * Served: (K, P) = (64, 64) or (128, 128); dual: (64, 64); N % 64 == 0; B*H*W % 4 == 0.  DBMM_E_UNSUPPORTED otherwise. */
int dbmm_bottleneck_block_chain_x2(const float* y1, const float* y1_absmax, const void* w2_plane_f16, int w2_exp,
                                   const float* scale2, const float* bias2, const void* w3_plane_f16, int w3_exp,
                                   const float* scale3, const float* bias3, const float* residual, const float* a2,
                                   const float* a2_absmax, const void* wd_plane_f16, const float* ratio, float* x_out,
                                   float* x_absmax, const void* w1_plane_f16, int w1_exp, const float* scale1,
                                   const float* bias1, float* y1_out, float* y1_out_absmax, int64_t B, int64_t H,
                                   int64_t W, int64_t K, int64_t N, int64_t P, void* stream);

/* The same GEMM (w_planes = 1 only) on the deep-pipelined 256 x 256 kernel (csrc/gemm_pair_8ph.hip): fp32 activations by
 * LDS-DMA, split into fp16 (hi, lo) when the fragments are read, two wave groups one barrier apart.  N % 256 == 0,
 * K % 64 == 0.  dbmm_gemm_bias_act_x2 routes the projections here where this kernel measured ahead (N >= 3072 with
 * K >= 1024, or K >= 4096; DBMM_GEMM_8PH = 0 never / 2 wherever it applies). */
int dbmm_gemm_pair_8ph(const float* a, int64_t lda, const float* a_absmax, const void* w_plane_f16, int w_exp, int64_t ldw,
                       const float* out_scale, const float* bias, const float* residual, int64_t ldr, float* c, int64_t ldc,
                       float* c_absmax, int64_t M, int64_t N, int64_t K, float alpha, int act, void* stream);

/* ---------------------------------------------------------------------------------------
 * fp16 mode of the transformer towers -- the reference's GPU path (convert_weights, clip/model.py:375-396; fp16
 * activations, fp32 LayerNorm statistics, clip/model.py:157-163).  Tensors marked f16 are IEEE half in HBM; every
 * product is one fp16 MFMA with fp32 accumulation; bias / QuickGELU / residual / softmax run in fp32 and the result
 * is rounded to fp16 once.  Throughput mode (BASELINE configs[4]); the fp32-accurate entry points above stay the
 * parity mode.
 * --------------------------------------------------------------------------------------- */
/* c f16 [M][ldc] = act(a f16 [M][lda] @ w f16 [N][ldw]^T + bias f32 [N]) + residual f16 [M][ldr].  K % 64 == 0, N % 8 == 0. */
int dbmm_gemm_f16(const void* a, int64_t lda, const void* w, int64_t ldw, const float* bias, const void* residual,
                  int64_t ldr, void* c, int64_t ldc, int64_t M, int64_t N, int64_t K, int act, void* stream);
/* The same with a workspace (16-B aligned, dbmm_workspace_bytes_igemm() bytes are enough): when the 256 x 256 tiles of the deep-pipelined
 * kernel leave a short last round on the 256 CUs, its tiles are cut along K over the idle CUs and summed by a second launch. */
int dbmm_gemm_f16_ws(const void* a, int64_t lda, const void* w, int64_t ldw, const float* bias, const void* residual,
                     int64_t ldr, void* c, int64_t ldc, int64_t M, int64_t N, int64_t K, int act, void* workspace,
                     size_t workspace_bytes, void* stream);
/* fp16 mode of the ModifiedResNet towers (clip/model.py:10-154 on the reference's GPU path: the image is cast to fp16, :146,
 * conv weights are fp16, BatchNorm parameters fp32).  Activations f16 NHWC; eval-mode BatchNorm as fp32 per-channel
 * scale / bias on the fp32 accumulator, residual add, ReLU and AvgPool2d(2) fused, ONE rounding to fp16 when stored.
 *   conv1x1: y f16 [M][Cout] = act(x f16 [M][Cin] @ w f16 [Cout][Cin]^T * scale + bias + residual f16 [M][Cout])
 *            (Bottleneck conv1 / conv3 / downsample conv).  Cin % 64 == 0, Cout % 8 == 0, else DBMM_E_UNSUPPORTED.
 *   conv3x3: stride 1, pad 1, + BatchNorm + ReLU, pool = 0 | 2 (AvgPool2d(2) of the result: Bottleneck conv2 of a stride-2
 *            block, stem conv3); w f16 [Cout][(cin / 32, kh, kw, 32)].  Cin % 32 == 0, Cout % 8 == 0; pool: H, W even.
 *   stem:    3x3 / stride 2 / pad 1 on the NCHW image (f32, or f16 with x_is_f16; rounded to fp16 first like the
 *            reference's cast), w f32 [kh][kw][3][Cout] with BatchNorm folded, bias f32 [Cout], ReLU, y f16 NHWC.  Cout 32 | 64.
 *   avgpool2: AvgPool2d(2) on f16 NHWC (the downsample branch of a stride-2 block, clip/model.py:36-38). */
int dbmm_conv1x1_bn_act_f16(const void* x, const void* w, const float* scale, const float* bias, const void* residual, void* y,
                            int64_t M, int64_t Cin, int64_t Cout, int act, void* stream);
/* fp16 mode, first block of a stage (clip/model.py:36-38, 42-55): out = act((y2 @ w3^T) * scale3 + (xp @ wd^T) * scale_d + bias) as ONE GEMM
 * over the concatenated K -- the downsample branch's output is never written or re-read.  y2 f16 [M][K] (conv2's output), xp f16 [M][K2]
 * (the pooled block input), w3 f16 [Cout][K], wd f16 [Cout][K2], ratio[n] = scale_d[n] / scale3[n] (scale3 non-zero), bias = both
 * BatchNorm biases added.  The kernel accumulates the second pair first, multiplies the fp32 accumulators by ratio[n] and continues with
 * the first.  On the deep-pipelined GEMM kernel when Cout % 256 == 0, K % 128 == 0, K2 % 128 == 0 and M >= 16384, otherwise on the
 * streaming 1x1 kernel (K % 32 == 0, K2 % 32 == 0, Cout > 64, Cout % 8 == 0: layer 1); DBMM_E_UNSUPPORTED (nothing launched) beyond that. */
int dbmm_conv1x1_dual_bn_act_f16(const void* y2, const void* w3, const float* scale3, const void* xp, const void* wd, const float* ratio,
                                 const float* bias, void* out, int64_t M, int64_t K, int64_t K2, int64_t Cout, int act, void* stream);
/* fp16 mode: conv3 + residual of one bottleneck block chained with conv1 of the NEXT block (clip/model.py:42-55 twice) in one launch:
 *   x_out  = relu((y2 @ w3^T) * scale3 + bias3 + residual)   f16 [M][N]      y1_out = relu((x_out @ w1^T) * scale1 + bias1)   f16 [M][P]
 * The wide tensor x_out is written once and not read back for conv1; x_out is rounded to fp16 before it feeds conv1, so the results equal
 * the two launches bit for bit.  y2 f16 [M][K], w3 f16 [N][K], w1 f16 [P][N].  K, P in {64, 128}, N % 64 == 0 (layers 1 - 2);
 * DBMM_E_UNSUPPORTED (nothing launched) otherwise -- the caller then issues the two convs. */
int dbmm_bottleneck_chain_f16(const void* y2, const void* w3, const float* scale3, const float* bias3, const void* residual, void* x_out,
                              const void* w1, const float* scale1, const float* bias1, void* y1_out, int64_t M, int64_t K, int64_t N,
                              int64_t P, void* stream);
/* the same chain at a stage seam (the block is the LAST of its stage, the next block downsamples): also x_pooled = AvgPool2d(2) of x_out
 * f16 [B*Ho/2*Wo/2][N], the next stage's downsample input (fp32 sum of the fp16 values in (dy, dx) order, times 0.25: equal to
 * dbmm_avgpool2_f16 of x_out bit for bit).  x_out may be NULL: the un-pooled tensor is then not written -- conv1 of the next block is
 * computed here and nothing else reads it.  Ho, Wo even, B*Ho*Wo % 4 == 0. */
int dbmm_bottleneck_chain_pool_f16(const void* y2, const void* w3, const float* scale3, const float* bias3, const void* residual, void* x_out,
                                   void* x_pooled, const void* w1, const float* scale1, const float* bias1, void* y1_out, int64_t B, int64_t Ho,
                                   int64_t Wo, int64_t K, int64_t N, int64_t P, void* stream);
/* the same chain for the FIRST block of a stage, whose shortcut is the downsample conv instead of a residual (dbmm_conv1x1_dual_bn_act_f16's
 * arguments and arithmetic, then conv1 of the next block): x_out = relu((y2 @ w3^T + (xp @ wd^T) * ratio) * scale3 + bias).
 * K = K2 = P = 64 (layer 1's first block); DBMM_E_UNSUPPORTED (nothing launched) otherwise. */
int dbmm_bottleneck_chain_dual_f16(const void* y2, const void* w3, const float* scale3, const void* xp, const void* wd, const float* ratio,
                                   const float* bias, void* x_out, const void* w1, const float* scale1, const float* bias1, void* y1_out,
                                   int64_t M, int64_t K, int64_t K2, int64_t N, int64_t P, void* stream);
int dbmm_conv1x1_bn_act_f16_ws(const void* x, const void* w, const float* scale, const float* bias, const void* residual, void* y,
                               int64_t M, int64_t Cin, int64_t Cout, int act, void* workspace, size_t workspace_bytes,
                               void* stream);          /* with a workspace, as dbmm_gemm_f16_ws */
/* fp16 mode, the LAST block of a stage (clip/model.py:50-54, then 36-38 of the next block): y = relu(conv1x1(x) * scale + bias + residual)
 * f16 [B*Ho*Wo][Cout] AND y_pooled = AvgPool2d(2) of y f16 [B*Ho/2*Wo/2][Cout] (equal to dbmm_avgpool2_f16 of y bit for bit) in one launch.
 * Cin in {128, 256}, Cout % 64 == 0, Ho and Wo even (layers 2 / 3); DBMM_E_UNSUPPORTED (nothing launched) otherwise -- the caller then issues
 * the conv and the pool. */
int dbmm_conv1x1_res_pool_f16(const void* x, const void* w, const float* scale, const float* bias, const void* residual, void* y,
                              void* y_pooled, int64_t B, int64_t Ho, int64_t Wo, int64_t Cin, int64_t Cout, void* stream);
int dbmm_conv3x3_bn_relu_f16(const void* x, const void* w, const float* scale, const float* bias, void* y, int64_t B, int64_t H,
                             int64_t W, int64_t Cin, int64_t Cout, int pool, void* stream);
int dbmm_conv_stem_s2_f16(const void* x_nchw, int x_is_f16, const float* w, const float* bias, void* y_nhwc, int64_t B, int64_t H,
                          int64_t W, int64_t Cout, void* stream);
/* the same conv with BatchNorm as a separate per-channel scale / bias: y = relu(conv(fp16(x), fp16(w)) * scale + bias).  w fp32
 * [kh][kw][cin][cout] holding the model's fp16 conv1 weights (rounded to fp16 here: exact for an fp16-stored model, clip/model.py:146-148
 * under convert_weights); runs on the MFMA gather kernel (option stem_mfma; 0: the FMA kernel). */
int dbmm_conv_stem_s2_bn_f16(const void* x_nchw, int x_is_f16, const float* w, const float* scale, const float* bias, void* y_nhwc,
                             int64_t B, int64_t H, int64_t W, int64_t Cout, void* stream);
int dbmm_avgpool2_f16(const void* x, void* y, int64_t B, int64_t H, int64_t W, int64_t C, void* stream);
/* softmax(q k^T / sqrt(64)) v per (image, head), head_dim 64; qkv f16 [B*L][3E] (q | k | v), out f16 [B*L][E]. */
int dbmm_mha_core_f16(const void* qkv, void* out, int64_t B, int64_t L, int64_t E, int64_t heads, int causal, void* stream);
/* y f16 [rows][ldy] = LayerNorm(x f16 [rows][ldx]) with f32 gamma / beta [E], statistics in fp32.  E % 8 == 0. */
int dbmm_layernorm_f16(const void* x, int64_t ldx, const float* gamma, const float* beta, void* y, int64_t ldy,
                       int64_t rows, int64_t E, float eps, void* stream);
/* NCHW image (f32, or f16 when x_is_f16) -> patch rows f16 [B*(R/P)^2][Kp], K = 3*P*P zero-padded to Kp. */
int dbmm_im2col_patch_f16(const void* x_nchw, int x_is_f16, void* out, int64_t B, int64_t R, int64_t P, int64_t Kp,
                          void* stream);
/* tokens f16 [B][L][W] = (class token | patches f16 [B*(L-1)][W]) + positional embedding (cls, pos f32). */
int dbmm_vit_tokens_f16(const void* patches, const float* cls, const float* pos, void* out, int64_t B, int64_t L,
                        int64_t W, void* stream);
/* out f16 [n][L][W] = table f32 [vocab][W][tokens] + pos f32 [L][W];  out f16 [n][W] = x f16 [n][L][W] at argmax(tokens). */
int dbmm_embed_gather_f16(const int32_t* tokens, const float* table, const float* pos, void* out, int64_t n, int64_t L,
                          int64_t W, int64_t vocab, void* stream);
int dbmm_gather_eot_f16(const int32_t* tokens, const void* x, void* out, int64_t n, int64_t L, int64_t W, void* stream);
int dbmm_cast_f32_f16(const float* x, void* y, int64_t n, void* stream);

/* ---------------------------------------------------------------------------------------
 * Device-side preprocessing (clip/clip.py:79-86: Resize(BICUBIC) -> CenterCrop -> ToTensor ->
 * Normalize) of one decoded RGB uint8 image [H][W][3] resident on the device.  Integer
 * resampling exactly as Pillow's 8-bit resampler (22-bit fixed-point coefficients, horizontal
 * then vertical pass, each rounded to uint8); the caller supplies the coefficient tables of
 * the R crop columns / rows (bounds = (first source index, tap count) pairs; the vertical
 * bounds relative to row0; see preprocess.py::resample_coeffs) as device int32 arrays.
 * mean3 / std3 are HOST pointers to 3 floats.  out_chw = float32 [3][R][R]; out_u8_hwc
 * (optional) = the resized + cropped uint8 image [R][R][3].  workspace >=
 * dbmm_workspace_bytes_preprocess(nrows, R) bytes.
 * ------------------------------------------------------------------------------------ */
size_t dbmm_workspace_bytes_preprocess(int64_t nrows, int64_t R);
int dbmm_resize_crop_normalize_u8(const uint8_t* img_hwc, int64_t H, int64_t W, const int32_t* h_bounds,
                                  const int32_t* h_coeffs, int64_t h_ksize, const int32_t* v_bounds,
                                  const int32_t* v_coeffs, int64_t v_ksize, int64_t row0, int64_t nrows,
                                  int64_t R, const float* mean3, const float* std3, float* out_chw,
                                  uint8_t* out_u8_hwc, void* workspace, size_t workspace_bytes, void* stream);
/* the same for a batch of B images of ONE geometry [B][H][W][3] (e.g. CelebA: every image 218 x 178) in two launches:
 * out_chw = float32 [B][3][R][R], out_u8_hwc (optional) [B][R][R][3], workspace >= B * dbmm_workspace_bytes_preprocess(nrows, R). */
int dbmm_resize_crop_normalize_u8_batch(const uint8_t* img_bhwc, int64_t B, int64_t H, int64_t W, const int32_t* h_bounds,
                                  const int32_t* h_coeffs, int64_t h_ksize, const int32_t* v_bounds,
                                  const int32_t* v_coeffs, int64_t v_ksize, int64_t row0, int64_t nrows,
                                  int64_t R, const float* mean3, const float* std3, float* out_chw,
                                  uint8_t* out_u8_hwc, void* workspace, size_t workspace_bytes, void* stream);

/* profiling aid: the 11 template arguments <BM,BN,WAVES_M,WAVES_N,AMODE,WMODE,BK,MINB,FAST,SK,DMA>
 * of the calling thread's most recent igemm launch (= the kernel name rocprofv3 reports). */
void dbmm_debug_last_igemm(int* out11);

/* `batch` independent GEMMs of identical shape in one launch (grid.y): problem b uses
 * a + b*stride_a, w + b*stride_w, bias + b*stride_bias, c + b*stride_c (element strides,
 * multiples of 4).  Used for the per-head products of the collapsed attention pool.
 *   op(a), op(w), alpha, act as in dbmm_gemm_bias_act (no residual); bias may be NULL; stride_w = 0 / stride_bias = 0 share one
 *   weight / bias between all problems.  ldc >= N (any value: rows are stored 16 B at a time when N and ldc are multiples of 4).
 *   1 <= batch <= 65535 (one grid row per problem), else DBMM_E_SHAPE; K % 4 != 0 (M % 4 != 0 with trans_a, N % 4 != 0 with
 *   trans_w) or ldc < N: DBMM_E_SHAPE; a, w, c or bias not 16-byte aligned, lda, ldw or one of the four strides (stride_bias when
 *   bias is given) not a multiple of 4: DBMM_E_ALIGN; a NULL a, w or c or an unknown act: DBMM_E_ARG.  Nothing is launched then. */
int dbmm_gemm_batched(const float* a, int64_t lda, int64_t stride_a, int trans_a, const float* w,
                      int64_t ldw, int64_t stride_w, int trans_w, const float* bias,
                      int64_t stride_bias, float* c, int64_t ldc, int64_t stride_c, int64_t M,
                      int64_t N, int64_t K, int64_t batch, float alpha, int act, void* stream);

/* ---------------------------------------------------------------------------------------
 * ModifiedResNet pieces (clip/model.py:94-154)
 * ------------------------------------------------------------------------------------ */

/* stem conv1: 3x3 stride 2 pad 1 on the NCHW image, BN folded, ReLU, NHWC out
 * (clip/model.py:108-110,140).  w is [3][3][3][Cout] = (kh, kw, cin, cout).  y_absmax (optional,
 * zeroed by the caller) receives max|y| like dbmm_conv_bn_act_x2's. */
int dbmm_conv_stem_s2(const float* x_nchw, const float* w, const float* bias, float* y_nhwc,
                      float* y_absmax, int64_t B, int64_t H, int64_t W, int64_t Cout, void* stream);

/* AvgPool2d(k) with kernel = stride = k, NHWC (clip/model.py:25,37,117). C % 4 == 0. */
int dbmm_avgpool2d(const float* x, float* y, int64_t B, int64_t H, int64_t W, int64_t C,
                   int64_t k, void* stream);

/* AttentionPool2d.forward (clip/model.py:68-91) on x[B,HW,C] (NHWC feature map).
 *   pos [HW+1][C]; wq [C][C] bq [C]; wkv [2C][C] bkv [2C] (k rows then v rows);
 *   wc [Dout][C] bc [Dout]; out [B][Dout].
 * workspace: dbmm_workspace_bytes_attnpool(B, HW, C) bytes. */
size_t dbmm_workspace_bytes_attnpool(int64_t B, int64_t HW, int64_t C);
int dbmm_attnpool(const float* x, const float* pos, const float* wq, const float* bq,
                  const float* wkv, const float* bkv, const float* wc, const float* bc,
                  float* out, int64_t B, int64_t HW, int64_t C, int64_t heads, int64_t Dout,
                  void* workspace, size_t workspace_bytes, void* stream);
/* The same on an fp32 (x_is_f16 = 0) or fp16 (1) feature map: the fp16 mode of the ModifiedResNet towers hands its fp16 map over without a
 * cast pass; tokens, projections and softmax stay in fp32 as above. */
int dbmm_attnpool_x(const void* x, int x_is_f16, const float* pos, const float* wq, const float* bq,
                    const float* wkv, const float* bkv, const float* wc, const float* bc, float* out,
                    int64_t B, int64_t HW, int64_t C, int64_t heads, int64_t Dout, void* workspace,
                    size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------
 * Transformer pieces (clip/model.py:157-240, 343-356)
 * ------------------------------------------------------------------------------------ */

/* LayerNorm over the last dim, fp32 statistics (clip/model.py:157-163).
 * x rows start at x + r*ldx (lets ln_post read only token 0 of every image).  y_absmax
 * (optional, zeroed by the caller) receives max|y| for a following dbmm_gemm_bias_act_x2. */
int dbmm_layernorm(const float* x, int64_t ldx, const float* gamma, const float* beta, float* y,
                   int64_t ldy, int64_t rows, int64_t E, float eps, float* y_absmax, void* stream);

/* softmax(q k^T * hd^-0.5 [+ causal mask]) v for packed qkv[B*L][3E] (batch-first rows),
 * head h uses columns [h*64, h*64+64) of each third.  head_dim must be 64 (all CLIP models).
 * Replaces the attention core inside nn.MultiheadAttention (clip/model.py:185-187). */
int dbmm_mha_core(const float* qkv, float* out, int64_t B, int64_t L, int64_t E, int64_t heads,
                  int causal, void* stream);

/* The same attention core on the 16-bit matrix cores at fp32 accuracy: q, k, v as fp16 (hi, lo) pairs under the exact
 * power-of-two scale derived from qkv_absmax (device scalar >= max|qkv|, the qkv GEMM's c_absmax), p as a pair under
 * 2^13, three partial products per fp32 product, fp32 accumulation (csrc/mha_pair.hip).  Same layouts as
 * dbmm_mha_core. */
int dbmm_mha_core_x2(const float* qkv, const float* qkv_absmax, float* out, int64_t B, int64_t L, int64_t E,
                     int64_t heads, int causal, void* stream);

/* x[n][L][W] = table[tokens[n][l]] + pos[l]  (clip/model.py:344-346).  tokens int32. */
int dbmm_embed_gather(const int32_t* tokens, const float* table, const float* pos, float* out,
                      int64_t n, int64_t L, int64_t W, int64_t vocab, void* stream);

/* patch im2col for the ViT stem conv (kernel = stride = P, clip/model.py:211,224):
 * out[B*g*g][3*P*P] in (cin, kh, kw) order = the flattened conv weight's K order. */
/* (out_absmax: optional device scalar, zeroed by the caller, receives max|out| = max|x| for the fp16-pair patch GEMM) */
int dbmm_im2col_patch(const float* x_nchw, float* out, float* out_absmax, int64_t B, int64_t R, int64_t P, void* stream);

/* tokens[B][g*g+1][W] = concat(class_embedding, patches[B][g*g][W]) + pos (clip/model.py:227-228) */
int dbmm_vit_tokens(const float* patches, const float* cls, const float* pos, float* out,
                    int64_t B, int64_t L, int64_t W, void* stream);

/* out[n][W] = x[n][eot[n]][W] where eot[n] = argmax_l tokens[n][l] (clip/model.py:354) */
int dbmm_gather_eot(const int32_t* tokens, const float* x, float* out, int64_t n, int64_t L,
                    int64_t W, void* stream);

/* ---------------------------------------------------------------------------------------
 * Adapter step (final_main.py:53-174, 426-496; demo/util.py:118-136)
 * ------------------------------------------------------------------------------------ */

/* BatchNorm1d batch statistics of h[B][H] (train mode): mean, invstd = rsqrt(biased var+eps);
 * running stats updated with momentum and the unbiased variance; nbt (int64) += 1.
 * running_* / nbt may be NULL. */
int dbmm_bn1d_stats(const float* h, int64_t B, int64_t H, float eps, float momentum, float* mean,
                    float* invstd, float* running_mean, float* running_var, int64_t* nbt,
                    void* stream);

/* r = relu(gamma * (h - mean) * invstd + beta).  var_mode = 1: the `invstd` argument holds a
 * variance (running_var, eval mode) and rsqrt(var + eps) is applied on the fly. */
int dbmm_bn1d_relu(const float* h, const float* mean, const float* invstd, const float* gamma,
                   const float* beta, float* r, int64_t B, int64_t H, int var_mode, float eps,
                   void* stream);

/* Adapter.forward (final_main.py:173): z = Linear2(relu(bn(Linear1(x)))).
 * train != 0: batch statistics (saved to mean/invstd, running stats updated).
 * Saves h (pre-BN) and r (post-ReLU) for the backward pass.
 * B <= 0, D <= 0, H <= 0, D % 4 != 0, H % 4 != 0, or train with B < 2: DBMM_E_SHAPE, like dbmm_adapter_bwd.  The shape is checked
 * before the first launch: a refused call leaves running_mean, running_var and nbt as they were. */
int dbmm_adapter_fwd(const float* x, const float* w1, const float* b1, const float* gamma,
                     const float* beta, float* running_mean, float* running_var, int64_t* nbt,
                     const float* w2, const float* b2, float* h, float* mean, float* invstd,
                     float* r, float* z, int64_t B, int64_t D, int64_t H, int train, float eps,
                     float momentum, void* stream);

/* Gradients of the adapter parameters given dz = dLoss/dz[B][D] (no grad w.r.t. x:
 * embeddings.detach(), final_main.py:455).  workspace: dbmm_workspace_bytes_adapter_bwd. */
size_t dbmm_workspace_bytes_adapter_bwd(int64_t B, int64_t D, int64_t H);
int dbmm_adapter_bwd(const float* x, const float* dz, const float* h, const float* mean,
                     const float* invstd, const float* r, const float* gamma, const float* beta,
                     const float* w2, float* dw1, float* db1, float* dgamma, float* dbeta,
                     float* dw2, float* db2, int64_t B, int64_t D, int64_t H, void* workspace,
                     size_t workspace_bytes, void* stream);

/* y[B][D] = x / ||x||_row, no epsilon (CLIP.forward, clip/model.py:362-363).  D % 4 == 0. */
int dbmm_l2norm_rows(const float* x, float* y, int64_t B, int64_t D, void* stream);

/* out[N] = sum over the B rows of x[B][N] in a fixed order (bias gradient of LinearClassifier, final_main.py:43-49).  N % 4 == 0. */
int dbmm_colsum(const float* x, float* out, int64_t B, int64_t N, void* stream);

/* tn[C][D] = (text[D][C] / ||text[:,c]||)^T  (final_main.py:77, column normalisation) */
int dbmm_text_colnorm(const float* text, float* tn, int64_t D, int64_t C, void* stream);

/* Fused row L2-norm + image x text logits + cross-entropy (final_main.py:68,78,302;
 * MultipleAdapter blend :123-127,138; zero-shot tail clip_inference.py:207-216):
 *   f = z/||z||;  feat = f                      (z_old == NULL)
 *                 feat = w*z_old/||z_old|| + (1-w)*f
 *   logits[b][c] = feat . tn[c] / T;   loss_rows[b] = CE(logits[b], labels[b]);
 *   pred[b] = argmax_c logits[b][c].
 * inv_norm[B] (1/||z||) is saved for the backward.  labels/loss_rows/pred/inv_norm may be
 * NULL.  C <= 8.  loss_mean (1 float, may be NULL) = mean of loss_rows.
 * Ids (every head, step and sweep entry of this header follows these rules; an id is compared as the 64-bit value it is, so
 * 2^32 + 1 is neither class 1 nor group 1):
 *   label outside [0, C): loss_rows[b] is NaN (and so is every mean or sum that takes it in); the row's logits and pred are
 *     unaffected; the backward subtracts no one-hot for it (dz and the parameters stay finite); a sweep counts the row in its
 *     group's n and never as correct.  Label -100 is such a label and nothing more: there is no ignore_index.
 *   group id outside [0, G): the row is in no counter, neither n nor correct; under group DRO it has weight 0 and is in no n_g or L_g.
 *   row index outside [0, n_rows) in a sweep's idx: clamped to 0 or n_rows - 1 at every use -- the embedding row, its label, its
 *     group and its row weight.
 * pred is the FIRST maximum of the row (the lower class on a tie), and so is the argmax behind the sweeps' counters. */
int dbmm_l2norm_sim_ce_fwd(const float* z, const float* z_old, float ebd_weight, const float* tn,
                           const int64_t* labels, float temperature, float* logits,
                           float* loss_rows, float* loss_mean, int64_t* pred, float* inv_norm,
                           int64_t B, int64_t D, int64_t C, void* stream);

/* dz[B][D] through the blend weight (1-w) and the row normalisation.
 *   dlogits == NULL: loss = grad_scale * mean_b CE; the softmax is recomputed from `logits`
 *                    and `labels` (fused training path).
 *   dlogits != NULL: dLoss/dlogits [B][C] is given by the caller (autograd of an external
 *                    criterion, e.g. nn.CrossEntropyLoss at final_main.py:456); logits, labels
 *                    and grad_scale are ignored.
 * A label outside [0, C) (64-bit compare) gets softmax * scale with no one-hot subtracted; see dbmm_l2norm_sim_ce_fwd. */
int dbmm_l2norm_sim_ce_bwd(const float* z, const float* inv_norm, float ebd_weight, int blended,
                           const float* tn, const float* logits, const int64_t* labels,
                           const float* dlogits, float temperature, float grad_scale, float* dz,
                           int64_t B, int64_t D, int64_t C, void* stream);

/* torch.optim.SGD step (demo/util.py:118-136; dampening 0, no nesterov) on n tensors in one
 * launch: g' = g + wd*p; buf = first ? g' : mu*buf + g'; p -= lr*buf.   n <= 16. */
int dbmm_sgd_momentum(int64_t n, float* const* params, const float* const* grads,
                      float* const* bufs, const int64_t* sizes, float lr, float momentum,
                      float weight_decay, int first_step, void* stream);

/* One training-step body in one call (final_main.py:455-466, :610-623): adapter forward (train-mode
 * BN), optional frozen old adapter (MultipleAdapter: pass o_* = NULL for CustomCLIP), fused
 * normalise + logits + CE, backward, SGD-momentum on the six trainable tensors (m_* = momentum
 * buffers).  ~20 kernel launches enqueued back to back, no host round trips.  tn = [C][D] from
 * dbmm_text_colnorm.  Outputs: logits [B][C], loss_rows [B], loss_mean [1]. */
size_t dbmm_workspace_bytes_adapter_train_step(int64_t B, int64_t D, int64_t H, int with_old);
int dbmm_adapter_train_step(const float* x, const int64_t* labels, float* w1, float* b1, float* gamma,
                            float* beta, float* running_mean, float* running_var, int64_t* nbt,
                            float* w2, float* b2, float* m_w1, float* m_b1, float* m_gamma,
                            float* m_beta, float* m_w2, float* m_b2, const float* o_w1,
                            const float* o_b1, const float* o_gamma, const float* o_beta,
                            float* o_running_mean, float* o_running_var, int64_t* o_nbt,
                            const float* o_w2, const float* o_b2, float ebd_weight, const float* tn,
                            float temperature, float lr, float momentum, float weight_decay,
                            int first_step, float* logits, float* loss_rows, float* loss_mean,
                            int64_t B, int64_t D, int64_t H, int64_t C, void* workspace,
                            size_t workspace_bytes, void* stream);

/* Online group DRO (Sagawa et al. 2020, "Distributionally Robust Neural Networks for Group Shifts", Algorithm 1) on the per-row
 * CE of a batch.  loss_rows fp32 [B], groups int64 [B], q_in / q_out fp32 [G] (may be the same array), eta the step size:
 *   n_g = rows of group g, L_g = mean loss of group g (float64 sums in a fixed order; 0 when n_g = 0), m = max L_g over the groups
 *   present, q'_g = q_g exp(eta (L_g - m)) (absent groups: L_g = 0), q_out = q' / sum q', robust_loss [1] = sum_g q_out_g L_g.
 * weights fp32 [3][G]: row 0 the row weights q_out_g / n_g (0 for an absent group), row 1 L_g, row 2 n_g.  A group id outside
 * [0, G) belongs to no bucket.  One launch of one workgroup; identical inputs give identical bits.
 * NULL pointer: DBMM_E_ARG; G outside 1..8 or B < 2: DBMM_E_SHAPE. */
int dbmm_group_dro_weights(const float* loss_rows, const int64_t* groups, const float* q_in, float* q_out, float* weights,
                           float* robust_loss, int64_t B, int64_t G, float eta, void* stream);

/* dbmm_l2norm_sim_ce_bwd's fused training path with a weight per row: loss = sum_b weights[groups[b]] CE_b (row 0 of
 * dbmm_group_dro_weights' output; weight 0 for a group id outside [0, G): that row's dz is exactly 0).  Labels as in
 * dbmm_l2norm_sim_ce_bwd.  G outside 1..8 or B < 2: DBMM_E_SHAPE, as dbmm_group_dro_weights. */
int dbmm_l2norm_sim_ce_bwd_weighted(const float* z, const float* inv_norm, float ebd_weight, int blended, const float* tn,
                                    const float* logits, const int64_t* labels, const int64_t* groups,
                                    const float* weights, int64_t G, float temperature, float* dz, int64_t B, int64_t D,
                                    int64_t C, void* stream);

/* dbmm_adapter_train_step under group DRO: the step minimises sum_g q_g L_g instead of the batch mean.  groups int64 [B],
 * q fp32 [G] (device state, updated in place by the step), eta the step size of q; robust_loss [1] takes loss_mean's place.
 * Same workspace.  Two launches more than dbmm_adapter_train_step (10 / 13 on the fast shape): the head is forward rows, the
 * group reduction + q update, weighted backward rows. */
int dbmm_adapter_train_step_gdro(const float* x, const int64_t* labels, float* w1, float* b1, float* gamma,
                                 float* beta, float* running_mean, float* running_var, int64_t* nbt,
                                 float* w2, float* b2, float* m_w1, float* m_b1, float* m_gamma,
                                 float* m_beta, float* m_w2, float* m_b2, const float* o_w1,
                                 const float* o_b1, const float* o_gamma, const float* o_beta,
                                 float* o_running_mean, float* o_running_var, int64_t* o_nbt,
                                 const float* o_w2, const float* o_b2, float ebd_weight, const float* tn,
                                 float temperature, float lr, float momentum, float weight_decay,
                                 int first_step, float* logits, float* loss_rows, float* robust_loss,
                                 const int64_t* groups, float* q, float eta, int64_t G,
                                 int64_t B, int64_t D, int64_t H, int64_t C, void* workspace,
                                 size_t workspace_bytes, void* stream);

/* Supervised-contrastive head (csrc/supcon.hip; Khosla et al. 2020, the reference's SupervisedContrastiveLoss batched over all
 * anchors).  z fp32 [B][D] (D % 4 == 0), labels int64 [B] (any values; only equality is used), tau the temperature:
 *   zn_i = z_i / ||z_i||,  S_ij = zn_i . zn_j / tau (j != i; the diagonal is excluded by index),  P(i) = { j != i : y_j == y_i },
 *   l_i = logsumexp_{j != i} S_ij - mean_{j in P(i)} S_ij  (0 for a row without positives),
 *   A = #{ i : |P(i)| > 0 },  L_con = sum_i l_i / A  (A == 0: L_con = 0 and a zero gradient).
 * The products run on the exact-fp32 MFMA; no floating-point atomics: identical inputs give identical bits.
 * dbmm_supcon_fwd, 2 launches (64 x 64 Gram tiles with per-row partials; one workgroup that merges them in column-tile order and
 * sums L_con in float64 in row order).  Outputs: con_loss [1] = L_con, loss_rows [B] = l_i, n_anchors [1] = A (as a float),
 * stats [4][B] = row max of S | sum_j exp(S_ij - max) | |P(i)| | 1 / ||z_i||.  ce_rows [B] (may be NULL; then mixed_loss may be
 * NULL too): per-row CE of the same batch, and mixed_loss [1] = fma(1 - weight, mean(ce_rows), weight * L_con).  The workspace
 * keeps S for the backward.
 * dbmm_supcon_bwd, 1 launch: dz [B][D] = fma(dz_in_scale, dz_in, weight * dL_con/dz) (dz_in may be NULL: weight * dL_con/dz; or dz
 * itself), from the forward's stats, n_anchors and workspace.
 * NULL pointer: DBMM_E_ARG; B < 2, D <= 0, D % 4 != 0 or tau <= 0: DBMM_E_SHAPE; B > 2048: DBMM_E_UNSUPPORTED (nothing is
 * launched); a workspace below dbmm_supcon_workspace_bytes(B, D): DBMM_E_WORKSPACE; z or the workspace not 16-byte aligned:
 * DBMM_E_ALIGN.  dbmm_supcon_workspace_bytes is 0 for a B outside 2 .. 2048. */
size_t dbmm_supcon_workspace_bytes(int64_t B, int64_t D);
int dbmm_supcon_fwd(const float* z, const int64_t* labels, float temperature, const float* ce_rows, float weight,
                    float* con_loss, float* mixed_loss, float* loss_rows, float* stats, float* n_anchors, int64_t B,
                    int64_t D, void* workspace, size_t workspace_bytes, void* stream);
int dbmm_supcon_bwd(const float* z, const int64_t* labels, float temperature, const float* stats, const float* n_anchors,
                    float weight, const float* dz_in, float dz_in_scale, float* dz, int64_t B, int64_t D,
                    const void* workspace, size_t workspace_bytes, void* stream);

/* dbmm_adapter_train_step with the contrastive head: the step minimises (1 - weight) * mean CE + weight * L_con, L_con the
 * supervised-contrastive loss of the TRAINABLE adapter's output z (not the blend with the old branch) under `labels` at
 * temperature tau.  loss_mean [1] receives the mixed loss, con_loss [1] L_con.  The workspace is that of
 * dbmm_adapter_train_step followed by dbmm_supcon_workspace_bytes(B, D) more bytes.  Three launches more than
 * dbmm_adapter_train_step (11 / 14 on the fast shape): Gram tiles, the reduction + the mixed loss, the contrastive backward onto
 * the CE head's dz.  B > 2048: DBMM_E_UNSUPPORTED, nothing launched. */
int dbmm_adapter_train_step_supcon(const float* x, const int64_t* labels, float* w1, float* b1, float* gamma,
                                   float* beta, float* running_mean, float* running_var, int64_t* nbt,
                                   float* w2, float* b2, float* m_w1, float* m_b1, float* m_gamma,
                                   float* m_beta, float* m_w2, float* m_b2, const float* o_w1,
                                   const float* o_b1, const float* o_gamma, const float* o_beta,
                                   float* o_running_mean, float* o_running_var, int64_t* o_nbt,
                                   const float* o_w2, const float* o_b2, float ebd_weight, const float* tn,
                                   float temperature, float lr, float momentum, float weight_decay,
                                   int first_step, float* logits, float* loss_rows, float* loss_mean,
                                   float weight, float tau, float* con_loss,
                                   int64_t B, int64_t D, int64_t H, int64_t C, void* workspace,
                                   size_t workspace_bytes, void* stream);

/* Contrastive head over sampled sets (csrc/supcon_sets.hip; Zhang & Re 2022, "Contrastive Adapters for Foundation Model Group
 * Robustness": the reference's SupervisedContrastiveLoss, one anchor per call, for T calls at once).  z fp32 [T S][D] (D % 4 == 0):
 * T sets of S = A + P + N rows; row 0 of a set is the anchor, rows A .. A+P-1 its positives, the last N rows its negatives; the
 * extra anchors (rows 1 .. A-1) take no loss and get a zero gradient.
 *   zn = z / ||z||,  c_j = zn_a . zn_j,  s_j = c_j / tau  (j in P u N),
 *   l_t = log sum_{P u N} exp(s_j) - (1 / P) sum_P s_p,  L = scale * sum_t l_t  (the sum over t in float64, in set order).
 * The dots are fp32 FMA chains in a fixed order; no floating-point atomics: identical inputs give identical bits.
 * dbmm_supcon_sets_fwd, 2 launches (one workgroup per set and chunk of 32 rows; one workgroup that merges the chunk partials in a fixed
 * order).  Outputs: loss [1] = L, loss_sets [T] = l_t (unscaled).  The workspace keeps c_j, 1 / ||z_j|| and the sets' max and sum
 * of exp for the backward.
 * dbmm_supcon_sets_bwd, 2 launches: dz [T S][D] = dL/dz from the forward's workspace (the same T, A, P, N, D, scale and tau).
 * NULL pointer: DBMM_E_ARG; T < 1, A < 1, P < 1, N < 1, D <= 0, D % 4 != 0, tau <= 0, T > 65535 or T S >= 2^31: DBMM_E_SHAPE;
 * D > 8192: DBMM_E_UNSUPPORTED; a workspace below dbmm_supcon_sets_workspace_bytes(T, S, D): DBMM_E_WORKSPACE; z, dz or the workspace
 * not 16-byte aligned: DBMM_E_ALIGN.  Nothing is launched on refusal.  dbmm_supcon_sets_workspace_bytes is 0 for a shape that is refused. */
size_t dbmm_supcon_sets_workspace_bytes(int64_t T, int64_t S, int64_t D);
int dbmm_supcon_sets_fwd(const float* z, float scale, float temperature, float* loss, float* loss_sets, int64_t T, int64_t A,
                         int64_t P, int64_t N, int64_t D, void* workspace, size_t workspace_bytes, void* stream);
int dbmm_supcon_sets_bwd(const float* z, float scale, float temperature, float* dz, int64_t T, int64_t A, int64_t P, int64_t N,
                         int64_t D, void* workspace, size_t workspace_bytes, void* stream);

/* One training step of the contrastive adapter in one call: dbmm_adapter_fwd (train-mode BatchNorm over the step's T S rows as ONE
 * batch), dbmm_supcon_sets_fwd, dbmm_supcon_sets_bwd, the adapter backward, SGD-momentum on the six trainable tensors.  The step
 * minimises L = scale * sum_t l_t and nothing else: no text matrix, no CE.  x fp32 [T S][D]; loss [1] = L, loss_sets [T] = l_t.
 * 11 launches.  The adapter's fast shape only (H == 128, D % 128 == 0, T S <= 2^20, x 16-byte aligned; else DBMM_E_UNSUPPORTED,
 * nothing launched); other refusals as dbmm_supcon_sets_fwd.  Workspace: dbmm_workspace_bytes_adapter_train_step_sets(T, S, D, H). */
size_t dbmm_workspace_bytes_adapter_train_step_sets(int64_t T, int64_t S, int64_t D, int64_t H);
int dbmm_adapter_train_step_sets(const float* x, float* w1, float* b1, float* gamma, float* beta, float* running_mean,
                                 float* running_var, int64_t* nbt, float* w2, float* b2, float* m_w1, float* m_b1,
                                 float* m_gamma, float* m_beta, float* m_w2, float* m_b2, float lr, float momentum,
                                 float weight_decay, int first_step, float scale, float tau, float* loss, float* loss_sets,
                                 int64_t T, int64_t A, int64_t P, int64_t N, int64_t D, int64_t H, void* workspace,
                                 size_t workspace_bytes, void* stream);

/* Replica-batched adapter step (csrc/adapter_sweep.hip): R <= 16 independent runs of one sweep group take one training step in
 * the launches of ONE dbmm_adapter_train_step (8, or 11 with a frozen old adapter), the replica being a grid dimension.  Fast shape
 * only (H == 128, D % 128 == 0; else DBMM_E_UNSUPPORTED); replica r's results are the bits dbmm_adapter_train_step gives for r alone.
 *   table [n_rows][D], labels / groups [n_rows]: one shared embedding table; idx [idx_R][idx_B] (= [R][B], else DBMM_E_SHAPE): replica
 *     r trains on rows idx[r][:], read in place (indices are clamped into the table -- to row 0 or n_rows - 1, as 64-bit values,
 *     for the embedding row, its label and its group alike; repeats are legal)
 *   params: 9 device pointers to stacked [R, ...] tensors (w1, b1, gamma, beta, running_mean, running_var, nbt int64 [R], w2, b2);
 *     bufs: the 6 stacked momentum buffers (w1, b1, gamma, beta, w2, b2); old: 9 pointers of the frozen adapters, or NULL.  The
 *     three arrays and lr [R] are HOST arrays, read during the call (the learning rates travel as kernel arguments)
 *   logits [R][B][C], loss_rows [R][B], loss_mean [R]: outputs.  counted != 0: counts int64 [R][G][2] += (n, correct) per group and
 *     loss_sum double [R] += (double)loss_mean * B, by the step's own launches.  B < 2: DBMM_E_SHAPE (train-mode BatchNorm1d).
 *     G outside 1..64: DBMM_E_SHAPE.  A row whose group id is outside [0, G) (64-bit compare) is in no counter; a row whose label
 *     is outside [0, C) has loss_rows NaN, is counted in its group's n, never as correct, and gets no one-hot in the backward
 *     (the id rules at dbmm_l2norm_sim_ce_fwd). */
size_t dbmm_workspace_bytes_adapter_sweep_step(int64_t R, int64_t B, int64_t D, int64_t H, int with_old);
int dbmm_adapter_sweep_step(const float* table, int64_t n_rows, const int64_t* idx, int64_t idx_R, int64_t idx_B,
                            const int64_t* labels, const int64_t* groups, void* const* params, float* const* bufs,
                            void* const* old, float ebd_weight, const float* tn, float temperature, const float* lr,
                            float momentum, float weight_decay, int first_step, float* logits, float* loss_rows,
                            float* loss_mean, int64_t* counts, double* loss_sum, int64_t G, int counted, int64_t R,
                            int64_t B, int64_t D, int64_t H, int64_t C, void* workspace, size_t workspace_bytes,
                            void* stream);

/* dbmm_adapter_sweep_step under group DRO: replica r takes the step dbmm_adapter_train_step_gdro takes for r alone (same bits).
 * The groups of the robust loss are `groups` (G <= 8 here), q fp32 [R][G] is updated in place, robust_loss [R] takes loss_mean's
 * place and is what loss_sum accumulates (times B).  Same workspace; two launches more than dbmm_adapter_sweep_step.  A row whose
 * group id is outside [0, G) (64-bit compare) has weight 0, is in no n_g or L_g and in no counter; labels and indices as in
 * dbmm_adapter_sweep_step. */
int dbmm_adapter_sweep_step_gdro(const float* table, int64_t n_rows, const int64_t* idx, int64_t idx_R, int64_t idx_B,
                                 const int64_t* labels, const int64_t* groups, void* const* params, float* const* bufs,
                                 void* const* old, float ebd_weight, const float* tn, float temperature, const float* lr,
                                 float momentum, float weight_decay, int first_step, float* logits, float* loss_rows,
                                 float* robust_loss, int64_t* counts, double* loss_sum, int64_t G, int counted, float* q,
                                 float eta, int64_t R, int64_t B, int64_t D, int64_t H, int64_t C, void* workspace,
                                 size_t workspace_bytes, void* stream);

/* Replica-batched evaluation forward: eval-mode adapters (running statistics; old + new blend when `old`), cosine logits, per-row
 * CE, group counters and the float64 loss sum (loss_sum[r] += sum_b (double)loss_rows[r][b], fixed order) of R replicas over the
 * SAME B rows: idx [B] rows of the table (clamped into it as in dbmm_adapter_sweep_step), or idx == NULL: rows row0 .. row0 + B - 1
 * (row0 < 0 or row0 + B > n_rows: DBMM_E_SHAPE).  5 launches (8 with `old`).  Out-of-range labels and group ids as in
 * dbmm_adapter_sweep_step. */
size_t dbmm_workspace_bytes_adapter_sweep_eval(int64_t R, int64_t B, int64_t D, int64_t H, int with_old);
int dbmm_adapter_sweep_eval(const float* table, int64_t n_rows, const int64_t* idx, int64_t row0, const int64_t* labels,
                            const int64_t* groups, void* const* params, void* const* old, float ebd_weight,
                            const float* tn, float temperature, float* logits, float* loss_rows, int64_t* counts,
                            double* loss_sum, int64_t G, int64_t R, int64_t B, int64_t D, int64_t H, int64_t C,
                            void* workspace, size_t workspace_bytes, void* stream);

/* One training step of the linear probe (final_main.py:43-49 LinearClassifier, trained at :426-496) in one call:
 * logits = x W^T + b, per-row CE and its mean, dlogits = (softmax - onehot) / B, dW = dlogits^T x, db = colsum dlogits, then
 * dbmm_sgd_momentum's update of w, b and their momentum buffers m_w, m_b in place.  x [B][D], labels int64 [B] in [0, C),
 * w / m_w [C][D], b / m_b [C]; outputs logits [B][C], loss_rows [B], loss_mean [1].  C <= 8, D % 4 == 0, D <= 1024, any B >= 1.
 * A label outside [0, C), compared as a 64-bit value (-100 included: no ignore_index): loss_rows[b] and loss_mean are NaN, the row's
 * logits are unaffected and no one-hot is subtracted, so w, b and the momenta stay finite.
 * Every sum runs in a fixed order: identical inputs give identical bits.  One kernel launch (after a 4-byte memset of the
 * workspace's ticket counter) up to the batch size of the option linear_step_one_launch_max_b, two launches above it.
 * x, w, m_w and the workspace 16-byte aligned; workspace = dbmm_workspace_bytes_linear_train_step(B, D, C) bytes (0: bad shape). */
size_t dbmm_workspace_bytes_linear_train_step(int64_t B, int64_t D, int64_t C);
int dbmm_linear_train_step(const float* x, const int64_t* labels, float* w, float* b, float* m_w, float* m_b,
                           float lr, float momentum, float weight_decay, int first_step,
                           float* logits, float* loss_rows, float* loss_mean,
                           int64_t B, int64_t D, int64_t C, void* workspace, size_t workspace_bytes, void* stream);

/* The linear probe's eval forward (validate, final_main.py:655-713): logits, per-row CE and the mean, no update.  Same shapes and
 * rules as dbmm_linear_train_step; workspace = dbmm_workspace_bytes_linear_ce_fwd(B) bytes. */
size_t dbmm_workspace_bytes_linear_ce_fwd(int64_t B);
int dbmm_linear_ce_fwd(const float* x, const float* w, const float* b, const int64_t* labels,
                       float* logits, float* loss_rows, float* loss_mean, int64_t B, int64_t D, int64_t C,
                       void* workspace, size_t workspace_bytes, void* stream);

/* Replica-batched linear-probe step (csrc/linear_sweep.hip): R <= 16 independent runs of one sweep group take one training step in
 * the launches of ONE dbmm_linear_train_step (one memset of the R ticket counters + one kernel up to the option
 * linear_step_one_launch_max_b, two kernels above it), the replica being a grid dimension.  Replica r's logits, loss_rows, loss_mean,
 * w, b, m_w, m_b are the bits dbmm_linear_train_step gives for r alone on table[idx[r]].
 *   table [n_rows][D], labels / groups [n_rows]: one shared embedding table; idx [idx_R][idx_B] (= [R][B], else DBMM_E_SHAPE): replica
 *     r trains on rows idx[r][:], read in place (indices are clamped into the table -- to row 0 or n_rows - 1, as 64-bit values,
 *     for the embedding row, its label, its group and its row weight alike; repeats are legal)
 *   w / m_w [R][C][D], b / m_b [R][C]: stacked; lr [R] is a HOST array, read during the call (the rates travel as kernel arguments)
 *   logits [R][B][C], loss_rows [R][B], loss_mean [R]: outputs.  counted != 0: counts int64 [R][G][2] += (n, correct) per group and
 *     loss_sum double [R] += (double)loss_mean[r] * B, by the step's own launches.  A row whose group id is outside [0, G) (64-bit
 *     compare) is in no counter; a row whose label is outside [0, C) scores NaN (dbmm_linear_train_step), is counted in its
 *     group's n and never as correct.
 * R outside 1..16, C outside 1..8, D % 4 != 0, D > 1024, G outside 1..64: DBMM_E_SHAPE.  table, w, m_w and the workspace 16-byte
 * aligned; workspace = dbmm_workspace_bytes_linear_sweep_step(R, B, D, C) bytes (linear in R; 0: bad shape). */
size_t dbmm_workspace_bytes_linear_sweep_step(int64_t R, int64_t B, int64_t D, int64_t C);
int dbmm_linear_sweep_step(const float* table, int64_t n_rows, const int64_t* idx, int64_t idx_R, int64_t idx_B,
                           const int64_t* labels, const int64_t* groups, float* w, float* b, float* m_w, float* m_b,
                           const float* lr, float momentum, float weight_decay, int first_step, float* logits,
                           float* loss_rows, float* loss_mean, int64_t* counts, double* loss_sum, int64_t G, int counted,
                           int64_t R, int64_t B, int64_t D, int64_t C, void* workspace, size_t workspace_bytes, void* stream);

/* Replica-batched evaluation forward of the linear probe: logits [R][B][C] and per-row CE [R][B] (the bits of dbmm_linear_ce_fwd),
 * group counters and the float64 loss sum (loss_sum[r] += sum_b (double)loss_rows[r][b], fixed order) of R replicas over the SAME B
 * rows: idx [B] rows of the table (clamped into it), or idx == NULL: rows row0 .. row0 + B - 1 (outside the table: DBMM_E_SHAPE).
 * One memset + one kernel whatever R is.  w [R][C][D], b [R][C].  Out-of-range labels and group ids as in dbmm_linear_sweep_step. */
size_t dbmm_workspace_bytes_linear_sweep_eval(int64_t R, int64_t B);
int dbmm_linear_sweep_eval(const float* table, int64_t n_rows, const int64_t* idx, int64_t row0, const int64_t* labels,
                           const int64_t* groups, const float* w, const float* b, float* logits, float* loss_rows,
                           int64_t* counts, double* loss_sum, int64_t G, int64_t R, int64_t B, int64_t D, int64_t C,
                           void* workspace, size_t workspace_bytes, void* stream);

/* ---- per-row loss weights: L = (1 / B) sum_b row_w[b] CE_b -------------------------------------------------------------------
 * row_w is fp32 and taken as it is (no normalisation; the schedule rescales to mean 1 once, on the host).  Every entry is its
 * unweighted sibling with the row's gradient scale (1 / B) row_w[b] where that one has 1 / B and the mean taken over the terms
 * loss_rows[b] * row_w[b] in the sibling's order: the same launch count, workspace, shape / alignment rules and error codes, and
 * all-ones weights give the sibling's bits (parameters, momenta, running statistics, logits, loss_rows, loss).  logits and loss_rows
 * are the UNWEIGHTED ones; a row of weight 0 still takes part in train-mode BatchNorm statistics.  No float atomics; same bits on
 * every call.
 *   dbmm_weighted_mean               out = (sum_i x[i] row_w[i]) / n, one workgroup (the order of dbmm_l2norm_sim_ce_fwd's loss_mean)
 *   dbmm_l2norm_sim_ce_bwd_rows      dbmm_l2norm_sim_ce_bwd's fused path (logits + labels given) with row_w [B]
 *   dbmm_adapter_train_step_weighted dbmm_adapter_train_step with row_w [B]; workspace = dbmm_workspace_bytes_adapter_train_step
 *   dbmm_linear_train_step_weighted  dbmm_linear_train_step with row_w [B], on both of its launch paths
 *   dbmm_adapter_sweep_step_weighted, dbmm_linear_sweep_step_weighted
 *       the sweep steps with row_w [Rw][n_rows] over the TABLE's rows, Rw = 1 (shared by the replicas) or R (else DBMM_E_SHAPE):
 *       batch row b of replica r weighs row_w[(Rw == 1 ? 0 : r) * n_rows + idx[r][b] clamped into the table], the clamp the labels
 *       use, in the backward's gradient scale and in the weighted mean alike.  The group counters stay unweighted; counted != 0
 *       adds (double)L[r] * B to loss_sum[r]. */
int dbmm_weighted_mean(const float* x, const float* row_w, float* out, int64_t n, void* stream);
int dbmm_l2norm_sim_ce_bwd_rows(const float* z, const float* inv_norm, float ebd_weight, int blended, const float* tn,
                                const float* logits, const int64_t* labels, const float* row_w, float temperature,
                                float grad_scale, float* dz, int64_t B, int64_t D, int64_t C, void* stream);
int dbmm_adapter_train_step_weighted(const float* x, const int64_t* labels, float* w1, float* b1, float* gamma,
                                     float* beta, float* rmean, float* rvar, int64_t* nbt, float* w2, float* b2,
                                     float* m_w1, float* m_b1, float* m_gamma, float* m_beta, float* m_w2,
                                     float* m_b2, const float* o_w1, const float* o_b1, const float* o_gamma,
                                     const float* o_beta, float* o_rmean, float* o_rvar, int64_t* o_nbt,
                                     const float* o_w2, const float* o_b2, float ebd_weight, const float* tn,
                                     float temperature, float lr, float momentum, float weight_decay,
                                     int first_step, float* logits, float* loss_rows, float* loss_mean,
                                     const float* row_w, int64_t B, int64_t D, int64_t H, int64_t C, void* workspace,
                                     size_t workspace_bytes, void* stream);
int dbmm_adapter_sweep_step_weighted(const float* table, int64_t n_rows, const int64_t* idx, int64_t idx_R, int64_t idx_B,
                                     const int64_t* labels, const int64_t* groups, void* const* params, float* const* bufs,
                                     void* const* old, float ebd_weight, const float* tn, float temperature, const float* lr,
                                     float momentum, float weight_decay, int first_step, float* logits, float* loss_rows,
                                     float* loss_mean, int64_t* counts, double* loss_sum, int64_t G, int counted,
                                     const float* row_w, int64_t Rw, int64_t R, int64_t B, int64_t D, int64_t H, int64_t C,
                                     void* workspace, size_t workspace_bytes, void* stream);
int dbmm_linear_train_step_weighted(const float* x, const int64_t* labels, float* w, float* b, float* m_w, float* m_b,
                                    float lr, float momentum, float weight_decay, int first_step, float* logits,
                                    float* loss_rows, float* loss_mean, const float* row_w, int64_t B, int64_t D, int64_t C,
                                    void* workspace, size_t workspace_bytes, void* stream);
int dbmm_linear_sweep_step_weighted(const float* table, int64_t n_rows, const int64_t* idx, int64_t idx_R, int64_t idx_B,
                                    const int64_t* labels, const int64_t* groups, float* w, float* b, float* m_w, float* m_b,
                                    const float* lr, float momentum, float weight_decay, int first_step, float* logits,
                                    float* loss_rows, float* loss_mean, int64_t* counts, double* loss_sum, int64_t G,
                                    int counted, const float* row_w, int64_t Rw, int64_t R, int64_t B, int64_t D, int64_t C,
                                    void* workspace, size_t workspace_bytes, void* stream);

/* out[i][:] = table[idx[i]][:] -- batch assembly from a device-resident embedding table
 * (replaces the DataLoader + per-item DataFrame lookups of data/ *_embeddings*.py) */
int dbmm_gather_rows(const float* table, const int64_t* idx, float* out, int64_t n_rows,
                     int64_t n_idx, int64_t D, void* stream);

/* update_dict (final_main.py:383-391) on device: counts[g][0] += 1, counts[g][1] += (argmax
 * logits == y, first index on ties) for every row; counts is int64 [G][2], accumulated (not
 * cleared).  G <= 64.  Rows whose id is outside [0, G) -- compared as 64-bit values -- count
 * for no group, here and in dbmm_group_loss_sum. */
int dbmm_group_count(const float* logits, const int64_t* y, const int64_t* g, int64_t* counts,
                     int64_t B, int64_t C, int64_t G, void* stream);

/* Per-group mean CE (build-side addition): sums[g] += loss_rows over g. */
int dbmm_group_loss_sum(const float* loss_rows, const int64_t* g, float* sums, int64_t B,
                        int64_t G, void* stream);

/* Group-wise sums of pairwise Euclidean distances without the N x N matrix (the numbers of GetGroupWiseStatEbd's
 * compute_averaged_pairwise_distance, demo/visualizer.py:650-690, for the whole split and every group in ONE pass):
 *   sums double [G][G], symmetric: sums[a][b] = sum over unordered pairs i < j with {groups[i], groups[j]} = {a, b} of
 *   ||x[i] - x[j]||_2.  The whole split's sum is the sum of the upper triangle (diagonal included); group a's own is sums[a][a].
 * x fp32 [N][D] (contiguous), groups int64 [N] in [0, G) (a row with a label outside belongs to no bucket), center fp32 [D]: any
 * vector near the rows' mean -- it is subtracted before the products are formed (distances do not change, the cancellation does).
 * fp32-accurate products (hi + lo fp16 planes under a power-of-two scale, fp32 accumulation), float64 sums in a fixed order: two
 * calls on the same input give the same bits.  Four launches and one memset on `stream`.
 * D % 64 != 0 or D > 4096: DBMM_E_UNSUPPORTED; G outside 1..8, N outside 1..2^23: DBMM_E_SHAPE; x, center and the workspace
 * 16-byte aligned.  The workspace holds the planes (about N * D * 4 bytes) and 512 bytes per workgroup, never N x N. */
size_t dbmm_workspace_bytes_pairdist(int64_t N, int64_t D);
int dbmm_pairdist_group_sums(const float* x, const int64_t* groups, const float* center, double* sums, int64_t N,
                             int64_t D, int64_t G, void* workspace, size_t workspace_bytes, void* stream);

/* Group-wise sums of RBF kernel values for L bandwidths in one pass (what MMD^2 and HSIC need of the Gram matrix), without N x N:
 *   sums double [L][G][G], symmetric in (a, b): sums[l][a][b] = sum over unordered pairs i < j with {groups[i], groups[j]} = {a, b}
 *   of exp(-gammas[l] ||x[i] - x[j]||^2).  The diagonal is excluded by index: a V-statistic adds n_a (K_ii = 1) on the host.
 * Operands, centring, split, d^2 and the walk of dbmm_pairdist_group_sums: the same tile kernel with another element map.  d^2 stays
 * in the accumulator registers; per bandwidth every element goes through the hardware exp2 (the argument is <= 0, underflow to 0 is
 * the answer) and the distance kernel's reduction (lane, wave, eight wave slots, workgroup, workgroups in order: float64, no
 * floating-point atomics), so two calls give the same bits and a bandwidth's sums do not depend on L or on its position.
 * gammas: a HOST array of L finite doubles > 0, read at call time (else DBMM_E_ARG).  L outside 1..4, G outside 1..8, N outside
 * 1..2^23: DBMM_E_SHAPE; D % 64 != 0 or D > 4096: DBMM_E_UNSUPPORTED; x, center and the workspace 16-byte aligned.  A d^2 is good to
 * about 7e-7 of its two rows' centred squared norms, a kernel value relatively to gamma times that.  The workspace is its own size:
 * dbmm_workspace_bytes_pairdist's with L x 512 bytes per workgroup instead of 512 (0 for L outside 1..4). */
size_t dbmm_workspace_bytes_pairdist_rbf(int64_t N, int64_t D, int64_t L);
int dbmm_pairdist_rbf_group_sums(const float* x, const int64_t* groups, const float* center, const double* gammas, int64_t L,
                                 double* sums, int64_t N, int64_t D, int64_t G, void* workspace, size_t workspace_bytes,
                                 void* stream);

/* Per-row, per-group sums of Euclidean distances without the N x N matrix (what a silhouette needs of the distances):
 *   sums double [N][G]: sums[i][g] = sum over j != i with groups[j] == g of ||x[i] - x[j]||_2.
 * Operands, centring, split and distance arithmetic of dbmm_pairdist_group_sums; the kernel walks the full square of 256 x 256
 * tiles and reduces every tile along its columns.  A column j >= N or with a label outside [0, G) is in no sum; a row with such a
 * label still gets its G sums.  The diagonal is excluded by index: a group's only row has exactly 0 for its own group, and an empty
 * group's column is exactly 0.  fp32 over the 64 columns of a wave (a fixed tree of depth 6), float64 above that in a fixed order, no
 * floating-point atomics: two calls on the same input give the same bits.  Four launches and two memsets on `stream`.
 * D % 64 != 0 or D > 4096: DBMM_E_UNSUPPORTED; G outside 1..16, N outside 1..2^23: DBMM_E_SHAPE; x, center and the workspace
 * 16-byte aligned.  The workspace holds the planes (about N * D * 4 bytes), 8 bytes per row and up to 16 partial [N][G] float64
 * matrices (one per column chunk of the schedule), never N x N. */
size_t dbmm_workspace_bytes_pairdist_rows(int64_t N, int64_t D, int64_t G);
int dbmm_pairdist_row_group_sums(const float* x, const int64_t* groups, const float* center, double* sums, int64_t N,
                                 int64_t D, int64_t G, void* workspace, size_t workspace_bytes, void* stream);

/* Per-row, per-group sums of RBF kernel values for L bandwidths in one pass (what a Parzen-window probe, the MMD witness function and a
 * normalised HSIC / CKA need of the Gram matrix), without N x N:
 *   sums double [L][N][G]: sums[l][i][g] = sum over j != i with groups[j] == g of exp(-gammas[l] ||x[i] - x[j]||^2).
 * dbmm_pairdist_row_group_sums' tile kernel with dbmm_pairdist_rbf_group_sums' element map: d^2 (clamped at 0) stays in the accumulator
 * registers and every bandwidth takes it through the hardware exp2 and the rows kernel's reduction (the fp32 tree over a wave's 64
 * columns, then float64 over the column waves, tiles and chunks in a fixed order; no floating-point atomics), one bandwidth after the
 * other in a runtime loop: two calls give the same bits, and a bandwidth's sums do not depend on L or on its position.  The pair (i, i)
 * is excluded by index (its d^2 is set to +inf: an exact 0 at every bandwidth), so a label's sum for the label's only row and the sums
 * of an empty label are exactly 0.  A column j >= N or with a label outside [0, G) -- compared as 64-bit values -- is in no sum; a row
 * with such a label still gets its L x G sums (query rows scored against the labelled ones).
 * gammas: a HOST array of L finite doubles > 0, read at call time (else DBMM_E_ARG).  L outside 1..4, G outside 1..16, N outside
 * 1..2^23: DBMM_E_SHAPE; D % 64 != 0 or D > 4096: DBMM_E_UNSUPPORTED; x, center and the workspace 16-byte aligned.  Four launches and
 * two memsets on `stream`.  The workspace is dbmm_workspace_bytes_pairdist_rows' with L times the partials: 16 x L x N x G float64
 * (0 for G outside 1..16 or L outside 1..4). */
size_t dbmm_workspace_bytes_pairdist_rbf_rows(int64_t N, int64_t D, int64_t G, int64_t L);
int dbmm_pairdist_rbf_row_group_sums(const float* x, const int64_t* groups, const float* center, const double* gammas, int64_t L,
                                     double* sums, int64_t N, int64_t D, int64_t G, void* workspace, size_t workspace_bytes,
                                     void* stream);

/* PCA of an embedding split: the scatter matrix without a centred copy of the rows (the deterministic map that stands in for the
 * UMAP / MDS projection of plot_umap, demo/visualizer.py:311-408; classical MDS of the distances dbmm_pairdist_group_sums reports):
 *   scatter double [D][D]: scatter[a][b] = sum_i (x[i][a] - center[a]) (x[i][b] - center[b]), about the GIVEN center exactly.
 * x fp32 [N][D] (contiguous), center fp32 [D]: any vector near the rows' mean -- it is subtracted on load; the caller removes
 * N (mean - center)(mean - center)^T in float64.  Exact fp32 products (v_mfma_f32_32x32x2_f32) over 64 x 64 tiles of the upper
 * triangle; no fp32 accumulation chain is longer than 1024 rows: every 1024 rows the tile is added to a float64 running tile.  A
 * workgroup owns one (tile, row range); the number of row ranges depends on (N, D) only, and a second launch adds the float64
 * partial tiles in range order and mirrors them: scatter is symmetric to the bit and two calls give the same bits.  Two launches on
 * `stream`, no memset, no floating-point atomics.
 * D % 64 != 0 or D > 4096: DBMM_E_UNSUPPORTED; N outside 1..2^23: DBMM_E_SHAPE; x, center and the workspace 16-byte aligned.  The
 * workspace holds the partial tiles only (32 KB per tile and row range, about 26 MB at D = 1024), never N x anything. */
size_t dbmm_workspace_bytes_covariance(int64_t N, int64_t D);
int dbmm_covariance(const float* x, const float* center, double* scatter, int64_t N, int64_t D, void* workspace,
                    size_t workspace_bytes, void* stream);

/* y fp32 [N][K] = (x - center) . basis^T: the coordinates of the rows in a fitted basis fp32 [K][D], K in 1..8 (else DBMM_E_SHAPE).
 * One read of x: a wave takes four rows at a time, float4 loads, one fp32 fmaf chain per (row, component) and a fixed shuffle tree,
 * so a row's coordinates do not depend on its neighbours or on N.  Shape and alignment rules of dbmm_covariance (basis too).  One
 * launch on `stream`. */
int dbmm_project_rows(const float* x, const float* center, const float* basis, float* y, int64_t N, int64_t D, int64_t K,
                      void* stream);

/* The top k eigenpairs of a symmetric positive semi-definite matrix C double [D][D] (symmetric to the bit, as dbmm_covariance writes
 * it) WITHOUT leaving the device: blocked subspace iteration on 16 vectors (k <= 8 plus oversampling) with a Rayleigh-Ritz step in
 * every iteration, all in float64.  One iteration, Q [D][16] orthonormal: Z = C Q; T = Q^T Z (symmetrised), G = Z^T Z; T = W theta W^T
 * by cyclic Jacobi in one workgroup (theta descending); Ritz vectors X = Q W, Y = Z W; residuals r_j = ||Y_j - theta_j X_j||_2 from
 * the vectors; converged when max_{j < k} r_j <= tol theta_1; else Q <- Y L^-T with L L^T = W^T G W.  The convergence factor per
 * iteration is lambda_17 / lambda_k: a k-th eigenvalue inside a flat bulk does not converge in any useful number of iterations.
 *   dbmm_sym_eig_begin    orthonormalises the start block q0 double [D][16] (Cholesky QR) into the workspace and resets the status.
 *                         One launch.
 *   dbmm_sym_eig_iterate  enqueues exactly n_iter iterations, three launches each (matvec and 16 x 16 partials per 16 rows; merge,
 *                         Jacobi, Cholesky in one workgroup; rotate per 16 rows), and one small launch that tests the last one's
 *                         residuals.  Every kernel reads the state first and does nothing unless it is `running`: iterations enqueued
 *                         after convergence are no-ops, and the result and the iteration count do not depend on how n_iter is cut
 *                         into calls.  Plain launches on `stream`; no memset, no floating-point atomics, partial sums in a fixed
 *                         order: two runs give the same bits.
 * Workspace, in doubles (Python reads views of it):
 *   [0]       iterations done
 *   [1]       state: 0 running, 1 converged, 2 breakdown (theta_1 not positive or not finite, Jacobi not converged after its cap of
 *             sweeps, a residual that is not finite, or -- after that iteration's residual test -- a Cholesky pivot that is not
 *             positive, not finite or below 2^-40 of the largest: a zero matrix, rank below 16)
 *   [2..17]   theta[16], descending, of the last completed Rayleigh-Ritz step
 *   [18..33]  r[16], the residual norms of the last tested iteration
 *   [34..63]  k, tol and internal words
 *   [64 ..]   the Ritz vectors VECTOR-MAJOR [16][D] (unit norm; the first k rows are the result), then Q, Z and the partials.
 * D % 64 != 0 or D > 4096: DBMM_E_UNSUPPORTED; k outside 1..8, n_iter < 0, tol not a positive finite number: DBMM_E_SHAPE; null
 * pointers, a short workspace and pointers that are not 16-byte aligned as dbmm_covariance answers them; every check precedes the
 * first launch.  dbmm_workspace_bytes_sym_eig: (64 + 81 D + 512) doubles, 0 for a D that is not served. */
size_t dbmm_workspace_bytes_sym_eig(int64_t D);
int dbmm_sym_eig_begin(const double* q0, int64_t D, int64_t k, double tol, void* workspace, size_t workspace_bytes, void* stream);
int dbmm_sym_eig_iterate(const double* C, int64_t D, int64_t n_iter, void* workspace, size_t workspace_bytes, void* stream);

/* Lloyd's k-means of the rows x fp32 [N][D] (contiguous) into K <= 16 clusters WITHOUT leaving the device: the label-free groups of
 * group DRO (Sohoni et al. 2020) and the question whether a representation separates the spurious attribute.  The reference has no
 * counterpart.  x is read twice per iteration; nothing N x D or N x K is allocated.
 *   dbmm_kmeans_begin    copies the start centres centers0 fp32 [K][D] into the workspace, sets every label to -1 and clears the status.
 *                        One launch.
 *   dbmm_kmeans_iterate  enqueues exactly n_iter iterations, three launches each:
 *                          assign  label[i] = argmin_j d2_ij (the lowest j on an exact tie), dmin[i] = min_j d2_ij, with
 *                                  d2_ij = sum_d (x_id - c_jd)^2 formed FROM THE DIFFERENCES in fp32 (one fmaf chain per (row, centre) in
 *                                  column order, a fixed shuffle tree): a row's result depends on that row and the centres only.  The
 *                                  rows whose label changed are counted with an integer atomic.
 *                          sums    per-cluster column sums per (one of P row ranges, 256 columns), rows in order, in float64 from the
 *                                  first add (there is no fp32 chain); P depends on (N, D) only.  Also the ranges' row counts and
 *                                  float64 sums of dmin.
 *                          merge   the partials added in a fixed order (range order within each quarter of the ranges, then the
 *                                  quarters in order); c_j <- fp32(sum_j / n_j) in float64; a cluster without rows
 *                                  keeps its centre (count 0).  When the assignment changed no label the state becomes `converged`
 *                                  instead and the centres stay the ones that labels, dmin and inertia were computed against.
 *                        Every kernel reads the state first and does nothing unless it is `running`: iterations enqueued after
 *                        convergence are no-ops, and the result and the iteration count do not depend on how n_iter is cut into calls.
 *                        Plain launches on `stream`; no memset, no floating-point atomics: two runs give the same bits.
 *   dbmm_kmeans_assign   the assignment alone against given centres fp32 [K][D], into labels int32 [N] and dmin fp32 [N]: one launch,
 *                        no workspace.  Places other rows (val, test) at fitted centres, so N may be below K here (N >= 1).  A slice
 *                        of the rows gets the bits of the slice of the whole assignment.
 * Workspace, in bytes (Python reads views of it); every part starts 16-byte aligned:
 *   [0, 256)    the status, 8-byte words: [0] int64 iterations done; [1] int64 state: 0 running, 1 converged; [2] int64 rows whose
 *               label changed in the last assignment; [3] double inertia = sum_i dmin[i] of the last assignment; [4..19] int64
 *               counts[16], the clusters' rows in the last assignment; [20..31] internal words
 *   [256, ..)   centres fp32 [K][D]
 *   then        labels int32 [N], padded to 16 bytes; dmin fp32 [N], padded to 16 bytes
 *   then        the partials: float64 [P][K][D] sums, int64 [P][16] counts, float64 [P] sums of dmin
 * with P = min(ceil(2048 / ceil(D / 256)), ceil(N / 64)), at least 1.
 * K < 1, N < K, D <= 0, D % 4 != 0, n_iter < 0: DBMM_E_SHAPE; K > 16 (that wants an MFMA tile kernel), D > 4096 or N >= 2^31:
 * DBMM_E_UNSUPPORTED; then null pointers: DBMM_E_ARG; a short workspace: DBMM_E_WORKSPACE; x, the centres or the workspace not
 * 16-byte aligned (labels, dmin of dbmm_kmeans_assign: 4-byte): DBMM_E_ALIGN.  Every check precedes the first launch.
 * dbmm_workspace_bytes_kmeans is 0 for a shape that is not served. */
size_t dbmm_workspace_bytes_kmeans(int64_t N, int64_t D, int64_t K);
int dbmm_kmeans_begin(const float* centers0, int64_t N, int64_t D, int64_t K, void* workspace, size_t workspace_bytes, void* stream);
int dbmm_kmeans_iterate(const float* x, int64_t N, int64_t D, int64_t K, int64_t n_iter, void* workspace, size_t workspace_bytes,
                        void* stream);
int dbmm_kmeans_assign(const float* x, const float* centers, int32_t* labels, float* dmin, int64_t N, int64_t D, int64_t K,
                       void* stream);

/* Linear concept erasure of the rows x fp32 [N][D] (contiguous): the moment that PCA's two (column sums, scatter) lack, and the
 * application of a fitted eraser.  The reference has no counterpart.
 *   dbmm_label_colsums  sums double [G][D]: sums[g][d] = sum over i with labels[i] == g of x[i][d], the RAW sums, and counts int64
 *                       [G], from ONE read of x.  labels int64 [N], compared as 64 bits: a value outside [0, G) (-1, G, 2^32 + 1) is
 *                       in no sum and no count.  Per (one of P row ranges, 256 columns) the rows are added in row order in float64
 *                       from the first add (there is no fp32 chain); the partials are added in a fixed order (range order within
 *                       each quarter of the ranges, then the quarters in order).  P = min(ceil(2048 / ceil(D / 256)), ceil(N / 64))
 *                       depends on (N, D) only.  Two launches on `stream`, no memset, no floating-point atomics: two calls give
 *                       the same bits.  The workspace holds the partials: float64 [P][G][D], then int64 [P][16].
 *   dbmm_erase_rows     y[i][d] = x[i][d] - sum_k ((x[i] - center) . A[k]) B[k][d] for A, B fp32 [R][D], R in 1..15, in one read and
 *                       one write of the rows; y may be x (a row is read completely before any of it is written) and must otherwise
 *                       not overlap it.  A wave takes 4 / 2 / 1 rows (D <= 1024 / <= 2048 / above) and keeps them in registers:
 *                       (x - center) in fp32, one fp32 fmaf chain per (row, k) over the lane's columns in column order, a fixed
 *                       shuffle tree, t = sum_k s_k B[k][d] as one fmaf chain in k order, y = x - t.  A row's result depends on that
 *                       row only: erasing a slice gives the bits of the slice.  One launch on `stream`, no workspace.
 * Both: D % 64 != 0 or D > 4096: DBMM_E_UNSUPPORTED; N outside 1..2^23, G outside 1..16, R outside 1..15: DBMM_E_SHAPE; then null
 * pointers: DBMM_E_ARG; a short workspace: DBMM_E_WORKSPACE; x, center, A, B, y or the workspace not 16-byte aligned (labels,
 * sums, counts: 8-byte): DBMM_E_ALIGN.  Every check precedes the first launch.  dbmm_workspace_bytes_label_colsums is 0 for a
 * shape that is not served. */
size_t dbmm_workspace_bytes_label_colsums(int64_t N, int64_t D, int64_t G);
int dbmm_label_colsums(const float* x, const int64_t* labels, double* sums, int64_t* counts, int64_t N, int64_t D, int64_t G,
                       void* workspace, size_t workspace_bytes, void* stream);
int dbmm_erase_rows(const float* x, const float* center, const float* A, const float* B, float* y, int64_t N, int64_t D, int64_t R,
                    void* stream);

/* L1-penalised logistic probes by FISTA, `iters` iterations in ONE launch (csrc/linear_prox.hip): replica r of R <= 256 is one
 * workgroup that keeps its iterate in LDS and minimises
 *     F(W, b) = (1 / n) sum_i CE(softmax(W x_i + b), y_i) + lam[r] ||W||_1        (the intercept b is not penalised)
 * over the rows idx[r][0 .. n) of a shared table fp32 [n_rows][D] (clamped into it; labels int64 [n_rows], read as labels[idx],
 * compared as 64 bits: a label outside [0, C) scores NaN).  The reference has no counterpart.  One iteration, from the state
 * (W, b, V, c, t):  G, g = gradient of the CE mean at (V, c);  W' = soft(V - step[r] G, step[r] lam[r]) with soft(z, tau) =
 * sign(z) max(|z| - tau, 0) (an exact +0 inside the threshold);  b' = c - step[r] g;  t' = (1 + sqrt(1 + 4 t^2)) / 2 in float64;
 * beta = (float)((t - 1) / t'), or 0 when accelerate == 0 (plain ISTA);  V' = W' + beta (W' - W), c' = b' + beta (b' - b).
 *   lam, step  fp32 [R], on the device (step = 1 / L, L = half the largest eigenvalue of (1 / n) [X, 1]^T [X, 1]: the caller's)
 *   w, v       fp32 [R][C][D];  b, c fp32 [R][C];  t float64 [R]: the state, updated in place.  A fresh fit starts from w = v,
 *              b = c, t = 1.  Nothing else is carried between iterations, so K iterations in one call are the K iterations of
 *              several calls, bit for bit.
 *   stats      fp32 [R][4], written by the call's last iteration: max |W' - W|, max |W'|, the number of nonzeros of W', and the CE
 *              mean at that iteration's (V, c).
 * Every sum has a fixed order that depends on (n, D, C) only: two calls give the same bits, and a replica's bits depend neither on R
 * nor on its place among the replicas.  One launch on `stream`, no workspace, no atomics.
 * Null pointer: DBMM_E_ARG; R outside 1..256, n < 1, C outside 1..8, D % 4 != 0, D outside 4..1024, n_rows < 1, iters outside
 * 1..2^20: DBMM_E_SHAPE; table, w, v or stats not 16-byte aligned (idx, labels, t: 8-byte): DBMM_E_ALIGN.  Every check precedes
 * the launch. */
int dbmm_linear_prox_fit(const float* table, int64_t n_rows, const int64_t* idx, const int64_t* labels, const float* lam,
                         const float* step, float* w, float* b, float* v, float* c, double* t, float* stats, int64_t R, int64_t n,
                         int64_t D, int64_t C, int64_t iters, int accelerate, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DBMM_H */
