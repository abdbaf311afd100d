"""The no-launch operand audit shared by tests/test_ops_validation.py (stub library, no GPU) and its one GPU test (real library).

The C ABI (include/dbmm.h) takes raw pointers, sizes and leading dimensions.  It can refuse bad dimensions; it cannot see whether a
pointer holds as many elements, of the dtype, on the device, that those dimensions imply.  That is the Python wrappers' job, and this
module checks that they do it, without launching anything:

  * `Stub` stands in for the loaded library (`_lib.lib`): it answers the option and `*_bytes` queries and records every other call;
  * `Registry` knows every tensor the wrappers allocate (through `ops._empty` / `preprocess._empty`) and every tensor of the call;
  * `SPEC` says, for each C entry and each pointer argument, which dtype the entry reads there and how many elements it indexes, as
    an expression of the call's integer arguments (written from include/dbmm.h; the pointer positions come from `_lib._SIGS`);
  * `audit` resolves each recorded pointer to a registered tensor and compares;
  * `CASES` is the matrix of valid calls, at the smallest shapes that reach each entry, and `mutations` derives the bad calls from it.
"""
import os
import re

import torch

from dbmm_amd import _lib, ops, preprocess

F32, F16, BF16, I32, I64, U8 = torch.float32, torch.float16, torch.bfloat16, torch.int32, torch.int64, torch.uint8
WS_BYTES = 4096                     # what the stub answers to every *_bytes query

# ---- the spec table ---------------------------------------------------------------------------------------------------------------
# entry -> (argument names in the header's order, derived integers, {pointer argument: cell})
# cell = (dtype, element count[, "null"]): dtype a torch dtype or an expression of the integer arguments; "null": NULL is allowed.
# `stream` is exempt, `workspace` is checked against `workspace_bytes`, HOST marks a host pointer (the three-float mean / std arrays).
HOST = "host"
_X16 = "F16 if x_is_f16 else F32"
_CONV = "Ho = (H + 2 * pad - KH) // stride + 1; Wo = (W + 2 * pad - KW) // stride + 1"
_GEMM_A = "(K - 1) * lda + M if trans_a else (M - 1) * lda + K"
_GEMM_W = "(K - 1) * ldw + N if trans_w else (N - 1) * ldw + K"
_PRE = {"h_bounds": (I32, "2 * R"), "h_coeffs": (I32, "R * h_ksize"), "v_bounds": (I32, "2 * R"), "v_coeffs": (I32, "R * v_ksize"),
        "mean3": HOST, "std3": HOST}

SPEC = {
    "dbmm_split_weight_planes": ("w planes N K stream", "", {"w": (F32, "N * K"), "planes": (BF16, "3 * N * K")}),
    "dbmm_split_weight_planes_f16": ("w planes N K w_exp stream", "", {"w": (F32, "N * K"), "planes": (F16, "2 * N * K")}),
    "dbmm_gemm_bias_act_ws": (
        "a lda trans_a w ldw trans_w bias residual ldr c ldc M N K alpha act workspace workspace_bytes stream", "",
        {"a": (F32, _GEMM_A), "w": (F32, _GEMM_W), "bias": (F32, "N", "null"), "residual": (F32, "(M - 1) * ldr + N", "null"),
         "c": (F32, "(M - 1) * ldc + N")}),
    "dbmm_gemm_bias_act_x3": (
        "a lda w w_planes ldw bias residual ldr c ldc M N K alpha act workspace workspace_bytes stream", "",
        {"a": (F32, "(M - 1) * lda + K"), "w": (F32, "(N - 1) * ldw + K"), "w_planes": (BF16, "3 * N * K"), "bias": (F32, "N", "null"),
         "residual": (F32, "(M - 1) * ldr + N", "null"), "c": (F32, "(M - 1) * ldc + N")}),
    "dbmm_gemm_bias_act_x2": (
        "a lda a_absmax w w_planes_f16 w_planes w_exp ldw out_scale bias residual ldr c ldc c_absmax M N K alpha act workspace "
        "workspace_bytes stream", "",
        {"a": (F32, "(M - 1) * lda + K"), "a_absmax": (F32, "1", "null"), "w": (F32, "(N - 1) * ldw + K"),
         "w_planes_f16": (F16, "w_planes * N * K", "null"), "out_scale": (F32, "N", "null"), "bias": (F32, "N", "null"),
         "residual": (F32, "(M - 1) * ldr + N", "null"), "c": (F32, "(M - 1) * ldc + N"), "c_absmax": (F32, "1", "null")}),
    "dbmm_conv_bn_act_ws": (
        "x w bias residual y B H W Cin Cout KH KW stride pad act w_layout workspace workspace_bytes stream", _CONV,
        {"x": (F32, "B * H * W * Cin"), "w": (F32, "Cout * KH * KW * Cin"), "bias": (F32, "Cout", "null"),
         "residual": (F32, "B * Ho * Wo * Cout", "null"), "y": (F32, "B * Ho * Wo * Cout")}),
    "dbmm_conv_bn_act_x3": (
        "x w w_planes bias residual y B H W Cin Cout KH KW stride pad act w_layout workspace workspace_bytes stream", _CONV,
        {"x": (F32, "B * H * W * Cin"), "w": (F32, "Cout * KH * KW * Cin"), "w_planes": (BF16, "3 * Cout * KH * KW * Cin"),
         "bias": (F32, "Cout", "null"), "residual": (F32, "B * Ho * Wo * Cout", "null"), "y": (F32, "B * Ho * Wo * Cout")}),
    "dbmm_conv_bn_act_x2": (
        "x x_absmax w w_planes_f16 w_planes w_exp out_scale bias residual y y_full y_absmax B H W Cin Cout KH KW stride pad act pool "
        "w_layout workspace workspace_bytes stream", _CONV,
        {"x": (F32, "B * H * W * Cin"), "x_absmax": (F32, "1", "null"), "w": (F32, "Cout * KH * KW * Cin"),
         "w_planes_f16": (F16, "w_planes * Cout * KH * KW * Cin", "null"), "out_scale": (F32, "Cout", "null"),
         "bias": (F32, "Cout", "null"), "residual": (F32, "B * Ho * Wo * Cout", "null"),
         "y": (F32, "B * (Ho // 2) * (Wo // 2) * Cout if pool == 2 else B * Ho * Wo * Cout"),
         "y_full": (F32, "B * Ho * Wo * Cout", "null"), "y_absmax": (F32, "1", "null")}),
    "dbmm_gemm_dual_bn_act_x2": (
        "a lda a_absmax w_plane_f16 w_exp ldw K out_scale a2 lda2 a2_absmax w2_plane_f16 ldw2 K2 ratio bias c ldc c_absmax M N act "
        "workspace workspace_bytes stream", "",
        {"a": (F32, "(M - 1) * lda + K"), "a_absmax": (F32, "1"), "w_plane_f16": (F16, "(N - 1) * ldw + K"), "out_scale": (F32, "N"),
         "a2": (F32, "(M - 1) * lda2 + K2"), "a2_absmax": (F32, "1"), "w2_plane_f16": (F16, "(N - 1) * ldw2 + K2"), "ratio": (F32, "N"),
         "bias": (F32, "N"), "c": (F32, "(M - 1) * ldc + N"), "c_absmax": (F32, "1", "null")}),
    "dbmm_conv3x3_c32_bn_relu_x2": (
        "x x_absmax w_plane_f16 w_exp scale bias y y_absmax B H W Cin Cout pool stream", "",
        {"x": (F32, "B * H * W * Cin"), "x_absmax": (F32, "1"), "w_plane_f16": (F16, "Cout * 9 * Cin"), "scale": (F32, "Cout"),
         "bias": (F32, "Cout"), "y": (F32, "B * (H // 2) * (W // 2) * Cout if pool == 2 else B * H * W * Cout"),
         "y_absmax": (F32, "1", "null")}),
    "dbmm_bottleneck_chain_x2": (
        "y2 y2_absmax w3_plane_f16 w3_exp scale3 bias3 residual x_out x_pooled x_absmax w1_plane_f16 w1_exp scale1 bias1 y1_out "
        "y1_absmax B Ho Wo K N P stream", "M = B * Ho * Wo",
        {"y2": (F32, "M * K"), "y2_absmax": (F32, "1"), "w3_plane_f16": (F16, "N * K"), "scale3": (F32, "N"), "bias3": (F32, "N"),
         "residual": (F32, "M * N"), "x_out": (F32, "M * N", "null"), "x_pooled": (F32, "B * (Ho // 2) * (Wo // 2) * N", "null"),
         "x_absmax": (F32, "1", "null"), "w1_plane_f16": (F16, "P * N"), "scale1": (F32, "P"), "bias1": (F32, "P"),
         "y1_out": (F32, "M * P"), "y1_absmax": (F32, "1", "null")}),
    "dbmm_bottleneck_chain_dual_x2": (
        "y2 y2_absmax w3_plane_f16 w3_exp scale3 bias a2 a2_absmax wd_plane_f16 ratio x_out x_absmax w1_plane_f16 w1_exp scale1 bias1 "
        "y1_out y1_absmax M K K2 N P stream", "",
        {"y2": (F32, "M * K"), "y2_absmax": (F32, "1"), "w3_plane_f16": (F16, "N * K"), "scale3": (F32, "N"), "bias": (F32, "N"),
         "a2": (F32, "M * K2"), "a2_absmax": (F32, "1"), "wd_plane_f16": (F16, "N * K2"), "ratio": (F32, "N"), "x_out": (F32, "M * N"),
         "x_absmax": (F32, "1", "null"), "w1_plane_f16": (F16, "P * N"), "scale1": (F32, "P"), "bias1": (F32, "P"),
         "y1_out": (F32, "M * P"), "y1_absmax": (F32, "1", "null")}),
    "dbmm_bottleneck_block_chain_x2": (
        "y1 y1_absmax w2_plane_f16 w2_exp scale2 bias2 w3_plane_f16 w3_exp scale3 bias3 residual a2 a2_absmax wd_plane_f16 ratio x_out "
        "x_absmax w1_plane_f16 w1_exp scale1 bias1 y1_out y1_out_absmax B H W K N P stream", "M = B * H * W",
        {"y1": (F32, "M * K"), "y1_absmax": (F32, "1"), "w2_plane_f16": (F16, "K * 9 * K"), "scale2": (F32, "K"), "bias2": (F32, "K"),
         "w3_plane_f16": (F16, "N * K"), "scale3": (F32, "N"), "bias3": (F32, "N"), "residual": (F32, "M * N", "null"),
         "a2": (F32, "M * 64", "null"), "a2_absmax": (F32, "1", "null"), "wd_plane_f16": (F16, "N * 64", "null"),
         "ratio": (F32, "N", "null"), "x_out": (F32, "M * N"), "x_absmax": (F32, "1", "null"), "w1_plane_f16": (F16, "P * N"),
         "scale1": (F32, "P"), "bias1": (F32, "P"), "y1_out": (F32, "M * P"), "y1_out_absmax": (F32, "1", "null")}),
    "dbmm_conv_stem_s2": (
        "x_nchw w bias y_nhwc y_absmax B H W Cout stream", "",
        {"x_nchw": (F32, "B * 3 * H * W"), "w": (F32, "27 * Cout"), "bias": (F32, "Cout"),
         "y_nhwc": (F32, "B * ((H - 1) // 2 + 1) * ((W - 1) // 2 + 1) * Cout"), "y_absmax": (F32, "1", "null")}),
    "dbmm_avgpool2d": ("x y B H W C k stream", "", {"x": (F32, "B * H * W * C"), "y": (F32, "B * (H // k) * (W // k) * C")}),
    "dbmm_attnpool_x": (
        "x x_is_f16 pos wq bq wkv bkv wc bc out B HW C heads Dout workspace workspace_bytes stream", "",
        {"x": (_X16, "B * HW * C"), "pos": (F32, "(HW + 1) * C"), "wq": (F32, "C * C"), "bq": (F32, "C"), "wkv": (F32, "2 * C * C"),
         "bkv": (F32, "2 * C"), "wc": (F32, "Dout * C"), "bc": (F32, "Dout"), "out": (F32, "B * Dout")}),
    "dbmm_layernorm": (
        "x ldx gamma beta y ldy rows E eps y_absmax stream", "",
        {"x": (F32, "(rows - 1) * ldx + E"), "gamma": (F32, "E"), "beta": (F32, "E"), "y": (F32, "(rows - 1) * ldy + E"),
         "y_absmax": (F32, "1", "null")}),
    "dbmm_mha_core": ("qkv out B L E heads causal stream", "", {"qkv": (F32, "B * L * 3 * E"), "out": (F32, "B * L * E")}),
    "dbmm_mha_core_x2": ("qkv qkv_absmax out B L E heads causal stream", "",
                         {"qkv": (F32, "B * L * 3 * E"), "qkv_absmax": (F32, "1"), "out": (F32, "B * L * E")}),
    "dbmm_embed_gather": ("tokens table pos out n L W vocab stream", "",
                          {"tokens": (I32, "n * L"), "table": (F32, "vocab * W"), "pos": (F32, "L * W"), "out": (F32, "n * L * W")}),
    "dbmm_im2col_patch": ("x_nchw out out_absmax B R P stream", "",
                          {"x_nchw": (F32, "B * 3 * R * R"), "out": (F32, "B * (R // P) ** 2 * 3 * P * P"),
                           "out_absmax": (F32, "1", "null")}),
    "dbmm_vit_tokens": ("patches cls pos out B L W stream", "",
                        {"patches": (F32, "B * (L - 1) * W"), "cls": (F32, "W"), "pos": (F32, "L * W"), "out": (F32, "B * L * W")}),
    "dbmm_gather_eot": ("tokens x out n L W stream", "", {"tokens": (I32, "n * L"), "x": (F32, "n * L * W"), "out": (F32, "n * W")}),
    "dbmm_text_colnorm": ("text tn D C stream", "", {"text": (F32, "D * C"), "tn": (F32, "C * D")}),
    "dbmm_l2norm_rows": ("x y B D stream", "", {"x": (F32, "B * D"), "y": (F32, "B * D")}),
    "dbmm_colsum": ("x out B N stream", "", {"x": (F32, "B * N"), "out": (F32, "N")}),
    # fp16 mode
    "dbmm_gemm_f16_ws": (
        "a lda w ldw bias residual ldr c ldc M N K act workspace workspace_bytes stream", "",
        {"a": (F16, "(M - 1) * lda + K"), "w": (F16, "(N - 1) * ldw + K"), "bias": (F32, "N", "null"),
         "residual": (F16, "(M - 1) * ldr + N", "null"), "c": (F16, "(M - 1) * ldc + N")}),
    "dbmm_mha_core_f16": ("qkv out B L E heads causal stream", "", {"qkv": (F16, "B * L * 3 * E"), "out": (F16, "B * L * E")}),
    "dbmm_layernorm_f16": ("x ldx gamma beta y ldy rows E eps stream", "",
                           {"x": (F16, "(rows - 1) * ldx + E"), "gamma": (F32, "E"), "beta": (F32, "E"),
                            "y": (F16, "(rows - 1) * ldy + E")}),
    "dbmm_im2col_patch_f16": ("x_nchw x_is_f16 out B R P Kp stream", "",
                              {"x_nchw": (_X16, "B * 3 * R * R"), "out": (F16, "B * (R // P) ** 2 * Kp")}),
    "dbmm_vit_tokens_f16": ("patches cls pos out B L W stream", "",
                            {"patches": (F16, "B * (L - 1) * W"), "cls": (F32, "W"), "pos": (F32, "L * W"), "out": (F16, "B * L * W")}),
    "dbmm_embed_gather_f16": ("tokens table pos out n L W vocab stream", "",
                              {"tokens": (I32, "n * L"), "table": (F32, "vocab * W"), "pos": (F32, "L * W"),
                               "out": (F16, "n * L * W")}),
    "dbmm_gather_eot_f16": ("tokens x out n L W stream", "",
                            {"tokens": (I32, "n * L"), "x": (F16, "n * L * W"), "out": (F16, "n * W")}),
    "dbmm_conv1x1_bn_act_f16_ws": (
        "x w scale bias residual y M Cin Cout act workspace workspace_bytes stream", "",
        {"x": (F16, "M * Cin"), "w": (F16, "Cout * Cin"), "scale": (F32, "Cout"), "bias": (F32, "Cout"),
         "residual": (F16, "M * Cout", "null"), "y": (F16, "M * Cout")}),
    "dbmm_conv1x1_dual_bn_act_f16": (
        "y2 w3 scale3 xp wd ratio bias out M K K2 Cout act stream", "",
        {"y2": (F16, "M * K"), "w3": (F16, "Cout * K"), "scale3": (F32, "Cout"), "xp": (F16, "M * K2"), "wd": (F16, "Cout * K2"),
         "ratio": (F32, "Cout"), "bias": (F32, "Cout"), "out": (F16, "M * Cout")}),
    "dbmm_bottleneck_chain_f16": (
        "y2 w3 scale3 bias3 residual x_out w1 scale1 bias1 y1_out M K N P stream", "",
        {"y2": (F16, "M * K"), "w3": (F16, "N * K"), "scale3": (F32, "N"), "bias3": (F32, "N"), "residual": (F16, "M * N"),
         "x_out": (F16, "M * N"), "w1": (F16, "P * N"), "scale1": (F32, "P"), "bias1": (F32, "P"), "y1_out": (F16, "M * P")}),
    "dbmm_bottleneck_chain_pool_f16": (
        "y2 w3 scale3 bias3 residual x_out x_pooled w1 scale1 bias1 y1_out B Ho Wo K N P stream", "M = B * Ho * Wo",
        {"y2": (F16, "M * K"), "w3": (F16, "N * K"), "scale3": (F32, "N"), "bias3": (F32, "N"), "residual": (F16, "M * N"),
         "x_out": (F16, "M * N", "null"), "x_pooled": (F16, "B * (Ho // 2) * (Wo // 2) * N"), "w1": (F16, "P * N"), "scale1": (F32, "P"),
         "bias1": (F32, "P"), "y1_out": (F16, "M * P")}),
    "dbmm_bottleneck_chain_dual_f16": (
        "y2 w3 scale3 xp wd ratio bias x_out w1 scale1 bias1 y1_out M K K2 N P stream", "",
        {"y2": (F16, "M * K"), "w3": (F16, "N * K"), "scale3": (F32, "N"), "xp": (F16, "M * K2"), "wd": (F16, "N * K2"),
         "ratio": (F32, "N"), "bias": (F32, "N"), "x_out": (F16, "M * N"), "w1": (F16, "P * N"), "scale1": (F32, "P"),
         "bias1": (F32, "P"), "y1_out": (F16, "M * P")}),
    "dbmm_conv3x3_bn_relu_f16": (
        "x w scale bias y B H W Cin Cout pool stream", "",
        {"x": (F16, "B * H * W * Cin"), "w": (F16, "Cout * 9 * Cin"), "scale": (F32, "Cout"), "bias": (F32, "Cout"),
         "y": (F16, "B * (H // 2) * (W // 2) * Cout if pool == 2 else B * H * W * Cout")}),
    "dbmm_conv_stem_s2_f16": (
        "x_nchw x_is_f16 w bias y_nhwc B H W Cout stream", "",
        {"x_nchw": (_X16, "B * 3 * H * W"), "w": (F32, "27 * Cout"), "bias": (F32, "Cout"),
         "y_nhwc": (F16, "B * ((H - 1) // 2 + 1) * ((W - 1) // 2 + 1) * Cout")}),
    "dbmm_conv_stem_s2_bn_f16": (
        "x_nchw x_is_f16 w scale bias y_nhwc B H W Cout stream", "",
        {"x_nchw": (_X16, "B * 3 * H * W"), "w": (F32, "27 * Cout"), "scale": (F32, "Cout"), "bias": (F32, "Cout"),
         "y_nhwc": (F16, "B * ((H - 1) // 2 + 1) * ((W - 1) // 2 + 1) * Cout")}),
    "dbmm_conv1x1_res_pool_f16": (
        "x w scale bias residual y y_pooled B Ho Wo Cin Cout stream", "M = B * Ho * Wo",
        {"x": (F16, "M * Cin"), "w": (F16, "Cout * Cin"), "scale": (F32, "Cout"), "bias": (F32, "Cout"), "residual": (F16, "M * Cout"),
         "y": (F16, "M * Cout"), "y_pooled": (F16, "B * (Ho // 2) * (Wo // 2) * Cout")}),
    "dbmm_avgpool2_f16": ("x y B H W C stream", "", {"x": (F16, "B * H * W * C"), "y": (F16, "B * (H // 2) * (W // 2) * C")}),
    # preprocessing
    "dbmm_resize_crop_normalize_u8": (
        "img_hwc H W h_bounds h_coeffs h_ksize v_bounds v_coeffs v_ksize row0 nrows R mean3 std3 out_chw out_u8_hwc workspace "
        "workspace_bytes stream", "",
        dict(_PRE, img_hwc=(U8, "H * W * 3"), out_chw=(F32, "3 * R * R"), out_u8_hwc=(U8, "R * R * 3", "null"))),
    "dbmm_resize_crop_normalize_u8_batch": (
        "img_bhwc B H W h_bounds h_coeffs h_ksize v_bounds v_coeffs v_ksize row0 nrows R mean3 std3 out_chw out_u8_hwc workspace "
        "workspace_bytes stream", "",
        dict(_PRE, img_bhwc=(U8, "B * H * W * 3"), out_chw=(F32, "B * 3 * R * R"), out_u8_hwc=(U8, "B * R * R * 3", "null"))),
}
AUDITED = frozenset(SPEC)

# The four sets below are literal names, so that a new export can join none of them unnoticed (test_every_export_is_audited_...).
# entries that launch nothing
LAUNCHLESS = frozenset({
    "dbmm_debug_last_igemm", "dbmm_error_string", "dbmm_get_option", "dbmm_set_option", "dbmm_split_planes_bytes",
    "dbmm_split_planes_f16_bytes", "dbmm_supcon_sets_workspace_bytes", "dbmm_supcon_workspace_bytes", "dbmm_version",
    "dbmm_workspace_bytes_adapter_bwd", "dbmm_workspace_bytes_adapter_sweep_eval", "dbmm_workspace_bytes_adapter_sweep_step",
    "dbmm_workspace_bytes_adapter_train_step", "dbmm_workspace_bytes_adapter_train_step_sets", "dbmm_workspace_bytes_attnpool",
    "dbmm_workspace_bytes_covariance", "dbmm_workspace_bytes_igemm", "dbmm_workspace_bytes_kmeans",
    "dbmm_workspace_bytes_label_colsums", "dbmm_workspace_bytes_linear_ce_fwd", "dbmm_workspace_bytes_linear_sweep_eval",
    "dbmm_workspace_bytes_linear_sweep_step", "dbmm_workspace_bytes_linear_train_step", "dbmm_workspace_bytes_pairdist",
    "dbmm_workspace_bytes_pairdist_rbf", "dbmm_workspace_bytes_pairdist_rbf_rows", "dbmm_workspace_bytes_pairdist_rows",
    "dbmm_workspace_bytes_preprocess", "dbmm_workspace_bytes_sym_eig"})

# exported for C callers and the kernel tests, reached by no wrapper of the package (test_ops_validation checks that): the Python
# boundary this audit is about does not exist for them
NO_WRAPPER = frozenset({
    "dbmm_attnpool", "dbmm_bn1d_relu", "dbmm_bn1d_stats", "dbmm_cast_f32_f16", "dbmm_conv1x1_bn_act", "dbmm_conv1x1_bn_act_f16",
    "dbmm_conv3x3_bn_act", "dbmm_conv_bn_act", "dbmm_gemm_batched", "dbmm_gemm_bias_act", "dbmm_gemm_f16", "dbmm_gemm_pair_8ph"})

# the training and analysis entries: their wrappers use ops._operand and have refusal tests in their own host suites.  Every name
# belongs to one of the families below (checked); dbmm_weighted_mean, the row-weighted mean beside dbmm_l2norm_sim_ce_bwd_rows,
# is the one entry outside the families the audit was first scoped by
NOT_AUDITED_FAMILIES = ("dbmm_l2norm_sim_ce_", "dbmm_supcon", "dbmm_adapter_", "dbmm_linear_", "dbmm_sgd_momentum", "dbmm_group_",
                        "dbmm_weighted_mean", "dbmm_pairdist_", "dbmm_covariance", "dbmm_project_rows", "dbmm_sym_eig_", "dbmm_kmeans_",
                        "dbmm_label_colsums", "dbmm_erase_rows", "dbmm_gather_rows")
NOT_AUDITED_YET = frozenset({
    "dbmm_adapter_bwd", "dbmm_adapter_fwd", "dbmm_adapter_sweep_eval", "dbmm_adapter_sweep_step",
    "dbmm_adapter_sweep_step_gdro", "dbmm_adapter_sweep_step_weighted", "dbmm_adapter_train_step",
    "dbmm_adapter_train_step_gdro", "dbmm_adapter_train_step_sets", "dbmm_adapter_train_step_supcon",
    "dbmm_adapter_train_step_weighted", "dbmm_covariance", "dbmm_erase_rows", "dbmm_gather_rows", "dbmm_group_count",
    "dbmm_group_dro_weights", "dbmm_group_loss_sum", "dbmm_kmeans_assign", "dbmm_kmeans_begin", "dbmm_kmeans_iterate",
    "dbmm_l2norm_sim_ce_bwd", "dbmm_l2norm_sim_ce_bwd_rows", "dbmm_l2norm_sim_ce_bwd_weighted", "dbmm_l2norm_sim_ce_fwd",
    "dbmm_label_colsums", "dbmm_linear_ce_fwd", "dbmm_linear_prox_fit", "dbmm_linear_sweep_eval", "dbmm_linear_sweep_step",
    "dbmm_linear_sweep_step_weighted", "dbmm_linear_train_step", "dbmm_linear_train_step_weighted", "dbmm_pairdist_group_sums",
    "dbmm_pairdist_rbf_group_sums", "dbmm_pairdist_rbf_row_group_sums", "dbmm_pairdist_row_group_sums", "dbmm_project_rows",
    "dbmm_sgd_momentum", "dbmm_supcon_bwd", "dbmm_supcon_fwd", "dbmm_supcon_sets_bwd", "dbmm_supcon_sets_fwd",
    "dbmm_sym_eig_begin", "dbmm_sym_eig_iterate", "dbmm_weighted_mean"})


def arg_names(entry):
    return SPEC[entry][0].split()


def pointer_positions(entry):
    """positions of the pointer arguments, from the ctypes signature the package binds"""
    return [i for i, t in enumerate(_lib._SIGS[entry]) if t is _lib._P]


# ---- registry, stub, audit --------------------------------------------------------------------------------------------------------

class Registry:
    """every tensor the audit may meet, by address range: what the wrappers allocate and the operands of the call under test"""

    def __init__(self):
        self.tensors = []

    def add(self, t):
        if isinstance(t, torch.Tensor) and t.device.type != "meta":
            self.tensors.append(t)
        return t

    def add_tree(self, tree):
        for _, t in leaves(tree):
            self.add(t)

    def empty(self, *size, **kw):
        """stand-in for ops._empty / preprocess._empty"""
        return self.add(torch.zeros(*size, **kw))

    def find(self, address):
        """the registered tensor that starts at `address`, else the smallest one that contains it"""
        best = None
        for t in self.tensors:
            start = t.data_ptr()
            end = start + max(t.numel(), 1 if t.numel() else 0) * t.element_size()
            if t.numel() and start == address:
                return t
            if start <= address < end and (best is None or t.numel() < best.numel()):
                best = t
        return best


class Stub:
    """stand-in for the loaded library: options and *_bytes queries are answered, every other entry is recorded and answers 0 (or
    DBMM_E_UNSUPPORTED where `unsupported(entry, named arguments)` says so)"""

    def __init__(self, unsupported=None):
        src = open(os.path.join(_lib.CSRC, "options.hip")).read()
        self.options = {m.group(1): int(m.group(2)) for m in re.finditer(r'\{"(\w+)",\s*(-?\d+)\}', src)}
        self.calls = []
        self.unsupported = unsupported

    def __getattr__(self, name):
        if name not in _lib._SIGS:
            raise AttributeError(name)

        def entry(*args):
            assert len(args) == len(_lib._SIGS[name]), f"{name}: {len(args)} arguments for a signature of {len(_lib._SIGS[name])}"
            if name == "dbmm_get_option":
                args[1]._obj.value = self.options[args[0].decode()]
                return 0
            if name == "dbmm_set_option":
                self.options[args[0].decode()] = int(args[1])
                return 0
            if name == "dbmm_version":
                return 100
            if name == "dbmm_error_string":
                return b"stub"
            if name == "dbmm_debug_last_igemm":
                return None
            if "_bytes" in name:
                return WS_BYTES
            self.calls.append((name, args))
            if self.unsupported is not None and name in SPEC and self.unsupported(name, dict(zip(arg_names(name), args))):
                return _lib.E_UNSUPPORTED
            return 0
        return entry


def fused_unsupported(entry, a):
    """the answers that send a wrapper down its fall-through path: the fused entries the wrappers may compose from others"""
    return (entry in ("dbmm_conv3x3_c32_bn_relu_x2", "dbmm_gemm_dual_bn_act_x2", "dbmm_bottleneck_chain_x2",
                      "dbmm_bottleneck_chain_dual_x2", "dbmm_bottleneck_block_chain_x2", "dbmm_conv1x1_bn_act_f16_ws",
                      "dbmm_conv1x1_dual_bn_act_f16", "dbmm_bottleneck_chain_f16", "dbmm_bottleneck_chain_pool_f16",
                      "dbmm_bottleneck_chain_dual_f16", "dbmm_conv3x3_bn_relu_f16", "dbmm_conv1x1_res_pool_f16")
            or (entry == "dbmm_conv_bn_act_x2" and a["pool"] == 2))


def _no_meta(*tensors):
    """stand-in for require_cuda on a machine without a GPU: host tensors play the device, meta tensors another device"""
    for t in tensors:
        if t is not None and t.device.type == "meta":
            raise _lib.DbmmError("operand on another device")


def install(monkeypatch, unsupported=None):
    """put the stub library, the device stand-ins and the registering allocator in place; returns (stub, registry)"""
    stub, reg = Stub(unsupported), Registry()
    monkeypatch.setattr(_lib, "lib", lambda: stub)
    for mod in (ops, preprocess):                       # both bind these names at import
        monkeypatch.setattr(mod, "require_cuda", _no_meta)
        monkeypatch.setattr(mod, "stream", lambda: None)
        monkeypatch.setattr(mod, "_empty", reg.empty, raising=False)     # (a module without the hook fails the audit of its outputs)
    monkeypatch.setattr(ops, "_ws_cache", {})
    monkeypatch.setattr(preprocess, "_dev_plans", {})
    real_plan = preprocess.plan

    def plan(*a, **k):                                  # the coefficient tables are built with torch.from_numpy(...).to(device)
        p = real_plan(*a, **k)
        reg.add_tree(p)
        return p
    monkeypatch.setattr(preprocess, "plan", plan)
    return stub, reg


def audit(stub, reg):
    """findings (strings) over every recorded call: each pointer argument resolves to a registered tensor of the spec's dtype, contiguous,
    with the spec's extent inside what remains of the tensor from that address"""
    found = []
    for entry, args in stub.calls:
        if entry not in SPEC:
            found.append(f"{entry}: not an audited entry")
            continue
        names, derive, cells = arg_names(entry), SPEC[entry][1], SPEC[entry][2]
        env = {n: v for n, v in zip(names, args) if isinstance(v, int) and n not in cells}
        env.update(F32=F32, F16=F16)
        exec(derive, {}, env)
        for i in pointer_positions(entry):
            name, address = names[i], args[i]
            if name == "stream" or cells.get(name) == HOST:
                continue
            if name == "workspace":
                t = reg.find(address) if address is not None else None
                need = env["workspace_bytes"]
                if t is None or t.data_ptr() + t.numel() * t.element_size() - address < need:
                    found.append(f"{entry}({name}): {need} workspace bytes are not there")
                continue
            dtype, count = cells[name][0], eval(cells[name][1], {}, env)
            if address is None:
                if "null" not in cells[name]:
                    found.append(f"{entry}({name}): NULL where the entry reads {count} elements")
                continue
            t = reg.find(address)
            if t is None:
                found.append(f"{entry}({name}): pointer {address} is no tensor on the device")
                continue
            if isinstance(dtype, str):
                dtype = eval(dtype, {}, env)
            if t.dtype != dtype:
                found.append(f"{entry}({name}): {t.dtype} where the entry reads {dtype}")
                continue
            if not t.is_contiguous():
                found.append(f"{entry}({name}): not contiguous")
                continue
            left = (t.data_ptr() + t.numel() * t.element_size() - address) // t.element_size()
            if left < count:
                found.append(f"{entry}({name}): {left} elements where the entry indexes {count}")
    return found


# ---- valid calls ------------------------------------------------------------------------------------------------------------------

def leaves(tree, path=()):
    """(path, tensor) of every tensor in nested tuples / lists / dicts"""
    if isinstance(tree, torch.Tensor):
        yield path, tree
    elif isinstance(tree, dict):
        for k, v in tree.items():
            yield from leaves(v, path + (k,))
    elif isinstance(tree, (tuple, list)):
        for i, v in enumerate(tree):
            yield from leaves(v, path + (i,))


def replaced(tree, path, new):
    if not path:
        return new
    if isinstance(tree, dict):
        return {k: (replaced(v, path[1:], new) if k == path[0] else v) for k, v in tree.items()}
    return type(tree)(replaced(v, path[1:], new) if i == path[0] else v for i, v in enumerate(tree))


def mapped(tree, fn):
    if isinstance(tree, torch.Tensor):
        return fn(tree)
    if isinstance(tree, dict):
        return {k: mapped(v, fn) for k, v in tree.items()}
    if isinstance(tree, (tuple, list)):
        return type(tree)(mapped(v, fn) for v in tree)
    return tree


_gen = torch.Generator().manual_seed(20)


def f32(*shape):
    """uniform in (-1, 1), every value exact in fp16 (so a weight equals its single fp16 plane)"""
    return (torch.rand(shape, generator=_gen) * 2 - 1).half().float()


def f16(*shape):
    return f32(*shape).half()


def pos(*shape):
    """a BatchNorm scale: in (0.5, 1.5)"""
    return (torch.rand(shape, generator=_gen) + 0.5).half().float()


def one():
    return torch.ones(1)                # an upper bound of max|x| for the operands above


def zero():
    return torch.zeros(1)


def conv_plan(N, K, wl=ops.WL_TAP_MAJOR, bias=True):
    """what the chain wrappers read of a plan entry (clip/model.py _pack_conv, an fp16-stored weight): one exact plane with its exponent
    and K order, BatchNorm scale and bias apart.  The entries they do not read (`w`, `p3`; a bias the dual form replaces) are left out:
    a mutation of an operand nobody reads is no bad call."""
    c = dict(wl=wl, ph=f16(1, N, K), we=0, sc=pos(N))
    return dict(c, b=f32(N)) if bias else c


def conv_f16(N, K):
    return (f16(N, K), pos(N), f32(N))


class Case:
    """one valid call: `fn` ("ops.gemm"), arguments by name (tensors may sit inside tuples and dicts), the shapes and dtypes of the
    tensors it returns (None: that slot is None), whether the wrapper answers None when its fused entry answers DBMM_E_UNSUPPORTED, and
    what the generated mutations may not assume:
      free: (operand path, mutation) pairs that give another VALID call, because that operand alone defines the dimension;
      converted: operands the wrapper converts itself (width and layout mutations are then served, on the converted tensor)."""

    def __init__(self, id, fn, kwargs, outs, free=(), converted=(), may_be_none=False):
        self.id, self.fn, self.kwargs, self.outs = id, fn, kwargs, outs
        self.free, self.converted, self.may_be_none = set(free), set(converted), may_be_none

    def call(self, kwargs=None):
        mod, name = self.fn.split(".")
        return getattr({"ops": ops, "preprocess": preprocess}[mod], name)(**(self.kwargs if kwargs is None else kwargs))


def _cases():
    R, T, C32 = ops.ACT_RELU, ops.WL_TAP_MAJOR, ops.WL_CHUNK32_MAJOR
    cs = []

    def add(*a, **k):
        cs.append(Case(*a, **k))
    # a weight alone defines N (and an activation alone its row count) where no other operand pins it: one row less is a smaller valid call
    ROWS_A = [(("a",), "row_short")]       # gemm: M = a's rows; bias pins N and w pins K, the residual (pitch ldr) need only be long enough
    BOTH = [(("x",), "width")]             # a wrapper that takes fp32 and fp16 input and tells the entry which (x_is_f16)
    add("split_planes", "ops.split_planes", dict(w=f32(8, 16)), [((3, 8, 16), BF16)], free=[(("w",), "row_short")])
    add("split_planes_f16", "ops.split_planes_f16", dict(w=torch.rand((8, 16), generator=_gen)), [((2, 8, 16), F16)],
        free=[(("w",), "row_short")])
    add("gemm", "ops.gemm", dict(a=f32(5, 8), w=f32(4, 8), bias=f32(4), residual=f32(5, 4), act=R), [((5, 4), F32)], free=ROWS_A)
    add("gemm-trans", "ops.gemm", dict(a=f32(8, 4), w=f32(8, 4), bias=f32(4), trans_a=True, trans_w=True), [((4, 4), F32)])
    add("gemm-lda-out", "ops.gemm", dict(a=f32(4 * 24 + 8), w=f32(4, 8), bias=f32(4), M=5, K=8, lda=24, out=f32(5, 4)), [((5, 4), F32)])
    add("gemm-x2", "ops.gemm", dict(a=f32(8, 32), w=(w := f32(8, 32)), bias=f32(8), residual=f32(8, 8), w_planes_f16=w.half().reshape(1, 8, 32),
                                    w_exp=0, a_absmax=one(), c_absmax=zero()), [((8, 8), F32)], free=ROWS_A)
    add("gemm-x3", "ops.gemm", dict(a=f32(8, 16), w=f32(40, 16), bias=f32(40), residual=f32(8, 40), w_planes=f32(3, 40, 16).bfloat16()),
        [((8, 40), F32)], free=ROWS_A)
    conv = dict(kh=3, kw=3, stride=1, pad=1, act=R)
    add("conv", "ops.conv_bn_act", dict(x=f32(1, 4, 4, 8), w=f32(8, 72), bias=f32(8), residual=f32(1, 4, 4, 8), **conv), [((1, 4, 4, 8), F32)])
    add("conv-x3", "ops.conv_bn_act", dict(x=f32(1, 4, 4, 16), w=f32(40, 144), bias=f32(40), residual=f32(1, 4, 4, 40),
                                           w_planes=f32(3, 40, 144).bfloat16(), **conv), [((1, 4, 4, 40), F32)])
    for pool in (1, 2):
        w = f32(32, 288)
        add(f"conv-patch-pool{pool}", "ops.conv_bn_act",
            dict(x=f32(1, 4, 28, 32), w=w, bias=f32(32), residual=None, w_layout=T, w_planes_f16=w.half().reshape(1, 32, 288), w_exp=0,
                 x_absmax=one(), y_absmax=zero(), out_scale=pos(32), pool=pool, **conv), [((1, 4 // pool, 28 // pool, 32), F32)])
    for keep in (False, True):
        w = f32(64, 32)
        add(f"conv-x2-pool-keep{int(keep)}", "ops.conv_bn_act",
            dict(x=f32(1, 4, 4, 32), w=w, bias=f32(64), residual=f32(1, 4, 4, 64), kh=1, kw=1, stride=1, pad=0, act=R,
                 w_planes_f16=w.half().reshape(1, 64, 32), w_exp=0, x_absmax=one(), y_absmax=zero(), out_scale=pos(64), pool=2, keep_full=keep),
            [((1, 2, 2, 64), F32)] + ([((1, 4, 4, 64), F32)] if keep else []))
    ND = 192 * 128            # the library serves the dual GEMM from 192 tiles of 128 x 128 on: four rows, 192 tiles of channels
    add("gemm_dual", "ops.gemm_dual",
        dict(a=f32(1, 2, 2, 64), a_absmax=one(), w_plane=f16(1, ND, 64), w_exp=0, out_scale=pos(ND), a2=f32(1, 2, 2, 64), a2_absmax=one(),
             w2_plane=f16(1, ND, 64), ratio=pos(ND), bias=f32(ND), c_absmax=zero()), [((1, 2, 2, ND), F32)], may_be_none=True)
    for tag, kw, outs in (("", dict(), [((1, 2, 2, 128), F32), ((1, 2, 2, 64), F32)]),
                          ("-pooled", dict(pooled=True), [((1, 2, 2, 128), F32), ((1, 1, 1, 128), F32), ((1, 2, 2, 64), F32)]),
                          ("-pooled-nokeep", dict(pooled=True, keep_full=False), [None, ((1, 1, 1, 128), F32), ((1, 2, 2, 64), F32)])):
        add("bottleneck_chain" + tag, "ops.bottleneck_chain",
            dict(y2=f32(1, 2, 2, 64), y2_absmax=one(), c3=conv_plan(128, 64), residual=f32(1, 2, 2, 128), c1=conv_plan(64, 128),
                 x_absmax=zero(), y1_absmax=zero(), **kw), outs, may_be_none=True)
        add("chain_f16" + tag, "ops.chain_f16",
            dict(y2=f16(1, 2, 2, 64), c3=conv_f16(128, 64), residual=f16(1, 2, 2, 128), c1=conv_f16(64, 128), **kw),
            [o and (o[0], F16) for o in outs], may_be_none=True)
    block = dict(y1=f32(1, 2, 2, 64), y1_absmax=one(), c2=conv_plan(64, 576, C32), c3=conv_plan(128, 64), c1=conv_plan(64, 128),
                 x_absmax=zero(), y1n_absmax=zero())
    add("block_chain-residual", "ops.bottleneck_block_chain", dict(block, residual=f32(1, 2, 2, 128)),
        [((1, 2, 2, 128), F32), ((1, 2, 2, 64), F32)], may_be_none=True)
    add("block_chain-dual", "ops.bottleneck_block_chain",
        dict(block, c3=conv_plan(128, 64, bias=False),
             dual=dict(a2=f32(1, 2, 2, 64), a2_absmax=one(), ds=dict(ph=f16(1, 128, 64)), ratio=pos(128), bias=f32(128))),
        [((1, 2, 2, 128), F32), ((1, 2, 2, 64), F32)], may_be_none=True)
    add("bottleneck_chain_dual", "ops.bottleneck_chain_dual",
        dict(y2=f32(1, 2, 2, 64), y2_absmax=one(), c3=conv_plan(128, 64, bias=False), a2=f32(1, 2, 2, 64), a2_absmax=one(),
             ds=dict(ph=f16(1, 128, 64)),
             ratio=pos(128), bias=f32(128), c1=conv_plan(64, 128), x_absmax=zero(), y1_absmax=zero()),
        [((1, 2, 2, 128), F32), ((1, 2, 2, 64), F32)], may_be_none=True)
    add("conv_stem_s2", "ops.conv_stem_s2", dict(x_nchw=f32(1, 3, 8, 8), w=f32(3, 3, 3, 32), bias=f32(32), y_absmax=zero()),
        [((1, 4, 4, 32), F32)])
    add("avgpool2d", "ops.avgpool2d", dict(x=f32(1, 4, 4, 8), k=2), [((1, 2, 2, 8), F32)])
    for tag, x in (("f32", f32(1, 2, 2, 64)), ("f16", f16(1, 2, 2, 64))):
        add("attnpool-" + tag, "ops.attnpool", dict(x=x, pos=f32(5, 64), wq=f32(64, 64), bq=f32(64), wkv=f32(128, 64), bkv=f32(128),
                                                    wc=f32(32, 64), bc=f32(32), heads=1), [((1, 32), F32)], free=BOTH)
    for sfx, mk, dt in (("", f32, F32), ("_f16", f16, F16)):
        am = dict(y_absmax=zero()) if not sfx else {}
        add("layernorm" + sfx, "ops.layernorm" + sfx, dict(x=mk(6, 64), gamma=pos(64), beta=f32(64), **am), [((6, 64), dt)],
            free=[(("x",), "row_short"), (("x",), "short1")])                               # rows = x.numel() // E, rounded down
        add("layernorm" + sfx + "-rows-ldx", "ops.layernorm" + sfx, dict(x=mk(192 + 64), gamma=pos(64), beta=f32(64), rows=2, ldx=192),
            [((2, 64), dt)])
        add("vit_tokens" + sfx, "ops.vit_tokens" + sfx, dict(patches=mk(8, 64), cls=f32(64), pos=f32(5, 64), B=2), [((2, 5, 64), dt)])
        add("embed_gather" + sfx, "ops.embed_gather" + sfx,
            dict(tokens=torch.arange(8).reshape(2, 4), table=f32(10, 64), pos=f32(4, 64)), [((2, 4, 64), dt), ((2, 4), I32)],
            converted=["tokens"], free=[(("tokens",), "row_short"), (("table",), "row_short")])   # n = tokens rows, vocab = table rows
        add("gather_eot" + sfx, "ops.gather_eot" + sfx, dict(tokens_i32=torch.arange(8, dtype=I32).reshape(2, 4), x=mk(2, 4, 64)),
            [((2, 64), dt)])
    add("mha_core", "ops.mha_core", dict(qkv=f32(8, 192), B=2, L=4, E=64, heads=1, causal=True), [((8, 64), F32)])
    add("mha_core-x2", "ops.mha_core", dict(qkv=f32(8, 192), B=2, L=4, E=64, heads=1, causal=False, qkv_absmax=one()), [((8, 64), F32)])
    add("mha_core_f16", "ops.mha_core_f16", dict(qkv=f16(8, 192), B=2, L=4, E=64, heads=1, causal=True), [((8, 64), F16)])
    add("im2col_patch", "ops.im2col_patch", dict(x_nchw=f32(1, 3, 8, 8), P=4, out_absmax=zero()), [((4, 48), F32)])
    for tag, x in (("f32", f32(1, 3, 8, 8)), ("f16", f16(1, 3, 8, 8))):
        add("im2col_patch_f16-" + tag, "ops.im2col_patch_f16", dict(x_nchw=x, P=4, Kp=64), [((4, 64), F16)], free=[(("x_nchw",), "width")])
        for scale in (None, pos(32)):
            add(f"conv_stem_s2_f16-{tag}-scale{int(scale is not None)}", "ops.conv_stem_s2_f16",
                dict(x_nchw=x.clone(), w=f32(3, 3, 3, 32), bias=f32(32), scale=scale), [((1, 4, 4, 32), F16)], free=[(("x_nchw",), "width")])
    add("text_colnorm", "ops.text_colnorm", dict(text=f32(64, 4)), [((4, 64), F32)], free=[(("text",), "row_short")])
    add("l2norm_rows", "ops.l2norm_rows", dict(x=f32(4, 64)), [((4, 64), F32)], free=[(("x",), "row_short")])
    add("colsum", "ops.colsum", dict(x=f32(4, 64)), [((64,), F32)], free=[(("x",), "row_short")])
    add("gemm_f16", "ops.gemm_f16", dict(a=f16(8, 64), w=f16(8, 64), bias=f32(8), residual=f16(8, 8), act=R), [((8, 8), F16)])
    add("gemm_f16-lda", "ops.gemm_f16", dict(a=f16(2 * 128 + 64), w=f16(8, 64), bias=f32(8), M=3, lda=128), [((3, 8), F16)])
    add("conv1x1_f16", "ops.conv1x1_f16", dict(x=f16(1, 2, 2, 64), w=f16(64, 64), scale=pos(64), bias=f32(64), residual=f16(1, 2, 2, 64)),
        [((1, 2, 2, 64), F16)], may_be_none=True)
    add("conv1x1_res_pool_f16", "ops.conv1x1_res_pool_f16", dict(x=f16(1, 2, 2, 128), c3=conv_f16(64, 128), residual=f16(1, 2, 2, 64)),
        [((1, 2, 2, 64), F16), ((1, 1, 1, 64), F16)], may_be_none=True)
    dual = dict(y2=f16(1, 2, 2, 64), w3=f16(128, 64), scale3=pos(128), xp=f16(1, 2, 2, 64), wd=f16(128, 64), ratio=pos(128), bias=f32(128))
    add("chain_dual_f16", "ops.chain_dual_f16", dict(dual, c1=conv_f16(64, 128)), [((1, 2, 2, 128), F16), ((1, 2, 2, 64), F16)],
        may_be_none=True)
    add("conv1x1_dual_f16", "ops.conv1x1_dual_f16", dict(mapped(dual, torch.clone)), [((1, 2, 2, 128), F16)], may_be_none=True)
    for pool in (1, 2):
        add(f"conv3x3_f16-pool{pool}", "ops.conv3x3_f16", dict(x=f16(1, 4, 4, 32), w=f16(32, 288), scale=pos(32), bias=f32(32), pool=pool),
            [((1, 4 // pool, 4 // pool, 32), F16)], may_be_none=True)
    add("avgpool2_f16", "ops.avgpool2_f16", dict(x=f16(1, 4, 4, 8)), [((1, 2, 2, 8), F16)])
    img = lambda *s: torch.randint(0, 256, s, generator=_gen, dtype=U8)
    add("preprocess_u8", "preprocess.preprocess_u8", dict(img_hwc=img(10, 12, 3), n_px=8), [((3, 8, 8), F32)])
    add("preprocess_u8-out-u8", "preprocess.preprocess_u8", dict(img_hwc=img(10, 12, 3), n_px=8, out=f32(3, 8, 8), return_u8=True),
        [((3, 8, 8), F32), ((8, 8, 3), U8)])
    add("preprocess_uniform", "preprocess.preprocess_uniform", dict(images_bhwc=img(2, 10, 12, 3), n_px=8), [((2, 3, 8, 8), F32)])
    add("preprocess_uniform-out", "preprocess.preprocess_uniform", dict(images_bhwc=img(2, 10, 12, 3), n_px=8, out=f32(2, 3, 8, 8)),
        [((2, 3, 8, 8), F32)])
    return cs


CASES = _cases()


# ---- mutations --------------------------------------------------------------------------------------------------------------------

_OTHER_WIDTH = {F32: F16, F16: F32, I32: I64, I64: I32, BF16: F32}


def _noncontiguous(t):
    """a view of t's shape and values that is not contiguous (None where every view of that shape is)"""
    if t.dim() >= 1 and t.shape[-1] > 1:
        big = torch.zeros(tuple(t.shape[:-1]) + (2 * t.shape[-1],), dtype=t.dtype)
        v = big[..., ::2]
    elif t.dim() >= 2 and t.shape[-2] > 1:
        v = torch.zeros(tuple(t.shape[:-2]) + (2 * t.shape[-2], t.shape[-1]), dtype=t.dtype)[..., ::2, :]
    else:
        return None
    v.copy_(t)
    return None if v.is_contiguous() else v


def mutations(case):
    """(operand path, mutation name, mutated kwargs) for every tensor operand of a valid call"""
    for path, t in leaves(case.kwargs):
        absmax = any(isinstance(p, str) and p.endswith("absmax") for p in path)
        muts = []
        if t.numel() > 1:
            muts.append(("short1", t.flatten()[:-1].clone()))
        if t.dim() == 2 and t.shape[0] > 1:
            muts.append(("row_short", t[:-1].clone()))
        if t.dtype in _OTHER_WIDTH:
            muts.append(("width", t.to(_OTHER_WIDTH[t.dtype])))
        nc = _noncontiguous(t)
        if nc is not None:
            muts.append(("noncontig", nc))
        muts.append(("meta", torch.empty(t.shape, dtype=t.dtype, device="meta")))
        if absmax:
            muts.append(("empty", t.flatten()[:0].clone()))
        muts.append(("none", None))                     # NULL: refused, or a valid call where the entry takes NULL there
        for name, new in muts:
            yield path, name, replaced(case.kwargs, path, new)
