"""ctypes binding of libmodcr_hip.so (C ABI: include/modcr_hip.h) + thin torch-tensor wrappers.

PyTorch is plumbing here: it owns device memory and the stream; every piece of arithmetic on the
hot path is a hand-written HIP kernel behind the C ABI.  There is NO fallback: if the shared
library is missing or a call fails, an exception is raised.
"""
import collections
import ctypes
import os

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libmodcr_hip.so")

BF16, F32, F16 = 0, 1, 2
ACT_NONE, ACT_GELU, ACT_TANH = 0, 1, 2
# modcr_linear_route: kernel ids (MODCR_ROUTE_*) and epilogue bits
ROUTE_KERNELS = {1: "f32_tile", 2: "f32_rowdot", 3: "ring128", 4: "ring192", 5: "ring256", 6: "p8", 7: "t192", 8: "d4"}
ROUTE_DIRECT, ROUTE_SPEC = 1, 2

# modcr_linear_bwd_weight_route / modcr_linear_bwd_input_route (MODCR_BWD_*)
BWD_WEIGHT_FORMS = {1: "f32", 2: "nt", 3: "half_tn", 4: "swapped", 5: "tn"}
BWD_PRODUCTS = {0: "f32", 1: "splitk", 2: "dispatch"}
BWD_REDUCTIONS = {0: "none", 1: "plain", 2: "transposed"}
BWD_DB_METHODS = {0: "none", 1: "fused_reduce", 2: "fused_fold", 3: "rowsum", 4: "block_fold", 5: "atomic", 6: "colsum"}
BWD_INPUT_FORMS = {1: "f32", 2: "fwd", 3: "splitk"}

_c = ctypes
_vp, _i32, _i64, _f32 = _c.c_void_p, _c.c_int32, _c.c_int64, _c.c_float

# name -> (restype, argtypes); mirrors include/modcr_hip.h one to one
SIGNATURES = {
    "modcr_version": (_i32, []),
    "modcr_last_error": (_c.c_char_p, []),
    "modcr_qkv_attn_fwd": (_i32, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i32, _vp, _vp, _vp, _i32, _i32,
                                  _i32, _i32, _i32, _i32, _vp, _i64, _i32, _vp]),
    "modcr_qkv_attn_dropout_fwd": (_i32, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i32, _vp, _vp, _vp, _i32, _i32,
                                          _i32, _i32, _i32, _i32, _f32, _c.c_uint64, _c.c_uint64, _vp, _i64, _i32, _vp]),
    "modcr_qkv_attn_dump_bytes": (_i64, [_i32, _i32, _i32]),
    "modcr_qkv_attn_lse_fwd": (_i32, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i32, _vp, _vp, _vp, _i32, _vp, _vp, _i32,
                                      _i32, _i32, _i32, _i32, _f32, _c.c_uint64, _c.c_uint64, _vp, _i64, _i32, _vp]),
    "modcr_qkv_attn_opt_fwd": (_i32, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i32, _vp, _vp, _vp, _i32, _vp, _vp, _i32,
                                      _i32, _i32, _i32, _i32, _f32, _c.c_uint64, _c.c_uint64, _i32, _vp, _i64, _i32, _vp]),
    "modcr_qkv_attn_rows_fwd": (_i32, [_vp, _vp, _vp, _vp, _vp, _vp, _i32, _vp, _vp, _i32, _vp, _i32, _i32, _i32, _i32, _f32, _c.c_uint64,
                                       _c.c_uint64, _i32, _i32, _vp]),
    "modcr_qkv_attn_bias_workspace": (_i64, [_i32, _i32, _i32, _i32, _i32]),
    "modcr_qkv_attn_bias_fwd": (_i32, [_vp, _vp, _vp, _vp, _vp, _i64, _i64, _i64, _vp, _i64, _vp, _i32, _vp, _vp, _vp, _i32,
                                       _i32, _i32, _i32, _i32, _i32, _f32, _c.c_uint64, _c.c_uint64, _i32, _vp, _i64, _i32, _vp]),
    "modcr_qkv_attn_long_drop_fwd": (_i32, [_vp, _vp, _vp, _vp, _vp, _i64, _i64, _i64, _vp, _i64, _vp, _i32, _vp, _vp, _vp, _i32,
                                            _i32, _i32, _i32, _i32, _i32, _f32, _c.c_uint64, _c.c_uint64, _i32, _vp, _i64, _i32, _vp]),
    "modcr_qkv_attn_long_align_fwd": (_i32, [_vp, _vp, _vp, _vp, _vp, _i64, _i64, _i64, _vp, _i64, _vp, _i32, _vp, _vp, _vp, _i32,
                                             _i32, _i32, _i32, _i32, _i32, _f32, _c.c_uint64, _c.c_uint64, _i32, _vp, _i64, _i32, _vp, _vp]),
    "modcr_qkv_attn_route": (_i32, [_i32, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _f32, _i32, _i64, _i32, _i32, _c.POINTER(_i32)]),
    "modcr_linear_splitk_workspace": (_i64, [_i32, _i32, _i32]),
    "modcr_linear_splitk_fwd": (_i32, [_vp, _i64, _vp, _i64, _vp, _vp, _i64, _i32, _i32, _i32, _i32, _i32, _vp, _i64, _vp]),
    "modcr_qkv_attn_workspace": (_i64, [_i32, _i32, _i32, _i32, _i32]),
    "modcr_time_next_attn": (_i32, [_vp, _vp]),
    "modcr_chunk_mean_q_fwd": (_i32, [_vp, _i64, _i64, _vp, _i32, _i32, _i32, _i32, _vp]),
    "modcr_build_phase_mask": (_i32, [_vp, _vp, _vp, _i32, _i32, _i32, _i32, _vp]),
    "modcr_pack_mask_bits": (_i32, [_vp, _vp, _i64, _i32, _vp]),
    "modcr_build_packed_mask": (_i32, [_vp, _vp, _i32, _i32, _i32, _vp]),
    "modcr_linear_fwd": (_i32, [_vp, _i64, _vp, _i64, _vp, _vp, _i64, _i32, _vp, _i64, _i32, _i32,
                                _i32, _i32, _i32, _i32, _vp]),
    "modcr_linear_route": (_i32, [_vp, _i64, _vp, _i64, _vp, _vp, _i64, _i32, _vp, _i64, _i32, _i32,
                                  _i32, _i32, _i32, _i32, _c.POINTER(_i32)]),
    "modcr_ffn_up_gelu_fwd": (_i32, [_vp, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _vp]),
    "modcr_linear_residual_ln_fwd": (_i32, [_vp, _i64, _vp, _vp, _vp, _vp, _vp, _f32, _vp, _i32, _i32,
                                            _i32, _vp, _i64, _i32, _vp]),
    "modcr_linear_dropout_residual_ln_workspace": (_i64, [_i32, _i32, _i32, _i32]),
    "modcr_linear_dropout_residual_ln_fwd": (_i32, [_vp, _i64, _vp, _vp, _vp, _vp, _vp, _f32, _vp, _vp, _i32, _i32, _i32, _i32, _f32, _c.c_uint64, _c.c_uint64, _vp, _i64, _i32, _vp]),
    "modcr_proj_residual_ln_fwd": (_i32, [_vp, _vp, _vp, _vp, _vp, _vp, _f32, _vp, _i32, _i32, _vp,
                                          _i64, _i32, _vp]),
    "modcr_ffn_down_residual_ln_fwd": (_i32, [_vp, _vp, _vp, _vp, _vp, _vp, _f32, _vp, _i32, _i32, _i32,
                                              _vp, _i64, _i32, _vp]),
    "modcr_layernorm_fwd": (_i32, [_vp, _i32, _vp, _i32, _vp, _vp, _f32, _vp, _i32, _i64, _i32, _i32,
                                   _i64, _vp]),
    "modcr_embed_ln_fwd": (_i32, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _f32, _vp, _i32, _i32, _i32,
                                  _i64, _i32, _i32, _i32, _i32, _vp]),
    "modcr_embed_ln_dropout_fwd": (_i32, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _f32, _vp, _i32, _i32, _i32,
                                          _i64, _i32, _i32, _i32, _i32, _f32, _c.c_uint64, _c.c_uint64, _vp]),
    "modcr_rows_scatter_dropout": (_i32, [_vp, _vp, _i64, _i32, _i32, _i64, _i32, _i32, _f32, _c.c_uint64, _c.c_uint64, _vp]),
    "modcr_cast_pad": (_i32, [_vp, _i64, _vp, _i64, _i64, _i32, _i32, _i32, _vp]),
    "modcr_convert": (_i32, [_vp, _i32, _vp, _i32, _i64, _vp]),
    "modcr_convert_segments": (_i32, [_vp, _vp, _vp, _i32, _i32, _i32, _vp]),
    "modcr_split3_bf16": (_i32, [_vp, _i64, _vp, _i64, _i64, _i32, _i32, _vp]),
    "modcr_align_attn_fwd": (_i32, [_vp, _vp, _vp, _i64, _vp, _vp, _i32, _i32, _i32, _i32, _f32, _f32, _c.c_uint64, _c.c_uint64,
                                    _vp, _i32, _vp]),
    "modcr_align_attn_bwd": (_i32, [_vp, _vp, _vp, _vp, _i64, _vp, _vp, _vp, _vp, _i64, _i32, _i32,
                                    _i32, _i32, _f32, _f32, _c.c_uint64, _c.c_uint64, _i32, _vp]),
    "modcr_cls_xattn_fwd": (_i32, [_vp, _vp, _vp, _vp, _i32, _i64, _vp, _vp, _vp, _i32, _i32, _i32, _f32, _c.c_uint64, _c.c_uint64, _vp]),
    "modcr_cls_xattn_bwd": (_i32, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i32, _i64, _vp, _i32, _i32, _i32, _f32, _c.c_uint64,
                                   _c.c_uint64, _vp]),
    "modcr_mc_ce_fwd_bwd": (_i32, [_vp, _vp, _vp, _vp, _vp, _i32, _i32, _vp]),
    "modcr_linear_bwd_input_workspace": (_i64, [_i32, _i32, _i32]),
    "modcr_linear_bwd_input": (_i32, [_vp, _i64, _i32, _vp, _i64, _vp, _i64, _i32, _i32, _i32, _i32, _i32, _vp, _i64, _vp]),
    "modcr_linear_bwd_weight_workspace": (_i64, [_i32, _i32, _i32]),
    "modcr_linear_bwd_weight": (_i32, [_vp, _i64, _i32, _vp, _i64, _vp, _vp, _i32, _i32, _i32, _i32, _i32, _vp, _i64, _vp]),
    "modcr_linear_bwd_weight_route": (_i32, [_vp, _i64, _i32, _vp, _i64, _vp, _vp, _i32, _i32, _i32, _i32, _i32, _vp, _i64, _c.POINTER(_i32)]),
    "modcr_linear_bwd_input_route": (_i32, [_vp, _i64, _i32, _vp, _i64, _vp, _i64, _vp, _i64, _i32, _i32, _i32, _i32, _i32, _vp, _i64,
                                            _c.POINTER(_i32)]),
    "modcr_layernorm_bwd": (_i32, [_vp, _vp, _vp, _vp, _f32, _vp, _vp, _vp, _i64, _i32, _vp]),
    "modcr_act_bwd": (_i32, [_vp, _vp, _vp, _i64, _i32, _vp]),
    "modcr_qkv_attn_bwd_workspace": (_i64, [_i32, _i32, _i32, _i32]),
    "modcr_qkv_attn_bwd": (_i32, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i32, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _i32,
                                  _vp, _i64, _i32, _vp]),
    "modcr_qkv_attn_dropout_bwd": (_i32, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i32, _vp, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _i32,
                                          _f32, _c.c_uint64, _c.c_uint64, _vp, _i32, _vp, _i64, _i32, _vp]),
    "modcr_qkv_attn_lse_bwd": (_i32, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i32, _vp, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _i32,
                                      _f32, _c.c_uint64, _c.c_uint64, _vp, _i32, _vp, _vp, _vp, _vp, _i64, _i32, _vp]),
    "modcr_qkv_attn_opt_bwd": (_i32, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i32, _vp, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _i32,
                                      _f32, _c.c_uint64, _c.c_uint64, _vp, _i32, _vp, _vp, _vp, _i32, _vp, _i64, _i32, _vp]),
    "modcr_qkv_attn_bias_bwd_workspace": (_i64, [_i32, _i32, _i32, _i32]),
    "modcr_qkv_attn_bias_bwd_route": (_i32, [_i32, _i32, _i32, _i32, _i32]),
    "modcr_qkv_attn_bias_bwd": (_i32, [_vp, _vp, _vp, _vp, _vp, _i64, _i64, _i64, _vp, _i64, _vp, _i32, _vp, _vp, _vp, _vp, _i32, _vp,
                                       _i32, _i32, _i32, _i32, _f32, _c.c_uint64, _c.c_uint64, _vp, _i64, _i32, _vp]),
    "modcr_qkv_attn_prefix_bwd_workspace": (_i64, [_i32, _i32, _i32, _i32, _i32]),
    "modcr_qkv_attn_prefix_bwd_route": (_i32, [_i32, _i32, _i32, _i32, _i32, _i32]),
    "modcr_qkv_attn_prefix_bwd": (_i32, [_vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _i64, _vp, _i64, _vp, _vp, _vp, _vp, _vp, _i32, _vp,
                                         _i32, _i32, _i32, _i32, _i32, _f32, _c.c_uint64, _c.c_uint64, _vp, _i64, _i32, _vp]),
    "modcr_qkv_attn_gate_bwd_workspace": (_i64, [_i32, _i32, _i32, _i32, _i32]),
    "modcr_qkv_attn_gate_bwd_route": (_i32, [_i32, _i32, _i32, _i32, _i32, _i32]),
    "modcr_qkv_attn_long_bwd_workspace": (_i64, [_i32, _i32, _i32, _i32, _i32]),
    "modcr_qkv_attn_long_bwd_route": (_i32, [_i32, _i32, _i32, _i32, _i32, _i32]),
    "modcr_qkv_attn_gate_bwd": (_i32, [_vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _i64, _vp, _i64, _vp, _i32, _vp, _vp, _vp, _vp, _vp, _i32,
                                       _vp, _vp, _i32, _i32, _i32, _i32, _i32, _f32, _c.c_uint64, _c.c_uint64, _vp, _i64, _i32, _vp]),
    "modcr_qkv_attn_long_bwd": (_i32, [_vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _i64, _vp, _i64, _vp, _i32, _vp, _vp, _vp, _vp, _vp, _i32,
                                       _vp, _vp, _i32, _i32, _i32, _i32, _i32, _f32, _c.c_uint64, _c.c_uint64, _vp, _i64, _i32, _vp]),
    "modcr_qkv_attn_long_drop_bwd_workspace": (_i64, [_i32, _i32, _i32, _i32, _i32]),
    "modcr_qkv_attn_long_drop_bwd_route": (_i32, [_i32, _i32, _i32, _i32, _i32, _i32]),
    "modcr_qkv_attn_long_drop_bwd": (_i32, [_vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _i64, _vp, _i64, _vp, _i32, _vp, _vp, _vp, _vp, _vp, _i32,
                                            _vp, _vp, _i32, _i32, _i32, _i32, _i32, _f32, _c.c_uint64, _c.c_uint64, _vp, _i64, _i32, _vp]),
    "modcr_qkv_attn_long_align_bwd_workspace": (_i64, [_i32, _i32, _i32, _i32, _i32]),
    "modcr_qkv_attn_long_align_bwd_route": (_i32, [_i32, _i32, _i32, _i32, _i32, _i32]),
    "modcr_qkv_attn_long_align_bwd": (_i32, [_vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _i64, _vp, _i64, _vp, _i32, _vp, _vp, _vp, _vp, _vp, _i32,
                                             _vp, _vp, _i32, _i32, _i32, _i32, _i32, _f32, _c.c_uint64, _c.c_uint64, _vp, _i64, _i32, _vp,
                                             _vp, _vp, _i32, _i32]),
    "modcr_linear_residual_ln_bwd_workspace": (_i64, [_i32, _i32, _i32]),
    "modcr_linear_residual_ln_bwd": (_i32, [_vp, _vp, _vp, _i64, _vp, _vp, _f32, _vp, _vp, _vp, _vp, _vp, _vp, _i32, _i32, _i32,
                                            _vp, _i64, _i32, _vp]),
    "modcr_linear_residual_ln_dropout_bwd": (_i32, [_vp, _i32, _vp, _i32, _vp, _i64, _vp, _vp, _f32, _vp, _vp, _vp, _vp, _vp, _vp, _i32, _i32, _i32, _f32, _c.c_uint64, _c.c_uint64, _vp, _i64, _i32, _vp]),
    "modcr_layernorm_dropout_bwd": (_i32, [_vp, _i32, _vp, _i32, _vp, _f32, _vp, _vp, _vp, _vp, _i64, _i32, _f32, _c.c_uint64, _c.c_uint64, _vp]),
    "modcr_proj_residual_ln_bwd": (_i32, [_vp, _vp, _vp, _vp, _vp, _f32, _vp, _vp, _vp, _vp, _vp, _vp, _i32, _i32, _vp, _i64, _i32, _vp]),
    "modcr_ffn_down_residual_ln_bwd": (_i32, [_vp, _vp, _vp, _vp, _vp, _f32, _vp, _vp, _vp, _vp, _vp, _vp, _i32, _i32, _i32, _vp, _i64,
                                              _i32, _vp]),
    "modcr_ffn_keep_supported": (_i32, [_i32, _i32, _i32, _i32]),
    "modcr_ffn_up_gelu_keep_fwd": (_i32, [_vp, _vp, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _vp]),
    "modcr_ffn_down_gelu_bwd_workspace": (_i64, [_i32, _i32, _i32]),
    "modcr_ffn_down_residual_ln_gelu_bwd": (_i32, [_vp, _i32, _vp, _i32, _vp, _vp, _vp, _f32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i32, _i32, _i32, _f32, _c.c_uint64, _c.c_uint64, _vp, _i64, _i32, _vp]),
    "modcr_ffn_up_du_bwd_workspace": (_i64, [_i32, _i32, _i32]),
    "modcr_ffn_up_du_bwd": (_i32, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i32, _i32, _i32, _vp, _i64, _i32, _vp]),
    "modcr_ffn_up_gelu_bwd_workspace": (_i64, [_i32, _i32, _i32]),
    "modcr_ffn_up_gelu_bwd": (_i32, [_vp, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i32, _i32, _i32, _vp, _i64, _i32, _vp]),
    "modcr_chunk_mean_q_bwd": (_i32, [_vp, _i64, _i64, _vp, _i32, _i32, _i32, _i32, _vp]),
    "modcr_dropout": (_i32, [_vp, _vp, _i64, _i32, _f32, _c.c_uint64, _c.c_uint64, _vp]),
    "modcr_dropout_residual_ln_fwd": (_i32, [_vp, _i32, _vp, _i32, _vp, _vp, _f32, _vp, _i32, _vp, _i32, _i64, _i32, _f32, _c.c_uint64, _c.c_uint64, _vp]),
    "modcr_dropout_residual_ln_rows_fwd": (_i32, [_vp, _i32, _vp, _i32, _vp, _vp, _f32, _vp, _i32, _vp, _i32, _i64, _i32, _f32, _c.c_uint64, _c.c_uint64,
                                                  _vp, _vp]),
    "modcr_linear_dropout_residual_ln_rows_fwd": (_i32, [_vp, _i64, _vp, _vp, _vp, _vp, _vp, _f32, _vp, _vp, _i32, _i32, _i32, _i32, _f32, _c.c_uint64,
                                                         _c.c_uint64, _vp, _vp, _i64, _i32, _vp]),
    "modcr_rows_take": (_i32, [_vp, _i64, _vp, _vp, _i64, _i32, _i32, _vp]),
    "modcr_embed_ln_dropout_rows_fwd": (_i32, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _f32, _vp, _i32, _i32, _i32,
                                               _i64, _i32, _i32, _i32, _i32, _f32, _c.c_uint64, _c.c_uint64, _vp, _i64, _vp]),
    "modcr_rows_place_dropout": (_i32, [_vp, _i64, _vp, _vp, _vp, _i64, _i64, _i32, _i32, _i64, _i32, _i32, _f32, _c.c_uint64, _c.c_uint64, _vp]),
    "modcr_cast_pad_rows": (_i32, [_vp, _i64, _i64, _vp, _i64, _i64, _i32, _i32, _vp, _vp]),
    "modcr_add": (_i32, [_vp, _vp, _i32, _vp, _i32, _i64, _vp]),
    "modcr_embedding_bwd_v": (_i32, [_vp, _vp, _vp, _vp, _i32, _i32, _i64, _i64, _vp]),
    "modcr_embedding_bwd": (_i32, [_vp, _vp, _vp, _vp, _i32, _i32, _i64, _vp]),
    "modcr_sumsq_f32": (_i32, [_vp, _i64, _vp, _vp]),
    "modcr_sumsq_partials": (_i32, []),
    "modcr_sumsq_f32_ordered": (_i32, [_vp, _i64, _vp, _vp, _i32, _vp]),
    "modcr_adamw_step": (_i32, [_vp, _vp, _vp, _vp, _i64, _vp, _f32, _f32, _f32, _f32, _f32, _f32, _f32, _f32, _vp]),
    "modcr_adamw_hf_step": (_i32, [_vp, _vp, _vp, _vp, _i64, _vp, _f32, _f32, _f32, _f32, _f32, _f32, _f32, _f32, _vp]),
}

_lib = None
_product_lib = None
TUNING_LIB_PATH = os.path.join(_HERE, "libmodcr_hip_tuning.so")


class ModcrHipError(RuntimeError):
    pass


def _load(path):
    if not os.path.exists(path):
        raise ModcrHipError(
            "%s not found -- build it with `make -C %s%s` (hipcc, gfx950). "
            "There is no CPU fallback for the ModCR hot path." % (path, os.path.join(_HERE, "..", "csrc"),
                                                                  " tuning" if path == TUNING_LIB_PATH else ""))
    l = ctypes.CDLL(path)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(l, name)          # AttributeError if the ABI drifted
        fn.restype = res
        fn.argtypes = args
    return l


def lib():
    """Load libmodcr_hip.so (built by __graft_entry__.build() / csrc/Makefile).  Fails loudly."""
    global _lib, _product_lib
    if _lib is None:
        _product_lib = _load(LIB_PATH)
        _lib = _product_lib
    return _lib


def use_tuning_library(on=True):
    """tools/ and a few tests only: route every call through libmodcr_hip_tuning.so (same sources, -DMODCR_TUNING), the
    build in which the MODCR_* environment knobs of csrc/common.h exist.  The product library reads no environment
    variable.  use_tuning_library(False) switches back."""
    global _lib
    lib()
    _lib = _load(TUNING_LIB_PATH) if on else _product_lib
    return _lib


def is_tuning_library():
    return _lib is not None and _lib is not _product_lib


def _check(rc, what):
    if rc != 0:
        raise ModcrHipError("%s failed (%d): %s" % (what, rc, lib().modcr_last_error().decode()))


def dt_of(t):
    if t.dtype == torch.bfloat16:
        return BF16
    if t.dtype == torch.float32:
        return F32
    if t.dtype == torch.float16:
        return F16
    raise ModcrHipError("unsupported dtype %s" % t.dtype)


def torch_dtype(dt):
    return {BF16: torch.bfloat16, F32: torch.float32, F16: torch.float16}[dt]


def _ptr(t):
    if t is None:
        return None
    if not t.is_cuda:
        raise ModcrHipError("tensor must live on the GPU (got %s)" % t.device)
    return ctypes.c_void_p(t.data_ptr())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _contig(t, dtype=None):
    if t is None:
        return None
    if dtype is not None and t.dtype != dtype:
        t = t.to(dtype)
    return t if t.is_contiguous() else t.contiguous()


# ------------------------------------------------------------------------------------------------
SPLITK = True        # tools may clear it for an A/B run: few-row GEMMs through the split-K entry


def linear(a, w, bias=None, act=ACT_NONE, residual=None, out_dtype=None, out=None):
    """act(a @ w.T + bias) (+ residual).  a [..., K] (last dim contiguous, uniform row stride),
    w [N, K].  Returns [..., N]."""
    dt = dt_of(w)
    if a.dtype != w.dtype:
        raise ModcrHipError("linear: activation %s vs weight %s" % (a.dtype, w.dtype))
    k = a.shape[-1]
    if a.dim() == 2 and a.stride(1) == 1:
        a2, lda = a, a.stride(0)
    else:
        a2 = a.reshape(-1, k)
        a2 = _contig(a2)
        lda = k
    m, n = a2.shape[0], w.shape[0]
    w = _contig(w)
    od = dt if out_dtype is None else out_dtype
    if out is None:
        out = torch.empty((m, n), dtype=torch_dtype(od), device=a.device)
    res2 = None
    if residual is not None:
        res2 = _contig(residual.reshape(-1, n))
    if dt == BF16 and res2 is None and 256 <= m <= 1024 and SPLITK and od != F16:
        need = lib().modcr_linear_splitk_workspace(m, n, k)         # few-row GEMMs of the heads: split-K over the chip
        if need:
            ws = _workspace("lin_splitk", need, a.device)
            _check(lib().modcr_linear_splitk_fwd(_ptr(a2), lda, _ptr(w), w.stride(0), _ptr(bias), _ptr(out), out.stride(0), m, n, k,
                                                 act, od, _ptr(ws), need, _stream()), "modcr_linear_splitk_fwd")
            return out.view(*a.shape[:-1], n) if (a.dim() != 2) else out
    _check(lib().modcr_linear_fwd(_ptr(a2), lda, _ptr(w), w.stride(0), _ptr(bias), _ptr(res2), n,
                                  dt_of(res2) if res2 is not None else 0, _ptr(out), out.stride(0), m, n,
                                  k, act, dt, od, _stream()), "modcr_linear_fwd")
    return out.view(*a.shape[:-1], n) if (a.dim() != 2) else out


LinearRoute = collections.namedtuple("LinearRoute", "kernel direct spec ngroup rev_walk")


def linear_route(a, w, bias=None, residual=None, out_dtype=None, act=ACT_NONE, lda=None, ldw=None, ldc=None, ldr=None, out=None,
                 dtype=None, res_dtype=None):
    """The route modcr_linear_fwd takes for these arguments (modcr_linear_route; nothing is launched or read):
    LinearRoute(kernel = a name of ROUTE_KERNELS, direct, spec = epilogue bits, ngroup = column tiles per group of the
    persistent 256 x 256 walk, rev_walk).  a [M, K] and w [N, K] tensors, or (rows, cols) tuples for a shape-only query
    (give `dtype`); a shape-only bias / residual / out is any non-tensor truthy value.  Non-tensors stand for 256-byte
    aligned allocations.  Strides default to a's / w's / out's row stride, the dense row otherwise."""
    def ptr_ld(t):
        if isinstance(t, torch.Tensor):
            return t.data_ptr(), t.stride(0) if t.dim() == 2 else t.shape[-1]
        return (256 if t else None), None
    m, k = (a.shape[0], a.shape[-1]) if isinstance(a, torch.Tensor) else a
    n = w.shape[0] if isinstance(w, torch.Tensor) else w[0]
    dt = dt_of(w) if isinstance(w, torch.Tensor) else (BF16 if dtype is None else dtype)
    od = dt if out_dtype is None else out_dtype
    (pa, sa), (pw, sw), (pb, _), (pr, sr), (pc, sc) = map(ptr_ld, (a, w, bias, residual, 1 if out is None else out))
    rdt = dt_of(residual) if isinstance(residual, torch.Tensor) else (res_dtype or 0)
    info = (_i32 * 4)()
    _check(lib().modcr_linear_route(pa, lda or sa or k, pw, ldw or sw or k, pb, pr, ldr or sr or n, rdt, pc, ldc or sc or n,
                                    m, n, k, act, dt, od, info), "modcr_linear_route")
    return LinearRoute(ROUTE_KERNELS[info[0]], int(bool(info[1] & ROUTE_DIRECT)), int(bool(info[1] & ROUTE_SPEC)), info[2], info[3])


BwdWeightRoute = collections.namedtuple("BwdWeightRoute", "form splits kps product direct_out reduction db")
BwdInputRoute = collections.namedtuple("BwdInputRoute", "form cast_pad inner")


def _route_ptr(t):
    """a tensor's address; a non-tensor stands for a 256-byte aligned allocation (truthy) or NULL"""
    return t.data_ptr() if isinstance(t, torch.Tensor) else (256 if t else None)


def linear_bwd_weight_route(m, n, k, dy_dtype=BF16, dtype=BF16, db=True, accumulate=False, workspace_bytes=None, lddy=None, ldx=None,
                            dy=True, x=True, dw=True, workspace=True):
    """The route modcr_linear_bwd_weight takes for dW [n, k] (+)= dY [m, n]^T . X [m, k] (modcr_linear_bwd_weight_route; nothing is
    launched or read): BwdWeightRoute(form = a name of BWD_WEIGHT_FORMS, splits, kps = 64-token K-tiles per split, product = a name
    of BWD_PRODUCTS, direct_out, reduction = a name of BWD_REDUCTIONS, db = a name of BWD_DB_METHODS).  Shapes, not tensors, so it
    runs without a GPU: dy / x / dw / db / workspace are tensors (their addresses) or truthy for a 256-byte aligned allocation.
    workspace_bytes: None = what modcr_linear_bwd_weight_workspace asks for, 0 = no workspace."""
    if workspace_bytes is None:
        workspace_bytes = lib().modcr_linear_bwd_weight_workspace(m, n, k)
    info = (_i32 * 7)()
    _check(lib().modcr_linear_bwd_weight_route(_route_ptr(dy), lddy or n, dy_dtype, _route_ptr(x), ldx or k, _route_ptr(dw), _route_ptr(db), m, n, k,
                                               int(bool(accumulate)), dtype, _route_ptr(workspace) if workspace_bytes else None, workspace_bytes,
                                               info), "modcr_linear_bwd_weight_route")
    return BwdWeightRoute(BWD_WEIGHT_FORMS[info[0]], info[1], info[2], BWD_PRODUCTS[info[3]], info[4], BWD_REDUCTIONS[info[5]],
                          BWD_DB_METHODS[info[6]])


def linear_bwd_input_route(m, n, k, dy_dtype=BF16, dtype=BF16, out_dtype=None, residual=None, workspace_bytes=None, lddy=None, ldw=None,
                           lddx=None, ldr=None, dy=True, w=True, dx=True, workspace=True):
    """The route modcr_linear_bwd_input takes for dX [m, k] = dY [m, n] . W [n, k] (+ residual, the composites' fp32 rows)
    (modcr_linear_bwd_input_route; nothing is launched or read): BwdInputRoute(form = a name of BWD_INPUT_FORMS, cast_pad,
    inner = the LinearRoute of the product behind form "fwd", None otherwise).  Arguments as linear_bwd_weight_route."""
    if workspace_bytes is None:
        workspace_bytes = lib().modcr_linear_bwd_input_workspace(m, n, k)
    info = (_i32 * 6)()
    _check(lib().modcr_linear_bwd_input_route(_route_ptr(dy), lddy or n, dy_dtype, _route_ptr(w), ldw or k, _route_ptr(residual), ldr or k,
                                              _route_ptr(dx), lddx or k, m, n, k, dtype, dtype if out_dtype is None else out_dtype,
                                              _route_ptr(workspace) if workspace_bytes else None, workspace_bytes, info),
           "modcr_linear_bwd_input_route")
    inner = None
    if BWD_INPUT_FORMS[info[0]] == "fwd":
        inner = LinearRoute(ROUTE_KERNELS[info[2]], int(bool(info[3] & ROUTE_DIRECT)), int(bool(info[3] & ROUTE_SPEC)), info[4], info[5])
    return BwdInputRoute(BWD_INPUT_FORMS[info[0]], info[1], inner)


def layernorm(x, gamma, beta, eps, residual=None, out_dtype=None, out=None, rows_per_group=0,
              group_stride=0):
    h = x.shape[-1]
    x2 = _contig(x.reshape(-1, h))
    m = x2.shape[0]
    od = dt_of(x2) if out_dtype is None else out_dtype
    ret = out
    if out is None:
        out = torch.empty((m, h), dtype=torch_dtype(od), device=x.device)
        ret = out.view(x.shape)
    r2 = _contig(residual.reshape(-1, h)) if residual is not None else None
    _check(lib().modcr_layernorm_fwd(_ptr(x2), dt_of(x2), _ptr(r2), dt_of(r2) if r2 is not None else 0,
                                     _ptr(gamma), _ptr(beta), float(eps), _ptr(out), od, m, h,
                                     rows_per_group, group_stride, _stream()), "modcr_layernorm_fwd")
    return ret


def _same_dtype(what, w, **tensors):
    """the C entries take ONE dtype code for the activations, the residual and the output: a tensor of another dtype would be read
    through the wrong element size (garbage, or reads past its end) and the C side cannot tell"""
    for name, t in tensors.items():
        if t is not None and t.dtype != w.dtype:
            raise ValueError("%s: %s is %s but the weights are %s" % (what, name, t.dtype, w.dtype))


def linear_residual_ln(a, w, bias, residual, gamma, beta, eps, workspace=None, out=None):
    """LN(a @ w.T + bias + residual): BertSelfOutput / BertOutput."""
    dt = dt_of(w)
    _same_dtype("linear_residual_ln", w, a=a, residual=residual, out=out)
    k = a.shape[-1]
    a2 = _contig(a.reshape(-1, k))
    m, n = a2.shape[0], w.shape[0]
    r2 = _contig(residual.reshape(-1, n))
    if workspace is None or workspace.numel() * workspace.element_size() < m * n * 4:
        workspace = torch.empty((m, n), dtype=torch.float32, device=a.device)
    if out is None:
        out = torch.empty((m, n), dtype=a.dtype, device=a.device)
    _check(lib().modcr_linear_residual_ln_fwd(_ptr(a2), k, _ptr(_contig(w)), _ptr(bias), _ptr(r2), _ptr(gamma),
                                              _ptr(beta), float(eps), _ptr(out), m, n, k, _ptr(workspace),
                                              workspace.numel() * workspace.element_size(), dt, _stream()),
           "modcr_linear_residual_ln_fwd")
    return out.view(*residual.shape)


def linear_dropout_residual_ln(a, w, bias, residual, gamma, beta, eps, p=0.0, seed=0, offset=0, out=None, pre_out=None, row_id=None):
    """LN(dropout(a @ w.T + bias) + residual): BertSelfOutput / BertOutput as one C-ABI call (GEMM -> IEEE-half rows -> mask +
    residual + LayerNorm pass).  p = 0: no dropout.  pre_out: fp32 or fp16 [M,N] tensor that receives the pre-LayerNorm rows.
    row_id: int32 [M] device table of the live-row layout (LiveRows): row m carries the dropout counters of row row_id[m]."""
    dt = dt_of(w)
    _same_dtype("linear_dropout_residual_ln", w, a=a, residual=residual, out=out)
    k = a.shape[-1]
    a2 = _contig(a.reshape(-1, k))
    m, n = a2.shape[0], w.shape[0]
    r2 = _contig(residual.reshape(-1, n))
    need = lib().modcr_linear_dropout_residual_ln_workspace(m, n, k, dt)
    ws = _workspace("lin_ln", need, a.device)
    if out is None:
        out = torch.empty((m, n), dtype=a.dtype, device=a.device)
    if pre_out is not None and (pre_out.dtype not in (torch.float32, torch.float16) or pre_out.numel() != m * n or not pre_out.is_contiguous()):
        raise ValueError("linear_dropout_residual_ln: pre_out must be a contiguous fp32 or fp16 [M,N] tensor")
    if row_id is not None:
        if row_id.dtype != torch.int32 or row_id.numel() < m or not row_id.is_contiguous():
            raise ValueError("linear_dropout_residual_ln: row_id must be a contiguous int32 table with an entry for each of the %d rows" % m)
        _check(lib().modcr_linear_dropout_residual_ln_rows_fwd(_ptr(a2), k, _ptr(_contig(w)), _ptr(bias), _ptr(r2), _ptr(gamma), _ptr(beta), float(eps),
                                                               _ptr(out), _ptr(pre_out), dt_of(pre_out) if pre_out is not None else F32, m, n, k, float(p),
                                                               seed, offset, _ptr(row_id), _ptr(ws), need, dt, _stream()),
               "modcr_linear_dropout_residual_ln_rows_fwd")
        return out.view(*residual.shape)
    _check(lib().modcr_linear_dropout_residual_ln_fwd(_ptr(a2), k, _ptr(_contig(w)), _ptr(bias), _ptr(r2), _ptr(gamma), _ptr(beta), float(eps),
                                                      _ptr(out), _ptr(pre_out), dt_of(pre_out) if pre_out is not None else F32, m, n, k, float(p), seed, offset,
                                                      _ptr(ws), need, dt, _stream()),
           "modcr_linear_dropout_residual_ln_fwd")
    return out.view(*residual.shape)


def pack_mask_bits(mask):
    """0/1 float mask [..., L] -> uint32 bits [..., ceil(L/32)] (as int32 storage)."""
    l = mask.shape[-1]
    m2 = _contig(mask.reshape(-1, l), torch.float32)
    bits = torch.empty((m2.shape[0], (l + 31) // 32), dtype=torch.int32, device=mask.device)
    _check(lib().modcr_pack_mask_bits(_ptr(m2), _ptr(bits), m2.shape[0], l, _stream()), "modcr_pack_mask_bits")
    return bits.view(*mask.shape[:-1], (l + 31) // 32)


def pack_factor(n, s, limit=192):
    """how many sequences of s rows share one attention row block of at most `limit` rows (a divisor of n; 1 = no packing)"""
    for k in range(limit // max(s, 1), 1, -1):
        if n % k == 0:
            return k
    return 1


def build_packed_mask(key_mask, k):
    """block-diagonal dense mask bits of k sequences per row block: key_mask [N, S] 0/1 -> bits [N / k, k S, ceil(k S / 32)]"""
    n, s = key_mask.shape
    km = _contig(key_mask, torch.float32)
    bits = torch.empty((n // k, k * s, (k * s + 31) // 32), dtype=torch.int32, device=key_mask.device)
    _check(lib().modcr_build_packed_mask(_ptr(km), _ptr(bits), n, s, k, _stream()), "modcr_build_packed_mask")
    return bits


def build_phase_mask(input_mask, chunk_mask, phase):
    n, s = input_mask.shape
    t = chunk_mask.shape[1]
    bits = torch.empty((n, s, (s + 31) // 32), dtype=torch.int32, device=input_mask.device)
    _check(lib().modcr_build_phase_mask(_ptr(_contig(input_mask, torch.float32)),
                                        _ptr(_contig(chunk_mask, torch.float32)), _ptr(bits), n, t, s - t,
                                        phase, _stream()), "modcr_build_phase_mask")
    return bits


ATTN_SIDE_POST_DROPOUT = 1      # include/modcr_hip.h: MODCR_ATTN_SIDE_POST_DROPOUT
# keys (P + S) the attention forward takes: the tile kernels up to 256, the streaming core of csrc/attn_long.hip above (eval
# mode only: no attention-probability dropout, no row statistics, no backward)
ATTN_TILE_KEYS = 256
ATTN_MAX_KEYS = 512
# keys up to which the opt-in wide dropout counter layout (csrc/attn_common.h: row stride 512 above 256 keys) carries the
# attention-probability dropout: qkv_attn(wide_dropout=True) / qkv_attn_long_bwd(wide_dropout=True)
ATTN_DROPOUT_WIDE_MAX_KEYS = 512
# keys up to which the opt-in dense mask bits on the bias route and the align map's gradient are served above 256 keys:
# qkv_attn(dense_bits=) / qkv_attn_long_bwd(dense_bits=, d_align=) (modcr_qkv_attn_long_align_fwd / _bwd; no prefix rows)
ATTN_LONG_ALIGN_MAX_KEYS = 512


def qkv_attn(x, wqkv, bqkv, key_mask=None, mask_bits=None, hist=None, chunk_id=None, want_probs=False,
             align_map=None, align_t=0, num_heads=None, workspace=None, out=None, attn_dropout=None, lse=None, dump=None,
             side_post_dropout=False, attn_bias=None, head_mask=None, row_start=None, wide_dropout=False, dense_bits=None):
    """Fused QKV projection + attention.  x [N,S,H]; returns (ctx [N,S,H], probs or None).
    row_start: int32 [N+1] device table of the live-row layout (LiveRows; modcr_qkv_attn_rows_fwd): x and ctx are [N,S,H] BUFFERS
    whose first row_start[N] rows hold the sequences' live rows back to back.  No hist / probs / lse / dump / attn_bias there; a
    shape the entry does not serve raises (ask qkv_attn_route(..., rows=True) first).
    attn_bias: any float tensor broadcastable to [N, A, S, P+S], ADDED to the scores before the softmax (the reference's additive
    attention_mask, soft biases, -inf entries); head_mask: [A], [1,A,1,1], [N,A] or [N,A,1,1], multiplies the probabilities of a
    head after softmax and dropout.  Either one sends the call to modcr_qkv_attn_bias_fwd (the streaming core with a float bias,
    P + S <= 512, dropout up to 256 keys); they replace key_mask / mask_bits and do not combine with lse / dump.
    wide_dropout (that route only): the call goes to modcr_qkv_attn_long_drop_fwd, which carries the dropout on to 512 keys under the
    wide counter layout; at P + S <= 256 or without dropout it changes nothing.
    dense_bits (that route only, and by itself it selects the route): int32 [N, S, ceil(S / 32)] dense mask bits (build_phase_mask /
    pack_mask_bits) read ON TOP of attn_bias, a clear bit = -10000 -- modcr_qkv_attn_long_align_fwd, 256 < S <= 512, no hist; the
    backward is qkv_attn_long_bwd(dense_bits=).  mask_bits keeps its meaning: the binary route, never together with attn_bias.
    attn_dropout = (p, seed, offset): training-mode dropout of the attention probabilities.
    side_post_dropout: probs / align_map are the probabilities AFTER that dropout, P o m / (1 - p), as the reference's modules
    return them (modeling_bert.py:69-74); default: the un-dropped ones (and no probs output under dropout).
    lse: fp32 [N, A, S] tensor that receives the row statistics qkv_attn_bwd(ctx=, lse=) wants (tile-kernel shapes only:
    lse_supported); dump: bf16 tensor of qkv_dump_numel(N, S, A) elements that receives the Q | K | V images (with lse)."""
    dt = dt_of(x)
    x = _contig(x)
    n, s, h = x.shape
    a = num_heads
    if row_start is not None:
        if hist is not None or want_probs or lse is not None or dump is not None or attn_bias is not None or head_mask is not None:
            raise ValueError("qkv_attn: the live-row layout takes no hist, probabilities, lse, dump, attn_bias or head_mask")
        if row_start.dtype != torch.int32 or row_start.numel() != n + 1 or not row_start.is_contiguous():
            raise ValueError("qkv_attn: row_start must be a contiguous int32 [N + 1] tensor")
        ctx = torch.empty_like(x) if out is None else out
        km = _contig(key_mask, torch.float32) if key_mask is not None else None
        ap, seed, off = attn_dropout if attn_dropout is not None else (0.0, 0, 0)
        _check(lib().modcr_qkv_attn_rows_fwd(_ptr(x), _ptr(_contig(wqkv)), _ptr(bqkv), _ptr(km), _ptr(mask_bits), _ptr(chunk_id),
                                             0 if chunk_id is None else chunk_id.shape[1], _ptr(ctx), _ptr(align_map), align_t, _ptr(row_start),
                                             n, s, h, a, float(ap), seed, off, ATTN_SIDE_POST_DROPOUT if side_post_dropout else 0, dt, _stream()),
               "modcr_qkv_attn_rows_fwd")
        return ctx, None
    p = 0 if hist is None else hist.shape[1]
    if p + s > ATTN_MAX_KEYS:
        raise ValueError("qkv_attn: P + S = %d keys exceeds the %d-key limit of the attention forward" % (p + s, ATTN_MAX_KEYS))
    if wide_dropout and attn_bias is None and head_mask is None and dense_bits is None:
        raise ValueError("qkv_attn: wide_dropout belongs to the attn_bias / head_mask route (fold a binary key mask with fold_key_mask)")
    if attn_bias is not None or head_mask is not None or dense_bits is not None:
        if key_mask is not None or mask_bits is not None:
            raise ValueError("qkv_attn: attn_bias / head_mask replace key_mask / mask_bits (fold a binary mask into the bias as 0 / -10000)")
        if lse is not None or dump is not None:
            raise ValueError("qkv_attn: no row statistics (lse) / q|k|v dump on the attn_bias / head_mask route (forward only)")
        return _qkv_attn_bias(x, wqkv, bqkv, attn_bias, head_mask, hist, chunk_id, want_probs, align_map, align_t, a, workspace, out,
                              attn_dropout, side_post_dropout, wide_dropout, dense_bits)
    if (dt == BF16 and attn_dropout is not None and attn_dropout[0] > 0.0 and side_post_dropout and (want_probs or align_map is not None)
            and not side_outputs_on_tiles(s, p, h, a)):
        # post-dropout side outputs are served by the bf16 TILE kernels only (modcr_qkv_attn_opt_fwd returns MODCR_ERR_UNSUPPORTED on
        # the older kernel's shapes: P + S <= 64, odd head counts below 193 rows, H not a multiple of 128, prefix rows): such a call
        # takes the exact-fp32 route, which carries the same mask at any length <= 256, and hands the context back in bf16
        if lse is not None or dump is not None:
            raise ValueError("qkv_attn: no row statistics on the exact-fp32 route this shape takes (S=%d P=%d A=%d H=%d)" % (s, p, a, h))
        ctx32, probs = qkv_attn(x.float(), wqkv.float(), bqkv, key_mask=key_mask, mask_bits=mask_bits,
                                hist=None if hist is None else hist.float(), chunk_id=chunk_id, want_probs=want_probs,
                                align_map=align_map, align_t=align_t, num_heads=a, attn_dropout=attn_dropout, side_post_dropout=True)
        if out is None:
            return ctx32.to(torch.bfloat16), probs
        out.copy_(ctx32)
        return out, probs
    hist = _contig(hist)
    ctx = torch.empty_like(x) if out is None else out
    probs = torch.empty((n, a, s, p + s), dtype=torch.float32, device=x.device) if want_probs else None
    need = lib().modcr_qkv_attn_workspace(n, s, p, h, dt)
    if need and (workspace is None or workspace.numel() * workspace.element_size() < need):
        workspace = torch.empty((need // 4,), dtype=torch.float32, device=x.device)
    km = _contig(key_mask, torch.float32) if key_mask is not None else None
    chunk_t = 0 if chunk_id is None else chunk_id.shape[1]
    ap, seed, off = attn_dropout if attn_dropout is not None else (0.0, 0, 0)
    if lse is not None and (lse.dtype != torch.float32 or tuple(lse.shape) != (n, a, s) or not lse.is_contiguous()):
        raise ValueError("qkv_attn: lse must be a contiguous fp32 [N, A, S] tensor")
    if dump is not None and (dump.dtype != torch.bfloat16 or dump.numel() != qkv_dump_numel(n, s, a) or not dump.is_contiguous() or lse is None):
        raise ValueError("qkv_attn: dump must be a contiguous bf16 tensor of qkv_dump_numel(N, S, A) elements, given together with lse")
    _check(lib().modcr_qkv_attn_opt_fwd(_ptr(x), _ptr(hist), _ptr(_contig(wqkv)), _ptr(bqkv), _ptr(km), _ptr(mask_bits),
                                        _ptr(chunk_id), chunk_t, _ptr(ctx), _ptr(probs), _ptr(align_map), align_t, _ptr(lse), _ptr(dump),
                                        n, s, p, h, a, float(ap), seed, off, ATTN_SIDE_POST_DROPOUT if side_post_dropout else 0,
                                        _ptr(workspace) if need else None, need, dt, _stream()),
           "modcr_qkv_attn_fwd")
    return ctx, probs


def _bias_strides(attn_bias, n, a, s, l):
    """attn_bias -> (fp32 tensor with unit key stride, element strides over sequence / head / query; 0 = broadcast).  Strides are
    taken from the tensor as it is (an expand()ed view stays a view); only a non-unit key stride or another dtype makes a copy."""
    b = attn_bias
    if not b.is_floating_point():
        raise ValueError("qkv_attn: attn_bias must be a float tensor, got %s" % b.dtype)
    if b.dim() > 4:
        raise ValueError("qkv_attn: attn_bias has %d dimensions, want at most 4 ([N, A, S, L])" % b.dim())
    b = b.reshape((1,) * (4 - b.dim()) + tuple(b.shape)) if b.dim() < 4 else b
    for d, full in enumerate((n, a, s)):
        if b.shape[d] not in (1, full):
            raise ValueError("qkv_attn: attn_bias %s does not broadcast to [N=%d, A=%d, S=%d, L=%d]" % (tuple(attn_bias.shape), n, a, s, l))
    if b.shape[3] != l:
        raise ValueError("qkv_attn: attn_bias %s: the key dimension must be P + S = %d" % (tuple(attn_bias.shape), l))
    if b.dtype != torch.float32:
        b = b.to(torch.float32)
    if l > 1 and b.stride(3) != 1:
        b = b.contiguous()
    return b, [0 if b.shape[d] == 1 else b.stride(d) for d in range(3)]


def _head_mask_2d(head_mask, n, a):
    """head_mask [A], [1,A,1,1], [N,A] or [N,A,1,1] -> (contiguous fp32 [1 or N, A], sequence stride in elements)"""
    hm = head_mask
    if hm.dim() == 4 and hm.shape[2] == 1 and hm.shape[3] == 1:
        hm = hm.reshape(hm.shape[0], hm.shape[1])
    elif hm.dim() == 1:
        hm = hm.reshape(1, -1)
    if hm.dim() != 2 or hm.shape[1] != a or hm.shape[0] not in (1, n):
        raise ValueError("qkv_attn: head_mask %s is not [A], [1,A,1,1], [N,A] or [N,A,1,1] (N=%d, A=%d)" % (tuple(head_mask.shape), n, a))
    hm = _contig(hm, torch.float32)
    return hm, (0 if hm.shape[0] == 1 else a)


def _dense_bits(bits, who, n, s):
    """dense mask bits of the bias route: a contiguous int32 [N, S, ceil(S / 32)] tensor (build_phase_mask / pack_mask_bits), as it is"""
    if bits.dtype != torch.int32 or tuple(bits.shape) != (n, s, (s + 31) // 32) or not bits.is_contiguous():
        raise ValueError("%s: dense_bits must be a contiguous int32 [N, S, ceil(S / 32)] = [%d, %d, %d] tensor, got %s %s" %
                         (who, n, s, (s + 31) // 32, tuple(bits.shape), bits.dtype))
    return bits


def _qkv_attn_bias(x, wqkv, bqkv, attn_bias, head_mask, hist, chunk_id, want_probs, align_map, align_t, a, workspace, out, attn_dropout,
                   side_post_dropout, wide_dropout=False, dense_bits=None):
    """qkv_attn with attn_bias / head_mask: modcr_qkv_attn_bias_fwd, or with wide_dropout modcr_qkv_attn_long_drop_fwd, or with
    dense_bits modcr_qkv_attn_long_align_fwd (the drop entry's arguments, then the bits)"""
    dt = dt_of(x)
    n, s, h = x.shape
    p = 0 if hist is None else hist.shape[1]
    l = p + s
    ap, seed, off = attn_dropout if attn_dropout is not None else (0.0, 0, 0)
    if ap > 0.0 and l > ATTN_TILE_KEYS and not wide_dropout:
        raise ValueError("qkv_attn: attention-probability dropout with attn_bias / head_mask stops at %d keys (P + S = %d)" % (ATTN_TILE_KEYS, l))
    bias, (bsn, bsa, bsq) = (None, (0, 0, 0)) if attn_bias is None else _bias_strides(attn_bias, n, a, s, l)
    hm, hsn = (None, 0) if head_mask is None else _head_mask_2d(head_mask, n, a)
    hist = _contig(hist)
    ctx = torch.empty_like(x) if out is None else out
    probs = torch.empty((n, a, s, l), dtype=torch.float32, device=x.device) if want_probs else None
    need = lib().modcr_qkv_attn_bias_workspace(n, s, p, h, dt)
    if workspace is None or workspace.numel() * workspace.element_size() < need:
        workspace = torch.empty(((need + 3) // 4,), dtype=torch.float32, device=x.device)
    chunk_t = 0 if chunk_id is None else chunk_id.shape[1]
    entry = "modcr_qkv_attn_long_align_fwd" if dense_bits is not None else "modcr_qkv_attn_long_drop_fwd" if wide_dropout else "modcr_qkv_attn_bias_fwd"
    more = () if dense_bits is None else (_ptr(_dense_bits(dense_bits, "qkv_attn", n, s)),)
    _check(getattr(lib(), entry)(_ptr(x), _ptr(hist), _ptr(_contig(wqkv)), _ptr(bqkv), _ptr(bias), bsn, bsa, bsq, _ptr(hm), hsn,
                                 _ptr(chunk_id), chunk_t, _ptr(ctx), _ptr(probs), _ptr(align_map), align_t, n, s, p, h, a,
                                 float(ap), seed, off, ATTN_SIDE_POST_DROPOUT if side_post_dropout else 0,
                                 _ptr(workspace), need, dt, _stream(), *more),
           entry)
    return ctx, probs


def additive_mask_is_binary(mask):
    """True iff every element of the additive mask is 0 or -10000 -- what the binary routes (key mask / dense mask bits) compute
    exactly.  One reduction and one host read; CPU tensors work too."""
    return bool(((mask == 0) | (mask == -10000.0)).all().item())


# modcr_qkv_attn_route: kernel families (MODCR_ATTN_ROUTE_*) and the bits of `present` (MODCR_ATTN_HAS_*)
ATTN_ROUTE_FAMILIES = {1: "tile", 2: "tile4", 3: "long_bf16", 4: "f32", 5: "long_f32"}
ATTN_HAS_BIAS, ATTN_HAS_DENSE_MASK, ATTN_HAS_CHUNK_ID, ATTN_HAS_PROBS, ATTN_HAS_ALIGN_MAP, ATTN_HAS_LSE, ATTN_HAS_QKV_DUMP = 1, 2, 4, 8, 16, 32, 64
ATTN_HAS_ROW_START = 128
AttnRoute = collections.namedtuple("AttnRoute", "rc family inst concat message")


def qkv_attn_route(n, s, p, h, a, dtype=BF16, bias=False, dense=False, chunk_t=0, probs=False, align_t=0, lse=False, dump=False,
                   attn_p=0.0, flags=0, workspace_bytes=None, workspace_aligned=True, rows=False):
    """The route the attention forward takes for these arguments (modcr_qkv_attn_route; nothing is launched or read):
    AttnRoute(rc = the call's return code, family = a name of ATTN_ROUTE_FAMILIES, inst = the five numbers that pick the
    instantiation, concat, message = the refusal's text).  bias: the call goes to modcr_qkv_attn_bias_fwd; chunk_t / align_t > 0:
    chunk_id / align_map are given; workspace_bytes None: what qkv_attn supplies for the shape; rows: the call is
    modcr_qkv_attn_rows_fwd (the live-row layout)."""
    present = ((ATTN_HAS_BIAS if bias else 0) | (ATTN_HAS_DENSE_MASK if dense else 0) | (ATTN_HAS_CHUNK_ID if chunk_t else 0) |
               (ATTN_HAS_PROBS if probs else 0) | (ATTN_HAS_ALIGN_MAP if align_t else 0) | (ATTN_HAS_LSE if lse else 0) |
               (ATTN_HAS_QKV_DUMP if dump else 0) | (ATTN_HAS_ROW_START if rows else 0))
    if workspace_bytes is None:
        workspace_bytes = (lib().modcr_qkv_attn_bias_workspace if bias else lib().modcr_qkv_attn_workspace)(n, s, p, h, dtype)
    info = (_i32 * 7)()
    rc = lib().modcr_qkv_attn_route(present, chunk_t, align_t, n, s, p, h, a, float(attn_p), flags, workspace_bytes,
                                    1 if workspace_aligned else 0, dtype, info)
    if rc != 0:
        return AttnRoute(rc, None, None, None, lib().modcr_last_error().decode())
    return AttnRoute(0, ATTN_ROUTE_FAMILIES[info[0]], tuple(info[1:6]), info[6], "")


def side_outputs_on_tiles(s, p, h, a):
    """shapes on which the bf16 TILE kernels serve a post-dropout probabilities output / align map: what the dispatcher of
    modcr_qkv_attn_opt_fwd answers for that call (64 < S <= 256 without prefix rows, H = 64 A a multiple of 128, head pairs up to
    192 rows, one head per workgroup above).  Asked with a probabilities output; an align map alone gets the same answer, since
    either one keeps prefix rows off the tile kernels and lands on the same generic tile variant.  Needs the built library, and a
    False answer leaves the refusal's text in modcr_last_error."""
    r = qkv_attn_route(1, s, p, h, a, probs=True, attn_p=0.5, flags=ATTN_SIDE_POST_DROPOUT)
    return r.rc == 0 and r.family == "tile4"


def qkv_dump_numel(n, s, a):
    """bf16 elements of qkv_attn's `dump` output: [N][A][3][LP][64]"""
    return lib().modcr_qkv_attn_dump_bytes(n, s, a) // 2


def lse_supported(x, num_heads, hist=None):
    """shapes on which qkv_attn runs a tile kernel (the ones that can write the row statistics `lse`)"""
    n, s, h = x.shape
    return (x.dtype == torch.bfloat16 and hist is None and 64 < s <= 192 and num_heads % 2 == 0 and h % 128 == 0 and h >= 256
            and h == num_heads * 64)


def embed_ln(input_ids, token_type_ids, position_ids, word, pos, typ, gamma, beta, eps, out, seq_stride, dropout=None):
    """dropout = (p, seed, offset): BertEmbeddings.dropout on the rows written, counters = flat indices of `out` [N, seq_stride, H]"""
    n, t = input_ids.shape
    h = word.shape[1]
    p, seed, off = dropout if dropout is not None else (0.0, 0, 0)
    _check(lib().modcr_embed_ln_dropout_fwd(_ptr(_contig(input_ids)), _ptr(_contig(token_type_ids)),
                                            _ptr(_contig(position_ids)), _ptr(word), _ptr(pos), _ptr(typ), _ptr(gamma),
                                            _ptr(beta), float(eps), _ptr(out), n, t, h, seq_stride, word.shape[0],
                                            pos.shape[0], typ.shape[0], dt_of(out), float(p), seed, off, _stream()), "modcr_embed_ln_dropout_fwd")
    return out


def rows_scatter_dropout(src, dst, row0, dropout=None):
    """src [N*R, H] -> dst[:, row0:row0+R] of the contiguous dst [N, S, H] under nn.Dropout (dropout = (p, seed, offset), None = plain
    copy); counters = flat indices of dst, so together with embed_ln(..., dropout=) the buffer carries the mask of ONE dropout call over it."""
    n, s, h = dst.shape
    assert dst.is_contiguous() and src.is_contiguous() and src.dtype == dst.dtype and src.numel() % (n * h) == 0
    r = src.numel() // (n * h)
    assert row0 + r <= s
    p, seed, off = dropout if dropout is not None else (0.0, 0, 0)
    _check(lib().modcr_rows_scatter_dropout(_ptr(src), _ptr(dst), n * r, h, r, s, row0, dt_of(dst), float(p), seed, off, _stream()),
           "modcr_rows_scatter_dropout")
    return dst


def embed_ln_rows(input_ids, token_type_ids, position_ids, word, pos, typ, gamma, beta, eps, out, seq_stride, row_start, dropout=None):
    """embed_ln into the live-row layout: row t of sequence n -> row row_start[n] + t of out [rows, H]; dropout counters = flat
    indices of the padded [N, seq_stride, H] buffer (modcr_embed_ln_dropout_rows_fwd)"""
    n, t = input_ids.shape
    h = word.shape[1]
    assert out.dim() == 2 and out.is_contiguous() and row_start.dtype == torch.int32 and row_start.numel() >= n
    p, seed, off = dropout if dropout is not None else (0.0, 0, 0)
    _check(lib().modcr_embed_ln_dropout_rows_fwd(_ptr(_contig(input_ids)), _ptr(_contig(token_type_ids)),
                                                 _ptr(_contig(position_ids)), _ptr(word), _ptr(pos), _ptr(typ), _ptr(gamma),
                                                 _ptr(beta), float(eps), _ptr(out), n, t, h, seq_stride, word.shape[0],
                                                 pos.shape[0], typ.shape[0], dt_of(out), float(p), seed, off, _ptr(row_start), out.shape[0],
                                                 _stream()), "modcr_embed_ln_dropout_rows_fwd")
    return out


def rows_place_dropout(src, dst, row_id, r, s, row0, dropout=None, src_start=None):
    """the region rows of a live-row layout (modcr_rows_place_dropout): dst [M, H] compact rows, row_id int32 [M] their rows in the
    padded [N, s, H] buffer; region j of sequence g comes from src row g r + j (src_start None) or src_start[g] + j.  Text rows
    (p % s < row0) are left alone, filler rows (row_id < 0) are zeroed.  dropout = (p, seed, offset): counters of the padded buffer."""
    m, h = dst.shape
    assert dst.is_contiguous() and src.is_contiguous() and src.dim() == 2 and src.dtype == dst.dtype and src.shape[1] == h
    assert row_id.dtype == torch.int32 and row_id.is_contiguous() and row_id.numel() == m and row0 + r <= s
    assert src_start is None or (src_start.dtype == torch.int32 and src_start.is_contiguous())
    groups = src.shape[0] // r if src_start is None else src_start.numel() - 1      # (src_start = a row_start table [N + 1])
    p, seed, off = dropout if dropout is not None else (0.0, 0, 0)
    _check(lib().modcr_rows_place_dropout(_ptr(src), src.shape[0], _ptr(dst), _ptr(row_id), _ptr(src_start), groups, m, h, r, s, row0, dt_of(dst),
                                          float(p), seed, off, _stream()), "modcr_rows_place_dropout")
    return dst


def cast_pad_rows(src, kp, src_row):
    """fp32 [rows, K] -> bf16 [M, kp]: row m = the zero-padded cast of src row src_row[m] (int32 [M]; outside the source: zeros)"""
    k = src.shape[-1]
    s2 = _contig(src.reshape(-1, k), torch.float32)
    assert src_row.dtype == torch.int32 and src_row.is_contiguous()
    dst = torch.empty((src_row.numel(), kp), dtype=torch.bfloat16, device=src.device)
    _check(lib().modcr_cast_pad_rows(_ptr(s2), k, s2.shape[0], _ptr(dst), kp, dst.shape[0], k, kp, _ptr(src_row), _stream()), "modcr_cast_pad_rows")
    return dst


def rows_take(src, idx, out=None):
    """out[i] = src[idx[i]] over rows (modcr_rows_take): src [rows, H] contiguous bf16 / fp32, idx int32 [M] on the device; an index
    outside [0, rows) gives a zero row.  out: contiguous [M, H] (default: a new tensor)."""
    assert src.dim() == 2 and src.is_contiguous() and idx.dtype == torch.int32 and idx.is_contiguous()
    m, h = idx.numel(), src.shape[1]
    if out is None:
        out = torch.empty((m, h), dtype=src.dtype, device=src.device)
    assert out.is_contiguous() and out.dtype == src.dtype and out.numel() == m * h
    _check(lib().modcr_rows_take(_ptr(src), src.shape[0], _ptr(out), _ptr(idx), m, h, dt_of(src), _stream()), "modcr_rows_take")
    return out


# ---- the live-row layout of a frozen encoder pass (include/modcr_hip.h: modcr_qkv_attn_rows_fwd) ----------------------------------
LIVE_ROW_ALIGN = 256     # launches use the live-row count rounded up to this (the fast GEMM routes need M % 256 == 0), capped at the capacity

LiveLayout = collections.namedtuple("LiveLayout", "seq_len m_live m_launch capacity row_start row_id take")
# one layout before its tables are on a device: the LiveLayout fields, with every table as an (offset, length) slice of LiveRows.host
_LayoutSpec = collections.namedtuple("_LayoutSpec", "seq_len m_live m_launch capacity row_start row_id take")


def _round_rows(m, capacity):
    return min((m + LIVE_ROW_ALIGN - 1) // LIVE_ROW_ALIGN * LIVE_ROW_ALIGN, capacity)


class LiveRows(object):
    """Host-built tables of the live-row layout for one batch of N sequences of T text rows + R region slots of which sequence n
    fills the first nreg[n] (input_mask[n, T:T+R] = 1...1 0...0).  Four layouts, each a LiveLayout of int32 tables:
      full  one [text | regions] pass: L_n = T + nreg[n] rows of S = T + R (all S rows where nreg[n] = 0: see `_pass_rows`)
      img   the image-only [CLS | regions] pass: L_n = 1 + nreg[n] rows of S = 1 + R
      pair  BertImgModel.forward_pair's buffer of N (T + R) + N (1 + R) rows: the full pass's live rows, then the image-only pass's
      reg   the region rows the region pipeline computes, back to back: the first (L_n of full) - T of the R slots of sequence n
    row_start [N + 1]: first compact row of every sequence (full / img: relative to the pass's first row; pair has none);
    row_id [m_launch]: the flat row of the padded buffer each compact row stands for (-1 for the filler rows up to m_launch; reg:
    the row of the [N R, D] region features);
    take[k] [N k]: the compact row of (n, j), j < k -- k = T (the text rows the heads read) and k = 1 ([CLS]); pair: take[T] and
    take[1] address the full pass, take["img"] [N] the image-only pass's [CLS] rows.
    All tables are slices of ONE int32 array (`host`, numpy), copied to the device once (`to`): no device -> host traffic."""

    def __init__(self, nreg, t, r):
        import numpy as np
        nreg = np.asarray(nreg, dtype=np.int64).reshape(-1)
        n = int(nreg.shape[0])
        if n == 0 or t < 1 or r < 1 or nreg.min() < 0 or nreg.max() > r:
            raise ValueError("LiveRows: need N > 0 region counts in [0, R] (T=%d, R=%d)" % (t, r))
        if n * (t + r) + n * (1 + r) >= 2 ** 31:
            raise ValueError("LiveRows: the row tables are int32")
        self.n, self.t, self.r, self.nreg = n, int(t), int(r), nreg
        self._parts, self._specs = [], {}
        rs_full, rid_full = self._pass_rows(t)
        rs_img, rid_img = self._pass_rows(1)
        m_full, m_img = int(rs_full[n]), int(rs_img[n])
        take_t = (rs_full[:n, None] + np.arange(t)[None, :]).reshape(-1)
        full = self._add("full", t + r, m_full, n * (t + r), rs_full, rid_full, {t: take_t, 1: rs_full[:n]})
        self._add("img", 1 + r, m_img, n * (1 + r), rs_img, rid_img, {1: rs_img[:n]})
        pair = self._add("pair", t + r, m_full + m_img, n * (t + r) + n * (1 + r), None, np.concatenate([rid_full, n * (t + r) + rid_img]),
                         {"img": m_full + rs_img[:n]})
        pair.take.update({t: full.take[t], 1: full.take[1]})
        # the region rows of the full pass's layout (it keeps at least the image-only pass's regions of every sequence)
        lreg = np.diff(rs_full) - t
        rs_reg = np.zeros(n + 1, np.int64)
        rs_reg[1:] = np.cumsum(lreg)
        seq = np.repeat(np.arange(n, dtype=np.int64), lreg)
        self._add("reg", r, int(rs_reg[n]), n * r, rs_reg, seq * r + (np.arange(int(rs_reg[n]), dtype=np.int64) - rs_reg[seq]), {})
        self.host = np.concatenate(self._parts)
        del self._parts
        self.blob = None
        self.full = self.img = self.pair = self.reg = None

    def _pass_rows(self, k_text):
        """(row_start, row_id) of one pass over [k_text text rows | R region slots].
        A [text | regions] sequence WITHOUT a live region keeps all its rows: under the phase masks a text row whose chunk-mask row is
        empty (padded text) then has every key hidden, its softmax is the uniform one over all S keys -- padded regions included --
        and padded text rows are read by the heads.  (With a live region such a row sees exactly the live regions; the image-only
        pass always has [CLS] as a live key.)"""
        import numpy as np
        n, r, nreg = self.n, self.r, self.nreg
        ln = k_text + (np.where(nreg == 0, r, nreg) if k_text > 1 else nreg)
        rs = np.zeros(n + 1, np.int64)
        rs[1:] = np.cumsum(ln)
        seq = np.repeat(np.arange(n, dtype=np.int64), ln)
        return rs, seq * (k_text + r) + (np.arange(int(rs[n]), dtype=np.int64) - rs[seq])

    def _put(self, a):
        import numpy as np
        off = sum(p_.shape[0] for p_ in self._parts)
        self._parts.append(np.ascontiguousarray(a, dtype=np.int32).reshape(-1))
        return (off, self._parts[-1].shape[0])

    def _add(self, name, seq_len, m_live, capacity, row_start, row_id, take):
        import numpy as np
        m_launch = _round_rows(m_live, capacity)
        rid = np.full(m_launch, -1, np.int64)
        rid[:m_live] = row_id
        spec = _LayoutSpec(seq_len, m_live, m_launch, capacity, None if row_start is None else self._put(row_start), self._put(rid),
                           {k: self._put(v) for k, v in take.items()})
        self._specs[name] = spec
        return spec

    def to(self, device, non_blocking=True):
        """copies the tables to `device` (one transfer, from pinned memory when that is a GPU, so that it does not hold the host)
        and builds the LiveLayouts over the device array; returns self"""
        host = torch.from_numpy(self.host)
        if torch.device(device).type == "cuda":
            host = host.pin_memory()
        self.blob = host.to(device, non_blocking=non_blocking)
        cut = lambda ol: None if ol is None else self.blob[ol[0]:ol[0] + ol[1]]
        for name, sp in self._specs.items():
            setattr(self, name, LiveLayout(sp.seq_len, sp.m_live, sp.m_launch, sp.capacity, cut(sp.row_start), cut(sp.row_id),
                                           {k: cut(v) for k, v in sp.take.items()}))
        return self

    def matches(self, n, t, r, device):
        return self.blob is not None and (self.n, self.t, self.r) == (n, t, r) and self.blob.device == device

    @property
    def dead_rows(self):
        return self._specs["pair"].capacity - self._specs["pair"].m_live


def live_rows_from_mask(input_mask, t):
    """LiveRows of a HOST input_mask [N, T + R] (0/1), or None when the layout does not apply: a device tensor (reading it would
    stall the stream), no region columns, a region part that is not in prefix form 1...1 0...0, or a dead [CLS] (then a query row
    could have every key hidden, and the padded route's uniform softmax over padded keys would matter)."""
    if not torch.is_tensor(input_mask) or input_mask.is_cuda or input_mask.dim() != 2 or input_mask.shape[1] <= t or t < 1:
        return None
    m = input_mask.detach().to(torch.float32).numpy()
    img = m[:, t:]
    nreg = (img != 0).sum(axis=1)
    import numpy as np
    want = (np.arange(img.shape[1])[None, :] < nreg[:, None]).astype(np.float32)
    if not np.array_equal(img, want) or not np.all(m[:, 0] == 1):
        return None
    return LiveRows(nreg, t, img.shape[1])


def cast_pad(src, kp, dtype):
    k = src.shape[-1]
    s2 = _contig(src.reshape(-1, k), torch.float32)
    dst = torch.empty((s2.shape[0], kp), dtype=torch_dtype(dtype), device=src.device)
    _check(lib().modcr_cast_pad(_ptr(s2), k, _ptr(dst), kp, s2.shape[0], k, kp, dtype, _stream()), "modcr_cast_pad")
    return dst


def split3(src, mode):
    """fp32 [M,K] -> bf16 [M,3K]: mode 0 = [hi|lo|hi] (activations), 1 = [hi|hi|lo] (weights)."""
    src = _contig(src, torch.float32)
    m, k = src.shape
    dst = torch.empty((m, 3 * k), dtype=torch.bfloat16, device=src.device)
    _check(lib().modcr_split3_bf16(_ptr(src), k, _ptr(dst), 3 * k, m, k, mode, _stream()), "modcr_split3_bf16")
    return dst


def convert(src, dtype):
    src = _contig(src)
    dst = torch.empty(src.shape, dtype=torch_dtype(dtype), device=src.device)
    _check(lib().modcr_convert(_ptr(src), dt_of(src), _ptr(dst), dtype, src.numel(), _stream()), "modcr_convert")
    return dst


def convert_segments(pairs):
    """[(src, dst), ...]: dst[:] = src (element-wise fp32 <-> bf16 conversions or copies) for all pairs in ONE launch per eight pairs
    (modcr_convert_segments).  All sources share a dtype and all destinations share a dtype; tensors contiguous, numel equal per pair."""
    if not pairs:
        return
    sdt, ddt = dt_of(pairs[0][0]), dt_of(pairs[0][1])
    for src, dst in pairs:
        if dt_of(src) != sdt or dt_of(dst) != ddt or src.numel() != dst.numel() or not (src.is_contiguous() and dst.is_contiguous()):
            raise ValueError("convert_segments: pairs must be contiguous, of equal size, with one source and one destination dtype")
    k = len(pairs)
    srcs = (_c.c_void_p * k)(*[p_[0].data_ptr() for p_ in pairs])
    dsts = (_c.c_void_p * k)(*[p_[1].data_ptr() for p_ in pairs])
    ns = (_c.c_int64 * k)(*[p_[0].numel() for p_ in pairs])
    _check(lib().modcr_convert_segments(srcs, dsts, ns, k, sdt, ddt, _stream()), "modcr_convert_segments")


def align_attn(q, k, v, heads, scale=1.0, want_probs=False, dropout=None, key_bias=None):
    """q [N,E] fp32, k/v [N,L,E] (bf16 or fp32) -> out [N,E] fp32, probs [N,heads,L] (unmasked softmax) or None.
    dropout = (p, seed, offset): training-mode dropout of the attention weights."""
    n, l, e = k.shape
    q, k, v = _contig(q, torch.float32), _contig(k), _contig(v)
    out = torch.empty_like(q)
    probs = torch.empty((n, heads, l), dtype=torch.float32, device=q.device) if want_probs else None
    p, seed, off = dropout if dropout is not None else (0.0, 0, 0)
    _check(lib().modcr_align_attn_fwd(_ptr(q), _ptr(k), _ptr(v), e, _ptr(out), _ptr(probs), n, l, e, heads,
                                      float(scale), float(p), seed, off,
                                      _ptr(_contig(key_bias, torch.float32)) if key_bias is not None else None, dt_of(k), _stream()),
           "modcr_align_attn_fwd")
    return out, probs


def align_attn_bwd(dout, q, k, v, probs, heads, scale=1.0, dropout=None):
    n, l, e = k.shape
    dout, q = _contig(dout, torch.float32), _contig(q, torch.float32)
    dq, dk, dv = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
    p, seed, off = dropout if dropout is not None else (0.0, 0, 0)
    _check(lib().modcr_align_attn_bwd(_ptr(dout), _ptr(q), _ptr(k), _ptr(v), e, _ptr(probs), _ptr(dq),
                                      _ptr(dk), _ptr(dv), e, n, l, e, heads, float(scale), float(p), seed, off, dt_of(k),
                                      _stream()),
           "modcr_align_attn_bwd")
    return dq, dk, dv


def _row_blocks(blocks):
    """host arrays of modcr_cls_xattn_*: [N, rows_i, E] bf16 views (last dim contiguous, one row stride for all) -> ctypes arrays"""
    n, _, e = blocks[0].shape
    ld = blocks[0].stride(1)
    for t in blocks:
        if t.dtype != torch.bfloat16 or t.dim() != 3 or t.shape[0] != n or t.shape[2] != e or t.stride(2) != 1 or t.stride(1) != ld:
            raise ValueError("cls_xattn: row blocks must be bf16 [N, rows, E] views with contiguous rows and one row stride")
    k = len(blocks)
    ptrs = (_c.c_void_p * k)(*[t.data_ptr() for t in blocks])
    strides = (_c.c_int64 * k)(*[t.stride(0) for t in blocks])
    rows = (_c.c_int32 * k)(*[t.shape[1] for t in blocks])
    return ptrs, strides, rows, k, ld, n, e, sum(t.shape[1] for t in blocks)


def cls_xattn(qt, blocks, heads, dropout=None):
    """Reassociated single-query cross-attention over frozen bf16 states (include/modcr_hip.h: modcr_cls_xattn_fwd).
    qt [N,heads,E] fp32; blocks: 1-3 bf16 [N,rows,E] views.  Returns (ctx [N,heads,E], ssum [N,heads], probs [N,heads,L])."""
    ptrs, strides, rows, k, ld, n, e, l = _row_blocks(blocks)
    qt = _contig(qt, torch.float32)
    ctx = torch.empty((n, heads, e), dtype=torch.float32, device=qt.device)
    ssum = torch.empty((n, heads), dtype=torch.float32, device=qt.device)
    probs = torch.empty((n, heads, l), dtype=torch.float32, device=qt.device)
    p, seed, off = dropout if dropout is not None else (0.0, 0, 0)
    _check(lib().modcr_cls_xattn_fwd(_ptr(qt), ptrs, strides, rows, k, ld, _ptr(ctx), _ptr(ssum), _ptr(probs), n, e, heads,
                                     float(p), seed, off, _stream()), "modcr_cls_xattn_fwd")
    return ctx, ssum, probs


def cls_xattn_bwd(dctx, dssum, ctx, ssum, probs, blocks, heads, dropout=None):
    ptrs, strides, rows, k, ld, n, e, l = _row_blocks(blocks)
    dctx, dssum = _contig(dctx, torch.float32), _contig(dssum, torch.float32)
    dqt = torch.empty_like(ctx)
    p, seed, off = dropout if dropout is not None else (0.0, 0, 0)
    _check(lib().modcr_cls_xattn_bwd(_ptr(dctx), _ptr(dssum), _ptr(ctx), _ptr(ssum), _ptr(probs), ptrs, strides, rows, k, ld,
                                     _ptr(dqt), n, e, heads, float(p), seed, off, _stream()), "modcr_cls_xattn_bwd")
    return dqt


def mc_ce(logits, label, want_grad=True, want_loss=True, grad_scale=None):
    """Soft-label CE over [B,C]; returns (loss scalar tensor or None, dlogits or None).
    grad_scale: 0-dim/1-element fp32 GPU tensor holding d(total)/d(loss), read on the device."""
    logits = _contig(logits, torch.float32)
    label = _contig(label, torch.float32)
    b, c = logits.shape
    loss = torch.empty((), dtype=torch.float32, device=logits.device) if want_loss else None
    dl = torch.empty_like(logits) if want_grad else None
    gs = _contig(grad_scale, torch.float32) if grad_scale is not None else None
    _check(lib().modcr_mc_ce_fwd_bwd(_ptr(logits), _ptr(label), _ptr(loss), _ptr(dl), _ptr(gs), b, c, _stream()),
           "modcr_mc_ce_fwd_bwd")
    return loss, dl


_scratch = {}


def _workspace(key, nbytes, device):
    """caller-owned scratch for the MFMA backward routes (grown on demand, reused across calls)"""
    b = _scratch.get((key, device))
    if b is None or b.numel() < nbytes:
        b = torch.empty((nbytes,), dtype=torch.uint8, device=device)
        _scratch[(key, device)] = b
    return b


def linear_bwd_input(dy, w, out_dtype=F32, mfma=True):
    """dX = dY @ W.  dY [M,N] fp32 or bf16, W [N,K] (fp32 or bf16).  mfma=False: exact-fp32 kernel."""
    dy = _contig(dy)
    m, n = dy.shape
    k = w.shape[1]
    dx = torch.empty((m, k), dtype=torch_dtype(out_dtype), device=dy.device)
    ws, nb = None, 0
    if mfma and n >= 64 and (dy.dtype == torch.float32 or n % 64 == 0):
        nb = lib().modcr_linear_bwd_input_workspace(m, n, k)
        ws = _workspace("bwd_in", nb, dy.device)
    _check(lib().modcr_linear_bwd_input(_ptr(dy), n, dt_of(dy), _ptr(_contig(w)), k, _ptr(dx), k, m, n, k, dt_of(w),
                                        out_dtype, _ptr(ws), nb, _stream()), "modcr_linear_bwd_input")
    return dx


def linear_bwd_weight(dy, x, dw, db=None, accumulate=False, mfma=True):
    """dW (+)= dY^T @ X, db (+)= colsum(dY).  dY [M,N] fp32/bf16, X [M,K] fp32/bf16, dW fp32 [N,K]."""
    dy = _contig(dy)
    x = _contig(x)
    m, n = dy.shape
    k = x.shape[1]
    ws, nb = None, 0
    if mfma:
        nb = lib().modcr_linear_bwd_weight_workspace(m, n, k)
        ws = _workspace("bwd_w", nb, dy.device)
    _check(lib().modcr_linear_bwd_weight(_ptr(dy), n, dt_of(dy), _ptr(x), k, _ptr(dw), _ptr(db), m, n, k,
                                         1 if accumulate else 0, dt_of(x), _ptr(ws), nb, _stream()),
           "modcr_linear_bwd_weight")
    return dw, db


def layernorm_bwd(dy, x, gamma, eps, dgamma=None, dbeta=None, residual=None):
    dy, x = _contig(dy, torch.float32), _contig(x, torch.float32)
    residual = _contig(residual, torch.float32) if residual is not None else None
    m, h = x.shape
    dx = torch.empty_like(x)
    _check(lib().modcr_layernorm_bwd(_ptr(dy), _ptr(x), _ptr(residual), _ptr(gamma), float(eps), _ptr(dx),
                                     _ptr(dgamma), _ptr(dbeta), m, h, _stream()), "modcr_layernorm_bwd")
    return dx


def act_bwd(dact, pre, act):
    dact, pre = _contig(dact, torch.float32), _contig(pre, torch.float32)
    out = torch.empty_like(pre)
    _check(lib().modcr_act_bwd(_ptr(dact), _ptr(pre), _ptr(out), pre.numel(), act, _stream()), "modcr_act_bwd")
    return out


def sumsq_accumulate(x, out, partials=None):
    """out (fp32 [1], zeroed by the caller) += sum(x^2).  With `partials` (fp32 [>= 1] workspace, sumsq_partials() entries are
    used at most) the sum is formed in a fixed order (bit-reproducible: the clip coefficient of data-parallel replicas)."""
    if partials is None:
        _check(lib().modcr_sumsq_f32(_ptr(x), x.numel(), _ptr(out), _stream()), "modcr_sumsq_f32")
    else:
        if partials.dtype != torch.float32 or not partials.is_contiguous():
            raise ValueError("sumsq_accumulate: partials must be a contiguous fp32 tensor")
        _check(lib().modcr_sumsq_f32_ordered(_ptr(x), x.numel(), _ptr(out), _ptr(partials), partials.numel(), _stream()),
               "modcr_sumsq_f32_ordered")


def sumsq_partials():
    return int(lib().modcr_sumsq_partials())


def adamw_step(p, g, m, v, sumsq, max_norm, lr, beta1, beta2, eps, weight_decay, bc1, bc2, form="hf"):
    """clip by the global norm in `sumsq` (device scalar) + AdamW update, in place on flat fp32 buffers.
    form "hf" = transformers.AdamW (what the reference trains with), "torch" = torch.optim.AdamW."""
    fn = {"hf": lib().modcr_adamw_hf_step, "torch": lib().modcr_adamw_step}[form]
    _check(fn(_ptr(p), _ptr(g), _ptr(m), _ptr(v), p.numel(), _ptr(sumsq), float(max_norm), float(lr),
              float(beta1), float(beta2), float(eps), float(weight_decay), float(bc1), float(bc2),
              _stream()), "modcr_adamw_%s_step" % form)


def qkv_attn_bwd(dctx, x, wqkv, bqkv, dwqkv, dbqkv, key_mask=None, mask_bits=None, chunk_id=None, num_heads=None,
                 accumulate=False, attn_dropout=None, d_align=None, align_t=0, dx_residual=None, ctx=None, lse=None, dump=None,
                 side_post_dropout=False, attn_bias=None, head_mask=None, d_bias=None, hist=None, d_head_mask=None):
    """Backward of qkv_attn: returns dx [N,S,H] in x's dtype; dwqkv [3H,H] / dbqkv [3H] fp32 are
    written (or added into when accumulate).  attn_dropout = the (p, seed, offset) the forward ran with; d_align [N,T,R] =
    gradient of the align map the forward accumulated (align_t = T); dx_residual (fp32, x's shape) is added to dx in the
    epilogue of its GEMM.  ctx + lse: the forward's context rows and the row statistics qkv_attn(lse=) wrote -- the attention
    core then runs as the five-product kernel (csrc/attn_bwd.hip) instead of recomputing the statistics.
    attn_bias / head_mask: the operands of a forward that ran qkv_attn(attn_bias=, head_mask=) (modcr_qkv_attn_bias_bwd, S <= 256);
    d_bias: a contiguous fp32 [N, A, S, S] tensor that receives the gradient of the DENSE bias (sum_to_size it to the bias's own
    shape).  They replace key_mask / mask_bits and do not combine with ctx / lse / dump / d_align.
    hist [N,P,H]: the prefix rows of a forward that ran qkv_attn(hist=, attn_bias= / head_mask=) (modcr_qkv_attn_prefix_bwd,
    P + S <= 256).  Returns (dx, d_hist [N,P,H] in x's dtype); attn_bias is then [.., L = P + S] and d_bias a contiguous fp32
    [N, A, S, L].  A binary key_mask [N, L] is folded on the host into a [N,1,1,L] 0 / -10000 bias (this route has no mask-bit
    variant; use the same fold in the forward).  Not with ctx / lse / dump / d_align / chunk_id / mask_bits.
    d_head_mask: a contiguous fp32 [N, A] tensor that receives the gradient of the head's multiplier, sum_i dctx_i . (P'.V)_i per
    sequence and head (sum_to_size it to the mask's own shape); the call then runs modcr_qkv_attn_gate_bwd, with or without hist, and
    every other result is what it is without d_head_mask.  head_mask=None with d_head_mask stands for a mask of ones."""
    if hist is not None:
        if ctx is not None or lse is not None or dump is not None or d_align is not None or chunk_id is not None or mask_bits is not None:
            raise ValueError("qkv_attn_bwd: hist (prefix rows) does not combine with ctx / lse / dump / d_align / chunk_id / mask_bits")
        if key_mask is not None:
            if attn_bias is not None:
                raise ValueError("qkv_attn_bwd: attn_bias replaces key_mask")
            attn_bias = fold_key_mask(key_mask)
        return _qkv_attn_bias_bwd(dctx, x, hist, wqkv, bqkv, dwqkv, dbqkv, attn_bias, head_mask, d_bias, None, num_heads, accumulate,
                                  attn_dropout, dx_residual, d_head_mask)
    if attn_bias is not None or head_mask is not None or d_bias is not None or d_head_mask is not None:
        if key_mask is not None or mask_bits is not None:
            raise ValueError("qkv_attn_bwd: attn_bias / head_mask replace key_mask / mask_bits")
        if ctx is not None or lse is not None or dump is not None:
            raise ValueError("qkv_attn_bwd: no ctx / lse / dump on the attn_bias / head_mask route (it recomputes the row statistics)")
        if d_align is not None:
            raise ValueError("qkv_attn_bwd: no align-map gradient (d_align) on the attn_bias / head_mask route")
        return _qkv_attn_bias_bwd(dctx, x, None, wqkv, bqkv, dwqkv, dbqkv, attn_bias, head_mask, d_bias, chunk_id, num_heads, accumulate,
                                  attn_dropout, dx_residual, d_head_mask)
    dt = dt_of(x)
    x, dctx = _contig(x), _contig(dctx)
    if (ctx is None) != (lse is None):
        raise ValueError("qkv_attn_bwd: ctx and lse come together")
    if ctx is not None and (ctx.dtype != x.dtype or ctx.shape != x.shape or not ctx.is_contiguous()):
        raise ValueError("qkv_attn_bwd: ctx must be a contiguous tensor of x's shape and dtype")

    n, s, h = x.shape
    if dump is not None and (lse is None or dump.dtype != torch.bfloat16 or dump.numel() != qkv_dump_numel(n, s, num_heads)):
        raise ValueError("qkv_attn_bwd: dump is qkv_attn's dump output of the same call shape, given with ctx and lse")
    dx = torch.empty_like(x)
    need = lib().modcr_qkv_attn_bwd_workspace(n, s, h, dt)
    ws = _workspace("attn_bwd", need, x.device)
    km = _contig(key_mask, torch.float32) if key_mask is not None else None
    chunk_t = 0 if chunk_id is None else chunk_id.shape[1]
    ap, seed, off = attn_dropout if attn_dropout is not None else (0.0, 0, 0)
    _check(lib().modcr_qkv_attn_opt_bwd(_ptr(dctx), _ptr(x), _ptr(_contig(wqkv)), _ptr(bqkv), _ptr(km), _ptr(mask_bits),
                                        _ptr(chunk_id), chunk_t,
                                        _ptr(_contig(dx_residual, torch.float32)) if dx_residual is not None else None,
                                        _ptr(dx), _ptr(dwqkv), _ptr(dbqkv), 1 if accumulate else 0,
                                        n, s, h, num_heads, float(ap), seed, off,
                                        _ptr(_contig(d_align, torch.float32)) if d_align is not None else None, int(align_t),
                                        _ptr(ctx), _ptr(lse), _ptr(dump), ATTN_SIDE_POST_DROPOUT if side_post_dropout else 0,
                                        _ptr(ws), need, dt, _stream()),
           "modcr_qkv_attn_bwd")
    return dx


ATTN_BWD_MAX_KEYS = 256
ATTN_BIAS_BWD_CORES = {0: "refused", 1: "mfma", 2: "exact"}


def _attn_bwd_route(entry, cores, *shape):
    return cores[getattr(lib(), entry + "_route")(*shape)]


def qkv_attn_bias_bwd_route(n, s, h, a, dtype=BF16):
    """The core modcr_qkv_attn_bias_bwd runs for this shape (nothing is launched): "mfma", "exact" or "refused"."""
    return _attn_bwd_route("modcr_qkv_attn_bias_bwd", ATTN_BIAS_BWD_CORES, n, s, h, a, dtype)


def qkv_attn_prefix_bwd_route(n, s, p, h, a, dtype=BF16):
    """The core modcr_qkv_attn_prefix_bwd runs for this shape (nothing is launched): "mfma", "exact" or "refused"."""
    return _attn_bwd_route("modcr_qkv_attn_prefix_bwd", ATTN_BIAS_BWD_CORES, n, s, p, h, a, dtype)


def qkv_attn_gate_bwd_route(n, s, p, h, a, dtype=BF16):
    """The core modcr_qkv_attn_gate_bwd runs for this shape, p >= 0 prefix rows (nothing is launched): "mfma", "exact" or "refused"."""
    return _attn_bwd_route("modcr_qkv_attn_gate_bwd", ATTN_BIAS_BWD_CORES, n, s, p, h, a, dtype)


def _attn_bias_bwd_operands(who, x, hist, attn_bias, head_mask, d_bias, d_head_mask, a, max_keys, bits=False):
    """the checks the bias / prefix / gate backward and qkv_attn_long_bwd share, before any tensor is touched:
    -> (P, fp32 bias or None, its three element strides, [1 or N, A] head mask or None, its sequence stride)"""
    n, s, h = x.shape
    p = 0
    if hist is not None:
        if hist.dim() != 3 or hist.shape[0] != n or hist.shape[2] != h or hist.shape[1] < 1 or hist.dtype != x.dtype:
            raise ValueError("%s: hist must be [N, P >= 1, H] in x's dtype, got %s %s" % (who, tuple(hist.shape), hist.dtype))
        p = hist.shape[1]
    l = p + s
    if l > max_keys:
        raise ValueError(("%s: P + S = %d keys exceeds the %d-key limit of the attention backward" if p else
                          "%s: S = %d exceeds the %d-key limit of the attention backward") % (who, l, max_keys))
    if attn_bias is None and head_mask is None and d_head_mask is None and not bits:        # (dense bits stand in for a bias)
        raise ValueError("%s: hist needs attn_bias, key_mask or head_mask" % who if p else "%s: d_bias without attn_bias" % who)
    bias, strides = (None, (0, 0, 0)) if attn_bias is None else _bias_strides(attn_bias, n, a, s, l)
    hm, hsn = (None, 0) if head_mask is None else _head_mask_2d(head_mask, n, a)
    if d_bias is not None and (bias is None or d_bias.dtype != torch.float32 or tuple(d_bias.shape) != (n, a, s, l) or not d_bias.is_contiguous()):
        raise ValueError("%s: d_bias must be a contiguous fp32 [N, A, S, %s] tensor, given together with attn_bias" % (who, "P + S" if p else "S"))
    if d_head_mask is not None and (d_head_mask.dtype != torch.float32 or tuple(d_head_mask.shape) != (n, a) or not d_head_mask.is_contiguous() or
                                    d_head_mask.device != x.device):
        raise ValueError("%s: d_head_mask must be a contiguous fp32 [N, A] = [%d, %d] tensor on x's device, got %s %s" %
                         (who, n, a, tuple(d_head_mask.shape), d_head_mask.dtype))
    return p, bias, strides, hm, hsn


# The bias family's four C entries take the same operands by name; each lacks some.  Their argument order, as include/modcr_hip.h has it:
_GATE_BWD_ARGS = ("dctx", "x", "hist", "wqkv", "bqkv", "bias", "bsn", "bsa", "bsq", "hm", "hsn", "chunk_id", "chunk_t", "res", "dx", "d_hist",
                  "dwqkv", "dbqkv", "accumulate", "d_bias", "d_head_mask", "n", "s", "p", "h", "a", "ap", "seed", "off", "ws", "need", "dt", "stream")
_ATTN_BIAS_BWD_ARGS = {
    "bias": tuple(k for k in _GATE_BWD_ARGS if k not in ("hist", "d_hist", "d_head_mask", "p")),
    "prefix": tuple(k for k in _GATE_BWD_ARGS if k not in ("chunk_id", "chunk_t", "d_head_mask")),
    "gate": _GATE_BWD_ARGS,
    "long": _GATE_BWD_ARGS,
    "long_drop": _GATE_BWD_ARGS,
    "long_align": _GATE_BWD_ARGS + ("bits", "d_align", "align_t", "flags"),
}


def _qkv_attn_bias_bwd(dctx, x, hist, wqkv, bqkv, dwqkv, dbqkv, attn_bias, head_mask, d_bias, chunk_id, a, accumulate, attn_dropout, dx_residual,
                       d_head_mask=None, long=False, wide_dropout=False, dense_bits=None, d_align=None, align_t=0, side_post_dropout=False):
    """The bias family of the attention backward, one marshalling path for its five C entries: long (qkv_attn_long_bwd) ->
    modcr_qkv_attn_long_bwd, or with wide_dropout modcr_qkv_attn_long_drop_bwd, else with d_head_mask -> modcr_qkv_attn_gate_bwd, else with hist -> modcr_qkv_attn_prefix_bwd, else
    modcr_qkv_attn_bias_bwd.  long with dense_bits / d_align -> modcr_qkv_attn_long_align_bwd (the long_drop entry's arguments, then
    bits, d_align, align_t, flags).  Returns dx, or (dx, d_hist) with hist."""
    who = "qkv_attn_long_bwd" if long else "qkv_attn_bwd"
    dt = dt_of(x)
    n, s, h = x.shape
    align = long and (dense_bits is not None or d_align is not None)
    if align:
        if dense_bits is not None:
            _dense_bits(dense_bits, who, n, s)
        if d_align is not None and (d_align.dtype != torch.float32 or tuple(d_align.shape) != (n, align_t, s - align_t) or not d_align.is_contiguous()):
            raise ValueError("%s: d_align must be a contiguous fp32 [N, align_t, S - align_t] tensor, got %s %s (align_t=%d)" %
                             (who, tuple(d_align.shape), d_align.dtype, align_t))
        if attn_bias is None and head_mask is None and d_head_mask is None and dense_bits is None:      # d_align alone: the zero bias
            attn_bias = torch.zeros((1, 1, 1, s if hist is None else hist.shape[1] + s), dtype=torch.float32, device=x.device)
    p, bias, (bsn, bsa, bsq), hm, hsn = _attn_bias_bwd_operands(who, x, hist, attn_bias, head_mask, d_bias, d_head_mask, a,
                                                                ATTN_BWD_LONG_MAX_KEYS if long else ATTN_BWD_MAX_KEYS,
                                                                bits=align and dense_bits is not None)
    ap, seed, off = attn_dropout if attn_dropout is not None else (0.0, 0, 0)
    if long and p + s > ATTN_BWD_MAX_KEYS and ap > 0 and not wide_dropout:
        raise ValueError("%s: attention-probability dropout (p=%g) is not implemented above %d keys (P + S = %d)" % (who, ap, ATTN_BWD_MAX_KEYS, p + s))
    entry = ("long_align" if align else "long_drop" if wide_dropout else "long") if long else "gate" if d_head_mask is not None else "prefix" if p else "bias"
    fn, ws_fn = {"bias": (lib().modcr_qkv_attn_bias_bwd, lib().modcr_qkv_attn_bias_bwd_workspace),
                 "prefix": (lib().modcr_qkv_attn_prefix_bwd, lib().modcr_qkv_attn_prefix_bwd_workspace),
                 "gate": (lib().modcr_qkv_attn_gate_bwd, lib().modcr_qkv_attn_gate_bwd_workspace),
                 "long": (lib().modcr_qkv_attn_long_bwd, lib().modcr_qkv_attn_long_bwd_workspace),
                 "long_drop": (lib().modcr_qkv_attn_long_drop_bwd, lib().modcr_qkv_attn_long_drop_bwd_workspace),
                 "long_align": (lib().modcr_qkv_attn_long_align_bwd, lib().modcr_qkv_attn_long_align_bwd_workspace)}[entry]
    x, dctx = _contig(x), _contig(dctx)
    dx = torch.empty_like(x)
    hist = _contig(hist) if p else None
    d_hist = torch.empty_like(hist) if p else None
    need = ws_fn(n, s, h, dt) if entry == "bias" else ws_fn(n, s, p, h, dt)
    tensors = dict(dctx=dctx, x=x, hist=hist, wqkv=_contig(wqkv), bqkv=bqkv, bias=bias, hm=hm, chunk_id=chunk_id, dx=dx, d_hist=d_hist, dwqkv=dwqkv,
                   dbqkv=dbqkv, d_bias=d_bias, d_head_mask=d_head_mask, ws=_workspace("attn_bwd", need, x.device), bits=dense_bits, d_align=d_align,
                   res=_contig(dx_residual, torch.float32) if dx_residual is not None else None)
    v = dict(n=n, s=s, p=p, h=h, a=a, dt=dt, bsn=bsn, bsa=bsa, bsq=bsq, hsn=hsn, ap=float(ap), seed=seed, off=off, need=need,
             chunk_t=0 if chunk_id is None else chunk_id.shape[1], accumulate=1 if accumulate else 0,
             align_t=int(align_t) if d_align is not None else 0, flags=ATTN_SIDE_POST_DROPOUT if side_post_dropout else 0)
    v.update((k, _ptr(t)) for k, t in tensors.items())          # (a tensor that is not on the GPU is refused here, before the stream is asked for)
    v["stream"] = _stream()
    _check(fn(*[v[k] for k in _ATTN_BIAS_BWD_ARGS[entry]]), "modcr_qkv_attn_%s_bwd" % entry)
    return (dx, d_hist) if p else dx


ATTN_BWD_LONG_MAX_KEYS = 512
ATTN_LONG_BWD_CORES = {0: "refused", 1: "mfma", 2: "exact", 3: "stream", 4: "stream-exact"}


def qkv_attn_long_bwd_route(n, s, p, h, a, dtype=BF16):
    """The core modcr_qkv_attn_long_bwd runs for this shape, p >= 0 prefix rows (nothing is launched): "mfma" / "exact" (P + S <= 256,
    modcr_qkv_attn_gate_bwd's), "stream" / "stream-exact" (256 < P + S <= 512, csrc/attn_long_bwd.hip) or "refused"."""
    return _attn_bwd_route("modcr_qkv_attn_long_bwd", ATTN_LONG_BWD_CORES, n, s, p, h, a, dtype)


def qkv_attn_long_align_bwd_route(n, s, p, h, a, dtype=BF16):
    """The core modcr_qkv_attn_long_align_bwd runs for this shape (nothing is launched): what qkv_attn_long_bwd_route answers."""
    return _attn_bwd_route("modcr_qkv_attn_long_align_bwd", ATTN_LONG_BWD_CORES, n, s, p, h, a, dtype)


def qkv_attn_long_bwd(dctx, x, wqkv, bqkv, dwqkv, dbqkv, key_mask=None, chunk_id=None, num_heads=None, accumulate=False, attn_dropout=None,
                      dx_residual=None, attn_bias=None, head_mask=None, d_bias=None, hist=None, d_head_mask=None, wide_dropout=False, **align):
    """qkv_attn_bwd's attn_bias / head_mask / hist route with the key limit 512 instead of 256 (modcr_qkv_attn_long_bwd): the backward
    of a forward that ran qkv_attn(attn_bias=, head_mask=, hist=) at P + S <= 512 keys.  Returns dx, or (dx, d_hist) with hist.  At
    P + S <= 256 the call is modcr_qkv_attn_gate_bwd's, bit for bit; above, the streaming cores run and attention dropout is refused.
    A binary key_mask [N, L] is folded into a [N,1,1,L] 0 / -10000 bias (fold the forward the same way); chunk_id only without hist.
    wide_dropout: the backward of a forward that ran qkv_attn(wide_dropout=True) (modcr_qkv_attn_long_drop_bwd): above 256 keys the
    streaming cores regenerate that forward's keep mask from attn_dropout = (p, seed, offset) under the wide counter layout; at
    P + S <= 256 or without dropout it changes nothing.
    dense_bits / d_align / align_t / side_post_dropout: the backward of a forward that ran qkv_attn(dense_bits=, align_map=, align_t=,
    side_post_dropout=) above 256 keys (modcr_qkv_attn_long_align_bwd, S <= ATTN_LONG_ALIGN_MAX_KEYS, no hist): the bits are read on
    top of attn_bias; d_align fp32 [N, align_t, S - align_t] is the gradient of that forward's align map.  A folded key_mask combines
    with both.  With either, dropout above 256 keys is carried as with wide_dropout.  (The four are keyword-only and taken through
    **align: the named parameters stay those of the bias / prefix / gate route, which tests/test_attn_long_bwd_host.py pins.)"""
    unknown = set(align) - {"dense_bits", "d_align", "align_t", "side_post_dropout"}
    if unknown:
        raise TypeError("qkv_attn_long_bwd() got an unexpected keyword argument %r" % sorted(unknown)[0])
    dense_bits, d_align = align.get("dense_bits"), align.get("d_align")
    if hist is not None and chunk_id is not None:
        raise ValueError("qkv_attn_long_bwd: hist (prefix rows) does not combine with chunk_id")
    if key_mask is not None:
        if attn_bias is not None:
            raise ValueError("qkv_attn_long_bwd: attn_bias replaces key_mask")
        attn_bias = fold_key_mask(key_mask)
    return _qkv_attn_bias_bwd(dctx, x, hist, wqkv, bqkv, dwqkv, dbqkv, attn_bias, head_mask, d_bias, chunk_id, num_heads, accumulate,
                              attn_dropout, dx_residual, d_head_mask, long=True,
                              wide_dropout=bool(wide_dropout) or dense_bits is not None or d_align is not None, dense_bits=dense_bits,
                              d_align=d_align, align_t=align.get("align_t", 0), side_post_dropout=bool(align.get("side_post_dropout", False)))


def fold_key_mask(key_mask):
    """binary key mask [N, L] (1 = attend) -> the additive [N,1,1,L] fp32 bias 0 / -10000 of the reference's extended mask"""
    if key_mask.dim() != 2:
        raise ValueError("fold_key_mask: key_mask must be [N, L], got %s" % (tuple(key_mask.shape),))
    return ((1.0 - key_mask.to(torch.float32)) * -10000.0).reshape(key_mask.shape[0], 1, 1, key_mask.shape[1])


def add(a, b, out_dtype=F32, out=None):
    """a (fp32) + b (fp32 or bf16) -> out_dtype (out: a contiguous tensor of that dtype and a's size to write into)"""
    a = _contig(a, torch.float32)
    b = _contig(b)
    if out is None:
        out = torch.empty(a.shape, dtype=torch_dtype(out_dtype), device=a.device)
    elif out.dtype != torch_dtype(out_dtype) or out.numel() != a.numel() or not out.is_contiguous():
        raise ValueError("add: out must be a contiguous %s tensor of %d elements" % (torch_dtype(out_dtype), a.numel()))
    _check(lib().modcr_add(_ptr(a), _ptr(b), dt_of(b), _ptr(out), out_dtype, a.numel(), _stream()), "modcr_add")
    return out


def embedding_bwd(ids, dy, dw, padding_idx=None):
    """dw[id] += sum of the rows of dy [M,H] fp32 whose id it is (ids int64, any shape with M elements); rows of padding_idx are
    skipped.  Deterministic (sorted-segment sums, one writer per table row).  Tables of at most four rows (token types) are reduced
    row by row instead: a segment of M / 2 rows is no work for one workgroup."""
    dy = _contig(dy, torch.float32)
    m, h = dy.shape
    flat = ids.reshape(-1)
    if flat.numel() != m:
        raise ValueError("embedding_bwd: %d ids for %d gradient rows" % (flat.numel(), m))
    if dw.dtype != torch.float32 or not dw.is_contiguous() or dw.shape[1] != h:
        raise ValueError("embedding_bwd: dw must be a contiguous fp32 [V,%d] tensor" % h)
    if dw.shape[0] <= 4:
        for v in range(dw.shape[0]):
            if padding_idx is not None and v == padding_idx:
                continue
            dw[v] += (dy * (flat == v).to(torch.float32)[:, None]).sum(0)
        return dw
    sid, order = torch.sort(flat, stable=True)
    _check(lib().modcr_embedding_bwd_v(_ptr(sid), _ptr(order), _ptr(dy), _ptr(dw), m, h, dw.shape[0],
                                       -1 if padding_idx is None else int(padding_idx), _stream()), "modcr_embedding_bwd")
    return dw


def _grad_out(t, shape, device, what):
    """a caller-provided fp32 gradient tensor (a view into the flat gradient buffer: written in place, no autograd add) or a fresh one"""
    if t is None:
        return torch.empty(shape, dtype=torch.float32, device=device)
    if t.dtype != torch.float32 or tuple(t.shape) != tuple(shape) or not t.is_contiguous() or t.data_ptr() % 16:
        raise ValueError("%s: the output gradient must be a contiguous, 16-byte aligned fp32 tensor of shape %s" % (what, tuple(shape)))
    return t


def linear_residual_ln_bwd(dy, pre, a, w, gamma, eps, dgamma, dbeta, dropout=None, dw_out=None, db_out=None):
    """backward of LN(dropout(a @ w.T + bias) + residual) from the saved pre-LN rows (fp32, or fp16 on the bf16 route): returns
    (d_pre fp32 [M,N] = gradient of the residual branch, da [M,K] in a's dtype, dw fp32, dbias fp32); dgamma / dbeta are accumulated.
    dy fp32 or bf16; dropout = (p, seed, offset) of the forward or None (bf16 route only)."""
    dy, pre = _contig(dy), (_contig(pre) if pre.dtype == torch.float16 else _contig(pre, torch.float32))
    a, w = _contig(a), _contig(w)
    m, n = pre.shape
    k = a.shape[1]
    dt = dt_of(a)
    d_pre = torch.empty(pre.shape, dtype=torch.float32, device=pre.device)
    da = torch.empty_like(a)
    dw = _grad_out(dw_out, (n, k), a.device, "linear_residual_ln_bwd dw")
    db = _grad_out(db_out, (n,), a.device, "linear_residual_ln_bwd db")
    need = lib().modcr_linear_residual_ln_bwd_workspace(m, n, k) if dt == BF16 else 0
    ws = _workspace("lrl_bwd", need, a.device) if need else None
    p, seed, off = dropout if dropout is not None else (0.0, 0, 0)
    _check(lib().modcr_linear_residual_ln_dropout_bwd(_ptr(dy), dt_of(dy), _ptr(pre), dt_of(pre), _ptr(a), k, _ptr(w), _ptr(gamma), float(eps),
                                                      _ptr(d_pre), _ptr(da), _ptr(dw), _ptr(db), _ptr(dgamma), _ptr(dbeta), m, n, k,
                                                      float(p), seed, off, _ptr(ws), need, dt, _stream()),
           "modcr_linear_residual_ln_dropout_bwd")
    return d_pre, da, dw, db


def ffn_up_gelu_bwd(dinter, x, w1, b1, dx_residual=None, dw_out=None, db_out=None):
    """backward of gelu(x @ w1.T + b1): returns (dx fp32 [M,H] (+ dx_residual fp32 [M,H], added in the GEMM's epilogue),
    dw1 fp32, db1 fp32)"""
    dinter, x, w1 = _contig(dinter), _contig(x), _contig(w1)
    m, h = x.shape
    i = w1.shape[0]
    dt = dt_of(x)
    dx = torch.empty((m, h), dtype=torch.float32, device=x.device)
    dw = _grad_out(dw_out, (i, h), x.device, "ffn_up_gelu_bwd dw1")
    db = _grad_out(db_out, (i,), x.device, "ffn_up_gelu_bwd db1")
    need = lib().modcr_ffn_up_gelu_bwd_workspace(m, h, i)
    ws = _workspace("ffn_up_bwd", need, x.device)
    _check(lib().modcr_ffn_up_gelu_bwd(_ptr(dinter), dt_of(dinter), _ptr(x), _ptr(w1), _ptr(b1),
                                       _ptr(_contig(dx_residual, torch.float32)) if dx_residual is not None else None, _ptr(dx), _ptr(dw), _ptr(db),
                                       m, h, i, _ptr(ws), need, dt, _stream()), "modcr_ffn_up_gelu_bwd")
    return dx, dw, db


def ffn_keep_supported(x, w1, b1=None):
    """True where the trainable FFN can keep its GELU input (modcr_ffn_keep_supported: bf16, M >= 256, M % 8 == 0, ...) and the
    operands sit on 16-byte boundaries (views into a packed buffer may not)"""
    if any(t is not None and (t.data_ptr() % 16 or not t.is_contiguous()) for t in (x, w1, b1)):
        return False
    return bool(lib().modcr_ffn_keep_supported(x.shape[0], x.shape[1], w1.shape[0], dt_of(x)))


def ffn_up_gelu_keep(x, w1, b1):
    """(gelu(x @ w1.T + b1), x @ w1.T + b1), both bf16 [M,I], from one GEMM (modcr_ffn_up_gelu_keep_fwd)"""
    x, w1 = _contig(x), _contig(w1)
    _same_dtype("ffn_up_gelu_keep", w1, x=x)
    m, h = x.shape
    i = w1.shape[0]
    out = torch.empty((m, i), dtype=x.dtype, device=x.device)
    pre_act = torch.empty((m, i), dtype=x.dtype, device=x.device)
    _check(lib().modcr_ffn_up_gelu_keep_fwd(_ptr(x), _ptr(w1), _ptr(_contig(b1, torch.float32)), _ptr(out), _ptr(pre_act), m, h, i,
                                            dt_of(x), _stream()), "modcr_ffn_up_gelu_keep_fwd")
    return out, pre_act


def ffn_down_residual_ln_gelu_bwd(dy, pre, inter, w2, gamma, eps, pre_act, dgamma, dbeta, dropout=None, want_db_u=False,
                                  dw_out=None, db_out=None, db_u_out=None):
    """backward of LN(dropout(inter @ w2.T + b2) + residual) that also crosses the GELU: returns (d_pre fp32 [M,H], d_u bf16 [M,I] =
    gradient of the GELU input, dw2 fp32, db2 fp32); dgamma / dbeta are accumulated (modcr_ffn_down_residual_ln_gelu_bwd)."""
    dy, pre = _contig(dy), (_contig(pre) if pre.dtype == torch.float16 else _contig(pre, torch.float32))
    inter, w2, pre_act = _contig(inter), _contig(w2), _contig(pre_act)
    _same_dtype("ffn_down_residual_ln_gelu_bwd", w2, inter=inter, pre_act=pre_act)
    m, h = pre.shape
    i = inter.shape[1]
    if pre_act.shape != inter.shape:
        raise ValueError("ffn_down_residual_ln_gelu_bwd: pre_act %s against inter %s" % (tuple(pre_act.shape), tuple(inter.shape)))
    dt = dt_of(inter)
    d_pre = torch.empty(pre.shape, dtype=torch.float32, device=pre.device)
    du = torch.empty_like(inter)
    db_u = _grad_out(db_u_out, (i,), inter.device, "ffn_down_residual_ln_gelu_bwd db_u") if want_db_u else None
    dw = _grad_out(dw_out, (h, i), inter.device, "ffn_down_residual_ln_gelu_bwd dw2")
    db = _grad_out(db_out, (h,), inter.device, "ffn_down_residual_ln_gelu_bwd db2")
    need = lib().modcr_ffn_down_gelu_bwd_workspace(m, h, i)
    ws = _workspace("lrl_bwd", need, inter.device)
    p, seed, off = dropout if dropout is not None else (0.0, 0, 0)
    _check(lib().modcr_ffn_down_residual_ln_gelu_bwd(_ptr(dy), dt_of(dy), _ptr(pre), dt_of(pre), _ptr(inter), _ptr(w2), _ptr(gamma), float(eps),
                                                     _ptr(pre_act), _ptr(d_pre), _ptr(du), _ptr(db_u), _ptr(dw), _ptr(db), _ptr(dgamma), _ptr(dbeta),
                                                     m, h, i, float(p), seed, off, _ptr(ws), need, dt, _stream()),
           "modcr_ffn_down_residual_ln_gelu_bwd")
    return (d_pre, du, dw, db, db_u) if want_db_u else (d_pre, du, dw, db)


def ffn_up_du_bwd(du, x, w1, dx_residual=None, db1=None, dw_out=None):
    """FFN-up backward from the GELU-input gradient: (dx [M,H] in x's dtype (+ dx_residual, summed in fp32), dw1 fp32, db1 fp32) (modcr_ffn_up_du_bwd).
    db1: the bias gradient when the caller already has it (db_u of ffn_down_residual_ln_gelu_bwd): the weight-gradient product then
    needs no transpose of du."""
    du, x, w1 = _contig(du), _contig(x), _contig(w1)
    _same_dtype("ffn_up_du_bwd", w1, du=du, x=x)
    m, h = x.shape
    i = w1.shape[0]
    dx = torch.empty((m, h), dtype=x.dtype, device=x.device)          # storage dtype (the fp32 sum with dx_residual is rounded once)
    dw = _grad_out(dw_out, (i, h), x.device, "ffn_up_du_bwd dw1")
    have_db = db1 is not None
    db = db1 if have_db else torch.empty((i,), dtype=torch.float32, device=x.device)
    need = lib().modcr_ffn_up_du_bwd_workspace(m, h, i)
    ws = _workspace("ffn_up_bwd", need, x.device)
    _check(lib().modcr_ffn_up_du_bwd(_ptr(du), _ptr(x), _ptr(w1),
                                     _ptr(_contig(dx_residual, torch.float32)) if dx_residual is not None else None, _ptr(dx), _ptr(dw),
                                     None if have_db else _ptr(db), m, h, i, _ptr(ws), need, dt_of(x), _stream()), "modcr_ffn_up_du_bwd")
    return dx, dw, db


class DropoutState(object):
    """(seed, running offset) of the counter-based dropout: every call consumes `numel` counters, so no two dropout
    sites / steps share mask bits; backward passes re-use the (seed, offset) pair their forward recorded."""

    def __init__(self, seed=0):
        self.seed, self.offset = int(seed) & (2 ** 64 - 1), 0

    def manual_seed(self, seed):
        self.seed, self.offset = int(seed) & (2 ** 64 - 1), 0

    def take(self, numel):
        off = (self.offset + 3) & ~3            # a multiple of 4: the row kernels then hash once per 16-byte piece (drop_apply4)
        self.offset = off + int(numel)
        return self.seed, off


DROPOUT = DropoutState(0)


def dropout(x, p, seed, offset, out=None):
    """x * mask / (1 - p) with the counter-based mask of (seed, offset); contiguous x, in place when out is x"""
    x = _contig(x)
    if out is None:
        out = torch.empty_like(x)
    _check(lib().modcr_dropout(_ptr(x), _ptr(out), x.numel(), dt_of(x), float(p), seed, offset, _stream()), "modcr_dropout")
    return out


def dropout_residual_ln(x, residual, gamma, beta, eps, p, seed, offset, out_dtype, pre_out=None):
    """LN(dropout(x) + residual): x [M,H] fp32, or fp16 (the bf16 path's sublayer output).  pre_out: contiguous fp32 or fp16 [M,H]
    tensor that receives the pre-LayerNorm rows dropout(x) + residual"""
    x = _contig(x) if x.dtype == torch.float16 else _contig(x, torch.float32)
    m, h = x.shape
    r2 = _contig(residual.reshape(m, h)) if residual is not None else None
    out = torch.empty((m, h), dtype=torch_dtype(out_dtype), device=x.device)
    if pre_out is not None and (pre_out.dtype not in (torch.float32, torch.float16) or pre_out.numel() != m * h or not pre_out.is_contiguous()):
        raise ValueError("dropout_residual_ln: pre_out must be a contiguous fp32 or fp16 [M,H] tensor")
    _check(lib().modcr_dropout_residual_ln_fwd(_ptr(x), dt_of(x), _ptr(r2), dt_of(r2) if r2 is not None else 0, _ptr(gamma), _ptr(beta),
                                               float(eps), _ptr(out), out_dtype, _ptr(pre_out), dt_of(pre_out) if pre_out is not None else F32,
                                               m, h, float(p), seed, offset, _stream()),
           "modcr_dropout_residual_ln_fwd")
    return out


def layernorm_dropout_bwd(dy, pre, gamma, eps, dgamma, dbeta, want_d_pre=True, want_d_sub=True, dropout=None):
    """LayerNorm backward of the encoder layer's output blocks from the saved pre-LN rows (modcr_layernorm_dropout_bwd): dy [M,H]
    fp32 or bf16, pre [M,H] fp32 or fp16, H in {256, 512, 768, 1024}.  Returns (d_pre fp32 [M,H] or None, d_sub bf16 [M,H] or None):
    d_sub is d_pre under the forward's dropout mask (dropout = (p, seed, offset); None: a plain bf16 copy).  dgamma / dbeta (fp32 [H]
    or None) are accumulated into."""
    dy, pre = _contig(dy), _contig(pre)
    m, h = pre.shape
    if tuple(dy.shape) != (m, h):
        raise ValueError("layernorm_dropout_bwd: dy %s against pre %s" % (tuple(dy.shape), tuple(pre.shape)))
    d_pre = torch.empty((m, h), dtype=torch.float32, device=pre.device) if want_d_pre else None
    d_sub = torch.empty((m, h), dtype=torch.bfloat16, device=pre.device) if want_d_sub else None
    p, seed, off = dropout if dropout is not None else (0.0, 0, 0)
    _check(lib().modcr_layernorm_dropout_bwd(_ptr(dy), dt_of(dy), _ptr(pre), dt_of(pre), _ptr(gamma), float(eps), _ptr(d_pre), _ptr(d_sub),
                                             _ptr(dgamma), _ptr(dbeta), m, h, float(p), seed, off, _stream()),
           "modcr_layernorm_dropout_bwd")
    return d_pre, d_sub
