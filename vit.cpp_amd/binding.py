"""ctypes binding over the C ABI of libvitx.so (include/vitx.h).

Plumbing for tests/ and bench.py: PyTorch provides device memory and streams,
every computation happens inside libvitx.so.  There is NO fallback: if the HIP
library is missing or no GPU is present, the calls raise.
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess
from typing import List, Optional, Tuple

import numpy as np

# the enums a model file or a zero-shot bank carries are numbered once, in ggml_file.py (which needs no library)
from .ggml_file import (ACT_TANH as ACT_GELU_TANH, ACT_ERF as ACT_GELU_ERF, ACT_QUICK as ACT_QUICK_GELU,      # vitx_model_activation (tanh-GELU without `arch`)
                        ZS_SOFTMAX, ZS_SIGMOID, POOL_CLS, POOL_CLS_MEAN, POOL_MAP,                           # vitx_zs_kind, vitx_model_head_pool
                        PP_REF_BICUBIC, PP_REF_BILINEAR, PP_PIL_BILINEAR, PP_PIL_BICUBIC, PP_STRETCH, PP_SHORTEST_EDGE)      # vitx_pp_filter, vitx_pp_resize

_HERE = os.path.dirname(os.path.abspath(__file__))
# VITX_LIB: development override (the -DVITX_LAB laboratory build, A/B builds).  bench.py marks its line invalid when it is set.
LIB_PATH = os.environ.get("VITX_LIB") or os.path.join(_HERE, "libvitx.so")

F16, BF16, MXFP8 = 0, 1, 2      # MXFP8: qkv, fc1 and fc2 on block-scaled e4m3 operands (include/vitx.h VITX_MXFP8; mxfp8.py)
LN_TEST_KEY = 0x7e570000        # vitx_ctx_options::ln_test is honoured only as LN_TEST_KEY | mode
BICUBIC, BILINEAR = 0, 1
EPI_BIAS, EPI_BIAS_GELU, EPI_BIAS_RESID, EPI_BIAS_F32, EPI_PATCH, EPI_BIAS_HILO = 0, 1, 2, 3, 4, 5
EPI_BIAS_GELU_ERF, EPI_BIAS_QGELU = 6, 7      # fc1 epilogues of the other two activations (same rounding points as EPI_BIAS_GELU)
ERR_IO, ERR_FORMAT, ERR_ARG, ERR_HIP, ERR_UNSUPPORTED, ERR_NOMEM = 1, 2, 3, 4, 5, 6      # status codes (VitxError.code)
GEMM_AUTO, GEMM_PP, GEMM_AUTO_SPLIT = 0, 1, 2          # vitx_op_gemm_ex `kernel` (or a ring configuration: 945, 445, 245, 122)
ATTN_AUTO, ATTN_SINGLE, ATTN_FLOW, ATTN_PERSIST, ATTN_STREAM = 0, 1, 3, 4, 5   # vitx_op_attention_ex `kernel`
ATTN_ROLLOUT = 1                # vitx_attn_enable flag
FEAT_CLS, FEAT_MEAN, FEAT_TOKENS, FEAT_L2 = 1, 2, 4, 8      # vitx_feat_enable flags
KIND_IMAGE, KIND_TEXT = 0, 1            # vitx_model_kind
TEXT_L2 = 1                             # vitx_text_embed flag
NN_LOGITS, NN_EMBED = 0, 1              # vitx_nn_source
DENSE_SCORE, DENSE_LOGITS = 1, 2        # vitx_dense_flags
DEPTH_NORM, DEPTH_LOGITS, DEPTH_FINE = 1, 2, 4      # vitx_depth_flags
POS_BICUBIC, POS_BICUBIC_AA = 0, 1      # vitx_pos_interp: F.interpolate(mode="bicubic") without / with antialias=True (include/vitx.h)

EXPORTS = [
    "vitx_status_str", "vitx_last_error", "vitx_model_load", "vitx_model_free", "vitx_model_uid", "vitx_model_hparams", "vitx_model_num_labels",
    "vitx_model_label", "vitx_model_num_tensors", "vitx_model_tensor_info", "vitx_model_tensor_f32", "vitx_quantize_file", "vitx_image_load", "vitx_image_decode", "vitx_image_free", "vitx_preprocess_u8", "vitx_preprocess_u8_device",
    "vitx_ctx_create", "vitx_ctx_create_ex", "vitx_ctx_free", "vitx_ctx_max_batch", "vitx_forward", "vitx_forward_device", "vitx_ctx_synchronize",
    "vitx_topk", "vitx_group_create", "vitx_group_free", "vitx_group_num_devices", "vitx_group_forward", "vitx_group_out_floats", "vitx_group_forward_device", "vitx_group_result", "vitx_group_result_rows", "vitx_profile_enable", "vitx_profile_read", "vitx_profile_bracket_us", "vitx_op_layernorm", "vitx_op_gemm", "vitx_op_gemm_ex", "vitx_op_attention", "vitx_op_attention_ex", "vitx_op_softmax", "vitx_op_softmax_dt", "vitx_trace_enable", "vitx_trace_read",
    "vitx_op_dequant", "vitx_op_gemm_q4", "vitx_ctx_weight_bytes", "vitx_ctx_shares_weights", "vitx_probe_mfma", "vitx_op_gemm_ln", "vitx_ctx_ln_fallbacks", "vitx_ctx_stream_retries",
    "vitx_model_in_channels", "vitx_model_seq_len", "vitx_ctx_out_rows", "vitx_ctx_split", "vitx_ctx_ln_fusion_active", "vitx_op_attention_f32", "vitx_op_attention_planes", "vitx_op_attention_cls", "vitx_preprocess_vitstr_u8", "vitx_vitstr_decode",
    "vitx_attn_enable", "vitx_attn_floats", "vitx_attn_images", "vitx_attn_read", "vitx_op_attention_map", "vitx_ctx_graph_launches",
    "vitx_op_rollout_factor", "vitx_op_rollout_step", "vitx_op_rollout_row",
    "vitx_mxfp8_quantize", "vitx_op_quantize_mxfp8", "vitx_op_layernorm_mxfp8", "vitx_op_gemm_mxfp8",
    "vitx_feat_enable", "vitx_feat_floats", "vitx_feat_images", "vitx_feat_read", "vitx_feat_device", "vitx_op_features",
    "vitx_ctx_img_size", "vitx_ctx_tokens", "vitx_pos_embed_resample", "vitx_op_pos_embed_resample", "vitx_model_resize_file",
    "vitx_op_topk", "vitx_op_dequant_jobs",
    "vitx_model_num_registers", "vitx_model_head_pool", "vitx_ctx_registers", "vitx_op_features_ex", "vitx_op_patch_embed",
    "vitx_model_activation", "vitx_model_has_pre_norm", "vitx_op_layernorm_f32",
    "vitx_model_preproc", "vitx_model_has_preproc", "vitx_preproc_at_size", "vitx_preprocess_ex", "vitx_preprocess_ex_device", "vitx_preprocess_ex_device_supports",
    "vitx_model_num_prefix", "vitx_model_pool_query", "vitx_op_attention_pool",
    "vitx_zeroshot_set", "vitx_zeroshot_classes", "vitx_zeroshot_images", "vitx_zeroshot_read", "vitx_zeroshot_device", "vitx_zeroshot_max_classes", "vitx_op_zeroshot",
    "vitx_nn_width", "vitx_nn_set", "vitx_nn_rows", "vitx_nn_k", "vitx_nn_labels", "vitx_nn_images", "vitx_nn_read", "vitx_nn_device", "vitx_nn_scratch_bytes",
    "vitx_op_nn_select", "vitx_op_nn_finish", "vitx_op_nn_state_bytes", "vitx_op_nn",
    "vitx_dense_set", "vitx_dense_classes", "vitx_dense_shape", "vitx_dense_images", "vitx_dense_read", "vitx_dense_device", "vitx_dense_scratch_bytes",
    "vitx_op_dense_labels", "vitx_dense_labels_host", "vitx_op_dense",
    "vitx_depth_set", "vitx_depth_bins", "vitx_depth_shape", "vitx_depth_images", "vitx_depth_read", "vitx_depth_device", "vitx_depth_scratch_bytes",
    "vitx_op_depth_fine", "vitx_op_depth_resize", "vitx_depth_host", "vitx_op_depth", "vitx_op_depth_rows",
    "vitx_model_kind", "vitx_model_text_info", "vitx_model_text_zs", "vitx_text_create", "vitx_text_free", "vitx_text_embed", "vitx_text_embed_device", "vitx_text_shares_weights", "vitx_text_check_ids",
    "vitx_op_text_embed", "vitx_op_text_pool", "vitx_op_attention_text", "vitx_op_attention_generic",
    "vitx_model_rope", "vitx_model_rope_table", "vitx_op_rope",
    "vitx_model_glu", "vitx_op_swiglu",
    "vitx_ctx_create_rect", "vitx_ctx_img_shape", "vitx_ctx_grid", "vitx_op_patch_embed_rect",
    "vitx_rect_shape", "vitx_preprocess_rect", "vitx_preprocess_rect_device", "vitx_preprocess_rect_device_supports",
    "vitx_pack_create", "vitx_pack_free", "vitx_pack_shares_weights", "vitx_pack_check", "vitx_pack_distinct_grids", "vitx_pack_forward", "vitx_pack_forward_device",
    "vitx_pack_feat_enable", "vitx_pack_feat_read", "vitx_pack_scratch_bytes", "vitx_pack_launches", "vitx_op_attention_packed", "vitx_op_attention_packed_tables", "vitx_op_rope_packed",
    "vitx_pack_dense_set", "vitx_pack_dense_out", "vitx_pack_dense_check", "vitx_pack_dense_read", "vitx_pack_dense_device", "vitx_pack_dense_scratch_bytes", "vitx_op_dense_labels_packed",
    "vitx_dense_pack_tables", "vitx_op_dense_labels_packed_tables",
    "vitx_pack_depth_set", "vitx_pack_depth_out", "vitx_pack_depth_check", "vitx_pack_depth_read", "vitx_pack_depth_device", "vitx_pack_depth_scratch_bytes",
    "vitx_op_depth_fine_packed", "vitx_op_depth_resize_packed", "vitx_depth_pack_tables", "vitx_op_depth_fine_packed_tables", "vitx_op_depth_resize_packed_tables",
    "vitx_pack_u8_set", "vitx_pack_u8_sources", "vitx_pack_forward_u8", "vitx_pack_u8_check", "vitx_pack_fit_shapes", "vitx_op_preprocess_pack",
    "vitx_pack_attn_enable", "vitx_pack_attn_floats", "vitx_pack_attn_read", "vitx_pack_attn_device", "vitx_pack_attn_check",
    "vitx_op_attention_map_packed", "vitx_op_rollout_step_packed", "vitx_op_rollout_row_packed",
]


class HParams(C.Structure):
    _fields_ = [("hidden_size", C.c_int32), ("num_hidden_layers", C.c_int32), ("num_attention_heads", C.c_int32), ("num_classes", C.c_int32),
                ("patch_size", C.c_int32), ("img_size", C.c_int32), ("ftype", C.c_int32), ("eps", C.c_float)]


class CtxOptions(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("streams", C.c_int32), ("graph", C.c_int32), ("quant_on_host", C.c_int32), ("q4_fused_rows", C.c_int32),
                ("split_first", C.c_int32), ("no_ln_fusion", C.c_int32), ("ln_test", C.c_int32), ("f16_fast_attention", C.c_int32), ("last_layer_all_rows", C.c_int32),
                ("img_size", C.c_int32), ("pos_interp", C.c_int32)]


class PackOptions(C.Structure):
    _fields_ = [("pos_interp", C.c_int), ("max_grids", C.c_int), ("reserved", C.c_int * 6)]


class Preproc(C.Structure):
    """vitx_preproc: how a model's publisher turns a decoded u8 RGB image into its input (include/vitx.h "each model's own preprocessing")."""
    _fields_ = [("resize_mode", C.c_int32), ("resize_a", C.c_int32), ("resize_b", C.c_int32), ("filter", C.c_int32), ("crop", C.c_int32), ("crop_round", C.c_int32),
                ("mean255", C.c_float * 3), ("std255", C.c_float * 3)]

    @classmethod
    def make(cls, resize_mode=PP_STRETCH, resize_a=224, resize_b=0, filter=PP_PIL_BICUBIC, crop=0, crop_round=0, mean255=(0.0, 0.0, 0.0), std255=(1.0, 1.0, 1.0)) -> "Preproc":
        return cls(resize_mode, resize_a, resize_b, filter, crop, crop_round, (C.c_float * 3)(*mean255), (C.c_float * 3)(*std255))

    @property
    def out_size(self) -> int:
        return self.crop or self.resize_a

    def fields(self) -> dict:
        return dict(resize_mode=self.resize_mode, resize_a=self.resize_a, resize_b=self.resize_b, filter=self.filter, crop=self.crop, crop_round=self.crop_round,
                    mean255=tuple(np.float32(v) for v in self.mean255), std255=tuple(np.float32(v) for v in self.std255))


class ProfEntry(C.Structure):
    _fields_ = [("name", C.c_char_p), ("launches", C.c_int32), ("total_ms", C.c_double), ("flops", C.c_double), ("bytes", C.c_double), ("busy_ms", C.c_double)]


class VitxError(RuntimeError):
    code = 0        # the vitx_status behind the error (ERR_*), where check() raised it


def build(force: bool = False) -> str:
    """Compile libvitx.so for gfx950 in-tree (hipcc cross-compiles without a GPU)."""
    args = ["make", "-C", _HERE, "-j8"] + (["-B"] if force else [])
    subprocess.check_call(args, stdout=subprocess.DEVNULL)
    return LIB_PATH


_lib = None


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise VitxError(f"{LIB_PATH} is missing: run __graft_entry__.build() (there is no CPU fallback)")
        L = C.CDLL(LIB_PATH)
        vp, ip = C.c_void_p, C.c_int
        L.vitx_status_str.restype = C.c_char_p; L.vitx_status_str.argtypes = [ip]
        L.vitx_last_error.restype = C.c_char_p
        L.vitx_model_load.argtypes = [C.c_char_p, C.POINTER(vp)]
        L.vitx_model_free.argtypes = [vp]
        L.vitx_model_hparams.argtypes = [vp, C.POINTER(HParams)]
        L.vitx_model_num_labels.argtypes = [vp]
        L.vitx_model_label.restype = C.c_char_p; L.vitx_model_label.argtypes = [vp, ip]
        L.vitx_model_num_tensors.argtypes = [vp]
        L.vitx_model_tensor_info.argtypes = [vp, ip, C.POINTER(C.c_char_p), C.POINTER(C.c_int32), C.POINTER(C.c_int64), C.POINTER(C.c_size_t)]
        L.vitx_model_tensor_f32.argtypes = [vp, ip, C.POINTER(C.c_float), C.c_size_t]
        L.vitx_quantize_file.argtypes = [C.c_char_p, C.c_char_p, ip]
        L.vitx_image_load.argtypes = [C.c_char_p, C.POINTER(C.POINTER(C.c_uint8)), C.POINTER(ip), C.POINTER(ip)]
        L.vitx_image_decode.argtypes = [C.c_char_p, C.c_size_t, C.POINTER(C.POINTER(C.c_uint8)), C.POINTER(ip), C.POINTER(ip)]
        L.vitx_image_free.argtypes = [C.POINTER(C.c_uint8)]
        L.vitx_preprocess_u8.argtypes = [C.POINTER(C.c_uint8), ip, ip, ip, ip, C.POINTER(C.c_float)]
        L.vitx_preprocess_u8_device.argtypes = [vp, ip, ip, ip, ip, ip, vp, vp]
        L.vitx_ctx_create.argtypes = [vp, ip, ip, ip, C.POINTER(vp)]
        L.vitx_ctx_create_ex.argtypes = [vp, ip, ip, ip, C.POINTER(CtxOptions), C.POINTER(vp)]
        L.vitx_ctx_free.argtypes = [vp]
        L.vitx_ctx_max_batch.argtypes = [vp]
        L.vitx_forward.argtypes = [vp, C.POINTER(C.c_float), ip, C.POINTER(C.c_float), C.POINTER(C.c_float)]
        L.vitx_forward_device.argtypes = [vp, vp, ip, vp, vp, vp]
        L.vitx_ctx_synchronize.argtypes = [vp]
        L.vitx_group_create.argtypes = [vp, C.POINTER(C.c_int), ip, ip, ip, C.POINTER(vp)]
        L.vitx_group_free.argtypes = [vp]
        L.vitx_group_num_devices.argtypes = [vp]
        L.vitx_group_forward.argtypes = [vp, C.POINTER(C.c_float), ip, C.POINTER(C.c_float)]
        L.vitx_group_out_floats.argtypes = [vp]
        L.vitx_group_forward_device.argtypes = [vp, C.POINTER(C.c_void_p), C.POINTER(ip), ip]
        L.vitx_group_result.restype = C.c_void_p; L.vitx_group_result.argtypes = [vp, ip]
        L.vitx_group_result_rows.argtypes = [vp]
        L.vitx_topk.argtypes = [C.POINTER(C.c_float), ip, ip, C.POINTER(C.c_int32), C.POINTER(C.c_float)]
        L.vitx_profile_enable.argtypes = [vp, ip]
        L.vitx_profile_read.argtypes = [vp, C.POINTER(ProfEntry), ip, C.POINTER(ip)]
        if hasattr(L, "vitx_profile_bracket_us"):      # (tools/ab_libs.py also loads builds that predate it)
            L.vitx_profile_bracket_us.argtypes = [vp, C.POINTER(C.c_double)]
        L.vitx_op_layernorm.argtypes = [ip, vp, vp, vp, vp, ip, ip, C.c_float, vp]
        L.vitx_op_gemm.argtypes = [ip, ip, vp, vp, vp, vp, ip, ip, ip, vp]
        L.vitx_op_attention.argtypes = [ip, vp, vp, ip, ip, ip, ip, vp]
        L.vitx_op_softmax.argtypes = [vp, vp, ip, ip, ip, vp]
        L.vitx_op_attention_ex.argtypes = [ip, ip, vp, vp, ip, ip, ip, ip, vp]
        L.vitx_op_softmax_dt.argtypes = [ip, vp, vp, ip, ip, ip, vp]
        L.vitx_op_gemm_ex.argtypes = [ip, ip, ip, vp, vp, vp, vp, vp, ip, ip, ip, ip, ip, vp]
        L.vitx_trace_enable.argtypes = [vp, C.POINTER(C.c_int32), ip]
        L.vitx_trace_read.argtypes = [vp, C.POINTER(C.c_float), C.c_size_t]
        L.vitx_op_dequant.argtypes = [ip, ip, vp, vp, vp, ip, ip, ip, vp]
        L.vitx_op_gemm_q4.argtypes = [ip, ip, vp, vp, vp, vp, vp, ip, ip, ip, ip, vp]
        L.vitx_ctx_weight_bytes.restype = C.c_size_t; L.vitx_ctx_weight_bytes.argtypes = [vp]
        L.vitx_ctx_shares_weights.restype = C.c_int; L.vitx_ctx_shares_weights.argtypes = [vp]
        L.vitx_ctx_ln_fallbacks.restype = C.c_longlong; L.vitx_ctx_ln_fallbacks.argtypes = [vp]
        L.vitx_ctx_stream_retries.argtypes = [vp]
        L.vitx_op_gemm_ln.argtypes = [ip, vp, vp, vp, vp, vp, vp, vp, ip, ip, ip, C.c_float, ip, ip, C.POINTER(ip), vp]
        L.vitx_probe_mfma.argtypes = [ip, ip, ip, C.c_double, C.POINTER(C.c_double), C.POINTER(C.c_double)]
        L.vitx_model_in_channels.argtypes = [vp]; L.vitx_model_seq_len.argtypes = [vp]; L.vitx_ctx_out_rows.argtypes = [vp]
        L.vitx_ctx_split.argtypes = [vp, ip, C.POINTER(C.c_int32), ip]
        L.vitx_ctx_ln_fusion_active.argtypes = [vp]
        L.vitx_op_attention_f32.argtypes = [vp, vp, ip, ip, ip, ip, vp]
        L.vitx_op_attention_planes.argtypes = [vp, C.c_long, vp, ip, ip, ip, ip, vp]
        if hasattr(L, "vitx_op_attention_cls"):
            L.vitx_op_attention_cls.argtypes = [ip, vp, C.c_long, vp, ip, ip, ip, ip, vp]
        L.vitx_preprocess_vitstr_u8.argtypes = [C.POINTER(C.c_uint8), ip, ip, ip, C.POINTER(C.c_float)]
        L.vitx_vitstr_decode.argtypes = [C.POINTER(C.c_float), ip, ip, C.POINTER(C.c_int32), C.POINTER(ip), C.POINTER(C.c_double)]
        if hasattr(L, "vitx_attn_enable"):
            L.vitx_attn_enable.argtypes = [vp, C.c_uint64, ip]
            L.vitx_attn_floats.argtypes = [vp]
            L.vitx_attn_images.argtypes = [vp]
            L.vitx_ctx_graph_launches.restype = C.c_longlong; L.vitx_ctx_graph_launches.argtypes = [vp]
            L.vitx_attn_read.argtypes = [vp, C.POINTER(C.c_float), C.c_size_t]
            L.vitx_op_attention_map.argtypes = [ip, vp, C.c_long, vp, vp, ip, ip, ip, ip, vp]
        if hasattr(L, "vitx_op_rollout_step"):
            L.vitx_op_rollout_factor.argtypes = [ip, vp, C.c_long, vp, ip, ip, ip, ip, vp]
            L.vitx_op_rollout_step.argtypes = [vp, vp, ip, ip, vp]
            L.vitx_op_rollout_row.argtypes = [vp, C.c_long, vp, vp, C.c_long, ip, ip, ip, vp]
        if hasattr(L, "vitx_mxfp8_quantize"):
            L.vitx_mxfp8_quantize.argtypes = [C.POINTER(C.c_float), ip, ip, ip, C.POINTER(C.c_uint8), C.POINTER(C.c_uint8)]
            L.vitx_op_quantize_mxfp8.argtypes = [vp, ip, ip, ip, vp, vp, vp]
            L.vitx_op_layernorm_mxfp8.argtypes = [vp, vp, vp, vp, vp, ip, ip, C.c_float, vp]
            L.vitx_op_gemm_mxfp8.argtypes = [ip, vp, vp, vp, vp, vp, vp, vp, ip, ip, ip, vp]
        if hasattr(L, "vitx_feat_enable"):
            L.vitx_feat_enable.argtypes = [vp, ip, C.c_uint64]
            L.vitx_feat_floats.argtypes = [vp]
            L.vitx_feat_images.argtypes = [vp]
            L.vitx_feat_read.argtypes = [vp, C.POINTER(C.c_float), C.c_size_t]
            L.vitx_feat_device.restype = C.c_void_p; L.vitx_feat_device.argtypes = [vp]
            L.vitx_op_features.argtypes = [vp, C.c_long, C.c_long, vp, vp, vp, vp, vp, C.c_long, ip, ip, ip, C.c_float, ip, vp]
        if hasattr(L, "vitx_ctx_img_size"):
            L.vitx_ctx_img_size.argtypes = [vp]; L.vitx_ctx_tokens.argtypes = [vp]
            L.vitx_pos_embed_resample.argtypes = [C.POINTER(C.c_float), ip, ip, ip, ip, ip, ip, C.POINTER(C.c_float)]
            L.vitx_op_pos_embed_resample.argtypes = [vp, ip, ip, ip, ip, ip, ip, vp, vp]
            L.vitx_model_resize_file.argtypes = [C.c_char_p, C.c_char_p, ip, ip]
        if hasattr(L, "vitx_op_topk"):
            L.vitx_op_topk.argtypes = [vp, ip, ip, ip, vp, vp]
            L.vitx_op_dequant_jobs.argtypes = [ip, ip, ip, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), C.POINTER(ip), C.POINTER(ip), C.POINTER(ip), vp]
        if hasattr(L, "vitx_model_num_registers"):
            L.vitx_model_num_registers.argtypes = [vp]; L.vitx_model_head_pool.argtypes = [vp]; L.vitx_ctx_registers.argtypes = [vp]
            L.vitx_op_features_ex.argtypes = [vp, C.c_long, C.c_long, vp, vp, vp, vp, vp, C.c_long, ip, ip, ip, ip, C.c_float, ip, vp, ip, vp]
            L.vitx_op_patch_embed.argtypes = [ip, vp, vp, vp, vp, vp, vp, ip, vp, ip, ip, ip, ip, ip, vp]
        if hasattr(L, "vitx_model_activation"):
            L.vitx_model_activation.argtypes = [vp]; L.vitx_model_has_pre_norm.argtypes = [vp]
            L.vitx_op_layernorm_f32.argtypes = [vp, vp, vp, vp, ip, ip, C.c_float, vp]
        if hasattr(L, "vitx_preprocess_ex"):
            pp = C.POINTER(Preproc)
            L.vitx_model_preproc.argtypes = [vp, pp]; L.vitx_model_has_preproc.argtypes = [vp]
            L.vitx_preproc_at_size.argtypes = [pp, ip, pp]
            L.vitx_preprocess_ex.argtypes = [pp, C.POINTER(C.c_uint8), ip, ip, C.POINTER(C.c_float)]
            L.vitx_preprocess_ex_device.argtypes = [pp, vp, ip, ip, ip, vp, vp]
            L.vitx_preprocess_ex_device_supports.argtypes = [pp, ip, ip]
        if hasattr(L, "vitx_model_num_prefix"):
            L.vitx_model_num_prefix.argtypes = [vp]
            L.vitx_model_pool_query.argtypes = [vp, C.POINTER(C.c_float)]
            L.vitx_op_attention_pool.argtypes = [vp, C.c_long, C.c_long, vp, vp, C.c_float, vp, vp, vp, ip, ip, ip, ip, vp]
        if hasattr(L, "vitx_zeroshot_set"):
            fp = C.POINTER(C.c_float)
            L.vitx_zeroshot_set.argtypes = [vp, fp, ip, ip, ip, C.c_float, C.c_float]
            L.vitx_zeroshot_classes.argtypes = [vp]; L.vitx_zeroshot_images.argtypes = [vp]; L.vitx_zeroshot_max_classes.argtypes = [ip]
            L.vitx_zeroshot_read.argtypes = [vp, fp, fp, C.c_size_t]
            L.vitx_zeroshot_device.restype = C.c_void_p; L.vitx_zeroshot_device.argtypes = [vp]
            L.vitx_op_zeroshot.argtypes = [ip, vp, C.c_long, vp, vp, vp, vp, vp, ip, ip, ip, ip, C.c_float, C.c_float, vp]
        if hasattr(L, "vitx_nn_set"):
            fp, i32p = C.POINTER(C.c_float), C.POINTER(C.c_int32)
            L.vitx_nn_width.argtypes = [vp, ip]
            L.vitx_nn_set.argtypes = [vp, fp, C.c_long, ip, ip, ip, i32p, ip, C.c_float]
            L.vitx_nn_rows.restype = C.c_long; L.vitx_nn_rows.argtypes = [vp]
            L.vitx_nn_k.argtypes = [vp]; L.vitx_nn_labels.argtypes = [vp]; L.vitx_nn_images.argtypes = [vp]
            L.vitx_nn_read.argtypes = [vp, i32p, fp, fp]
            L.vitx_nn_device.restype = C.c_void_p; L.vitx_nn_device.argtypes = [vp]
            L.vitx_nn_scratch_bytes.restype = C.c_size_t; L.vitx_nn_scratch_bytes.argtypes = [vp]
            L.vitx_op_nn_select.argtypes = [vp, C.c_long, ip, ip, C.c_long, vp, ip, ip, vp]
            L.vitx_op_nn_finish.argtypes = [vp, ip, ip, vp, ip, C.c_float, vp, vp, vp]
            L.vitx_op_nn_state_bytes.restype = C.c_size_t; L.vitx_op_nn_state_bytes.argtypes = [ip, ip]
            L.vitx_op_nn.argtypes = [ip, vp, C.c_long, ip, ip, vp, C.c_long, ip, ip, ip, vp, vp, vp, vp, vp]
        if hasattr(L, "vitx_dense_set"):
            fp, u8p, intp = C.POINTER(C.c_float), C.POINTER(C.c_uint8), C.POINTER(C.c_int)
            L.vitx_dense_set.argtypes = [vp, fp, fp, ip, ip, C.c_uint64, ip, ip, ip]
            L.vitx_dense_classes.argtypes = [vp]; L.vitx_dense_images.argtypes = [vp]
            L.vitx_dense_shape.argtypes = [vp, intp, intp]
            L.vitx_dense_read.argtypes = [vp, u8p, fp, fp]
            L.vitx_dense_device.restype = C.c_void_p; L.vitx_dense_device.argtypes = [vp]
            L.vitx_dense_scratch_bytes.restype = C.c_size_t; L.vitx_dense_scratch_bytes.argtypes = [vp]
            L.vitx_op_dense_labels.argtypes = [vp, C.c_long, ip, ip, ip, ip, ip, ip, vp, vp, vp]
            L.vitx_dense_labels_host.argtypes = [vp, C.c_long, ip, ip, ip, ip, ip, ip, vp, vp]
            L.vitx_op_dense.argtypes = [ip, vp, vp, vp, vp, ip, ip, ip, ip, ip, ip, ip, vp, vp, vp]
        if hasattr(L, "vitx_depth_set"):
            fp, intp, cf = C.POINTER(C.c_float), C.POINTER(C.c_int), C.c_float
            L.vitx_depth_set.argtypes = [vp, fp, fp, fp, fp, ip, ip, C.c_uint64, ip, cf, cf, ip, ip, ip]
            L.vitx_depth_bins.argtypes = [vp]; L.vitx_depth_images.argtypes = [vp]
            L.vitx_depth_shape.argtypes = [vp, intp, intp, intp, intp]
            L.vitx_depth_read.argtypes = [vp, fp, fp, fp, fp]
            L.vitx_depth_device.restype = C.c_void_p; L.vitx_depth_device.argtypes = [vp]
            L.vitx_depth_scratch_bytes.restype = C.c_size_t; L.vitx_depth_scratch_bytes.argtypes = [vp]
            L.vitx_op_depth_fine.argtypes = [vp, C.c_long, vp, vp, ip, ip, ip, ip, ip, vp, vp]
            L.vitx_op_depth_resize.argtypes = [vp, ip, ip, ip, ip, ip, cf, cf, vp, vp]
            L.vitx_depth_host.argtypes = [vp, C.c_long, vp, vp, ip, ip, ip, ip, ip, ip, ip, cf, cf, vp, vp]
            L.vitx_op_depth.argtypes = [ip, vp, vp, vp, vp, vp, vp, vp, vp, ip, ip, ip, ip, ip, ip, ip, ip, cf, cf, vp, vp, vp]
            L.vitx_op_depth_rows.argtypes = [ip, vp, C.c_long, vp, C.c_long, ip, ip, vp]
        if hasattr(L, "vitx_text_create"):
            i32p = C.POINTER(C.c_int32)
            L.vitx_model_kind.argtypes = [vp]
            L.vitx_model_text_info.argtypes = [vp, C.POINTER(ip), C.POINTER(ip), C.POINTER(ip), C.POINTER(ip)]
            L.vitx_model_text_zs.argtypes = [vp, C.POINTER(ip), C.POINTER(C.c_float), C.POINTER(C.c_float)]
            L.vitx_text_create.argtypes = [vp, ip, ip, ip, C.POINTER(vp)]
            L.vitx_text_free.argtypes = [vp]
            L.vitx_text_embed.argtypes = [vp, i32p, ip, ip, C.POINTER(C.c_float)]
            L.vitx_text_embed_device.argtypes = [vp, i32p, ip, ip, vp, vp]
            L.vitx_text_shares_weights.argtypes = [vp]
            L.vitx_text_check_ids.argtypes = [vp, i32p, ip, i32p]
            L.vitx_op_text_embed.argtypes = [ip, vp, vp, vp, vp, ip, ip, ip, vp]
            L.vitx_op_text_pool.argtypes = [ip, vp, vp, vp, vp, vp, ip, ip, ip, C.c_float, vp]
            L.vitx_op_attention_text.argtypes = [ip, vp, vp, ip, ip, ip, ip, ip, vp]
            L.vitx_op_attention_generic.argtypes = [ip, vp, vp, ip, ip, ip, ip, vp]
        if hasattr(L, "vitx_op_rope"):
            L.vitx_model_rope.argtypes = [vp, C.POINTER(ip), C.POINTER(C.c_float)]
            L.vitx_model_rope_table.argtypes = [vp, ip, ip, C.POINTER(C.c_float), C.POINTER(C.c_float)]
            L.vitx_op_rope.argtypes = [ip, vp, C.c_long, vp, vp, ip, ip, ip, ip, ip, vp]
        if hasattr(L, "vitx_op_swiglu"):
            L.vitx_model_glu.argtypes = [vp, C.POINTER(ip), C.POINTER(ip)]
            L.vitx_op_swiglu.argtypes = [ip, vp, C.c_long, vp, C.c_long, C.c_long, ip, vp]
        if hasattr(L, "vitx_ctx_create_rect"):
            pp = C.POINTER(Preproc)
            L.vitx_ctx_create_rect.argtypes = [vp, ip, ip, ip, C.POINTER(CtxOptions), ip, ip, C.POINTER(vp)]
            L.vitx_ctx_img_shape.argtypes = [vp, C.POINTER(ip), C.POINTER(ip)]
            L.vitx_ctx_grid.argtypes = [vp, C.POINTER(ip), C.POINTER(ip)]
            L.vitx_op_patch_embed_rect.argtypes = [ip, vp, vp, vp, vp, vp, vp, ip, ip, ip, ip, ip, ip, ip, vp]
            L.vitx_rect_shape.argtypes = [ip, ip, ip, ip, ip, C.POINTER(ip), C.POINTER(ip)]
            L.vitx_preprocess_rect.argtypes = [pp, C.POINTER(C.c_uint8), ip, ip, ip, ip, C.POINTER(C.c_float)]
            L.vitx_preprocess_rect_device.argtypes = [pp, vp, ip, ip, ip, ip, ip, vp, vp]
            L.vitx_preprocess_rect_device_supports.argtypes = [pp, ip, ip, ip, ip]
        if hasattr(L, "vitx_pack_create"):
            i32p, fp = C.POINTER(C.c_int32), C.POINTER(C.c_float)
            L.vitx_pack_create.argtypes = [vp, ip, ip, ip, ip, C.POINTER(PackOptions), C.POINTER(vp)]
            L.vitx_pack_free.argtypes = [vp]
            L.vitx_pack_shares_weights.argtypes = [vp]
            L.vitx_pack_check.argtypes = [vp, i32p, ip, ip, ip, i32p]
            L.vitx_pack_distinct_grids.argtypes = [vp, i32p, ip]
            L.vitx_pack_forward.argtypes = [vp, fp, i32p, ip, fp, fp]
            L.vitx_pack_forward_device.argtypes = [vp, vp, i32p, ip, vp, vp, vp]
            L.vitx_pack_feat_enable.argtypes = [vp, ip]
            L.vitx_pack_feat_read.argtypes = [vp, fp, fp]
            L.vitx_pack_scratch_bytes.restype = C.c_size_t; L.vitx_pack_scratch_bytes.argtypes = [vp]
            L.vitx_pack_launches.argtypes = [vp, C.POINTER(ip)]
            L.vitx_op_attention_packed.argtypes = [ip, vp, vp, vp, ip, ip, ip, vp]
            L.vitx_op_attention_packed_tables.argtypes = [ip, vp, vp, vp, vp, ip, C.c_long, ip, ip, vp]
            L.vitx_op_rope_packed.argtypes =[ip, vp, C.c_long, vp, vp, vp, vp, ip, ip, ip, ip, vp]
        if hasattr(L, "vitx_pack_dense_set"):
            i32p, fp = C.POINTER(C.c_int32), C.POINTER(C.c_float)
            L.vitx_pack_dense_set.argtypes = [vp, fp, fp, ip, ip, C.c_uint64, C.c_long, ip]
            L.vitx_pack_dense_out.argtypes = [vp, i32p, ip]
            L.vitx_pack_dense_check.argtypes = [vp, i32p, i32p, ip, ip, C.c_long, C.POINTER(C.c_int64), i32p]
            L.vitx_pack_dense_read.argtypes = [vp, C.POINTER(C.c_uint8), fp, fp]
            L.vitx_pack_dense_device.restype = C.c_void_p; L.vitx_pack_dense_device.argtypes = [vp]
            L.vitx_pack_dense_scratch_bytes.restype = C.c_size_t; L.vitx_pack_dense_scratch_bytes.argtypes = [vp]
            L.vitx_op_dense_labels_packed.argtypes = [vp, C.c_long, i32p, i32p, i32p, ip, ip, vp, vp, vp]
            L.vitx_dense_pack_tables.argtypes = [i32p, i32p, i32p, ip, i32p, C.POINTER(ip), C.POINTER(ip)]
            L.vitx_op_dense_labels_packed_tables.argtypes = [vp, C.c_long, vp, ip, ip, ip, ip, vp, vp, vp]
        if hasattr(L, "vitx_pack_depth_set"):
            i32p, i64p, fp, cf = C.POINTER(C.c_int32), C.POINTER(C.c_int64), C.POINTER(C.c_float), C.c_float
            L.vitx_pack_depth_set.argtypes = [vp, fp, fp, fp, fp, ip, ip, C.c_uint64, ip, cf, cf, C.c_long, ip]
            L.vitx_pack_depth_out.argtypes = [vp, i32p, ip]
            L.vitx_pack_depth_check.argtypes = [vp, i32p, i32p, ip, ip, ip, C.c_long, i64p, i64p, i32p, i32p]
            L.vitx_pack_depth_read.argtypes = [vp, fp, fp, fp, fp]
            L.vitx_pack_depth_device.restype = C.c_void_p; L.vitx_pack_depth_device.argtypes = [vp]
            L.vitx_pack_depth_scratch_bytes.restype = C.c_size_t; L.vitx_pack_depth_scratch_bytes.argtypes = [vp]
            L.vitx_op_depth_fine_packed.argtypes = [vp, C.c_long, vp, vp, i32p, i32p, i32p, ip, ip, ip, vp, vp]
            L.vitx_op_depth_resize_packed.argtypes = [vp, i32p, i32p, ip, cf, cf, vp, vp]
            L.vitx_depth_pack_tables.argtypes = [i32p, i32p, i32p, i32p, ip, ip, i32p, C.POINTER(ip), C.POINTER(ip), C.POINTER(ip)]
            L.vitx_op_depth_fine_packed_tables.argtypes = [vp, C.c_long, vp, C.c_long, vp, vp, ip, ip, ip, ip, vp, vp]
            L.vitx_op_depth_resize_packed_tables.argtypes = [vp, vp, ip, ip, cf, cf, vp, vp]
        if hasattr(L, "vitx_pack_u8_set"):
            i32p, fp, pp = C.POINTER(C.c_int32), C.POINTER(C.c_float), C.POINTER(Preproc)
            L.vitx_pack_u8_set.argtypes = [vp, pp, C.c_size_t]
            L.vitx_pack_u8_sources.argtypes = [vp, i32p, ip]
            L.vitx_pack_forward_u8.argtypes = [vp, C.POINTER(C.c_uint8), i32p, i32p, ip, fp, fp]
            L.vitx_pack_u8_check.argtypes = [vp, pp, i32p, i32p, ip, C.c_size_t, C.POINTER(C.c_int64), i32p, C.POINTER(ip)]
            L.vitx_pack_fit_shapes.argtypes = [vp, i32p, ip, ip, ip, i32p]
            L.vitx_op_preprocess_pack.argtypes = [pp, vp, i32p, i32p, ip, vp]
        if hasattr(L, "vitx_pack_attn_enable"):
            i32p = C.POINTER(C.c_int32)
            L.vitx_pack_attn_enable.argtypes = [vp, C.c_uint64, ip, C.c_long]
            L.vitx_pack_attn_floats.argtypes = [vp]
            L.vitx_pack_attn_read.argtypes = [vp, C.POINTER(C.c_float), C.c_size_t]
            L.vitx_pack_attn_device.restype = C.c_void_p; L.vitx_pack_attn_device.argtypes = [vp]
            L.vitx_pack_attn_check.argtypes = [vp, i32p, ip, C.c_uint64, ip, C.c_long, i32p, i32p]
            L.vitx_op_attention_map_packed.argtypes = [ip, vp, vp, vp, i32p, ip, ip, ip, ip]
            L.vitx_op_rollout_step_packed.argtypes = [vp, vp, i32p, ip]
            L.vitx_op_rollout_row_packed.argtypes = [vp, vp, vp, i32p, ip, ip]
        _lib = L
    return _lib


def check(rc: int, what: str = "") -> None:
    if rc != 0:
        L = lib()
        e = VitxError(f"{what}: {L.vitx_status_str(rc).decode()} ({rc}): {L.vitx_last_error().decode()}")
        e.code = rc
        raise e


class Model:
    """Parsed weight file (vit_model_load, vit.cpp:308-712)."""

    def __init__(self, path: str):
        self._h = C.c_void_p()
        check(lib().vitx_model_load(path.encode(), C.byref(self._h)), f"vitx_model_load({path})")
        hp = HParams(); lib().vitx_model_hparams(self._h, C.byref(hp))
        self.hparams = hp
        self.path = path

    def close(self):
        if getattr(self, "_h", None) and self._h:
            lib().vitx_model_free(self._h); self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:       # interpreter shutdown: module globals may already be gone
            pass

    @property
    def kind(self) -> int: return lib().vitx_model_kind(self._h)                    # KIND_IMAGE, or KIND_TEXT for a text-tower file (patch_size 0)

    @property
    def text_info(self) -> dict:
        """{"vocab", "tokens", "causal", "eos"} of a text-tower file (eos -1: the last position is pooled); VitxError for an image file."""
        v = [C.c_int() for _ in range(4)]
        check(lib().vitx_model_text_info(self._h, *[C.byref(x) for x in v]), "vitx_model_text_info")
        return dict(vocab=v[0].value, tokens=v[1].value, causal=v[2].value, eos=v[3].value)

    @property
    def text_zs(self):
        """(kind, scale, bias) of a text-tower file's `zs` tensor, or None."""
        k, s, b = C.c_int(), C.c_float(), C.c_float()
        return (k.value, s.value, b.value) if lib().vitx_model_text_zs(self._h, C.byref(k), C.byref(s), C.byref(b)) else None

    @property
    def in_channels(self) -> int: return lib().vitx_model_in_channels(self._h)      # 3, or 1 for a ViTSTR file
    @property
    def seq_len(self) -> int: return lib().vitx_model_seq_len(self._h)              # 0 (classifier) or 25 (ViTSTR: rows per image)
    @property
    def num_registers(self) -> int:                                                 # register tokens (reg_token [1][R][D]); 0 without
        return lib().vitx_model_num_registers(self._h) if hasattr(lib(), "vitx_model_num_registers") else 0
    @property
    def head_pool(self) -> int:                                                     # POOL_CLS, or POOL_CLS_MEAN for a [C][2 D] head
        return lib().vitx_model_head_pool(self._h) if hasattr(lib(), "vitx_model_head_pool") else 0
    @property
    def num_prefix(self) -> int:                                                    # tokens in front of the patches: 1 + registers, or 0 for a POOL_MAP file
        return lib().vitx_model_num_prefix(self._h) if hasattr(lib(), "vitx_model_num_prefix") else 1 + self.num_registers

    def pool_query(self) -> np.ndarray:
        """vitx_model_pool_query: u [H, D] f32 of a POOL_MAP file, u_h = Wk_h^T q_h / sqrt(d) (the probe folded through the K projection)."""
        hp = self.hparams
        u = np.empty((hp.num_attention_heads, hp.hidden_size), np.float32)
        check(lib().vitx_model_pool_query(self._h, u.ctypes.data_as(C.POINTER(C.c_float))), "vitx_model_pool_query")
        return u

    @property
    def rope(self):
        """(kind, theta) of a file with a `rope` tensor (rotary position embeddings on q and k of the patch tokens), or None."""
        k, t = C.c_int(), C.c_float()
        return (k.value, t.value) if lib().vitx_model_rope(self._h, C.byref(k), C.byref(t)) else None

    @property
    def glu(self):
        """(kind, F) of a file with a `glu` tensor (a gated MLP of hidden width F: fc1 is [2 F][D], fc2 [D][F]), or None."""
        k, w = C.c_int(), C.c_int()
        return (k.value, w.value) if lib().vitx_model_glu(self._h, C.byref(k), C.byref(w)) else None

    def rope_table(self, grid) -> Tuple[np.ndarray, np.ndarray]:
        """vitx_model_rope_table: (cos, sin), each f32 [gh * gw, head_dim / 2], for a grid g or (gh, gw); row-major over (y, x)."""
        gh, gw = _grid(grid)
        hp = self.hparams
        half = hp.hidden_size // hp.num_attention_heads // 2
        fp = C.POINTER(C.c_float)
        cos = np.empty((max(gh, 0) * max(gw, 0), half), np.float32); sin = np.empty_like(cos)
        check(lib().vitx_model_rope_table(self._h, gh, gw, cos.ctypes.data_as(fp), sin.ctypes.data_as(fp)), "vitx_model_rope_table")
        return cos, sin

    @property
    def activation(self) -> int:                                                    # ACT_GELU_TANH / ACT_GELU_ERF / ACT_QUICK_GELU (the file's `arch`)
        return lib().vitx_model_activation(self._h) if hasattr(lib(), "vitx_model_activation") else 0
    @property
    def has_pre_norm(self) -> bool:                                                 # pre_norm.weight / pre_norm.bias: CLIP's pre_layrnorm
        return bool(lib().vitx_model_has_pre_norm(self._h)) if hasattr(lib(), "vitx_model_has_pre_norm") else False
    @property
    def has_preproc(self) -> bool:                                                  # the file carries a `preproc` tensor
        return bool(lib().vitx_model_has_preproc(self._h))

    def preproc(self) -> "Preproc":
        """vitx_model_preproc: the file's preprocessing; without the tensor the reference default (stretch, REF_BICUBIC, ImageNet mean / std)."""
        pp = Preproc()
        check(lib().vitx_model_preproc(self._h, C.byref(pp)), "vitx_model_preproc")
        return pp

    @property
    def num_classes(self) -> int: return self.hparams.num_classes
    @property
    def img_size(self) -> int: return self.hparams.img_size

    def label(self, i: int) -> Optional[str]:
        s = lib().vitx_model_label(self._h, i)
        return s.decode() if s is not None else None

    def tensors(self) -> List[Tuple[str, int, Tuple[int, ...], int]]:
        out = []
        for i in range(lib().vitx_model_num_tensors(self._h)):
            name = C.c_char_p(); t = C.c_int32(); ne = (C.c_int64 * 4)(); nb = C.c_size_t()
            check(lib().vitx_model_tensor_info(self._h, i, C.byref(name), C.byref(t), ne, C.byref(nb)))
            out.append((name.value.decode(), t.value, tuple(ne), nb.value))
        return out

    def tensor_f32(self, index: int) -> np.ndarray:
        _, _, ne, _ = self.tensors()[index]
        n = int(np.prod(ne)); a = np.empty(n, np.float32)
        check(lib().vitx_model_tensor_f32(self._h, index, a.ctypes.data_as(C.POINTER(C.c_float)), n))
        return a.reshape(tuple(reversed(ne)))


def quantize_file(path_in: str, path_out: str, ftype: int) -> None:
    """Native `quantize` (quantize.cpp:34-353): f16/f32 file -> q4_0/q4_1/q5_0/q5_1/q8_0 file."""
    check(lib().vitx_quantize_file(path_in.encode(), path_out.encode(), ftype), "vitx_quantize_file")


def resize_file(path_in: str, path_out: str, img_size: int, interp: int = POS_BICUBIC) -> None:
    """vitx_model_resize_file: the same model at another img_size (pos_embed resampled on the host, every other byte copied through)."""
    check(lib().vitx_model_resize_file(path_in.encode(), path_out.encode(), img_size, interp), "vitx_model_resize_file")


def _grid(g) -> Tuple[int, int]:
    return (int(g), int(g)) if np.isscalar(g) else (int(g[0]), int(g[1]))


def _layer_mask(layers, prefix: str = "", span: str = "0 .. 63") -> int:
    """Layer indices -> the layer mask of the C API (bit l = layer l); `prefix` and `span` are the caller's spelling of the ValueError."""
    mask = 0
    for l in layers:
        if not 0 <= int(l) < 64:
            raise ValueError(f"{prefix}layer {l} outside {span}")
        mask |= 1 << int(l)
    return mask


def _head_arrays(prefix: str, weight, bias):
    """(weight [K, Dc], bias [K] or None) of a linear head as contiguous f32 arrays, or ValueError."""
    w = np.ascontiguousarray(weight, dtype=np.float32)
    if w.ndim != 2:
        raise ValueError(f"{prefix}weight must be [K, Dc]")
    b = None
    if bias is not None:
        b = np.ascontiguousarray(bias, dtype=np.float32)
        if b.shape != (w.shape[0],):
            raise ValueError(f"{prefix}bias must be [K]")
    return w, b


def pos_embed_resample(pos: np.ndarray, grid_out, interp: int = POS_BICUBIC, grid_in=None) -> np.ndarray:
    """vitx_pos_embed_resample on the host: pos [1 + gy * gx, D] f32 (row 0 = class token) -> [1 + gy' * gx', D].  grid_out (and grid_in) are a
    side or a (gy, gx) pair; grid_in defaults to the square grid the row count implies."""
    p = np.ascontiguousarray(pos, np.float32)
    if p.ndim != 2:
        raise ValueError(f"pos must be [1 + gy * gx, D], got {p.shape}")
    if grid_in is None:
        g = int(round((p.shape[0] - 1) ** 0.5)); grid_in = (g, g)
    (gy, gx), (oy, ox) = _grid(grid_in), _grid(grid_out)
    if 1 + gy * gx != p.shape[0]:
        raise ValueError(f"pos has {p.shape[0]} rows, a {gy} x {gx} grid needs {1 + gy * gx}")
    out = np.empty((1 + max(oy, 0) * max(ox, 0), p.shape[1]), np.float32)
    fp = C.POINTER(C.c_float)
    check(lib().vitx_pos_embed_resample(p.ctypes.data_as(fp), gy, gx, p.shape[1], oy, ox, interp, out.ctypes.data_as(fp)), "vitx_pos_embed_resample")
    return out


def op_pos_embed_resample(d_pos: int, grid_in, D: int, grid_out, interp: int, d_out: int, stream: int = 0) -> None:
    """vitx_op_pos_embed_resample: the device kernel (device pointers, same arguments and bits as pos_embed_resample; only enqueues)."""
    (gy, gx), (oy, ox) = _grid(grid_in), _grid(grid_out)
    check(lib().vitx_op_pos_embed_resample(d_pos, gy, gx, D, oy, ox, interp, d_out, stream or None), "vitx_op_pos_embed_resample")


def load_image(path: str) -> np.ndarray:
    """load_image_from_file (vit.cpp:109-127): JPEG / PNG / PPM file -> HWC u8 RGB, decoded by libvitx.so itself."""
    data = C.POINTER(C.c_uint8)(); nx = C.c_int(); ny = C.c_int()
    check(lib().vitx_image_load(path.encode(), C.byref(data), C.byref(nx), C.byref(ny)), f"vitx_image_load({path})")
    try:
        return np.ctypeslib.as_array(data, shape=(ny.value, nx.value, 3)).copy()
    finally:
        lib().vitx_image_free(data)


def decode_image(blob: bytes) -> np.ndarray:
    data = C.POINTER(C.c_uint8)(); nx = C.c_int(); ny = C.c_int()
    check(lib().vitx_image_decode(blob, len(blob), C.byref(data), C.byref(nx), C.byref(ny)), "vitx_image_decode")
    try:
        return np.ctypeslib.as_array(data, shape=(ny.value, nx.value, 3)).copy()
    finally:
        lib().vitx_image_free(data)


def preprocess(img_u8: np.ndarray, img_size: int, interp: int = BICUBIC) -> np.ndarray:
    """vit_image_preprocess (vit.cpp:289-305): HWC u8 any size -> HWC f32 [S,S,3]."""
    img = np.ascontiguousarray(img_u8, np.uint8); ny, nx = img.shape[:2]
    out = np.empty((img_size, img_size, 3), np.float32)
    check(lib().vitx_preprocess_u8(img.ctypes.data_as(C.POINTER(C.c_uint8)), nx, ny, img_size, interp, out.ctypes.data_as(C.POINTER(C.c_float))), "vitx_preprocess_u8")
    return out


def preproc_at_size(pp: Preproc, img_size: int) -> Preproc:
    """vitx_preproc_at_size: the description for a context at another img_size (the crop fraction is kept, rounded to nearest)."""
    out = Preproc()
    check(lib().vitx_preproc_at_size(C.byref(pp), img_size, C.byref(out)), "vitx_preproc_at_size")
    return out


def preprocess_ex(img_u8: np.ndarray, pp: Preproc) -> np.ndarray:
    """vitx_preprocess_ex: HWC u8 any size -> HWC f32 [S,S,3] by the description (resize, centre crop, mean / std), on the host."""
    img = np.ascontiguousarray(img_u8, np.uint8); ny, nx = img.shape[:2]
    S = max(int(pp.out_size), 1)
    out = np.empty((S, S, 3), np.float32)
    check(lib().vitx_preprocess_ex(C.byref(pp), img.ctypes.data_as(C.POINTER(C.c_uint8)), nx, ny, out.ctypes.data_as(C.POINTER(C.c_float))), "vitx_preprocess_ex")
    return out


def preprocess_ex_device(pp: Preproc, d_u8: int, n: int, nx: int, ny: int, d_out: int, stream: int = 0) -> None:
    """vitx_preprocess_ex_device: the same on the GPU for n images of one source size (device pointers; one launch, enqueue only)."""
    check(lib().vitx_preprocess_ex_device(C.byref(pp), d_u8, n, nx, ny, d_out, stream or None), "vitx_preprocess_ex_device")


def preprocess_ex_device_supports(pp: Preproc, nx: int, ny: int) -> bool:
    """vitx_preprocess_ex_device_supports: whether the device kernel's LDS tile covers this down-scale (no device call)."""
    return bool(lib().vitx_preprocess_ex_device_supports(C.byref(pp), nx, ny))


def rect_shape(nx: int, ny: int, patch: int, short_side: int, max_long: int = 0) -> Tuple[int, int]:
    """vitx_rect_shape: the aspect-preserving (out_w, out_h) for an nx x ny source: the short side becomes short_side, the long side the largest
    multiple of patch that keeps the aspect (capped at max_long when that is not 0).  500 x 375, patch 16, short 224 -> (288, 224)."""
    w, h = C.c_int(), C.c_int()
    check(lib().vitx_rect_shape(nx, ny, patch, short_side, max_long, C.byref(w), C.byref(h)), "vitx_rect_shape")
    return w.value, h.value


def preprocess_rect(img_u8: np.ndarray, pp: Preproc, out_w: int, out_h: int) -> np.ndarray:
    """vitx_preprocess_rect: HWC u8 any size -> HWC f32 [out_h, out_w, 3], stretched with the description's PIL filter, mean / std; no crop."""
    img = np.ascontiguousarray(img_u8, np.uint8); ny, nx = img.shape[:2]
    out = np.empty((max(int(out_h), 1), max(int(out_w), 1), 3), np.float32)
    check(lib().vitx_preprocess_rect(C.byref(pp), img.ctypes.data_as(C.POINTER(C.c_uint8)), nx, ny, out_w, out_h, out.ctypes.data_as(C.POINTER(C.c_float))), "vitx_preprocess_rect")
    return out


def preprocess_rect_device(pp: Preproc, d_u8: int, n: int, nx: int, ny: int, out_w: int, out_h: int, d_out: int, stream: int = 0) -> None:
    """vitx_preprocess_rect_device: the same on the GPU for n images of one source size (device pointers; one launch, enqueue only)."""
    check(lib().vitx_preprocess_rect_device(C.byref(pp), d_u8, n, nx, ny, out_w, out_h, d_out, stream or None), "vitx_preprocess_rect_device")


def preprocess_rect_device_supports(pp: Preproc, nx: int, ny: int, out_w: int, out_h: int) -> bool:
    """vitx_preprocess_rect_device_supports: whether the device kernel's LDS tile covers this down-scale (no device call)."""
    return bool(lib().vitx_preprocess_rect_device_supports(C.byref(pp), nx, ny, out_w, out_h))


def preprocess_vitstr(img_u8: np.ndarray, img_size: int) -> np.ndarray:
    """vit_image_preprocess of extensions/vitstr.cpp (vitstr.cpp:135-201): HWC u8 RGB -> [S,S] f32 grey in [-1, 1]."""
    img = np.ascontiguousarray(img_u8, np.uint8); ny, nx = img.shape[:2]
    out = np.empty((img_size, img_size), np.float32)
    check(lib().vitx_preprocess_vitstr_u8(img.ctypes.data_as(C.POINTER(C.c_uint8)), nx, ny, img_size, out.ctypes.data_as(C.POINTER(C.c_float))), "vitx_preprocess_vitstr_u8")
    return out


def vitstr_decode(probs: np.ndarray):
    """Greedy decode of one image's [25, C] probabilities (vitstr.cpp:1025-1051) -> (class ids, score)."""
    p = np.ascontiguousarray(probs, np.float32); R, Cn = p.shape
    ids = (C.c_int32 * R)(); n = C.c_int(); score = C.c_double()
    check(lib().vitx_vitstr_decode(p.ctypes.data_as(C.POINTER(C.c_float)), R, Cn, ids, C.byref(n), C.byref(score)), "vitx_vitstr_decode")
    return list(ids)[:n.value], score.value


def preprocess_device(d_u8: int, n: int, nx: int, ny: int, img_size: int, d_out: int, interp: int = BICUBIC, stream: int = 0) -> None:
    """vit_image_preprocess on the GPU (device pointers; enqueue only)."""
    check(lib().vitx_preprocess_u8_device(d_u8, n, nx, ny, img_size, interp, d_out, stream or None), "vitx_preprocess_u8_device")


def _check_image_shape(model: "Model", x: np.ndarray, img_size=None) -> None:
    """[n, h, w, 3] for a classifier, [n, S, S] (one grey plane) for a ViTSTR file: the C ABI reads n * h * w * in_channels floats.
    img_size is the context's side S (h = w = S) or its (h, w) shape (a Group runs at the file's)."""
    h, w = _grid(model.img_size if img_size is None else img_size)
    want = (h, w, 3) if model.in_channels == 3 else (h, w)
    if x.ndim != 1 + len(want) or tuple(x.shape[1:]) != want:
        raise ValueError(f"images must be [n, {', '.join(map(str, want))}] for this model, got {tuple(x.shape)}")


class Context:
    """Per-(thread, GPU) execution context (vit_state): weights in HBM + activation scratch."""

    def __init__(self, model: Model, device: int = 0, max_batch: int = 1, dtype: int = F16, img_shape=None, **options):
        """options: the fields of vitx_ctx_options (streams, graph, quant_on_host, q4_fused_rows, split_first, no_ln_fusion, ...,
        img_size, pos_interp: a context at another input size than the file's, on the position table resampled to its grid).
        img_shape = (h, w): a rectangular context (vitx_ctx_create_rect) for [n, h, w, 3] images; not together with img_size."""
        if img_shape is not None and options.get("img_size"):
            raise ValueError("img_shape and img_size cannot both be given")
        self.model = model; self.device = device; self.max_batch = max_batch; self.dtype = dtype
        self._h = C.c_void_p()
        opt = CtxOptions(struct_size=C.sizeof(CtxOptions))
        for k, v in options.items():
            if k not in dict(CtxOptions._fields_) or k == "struct_size":
                raise TypeError(f"unknown context option {k!r}")
            setattr(opt, k, int(v))
        # struct_size = the smallest prefix that covers every field that is set: a library that predates a trailing field (tools/ab_libs.py loads
        # older builds through VITX_LIB) rejects a struct_size above its own sizeof(vitx_ctx_options) -- zero trailing fields are its defaults anyway
        names = [f for f, _ in CtxOptions._fields_]
        last = max([i for i, f in enumerate(names) if f != "struct_size" and getattr(opt, f) != 0] + [names.index("f16_fast_attention")])
        opt.struct_size = 4 * (last + 1)
        if img_shape is not None:
            ih, iw = (int(v) for v in img_shape)
            check(lib().vitx_ctx_create_rect(model._h, device, max_batch, dtype, C.byref(opt), ih, iw, C.byref(self._h)), "vitx_ctx_create_rect")
        else:
            check(lib().vitx_ctx_create_ex(model._h, device, max_batch, dtype, C.byref(opt), C.byref(self._h)), "vitx_ctx_create_ex")
        # the geometry of THIS context (vitx_ctx_options::img_size); a build that predates the option runs at the file's
        L = lib()
        self.img_size = int(L.vitx_ctx_img_size(self._h)) if hasattr(L, "vitx_ctx_img_size") else model.img_size
        self.tokens = int(L.vitx_ctx_tokens(self._h)) if hasattr(L, "vitx_ctx_tokens") else (model.img_size // model.hparams.patch_size) ** 2 + 1
        self.grid = self.img_size // model.hparams.patch_size      # the side of a square context's grid; 0 for a non-square context (grid_hw)
        # img_shape = (h, w) and grid_hw = (gh, gw) of any context; img_size is 0 for a non-square one
        self.img_shape = (self.img_size, self.img_size); self.grid_hw = (self.grid, self.grid)
        if hasattr(L, "vitx_ctx_img_shape"):
            a, b = C.c_int(), C.c_int()
            check(L.vitx_ctx_img_shape(self._h, C.byref(a), C.byref(b)), "vitx_ctx_img_shape"); self.img_shape = (a.value, b.value)
            check(L.vitx_ctx_grid(self._h, C.byref(a), C.byref(b)), "vitx_ctx_grid"); self.grid_hw = (a.value, b.value)
        self.registers = int(L.vitx_ctx_registers(self._h)) if hasattr(L, "vitx_ctx_registers") else 0
        self.prefix = model.num_prefix                # tokens in front of the patches: the class token and the registers (0 for a POOL_MAP model)

    def close(self):
        if getattr(self, "_h", None) and self._h:
            lib().vitx_ctx_free(self._h); self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def forward(self, imgs_hwc: np.ndarray, want_logits: bool = False):
        """Host arrays in/out (copies + sync): [n,h,w,3] f32 (the context's img_shape) -> probs [n,C] (and logits)."""
        x = np.ascontiguousarray(imgs_hwc, np.float32); n = x.shape[0]
        _check_image_shape(self.model, x, self.img_shape)
        R = self.model.seq_len                      # ViTSTR: [n, S, S] grey in, [n, 25, C] out
        probs = np.empty((n, self.model.num_classes) if R == 0 else (n, R, self.model.num_classes), np.float32)
        logits = np.empty_like(probs) if want_logits else None
        fp = C.POINTER(C.c_float)
        check(lib().vitx_forward(self._h, x.ctypes.data_as(fp), n, probs.ctypes.data_as(fp), logits.ctypes.data_as(fp) if want_logits else None), "vitx_forward")
        return (probs, logits) if want_logits else probs

    def forward_device(self, d_imgs: int, n: int, d_probs: int, d_logits: int = 0, stream: int = 0) -> None:
        """Device pointers; only enqueues on `stream` (0 = the context's own stream)."""
        check(lib().vitx_forward_device(self._h, d_imgs, n, d_probs, d_logits or None, stream or None), "vitx_forward_device")

    def trace_enable(self, image_ids) -> None:
        """Record the f32 residual stream of these images after the patch embedding and after every layer (vitx_trace_enable)."""
        ids = (C.c_int32 * len(image_ids))(*image_ids)
        check(lib().vitx_trace_enable(self._h, ids, len(image_ids)), "vitx_trace_enable")
        self._trace_n = len(image_ids)

    def trace_read(self) -> np.ndarray:
        """[L + 1, n_ids, tokens, hidden] f32 of the last forward."""
        hp = self.model.hparams
        N = self.tokens
        out = np.empty((hp.num_hidden_layers + 1, self._trace_n, N, hp.hidden_size), np.float32)
        check(lib().vitx_trace_read(self._h, out.ctypes.data_as(C.POINTER(C.c_float)), out.size), "vitx_trace_read")
        return out

    def attn_enable(self, layers=None, rollout: bool = False) -> None:
        """Attention maps of every later forward (vitx_attn_enable): the class-token maps of `layers` (None = every layer, [] = none) and,
        with rollout=True, the attention-rollout row.  attn_enable([]) turns them off and frees the buffers."""
        L = self.model.hparams.num_hidden_layers
        sel = list(range(L)) if layers is None else sorted(set(int(l) for l in layers))
        mask = _layer_mask(sel, span="0..63")
        check(lib().vitx_attn_enable(self._h, mask, ATTN_ROLLOUT if rollout else 0), "vitx_attn_enable")
        self._attn_layers, self._attn_rollout = sel, bool(rollout)

    def attn_disable(self) -> None:
        self.attn_enable([], rollout=False)

    def attn_read(self, n: Optional[int] = None):
        """Maps of the last forward made with maps on, all of its n images: (cls [n, n_sel, H, N] f32, rollout [n, N] f32 or None).
        Index 0 of a map is the class token, 1 .. registers the register tokens (models that have them), then the patches in raster order
        (attn_grid reshapes).  `n`, if given, must be that batch."""
        hp = self.model.hparams
        N, H = self.tokens, hp.num_attention_heads
        fpi = lib().vitx_attn_floats(self._h)
        sel, roll = getattr(self, "_attn_layers", []), getattr(self, "_attn_rollout", False)
        assert fpi == len(sel) * H * N + (N if roll else 0)
        have = lib().vitx_attn_images(self._h)
        if n is not None and n != have:
            raise ValueError(f"attn_read: the last forward with maps on had {have} images, not {n}")
        n = have
        if n == 0:
            raise VitxError("attn_read: no forward has run with attention maps on since attn_enable")
        out = np.empty((n, fpi), np.float32)
        check(lib().vitx_attn_read(self._h, out.ctypes.data_as(C.POINTER(C.c_float)), out.size), "vitx_attn_read")
        cls = out[:, :len(sel) * H * N].reshape(n, len(sel), H, N)
        return cls, (out[:, len(sel) * H * N:].copy() if roll else None)

    def attn_grid(self, m: np.ndarray) -> np.ndarray:
        """[..., N] map -> [..., gh, gw] patch grid (the context's grid_hw; g x g for a square context): drops the class token and the register tokens."""
        gh, gw = self.grid_hw
        return np.asarray(m)[..., self.prefix:].reshape(*np.shape(m)[:-1], gh, gw)

    def feat_enable(self, cls: bool = True, mean: bool = False, tokens: bool = False, l2: bool = False, layers=None) -> None:
        """Embeddings and token features of every later forward (vitx_feat_enable): the final-norm class embedding, the mean of the patch
        features and / or the patch features themselves, of `layers` (None = the last layer).  l2=True divides cls and mean by their norm.
        mean or tokens of the last layer make it compute every row (the probabilities of a last_layer_all_rows=1 context)."""
        L = self.model.hparams.num_hidden_layers
        sel = [L - 1] if layers is None else sorted(set(int(l) for l in layers))
        mask = _layer_mask(sel, span="0..63")
        flags = (FEAT_CLS if cls else 0) | (FEAT_MEAN if mean else 0) | (FEAT_TOKENS if tokens else 0) | (FEAT_L2 if l2 else 0)
        if not sel:
            raise ValueError("feat_enable: no layer selected (feat_disable() turns the features off)")
        check(lib().vitx_feat_enable(self._h, flags, mask), "vitx_feat_enable")
        self._feat_layers, self._feat_flags = (sel if flags else []), flags

    def feat_disable(self) -> None:
        check(lib().vitx_feat_enable(self._h, 0, 0), "vitx_feat_enable")
        self._feat_layers, self._feat_flags = [], 0

    def feat_read(self, n: Optional[int] = None):
        """Features of the last forward made with features on, all of its n images: {layer: {"cls": [n, D], "mean": [n, D],
        "tokens": [n, N - T, D]}} f32 with the selected kinds only (T = 1 + registers: the patch rows).  `n`, if given, must be that batch."""
        hp = self.model.hparams
        N, D, T = self.tokens, hp.hidden_size, self.prefix
        sel, flags = getattr(self, "_feat_layers", []), getattr(self, "_feat_flags", 0)
        fpi = lib().vitx_feat_floats(self._h)
        have = lib().vitx_feat_images(self._h)
        if n is not None and n != have:
            raise ValueError(f"feat_read: the last forward with features on had {have} images, not {n}")
        n = have
        if n == 0:
            raise VitxError("feat_read: no forward has run with features on since feat_enable")
        out = np.empty((n, fpi), np.float32)
        check(lib().vitx_feat_read(self._h, out.ctypes.data_as(C.POINTER(C.c_float)), out.size), "vitx_feat_read")
        kinds = [(k, rows) for k, bit, rows in (("cls", FEAT_CLS, 1), ("mean", FEAT_MEAN, 1), ("tokens", FEAT_TOKENS, N - T)) if flags & bit]
        assert fpi == len(sel) * D * sum(rows for _, rows in kinds)
        res, off = {}, 0
        for l in sel:
            res[l] = {}
            for k, rows in kinds:
                v = out[:, off:off + rows * D]
                res[l][k] = v.reshape(n, N - T, D) if k == "tokens" else v
                off += rows * D
        return res

    def feat_device(self) -> Tuple[int, int]:
        """(device pointer of the feature buffer [capacity][floats per image] f32, floats per image) for callers that stay on the GPU
        (vitx_feat_device); the layout per image is feat_read()'s order.  Ordered after the forward's stream, like d_probs."""
        return int(lib().vitx_feat_device(self._h) or 0), int(lib().vitx_feat_floats(self._h))

    def zeroshot_set(self, embeds: Optional[np.ndarray], kind: int = ZS_SOFTMAX, scale: float = 1.0, bias: float = 0.0) -> None:
        """Zero-shot logits and probabilities of every later forward against the bank `embeds` [K, E] f32 of unit-length class embeddings
        (vitx_zeroshot_set; E = the context's embedding width: num_classes of a CLIP file, hidden_size of a SigLIP file).  kind ZS_SOFTMAX /
        ZS_SIGMOID, scale = exp(logit_scale), bias = logit_bias.  None turns the output off and frees its buffers."""
        if embeds is None:
            check(lib().vitx_zeroshot_set(self._h, None, 0, 0, 0, 0.0, 0.0), "vitx_zeroshot_set")
            return
        e = np.ascontiguousarray(embeds, dtype=np.float32)
        if e.ndim != 2:
            raise ValueError("zeroshot_set: embeds must be [K, E]")
        check(lib().vitx_zeroshot_set(self._h, e.ctypes.data_as(C.POINTER(C.c_float)), e.shape[0], e.shape[1], int(kind), float(scale), float(bias)), "vitx_zeroshot_set")

    def zeroshot_read(self, n: Optional[int] = None, want_logits: bool = False):
        """Zero-shot probabilities [n, K] f32 of the last forward made with a bank set (and, want_logits, the logits).  `n`, if given, must be that batch."""
        K, have = lib().vitx_zeroshot_classes(self._h), lib().vitx_zeroshot_images(self._h)
        if n is not None and n != have:
            raise ValueError(f"zeroshot_read: the last forward with a bank set had {have} images, not {n}")
        probs = np.empty((max(have, 1), max(K, 1)), np.float32)
        logits = np.empty_like(probs) if want_logits else None
        fp = C.POINTER(C.c_float)
        check(lib().vitx_zeroshot_read(self._h, probs.ctypes.data_as(fp), logits.ctypes.data_as(fp) if want_logits else None, have * K), "vitx_zeroshot_read")
        return (probs, logits) if want_logits else probs

    def zeroshot_device(self) -> Tuple[int, int]:
        """(device pointer of the zero-shot buffer [capacity][2][K] f32 -- per image the probabilities, then the logits --, K) for callers that
        stay on the GPU (vitx_zeroshot_device).  Ordered after the forward's stream, like d_probs."""
        return int(lib().vitx_zeroshot_device(self._h) or 0), int(lib().vitx_zeroshot_classes(self._h))

    def nn_width(self, source: int) -> int:
        """vitx_nn_width: the width E of the source embedding (NN_LOGITS: num_classes; NN_EMBED: the head operand's, D or 2 D)."""
        return int(lib().vitx_nn_width(self._h, int(source)))

    def nn_set(self, gallery: Optional[np.ndarray], k: int = 1, source: int = NN_EMBED, labels=None, n_labels: int = 0, temperature: float = 0.07) -> None:
        """The k nearest rows of `gallery` [G, E] f32 (unit rows: the engine does not renormalise them) for every image of every later forward, and --
        labels [G] i32 in [0, n_labels) -- the temperature-weighted vote of their labels (vitx_nn_set).  None turns the output off and frees its buffers."""
        if gallery is None:
            check(lib().vitx_nn_set(self._h, None, 0, 0, 0, 0, None, 0, 0.0), "vitx_nn_set")
            return
        g = np.ascontiguousarray(gallery, dtype=np.float32)
        if g.ndim != 2:
            raise ValueError("nn_set: gallery must be [G, E]")
        lab = None
        if labels is not None:
            lab = np.ascontiguousarray(labels, dtype=np.int32)
            if lab.shape != (g.shape[0],):
                raise ValueError("nn_set: labels must be [G]")
        check(lib().vitx_nn_set(self._h, g.ctypes.data_as(C.POINTER(C.c_float)), g.shape[0], g.shape[1], int(k), int(source),
                                lab.ctypes.data_as(C.POINTER(C.c_int32)) if lab is not None else None, int(n_labels), float(temperature)), "vitx_nn_set")

    def nn_read(self, n: Optional[int] = None):
        """(idx [n, k] i32, score [n, k] f32, vote [n, n_labels] f32 or None) of the last forward made with a gallery set, best first.  `n`, if given,
        must be that batch."""
        L = lib()
        k, nl, have = L.vitx_nn_k(self._h), L.vitx_nn_labels(self._h), L.vitx_nn_images(self._h)
        if n is not None and n != have:
            raise ValueError(f"nn_read: the last forward with a gallery set had {have} images, not {n}")
        idx = np.empty((max(have, 1), max(k, 1)), np.int32)
        score = np.empty(idx.shape, np.float32)
        vote = np.empty((max(have, 1), nl), np.float32) if nl else None
        check(L.vitx_nn_read(self._h, idx.ctypes.data_as(C.POINTER(C.c_int32)), score.ctypes.data_as(C.POINTER(C.c_float)),
                             vote.ctypes.data_as(C.POINTER(C.c_float)) if nl else None), "vitx_nn_read")
        return idx, score, vote

    def nn_device(self) -> Tuple[int, int]:
        """(device pointer of the result [capacity][k] {f32 score, i32 index}, k) for callers that stay on the GPU (vitx_nn_device); (0, 0) while off."""
        return int(lib().vitx_nn_device(self._h) or 0), int(lib().vitx_nn_k(self._h))

    def nn_scratch_bytes(self) -> int:
        return int(lib().vitx_nn_scratch_bytes(self._h))

    def dense_set(self, weight: Optional[np.ndarray], bias: Optional[np.ndarray] = None, layers=None, out_shape: Optional[Tuple[int, int]] = None,
                  score: bool = False, logits: bool = False) -> None:
        """A linear head `weight` [K, Dc] f32 (+ `bias` [K]) over the patch tokens of `layers` (indices; None: the last layer) for every later forward:
        per image a label map [out_h, out_w] u8 (`out_shape` None: the context's image shape), with `score` the winner's value, with `logits` the patch
        logits (vitx_dense_set).  weight None turns the output off and frees its buffers."""
        if weight is None:
            check(lib().vitx_dense_set(self._h, None, None, 0, 0, 0, 0, 0, 0), "vitx_dense_set")
            return
        w, b = _head_arrays("dense_set: ", weight, bias)
        mask = _layer_mask([] if layers is None else layers, "dense_set: ")
        oh, ow = (0, 0) if out_shape is None else (int(out_shape[0]), int(out_shape[1]))
        fp = C.POINTER(C.c_float)
        check(lib().vitx_dense_set(self._h, w.ctypes.data_as(fp), b.ctypes.data_as(fp) if b is not None else None, w.shape[0], w.shape[1], mask, oh, ow,
                                   (DENSE_SCORE if score else 0) | (DENSE_LOGITS if logits else 0)), "vitx_dense_set")
        self._dense_flags = (bool(score), bool(logits))

    def dense_shape(self) -> Tuple[int, int]:
        oh, ow = C.c_int(0), C.c_int(0)
        check(lib().vitx_dense_shape(self._h, C.byref(oh), C.byref(ow)), "vitx_dense_shape")
        return oh.value, ow.value

    def dense_read(self, n: Optional[int] = None):
        """(labels [n, out_h, out_w] u8, score [n, out_h, out_w] f32 or None, logits [n, Np, K] f32 or None) of the last forward made with a dense head
        set.  `n`, if given, must be that batch."""
        L = lib()
        have, K = L.vitx_dense_images(self._h), L.vitx_dense_classes(self._h)
        if n is not None and n != have:
            raise ValueError(f"dense_read: the last forward with a dense head set had {have} images, not {n}")
        oh, ow = self.dense_shape()
        gh, gw = self.grid_hw
        want_score, want_logits = getattr(self, "_dense_flags", (False, False)) if K else (False, False)
        labels = np.empty((max(have, 1), max(oh, 1), max(ow, 1)), np.uint8)
        score = np.empty(labels.shape, np.float32) if want_score else None
        logits = np.empty((max(have, 1), gh * gw, max(K, 1)), np.float32) if want_logits else None
        fp = C.POINTER(C.c_float)
        check(L.vitx_dense_read(self._h, labels.ctypes.data_as(C.POINTER(C.c_uint8)), score.ctypes.data_as(fp) if want_score else None,
                                logits.ctypes.data_as(fp) if want_logits else None), "vitx_dense_read")
        return labels, score, logits

    def dense_device(self) -> Tuple[int, Tuple[int, int]]:
        """(device pointer of the labels [capacity][out_h][out_w] u8, (out_h, out_w)) for callers that stay on the GPU; (0, (0, 0)) while off."""
        return int(lib().vitx_dense_device(self._h) or 0), self.dense_shape()

    def dense_scratch_bytes(self) -> int:
        return int(lib().vitx_dense_scratch_bytes(self._h))

    def depth_set(self, wp: Optional[np.ndarray], wc: Optional[np.ndarray] = None, bias: Optional[np.ndarray] = None, bins: Optional[np.ndarray] = None,
                  layers=None, upsample: int = 4, min_depth: float = 0.001, max_depth: float = 10.0, out_shape: Optional[Tuple[int, int]] = None,
                  norm: bool = False, logits: bool = False, fine: bool = False) -> None:
        """A binned depth head for every later forward (vitx_depth_set): `wp` [K, Dc] f32 over the patch tokens of `layers` (indices; None: the last
        layer), `wc` [K, Dc] over the class tokens (None: no class half), `bias` [K], `bins` [K] the bin centres; per image a depth map [out_h, out_w]
        f32 (`out_shape` None: the context's image shape).  `norm`: the rows are the final-norm features, not the raw residual stream; `logits` /
        `fine`: the patch logits and offsets / the fine plane are kept for depth_read.  wp None turns the output off and frees its buffers."""
        fp = C.POINTER(C.c_float)
        if wp is None:
            check(lib().vitx_depth_set(self._h, None, None, None, None, 0, 0, 0, 0, 0.0, 0.0, 0, 0, 0), "vitx_depth_set")
            return
        w = np.ascontiguousarray(wp, dtype=np.float32)
        if w.ndim != 2:
            raise ValueError("depth_set: wp must be [K, Dc]")
        K = w.shape[0]

        def opt(a, shape, name):
            if a is None:
                return None
            a = np.ascontiguousarray(a, dtype=np.float32)
            if a.shape != shape:
                raise ValueError(f"depth_set: {name} must be {list(shape)}")
            return a
        c, b, bn = opt(wc, w.shape, "wc"), opt(bias, (K,), "bias"), opt(bins, (K,), "bins")
        if bn is None:
            raise ValueError("depth_set: bins [K] are required")
        mask = _layer_mask([] if layers is None else layers, "depth_set: ")
        oh, ow = (0, 0) if out_shape is None else (int(out_shape[0]), int(out_shape[1]))
        ptr = lambda a: a.ctypes.data_as(fp) if a is not None else None
        check(lib().vitx_depth_set(self._h, ptr(w), ptr(c), ptr(b), ptr(bn), K, w.shape[1], mask, int(upsample), float(min_depth), float(max_depth), oh, ow,
                                   (DEPTH_NORM if norm else 0) | (DEPTH_LOGITS if logits else 0) | (DEPTH_FINE if fine else 0)), "vitx_depth_set")
        self._depth_flags = (bool(logits), bool(fine))

    def depth_shape(self) -> Tuple[int, int, int, int]:
        """(out_h, out_w, fine_h, fine_w); zeros while off."""
        v = [C.c_int(0) for _ in range(4)]
        check(lib().vitx_depth_shape(self._h, *[C.byref(x) for x in v]), "vitx_depth_shape")
        return tuple(x.value for x in v)

    def depth_read(self, n: Optional[int] = None):
        """(depth [n, out_h, out_w] f32, fine [n, fh, fw] or None, logits [n, Np, K] or None, offsets [n, K] or None) of the last forward made with a
        depth head set.  `n`, if given, must be that batch."""
        L = lib()
        have, K = L.vitx_depth_images(self._h), L.vitx_depth_bins(self._h)
        if n is not None and n != have:
            raise ValueError(f"depth_read: the last forward with a depth head set had {have} images, not {n}")
        oh, ow, fh, fw = self.depth_shape()
        gh, gw = self.grid_hw
        want_logits, want_fine = getattr(self, "_depth_flags", (False, False)) if K else (False, False)
        m = max(have, 1)
        depth = np.empty((m, max(oh, 1), max(ow, 1)), np.float32)
        fine = np.empty((m, max(fh, 1), max(fw, 1)), np.float32) if want_fine else None
        logits = np.empty((m, gh * gw, max(K, 1)), np.float32) if want_logits else None
        offsets = np.empty((m, max(K, 1)), np.float32) if want_logits else None
        fp = C.POINTER(C.c_float)
        ptr = lambda a: a.ctypes.data_as(fp) if a is not None else None
        check(L.vitx_depth_read(self._h, ptr(depth), ptr(fine), ptr(logits), ptr(offsets)), "vitx_depth_read")
        return depth, fine, logits, offsets

    def depth_device(self) -> Tuple[int, Tuple[int, int]]:
        """(device pointer of the depth maps [capacity][out_h][out_w] f32, (out_h, out_w)) for callers that stay on the GPU; (0, (0, 0)) while off."""
        return int(lib().vitx_depth_device(self._h) or 0), self.depth_shape()[:2]

    def depth_scratch_bytes(self) -> int:
        return int(lib().vitx_depth_scratch_bytes(self._h))

    def synchronize(self) -> None:
        check(lib().vitx_ctx_synchronize(self._h), "vitx_ctx_synchronize")

    def split(self, n: int) -> List[int]:
        """Sizes of the contiguous sub-batches a forward of n images is cut into (vitx_ctx_split); [n] on one stream."""
        m = (C.c_int32 * 4)()
        k = lib().vitx_ctx_split(self._h, n, m, 4)
        if k <= 0:
            raise VitxError(f"vitx_ctx_split({n}) failed")
        return [int(m[i]) for i in range(k)]

    def boundary_rows(self, n: int) -> List[int]:
        """Image ids on either side of every sub-batch boundary of an n-image forward, plus both ends of the batch."""
        ids, off = {0, min(1, n - 1), max(0, n - 2), n - 1}, 0
        for sz in self.split(n)[:-1]:
            off += sz
            ids.update({off - 1, off})
        return sorted(i for i in ids if 0 <= i < n)

    def weight_bytes(self) -> int:
        """Device bytes held by the weight matrices (quantised tensors stay in block form: 4.5 ... 8.5 bits per weight)."""
        return int(lib().vitx_ctx_weight_bytes(self._h))

    def shares_weights(self) -> bool:
        """True when this context attached to a device copy of the weights another context of the same model had uploaded."""
        return bool(lib().vitx_ctx_shares_weights(self._h))

    def ln_fallbacks(self) -> int:
        """GEMM tiles whose fused LayerNorm was left to the fix-up launch since the context was created (vitx_ctx_ln_fallbacks)."""
        return int(lib().vitx_ctx_ln_fallbacks(self._h))

    def ln_fusion_active(self) -> int:
        """1 fused LayerNorms, 0 stand-alone launches, -1 switched off by the fall-back budget (vitx_ctx_ln_fusion_active)."""
        return int(lib().vitx_ctx_ln_fusion_active(self._h))

    def graph_launches(self) -> int:
        """Forwards enqueued by launching a cached hipGraph (vitx_ctx_graph_launches; contexts created with graph=1)."""
        return int(lib().vitx_ctx_graph_launches(self._h))

    def stream_retries(self) -> int:
        """Internal sub-batch streams re-created because they did not run beside the caller's stream (vitx_ctx_stream_retries)."""
        return int(lib().vitx_ctx_stream_retries(self._h))

    def profile_enable(self, on: bool = True) -> None:
        check(lib().vitx_profile_enable(self._h, int(on)))

    def profile_bracket_us(self) -> float:
        """Microseconds one HIP-event bracket adds to a launch (vitx_profile_bracket_us); profile_read() intervals are raw."""
        v = C.c_double()
        check(lib().vitx_profile_bracket_us(self._h, C.byref(v)), "vitx_profile_bracket_us")
        return float(v.value)

    def profile_read(self):
        arr = (ProfEntry * 24)(); n = C.c_int()      # VITX_PROF_MAX_CLASSES
        check(lib().vitx_profile_read(self._h, arr, len(arr), C.byref(n)), "vitx_profile_read")
        return [dict(name=arr[i].name.decode(), launches=arr[i].launches, total_ms=arr[i].total_ms, flops=arr[i].flops, bytes=arr[i].bytes, busy_ms=arr[i].busy_ms) for i in range(n.value)]


class TextContext:
    """A text tower on one GPU (include/vitx.h "the text tower"): token ids [n][T] in, projected embeddings [n][E] out.  No tokenizer, no mask."""

    def __init__(self, model: Model, max_prompts: int = 1, dtype: int = F16, device: int = 0):
        self._h = C.c_void_p()
        self.model = model
        check(lib().vitx_text_create(model._h, device, max_prompts, dtype, C.byref(self._h)), "vitx_text_create")
        self.max_prompts = max_prompts
        self.tokens = model.hparams.img_size
        self.width = model.hparams.num_classes

    def close(self):
        if getattr(self, "_h", None) and self._h:
            lib().vitx_text_free(self._h); self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _ids(self, ids) -> np.ndarray:
        a = np.asarray(ids)
        if a.ndim != 2 or a.shape[1] != self.tokens or not np.issubdtype(a.dtype, np.integer):
            raise ValueError(f"ids must be integers [prompts][{self.tokens}], got {a.dtype} {a.shape}")
        if a.size and (a.min() < -2 ** 31 or a.max() >= 2 ** 31):
            raise ValueError("ids do not fit int32")
        return np.ascontiguousarray(a, np.int32)

    def embed(self, ids, l2: bool = False) -> np.ndarray:
        """[n][E] f32; l2: every row divided by its norm (VITX_TEXT_L2).  More than max_prompts rows run as several calls: a prompt's bits do not
        depend on its batch."""
        a = self._ids(ids)
        out = np.empty((a.shape[0], self.width), np.float32)
        for i in range(0, a.shape[0], self.max_prompts):
            part = a[i:i + self.max_prompts]
            check(lib().vitx_text_embed(self._h, part.ctypes.data_as(C.POINTER(C.c_int32)), part.shape[0], TEXT_L2 if l2 else 0,
                                        out[i:].ctypes.data_as(C.POINTER(C.c_float))), "vitx_text_embed")
        return out

    def embed_device(self, ids, d_out: int, l2: bool = False, stream: int = 0) -> None:
        a = self._ids(ids)
        check(lib().vitx_text_embed_device(self._h, a.ctypes.data_as(C.POINTER(C.c_int32)), a.shape[0], TEXT_L2 if l2 else 0, d_out, stream), "vitx_text_embed_device")

    @property
    def shares_weights(self) -> bool:
        return bool(lib().vitx_text_shares_weights(self._h))


def text_check_ids(model: Model, ids) -> np.ndarray:
    """The id checks of vitx_text_embed on the host (no device): the pooled position of every prompt, or VitxError (ERR_ARG) for an id outside the
    vocabulary or a prompt without the EOS id."""
    a = np.ascontiguousarray(ids, np.int32)
    pooled = np.empty(a.shape[0], np.int32)
    i32p = C.POINTER(C.c_int32)
    check(lib().vitx_text_check_ids(model._h, a.ctypes.data_as(i32p), a.shape[0], pooled.ctypes.data_as(i32p)), "vitx_text_check_ids")
    return pooled


def text_bank(text_ctx: "TextContext", ids, groups=None, embeds=None):
    """The zero-shot bank of the prompts `ids` [P][T] made by the engine: (embeds [K][E] float64, kind, scale, bias) -- what convert.save_bank and
    Context.zeroshot_set take.  The prompt-ensembling rule is convert.zeroshot_bank's, float64 past the tower: every embedding is normalised;
    with groups [P] of class ids 0 .. K-1 the normalised rows of a class are averaged and the mean is normalised again.  kind, scale and bias
    are the text file's `zs` tensor; a file without one (a tower converted alone) gives (ZS_SOFTMAX, 1.0, 0.0).  embeds: text_ctx.embed(ids) where
    the caller already has it (the tower is then not run again)."""
    e = (text_ctx.embed(ids) if embeds is None else np.asarray(embeds)).astype(np.float64)
    l2 = lambda x: x / np.sqrt((x * x).sum(axis=1, keepdims=True))
    e = l2(e)
    if groups is not None:
        g = np.asarray(groups, dtype=np.int64)
        if g.shape != (e.shape[0],) or g.min() < 0:
            raise ValueError("text_bank: groups must give one class id >= 0 per prompt")
        K = int(g.max()) + 1
        counts = np.bincount(g, minlength=K)
        if (counts == 0).any():
            raise ValueError(f"text_bank: class {int(np.flatnonzero(counts == 0)[0])} has no prompt")
        mean = np.zeros((K, e.shape[1]), np.float64)
        np.add.at(mean, g, e)
        e = l2(mean / counts[:, None])
    kind, scale, bias = text_ctx.model.text_zs or (0, 1.0, 0.0)
    return e, kind, scale, bias


def _pack_shapes(shapes) -> np.ndarray:
    a = np.ascontiguousarray(shapes, np.int32)
    if a.ndim != 2 or a.shape[1] != 2:
        raise ValueError(f"shapes must be [n][2] = (h, w), got {a.shape}")
    return a


def pack_check(model: Model, shapes, max_tokens: int, max_images: int) -> np.ndarray:
    """vitx_pack_check (host only): row0 [n + 1] of a pack of images of `shapes` [n][2] = (h, w), or VitxError (ERR_ARG) for what a packed forward refuses."""
    a = _pack_shapes(shapes)
    row0 = np.empty(a.shape[0] + 1, np.int32)
    i32p = C.POINTER(C.c_int32)
    check(lib().vitx_pack_check(model._h, a.ctypes.data_as(i32p), a.shape[0], max_tokens, max_images, row0.ctypes.data_as(i32p)), "vitx_pack_check")
    return row0


def pack_distinct_grids(model: Model, shapes) -> int:
    """vitx_pack_distinct_grids (host only): the distinct grids among `shapes` -- what a packed forward compares with its context's max_grids."""
    a = _pack_shapes(shapes)
    return int(lib().vitx_pack_distinct_grids(model._h, a.ctypes.data_as(C.POINTER(C.c_int32)), a.shape[0]))


def pack_images(imgs_u8, pp: Preproc, short_side: int, max_long: int = 0, *, patch: int):
    """Every u8 HWC image at its own aspect-preserving shape (rect_shape, then preprocess_rect): (pixels, shapes) -- pixels the f32 HWC images end to
    end in one flat array, shapes int32 [n][2] = (h, w): what PackContext.forward_flat takes."""
    shapes, flat = [], []
    for img in imgs_u8:
        ny, nx = np.asarray(img).shape[:2]
        w, h = rect_shape(nx, ny, patch, short_side, max_long)
        shapes.append((h, w)); flat.append(preprocess_rect(img, pp, w, h).ravel())
    return np.concatenate(flat), np.asarray(shapes, np.int32)


def pack_fit_shapes(model: Model, src_shapes, short_side: int, max_long: int = 0) -> np.ndarray:
    """vitx_pack_fit_shapes (host only): rect_shape per source of `src_shapes` [n][2] = (ny, nx) -> shapes int32 [n][2] = (h, w)."""
    a = _pack_shapes(src_shapes)
    out = np.empty_like(a)
    i32p = C.POINTER(C.c_int32)
    check(lib().vitx_pack_fit_shapes(model._h, a.ctypes.data_as(i32p), a.shape[0], short_side, max_long, out.ctypes.data_as(i32p)), "vitx_pack_fit_shapes")
    return out


def pack_u8_check(model: Model, pp: Optional[Preproc], src_shapes, shapes, max_src_bytes: int = 0):
    """vitx_pack_u8_check (host only): (src0 int64 [n + 1], tile0 int32 [n + 1], lds) of a packed forward of `shapes` [n][2] = (h, w) fed from u8 sources of
    `src_shapes` [n][2] = (ny, nx) -- source i is bytes src0[i] .. src0[i + 1] - 1, tile0 the running count of the preprocessing launch's 32 x 8 tiles,
    lds its dynamic LDS -- or VitxError for what such a forward refuses.  pp None: the file's description; max_src_bytes 0: no bound."""
    a, o = _pack_shapes(src_shapes), _pack_shapes(shapes)
    n = o.shape[0]
    if a.shape[0] != n:      # the C call takes one n: a list of another length is refused there as a forward refuses it
        e = VitxError(f"vitx_pack_u8_check: u8 sources were declared for {a.shape[0]} images, the call has {n}")
        e.code = ERR_ARG
        raise e
    src0, tile0, lds = np.empty(n + 1, np.int64), np.empty(n + 1, np.int32), C.c_int()
    i32p = C.POINTER(C.c_int32)
    check(lib().vitx_pack_u8_check(model._h, C.byref(pp) if pp is not None else None, a.ctypes.data_as(i32p), o.ctypes.data_as(i32p), n, max_src_bytes,
                                   src0.ctypes.data_as(C.POINTER(C.c_int64)), tile0.ctypes.data_as(i32p), C.byref(lds)), "vitx_pack_u8_check")
    return src0, tile0, lds.value


def preprocess_pack(pp: Preproc, d_srcs: int, src_shapes, out_shapes, d_out: int) -> None:
    """vitx_op_preprocess_pack (test only; null stream, synchronous): u8 HWC sources of `src_shapes` [n][2] = (ny, nx) strictly end to end at d_srcs (4-byte
    aligned, readable up to the byte count rounded up to 4), each stretched to its own out_shapes [n][2] = (h, w) -> d_out f32 HWC, end to end."""
    a, o = _pack_shapes(src_shapes), _pack_shapes(out_shapes)
    if a.shape[0] != o.shape[0]:
        raise ValueError(f"{a.shape[0]} source shapes, {o.shape[0]} output shapes")
    i32p = C.POINTER(C.c_int32)
    check(lib().vitx_op_preprocess_pack(C.byref(pp), d_srcs or None, a.ctypes.data_as(i32p), o.ctypes.data_as(i32p), a.shape[0], d_out or None), "vitx_op_preprocess_pack")


class PackContext:
    """A packed context (include/vitx.h "packed batches"): images of different shapes, their tokens end to end, in one forward."""

    def __init__(self, model: Model, device: int = 0, max_tokens: int = 1024, max_images: int = 16, dtype: int = F16, pos_interp: int = POS_BICUBIC, max_grids: int = 0):
        self._h = C.c_void_p()
        self.model = model; self.max_tokens = max_tokens; self.max_images = max_images; self.dtype = dtype
        opt = PackOptions(pos_interp=pos_interp, max_grids=max_grids)
        check(lib().vitx_pack_create(model._h, device, max_tokens, max_images, dtype, C.byref(opt), C.byref(self._h)), "vitx_pack_create")
        self._shapes = None; self._feat = 0
        self._dense = self._dense_out = self._dense_shapes = None
        self._depth = self._depth_out = self._depth_shapes = None

    def close(self):
        if getattr(self, "_h", None) and self._h:
            lib().vitx_pack_free(self._h); self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def forward_flat(self, pixels: np.ndarray, shapes):
        """pixels: the images' f32 HWC pixels end to end; shapes [n][2] = (h, w).  Returns (probs, logits), each [n, C]."""
        s = _pack_shapes(shapes); n = s.shape[0]
        x = np.ascontiguousarray(pixels, np.float32).ravel()
        if x.size != int((s[:, 0].astype(np.int64) * s[:, 1]).sum()) * 3:
            raise ValueError(f"pixels hold {x.size} floats, the shapes {int((s[:, 0].astype(np.int64) * s[:, 1]).sum()) * 3}")
        probs = np.empty((n, self.model.num_classes), np.float32); logits = np.empty_like(probs)
        fp = C.POINTER(C.c_float)
        rc = lib().vitx_pack_forward(self._h, x.ctypes.data_as(fp), s.ctypes.data_as(C.POINTER(C.c_int32)), n, probs.ctypes.data_as(fp), logits.ctypes.data_as(fp))
        self._dense_forward(s, rc == 0); self._attn_forward(s, rc == 0)
        check(rc, "vitx_pack_forward")
        self._shapes = s
        return probs, logits

    def forward(self, imgs):
        """A list of f32 HWC arrays [h_i, w_i, 3], each of its own shape -> (probs, logits), each [n, C]."""
        arrs = [np.ascontiguousarray(a, np.float32) for a in imgs]
        for a in arrs:
            if a.ndim != 3 or a.shape[2] != 3:
                raise ValueError(f"every image must be [h, w, 3], got {a.shape}")
        return self.forward_flat(np.concatenate([a.ravel() for a in arrs]) if arrs else np.empty(0, np.float32), [a.shape[:2] for a in arrs])

    def forward_device(self, d_imgs: int, shapes, d_probs: int, d_logits: int = 0, stream: int = 0) -> None:
        """Device pointers, host shapes; only enqueues on `stream` (0 = the context's own stream)."""
        s = _pack_shapes(shapes)
        rc = lib().vitx_pack_forward_device(self._h, d_imgs, s.ctypes.data_as(C.POINTER(C.c_int32)), s.shape[0], d_probs, d_logits or None, stream or None)
        self._dense_forward(s, rc == 0); self._attn_forward(s, rc == 0)
        check(rc, "vitx_pack_forward_device")
        self._shapes = s

    def u8_set(self, pp: Optional[Preproc] = None, max_src_bytes: int = 0) -> None:
        """u8 sources for later calls (vitx_pack_u8_set): the description (None: the file's) and the most source bytes forward_u8 may upload; 0: off."""
        check(lib().vitx_pack_u8_set(self._h, C.byref(pp) if pp is not None else None, int(max_src_bytes)), "vitx_pack_u8_set")

    def u8_sources(self, src_shapes) -> None:
        """The NEXT forward_device call's d_imgs holds u8 HWC sources of `src_shapes` [n][2] = (ny, nx) end to end (vitx_pack_u8_sources); that call consumes
        the declaration.  None withdraws it."""
        if src_shapes is None:
            check(lib().vitx_pack_u8_sources(self._h, None, 0), "vitx_pack_u8_sources")
            return
        s = _pack_shapes(src_shapes)
        check(lib().vitx_pack_u8_sources(self._h, s.ctypes.data_as(C.POINTER(C.c_int32)), s.shape[0]), "vitx_pack_u8_sources")

    def forward_u8(self, imgs_u8, shapes):
        """A list of u8 HWC originals [ny_i, nx_i, 3], each stretched on the device to its own shapes[i] = (h, w), in one forward (vitx_pack_forward_u8).
        Returns (probs, logits), each [n, C]."""
        arrs = [np.ascontiguousarray(a, np.uint8) for a in imgs_u8]
        for a in arrs:
            if a.ndim != 3 or a.shape[2] != 3:
                raise ValueError(f"every image must be [ny, nx, 3], got {a.shape}")
        s = _pack_shapes(shapes); n = s.shape[0]
        src = _pack_shapes([a.shape[:2] for a in arrs]) if arrs else np.empty((0, 2), np.int32)
        if src.shape[0] != n:
            raise ValueError(f"{src.shape[0]} images, {n} shapes")
        flat = np.concatenate([a.ravel() for a in arrs]) if arrs else np.empty(0, np.uint8)
        probs = np.empty((n, self.model.num_classes), np.float32); logits = np.empty_like(probs)
        fp, i32p = C.POINTER(C.c_float), C.POINTER(C.c_int32)
        rc = lib().vitx_pack_forward_u8(self._h, flat.ctypes.data_as(C.POINTER(C.c_uint8)), src.ctypes.data_as(i32p), s.ctypes.data_as(i32p), n,
                                        probs.ctypes.data_as(fp), logits.ctypes.data_as(fp))
        self._dense_forward(s, rc == 0); self._attn_forward(s, rc == 0)
        check(rc, "vitx_pack_forward_u8")
        self._shapes = s
        return probs, logits

    def attn_enable(self, layers=None, rollout: bool = False, max_sq_tokens: int = 0) -> None:
        """Attention maps of every later forward (vitx_pack_attn_enable), Context.attn_enable's arguments and meaning, per image on its own grid: the
        class-token maps of `layers` (None = every layer, [] = none) and, with rollout=True, the attention-rollout row.  max_sq_tokens: the most
        floats the rollout matrices of one call may hold, the sum of N_i^2 (0: max_tokens x min(max_tokens, 1024), whatever a call can name).
        attn_enable([]) turns them off and frees the buffers."""
        L = self.model.hparams.num_hidden_layers
        sel = list(range(L)) if layers is None else sorted(set(int(l) for l in layers))
        mask = _layer_mask(sel, span="0..63")
        if rollout and not max_sq_tokens:
            max_sq_tokens = min(self.max_tokens * min(self.max_tokens, 1024), 2 ** 31 - 1)
        check(lib().vitx_pack_attn_enable(self._h, mask, ATTN_ROLLOUT if rollout else 0, int(max_sq_tokens)), "vitx_pack_attn_enable")
        self._attn_layers, self._attn_rollout, self._attn_shapes = sel, bool(rollout), None

    def attn_disable(self) -> None:
        self.attn_enable([], rollout=False)

    def attn_read(self):
        """Maps of the last forward made with maps on: per image (cls [n_sel, H, N_i] f32, rollout [N_i] f32 or None), N_i = prefix + gh_i gw_i.  Index 0
        of a map is the class token, then the register tokens, then the patches in raster order of the image's own grid (attn_grid reshapes)."""
        sel, roll = getattr(self, "_attn_layers", []), getattr(self, "_attn_rollout", False)
        s = getattr(self, "_attn_shapes", None)
        hp = self.model.hparams
        H, P, Tp = hp.num_attention_heads, hp.patch_size, self.model.num_prefix
        fpt = lib().vitx_pack_attn_floats(self._h)
        if s is None or fpt == 0:
            # the library's own text (and its code) for a read before any forward with maps on
            check(lib().vitx_pack_attn_read(self._h, np.empty(1, np.float32).ctypes.data_as(C.POINTER(C.c_float)), 0), "vitx_pack_attn_read")
            raise VitxError("attn_read: no forward has run with attention maps on since attn_enable")
        assert fpt == len(sel) * H + (1 if roll else 0)
        toks = [Tp + (int(h) // P) * (int(w) // P) for h, w in s]
        out = np.empty(sum(toks) * fpt, np.float32)
        check(lib().vitx_pack_attn_read(self._h, out.ctypes.data_as(C.POINTER(C.c_float)), out.size), "vitx_pack_attn_read")
        res, at = [], 0
        for N in toks:
            blk = out[at * fpt:(at + N) * fpt]
            res.append((blk[:len(sel) * H * N].reshape(len(sel), H, N), blk[len(sel) * H * N:].copy() if roll else None))
            at += N
        return res

    def attn_grid(self, i: int, m: np.ndarray) -> np.ndarray:
        """[..., N_i] map of image i of the last forward with maps on -> [..., gh_i, gw_i]: drops the class token and the register tokens."""
        P = self.model.hparams.patch_size
        h, w = self._attn_shapes[i]
        return np.asarray(m)[..., self.model.num_prefix:].reshape(*np.shape(m)[:-1], int(h) // P, int(w) // P)

    @property
    def attn_device(self) -> int:
        """The device buffer of the maps (vitx_pack_attn_device), image i at float row0[i] * floats-per-token; 0 while off."""
        return int(lib().vitx_pack_attn_device(self._h) or 0)

    def feat_enable(self, cls: bool = True, tokens: bool = False) -> None:
        """Last-layer features of every later forward (vitx_pack_feat_enable); neither: off."""
        self._feat = (FEAT_CLS if cls else 0) | (FEAT_TOKENS if tokens else 0)
        check(lib().vitx_pack_feat_enable(self._h, self._feat), "vitx_pack_feat_enable")

    def feat_read(self):
        """(cls [n, D] or None, tokens: a list of per-image [gh_i, gw_i, D] arrays or None) of the last forward."""
        if self._shapes is None:
            raise VitxError("feat_read: no forward has run")
        D, P = self.model.hparams.hidden_size, self.model.hparams.patch_size
        grids = [(int(h) // P, int(w) // P) for h, w in self._shapes]
        flags = getattr(self, "_feat", 0)
        cls = np.empty((len(grids), D), np.float32) if flags & FEAT_CLS else None
        tok = np.empty((sum(a * b for a, b in grids), D), np.float32) if flags & FEAT_TOKENS else None
        fp = C.POINTER(C.c_float)
        check(lib().vitx_pack_feat_read(self._h, cls.ctypes.data_as(fp) if cls is not None else None, tok.ctypes.data_as(fp) if tok is not None else None), "vitx_pack_feat_read")
        if tok is None:
            return cls, None
        out, at = [], 0
        for a, b in grids:
            out.append(tok[at:at + a * b].reshape(a, b, D)); at += a * b
        return cls, out

    def dense_set(self, weight: Optional[np.ndarray], bias: Optional[np.ndarray] = None, layers=None, max_pixels: int = 0, score: bool = False,
                  logits: bool = False) -> None:
        """A linear head `weight` [K, Dc] f32 (+ `bias` [K]) over the patch tokens of `layers` (indices; None: the last layer) for every later forward:
        per image a label map u8 at the image's own shape (or dense_out's), with `score` the winner's value, with `logits` the patch logits
        (vitx_pack_dense_set).  max_pixels: the output pixels one forward may hold (0: max_tokens x patch x patch, every image at its own shape).
        weight None turns the output off and frees its buffers."""
        if weight is None:
            check(lib().vitx_pack_dense_set(self._h, None, None, 0, 0, 0, 0, 0), "vitx_pack_dense_set")
            self._dense = None
            return
        w, b = _head_arrays("dense_set: ", weight, bias)
        mask = _layer_mask([] if layers is None else layers, "dense_set: ")
        P = self.model.hparams.patch_size
        fp = C.POINTER(C.c_float)
        check(lib().vitx_pack_dense_set(self._h, w.ctypes.data_as(fp), b.ctypes.data_as(fp) if b is not None else None, w.shape[0], w.shape[1], mask,
                                        int(max_pixels) or self.max_tokens * P * P, (DENSE_SCORE if score else 0) | (DENSE_LOGITS if logits else 0)), "vitx_pack_dense_set")
        self._dense = (w.shape[0], bool(score), bool(logits))
        self._dense_out = self._dense_shapes = None

    def dense_out(self, shapes) -> None:
        """Output shapes [n][2] = (out_h, out_w) of the NEXT forward's label maps (vitx_pack_dense_out), e.g. the sizes of the originals; that forward
        consumes them.  None withdraws them."""
        if shapes is None:
            check(lib().vitx_pack_dense_out(self._h, None, 0), "vitx_pack_dense_out")
            self._dense_out = None
            return
        s = _pack_shapes(shapes)
        check(lib().vitx_pack_dense_out(self._h, s.ctypes.data_as(C.POINTER(C.c_int32)), s.shape[0]), "vitx_pack_dense_out")
        self._dense_out = s

    def _attn_forward(self, s, ok: bool) -> None:
        """Book-keeping of a forward call for attn_read: a call that ran with maps on fixed the shapes of its maps."""
        if ok and (getattr(self, "_attn_layers", None) or getattr(self, "_attn_rollout", False)):
            self._attn_shapes = s

    def _dense_forward(self, s, ok: bool) -> None:
        """Book-keeping of a forward call for dense_read and depth_read: the call consumed dense_out's and depth_out's shapes; a call that ran fixed the
        shapes of its maps."""
        out, self._dense_out = getattr(self, "_dense_out", None), None
        if ok and getattr(self, "_dense", None):
            self._dense_shapes = (s.copy(), (out if out is not None else s).copy())
        out, self._depth_out = getattr(self, "_depth_out", None), None
        if ok and getattr(self, "_depth", None):
            self._depth_shapes = (s.copy(), (out if out is not None else s).copy())

    def dense_read(self):
        """(labels: a list of per-image [out_h_i, out_w_i] u8 arrays, scores: the same in f32 or None, logits: a list of [gh_i gw_i, K] f32 or None) of the
        last forward made with the dense head set (vitx_pack_dense_read)."""
        if not getattr(self, "_dense", None) or getattr(self, "_dense_shapes", None) is None:
            e = VitxError("dense_read: no forward has run with a dense head set")
            e.code = ERR_ARG
            raise e
        K, want_score, want_logits = self._dense
        shapes, outs = self._dense_shapes
        P = self.model.hparams.patch_size
        px = [int(h) * int(w) for h, w in outs]
        npatch = [(int(h) // P) * (int(w) // P) for h, w in shapes]
        labels = np.empty(sum(px), np.uint8)
        score = np.empty(sum(px), np.float32) if want_score else None
        logits = np.empty((sum(npatch), K), np.float32) if want_logits else None
        fp = C.POINTER(C.c_float)
        check(lib().vitx_pack_dense_read(self._h, labels.ctypes.data_as(C.POINTER(C.c_uint8)), score.ctypes.data_as(fp) if want_score else None,
                                         logits.ctypes.data_as(fp) if want_logits else None), "vitx_pack_dense_read")
        lab, sc, lg, at, ar = [], [], [], 0, 0
        for (oh, ow), p_, r_ in zip(outs, px, npatch):
            lab.append(labels[at:at + p_].reshape(int(oh), int(ow)))
            if want_score:
                sc.append(score[at:at + p_].reshape(int(oh), int(ow)))
            if want_logits:
                lg.append(logits[ar:ar + r_])
            at += p_; ar += r_
        return lab, (sc if want_score else None), (lg if want_logits else None)

    def dense_device(self) -> int:
        """Device pointer of the label buffer (the maps of a forward end to end, u8), 0 while off."""
        return int(lib().vitx_pack_dense_device(self._h) or 0)

    def dense_scratch_bytes(self) -> int:
        return int(lib().vitx_pack_dense_scratch_bytes(self._h))

    def depth_set(self, wp: Optional[np.ndarray], wc: Optional[np.ndarray] = None, bias: Optional[np.ndarray] = None, bins: Optional[np.ndarray] = None,
                  layers=None, upsample: int = 4, min_depth: float = 0.001, max_depth: float = 10.0, max_pixels: int = 0, norm: bool = False,
                  logits: bool = False, fine: bool = False) -> None:
        """A binned depth head for every later forward (vitx_pack_depth_set), Context.depth_set's arguments and meaning: per image a depth map f32 at the
        image's own shape (or depth_out's).  max_pixels: the output pixels one forward may hold (0: max_tokens x patch x patch, every image at its own
        shape).  wp None turns the output off and frees its buffers."""
        fp = C.POINTER(C.c_float)
        if wp is None:
            check(lib().vitx_pack_depth_set(self._h, None, None, None, None, 0, 0, 0, 0, 0.0, 0.0, 0, 0), "vitx_pack_depth_set")
            self._depth = None
            return
        w = np.ascontiguousarray(wp, dtype=np.float32)
        if w.ndim != 2:
            raise ValueError("depth_set: wp must be [K, Dc]")
        K = w.shape[0]

        def opt(a, shape, name):
            if a is None:
                return None
            a = np.ascontiguousarray(a, dtype=np.float32)
            if a.shape != shape:
                raise ValueError(f"depth_set: {name} must be {list(shape)}")
            return a
        c, b, bn = opt(wc, w.shape, "wc"), opt(bias, (K,), "bias"), opt(bins, (K,), "bins")
        if bn is None:
            raise ValueError("depth_set: bins [K] are required")
        mask = _layer_mask([] if layers is None else layers, "depth_set: ")
        P = self.model.hparams.patch_size
        ptr = lambda a: a.ctypes.data_as(fp) if a is not None else None
        check(lib().vitx_pack_depth_set(self._h, ptr(w), ptr(c), ptr(b), ptr(bn), K, w.shape[1], mask, int(upsample), float(min_depth), float(max_depth),
                                        int(max_pixels) or self.max_tokens * P * P,
                                        (DEPTH_NORM if norm else 0) | (DEPTH_LOGITS if logits else 0) | (DEPTH_FINE if fine else 0)), "vitx_pack_depth_set")
        self._depth = (K, int(upsample), bool(logits), bool(fine))
        self._depth_out = self._depth_shapes = None

    def depth_out(self, shapes) -> None:
        """Output shapes [n][2] = (out_h, out_w) of the NEXT forward's depth maps (vitx_pack_depth_out), e.g. the sizes of the originals; that forward
        consumes them.  None withdraws them."""
        if shapes is None:
            check(lib().vitx_pack_depth_out(self._h, None, 0), "vitx_pack_depth_out")
            self._depth_out = None
            return
        s = _pack_shapes(shapes)
        check(lib().vitx_pack_depth_out(self._h, s.ctypes.data_as(C.POINTER(C.c_int32)), s.shape[0]), "vitx_pack_depth_out")
        self._depth_out = s

    def depth_read(self):
        """(depth: a list of per-image [out_h_i, out_w_i] f32 arrays, fine: a list of [u gh_i, u gw_i] f32 or None, logits: a list of [gh_i gw_i, K] f32 or
        None, offsets [n, K] f32 or None) of the last forward made with the depth head set (vitx_pack_depth_read)."""
        if not getattr(self, "_depth", None) or getattr(self, "_depth_shapes", None) is None:
            e = VitxError("depth_read: no forward has run with a depth head set")
            e.code = ERR_ARG
            raise e
        K, u, want_logits, want_fine = self._depth
        shapes, outs = self._depth_shapes
        P = self.model.hparams.patch_size
        grids = [(int(h) // P, int(w) // P) for h, w in shapes]
        px = [int(h) * int(w) for h, w in outs]
        npatch = [a * b for a, b in grids]
        depth = np.empty(sum(px), np.float32)
        fine = np.empty(u * u * sum(npatch), np.float32) if want_fine else None
        logits = np.empty((sum(npatch), K), np.float32) if want_logits else None
        offsets = np.empty((len(grids), K), np.float32) if want_logits else None
        fp = C.POINTER(C.c_float)
        ptr = lambda a: a.ctypes.data_as(fp) if a is not None else None
        check(lib().vitx_pack_depth_read(self._h, ptr(depth), ptr(fine), ptr(logits), ptr(offsets)), "vitx_pack_depth_read")
        dm, fn, lg, at, af, ar = [], [], [], 0, 0, 0
        for (oh, ow), (gh, gw), p_, r_ in zip(outs, grids, px, npatch):
            dm.append(depth[at:at + p_].reshape(int(oh), int(ow)))
            if want_fine:
                fn.append(fine[af:af + u * u * r_].reshape(u * gh, u * gw))
            if want_logits:
                lg.append(logits[ar:ar + r_])
            at += p_; af += u * u * r_; ar += r_
        return dm, (fn if want_fine else None), (lg if want_logits else None), offsets

    def depth_device(self) -> int:
        """Device pointer of the depth buffer (the maps of a forward end to end, f32), 0 while off."""
        return int(lib().vitx_pack_depth_device(self._h) or 0)

    def depth_scratch_bytes(self) -> int:
        return int(lib().vitx_pack_depth_scratch_bytes(self._h))

    @property
    def shares_weights(self) -> bool:
        return bool(lib().vitx_pack_shares_weights(self._h))

    @property
    def scratch_bytes(self) -> int:
        return int(lib().vitx_pack_scratch_bytes(self._h))

    @property
    def launches(self) -> Tuple[int, int]:
        """(kernel launches, patch-embedding launches among them) of the last forward call."""
        pe = C.c_int()
        return int(lib().vitx_pack_launches(self._h, C.byref(pe))), pe.value


def op_attention_packed(dtype: int, d_qkv: int, d_out: int, d_row0: int, n: int, D: int, H: int, stream: int = 0) -> None:
    """vitx_op_attention_packed: attention over a pack, image i = rows row0[i] .. row0[i + 1] - 1 (d_row0 int32 [n + 1] on the device)."""
    check(lib().vitx_op_attention_packed(dtype, d_qkv, d_out, d_row0, n, D, H, stream or None), "vitx_op_attention_packed")


def pack_attn_check(model: Model, shapes, layers=None, rollout: bool = False, max_sq_tokens: int = 0, *, layer_mask: Optional[int] = None, flags: Optional[int] = None):
    """vitx_pack_attn_check (host only): (rblk0 int32 [n + 1], sq0 int32 [n + 1]) of a packed forward of `shapes` [n][2] with attention maps on, or VitxError
    for what vitx_pack_attn_enable refuses in its arguments (ERR_ARG) and what such a call is refused for (ERR_UNSUPPORTED above 1024 tokens with rollout,
    ERR_ARG above max_sq_tokens).  layer_mask / flags: the raw arguments, for the refusals the keyword form cannot express."""
    a = _pack_shapes(shapes)
    n = a.shape[0]
    if layer_mask is None:
        L = model.hparams.num_hidden_layers
        layer_mask = _layer_mask(list(range(L)) if layers is None else sorted(set(int(l) for l in layers)), span="0..63")
    if flags is None:
        flags = ATTN_ROLLOUT if rollout else 0
    i32p = C.POINTER(C.c_int32)
    rblk0, sq0 = np.zeros(n + 1, np.int32), np.zeros(n + 1, np.int32)
    check(lib().vitx_pack_attn_check(model._h, a.ctypes.data_as(i32p), n, layer_mask, flags, int(max_sq_tokens), rblk0.ctypes.data_as(i32p), sq0.ctypes.data_as(i32p)),
          "vitx_pack_attn_check")
    return rblk0, sq0


def _row0(row0) -> np.ndarray:
    r = np.ascontiguousarray(row0, np.int32)
    if r.ndim != 1 or r.size < 2:
        raise ValueError("row0 is [n + 1]")
    return r


def op_attention_map_packed(dtype: int, d_qkv: int, d_cls: int, d_mean: int, row0, D: int, H: int, half_identity: bool = False) -> None:
    """vitx_op_attention_map_packed (test only; null stream, synchronous): the class-token maps and / or the head mean (half_identity: the rollout factor) of a
    pack, host row0 [n + 1].  d_cls: image i's [H, N_i] at float row0[i] * H; d_mean: its [N_i, N_i] at float sum_(j < i) N_j^2; either may be 0."""
    r = _row0(row0)
    check(lib().vitx_op_attention_map_packed(dtype, d_qkv or None, d_cls or None, d_mean or None, r.ctypes.data_as(C.POINTER(C.c_int32)), r.size - 1, D, H,
                                             1 if half_identity else 0), "vitx_op_attention_map_packed")


def op_rollout_step_packed(d_a: int, d_r: int, row0) -> None:
    """vitx_op_rollout_step_packed (test only; synchronous): a_i <- a_i . r_i per image of a pack, image i's matrices at float sum_(j < i) N_j^2 of both."""
    r = _row0(row0)
    check(lib().vitx_op_rollout_step_packed(d_a or None, d_r or None, r.ctypes.data_as(C.POINTER(C.c_int32)), r.size - 1), "vitx_op_rollout_step_packed")


def op_rollout_row_packed(d_cls: int, d_r: int, d_out: int, row0, H: int) -> None:
    """vitx_op_rollout_row_packed (test only; synchronous): the last rollout factor's row per image of a pack; d_cls as op_attention_map_packed writes it,
    d_r as op_rollout_step_packed (0: the row itself), d_out: image i's row [N_i] at float row0[i]."""
    r = _row0(row0)
    check(lib().vitx_op_rollout_row_packed(d_cls or None, d_r or None, d_out or None, r.ctypes.data_as(C.POINTER(C.c_int32)), r.size - 1, H), "vitx_op_rollout_row_packed")


def pack_dense_check(model: Model, shapes, out_shapes, K: int, max_pixels: int):
    """vitx_pack_dense_check (host only): (pix0 int64 [n + 1], tile0 int32 [n + 1]) of a packed forward of `shapes` [n][2] with a dense head of K classes and
    max_pixels set -- image i's maps are elements pix0[i] .. pix0[i + 1] - 1, tile0 the running count of the label launch's 64 x 16 tiles -- or
    VitxError for what such a forward refuses.  out_shapes [n][2] = (out_h, out_w), None: the images' own shapes."""
    a = _pack_shapes(shapes)
    o = None if out_shapes is None else _pack_shapes(out_shapes)
    # the C call takes one n: a list of another length is refused there as a forward refuses it, through the n the head would see
    n = a.shape[0]
    if o is not None and o.shape[0] != n:
        e = VitxError(f"vitx_pack_dense_check: output shapes were given for {o.shape[0]} images, the call has {n}")
        e.code = ERR_ARG
        raise e
    pix0, tile0 = np.empty(n + 1, np.int64), np.empty(n + 1, np.int32)
    i32p = C.POINTER(C.c_int32)
    check(lib().vitx_pack_dense_check(model._h, a.ctypes.data_as(i32p), o.ctypes.data_as(i32p) if o is not None else None, n, K, max_pixels,
                                      pix0.ctypes.data_as(C.POINTER(C.c_int64)), tile0.ctypes.data_as(i32p)), "vitx_pack_dense_check")
    return pix0, tile0


def op_dense_labels_packed(d_logits: int, ld: int, grids, outs, lrow, K: int, d_labels: int, d_score: int = 0, stream: int = 0) -> None:
    """vitx_op_dense_labels_packed: the label kernel on a pack.  d_logits [rows, ld] f32 on the device; host grids [n][2] = (gh, gw), outs [n][2] =
    (out_h, out_w), lrow [n] = each image's first logit row -> d_labels u8 (and d_score f32), the images' maps end to end."""
    g, o = _pack_shapes(grids), _pack_shapes(outs)
    r = np.ascontiguousarray(lrow, np.int32)
    if o.shape != g.shape or r.shape != (g.shape[0],):
        raise ValueError("op_dense_labels_packed: grids and outs are [n][2], lrow is [n]")
    i32p = C.POINTER(C.c_int32)
    check(lib().vitx_op_dense_labels_packed(d_logits or None, ld, g.ctypes.data_as(i32p), o.ctypes.data_as(i32p), r.ctypes.data_as(i32p), g.shape[0], K, d_labels or None,
                                            d_score or None, stream or None), "vitx_op_dense_labels_packed")


def dense_pack_tables(grids, outs, lrow):
    """vitx_dense_pack_tables (host only): (tab int32 [n + 1 + 10 n], tiles, cells) -- the device table of the packed label launch, to be uploaded by
    the caller for op_dense_labels_packed_tables."""
    g, o = _pack_shapes(grids), _pack_shapes(outs)
    r = np.ascontiguousarray(lrow, np.int32)
    if o.shape != g.shape or r.shape != (g.shape[0],):
        raise ValueError("dense_pack_tables: grids and outs are [n][2], lrow is [n]")
    n = g.shape[0]
    tab, tiles, cells = np.zeros(n + 1 + 10 * n, np.int32), C.c_int(), C.c_int()
    i32p = C.POINTER(C.c_int32)
    check(lib().vitx_dense_pack_tables(g.ctypes.data_as(i32p), o.ctypes.data_as(i32p), r.ctypes.data_as(i32p), n, tab.ctypes.data_as(i32p), C.byref(tiles), C.byref(cells)),
          "vitx_dense_pack_tables")
    return tab, tiles.value, cells.value


def op_dense_labels_packed_tables(d_logits: int, ld: int, d_tab: int, n: int, tiles: int, cells: int, K: int, d_labels: int, d_score: int = 0, stream: int = 0) -> None:
    """vitx_op_dense_labels_packed_tables: the packed label launch on a table of dense_pack_tables already on the device; only enqueues."""
    check(lib().vitx_op_dense_labels_packed_tables(d_logits or None, ld, d_tab or None, n, tiles, cells, K, d_labels or None, d_score or None, stream or None),
          "vitx_op_dense_labels_packed_tables")


def pack_depth_check(model: Model, shapes, out_shapes, K: int, upsample: int, max_pixels: int):
    """vitx_pack_depth_check (host only): (pix0 int64 [n + 1], fine0 int64 [n + 1], ftile0 int32 [n + 1], otile0 int32 [n + 1]) of a packed forward of
    `shapes` [n][2] with a depth head of K bins, `upsample` and max_pixels set -- image i's map is floats pix0[i] .. pix0[i + 1] - 1, its fine plane
    fine0[i] .., ftile0 / otile0 the running counts of the fine launch's 16 x 16 and the resize launch's 64 x 16 tiles -- or VitxError for what such a
    forward refuses.  out_shapes [n][2] = (out_h, out_w), None: the images' own shapes."""
    a = _pack_shapes(shapes)
    o = None if out_shapes is None else _pack_shapes(out_shapes)
    # the C call takes one n: a list of another length is refused there as a forward refuses it, through the n the head would see
    n = a.shape[0]
    if o is not None and o.shape[0] != n:
        e = VitxError(f"vitx_pack_depth_check: output shapes were given for {o.shape[0]} images, the call has {n}")
        e.code = ERR_ARG
        raise e
    pix0, fine0, ftile0, otile0 = np.empty(n + 1, np.int64), np.empty(n + 1, np.int64), np.empty(n + 1, np.int32), np.empty(n + 1, np.int32)
    i32p, i64p = C.POINTER(C.c_int32), C.POINTER(C.c_int64)
    check(lib().vitx_pack_depth_check(model._h, a.ctypes.data_as(i32p), o.ctypes.data_as(i32p) if o is not None else None, n, K, upsample, max_pixels,
                                      pix0.ctypes.data_as(i64p), fine0.ctypes.data_as(i64p), ftile0.ctypes.data_as(i32p), otile0.ctypes.data_as(i32p)), "vitx_pack_depth_check")
    return pix0, fine0, ftile0, otile0


def op_depth_fine_packed(d_logits: int, ld: int, d_offsets: int, d_bins: int, grids, lrow, orow, K: int, upsample: int, d_fine: int, stream: int = 0) -> None:
    """vitx_op_depth_fine_packed: the fine kernel on a pack.  d_logits [rows, ld] f32, d_offsets [., ld] f32 (or 0) and d_bins [K] on the device; host grids
    [n][2] = (gh, gw), lrow [n] = each image's first logit row, orow [n] = its offsets row (None without offsets) -> d_fine f32, the planes end to end."""
    g = _pack_shapes(grids)
    r = np.ascontiguousarray(lrow, np.int32)
    q = None if orow is None else np.ascontiguousarray(orow, np.int32)
    if r.shape != (g.shape[0],) or (q is not None and q.shape != r.shape):
        raise ValueError("op_depth_fine_packed: grids is [n][2], lrow and orow are [n]")
    i32p = C.POINTER(C.c_int32)
    check(lib().vitx_op_depth_fine_packed(d_logits or None, ld, d_offsets or None, d_bins or None, g.ctypes.data_as(i32p), r.ctypes.data_as(i32p),
                                          q.ctypes.data_as(i32p) if q is not None else None, g.shape[0], K, upsample, d_fine or None, stream or None), "vitx_op_depth_fine_packed")


def op_depth_resize_packed(d_fine: int, fines, outs, min_depth: float, max_depth: float, d_out: int, stream: int = 0) -> None:
    """vitx_op_depth_resize_packed: the resize kernel on a pack.  d_fine = the fine planes end to end; host fines [n][2] = (fh, fw), outs [n][2] =
    (out_h, out_w) -> d_out f32, the maps end to end."""
    f, o = _pack_shapes(fines), _pack_shapes(outs)
    if o.shape != f.shape:
        raise ValueError("op_depth_resize_packed: fines and outs are [n][2]")
    i32p = C.POINTER(C.c_int32)
    check(lib().vitx_op_depth_resize_packed(d_fine or None, f.ctypes.data_as(i32p), o.ctypes.data_as(i32p), f.shape[0], min_depth, max_depth, d_out or None, stream or None),
          "vitx_op_depth_resize_packed")


def depth_pack_tables(grids, outs, lrow, orow, upsample: int):
    """vitx_depth_pack_tables (host only): (tab int32 [2 (n + 1) + 16 n], ftiles, otiles, cells) -- the device table of the packed fine and resize
    launches, to be uploaded by the caller for op_depth_fine_packed_tables / op_depth_resize_packed_tables."""
    g, o = _pack_shapes(grids), _pack_shapes(outs)
    r, q = np.ascontiguousarray(lrow, np.int32), np.ascontiguousarray(orow, np.int32)
    if o.shape != g.shape or r.shape != (g.shape[0],) or q.shape != r.shape:
        raise ValueError("depth_pack_tables: grids and outs are [n][2], lrow and orow are [n]")
    n = g.shape[0]
    tab, ft, ot, cells = np.zeros(2 * (n + 1) + 16 * n, np.int32), C.c_int(), C.c_int(), C.c_int()
    i32p = C.POINTER(C.c_int32)
    check(lib().vitx_depth_pack_tables(g.ctypes.data_as(i32p), o.ctypes.data_as(i32p), r.ctypes.data_as(i32p), q.ctypes.data_as(i32p), n, upsample, tab.ctypes.data_as(i32p),
                                       C.byref(ft), C.byref(ot), C.byref(cells)), "vitx_depth_pack_tables")
    return tab, ft.value, ot.value, cells.value


def op_depth_fine_packed_tables(d_logits: int, ld: int, d_offsets: int, ldo: int, d_bins: int, d_tab: int, n: int, tiles: int, cells: int, K: int, d_fine: int,
                                stream: int = 0) -> None:
    """vitx_op_depth_fine_packed_tables: the packed fine launch on a table of depth_pack_tables already on the device; only enqueues."""
    check(lib().vitx_op_depth_fine_packed_tables(d_logits or None, ld, d_offsets or None, ldo, d_bins or None, d_tab or None, n, tiles, cells, K, d_fine or None, stream or None),
          "vitx_op_depth_fine_packed_tables")


def op_depth_resize_packed_tables(d_fine: int, d_tab: int, n: int, tiles: int, min_depth: float, max_depth: float, d_out: int, stream: int = 0) -> None:
    """vitx_op_depth_resize_packed_tables: the packed resize launch on a table of depth_pack_tables already on the device; only enqueues."""
    check(lib().vitx_op_depth_resize_packed_tables(d_fine or None, d_tab or None, n, tiles, min_depth, max_depth, d_out or None, stream or None), "vitx_op_depth_resize_packed_tables")


def op_rope_packed(dtype: int, d_qkv: int, d_cos: int, d_sin: int, d_row0: int, d_table_off: int, n: int, prefix: int, D: int, H: int, stream: int = 0) -> None:
    """vitx_op_rope_packed: vitx_op_rope on a pack; image i's table starts d_table_off[i] floats into d_cos and d_sin."""
    check(lib().vitx_op_rope_packed(dtype, d_qkv, 0, d_cos, d_sin, d_row0, d_table_off, n, prefix, D, H, stream or None), "vitx_op_rope_packed")


class Group:
    """Several GPUs in one process: batch shards + one RCCL all-gather of the probabilities (vitx_group_*)."""

    def __init__(self, model: Model, devices, max_batch_per_device: int, dtype: int = F16):
        self.model = model
        devs = (C.c_int * len(devices))(*devices)
        self._h = C.c_void_p()
        check(lib().vitx_group_create(model._h, devs, len(devices), max_batch_per_device, dtype, C.byref(self._h)), "vitx_group_create")

    def forward(self, imgs_hwc: np.ndarray) -> np.ndarray:
        """Host images in, [n, C] probabilities out ([n, 25, C] for a ViTSTR file: vitx_group_out_floats floats per image)."""
        x = np.ascontiguousarray(imgs_hwc, np.float32); n = x.shape[0]
        _check_image_shape(self.model, x)
        R = self.model.seq_len
        probs = np.empty((n, self.model.num_classes) if R == 0 else (n, R, self.model.num_classes), np.float32)
        assert probs[0].size == lib().vitx_group_out_floats(self._h)
        fp = C.POINTER(C.c_float)
        check(lib().vitx_group_forward(self._h, x.ctypes.data_as(fp), n, probs.ctypes.data_as(fp)), "vitx_group_forward")
        return probs

    def forward_device(self, d_imgs: List[int], n_local: List[int], topk: int = 0) -> Tuple[List[int], int]:
        """Device-resident shards (one device pointer and image count per device).  Returns (per-device pointers to the gathered result,
        n_max): [n_devices][n_max][C] f32, or [n_devices][n_max][rows][topk] {f32, i32} pairs when topk > 0 (vitx_group_forward_device)."""
        nd = lib().vitx_group_num_devices(self._h)
        assert len(d_imgs) == nd and len(n_local) == nd
        ptrs = (C.c_void_p * nd)(*[p or None for p in d_imgs]); cnt = (C.c_int * nd)(*n_local)
        check(lib().vitx_group_forward_device(self._h, ptrs, cnt, topk), "vitx_group_forward_device")
        return [lib().vitx_group_result(self._h, r) for r in range(nd)], lib().vitx_group_result_rows(self._h)

    def close(self):
        if getattr(self, "_h", None) and self._h:
            lib().vitx_group_free(self._h); self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def probe_mfma(device: int = 0, dtype: int = BF16, fill: int = 2, target_ms: float = 150.0) -> Tuple[float, float]:
    """(TFLOP/s, shader MHz) of back-to-back MFMAs on register operands: the power-managed ceiling of the matrix pipe (vitx_probe_mfma)."""
    tf = C.c_double(); mhz = C.c_double()
    check(lib().vitx_probe_mfma(device, dtype, fill, target_ms, C.byref(tf), C.byref(mhz)), "vitx_probe_mfma")
    return tf.value, mhz.value


def op_attention_map(dtype: int, d_qkv: int, d_cls: int, d_mean: int, n_img: int, N: int, D: int, H: int, lo_off: int = 0, stream: int = 0) -> None:
    """vitx_op_attention_map: class-token maps [n_img, H, N] and / or the head mean [n_img, N, N] (f32, device pointers; 0 = not wanted)."""
    check(lib().vitx_op_attention_map(dtype, d_qkv, lo_off, d_cls or None, d_mean or None, n_img, N, D, H, stream or None), "vitx_op_attention_map")


def op_rollout_factor(dtype: int, d_qkv: int, d_out: int, n_img: int, N: int, D: int, H: int, lo_off: int = 0, stream: int = 0) -> None:
    """vitx_op_rollout_factor: the rollout factor 0.5 mean_h A_h + 0.5 I [n_img, N, N] (f32, device pointers)."""
    check(lib().vitx_op_rollout_factor(dtype, d_qkv, lo_off, d_out, n_img, N, D, H, stream or None), "vitx_op_rollout_factor")


def op_rollout_step(d_a: int, d_r: int, n_img: int, N: int, stream: int = 0) -> None:
    """vitx_op_rollout_step: a[b] <- a[b] . r[b] in place over a ([n_img, N, N] f32 each, device pointers)."""
    check(lib().vitx_op_rollout_step(d_a, d_r, n_img, N, stream or None), "vitx_op_rollout_step")


def op_rollout_row(d_cls: int, cls_stride: int, d_r: int, d_out: int, out_stride: int, n_img: int, N: int, H: int, stream: int = 0) -> None:
    """vitx_op_rollout_row: row 0 of the last rollout factor (from class-token maps [H, N] per image) times r [n_img, N, N]; d_r 0: that row itself."""
    check(lib().vitx_op_rollout_row(d_cls, cls_stride, d_r or None, d_out, out_stride, n_img, N, H, stream or None), "vitx_op_rollout_row")


def op_features(d_x: int, row_stride: int, img_stride: int, d_w: int, d_b: int, d_cls: int, d_mean: int, d_tokens: int, out_img_stride: int,
                n_img: int, N: int, D: int, eps: float = 1e-6, l2: bool = False, stream: int = 0) -> None:
    """vitx_op_features: the f32 final-norm features of n_img images of N rows (device pointers; 0 = output not wanted; strides in floats)."""
    check(lib().vitx_op_features(d_x, row_stride, img_stride, d_w, d_b, d_cls or None, d_mean or None, d_tokens or None, out_img_stride,
                                 n_img, N, D, eps, int(l2), stream or None), "vitx_op_features")


def op_features_ex(d_x: int, row_stride: int, img_stride: int, d_w: int, d_b: int, d_cls: int, d_mean: int, d_tokens: int, out_img_stride: int,
                   n_img: int, N: int, first: int, D: int, eps: float = 1e-6, l2: bool = False, d_z: int = 0, dtype: int = F16, stream: int = 0) -> None:
    """vitx_op_features_ex: op_features with the first patch row `first` (1 + registers) and, with d_z, the pooled head's operand
    [n_img, 2 D] = RNE(cls) ‖ RNE(mean) in `dtype`."""
    check(lib().vitx_op_features_ex(d_x, row_stride, img_stride, d_w, d_b, d_cls or None, d_mean or None, d_tokens or None, out_img_stride,
                                    n_img, N, first, D, eps, int(l2), d_z or None, dtype, stream or None), "vitx_op_features_ex")


def op_patch_embed(dtype: int, d_img: int, d_w: int, d_bias: int, d_pos: int, d_cls: int, d_reg: int, R: int, d_X: int, n_img: int, S: int, P: int,
                   Cin: int, D: int, stream: int = 0) -> None:
    """vitx_op_patch_embed (test only; synchronous): the forward's patch-embedding kernel with R register rows per image.  d_w is the f32
    kernel [D, Cin * P * P] in the file's order; every pointer is a device pointer to f32.  d_cls = 0 (R = 0): a model without a class token --
    no prefix row, d_pos [(S/P)^2, D]."""
    check(lib().vitx_op_patch_embed(dtype, d_img, d_w, d_bias, d_pos, d_cls or None, d_reg or None, R, d_X, n_img, S, P, Cin, D, stream or None), "vitx_op_patch_embed")


def op_patch_embed_rect(dtype: int, d_img: int, d_w: int, d_bias: int, d_pos: int, d_cls: int, d_reg: int, R: int, d_X: int, n_img: int, img_h: int, img_w: int,
                        P: int, Cin: int, D: int) -> None:
    """vitx_op_patch_embed_rect (test only; synchronous): vitx_op_patch_embed on [n, img_h, img_w, Cin] images; d_pos [prefix rows + (img_h/P)(img_w/P), D]."""
    check(lib().vitx_op_patch_embed_rect(dtype, d_img, d_w, d_bias, d_pos, d_cls or None, d_reg or None, R, n_img, img_h, img_w, P, Cin, D, d_X), "vitx_op_patch_embed_rect")


def op_attention_pool(d_x: int, row_stride: int, img_stride: int, d_ln_w: int, d_ln_b: int, eps: float, d_u: int, d_M: int, d_p: int,
                      n_img: int, N: int, D: int, H: int, stream: int = 0) -> None:
    """vitx_op_attention_pool: the pooling kernel of the attention-pooling head (device pointers, strides in floats): M [n_img, H, D] f32 and,
    with d_p, the probabilities [n_img, H, N] f32."""
    check(lib().vitx_op_attention_pool(d_x, row_stride, img_stride, d_ln_w, d_ln_b, eps, d_u, d_M, d_p or None, n_img, N, D, H, stream or None), "vitx_op_attention_pool")


def op_rope(dtype: int, d_qkv: int, d_cos: int, d_sin: int, n_img: int, N: int, prefix: int, D: int, H: int, lo_off: int = 0, stream: int = 0) -> None:
    """vitx_op_rope: rotary position embeddings in place on d_qkv [n_img * N, 3 D] (lo_off: the parity mode's lo plane); cos / sin f32 [N - prefix, head_dim / 2].  Only enqueues."""
    check(lib().vitx_op_rope(dtype, d_qkv, lo_off, d_cos, d_sin, n_img, N, prefix, D, H, stream), "vitx_op_rope")


def op_swiglu(dtype: int, d_in: int, ld_in: int, d_out: int, ld_out: int, rows: int, F: int, stream: int = 0) -> None:
    """vitx_op_swiglu: d_out[r][j] = RNE(silu(d_in[r][j]) * d_in[r][F + j]), j < F, rows of ld_in / ld_out elements of `dtype`.  Only enqueues."""
    check(lib().vitx_op_swiglu(dtype, d_in, ld_in, d_out, ld_out, rows, F, stream or None), "vitx_op_swiglu")


def op_text_embed(table_f16: bool, d_tok: int, d_pos: int, d_ids: int, d_x: int, n: int, T: int, D: int, stream: int = 0) -> None:
    check(lib().vitx_op_text_embed(1 if table_f16 else 0, d_tok, d_pos, d_ids, d_x, n, T, D, stream), "vitx_op_text_embed")


def op_text_pool(dtype: int, d_x: int, d_pooled: int, d_w: int, d_b: int, d_z: int, n: int, T: int, D: int, eps: float = 1e-6, stream: int = 0) -> None:
    check(lib().vitx_op_text_pool(dtype, d_x, d_pooled, d_w, d_b, d_z, n, T, D, eps, stream), "vitx_op_text_pool")


def op_attention_text(dtype: int, d_qkv: int, d_out: int, n: int, T: int, D: int, H: int, causal: bool, stream: int = 0) -> None:
    check(lib().vitx_op_attention_text(dtype, d_qkv, d_out, n, T, D, H, 1 if causal else 0, stream), "vitx_op_attention_text")


def zeroshot_max_classes(E: int) -> int:
    """vitx_zeroshot_max_classes: the largest bank (classes) of width E the bank GEMM's 32-bit window takes; 0 for an E that is not a multiple of 64."""
    return int(lib().vitx_zeroshot_max_classes(E))


def op_zeroshot(dtype: int, d_z: int, z_stride: int, d_bank: int, d_a: int, d_acc: int, d_probs: int, d_logits: int, n: int, K: int, E: int,
                kind: int = ZS_SOFTMAX, scale: float = 1.0, bias: float = 0.0, stream: int = 0) -> None:
    """vitx_op_zeroshot: the zero-shot launches on their own (device pointers; z_stride in floats).  d_bank [K_pad, E] in `dtype` (K_pad = K
    rounded up to 128, zero rows beyond K), d_a [n_pad, E] in `dtype`, d_acc [n_pad + 1, K_pad] f32 (n_pad = n rounded up to 256),
    d_probs and d_logits [n, K] f32."""
    check(lib().vitx_op_zeroshot(dtype, d_z or None, z_stride, d_bank or None, d_a or None, d_acc or None, d_probs or None, d_logits or None, n, K, E,
                                 int(kind), float(scale), float(bias), stream or None), "vitx_op_zeroshot")


def op_nn_state_bytes(n: int, k: int) -> int:
    return int(lib().vitx_op_nn_state_bytes(n, k))


def op_nn_select(d_scores: int, ld: int, n: int, cols: int, base_index: int, d_state: int, k: int, first: bool, stream: int = 0) -> None:
    """vitx_op_nn_select: merge columns 0 .. cols of the f32 score rows [n, ld] (column j = gallery row base_index + j) into the running top-k state."""
    check(lib().vitx_op_nn_select(d_scores or None, ld, n, cols, base_index, d_state or None, k, int(bool(first)), stream or None), "vitx_op_nn_select")


def op_nn_finish(d_state: int, n: int, k: int, d_pairs: int, d_labels: int = 0, n_labels: int = 0, temperature: float = 0.0, d_vote: int = 0, stream: int = 0) -> None:
    """vitx_op_nn_finish: the state -> pairs [n, k] {f32 score, i32 index} best first and, with labels, the vote [n, n_labels]."""
    check(lib().vitx_op_nn_finish(d_state or None, n, k, d_labels or None, n_labels, float(temperature), d_pairs or None, d_vote or None, stream or None), "vitx_op_nn_finish")


def op_nn(dtype: int, d_z: int, z_stride: int, z_is_operand: bool, n: int, d_gallery: int, G: int, E: int, k: int, chunk: int, d_a: int, d_acc: int,
          d_state: int, d_pairs: int, stream: int = 0) -> None:
    """vitx_op_nn: the nearest-neighbour launches of a forward on their own (device pointers; z_stride in elements of z's type).  d_gallery [G_pad, E]
    in `dtype` (G_pad = G rounded up to 128, zero rows beyond G), d_a [n_pad, E] `dtype`, d_acc [n_pad + 1, chunk] f32 with n_pad = n rounded up to 256."""
    check(lib().vitx_op_nn(dtype, d_z or None, z_stride, int(bool(z_is_operand)), n, d_gallery or None, G, E, k, chunk, d_a or None, d_acc or None,
                           d_state or None, d_pairs or None, stream or None), "vitx_op_nn")


def op_dense_labels(d_logits: int, ld: int, n: int, gh: int, gw: int, K: int, out_h: int, out_w: int, d_labels: int, d_score: int = 0, stream: int = 0) -> None:
    """vitx_op_dense_labels: logits [n gh gw, ld] f32 on the device -> labels [n, out_h, out_w] u8 (and scores f32): bilinear resampling + arg-max."""
    check(lib().vitx_op_dense_labels(d_logits or None, ld, n, gh, gw, K, out_h, out_w, d_labels or None, d_score or None, stream or None), "vitx_op_dense_labels")


def dense_labels_host(logits: np.ndarray, n: int, gh: int, gw: int, K: int, out_h: int, out_w: int, want_score: bool = True):
    """vitx_dense_labels_host: the label kernel's arithmetic on the host.  logits [n gh gw, ld] f32 -> (labels [n, out_h, out_w] u8, score or None)."""
    lg = np.ascontiguousarray(logits, np.float32)
    if lg.ndim != 2 or lg.shape[0] != n * gh * gw:
        raise ValueError("dense_labels_host: logits must be [n gh gw, ld]")
    labels = np.empty((n, out_h, out_w), np.uint8)
    score = np.empty((n, out_h, out_w), np.float32) if want_score else None
    check(lib().vitx_dense_labels_host(lg.ctypes.data, lg.shape[1], n, gh, gw, K, out_h, out_w, labels.ctypes.data, score.ctypes.data if want_score else None),
          "vitx_dense_labels_host")
    return labels, score


def op_dense(dtype: int, d_a: int, d_w: int, d_bias: int, d_logits: int, n: int, gh: int, gw: int, K: int, Dc: int, out_h: int, out_w: int,
             d_labels: int, d_score: int = 0, stream: int = 0) -> None:
    """vitx_op_dense: the dense head's launches on a given operand (device pointers): d_a [M_pad, Dc] `dtype` (M_pad = n gh gw rounded up to 256), d_w
    [K_pad, Dc] (K_pad = K rounded up to 128, zero rows beyond K), d_bias [K_pad] f32 -> d_logits [M_pad, K_pad] f32, d_labels, d_score."""
    check(lib().vitx_op_dense(dtype, d_a or None, d_w or None, d_bias or None, d_logits or None, n, gh, gw, K, Dc, out_h, out_w, d_labels or None, d_score or None,
                              stream or None), "vitx_op_dense")


def dense_head(path: str) -> dict:
    """A dense head file (convert.dense_head / convert.py --dense-head-out): an .npz with weight [K, Dc] f32, bias [K] f32, layers (indices) and,
    optionally, names [K].  Returns {"weight", "bias", "layers", "names"} (names None when absent)."""
    with np.load(path, allow_pickle=False) as z:
        if "weight" not in z or "bias" not in z or "layers" not in z:
            raise ValueError(f"{path}: a dense head file holds weight, bias and layers")
        w, b = np.ascontiguousarray(z["weight"], np.float32), np.ascontiguousarray(z["bias"], np.float32)
        layers = [int(l) for l in np.asarray(z["layers"]).reshape(-1)]
        names = [str(s) for s in z["names"]] if "names" in z else None
    if w.ndim != 2 or b.shape != (w.shape[0],):
        raise ValueError(f"{path}: weight must be [K, Dc] and bias [K]")
    if names is not None and len(names) != w.shape[0]:
        raise ValueError(f"{path}: {len(names)} names for {w.shape[0]} classes")
    return {"weight": w, "bias": b, "layers": layers, "names": names}


def op_depth_fine(d_logits: int, ld: int, d_offsets: int, d_bins: int, n: int, gh: int, gw: int, K: int, upsample: int, d_fine: int, stream: int = 0) -> None:
    """vitx_op_depth_fine: logits [n gh gw, ld] f32 (+ offsets [n, ld] or 0) and bins [K] on the device -> fine [n, u gh, u gw] f32."""
    check(lib().vitx_op_depth_fine(d_logits or None, ld, d_offsets or None, d_bins or None, n, gh, gw, K, upsample, d_fine or None, stream or None), "vitx_op_depth_fine")


def op_depth_resize(d_fine: int, n: int, fh: int, fw: int, out_h: int, out_w: int, min_depth: float, max_depth: float, d_out: int, stream: int = 0) -> None:
    """vitx_op_depth_resize: fine [n, fh, fw] f32 on the device -> depth [n, out_h, out_w] f32, resampled bilinearly and clamped."""
    check(lib().vitx_op_depth_resize(d_fine or None, n, fh, fw, out_h, out_w, min_depth, max_depth, d_out or None, stream or None), "vitx_op_depth_resize")


def depth_host(logits: np.ndarray, offsets: Optional[np.ndarray], bins: np.ndarray, n: int, gh: int, gw: int, K: int, upsample: int, out_h: int, out_w: int,
               min_depth: float, max_depth: float):
    """vitx_depth_host: the two depth kernels' arithmetic on the host.  logits [n gh gw, ld] f32, offsets [n, ld] or None, bins [K] ->
    (depth [n, out_h, out_w] f32, fine [n, u gh, u gw] f32)."""
    lg = np.ascontiguousarray(logits, np.float32)
    if lg.ndim != 2 or lg.shape[0] != n * gh * gw:
        raise ValueError("depth_host: logits must be [n gh gw, ld]")
    off = None if offsets is None else np.ascontiguousarray(offsets, np.float32)
    if off is not None and off.shape != (n, lg.shape[1]):
        raise ValueError("depth_host: offsets must be [n, ld]")
    bn = np.ascontiguousarray(bins, np.float32)
    if bn.ndim != 1 or bn.shape[0] < K:
        raise ValueError("depth_host: bins must be [K]")
    depth = np.empty((n, max(out_h, 1), max(out_w, 1)), np.float32)
    fine = np.empty((n, max(upsample * gh, 1), max(upsample * gw, 1)), np.float32)
    check(lib().vitx_depth_host(lg.ctypes.data, lg.shape[1], off.ctypes.data if off is not None else None, bn.ctypes.data, n, gh, gw, K, upsample, out_h, out_w,
                                min_depth, max_depth, depth.ctypes.data, fine.ctypes.data), "vitx_depth_host")
    return depth, fine


def op_depth(dtype: int, d_a: int, d_wp: int, d_acls: int, d_wc: int, d_bias: int, d_bins: int, d_logits: int, d_offsets: int, n: int, gh: int, gw: int, K: int,
             Dc: int, upsample: int, out_h: int, out_w: int, min_depth: float, max_depth: float, d_fine: int, d_depth: int, stream: int = 0) -> None:
    """vitx_op_depth: the depth head's launches on given operands (device pointers): d_a [M_pad, Dc] `dtype` (M_pad = n gh gw rounded up to 256), d_wp and
    d_wc [K_pad, Dc], d_acls [n_pad, Dc] (d_acls = d_wc = 0: no class half), d_bias [K_pad] f32, d_bins [K] -> d_logits [M_pad + 1, K_pad] f32, d_offsets
    [n_pad, K_pad] f32, d_fine, d_depth."""
    check(lib().vitx_op_depth(dtype, d_a or None, d_wp or None, d_acls or None, d_wc or None, d_bias or None, d_bins or None, d_logits or None, d_offsets or None,
                              n, gh, gw, K, Dc, upsample, out_h, out_w, min_depth, max_depth, d_fine or None, d_depth or None, stream or None), "vitx_op_depth")


def op_depth_rows(dtype: int, d_x: int, ldx: int, d_y: int, ldy: int, rows: int, D: int, stream: int = 0) -> None:
    """vitx_op_depth_rows: f32 rows (stride ldx) -> rows of `dtype` (stride ldy elements), rounded to nearest even."""
    check(lib().vitx_op_depth_rows(dtype, d_x or None, ldx, d_y or None, ldy, rows, D, stream or None), "vitx_op_depth_rows")


def depth_bins(K: int, lo: float, hi: float, kind: str = "UD") -> np.ndarray:
    """The K bin centres of a depth head between lo and hi: "UD" linspace, "SID" logspace (mmseg's bins_strategy), computed in float64 and
    rounded once to f32."""
    if K < 1 or not (0.0 < lo <= hi) or not np.isfinite(hi):
        raise ValueError("depth_bins: K >= 1 and 0 < lo <= hi")
    if kind == "UD":
        return np.linspace(np.float64(lo), np.float64(hi), K).astype(np.float32)
    if kind == "SID":
        return np.logspace(np.log10(np.float64(lo)), np.log10(np.float64(hi)), K).astype(np.float32)
    raise ValueError(f"depth_bins: kind {kind!r} is neither 'UD' nor 'SID'")


def depth_head(path: str) -> dict:
    """A depth head file (convert.depth_head / convert.py --depth-head-out): an .npz with wp [K, Dc] f32, optionally wc [K, Dc], bias [K], bins [K],
    layers (indices), upsample, min_depth, max_depth and norm.  Returns a dict with those keys (wc None when absent)."""
    with np.load(path, allow_pickle=False) as z:
        for k in ("wp", "bias", "bins", "layers", "upsample", "min_depth", "max_depth", "norm"):
            if k not in z:
                raise ValueError(f"{path}: a depth head file holds wp, bias, bins, layers, upsample, min_depth, max_depth and norm (no {k})")
        wp, b, bn = (np.ascontiguousarray(z[k], np.float32) for k in ("wp", "bias", "bins"))
        wc = np.ascontiguousarray(z["wc"], np.float32) if "wc" in z else None
        layers = [int(l) for l in np.asarray(z["layers"]).reshape(-1)]
        u, lo, hi, norm = int(z["upsample"]), float(z["min_depth"]), float(z["max_depth"]), bool(z["norm"])
    if wp.ndim != 2 or b.shape != (wp.shape[0],) or bn.shape != (wp.shape[0],) or (wc is not None and wc.shape != wp.shape):
        raise ValueError(f"{path}: wp (and wc) must be [K, Dc], bias and bins [K]")
    return {"wp": wp, "wc": wc, "bias": b, "bins": bn, "layers": layers, "upsample": u, "min_depth": lo, "max_depth": hi, "norm": norm}


def round_operand(x: np.ndarray, dtype: int) -> np.ndarray:
    """x rounded (RNE) to a context's operand type, as f32: fp16 for F16, bf16 for BF16 and MXFP8 (finite values)."""
    x = np.ascontiguousarray(x, np.float32)
    if dtype == F16:
        return x.astype(np.float16).astype(np.float32)
    b = x.view(np.uint32).astype(np.uint64)
    b = ((b + 0x7fff + ((b >> 16) & 1)) >> 16) << 16
    return b.astype(np.uint32).view(np.float32)


def nn_gallery(ctx: "Context", images: np.ndarray, source: int = NN_EMBED) -> np.ndarray:
    """Gallery rows [n, E] f32 of unit length for Context.nn_set, from forwards of `images` [n, h, w, 3] through ctx: the logits rows (NN_LOGITS), or
    (NN_EMBED) the head GEMM's operand rows -- RNE of the last layer's FEAT_CLS feature (and of FEAT_MEAN behind it for a cls + mean head), which the
    header pins to the operand bit for bit.  Normalised in float64, rounded once to f32.  Runs in batches of ctx.max_batch; leaves the features off."""
    x = np.ascontiguousarray(images, np.float32)
    pooled = source == NN_EMBED and ctx.model.head_pool == POOL_CLS_MEAN
    if source == NN_EMBED:
        ctx.feat_enable(cls=True, mean=pooled)
    elif source != NN_LOGITS:
        raise ValueError(f"nn_gallery: unknown source {source}")
    rows = []
    try:
        for i0 in range(0, x.shape[0], ctx.max_batch):
            xb = x[i0:i0 + ctx.max_batch]
            _, lg = ctx.forward(xb, want_logits=True)
            if source == NN_LOGITS:
                rows.append(lg.astype(np.float64))
                continue
            f = ctx.feat_read(xb.shape[0])[ctx.model.hparams.num_hidden_layers - 1]
            z = np.concatenate([f["cls"], f["mean"]], axis=1) if pooled else f["cls"]
            rows.append(round_operand(z, ctx.dtype).astype(np.float64))
    finally:
        if source == NN_EMBED:
            ctx.feat_disable()
    z = np.concatenate(rows, axis=0)
    nrm = np.sqrt((z * z).sum(-1, keepdims=True))
    return np.divide(z, nrm, out=np.zeros_like(z), where=nrm > 0).astype(np.float32)


def mx_k_pad(K: int) -> int:
    """Row length of an MXFP8 operand: K rounded up to the 128-deep K step of the block-scaled MFMA."""
    return (K + 127) // 128 * 128


def mxfp8_quantize(x: np.ndarray, k_pad: Optional[int] = None) -> Tuple[np.ndarray, np.ndarray]:
    """Host encoder (vitx_mxfp8_quantize): f32 [rows, K] -> (e4m3 bytes [rows, k_pad] uint8, E8M0 scales [rows, k_pad / 32] uint8)."""
    x = np.ascontiguousarray(np.atleast_2d(x), np.float32)
    rows, K = x.shape
    k_pad = mx_k_pad(K) if k_pad is None else k_pad
    q = np.zeros((rows, k_pad), np.uint8); s = np.zeros((rows, max(k_pad // 32, 1)), np.uint8)
    check(lib().vitx_mxfp8_quantize(x.ctypes.data_as(C.POINTER(C.c_float)), rows, K, k_pad, q.ctypes.data_as(C.POINTER(C.c_uint8)),
                                    s.ctypes.data_as(C.POINTER(C.c_uint8))), "vitx_mxfp8_quantize")
    return q, s


def op_layernorm_f32(d_x: int, d_w: int, d_b: int, d_y: int, M: int, D: int, eps: float = 1e-6, stream: int = 0) -> None:
    """vitx_op_layernorm_f32: y [M][D] f32 = the LayerNorm of x [M][D] f32 before any rounding (d_y == d_x: in place).  Only enqueues."""
    check(lib().vitx_op_layernorm_f32(d_x, d_w, d_b, d_y, M, D, eps, stream or None), "vitx_op_layernorm_f32")


def op_quantize_mxfp8(d_x: int, rows: int, K: int, k_pad: int, d_q: int, d_scales: int, stream: int = 0) -> None:
    """vitx_op_quantize_mxfp8: the device encoder on f32 [rows][K] (device pointers)."""
    check(lib().vitx_op_quantize_mxfp8(d_x, rows, K, k_pad, d_q, d_scales, stream or None), "vitx_op_quantize_mxfp8")


def op_layernorm_mxfp8(d_x: int, d_w: int, d_b: int, d_q: int, d_scales: int, M: int, D: int, eps: float = 1e-6, stream: int = 0) -> None:
    """vitx_op_layernorm_mxfp8: LayerNorm of f32 [M][D] -> MX [M][mx_k_pad(D)] + scales (device pointers)."""
    check(lib().vitx_op_layernorm_mxfp8(d_x, d_w, d_b, d_q, d_scales, M, D, eps, stream or None), "vitx_op_layernorm_mxfp8")


def op_gemm_mxfp8(epi: int, d_a: int, d_as: int, d_w: int, d_ws: int, d_bias: int, d_out: int, d_out_scales: int, M: int, N: int, K: int, stream: int = 0) -> None:
    """vitx_op_gemm_mxfp8: epi EPI_BIAS (bf16 out), EPI_BIAS_GELU (MX out + scales), EPI_BIAS_RESID (f32 out +=)."""
    check(lib().vitx_op_gemm_mxfp8(epi, d_a, d_as, d_w, d_ws, d_bias, d_out, d_out_scales or None, M, N, K, stream or None), "vitx_op_gemm_mxfp8")


def topk(probs_row: np.ndarray, k: int = 5):
    p = np.ascontiguousarray(probs_row, np.float32); k = min(k, p.size)
    idx = (C.c_int32 * k)(); val = (C.c_float * k)()
    check(lib().vitx_topk(p.ctypes.data_as(C.POINTER(C.c_float)), p.size, k, idx, val), "vitx_topk")
    return list(idx), list(val)
