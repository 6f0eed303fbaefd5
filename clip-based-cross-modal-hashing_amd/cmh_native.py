"""ctypes binding of libcmh.so (include/cmh.h) for the Python host side.

PyTorch is plumbing here: it owns device memory and streams; every computation of the hot path
happens inside libcmh.so (hand-written HIP, gfx950).  There is NO CPU or eager-PyTorch fallback:
a missing library or a non-GPU tensor raises.
"""
from __future__ import annotations

import ctypes as C
import os
import threading

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("CMH_LIB") or os.path.join(_HERE, "csrc", "build", "libcmh.so")   # CMH_LIB: A/B a kernel build

ABI_VERSION = 6            # include/cmh.h CMH_VERSION: bumped whenever a struct layout or a signature changes
F32, BF16, FP8 = 0, 1, 2
ACT_NONE, ACT_TANH, ACT_RELU = 0, 1, 2
TIE_REFERENCE, TIE_STABLE = 0, 1


class NativeError(RuntimeError):
    pass


class BlockWeights(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in (
        "in_proj_w", "in_proj_b", "out_proj_w", "out_proj_b", "ln1_w", "ln1_b", "ln2_w", "ln2_b",
        "fc_w", "fc_b", "proj_w", "proj_b",
        "in_proj_cs", "out_proj_cs", "fc_cs", "proj_cs")] + [("act_scale", C.c_float * 4)]     # fp8 mode only


class GemmProblem(C.Structure):
    """include/cmh.h cmh_gemm_problem: one of the two GEMMs of a grouped launch."""
    _fields_ = [("x", C.c_void_p), ("w", C.c_void_p), ("bias", C.c_void_p), ("residual", C.c_void_p), ("out", C.c_void_p),
                ("M", C.c_int32), ("N", C.c_int32), ("K", C.c_int32), ("m_dev", C.c_void_p), ("colscale", C.c_void_p),
                ("alpha", C.c_float), ("out_scale", C.c_float)]


class VitWeights(C.Structure):
    _fields_ = [("gemm_dtype", C.c_int32), ("resolution", C.c_int32), ("patch", C.c_int32),
                ("width", C.c_int32), ("layers", C.c_int32), ("embed_dim", C.c_int32),
                ("conv1_w", C.c_void_p), ("class_embedding", C.c_void_p),
                ("positional_embedding", C.c_void_p), ("ln_pre_w", C.c_void_p), ("ln_pre_b", C.c_void_p),
                ("ln_post_w", C.c_void_p), ("ln_post_b", C.c_void_p), ("proj_t", C.c_void_p),
                ("blocks", C.POINTER(BlockWeights))]


class TextWeights(C.Structure):
    _fields_ = [("gemm_dtype", C.c_int32), ("context_length", C.c_int32), ("vocab_size", C.c_int32),
                ("width", C.c_int32), ("layers", C.c_int32), ("embed_dim", C.c_int32),
                ("token_embedding", C.c_void_p), ("positional_embedding", C.c_void_p),
                ("ln_final_w", C.c_void_p), ("ln_final_b", C.c_void_p), ("text_projection_t", C.c_void_p),
                ("blocks", C.POINTER(BlockWeights))]


class BlockGrads(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in (
        "in_proj_w", "in_proj_b", "out_proj_w", "out_proj_b", "ln1_w", "ln1_b", "ln2_w", "ln2_b",
        "fc_w", "fc_b", "proj_w", "proj_b")]


class VitGrads(C.Structure):
    _fields_ = [("conv1_w", C.c_void_p), ("class_embedding", C.c_void_p), ("positional_embedding", C.c_void_p),
                ("ln_pre_w", C.c_void_p), ("ln_pre_b", C.c_void_p), ("ln_post_w", C.c_void_p), ("ln_post_b", C.c_void_p),
                ("proj", C.c_void_p), ("blocks", C.POINTER(BlockGrads))]


class TextGrads(C.Structure):
    _fields_ = [("token_embedding", C.c_void_p), ("positional_embedding", C.c_void_p), ("ln_final_w", C.c_void_p),
                ("ln_final_b", C.c_void_p), ("text_projection", C.c_void_p), ("blocks", C.POINTER(BlockGrads))]


class AdamTensor(C.Structure):
    _fields_ = [("p", C.c_void_p), ("g", C.c_void_p), ("m", C.c_void_p), ("v", C.c_void_p), ("n", C.c_int64),
                ("lr", C.c_float), ("weight_decay", C.c_float), ("max_grad_norm", C.c_float), ("p_bf16", C.c_void_p)]


class Taps(C.Structure):
    _fields_ = [("ptrs", C.POINTER(C.c_void_p)), ("count", C.c_int32)]


_lib = None
_lock = threading.Lock()

_i32, _i64, _f, _p, _sz = C.c_int32, C.c_int64, C.c_float, C.c_void_p, C.c_size_t

# name -> (restype, argtypes); exactly the symbols include/cmh.h declares
SIGNATURES = {
    "cmh_last_error": (C.c_char_p, []),
    "cmh_version": (C.c_int, []),
    "cmh_vit_workspace_bytes": (_sz, [C.POINTER(VitWeights), _i32]),
    "cmh_text_workspace_bytes": (_sz, [C.POINTER(TextWeights), _i32, _i32]),
    "cmh_vit_encode": (C.c_int, [C.POINTER(VitWeights), _p, _i32, _p, _p, _sz, C.POINTER(Taps), _p]),
    "cmh_text_encode": (C.c_int, [C.POINTER(TextWeights), _p, _i32, _i32, _p, _p, _p, _sz, C.POINTER(Taps), _p]),
    "cmh_text_encode_packed": (C.c_int, [C.POINTER(TextWeights), _p, _i32, _i32, _p, _p, _p, _sz, _p]),
    "cmh_vit_calibrate_fp8": (C.c_int, [C.POINTER(VitWeights), _p, _i32, _p, _p, _p, _sz, _p]),
    "cmh_text_calibrate_fp8": (C.c_int, [C.POINTER(TextWeights), _p, _i32, _i32, _p, _p, _p, _sz, _p]),
    "cmh_linear_gemm": (C.c_int, [_i32, _p, _p, _p, _p, _p, _i32, _i32, _i32, _i32, _p]),
    "cmh_layernorm": (C.c_int, [_p, _p, _p, _p, _i32, _i32, _i32, _p]),
    "cmh_attention": (C.c_int, [_i32, _p, _p, _i32, _i32, _i32, _i32, _p, _p]),
    "cmh_attention_pair": (C.c_int, [_i32, _p, _p, _i32, _i32, _i32, _i32, _p, _p, _p, _i32, _i32, _i32, _i32, _p, _p]),
    "cmh_gemm_tuning": (C.c_int, [_i32, _i32]),
    "cmh_set_pooled_tail": (C.c_int, [_i32]),
    "cmh_set_gemm_rows": (C.c_int, [_i32]),
    "cmh_set_gemm_grouped": (C.c_int, [_i32]),
    "cmh_set_gemm_lc": (C.c_int, [_i32]),
    "cmh_gemm_route": (C.c_int, [_i32] * 8),
    "cmh_gemm_plan": (C.c_int, [_i32, _i32, C.POINTER(_i32), C.POINTER(_i32), C.POINTER(_i32)]),
    "cmh_set_grad_stream16": (C.c_int, [_i32]),
    "cmh_set_text_token_packing": (C.c_int, [_i32]),
    "cmh_linear_gemm_grouped": (C.c_int, [_i32, C.POINTER(GemmProblem), C.POINTER(GemmProblem), _i32, _p]),
    "cmh_clip_encode_pair": (C.c_int, [C.POINTER(VitWeights), _p, C.POINTER(TextWeights), _p, _i32, _i32, _i32, _p, _p, _p, _p, _sz, _p, _sz, _p]),
    "cmh_clip_encode_pair2": (C.c_int, [C.POINTER(VitWeights), _p, _i32, _p, _i32, C.POINTER(TextWeights), _p, _i32, _i32, _p, _p, _p, _p, _sz, _p, _sz, _p]),
    "cmh_msl_workspace_bytes": (_sz, [_i32]),
    "cmh_msl_loss": (C.c_int, [_p, _p, _p, _i32, _i32, _i32, _p, _p, _sz, _p]),
    "cmh_msl_loss_backward": (C.c_int, [_p, _p, _p, _i32, _i32, _i32, _p, _p, _p, _p, _sz, _p]),
    "cmh_spl_workspace_bytes": (_sz, [_i32]),
    "cmh_spl_loss": (C.c_int, [_p, _p, _p, _i32, _i32, _i32, _f, _f, _p, _p, _sz, _p]),
    "cmh_spl_loss_backward": (C.c_int, [_p, _p, _p, _i32, _i32, _i32, _f, _f, _p, _p, _p, _p, _sz, _p]),
    "cmh_qmi_workspace_bytes": (_sz, [_i32]),
    "cmh_qmi_loss": (C.c_int, [_p, _p, _p, _i32, _i32, _i32, _f, _p, _p, _p, _sz, _p]),
    "cmh_qmi_loss_backward": (C.c_int, [_p, _p, _p, _i32, _i32, _i32, _f, _p, _p, _p, _p, _p, _sz, _p]),
    "cmh_ddbh_workspace_bytes": (_sz, [_i32]),
    "cmh_ddbh_bp_loss": (C.c_int, [_p, _p, _i32, _p, _i32, _i32, _i32] + [C.c_double] * 6 + [_p, _p, _p, _p, _sz, _p]),
    "cmh_ddbh_bp_loss_backward": (C.c_int, [_p, _p, _i32, _p, _i32, _i32, _i32] + [C.c_double] * 6 + [_p, _p, _p, _p, _p, _p]),
    "cmh_ddbh_quant_loss": (C.c_int, [_p, _i32, _p, _i32, _i32, _i32, _p, _p, _p, _sz, _p]),
    "cmh_ddbh_quant_loss_backward": (C.c_int, [_p, _i32, _p, _i32, _i32, _p, _p, _p]),
    # label-free joint-semantics loss (csrc/djsrh.hip): none of the cmh_djsrh_* entries has an upstream counterpart
    "cmh_djsrh_workspace_bytes": (_sz, [_i32, _i32, _i32]),             # no upstream counterpart
    "cmh_djsrh_target": (C.c_int, [_p, _p, _i32, _i32, _f, _f, _f, _p, _p, _sz, _p]),      # no upstream counterpart
    "cmh_msc_triplet_workspace_bytes": (_sz, [_i32]),
    "cmh_msc_triplet_loss": (C.c_int, [_p, _p, _i32, _p, _i32, _i32, _i32, _f, _i32, _i32, _p, _p, _p, _p, _p, _p, _p, _sz, _p]),
    "cmh_msc_triplet_loss_backward": (C.c_int, [_p, _p, _i32, _i32, _i32, _i32, _p, _p, _p, _p, _p, _p, _p, _p]),
    "cmh_dws_workspace_bytes": (_sz, [_i32, _i32, _i32]),
    "cmh_dws_distances": (C.c_int, [_p, _p, _i32, _i32, _i32, _p, _p, _p, _p]),
    "cmh_dws_mine": (C.c_int, [_p, _i32, _p, _i32, _i32, _i32, _f, _i32, _p, _p, _p, _p, _sz, _p]),
    "cmh_dws_margin_loss": (C.c_int, [_p, _p, _i32, _p, _p, _i32, _i32, _f, _p, _p, _p, _p, _sz, _p]),
    "cmh_dws_margin_loss_backward": (C.c_int, [_p, _p, _i32, _p, _i32, _i32, _i32, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p]),
    "cmh_cpf_workspace_bytes": (_sz, [_i32, _i32, _i32]),
    "cmh_cpf_tape_bytes": (_sz, [_i32, _i32, _i32]),
    "cmh_cpf_loss": (C.c_int, [_p, _p, _p, _p, _i32, _i32, _i32, _f, _f, _f, _f, _f, _f, _f, _p, _p, _p, _p, _p, _sz, _p]),
    "cmh_cpf_loss_backward": (C.c_int, [_p, _p, _p, _i32, _i32, _i32, _f, _f, _f, _f, _f, _p, _p, _p, _p, _p]),
    "cmh_djsrh_loss": (C.c_int, [_p, _p, _p, _i32, _i32, _f, _f, _p, _p, _p, _p, _sz, _p]),   # no upstream counterpart
    "cmh_djsrh_loss_backward": (C.c_int, [_p, _p, _p, _i32, _i32, _f, _f, _p, _p, _p, _p, _sz, _p]),   # no upstream counterpart
    "cmh_fp8_quantize_weight": (C.c_int, [_p, _p, _p, _i32, _i32, _p]),
    "cmh_fp8_quantize": (C.c_int, [_p, _i32, _p, _i64, _f, _p]),
    "cmh_fp8_dequantize": (C.c_int, [_p, _p, _i64, _f, _p]),
    "cmh_amax": (C.c_int, [_p, _i32, _i64, _p, _p]),
    "cmh_linear_gemm_fp8": (C.c_int, [_p, _p, _p, _f, _p, _p, _p, _f, _i32, _i32, _i32, _i32, _p]),
    "cmh_prof_gemm_begin": (C.c_int, [_i32]),
    "cmh_prof_gemm_end": (C.c_int, [C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_int64)]),
    "cmh_prof_gemm_by_kernel": (C.c_int, [C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_int64)]),
    "cmh_prof_gemm_conv1_fused": (C.c_int, [C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_int64)]),
    "cmh_set_conv1_fused": (C.c_int, [_i32]),
    "cmh_vit_patch_embed": (C.c_int, [C.POINTER(VitWeights), _p, _i32, _p, _i32, _i32, _p, _sz, _p, _p]),
    "cmh_cast_f32_to_bf16": (C.c_int, [_p, _p, _i64, _p]),
    "cmh_linear_act": (C.c_int, [_p, _p, _p, _p, _f, _i32, _p, _i32, _i32, _i32, _p]),
    "cmh_pair_softmax": (C.c_int, [_p, _p, _i32, _i32, _p]),
    "cmh_sign_codes": (C.c_int, [_p, _p, _i64, _p]),
    "cmh_pair_argmax_codes": (C.c_int, [_p, _p, _i32, _i32, _p]),
    "cmh_pack_codes": (C.c_int, [_p, _i64, _i32, _p, _p, _p, _p]),
    "cmh_unpack_codes": (C.c_int, [_p, _p, _i64, _i32, _p, _p]),
    "cmh_map_mean": (C.c_int, [_p, _i32, _p, _p]),
    "cmh_pack_labels": (C.c_int, [_p, _i64, _i32, _p, _p, _p]),
    "cmh_hamming_dist": (C.c_int, [_p, _p, _p, _p, _i32, _i64, _i32, _p, _p]),
    "cmh_calc_neighbor": (C.c_int, [_p, _p, _i32, _i32, _i32, _p, _p]),
    "cmh_map_workspace_bytes": (_sz, [_i32, _i64, _i32, _i32]),
    "cmh_hamming_map": (C.c_int, [_p, _p, _p, _p, _p, _p, _i32, _i64, _i32, _i32, _i64, _i32, _i32, _p, _p, _p,
                                  _p, _sz, _p]),
    "cmh_retrieval_workspace_bytes": (_sz, [_i32, _i64, _i32]),
    "cmh_hamming_hist": (C.c_int, [_p, _p, _p, _p, _p, _p, _i32, _i64, _i32, _i32, _p, _p, _sz, _p]),
    "cmh_hamming_topk": (C.c_int, [_p, _p, _p, _p, _p, _p, _i32, _i64, _i32, _i32, _i64, _p, _p, _p, _p, _p, _sz, _p]),
    "cmh_hamming_topk_graded": (C.c_int, [_p, _p, _p, _p, _p, _p, _i32, _i64, _i32, _i32, _i64, _p, _p, _p, _p, _p, _p, _sz, _p]),
    "cmh_map_count_workspace_bytes": (_sz, [_i32, _i64, _i32]),
    "cmh_hamming_ap_partial": (C.c_int, [_p, _p, _p, _p, _p, _p, _i32, _i64, _i32, _i32, _i64, _p, _p, _p, _p, _p, _sz, _p]),
    "cmh_range_workspace_bytes": (_sz, [_i32, _i64, _i32]),
    "cmh_hamming_range": (C.c_int, [_p, _p, _p, _p, _p, _p, _i32, _i64, _i32, _i32, _i32, _p, _p, _p, _i32, _p, _p, _p, _p, _p, _sz, _p]),
    "cmh_ap_finish": (C.c_int, [_p, _p, _i32, _i32, _i64, _p, _p, _p]),
    "cmh_rank_workspace_bytes": (_sz, [_i32, _i64, _i32, _i32]),
    "cmh_hamming_rank": (C.c_int, [_p, _p, _p, _p, _i32, _i64, _i32, _p, _p, _p, _i32, _p, _p, _sz, _p]),
    "cmh_label_overlap_workspace_bytes": (_sz, [_i32, _i64, _i32]),
    "cmh_label_overlap_hist": (C.c_int, [_p, _p, _i32, _i64, _i32, _p, _p, _sz, _p]),
    "cmh_topk_few_workspace_bytes": (_sz, [_i32, _i64, _i32]),
    "cmh_hamming_topk_few": (C.c_int, [_p, _p, _p, _p, _i32, _i64, _i32, _i32, _p, _p, _p, _sz, _p]),
    "cmh_soft_query_planes": (C.c_int, [_p, _i32, _i32, _p, _p, _p, _p, _p, _p]),
    "cmh_soft_topk_workspace_bytes": (_sz, [_i32, _i64, _i32]),
    "cmh_soft_topk": (C.c_int, [_p, _p, _p, _p, _i32, _i64, _i32, _i32, _p, _p, _p, _sz, _p]),
    "cmh_topk_few_masked_workspace_bytes": (_sz, [_i32, _i64, _i32]),
    "cmh_hamming_topk_few_masked": (C.c_int, [_p, _p, _p, _p, _p, _i32, _i64, _i32, _i32, _p, _p, _p, _p, _sz, _p]),
    "cmh_soft_ap_workspace_bytes": (_sz, [_i32, _i64, _i32, _i32]),
    "cmh_soft_ap": (C.c_int, [_p, _p, _p, _p, _p, _p, _i32, _i32, _i64, _i32, _i32, _p, _p, _p, _p, _sz, _p]),
    "cmh_soft_topk_masked_workspace_bytes": (_sz, [_i32, _i64, _i32]),
    "cmh_soft_topk_masked": (C.c_int, [_p, _p, _p, _p, _p, _i32, _i64, _i32, _i32, _p, _p, _p, _p, _sz, _p]),
    "cmh_mask_from_labels": (C.c_int, [_p, _p, _i32, _i64, _i32, _p, _p]),
    "cmh_mask_from_ids": (C.c_int, [_p, _i64, _i64, _i32, _p, _p, _p]),
    "cmh_code_gram_workspace_bytes": (_sz, [_i64, _i32, _i32, _i64]),
    "cmh_code_gram": (C.c_int, [_p, _p, _p, _p, _i64, _i32, _i32, _i64, _p, _p, _p, _p, _p, _p, _sz, _p]),
    "cmh_code_sort_workspace_bytes": (_sz, [_i64, _i32]),
    "cmh_code_sort": (C.c_int, [_p, _i64, _i32, _p, _p, _sz, _p]),
    "cmh_code_bucket_count": (C.c_int, [_p, _p, _i64, _i32, _p, _p, _p, _sz, _p]),
    "cmh_code_bucket_fill": (C.c_int, [_p, _p, _p, _i64, _i32, _i64, _p, _p, _p]),
    "cmh_bucket_probe_count": (C.c_int, [_p, _i32, _p, _p, _i64, _i32, _i32, _p, _p, _p]),
    "cmh_bucket_probe_fill": (C.c_int, [_p, _i32, _p, _p, _i64, _i32, _i32, _p, _i64, _p, _p, _p]),
    "cmh_mih_build_workspace_bytes": (_sz, [_i64, _i32]),
    "cmh_mih_build": (C.c_int, [_p, _i64, _i32, _p, _p, _p, _sz, _p]),
    "cmh_mih_count": (C.c_int, [_p, _i32, _p, _i64, _i32, _i32, _p, _p, _p, _p]),
    "cmh_mih_fill": (C.c_int, [_p, _i32, _p, _i64, _i32, _i32, _p, _p, _p, _i64, _p, _p, _p]),
    "cmh_mih_knn_count": (C.c_int, [_p, _i32, _p, _i64, _i32, _i32, _i32, _p, _p, _p, _p, _p, _p]),
    "cmh_mih_knn_fill": (C.c_int, [_p, _i32, _p, _i64, _i32, _p, _p, _p, _p, _i64, _p, _p, _p]),
    "cmh_topk_merge": (C.c_int, [_p, _p, _p, _i32, _p, _p, _p, _i32, _i32, _i32, _i32, _p, _p, _p, _p]),
    "cmh_loss_workspace_bytes": (_sz, [_i32, _i32, _i32]),
    "cmh_dsph_hyp_loss": (C.c_int, [_p, _p, _p, _p, _i32, _i32, _i32, _f, _f, _p, _p, _sz, _p]),
    "cmh_dchmt_loss": (C.c_int, [_p, _p, _p, _i32, _i32, _i32, _i32, _i32, _i32, _f, _f, _p, _p, _sz, _p]),
    "cmh_batchnorm1d_train": (C.c_int, [_p, _p, _p, _f, _p, _i32, _i32, _p]),
    "cmh_twdh_targets": (C.c_int, [_p, _p, _p, _p, _i32, _i32, _i32, _p]),
    "cmh_twdh_loss": (C.c_int, [_p, _p, _p, _i32, _i32, _p, _p, _sz, _p]),
    "cmh_dnph_loss": (C.c_int, [_p, _p, _p, _p, _p, _p, _p, _p, _i32, _i32, _i32, _f, _f, _p, _p, _sz, _p]),
    "cmh_assign_rows_workspace_bytes": (_sz, [_i32, _i32]),
    "cmh_assign_rows": (C.c_int, [_p, _p, _i32, _i32, _i32, _p, _p, _p, _sz, _p]),
    # training-free heads (csrc/itq.hip): none of the cmh_itq_* entries has an upstream counterpart
    "cmh_itq_moments_workspace_bytes": (_sz, [_i64, _i32]),             # no upstream counterpart
    "cmh_itq_moments": (C.c_int, [_p, _i64, _i32, _p, _p, _i32, _p, _sz, _p]),             # no upstream counterpart
    "cmh_itq_covariance": (C.c_int, [_p, _p, _p, _p, _i64, _i32, _p, _p, _p, _p, _p]),     # no upstream counterpart
    "cmh_itq_eigh_workspace_bytes": (_sz, [_i32, _i32]),                # no upstream counterpart
    "cmh_itq_eigh": (C.c_int, [_p, _i32, _i32, _p, _p, C.POINTER(C.c_int32), _p, _sz, _p]),   # no upstream counterpart
    "cmh_itq_project": (C.c_int, [_p, _i64, _i32, _i32, _p, _p, _p, _p, _p]),              # no upstream counterpart
    "cmh_itq_step_workspace_bytes": (_sz, [_i64, _i32]),                # no upstream counterpart
    "cmh_itq_step": (C.c_int, [_p, _i64, _i32, _p, _p, _p, _p, _p, _p, _sz, _p]),          # no upstream counterpart
    "cmh_itq_polar_workspace_bytes": (_sz, [_i32]),                     # no upstream counterpart
    "cmh_itq_polar": (C.c_int, [_p, _i32, _p, _p, _p, _sz, _p]),                            # no upstream counterpart
    "cmh_itq_rotate_workspace_bytes": (_sz, [_i64, _i32]),              # no upstream counterpart
    "cmh_itq_rotate": (C.c_int, [_p, _i64, _i32, _p, _i32, _p, _p, _p, _p, _sz, _p]),      # no upstream counterpart
    "cmh_itq_heads": (C.c_int, [_p, _p, _p, _p, _p, _p, _i64, _i32, _i32, _p, _p, _p, _p, _p, _p]),   # no upstream counterpart
    "cmh_itq_heads_pair": (C.c_int, [_p, _p, _p, _p, _p, _p, _p, _i64, _i32, _i32, _p, _p, _p, _p, _p, _p]),   # no upstream counterpart
    "cmh_itq_cross_moments_workspace_bytes": (_sz, [_i64, _i32]),       # no upstream counterpart
    "cmh_itq_cross_moments": (C.c_int, [_p, _p, _i64, _i32, _p, _i32, _p, _sz, _p]),       # no upstream counterpart
    "cmh_itq_cca_covariance": (C.c_int, [_p, _p, _p, _p, _p, _i64, _i32, _p, _p, _p, _p, _p, _p, _p]),   # no upstream counterpart
    "cmh_itq_inv_sqrt": (C.c_int, [_p, _i32, C.c_double, _p, _p, _p]),   # no upstream counterpart
    "cmh_itq_matmul": (C.c_int, [_p, _p, _p, _p, _i32, _i32, _i32, _i32, _i32, _p, _p]),   # no upstream counterpart
    # supervised training-free heads (csrc/dch.hip): none of the cmh_dch_* entries has an upstream counterpart
    "cmh_dch_covariance": (C.c_int, [_p, _p, _p, _i64, _i32, _p, _p]),                     # no upstream counterpart
    "cmh_dch_start": (C.c_int, [_p, _p, _i64, _i32, _p, _p]),                              # no upstream counterpart
    "cmh_dch_xtb_workspace_bytes": (_sz, [_i64, _i32, _i32]),           # no upstream counterpart
    "cmh_dch_xtb": (C.c_int, [_p, _p, _i64, _i32, _i32, _p, _p, _i32, _p, _sz, _p]),       # no upstream counterpart
    "cmh_dch_btb_workspace_bytes": (_sz, [_i64, _i32]),                 # no upstream counterpart
    "cmh_dch_btb": (C.c_int, [_p, _i64, _i32, _p, _p, _sz, _p]),                            # no upstream counterpart
    "cmh_dch_center": (C.c_int, [_p, _p, _p, _p, _i64, _i32, _i32, _p, _p]),               # no upstream counterpart
    "cmh_dch_solve": (C.c_int, [_p, C.c_double, _p, _i32, _i32, _p, _p, _p]),              # no upstream counterpart
    "cmh_dch_targets_workspace_bytes": (_sz, [_i64]),                   # no upstream counterpart
    "cmh_dch_targets": (C.c_int, [_p, _p, _p, _p, _p, C.c_double, C.c_double, _i64, _i32, _i32, _p, _p, _p, _sz, _p]),   # no upstream counterpart
    "cmh_dch_dcc_workspace_bytes": (_sz, [_i64, _i32]),                 # no upstream counterpart
    "cmh_dch_dcc": (C.c_int, [_p, _p, _p, _i64, _i32, _i32, _p, _p, _p, _sz, _p]),         # no upstream counterpart
    "cmh_vit_encode_tokens": (C.c_int, [C.POINTER(VitWeights), _p, _i32, _p, _p, _sz, _p]),
    "cmh_text_encode_tokens": (C.c_int, [C.POINTER(TextWeights), _p, _i32, _i32, _p, _p, _p, _p, _sz, _p]),
    "cmh_text_encode_tokens_packed": (C.c_int, [C.POINTER(TextWeights), _p, _i32, _i32, _p, _p, _p, _p, _sz, _p]),
    "cmh_blocks_workspace_bytes": (_sz, [_i32, _i32, _i32, _i32]),
    "cmh_transformer_blocks": (C.c_int, [C.POINTER(BlockWeights), _i32, _i32, _p, _i32, _i32, _i32, _i32, _p, _p, _sz, _p]),
    "cmh_mith_lta": (C.c_int, [_p, _p, _p, _p, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _p]),
    "cmh_add_positional": (C.c_int, [_p, _p, _i32, _i32, _i32, _p]),
    "cmh_bitwise_hash": (C.c_int, [_p, _p, _p, _p, _i32, _i32, _i32, _p]),
    "cmh_l2_normalize_rows": (C.c_int, [_p, _p, _i32, _i32, _p]),
    "cmh_mith_mix": (C.c_int, [_p, _p, _p, _p, _f, _p, _p, _p, _i64, _p]),
    "cmh_sq_diff_sum": (C.c_int, [_p, _p, _i64, _p, _p, _sz, _p]),
    "cmh_mith_bayesian_loss": (C.c_int, [_p, _p, _p, _p, _i32, _i32, _i32, _i32, _p, _p, _sz, _p]),
    "cmh_info_nce": (C.c_int, [_p, _p, _i32, _i32, _i32, _f, _p, _p, _sz, _p]),
    "cmh_transpose": (C.c_int, [_p, _i32, _p, _i32, _i32, _i32, _p]),
    "cmh_colsum_workspace_bytes": (_sz, [_i32, _i32]),
    "cmh_colsum": (C.c_int, [_p, _i32, _i32, _i32, _p, _p, _sz, _p]),
    "cmh_layernorm_backward_workspace_bytes": (_sz, [_i32, _i32]),
    "cmh_layernorm_backward": (C.c_int, [_p, _i32, _p, _i32, _p, _i32, _i32, _p, _i32, _p, _p, _p, _sz, _p]),
    "cmh_quick_gelu": (C.c_int, [_p, _p, _i64, _i32, _p]),
    "cmh_attention_backward": (C.c_int, [_i32, _p, _p, _p, _p, _i32, _i32, _i32, _i32, _p, _p]),
    "cmh_linear_wgrad_workspace_bytes": (_sz, [_i32, _i32, _i32, _i32]),
    "cmh_linear_wgrad": (C.c_int, [_i32, _p, _i32, _p, _i32, _i32, _i32, _i32, _p, _p, _p, _sz, _p]),
    "cmh_linear_act_backward": (C.c_int, [_p, _p, _p, _p, _p, _f, _i32, _p, _p, _p, _i32, _i32, _i32, _p, _sz, _p]),
    "cmh_head_backward_workspace_bytes": (_sz, [_i32, _i32, _i32]),
    "cmh_pair_softmax_backward": (C.c_int, [_p, _p, _p, _i32, _i32, _p]),
    "cmh_dchmt_loss_backward": (C.c_int, [_p, _p, _p, _i32, _i32, _i32, _i32, _i32, _i32, _f, _f, _p, _p, _p, _p, _sz, _p]),
    "cmh_dsph_hyp_loss_backward": (C.c_int, [_p, _p, _p, _p, _i32, _i32, _i32, _f, _f, _p, _p, _p, _p, _p, _sz, _p]),
    "cmh_dnph_backward_workspace_bytes": (_sz, [_i32, _i32, _i32]),
    "cmh_dnph_loss_backward": (C.c_int, [_p] * 8 + [_i32, _i32, _i32, _f, _f, _p] + [_p] * 5 + [_p, _sz, _p]),
    "cmh_image_preprocess_workspace_bytes": (_sz, [_i32, _i32, _i32, _i32]),
    "cmh_image_preprocess": (C.c_int, [_p, _p, _p, _i32, _i32, _i32, _i32, _i32, C.POINTER(C.c_float), C.POINTER(C.c_float),
                                       _p, _p, _p, _sz, _p]),
    "cmh_vit_forward_train_tokens": (C.c_int, [C.POINTER(VitWeights), _p, _i32, _p, _p, _sz, _p]),
    "cmh_vit_backward_tokens": (C.c_int, [C.POINTER(VitWeights), _i32, _p, C.POINTER(VitGrads), _p, _sz, _p]),
    "cmh_text_forward_train_tokens": (C.c_int, [C.POINTER(TextWeights), _p, _i32, _i32, _p, _p, _p, _p, _sz, _p]),
    "cmh_text_forward_train_tokens_packed": (C.c_int, [C.POINTER(TextWeights), _p, _i32, _i32, _p, _p, _p, _p, _sz, _p]),
    "cmh_text_backward_tokens": (C.c_int, [C.POINTER(TextWeights), _p, _i32, _i32, _p, _p, C.POINTER(TextGrads), _p, _sz, _p]),
    "cmh_blocks_train_bytes": (_sz, [_i32, _i32, _i32, _i32, _i32]),
    "cmh_blocks_forward_train": (C.c_int, [C.POINTER(BlockWeights), _i32, _i32, _p, _p, _i32, _i32, _i32, _p, _sz, _p]),
    "cmh_blocks_backward": (C.c_int, [C.POINTER(BlockWeights), C.POINTER(BlockGrads), _i32, _i32, _p, _p, _i32, _i32, _i32, _p, _sz, _p]),
    "cmh_mith_lta_backward": (C.c_int, [_p, _p, _p, _p, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _p]),
    "cmh_gelu": (C.c_int, [_p, _p, C.c_int64, _p]),
    "cmh_gelu_backward": (C.c_int, [_p, _p, _p, C.c_int64, _p]),
    "cmh_l2_normalize_backward": (C.c_int, [_p, _p, _p, _i32, _i32, _p]),
    "cmh_bitwise_hash_backward": (C.c_int, [_p, _p, _p, _p, _p, _p, _p, _i32, _i32, _i32, _p]),
    "cmh_mith_bayesian_backward_workspace_bytes": (_sz, [_i32, _i32]),
    "cmh_info_nce_workspace_bytes": (_sz, [_i32, _i32]),
    "cmh_mith_bayesian_loss_backward": (C.c_int, [_p, _p, _p, _p, _i32, _i32, _i32, _i32, _p, _p, _p, _sz, _p]),
    "cmh_info_nce_backward": (C.c_int, [_p, _p, _i32, _i32, _i32, _f, _p, _p, _p, _p, _sz, _p]),
    "cmh_sq_diff_sum_backward": (C.c_int, [_p, _p, C.c_int64, _p, _p, _p, _p]),
    "cmh_batchnorm1d_update_running": (C.c_int, [_p, _f, _p, _p, _i32, _i32, _p]),
    "cmh_batchnorm1d_backward": (C.c_int, [_p, _p, _f, _p, _p, _p, _p, _i32, _i32, _p]),
    "cmh_twdh_loss_backward": (C.c_int, [_p, _p, _p, _i32, _i32, _p, _p, _p, _p, _p]),
    "cmh_image_normalize": (C.c_int, [_p, _p, _i32, _i32, C.POINTER(C.c_float), C.POINTER(C.c_float), _p, _p]),
    "cmh_bpe_create": (C.c_int, [C.c_char_p, _sz, C.POINTER(_p)]),
    "cmh_bpe_destroy": (None, [_p]),
    "cmh_bpe_vocab_size": (_i32, [_p]),
    "cmh_bpe_encode_captions": (C.c_int, [_p, C.c_char_p, _p, _i32, _i32, _p, _p, _i32]),
    "cmh_vit_train_bytes": (_sz, [C.POINTER(VitWeights), _i32]),
    "cmh_vit_forward_train": (C.c_int, [C.POINTER(VitWeights), _p, _i32, _p, _p, _sz, _p]),
    "cmh_vit_backward": (C.c_int, [C.POINTER(VitWeights), _i32, _p, C.POINTER(VitGrads), _p, _sz, _p]),
    "cmh_vit_backward_part": (C.c_int, [C.POINTER(VitWeights), _i32, _p, C.POINTER(VitGrads), _p, _sz, _i32, _i32, _p]),
    "cmh_text_train_bytes": (_sz, [C.POINTER(TextWeights), _i32, _i32]),
    "cmh_text_forward_train": (C.c_int, [C.POINTER(TextWeights), _p, _i32, _i32, _p, _p, _p, _sz, _p]),
    "cmh_text_backward": (C.c_int, [C.POINTER(TextWeights), _p, _i32, _i32, _p, _p, C.POINTER(TextGrads), _p, _sz, _p]),
    "cmh_text_backward_part": (C.c_int, [C.POINTER(TextWeights), _p, _i32, _i32, _p, _p, C.POINTER(TextGrads), _p, _sz, _i32, _i32, _p]),
    "cmh_bert_adam_workspace_bytes": (_sz, [_i32, _i64]),
    "cmh_bert_adam_step": (C.c_int, [C.POINTER(AdamTensor), _i32, C.c_double, C.c_double, C.c_double, _p, _sz, _p]),
}


def lib():
    """Load libcmh.so (built by `__graft_entry__.build()` / `make -C csrc`).  Fails loudly."""
    global _lib
    with _lock:
        if _lib is None:
            if not os.path.exists(LIB_PATH):
                raise NativeError(
                    f"{LIB_PATH} is missing: build it with `python __graft_entry__.py` (or `make -C "
                    f"{os.path.dirname(os.path.dirname(LIB_PATH))}`); there is no CPU fallback for the hot path")
            l = C.CDLL(LIB_PATH)
            for name, (res, args) in SIGNATURES.items():
                fn = getattr(l, name)          # AttributeError if the ABI lost a symbol
                fn.restype, fn.argtypes = res, args
            if l.cmh_version() != ABI_VERSION:  # a stale or diagnostic build with other struct layouts would read garbage pointers
                raise NativeError(f"{LIB_PATH}: cmh_version() = {l.cmh_version()}, this binding was written for {ABI_VERSION}; rebuild it")
            _lib = l
    return _lib


def check(rc: int, what: str):
    if rc != 0:
        raise NativeError(f"{what} failed (code {rc}): {lib().cmh_last_error().decode(errors='replace')}")


# ------------------------------------------------------------------------------------------ helpers
def require_gpu(*tensors):
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise NativeError("libcmh runs on the GPU only (tensor on %s); there is no CPU fallback" % t.device)


def ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def stream_ptr(device=None):
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


_ws_cache: dict = {}


def workspace(nbytes: int, device, tag: str = "") -> torch.Tensor:
    """Per-(device, CURRENT STREAM, tag) grow-only scratch buffer (uint8, 256-byte aligned by the caching allocator).  One buffer per
    stream: the towers, the two branches of MITH's HashingModel and consecutive batches of the evaluation loops run on different
    streams at the same time, and a scratch buffer shared between them would be a data race (round-4 advisor finding)."""
    key = (str(device), int(torch.cuda.current_stream(device).cuda_stream) if torch.cuda.is_available() else 0, tag)
    buf = _ws_cache.get(key)
    if buf is None or buf.numel() < nbytes:
        buf = torch.empty(max(int(nbytes), 256), dtype=torch.uint8, device=device)
        _ws_cache[key] = buf
    return buf


def f32c(t: torch.Tensor) -> torch.Tensor:
    if t.dtype != torch.float32:
        t = t.float()
    return t.contiguous()


def cast_bf16(src: torch.Tensor) -> torch.Tensor:
    """f32 -> bf16 copy through the library's RNE cast kernel."""
    src = f32c(src)
    require_gpu(src)
    dst = torch.empty(src.shape, dtype=torch.bfloat16, device=src.device)
    check(lib().cmh_cast_f32_to_bf16(ptr(src), ptr(dst), src.numel(), stream_ptr(src.device)), "cmh_cast_f32_to_bf16")
    return dst


def _kind(t: torch.Tensor) -> int:
    return {torch.float32: 0, torch.bfloat16: 1, torch.float16: 2}[t.dtype]


def fp8_quantize_weight(w: torch.Tensor):
    """w f32 [N,K] -> (e4m3 bytes [N,K] uint8, colscale f32 [N]) with w ~ fp8 * colscale[:, None]."""
    w = f32c(w)
    require_gpu(w)
    Nn, K = w.shape
    q = torch.empty(Nn, K, dtype=torch.uint8, device=w.device)
    cs = torch.empty(Nn, dtype=torch.float32, device=w.device)
    check(lib().cmh_fp8_quantize_weight(ptr(w), ptr(q), ptr(cs), Nn, K, stream_ptr(w.device)), "cmh_fp8_quantize_weight")
    return q, cs


def fp8_quantize(x: torch.Tensor, scale: float) -> torch.Tensor:
    """x (f32 / bf16 / f16) -> e4m3 bytes of clamp(x / scale, +-448), same shape, uint8."""
    require_gpu(x)
    x = x.contiguous()
    q = torch.empty(x.shape, dtype=torch.uint8, device=x.device)
    check(lib().cmh_fp8_quantize(ptr(x), _kind(x), ptr(q), x.numel(), float(scale), stream_ptr(x.device)), "cmh_fp8_quantize")
    return q


def fp8_dequantize(q: torch.Tensor, scale: float = 1.0) -> torch.Tensor:
    require_gpu(q)
    q = q.contiguous()
    out = torch.empty(q.shape, dtype=torch.float32, device=q.device)
    check(lib().cmh_fp8_dequantize(ptr(q), ptr(out), q.numel(), float(scale), stream_ptr(q.device)), "cmh_fp8_dequantize")
    return out


def amax(x: torch.Tensor, into: torch.Tensor | None = None) -> torch.Tensor:
    """max |x| as a device scalar (accumulated into `into` when given)."""
    require_gpu(x)
    x = x.contiguous()
    out = torch.zeros(1, dtype=torch.float32, device=x.device) if into is None else into
    check(lib().cmh_amax(ptr(x), _kind(x), x.numel(), ptr(out), stream_ptr(x.device)), "cmh_amax")
    return out


EPI_OUT_FP8 = 4096


def linear_gemm_fp8(x8, w8, colscale, alpha, bias=None, residual=None, quickgelu=False, out="f32", out_scale=1.0):
    """epi(alpha * colscale[n] * (x8 @ w8.T)) on e4m3 operands (uint8 tensors); out in {"f32", "bf16", "f16", "fp8"}."""
    require_gpu(x8, w8, colscale, bias, residual)
    if x8.dtype != torch.uint8 or w8.dtype != torch.uint8:
        raise NativeError("linear_gemm_fp8: operands are e4m3 bytes (uint8 tensors)")
    x8, w8 = x8.contiguous(), w8.contiguous()
    M, K = x8.shape
    Nn = w8.shape[0]
    if w8.shape[1] != K or colscale.numel() != Nn or (bias is not None and bias.numel() != Nn) or \
            (residual is not None and tuple(residual.shape) != (M, Nn)):
        raise NativeError(f"linear_gemm_fp8: x {tuple(x8.shape)}, w {tuple(w8.shape)}, colscale / bias / residual shapes do not fit together")
    odt = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16, "fp8": torch.uint8}[out]
    o = torch.empty(M, Nn, dtype=odt, device=x8.device)
    res_f16 = residual is not None and residual.dtype == torch.float16
    if residual is not None:
        residual = residual.contiguous() if res_f16 else f32c(residual)
    epi = (EPI_BIAS if bias is not None else 0) | (EPI_QUICKGELU if quickgelu else 0) | (EPI_RESIDUAL if residual is not None else 0) | \
          (EPI_RES_F16 if res_f16 else 0) | {"f32": 0, "bf16": EPI_OUT_BF16, "f16": EPI_OUT_F16, "fp8": EPI_OUT_FP8}[out]
    check(lib().cmh_linear_gemm_fp8(ptr(x8), ptr(w8), ptr(f32c(colscale)), float(alpha), ptr(None if bias is None else f32c(bias)),
                                    ptr(residual), ptr(o), float(out_scale), M, Nn, K, epi, stream_ptr(x8.device)), "cmh_linear_gemm_fp8")
    return o


def set_gemm_grouped(on: int = -1):
    """Layer i of both towers as ONE grouped GEMM launch (csrc/gemm_wide.hip, GRP): 1 on (default), 0 = two plain launches, -1 = environment
    (CMH_GEMM_GROUPED=0 is off).  Results never depend on it."""
    check(lib().cmh_set_gemm_grouped(int(on)), "cmh_set_gemm_grouped")


def linear_gemm_grouped(problems, quickgelu=False, out="f32", m_dev=(None, None)):
    """Two GEMMs of one kind as one launch (include/cmh.h: cmh_linear_gemm_grouped).  problems = two dicts with x, w and optionally
    bias, residual, and - e4m3 operands (uint8 tensors) - colscale, alpha, out_scale; out in {"f32", "bf16", "f16", "fp8"};
    m_dev: per problem an int32 device tensor holding the real row count (or None).  Returns the two outputs."""
    assert len(problems) == 2
    kinds = {("u8" if p["x"].dtype == torch.uint8 else ("bf16" if p["x"].dtype == torch.bfloat16 else "f32")) for p in problems}
    if len(kinds) != 1:
        raise NativeError("linear_gemm_grouped: both problems must share the operand type")
    kind = kinds.pop()
    dt = {"f32": F32, "bf16": BF16, "u8": FP8}[kind]
    odt = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16, "fp8": torch.uint8}[out]
    has_bias = problems[0].get("bias") is not None
    has_res = problems[0].get("residual") is not None
    res_f16 = has_res and problems[0]["residual"].dtype == torch.float16
    epi = (EPI_BIAS if has_bias else 0) | (EPI_QUICKGELU if quickgelu else 0) | (EPI_RESIDUAL if has_res else 0) | \
          (EPI_RES_F16 if res_f16 else 0) | {"f32": 0, "bf16": EPI_OUT_BF16, "f16": EPI_OUT_F16, "fp8": EPI_OUT_FP8}[out]
    structs, outs, keep = [], [], []
    for p, md in zip(problems, m_dev):
        x, w = p["x"].contiguous(), p["w"].contiguous()
        require_gpu(x, w, p.get("bias"), p.get("residual"), p.get("colscale"), md)
        M, K = x.shape
        Nn = w.shape[0]
        if w.shape[1] != K or (p.get("bias") is not None) != has_bias or (p.get("residual") is not None) != has_res or \
                (has_bias and p["bias"].numel() != Nn) or (has_res and tuple(p["residual"].shape) != (M, Nn)) or \
                (kind == "u8" and (p.get("colscale") is None or p["colscale"].numel() != Nn)):
            raise NativeError(f"linear_gemm_grouped: x {tuple(x.shape)}, w {tuple(w.shape)}: operand shapes / kinds do not fit together")
        o = torch.empty(M, Nn, dtype=odt, device=x.device)
        bias = f32c(p["bias"]) if has_bias else None
        res = None
        if has_res:
            res = p["residual"].contiguous() if res_f16 else f32c(p["residual"])
        cs = f32c(p["colscale"]) if kind == "u8" else None
        g = GemmProblem(ptr(x), ptr(w), ptr(bias), ptr(res), ptr(o), M, Nn, K, ptr(md), ptr(cs), float(p.get("alpha", 1.0)),
                        float(p.get("out_scale", 1.0)))
        structs.append(g)
        outs.append(o)
        keep += [x, w, bias, res, cs]
    check(lib().cmh_linear_gemm_grouped(dt, C.byref(structs[0]), C.byref(structs[1]), epi, stream_ptr(outs[0].device)),
          "cmh_linear_gemm_grouped")
    return outs


def set_pooled_tail(on: bool):
    """Carry only the pooled rows through the last block of encode_image / encode_text (default on; include/cmh.h)."""
    check(lib().cmh_set_pooled_tail(1 if on else 0), "cmh_set_pooled_tail")


def set_conv1_fused(on: int = -1):
    """The image tower's inference stem as one implicit-GEMM launch (csrc/conv1_stem.hip): 1 on (default), 0 = patchify + GEMM,
    -1 = environment (CMH_CONV1_FUSED).  Same bits either way."""
    check(lib().cmh_set_conv1_fused(int(on)), "cmh_set_conv1_fused")


def set_gemm_rows(on: int = -1):
    """Few-row GEMMs (M <= 512) on 64 x 64 tiles (csrc/gemm_rows.hip): 1 on (default), 0 = the wide kernel takes them, -1 = environment."""
    check(lib().cmh_set_gemm_rows(int(on)), "cmh_set_gemm_rows")


def set_text_token_packing(on: int):
    """the all-token text trunk (MITH) skips the positions behind a caption's last unpadded token (1, the default); 0: computes every
    position; -1 = CMH_TEXT_PACK_TOKENS"""
    check(lib().cmh_set_text_token_packing(int(on)), "cmh_set_text_token_packing")


def set_grad_stream16(on: int):
    """bf16 training mode: carry the towers' residual-gradient stream as bf16 (1, the default), as f32 (0); -1 = CMH_GRAD_STREAM16"""
    check(lib().cmh_set_grad_stream16(int(on)), "cmh_set_grad_stream16")


def set_gemm_lc(mode: int):
    """Loader / consumer GEMM kernels (csrc/gemm_lc.hip): -1 environment (CMH_GEMM_LC, unset = 8), 0 the wide kernel only, 1 / 2 / 3 the
    8-wave kernel for every eligible launch (2: all but the QuickGELU launches; otherwise alike), 4 the 12-wave 128-row form, 7 the fp8
    QKV form, 8 per launch the 12-wave 160-row form or the wide kernel, whichever the cost model prices lower (the default; never the
    128-row form), 9 the 12-wave 160-row form for every eligible launch."""
    check(lib().cmh_set_gemm_lc(int(mode)), "cmh_set_gemm_lc")


def gemm_route(a, b=None, epi=0, dt=None):
    """Which kernel takes a bf16 launch of shape a = (M, N, K) (grouped with b) under the current set_gemm_lc mode, without launching
    it: 0 the wide kernel, 1 the 8-wave loader / consumer kernel, 2 the 12-wave 128-row form, 3 the 12-wave 160-row form."""
    mb, nb, kb = b if b is not None else (0, 0, 0)
    rc = lib().cmh_gemm_route(BF16 if dt is None else dt, *a, mb, nb, kb, int(epi))
    if rc < 0:
        raise NativeError(f"cmh_gemm_route: {lib().cmh_last_error()}")
    return rc


PLAN_FIELDS = ("family", "rows", "grid", "order", "dge", "res", "grouped")


def gemm_plan(a, b=None, epi=0, dt=None):
    """The plan of a GEMM request under the current switches, without launching it (include/cmh.h: cmh_gemm_plan).  a, b: (M, N, K) or
    (M, N, K, rows_on_device, hint).  -> (route, [one dict of PLAN_FIELDS per launch])."""
    def five(s):
        return (_i32 * 5)(*(tuple(s) + (0, 0))[:5])
    out = (_i32 * 16)()
    check(lib().cmh_gemm_plan(BF16 if dt is None else dt, int(epi), five(a), None if b is None else five(b), out), "cmh_gemm_plan")
    return out[1], [dict(zip(PLAN_FIELDS, out[2 + 7 * i:9 + 7 * i])) for i in range(out[0])]


def gemm_tuning(tile_rows: int = -1, order_group: int = -1):
    """Pin the wide GEMM's tile height (96 / 128 / 160) and tile-order group (0 = n-fastest); -1 = automatic."""
    check(lib().cmh_gemm_tuning(int(tile_rows), int(order_group)), "cmh_gemm_tuning")


def prof_gemm_begin(max_launches: int):
    check(lib().cmh_prof_gemm_begin(int(max_launches)), "cmh_prof_gemm_begin")


def prof_gemm_end():
    """-> (sum of GEMM launch durations [ms], sum of algorithmic FLOPs, number of launches)"""
    ms, fl, n = C.c_double(), C.c_double(), C.c_int64()
    check(lib().cmh_prof_gemm_end(C.byref(ms), C.byref(fl), C.byref(n)), "cmh_prof_gemm_end")
    return ms.value, fl.value, n.value


def prof_gemm_by_kernel():
    """after prof_gemm_end(): {kernel: (ms, flops, launches)} of the timed launches, split by the kernel that ran them"""
    ms, fl, n = (C.c_double * 3)(), (C.c_double * 3)(), (C.c_int64 * 3)()
    check(lib().cmh_prof_gemm_by_kernel(ms, fl, n), "cmh_prof_gemm_by_kernel")
    by = {k: (ms[i], fl[i], n[i]) for i, k in enumerate(("gemm_wide_kernel", "gemm_rows_kernel", "fallback"))}
    c_ms, c_fl, c_n = C.c_double(), C.c_double(), C.c_int64()
    check(lib().cmh_prof_gemm_conv1_fused(C.byref(c_ms), C.byref(c_fl), C.byref(c_n)), "cmh_prof_gemm_conv1_fused")
    if c_n.value:           # the fused conv1 stem (set_conv1_fused), listed in the sessions that launched it
        by["conv1_stem_kernel"] = (c_ms.value, c_fl.value, c_n.value)
    return by


# ------------------------------------------------------------------------------------------ tower blocks
EPI_BIAS, EPI_QUICKGELU, EPI_RESIDUAL, EPI_OUT_BF16 = 1, 2, 4, 8
EPI_RES_F16, EPI_OUT_F16 = 64, 128


def linear_gemm(x, w, bias=None, residual=None, quickgelu=False, out_bf16=False, out_f16=False):
    """out = epi(x @ w.T); x,w both f32 or both bf16 (dtype picks the MFMA path).  A float16 `residual` / `out_f16` is the
    bf16 mode's fp16 residual stream (CMH_EPI_RES_F16 / CMH_EPI_OUT_F16, N % 256 == 0)."""
    require_gpu(x, w, bias, residual)
    dt = BF16 if x.dtype == torch.bfloat16 else F32
    if (w.dtype == torch.bfloat16) != (dt == BF16):
        raise NativeError("linear_gemm: x and w must share a dtype")
    if out_bf16 and out_f16:
        raise NativeError("linear_gemm: out_bf16 and out_f16 exclude each other")
    x, w = x.contiguous(), w.contiguous()
    M, K = x.shape
    Nn = w.shape[0]
    if w.dim() != 2 or w.shape[1] != K or (bias is not None and bias.numel() != Nn) or \
            (residual is not None and tuple(residual.shape) != (M, Nn)):
        raise NativeError(f"linear_gemm: x {tuple(x.shape)}, w {tuple(w.shape)}, bias / residual shapes do not fit together")
    odt = torch.bfloat16 if out_bf16 else (torch.float16 if out_f16 else torch.float32)
    out = torch.empty(M, Nn, dtype=odt, device=x.device)
    res_f16 = residual is not None and residual.dtype == torch.float16
    if residual is not None:
        residual = residual.contiguous() if res_f16 else f32c(residual)
    epi = (EPI_BIAS if bias is not None else 0) | (EPI_QUICKGELU if quickgelu else 0) | \
          (EPI_RESIDUAL if residual is not None else 0) | (EPI_OUT_BF16 if out_bf16 else 0) | \
          (EPI_RES_F16 if res_f16 else 0) | (EPI_OUT_F16 if out_f16 else 0)
    check(lib().cmh_linear_gemm(dt, ptr(x), ptr(w), ptr(None if bias is None else f32c(bias)), ptr(residual), ptr(out),
                                M, Nn, K, epi, stream_ptr(x.device)), "cmh_linear_gemm")
    return out


def layernorm(x, w, b, out_bf16=False):
    x, w, b = f32c(x), f32c(w), f32c(b)
    require_gpu(x, w, b)
    M, d = x.shape
    if w.numel() != d or b.numel() != d:
        raise NativeError(f"layernorm: rows of {d} elements, weight {tuple(w.shape)}, bias {tuple(b.shape)}")
    out = torch.empty(M, d, dtype=torch.bfloat16 if out_bf16 else torch.float32, device=x.device)
    check(lib().cmh_layernorm(ptr(x), ptr(w), ptr(b), ptr(out), BF16 if out_bf16 else F32, M, d, stream_ptr(x.device)),
          "cmh_layernorm")
    return out


def attention(qkv, B, T, causal, key_padding_mask=None):
    require_gpu(qkv, key_padding_mask)
    qkv = qkv.contiguous()
    dt = BF16 if qkv.dtype == torch.bfloat16 else F32
    d = qkv.shape[1] // 3
    o = torch.empty(B * T, d, dtype=qkv.dtype, device=qkv.device)
    kpm = None if key_padding_mask is None else key_padding_mask.to(torch.uint8).contiguous()
    check(lib().cmh_attention(dt, ptr(qkv), ptr(o), B, T, d, int(bool(causal)), ptr(kpm), stream_ptr(qkv.device)),
          "cmh_attention")
    return o


def attention_pair(qkv0, B0, T0, causal0, qkv1, B1, T1, causal1, key_padding_mask0=None, key_padding_mask1=None, out=None):
    """Both attentions in one launch -> (o0, o1), or None when the library has no pair kernel for these two problems (nothing was
    launched; call `attention` twice).  out: optional (o0, o1) buffers to write into."""
    require_gpu(qkv0, qkv1, key_padding_mask0, key_padding_mask1)
    if qkv0.dtype != qkv1.dtype:
        raise NativeError("attention_pair: the two problems differ in dtype")
    qkv0, qkv1 = qkv0.contiguous(), qkv1.contiguous()
    dt = BF16 if qkv0.dtype == torch.bfloat16 else F32
    d0, d1 = qkv0.shape[1] // 3, qkv1.shape[1] // 3
    o0, o1 = out if out is not None else (torch.empty(B0 * T0, d0, dtype=qkv0.dtype, device=qkv0.device),
                                          torch.empty(B1 * T1, d1, dtype=qkv1.dtype, device=qkv1.device))
    k0 = None if key_padding_mask0 is None else key_padding_mask0.to(torch.uint8).contiguous()
    k1 = None if key_padding_mask1 is None else key_padding_mask1.to(torch.uint8).contiguous()
    rc = lib().cmh_attention_pair(dt, ptr(qkv0), ptr(o0), B0, T0, d0, int(bool(causal0)), ptr(k0),
                                  ptr(qkv1), ptr(o1), B1, T1, d1, int(bool(causal1)), ptr(k1), stream_ptr(qkv0.device))
    if rc == 1:
        return None
    check(rc, "cmh_attention_pair")
    return o0, o1


# ------------------------------------------------------------------------------------------ heads
def linear_act(x, w, b, act=ACT_NONE, drop_mask=None, p=0.2):
    x, w = f32c(x), f32c(w)
    b = None if b is None else f32c(b)
    require_gpu(x, w, b, drop_mask)
    M, K = x.shape
    N = w.shape[0]
    if w.shape[1] != K:
        raise NativeError(f"linear_act: x [{M},{K}] vs w {tuple(w.shape)}")
    y = torch.empty(M, N, dtype=torch.float32, device=x.device)
    dm = None if drop_mask is None else f32c(drop_mask)
    check(lib().cmh_linear_act(ptr(x), ptr(w), ptr(b), ptr(dm), 1.0 / (1.0 - p), act, ptr(y), M, N, K,
                               stream_ptr(x.device)), "cmh_linear_act")
    return y


def pair_softmax(z):
    z = f32c(z)
    require_gpu(z)
    M, K2 = z.shape
    out = torch.empty_like(z)
    check(lib().cmh_pair_softmax(ptr(z), ptr(out), M, K2 // 2, stream_ptr(z.device)), "cmh_pair_softmax")
    return out


def sign_codes(h):
    h = f32c(h)
    require_gpu(h)
    out = torch.empty_like(h)
    check(lib().cmh_sign_codes(ptr(h), ptr(out), h.numel(), stream_ptr(h.device)), "cmh_sign_codes")
    return out


def pair_argmax_codes(p):
    p = f32c(p)
    require_gpu(p)
    M, K2 = p.shape
    out = torch.empty(M, K2 // 2, dtype=torch.float32, device=p.device)
    check(lib().cmh_pair_argmax_codes(ptr(p), ptr(out), M, K2 // 2, stream_ptr(p.device)), "cmh_pair_argmax_codes")
    return out


# ------------------------------------------------------------------------------------------ hamming / mAP
def pack_codes(codes, validate=True):
    """f32 codes in {-1,0,+1} [n, K] -> (sign_plane, nz_plane) int32 [n, ceil(K/32)].
    validate=True reads the device-side domain flag back (one host sync); pass False on a timed path."""
    codes = f32c(codes)
    require_gpu(codes)
    n, K = codes.shape
    W = (K + 31) // 32
    sp = torch.empty(n, W, dtype=torch.int32, device=codes.device)
    nz = torch.empty(n, W, dtype=torch.int32, device=codes.device)
    bad = torch.zeros(1, dtype=torch.int32, device=codes.device)
    check(lib().cmh_pack_codes(ptr(codes), n, K, ptr(sp), ptr(nz), ptr(bad), stream_ptr(codes.device)), "cmh_pack_codes")
    if validate and int(bad.item()):
        raise NativeError("pack_codes: hash codes must be exactly -1, 0 or +1 (sign()/argmax codes)")
    return sp, nz


def unpack_codes(sign_plane, nz_plane, bits: int):
    """(sign_plane, nz_plane) int32 [n, ceil(bits/32)] -> f32 codes [n, bits] in {-1, 0, +1} (the inverse of pack_codes)."""
    require_gpu(sign_plane, nz_plane)
    sp, nz = sign_plane.contiguous(), nz_plane.contiguous()
    n, W = sp.shape
    if sp.dtype != torch.int32 or nz.dtype != torch.int32 or tuple(nz.shape) != (n, W) or W != (int(bits) + 31) // 32:
        raise NativeError(f"unpack_codes: planes {tuple(sp.shape)} / {tuple(nz.shape)} do not hold {bits}-bit codes")
    out = torch.empty(n, int(bits), dtype=torch.float32, device=sp.device)
    if n:
        check(lib().cmh_unpack_codes(ptr(sp), ptr(nz), n, int(bits), ptr(out), stream_ptr(sp.device)), "cmh_unpack_codes")
    return out


def map_mean(ap):
    """f32 [Q] per-query APs -> their mean as the ranking kernel forms it: a sequential f32 sum in query order, / Q (0-dim tensor)."""
    ap = f32c(ap)
    require_gpu(ap)
    out = torch.empty(1, dtype=torch.float32, device=ap.device)
    check(lib().cmh_map_mean(ptr(ap), ap.numel(), ptr(out), stream_ptr(ap.device)), "cmh_map_mean")
    return out[0]


def pack_labels(labels):
    labels = f32c(labels)
    require_gpu(labels)
    n, Cn = labels.shape
    LW = (Cn + 31) // 32
    out = torch.empty(n, LW, dtype=torch.int32, device=labels.device)
    bad = torch.zeros(1, dtype=torch.int32, device=labels.device)
    check(lib().cmh_pack_labels(ptr(labels), n, Cn, ptr(out), ptr(bad), stream_ptr(labels.device)), "cmh_pack_labels")
    if int(bad.item()):
        raise NativeError("pack_labels: labels must be non-negative (multi-hot)")
    return out


def hamming_dist(q_planes, r_planes, bits):
    (qs, qn), (rs, rn) = q_planes, r_planes
    Q, N = qs.shape[0], rs.shape[0]
    W = (bits + 31) // 32
    fit("hamming_dist", (qs, (Q, W)), (qn, (Q, W)), (rs, (N, W)), (rn, (N, W)))
    out = torch.empty(Q, N, dtype=torch.float32, device=qs.device)
    check(lib().cmh_hamming_dist(ptr(qs), ptr(qn), ptr(rs), ptr(rn), Q, N, bits, ptr(out), stream_ptr(qs.device)),
          "cmh_hamming_dist")
    return out


def calc_neighbor(la, lb, classes):
    A, B = la.shape[0], lb.shape[0]
    fit("calc_neighbor", (la, (A, (classes + 31) // 32)), (lb, (B, (classes + 31) // 32)))
    out = torch.empty(A, B, dtype=torch.float32, device=la.device)
    check(lib().cmh_calc_neighbor(ptr(la), ptr(lb), A, B, classes, ptr(out), stream_ptr(la.device)), "cmh_calc_neighbor")
    return out


def hamming_map(q_planes, q_lab, r_planes, r_lab, bits, classes, topk=None, tie_order=TIE_REFERENCE,
                want_perm=False, depth_limit=-1):
    """-> (map 0-dim f32 tensor, ap [Q] f32, perm [Q,N] int32 or None)"""
    (qs, qn), (rs, rn) = q_planes, r_planes
    dev = qs.device
    Q, N = qs.shape[0], rs.shape[0]
    W, LW = (bits + 31) // 32, (classes + 31) // 32
    fit("hamming_map", (qs, (Q, W)), (qn, (Q, W)), (rs, (N, W)), (rn, (N, W)), (q_lab, (Q, LW)), (r_lab, (N, LW)))
    ap = torch.empty(Q, dtype=torch.float32, device=dev)
    mp = torch.empty(1, dtype=torch.float32, device=dev)
    perm = torch.empty(Q, N, dtype=torch.int32, device=dev) if want_perm else None
    need = lib().cmh_map_workspace_bytes(Q, N, bits, tie_order)
    ws = workspace(need, dev, "map")
    check(lib().cmh_hamming_map(ptr(qs), ptr(qn), ptr(q_lab), ptr(rs), ptr(rn), ptr(r_lab), Q, N, bits, classes,
                                0 if topk is None else int(topk), tie_order, depth_limit, ptr(ap), ptr(mp), ptr(perm),
                                ptr(ws), ws.numel(), stream_ptr(dev)), "cmh_hamming_map")
    return mp[0], ap, perm


def _retrieval_operands(what, q_planes, r_planes, bits, q_lab, r_lab):
    (qs, qn), (rs, rn) = q_planes, r_planes
    require_gpu(qs, qn, rs, rn, q_lab, r_lab)
    Q, N = qs.shape[0], rs.shape[0]
    W = (int(bits) + 31) // 32
    if (q_lab is None) != (r_lab is None):
        raise NativeError(f"{what}: labels on one side only")
    LW = 0 if q_lab is None else q_lab.shape[1]
    fit(what, (qs, (Q, W)), (qn, (Q, W)), (rs, (N, W)), (rn, (N, W)), (q_lab, (Q, LW)), (r_lab, (N, LW)))
    for t in (qs, qn, rs, rn, q_lab, r_lab):
        if t is not None and (t.dtype != torch.int32 or not t.is_contiguous()):
            raise NativeError(f"{what}: packed operands are contiguous int32 tensors (pack_codes / pack_labels)")
    return qs, qn, rs, rn, Q, N, LW


check_retrieval_operands = _retrieval_operands      # for callers that use labels beside a native call that takes none (utils/retrieval.py)


def hamming_hist(q_planes, r_planes, bits, q_lab=None, r_lab=None):
    """-> counts int32 [Q, 2*bits+1, 2]: counts[i, h, 1] = database items at calc_hammingDist == h/2 from query i that share a
    label with it, counts[i, h, 0] = the others (everything without labels)."""
    qs, qn, rs, rn, Q, N, LW = _retrieval_operands("hamming_hist", q_planes, r_planes, bits, q_lab, r_lab)
    dev = qs.device
    counts = torch.empty(Q, 2 * int(bits) + 1, 2, dtype=torch.int32, device=dev)
    ws = workspace(lib().cmh_retrieval_workspace_bytes(Q, N, int(bits)), dev, "retrieval")
    check(lib().cmh_hamming_hist(ptr(qs), ptr(qn), ptr(q_lab), ptr(rs), ptr(rn), ptr(r_lab), Q, N, int(bits), 32 * LW,
                                 ptr(counts), ptr(ws), ws.numel(), stream_ptr(dev)), "cmh_hamming_hist")
    return counts


def _counts_operand(what, name, t, Q, bits, dev):
    if t is None:
        return None
    fit(what, (t, (Q, 2 * int(bits) + 1, 2)))
    if t.dtype != torch.int32 or not t.is_contiguous() or t.device != dev:
        raise NativeError(f"{what}: {name} is a contiguous int32 tensor [Q, 2 * bits + 1, 2] on the operands' device (hamming_hist)")
    return t


def hamming_ap_partial(q_planes, r_planes, bits, q_lab, r_lab, topk=None, total_counts=None, prior_counts=None, want_counts=False):
    """The AP sums of one database shard by counting (no ranking): -> ap_sum float64 [Q] = the sum, over the shard's relevant items
    whose rank among the relevant items of the WHOLE database is <= min(k, R), of relrank / rank; ties by ascending database index
    (torch.sort(stable=True)).  total_counts / prior_counts: hamming_hist's histograms of the whole database and of the shards
    before this one (None: this call's own / none).  topk=None: k = the whole database.  [+ this shard's counts with want_counts].
    The sums of the shards add; ap_finish turns them into APs."""
    if q_lab is None or r_lab is None:
        raise NativeError("hamming_ap_partial: needs the labels of both sides")
    qs, qn, rs, rn, Q, N, LW = _retrieval_operands("hamming_ap_partial", q_planes, r_planes, bits, q_lab, r_lab)
    dev = qs.device
    total_counts = _counts_operand("hamming_ap_partial", "total_counts", total_counts, Q, bits, dev)
    prior_counts = _counts_operand("hamming_ap_partial", "prior_counts", prior_counts, Q, bits, dev)
    ap_sum = torch.empty(Q, dtype=torch.float64, device=dev)
    counts = torch.empty(Q, 2 * int(bits) + 1, 2, dtype=torch.int32, device=dev) if want_counts else None
    ws = workspace(lib().cmh_map_count_workspace_bytes(Q, N, int(bits)), dev, "retrieval")
    check(lib().cmh_hamming_ap_partial(ptr(qs), ptr(qn), ptr(q_lab), ptr(rs), ptr(rn), ptr(r_lab), Q, N, int(bits), 32 * LW,
                                       0 if topk is None else int(topk), ptr(total_counts), ptr(prior_counts), ptr(counts),
                                       ptr(ap_sum), ptr(ws), ws.numel(), stream_ptr(dev)), "cmh_hamming_ap_partial")
    return (ap_sum, counts) if want_counts else ap_sum


def ap_finish(ap_sum, total_counts, bits, topk=None):
    """ap_sum float64 [Q] (hamming_ap_partial, added over the shards), total_counts int32 [Q, 2 * bits + 1, 2] of the whole database
    -> (map 0-dim f32, ap f32 [Q]): ap = ap_sum / min(k, R), 0 where R = 0; map = their mean as map_mean forms it."""
    require_gpu(ap_sum, total_counts)
    Q = ap_sum.numel()
    if ap_sum.dtype != torch.float64 or ap_sum.dim() != 1 or not ap_sum.is_contiguous() or Q < 1:
        raise NativeError("ap_finish: ap_sum is a contiguous float64 tensor [Q]")
    total_counts = _counts_operand("ap_finish", "total_counts", total_counts, Q, bits, ap_sum.device)
    if total_counts is None:
        raise NativeError("ap_finish: needs the histogram of the whole database")
    ap = torch.empty(Q, dtype=torch.float32, device=ap_sum.device)
    mp = torch.empty(1, dtype=torch.float32, device=ap_sum.device)
    check(lib().cmh_ap_finish(ptr(ap_sum), ptr(total_counts), Q, int(bits), 0 if topk is None else int(topk), ptr(ap), ptr(mp),
                              stream_ptr(ap_sum.device)), "cmh_ap_finish")
    return mp[0], ap


def hamming_topk(q_planes, r_planes, bits, k, q_lab=None, r_lab=None, want_counts=False):
    """The k nearest database items of every query, ordered by (distance, database index) = the first k columns of
    torch.sort(hamming_dist, stable=True).  -> (idx int32 [Q, k], dist f32 [Q, k], rel uint8 [Q, k] or None without labels)
    [+ counts as hamming_hist with want_counts]."""
    qs, qn, rs, rn, Q, N, LW = _retrieval_operands("hamming_topk", q_planes, r_planes, bits, q_lab, r_lab)
    dev = qs.device
    k = int(k)
    if not 1 <= k <= N:
        raise NativeError(f"hamming_topk: k={k} outside [1, N={N}]")
    idx = torch.empty(Q, k, dtype=torch.int32, device=dev)
    dist = torch.empty(Q, k, dtype=torch.float32, device=dev)
    rel = torch.empty(Q, k, dtype=torch.uint8, device=dev) if LW else None
    counts = torch.empty(Q, 2 * int(bits) + 1, 2, dtype=torch.int32, device=dev) if want_counts else None
    ws = workspace(lib().cmh_retrieval_workspace_bytes(Q, N, int(bits)), dev, "retrieval")
    check(lib().cmh_hamming_topk(ptr(qs), ptr(qn), ptr(q_lab), ptr(rs), ptr(rn), ptr(r_lab), Q, N, int(bits), 32 * LW, k,
                                 ptr(idx), ptr(dist), ptr(rel), ptr(counts), ptr(ws), ws.numel(), stream_ptr(dev)),
          "cmh_hamming_topk")
    return (idx, dist, rel, counts) if want_counts else (idx, dist, rel)


FEW_Q_MAX = 64               # include/cmh.h CMH_FEW_Q_MAX, CMH_FEW_K_MAX, CMH_FEW_BITS_MAX: the limits of cmh_hamming_topk_few
FEW_K_MAX = 4096
FEW_BITS_MAX = 128


def hamming_topk_few(q_planes, r_planes, bits, k):
    """hamming_topk for few queries against a database of any size up to 2^31 - 1 items in ONE native call (csrc/retrieval_few.hip:
    lanes own items): -> (idx int32 [Q, k], dist f32 [Q, k]), row q = the first k columns of torch.sort(hamming_dist[q], stable=True).
    1 <= Q <= FEW_Q_MAX, bits <= FEW_BITS_MAX, 1 <= k <= min(N, FEW_K_MAX); no labels (gather the k results' label words)."""
    qs, qn, rs, rn, Q, N, _ = _retrieval_operands("hamming_topk_few", q_planes, r_planes, bits, None, None)
    dev = qs.device
    k = int(k)
    if not 1 <= k <= FEW_K_MAX:                                     # (before anything of Q x k entries is allocated)
        raise NativeError(f"hamming_topk_few: k={k} outside [1, {FEW_K_MAX}]")
    if k > N:
        raise NativeError(f"hamming_topk_few: k={k} exceeds N={N}")
    idx = torch.empty(Q, k, dtype=torch.int32, device=dev)
    dist = torch.empty(Q, k, dtype=torch.float32, device=dev)
    need = lib().cmh_topk_few_workspace_bytes(Q, N, int(bits))      # 0 outside the limits: the call below refuses with the reason
    ws = workspace(need, dev, "retrieval_few")
    check(lib().cmh_hamming_topk_few(ptr(qs), ptr(qn), ptr(rs), ptr(rn), Q, N, int(bits), k, ptr(idx), ptr(dist),
                                     ptr(ws), ws.numel(), stream_ptr(dev)), "cmh_hamming_topk_few")
    return idx, dist


SOFT_LEVELS = 15             # include/cmh.h CMH_SOFT_LEVELS: a soft query's weights are integers in [-15, 15]
SOFT_Q_MAX = 64              # ... CMH_SOFT_Q_MAX, CMH_SOFT_K_MAX, CMH_SOFT_BITS_MAX: the limits of cmh_soft_topk
SOFT_K_MAX = 4096
SOFT_BITS_MAX = 128
SOFT_ROWS_MAX = 65535        # rows of one cmh_soft_query_planes


def soft_query_planes(u):
    """The head's real-valued output u f32 [Q, bits] (any Q, bits <= SOFT_BITS_MAX) -> (q_sign int32 [Q, W], q_mag int32 [Q, 4, W],
    wsum int32 [Q], scale f32 [Q]): per row s = max |u_i| and the weights w_i = rint((u_i / s) * 15) in [-15, 15] (all 0 when s == 0)
    as a sign plane (bit set: w_i > 0) and the four bit planes of |w_i|; wsum = sum |w_i|, scale = s.  A non-finite entry raises
    (one host sync reads the flag back)."""
    u = f32c(u)
    require_gpu(u)
    if u.dim() != 2 or u.shape[0] < 1:
        raise NativeError(f"soft_query_planes: u of shape {tuple(u.shape)}, expected [Q >= 1, bits]")
    Q, bits = u.shape
    if not 1 <= bits <= SOFT_BITS_MAX:
        raise NativeError(f"soft_query_planes: bits={bits} outside [1, {SOFT_BITS_MAX}]")
    dev, W = u.device, (bits + 31) // 32
    q_sign = torch.empty(Q, W, dtype=torch.int32, device=dev)
    q_mag = torch.empty(Q, 4, W, dtype=torch.int32, device=dev)
    wsum = torch.empty(Q, dtype=torch.int32, device=dev)
    scale = torch.empty(Q, dtype=torch.float32, device=dev)
    bad = torch.zeros(1, dtype=torch.int32, device=dev)
    for a in range(0, Q, SOFT_ROWS_MAX):
        b = min(Q, a + SOFT_ROWS_MAX)
        check(lib().cmh_soft_query_planes(ptr(u[a:b]), b - a, bits, ptr(q_sign[a:b]), ptr(q_mag[a:b]), ptr(wsum[a:b]), ptr(scale[a:b]),
                                          ptr(bad), stream_ptr(dev)), "cmh_soft_query_planes")
    if int(bad.item()):
        raise NativeError("soft_query_planes: a soft query must be finite (NaN or Inf in the head's output)")
    return q_sign, q_mag, wsum, scale


def soft_topk(q, r_planes, bits, k):
    """The first k database items of every soft query in ascending (wdist, database index), one native call over a database of
    any size up to 2^31 - 1 items (csrc/retrieval_soft.hip): q = (q_sign, q_mag[, wsum, scale]) of soft_query_planes, r_planes =
    pack_codes' -> (idx int32 [Q, k], wdist int32 [Q, k]), wdist = sum |w_i| - sum w_i r_i.  1 <= Q <= SOFT_Q_MAX, bits <=
    SOFT_BITS_MAX, 1 <= k <= min(N, SOFT_K_MAX)."""
    (qs, qm), (rs, rn) = q[:2], r_planes
    require_gpu(qs, qm, rs, rn)
    Q, N = qs.shape[0], rs.shape[0]
    W = (int(bits) + 31) // 32
    fit("soft_topk", (qs, (Q, W)), (qm, (Q, 4, W)), (rs, (N, W)), (rn, (N, W)))
    for t in (qs, qm, rs, rn):
        if t.dtype != torch.int32 or not t.is_contiguous():
            raise NativeError("soft_topk: packed operands are contiguous int32 tensors (soft_query_planes / pack_codes)")
    dev = qs.device
    k = int(k)
    if not 1 <= k <= SOFT_K_MAX:                                    # (before anything of Q x k entries is allocated)
        raise NativeError(f"soft_topk: k={k} outside [1, {SOFT_K_MAX}]")
    if k > N:
        raise NativeError(f"soft_topk: k={k} exceeds N={N}")
    idx = torch.empty(Q, k, dtype=torch.int32, device=dev)
    wdist = torch.empty(Q, k, dtype=torch.int32, device=dev)
    need = lib().cmh_soft_topk_workspace_bytes(Q, N, int(bits))     # 0 outside the limits: the call below refuses with the reason
    ws = workspace(need, dev, "retrieval_soft")
    check(lib().cmh_soft_topk(ptr(qs), ptr(qm), ptr(rs), ptr(rn), Q, N, int(bits), k, ptr(idx), ptr(wdist), ptr(ws), ws.numel(),
                              stream_ptr(dev)), "cmh_soft_topk")
    return idx, wdist


def soft_ap(q, r_planes, bits, q_lab, r_lab, k=None):
    """AP, relevant count and rank sum of every soft query over the WHOLE database by counting (cmh_soft_ap, csrc/retrieval_soft.hip):
    no ranking, any database up to 2^31 - 1 items in one call.  q = (q_sign, q_mag[, ...]) of soft_query_planes, r_planes = pack_codes',
    q_lab / r_lab = pack_labels' -> (ap f32 [Q], relevant int32 [Q], rank_sum int64 [Q]): ap over the first k (None: all) items in
    ascending (wdist, database index), 0 without a relevant item; rank_sum = the sum of the ranks of ALL relevant items.
    1 <= Q <= SOFT_Q_MAX, bits <= SOFT_BITS_MAX, 1 <= k <= N."""
    if q_lab is None or r_lab is None:
        raise NativeError("soft_ap: needs the labels of both sides")
    (qs, qm), (rs, rn) = q[:2], r_planes
    require_gpu(qs, qm, rs, rn, q_lab, r_lab)
    Q, N = qs.shape[0], rs.shape[0]
    W, LW = (int(bits) + 31) // 32, q_lab.shape[-1]
    fit("soft_ap", (qs, (Q, W)), (qm, (Q, 4, W)), (rs, (N, W)), (rn, (N, W)), (q_lab, (Q, LW)), (r_lab, (N, LW)))
    for t in (qs, qm, rs, rn, q_lab, r_lab):
        if t.dtype != torch.int32 or not t.is_contiguous():
            raise NativeError("soft_ap: packed operands are contiguous int32 tensors (soft_query_planes / pack_codes / pack_labels)")
    if k is not None and not 1 <= int(k) <= N:
        raise NativeError(f"soft_ap: k={k} outside [1, N={N}]")
    dev = qs.device
    ap = torch.empty(Q, dtype=torch.float32, device=dev)
    relevant = torch.empty(Q, dtype=torch.int32, device=dev)
    rank_sum = torch.empty(Q, dtype=torch.int64, device=dev)
    need = lib().cmh_soft_ap_workspace_bytes(Q, N, int(bits), LW)    # 0 outside the limits: the call below refuses with the reason
    ws = workspace(need, dev, "retrieval_soft_ap")
    check(lib().cmh_soft_ap(ptr(qs), ptr(qm), ptr(rs), ptr(rn), ptr(q_lab), ptr(r_lab), LW, Q, N, int(bits), 0 if k is None else int(k),
                            ptr(ap), ptr(relevant), ptr(rank_sum), ptr(ws), ws.numel(), stream_ptr(dev)), "cmh_soft_ap")
    return ap, relevant, rank_sum


MASK_ANY, MASK_ALL, MASK_NONE = 0, 1, 2     # include/cmh.h CMH_MASK_*: the modes of cmh_mask_from_labels


def mask_words(n):
    """Words of an allow-mask over n items: int64 [ceil(n / 64)], bit j % 64 of word j / 64 = item j is admitted."""
    return (int(n) + 63) // 64


def _mask_operand(what, allow, N):
    require_gpu(allow)
    if allow.dtype != torch.int64 or allow.dim() != 1 or not allow.is_contiguous() or allow.numel() != mask_words(N):
        raise NativeError(f"{what}: the allow-mask is a contiguous int64 tensor [{mask_words(N)}] for {N} items, "
                          f"not {allow.dtype} {tuple(allow.shape)}")
    return allow


def hamming_topk_few_masked(q_planes, r_planes, allow, bits, k):
    """hamming_topk_few over only the items the allow-mask admits (int64 [ceil(N / 64)] on the GPU): -> (idx int32 [Q, k], dist f32
    [Q, k], found int32 [Q]).  Row q holds the first found[q] = min(k, admitted) admitted items in ascending (distance, DATABASE
    index); the columns behind hold idx = -1, dist = +inf.  k is checked against N; nothing synchronises."""
    qs, qn, rs, rn, Q, N, _ = _retrieval_operands("hamming_topk_few_masked", q_planes, r_planes, bits, None, None)
    allow = _mask_operand("hamming_topk_few_masked", allow, N)
    dev = qs.device
    k = int(k)
    if not 1 <= k <= FEW_K_MAX:
        raise NativeError(f"hamming_topk_few_masked: k={k} outside [1, {FEW_K_MAX}]")
    if k > N:
        raise NativeError(f"hamming_topk_few_masked: k={k} exceeds N={N}")
    idx = torch.empty(Q, k, dtype=torch.int32, device=dev)
    dist = torch.empty(Q, k, dtype=torch.float32, device=dev)
    found = torch.empty(Q, dtype=torch.int32, device=dev)
    need = lib().cmh_topk_few_masked_workspace_bytes(Q, N, int(bits))
    ws = workspace(need, dev, "retrieval_few")
    check(lib().cmh_hamming_topk_few_masked(ptr(qs), ptr(qn), ptr(rs), ptr(rn), ptr(allow), Q, N, int(bits), k, ptr(idx), ptr(dist),
                                            ptr(found), ptr(ws), ws.numel(), stream_ptr(dev)), "cmh_hamming_topk_few_masked")
    return idx, dist, found


def soft_topk_masked(q, r_planes, allow, bits, k):
    """soft_topk over only the items the allow-mask admits: -> (idx int32 [Q, k], wdist int32 [Q, k], found int32 [Q]); the columns
    at and behind found[q] hold idx = -1, wdist = 2^31 - 1."""
    (qs, qm), (rs, rn) = q[:2], r_planes
    require_gpu(qs, qm, rs, rn)
    Q, N = qs.shape[0], rs.shape[0]
    W = (int(bits) + 31) // 32
    fit("soft_topk_masked", (qs, (Q, W)), (qm, (Q, 4, W)), (rs, (N, W)), (rn, (N, W)))
    for t in (qs, qm, rs, rn):
        if t.dtype != torch.int32 or not t.is_contiguous():
            raise NativeError("soft_topk_masked: packed operands are contiguous int32 tensors (soft_query_planes / pack_codes)")
    allow = _mask_operand("soft_topk_masked", allow, N)
    dev = qs.device
    k = int(k)
    if not 1 <= k <= SOFT_K_MAX:
        raise NativeError(f"soft_topk_masked: k={k} outside [1, {SOFT_K_MAX}]")
    if k > N:
        raise NativeError(f"soft_topk_masked: k={k} exceeds N={N}")
    idx = torch.empty(Q, k, dtype=torch.int32, device=dev)
    wdist = torch.empty(Q, k, dtype=torch.int32, device=dev)
    found = torch.empty(Q, dtype=torch.int32, device=dev)
    need = lib().cmh_soft_topk_masked_workspace_bytes(Q, N, int(bits))
    ws = workspace(need, dev, "retrieval_soft")
    check(lib().cmh_soft_topk_masked(ptr(qs), ptr(qm), ptr(rs), ptr(rn), ptr(allow), Q, N, int(bits), k, ptr(idx), ptr(wdist),
                                     ptr(found), ptr(ws), ws.numel(), stream_ptr(dev)), "cmh_soft_topk_masked")
    return idx, wdist, found


def mask_from_labels(r_lab, need, mode, classes):
    """-> an allow-mask int64 [ceil(N / 64)] from packed labels r_lab int32 [N, LW] and the packed class set need int32 [LW]:
    MASK_ANY (label & need) != 0, MASK_ALL (label & need) == need, MASK_NONE (label & need) == 0; tail bits zero."""
    require_gpu(r_lab, need)
    N_, LW = r_lab.shape[0], (int(classes) + 31) // 32
    fit("mask_from_labels", (r_lab, (N_, LW)), (need, (LW,)))
    for t in (r_lab, need):
        if t.dtype != torch.int32 or not t.is_contiguous():
            raise NativeError("mask_from_labels: packed labels are contiguous int32 tensors (pack_labels)")
    allow = torch.empty(mask_words(N_), dtype=torch.int64, device=r_lab.device)
    check(lib().cmh_mask_from_labels(ptr(r_lab), ptr(need), int(mode), N_, int(classes), ptr(allow), stream_ptr(r_lab.device)),
          "cmh_mask_from_labels")
    return allow


def mask_from_ids(allow, ids, n, value):
    """Sets (value 1) or clears (value 0) the bits of the items `ids` (int32 [M] on the GPU, duplicates are legal) in the allow-mask
    over n items, in place.  An id outside [0, n) changes nothing and raises after the call (one host sync reads the flag back)."""
    allow = _mask_operand("mask_from_ids", allow, n)
    require_gpu(ids)
    if ids.dtype != torch.int32 or ids.dim() != 1 or not ids.is_contiguous():
        raise NativeError("mask_from_ids: ids is a contiguous int32 tensor [M]")
    bad = torch.zeros(1, dtype=torch.int32, device=allow.device)
    check(lib().cmh_mask_from_ids(ptr(ids), ids.numel(), int(n), int(value), ptr(allow), ptr(bad), stream_ptr(allow.device)),
          "cmh_mask_from_ids")
    if int(bad.item()):
        raise NativeError(f"mask_from_ids: an id outside [0, {int(n)})")
    return allow


GRAM_BITS_MAX = 256          # include/cmh.h CMH_GRAM_BITS_MAX, CMH_GRAM_CHUNK_MAX: the limits of cmh_code_gram
GRAM_CHUNK_MAX = 1 << 20     # the most items one workgroup of it owns: the unit its 32-bit partial sums are bounded over


def code_gram(a_planes, b_planes, abits, bbits, chunk_items=0):
    """The integers of the code diagnostics from two packed operands over the same N items (each a (sign, nz) pair of contiguous
    int32 planes [N, ceil(bits / 32)]; packed labels as (lab, lab), |code| as (nz, nz)) -> (gram int64 [abits, bbits], a_sum,
    a_abs int64 [abits], b_sum, b_abs int64 [bbits]); gram[i][j] = sum_n a_i(n) b_j(n), exact.  chunk_items: 0 = the plan's
    choice, else the items per workgroup (a multiple of 64 up to GRAM_CHUNK_MAX)."""
    (a_s, a_n), (b_s, b_n) = a_planes, b_planes
    require_gpu(a_s, a_n, b_s, b_n)
    n, abits, bbits = a_s.shape[0], int(abits), int(bbits)
    fit("code_gram", (a_s, (n, (abits + 31) // 32)), (a_n, (n, (abits + 31) // 32)), (b_s, (n, (bbits + 31) // 32)),
        (b_n, (n, (bbits + 31) // 32)))
    for t in (a_s, a_n, b_s, b_n):
        if t.dtype != torch.int32 or not t.is_contiguous():
            raise NativeError("code_gram: packed operands are contiguous int32 tensors (pack_codes / pack_labels)")
    dev = a_s.device
    gram = torch.empty(abits, bbits, dtype=torch.int64, device=dev)
    sums = [torch.empty(k, dtype=torch.int64, device=dev) for k in (abits, abits, bbits, bbits)]
    need = lib().cmh_code_gram_workspace_bytes(n, abits, bbits, int(chunk_items))      # 0 outside the limits: the call refuses with the reason
    ws = workspace(need, dev, "code_gram")
    check(lib().cmh_code_gram(ptr(a_s), ptr(a_n), ptr(b_s), ptr(b_n), n, abits, bbits, int(chunk_items), ptr(gram), *(ptr(t) for t in sums),
                              ptr(ws), ws.numel(), stream_ptr(dev)), "cmh_code_gram")
    return (gram, *sums)


SORT_TILE = 2048             # include/cmh.h CMH_SORT_TILE: sorted positions per workgroup of a pass of cmh_code_sort
BUCKET_BITS_MAX = 128        # ... CMH_BUCKET_BITS_MAX, CMH_BUCKET_RADIUS_MAX: the limits of cmh_bucket_probe_count / _fill
BUCKET_RADIUS_MAX = 2
SORT_BITS_MAX = 2048         # the longest code cmh_code_sort takes: pack_codes' limit


def _sign_plane(what, sign, bits):
    """A contiguous int32 sign plane [n, ceil(bits / 32)] on the GPU -> (n, bits)."""
    require_gpu(sign)
    bits = int(bits)
    if sign.dtype != torch.int32 or sign.dim() != 2 or not sign.is_contiguous():
        raise NativeError(f"{what}: the sign plane is a contiguous int32 tensor [n, words] (pack_codes)")
    if not 1 <= bits <= SORT_BITS_MAX:
        raise NativeError(f"{what}: bits={bits} outside [1, {SORT_BITS_MAX}]")
    fit(what, (sign, (sign.shape[0], (bits + 31) // 32)))
    return sign.shape[0], bits


def code_sort(sign, bits):
    """-> order int32 [n]: the item indices in ascending key order (a row's sign words cut to `bits` bits, word W - 1 most
    significant), equal keys by ascending index (stable)."""
    n, bits = _sign_plane("code_sort", sign, bits)
    dev = sign.device
    order = torch.empty(n, dtype=torch.int32, device=dev)
    ws = workspace(lib().cmh_code_sort_workspace_bytes(n, bits), dev, "code_sort")      # 0 outside the limits: the call refuses with the reason
    check(lib().cmh_code_sort(ptr(sign), n, bits, ptr(order), ptr(ws), ws.numel(), stream_ptr(dev)), "cmh_code_sort")
    return order


def code_buckets(sign, order, bits):
    """The groups of equal keys of a sorted plane -> (starts int32 [U + 1], codes int32 [U, W]): bucket b holds the items
    order[starts[b]:starts[b + 1]], all of key codes[b]; the buckets ascend by key.  U comes to the host: the one read."""
    n, bits = _sign_plane("code_buckets", sign, bits)
    dev = sign.device
    fit("code_buckets", (order, (n,)))
    if order.dtype != torch.int32 or not order.is_contiguous() or order.device != dev:
        raise NativeError("code_buckets: order is code_sort's contiguous int32 tensor [n] on the plane's device")
    head = torch.empty(n, dtype=torch.int32, device=dev)
    count = torch.empty(1, dtype=torch.int64, device=dev)
    ws = workspace(lib().cmh_code_sort_workspace_bytes(n, bits), dev, "code_sort")
    check(lib().cmh_code_bucket_count(ptr(sign), ptr(order), n, bits, ptr(head), ptr(count), ptr(ws), ws.numel(), stream_ptr(dev)),
          "cmh_code_bucket_count")
    U = int(count)
    starts = torch.empty(U + 1, dtype=torch.int32, device=dev)
    codes = torch.empty(U, sign.shape[1], dtype=torch.int32, device=dev)
    check(lib().cmh_code_bucket_fill(ptr(sign), ptr(order), ptr(head), n, bits, U, ptr(starts), ptr(codes), stream_ptr(dev)),
          "cmh_code_bucket_fill")
    return starts, codes


def _probe_operands(what, q_sign, codes, starts, bits, radius):
    require_gpu(q_sign, codes, starts)
    bits, radius = int(bits), int(radius)
    if not 1 <= bits <= BUCKET_BITS_MAX:
        raise NativeError(f"{what}: bits={bits} outside [1, BUCKET_BITS_MAX = {BUCKET_BITS_MAX}]")
    if not 0 <= radius <= BUCKET_RADIUS_MAX:
        raise NativeError(f"{what}: radius={radius} outside [0, BUCKET_RADIUS_MAX = {BUCKET_RADIUS_MAX}]")
    W = (bits + 31) // 32
    Q, U = q_sign.shape[0], codes.shape[0]
    if not 1 <= Q <= QUERIES_MAX:
        raise NativeError(f"{what}: Q={Q} outside [1, {QUERIES_MAX}] per call")
    fit(what, (q_sign, (Q, W)), (codes, (U, W)), (starts, (U + 1,)))
    for t in (q_sign, codes, starts):
        if t.dtype != torch.int32 or not t.is_contiguous() or t.device != q_sign.device:
            raise NativeError(f"{what}: query planes, codes and starts are contiguous int32 tensors on one device")
    return Q, U, bits, radius


def bucket_probe_count(q_sign, codes, starts, bits, radius):
    """-> (n_hit_buckets int32 [Q], n_hit_items int64 [Q]): of each query's probes (its key with at most `radius` bits flipped) the
    ones that are a bucket's key, and the items of those buckets."""
    Q, U, bits, radius = _probe_operands("bucket_probe_count", q_sign, codes, starts, bits, radius)
    dev = q_sign.device
    nb = torch.empty(Q, dtype=torch.int32, device=dev)
    ni = torch.empty(Q, dtype=torch.int64, device=dev)
    check(lib().cmh_bucket_probe_count(ptr(q_sign), Q, ptr(codes), ptr(starts), U, bits, radius, ptr(nb), ptr(ni), stream_ptr(dev)),
          "cmh_bucket_probe_count")
    return nb, ni


def bucket_probe_fill(q_sign, codes, starts, bits, radius, bucket_offsets, total):
    """bucket_offsets int64 [Q + 1] = the exclusive prefix sum of bucket_probe_count's n_hit_buckets, total = its last entry (>= 1)
    -> (hit_bucket int32 [total], hit_dist int32 [total]): query q's hits from bucket_offsets[q] on, in probe order."""
    Q, U, bits, radius = _probe_operands("bucket_probe_fill", q_sign, codes, starts, bits, radius)
    dev = q_sign.device
    total = int(total)
    if bucket_offsets.dtype != torch.int64 or tuple(bucket_offsets.shape) != (Q + 1,) or not bucket_offsets.is_contiguous() \
            or bucket_offsets.device != dev:
        raise NativeError("bucket_probe_fill: bucket_offsets is a contiguous int64 tensor [Q + 1] on the operands' device")
    hb = torch.empty(total, dtype=torch.int32, device=dev)
    hd = torch.empty(total, dtype=torch.int32, device=dev)
    check(lib().cmh_bucket_probe_fill(ptr(q_sign), Q, ptr(codes), ptr(starts), U, bits, radius, ptr(bucket_offsets), total, ptr(hb),
                                      ptr(hd), stream_ptr(dev)), "cmh_bucket_probe_fill")
    return hb, hd


MIH_SUB_BITS = 16            # include/cmh.h CMH_MIH_SUB_BITS, CMH_MIH_SUB_RADIUS_MAX: the substring width of cmh_mih_* and the
MIH_SUB_RADIUS_MAX = 2       # largest radius a substring is probed at (csrc/retrieval_mih.hip)
MIH_KEYS = 1 << MIH_SUB_BITS


def mih_substrings(bits):
    """m = ceil(bits / MIH_SUB_BITS): the substrings (tables) of a code."""
    return (int(bits) + MIH_SUB_BITS - 1) // MIH_SUB_BITS


def _mih_table(what, sign, bits):
    n, bits = _sign_plane(what, sign, bits)
    if bits > BUCKET_BITS_MAX:
        raise NativeError(f"{what}: bits={bits} outside [1, BUCKET_BITS_MAX = {BUCKET_BITS_MAX}]")
    return n, bits, mih_substrings(bits)


def mih_build(sign, bits):
    """-> (order int32 [m, n], starts int32 [m, 65537]), m = ceil(bits / 16): per 16-bit substring of the sign plane the item indices
    by ascending (key, index), and the first position of every key; bucket `key` of table j is order[j, starts[j, key]:starts[j, key + 1]]."""
    n, bits, m = _mih_table("mih_build", sign, bits)
    dev = sign.device
    order = torch.empty(m, n, dtype=torch.int32, device=dev)
    starts = torch.empty(m, MIH_KEYS + 1, dtype=torch.int32, device=dev)
    ws = workspace(lib().cmh_mih_build_workspace_bytes(n, bits), dev, "code_sort")
    check(lib().cmh_mih_build(ptr(sign), n, bits, ptr(order), ptr(starts), ptr(ws), ws.numel(), stream_ptr(dev)), "cmh_mih_build")
    return order, starts


def _mih_operands(what, q_sign, db_sign, bits, radius, order, starts, radius_name="radius"):
    require_gpu(q_sign, db_sign, order, starts)
    n, bits, m = _mih_table(what, db_sign, bits)
    radius = int(radius)
    if not 0 <= radius <= (MIH_SUB_RADIUS_MAX + 1) * m - 1:
        raise NativeError(f"{what}: {radius_name}={radius} outside [0, {(MIH_SUB_RADIUS_MAX + 1) * m - 1}] at {bits} bits")
    Q = q_sign.shape[0]
    if not 1 <= Q <= QUERIES_MAX:
        raise NativeError(f"{what}: Q={Q} outside [1, {QUERIES_MAX}] per call")
    fit(what, (q_sign, (Q, db_sign.shape[1])), (order, (m, n)), (starts, (m, MIH_KEYS + 1)))
    for t in (q_sign, order, starts):
        if t.dtype != torch.int32 or not t.is_contiguous() or t.device != db_sign.device:
            raise NativeError(f"{what}: query planes, order and starts are contiguous int32 tensors on the database's device")
    return Q, n, bits, radius


def mih_count(q_sign, db_sign, bits, radius, order, starts):
    """-> n_hits int32 [Q]: the database items within `radius` whole bits of each query, found through mih_build's tables."""
    Q, n, bits, radius = _mih_operands("mih_count", q_sign, db_sign, bits, radius, order, starts)
    dev = q_sign.device
    hits = torch.empty(Q, dtype=torch.int32, device=dev)
    check(lib().cmh_mih_count(ptr(q_sign), Q, ptr(db_sign), n, bits, radius, ptr(order), ptr(starts), ptr(hits), stream_ptr(dev)),
          "cmh_mih_count")
    return hits


def mih_fill(q_sign, db_sign, bits, radius, order, starts, offsets, total):
    """offsets int64 [Q + 1] = the exclusive prefix sum of mih_count's n_hits, total = its last entry (>= 1) -> (idx int32 [total],
    dist int32 [total]): query q's items from offsets[q] on, each once, in the order of the kernel's walk (the same on every call)."""
    Q, n, bits, radius = _mih_operands("mih_fill", q_sign, db_sign, bits, radius, order, starts)
    dev = q_sign.device
    total = int(total)
    if offsets.dtype != torch.int64 or tuple(offsets.shape) != (Q + 1,) or not offsets.is_contiguous() or offsets.device != dev:
        raise NativeError("mih_fill: offsets is a contiguous int64 tensor [Q + 1] on the operands' device")
    idx = torch.empty(total, dtype=torch.int32, device=dev)
    dist = torch.empty(total, dtype=torch.int32, device=dev)
    check(lib().cmh_mih_fill(ptr(q_sign), Q, ptr(db_sign), n, bits, radius, ptr(order), ptr(starts), ptr(offsets), total, ptr(idx),
                             ptr(dist), stream_ptr(dev)), "cmh_mih_fill")
    return idx, dist


def mih_knn_count(q_sign, db_sign, bits, k, r_cap, order, starts):
    """-> (radius, n_ball, n_less) int32 [Q]: per query the smallest radius r* <= r_cap whose ball holds at least k items, found by
    growing it through mih_build's tables, |ball(r*)| and |ball(r* - 1)|; radius = -1 and n_ball = n_less = |ball(r_cap)| where
    fewer than k items lie within r_cap."""
    Q, n, bits, r_cap = _mih_operands("mih_knn_count", q_sign, db_sign, bits, r_cap, order, starts, "r_cap")
    k = int(k)
    if not 1 <= k <= n:
        raise NativeError(f"mih_knn_count: k={k} outside [1, N={n}]")
    dev = q_sign.device
    radius, n_ball, n_less = (torch.empty(Q, dtype=torch.int32, device=dev) for _ in range(3))
    check(lib().cmh_mih_knn_count(ptr(q_sign), Q, ptr(db_sign), n, bits, k, r_cap, ptr(order), ptr(starts), ptr(radius), ptr(n_ball),
                                  ptr(n_less), stream_ptr(dev)), "cmh_mih_knn_count")
    return radius, n_ball, n_less


def mih_knn_fill(q_sign, db_sign, bits, radius, order, starts, offsets, total):
    """radius int32 [Q] (mih_knn_count's; a query with a radius below 0 is not walked), offsets int64 [Q + 1] = the exclusive prefix
    sum of the walked queries' n_ball (0 for the others), total = its last entry (>= 1) -> (idx int32 [total], dist int32 [total]):
    query q's ball from offsets[q] on, each item once, in the order of the kernel's walk (the same on every call)."""
    Q, n, bits, _ = _mih_operands("mih_knn_fill", q_sign, db_sign, bits, 0, order, starts)
    dev = q_sign.device
    total = int(total)
    if radius.dtype != torch.int32 or tuple(radius.shape) != (Q,) or not radius.is_contiguous() or radius.device != dev:
        raise NativeError("mih_knn_fill: radius is a contiguous int32 tensor [Q] on the operands' device")
    if offsets.dtype != torch.int64 or tuple(offsets.shape) != (Q + 1,) or not offsets.is_contiguous() or offsets.device != dev:
        raise NativeError("mih_knn_fill: offsets is a contiguous int64 tensor [Q + 1] on the operands' device")
    idx = torch.empty(total, dtype=torch.int32, device=dev)
    dist = torch.empty(total, dtype=torch.int32, device=dev)
    check(lib().cmh_mih_knn_fill(ptr(q_sign), Q, ptr(db_sign), n, bits, ptr(radius), ptr(order), ptr(starts), ptr(offsets), total,
                                 ptr(idx), ptr(dist), stream_ptr(dev)), "cmh_mih_knn_fill")
    return idx, dist


GRADE_CLASSES_MAX = 255     # a grade is one byte
TOPK_MAX = 524287            # include/cmh.h CMH_TOPK_MAX: the largest N (and k) of the four retrieval entry points
QUERIES_MAX = 65535          # ... and their largest Q


def _grade_classes(what, classes, LW):
    """The class count of the graded entry points: the caller's, or what the packed words can hold (at most 255: the kernel
    saturates a grade there, so the 256th bit of eight words cannot wrap it)."""
    classes = min(32 * LW, GRADE_CLASSES_MAX) if classes is None else int(classes)
    if classes < 1 or (classes + 31) // 32 != LW:
        raise NativeError(f"{what}: classes={classes} does not fit label operands of {LW} words")
    return classes


def hamming_topk_graded(q_planes, r_planes, bits, k, q_lab, r_lab, want_counts=False, classes=None):
    """hamming_topk with the NUMBER of shared labels where it has the hit flag: -> (idx int32 [Q, k], dist f32 [Q, k],
    grade uint8 [Q, k]) [+ counts as hamming_hist with want_counts].  idx and dist are hamming_topk's, grade > 0 is its rel.
    Labels are required, at most 255 classes (`classes`: the count behind pack_labels' words, 32 per word when None)."""
    if q_lab is None or r_lab is None:
        raise NativeError("hamming_topk_graded: needs the labels of both sides")
    qs, qn, rs, rn, Q, N, LW = _retrieval_operands("hamming_topk_graded", q_planes, r_planes, bits, q_lab, r_lab)
    dev = qs.device
    k = int(k)
    if not 1 <= k <= N:
        raise NativeError(f"hamming_topk_graded: k={k} outside [1, N={N}]")
    classes = _grade_classes("hamming_topk_graded", classes, LW)
    idx = torch.empty(Q, k, dtype=torch.int32, device=dev)
    dist = torch.empty(Q, k, dtype=torch.float32, device=dev)
    grade = torch.empty(Q, k, dtype=torch.uint8, device=dev)
    counts = torch.empty(Q, 2 * int(bits) + 1, 2, dtype=torch.int32, device=dev) if want_counts else None
    ws = workspace(lib().cmh_retrieval_workspace_bytes(Q, N, int(bits)), dev, "retrieval")
    check(lib().cmh_hamming_topk_graded(ptr(qs), ptr(qn), ptr(q_lab), ptr(rs), ptr(rn), ptr(r_lab), Q, N, int(bits), classes, k,
                                        ptr(idx), ptr(dist), None, ptr(grade), ptr(counts), ptr(ws), ws.numel(), stream_ptr(dev)),
          "cmh_hamming_topk_graded")
    return (idx, dist, grade, counts) if want_counts else (idx, dist, grade)


def hamming_range(q_planes, r_planes, bits, radius_h, q_lab=None, r_lab=None, total_counts=None, prior_counts=None, row_off=None,
                  idx_base=0, out=None, want_counts=False):
    """The fill pass of a radius search: every database item at half-distance h <= radius_h from query q goes into the flat buffers
    out = (idx int32 [T], dist f32 [T], rel uint8 [T] or None), at row_off[q] (int64 [Q]) + its place in the order (distance, database
    index); idx = idx_base + its row, dist = 0.5 * h.  The caller sizes the rows from hamming_hist: query q writes exactly
    [row_off[q], row_off[q] + ball(q)), ball(q) = the items of total_counts (None: of this database) in the bins 0..radius_h, and
    nothing else of `out`.  total_counts / prior_counts: the histograms of the whole database and of the shards before this one, as
    hamming_ap_partial takes them.  -> out [+ this database's counts with want_counts]."""
    qs, qn, rs, rn, Q, N, LW = _retrieval_operands("hamming_range", q_planes, r_planes, bits, q_lab, r_lab)
    dev = qs.device
    radius_h, idx_base = int(radius_h), int(idx_base)
    if not 0 <= radius_h <= 2 * int(bits):
        raise NativeError(f"hamming_range: radius_h={radius_h} outside [0, {2 * int(bits)}]")
    if not 0 <= idx_base <= 2 ** 31 - 1 - N:
        raise NativeError(f"hamming_range: idx_base={idx_base} outside [0, 2^31 - 1 - N]")
    total_counts = _counts_operand("hamming_range", "total_counts", total_counts, Q, bits, dev)
    prior_counts = _counts_operand("hamming_range", "prior_counts", prior_counts, Q, bits, dev)
    if row_off is None or row_off.dtype != torch.int64 or tuple(row_off.shape) != (Q,) or not row_off.is_contiguous() or row_off.device != dev:
        raise NativeError("hamming_range: row_off is a contiguous int64 tensor [Q] on the operands' device")
    if not isinstance(out, (tuple, list)) or len(out) != 3 or out[0] is None or out[1] is None:
        raise NativeError("hamming_range: out is an (idx, dist, rel or None) tuple of flat buffers")
    idx, dist, rel = out
    if rel is not None and not LW:
        raise NativeError("hamming_range: hit flags asked for without labels")
    for t, dt in ((idx, torch.int32), (dist, torch.float32), (rel, torch.uint8)):
        if t is not None and (t.dtype != dt or t.dim() != 1 or not t.is_contiguous() or t.device != dev or t.numel() != idx.numel()):
            raise NativeError("hamming_range: out holds contiguous flat int32 idx, float32 dist and uint8 rel buffers of one length "
                              "on the operands' device")
    counts = torch.empty(Q, 2 * int(bits) + 1, 2, dtype=torch.int32, device=dev) if want_counts else None
    ws = workspace(lib().cmh_range_workspace_bytes(Q, N, int(bits)), dev, "retrieval")
    check(lib().cmh_hamming_range(ptr(qs), ptr(qn), ptr(q_lab), ptr(rs), ptr(rn), ptr(r_lab), Q, N, int(bits), 32 * LW, radius_h,
                                  ptr(total_counts), ptr(prior_counts), ptr(row_off), idx_base, ptr(idx), ptr(dist), ptr(rel),
                                  ptr(counts), ptr(ws), ws.numel(), stream_ptr(dev)), "cmh_hamming_range")
    return ((idx, dist, rel), counts) if want_counts else (idx, dist, rel)


RANK_TARGETS_MAX = 8         # target slots per query of one cmh_hamming_rank


def hamming_rank(q_planes, r_planes, bits, t_planes, bound):
    """The three counts behind the rank of given targets, by one walk over the database (no list, no sort):
    -> int32 [Q, G, 3] = (less, ties_before, ties).  t_planes: the packed planes of the targets, a pair of int32 [Q, G, W] (or
    [Q * G, W]) tensors; bound int32 [Q, G] (or [Q * G]), 1 <= G <= 8: database items with index < bound count as before the target
    among its ties (the target's own row in this database; clamp(t - a, 0, b - a) for the shard [a, b) of a larger one), -1 = the
    slot has no target and gives three zeros.  less + ties_before is the target's column in hamming_topk's row; the counts of the
    shards of a database add."""
    qs, qn, rs, rn, Q, N, _ = _retrieval_operands("hamming_rank", q_planes, r_planes, bits, None, None)
    ts, tn = t_planes
    require_gpu(ts, tn, bound)
    dev, W = qs.device, (int(bits) + 31) // 32
    if Q < 1 or bound.dim() not in (1, 2) or bound.numel() % Q:
        raise NativeError(f"hamming_rank: bound of shape {tuple(bound.shape)} for {Q} queries")
    G = bound.numel() // Q
    if not 1 <= G <= RANK_TARGETS_MAX:
        raise NativeError(f"hamming_rank: G={G} targets per query outside [1, {RANK_TARGETS_MAX}]")
    if bound.dim() == 2:
        fit("hamming_rank", (bound, (Q, G)))
    for t in (ts, tn):
        fit("hamming_rank", (t, (Q, G, W) if t.dim() == 3 else (Q * G, W)))
    for t in (ts, tn, bound):
        if t.dtype != torch.int32 or not t.is_contiguous() or t.device != dev:
            raise NativeError("hamming_rank: target planes and bound are contiguous int32 tensors on the operands' device")
    out = torch.empty(Q, G, 3, dtype=torch.int32, device=dev)
    ws = workspace(lib().cmh_rank_workspace_bytes(Q, N, int(bits), G), dev, "retrieval")
    check(lib().cmh_hamming_rank(ptr(qs), ptr(qn), ptr(rs), ptr(rn), Q, N, int(bits), ptr(ts), ptr(tn), ptr(bound), G, ptr(out),
                                 ptr(ws), ws.numel(), stream_ptr(dev)), "cmh_hamming_rank")
    return out


def label_overlap_hist(q_lab, r_lab, classes):
    """-> int32 [Q, classes+1]: entry [q, g] = database items that share exactly g labels with query q (packed labels of
    pack_labels, at most 255 classes).  Every row sums to N; N - [:, 0] = the query's relevant items."""
    if q_lab is None or r_lab is None:
        raise NativeError("label_overlap_hist: needs the labels of both sides")
    require_gpu(q_lab, r_lab)
    classes = int(classes)
    Q, N, LW = q_lab.shape[0], r_lab.shape[0], (classes + 31) // 32
    fit("label_overlap_hist", (q_lab, (Q, LW)), (r_lab, (N, LW)))
    for t in (q_lab, r_lab):
        if t.dtype != torch.int32 or not t.is_contiguous():
            raise NativeError("label_overlap_hist: packed operands are contiguous int32 tensors (pack_labels)")
    dev = q_lab.device
    out = torch.empty(Q, classes + 1, dtype=torch.int32, device=dev)
    ws = workspace(lib().cmh_label_overlap_workspace_bytes(Q, N, classes), dev, "retrieval")
    check(lib().cmh_label_overlap_hist(ptr(q_lab), ptr(r_lab), Q, N, classes, ptr(out), ptr(ws), ws.numel(), stream_ptr(dev)),
          "cmh_label_overlap_hist")
    return out


def _topk_list(what, name, lst, Q=None):
    if not isinstance(lst, (tuple, list)) or len(lst) != 3:
        raise NativeError(f"{what}: {name} is an (idx, dist, tag or None) tuple")
    idx, dist, tag = lst
    if idx is None or dist is None or idx.dim() != 2:
        raise NativeError(f"{what}: {name} needs idx and dist of shape [Q, k]")
    require_gpu(idx, dist, tag)
    rows, width = idx.shape
    fit(what, (idx, (rows if Q is None else Q, width)), (dist, (idx.shape[0], width)), (tag, (idx.shape[0], width)))
    for t, dt in ((idx, torch.int32), (dist, torch.float32), (tag, torch.uint8)):
        if t is not None and (t.dtype != dt or not t.is_contiguous()):
            raise NativeError(f"{what}: {name} holds contiguous int32 idx, float32 dist and uint8 tag tensors")
    return idx, dist, tag, rows, width


def topk_merge(a, b, b_base, k, out=None):
    """Two top-k lists of the same queries, a = (idx int32 [Q, ka], dist f32 [Q, ka], tag uint8 [Q, ka] or None) and b likewise
    with its own width kb -> (idx int32 [Q, k], dist f32 [Q, k], tag uint8 [Q, k] or None): the first k entries of their union in
    the order of hamming_topk.  Rows are ascending by (dist, idx); b's indices are local to a shard that starts at item b_base,
    behind every item of a, and come out as idx + b_base.  tag = the hit flags or the grades that travel with the entries: on both
    lists or on neither.  1 <= k <= ka + kb.  out: (idx, dist, tag) of the output's shape to write into in place of
    fresh ones (what lets a fold over many shards reuse two buffers); their bytes overlap neither a's nor b's nor each other's."""
    a_idx, a_dist, a_tag, Q, ka = _topk_list("topk_merge", "a", a)
    b_idx, b_dist, b_tag, _, kb = _topk_list("topk_merge", "b", b, Q)
    if (a_tag is None) != (b_tag is None):
        raise NativeError("topk_merge: tags on one list only")
    k, b_base = int(k), int(b_base)
    if Q < 1 or ka < 1 or kb < 1 or not 1 <= k <= ka + kb:
        raise NativeError(f"topk_merge: k={k} outside [1, ka + kb = {ka + kb}] (Q={Q}, ka={ka}, kb={kb})")
    if not 0 <= b_base <= 2 ** 31 - 1 - kb:
        raise NativeError(f"topk_merge: b_base={b_base} outside [0, 2^31 - 1 - kb]")
    dev = a_idx.device
    if out is None:
        idx = torch.empty(Q, k, dtype=torch.int32, device=dev)
        dist = torch.empty(Q, k, dtype=torch.float32, device=dev)
        tag = torch.empty(Q, k, dtype=torch.uint8, device=dev) if a_tag is not None else None
    else:
        idx, dist, tag, _, _ = _topk_list("topk_merge", "out", out, Q)
        fit("topk_merge", (idx, (Q, k)))
        if (tag is None) != (a_tag is None):
            raise NativeError("topk_merge: out carries tags exactly when the lists do")
        span = lambda t: (t.data_ptr(), t.data_ptr() + t.numel() * t.element_size())      # contiguous: the bytes it covers
        ins = [span(t) for t in (a_idx, a_dist, a_tag, b_idx, b_dist, b_tag) if t is not None]
        outs = [span(t) for t in (idx, dist, tag) if t is not None]
        if any(o[0] < i[1] and i[0] < o[1] for o in outs for i in ins) or any(
                outs[x][0] < outs[y][1] and outs[y][0] < outs[x][1] for x in range(len(outs)) for y in range(x)):
            raise NativeError("topk_merge: out must not overlap a, b or itself")
    check(lib().cmh_topk_merge(ptr(a_idx), ptr(a_dist), ptr(a_tag), ka, ptr(b_idx), ptr(b_dist), ptr(b_tag), kb, b_base, Q, k,
                               ptr(idx), ptr(dist), ptr(tag), stream_ptr(dev)), "cmh_topk_merge")
    return idx, dist, tag


# ------------------------------------------------------------------------------------------ losses
def fit(what, *pairs):
    """pairs of (tensor, expected shape): the kernels take their sizes from ONE operand, so every other operand is checked here
    (a mismatched operand would be read out of bounds)."""
    for t, shape in pairs:
        if t is not None and tuple(t.shape) != tuple(shape):
            raise NativeError(f"{what}: operand of shape {tuple(t.shape)} where {tuple(shape)} is expected")


def dsph_hyp_loss(x, y, label, proxies, threshold, alpha):
    x, y, label, proxies = f32c(x), f32c(y), f32c(label), f32c(proxies)
    require_gpu(x, y, label, proxies)
    B, K = x.shape
    Cn = label.shape[1]
    fit("dsph_hyp_loss", (y, (B, K)), (label, (B, Cn)), (proxies, (Cn, K)))
    out = torch.empty(1, dtype=torch.float32, device=x.device)
    ws = workspace(lib().cmh_loss_workspace_bytes(B, K, Cn), x.device, "loss")
    check(lib().cmh_dsph_hyp_loss(ptr(x), ptr(y), ptr(label), ptr(proxies), B, K, Cn, float(threshold), float(alpha),
                                  ptr(out), ptr(ws), ws.numel(), stream_ptr(x.device)), "cmh_dsph_hyp_loss")
    return out[0]


def msl_loss(feats, labels, feat2=None):
    """DMsH-LN multi-similarity loss (train/DMsH_LN/MSLOSS.py:13-55) -> loss 0-dim"""
    feats, labels = f32c(feats), f32c(labels)
    feat2 = None if feat2 is None else f32c(feat2)
    require_gpu(feats, labels, feat2)
    B, K = feats.shape
    fit("msl_loss", (labels, (B, labels.shape[1])))
    if feat2 is not None:
        fit("msl_loss", (feat2, (B, K)))
    out = torch.empty(1, dtype=torch.float32, device=feats.device)
    ws = workspace(lib().cmh_msl_workspace_bytes(B), feats.device, "loss")
    check(lib().cmh_msl_loss(ptr(feats), ptr(feat2), ptr(labels), B, K, labels.shape[1], ptr(out), ptr(ws), ws.numel(),
                             stream_ptr(feats.device)), "cmh_msl_loss")
    return out[0]


def msl_loss_backward(feats, labels, feat2, dloss):
    """-> (dfeats, dfeat2 | None); with feat2 = None the gradients of both roles of feats are summed into dfeats"""
    B, K = feats.shape
    dfeats = torch.empty_like(feats)
    dfeat2 = None if feat2 is None else torch.empty_like(feat2)
    ws = workspace(lib().cmh_msl_workspace_bytes(B), feats.device, "loss")
    check(lib().cmh_msl_loss_backward(ptr(feats), ptr(feat2), ptr(labels), B, K, labels.shape[1], ptr(f32c(dloss).reshape(1)),
                                      ptr(dfeats), ptr(dfeat2), ptr(ws), ws.numel(), stream_ptr(feats.device)), "cmh_msl_loss_backward")
    return dfeats, dfeat2


def spl_loss(a, b, labels, temperature, delta):
    """DHaPH self-paced contrastive loss (train/DHaPH/MSLoss.py:13-33); b = None: a against itself -> loss 0-dim"""
    a, labels = f32c(a), f32c(labels)
    b = None if b is None else f32c(b)
    require_gpu(a, labels, b)
    B, K = a.shape
    fit("spl_loss", (labels, (B, labels.shape[1])), (b, (B, K)))
    out = torch.empty(1, dtype=torch.float32, device=a.device)
    ws = workspace(lib().cmh_spl_workspace_bytes(B), a.device, "loss")
    check(lib().cmh_spl_loss(ptr(a), ptr(b), ptr(labels), B, K, labels.shape[1], float(temperature), float(delta), ptr(out), ptr(ws),
                             ws.numel(), stream_ptr(a.device)), "cmh_spl_loss")
    return out[0]


def spl_loss_backward(a, b, labels, temperature, delta, dloss):
    """-> (da, db | None); with b = None the gradients of both roles of a are summed into da"""
    B, K = a.shape
    da = torch.empty_like(a)
    db = None if b is None else torch.empty_like(b)
    ws = workspace(lib().cmh_spl_workspace_bytes(B), a.device, "loss")
    check(lib().cmh_spl_loss_backward(ptr(a), ptr(b), ptr(labels), B, K, labels.shape[1], float(temperature), float(delta),
                                      ptr(f32c(dloss).reshape(1)), ptr(da), ptr(db), ptr(ws), ws.numel(), stream_ptr(a.device)),
          "cmh_spl_loss_backward")
    return da, db


def qmi_loss(img, txt, label, eps=1e-8):
    """DNpH qmi_loss (train/DNpH_TMM/loss.py:5-72, defaults) -> (loss 0-dim, sum_d [1] for the backward, packed labels)"""
    img, txt, label = f32c(img), f32c(txt), f32c(label)
    require_gpu(img, txt, label)
    B, K = img.shape
    Cn = label.shape[1]
    fit("qmi_loss", (txt, (B, K)), (label, (B, Cn)))
    packed = pack_labels(label)
    out = torch.empty(1, dtype=torch.float32, device=img.device)
    sum_d = torch.empty(1, dtype=torch.float32, device=img.device)
    ws = workspace(lib().cmh_qmi_workspace_bytes(B), img.device, "loss")
    check(lib().cmh_qmi_loss(ptr(img), ptr(txt), ptr(packed), B, K, Cn, float(eps), ptr(out), ptr(sum_d), ptr(ws), ws.numel(),
                             stream_ptr(img.device)), "cmh_qmi_loss")
    return out[0], sum_d, packed


def qmi_loss_backward(img, txt, packed, classes, sum_d, dloss, eps=1e-8):
    B, K = img.shape
    dimg, dtxt = torch.empty_like(img), torch.empty_like(txt)
    ws = workspace(lib().cmh_qmi_workspace_bytes(B), img.device, "loss")
    check(lib().cmh_qmi_loss_backward(ptr(img), ptr(txt), ptr(packed), B, K, int(classes), float(eps), ptr(sum_d), ptr(f32c(dloss).reshape(1)),
                                      ptr(dimg), ptr(dtxt), ptr(ws), ws.numel(), stream_ptr(img.device)), "cmh_qmi_loss_backward")
    return dimg, dtxt


def _ptr_array(tensors):
    """a host array of device pointers (the `const float* const*` operands of the DDBH entry points)"""
    return (C.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])


def _ddbh_operands(what, pairs, label):
    made = {}                                                   # one f32 contiguous copy per distinct operand: `v is u` stays so
    pairs = [tuple(made.setdefault(id(t), f32c(t)) for t in pr) for pr in pairs]
    label = f32c(label)
    require_gpu(label, *[t for pr in pairs for t in pr])
    if pairs[0][0].dim() != 2 or label.dim() != 2:
        raise NativeError(f"{what}: codes [B, K] and labels [B, C] are expected")
    B, K = pairs[0][0].shape
    fit(what, (label, (B, label.shape[1])), *[(t, (B, K)) for pr in pairs for t in pr])
    return pairs, label, B, K, label.shape[1]


def ddbh_bp_loss(pairs, label, scalars):
    """DDBH BPLoss.forward (train/DDBH/loss.py:15-78) for up to four (u, v) pairs over one label matrix in one launch; scalars =
    (y_p, right, left, lowerBound, upperBound, percent) -> (loss [n], rows and count for the backward, the operands as passed)"""
    pairs, label, B, K, Cn = _ddbh_operands("ddbh_bp_loss", pairs, label)
    n, dev = len(pairs), label.device
    loss = torch.empty(n, dtype=torch.float32, device=dev)
    rows = torch.empty(n, B, 8, dtype=torch.int32, device=dev)
    count = torch.empty(n, dtype=torch.int32, device=dev)
    ws = workspace(lib().cmh_ddbh_workspace_bytes(B), dev, "loss")
    check(lib().cmh_ddbh_bp_loss(_ptr_array([u for u, _ in pairs]), _ptr_array([v for _, v in pairs]), n, ptr(label), B, K, Cn,
                                 *[float(s) for s in scalars], ptr(loss), ptr(rows), ptr(count), ptr(ws), ws.numel(), stream_ptr(dev)),
          "cmh_ddbh_bp_loss")
    return loss, rows, count, pairs, label


def ddbh_bp_loss_backward(pairs, label, scalars, rows, count, dloss):
    """-> [(du, dv)] per pair, each f32 [B, K] (two buffers even where u is v)"""
    B, K = pairs[0][0].shape
    n = len(pairs)
    du = [torch.empty_like(u) for u, _ in pairs]
    dv = [torch.empty_like(v) for _, v in pairs]
    dloss = f32c(dloss).reshape(n)
    check(lib().cmh_ddbh_bp_loss_backward(_ptr_array([u for u, _ in pairs]), _ptr_array([v for _, v in pairs]), n, ptr(label), B, K,
                                          label.shape[1], *[float(s) for s in scalars], ptr(rows), ptr(count), ptr(dloss),
                                          _ptr_array(du), _ptr_array(dv), stream_ptr(label.device)), "cmh_ddbh_bp_loss_backward")
    return list(zip(du, dv))


def ddbh_quant_loss(hs, label):
    """DDBH's quantisation term mean(s @ (h - sign h)^2) (train/DDBH/hash_train.py:64-76) of up to four matrices over one label
    matrix -> (loss [n], colsum [B] for the backward, the operands as passed)"""
    pairs, label, B, K, Cn = _ddbh_operands("ddbh_quant_loss", [(h, h) for h in hs], label)
    hs = [h for h, _ in pairs]
    n, dev = len(hs), label.device
    loss = torch.empty(n, dtype=torch.float32, device=dev)
    colsum = torch.empty(B, dtype=torch.float32, device=dev)
    ws = workspace(lib().cmh_ddbh_workspace_bytes(B), dev, "loss")
    check(lib().cmh_ddbh_quant_loss(_ptr_array(hs), n, ptr(label), B, K, Cn, ptr(loss), ptr(colsum), ptr(ws), ws.numel(), stream_ptr(dev)),
          "cmh_ddbh_quant_loss")
    return loss, colsum, hs


def ddbh_quant_loss_backward(hs, colsum, dloss):
    B, K = hs[0].shape
    dh = [torch.empty_like(h) for h in hs]
    dloss = f32c(dloss).reshape(len(hs))
    check(lib().cmh_ddbh_quant_loss_backward(_ptr_array(hs), len(hs), ptr(colsum), B, K, ptr(dloss), _ptr_array(dh), stream_ptr(colsum.device)),
          "cmh_ddbh_quant_loss_backward")
    return dh


MSC_MAX_B, MSC_MAX_K = 1024, 128                            # csrc/msc.hip's limits, for the wrapper's message
MSC_MINING = {"all": 0, "semi-hard": 1}                      # the two rules of the reference (train/DPSIH/Loss.py:118-120)


def msc_triplet_loss(pairs, label, margin, mining="all", normalize=False):
    """Multi_Semantic_Correlation_Loss.forward (train/DPSIH/Loss.py:85-137) for up to four (u, v) pairs over one label matrix in one
    call -> (loss f32 [n], count i64 [n], sim f32 [n, B, B], saved = what msc_triplet_loss_backward takes)"""
    if mining not in MSC_MINING:
        raise NativeError(f"msc_triplet_loss: mining {mining!r}: one of {sorted(MSC_MINING)}")
    pairs, label, B, K, Cn = _ddbh_operands("msc_triplet_loss", pairs, label)
    if not (1 <= B <= MSC_MAX_B and 1 <= K <= MSC_MAX_K):
        raise NativeError(f"msc_triplet_loss: B={B} K={K}: 1 <= B <= {MSC_MAX_B} and 1 <= K <= {MSC_MAX_K} are built")
    n, dev = len(pairs), label.device
    loss = torch.empty(n, dtype=torch.float32, device=dev)
    count = torch.empty(n, dtype=torch.int64, device=dev)
    sim = torch.empty(n, B, B, dtype=torch.float32, device=dev)
    coef = torch.empty(n, B, B, dtype=torch.int32, device=dev)
    unit = torch.empty(2 * n, B, K, dtype=torch.float32, device=dev) if normalize else None
    divisor = torch.empty(2 * n, B, dtype=torch.float32, device=dev) if normalize else None
    ws = workspace(lib().cmh_msc_triplet_workspace_bytes(B), dev, "loss")
    check(lib().cmh_msc_triplet_loss(_ptr_array([u for u, _ in pairs]), _ptr_array([v for _, v in pairs]), n, ptr(label), B, K, Cn,
                                     float(margin), MSC_MINING[mining], int(bool(normalize)), ptr(loss), ptr(count), ptr(sim), ptr(coef),
                                     ptr(unit), ptr(divisor), ptr(ws), ws.numel(), stream_ptr(dev)), "cmh_msc_triplet_loss")
    return loss, count, sim, (pairs, coef, count, unit, divisor)


def msc_triplet_loss_backward(saved, dloss):
    """-> [(du, dv)] per pair, each f32 [B, K]; an intra-modal pair (v is u) gets its whole gradient in du and dv = None"""
    pairs, coef, count, unit, divisor = saved
    B, K = pairs[0][0].shape
    n = len(pairs)
    du = [torch.empty_like(u) for u, _ in pairs]
    dv = [None if v.data_ptr() == u.data_ptr() else torch.empty_like(v) for u, v in pairs]     # as the library tells them apart
    dloss = f32c(dloss).reshape(n)
    dv_ptrs = (C.c_void_p * n)(*[None if t is None else t.data_ptr() for t in dv])
    check(lib().cmh_msc_triplet_loss_backward(_ptr_array([u for u, _ in pairs]), _ptr_array([v for _, v in pairs]), n, B, K,
                                              int(unit is not None), ptr(coef), ptr(count), ptr(unit), ptr(divisor), ptr(dloss),
                                              _ptr_array(du), dv_ptrs, stream_ptr(coef.device)), "cmh_msc_triplet_loss_backward")
    return list(zip(du, dv))


CPF_MAX_B, CPF_MAX_K, CPF_MAX_C = 1024, 128, 1024           # csrc/cpf.hip's limits, for the wrapper's message
CPF_ROWS, CPF_CHUNK, CPF_SLICE = 16, 64, 256                # its rows per workgroup, classes per staged proxy tile, partners per backward slice
CPF_SCALARS = dict(tau=0.9, psi=0.7, sp=1.3, sn=1.3, mu=1.0, b=2.0)       # reference train/DScPH/CPF_loss.py:17-22


def cpf_loss(hi, ht, label, proxies, scalars=None, quant_weight=1.0, keep=False, cos=None):
    """CPF.forward (train/DScPH/CPF_loss.py:24-54) plus the step's two quantisation terms (train/DScPH/hash_train.py:64-70) in one call
    -> (loss f32 [1], terms f32 [4] = L_img, L_txt, q_img, q_txt, cos f32 [2, B, C], saved = what cpf_loss_backward takes, or None
    without `keep`).  `cos` may be handed in as a view to fill."""
    hi, ht, label, proxies = f32c(hi), f32c(ht), f32c(label), f32c(proxies)
    require_gpu(hi, ht, label, proxies)
    if hi.dim() != 2 or label.dim() != 2 or proxies.dim() != 2:
        raise NativeError("cpf_loss: hi, ht f32 [B, K], labels f32 [B, C] and proxies f32 [C, K] are expected")
    (B, K), Cn = hi.shape, label.shape[1]
    fit("cpf_loss", (ht, (B, K)), (label, (B, Cn)), (proxies, (Cn, K)))
    need = lib().cmh_cpf_workspace_bytes(B, K, Cn)
    if need == 0:
        raise NativeError(f"cpf_loss: B={B} K={K} C={Cn}: 1 <= B <= {CPF_MAX_B}, 1 <= K <= {CPF_MAX_K}, 1 <= C <= {CPF_MAX_C} are built")
    s = dict(CPF_SCALARS, **(scalars or {}))
    dev = hi.device
    ws = workspace(need, dev, "loss")
    loss, terms = torch.empty(1, dtype=torch.float32, device=dev), torch.empty(4, dtype=torch.float32, device=dev)
    cos = _out_view("cpf_loss", "cos", cos, (2, B, Cn), torch.float32, dev)
    tape = torch.empty(lib().cmh_cpf_tape_bytes(B, K, Cn) // 4, dtype=torch.float32, device=dev) if keep else None
    check(lib().cmh_cpf_loss(ptr(hi), ptr(ht), ptr(label), ptr(proxies), B, K, Cn, s["tau"], s["psi"], s["sp"], s["sn"], s["mu"], s["b"],
                             float(quant_weight), ptr(terms), ptr(loss), ptr(cos), ptr(tape), ptr(ws), ws.numel(), stream_ptr(dev)),
          "cmh_cpf_loss")
    return loss, terms, cos, ((label, cos, tape, (B, K, Cn), s, float(quant_weight)) if keep else None)


def cpf_loss_backward(saved, dloss):
    """-> d_hi, d_ht f32 [B, K], d_proxies f32 [C, K] = dloss * d loss / d hi, ht, proxies from the forward's cosines and tape"""
    label, cos, tape, (B, K, Cn), s, quant_weight = saved
    dev = cos.device
    d_hi, d_ht = (torch.empty(B, K, dtype=torch.float32, device=dev) for _ in range(2))
    d_w = torch.empty(Cn, K, dtype=torch.float32, device=dev)
    check(lib().cmh_cpf_loss_backward(ptr(label), ptr(cos), ptr(tape), B, K, Cn, s["tau"], s["sp"], s["sn"], s["mu"], quant_weight,
                                      ptr(f32c(dloss).reshape(1)), ptr(d_hi), ptr(d_ht), ptr(d_w), stream_ptr(dev)), "cmh_cpf_loss_backward")
    return d_hi, d_ht, d_w


DWS_MAX_B, DWS_MAX_K, DWS_MAX_C, DWS_MAX_PAIRS = 1024, 128, 1024, 3       # csrc/dws.hip's limits, for the wrappers' messages
DWS_SPACES = {"distances": 0, "embeddings": 1}              # what the miner measures: the rows of D (upstream), or D itself (the paper)


def _dws_ws(what, B, K, Cn, dev):
    need = lib().cmh_dws_workspace_bytes(B, K, Cn)
    if need == 0:
        raise NativeError(f"{what}: B={B} K={K} C={Cn}: 1 <= B <= {DWS_MAX_B}, 1 <= K <= {DWS_MAX_K}, 1 <= C <= {DWS_MAX_C} are built")
    return workspace(need, dev, "loss")


def dws_distances(pairs):
    """MarginLoss.forward's distances (train/DDWSH/loss.py:17-20) for up to three (u, v) pairs -> (dist f32 [n, B, B], saved = the
    operands as passed, their unit rows [2n, B, K] and divisors [2n, B])"""
    made = {}                                                   # one f32 contiguous copy per distinct operand: `v is u` stays so
    pairs = [tuple(made.setdefault(id(t), f32c(t)) for t in pr) for pr in pairs]
    require_gpu(*[t for pr in pairs for t in pr])
    if not 1 <= len(pairs) <= DWS_MAX_PAIRS or pairs[0][0].dim() != 2:
        raise NativeError(f"dws_distances: 1 .. {DWS_MAX_PAIRS} pairs of codes [B, K] are expected")
    B, K = pairs[0][0].shape
    fit("dws_distances", *[(t, (B, K)) for pr in pairs for t in pr])
    if not (1 <= B <= DWS_MAX_B and 1 <= K <= DWS_MAX_K):
        raise NativeError(f"dws_distances: B={B} K={K}: 1 <= B <= {DWS_MAX_B} and 1 <= K <= {DWS_MAX_K} are built")
    n, dev = len(pairs), pairs[0][0].device
    dist = torch.empty(n, B, B, dtype=torch.float32, device=dev)
    unit = torch.empty(2 * n, B, K, dtype=torch.float32, device=dev)
    divisor = torch.empty(2 * n, B, dtype=torch.float32, device=dev)
    check(lib().cmh_dws_distances(_ptr_array([u for u, _ in pairs]), _ptr_array([v for _, v in pairs]), n, B, K, ptr(dist), ptr(unit),
                                  ptr(divisor), stream_ptr(dev)), "cmh_dws_distances")
    return dist, (pairs, unit, divisor)


def dws_mine(dist, label, K, uniforms, cutoff=0.5, space="distances", weights=False):
    """DistanceWeightedMiner.__call__ (train/DDWSH/loss.py:91-128) on dist [n, B, B] with the uniforms [n, B, 2] = (u_p, u_n) handed in
    -> (triplets i32 [n, B, 2] = (positive, negative) or (-1, -1), w f64 [n, B, B] with `weights`, else None)"""
    if space not in DWS_SPACES:
        raise NativeError(f"dws_mine: space {space!r}: one of {sorted(DWS_SPACES)}")
    dist, label, uniforms = f32c(dist), f32c(label), f32c(uniforms)
    require_gpu(dist, label, uniforms)
    if dist.dim() != 3 or label.dim() != 2:
        raise NativeError("dws_mine: dist f32 [n, B, B] and labels f32 [B, C] are expected")
    n, B, Cn = dist.shape[0], dist.shape[1], label.shape[1]
    fit("dws_mine", (dist, (n, B, B)), (label, (B, Cn)), (uniforms, (n, B, 2)))
    if not 1 <= n <= DWS_MAX_PAIRS:
        raise NativeError(f"dws_mine: pairs={n}: 1 .. {DWS_MAX_PAIRS} are built")
    dev = dist.device
    ws = _dws_ws("dws_mine", B, K, Cn, dev)
    trip = torch.empty(n, B, 2, dtype=torch.int32, device=dev)
    w = torch.empty(n, B, B, dtype=torch.float64, device=dev) if weights else None
    check(lib().cmh_dws_mine(ptr(dist), n, ptr(label), B, int(K), Cn, float(cutoff), DWS_SPACES[space], ptr(uniforms), ptr(trip), ptr(w),
                             ptr(ws), ws.numel(), stream_ptr(dev)), "cmh_dws_mine")
    return trip, w


def dws_margin_loss(pairs, label, beta, triplets, margin=0.2, pre=None):
    """MarginLoss.forward (train/DDWSH/loss.py:16-49) for up to three (u, v) pairs over one label matrix, on the triplets i32 [n, B, 2]
    given -> (loss f32 [n], count i64 [n], dist f32 [n, B, B], saved = what dws_margin_loss_backward takes).  pre: what dws_distances
    returned for these pairs, when the caller has it already (the sampler ran on it)"""
    dist, (pairs, unit, divisor) = pre if pre is not None else dws_distances(pairs)
    label, beta = f32c(label), f32c(beta)
    require_gpu(label, beta, triplets)
    n, B, Cn = dist.shape[0], dist.shape[1], label.shape[-1]
    if label.dim() != 2 or triplets.dtype != torch.int32:
        raise NativeError("dws_margin_loss: labels f32 [B, C] and triplets i32 [n, B, 2] are expected")
    triplets = triplets.contiguous()
    fit("dws_margin_loss", (label, (B, Cn)), (beta, (Cn,)), (triplets, (n, B, 2)))
    dev = dist.device
    ws = _dws_ws("dws_margin_loss", B, pairs[0][0].shape[1], Cn, dev)
    loss = torch.empty(n, dtype=torch.float32, device=dev)
    count = torch.empty(n, dtype=torch.int64, device=dev)
    tape = torch.empty(n, B, 4, dtype=torch.float32, device=dev)
    check(lib().cmh_dws_margin_loss(ptr(dist), ptr(triplets), n, ptr(label), ptr(beta), B, Cn, float(margin), ptr(loss), ptr(count), ptr(tape),
                                    ptr(ws), ws.numel(), stream_ptr(dev)), "cmh_dws_margin_loss")
    return loss, count, dist, (pairs, label, dist, triplets, tape, count, unit, divisor)


def dws_margin_loss_backward(saved, dloss):
    """-> ([(du, dv)] per pair, each f32 [B, K]; an intra-modal pair (v is u) gets its whole gradient in du and dv = None), dbeta f32 [C]"""
    pairs, label, dist, triplets, tape, count, unit, divisor = saved
    B, K = pairs[0][0].shape
    n, Cn = len(pairs), label.shape[1]
    du = [torch.empty_like(u) for u, _ in pairs]
    dv = [None if v.data_ptr() == u.data_ptr() else torch.empty_like(v) for u, v in pairs]     # as the library tells them apart
    dbeta = torch.empty(Cn, dtype=torch.float32, device=label.device)
    dloss = f32c(dloss).reshape(n)
    dv_ptrs = (C.c_void_p * n)(*[None if t is None else t.data_ptr() for t in dv])
    check(lib().cmh_dws_margin_loss_backward(_ptr_array([u for u, _ in pairs]), _ptr_array([v for _, v in pairs]), n, ptr(label), B, K, Cn,
                                             ptr(dist), ptr(triplets), ptr(tape), ptr(count), ptr(unit), ptr(divisor), ptr(dloss),
                                             _ptr_array(du), dv_ptrs, ptr(dbeta), stream_ptr(label.device)), "cmh_dws_margin_loss_backward")
    return list(zip(du, dv)), dbeta


DJSRH_MAX_B, DJSRH_MAX_K, DJSRH_MAX_D = 1024, 128, 4096     # csrc/djsrh.hip's limits, for the wrappers' messages


def _djsrh_pair(what, a, b):
    a, b = f32c(a), f32c(b)
    require_gpu(a, b)
    if a.dim() != 2:
        raise NativeError(f"{what}: two f32 matrices [B, n] are expected")
    fit(what, (b, a.shape))
    return a, b


def _djsrh_ws(what, B, K, D, dev):
    need = lib().cmh_djsrh_workspace_bytes(B, K, D)
    if need == 0:
        raise NativeError(f"{what}: B={B} K={K} D={D}: 1 <= B <= {DJSRH_MAX_B}, 1 <= K <= {DJSRH_MAX_K}, 1 <= D <= {DJSRH_MAX_D} are built")
    return workspace(need, dev, "loss")


def djsrh_target(fi, ft, beta, eta, mu):
    """DJSRH's joint-semantics affinity of a batch from the stock towers' features fi, ft [B, D] -> S f32 [B, B] =
    mu ((1 - eta) St + (eta / B) St St^T), St = beta (2 cos(fi) - 1) + (1 - beta) (2 cos(ft) - 1); symmetric bit for bit"""
    fi, ft = _djsrh_pair("djsrh_target", fi, ft)
    B, D = fi.shape
    ws = _djsrh_ws("djsrh_target", B, 1, D, fi.device)
    S = torch.empty(B, B, dtype=torch.float32, device=fi.device)
    check(lib().cmh_djsrh_target(ptr(fi), ptr(ft), B, D, float(beta), float(eta), float(mu), ptr(S), ptr(ws), ws.numel(), stream_ptr(fi.device)),
          "cmh_djsrh_target")
    return S


def djsrh_loss(hi, ht, S, lambda1, lambda2, keep=False):
    """lambda1 mean((b_I b_I^T - S)^2) + mean((b_I b_T^T - S)^2) + lambda2 mean((b_T b_T^T - S)^2), b the row-normalised hi, ht [B, K]
    -> (loss [1], terms [3], tape for the backward or None, the operands as passed)"""
    hi, ht = _djsrh_pair("djsrh_loss", hi, ht)
    S = f32c(S)
    require_gpu(S)
    B, K = hi.shape
    fit("djsrh_loss", (S, (B, B)))
    dev = hi.device
    ws = _djsrh_ws("djsrh_loss", B, K, 1, dev)
    loss, terms = torch.empty(1, dtype=torch.float32, device=dev), torch.empty(3, dtype=torch.float32, device=dev)
    tape = torch.empty(2 * B + 3 * B * B, dtype=torch.float32, device=dev) if keep else None
    check(lib().cmh_djsrh_loss(ptr(hi), ptr(ht), ptr(S), B, K, float(lambda1), float(lambda2), ptr(terms), ptr(loss), ptr(tape), ptr(ws),
                               ws.numel(), stream_ptr(dev)), "cmh_djsrh_loss")
    return loss, terms, tape, hi, ht


def djsrh_loss_backward(hi, ht, tape, lambda1, lambda2, dloss):
    """-> d_hi, d_ht f32 [B, K] = dloss * d loss / d hi, ht from the forward's tape"""
    B, K = hi.shape
    d_hi, d_ht = torch.empty_like(hi), torch.empty_like(ht)
    ws = _djsrh_ws("djsrh_loss_backward", B, K, 1, hi.device)
    check(lib().cmh_djsrh_loss_backward(ptr(hi), ptr(ht), ptr(tape), B, K, float(lambda1), float(lambda2), ptr(f32c(dloss).reshape(1)),
                                        ptr(d_hi), ptr(d_ht), ptr(ws), ws.numel(), stream_ptr(hi.device)), "cmh_djsrh_loss_backward")
    return d_hi, d_ht


def dchmt_loss(img, txt, label, output_dim, similarity="euclidean", loss_type="l2", vartheta=0.5, sim_threshold=0.1):
    img, txt, label = f32c(img), f32c(txt), f32c(label)
    require_gpu(img, txt, label)
    B, D = img.shape
    Cn = label.shape[1]
    fit("dchmt_loss", (txt, (B, D)), (label, (B, Cn)))
    out = torch.empty(1, dtype=torch.float32, device=img.device)
    ws = workspace(lib().cmh_loss_workspace_bytes(B, D, Cn), img.device, "loss")
    sim = {"euclidean": 0, "cosine": 1}[similarity]
    lt = {"l1": 1, "l2": 2}[loss_type]
    check(lib().cmh_dchmt_loss(ptr(img), ptr(txt), ptr(label), B, D, Cn, int(output_dim), sim, lt, float(vartheta),
                               float(sim_threshold), ptr(out), ptr(ws), ws.numel(), stream_ptr(img.device)),
          "cmh_dchmt_loss")
    return out[0]


# ------------------------------------------------------------------------------------------ DNPH / TwDH
def batchnorm1d_train(x, w, b, eps=1e-5):
    x, w, b = f32c(x), f32c(w), f32c(b)
    require_gpu(x, w, b)
    B, d = x.shape
    fit("batchnorm1d_train", (w, (d,)), (b, (d,)))
    y = torch.empty_like(x)
    check(lib().cmh_batchnorm1d_train(ptr(x), ptr(w), ptr(b), float(eps), ptr(y), B, d, stream_ptr(x.device)),
          "cmh_batchnorm1d_train")
    return y


def twdh_targets(label, center, random_center):
    label, center, random_center = f32c(label), f32c(center), f32c(random_center)
    require_gpu(label, center, random_center)
    B, Cn = label.shape
    K = center.shape[1]
    fit("twdh_targets", (center, (Cn, K)), (random_center, (K,)))
    code = torch.empty(B, K, dtype=torch.float32, device=label.device)
    check(lib().cmh_twdh_targets(ptr(label), ptr(center), ptr(random_center), ptr(code), B, Cn, K,
                                 stream_ptr(label.device)), "cmh_twdh_targets")
    return code


def twdh_loss(p_img, p_txt, target):
    """-> (nce, quan) 0-dim tensors for one code length."""
    p_img, p_txt, target = f32c(p_img), f32c(p_txt), f32c(target)
    require_gpu(p_img, p_txt, target)
    B, K = target.shape
    fit("twdh_loss", (p_img, (B, 2 * K)), (p_txt, (B, 2 * K)))
    out = torch.empty(2, dtype=torch.float32, device=p_img.device)
    ws = workspace(256, p_img.device, "loss")
    check(lib().cmh_twdh_loss(ptr(p_img), ptr(p_txt), ptr(target), B, K, ptr(out), ptr(ws), ws.numel(),
                              stream_ptr(p_img.device)), "cmh_twdh_loss")
    return out[0], out[1]


def dnph_loss(hash_img, hash_txt, pre_img, pre_txt, label, proxies, noise_img=None, noise_txt=None, margin=1.0,
              noise_weight=0.1):
    """-> (loss, p_loss + d_loss, noise) 0-dim tensors."""
    ts = [f32c(t) for t in (hash_img, hash_txt, pre_img, pre_txt, label, proxies)]
    ni = None if noise_img is None else f32c(noise_img)
    nt = None if noise_txt is None else f32c(noise_txt)
    require_gpu(*ts, ni, nt)
    B, K = ts[0].shape
    Cn = ts[4].shape[1]
    fit("dnph_loss", (ts[1], (B, K)), (ts[2], (B, Cn)), (ts[3], (B, Cn)), (ts[4], (B, Cn)), (ts[5], (Cn, K)), (ni, (B, K)), (nt, (B, K)))
    out = torch.empty(3, dtype=torch.float32, device=ts[0].device)
    ws = workspace(256, ts[0].device, "loss")
    check(lib().cmh_dnph_loss(*[ptr(t) for t in ts], ptr(ni), ptr(nt), B, K, Cn, float(margin), float(noise_weight),
                              ptr(out), ptr(ws), ws.numel(), stream_ptr(ts[0].device)), "cmh_dnph_loss")
    return out[0], out[1], out[2]


def assign_rows(emb, rows, return_col=False):
    """gene_noise on the device (train/DNPH_TOMM/b_reg.py): emb f32 [P, B, K] (or [B, K]) and the noise matrix rows f32 [B, K] ->
    the rows of `rows` assigned to the samples of each problem at minimal total L2 cost, f32 like emb; with return_col also the
    permutation, int32 [P, B] (row i gets rows[col[p, i]]).  No host synchronisation."""
    emb, rows = f32c(emb), f32c(rows)
    require_gpu(emb, rows)
    single = emb.dim() == 2
    if single:
        emb = emb.unsqueeze(0)
    if emb.dim() != 3 or rows.dim() != 2:
        raise NativeError(f"assign_rows: emb {tuple(emb.shape)} / rows {tuple(rows.shape)}, expected [P, B, K] and [B, K]")
    P, B, K = emb.shape
    fit("assign_rows", (rows, (B, K)))
    dev = emb.device
    out = torch.empty(P, B, K, dtype=torch.float32, device=dev)
    col = torch.empty(P, B, dtype=torch.int32, device=dev) if return_col else None
    ws = workspace(lib().cmh_assign_rows_workspace_bytes(P, B), dev, f"assign@{stream_ptr(dev)}")
    check(lib().cmh_assign_rows(ptr(emb), ptr(rows), P, B, K, ptr(out), ptr(col), ptr(ws), ws.numel(), stream_ptr(dev)),
          "cmh_assign_rows")
    if single:
        out, col = out[0], (None if col is None else col[0])
    return (out, col) if return_col else out


# ------------------------------------------------------------------------------------------ training-free heads (csrc/itq.hip)
ITQ_MAX_D, ITQ_MAX_K, ITQ_EIGH_SWEEPS = 1024, 128, 60


def _f64c(t):
    if t.dtype != torch.float64:
        raise NativeError(f"the fit runs in f64: operand of dtype {t.dtype}")
    return t.contiguous()


def _running(what, *pairs):
    """Running sums passed back in to be added to, as (tensor, shape) pairs: each contiguous f64 of its shape, on the GPU (None passes)."""
    fit(what, *pairs)
    for t, _ in pairs:
        if t is not None and (t.dtype != torch.float64 or not t.is_contiguous()):
            raise NativeError(f"{what}: the running sums must be contiguous f64 tensors")
    require_gpu(*(t for t, _ in pairs))


def _out_view(what, name, t, shape, dtype, dev):
    """An output the caller may hand in as a view to fill: made here where None, else contiguous, of this shape and dtype, on the GPU."""
    if t is None:
        return torch.empty(shape, dtype=dtype, device=dev)
    fit(what, (t, shape))
    if t.dtype != dtype or not t.is_contiguous():
        raise NativeError(f"{what}: {name} must be a contiguous {str(dtype).replace('torch.', '')} tensor")
    require_gpu(t)
    return t


def _head_outputs(d, k, dev):
    """-> W_i, b_i, W_t, b_t (f32 [K, D] / [K]) and s (f64 [1]) for the heads entries to fill"""
    W_i, W_t = (torch.empty(k, d, dtype=torch.float32, device=dev) for _ in range(2))
    b_i, b_t = (torch.empty(k, dtype=torch.float32, device=dev) for _ in range(2))
    return W_i, b_i, W_t, b_t, torch.empty(1, dtype=torch.float64, device=dev)


def itq_moments(F, sums=None):
    """Running f64 sums of one batch of f32 features F [N, D]: (sum [D], sq [D, D]) (+)= (sum_n f, sum_n f f^T).  `sums`: the pair a
    previous call returned, updated in place; None starts new ones."""
    F = f32c(F)
    require_gpu(F)
    if F.dim() != 2 or F.shape[0] < 1:
        raise NativeError(f"itq_moments: features {tuple(F.shape)}, expected [N, D] with N >= 1")
    n, d = F.shape
    dev = F.device
    if sums is None:
        sums, acc = (torch.empty(d, dtype=torch.float64, device=dev), torch.empty(d, d, dtype=torch.float64, device=dev)), 0
    else:
        _running("itq_moments", (sums[0], (d,)), (sums[1], (d, d)))
        acc = 1
    ws = workspace(lib().cmh_itq_moments_workspace_bytes(n, d), dev, "itq")
    check(lib().cmh_itq_moments(ptr(F), n, d, ptr(sums[0]), ptr(sums[1]), acc, ptr(ws), ws.numel(), stream_ptr(dev)), "cmh_itq_moments")
    return sums


def itq_covariance(sums_i, sums_t, n):
    """-> mu_i [D], mu_t [D], alpha [2], C [D, D] (f64) from the running sums of both modalities over n pairs."""
    d = sums_i[0].shape[0]
    fit("itq_covariance", (sums_i[0], (d,)), (sums_i[1], (d, d)), (sums_t[0], (d,)), (sums_t[1], (d, d)))
    ops = [_f64c(t) for t in (sums_i[0], sums_i[1], sums_t[0], sums_t[1])]
    require_gpu(*ops)
    dev = ops[0].device
    mu_i, mu_t = (torch.empty(d, dtype=torch.float64, device=dev) for _ in range(2))
    alpha = torch.empty(2, dtype=torch.float64, device=dev)
    cov = torch.empty(d, d, dtype=torch.float64, device=dev)
    check(lib().cmh_itq_covariance(*(ptr(t) for t in ops), int(n), d, ptr(mu_i), ptr(mu_t), ptr(alpha), ptr(cov), stream_ptr(dev)),
          "cmh_itq_covariance")
    return mu_i, mu_t, alpha, cov


def itq_eigh(cov, max_sweeps=ITQ_EIGH_SWEEPS):
    """Symmetric eigen-decomposition of cov [D, D] f64 (upper triangle) by cyclic Jacobi -> evals [D] descending, evecs [D, D]
    (column j goes with evals[j], largest entry positive), sweeps run, converged."""
    cov = _f64c(cov)
    require_gpu(cov)
    if cov.dim() != 2 or cov.shape[0] != cov.shape[1]:
        raise NativeError(f"itq_eigh: matrix {tuple(cov.shape)}, expected [D, D]")
    d, dev = cov.shape[0], cov.device
    evals = torch.empty(d, dtype=torch.float64, device=dev)
    evecs = torch.empty(d, d, dtype=torch.float64, device=dev)
    info = (C.c_int32 * 2)(0, 0)
    ws = workspace(lib().cmh_itq_eigh_workspace_bytes(d, max_sweeps), dev, "itq")
    check(lib().cmh_itq_eigh(ptr(cov), d, max_sweeps, ptr(evals), ptr(evecs), info, ptr(ws), ws.numel(), stream_ptr(dev)), "cmh_itq_eigh")
    return evals, evecs, int(info[0]), bool(info[1])


def itq_project(F, mu, alpha, P, out=None):
    """V [N, K] f64 = alpha * (F - mu) P; alpha: one f64 element on the device; out: a [N, K] f64 view to fill (rows of a larger V)."""
    F, mu, alpha, P = f32c(F), _f64c(mu), _f64c(alpha), _f64c(P)
    require_gpu(F, mu, alpha, P)
    n, d = F.shape
    k = P.shape[1]
    fit("itq_project", (mu, (d,)), (P, (d, k)))
    if alpha.numel() != 1:
        raise NativeError("itq_project: alpha must hold one element")
    out = _out_view("itq_project", "out", out, (n, k), torch.float64, F.device)
    check(lib().cmh_itq_project(ptr(F), n, d, k, ptr(mu), ptr(alpha), ptr(P), ptr(out), stream_ptr(F.device)), "cmh_itq_project")
    return out


def itq_step(V, R):
    """One pass: Z = V R [rows, K] f64, B = (Z >= 0 ? +1 : -1) int8, M = B^T V [K, K], obj2 = (|B - Z|^2, |Z|^2)."""
    V, R = _f64c(V), _f64c(R)
    require_gpu(V, R)
    rows, k = V.shape
    fit("itq_step", (R, (k, k)))
    dev = V.device
    Z = torch.empty(rows, k, dtype=torch.float64, device=dev)
    B = torch.empty(rows, k, dtype=torch.int8, device=dev)
    M = torch.empty(k, k, dtype=torch.float64, device=dev)
    obj2 = torch.empty(2, dtype=torch.float64, device=dev)
    ws = workspace(lib().cmh_itq_step_workspace_bytes(rows, k), dev, "itq")
    check(lib().cmh_itq_step(ptr(V), rows, k, ptr(R), ptr(Z), ptr(B), ptr(M), ptr(obj2), ptr(ws), ws.numel(), stream_ptr(dev)), "cmh_itq_step")
    return Z, B, M, obj2


def itq_polar(M, want_sweeps=False):
    """(orthogonal polar factor of M [K, K] f64)^T, ITQ's rotation update."""
    M = _f64c(M)
    require_gpu(M)
    if M.dim() != 2 or M.shape[0] != M.shape[1]:
        raise NativeError(f"itq_polar: matrix {tuple(M.shape)}, expected [K, K]")
    k, dev = M.shape[0], M.device
    R = torch.empty(k, k, dtype=torch.float64, device=dev)
    sweeps = torch.zeros(1, dtype=torch.int32, device=dev) if want_sweeps else None
    ws = workspace(lib().cmh_itq_polar_workspace_bytes(k), dev, "itq")
    check(lib().cmh_itq_polar(ptr(M), k, ptr(R), ptr(sweeps), ptr(ws), ws.numel(), stream_ptr(dev)), "cmh_itq_polar")
    return (R, sweeps) if want_sweeps else R


def itq_rotate(V, R0, iters):
    """ITQ from R0 -> R [K, K], obj [iters + 1] (|B - Z|^2 at the start of each iteration, then for R), zz = |V R|^2; all on the
    device, nothing is read back."""
    V, R0 = _f64c(V), _f64c(R0)
    require_gpu(V, R0)
    rows, k = V.shape
    fit("itq_rotate", (R0, (k, k)))
    dev = V.device
    R = torch.empty(k, k, dtype=torch.float64, device=dev)
    obj = torch.empty(int(iters) + 1, dtype=torch.float64, device=dev)
    zz = torch.empty(1, dtype=torch.float64, device=dev)
    ws = workspace(lib().cmh_itq_rotate_workspace_bytes(rows, k), dev, "itq")
    check(lib().cmh_itq_rotate(ptr(V), rows, k, ptr(R0), int(iters), ptr(R), ptr(obj), ptr(zz), ptr(ws), ws.numel(), stream_ptr(dev)),
          "cmh_itq_rotate")
    return R, obj, zz


def itq_heads(P, R, mu_i, mu_t, alpha, zz, rows):
    """-> W_i, b_i, W_t, b_t (f32 [K, D] / [K]) and s (f64 [1]): s = 0.5 / rms(V R), W_m = s alpha_m (P R)^T, b_m = -W_m mu_m."""
    ops = [_f64c(t) for t in (P, R, mu_i, mu_t, alpha, zz)]
    require_gpu(*ops)
    d, k = ops[0].shape
    fit("itq_heads", (ops[1], (k, k)), (ops[2], (d,)), (ops[3], (d,)), (ops[4], (2,)), (ops[5], (1,)))
    dev = ops[0].device
    outs = _head_outputs(d, k, dev)
    check(lib().cmh_itq_heads(*(ptr(t) for t in ops), int(rows), d, k, *(ptr(t) for t in outs), stream_ptr(dev)), "cmh_itq_heads")
    return outs


def itq_heads_pair(P_i, P_t, R, mu_i, mu_t, alpha, zz, rows):
    """itq_heads with one projection per modality: W_m = s alpha_m (P_m R)^T."""
    ops = [_f64c(t) for t in (P_i, P_t, R, mu_i, mu_t, alpha, zz)]
    require_gpu(*ops)
    d, k = ops[0].shape
    fit("itq_heads_pair", (ops[1], (d, k)), (ops[2], (k, k)), (ops[3], (d,)), (ops[4], (d,)), (ops[5], (2,)), (ops[6], (1,)))
    dev = ops[0].device
    outs = _head_outputs(d, k, dev)
    check(lib().cmh_itq_heads_pair(*(ptr(t) for t in ops), int(rows), d, k, *(ptr(t) for t in outs), stream_ptr(dev)), "cmh_itq_heads_pair")
    return outs


def itq_cross_moments(Fi, Ft, cross=None):
    """Running f64 cross sum of one batch of paired f32 features [N, D]: cross [D, D] (+)= sum_n f_i f_t^T (not symmetric).  `cross`:
    what a previous call returned, updated in place; None starts a new one."""
    Fi, Ft = f32c(Fi), f32c(Ft)
    require_gpu(Fi, Ft)
    if Fi.dim() != 2 or Fi.shape[0] < 1:
        raise NativeError(f"itq_cross_moments: features {tuple(Fi.shape)}, expected [N, D] with N >= 1")
    n, d = Fi.shape
    fit("itq_cross_moments", (Ft, (n, d)))
    dev = Fi.device
    if cross is None:
        cross, acc = torch.empty(d, d, dtype=torch.float64, device=dev), 0
    else:
        _running("itq_cross_moments", (cross, (d, d)))
        acc = 1
    ws = workspace(lib().cmh_itq_cross_moments_workspace_bytes(n, d), dev, "itq")
    check(lib().cmh_itq_cross_moments(ptr(Fi), ptr(Ft), n, d, ptr(cross), acc, ptr(ws), ws.numel(), stream_ptr(dev)), "cmh_itq_cross_moments")
    return cross


def itq_cca_covariance(sums_i, sums_t, cross, n):
    """-> mu_i [D], mu_t [D], alpha [2], S_ii, S_tt, S_it [D, D] (f64) from the running sums of both modalities and their cross sum
    over n pairs: S_mm = alpha_m^2 cov(f_m) (trace 1), S_it = alpha_i alpha_t cov(f_i, f_t)."""
    d = sums_i[0].shape[0]
    fit("itq_cca_covariance", (sums_i[0], (d,)), (sums_i[1], (d, d)), (sums_t[0], (d,)), (sums_t[1], (d, d)), (cross, (d, d)))
    ops = [_f64c(t) for t in (sums_i[0], sums_i[1], sums_t[0], sums_t[1], cross)]
    require_gpu(*ops)
    dev = ops[0].device
    mu_i, mu_t = (torch.empty(d, dtype=torch.float64, device=dev) for _ in range(2))
    alpha = torch.empty(2, dtype=torch.float64, device=dev)
    S_ii, S_tt, S_it = (torch.empty(d, d, dtype=torch.float64, device=dev) for _ in range(3))
    check(lib().cmh_itq_cca_covariance(*(ptr(t) for t in ops), int(n), d, ptr(mu_i), ptr(mu_t), ptr(alpha), ptr(S_ii), ptr(S_tt), ptr(S_it),
                                       stream_ptr(dev)), "cmh_itq_cca_covariance")
    return mu_i, mu_t, alpha, S_ii, S_tt, S_it


def itq_inv_sqrt(values, shift=0.0, want_root=False):
    """1 / sqrt(values + shift) (0 where values + shift <= 0) of an f64 vector, and with want_root also sqrt(max(values + shift, 0))."""
    values = _f64c(values)
    require_gpu(values)
    if values.dim() != 1:
        raise NativeError(f"itq_inv_sqrt: values {tuple(values.shape)}, expected a vector")
    out = torch.empty_like(values)
    root = torch.empty_like(values) if want_root else None
    check(lib().cmh_itq_inv_sqrt(ptr(values), values.shape[0], float(shift), ptr(out), ptr(root), stream_ptr(values.device)), "cmh_itq_inv_sqrt")
    return (out, root) if want_root else out


def itq_matmul(A, B, d=None, col_scale=None, trans_a=False, trans_b=False):
    """C [M, N] f64 = op(A) diag(d) op(B) diag(col_scale): op(A) = A [M, Kc] or, with trans_a, the transpose of A [Kc, M]; op(B) =
    B [Kc, N] or, with trans_b, the transpose of B [N, Kc]; d [Kc] and col_scale [N] optional.  One fma chain per element over the
    contraction index in ascending order: two calls give equal bits, and A A^T is symmetric bit for bit."""
    A, B = _f64c(A), _f64c(B)
    d = None if d is None else _f64c(d)
    col_scale = None if col_scale is None else _f64c(col_scale)
    require_gpu(A, B, d, col_scale)
    if A.dim() != 2 or B.dim() != 2:
        raise NativeError(f"itq_matmul: operands {tuple(A.shape)} and {tuple(B.shape)}, expected two matrices")
    m, kc = (A.shape[1], A.shape[0]) if trans_a else A.shape
    n = B.shape[0] if trans_b else B.shape[1]
    fit("itq_matmul", (B, (n, kc) if trans_b else (kc, n)), (d, (kc,)), (col_scale, (n,)))
    out = torch.empty(m, n, dtype=torch.float64, device=A.device)
    check(lib().cmh_itq_matmul(ptr(A), ptr(B), ptr(d), ptr(col_scale), m, n, kc, int(bool(trans_a)), int(bool(trans_b)), ptr(out),
                               stream_ptr(A.device)), "cmh_itq_matmul")
    return out


# ------------------------------------------------------------------------------------------ supervised training-free heads (csrc/dch.hip)
DCH_MAX_C, DCH_MAX_ROUNDS = 1024, 64


def _codes(B, what):
    if B.dtype != torch.int8 or B.dim() != 2 or not B.is_contiguous():
        raise NativeError(f"{what}: B must be a contiguous int8 [N, K] tensor of +1 / -1")
    require_gpu(B)
    return B


def dch_covariance(sq, mu, alpha, n):
    """S [D, D] f64 = alpha^2 (sq / n - mu mu^T) of one modality; alpha: one f64 element on the device."""
    sq, mu, alpha = _f64c(sq), _f64c(mu), _f64c(alpha)
    require_gpu(sq, mu, alpha)
    d = mu.shape[0]
    fit("dch_covariance", (sq, (d, d)), (alpha, (1,)))
    S = torch.empty(d, d, dtype=torch.float64, device=sq.device)
    check(lib().cmh_dch_covariance(ptr(sq), ptr(mu), ptr(alpha), int(n), d, ptr(S), stream_ptr(sq.device)), "cmh_dch_covariance")
    return S


def dch_start(Za, Zb):
    """B int8 [N, K] = +1 where Za + Zb >= 0, else -1."""
    Za, Zb = _f64c(Za), _f64c(Zb)
    require_gpu(Za, Zb)
    n, k = Za.shape
    fit("dch_start", (Zb, (n, k)))
    B = torch.empty(n, k, dtype=torch.int8, device=Za.device)
    check(lib().cmh_dch_start(ptr(Za), ptr(Zb), n, k, ptr(B), stream_ptr(Za.device)), "cmh_dch_start")
    return B


def dch_xtb(X, B, want_bsum=False, into=None):
    """X^T B [Dx, K] f64 for X f32 [N, Dx] and B int8 [N, K]; with want_bsum also 1^T B [K].  `into`: what a previous call returned (the
    matrix, or the pair with want_bsum), added to in place."""
    X, B = f32c(X), _codes(B, "dch_xtb")
    require_gpu(X)
    if X.dim() != 2 or X.shape[0] < 1:
        raise NativeError(f"dch_xtb: rows {tuple(X.shape)}, expected [N, Dx] with N >= 1")
    n, dx = X.shape
    k = B.shape[1]
    fit("dch_xtb", (B, (n, k)))
    dev = X.device
    if into is None:
        out, bsum, acc = torch.empty(dx, k, dtype=torch.float64, device=dev), None, 0
        if want_bsum:
            bsum = torch.empty(k, dtype=torch.float64, device=dev)
    else:
        out, bsum = into if want_bsum else (into, None)
        _running("dch_xtb", (out, (dx, k)), (bsum, (k,)))
        acc = 1
    ws = workspace(lib().cmh_dch_xtb_workspace_bytes(n, dx, k), dev, "dch")
    check(lib().cmh_dch_xtb(ptr(X), ptr(B), n, dx, k, ptr(out), ptr(bsum), acc, ptr(ws), ws.numel(), stream_ptr(dev)), "cmh_dch_xtb")
    return (out, bsum) if want_bsum else out


def dch_btb(B):
    """B^T B [K, K] f64 (exact integers)."""
    B = _codes(B, "dch_btb")
    n, k = B.shape
    out = torch.empty(k, k, dtype=torch.float64, device=B.device)
    ws = workspace(lib().cmh_dch_btb_workspace_bytes(n, k), B.device, "dch")
    check(lib().cmh_dch_btb(ptr(B), n, k, ptr(out), ptr(ws), ws.numel(), stream_ptr(B.device)), "cmh_dch_btb")
    return out


def dch_center(T, bsum, mu, alpha, n):
    """U [D, K] = alpha (T - mu bsum^T) / n for T = F^T B: X^T B / n with X = alpha (F - mu)."""
    T, bsum, mu, alpha = _f64c(T), _f64c(bsum), _f64c(mu), _f64c(alpha)
    require_gpu(T, bsum, mu, alpha)
    d, k = T.shape
    fit("dch_center", (bsum, (k,)), (mu, (d,)), (alpha, (1,)))
    U = torch.empty(d, k, dtype=torch.float64, device=T.device)
    check(lib().cmh_dch_center(ptr(T), ptr(bsum), ptr(mu), ptr(alpha), int(n), d, k, ptr(U), stream_ptr(T.device)), "cmh_dch_center")
    return U


def dch_solve(A, R, shift=0.0, info=None):
    """W [K, C] = (A + shift I)^-1 R by Cholesky for a symmetric positive definite A [K, K] -> W, info (int32 [1] on the device: 0, or
    1 + the first pivot that is not positive, W then zeros).  `info`: a one-element int32 view to fill."""
    A, R = _f64c(A), _f64c(R)
    require_gpu(A, R)
    if A.dim() != 2 or A.shape[0] != A.shape[1] or R.dim() != 2:
        raise NativeError(f"dch_solve: operands {tuple(A.shape)} and {tuple(R.shape)}, expected [K, K] and [K, C]")
    k, c = R.shape
    fit("dch_solve", (A, (k, k)))
    if info is None:
        info = torch.zeros(1, dtype=torch.int32, device=A.device)
    if info.dtype != torch.int32 or info.numel() != 1:
        raise NativeError("dch_solve: info must hold one int32")
    require_gpu(info)
    W = torch.empty(k, c, dtype=torch.float64, device=A.device)
    check(lib().cmh_dch_solve(ptr(A), float(shift), ptr(R), k, c, ptr(W), ptr(info), stream_ptr(A.device)), "cmh_dch_solve")
    return W, info


def dch_targets(Y, B, W, Z_i, Z_t, mu, lam, want_q=True, obj2=None):
    """-> Qt [K, N] f64 (bit-major; None without want_q) = (Y W^T + mu Z_i + mu Z_t)^T and obj2 [2] = (the objective |Y - B W|^2 +
    lam |W|^2 + mu (|B - Z_i|^2 + |B - Z_t|^2), |Z_i|^2 + |Z_t|^2).  `obj2`: a two-element f64 view to fill."""
    Y, B, W, Z_i, Z_t = f32c(Y), _codes(B, "dch_targets"), _f64c(W), _f64c(Z_i), _f64c(Z_t)
    require_gpu(Y, W, Z_i, Z_t)
    n, k = B.shape
    if Y.dim() != 2:
        raise NativeError(f"dch_targets: labels {tuple(Y.shape)}, expected [N, C]")
    c = Y.shape[1]
    fit("dch_targets", (Y, (n, c)), (W, (k, c)), (Z_i, (n, k)), (Z_t, (n, k)))
    dev = B.device
    Qt = torch.empty(k, n, dtype=torch.float64, device=dev) if want_q else None
    obj2 = _out_view("dch_targets", "obj2", obj2, (2,), torch.float64, dev)
    ws = workspace(lib().cmh_dch_targets_workspace_bytes(n), dev, "dch")
    check(lib().cmh_dch_targets(ptr(Y), ptr(B), ptr(W), ptr(Z_i), ptr(Z_t), float(mu), float(lam), n, k, c, ptr(Qt), ptr(obj2), ptr(ws),
                                ws.numel(), stream_ptr(dev)), "cmh_dch_targets")
    return Qt, obj2


def dch_dcc(Qt, G, B, rounds, flips=None, min_margin=None):
    """`rounds` rounds of the bit-cyclic coordinate descent on B int8 [N, K], IN PLACE, from the targets Qt [K, N] and G [K, K] ->
    flips int64 [rounds], min_margin f64 [1] (device).  `flips` / `min_margin`: views of that shape to fill."""
    Qt, G, B = _f64c(Qt), _f64c(G), _codes(B, "dch_dcc")
    require_gpu(Qt, G)
    n, k = B.shape
    rounds = int(rounds)
    fit("dch_dcc", (Qt, (k, n)), (G, (k, k)))
    dev = B.device
    flips = _out_view("dch_dcc", "flips", flips, (max(rounds, 0),), torch.int64, dev)
    min_margin = _out_view("dch_dcc", "min_margin", min_margin, (1,), torch.float64, dev)
    ws = workspace(lib().cmh_dch_dcc_workspace_bytes(n, rounds), dev, "dch")
    check(lib().cmh_dch_dcc(ptr(Qt), ptr(G), ptr(B), n, k, rounds, ptr(flips), ptr(min_margin), ptr(ws), ws.numel(), stream_ptr(dev)), "cmh_dch_dcc")
    return flips, min_margin


# ------------------------------------------------------------------------------------------ optimiser
def bf16_copy_of(p):
    """the encoder's bf16 GEMM copy of a parameter (model/base/model.py::_gemm_w) if it has one the fused step can rewrite - bf16,
    contiguous, of p's size, on p's device - else None: anything else hung on `_cmh_bf16` is left alone and never stamped current"""
    copy = getattr(p, "_cmh_bf16", None)
    if copy is None or copy.dtype != torch.bfloat16 or copy.numel() != p.numel() or copy.device != p.device or not copy.is_contiguous():
        return None
    return copy


def bert_adam_step(entries, b1, b2, eps):
    """One fused BertAdam step over `entries` = [(param, grad, next_m, next_v, lr_scheduled, weight_decay, max_grad_norm)]
    (all f32, contiguous, on one GPU).  Updates param / next_m / next_v in place and, like clip_grad_norm_, the clipped grad."""
    if not entries:
        return
    dev = entries[0][0].device
    arr = (AdamTensor * len(entries))()
    total = 0
    for i, (p, g, m, v, lr, wd, mx) in enumerate(entries):
        require_gpu(p, g, m, v)
        for t in (p, g, m, v):
            if t.dtype != torch.float32 or not t.is_contiguous() or t.numel() != p.numel():
                raise NativeError("bert_adam_step: tensors must be contiguous f32 of one size")
        copy = bf16_copy_of(p)
        arr[i] = AdamTensor(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), p.numel(), float(lr), float(wd), float(mx),
                            None if copy is None else copy.data_ptr())
        total += p.numel()
    need = lib().cmh_bert_adam_workspace_bytes(len(entries), total)
    ws = workspace(need, dev, "adam")
    check(lib().cmh_bert_adam_step(arr, len(entries), float(b1), float(b2), float(eps), ptr(ws), ws.numel(), stream_ptr(dev)),
          "cmh_bert_adam_step")
