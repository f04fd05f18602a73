"""ctypes binding of libvsscore.so (C ABI: ``include/vs_scorer.h``) and its in-tree build.

The library is the product path; nothing here falls back to PyTorch or to the oracle.  If the
shared object is missing or a symbol is absent, ``load()`` raises — loudly — instead.
"""
from __future__ import annotations

import concurrent.futures
import ctypes as C
import os
import subprocess
import threading
from typing import NamedTuple

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(HERE, "csrc")
INCLUDE = os.path.join(ROOT, "include")
LIB_PATH = os.path.join(HERE, "libvsscore.so")
DIAG_LIB_PATH = os.path.join(HERE, "libvsscore_diag.so")
SOURCES = ("vs_kernels.hip", "vs_attention.hip", "vs_attention_w64.hip", "vs_mlp_fused.hip", "vs_gemm_ring.hip", "vs_scorer.cpp", "vs_eval.cpp",
           "vs_train_kernels.hip", "vs_train_attention.hip", "vs_train_attention_bf16.hip", "vs_train_gemm_rows.hip", "vs_pretrain_kernels.hip",
           "vs_train.cpp", "vs_segment.hip", "vs_segment_gram.hip", "vs_segment.cpp", "vs_optim.hip", "vs_attention_maps.hip",
           "vs_eval_device.hip", "vs_eval_device.cpp", "vs_summary.hip", "vs_summary.cpp", "vs_batch.hip", "vs_cnn.hip", "vs_cnn.cpp",
           "vs_resize.hip", "vs_resize.cpp", "vs_cnn3d.hip", "vs_cnn3d.cpp", "vs_weights.cpp", "vs_error.cpp")
# vs_resize.cpp computes PIL's coefficient tables in double: no multiply-add of it may be contracted, whatever the host
EXTRA_FLAGS = {"vs_resize.cpp": ("-ffp-contract=off",)}
ABI_VERSION = 3

VS_OK, VS_ERR_INVALID, VS_ERR_WORKSPACE, VS_ERR_HIP = 0, 1, 2, 3
VS_FLAG_SIGMOID = 1
VS_FLAG_BF16_ATTENTION = 2
VS_FLAG_BF16_LINEAR = 4
VS_FLAG_F16X3_LINEAR = 8
VS_FLAG_F16X3_ATTENTION = 16
VS_FLAG_SPLITK = 32              # opt-in latency mode for reference-sized calls (include/vs_scorer.h)
VS_TRAIN_FLAG_BF16_LINEAR = 1
VS_TRAIN_FLAG_BF16_ATTENTION = 2
VS_TRAIN_FLAG_FP16 = 4          # modifier: the 16-bit type is IEEE fp16 (the reference's own autocast type) instead of bf16
VS_TRAIN_FLAG_PACKED_LP_ATTENTION = 8     # packed calls only: with BF16_ATTENTION, the packed attention on the 16-bit pipe too

VS_ADAM_MAX_TENSORS = 64
VS_GRAD_NORM_L2, VS_GRAD_NORM_MAX = 0, 1
VS_KTS_FEATURES_F32, VS_KTS_KERNEL_F32, VS_KTS_KERNEL_F64 = 0, 1, 2
VS_KTS_SCORES, VS_KTS_BACKTRACK, VS_KTS_AUTO = 0, 1, 2
VS_KTS_GRAM_DOT, VS_KTS_GRAM_COSINE, VS_KTS_GRAM_RBF = 0, 1, 2
VS_CNN_INPUT_F32_NCHW, VS_CNN_INPUT_U8_NHWC, VS_CNN_INPUT_F32_NHWC = 0, 1, 2
VS_CNN_NUM_CONVS, VS_CNN_FEATURES = 57, 1024
VS_CNN3D_INPUT_F32_NCDHW, VS_CNN3D_INPUT_U8_NDHWC, VS_CNN3D_INPUT_F32_NDHWC = 0, 1, 2
VS_R3D_NUM_CONVS, VS_R3D_FEATURES = 20, 512
VS_RESIZE_SWAP_RB = 1
VS_RESIZE_PATH_FUSED, VS_RESIZE_PATH_SMALL_TILE = 0, 1
NUM_STAGES = 6


class ModelDesc(C.Structure):
    _fields_ = [("d_model", C.c_int32), ("num_heads", C.c_int32), ("num_layers", C.c_int32),
                ("in_features", C.c_int32), ("max_len", C.c_int32), ("num_classes", C.c_int32)]


_LAYER_FIELDS = ("wq", "bq", "wk", "bk", "wv", "bv", "wo", "bo", "ln1_g", "ln1_b",
                 "w1", "b1", "w2", "b2", "ln2_g", "ln2_b")


class LayerParams(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in _LAYER_FIELDS]


class ModelParams(C.Structure):
    _fields_ = [("embed_w", C.c_void_p), ("embed_b", C.c_void_p), ("pos_embedding", C.c_void_p),
                ("layers", C.POINTER(LayerParams)), ("final_w", C.c_void_p), ("final_b", C.c_void_p)]


class DropoutCfg(C.Structure):
    _fields_ = [("p_embed", C.c_float), ("p", C.c_float), ("seed", C.c_uint64), ("flags", C.c_uint32), ("reserved", C.c_uint32)]


class EvalVideo(C.Structure):   # vs_eval_video (include/vs_eval.h)
    _fields_ = [("scores", C.c_void_p), ("positions", C.c_void_p), ("change_points", C.c_void_p), ("user_summary", C.c_void_p),
                ("user_scores", C.c_void_p)] + [(n, C.c_int32) for n in ("n_scores", "n_positions", "n_frames", "n_shots", "n_users",
                                                                        "user_len", "n_score_users", "use_max", "user_scores_f32")]


LayerGrads = LayerParams        # vs_layer_grads: same field names, destinations instead of sources


class ModelGrads(C.Structure):  # vs_model_grads (no positional table: it is a buffer, not a parameter)
    _fields_ = [("embed_w", C.c_void_p), ("embed_b", C.c_void_p), ("layers", C.POINTER(LayerParams)),
                ("final_w", C.c_void_p), ("final_b", C.c_void_p)]


class AdamCfg(C.Structure):    # vs_adam_cfg (include/vs_optim.h)
    _fields_ = [("lr", C.c_double), ("beta1", C.c_double), ("beta2", C.c_double), ("eps", C.c_double),
                ("weight_decay", C.c_double), ("decoupled", C.c_int32), ("reserved", C.c_int32)]


class AdamTensor(C.Structure):  # vs_adam_tensor
    _fields_ = [("p", C.c_void_p), ("g", C.c_void_p), ("m", C.c_void_p), ("v", C.c_void_p), ("mirror", C.c_void_p),
                ("step", C.c_void_p), ("n", C.c_size_t)]


class KtsKernel(C.Structure):   # vs_kts_kernel (include/vs_segment.h)
    _fields_ = [("kind", C.c_int32), ("reserved", C.c_int32), ("gamma", C.c_double)]


class GradTensor(C.Structure):  # vs_grad_tensor
    _fields_ = [("g", C.c_void_p), ("n", C.c_size_t)]


class CnnConvParams(C.Structure):   # vs_cnn_conv_params (include/features/vs_features.h)
    _fields_ = [(n, C.c_void_p) for n in ("weight", "gamma", "beta", "running_mean", "running_var")]


class CnnParams(C.Structure):       # vs_cnn_params
    _fields_ = [("conv", CnnConvParams * VS_CNN_NUM_CONVS)]


class Cnn3dConvParams(C.Structure):     # vs_cnn3d_conv_params (include/features/vs_video_features.h)
    _fields_ = [(n, C.c_void_p) for n in ("weight", "gamma", "beta", "running_mean", "running_var")]


class R3dParams(C.Structure):           # vs_r3d_params
    _fields_ = [("conv", Cnn3dConvParams * VS_R3D_NUM_CONVS)]


# --------------------------------------------------------------------------------------------
# the C ABI: {header: {symbol: (restype, argtypes)}}, every prototype of include/*.h once (tests/test_binding_host.py
# compares names, argument counts and return kinds with the headers).  A wrong entry does not fail: it truncates.
# --------------------------------------------------------------------------------------------
_P, _I, _Z, _F, _D, _U32, _U64, _RC = C.c_void_p, C.c_int32, C.c_size_t, C.c_float, C.c_double, C.c_uint32, C.c_uint64, C.c_int
_ref = C.POINTER
_LINEAR = [_P] * 4 + [_I] * 4 + [_P, _I, _P]
_LINEAR_OPERANDS = [_P] * 4 + [_I] * 5 + [_P]
_LINEAR_LN = [_P] * 7 + [_I] * 3 + [_P] * 2 + [_I] * 2 + [_P] * 2
_ATTENTION = [_P] * 5 + [_I] * 4 + [_F, _P]
_BYTES_BT = (_Z, [_P, _I, _I])                     # (weights or lengths, B, T or width) -> bytes
_DROPOUT_MASK = [_P, _I, _I, _I, _U64, _U32, _F, _P]
_KTS_SIZES = [_P, _I, _I, _I, _P, _I]
_BINDINGS = {
    "vs_scorer.h": {
        "vs_abi_version": (_RC, []),
        "vs_last_error": (C.c_char_p, []),
        "vs_weights_pack": (_RC, [_ref(ModelDesc), _ref(ModelParams), _P, _ref(_P)]),
        "vs_weights_free": (None, [_P]),
        "vs_weights_update": (_RC, [_P, _ref(ModelParams), _P]),
        "vs_weights_set_norm_width": (_RC, [_P, _I]),
        "vs_set_option": (_RC, [C.c_char_p, _I]),
        "vs_scorer_workspace_bytes": _BYTES_BT,
        "vs_scorer_forward": (_RC, [_P, _P, _P, _I, _I, _U32, _P, _P, _P, _Z, _P]),
        "vs_scorer_workspace_bytes_packed": (_Z, [_P, _P, _I]),
        "vs_scorer_forward_packed": (_RC, [_P, _P, _P, _P, _I, _U32, _P, _P, _P, _Z, _P]),
        "vs_scorer_workspace_bytes_cls": _BYTES_BT,
        "vs_scorer_forward_cls": (_RC, [_P, _P, _P, _P, _I, _I, _U32, _P, _P, _P, _Z, _P]),
        "vs_linear_f32": (_RC, _LINEAR),
        "vs_qkv_proj_f32": (_RC, [_P] * 4 + [_I] * 4 + [_P]),
        "vs_attention_f32": (_RC, _ATTENTION),
        "vs_attention_bf16": (_RC, _ATTENTION),
        "vs_attention_bf16_stored": (_RC, [_P] * 5 + [_I] * 4 + [_P]),
        "vs_attention_qscale": (_F, [_F]),
        "vs_attention_f16x3": (_RC, _ATTENTION),
        "vs_linear_residual_layernorm_f32": (_RC, _LINEAR_LN),
        "vs_linear_bf16": (_RC, _LINEAR),
        "vs_linear_residual_layernorm_bf16": (_RC, _LINEAR_LN),
        "vs_linear_f16x3": (_RC, _LINEAR),
        "vs_linear_residual_layernorm_f16x3": (_RC, _LINEAR_LN),
        "vs_mlp_block_bf16": (_RC, [_P, _I, _P, _P, _I, _I, _I, _P, _P]),
        "vs_linear_bf16_operands": (_RC, _LINEAR_OPERANDS),
        "vs_qkv_proj_bf16_operands": (_RC, _LINEAR_OPERANDS),
        "vs_to_bf16": (_RC, [_P, _P, _Z, _P]),
        "vs_linear_bf16_a16": (_RC, [_P] * 4 + [_I] * 3 + [_P, _P]),
        "vs_profile_enable": (_RC, [_I]),
        "vs_profile_collect": (_RC, [_ref(_D), _ref(C.c_int64)]),
        "vs_stage_name": (C.c_char_p, [_I]),
    },
    "vs_eval.h": {
        "vs_eval_upsample": (_RC, [_P, _I, _P, _I, _I, _P]),
        "vs_eval_knapsack": (_RC, [_I, _P, _P, _I, _P, _ref(_I)]),
        "vs_eval_generate_summary": (_RC, [_P, _I, _P, _I, _I, _P, _I, _P, _I]),
        "vs_eval_fscore": (_RC, [_P, _I, _P, _I, _I, _I, _ref(_D)]),
        "vs_eval_rank_correlation": (_RC, [_P, _I, _P, _I, _ref(_D), _ref(_D)]),
        "vs_eval_corpus": (_RC, [_ref(EvalVideo), _I, _I, _P, _P, _P]),
    },
    "vs_eval_device.h": {       # the same evaluation from device-resident scores; opt-in
        "vs_eval_set_create": (_RC, [_ref(EvalVideo), _I, _P, _ref(_P)]),
        "vs_eval_set_free": (None, [_P]),
        "vs_eval_set_workspace_bytes": (_Z, [_P, _P, _I]),
        "vs_eval_set_run": (_RC, [_P, _P, _P, _I] + [_P] * 5 + [_Z, _P]),
    },
    "vs_summary.h": {           # scores on the device in, the summary and its selected frames on the device out
        "vs_summarize_workspace_bytes": (_Z, [_I] + [_P] * 4 + [_D]),
        "vs_summarize": (_RC, [_I] + [_P] * 6 + [_D] + [_P] * 7 + [_Z, _P]),
    },
    "vs_batch.h": {             # the batches of a training epoch cut from a device-resident set
        "vs_batch_gather_packed": (_RC, [_P] * 3 + [_I] + [_P] * 2 + [_I, C.c_int64, _I] + [_P] * 3),
        "vs_batch_gather_padded": (_RC, [_P] * 3 + [_I] + [_P] * 2 + [_I] * 3 + [_F, _I] + [_P] * 4),
        "vs_batch_gather_rows": (_RC, [_P, _I, _P, _I, _I, _P, _P]),
    },
    "vs_train.h": {
        "vs_train_prepare": (_RC, [_P, _P]),
        "vs_train_saved_bytes": _BYTES_BT,
        "vs_train_workspace_bytes": _BYTES_BT,
        "vs_train_forward": (_RC, [_P, _P, _P, _I, _I, _ref(DropoutCfg), _P, _P, _P, _Z, _P, _Z, _P]),
        "vs_train_backward": (_RC, [_P, _P, _P, _I, _I, _ref(DropoutCfg), _P, _P, _P, _Z, _ref(ModelGrads), _P, _P, _Z, _P]),
        "vs_mse_mask_loss_forward": (_RC, [_P, _P, _P, _I, _I, _P, _P, _P]),
        "vs_mse_mask_loss_backward": (_RC, [_P, _P, _P, _P, _I, _I, _P, _P]),
        "vs_train_attention_forward": (_RC, [_P] * 6 + [_I] * 4 + [_F, _U64, _U32, _F, _P]),
        "vs_train_attention_backward": (_RC, [_P] * 9 + [_I] * 4 + [_F, _U64, _U32, _F, _P]),
        "vs_train_attention_dropout_bits_bytes": (_Z, [_I] * 3),
        "vs_train_attention_dropout_bits": (_RC, _DROPOUT_MASK),
        "vs_train_attention_forward_bf16": (_RC, [_P] * 6 + [_I] * 4 + [_F, _F, _P, _I, _P]),
        "vs_train_attention_backward_bf16": (_RC, [_P] * 9 + [_I] * 4 + [_F, _F, _P, _I, _P]),
        "vs_train_wgrad_scratch_floats": (_Z, [_I] * 3),
        "vs_train_wgrad": (_RC, [_P, _P, _I, _I, _I, _P, _P, _P, _P]),
        "vs_train_wgrad_bf16": (_RC, [_P, _P, _I, _I, _I, _P, _P, _P, _P]),
        "vs_train_dropout_mask_attention": (_RC, _DROPOUT_MASK),
        "vs_train_dropout_mask_rows": (_RC, [_P, _I, _I, _U64, _U32, _F, _P]),
        "vs_train_dropout_site": (_U32, [_I, _I]),
        "vs_train_saved_field": (_RC, [_P, _I, _I, _I, _I, _ref(_Z), _ref(_Z)]),
        "vs_train_last_format": (_U32, []),
        "vs_pretrain_head_state_bytes": (_Z, [_I] * 3),
        "vs_pretrain_head_workspace_bytes": (_Z, [_I] * 4),
        "vs_pretrain_head_forward": (_RC, [_P] * 6 + [_I] * 4 + [_F, _I] + [_P] * 4),
        "vs_pretrain_head_backward": (_RC, [_P] * 8 + [_I] * 4 + [_F, _I] + [_P] * 5 + [_Z, _P]),
        # packed ragged batches (lengths: host int32 array, then the same values on the device)
        "vs_train_check_packed": (_RC, [_ref(ModelDesc), _P, _I]),
        "vs_train_saved_bytes_desc": (_Z, [_ref(ModelDesc), _P, _I, _I]),
        "vs_train_saved_bytes_packed": (_Z, [_P, _P, _I]),
        "vs_train_workspace_bytes_packed": (_Z, [_P, _P, _I]),
        "vs_train_forward_packed": (_RC, [_P, _P, _P, _P, _I, _ref(DropoutCfg), _P, _P, _P, _Z, _P, _Z, _P]),
        "vs_train_backward_packed": (_RC, [_P, _P, _P, _P, _I, _ref(DropoutCfg), _P, _P, _P, _Z, _ref(ModelGrads), _P, _P, _Z, _P]),
        "vs_mse_packed_loss_forward": (_RC, [_P, _P, _I, _D, _P, _P, _P]),
        "vs_mse_packed_loss_backward": (_RC, [_P, _P, _P, _I, _D, _P, _P]),
        "vs_train_attention_packed_scratch_bytes": _BYTES_BT,
        "vs_train_attention_forward_packed": (_RC, [_P] * 7 + [_I] * 3 + [_F, _U64, _U32, _F, _P, _Z, _P]),
        "vs_train_attention_backward_packed": (_RC, [_P] * 9 + [_I] * 3 + [_F, _U64, _U32, _F, _P, _Z, _P]),
        "vs_train_dropout_mask_attention_packed": (_RC, [_P, _P, _I, _I, _U64, _U32, _F, _P]),
        "vs_train_saved_field_packed": (_RC, [_P, _P, _I, _I, _I, _ref(_Z), _ref(_Z)]),
        # ... on the 16-bit pipe: (..., scale, seed, site, p, f16, scratch, scratch_bytes, stream)
        "vs_train_attention_packed_lp_scratch_bytes": _BYTES_BT,
        "vs_train_attention_forward_packed_lp": (_RC, [_P] * 7 + [_I] * 3 + [_F, _U64, _U32, _F, _I, _P, _Z, _P]),
        "vs_train_attention_backward_packed_lp": (_RC, [_P] * 9 + [_I] * 3 + [_F, _U64, _U32, _F, _I, _P, _Z, _P]),
        # ... and the pretraining head on them: (hidden, logits, lengths, lengths_dev, B, ref_len, vid, vt_w, ...)
        "vs_pretrain_head_state_bytes_packed": _BYTES_BT,
        "vs_pretrain_head_workspace_bytes_packed": (_Z, [_P, _I, _I, _I]),
        "vs_pretrain_head_forward_packed": (_RC, [_P] * 4 + [_I] * 2 + [_P] * 3 + [_I] * 2 + [_F, _I] + [_P] * 4),
        "vs_pretrain_head_backward_packed": (_RC, [_P] * 4 + [_I] * 2 + [_P] * 5 + [_I] * 2 + [_F, _I] + [_P] * 5 + [_Z, _P]),
    },
    "vs_segment.h": {           # kernel temporal segmentation
        "vs_kts_workspace_bytes": (_Z, _KTS_SIZES),
        "vs_kts_segment": (_RC, [_P, _I, _I, _P, _I] + [_P] * 5 + [_I] + [_P] * 4 + [_Z, _P]),
        "vs_kts_scatters": (_RC, [_P, _I, _I, _I, _P, _P, _Z, _P]),
        # cosine / Gaussian kernels, the one-launch ragged Gram, the score of given change points
        "vs_kts_gram_workspace_bytes": _BYTES_BT,
        "vs_kts_gram": (_RC, [_P, _I, _P, _I, _ref(KtsKernel), _P, _P, _Z, _P]),
        "vs_kts_workspace_bytes_k": (_Z, _KTS_SIZES + [_ref(KtsKernel)]),
        "vs_kts_segment_k": (_RC, [_P, _I, _I, _P, _I] + [_P] * 5 + [_I, _ref(KtsKernel)] + [_P] * 4 + [_Z, _P]),
        "vs_kts_eval_score": (_RC, [_P, _I, _I, _ref(KtsKernel), _P, _I] + [_P] * 4 + [_Z, _P]),
    },
    "vs_optim.h": {             # the Adam step
        "vs_adam_step_tensors": (_RC, [_ref(AdamTensor), _I, _ref(AdamCfg), _P, _P, _P, _P]),
        "vs_adam_state_bytes": (_Z, [_P]),
        "vs_adam_state_init": (_RC, [_P, _P, _P]),
        "vs_adam_state_field": (_RC, [_P, _I, _I, _ref(_Z), _ref(_Z)]),
        "vs_adam_step": (_RC, [_P, _ref(ModelParams), _ref(ModelGrads), _P, _ref(AdamCfg), _P, _P, _P]),
        "vs_grad_norm_workspace_bytes": (_Z, [_ref(GradTensor), _I]),
        "vs_grad_norm_tensors": (_RC, [_ref(GradTensor), _I, _I, _D, _P, _P, _P, _Z, _P]),
        "vs_grad_norm": (_RC, [_P, _ref(ModelGrads), _I, _D, _P, _P, _P, _Z, _P]),
        "vs_grad_scale_tensors": (_RC, [_ref(GradTensor), _I, _P, _P]),
    },
    "vs_inspect.h": {           # attention maps on request
        "vs_inspect_workspace_bytes": (_Z, [_P, _I, _I, _I]),
        "vs_inspect_forward": (_RC, [_P] * 4 + [_I] * 2 + [_ref(_I), _I] + [_P] * 6 + [_Z, _P]),
        "vs_attention_probs_workspace_bytes": (_Z, [_I] * 3),
        "vs_attention_probs_f32": (_RC, [_P] * 6 + [_I] * 4 + [_F, _P, _Z, _P]),
    },
}
(EXPORTS, EVAL_EXPORTS, EVAL_DEVICE_EXPORTS, SUMMARY_EXPORTS, BATCH_EXPORTS, TRAIN_EXPORTS, SEGMENT_EXPORTS, OPTIM_EXPORTS,
 INSPECT_EXPORTS) = (tuple(_BINDINGS["vs_%s.h" % h]) for h in ("scorer", "eval", "eval_device", "summary", "batch", "train", "segment",
                                                                "optim", "inspect"))

# The attention maps on packed ragged batches: include/packed/vs_inspect_packed.h, an addition BESIDE the table above (which
# is every prototype of include/*.h, pinned by tests/test_binding_host.py) with the same form and the same check of its own
# (tests/test_attention_maps_packed_host.py).  lengths: host int32 array, then the same values on the device.
PACKED_INSPECT_HEADER = os.path.join("packed", "vs_inspect_packed.h")
_PACKED_INSPECT_BINDINGS = {
    "vs_inspect_workspace_bytes_packed": (_Z, [_P, _P, _I]),
    "vs_inspect_forward_packed": (_RC, [_P] * 4 + [_I, _ref(_I), _I] + [_P] * 6 + [_Z, _P]),
    "vs_attention_probs_packed_workspace_bytes": (_Z, [_P, _I, _I]),
    "vs_attention_probs_packed_f32": (_RC, [_P] * 4 + [_I] * 3 + [_F] + [_P] * 4 + [_Z, _P]),
}
PACKED_INSPECT_EXPORTS = tuple(_PACKED_INSPECT_BINDINGS)

# The GoogLeNet pool5 frame features: include/features/vs_features.h, a table of its own beside the two above, with the same
# form and the same check (tests/test_features_host.py).
FEATURES_HEADER = os.path.join("features", "vs_features.h")
_FEATURES_BINDINGS = {
    "vs_cnn_pack": (_RC, [_ref(CnnParams), _P, _ref(_P)]),
    "vs_cnn_free": (None, [_P]),
    "vs_cnn_min_side": (_I, []),
    "vs_cnn_workspace_bytes": (_Z, [_I] * 3),
    "vs_cnn_forward": (_RC, [_P, _P] + [_I] * 4 + [_P, _P, _Z, _P]),
    "vs_cnn_packed_floats": (_Z, [_I] * 3),
    "vs_cnn_pack_conv": (_RC, [_ref(CnnConvParams)] + [_I] * 3 + [_P, _P]),
    "vs_cnn_conv": (_RC, [_P] + [_I] * 5 + [_P] + [_I] * 4 + [_P, _I, _I, _P]),
    "vs_cnn_maxpool": (_RC, [_P] + [_I] * 8 + [_P, _P]),
}
FEATURES_EXPORTS = tuple(_FEATURES_BINDINGS)

# The frame resize in front of them: include/features/vs_resize.h, again a table of its own (tests/test_resize_host.py).
RESIZE_HEADER = os.path.join("features", "vs_resize.h")
_RESIZE_BINDINGS = {
    "vs_resize_output_size": (_RC, [_I] * 3 + [_ref(_I)] * 2),
    "vs_resize_plan_create": (_RC, [_I] * 4 + [_P, _ref(_P)]),
    "vs_resize_plan_free": (None, [_P]),
    "vs_resize_plan_describe": (_RC, [_P] + [_ref(_I)] * 3),
    "vs_resize_workspace_bytes": (_Z, [_P, _I]),
    "vs_resize_run": (_RC, [_P, _P, _I, _U32, _P, _P, _Z, _P]),
}
RESIZE_EXPORTS = tuple(_RESIZE_BINDINGS)

# The R3D-18 video-level feature: include/features/vs_video_features.h, a table of its own (tests/test_video_features_host.py).
VIDEO_FEATURES_HEADER = os.path.join("features", "vs_video_features.h")
_VIDEO_FEATURES_BINDINGS = {
    "vs_r3d_pack": (_RC, [_ref(R3dParams), _P, _ref(_P)]),
    "vs_r3d_free": (None, [_P]),
    "vs_r3d_workspace_bytes": (_Z, [_I] * 4),
    "vs_r3d_flops": (_D, [_I] * 4),
    "vs_r3d_normalisation": (_RC, [_ref(_F)]),
    "vs_r3d_forward": (_RC, [_P, _P] + [_I] * 5 + [_P, _P, _Z, _P]),
    "vs_cnn3d_packed_floats": (_Z, [_I] * 4),
    "vs_cnn3d_pack_conv": (_RC, [_ref(Cnn3dConvParams)] + [_I] * 4 + [_P, _P]),
    "vs_cnn3d_conv": (_RC, [_P] + [_I] * 6 + [_P] + [_I] * 7 + [_P, _I, _P, _P]),
}
VIDEO_FEATURES_EXPORTS = tuple(_VIDEO_FEATURES_BINDINGS)


def hipcc_path() -> str:
    for p in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc"):
        if p and os.path.exists(p):
            return p
    return "hipcc"


def needs_build() -> bool:
    if not os.path.exists(LIB_PATH):
        return True
    t = os.path.getmtime(LIB_PATH)
    deps = [os.path.join(CSRC, f) for f in os.listdir(CSRC)] + [os.path.join(INCLUDE, f) for f in os.listdir(INCLUDE)]
    deps.append(os.path.join(INCLUDE, PACKED_INSPECT_HEADER))
    deps.append(os.path.join(INCLUDE, FEATURES_HEADER))
    deps.append(os.path.join(INCLUDE, RESIZE_HEADER))
    deps.append(os.path.join(INCLUDE, VIDEO_FEATURES_HEADER))
    return any(os.path.getmtime(d) > t for d in deps)


def build(force: bool = False, verbose: bool = False, diag: bool = False) -> str:
    """Cross-compiles the HIP sources for gfx950 into the in-tree ``libvsscore.so``
    (works without a GPU).  Returns the library path.  ``diag=True`` builds ``libvsscore_diag.so`` instead: the same
    sources with ``-DVS_WITH_DIAG`` (stamped GEMM and attention instantiations, the timing ablations of the bf16
    layer-tail and one-wave-per-SIMD attention kernels) for ``tools/`` only - the product library does not carry them."""
    if diag:
        return _build(DIAG_LIB_PATH, ["-DVS_WITH_DIAG"], verbose)
    if not force and not needs_build():
        return LIB_PATH
    return _build(LIB_PATH, [], verbose)


def _build(out_path: str, extra, verbose: bool) -> str:
    flags = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Wno-unused-value", "-fno-slp-vectorize",
             "-pthread", "-I" + INCLUDE, "-I" + CSRC] + list(extra)
    # -fno-slp-vectorize: packed f32 VALU (v_pk_mul/add_f32) beside MFMAs costs more than the scalar
    # forms it replaces (MI355X_MICROARCH.md, cycle constants); keep elementwise epilogue/softmax ops scalar
    tmp = out_path + ".tmp.%d" % os.getpid()
    objs = [tmp + "." + src.replace(".", "_") + ".o" for src in SOURCES]     # vs_segment.hip / .cpp: distinct objects

    def compile_one(pair):
        src, obj = pair
        cmd = [hipcc_path()] + flags + list(EXTRA_FLAGS.get(src, ())) + ["-c", os.path.join(CSRC, src), "-o", obj]
        if verbose:
            print(" ".join(cmd))
        return subprocess.run(cmd, capture_output=True, text=True)

    try:
        # one hipcc per translation unit, side by side (the two kernel files dominate the build time)
        with concurrent.futures.ThreadPoolExecutor(max_workers=len(SOURCES)) as pool:
            for r in pool.map(compile_one, zip(SOURCES, objs)):
                if r.returncode != 0:
                    raise RuntimeError("hipcc failed building libvsscore.so:\n" + r.stdout + r.stderr)
        cmd = [hipcc_path(), "--offload-arch=gfx950", "-shared", "-fPIC", "-pthread"] + objs + ["-o", tmp]
        if verbose:
            print(" ".join(cmd))
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError("hipcc failed linking libvsscore.so:\n" + r.stdout + r.stderr)
    finally:
        for o in objs:
            if os.path.exists(o):
                os.remove(o)
    os.replace(tmp, out_path)
    return out_path


def _bind(lib) -> None:
    """Checks that ``lib`` has every symbol of ``_BINDINGS`` and the binding's ABI version, then sets the signatures."""
    table = {name: sig for group in _BINDINGS.values() for name, sig in group.items()}
    for name in table:
        if not hasattr(lib, name):
            raise RuntimeError("libvsscore.so lacks symbol %s (stale build?)" % name)
    for name, (restype, argtypes) in table.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = restype, argtypes
    if lib.vs_abi_version() != ABI_VERSION:
        raise RuntimeError("libvsscore.so ABI %d != binding ABI %d" % (lib.vs_abi_version(), ABI_VERSION))


def _bind_table(lib, table) -> None:
    for name in table:
        if not hasattr(lib, name):
            raise RuntimeError("libvsscore.so lacks symbol %s (stale build?)" % name)
    for name, (restype, argtypes) in table.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = restype, argtypes


def _bind_packed_inspect(lib) -> None:
    """``_bind`` for the table of include/packed/vs_inspect_packed.h: every symbol present, then the signatures."""
    _bind_table(lib, _PACKED_INSPECT_BINDINGS)


def _bind_features(lib) -> None:
    """``_bind`` for the table of include/features/vs_features.h."""
    _bind_table(lib, _FEATURES_BINDINGS)


def _bind_resize(lib) -> None:
    """``_bind`` for the table of include/features/vs_resize.h."""
    _bind_table(lib, _RESIZE_BINDINGS)


def _bind_video_features(lib) -> None:
    """``_bind`` for the table of include/features/vs_video_features.h."""
    _bind_table(lib, _VIDEO_FEATURES_BINDINGS)


_lib = None
_lock = threading.Lock()


def load() -> C.CDLL:
    """dlopen + signature setup.  Raises RuntimeError when the library is missing/stale-ABI."""
    global _lib
    if _lib is not None:
        return _lib
    with _lock:
        if _lib is not None:
            return _lib
        # VS_LIBRARY: tools/ point this at libvsscore_diag.so (build(diag=True)); never a fallback
        path = os.environ.get("VS_LIBRARY") or LIB_PATH
        if not os.path.exists(path):
            raise RuntimeError(
                "libvsscore.so not found at %s — the HIP scorer library is not built. "
                "Run `python -c 'import __graft_entry__ as g; g.build()'` (needs hipcc). "
                "There is no PyTorch/CPU fallback for the scoring path." % path)
        lib = C.CDLL(path)
        _bind(lib)
        _bind_packed_inspect(lib)
        _bind_features(lib)
        _bind_resize(lib)
        _bind_video_features(lib)
        _lib = lib
    return _lib


class TrainForm(NamedTuple):
    """The word of ``vs_train_last_format`` decoded (bits 0..5 of include/vs_train.h; ``VsTrainForm`` in csrc/vs_train_plan.h):
    lp - 16-bit Linear / dgrad / wgrad products; lpa - 16-bit attention products; qkv16 / h16 - q / k / v, the MLP hidden
    tensor stored as 16-bit planes; rows16 - written by the A-stationary GEMM; f16 - the 16-bit type is fp16, not bf16."""
    lp: bool
    lpa: bool
    qkv16: bool
    h16: bool
    rows16: bool
    f16: bool

    def dtype(self, low_precision: bool) -> str:
        """'fp32', or the 16-bit type's name where ``low_precision`` (one of the fields above, or several or-ed) holds"""
        return ("fp16" if self.f16 else "bf16") if low_precision else "fp32"


def train_form(word: int) -> TrainForm:
    return TrainForm(*(bool(word >> bit & 1) for bit in range(6)))


def set_option(name: str, value: int) -> None:
    """A/B / test switch of the library (include/vs_scorer.h: vs_set_option); value < 0 restores the default."""
    check(load().vs_set_option(name.encode(), int(value)))


def profile_collect():
    """{stage_name: (ms_sum, launches)} of the stages recorded since vs_profile_enable(1)."""
    lib = load()
    ms = (C.c_double * NUM_STAGES)()
    n = (C.c_int64 * NUM_STAGES)()
    check(lib.vs_profile_collect(ms, n))
    return {lib.vs_stage_name(i).decode(): (ms[i], n[i]) for i in range(NUM_STAGES)}


def check(rc: int) -> None:
    """Non-zero status -> RuntimeError with the library's message (reference: ATen RuntimeError)."""
    if rc != VS_OK:
        msg = load().vs_last_error().decode("utf-8", "replace")
        raise RuntimeError("libvsscore: %s (status %d)" % (msg, rc))
