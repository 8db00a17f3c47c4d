"""
ctypes binding of libktf_hip.so (the C-ABI declared in include/ktf_hip.h).

This is the only place the Python host side touches native code. There is NO CPU
fallback: if the shared library is missing or no MI355X is visible, every compute
entry point raises (`KtfBackendError`) instead of silently computing elsewhere.
"""

import ctypes as C
import threading
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# The product loads the in-tree library. KTF_LIBRARY names another build of the same ABI (probe / timing-ablation builds of
# tools/) and is honoured ONLY together with KTF_ALLOW_LIBRARY_OVERRIDE=1, so that a variable left over in a shell cannot
# silently swap the library; bench.py records the path that was loaded.
_OVERRIDE = os.environ.get("KTF_LIBRARY") if os.environ.get("KTF_ALLOW_LIBRARY_OVERRIDE") == "1" else None
LIB_PATH = _OVERRIDE or os.path.join(_HERE, "libktf_hip.so")

KTF_F32, KTF_BF16, KTF_BF16P = 0, 1, 3
KTF_F16 = 2                       # ktf_egs_*: the bank's other element type (include/ktf_egs.h)
PAIR = "bf16p"                    # stands for KTF_BF16P where a torch dtype is expected: pairs live in float32 tensors
GEMM_F32, GEMM_BF16, GEMM_BF16X3, GEMM_F16MX, GEMM_BF16X4 = 0, 1, 2, 5, 6
ACT_NONE, ACT_RELU, ACT_SIGMOID, ACT_TANH = 0, 1, 2, 3
(ACT_ELU, ACT_SELU, ACT_SOFTPLUS, ACT_SOFTSIGN, ACT_SWISH, ACT_GELU, ACT_EXPONENTIAL, ACT_HARD_SIGMOID,
 ACT_SOFTMAX) = range(4, 13)         # run as a pass of their own (ktf_activation_f32)
TDNN_REF_TILES, TDNN_DET_STATS, TDNN_K_INTERLEAVED, TDNN_W_TILED = 1, 2, 4, 8   # KtfTdnnDesc.flags
TAIL_SKIP_EMPTY = 1                 # ktf_xvec_tail_f32 flags
TDNN_MX_LOADER = 1 << 24          # ktf_tdnn_mx*: the loader-wave kernel (csrc/tdnn_mxl.hip) and its weight images

IN_WAV, IN_FRAMES, IN_WINDOWED, IN_WAV_I16 = 0, 1, 2, 3
OUT_FRAMES, OUT_WINDOWED, OUT_FBANK, OUT_MFCC = 0, 1, 2, 3
FE_NONE, FE_FRAMING, FE_GENERIC, FE_FAST512 = 0, 1, 2, 3      # KtfFrontendPlan.kernel


class KtfBackendError(RuntimeError):
    pass


def ktf_dtype(t):
    """torch dtype -> KTF_* element type of an activation / weight buffer."""
    import torch
    return {torch.float32: KTF_F32, torch.bfloat16: KTF_BF16, PAIR: KTF_BF16P}[t]


def act_torch_dtype(gemm):
    """Storage dtype of the frame-level activations for a GEMM mode."""
    import torch
    return {GEMM_BF16: torch.bfloat16}.get(gemm, torch.float32)


class FrontendCfg(C.Structure):
    _fields_ = [
        ("frame_size", C.c_int32), ("frame_shift", C.c_int32), ("nfft", C.c_int32), ("num_mels", C.c_int32),
        ("num_ceps", C.c_int32), ("remove_dc", C.c_int32), ("raw_energy", C.c_int32), ("use_energy", C.c_int32),
        ("use_power", C.c_int32), ("use_log", C.c_int32), ("use_lifter", C.c_int32), ("preemph", C.c_float),
        ("dither", C.c_float), ("energy_floor", C.c_float), ("eps", C.c_float), ("pad_mode", C.c_int32), ("row_stride", C.c_int32),
    ]


class FrontendTables(C.Structure):
    _fields_ = [
        ("window", C.c_void_p), ("twiddle", C.c_void_p), ("rtwiddle", C.c_void_p), ("mel_start", C.c_void_p),
        ("mel_len", C.c_void_p), ("mel_w", C.c_void_p), ("dct", C.c_void_p), ("lifter", C.c_void_p),
        ("fast_tw", C.c_void_p), ("fast_mel_meta", C.c_void_p), ("fast_mel_w", C.c_void_p),
        ("mel_stride", C.c_int32), ("reserved", C.c_int32),
    ]


class FrontendPlan(C.Structure):
    _fields_ = [("kernel", C.c_int32), ("log2_nfft", C.c_int32), ("dither", C.c_int32), ("kind", C.c_int32), ("mfix", C.c_int32),
                ("std", C.c_int32), ("nq", C.c_int32), ("grid_x", C.c_int32), ("grid_y", C.c_int32), ("lds_bytes", C.c_int64),
                ("T", C.c_int64)]


class VadCfg(C.Structure):
    _fields_ = [("energy_threshold", C.c_float), ("energy_mean_scale", C.c_float), ("proportion_threshold", C.c_float),
                ("frames_context", C.c_int32), ("energy_coeff", C.c_int32)]


class CmvnCfg(C.Structure):
    _fields_ = [("window", C.c_int32), ("norm_vars", C.c_int32), ("valid", C.c_int32), ("reserved", C.c_int32)]


class VcPlan(C.Structure):
    _fields_ = [("pos_ints", C.c_int64), ("stage_floats", C.c_int64), ("bs_floats", C.c_int64), ("col_floats", C.c_int64),
                ("lds_bytes", C.c_int64), ("nsplit", C.c_int32), ("lds_form", C.c_int32)]


class TdnnDesc(C.Structure):
    _fields_ = [("units", C.c_int32), ("din", C.c_int32), ("din_pad", C.c_int32), ("nctx", C.c_int32),
                ("ctx", C.c_int32 * 16), ("subsampling", C.c_int32), ("valid", C.c_int32), ("act", C.c_int32),
                ("gemm", C.c_int32), ("x_dtype", C.c_int32), ("w_dtype", C.c_int32), ("y_dtype", C.c_int32),
                ("flags", C.c_int32)]


class OptimSeg(C.Structure):
    _fields_ = [("begin", C.c_int64), ("end", C.c_int64), ("group", C.c_int32), ("max_change", C.c_float)]


class OptimGroup(C.Structure):
    _fields_ = [("lr", C.c_double), ("weight_decay", C.c_double)]


class EgsIndex(C.Structure):
    _fields_ = [("spk_order", C.c_void_p), ("spk_off", C.c_void_p), ("spk_utts", C.c_void_p), ("spk_utt_len", C.c_void_p)]


_P = C.c_void_p
_i64, _i32, _f32, _u64 = C.c_int64, C.c_int32, C.c_float, C.c_uint64

# name -> (restype, argtypes); mirrors include/ktf_hip.h one to one
PROTOTYPES = {
    "ktf_version": (_i32, []),
    "ktf_last_error": (C.c_size_t, [C.c_char_p, C.c_size_t]),
    "ktf_build_id": (C.c_char_p, []),
    "ktf_clock_probe": (C.c_int, [_P, _i64, _P]),
    "ktf_num_frames": (_i64, [_i64, _i32, _i32]),
    "ktf_num_frames_padded": (_i64, [_i64, _i32, _i32, _i32]),
    "ktf_frontend_f32": (C.c_int, [_P, _i64, _i64, _i32, C.POINTER(FrontendCfg), C.POINTER(FrontendTables), _i32, _P, _P, _u64, _P]),
    "ktf_frontend_plan": (C.c_int, [_i64, _i64, _i32, C.POINTER(FrontendCfg), C.POINTER(FrontendTables), _i32, C.POINTER(FrontendPlan)]),
    "ktf_dct_f32": (C.c_int, [_P, _i64, _i32, _i32, _P, _P, _P, _P]),
    "ktf_vad_mask_f32": (C.c_int, [_P, _i64, _i64, _i32, C.POINTER(VadCfg), _P, _P]),
    "ktf_vad_index": (C.c_int, [_P, _i64, _i64, _i32, C.POINTER(VadCfg), _P, _P, _P]),
    "ktf_cmvn_f32": (C.c_int, [_P, _i64, _i64, _i32, _i64, _P, C.POINTER(CmvnCfg), _P, _i64, _P, _P, _P]),
    "ktf_vad_cmvn": (C.c_int, [_P, _i64, _i64, _i32, C.POINTER(VadCfg), C.POINTER(CmvnCfg), _P, _i32, _i64, _P, _P, _P, _P]),
    "ktf_vad_cmvn_plan": (C.c_int, [_i64, _i64, _i32, _i64, C.POINTER(VcPlan)]),
    "ktf_cmvn_plan": (C.c_int, [_i64, _i32, _i64, C.POINTER(VcPlan)]),
    "ktf_route_short": (C.c_int, [_P, _i64, _i32, _P, _P, _P, _i32, _P]),
    "ktf_tdnn_out_len": (_i64, [_i64, C.POINTER(TdnnDesc)]),
    "ktf_tdnn_out_lens": (C.c_int, [_P, _i64, C.POINTER(TdnnDesc), _P, _P]),
    "ktf_tdnn_last_kernel": (C.c_char_p, []),
    "ktf_tdnn": (C.c_int, [_P, _i64, _i64, _i64, _P, C.POINTER(TdnnDesc), _P, _P, _P, _P, _P, _P, _i64, _P, _P]),
    "ktf_tdnn_stats": (C.c_int, [_P, _i64, _i64, _i64, _P, C.POINTER(TdnnDesc), _P, _P, _P, _P, _P, _P, _P]),
    "ktf_tdnn_split": (C.c_int, [_P, _P, _i64, _i64, _i64, _P, C.POINTER(TdnnDesc), _P, _P, _P, _P, _P, _P, _P, _i64, _P, _P]),
    "ktf_tdnn_split_flat": (C.c_int, [_P, _P, _i64, _i64, _i64, _P, _P, C.POINTER(TdnnDesc), _P, _P, _P, _P, _P, _P, _P, _i64, _P]),
    "ktf_tdnn_split_stats": (C.c_int, [_P, _P, _i64, _i64, _i64, _P, C.POINTER(TdnnDesc), _P, _P, _P, _P, _P, _P, _P]),
    "ktf_tdnn_split_flat_stats": (C.c_int, [_P, _P, _i64, _i64, _i64, _P, _P, C.POINTER(TdnnDesc), _P, _P, _P, _P, _P, _P, _P]),
    "ktf_flat_row_map_rows": (_i64, [_i64, _i64]),
    "ktf_flat_row_map": (C.c_int, [_P, _i64, _i64, _P, _P]),
    "ktf_flat_stats_slots": (_i64, [_i64]),
    "ktf_stats_finalize_flat": (C.c_int, [_P, _i64, _P, _i64, _i64, _i32, _i32, _f32, _P, _i64, _P]),
    "ktf_split_bf16": (C.c_int, [_P, _i64, _i32, _i64, _P, _P, _i64, _P]),
    "ktf_split_bf16_rows": (C.c_int, [_P, _i64, _i64, _i32, _i64, _P, _P, _P, _i64, _P]),
    "ktf_mx_planes": (C.c_int, [_P, _i64, _i64, _i32, _i64, _P, _P, _P, _P, _P, _P]),
    "ktf_tdnn_mx": (C.c_int, [_P, _P, _P, _P, _i64, _i64, _P, C.POINTER(TdnnDesc), _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _i64, _P]),
    "ktf_tdnn_mx_flat": (C.c_int, [_P, _P, _P, _P, _i64, _i64, _P, _P, C.POINTER(TdnnDesc), _P, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    "ktf_tdnn_mx_flat_stats": (C.c_int, [_P, _P, _P, _P, _i64, _i64, _P, _P, C.POINTER(TdnnDesc), _P, _P, _P, _P, _P, _P, _P]),
    "ktf_tdnn_mx_stats": (C.c_int, [_P, _P, _P, _P, _i64, _i64, _P, C.POINTER(TdnnDesc), _P, _P, _P, _P, _P, _P, _P]),
    "ktf_stats_finalize": (C.c_int, [_P, _P, _i64, _i64, _i32, _i32, _f32, _P, _i64, _P]),
    "ktf_stats_slots": (_i64, [_i64]),
    "ktf_tdnn_stats_slots": (_i64, [_i64, _i32]),
    "ktf_tdnn_slot_rows": (_i32, [_i32]),
    "ktf_mx_stats_slots": (_i64, [_i64, _i32]),
    "ktf_mx_slot_rows": (_i32, [_i32]),
    "ktf_stats_finalize_slots": (C.c_int, [_P, _i64, _i32, _P, _i64, _i64, _i32, _i32, _f32, _P, _i64, _P]),
    "ktf_affine_act_f32": (C.c_int, [_P, _i64, _i32, _i32, _P, _P, _P, _P]),
    "ktf_activation_f32": (C.c_int, [_P, _i64, _i64, _i32, _i64, _P, _i32, _P, _P, _P]),
    "ktf_convert_pad": (C.c_int, [_P, _i32, _i64, _i32, _i64, _P, _i32, _i64, _P]),
    "ktf_stats_pool": (C.c_int, [_P, _i32, _i64, _i64, _i32, _i64, _P, _i32, _i32, _f32, _P, _i64, _P]),
    "ktf_stats_pool_windowed_f32": (C.c_int, [_P, _i64, _i64, _i32, _i32, _i32, _i32, _i32, _i32, _i64, _i32, _f32, _P, _P]),
    "ktf_xvec_post_f32": (C.c_int, [_P, _i64, _i32, _i32, _P, _P, _P, _P, _P]),
    "ktf_xvec_tail_f32": (C.c_int, [_P, _i64, _P, _i64, _i32, _P, _i64, _i64, _i32, _i32, _f32, _P, _i64, _P, _i32, _P, _P, _P, _i32, _P, _P, _P, _P, _i32, _i32, _P]),
    "ktf_plda_f64": (C.c_int, [_P, _i64, _i32, _P, _P, _P, _i32, _i32, _P, _P, _P]),
    "ktf_plda_f32": (C.c_int, [_P, _i64, _i32, _P, _P, _P, _i32, _i32, _P, _P, _P]),
    "ktf_plda_score_f64": (C.c_int, [_P, _i64, _P, _i64, _i32, _P, _P, _P]),
    "ktf_plda_score_f32": (C.c_int, [_P, _i64, _P, _i64, _i32, _P, _P, _P]),
    "ktf_spk_mean_f32": (C.c_int, [_P, _i64, _i32, _P, _i64, _P, _i64, _P, _P, _P]),
    "ktf_plda_transform_n_f64": (C.c_int, [_P, _i64, _i32, _P, _P, _P, _P, _i32, _i32, _P, _P]),
    "ktf_plda_transform_n_f32": (C.c_int, [_P, _i64, _i32, _P, _P, _P, _P, _i32, _i32, _P, _P]),
    "ktf_plda_score_n_f64": (C.c_int, [_P, _i64, _P, _i64, _i32, _P, _P, _P, _P]),
    "ktf_plda_score_n_f32": (C.c_int, [_P, _i64, _P, _i64, _i32, _P, _P, _P, _P]),
    "ktf_plda_trials_workspace_bytes": (_i64, [_i64, _i64, _i32, _i32]),
    "ktf_plda_trials_f64": (C.c_int, [_P, _i64, _P, _i64, _i32, _P, _P, _P, _i64, _P, _P, C.c_size_t, _P]),
    "ktf_plda_trials_f32": (C.c_int, [_P, _i64, _P, _i64, _i32, _P, _P, _P, _i64, _P, _P, C.c_size_t, _P]),
    "ktf_topn_stats_f64": (C.c_int, [_P, _i64, _i64, _i64, _i32, _P, _P, _P]),
    "ktf_topn_stats_f32": (C.c_int, [_P, _i64, _i64, _i64, _i32, _P, _P, _P]),
    "ktf_plda_cohort_workspace_bytes": (_i64, [_i64, _i64, _i32, _i32]),
    "ktf_plda_cohort_stats_f64": (C.c_int, [_P, _i64, _P, _i64, _i32, _P, _P, _i32, _i32, _P, _P, _P, C.c_size_t, _P]),
    "ktf_plda_cohort_stats_f32": (C.c_int, [_P, _i64, _P, _i64, _i32, _P, _P, _i32, _i32, _P, _P, _P, C.c_size_t, _P]),
    "ktf_plda_dense_workspace_bytes": (_i64, [_P, _i32, _i32, C.c_double]),
    "ktf_plda_dense_f64": (C.c_int, [_P, _i64, _i32, _P, _P, _i32, C.c_double, _P, _P, _P, _P, _P, _P, _i32, _i32, _P, _P, _P,
                                     C.c_size_t, _P, _P]),
    "ktf_plda_dense_f32": (C.c_int, [_P, _i64, _i32, _P, _P, _i32, C.c_double, _P, _P, _P, _P, _P, _P, _i32, _i32, _P, _P, _P,
                                     C.c_size_t, _P, _P]),
    "ktf_ahc_workspace_bytes": (_i64, [_P, _i32, _i32]),
    "ktf_ahc_f64": (C.c_int, [_P, _P, _P, _i32, _i32, C.c_double, _P, C.c_double, _P, _P, _P, C.c_size_t, _P]),
    "ktf_ahc_f32": (C.c_int, [_P, _P, _P, _i32, _i32, C.c_double, _P, C.c_double, _P, _P, _P, C.c_size_t, _P]),
    "ktf_diar_segments": (C.c_int, [_P, _i32, _P, _P, _i32, C.POINTER(VadCfg), _P, _P, _P]),
    "ktf_diar_windows": (C.c_int, [_P, _P, _P, _i32, _i32, _i32, _i32, _P, _P, _P]),
    "ktf_diar_compact": (C.c_int, [_P, _P, _P, _P, _P, _i32, _i64, _i64, _P, _P, _P]),
    "ktf_diar_segment_cmn": (C.c_int, [_P, _i32, _P, _P, _i32, _P, _i64, C.POINTER(CmvnCfg), _P, _P, _P]),
    "ktf_diar_gather": (C.c_int, [_P, _i32, _P, _P, _i32, _P, _i64, _i64, _i64, _i32, _P, _i32, _i32, _P, _P]),
    "ktf_ivector_post_f32": (C.c_int, [_P, _i64, _i32, _i64, _P, _P, _i32, _i32, _f32, _P, _P, _P]),
    "ktf_ivector_workspace_bytes": (_i64, [_i32, _i32, _i32, _i32]),
    "ktf_ivector_extract": (C.c_int, [_P, _i64, _i32, _i64, _P, _i32, _P, _P, _i32, _f32, _f32, _f32, _P, _P, _i32, _i32, C.c_double,
                                      _P, _i32, _P, C.c_size_t, _P]),
    "ktf_ivector_train_workspace_bytes": (_i64, [_i32, _i32, _i32, _i32]),
    "ktf_ivector_acc_stats": (C.c_int, [_P, _i64, _i32, _i64, _P, _i32, _P, _P, _i32, _f32, _P, _P, _i32, _i32, C.c_double, _P, _P, _P, _P,
                                        _P, _P, _P, C.c_size_t, _P]),
    "ktf_ivector_acc2_workspace_bytes": (_i64, [_i64, _i32, _i32]),
    "ktf_ivector_acc_second_order": (C.c_int, [_P, _i64, _i32, _i64, _P, _P, _i32, _f32, _i32, _P, _P, C.c_size_t, _P]),
    "ktf_atb_f64": (C.c_int, [_P, _i64, _P, _i64, _P, _i64, _i64, _i64, _i64, _P]),
    "ktf_fgmm_workspace_bytes": (_i64, [_i64, _i32, _i32, _i32]),
    "ktf_fgmm_post_f32": (C.c_int, [_P, _i64, _i32, _i64, _P, _i32, _P, _P, _P, _i32, _f32, _P, _P, _P, C.c_size_t, _P]),
    "ktf_fgmm_post_ll_f32": (C.c_int, [_P, _i64, _i32, _i64, _P, _i32, _P, _P, _P, _i32, _f32, _P, _P, _P, _P, C.c_size_t, _P]),
    "ktf_gmm_post_preselect_f32": (C.c_int, [_P, _i64, _i32, _i64, _P, _i32, _P, _P, _P, _i32, _P, _P, _P, _P]),
    "ktf_gmm_post_dense_workspace_bytes": (_i64, [_i64, _i32]),
    "ktf_gmm_post_dense_f32": (C.c_int, [_P, _i64, _i32, _i64, _P, _P, _i32, _P, _P, _P, _P, C.c_size_t, _P]),
    "ktf_gmm_acc_workspace_bytes": (_i64, [_i64, _i32, _i32, _i32, _i32]),
    "ktf_gmm_acc_f64": (C.c_int, [_P, _i64, _i32, _i64, _P, _P, _i32, _i32, _i32, _P, _P, _P, _P, C.c_size_t, _P]),
    "ktf_add_deltas_f32": (C.c_int, [_P, _i64, _i64, _i32, _i64, _i64, _P, _P, _i32, _i32, _P, _P]),
    "ktf_train_class_means": (C.c_int, [_P, _i64, _i32, _P, _i64, _P, _i64, _P, _P, _P]),
    "ktf_train_workspace_bytes": (_i64, [_i64, _i32]),
    "ktf_train_mean_f32": (C.c_int, [_P, _i64, _i32, _P, _P, C.c_size_t, _P]),
    "ktf_train_mean_f64": (C.c_int, [_P, _i64, _i32, _P, _P, C.c_size_t, _P]),
    "ktf_train_gram_f32": (C.c_int, [_P, _i64, _i32, _P, _i64, _P, _P, _P, _P, C.c_size_t, _P]),
    "ktf_train_gram_f64": (C.c_int, [_P, _i64, _i32, _P, _i64, _P, _P, _P, _P, C.c_size_t, _P]),
    "ktf_plda_em_project": (C.c_int, [_P, _i64, _i32, _P, _P, _P, _P, _P, _P, _P]),
    "ktf_vb_post_workspace_bytes": (_i64, [_i64, _i32]),
    "ktf_vb_post_f32": (C.c_int, [_P, _i64, _i32, _i64, _P, _P, _i32, _i32, _f32, _f32, _f32, _P, _P, _P, _P, _P, C.c_size_t, _P]),
    "ktf_vb_bucket_workspace_bytes": (_i64, [_i64, _i32, _i32]),
    "ktf_vb_bucket": (C.c_int, [_P, _i64, _i32, _i32, _P, _P, _P, C.c_size_t, _P]),
    "ktf_vb_speaker_stats": (C.c_int, [_P, _i64, _i32, _i64, _P, _P, _i32, _i64, _i32, _P, _i32, _P, _P, _i32, _P, _P, _i32, _P, _P, _P]),
    "ktf_vb_update_workspace_bytes": (_i64, [_i32, _i32, _i32, _i32]),
    "ktf_vb_speaker_update": (C.c_int, [_P, _P, _i32, _i32, _i32, _i32, _P, _P, _P, _P, _P, _P, _P, _P, C.c_size_t, _P]),
    "ktf_vb_block_loglike": (C.c_int, [_P, _i64, _i32, _i64, _P, _P, _i32, _i64, _i32, _P, _P, _i32, _i32, _P, _P, _P, _i32, _P, _P]),
    "ktf_vb_fb_workspace_bytes": (_i64, [_i64, _i32]),
    "ktf_vb_forward_backward": (C.c_int, [_P, _P, _i32, _i64, _i32, _P, C.c_double, _P, _P, _P, _P, C.c_size_t, _P]),
    "ktf_vb_fb_serial_workspace_bytes": (_i64, [_i64, _i32]),
    "ktf_vb_forward_backward_serial": (C.c_int, [_P, _P, _i32, _i64, _i32, _P, C.c_double, _P, _P, _P, _P, C.c_size_t, _P]),
    "ktf_vb_loglike_sums": (C.c_int, [_P, _P, _i32, _i64, _P, _P]),
    "ktf_vb_bound": (C.c_int, [_P, _P, _P, _i32, _i32, C.c_double, _P, _P]),
    "ktf_vbx_prepare": (C.c_int, [_P, _i64, _i32, _P, _P, _P, _P]),
    "ktf_vbx_update_workspace_bytes": (_i64, [_i64, _i32, _i32]),
    "ktf_vbx_speaker_update": (C.c_int, [_P, _P, _i64, _i32, _i32, _P, _i32, _P, C.c_double, _P, _P, _P, _P, _P, C.c_size_t, _P]),
    "ktf_vbx_loglike": (C.c_int, [_P, _P, _i64, _i32, _i32, _P, _i32, _P, _P, C.c_double, _P, _P]),
}
# name -> (restype, argtypes); mirrors include/ktf_augment.h one to one (a table of its own: PROTOTYPES is ktf_hip.h's)
AUGMENT_PROTOTYPES = {
    "ktf_aug_partition": (_i32, []),
    "ktf_aug_tables_floats": (_i64, []),
    "ktf_aug_tables": (C.c_int, [_P, _P]),
    "ktf_aug_rir_spectra_floats": (_i64, [_P, _i32, _i32]),
    "ktf_aug_rir_prepare": (C.c_int, [_P, _P, _P, _i32, _i32, _P, _P, _P, _P]),
    "ktf_aug_workspace_bytes": (_i64, [_P, _P, _i32, _P, _i32, _i32, _i64]),
    "ktf_aug_convolve": (C.c_int, [_P, _i32, _i64, _P, _P, _P, _P, _i32, _P, _i32, _i32, _P, _P, _P, _P, _P, _i64, _P, _P, C.c_size_t,
                                   _P]),
    "ktf_aug_mix": (C.c_int, [_P, _P, _P, _P, _i32, _P, _i32, _i32, _P, _P, _P, _P, _P, _P, _P, _P, _i32, _i32, _i32, C.c_double, _P,
                              _i32, _i64, _i64, _P, _P, C.c_size_t, _P]),
}
# name -> (restype, argtypes); mirrors include/ktf_resample.h one to one
RESAMPLE_PROTOTYPES = {
    "ktf_rs_tile": (_i32, []),
    "ktf_rs_plan_sizes": (C.c_int, [_i32, _i32, C.c_double, _i32, _P, _P, _P]),
    "ktf_rs_plan": (C.c_int, [_i32, _i32, C.c_double, _i32, _P, _P, _P, _i32]),
    "ktf_rs_num_out": (_i64, [_i64, _i32, _i32]),
    "ktf_rs_resample": (C.c_int, [_P, _i32, _i64, _P, _P, _i32, _i32, _i32, _P, _P, _P, _P, _P, _i32, _P, _i32, _i64, _i64, _P]),
}
# name -> (restype, argtypes); mirrors include/ktf_grad.h one to one
GRAD_PROTOTYPES = {
    "ktf_grad_tdnn_row_tile": (_i32, []),
    "ktf_grad_tdnn_slot_rows": (_i32, []),
    "ktf_grad_tdnn_workspace_bytes": (_i64, [_i64, _i64, C.POINTER(TdnnDesc)]),
    "ktf_grad_tdnn_data": (C.c_int, [_P, _i64, _i64, _i64, _P, C.POINTER(TdnnDesc), _P, _P, _i64, _P, C.c_size_t, _P]),
    "ktf_grad_tdnn_weights": (C.c_int, [_P, _i64, _i64, _i64, _P, C.POINTER(TdnnDesc), _P, _i64, _P, _P, _P, C.c_size_t, _P]),
    "ktf_grad_stats_pool": (C.c_int, [_P, _i64, _i64, _i32, _i64, _P, _i32, _i32, _f32, _P, _i64, _P, _i64, _P]),
    "ktf_grad_tdnn16_workspace_bytes": (_i64, [_i64, _i64, C.POINTER(TdnnDesc), _i32]),
    "ktf_grad_tdnn16_data": (C.c_int, [_P, _i64, _i64, _i64, _P, C.POINTER(TdnnDesc), _P, _P, _i64, _P, C.c_size_t, _i32, _P]),
    "ktf_grad_tdnn16_weights": (C.c_int, [_P, _i64, _i64, _i64, _P, C.POINTER(TdnnDesc), _P, _i64, _P, _P, _P, C.c_size_t, _i32, _P]),
}
# name -> (restype, argtypes); mirrors include/ktf_norm.h one to one
NORM_PROTOTYPES = {
    "ktf_norm_slot_rows": (_i32, []),
    "ktf_norm_workspace_bytes": (_i64, [_i64, _i64, _i32]),
    "ktf_norm_relu_bn_forward": (C.c_int, [_P, _i64, _i64, _i64, _i32, _P, _i32, _i32, _P, _P, _P, C.c_double, C.c_double, _P, _i64, _P, _P,
                                           C.c_size_t, _P]),
    "ktf_norm_relu_bn_backward": (C.c_int, [_P, _i64, _P, _i64, _i64, _i64, _i32, _P, _i32, _i32, _P, _P, _P, _i64, _P, _P, C.c_size_t, _P]),
}
# name -> (restype, argtypes); mirrors include/ktf_loss.h one to one
LOSS_PROTOTYPES = {
    "ktf_loss_slot_rows": (_i32, []),
    "ktf_loss_workspace_bytes": (_i64, [_i64, _i64]),
    "ktf_loss_row_inv_norm": (C.c_int, [_P, _i64, _i64, _i64, C.c_double, _P, _P]),
    "ktf_loss_row_inv_norm_backward": (C.c_int, [_P, _i64, _i64, _i64, C.c_double, _P, _P, _P, _i64, _P]),
    "ktf_loss_margin_softmax_forward": (C.c_int, [_P, _i64, _i64, _i64, _P, _P, _P, _i32, C.c_double, C.c_double, _P, _P, _P, _P, C.c_size_t,
                                                  _P]),
    "ktf_loss_margin_softmax_backward": (C.c_int, [_P, _i64, _i64, _i64, _P, _P, _P, _i32, C.c_double, C.c_double, _P, _P, _P, _i64, _P, _P, _P,
                                                   C.c_size_t, _P]),
}
# name -> (restype, argtypes); mirrors include/ktf_egs.h one to one
_U32P = C.POINTER(C.c_uint32)
EGS_PROTOTYPES = {
    "ktf_egs_philox": (C.c_int, [_U32P, _U32P, _U32P]),
    "ktf_egs_draw": (C.c_int, [C.POINTER(EgsIndex), _i64, _i64, _i64, _u64, _u64, _i64, _i64, _i64, _i64, _P, _P, _P, _P]),
    "ktf_egs_gather": (C.c_int, [_P, _i32, _i64, _i64, _i64, _P, _P, _i64, _P, _P, _i64, _i64, _P, _i64, _P]),
    "ktf_egs_sample": (C.c_int, [C.POINTER(EgsIndex), _i64, _i64, _i64, _u64, _u64, _i64, _i64, _i64, _i64, _P, _i32, _i64, _i64, _i64, _P, _P,
                                 _P, _i64, _P, _P, _P, _P]),
}
# name -> (restype, argtypes); mirrors include/ktf_optim.h one to one
OPTIM_PROTOTYPES = {
    "ktf_optim_slot_elems": (_i64, []),
    "ktf_optim_workspace_bytes": (_i64, [_i64, _i32]),
    "ktf_optim_step": (C.c_int, [_P, _P, _P, _P, _i64, _P, _P, _i32, _P, _i32, _i32, C.c_double, _i32, C.c_double, C.c_double, C.c_double,
                                 _i64, _i32, C.c_double, C.c_double, _P, _P, C.c_size_t, _P]),
}
# name -> (restype, argtypes); mirrors include/ktf_head.h one to one
HEAD_PROTOTYPES = {
    "ktf_head_slot_rows": (_i32, []),
    "ktf_head_workspace_bytes": (_i64, [_i64, _i64, _i64]),
    "ktf_head_forward": (C.c_int, [_P, _i64, _i64, _i64, _i64, _P, _P, _P, _i32, C.c_double, C.c_double, _i32, C.c_double, C.c_double, _P, _P,
                                   _P, _P, _P, _P, C.c_size_t, _P]),
    "ktf_head_backward": (C.c_int, [_P, _i64, _i64, _i64, _i64, _P, _P, _P, _i32, C.c_double, C.c_double, _i32, C.c_double, C.c_double, _P, _P,
                                    _P, _P, _i64, _P, _P, _P, C.c_size_t, _P]),
}
# name -> (restype, argtypes); mirrors include/ktf_attn.h one to one
ATTN_PROTOTYPES = {
    "ktf_attn_pool": (C.c_int, [_P, _i64, _i64, _i32, _i64, _P, _i32, _i64, _P, _i32, _f32, _P, _i64, _P, _P, _P]),
    "ktf_attn_pool_backward_workspace_bytes": (_i64, [_i64, _i32, _i32]),
    "ktf_attn_pool_backward": (C.c_int, [_P, _i64, _i64, _i32, _i64, _P, _i32, _i64, _P, _i32, _f32, _P, _P, _P, _i64, _P, _i64, _P, _i64, _P,
                                         C.c_size_t, _P]),
}
ATTN_MAX_BATCH, ATTN_MAX_ROWS, ATTN_MAX_DIM = 65535, 1 << 30, 1 << 20   # ktf_attn_*: utterances, frames and channels per call
HEAD_MAX_CENTERS, HEAD_MAX_TOPK = 8, 64   # ktf_head_*: sub-centres per class; penalised classes per row
OPTIM_SGD, OPTIM_ADAM, OPTIM_MAX_GROUPS = 0, 1, 8   # ktf_optim_*: kind; groups per call
EGS_THREADS, EGS_MAX_SLICES = 256, 32   # ktf_egs_*: threads of a workgroup; workgroups per batch row at most
LOSS_SOFTMAX, LOSS_AM, LOSS_AAM = 0, 1, 2   # ktf_loss_*: kind
LOSS_SIN2_FLOOR = 2.0 ** -20
AUG_META, AUG_STATS = 8, 4         # ktf_aug_*: int32 per RIR of the bank's meta; doubles per row of the statistics
PLDA_DENSE_NO_PCA = -1.0            # ktf_plda_dense_*: target_energy for "no PCA"
PLDA_DENSE_MAX_DIM = 512
PLDA_DENSE_MAX_SWEEPS = 30
AHC_MAX_N = 32767                   # ktf_ahc_*: rows per recording
AHC_LDS_SLOTS = 5120                # ... up to which the merge loop's state sits in LDS
IVECTOR_MAX_FEAT_DIM, IVECTOR_MAX_GAUSS, IVECTOR_MAX_GSELECT, IVECTOR_MAX_DIM = 128, 8192, 64, 1024   # ktf_ivector_*
GMM_ACC_ITEM_ROWS = 1024            # ktf_gmm_acc_f64: rows of a bucket per item
ADD_DELTAS_MAX_CONTEXT = 32         # ktf_add_deltas_f32: order * window
TRAIN_MAX_DIM = 1024                # ktf_train_*, ktf_plda_em_project
VB_MAX_SPEAKERS, VB_FB_CHUNK = 16, 128   # ktf_vb_*: speakers per recording, blocks per chunk of the forward-backward scan
VBX_MAX_DIM, VBX_UPDATE_ROWS = 512, 256  # ktf_vbx_*: dimensions; windows per workgroup of the speaker update
RS_MAX_SAMPLES = 1 << 30            # ktf_rs_*: samples per row, in or out

_lib = None


def load():
    """dlopen libktf_hip.so and bind every symbol of the headers. Raises if it is missing."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise KtfBackendError(
            f"{LIB_PATH} not found: build it with `make -C kaldi-tflite_amd/csrc` (or __graft_entry__.build()). "
            "There is no CPU fallback.")
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in (list(PROTOTYPES.items()) + list(AUGMENT_PROTOTYPES.items()) + list(RESAMPLE_PROTOTYPES.items())
                              + list(GRAD_PROTOTYPES.items()) + list(NORM_PROTOTYPES.items()) + list(LOSS_PROTOTYPES.items())
                              + list(EGS_PROTOTYPES.items()) + list(OPTIM_PROTOTYPES.items()) + list(HEAD_PROTOTYPES.items())
                              + list(ATTN_PROTOTYPES.items())):
        fn = getattr(lib, name)          # AttributeError = header/library mismatch
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def last_error():
    lib = load()
    buf = C.create_string_buffer(512)
    lib.ktf_last_error(buf, 512)
    return buf.value.decode(errors="replace")


def check(rc, what):
    """Map the C return code to the reference's exception convention (ValueError for bad arguments)."""
    if rc == 0:
        return
    msg = last_error()
    if rc == -1:
        raise ValueError(msg or what)
    if rc == -3:
        raise NotImplementedError(msg or what)
    raise KtfBackendError(f"{what}: rc={rc}: {msg}")


def require_gpu():
    import torch
    if not torch.cuda.is_available():
        raise KtfBackendError("no MI355X / ROCm device visible: kaldi_tflite_amd computes only on the GPU (no CPU fallback)")
    load()


class _Scope(threading.local):
    dev = None          # device index the enclosing launch_scope made current
    stream = None       # ... and its current stream at entry, as a c_void_p


_scope = _Scope()


class launch_scope:
    """One extraction = ~10 launches on one device and one stream: looked up once here instead of once per launch (torch's
    current_stream / device context managers were a quarter of the host time of a batch-1 call). Inside the scope `on_device(d)` is a
    no-op for the scope's device and `stream_ptr()` returns the stream that was current at entry; nested scopes fall back to the
    per-call lookups, and `on_device(another device)` suspends the scope (device and stream) until it exits. Code that switches streams must do so OUTSIDE (as extract_stream does)."""

    def __init__(self, device):
        import torch
        self.device = torch.device(device)
        self.ctx = None
        self.outer = None

    def __enter__(self):
        import torch
        self.outer = (_scope.dev, _scope.stream)
        idx = self.device.index if self.device.index is not None else torch.cuda.current_device()
        if _scope.dev != idx:
            self.ctx = torch.cuda.device(idx)
            self.ctx.__enter__()
        _scope.dev = idx
        _scope.stream = C.c_void_p(torch.cuda.current_stream(idx).cuda_stream)
        return self

    def __exit__(self, *exc):
        _scope.dev, _scope.stream = self.outer
        if self.ctx is not None:
            self.ctx.__exit__(*exc)
        return False


class _Noop:
    def __enter__(self):
        return self

    def __exit__(self, *exc):
        return False


_NOOP = _Noop()


class _OtherDevice:
    """`on_device(d)` for a device that is not the enclosing launch_scope's: makes it current and hides the scope's cached stream
    for the duration -- that stream belongs to the scope's device, and `stream_ptr()` must hand the call the target device's
    current stream (an invalid handle or a launch on the wrong queue otherwise)."""

    def __init__(self, device):
        import torch
        self.ctx = torch.cuda.device(device)
        self.saved = None

    def __enter__(self):
        self.saved = (_scope.dev, _scope.stream)
        _scope.dev, _scope.stream = None, None
        self.ctx.__enter__()
        return self

    def __exit__(self, *exc):
        self.ctx.__exit__(*exc)
        _scope.dev, _scope.stream = self.saved
        return False


def on_device(device):
    """`with on_device(t.device):` around a library call: makes the device current (torch.cuda.device), unless an enclosing
    launch_scope already did; for any other device the scope is suspended (its cached stream is not that device's)."""
    import torch
    idx = device.index if isinstance(device, torch.device) else device
    if _scope.dev is not None and (idx is None or idx == _scope.dev):
        return _NOOP
    if _scope.dev is not None:
        return _OtherDevice(device)
    return torch.cuda.device(device)


def stream_ptr():
    if _scope.stream is not None:
        return _scope.stream
    import torch
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def ptr(t):
    """device pointer of a torch tensor (or None)."""
    if t is None:
        return None
    return C.c_void_p(t.data_ptr())
