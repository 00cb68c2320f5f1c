"""ctypes binding of libhsp.so (the C ABI declared in include/hsp.h).

The product path has no CPU or eager fallback: if the shared library is missing, or a
tensor is not an fp32 tensor on a ROCm device, the call raises.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("HSP_LIB", os.path.join(_HERE, "libhsp.so"))  # HSP_LIB: kernel A/B builds

# enums of include/hsp.h
PRO_NONE, PRO_LRELU, PRO_ACT1D, PRO_SILU = 0, 1, 2, 3
ACT_NONE, ACT_TANH, ACT_GELU_TANH, ACT_RELU, ACT_MISH, ACT_SILU, ACT_SOFTPLUS, ACT_GELU_ERF = 0, 1, 2, 3, 4, 5, 6, 7
ACT_ACT1D = 8          # the next Activation1d from the conv epilogue (hsp.h: HSP_ACT_ACT1D)
ROWS_PLAIN, ROWS_GATE_WN, ROWS_GATE_GLU, ROWS_SHUFFLE = 0, 1, 2, 3
MASK_NONE, MASK_PRE, MASK_POST, MASK_BOTH = 0, 1, 2, 3
EINVAL = -1
MHA_TOK, MHA_MFMA_WHOLE, MHA_MFMA_SLAB, MHA_MFMA_STREAM, MHA_ROW, MHA_ROW_STREAM = range(6)   # hsp_mha_plan kernel ids

_fp = C.c_void_p


class Conv1dArgs(C.Structure):
    """Mirror of ``hsp_conv1d_args`` (include/hsp.h) -- field order is the ABI."""
    _fields_ = [
        ("x", _fp), ("x_bs", C.c_int64), ("x_cs", C.c_int64), ("x_ts", C.c_int64),
        ("B", C.c_int32), ("Cin", C.c_int32), ("Lin", C.c_int32),
        ("w", _fp), ("K", C.c_int32), ("M", C.c_int32), ("dil", C.c_int32), ("pad", C.c_int32), ("stride", C.c_int32),
        ("zeros", _fp), ("w_ld", C.c_int32),
        ("y", _fp), ("y_bs", C.c_int64), ("y_cs", C.c_int64),
        ("Cout", C.c_int32), ("Lout", C.c_int32), ("ncols", C.c_int32),
        ("prologue", C.c_int32), ("slope", C.c_float),
        ("alpha_exp", _fp), ("beta_inv", _fp), ("filt", _fp),
        ("rows", C.c_int32), ("gate_half", C.c_int32), ("up", C.c_int32), ("shuf_pad", C.c_int32),
        ("bias", _fp), ("cbias", _fp), ("cbias_bs", C.c_int64),
        ("act", C.c_int32),
        ("mask", _fp), ("mask_bs", C.c_int64), ("mask_mode", C.c_int32),
        ("cscale", _fp), ("cscale_bs", C.c_int64), ("scale", C.c_float),
        ("res", _fp), ("res_bs", C.c_int64), ("res_cs", C.c_int64),
        ("accumulate", C.c_int32), ("post_scale", C.c_float), ("debug", C.c_int32),
        ("ln_c1", _fp), ("ln_eps", C.c_float),
        ("split_row", C.c_int32), ("accumulate2", C.c_int32), ("mask_mode2", C.c_int32), ("y2", _fp),
        ("y2_bs", C.c_int64), ("y2_cs", C.c_int64), ("res_ts", C.c_int64), ("w_bs", C.c_int64),
        ("fold_cols", C.c_int32),
    ]


class MhaArgs(C.Structure):
    """Mirror of ``hsp_mha_args``."""
    _fields_ = [
        ("q", _fp), ("k", _fp), ("v", _fp), ("o", _fp),
        ("q_bs", C.c_int64), ("k_bs", C.c_int64), ("v_bs", C.c_int64), ("o_bs", C.c_int64),
        ("B", C.c_int32), ("H", C.c_int32), ("D", C.c_int32), ("Tq", C.c_int32), ("Tk", C.c_int32),
        ("qk_scale", C.c_float),
        ("mask_q", _fp), ("mask_k", _fp), ("rel_k", _fp), ("rel_v", _fp), ("window", C.c_int32),
        ("q_cs", C.c_int64), ("k_cs", C.c_int64), ("v_cs", C.c_int64), ("o_cs", C.c_int64),
        ("mask_dense", _fp), ("mask_dense_bs", C.c_int64),
    ]


class MhaProjArgs(C.Structure):
    """Mirror of ``hsp_mha_proj_args``."""
    _fields_ = [
        ("q", _fp), ("k", _fp), ("v", _fp),
        ("q_bs", C.c_int64), ("q_cs", C.c_int64), ("k_bs", C.c_int64), ("k_cs", C.c_int64), ("v_bs", C.c_int64),
        ("v_cs", C.c_int64),
        ("B", C.c_int32), ("H", C.c_int32), ("D", C.c_int32), ("Tq", C.c_int32), ("Tk", C.c_int32),
        ("qk_scale", C.c_float),
        ("wt", _fp), ("M", C.c_int32), ("wt_ld", C.c_int32),
        ("bias", _fp), ("mask", _fp), ("mask_bs", C.c_int64), ("cscale", _fp), ("cscale_bs", C.c_int64),
        ("res", _fp), ("res_bs", C.c_int64), ("res_cs", C.c_int64), ("res_ts", C.c_int64),
        ("y", _fp), ("y_bs", C.c_int64), ("y_cs", C.c_int64), ("y_ts", C.c_int64), ("debug", C.c_int32),
        ("key_len", _fp),
    ]


class DftSegArgs(C.Structure):
    """Mirror of ``hsp_dftseg_args``."""
    _fields_ = [
        ("x", _fp), ("x_bs", C.c_int64), ("x_cs", C.c_int64),
        ("y", _fp), ("y_bs", C.c_int64), ("y_cs", C.c_int64),
        ("B", C.c_int32), ("C", C.c_int32), ("L", C.c_int32),
        ("k", C.c_int32), ("dil", C.c_int32), ("pad", C.c_int32), ("nseg", C.c_int32), ("Np", C.c_int32),
        ("xf", _fp), ("xf_bs", C.c_int64), ("dft", _fp),
        ("bias", _fp), ("res", _fp), ("res_bs", C.c_int64), ("res_cs", C.c_int64),
        ("accumulate", C.c_int32), ("post_scale", C.c_float),
        ("act_alpha_exp", _fp), ("act_beta_inv", _fp), ("act_filt", _fp), ("prod3", C.c_int32),
        ("act_len", _fp),
    ]


class Cprod3Args(C.Structure):
    """Mirror of ``hsp_cprod3_args``."""
    _fields_ = [
        ("xf", _fp), ("yf", _fp), ("w", _fp), ("zeros", _fp), ("xf_bs", C.c_int64), ("yf_bs", C.c_int64),
        ("bins", C.c_int32), ("C", C.c_int32), ("Np", C.c_int32), ("debug", C.c_int32),
    ]


class SampleArgs(C.Structure):
    """Mirror of ``hsp_sample_args``."""
    _fields_ = [
        ("temperature", C.c_float), ("top_k", C.c_int32), ("top_p", C.c_float), ("repetition_penalty", C.c_float),
        ("seeds", _fp), ("probs", _fp), ("probs_bs", C.c_int64),
    ]


class PlmDecodeArgs(C.Structure):
    """Mirror of ``hsp_plm_decode_args``."""
    _fields_ = [
        ("x", _fp), ("x_bs", C.c_int64), ("x_cs", C.c_int64),
        ("y", _fp), ("y_bs", C.c_int64), ("y_cs", C.c_int64),
        ("k_cache", _fp), ("v_cache", _fp), ("bs", C.c_int64), ("cs", C.c_int64),
        ("t", C.c_int32), ("B", C.c_int32), ("D", C.c_int32), ("H", C.c_int32), ("F", C.c_int32), ("eps", C.c_float),
        ("g1", _fp), ("b1", _fp), ("wqkv_t", _fp), ("bqkv", _fp), ("wo_t", _fp), ("bo", _fp), ("g2", _fp), ("b2", _fp),
        ("w1_t", _fp), ("c1", _fp), ("w2_t", _fp), ("c2", _fp),
        ("workspace", _fp), ("workspace_bytes", C.c_int64), ("debug", C.c_int32),
    ]


class PlmPrefillAttnArgs(C.Structure):
    """Mirror of ``hsp_plm_prefill_attn_args``."""
    _fields_ = [
        ("qkv", _fp), ("q_rs", C.c_int64), ("out", _fp), ("o_rs", C.c_int64),
        ("k_cache", _fp), ("v_cache", _fp), ("cs", C.c_int64),
        ("n", C.c_int32), ("D", C.c_int32), ("H", C.c_int32), ("debug", C.c_int32),
    ]


class ProsodyArgs(C.Structure):
    """Mirror of ``hsp_prosody_args``."""
    _fields_ = [
        ("x", _fp), ("x_bs", C.c_int64), ("x_cs", C.c_int64), ("lengths", _fp),
        ("B", C.c_int32), ("D", C.c_int32), ("T", C.c_int32), ("k", C.c_int32), ("w_ld", C.c_int32), ("bins", C.c_int32),
        ("w1a", _fp), ("b1a", _fp), ("w1b", _fp), ("b1b", _fp), ("w2a", _fp), ("b2a", _fp), ("w2b", _fp), ("b2b", _fp),
        ("embed", _fp), ("codes", _fp), ("c_bs", C.c_int64), ("pooled", _fp), ("p_bs", C.c_int64),
    ]


class LimiterArgs(C.Structure):
    """Mirror of ``hsp_limiter_args``."""
    _fields_ = [
        ("x", _fp), ("x_bs", C.c_int64), ("lengths", _fp), ("gains", _fp), ("B", C.c_int32), ("n", C.c_int64),
        ("bank", _fp), ("F", C.c_int32), ("Z", C.c_int32), ("W", C.c_int32), ("ceiling", C.c_float),
        ("y", _fp), ("y_bs", C.c_int64), ("min_gain", _fp), ("tp", _fp),
    ]


class F0EditArgs(C.Structure):
    """Mirror of ``hsp_f0_edit_args``."""
    _fields_ = [
        ("lf0", _fp), ("lf0_bs", C.c_int64), ("lengths", _fp), ("B", C.c_int32), ("n", C.c_int64),
        ("shift", _fp), ("range", _fp), ("target_hz", _fp), ("offsets", _fp), ("off_bs", C.c_int64),
        ("f_min", C.c_float), ("f_max", C.c_float), ("out", _fp), ("out_bs", C.c_int64), ("mean_hz", _fp),
    ]


WSPEC_BLOCK, WSPEC_THREE = 0, 1


# symbol -> (restype, argtypes); every symbol include/hsp.h declares
SIGNATURES = {
    "hsp_version": (C.c_int, []),
    "hsp_arch": (C.c_char_p, []),
    "hsp_conv1d_mfma_f32": (C.c_int, [C.POINTER(Conv1dArgs), _fp]),
    "hsp_conv1d_direct_f32": (C.c_int, [C.POINTER(Conv1dArgs), _fp]),
    "hsp_conv1d_mfma_plan": (C.c_int, [C.POINTER(Conv1dArgs), C.POINTER(C.c_int32 * 4)]),
    "hsp_act1d_snakebeta_f32": (C.c_int, [_fp, _fp, C.c_int32, C.c_int32, C.c_int32, _fp, _fp, _fp, _fp]),
    "hsp_act1d_snakebeta_ragged_f32": (C.c_int, [_fp, _fp, C.c_int32, C.c_int32, C.c_int32, _fp, _fp, _fp, _fp, _fp]),
    "hsp_snake_consts_f32": (C.c_int, [_fp, _fp, _fp, _fp, C.c_int32, _fp]),
    "hsp_fold_weight_norm_f32": (C.c_int, [_fp, _fp, _fp, C.c_int32, C.c_int32, _fp]),
    "hsp_gather_f32": (C.c_int, [_fp, _fp, _fp, C.c_int64, _fp]),
    "hsp_sequence_mask_f32": (C.c_int, [_fp, _fp, C.c_int32, C.c_int32, _fp]),
    "hsp_flip_channels_f32": (C.c_int, [_fp, _fp, C.c_int32, C.c_int32, C.c_int32, _fp]),
    "hsp_sample_prior_f32": (C.c_int, [_fp, _fp, _fp, _fp, C.c_int32, C.c_int32, C.c_int32, C.c_float, _fp]),
    "hsp_randn_rows_f32": (C.c_int, [_fp, _fp, C.c_int32, C.c_int32, C.c_int32, _fp]),
    "hsp_sample_prior_seeded_f32": (C.c_int, [_fp, _fp, _fp, _fp, C.c_int32, C.c_int32, C.c_int32, C.c_float, _fp]),
    "hsp_layernorm_mod_f32": (C.c_int, [_fp, _fp, C.c_int32, C.c_int32, C.c_int32, C.c_float, _fp, _fp, _fp,
                                        C.c_int64, _fp, _fp, _fp]),
    "hsp_mha_f32": (C.c_int, [C.POINTER(MhaArgs), _fp]),
    "hsp_mha_plan": (C.c_int, [C.POINTER(MhaArgs), C.POINTER(C.c_int32 * 4)]),
    "hsp_mha_proj_f32": (C.c_int, [C.POINTER(MhaProjArgs), _fp]),
    "hsp_dftseg_fwd_f32": (C.c_int, [C.POINTER(DftSegArgs), _fp]),
    "hsp_dftseg_inv_f32": (C.c_int, [C.POINTER(DftSegArgs), _fp]),
    "hsp_dftseg_tables_f32": (C.c_int, [_fp, _fp]),
    "hsp_dftseg_pair_supported": (C.c_int, [C.POINTER(DftSegArgs), C.POINTER(DftSegArgs)]),
    "hsp_dftseg_pair_f32": (C.c_int, [C.POINTER(DftSegArgs), C.POINTER(DftSegArgs), _fp]),
    "hsp_dftseg_supported": (C.c_int, [C.POINTER(DftSegArgs)]),
    "hsp_cprod3_f32": (C.c_int, [C.POINTER(Cprod3Args), _fp]),
    "hsp_cprod3_supported": (C.c_int, [C.POINTER(Cprod3Args)]),
    "hsp_dftseg_weight_spectrum_f32": (C.c_int, [_fp, C.c_int32, C.c_int32, C.c_int32, _fp, _fp, C.c_int32, _fp]),
    "hsp_mha_proj_supported": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_int32]),
    "hsp_masked_mean_f32": (C.c_int, [_fp, _fp, _fp, C.c_int32, C.c_int32, C.c_int32, _fp]),
    "hsp_mask_mul_f32": (C.c_int, [_fp, _fp, _fp, C.c_int32, C.c_int32, C.c_int32, _fp]),
    "hsp_linear_interp_f32": (C.c_int, [_fp, _fp, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _fp]),
    "hsp_linear_interp_ragged_f32": (C.c_int, [_fp, _fp, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _fp, _fp, _fp]),
    "hsp_axpby_f32": (C.c_int, [_fp, _fp, _fp, C.c_float, C.c_float, C.c_int64, _fp]),
    "hsp_plm_embed_f32": (C.c_int, [_fp, C.c_int64, C.c_int64, C.c_int32, _fp, C.c_int64, _fp, C.c_int32, C.c_int32,
                                    _fp, C.c_int32, _fp, _fp, C.c_int64, C.c_int64, C.c_int32, C.c_int32, _fp]),
    "hsp_plm_embed_step_f32": (C.c_int, [_fp, C.c_int64, C.c_int64, C.c_int32, _fp, C.c_int64, _fp, C.c_int32, C.c_int32,
                                         _fp, C.c_int32, _fp, _fp, C.c_int64, C.c_int64, C.c_int32, C.c_int32, _fp, C.c_int64,
                                         C.c_int64, C.c_int32, _fp]),
    "hsp_argmax_f32": (C.c_int, [_fp, C.c_int64, C.c_int64, C.c_int32, C.c_int32, _fp, C.c_int64, _fp]),
    "hsp_plm_embed_sample_f32": (C.c_int, [_fp, C.c_int64, C.c_int64, C.c_int32, _fp, C.c_int64, _fp, C.c_int32,
                                           C.c_int32, _fp, C.c_int32, _fp, _fp, C.c_int64, C.c_int64, C.c_int32,
                                           C.c_int32, _fp, C.c_int64, C.c_int64, C.c_int32, C.c_int32,
                                           C.POINTER(SampleArgs), _fp]),
    "hsp_sample_f32": (C.c_int, [_fp, C.c_int64, C.c_int64, C.c_int32, C.c_int32, _fp, C.c_int64, C.c_int32,
                                 C.POINTER(SampleArgs), _fp]),
    "hsp_plm_decode_supported": (C.c_int, [C.c_int32, C.c_int32, C.c_int32]),
    "hsp_plm_decode_workspace_bytes": (C.c_int64, [C.c_int32, C.c_int32]),
    "hsp_plm_decode_layer_f32": (C.c_int, [C.POINTER(PlmDecodeArgs), _fp]),
    "hsp_plm_decode_layer_pos_f32": (C.c_int, [C.POINTER(PlmDecodeArgs), _fp, _fp]),
    "hsp_plm_embed_pos_f32": (C.c_int, [_fp, C.c_int64, C.c_int64, C.c_int32, _fp, C.c_int64, _fp, C.c_int32, C.c_int32,
                                        _fp, C.c_int32, _fp, _fp, C.c_int64, C.c_int64, C.c_int32, _fp, C.c_int32, _fp]),
    "hsp_plm_choose_advance_f32": (C.c_int, [_fp, C.c_int64, C.c_int64, C.c_int32, C.c_int32, _fp, C.c_int64, _fp, _fp,
                                             C.c_int32, C.POINTER(SampleArgs), _fp]),
    "hsp_plm_prefill_attn_supported": (C.c_int, [C.c_int32, C.c_int32]),
    "hsp_plm_prefill_attn_f32": (C.c_int, [C.POINTER(PlmPrefillAttnArgs), _fp]),
    "hsp_embedding_sum_f32": (C.c_int, [_fp, _fp, _fp, _fp, _fp, _fp, C.c_int32, C.c_int32, C.c_int32, C.c_float, _fp,
                                        C.c_int64, C.c_int64, C.c_int32, C.c_int32, C.c_int32, _fp]),
    "hsp_lstm_bidir_f32": (C.c_int, [_fp, C.c_int64, _fp, _fp, _fp, _fp, C.c_int64, C.c_int64, C.c_int32, C.c_int32,
                                     C.c_int32, _fp]),
    "hsp_duration_f32": (C.c_int, [_fp, C.c_int64, _fp, C.c_float, _fp, C.c_int64, _fp, C.c_int32, C.c_int32, _fp]),
    "hsp_duration_scaled_f32": (C.c_int, [_fp, C.c_int64, _fp, C.c_float, _fp, C.c_int64, _fp, C.c_int32, C.c_int32, _fp,
                                          C.c_int64, _fp]),
    "hsp_gaussian_upsample_f32": (C.c_int, [_fp, C.c_int64, C.c_int64, _fp, C.c_int64, _fp, C.c_int64, _fp, _fp, _fp,
                                            C.c_int32, C.c_int32, C.c_int32, C.c_int32, _fp]),
    "hsp_act_f32": (C.c_int, [_fp, _fp, C.c_int64, C.c_int32, _fp]),
    "hsp_reflect_pad_f32": (C.c_int, [_fp, C.c_int64, _fp, C.c_int32, C.c_int32, C.c_int32, _fp]),
    "hsp_f0_convert_f32": (C.c_int, [_fp, C.c_int32, _fp, C.c_int32, _fp, _fp]),
    "hsp_reflect_pad_ragged_f32": (C.c_int, [_fp, C.c_int64, _fp, _fp, C.c_int64, C.c_int32, C.c_int32, C.c_int32,
                                             C.c_int32, _fp]),
    "hsp_f0_convert_batch_f32": (C.c_int, [_fp, C.c_int64, _fp, _fp, C.c_int64, _fp, C.c_int32, _fp, C.c_int64, C.c_int32,
                                           C.c_int32, _fp]),
    "hsp_stft_frames_ragged_f32": (C.c_int, [_fp, C.c_int64, _fp, _fp, _fp, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                             C.c_int32, C.c_int32, _fp]),
    "hsp_abs_max_rows_f32": (C.c_int, [_fp, C.c_int64, _fp, _fp, C.c_int32, C.c_int64, _fp]),
    "hsp_peak_int16_gains": (C.c_int, [_fp, C.c_int64, _fp, _fp, _fp, C.c_int64, C.c_int32, C.c_int64, _fp]),
    "hsp_mag_pha_f32": (C.c_int, [_fp, C.c_int64, _fp, _fp, C.c_int32, C.c_int32, C.c_float, _fp]),
    "hsp_lsigmoid_mul_f32": (C.c_int, [_fp, _fp, C.c_float, _fp, _fp, C.c_int32, C.c_int32, _fp]),
    "hsp_atan2_f32": (C.c_int, [_fp, _fp, _fp, C.c_int64, _fp]),
    "hsp_polar_f32": (C.c_int, [_fp, _fp, C.c_float, _fp, C.c_int64, _fp, C.c_int64, C.c_int32, C.c_int32, _fp]),
    "hsp_norm_factor_rows_f32": (C.c_int, [_fp, C.c_int64, _fp, _fp, _fp, C.c_int32, C.c_int64, _fp]),
    "hsp_stft_frames_packed_f32": (C.c_int, [_fp, C.c_int64, _fp, _fp, _fp, _fp, _fp, _fp, C.c_int32, C.c_int64, C.c_int32,
                                             C.c_int32, C.c_int32, C.c_int32, _fp]),
    "hsp_instnorm_prelu_seg_f32": (C.c_int, [_fp, C.c_int64, C.c_int32, C.c_int32, C.c_int32, _fp, _fp, C.c_int32, _fp, _fp,
                                             _fp, C.c_float, _fp]),
    "hsp_zero_gaps_f32": (C.c_int, [_fp, C.c_int64, C.c_int32, C.c_int32, C.c_int32, _fp, _fp, C.c_int32, _fp]),
    "hsp_dwconv_bn_silu_seg_f32": (C.c_int, [_fp, _fp, _fp, _fp, _fp, _fp, _fp, C.c_float, _fp, C.c_int32, C.c_int32,
                                             C.c_int32, C.c_int32, _fp, _fp, C.c_int32, _fp]),
    "hsp_istft_ola_seg_f32": (C.c_int, [_fp, C.c_int64, _fp, _fp, _fp, C.c_int64, C.c_int64, C.c_int32, C.c_int32, _fp, _fp,
                                        C.c_int32, C.c_int32, _fp]),
    "hsp_maxpool1d_f32": (C.c_int, [_fp, C.c_int64, C.c_int64, _fp, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _fp]),
    "hsp_vq_nearest_f32": (C.c_int, [_fp, C.c_int64, C.c_int64, _fp, _fp, C.c_int64, C.c_int32, C.c_int32, C.c_int32,
                                     C.c_int32, C.c_int32, C.c_int32, _fp]),
    "hsp_prosody_encode_f32": (C.c_int, [C.POINTER(ProsodyArgs), _fp]),
    "hsp_add_cbias_f32": (C.c_int, [_fp, C.c_int64, C.c_int64, _fp, C.c_int64, _fp, C.c_int32, C.c_int32, C.c_int32, _fp]),
    "hsp_zero_below_f32": (C.c_int, [_fp, C.c_float, _fp, C.c_int64, _fp]),
    "hsp_peak_int16": (C.c_int, [_fp, C.c_int64, _fp, C.c_float, _fp, C.c_int64, C.c_int32, C.c_int64, _fp]),
    "hsp_f0_edit_rows_f32": (C.c_int, [C.POINTER(F0EditArgs), _fp]),
    "hsp_loudness_workspace_bytes": (C.c_int64, [C.c_int32, C.c_int64]),
    "hsp_loudness_coefs_f64": (C.c_int, [C.c_int32, _fp]),
    "hsp_loudness_f32": (C.c_int, [_fp, C.c_int64, _fp, C.c_int32, C.c_int64, C.c_int32, _fp, C.c_int64, _fp, _fp, _fp]),
    "hsp_loudness_gains_f32": (C.c_int, [_fp, _fp, C.c_float, C.c_float, _fp, _fp, C.c_int32, _fp]),
    "hsp_true_peak_f32": (C.c_int, [_fp, C.c_int64, _fp, _fp, C.c_int32, C.c_int64, _fp, C.c_int32, C.c_int32, _fp, _fp]),
    "hsp_limiter_f32": (C.c_int, [C.POINTER(LimiterArgs), _fp]),
    "hsp_gain_update_f32": (C.c_int, [_fp, _fp, C.c_float, _fp, C.c_int32, _fp]),
    "hsp_limiter_stats_f32": (C.c_int, [_fp, _fp, C.c_float, _fp, _fp, _fp, C.c_int32, _fp]),
    "hsp_gain_int16_f32": (C.c_int, [_fp, C.c_int64, _fp, _fp, _fp, C.c_int64, C.c_int32, C.c_int64, _fp]),
    "hsp_resample_f32": (C.c_int, [_fp, C.c_int64, _fp, C.c_int32, C.c_int32, _fp, _fp, C.c_int32, C.c_int32, C.c_int32,
                                   C.c_int32, _fp, C.c_int64, C.c_int32, _fp]),
    "hsp_copy_strided_f32": (C.c_int, [_fp, C.c_int64, C.c_int64, C.c_int64, _fp, C.c_int32, C.c_int32, C.c_int32,
                                       _fp]),
    "hsp_conv1d_f32": (C.c_int, [C.POINTER(Conv1dArgs), _fp]),
    "hsp_convtr1d_f32": (C.c_int, [C.POINTER(Conv1dArgs), _fp]),
    "hsp_wn_layer_f32": (C.c_int, [C.POINTER(Conv1dArgs), C.POINTER(Conv1dArgs), C.POINTER(Conv1dArgs), _fp]),
    "hsp_ffn_conv_f32": (C.c_int, [C.POINTER(Conv1dArgs), C.POINTER(Conv1dArgs), _fp]),
    "hsp_layernorm_modulate_f32": (C.c_int, [_fp, _fp, C.c_int32, C.c_int32, C.c_int32, C.c_float, _fp, _fp, _fp,
                                             C.c_int64, _fp]),
    "hsp_stft_frames_f32": (C.c_int, [_fp, _fp, _fp, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                      _fp]),
    "hsp_power_mel_log_f32": (C.c_int, [_fp, C.c_int64, C.c_int32, _fp, _fp, _fp, _fp, C.c_int32, C.c_int32, C.c_int32,
                                        C.c_int32, C.c_float, _fp]),
}

_lib: Optional[C.CDLL] = None


class HspError(RuntimeError):
    pass


def lib() -> C.CDLL:
    """Load libhsp.so once.  Raises (never falls back) when it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise HspError(
                f"{LIB_PATH} not found: build the HIP kernels first "
                "(python -c 'import __graft_entry__ as g; g.build()' or make -C megatts2_hierspeechpp_amd/csrc). "
                "There is no CPU fallback for the product path.")
        handle = C.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(handle, name)  # AttributeError if the .so lacks a declared symbol
            fn.restype, fn.argtypes = res, args
        _lib = handle
    return _lib


def check(code: int, what: str) -> None:
    if code != 0:
        kind = "invalid arguments" if code == EINVAL else f"hipError_t {code}"
        raise HspError(f"{what} failed: {kind}")


def call(name: str, *args) -> None:
    """One launch on the current stream: ``lib().<name>(*args, stream_ptr())``, its status checked under that name."""
    check(getattr(lib(), name)(*args, stream_ptr()), name)


def timed(hook, kind: str, launch, soft: bool = False):
    """The event bracket of a measured launch: ``launch()`` performs the C call and returns its status, checked under
    ``kind``; when ``hook`` (the caller's measurement hook, or None) is set it runs between two timing events on the
    current stream.  Without a hook no event is created.  ``soft``: a launch the library refuses with HSP_EINVAL is not
    an error and has no events.  Returns (status, ev_start, ev_end); the caller reports them to its hook."""
    e0 = e1 = None
    if hook is not None:
        e0, e1 = (torch.cuda.Event(enable_timing=True) for _ in range(2))
        e0.record()
    rc = launch()
    if soft and rc == EINVAL:
        return rc, None, None
    check(rc, kind)
    if hook is not None:
        e1.record()
    return 0, e0, e1


def ptr(t: Optional[torch.Tensor]) -> Optional[int]:
    """Device pointer of an fp32 (or int) ROCm tensor; None passes through as NULL."""
    if t is None:
        return None
    if not t.is_cuda:
        raise HspError("libhsp kernels run on the GPU only (got a CPU tensor); there is no CPU fallback")
    return t.data_ptr()


def fptr(t: Optional[torch.Tensor]) -> Optional[int]:
    if t is not None and t.dtype != torch.float32:
        raise HspError(f"expected float32, got {t.dtype}")
    return ptr(t)


def stream_ptr() -> int:
    return torch.cuda.current_stream().cuda_stream
