"""ctypes binding of ``libdia_hip.so`` (``include/dia_hip.h``).

The library is the product path.  There is no CPU fallback: if the shared object is missing or
does not export the expected ABI this module raises, and every call that returns a non-zero
status raises :class:`DiaHipError` carrying ``dia_last_error()``.
"""

from __future__ import annotations

import ctypes as C
import os
from typing import Optional

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("DIA_HIP_LIB") or os.path.join(_HERE, "libdia_hip.so")   # override: experiments only

ABI_VERSION = 8
KV_F32, KV_BF16, KV_BF16X2 = 0, 1, 2
EPI_SCALE_STORE, EPI_RESID_EMIT, EPI_SWIGLU_EMIT, EPI_CROSSKV = 0, 1, 2, 3
W_DENSE, W_SPARSE24, W_MXFP8, W_MXFP4, W_USPARSE = 0, 1, 2, 4, 5         # dia_gemm_args.w_format (3 is not assigned)
ATTN_SELF, ATTN_CROSS, ATTN_ENC = 0, 1, 2

EXPORTS = (
    "dia_last_error", "dia_abi_version", "dia_device_count", "dia_set_tuning", "dia_get_tuning", "dia_has_experiments", "dia_gemm", "dia_gemm_timed", "dia_gemm_wo_deferred", "dia_mlp_fused", "dia_mlp_fused_timed", "dia_engine_mlp_fused", "dia_attn", "dia_attn_scratch_floats", "dia_enc_kv_prep", "dia_enc_attn", "dia_dec_prefill_embed", "dia_dec_prefill_kv", "dia_dec_prefill_attn",
    "dia_embed_text", "dia_embed_tokens", "dia_sample", "dia_slot_admit", "dia_slot_retire", "dia_emit_frames", "dia_prefetch", "dia_engine_create", "dia_engine_destroy",
    "dia_engine_decode", "dia_engine_set_prefetch", "dia_engine_set_x_alt", "dia_engine_step_logits_only", "dia_engine_profile_step", "dia_engine_time_step", "dia_timed_kernel_name", "dia_engine_launches_per_step", "dia_mxfp8_classes", "dia_mxfp4_classes", "dia_engine_set_mxfp4", "dia_usparse_classes", "dia_engine_set_usparse",
    "dia_score", "dia_engine_set_score",
    "dia_act_stats", "dia_engine_set_calib",
    "dia_act_gram", "dia_engine_set_gram",
    "dia_lora_apply", "dia_lora_crosskv", "dia_engine_set_lora",
    "dia_kv_quantize_fp8", "dia_attn_cross_fp8", "dia_engine_set_cross_fp8",
    "dia_attn_self_fp8", "dia_engine_set_self_fp8", "dia_dec_prefill_kv_fp8", "dia_dec_prefill_attn_fp8",
    "dia_codec_embed", "dia_codec_conv", "dia_codec_convt", "dia_codec_convs", "dia_codec_quantize",
    "dia_codec_conv_bf16", "dia_codec_convt_bf16",
    "dia_resample",
    "dia_timescale",
    "dia_loudness",
    "dia_spectral",
    "dia_seg_mlp", "dia_seg_workspace_bytes", "dia_seg_workspace_control_bytes", "dia_seg_slots", "dia_seg_supported", "dia_seg_error",
)


class DiaHipError(RuntimeError):
    pass


class GemmArgs(C.Structure):
    _fields_ = [
        ("A", C.c_void_p), ("a_plane_stride", C.c_int64), ("a_ktiles", C.c_int32), ("M", C.c_int32),
        ("W", C.c_void_p), ("KT", C.c_int32), ("nstrips", C.c_int32), ("epi", C.c_int32), ("nw", C.c_int32),
        ("ssq_in", C.c_void_p), ("ssq_in_n", C.c_int32), ("ssq_ld", C.c_int32), ("inv_d", C.c_float), ("eps", C.c_float),
        ("out", C.c_void_p), ("ldo", C.c_int32), ("spw", C.c_int32),
        ("gnext", C.c_void_p), ("P", C.c_void_p), ("p_plane_stride", C.c_int64), ("p_ktiles", C.c_int32), ("_pad1", C.c_int32),
        ("ssq_out", C.c_void_p),
        ("kc", C.c_void_p), ("vc", C.c_void_p), ("kv_dtype", C.c_int32), ("kv_heads", C.c_int32), ("kv_cap", C.c_int32),
        ("kv_batch_index", C.c_int32), ("cos_t", C.c_void_p), ("sin_t", C.c_void_p),
        ("cmap", C.c_void_p), ("strip_map", C.c_void_p),
        ("sk_scratch", C.c_void_p), ("sk_tickets", C.c_void_p), ("sk", C.c_int32), ("kv_vblocked", C.c_int32),
        ("row_b", C.c_void_p), ("seg_off", C.c_void_p), ("sk_scratch_floats", C.c_int64),
        ("sp_blocks", C.c_void_p), ("sp_toff", C.c_void_p),
        ("act_f32", C.c_int32), ("w_planes", C.c_int32), ("kv_plane_stride", C.c_int64),
        ("w_layout", C.c_int32), ("kv_layer_strips", C.c_int32), ("kv_layer_stride", C.c_int64),
        ("w_format", C.c_int32), ("_pad2", C.c_int32),
    ]


class Mxfp4Layer(C.Structure):
    _fields_ = [("w_" + k, C.c_void_p) for k in ("qkv", "o", "cq", "co", "wi", "wo")]


class Mxfp4Streams(C.Structure):
    _fields_ = [("n_layer", C.c_int32), ("_pad", C.c_int32), ("layers", C.POINTER(Mxfp4Layer)), ("w_logits", C.c_void_p)]


class UsMat(C.Structure):
    """dia_us_mat: one matrix as an unstructured sparse stream (layout.tile_weight_us); dia_gemm_args.W points to one with W_USPARSE"""
    _fields_ = [("stream", C.c_void_p), ("rate", C.c_int32), ("_pad", C.c_int32)]


class UsLayer(C.Structure):
    _fields_ = [("w_" + k, UsMat) for k in ("qkv", "o", "cq", "co", "wi", "wo")]


class UsStreams(C.Structure):
    _fields_ = [("n_layer", C.c_int32), ("_pad", C.c_int32), ("layers", C.POINTER(UsLayer)), ("w_logits", UsMat)]


class WoDeferArgs(C.Structure):
    _fields_ = [
        ("slices", C.c_void_p), ("slice_stride", C.c_int64), ("nslices", C.c_int32), ("defer", C.c_int32),
        ("xold", C.c_void_p), ("xnew", C.c_void_p), ("ldx", C.c_int32), ("_pad0", C.c_int32),
    ]


class AttnArgs(C.Structure):
    _fields_ = [
        ("mode", C.c_int32), ("kv_dtype", C.c_int32), ("n_kv_heads", C.c_int32), ("group", C.c_int32),
        ("n_rows", C.c_int32), ("kv_cap", C.c_int32),
        ("q", C.c_void_p), ("ldq", C.c_int32), ("q_off", C.c_int32), ("k_off", C.c_int32), ("v_off", C.c_int32),
        ("kc", C.c_void_p), ("vc", C.c_void_p), ("cur", C.c_void_p), ("len", C.c_void_p),
        ("enc_len", C.c_int32), ("rope_rows", C.c_int32), ("cos_t", C.c_void_p), ("sin_t", C.c_void_p),
        ("P", C.c_void_p), ("p_plane_stride", C.c_int64), ("p_ktiles", C.c_int32), ("_pad1", C.c_int32),
        ("scratch", C.c_void_p), ("tickets", C.c_void_p), ("head_map", C.c_void_p),
        ("v_blocked", C.c_int32), ("act_f32", C.c_int32), ("kv_plane_stride", C.c_int64),
    ]


class EncAttnArgs(C.Structure):
    _fields_ = [
        ("qkv", C.c_void_p), ("ldq", C.c_int32), ("q_off", C.c_int32), ("k_off", C.c_int32), ("v_off", C.c_int32),
        ("heads", C.c_int32), ("rows", C.c_int32),
        ("row_b", C.c_void_p), ("seg_off", C.c_void_p), ("seg_len", C.c_void_p), ("cos_t", C.c_void_p), ("sin_t", C.c_void_p),
        ("kp", C.c_void_p), ("vp", C.c_void_p), ("P", C.c_void_p), ("p_plane_stride", C.c_int64), ("p_ktiles", C.c_int32),
        ("_pad0", C.c_int32),
    ]


class DecPrefillArgs(C.Structure):
    _fields_ = [
        ("row_seg", C.c_void_p), ("seg_off", C.c_void_p), ("seg_len", C.c_void_p), ("seg_row", C.c_void_p),
        ("rows", C.c_int32), ("_pad0", C.c_int32),
        ("tokens", C.c_void_p), ("T", C.c_int32), ("C", C.c_int32), ("V", C.c_int32), ("D", C.c_int32),
        ("emb", C.c_void_p), ("g", C.c_void_p), ("x", C.c_void_p),
        ("P", C.c_void_p), ("p_plane_stride", C.c_int64), ("p_ktiles", C.c_int32), ("ssq_ld", C.c_int32),
        ("ssq", C.c_void_p),
        ("q", C.c_void_p), ("ldq", C.c_int32), ("q_off", C.c_int32), ("k_off", C.c_int32), ("v_off", C.c_int32),
        ("q_heads", C.c_int32), ("kv_heads", C.c_int32), ("kv_cap", C.c_int32), ("causal", C.c_int32),
        ("kc", C.c_void_p), ("vc", C.c_void_p), ("cos_t", C.c_void_p), ("sin_t", C.c_void_p), ("text_len", C.c_void_p),
    ]


class EmbedArgs(C.Structure):
    _fields_ = [
        ("tokens", C.c_void_p), ("cur", C.c_void_p),
        ("B", C.c_int32), ("T", C.c_int32), ("C", C.c_int32), ("V", C.c_int32), ("D", C.c_int32), ("act_f32", C.c_int32),
        ("emb", C.c_void_p), ("g", C.c_void_p), ("x", C.c_void_p), ("P", C.c_void_p),
        ("p_plane_stride", C.c_int64), ("p_ktiles", C.c_int32), ("ssq_ld", C.c_int32), ("ssq", C.c_void_p),
        ("cmap", C.c_void_p),
        ("slots", C.c_void_p), ("n_slots", C.c_int32), ("_pad0", C.c_int32),
    ]


class SampleArgs(C.Structure):
    _fields_ = [
        ("logits", C.c_void_p), ("ld_logits", C.c_int32), ("B", C.c_int32), ("T", C.c_int32), ("C", C.c_int32),
        ("V", C.c_int32), ("max_tokens", C.c_int32),
        ("cfg_scale", C.c_float), ("temperature", C.c_float), ("top_p", C.c_float), ("top_k", C.c_int32),
        ("eos", C.c_int32), ("pad", C.c_int32), ("bos", C.c_int32), ("max_delay", C.c_int32),
        ("ignore_eos", C.c_int32), ("teacher", C.c_int32),
        ("delay", C.c_void_p), ("noise", C.c_void_p), ("noise_steps", C.c_int32), ("_pad0", C.c_int32),
        ("tokens", C.c_void_p), ("pred", C.c_void_p), ("cur", C.c_void_p), ("fsm", C.c_void_p),
        ("first_step", C.c_void_p), ("embed", EmbedArgs),
        ("slot_cfg_scale", C.c_void_p), ("slot_temperature", C.c_void_p), ("slot_top_p", C.c_void_p),
        ("slot_top_k", C.c_void_p), ("slot_max_tokens", C.c_void_p),
    ]


SLOTS_PER_CALL = 64                                       # DIA_SLOTS_PER_CALL


class SlotAdmitArgs(C.Structure):
    """dia_slot_admit_args: the per-slot arrays up to `top_k` are HOST arrays read during the call, `prefix` and everything
    behind it are device pointers"""
    _fields_ = [
        ("B", C.c_int32), ("T", C.c_int32), ("C", C.c_int32), ("S", C.c_int32), ("max_delay", C.c_int32), ("n", C.c_int32),
        ("slot", C.POINTER(C.c_int32)), ("text_len", C.POINTER(C.c_int32)), ("first_step", C.POINTER(C.c_int32)),
        ("prefix_rows", C.POINTER(C.c_int32)), ("max_tokens", C.POINTER(C.c_int32)),
        ("cfg_scale", C.POINTER(C.c_float)), ("temperature", C.POINTER(C.c_float)), ("top_p", C.POINTER(C.c_float)),
        ("top_k", C.POINTER(C.c_int32)),
        ("prefix", C.c_void_p), ("prefix_ld", C.c_int32), ("_pad0", C.c_int32),
        ("tokens", C.c_void_p), ("pred", C.c_void_p), ("cur", C.c_void_p), ("fsm", C.c_void_p),
        ("d_first_step", C.c_void_p), ("d_text_len", C.c_void_p),
        ("slot_cfg_scale", C.c_void_p), ("slot_temperature", C.c_void_p), ("slot_top_p", C.c_void_p),
        ("slot_top_k", C.c_void_p), ("slot_max_tokens", C.c_void_p),
    ]


EMIT_RESET = 1                                            # DIA_EMIT_RESET


class EmitArgs(C.Structure):
    """dia_emit_args: `slot` is a HOST array read during the call, everything behind it are device pointers"""
    _fields_ = [
        ("B", C.c_int32), ("T", C.c_int32), ("C", C.c_int32), ("max_delay", C.c_int32), ("codebook_size", C.c_int32),
        ("cap", C.c_int32), ("n", C.c_int32), ("flags", C.c_int32),
        ("slot", C.POINTER(C.c_int32)),
        ("tokens", C.c_void_p), ("cur", C.c_void_p), ("fsm", C.c_void_p), ("first_step", C.c_void_p), ("delay", C.c_void_p),
        ("emitted", C.c_void_p), ("out", C.c_void_p), ("state", C.c_void_p),
    ]


class ScoreArgs(C.Structure):
    """dia_score_args: teacher-forced scoring of token row cur[b] (csrc/score.hip)"""
    _fields_ = [
        ("logits", C.c_void_p), ("ld_logits", C.c_int32), ("B", C.c_int32), ("T", C.c_int32), ("C", C.c_int32),
        ("V", C.c_int32), ("cfg_scale", C.c_float), ("cfg_scales", C.c_void_p),
        ("eos", C.c_int32), ("pad", C.c_int32), ("bos", C.c_int32), ("_pad0", C.c_int32),
        ("tokens", C.c_void_p), ("cur", C.c_void_p), ("first_step", C.c_void_p), ("fsm", C.c_void_p), ("out", C.c_void_p),
    ]


class ActStatsArgs(C.Structure):
    """dia_act_stats_args: per-channel sums of squares of one activation plane set's counted rows (csrc/calib.hip)"""
    _fields_ = [
        ("x", C.c_void_p), ("plane_stride", C.c_int64), ("ktiles", C.c_int32), ("ktiles_used", C.c_int32),
        ("M", C.c_int32), ("rows_pad", C.c_int32), ("act_f32", C.c_int32), ("ssq_in_n", C.c_int32),
        ("ssq_in", C.c_void_p), ("ssq_ld", C.c_int32), ("inv_d", C.c_float), ("eps", C.c_float), ("rows_per_slot", C.c_int32),
        ("row_mask", C.c_void_p), ("cur", C.c_void_p), ("first_step", C.c_void_p), ("fsm", C.c_void_p),
        ("T", C.c_int32), ("_pad0", C.c_int32), ("acc", C.c_void_p), ("counter", C.c_void_p),
    ]


class CalibArgs(C.Structure):
    """dia_calib_args: acc / kt are HOST arrays of 6 * n_layer + 1 taps (copied), counters a device array"""
    _fields_ = [("n_layer", C.c_int32), ("_pad0", C.c_int32), ("acc", C.POINTER(C.c_void_p)), ("kt", C.POINTER(C.c_int32)),
                ("counters", C.c_void_p)]


class ActGramArgs(C.Structure):
    """dia_act_gram_args: the fields of dia_act_stats_args, the packed Gram matrix in the place of acc (csrc/gram.hip)"""
    _fields_ = [(("gram", t) if n == "acc" else (n, t)) for n, t in ActStatsArgs._fields_]


class GramArgs(C.Structure):
    """dia_gram_args: gram / kt are HOST arrays of 6 * n_layer + 1 taps (copied; a NULL gram = no launch), counters a device array"""
    _fields_ = [("n_layer", C.c_int32), ("_pad0", C.c_int32), ("gram", C.POINTER(C.c_void_p)), ("kt", C.POINTER(C.c_int32)),
                ("counters", C.c_void_p)]


LORA_MAX_RANK, LORA_MAX_SEGS = 64, 3                     # DIA_LORA_MAX_RANK, DIA_LORA_MAX_SEGS


class LoraSeg(C.Structure):
    """dia_lora_seg: one adapted module; A / B / rank / scale are DEVICE tables indexed by adapter"""
    _fields_ = [
        ("col_off", C.c_int32), ("n_cols", C.c_int32), ("A", C.c_void_p), ("B", C.c_void_p), ("rank", C.c_void_p),
        ("scale", C.c_void_p), ("max_rank", C.c_int32), ("_pad0", C.c_int32),
    ]


class LoraArgs(C.Structure):
    """dia_lora_args: the low-rank correction of a SCALE_STORE projection's output (csrc/lora.hip)"""
    _fields_ = [
        ("x", C.c_void_p), ("ldx", C.c_int32), ("D", C.c_int32), ("gain", C.c_void_p), ("eps", C.c_float), ("M", C.c_int32),
        ("row_slot", C.c_void_p), ("rows_per_slot", C.c_int32), ("n_slots", C.c_int32), ("adapter_of_slot", C.c_void_p),
        ("n_adapters", C.c_int32), ("n_segs", C.c_int32), ("seg", LoraSeg * LORA_MAX_SEGS),
        ("out", C.c_void_p), ("ldo", C.c_int32), ("_pad0", C.c_int32),
    ]


class LoraCrossKvArgs(C.Structure):
    """dia_lora_crosskv_args: the same correction added into the cross K/V caches"""
    _fields_ = [
        ("x", C.c_void_p), ("ldx", C.c_int32), ("D", C.c_int32), ("gain", C.c_void_p), ("eps", C.c_float), ("M", C.c_int32),
        ("row_b", C.c_void_p), ("seg_off", C.c_void_p), ("adapter_of_slot", C.c_void_p), ("n_slots", C.c_int32),
        ("n_adapters", C.c_int32), ("k", LoraSeg), ("v", LoraSeg), ("kc", C.c_void_p), ("vc", C.c_void_p),
        ("kv_dtype", C.c_int32), ("kv_heads", C.c_int32), ("kv_cap", C.c_int32), ("kv_batch_index", C.c_int32),
        ("kv_vblocked", C.c_int32), ("rope_rows", C.c_int32), ("kv_plane_stride", C.c_int64),
        ("cos_t", C.c_void_p), ("sin_t", C.c_void_p),
    ]


class LoraLayer(C.Structure):
    _fields_ = [("q", LoraSeg), ("k", LoraSeg), ("v", LoraSeg), ("cq", LoraSeg)]


class LoraStep(C.Structure):
    """dia_lora_step: what dia_engine_set_lora takes beside the engine's description"""
    _fields_ = [("n_layer", C.c_int32), ("n_adapters", C.c_int32), ("layers", C.POINTER(LoraLayer)), ("adapter_of_slot", C.c_void_p)]


class KvFp8Ptrs(C.Structure):
    """dia_kv_fp8_ptrs: the e4m3 copy of one layer's cross caches (k8 / v8 bytes, ks / vs one fp32 scale per key and head)"""
    _fields_ = [("k8", C.c_void_p), ("v8", C.c_void_p), ("ks", C.c_void_p), ("vs", C.c_void_p)]


class KvFp8Args(C.Structure):
    """dia_kv_fp8_args: `row` and `len` are HOST arrays read during the call, everything else device pointers and shapes"""
    _fields_ = [
        ("kc", C.c_void_p), ("vc", C.c_void_p), ("out", KvFp8Ptrs),
        ("B", C.c_int32), ("heads", C.c_int32), ("S", C.c_int32), ("n", C.c_int32),
        ("row", C.POINTER(C.c_int32)), ("len", C.POINTER(C.c_int32)),
        ("n_layer", C.c_int32), ("_pad0", C.c_int32), ("kv_layer_stride", C.c_int64), ("f8_layer_stride", C.c_int64),
    ]


RESAMPLE_OPEN = -1                                        # DIA_RESAMPLE_OPEN


class ResampleArgs(C.Structure):
    """dia_resample_args: x / y / bank / first are device pointers, the five per-row arrays HOST arrays read during the call"""
    _fields_ = [
        ("x", C.c_void_p), ("y", C.c_void_p), ("bank", C.c_void_p), ("first", C.c_void_p),
        ("B", C.c_int32), ("ldx", C.c_int32), ("ldy", C.c_int32), ("o", C.c_int32), ("n", C.c_int32), ("nt", C.c_int32),
        ("in_start", C.POINTER(C.c_int64)), ("out_start", C.POINTER(C.c_int64)), ("total", C.POINTER(C.c_int64)),
        ("in_count", C.POINTER(C.c_int32)), ("out_count", C.POINTER(C.c_int32)),
    ]


TS_INTERP, TS_WSOLA = 0, 1                                # DIA_TS_INTERP / DIA_TS_WSOLA
TS_OPEN = -1                                              # DIA_TS_OPEN


class TimescaleArgs(C.Structure):
    """dia_timescale_args: x / y / win / centre / delta are device pointers, the nine per-row arrays HOST arrays read during the call"""
    _fields_ = [
        ("x", C.c_void_p), ("y", C.c_void_p), ("win", C.c_void_p), ("centre", C.c_void_p), ("delta", C.c_void_p),
        ("mode", C.c_int32), ("B", C.c_int32), ("ldx", C.c_int32), ("ldy", C.c_int32), ("ldk", C.c_int32),
        ("window", C.c_int32), ("tolerance", C.c_int32), ("_pad0", C.c_int32),
        ("in_start", C.POINTER(C.c_int64)), ("out_start", C.POINTER(C.c_int64)), ("total", C.POINTER(C.c_int64)),
        ("out_total", C.POINTER(C.c_int64)), ("k0", C.POINTER(C.c_int64)), ("k1", C.POINTER(C.c_int64)),
        ("delta_prev", C.POINTER(C.c_int32)), ("in_count", C.POINTER(C.c_int32)), ("out_count", C.POINTER(C.c_int32)),
    ]


LOUD_MEASURE, LOUD_APPLY = 0, 1                           # DIA_LOUD_MEASURE / DIA_LOUD_APPLY


class LoudnessArgs(C.Structure):
    """dia_loudness_args: x / y / steps / peaks / ws / table / bank are device pointers, the five arrays at the end HOST arrays read
    during the call"""
    _fields_ = [
        ("x", C.c_void_p), ("y", C.c_void_p), ("steps", C.c_void_p), ("peaks", C.c_void_p), ("ws", C.c_void_p), ("table", C.c_void_p),
        ("bank", C.c_void_p), ("ws_doubles", C.c_int64),
        ("mode", C.c_int32), ("B", C.c_int32), ("ldx", C.c_int32), ("ldy", C.c_int32), ("ld_steps", C.c_int32),
        ("step", C.c_int32), ("chunk", C.c_int32), ("chunks", C.c_int32), ("nt", C.c_int32), ("_pad0", C.c_int32),
        ("first", C.POINTER(C.c_int32)), ("len", C.POINTER(C.c_int32)), ("in_off", C.POINTER(C.c_int32)),
        ("out_count", C.POINTER(C.c_int32)), ("gain", C.POINTER(C.c_double)),
    ]


class SpectralArgs(C.Structure):
    """dia_spectral_args: a / b / basis / fb / fb_range / partial / out are device pointers, len a HOST array read during the call"""
    _fields_ = [
        ("a", C.c_void_p), ("b", C.c_void_p), ("basis", C.c_void_p), ("fb", C.c_void_p), ("fb_range", C.c_void_p),
        ("partial", C.c_void_p), ("out", C.c_void_p),
        ("B", C.c_int32), ("ld", C.c_int32), ("window", C.c_int32), ("n_mels", C.c_int32),
        ("tiles", C.c_int32), ("out_frames", C.c_int32), ("power", C.c_int32), ("_pad0", C.c_int32),
        ("eps", C.c_double), ("len", C.POINTER(C.c_int32)),
    ]


class DecLayer(C.Structure):
    _fields_ = [
        ("w_qkv", C.c_void_p), ("w_o", C.c_void_p), ("w_cq", C.c_void_p), ("w_co", C.c_void_p),
        ("w_wi", C.c_void_p), ("w_wo", C.c_void_p), ("w_wo_diag", C.c_void_p),
        ("g_sa", C.c_void_p), ("g_ca", C.c_void_p), ("g_mlp", C.c_void_p),
        ("k_self", C.c_void_p), ("v_self", C.c_void_p), ("k_cross", C.c_void_p), ("v_cross", C.c_void_p),
        ("kt_qkv", C.c_int32), ("ns_qkv", C.c_int32), ("kt_o", C.c_int32), ("ns_o", C.c_int32),
        ("kt_cq", C.c_int32), ("ns_cq", C.c_int32), ("kt_co", C.c_int32), ("ns_co", C.c_int32),
        ("kt_wi", C.c_int32), ("ns_wi", C.c_int32), ("kt_wo", C.c_int32), ("ns_wo", C.c_int32),
        ("cmap_ca", C.c_void_p), ("cmap_mlp", C.c_void_p), ("cmap_next", C.c_void_p),
        ("smap_qkv", C.c_void_p), ("smap_cq", C.c_void_p), ("hmap_self", C.c_void_p), ("hmap_cross", C.c_void_p),
        ("w_qkv_24", C.c_void_p), ("w_o_24", C.c_void_p), ("w_cq_24", C.c_void_p), ("w_co_24", C.c_void_p),
        ("w_wi_24", C.c_void_p), ("w_wo_24", C.c_void_p),
        ("w_qkv_f8", C.c_void_p), ("w_o_f8", C.c_void_p), ("w_cq_f8", C.c_void_p), ("w_co_f8", C.c_void_p),
        ("w_wi_f8", C.c_void_p), ("w_wo_f8", C.c_void_p),
    ]


class EngineDesc(C.Structure):
    _fields_ = [
        ("n_layer", C.c_int32), ("D", C.c_int32), ("F", C.c_int32), ("q_heads", C.c_int32), ("kv_heads", C.c_int32),
        ("cq_heads", C.c_int32), ("C", C.c_int32), ("V", C.c_int32),
        ("B", C.c_int32), ("T", C.c_int32), ("S", C.c_int32), ("kv_dtype", C.c_int32),
        ("rows_pad", C.c_int32), ("ld_logits", C.c_int32), ("eps", C.c_float), ("v_blocked", C.c_int32),
        ("layers", C.POINTER(DecLayer)), ("w_logits", C.c_void_p), ("kt_logits", C.c_int32), ("ns_logits", C.c_int32),
        ("g_final", C.c_void_p),
        ("x", C.c_void_p), ("planes_x", C.c_void_p), ("planes_a", C.c_void_p), ("planes_h", C.c_void_p),
        ("ssq", C.c_void_p), ("qkv", C.c_void_p), ("qc", C.c_void_p), ("logits", C.c_void_p),
        ("cos_t", C.c_void_p), ("sin_t", C.c_void_p), ("text_len", C.c_void_p),
        ("sk_scratch", C.c_void_p), ("sk_tickets", C.c_void_p),
        ("attn_scratch", C.c_void_p), ("attn_tickets", C.c_void_p), ("sk_scratch_floats", C.c_int64), ("mlp_barrier", C.c_void_p),
        ("act_f32", C.c_int32), ("w_planes", C.c_int32),
        ("sample", SampleArgs),
        ("seg_w", C.POINTER(C.c_void_p)), ("seg_ws", C.c_void_p),
        ("kv_plane_self", C.c_int64), ("kv_plane_cross", C.c_int64),
        ("w_logits_24", C.c_void_p), ("w_logits_f8", C.c_void_p),
    ]


class SegArgs(C.Structure):
    _fields_ = [
        ("a_in", C.c_void_p), ("a_ktiles", C.c_int32), ("M", C.c_int32),
        ("W", C.c_void_p), ("nslots", C.c_int32), ("has_qkv", C.c_int32), ("D", C.c_int32), ("F", C.c_int32),
        ("x", C.c_void_p), ("ldx", C.c_int32), ("_pad0", C.c_int32),
        ("g_mlp", C.c_void_p), ("g_next", C.c_void_p), ("qkv_out", C.c_void_p), ("ldq", C.c_int32), ("_pad1", C.c_int32),
        ("planes_x", C.c_void_p), ("xkt", C.c_int32), ("_pad2", C.c_int32), ("ssq", C.c_void_p), ("ssq_ld", C.c_int32), ("eps", C.c_float),
        ("ws", C.c_void_p), ("timeout_us", C.c_int32), ("_pad3", C.c_int32), ("stamps", C.c_void_p),
    ]


_lib: Optional[C.CDLL] = None


def lib() -> C.CDLL:
    """Load the HIP library once.  Raises (never falls back) when it is absent or stale."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.isfile(LIB_PATH):
        raise DiaHipError(
            f"{LIB_PATH} is missing: build it with `python __graft_entry__.py` or "
            f"`make -C dia-tts-prune_amd/csrc` (hipcc --offload-arch=gfx950). There is no CPU fallback."
        )
    # torch ships its own libamdhip64 / libhsa-runtime64; load it FIRST so that this library binds to
    # the same HIP runtime instance as the tensors whose pointers it receives (two runtimes in one
    # process do not share a device context)
    import torch  # noqa: F401

    try:
        L = C.CDLL(LIB_PATH)
    except OSError as e:  # e.g. libamdhip64.so not found
        raise DiaHipError(f"cannot load {LIB_PATH}: {e}") from e
    for name in EXPORTS:
        if not hasattr(L, name):
            raise DiaHipError(f"{LIB_PATH} does not export {name}; rebuild it")
    L.dia_last_error.restype = C.c_char_p
    L.dia_abi_version.restype = C.c_int
    if L.dia_abi_version() != ABI_VERSION:
        raise DiaHipError(f"ABI mismatch: library {L.dia_abi_version()} vs binding {ABI_VERSION}")
    L.dia_set_tuning.argtypes = [C.c_char_p, C.c_int]
    L.dia_get_tuning.argtypes = [C.c_char_p]
    L.dia_has_experiments.restype = C.c_int
    L.dia_gemm.argtypes = [C.POINTER(GemmArgs), C.c_void_p]
    L.dia_gemm_timed.argtypes = [C.POINTER(GemmArgs), C.c_void_p, C.POINTER(C.c_float)]
    L.dia_gemm_wo_deferred.argtypes = [C.POINTER(GemmArgs), C.POINTER(WoDeferArgs), C.c_void_p, C.POINTER(C.c_float)]
    L.dia_engine_set_x_alt.argtypes = [C.c_void_p, C.c_void_p]
    L.dia_mlp_fused.argtypes = [C.POINTER(GemmArgs), C.POINTER(GemmArgs), C.c_void_p, C.c_void_p]
    L.dia_mlp_fused_timed.argtypes = [C.POINTER(GemmArgs), C.POINTER(GemmArgs), C.c_void_p, C.c_void_p, C.POINTER(C.c_float)]
    L.dia_engine_mlp_fused.argtypes = [C.c_void_p]
    L.dia_attn.argtypes = [C.POINTER(AttnArgs), C.c_void_p]
    L.dia_attn_scratch_floats.argtypes = [C.c_int, C.c_int, C.c_int]
    L.dia_enc_attn.argtypes = [C.POINTER(EncAttnArgs), C.c_void_p]
    for fn in (L.dia_dec_prefill_embed, L.dia_dec_prefill_kv, L.dia_dec_prefill_attn):
        fn.argtypes = [C.POINTER(DecPrefillArgs), C.c_void_p]
    L.dia_enc_kv_prep.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                  C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.dia_embed_text.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                 C.c_int64, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    L.dia_embed_tokens.argtypes = [C.POINTER(EmbedArgs), C.c_void_p]
    L.dia_sample.argtypes = [C.POINTER(SampleArgs), C.c_void_p]
    L.dia_slot_admit.argtypes = [C.POINTER(SlotAdmitArgs), C.c_void_p]
    L.dia_slot_retire.argtypes = [C.POINTER(SlotAdmitArgs), C.c_void_p]
    L.dia_emit_frames.argtypes = [C.POINTER(EmitArgs), C.c_void_p]
    L.dia_prefetch.argtypes = [C.c_void_p, C.c_int64, C.c_int, C.c_void_p]
    L.dia_engine_create.argtypes = [C.POINTER(EngineDesc), C.c_void_p, C.POINTER(C.c_void_p)]
    L.dia_engine_destroy.argtypes = [C.c_void_p]
    L.dia_engine_decode.argtypes = [C.c_void_p, C.c_int, C.c_int]
    L.dia_engine_step_logits_only.argtypes = [C.c_void_p]
    L.dia_engine_set_prefetch.argtypes = [C.c_void_p, C.c_int]
    L.dia_engine_launches_per_step.argtypes = [C.c_void_p]
    L.dia_engine_profile_step.argtypes = [C.c_void_p, C.POINTER(C.c_float), C.c_int]
    L.dia_engine_time_step.argtypes = [C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_int]
    L.dia_timed_kernel_name.argtypes = [C.c_int]
    L.dia_timed_kernel_name.restype = C.c_char_p
    L.dia_mxfp8_classes.argtypes = [C.c_int]
    L.dia_mxfp4_classes.argtypes = [C.c_int]
    L.dia_engine_set_mxfp4.argtypes = [C.c_void_p, C.POINTER(Mxfp4Streams)]
    L.dia_usparse_classes.argtypes = [C.c_int]
    L.dia_engine_set_usparse.argtypes = [C.c_void_p, C.POINTER(UsStreams)]
    L.dia_score.argtypes = [C.POINTER(ScoreArgs), C.c_void_p]
    L.dia_engine_set_score.argtypes = [C.c_void_p, C.POINTER(ScoreArgs)]
    L.dia_act_stats.argtypes = [C.POINTER(ActStatsArgs), C.c_void_p]
    L.dia_engine_set_calib.argtypes = [C.c_void_p, C.POINTER(CalibArgs)]
    L.dia_act_gram.argtypes = [C.POINTER(ActGramArgs), C.c_void_p]
    L.dia_engine_set_gram.argtypes = [C.c_void_p, C.POINTER(GramArgs)]
    L.dia_lora_apply.argtypes = [C.POINTER(LoraArgs), C.c_void_p]
    L.dia_lora_crosskv.argtypes = [C.POINTER(LoraCrossKvArgs), C.c_void_p]
    L.dia_engine_set_lora.argtypes = [C.c_void_p, C.POINTER(LoraStep)]
    L.dia_kv_quantize_fp8.argtypes = [C.POINTER(KvFp8Args), C.c_void_p]
    L.dia_attn_cross_fp8.argtypes = [C.POINTER(AttnArgs), C.POINTER(KvFp8Ptrs), C.c_void_p]
    L.dia_engine_set_cross_fp8.argtypes = [C.c_void_p, C.POINTER(KvFp8Ptrs)]
    L.dia_attn_self_fp8.argtypes = [C.POINTER(AttnArgs), C.POINTER(KvFp8Ptrs), C.c_void_p]
    L.dia_engine_set_self_fp8.argtypes = [C.c_void_p, C.POINTER(KvFp8Ptrs)]
    for fn in (L.dia_dec_prefill_kv_fp8, L.dia_dec_prefill_attn_fp8):
        fn.argtypes = [C.POINTER(DecPrefillArgs), C.POINTER(KvFp8Ptrs), C.c_void_p]
    L.dia_resample.argtypes = [C.POINTER(ResampleArgs), C.c_void_p]
    L.dia_timescale.argtypes = [C.POINTER(TimescaleArgs), C.c_void_p]
    L.dia_loudness.argtypes = [C.POINTER(LoudnessArgs), C.c_void_p]
    L.dia_spectral.argtypes = [C.POINTER(SpectralArgs), C.c_void_p]
    L.dia_seg_mlp.argtypes = [C.POINTER(SegArgs), C.c_void_p]
    L.dia_seg_workspace_bytes.restype = C.c_int64
    L.dia_seg_workspace_control_bytes.restype = C.c_int64
    L.dia_seg_slots.argtypes = [C.c_int]
    L.dia_seg_supported.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int]
    L.dia_seg_error.argtypes = [C.c_void_p, C.c_void_p]
    _lib = L
    return L


def set_tuning(name: str, value: int) -> None:
    """launch-heuristic override (csrc/tuning.hpp); value < 0 clears it"""
    check(lib().dia_set_tuning(name.encode(), int(value)), f"dia_set_tuning({name})")


def get_tuning(name: str) -> int:
    """current value of a launch-heuristic override, -1 = unset (DIA_TUNE is read on first use)"""
    return int(lib().dia_get_tuning(name.encode()))


def mxfp8_mask(rows: int) -> int:
    """launch classes (bit m = matrix m of engine.STEP_MATS) that a decode step of `rows` rows streams as MXFP8 when the model carries
    the streams: the library's measured default, or the knob mxfp8"""
    return int(lib().dia_mxfp8_classes(int(rows)))


def usparse_mask(rows: int) -> int:
    """as mxfp8_mask for the unstructured sparse streams and the knob usparse (0 above 4 rows)"""
    return int(lib().dia_usparse_classes(int(rows)))


def mxfp4_mask(rows: int) -> int:
    """as mxfp8_mask for the MXFP4 streams and the knob mxfp4"""
    return int(lib().dia_mxfp4_classes(int(rows)))


def has_experiments() -> bool:
    return bool(lib().dia_has_experiments())


def check(rc: int, what: str = "") -> None:
    if rc != 0:
        msg = lib().dia_last_error()
        raise DiaHipError(f"{what} failed ({rc}): {msg.decode() if msg else ''}")


def ptr(t) -> int:
    """Raw device pointer of a torch tensor (or None -> NULL)."""
    return 0 if t is None else t.data_ptr()
