"""ctypes binding of ``libmra_hip.so`` (the C ABI declared in ``include/mra.h``).

There is no CPU fallback: if the library is missing this raises, and every op in
``mraudio_amd`` goes through it.  ``torch`` is imported first on purpose: the PyTorch-ROCm wheel
ships its own ``libamdhip64.so.7`` and the HIP runtime must be shared with it so that the device
pointers and streams torch hands us are valid inside the kernels' launches.
"""
from __future__ import annotations

import ctypes as C
import os

import torch  # noqa: F401  (loads the HIP runtime the extension binds to)

MRA_F32, MRA_F16, MRA_BF16 = 0, 1, 2
_ERR = {-1: "MRA_EINVAL", -2: "MRA_ESTATE", -3: "MRA_EHIP", -4: "MRA_ENOMEM", -5: "MRA_ENAME"}

LIB_NAME = "libmra_hip.so"
LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), LIB_NAME)


class mra_cfg(C.Structure):
    _fields_ = [
        ("hidden", C.c_int32), ("heads", C.c_int32), ("inter", C.c_int32), ("layers", C.c_int32),
        ("cross_freq", C.c_int32), ("enc_width", C.c_int32), ("n_query", C.c_int32), ("vocab", C.c_int32),
        ("max_pos", C.c_int32), ("ln_eps", C.c_float), ("enc_ln_eps", C.c_float), ("llm_hidden", C.c_int32),
        ("op_dtype", C.c_int32),
    ]


class mra_vit_cfg(C.Structure):
    _fields_ = [("dim", C.c_int32), ("heads", C.c_int32), ("mlp", C.c_int32), ("depth", C.c_int32), ("patch", C.c_int32),
                ("img", C.c_int32), ("ln_eps", C.c_float), ("op_dtype", C.c_int32), ("residual_dtype", C.c_int32)]


MRA_BEATS_GATE_Q, MRA_BEATS_GATE_INPUT = 0, 1
MRA_LORA_NR, MRA_LORA_RN = 0, 1                  # a small fp32 matrix stored [width][R] (lora_B) or [R][width] (lora_A)


class mra_beats_cfg(C.Structure):
    _fields_ = [("dim", C.c_int32), ("heads", C.c_int32), ("ffn", C.c_int32), ("layers", C.c_int32), ("embed_dim", C.c_int32),
                ("patch", C.c_int32), ("mel_bins", C.c_int32), ("conv_pos", C.c_int32), ("conv_pos_groups", C.c_int32),
                ("num_buckets", C.c_int32), ("max_distance", C.c_int32), ("ln_eps", C.c_float), ("deep_norm_alpha", C.c_float),
                ("gate_from", C.c_int32), ("op_dtype", C.c_int32)]


class mra_rows_src(C.Structure):
    """include/mra.h mra_rows_src: one source of mra_gather_rows, ``[rows][ld]`` of ``dtype`` on the device."""
    _fields_ = [("ptr", C.c_void_p), ("ld", C.c_int64), ("rows", C.c_int32), ("dtype", C.c_int32)]


class mra_gemm_desc(C.Structure):
    """include/mra.h mra_gemm_desc: one problem of mra_debug_gemm / mra_debug_gemm_plan (the GemmProb fields of csrc/kernels.h the forwards
    set, plus the byte size of every buffer).  ``struct_bytes`` must be ``ctypes.sizeof(mra_gemm_desc)``."""
    _fields_ = [
        ("struct_bytes", C.c_uint64),
        ("A", C.c_void_p), ("W", C.c_void_p), ("bias", C.c_void_p), ("C", C.c_void_p), ("R", C.c_void_p),
        ("a_view", C.c_int64 * 3), ("c_view", C.c_int64 * 3), ("r_view", C.c_int64 * 3),
        ("M", C.c_int32), ("N", C.c_int32), ("K", C.c_int32),
        ("kv_tokens", C.c_int32), ("kv_items", C.c_int32), ("kv_heads", C.c_int32),
        ("batch", C.c_int32), ("bias_bs", C.c_int32),
        ("a_bs", C.c_int64), ("w_bs", C.c_int64), ("c_bs_bytes", C.c_int64),
        ("n_ragged", C.c_int32), ("w_ld", C.c_int32), ("k_rows", C.c_int32), ("w_kwrap", C.c_int32),
        ("ln_gain", C.c_void_p), ("ln_bias", C.c_void_p), ("ln_y32", C.c_void_p), ("ln_y16", C.c_void_p), ("ln_counter", C.c_void_p),
        ("ln_y32_view", C.c_int64 * 3), ("ln_y16_view", C.c_int64 * 3),
        ("ln_eps", C.c_float), ("alpha", C.c_float),
        ("stat_m", C.c_void_p), ("stat_l", C.c_void_p), ("pscale", C.c_void_p),
        ("ps_ntiles", C.c_int32), ("tile_cfg", C.c_int32), ("persist", C.c_int32), ("reserved", C.c_int32),
        ("a_bytes", C.c_uint64), ("w_bytes", C.c_uint64), ("bias_bytes", C.c_uint64), ("c_bytes", C.c_uint64), ("r_bytes", C.c_uint64),
        ("ln_gain_bytes", C.c_uint64), ("ln_bias_bytes", C.c_uint64), ("ln_y32_bytes", C.c_uint64), ("ln_y16_bytes", C.c_uint64),
        ("ln_counter_bytes", C.c_uint64), ("stat_m_bytes", C.c_uint64), ("stat_l_bytes", C.c_uint64), ("pscale_bytes", C.c_uint64),
        ("col_scale", C.c_void_p), ("cs_bs", C.c_int64), ("col_stats", C.c_int32), ("cs_eps", C.c_float),
        ("col_scale_bytes", C.c_uint64),
        ("aux", C.c_void_p), ("aux_bytes", C.c_uint64),
        ("k128", C.c_int32), ("ps_stats", C.c_int32),
    ]


class mra_lm_linear(C.Structure):
    """include/mra.h mra_lm_linear: W [N][K] (16-bit, pitch ldw) with an optional fp32 adapter A [R][K], Bw [N][R]."""
    _fields_ = [("W", C.c_void_p), ("ldw", C.c_int64), ("A", C.c_void_p), ("Bw", C.c_void_p), ("N", C.c_int32), ("R", C.c_int32),
                ("scale", C.c_float), ("reserved", C.c_int32)]


class mra_lm_layer(C.Structure):
    _fields_ = [("norm1", C.c_void_p), ("norm2", C.c_void_p), ("q", mra_lm_linear), ("k", mra_lm_linear), ("v", mra_lm_linear),
                ("o", mra_lm_linear), ("gate", mra_lm_linear), ("up", mra_lm_linear), ("down", mra_lm_linear), ("kcache", C.c_void_p),
                ("vcache", C.c_void_p)]


class mra_lm_step_desc(C.Structure):
    """include/mra.h mra_lm_step_desc.  ``struct_bytes`` must be ``ctypes.sizeof(mra_lm_step_desc)``."""
    _fields_ = [
        ("struct_bytes", C.c_uint64),
        ("B", C.c_int32), ("hidden", C.c_int32), ("intermediate", C.c_int32), ("Hq", C.c_int32), ("Hkv", C.c_int32), ("D", C.c_int32),
        ("L", C.c_int32), ("V", C.c_int32), ("dtype", C.c_int32), ("Smax", C.c_int32),
        ("eps", C.c_float), ("attn_scale", C.c_float),
        ("layers", C.POINTER(mra_lm_layer)), ("embed", C.c_void_p), ("ld_embed", C.c_int64), ("final_norm", C.c_void_p),
        ("head", C.c_void_p), ("ld_head", C.c_int64),
        ("k_sb", C.c_int64), ("k_sh", C.c_int64), ("k_ss", C.c_int64), ("v_sb", C.c_int64), ("v_sh", C.c_int64), ("v_ss", C.c_int64),
        ("mask", C.c_void_p), ("mask_sb", C.c_int64), ("position", C.c_void_p), ("pos_offset", C.c_int32), ("slot", C.c_int32),
        ("cos", C.c_void_p), ("sin", C.c_void_p), ("rope_ld", C.c_int64), ("rope_rows", C.c_int32), ("n_eos", C.c_int32),
        ("tokens_in", C.c_void_p), ("h", C.c_void_p), ("logits", C.c_void_p), ("ld_logits", C.c_int64), ("tokens_out", C.c_void_p),
        ("finished", C.c_void_p), ("pad", C.c_int32), ("eos", C.c_int32 * 8), ("reserved", C.c_int32),
        ("workspace", C.c_void_p), ("workspace_bytes", C.c_uint64),
    ]


class mra_lm_skinny_desc(C.Structure):
    """include/mra.h mra_lm_skinny_desc: one launch of the step's skinny kernel (mra_debug_lm_skinny), every buffer with its byte size."""
    _fields_ = [
        ("struct_bytes", C.c_uint64),
        ("B", C.c_int32), ("K", C.c_int32), ("dtype", C.c_int32), ("epilogue", C.c_int32), ("nseg", C.c_int32), ("out_f32", C.c_int32),
        ("x", C.c_void_p), ("ldx", C.c_int64), ("x_bytes", C.c_uint64),
        ("norm_gain", C.c_void_p), ("eps", C.c_float), ("reserved", C.c_int32),
        ("seg", mra_lm_linear * 3), ("w_bytes", C.c_uint64 * 3),
        ("out", C.c_void_p * 3), ("ldo", C.c_int64 * 3), ("out_bytes", C.c_uint64 * 3),
        ("res", C.c_void_p), ("ldres", C.c_int64), ("res_bytes", C.c_uint64),
        ("Hq", C.c_int32), ("Hkv", C.c_int32), ("D", C.c_int32), ("slot", C.c_int32), ("pos_offset", C.c_int32), ("rope_rows", C.c_int32),
        ("position", C.c_void_p), ("cos", C.c_void_p), ("sin", C.c_void_p), ("rope_ld", C.c_int64), ("rope_bytes", C.c_uint64),
        ("kcache", C.c_void_p), ("vcache", C.c_void_p),
        ("k_sb", C.c_int64), ("k_sh", C.c_int64), ("k_ss", C.c_int64), ("v_sb", C.c_int64), ("v_sh", C.c_int64), ("v_ss", C.c_int64),
        ("kcache_bytes", C.c_uint64), ("vcache_bytes", C.c_uint64),
        ("workspace", C.c_void_p), ("workspace_bytes", C.c_uint64),
    ]


LM_EPI_PLAIN, LM_EPI_RES, LM_EPI_SWIGLU, LM_EPI_ROPE = 0, 1, 2, 3     # mra_lm_skinny_desc.epilogue (csrc/kernels.h LmEpi)
LM_CB = 16                                                           # columns per workgroup of the skinny kernel (the rotary form: D)


# name -> (restype, argtypes); must list every symbol include/mra.h declares (tests check this)
PROTOTYPES = {
    "mra_cfg_default": (None, [C.POINTER(mra_cfg), C.c_int32]),
    "mra_last_error": (C.c_char_p, []),
    "mra_version": (C.c_char_p, []),
    "mra_qformer_create": (C.c_int, [C.POINTER(mra_cfg), C.POINTER(C.c_void_p)]),
    "mra_qformer_destroy": (None, [C.c_void_p]),
    "mra_qformer_load": (C.c_int, [C.c_void_p, C.c_char_p, C.c_void_p, C.c_int32, C.POINTER(C.c_int64), C.c_int32,
                                   C.c_void_p]),
    "mra_qformer_missing": (C.c_int, [C.c_void_p, C.c_char_p, C.c_size_t]),
    "mra_modality_ln": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p,
                                  C.c_void_p]),
    "mra_qformer_workspace_bytes": (C.c_size_t, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32]),
    "mra_qformer_forward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32,
                                      C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t,
                                      C.c_void_p]),
    "mra_qformer_raw_features_ok": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32]),
    "mra_qformer_forward_raw": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32,
                                          C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t,
                                          C.c_void_p]),
    "mra_qformer_pair_workspace_bytes": (C.c_size_t, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32]),
    "mra_qformer_forward_pair": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                           C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "mra_qformer_forward_pair_raw": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                               C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "mra_qformer_multi_workspace_bytes": (C.c_size_t, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32]),
    "mra_qformer_forward_multi": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                            C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "mra_qformer_set_kv_events": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "mra_qformer_set_kv_done_event": (C.c_int, [C.c_void_p, C.c_void_p]),
    "mra_qformer_set_cross_mode": (C.c_int, [C.c_void_p, C.c_int32]),
    "mra_qformer_set_cross_precision": (C.c_int, [C.c_void_p, C.c_int32]),
    "mra_qformer_cross_precision_report": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_float), C.c_int32]),
    "mra_qformer_set_option": (C.c_int, [C.c_void_p, C.c_char_p, C.c_int32]),
    "mra_qformer_prepare": (C.c_int, [C.c_void_p, C.c_void_p]),
    "mra_kv_cache_bytes": (C.c_size_t, [C.c_void_p, C.c_int32, C.c_int32]),
    "mra_kv_project": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]),
    "mra_llm_proj": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_size_t,
                               C.c_void_p]),
    "mra_llm_proj_backward_workspace_bytes": (C.c_size_t, [C.c_void_p, C.c_int32, C.c_int32]),
    "mra_llm_proj_backward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p,
                                        C.c_void_p, C.c_size_t, C.c_void_p]),
    "mra_cosine_score": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p,
                                   C.c_void_p, C.c_void_p]),
    "mra_lora_down": (C.c_int, [C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_float, C.c_double,
                                C.c_uint64, C.c_void_p, C.c_void_p]),
    "mra_lora_up_add": (C.c_int, [C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_float,
                                  C.c_double, C.c_uint64, C.c_void_p]),
    "mra_lora_wgrad": (C.c_int, [C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_float,
                                 C.c_double, C.c_uint64, C.c_void_p]),
    "mra_lm_head_ce_workspace_bytes": (C.c_size_t, [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32]),
    "mra_lm_head_ce_forward": (C.c_int, [C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_void_p,
                                         C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_int32, C.c_void_p]),
    "mra_lm_head_ce_backward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p,
                                          C.c_size_t, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p]),
    "mra_decode_attention_workspace_bytes": (C.c_size_t, [C.c_int32, C.c_int32, C.c_int32, C.c_int32]),
    "mra_decode_attention": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_void_p, C.c_int64, C.c_int64,
                                       C.c_int64, C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_float,
                                       C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "mra_prefill_attention": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_void_p, C.c_int64,
                                        C.c_int64, C.c_int64, C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                        C.c_int32, C.c_int32, C.c_float, C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p]),
    "mra_prefill_attention_backward_workspace_bytes": (C.c_size_t, [C.c_int32, C.c_int32, C.c_int32]),
    "mra_prefill_attention_backward": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_void_p,
                                                 C.c_int64, C.c_int64, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int64, C.c_int64,
                                                 C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                                 C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_float, C.c_void_p, C.c_int64, C.c_int64, C.c_int64,
                                                 C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_void_p,
                                                 C.c_size_t, C.c_void_p]),
    "mra_lm_step_workspace_bytes": (C.c_size_t, [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32]),
    "mra_lm_step": (C.c_int, [C.POINTER(mra_lm_step_desc), C.c_void_p]),
    "mra_debug_lm_skinny": (C.c_int, [C.POINTER(mra_lm_skinny_desc), C.c_void_p]),
    "mra_debug_lm_argmax": (C.c_int, [C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(C.c_int32), C.c_int32,
                                      C.c_void_p]),
    "mra_gather_rows": (C.c_int, [C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.POINTER(mra_rows_src), C.c_int32, C.c_void_p,
                                  C.c_void_p]),
    "mra_fuse_logits": (C.c_int, [C.POINTER(C.c_void_p), C.POINTER(C.c_float), C.c_int32, C.c_int32, C.c_void_p,
                                  C.c_void_p]),
    "mra_span_from_logits": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_float, C.c_void_p, C.c_void_p]),
    "mra_windows_from_logits": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_float, C.c_int32, C.c_float, C.c_int32, C.c_void_p,
                                          C.c_void_p, C.c_void_p, C.c_void_p]),
    "mra_qformer_grad_bytes": (C.c_size_t, [C.c_void_p]),
    "mra_qformer_load_flat": (C.c_int32, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "mra_qformer_grad_offset": (C.c_int, [C.c_void_p, C.c_char_p, C.POINTER(C.c_size_t), C.POINTER(C.c_int64)]),
    "mra_qformer_enable_training": (C.c_int, [C.c_void_p, C.c_void_p]),
    "mra_qformer_adam_step": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_float, C.c_float, C.c_float,
                                        C.c_float, C.c_float, C.c_int32, C.c_int32, C.c_void_p]),
    "mra_qformer_train_workspace_bytes": (C.c_size_t, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32]),
    "mra_qformer_forward_train": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32,
                                            C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "mra_qformer_backward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32,
                                       C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "mra_qformer_multi_train_workspace_bytes": (C.c_size_t, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32]),
    "mra_qformer_forward_multi_train": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                                  C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "mra_qformer_backward_multi": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                             C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "mra_qformer_backward_enc": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]),
    "mra_modality_ln_backward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                           C.c_void_p]),
    "mra_debug_kvgrad_gemm": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int32, C.c_int32, C.c_void_p, C.c_size_t, C.c_void_p]),
    "mra_qformer_flops": (C.c_double, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32]),
    "mra_vit_cfg_default": (None, [C.POINTER(mra_vit_cfg)]),
    "mra_vit_create": (C.c_int, [C.POINTER(mra_vit_cfg), C.POINTER(C.c_void_p)]),
    "mra_vit_destroy": (None, [C.c_void_p]),
    "mra_vit_load": (C.c_int, [C.c_void_p, C.c_char_p, C.c_void_p, C.c_int32, C.POINTER(C.c_int64), C.c_int32, C.c_void_p]),
    "mra_vit_missing": (C.c_int, [C.c_void_p]),
    "mra_vit_workspace_bytes": (C.c_size_t, [C.c_void_p, C.c_int32]),
    "mra_vit_forward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "mra_vit_flops": (C.c_double, [C.c_void_p, C.c_int32]),
    "mra_vit_set_option": (C.c_int, [C.c_void_p, C.c_char_p, C.c_int32]),
    "mra_beats_cfg_default": (None, [C.POINTER(mra_beats_cfg)]),
    "mra_beats_create": (C.c_int, [C.POINTER(mra_beats_cfg), C.POINTER(C.c_void_p)]),
    "mra_beats_destroy": (None, [C.c_void_p]),
    "mra_beats_load": (C.c_int, [C.c_void_p, C.c_char_p, C.c_void_p, C.c_int32, C.POINTER(C.c_int64), C.c_int32, C.c_void_p]),
    "mra_beats_missing": (C.c_int, [C.c_void_p]),
    "mra_beats_workspace_bytes": (C.c_size_t, [C.c_void_p, C.c_int32, C.c_int32]),
    "mra_beats_forward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "mra_beats_flops": (C.c_double, [C.c_void_p, C.c_int32, C.c_int32]),
    "mra_beats_set_option": (C.c_int, [C.c_void_p, C.c_char_p, C.c_int32]),
    "mra_fbank_create": (C.c_int, [C.POINTER(C.c_void_p)]),
    "mra_fbank_destroy": (None, [C.c_void_p]),
    "mra_fbank_forward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p]),
    "mra_fbank_flops": (C.c_double, [C.c_void_p, C.c_int32, C.c_int32]),
    "mra_resample_create": (C.c_int, [C.c_int32, C.c_int32, C.POINTER(C.c_void_p)]),
    "mra_resample_destroy": (None, [C.c_void_p]),
    "mra_resample_out_samples": (C.c_int64, [C.c_int32, C.c_int32, C.c_int64]),
    "mra_resample_forward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p]),
    "mra_resample_flops": (C.c_double, [C.c_void_p, C.c_int64]),
    "mra_video_crop_table": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]),
    "mra_video_frames_forward": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32,
                                           C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_int32, C.c_void_p, C.c_int32, C.c_void_p]),
    "mra_video_frames_bytes": (C.c_double, [C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_int32]),
    "mra_debug_video_frames_forward": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32,
                                                 C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_int32, C.c_void_p, C.c_int32, C.c_int32,
                                                 C.c_void_p]),
    "mra_debug_gemm_launches": (C.c_int64, [C.c_int32, C.c_int32]),
    "mra_debug_vit_attention": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]),
    "mra_debug_shared_kv_workspace_bytes": (C.c_size_t, [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32]),
    "mra_debug_shared_kv_attention": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                                C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "mra_debug_attention_bwd": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32,
                                          C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mra_debug_beats_attention": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]),
    "mra_debug_beats_posconv": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p]),
    "mra_debug_self_attention": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mra_debug_self_attention_bwd": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                               C.c_void_p, C.c_void_p]),
    "mra_debug_ln_rows": (C.c_int, [C.c_void_p, C.POINTER(C.c_int64), C.c_int32, C.c_int32, C.POINTER(C.c_void_p), C.c_int32, C.c_int32, C.c_int32,
                                    C.c_float, C.c_void_p, C.POINTER(C.c_int64), C.c_void_p, C.POINTER(C.c_int64), C.c_int32, C.c_void_p]),
    "mra_debug_embed_ln": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p,
                                     C.c_void_p, C.c_void_p, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]),
    "mra_debug_modality_ln": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_float,
                                        C.c_void_p, C.c_int32, C.c_void_p]),
    "mra_debug_softmax_rows": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_float, C.c_int32,
                                         C.c_void_p]),
    "mra_debug_fold_query": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t,
                                       C.c_void_p, C.c_size_t, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p]),
    "mra_debug_fold_query_launches": (C.c_int64, []),
    "mra_debug_qkv_attention": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p,
                                          C.c_void_p]),
    "mra_debug_qkv_attention_launches": (C.c_int64, []),
    "mra_debug_attention_launches": (C.c_int64, [C.c_int32]),
    "mra_debug_self_fuse_plan": (C.c_int32, [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32]),
    "mra_debug_fold_rowfactor_launches": (C.c_int64, []),
    "mra_debug_fold_rowfactor": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_int64, C.c_int32,
                                           C.c_int32, C.c_void_p, C.c_void_p]),
    "mra_debug_softmax_rescale": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                            C.c_void_p, C.c_void_p]),
    "mra_debug_transpose_pad": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int64, C.c_int64, C.c_int32, C.c_int32,
                                          C.c_void_p]),
    "mra_debug_split": (C.c_int, [C.c_int32, C.c_void_p, C.POINTER(C.c_int64), C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_int32,
                                  C.c_void_p]),
    "mra_debug_gemm_tn_group": (C.c_int, [C.c_int32, C.POINTER(C.c_void_p), C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_void_p),
                                          C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_int32),
                                          C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.c_int32, C.c_void_p]),
    "mra_debug_ln_bwd": (C.c_int, [C.POINTER(C.c_void_p), C.POINTER(C.c_int64), C.c_int32, C.c_float, C.POINTER(C.c_void_p), C.POINTER(C.c_int64),
                                   C.c_int32, C.c_float, C.c_int32, C.c_int32, C.c_void_p]),
    "mra_debug_embed_bwd": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p,
                                      C.c_void_p]),
    "mra_debug_transpose16_batch_scratch_bytes": (C.c_size_t, [C.c_int32]),
    "mra_debug_transpose16_batch": (C.c_int, [C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.c_int32,
                                              C.c_int32, C.c_void_p, C.c_size_t, C.c_void_p]),
    "mra_debug_gemm_gelu": (C.c_int, [C.c_int32, C.POINTER(C.c_void_p), C.POINTER(C.c_int64), C.POINTER(C.c_void_p), C.POINTER(C.c_void_p),
                                      C.POINTER(C.c_void_p), C.POINTER(C.c_int64), C.POINTER(C.c_void_p), C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                                      C.POINTER(C.c_int32), C.c_int32, C.c_int32, C.c_int32, C.c_void_p]),
    "mra_debug_gemm": (C.c_int, [C.POINTER(mra_gemm_desc), C.c_int32, C.c_int32, C.c_int32, C.c_void_p]),
    "mra_debug_gemm_plan": (C.c_int, [C.POINTER(mra_gemm_desc), C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_int32)]),
    "mra_debug_vit_fold_weight": (C.c_int, [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p,
                                            C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_int32, C.c_int32, C.c_int32, C.c_void_p]),
    "mra_debug_vit_group_stats": (C.c_int, [C.c_void_p, C.c_size_t, C.c_int64, C.c_int32, C.c_int32, C.c_float, C.c_void_p, C.c_size_t, C.c_void_p]),
    "mra_debug_vit_row_stats": (C.c_int, [C.c_void_p, C.c_size_t, C.c_int32, C.c_int64, C.c_int32, C.c_float, C.c_void_p, C.c_size_t, C.c_void_p,
                                          C.c_size_t, C.c_int32, C.c_void_p]),
}

# GemmFamily / GemmEpi codes of mra_debug_gemm_launches (csrc/kernels.h)
GF_V1_64, GF_V1_128, GF_WS_256, GF_P8_256, GF_WS_128x384, GF_WS_176x384, GF_K128_64x128, GF_P8_TAIL, GF_P8_MIXED, GF_K128_64x64 = 0, 1, 3, 4, 5, 6, 7, 8, 9, 10
GF_RING_144x128, GF_RING_192x128, GF_RING_96x64 = 11, 12, 13                         # gemm_ring_kernel: the layer chain's exact-fit tiles
GEMM_FAMILIES = 14
EPI_OP, EPI_GELU_OP, EPI_RES_F32, EPI_F32, EPI_KV, EPI_SOFTPART, EPI_RES_OP = 0, 1, 2, 3, 4, 5, 8
EPI_RES_F32_STAT, EPI_LNF_OP, EPI_LNF_GELU_OP, EPI_RES_OP_STAT = 10, 11, 12, 13     # the ViT's folded LayerNorms (csrc/kernels.h)
EPI_GELU_BOTH, EPI_GELU_BWD = 6, 7                                                   # the training step's feed-forward epilogues
EPI_RES_LN = 9                                                                       # EPI_RES_F32 + the LayerNorm of the finished rows (ring 96 x 64)
GT_AUTO, GT_64, GT_128, GT_256 = 0, 1, 2, 3                                          # GemmTile codes mra_debug_gemm_gelu takes
GT_WS_128x384, GT_WS_176x384, GT_K128_64x128, GT_P8_TAIL, GT_P8_MIXED = 4, 5, 6, 7, 8   # ... and the further ones of mra_debug_gemm
GT_RING_144x128, GT_RING_192x128, GT_RING_96x64 = 9, 10, 11
GEMM_TN_MAX_JOBS = 4


def gemm_launches(family: int, epi: int) -> int:
    return int(lib().mra_debug_gemm_launches(family, epi))

_lib = None


class MraError(RuntimeError):
    pass


def lib() -> C.CDLL:
    """The loaded extension; raises (never falls back) when it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise MraError(
                f"{LIB_PATH} is missing: build the HIP extension first "
                "(python -c 'import __graft_entry__ as g; g.build()' or make -C mraudio_amd/csrc). "
                "mraudio_amd has no CPU fallback."
            )
        handle = C.CDLL(LIB_PATH)
        for name, (res, args) in PROTOTYPES.items():
            fn = getattr(handle, name)
            fn.restype = res
            fn.argtypes = args
        _lib = handle
    return _lib


def check(rc: int, what: str) -> None:
    if rc != 0:
        msg = lib().mra_last_error().decode("utf-8", "replace")
        raise MraError(f"{what}: {_ERR.get(rc, rc)}: {msg}")


def ptr(t) -> C.c_void_p:
    """Device (or host) address of a tensor, None -> NULL."""
    return C.c_void_p(0 if t is None else t.data_ptr())


def current_stream() -> C.c_void_p:
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def mra_dtype(dt: torch.dtype) -> int:
    if dt == torch.float32:
        return MRA_F32
    if dt == torch.float16:
        return MRA_F16
    if dt == torch.bfloat16:
        return MRA_BF16
    raise MraError(f"unsupported dtype {dt}")


def torch_dtype(code: int) -> torch.dtype:
    return {MRA_F32: torch.float32, MRA_F16: torch.float16, MRA_BF16: torch.bfloat16}[code]
