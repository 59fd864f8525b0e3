"""ctypes binding of libarchi_hip.so (include/archi_knn.h).

There is no CPU fallback: if the HIP library is missing or no gfx950 device is
visible, every entry point raises. The oracle under oracle/ is test
infrastructure and is never imported from here.
"""
from __future__ import annotations

import ctypes
import os
import threading

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libarchi_hip.so")

DTYPES = {"f32": 0, "bf16": 1, "f16": 2}
# store-level metric names (postgres_vectorstore.py:74-78) -> AK_METRIC_*
METRICS = {"cosine": 0, "l2": 1, "inner_product": 2}
SEARCH_MODES = {"auto": 0, "exact": 1, "fast_only": 2}
POOLING = {"mean": 0, "cls": 1, "last": 2}      # AK_POOL_*; "last": ak_llama_forward_lens and ak_qwen2_forward_lens only


class HipBackendError(RuntimeError):
    """Raised when the HIP backend is unavailable or a call fails."""


class StaleFilterError(HipBackendError):
    """A search was handed a row_filter built for another layout of the index (AK_ERR_STALE_FILTER): a writer added rows
    or reclaimed tombstones between the mask's construction and the search. Rebuild the mask and retry."""


ERR_STALE_FILTER = -11
ERR_COMM_BROKEN = -13
ABI_VERSION = 5          # AK_ABI_VERSION of include/archi_knn.h this binding was written against

# switches that exist only in libarchi_hip_dbg.so (`make -C archi_amd/csrc dbg`): instrumented kernels, stage-skipping
# ablations (WRONG RESULTS) and the superseded kernel generations kept as A/B references. One of them in the environment --
# or ARCHI_HIP_DBG=1 -- makes load() pick that library.
DBG_SWITCHES = ("AK_SCAN_DBG", "AK_SCAN_ABLATE", "AK_FFN_DBG", "AK_FFN_ABLATE", "AK_TAIL_ABLATE", "AK_QKV_DBG", "AK_GEMM_ABLATE",
                "AK_ENC_NOFFN", "AK_FFN_W8", "AK_FFN_PAIR", "AK_FFN_ATT", "AK_ATTN_DBG")


class AkBertConfig(ctypes.Structure):
    _fields_ = [
        ("vocab_size", ctypes.c_int),
        ("hidden", ctypes.c_int),
        ("layers", ctypes.c_int),
        ("heads", ctypes.c_int),
        ("intermediate", ctypes.c_int),
        ("max_position", ctypes.c_int),
        ("type_vocab", ctypes.c_int),
        ("ln_eps", ctypes.c_float),
        ("residual_bf16", ctypes.c_int),
        ("precision", ctypes.c_int),
    ]


class AkDecoderConfig(ctypes.Structure):
    _fields_ = [
        ("vocab_size", ctypes.c_int),
        ("hidden", ctypes.c_int),
        ("layers", ctypes.c_int),
        ("q_heads", ctypes.c_int),
        ("kv_heads", ctypes.c_int),
        ("head_dim", ctypes.c_int),
        ("intermediate", ctypes.c_int),
        ("max_position", ctypes.c_int),
        ("rms_eps", ctypes.c_float),
        ("rope_theta", ctypes.c_float),
    ]


MBERT_MAX_LAYERS = 64     # AK_MBERT_MAX_LAYERS


class AkModernBertConfig(ctypes.Structure):
    _fields_ = [
        ("vocab_size", ctypes.c_int),
        ("hidden", ctypes.c_int),
        ("layers", ctypes.c_int),
        ("heads", ctypes.c_int),
        ("intermediate", ctypes.c_int),
        ("max_position", ctypes.c_int),
        ("norm_eps", ctypes.c_float),
        ("global_rope_theta", ctypes.c_float),
        ("local_rope_theta", ctypes.c_float),
        ("half_window", ctypes.c_int),
        ("layer_global", ctypes.c_int * MBERT_MAX_LAYERS),
    ]


GEMMA_MAX_LAYERS = 64     # AK_GEMMA_MAX_LAYERS


class AkGemmaConfig(ctypes.Structure):
    _fields_ = [
        ("vocab_size", ctypes.c_int),
        ("hidden", ctypes.c_int),
        ("layers", ctypes.c_int),
        ("q_heads", ctypes.c_int),
        ("kv_heads", ctypes.c_int),
        ("head_dim", ctypes.c_int),
        ("intermediate", ctypes.c_int),
        ("max_position", ctypes.c_int),
        ("rms_eps", ctypes.c_float),
        ("global_rope_theta", ctypes.c_float),
        ("local_rope_theta", ctypes.c_float),
        ("query_pre_attn_scalar", ctypes.c_float),
        ("half_window", ctypes.c_int),
        ("attn_softcap", ctypes.c_float),
        ("final_softcap", ctypes.c_float),
        ("rope_type", ctypes.c_int),
        ("activation", ctypes.c_int),
        ("attention_bias", ctypes.c_int),
        ("n_dense", ctypes.c_int),
        ("dense_out", ctypes.c_int * 2),
        ("layer_global", ctypes.c_int * GEMMA_MAX_LAYERS),
    ]


class AkNomicBertConfig(ctypes.Structure):
    _fields_ = [
        ("vocab_size", ctypes.c_int),
        ("hidden", ctypes.c_int),
        ("layers", ctypes.c_int),
        ("heads", ctypes.c_int),
        ("intermediate", ctypes.c_int),
        ("type_vocab", ctypes.c_int),
        ("max_position", ctypes.c_int),
        ("ln_eps", ctypes.c_float),
        ("rope_theta", ctypes.c_float),
    ]


class AkT5Config(ctypes.Structure):
    _fields_ = [
        ("vocab_size", ctypes.c_int),
        ("hidden", ctypes.c_int),
        ("layers", ctypes.c_int),
        ("heads", ctypes.c_int),
        ("head_dim", ctypes.c_int),
        ("d_ff", ctypes.c_int),
        ("gated", ctypes.c_int),
        ("max_distance", ctypes.c_int),
        ("ln_eps", ctypes.c_float),
        ("n_dense", ctypes.c_int),
        ("dense_out", ctypes.c_int * 2),
    ]


class AkLlamaConfig(ctypes.Structure):
    _fields_ = [
        ("vocab_size", ctypes.c_int),
        ("hidden", ctypes.c_int),
        ("layers", ctypes.c_int),
        ("q_heads", ctypes.c_int),
        ("kv_heads", ctypes.c_int),
        ("head_dim", ctypes.c_int),
        ("intermediate", ctypes.c_int),
        ("max_position", ctypes.c_int),
        ("rms_eps", ctypes.c_float),
        ("rope_theta", ctypes.c_float),
        ("sliding_window", ctypes.c_int),
        ("bidirectional", ctypes.c_int),
    ]


class AkQwen2Config(ctypes.Structure):
    _fields_ = [
        ("vocab_size", ctypes.c_int),
        ("hidden", ctypes.c_int),
        ("layers", ctypes.c_int),
        ("q_heads", ctypes.c_int),
        ("kv_heads", ctypes.c_int),
        ("head_dim", ctypes.c_int),
        ("intermediate", ctypes.c_int),
        ("max_position", ctypes.c_int),
        ("rms_eps", ctypes.c_float),
        ("rope_theta", ctypes.c_float),
        ("bidirectional", ctypes.c_int),
    ]


_lock = threading.Lock()
_lib = None
_inited_device = None

# every symbol include/archi_knn.h declares: (name, restype, argtypes)
_P, _I, _I64, _U64, _U32, _D = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_double
SYMBOLS = [
    ("ak_last_error", ctypes.c_char_p, []),
    ("ak_version", ctypes.c_char_p, []),
    ("ak_abi_version", _I, []),
    ("ak_debug_set", _I, [ctypes.c_char_p, ctypes.c_char_p]),
    ("ak_init", _I, [_I]),
    ("ak_device_info", _I, [ctypes.c_char_p, _I, ctypes.POINTER(_I), ctypes.POINTER(_I64)]),
    ("ak_sync", _I, [_P]),
    ("ak_index_create", _I, [_I64, _I, _I, _I, ctypes.POINTER(_P)]),
    ("ak_index_destroy", _I, [_P]),
    ("ak_index_add", _I, [_P, _P, _I, _I64, _P, _I]),
    ("ak_index_generate", _I, [_P, _U64, _U32, _U64, _I64, _I, _I64]),
    ("ak_index_remove", _I, [_P, _P, _I64, ctypes.POINTER(_I64)]),
    ("ak_index_count", _I, [_P, ctypes.POINTER(_I64)]),
    ("ak_index_fetch", _I, [_P, _P, _I64, _P]),
    ("ak_index_lookup", _I, [_P, _P, _I64, _P]),
    ("ak_index_distances", _I, [_P, _P, _P, _I64, _P, _P]),
    ("ak_index_search", _I, [_P, _P, _I, _I, _I, _P, _I64, _U64, _P, _P, _P, _P]),
    ("ak_index_mmr_search", _I, [_P, _P, _I, _I, _I, _D, _I, _P, _I64, _U64, _P, _P, _P, _P, _P]),
    ("ak_index_group_search", _I, [_P, _P, _I, _I, _I, _I, _P, _P, _I64, _U64, _P, _P, _P, _P, _P, _P]),
    ("ak_index_lex_attach", _I, [_P, _P, _I64, _P, _P, _P, _P, _U64]),
    ("ak_index_lex_clear", _I, [_P, _U64]),
    ("ak_index_lex_info", _I, [_P, ctypes.POINTER(_U64), ctypes.POINTER(_I64), ctypes.POINTER(_I64), ctypes.POINTER(_I64)]),
    ("ak_index_lex_scores", _I, [_P, _P, _I, _D, _D, _D, _P, _P, _P]),
    ("ak_index_hybrid_search", _I, [_P, _P, _P, _I, _D, _D, _D, _D, _D, _P, _I64, _P, _I64, _U64, _I, _P, _P, ctypes.POINTER(_I),
                                    _P, _P, ctypes.POINTER(_I), _P]),
    ("ak_index_hybrid_search_batch", _I, [_P, _P, _I, _P, _P, _D, _D, _D, _D, _D, _P, _I64, _P, _I64, _U64, _I, _P, _P, _P, _P, _P, _P, _P]),
    ("ak_index_search_dev", _I, [_P, _P, _I, _I, _I, _P, _I64, _U64, _P, _P, _P, _P]),
    ("ak_index_slots", _I, [_P, ctypes.POINTER(_I64), ctypes.POINTER(_I64), ctypes.POINTER(_U64)]),
    ("ak_index_compact", _I, [_P, ctypes.POINTER(_I64)]),
    ("ak_index_scan_plan", _I, [_P, _I, _I, _P]),
    ("ak_index_i8_info", _I, [_P, _P]),
    ("ak_index_debug_read", _I, [_P, _P, _I]),
    ("ak_index_profile", _I, [_P, _I]),
    ("ak_index_profile_read", _I, [_P, _P, _I, ctypes.POINTER(_I)]),
    ("ak_merge_topk_dev", _I, [_I, _I, _I, _P, _P, _P, _P, _P]),
    ("ak_merge_shards_dev", _I, [_I, _I, _I, _P, _I64, _P, _P, _P, _P]),
    ("ak_comm_unique_id", _I, [_P]),
    ("ak_comm_create", _I, [_P, _I, _I, ctypes.POINTER(_P)]),
    ("ak_comm_destroy", _I, [_P]),
    ("ak_index_search_sharded_dev", _I, [_P, _P, _P, _I, _I, _P, _I64, _U64, _P, _P, ctypes.POINTER(_I64), _P]),
    ("ak_shard_payload_begin_dev", _I, [_P, _I, _I, _P]),
    ("ak_shard_fail_payload_dev", _I, [_P, _I, _I, _I, _P]),
    ("ak_shard_status_dev", _I, [_I, _P, _I64, _P, _P]),
    ("ak_shard_gather_rows_dev", _I, [_P, _P, _I, _I, _P, _P]),
    ("ak_shard_scatter_topk_dev", _I, [_P, _I, _I, _P, _P, _P, _P, _P]),
    ("ak_l2_normalize_dev", _I, [_P, _I64, _I, _P]),
    ("ak_encoder_create", _I, [ctypes.POINTER(AkBertConfig), _P, _I, ctypes.POINTER(_P)]),
    ("ak_encoder_destroy", _I, [_P]),
    ("ak_encoder_forward", _I, [_P, _P, _P, _I, _I, _I, _I, _P, _P]),
    ("ak_encoder_forward_lens", _I, [_P, _P, _I, _P, _I, _I, _I, _I, _I, _P, _P]),
    ("ak_encoder_gelu_table", _I, [_P]),
    ("ak_encoder_set_rel_bias", _I, [_P, _P, _I, _I]),
    ("ak_encoder_set_positions_from_ids", _I, [_P, _I, _I]),
    ("ak_decoder_create", _I, [ctypes.POINTER(AkDecoderConfig), _P, _I, ctypes.POINTER(_P)]),
    ("ak_decoder_destroy", _I, [_P]),
    ("ak_decoder_forward_lens", _I, [_P, _P, _I, _P, _I, _I, _I, _I, _P, _P]),
    ("ak_decoder_rope_table", _I, [ctypes.c_float, _I, _I, _P, _P]),
    ("ak_decoder_rope_table_inv", _I, [_P, _I, _I, _P, _P]),
    ("ak_mbert_create", _I, [ctypes.POINTER(AkModernBertConfig), _P, _I, ctypes.POINTER(_P)]),
    ("ak_mbert_destroy", _I, [_P]),
    ("ak_mbert_forward_lens", _I, [_P, _P, _I, _P, _I, _I, _I, _I, _I, _P, _P]),
    ("ak_gemma_create", _I, [ctypes.POINTER(AkGemmaConfig), _P, _I, ctypes.POINTER(_P)]),
    ("ak_gemma_destroy", _I, [_P]),
    ("ak_gemma_set_rope_inv_freq", _I, [_P, _P, _P]),
    ("ak_gemma_forward_lens", _I, [_P, _P, _I, _P, _I, _I, _I, _I, _I, _P, _P]),
    ("ak_nomic_create", _I, [ctypes.POINTER(AkNomicBertConfig), _P, _I, ctypes.POINTER(_P)]),
    ("ak_nomic_destroy", _I, [_P]),
    ("ak_nomic_forward_lens", _I, [_P, _P, _I, _P, _I, _I, _I, _I, _I, _P, _P]),
    ("ak_t5_create", _I, [ctypes.POINTER(AkT5Config), _P, _I, ctypes.POINTER(_P)]),
    ("ak_t5_destroy", _I, [_P]),
    ("ak_t5_forward_lens", _I, [_P, _P, _I, _P, _I, _I, _I, _I, _I, _P, _P]),
    ("ak_llama_create", _I, [ctypes.POINTER(AkLlamaConfig), _P, _I, ctypes.POINTER(_P)]),
    ("ak_llama_destroy", _I, [_P]),
    ("ak_llama_set_rope_inv_freq", _I, [_P, _P]),
    ("ak_llama_forward_lens", _I, [_P, _P, _I, _P, _I, _I, _I, _I, _I, _P, _P]),
    ("ak_qwen2_create", _I, [ctypes.POINTER(AkQwen2Config), _P, _I, ctypes.POINTER(_P)]),
    ("ak_qwen2_destroy", _I, [_P]),
    ("ak_qwen2_set_rope_inv_freq", _I, [_P, _P]),
    ("ak_qwen2_forward_lens", _I, [_P, _P, _I, _P, _I, _I, _I, _I, _I, _P, _P]),
    ("ak_wordpiece_create", _I, [ctypes.c_char_p, _I, ctypes.POINTER(_P)]),
    ("ak_wordpiece_create_ex", _I, [ctypes.c_char_p, _I, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_char_p,
                                    ctypes.POINTER(ctypes.c_char_p), _I, ctypes.POINTER(_P)]),
    ("ak_wordpiece_destroy", _I, [_P]),
    ("ak_wordpiece_encode", _I, [_P, _P, _P, _I64, _I, _I, _P, _P]),
]


class AkKtGemm(ctypes.Structure):
    """Argument block of ak_kt_gemm (csrc/kernel_test.hip): the GemmArgs fields that modes 0, 1, 2, 4, 7 and 8 read."""
    _fields_ = [
        ("X", _P), ("W", _P), ("bias", _P),
        ("T", _I), ("N", _I), ("K", _I),
        ("out_bf16", _P), ("ldo", _I),
        ("out_f32", _P),
        ("res16", _P),
        ("q", _P), ("k", _P), ("vt", _P), ("H", _I), ("S", _I), ("qscale", ctypes.c_float),
    ]


class AkKtGemmLazy(ctypes.Structure):
    """Argument block of ak_kt_gemm_lazy (csrc/kernel_test.hip): the GemmArgs fields the lazy-LayerNorm modes 0, 1 and 4 read."""
    _fields_ = [
        ("X", _P), ("W", _P), ("bias", _P),
        ("T", _I), ("N", _I), ("K", _I),
        ("out_bf16", _P), ("ldo", _I),
        ("res16", _P),
        ("q", _P), ("k", _P), ("vt", _P), ("H", _I), ("S", _I), ("qscale", ctypes.c_float),
        ("fold_c", _P), ("a_stats", _P), ("res_stats", _P), ("res_g", _P), ("res_b", _P), ("out_g", _P),
        ("out_stats", _P),
        ("nslot", _I), ("inv_h", ctypes.c_float), ("eps", ctypes.c_float),
    ]


# single-launch entry points for the kernel-level tests (csrc/kernel_test.hip): libarchi_hip_dbg.so only, bound only when
# load() picked that library. They are not part of include/archi_knn.h.
KT_SYMBOLS = [
    ("ak_kt_attn", _I, [_P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _P, _P, _P, _I, _P]),
    ("ak_kt_attn_long", _I, [_P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _P]),
    ("ak_kt_attn_window", _I, [_P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _P]),
    ("ak_kt_attn_causal", _I, [_P, _P, _P, _P, _P, _I, _I, _I, _I, _P]),
    ("ak_kt_gemm", _I, [_I, ctypes.POINTER(AkKtGemm), _P]),
    ("ak_kt_gemm_skinny", _I, [_P, _P, _P, _I, _I, _I, _P, _P, _I, _P]),
    ("ak_kt_gemm_skinny_qkv", _I, [_P, _P, _P, _I, _I, _I, _P, _P, _P, _I, _I, ctypes.c_float, _P]),
    ("ak_kt_vt_pos", _I, [_I]),
    ("ak_kt_gemm_ln", _I, [_P, _P, _P, _P, _P, _P, _P, _I, _I, ctypes.c_float, _P]),
    ("ak_kt_ffn384_weight_bytes", _I64, [_I]),
    ("ak_kt_ffn384", _I, [_P] * 13 + [_I, _I, ctypes.c_float, _P]),
    ("ak_kt_qkv384_weight_bytes", _I64, []),
    ("ak_kt_qkv384", _I, [_P] * 7 + [_I, _I, _I, ctypes.c_float, _I, _P]),
    ("ak_kt_gemm_lazy", _I, [_I, ctypes.POINTER(AkKtGemmLazy), _P]),
    ("ak_kt_ln_finalize", _I, [_P, _I, _I64, ctypes.c_float, ctypes.c_float, _P, _P]),
    ("ak_kt_fold_ln", _I, [_P, _P, _P, _P, _I, _I, _P, _P, _P]),
    ("ak_kt_layernorm", _I, [_P, _P, _P, _P, _P, _I, _I, ctypes.c_float, _P, _P, _P, _P]),
    ("ak_kt_layernorm16", _I, [_P, _P, _P, _I, _I, ctypes.c_float, _P, _P]),
    ("ak_kt_ln_apply16", _I, [_P, _P, _P, _P, _I64, _I, _P, _P]),
]

# the EmbeddingGemma kernels' single-launch entry points (tests/test_gemma_kernels_gpu.py): libarchi_hip_dbg.so only, like
# KT_SYMBOLS, and a set of their own (ak_ktg_*)
KTG_SYMBOLS = [
    ("ak_ktg_attn_gqa", _I, [_P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _P]),
    ("ak_ktg_qk_norm_rope", _I, [_P, _I, _I, _I, _I, _P, _P, ctypes.c_float, _P, _P, ctypes.c_float, _P, _P, _P, _P]),
    ("ak_ktg_gemm_geglu_tanh", _I, [_P, _P, _P, _I, _I, _I, _P, _P]),
]

# the small kernels of the stacks (decoder128.hip, mbert.hip, nomic.hip, gemma.hip) and k_gemm MODE 3, one launch each
# (tests/test_stack_kernels_gpu.py, tests/test_llama_kernels_gpu.py): libarchi_hip_dbg.so only, a third set of its own (ak_kts_*)
_F = ctypes.c_float
_EMBED = [_P, _I, _P, _I, _I, _I, _I, _I, _P, _P, _F, _P, _P]
KTS_SYMBOLS = [
    ("ak_kts_dec_embed", _I, _EMBED + [_P, _P]),
    ("ak_kts_dec_add_rmsnorm", _I, [_P, _P, _I64, _I, _P, _F, _P, _P]),
    ("ak_kts_dec_qk_rope", _I, [_P, _I, _I, _I, _I, _P, _P, _F, _P, _P, _F, _P, _P, _P, _P]),
    ("ak_kts_dec_pool", _I, [_P, _P, _I, _I, _I, _P, _F, _I, _P, _P]),
    ("ak_kts_mb_embed", _I, _EMBED + [_P, _P, _P]),
    ("ak_kts_mb_add_ln", _I, [_P, _P, _I64, _I, _P, _F, _P, _P]),
    ("ak_kts_mb_rope", _I, [_P, _P, _I64, _I, _I, _P, _P, _P]),
    ("ak_kts_mb_pool", _I, [_P, _P, _I, _I, _I, _F, _P, _I, _I, _P, _P, _P]),
    ("ak_kts_nb_embed", _I, [_P, _I, _P, _I, _I, _I, _I, _I, _P, _P, _P, _P, _F, _P, _P, _P, _P, _P]),
    ("ak_kts_nb_add_ln", _I, [_P, _P, _I64, _I, _P, _P, _F, _P, _P]),
    ("ak_kts_nb_pool", _I, [_P, _P, _I, _I, _I, _I, _I, _P, _P, _P]),
    ("ak_kts_gm_fold1p", _I, [_P, _I, _P, _P]),
    ("ak_kts_gm_embed", _I, _EMBED + [_P, _P]),
    ("ak_kts_gm_norm_add_norm", _I, [_P, _P, _I64, _I, _P, _P, _F, _P, _P, _P]),
    ("ak_kts_gm_pool", _I, [_P, _P, _I, _I, _I, _P, _P, _P]),
    ("ak_kts_gm_dense", _I, [_P, _P, _I, _I, _I, _P, _P]),
    ("ak_kts_gm_l2", _I, [_P, _I, _I, _I, _P, _P]),
    ("ak_kts_gemm_bf16", _I, [_P, _P, _P, _I, _I, _I, _P, _P]),
    ("ak_kts_ll_attn", _I, [_P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _P]),
    ("ak_kts_ll_pool", _I, [_P, _P, _I, _I, _I, _P, _F, _I, _P, _P, _P]),
    ("ak_kts_ll_rope", _I, [_P, _I, _I, _I, _I, _P, _P, _F, _P, _P, _P, _P]),
    ("ak_kts_q2_attn", _I, [_P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _P]),      # launch_attn_causal_split (tests/test_qwen2_kernels_gpu.py)
    ("ak_kts_t5_attn", _I, [_P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _P, _I, _P]),      # launch_attn_relbias (tests/test_t5_kernels_gpu.py)
    ("ak_kts_t5_gemm_relu", _I, [_P, _P, _P, _I, _I, _I, _P, _P]),                              # launch_gemm(10)
    # query_norms + one re-rank launch, which = 0 thread-per-candidate / 1 panel (tests/test_rerank_panel_gpu.py); the kernel rerank() picks
    ("ak_kts_rr_rerank", _I, [_P, _P, _I, _I, _P, _P, _P, _P, _I, _P]),
    ("ak_kts_rr_choice", _I, [_P]),
]

# the float32 and split-bf16 parity modes' launchers, one launch each (tests/test_parity_kernels_gpu.py): libarchi_hip_dbg.so only, a
# fourth set of its own (ak_ktp_*)
KTP_SYMBOLS = [
    ("ak_ktp_gemm_f32", _I, [_I, _P, _P, _P, _P, _I, _I, _I, _P, _I, _I, _P]),
    ("ak_ktp_gemm_x3", _I, [_I, _P, _P, _P, _P, _P, _I, _I, _I, _P, _I, _I, _P]),
    ("ak_ktp_gemm_f32_scalar", _I, [_I, _P, _P, _P, _I, _I, _I, _P, _P]),      # k32_gemm, the cross-check k32m_gemm's comment names
    ("ak_ktp_attn_f32", _I, [_P, _P, _I, _I, _I, _I, _P, _P, _P]),
    ("ak_ktp_attn_x3", _I, [_P, _P, _I, _I, _I, _I, _P, _P, _P]),
    ("ak_ktp_attn_x3_split", _I, [_P, _I, _P, _I, _I, _I, _I, _P, _P, _P]),
    ("ak_ktp_split_hilo", _I, [_P, _I64, _P, _P, _P]),
    ("ak_ktp_split_rows", _I, [_P, _I64, _I, _P, _P]),
    ("ak_ktp_embed_split", _I, [_P, _I64, _I, _I, _I, _P, _P, _P, _P, _P, _F, _P, _P, _P, _P]),
    ("ak_ktp_add_ln_split", _I, [_P, _I, _P, _I64, _I, _P, _P, _F, _P, _P, _P]),
    ("ak_ktp_embed_f32", _I, [_P, _I64, _I, _I, _I, _P, _P, _P, _P, _P, _F, _P, _P, _P]),
    ("ak_ktp_add_ln_f32", _I, [_P, _P, _I64, _I, _P, _P, _F, _P, _P]),
    ("ak_ktp_pool_f32", _I, [_P, _P, _I, _I, _I, _I, _I, _P, _P]),
    ("ak_ktp_gemm_x3w", _I, [_I, _P, _P, _P, _I, _I, _I, _P, _P, _I, _P]),
    ("ak_ktp_gemm_ln_x3", _I, [_P, _P, _P, _P, _P, _P, _P, _I, _I, _F, _P]),
]


def load() -> ctypes.CDLL:
    """dlopen the library and bind every declared symbol (no GPU needed)."""
    global _lib
    with _lock:
        if _lib is None:
            # torch ships its own libamdhip64.so.7 + libhsa-runtime64; two HIP runtimes in one
            # process cannot both open the GPU. Loading torch's first makes the dynamic loader
            # resolve our NEEDED libamdhip64.so.7 to the copy torch already mapped.
            import torch  # noqa: F401
            # measurement switches select the library that carries the instrumented kernel instantiations (`make dbg`)
            path = LIB_PATH
            if os.environ.get("ARCHI_HIP_DBG") or any(os.environ.get(v) for v in DBG_SWITCHES) or \
                    os.environ.get("AK_ATTN_STREAM", "") in ("3", "4"):
                dbg = os.path.join(_HERE, "lib", "libarchi_hip_dbg.so")
                if not os.path.exists(dbg):
                    raise HipBackendError(f"{dbg} not found: the instrumented kernels are built by `make -C archi_amd/csrc dbg`")
                path = dbg
            if not os.path.exists(LIB_PATH):
                raise HipBackendError(
                    f"{LIB_PATH} not found: build it with `make -C archi_amd/csrc` "
                    "(or __graft_entry__.build()); archi_amd has no CPU fallback")
            lib = ctypes.CDLL(path)
            for name, res, args in SYMBOLS:
                fn = getattr(lib, name)  # AttributeError if the .so lacks a declared symbol
                fn.restype = res
                fn.argtypes = args
            if path != LIB_PATH:
                for name, res, args in KT_SYMBOLS + KTG_SYMBOLS + KTS_SYMBOLS + KTP_SYMBOLS:
                    fn = getattr(lib, name)
                    fn.restype = res
                    fn.argtypes = args
            got = lib.ak_abi_version()
            if got != ABI_VERSION:
                raise HipBackendError(f"{path}: ABI version {got}, this binding expects {ABI_VERSION} "
                                      "(rebuild with `make -C archi_amd/csrc`; signatures moved between the two)")
            _lib = lib
    return _lib


def is_dbg_library() -> bool:
    """True when load() picked libarchi_hip_dbg.so (the A/B reference kernels and the stage-skipping switches live there)."""
    lib = load()
    return bool(getattr(lib, "_name", "").endswith("libarchi_hip_dbg.so"))


def debug_set(name: str, value: str | None) -> None:
    """Set one of the library's measurement switches for this process (ak_debug_set): the library reads its environment once,
    so a test or probe that wants another scan tile mid-process says so here. None restores the default."""
    check(load().ak_debug_set(name.encode(), None if value is None else str(value).encode()), f"ak_debug_set({name})")


def last_error() -> str:
    return (load().ak_last_error() or b"").decode("utf-8", "replace")


def check(rc: int, what: str) -> None:
    if rc == ERR_STALE_FILTER:
        raise StaleFilterError(f"{what}: {last_error()}")
    if rc != 0:
        raise HipBackendError(f"{what} failed (rc={rc}): {last_error()}")


def init(device: int | None = None) -> ctypes.CDLL:
    """Bind this process to one GPU (one process per GPU). LOCAL_RANK selects it by default."""
    global _inited_device
    lib = load()
    if device is None:
        device = int(os.environ.get("LOCAL_RANK", "0")) if _inited_device is None else _inited_device
    if _inited_device != device:
        check(lib.ak_init(device), "ak_init")
        _inited_device = device
    return lib


def bound_device() -> int:
    """The GPU this process is bound to (ak_init's device; one process per GPU). torch tensors and streams handed to
    the C ABI must live on THIS device -- torch.cuda.current_device() is a per-thread default that a torchrun rank > 0
    process may never have set."""
    if _inited_device is None:
        raise HipBackendError("libarchi_hip is not initialised: call archi_amd._lib.init() first")
    return _inited_device
