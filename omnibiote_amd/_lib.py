"""ctypes binding of libomnibiote_hip.so (C ABI: include/omnibiote_hip.h).

Loaded lazily and exactly once; a missing or unloadable library is a hard error (there is no fallback path).
"""
from __future__ import annotations

import ctypes as C
import os
import threading

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("OBTE_LIB_PATH") or os.path.join(_HERE, "libomnibiote_hip.so")   # override: A/B builds

c_bf16_p = C.c_void_p
c_f32_p = C.c_void_p
c_stream = C.c_void_p


class GemmArgs(C.Structure):
    _fields_ = [("a", C.c_void_p), ("b", C.c_void_p), ("d", C.c_void_p), ("aux", C.c_void_p), ("d2", C.c_void_p),
                ("M", C.c_int64), ("N", C.c_int64), ("K", C.c_int64),
                ("lda", C.c_int64), ("ldb", C.c_int64), ("ldd", C.c_int64),
                ("a_kmajor", C.c_int32), ("b_kmajor", C.c_int32), ("epilogue", C.c_int32), ("alpha", C.c_float),
                ("dropout_p", C.c_float), ("dropout_site", C.c_int32), ("dropout_seed", C.c_uint64),
                ("rope_cos", C.c_void_p), ("rope_sin", C.c_void_p), ("rope_T", C.c_int64), ("rope_head_dim", C.c_int32),
                ("acc32", C.c_void_p), ("acc32_mode", C.c_int32)]


class AttnFwdArgs(C.Structure):
    _fields_ = [("qkv", C.c_void_p), ("o", C.c_void_p), ("lse", C.c_void_p),
                ("key_ranges", C.c_void_p), ("mask", C.c_void_p),
                ("mask_sb", C.c_int64), ("mask_sh", C.c_int64), ("mask_sq", C.c_int64),
                ("B", C.c_int64), ("T", C.c_int64), ("n_head", C.c_int32), ("head_dim", C.c_int32), ("scale", C.c_float),
                ("dropout_p", C.c_float), ("dropout_seed", C.c_uint64), ("ranges_exact", C.c_void_p), ("drop_bits", C.c_void_p)]


class AttnBwdArgs(C.Structure):
    _fields_ = [("qkv", C.c_void_p), ("o", C.c_void_p), ("d_o", C.c_void_p), ("lse", C.c_void_p),
                ("delta", C.c_void_p), ("dqkv", C.c_void_p), ("rope_cos", C.c_void_p), ("rope_sin", C.c_void_p),
                ("key_ranges", C.c_void_p), ("mask", C.c_void_p),
                ("mask_sb", C.c_int64), ("mask_sh", C.c_int64), ("mask_sq", C.c_int64),
                ("B", C.c_int64), ("T", C.c_int64), ("n_head", C.c_int32), ("head_dim", C.c_int32), ("scale", C.c_float),
                ("dropout_p", C.c_float), ("dropout_seed", C.c_uint64), ("query_bounds", C.c_void_p), ("ranges_exact", C.c_void_p),
                ("ws", C.c_void_p), ("ws_bytes", C.c_int64), ("drop_bits", C.c_void_p)]


class BlockDesc(C.Structure):
    _fields_ = [("B", C.c_int64), ("T", C.c_int64), ("n_embd", C.c_int32), ("n_head", C.c_int32),
                ("ln1_w", C.c_void_p), ("attn_w", C.c_void_p), ("proj_w", C.c_void_p),
                ("ln2_w", C.c_void_p), ("fc_w", C.c_void_p), ("mlp_w", C.c_void_p),
                ("rope_cos", C.c_void_p), ("rope_sin", C.c_void_p),
                ("key_ranges", C.c_void_p), ("mask", C.c_void_p),
                ("mask_sb", C.c_int64), ("mask_sh", C.c_int64), ("mask_sq", C.c_int64),
                ("dropout_p", C.c_float), ("dropout_seed", C.c_uint64), ("query_bounds", C.c_void_p),
                ("ln1_partials", C.c_void_p), ("ln2_partials", C.c_void_p), ("ln_partial_mode", C.c_int32),
                ("ranges_exact", C.c_void_p), ("out_rows", C.c_void_p), ("n_out_rows", C.c_int64),
                ("dy_masked", C.c_void_p), ("dx_masked", C.c_void_p), ("dx_mask_seed", C.c_uint64),
                ("attn_w_acc32", C.c_void_p), ("proj_w_acc32", C.c_void_p), ("fc_w_acc32", C.c_void_p), ("mlp_w_acc32", C.c_void_p),
                ("w_acc32_mode", C.c_int32)]


LN_PARTIAL_FIRST, LN_PARTIAL_MORE, LN_PARTIAL_LAST = 1, 2, 3
ACC32_FIRST, ACC32_MORE, ACC32_LAST = 1, 2, 3   # a gradient summed in fp32 over the passes of one optimizer step (OBTE_ACC32_*)
MT_MAX = 32
MT_CHUNK = 16384   # elements one workgroup of a multi-tensor launch serves (csrc/elementwise.hip)


class MtArgs(C.Structure):
    _fields_ = [("p", C.c_void_p * MT_MAX), ("g", C.c_void_p * MT_MAX), ("m", C.c_void_p * MT_MAX), ("v", C.c_void_p * MT_MAX),
                ("n", C.c_int64 * MT_MAX), ("lr", C.c_float * MT_MAX), ("weight_decay", C.c_float * MT_MAX),
                ("step", C.c_int32 * MT_MAX), ("count", C.c_int32),
                ("lr64", C.c_double * MT_MAX), ("weight_decay64", C.c_double * MT_MAX)]


class MtMasterArgs(C.Structure):
    _fields_ = [("p", C.c_void_p * MT_MAX), ("g", C.c_void_p * MT_MAX), ("master", C.c_void_p * MT_MAX), ("m", C.c_void_p * MT_MAX),
                ("v", C.c_void_p * MT_MAX), ("n", C.c_int64 * MT_MAX), ("lr", C.c_double * MT_MAX), ("weight_decay", C.c_double * MT_MAX),
                ("step", C.c_int32 * MT_MAX), ("count", C.c_int32)]


EPI_NONE, EPI_GELU, EPI_ADD, EPI_GELU_BWD, EPI_ADD_DROPOUT, EPI_ROPE_QK = 0, 1, 2, 3, 4, 5
EPI_ACC32 = 8
EPI_GELU_ACT = 9   # the activation alone: EPI_GELU's d2 as d, for a forward nobody will differentiate
ATTN_DECODE_MAX_SPLITS = 64   # OBTE_ATTN_DECODE_MAX_SPLITS
SITE_EMBED, SITE_ATTN, SITE_RESID, SITE_MLP, SITE_USER = 0, 1, 2, 3, 7

# name -> (restype, argtypes); every symbol include/omnibiote_hip.h declares
SYMBOLS = {
    "obte_abi_version": (C.c_int, []),
    "obte_last_error": (C.c_char_p, []),
    "obte_struct_sizes": (C.c_int, [C.c_void_p, C.c_int]),
    "obte_device_status": (C.c_int, [C.c_int]),
    "obte_fault_inject": (C.c_int, [C.c_int]),
    "obte_profile_enable": (C.c_int, [C.c_int]),
    "obte_profile_collect": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]),
    "obte_layernorm_fwd": (C.c_int, [C.c_void_p] * 5 + [C.c_int64, C.c_int, C.c_float, c_stream]),
    "obte_layernorm_bwd_ws_rows": (C.c_int, []),
    "obte_layernorm_bwd": (C.c_int, [C.c_void_p] * 9 + [C.c_int64, C.c_int, c_stream]),
    "obte_layernorm_bwd_acc": (C.c_int, [C.c_void_p] * 9 + [C.c_int64, C.c_int, C.c_int, c_stream]),
    "obte_layernorm_bwd_partial": (C.c_int, [C.c_void_p] * 9 + [C.c_int64, C.c_int, C.c_int, c_stream]),
    "obte_layernorm_bwd_dropout": (C.c_int, [C.c_void_p] * 10 + [C.c_int64, C.c_int, C.c_int, C.c_int, C.c_float, C.c_uint64, C.c_int32, c_stream]),
    "obte_gemm_bf16": (C.c_int, [C.POINTER(GemmArgs), c_stream]),
    "obte_gemm_workspace_bytes": (C.c_int64, [C.c_int64, C.c_int64, C.c_int64]),
    "obte_gemm_bf16_ws": (C.c_int, [C.POINTER(GemmArgs), C.c_void_p, C.c_int64, c_stream]),
    "obte_gemm_grouped_bf16": (C.c_int, [C.POINTER(GemmArgs), C.c_int, c_stream]),
    "obte_gemm_plan_set": (C.c_int, [C.c_int] * 3 + [C.c_int64] * 3 + [C.c_int] * 3),
    "obte_gemm_plan_clear": (C.c_int, []),
    "obte_rope_qk_inplace": (C.c_int, [C.c_void_p] * 3 + [C.c_int64, C.c_int64, C.c_int, C.c_int, C.c_int, c_stream]),
    "obte_attn_fwd": (C.c_int, [C.POINTER(AttnFwdArgs), c_stream]),
    "obte_mask_bounds": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_int64, C.c_int32, C.c_int64, C.c_void_p, C.c_void_p,
                                   C.c_void_p, C.c_void_p, C.c_void_p, c_stream]),
    "obte_attn_bwd": (C.c_int, [C.POINTER(AttnBwdArgs), c_stream]),
    "obte_attn_drop_bits_bytes": (C.c_int64, [C.c_int64, C.c_int64, C.c_int32]),
    "obte_attn_bwd_ws_bytes": (C.c_int64, [C.c_int64, C.c_int64, C.c_int32, C.c_int32]),
    "obte_attn_bwd_select": (C.c_int, [C.c_int]),
    "obte_embedding_fwd": (C.c_int, [C.c_void_p] * 3 + [C.c_int64, C.c_int, C.c_int64, c_stream]),
    "obte_embedding_fwd_dropout": (C.c_int, [C.c_void_p] * 3 + [C.c_int64, C.c_int, C.c_int64, C.c_float, C.c_uint64, c_stream]),
    "obte_embedding_bwd_dropout": (C.c_int, [C.c_void_p] * 5 + [C.c_int64, C.c_int, C.c_int64, C.c_int, C.c_float, C.c_uint64, c_stream]),
    "obte_dropout_bf16": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_float, C.c_uint64, C.c_int32, c_stream]),
    "obte_embedding_bwd_ws_bytes": (C.c_int64, [C.c_int64, C.c_int]),
    "obte_embedding_bwd": (C.c_int, [C.c_void_p] * 5 + [C.c_int64, C.c_int, C.c_int64, c_stream]),
    "obte_embedding_bwd_acc": (C.c_int, [C.c_void_p] * 5 + [C.c_int64, C.c_int, C.c_int64, C.c_int, c_stream]),
    "obte_embedding_bwd_acc32": (C.c_int, [C.c_void_p] * 6 + [C.c_int64, C.c_int, C.c_int64, C.c_int, C.c_float, C.c_uint64, c_stream]),
    "obte_acc32_add_bf16": (C.c_int, [C.c_void_p] * 3 + [C.c_int64, C.c_int, c_stream]),
    "obte_key_ranges_from_tokens": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_int, C.c_int64, C.c_void_p, c_stream]),
    "obte_token_order_ws_bytes": (C.c_int64, [C.c_int64, C.c_int64, C.c_int64]),
    "obte_token_order": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, c_stream]),
    "obte_masked_ce_fwd_bwd": (C.c_int, [C.c_void_p] * 4 + [C.c_float] + [C.c_void_p] * 3 + [C.c_int64, C.c_int64, c_stream]),
    "obte_masked_ce_fwd_bwd_reuse": (C.c_int, [C.c_void_p] * 5 + [C.c_float] + [C.c_void_p] * 2 + [C.c_int64, C.c_int64, c_stream]),
    "obte_rows_gather_bf16": (C.c_int, [C.c_void_p] * 3 + [C.c_int64, C.c_int64, C.c_int32, c_stream]),
    "obte_rows_scatter_bf16": (C.c_int, [C.c_void_p] * 3 + [C.c_int64, C.c_int64, C.c_int32, c_stream]),
    "obte_masked_ce_rows": (C.c_int, [C.c_void_p] * 4 + [C.c_float] + [C.c_void_p] * 3 + [C.c_int64, C.c_int64, C.c_int64, c_stream]),
    "obte_adamw_bf16": (C.c_int, [C.c_void_p] * 4 + [C.c_int64] + [C.c_float] * 5 + [C.c_int32, C.c_void_p, c_stream]),
    "obte_sumsq_bf16": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, c_stream]),
    "obte_adamw_multi_bf16": (C.c_int, [C.POINTER(MtArgs), C.c_float, C.c_float, C.c_float, C.c_void_p, c_stream]),
    "obte_sumsq_multi_bf16": (C.c_int, [C.POINTER(MtArgs), C.c_void_p, c_stream]),
    "obte_sumsq_multi_bf16_each": (C.c_int, [C.POINTER(MtArgs), C.c_void_p, c_stream]),
    "obte_adamw_multi_bf16_ref": (C.c_int, [C.POINTER(MtArgs), C.c_double, C.c_double, C.c_double, C.c_void_p, c_stream]),
    "obte_adamw_multi_master": (C.c_int, [C.POINTER(MtMasterArgs), C.c_double, C.c_double, C.c_double, C.c_void_p, c_stream]),
    "obte_sumsq_multi_partials_count": (C.c_int64, [C.POINTER(MtArgs)]),
    "obte_sumsq_multi_bf16_partials": (C.c_int, [C.POINTER(MtArgs), C.c_void_p, c_stream]),
    "obte_clip_coef_from_partials": (C.c_int, [C.c_void_p, C.c_int64, C.c_float, C.c_void_p, c_stream]),
    "obte_block_act_bytes": (C.c_int64, [C.c_int64, C.c_int64, C.c_int32, C.c_int32]),
    "obte_block_act_bytes_p": (C.c_int64, [C.c_int64, C.c_int64, C.c_int32, C.c_int32, C.c_float]),
    "obte_block_bwd_ws_bytes": (C.c_int64, [C.c_int64, C.c_int64, C.c_int32, C.c_int32]),
    "obte_block_fwd": (C.c_int, [C.POINTER(BlockDesc), C.c_void_p, C.c_void_p, C.c_void_p, c_stream]),
    "obte_block_infer_ws_bytes": (C.c_int64, [C.c_int64, C.c_int64, C.c_int32, C.c_int32]),
    "obte_block_fwd_infer": (C.c_int, [C.POINTER(BlockDesc), C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, c_stream]),
    "obte_block_bwd": (C.c_int, [C.POINTER(BlockDesc)] + [C.c_void_p] * 11 + [c_stream]),
    "obte_block_bwd_acc": (C.c_int, [C.POINTER(BlockDesc)] + [C.c_void_p] * 11 + [C.c_int, c_stream]),
    "obte_causal_bounds": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, c_stream]),
    "obte_kv_cache_bytes": (C.c_int64, [C.c_int64, C.c_int64, C.c_int32, C.c_int32]),
    "obte_kv_cache_store": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_int32, C.c_int32, C.c_void_p, C.c_int64, C.c_int64, c_stream]),
    "obte_attn_decode_ws_bytes": (C.c_int64, [C.c_int64, C.c_int32, C.c_int32]),
    "obte_attn_decode_splits": (C.c_int, [C.c_int64, C.c_int32, C.c_int32, C.c_int64]),
    "obte_attn_decode": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_int32, C.c_int32,
                                   C.c_float, C.c_int32, C.c_void_p, C.c_int64, c_stream]),
    "obte_block_fwd_prefill": (C.c_int, [C.POINTER(BlockDesc), C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, c_stream]),
    "obte_block_decode_ws_bytes": (C.c_int64, [C.c_int64, C.c_int32, C.c_int32]),
    "obte_block_decode": (C.c_int, [C.POINTER(BlockDesc), C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_int64, c_stream]),
}

# generation with one cache position per row (include/omnibiote_hip_rows.h): a table of its own, bound by lib() in the same loop —
# SYMBOLS is, name for name and in order, what include/omnibiote_hip.h declares
SYMBOLS_ROWS = {
    "obte_kv_cache_rope_store_rows": (C.c_int, [C.c_void_p] * 4 + [C.c_int64, C.c_int64, C.c_int32, C.c_int32, C.c_void_p, C.c_int64, c_stream]),
    "obte_attn_decode_rows": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_int64, C.c_int32,
                                        C.c_int32, C.c_float, C.c_int32, C.c_void_p, C.c_int64, c_stream]),
    "obte_block_decode_rows": (C.c_int, [C.POINTER(BlockDesc), C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64,
                                         c_stream]),
}

# the weight-streaming product for small M (include/omnibiote_hip_small_m.h): again a table of its own
SYMBOLS_SMALL_M = {
    "obte_linear_small_m_bf16": (C.c_int, [C.POINTER(GemmArgs), c_stream]),
    "obte_small_m_max_set": (C.c_int, [C.c_int]),
    "obte_small_m_max": (C.c_int, []),
}
SMALL_M_MAX_ROWS = 64   # the largest M obte_linear_small_m_bf16 takes

# next-token sampling on the device (include/omnibiote_hip_sample.h): a table of its own as well
SYMBOLS_SAMPLE = {
    "obte_sample_logits_bf16": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_void_p, C.c_float, C.c_int32, C.c_float, C.c_void_p, C.c_void_p,
                                          c_stream]),
}

# n new positions per row against a filled cache (include/omnibiote_hip_extend.h): a table of its own as well
ATTN_EXTEND_MAX_SPLITS = 32   # OBTE_ATTN_EXTEND_MAX_SPLITS
SYMBOLS_EXTEND = {
    "obte_attn_extend_splits": (C.c_int, [C.c_int64, C.c_int32, C.c_int32, C.c_int64, C.c_int64]),
    "obte_attn_extend_ws_bytes": (C.c_int64, [C.c_int64, C.c_int32, C.c_int32, C.c_int64, C.c_int32]),
    "obte_kv_cache_rope_store_chunk": (C.c_int, [C.c_void_p] * 4 + [C.c_int64, C.c_int64, C.c_int64, C.c_int32, C.c_int32, C.c_void_p, C.c_int64, c_stream]),
    "obte_attn_extend": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_int64, C.c_void_p, C.c_int32,
                                   C.c_int32, C.c_float, C.c_int32, C.c_void_p, C.c_int64, c_stream]),
    "obte_block_extend_ws_bytes": (C.c_int64, [C.c_int64, C.c_int64, C.c_int32, C.c_int32]),
    "obte_block_extend": (C.c_int, [C.POINTER(BlockDesc), C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, c_stream]),
}

# speculative decoding, the verification of a block of drafted tokens (include/omnibiote_hip_spec.h): a table of its own as well
SPEC_VERIFY_MAX_K = 31   # the most drafted tokens per row obte_spec_verify_bf16 takes
SYMBOLS_SPEC = {
    "obte_spec_verify_ws_bytes": (C.c_int64, [C.c_int64, C.c_int64]),
    "obte_spec_verify_bf16": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p,
                                        C.c_float, C.c_int32, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, c_stream]),
}

# the key/value cache stored as OCP e4m3 (include/omnibiote_hip_kv8.h): a table of its own as well
SYMBOLS_KV8 = {
    "obte_kv8_cache_bytes": (C.c_int64, [C.c_int64, C.c_int64, C.c_int32, C.c_int32]),
    "obte_kv8_cache_store": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_int32, C.c_int32, C.c_void_p, C.c_int64, C.c_int64, c_stream]),
    "obte_kv8_cache_rope_store_rows": (C.c_int, [C.c_void_p] * 4 + [C.c_int64, C.c_int64, C.c_int32, C.c_int32, C.c_void_p, C.c_int64, c_stream]),
    "obte_attn_decode_kv8": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_void_p, C.c_int32,
                                       C.c_int32, C.c_float, C.c_int32, C.c_void_p, C.c_int64, c_stream]),
    "obte_block_fwd_prefill_kv8": (C.c_int, [C.POINTER(BlockDesc), C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, c_stream]),
    "obte_block_decode_kv8": (C.c_int, [C.POINTER(BlockDesc), C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64,
                                        c_stream]),
}

# a prefix cache shared by groups of rows, many samples per prompt (include/omnibiote_hip_shared.h): a table of its own as well
ATTN_SHARED_MAX_SPLITS = 32   # OBTE_ATTN_SHARED_MAX_SPLITS
SYMBOLS_SHARED = {
    "obte_attn_shared_prefix_splits": (C.c_int, [C.c_int64, C.c_int64, C.c_int32, C.c_int32, C.c_int64]),
    "obte_attn_decode_shared_ws_bytes": (C.c_int64, [C.c_int64, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_int32]),
    "obte_attn_decode_shared": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_void_p, C.c_int64, C.c_int64, C.c_int64,
                                          C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_float, C.c_int32, C.c_int32, C.c_void_p, C.c_int64, c_stream]),
    "obte_block_decode_shared_ws_bytes": (C.c_int64, [C.c_int64, C.c_int64, C.c_int32, C.c_int32]),
    "obte_block_decode_shared": (C.c_int, [C.POINTER(BlockDesc), C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_void_p, C.c_int64,
                                           C.c_int64, C.c_void_p, C.c_int64, c_stream]),
}

# the generation loop's state on the device (include/omnibiote_hip_loop.h): a table of its own as well
SYMBOLS_LOOP = {
    "obte_gen_advance": (C.c_int, [C.c_void_p] * 4 + [C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p, C.c_int64,
                                   C.c_void_p, C.c_int64, C.c_int32, C.c_int64, c_stream]),
}

# the sampler and the draft verification over a restricted vocabulary (include/omnibiote_hip_constrain.h): a table of its own as well
SYMBOLS_CONSTRAIN = {
    "obte_sample_logits_constrained_bf16": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_void_p, C.c_float, C.c_int32, C.c_float,
                                                      C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, c_stream]),
    "obte_spec_verify_constrained_bf16": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_void_p,
                                                    C.c_void_p, C.c_float, C.c_int32, C.c_float, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_int32,
                                                    C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, c_stream]),
}

# the decode step's weights stored as OCP e4m3 (include/omnibiote_hip_w8.h): a table of its own as well
SYMBOLS_W8 = {
    "obte_linear_small_m_w8": (C.c_int, [C.POINTER(GemmArgs), C.c_void_p, C.c_int64, C.c_void_p, c_stream]),
    "obte_block_step_w8": (C.c_int, [C.POINTER(BlockDesc), C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32,
                                     C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, c_stream]),
}

# the decode step's weights stored as OCP MXFP4 (include/omnibiote_hip_w4.h): a table of its own as well
SYMBOLS_W4 = {
    "obte_linear_small_m_w4": (C.c_int, [C.POINTER(GemmArgs), C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, c_stream]),
    "obte_block_step_w4": (C.c_int, [C.POINTER(BlockDesc), C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32,
                                     C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, c_stream]),
}

# sequence scoring, the readout fused with its log-softmax (include/omnibiote_hip_score.h): a table of its own as well
READOUT_SCORE_MAX_SLICES, READOUT_SCORE_MAX_K = 64, 64
SYMBOLS_SCORE = {
    "obte_readout_score_slices": (C.c_int32, [C.c_int64, C.c_int64]),
    "obte_readout_score_ws_bytes": (C.c_int64, [C.c_int64, C.c_int64, C.c_int32]),
    "obte_readout_score_bf16": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_int64, C.c_float, C.c_void_p, C.c_int64,
                                          C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int64, c_stream]),
}

# encoder infilling, the draw fused into the readout and the unmasking loop's bookkeeping (include/omnibiote_hip_fill.h): a table of its
# own as well
SITE_FILL = 8                                      # OBTE_SITE_FILL: the noise rule's site constant
FILL_CONFIDENCE, FILL_RANDOM, FILL_LEFT = 0, 1, 2  # OBTE_FILL_*
FILL_MAX_SEG = 8192                                # the most entries per sequence obte_fill_commit takes
SYMBOLS_FILL = {
    "obte_readout_sample_slices": (C.c_int32, [C.c_int64, C.c_int64]),
    "obte_readout_sample_ws_bytes": (C.c_int64, [C.c_int64, C.c_int64, C.c_int32]),
    "obte_readout_sample_bf16": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_int64, C.c_float, C.c_float, C.c_uint64,
                                           C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int64, c_stream]),
    "obte_fill_commit": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_uint64,
                                   C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, c_stream]),
}

# the sampler with repetition, presence and frequency penalties (include/omnibiote_hip_penalty.h): a table of its own as well
PENALTY_MAX_GEN, PENALTY_MAX_PROMPT = 32767, 2 ** 24 - 1   # the largest gen_max and prompt_max the call takes
SYMBOLS_PENALTY = {
    "obte_sample_logits_penalized_bf16": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_void_p, C.c_float, C.c_int32, C.c_float,
                                                    C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_int32,
                                                    C.c_void_p, C.c_int64, C.c_void_p, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int32,
                                                    C.c_float, C.c_float, C.c_float, C.c_float, C.c_void_p, C.c_void_p, c_stream]),
}

# the distillation loss of a causal-LM training step (include/omnibiote_hip_distill.h): a table of its own as well
DISTILL_MAX_VOCAB = 131072                                 # the widest row obte_distill_ce_rows takes
SYMBOLS_DISTILL = {
    "obte_distill_ce_rows": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_void_p, C.c_float, C.c_float, C.c_float,
                                       C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, c_stream]),
}

# beam search, the selection and the attention / block step through an ancestry table (include/omnibiote_hip_beam.h): a table of its own
# as well
BEAM_MAX_WIDTH = 32                                        # OBTE_BEAM_MAX_WIDTH
SYMBOLS_BEAM = {
    "obte_beam_select_ws_bytes": (C.c_int64, [C.c_int64, C.c_int64]),
    "obte_beam_select_bf16": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64,
                                        C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                        C.c_int64, c_stream]),
    "obte_attn_decode_beam": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_void_p, C.c_int64, C.c_int64, C.c_int64,
                                        C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_float, C.c_int32, C.c_int32, C.c_void_p, C.c_int64, c_stream]),
    "obte_block_decode_beam_ws_bytes": (C.c_int64, [C.c_int64, C.c_int64, C.c_int32, C.c_int32]),
    "obte_block_decode_beam": (C.c_int, [C.POINTER(BlockDesc), C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_void_p, C.c_int64,
                                         C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, c_stream]),
}

# the key/value cache in pages of 64 positions, one pool for rows of any lengths (include/omnibiote_hip_paged.h): a table of its own as well
KV_PAGE = 64                                               # OBTE_KV_PAGE
SYMBOLS_PAGED = {
    "obte_kv_paged_bytes": (C.c_int64, [C.c_int64, C.c_int32, C.c_int32]),
    "obte_kv_paged_store": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_int32, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, c_stream]),
    "obte_kv_paged_rope_store_rows": (C.c_int, [C.c_void_p] * 4 + [C.c_int64, C.c_int64, C.c_int32, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, c_stream]),
    "obte_attn_decode_paged": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p,
                                         C.c_int64, C.c_int32, C.c_int32, C.c_float, C.c_int32, C.c_void_p, C.c_int64, c_stream]),
    "obte_block_fwd_prefill_paged": (C.c_int, [C.POINTER(BlockDesc), C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64,
                                               c_stream]),
    "obte_block_decode_paged": (C.c_int, [C.POINTER(BlockDesc), C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64,
                                          C.c_void_p, C.c_int64, c_stream]),
}

# the pages as OCP e4m3 codes with one scale per head vector (include/omnibiote_hip_paged8.h): SYMBOLS_PAGED's argument lists over the e4m3 pool
SYMBOLS_PAGED8 = {
    "obte_kv8_paged_bytes": (C.c_int64, [C.c_int64, C.c_int32, C.c_int32]),
    "obte_kv8_paged_store": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_int32, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, c_stream]),
    "obte_kv8_paged_rope_store_rows": (C.c_int, [C.c_void_p] * 4 + [C.c_int64, C.c_int64, C.c_int32, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, c_stream]),
    "obte_attn_decode_paged8": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p,
                                          C.c_int64, C.c_int32, C.c_int32, C.c_float, C.c_int32, C.c_void_p, C.c_int64, c_stream]),
    "obte_block_fwd_prefill_paged8": (C.c_int, [C.POINTER(BlockDesc), C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64,
                                                c_stream]),
    "obte_block_decode_paged8": (C.c_int, [C.POINTER(BlockDesc), C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64,
                                           C.c_void_p, C.c_int64, c_stream]),
}

# several new positions per row against the pages of a bf16 pool (include/omnibiote_hip_paged_extend.h): SYMBOLS_EXTEND's argument lists with
# (pool, n_pages, table, table_ld) in the place of (cache, T_max)
SYMBOLS_PAGED_EXTEND = {
    "obte_attn_extend_paged": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int64,
                                         C.c_void_p, C.c_int32, C.c_int32, C.c_float, C.c_int32, C.c_void_p, C.c_int64, c_stream]),
    "obte_kv_paged_rope_store_chunk": (C.c_int, [C.c_void_p] * 4 + [C.c_int64, C.c_int64, C.c_int64, C.c_int32, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64,
                                                                    c_stream]),
    "obte_block_extend_paged": (C.c_int, [C.POINTER(BlockDesc), C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p,
                                          C.c_int64, c_stream]),
}

# attention maps, the softmax weights of one layer as a tensor (include/omnibiote_hip_probs.h): a table of its own as well, and the one
# aggregate type obte_struct_sizes does not list (lib() checks its size against obte_attn_probs_args_bytes)
class AttnProbsArgs(C.Structure):
    _fields_ = [("qkv", C.c_void_p), ("key_ranges", C.c_void_p), ("mask", C.c_void_p),
                ("mask_sb", C.c_int64), ("mask_sh", C.c_int64), ("mask_sq", C.c_int64), ("ranges_exact", C.c_void_p),
                ("B", C.c_int64), ("T", C.c_int64), ("n_head", C.c_int32), ("head_dim", C.c_int32), ("scale", C.c_float),
                ("out", C.c_void_p), ("out_sb", C.c_int64), ("out_bf16", C.c_int32), ("head_mean", C.c_int32),
                ("ws", C.c_void_p), ("ws_bytes", C.c_int64)]


SYMBOLS_PROBS = {
    "obte_attn_probs_args_bytes": (C.c_int64, []),
    "obte_attn_probs_ws_bytes": (C.c_int64, [C.c_int64, C.c_int64, C.c_int32]),
    "obte_attn_probs": (C.c_int, [C.POINTER(AttnProbsArgs), c_stream]),
}

# speculative decoding without a draft model, the n-gram lookup draft and the verification of a drafted token (include/omnibiote_hip_lookup.h):
# a table of its own as well
LOOKUP_MAX_HISTORY, LOOKUP_MAX_NGRAM = 8192, 16           # OBTE_LOOKUP_MAX_HISTORY, OBTE_LOOKUP_MAX_NGRAM
SYMBOLS_LOOKUP = {
    "obte_lookup_draft": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_int64, C.c_void_p, C.c_void_p,
                                    c_stream]),
    "obte_spec_verify_point_ws_bytes": (C.c_int64, [C.c_int64, C.c_int64]),
    "obte_spec_verify_point_bf16": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_float, C.c_int32,
                                              C.c_float, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, c_stream]),
}

_lib = None
_lock = threading.Lock()


class HipLibraryError(RuntimeError):
    pass


def lib():
    """The loaded library.  Raises HipLibraryError if it is missing: build it with
    ``python -c 'import __graft_entry__ as g; g.build()'`` (or ``make -C omnibiote_amd/csrc``)."""
    global _lib
    if _lib is not None:
        return _lib
    with _lock:
        if _lib is None:
            # PyTorch-ROCm ships its own libamdhip64; load it first so that this library binds to the SAME HIP
            # runtime instance that owns torch's streams and allocations (two runtimes in one process do not
            # share devices, streams or pointers).
            import torch  # noqa: F401
            if not os.path.exists(LIB_PATH):
                raise HipLibraryError(f"{LIB_PATH} not found: the HIP library has not been built "
                                      "(make -C omnibiote_amd/csrc). There is no CPU fallback.")
            try:
                l = C.CDLL(LIB_PATH)
            except OSError as e:
                raise HipLibraryError(f"cannot load {LIB_PATH}: {e}") from e
            for name, (res, args) in (list(SYMBOLS.items()) + list(SYMBOLS_ROWS.items()) + list(SYMBOLS_SMALL_M.items()) + list(SYMBOLS_SAMPLE.items())
                                            + list(SYMBOLS_EXTEND.items()) + list(SYMBOLS_SPEC.items()) + list(SYMBOLS_KV8.items())
                                            + list(SYMBOLS_SHARED.items()) + list(SYMBOLS_LOOP.items()) + list(SYMBOLS_CONSTRAIN.items())
                                            + list(SYMBOLS_W8.items()) + list(SYMBOLS_SCORE.items()) + list(SYMBOLS_FILL.items()) + list(SYMBOLS_PENALTY.items())
                                            + list(SYMBOLS_DISTILL.items()) + list(SYMBOLS_BEAM.items()) + list(SYMBOLS_PAGED.items())
                                            + list(SYMBOLS_PAGED8.items()) + list(SYMBOLS_W4.items()) + list(SYMBOLS_PAGED_EXTEND.items())
                                            + list(SYMBOLS_PROBS.items()) + list(SYMBOLS_LOOKUP.items())):
                try:
                    fn = getattr(l, name)
                except AttributeError as e:
                    raise HipLibraryError(f"{LIB_PATH} does not export {name}") from e
                fn.restype = res
                fn.argtypes = args
            sizes = (C.c_int64 * 8)()
            n = l.obte_struct_sizes(sizes, 8)
            mine = [C.sizeof(GemmArgs), C.sizeof(AttnFwdArgs), C.sizeof(AttnBwdArgs), C.sizeof(MtArgs), C.sizeof(BlockDesc), C.sizeof(MtMasterArgs)]
            if n != len(mine) or list(sizes[:n]) != mine:
                raise HipLibraryError(f"struct layout mismatch between _lib.py {mine} and {LIB_PATH} {list(sizes[:n])}")
            if l.obte_attn_probs_args_bytes() != C.sizeof(AttnProbsArgs):
                raise HipLibraryError(f"struct layout mismatch between _lib.py AttnProbsArgs ({C.sizeof(AttnProbsArgs)}) and {LIB_PATH} "
                                      f"({l.obte_attn_probs_args_bytes()})")
            _lib = l
    return _lib


def check(rc: int, what: str = "") -> None:
    if rc != 0:
        msg = lib().obte_last_error()
        raise RuntimeError(f"{what or 'libomnibiote_hip'} failed (code {rc}): {msg.decode() if msg else ''}")


STATUS_ATTN_BWD_HANDOFF = 1


class DeviceStatusError(RuntimeError):
    """A kernel reported, through the library's device status word, that a launch's results are invalid."""


def check_device_status(what: str = "") -> None:
    """Raise if any kernel has reported a failure since the last check (include/omnibiote_hip.h, obte_device_status).  A plain host
    read of pinned memory: meaningful for work the caller has already synchronised with — call it right after a `.item()`, a
    stream / device synchronise or an event wait.  The bits are cleared, so one failure is raised once."""
    v = lib().obte_device_status(1)
    if v != 0:
        msg = lib().obte_last_error()
        raise DeviceStatusError(f"{what + ': ' if what else ''}{msg.decode() if msg else f'device status {v}'}")
