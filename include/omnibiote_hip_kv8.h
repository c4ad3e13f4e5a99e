/* libomnibiote_hip.so — generation on a key/value cache stored as OCP e4m3 (the companion of omnibiote_hip.h, which it includes: the same
 * ABI version, the same conventions — caller-owned buffers, the caller's stream, no allocation, no synchronisation, no atomics or flags,
 * every argument checked on the host before any launch with obte_last_error naming the entry point — and no new struct). */
#ifndef OMNIBIOTE_HIP_KV8_H
#define OMNIBIOTE_HIP_KV8_H
#include "omnibiote_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

/* ---- the format ---------------------------------------------------------------------------------------------------------
 * One layer's cache, in this order, base 16-byte aligned:
 *   K codes  uint8 [B, H, T_max, hs]      V codes  the same shape      K scales  fp32 [B, H, T_max]      V scales  the same shape
 * 2 (hs + 4) bytes per (b, h, position) against the bf16 cache's 4 hs; hs = head_dim is 64 or 128.  A head vector x of hs bf16
 * values is stored as  code_i = RNE_e4m3(x_i * 2^-e),  scale = 2^e  (an fp32),  e the smallest integer >= -126 with
 * max|x_i| * 2^-e <= 448.  The encoding is OCP e4m3fn (no infinities, 0x7F / 0xFF are NaN, largest finite 448).  The scale is a power
 * of two: the product is exact, the conversion is the only rounding, no code is a NaN, nothing saturates, and the cache's bytes are a
 * pure function of the bf16 inputs (omnibiote_amd/kvquant.py states the rule in plain torch).  Inputs are finite by contract: a
 * non-finite element leaves that vector's codes and scale unspecified and touches no other byte.  A reader forms float(code) * scale.
 *
 * Only ONE query per (batch, head) attends over this cache.  There is no e4m3 form of obte_attn_extend, obte_kv_cache_rope_store_chunk
 * or obte_block_extend: several new positions per row in one call (chunked prefill, draft verification) need a bf16 cache. */

/* 2 * B * n_head * T_max * (head_dim + 4); 0 for a shape the entry points reject (obte_kv_cache_bytes' rule) */
int64_t obte_kv8_cache_bytes(int64_t B, int64_t T_max, int32_t n_head, int32_t head_dim);
/* obte_kv_cache_store's contract with the quantised store: the k and v thirds of the already rotated packed qkv [B * t, 3C] go to
 * positions pos0 .. pos0 + t - 1 of every head.  No other cache byte is touched.  qkv and cache8 16-byte aligned. */
int obte_kv8_cache_store(const obte_bf16* qkv, int64_t B, int64_t t, int32_t n_head, int32_t head_dim, void* cache8, int64_t T_max, int64_t pos0,
                         obte_stream s);
/* obte_kv_cache_rope_store_rows' contract (omnibiote_hip_rows.h) with the quantised store: the q and k thirds of an active row b
 * (0 <= pos[b] <= max_pos < T_max) of the unrotated packed qkv [B, 3C] are rotated in place in the arithmetic of OBTE_EPI_ROPE_QK — the
 * bits obte_kv_cache_rope_store_rows leaves in qkv — and the rotated k and the v are quantised into position pos[b].  A row whose
 * position lies outside [0, max_pos] is left alone entirely. */
int obte_kv8_cache_rope_store_rows(obte_bf16* qkv, const float* rope_cos, const float* rope_sin, const int32_t* pos, int64_t max_pos, int64_t B,
                                   int32_t n_head, int32_t head_dim, void* cache8, int64_t T_max, obte_stream s);
/* obte_attn_decode on the e4m3 cache.  n_keys_rows == NULL: every row over positions [0, n_keys), 1 <= n_keys <= T_max.  Otherwise
 * (obte_attn_decode_rows' form) row b attends over n_keys_rows[b] keys, a device int32 [B]; it is active iff 1 <= n_keys_rows[b] <=
 * n_keys (the host's bound), an inactive row's o is exact zeros and its lse -inf.  Split semantics, splits = 0, forced counts, the
 * workspace (obte_attn_decode_ws_bytes), the partials and the combine launch are obte_attn_decode's; a row of the rows form is, bit
 * for bit, the uniform call at that row's count and the same split count.  The key's scale multiplies its score, the value's scale
 * its probability in P V, all in fp32.  Whatever the cache holds at positions >= a row's count (codes 0x7F, NaN scales) reaches no
 * result.  The launch profiler records kind 105 with (B * n_head, n_keys, head_dim). */
int obte_attn_decode_kv8(const obte_bf16* q, int64_t q_ld, const void* cache8, obte_bf16* o, float* lse, int64_t B, int64_t T_max, int64_t n_keys,
                         const int32_t* n_keys_rows, int32_t n_head, int32_t head_dim, float scale, int32_t splits, void* ws, int64_t ws_bytes,
                         obte_stream s);
/* obte_block_fwd_prefill with the cache stored quantised at pos0 = 0: y is bit for bit obte_block_fwd_infer's (the prompt's own
 * attention reads the unquantised packed qkv).  The workspace is obte_block_infer_ws_bytes. */
int obte_block_fwd_prefill_kv8(const obte_block_desc* d, const obte_bf16* x, obte_bf16* y, void* ws, int64_t ws_bytes, void* cache8, int64_t T_max,
                               obte_stream s);
/* obte_block_decode (pos_rows == NULL: every row at position pos) and obte_block_decode_rows (pos_rows a device int32 [B], pos the
 * host's bound on it) with obte_kv8_cache_store / obte_kv8_cache_rope_store_rows and obte_attn_decode_kv8 in the places of their bf16
 * launchers: the same launch sequence, descriptor rules and workspace (obte_block_decode_ws_bytes). */
int obte_block_decode_kv8(const obte_block_desc* d, const obte_bf16* x, obte_bf16* y, void* cache8, int64_t T_max, int64_t pos, const int32_t* pos_rows,
                          void* ws, int64_t ws_bytes, obte_stream s);

#ifdef __cplusplus
}
#endif
#endif
