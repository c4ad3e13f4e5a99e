/* libomnibiote_hip.so — continuing a filled key/value cache by several positions per row in one call (the companion of
 * omnibiote_hip.h, which it includes: the same ABI version, the same conventions — caller-owned buffers, the caller's stream, no
 * allocation, no synchronisation, every argument checked on the host before any launch — and no new struct). */
#ifndef OMNIBIOTE_HIP_EXTEND_H
#define OMNIBIOTE_HIP_EXTEND_H
#include "omnibiote_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

/* ---- n new positions per row against a cache that already holds p ---------------------------------------------------------
 * obte_block_fwd_prefill starts a cache at position 0 and obte_block_decode appends one position per row; these append n = n_new >= 1
 * positions: a second prompt segment, a block of drafted tokens to verify, a continuation to score, a long prompt in chunks.
 *
 * Row b's chunk starts at position p_b.  Uniform form (pos_rows == NULL): p_b = pos for every row, a host integer, 0 <= pos and
 * pos + n <= T_max.  Rows form: pos_rows is a device int32 [B], p_b = pos_rows[b], and pos is the host bound, pos + n <= T_max; row b is
 * ACTIVE iff 0 <= pos_rows[b] <= pos and any other value makes it INACTIVE exactly as omnibiote_hip_rows.h defines it — nothing of the row
 * is stored, no byte of its cache is read, its n output rows are exact zeros and its lse -inf.
 *
 * obte_attn_extend: softmax(q k^T * scale) v for n queries per (b, h).  The query of (b, j, h) is read at
 * q + (b*n + j)*q_ld + h*hs (q_ld = 3C reads the q third of a packed row in place) and attends over cache positions [0, p_b + j + 1):
 * the caller has stored the chunk's own keys and values first, and the chunk is causal inside itself.  o is bf16 [B*n, C], heads side by
 * side; lse (nullable) fp32 [B, H, n], defined as obte_attn_decode defines it.  head_dim in {64, 128}, B * n_head <= 65535, q, cache and
 * o 16-byte aligned.
 * Per (b, h) the queries are cut into tiles of 32 and the keys a tile can see, [0, p_b + min(n, 32 (tile + 1))), into `splits` runs of
 * ceil(ceil(keys / splits) / 32) * 32 keys, one workgroup each; a workgroup writes an fp32 partial to ws and a second launch combines
 * the partials in split order — no atomics, no flags, no hand-off between workgroups: two launches of the same call give the same
 * bytes, and a row of the rows form is, bit for bit, the uniform call at that row's position and the same split count.  With one split
 * the kernel writes o and lse itself, there is no second launch and ws may be NULL.  splits = 0: obte_attn_extend_splits(B, n_head,
 * head_dim, n_new, pos + n_new), a pure function; 1 .. OBTE_ATTN_EXTEND_MAX_SPLITS forces a count (a split without keys contributes
 * exactly nothing).  obte_attn_extend_ws_bytes: the bytes that count needs (16-byte aligned); splits = 0 there means the largest count
 * the default rule can return for this (B, n_head, head_dim, n_new); 0 for a shape the entry points reject.
 * Cache positions >= p_b + n never reach a result, whatever bit patterns they hold (NaN included); a later position of the same chunk is
 * masked by its score.  fp32 scores, fp32 online softmax in the exp2 domain, the normaliser summed from the fp32 probabilities,
 * probabilities rounded to bf16 for the P V product (v_mfma_f32_32x32x16_bf16 both times), fp32 accumulation, one rounding of o.
 * The launch profiler records kind 104 with (B * n_head, pos + n_new, head_dim).
 *
 * obte_kv_cache_rope_store_chunk: the rows form's rotate-and-store, obte_kv_cache_rope_store_rows generalised from row b to rows
 * b*n + j at position pos_rows[b] + j.  qkv is the packed [B*n, 3C] activation BEFORE RoPE, changed in place: the q and k thirds of an
 * active row's n rows are rotated by rows pos_rows[b] + j of the FULL tables (fp32 [>= max_pos + n, hs / 2]) in the arithmetic of
 * OBTE_EPI_ROPE_QK — the same bits as that epilogue followed by obte_kv_cache_store — and the rotated k and the v go to those cache
 * positions.  max_pos >= 0, max_pos + n <= T_max.  One launch, 16 bytes per lane, no other cache byte touched.
 *
 * obte_block_extend: the block on n new positions per row.  d->T = n; x and y are [B*n, C], y may alias x.  key_ranges, mask,
 * query_bounds, out_rows must be NULL and dropout_p 0, else OBTE_EUNSUPPORTED.  d->rope_cos / rope_sin are the FULL tables, at least
 * pos + n rows.  Uniform: LayerNorm, c_attn with OBTE_EPI_ROPE_QK at table rows pos .. pos + n - 1, obte_kv_cache_store(t = n,
 * pos0 = pos), obte_attn_extend, then obte_block_fwd_infer's tail.  Rows form (pos_rows != NULL): c_attn with OBTE_EPI_NONE,
 * obte_kv_cache_rope_store_chunk, obte_attn_extend with pos_rows.  With B*n <= obte_small_m_max() the four products run on
 * obte_linear_small_m_bf16, else through obte_gemm_bf16_ws.  ws: obte_block_extend_ws_bytes() bytes (0 for a shape the block rejects),
 * 256-byte aligned: obte_block_infer_ws_bytes(B, n, ...) plus the attention partials.  Neither workspace size is monotone in n_new (the
 * default split count drops where a query tile is added): a caller that keeps a buffer across calls asks for the size of each n. */
#define OBTE_ATTN_EXTEND_MAX_SPLITS 32
int obte_attn_extend_splits(int64_t B, int32_t n_head, int32_t head_dim, int64_t n_new, int64_t n_keys);
int64_t obte_attn_extend_ws_bytes(int64_t B, int32_t n_head, int32_t head_dim, int64_t n_new, int32_t splits);
int obte_kv_cache_rope_store_chunk(obte_bf16* qkv, const float* rope_cos, const float* rope_sin, const int32_t* pos_rows, int64_t max_pos, int64_t B,
                                   int64_t n_new, int32_t n_head, int32_t head_dim, obte_bf16* cache, int64_t T_max, obte_stream s);
int obte_attn_extend(const obte_bf16* q, int64_t q_ld, const obte_bf16* cache, obte_bf16* o, float* lse, int64_t B, int64_t T_max, int64_t n_new,
                     int64_t pos, const int32_t* pos_rows, int32_t n_head, int32_t head_dim, float scale, int32_t splits, void* ws, int64_t ws_bytes,
                     obte_stream s);
int64_t obte_block_extend_ws_bytes(int64_t B, int64_t n_new, int32_t n_embd, int32_t n_head);
int obte_block_extend(const obte_block_desc* d, const obte_bf16* x, obte_bf16* y, obte_bf16* kv_cache, int64_t T_max, int64_t pos,
                      const int32_t* pos_rows, void* ws, int64_t ws_bytes, obte_stream s);

#ifdef __cplusplus
}
#endif
#endif
