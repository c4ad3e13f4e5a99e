/* libomnibiote_hip.so — generation with one cache position per row (the companion of omnibiote_hip.h, which it includes: the same
 * ABI version, the same conventions — caller-owned buffers, the caller's stream, no allocation, no synchronisation — and no new struct). */
#ifndef OMNIBIOTE_HIP_ROWS_H
#define OMNIBIOTE_HIP_ROWS_H
#include "omnibiote_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

/* ---- generation from prompts of different lengths: one cache position per row ---------------------------------------
 * The generation entry points of omnibiote_hip.h put every row of the batch at ONE position, a host integer.  These take the
 * positions as a device array, int32 [B], read by the kernels themselves (no host synchronisation), plus a host upper bound.
 * The row convention, the same in all three: row b is ACTIVE iff its value lies inside the bound stated below; any other value makes it INACTIVE — nothing of that row is
 * stored, no byte of its cache is read, its attention output row is exact zeros and its lse -inf.  An out-of-range device value is
 * therefore memory-safe without a status word, and a negative value is how a caller parks a finished row.  A prompt needs no rows
 * form: under the causal mask a right-padded prompt's real positions never see the padding, and the cache positions the padding
 * fills are overwritten by the row's own generated tokens before any query of that row reaches them.
 *
 * obte_kv_cache_rope_store_rows: one decode step's rotate-and-store.  qkv is the packed [B, 3C] activation BEFORE RoPE (c_attn with
 * OBTE_EPI_NONE), changed in place: the q and k thirds of an active row b (0 <= pos[b] <= max_pos, 0 <= max_pos < T_max) are rotated by
 * row pos[b] of the FULL tables rope_cos / rope_sin (fp32 [>= max_pos + 1, hs / 2]) in the arithmetic of OBTE_EPI_ROPE_QK — fp32 on the
 * bf16 values, the same expression, the same bits — and the rotated k and the v are written to cache position pos[b] of every head.
 * No other cache byte is touched.  One launch, 16 bytes per lane: it stands where obte_kv_cache_store stands in a uniform step. */
int obte_kv_cache_rope_store_rows(obte_bf16* qkv, const float* rope_cos, const float* rope_sin, const int32_t* pos, int64_t max_pos, int64_t B,
                                  int32_t n_head, int32_t head_dim, obte_bf16* cache, int64_t T_max, obte_stream s);
/* obte_attn_decode with one key count per row: row b attends over cache positions [0, n_keys[b]), n_keys a device int32 [B]; active iff
 * 1 <= n_keys[b] <= max_keys (host, 1 <= max_keys <= T_max).  The split count is one per launch (it is the grid): splits = 0 means
 * obte_attn_decode_splits(B, n_head, head_dim, max_keys), a forced count works as there.  Every workgroup derives its own key range
 * from its row's count by obte_attn_decode's rule applied per row — ceil(ceil(n_keys[b] / splits) / 64) * 64 keys per split — so row b
 * of o and lse is, bit for bit, what obte_attn_decode gives for n_keys = n_keys[b] at the same split count, and a short row's splits
 * share its keys.  Everything else is obte_attn_decode's: the workspace, the tail rule, the combine launch, no atomics or flags.
 * The launch profiler records kind 102 with max_keys. */
int obte_attn_decode_rows(const obte_bf16* q, int64_t q_ld, const obte_bf16* cache, obte_bf16* o, float* lse, int64_t B, int64_t T_max,
                          const int32_t* n_keys, int64_t max_keys, int32_t n_head, int32_t head_dim, float scale, int32_t splits, void* ws,
                          int64_t ws_bytes, obte_stream s);
/* obte_block_decode with row b at position pos[b] (device int32 [B]; active iff 0 <= pos[b] <= max_pos, 0 <= max_pos < T_max): LayerNorm,
 * c_attn with OBTE_EPI_NONE, obte_kv_cache_rope_store_rows, obte_attn_decode_rows over pos[b] + 1 keys (formed in the kernel: as many
 * launches as a uniform step), then obte_block_decode's tail.  The descriptor rules and the workspace (obte_block_decode_ws_bytes) are
 * obte_block_decode's; d->rope_cos / rope_sin are the FULL tables, at least max_pos + 1 rows.  y may alias x.  An inactive row's y is
 * the block applied to a zero attention output: finite, and of no use to the caller. */
int obte_block_decode_rows(const obte_block_desc* d, const obte_bf16* x, obte_bf16* y, obte_bf16* kv_cache, int64_t T_max, const int32_t* pos,
                           int64_t max_pos, void* ws, int64_t ws_bytes, obte_stream s);

#ifdef __cplusplus
}
#endif
#endif
