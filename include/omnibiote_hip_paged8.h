/* libomnibiote_hip.so — generation on a PAGED key/value cache stored as OCP e4m3 (the companion of omnibiote_hip_paged.h and
 * omnibiote_hip_kv8.h, which it includes: the same ABI version, the same conventions — caller-owned buffers, the caller's stream, no
 * allocation, no synchronisation, every argument checked on the host before any launch with obte_last_error naming the entry point —
 * and no new struct). */
#ifndef OMNIBIOTE_HIP_PAGED8_H
#define OMNIBIOTE_HIP_PAGED8_H
#include "omnibiote_hip_paged.h"
#include "omnibiote_hip_kv8.h"
#ifdef __cplusplus
extern "C" {
#endif

/* ---- the format ---------------------------------------------------------------------------------------------------------
 * One layer's pool of n_pages pages of OBTE_KV_PAGE = 64 positions, in this order, base 16-byte aligned:
 *   K codes  uint8 [n_pages, H, 64, hs]      V codes  the same shape      K scales  fp32 [n_pages, H, 64]      V scales  the same shape
 * 2 * n_pages * H * 64 * (hs + 4) bytes: per cached vector 2 (hs + 4) bytes against the bf16 pool's 4 hs (0.516 at hs = 128).  hs =
 * head_dim is 64 or 128, n_pages < 2^24.  The 64 x hs codes of one (page, head) are contiguous, and so are its 64 scales.
 *
 * A head vector is quantised exactly as omnibiote_hip_kv8.h defines it (code_i = RNE_e4m3(x_i * 2^-e), scale = 2^e, e the smallest
 * integer >= -126 with max|x_i| * 2^-e <= 448; omnibiote_amd/kvquant.py in plain torch): the pool holds the codes and scales the
 * rectangular e4m3 cache holds, at other addresses.
 *
 * The table and its rules are exactly those of omnibiote_hip_paged.h: int32 [rows, table_ld], entry j of row b the page of positions
 * [64 j, 64 j + 64) of that row; an entry outside [0, n_pages) means NO PAGE: nothing is stored there, the loads of its codes AND of
 * its scales are sent to page 0, and its weight is an exact 0 — selected, not multiplied, so whatever page 0 holds (codes 0x7F, NaN
 * or infinite scales: it may be a page nobody holds) reaches no result.
 * omnibiote_amd/paged.py states the layout in plain torch (paged8_gather_reference, paged8_scatter_reference).
 *
 * As on both parents, ONE query per (batch, head) attends over this cache and one position per row joins it per call: there is no
 * extend, chunked-prefill or draft-verification form. */
int64_t obte_kv8_paged_bytes(int64_t n_pages, int32_t n_head, int32_t head_dim);   /* 0 for a rejected shape */

/* The prefill's store through the table: obte_kv_paged_store's contract (positions [0, t) of each row, t <= 64 * table_ld, a position
 * without a page skipped) with obte_kv8_cache_store's quantiser.  No other byte of the pool is touched. */
int obte_kv8_paged_store(const obte_bf16* qkv, int64_t B, int64_t t, int32_t n_head, int32_t head_dim, void* pool8, int64_t n_pages, const int32_t* table,
                         int64_t table_ld, obte_stream s);
/* One decode step's rotate-and-store at pos[b]: qkv is left with the bits obte_kv_cache_rope_store_rows leaves, and the codes and
 * scales obte_kv8_cache_rope_store_rows writes go to slot pos[b] % 64 of page table[b][pos[b] / 64].  An active row (0 <= pos[b] <=
 * max_pos, max_pos < 64 * table_ld) whose position has no page is rotated and not stored. */
int obte_kv8_paged_rope_store_rows(obte_bf16* qkv, const float* rope_cos, const float* rope_sin, const int32_t* pos, int64_t max_pos, int64_t B,
                                   int32_t n_head, int32_t head_dim, void* pool8, int64_t n_pages, const int32_t* table, int64_t table_ld, obte_stream s);
/* obte_attn_decode_paged's arguments over the e4m3 pool.  Row b of o and lse is, bit for bit, what obte_attn_decode_kv8 gives with
 * n_keys_rows at the same split count on a rectangular e4m3 cache holding the same codes and scales at the same positions.  The
 * workspace (obte_attn_decode_ws_bytes), the split rule and the combine launch are the same.  A row all of whose pages are missing, or
 * whose count lies outside [1, max_keys], gives exact zeros and lse = -inf.  The launch profiler records kind 119 with
 * (B * n_head, max_keys, head_dim). */
int obte_attn_decode_paged8(const obte_bf16* q, int64_t q_ld, const void* pool8, int64_t n_pages, const int32_t* table, int64_t table_ld, obte_bf16* o,
                            float* lse, int64_t B, const int32_t* n_keys, int64_t max_keys, int32_t n_head, int32_t head_dim, float scale, int32_t splits,
                            void* ws, int64_t ws_bytes, obte_stream s);
/* obte_block_fwd_prefill_paged with the quantised store: y bit for bit obte_block_fwd_infer's, the workspace obte_block_infer_ws_bytes. */
int obte_block_fwd_prefill_paged8(const obte_block_desc* d, const obte_bf16* x, obte_bf16* y, void* ws, int64_t ws_bytes, void* pool8, int64_t n_pages,
                                  const int32_t* table, int64_t table_ld, obte_stream s);
/* obte_block_decode_paged with the two launchers above: y bit for bit obte_block_decode_kv8's rows form on a rectangular e4m3 cache
 * holding the same vectors.  The workspace is obte_block_decode_ws_bytes; max_pos < 64 * table_ld. */
int obte_block_decode_paged8(const obte_block_desc* d, const obte_bf16* x, obte_bf16* y, void* pool8, int64_t n_pages, const int32_t* table, int64_t table_ld,
                             const int32_t* pos, int64_t max_pos, void* ws, int64_t ws_bytes, obte_stream s);

#ifdef __cplusplus
}
#endif
#endif
