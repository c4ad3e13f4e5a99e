/* libomnibiote_hip.so — several new positions per row against a PAGED key/value cache (the companion of omnibiote_hip_paged.h and
 * omnibiote_hip_extend.h, which it includes: the same ABI version, the same conventions — caller-owned buffers, the caller's stream, no
 * allocation, no synchronisation, every argument checked on the host before any launch — and no new struct). */
#ifndef OMNIBIOTE_HIP_PAGED_EXTEND_H
#define OMNIBIOTE_HIP_PAGED_EXTEND_H
#include "omnibiote_hip_paged.h"
#include "omnibiote_hip_extend.h"
#ifdef __cplusplus
extern "C" {
#endif

/* ---- n new positions per row whose earlier keys live in pages ------------------------------------------------------------
 * What a request needs that REUSES pages another request has filled: its table row names those pages for its first 64 m positions (a
 * table entry may name any page; two rows may name one page as long as neither stores to it), and only its remaining prompt tokens are
 * computed — n at a time, from position pos_rows[b] on, against the keys the pages hold.  The pool and the table are those of
 * omnibiote_hip_paged.h (bf16 only; the e4m3 pool has no such form), the rows form and its inactive rows those of omnibiote_hip_extend.h.
 *
 * obte_attn_extend_paged: the rows form of obte_attn_extend over a pool.  pos_rows is required; pos is its host bound and
 * pos + n_new <= 64 * table_ld.  The partition of a row's keys, the split rule (obte_attn_extend_splits), the workspace
 * (obte_attn_extend_ws_bytes) and the combine launch are obte_attn_extend's, and row b of o and lse is, bit for bit, what the rows form
 * gives at the same split count on a rectangular cache holding the same vectors at the same positions: split boundaries and wave tiles
 * are multiples of 32 keys, so every 32-key tile lies in one page and only addresses change.  The K vector of (page, head h, key) stands at
 * pool + ((page * H + h) * 64 + key % 64) * hs, its V n_pages * H * 64 * hs elements behind.  A table entry outside [0, n_pages) means that
 * those 64 keys are not there: their loads go to page 0, their V is a selected zero and their score a selected -inf (obte_attn_decode_paged's
 * convention), so a wrong table is memory-safe; a tile, split or row without any key that is there carries (m = -inf, l = 0, O = 0) and a
 * row without any ends as exact zeros with lse = -inf.  The launch profiler records kind 120 with (B * n_head, pos + n_new, head_dim).
 *
 * obte_kv_paged_rope_store_chunk: obte_kv_cache_rope_store_chunk through the table — the same rotation of qkv [B*n_new, 3C] in place, the
 * same bits stored, position pos_rows[b] + j of row b to slot (pos_rows[b] + j) % 64 of page table[b][(pos_rows[b] + j) / 64].
 * max_pos >= 0, max_pos + n_new <= 64 * table_ld.  A position without a page is rotated and not stored; a row outside [0, max_pos] is
 * left alone.  One launch.
 *
 * obte_block_extend_paged: obte_block_extend's rows form on pages.  d->T = n; the same sequence and workspace
 * (obte_block_extend_ws_bytes) with the two launchers above in place of its store and attention; y bit for bit its y on a rectangular
 * cache holding the same vectors.  pos + d->T <= 64 * table_ld; d->rope_cos / rope_sin are the FULL tables, at least pos + n rows. */
int obte_attn_extend_paged(const obte_bf16* q, int64_t q_ld, const obte_bf16* pool, int64_t n_pages, const int32_t* table, int64_t table_ld, obte_bf16* o,
                           float* lse, int64_t B, int64_t n_new, int64_t pos, const int32_t* pos_rows, int32_t n_head, int32_t head_dim, float scale,
                           int32_t splits, void* ws, int64_t ws_bytes, obte_stream s);
int obte_kv_paged_rope_store_chunk(obte_bf16* qkv, const float* rope_cos, const float* rope_sin, const int32_t* pos_rows, int64_t max_pos, int64_t B,
                                   int64_t n_new, int32_t n_head, int32_t head_dim, obte_bf16* pool, int64_t n_pages, const int32_t* table, int64_t table_ld,
                                   obte_stream s);
int obte_block_extend_paged(const obte_block_desc* d, const obte_bf16* x, obte_bf16* y, obte_bf16* pool, int64_t n_pages, const int32_t* table,
                            int64_t table_ld, int64_t pos, const int32_t* pos_rows, void* ws, int64_t ws_bytes, obte_stream s);

#ifdef __cplusplus
}
#endif
#endif
