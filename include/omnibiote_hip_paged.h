/* libomnibiote_hip.so — generation on a PAGED key/value cache (the companion of omnibiote_hip.h, which it includes through
 * omnibiote_hip_rows.h: the same ABI version, the same conventions — caller-owned buffers, the caller's stream, no allocation, no
 * synchronisation — and no new struct). */
#ifndef OMNIBIOTE_HIP_PAGED_H
#define OMNIBIOTE_HIP_PAGED_H
#include "omnibiote_hip_rows.h"
#ifdef __cplusplus
extern "C" {
#endif

/* ---- a key/value cache in pages: rows of any lengths share one pool ---------------------------------------------------
 * The caches of omnibiote_hip.h are rectangles, B rows of T_max positions.  Here one layer's keys and values live in a POOL of pages of
 * OBTE_KV_PAGE = 64 positions, and a TABLE says which page holds which 64 positions of which row, so memory follows what the rows hold
 * and a finished row's pages go to the next one.  64 is the unit every split boundary of obte_attn_decode falls on, and one (head size
 * 128) or half a (head size 64) round of its workgroup: the page of every key a workgroup loads in a round is known from the block
 * index and the loop counter alone, and the table is read once per round and page with a workgroup-uniform index.
 *
 * The pool of one layer: obte_kv_paged_bytes(n_pages, n_head, head_dim) bytes, 16-byte aligned — K bf16 [n_pages, H, 64, hs], V behind it
 * in the same shape.  Every head of a page belongs to the same row and the same 64 positions; the 64 x hs block of one (page, head) is
 * contiguous.  0 for an unsupported shape (head_dim 64 or 128, n_pages < 2^24).
 *
 * The table: int32 [rows, table_ld] on the device, entry j of row b the page that holds positions [64 j, 64 j + 64) of that row.  An
 * entry outside [0, n_pages) means NO PAGE: nothing is stored to it, and its keys are not there — exactly as keys at or beyond a row's
 * count are not there; their loads are sent to page 0 and their weight is an exact 0.  A wrong table is therefore memory-safe without a
 * status word, as an out-of-range position is (omnibiote_hip_rows.h).  `rows` is whatever the call's B is: the pointer may address any
 * subset of consecutive rows of a larger table, or a gathered copy of some of its rows — which is how a few newly admitted prompts are
 * prefilled into a pool other rows are using.  Two rows must not name one page (nothing checks it).  bf16 only. */
#define OBTE_KV_PAGE 64
int64_t obte_kv_paged_bytes(int64_t n_pages, int32_t n_head, int32_t head_dim);

/* The prefill's store: the k and v thirds of the packed, rotated qkv [B * t, 3C] go to positions [0, t) of each row, through the table
 * (obte_kv_cache_store at pos0 = 0).  A position without a page is skipped — so right padding beyond a row's own pages disappears.
 * t <= 64 * table_ld. */
int obte_kv_paged_store(const obte_bf16* qkv, int64_t B, int64_t t, int32_t n_head, int32_t head_dim, obte_bf16* pool, int64_t n_pages,
                        const int32_t* table, int64_t table_ld, obte_stream s);
/* One decode step's rotate-and-store at pos[b]: obte_kv_cache_rope_store_rows's arithmetic, the same bits in qkv and in the stored
 * vectors; an active row (0 <= pos[b] <= max_pos, max_pos < 64 * table_ld) whose position has no page is rotated and not stored. */
int obte_kv_paged_rope_store_rows(obte_bf16* qkv, const float* rope_cos, const float* rope_sin, const int32_t* pos, int64_t max_pos, int64_t B,
                                  int32_t n_head, int32_t head_dim, obte_bf16* pool, int64_t n_pages, const int32_t* table, int64_t table_ld,
                                  obte_stream s);
/* obte_attn_decode_rows over pages: row b attends over its positions [0, n_keys[b]) that have a page; active iff 1 <= n_keys[b] <=
 * max_keys (host, 1 <= max_keys <= 64 * table_ld).  The workspace (obte_attn_decode_ws_bytes), the split rule per row, the combine
 * launch and `splits` are obte_attn_decode_rows's, and row b of o and lse is, bit for bit, what that call gives at the same split count
 * on a rectangular cache holding the same vectors at the same positions: only addresses change, the order of every sum is that
 * kernel's.  A row all of whose pages are missing gives exact zeros and lse = -inf.  The launch profiler records kind 102. */
int obte_attn_decode_paged(const obte_bf16* q, int64_t q_ld, const obte_bf16* pool, int64_t n_pages, const int32_t* table, int64_t table_ld,
                           obte_bf16* o, float* lse, int64_t B, const int32_t* n_keys, int64_t max_keys, int32_t n_head, int32_t head_dim, float scale,
                           int32_t splits, void* ws, int64_t ws_bytes, obte_stream s);
/* obte_block_fwd_prefill into pages: the same sequence and workspace (obte_block_infer_ws_bytes), y bit for bit its y; the rotated keys
 * and the values of positions [0, d->T) of row b go to the pages of table row b (d->T <= 64 * table_ld). */
int obte_block_fwd_prefill_paged(const obte_block_desc* d, const obte_bf16* x, obte_bf16* y, void* ws, int64_t ws_bytes, obte_bf16* pool, int64_t n_pages,
                                 const int32_t* table, int64_t table_ld, obte_stream s);
/* obte_block_decode_rows on pages: the same sequence and workspace (obte_block_decode_ws_bytes) with the two launchers above in place
 * of its store and attention; y bit for bit its y on a rectangular cache holding the same vectors.  max_pos < 64 * table_ld. */
int obte_block_decode_paged(const obte_block_desc* d, const obte_bf16* x, obte_bf16* y, obte_bf16* pool, int64_t n_pages, const int32_t* table,
                            int64_t table_ld, const int32_t* pos, int64_t max_pos, void* ws, int64_t ws_bytes, obte_stream s);

#ifdef __cplusplus
}
#endif
#endif
