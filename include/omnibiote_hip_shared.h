/* libomnibiote_hip.so — many samples per prompt: one-query attention and the decode step of a block over a key/value cache whose
 * prefix is shared by a group of rows (the companion of omnibiote_hip.h, which it includes: the same ABI version, the same conventions
 * — caller-owned buffers, the caller's stream, no allocation, no synchronisation, no atomics or flags, every argument checked on the
 * host before any launch — and no new struct). */
#ifndef OMNIBIOTE_HIP_SHARED_H
#define OMNIBIOTE_HIP_SHARED_H
#include "omnibiote_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

/* ---- P prompts, G samples of each ---------------------------------------------------------------------------------------------
 * B = P*G rows, row b = p*G + g.  The PREFIX cache is an ordinary bf16 layer cache of P rows (obte_kv_cache_bytes(P, T_pre, ...):
 * K [P, H, T_pre, hs], then V), filled by obte_block_fwd_prefill on the P prompts; its positions [0, n_prefix) are the prompt, the same
 * for the G rows of a group, stored and read once per group instead of once per row.  The SUFFIX cache is an ordinary bf16 layer cache
 * of B rows (K [B, H, T_suf, hs], then V): slot i of row b holds the row's own position n_prefix + i.
 *
 * obte_attn_decode_shared: softmax(q [K_prefix(p)[0:n_prefix] ; K_suffix(b)[0:n_suffix]]^T * scale) [V_prefix ; V_suffix] for one query
 * per (b, h), read at q + b*q_ld + h*hs.  o is bf16 [B, C]; lse (nullable) fp32 [B, H], defined as obte_attn_decode defines it.
 * 1 <= n_prefix <= T_pre, 0 <= n_suffix <= T_suf (with n_suffix = 0 the suffix contributes exactly nothing, suffix_cache is not read
 * and may be NULL).  head_dim in {64, 128}, P * n_head <= 65535, B * n_head <= 65535, G < 2^20; q, both caches, o and ws 16-byte
 * aligned, lse 4-byte aligned, q_ld a multiple of 8 and at least n_head * head_dim.
 * Three launches (two when n_suffix = 0):
 *   - prefix: obte_attn_extend's kernel with the group read as the chunk — the G queries of (p, h) in tiles of 32, every tile against
 *     all n_prefix keys with no mask by position (v_mfma_f32_32x32x16_bf16 both times), the keys cut into prefix_splits runs of
 *     ceil(ceil(n_prefix / prefix_splits) / 32) * 32; each (p, h, tile, split) writes an fp32 partial.  A padding query (j >= G) reads the
 *     group's last row and is never combined.
 *   - suffix: obte_attn_decode's kernel on the B rows of the suffix cache over n_suffix keys, cut into suffix_splits runs as
 *     obte_attn_decode cuts them, every (b, h, split) writing a partial (at one split too).
 *   - combine: one workgroup per (b, h) takes the maximum over the row's prefix partials and then its suffix partials, makes it finite,
 *     and sums the prefix partials in split order, then the suffix partials in split order, each rescaled to that maximum; one rounding
 *     of o.  An empty split carries (m = -inf, l = 0, 0) and adds exactly nothing.
 * Partials in ws, both fp32:
 *   - prefix, at ws: [P*H][ceil(G / 32) tiles][prefix_splits][hs/2 + 2][64]: the tile's transposed output accumulators as the MFMA
 *     leaves them — register 16*(d / 32) + (d % 4) + 4*((d % 32) / 8) of lane (query % 32) + 32*((d / 4) % 2) holds dimension d — then the
 *     running maximum m and the normaliser l of the lane's query, in the exp2 domain (scores times scale * log2 e);
 *   - suffix, behind them: [B*H][suffix_splits][hs + 4]: acc[hs], m, l, two unused (obte_attn_decode's partial).
 * Two launches of the same call give the same bytes.  Row (p, g) depends on its own query, prompt p's prefix, its own suffix row and
 * the two split counts alone: the same bits at every G and every P.  Prefix positions >= n_prefix and suffix slots >= n_suffix never
 * reach a result, whatever bit patterns they hold (NaN included).
 * prefix_splits = 0: obte_attn_shared_prefix_splits(P, G, n_head, head_dim, n_prefix), a pure function (1 for a rejected shape);
 * 1 .. OBTE_ATTN_SHARED_MAX_SPLITS forces a count.  suffix_splits = 0: obte_attn_decode_splits(B, n_head, head_dim, n_suffix);
 * 1 .. OBTE_ATTN_DECODE_MAX_SPLITS forces one.  obte_attn_decode_shared_ws_bytes: the bytes both sets of partials need at these counts;
 * 0 there means the largest count the default rule can return for this shape; 0 bytes for a shape the entry point rejects.
 * The launch profiler records kind 106 for the prefix launch with (P * n_head * tiles, n_prefix, head_dim), kind 102 for the suffix
 * launch with (B * n_head, n_suffix, head_dim) and kind 107 for the combine with (B * n_head, prefix_splits + suffix_splits, head_dim).
 *
 * obte_block_decode_shared: obte_block_decode on such a pair of caches.  d->B = P*G, d->T = 1; x and y are [B, C], y may alias x; the
 * descriptor rules are obte_block_decode's (key_ranges, mask, query_bounds, out_rows NULL and dropout_p 0, else OBTE_EUNSUPPORTED).
 * Every row's new token stands at absolute position n_prefix + suf_pos, suffix slot suf_pos, 0 <= suf_pos < T_suf; d->rope_cos /
 * rope_sin are the FULL tables, at least n_prefix + suf_pos + 1 rows.  LayerNorm, c_attn with OBTE_EPI_ROPE_QK at table row
 * n_prefix + suf_pos, obte_kv_cache_store(qkv, B, 1, ..., suffix_cache, T_suf, suf_pos), obte_attn_decode_shared with
 * n_suffix = suf_pos + 1 and default splits, then obte_block_fwd_infer's tail.  With B <= obte_small_m_max() the four products run on
 * obte_linear_small_m_bf16, else through obte_gemm_bf16_ws.  ws: obte_block_decode_shared_ws_bytes() bytes (0 for a shape the block
 * rejects), 256-byte aligned: obte_block_infer_ws_bytes(B, 1, ...) plus the attention partials. */
#define OBTE_ATTN_SHARED_MAX_SPLITS 32
int obte_attn_shared_prefix_splits(int64_t P, int64_t G, int32_t n_head, int32_t head_dim, int64_t n_prefix);
int64_t obte_attn_decode_shared_ws_bytes(int64_t P, int64_t G, int32_t n_head, int32_t head_dim, int32_t prefix_splits, int32_t suffix_splits);
int obte_attn_decode_shared(const obte_bf16* q, int64_t q_ld, const obte_bf16* prefix_cache, int64_t P, int64_t T_pre, int64_t n_prefix,
                            const obte_bf16* suffix_cache, int64_t G, int64_t T_suf, int64_t n_suffix, obte_bf16* o, float* lse, int32_t n_head,
                            int32_t head_dim, float scale, int32_t prefix_splits, int32_t suffix_splits, void* ws, int64_t ws_bytes, obte_stream s);
int64_t obte_block_decode_shared_ws_bytes(int64_t P, int64_t G, int32_t n_embd, int32_t n_head);
int obte_block_decode_shared(const obte_block_desc* d, const obte_bf16* x, obte_bf16* y, const obte_bf16* prefix_cache, int64_t P, int64_t T_pre,
                             int64_t n_prefix, obte_bf16* suffix_cache, int64_t T_suf, int64_t suf_pos, void* ws, int64_t ws_bytes, obte_stream s);

#ifdef __cplusplus
}
#endif
#endif
