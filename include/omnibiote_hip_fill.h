/* libomnibiote_hip.so — encoder infilling: a categorical draw fused into the readout product, and the bookkeeping of an unmasking loop
 * (a companion of omnibiote_hip.h, which it includes: the same ABI version, the same conventions — caller-owned buffers, the caller's
 * stream, no allocation, no synchronisation — and no new aggregate type). */
#ifndef OMNIBIOTE_HIP_FILL_H
#define OMNIBIOTE_HIP_FILL_H
#include "omnibiote_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

/* ---- the noise rule (restated in float64 by omnibiote_amd/sampling.py: gumbel_noise, readout_sample_reference) -----------------------
 * Counter-based, in the style of the dropout mask (csrc/common.h: obte_hash32, drop_rowkey, make_drop).  For a row key k (int64), a
 * column v and a 64-bit seed:
 *   rowkey = drop_rowkey(k, make_drop(0, seed, OBTE_SITE_FILL))        OBTE_SITE_FILL = 8
 *   h      = obte_hash32(rowkey ^ v)                                   32 bits
 *   w      = (h + 0.5) 2^-32                                           in (0, 1)
 *   E      = -ln(1 - w)                                                Exp(1)
 *   g      = -ln E                                                     Gumbel
 *   perturbed[v] = y[v] + g,   y[v] = z[v] inv_temp                    z: obte_readout_score_bf16's bf16 logit; inv_temp an fp32 number
 * The token is argmax_v perturbed[v] (the Gumbel-max rule: a draw from softmax(y)), the smaller column among equal values.  The
 * kernel evaluates the rule in fp32: 1 - w as (~h + 0.5) 2^-32, E by -ln2 log2(1 - w) for w >= 1/16 and by the series
 * w + w^2/2 + ... + w^6/6 below, y as one fp32 product.  g is finite for every h (|g| < 23), and for |y| <= 128 the kernel's perturbed
 * value lies within 2^-15 of the rule's (DESIGN 14.13 has the terms; sampling.GUMBEL_EPS).
 *
 * ---- one token per row drawn from the readout's distribution, without the (R, V) logits ------------------------------------------------
 * x, ldx, w, ldw, R, V, C, alpha: as obte_readout_score_bf16.  keys int64 [R] (NULL: row r has key r), allowed: a packed bit mask of
 * the columns a row may draw (NULL: all) — column v is bit v & 7 of byte v >> 3 (obte_sample_logits_constrained_bf16's layout), row r's
 * mask starts allowed_ld r bytes in, allowed_ld = 0: one mask for all rows; no byte beyond a row's ceil(V / 8) is read and bits of
 * columns >= V are ignored.  tokens int32 [R], logprob fp32 [R], lse fp32 [R]:
 *   lse[r]     = log sum_{v allowed} exp(y[r, v]), in fp32 as obte_readout_score_bf16 forms it (the same order of every sum)
 *   tokens[r]  = argmax over the allowed columns of perturbed[r, v], the smaller column among equal values
 *   logprob[r] = y[r, tokens[r]] - lse[r], one fp32 subtraction: the log-probability of the token under the renormalised distribution
 * inv_temp == 0 is the greedy call: no noise, tokens[r] = the smallest allowed column of the maximal z, lse and logprob as for
 * inv_temp = 1 (with no mask: obte_readout_score_bf16's bits at the same `slices`).  A row that allows nothing (or whose allowed
 * logits are all -inf or NaN) gets tokens = -1 and logprob = -inf.
 * The kernel is obte_readout_score_bf16's — tile body, staging, thread mapping, (max, sum) arithmetic — with a running best
 * (perturbed value, column, y) per thread beside the pair; the combine launch folds the slices' bests under the same total order, so
 * the token depends on neither `slices`, R, the other rows nor a row's place in its tile.  ws holds a pair and a best per row and
 * slice: 20 R slices bytes.  `slices` = 0 picks the split obte_readout_sample_slices reports: the one that minimises (rounds of 512
 * resident workgroups) x (128-column tiles in the longest slice), at most 64 — not always obte_readout_score_slices' choice.  Bitwise
 * repeatable.
 * OBTE_EINVAL before any launch: obte_readout_score_bf16's conditions on the arguments they share; inv_temp negative, infinite or
 * NaN; allowed_ld negative, or positive and below ceil(V / 8); keys not 8-byte aligned; tokens, logprob or lse not 4-byte aligned
 * (allowed may lie at any byte address). */
int32_t obte_readout_sample_slices(int64_t R, int64_t V);
int64_t obte_readout_sample_ws_bytes(int64_t R, int64_t V, int32_t slices);
int obte_readout_sample_bf16(const void* x, int64_t ldx, const void* w, int64_t ldw, int64_t R, int64_t V, int64_t C, float alpha,
                             float inv_temp, uint64_t seed, const int64_t* keys, const void* allowed, int64_t allowed_ld,
                             int32_t* tokens, float* logprob, float* lse, int32_t slices, void* ws, int64_t ws_bytes, obte_stream stream);

/* ---- an unmasking loop's bookkeeping (restated in plain torch by sampling.fill_commit_reference) ---------------------------------------
 * rows int64 [n]: flat positions b T + t of a (B, T) batch, ascending; sequence b's entries are the run [seg_off[b], seg_off[b + 1])
 * (seg_off int32 [B + 1] on the device, at most max_seg entries per sequence: the host's bound, max_seg <= 8192).  tokens int32 [n] and
 * logprob fp32 [n] belong to the entries.  One workgroup per sequence selects take[b] (int32 [B]) of its entries by `order`:
 *   OBTE_FILL_CONFIDENCE (0)  larger logprob first, NaN counted as -inf
 *   OBTE_FILL_RANDOM     (1)  smaller drop_rowkey(position, make_drop(0, seed, OBTE_SITE_FILL)) first
 *   OBTE_FILL_LEFT       (2)  lowest position first
 * equal ranks go to the lower position.  A selected entry's token goes to idx[position] (int64 [n_idx], in place) and its logprob to
 * out_logprob[position] (fp32 [n_idx]); the others' positions go, still ascending, to rows_next[seg_off_next[b] ...] (int64
 * [n_next], seg_off_next int32 [B + 1]).  take[b] outside [0, n_b] makes sequence b a no-op: all of its positions are copied.  Nothing is
 * written through a position outside [0, n_idx) or behind seg_off_next[b + 1] or n_next, a sequence whose run is not inside [0, n] or is
 * longer than max_seg does nothing at all, and no other element of idx or out_logprob is touched.  No atomics and no flags: ranks are
 * counted in LDS.
 * OBTE_EINVAL before the launch: a null pointer; B < 1; n, n_next < 0; n_idx < 1; max_seg outside [0, 8192]; an unknown order;
 * rows_next the same address as rows; rows, rows_next, idx not 8-byte or the others not 4-byte aligned. */
enum { OBTE_FILL_CONFIDENCE = 0, OBTE_FILL_RANDOM = 1, OBTE_FILL_LEFT = 2 };
int obte_fill_commit(const int64_t* rows, const int32_t* seg_off, int64_t n, int64_t B, int32_t max_seg, const int32_t* tokens,
                     const float* logprob, const int32_t* take, int32_t order, uint64_t seed, int64_t* idx, float* out_logprob,
                     int64_t n_idx, int64_t* rows_next, const int32_t* seg_off_next, int64_t n_next, obte_stream stream);

#ifdef __cplusplus
}
#endif
#endif
