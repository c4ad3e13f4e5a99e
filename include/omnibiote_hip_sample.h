/* libomnibiote_hip.so — next-token sampling on the device (a companion of omnibiote_hip.h, which it includes: the same ABI version, the
 * same conventions — caller-owned buffers, the caller's stream, no allocation, no synchronisation — and no new struct). */
#ifndef OMNIBIOTE_HIP_SAMPLE_H
#define OMNIBIOTE_HIP_SAMPLE_H
#include "omnibiote_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

/* ---- a token from every row of logits: temperature, top-k, top-p, softmax and the draw in one launch -------------------------------
 * logits [B, V] bf16 (row stride ld elements; 1 <= V <= 65536, more is OBTE_EUNSUPPORTED), u [B] uniform numbers or NULL, token [B],
 * n_kept [B] or NULL.  Per row, with T = temperature:
 *   kept set   every entry whose value is at least a threshold value, so a tie at the threshold is kept whole; NaN and -inf are never
 *              kept.  top_k >= 1: the threshold is the k-th largest value (top_k <= 0 or >= V: no cut).  top_p < 1, applied to what
 *              top-k kept, with weights exp((x - max) / T): walking the distinct values downwards and adding each value's whole mass,
 *              the threshold is the first value at which the running mass reaches top_p times the total (top_p = 1: no cut).  The
 *              largest value is always kept.
 *   draw       over the kept entries in index order the token is the first index whose cumulative probability exceeds u[b]; u >= 1
 *              gives the last kept entry of non-zero weight, u < 0 or NaN the first.
 *   greedy     u == NULL, T == 0 or top_k == 1: the lowest index of the row maximum, n_kept = 1.
 *   nothing    a row with no entry above -inf that is not NaN: token 0, n_kept = 0.  A row holding +inf gives a +inf entry.
 * The weights are 64-bit fixed point, floor(exp2((x - max) log2(e) / T) 2^40) with the hardware's exp2 (about one fp32 ulp): every sum
 * is an integer sum, so a call's result is bitwise repeatable, and row b's depends on row b and u[b] alone, whatever B is.  An entry whose
 * weight is below 2^-40 of the maximum's carries weight zero: it counts in n_kept and is never drawn.  A cumulative probability
 * differs from its exact value by a few 1e-7.  n_kept[b] is the size of the kept set.
 * One workgroup per row holds the row in registers: the row is read once, 16 bytes at a time — the group of 8 columns that holds
 * column V - 1 is read whole (ld % 8 == 0 keeps it inside the row), but columns >= V never reach a result, and nothing but token[0..B)
 * and n_kept[0..B) is written.  No workspace, no atomics on global memory.  Safe for any bit pattern in logits and u.
 * OBTE_EINVAL before any launch: logits or token NULL; logits not 16-byte aligned, ld % 8 != 0 or ld < V; B < 1 or V < 1; temperature
 * negative or not finite; top_p outside (0, 1] or NaN; u or n_kept not 4-byte aligned, token not 8-byte aligned.
 * The launch profiler records kind 114 over (B, V, greedy). */
int obte_sample_logits_bf16(const obte_bf16* logits, int64_t ld, int64_t B, int64_t V, const float* u, float temperature, int32_t top_k, float top_p,
                            int64_t* token, int32_t* n_kept, obte_stream s);

#ifdef __cplusplus
}
#endif
#endif
