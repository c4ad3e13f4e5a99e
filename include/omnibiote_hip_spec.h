/* libomnibiote_hip.so — speculative decoding: verification of a block of drafted tokens on the device (a companion of omnibiote_hip.h,
 * which it includes: the same ABI version, the same conventions — caller-owned buffers, the caller's stream, no allocation, no
 * synchronisation — and no new struct). */
#ifndef OMNIBIOTE_HIP_SPEC_H
#define OMNIBIOTE_HIP_SPEC_H
#include "omnibiote_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

/* ---- which of k drafted tokens stand, and the token behind them ----------------------------------------------------------------------
 * Per batch row b: target logits p[b, 0..k] (row b (k + 1) + j of p, stride ld_p elements), draft logits q[b, 0..k-1] (row b k + j of q),
 * the drafted tokens draft[b, 0..k-1], uniforms u_accept[b, 0..k-1] and u_draw[b].  1 <= V <= 65536 and 1 <= k <= 31 (more of either is
 * OBTE_EUNSUPPORTED).  P_j and Q_j are the distributions obte_sample_logits_bf16 (omnibiote_hip_sample.h) draws from on p[b, j] and
 * q[b, j] under the same temperature, top_k and top_p: the same kept set and the same 2^40 fixed-point weights w with their integer
 * total t, so P_j(i) = wp_i / tp and Q_j(i) = wq_i / tq are ratios of integers.
 *   accept     walking j = 0, 1, ...: x = draft[b, j] stands while u_accept[b, j] < P_j(x) / Q_j(x).  P_j(x) = 0 (not kept by the target,
 *              weight below 2^-40 of the maximum's, or x outside [0, V): such an x is never used as an index) never stands; otherwise
 *              Q_j(x) = 0 stands; a u that is NaN, negative or zero counts as 0.  The comparison is exact: u is a float m 2^e, and
 *              m 2^e (wq_x tp) < wp_x tq is decided in 128-bit integers — no operand is rounded at all.
 *   n_accept   a = the number that stand, 0 <= a <= k.
 *   token      a == k: the draw of obte_sample_logits_bf16 on p[b, k] and u_draw[b], bit for bit (the same integers).  a < k: the first
 *              index whose cumulative probability exceeds u_draw[b] under max(0, P_a - Q_a), renormalised; u_draw >= 1 gives the last
 *              entry of non-zero weight, < 0 or NaN the first.  Each entry is rounded once, to the integer
 *                  r_i = floor(max(0, wp_i tq - wq_i tp) / 2^S),   S = bits(tp) + bits(tq) - 62   (bits(t): the position of t's top bit + 1)
 *              with the products exact in 128 bits; the r_i sum below 2^62 and the token is found in their integer prefix sums
 *              (a cumulative probability is off by less than 65536 / 2^60 of the residual's mass for this rounding, plus the
 *              weights' own few 1e-7).  All r_i zero (P_a <= Q_a everywhere), or a draft row with nothing to sample: the draw is from P_a.
 *              A target row with no entry above -inf that is not NaN gives token 0.
 *   greedy     u_accept == NULL, u_draw == NULL, temperature == 0 or top_k == 1: x stands while it is the lowest index of p[b, j]'s
 *              maximum (0 for a row with nothing); token is that index of p[b, a].  q is not read and may be NULL — only then.
 * Every sum is an integer sum: a call's result is bitwise repeatable, and row b's depends on row b's inputs alone, whatever B is.
 * Two launches: one workgroup per logits row — B (2 k + 1) of them, B (k + 1) when greedy — leaves 32 bytes in ws (the row's maximum
 * and its lowest index, threshold, integer total, kept count, the drafted token's weight); then one workgroup per batch row finds a,
 * reads p[b, a] (and q[b, a] when a < k) once more and draws.  Rows are read 16 bytes at a time as the sampler reads them (the group of 8
 * columns that holds column V - 1 is read whole; columns >= V never reach a result).  Nothing is written but n_accept[0..B), token[0..B)
 * and ws[0..obte_spec_verify_ws_bytes(B, k)); no atomics or flags on global memory.  Safe for any bit pattern in p, q, u_accept, u_draw
 * and draft.
 * OBTE_EINVAL before any launch: p, draft, n_accept, token or ws NULL; q NULL when the call is not greedy; p or q not 16-byte aligned,
 * ld_p or ld_q not a multiple of 8 or smaller than V; B < 1, k < 1 or V < 1; temperature negative or not finite; top_p outside (0, 1] or
 * NaN; u_accept, u_draw or n_accept not 4-byte aligned, draft, token or ws not 8-byte aligned; ws_bytes too small.
 * The launch profiler records kind 115 over (B, k, V), once for both launches. */
int64_t obte_spec_verify_ws_bytes(int64_t B, int64_t k);
int obte_spec_verify_bf16(const obte_bf16* p, int64_t ld_p, const obte_bf16* q, int64_t ld_q, const int64_t* draft, int64_t B, int64_t k, int64_t V,
                          const float* u_accept, const float* u_draw, float temperature, int32_t top_k, float top_p, int32_t* n_accept, int64_t* token,
                          void* ws, int64_t ws_bytes, obte_stream s);

#ifdef __cplusplus
}
#endif
#endif
