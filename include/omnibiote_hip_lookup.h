/* libomnibiote_hip.so — speculative decoding without a draft model: an n-gram lookup in a row's own history drafts k tokens on the
 * device, and the verification takes a drafted token in the place of a draft distribution (a companion of omnibiote_hip.h, which it
 * includes: the same ABI version, the same conventions — caller-owned buffers, the caller's stream, no allocation, no synchronisation
 * — and no new struct). */
#ifndef OMNIBIOTE_HIP_LOOKUP_H
#define OMNIBIOTE_HIP_LOOKUP_H
#include "omnibiote_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

#define OBTE_LOOKUP_MAX_HISTORY 8192   /* the longest history row (hist_ld) obte_lookup_draft takes */
#define OBTE_LOOKUP_MAX_NGRAM 16       /* the longest suffix it matches (g_max) */

/* ---- the k tokens that followed the most recent longest earlier occurrence of the row's last tokens -----------------------------------
 * hist int64 [B, hist_ld] and lens int32 [B] on the device; draft int64 [B, k] and match_len int32 [B] are written.  1 <= k <= 31,
 * 1 <= g_min <= g_max <= 16, 1 <= V <= 65536, 1 <= hist_ld <= OBTE_LOOKUP_MAX_HISTORY (more of k or hist_ld is OBTE_EUNSUPPORTED).
 * Row b is active iff 1 <= n = lens[b] <= hist_ld; an inactive row gets draft = zeros and match_len = 0, and no byte of its hist row is
 * read.  For an active row, with h = hist[b]:
 *   equality   a token outside [0, V) equals nothing, not even itself.
 *   m(e)       for a candidate end e in [1, n - 1]: the largest m <= min(g_max, e) with h[e-1-i] == h[n-1-i] for all i < m — how many
 *              of the tokens before position e agree with the row's last tokens.
 *   e*         the e with the largest m(e), among equals the largest e: the most recent occurrence.
 *   match      m(e*) >= g_min: match_len = m(e*), and with the period d = n - e*, draft[j] = h[e* + (j mod d)] — the history continued
 *              periodically past its end, so a tandem repeat of period d is drafted for all k positions and not cut off at n.
 *   otherwise  (n = 1 included) match_len = 0 and every draft[j] = h[n-1]: the same formula with e* = n - 1.
 * The drafted values are hist's own 64-bit values, whatever they are.  The result is a pure function of row b's inputs, whatever B
 * is, and bitwise repeatable.  One launch, one workgroup of 256 threads per row: the row's first n tokens are staged in LDS as 32-bit
 * words (one sentinel for everything outside [0, V)), thread t compares backwards from e = t + 1, t + 257, ..., the best
 * m << 16 | e is a maximum over the workgroup, and the first k lanes write the draft.  Nothing is written but draft[0..B k) and
 * match_len[0..B); no atomics or flags on global memory.  Safe for any bit pattern in hist and lens: no index is formed from a token,
 * none from a length that has not passed the range check.
 * OBTE_EINVAL before any launch: hist, lens, draft or match_len NULL; B < 1 or B >= 2^24; hist_ld < 1; k < 1; g_min < 1, g_max < g_min
 * or g_max > 16; V < 1 or V > 65536; hist or draft not 8-byte aligned, lens or match_len not 4-byte aligned.
 * The launch profiler records kind 122 over (B, hist_ld, k). */
int obte_lookup_draft(const int64_t* hist, int64_t hist_ld, const int32_t* lens, int64_t B, int32_t k, int32_t g_min, int32_t g_max, int64_t V,
                      int64_t* draft, int32_t* match_len, obte_stream s);

/* ---- obte_spec_verify_bf16 (omnibiote_hip_spec.h) for a draft that is a token and not a distribution --------------------------------
 * The arguments of obte_spec_verify_bf16 without q and ld_q, under the same rules, limits and alignment checks.  The draft
 * distribution of position j is the point mass on draft[b, j]: n_accept and token are, bit for bit, what obte_spec_verify_bf16
 * returns when q[b, j] is the row that is 0 at draft[b, j] and -inf everywhere else — a row of all -inf for a drafted token outside
 * [0, V).  In words: x_j stands while u_accept[b, j] < P_j(x_j); behind a rejection at a the token is drawn from P_a with x_a's weight
 * removed (from P_a itself if nothing is left); behind k acceptances it is the sampler's draw on p[b, k].  The greedy form is
 * obte_spec_verify_bf16's, which never reads q.
 * The same two launches with the draft row synthesised instead of loaded: its summary is (total 2^40, weight of x 2^40) and its
 * column weights in the residual are 2^40 at x and 0 elsewhere — the integers obte_spec_verify_bf16 computes of the one-hot row — so
 * the first launch runs B (k + 1) workgroups and no (B, k, V) tensor exists.
 * ws: obte_spec_verify_point_ws_bytes(B, k) = 32 B (k + 1) bytes (0 for B < 1, k < 1 or k > 31), contents irrelevant before and after.
 * OBTE_EINVAL before any launch: as obte_spec_verify_bf16, less the checks of q.
 * The launch profiler records kind 123 over (B, k, V), once for both launches. */
int64_t obte_spec_verify_point_ws_bytes(int64_t B, int64_t k);
int obte_spec_verify_point_bf16(const obte_bf16* p, int64_t ld_p, const int64_t* draft, int64_t B, int64_t k, int64_t V, const float* u_accept,
                                const float* u_draw, float temperature, int32_t top_k, float top_p, int32_t* n_accept, int64_t* token, void* ws,
                                int64_t ws_bytes, obte_stream s);

#ifdef __cplusplus
}
#endif
#endif
