/* libomnibiote_hip.so — the generation loop's state on the device (a companion of omnibiote_hip.h, which it includes: the same ABI
 * version, the same conventions — caller-owned buffers, the caller's stream, no allocation, no synchronisation — and no new struct). */
#ifndef OMNIBIOTE_HIP_LOOP_H
#define OMNIBIOTE_HIP_LOOP_H
#include "omnibiote_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

/* ---- a step's sampled tokens into the next step's inputs, in one launch ---------------------------------------------------------------
 * Everything a generation loop does between the sampler and the next step's first block, with no value passing through the host: a
 * launch's arguments are the same for every step, so a captured graph can replay it.  All state is per row; row b of every array is read
 * and written by row b's workgroup alone.
 *   sampled [B] int64   the tokens the sampler drew from this step's logits (read only)
 *   pos     [B] int32   row b's next cache position, the rows convention of omnibiote_hip_rows.h: >= 0 running, negative parked
 *   count   [B] int32   the steps row b has seen
 *   out     [B, out_ld] int64, n_new [B] int32   the tokens row b has emitted and how many
 *   token   [B] int64   row b's last emitted token: the next step's input
 *   wte     [vocab, cols] bf16, x [B, cols] bf16   the embedding table and the next step's activations
 *   us      [us_steps, B] fp32 or NULL, u [B] fp32   the uniforms of a whole call and the next step's row of them (u is not touched,
 *                                                    and may be NULL, when us is NULL)
 * For row b, with commit 0 or 1 (host) and eos (host; negative: none):
 *   p = pos[b]; the row is RUNNING iff p >= 0.  If commit != 0 and running: p += 1 (the step that just ran stored at p).
 *   s = count[b], t = sampled[b].
 *   If running and 0 <= s < out_ld:  out[b, s] = t,  n_new[b] += 1,  token[b] = t,  and if eos >= 0 and t == eos: p = -1 (parked).
 *   Otherwise nothing of out, n_new or token changes (a parked row; a row whose out is full goes on running, unrecorded).
 *   pos[b] = p, count[b] = s + 1.  (32-bit wrap-around, never undefined: a position that wraps is negative, hence parked.)
 *   x[b, :] = wte[clamp(token[b], 0, vocab - 1), :] for EVERY row, parked or not, from the token[b] this call leaves: 16 bytes per
 *     lane, the bytes of obte_embedding_fwd.  A parked row's activations are finite; nobody reads them.
 *   If us != NULL:  u[b] = us[clamp(s + 1, 0, us_steps - 1) * B + b], the next step's uniforms.
 * One workgroup per row.  Nothing but pos, count, u, x, token[0..B), n_new[0..B) and out[b, s] is written.  No workspace, no atomics, no
 * flags.  Memory-safe for any bit pattern in sampled, pos, count and token: no index is formed from them without a clamp or the range
 * check above.
 * OBTE_EINVAL before any launch: sampled, pos, count, out, n_new, token, wte or x NULL, or us given and u NULL; wte or x not 16-byte
 * aligned; sampled, out or token not 8-byte aligned; pos, count, n_new, us or u not 4-byte aligned; cols < 8 or cols % 8 != 0; B < 1 or
 * B >= 2^31; vocab < 1; out_ld < 1; us given and us_steps < 1. */
int obte_gen_advance(const int64_t* sampled, int32_t* pos, int32_t* count, int64_t* out, int64_t out_ld, int32_t* n_new, int64_t* token,
                     const obte_bf16* wte, int64_t vocab, int32_t cols, obte_bf16* x, const float* us, int64_t us_steps, float* u, int64_t eos,
                     int32_t commit, int64_t B, obte_stream s);

#ifdef __cplusplus
}
#endif
#endif
