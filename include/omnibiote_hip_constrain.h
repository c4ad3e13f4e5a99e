/* libomnibiote_hip.so — constrained generation: the sampler and the draft verification over a restricted vocabulary (a companion of
 * omnibiote_hip.h, which it includes: the same ABI version, the same conventions — caller-owned buffers, the caller's stream, no
 * allocation, no synchronisation — and no new aggregate type). */
#ifndef OMNIBIOTE_HIP_CONSTRAIN_H
#define OMNIBIOTE_HIP_CONSTRAIN_H
#include "omnibiote_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

/* ---- obte_sample_logits_bf16 and obte_spec_verify_bf16 with columns excluded per row ------------------------------------------------
 * Both functions take, on top of every argument of the function they restrict (omnibiote_hip_sample.h, omnibiote_hip_spec.h):
 *   allowed      a bit mask of the columns, or NULL (no mask).  Column i of batch row b is EXCLUDED if allowed != NULL and bit i & 7 of
 *                byte allowed[b allowed_ld + (i >> 3)] is 0.  allowed_ld == 0: one mask for every row; otherwise allowed_ld >= ceil(V / 8)
 *                bytes between the rows' masks.  Bits of columns >= V are ignored.  Exactly ceil(V / 8) bytes per mask row are read, at
 *                any alignment.
 *   hold_token   column hold_token is also excluded in row b while (emitted ? emitted[b] : 0) + j < min_emitted, emitted [B] int32 or
 *                NULL.  j is 0 in the sampler; in the verification j is the drafted position 0..k of the logits row, applied to p[b, j]
 *                and to q[b, j] alike, so a hold may end in the middle of a drafted block.  hold_token < 0 or >= V holds nothing.  The
 *                sum is formed in 64 bits: it cannot overflow, whatever emitted holds.
 * An excluded column is treated exactly as an entry holding -inf: it is never kept, does not count towards top-k, carries no mass and
 * is never the maximum.  A row with nothing left gives token 0 and n_kept 0.  A drafted token that is excluded has P_j(x) = 0 and never
 * stands (in a greedy call: it is not the lowest index of the maximum of what is left).  The result is, bit for bit, what the
 * unrestricted function gives on a copy of the logits whose excluded columns were overwritten with -inf: both see key 0 in the same
 * places, and every sum is an integer sum.
 * Everything else is the rule of omnibiote_hip_sample.h / omnibiote_hip_spec.h word for word: the kept set, the 2^40 fixed-point
 * weights, the draw, the exact acceptance test, the residual and its one rounding, greedy mode (u == NULL, temperature == 0 or
 * top_k == 1), the launch shapes, obte_spec_verify_ws_bytes and the workspace's layout, bitwise repeatability and row independence.
 * Safe for any bit pattern in logits / p / q, u, draft, emitted and the mask: no index is formed from them without a range check.
 * The lane that loads the 16 bytes of columns 8 c .. 8 c + 7 loads byte c of its row's mask, 64 consecutive bytes per wave, and clears
 * the excluded keys as it packs them; the verification's second launch, which reads p[b, a] and q[b, a] once more, applies the same
 * exclusion with j = a.  Nothing is written but token[0..B), n_kept[0..B) / n_accept[0..B) and the workspace; no atomics or flags on
 * global memory.
 * OBTE_EINVAL before any launch: everything the restricted function rejects, and allowed_ld < 0, allowed_ld non-zero and smaller than
 * ceil(V / 8), emitted not 4-byte aligned, min_emitted < 0.  allowed == NULL with nothing held is legal and gives the unrestricted
 * function's bits.  The launch profiler records the kinds of the unrestricted functions, 114 and 115. */
int obte_sample_logits_constrained_bf16(const obte_bf16* logits, int64_t ld, int64_t B, int64_t V, const float* u, float temperature, int32_t top_k,
                                        float top_p, const uint8_t* allowed, int64_t allowed_ld, int64_t hold_token, const int32_t* emitted,
                                        int32_t min_emitted, int64_t* token, int32_t* n_kept, obte_stream s);
int obte_spec_verify_constrained_bf16(const obte_bf16* p, int64_t ld_p, const obte_bf16* q, int64_t ld_q, const int64_t* draft, int64_t B, int64_t k,
                                      int64_t V, const float* u_accept, const float* u_draw, float temperature, int32_t top_k, float top_p,
                                      const uint8_t* allowed, int64_t allowed_ld, int64_t hold_token, const int32_t* emitted, int32_t min_emitted,
                                      int32_t* n_accept, int64_t* token, void* ws, int64_t ws_bytes, obte_stream s);

#ifdef __cplusplus
}
#endif
#endif
