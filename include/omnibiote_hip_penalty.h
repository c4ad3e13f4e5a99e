/* libomnibiote_hip.so — penalised generation: the sampler with repetition, presence and frequency penalties read from every row's own
 * history (a companion of omnibiote_hip.h, which it includes: the same ABI version, the same conventions — caller-owned buffers, the
 * caller's stream, no allocation, no synchronisation — and no new aggregate type). */
#ifndef OMNIBIOTE_HIP_PENALTY_H
#define OMNIBIOTE_HIP_PENALTY_H
#include "omnibiote_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

/* ---- obte_sample_logits_constrained_bf16 with the columns of the row's history rewritten ------------------------------------------
 * The function takes, on top of every argument of obte_sample_logits_constrained_bf16 (omnibiote_hip_constrain.h):
 *   prompt       int64 token ids, row b at prompt + b prompt_ld, or NULL (then prompt_max must be 0).
 *   prompt_len   [B] int32 on the device, or NULL: every row holds prompt_max ids.  Row b's prompt is its first
 *                prompt_len_b = clamp(prompt_len[b], 0, prompt_max) ids.  prompt_max (host): 0 <= prompt_max <= prompt_ld, < 2^24.
 *   gen          int64 token ids, row b at gen + b gen_ld, or NULL (then gen_max must be 0): what the row has generated.
 *   n_gen        [B] int32 on the device, or NULL.  Row b's generated list is its first
 *                n_gen_b = clamp((n_gen ? n_gen[b] : 0) + n_gen_all, 0, gen_max) ids, the sum formed in 64 bits: it cannot overflow,
 *                whatever n_gen holds.  gen_max (host): 0 <= gen_max <= gen_ld, <= 32767.
 *   repetition   r > 0; inv_repetition = (float)(1.0 / (double)r), computed by the caller: the device does not divide.
 *   presence, frequency   pp and fp.  All four finite fp32.
 * The rule, for row b.  Ids outside [0, V) in either list are ignored.  ctx(i): column i occurs in the prompt or in the generated
 * list; c(i): how often it occurs in the generated list (exact: at most gen_max <= 32767).  For a column with ctx(i), x the fp32 value
 * of its bf16 logit, every operation rounded to fp32 on its own (no fused multiply-add):
 *   1. if r != 1:      x = x < 0 ? x * r : x * inv_repetition
 *   2. if c(i) > 0:    x = x - (pp + fp * (float)c(i))        the product rounded first, then the sum, then the difference
 *   3. the column's logit becomes x rounded to bf16, to nearest even.
 * Every other column keeps its bits.  -inf stays -inf, NaN stays NaN, +inf follows IEEE 754 (+inf - +inf is NaN: the column is never
 * kept).  Repetition acts on prompt and generated tokens alike, once per distinct token; presence and frequency act on generated
 * tokens only.
 * The result is, bit for bit — token, n_kept and every integer sum — what obte_sample_logits_constrained_bf16 gives with the same other
 * arguments on a copy of the logits with these columns rewritten (in plain torch: sampling.penalize_reference).  The mask and the held
 * token apply to the rewritten row: an excluded column is -inf whatever its history.  With repetition == 1, presence == 0 and
 * frequency == 0, or with prompt_max == 0 and gen_max == 0, the call launches the constrained function's kernels and gives its bits.
 * Everything else is the rule of omnibiote_hip_sample.h / omnibiote_hip_constrain.h word for word: the kept set, the 2^40 fixed-point
 * weights, the draw, greedy mode, the three launch shapes, bitwise repeatability and row independence (row b is a function of row b's
 * logits, u, mask, emitted, lists and counts alone).
 * One launch, one workgroup per row.  The workgroup counts the row's history into a table in LDS — one 16-bit entry per column, bit 15
 * "in the prompt", bits 0..14 the generated count, built with LDS atomics, whose integer sums do not depend on their order — and the
 * lane that loads the 16 bytes of columns 8 c .. 8 c + 7 reads its eight entries as one 16-byte LDS read and rewrites the columns
 * whose entry is not 0.  The table is dynamic LDS sized by the launch shape: max(16 ceil(V / 8), 32768) bytes, 128 KiB at V = 65536;
 * the select's histogram reuses it.
 * Read: what the constrained function reads, prompt_len[b] and n_gen[b] where given, and exactly prompt_len_b ids of prompt row b
 * and n_gen_b ids of gen row b — nothing beyond them, whatever lies there.  Written: token[0..B) and n_kept[0..B), nothing else; no
 * atomics, flags or workspace in global memory.  Safe for any bit pattern in logits, u, emitted, the mask, the lists and the counts:
 * no index is formed from them without a range check.
 * OBTE_EINVAL before any launch: everything obte_sample_logits_constrained_bf16 rejects; prompt_max or gen_max negative;
 * gen_max > 32767 or gen_max > gen_ld; prompt_max > prompt_ld or prompt_max >= 2^24; prompt NULL with prompt_max != 0, gen NULL with
 * gen_max != 0; prompt or gen not 8-byte aligned, prompt_len or n_gen not 4-byte aligned; repetition <= 0, or any of repetition,
 * inv_repetition, presence, frequency not finite.  The launch profiler records the sampler's kind, 114. */
int obte_sample_logits_penalized_bf16(const obte_bf16* logits, int64_t ld, int64_t B, int64_t V, const float* u, float temperature, int32_t top_k,
                                      float top_p, const uint8_t* allowed, int64_t allowed_ld, int64_t hold_token, const int32_t* emitted,
                                      int32_t min_emitted, const int64_t* prompt, int64_t prompt_ld, const int32_t* prompt_len, int32_t prompt_max,
                                      const int64_t* gen, int64_t gen_ld, const int32_t* n_gen, int64_t n_gen_all, int32_t gen_max, float repetition,
                                      float inv_repetition, float presence, float frequency, int64_t* token, int32_t* n_kept, obte_stream s);

#ifdef __cplusplus
}
#endif
#endif
