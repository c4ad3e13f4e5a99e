/* libomnibiote_hip.so — beam search: the selection of the W best continuations per prompt on the device, and one-query attention /
 * the decode step of a block over a shared-prefix cache whose suffix slots are read through an ancestry table (a companion of
 * omnibiote_hip.h, which it includes: the same ABI version, the same conventions — caller-owned buffers, the caller's stream, no
 * allocation, no synchronisation, no atomics or flags in global memory, every argument checked on the host before any launch — and no
 * new aggregate type). */
#ifndef OMNIBIOTE_HIP_BEAM_H
#define OMNIBIOTE_HIP_BEAM_H
#include "omnibiote_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

/* ---- P prompts, W beams of each ------------------------------------------------------------------------------------------------
 * B = P*W rows, row b = p*W + g is beam g of prompt p (the layout of omnibiote_hip_shared.h with G = W).  1 <= W <= OBTE_BEAM_MAX_WIDTH
 * (one query tile of the prefix launch; W*W <= 1024 merge candidates per group), 1 <= V <= 65536 (more is OBTE_EUNSUPPORTED).
 *
 * obte_beam_select_bf16: one beam step for all P groups.
 *   in   logits bf16 [B, V] (row stride ld elements; 16-byte aligned, ld % 8 == 0, ld >= V: obte_sample_logits_bf16's rules), score_in
 *        fp32 [B], done_in uint8 [B], eos_token (-1: none; else inside [0, V)), allowed / allowed_ld (the packed bit mask of
 *        omnibiote_hip_constrain.h: NULL, one row for all with allowed_ld = 0, or one row per logits row allowed_ld >= ceil(V / 8) bytes
 *        apart), ancestry_in int32 [B, T_suf], slot (the suffix slot the chosen tokens will occupy, 0 <= slot < T_suf).
 *   out  parent int32 [B] (a global row index inside the row's own group), token int64 [B], score_out fp32 [B], done_out uint8 [B],
 *        ancestry_out int32 [B, T_suf] (must not overlap ancestry_in), token_hist int64 [T_suf, B] of which row `slot` is written.
 *        score_out / done_out may be score_in / done_in themselves: the first launch has read them into the workspace.
 * The rule (omnibiote_amd/sampling.py, beam_step_reference, states it in float64):
 *   - a LIVE row (score_in finite, done_in 0) proposes (b, v) for every column v that is not NaN, not -inf and not excluded by the mask,
 *     with S = score_in[b] + (x_v - max_b) - ln Z_b, Z_b = sum over the row's candidate columns of exp(x - max_b).  The entries equal
 *     to the maximum have x - max = 0 exactly (a row holding +inf proposes its +inf entries); a column whose S is -inf in fp32 is no
 *     candidate.
 *   - ln Z_b comes from the INTEGER sum of the 2^40 fixed-point weights of obte_sample_logits_bf16 at temperature 1,
 *     ln Z_b = ln(sum_v floor(exp2((x_v - max_b) log2 e) 2^40)) - 40 ln 2, formed in double: bitwise repeatable and a function of row b
 *     alone, whatever P and W are; it differs from the exact value by about 1e-7.  S is summed in double and rounded to fp32 once.
 *   - a DONE row (done_in != 0) with a finite score proposes exactly one candidate, (b, eos_token) with S = score_in[b] (token 0 with no
 *     eos_token).
 *   - a DEAD row (score_in -inf, +inf or NaN) and a row without a candidate column propose nothing.
 *   - per group the W best candidates by S descending go to the group's rows in rank order, rank r to row p*W + r; equal fp32 S breaks to
 *     the lower beam, then the lower token.  Within a row the order by S is the order by x, so the first launch reduces every row to its
 *     W best columns by (x descending, column ascending) and the second merges the W*W candidates of a group.
 *   - parent[p*W + r] = the candidate's row, token = its column, score_out = S, done_out = done_in[parent] or token == eos_token.
 *   - a group with fewer than W candidates leaves the remaining ranks dead: parent = the row itself, token = eos_token (0 if none),
 *     score_out = -inf, done_out = 1.
 *   - ancestry_out[b][j] = ancestry_in[parent[b]][j] for j < slot and ancestry_out[b][slot] = b % W; entries j > slot are neither
 *     written nor read.  Values are local beam indices in [0, W); what ancestry_in holds is copied as it is.
 *   - token_hist[slot][b] = token[b].
 * Any bit pattern in logits, score_in, done_in and the mask is safe; columns >= V never reach a result; nothing outside the listed
 * outputs and the workspace is written.  Two calls give the same bytes; group p's outputs do not depend on P.
 * Two launches: one workgroup per row (the row read once, 16 bytes per lane, held in registers as obte_sample_logits_bf16 holds it: its
 * maximum, the integer normaliser, the two-level select of the W-th largest value, the ties at that value by ascending column), then one
 * workgroup per group.  ws: obte_beam_select_ws_bytes(P, W) bytes (0 for a rejected shape), 16-byte aligned: per row W packed
 * (key << 16 | 65535 - column) words, then per row (ln Z as a double, score_in, the maximum's key and the row's state).
 * OBTE_EINVAL before any launch: a null pointer among the required ones; P < 1, W outside [1, OBTE_BEAM_MAX_WIDTH], V < 1, T_suf < 1,
 * slot outside [0, T_suf); eos_token < -1 or >= V; logits not 16-byte aligned, ld % 8 != 0, ld < V; allowed_ld negative or non-zero
 * and smaller than ceil(V / 8); score_in, score_out, parent, ancestry_in, ancestry_out not 4-byte aligned, token, token_hist not 8-byte
 * aligned; ancestry_in and ancestry_out overlapping; ws NULL, misaligned or short.
 * The launch profiler records kind 116 over (B, V, W) for the first launch and kind 117 over (P, W, slot) for the second.
 *
 * obte_attn_decode_beam: obte_attn_decode_shared (omnibiote_hip_shared.h) with one more operand, ancestry int32 [B, T_suf], 4-byte
 * aligned (G is the group size: any G obte_attn_decode_shared takes).  Suffix slot j of row b = p*G + g is read from suffix-cache row
 * p*G + ancestry[b][j] instead of row b.  A value outside [0, G) makes that key contribute exactly nothing: its score is -inf, its V a
 * selected zero, and no address is formed from it.  Entries at j >= n_suffix are never read (n_suffix = 0: ancestry may be NULL).
 * Prefix launch, split rules, workspace layout and size (obte_attn_decode_shared_ws_bytes), combine and lse are those of
 * obte_attn_decode_shared; the suffix launch is its kernel with one int32 load per key, issued for a round's keys ahead of their K / V
 * loads.  With ancestry[b][j] = b % G everywhere o and lse are bit for bit obte_attn_decode_shared's; with any table of valid entries
 * they are bit for bit obte_attn_decode_shared's on a suffix cache gathered physically by that table, at the same split counts.
 * The launch profiler records kinds 106 and 107 as obte_attn_decode_shared does and kind 118 over (B * n_head, n_suffix, head_dim) for
 * the suffix launch.
 *
 * obte_block_decode_beam: obte_block_decode_shared with that table (4-byte aligned, [B, T_suf]): the same descriptor rules, the same
 * workspace (obte_block_decode_beam_ws_bytes = obte_block_decode_shared_ws_bytes).  Row b stores its own new key and value at
 * (row b, slot suf_pos) as obte_block_decode_shared does; the table's column suf_pos must already name it (ancestry[b][suf_pos] =
 * b % G: obte_beam_select_bf16 with slot = suf_pos has written exactly that). */
#define OBTE_BEAM_MAX_WIDTH 32
int64_t obte_beam_select_ws_bytes(int64_t P, int64_t W);
int obte_beam_select_bf16(const obte_bf16* logits, int64_t ld, int64_t P, int64_t W, int64_t V, const float* score_in, const uint8_t* done_in,
                          int64_t eos_token, const uint8_t* allowed, int64_t allowed_ld, const int32_t* ancestry_in, int64_t T_suf, int64_t slot,
                          int32_t* parent, int64_t* token, float* score_out, uint8_t* done_out, int32_t* ancestry_out, int64_t* token_hist, void* ws,
                          int64_t ws_bytes, obte_stream s);
int obte_attn_decode_beam(const obte_bf16* q, int64_t q_ld, const obte_bf16* prefix_cache, int64_t P, int64_t T_pre, int64_t n_prefix,
                          const obte_bf16* suffix_cache, int64_t G, int64_t T_suf, int64_t n_suffix, const int32_t* ancestry, obte_bf16* o, float* lse,
                          int32_t n_head, int32_t head_dim, float scale, int32_t prefix_splits, int32_t suffix_splits, void* ws, int64_t ws_bytes,
                          obte_stream s);
int64_t obte_block_decode_beam_ws_bytes(int64_t P, int64_t G, int32_t n_embd, int32_t n_head);
int obte_block_decode_beam(const obte_block_desc* d, const obte_bf16* x, obte_bf16* y, const obte_bf16* prefix_cache, int64_t P, int64_t T_pre,
                           int64_t n_prefix, obte_bf16* suffix_cache, int64_t T_suf, int64_t suf_pos, const int32_t* ancestry, void* ws, int64_t ws_bytes,
                           obte_stream s);

#ifdef __cplusplus
}
#endif
#endif
