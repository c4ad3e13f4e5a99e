/* libomnibiote_hip.so — attention maps: the softmax weights of one layer's attention as a tensor (a companion of omnibiote_hip.h, which
 * it includes: the same ABI version, the same conventions — caller-owned buffers, the caller's stream, no allocation, no
 * synchronisation).  Replaces the reference's flash=False path, training/model.py CausalSelfAttention: att = softmax(q k^T * scale +
 * mask), read there through a forward hook on attn_dropout.  One new aggregate type, obte_attn_probs_args; obte_struct_sizes does not
 * list it (its six entries stay as they are), obte_attn_probs_args_bytes() returns its size instead. */
#ifndef OMNIBIOTE_HIP_PROBS_H
#define OMNIBIOTE_HIP_PROBS_H
#include "omnibiote_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

/* ---- P[b, h, i, j] = exp(s_ij - m_i) / l_i ---------------------------------------------------------------------------------------------
 *   s_ij = (q_i . k_j) * scale (+ mask[b, h, i, j]), the product on the bf16 MFMA with fp32 accumulation, everything after it in fp32;
 *   m_i  = max_j s_ij and l_i = sum_j exp(s_ij - m_i) over the keys the mask form includes.
 * qkv, key_ranges, mask (+ element strides), ranges_exact: exactly what obte_attn_fwd_args names so, with its three mask forms —
 *   no mask;  key_ranges alone: key j is included for query i iff k_start <= j < k_end (causal and document-causal masks are ranges), an
 *   excluded key's weight is exactly 0 and a query with an empty range has a row of zeros;  a dense additive mask (any strides, the last
 *   dimension contiguous): every key j < T is included and the mask's values decide — key_ranges beside it are obte_mask_bounds' loop
 *   bounds (key tiles outside the union of a 128-query block's bounds are written as zeros without being computed), and with
 *   ranges_exact the range rule serves a mask that flag says IS a range mask.
 * A row whose every key carries a -1e9-class mask value comes out as fp32 arithmetic leaves it: the scores vanish beside the mask and
 * the row is uniform, 1/T per key — what obte_attn_fwd computes its output row from as well.
 * out: fp32 (out_bf16 = 0) or bf16 (out_bf16 = 1: the round-to-nearest-even bf16 of the fp32 value).  Batch element b starts at element
 * b * out_sb; within it the layout is contiguous, [n_head][T][T], or [T][T] with head_mean = 1: (1 / n_head) * sum over the heads in
 * ascending order, in fp32.  out_sb >= that payload, so one call can write one layer's slice of a larger tensor; every element of the
 * payload is written, nothing between two batch elements' payloads is touched.  All offsets are 64-bit.
 * Two launches of one tile body (128 queries x 64 keys per workgroup step, head size 64 or 128, any T >= 1): the first leaves the pair
 * (m_i in log2 units, l_i) per (b, h, i) in ws, the second recomputes every score tile and stores the weights.  The forward's lse is not
 * taken: one fp32 cannot hold log l beside m ~ -1e9.  No atomics: the results are bitwise repeatable.
 * The opt-in launch profiler (obte_profile_*) records a call, both launches in one record, as kind 121 over (maps stored = B or
 * B * n_head, T, head_dim).
 * ws: obte_attn_probs_ws_bytes(B, T, n_head) = 8 * B * n_head * T bytes (0 for B, T or n_head < 1), contents irrelevant before and after.
 * OBTE_EINVAL before any launch: null args, qkv, out or ws; B, T or n_head < 1, B or n_head >= 65536, T >= 2^24; head_dim other than 64
 * or 128; out_sb below the payload; ws_bytes below obte_attn_probs_ws_bytes(); qkv not 16-byte aligned, ws not 8-byte aligned, out not
 * aligned to its element (4 or 2 bytes), key_ranges not 4-byte or mask not 2-byte aligned. */
typedef struct {
    const obte_bf16* qkv;                       /* [B*T, 3C] packed and rotated, as obte_attn_fwd reads it */
    const int32_t* key_ranges;                  /* [B*T, 2] or null */
    const obte_bf16* mask;                      /* additive, or null */
    int64_t mask_sb, mask_sh, mask_sq;          /* element strides of mask's batch, head and query dimensions */
    const int32_t* ranges_exact;                /* nullable; with mask + key_ranges: the device flag obte_mask_bounds wrote */
    int64_t B, T;
    int32_t n_head, head_dim;
    float scale;
    void* out;
    int64_t out_sb;                             /* elements between two batch elements of out */
    int32_t out_bf16;                           /* 0: fp32, 1: bf16 */
    int32_t head_mean;                          /* 0: every head, 1: their mean */
    void* ws;
    int64_t ws_bytes;
} obte_attn_probs_args;

int64_t obte_attn_probs_args_bytes(void);
int64_t obte_attn_probs_ws_bytes(int64_t B, int64_t T, int32_t n_head);
int obte_attn_probs(const obte_attn_probs_args* a, obte_stream s);

#ifdef __cplusplus
}
#endif
#endif
