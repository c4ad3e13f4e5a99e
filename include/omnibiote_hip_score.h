/* libomnibiote_hip.so — sequence scoring: the readout product fused with its log-softmax (a companion of omnibiote_hip.h, which it
 * includes: the same ABI version, the same conventions — caller-owned buffers, the caller's stream, no allocation, no synchronisation —
 * and no new aggregate type). */
#ifndef OMNIBIOTE_HIP_SCORE_H
#define OMNIBIOTE_HIP_SCORE_H
#include "omnibiote_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

/* ---- log-probabilities of listed tokens at R positions, without the (R, V) logits ----------------------------------------------------
 * x [R, C] bf16 (row stride ldx elements), w [V, C] bf16 (row stride ldw; the readout weight, k-contiguous like every forward product),
 * targets [R, K] int32, logprobs [R, K] fp32, lse [R] fp32, logits_at [R, K] fp32.
 *   z[r, v]          = bf16(alpha * sum_c x[r, c] w[v, c]), accumulated in fp32 and rounded once: obte_gemm_bf16's rule for the readout
 *   lse[r]           = log sum_{v < V} exp(z[r, v]), in fp32 with the maximum subtracted
 *   logits_at[r, k]  = z[r, targets[r, k]]
 *   logprobs[r, k]   = logits_at[r, k] - lse[r], one fp32 subtraction
 * A target of -1 means "no candidate": both outputs are 0 there.  Any other value outside [0, V) is the caller's error: nothing is read
 * out of bounds for it and both outputs are NaN.
 * Two launches.  The first is a 128 x 128 tile product whose workgroups each own one 128-row tile of x and one contiguous slice of the
 * vocabulary: after every tile's K loop the tile is staged in LDS as bf16, columns >= V are masked to -inf, a running (max, sum) per row
 * is updated in registers, and a target that lies in the tile is read from the staged tile into logits_at.  Per row and slice one
 * (max, sum) pair goes to ws.  The second launch combines a row's pairs in slice order into lse and writes logprobs.  Nothing of size
 * R V is allocated or written: ws is 8 R slices bytes.  `slices` = 0 picks the split that obte_readout_score_slices reports (row tiles x
 * slices fills the device about twice, at most 64 and at most one slice per 128 columns); more slices than 128-column tiles are
 * treated as that many.  Results are bitwise repeatable, and at a fixed `slices` row r's three outputs have the same bits whatever R
 * is and whatever the other rows hold.  Correct for R = 1, but a tile product: not a weight-streaming kernel for few rows.
 * OBTE_EINVAL before any launch: a null pointer; R < 1; V < 1 or V >= 2^31; K < 1 or K > 64; C < 64 or C % 64 != 0; ldx or ldw not a
 * multiple of 8, smaller than C or above 2^22; slices outside [0, 64]; ws_bytes below obte_readout_score_ws_bytes(R, V, slices); x or
 * w not 16-byte aligned, ws not 8-byte aligned, targets, logprobs, lse or logits_at not 4-byte aligned.
 * obte_readout_score_slices returns 1 and obte_readout_score_ws_bytes -1 for arguments outside those ranges. */
int32_t obte_readout_score_slices(int64_t R, int64_t V);
int64_t obte_readout_score_ws_bytes(int64_t R, int64_t V, int32_t slices);
int obte_readout_score_bf16(const void* x, int64_t ldx, const void* w, int64_t ldw, int64_t R, int64_t V, int64_t C, float alpha,
                            const void* targets, int64_t K, void* logprobs, void* lse, void* logits_at,
                            int32_t slices, void* ws, int64_t ws_bytes, obte_stream stream);

#ifdef __cplusplus
}
#endif
#endif
