/* libomnibiote_hip.so — distillation loss for training an autoregressive model against a teacher (a companion of omnibiote_hip.h,
 * which it includes: the same ABI version, the same conventions — caller-owned buffers, the caller's stream, no allocation, no
 * synchronisation, no atomics or flags — and no new aggregate type). */
#ifndef OMNIBIOTE_HIP_DISTILL_H
#define OMNIBIOTE_HIP_DISTILL_H
#include "omnibiote_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

/* ---- cross entropy + temperature-scaled KL(teacher || student) over listed rows, forward and backward in one launch ------------------
 * logits, teacher_logits, dlogits [n_rows, vocab] bf16 (the compact form: the rows are already the listed ones), target [n_rows] int64
 * (clamped into [0, vocab)), row_scale_vec fp32 [n_rows] or NULL (= 1), row_loss fp32 [n_rows], row_ce / row_kl fp32 [n_rows] or NULL.
 * With s, t a row's student and teacher logits as floats, b = inv_temperature, P = softmax(s), p = softmax(b s), q = softmax(b t) and
 * w = row_scale * row_scale_vec[r]:
 *   CE        = lse(s) - s[target]
 *   KL        = sum_v q_v (b t_v - b s_v) - lse(b t) + lse(b s)
 *   row_ce    = CE,  row_kl = KL                                   (unweighted)
 *   row_loss  = w (ce_weight CE + kl_weight KL)
 *   dlogits_v = bf16( w ( ce_weight (P_v - [v = target]) + kl_weight b (p_v - q_v) ) )      (fp32 arithmetic, one rounding)
 * The usual mix alpha CE + (1 - alpha) tau^2 KL at temperature tau is ce_weight = alpha, kl_weight = (1 - alpha) tau^2, b = 1 / tau.
 * One workgroup of 512 threads per row.  vocab <= 65 536: both rows are loaded once into registers (16-byte loads, all in flight
 * before the first reduction) and the gradient is formed from the registers; above that both rows are read a second time for the
 * gradient.  The same operations in the same order per element either way.  Bitwise repeatable; a row's four results do not depend
 * on n_rows or on the other rows.
 * OBTE_EINVAL before any launch: a null logits, teacher_logits, target, row_loss or dlogits; n_rows < 1 or >= 2^31; vocab < 8,
 * vocab % 8 != 0 or vocab > 131 072; logits, teacher_logits or dlogits not 16-byte aligned; dlogits overlapping either input;
 * inv_temperature not a positive finite number; a weight or row_scale that is not finite. */
int obte_distill_ce_rows(const obte_bf16* logits, const obte_bf16* teacher_logits, const int64_t* target,
                         float row_scale, const float* row_scale_vec, float ce_weight, float kl_weight, float inv_temperature,
                         float* row_loss, float* row_ce, float* row_kl, obte_bf16* dlogits, int64_t n_rows, int64_t vocab,
                         obte_stream s);

#ifdef __cplusplus
}
#endif
#endif
