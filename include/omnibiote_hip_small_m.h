/* libomnibiote_hip.so — the weight-streaming product for small M (a companion of omnibiote_hip.h, which it includes: the same ABI
 * version, the same conventions — caller-owned buffers, the caller's stream, no allocation, no synchronisation — and no new struct). */
#ifndef OMNIBIOTE_HIP_SMALL_M_H
#define OMNIBIOTE_HIP_SMALL_M_H
#include "omnibiote_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

/* ---- x W^T for 1 <= M <= 64 rows: generation at the weights' read rate ------------------------------------------------
 * D[M, N] = epilogue(bf16(alpha * sum_k a[m, k] b[n, k])): obte_gemm_bf16's x W^T layout (a_kmajor = b_kmajor = 1, anything else
 * OBTE_EUNSUPPORTED) on a kernel that reads every byte of b once, 16 bytes per lane straight into the MFMA fragment, instead of the
 * 256-row tile structures.  The fields of obte_gemm_args mean what they mean for obte_gemm_bf16 (leading dimensions, alpha, aux, the
 * RoPE fields) and the same rules hold: K % 64 == 0, N % 8 == 0, leading dimensions % 8 == 0, alpha != 1 only with NONE / ADD.
 * Epilogues: OBTE_EPI_NONE, OBTE_EPI_ADD (aux may alias d), OBTE_EPI_GELU_ACT, OBTE_EPI_ROPE_QK, each in the arithmetic of
 * obte_gemm_bf16's — the product rounded to bf16 first, the epilogue on the rounded value — so equal products give equal bits;
 * every other epilogue is OBTE_EUNSUPPORTED.  The fp32 summation order is a function of K alone: row m of d depends on a[m] and b
 * only, has the same bits at every M and in every call.  Rows >= M of a are never read; nothing outside [M, N] of d is written
 * (ldd > N is legal, as is N % 16 == 8).  No workspace.  The launch profiler records kind 8012 + epilogue (structure 8). */
int obte_linear_small_m_bf16(const obte_gemm_args* g, obte_stream s);
/* The largest M = batch at which obte_block_decode / obte_block_decode_rows run their four products through the call above
 * (obte_block_fwd_infer and obte_block_fwd_prefill never do).  0..64, 0 = never; process-wide, read per call; the default is 64, or 0
 * with OBTE_SMALL_M=0 in the environment when the library loads.  Returns the previous value (OBTE_EINVAL, value unchanged, outside 0..64). */
int obte_small_m_max_set(int m);
int obte_small_m_max(void);

#ifdef __cplusplus
}
#endif
#endif
