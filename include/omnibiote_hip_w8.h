/* libomnibiote_hip.so — generation with the decode step's weights stored as OCP e4m3 (a companion of omnibiote_hip.h, which it includes:
 * the same ABI version, the same conventions — caller-owned buffers, the caller's stream, no allocation, no synchronisation, every argument
 * checked on the host before any launch with obte_last_error naming the entry point — and no new aggregate type). */
#ifndef OMNIBIOTE_HIP_W8_H
#define OMNIBIOTE_HIP_W8_H
#include "omnibiote_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

/* ---- the format ---------------------------------------------------------------------------------------------------------
 * A weight W [N, K] bf16 is stored as  codes uint8 [N, ld_codes]  and  scales fp32 [N]:  row n is one vector of the e4m3 cache's
 * rule (omnibiote_hip_kv8.h): code = RNE_e4m3(W[n, k] * 2^-e), scale[n] = 2^e, e the smallest integer >= -126 with
 * max_k |W[n, k]| * 2^-e <= 448.  OCP e4m3fn; the scale is a power of two, so float(code) * scale is exactly a bf16 (the dequantised
 * weight), no code is a NaN and nothing saturates.  omnibiote_amd/w8quant.py states the rule in plain torch.
 * Memory order of a row: K / 64 groups of 64 bytes, and within a group byte 16 q + 8 s + j (q < 4, s < 2, j < 8) holds the code of
 * k = 64 group + 32 s + 8 q + j — the two 8-element MFMA fragments of a lane as one 16-byte load (w8quant.pack_codes /
 * unpack_codes).  Bytes K .. ld_codes - 1 of a row are never read. */

/* obte_linear_small_m_bf16 (omnibiote_hip_small_m.h) with W in this format: g means what it means there, except that g->b and g->ldb
 * are ignored.  1 <= M <= 64, K % 64 == 0, N % 8 == 0, epilogues NONE / ADD / GELU_ACT / ROPE_QK with the same alpha rule;
 * ld_codes % 16 == 0, ld_codes >= K, codes 16-byte and scales 4-byte aligned; anything else OBTE_EINVAL / OBTE_EUNSUPPORTED.  Both
 * kernels of the bf16 product, chosen by (N, K) as there, with the same chunk -> wave assignment, chunk order, k -> MFMA slot and wave
 * order of the sum; a lane converts its codes to bf16 fragments exactly and the row's scale multiplies the fp32 sum before alpha:
 * d = epilogue(bf16(alpha * (scale[n] * sum))).  THE CONTRACT: for every supported call d has the bits obte_linear_small_m_bf16 leaves
 * on the dequantised weight bf16(float(code) * scale).  Outside it: a row whose largest magnitude lies below 2^-100, where the
 * dequantised weights or the partial sums of the bf16 product enter the subnormals of bf16 / fp32 and the scale no longer factors out.
 * Rows >= M of a are never read, nothing outside [M, N] of d is written, codes and scales of rows >= N are never read.  No workspace.
 * The launch profiler records kind 9012 + epilogue (structure 9). */
int obte_linear_small_m_w8(const obte_gemm_args* g, const void* codes, int64_t ld_codes, const float* scales, obte_stream s);
/* obte_block_decode / obte_block_decode_rows (pos_rows NULL or a device int32 [B], pos then its bound) on a bf16 cache (cache_e4m3 == 0)
 * or obte_block_decode_kv8 on an e4m3 one (cache_e4m3 != 0), with the four products on the call above: codes[i] / scales[i], two host
 * arrays of four device pointers in the order c_attn, attention c_proj, c_fc, MLP c_proj, each with ld_codes = its K.  d is the
 * descriptor of those calls (d->T == 1) and its four bf16 weight pointers hold the DEQUANTISED weights: at d->B > obte_small_m_max()
 * the products run on the tile structures from them, the same model to that path's summation order.  Workspace:
 * obte_block_decode_ws_bytes. */
int obte_block_step_w8(const obte_block_desc* d, const void* const* codes, const float* const* scales, const obte_bf16* x, obte_bf16* y_out, void* cache,
                       int32_t cache_e4m3, int64_t T_max, int64_t pos, const int32_t* pos_rows, void* ws, int64_t ws_bytes, obte_stream s);

#ifdef __cplusplus
}
#endif
#endif
