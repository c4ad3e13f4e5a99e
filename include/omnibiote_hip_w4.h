/* libomnibiote_hip.so — generation with the decode step's weights stored as OCP MXFP4 (a companion of omnibiote_hip.h, which it includes:
 * the same ABI version, the same conventions — caller-owned buffers, the caller's stream, no allocation, no synchronisation, every argument
 * checked on the host before any launch with obte_last_error naming the entry point — and no new aggregate type). */
#ifndef OMNIBIOTE_HIP_W4_H
#define OMNIBIOTE_HIP_W4_H
#include "omnibiote_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

/* ---- the format ---------------------------------------------------------------------------------------------------------
 * A weight W [N, K] bf16 is stored as  codes uint8 [N, ld_codes]  (two 4-bit codes per byte, K / 2 bytes used)  and  scales uint8
 * [N, ld_scales]  (K / 32 bytes used).  A block is 32 consecutive k of one row.  Block b of row n has the scale 2^e stored as the e8m0 byte
 * e + 127, e the smallest integer >= -125 with max_block |W| * 2^-e <= 6 (nothing saturates; not the OCP text's floor rule), and its codes are
 * OCP e2m1 (sign bit 3, exponent bits 2-1, mantissa bit 0: magnitudes 0, 0.5, 1, 1.5, 2, 3, 4, 6) of W * 2^-e rounded to nearest, ties to
 * even.  value(code) * 2^e is exactly a bf16 (the dequantised weight).  The quantiser produces no scale byte 0, 1 or 255 and no code 0x8 (-0);
 * the kernel accepts the bytes 1 .. 254 and every code.  omnibiote_amd/w4quant.py states the rule in plain torch.
 * Memory order of a row's codes: K / 64 groups of 32 bytes, and within a group byte 8 q + 4 s + j / 2 (q < 4, s < 2, j < 8) holds the code of
 * k = 64 group + 32 s + 8 q + j, an even j in the low nibble, an odd j in the high one — the two 8-element MFMA fragments of a lane as one
 * 8-byte load, 32 contiguous bytes per row, chunk and wave (w4quant.pack_codes / unpack_codes).  The scale bytes of a row lie in block order:
 * byte b is block b's, k = 32 b .. 32 b + 31.  Bytes K / 2 .. ld_codes - 1 and K / 32 .. ld_scales - 1 of a row are never read. */

/* obte_linear_small_m_bf16 (omnibiote_hip_small_m.h) with W in this format: g means what it means there, except that g->b and g->ldb
 * are ignored.  1 <= M <= 64, K % 64 == 0, N % 8 == 0, epilogues NONE / ADD / GELU_ACT / ROPE_QK with the same alpha rule; row strides in
 * bytes, ld_codes % 8 == 0, ld_codes >= K / 2, ld_scales % 2 == 0, ld_scales >= K / 32; codes 8-byte and scales 2-byte aligned; anything else
 * OBTE_EINVAL / OBTE_EUNSUPPORTED.  Both kernels of the bf16 product, chosen by (N, K) as there, with the same chunk -> wave assignment, chunk
 * order, k -> MFMA slot and wave order of the sum; a lane converts its codes to bf16 fragments with the block's scale applied, exactly, and
 * nothing else differs: d = epilogue(bf16(alpha * sum)).  THE CONTRACT: for every supported call d has the bits obte_linear_small_m_bf16
 * leaves on the dequantised weight.  Rows >= M of a are never read, nothing outside [M, N] of d is written, codes and scales of rows >= N are
 * never read.  No workspace.  The launch profiler records kind 10012 + epilogue (structure 10). */
int obte_linear_small_m_w4(const obte_gemm_args* g, const void* codes, int64_t ld_codes, const void* scales, int64_t ld_scales, obte_stream s);
/* obte_block_step_w8 (omnibiote_hip_w8.h) with the four products on the call above: codes[i] / scales[i], two host arrays of four device
 * pointers in the order c_attn, attention c_proj, c_fc, MLP c_proj, each with ld_codes = its K / 2 and ld_scales = its K / 32.  Both position
 * forms (pos_rows NULL or a device int32 [B], pos then its bound), both cache formats (cache_e4m3).  d's four bf16 weight pointers hold the
 * DEQUANTISED weights: at d->B > obte_small_m_max() the products run on the tile structures from them.  Workspace:
 * obte_block_decode_ws_bytes. */
int obte_block_step_w4(const obte_block_desc* d, const void* const* codes, const void* const* scales, const obte_bf16* x, obte_bf16* y_out, void* cache,
                       int32_t cache_e4m3, int64_t T_max, int64_t pos, const int32_t* pos_rows, void* ws, int64_t ws_bytes, obte_stream s);

#ifdef __cplusplus
}
#endif
#endif
