"""The e4m3 weight format of the decode step's products in plain torch (include/omnibiote_hip_w8.h): the tests' yardstick for
csrc/gemm_small_m.hip's WE4m3 policy, as kvquant.py is for the cache.  Quantising and packing run here, once per model, on any device;
there is no kernel for them.

A weight W (N, K) bf16, K % 64 == 0, is stored as codes uint8 (N, K) and scales fp32 (N,).  Row n is ONE vector of
``kvquant.quantize_reference``: the same amax rule, the same round-to-nearest-even conversion to OCP e4m3fn, a power-of-two scale, no NaN
code, nothing saturates.  One scale per output row.  ``float(code) * scale`` has at most 4 significant bits and is exactly a bf16: the
dequantised weight, which ``dequantize_weight`` returns.  The worst error of one weight is half an e4m3 step at the top binade, 16 scaled
units against a row maximum above 224: below amax / 14.

Memory order.  The kernel's lane (row l & 15, q = l >> 4) feeds two MFMAs per 64-deep chunk of K, with k = 8 q + j and k = 32 + 8 q + j
(j < 8).  So that both fragments are one 16-byte load, every group of 64 codes is stored permuted: byte 16 q + 8 s + j of the group
holds the code of k = 32 s + 8 q + j.  ``pack_codes`` takes codes in k order to that stored order, ``unpack_codes`` back; everything
else here and in ops / model handles codes in STORED order only, and nothing but this module and the kernel knows what that order is."""
from __future__ import annotations

import torch

from . import kvquant

ROW_CHUNK = 4096   # rows quantised at a time: the float64 copy of a 65 536 x 1024 readout would be 512 MB, a chunk's is 32 MB


def _check_codes(codes, what):
    if codes.dtype != torch.uint8 or codes.dim() != 2 or codes.shape[1] % 64 != 0:
        raise ValueError(f"{what}: expected uint8 (N, K) with K a multiple of 64, got {codes.dtype} {tuple(codes.shape)}")


def pack_codes(codes):
    """codes uint8 (N, K) in k order -> the stored order (a new contiguous tensor)"""
    _check_codes(codes, "pack_codes")
    n, k = codes.shape
    return codes.reshape(n, k // 64, 2, 4, 8).permute(0, 1, 3, 2, 4).reshape(n, k).contiguous()


def unpack_codes(packed):
    """the inverse of pack_codes"""
    _check_codes(packed, "unpack_codes")
    n, k = packed.shape
    return packed.reshape(n, k // 64, 4, 2, 8).permute(0, 1, 3, 2, 4).reshape(n, k).contiguous()


def quantize_weight(w):
    """W (N, K) bf16 -> (codes uint8 (N, K) in stored order, scales fp32 (N,))"""
    if w.dtype != torch.bfloat16 or w.dim() != 2 or w.shape[1] % 64 != 0:
        raise ValueError(f"quantize_weight: expected bf16 (N, K) with K a multiple of 64, got {w.dtype} {tuple(w.shape)}")
    codes = torch.empty(w.shape, dtype=torch.uint8, device=w.device)
    scales = torch.empty(w.shape[0], dtype=torch.float32, device=w.device)
    for r in range(0, w.shape[0], ROW_CHUNK):
        c, s = kvquant.quantize_reference(w[r:r + ROW_CHUNK].detach())
        codes[r:r + ROW_CHUNK] = pack_codes(c)
        scales[r:r + ROW_CHUNK] = s
    return codes, scales


def dequantize_weight(codes, scales):
    """codes uint8 (N, K) in stored order, scales fp32 (N,) -> bf16 (N, K): float(code) * scale, exactly (the fp32 product is exact and
    has at most 4 significant bits).  The corners: a row whose maximum lies within 1/16 of bf16's largest value has the code 256 under
    the scale 2^120, and 2^128 is +inf; a row under the smallest scale 2^-126 can hold values below bf16's smallest normal."""
    _check_codes(codes, "dequantize_weight")
    if scales.dtype != torch.float32 or scales.shape != (codes.shape[0],):
        raise ValueError(f"dequantize_weight: scales must be float32 ({codes.shape[0]},), got {scales.dtype} {tuple(scales.shape)}")
    out = torch.empty(codes.shape, dtype=torch.bfloat16, device=codes.device)
    for r in range(0, codes.shape[0], ROW_CHUNK):
        out[r:r + ROW_CHUNK] = kvquant.dequantize_reference(unpack_codes(codes[r:r + ROW_CHUNK]), scales[r:r + ROW_CHUNK]).to(torch.bfloat16)
    return out
