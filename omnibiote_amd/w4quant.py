"""The MXFP4 weight format of the decode step's products in plain torch (include/omnibiote_hip_w4.h): the tests' yardstick for
csrc/gemm_small_m.hip's WMxfp4 policy, as w8quant.py is for WE4m3.  Quantising and packing run here, once per model, on any device; there
is no kernel for them.

A weight W (N, K) bf16, K % 64 == 0, is stored as codes uint8 (N, K / 2), two 4-bit codes per byte, and scales uint8 (N, K / 32).  One
BLOCK is 32 consecutive k of one row.  Its scale is 2^e, stored as the e8m0 byte e + 127, with e the smallest integer, not below -125,
for which amax_block * 2^-e <= 6: nothing saturates (this is kvquant's amax rule, deliberately not the OCP text's floor(log2 amax) - 2,
which clips up to a quarter of the top binade).  An all-zero block gets e = -125.  The bytes produced are 2 .. 253: never 255 (NaN), 0 or
1.  Its elements are OCP e2m1 codes of W * 2^-e — sign bit 3, exponent bits 2-1, mantissa bit 0; the magnitudes 0, 0.5, 1, 1.5, 2, 3, 4,
6 — rounded to nearest on that grid, ties to the even code.  The quantiser never emits 0x8 (-0); the dequantiser maps it to -0.
``value(code) * 2^e`` has at most 2 significant bits and is exactly a bf16: the dequantised weight, which ``dequantize_weight`` returns.

The worst error of one weight: the scaled block maximum lies above 3 and the widest gap of the grid below 6 is 2, so the error is at most
one scaled unit against a scaled maximum above 3: below amax_block / 3.  (A block clamped at e = -125 is outside that statement: see
``dequantize_weight``.)

Memory order.  The kernel's lane (row l & 15, q = l >> 4) feeds two MFMAs per 64-deep chunk of K, with k = 8 q + j and k = 32 + 8 q + j
(j < 8).  So that both fragments are one 8-byte load, every group of 64 codes is stored permuted in 32 bytes: byte 8 q + 4 s + j // 2 of
the group holds the code of k = 32 s + 8 q + j, an even j in the low nibble and an odd j in the high one.  ``pack_codes`` takes codes in k
order (one per byte) to that stored order, ``unpack_codes`` back; everything else here and in ops / model handles codes in STORED order
only, and nothing but this module and the kernel knows what that order is.  The scale bytes lie in block order: byte b of a row is the
scale of k = 32 b .. 32 b + 31."""
from __future__ import annotations

import torch

ROW_CHUNK = 4096   # rows quantised at a time, as w8quant does: the float64 copy of a chunk of a 65 536 x 1024 readout is 32 MB
E_MIN = -125       # 0.5 * 2^-125 is bf16's smallest normal: no dequantised weight is a subnormal
MAGNITUDES = (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0)


def pack_codes(codes):
    """codes uint8 (N, K) in k order, one code (0 .. 15) per byte -> the stored order, uint8 (N, K / 2) (a new contiguous tensor)"""
    if codes.dtype != torch.uint8 or codes.dim() != 2 or codes.shape[1] % 64 != 0:
        raise ValueError(f"pack_codes: expected uint8 (N, K) with K a multiple of 64, got {codes.dtype} {tuple(codes.shape)}")
    if codes.numel() and int(codes.max()) > 15:
        raise ValueError("pack_codes: a code above 15")
    n, k = codes.shape
    c = codes.reshape(n, k // 64, 2, 4, 4, 2).permute(0, 1, 3, 2, 4, 5)          # (n, group, q, s, j // 2, j & 1)
    return (c[..., 0] | (c[..., 1] << 4)).reshape(n, k // 2).contiguous()


def unpack_codes(packed):
    """the inverse of pack_codes: uint8 (N, K / 2) in stored order -> uint8 (N, K) in k order, one code per byte"""
    if packed.dtype != torch.uint8 or packed.dim() != 2 or packed.shape[1] % 32 != 0:
        raise ValueError(f"unpack_codes: expected uint8 (N, K / 2) with K a multiple of 64, got {packed.dtype} {tuple(packed.shape)}")
    n, kh = packed.shape
    c = torch.stack((packed & 15, packed >> 4), dim=-1)                           # (n, K / 2, j & 1)
    return c.reshape(n, kh // 32, 4, 2, 4, 2).permute(0, 1, 3, 2, 4, 5).reshape(n, 2 * kh).contiguous()


def _pow2(e):
    """2^e as float64 from its bits, e an int64 tensor in [-1022, 1023]"""
    return ((e.long() + 1023) << 52).view(torch.float64)


def _quantize_rows(w):
    xd = w.double().reshape(w.shape[0], -1, 32)
    amax = xd.abs().amax(dim=-1)
    m, E = torch.frexp(amax)                                                      # amax = m 2^E, 0.5 <= m < 1 (0 -> (0, 0)); 6 = 0.75 * 2^3
    e = torch.where(m <= 0.75, E - 3, E - 2)
    e = torch.where(amax == 0, torch.full_like(e, E_MIN), e).clamp_(min=E_MIN)
    scaled = xd * _pow2(-e).unsqueeze(-1)                                         # exact: |scaled| <= 6
    a = scaled.abs()
    # round to nearest on the grid, a tie to the even code: > at the midpoints below an even code, >= at those below an odd one's upper neighbour
    code = ((a > 0.25).to(torch.uint8) + (a >= 0.75).to(torch.uint8) + (a > 1.25).to(torch.uint8) + (a >= 1.75).to(torch.uint8)
            + (a > 2.5).to(torch.uint8) + (a >= 3.5).to(torch.uint8) + (a > 5.0).to(torch.uint8))
    code = code | (((scaled < 0) & (code != 0)).to(torch.uint8) << 3)
    return code.reshape(w.shape), (e + 127).to(torch.uint8)


def quantize_weight(w):
    """W (N, K) bf16 -> (codes uint8 (N, K / 2) in stored order, scales uint8 (N, K / 32))"""
    if w.dtype != torch.bfloat16 or w.dim() != 2 or w.shape[1] % 64 != 0:
        raise ValueError(f"quantize_weight: expected bf16 (N, K) with K a multiple of 64, got {w.dtype} {tuple(w.shape)}")
    n, k = w.shape
    codes = torch.empty((n, k // 2), dtype=torch.uint8, device=w.device)
    scales = torch.empty((n, k // 32), dtype=torch.uint8, device=w.device)
    for r in range(0, n, ROW_CHUNK):
        c, s = _quantize_rows(w[r:r + ROW_CHUNK].detach())
        codes[r:r + ROW_CHUNK] = pack_codes(c)
        scales[r:r + ROW_CHUNK] = s
    return codes, scales


def dequantize_weight(codes, scales):
    """codes uint8 (N, K / 2) in stored order, scales uint8 (N, K / 32) -> bf16 (N, K): value(code) * 2^(scale - 127), exactly (2
    significant bits, and for the bytes 2 .. 253 an exponent inside bf16's normal range), the code 0x8 giving -0.  The corners: a block
    whose maximum lies in the upper quarter of bf16's top binade, at or above 1.75 * 2^127 (bf16's largest values), has the code of 4
    under the scale 2^126, and 2^128 is +inf (any block under that scale with a code of 4 or 6 is); a block clamped at e = -125 — maximum
    at most 1.5 * 2^-124 — keeps values down to 2^-126 on the grid of 2^-126, loses what lies below half of that, and the amax / 3
    statement does not hold for it.  The scale byte 255 gives NaN, as e8m0 says; 0 and 1 give the subnormals bf16 has for them."""
    if codes.dtype != torch.uint8 or codes.dim() != 2 or codes.shape[1] % 32 != 0:
        raise ValueError(f"dequantize_weight: expected codes uint8 (N, K / 2) with K a multiple of 64, got {codes.dtype} {tuple(codes.shape)}")
    n, kh = codes.shape
    if scales.dtype != torch.uint8 or scales.shape != (n, kh // 16):
        raise ValueError(f"dequantize_weight: scales must be uint8 ({n}, {kh // 16}), got {scales.dtype} {tuple(scales.shape)}")
    table = torch.tensor(MAGNITUDES + tuple(-m for m in MAGNITUDES), dtype=torch.float64, device=codes.device)
    out = torch.empty((n, 2 * kh), dtype=torch.bfloat16, device=codes.device)
    for r in range(0, n, ROW_CHUNK):
        c = unpack_codes(codes[r:r + ROW_CHUNK])
        s = scales[r:r + ROW_CHUNK].long()
        scale = torch.where(s == 255, torch.full(s.shape, float("nan"), dtype=torch.float64, device=s.device), _pow2(s.clamp(max=254) - 127))
        v = table[c.long()].reshape(c.shape[0], -1, 32) * scale.unsqueeze(-1)
        out[r:r + ROW_CHUNK] = v.reshape(c.shape).to(torch.bfloat16)
    return out
