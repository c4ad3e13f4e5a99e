"""The e4m3 key/value cache's format in plain torch (include/omnibiote_hip_kv8.h): the tests' yardstick for csrc/attention_decode.hip's e4m3 format, as
sampling.py is for the sampler.  Nothing here runs on a generation path.

A head vector x of hs bf16 values is stored as hs codes and one fp32 scale:

    amax   = max |x_i|
    e      = the smallest integer >= -126 with amax * 2^-e <= 448          (a zero vector: -126)
             in bits: amax = m * 2^E with 0.5 <= m < 1, then e = E - 9 if m <= 0.875 else E - 8
    scale  = 2^e
    code_i = RNE_e4m3(x_i * 2^-e)                                         (OCP e4m3fn: torch.float8_e4m3fn)

The product is exact in fp32 wherever its value can matter (what underflows fp32 lies far below half of e4m3's smallest subnormal and
rounds to zero either way), so the conversion is the only rounding: the cache is a pure function of the bf16 inputs, no code is a NaN and
nothing saturates.  Inputs are finite by contract.  ``float(code) * scale`` reads a value back, exactly in fp32.

One layer's cache, in this order: K codes uint8 [B, H, T_max, hs], V codes, K scales fp32 [B, H, T_max], V scales."""
from __future__ import annotations

import torch


def cache_bytes(B, T_max, H, hs) -> int:
    """obte_kv8_cache_bytes for a supported shape"""
    return 2 * B * H * T_max * (hs + 4)


def quantize_reference(x):
    """x (..., hs) bf16 -> (codes uint8 (..., hs), scales fp32 (...)), each vector along the last dimension on its own.  Any device;
    the arithmetic is float64, where every step but the final conversion is exact."""
    if x.dtype != torch.bfloat16:
        raise ValueError(f"quantize_reference: expected bf16, got {x.dtype}")
    xd = x.double()
    amax = xd.abs().amax(dim=-1)
    m, E = torch.frexp(amax)                                            # amax = m 2^E, 0.5 <= m < 1 (0 -> (0, 0))
    e = torch.where(m <= 0.875, E - 9, E - 8)
    e = torch.where(amax == 0, torch.full_like(e, -126), e).clamp_(min=-126)
    scaled = xd * _pow2(-e).unsqueeze(-1)                               # exact: |scaled| <= 448
    codes = scaled.float().to(torch.float8_e4m3fn).view(torch.uint8)
    return codes, _pow2(e).float()


def _pow2(e):
    """2^e as float64 from its bits, e an int64 tensor in [-1022, 1023]"""
    return ((e.long() + 1023) << 52).view(torch.float64)


def dequantize_reference(codes, scales):
    """codes uint8 (..., hs), scales fp32 (...) -> fp32 (..., hs): float(code) * scale.  Exact, with one corner: a vector whose maximum
    lies within 1/16 of bf16's largest value has the code 256 under the scale 2^120, and 2^128 is +inf in fp32."""
    return codes.view(torch.float8_e4m3fn).float() * scales.unsqueeze(-1)


def split_cache(cache, B, T_max, H, hs):
    """The four parts of one layer's flat uint8 cache as views: (K codes, V codes) uint8 [B, H, T_max, hs], (K scales, V scales) fp32
    [B, H, T_max]"""
    n = B * H * T_max
    flat = cache.view(torch.uint8).reshape(-1)
    if flat.numel() != cache_bytes(B, T_max, H, hs):
        raise ValueError(f"split_cache: {flat.numel()} bytes, expected {cache_bytes(B, T_max, H, hs)}")
    kc, vc = flat[:n * hs].view(B, H, T_max, hs), flat[n * hs:2 * n * hs].view(B, H, T_max, hs)
    sc = flat[2 * n * hs:].view(torch.float32)
    return kc, vc, sc[:n].view(B, H, T_max), sc[n:].view(B, H, T_max)
