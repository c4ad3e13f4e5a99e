"""Tensor-level wrappers over the C ABI (include/omnibiote_hip.h).

Each function validates shapes/dtypes/devices on the host (the kernels assume them), borrows raw device
pointers from PyTorch-owned tensors for the duration of the call, and enqueues on PyTorch's *current* HIP
stream.  Nothing here synchronises the host.  PyTorch is plumbing only: allocation, streams, autograd glue.
"""
from __future__ import annotations

import contextlib
import ctypes as C
import os
from typing import NamedTuple, Optional, Tuple, Union

import torch

from . import _lib as L

bf16 = torch.bfloat16


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _need(t: torch.Tensor, name: str, dtype=bf16, contiguous: bool = True) -> None:
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name}: expected a tensor")
    if not t.is_cuda:
        raise RuntimeError(f"{name}: the OmniBioTE HIP path runs on MI355X only; got a {t.device} tensor "
                           "(there is no CPU fallback)")
    if dtype is not None and t.dtype != dtype:
        raise RuntimeError(f"{name}: expected dtype {dtype}, got {t.dtype}")
    if contiguous and not t.is_contiguous():
        raise RuntimeError(f"{name}: expected a contiguous tensor")


def _ptr(t: Optional[torch.Tensor]):
    return None if t is None else t.data_ptr()


# ---------------------------------------------------------------------------------------------------- LayerNorm
def layernorm_fwd(x: torch.Tensor, w: torch.Tensor, eps: float = 1e-5):
    _need(x, "x"); _need(w, "weight")
    cols = x.shape[-1]
    rows = x.numel() // cols
    assert w.numel() == cols
    y = torch.empty_like(x)
    mean = torch.empty(rows, dtype=torch.float32, device=x.device)
    rstd = torch.empty(rows, dtype=torch.float32, device=x.device)
    L.check(L.lib().obte_layernorm_fwd(_ptr(x), _ptr(w), _ptr(y), _ptr(mean), _ptr(rstd), rows, cols, eps, _stream()),
            "obte_layernorm_fwd")
    return y, mean, rstd


def ln_partials_buffer(cols: int, device) -> torch.Tensor:
    """A persistent fp32 partial-sum buffer for obte_layernorm_bwd_partial (one per LayerNorm weight)."""
    return torch.empty(L.lib().obte_layernorm_bwd_ws_rows() * cols, dtype=torch.float32, device=device)


def layernorm_bwd(dy, x, w, mean, rstd, dresid=None, accumulate_into=None, partials=None, partial_mode=0, dropout=None):
    """accumulate_into: an existing bf16 weight gradient to add into in place (then the returned dw is None).
    partials + partial_mode (L.LN_PARTIAL_*): accumulate the weight gradient over calls in the caller's fp32 buffer; dw is
    returned only by LN_PARTIAL_LAST (None otherwise).
    dropout=(p, seed, site): also return dropout(dx) under that mask as a third value (obte_layernorm_bwd_dropout)."""
    _need(dy, "dy"); _need(x, "x"); _need(w, "weight")
    _need(mean, "mean", torch.float32); _need(rstd, "rstd", torch.float32)
    cols = x.shape[-1]
    rows = x.numel() // cols
    assert dy.shape == x.shape and mean.numel() == rows and rstd.numel() == rows
    if dresid is not None:
        _need(dresid, "dresid"); assert dresid.shape == x.shape
    dx = torch.empty_like(x)
    if dropout is not None:
        dp, dseed, dsite = dropout
        dxd = torch.empty_like(x)
        if partial_mode:
            _need(partials, "partials", torch.float32)
            assert accumulate_into is None and partials.numel() == L.lib().obte_layernorm_bwd_ws_rows() * cols
            dw = torch.empty_like(w) if partial_mode == L.LN_PARTIAL_LAST else None
            buf = partials
        else:
            dw = accumulate_into if accumulate_into is not None else torch.empty_like(w)
            buf = torch.empty(L.lib().obte_layernorm_bwd_ws_rows() * cols, dtype=torch.float32, device=x.device)
        L.check(L.lib().obte_layernorm_bwd_dropout(_ptr(dy), _ptr(x), _ptr(w), _ptr(mean), _ptr(rstd), _ptr(dresid), _ptr(dx), _ptr(dxd), _ptr(dw),
                                                    _ptr(buf), rows, cols, int(partial_mode), int(accumulate_into is not None), float(dp), int(dseed),
                                                    int(dsite), _stream()), "obte_layernorm_bwd_dropout")
        return dx, (None if (accumulate_into is not None and not partial_mode) else dw), dxd
    if partial_mode:
        _need(partials, "partials", torch.float32)
        assert accumulate_into is None and partials.numel() == L.lib().obte_layernorm_bwd_ws_rows() * cols
        dw = torch.empty_like(w) if partial_mode == L.LN_PARTIAL_LAST else None
        L.check(L.lib().obte_layernorm_bwd_partial(_ptr(dy), _ptr(x), _ptr(w), _ptr(mean), _ptr(rstd), _ptr(dresid), _ptr(dx), _ptr(dw),
                                                    _ptr(partials), rows, cols, int(partial_mode), _stream()), "obte_layernorm_bwd_partial")
        return dx, dw
    if accumulate_into is not None:
        _need(accumulate_into, "grad"); assert accumulate_into.shape == w.shape
    dw = accumulate_into if accumulate_into is not None else torch.empty_like(w)
    ws = torch.empty(L.lib().obte_layernorm_bwd_ws_rows() * cols, dtype=torch.float32, device=x.device)
    L.check(L.lib().obte_layernorm_bwd_acc(_ptr(dy), _ptr(x), _ptr(w), _ptr(mean), _ptr(rstd), _ptr(dresid), _ptr(dx),
                                            _ptr(dw), _ptr(ws), rows, cols, int(accumulate_into is not None), _stream()),
            "obte_layernorm_bwd")
    return dx, (None if accumulate_into is not None else dw)


# --------------------------------------------------------------------------------------------------------- GEMM
def _check_acc32(acc32, acc32_mode, shape, name="acc32"):
    """The fp32 buffer of a gradient summed over the passes of a step (L.ACC32_*): the gradient's shape, persistent, caller-owned."""
    if acc32_mode not in (L.ACC32_FIRST, L.ACC32_MORE, L.ACC32_LAST):
        raise ValueError(f"acc32_mode must be L.ACC32_FIRST, _MORE or _LAST with an acc32 buffer, got {acc32_mode}")
    _need(acc32, name, torch.float32)
    if tuple(acc32.shape) != tuple(shape):
        raise RuntimeError(f"{name}: expected the gradient's shape {tuple(shape)}, got {tuple(acc32.shape)}")


def acc32_add_(acc32, src, mode, out=None):
    """acc32 (+)= src by mode (L.ACC32_*; FIRST: acc32 = src); src None: a zero contribution.  LAST returns bf16(acc32) (in
    ``out`` when given), the others None.  The unfused form of the fp32 gradient sum (obte_acc32_add_bf16): for a gradient
    the fused epilogues cannot take, and the flush of a weight whose backward node did not run in a pass."""
    _check_acc32(acc32, mode, acc32.shape)
    n = acc32.numel()
    if src is not None:
        _need(src, "src"); assert src.numel() == n
    if mode == L.ACC32_LAST:
        out = torch.empty(acc32.shape, dtype=bf16, device=acc32.device) if out is None else out
        _need(out, "out"); assert out.numel() == n
    else:
        out = None
    L.check(L.lib().obte_acc32_add_bf16(_ptr(acc32), _ptr(src), _ptr(out), n, int(mode), _stream()), "obte_acc32_add_bf16")
    return out


def gemm(a, b, M, N, K, a_kmajor=True, b_kmajor=True, epilogue=L.EPI_NONE, aux=None, alpha=1.0, out=None, dropout=None,
         rope=None, acc32=None, acc32_mode=0):
    """D[M,N] = epilogue(alpha * sum_k A(m,k) B(n,k)); see include/omnibiote_hip.h.  Returns d, or (d, d2) for
    the GELU epilogue (EPI_GELU_ACT: d alone, the activation).  EPI_ACC32 (acc32 fp32 [M,N] + acc32_mode): d is formed by L.ACC32_LAST only, else None is returned."""
    _need(a, "a"); _need(b, "b")
    lda = K if a_kmajor else M
    ldb = K if b_kmajor else N
    assert a.numel() == M * K, (a.shape, M, K)
    assert b.numel() == N * K, (b.shape, N, K)
    if epilogue == L.EPI_ACC32:
        _check_acc32(acc32, acc32_mode, (M, N))
        assert not a_kmajor and not b_kmajor, "EPI_ACC32: the weight-gradient layout only"
        if acc32_mode != L.ACC32_LAST:
            g = L.GemmArgs(_ptr(a), _ptr(b), None, None, None, M, N, K, lda, ldb, N, 0, 0, epilogue, float(alpha), 0.0, 0, 0)
            g.acc32, g.acc32_mode = _ptr(acc32), int(acc32_mode)
            _gemm_launch(g, M, N, K, True, a.device)
            return None
    else:
        assert acc32 is None and not acc32_mode, "acc32 / acc32_mode go with EPI_ACC32"
    d = out if out is not None else torch.empty((M, N), dtype=bf16, device=a.device)
    _need(d, "d"); assert d.numel() == M * N
    d2 = None
    if epilogue == L.EPI_GELU:
        d2 = torch.empty((M, N), dtype=bf16, device=a.device)
    if epilogue == L.EPI_GELU_ACT:
        assert a_kmajor and b_kmajor, "EPI_GELU_ACT: the x W^T layout only"
    if epilogue in (L.EPI_ADD, L.EPI_GELU_BWD, L.EPI_ADD_DROPOUT):
        _need(aux, "aux"); assert aux.numel() == M * N
    dp, dseed, dsite = dropout if dropout is not None else (0.0, 0, 0)   # (p, seed, site) for EPI_ADD_DROPOUT
    g = L.GemmArgs(_ptr(a), _ptr(b), _ptr(d), _ptr(aux), _ptr(d2), M, N, K, lda, ldb, N,
                   int(a_kmajor), int(b_kmajor), epilogue, float(alpha), float(dp), int(dsite), int(dseed))
    if epilogue == L.EPI_ROPE_QK:   # rope = (cos, sin, T, head_dim)
        cos, sin, rT, rhs = rope
        _need(cos, "cos", torch.float32); _need(sin, "sin", torch.float32)
        assert cos.shape[0] >= rT and cos.shape[-1] == rhs // 2
        g.rope_cos, g.rope_sin, g.rope_T, g.rope_head_dim = _ptr(cos), _ptr(sin), rT, rhs
    if epilogue == L.EPI_ACC32:
        g.acc32, g.acc32_mode = _ptr(acc32), int(acc32_mode)
    _gemm_launch(g, M, N, K, epilogue in (L.EPI_NONE, L.EPI_ADD, L.EPI_ACC32), a.device)
    return (d, d2) if d2 is not None else d


def _gemm_launch(g, M, N, K, may_split, device):
    ws_bytes = int(L.lib().obte_gemm_workspace_bytes(M, N, K)) if (may_split and M * N <= (1 << 23)) else 0
    if ws_bytes > 0:
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=device)
        L.check(L.lib().obte_gemm_bf16_ws(C.byref(g), _ptr(ws), ws_bytes, _stream()), "obte_gemm_bf16_ws")
    else:
        L.check(L.lib().obte_gemm_bf16(C.byref(g), _stream()), "obte_gemm_bf16")


def gemm_grouped(problems):
    """Up to six GEMMs in a single launch (obte_gemm_grouped_bf16).  ``problems`` is a list of dicts with keys
    a, b, M, N, K, out and optionally a_kmajor / b_kmajor (default False: the weight-gradient layout) and accumulate
    (out += alpha A B in place) / alpha.  A problem in the weight-gradient layout may carry acc32 (fp32 [M,N]) + acc32_mode
    (L.ACC32_*) instead: summed into that buffer (EPI_ACC32), ``out`` needed and written by L.ACC32_LAST only (None otherwise).
    Put the problems with the longest K first.  Returns the outs."""
    assert 1 <= len(problems) <= 6
    arr = (L.GemmArgs * len(problems))()
    outs = []
    for i, q in enumerate(problems):
        a, b, M, N, K, out = q["a"], q["b"], q["M"], q["N"], q["K"], q.get("out")
        ak, bk, acc = bool(q.get("a_kmajor", False)), bool(q.get("b_kmajor", False)), bool(q.get("accumulate", False))
        acc32, mode = q.get("acc32"), int(q.get("acc32_mode", 0) or 0)
        _need(a, "a"); _need(b, "b")
        assert a.numel() == M * K and b.numel() == N * K
        epi = L.EPI_ADD if acc else L.EPI_NONE
        if acc32 is not None or mode:
            _check_acc32(acc32, mode, (M, N))
            assert not ak and not bk and not acc, "acc32: the weight-gradient layout, no bf16 accumulation"
            epi = L.EPI_ACC32
            if mode != L.ACC32_LAST:
                out = None
            elif out is None:
                out = torch.empty((M, N), dtype=bf16, device=a.device)
        if out is not None:
            _need(out, "out"); assert out.numel() == M * N
        else:
            assert epi == L.EPI_ACC32, "out is needed"
        arr[i] = L.GemmArgs(_ptr(a), _ptr(b), _ptr(out), _ptr(out) if acc else None, None, M, N, K,
                            K if ak else M, K if bk else N, N, int(ak), int(bk),
                            epi, float(q.get("alpha", 1.0)), 0.0, 0, 0)
        if epi == L.EPI_ACC32:
            arr[i].acc32, arr[i].acc32_mode = _ptr(acc32), mode
        outs.append(out)
    L.check(L.lib().obte_gemm_grouped_bf16(arr, len(problems), _stream()), "obte_gemm_grouped_bf16")
    return outs


def linear_fwd(x2d, w, epilogue=L.EPI_NONE, aux=None, alpha=1.0, dropout=None):
    """y = x W^T for x [M,K], W [N,K] (nn.Linear forward)."""
    M, K = x2d.shape
    N = w.shape[0]
    assert w.shape[1] == K
    return gemm(x2d, w, M, N, K, True, True, epilogue, aux, alpha, dropout=dropout)


def linear_small_m(x2d, w, epilogue=L.EPI_NONE, aux=None, alpha=1.0, rope=None, out=None):
    """y = epilogue(alpha * x W^T) for x [M, K] of 1 <= M <= 64 rows, W [N, K] (obte_linear_small_m_bf16): the weight-streaming kernel,
    which reads W once.  Epilogues EPI_NONE, EPI_ADD (aux [M, N], may be ``out``), EPI_GELU_ACT, EPI_ROPE_QK (rope = (cos, sin, T,
    head_dim)), in gemm()'s arithmetic.  x2d may be a row-strided view (stride 1 along K); so may ``out`` and ``aux``, with ONE row
    stride between them, a multiple of 8."""
    _need(x2d, "x", contiguous=False); _need(w, "w")
    M, K = x2d.shape
    N = w.shape[0]
    assert w.shape[1] == K and x2d.stride(1) == 1
    d = out if out is not None else torch.empty((M, N), dtype=bf16, device=x2d.device)
    _need(d, "out", contiguous=False); assert d.shape == (M, N) and d.stride(1) == 1
    if epilogue == L.EPI_ADD:
        _need(aux, "aux", contiguous=False); assert aux.shape == (M, N) and aux.stride(1) == 1 and (M == 1 or aux.stride(0) == d.stride(0))
    g = L.GemmArgs(_ptr(x2d), _ptr(w), _ptr(d), _ptr(aux), None, M, N, K, x2d.stride(0) if M > 1 else K, K, d.stride(0) if M > 1 else N,
                   1, 1, epilogue, float(alpha), 0.0, 0, 0)
    if epilogue == L.EPI_ROPE_QK:
        cos, sin, rT, rhs = rope
        _need(cos, "cos", torch.float32); _need(sin, "sin", torch.float32)
        assert cos.shape[0] >= rT and cos.shape[-1] == rhs // 2
        g.rope_cos, g.rope_sin, g.rope_T, g.rope_head_dim = _ptr(cos), _ptr(sin), rT, rhs
    L.check(L.lib().obte_linear_small_m_bf16(C.byref(g), _stream()), "obte_linear_small_m_bf16")
    return d


def linear_small_m_w8(x2d, codes, scales, epilogue=L.EPI_NONE, aux=None, alpha=1.0, rope=None, out=None):
    """linear_small_m with W as e4m3 codes uint8 [N, K] (in w8quant's stored order; a row-strided view with a stride that is a multiple
    of 16 is fine) and scales fp32 [N] (obte_linear_small_m_w8): bit for bit linear_small_m on ``w8quant.dequantize_weight(codes,
    scales)``, reading half the bytes.  The same epilogues, aux, alpha, rope and out."""
    _need(x2d, "x", contiguous=False); _need(codes, "codes", torch.uint8, contiguous=False); _need(scales, "scales", torch.float32)
    M, K = x2d.shape
    N = codes.shape[0]
    assert codes.dim() == 2 and codes.shape[1] == K and codes.stride(1) == 1 and scales.shape == (N,) and x2d.stride(1) == 1
    d = out if out is not None else torch.empty((M, N), dtype=bf16, device=x2d.device)
    _need(d, "out", contiguous=False); assert d.shape == (M, N) and d.stride(1) == 1
    if epilogue == L.EPI_ADD:
        _need(aux, "aux", contiguous=False); assert aux.shape == (M, N) and aux.stride(1) == 1 and (M == 1 or aux.stride(0) == d.stride(0))
    g = L.GemmArgs(_ptr(x2d), None, _ptr(d), _ptr(aux), None, M, N, K, x2d.stride(0) if M > 1 else K, K, d.stride(0) if M > 1 else N,
                   1, 1, epilogue, float(alpha), 0.0, 0, 0)
    if epilogue == L.EPI_ROPE_QK:
        cos, sin, rT, rhs = rope
        _need(cos, "cos", torch.float32); _need(sin, "sin", torch.float32)
        assert cos.shape[0] >= rT and cos.shape[-1] == rhs // 2
        g.rope_cos, g.rope_sin, g.rope_T, g.rope_head_dim = _ptr(cos), _ptr(sin), rT, rhs
    L.check(L.lib().obte_linear_small_m_w8(C.byref(g), _ptr(codes), codes.stride(0) if N > 1 else K, _ptr(scales), _stream()), "obte_linear_small_m_w8")
    return d


def linear_small_m_w4(x2d, codes, scales, epilogue=L.EPI_NONE, aux=None, alpha=1.0, rope=None, out=None):
    """linear_small_m with W as MXFP4: codes uint8 [N, K / 2] (in w4quant's stored order) and block scales uint8 [N, K / 32]
    (obte_linear_small_m_w4); either may be a row-strided view, the codes' stride a multiple of 8, the scales' even.  Bit for bit
    linear_small_m on ``w4quant.dequantize_weight(codes, scales)``, reading a quarter of the bytes and a sixteenth.  The same epilogues,
    aux, alpha, rope and out."""
    _need(x2d, "x", contiguous=False); _need(codes, "codes", torch.uint8, contiguous=False); _need(scales, "scales", torch.uint8, contiguous=False)
    M, K = x2d.shape
    N = codes.shape[0]
    assert K % 64 == 0 and codes.dim() == 2 and codes.shape[1] == K // 2 and codes.stride(1) == 1 and x2d.stride(1) == 1
    assert scales.dim() == 2 and scales.shape == (N, K // 32) and scales.stride(1) == 1
    d = out if out is not None else torch.empty((M, N), dtype=bf16, device=x2d.device)
    _need(d, "out", contiguous=False); assert d.shape == (M, N) and d.stride(1) == 1
    if epilogue == L.EPI_ADD:
        _need(aux, "aux", contiguous=False); assert aux.shape == (M, N) and aux.stride(1) == 1 and (M == 1 or aux.stride(0) == d.stride(0))
    g = L.GemmArgs(_ptr(x2d), None, _ptr(d), _ptr(aux), None, M, N, K, x2d.stride(0) if M > 1 else K, K, d.stride(0) if M > 1 else N,
                   1, 1, epilogue, float(alpha), 0.0, 0, 0)
    if epilogue == L.EPI_ROPE_QK:
        cos, sin, rT, rhs = rope
        _need(cos, "cos", torch.float32); _need(sin, "sin", torch.float32)
        assert cos.shape[0] >= rT and cos.shape[-1] == rhs // 2
        g.rope_cos, g.rope_sin, g.rope_T, g.rope_head_dim = _ptr(cos), _ptr(sin), rT, rhs
    L.check(L.lib().obte_linear_small_m_w4(C.byref(g), _ptr(codes), codes.stride(0) if N > 1 else K // 2, _ptr(scales), scales.stride(0) if N > 1 else K // 32,
                                           _stream()), "obte_linear_small_m_w4")
    return d


@contextlib.contextmanager
def small_m_max(m: int):
    """Within the block, decode steps and last-position readouts of at most ``m`` rows (0..64, 0: none) take the weight-streaming
    product (obte_small_m_max_set: process-wide); the previous value comes back on exit.  The default is 64, or 0 under OBTE_SMALL_M=0."""
    prev = L.lib().obte_small_m_max_set(int(m))
    L.check(min(prev, 0), "obte_small_m_max_set")
    try:
        yield
    finally:
        L.lib().obte_small_m_max_set(prev)


def pack_token_mask(mask):
    """bool (..., V) on the device -> uint8 (..., ceil(V / 8)) on the device: column i is bit i & 7 of byte i >> 3 (sampling.pack_token_mask:
    the ``allowed_packed`` of ``sample_logits`` and ``spec_verify``).  A few torch launches, once per mask — not part of a step."""
    _need(mask, "mask", torch.bool, contiguous=False)
    from .sampling import pack_token_mask as pack
    return pack(mask)


def _constraint(what, B, V, device, allowed, allowed_packed, hold_token, emitted, min_emitted):
    """The restriction of include/omnibiote_hip_constrain.h as the C call's five arguments ``(mask tensor or None, allowed_ld, hold_token,
    emitted or None, min_emitted)`` — None when no keyword was given: the caller takes the unrestricted symbol."""
    if allowed is None and allowed_packed is None and hold_token is None and emitted is None and min_emitted == 0:
        return None
    if allowed is not None and allowed_packed is not None:
        raise ValueError(f"{what}: allowed and allowed_packed are the same mask in two forms: give one")
    nb = (V + 7) // 8
    if allowed is not None:
        _need(allowed, "allowed", torch.bool, contiguous=False)
        if allowed.shape not in ((V,), (B, V)):
            raise ValueError(f"{what}: allowed must be bool ({V},) or ({B}, {V}), got {tuple(allowed.shape)}")
        allowed_packed = pack_token_mask(allowed)
    ld = 0
    if allowed_packed is not None:
        _need(allowed_packed, "allowed_packed", torch.uint8, contiguous=False)
        if allowed_packed.dim() not in (1, 2) or allowed_packed.shape[-1] < nb or (allowed_packed.dim() == 2 and allowed_packed.shape[0] != B):
            raise ValueError(f"{what}: allowed_packed must be uint8 (n,) or ({B}, n) with n >= ceil(V / 8) = {nb}, got {tuple(allowed_packed.shape)}")
        if allowed_packed.stride(-1) != 1 and allowed_packed.shape[-1] > 1:
            raise ValueError(f"{what}: allowed_packed must have stride 1 along the bytes of a mask")
        if allowed_packed.dim() == 2 and B > 1:
            ld = allowed_packed.stride(0)
            if ld < nb:
                raise ValueError(f"{what}: the rows of allowed_packed must lie at least ceil(V / 8) = {nb} bytes apart, got a stride of {ld}")
    if emitted is not None:
        _need(emitted, "emitted", torch.int32)
        if emitted.shape != (B,):
            raise ValueError(f"{what}: emitted must be int32 ({B},), got {tuple(emitted.shape)}")
    if isinstance(min_emitted, bool) or not isinstance(min_emitted, int) or not 0 <= min_emitted < 2 ** 31:
        raise ValueError(f"{what}: min_emitted must be an integer in [0, 2^31), got {min_emitted!r}")
    hold = -1 if hold_token is None else int(hold_token)
    if not -2 ** 63 <= hold < 2 ** 63:
        raise ValueError(f"{what}: hold_token must fit 64 bits, got {hold_token!r}")
    return allowed_packed, ld, hold, emitted, min_emitted


class Penalty(NamedTuple):
    """The ``penalty`` of ``sample_logits``: every row's history and the three numbers of include/omnibiote_hip_penalty.h.  ``prompt`` (B, Tp)
    and ``gen`` (B, S) int64 on the device (rows may be strided) or None; ``prompt_len`` / ``n_gen``: how many of a row's ids count — None
    (the whole width), a host integer in [0, width] (every row: the call's NULL forms) or (B,) int32 on the device, clamped to the width
    by the kernel.  S, or a host ``n_gen``, is at most 32767."""
    prompt: Optional[torch.Tensor] = None
    prompt_len: Union[None, int, torch.Tensor] = None
    gen: Optional[torch.Tensor] = None
    n_gen: Union[None, int, torch.Tensor] = None
    repetition: float = 1.0
    presence: float = 0.0
    frequency: float = 0.0


def _history(what, name, ids, n, B, most):
    """one list of a ``Penalty`` as the C call's ``(ids tensor or None, ld, counts tensor or None, n_all, bound)``"""
    if ids is None:
        if n is not None:
            raise ValueError(f"{what}: penalty.{name} is None, and its count is not")
        return None, 0, None, 0, 0
    _need(ids, f"penalty.{name}", torch.int64, contiguous=False)
    if ids.dim() != 2 or ids.shape[0] != B:
        raise ValueError(f"{what}: penalty.{name} must be int64 ({B}, n), got {tuple(ids.shape)}")
    width = ids.shape[1]
    if ids.stride(1) != 1 and width > 1:
        raise ValueError(f"{what}: penalty.{name} must have stride 1 along a row's ids")
    ld = ids.stride(0) if B > 1 else width
    if ld < width:
        raise ValueError(f"{what}: the rows of penalty.{name} must lie at least their width {width} apart, got a stride of {ld}")
    if isinstance(n, torch.Tensor):
        _need(n, f"the count of penalty.{name}", torch.int32)
        if n.shape != (B,):
            raise ValueError(f"{what}: the count of penalty.{name} must be int32 ({B},), got {tuple(n.shape)}")
        counts, n_all, bound = n, 0, width
    else:
        if n is not None and (isinstance(n, bool) or not isinstance(n, int) or not 0 <= n <= width):
            raise ValueError(f"{what}: the count of penalty.{name} must be None, an integer in [0, {width}] or an int32 ({B},) tensor, got {n!r}")
        counts, bound = None, width if n is None else n
        n_all = bound
    if bound > most:
        raise ValueError(f"{what}: penalty.{name} counts up to {bound} ids per row, more than the {most} the kernel takes")
    return (ids if bound > 0 else None), ld, counts, n_all, bound


def _penalty(what, B, penalty):
    """``penalty`` as the C call's arguments behind min_emitted — None for a penalty that changes nothing: the caller takes the symbol it
    took without one."""
    if penalty is None:
        return None
    if not isinstance(penalty, Penalty):
        raise TypeError(f"{what}: penalty must be an ops.Penalty, got {type(penalty).__name__}")
    from .sampling import penalty_numbers
    try:
        r, inv, pp, fp = penalty_numbers(penalty.repetition, penalty.presence, penalty.frequency)
    except ValueError as e:
        raise ValueError(f"{what}: penalty: {e}") from None
    prompt, prompt_ld, prompt_len, _, prompt_max = _history(what, "prompt", penalty.prompt, penalty.prompt_len, B, L.PENALTY_MAX_PROMPT)
    gen, gen_ld, n_gen, n_gen_all, gen_max = _history(what, "gen", penalty.gen, penalty.n_gen, B, L.PENALTY_MAX_GEN)
    if (r == 1.0 and pp == 0.0 and fp == 0.0) or (prompt_max == 0 and gen_max == 0):
        return None
    return (_ptr(prompt), prompt_ld, _ptr(prompt_len), prompt_max, _ptr(gen), gen_ld, _ptr(n_gen), n_gen_all, gen_max, r, inv, pp, fp)


def sample_logits(logits, u=None, temperature=1.0, top_k=None, top_p=None, return_kept=False, out=None, allowed=None, allowed_packed=None,
                  hold_token=None, emitted=None, min_emitted=0, penalty=None):
    """The next token of every row of ``logits`` (B, V) bf16, V <= 65536, in one launch (obte_sample_logits_bf16; the rule:
    include/omnibiote_hip_sample.h, restated in plain torch by sampling.sample_reference): temperature, top-k, top-p, softmax and the
    draw against ``u`` (B,) float32 uniforms.  ``u is None``, ``temperature == 0`` or ``top_k == 1``: the lowest index of the row maximum.
    logits may be a row-strided view: last-dimension stride 1, row stride a multiple of 8.  Returns (B,) int64 (``out`` when given: a
    caller's buffer that keeps its address from step to step), with ``return_kept`` also the size of every row's kept set, (B,) int32.

    The restriction (obte_sample_logits_constrained_bf16; the rule: include/omnibiote_hip_constrain.h, in plain torch
    sampling.constrain_reference): ``allowed`` bool (V,) or (B, V) — packed here, a few torch launches — or ``allowed_packed`` uint8
    (n,) or (B, n), n >= ceil(V / 8), as ``pack_token_mask`` makes it (any byte address; rows may be strided): a column whose bit is clear is
    treated as -inf.  ``hold_token`` is excluded too in every row with ``emitted[b] < min_emitted`` (``emitted`` (B,) int32 on the device,
    None: 0).  With none of the five given the call is the unrestricted one.

    ``penalty`` (an ``ops.Penalty``; obte_sample_logits_penalized_bf16; the rule: include/omnibiote_hip_penalty.h, in plain torch
    sampling.penalize_reference): the columns of every row's prompt and generated tokens are rewritten under the repetition, presence and
    frequency penalties as the row is loaded — bit for bit this call on ``penalize_reference(logits, ...)``, in the same single launch, the
    restriction applied to the rewritten row.  None, neutral numbers (1, 0, 0) or two empty lists: the call is the one above."""
    _need(logits, "logits", contiguous=False)
    if logits.dim() != 2 or logits.shape[0] < 1 or logits.shape[1] < 1:
        raise ValueError(f"sample_logits: logits must be (B, V) with B, V >= 1, got {tuple(logits.shape)}")
    B, V = logits.shape
    if logits.stride(1) != 1 and V > 1:
        raise RuntimeError("sample_logits: logits must have stride 1 along the vocabulary")
    ld = logits.stride(0) if B > 1 else (V + 7) // 8 * 8
    if u is not None:
        _need(u, "u", torch.float32)
        if u.shape != (B,):
            raise ValueError(f"sample_logits: u must be ({B},), got {tuple(u.shape)}")
    if top_k is not None and top_k < 1:
        raise ValueError(f"sample_logits: top_k must be at least 1, got {top_k}")
    token = torch.empty(B, dtype=torch.int64, device=logits.device) if out is None else out
    if out is not None:
        _need(out, "out", torch.int64)
        if out.shape != (B,):
            raise ValueError(f"sample_logits: out must be ({B},), got {tuple(out.shape)}")
    kept = torch.empty(B, dtype=torch.int32, device=logits.device) if return_kept else None
    con = _constraint("sample_logits", B, V, logits.device, allowed, allowed_packed, hold_token, emitted, min_emitted)
    pen = _penalty("sample_logits", B, penalty)
    if pen is not None:
        con = con if con is not None else (None, 0, -1, None, 0)
        L.check(L.lib().obte_sample_logits_penalized_bf16(_ptr(logits), ld, B, V, _ptr(u), float(temperature),
                                                          0 if top_k is None else min(int(top_k), 2 ** 31 - 1), 1.0 if top_p is None else float(top_p),
                                                          _ptr(con[0]), con[1], con[2], _ptr(con[3]), con[4], *pen, _ptr(token), _ptr(kept), _stream()),
                "obte_sample_logits_penalized_bf16")
        return (token, kept) if return_kept else token
    if con is not None:
        L.check(L.lib().obte_sample_logits_constrained_bf16(_ptr(logits), ld, B, V, _ptr(u), float(temperature),
                                                            0 if top_k is None else min(int(top_k), 2 ** 31 - 1), 1.0 if top_p is None else float(top_p),
                                                            _ptr(con[0]), con[1], con[2], _ptr(con[3]), con[4], _ptr(token), _ptr(kept), _stream()),
                "obte_sample_logits_constrained_bf16")
        return (token, kept) if return_kept else token
    L.check(L.lib().obte_sample_logits_bf16(_ptr(logits), ld, B, V, _ptr(u), float(temperature), 0 if top_k is None else min(int(top_k), 2 ** 31 - 1),
                                            1.0 if top_p is None else float(top_p), _ptr(token), _ptr(kept), _stream()), "obte_sample_logits_bf16")
    return (token, kept) if return_kept else token


def gen_advance(sampled, pos, count, out, n_new, token, wte, x, us=None, u=None, eos=None, commit=1):
    """A step's sampled tokens into the next step's inputs, in one launch and in place (obte_gen_advance; the rule:
    include/omnibiote_hip_loop.h, restated in plain torch by sampling.advance_reference).  ``sampled`` (B,) int64 is read; ``pos``, ``count``,
    ``n_new`` (B,) int32, ``out`` (B, S) int64, ``token`` (B,) int64, ``x`` (B, C) bf16 and, with the call's uniforms ``us`` (steps, B)
    float32, ``u`` (B,) float32 are updated: a running row (pos >= 0) moves on by ``commit`` (0 or 1), records its token in column
    count[b] of out while that column exists, parks itself on ``eos`` (None: no such token); every row's x becomes the embedding of
    its token and its u the next step's row of us.  Every argument keeps its address: the call is the same for every step."""
    _need(sampled, "sampled", torch.int64); _need(token, "token", torch.int64); _need(out, "out", torch.int64)
    _need(wte, "wte"); _need(x, "x")
    if sampled.dim() != 1 or sampled.shape[0] < 1:
        raise ValueError(f"gen_advance: sampled must be (B,) with B >= 1, got {tuple(sampled.shape)}")
    B = sampled.shape[0]
    for t, name in ((pos, "pos"), (count, "count"), (n_new, "n_new")):
        _need_rows(t, name, B)
    if token.shape != (B,) or out.dim() != 2 or out.shape[0] != B or out.shape[1] < 1:
        raise ValueError(f"gen_advance: token must be ({B},) and out ({B}, S >= 1), got {tuple(token.shape)} and {tuple(out.shape)}")
    if wte.dim() != 2 or x.shape != (B, wte.shape[1]):
        raise ValueError(f"gen_advance: wte must be (vocab, C) and x ({B}, C), got {tuple(wte.shape)} and {tuple(x.shape)}")
    if commit not in (0, 1):
        raise ValueError(f"gen_advance: commit must be 0 or 1, got {commit!r}")
    if us is not None:
        _need(us, "us", torch.float32); _need(u, "u", torch.float32)
        if us.dim() != 2 or us.shape[0] < 1 or us.shape[1] != B or u.shape != (B,):
            raise ValueError(f"gen_advance: us must be (steps >= 1, {B}) and u ({B},), got {tuple(us.shape)} and {tuple(u.shape)}")
    L.check(L.lib().obte_gen_advance(_ptr(sampled), _ptr(pos), _ptr(count), _ptr(out), out.shape[1], _ptr(n_new), _ptr(token), _ptr(wte), wte.shape[0],
                                     wte.shape[1], _ptr(x), _ptr(us), 0 if us is None else us.shape[0], _ptr(u) if us is not None else None,
                                     -1 if eos is None else int(eos), int(commit), B, _stream()), "obte_gen_advance")


def spec_verify(p, q, draft, u_accept=None, u_draw=None, temperature=1.0, top_k=None, top_p=None, allowed=None, allowed_packed=None, hold_token=None,
                emitted=None, min_emitted=0):
    """Speculative decoding's verification in two launches (obte_spec_verify_bf16; the rule: include/omnibiote_hip_spec.h, restated in
    plain torch by sampling.verify_reference).  ``p`` (B, k + 1, V) bf16: the target's logits behind the pending token and behind each of
    the k drafted tokens ``draft`` (B, k) int64; ``q`` (B, k, V) bf16: the logits the draft drew them from; ``u_accept`` (B, k) and
    ``u_draw`` (B,) float32 uniforms.  1 <= k <= 31, V <= 65536.  Without uniforms, with ``temperature == 0`` or ``top_k == 1`` the call is
    greedy — a drafted token stands while it is the lowest index of the target row's maximum — and ``q`` may be None.  p and q may be
    row-strided views: last-dimension stride 1, row stride a multiple of 8, rows evenly spaced.  Returns ``(n_accept (B,) int32, token
    (B,) int64)``: how many drafted tokens stand and the token behind them.

    ``allowed`` / ``allowed_packed`` / ``hold_token`` / ``emitted`` / ``min_emitted`` as in ``sample_logits``, one mask row per batch row
    (obte_spec_verify_constrained_bf16): the restriction applies to p[b, j] and q[b, j] alike, the hold while ``emitted[b] + j <
    min_emitted`` at drafted position j, and a drafted token that is excluded never stands.  With none given: the unrestricted call."""
    _need(p, "p", contiguous=False)
    if p.dim() != 3 or p.shape[0] < 1 or p.shape[1] < 2 or p.shape[2] < 1:
        raise ValueError(f"spec_verify: p must be (B, k + 1, V) with B, k, V >= 1, got {tuple(p.shape)}")
    B, k, V = p.shape[0], p.shape[1] - 1, p.shape[2]

    def row_stride(t, rows, name):
        if t.stride(2) != 1 and V > 1:
            raise RuntimeError(f"spec_verify: {name} must have stride 1 along the vocabulary")
        ld = t.stride(1) if rows > 1 else t.stride(0)
        if B > 1 and rows > 1 and t.stride(0) != rows * ld:
            raise RuntimeError(f"spec_verify: the rows of {name} must be evenly spaced (stride(0) == {rows} * stride(1))")
        return ld if B * rows > 1 else (V + 7) // 8 * 8

    ld_p = row_stride(p, k + 1, "p")
    ld_q = 0
    if q is not None:
        _need(q, "q", contiguous=False)
        if q.shape != (B, k, V):
            raise ValueError(f"spec_verify: q must be ({B}, {k}, {V}), got {tuple(q.shape)}")
        ld_q = row_stride(q, k, "q")
    _need(draft, "draft", torch.int64)
    if draft.shape != (B, k):
        raise ValueError(f"spec_verify: draft must be ({B}, {k}), got {tuple(draft.shape)}")
    if (u_accept is None) != (u_draw is None):
        raise ValueError("spec_verify: u_accept and u_draw come together (both None: greedy)")
    if u_accept is not None:
        _need(u_accept, "u_accept", torch.float32); _need(u_draw, "u_draw", torch.float32)
        if u_accept.shape != (B, k) or u_draw.shape != (B,):
            raise ValueError(f"spec_verify: u_accept must be ({B}, {k}) and u_draw ({B},), got {tuple(u_accept.shape)} and {tuple(u_draw.shape)}")
    if top_k is not None and top_k < 1:
        raise ValueError(f"spec_verify: top_k must be at least 1, got {top_k}")
    if q is None and not (u_accept is None or temperature == 0 or top_k == 1):
        raise ValueError("spec_verify: q is None: only a greedy call goes without the draft's logits")
    n_accept = torch.empty(B, dtype=torch.int32, device=p.device)
    token = torch.empty(B, dtype=torch.int64, device=p.device)
    ws_bytes = max(int(L.lib().obte_spec_verify_ws_bytes(B, min(k, L.SPEC_VERIFY_MAX_K))), 8)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=p.device)
    con = _constraint("spec_verify", B, V, p.device, allowed, allowed_packed, hold_token, emitted, min_emitted)
    if con is not None:
        L.check(L.lib().obte_spec_verify_constrained_bf16(_ptr(p), ld_p, _ptr(q), ld_q, _ptr(draft), B, k, V, _ptr(u_accept), _ptr(u_draw), float(temperature),
                                                          0 if top_k is None else min(int(top_k), 2 ** 31 - 1), 1.0 if top_p is None else float(top_p),
                                                          _ptr(con[0]), con[1], con[2], _ptr(con[3]), con[4], _ptr(n_accept), _ptr(token), _ptr(ws), ws_bytes,
                                                          _stream()), "obte_spec_verify_constrained_bf16")
        return n_accept, token
    L.check(L.lib().obte_spec_verify_bf16(_ptr(p), ld_p, _ptr(q), ld_q, _ptr(draft), B, k, V, _ptr(u_accept), _ptr(u_draw), float(temperature),
                                          0 if top_k is None else min(int(top_k), 2 ** 31 - 1), 1.0 if top_p is None else float(top_p),
                                          _ptr(n_accept), _ptr(token), _ptr(ws), ws_bytes, _stream()), "obte_spec_verify_bf16")
    return n_accept, token


def _ngram(what, ngram):
    """``ngram`` as (g_min, g_max), 1 <= g_min <= g_max <= 16, or a ValueError in ``what``'s name"""
    ok = isinstance(ngram, (tuple, list)) and len(ngram) == 2 and all(isinstance(g, int) and not isinstance(g, bool) for g in ngram)
    if not ok or not 1 <= ngram[0] <= ngram[1] <= L.LOOKUP_MAX_NGRAM:
        raise ValueError(f"{what}: ngram must be (g_min, g_max) integers with 1 <= g_min <= g_max <= {L.LOOKUP_MAX_NGRAM}, got {ngram!r}")
    return int(ngram[0]), int(ngram[1])


def lookup_draft(hist, lens, k, ngram=(1, 4), vocab=65536):
    """k drafted tokens per row from the row's own history, in one launch (obte_lookup_draft; the rule: include/omnibiote_hip_lookup.h,
    restated in a plain loop by sampling.lookup_reference).  ``hist`` (B, W) int64, W <= 8192, rows at least W apart with stride 1
    along a row; ``lens`` (B,) int32: row b's tokens are hist[b, :lens[b]].  The longest suffix of them of ``ngram`` = (g_min, g_max)
    tokens that occurs earlier in the row — the most recent occurrence among equals — is followed by the draft, continued periodically
    past the end of the history; without a match every drafted token repeats the last one.  Tokens outside [0, ``vocab``) match nothing;
    a row with lens outside [1, W] gets zeros.  1 <= k <= 31.  Returns ``(draft (B, k) int64, match_len (B,) int32)``."""
    _need(hist, "hist", torch.int64, contiguous=False); _need(lens, "lens", torch.int32)
    if hist.dim() != 2 or hist.shape[0] < 1 or hist.shape[1] < 1:
        raise ValueError(f"lookup_draft: hist must be (B, W) with B, W >= 1, got {tuple(hist.shape)}")
    B, W = hist.shape
    if W > L.LOOKUP_MAX_HISTORY:
        raise ValueError(f"lookup_draft: a history of {W} tokens per row exceeds the {L.LOOKUP_MAX_HISTORY} the kernel takes")
    if hist.stride(1) != 1 and W > 1:
        raise ValueError("lookup_draft: hist must have stride 1 along a row")
    if B > 1 and hist.stride(0) != W:
        raise ValueError(f"lookup_draft: the rows of hist must lie their width {W} apart, got a stride of {hist.stride(0)}")
    if lens.shape != (B,):
        raise ValueError(f"lookup_draft: lens must be ({B},), got {tuple(lens.shape)}")
    if isinstance(k, bool) or not isinstance(k, int) or not 1 <= k <= L.SPEC_VERIFY_MAX_K:
        raise ValueError(f"lookup_draft: k must lie in [1, {L.SPEC_VERIFY_MAX_K}], got {k!r}")
    g_min, g_max = _ngram("lookup_draft", ngram)
    if isinstance(vocab, bool) or not isinstance(vocab, int) or not 1 <= vocab <= 65536:
        raise ValueError(f"lookup_draft: vocab must lie in [1, 65536], got {vocab!r}")
    draft = torch.empty((B, k), dtype=torch.int64, device=hist.device)
    match_len = torch.empty(B, dtype=torch.int32, device=hist.device)
    L.check(L.lib().obte_lookup_draft(_ptr(hist), W, _ptr(lens), B, k, g_min, g_max, vocab, _ptr(draft), _ptr(match_len), _stream()), "obte_lookup_draft")
    return draft, match_len


def spec_verify_point(p, draft, u_accept=None, u_draw=None, temperature=1.0, top_k=None, top_p=None):
    """``spec_verify`` for drafted tokens that come without a distribution (obte_spec_verify_point_bf16; the rule:
    include/omnibiote_hip_lookup.h, in plain torch sampling.verify_point_reference): bit for bit ``spec_verify`` with the q that is 0 at
    ``draft[b, j]`` and -inf everywhere else, which is never built — x_j stands while ``u_accept[b, j] < P_j(x_j)``, and behind a
    rejection the token is drawn from P_a with x_a's weight removed.  ``p``, ``draft``, the uniforms and the returned ``(n_accept (B,) int32,
    token (B,) int64)`` as in ``spec_verify``; without uniforms, with ``temperature == 0`` or ``top_k == 1`` the call is greedy."""
    _need(p, "p", contiguous=False)
    if p.dim() != 3 or p.shape[0] < 1 or p.shape[1] < 2 or p.shape[2] < 1:
        raise ValueError(f"spec_verify_point: p must be (B, k + 1, V) with B, k, V >= 1, got {tuple(p.shape)}")
    B, k, V = p.shape[0], p.shape[1] - 1, p.shape[2]
    if p.stride(2) != 1 and V > 1:
        raise RuntimeError("spec_verify_point: p must have stride 1 along the vocabulary")
    ld_p = p.stride(1)
    if B > 1 and p.stride(0) != (k + 1) * ld_p:
        raise RuntimeError(f"spec_verify_point: the rows of p must be evenly spaced (stride(0) == {k + 1} * stride(1))")
    _need(draft, "draft", torch.int64)
    if draft.shape != (B, k):
        raise ValueError(f"spec_verify_point: draft must be ({B}, {k}), got {tuple(draft.shape)}")
    if (u_accept is None) != (u_draw is None):
        raise ValueError("spec_verify_point: u_accept and u_draw come together (both None: greedy)")
    if u_accept is not None:
        _need(u_accept, "u_accept", torch.float32); _need(u_draw, "u_draw", torch.float32)
        if u_accept.shape != (B, k) or u_draw.shape != (B,):
            raise ValueError(f"spec_verify_point: u_accept must be ({B}, {k}) and u_draw ({B},), got {tuple(u_accept.shape)} and {tuple(u_draw.shape)}")
    if top_k is not None and top_k < 1:
        raise ValueError(f"spec_verify_point: top_k must be at least 1, got {top_k}")
    n_accept = torch.empty(B, dtype=torch.int32, device=p.device)
    token = torch.empty(B, dtype=torch.int64, device=p.device)
    ws_bytes = max(int(L.lib().obte_spec_verify_point_ws_bytes(B, min(k, L.SPEC_VERIFY_MAX_K))), 8)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=p.device)
    L.check(L.lib().obte_spec_verify_point_bf16(_ptr(p), ld_p, _ptr(draft), B, k, V, _ptr(u_accept), _ptr(u_draw), float(temperature),
                                                0 if top_k is None else min(int(top_k), 2 ** 31 - 1), 1.0 if top_p is None else float(top_p),
                                                _ptr(n_accept), _ptr(token), _ptr(ws), ws_bytes, _stream()), "obte_spec_verify_point_bf16")
    return n_accept, token


def dropout(x, p, seed, site=L.SITE_USER, out=None):
    """out = dropout(x) with the library's counter-based mask: x is read as a matrix [numel / last dim, last dim] and
    element (row, col) decides (include/omnibiote_hip.h, dropout); x may alias out."""
    _need(x, "x")
    out = torch.empty_like(x) if out is None else out
    L.check(L.lib().obte_dropout_bf16(_ptr(x), _ptr(out), x.numel(), int(x.shape[-1]), float(p), int(seed), int(site), _stream()),
            "obte_dropout_bf16")
    return out


def linear_dgrad(dy2d, w, epilogue=L.EPI_NONE, aux=None, alpha=1.0):
    """dx = dy W for dy [M,N], W [N,K]."""
    M, N = dy2d.shape
    K = w.shape[1]
    assert w.shape[0] == N
    return gemm(dy2d, w, M, K, N, True, False, epilogue, aux, alpha)


def linear_wgrad(dy2d, x2d, alpha=1.0, accumulate_into=None, acc32=None, acc32_mode=0):
    """dW = dy^T x for dy [M,N], x [M,K] -> [N,K].  accumulate_into: add into this tensor in place (alpha must be 1).
    acc32 (fp32 [N,K]) + acc32_mode (L.ACC32_*): the contribution alpha dy^T x goes into that buffer before any rounding to
    bf16; returns None for FIRST / MORE and bf16(acc32), the total, for LAST."""
    M, N = dy2d.shape
    K = x2d.shape[1]
    assert x2d.shape[0] == M
    if acc32 is not None or acc32_mode:
        assert accumulate_into is None, "acc32 replaces accumulate_into"
        return gemm(dy2d, x2d, N, K, M, False, False, L.EPI_ACC32, None, alpha, acc32=acc32, acc32_mode=acc32_mode)
    if accumulate_into is not None:
        return gemm(dy2d, x2d, N, K, M, False, False, L.EPI_ADD, accumulate_into, alpha, out=accumulate_into)
    return gemm(dy2d, x2d, N, K, M, False, False, L.EPI_NONE, None, alpha)


def _tiles256(m, n):
    return ((m + 255) // 256) * ((n + 255) // 256)


def linear_bwd_pair_is_grouped(M, N, K) -> bool:
    """Whether linear_bwd (dy [M,N], x [M,K], W [N,K]) takes the single grouped launch.  Only on request (OBTE_GROUPED_LM=1):
    the readout's pair — an input gradient of few 256x256 tiles with a long K (= vocabulary) beside a weight gradient of many
    tiles with a short K (= rows) — was grouped by default in rounds 3-4, when the single launches had no good split-K plans;
    with the tuned plans the two launches are faster (round 5, masked rows 4 740-4 915: 1 030-1 080 us against 1 440-1 460 us
    grouped; the step with every pass grouped 108.3 ms, with none 105.9 ms), so the default is the two launches."""
    import os
    return os.environ.get("OBTE_GROUPED_LM", "") == "1" and M >= 128 and N >= 128


def linear_bwd(dy2d, x2d, w, alpha=1.0, accumulate_into=None, acc32=None, acc32_mode=0):
    """Both gradients of y = alpha x W^T: dx = alpha dy W, dW = alpha dy^T x (added into ``accumulate_into`` when given; summed
    into the fp32 buffer ``acc32`` by ``acc32_mode`` as in linear_wgrad: dW is then None for FIRST / MORE, the total for LAST).
    Returns (dx, dW or None).  One grouped launch when linear_bwd_pair_is_grouped, else the two single launches."""
    M, N = dy2d.shape
    K = x2d.shape[1]
    if not linear_bwd_pair_is_grouped(M, N, K):
        dx = linear_dgrad(dy2d, w, alpha=alpha)
        dw = linear_wgrad(dy2d, x2d, alpha=alpha, accumulate_into=accumulate_into, acc32=acc32, acc32_mode=acc32_mode)
        return dx, (None if accumulate_into is not None else dw)
    dx = torch.empty((M, K), dtype=bf16, device=dy2d.device)
    if acc32 is not None or acc32_mode:
        assert accumulate_into is None, "acc32 replaces accumulate_into"
        outs = gemm_grouped([dict(a=dy2d, b=w, M=M, N=K, K=N, out=dx, a_kmajor=True, alpha=alpha),
                             dict(a=dy2d, b=x2d, M=N, N=K, K=M, acc32=acc32, acc32_mode=acc32_mode, alpha=alpha)])
        return dx, outs[1]
    dw = accumulate_into if accumulate_into is not None else torch.empty((N, K), dtype=bf16, device=dy2d.device)
    gemm_grouped([dict(a=dy2d, b=w, M=M, N=K, K=N, out=dx, a_kmajor=True, alpha=alpha),
                  dict(a=dy2d, b=x2d, M=N, N=K, K=M, out=dw, accumulate=accumulate_into is not None, alpha=alpha)])
    return dx, (None if accumulate_into is not None else dw)


# --------------------------------------------------------------------------------------------------------- RoPE
def rope_qk_(qkv, cos, sin, B, T, H, hs, inverse=False):
    _need(qkv, "qkv"); _need(cos, "cos", torch.float32); _need(sin, "sin", torch.float32)
    assert qkv.numel() == B * T * 3 * H * hs
    assert cos.shape[-1] == hs // 2 and cos.shape[0] >= T and cos.shape == sin.shape
    L.check(L.lib().obte_rope_qk_inplace(_ptr(qkv), _ptr(cos), _ptr(sin), B, T, H, hs, int(inverse), _stream()),
            "obte_rope_qk_inplace")
    return qkv


# ---------------------------------------------------------------------------------------------------- attention
class MaskSpec:
    """How a mask reaches the kernels: per-query key ranges (int32 [B,T,2]) or a dense additive bf16 tensor
    (B, H|1, T, T), possibly an expand() view with stride-0 heads, last dim contiguous."""

    __slots__ = ("ranges", "dense", "sb", "sh", "sq", "qbounds", "exact")

    def __init__(self, ranges=None, dense=None, qbounds=None, exact=None):
        """With ``dense``: ``ranges`` / ``qbounds`` are the optional loop bounds of obte_mask_bounds (per query / per key);
        the dense values still decide every weight — unless ``exact`` (obte_mask_bounds' device flag) says the mask IS a
        range mask, in which case the range kernels serve it (include/omnibiote_hip.h, obte_mask_bounds).
        Without ``dense``: ``ranges`` is the mask, and ``qbounds`` the per-key table of an asymmetric one (a causal mask:
        masks.RangeMask.query_bounds); None: symmetric."""
        self.ranges, self.dense, self.qbounds, self.exact = ranges, dense, qbounds, exact
        self.sb = self.sh = self.sq = 0
        if dense is not None:
            self.sb, self.sh, self.sq = dense.stride(0), dense.stride(1), dense.stride(2)

    @staticmethod
    def dense_with_bounds(m):
        """A dense additive mask (B, H, T, T) plus the conservative bounds that let the kernels skip the key tiles every
        row masks out (one pass over the mask per model forward; shared by all layers)."""
        B, H, T, _ = m.shape
        kb = torch.empty((B, T, 2), dtype=torch.int32, device=m.device)
        qb = torch.empty((B, T, 2), dtype=torch.int32, device=m.device)
        scratch = torch.empty((B * T,), dtype=torch.uint8, device=m.device)
        exact = torch.empty((1,), dtype=torch.int32, device=m.device)
        counts = torch.empty((B * T,), dtype=torch.int32, device=m.device)
        L.check(L.lib().obte_mask_bounds(_ptr(m), m.stride(0), m.stride(1), m.stride(2), B, H, T, _ptr(kb), _ptr(qb), _ptr(scratch),
                                         _ptr(exact), _ptr(counts), _stream()), "obte_mask_bounds")
        return MaskSpec(ranges=kb, dense=m, qbounds=qb, exact=exact)

    @staticmethod
    def from_user(attn_mask, B, T, H, device):
        if attn_mask is None:
            return MaskSpec()
        if isinstance(attn_mask, MaskSpec):
            return attn_mask
        if hasattr(attn_mask, "key_ranges"):  # masks.RangeMask
            r = attn_mask.key_ranges
            _need(r, "key_ranges", torch.int32)
            if tuple(r.shape) != (B, T, 2):
                raise RuntimeError(f"key_ranges must be (B,T,2)=({B},{T},2), got {tuple(r.shape)}")
            qb = getattr(attn_mask, "query_bounds", None)
            if qb is not None:
                _need(qb, "query_bounds", torch.int32)
                if tuple(qb.shape) != (B, T, 2):
                    raise RuntimeError(f"query_bounds must be (B,T,2)=({B},{T},2), got {tuple(qb.shape)}")
            return MaskSpec(ranges=r, qbounds=qb)
        m = attn_mask
        if not isinstance(m, torch.Tensor):
            raise TypeError("attn_mask must be None, a tensor or a RangeMask")
        if m.dim() == 3:
            m = m.unsqueeze(1)
        if m.dim() != 4 or m.shape[0] != B or m.shape[2] != T or m.shape[3] != T or m.shape[1] not in (1, H):
            raise RuntimeError(f"attn_mask must be (B, n_head, T, T)=({B},{H},{T},{T}), got {tuple(attn_mask.shape)}")
        if not m.is_cuda:
            raise RuntimeError("attn_mask must be on the GPU")
        if m.dtype == torch.bool:
            raise RuntimeError("boolean masks are not part of the reference's contract; pass an additive float mask")
        if m.dtype != bf16 or m.stride(3) != 1:
            # convert without materialising H copies of an expand()ed mask
            if m.shape[1] == 1 or m.stride(1) == 0:
                m = m[:, :1].to(bf16).contiguous()
            else:
                m = m.to(bf16).contiguous()
        if m.shape[1] == 1:
            m = m.expand(B, H, T, T)
        return MaskSpec.dense_with_bounds(m)


def attn_fwd(qkv, B, T, H, hs, scale, mask: Optional[MaskSpec] = None, dropout_p=0.0, dropout_seed=0, keep_bits=False):
    """keep_bits (dropout only): also return the forward's keep decisions in key-major order (include/omnibiote_hip.h,
    obte_attn_fwd_args::drop_bits) for attn_bwd(drop_bits=...): (o, lse, bits)."""
    _need(qkv, "qkv"); assert qkv.numel() == B * T * 3 * H * hs
    mask = mask or MaskSpec()
    o = torch.empty((B, T, H * hs), dtype=bf16, device=qkv.device)
    lse = torch.empty((B, H, T), dtype=torch.float32, device=qkv.device)
    bits = None
    if keep_bits and dropout_p > 0.0:   # (zeroed: words of key tiles the forward skips stay defined; they belong to masked pairs)
        bits = torch.zeros(int(L.lib().obte_attn_drop_bits_bytes(B, T, H)) // 4, dtype=torch.int32, device=qkv.device)
    a = L.AttnFwdArgs(_ptr(qkv), _ptr(o), _ptr(lse), _ptr(mask.ranges), _ptr(mask.dense), mask.sb, mask.sh, mask.sq,
                      B, T, H, hs, float(scale), float(dropout_p), int(dropout_seed), _ptr(mask.exact), _ptr(bits))
    L.check(L.lib().obte_attn_fwd(C.byref(a), _stream()), "obte_attn_fwd")
    return (o, lse, bits) if keep_bits else (o, lse)


def attn_bwd(qkv, o, d_o, lse, B, T, H, hs, scale, mask: Optional[MaskSpec] = None, rope=None, dropout_p=0.0, dropout_seed=0,
             one_kernel: bool = True, drop_bits=None):
    """one_kernel: hand the library the scratch that lets it run the one-kernel backward where that form applies (head size
    128, no dense mask; with dropout: only from the forward's keep bits, drop_bits — include/omnibiote_hip.h,
    obte_attn_bwd_args::ws); False: the dQ + dK/dV kernel pair."""
    _need(qkv, "qkv"); _need(o, "o"); _need(d_o, "d_o"); _need(lse, "lse", torch.float32)
    mask = mask or MaskSpec()
    dqkv = torch.empty_like(qkv)
    delta = torch.empty((B, H, T), dtype=torch.float32, device=qkv.device)
    cos, sin = rope if rope is not None else (None, None)
    ws_bytes = int(L.lib().obte_attn_bwd_ws_bytes(B, T, H, hs)) if (one_kernel and (dropout_p == 0.0 or drop_bits is not None) and mask.dense is None) else 0
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=qkv.device) if ws_bytes > 0 else None
    a = L.AttnBwdArgs(_ptr(qkv), _ptr(o), _ptr(d_o), _ptr(lse), _ptr(delta), _ptr(dqkv), _ptr(cos), _ptr(sin),
                      _ptr(mask.ranges), _ptr(mask.dense), mask.sb, mask.sh, mask.sq, B, T, H, hs, float(scale),
                      float(dropout_p), int(dropout_seed), _ptr(mask.qbounds), _ptr(mask.exact), _ptr(ws), ws_bytes, _ptr(drop_bits))
    L.check(L.lib().obte_attn_bwd(C.byref(a), _stream()), "obte_attn_bwd")
    return dqkv


def attn_probs_workspace(B, T, H, device) -> torch.Tensor:
    """The (m, l) pairs of ``attn_probs``: 8 * B * H * T bytes, contents irrelevant before and after; one buffer serves every layer."""
    return torch.empty(int(L.lib().obte_attn_probs_ws_bytes(B, T, H)), dtype=torch.uint8, device=device)


def attn_probs(qkv, B, T, H, hs, scale, mask: Optional[MaskSpec] = None, heads="all", dtype=torch.float32, out=None, ws=None):
    """The softmax weights of the attention ``attn_fwd`` runs on the same operands (include/omnibiote_hip_probs.h; the rule:
    attnmaps.attention_probs_reference in fp32): (B, H, T, T), or (B, T, T) with ``heads="mean"`` — the heads' mean, summed in fp32
    in ascending order; fp32 or bf16 (the rounded fp32 value).  ``out``: a tensor of that shape and dtype whose dimensions after
    the first are contiguous; its batch stride may be larger than the payload (one layer's slice of a larger tensor), nothing
    between the batch rows is touched.  ``ws``: ``attn_probs_workspace(B, T, H, device)``."""
    if not isinstance(heads, str) or heads not in ("all", "mean"):
        raise ValueError(f"attn_probs: heads must be \"all\" or \"mean\", got {heads!r}")
    if dtype not in (torch.float32, bf16):
        raise ValueError(f"attn_probs: dtype must be torch.float32 or torch.bfloat16, got {dtype}")
    _need(qkv, "qkv"); assert qkv.numel() == B * T * 3 * H * hs
    mask = mask or MaskSpec()
    mean = heads == "mean"
    shape = (B, T, T) if mean else (B, H, T, T)
    if out is None:
        out = torch.empty(shape, dtype=dtype, device=qkv.device)
    _need(out, "out", dtype, contiguous=False)
    if tuple(out.shape) != shape or (B > 0 and not out[0].is_contiguous()):
        raise RuntimeError(f"attn_probs: out must be {shape} with every dimension after the first contiguous, got {tuple(out.shape)} "
                           f"with strides {out.stride()}")
    need = int(L.lib().obte_attn_probs_ws_bytes(B, T, H))
    if ws is None:
        ws = torch.empty(need, dtype=torch.uint8, device=qkv.device)
    _need(ws, "ws", torch.uint8)
    a = L.AttnProbsArgs(_ptr(qkv), _ptr(mask.ranges), _ptr(mask.dense), mask.sb, mask.sh, mask.sq, _ptr(mask.exact), B, T, H, hs, float(scale),
                        _ptr(out), out.stride(0) if B > 1 else out[0].numel(), int(dtype == bf16), int(mean), _ptr(ws), ws.numel())
    L.check(L.lib().obte_attn_probs(C.byref(a), _stream()), "obte_attn_probs")
    return out


# ---------------------------------------------------------------------------------------------------- embedding
def embedding_fwd(idx, wte, dropout_p=0.0, dropout_seed=0):
    _need(idx, "idx", torch.int64); _need(wte, "wte")
    V, Cc = wte.shape
    out = torch.empty(tuple(idx.shape) + (Cc,), dtype=bf16, device=wte.device)
    L.check(L.lib().obte_embedding_fwd_dropout(_ptr(idx), _ptr(wte), _ptr(out), idx.numel(), Cc, V, float(dropout_p),
                                                int(dropout_seed), _stream()), "obte_embedding_fwd")
    return out


def embedding_bwd(idx, dout, vocab, accumulate_into=None, dropout_p=0.0, dropout_seed=0, order=None, acc32=None, acc32_mode=0):
    """accumulate_into: an existing dense (vocab, C) gradient; the touched rows are updated in place
    (bf16(old + bf16(sum))), nothing else is read or written.  order: a stable argsort of idx.reshape(-1) as int32, if
    the caller has one already (the harness sorts a whole optimizer step's ids in one call).
    acc32 (fp32 (vocab, C)) + acc32_mode (L.ACC32_*): the rows' fp32 sums go into that buffer before any rounding (FIRST zeroes it
    first); returns None for FIRST / MORE and bf16(acc32) for LAST."""
    _need(idx, "idx", torch.int64); _need(dout, "dout")
    rows, Cc = idx.numel(), dout.shape[-1]
    if order is None:
        if prelude_hip():
            order = token_order(idx.reshape(1, -1), vocab).reshape(-1)
        else:
            order = torch.sort(idx.reshape(-1), stable=True).indices.to(torch.int32)
    else:
        _need(order, "order", torch.int32); assert order.numel() == rows
    ws = torch.empty(max(int(L.lib().obte_embedding_bwd_ws_bytes(rows, Cc)), 16), dtype=torch.uint8, device=dout.device)
    if acc32 is not None or acc32_mode:
        assert accumulate_into is None, "acc32 replaces accumulate_into"
        _check_acc32(acc32, acc32_mode, (vocab, Cc))
        dwte = torch.empty((vocab, Cc), dtype=bf16, device=dout.device) if acc32_mode == L.ACC32_LAST else None
        L.check(L.lib().obte_embedding_bwd_acc32(_ptr(idx), _ptr(order), _ptr(dout), _ptr(acc32), _ptr(dwte), _ptr(ws), rows, Cc, vocab,
                                                  int(acc32_mode), float(dropout_p), int(dropout_seed), _stream()), "obte_embedding_bwd_acc32")
        return dwte
    if accumulate_into is not None:
        _need(accumulate_into, "grad"); assert tuple(accumulate_into.shape) == (vocab, Cc)
        L.check(L.lib().obte_embedding_bwd_dropout(_ptr(idx), _ptr(order), _ptr(dout), _ptr(accumulate_into), _ptr(ws), rows, Cc,
                                                    vocab, 1, float(dropout_p), int(dropout_seed), _stream()), "obte_embedding_bwd")
        return None
    dwte = torch.empty((vocab, Cc), dtype=bf16, device=dout.device)
    L.check(L.lib().obte_embedding_bwd_dropout(_ptr(idx), _ptr(order), _ptr(dout), _ptr(dwte), _ptr(ws), rows, Cc, vocab, 0,
                                                float(dropout_p), int(dropout_seed), _stream()), "obte_embedding_bwd")
    return dwte


# ------------------------------------------------------------------------------------------------ step prelude
def prelude_hip() -> bool:
    """OBTE_PRELUDE_HIP=0: key ranges and the embedding sort order from tensor ops / torch.sort instead of the HIP entry
    points.  Both forms give the same integers."""
    return os.environ.get("OBTE_PRELUDE_HIP", "") != "0"


def key_ranges_from_tokens(ids, eos_token: int = 3, padding: bool = False, group: int = 0):
    """int32 (B, T, 2): the [k_start, k_end) of every query under the reference's document mask
    (masks.RangeMask.from_tokens is the tensor-op form of the same function)."""
    _need(ids, "ids", torch.int64)
    if ids.dim() != 2 or ids.numel() == 0:
        raise RuntimeError(f"ids: expected a non-empty (B, T) tensor, got {tuple(ids.shape)}")
    B, T = ids.shape
    out = torch.empty((B, T, 2), dtype=torch.int32, device=ids.device)
    L.check(L.lib().obte_key_ranges_from_tokens(_ptr(ids), B, T, int(eos_token), 1 if padding else 0, int(group), _ptr(out),
                                                _stream()), "obte_key_ranges_from_tokens")
    return out


def causal_bounds(doc_ranges=None, B: Optional[int] = None, T: Optional[int] = None, device=None):
    """(key_ranges, query_bounds), int32 (B, T, 2) each: the causal mask's pair of tables (obte_causal_bounds), under the symmetric
    range mask ``doc_ranges`` (int32 (B, T, 2), e.g. key_ranges_from_tokens' output) if one is given — then B, T and the device
    are its own.  masks.RangeMask.causal / from_tokens(causal=True) are the tensor-op form of the same function."""
    if doc_ranges is not None:
        _need(doc_ranges, "doc_ranges", torch.int32)
        if doc_ranges.dim() != 3 or doc_ranges.shape[-1] != 2 or doc_ranges.numel() == 0:
            raise RuntimeError(f"doc_ranges: expected a non-empty (B, T, 2) tensor, got {tuple(doc_ranges.shape)}")
        if (B is not None and B != doc_ranges.shape[0]) or (T is not None and T != doc_ranges.shape[1]):
            raise RuntimeError(f"doc_ranges {tuple(doc_ranges.shape)} does not match B {B}, T {T}")
        B, T, device = doc_ranges.shape[0], doc_ranges.shape[1], doc_ranges.device
    elif B is None or T is None or device is None or B <= 0 or T <= 0:
        raise RuntimeError("causal_bounds: without doc_ranges, B >= 1, T >= 1 and the device are needed")
    kr = torch.empty((B, T, 2), dtype=torch.int32, device=device)
    qb = torch.empty((B, T, 2), dtype=torch.int32, device=device)
    L.check(L.lib().obte_causal_bounds(_ptr(doc_ranges), B, T, _ptr(kr), _ptr(qb), _stream()), "obte_causal_bounds")
    return kr, qb


def token_order_workspace(segments: int, seg_len: int, vocab: int, device) -> torch.Tensor:
    nbytes = int(L.lib().obte_token_order_ws_bytes(segments, seg_len, vocab))
    if nbytes <= 0:
        raise RuntimeError(f"token_order: unsupported shape ({segments} x {seg_len} ids, vocab {vocab}): segments * seg_len "
                           "must be below 2^31 and vocab in 1 .. 2^17")
    return torch.empty(nbytes, dtype=torch.uint8, device=device)


def token_order(ids_2d, vocab: int, ws: Optional[torch.Tensor] = None):
    """int32 (segments, seg_len): row g is the stable argsort of ids_2d[g] — the ``order`` of embedding_bwd for that row.
    ws: a buffer from token_order_workspace for this shape, if the caller keeps one."""
    _need(ids_2d, "ids", torch.int64)
    if ids_2d.dim() != 2 or ids_2d.numel() == 0:
        raise RuntimeError(f"ids: expected a non-empty (segments, seg_len) tensor, got {tuple(ids_2d.shape)}")
    segments, seg_len = ids_2d.shape
    if ws is None:
        ws = token_order_workspace(segments, seg_len, vocab, ids_2d.device)
    else:
        _need(ws, "ws", torch.uint8)
        assert ws.numel() >= int(L.lib().obte_token_order_ws_bytes(segments, seg_len, vocab)) > 0
    order = torch.empty((segments, seg_len), dtype=torch.int32, device=ids_2d.device)
    L.check(L.lib().obte_token_order(_ptr(ids_2d), segments, seg_len, int(vocab), _ptr(order), _ptr(ws), _stream()),
            "obte_token_order")
    return order


# ---------------------------------------------------------------------------------------------- loss, optimizer
class DLogitsBuffer:
    """A gradient buffer reused across micro-batches by ``masked_ce``: only the rows whose masked-ness changed since
    the previous call are written (the other ~85 % already hold zeros).  The caller must be done with the previous
    contents (i.e. have run the backward that consumes them) before the next ``masked_ce`` on the same buffer — true for
    a training loop, where forward/loss/backward of one micro-batch are enqueued before the next begins."""

    def __init__(self):
        self.buf = None
        self.prev_mask = None

    def get(self, like: torch.Tensor):
        if self.buf is None or self.buf.shape != like.shape or self.buf.device != like.device:
            self.buf = torch.empty_like(like)
            self.prev_mask = None      # fresh memory: the next call writes every row
        return self.buf


def masked_ce(logits, targets, mlm_mask, n_accum: int, reuse: Optional[DLogitsBuffer] = None):
    """Returns (loss scalar fp32 tensor, dlogits bf16) with the reference's micro-batch normalisation
    (train_encoder.py:301-305): loss = sum_masked(CE)/n_accum / count."""
    _need(logits, "logits"); _need(targets, "targets", torch.int64)
    V = logits.shape[-1]
    rows = logits.numel() // V
    assert targets.numel() == rows and mlm_mask.numel() == rows
    m8 = mlm_mask.reshape(-1).to(torch.uint8).contiguous()
    inv_count = (1.0 / m8.sum(dtype=torch.float32)).reshape(1)
    row_loss = torch.empty(rows, dtype=torch.float32, device=logits.device)
    if reuse is None:
        dlogits, prev = torch.empty_like(logits), None
    else:
        dlogits, prev = reuse.get(logits), reuse.prev_mask
    L.check(L.lib().obte_masked_ce_fwd_bwd_reuse(_ptr(logits), _ptr(targets), _ptr(m8), _ptr(prev), _ptr(inv_count), 1.0 / n_accum,
                                                  _ptr(row_loss), _ptr(dlogits), rows, V, _stream()), "obte_masked_ce_fwd_bwd")
    if reuse is not None:
        reuse.prev_mask = m8
    loss = row_loss.sum() * inv_count[0]
    return loss, dlogits


def masked_ce_rows(logits, targets, rows, n_accum: int, row_weights: Optional[torch.Tensor] = None):
    """The same loss on a compact list of masked positions: ``rows`` int64 (n,) ascending row indices into the dense
    logits (viewed [M, V]) — or None when logits and targets already hold the listed rows alone ([n, V] and (n,): the
    readout that computes the masked rows only).  Returns (loss, dlogits_rows bf16 [n, V]) — the rows of d(logits) that are
    not exact zeros.
    row_weights (fp32 (n,), optional): replaces the 1/n normalisation by a weight per listed row — a call that covers
    several micro-batches passes 1 / (masked tokens of the row's own micro-batch)."""
    _need(logits, "logits"); _need(targets, "targets", torch.int64)
    V = logits.shape[-1]
    M = logits.numel() // V
    if rows is not None:
        _need(rows, "rows", torch.int64)
    n = rows.numel() if rows is not None else M
    assert targets.numel() == M and 0 < n <= M
    if row_weights is not None:
        _need(row_weights, "row_weights", torch.float32); assert row_weights.numel() == n
    # the 1 / n of the mean is known on the host here (the list's length): it travels in the by-value row scale, and the device-side
    # gradient scale is a constant 1 (a NULL grad_scale: no persistent [1.0] tensor whose fill another stream would have to be
    # ordered after) — no fill launch per call, and the loss is the plain sum of the row losses
    row_scale = (1.0 if row_weights is not None else 1.0 / n) / n_accum
    row_loss = torch.empty(n, dtype=torch.float32, device=logits.device)
    dl = torch.empty((n, V), dtype=bf16, device=logits.device)
    L.check(L.lib().obte_masked_ce_rows(_ptr(logits), _ptr(targets), _ptr(rows), None, row_scale, _ptr(row_weights),
                                        _ptr(row_loss), _ptr(dl), n, M, V, _stream()), "obte_masked_ce_rows")
    return row_loss.sum(), dl


def distill_ce_rows_per_row(logits, teacher_logits, targets, n_accum: int, row_weights: Optional[torch.Tensor] = None, alpha: float = 0.5,
                            temperature: float = 1.0):
    """obte_distill_ce_rows (include/omnibiote_hip_distill.h; the rule in float64: distill.distill_reference) on the compact form —
    logits and teacher_logits bf16 [n, V] hold the listed rows alone, targets int64 (n,).  Per row: the cross entropy against the
    label and KL(softmax(teacher / temperature) || softmax(student / temperature)); the loss mixes them as alpha CE + (1 - alpha)
    temperature^2 KL under masked_ce_rows' normalisation (1 / (n n_accum), or row_weights[r] / n_accum).
    Returns (row_loss fp32 (n,) weighted, dlogits bf16 [n, V], row_ce fp32 (n,), row_kl fp32 (n,); the last two unweighted)."""
    from .distill import distill_weights
    _need(logits, "logits"); _need(teacher_logits, "teacher_logits"); _need(targets, "targets", torch.int64)
    if logits.dim() != 2 or teacher_logits.shape != logits.shape or teacher_logits.device != logits.device:
        raise RuntimeError(f"distill_ce_rows: logits and teacher_logits must be [n, V] on one device, got {tuple(logits.shape)} and {tuple(teacher_logits.shape)}")
    n, V = logits.shape
    if targets.numel() != n or n == 0:
        raise RuntimeError(f"distill_ce_rows: {n} rows of logits, {targets.numel()} targets (at least one row is needed)")
    if row_weights is not None:
        _need(row_weights, "row_weights", torch.float32)
        if row_weights.numel() != n:
            raise RuntimeError(f"distill_ce_rows: {n} rows, {row_weights.numel()} row_weights")
    ce_weight, kl_weight, inv_t = distill_weights(alpha, temperature)
    row_scale = (1.0 if row_weights is not None else 1.0 / n) / n_accum
    out = torch.empty((3, n), dtype=torch.float32, device=logits.device)   # row_loss, row_ce, row_kl
    dl = torch.empty((n, V), dtype=bf16, device=logits.device)
    L.check(L.lib().obte_distill_ce_rows(_ptr(logits), _ptr(teacher_logits), _ptr(targets), row_scale, _ptr(row_weights), ce_weight, kl_weight, inv_t,
                                         _ptr(out[0]), _ptr(out[1]), _ptr(out[2]), _ptr(dl), n, V, _stream()), "obte_distill_ce_rows")
    return out[0], dl, out[1], out[2]


def distill_ce_rows(logits, teacher_logits, targets, n_accum: int, row_weights: Optional[torch.Tensor] = None, alpha: float = 0.5,
                    temperature: float = 1.0):
    """The distillation loss of a causal-LM step in the place of masked_ce_rows (compact form): (loss, dlogits bf16 [n, V], row_ce, row_kl)
    — loss the sum of the weighted row losses; see distill_ce_rows_per_row."""
    row_loss, dl, row_ce, row_kl = distill_ce_rows_per_row(logits, teacher_logits, targets, n_accum, row_weights, alpha, temperature)
    return row_loss.sum(), dl, row_ce, row_kl


class _NextTokenLossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, targets, rows):
        loss, dl = masked_ce_rows(logits, targets, rows, 1)
        ctx.save_for_backward(dl, rows)
        ctx.shape = logits.shape
        return loss

    @staticmethod
    def backward(ctx, dloss):
        dl, rows = ctx.saved_tensors
        V = ctx.shape[-1]
        d = torch.zeros(ctx.shape, dtype=dl.dtype, device=dl.device)
        d.view(-1, V).index_copy_(0, rows, dl * dloss.to(dl.dtype))
        return d, None, None


def next_token_loss(logits, idx):
    """Mean cross entropy of position t's logits against token t + 1, over the first T - 1 positions of every row: the loss of
    an autoregressive model (``OmniBioTAConfig.autoregressive``) on its own input.  logits bf16 (B, T, V), idx int64 (B, T),
    T >= 2.  obte_masked_ce_rows on the row list {b T + t : t < T - 1}; differentiable with respect to the logits."""
    _need(logits, "logits"); _need(idx, "idx", torch.int64)
    B, T = idx.shape
    if logits.dim() != 3 or tuple(logits.shape[:2]) != (B, T) or T < 2:
        raise RuntimeError(f"next_token_loss: logits (B, T, V) and idx (B, T) with T >= 2, got {tuple(logits.shape)} and {tuple(idx.shape)}")
    targets = torch.roll(idx, shifts=-1, dims=1).contiguous().reshape(-1)      # (the wrapped last column is not a listed row)
    rows = (torch.arange(B, device=idx.device).view(B, 1) * T + torch.arange(T - 1, device=idx.device).view(1, T - 1)).reshape(-1)
    return _NextTokenLossFn.apply(logits.contiguous(), targets, rows)


def readout_score_workspace(R: int, V: int, slices: int = 0, device=None) -> torch.Tensor:
    """The workspace of ``readout_score`` for R rows over V columns: one (max, sum) pair per row and slice, 8 R slices bytes."""
    n = L.lib().obte_readout_score_ws_bytes(R, V, slices)
    if n < 0:
        raise ValueError(f"readout_score_workspace: R >= 1, 1 <= V < 2^31 and 0 <= slices <= {L.READOUT_SCORE_MAX_SLICES}, got R={R} V={V} slices={slices}")
    return torch.empty(n, dtype=torch.uint8, device=device)


def readout_score(x, w, targets, alpha=1.0, slices=0, ws=None):
    """Log-probabilities under the readout without its logits (obte_readout_score_bf16): x bf16 (R, C), w bf16 (V, C) — both may be
    row-strided views with stride 1 along C — and targets int64 or int32 (R, K) or (R,), 1 <= K <= 64.  With
    z = bf16(alpha x w^T), the logits ``linear_fwd(x, w, alpha=alpha)`` would write, returns fp32 ``(logprobs, lse, logits_at)``:
    lse (R,) = logsumexp(z) over the V columns, logits_at = z at the targets, logprobs = logits_at - lse, the latter two shaped like
    ``targets``.  A target of -1 gives 0 in both; any other value outside [0, V) gives NaN in both.  Nothing of R V elements is
    allocated: ``ws`` (``readout_score_workspace``; None: allocated here) is 8 R slices bytes, ``slices`` = 0 lets the library pick the
    split over V.  Bitwise repeatable; at a fixed ``slices`` a row's results do not depend on the other rows."""
    _need(x, "x", contiguous=False); _need(w, "w", contiguous=False)
    if not isinstance(targets, torch.Tensor):
        raise TypeError("targets: expected a tensor")
    if not targets.is_cuda:
        raise RuntimeError(f"targets: the OmniBioTE HIP path runs on MI355X only; got a {targets.device} tensor (there is no CPU fallback)")
    if x.dim() != 2 or w.dim() != 2 or x.shape[1] != w.shape[1] or x.shape[0] < 1 or w.shape[0] < 1:
        raise ValueError(f"readout_score: x (R, C) and w (V, C), got {tuple(x.shape)} and {tuple(w.shape)}")
    R, Cc = x.shape
    V = w.shape[0]
    if x.stride(1) != 1 or w.stride(1) != 1:
        raise ValueError("readout_score: x and w must have stride 1 along C")
    if targets.dtype not in (torch.int64, torch.int32):
        raise ValueError(f"readout_score: targets must be int64 or int32, got {targets.dtype}")
    if targets.dim() not in (1, 2) or targets.shape[0] != R or (targets.dim() == 2 and not 1 <= targets.shape[1] <= L.READOUT_SCORE_MAX_K):
        raise ValueError(f"readout_score: targets must be ({R},) or ({R}, K) with 1 <= K <= {L.READOUT_SCORE_MAX_K}, got {tuple(targets.shape)}")
    if Cc % 64 != 0 or Cc < 64:
        raise ValueError(f"readout_score: C must be a multiple of 64, got {Cc}")
    if isinstance(slices, bool) or not isinstance(slices, int) or not 0 <= slices <= L.READOUT_SCORE_MAX_SLICES:
        raise ValueError(f"readout_score: slices must be an integer in [0, {L.READOUT_SCORE_MAX_SLICES}], got {slices!r}")
    K = 1 if targets.dim() == 1 else targets.shape[1]
    ldx = x.stride(0) if R > 1 else Cc
    ldw = w.stride(0) if V > 1 else Cc
    need = L.lib().obte_readout_score_ws_bytes(R, V, slices)
    if ws is None:
        ws = torch.empty(max(need, 0), dtype=torch.uint8, device=x.device)
    else:
        _need(ws, "ws", dtype=None)
        if ws.numel() * ws.element_size() < need:
            raise ValueError(f"readout_score: ws holds {ws.numel() * ws.element_size()} bytes, {need} are needed")
    tg = targets.to(torch.int32).contiguous()      # (token ids fit: V < 2^31; an id beyond int32 is out of range either way)
    if targets.dtype == torch.int64:
        tg = torch.where((targets < -1) | (targets >= V), torch.full_like(tg, -2), tg).contiguous()
    logprobs = torch.empty(targets.shape, dtype=torch.float32, device=x.device)
    logits_at = torch.empty(targets.shape, dtype=torch.float32, device=x.device)
    lse = torch.empty(R, dtype=torch.float32, device=x.device)
    L.check(L.lib().obte_readout_score_bf16(_ptr(x), ldx, _ptr(w), ldw, R, V, Cc, float(alpha), _ptr(tg), K, _ptr(logprobs), _ptr(lse), _ptr(logits_at),
                                            slices, _ptr(ws), ws.numel() * ws.element_size(), _stream()), "obte_readout_score_bf16")
    return logprobs, lse, logits_at


def readout_sample_workspace(R: int, V: int, slices: int = 0, device=None) -> torch.Tensor:
    """The workspace of ``readout_sample`` for R rows over V columns: a (max, sum) pair and a best triple per row and slice, 20 R slices bytes."""
    n = L.lib().obte_readout_sample_ws_bytes(R, V, slices)
    if n < 0:
        raise ValueError(f"readout_sample_workspace: R >= 1, 1 <= V < 2^31 and 0 <= slices <= {L.READOUT_SCORE_MAX_SLICES}, got R={R} V={V} slices={slices}")
    return torch.empty(n, dtype=torch.uint8, device=device)


def _seed64(what, seed):
    if isinstance(seed, bool) or not isinstance(seed, int) or not 0 <= seed < 2 ** 64:
        raise ValueError(f"{what}: seed must be an integer in [0, 2^64), got {seed!r}")
    return seed


def readout_sample(x, w, temperature, seed, keys=None, allowed=None, allowed_packed=None, alpha=1.0, slices=0, ws=None):
    """One token per row drawn from the readout's distribution without its logits (obte_readout_sample_bf16; the rule:
    include/omnibiote_hip_fill.h, in float64 sampling.readout_sample_reference): x bf16 (R, C), w bf16 (V, C), both possibly row-strided.
    With z = bf16(alpha x w^T) and y = z fp32(1 / temperature), returns ``(tokens int64 (R,), logprob fp32 (R,), lse fp32 (R,))``:
    the token is argmax_v y[v] + g[v] with the counter-based Gumbel noise g of (``seed``, the row's key, v) — a draw from softmax(y) —
    logprob its log-probability and lse = logsumexp(y).  ``keys`` int64 (R,) on the device (None: the row numbers): a row's draw depends
    on its key, its logits and the seed alone, not on R, ``slices`` or its place in the batch.  ``temperature`` 0: the lowest index of
    the maximum, lse and logprob as at temperature 1.  ``allowed`` bool (V,) or (R, V), or ``allowed_packed`` uint8 (n,) or (R, n) as
    ``pack_token_mask`` makes it: an excluded column enters neither the sum nor the draw; a row that allows nothing gets -1, -inf, -inf.
    Nothing of R V elements is allocated: ``ws`` (``readout_sample_workspace``; None: allocated here) is 20 R slices bytes."""
    from .sampling import inv_temperature
    _need(x, "x", contiguous=False); _need(w, "w", contiguous=False)
    if x.dim() != 2 or w.dim() != 2 or x.shape[1] != w.shape[1] or x.shape[0] < 1 or w.shape[0] < 1:
        raise ValueError(f"readout_sample: x (R, C) and w (V, C), got {tuple(x.shape)} and {tuple(w.shape)}")
    R, Cc = x.shape
    V = w.shape[0]
    if x.stride(1) != 1 or w.stride(1) != 1:
        raise ValueError("readout_sample: x and w must have stride 1 along C")
    if Cc % 64 != 0 or Cc < 64:
        raise ValueError(f"readout_sample: C must be a multiple of 64, got {Cc}")
    if isinstance(slices, bool) or not isinstance(slices, int) or not 0 <= slices <= L.READOUT_SCORE_MAX_SLICES:
        raise ValueError(f"readout_sample: slices must be an integer in [0, {L.READOUT_SCORE_MAX_SLICES}], got {slices!r}")
    try:
        inv_temp = inv_temperature(temperature)
    except ValueError as e:
        raise ValueError(f"readout_sample: {e}") from None
    seed = _seed64("readout_sample", seed)
    if keys is not None:
        _need(keys, "keys", torch.int64)
        if keys.shape != (R,):
            raise ValueError(f"readout_sample: keys must be int64 ({R},), got {tuple(keys.shape)}")
    con = _constraint("readout_sample", R, V, x.device, allowed, allowed_packed, None, None, 0)
    mask, mask_ld = (None, 0) if con is None else (con[0], con[1])
    ldx = x.stride(0) if R > 1 else Cc
    ldw = w.stride(0) if V > 1 else Cc
    need = L.lib().obte_readout_sample_ws_bytes(R, V, slices)
    if ws is None:
        ws = torch.empty(max(need, 0), dtype=torch.uint8, device=x.device)
    else:
        _need(ws, "ws", dtype=None)
        if ws.numel() * ws.element_size() < need:
            raise ValueError(f"readout_sample: ws holds {ws.numel() * ws.element_size()} bytes, {need} are needed")
    tokens = torch.empty(R, dtype=torch.int32, device=x.device)
    logprob = torch.empty(R, dtype=torch.float32, device=x.device)
    lse = torch.empty(R, dtype=torch.float32, device=x.device)
    L.check(L.lib().obte_readout_sample_bf16(_ptr(x), ldx, _ptr(w), ldw, R, V, Cc, float(alpha), inv_temp, seed, _ptr(keys), _ptr(mask), mask_ld,
                                             _ptr(tokens), _ptr(logprob), _ptr(lse), slices, _ptr(ws), ws.numel() * ws.element_size(), _stream()),
            "obte_readout_sample_bf16")
    return tokens.long(), logprob, lse


FILL_ORDERS = {"confidence": L.FILL_CONFIDENCE, "random": L.FILL_RANDOM, "left": L.FILL_LEFT}


def fill_commit(rows, seg_off, tokens, logprob, take, order, seed, idx, out_logprob, rows_next, seg_off_next, max_seg):
    """An unmasking iteration's bookkeeping in one launch and in place (obte_fill_commit; the rule: include/omnibiote_hip_fill.h, in plain
    torch sampling.fill_commit_reference).  ``rows`` int64 (n,) ascending flat positions, sequence b's entries the run
    [seg_off[b], seg_off[b + 1]) (``seg_off`` int32 (B + 1,) on the device; ``max_seg`` <= 8192: the host's bound on a run);
    ``tokens`` int64 or int32 (n,) and ``logprob`` fp32 (n,) belong to the entries.  ``take`` int32 (B,) of each sequence's entries are
    selected by ``order`` ("confidence", "random" under ``seed``, "left"): their tokens go to ``idx`` (int64, any shape, contiguous) and
    their logprobs to ``out_logprob`` (fp32, as many elements) at the entries' positions; the other positions go, ascending, to
    ``rows_next`` (int64) at ``seg_off_next[b]`` (int32 (B + 1,)).  Returns nothing."""
    if order not in FILL_ORDERS:
        raise ValueError(f"fill_commit: order must be one of {tuple(FILL_ORDERS)}, got {order!r}")
    seed = _seed64("fill_commit", seed)
    for t, name, dt in ((rows, "rows", torch.int64), (seg_off, "seg_off", torch.int32), (logprob, "logprob", torch.float32), (take, "take", torch.int32),
                        (idx, "idx", torch.int64), (out_logprob, "out_logprob", torch.float32), (rows_next, "rows_next", torch.int64),
                        (seg_off_next, "seg_off_next", torch.int32)):
        _need(t, name, dt)
    _need(tokens, "tokens", None)
    if tokens.dtype not in (torch.int64, torch.int32):
        raise ValueError(f"fill_commit: tokens must be int64 or int32, got {tokens.dtype}")
    n, B = rows.numel(), take.numel()
    if rows.dim() != 1 or tokens.shape != (n,) or logprob.shape != (n,):
        raise ValueError(f"fill_commit: rows, tokens and logprob must be (n,), got {tuple(rows.shape)}, {tuple(tokens.shape)} and {tuple(logprob.shape)}")
    if B < 1 or take.dim() != 1 or seg_off.shape != (B + 1,) or seg_off_next.shape != (B + 1,):
        raise ValueError(f"fill_commit: take (B,), seg_off and seg_off_next (B + 1,), got {tuple(take.shape)}, {tuple(seg_off.shape)} and "
                         f"{tuple(seg_off_next.shape)}")
    if idx.numel() < 1 or out_logprob.numel() != idx.numel():
        raise ValueError(f"fill_commit: idx and out_logprob must hold the same number (>= 1) of elements, got {idx.numel()} and {out_logprob.numel()}")
    if isinstance(max_seg, bool) or not isinstance(max_seg, int) or not 0 <= max_seg <= L.FILL_MAX_SEG:
        raise ValueError(f"fill_commit: max_seg must be an integer in [0, {L.FILL_MAX_SEG}] (entries per sequence), got {max_seg!r}")
    if rows_next.dim() != 1 or (n > 0 and rows_next.data_ptr() == rows.data_ptr()):
        raise ValueError("fill_commit: rows_next must be a 1-D buffer of its own")
    tk = tokens if tokens.dtype == torch.int32 else tokens.to(torch.int32)
    pad = torch.empty(2, dtype=torch.int64, device=idx.device)    # an empty tensor has no address: the C call wants non-null, distinct pointers
    one, two = pad[:1], pad[1:]
    L.check(L.lib().obte_fill_commit(_ptr(rows if n else one), _ptr(seg_off), n, B, max_seg, _ptr(tk if n else one), _ptr(logprob if n else one), _ptr(take),
                                     FILL_ORDERS[order], seed, _ptr(idx), _ptr(out_logprob), idx.numel(), _ptr(rows_next if rows_next.numel() else two),
                                     _ptr(seg_off_next), rows_next.numel(), _stream()), "obte_fill_commit")


def adamw_step_(p, g, m, v, lr, beta1, beta2, eps, weight_decay, step, clip_coef=None):
    for t, n in ((p, "p"), (g, "g"), (m, "m"), (v, "v")):
        _need(t, n)
    assert p.numel() == g.numel() == m.numel() == v.numel()
    L.check(L.lib().obte_adamw_bf16(_ptr(p), _ptr(g), _ptr(m), _ptr(v), p.numel(), lr, beta1, beta2, eps, weight_decay,
                                     int(step), _ptr(clip_coef), _stream()), "obte_adamw_bf16")


def sumsq_(g, out):
    _need(g, "g"); _need(out, "out", torch.float32)
    L.check(L.lib().obte_sumsq_bf16(_ptr(g), g.numel(), _ptr(out), _stream()), "obte_sumsq_bf16")


# -------------------------------------------------------------------------------------------------------- block
def _block_desc(B, T, Cc, H, params, rope, mask: MaskSpec, dropout_p=0.0, dropout_seed=0, ln_partials=None, ln_partial_mode=0, out_rows=None,
                dy_masked=None, dx_masked=None, dx_mask_seed=0, acc32=None, acc32_mode=0):
    ln1, attn_w, proj_w, ln2, fc_w, mlp_w = params
    p1, p2 = ln_partials if ln_partials is not None else (None, None)
    if out_rows is not None:
        _need(out_rows, "out_rows", torch.int64)
        assert 0 < out_rows.numel() <= B * T, "the rows form of the block: a non-empty list of positions"
    a32 = acc32 if acc32_mode else (None, None, None, None)   # the four matrices' fp32 sums: attn, proj, fc, mlp
    return L.BlockDesc(B, T, Cc, H, _ptr(ln1), _ptr(attn_w), _ptr(proj_w), _ptr(ln2), _ptr(fc_w), _ptr(mlp_w),
                       _ptr(rope[0]), _ptr(rope[1]), _ptr(mask.ranges), _ptr(mask.dense), mask.sb, mask.sh, mask.sq,
                       float(dropout_p), int(dropout_seed), _ptr(mask.qbounds), _ptr(p1), _ptr(p2), int(ln_partial_mode), _ptr(mask.exact),
                       _ptr(out_rows), 0 if out_rows is None else out_rows.numel(), _ptr(dy_masked), _ptr(dx_masked), int(dx_mask_seed),
                       _ptr(a32[0]), _ptr(a32[1]), _ptr(a32[2]), _ptr(a32[3]), int(acc32_mode))


def block_fwd(x, params, rope, H, mask: MaskSpec, dropout_p=0.0, dropout_seed=0, out_rows=None):
    """One transformer block forward.  Returns (y, act) where act is the opaque saved-activation buffer.
    out_rows (int64 (n,), ascending distinct rows of the [B*T, C] activation): only those positions of the output are
    wanted — y is [n, C], the MLP half runs on them alone (include/omnibiote_hip.h, obte_block_desc::out_rows).  With dropout
    the mask of the MLP projection (site 3) is that of the [n, C] output — element (i, c) — in forward and backward alike."""
    _need(x, "x")
    B, T, Cc = x.shape
    for i, w in enumerate(params):
        _need(w, f"param{i}")
    _need(rope[0], "rope_cos", torch.float32); _need(rope[1], "rope_sin", torch.float32)
    assert rope[0].shape[0] >= T
    y = torch.empty_like(x) if out_rows is None else torch.empty((out_rows.numel(), Cc), dtype=bf16, device=x.device)
    act = torch.empty(int(L.lib().obte_block_act_bytes_p(B, T, Cc, H, float(dropout_p))), dtype=torch.uint8, device=x.device)
    d = _block_desc(B, T, Cc, H, params, rope, mask, dropout_p, dropout_seed, out_rows=out_rows)
    L.check(L.lib().obte_block_fwd(C.byref(d), _ptr(x), _ptr(y), _ptr(act), _stream()), "obte_block_fwd")
    return y, act


def infer_enabled() -> bool:
    """OBTE_INFER=0: a forward nobody can differentiate runs the training forward (block_fwd, the two-output GELU epilogue)
    instead of block_infer / EPI_GELU_ACT.  Same results.  Read per call."""
    return os.environ.get("OBTE_INFER", "") != "0"


def block_infer_workspace(B, T, Cc, H, device) -> torch.Tensor:
    """The scratch of block_infer for this shape: contents irrelevant before and after, so one buffer serves every block of a forward."""
    nbytes = int(L.lib().obte_block_infer_ws_bytes(B, T, Cc, H))
    if nbytes <= 0:
        raise RuntimeError(f"block_infer: unsupported shape (B {B}, T {T}, n_embd {Cc}, n_head {H}): head size 64 or 128, "
                           "n_embd a multiple of 64 and <= 4096")
    return torch.empty(nbytes, dtype=torch.uint8, device=device)


def block_infer(x, params, rope, H, mask: MaskSpec, dropout_p=0.0, dropout_seed=0, ws=None, out=None):
    """One transformer block forward with nothing kept for a backward (obte_block_fwd_infer): y, bit for bit block_fwd's.
    ws: a buffer from block_infer_workspace for this shape (allocated here when None).  out: where y goes; it may be x itself."""
    return _block_call(x, params, rope, H, ws, out, block_infer_workspace, lambda d, y, w: L.check(
        L.lib().obte_block_fwd_infer(d, _ptr(x), _ptr(y), _ptr(w), w.numel(), _stream()), "obte_block_fwd_infer"), mask, dropout_p, dropout_seed)


def _block_call(x, params, rope, H, ws, out, new_ws, call, mask=None, dropout_p=0.0, dropout_seed=0, cache=None, T_max=0, rows=None, at=0, one=False, kv8=False):
    """What block_infer, block_prefill, block_decode, block_decode_rows and block_extend share: the checks of x (B, T, C — or, ``one``, (B, C)
    at T = 1), the cache, ``rows`` (a per-row int32 tensor and its name), the parameters and the tables (``at`` + T rows of them), the
    workspace (``new_ws(B, T, C, H, device)`` when ws is None) and the output (x's like when out is None), then ``call(d, y, ws)`` with the
    descriptor by reference.  ``kv8``: the cache is the e4m3 one (kv8_cache_buffer).  Returns y."""
    _need(x, "x")
    if cache is not None:
        _need(cache, "cache", torch.uint8 if kv8 else bf16)
    if one:
        (B, Cc), T = x.shape, 1
    else:
        B, T, Cc = x.shape
    if rows is not None:
        _need_rows(*rows, B)
    for i, w in enumerate(params):
        _need(w, f"param{i}")
    _need(rope[0], "rope_cos", torch.float32); _need(rope[1], "rope_sin", torch.float32)
    assert rope[0].shape[0] >= at + T
    assert cache is None or cache.numel() * cache.element_size() == (L.lib().obte_kv8_cache_bytes if kv8 else L.lib().obte_kv_cache_bytes)(B, T_max, H, Cc // H)
    if ws is None:
        ws = new_ws(B, T, Cc, H, x.device)
    else:
        _need(ws, "ws", torch.uint8)
    y = torch.empty_like(x) if out is None else out
    _need(y, "out"); assert y.shape == x.shape
    d = _block_desc(B, T, Cc, H, params, rope, MaskSpec() if mask is None else mask, dropout_p, dropout_seed)
    call(C.byref(d), y, ws)
    return y


# --------------------------------------------------------------------------------------------------- generation
def kv_cache_buffer(B, T_max, H, hs, device) -> torch.Tensor:
    """One layer's key/value cache (K [B, H, T_max, hs], then V, bf16) as the flat bf16 tensor the entry points take."""
    nbytes = int(L.lib().obte_kv_cache_bytes(B, T_max, H, hs))
    if nbytes <= 0:
        raise RuntimeError(f"kv_cache_buffer: unsupported shape (B {B}, T_max {T_max}, n_head {H}, head size {hs}): head size 64 or 128")
    return torch.empty(nbytes // 2, dtype=bf16, device=device)


def kv_cache_store(qkv, B, t, H, hs, cache, T_max, pos0):
    """Copy the k and v thirds of the packed, rotated qkv [B*t, 3C] into positions [pos0, pos0 + t) of the cache (obte_kv_cache_store)."""
    _need(qkv, "qkv"); _need(cache, "cache")
    assert qkv.numel() == B * t * 3 * H * hs and cache.numel() * 2 == L.lib().obte_kv_cache_bytes(B, T_max, H, hs)
    L.check(L.lib().obte_kv_cache_store(_ptr(qkv), B, t, H, hs, _ptr(cache), T_max, pos0, _stream()), "obte_kv_cache_store")
    return cache


def attn_decode(q, cache, B, T_max, n_keys, H, hs, scale, splits=0, q_ld=None, ws=None):
    """One query per (b, h) over cache positions [0, n_keys) (obte_attn_decode): (o (B, C) bf16, lse (B, H) fp32).  q: any bf16 tensor
    whose row b holds the query of head h at b * q_ld + h * hs (q_ld defaults to its last dimension: 3C reads a packed row in place).
    splits: 0 = the library's choice, else a forced count."""
    return _attn_decode_call(q, cache, B, T_max, H, hs, q_ld, ws, None, lambda q_ld, o, lse, w: L.check(
        L.lib().obte_attn_decode(_ptr(q), q_ld, _ptr(cache), _ptr(o), _ptr(lse), B, T_max, n_keys, H, hs, float(scale), int(splits), _ptr(w), w.numel(),
                                 _stream()), "obte_attn_decode"))


def _attn_decode_call(q, cache, B, T_max, H, hs, q_ld, ws, rows, call):
    """What attn_decode and attn_decode_rows (``rows``: its per-row counts) share: the checks, the default q_ld and workspace, the outputs,
    then ``call(q_ld, o, lse, ws)``.  Returns (o, lse)."""
    _need(q, "q"); _need(cache, "cache")
    if rows is not None:
        _need_rows(rows, "n_keys", B)
    q_ld = q.shape[-1] if q_ld is None else q_ld
    assert q.numel() >= (B - 1) * q_ld + H * hs and cache.numel() * 2 == L.lib().obte_kv_cache_bytes(B, T_max, H, hs)
    o = torch.empty((B, H * hs), dtype=bf16, device=q.device)
    lse = torch.empty((B, H), dtype=torch.float32, device=q.device)
    if ws is None:
        ws = torch.empty(int(L.lib().obte_attn_decode_ws_bytes(B, H, hs)), dtype=torch.uint8, device=q.device)
    call(q_ld, o, lse, ws)
    return o, lse


def block_prefill(x, params, rope, H, mask: MaskSpec, cache, T_max, ws=None, out=None):
    """block_infer (y bit for bit its y, the same workspace) that also leaves the block's rotated keys and its values in positions
    [0, T) of `cache` (obte_block_fwd_prefill).  No dropout on a generation path."""
    return _block_call(x, params, rope, H, ws, out, block_infer_workspace, lambda d, y, w: L.check(
        L.lib().obte_block_fwd_prefill(d, _ptr(x), _ptr(y), _ptr(w), w.numel(), _ptr(cache), T_max, _stream()), "obte_block_fwd_prefill"),
        mask, cache=cache, T_max=T_max)


def block_decode_workspace(B, Cc, H, device) -> torch.Tensor:
    nbytes = int(L.lib().obte_block_decode_ws_bytes(B, Cc, H))
    if nbytes <= 0:
        raise RuntimeError(f"block_decode: unsupported shape (B {B}, n_embd {Cc}, n_head {H}): head size 64 or 128, "
                           "n_embd a multiple of 64 and <= 4096")
    return torch.empty(nbytes, dtype=torch.uint8, device=device)


def block_decode(x, params, rope, H, cache, T_max, pos, ws=None, out=None):
    """One new position per batch row, every row at position `pos`, against the cache (obte_block_decode): x (B, C) -> y (B, C).
    rope: the FULL tables (at least pos + 1 rows).  out may be x itself."""
    return _block_call(x, params, rope, H, ws, out, _decode_ws, lambda d, y, w: L.check(
        L.lib().obte_block_decode(d, _ptr(x), _ptr(y), _ptr(cache), T_max, pos, _ptr(w), w.numel(), _stream()), "obte_block_decode"),
        cache=cache, T_max=T_max, at=pos, one=True)


def _decode_ws(B, T, Cc, H, device):
    return block_decode_workspace(B, Cc, H, device)


# ---- one cache position per row: a batch whose rows stand at different positions (include/omnibiote_hip_rows.h, the row convention) ----
def _need_rows(t, name, B):
    _need(t, name, torch.int32)
    if t.shape != (B,):
        raise ValueError(f"{name}: expected shape ({B},), got {tuple(t.shape)}")


def kv_cache_rope_store_rows(qkv, rope, pos, max_pos, B, H, hs, cache, T_max):
    """One decode step's rotate-and-store (obte_kv_cache_rope_store_rows): the q and k thirds of row b of the unrotated packed qkv
    [B, 3C] are rotated in place by row pos[b] of the FULL tables, the rotated k and the v written to cache position pos[b].  pos: int32
    (B,) on the device; a row whose value lies outside [0, max_pos] is left alone."""
    _need(qkv, "qkv"); _need(cache, "cache"); _need_rows(pos, "pos", B)
    _need(rope[0], "rope_cos", torch.float32); _need(rope[1], "rope_sin", torch.float32)
    assert qkv.numel() == B * 3 * H * hs and cache.numel() * 2 == L.lib().obte_kv_cache_bytes(B, T_max, H, hs)
    assert rope[0].shape[0] > max_pos and rope[1].shape[0] > max_pos
    L.check(L.lib().obte_kv_cache_rope_store_rows(_ptr(qkv), _ptr(rope[0]), _ptr(rope[1]), _ptr(pos), int(max_pos), B, H, hs, _ptr(cache), T_max,
                                                  _stream()), "obte_kv_cache_rope_store_rows")
    return qkv


def attn_decode_rows(q, cache, B, T_max, n_keys, max_keys, H, hs, scale, splits=0, q_ld=None, ws=None):
    """attn_decode with one key count per row (obte_attn_decode_rows): n_keys int32 (B,) on the device, row b over cache positions
    [0, n_keys[b]); a row whose count lies outside [1, max_keys] gives zeros and lse = -inf.  splits = 0: the library's choice at max_keys."""
    return _attn_decode_call(q, cache, B, T_max, H, hs, q_ld, ws, n_keys, lambda q_ld, o, lse, w: L.check(
        L.lib().obte_attn_decode_rows(_ptr(q), q_ld, _ptr(cache), _ptr(o), _ptr(lse), B, T_max, _ptr(n_keys), int(max_keys), H, hs, float(scale),
                                      int(splits), _ptr(w), w.numel(), _stream()), "obte_attn_decode_rows"))


def block_decode_rows(x, params, rope, H, cache, T_max, pos, max_pos, ws=None, out=None):
    """block_decode with row b at position pos[b] (obte_block_decode_rows): pos int32 (B,) on the device, read there; max_pos the host's
    bound on it (a row outside [0, max_pos] stores nothing and attends to nothing).  rope: the FULL tables.  out may be x itself."""
    return _block_call(x, params, rope, H, ws, out, _decode_ws, lambda d, y, w: L.check(
        L.lib().obte_block_decode_rows(d, _ptr(x), _ptr(y), _ptr(cache), T_max, _ptr(pos), int(max_pos), _ptr(w), w.numel(), _stream()),
        "obte_block_decode_rows"), cache=cache, T_max=T_max, rows=(pos, "pos"), at=max_pos, one=True)


# ---- the key/value cache stored as OCP e4m3 (include/omnibiote_hip_kv8.h; the format in plain torch: kvquant.py) ----
def kv8_cache_buffer(B, T_max, H, hs, device) -> torch.Tensor:
    """One layer's e4m3 key/value cache (K codes [B, H, T_max, hs], V codes, K scales fp32 [B, H, T_max], V scales) as the flat uint8
    tensor the kv8 entry points take: 2 (hs + 4) bytes per cached head vector against the bf16 cache's 4 hs."""
    nbytes = int(L.lib().obte_kv8_cache_bytes(B, T_max, H, hs))
    if nbytes <= 0:
        raise RuntimeError(f"kv8_cache_buffer: unsupported shape (B {B}, T_max {T_max}, n_head {H}, head size {hs}): head size 64 or 128")
    return torch.empty(nbytes, dtype=torch.uint8, device=device)


def _need_kv8(cache, B, T_max, H, hs):
    _need(cache, "cache", torch.uint8)
    assert cache.numel() == L.lib().obte_kv8_cache_bytes(B, T_max, H, hs)


def kv8_cache_store(qkv, B, t, H, hs, cache, T_max, pos0):
    """kv_cache_store into an e4m3 cache (obte_kv8_cache_store): the k and v thirds of the packed, rotated qkv [B*t, 3C], quantised per
    head vector, into positions [pos0, pos0 + t)."""
    _need(qkv, "qkv"); _need_kv8(cache, B, T_max, H, hs)
    assert qkv.numel() == B * t * 3 * H * hs
    L.check(L.lib().obte_kv8_cache_store(_ptr(qkv), B, t, H, hs, _ptr(cache), T_max, pos0, _stream()), "obte_kv8_cache_store")
    return cache


def kv8_cache_rope_store_rows(qkv, rope, pos, max_pos, B, H, hs, cache, T_max):
    """kv_cache_rope_store_rows into an e4m3 cache (obte_kv8_cache_rope_store_rows): qkv is left with the same bits, the rotated k and
    the v of row b are quantised into cache position pos[b]; a row whose value lies outside [0, max_pos] is left alone."""
    _need(qkv, "qkv"); _need_kv8(cache, B, T_max, H, hs); _need_rows(pos, "pos", B)
    _need(rope[0], "rope_cos", torch.float32); _need(rope[1], "rope_sin", torch.float32)
    assert qkv.numel() == B * 3 * H * hs
    assert rope[0].shape[0] > max_pos and rope[1].shape[0] > max_pos
    L.check(L.lib().obte_kv8_cache_rope_store_rows(_ptr(qkv), _ptr(rope[0]), _ptr(rope[1]), _ptr(pos), int(max_pos), B, H, hs, _ptr(cache), T_max,
                                                   _stream()), "obte_kv8_cache_rope_store_rows")
    return qkv


def attn_decode_kv8(q, cache, B, T_max, n_keys, H, hs, scale, splits=0, q_ld=None, ws=None, n_keys_rows=None, out=None, lse=None):
    """attn_decode over an e4m3 cache (obte_attn_decode_kv8): (o (B, C) bf16, lse (B, H) fp32).  n_keys_rows: None, every row over
    cache positions [0, n_keys); or int32 (B,) on the device, row b over [0, n_keys_rows[b]) with n_keys the host's bound (a row whose
    count lies outside [1, n_keys] gives zeros and lse = -inf).  splits, q_ld and ws as in attn_decode; out / lse: where the results go
    (allocated here when None)."""
    _need(q, "q", contiguous=False); _need_kv8(cache, B, T_max, H, hs)
    if n_keys_rows is not None:
        _need_rows(n_keys_rows, "n_keys_rows", B)
    q_ld = q.shape[-1] if q_ld is None else q_ld
    assert not q.is_contiguous() or q.numel() >= (B - 1) * q_ld + H * hs     # (a strided q: rows of q_ld elements, the caller's account)
    o = torch.empty((B, H * hs), dtype=bf16, device=q.device) if out is None else out
    lse = torch.empty((B, H), dtype=torch.float32, device=q.device) if lse is None else lse
    if ws is None:
        ws = torch.empty(int(L.lib().obte_attn_decode_ws_bytes(B, H, hs)), dtype=torch.uint8, device=q.device)
    L.check(L.lib().obte_attn_decode_kv8(_ptr(q), q_ld, _ptr(cache), _ptr(o), _ptr(lse), B, T_max, int(n_keys), _ptr(n_keys_rows), H, hs, float(scale),
                                         int(splits), _ptr(ws), ws.numel(), _stream()), "obte_attn_decode_kv8")
    return o, lse


def block_prefill_kv8(x, params, rope, H, mask: MaskSpec, cache, T_max, ws=None, out=None):
    """block_prefill into an e4m3 cache (obte_block_fwd_prefill_kv8): y bit for bit block_infer's, the prompt's own attention on the
    unquantised qkv, the rotated keys and the values quantised into positions [0, T)."""
    return _block_call(x, params, rope, H, ws, out, block_infer_workspace, lambda d, y, w: L.check(
        L.lib().obte_block_fwd_prefill_kv8(d, _ptr(x), _ptr(y), _ptr(w), w.numel(), _ptr(cache), T_max, _stream()), "obte_block_fwd_prefill_kv8"),
        mask, cache=cache, T_max=T_max, kv8=True)


def block_decode_kv8(x, params, rope, H, cache, T_max, pos, pos_rows=None, ws=None, out=None):
    """block_decode (pos_rows None: every row at position `pos`) or block_decode_rows (pos_rows int32 (B,) on the device, `pos` the
    host's bound on it) against an e4m3 cache (obte_block_decode_kv8): x (B, C) -> y (B, C).  rope: the FULL tables.  out may be x."""
    return _block_call(x, params, rope, H, ws, out, _decode_ws, lambda d, y, w: L.check(
        L.lib().obte_block_decode_kv8(d, _ptr(x), _ptr(y), _ptr(cache), T_max, int(pos), _ptr(pos_rows), _ptr(w), w.numel(), _stream()),
        "obte_block_decode_kv8"), cache=cache, T_max=T_max, rows=None if pos_rows is None else (pos_rows, "pos_rows"), at=pos, one=True, kv8=True)


# ---- the decode step with its weights stored as OCP e4m3 (include/omnibiote_hip_w8.h; the format in plain torch: w8quant.py) ----
def block_step_w8(x, params, w8, rope, H, cache, T_max, pos, pos_rows=None, kv8=False, ws=None, out=None):
    """block_decode (pos_rows None: every row at position ``pos``), block_decode_rows (pos_rows int32 (B,) on the device, ``pos`` the
    host's bound on it) or, ``kv8``, block_decode_kv8 with the four products on linear_small_m_w8 (obte_block_step_w8): x (B, C) -> y (B, C).
    w8 = (codes, scales): four uint8 (N, K) tensors in w8quant's stored order and four fp32 (N,) ones, in the order c_attn, attention c_proj,
    c_fc, MLP c_proj.  ``params`` holds the DEQUANTISED four weights (``w8quant.dequantize_weight``): the result has the bits of the
    bf16 step on them, and above small_m_max rows the products run on the tile structures from them."""
    codes, scales = w8
    if len(codes) != 4 or len(scales) != 4:
        raise ValueError("block_step_w8: w8 = (four code tensors, four scale tensors)")
    for i, (c, sc, w) in enumerate(zip(codes, scales, (params[1], params[2], params[4], params[5]))):
        _need(c, f"codes{i}", torch.uint8); _need(sc, f"scales{i}", torch.float32)
        if c.shape != w.shape or sc.shape != (w.shape[0],):
            raise ValueError(f"block_step_w8: codes{i} {tuple(c.shape)} / scales{i} {tuple(sc.shape)} do not match the weight {tuple(w.shape)}")
    cp = (C.c_void_p * 4)(*[_ptr(c) for c in codes])
    sp = (C.c_void_p * 4)(*[_ptr(sc) for sc in scales])
    return _block_call(x, params, rope, H, ws, out, _decode_ws, lambda d, y, w: L.check(
        L.lib().obte_block_step_w8(d, cp, sp, _ptr(x), _ptr(y), _ptr(cache), 1 if kv8 else 0, T_max, int(pos), _ptr(pos_rows), _ptr(w), w.numel(),
                                   _stream()), "obte_block_step_w8"),
        cache=cache, T_max=T_max, rows=None if pos_rows is None else (pos_rows, "pos_rows"), at=pos, one=True, kv8=kv8)


# ---- the same with the weights stored as OCP MXFP4 (include/omnibiote_hip_w4.h; the format in plain torch: w4quant.py) ----
def block_step_w4(x, params, w4, rope, H, cache, T_max, pos, pos_rows=None, kv8=False, ws=None, out=None):
    """block_step_w8 with the four products on linear_small_m_w4 (obte_block_step_w4): x (B, C) -> y (B, C).  w4 = (codes, scales): four
    uint8 (N, K / 2) tensors in w4quant's stored order and four uint8 (N, K / 32) ones, in the order c_attn, attention c_proj, c_fc, MLP
    c_proj.  ``params`` holds the DEQUANTISED four weights (``w4quant.dequantize_weight``): the result has the bits of the bf16 step on
    them, and above small_m_max rows the products run on the tile structures from them."""
    codes, scales = w4
    if len(codes) != 4 or len(scales) != 4:
        raise ValueError("block_step_w4: w4 = (four code tensors, four scale tensors)")
    for i, (c, sc, w) in enumerate(zip(codes, scales, (params[1], params[2], params[4], params[5]))):
        _need(c, f"codes{i}", torch.uint8); _need(sc, f"scales{i}", torch.uint8)
        if w.shape[1] % 64 != 0 or c.shape != (w.shape[0], w.shape[1] // 2) or sc.shape != (w.shape[0], w.shape[1] // 32):
            raise ValueError(f"block_step_w4: codes{i} {tuple(c.shape)} / scales{i} {tuple(sc.shape)} do not match the weight {tuple(w.shape)}")
    cp = (C.c_void_p * 4)(*[_ptr(c) for c in codes])
    sp = (C.c_void_p * 4)(*[_ptr(sc) for sc in scales])
    return _block_call(x, params, rope, H, ws, out, _decode_ws, lambda d, y, w: L.check(
        L.lib().obte_block_step_w4(d, cp, sp, _ptr(x), _ptr(y), _ptr(cache), 1 if kv8 else 0, T_max, int(pos), _ptr(pos_rows), _ptr(w), w.numel(),
                                   _stream()), "obte_block_step_w4"),
        cache=cache, T_max=T_max, rows=None if pos_rows is None else (pos_rows, "pos_rows"), at=pos, one=True, kv8=kv8)


# ---- n new positions per row against a filled cache (include/omnibiote_hip_extend.h) ----
def kv_cache_rope_store_chunk(qkv, rope, pos, max_pos, B, n, H, hs, cache, T_max):
    """The rows form's rotate-and-store of a chunk (obte_kv_cache_rope_store_chunk): the q and k thirds of rows b * n + j of the unrotated
    packed qkv [B * n, 3C] are rotated in place by row pos[b] + j of the FULL tables, the rotated k and the v written to cache position
    pos[b] + j.  pos: int32 (B,) on the device; a row whose value lies outside [0, max_pos] is left alone."""
    _need(qkv, "qkv"); _need(cache, "cache"); _need_rows(pos, "pos", B)
    _need(rope[0], "rope_cos", torch.float32); _need(rope[1], "rope_sin", torch.float32)
    assert qkv.numel() == B * n * 3 * H * hs and cache.numel() * 2 == L.lib().obte_kv_cache_bytes(B, T_max, H, hs)
    assert rope[0].shape[0] >= max_pos + n and rope[1].shape[0] >= max_pos + n
    L.check(L.lib().obte_kv_cache_rope_store_chunk(_ptr(qkv), _ptr(rope[0]), _ptr(rope[1]), _ptr(pos), int(max_pos), B, n, H, hs, _ptr(cache), T_max,
                                                   _stream()), "obte_kv_cache_rope_store_chunk")
    return qkv


def attn_extend(q, cache, B, T_max, n, pos, H, hs, scale, splits=0, q_ld=None, ws=None, pos_rows=None, out=None, lse=None):
    """n queries per (b, h) at positions p_b .. p_b + n - 1, query j over cache positions [0, p_b + j + 1) (obte_attn_extend):
    (o (B * n, C) bf16, lse (B, H, n) fp32).  The chunk's own keys and values are in the cache already.  p_b = pos for every row, or
    pos_rows[b] (int32 (B,) on the device, pos then its bound; a row outside [0, pos] gives zeros and lse = -inf).  q: any bf16 tensor
    whose row b * n + j holds the query of head h at (b * n + j) * q_ld + h * hs (q_ld defaults to its last dimension).  splits: 0 = the
    library's choice, else a forced count.  out / lse: where the results go (allocated here when None)."""
    _need(q, "q", contiguous=False); _need(cache, "cache")
    if pos_rows is not None:
        _need_rows(pos_rows, "pos_rows", B)
    q_ld = q.shape[-1] if q_ld is None else q_ld
    assert n >= 1 and cache.numel() * 2 == L.lib().obte_kv_cache_bytes(B, T_max, H, hs)
    o = torch.empty((B * n, H * hs), dtype=bf16, device=q.device) if out is None else out
    lse = torch.empty((B, H, n), dtype=torch.float32, device=q.device) if lse is None else lse
    if ws is None:
        ws = torch.empty(max(int(L.lib().obte_attn_extend_ws_bytes(B, H, hs, n, int(splits))), 16), dtype=torch.uint8, device=q.device)
    L.check(L.lib().obte_attn_extend(_ptr(q), q_ld, _ptr(cache), _ptr(o), _ptr(lse), B, T_max, n, int(pos), _ptr(pos_rows), H, hs, float(scale),
                                     int(splits), _ptr(ws), ws.numel(), _stream()), "obte_attn_extend")
    return o, lse


def block_extend_ws_bytes(B, n, Cc, H) -> int:
    """obte_block_extend_ws_bytes, an unsupported shape raised.  NOT monotone in n (the attention partials follow the default split
    count, which drops as n grows): a buffer kept for reuse is judged by its bytes, not by the n it was made for."""
    nbytes = int(L.lib().obte_block_extend_ws_bytes(B, n, Cc, H))
    if nbytes <= 0:
        raise RuntimeError(f"block_extend: unsupported shape (B {B}, n {n}, n_embd {Cc}, n_head {H}): head size 64 or 128, "
                           "n_embd a multiple of 64 and <= 4096")
    return nbytes


def block_extend_workspace(B, n, Cc, H, device) -> torch.Tensor:
    return torch.empty(block_extend_ws_bytes(B, n, Cc, H), dtype=torch.uint8, device=device)


def block_extend(x, params, rope, H, cache, T_max, pos, pos_rows=None, ws=None, out=None):
    """n new positions per batch row against the cache (obte_block_extend): x (B, n, C) -> y (B, n, C).  Row b's positions start at
    `pos`, or at pos_rows[b] (int32 (B,) on the device, read there; pos is then the host's bound on it, and a row outside [0, pos] stores
    nothing and attends to nothing).  rope: the FULL tables (at least pos + n rows).  out may be x itself."""
    return _block_call(x, params, rope, H, ws, out, block_extend_workspace, lambda d, y, w: L.check(
        L.lib().obte_block_extend(d, _ptr(x), _ptr(y), _ptr(cache), T_max, int(pos), _ptr(pos_rows), _ptr(w), w.numel(), _stream()), "obte_block_extend"),
        cache=cache, T_max=T_max, rows=None if pos_rows is None else (pos_rows, "pos_rows"), at=pos)


# ---- a prefix cache shared by groups of rows: many samples per prompt (include/omnibiote_hip_shared.h) ----
def attn_decode_shared(q, prefix_cache, P, T_pre, n_prefix, suffix_cache, G, T_suf, n_suffix, H, hs, scale, prefix_splits=0, suffix_splits=0, q_ld=None,
                       ws=None, out=None, lse=None):
    """One query per (b, h) of B = P * G rows, row b = p * G + g, over positions [0, n_prefix) of row p of the prefix cache followed by
    slots [0, n_suffix) of row b of the suffix cache (obte_attn_decode_shared): (o (B, C) bf16, lse (B, H) fp32).  Both caches are
    kv_cache_buffer's, of P and of B rows.  q: any bf16 tensor whose row b holds the query of head h at b * q_ld + h * hs (q_ld
    defaults to its last dimension).  n_suffix = 0: the prefix alone (suffix_cache may then be None).  The split counts: 0 = the
    library's choice, else a forced count.  out / lse: where the results go (allocated here when None)."""
    _need(q, "q", contiguous=False); _need(prefix_cache, "prefix_cache")
    B = P * G
    q_ld = q.shape[-1] if q_ld is None else q_ld
    assert prefix_cache.numel() * 2 == L.lib().obte_kv_cache_bytes(P, T_pre, H, hs)
    if suffix_cache is not None:
        _need(suffix_cache, "suffix_cache")
        assert suffix_cache.numel() * 2 == L.lib().obte_kv_cache_bytes(B, T_suf, H, hs)
    o = torch.empty((B, H * hs), dtype=bf16, device=q.device) if out is None else out
    lse = torch.empty((B, H), dtype=torch.float32, device=q.device) if lse is None else lse
    if ws is None:
        ws = torch.empty(max(int(L.lib().obte_attn_decode_shared_ws_bytes(P, G, H, hs, int(prefix_splits), int(suffix_splits))), 16), dtype=torch.uint8,
                         device=q.device)
    L.check(L.lib().obte_attn_decode_shared(_ptr(q), q_ld, _ptr(prefix_cache), P, T_pre, int(n_prefix), _ptr(suffix_cache), G, T_suf, int(n_suffix), _ptr(o),
                                            _ptr(lse), H, hs, float(scale), int(prefix_splits), int(suffix_splits), _ptr(ws), ws.numel(), _stream()),
            "obte_attn_decode_shared")
    return o, lse


def block_decode_shared_workspace(P, G, Cc, H, device) -> torch.Tensor:
    nbytes = int(L.lib().obte_block_decode_shared_ws_bytes(P, G, Cc, H))
    if nbytes <= 0:
        raise RuntimeError(f"block_decode_shared: unsupported shape (P {P}, G {G}, n_embd {Cc}, n_head {H}): head size 64 or 128, "
                           "n_embd a multiple of 64 and <= 4096, P * G * n_head <= 65535")
    return torch.empty(nbytes, dtype=torch.uint8, device=device)


def block_decode_shared(x, params, rope, H, prefix_cache, P, T_pre, n_prefix, suffix_cache, T_suf, suf_pos, ws=None, out=None):
    """block_decode for P groups of G = B / P rows over a shared prefix (obte_block_decode_shared): x (B, C) -> y (B, C).  Every row's new
    token stands at absolute position n_prefix + suf_pos and joins slot suf_pos of its row of the suffix cache; it attends over
    positions [0, n_prefix) of its group's row of the prefix cache and its own slots [0, suf_pos].  rope: the FULL tables (at least
    n_prefix + suf_pos + 1 rows).  out may be x itself."""
    _need(prefix_cache, "prefix_cache")
    B, Cc = x.shape
    if P < 1 or B % P:
        raise ValueError(f"block_decode_shared: {B} rows are not P = {P} groups of equal size")
    assert prefix_cache.numel() * 2 == L.lib().obte_kv_cache_bytes(P, T_pre, H, Cc // H)
    return _block_call(x, params, rope, H, ws, out, lambda B_, T_, C_, H_, dev: block_decode_shared_workspace(P, B_ // P, C_, H_, dev), lambda d, y, w: L.check(
        L.lib().obte_block_decode_shared(d, _ptr(x), _ptr(y), _ptr(prefix_cache), P, T_pre, int(n_prefix), _ptr(suffix_cache), T_suf, int(suf_pos), _ptr(w),
                                         w.numel(), _stream()), "obte_block_decode_shared"),
        cache=suffix_cache, T_max=T_suf, at=n_prefix + suf_pos, one=True)


# ---- beam search: the selection, and the shared-prefix step through an ancestry table (include/omnibiote_hip_beam.h) ----
BEAM_MAX_WIDTH = L.BEAM_MAX_WIDTH


def beam_select_workspace(P, W, device) -> torch.Tensor:
    nbytes = int(L.lib().obte_beam_select_ws_bytes(P, W))
    if nbytes <= 0:
        raise RuntimeError(f"beam_select: unsupported shape (P {P}, W {W}): P >= 1, 1 <= W <= {BEAM_MAX_WIDTH}")
    return torch.empty(nbytes, dtype=torch.uint8, device=device)


def beam_select(logits, score, done, ancestry_in, ancestry_out, token_hist, slot, W, eos_token=None, allowed_packed=None, parent=None, token=None,
                score_out=None, done_out=None, ws=None):
    """One beam step for the P = B / W groups of ``logits`` (B, V) bf16, row b = p * W + g (obte_beam_select_bf16; the rule:
    include/omnibiote_hip_beam.h, restated in float64 by sampling.beam_step_reference): per group the W best of the W * V candidates
    ``score[b] + log_softmax(logits[b])[v]``, equal scores to the lower beam and then the lower token, in two launches and one read of the
    logits.  ``score`` (B,) fp32, ``done`` (B,) uint8, ``ancestry_in`` / ``ancestry_out`` (B, T_suf) int32 (two buffers), ``token_hist``
    (T_suf, B) int64, ``slot`` the suffix slot the chosen tokens will occupy.  ``allowed_packed``: uint8 (n,) or (B, n), n >= ceil(V / 8),
    as ``pack_token_mask`` makes it.  ``score_out`` / ``done_out`` may be ``score`` / ``done`` themselves.  Returns (parent (B,) int32,
    token (B,) int64, score_out, done_out); ancestry_out[:, :slot + 1] and token_hist[slot] are written."""
    _need(logits, "logits", contiguous=False)
    if logits.dim() != 2 or logits.stride(1) != 1 and logits.shape[1] > 1:
        raise ValueError(f"beam_select: logits must be (B, V) with last-dimension stride 1, got {tuple(logits.shape)} strides {logits.stride()}")
    B, V = logits.shape
    if W < 1 or B % W:
        raise ValueError(f"beam_select: {B} rows are not groups of W = {W}")
    dev = logits.device
    _need(score, "score", torch.float32); _need(done, "done", torch.uint8)
    _need(ancestry_in, "ancestry_in", torch.int32); _need(ancestry_out, "ancestry_out", torch.int32); _need(token_hist, "token_hist", torch.int64)
    T_suf = ancestry_in.shape[1]
    if ancestry_in.shape != (B, T_suf) or ancestry_out.shape != (B, T_suf) or token_hist.shape != (T_suf, B) or score.shape != (B,) or done.shape != (B,):
        raise ValueError(f"beam_select: score, done ({B},), ancestry_in, ancestry_out ({B}, T_suf) and token_hist (T_suf, {B}) do not fit")
    ld_mask = 0
    if allowed_packed is not None:
        _need(allowed_packed, "allowed_packed", torch.uint8, contiguous=False)
        nb = (V + 7) // 8
        if allowed_packed.dim() == 2 and allowed_packed.shape[0] == B and allowed_packed.shape[1] >= nb and allowed_packed.stride(1) == 1:
            ld_mask = allowed_packed.stride(0)
        elif not (allowed_packed.dim() == 1 and allowed_packed.shape[0] >= nb and allowed_packed.stride(0) == 1):
            raise ValueError(f"beam_select: allowed_packed must be uint8 (n,) or ({B}, n) with n >= {nb}, got {tuple(allowed_packed.shape)}")
    parent = torch.empty(B, dtype=torch.int32, device=dev) if parent is None else parent
    token = torch.empty(B, dtype=torch.int64, device=dev) if token is None else token
    score_out = torch.empty(B, dtype=torch.float32, device=dev) if score_out is None else score_out
    done_out = torch.empty(B, dtype=torch.uint8, device=dev) if done_out is None else done_out
    if ws is None:
        ws = beam_select_workspace(B // W, W, dev)
    L.check(L.lib().obte_beam_select_bf16(_ptr(logits), logits.stride(0), B // W, W, V, _ptr(score), _ptr(done),
                                          -1 if eos_token is None else int(eos_token), _ptr(allowed_packed), ld_mask, _ptr(ancestry_in), T_suf, int(slot),
                                          _ptr(parent), _ptr(token), _ptr(score_out), _ptr(done_out), _ptr(ancestry_out), _ptr(token_hist), _ptr(ws), ws.numel(),
                                          _stream()), "obte_beam_select_bf16")
    return parent, token, score_out, done_out


def attn_decode_beam(q, prefix_cache, P, T_pre, n_prefix, suffix_cache, G, T_suf, n_suffix, ancestry, H, hs, scale, prefix_splits=0, suffix_splits=0, q_ld=None,
                     ws=None, out=None, lse=None):
    """``attn_decode_shared`` with the suffix slots read through ``ancestry`` (B, T_suf) int32 (obte_attn_decode_beam): slot j of row
    b = p * G + g comes from suffix-cache row p * G + ancestry[b, j]; an entry outside [0, G) is a key that is not there.  The identity
    table gives attn_decode_shared's bits; a valid table those of attn_decode_shared on the suffix cache gathered by it."""
    _need(q, "q", contiguous=False); _need(prefix_cache, "prefix_cache")
    B = P * G
    q_ld = q.shape[-1] if q_ld is None else q_ld
    assert prefix_cache.numel() * 2 == L.lib().obte_kv_cache_bytes(P, T_pre, H, hs)
    if suffix_cache is not None:
        _need(suffix_cache, "suffix_cache")
        assert suffix_cache.numel() * 2 == L.lib().obte_kv_cache_bytes(B, T_suf, H, hs)
    if ancestry is not None:
        _need(ancestry, "ancestry", torch.int32)
        assert ancestry.shape == (B, T_suf)
    o = torch.empty((B, H * hs), dtype=bf16, device=q.device) if out is None else out
    lse = torch.empty((B, H), dtype=torch.float32, device=q.device) if lse is None else lse
    if ws is None:
        ws = torch.empty(max(int(L.lib().obte_attn_decode_shared_ws_bytes(P, G, H, hs, int(prefix_splits), int(suffix_splits))), 16), dtype=torch.uint8,
                         device=q.device)
    L.check(L.lib().obte_attn_decode_beam(_ptr(q), q_ld, _ptr(prefix_cache), P, T_pre, int(n_prefix), _ptr(suffix_cache), G, T_suf, int(n_suffix), _ptr(ancestry),
                                          _ptr(o), _ptr(lse), H, hs, float(scale), int(prefix_splits), int(suffix_splits), _ptr(ws), ws.numel(), _stream()),
            "obte_attn_decode_beam")
    return o, lse


def block_decode_beam_workspace(P, G, Cc, H, device) -> torch.Tensor:
    nbytes = int(L.lib().obte_block_decode_beam_ws_bytes(P, G, Cc, H))
    if nbytes <= 0:
        raise RuntimeError(f"block_decode_beam: unsupported shape (P {P}, G {G}, n_embd {Cc}, n_head {H}): head size 64 or 128, "
                           "n_embd a multiple of 64 and <= 4096, P * G * n_head <= 65535")
    return torch.empty(nbytes, dtype=torch.uint8, device=device)


def block_decode_beam(x, params, rope, H, prefix_cache, P, T_pre, n_prefix, suffix_cache, T_suf, suf_pos, ancestry, ws=None, out=None):
    """``block_decode_shared`` with the suffix slots [0, suf_pos] read through ``ancestry`` (B, T_suf) int32 (obte_block_decode_beam).  Row b
    stores its new key and value at (row b, slot suf_pos); ancestry[b, suf_pos] must already be b % G (``beam_select`` at that slot wrote it)."""
    _need(prefix_cache, "prefix_cache"); _need(ancestry, "ancestry", torch.int32)
    B, Cc = x.shape
    if P < 1 or B % P:
        raise ValueError(f"block_decode_beam: {B} rows are not P = {P} groups of equal size")
    assert prefix_cache.numel() * 2 == L.lib().obte_kv_cache_bytes(P, T_pre, H, Cc // H) and ancestry.shape == (B, T_suf)
    return _block_call(x, params, rope, H, ws, out, lambda B_, T_, C_, H_, dev: block_decode_beam_workspace(P, B_ // P, C_, H_, dev), lambda d, y, w: L.check(
        L.lib().obte_block_decode_beam(d, _ptr(x), _ptr(y), _ptr(prefix_cache), P, T_pre, int(n_prefix), _ptr(suffix_cache), T_suf, int(suf_pos), _ptr(ancestry),
                                       _ptr(w), w.numel(), _stream()), "obte_block_decode_beam"),
        cache=suffix_cache, T_max=T_suf, at=n_prefix + suf_pos, one=True)


# ---- the key/value cache in pages: one pool for rows of any lengths (include/omnibiote_hip_paged.h; the format in plain torch: paged.py) ----
KV_PAGE = L.KV_PAGE


def kv_paged_buffer(n_pages, H, hs, device) -> torch.Tensor:
    """One layer's pool of ``n_pages`` pages (K [n_pages, H, 64, hs], then V, bf16) as the flat bf16 tensor the entry points take."""
    nbytes = int(L.lib().obte_kv_paged_bytes(n_pages, H, hs))
    if nbytes <= 0:
        raise RuntimeError(f"kv_paged_buffer: unsupported shape (n_pages {n_pages}, n_head {H}, head size {hs}): head size 64 or 128")
    return torch.empty(nbytes // 2, dtype=bf16, device=device)


def _need_paged(pool, table, B, n_pages, H, hs, e4m3=False):
    """the pool (bf16; e4m3: the uint8 pool of include/omnibiote_hip_paged8.h) and the (B, table_ld) int32 table of a paged call; returns table_ld"""
    _need(pool, "pool", torch.uint8 if e4m3 else bf16); _need(table, "table", torch.int32)
    if table.dim() != 2 or table.shape[0] != B:
        raise ValueError(f"table: expected shape ({B}, table_ld), got {tuple(table.shape)}")
    if e4m3:
        assert pool.numel() == L.lib().obte_kv8_paged_bytes(n_pages, H, hs)
    else:
        assert pool.numel() * 2 == L.lib().obte_kv_paged_bytes(n_pages, H, hs)
    return table.shape[1]


def kv_paged_store(qkv, B, t, H, hs, pool, n_pages, table):
    """Copy the k and v thirds of the packed, rotated qkv [B*t, 3C] into positions [0, t) of each row, through the page table
    (obte_kv_paged_store); a position whose table entry is no page of the pool is skipped.  table: int32 (B, table_ld) on the device."""
    _need(qkv, "qkv")
    ld = _need_paged(pool, table, B, n_pages, H, hs)
    assert qkv.numel() == B * t * 3 * H * hs and t <= KV_PAGE * ld
    L.check(L.lib().obte_kv_paged_store(_ptr(qkv), B, t, H, hs, _ptr(pool), n_pages, _ptr(table), ld, _stream()), "obte_kv_paged_store")
    return pool


def kv_paged_rope_store_rows(qkv, rope, pos, max_pos, B, H, hs, pool, n_pages, table):
    """kv_cache_rope_store_rows into pages (obte_kv_paged_rope_store_rows): the same rotation of qkv in place, the rotated k and the v to
    slot pos[b] % 64 of page table[b, pos[b] // 64] — or nowhere, if that is no page of the pool."""
    _need(qkv, "qkv"); _need_rows(pos, "pos", B)
    ld = _need_paged(pool, table, B, n_pages, H, hs)
    _need(rope[0], "rope_cos", torch.float32); _need(rope[1], "rope_sin", torch.float32)
    assert qkv.numel() == B * 3 * H * hs and max_pos < KV_PAGE * ld
    assert rope[0].shape[0] > max_pos and rope[1].shape[0] > max_pos
    L.check(L.lib().obte_kv_paged_rope_store_rows(_ptr(qkv), _ptr(rope[0]), _ptr(rope[1]), _ptr(pos), int(max_pos), B, H, hs, _ptr(pool), n_pages, _ptr(table),
                                                  ld, _stream()), "obte_kv_paged_rope_store_rows")
    return qkv


def attn_decode_paged(q, pool, n_pages, table, B, n_keys, max_keys, H, hs, scale, splits=0, q_ld=None, ws=None):
    """attn_decode_rows over pages (obte_attn_decode_paged): row b over its positions [0, n_keys[b]) that have a page, read through
    table (B, table_ld) int32; bit for bit attn_decode_rows on a rectangular cache holding the same vectors.  Returns (o, lse)."""
    _need(q, "q"); _need_rows(n_keys, "n_keys", B)
    ld = _need_paged(pool, table, B, n_pages, H, hs)
    q_ld = q.shape[-1] if q_ld is None else q_ld
    assert q.numel() >= (B - 1) * q_ld + H * hs and max_keys <= KV_PAGE * ld
    o = torch.empty((B, H * hs), dtype=bf16, device=q.device)
    lse = torch.empty((B, H), dtype=torch.float32, device=q.device)
    if ws is None:
        ws = torch.empty(int(L.lib().obte_attn_decode_ws_bytes(B, H, hs)), dtype=torch.uint8, device=q.device)
    L.check(L.lib().obte_attn_decode_paged(_ptr(q), q_ld, _ptr(pool), n_pages, _ptr(table), ld, _ptr(o), _ptr(lse), B, _ptr(n_keys), int(max_keys), H, hs,
                                           float(scale), int(splits), _ptr(ws), ws.numel(), _stream()), "obte_attn_decode_paged")
    return o, lse


def block_prefill_paged(x, params, rope, H, mask: MaskSpec, pool, n_pages, table, ws=None, out=None):
    """block_prefill into pages (obte_block_fwd_prefill_paged): y bit for bit block_infer's, the same workspace; the rotated keys and the
    values of positions [0, T) of row b go to the pages of table row b, int32 (B, table_ld) — any rows of a larger table, gathered."""
    B, T, Cc = x.shape
    ld = _need_paged(pool, table, B, n_pages, H, Cc // H)
    assert T <= KV_PAGE * ld
    return _block_call(x, params, rope, H, ws, out, block_infer_workspace, lambda d, y, w: L.check(
        L.lib().obte_block_fwd_prefill_paged(d, _ptr(x), _ptr(y), _ptr(w), w.numel(), _ptr(pool), n_pages, _ptr(table), ld, _stream()),
        "obte_block_fwd_prefill_paged"), mask)


def block_decode_paged(x, params, rope, H, pool, n_pages, table, pos, max_pos, ws=None, out=None):
    """block_decode_rows on pages (obte_block_decode_paged): row b at position pos[b], stored to and read from the pages of table row b.
    The workspace is block_decode's.  rope: the FULL tables.  out may be x itself."""
    B, Cc = x.shape
    ld = _need_paged(pool, table, B, n_pages, H, Cc // H)
    assert max_pos < KV_PAGE * ld
    return _block_call(x, params, rope, H, ws, out, _decode_ws, lambda d, y, w: L.check(
        L.lib().obte_block_decode_paged(d, _ptr(x), _ptr(y), _ptr(pool), n_pages, _ptr(table), ld, _ptr(pos), int(max_pos), _ptr(w), w.numel(), _stream()),
        "obte_block_decode_paged"), rows=(pos, "pos"), at=max_pos, one=True)


# ---- several new positions per row against the pages of a bf16 pool (include/omnibiote_hip_paged_extend.h) ----
def kv_paged_rope_store_chunk(qkv, rope, pos, max_pos, B, n, H, hs, pool, n_pages, table):
    """kv_cache_rope_store_chunk into pages (obte_kv_paged_rope_store_chunk): the same rotation of the packed qkv [B * n, 3C] in place, the
    rotated k and the v of row b * n + j to slot (pos[b] + j) % 64 of page table[b, (pos[b] + j) // 64] — or nowhere, if that is no page
    of the pool.  pos: int32 (B,) on the device; a row whose value lies outside [0, max_pos] is left alone."""
    _need(qkv, "qkv"); _need_rows(pos, "pos", B)
    ld = _need_paged(pool, table, B, n_pages, H, hs)
    _need(rope[0], "rope_cos", torch.float32); _need(rope[1], "rope_sin", torch.float32)
    assert qkv.numel() == B * n * 3 * H * hs and max_pos + n <= KV_PAGE * ld
    assert rope[0].shape[0] >= max_pos + n and rope[1].shape[0] >= max_pos + n
    L.check(L.lib().obte_kv_paged_rope_store_chunk(_ptr(qkv), _ptr(rope[0]), _ptr(rope[1]), _ptr(pos), int(max_pos), B, n, H, hs, _ptr(pool), n_pages,
                                                   _ptr(table), ld, _stream()), "obte_kv_paged_rope_store_chunk")
    return qkv


def attn_extend_paged(q, pool, n_pages, table, B, n, pos, H, hs, scale, pos_rows, splits=0, q_ld=None, ws=None, out=None, lse=None):
    """attn_extend's rows form over pages (obte_attn_extend_paged): n queries per (b, h) at positions pos_rows[b] .. pos_rows[b] + n - 1,
    query j over the positions [0, pos_rows[b] + j + 1) of row b that have a page, read through table (B, table_ld) int32; bit for bit
    attn_extend(pos_rows=) on a rectangular cache holding the same vectors.  pos: the host's bound on pos_rows (a row outside [0, pos]
    gives zeros and lse = -inf), pos + n <= 64 * table_ld.  Returns (o (B * n, C) bf16, lse (B, H, n) fp32)."""
    _need(q, "q", contiguous=False); _need_rows(pos_rows, "pos_rows", B)
    ld = _need_paged(pool, table, B, n_pages, H, hs)
    q_ld = q.shape[-1] if q_ld is None else q_ld
    assert n >= 1 and pos + n <= KV_PAGE * ld
    o = torch.empty((B * n, H * hs), dtype=bf16, device=q.device) if out is None else out
    lse = torch.empty((B, H, n), dtype=torch.float32, device=q.device) if lse is None else lse
    if ws is None:
        ws = torch.empty(max(int(L.lib().obte_attn_extend_ws_bytes(B, H, hs, n, int(splits))), 16), dtype=torch.uint8, device=q.device)
    L.check(L.lib().obte_attn_extend_paged(_ptr(q), q_ld, _ptr(pool), n_pages, _ptr(table), ld, _ptr(o), _ptr(lse), B, n, int(pos), _ptr(pos_rows), H, hs,
                                           float(scale), int(splits), _ptr(ws), ws.numel(), _stream()), "obte_attn_extend_paged")
    return o, lse


def block_extend_paged(x, params, rope, H, pool, n_pages, table, pos, pos_rows, ws=None, out=None):
    """block_extend's rows form on pages (obte_block_extend_paged): x (B, n, C) -> y (B, n, C), row b's positions from pos_rows[b] on
    (int32 (B,) on the device; pos the host's bound on it, pos + n <= 64 * table_ld), stored to and read from the pages of table row b.
    The workspace is block_extend's.  rope: the FULL tables (at least pos + n rows).  out may be x itself."""
    B, n, Cc = x.shape
    ld = _need_paged(pool, table, B, n_pages, H, Cc // H)
    assert pos + n <= KV_PAGE * ld
    return _block_call(x, params, rope, H, ws, out, block_extend_workspace, lambda d, y, w: L.check(
        L.lib().obte_block_extend_paged(d, _ptr(x), _ptr(y), _ptr(pool), n_pages, _ptr(table), ld, int(pos), _ptr(pos_rows), _ptr(w), w.numel(), _stream()),
        "obte_block_extend_paged"), rows=(pos_rows, "pos_rows"), at=pos)


# ---- the pages as OCP e4m3 (include/omnibiote_hip_paged8.h; the format in plain torch: paged.py, the quantiser: kvquant.py) ----
def kv8_paged_buffer(n_pages, H, hs, device) -> torch.Tensor:
    """One layer's e4m3 pool of ``n_pages`` pages (K codes [n_pages, H, 64, hs], V codes, K scales fp32 [n_pages, H, 64], V scales) as the
    flat uint8 tensor the entry points take: 2 (hs + 4) bytes per cached head vector against the bf16 pool's 4 hs."""
    nbytes = int(L.lib().obte_kv8_paged_bytes(n_pages, H, hs))
    if nbytes <= 0:
        raise RuntimeError(f"kv8_paged_buffer: unsupported shape (n_pages {n_pages}, n_head {H}, head size {hs}): head size 64 or 128")
    return torch.empty(nbytes, dtype=torch.uint8, device=device)


def kv8_paged_store(qkv, B, t, H, hs, pool, n_pages, table):
    """kv_paged_store into an e4m3 pool (obte_kv8_paged_store): the k and v thirds of the packed, rotated qkv [B*t, 3C], quantised per head
    vector as kv8_cache_store quantises them, into positions [0, t) of each row through the page table; a position without a page is skipped."""
    _need(qkv, "qkv")
    ld = _need_paged(pool, table, B, n_pages, H, hs, e4m3=True)
    assert qkv.numel() == B * t * 3 * H * hs and t <= KV_PAGE * ld
    L.check(L.lib().obte_kv8_paged_store(_ptr(qkv), B, t, H, hs, _ptr(pool), n_pages, _ptr(table), ld, _stream()), "obte_kv8_paged_store")
    return pool


def kv8_paged_rope_store_rows(qkv, rope, pos, max_pos, B, H, hs, pool, n_pages, table):
    """kv_paged_rope_store_rows into an e4m3 pool (obte_kv8_paged_rope_store_rows): qkv is left with the same bits, kv8_cache_rope_store_rows's
    codes and scales go to slot pos[b] % 64 of page table[b, pos[b] // 64] — or nowhere, if that is no page of the pool."""
    _need(qkv, "qkv"); _need_rows(pos, "pos", B)
    ld = _need_paged(pool, table, B, n_pages, H, hs, e4m3=True)
    _need(rope[0], "rope_cos", torch.float32); _need(rope[1], "rope_sin", torch.float32)
    assert qkv.numel() == B * 3 * H * hs and max_pos < KV_PAGE * ld
    assert rope[0].shape[0] > max_pos and rope[1].shape[0] > max_pos
    L.check(L.lib().obte_kv8_paged_rope_store_rows(_ptr(qkv), _ptr(rope[0]), _ptr(rope[1]), _ptr(pos), int(max_pos), B, H, hs, _ptr(pool), n_pages, _ptr(table),
                                                   ld, _stream()), "obte_kv8_paged_rope_store_rows")
    return qkv


def attn_decode_paged8(q, pool, n_pages, table, B, n_keys, max_keys, H, hs, scale, splits=0, q_ld=None, ws=None, out=None, lse=None):
    """attn_decode_paged over an e4m3 pool (obte_attn_decode_paged8): bit for bit attn_decode_kv8(n_keys_rows=) on a rectangular e4m3 cache
    holding the same codes and scales.  q_ld, ws, out and lse as in attn_decode_kv8.  Returns (o, lse)."""
    _need(q, "q", contiguous=False); _need_rows(n_keys, "n_keys", B)
    ld = _need_paged(pool, table, B, n_pages, H, hs, e4m3=True)
    q_ld = q.shape[-1] if q_ld is None else q_ld
    assert (not q.is_contiguous() or q.numel() >= (B - 1) * q_ld + H * hs) and max_keys <= KV_PAGE * ld
    o = torch.empty((B, H * hs), dtype=bf16, device=q.device) if out is None else out
    lse = torch.empty((B, H), dtype=torch.float32, device=q.device) if lse is None else lse
    if ws is None:
        ws = torch.empty(int(L.lib().obte_attn_decode_ws_bytes(B, H, hs)), dtype=torch.uint8, device=q.device)
    L.check(L.lib().obte_attn_decode_paged8(_ptr(q), q_ld, _ptr(pool), n_pages, _ptr(table), ld, _ptr(o), _ptr(lse), B, _ptr(n_keys), int(max_keys), H, hs,
                                            float(scale), int(splits), _ptr(ws), ws.numel(), _stream()), "obte_attn_decode_paged8")
    return o, lse


def block_prefill_paged8(x, params, rope, H, mask: MaskSpec, pool, n_pages, table, ws=None, out=None):
    """block_prefill_paged into an e4m3 pool (obte_block_fwd_prefill_paged8): y bit for bit block_infer's, the rotated keys and the values
    quantised into the pages of table row b."""
    B, T, Cc = x.shape
    ld = _need_paged(pool, table, B, n_pages, H, Cc // H, e4m3=True)
    assert T <= KV_PAGE * ld
    return _block_call(x, params, rope, H, ws, out, block_infer_workspace, lambda d, y, w: L.check(
        L.lib().obte_block_fwd_prefill_paged8(d, _ptr(x), _ptr(y), _ptr(w), w.numel(), _ptr(pool), n_pages, _ptr(table), ld, _stream()),
        "obte_block_fwd_prefill_paged8"), mask)


def block_decode_paged8(x, params, rope, H, pool, n_pages, table, pos, max_pos, ws=None, out=None):
    """block_decode_paged on an e4m3 pool (obte_block_decode_paged8): y bit for bit block_decode_kv8's rows form on a rectangular e4m3 cache
    holding the same vectors.  The workspace is block_decode's.  rope: the FULL tables.  out may be x itself."""
    B, Cc = x.shape
    ld = _need_paged(pool, table, B, n_pages, H, Cc // H, e4m3=True)
    assert max_pos < KV_PAGE * ld
    return _block_call(x, params, rope, H, ws, out, _decode_ws, lambda d, y, w: L.check(
        L.lib().obte_block_decode_paged8(d, _ptr(x), _ptr(y), _ptr(pool), n_pages, _ptr(table), ld, _ptr(pos), int(max_pos), _ptr(w), w.numel(), _stream()),
        "obte_block_decode_paged8"), rows=(pos, "pos"), at=max_pos, one=True)


def block_bwd(x, dy, act, params, rope, H, mask: MaskSpec, accumulate_into=None, dropout_p=0.0, dropout_seed=0, ln_partials=None,
              ln_partial_mode=0, out_rows=None, dy_masked=None, dx_mask_seed=None, acc32=None, acc32_mode=0):
    """accumulate_into: optional list of 6 tensors-or-None (same order as params).  When the four matrix entries are all
    given, their gradients are added into those tensors in place and the corresponding returned grads are None; the
    same, independently, for the two LayerNorm weights (entries 0 and 3).
    ln_partials=(buf1, buf2) + ln_partial_mode (L.LN_PARTIAL_*): the two LayerNorm weight gradients are accumulated over
    calls in those fp32 buffers instead (see layernorm_bwd); their returned grads are None except with LN_PARTIAL_LAST.
    Dropout hand-off between blocks (include/omnibiote_hip.h, obte_block_desc::dy_masked): dy_masked = dropout(dy) under THIS
    block's (seed, site 3) mask if the block above already wrote it; dx_mask_seed = the seed of the block BELOW: then
    dropout(dx) under that block's mask is written too and returned as a third value (else None).
    acc32=(attn, proj, fc, mlp) fp32 buffers of those four weights' shapes + acc32_mode (L.ACC32_*): the four matrix gradients are
    summed into them over calls, before any rounding to bf16 (include/omnibiote_hip.h, OBTE_EPI_ACC32); their returned grads are
    None for FIRST / MORE and bf16(buffer) for LAST.  The LayerNorm weights keep ln_partials."""
    _need(x, "x"); _need(dy, "dy")
    B, T, Cc = x.shape
    assert dy.numel() == (B * T if out_rows is None else out_rows.numel()) * Cc, "dy: one row per (wanted) position"
    ws = torch.empty(int(L.lib().obte_block_bwd_ws_bytes(B, T, Cc, H)), dtype=torch.uint8, device=x.device)
    dx = torch.empty_like(x)
    acc = accumulate_into is not None and all(accumulate_into[i] is not None for i in (1, 2, 4, 5))
    if acc32 is not None or acc32_mode:
        assert not acc, "acc32 replaces accumulate_into for the four matrices"
        assert acc32 is not None and len(acc32) == 4
        for t, i in zip(acc32, (1, 2, 4, 5)):
            _check_acc32(t, acc32_mode, params[i].shape)
    w32_none = acc32_mode in (L.ACC32_FIRST, L.ACC32_MORE)
    acc_ln = (not ln_partial_mode) and accumulate_into is not None and all(accumulate_into[i] is not None for i in (0, 3))
    if ln_partial_mode:
        for t in ln_partials:
            _need(t, "ln_partials", torch.float32)
            assert t.numel() == L.lib().obte_layernorm_bwd_ws_rows() * Cc
    grads = []
    for i, w in enumerate(params):
        if (acc and i in (1, 2, 4, 5)) or (acc_ln and i in (0, 3)):
            g = accumulate_into[i]
            _need(g, "grad"); assert g.shape == w.shape
            grads.append(g)
        elif w32_none and i in (1, 2, 4, 5):
            grads.append(None)        # (not written before the last pass)
        else:
            grads.append(torch.empty_like(w))
    dx_masked = torch.empty_like(x) if (dx_mask_seed is not None and dropout_p > 0.0) else None
    if dy_masked is not None:
        _need(dy_masked, "dy_masked"); assert dy_masked.numel() == dy.numel() and dropout_p > 0.0
    d = _block_desc(B, T, Cc, H, params, rope, mask, dropout_p, dropout_seed, ln_partials, ln_partial_mode, out_rows=out_rows,
                    dy_masked=dy_masked, dx_masked=dx_masked, dx_mask_seed=dx_mask_seed or 0, acc32=acc32, acc32_mode=acc32_mode)
    L.check(L.lib().obte_block_bwd_acc(C.byref(d), _ptr(x), _ptr(dy), _ptr(act), _ptr(ws), _ptr(dx), *[_ptr(g) for g in grads],
                                        int(acc) + 2 * int(acc_ln), _stream()), "obte_block_bwd")
    ln_none = ln_partial_mode in (L.LN_PARTIAL_FIRST, L.LN_PARTIAL_MORE)
    grads = [None if (((acc or w32_none) and i in (1, 2, 4, 5)) or ((acc_ln or ln_none) and i in (0, 3))) else g for i, g in enumerate(grads)]
    if dx_mask_seed is not None:
        return dx, grads, dx_masked
    return dx, grads
