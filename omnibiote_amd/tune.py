"""GEMM plan tuner: measure, don't guess.

The library holds two GEMM structures and several tile/split choices (include/omnibiote_hip.h, "Tuned plans").
Which one is fastest for a shape depends on tile quantisation against 256 CUs, on K, and on where the operands
are served from — the measured spread on the small config is up to 2x per shape.  ``tune_model_shapes`` times every
candidate once per GEMM shape of the training step on the actual device (HIP events on the launch stream, random
data) and records the winner in the library's plan table; it is called once at start-up (bench.py, the harness).
"""
from __future__ import annotations

from typing import Dict, Iterable, List, Tuple

import torch

from . import _lib as L
from . import ops

_done: Dict[tuple, tuple] = {}


_flush = {}


def _flush_caches(device) -> None:
    """Write 512 MiB: the operands of the next timed launch then come from HBM, as they do inside a training step (the
    256-MiB Infinity Cache would otherwise serve every repetition of a shape whose tensors fit it, and the plan picked on
    those timings is not always the one that is fastest cold)."""
    import os
    if os.environ.get("OBTE_TUNE_WARM") == "1":
        return
    buf = _flush.get(str(device))
    if buf is None:
        buf = torch.empty(512 << 20, dtype=torch.uint8, device=device)
        _flush[str(device)] = buf
    buf.zero_()


def _time_once(a, b, M, N, K, ak, bk, epi, aux, out, reps=6, rope=None) -> float:
    ops.gemm(a, b, M, N, K, ak, bk, epi, aux, out=out, rope=rope)
    torch.cuda.synchronize()
    best = float("inf")
    for _ in range(reps):
        _flush_caches(a.device)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        ops.gemm(a, b, M, N, K, ak, bk, epi, aux, out=out, rope=rope)
        e1.record()
        e1.synchronize()
        best = min(best, e0.elapsed_time(e1))
    return best


def v7_applies(M: int, N: int, K: int, epi: int, a_kmajor: bool, b_kmajor: bool) -> bool:
    """Mirror of structure 7's rule (csrc/gemm.cpp runs_as_given, csrc/gemm_common.h gemm_has_form): whole 256 x 256 tiles, one or more per CU, K >= 256, x W^T or dy W
    with the epilogues it is built for, an output that stays within the Infinity Cache."""
    if not a_kmajor:
        return False
    ok_epi = (L.EPI_NONE, L.EPI_GELU, L.EPI_ADD, L.EPI_ADD_DROPOUT, L.EPI_ROPE_QK) if b_kmajor else (L.EPI_NONE, L.EPI_GELU_BWD)
    return (epi in ok_epi and M % 256 == 0 and N % 256 == 0 and K % 64 == 0 and K >= 256 and (M // 256) * (N // 256) >= 256
            and M * N * 2 <= (256 << 20))


def candidates(M: int, N: int, K: int, epi: int, a_kmajor: bool = False, b_kmajor: bool = False) -> List[Tuple[int, int, int]]:
    """(variant, bn, splits)."""
    c = [(1, 128, 1), (2, 128, 1)]
    if a_kmajor and b_kmajor and N % 192 == 0 and epi != L.EPI_GELU_BWD:
        c.append((2, 192, 1))      # 256 x 192 tiles: full rounds where N / 256 leaves a ragged one (c_attn: 3072 -> 512 tiles)
    if v7_applies(M, N, K, epi, a_kmajor, b_kmajor):
        c.append((7, 256, 1))      # the 256 x 256 half-tile ring, persistent: the LDS-DMA stream runs on across tiles (csrc/gemm_bf16_v7.hip)
    if K >= 128:
        c.append((4, 128, 1))      # the half-tile ring at two workgroups per CU
    if N >= 256:
        c.append((2, 256, 1))
        if K >= 128:
            c.append((3, 256, 1))
    nk = (K + 63) // 64
    if epi in (L.EPI_NONE, L.EPI_ADD) and M * N * 4 * 8 <= (1 << 28):   # split-K only for small outputs (weight gradients, the rows form's projections)
        for bn in (128, 256):
            if bn == 256 and N < 256:
                continue
            tiles = ((M + 255) // 256) * ((N + bn - 1) // bn)
            for s in (2, 3, 4, 5, 6, 8, 10, 12, 16):
                if nk // s >= 8 and tiles * s <= 1024:
                    c.append((2, bn, s))
                    c.append((3, bn, s) if bn == 256 else (4, bn, s))
    return c


def rank_candidates(times: dict) -> list:
    """{(variant, bn, splits): ms} -> [(ms, variant, bn, splits), ...], the plan to use first.  Candidates within 3 % of the
    fastest are a tie at this protocol's resolution (cold operands, three repetitions): the structure with the deeper ring
    goes first — inside the step, with warm operands and neighbours, it is the one that holds its time (the row-compact readout
    input gradient: 160-195 us on the half-tile ring against 190-215 us when the K-tile ring won the coin toss)."""
    results = sorted((t, c[0], c[1], c[2]) for c, t in times.items())
    prefer = {7: 0, 3: 1, 2: 2, 4: 3, 1: 4}
    tied = [r for r in results if r[0] <= results[0][0] * 1.03]
    tied.sort(key=lambda r: (prefer.get(r[1], 9), r[0]))
    return tied[:1] + [r for r in results if r is not tied[0]]


def tune_gemm(M: int, N: int, K: int, a_kmajor: bool, b_kmajor: bool, epi: int = L.EPI_NONE, device="cuda", verbose=False):
    key = (M, N, K, a_kmajor, b_kmajor, epi)
    if key in _done:
        return _done[key]
    lib = L.lib()
    g = torch.Generator(device=device).manual_seed(0)
    a = torch.randn(M * K, device=device, generator=g).to(torch.bfloat16)
    b = torch.randn(N * K, device=device, generator=g).to(torch.bfloat16)
    aux = torch.randn(M * N, device=device, generator=g).to(torch.bfloat16) if epi in (L.EPI_ADD, L.EPI_GELU_BWD) else None
    out = torch.empty(M * N, device=device, dtype=torch.bfloat16)
    rope = None
    if epi == L.EPI_ROPE_QK:   # the c_attn projection is timed WITH its RoPE epilogue (tables of a plausible shape: the cost is the same)
        hs = 128 if (N // 3) % 128 == 0 else 64
        T = min(M, 1024)
        tab = torch.randn(T, hs // 2, device=device, generator=g)
        rope = (torch.cos(tab), torch.sin(tab), T, hs)
    # round-robin over the candidates (three rounds, best time kept): the clock the chip holds drifts while it is being
    # measured, and timing the candidates one after the other hands the later ones a different machine
    cands = candidates(M, N, K, epi, a_kmajor, b_kmajor)
    best = {c: float("inf") for c in cands}
    for _ in range(3):
        for c in cands:
            variant, bn, splits = c
            L.check(lib.obte_gemm_plan_set(int(a_kmajor), int(b_kmajor), epi, M, N, K, variant, bn, splits), "obte_gemm_plan_set")
            best[c] = min(best[c], _time_once(a, b, M, N, K, a_kmajor, b_kmajor, epi, aux, out, reps=3, rope=rope))
    results = rank_candidates(best)
    t, variant, bn, splits = results[0]
    L.check(lib.obte_gemm_plan_set(int(a_kmajor), int(b_kmajor), epi, M, N, K, variant, bn, splits), "obte_gemm_plan_set")
    _done[key] = (variant, bn, splits, t)
    if verbose:
        tf = 2.0 * M * N * K / (t * 1e-3) / 1e12
        print(f"tune M={M} N={N} K={K} {'k' if a_kmajor else 'm'}{'k' if b_kmajor else 'n'} epi={epi}: "
              f"structure {variant} bn={bn} splits={splits}  {t * 1e3:.1f} us  {tf:.0f} TFLOP/s   "
              f"(others: {[(v, n, s, round(x * 1e3)) for x, v, n, s in results[1:4]]})", flush=True)
    return _done[key]


def model_gemm_shapes(rows: int, n_embd: int, vocab: int):
    """Every GEMM of one training micro-step: (M, N, K, a_kmajor, b_kmajor, epilogue)."""
    M, C, V = rows, n_embd, vocab
    Mm = max(64, int(round(0.15 * rows / 8)) * 8)
    E = L
    return [
        (M, 3 * C, C, True, True, E.EPI_ROPE_QK if C % 64 == 0 else E.EPI_NONE), (M, C, C, True, True, E.EPI_ADD), (M, 4 * C, C, True, True, E.EPI_GELU),
        (M, C, 4 * C, True, True, E.EPI_ADD), (M, V, C, True, True, E.EPI_NONE),
        (M, 4 * C, C, True, False, E.EPI_GELU_BWD), (M, C, 4 * C, True, False, E.EPI_NONE), (M, C, C, True, False, E.EPI_NONE),
        (M, C, 3 * C, True, False, E.EPI_NONE), (M, C, V, True, False, E.EPI_NONE),
        (C, 4 * C, M, False, False, E.EPI_NONE), (4 * C, C, M, False, False, E.EPI_NONE), (C, C, M, False, False, E.EPI_NONE),
        (3 * C, C, M, False, False, E.EPI_NONE), (V, C, M, False, False, E.EPI_NONE),
        # the readout over the MLM-masked rows (about 15 % of M; the library applies these plans to counts within 20 %): its
        # two backward products, and the forward of the readout that computes the masked rows only
        (Mm, C, V, True, False, E.EPI_NONE), (V, C, Mm, False, False, E.EPI_NONE), (Mm, V, C, True, True, E.EPI_NONE),
        # the last block's MLP half on those positions (model.forward(rows=...)): forward, input gradients, weight gradients
        (Mm, 4 * C, C, True, True, E.EPI_GELU), (Mm, C, 4 * C, True, True, E.EPI_ADD),
        (Mm, 4 * C, C, True, False, E.EPI_GELU_BWD), (Mm, C, 4 * C, True, False, E.EPI_NONE),
        (C, 4 * C, Mm, False, False, E.EPI_NONE), (4 * C, C, Mm, False, False, E.EPI_NONE),
        # and its attention projection on those positions (rows form without dropout: csrc/block.cpp rows_proj)
        (Mm, C, C, True, True, E.EPI_ADD), (Mm, C, C, True, False, E.EPI_NONE), (C, C, Mm, False, False, E.EPI_NONE),
        # its c_attn by output thirds (rows_qsplit): k and v of every position, q of those positions; and the three backward products
        (M, 2 * C, C, True, True, E.EPI_NONE), (Mm, C, C, True, True, E.EPI_NONE), (M, C, 2 * C, True, False, E.EPI_NONE),
        (2 * C, C, M, False, False, E.EPI_NONE),
    ]


def tune_model_shapes(rows: int, n_embd: int, vocab: int, device="cuda", verbose=False):
    for (M, N, K, ak, bk, epi) in model_gemm_shapes(rows, n_embd, vocab):
        tune_gemm(M, N, K, ak, bk, epi, device=device, verbose=verbose)
    torch.cuda.synchronize()
    _flush.clear()
    torch.cuda.empty_cache()


def export_plans() -> list:
    """The plans chosen so far as plain rows (JSON-able; also what rank 0 broadcasts to the other ranks)."""
    return [{"M": k[0], "N": k[1], "K": k[2], "a_kmajor": bool(k[3]), "b_kmajor": bool(k[4]), "epilogue": int(k[5]),
             "variant": v[0], "bn": v[1], "splits": v[2], "ms": v[3]} for k, v in sorted(_done.items())]


def save_plans(path: str) -> None:
    """Write the plans chosen so far as JSON (one object per GEMM shape) — tune once per device, reuse afterwards."""
    import json
    with open(path, "w") as f:
        json.dump(export_plans(), f, indent=1)


def load_plans(path: str) -> int:
    """Install plans written by ``save_plans`` into the library's table; returns how many.  No launches."""
    import json
    with open(path) as f:
        return import_plans(json.load(f))


REMOVED_STRUCTURES = (5, 6)   # plan files of older builds may name them: those shapes are simply tuned again


def import_plans(rows: list) -> int:
    lib = L.lib()
    rows = [r for r in rows if int(r["variant"]) not in REMOVED_STRUCTURES]
    for r in rows:
        L.check(lib.obte_gemm_plan_set(int(r["a_kmajor"]), int(r["b_kmajor"]), int(r["epilogue"]), int(r["M"]), int(r["N"]), int(r["K"]),
                                       int(r["variant"]), int(r["bn"]), int(r["splits"])), "obte_gemm_plan_set")
        _done[(int(r["M"]), int(r["N"]), int(r["K"]), bool(r["a_kmajor"]), bool(r["b_kmajor"]), int(r["epilogue"]))] = (
            int(r["variant"]), int(r["bn"]), int(r["splits"]), float(r.get("ms", 0.0)))
    return len(rows)
