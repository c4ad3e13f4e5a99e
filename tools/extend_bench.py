"""Continuing a filled key/value cache by n tokens per row in one call, on the small config (8 layers, 1024 wide, 8 heads of 128; bf16),
against what the same n tokens cost before: n decode steps.  Contenders alternate in one process over --rounds rounds after warm-up;
device events around windows of calls; median and [min - max] over the rounds.  Cache flush policy: none is flushed — every attention
call runs on the next of the model's 8 per-layer caches in turn, as a real step walks them; `served_from` says whether that set exceeds
the 256 MB Infinity Cache (only then is a share of 6.3 TB/s an HBM figure).

  (a) obte_attn_extend alone (the C entry point on preallocated buffers) at B x ctx in {1, 8, 64} x 2048 and n in {2, 4, 8, 16, 32, 64},
      the chunk ending at position ctx: the library's split count and every forced count of --sweep, against n calls of
      obte_attn_decode over ctx - n + 1 .. ctx keys; and the bytes of ONE read of the cache (2 B H ctx hs 2) over the time as a share of
      6.3 TB/s (query tiles beyond the first read the prefix again: at n = 64 the kernel reads it twice).
  (b) OmniBioTA.extend of n tokens against n decode_steps over the same positions, at --model-batches x 2048.
  (c) prefill(chunk = 256 / 512) against prefill at 8 x 2048: time, and the peak of torch.cuda.max_memory_allocated above the level
      before the call.
One JSON line per measurement.

    python tools/extend_bench.py [--parts a,b,c] [--batches 1,8,64] [--context 2048] [--chunks 2,4,8,16,32,64] [--rounds 5] [--steps 100]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from decode_bench import HBM_RATE, INFINITY_CACHE, build, summary, timed   # noqa: E402


def alternate(legs, rounds, windows):
    """legs: name -> fn; windows: name -> calls per window.  us per call, per leg, over the rounds (order reversed every other round)"""
    for fn in legs.values():
        for _ in range(3):
            fn()
    us = {k: [] for k in legs}
    for r in range(rounds):
        for leg in (list(legs) if r % 2 == 0 else list(legs)[::-1]):
            us[leg].append(timed(legs[leg], windows[leg]))
    return us


def attention_alone(m, B, ctx, chunks, sweep, rounds, steps, dev):
    from omnibiote_amd import _lib, ops
    lib, stream = _lib.lib(), torch.cuda.current_stream().cuda_stream
    H, C = m.config.n_head, m.config.n_embd
    hs = C // H
    gen = torch.Generator(device=dev).manual_seed(B)
    caches = [ops.kv_cache_buffer(B, ctx, H, hs, dev).normal_(generator=gen) for _ in m.transformer.h]
    ptrs = [kv.data_ptr() for kv in caches]
    nbytes = 2 * B * H * ctx * hs * 2
    set_bytes = nbytes * len(caches)
    dws = torch.empty(int(lib.obte_attn_decode_ws_bytes(B, H, hs)), dtype=torch.uint8, device=dev)
    for n in chunks:
        q = torch.randn(B * n, 3 * C, device=dev, generator=gen).to(torch.bfloat16)
        o = torch.empty(B * n, C, device=dev, dtype=torch.bfloat16)
        ws = torch.empty(int(lib.obte_attn_extend_ws_bytes(B, H, hs, n, _lib.ATTN_EXTEND_MAX_SPLITS)), dtype=torch.uint8, device=dev)
        pos = ctx - n
        state = {"i": 0}

        def extend(splits):
            def call():
                state["i"] += 1
                rc = lib.obte_attn_extend(q.data_ptr(), 3 * C, ptrs[state["i"] % len(ptrs)], o.data_ptr(), None, B, ctx, n, pos, None, H, hs, 8.0 / C, splits,
                                          ws.data_ptr(), ws.numel(), stream)
                if rc != 0:
                    _lib.check(rc, "obte_attn_extend")
            return call

        def decodes():          # what the same n queries cost today: one call per position (each reads row j of the first batch row's block)
            state["i"] += 1
            kv = ptrs[state["i"] % len(ptrs)]
            for j in range(n):
                rc = lib.obte_attn_decode(q.data_ptr() + j * 3 * C * 2, 3 * C, kv, o.data_ptr(), None, B, ctx, pos + j + 1, H, hs, 8.0 / C, 0, dws.data_ptr(),
                                          dws.numel(), stream)
                if rc != 0:
                    _lib.check(rc, "obte_attn_decode")
        default = int(lib.obte_attn_extend_splits(B, H, hs, n, ctx))
        counts = [0] + [s for s in sweep if s == 1 or s * 32 <= ctx]
        legs = {("default" if s == 0 else str(s)): extend(s) for s in counts}
        legs["n_decode_calls"] = decodes
        windows = {k: steps for k in legs}
        windows["n_decode_calls"] = max(3, steps // n)
        us = alternate(legs, rounds, windows)
        med = {k: statistics.median(v) for k, v in us.items()}
        best = min((k for k in med if k not in ("default", "n_decode_calls")), key=lambda k: med[k])
        print(json.dumps({"part": "a", "B": B, "context": ctx, "n": n, "default_splits": default, "cache_bytes_one_read": nbytes, "set_bytes": set_bytes,
                          "served_from": "HBM" if set_bytes > INFINITY_CACHE else "Infinity Cache (not an HBM measurement)",
                          "windows": {"calls": steps, "rounds": rounds}, "us": {k: summary(v) for k, v in us.items()},
                          "one_read_share_of_6.3TBps_default": round(nbytes / (med["default"] * 1e-6) / HBM_RATE, 3),
                          "decode_calls_over_extend_default": round(med["n_decode_calls"] / med["default"], 2),
                          "best_forced": best, "default_over_best_forced": round(med["default"] / med[best], 3)}), flush=True)
    del caches
    torch.cuda.empty_cache()


def model_tokens(m, B, ctx, chunks, rounds, steps, dev):
    from omnibiote_amd.model import KVCache
    g = torch.Generator(device=dev).manual_seed(B * 10007 + ctx)
    idx = torch.randint(4, m.config.vocab_size, (B, ctx), device=dev, generator=g)
    cache = KVCache(m, B, ctx)
    for n in chunks:
        pos = ctx - n
        m.prefill(idx[:, :pos], cache, chunk=512)
        tok = idx[:, pos:].contiguous()
        cols = [tok[:, j].contiguous() for j in range(n)]

        def extend():               # the same positions every time: the context stays ctx long
            cache.pos = pos
            m.extend(tok, cache)

        def steps_n():
            cache.pos = pos
            for j in range(n):
                m.decode_step(cols[j], cache)
        w = max(3, steps // n)
        us = alternate({"extend": extend, "n_decode_steps": steps_n}, rounds, {"extend": w, "n_decode_steps": w})
        med = {k: statistics.median(v) for k, v in us.items()}
        print(json.dumps({"part": "b", "B": B, "context": ctx, "n": n, "windows": {"calls": w, "rounds": rounds}, "us_per_call": {k: summary(v, 1) for k, v in us.items()},
                          "us_per_token": {k: round(v / n, 1) for k, v in med.items()}, "n_decode_steps_over_extend": round(med["n_decode_steps"] / med["extend"], 2)}),
              flush=True)
    del cache
    torch.cuda.empty_cache()


def chunked_prefill(m, B, ctx, rounds, dev):
    from omnibiote_amd.model import KVCache
    g = torch.Generator(device=dev).manual_seed(7)
    idx = torch.randint(4, m.config.vocab_size, (B, ctx), device=dev, generator=g)
    legs, peaks = {}, {}
    for chunk in (None, 256, 512):
        name = "prefill" if chunk is None else f"chunk_{chunk}"
        cache = KVCache(m, B, ctx)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        m.prefill(idx, cache, chunk=chunk)
        torch.cuda.synchronize()
        peaks[name] = torch.cuda.max_memory_allocated() - before
        legs[name] = (lambda c, k: lambda: m.prefill(idx, c, chunk=k))(cache, chunk)
    us = alternate(legs, rounds, {k: 5 for k in legs})
    print(json.dumps({"part": "c", "B": B, "context": ctx, "windows": {"calls": 5, "rounds": rounds}, "us_per_prefill": {k: summary(v, 0) for k, v in us.items()},
                      "peak_bytes_above_the_level_before": peaks}), flush=True)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--parts", default="a,b,c")
    p.add_argument("--batches", default="1,8,64", help="(a)")
    p.add_argument("--model-batches", default="1,8", help="(b)")
    p.add_argument("--context", type=int, default=2048)
    p.add_argument("--chunks", default="2,4,8,16,32,64")
    p.add_argument("--sweep", default="1,2,4,8,16,32", help="forced split counts for obte_attn_extend alone")
    p.add_argument("--rounds", type=int, default=5)
    p.add_argument("--steps", type=int, default=100, help="calls per timed window")
    a = p.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    parts = a.parts.split(",")
    chunks = [int(c) for c in a.chunks.split(",")]
    m = build(a.context, dev)
    if "a" in parts:
        for B in [int(b) for b in a.batches.split(",")]:
            attention_alone(m, B, a.context, chunks, [int(s) for s in a.sweep.split(",")], a.rounds, a.steps, dev)
    if "b" in parts:
        for B in [int(b) for b in a.model_batches.split(",")]:
            model_tokens(m, B, a.context, chunks, a.rounds, a.steps, dev)
    if "c" in parts:
        chunked_prefill(m, 8, a.context, a.rounds, dev)


if __name__ == "__main__":
    main()
