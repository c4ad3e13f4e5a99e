"""The paged key/value cache and continuous batching on the small config (8 layers, 1024 wide, 8 heads of 128; bf16): what the page
table costs a step, and what releasing finished rows buys a workload.  Contenders alternate in one process over --rounds rounds after
warm-up; median and [min - max] over the rounds.  One JSON line per measurement.

  attention   obte_attn_decode_paged against obte_attn_decode_rows on the same keys, the pool's pages in random order (and, as a probe of what
              the random order itself costs, in row order), every row over ctx keys, each call on the next layer's cache, at B x ctx in
              {64 x 2048, 8 x 2048}.  The paged call reads the same bytes plus one table entry per 64 keys and head.  `served_from` says
              whether a set of caches exceeds the 256 MB Infinity Cache: one that does not is not an HBM measurement.
  step        OmniBioTA.decode_step on a KVCache in rows mode and on a PagedKVCache at the same shapes, every window walking the same
              positions up to ctx - 2 (the paged step includes its host side: the page bookkeeping of every row).
  workload    --prompts prompts (default 256), lengths spread evenly over [64, 1024], in a seeded random order, up to 256 new tokens each,
              through generate_many(batch=64) and through generate(lengths=, sampler="device") over the same prompts in input-order
              batches of 64: tokens per second of wall time (a device synchronise at the end), the cache bytes each holds at its peak, and
              the share of row-steps spent on rows that had already finished.  A randomly initialised model with the 65536-token readout
              practically never draws one given token, so rows would never end: the workload's model has --vocab tokens (default 256),
              where every draw meets the eos_token with a probability near 1 / vocab and the rows end at spread-out times.  Also with a
              pool of --pool-share (default 0.65) of the default page count.

  --kv8       the e4m3 pool (include/omnibiote_hip_paged8.h) in the same three parts, under the same protocol:
              attention   obte_attn_decode_paged8 (pages in random order, and in row order) against obte_attn_decode_kv8's rows form on a
                          rectangle holding the same codes and scales, and in the same process the bf16 pair above and paged e4m3 against
                          paged bf16 (the byte ratio is (hs + 4) / (2 hs) = 0.516);
              step        decode_step on PagedKVCache(dtype="fp8") against KVCache(dtype="fp8") in rows mode and against the bf16 pool;
              workload    the same prompts also through generate_many(kv_dtype="fp8") at the default page count.

  --share     prompt pages shared between requests (include/omnibiote_hip_paged_extend.h), instead of the parts above:
              extend      obte_attn_extend_paged, the pool's pages in random order, against obte_attn_extend's rows form on a rectangle holding
                          the same keys, every row's n new positions behind ctx - n cached ones, at B x ctx in {8 x 2048, 64 x 2048} and
                          n in {32, 64}, each call on the next layer's cache;
              sharing     a seeded workload of --prompts prompts, each one of 4 prefixes of 512 tokens followed by a tail of 16 .. 256
                          tokens of its own, 128 new tokens, batch 64, no eos_token: generate_many(share_prefix=True) against
                          share_prefix=False — tokens per second of wall time, and from `stats` the prompt positions computed, the
                          pages in use at the peak and the decode steps.

    python tools/paged_bench.py [--kv8 | --share] [--parts attention,step,workload] [--rounds 5] [--steps 200]
"""
import argparse
import contextlib
import io
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from decode_bench import HBM_RATE, INFINITY_CACHE, build, summary, timed  # noqa: E402


def _gap(us, a, b, nd=2):
    """median(a) - median(b) and both spreads"""
    return [round(statistics.median(us[a]) - statistics.median(us[b]), nd)] + [round(max(us[k]) - min(us[k]), nd) for k in (a, b)]


def attention(m, B, ctx, rounds, steps, dev):
    from omnibiote_amd import _lib, ops
    from omnibiote_amd.paged import paged_scatter_reference
    lib = _lib.lib()
    H, C = m.config.n_head, m.config.n_embd
    hs, n_layer, n_pages = C // H, m.config.n_layer, B * ctx // 64
    gen = torch.Generator(device=dev).manual_seed(B * 10007 + ctx)
    table = torch.randperm(n_pages, device=dev, generator=gen).view(B, ctx // 64).to(torch.int32)
    ordered = torch.arange(n_pages, device=dev, dtype=torch.int32).view(B, ctx // 64)   # the probe: the same pool layout, row b's pages side by side
    rects, pools, pools_ordered = [], [], []
    for _ in range(n_layer):
        rect = ops.kv_cache_buffer(B, ctx, H, hs, dev).normal_(generator=gen)
        K, V = rect.view(2, B, H, ctx, hs)
        rects.append(rect)
        pools.append(paged_scatter_reference(K, V, table, n_pages))
        pools_ordered.append(paged_scatter_reference(K, V, ordered, n_pages))
    q = torch.randn(B, 3 * C, device=dev, generator=gen).to(torch.bfloat16)
    counts = torch.full((B,), ctx, dtype=torch.int32, device=dev)
    ws = torch.empty(int(lib.obte_attn_decode_ws_bytes(B, H, hs)), dtype=torch.uint8, device=dev)
    o = torch.empty(B, C, device=dev, dtype=torch.bfloat16)
    lse = torch.empty(B, H, device=dev, dtype=torch.float32)
    stream = torch.cuda.current_stream().cuda_stream
    state = {"i": 0}

    def rows():                # the C entry points themselves on preallocated outputs, each call on the next layer's cache
        state["i"] += 1
        rc = lib.obte_attn_decode_rows(q.data_ptr(), 3 * C, rects[state["i"] % n_layer].data_ptr(), o.data_ptr(), lse.data_ptr(), B, ctx, counts.data_ptr(), ctx,
                                       H, hs, 8.0 / C, 0, ws.data_ptr(), ws.numel(), stream)
        if rc != 0:
            _lib.check(rc, "obte_attn_decode_rows")

    def paged(pools=pools, table=table):
        state["i"] += 1
        rc = lib.obte_attn_decode_paged(q.data_ptr(), 3 * C, pools[state["i"] % n_layer].data_ptr(), n_pages, table.data_ptr(), ctx // 64, o.data_ptr(),
                                        lse.data_ptr(), B, counts.data_ptr(), ctx, H, hs, 8.0 / C, 0, ws.data_ptr(), ws.numel(), stream)
        if rc != 0:
            _lib.check(rc, "obte_attn_decode_paged")
    a, _ = ops.attn_decode_rows(q, rects[0], B, ctx, counts, ctx, H, hs, 8.0 / C)
    b, _ = ops.attn_decode_paged(q, pools[0], n_pages, table, B, counts, ctx, H, hs, 8.0 / C)
    legs = {"rows": rows, "paged": paged, "paged_pages_in_order": lambda: paged(pools_ordered, ordered)}
    for fn in legs.values():
        for _ in range(8):
            fn()
    us = {k: [] for k in legs}
    for r in range(rounds):
        for k in (list(legs) if r % 2 == 0 else list(legs)[::-1]):
            us[k].append(timed(legs[k], steps))
    nbytes, set_bytes = 4 * B * H * ctx * hs, sum(t.numel() * 2 for t in rects)
    med = {k: statistics.median(v) for k, v in us.items()}
    return {"part": "attention", "B": B, "context": ctx, "windows": {"calls": steps, "rounds": rounds}, "same_bits": bool(torch.equal(a, b)),
            "splits": int(lib.obte_attn_decode_splits(B, H, hs, ctx)), "bytes_per_call": nbytes, "table_bytes_per_call": 4 * B * ctx // 64, "set_bytes": set_bytes,
            "served_from": "HBM" if set_bytes > INFINITY_CACHE else "Infinity Cache (not an HBM measurement)",
            "us": {k: summary(v) for k, v in us.items()}, "share_of_6.3TBps": {k: round(nbytes / (med[k] * 1e-6) / HBM_RATE, 3) for k in legs},
            "paged_over_rows": round(med["paged"] / med["rows"], 3), "paged_minus_rows_us_and_spreads": _gap(us, "paged", "rows"),
            "in_order_minus_rows_us_and_spreads": _gap(us, "paged_pages_in_order", "rows")}


def attention8(m, B, ctx, rounds, steps, dev):
    """--kv8: the four one-query calls over the same keys' worth of positions, alternating in one process"""
    from omnibiote_amd import _lib, ops
    from omnibiote_amd.kvquant import split_cache
    from omnibiote_amd.paged import paged8_scatter_reference, paged_scatter_reference
    lib = _lib.lib()
    H, C = m.config.n_head, m.config.n_embd
    hs, n_layer, n_pages, ld = C // H, m.config.n_layer, B * ctx // 64, ctx // 64
    gen = torch.Generator(device=dev).manual_seed(B * 10007 + ctx)
    table = torch.randperm(n_pages, device=dev, generator=gen).view(B, ld).to(torch.int32)
    ordered = torch.arange(n_pages, device=dev, dtype=torch.int32).view(B, ld)
    rects, pools, rects8, pools8, pools8_ordered = [], [], [], [], []
    for _ in range(n_layer):
        rect = ops.kv_cache_buffer(B, ctx, H, hs, dev).normal_(generator=gen)
        K, V = rect.view(2, B, H, ctx, hs)
        rects.append(rect)
        pools.append(paged_scatter_reference(K, V, table, n_pages))
        rect8 = ops.kv8_cache_buffer(B, ctx, H, hs, dev)
        kc, vc, ks, vs = split_cache(rect8, B, ctx, H, hs)
        kc.random_(0, 0x7F, generator=gen); vc.random_(0, 0x7F, generator=gen)          # finite codes, scales of the keys' size: only the time is read
        ks.fill_(2.0 ** -7); vs.fill_(2.0 ** -7)
        codes, scales = torch.stack([kc, vc]), torch.stack([ks, vs])
        rects8.append(rect8)
        pools8.append(paged8_scatter_reference(codes, scales, table, n_pages))
        pools8_ordered.append(paged8_scatter_reference(codes, scales, ordered, n_pages))
        del codes, scales
    q = torch.randn(B, 3 * C, device=dev, generator=gen).to(torch.bfloat16)
    counts = torch.full((B,), ctx, dtype=torch.int32, device=dev)
    ws = torch.empty(int(lib.obte_attn_decode_ws_bytes(B, H, hs)), dtype=torch.uint8, device=dev)
    o = torch.empty(B, C, device=dev, dtype=torch.bfloat16)
    lse = torch.empty(B, H, device=dev, dtype=torch.float32)
    stream = torch.cuda.current_stream().cuda_stream
    state = {"i": 0}

    def call(name, *args):
        rc = getattr(lib, name)(*args)
        if rc != 0:
            _lib.check(rc, name)

    def nxt(bufs):
        state["i"] += 1
        return bufs[state["i"] % n_layer].data_ptr()
    tail = (H, hs, 8.0 / C, 0, ws.data_ptr(), ws.numel(), stream)
    legs = {
        "rows": lambda: call("obte_attn_decode_rows", q.data_ptr(), 3 * C, nxt(rects), o.data_ptr(), lse.data_ptr(), B, ctx, counts.data_ptr(), ctx, *tail),
        "paged": lambda: call("obte_attn_decode_paged", q.data_ptr(), 3 * C, nxt(pools), n_pages, table.data_ptr(), ld, o.data_ptr(), lse.data_ptr(), B, counts.data_ptr(),
                              ctx, *tail),
        "kv8_rows": lambda: call("obte_attn_decode_kv8", q.data_ptr(), 3 * C, nxt(rects8), o.data_ptr(), lse.data_ptr(), B, ctx, ctx, counts.data_ptr(), *tail),
        "paged8": lambda: call("obte_attn_decode_paged8", q.data_ptr(), 3 * C, nxt(pools8), n_pages, table.data_ptr(), ld, o.data_ptr(), lse.data_ptr(), B,
                               counts.data_ptr(), ctx, *tail),
        "paged8_pages_in_order": lambda: call("obte_attn_decode_paged8", q.data_ptr(), 3 * C, nxt(pools8_ordered), n_pages, ordered.data_ptr(), ld, o.data_ptr(),
                                              lse.data_ptr(), B, counts.data_ptr(), ctx, *tail),
    }
    a, _ = ops.attn_decode_kv8(q, rects8[0], B, ctx, ctx, H, hs, 8.0 / C, n_keys_rows=counts)
    b, _ = ops.attn_decode_paged8(q, pools8[0], n_pages, table, B, counts, ctx, H, hs, 8.0 / C)
    for fn in legs.values():
        for _ in range(8):
            fn()
    us = {k: [] for k in legs}
    for r in range(rounds):
        for k in (list(legs) if r % 2 == 0 else list(legs)[::-1]):
            us[k].append(timed(legs[k], steps))
    nbytes = {"rows": 4 * B * H * ctx * hs, "kv8_rows": 2 * B * H * ctx * (hs + 4)}
    nbytes["paged"], nbytes["paged8"], nbytes["paged8_pages_in_order"] = nbytes["rows"], nbytes["kv8_rows"], nbytes["kv8_rows"]
    set8 = sum(t.numel() for t in rects8)
    med = {k: statistics.median(v) for k, v in us.items()}
    return {"part": "attention", "kv8": True, "B": B, "context": ctx, "windows": {"calls": steps, "rounds": rounds}, "same_bits": bool(torch.equal(a, b)),
            "splits": int(lib.obte_attn_decode_splits(B, H, hs, ctx)), "bytes_per_call": nbytes, "table_bytes_per_call": 4 * B * ld,
            "set_bytes": {"bf16": sum(t.numel() * 2 for t in rects), "e4m3": set8},
            "served_from": {"bf16": "HBM" if sum(t.numel() * 2 for t in rects) > INFINITY_CACHE else "Infinity Cache (not an HBM measurement)",
                            "e4m3": "HBM" if set8 > INFINITY_CACHE else "Infinity Cache (not an HBM measurement)"},
            "us": {k: summary(v) for k, v in us.items()}, "share_of_6.3TBps": {k: round(nbytes[k] / (med[k] * 1e-6) / HBM_RATE, 3) for k in legs},
            "paged8_over_kv8_rows": round(med["paged8"] / med["kv8_rows"], 4), "paged8_minus_kv8_rows_us_and_spreads": _gap(us, "paged8", "kv8_rows"),
            "in_order_minus_kv8_rows_us_and_spreads": _gap(us, "paged8_pages_in_order", "kv8_rows"),
            "paged_over_rows": round(med["paged"] / med["rows"], 4), "paged_minus_rows_us_and_spreads": _gap(us, "paged", "rows"),
            "paged8_over_paged": round(med["paged8"] / med["paged"], 3), "kv8_rows_over_rows": round(med["kv8_rows"] / med["rows"], 3),
            "byte_ratio": round((hs + 4) / (2 * hs), 3)}


def step8(m, B, ctx, rounds, steps, dev):
    """--kv8: decode_step on the e4m3 pool, on the e4m3 rectangle in rows mode and on the bf16 pool, every window walking the same positions"""
    from omnibiote_amd.model import KVCache, PagedKVCache
    first = ctx - 1 - steps
    gen = torch.Generator(device=dev).manual_seed(B * 10007 + ctx)
    last = torch.randint(4, m.config.vocab_size, (B,), device=dev, generator=gen)
    order = torch.randperm(B * ctx // 64, generator=torch.Generator().manual_seed(1)).tolist()
    rect8 = KVCache(m, B, ctx, dtype="fp8")
    caches = {"paged": PagedKVCache(m, B, B * ctx // 64, ctx, free_order=order), "paged8": PagedKVCache(m, B, B * ctx // 64, ctx, free_order=order, dtype="fp8")}
    for kv in caches["paged"].layers:
        kv.normal_(generator=gen)
    for kv in rect8.layers + caches["paged8"].layers:                   # every code 1.0 and every scale the fp32 of the same bytes, 4.4e-5: finite
        kv.fill_(0x38)
    for c in caches.values():
        for b in range(B):
            c.assign(b, ctx)

    def window(kind):
        if kind == "kv8_rows":
            rect8.reset(first, torch.full((B,), first, dtype=torch.int32, device=dev), first)
            cache = rect8
        else:
            cache = caches[kind]
            cache.start_rows(range(B), [first] * B)
        return timed(lambda: m.decode_step(last, cache), steps)
    legs = ("kv8_rows", "paged8", "paged")
    for k in legs:
        window(k)
    us = {k: [] for k in legs}
    for r in range(rounds):
        for k in (legs if r % 2 == 0 else legs[::-1]):
            us[k].append(window(k))
    med = {k: statistics.median(v) for k, v in us.items()}
    return {"part": "step", "kv8": True, "B": B, "context": ctx, "windows": {"decode_steps": steps, "rounds": rounds, "positions": [first, ctx - 2]},
            "us_per_token": {k: summary(v, 1) for k, v in us.items()}, "paged8_over_kv8_rows": round(med["paged8"] / med["kv8_rows"], 3),
            "paged8_minus_kv8_rows_us_and_spreads": _gap(us, "paged8", "kv8_rows", 1), "paged8_over_paged": round(med["paged8"] / med["paged"], 3),
            "tokens_per_s": {k: round(B / med[k] * 1e6) for k in legs}}


def step(m, B, ctx, rounds, steps, dev):
    from omnibiote_amd.model import KVCache, PagedKVCache
    first = ctx - 1 - steps
    gen = torch.Generator(device=dev).manual_seed(B * 10007 + ctx)
    last = torch.randint(4, m.config.vocab_size, (B,), device=dev, generator=gen)
    rect, paged = KVCache(m, B, ctx), PagedKVCache(m, B, B * ctx // 64, ctx, free_order=torch.randperm(B * ctx // 64, generator=torch.Generator().manual_seed(1)).tolist())
    for kv in rect.layers + paged.layers:                              # finite values of the keys' size: only the time is read
        kv.normal_(generator=gen)
    for b in range(B):
        paged.assign(b, ctx)

    def window(kind):
        if kind == "rows":
            rect.reset(first, torch.full((B,), first, dtype=torch.int32, device=dev), first)
            cache = rect
        else:
            paged.start_rows(range(B), [first] * B)                     # (the rows hold their pages: only the positions move)
            cache = paged
        return timed(lambda: m.decode_step(last, cache), steps)
    legs = ("rows", "paged")
    for k in legs:
        window(k)
    us = {k: [] for k in legs}
    for r in range(rounds):
        for k in (legs if r % 2 == 0 else legs[::-1]):
            us[k].append(window(k))
    med = {k: statistics.median(v) for k, v in us.items()}
    return {"part": "step", "B": B, "context": ctx, "windows": {"decode_steps": steps, "rounds": rounds, "positions": [first, ctx - 2]},
            "us_per_token": {k: summary(v, 1) for k, v in us.items()}, "paged_over_rows": round(med["paged"] / med["rows"], 3),
            "paged_minus_rows_us_and_spreads": _gap(us, "paged", "rows", 1), "tokens_per_s": {k: round(B / med[k] * 1e6) for k in legs}}


def extend_attention(m, B, ctx, n, rounds, steps, dev):
    """--share: n queries per row behind ctx - n cached positions, through the page table and on the rectangle, alternating in one process"""
    from omnibiote_amd import _lib, ops
    from omnibiote_amd.paged import paged_scatter_reference
    lib = _lib.lib()
    H, C = m.config.n_head, m.config.n_embd
    hs, n_layer, n_pages, ld = C // H, m.config.n_layer, B * ctx // 64, ctx // 64
    gen = torch.Generator(device=dev).manual_seed(B * 10007 + ctx + n)
    table = torch.randperm(n_pages, device=dev, generator=gen).view(B, ld).to(torch.int32)
    rects, pools = [], []
    for _ in range(n_layer):
        rect = ops.kv_cache_buffer(B, ctx, H, hs, dev).normal_(generator=gen)
        K, V = rect.view(2, B, H, ctx, hs)
        rects.append(rect)
        pools.append(paged_scatter_reference(K, V, table, n_pages))
    q = torch.randn(B * n, 3 * C, device=dev, generator=gen).to(torch.bfloat16)
    pos = ctx - n
    starts = torch.full((B,), pos, dtype=torch.int32, device=dev)
    ws = torch.empty(max(int(lib.obte_attn_extend_ws_bytes(B, H, hs, n, 0)), 16), dtype=torch.uint8, device=dev)
    o = torch.empty(B * n, C, device=dev, dtype=torch.bfloat16)
    lse = torch.empty(B, H, n, device=dev, dtype=torch.float32)
    stream = torch.cuda.current_stream().cuda_stream
    state = {"i": 0}

    def rows():
        state["i"] += 1
        rc = lib.obte_attn_extend(q.data_ptr(), 3 * C, rects[state["i"] % n_layer].data_ptr(), o.data_ptr(), lse.data_ptr(), B, ctx, n, pos, starts.data_ptr(), H, hs,
                                  8.0 / C, 0, ws.data_ptr(), ws.numel(), stream)
        if rc != 0:
            _lib.check(rc, "obte_attn_extend")

    def paged():
        state["i"] += 1
        rc = lib.obte_attn_extend_paged(q.data_ptr(), 3 * C, pools[state["i"] % n_layer].data_ptr(), n_pages, table.data_ptr(), ld, o.data_ptr(), lse.data_ptr(), B, n,
                                        pos, starts.data_ptr(), H, hs, 8.0 / C, 0, ws.data_ptr(), ws.numel(), stream)
        if rc != 0:
            _lib.check(rc, "obte_attn_extend_paged")
    a, _ = ops.attn_extend(q, rects[0], B, ctx, n, pos, H, hs, 8.0 / C, pos_rows=starts)
    b, _ = ops.attn_extend_paged(q, pools[0], n_pages, table, B, n, pos, H, hs, 8.0 / C, starts)
    legs = {"rows": rows, "paged": paged}
    for fn in legs.values():
        for _ in range(8):
            fn()
    us = {k: [] for k in legs}
    for r in range(rounds):
        for k in (list(legs) if r % 2 == 0 else list(legs)[::-1]):
            us[k].append(timed(legs[k], steps))
    nbytes, set_bytes = 4 * B * H * ctx * hs * ((n + 31) // 32), sum(t.numel() * 2 for t in rects)
    med = {k: statistics.median(v) for k, v in us.items()}
    return {"part": "extend", "B": B, "context": ctx, "n_new": n, "windows": {"calls": steps, "rounds": rounds}, "same_bits": bool(torch.equal(a, b)),
            "splits": int(lib.obte_attn_extend_splits(B, H, hs, n, ctx)), "bytes_read_per_call_at_most": nbytes, "set_bytes": set_bytes,
            "served_from": "HBM" if set_bytes > INFINITY_CACHE else "Infinity Cache (not an HBM measurement)",
            "us": {k: summary(v) for k, v in us.items()}, "paged_over_rows": round(med["paged"] / med["rows"], 4),
            "paged_minus_rows_us_and_spreads": _gap(us, "paged", "rows")}


def sharing(n_prompts, vocab, rounds, dev):
    """--share: generate_many with and without share_prefix over prompts that carry one of 4 prefixes of 512 tokens"""
    new, batch, n_prefix, prefix_len = 128, 64, 4, 512
    m = build_small_vocab(prefix_len + 256 + new, vocab, dev)
    g = torch.Generator().manual_seed(17)
    prefixes = [torch.randint(8, vocab, (prefix_len,), generator=g) for _ in range(n_prefix)]
    tails = torch.randint(16, 257, (n_prompts,), generator=g).tolist()
    which = torch.randint(0, n_prefix, (n_prompts,), generator=g).tolist()
    prompts = [torch.cat([prefixes[w], torch.randint(8, vocab, (t,), generator=g)]).to(dev) for w, t in zip(which, tails)]
    legs = {"share_prefix_false": False, "share_prefix_true": True}
    res = {k: {"tokens_per_s": [], "wall_s": []} for k in legs}
    for r in range(rounds + 1):                                         # (round 0 warms up)
        for k in (list(legs) if r % 2 == 0 else list(legs)[::-1]):
            stats = {}
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = m.generate_many(prompts, new, batch, generator=torch.Generator(device=dev).manual_seed(3), share_prefix=legs[k], stats=stats)
            torch.cuda.synchronize()
            wall = time.perf_counter() - t0
            if r == 0:
                res[k].update(new_tokens=sum(o.numel() - p.numel() for o, p in zip(out, prompts)), **stats)
                continue
            res[k]["tokens_per_s"].append(res[k]["new_tokens"] / wall)
            res[k]["wall_s"].append(wall)
    base = statistics.median(res["share_prefix_false"]["tokens_per_s"])
    spreads = [round(max(res[k]["tokens_per_s"]) - min(res[k]["tokens_per_s"])) for k in legs]
    for v in res.values():
        v["over_share_prefix_false"] = round(statistics.median(v["tokens_per_s"]) / base, 3)
        v["tokens_per_s"], v["wall_s"] = summary(v["tokens_per_s"], 0), summary(v["wall_s"], 3)
    return {"part": "sharing", "prompts": n_prompts, "prefixes": n_prefix, "prefix_tokens": prefix_len, "tails": [min(tails), max(tails)], "max_new_tokens": new,
            "batch": batch, "vocab": vocab, "rounds": rounds, "tokens_per_s_spreads": spreads, **res}


def build_small_vocab(block_size, vocab, dev):
    """decode_bench.build's model with another vocabulary (the workload: see the head of this file)"""
    import warnings
    from omnibiote_amd.model import OmniBioTA, OmniBioTAConfig
    from omnibiote_amd.mup_compat import set_base_shapes

    def make(n_embd, n_head):
        c = OmniBioTAConfig()
        c.block_size, c.vocab_size, c.n_layer, c.n_head, c.n_embd, c.dropout, c.flash = block_size, vocab, 8, n_head, n_embd, 0.0, True
        c.autoregressive = True
        return OmniBioTA(c)
    torch.manual_seed(0)
    with contextlib.redirect_stdout(io.StringIO()), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        m = make(1024, 8)
        set_base_shapes(m, make(24, 3), delta=make(48, 12))
        m.to(torch.bfloat16)
    return m.to(dev).eval()


def workload(n_prompts, vocab, pool_share, rounds, dev, kv8=False):
    from omnibiote_amd import _lib
    from omnibiote_amd.paged import PagedSchedule, pool8_bytes, pool_bytes
    new, batch, eos = 256, 64, 7
    m = build_small_vocab(1024 + new, vocab, dev)
    cfg = m.config
    H, hs = cfg.n_head, cfg.n_embd // cfg.n_head
    g = torch.Generator().manual_seed(11)
    lens = torch.linspace(64, 1024, n_prompts).long()[torch.randperm(n_prompts, generator=g)].tolist()
    prompts = [torch.randint(8, vocab, (n,), generator=g).to(dev) for n in lens]
    default_pages = PagedSchedule(lens, new, batch).n_pages
    pools = {"generate_many": default_pages, f"generate_many_{pool_share}_pool": max(int(default_pages * pool_share), max(PagedSchedule(lens, new, batch).need))}
    calls = {"n": 0}
    plain_step = m.decode_step

    def counted(*a, **k):
        calls["n"] += 1
        return plain_step(*a, **k)
    m.decode_step = counted

    def many(n_pages, kv_dtype="bf16"):
        def run():
            out = m.generate_many(prompts, new, batch, n_pages=n_pages, eos_token=eos, generator=torch.Generator(device=dev).manual_seed(3), kv_dtype=kv_dtype)
            return [o.numel() - n for o, n in zip(out, lens)], None
        return run

    def batched():
        made, peak = [], 0
        for i in range(0, n_prompts, batch):
            part, ln = prompts[i:i + batch], lens[i:i + batch]
            idx = torch.nn.utils.rnn.pad_sequence(part, batch_first=True)
            _, n_out = m.generate(idx, new, lengths=ln, sampler="device", eos_token=eos, generator=torch.Generator(device=dev).manual_seed(3))
            made += [int(a) - b for a, b in zip(n_out.tolist(), ln)]
            peak = max(peak, cfg.n_layer * int(_lib.lib().obte_kv_cache_bytes(len(part), max(ln) + new, H, hs)))
        return made, peak
    legs = {"generate_batches": batched, **{k: many(v) for k, v in pools.items()}}
    if kv8:                                                             # the same page count at about half the bytes
        pools["generate_many_fp8"] = default_pages
        legs["generate_many_fp8"] = many(default_pages, "fp8")
    res = {k: {"tokens_per_s": [], "wall_s": []} for k in legs}
    for r in range(rounds + 1):                                         # (round 0 warms up)
        for k in (list(legs) if r % 2 == 0 else list(legs)[::-1]):
            calls["n"] = 0
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            made, peak = legs[k]()
            torch.cuda.synchronize()
            wall = time.perf_counter() - t0
            if r == 0:
                res[k].update(new_tokens=sum(made), rows_ended_by_eos=sum(1 for n in made if n < new), decode_steps=calls["n"],
                              share_of_row_steps_on_finished_rows=round(1 - sum(n - 1 for n in made) / max(calls["n"] * batch, 1), 3),
                              peak_cache_bytes=peak if peak is not None else cfg.n_layer * (pool8_bytes if k.endswith("_fp8") else pool_bytes)(pools[k], H, hs))
                continue
            res[k]["tokens_per_s"].append(sum(made) / wall)
            res[k]["wall_s"].append(wall)
    base = statistics.median(res["generate_batches"]["tokens_per_s"])
    for k, v in res.items():
        v["over_generate_batches"] = round(statistics.median(v["tokens_per_s"]) / base, 3)
        v["tokens_per_s"], v["wall_s"] = summary(v["tokens_per_s"], 0), summary(v["wall_s"], 3)
    return {"part": "workload", "prompts": n_prompts, "lengths": [min(lens), max(lens)], "max_new_tokens": new, "batch": batch, "vocab": vocab, "eos_token": eos,
            "pages": pools, "rounds": rounds, **res}


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--parts", default="attention,step,workload")
    p.add_argument("--rounds", type=int, default=5)
    p.add_argument("--steps", type=int, default=200, help="attention calls and decode steps per timed window")
    p.add_argument("--prompts", type=int, default=256)
    p.add_argument("--vocab", type=int, default=256)
    p.add_argument("--pool-share", type=float, default=0.65)
    p.add_argument("--kv8", action="store_true", help="the e4m3 pool: see the head of this file")
    p.add_argument("--share", action="store_true", help="prompt pages shared between requests (parts extend,sharing): see the head of this file")
    a = p.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    parts = a.parts.split(",")
    if a.share:
        parts = ["extend", "sharing"] if a.parts == p.get_default("parts") else parts
        if "extend" in parts:
            m = build(2048, dev)
            for B, ctx in ((8, 2048), (64, 2048)):
                for n in (32, 64):
                    print(json.dumps(extend_attention(m, B, ctx, n, a.rounds, a.steps, dev)), flush=True)
                    torch.cuda.empty_cache()
            del m
            torch.cuda.empty_cache()
        if "sharing" in parts:
            print(json.dumps(sharing(a.prompts, a.vocab, a.rounds, dev)), flush=True)
        return
    if "attention" in parts or "step" in parts:
        m = build(2048, dev)
        for B, ctx in ((64, 2048), (8, 2048)):
            if "attention" in parts:
                print(json.dumps((attention8 if a.kv8 else attention)(m, B, ctx, a.rounds, a.steps, dev)), flush=True)
                torch.cuda.empty_cache()
            if "step" in parts:
                print(json.dumps((step8 if a.kv8 else step)(m, B, ctx, a.rounds, a.steps, dev)), flush=True)
                torch.cuda.empty_cache()
        del m
        torch.cuda.empty_cache()
    if "workload" in parts:
        print(json.dumps(workload(a.prompts, a.vocab, a.pool_share, a.rounds, dev, a.kv8)), flush=True)


if __name__ == "__main__":
    main()
