"""Autoregressive generation on the small config (8 layers, 1024 wide, 8 heads of 128; bf16): what a generated token costs.

For every batch size B and context length ctx (the new token attends over ctx positions):
  1. time per generated token: OmniBioTA.decode_step against a key/value cache that holds ctx - 1 positions, versus what the code
     offered before the cache existed for the same token: model(idx)[:, -1] under no_grad over the whole ctx-token prefix.  Both
     contenders alternate in one process over --rounds rounds after warm-up; device events around windows of --steps decode steps
     (the full forward: as many calls as fit ~--baseline_ms, at least 3).  Median and [min - max] over the rounds.
  2. obte_attn_decode alone over one cache per layer in turn (the set a real step walks through: n_layer caches), for the library's own
     split count and for every forced count of --sweep: time, and the cache bytes one call must read (2 B H ctx hs 2) over that time as
     a share of 6.3 TB/s.  A set of caches that fits the 256 MB Infinity Cache is not an HBM measurement: `served_from` says which.
  3. the launch profiler's split of a decode step: attention (kind 102), the projections (the GEMM kinds), the rest (LayerNorm, the
     cache store, the embedding, the readout's LayerNorm, and every gap between launches).
One JSON line per (B, ctx).

    python tools/decode_bench.py [--batches 1,8,64] [--contexts 128,1024,2048] [--rounds 5] [--steps 300]

--ragged: the one-position-per-row step (a cache prefilled with ``lengths``: obte_block_decode_rows) instead of the above, at
B x ctx in {8 x 2048, 64 x 2048} unless --batches / --contexts say otherwise.  Two contenders alternate in one process over the same
windows and rounds: the rows path with every row at position ctx - 1, and the uniform path at that position (the same cache, the same
token).  Then one ragged batch, the rows' positions spread evenly over [ctx / 4, ctx).  One JSON line per (B, ctx).

    python tools/decode_bench.py --ragged [--rounds 5] [--steps 300]

--small-m: the weight-streaming product for M <= 64 (obte_linear_small_m_bf16) against the tile structures (obte_gemm_bf16), both
alternating in one process over the same windows and rounds.  (a) the product alone, the C entry points on preallocated buffers: the
five shapes of the small config at M = 1, 8, 16, 32, 64, each call on the next of eight distinct copies of a block weight (three of the
readout's 134 MB) as a decode step walks its layers; `served_from` says whether the set of copies exceeds the 256 MB Infinity Cache, and
the readout's bytes over its time are given as a share of 6.3 TB/s.  One JSON line per shape.  (b) decode_step with small_m_max at the
library's default against 0 at B x ctx in {1 x 2048, 8 x 2048, 64 x 1024, 64 x 2048}, the rows step at 8 x 2048 (every row at ctx - 1)
the same way, and the launch profiler's split of a step on the new path.  One JSON line per (B, ctx).

    python tools/decode_bench.py --small-m [--rounds 5] [--steps 300]

--kv8: the e4m3 key/value cache (KVCache(dtype="fp8"), include/omnibiote_hip_kv8.h) against the bf16 cache at B x ctx in {8 x 2048,
64 x 1024, 64 x 2048} unless --batches / --contexts say otherwise, both alternating in one process over the same windows and rounds:
(a) the attention alone, obte_attn_decode_kv8 and obte_attn_decode on preallocated outputs, each walking its own set of per-layer caches,
at the library's split count (at 8 x 2048 also under every forced count of --sweep: does the bf16 split rule still pick well with half the
bytes?); the bytes a call reads — 2 B H ctx (hs + 4) against 4 B H ctx hs — over its time as a share of 6.3 TB/s, the bytes of both cache
sets, and `served_from` for each: a set that fits the 256 MB Infinity Cache is not an HBM measurement.  (b) decode_step on both caches.
One JSON line per (B, ctx), then one line with the deviation of the fp8 attention output from the bf16 one on unit-variance inputs.

    python tools/decode_bench.py --kv8 [--rounds 5] [--steps 300]

--shared: G samples of one prompt on a shared-prefix cache (SharedPrefixCache, include/omnibiote_hip_shared.h) against the same rows on a
replicated KVCache, at P = 1, G in {8, 64}, n_prefix = 2048, n_suffix in {1, 256}, both alternating in one process over the same windows
and rounds: (a) the attention alone, obte_attn_decode_shared and obte_attn_decode on preallocated outputs at the library's split counts,
each walking its own set of per-layer caches, with the bytes each must read by the model 4 hs B H n against
4 hs H (P ceil(G / 32) n_prefix + B n_suffix); (b) decode_step on both caches; (c) the prefill of generate (G rows against one), one call
per window; and the bytes of both cache sets.  One JSON line per (G, n_suffix).

    python tools/decode_bench.py --shared [--rounds 5] [--steps 300]

--graph: the device-resident token loop (model.DecodeLoop, include/omnibiote_hip_loop.h) at B x ctx in {1, 8, 64} x 2048 unless --batches /
--contexts say otherwise, with sampling (T = 0.8, top_k = 200, top_p = 0.9) and an eos_token that no row draws.  Contenders alternate in one
process over the same windows and rounds, every window walking the same cache positions up to ctx - 2: today's loop (decode_step on the rows
path + ops.sample_logits + the host's bookkeeping, without its per-token host read), DecodeLoop eager, DecodeLoop captured, and the captured
loop without an eos_token (no host read at all).  Also the one-time cost of building each loop (warm-up + capture) and the kernel nodes of
one step before and after, counted in captured graphs of their own.  One JSON line per (B, ctx).

    python tools/decode_bench.py --graph [--constrained] [--penalized] [--rounds 5] [--steps 300]

--penalized (with --graph): also the captured loop with repetition, presence and frequency penalties (include/omnibiote_hip_penalty.h) — the
sampler reads the prompt of ctx - 1 - steps tokens and the loop's own tokens so far, in its one launch.

--w8: the decode step's weights as e4m3 (model.quantize_weights(), include/omnibiote_hip_w8.h) against bf16, both alternating in one process over
the same windows and rounds.  (a) the product alone, obte_linear_small_m_w8 against obte_linear_small_m_bf16 on preallocated buffers: the four
block shapes and the readout at widths C = 1024 and 2048, M = 1, 8, 64, each call on the next of enough distinct copies of the weight that
BOTH sets exceed the 256 MB Infinity Cache (`served_from` says so); each format's weight bytes over its time as a share of 6.3 TB/s, and the
byte ratio (K + 4) / (2 K).  `kernel` says which of the two kernels a shape takes.  One JSON line per (C, shape).  (b) decode_step with and
without weights= on the small (8 layers, 1024 wide) and the large (24 layers, 2048 wide) config at B x ctx in {1, 8, 64} x 2048 (cache contents:
random values, only the time is read), and the captured DecodeLoop at B = 1.  One JSON line per (config, B).  --w8-part products|small|large
runs one part.

    python tools/decode_bench.py --w8 [--w8-part products] [--rounds 5] [--steps 300]

--w4: --w8 with MXFP4 weights (model.quantize_weights(format="mxfp4"), include/omnibiote_hip_w4.h) as a third leg of every comparison, the three
alternating in one process.  The products at M = 1 and 64, on enough copies that the MXFP4 set, the smallest, exceeds the Infinity Cache; the byte
ratio to e4m3 is (K / 2 + K / 32) / (K + 4).  Every line carries mxfp4_over_e4m3 and mxfp4_over_bf16 beside what --w8 prints.

    python tools/decode_bench.py --w4 [--w8-part products] [--rounds 5] [--steps 300]
"""
import argparse
import contextlib
import io
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_RATE = 6.3e12           # achievable HBM bytes/s of an MI355X
INFINITY_CACHE = 256 << 20


def summary(v, nd=2):
    return {"median": round(statistics.median(v), nd), "min": round(min(v), nd), "max": round(max(v), nd)}


def timed(fn, n):
    """microseconds per call of fn over a window of n calls between two device events"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / n * 1e3


def build(block_size, dev, n_layer=8, n_embd=1024, n_head=8, on_device=False):
    """the small config as an autoregressive model, muP base shapes set as the trainer sets them (train_encoder.build_model); ``n_layer``
    other than its 8: the same width with fewer layers (spec_bench.py's draft); ``n_embd`` / ``n_head``: another width (--w8's large config)"""
    import warnings
    from omnibiote_amd.model import OmniBioTA, OmniBioTAConfig
    from omnibiote_amd.mup_compat import set_base_shapes

    def make(n_embd, n_head):
        c = OmniBioTAConfig()
        c.block_size, c.vocab_size, c.n_layer, c.n_head, c.n_embd, c.dropout, c.flash = block_size, 2 ** 16, n_layer, n_head, n_embd, 0.0, True
        c.autoregressive = True
        return OmniBioTA(c)
    torch.manual_seed(0)
    with contextlib.redirect_stdout(io.StringIO()), warnings.catch_warnings():
        warnings.simplefilter("ignore")          # "Casting complex values to real": the reference's cos-only RoPE regime
        with torch.device(dev if on_device else "cpu"):   # (on_device: a billion parameters are initialised where they will live)
            m = make(n_embd, n_head)
        set_base_shapes(m, make(24, 3), delta=make(48, 12))
        m.to(torch.bfloat16)
    return m.to(dev).eval()


def token_time(m, B, ctx, rounds, steps, baseline_ms, dev):
    from omnibiote_amd.model import KVCache
    g = torch.Generator(device=dev).manual_seed(B * 10007 + ctx)
    idx = torch.randint(4, m.config.vocab_size, (B, ctx), device=dev, generator=g)
    cache = KVCache(m, B, ctx)
    if ctx > 1:
        m.prefill(idx[:, :ctx - 1], cache)
    last = idx[:, -1].contiguous()

    def step():                      # the same position every time: the context stays ctx long
        cache.pos = ctx - 1
        m.decode_step(last, cache)

    def full():
        with torch.no_grad():
            m(idx)[:, -1]
    for _ in range(3):
        step()
    full()
    n_full = max(3, min(steps, int(baseline_ms * 1e3 / max(timed(full, 1), 1.0))))
    us = {"decode_step": [], "full_forward": []}
    for r in range(rounds):
        for leg in (("decode_step", "full_forward") if r % 2 == 0 else ("full_forward", "decode_step")):
            us[leg].append(timed(step, steps) if leg == "decode_step" else timed(full, n_full))
    return us, cache, last, n_full


def ragged_time(m, B, ctx, rounds, steps, dev):
    from omnibiote_amd.model import KVCache
    g = torch.Generator(device=dev).manual_seed(B * 10007 + ctx)
    idx = torch.randint(4, m.config.vocab_size, (B, ctx), device=dev, generator=g)
    cache = KVCache(m, B, ctx)
    m.prefill(idx[:, :ctx - 1], cache)
    last = idx[:, -1].contiguous()
    equal = torch.full((B,), ctx - 1, dtype=torch.int32, device=dev)
    spread = torch.linspace(ctx // 4, ctx - 1, B, device=dev).to(torch.int32)

    def uniform():                   # the same position every time: the context stays ctx long
        cache.reset(ctx - 1)
        m.decode_step(last, cache)

    def rows(at):
        def step():
            cache.reset(ctx - 1, at)
            m.decode_step(last, cache)
        return step
    legs = {"rows_equal": rows(equal), "uniform": uniform}
    for fn in list(legs.values()) + [rows(spread)]:
        for _ in range(3):
            fn()
    us = {k: [] for k in legs}
    for r in range(rounds):
        for leg in (list(legs) if r % 2 == 0 else list(legs)[::-1]):
            us[leg].append(timed(legs[leg], steps))
    us["rows_spread"] = [timed(rows(spread), steps) for _ in range(rounds)]
    u = us["uniform"]
    gap = statistics.median(us["rows_equal"]) - statistics.median(u)
    return {"B": B, "context": ctx, "windows": {"decode_steps": steps, "rounds": rounds},
            "us_per_token": {k: summary(v, 1) for k, v in us.items()},
            "rows_equal_minus_uniform_us": round(gap, 1), "uniform_spread_us": round(max(u) - min(u), 1),
            "spread_positions": [int(spread.min()), int(spread.max())]}


def attention_alone(m, cache, B, ctx, rounds, steps, sweep, dev):
    from omnibiote_amd import _lib
    H, C = m.config.n_head, m.config.n_embd
    hs = C // H
    q = torch.randn(B, 3 * C, device=dev, generator=torch.Generator(device=dev).manual_seed(1)).to(torch.bfloat16)
    ws = torch.empty(int(_lib.lib().obte_attn_decode_ws_bytes(B, H, hs)), dtype=torch.uint8, device=dev)
    default = int(_lib.lib().obte_attn_decode_splits(B, H, hs, ctx))
    counts = [0] + [s for s in sweep if s == 1 or s * 64 <= max(ctx, 64)]
    o = torch.empty(B, C, device=dev, dtype=torch.bfloat16)
    lse = torch.empty(B, H, device=dev, dtype=torch.float32)
    state = {"i": 0}
    fn, stream = _lib.lib().obte_attn_decode, torch.cuda.current_stream().cuda_stream
    ptrs = [kv.data_ptr() for kv in cache.layers]

    def call(splits):          # the C entry point itself on preallocated outputs: the host side of a call is a few microseconds
        state["i"] += 1
        rc = fn(q.data_ptr(), 3 * C, ptrs[state["i"] % len(ptrs)], o.data_ptr(), lse.data_ptr(), B, cache.max_len, ctx, H, hs, 8.0 / C, splits,
                ws.data_ptr(), ws.numel(), stream)
        if rc != 0:
            _lib.check(rc, "obte_attn_decode")
    us = {s: [] for s in counts}
    for s in counts:
        for _ in range(8):
            call(s)
    for r in range(rounds):
        for s in (counts if r % 2 == 0 else counts[::-1]):
            us[s].append(timed(lambda: call(s), steps))
    nbytes = 2 * B * H * ctx * hs * 2
    set_bytes = nbytes * len(cache.layers)
    med = {s: statistics.median(v) for s, v in us.items()}
    return {"default_splits": default, "cache_bytes_per_call": nbytes, "set_bytes": set_bytes,
            "served_from": "HBM" if set_bytes > INFINITY_CACHE else "Infinity Cache (not an HBM measurement)",
            "us": {("default" if s == 0 else str(s)): summary(v) for s, v in us.items()},
            "share_of_6.3TBps": {("default" if s == 0 else str(s)): round(nbytes / (med[s] * 1e-6) / HBM_RATE, 3) for s in counts},
            "default_over_one_split": round(med[0] / med[1], 3)}


def step_split(m, cache, last, ctx, n_steps):
    """the launch profiler over n_steps decode steps: per-step microseconds in attention, in the projections, and the rest"""
    import ctypes as C
    from omnibiote_amd import _lib
    lib = _lib.lib()

    def step():
        cache.pos = ctx - 1
        m.decode_step(last, cache)
    lib.obte_profile_enable(1)
    total = timed(step, n_steps)
    cap = 16384
    ms, dims, kind = (C.c_double * cap)(), (C.c_int64 * (3 * cap))(), (C.c_int32 * cap)()
    n = lib.obte_profile_collect(ms, dims, kind, cap)
    lib.obte_profile_enable(0)
    attn = sum(ms[i] for i in range(n) if kind[i] == 102) * 1e3 / n_steps
    proj = sum(ms[i] for i in range(n) if kind[i] % 1000 < 100) * 1e3 / n_steps
    rest = max(total - attn - proj, 0.0)
    return {"us_per_step_under_the_profiler": round(total, 1), "attention_us": round(attn, 1), "projections_us": round(proj, 1),
            "rest_us": round(rest, 1), "share": {"attention": round(attn / total, 3), "projections": round(proj / total, 3),
                                                  "rest": round(rest / total, 3)}}


SMALL_M_SHAPES = (("c_attn", 3072, 1024, 8), ("proj", 1024, 1024, 8), ("fc", 4096, 1024, 8), ("mlp", 1024, 4096, 8), ("readout", 65536, 1024, 3))
SMALL_M_ROWS = (1, 8, 16, 32, 64)


def small_m_products(rounds, steps, dev):
    import ctypes as C
    from omnibiote_amd import _lib
    lib, stream = _lib.lib(), torch.cuda.current_stream().cuda_stream
    gen = torch.Generator(device=dev).manual_seed(5)
    for name, N, K, copies in SMALL_M_SHAPES:
        ws = [torch.randn(N, K, device=dev, generator=gen).mul_(0.02).to(torch.bfloat16) for _ in range(copies)]
        set_bytes = copies * N * K * 2
        out = {"product": name, "N": N, "K": K, "weight_copies": copies, "set_bytes": set_bytes,
               "served_from": "HBM" if set_bytes > INFINITY_CACHE else "Infinity Cache (not an HBM measurement)", "M": {}}
        for M in SMALL_M_ROWS:
            x = torch.randn(M, K, device=dev, generator=gen).to(torch.bfloat16)
            d = torch.empty(M, N, device=dev, dtype=torch.bfloat16)
            args = [_lib.GemmArgs(x.data_ptr(), w.data_ptr(), d.data_ptr(), None, None, M, N, K, K, K, N, 1, 1, _lib.EPI_NONE, 1.0, 0.0, 0, 0) for w in ws]
            state = {"i": 0}

            def call(fn, what):
                state["i"] += 1
                rc = fn(C.byref(args[state["i"] % copies]), stream)
                if rc != 0:
                    _lib.check(rc, what)
            legs = {"small_m": lambda: call(lib.obte_linear_small_m_bf16, "obte_linear_small_m_bf16"), "tile": lambda: call(lib.obte_gemm_bf16, "obte_gemm_bf16")}
            for fn in legs.values():
                for _ in range(8):
                    fn()
            us = {k: [] for k in legs}
            for r in range(rounds):
                for leg in (list(legs) if r % 2 == 0 else list(legs)[::-1]):
                    us[leg].append(timed(legs[leg], steps))
            med = {k: statistics.median(v) for k, v in us.items()}
            row = {"us": {k: summary(v) for k, v in us.items()}, "tile_over_small_m": round(med["tile"] / med["small_m"], 2),
                   "small_m_minus_tile_us": round(med["small_m"] - med["tile"], 2), "tile_spread_us": round(max(us["tile"]) - min(us["tile"]), 2),
                   "weight_bytes_share_of_6.3TBps": round(N * K * 2 / (med["small_m"] * 1e-6) / HBM_RATE, 3)}
            out["M"][str(M)] = row
        print(json.dumps(out), flush=True)
        del ws
        torch.cuda.empty_cache()


def small_m_tokens(m, B, ctx, rounds, steps, dev, ragged=False):
    """decode_step at the library's default small_m_max against 0, alternating; then the profiler's split of a step on the default"""
    from omnibiote_amd import _lib, ops
    from omnibiote_amd.model import KVCache
    default = _lib.lib().obte_small_m_max()
    g = torch.Generator(device=dev).manual_seed(B * 10007 + ctx)
    idx = torch.randint(4, m.config.vocab_size, (B, ctx), device=dev, generator=g)
    cache = KVCache(m, B, ctx)
    m.prefill(idx[:, :ctx - 1], cache)
    last = idx[:, -1].contiguous()
    equal = torch.full((B,), ctx - 1, dtype=torch.int32, device=dev)

    def step():                      # the same position every time: the context stays ctx long
        cache.reset(ctx - 1, equal if ragged else None)
        m.decode_step(last, cache)

    def under(limit):
        def leg():
            with ops.small_m_max(limit):
                return timed(step, steps)
        return leg
    legs = {"small_m_default": under(default), "small_m_0": under(0)}
    for limit in (default, 0):
        with ops.small_m_max(limit):
            for _ in range(3):
                step()
    us = {k: [] for k in legs}
    for r in range(rounds):
        for leg in (list(legs) if r % 2 == 0 else list(legs)[::-1]):
            us[leg].append(legs[leg]())
    med = {k: statistics.median(v) for k, v in us.items()}
    out = {"B": B, "context": ctx, "step": "rows (every row at ctx - 1)" if ragged else "uniform", "small_m_max_default": default,
           "windows": {"decode_steps": steps, "rounds": rounds}, "us_per_token": {k: summary(v, 1) for k, v in us.items()},
           "off_over_default": round(med["small_m_0"] / med["small_m_default"], 2),
           "tokens_per_s_default": round(B / med["small_m_default"] * 1e6)}
    if not ragged:
        out["step_split_default"] = step_split(m, cache, last, ctx, 20)
    return out


def kv8_compare(m, B, ctx, rounds, steps, sweep, dev):
    """the e4m3 cache against the bf16 cache: the attention alone over each set of per-layer caches, and decode_step"""
    from omnibiote_amd import _lib
    from omnibiote_amd.model import KVCache
    lib = _lib.lib()
    H, C = m.config.n_head, m.config.n_embd
    hs = C // H
    g = torch.Generator(device=dev).manual_seed(B * 10007 + ctx)
    idx = torch.randint(4, m.config.vocab_size, (B, ctx), device=dev, generator=g)
    caches = {"bf16": KVCache(m, B, ctx), "fp8": KVCache(m, B, ctx, dtype="fp8")}
    for cache in caches.values():
        m.prefill(idx[:, :ctx - 1], cache)
    last = idx[:, -1].contiguous()
    q = torch.randn(B, 3 * C, device=dev, generator=torch.Generator(device=dev).manual_seed(1)).to(torch.bfloat16)
    ws = torch.empty(int(lib.obte_attn_decode_ws_bytes(B, H, hs)), dtype=torch.uint8, device=dev)
    o = torch.empty(B, C, device=dev, dtype=torch.bfloat16)
    lse = torch.empty(B, H, device=dev, dtype=torch.float32)
    stream = torch.cuda.current_stream().cuda_stream
    ptrs = {k: [kv.data_ptr() for kv in cache.layers] for k, cache in caches.items()}
    state = {"i": 0}

    def attn(kind, splits):    # the C entry points themselves on preallocated outputs, each call on the next layer's cache
        state["i"] += 1
        kv = ptrs[kind][state["i"] % len(ptrs[kind])]
        if kind == "fp8":
            rc = lib.obte_attn_decode_kv8(q.data_ptr(), 3 * C, kv, o.data_ptr(), lse.data_ptr(), B, ctx, ctx, None, H, hs, 8.0 / C, splits, ws.data_ptr(),
                                          ws.numel(), stream)
        else:
            rc = lib.obte_attn_decode(q.data_ptr(), 3 * C, kv, o.data_ptr(), lse.data_ptr(), B, ctx, ctx, H, hs, 8.0 / C, splits, ws.data_ptr(), ws.numel(),
                                      stream)
        if rc != 0:
            _lib.check(rc, "obte_attn_decode" + ("_kv8" if kind == "fp8" else ""))

    def step(kind):
        def fn():                    # the same position every time: the context stays ctx long
            caches[kind].reset(ctx - 1)
            m.decode_step(last, caches[kind])
        return fn
    counts = [0] + [s for s in sweep if s == 1 or s * 64 <= max(ctx, 64)]
    legs = {(kind, s): (lambda kind=kind, s=s: attn(kind, s)) for s in counts for kind in ("bf16", "fp8")}
    legs.update({(kind, "step"): step(kind) for kind in ("bf16", "fp8")})
    for key, fn in legs.items():
        for _ in range(3 if key[1] == "step" else 8):
            fn()
    us = {key: [] for key in legs}
    for r in range(rounds):
        for key in (list(legs) if r % 2 == 0 else list(legs)[::-1]):
            us[key].append(timed(legs[key], steps))
    med = {key: statistics.median(v) for key, v in us.items()}
    nbytes = {"bf16": 4 * B * H * ctx * hs, "fp8": 2 * B * H * ctx * (hs + 4)}
    sets = {k: sum(kv.numel() * kv.element_size() for kv in caches[k].layers) for k in caches}
    name = lambda s: "default" if s == 0 else str(s)   # noqa: E731
    out = {"B": B, "context": ctx, "windows": {"calls": steps, "rounds": rounds}, "default_splits": int(lib.obte_attn_decode_splits(B, H, hs, ctx)),
           "cache_set_bytes": sets, "fp8_over_bf16_bytes": round(sets["fp8"] / sets["bf16"], 3),
           "served_from": {k: "HBM" if v > INFINITY_CACHE else "Infinity Cache (not an HBM measurement)" for k, v in sets.items()},
           "attention_bytes_per_call": nbytes,
           "attention_us": {k: {name(s): summary(us[(k, s)]) for s in counts} for k in caches},
           "attention_share_of_6.3TBps": {k: {name(s): round(nbytes[k] / (med[(k, s)] * 1e-6) / HBM_RATE, 3) for s in counts} for k in caches},
           "attention_fp8_over_bf16": {name(s): round(med[("fp8", s)] / med[("bf16", s)], 3) for s in counts},
           "decode_step_us": {k: summary(us[(k, "step")], 1) for k in caches},
           "decode_step_fp8_over_bf16": round(med[("fp8", "step")] / med[("bf16", "step")], 3)}
    return out


def kv8_unit_variance_deviation(dev, B=8, H=8, hs=128, T=2048):
    """what e4m3 does to one attention output on unit-variance q, k, v: |o_fp8 - o_bf16| against the bf16 cache's output"""
    from omnibiote_amd import ops
    C = H * hs
    qkv = torch.randn(B, T, 3 * C, device=dev, generator=torch.Generator(device=dev).manual_seed(2)).to(torch.bfloat16)
    bf, f8 = ops.kv_cache_buffer(B, T, H, hs, dev), ops.kv8_cache_buffer(B, T, H, hs, dev)
    ops.kv_cache_store(qkv, B, T, H, hs, bf, T, 0)
    ops.kv8_cache_store(qkv, B, T, H, hs, f8, T, 0)
    q = qkv[:, -1].contiguous()
    a, _ = ops.attn_decode(q, bf, B, T, T, H, hs, 8.0 / C)
    b, _ = ops.attn_decode_kv8(q, f8, B, T, T, H, hs, 8.0 / C)
    d = (a.float() - b.float()).abs()
    return {"unit_variance_attention": {"B": B, "H": H, "hs": hs, "keys": T, "max_abs_deviation": round(d.max().item(), 5),
                                        "mean_abs_deviation": round(d.mean().item(), 6), "rms_of_bf16_output": round(a.float().square().mean().sqrt().item(), 5)}}


def shared_compare(m, G, n_prefix, n_suffix, rounds, steps, dev):
    """G samples of one prompt: the shared-prefix cache against the replicated cache — the attention alone, decode_step, the prefill"""
    from omnibiote_amd import _lib
    from omnibiote_amd.model import KVCache, SharedPrefixCache
    lib = _lib.lib()
    H, C = m.config.n_head, m.config.n_embd
    hs, ctx = C // H, n_prefix + n_suffix
    g = torch.Generator(device=dev).manual_seed(G * 10007 + ctx)
    prompt = torch.randint(4, m.config.vocab_size, (1, n_prefix), device=dev, generator=g)
    rows = prompt.repeat_interleave(G, 0).contiguous()
    last = torch.randint(4, m.config.vocab_size, (G,), device=dev, generator=g)
    caches = {"replicated": KVCache(m, G, ctx), "shared": SharedPrefixCache(m, 1, G, n_prefix, n_suffix)}
    for kv in caches["replicated"].layers:                     # the rows' own positions hold finite values of the keys' size (only the time is read)
        kv.normal_()
    for _, suffix in caches["shared"].layers:
        suffix.normal_()
    prefill = {"replicated": lambda: m.prefill(rows, caches["replicated"]), "shared": lambda: m.prefill(prompt, caches["shared"])}
    q = torch.randn(G, 3 * C, device=dev, generator=torch.Generator(device=dev).manual_seed(1)).to(torch.bfloat16)
    ws = torch.empty(max(int(lib.obte_attn_decode_ws_bytes(G, H, hs)), int(lib.obte_attn_decode_shared_ws_bytes(1, G, H, hs, 0, 0))), dtype=torch.uint8, device=dev)
    o = torch.empty(G, C, device=dev, dtype=torch.bfloat16)
    lse = torch.empty(G, H, device=dev, dtype=torch.float32)
    stream = torch.cuda.current_stream().cuda_stream
    rep_ptrs = [kv.data_ptr() for kv in caches["replicated"].layers]
    sh_ptrs = [(a.data_ptr(), b.data_ptr()) for a, b in caches["shared"].layers]
    state = {"i": 0}

    def attn(kind):            # the C entry points themselves on preallocated outputs, each call on the next layer's cache
        state["i"] += 1
        if kind == "shared":
            pre, suf = sh_ptrs[state["i"] % len(sh_ptrs)]
            rc = lib.obte_attn_decode_shared(q.data_ptr(), 3 * C, pre, 1, n_prefix, n_prefix, suf, G, n_suffix, n_suffix, o.data_ptr(), lse.data_ptr(), H, hs,
                                             8.0 / C, 0, 0, ws.data_ptr(), ws.numel(), stream)
        else:
            rc = lib.obte_attn_decode(q.data_ptr(), 3 * C, rep_ptrs[state["i"] % len(rep_ptrs)], o.data_ptr(), lse.data_ptr(), G, ctx, ctx, H, hs, 8.0 / C, 0,
                                      ws.data_ptr(), ws.numel(), stream)
        if rc != 0:
            _lib.check(rc, "obte_attn_decode" + ("_shared" if kind == "shared" else ""))

    def step(kind):
        def fn():                    # the same position every time: the last suffix slot, the context stays ctx long
            caches[kind].reset(ctx - 1)
            m.decode_step(last, caches[kind])
        return fn
    for kind in caches:
        prefill[kind]()
    legs = {(kind, what): (step(kind) if what == "step" else (lambda kind=kind: attn(kind))) for what in ("attention", "step") for kind in caches}
    for key, fn in legs.items():
        for _ in range(3 if key[1] == "step" else 8):
            fn()
    us = {key: [] for key in legs}
    us.update({(kind, "prefill"): [] for kind in caches})
    for r in range(rounds):
        for key in (list(legs) if r % 2 == 0 else list(legs)[::-1]):
            us[key].append(timed(legs[key], steps))
        for kind in (list(caches) if r % 2 == 0 else list(caches)[::-1]):
            us[(kind, "prefill")].append(timed(prefill[kind], 1))
    med = {key: statistics.median(v) for key, v in us.items()}
    sets = {"replicated": sum(kv.numel() * 2 for kv in caches["replicated"].layers), "shared": sum(a.numel() * 2 + b.numel() * 2 for a, b in caches["shared"].layers)}
    nbytes = {"replicated": 4 * hs * G * H * ctx, "shared": 4 * hs * H * (-(-G // 32) * n_prefix + G * n_suffix)}
    out = {"P": 1, "G": G, "n_prefix": n_prefix, "n_suffix": n_suffix, "windows": {"calls": steps, "rounds": rounds, "prefills_per_window": 1},
           "splits": {"replicated": int(lib.obte_attn_decode_splits(G, H, hs, ctx)), "shared_prefix": int(lib.obte_attn_shared_prefix_splits(1, G, H, hs, n_prefix)),
                      "shared_suffix": int(lib.obte_attn_decode_splits(G, H, hs, n_suffix))},
           "cache_set_bytes": sets, "replicated_over_shared_set_bytes": round(sets["replicated"] / sets["shared"], 2),
           "served_from": {k: "HBM" if v > INFINITY_CACHE else "Infinity Cache (not an HBM measurement)" for k, v in sets.items()},
           "attention_bytes_per_call": nbytes, "replicated_over_shared_attention_bytes": round(nbytes["replicated"] / nbytes["shared"], 2)}
    for what, nd in (("attention", 2), ("step", 1), ("prefill", 1)):
        out[what + "_us"] = {k: summary(us[(k, what)], nd) for k in caches}
        out[what + "_replicated_over_shared"] = round(med[("replicated", what)] / med[("shared", what)], 2)
        gap = med[("replicated", what)] - med[("shared", what)]
        spreads = [max(us[(k, what)]) - min(us[(k, what)]) for k in caches]
        out[what + "_gap_us_and_spreads"] = [round(gap, 2)] + [round(v, 2) for v in spreads]
    return out


def _graph_nodes(record):
    """the kernel nodes of what ``record()`` launches, counted in a captured graph of its own that is never replayed (None if the runtime
    does not hand the graph out)"""
    import ctypes as C
    try:
        g = torch.cuda.CUDAGraph(keep_graph=True)
        with torch.cuda.graph(g):
            record()
        hip = C.CDLL(os.path.join(os.path.dirname(torch.__file__), "lib", "libamdhip64.so"))
        n = C.c_size_t(0)
        rc = hip.hipGraphGetNodes(C.c_void_p(g.raw_cuda_graph()), None, C.byref(n))
        return int(n.value) if rc == 0 else None
    except Exception as e:   # a count is a report, not a measurement the table depends on
        print(f"# graph node count unavailable: {type(e).__name__}: {e}", file=sys.stderr)
        return None


def graph_compare(m, B, ctx, rounds, steps, dev, constrained=False, penalized=False):
    """A generated token with sampling (T = 0.8, top_k = 200, top_p = 0.9) and an eos_token nobody draws, three ways, alternating in one
    process: today's loop (decode_step on the rows path + ops.sample_logits + the ragged host loop's bookkeeping, without its per-token host
    read), DecodeLoop eager and DecodeLoop captured (both read the positions once per 16 steps), and the captured loop with no eos_token
    (no host read at all).  Every window walks the same positions, ctx - 1 - steps .. ctx - 2, so every contender attends over the same
    keys; only run() / the steps are between the events.  ``constrained`` adds the captured loop under a restriction
    (include/omnibiote_hip_constrain.h): per-row masks that allow a random half of the vocabulary and a minimum length nobody reaches;
    ``penalized`` the captured loop under penalties 1.3 / 0.1 / 0.2 (include/omnibiote_hip_penalty.h) over the prompt and its own tokens."""
    import time
    from omnibiote_amd import ops
    from omnibiote_amd.model import DecodeLoop, KVCache, TokenPenalty
    V = m.config.vocab_size
    first = ctx - 1 - steps
    g = torch.Generator(device=dev).manual_seed(B * 10007 + ctx)
    idx = torch.randint(4, V, (B, first), device=dev, generator=g)
    us = torch.rand((steps + 1, B), device=dev, generator=g)
    setting = dict(temperature=0.8, top_k=200, top_p=0.9)
    eos = V                                                        # a valid "no row ever finishes": the bookkeeping runs, nothing parks
    caches = {k: KVCache(m, B, ctx) for k in ("eager", "device", "graph", "graph_no_eos") + (("graph_constrained",) if constrained else ())
              + (("graph_penalized",) if penalized else ())}
    logits0 = {k: m.prefill(idx, c, lengths=[first] * B) for k, c in caches.items()}
    loops, build_ms = {}, {}
    for k in list(caches)[1:]:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        extra = dict(allowed=ops.pack_token_mask(torch.rand((B, V), device=dev, generator=g) < 0.5), hold_min=steps + 1) if k == "graph_constrained" else {}
        if k == "graph_penalized":
            extra = dict(penalty=TokenPenalty.of("decode_bench", 1.3, 0.1, 0.2, steps + 1).bind(idx, None, own_buffer=False))
        loops[k] = DecodeLoop(m, caches[k], max_steps=steps + 1, uniforms=us, eos_token=None if k == "graph_no_eos" else eos, capture=k != "device", **setting,
                              **extra)
        torch.cuda.synchronize()
        build_ms[k] = round((time.perf_counter() - t0) * 1e3, 1)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    none_done = torch.zeros(B, dtype=torch.bool, device=dev)

    def eager_steps(cache, logits, n):
        done = none_done
        for i in range(n):
            nxt = ops.sample_logits(logits, us[i], **setting)
            valid = ~done                                          # noqa: F841 (the loop appends it)
            done = done | (nxt == eos)
            cache.park(done)
            logits = m.decode_step(nxt, cache)

    def window(k):
        cache = caches[k]
        if k == "eager":
            cache.reset(first, torch.full((B,), first, dtype=torch.int32, device=dev), first)
            torch.cuda.synchronize()
            e0.record()
            eager_steps(cache, logits0[k], steps)
        else:
            loops[k].positions.fill_(first)
            cache.reset(first, loops[k].positions, first)
            loops[k].start(logits0[k])
            torch.cuda.synchronize()
            e0.record()
            loops[k].run(steps)
        e1.record()
        e1.synchronize()
        assert cache.pos == ctx - 1
        return e0.elapsed_time(e1) / steps * 1e3
    legs = list(caches)
    for k in legs:
        window(k)
    usec = {k: [] for k in legs}
    for r in range(rounds):
        for k in (legs if r % 2 == 0 else legs[::-1]):
            usec[k].append(window(k))
    med = {k: statistics.median(v) for k, v in usec.items()}
    spread = {k: max(v) - min(v) for k, v in usec.items()}

    caches["eager"].reset(first, torch.full((B,), first, dtype=torch.int32, device=dev), first)

    def eager_once():                                              # (the window's set-up stays outside: one step's kernels alone)
        eager_steps(caches["eager"], logits0["eager"], 1)
    loops["device"].positions.fill_(first)
    caches["device"].reset(first, loops["device"].positions, first)
    nodes = {"eager_step": _graph_nodes(eager_once), "loop_body": _graph_nodes(loops["device"]._body)}
    out = {"B": B, "context": ctx, "setting": setting, "windows": {"steps": steps, "rounds": rounds, "positions": [first, ctx - 2]},
           "us_per_token": {k: summary(v, 1) for k, v in usec.items()},
           "eager_over": {k: round(med["eager"] / med[k], 2) for k in legs if k != "eager"},
           "gap_us_and_spreads": {k: [round(med["eager"] - med[k], 1), round(spread["eager"], 1), round(spread[k], 1)] for k in legs if k != "eager"},
           "tokens_per_s": {k: round(B / med[k] * 1e6) for k in legs},
           "loop_build_ms": build_ms, "kernel_nodes_per_step": nodes}
    return out


W8_ROWS = (1, 8, 64)


def w8_products(C_, rounds, steps, dev, mxfp4=False, rows=W8_ROWS):
    """obte_linear_small_m_w8 against obte_linear_small_m_bf16 alone at width C_, every call on the next distinct copy of the weight;
    ``mxfp4``: obte_linear_small_m_w4 as a third leg, the copies counted so that ITS set, the smallest, is 1.25 Infinity Caches"""
    import ctypes as C
    from omnibiote_amd import _lib, w4quant, w8quant
    lib, stream = _lib.lib(), torch.cuda.current_stream().cuda_stream
    gen = torch.Generator(device=dev).manual_seed(5)
    for name, N, K in (("c_attn", 3 * C_, C_), ("proj", C_, C_), ("fc", 4 * C_, C_), ("mlp", C_, 4 * C_), ("readout", 65536, C_)):
        copies = -(-(INFINITY_CACHE * 5 // 4) // (N * K // 2 if mxfp4 else N * K))   # the smallest set is 1.25 Infinity Caches
        w = torch.randn(N, K, device=dev, generator=gen).mul_(0.02).to(torch.bfloat16)
        codes, scales = w8quant.quantize_weight(w)
        ws = [w] + [w.clone() for _ in range(copies - 1)]
        cs = [codes] + [codes.clone() for _ in range(copies - 1)]
        ss = [scales] + [scales.clone() for _ in range(copies - 1)]
        if mxfp4:
            c4, s4 = w4quant.quantize_weight(w)
            cs4 = [c4] + [c4.clone() for _ in range(copies - 1)]
            ss4 = [s4] + [s4.clone() for _ in range(copies - 1)]
        strips, ch = -(-N // 16), K // 256 if K % 256 == 0 else 0
        out = {"width": C_, "product": name, "N": N, "K": K, "weight_copies": copies,
               "kernel": "x-stationary" if strips > 512 and ch in (1, 2, 4) else "one strip per workgroup",
               "set_bytes": {"bf16": copies * N * K * 2, "e4m3": copies * N * (K + 4)},
               "served_from": "HBM" if copies * N * K // (2 if mxfp4 else 1) > INFINITY_CACHE else "Infinity Cache (not an HBM measurement)",
               "byte_ratio": round((K + 4) / (2 * K), 4), "M": {}}
        if mxfp4:
            out["set_bytes"]["mxfp4"] = copies * N * (K // 2 + K // 32)
            out["mxfp4_byte_ratio_to_e4m3"] = round((K // 2 + K // 32) / (K + 4), 4)
        for M in rows:
            x = torch.randn(M, K, device=dev, generator=gen).to(torch.bfloat16)
            d = torch.empty(M, N, device=dev, dtype=torch.bfloat16)
            args = [_lib.GemmArgs(x.data_ptr(), wi.data_ptr(), d.data_ptr(), None, None, M, N, K, K, K, N, 1, 1, _lib.EPI_NONE, 1.0, 0.0, 0, 0) for wi in ws]
            state = {"i": 0}

            def bf16():
                state["i"] += 1
                rc = lib.obte_linear_small_m_bf16(C.byref(args[state["i"] % copies]), stream)
                if rc != 0:
                    _lib.check(rc, "obte_linear_small_m_bf16")

            def e4m3():
                state["i"] += 1
                i = state["i"] % copies
                rc = lib.obte_linear_small_m_w8(C.byref(args[i]), cs[i].data_ptr(), K, ss[i].data_ptr(), stream)
                if rc != 0:
                    _lib.check(rc, "obte_linear_small_m_w8")

            def fp4():
                state["i"] += 1
                i = state["i"] % copies
                rc = lib.obte_linear_small_m_w4(C.byref(args[i]), cs4[i].data_ptr(), K // 2, ss4[i].data_ptr(), K // 32, stream)
                if rc != 0:
                    _lib.check(rc, "obte_linear_small_m_w4")
            legs = {"bf16": bf16, "e4m3": e4m3, **({"mxfp4": fp4} if mxfp4 else {})}
            for fn in legs.values():
                for _ in range(8):
                    fn()
            us = {k: [] for k in legs}
            for r in range(rounds):
                for leg in (list(legs) if r % 2 == 0 else list(legs)[::-1]):
                    us[leg].append(timed(legs[leg], steps))
            med = {k: statistics.median(v) for k, v in us.items()}
            out["M"][str(M)] = {"us": {k: summary(v) for k, v in us.items()}, "e4m3_over_bf16": round(med["e4m3"] / med["bf16"], 3),
                                "gap_us_and_spreads": [round(med["bf16"] - med["e4m3"], 2)] + [round(max(v) - min(v), 2) for v in us.values()],
                                "share_of_6.3TBps": {"bf16": round(N * K * 2 / (med["bf16"] * 1e-6) / HBM_RATE, 3),
                                                     "e4m3": round(N * (K + 4) / (med["e4m3"] * 1e-6) / HBM_RATE, 3)}}
            if mxfp4:
                out["M"][str(M)]["mxfp4_over_e4m3"] = round(med["mxfp4"] / med["e4m3"], 3)
                out["M"][str(M)]["mxfp4_over_bf16"] = round(med["mxfp4"] / med["bf16"], 3)
                out["M"][str(M)]["share_of_6.3TBps"]["mxfp4"] = round(N * (K // 2 + K // 32) / (med["mxfp4"] * 1e-6) / HBM_RATE, 3)
        print(json.dumps(out), flush=True)
        if mxfp4:
            del cs4, ss4, c4, s4
        del ws, cs, ss, w, codes, scales
        torch.cuda.empty_cache()


def w8_tokens(m, wq, config, B, ctx, rounds, steps, dev, graph=False, wq4=None):
    """decode_step with and without weights=, alternating; ``graph``: also the captured DecodeLoop both ways; ``wq4``: the MXFP4 snapshot as
    a third leg of both"""
    from omnibiote_amd.model import DecodeLoop, KVCache
    g = torch.Generator(device=dev).manual_seed(B * 10007 + ctx)
    last = torch.randint(4, m.config.vocab_size, (B,), device=dev, generator=g)
    cache = KVCache(m, B, ctx)
    for kv in cache.layers:                                           # finite values of the keys' size: only the time is read
        kv.normal_()

    def step(weights):
        def fn():                    # the same position every time: the context stays ctx long
            cache.reset(ctx - 1)
            if weights is None:
                m.decode_step(last, cache)
            else:
                m.decode_step(last, cache, weights=weights)
        return fn
    legs = {"bf16": step(None), "e4m3": step(wq), **({"mxfp4": step(wq4)} if wq4 is not None else {})}
    for fn in legs.values():
        for _ in range(3):
            fn()
    us = {k: [] for k in legs}
    for r in range(rounds):
        for leg in (list(legs) if r % 2 == 0 else list(legs)[::-1]):
            us[leg].append(timed(legs[leg], steps))
    med = {k: statistics.median(v) for k, v in us.items()}
    out = {"config": config, "B": B, "context": ctx, "windows": {"decode_steps": steps, "rounds": rounds},
           "decode_step_us": {k: summary(v, 1) for k, v in us.items()}, "e4m3_over_bf16": round(med["e4m3"] / med["bf16"], 3),
           "gap_us_and_spreads": [round(med["bf16"] - med["e4m3"], 1)] + [round(max(v) - min(v), 1) for v in us.values()]}
    if wq4 is not None:
        out["mxfp4_over_e4m3"], out["mxfp4_over_bf16"] = round(med["mxfp4"] / med["e4m3"], 3), round(med["mxfp4"] / med["bf16"], 3)
    if graph:
        first = ctx - 1 - steps
        idx = torch.randint(4, m.config.vocab_size, (B, first), device=dev, generator=g)
        runs = {}
        for k, w in (("bf16", None), ("e4m3", wq)) + ((("mxfp4", wq4),) if wq4 is not None else ()):
            c = KVCache(m, B, ctx)
            extra = {} if w is None else {"weights": w}
            logits = m.prefill(idx, c, lengths=[first] * B, **extra)
            runs[k] = (c, logits, DecodeLoop(m, c, max_steps=steps + 1, capture=True, **extra))
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

        def window(k):
            c, logits, loop = runs[k]
            loop.positions.fill_(first)
            c.reset(first, loop.positions, first)
            loop.start(logits)
            torch.cuda.synchronize()
            e0.record()
            loop.run(steps)
            e1.record()
            e1.synchronize()
            return e0.elapsed_time(e1) / steps * 1e3
        for k in runs:
            window(k)
        gus = {k: [] for k in runs}
        for r in range(rounds):
            for k in (list(runs) if r % 2 == 0 else list(runs)[::-1]):
                gus[k].append(window(k))
        out["graph_loop_us_per_token"] = {k: summary(v, 1) for k, v in gus.items()}
        out["graph_loop_e4m3_over_bf16"] = round(statistics.median(gus["e4m3"]) / statistics.median(gus["bf16"]), 3)
        if wq4 is not None:
            out["graph_loop_mxfp4_over_e4m3"] = round(statistics.median(gus["mxfp4"]) / statistics.median(gus["e4m3"]), 3)
    return out


def w8_deviation(m, wq, dev, B=2, T0=20, steps=6):
    """what e4m3 weights do to the logits of this (randomly initialised) model: max |logit(weights=) - logit(bf16)| over a few steps"""
    from omnibiote_amd.model import KVCache
    idx = torch.randint(4, m.config.vocab_size, (B, T0), device=dev, generator=torch.Generator(device=dev).manual_seed(9))
    ca, cb = KVCache(m, B, T0 + steps), KVCache(m, B, T0 + steps)
    la, lb = m.prefill(idx, ca, weights=wq), m.prefill(idx, cb)
    worst, size = 0.0, 0.0
    for _ in range(steps):
        worst, size = max(worst, (la.float() - lb.float()).abs().max().item()), max(size, lb.float().abs().max().item())
        tok = lb.float().argmax(-1)
        la, lb = m.decode_step(tok, ca, weights=wq), m.decode_step(tok, cb)
    return {"max_abs_logit_deviation": round(worst, 4), "max_abs_logit": round(size, 4)}


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--batches", default=None, help="default 1,8,64 (--ragged: 8,64)")
    p.add_argument("--contexts", default=None, help="default 128,1024,2048 (--ragged: 2048)")
    p.add_argument("--ragged", action="store_true", help="the one-position-per-row step against the uniform step")
    p.add_argument("--small-m", action="store_true", help="the weight-streaming product against the tile structures: alone, and in a decode step")
    p.add_argument("--kv8", action="store_true", help="the e4m3 key/value cache against the bf16 cache: the attention alone, and decode_step")
    p.add_argument("--shared", action="store_true", help="G samples of one prompt: the shared-prefix cache against the replicated cache")
    p.add_argument("--graph", action="store_true", help="the device-resident token loop, eager and captured, against today's host-driven loop")
    p.add_argument("--constrained", action="store_true", help="with --graph: also the captured loop under per-row token masks and a minimum length")
    p.add_argument("--w8", action="store_true", help="e4m3 weights against bf16: the product alone, decode_step on the small and the large config")
    p.add_argument("--w8-part", default="products,small,large", help="with --w8 / --w4: which parts run")
    p.add_argument("--w4", action="store_true", help="--w8 with MXFP4 weights as a third leg of every comparison (products at M = 1 and 64)")
    p.add_argument("--penalized", action="store_true", help="with --graph: also the captured loop under repetition, presence and frequency penalties")
    p.add_argument("--rounds", type=int, default=5)
    p.add_argument("--steps", type=int, default=300, help="decode steps (and attention calls) per timed window")
    p.add_argument("--baseline_ms", type=float, default=400.0, help="the full forward's window: as many calls as fit, at least 3")
    p.add_argument("--sweep", default="1,2,4,8,16,32,64", help="forced split counts for obte_attn_decode alone")
    a = p.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    if a.w8 or a.w4:
        parts = a.w8_part.split(",")
        if "products" in parts:
            for C_ in (1024, 2048):
                w8_products(C_, a.rounds, a.steps, dev, mxfp4=a.w4, rows=(1, 64) if a.w4 else W8_ROWS)
        for config, kw in (("small", dict(n_layer=8, n_embd=1024, n_head=8)), ("large", dict(n_layer=24, n_embd=2048, n_head=16, on_device=True))):
            if config not in parts:
                continue
            m = build(2048, dev, **kw)
            wq = m.quantize_weights()
            wq4 = m.quantize_weights(format="mxfp4") if a.w4 else None
            print(json.dumps({"config": config, **w8_deviation(m, wq, dev)}), flush=True)
            if a.w4:
                print(json.dumps({"config": config, "format": "mxfp4", **w8_deviation(m, wq4, dev)}), flush=True)
            for B in (1, 8, 64):
                print(json.dumps(w8_tokens(m, wq, config, B, 2048, a.rounds, a.steps, dev, graph=B == 1, wq4=wq4)), flush=True)
                torch.cuda.empty_cache()
            del m, wq, wq4
            torch.cuda.empty_cache()
        return
    if a.graph:
        shapes = tuple((int(b), int(c)) for b in (a.batches or "1,8,64").split(",") for c in (a.contexts or "2048").split(","))
        m = build(max(c for _, c in shapes), dev)
        for B, ctx in shapes:
            print(json.dumps(graph_compare(m, B, ctx, a.rounds, a.steps, dev, a.constrained, a.penalized)), flush=True)
            torch.cuda.empty_cache()
        return
    if a.small_m:
        small_m_products(a.rounds, a.steps, dev)
        m = build(2048, dev)
        for B, ctx, ragged in ((1, 2048, False), (8, 2048, False), (8, 2048, True), (64, 1024, False), (64, 2048, False)):
            print(json.dumps(small_m_tokens(m, B, ctx, a.rounds, a.steps, dev, ragged)), flush=True)
            torch.cuda.empty_cache()
        return
    if a.shared:
        m = build(2048 + 256, dev)
        for G in (8, 64):
            for n_suffix in (1, 256):
                print(json.dumps(shared_compare(m, G, 2048, n_suffix, a.rounds, a.steps, dev)), flush=True)
                torch.cuda.empty_cache()
        return
    if a.kv8:
        shapes = ((8, 2048), (64, 1024), (64, 2048))
        if a.batches or a.contexts:
            shapes = tuple((int(b), int(c)) for b in (a.batches or "8,64").split(",") for c in (a.contexts or "2048").split(","))
        m = build(max(c for _, c in shapes), dev)
        sweep = [int(s) for s in a.sweep.split(",")]
        for B, ctx in shapes:
            print(json.dumps(kv8_compare(m, B, ctx, a.rounds, a.steps, sweep if (B, ctx) == (8, 2048) else [], dev)), flush=True)
            torch.cuda.empty_cache()
        print(json.dumps(kv8_unit_variance_deviation(dev)), flush=True)
        return
    contexts = [int(c) for c in (a.contexts or ("2048" if a.ragged else "128,1024,2048")).split(",")]
    batches = [int(b) for b in (a.batches or ("8,64" if a.ragged else "1,8,64")).split(",")]
    m = build(max(contexts), dev)
    sweep = [int(s) for s in a.sweep.split(",")]
    for B in batches:
        for ctx in contexts:
            if a.ragged:
                print(json.dumps(ragged_time(m, B, ctx, a.rounds, a.steps, dev)), flush=True)
                torch.cuda.empty_cache()
                continue
            us, cache, last, n_full = token_time(m, B, ctx, a.rounds, a.steps, a.baseline_ms, dev)
            d, f = statistics.median(us["decode_step"]), statistics.median(us["full_forward"])
            out = {"B": B, "context": ctx, "windows": {"decode_steps": a.steps, "full_forwards": n_full, "rounds": a.rounds},
                   "us_per_token": {k: summary(v, 1) for k, v in us.items()}, "full_forward_over_decode_step": round(f / d, 1),
                   "tokens_per_s_decode": round(B / d * 1e6),
                   "attn_decode": attention_alone(m, cache, B, ctx, a.rounds, a.steps, sweep, dev),
                   "step_split": step_split(m, cache, last, ctx, 20)}
            print(json.dumps(out), flush=True)
            del cache
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
