"""Beam search on the small config (8 layers, 1024 wide, 8 heads of 128; bf16; V = 65 536): what the selection, the ancestry form of the
attention and a beam step cost.  Contenders alternate in one process over --rounds rounds after warm-up, device events around windows of
--steps calls; median and [min - max] over the rounds.  One JSON line per cell.

  (a) select     ops.beam_select (obte_beam_select_bf16: two launches, one read of the bf16 logits) against float log_softmax + topk over
                 (P, W V) in torch (with the parents', tokens' and ancestry's bookkeeping left out: the torch side is only the two passes),
                 at P x W = 1 x 8, 8 x 8, 2 x 32: time and the peak of newly allocated memory of one call.
  (b) attention  obte_attn_decode_beam with a random valid table against obte_attn_decode_shared on the same caches, and against
                 index_select of the suffix buffer by the step's parents followed by obte_attn_decode_shared — the copy a cache reorder
                 pays per layer and step — at n_prefix = 2048, n_suffix in {64, 256, 1024}, P x W = 8 x 8 and 2 x 32; every call on the next
                 of the per-layer caches.  `beam_loses` names a contender the ancestry form is slower than by more than both spreads.
  (c) token      one generate_beam token (select + embedding + block_decode_beam per layer + readout) against one generate(num_samples=W)
                 token with the device sampler (ops.sample_logits + decode_step), at n_prefix = 2048, suffix slot 255.

    python tools/beam_bench.py [--part select,attention,token] [--rounds 5] [--steps 200]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from decode_bench import build, summary, timed   # noqa: E402

V = 2 ** 16


def alternate(legs, rounds, steps, warm=5):
    for fn in legs.values():
        for _ in range(warm):
            fn()
    us = {k: [] for k in legs}
    for r in range(rounds):
        for k in (list(legs) if r % 2 == 0 else list(legs)[::-1]):
            us[k].append(timed(legs[k], steps))
    return us


def verdict(us, mine, others):
    """the contenders `mine` is slower than by more than both spreads"""
    med = {k: statistics.median(v) for k, v in us.items()}
    spread = {k: max(v) - min(v) for k, v in us.items()}
    return [k for k in others if med[mine] - med[k] > max(spread[mine], spread[k])]


def peak_new_bytes(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return int(torch.cuda.max_memory_allocated() - base)


def select_cell(P, W, rounds, steps, dev):
    from omnibiote_amd import ops
    B, n = P * W, 64
    g = torch.Generator(device=dev).manual_seed(B)
    logits = (torch.randn(B, V, device=dev, generator=g) * 2).to(torch.bfloat16)
    score = -torch.rand(B, device=dev, generator=g)
    done = torch.zeros(B, dtype=torch.uint8, device=dev)
    anc = [torch.randint(0, W, (B, n), device=dev, generator=g, dtype=torch.int32), torch.zeros((B, n), dtype=torch.int32, device=dev)]
    hist = torch.zeros((n, B), dtype=torch.int64, device=dev)
    parent, token = torch.empty(B, dtype=torch.int32, device=dev), torch.empty(B, dtype=torch.int64, device=dev)
    s_out, d_out = torch.empty_like(score), torch.empty_like(done)
    ws = ops.beam_select_workspace(P, W, dev)

    def hip():
        ops.beam_select(logits, score, done, anc[0], anc[1], hist, n // 2, W, parent=parent, token=token, score_out=s_out, done_out=d_out, ws=ws)

    def torch_two_passes():
        lp = torch.log_softmax(logits.float(), dim=-1) + score.view(B, 1)
        return torch.topk(lp.view(P, W * V), W, dim=-1)
    us = alternate({"beam_select": hip, "torch": torch_two_passes}, rounds, steps)
    med = {k: statistics.median(v) for k, v in us.items()}
    return {"part": "select", "P": P, "W": W, "V": V, "windows": {"calls": steps, "rounds": rounds}, "us": {k: summary(v) for k, v in us.items()},
            "torch_over_beam_select": round(med["torch"] / med["beam_select"], 2),
            "peak_new_bytes": {"beam_select": peak_new_bytes(hip), "torch": peak_new_bytes(torch_two_passes)},
            "logits_bytes_share_of_6.3TBps": round(B * V * 2 / (med["beam_select"] * 1e-6) / 6.3e12, 3), "beam_loses": verdict(us, "beam_select", ["torch"])}


def attention_cell(P, W, n_prefix, n_suffix, layers, rounds, steps, dev):
    from omnibiote_amd import _lib, ops
    lib = _lib.lib()
    H, hs = 8, 128
    C, B = H * hs, P * W
    g = torch.Generator(device=dev).manual_seed(B + n_suffix)
    prefixes = [ops.kv_cache_buffer(P, n_prefix, H, hs, dev).normal_() for _ in range(layers)]
    suffixes = [ops.kv_cache_buffer(B, n_suffix, H, hs, dev).normal_() for _ in range(layers)]
    gathered = torch.empty_like(suffixes[0])
    q = torch.randn(B, 3 * C, device=dev, generator=g).to(torch.bfloat16)
    table = torch.randint(0, W, (B, n_suffix), device=dev, generator=g, dtype=torch.int32)
    parents = (torch.arange(B, device=dev) // W * W + torch.randint(0, W, (B,), device=dev, generator=g)).repeat(2)   # the K rows, then the V rows
    parents[B:] += B
    o, lse = torch.empty(B, C, device=dev, dtype=torch.bfloat16), torch.empty(B, H, device=dev, dtype=torch.float32)
    ws = torch.empty(int(lib.obte_attn_decode_shared_ws_bytes(P, W, H, hs, 0, 0)), dtype=torch.uint8, device=dev)
    stream = torch.cuda.current_stream().cuda_stream
    state = {"i": 0}

    def shared(suffix=None):
        state["i"] += 1
        i = state["i"] % layers
        rc = lib.obte_attn_decode_shared(q.data_ptr(), 3 * C, prefixes[i].data_ptr(), P, n_prefix, n_prefix, (suffix if suffix is not None else suffixes[i]).data_ptr(),
                                         W, n_suffix, n_suffix, o.data_ptr(), lse.data_ptr(), H, hs, 8.0 / C, 0, 0, ws.data_ptr(), ws.numel(), stream)
        if rc != 0:
            _lib.check(rc, "obte_attn_decode_shared")

    def beam():
        state["i"] += 1
        i = state["i"] % layers
        rc = lib.obte_attn_decode_beam(q.data_ptr(), 3 * C, prefixes[i].data_ptr(), P, n_prefix, n_prefix, suffixes[i].data_ptr(), W, n_suffix, n_suffix,
                                       table.data_ptr(), o.data_ptr(), lse.data_ptr(), H, hs, 8.0 / C, 0, 0, ws.data_ptr(), ws.numel(), stream)
        if rc != 0:
            _lib.check(rc, "obte_attn_decode_beam")

    def gather_then_shared():
        i = (state["i"] + 1) % layers
        torch.index_select(suffixes[i].view(2 * B, -1), 0, parents, out=gathered.view(2 * B, -1))
        shared(gathered)
    us = alternate({"beam": beam, "shared": shared, "index_select_then_shared": gather_then_shared}, rounds, steps, warm=8)
    med = {k: statistics.median(v) for k, v in us.items()}
    suffix_bytes = suffixes[0].numel() * 2
    return {"part": "attention", "P": P, "W": W, "n_prefix": n_prefix, "n_suffix": n_suffix, "layers": layers, "windows": {"calls": steps, "rounds": rounds},
            "suffix_cache_bytes_per_layer": suffix_bytes, "us": {k: summary(v) for k, v in us.items()},
            "beam_over_shared": round(med["beam"] / med["shared"], 3), "gather_route_over_beam": round(med["index_select_then_shared"] / med["beam"], 2),
            "beam_loses": verdict(us, "beam", ["shared", "index_select_then_shared"])}


def token_cell(m, P, W, n_prefix, slot, rounds, steps, dev):
    from omnibiote_amd import ops
    from omnibiote_amd.model import SharedPrefixCache
    B, n = P * W, slot + 1
    g = torch.Generator(device=dev).manual_seed(B)
    prompt = torch.randint(4, V, (P, n_prefix), device=dev, generator=g)
    caches = {k: SharedPrefixCache(m, P, W, n_prefix, n) for k in ("beam", "sample")}
    logits = {k: m.prefill(prompt, c).clone() for k, c in caches.items()}
    for c in caches.values():
        for _, suffix in c.layers:
            suffix.normal_()
    score = -torch.rand(B, device=dev, generator=g)
    done = torch.zeros(B, dtype=torch.uint8, device=dev)
    anc = [torch.randint(0, W, (B, n), device=dev, generator=g, dtype=torch.int32), torch.zeros((B, n), dtype=torch.int32, device=dev)]
    hist = torch.zeros((n, B), dtype=torch.int64, device=dev)
    parent, token = torch.empty(B, dtype=torch.int32, device=dev), torch.empty(B, dtype=torch.int64, device=dev)
    s_out, d_out = torch.empty_like(score), torch.empty_like(done)
    ws = ops.beam_select_workspace(P, W, dev)
    u = torch.rand(B, device=dev, generator=g)
    wte = m.transformer.wte.weight

    def beam():                      # the same slot every time: the context stays n_prefix + slot + 1 long
        c = caches["beam"]
        ops.beam_select(logits["beam"], score, done, anc[0], anc[1], hist, slot, W, parent=parent, token=token, score_out=s_out, done_out=d_out, ws=ws)
        x = ops.embedding_fwd(token, wte)
        for block, (prefix, suffix) in zip(m.transformer.h, c.layers):
            ops.block_decode_beam(x, m._block_params(block), block.attn.rope(), m.config.n_head, prefix, P, c.prefix_len, c.n_prefix, suffix, c.max_new, slot,
                                  anc[1], ws=c.decode_ws, out=x)
        m._readout_rows(m.transformer.ln_f(x))

    def sample():
        c = caches["sample"]
        c.reset(n_prefix + slot)
        m.decode_step(ops.sample_logits(logits["sample"], u, temperature=0.8, top_k=200, top_p=0.9), c)
    us = alternate({"beam_token": beam, "sampled_token": sample}, rounds, steps, warm=3)
    med = {k: statistics.median(v) for k, v in us.items()}
    return {"part": "token", "P": P, "W": W, "n_prefix": n_prefix, "suffix_slot": slot, "windows": {"tokens": steps, "rounds": rounds},
            "us_per_token": {k: summary(v, 1) for k, v in us.items()}, "beam_over_sampled": round(med["beam_token"] / med["sampled_token"], 3),
            "beam_loses": verdict(us, "beam_token", ["sampled_token"])}


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--part", default="select,attention,token")
    p.add_argument("--rounds", type=int, default=5)
    p.add_argument("--steps", type=int, default=200)
    p.add_argument("--layers", type=int, default=8, help="(b): the per-layer caches a call walks through")
    a = p.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    parts = a.part.split(",")
    if "select" in parts:
        for P, W in ((1, 8), (8, 8), (2, 32)):
            print(json.dumps(select_cell(P, W, a.rounds, a.steps, dev)), flush=True)
            torch.cuda.empty_cache()
    if "attention" in parts:
        for P, W in ((8, 8), (2, 32)):
            for n_suffix in (64, 256, 1024):
                print(json.dumps(attention_cell(P, W, 2048, n_suffix, a.layers, a.rounds, a.steps, dev)), flush=True)
                torch.cuda.empty_cache()
    if "token" in parts:
        m = build(2048 + 256, dev)
        for P, W in ((1, 8), (8, 8), (2, 32)):
            print(json.dumps(token_cell(m, P, W, 2048, 255, a.rounds, a.steps, dev)), flush=True)
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
