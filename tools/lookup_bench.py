"""Speculative decoding without a draft model on the small config (8 layers, 1024 wide, 8 heads of 128; bf16; vocabulary 65 536): what the
n-gram lookup draft and the point verification cost, what a lookup-and-verify round costs against plain decoding, and what the loop
yields on repetitive and on random prompts.  Contenders alternate in one process over --rounds rounds after warm-up; device events
around windows of calls; median and [min - max] over the rounds.  Every comparison is against a path that existed before the lookup.

  (a) obte_lookup_draft alone (ops.lookup_draft) at histories of 2048 and 8192 tokens, B in {1, 8}, k = 8: 4-symbol rows (every compare
      runs long) and random rows over the whole vocabulary (every compare stops at once).
  (b) ops.spec_verify_point against the route it replaces: filling a (B, k, V) one-hot bf16 q (a fill and a scatter into a reused
      buffer) and ops.spec_verify on it; V = 65 536, temperature 0.9 and top_k = 50.
  (c) one round — OmniBioTA.lookup_and_verify: the lookup, the target's extend over k + 1 tokens, the verification — against one
      decode_step plus ops.sample_logits, at --context, k in {4, 8, 16}; the break-even: the accepted tokens per round at which a round
      costs what plain decoding costs for the tokens it emits.
  (d) generate_lookup against generate (sampler="device") on two seeded prompt sets, period-12 tandem repeats and i.i.d. tokens:
      tokens per second and the acceptance rate.  The weights are random: the acceptance rate says little about a trained model —
      a random model continues a repeat no more readily than anything else; the round's cost and the break-even do not depend on it.
One JSON line per measurement.

    python tools/lookup_bench.py [--parts a,b,c,d] [--batches 1,8] [--ks 4,8,16] [--context 2048] [--new 128] [--rounds 5] [--steps 100]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from decode_bench import build, summary   # noqa: E402
from extend_bench import alternate        # noqa: E402

T, TOP_K = 0.9, 50


def lookup_alone(B, W, k, rounds, steps, dev):
    from omnibiote_amd import ops
    g = torch.Generator(device=dev).manual_seed(B * 100 + W)
    lens = torch.full((B,), W, dtype=torch.int32, device=dev)
    rows = {"four_symbols": (torch.randint(0, 4, (B, W), device=dev, generator=g), 4),
            "random_65536": (torch.randint(0, 2 ** 16, (B, W), device=dev, generator=g), 2 ** 16)}
    legs = {n: (lambda h=h, V=V: ops.lookup_draft(h, lens, k, (1, 4), V)) for n, (h, V) in rows.items()}
    us = alternate(legs, rounds, {n: steps for n in legs})
    print(json.dumps({"part": "a", "B": B, "history": W, "k": k, "ngram": [1, 4], "history_bytes": B * W * 8, "windows": {"calls": steps, "rounds": rounds},
                      "us": {n: summary(v) for n, v in us.items()}}), flush=True)


def verify_alone(B, k, V, rounds, steps, dev):
    from omnibiote_amd import ops
    g = torch.Generator(device=dev).manual_seed(B * 100 + k)
    p = (torch.randn(B, k + 1, V, device=dev, generator=g) * 2).to(torch.bfloat16)
    x = torch.where(torch.rand(B, k, device=dev, generator=g) < 0.5, p[:, :k].float().argmax(dim=2), torch.randint(0, V, (B, k), device=dev, generator=g))
    ua, ud = torch.rand(B, k, device=dev, generator=g), torch.rand(B, device=dev, generator=g)
    q = torch.empty(B, k, V, dtype=torch.bfloat16, device=dev)          # reused: the one-hot route pays the fill, not the allocation
    zero = torch.zeros(B, k, 1, dtype=torch.bfloat16, device=dev)

    def one_hot_route():
        q.fill_(float("-inf"))
        q.scatter_(2, x.unsqueeze(2), zero)
        return ops.spec_verify(p, q, x, ua, ud, T, TOP_K)
    legs = {"spec_verify_point": lambda: ops.spec_verify_point(p, x, ua, ud, T, TOP_K), "one_hot_fill+spec_verify": one_hot_route}
    us = alternate(legs, rounds, {n: steps for n in legs})
    med = {n: statistics.median(v) for n, v in us.items()}
    a, b = ops.spec_verify_point(p, x, ua, ud, T, TOP_K), one_hot_route()
    print(json.dumps({"part": "b", "B": B, "k": k, "V": V, "windows": {"calls": steps, "rounds": rounds}, "us": {n: summary(v) for n, v in us.items()},
                      "one_hot_route_over_point": round(med["one_hot_fill+spec_verify"] / med["spec_verify_point"], 2),
                      "same_integers": bool(torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])), "mean_accepted": round(float(a[0].float().mean()), 2)}),
          flush=True)


def one_round(m, B, ctx, k, rounds, steps, dev):
    from omnibiote_amd import ops
    from omnibiote_amd.model import KVCache
    g = torch.Generator(device=dev).manual_seed(B * 10007 + ctx)
    idx = torch.randint(4, m.config.vocab_size, (B, ctx), device=dev, generator=g)
    pos = ctx - k - 1
    cache = KVCache(m, B, ctx)
    m.prefill(idx[:, :pos], cache, lengths=[pos] * B, chunk=512)
    pending = idx[:, pos].contiguous()
    hist = idx[:, :pos + 1].contiguous()
    lens = torch.full((B,), pos + 1, dtype=torch.int32, device=dev)
    accepted = []

    def lookup_round():
        r = torch.rand(B * (k + 1), device=dev, generator=g)
        accepted.append(m.lookup_and_verify(pending, cache, hist, lens, k, (r[:B * k].view(B, k), r[B * k:]), T, TOP_K)[1])
        cache.rewind_rows([k + 1] * B, now=[pos + k + 1] * B)            # the same positions every time: the context stays ctx long

    def step_and_sample():
        ops.sample_logits(m.decode_step(pending, cache), torch.rand(B, device=dev, generator=g), T, TOP_K)
        cache.rewind_rows([1] * B, now=[pos + 1] * B)
    w = max(3, steps // 4)
    us = alternate({"round": lookup_round, "decode_step+sample": step_and_sample}, rounds, {"round": w, "decode_step+sample": w})
    med = {n: statistics.median(v) for n, v in us.items()}
    mean_a = float(torch.stack(accepted).float().mean())
    print(json.dumps({"part": "c", "B": B, "context": ctx, "k": k, "windows": {"calls": w, "rounds": rounds},
                      "us_per_call": {n: summary(v, 1) for n, v in us.items()},
                      "round_over_step": round(med["round"] / med["decode_step+sample"], 2),
                      "break_even_accepted_per_round": round(med["round"] / med["decode_step+sample"] - 1, 2),
                      "mean_accepted_random_weights": round(mean_a, 3)}), flush=True)
    del cache
    torch.cuda.empty_cache()


def loops(m, B, t0, new, k, rounds, dev):
    g = torch.Generator().manual_seed(B * 31 + t0)
    V = m.config.vocab_size
    unit = torch.randint(4, V, (B, 12), generator=g)
    prompts = {"period_12_repeats": unit.repeat(1, t0 // 12 + 1)[:, :t0].contiguous().to(dev), "iid_tokens": torch.randint(4, V, (B, t0), generator=g).to(dev)}
    for name, idx in prompts.items():
        stats = {}

        def lookup():
            out, s = m.generate_lookup(idx, new, k=k, temperature=T, top_k=TOP_K, generator=torch.Generator(device=dev).manual_seed(1), return_stats=True)
            stats.update(s)
            return out

        def plain():
            return m.generate(idx, new, temperature=T, top_k=TOP_K, generator=torch.Generator(device=dev).manual_seed(1), sampler="device")
        legs, secs = {"generate_lookup": lookup, "generate": plain}, {"generate_lookup": [], "generate": []}
        for fn in legs.values():
            fn()
        for r in range(rounds):
            for leg in (list(legs) if r % 2 == 0 else list(legs)[::-1]):
                torch.cuda.synchronize()
                t = time.perf_counter()
                legs[leg]()
                torch.cuda.synchronize()
                secs[leg].append(time.perf_counter() - t)
        tps = {n: [B * new / s for s in v] for n, v in secs.items()}
        print(json.dumps({"part": "d", "prompts": name, "B": B, "prompt_tokens": t0, "new_tokens": new, "k": k, "rounds_timed": rounds,
                          "tokens_per_s": {n: summary(v, 0) for n, v in tps.items()},
                          "lookup_over_generate": round(statistics.median(tps["generate_lookup"]) / statistics.median(tps["generate"]), 2),
                          "stats": stats, "acceptance_rate_random_weights": round(stats["accepted"] / max(stats["drafted"], 1), 3),
                          "matched_row_rounds": round(stats["matched"] * k / max(stats["drafted"], 1), 3)}), flush=True)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--parts", default="a,b,c,d")
    p.add_argument("--batches", default="1,8")
    p.add_argument("--ks", default="4,8,16", help="(b), (c)")
    p.add_argument("--context", type=int, default=2048, help="(c); (d) starts from a quarter of it")
    p.add_argument("--new", type=int, default=128, help="(d): new tokens per row")
    p.add_argument("--rounds", type=int, default=5)
    p.add_argument("--steps", type=int, default=100, help="calls per timed window")
    a = p.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    parts, ks, batches = a.parts.split(","), [int(k) for k in a.ks.split(",")], [int(b) for b in a.batches.split(",")]
    if "a" in parts:
        for B in batches:
            for W in (2048, 8192):
                lookup_alone(B, W, 8, a.rounds, a.steps, dev)
    if "b" in parts:
        for B in batches:
            for k in ks:
                verify_alone(B, k, 2 ** 16, a.rounds, a.steps, dev)
    if "c" in parts or "d" in parts:
        m = build(a.context, dev)
        for B in batches:
            for k in ks if "c" in parts else []:
                one_round(m, B, a.context, k, a.rounds, a.steps, dev)
        for B in batches if "d" in parts else []:
            loops(m, B, a.context // 4, a.new, 8, max(2, a.rounds // 2), dev)


if __name__ == "__main__":
    main()
