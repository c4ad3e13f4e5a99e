"""What choosing the next token costs: the torch sampler (model.sample_next) against the device sampler (ops.sample_logits, one launch of
obte_sample_logits_bf16), both alternating in one process over the same windows and rounds.  Vocabulary 65 536, B in {1, 8, 64};
settings: greedy; plain (T = 0.8); top_k = 200; top_p = 0.9; top_k = 200 with top_p = 0.9 (T = 0.8 throughout).

  (a) the sampler alone on one fixed (B, 65536) bf16 tensor of logits (randn * 2) — at most 8 MB, so the logits stay cache-resident in
      every window: this is the sampler's own cost, not a read of cold logits.  The device sampler's uniforms are drawn once outside
      the window, as generate() draws them once per call; the torch sampler draws inside multinomial.
  (b) a generated token: decode_step + the sampler on the step's own logits at B x 2048 on the small config (8 layers, 1024 wide), the
      cache holding 2047 positions, the same position every time.
Device events around windows of --steps calls, --rounds rounds after warm-up; median [min - max] in microseconds.  One JSON line per
(part, B).

    python tools/sample_bench.py [--batches 1,8,64] [--rounds 5] [--steps 300] [--part a|b|ab]

--constrained: what a restricted vocabulary costs (include/omnibiote_hip_constrain.h), the sampler alone as in (a), B in {1, 64} unless
--batches says otherwise, greedy and top_k = 200 with top_p = 0.9, half the vocabulary allowed.  Four contenders alternate: the
unconstrained call; the constrained call with one shared mask and with per-row masks; and what a caller had to do before — masked_fill
in torch into a second tensor, then the unconstrained call.  The expectation: constrained <= unconstrained (1 + 1/16) + the unconstrained
call's own spread — it reads V / 8 mask bytes on top of 2 V logits bytes — and below the masked_fill route.

    python tools/sample_bench.py --constrained [--batches 1,64] [--rounds 5] [--steps 300]

--penalized: what repetition, presence and frequency penalties cost (include/omnibiote_hip_penalty.h), the sampler alone as in (a), B in
{1, 64} unless --batches says otherwise, histories of 256 and 2048 tokens per row (half prompt, half generated, random ids), greedy and
top_k = 200 with top_p = 0.9, penalties 1.3 / 0.1 / 0.2.  Three contenders alternate: the unpenalised call; the penalised call; and what
a caller had to do before — gather / scatter on a copy of the logits in torch, then the unpenalised call.

    python tools/sample_bench.py --penalized [--batches 1,64] [--rounds 5] [--steps 300]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

VOCAB = 2 ** 16
SETTINGS = (("greedy", dict(temperature=0.8, top_k=1)), ("plain", dict(temperature=0.8)), ("top_k=200", dict(temperature=0.8, top_k=200)),
            ("top_p=0.9", dict(temperature=0.8, top_p=0.9)), ("top_k=200,top_p=0.9", dict(temperature=0.8, top_k=200, top_p=0.9)))


def summary(v, nd=1):
    return {"median": round(statistics.median(v), nd), "min": round(min(v), nd), "max": round(max(v), nd)}


def alternate(legs, rounds, steps, warm=5):
    from decode_bench import timed
    for fn in legs.values():
        for _ in range(warm):
            fn()
    us = {k: [] for k in legs}
    for r in range(rounds):
        for leg in (list(legs) if r % 2 == 0 else list(legs)[::-1]):
            us[leg].append(timed(legs[leg], steps))
    out = {k: summary(v) for k, v in us.items()}
    t, d = us["torch"], us["device"]
    out["torch_over_device"] = round(statistics.median(t) / statistics.median(d), 2)
    out["device_slower_beyond_both_spreads"] = statistics.median(d) - statistics.median(t) > (max(t) - min(t)) + (max(d) - min(d))
    return out


def samplers(logits_of, B, dev, kw, gen):
    from omnibiote_amd import ops
    from omnibiote_amd.model import sample_next
    u = torch.rand(B, device=dev, generator=gen)
    greedy = kw.get("top_k") == 1

    def torch_leg():
        return sample_next(logits_of(), kw["temperature"], kw.get("top_k"), gen, kw.get("top_p"))

    def device_leg():
        return ops.sample_logits(logits_of(), None if greedy else u, kw["temperature"], kw.get("top_k"), kw.get("top_p"))
    return {"torch": torch_leg, "device": device_leg}


def sampler_alone(B, rounds, steps, dev):
    gen = torch.Generator(device=dev).manual_seed(B)
    logits = (torch.randn(B, VOCAB, device=dev, generator=gen) * 2).to(torch.bfloat16)
    out = {"part": "sampler alone", "B": B, "V": VOCAB, "logits_bytes": logits.numel() * 2, "logits": "cache-resident (one fixed tensor)",
           "windows": {"calls": steps, "rounds": rounds}, "us": {}}
    for name, kw in SETTINGS:
        out["us"][name] = alternate(samplers(lambda: logits, B, dev, kw, gen), rounds, steps)
    return out


def constrained_compare(B, rounds, steps, dev):
    from decode_bench import timed
    from omnibiote_amd import ops
    gen = torch.Generator(device=dev).manual_seed(B + 1)
    logits = (torch.randn(B, VOCAB, device=dev, generator=gen) * 2).to(torch.bfloat16)
    u = torch.rand(B, device=dev, generator=gen)
    rows = torch.rand(B, VOCAB, device=dev, generator=gen) < 0.5
    shared, per_row = ops.pack_token_mask(rows[0].contiguous()), ops.pack_token_mask(rows)
    excluded = ~rows
    out = {"part": "constrained sampler alone", "B": B, "V": VOCAB, "allowed": "a random half", "windows": {"calls": steps, "rounds": rounds}, "us": {}}
    for name, kw in (SETTINGS[0], SETTINGS[4]):
        uu = None if kw.get("top_k") == 1 else u
        args = (kw["temperature"], kw.get("top_k"), kw.get("top_p"))
        legs = {"unconstrained": lambda: ops.sample_logits(logits, uu, *args),
                "constrained_shared": lambda: ops.sample_logits(logits, uu, *args, allowed_packed=shared),
                "constrained_per_row": lambda: ops.sample_logits(logits, uu, *args, allowed_packed=per_row),
                "masked_fill_then_unconstrained": lambda: ops.sample_logits(logits.masked_fill(excluded, float("-inf")), uu, *args)}
        for fn in legs.values():
            for _ in range(5):
                fn()
        us = {k: [] for k in legs}
        for r in range(rounds):
            for leg in (list(legs) if r % 2 == 0 else list(legs)[::-1]):
                us[leg].append(timed(legs[leg], steps))
        med = {k: statistics.median(v) for k, v in us.items()}
        res = {k: summary(v) for k, v in us.items()}
        bound = med["unconstrained"] * (1 + 1 / 16) + (max(us["unconstrained"]) - min(us["unconstrained"]))
        res["bound_unconstrained_plus_a_sixteenth_plus_its_spread"] = round(bound, 1)
        for k in ("constrained_shared", "constrained_per_row"):
            res[k + "_within_bound"] = med[k] <= bound
            res[k + "_beats_masked_fill"] = med[k] < med["masked_fill_then_unconstrained"]
        out["us"][name] = res
    return out


def penalized_compare(B, hist, rounds, steps, dev):
    from decode_bench import timed
    from omnibiote_amd import ops
    from omnibiote_amd.sampling import penalty_numbers
    gen = torch.Generator(device=dev).manual_seed(B + hist)
    logits = (torch.randn(B, VOCAB, device=dev, generator=gen) * 2).to(torch.bfloat16)
    u = torch.rand(B, device=dev, generator=gen)
    prompt, made = (torch.randint(0, VOCAB, (B, hist // 2), device=dev, generator=gen) for _ in range(2))
    both, ones = torch.cat([prompt, made], dim=1), torch.ones((B, hist // 2), device=dev)
    r, inv, pp, fp = penalty_numbers(1.3, 0.1, 0.2)
    pen = ops.Penalty(prompt, None, made, None, r, pp, fp)

    def torch_route(uu, args):                                     # the rule's effect in the fewest torch launches: not bit for bit the rule
        v = logits.gather(1, both).float()
        y = logits.scatter(1, both, torch.where(v < 0, v * r, v * inv).to(torch.bfloat16))
        cnt = torch.zeros((B, VOCAB), device=dev).scatter_add_(1, made, ones)
        y = torch.where(cnt > 0, (y.float() - (pp + fp * cnt)).to(torch.bfloat16), y)
        return ops.sample_logits(y, uu, *args)
    out = {"part": "penalized sampler alone", "B": B, "V": VOCAB, "history": {"prompt": hist // 2, "generated": hist // 2},
           "penalties": {"repetition": 1.3, "presence": 0.1, "frequency": 0.2}, "windows": {"calls": steps, "rounds": rounds}, "us": {}}
    for name, kw in (SETTINGS[0], SETTINGS[4]):
        uu = None if kw.get("top_k") == 1 else u
        args = (kw["temperature"], kw.get("top_k"), kw.get("top_p"))
        legs = {"unpenalized": lambda: ops.sample_logits(logits, uu, *args),
                "penalized": lambda: ops.sample_logits(logits, uu, *args, penalty=pen),
                "torch_route_then_unpenalized": lambda: torch_route(uu, args)}
        for fn in legs.values():
            for _ in range(5):
                fn()
        us = {k: [] for k in legs}
        for r_ in range(rounds):
            for leg in (list(legs) if r_ % 2 == 0 else list(legs)[::-1]):
                us[leg].append(timed(legs[leg], steps))
        med = {k: statistics.median(v) for k, v in us.items()}
        res = {k: summary(v) for k, v in us.items()}
        res["penalized_over_unpenalized"] = round(med["penalized"] / med["unpenalized"], 3)
        res["penalized_beats_torch_route"] = med["penalized"] < med["torch_route_then_unpenalized"]
        out["us"][name] = res
    return out


def generated_token(m, B, ctx, rounds, steps, dev):
    from omnibiote_amd.model import KVCache
    gen = torch.Generator(device=dev).manual_seed(B * 10007 + ctx)
    idx = torch.randint(4, m.config.vocab_size, (B, ctx), device=dev, generator=gen)
    cache = KVCache(m, B, ctx)
    m.prefill(idx[:, :ctx - 1], cache)
    last = idx[:, -1].contiguous()

    def step():                      # the same position every time: the context stays ctx long
        cache.pos = ctx - 1
        return m.decode_step(last, cache)
    out = {"part": "decode_step + sampler", "B": B, "context": ctx, "windows": {"steps": steps, "rounds": rounds}, "us": {}}
    from decode_bench import timed
    for _ in range(3):
        step()
    out["decode_step_alone_us"] = summary([timed(step, steps) for _ in range(rounds)])
    for name, kw in SETTINGS:
        out["us"][name] = alternate(samplers(step, B, dev, kw, gen), rounds, steps, warm=3)
    return out


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--batches", default=None, help="default 1,8,64 (--constrained, --penalized: 1,64)")
    p.add_argument("--constrained", action="store_true", help="the constrained sampler against the unconstrained one and the masked_fill route")
    p.add_argument("--penalized", action="store_true", help="the penalised sampler against the unpenalised one and the gather / scatter route")
    p.add_argument("--context", type=int, default=2048)
    p.add_argument("--rounds", type=int, default=5)
    p.add_argument("--steps", type=int, default=300)
    p.add_argument("--part", default="ab", choices=("a", "b", "ab"))
    a = p.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    batches = [int(b) for b in (a.batches or ("1,64" if a.constrained or a.penalized else "1,8,64")).split(",")]
    if a.penalized:
        for B in batches:
            for hist in (256, 2048):
                print(json.dumps(penalized_compare(B, hist, a.rounds, a.steps, dev)), flush=True)
        return
    if a.constrained:
        for B in batches:
            print(json.dumps(constrained_compare(B, a.rounds, a.steps, dev)), flush=True)
        return
    if "a" in a.part:
        for B in batches:
            print(json.dumps(sampler_alone(B, a.rounds, a.steps, dev)), flush=True)
    if "b" in a.part:
        from decode_bench import build
        m = build(a.context, dev)
        for B in batches:
            print(json.dumps(generated_token(m, B, a.context, a.rounds, a.steps, dev)), flush=True)
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
