"""What a log-probability costs: the fused readout + log-softmax (ops.readout_score, obte_readout_score_bf16) against the two routes that
materialise the (R, V) logits, all alternating in one process over the same windows and rounds.

  (a) the readout alone, x (R, C) ~ N(0, 1) and w (V, C) ~ 0.02 N(0, 1) in bf16, V = 65 536, one target per row (K = 1):
        fused        ops.readout_score
        softmax      ops.linear_fwd, then log_softmax in float and a gather, in torch
        masked_ce    ops.linear_fwd, then ops.masked_ce_rows: the route train_encoder.evaluate takes today (it writes a gradient too)
      with every contender's peak of allocated bytes above the operands during one call.
  (b) the model: OmniBioTA.score(idx) against ops.next_token_loss(model(idx), idx) on the small config (8 layers, 1024 wide) at 8 x 1024,
      and the forward in front of either readout: with score()'s row list (all but every row's last position) and without one.
Device events around windows of --steps calls, --rounds rounds after warm-up; median [min - max] in microseconds.  One JSON line per
shape.  The fused call does the product's 2 R V C flops on the first tile structure's two-stage loop, not on the tuned structures
linear_fwd resolves to, and saves about 2 R V 2 bytes of logits traffic: which effect wins where is what this measures.

    python tools/score_bench.py [--rows 1024,8192] [--widths 1024,2048] [--rounds 5] [--steps 100] [--part a|b|ab]
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


def summary(v, nd=1):
    return {"median": round(statistics.median(v), nd), "min": round(min(v), nd), "max": round(max(v), nd)}


def alternate(legs, rounds, steps, warm=3):
    from decode_bench import timed
    for fn in legs.values():
        for _ in range(warm):
            fn()
    us = {k: [] for k in legs}
    for r in range(rounds):
        for leg in (list(legs) if r % 2 == 0 else list(legs)[::-1]):
            us[leg].append(timed(legs[leg], steps))
    out = {k: summary(v) for k, v in us.items()}
    first = next(iter(legs))
    for k in list(legs)[1:]:
        out[f"{k}_over_{first}"] = round(statistics.median(us[k]) / statistics.median(us[first]), 2)
    return out


def peak_above(fn):
    """peak of allocated bytes during one call of fn, above what was allocated before it"""
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    keep = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    del keep
    return peak


def readout_alone(R, Cc, rounds, steps, dev):
    from omnibiote_amd import _lib, ops
    gen = torch.Generator(device=dev).manual_seed(R + Cc)
    x = torch.randn(R, Cc, device=dev, generator=gen).to(torch.bfloat16)
    w = (0.02 * torch.randn(VOCAB, Cc, device=dev, generator=gen)).to(torch.bfloat16)
    t = torch.randint(0, VOCAB, (R,), device=dev, generator=gen)

    def fused():
        return ops.readout_score(x, w, t)[0]

    def softmax():
        return torch.log_softmax(ops.linear_fwd(x, w).float(), dim=-1).gather(1, t.unsqueeze(1))

    def masked_ce():
        return ops.masked_ce_rows(ops.linear_fwd(x, w), t, None, 1)[0]
    legs = {"fused": fused, "softmax": softmax, "masked_ce": masked_ce}
    out = {"part": "readout alone", "R": R, "V": VOCAB, "C": Cc, "K": 1, "slices": _lib.lib().obte_readout_score_slices(R, VOCAB),
           "logits_bytes": R * VOCAB * 2, "windows": {"calls": steps, "rounds": rounds},
           "peak_bytes_above_operands": {k: peak_above(fn) for k, fn in legs.items()}}
    out["us"] = alternate(legs, rounds, steps)
    out["tflops_fused"] = round(2 * R * VOCAB * Cc / out["us"]["fused"]["median"] / 1e6, 1)
    return out


def model_score(rounds, steps, dev, B=8, T=1024):
    from decode_bench import build
    from omnibiote_amd import ops
    m = build(T, dev)
    idx = torch.randint(4, VOCAB, (B, T), device=dev, generator=torch.Generator(device=dev).manual_seed(1))

    def score():
        return m.score(idx).total

    def logits_loss():
        with torch.no_grad():
            return ops.next_token_loss(m(idx), idx)
    rows = (torch.arange(B, device=dev).view(B, 1) * T + torch.arange(T - 1, device=dev).view(1, T - 1)).reshape(-1)

    def embeddings_rows():          # what score() runs in front of the readout, and the same without the row list
        with torch.no_grad():
            return m(idx, return_embeddings=True, rows=rows)

    def embeddings_all():
        with torch.no_grad():
            return m(idx, return_embeddings=True)
    legs = {"score": score, "logits_loss": logits_loss, "embeddings_rows": embeddings_rows, "embeddings_all": embeddings_all}
    out = {"part": "model", "config": "small (8 layers, 1024 wide)", "B": B, "T": T, "windows": {"calls": steps, "rounds": rounds},
           "peak_bytes_above_model_and_tokens": {k: peak_above(fn) for k, fn in legs.items()}}
    out["us"] = alternate(legs, rounds, steps)
    a, b = -(score().double().sum() / (B * (T - 1))).item(), logits_loss().item()
    out["mean_loss"] = {"score": round(a, 5), "logits_loss": round(b, 5)}
    return out


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--rows", default="1024,8192")
    p.add_argument("--widths", default="1024,2048")
    p.add_argument("--rounds", type=int, default=5)
    p.add_argument("--steps", type=int, default=100)
    p.add_argument("--part", default="ab", choices=("a", "b", "ab"))
    a = p.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    if "a" in a.part:
        for Cc in (int(v) for v in a.widths.split(",")):
            for R in (int(v) for v in a.rows.split(",")):
                print(json.dumps(readout_alone(R, Cc, a.rounds, a.steps, dev)), flush=True)
                torch.cuda.empty_cache()
    if "b" in a.part:
        print(json.dumps(model_score(a.rounds, a.steps, dev)), flush=True)


if __name__ == "__main__":
    main()
