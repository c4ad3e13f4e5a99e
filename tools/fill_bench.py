"""What a drawn token costs: the fused readout + Gumbel-max draw (ops.readout_sample, obte_readout_sample_bf16) against the route that
materialises the (R, V) logits, alternating in one process over the same windows and rounds.

  (a) the readout alone, x (R, C) ~ N(0, 1) and w (V, C) ~ 0.02 N(0, 1) in bf16, V = 65 536, temperature 0.8, no truncation:
        fused         ops.readout_sample
        materialised  ops.linear_fwd, then ops.sample_logits against uniforms
      with either route's peak of allocated bytes above the operands during one call.
  (b) the model: one iteration of OmniBioTA.infill (steps = 1: forward on the masked rows, fused draw, commit) on the small config
      (8 layers, 1024 wide) at 8 x 1024 with 15 % and with 100 % of the positions masked, against the forward on those rows alone.
Device events around windows of --steps calls, --rounds rounds after warm-up; median [min - max] in microseconds.  One JSON line per cell.

    python tools/fill_bench.py [--rows 1024,8192,19200] [--widths 1024,2048] [--rounds 5] [--steps 100] [--part a|b|ab]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from score_bench import VOCAB, alternate, peak_above  # noqa: E402

TEMPERATURE = 0.8


def readout_alone(R, Cc, rounds, steps, dev):
    from omnibiote_amd import _lib, ops
    gen = torch.Generator(device=dev).manual_seed(R + Cc)
    x = torch.randn(R, Cc, device=dev, generator=gen).to(torch.bfloat16)
    w = (0.02 * torch.randn(VOCAB, Cc, device=dev, generator=gen)).to(torch.bfloat16)
    keys = torch.arange(R, device=dev)
    u = torch.rand(R, device=dev, generator=gen)

    def fused():
        return ops.readout_sample(x, w, TEMPERATURE, 17, keys=keys)[0]

    def materialised():
        return ops.sample_logits(ops.linear_fwd(x, w), u, temperature=TEMPERATURE)
    legs = {"fused": fused, "materialised": materialised}
    out = {"part": "readout alone", "R": R, "V": VOCAB, "C": Cc, "slices": _lib.lib().obte_readout_sample_slices(R, VOCAB),
           "logits_bytes": R * VOCAB * 2, "windows": {"calls": steps, "rounds": rounds},
           "peak_bytes_above_operands": {k: peak_above(fn) for k, fn in legs.items()}}
    out["us"] = alternate(legs, rounds, steps)
    out["tflops_fused"] = round(2 * R * VOCAB * Cc / out["us"]["fused"]["median"] / 1e6, 1)
    return out


def model_infill(fraction, rounds, steps, dev, B=8, T=1024):
    from decode_bench import build
    m = build(T, dev)
    m.config.autoregressive = False                      # the same weights as an encoder: full attention
    for block in m.transformer.h:
        block.attn.autoregressive = False
    gen = torch.Generator(device=dev).manual_seed(2)
    idx = torch.randint(4, VOCAB, (B, T), device=dev, generator=gen)
    masked = torch.rand(B, T, device=dev, generator=gen) < fraction if fraction < 1 else torch.ones(B, T, dtype=torch.bool, device=dev)
    start = idx.masked_fill(masked, 2)
    rows = masked.flatten().nonzero().flatten()

    def infill():
        return m.infill(idx, masked, steps=1, temperature=TEMPERATURE, seed=3)[0]

    def forward_rows():
        with torch.no_grad():
            return m(start, return_embeddings=True, rows=rows)
    legs = {"infill": infill, "forward_rows": forward_rows}
    out = {"part": "model", "config": "small (8 layers, 1024 wide)", "B": B, "T": T, "masked": int(rows.numel()), "fraction": fraction,
           "windows": {"calls": steps, "rounds": rounds}, "peak_bytes_above_model_and_tokens": {k: peak_above(fn) for k, fn in legs.items()}}
    out["us"] = alternate(legs, rounds, steps)
    return out


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--rows", default="1024,8192,19200")
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
        for fraction in (0.15, 1.0):
            print(json.dumps(model_infill(fraction, a.rounds, a.steps, dev)), flush=True)


if __name__ == "__main__":
    main()
