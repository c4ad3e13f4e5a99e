"""What a layer's attention maps cost: ops.attn_probs (obte_attn_probs, csrc/attention_probs.hip) at the small config's attention shape,
8 x 1024 tokens, 8 heads of 128, alternating in one process with ops.attn_fwd on the same operands.

    heads_fp32    (B, H, T, T) fp32:  268 MB stored per call
    heads_bf16    (B, H, T, T) bf16:  134 MB
    mean_fp32     (B, T, T) fp32, the heads' mean: 34 MB stored, the same two score passes over every head
    attn_fwd      the fused forward, which stores B T C bf16 and no weight

The per-head forms should be bound by their store (compare the rate with LayerNorm's in the README table), the head mean by its two
score passes.  Device events around windows of --steps calls, --rounds rounds after warm-up, the legs alternating; median [min - max] in
microseconds and the bytes of `out` stored per second.  Output and workspace are allocated once, outside the windows.  One JSON line per
mask form.

    python tools/probs_bench.py [--masks none,causal,dense] [--rounds 7] [--steps 50] [--B 8] [--T 1024] [--heads 8] [--hs 128]
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


def summary(v, nd=1):
    return {"median": round(statistics.median(v), nd), "min": round(min(v), nd), "max": round(max(v), nd)}


def mask_spec(kind, B, T, H, dev):
    from omnibiote_amd import ops
    from omnibiote_amd.masks import RangeMask
    if kind == "none":
        return None
    if kind == "causal":
        return ops.MaskSpec.from_user(RangeMask.causal(B, T, dev), B, T, H, dev)
    if kind == "dense":      # the reference's document mask as its (B, H, T, T) tensor, stride-0 heads: three documents per row
        doc = (torch.arange(T, device=dev) * 3 // T).view(1, T)
        m = torch.where(doc.view(1, T, 1) == doc.view(1, 1, T), 0.0, -1e9).to(torch.bfloat16).expand(B, T, T)
        return ops.MaskSpec.from_user(m.unsqueeze(1).expand(B, H, T, T), B, T, H, dev)
    raise SystemExit(f"unknown mask form {kind!r}")


def one(kind, B, T, H, hs, rounds, steps, dev):
    from decode_bench import timed
    from omnibiote_amd import ops
    C = H * hs
    gen = torch.Generator(device=dev).manual_seed(T + hs)
    qkv = torch.randn(B, T, 3 * C, device=dev, generator=gen).to(torch.bfloat16)
    scale = 8.0 / C
    spec = mask_spec(kind, B, T, H, dev)
    ws = ops.attn_probs_workspace(B, T, H, dev)
    outs = {"heads_fp32": torch.empty((B, H, T, T), dtype=torch.float32, device=dev),
            "heads_bf16": torch.empty((B, H, T, T), dtype=torch.bfloat16, device=dev),
            "mean_fp32": torch.empty((B, T, T), dtype=torch.float32, device=dev)}
    legs = {
        "heads_fp32": lambda: ops.attn_probs(qkv, B, T, H, hs, scale, spec, out=outs["heads_fp32"], ws=ws),
        "heads_bf16": lambda: ops.attn_probs(qkv, B, T, H, hs, scale, spec, dtype=torch.bfloat16, out=outs["heads_bf16"], ws=ws),
        "mean_fp32": lambda: ops.attn_probs(qkv, B, T, H, hs, scale, spec, heads="mean", out=outs["mean_fp32"], ws=ws),
        "attn_fwd": lambda: ops.attn_fwd(qkv, B, T, H, hs, scale, spec),
    }
    for fn in legs.values():
        for _ in range(3):
            fn()
    us = {k: [] for k in legs}
    for r in range(rounds):
        for leg in (list(legs) if r % 2 == 0 else list(legs)[::-1]):
            us[leg].append(timed(legs[leg], steps))
    res = {"mask": kind, "B": B, "T": T, "heads": H, "head_size": hs, "windows": {"calls": steps, "rounds": rounds},
           "us": {k: summary(v) for k, v in us.items()}}
    res["bytes_stored"] = {k: o.numel() * o.element_size() for k, o in outs.items()}
    res["TB_per_s_stored"] = {k: round(res["bytes_stored"][k] / statistics.median(us[k]) / 1e6, 3) for k in outs}
    # score flops of the two passes (2 B H T T hs each) per second, for the leg they bound
    res["mean_score_TFLOPs"] = round(2 * 2 * B * H * T * T * hs / statistics.median(us["mean_fp32"]) / 1e6, 1)
    return res


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--masks", default="none,causal,dense")
    p.add_argument("--rounds", type=int, default=7)
    p.add_argument("--steps", type=int, default=50)
    p.add_argument("--B", type=int, default=8)
    p.add_argument("--T", type=int, default=1024)
    p.add_argument("--heads", type=int, default=8)
    p.add_argument("--hs", type=int, default=128)
    a = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("probs_bench.py measures on the GPU; there is none here")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    for kind in a.masks.split(","):
        print(json.dumps(one(kind, a.B, a.T, a.heads, a.hs, a.rounds, a.steps, dev)), flush=True)


if __name__ == "__main__":
    main()
