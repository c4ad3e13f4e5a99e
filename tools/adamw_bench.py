"""Measurement: the optimizer step of one config's parameter tensors, reference-rounding kernel (obte_adamw_multi_bf16_ref, 14
bytes per parameter) beside the fp32-master kernel (obte_adamw_multi_master, 28 bytes per parameter), in the same run.
HIP-event timing around the launches of one step (no clipping: the update kernels alone), caches flushed before every
repetition as tune.py flushes them, best and median of the repetitions; prints microseconds and achieved TB/s for both and
the ratio of the bandwidths.  Also times step(max_norm=1.0) of both modes (norm + coefficient + update).

    python tools/adamw_bench.py [--config small] [--reps 10]
"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from omnibiote_amd import train_encoder as TE
from omnibiote_amd import tune
from omnibiote_amd.model import OmniBioTA, OmniBioTAConfig

CONFIGS = {"small": (8, 1024, 8), "large": (24, 2048, 16), "tiny": (2, 128, 2)}   # n_layer, n_embd, n_head (bench.py's)


def shapes_of(config: str):
    n_layer, n_embd, n_head = CONFIGS[config]
    c = OmniBioTAConfig()
    c.block_size, c.vocab_size, c.n_layer, c.n_head, c.n_embd, c.dropout, c.flash = 1024, 2 ** 16, n_layer, n_head, n_embd, 0.0, True
    with torch.device("meta"):
        m = OmniBioTA(c)
    return [tuple(p.shape) for p in m.parameters()]


def timed(opt, params, reps, max_norm):
    dev = params[0].device
    out = []
    for _ in range(reps + 2):
        for _ in range(4):   # 2 GiB written: the caches are cold, and the host has queued the whole step before the GPU reaches e0
            tune._flush_caches(dev)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        opt.step(max_norm=max_norm)
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1) * 1e3)
    return out[2:]   # the first two build the state and warm the code


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="small", choices=sorted(CONFIGS))
    ap.add_argument("--reps", type=int, default=10)
    a = ap.parse_args()
    shapes = shapes_of(a.config)
    n = sum(int(torch.Size(s).numel()) for s in shapes)
    print(f"{a.config}: {len(shapes)} tensors, {n / 1e6:.1f} M parameters, {-(-len(shapes) // 32)} launches per step")
    gen = torch.Generator(device="cuda").manual_seed(0)
    rows = {}
    for name, kw, bytes_per in (("reference rounding (bf16 state)", dict(), 14), ("master weights (fp32 state)", dict(master_weights=True), 28)):
        ps = [torch.nn.Parameter((torch.randn(s, device="cuda", generator=gen) * 0.02).to(torch.bfloat16)) for s in shapes]
        for p in ps:
            p.grad = (torch.randn(p.shape, device="cuda", generator=gen) * 1e-3).to(torch.bfloat16)
        opt = TE.FusedAdamW(ps, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, **kw)
        for what, max_norm, b in (("update", None, bytes_per), ("clip + update", 1.0, bytes_per + 2)):
            us = timed(opt, ps, a.reps, max_norm)
            best, med = min(us), statistics.median(us)
            rows[(name, what)] = best
            print(f"{name:34s} {what:14s} best {best:8.1f} us  median {med:8.1f} us   {b} B/param -> {n * b / best / 1e6:6.2f} TB/s (best)")
        del opt, ps
        torch.cuda.empty_cache()
    r, m = rows[("reference rounding (bf16 state)", "update")], rows[("master weights (fp32 state)", "update")]
    print(f"update alone: master / reference time {m / r:.2f}x (2.00x at equal bandwidth); bandwidth master / reference {(28 / m) / (14 / r):.2f}")


if __name__ == "__main__":
    main()
