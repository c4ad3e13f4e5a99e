"""What --fp32_grad_accum costs: the headline configuration of bench.py (small, 128 rows, 8-row micro-batches, masked readout,
two streams) with the weight gradients summed in bf16 (default) and in fp32, ALTERNATING in one process after warm-up — the same
model, optimizer, batches and tuned plans, so what differs is the accumulation alone — and one block's weight-gradient launch
(the grouped launch of its four matrices beside dh1) three ways: OBTE_EPI_ADD (bf16 read-modify-write, the default),
OBTE_EPI_ACC32 (fp32 read-modify-write in the epilogue) and the unfused fallback (plain products to bf16 scratch, then
obte_acc32_add_bf16 per matrix).  Prints one JSON line.

    python tools/grad_accum_bench.py [--rounds 5] [--steps 3] [--micro_batches_per_pass 2] [--plan_cache plans.json]
"""
import argparse
import contextlib
import io
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def time_launch(fn, iters=20, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    us = sorted(a.elapsed_time(b) * 1e3 for a, b in ev)
    return {"median_us": round(us[len(us) // 2], 1), "min_us": round(us[0], 1), "max_us": round(us[-1], 1)}


def block_wgrad_three_ways(C, M, dev):
    """The block's grouped weight-gradient launch at n_embd C over M tokens (block.cpp, bwd_c_attn): fc, mlp, attn, proj + dh1."""
    from omnibiote_amd import _lib as L
    from omnibiote_amd import ops
    bf = torch.bfloat16
    r = lambda *s: (torch.randn(*s, device=dev) * 0.05).to(bf)
    dhpre, h2, dy, hact, dqkv, h1, dx1, y, w_attn = r(M, 4 * C), r(M, C), r(M, C), r(M, 4 * C), r(M, 3 * C), r(M, C), r(M, C), r(M, C), r(3 * C, C)
    shapes = [(4 * C, C), (C, 4 * C), (3 * C, C), (C, C)]
    pairs = [(dhpre, h2), (dy, hact), (dqkv, h1), (dx1, y)]
    grads = [torch.zeros(s, dtype=bf, device=dev) for s in shapes]
    scratch = [torch.empty(s, dtype=bf, device=dev) for s in shapes]
    acc32 = [torch.zeros(s, dtype=torch.float32, device=dev) for s in shapes]
    dh1 = torch.empty(M, C, dtype=bf, device=dev)
    side = dict(a=dqkv, b=w_attn, M=M, N=C, K=3 * C, out=dh1, a_kmajor=True)

    def group(extra):
        return [dict(a=a, b=b, M=s[0], N=s[1], K=M, **e) for (a, b), s, e in zip(pairs, shapes, extra)] + [side]

    add = lambda: ops.gemm_grouped(group([dict(out=g, accumulate=True) for g in grads]))
    fused = lambda: ops.gemm_grouped(group([dict(acc32=b, acc32_mode=L.ACC32_MORE) for b in acc32]))

    def unfused():
        ops.gemm_grouped(group([dict(out=t) for t in scratch]))
        for b, t in zip(acc32, scratch):
            ops.acc32_add_(b, t, L.ACC32_MORE)

    n = sum(s[0] * s[1] for s in shapes)
    return {"n_embd": C, "tokens": M, "weight_elements": n,
            "bytes_rmw": {"add_bf16": 4 * n, "acc32_fused": 8 * n, "acc32_unfused": 2 * n + 2 * n + 8 * n},
            "add_bf16": time_launch(add), "acc32_fused": time_launch(fused), "acc32_unfused": time_launch(unfused)}


def main():
    import bench
    p = argparse.ArgumentParser()
    p.add_argument("--rounds", type=int, default=5, help="alternations bf16 / fp32 after warm-up")
    p.add_argument("--steps", type=int, default=3, help="optimizer steps per setting and round")
    p.add_argument("--micro_batches_per_pass", type=int, default=2)
    p.add_argument("--plan_cache", default="")
    p.add_argument("--config", default="small", choices=sorted(bench.CONFIGS))
    p.add_argument("--no_step", action="store_true", help="only the block weight-gradient launch")
    a = p.parse_args()
    b = bench.parse([])                 # bench.py's defaults: the headline configuration
    b.config = a.config
    cfg = bench.CONFIGS[b.config]
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    from omnibiote_amd import _lib, tune
    from omnibiote_amd import train_encoder as TE
    _lib.lib()
    k = max(1, a.micro_batches_per_pass)
    rows_pass = k * b.mini_batch_size * cfg["ctx_len"]
    if a.plan_cache and os.path.exists(a.plan_cache):
        tune.load_plans(a.plan_cache)
    else:
        tune.tune_model_shapes(rows_pass, cfg["n_embd"], 2 ** 16, device=dev)
        if a.plan_cache:
            tune.save_plans(a.plan_cache)
    out = {"config": b.config, "rows_per_rank": b.rows_per_rank, "mini_batch_size": b.mini_batch_size, "micro_batches_per_pass": k,
           "pipeline_streams": b.pipeline_streams, "readout": b.readout}
    out["block_wgrad_launch"] = block_wgrad_three_ways(cfg["n_embd"], rows_pass, dev)
    if not a.no_step:
        h = bench.harness_args(cfg, b, 1)
        torch.manual_seed(1234)
        np.random.seed(1234)
        with contextlib.redirect_stdout(io.StringIO()):
            m = TE.build_model(h, dev)
        opt, sched = TE.build_optimizer(m, h, 1000)
        mk = lambda mode: TE.TrainStep(m, opt, sched, mini_batch_size=b.mini_batch_size, n_head=cfg["n_head"], lm_head_impl=b.readout,
                                       pipeline_streams=b.pipeline_streams, micro_batches_per_pass=k, backward_order=b.backward_order,
                                       grad_accum=mode)
        steps = {"bf16": mk("bf16"), "fp32": mk("fp32")}
        rng = np.random.default_rng(1234)
        host = [TE.synthetic_rows(b.rows_per_rank, cfg["ctx_len"], 2 ** 16, rng, single_document=not b.multi_document) for _ in range(4)]
        dev_b = [torch.from_numpy(x).to(dev) for x in host]
        for mode in ("bf16", "fp32"):           # warm-up: allocations, the fp32 buffers, both sets of kernels
            for i in range(2):
                steps[mode](dev_b[i], input_ids_host=host[i])
        torch.cuda.synchronize()
        ms = {"bf16": [], "fp32": []}
        for r in range(a.rounds):
            for mode in (("bf16", "fp32") if r % 2 == 0 else ("fp32", "bf16")):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for i in range(a.steps):
                    steps[mode](dev_b[(r + i) % 4], input_ids_host=host[(r + i) % 4])
                torch.cuda.synchronize()
                ms[mode].append((time.perf_counter() - t0) / a.steps * 1e3)
        summ = lambda v: {"median_ms": round(statistics.median(v), 3), "min_ms": round(min(v), 3), "max_ms": round(max(v), 3),
                          "runs_ms": [round(x, 3) for x in v]}
        out["step"] = {mode: summ(v) for mode, v in ms.items()}
        out["step"]["fp32_over_bf16"] = round(statistics.median(ms["fp32"]) / statistics.median(ms["bf16"]), 4)
        out["fp32_buffers_bytes"] = 4 * sum(p.numel() for n, p in m.named_parameters() if p.dim() == 2)
        out["max_memory_allocated_bytes"] = int(torch.cuda.max_memory_allocated())
    print(json.dumps(out))


if __name__ == "__main__":
    main()
