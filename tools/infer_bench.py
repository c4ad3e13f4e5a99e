"""Forward-only throughput: tokens/s of model(idx, mask, return_embeddings=True) under torch.no_grad() — what the reference's
evaluation scripts and the trainer's evaluate() spend their time in — on the small config at 8 and 32 rows of T = 1024
(single-document rows), with OBTE_INFER=1 (ops.block_infer: nothing kept, the one-output GELU epilogue) and OBTE_INFER=0 (the
training forward, the path before the switch existed) ALTERNATING in one process after warm-up: same model, batch and tuned plans.
Beside it c_fc alone, OBTE_EPI_GELU against OBTE_EPI_GELU_ACT under the same plan, and torch.cuda.max_memory_allocated of a
forward on either path.  Prints one JSON line per row count and one for the epilogue pair.

    python tools/infer_bench.py [--rounds 7] [--iters 5] [--rows 8,32] [--config small] [--plan_cache plans.json]
(--plan_cache: one file per row count, plans.json.<rows>: loaded if present, else tuned and written)
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


def summary(v):
    return {"median": round(statistics.median(v), 3), "min": round(min(v), 3), "max": round(max(v), 3)}


def forward_legs(m, idx, mask, rounds, iters):
    """ms per forward on both paths, alternating (the order flipped every round), and the peak memory of one forward on each."""
    def run(n):
        with torch.no_grad():
            for _ in range(n):
                m(idx, attn_mask=mask, return_embeddings=True)
    ms, peak = {"1": [], "0": []}, {}
    for leg in ("1", "0"):                       # warm-up: allocations, both sets of kernels
        os.environ["OBTE_INFER"] = leg
        run(2)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        level = torch.cuda.memory_allocated()
        run(1)
        torch.cuda.synchronize()
        peak[leg] = int(torch.cuda.max_memory_allocated() - level)
    for r in range(rounds):
        for leg in (("1", "0") if r % 2 == 0 else ("0", "1")):
            os.environ["OBTE_INFER"] = leg
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run(iters)
            torch.cuda.synchronize()
            ms[leg].append((time.perf_counter() - t0) / iters * 1e3)
    os.environ.pop("OBTE_INFER", None)
    return ms, peak


def c_fc_pair(M, C, rounds, iters, dev):
    """c_fc [M, 4C] over K = C with either epilogue, alternating, HIP events around `iters` launches; both take the GELU plan."""
    from omnibiote_amd import _lib as L
    from omnibiote_amd import ops
    g = torch.Generator(device=dev).manual_seed(0)
    x = torch.randn(M, C, device=dev, generator=g).to(torch.bfloat16)
    w = (torch.randn(4 * C, C, device=dev, generator=g) * C ** -0.5).to(torch.bfloat16)
    out = torch.empty(M, 4 * C, device=dev, dtype=torch.bfloat16)
    us = {"gelu": [], "gelu_act": []}
    epi = {"gelu": L.EPI_GELU, "gelu_act": L.EPI_GELU_ACT}
    for k in epi:
        for _ in range(3):
            ops.gemm(x, w, M, 4 * C, C, True, True, epi[k], out=out)
    for r in range(rounds):
        for k in (("gelu", "gelu_act") if r % 2 == 0 else ("gelu_act", "gelu")):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            for _ in range(iters):
                ops.gemm(x, w, M, 4 * C, C, True, True, epi[k], out=out)   # (GELU allocates its second output per call, as in ops.linear_fwd)
            e1.record()
            e1.synchronize()
            us[k].append(e0.elapsed_time(e1) / iters * 1e3)
    flop = 2.0 * M * 4 * C * C
    return {"shape": [M, 4 * C, C], "us": {k: summary(v) for k, v in us.items()},
            "tflops_median": {k: round(flop / (statistics.median(v) * 1e-6) / 1e12, 1) for k, v in us.items()},
            "gelu_act_over_gelu": round(statistics.median(us["gelu_act"]) / statistics.median(us["gelu"]), 4)}


def main():
    import bench
    p = argparse.ArgumentParser()
    p.add_argument("--rounds", type=int, default=7, help="alternations OBTE_INFER=1 / 0 after warm-up")
    p.add_argument("--iters", type=int, default=5, help="forwards per leg and round")
    p.add_argument("--rows", default="8,32")
    p.add_argument("--config", default="small", choices=sorted(bench.CONFIGS))
    p.add_argument("--plan_cache", default="")
    a = p.parse_args()
    cfg = bench.CONFIGS[a.config]
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    from omnibiote_amd import _lib, tune
    from omnibiote_amd import train_encoder as TE
    from omnibiote_amd.masks import RangeMask
    _lib.lib()
    h = bench.harness_args(cfg, bench.parse([]), 1)
    with contextlib.redirect_stdout(io.StringIO()):
        m = TE.build_model(h, dev).eval()
    T, C = cfg["ctx_len"], cfg["n_embd"]
    rng = np.random.default_rng(1234)
    for rows in [int(r) for r in a.rows.split(",")]:
        cache = f"{a.plan_cache}.{rows}" if a.plan_cache else ""     # (the plans are per shape, so per row count)
        if cache and os.path.exists(cache):
            tune.load_plans(cache)
        else:
            tune.tune_model_shapes(rows * T, C, 2 ** 16, device=dev)
            if cache:
                tune.save_plans(cache)
        idx = torch.from_numpy(TE.synthetic_rows(rows, T, 2 ** 16, rng, single_document=True)).to(dev)
        mask = RangeMask.from_tokens(idx)
        ms, peak = forward_legs(m, idx, mask, a.rounds, a.iters)
        unit = rows * T * C * 2
        out = {"config": a.config, "rows": rows, "tokens": rows * T,
               "ms_per_forward": {"infer": summary(ms["1"]), "train_forward": summary(ms["0"])},
               "tokens_per_s_median": {"infer": round(rows * T / statistics.median(ms["1"]) * 1e3), "train_forward": round(rows * T / statistics.median(ms["0"]) * 1e3)},
               "infer_over_train_forward_time": round(statistics.median(ms["1"]) / statistics.median(ms["0"]), 4),
               "peak_bytes_over_level": {"infer": peak["1"], "train_forward": peak["0"]},
               "peak_in_activation_units": {"infer": round(peak["1"] / unit, 2), "train_forward": round(peak["0"] / unit, 2)}}
        print(json.dumps(out), flush=True)
        print(json.dumps({"c_fc": c_fc_pair(rows * T, C, a.rounds, 10, dev)}), flush=True)
        _lib.lib().obte_gemm_plan_clear()


if __name__ == "__main__":
    main()
