"""What the next-token objective and distillation cost.  Contenders ALTERNATE in one process after warm-up (same tuned plans, same
batches); every figure is a median with its [min-max] over the rounds.  Prints one JSON line.

  (a) the CLM step against the MLM step at bench.py's headline configuration (small, ctx 1024, 128 rows in micro-batches of 8, four per
      pass, two streams): tokens/s of both and the rows each readout pass runs on — MLM scores ~15 % of the positions, CLM nearly all.
  (b) obte_distill_ce_rows alone at 8192 x 65 536 against the torch route (two float log_softmax, kl_div, cross_entropy, autograd):
      us per call, and the fraction of 3 * rows * V * 2 bytes (two rows read, one written) at the HBM rate the README quotes for the
      CE kernel.
  (c) a distilled step (a teacher of the student's size) against the plain CLM step.

    python tools/clm_bench.py [--rounds 5] [--steps 2] [--kernel_rows 8192] [--plan_cache plans.json] [--only a|b|c]
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

CE_HBM_TBS = 5.5      # README, "CE 5.5 TB/s": what masked_ce_rows reaches inside the step


def summ(v, unit, digits=1):
    return {f"median_{unit}": round(statistics.median(v), digits), f"min_{unit}": round(min(v), digits), f"max_{unit}": round(max(v), digits)}


def alternate(contenders, rounds, run):
    """contenders: {name: object}; run(object) -> a figure for one window.  Round r runs them in order, round r + 1 in reverse."""
    names = list(contenders)
    out = {n: [] for n in names}
    for r in range(rounds):
        for n in (names if r % 2 == 0 else names[::-1]):
            out[n].append(run(contenders[n]))
    return out


def kernel_alone(rows, V, rounds, dev):
    import torch.nn.functional as F
    from omnibiote_amd import ops
    g = torch.Generator(device=dev).manual_seed(0)
    s = (torch.randn(rows, V, device=dev, generator=g) * 1.5).to(torch.bfloat16)
    t = (s.float() + 0.5 * torch.randn(rows, V, device=dev, generator=g)).to(torch.bfloat16)
    tgt = torch.randint(0, V, (rows,), device=dev, generator=g)
    alpha, temp = 0.5, 2.0

    def hip():
        ops.distill_ce_rows(s, t, tgt, 1, None, alpha, temp)

    def torch_route():
        x = s.detach().requires_grad_(True)
        ls = F.log_softmax(x.float() / temp, dim=-1)
        lt = F.log_softmax(t.float() / temp, dim=-1)
        loss = alpha * F.cross_entropy(x.float(), tgt) + (1 - alpha) * temp * temp * F.kl_div(ls, lt, reduction="batchmean", log_target=True)
        loss.backward()

    def window(fn, calls=5):
        fn(); torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(calls):
            fn()
        e1.record(); e1.synchronize()
        return e0.elapsed_time(e1) * 1e3 / calls

    us = alternate({"hip": hip, "torch": torch_route}, rounds, window)
    torch.cuda.reset_peak_memory_stats()
    hip(); torch.cuda.synchronize()
    peak_hip = torch.cuda.max_memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    torch_route(); torch.cuda.synchronize()
    peak_torch = torch.cuda.max_memory_allocated()
    byts = 3.0 * rows * V * 2
    med = statistics.median(us["hip"])
    return {"rows": rows, "vocab": V, "alpha": alpha, "temperature": temp, "calls_per_window": 5,
            "hip_us": summ(us["hip"], "us"), "torch_us": summ(us["torch"], "us"),
            "torch_over_hip": round(statistics.median(us["torch"]) / med, 2),
            "algorithmic_bytes": byts, "hip_tb_per_s": round(byts / med / 1e6, 2),
            "fraction_of_ce_hbm_rate": round(byts / med / 1e6 / CE_HBM_TBS, 3), "ce_hbm_rate_tb_per_s": CE_HBM_TBS,
            "peak_bytes_hip": int(peak_hip), "peak_bytes_torch": int(peak_torch)}


def main():
    import bench
    p = argparse.ArgumentParser()
    p.add_argument("--rounds", type=int, default=5)
    p.add_argument("--steps", type=int, default=2, help="optimizer steps per contender and round")
    p.add_argument("--kernel_rows", type=int, default=8192)
    p.add_argument("--micro_batches_per_pass", type=int, default=4)
    p.add_argument("--plan_cache", default="")
    p.add_argument("--config", default="small", choices=sorted(bench.CONFIGS))
    p.add_argument("--only", default="", choices=["", "a", "b", "c"])
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
    out = {"config": b.config, "rows_per_rank": b.rows_per_rank, "mini_batch_size": b.mini_batch_size, "micro_batches_per_pass": k,
           "pipeline_streams": b.pipeline_streams, "rounds": a.rounds, "steps_per_window": a.steps}
    if a.only in ("", "b"):
        out["distill_kernel"] = kernel_alone(a.kernel_rows, 2 ** 16, a.rounds, dev)
    if a.only in ("", "a", "c"):
        if a.plan_cache and os.path.exists(a.plan_cache):
            tune.load_plans(a.plan_cache)
        else:
            tune.tune_model_shapes(k * b.mini_batch_size * cfg["ctx_len"], cfg["n_embd"], 2 ** 16, device=dev)
            if a.plan_cache:
                tune.save_plans(a.plan_cache)
        T = cfg["ctx_len"]
        rng = np.random.default_rng(1234)
        host = [TE.synthetic_rows(b.rows_per_rank, T, 2 ** 16, rng, single_document=not b.multi_document) for _ in range(2)]
        dev_b = [torch.from_numpy(x).to(dev) for x in host]
        tokens = b.rows_per_rank * T

        def model_and_step(objective, teacher=None):
            h = bench.harness_args(cfg, b, 1)
            h.objective = objective
            torch.manual_seed(1234)
            np.random.seed(1234)
            with contextlib.redirect_stdout(io.StringIO()):
                m = TE.build_model(h, dev)
            opt, sched = TE.build_optimizer(m, h, 1000)
            return m, TE.TrainStep(m, opt, sched, mini_batch_size=b.mini_batch_size, n_head=cfg["n_head"], lm_head_impl="masked",
                                   pipeline_streams=b.pipeline_streams, micro_batches_per_pass=k, backward_order=b.backward_order,
                                   objective=objective, teacher=teacher)

        def window(step):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for i in range(a.steps):
                step(dev_b[i % 2], input_ids_host=host[i % 2])
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) / a.steps * 1e3

        def compare(steps):
            for s in steps.values():      # warm-up: allocations, both sets of kernels
                window(s)
            ms = alternate(steps, a.rounds, window)
            res = {n: dict(summ(v, "ms", 2), tokens_per_s=round(tokens / statistics.median(v) * 1e3)) for n, v in ms.items()}
            names = list(steps)
            res[f"{names[1]}_over_{names[0]}"] = round(statistics.median(ms[names[1]]) / statistics.median(ms[names[0]]), 3)
            return res

        _, clm = model_and_step("clm")
        if a.only in ("", "a"):
            _, mlm = model_and_step("mlm")
            out["clm_vs_mlm_step"] = compare({"mlm": mlm, "clm": clm})
            rows_mlm = sum(int(r.numel()) for r in mlm._mask_rows_host)
            rows_clm = sum(int(r.numel()) for r in clm._mask_rows_host)
            out["clm_vs_mlm_step"]["readout_rows_per_step"] = {"mlm": rows_mlm, "clm": rows_clm, "ratio": round(rows_clm / max(rows_mlm, 1), 2)}
            del mlm
        if a.only in ("", "c"):
            teacher, _ = model_and_step("clm")
            _, distilled = model_and_step("clm", teacher=teacher)
            out["distilled_vs_clm_step"] = compare({"clm": clm, "distilled": distilled})
        out["max_memory_allocated_bytes"] = int(torch.cuda.max_memory_allocated())
    print(json.dumps(out))


if __name__ == "__main__":
    main()
