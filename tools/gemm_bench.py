"""Micro-benchmark of the GEMM entry point on the hot-path shapes (random bf16 data).  Usage:
    python tools/gemm_bench.py [--reps 20] [--shapes small|all] [--only NAME] [--structure S [--bn BN] [--splits N]]
Prints TFLOP/s per shape (median of reps, HIP events on the launch stream).  --structure installs the plan (S, BN, N splits) for
every shape through obte_gemm_plan_set (BN: the structure's width, 256 for structure 2 unless given; N: 1 unless given, and 1 for
the products whose epilogue has no split-K form)."""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from omnibiote_amd import _lib as L, ops  # noqa: E402

M = int(os.environ.get("OBTE_BENCH_M", "8192"))   # rows per launch (8192 = one micro-batch of 8 x 1024 tokens)
C, V = 1024, 65536
SHAPES = {
    # name: (kind, M, N, K)
    "fwd_qkv": ("nt", M, 3 * C, C), "fwd_proj": ("nt_add", M, C, C), "fwd_fc": ("nt_gelu", M, 4 * C, C),
    "fwd_fc_act": ("nt_geluact", M, 4 * C, C),   # c_fc of a forward without a backward: the activation alone
    "fwd_mlp": ("nt_add", M, C, 4 * C), "fwd_lm": ("nt", M, V, C),
    "dg_mlp": ("nn_gelubwd", M, 4 * C, C), "dg_fc": ("nn", M, C, 4 * C), "dg_proj": ("nn", M, C, C),
    "dg_qkv": ("nn", M, C, 3 * C), "dg_lm": ("nn", M, C, V),
    "wg_mlp": ("tn", C, 4 * C, M), "wg_fc": ("tn", 4 * C, C, M), "wg_proj": ("tn", C, C, M), "wg_qkv": ("tn", 3 * C, C, M),
    "wg_lm": ("tn", V, C, M),
}


def run(name, reps, structure=0, bn=0, splits=1):
    kind, m, n, k = SHAPES[name]
    dev = "cuda"
    g = torch.Generator(device=dev).manual_seed(0)
    a = torch.randn(m * k, device=dev, generator=g).to(torch.bfloat16)
    b = torch.randn(n * k, device=dev, generator=g).to(torch.bfloat16)
    aux = torch.randn(m * n, device=dev, generator=g).to(torch.bfloat16) if ("add" in kind or "gelubwd" in kind) else None
    ak, bk = kind.startswith("nt") or kind.startswith("nn"), kind.startswith("nt")
    epi = {"nt": L.EPI_NONE, "nn": L.EPI_NONE, "tn": L.EPI_NONE, "nt_add": L.EPI_ADD, "nt_gelu": L.EPI_GELU, "nt_geluact": L.EPI_GELU_ACT, "nn_gelubwd": L.EPI_GELU_BWD}[kind]
    out = torch.empty(m * n, device=dev, dtype=torch.bfloat16)
    if structure:
        s = splits if epi in (L.EPI_NONE, L.EPI_ADD) else 1
        L.check(L.lib().obte_gemm_plan_set(int(ak), int(bk), epi, m, n, k, structure, bn, s), "obte_gemm_plan_set")
    for _ in range(3):
        ops.gemm(a, b, m, n, k, ak, bk, epi, aux, out=out)
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        ops.gemm(a, b, m, n, k, ak, bk, epi, aux, out=out)
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    ts.sort()
    med = ts[len(ts) // 2]
    print(f"{name:9s} {kind:11s} M={m:6d} N={n:6d} K={k:6d}  {med * 1e3:9.1f} us  {2.0 * m * n * k / (med * 1e-3) / 1e12:7.1f} TFLOP/s", flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--only", default="")
    ap.add_argument("--structure", type=int, default=0, help="force this GEMM structure (1, 2, 3, 4, 7) through the plan table")
    ap.add_argument("--bn", type=int, default=0, help="its tile width (default: the structure's own; 256 for structure 2)")
    ap.add_argument("--splits", type=int, default=1, help="its split-K count (epilogue NONE / ADD products only; the others run unsplit)")
    args = ap.parse_args()
    bn = args.bn or {1: 128, 4: 128}.get(args.structure, 256)
    for name in SHAPES:
        if args.only and name not in args.only.split(","):
            continue
        run(name, args.reps, args.structure, bn, args.splits)
