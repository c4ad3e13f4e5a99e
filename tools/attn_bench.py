"""Attention micro-benchmark on the hot-path shape (B=8, H=8, T=1024, hs=128, single-document key ranges).
    python tools/attn_bench.py [--reps 10] [--T 1024] [--hs 128]
    python tools/attn_bench.py --causal [--rounds 5]     the same shape unmasked and under the causal range mask, alternating in
                                                         one process: median and spread over the rounds, forward and backward"""
import argparse, os, sys
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from omnibiote_amd import ops, masks

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--B", type=int, default=8); ap.add_argument("--H", type=int, default=8)
ap.add_argument("--T", type=int, default=1024); ap.add_argument("--hs", type=int, default=128)
ap.add_argument("--dense", action="store_true", help="pass the mask as the reference's dense additive (B,H,T,T) expand() view")
ap.add_argument("--nomask", action="store_true", help="no mask at all (rows without EOS attend everywhere)")
ap.add_argument("--two_kernel", action="store_true", help="backward as the dQ + dK/dV kernel pair (default: the one-kernel form where it applies)")
ap.add_argument("--multi", action="store_true", help="multi-document rows (block-diagonal mask) instead of one document per row")
ap.add_argument("--causal", action="store_true", help="compare no mask against the causal range mask (masks.RangeMask.causal), alternating, forward and backward")
ap.add_argument("--rounds", type=int, default=5, help="--causal: rounds of (unmasked, causal) measurements; each is a median over --reps launches")
a = ap.parse_args()
B, H, T, hs = a.B, a.H, a.T, a.hs
dev = "cuda"
g = torch.Generator(device=dev).manual_seed(0)
qkv = torch.randn(B, T, 3 * H * hs, device=dev, generator=g).to(torch.bfloat16)
d_o = torch.randn(B, T, H * hs, device=dev, generator=g).to(torch.bfloat16)
tok = torch.randint(20, 100, (B, T), device=dev)
if a.multi:
    for b in range(B):
        tok[b, torch.randint(8, T - 8, (3,))] = 3
rm = masks.RangeMask.from_tokens(tok)
spec = ops.MaskSpec(ranges=rm.key_ranges)
if a.nomask:
    spec = None
if a.dense:
    spec = ops.MaskSpec.from_user(rm.dense(torch.bfloat16).unsqueeze(1).expand(-1, H, -1, -1), B, T, H, dev)
scale = 8.0 / (H * hs)
def timeit(fn):
    for _ in range(2): fn()
    torch.cuda.synchronize(); ts = []
    for _ in range(a.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record(); e1.synchronize(); ts.append(e0.elapsed_time(e1))
    ts.sort(); return ts[len(ts) // 2] * 1e3
if a.causal:
    # Executed work under the causal mask: a 256-query forward workgroup runs the 64-key tiles up to its last query, a 256-key
    # backward workgroup the 32-query slices from its first key on — about (T + 256) / (2 T) of the unmasked tile count either
    # way.  The figures printed are times; the ratio causal / unmasked is shown beside that share.
    cspec = ops.MaskSpec.from_user(masks.RangeMask.causal(B, T, dev), B, T, H, dev)
    variants = {"unmasked": None, "causal": cspec}
    state = {k: ops.attn_fwd(qkv, B, T, H, hs, scale, v) for k, v in variants.items()}
    res = {(k, d): [] for k in variants for d in ("fwd", "bwd")}
    for _ in range(a.rounds):
        for k, v in variants.items():   # alternating: both variants see the same machine state
            o, lse = state[k]
            res[k, "fwd"].append(timeit(lambda: ops.attn_fwd(qkv, B, T, H, hs, scale, v)))
            res[k, "bwd"].append(timeit(lambda: ops.attn_bwd(qkv, o, d_o, lse, B, T, H, hs, scale, v, one_kernel=not a.two_kernel)))
    nq, nk = (T + 255) // 256, (T + 63) // 64
    share = sum(min(nk, (min(T, 256 * (i + 1)) + 63) // 64) for i in range(nq)) / (nq * nk)
    print(f"attn B={B} H={H} T={T} hs={hs}, {a.rounds} rounds x median of {a.reps}; backward: {'kernel pair' if a.two_kernel else 'one-kernel form where it applies'}", flush=True)
    med = {}
    for key, ts in res.items():
        ts = sorted(ts); med[key] = ts[len(ts) // 2]
        print(f"  {key[0]:9s} {key[1]}  median {med[key]:8.1f} us   min {ts[0]:8.1f}   max {ts[-1]:8.1f}", flush=True)
    print(f"  causal / unmasked: fwd {med['causal', 'fwd'] / med['unmasked', 'fwd']:.3f}  bwd {med['causal', 'bwd'] / med['unmasked', 'bwd']:.3f}"
          f"   (share of the forward's key tiles executed: {share:.3f})", flush=True)
    sys.exit(0)
o, lse = ops.attn_fwd(qkv, B, T, H, hs, scale, spec)
tf = timeit(lambda: ops.attn_fwd(qkv, B, T, H, hs, scale, spec))
tb = timeit(lambda: ops.attn_bwd(qkv, o, d_o, lse, B, T, H, hs, scale, spec, one_kernel=not a.two_kernel))
fl = 4.0 * B * H * T * T * hs
print(f"attn fwd {tf:8.1f} us {fl / tf / 1e6:7.1f} TFLOP/s | bwd {tb:8.1f} us {2.5 * fl / tb / 1e6:7.1f} TFLOP/s (algorithmic)", flush=True)
