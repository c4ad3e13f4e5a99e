"""Speculative decoding on the small config (8 layers, 1024 wide, 8 heads of 128; bf16; vocabulary 65 536): what verifying a block of
drafted tokens costs, and what a draft-and-verify round costs against plain decoding.  Contenders alternate in one process over --rounds
rounds after warm-up; device events around windows of calls; median and [min - max] over the rounds.

  (a) obte_spec_verify_bf16 alone (ops.spec_verify on preallocated logits) at V = 65 536, B in {1, 8, 64}, k in {2, 4, 8}, temperature
      0.9 and top_k = 50, against the same rule in ordinary torch (fp32: a softmax, a top-k threshold, the ratio, a cumsum over the
      residual) on the same logits.
  (b) one round — k + 1 draft decode_steps with k draws, the target's extend over k + 1 tokens, the verification: OmniBioTA.draft_and_verify
      — against k + 1 decode_steps of the target, at --model-batches x --context; the draft has the target's width and 2 layers.
  (c) what that round yields: tokens per round at the acceptance rate the run happened to have, and the break-even — the tokens per
      round at which a round costs what plain decoding costs for them.  The weights are random: the acceptance rate says nothing
      about a trained pair; the round's cost and the break-even do not depend on it.
One JSON line per measurement.

    python tools/spec_bench.py [--parts a,b] [--batches 1,8,64] [--model-batches 1,8] [--ks 2,4,8] [--context 2048] [--rounds 5] [--steps 100]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from decode_bench import build, summary   # noqa: E402
from extend_bench import alternate        # noqa: E402

T, TOP_K = 0.9, 50


def torch_verify(p, q, x, ua, ud):
    """the rule of sampling.verify_reference in fp32 torch, top-k and temperature only: (n_accept, token)"""
    def dist(z):
        z = z.float() / T
        kth = torch.topk(z, TOP_K, dim=-1).values[..., -1:]
        return torch.softmax(z.masked_fill(z < kth, float("-inf")), dim=-1)
    B, k = x.shape
    P, Q = dist(p), dist(q)
    px, qx = P[:, :k].gather(2, x.unsqueeze(2)).squeeze(2), Q.gather(2, x.unsqueeze(2)).squeeze(2)
    ok = (px > 0) & ((qx == 0) | (ua * qx < px))
    a = ok.long().cumprod(dim=1).sum(dim=1)
    rows = torch.arange(B, device=p.device)
    pa = P[rows, a]
    res = torch.where((a < k).unsqueeze(1), (pa - Q[rows, a.clamp(max=k - 1)]).clamp(min=0), torch.zeros_like(pa))
    w = torch.where(res.sum(dim=1, keepdim=True) > 0, res, pa)
    cdf = w.cumsum(dim=1)
    tok = torch.searchsorted(cdf, (ud * cdf[:, -1]).unsqueeze(1), right=True).squeeze(1).clamp(max=p.shape[2] - 1)
    return a, tok


def verify_alone(B, k, V, rounds, steps, dev):
    from omnibiote_amd import ops
    g = torch.Generator(device=dev).manual_seed(B * 100 + k)
    p = (torch.randn(B, k + 1, V, device=dev, generator=g) * 2).to(torch.bfloat16)
    q = (p[:, :k].float() + torch.randn(B, k, V, device=dev, generator=g)).to(torch.bfloat16)
    x = torch.stack([ops.sample_logits(q[:, j], torch.rand(B, device=dev, generator=g), T, TOP_K) for j in range(k)], dim=1)
    ua, ud = torch.rand(B, k, device=dev, generator=g), torch.rand(B, device=dev, generator=g)
    legs = {"spec_verify": lambda: ops.spec_verify(p, q, x, ua, ud, T, TOP_K), "torch": lambda: torch_verify(p, q, x, ua, ud)}
    us = alternate(legs, rounds, {"spec_verify": steps, "torch": max(3, steps // 10)})
    med = {n: statistics.median(v) for n, v in us.items()}
    a_hip, a_torch = ops.spec_verify(p, q, x, ua, ud, T, TOP_K)[0], torch_verify(p, q, x, ua, ud)[0]
    print(json.dumps({"part": "a", "B": B, "k": k, "V": V, "logits_bytes": (2 * k + 1) * B * V * 2, "windows": {"calls": steps, "rounds": rounds},
                      "us": {n: summary(v) for n, v in us.items()}, "torch_over_spec_verify": round(med["torch"] / med["spec_verify"], 1),
                      "mean_accepted": round(float(a_hip.float().mean()), 2), "rows_where_torch_accepts_another_count": int((a_hip.long() != a_torch).sum())}),
          flush=True)


def one_round(m, d, B, ctx, k, rounds, steps, dev):
    from omnibiote_amd.model import KVCache
    g = torch.Generator(device=dev).manual_seed(B * 10007 + ctx)
    idx = torch.randint(4, m.config.vocab_size, (B, ctx), device=dev, generator=g)
    pos = ctx - k - 1
    cache, dcache = KVCache(m, B, ctx), KVCache(d, B, ctx)
    m.prefill(idx[:, :pos], cache, lengths=[pos] * B, chunk=512)
    d.prefill(idx[:, :pos], dcache, lengths=[pos] * B, chunk=512)
    pending = idx[:, pos].contiguous()
    cols = [idx[:, pos + j].contiguous() for j in range(k + 1)]
    accepted = []

    def back(*caches):                  # the same positions every time: the context stays ctx long
        for c in caches:
            c.rewind_rows([k + 1] * B, now=[pos + k + 1] * B)

    def spec_round():
        r = torch.rand(B * (2 * k + 1), device=dev, generator=g)
        us = r[:k * B].view(k, B), r[k * B:2 * k * B].view(B, k), r[2 * k * B:]
        accepted.append(m.draft_and_verify(d, pending, cache, dcache, k, us, T, TOP_K)[1])
        back(cache, dcache)

    def steps_k1():
        for j in range(k + 1):
            m.decode_step(cols[j], cache)
        back(cache)
    w = max(3, steps // (k + 1))
    us = alternate({"round": spec_round, "k+1_decode_steps": steps_k1}, rounds, {"round": w, "k+1_decode_steps": w})
    med = {n: statistics.median(v) for n, v in us.items()}
    step = med["k+1_decode_steps"] / (k + 1)
    mean_a = float(torch.stack(accepted).float().mean())
    print(json.dumps({"part": "b", "B": B, "context": ctx, "k": k, "draft_layers": len(d.transformer.h), "windows": {"calls": w, "rounds": rounds},
                      "us_per_call": {n: summary(v, 1) for n, v in us.items()}, "us_per_decode_step": round(step, 1),
                      "part_c": {"mean_accepted_random_weights": round(mean_a, 3), "tokens_per_round": round(mean_a + 1, 3),
                                 "us_per_token_this_run": round(med["round"] / (mean_a + 1), 1),
                                 "break_even_tokens_per_round": round(med["round"] / step, 2),
                                 "break_even_accepted_of_k": round(med["round"] / step - 1, 2)}}), flush=True)
    del cache, dcache
    torch.cuda.empty_cache()


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--parts", default="a,b", help="(c) is reported with (b)")
    p.add_argument("--batches", default="1,8,64", help="(a)")
    p.add_argument("--model-batches", default="1,8", help="(b)")
    p.add_argument("--ks", default="2,4,8")
    p.add_argument("--context", type=int, default=2048)
    p.add_argument("--rounds", type=int, default=5)
    p.add_argument("--steps", type=int, default=100, help="calls per timed window")
    a = p.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    parts, ks = a.parts.split(","), [int(k) for k in a.ks.split(",")]
    if "a" in parts:
        for B in [int(b) for b in a.batches.split(",")]:
            for k in ks:
                verify_alone(B, k, 2 ** 16, a.rounds, a.steps, dev)
    if "b" in parts:
        m, d = build(a.context, dev), build(a.context, dev, n_layer=2)
        for B in [int(b) for b in a.model_batches.split(",")]:
            for k in ks:
                one_round(m, d, B, a.context, k, a.rounds, a.steps, dev)


if __name__ == "__main__":
    main()
