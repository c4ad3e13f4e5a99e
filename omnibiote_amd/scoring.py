"""The scoring rule in plain torch, in float64, on any device: what obte_readout_score_bf16 (include/omnibiote_hip_score.h) and
``ops.readout_score`` implement, written once to be read and to be tested against.  Not on any hot path: it forms the (R, V) logits.

For x (R, C), the readout weight w (V, C), targets (R, K) or (R,) and the readout's alpha:

  z[r, v]          alpha * sum_c x[r, c] w[v, c] — exactly, in float64.  The kernel rounds this once to bf16 (the readout's own rule);
                   the reference deliberately does not, and ``zbound`` says how far the kernel's z may lie from it.
  lse[r]           log sum_v exp(z[r, v])
  logits_at[r, k]  z[r, targets[r, k]]
  logprobs[r, k]   logits_at[r, k] - lse[r]
  a target of -1   "no candidate": 0 in both; any other value outside [0, V): NaN in both.
  zbound[r, v]     2^-8 |z| + C 2^-24 alpha sum_c |x[r, c] w[v, c]|: half a bf16 spacing (8 significant bits: the spacing at |z| is
                   at most 2^-7 |z|), plus the worst case of a length-C fp32 sum (each of C additions errs by at most 2^-24 of the
                   running sum of magnitudes).
"""
from __future__ import annotations

import torch


def score_reference(x, w, targets, alpha=1.0):
    """(logprobs, lse, logits_at, zbound) of the rule above, all float64: logprobs and logits_at shaped like ``targets``, lse (R,),
    zbound (R, V)."""
    if x.dim() != 2 or w.dim() != 2 or x.shape[1] != w.shape[1]:
        raise ValueError(f"score_reference: x (R, C) and w (V, C), got {tuple(x.shape)} and {tuple(w.shape)}")
    r, c = x.shape
    v = w.shape[0]
    if targets.dim() not in (1, 2) or targets.shape[0] != r or targets.dtype not in (torch.int64, torch.int32):
        raise ValueError(f"score_reference: targets must be integer ({r},) or ({r}, K), got {targets.dtype} {tuple(targets.shape)}")
    xd, wd = x.double(), w.double()
    z = float(alpha) * (xd @ wd.t())
    zbound = 2.0 ** -8 * z.abs() + c * 2.0 ** -24 * abs(float(alpha)) * (xd.abs() @ wd.abs().t())
    lse = torch.logsumexp(z, dim=1)
    t = targets.long().reshape(r, -1)
    inside = (t >= 0) & (t < v)
    at = z.gather(1, t.clamp(0, v - 1))
    nan = torch.full_like(at, float("nan"))
    zero = torch.zeros_like(at)
    logits_at = torch.where(inside, at, torch.where(t == -1, zero, nan))
    logprobs = torch.where(inside, at - lse.unsqueeze(1), torch.where(t == -1, zero, nan))
    return logprobs.reshape(targets.shape), lse, logits_at.reshape(targets.shape), zbound
