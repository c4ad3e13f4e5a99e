"""The next-token sampling rule in plain torch, in float64, on any device: what obte_sample_logits_bf16 (include/omnibiote_hip_sample.h)
and ``model.sample_next`` implement, written once to be read and to be tested against.  Not on any hot path.

For one row x[0..V) of logits, a temperature T > 0, an optional top_k >= 1, an optional top_p in (0, 1] and a uniform number u:

  kept set  every entry whose value is at least a threshold value, so a tie at the threshold is kept whole.  NaN and -inf are never
            kept.  top-k: the threshold is the k-th largest value (k >= V or no top_k: no cut).  top-p, applied to what top-k kept
            with weights exp((x - max) / T): walking the distinct values downwards and adding each value's whole mass, the threshold
            is the first value at which the running mass reaches top_p times the total (top_p = 1: no cut).  The largest value is always kept.
  draw      over the kept entries in index order the token is the first index whose cumulative probability exceeds u; u >= 1 gives
            the last kept entry of non-zero weight, u < 0 or NaN the first.
  greedy    top_k == 1, T == 0 or no u: the lowest index of the row maximum.
  nothing   a row with no finite entry (and no +inf) gives token 0 and a kept count of 0; a row holding +inf gives a +inf entry.
"""
from __future__ import annotations

import torch


def _per_row(v, b, device, dtype):
    """v (None, a number or a (B,) tensor) as a (B,) tensor"""
    if v is None:
        return None
    t = torch.as_tensor(v, dtype=dtype, device=device)
    return t.expand(b).clone() if t.dim() == 0 else t.reshape(b)


def sample_reference(logits, u, temperature=1.0, top_k=None, top_p=None, n_kept=None):
    """(token, kept count, cumulative distribution) of every row of ``logits`` — (B, V), or (V,) for one row — under the rule above.
    ``u``: None (greedy), a number or (B,).  ``n_kept`` (a number or (B,)): the kept set is built from that count — the n largest
    entries, the tie at the n-th kept whole — instead of being derived from top_k / top_p.  token and count are int64 (B,), the
    distribution float64 (B, V): cdf[t] = the probability of a token <= t (for a greedy row the step at its token; zeros for a row with
    nothing to sample).  One row in, scalars and (V,) out."""
    one = logits.dim() == 1
    x = (logits.unsqueeze(0) if one else logits).double()
    if x.dim() != 2:
        raise ValueError(f"sample_reference: logits must be (B, V) or (V,), got {tuple(logits.shape)}")
    if temperature < 0:
        raise ValueError(f"sample_reference: temperature must not be negative, got {temperature}")
    if top_k is not None and top_k < 1:
        raise ValueError(f"sample_reference: top_k must be at least 1, got {top_k}")
    if top_p is not None and not 0 < top_p <= 1:
        raise ValueError(f"sample_reference: top_p must lie in (0, 1], got {top_p}")
    b, v = x.shape
    dev = x.device
    neg = torch.full((), float("-inf"), dtype=torch.float64, device=dev)
    valid = ~torch.isnan(x) & (x > neg)
    xs = torch.where(valid, x, neg)
    nv = valid.sum(dim=1)
    m = xs.max(dim=1, keepdim=True).values
    col = torch.arange(v, device=dev).unsqueeze(0)
    first_max = torch.where(valid & (xs == m), col, v).min(dim=1).values                 # (v for a row with nothing)
    greedy = u is None or temperature == 0 or (top_k == 1 and n_kept is None)
    if greedy:
        token = torch.where(nv > 0, first_max, torch.zeros_like(first_max))
        cdf = ((col >= token.unsqueeze(1)) & (nv > 0).unsqueeze(1)).double()
        out = token, (nv > 0).long(), cdf
        return tuple(t[0] for t in out) if one else out
    # weights: the maximum's own is 1 exactly (a +inf row: inf - inf is never formed)
    w = torch.where(valid, torch.where(xs == m, torch.ones_like(xs), torch.exp((xs - m) / temperature)), torch.zeros_like(xs))
    sv, order = torch.sort(xs, dim=1, descending=True, stable=True)
    rank = col.expand(b, v)
    if n_kept is not None:
        n = _per_row(n_kept, b, dev, torch.int64).clamp(max=v)
        thr = sv.gather(1, (n - 1).clamp(min=0).unsqueeze(1))
        kept = valid & (xs >= thr) & (n > 0).unsqueeze(1)
    else:
        kept = valid
        if top_k is not None and top_k < v:
            kk = nv.clamp(max=top_k)
            thr = sv.gather(1, (kk - 1).clamp(min=0).unsqueeze(1))
            kept = kept & (xs >= thr)
        if top_p is not None and top_p < 1:
            ws = torch.where(kept, w, torch.zeros_like(w)).gather(1, order)             # masses in descending order of value
            csum = ws.cumsum(dim=1)
            n_in = kept.sum(dim=1, keepdim=True)
            end = torch.ones_like(kept)
            end[:, :-1] = sv[:, :-1] != sv[:, 1:]                                        # the last entry of every run of one value
            reach = end & (rank < n_in) & (csum >= top_p * csum[:, -1:])
            at = reach.to(torch.uint8).argmax(dim=1, keepdim=True)                       # the first such run
            kept = kept & (xs >= sv.gather(1, at))
    wk = torch.where(kept, w, torch.zeros_like(w))
    csum = wk.cumsum(dim=1)
    total = csum[:, -1:]
    cdf = torch.where(total > 0, csum / torch.where(total > 0, total, torch.ones_like(total)), torch.zeros_like(csum))
    uu = _per_row(u, b, dev, torch.float64).unsqueeze(1)
    uu = torch.where(uu > 0, uu, torch.zeros_like(uu))                                   # u < 0 or NaN: the first
    over = (cdf > uu) & (wk > 0)
    first = torch.where(over, col, v).min(dim=1).values
    last = torch.where(wk > 0, col, -1).max(dim=1).values                                # u >= 1: the last of non-zero weight
    token = torch.where((first < v) & (uu.squeeze(1) < 1), first, last).clamp(min=0)
    count = kept.sum(dim=1)
    token = torch.where(count > 0, token, torch.zeros_like(token))
    out = token, count, cdf
    return tuple(t[0] for t in out) if one else out
