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
    token, cdf = _draw(wk, u)
    count = kept.sum(dim=1)
    token = torch.where(count > 0, token, torch.zeros_like(token))
    out = token, count, cdf
    return tuple(t[0] for t in out) if one else out


def _draw(wk, u):
    """(token, cumulative distribution) of every row of the weights ``wk`` (B, V) float64, not normalised, zero outside the kept set: the
    first index whose cumulative probability exceeds u; u >= 1: the last entry of non-zero weight; u < 0 or NaN: the first.  A row of
    zeros gives token 0 and a distribution of zeros."""
    b, v = wk.shape
    col = torch.arange(v, device=wk.device).unsqueeze(0)
    csum = wk.cumsum(dim=1)
    total = csum[:, -1:]
    cdf = torch.where(total > 0, csum / torch.where(total > 0, total, torch.ones_like(total)), torch.zeros_like(csum))
    uu = _per_row(u, b, wk.device, torch.float64).unsqueeze(1)
    uu = torch.where(uu > 0, uu, torch.zeros_like(uu))                                   # u < 0 or NaN: the first
    over = (cdf > uu) & (wk > 0)
    first = torch.where(over, col, v).min(dim=1).values
    last = torch.where(wk > 0, col, -1).max(dim=1).values                                # u >= 1: the last of non-zero weight
    return torch.where((first < v) & (uu.squeeze(1) < 1), first, last).clamp(min=0), cdf


def verify_distributions(p, q, temperature=1.0, top_k=None, top_p=None, n_kept_p=None, n_kept_q=None):
    """(P (B, k + 1, V), Q (B, k, V)) float64: the distribution ``sample_reference`` draws from on every row of the target's logits ``p``
    (B, k + 1, V) and of the draft's ``q`` (B, k, V) — its kept set, ties kept whole, and its normalised weights (zeros for a row with
    nothing to sample).  ``n_kept_p`` (B, k + 1) / ``n_kept_q`` (B, k): the kept sets rebuilt from those counts, as ``sample_reference``
    does with ``n_kept``."""
    def dist(x, n):
        b, r, v = x.shape
        cdf = sample_reference(x.reshape(b * r, v), 0.5, temperature, top_k, top_p, None if n is None else torch.as_tensor(n).reshape(b * r))[2]
        return torch.diff(cdf, dim=1, prepend=torch.zeros(b * r, 1, dtype=torch.float64, device=cdf.device)).view(b, r, v)
    return dist(p, n_kept_p), dist(q, n_kept_q)


def verify_reference(p, q, draft, u_accept=None, u_draw=None, temperature=1.0, top_k=None, top_p=None, n_kept_p=None, n_kept_q=None):
    """Speculative decoding's accept / reject rule in plain torch, in float64, on any device: what obte_spec_verify_bf16
    (include/omnibiote_hip_spec.h) implements.  ``p`` (B, k + 1, V): the target's logits behind the pending token and behind each drafted
    token; ``q`` (B, k, V): the logits the draft drew from; ``draft`` (B, k) integers; ``u_accept`` (B, k) and ``u_draw`` (B,) uniforms.  One
    batch row — (k + 1, V), (k, V), (k,), (k,) and a number — gives scalars and (V,).

    With P_j and Q_j what ``sample_reference`` makes of p[j] and q[j] under the same temperature, top_k and top_p:
      accept   walking j = 0, 1, ...: x_j stands while u_accept[j] < P_j(x_j) / Q_j(x_j).  P_j(x_j) == 0 — outside the target's kept set, or
               outside [0, V) — never stands; otherwise Q_j(x_j) == 0 stands; a u_accept that is NaN or negative counts as 0.
      token    a = the number that stand.  a == k: the draw of ``sample_reference(p[k], u_draw, ...)``.  a < k: the first index whose
               cumulative probability exceeds u_draw under max(0, P_a - Q_a) / Z, Z its sum — from P_a if Z == 0; u_draw's edge cases as
               in ``sample_reference``.
      greedy   temperature == 0, top_k == 1 or no uniforms: x_j stands while it is the lowest index of p[j]'s maximum; the token is that
               index of p[a].  q is not read and may be None.
    Returns (a int64 (B,), token int64 (B,), the cumulative distribution float64 (B, V) the token was drawn from)."""
    one = p.dim() == 2
    if one:
        p, draft = p.unsqueeze(0), torch.as_tensor(draft).unsqueeze(0)
        q = None if q is None else q.unsqueeze(0)
        u_accept = None if u_accept is None else torch.as_tensor(u_accept).unsqueeze(0)
    if p.dim() != 3 or p.shape[1] < 2:
        raise ValueError(f"verify_reference: p must be (B, k + 1, V) or (k + 1, V) with k >= 1, got {tuple(p.shape)}")
    b, k, v = p.shape[0], p.shape[1] - 1, p.shape[2]
    dev = p.device
    x = torch.as_tensor(draft, device=dev).to(torch.int64)
    if x.shape != (b, k):
        raise ValueError(f"verify_reference: draft must be ({b}, {k}), got {tuple(x.shape)}")
    inside = (x >= 0) & (x < v)
    xc = x.clamp(0, v - 1).unsqueeze(2)
    rows = torch.arange(b, device=dev)
    greedy = u_accept is None or u_draw is None or temperature == 0 or top_k == 1
    if greedy:
        top = sample_reference(p.reshape(b * (k + 1), v), None)[0].view(b, k + 1)
        ok = inside & (x == top[:, :k])
        a = ok.long().cumprod(dim=1).sum(dim=1)
        token = top[rows, a]
        out = a, token, (torch.arange(v, device=dev).unsqueeze(0) >= token.unsqueeze(1)).double()
        return tuple(t[0] for t in out) if one else out
    if q is None or q.shape != (b, k, v):
        raise ValueError(f"verify_reference: q must be ({b}, {k}, {v}) unless the call is greedy")
    P, Q = verify_distributions(p, q, temperature, top_k, top_p, n_kept_p, n_kept_q)
    px = torch.where(inside, P[:, :k].gather(2, xc).squeeze(2), torch.zeros((), dtype=torch.float64, device=dev))
    qx = torch.where(inside, Q.gather(2, xc).squeeze(2), torch.zeros((), dtype=torch.float64, device=dev))
    ua = torch.as_tensor(u_accept, dtype=torch.float64, device=dev).reshape(b, k)
    ua = torch.where(ua > 0, ua, torch.zeros_like(ua))                                   # NaN or negative: 0
    ok = (px > 0) & ((qx == 0) | (ua < px / torch.where(qx > 0, qx, torch.ones_like(qx))))
    a = ok.long().cumprod(dim=1).sum(dim=1)
    pa = P[rows, a]
    res = (pa - Q[rows, a.clamp(max=k - 1)]).clamp(min=0)
    res = torch.where((a < k).unsqueeze(1), res, torch.zeros_like(res))
    w = torch.where(res.sum(dim=1, keepdim=True) > 0, res, pa)                           # a == k or Z == 0: P_a itself
    token, cdf = _draw(w, u_draw)
    token = torch.where(w.sum(dim=1) > 0, token, torch.zeros_like(token))
    bonus = sample_reference(p[:, k], u_draw, temperature, top_k, top_p, None if n_kept_p is None else torch.as_tensor(n_kept_p).reshape(b, k + 1)[:, k])
    token, cdf = torch.where(a == k, bonus[0], token), torch.where((a == k).unsqueeze(1), bonus[2], cdf)
    out = a, token, cdf
    return tuple(t[0] for t in out) if one else out


def verify_point_reference(p, draft, u_accept=None, u_draw=None, temperature=1.0, top_k=None, top_p=None):
    """``verify_reference`` for a draft that is a token and not a distribution (obte_spec_verify_point_bf16,
    include/omnibiote_hip_lookup.h): by definition ``verify_reference`` on the q whose row (b, j) is 0 at draft[b, j] and -inf everywhere
    else — all -inf for a drafted token outside [0, V).  x_j stands while u_accept[j] < P_j(x_j); behind a rejection at a the token is
    drawn from P_a with x_a's weight removed; behind k acceptances it is the draw on p[k].  ``p`` (B, k + 1, V) or (k + 1, V), ``draft``
    (B, k) or (k,); returns what ``verify_reference`` returns."""
    x = torch.as_tensor(draft, device=p.device).to(torch.int64)
    v = p.shape[-1]
    q = torch.full(tuple(x.shape) + (v,), float("-inf"), dtype=p.dtype, device=p.device)
    inside = (x >= 0) & (x < v)
    q.scatter_(-1, x.clamp(0, v - 1).unsqueeze(-1), torch.where(inside, 0.0, float("-inf")).to(p.dtype).unsqueeze(-1))
    return verify_reference(p, q, x, u_accept, u_draw, temperature, top_k, top_p)


def lookup_reference(hist, lens, k, g_min, g_max, V):
    """The n-gram lookup draft in a plain loop (obte_lookup_draft, include/omnibiote_hip_lookup.h), written to be read: ``hist`` (B, W)
    integers, ``lens`` (B,) integers.  Row b is active iff 1 <= n = lens[b] <= W.  A token outside [0, V) equals nothing, not even itself.
    For a candidate end e in [1, n - 1], m(e) is the number of tokens before e — at most min(g_max, e) — that agree with the row's last
    tokens, walking backwards; e* has the largest m(e), among equals the largest e.  m(e*) >= g_min: match_len = m(e*) and
    draft[j] = hist[e* + (j mod (n - e*))], the history continued periodically past its end.  Otherwise match_len = 0 and every
    draft[j] = hist[n - 1].  An inactive row gives zeros.  Returns (draft int64 (B, k), match_len int32 (B,)) on the CPU."""
    rows = torch.as_tensor(hist).cpu().to(torch.int64).tolist()
    ns = torch.as_tensor(lens).cpu().to(torch.int64).tolist()
    draft, match = [], []
    for h, n in zip(rows, ns):
        if not 1 <= n <= len(h):
            draft.append([0] * k)
            match.append(0)
            continue

        def same(i, j):
            return 0 <= h[i] < V and h[i] == h[j]

        best_m, best_e = 0, n - 1
        for e in range(1, n):
            m = 0
            while m < min(g_max, e) and same(e - 1 - m, n - 1 - m):
                m += 1
            if m >= max(best_m, g_min):                                                  # (e rises: an equal m later on is more recent)
                best_m, best_e = m, e
        d = n - best_e
        draft.append([h[best_e + j % d] for j in range(k)])
        match.append(best_m)
    return torch.tensor(draft, dtype=torch.int64).view(len(rows), k), torch.tensor(match, dtype=torch.int32)


def pack_token_mask(mask):
    """bool (..., V) -> uint8 (..., ceil(V / 8)): column i is bit i & 7 of byte i >> 3, the padding bits of the last byte clear (the
    ``allowed`` argument of include/omnibiote_hip_constrain.h).  Plain torch on any device."""
    if mask.dtype != torch.bool or mask.dim() < 1 or mask.shape[-1] < 1:
        raise ValueError(f"pack_token_mask: mask must be bool (..., V) with V >= 1, got {mask.dtype} {tuple(mask.shape)}")
    v = mask.shape[-1]
    nb = (v + 7) // 8
    bits = torch.zeros(mask.shape[:-1] + (nb * 8,), dtype=torch.int32, device=mask.device)
    bits[..., :v] = mask
    weight = (1 << torch.arange(8, device=mask.device, dtype=torch.int32))
    return (bits.view(mask.shape[:-1] + (nb, 8)) * weight).sum(dim=-1).to(torch.uint8)


def unpack_token_mask(packed, v):
    """uint8 (..., n >= ceil(V / 8)) -> bool (..., V): the inverse of ``pack_token_mask``; bits of columns >= V are ignored."""
    if packed.dtype != torch.uint8 or packed.dim() < 1 or v < 1 or packed.shape[-1] * 8 < v:
        raise ValueError(f"unpack_token_mask: packed must be uint8 (..., >= ceil(V / 8)) with V = {v} >= 1, got {packed.dtype} {tuple(packed.shape)}")
    col = torch.arange(v, device=packed.device)
    return ((packed[..., col >> 3].to(torch.int32) >> (col & 7).to(torch.int32)) & 1).bool()


def constrain_reference(logits, allowed=None, hold_token=None, emitted=None, min_emitted=0, offset=0):
    """``logits`` (B, V) or (V,) with the excluded columns set to -inf: the restriction of include/omnibiote_hip_constrain.h in plain
    torch on any device.  ``allowed``: bool (V,) — one mask for every row — or (B, V); a False column is excluded.  ``hold_token`` (None,
    negative or >= V: nothing) is excluded too in every row b with ``emitted[b] + offset < min_emitted``; ``emitted``: None (0), a number
    or (B,) integers; ``offset``: the drafted position j of the row (0 in the sampler).  ``sample_reference`` / ``verify_reference`` on
    the result are what the constrained kernels implement."""
    one = logits.dim() == 1
    x = logits.unsqueeze(0) if one else logits
    if x.dim() != 2:
        raise ValueError(f"constrain_reference: logits must be (B, V) or (V,), got {tuple(logits.shape)}")
    if min_emitted < 0:
        raise ValueError(f"constrain_reference: min_emitted must not be negative, got {min_emitted}")
    b, v = x.shape
    out = torch.zeros((b, v), dtype=torch.bool, device=x.device)         # excluded
    if allowed is not None:
        a = torch.as_tensor(allowed, device=x.device)
        if a.dtype != torch.bool or a.shape not in ((v,), (b, v)):
            raise ValueError(f"constrain_reference: allowed must be bool ({v},) or ({b}, {v}), got {a.dtype} {tuple(a.shape)}")
        out = out | ~a.expand(b, v)
    if hold_token is not None and 0 <= int(hold_token) < v:
        e = torch.zeros(b, dtype=torch.int64, device=x.device) if emitted is None else _per_row(emitted, b, x.device, torch.int64)
        out[:, int(hold_token)] |= e + int(offset) < int(min_emitted)
    res = x.masked_fill(out, float("-inf"))
    return res[0] if one else res


def _history_counts(what, ids, n, b, v, device):
    """how often every column occurs among the first n[b] ids of row b — ``ids`` (B, W) integers or None, ``n`` None (W), a number or (B,),
    clamped to [0, W]; ids outside [0, V) are ignored — as (B, V) int64"""
    if ids is None:
        return torch.zeros((b, v), dtype=torch.int64, device=device)
    t = torch.as_tensor(ids, device=device)
    t = t.unsqueeze(0) if t.dim() == 1 and b == 1 else t
    if t.dim() != 2 or t.shape[0] != b or t.is_floating_point() or t.is_complex() or t.dtype == torch.bool:
        raise ValueError(f"penalize_reference: {what} must be ({b}, n) integers, got {t.dtype} {tuple(t.shape)}")
    t = t.to(torch.int64)
    w = t.shape[1]
    n = torch.full((b,), w, dtype=torch.int64, device=device) if n is None else _per_row(n, b, device, torch.int64).clamp(0, w)
    live = (torch.arange(w, device=device).unsqueeze(0) < n.unsqueeze(1)) & (t >= 0) & (t < v)
    cnt = torch.zeros((b, v + 1), dtype=torch.int64, device=device)
    cnt.scatter_add_(1, torch.where(live, t, torch.full_like(t, v)), live.to(torch.int64))
    return cnt[:, :v]


def penalty_numbers(repetition=1.0, presence=0.0, frequency=0.0):
    """The four fp32 numbers of include/omnibiote_hip_penalty.h as Python floats: ``(r, inv_r, pp, fp)``, each the fp32 rounding of the
    argument, ``inv_r = float32(1 / float64(r))``.  ValueError unless all are finite fp32 and r > 0."""
    import ctypes
    import math
    r, pp, fp = (ctypes.c_float(float(v)).value for v in (repetition, presence, frequency))
    if not (math.isfinite(r) and math.isfinite(pp) and math.isfinite(fp)) or not r > 0:
        raise ValueError(f"repetition must be positive and repetition, presence and frequency finite in fp32, got {repetition!r}, {presence!r}, "
                         f"{frequency!r}")
    inv = ctypes.c_float(1.0 / r).value
    if not math.isfinite(inv):
        raise ValueError(f"repetition {repetition!r} is too small: 1 / repetition overflows fp32")
    return r, inv, pp, fp


def penalize_reference(logits, prompt=None, prompt_len=None, gen=None, n_gen=None, repetition=1.0, presence=0.0, frequency=0.0):
    """A bf16 copy of ``logits`` (B, V) or (V,) with the columns of every row's history rewritten: the rule of
    include/omnibiote_hip_penalty.h in plain torch on any device, in fp32 operations each rounded on its own.  ``prompt`` (B, Tp) and
    ``gen`` (B, S) integers or None; row b's lists are their first ``prompt_len[b]`` / ``n_gen[b]`` ids (None: the whole width, else a number
    or (B,), clamped to the width); ids outside [0, V) are ignored.  For a column i in either list, x the fp32 value of its bf16 logit
    (``logits`` of another dtype are rounded to bf16 first) and c(i) its count in the generated list:

      1. repetition r != 1:  x = x * r if x < 0 else x * float32(1 / float64(r))
      2. c(i) > 0:           x = x - (presence + frequency * float32(c(i)))
      3. the column becomes x rounded to bf16 (nearest even); every other column keeps its bits.

    ``ops.sample_logits(logits, penalty=...)`` returns bit for bit what ``ops.sample_logits`` returns on this copy."""
    one = logits.dim() == 1
    x = (logits.unsqueeze(0) if one else logits).to(torch.bfloat16)
    if x.dim() != 2:
        raise ValueError(f"penalize_reference: logits must be (B, V) or (V,), got {tuple(logits.shape)}")
    r, inv, pp, fp = penalty_numbers(repetition, presence, frequency)
    b, v = x.shape
    dev = x.device
    c = _history_counts("gen", gen, n_gen, b, v, dev)
    ctx = (_history_counts("prompt", prompt, prompt_len, b, v, dev) > 0) | (c > 0)
    f32 = lambda value: torch.tensor(value, dtype=torch.float32, device=dev)
    y = x.float()
    if r != 1.0:
        y = torch.where(y < 0, y * f32(r), y * f32(inv))
    prod = f32(fp) * c.to(torch.float32)                                  # the product, then the sum, then the difference
    total = f32(pp) + prod
    y = torch.where(c > 0, y - total, y)
    res = torch.where(ctx, y.to(torch.bfloat16), x)
    return res[0] if one else res


def advance_reference(sampled, pos, count, out, n_new, token, wte, us=None, eos=None, commit=1):
    """The generation loop's per-row bookkeeping in plain torch on any device: what obte_gen_advance (include/omnibiote_hip_loop.h)
    implements.  Nothing is changed in place; returns the new ``(pos, count, out, n_new, token, x, u)``.  ``sampled`` (B,) int64 are the
    tokens drawn from the step's logits, ``pos`` (B,) int32 every row's next cache position (negative: parked), ``count`` (B,) int32 the
    steps the row has seen, ``out`` (B, S) int64 and ``n_new`` (B,) int32 what it has emitted, ``token`` (B,) int64 its last emitted token,
    ``wte`` (vocab, C), ``us`` (steps, B) the uniforms of a whole call or None.  For row b:

      running   pos[b] >= 0.  With ``commit`` (0 or 1) a running row moves on: p = pos[b] + commit — the step that just ran stored at pos[b].
      record    a running row with 0 <= s = count[b] < S:  out[b, s] = sampled[b], n_new[b] += 1, token[b] = sampled[b], and if that is
                ``eos`` (None or negative: no such token) the row is parked, p = -1.  Otherwise out, n_new and token stay as they are.
      always    pos[b] = p, count[b] = s + 1, x[b] = wte[clamp(token[b], 0, vocab - 1)] from the token this call leaves, and with ``us``
                u[b] = us[clamp(s + 1, 0, steps - 1), b], the next step's uniforms (u is None without ``us``).
    int32 arithmetic wraps as the kernel's does."""
    if commit not in (0, 1):
        raise ValueError(f"advance_reference: commit must be 0 or 1, got {commit!r}")
    b, width = out.shape
    rows = torch.arange(b, device=out.device)
    running = pos >= 0
    p = torch.where(running, pos + commit, pos) if commit else pos.clone()
    record = running & (count >= 0) & (count.long() < width)
    col = count.long().clamp(0, width - 1)
    new_out = out.clone()
    new_out[rows, col] = torch.where(record, sampled, out[rows, col])
    new_n = n_new + record.to(n_new.dtype)
    new_token = torch.where(record, sampled, token)
    if eos is not None and eos >= 0:
        p = torch.where(record & (sampled == eos), torch.full_like(p, -1), p)
    x = wte[new_token.clamp(0, wte.shape[0] - 1)]
    u = None if us is None else us[(count.long() + 1).clamp(0, us.shape[0] - 1), rows]
    return p, count + 1, new_out, new_n, new_token, x, u


# ---------------------------------------------------------------------------------------------------------------- encoder infilling
# The rules of include/omnibiote_hip_fill.h in plain torch, in float64: the counter-based Gumbel noise, the draw fused into the readout
# (obte_readout_sample_bf16), the unmasking schedule and the loop's bookkeeping (obte_fill_commit).
SITE_FILL = 8            # OBTE_SITE_FILL
GUMBEL_EPS = 2.0 ** -15  # how far the kernel's fp32 perturbed value y + g may lie from the float64 rule's, for |y| <= 128
_M32 = 0xFFFFFFFF


def _hash32(x):
    """csrc/common.h's obte_hash32 on an int64 tensor of 32-bit values (int64 products wrap mod 2^64: the low 32 bits are right)"""
    x = x & _M32
    x = x ^ (x >> 16)
    x = (x * 0x7FEB352D) & _M32
    x = x ^ (x >> 15)
    x = (x * 0x846CA68B) & _M32
    return x ^ (x >> 16)


def _rowkey(keys, seed, site=SITE_FILL):
    """drop_rowkey(key, make_drop(0, seed, site)): int64 keys of any shape -> 32-bit values as int64"""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    s0 = (seed & _M32) ^ ((site * 0x632BE5AB) & _M32)
    s1 = ((seed >> 32) + site * 0x9E3779B9) & _M32
    k = torch.as_tensor(keys, dtype=torch.int64)
    lo, hi = k & _M32, (k >> 32) & _M32
    return _hash32((_hash32(lo ^ s0) + ((hi * 0x9E3779B1) & _M32) + s1) & _M32)


def gumbel_of_hash(h):
    """g = -ln(-ln(1 - w)), w = (h + 0.5) 2^-32, float64, for 32-bit values h (an int64 tensor).  1 - w = (2^32 - h - 0.5) 2^-32 is exact
    in float64, so this is the rule to the last bits of two float64 logarithms; finite for every h: |g| < 23."""
    h = torch.as_tensor(h, dtype=torch.int64)
    u = ((1 << 32) - h).double() - 0.5                         # exact: below 2^53
    return -torch.log(-torch.log(u * 2.0 ** -32))


def gumbel_noise(seed, keys, V):
    """(n, V) float64: the noise of columns 0 .. V - 1 for the rows with the int64 ``keys`` (n,) under ``seed``:
    g[i, v] = gumbel_of_hash(obte_hash32(rowkey(keys[i]) ^ v))."""
    k = torch.as_tensor(keys, dtype=torch.int64)
    if k.dim() != 1 or V < 1:
        raise ValueError(f"gumbel_noise: keys must be (n,) and V >= 1, got {tuple(k.shape)} and {V}")
    col = torch.arange(V, dtype=torch.int64, device=k.device)
    return gumbel_of_hash(_hash32(_rowkey(k, seed).unsqueeze(1) ^ col.unsqueeze(0)))


def inv_temperature(temperature):
    """The fp32 number the kernel multiplies the logits by, as a Python float: fp32(1 / temperature); 0 for temperature 0 (greedy)"""
    t = float(temperature)
    if not t >= 0 or t == float("inf"):
        raise ValueError(f"temperature must be finite and not negative, got {temperature}")
    if t == 0:
        return 0.0
    it = float(torch.tensor(1.0 / t, dtype=torch.float64).to(torch.float32))
    if it == float("inf"):
        raise ValueError(f"temperature {temperature} is too small: 1 / temperature overflows fp32")
    return it


def readout_sample_reference(x, w, temperature, seed, keys=None, allowed=None, alpha=1.0):
    """(tokens int64 (R,), logprob (R,), lse (R,), perturbed (R, V), y (R, V)), the last four float64: the rule of
    obte_readout_sample_bf16.  z = bf16(alpha x w^T) from the float64 product (the kernel's z when its fp32 sum is exact),
    y = z inv_temperature(temperature), -inf where ``allowed`` (bool (V,) or (R, V)) is False; perturbed = y + gumbel_noise(seed, keys);
    token = the first index of the maximum of perturbed, lse = logsumexp(y), logprob = y[token] - lse.  temperature 0: no noise, the
    first index of the maximum of z over the allowed columns, lse and logprob at temperature 1.  A row with no finite allowed y:
    token -1, logprob -inf.  ``keys`` None: the row numbers."""
    if x.dim() != 2 or w.dim() != 2 or x.shape[1] != w.shape[1]:
        raise ValueError(f"readout_sample_reference: x (R, C) and w (V, C), got {tuple(x.shape)} and {tuple(w.shape)}")
    r, v = x.shape[0], w.shape[0]
    it = inv_temperature(temperature)
    z = (float(alpha) * (x.double() @ w.double().t())).to(torch.bfloat16).double()
    y = constrain_reference(z * (it if it > 0 else 1.0), allowed)
    if it > 0:
        k = torch.arange(r, dtype=torch.int64) if keys is None else torch.as_tensor(keys, dtype=torch.int64)
        if k.shape != (r,):
            raise ValueError(f"readout_sample_reference: keys must be ({r},), got {tuple(k.shape)}")
        pert = y + gumbel_noise(seed, k.to(y.device), v)
    else:
        pert = y.clone()
    best = pert.max(dim=1, keepdim=True).values
    col = torch.arange(v, device=y.device).unsqueeze(0)
    some = torch.isfinite(best.squeeze(1))
    token = torch.where(pert == best, col, v).min(dim=1).values
    token = torch.where(some, token, torch.full_like(token, -1))
    lse = torch.logsumexp(y, dim=1)
    ninf = torch.full_like(lse, float("-inf"))
    logprob = torch.where(some, y.gather(1, token.clamp(min=0).unsqueeze(1)).squeeze(1) - torch.where(some, lse, torch.zeros_like(lse)), ninf)
    return token, logprob, torch.where(some, lse, ninf), pert, y


def fill_schedule(m, steps):
    """How many of ``m`` masked positions each of ``steps`` iterations commits: with rem left and steps - s iterations to go, iteration s
    takes ceil(rem / (steps - s)).  The list sums to m and never increases; steps > m: one per iteration, then nothing."""
    if isinstance(m, bool) or isinstance(steps, bool) or not isinstance(m, int) or not isinstance(steps, int) or m < 0 or steps < 1:
        raise ValueError(f"fill_schedule: m >= 0 and steps >= 1 integers, got {m!r} and {steps!r}")
    out, rem = [], m
    for s in range(steps):
        k = -(-rem // (steps - s))
        out.append(k)
        rem -= k
    return out


def fill_iteration_seed(seed, s):
    """The seed of iteration ``s`` of an unmasking loop run under ``seed``: (seed + s 0x9E3779B97F4A7C15) mod 2^64"""
    return (int(seed) + int(s) * 0x9E3779B97F4A7C15) & 0xFFFFFFFFFFFFFFFF


FILL_ORDERS = ("confidence", "random", "left")


def fill_commit_reference(rows, seg_off, tokens, logprob, take, order, seed, idx, out_logprob, seg_off_next, rows_next=None):
    """obte_fill_commit in plain torch on any device; nothing is changed in place.  ``rows`` int64 (n,) ascending flat positions, sequence
    b's entries the run [seg_off[b], seg_off[b + 1]); ``tokens`` and ``logprob`` (n,) belong to them; ``take`` (B,) of each sequence's
    entries are selected — ``order`` "confidence": larger logprob first, NaN as -inf; "random": smaller drop_rowkey(position) under
    ``seed`` first; "left": lowest position first; equal ranks to the lower position — and written through to copies of ``idx`` (flat
    int64) and ``out_logprob`` (flat fp32); the other positions go, ascending, to ``rows_next`` at seg_off_next[b].  take[b] outside
    [0, n_b]: nothing selected.  Returns (idx, out_logprob, rows_next); rows_next starts as the argument's copy, or -1 everywhere in
    seg_off_next[-1] entries."""
    if order not in FILL_ORDERS:
        raise ValueError(f"fill_commit_reference: order must be one of {FILL_ORDERS}, got {order!r}")
    so, sn, tk = [int(v) for v in seg_off], [int(v) for v in seg_off_next], [int(v) for v in take]
    idx, out_logprob = idx.clone(), out_logprob.clone()
    nxt = torch.full((sn[-1],), -1, dtype=torch.int64, device=rows.device) if rows_next is None else rows_next.clone()
    for b in range(len(tk)):
        lo, hi = so[b], so[b + 1]
        nb = hi - lo
        k = tk[b] if 0 <= tk[b] <= nb else 0
        pos = rows[lo:hi]
        if order == "confidence":
            lp = logprob[lo:hi].double()
            key = -torch.where(torch.isnan(lp), torch.full_like(lp, float("-inf")), lp)
        elif order == "random":
            key = _rowkey(pos.cpu(), seed).to(rows.device)
        else:
            key = torch.zeros(nb, dtype=torch.int64, device=rows.device)
        first = torch.sort(key, stable=True).indices[:k]                      # stable: equal ranks to the lower position
        sel = torch.zeros(nb, dtype=torch.bool, device=rows.device)
        sel[first] = True
        idx[pos[sel]] = tokens[lo:hi][sel].to(idx.dtype)
        out_logprob[pos[sel]] = logprob[lo:hi][sel].to(out_logprob.dtype)
        rest = pos[~sel]
        nxt[sn[b]:sn[b] + rest.numel()] = rest
    return idx, out_logprob, nxt


# ---- beam search (include/omnibiote_hip_beam.h) ------------------------------------------------------------------------------------
def beam_step_reference(logits, score, done, ancestry, slot, W, eos_token=None, allowed=None):
    """One beam step, obte_beam_select_bf16's rule in float64 on the CPU.  ``logits`` (B, V), B = P * W rows, row b = p * W + g; ``score``
    (B,), ``done`` (B,), ``ancestry`` (B, T_suf) integers, ``slot`` the suffix slot of the chosen tokens; ``allowed``: None, bool (V,) or (B, V).

      - a live row (score finite, not done) proposes (b, v) for every column v that is not NaN, not -inf and not excluded, with
        S = score[b] + (x_v - max_b) - ln Z_b, Z_b the sum of exp(x - max_b) over the row's candidate columns; a column whose S is -inf
        as an fp32 number is no candidate;
      - a done row with a finite score proposes (b, eos_token) alone (token 0 without an eos_token) with S = score[b];
      - a dead row (score not finite) and a row without a candidate column propose nothing;
      - per group the W best by S descending take the group's rows in rank order, equal S to the lower beam, then the lower token;
      - done_out = done[parent] or token == eos_token; a rank without a candidate is dead: parent the row itself, token eos_token (0
        if none), score -inf, done;
      - ancestry_out[b, j] = ancestry[parent[b], j] for j < slot and ancestry_out[b, slot] = b % W.

    Returns (parent (B,) int64 global rows, token (B,) int64, score_out (B,) float64, done_out (B,) bool, ancestry_out (B, slot + 1)
    int64, sorted): ``sorted`` is, per group, the float64 scores of its best candidates in that order — the W that placed and the next
    one where there is one, for a test's margins."""
    x = torch.as_tensor(logits).detach().cpu().double()
    b, v = x.shape
    if W < 1 or b % W:
        raise ValueError(f"beam_step_reference: {b} rows are not groups of W = {W}")
    score = torch.as_tensor(score).detach().cpu().double().reshape(b)
    done = torch.as_tensor(done).detach().cpu().reshape(b) != 0
    anc = torch.as_tensor(ancestry).detach().cpu().to(torch.int64)
    eos = -1 if eos_token is None else int(eos_token)
    fill = 0 if eos < 0 else eos
    ok = ~(torch.isnan(x) | (x == float("-inf")))
    if allowed is not None:
        ok = ok & torch.as_tensor(allowed).detach().cpu().bool().expand(b, v)
    xm = torch.where(ok, x, torch.full_like(x, float("-inf")))
    cands = []                                                   # per row: [(S, beam, token)]
    for r in range(b):
        g, out = r % W, []
        if not torch.isfinite(score[r]):
            pass
        elif done[r]:
            out.append((float(score[r]), g, fill))
        elif bool(ok[r].any()):
            mx = xm[r].max()
            d = torch.where(xm[r] == mx, torch.zeros_like(xm[r]), xm[r] - mx)          # (the maximum's own x - max is 0: inf - inf is never formed)
            d = torch.where(ok[r], d, torch.full_like(d, float("-inf")))
            s = score[r] + d - torch.log(torch.exp(d).sum())
            top = torch.sort(s, descending=True, stable=True)                          # stable: equal S to the lower token
            for sv, tv in zip(top.values[:W + 1].tolist(), top.indices[:W + 1].tolist()):
                if ok[r, tv] and torch.tensor(sv, dtype=torch.float32).item() != float("-inf"):
                    out.append((sv, g, tv))
        cands.append(out)
    parent = torch.empty(b, dtype=torch.int64)
    token = torch.empty(b, dtype=torch.int64)
    s_out = torch.empty(b, dtype=torch.float64)
    d_out = torch.empty(b, dtype=torch.bool)
    a_out = torch.empty((b, slot + 1), dtype=torch.int64)
    ranked = []
    for p in range(b // W):
        row0 = p * W
        group = sorted((c for r in range(row0, row0 + W) for c in cands[r]), key=lambda c: (-c[0], c[1], c[2]))
        ranked.append(torch.tensor([c[0] for c in group[:W + 1]], dtype=torch.float64))
        for r in range(W):
            i = row0 + r
            if r < len(group):
                sv, g, tv = group[r]
                parent[i], token[i], s_out[i], d_out[i] = row0 + g, tv, sv, bool(done[row0 + g]) or tv == eos
            else:
                parent[i], token[i], s_out[i], d_out[i] = i, fill, float("-inf"), True
            a_out[i, :slot] = anc[parent[i], :slot]
            a_out[i, slot] = r
    return parent, token, s_out, d_out, a_out, ranked


def beam_sequences_reference(token_hist, ancestry, n, W, eos_token=None, pad_token=None):
    """The new tokens of every beam from a beam search's two tables: ``token_hist`` (T_suf, B) — row j the tokens chosen at step j, by
    the row they went to — and the final ``ancestry`` (B, T_suf) — the local beam that held row b's token of step j: sequences[b, j] =
    token_hist[j, b - b % W + ancestry[b, j]] for j < n.  ``lengths`` counts the tokens up to and including the first ``eos_token`` (n
    without one); the positions behind it hold ``pad_token`` (default: eos_token, or 0).  Returns (sequences (B, n) int64, lengths (B,) int64)."""
    th = torch.as_tensor(token_hist).to(torch.int64)
    anc = torch.as_tensor(ancestry).to(torch.int64)
    b = anc.shape[0]
    rows = (torch.arange(b, device=anc.device) // W * W).unsqueeze(1) + anc[:, :n]                     # (B, n): the row that held the token
    seq = th[:n].t().gather(0, rows) if n > 0 else torch.empty((b, 0), dtype=torch.int64, device=anc.device)
    lengths = torch.full((b,), n, dtype=torch.int64, device=anc.device)
    if eos_token is not None and n > 0:
        hit = seq == int(eos_token)
        first = torch.where(hit.any(dim=1), hit.int().argmax(dim=1) + 1, lengths)
        lengths = first
        pad = int(eos_token) if pad_token is None else int(pad_token)
        seq = torch.where(torch.arange(n, device=anc.device).unsqueeze(0) >= lengths.unsqueeze(1), torch.full_like(seq, pad), seq)
    return seq, lengths
