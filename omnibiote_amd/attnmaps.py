"""Attention maps, the rule in plain torch: what ``ops.attn_probs`` / ``OmniBioTA.attention_maps`` compute, stated without any GPU code
(the yardstick of tests/test_probs_host.py and tests/test_hip_probs.py, as sampling.py, scoring.py and paged.py are for theirs).

The reference forms these weights with ``flash=False`` (training/model.py, CausalSelfAttention): ``att = softmax(q k^T * 8 / n_embd +
mask)``, handed through ``attn_dropout`` where a forward hook can read them.  ``apc`` is the average-product correction contact-map
work applies to such maps; it exists in torch only."""
from __future__ import annotations

import torch


def attention_probs_reference(qkv, n_head, scale, mask_add=None, key_ranges=None, dtype=torch.float64):
    """The softmax weights (B, H, T, T) of one attention layer.

    ``qkv``: the packed, already rotated (B, T, 3C) activation as ``ops.attn_fwd`` reads it (head h at column h * hs, k at + C).
    Scores s_ij = (q_i . k_j) * scale, plus ``mask_add`` (broadcastable to (B, H, T, T)) when given.  With ``key_ranges`` (B, T, 2),
    [k_start, k_end) per query, the keys outside the range are excluded: their weight is exactly 0.  P = exp(s - m) / l with m the
    row maximum and l the row sum over the included keys; an empty range gives a row of zeros.  All arithmetic in ``dtype``:
    float64 is the yardstick, float32 the rule as the kernel must evaluate it — for a row of a dense mask whose every key carries
    -1e9 the score is absorbed in fp32 and the row is uniform 1 / T, as in the reference's own arithmetic; in float64 it is not."""
    B, T, C3 = qkv.shape
    C = C3 // 3
    hs = C // n_head
    q, k, _ = qkv.to(dtype).split(C, dim=2)
    q = q.reshape(B, T, n_head, hs).transpose(1, 2)
    k = k.reshape(B, T, n_head, hs).transpose(1, 2)
    s = (q @ k.transpose(-2, -1)) * torch.tensor(scale, dtype=dtype)
    if mask_add is not None:
        s = s + mask_add.to(dtype)
    inc = torch.ones((B, 1, T, T), dtype=torch.bool)
    if key_ranges is not None:
        r = key_ranges.to(torch.int64).cpu()
        j = torch.arange(T).view(1, 1, T)
        inc = ((j >= r[:, :, 0:1]) & (j < r[:, :, 1:2])).unsqueeze(1)
    inc = inc.expand(B, n_head, T, T)
    neg = torch.full_like(s, float("-inf"))
    s = torch.where(inc, s, neg)
    m = s.max(dim=-1, keepdim=True).values
    m = torch.where(torch.isinf(m), torch.zeros_like(m), m)   # nothing included (or everything at -inf): exp(-inf - 0) = 0
    e = torch.where(inc, torch.exp(s - m), torch.zeros_like(s))
    l = e.sum(dim=-1, keepdim=True)
    return torch.where(l > 0, e / torch.where(l > 0, l, torch.ones_like(l)), torch.zeros_like(e))


def head_mean(P):
    """The mean over the head axis of (B, H, T, T) weights -> (B, T, T), fp32, the heads added in ascending order."""
    P = P.to(torch.float32)
    acc = P[:, 0].clone()
    for h in range(1, P.shape[1]):
        acc = acc + P[:, h]
    return acc * torch.tensor(1.0 / P.shape[1], dtype=torch.float32)


def apc(maps):
    """Symmetrise over the last two axes, F = (M + M^T) / 2, then the average-product correction F_ij - F_i. F_.j / F_.. (row sum
    times column sum over the total).  Any leading axes; the dtype of ``maps`` is kept."""
    F = (maps + maps.transpose(-2, -1)) / 2
    rows = F.sum(dim=-1, keepdim=True)
    cols = rows.transpose(-2, -1)          # F is symmetric: its column sums ARE its row sums, and the result stays symmetric bit for bit
    total = rows.sum(dim=-2, keepdim=True)
    return F - rows * cols / total
