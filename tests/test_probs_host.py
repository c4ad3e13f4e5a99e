"""Attention maps, host side: the rule (omnibiote_amd/attnmaps.py) against the oracle's attention, its exact zeros and uniform rows,
the average-product correction, and the argument checks of OmniBioTA.attention_maps on a CPU model.  No GPU."""
import numpy as np
import pytest
import torch

import omnibiote_ref as R
from omnibiote_amd.attnmaps import apc, attention_probs_reference, head_mean

BF = torch.bfloat16


def _qkv(B, T, H, hs, seed):
    """tests/test_hip_ops.py::_attn_case: a seeded bf16 qkv and its float q, k, v as (B, H, T, hs)"""
    C = H * hs
    g = torch.Generator().manual_seed(seed)
    qkv = torch.randn(B, T, 3 * C, generator=g).to(BF)
    q, k, v = [t.reshape(B, T, H, hs).transpose(1, 2).double() for t in qkv.split(C, dim=2)]
    return qkv, q, k, v


def _doc_masks(B, T, seed):
    rng = np.random.default_rng(seed)
    tokens = rng.integers(20, 100, size=(B, T))
    tokens[0, [T // 3, T // 2]] = R.EOS_TOKEN
    tokens[1, [5, T - 10]] = R.EOS_TOKEN
    blocks = R.document_blocks(tokens)
    return R.dense_mask_from_blocks(blocks, T), torch.from_numpy(R.key_ranges_from_blocks(blocks, T))


def _causal(B, T):
    r = torch.zeros(B, T, 2, dtype=torch.int32)
    r[:, :, 1] = torch.arange(1, T + 1, dtype=torch.int32)
    return r, torch.where(torch.tril(torch.ones(T, T, dtype=torch.bool)), 0.0, R.MASKED_VALUE).expand(B, T, T)


@pytest.mark.parametrize("mode", ["none", "ranges", "dense", "causal"])
def test_rule_times_v_is_the_oracles_attention(mode):
    B, T, H, hs = 2, 77, 2, 64
    scale = 8.0 / (H * hs)
    qkv, q, k, v = _qkv(B, T, H, hs, seed=3)
    dense, ranges = _doc_masks(B, T, seed=T)
    mask_add, kw = None, {}
    if mode == "ranges":
        mask_add, kw = dense, dict(key_ranges=ranges)
    elif mode == "dense":
        mask_add, kw = dense, dict(mask_add=dense.unsqueeze(1))
    elif mode == "causal":
        cr, mask_add = _causal(B, T)
        kw = dict(key_ranges=cr)
    P = attention_probs_reference(qkv, H, scale, **kw)
    assert P.dtype == torch.float64 and tuple(P.shape) == (B, H, T, T)
    ref = R.attention(q, k, v, scale, None if mask_add is None else mask_add.unsqueeze(1).double())
    assert (P @ v - ref).abs().max().item() <= 1e-12


def test_excluded_keys_are_exact_zeros_rows_sum_to_one_and_an_empty_range_is_zeros():
    B, T, H, hs = 2, 70, 2, 64
    qkv, _, _, _ = _qkv(B, T, H, hs, seed=5)
    _, ranges = _doc_masks(B, T, seed=1)
    ranges = ranges.clone()
    ranges[1, 33] = torch.tensor([12, 12])          # an empty range
    P = attention_probs_reference(qkv, H, 0.0625, key_ranges=ranges)
    j = torch.arange(T).view(1, 1, T)
    inside = ((j >= ranges[:, :, 0:1]) & (j < ranges[:, :, 1:2])).unsqueeze(1).expand_as(P)
    assert torch.equal(P[~inside], torch.zeros_like(P[~inside]))
    assert (P[inside] > 0).all()
    sums = P.sum(-1)
    assert torch.equal(sums[1, :, 33], torch.zeros(H, dtype=torch.float64)) and torch.isfinite(P).all()
    sums[1, :, 33] = 1.0
    assert (sums - 1.0).abs().max().item() <= 1e-14


def test_key_padding_rows_are_exactly_uniform_in_fp32_and_not_in_fp64():
    B, T, H, hs, pad = 2, 40, 2, 64, 29
    qkv, _, _, _ = _qkv(B, T, H, hs, seed=7)
    allowed = torch.zeros(T, T, dtype=torch.bool)
    allowed[:pad, :pad] = True                       # the reference's pad_attn: rows and columns beyond the pad position are masked
    mask = torch.where(allowed, 0.0, R.MASKED_VALUE).expand(B, 1, T, T)
    P32 = attention_probs_reference(qkv, H, 0.0625, mask_add=mask, dtype=torch.float32)
    assert P32.dtype == torch.float32
    assert torch.equal(P32[:, :, pad:], torch.full((B, H, T - pad, T), 1.0 / T, dtype=torch.float32))
    assert torch.equal(P32[:, :, :pad, pad:], torch.zeros(B, H, pad, T - pad))
    P64 = attention_probs_reference(qkv, H, 0.0625, mask_add=mask)
    assert (P64[:, :, pad:] - 1.0 / T).abs().max().item() > 1e-3     # float64 keeps the scores beside -1e9
    assert (P64[:, :, :pad].float() - P32[:, :, :pad]).abs().max().item() <= 1e-6


def test_head_mean_adds_the_heads_in_ascending_order_in_fp32():
    g = torch.Generator().manual_seed(2)
    P = torch.rand(2, 3, 5, 5, generator=g, dtype=torch.float64)
    want = ((P[:, 0].float() + P[:, 1].float()) + P[:, 2].float()) * torch.tensor(1.0 / 3.0, dtype=torch.float32)
    got = head_mean(P)
    assert got.dtype == torch.float32 and torch.equal(got, want)


def test_apc_is_symmetric_with_vanishing_row_and_column_sums():
    g = torch.Generator().manual_seed(4)
    M = torch.rand(2, 3, 17, 17, generator=g, dtype=torch.float64)
    A = apc(M)
    assert A.dtype == torch.float64 and A.shape == M.shape
    assert torch.equal(A, A.transpose(-2, -1))
    assert A.sum(-1).abs().max().item() <= 1e-13 and A.sum(-2).abs().max().item() <= 1e-13
    F = (M + M.transpose(-2, -1)) / 2
    i, j = 3, 11
    want = F[1, 2, i, j] - F[1, 2, i].sum() * F[1, 2, :, j].sum() / F[1, 2].sum()
    assert abs(A[1, 2, i, j].item() - want.item()) <= 1e-14


def _model(n_layer=3):
    from omnibiote_amd.model import OmniBioTA, OmniBioTAConfig
    c = OmniBioTAConfig()
    c.block_size, c.vocab_size, c.n_layer, c.n_head, c.n_embd, c.dropout, c.flash = 32, 64, n_layer, 2, 128, 0.1, True
    return OmniBioTA(c)


def test_attention_maps_validates_before_any_device_work():
    m = _model().train()
    idx = torch.zeros(2, 8, dtype=torch.int64)
    for layers, word in (([1, 0], "ascending"), ([1, 1], "ascending"), ([0, 3], r"\[0, 3\)"), ([-1], r"\[0, 3\)"), ([], "non-empty"),
                         ([0.5], "non-empty"), (1, "non-empty")):
        with pytest.raises(ValueError, match=word):
            m.attention_maps(idx, layers=layers)
    with pytest.raises(ValueError, match="heads"):
        m.attention_maps(idx, heads="max")
    with pytest.raises(ValueError, match="heads"):
        m.attention_maps(idx, heads=[0])
    for dtype in (torch.float16, torch.float64, "fp32"):
        with pytest.raises(ValueError, match="dtype"):
            m.attention_maps(idx, dtype=dtype)
    with pytest.raises(ValueError, match="idx"):
        m.attention_maps(idx.int())
    with pytest.raises(ValueError, match="block size"):
        m.attention_maps(torch.zeros(2, 33, dtype=torch.int64))
    # valid arguments reach the device check (a CPU model has no attention to show), and the flags are as before
    with pytest.raises(RuntimeError, match="MI355X|GPU|HIP"):
        m.attention_maps(idx, layers=[0, 2], heads="mean", dtype=torch.bfloat16)
    assert all(mod.training for mod in m.modules())


def test_ops_attn_probs_has_no_cpu_fallback_and_checks_its_words():
    from omnibiote_amd import ops
    qkv = torch.zeros(1, 8, 3 * 128, dtype=BF)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.attn_probs(qkv, 1, 8, 2, 64, 0.0625)
    with pytest.raises(ValueError, match="heads"):
        ops.attn_probs(qkv, 1, 8, 2, 64, 0.0625, heads="sum")
    with pytest.raises(ValueError, match="dtype"):
        ops.attn_probs(qkv, 1, 8, 2, 64, 0.0625, dtype=torch.float16)
