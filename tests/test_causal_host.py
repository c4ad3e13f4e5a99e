"""Autoregressive mode, host side (CPU only): the causal pair of range tables built by tensor ops, and the oracle under a
tril mask pinned against vectors captured from the reference's own autoregressive model (tools/gen_golden_causal.py)."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import omnibiote_ref as R
from omnibiote_amd.masks import RangeMask


# ------------------------------------------------------------------------------------------------ table construction
def _tokens():
    """Multi-document rows: row 0 two EOS, row 1 three EOS (a row >= 1 with two or more: its first two documents share one
    block, the reference's merge quirk), row 2 none, row 3 EOS at both ends and two in a row."""
    B, T = 4, 45
    tok = np.random.default_rng(0).integers(20, 100, size=(B, T)).astype(np.int64)
    tok[0, [7, 30]] = R.EOS_TOKEN
    tok[1, [4, 19, 33]] = R.EOS_TOKEN
    tok[3, [0, 21, 22, T - 1]] = R.EOS_TOKEN
    return tok


def _columns(allowed):
    """brute force: [first, last + 1) of every column of a (B, T, T) boolean mask, contiguity checked; empty: None"""
    B, T, _ = allowed.shape
    out = {}
    for b in range(B):
        for k in range(T):
            qs = np.nonzero(allowed[b, :, k])[0]
            if len(qs) == 0:
                out[b, k] = None
                continue
            assert len(qs) == qs[-1] - qs[0] + 1, f"column ({b}, {k}) is not one contiguous run"
            out[b, k] = (int(qs[0]), int(qs[-1]) + 1)
    return out


def _check_pair(rm, want_allowed):
    B, T, _ = want_allowed.shape
    assert rm.query_bounds is not None and rm.query_bounds.dtype == torch.int32 and tuple(rm.query_bounds.shape) == (B, T, 2)
    np.testing.assert_array_equal((rm.dense(torch.float32) == 0).numpy(), want_allowed)
    qb = rm.query_bounds.numpy()
    for (b, k), run in _columns(want_allowed).items():
        if run is None:
            assert qb[b, k, 0] == qb[b, k, 1], (b, k)          # an empty result is [x, x)
        else:
            assert tuple(qb[b, k]) == run, (b, k, tuple(qb[b, k]), run)
    kr = rm.key_ranges.numpy()
    assert (kr[..., 1] >= kr[..., 0]).all() and (qb[..., 1] >= qb[..., 0]).all()


def test_causal_tables_without_documents():
    for B, T in [(1, 1), (2, 33), (3, 64)]:
        rm = RangeMask.causal(B, T, "cpu")
        tril = np.broadcast_to(np.tril(np.ones((T, T), dtype=bool)), (B, T, T))
        _check_pair(rm, tril)
        t = np.arange(T)
        np.testing.assert_array_equal(rm.key_ranges.numpy(), np.broadcast_to(np.stack([0 * t, t + 1], 1), (B, T, 2)))
        np.testing.assert_array_equal(rm.query_bounds.numpy(), np.broadcast_to(np.stack([t, 0 * t + T], 1), (B, T, 2)))


@pytest.mark.parametrize("group", [0, 2])
def test_document_causal_tables_are_tril_and_document_mask(group):
    tok = _tokens()
    B, T = tok.shape
    ids = torch.from_numpy(tok)
    doc = RangeMask.from_tokens(ids, padding=False, group=group)
    assert doc.query_bounds is None                                   # the symmetric mask is unchanged
    if group == 0:   # the independent restatement of the reference's builder (quirk included) agrees on the document part
        np.testing.assert_array_equal((doc.dense(torch.float32) == 0).numpy(),
                                      (R.dense_mask_from_blocks(R.document_blocks(tok), T) == 0).numpy())
        assert tuple(doc.key_ranges[1, 0].tolist()) == (0, 20)        # the merge quirk: row 1's first two documents are one block
    allowed = (doc.dense(torch.float32) == 0).numpy() & np.tril(np.ones((T, T), dtype=bool))[None]
    rm = RangeMask.from_tokens(ids, padding=False, group=group, causal=True)
    _check_pair(rm, allowed)
    moved = rm.to("cpu")
    assert torch.equal(moved.key_ranges, rm.key_ranges) and torch.equal(moved.query_bounds, rm.query_bounds)


def test_document_causal_tables_with_a_pad_tail():
    """padding=True: the PAD tail after the last EOS has the empty range, as a query and as a key."""
    tok = _tokens()
    tok[1, 34:] = 1
    ids = torch.from_numpy(tok)
    doc = RangeMask.from_tokens(ids, padding=True)
    allowed = (doc.dense(torch.float32) == 0).numpy() & np.tril(np.ones((tok.shape[1],) * 2, dtype=bool))[None]
    assert not allowed[1, 34:].any() and not allowed[1, :, 34:].any()
    _check_pair(RangeMask.from_tokens(ids, padding=True, causal=True), allowed)


def test_range_mask_constructor_checks_the_second_table():
    kr = torch.zeros(2, 5, 2, dtype=torch.int32)
    assert RangeMask(kr).query_bounds is None
    with pytest.raises(AssertionError):
        RangeMask(kr, torch.zeros(2, 4, 2, dtype=torch.int32))
    with pytest.raises(AssertionError):
        RangeMask(kr, torch.zeros(2, 5, 2, dtype=torch.int64))


# ------------------------------------------------------------------------------------------- oracle against the reference
def _load(golden_dir, name):
    return np.load(os.path.join(golden_dir, name + ".npz"))


def _cfg(g):
    bs, V, L, H, C, flash = [int(v) for v in g["cfg"]]
    return R.RefConfig(block_size=bs, vocab_size=V, n_layer=L, n_head=H, n_embd=C, flash=bool(flash), autoregressive=True)


def _tril_add(T):
    return torch.where(torch.tril(torch.ones(T, T, dtype=torch.bool)), 0.0, R.MASKED_VALUE).view(1, 1, T, T)


def _loss(logits, tokens):
    """The fixtures' loss (tools/gen_golden_causal.py): position t against token t + 1 over the first T - 1 positions, mean."""
    return F.cross_entropy(logits[:, :-1].reshape(-1, logits.shape[-1]), tokens[:, 1:].reshape(-1))


CAUSAL_CASES = ["tiny_fp32_causal", "tiny_fp32_causal_manual"]


def test_the_two_reference_runs_bound_each_other(golden_dir):
    """SDPA (is_causal=True) against the manual tril path of the reference.  Measured when the fixtures were written: emb 9.5e-7,
    logits 1.6e-7, loss 0, gradients <= 5.6e-7 of the tensor's largest entry — all inside the fp32 bars used below, so those
    bars stand as they are."""
    a, b = _load(golden_dir, CAUSAL_CASES[0]), _load(golden_dir, CAUSAL_CASES[1])
    np.testing.assert_array_equal(a["tokens"], b["tokens"])
    assert np.abs(a["emb"] - b["emb"]).max() <= 2e-5
    assert np.abs(a["logits"] - b["logits"]).max() <= 2e-5
    assert abs(float(a["loss"]) - float(b["loss"])) <= 2e-6
    for k in a.files:
        if k.startswith("grad_sample/"):
            assert np.abs(a[k] - b[k]).max() <= 1e-6 + 1e-4 * np.abs(a[k]).max(), k


@pytest.mark.parametrize("name", CAUSAL_CASES)
def test_oracle_with_a_tril_mask_matches_the_autoregressive_reference(golden_dir, name):
    g = _load(golden_dir, name)
    cfg = _cfg(g)
    tok = torch.from_numpy(g["tokens"])
    T = tok.shape[1]
    w = {k: v.requires_grad_(True) for k, v in R.hash_weights(cfg).items()}
    emb = R.model_forward(w, cfg, tok, _tril_add(T), return_embeddings=True)
    np.testing.assert_allclose(emb.detach().numpy(), g["emb"], rtol=0, atol=2e-5)
    logits = R.model_forward(w, cfg, tok, _tril_add(T))
    np.testing.assert_allclose(logits.detach().numpy(), g["logits"], rtol=0, atol=2e-5)
    loss = _loss(logits, tok)
    assert abs(loss.item() - float(g["loss"])) <= 2e-6
    loss.backward()
    stride = int(g["grad_stride"])
    for k, p in w.items():
        want = g["grad_sample/" + k]
        np.testing.assert_allclose(p.grad.flatten()[::stride].numpy(), want, rtol=0, atol=1e-6 + 1e-4 * np.abs(want).max(), err_msg=k)
        assert abs(p.grad.double().sum().item() - float(g["grad_sum/" + k])) <= 1e-4 * float(g["grad_abs/" + k]) + 1e-7, k


def test_the_fixture_is_causal_and_not_the_encoder(golden_dir):
    """Without the tril mask the oracle is clearly off the fixture: the fixtures pin the causal path, not the encoder's."""
    g = _load(golden_dir, CAUSAL_CASES[0])
    cfg = _cfg(g)
    emb = R.model_forward(R.hash_weights(cfg), cfg, torch.from_numpy(g["tokens"]), None, return_embeddings=True)
    assert np.abs(emb.numpy() - g["emb"]).max() > 1e-2
