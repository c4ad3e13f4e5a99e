"""Autoregressive mode on the GPU: causal attention as an ASYMMETRIC range mask (per-query key ranges + per-key query bounds)
through the attention kernels in both backward forms, the tables built on the device, and the block / model path of
``OmniBioTAConfig.autoregressive`` against the reference's own autoregressive runs (tests/golden/tiny_fp32_causal*.npz) and
against the CPU oracle under a tril mask."""
import os
import warnings

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import omnibiote_ref as R
from test_hip_ops import BF, DEV, _attn_case, close, rnd

pytestmark = pytest.mark.gpu


def ops():
    from omnibiote_amd import ops as o
    return o


def lib():
    from omnibiote_amd import _lib
    return _lib.lib()


def _tril(T):
    return torch.tril(torch.ones(T, T, dtype=torch.bool))


def _add(allowed):
    """boolean (.., T, T) -> the additive 0 / -1e9 mask, with a head axis"""
    m = torch.where(allowed, 0.0, R.MASKED_VALUE)
    return m.view(1, 1, *m.shape) if m.dim() == 2 else m.unsqueeze(1)


def _doc_tokens(B, T, seed):
    tok = np.random.default_rng(seed).integers(20, 100, size=(B, T)).astype(np.int64)
    tok[0, [T // 5, T // 2, T // 2 + 40]] = R.EOS_TOKEN      # documents that start and end inside / across key blocks
    tok[1, [3, T // 3, T - 7]] = R.EOS_TOKEN                 # a row >= 1 with several EOS: the merge quirk
    return tok


# =================================================================================================== kernels
def _attention_both_ways(B, T, H, hs, allowed, mask, seed):
    """ops.attn_fwd / attn_bwd under `mask` (a RangeMask with both tables) against R.attention on CPU fp32 with the additive
    form of `allowed`, autograd for the gradients.  Tolerances: the rule of tests/test_hip_ops.py's attention tests
    (2^-7 |ref| + an absolute term for the reduction length: 6e-3 forward, 1.5e-2 backward), the same helper."""
    o = ops()
    C = H * hs
    scale = 8.0 / C
    qkv, q, k, v = _attn_case(B, T, H, hs, seed=seed)
    qf, kf, vf = q.requires_grad_(True), k.requires_grad_(True), v.requires_grad_(True)
    mask_add = _add(allowed)
    ref = R.attention(qf, kf, vf, scale, mask_add)
    d_o = rnd(B, T, C, seed=seed + 1)
    ref.backward(d_o.reshape(B, T, H, hs).transpose(1, 2).float())
    dref = torch.cat([g.transpose(1, 2).reshape(B, T, C) for g in (qf.grad, kf.grad, vf.grad)], dim=2)
    spec = o.MaskSpec.from_user(mask, B, T, H, DEV)
    assert spec.dense is None and spec.ranges is not None and spec.qbounds is not None
    qd, dd = qkv.to(DEV), d_o.to(DEV)
    got, lse = o.attn_fwd(qd, B, T, H, hs, scale, spec)
    close(got, ref.transpose(1, 2).reshape(B, T, C), atol=6e-3, what=f"causal attn fwd hs={hs} T={T}")
    att = (q @ k.transpose(-2, -1)).detach() * scale + mask_add
    close(lse, torch.logsumexp(att, dim=-1), atol=2e-3, rtol=1e-3, what="lse")
    two = o.attn_bwd(qd, got, dd, lse, B, T, H, hs, scale, spec, one_kernel=False)
    close(two, dref, atol=1.5e-2, what=f"causal attn bwd (kernel pair) hs={hs} T={T}")
    if hs != 128:
        return
    assert lib().obte_attn_bwd_ws_bytes(B, T, H, hs) > 0      # the one-kernel form applies: that is what runs below
    one = o.attn_bwd(qd, got, dd, lse, B, T, H, hs, scale, spec, one_kernel=True)
    torch.cuda.synchronize()
    assert lib().obte_device_status(0) == 0, "the one-kernel backward's hand-off chain gave up under the causal slice ranges"
    again = o.attn_bwd(qd, got, dd, lse, B, T, H, hs, scale, spec, one_kernel=True)
    torch.cuda.synchronize()
    assert lib().obte_device_status(0) == 0
    assert torch.equal(one, again), "one-kernel backward is not run-to-run bitwise"
    close(one, dref, atol=1.5e-2, what=f"causal attn bwd (one kernel) hs={hs} T={T}")
    close(one, two.float().cpu(), atol=1.5e-2, what="one-kernel form vs kernel pair")
    # with the inverse RoPE of the epilogues, as the block calls it
    tab = torch.randn(T, hs // 2, generator=torch.Generator().manual_seed(1))
    rope = (torch.cos(tab).to(DEV), torch.sin(tab).to(DEV))
    one_r = o.attn_bwd(qd, got, dd, lse, B, T, H, hs, scale, spec, rope=rope)
    two_r = o.attn_bwd(qd, got, dd, lse, B, T, H, hs, scale, spec, rope=rope, one_kernel=False)
    torch.cuda.synchronize()
    assert lib().obte_device_status(0) == 0
    assert torch.equal(one_r, o.attn_bwd(qd, got, dd, lse, B, T, H, hs, scale, spec, rope=rope))
    close(one_r, two_r.float().cpu(), atol=1.5e-2, what="one-kernel form vs kernel pair, inverse RoPE")


# T crosses the 32-query slice, the 64-key tile, the 256-query block and the 256-key block; 600 and 1100: 3 and 5 key blocks in a chain
@pytest.mark.parametrize("hs,T", [(64, 1), (64, 33), (64, 257), (128, 33), (128, 257), (128, 600), (128, 1100)])
def test_causal_attention_against_the_oracle(hs, T):
    from omnibiote_amd.masks import RangeMask
    B, H = 2, 2
    _attention_both_ways(B, T, H, hs, _tril(T), RangeMask.causal(B, T, DEV), seed=hs + T)


def test_document_causal_attention_against_the_oracle():
    """document ∩ causal at T = 600, tables from the device builder: ragged slice ranges with a diagonal edge, both backward forms"""
    from omnibiote_amd.masks import RangeMask
    B, H, hs, T = 2, 2, 128, 600
    tok = _doc_tokens(B, T, 4)
    allowed = (R.dense_mask_from_blocks(R.document_blocks(tok), T) == 0) & _tril(T)
    _attention_both_ways(B, T, H, hs, allowed, RangeMask.from_tokens(torch.from_numpy(tok).to(DEV), causal=True), seed=9)


def test_causal_bounds_on_the_device_equal_the_tensor_ops(monkeypatch):
    from omnibiote_amd.masks import RangeMask
    o = ops()
    for B, T in [(1, 1), (3, 77), (2, 600)]:
        kr, qb = o.causal_bounds(None, B, T, DEV)
        cpu = RangeMask.causal(B, T, "cpu")
        assert torch.equal(kr.cpu(), cpu.key_ranges) and torch.equal(qb.cpu(), cpu.query_bounds)
    for padding in (False, True):
        tok = _doc_tokens(2, 600, 7)
        if padding:
            tok[1, 594:] = 1
        ids = torch.from_numpy(tok)
        cpu = RangeMask.from_tokens(ids, padding=padding, causal=True)                       # tensor ops
        doc = o.key_ranges_from_tokens(ids.to(DEV), R.EOS_TOKEN, padding, 0)
        kr, qb = o.causal_bounds(doc)                                                        # composes with the key-range launch
        assert torch.equal(kr.cpu(), cpu.key_ranges) and torch.equal(qb.cpu(), cpu.query_bounds)
        dev = RangeMask.from_tokens(ids.to(DEV), padding=padding, causal=True)               # the same through the mask class
        assert torch.equal(dev.key_ranges, kr) and torch.equal(dev.query_bounds, qb)
        monkeypatch.setenv("OBTE_PRELUDE_HIP", "0")                                          # GPU tensors, tensor ops
        alt = RangeMask.from_tokens(ids.to(DEV), padding=padding, causal=True)
        monkeypatch.delenv("OBTE_PRELUDE_HIP")
        assert torch.equal(alt.key_ranges, kr) and torch.equal(alt.query_bounds, qb)
    with pytest.raises(RuntimeError):
        o.causal_bounds(None, 0, 5, DEV)


# =================================================================================================== block and model
def _model(cfg: R.RefConfig, w, autoregressive, rope_mode="cos_only", flash=True):
    from omnibiote_amd.model import OmniBioTA, OmniBioTAConfig
    from omnibiote_amd.mup_compat import set_base_shapes
    c = OmniBioTAConfig()
    c.block_size, c.vocab_size, c.n_layer, c.n_head, c.n_embd, c.dropout, c.flash = cfg.block_size, cfg.vocab_size, cfg.n_layer, cfg.n_head, cfg.n_embd, 0.0, flash
    c.autoregressive = autoregressive
    m = OmniBioTA(c)
    cb = OmniBioTAConfig(); cb.block_size, cb.vocab_size, cb.n_layer, cb.dropout, cb.flash = cfg.block_size, cfg.vocab_size, cfg.n_layer, 0.0, True
    cb.n_embd, cb.n_head = 24, 3
    base = OmniBioTA(cb)
    cb.n_embd, cb.n_head = 48, 12
    delta = OmniBioTA(cb)
    set_base_shapes(m, base, delta=delta, rescale_params=False)
    m.load_state_dict(w, strict=False)
    if rope_mode == "cos_only":          # what the reference does: module.to(bfloat16)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            m.to(BF)
    else:                                # bf16 parameters, the complex RoPE buffer kept: the fp32 reference's rotation
        for p in m.parameters():
            p.data = p.data.to(BF)
    return m.to(DEV)


def _grad_bars(named_got, want_of, what):
    bad = []
    for k, g in named_got:
        got, want = g.float().cpu().flatten(), want_of(k)
        assert torch.isfinite(got).all(), k
        cos = (torch.dot(got, want) / (got.norm() * want.norm() + 1e-30)).item()
        rel = ((got - want).norm() / (want.norm() + 1e-30)).item()
        if not (cos >= 0.9995 and rel <= 0.04):
            bad.append((k, cos, rel))
    assert not bad, (what, bad)


def _stats(got, ref):
    d = (got.detach().float().cpu() - ref).abs()
    return d.max().item(), d.mean().item()


@pytest.mark.parametrize("name", ["tiny_fp32_causal", "tiny_fp32_causal_manual"])
def test_autoregressive_model_matches_the_reference_fixtures(golden_dir, name):
    """The reference's own autoregressive model (SDPA is_causal=True / its manual tril path) on the tiny config: emb, logits, the
    next-token loss and sampled gradients, at the model bars of DESIGN §3."""
    from omnibiote_amd import model as M
    g = np.load(os.path.join(golden_dir, name + ".npz"))
    bs, V, Lyr, H, C, flash = [int(v) for v in g["cfg"]]
    cfg = R.RefConfig(block_size=bs, vocab_size=V, n_layer=Lyr, n_head=H, n_embd=C)
    m = _model(cfg, R.hash_weights(cfg), True, rope_mode="complex", flash=bool(flash))
    assert ("transformer.h.0.attn.bias" in m.state_dict()) == (not flash)      # the tril buffer: registered as in the reference, unread
    idx = torch.from_numpy(g["tokens"]).to(DEV)
    mx, mean = _stats(m(idx, return_embeddings=True), torch.from_numpy(g["emb"]))
    assert mx <= 0.05 and mean <= 5e-3, (mx, mean)
    logits = m(idx)
    mx, mean = _stats(logits, torch.from_numpy(g["logits"]))
    assert mx <= 5e-3 and mean <= 1e-3, (mx, mean)
    loss = M.next_token_loss(logits, idx)
    assert abs(loss.item() - float(g["loss"])) <= 2e-3, (loss.item(), float(g["loss"]))
    loss.backward()
    stride = int(g["grad_stride"])
    _grad_bars([(k, p.grad.flatten()[::stride]) for k, p in m.named_parameters()], lambda k: torch.from_numpy(g["grad_sample/" + k]), name)


# ---- head size 128: 256d / 2h, 2 layers, T = 600 (three key blocks: the one-kernel backward under the block path) -----------------
WIDE = dict(block_size=600, vocab_size=512, n_layer=2, n_head=2, n_embd=256)
_cache = {}


def _wide():
    """weights, tokens and the oracle's causal run (computed once, shared, never modified)"""
    if not _cache:
        cfg = R.RefConfig(**WIDE)
        w = R.hash_weights(cfg)
        B, T = 2, WIDE["block_size"]
        tok = _doc_tokens(B, T, 11)
        ids = torch.from_numpy(tok)
        wb = {k: v.to(BF).float().requires_grad_(True) for k, v in w.items()}
        rope = R.cast_rope_table(R.rope_table(cfg.n_embd // cfg.n_head, T), BF)
        emb = R.model_forward(wb, cfg, ids, _add(_tril(T)), rope=rope, return_embeddings=True).detach()
        logits = R.model_forward(wb, cfg, ids, _add(_tril(T)), rope=rope)
        loss = F.cross_entropy(logits[:, :-1].reshape(-1, cfg.vocab_size), ids[:, 1:].reshape(-1))
        loss.backward()
        _cache.update(cfg=cfg, w=w, tok=tok, ids=ids, rope=rope, emb=emb, logits=logits.detach(), loss=loss.item(),
                      grads={k: v.grad.flatten() for k, v in wb.items()})
    return _cache


def test_autoregressive_model_head_size_128_vs_the_oracle():
    from omnibiote_amd import model as M
    c = _wide()
    m = _model(c["cfg"], c["w"], True)
    idx = c["ids"].to(DEV)
    mx, mean = _stats(m(idx, return_embeddings=True), c["emb"])
    assert mx <= 0.05 and mean <= 5e-3, (mx, mean)
    logits = m(idx)
    mx, mean = _stats(logits, c["logits"])
    assert mx <= 5e-3 and mean <= 1e-3, (mx, mean)
    loss = M.next_token_loss(logits, idx)
    assert abs(loss.item() - c["loss"]) <= 2e-3, (loss.item(), c["loss"])
    loss.backward()
    torch.cuda.synchronize()
    assert lib().obte_device_status(0) == 0
    _grad_bars([(k, p.grad) for k, p in m.named_parameters()], lambda k: c["grads"][k], "256d/2h T=600")


def test_causality_is_exact_in_the_model_and_in_the_block():
    """Tokens at positions >= t0 cannot reach positions < t0: bitwise.  t0 = 300 of T = 600 falls inside a 256-query block, a
    64-key tile's middle and a 32-query slice's middle.  Block level: a gradient that is zero at rows >= t0 leaves dx exactly zero there."""
    from omnibiote_amd.masks import RangeMask
    from omnibiote_amd.model import rope_tables
    c = _wide()
    cfg, T, t0 = c["cfg"], WIDE["block_size"], 300
    m = _model(cfg, c["w"], True)
    idx = c["ids"].to(DEV)
    other = idx.clone()
    other[:, t0:] = torch.randint(20, cfg.vocab_size, (idx.shape[0], T - t0), generator=torch.Generator().manual_seed(3)).to(DEV)
    with torch.no_grad():
        a, b = m(idx, return_embeddings=True), m(other, return_embeddings=True)
    assert torch.equal(a[:, :t0], b[:, :t0])
    assert not torch.equal(a[:, t0:], b[:, t0:])
    o = ops()
    B, C, H = 2, cfg.n_embd, cfg.n_head
    pre = "transformer.h.0."
    names = ["ln_1.weight", "attn.c_attn.weight", "attn.c_proj.weight", "ln_2.weight", "mlp.c_fc.weight", "mlp.c_proj.weight"]
    params = tuple(c["w"][pre + n].to(BF).to(DEV) for n in names)
    rope = rope_tables(c["rope"].to(DEV))
    spec = o.MaskSpec.from_user(RangeMask.causal(B, T, DEV), B, T, H, DEV)
    x, dy = rnd(B, T, C, seed=1).to(DEV), rnd(B, T, C, seed=2, scale=0.1).to(DEV)
    dy[:, t0:] = 0
    _, act = o.block_fwd(x, params, rope, H, spec)
    dx, _ = o.block_bwd(x, dy, act, params, rope, H, spec)
    torch.cuda.synchronize()
    assert lib().obte_device_status(0) == 0
    assert (dx[:, t0:] == 0).all() and (dx[:, :t0] != 0).any()


def test_forward_only_path_is_bitwise_the_training_forward(monkeypatch):
    c = _wide()
    m = _model(c["cfg"], c["w"], True)
    idx = c["ids"].to(DEV)
    with torch.no_grad():
        fast = m(idx)
        monkeypatch.setenv("OBTE_INFER", "0")
        train = m(idx)
    assert torch.equal(fast, train)
    mx, mean = _stats(fast, c["logits"])
    assert mx <= 5e-3 and mean <= 1e-3, (mx, mean)


def test_forward_rows_on_the_causal_model():
    """forward(rows=...): the last block's attention runs with its queries at the listed rows and needs each key's gathered-query
    interval from the per-key table (the symmetric derivation is wrong for a causal mask).  Bars: those of
    tests/test_hip_model.py::test_forward_rows_returns_the_listed_positions_of_the_full_forward."""
    c = _wide()
    cfg = c["cfg"]
    C, V, T = cfg.n_embd, cfg.vocab_size, WIDE["block_size"]
    m = _model(cfg, c["w"], True)
    idx = c["ids"].to(DEV)
    n = 90
    rows = torch.sort(torch.randperm(2 * T, generator=torch.Generator().manual_seed(1))[:n]).values.to(DEV)

    def near(a, b, atol, rtol):
        a, b = a.float(), b.float()
        assert ((a - b).abs() <= atol + rtol * b.abs()).all(), (a - b).abs().max().item()
    near(m(idx, return_embeddings=True, rows=rows), m(idx, return_embeddings=True).reshape(-1, C)[rows], 4e-3, 2.0 ** -7)
    near(m(idx, rows=rows), m(idx).reshape(-1, V)[rows], 2e-2, 2.0 ** -6)
    gsel = torch.randn(n, C, device=DEV, generator=torch.Generator(device=DEV).manual_seed(3)).to(BF) * 0.1
    grads = {}
    for tag in ("rows", "full"):
        m.zero_grad(set_to_none=True)
        out = m(idx, return_embeddings=True, rows=rows) if tag == "rows" else m(idx, return_embeddings=True).reshape(-1, C)[rows]
        out.backward(gsel)
        grads[tag] = {k: p.grad.float().clone() for k, p in m.named_parameters() if p.grad is not None}
    assert grads["rows"].keys() == grads["full"].keys()
    for k in grads["full"]:
        a, b = grads["rows"][k], grads["full"][k]
        assert (a - b).norm().item() <= 0.02 * b.norm().item() + 1e-6, k


def test_autoregressive_model_with_dropout_vs_oracle_with_the_restated_masks():
    """Training mode at dropout 0.1: the forward's keep bits feed the one-kernel backward under the causal pair; the oracle gets the
    product's restated masks.  Bars: those of tests/test_hip_headline.py's dropout step."""
    from omnibiote_amd import model as M
    from omnibiote_amd import train_encoder as TE
    c = _wide()
    cfg, T, p_drop = c["cfg"], WIDE["block_size"], 0.1
    m = _model(cfg, c["w"], True)
    TE.set_dropout(m, p_drop)
    m.train()
    idx = c["ids"].to(DEV)
    torch.manual_seed(77)
    seeds = [M._new_seed() for _ in range(1 + cfg.n_layer)]     # the embedding's, then one per block, in the order forward() draws them
    torch.manual_seed(77)
    logits = m(idx)
    loss = M.next_token_loss(logits, idx)
    loss.backward()
    torch.cuda.synchronize()
    assert lib().obte_device_status(0) == 0
    wb = {k: v.to(BF).float().requires_grad_(True) for k, v in c["w"].items()}
    ref_logits = R.model_forward(wb, cfg, c["ids"], _add(_tril(T)), rope=c["rope"], dropout=(p_drop, seeds))
    ref_loss = F.cross_entropy(ref_logits[:, :-1].reshape(-1, cfg.vocab_size), c["ids"][:, 1:].reshape(-1))
    ref_loss.backward()
    mx, mean = _stats(logits, ref_logits.detach())
    assert mx <= 2e-2 and mean <= 2e-3, (mx, mean)
    assert abs(loss.item() - ref_loss.item()) <= 0.02, (loss.item(), ref_loss.item())
    _grad_bars([(k, p.grad) for k, p in m.named_parameters()], lambda k: wb[k].grad.flatten(), "dropout 0.1")


def test_explicit_mask_on_an_autoregressive_model_is_not_causal_as_in_the_reference():
    """The reference's quirk (model.py:131-145, is_causal=False): with a mask given, an autoregressive model applies the mask alone.
    Bitwise the encoder's result, one warning for two calls."""
    from omnibiote_amd.masks import RangeMask
    c = _wide()
    idx = c["ids"].to(DEV)
    doc = RangeMask.from_tokens(idx)
    enc, ar = _model(c["cfg"], c["w"], False), _model(c["cfg"], c["w"], True)
    with torch.no_grad():
        want = enc(idx, attn_mask=doc, return_embeddings=True)
        with warnings.catch_warnings(record=True) as rec:
            warnings.simplefilter("default")
            got = ar(idx, attn_mask=doc, return_embeddings=True)
            got2 = ar(idx, attn_mask=doc, return_embeddings=True)
        causal = ar(idx, return_embeddings=True)
    assert torch.equal(got, want) and torch.equal(got2, want)
    assert not torch.equal(got, causal)
    assert len([r for r in rec if "NOT causal" in str(r.message)]) == 1, [str(r.message) for r in rec]


def test_document_causal_pair_under_either_config_vs_the_oracle():
    """RangeMask.from_tokens(ids, causal=True): tril ∧ document, under the encoder config (and, bitwise the same, handed explicitly to
    an autoregressive model)."""
    from omnibiote_amd.masks import RangeMask
    c = _wide()
    cfg, T = c["cfg"], WIDE["block_size"]
    idx = c["ids"].to(DEV)
    allowed = (R.dense_mask_from_blocks(R.document_blocks(c["tok"]), T) == 0) & _tril(T)
    wb = {k: v.to(BF).float().requires_grad_(True) for k, v in c["w"].items()}
    ref = R.model_forward(wb, cfg, c["ids"], _add(allowed), rope=c["rope"], return_embeddings=True)
    ref.square().sum().backward()
    enc = _model(cfg, c["w"], False)
    pair = RangeMask.from_tokens(idx, causal=True)
    emb = enc(idx, attn_mask=pair, return_embeddings=True)
    mx, mean = _stats(emb, ref.detach())
    assert mx <= 0.05 and mean <= 5e-3, (mx, mean)
    emb.float().square().sum().backward()
    torch.cuda.synchronize()
    assert lib().obte_device_status(0) == 0
    _grad_bars([(k, p.grad) for k, p in enc.named_parameters() if p.grad is not None], lambda k: wb[k].grad.flatten(), "document-causal")
    ar = _model(cfg, c["w"], True)
    with torch.no_grad(), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        assert torch.equal(ar(idx, attn_mask=pair, return_embeddings=True), emb.detach())


def test_selfattention_module_is_causal_under_the_flag():
    """The module-level SelfAttention (ops.attn_fwd / attn_bwd with the pair): an autoregressive module without a mask computes what
    the encoder's module computes under RangeMask.causal, bitwise, forward and backward, and not what it computes unmasked."""
    from omnibiote_amd.masks import RangeMask
    c = _wide()
    B, T, C = 2, 257, c["cfg"].n_embd
    enc, ar = _model(c["cfg"], c["w"], False).transformer.h[0].attn, _model(c["cfg"], c["w"], True).transformer.h[0].attn
    x = rnd(B, T, C, seed=4).to(DEV)
    outs = {}
    for tag, mod, mask in (("ar", ar, None), ("enc", enc, RangeMask.causal(B, T, DEV)), ("none", enc, None)):
        xi = x.clone().requires_grad_(True)
        y = mod(xi, attn_mask=mask)
        y.float().square().sum().backward()
        outs[tag] = (y.detach(), xi.grad.clone())
    torch.cuda.synchronize()
    assert lib().obte_device_status(0) == 0
    assert torch.equal(outs["ar"][0], outs["enc"][0]) and torch.equal(outs["ar"][1], outs["enc"][1])
    assert not torch.equal(outs["ar"][0], outs["none"][0])
