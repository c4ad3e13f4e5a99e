"""Autoregressive generation on the GPU: the key/value cache, attention for one query per sequence (obte_attn_decode) under every
split count, the prefill and decode forms of the block, and OmniBioTA.prefill / decode_step / generate — against the CPU oracle
(oracle/omnibiote_ref.py, fp32) at the project's bars for the same quantities: attention forward 2^-7 |ref| + 6e-3, lse atol 2e-3 /
rtol 1e-3, block forward atol 3e-2 / rtol 2^-6, model logits max <= 5e-3 / mean <= 1e-3 (tests/test_hip_causal.py)."""
import numpy as np
import pytest
import torch

import omnibiote_ref as R
from test_hip_causal import _add, _model, _tril
from test_hip_ops import BF, DEV, _attn_case, close, rnd

pytestmark = pytest.mark.gpu

NAMES = ["ln_1.weight", "attn.c_attn.weight", "attn.c_proj.weight", "ln_2.weight", "mlp.c_fc.weight", "mlp.c_proj.weight"]


def ops():
    from omnibiote_amd import ops as o
    return o


def L():
    from omnibiote_amd import _lib
    return _lib


def _views(cache, B, H, T_max, hs):
    """(K, V) views [B, H, T_max, hs] of a layer's cache"""
    kv = cache.view(2, B, H, T_max, hs)
    return kv[0], kv[1]


def _thirds(qkv, B, t, H, hs):
    """the k and v thirds of a packed [B, t, 3C] activation as [B, H, t, hs]"""
    C = H * hs
    k, v = qkv[..., C:2 * C], qkv[..., 2 * C:]
    return [z.reshape(B, t, H, hs).transpose(1, 2) for z in (k, v)]


# =================================================================================================== the cache
@pytest.mark.parametrize("hs", [64, 128])
def test_kv_cache_store_is_exact_and_touches_nothing_else(hs):
    o = ops()
    B, H, T_max = 2, 2, 77
    C = H * hs
    marker = 0x1234
    cache = o.kv_cache_buffer(B, T_max, H, hs, DEV)
    cache.view(torch.int16).fill_(marker)
    prompt = rnd(B, 33, 3 * C, seed=hs).to(DEV)
    step = rnd(B, 1, 3 * C, seed=hs + 1).to(DEV)
    o.kv_cache_store(prompt, B, 33, H, hs, cache, T_max, 0)
    o.kv_cache_store(step, B, 1, H, hs, cache, T_max, 33)
    K, V = _views(cache, B, H, T_max, hs)
    for got, want_p, want_s in zip((K, V), _thirds(prompt, B, 33, H, hs), _thirds(step, B, 1, H, hs)):
        assert torch.equal(got[:, :, :33].view(torch.int16), want_p.contiguous().view(torch.int16))
        assert torch.equal(got[:, :, 33:34].view(torch.int16), want_s.contiguous().view(torch.int16))
        assert (got[:, :, 34:].view(torch.int16) == marker).all()


# =================================================================================================== one-query attention
_att = {}


def _decode_case(B, H, hs, T_max):
    """qkv of T_max positions, the cache holding all of them, and the query / oracle pieces per n_keys (computed once, never modified)"""
    key = (B, H, hs, T_max)
    if key not in _att:
        o = ops()
        qkv, q, k, v = _attn_case(B, T_max, H, hs, seed=hs + T_max)
        cache = o.kv_cache_buffer(B, T_max, H, hs, DEV)
        o.kv_cache_store(qkv.to(DEV), B, T_max, H, hs, cache, T_max, 0)
        _att[key] = dict(qkv=qkv, q=q, k=k, v=v, cache=cache, ref={})
    return _att[key]


def _oracle(c, n, scale):
    """o (B, C) and lse (B, H) of the query at position n - 1 over keys [0, n): the last row of the causal case of length n"""
    if n not in c["ref"]:
        q, k, v = c["q"][:, :, n - 1:n], c["k"][:, :, :n], c["v"][:, :, :n]
        B, H = q.shape[:2]
        out = R.attention(q, k, v, scale).transpose(1, 2).reshape(B, -1)
        lse = torch.logsumexp((q @ k.transpose(-2, -1)) * scale, dim=-1).reshape(B, H)
        c["ref"][n] = (out, lse)
    return c["ref"][n]


@pytest.mark.parametrize("hs", [64, 128])
@pytest.mark.parametrize("n_keys", [1, 2, 63, 64, 65, 257, 600, 1100])
def test_attn_decode_against_the_oracle(hs, n_keys):
    """Every split count: the library's own, 1, and forced counts that leave splits empty at the small n_keys (a split owns a multiple
    of 64 keys).  The query read in place from a packed row (q_ld = 3C) and from a dense [B, C] give the same bytes."""
    o = ops()
    B, H, T_max = 2, 2, 1100
    C = H * hs
    scale = 8.0 / C
    c = _decode_case(B, H, hs, T_max)
    ref_o, ref_lse = _oracle(c, n_keys, scale)
    packed = c["qkv"][:, n_keys - 1].contiguous().to(DEV)       # [B, 3C]: the packed row of the new position
    dense = packed[:, :C].contiguous()
    for splits in (0, 1, 2, 7, L().ATTN_DECODE_MAX_SPLITS):
        got, lse = o.attn_decode(packed, c["cache"], B, T_max, n_keys, H, hs, scale, splits=splits)
        close(got, ref_o, atol=6e-3, what=f"attn_decode hs={hs} n_keys={n_keys} splits={splits}")
        close(lse, ref_lse, atol=2e-3, rtol=1e-3, what=f"lse hs={hs} n_keys={n_keys} splits={splits}")
        got_c, lse_c = o.attn_decode(dense, c["cache"], B, T_max, n_keys, H, hs, scale, splits=splits)
        assert torch.equal(got, got_c) and torch.equal(lse, lse_c)


def test_attn_decode_one_sequence_one_head():
    o = ops()
    B, H, hs, T_max, n_keys = 1, 1, 128, 300, 300
    scale = 8.0 / (H * hs)
    c = _decode_case(B, H, hs, T_max)
    ref_o, ref_lse = _oracle(c, n_keys, scale)
    for splits in (0, 1, 7):
        got, lse = o.attn_decode(c["qkv"][:, n_keys - 1].contiguous().to(DEV), c["cache"], B, T_max, n_keys, H, hs, scale, splits=splits)
        close(got, ref_o, atol=6e-3, what=f"B=H=1 splits={splits}")
        close(lse, ref_lse, atol=2e-3, rtol=1e-3, what="lse")


@pytest.mark.parametrize("splits", [1, 7])
def test_attn_decode_is_bitwise_repeatable(splits):
    o = ops()
    B, H, hs, T_max = 2, 2, 128, 1100
    c = _decode_case(B, H, hs, T_max)
    q = c["qkv"][:, 999].contiguous().to(DEV)
    a = o.attn_decode(q, c["cache"], B, T_max, 1000, H, hs, 8.0 / 256, splits=splits)
    b = o.attn_decode(q, c["cache"], B, T_max, 1000, H, hs, 8.0 / 256, splits=splits)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


@pytest.mark.parametrize("hs", [64, 128])
@pytest.mark.parametrize("n_keys", [1, 65, 300])
def test_attn_decode_never_reads_the_tail_into_the_result(hs, n_keys):
    """positions >= n_keys of K and V hold zeros, then the bf16 NaN pattern 0x7FC0: finite and bitwise the same result"""
    o = ops()
    B, H, T_max = 2, 2, 384
    C = H * hs
    qkv = rnd(B, T_max, 3 * C, seed=hs + n_keys).to(DEV)
    q = qkv[:, n_keys - 1].contiguous()
    cache = o.kv_cache_buffer(B, T_max, H, hs, DEV)
    o.kv_cache_store(qkv, B, T_max, H, hs, cache, T_max, 0)
    for splits in (0, 1, 7):
        res = []
        for pattern in (0, 0x7FC0):
            cache.view(torch.int16).view(2, B, H, T_max, hs)[:, :, :, n_keys:] = pattern
            if pattern and n_keys < T_max:
                assert torch.isnan(cache.view(2, B, H, T_max, hs)[:, :, :, n_keys:]).all()
            res.append(o.attn_decode(q, cache, B, T_max, n_keys, H, hs, 8.0 / C, splits=splits))
        for a, b in zip(*res):
            assert torch.isfinite(a).all() and torch.isfinite(b).all()
            assert torch.equal(a, b)


def test_attn_decode_peaked_softmax_across_splits():
    """n_keys = 600 under 7 forced splits (128 keys each: five hold keys, two are empty).  One key of the last split that holds keys is
    aligned with q so that its scaled score exceeds every other by more than 40, and q is scaled so that the others span +-30: the
    partials of the other splits carry weights of e^-40 and below against a maximum they never saw."""
    o = ops()
    B, H, hs, n_keys, T_max, star = 2, 2, 128, 600, 600, 590
    C = H * hs
    scale = 8.0 / C
    qkv = rnd(B, T_max, 3 * C, seed=5)
    q = qkv[:, -1, :C].reshape(B, H, hs).float()
    k = qkv[:, :, C:2 * C].reshape(B, T_max, H, hs).transpose(1, 2).float()
    others = torch.einsum("bhd,bhtd->bht", q, k) * scale
    q = (q * (30.0 / others.abs().amax(dim=-1, keepdim=True))).to(BF)            # the other scores now span +-30 (per (b, h))
    qf = q.float()
    kstar = (qf * ((30.0 + 50.0) / (scale * qf.square().sum(-1, keepdim=True)))).to(BF)   # q . k* scale = 80
    qkv[:, -1, :C] = q.reshape(B, C)
    qkv[:, star, C:2 * C] = kstar.reshape(B, C)
    qq = qkv[:, -1:, :C].reshape(B, 1, H, hs).transpose(1, 2).float()
    kk = qkv[:, :, C:2 * C].reshape(B, T_max, H, hs).transpose(1, 2).float()
    vv = qkv[:, :, 2 * C:].reshape(B, T_max, H, hs).transpose(1, 2).float()
    s = (qq @ kk.transpose(-2, -1)).squeeze(2) * scale                            # [B, H, T]
    rest = torch.cat([s[..., :star], s[..., star + 1:]], dim=-1)
    assert (s[..., star] - rest.amax(dim=-1) > 40).all() and (rest.abs().amax(dim=-1) > 25).all() and (rest.abs().amax(dim=-1) < 35).all()
    ref = R.attention(qq, kk, vv, scale).transpose(1, 2).reshape(B, C)
    ref_lse = torch.logsumexp(s, dim=-1)
    assert torch.isfinite(ref).all() and torch.isfinite(ref_lse).all() and ref_lse.abs().max() < 100     # far inside fp32
    cache = o.kv_cache_buffer(B, T_max, H, hs, DEV)
    o.kv_cache_store(qkv.to(DEV), B, T_max, H, hs, cache, T_max, 0)
    for splits in (7, 0, 1):
        got, lse = o.attn_decode(qkv[:, -1].contiguous().to(DEV), cache, B, T_max, n_keys, H, hs, scale, splits=splits)
        close(got, ref, atol=6e-3, what=f"peaked softmax, splits={splits}")
        close(lse, ref_lse, atol=2e-3, rtol=1e-3, what=f"peaked lse, splits={splits}")


# =================================================================================================== block
def _block_setup(C, H, T):
    from omnibiote_amd.masks import RangeMask
    from omnibiote_amd.model import rope_tables
    o = ops()
    B = 2
    cfg = R.RefConfig(block_size=T, vocab_size=256, n_layer=1, n_head=H, n_embd=C)
    w = {k: v.to(BF) for k, v in R.hash_weights(cfg).items()}
    pre = "transformer.h.0."
    tab = R.cast_rope_table(R.rope_table(C // H, T), BF)
    params = tuple(w[pre + n].to(DEV) for n in NAMES)
    rope = rope_tables(tab.to(DEV))
    x = rnd(B, T, C, seed=1)
    return dict(o=o, B=B, cfg=cfg, w=w, pre=pre, tab=tab, params=params, rope=rope, x=x,
                causal=lambda t: o.MaskSpec.from_user(RangeMask.causal(B, t, DEV), B, t, H, DEV))


@pytest.mark.parametrize("C,H", [(128, 2), (256, 2)])
def test_block_prefill_is_block_infer_and_leaves_the_cache(C, H):
    T, T_max = 130, 160
    c = _block_setup(C, H, T)
    o, B, hs = c["o"], c["B"], C // H
    x = c["x"].to(DEV)
    spec = c["causal"](T)
    want = o.block_infer(x, c["params"], c["rope"], H, spec)
    cache = o.kv_cache_buffer(B, T_max, H, hs, DEV)
    cache.view(torch.int16).fill_(0x1234)
    got = o.block_prefill(x, c["params"], c["rope"], H, spec, cache, T_max)
    assert torch.equal(got, want)
    h1, _, _ = o.layernorm_fwd(x, c["params"][0])
    qkv = o.gemm(h1.view(B * T, C), c["params"][1], B * T, 3 * C, C, epilogue=L().EPI_ROPE_QK, rope=(c["rope"][0], c["rope"][1], T, hs))
    mine = o.kv_cache_buffer(B, T_max, H, hs, DEV)
    mine.view(torch.int16).fill_(0x1234)
    o.kv_cache_store(qkv, B, T, H, hs, mine, T_max, 0)
    assert torch.equal(cache.view(torch.int16), mine.view(torch.int16))
    assert not (_views(cache, B, H, T_max, hs)[0][:, :, :T].view(torch.int16) == 0x1234).all()


@pytest.mark.parametrize("C,H", [(128, 2), (256, 2)])
def test_block_decode_step_by_step_vs_oracle(C, H):
    """prefill x[:, :130], then positions 130 .. 159 one at a time: each against the oracle's causal block forward of the whole x at
    that row (the block bar), and within twice that bar of block_infer's row (both sides are within one bar of the oracle)."""
    T0, T = 130, 160
    c = _block_setup(C, H, T)
    o, B, hs = c["o"], c["B"], C // H
    xf = c["x"].float()
    ref = R.block_forward(xf, {k: v.float() for k, v in c["w"].items()}, c["pre"], c["cfg"], c["tab"], _add(_tril(T)))
    x = c["x"].to(DEV)
    full = o.block_infer(x, c["params"], c["rope"], H, c["causal"](T))
    cache = o.kv_cache_buffer(B, T, H, hs, DEV)
    y0 = o.block_prefill(x[:, :T0].contiguous(), c["params"], c["rope"], H, c["causal"](T0), cache, T)
    close(y0, ref[:, :T0], atol=3e-2, rtol=2.0 ** -6, what="block prefill")
    ws = o.block_decode_workspace(B, C, H, DEV)
    worst = 0.0
    for t in range(T0, T):
        xt = x[:, t].contiguous()
        yt = o.block_decode(xt, c["params"], c["rope"], H, cache, T, t, ws=ws)
        close(yt, ref[:, t], atol=3e-2, rtol=2.0 ** -6, what=f"block decode, position {t}")
        d = (yt.float() - full[:, t].float()).abs()
        assert (d <= 2 * (3e-2 + 2.0 ** -6 * full[:, t].float().abs())).all()
        worst = max(worst, d.max().item())
        if t == T0:                                   # y may alias x
            assert torch.equal(o.block_decode(xt, c["params"], c["rope"], H, cache, T, t, ws=ws, out=xt), yt)
    print(f"block_decode vs block_infer rows, C={C}: largest distance {worst:.4g}")


# =================================================================================================== model
_models = {}


def _gen_case(C):
    """config {block 200, vocab 512, 2 layers, 2 heads, n_embd C}: the model, tokens and the oracle's causal logits (computed once)"""
    if C not in _models:
        cfg = R.RefConfig(block_size=200, vocab_size=512, n_layer=2, n_head=2, n_embd=C)
        w = R.hash_weights(cfg)
        B, T = 2, 199
        ids = torch.from_numpy(np.random.default_rng(C).integers(4, cfg.vocab_size, size=(B, T)).astype(np.int64))
        wb = {k: v.to(BF).float() for k, v in w.items()}
        rope = R.cast_rope_table(R.rope_table(cfg.n_embd // cfg.n_head, T), BF)
        with torch.no_grad():
            logits = R.model_forward(wb, cfg, ids, _add(_tril(T)), rope=rope)
        _models[C] = dict(cfg=cfg, m=_model(cfg, w, True), ids=ids, logits=logits)
    return _models[C]


@pytest.mark.parametrize("C", [256, 128])
def test_teacher_forced_decode_matches_the_oracle(C):
    from omnibiote_amd.model import KVCache
    c = _gen_case(C)
    m, idx = c["m"], c["ids"].to(DEV)
    cache = KVCache(m, 2)
    assert cache.max_len == 200
    got = [m.prefill(idx[:, :130], cache)]                        # the logits of position 129
    for t in range(130, 199):
        assert cache.pos == t
        got.append(m.decode_step(idx[:, t], cache))               # the logits of position t
    got = torch.stack(got, dim=1).float().cpu()                   # positions 129 .. 198
    d = (got - c["logits"][:, 129:199]).abs()
    assert torch.isfinite(got).all()
    assert d.max().item() <= 5e-3 and d.mean().item() <= 1e-3, (d.max().item(), d.mean().item())
    with pytest.raises(ValueError, match="batch"):
        m.decode_step(idx[:1, 0], cache)
    with pytest.raises(ValueError, match="batch"):
        m.prefill(idx[:1, :10], cache)


def test_generate_greedy_follows_the_full_forward():
    """top_k = 1, 40 new tokens from a 130-token prompt.  In ONE causal forward over the finished sequence the logit of every generated
    token lies within 2e-2 of its position's maximum: the decode path and the full forward are each within 5e-3 of the oracle, hence
    within 1e-2 of each other, and an argmax taken on one side can lose at most twice that on the other."""
    c = _gen_case(256)
    m, idx = c["m"], c["ids"][:, :130].to(DEV)
    out = m.generate(idx, 40, top_k=1)
    assert out.shape == (2, 170) and out.dtype == torch.int64
    assert torch.equal(out[:, :130], idx)
    with torch.no_grad():
        logits = m(out).float()
    at = logits[:, 129:169]                                        # position t predicts token t + 1
    chosen = at.gather(-1, out[:, 130:].unsqueeze(-1)).squeeze(-1)
    gap = at.max(dim=-1).values - chosen
    print(f"greedy generate: largest logit gap to the full forward's maximum {gap.max().item():.4g}")
    assert (gap <= 2e-2).all(), gap.max().item()
    from omnibiote_amd import train_encoder as TE
    was = m.training
    TE.set_dropout(m, 0.1)                                         # dropout never applies on the generation path
    m.train()
    try:
        assert torch.equal(m.generate(idx, 40, top_k=1), out)
    finally:
        TE.set_dropout(m, 0.0)
        m.train(was)


def test_generate_sampled_is_seeded_and_eos_stops_it():
    c = _gen_case(256)
    m, idx = c["m"], c["ids"][:, :130].to(DEV)
    a = m.generate(idx, 20, temperature=0.9, top_k=50, generator=torch.Generator(device=DEV).manual_seed(11))
    b = m.generate(idx, 20, temperature=0.9, top_k=50, generator=torch.Generator(device=DEV).manual_seed(11))
    assert a.shape == (2, 150) and torch.equal(a, b) and torch.equal(a[:, :130], idx)
    first = m.generate(idx, 1, top_k=1)[:, -1]                    # the first step's argmax of every row
    eos = int(first[0])
    out = m.generate(idx, 20, top_k=1, eos_token=eos)
    gen = out[:, 130:]
    assert int(gen[0, 0]) == eos                                   # row 0 finishes at its first token
    ends = []
    for r in range(2):
        hit = (gen[r] == eos).nonzero().flatten()
        if hit.numel():
            assert (gen[r, int(hit[0]):] == eos).all()             # a finished row keeps producing it
            ends.append(int(hit[0]))
    # returned early: right after the step at which the last row finished, else all 20 tokens
    assert gen.shape[1] == (max(ends) + 1 if len(ends) == 2 else 20)
    one = m.generate(idx[:1], 20, top_k=1, eos_token=eos)         # the one row whose first token is eos: a single step
    assert one.shape == (1, 131) and int(one[0, -1]) == eos


def test_cache_reuse_ignores_stale_positions():
    from omnibiote_amd.model import KVCache
    c = _gen_case(256)
    m, idx = c["m"], c["ids"].to(DEV)
    used = KVCache(m, 2)
    m.prefill(idx[:, :150], used)
    for t in range(150, 160):
        m.decode_step(idx[:, t], used)
    fresh = KVCache(m, 2)
    for layer in fresh.layers:
        layer.view(torch.int16).fill_(0x7FC0)                      # NaN everywhere it has not written
    res = []
    for cache in (used, fresh):
        a = m.prefill(idx[:, 60:100].contiguous(), cache)
        assert cache.pos == 40
        res.append((a, m.decode_step(idx[:, 100], cache)))
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])
    assert torch.isfinite(res[0][1]).all()
