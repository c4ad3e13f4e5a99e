"""Attention maps on the GPU: ops.attn_probs / OmniBioTA.attention_maps against the rule in torch (omnibiote_amd/attnmaps.py).

The yardstick is the float64 rule on the same bf16 qkv.  The bound of a case is not a constant: the test evaluates the fp32 rule on the
CPU and allows 16 x its worst relative error against float64 (the factor covers the MFMA's summation order and the hardware exp2, which
differ from the CPU's), with atol = 1e-30 for weights that underflow; a case whose bound comes out above 2^-12 fails as inconclusive.
References are computed once per case, shared, and never modified.  Every test prints its figures before it asserts."""
import ctypes as C

import numpy as np
import pytest
import torch

import fenced as F
import omnibiote_ref as R
from omnibiote_amd.attnmaps import attention_probs_reference, head_mean
from test_hip_ops import close

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF = torch.bfloat16
ATOL = 1e-30
FACTOR = 16.0
INCONCLUSIVE = 2.0 ** -12
MODES = ["none", "ranges", "dense", "causal"]


def ops():
    from omnibiote_amd import ops as o
    return o


def L():
    from omnibiote_amd import _lib
    return _lib


def _qkv(B, T, H, hs, seed, gain=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(B, T, 3 * H * hs, generator=g) * gain).to(BF)


def _doc(B, T):
    """the masks of tests/test_hip_ops.py::test_attention_fwd_bwd: dense additive (B, T, T) fp32 and key ranges (B, T, 2) int32"""
    rng = np.random.default_rng(T)
    tokens = rng.integers(20, 100, size=(B, T))
    tokens[0, [T // 3, T // 2]] = R.EOS_TOKEN
    tokens[1, [5, T - 10]] = R.EOS_TOKEN
    blocks = R.document_blocks(tokens)
    return R.dense_mask_from_blocks(blocks, T), torch.from_numpy(R.key_ranges_from_blocks(blocks, T))


def _causal_ranges(B, T):
    r = torch.zeros(B, T, 2, dtype=torch.int32)
    r[:, :, 1] = torch.arange(1, T + 1, dtype=torch.int32)
    return r


def _pad_mask(B, T, pad):
    """the reference's pad_attn: rows and columns beyond the pad position carry -1e9"""
    allowed = torch.zeros(T, T, dtype=torch.bool)
    allowed[:pad, :pad] = True
    return torch.where(allowed, 0.0, R.MASKED_VALUE).expand(B, T, T).contiguous()


def _dense_spec(dense, B, H, T):
    return ops().MaskSpec.from_user(dense.to(BF).to(DEV).unsqueeze(1).expand(B, H, T, T), B, T, H, DEV)


def _mask(mode, B, H, T):
    """(the MaskSpec of the call, the rule's keyword arguments, the (B, T, T) bool map of included keys)"""
    o = ops()
    if mode == "none":
        return None, {}, torch.ones(B, T, T, dtype=torch.bool)
    if mode == "causal":
        from omnibiote_amd.masks import RangeMask
        return o.MaskSpec.from_user(RangeMask.causal(B, T, DEV), B, T, H, DEV), dict(key_ranges=_causal_ranges(B, T)), \
            torch.tril(torch.ones(T, T, dtype=torch.bool)).expand(B, T, T)
    dense, ranges = _doc(B, T)
    if mode == "ranges":
        return o.MaskSpec(ranges=ranges.to(DEV)), dict(key_ranges=ranges), dense == 0
    return _dense_spec(dense, B, H, T), dict(mask_add=dense.unsqueeze(1)), dense == 0


_refs = {}


def _case(mode, hs, T, B=2, H=2, gain=1.0):
    """qkv, the float64 rule, the bound's rtol and the included-key map of a case: computed once, shared, never modified"""
    key = (mode, hs, T, B, H, gain)
    if key not in _refs:
        qkv = _qkv(B, T, H, hs, seed=hs + T, gain=gain)
        scale = 8.0 / (H * hs)
        _, kw, inc = _mask(mode, B, H, T)
        p64 = attention_probs_reference(qkv, H, scale, **kw)
        p32 = attention_probs_reference(qkv, H, scale, dtype=torch.float32, **kw)
        big = p64 > ATOL
        rel = ((p32.double() - p64).abs()[big] / p64[big]).max().item()
        _refs[key] = dict(qkv=qkv, scale=scale, p64=p64, rel32=rel, rtol=FACTOR * rel, inc=inc)
    return _refs[key]


def _conclusive(c, what):
    print(f"PROBS_BOUND {what}: fp32 rule rel err {c['rel32']:.3e}, rtol {c['rtol']:.3e}")
    if not c["rtol"] <= INCONCLUSIVE:
        pytest.fail(f"{what}: inconclusive, the bound 16 x {c['rel32']:.3e} is above 2^-12")


def _within(got, p64, rtol, what):
    got = got.detach().double().cpu()
    assert got.shape == p64.shape, (got.shape, p64.shape)
    assert torch.isfinite(got).all(), f"{what}: non-finite weights"
    err = (got - p64).abs()
    big = p64 > ATOL
    worst = (err[big] / p64[big]).max().item() if big.any() else 0.0
    print(f"PROBS_ERR {what}: max rel err {worst:.3e} (rtol {rtol:.3e}), max abs err {err.max().item():.3e}")
    bad = err > rtol * p64 + ATOL
    assert not bad.any(), f"{what}: {int(bad.sum())}/{bad.numel()} off, max rel err {worst:.3e} > rtol {rtol:.3e}"


def _run(c, mode, hs, T, B=2, H=2, **kw):
    spec, _, _ = _mask(mode, B, H, T)
    return ops().attn_probs(c["qkv"].to(DEV), B, T, H, hs, c["scale"], spec, **kw)


# ---- 1. parity with the rule ----------------------------------------------------------------------------------------------------------
def _parity(mode, hs, T, gain, what):
    B, H = 2, 2
    c = _case(mode, hs, T, gain=gain)
    _conclusive(c, what)
    got = _run(c, mode, hs, T)
    assert got.dtype == torch.float32 and tuple(got.shape) == (B, H, T, T)
    _within(got, c["p64"], c["rtol"], what)
    g = got.cpu()
    out = ~c["inc"].unsqueeze(1).expand(B, H, T, T)
    assert torch.equal(g[out], torch.zeros_like(g[out])), f"{what}: an excluded key has a non-zero weight"
    sums = g.double().sum(-1)
    dev = (sums - 1.0).abs().max().item()
    print(f"PROBS_ROWSUM {what}: max |sum - 1| {dev:.3e}")
    assert dev <= c["rtol"] + T * 2.0 ** -24


@pytest.mark.parametrize("hs", [64, 128])
@pytest.mark.parametrize("T", [64, 77, 130, 256])
@pytest.mark.parametrize("mode", MODES)
def test_weights_match_the_float64_rule(hs, T, mode):
    _parity(mode, hs, T, 1.0, f"{mode} hs={hs} T={T}")


@pytest.mark.parametrize("mode", MODES)
def test_peaked_weights_match_the_float64_rule(mode):
    """inputs scaled by 4: scores reach about +-28, weights about 1e-19"""
    _parity(mode, 128, 130, 4.0, f"peaked {mode} hs=128 T=130")


# ---- 2. dense against ranges ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hs,T", [(64, 77), (128, 130), (64, 256)])
def test_dense_and_range_forms_of_one_mask_agree(hs, T):
    c = _case("ranges", hs, T)
    _conclusive(c, f"dense vs ranges hs={hs} T={T}")
    a = _run(c, "ranges", hs, T).cpu()
    b = _run(c, "dense", hs, T).cpu()
    d = (a.double() - b.double()).abs()
    print(f"PROBS_FORMS hs={hs} T={T}: max |ranges - dense| {d.max().item():.3e}")
    assert not (d > c["rtol"] * c["p64"] + ATOL).any()
    assert torch.equal(a == 0, b == 0)


# ---- 3. key-padding dense mask --------------------------------------------------------------------------------------------------------
def _pad_case(hs, T, pad, B=2, H=2):
    key = ("pad", hs, T, pad, B, H)
    if key not in _refs:
        qkv = _qkv(B, T, H, hs, seed=3 * hs + T)
        scale = 8.0 / (H * hs)
        dense = _pad_mask(B, T, pad)
        p64 = attention_probs_reference(qkv, H, scale, mask_add=dense.unsqueeze(1))
        p32 = attention_probs_reference(qkv, H, scale, mask_add=dense.unsqueeze(1), dtype=torch.float32)
        live64, live32 = p64[:, :, :pad], p32[:, :, :pad].double()
        big = live64 > ATOL
        rel = ((live32 - live64).abs()[big] / live64[big]).max().item()
        _refs[key] = dict(qkv=qkv, scale=scale, dense=dense, p64=p64, p32=p32, rel32=rel, rtol=FACTOR * rel)
    return _refs[key]


@pytest.mark.parametrize("bounds", [True, False])
@pytest.mark.parametrize("hs,T,pad", [(64, 77, 50), (128, 130, 97)])
def test_key_padding_mask_padded_queries_are_uniform(hs, T, pad, bounds):
    """bounds: the mask through MaskSpec.from_user (obte_mask_bounds' tables beside it) or the dense tensor alone"""
    B, H = 2, 2
    c = _pad_case(hs, T, pad)
    _conclusive(c, f"key padding hs={hs} T={T}")
    o = ops()
    spec = _dense_spec(c["dense"], B, H, T) if bounds else o.MaskSpec(dense=c["dense"].to(BF).to(DEV).unsqueeze(1).expand(B, H, T, T))
    got = o.attn_probs(c["qkv"].to(DEV), B, T, H, hs, c["scale"], spec).cpu()
    assert torch.isfinite(got).all()
    padded = got[:, :, pad:].double()
    dev = (padded - 1.0 / T).abs().max().item()
    print(f"PROBS_PAD hs={hs} T={T} bounds={bounds}: padded rows max |w - 1/T| {dev:.3e}")
    assert dev <= c["rtol"] / T + ATOL
    assert torch.equal(c["p32"][:, :, pad:], torch.full((B, H, T - pad, T), 1.0 / T, dtype=torch.float32))   # the fp32 rule itself
    _within(got[:, :, :pad], c["p64"][:, :, :pad], c["rtol"], f"key padding hs={hs} T={T} bounds={bounds}, live rows")
    assert torch.equal(got[:, :, :pad, pad:], torch.zeros(B, H, pad, T - pad))


# ---- 4. empty ranges ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hs,T", [(64, 77), (128, 130)])
def test_an_empty_key_range_gives_a_row_of_zeros_and_moves_nothing_else(hs, T):
    B, H = 2, 2
    c = _case("ranges", hs, T)
    o = ops()
    _, ranges = _doc(B, T)
    q = T // 2 + 3
    edited = ranges.clone()
    edited[1, q] = torch.tensor([9, 9], dtype=torch.int32)
    qkv = c["qkv"].to(DEV)
    plain = o.attn_probs(qkv, B, T, H, hs, c["scale"], o.MaskSpec(ranges=ranges.to(DEV))).cpu()
    got = o.attn_probs(qkv, B, T, H, hs, c["scale"], o.MaskSpec(ranges=edited.to(DEV))).cpu()
    assert torch.isfinite(got).all()
    assert torch.equal(got[1, :, q], torch.zeros(H, T))
    keep = torch.ones(B, H, T, dtype=torch.bool)
    keep[1, :, q] = False
    F.assert_same_bits(got[keep], plain[keep], "rows beside the empty one")


# ---- 5. consistency with the forward ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hs", [64, 128])
@pytest.mark.parametrize("mode", MODES + ["empty", "pad", "pad_alone"])
def test_weights_times_v_is_the_forwards_output(hs, mode):
    """P @ v formed in fp32 on the host from the fp32 per-head maps against ops.attn_fwd's o on the same operands and MaskSpec, at the
    attention forward's own tolerance — rows with nothing to attend to (an empty range, padded queries) included"""
    B, H, T = 2, 2, 130
    C = H * hs
    o = ops()
    qkv = _qkv(B, T, H, hs, seed=hs + T)
    scale = 8.0 / C
    if mode == "empty":
        _, ranges = _doc(B, T)
        ranges = ranges.clone()
        ranges[1, T // 2 + 3] = torch.tensor([9, 9], dtype=torch.int32)
        spec = o.MaskSpec(ranges=ranges.to(DEV))
    elif mode == "pad":
        spec = _dense_spec(_pad_mask(B, T, 97), B, H, T)
    elif mode == "pad_alone":
        spec = o.MaskSpec(dense=_pad_mask(B, T, 97).to(BF).to(DEV).unsqueeze(1).expand(B, H, T, T))
    else:
        spec = _mask(mode, B, H, T)[0]
    P = o.attn_probs(qkv.to(DEV), B, T, H, hs, scale, spec).cpu()
    out, _ = o.attn_fwd(qkv.to(DEV), B, T, H, hs, scale, spec)
    v = qkv.float()[..., 2 * C:].reshape(B, T, H, hs).transpose(1, 2)
    pv = (P @ v).transpose(1, 2).reshape(B, T, C)
    print(f"PROBS_FWD {mode} hs={hs}: max |P v - o| {(pv - out.float().cpu()).abs().max().item():.3e}")
    close(out, pv, atol=6e-3, what=f"P v against attn_fwd, {mode} hs={hs}")


# ---- 6. head mean ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["none", "ranges", "dense"])
def test_head_mean_is_the_fp32_mean_of_the_heads(mode):
    B, H, hs, T = 2, 3, 64, 130
    c = _case(mode, hs, T, B=B, H=H)
    _conclusive(c, f"head mean {mode}")
    per_head = _run(c, mode, hs, T, B=B, H=H).cpu()
    mean = _run(c, mode, hs, T, B=B, H=H, heads="mean").cpu()
    assert mean.dtype == torch.float32 and tuple(mean.shape) == (B, T, T)
    d = (mean - head_mean(per_head)).abs().max().item()
    print(f"PROBS_MEAN {mode}: max |mean - mean of heads| {d:.3e}")
    assert d <= H * 2.0 ** -23
    _within(mean, c["p64"].mean(dim=1), c["rtol"], f"head mean {mode} against the float64 rule")


# ---- 7. bf16 output -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("heads", ["all", "mean"])
@pytest.mark.parametrize("mode,hs,T", [("ranges", 64, 77), ("dense", 128, 130)])
def test_bf16_output_is_the_rounded_fp32_output(mode, hs, T, heads):
    c = _case(mode, hs, T)
    f32 = _run(c, mode, hs, T, heads=heads)
    b16 = _run(c, mode, hs, T, heads=heads, dtype=BF)
    assert b16.dtype == BF and torch.equal(b16, f32.to(BF))


# ---- 8. same bits twice ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("heads", ["all", "mean"])
@pytest.mark.parametrize("mode,hs,T", [("causal", 64, 256), ("dense", 128, 130)])
def test_two_calls_give_the_same_bits(mode, hs, T, heads):
    c = _case(mode, hs, T)
    F.assert_same_bits(_run(c, mode, hs, T, heads=heads), _run(c, mode, hs, T, heads=heads), f"{mode} {heads}")


# ---- 9. guard bands -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hs", [64, 128])
@pytest.mark.parametrize("mode", ["ranges", "dense"])
@pytest.mark.parametrize("heads,dtype", [("all", torch.float32), ("mean", torch.bfloat16)])
def test_guard_bands_stay_untouched_at_16_byte_alignment(hs, mode, heads, dtype):
    """qkv, out (batch stride larger than the payload) and the workspace inside poisoned buffers, 16-byte aligned and no more"""
    B, H, T = 2, 2, 77
    o = ops()
    c = _case(mode, hs, T)
    spec = _mask(mode, B, H, T)[0]
    plain = o.attn_probs(c["qkv"].to(DEV), B, T, H, hs, c["scale"], spec, heads=heads, dtype=dtype)
    qkv, hq = F.fenced(c["qkv"].to(DEV), poison="nan")
    payload = (T * T) if heads == "mean" else (H * T * T)
    flat, ho = F.fenced((B, payload), dtype, poison="mark", ld=payload + 40)
    out = flat.unflatten(1, (T, T) if heads == "mean" else (H, T, T))
    ws, hw = F.fenced((int(L().lib().obte_attn_probs_ws_bytes(B, T, H)),), torch.uint8, poison="mark")
    assert qkv.data_ptr() % 512 == 16 and out.data_ptr() % 512 == 16 and ws.data_ptr() % 512 == 16 and out.stride(0) == payload + 40
    got = o.attn_probs(qkv, B, T, H, hs, c["scale"], spec, heads=heads, dtype=dtype, out=out, ws=ws)
    torch.cuda.synchronize()
    F.assert_guards(hq, ho, hw)
    F.assert_same_bits(got, plain, f"fenced {mode} hs={hs} {heads}")


# ---- 10. refusals ---------------------------------------------------------------------------------------------------------------------
def test_bad_arguments_are_refused_before_any_launch():
    B, H, T, hs = 1, 2, 64, 64
    lib = L().lib()
    qkv = torch.zeros(B, T, 3 * H * hs, dtype=BF, device=DEV)
    out = torch.full((B, H, T, T), 7.0, dtype=torch.float32, device=DEV)
    need = int(lib.obte_attn_probs_ws_bytes(B, T, H))
    assert need == 8 * B * H * T
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    stream = torch.cuda.current_stream().cuda_stream

    def call(**edit):
        kw = dict(qkv=qkv.data_ptr(), head_dim=hs, ws_bytes=need, out=out.data_ptr(), ws=ws.data_ptr())
        kw.update(edit)
        a = L().AttnProbsArgs(kw["qkv"], None, None, 0, 0, 0, None, B, T, H, kw["head_dim"], 0.0625, kw["out"], H * T * T, 0, 0, kw["ws"], kw["ws_bytes"])
        rc = lib.obte_attn_probs(C.byref(a), stream)
        return rc, (lib.obte_last_error() or b"").decode()

    for edit, word in ((dict(head_dim=32), "head_dim"), (dict(qkv=None), "qkv"), (dict(ws_bytes=need - 1), "ws_bytes"), (dict(out=None), "out"),
                       (dict(ws=None), "ws"), (dict(qkv=qkv.data_ptr() + 8), "aligned"), (dict(ws=ws.data_ptr() + 4), "aligned")):
        rc, msg = call(**edit)
        assert rc == -1 and "obte_attn_probs" in msg and word in msg, (edit, rc, msg)
    torch.cuda.synchronize()
    assert torch.equal(out, torch.full_like(out, 7.0))            # nothing was launched
    assert lib.obte_device_status(0) == 0
    assert call()[0] == 0
    with pytest.raises(RuntimeError, match="obte_attn_probs"):
        ops().attn_probs(qkv, B, T, H, hs, 0.0625, ws=ws[:-1])


# ---- 11. the model against the oracle ---------------------------------------------------------------------------------------------------
TINY = dict(block_size=64, vocab_size=512, n_layer=2, n_head=2, n_embd=128)


def _model(cfg, w, autoregressive):
    import warnings
    from omnibiote_amd.model import OmniBioTA, OmniBioTAConfig
    from omnibiote_amd.mup_compat import set_base_shapes
    c = OmniBioTAConfig()
    c.block_size, c.vocab_size, c.n_layer, c.n_head, c.n_embd, c.dropout, c.flash = cfg.block_size, cfg.vocab_size, cfg.n_layer, cfg.n_head, cfg.n_embd, 0.1, True
    c.autoregressive = autoregressive
    m = OmniBioTA(c)
    cb = OmniBioTAConfig(); cb.block_size, cb.vocab_size, cb.n_layer, cb.dropout, cb.flash = cfg.block_size, cfg.vocab_size, cfg.n_layer, 0.0, True
    cb.n_embd, cb.n_head = 24, 3
    base = OmniBioTA(cb)
    cb.n_embd, cb.n_head = 48, 12
    delta = OmniBioTA(cb)
    set_base_shapes(m, base, delta=delta, rescale_params=False)
    m.load_state_dict(w, strict=False)
    with warnings.catch_warnings():      # what the reference does: module.to(bfloat16), the RoPE buffer keeps its cosines
        warnings.simplefilter("ignore")
        m.to(BF)
    return m.to(DEV)


def _oracle_maps(monkeypatch, cfg, w, idx, mask_add, dtype):
    """the oracle's forward with its attention wrapped: the float64 softmax of every layer's recorded (q, k, scale, mask)"""
    seen = []
    inner = R.attention

    def recording(q, k, v, scale, mask=None, drop_mask=None):
        seen.append((q.detach().double(), k.detach().double(), scale, None if mask is None else mask.detach().double()))
        return inner(q, k, v, scale, mask, drop_mask)

    monkeypatch.setattr(R, "attention", recording)
    weights = {k: v.to(BF).to(dtype) for k, v in w.items()}          # the same bf16-valued weights in both modes
    rope = R.cast_rope_table(R.rope_table(cfg.n_embd // cfg.n_head, idx.shape[1]), BF)
    with torch.no_grad():
        R.model_forward(weights, cfg, idx, None if mask_add is None else mask_add.to(dtype), rope=rope, return_embeddings=True)
    monkeypatch.setattr(R, "attention", inner)
    maps = []
    for q, k, scale, mask in seen:
        s = (q @ k.transpose(-2, -1)) * scale
        maps.append(torch.softmax(s if mask is None else s + mask, dim=-1))
    assert len(maps) == cfg.n_layer
    return torch.stack(maps, dim=1)                                   # (B, layers, H, T, T)


@pytest.mark.parametrize("autoregressive", [False, True])
def test_model_maps_against_the_oracle(monkeypatch, autoregressive):
    """The tiny configuration of the model tests, as an encoder under a document mask and autoregressive.  Expected: the float64 softmax
    of what the oracle's attention receives in its fp32 run (bf16-valued weights, the bf16 module's cos-only RoPE).  The bound is
    measured on the oracle alone: 4 x the largest difference between the maps of its fp32 run and of its bf16 run, the size of bf16
    noise in the hidden states."""
    from omnibiote_amd.masks import RangeMask
    cfg = R.RefConfig(**TINY)
    w = R.hash_weights(cfg)
    B, T, H = 2, 64, cfg.n_head
    rng = np.random.default_rng(5)
    tok = rng.integers(20, cfg.vocab_size, size=(B, T))
    tok[0, [20, 41]] = R.EOS_TOKEN
    tok[1, [9, 30, 50]] = R.EOS_TOKEN
    idx = torch.from_numpy(tok)
    if autoregressive:
        mask_add = torch.where(torch.tril(torch.ones(T, T, dtype=torch.bool)), 0.0, R.MASKED_VALUE).expand(B, 1, T, T)
        user_mask = None
    else:
        mask_add = R.dense_mask_from_blocks(R.document_blocks(tok), T).unsqueeze(1)
        user_mask = RangeMask.from_tokens(idx.to(DEV))
    want = _oracle_maps(monkeypatch, cfg, w, idx, mask_add, torch.float32)
    noisy = _oracle_maps(monkeypatch, cfg, w, idx, mask_add, BF)
    noise = (want - noisy).abs().max().item()
    m = _model(cfg, w, autoregressive).train()
    m.transformer.h[1].eval()
    flags = [(mod, mod.training) for mod in m.modules()]
    got = m.attention_maps(idx.to(DEV), attn_mask=user_mask)
    assert got.dtype == torch.float32 and tuple(got.shape) == (B, cfg.n_layer, H, T, T)
    err = (got.double().cpu() - want).abs().max().item()
    print(f"PROBS_MODEL autoregressive={autoregressive}: max |maps - oracle| {err:.3e}, oracle fp32 vs bf16 {noise:.3e}")
    assert torch.isfinite(got).all() and err <= 4 * noise
    assert all(mod.training == was for mod, was in flags)
    one = m.attention_maps(idx.to(DEV), attn_mask=user_mask, layers=[1])
    F.assert_same_bits(one[:, 0], got[:, 1], "layers=[1] against slice 1 of every layer")
    mean = m.attention_maps(idx.to(DEV), attn_mask=user_mask, heads="mean")
    assert tuple(mean.shape) == (B, cfg.n_layer, T, T)
    d = (mean.cpu() - head_mean(got.cpu().flatten(0, 1)).unflatten(0, (B, cfg.n_layer))).abs().max().item()
    assert d <= H * 2.0 ** -23, d
    assert all(mod.training == was for mod, was in flags)
