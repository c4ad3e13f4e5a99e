"""The e4m3 key/value cache on the GPU (include/omnibiote_hip_kv8.h): the store kernels bit for bit against the format's yardstick
(omnibiote_amd/kvquant.py), one-query attention over it against float64 ON THE DEQUANTISED CACHE — so the quantisation error is not in
the tolerance, and the bars are the project's own for the same quantities (tests/test_hip_generate.py): attention 2^-7 |ref| + 6e-3, lse
atol 2e-3 / rtol 1e-3, block atol 3e-2 / rtol 2^-6, model logits max <= 5e-3 / mean <= 1e-3 — the prefill and decode forms of the block,
and OmniBioTA.prefill / decode_step / generate on KVCache(dtype="fp8")."""
import pytest
import torch
import torch.nn.functional as F

import omnibiote_ref as R
from fenced import assert_guards, assert_same_bits, fenced
from test_hip_causal import _add, _tril
from test_hip_generate import _block_setup, _gen_case
from test_hip_ops import BF, DEV, close, rnd

pytestmark = pytest.mark.gpu


def ops():
    from omnibiote_amd import ops as o
    return o


def L():
    from omnibiote_amd import _lib
    return _lib


def KQ():
    from omnibiote_amd import kvquant
    return kvquant


def _thirds(qkv, B, t, H, hs):
    """the k and v thirds of a packed [B, t, 3C] activation as [B, H, t, hs]"""
    C = H * hs
    return [z.reshape(B, t, H, hs).transpose(1, 2).contiguous() for z in (qkv[..., C:2 * C], qkv[..., 2 * C:])]


def _parts(cache, B, T_max, H, hs):
    """the cache on the host: (K codes, V codes, K scales, V scales)"""
    return KQ().split_cache(cache.cpu(), B, T_max, H, hs)


def _dequantized(cache, B, T_max, H, hs):
    """(K, V) float64 [B, H, T_max, hs] as a reader of the cache forms them"""
    kc, vc, ks, vs = _parts(cache, B, T_max, H, hs)
    return (kc.view(torch.float8_e4m3fn).double() * ks.double().unsqueeze(-1), vc.view(torch.float8_e4m3fn).double() * vs.double().unsqueeze(-1))


# =================================================================================================== the store
def _store_inputs(B, t, H, hs, seed):
    """packed [B, t, 3C] bf16 whose k and v head vectors have magnitudes spread over 2^+-20, with a zero vector, vectors whose maximum
    is exactly 448 * 2^j and ones a bf16 ulp above that"""
    C = H * hs
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, t, 3, H, hs, generator=g) * torch.exp2(torch.randint(-20, 21, (B, t, 3, H, 1), generator=g).float())
    x = x.to(BF)
    x[0, 0, 1, 0] = 0                                                   # a zero key vector
    x[B - 1, t - 1, 2, H - 1] = 0                                       # and a zero value vector
    for n, j in enumerate((-9, 0, 5)):
        if n + 1 >= t:
            break
        for third in (1, 2):
            v = ((torch.rand(hs, generator=g) * 2 - 1) * 2.0 ** j).to(BF)
            v[(7 * n + third) % hs] = 448.0 * 2.0 ** j
            x[0, n + 1, third, 1] = v                                   # the maximum exactly 448 * 2^j: scale 2^j
            v = v.clone()
            v[(7 * n + third) % hs] = (v[(7 * n + third) % hs].view(torch.int16) + 1).view(BF)
            x[1, n + 1, third, 0] = v                                   # one ulp above: scale 2^(j + 1)
    return x.reshape(B, t, 3 * C)


@pytest.mark.parametrize("hs", [64, 128])
def test_kv8_cache_store_is_the_reference_bit_for_bit_and_touches_nothing_else(hs):
    o = ops()
    B, H, T_max = 2, 2, 77
    cache = o.kv8_cache_buffer(B, T_max, H, hs, DEV)
    assert cache.numel() == 2 * B * H * T_max * (hs + 4) and cache.data_ptr() % 16 == 0
    cache.fill_(0x5A)
    prompt, step = _store_inputs(B, 33, H, hs, hs), _store_inputs(B, 1, H, hs, hs + 1)
    o.kv8_cache_store(prompt.to(DEV), B, 33, H, hs, cache, T_max, 0)
    o.kv8_cache_store(step.to(DEV), B, 1, H, hs, cache, T_max, 33)
    kc, vc, ks, vs = _parts(cache, B, T_max, H, hs)
    seen = set()
    for codes, scales, want_p, want_s in zip((kc, vc), (ks, vs), _thirds(prompt, B, 33, H, hs), _thirds(step, B, 1, H, hs)):
        for lo, hi, want in ((0, 33, want_p), (33, 34, want_s)):
            wc, wsc = KQ().quantize_reference(want)
            assert torch.equal(codes[:, :, lo:hi], wc), f"codes of positions [{lo}, {hi})"
            assert torch.equal(scales[:, :, lo:hi].view(torch.int32), wsc.view(torch.int32)), f"scales of positions [{lo}, {hi})"
            seen.update(wsc.flatten().tolist())
        assert bool((codes[:, :, 34:] == 0x5A).all()) and bool((scales[:, :, 34:].view(torch.int32) == 0x5A5A5A5A).all())
    assert 2.0 ** -126 in seen and {2.0 ** -9, 2.0 ** -8, 1.0, 2.0, 32.0, 64.0} <= seen and len(seen) > 30     # the planted cases were there


@pytest.mark.parametrize("hs", [64, 128])
def test_kv8_rope_store_rows_rotates_as_the_bf16_form_and_quantises(hs):
    """the rows form: qkv is left with the bits obte_kv_cache_rope_store_rows leaves, the cache holds the reference of the rotated k and
    the v at every active row's position, and a row at -1 or above max_pos is left alone entirely"""
    from omnibiote_amd.model import rope_tables
    o = ops()
    B, H, T_max, max_pos = 5, 2, 77, 40
    C = H * hs
    rope = rope_tables(R.rope_table(hs, T_max).to(DEV))
    pos = torch.tensor([5, -1, 40, 41, 0], dtype=torch.int32, device=DEV)
    qkv0 = _store_inputs(B, 1, H, hs, 3 * hs).reshape(B, 3 * C).to(DEV)
    bf = o.kv_cache_buffer(B, T_max, H, hs, DEV)
    want_qkv = o.kv_cache_rope_store_rows(qkv0.clone(), rope, pos, max_pos, B, H, hs, bf, T_max)
    cache = o.kv8_cache_buffer(B, T_max, H, hs, DEV)
    cache.fill_(0x5A)
    got_qkv = o.kv8_cache_rope_store_rows(qkv0.clone(), rope, pos, max_pos, B, H, hs, cache, T_max)
    assert torch.equal(got_qkv.view(torch.int16), want_qkv.view(torch.int16))
    assert torch.equal(got_qkv[1], qkv0[1]) and torch.equal(got_qkv[3], qkv0[3]) and not torch.equal(got_qkv[0], qkv0[0])
    kc, vc, ks, vs = _parts(cache, B, T_max, H, hs)
    untouched = torch.ones(B, H, T_max, dtype=torch.bool)
    for codes, scales, want in zip((kc, vc), (ks, vs), _thirds(want_qkv.cpu().view(B, 1, 3 * C), B, 1, H, hs)):
        wc, wsc = KQ().quantize_reference(want)
        for b, p in ((0, 5), (2, 40), (4, 0)):
            assert torch.equal(codes[b, :, p], wc[b, :, 0]) and torch.equal(scales[b, :, p].view(torch.int32), wsc[b, :, 0].view(torch.int32)), (b, p)
            untouched[b, :, p] = False
        assert bool((codes[untouched] == 0x5A).all()) and bool((scales.view(torch.int32)[untouched] == 0x5A5A5A5A).all())


# =================================================================================================== one-query attention
_att = {}


def _decode_case(B, H, hs, T_max):
    """qkv of T_max positions whose keys and values carry a per-key factor 2^[-6, 6], drawn independently for K and V — a kernel that
    drops or swaps a scale misses the bar by orders of magnitude — the e4m3 cache of all of them, the cache read back and dequantised in
    float64, and the float64 results per n_keys (computed once, never modified)"""
    key = (B, H, hs, T_max)
    if key not in _att:
        o = ops()
        C = H * hs
        g = torch.Generator().manual_seed(hs + T_max)
        x = torch.randn(B, T_max, 3, H, hs, generator=g)
        x[:, :, 1:] *= torch.exp2(torch.randint(-6, 7, (B, T_max, 2, H, 1), generator=g).float())
        qkv = x.to(BF).reshape(B, T_max, 3 * C)
        cache = o.kv8_cache_buffer(B, T_max, H, hs, DEV)
        o.kv8_cache_store(qkv.to(DEV), B, T_max, H, hs, cache, T_max, 0)
        K, V = _dequantized(cache, B, T_max, H, hs)
        _att[key] = dict(qkv=qkv, cache=cache, K=K, V=V, ref={})
    return _att[key]


def _reference(K, V, q, n, scale):
    """float64: o (B, C) and lse (B, H) of q (B, H, hs) over keys [0, n) of the dequantised cache"""
    s = torch.einsum("bhd,bhtd->bht", q.double(), K[:, :, :n]) * scale
    out = torch.einsum("bht,bhtd->bhd", torch.softmax(s, dim=-1), V[:, :, :n])
    return out.reshape(q.shape[0], -1), torch.logsumexp(s, dim=-1)


def _oracle(c, n, H, hs, scale):
    if n not in c["ref"]:
        B = c["qkv"].shape[0]
        c["ref"][n] = _reference(c["K"], c["V"], c["qkv"][:, n - 1, :H * hs].reshape(B, H, hs), n, scale)
    return c["ref"][n]


@pytest.mark.parametrize("hs", [64, 128])
@pytest.mark.parametrize("n_keys", [1, 2, 63, 64, 65, 257, 600, 1100])
def test_attn_decode_kv8_against_float64_on_the_dequantised_cache(hs, n_keys):
    """Every split count: the library's own, 1, and forced counts that leave splits empty at the small n_keys.  The query read in place
    from a packed row (q_ld = 3C) and from a dense [B, C] give the same bytes."""
    o = ops()
    B, H, T_max = 2, 2, 1100
    C = H * hs
    scale = 8.0 / C
    c = _decode_case(B, H, hs, T_max)
    ref_o, ref_lse = _oracle(c, n_keys, H, hs, scale)
    packed = c["qkv"][:, n_keys - 1].contiguous().to(DEV)
    dense = packed[:, :C].contiguous()
    for splits in (0, 1, 2, 7, L().ATTN_DECODE_MAX_SPLITS):
        got, lse = o.attn_decode_kv8(packed, c["cache"], B, T_max, n_keys, H, hs, scale, splits=splits)
        close(got, ref_o, atol=6e-3, what=f"attn_decode_kv8 hs={hs} n_keys={n_keys} splits={splits}")
        close(lse, ref_lse, atol=2e-3, rtol=1e-3, what=f"lse hs={hs} n_keys={n_keys} splits={splits}")
        got_c, lse_c = o.attn_decode_kv8(dense, c["cache"], B, T_max, n_keys, H, hs, scale, splits=splits)
        assert torch.equal(got, got_c) and torch.equal(lse, lse_c)


@pytest.mark.parametrize("hs", [64, 128])
@pytest.mark.parametrize("splits", [1, 3, 7])
def test_attn_decode_kv8_repeats_and_its_rows_form_is_the_uniform_form(hs, splits):
    o = ops()
    B, H, T_max = 2, 2, 1100
    C = H * hs
    c = _decode_case(B, H, hs, T_max)
    q = c["qkv"][:, 999].contiguous().to(DEV)
    uni = {}
    for n in (1, 64, 65, 600):
        uni[n] = o.attn_decode_kv8(q, c["cache"], B, T_max, n, H, hs, 8.0 / C, splits=splits)
        again = o.attn_decode_kv8(q, c["cache"], B, T_max, n, H, hs, 8.0 / C, splits=splits)
        assert torch.equal(uni[n][0], again[0]) and torch.equal(uni[n][1], again[1])
    for counts in ((1, 600), (64, 65), (65, 64), (600, 1)):
        rows = torch.tensor(counts, dtype=torch.int32, device=DEV)
        got, lse = o.attn_decode_kv8(q, c["cache"], B, T_max, 700, H, hs, 8.0 / C, splits=splits, n_keys_rows=rows)
        for b, n in enumerate(counts):
            assert torch.equal(got[b], uni[n][0][b]) and torch.equal(lse[b], uni[n][1][b]), (counts, b)
    for counts in ((0, 65), (601, -3)):                                 # outside [1, the host's bound = 600]: inactive
        rows = torch.tensor(counts, dtype=torch.int32, device=DEV)
        got, lse = o.attn_decode_kv8(q, c["cache"], B, T_max, 600, H, hs, 8.0 / C, splits=splits, n_keys_rows=rows)
        for b, n in enumerate(counts):
            if 1 <= n <= 600:
                assert torch.equal(got[b], uni[n][0][b]) and torch.equal(lse[b], uni[n][1][b])
            else:
                assert bool((got[b].view(torch.int16) == 0).all()) and bool((lse[b] == float("-inf")).all())


@pytest.mark.parametrize("hs", [64, 128])
@pytest.mark.parametrize("n_keys", [1, 65, 257])
def test_attn_decode_kv8_never_reads_the_tail_into_the_result(hs, n_keys):
    """positions >= n_keys hold zero codes and zero scales, then the NaN code 0x7F and NaN scales: finite and bitwise the same result"""
    o = ops()
    B, H, T_max = 2, 2, 384
    C = H * hs
    qkv = rnd(B, T_max, 3 * C, seed=hs + n_keys).to(DEV)
    q = qkv[:, n_keys - 1].contiguous()
    cache = o.kv8_cache_buffer(B, T_max, H, hs, DEV)
    o.kv8_cache_store(qkv, B, T_max, H, hs, cache, T_max, 0)
    kc, vc, ks, vs = KQ().split_cache(cache, B, T_max, H, hs)
    for splits in (0, 1, 7):
        res = []
        for code, word in ((0, 0), (0x7F, 0x7FC00000)):
            kc[:, :, n_keys:] = code
            vc[:, :, n_keys:] = code
            ks.view(torch.int32)[:, :, n_keys:] = word
            vs.view(torch.int32)[:, :, n_keys:] = word
            if word:
                assert torch.isnan(ks[:, :, n_keys:]).all() and torch.isnan(vc[:, :, n_keys:].view(torch.float8_e4m3fn).float()).all()
            res.append(o.attn_decode_kv8(q, cache, B, T_max, n_keys, H, hs, 8.0 / C, splits=splits))
        for a, b in zip(*res):
            assert torch.isfinite(a).all() and torch.isfinite(b).all()
            assert torch.equal(a, b)


def test_attn_decode_kv8_peaked_softmax_across_splits():
    """tests/test_hip_generate.py's case on the e4m3 cache: n_keys = 600 under 7 forced splits, one key of the last split that holds keys
    ahead of every other score by more than 40 while the others span about +-30 (judged on the dequantised cache, like the reference)"""
    o = ops()
    B, H, hs, n_keys, T_max, star = 2, 2, 128, 600, 600, 590
    C = H * hs
    scale = 8.0 / C
    qkv = rnd(B, T_max, 3 * C, seed=5)
    q = qkv[:, -1, :C].reshape(B, H, hs).float()
    k = qkv[:, :, C:2 * C].reshape(B, T_max, H, hs).transpose(1, 2).float()
    others = torch.einsum("bhd,bhtd->bht", q, k) * scale
    q = (q * (30.0 / others.abs().amax(dim=-1, keepdim=True))).to(BF)
    qf = q.float()
    kstar = (qf * ((30.0 + 50.0) / (scale * qf.square().sum(-1, keepdim=True)))).to(BF)
    qkv[:, -1, :C] = q.reshape(B, C)
    qkv[:, star, C:2 * C] = kstar.reshape(B, C)
    cache = o.kv8_cache_buffer(B, T_max, H, hs, DEV)
    o.kv8_cache_store(qkv.to(DEV), B, T_max, H, hs, cache, T_max, 0)
    K, V = _dequantized(cache, B, T_max, H, hs)
    s = torch.einsum("bhd,bhtd->bht", q.double(), K) * scale
    rest = torch.cat([s[..., :star], s[..., star + 1:]], dim=-1)
    assert (s[..., star] - rest.amax(dim=-1) > 40).all() and (rest.abs().amax(dim=-1) > 22).all() and (rest.abs().amax(dim=-1) < 38).all()
    ref, ref_lse = _reference(K, V, q, n_keys, scale)
    for splits in (7, 0, 1):
        got, lse = o.attn_decode_kv8(qkv[:, -1].contiguous().to(DEV), cache, B, T_max, n_keys, H, hs, scale, splits=splits)
        close(got, ref, atol=6e-3, what=f"peaked softmax, splits={splits}")
        close(lse, ref_lse, atol=2e-3, rtol=1e-3, what=f"peaked lse, splits={splits}")


# =================================================================================================== guard bands
@pytest.mark.parametrize("hs", [64, 128])
def test_kv8_kernels_inside_guard_bands(hs):
    """the three kernels with their operands 16 bytes into buffers that are NaN (inputs: bf16 NaN, the NaN code 0x7F) or a marker (outputs)
    everywhere else: the plain call's bits, and every guard intact"""
    from omnibiote_amd.model import rope_tables
    o = ops()
    B, H, T_max, t = 2, 2, 200, 150
    C = H * hs
    scale = 8.0 / C
    nbytes = 2 * B * H * T_max * (hs + 4)
    qkv = rnd(B, t, 3 * C, seed=hs).to(DEV)
    plain = o.kv8_cache_buffer(B, T_max, H, hs, DEV)
    plain.fill_(0x7F)
    o.kv8_cache_store(qkv, B, t, H, hs, plain, T_max, 0)
    fq, hq = fenced(qkv.view(B * t, 3 * C), poison="nan")
    fc, hc = fenced((nbytes,), dtype=torch.uint8, poison=0x7F, back_rows=1)
    o.kv8_cache_store(fq, B, t, H, hs, fc, T_max, 0)
    assert_same_bits(fc, plain, "cache after the store")
    assert_guards(hq, hc)
    # one step's rotate-and-store at positions 150 and 151
    rope = rope_tables(R.rope_table(hs, T_max).to(DEV))
    pos = torch.tensor([150, 151], dtype=torch.int32, device=DEV)
    step = rnd(B, 3 * C, seed=hs + 1).to(DEV)
    want_step = o.kv8_cache_rope_store_rows(step.clone(), rope, pos, 151, B, H, hs, plain, T_max)
    fs, hs_ = fenced(step, poison="nan")
    fcos, hcos = fenced(rope[0][:152].contiguous(), poison="nan")
    fsin, hsin = fenced(rope[1][:152].contiguous(), poison="nan")
    fp, hp = fenced(pos, poison="mark")
    o.kv8_cache_rope_store_rows(fs, (fcos, fsin), fp, 151, B, H, hs, fc, T_max)
    assert_same_bits(fs, want_step, "qkv after the rotation")
    assert_same_bits(fc, plain, "cache after the step")
    assert_guards(hs_, hcos, hsin, hp, hc)
    # attention over the 152 positions, uniform and per row
    q = want_step[:, :C].contiguous()
    for splits in (1, 3):
        for rows in (None, torch.tensor([152, 77], dtype=torch.int32, device=DEV)):
            want = o.attn_decode_kv8(q, plain, B, T_max, 152, H, hs, scale, splits=splits, n_keys_rows=rows)
            fqq, hqq = fenced(q, poison="nan", ld=C + 8)
            fo, ho = fenced((B, C), dtype=BF, poison="mark")
            fl, hl = fenced((B, H), dtype=torch.float32, poison="mark")
            ws, hw = fenced((int(L().lib().obte_attn_decode_ws_bytes(B, H, hs)),), dtype=torch.uint8, poison="mark", back_rows=1)
            fr, hr = (None, None) if rows is None else fenced(rows, poison="mark")
            got = o.attn_decode_kv8(fqq, fc, B, T_max, 152, H, hs, scale, splits=splits, q_ld=C + 8, ws=ws, n_keys_rows=fr, out=fo, lse=fl)
            assert_same_bits(got[0], want[0], "o")
            assert_same_bits(got[1], want[1], "lse")
            assert_guards(*[h for h in (hqq, hc, ho, hl, hr) if h is not None])
            used = B * H * splits * (hs + 4) * 4 if splits > 1 else 0
            assert bool((ws[used:] == 0x5A).all())                     # the workspace: nothing beyond the partials of `splits` splits


# =================================================================================================== block
NAMES = ["ln_1.weight", "attn.c_attn.weight", "attn.c_proj.weight", "ln_2.weight", "mlp.c_fc.weight", "mlp.c_proj.weight"]


@pytest.mark.parametrize("C,H", [(128, 2), (256, 2)])
def test_block_prefill_kv8_is_block_infer_and_leaves_the_quantised_cache(C, H):
    T, T_max = 130, 160
    c = _block_setup(C, H, T)
    o, B, hs = c["o"], c["B"], C // H
    x = c["x"].to(DEV)
    spec = c["causal"](T)
    want = o.block_infer(x, c["params"], c["rope"], H, spec)
    cache = o.kv8_cache_buffer(B, T_max, H, hs, DEV)
    cache.fill_(0x5A)
    got = o.block_prefill_kv8(x, c["params"], c["rope"], H, spec, cache, T_max)
    assert torch.equal(got, want)
    h1, _, _ = o.layernorm_fwd(x, c["params"][0])
    qkv = o.gemm(h1.view(B * T, C), c["params"][1], B * T, 3 * C, C, epilogue=L().EPI_ROPE_QK, rope=(c["rope"][0], c["rope"][1], T, hs))
    kc, vc, ks, vs = _parts(cache, B, T_max, H, hs)
    for codes, scales, want_kv in zip((kc, vc), (ks, vs), _thirds(qkv.cpu().view(B, T, 3 * C), B, T, H, hs)):
        wc, wsc = KQ().quantize_reference(want_kv)
        assert torch.equal(codes[:, :, :T], wc) and torch.equal(scales[:, :, :T].view(torch.int32), wsc.view(torch.int32))
        assert bool((codes[:, :, T:] == 0x5A).all()) and bool((scales[:, :, T:].view(torch.int32) == 0x5A5A5A5A).all())


def _block_step_reference(c, C, H, xt, t, K, V):
    """the oracle's block arithmetic (oracle/omnibiote_ref.py: block_forward) on ONE position t per row, xt (B, C) fp32, its attention
    over the keys and values [0, t] handed in as (B, H, t + 1, hs)"""
    w, pre = {k: v.float() for k, v in c["w"].items()}, c["pre"]
    B, hs = xt.shape[0], C // H
    h1 = R.layer_norm(xt, w[pre + "ln_1.weight"])
    q = F.linear(h1, w[pre + "attn.c_attn.weight"])[:, :C]
    q = R.apply_rope(q.reshape(B, 1, H, hs), c["tab"][t:t + 1]).transpose(1, 2)
    y = R.attention(q, K, V, 8.0 / C).transpose(1, 2).reshape(B, C)
    x1 = xt + F.linear(y, w[pre + "attn.c_proj.weight"])
    a = R.gelu_erf(F.linear(R.layer_norm(x1, w[pre + "ln_2.weight"]), w[pre + "mlp.c_fc.weight"]))
    return x1 + F.linear(a, w[pre + "mlp.c_proj.weight"])


@pytest.mark.parametrize("C,H", [(128, 2), (256, 2)])
@pytest.mark.parametrize("rows", [False, True])
def test_block_decode_kv8_step_by_step_vs_the_oracle_on_the_dequantised_cache(C, H, rows):
    """prefill x[:, :130], then positions 130 .. 159 one at a time, uniform or with the positions on the device: each step against the
    oracle's block arithmetic with the keys and values of positions [0, t] taken from the device's cache, dequantised (the block bar)"""
    T0, T = 130, 160
    c = _block_setup(C, H, T)
    o, B, hs = c["o"], c["B"], C // H
    x = c["x"].to(DEV)
    cache = o.kv8_cache_buffer(B, T, H, hs, DEV)
    o.block_prefill_kv8(x[:, :T0].contiguous(), c["params"], c["rope"], H, c["causal"](T0), cache, T)
    ws = o.block_decode_workspace(B, C, H, DEV)
    got = []
    for t in range(T0, T):
        xt = x[:, t].contiguous()
        pos_rows = torch.full((B,), t, dtype=torch.int32, device=DEV) if rows else None
        got.append(o.block_decode_kv8(xt, c["params"], c["rope"], H, cache, T, t, pos_rows=pos_rows, ws=ws))
        if t == T0:                                   # y may alias x (the step wrote position t: the same bytes again)
            assert torch.equal(o.block_decode_kv8(xt, c["params"], c["rope"], H, cache, T, t, pos_rows=pos_rows, ws=ws, out=xt), got[0])
    K, V = [z.float() for z in _dequantized(cache, B, T, H, hs)]      # (exact: 4 significant bits times a power of two)
    for t in range(T0, T):
        ref = _block_step_reference(c, C, H, c["x"][:, t].float(), t, K[:, :, :t + 1], V[:, :, :t + 1])
        close(got[t - T0], ref, atol=3e-2, rtol=2.0 ** -6, what=f"block decode kv8, position {t}")


# =================================================================================================== model
_quant_logits = {}


def _reference_logits(C, T0=130):
    """The oracle's forward of _gen_case(C)'s tokens where, per layer, rows < T0 take the unquantised attention (the prompt's own) and
    rows >= T0 attend over dequantize(quantize(bf16(k))) and the same of v: what prefill(T0) and decode steps on an fp8 cache compute."""
    if C not in _quant_logits:
        c = _gen_case(C)
        cfg, ids = c["cfg"], c["ids"]
        p = {k: v.to(BF).float() for k, v in R.hash_weights(cfg).items()}
        B, T = ids.shape
        H, hs = cfg.n_head, cfg.n_embd // cfg.n_head
        rope = R.cast_rope_table(R.rope_table(hs, T), BF)
        mask = _add(_tril(T))
        with torch.no_grad():
            x = F.embedding(ids, p["transformer.wte.weight"])
            for i in range(cfg.n_layer):
                pre = f"transformer.h.{i}."
                qkv = F.linear(R.layer_norm(x, p[pre + "ln_1.weight"]), p[pre + "attn.c_attn.weight"])
                q, k, v = qkv.split(C, dim=2)
                q = R.apply_rope(q.reshape(B, T, H, hs), rope).transpose(1, 2)
                k = R.apply_rope(k.reshape(B, T, H, hs), rope).transpose(1, 2)
                v = v.reshape(B, T, H, hs).transpose(1, 2)
                kq, vq = [KQ().dequantize_reference(*KQ().quantize_reference(z.to(BF))) for z in (k, v)]
                y = torch.cat([R.attention(q[:, :, :T0], k, v, 8.0 / C, mask[..., :T0, :]),
                               R.attention(q[:, :, T0:], kq, vq, 8.0 / C, mask[..., T0:, :])], dim=2)
                x = x + F.linear(y.transpose(1, 2).reshape(B, T, C), p[pre + "attn.c_proj.weight"])
                a = R.gelu_erf(F.linear(R.layer_norm(x, p[pre + "ln_2.weight"]), p[pre + "mlp.c_fc.weight"]))
                x = x + F.linear(a, p[pre + "mlp.c_proj.weight"])
            emb = R.layer_norm(x, p["transformer.ln_f.weight"])
            _quant_logits[C] = R.readout(emb, p["lm_head.weight"], cfg.n_embd / cfg.mup_base_width)
    return _quant_logits[C]


@pytest.mark.parametrize("C", [256, 128])
def test_teacher_forced_decode_on_an_fp8_cache_matches_the_oracle(C):
    """test_teacher_forced_decode_matches_the_oracle's case and bar on KVCache(dtype="fp8"), against the oracle with the quantiser in the
    decode rows' attention.  This checks the plumbing, not the format: on this model (random weights) quantisation itself moves the
    logits by only 4e-4 .. 8e-4, an order of magnitude inside the bar — a wrong scale or position is not."""
    from omnibiote_amd.model import KVCache
    c = _gen_case(C)
    m, idx = c["m"], c["ids"].to(DEV)
    cache = KVCache(m, 2, dtype="fp8")
    assert cache.dtype == "fp8" and cache.max_len == 200 and all(layer.dtype == torch.uint8 for layer in cache.layers)
    got = [m.prefill(idx[:, :130], cache)]
    for t in range(130, 199):
        assert cache.pos == t
        got.append(m.decode_step(idx[:, t], cache))
    got = torch.stack(got, dim=1).float().cpu()                   # positions 129 .. 198
    ref = _reference_logits(C)[:, 129:199]
    d = (got - ref).abs()
    moved = (ref - c["logits"][:, 129:199]).abs()
    print(f"fp8 cache, C={C}: logits vs the quantised oracle max {d.max().item():.3g} mean {d.mean().item():.3g}; "
          f"the quantiser moves the oracle's logits by max {moved.max().item():.3g} mean {moved.mean().item():.3g}")
    assert torch.isfinite(got).all()
    assert d.max().item() <= 5e-3 and d.mean().item() <= 1e-3, (d.max().item(), d.mean().item())


def _hand_loop(m, idx, n_new, lengths=None):
    from omnibiote_amd.model import KVCache, _next_tokens
    longest = idx.shape[1] if lengths is None else max(lengths)
    cache = KVCache(m, idx.shape[0], longest + n_new, dtype="fp8")
    logits = m.prefill(idx[:, :longest], cache, lengths=lengths)
    toks = []
    for i in range(n_new):
        toks.append(_next_tokens("generate", logits, 1.0, 1, None, None, None))
        if i + 1 < n_new:
            logits = m.decode_step(toks[-1], cache)
    return torch.stack(toks, dim=1), cache


def test_generate_on_an_fp8_cache():
    from omnibiote_amd.model import KVCache
    c = _gen_case(256)
    m, idx = c["m"], c["ids"][:, :130].to(DEV)
    cfg = c["cfg"]
    out = m.generate(idx, 24, top_k=1, kv_dtype="fp8")
    assert out.shape == (2, 154) and torch.equal(out[:, :130], idx)
    toks, cache = _hand_loop(m, idx, 24)
    assert torch.equal(out[:, 130:], toks)
    per_layer = L().lib().obte_kv8_cache_bytes(2, 154, cfg.n_head, cfg.n_embd // cfg.n_head)
    assert cache.dtype == "fp8" and sum(layer.numel() * layer.element_size() for layer in cache.layers) == cfg.n_layer * per_layer
    bf = KVCache(m, 2, 154)
    assert bf.dtype == "bf16" and sum(layer.numel() * layer.element_size() for layer in bf.layers) * (128 + 4) == cfg.n_layer * per_layer * 2 * 128
    # prompts of different lengths: one position per row
    lens = [130, 97]
    rag, rag_len = m.generate(idx, 24, top_k=1, lengths=lens, kv_dtype="fp8")
    toks_r, cache_r = _hand_loop(m, idx, 24, lengths=lens)
    assert cache_r.positions is not None and rag_len.tolist() == [154, 121]
    for b, n in enumerate(lens):
        assert torch.equal(rag[b, :n], idx[b, :n]) and torch.equal(rag[b, n:n + 24], toks_r[b])
    same, same_len = m.generate(idx, 24, top_k=1, lengths=[130, 130], kv_dtype="fp8")       # equal lengths: the uniform path's tokens
    assert torch.equal(same, out) and same_len.tolist() == [154, 154]
    # the device sampler runs on it, seeded
    a = m.generate(idx, 12, temperature=0.9, top_k=50, sampler="device", generator=torch.Generator(device=DEV).manual_seed(3), kv_dtype="fp8")
    b = m.generate(idx, 12, temperature=0.9, top_k=50, sampler="device", generator=torch.Generator(device=DEV).manual_seed(3), kv_dtype="fp8")
    assert a.shape == (2, 142) and torch.equal(a, b) and int(a[:, 130:].min()) >= 0 and int(a[:, 130:].max()) < cfg.vocab_size
    with pytest.raises(ValueError, match="kv_dtype"):
        m.generate(idx, 4, kv_dtype="fp4")


def test_an_fp8_cache_refuses_several_positions_per_call_and_keeps_its_state():
    from omnibiote_amd.model import KVCache
    c = _gen_case(256)
    m, idx = c["m"], c["ids"][:, :140].to(DEV)
    cache = KVCache(m, 2, 160, dtype="fp8")
    m.prefill(idx[:, :130], cache)
    with pytest.raises(NotImplementedError, match="fp8 cache"):
        m.extend(idx[:, 130:134], cache)
    with pytest.raises(NotImplementedError, match="fp8 cache"):
        m.prefill(idx, cache, chunk=64)
    with pytest.raises(NotImplementedError, match="fp8 cache"):
        m.draft_and_verify(m, idx[:, 130], cache, KVCache(m, 2, 160), 3)
    with pytest.raises(NotImplementedError, match="fp8"):
        m.generate_speculative(idx, 8, m, kv_dtype="fp8")
    assert cache.pos == 130 and cache.positions is None
    with pytest.raises(ValueError, match="dtype"):
        KVCache(m, 2, dtype="fp16")
    # the position operations touch no cache byte: they work as they are
    before = [layer.clone() for layer in cache.layers]
    cache.rewind(10)
    assert cache.pos == 120 and all(torch.equal(a, b) for a, b in zip(before, cache.layers))
    logits = m.decode_step(idx[:, 120], cache)                       # and the cache goes on from there
    assert cache.pos == 121 and torch.isfinite(logits).all()
