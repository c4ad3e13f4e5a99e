"""Many samples per prompt on the GPU (include/omnibiote_hip_shared.h): obte_attn_decode_shared against float64 torch on the concatenated
keys under default and forced split counts, bit for bit against itself (repeats, other group sizes and prompt counts, stale and foreign
cache contents), a peaked softmax in each part, guard bands, the block step against obte_block_decode on a replicated cache,
SharedPrefixCache / prefill / decode_step teacher-forced against the CPU oracle and generate(num_samples=) — at the bars of
tests/test_hip_extend.py for the same quantities: attention 2^-7 |ref| + 6e-3, lse atol 2e-3 / rtol 1e-3, block forward atol 3e-2 /
rtol 2^-6 (two paths against each other: twice that), model logits max <= 5e-3 / mean <= 1e-3 against the oracle and max <= 1e-2 /
mean <= 2e-3 between two paths."""
import numpy as np
import pytest
import torch

import omnibiote_ref as R
from fenced import assert_guards, assert_same_bits, fenced
from test_hip_causal import _add, _tril
from test_hip_generate import L, _block_setup, _gen_case, ops
from test_hip_ops import BF, DEV, close, rnd

pytestmark = pytest.mark.gpu

MAX = 32                      # OBTE_ATTN_SHARED_MAX_SPLITS
SPLITS = ((0, 0), (1, 1), (3, 2), (MAX, 1))
NAN = 0x7FC0
T_PRE, T_SUF = 704, 66


def _bits(t):
    return t.view(torch.int16) if t.dtype == BF else t.view(torch.int32)


def _same(a, b):
    return torch.equal(_bits(a[0]), _bits(b[0])) and torch.equal(_bits(a[1]), _bits(b[1]))


def _cache_of(k, v):
    """a layer cache (K [R, H, T, hs], then V) holding k and v"""
    return torch.stack([k, v]).contiguous().view(-1).to(DEV)


_cases = {}


def _case(hs, P, H, G, seed=0):
    """q (B, C), a prefix of T_PRE positions per prompt and a suffix of T_SUF slots per row, random bf16 (made once, never modified)"""
    key = (hs, P, H, G, seed)
    if key not in _cases:
        B = P * G
        c = dict(q=rnd(B, H * hs, seed=seed + 1), kp=rnd(P, H, T_PRE, hs, seed=seed + 2), vp=rnd(P, H, T_PRE, hs, seed=seed + 3),
                 ks=rnd(B, H, T_SUF, hs, seed=seed + 4), vs=rnd(B, H, T_SUF, hs, seed=seed + 5))
        c["prefix"], c["suffix"] = _cache_of(c["kp"], c["vp"]), _cache_of(c["ks"], c["vs"])
        _cases[key] = c
    return _cases[key]


def _reference(q, kp, vp, ks, vs, G, n_prefix, n_suffix, scale):
    """float64 softmax(q [K_prefix ; K_suffix]^T scale) [V_prefix ; V_suffix]: o (B, C) and lse (B, H)"""
    B, (P, H, _, hs) = q.shape[0], kp.shape
    k = torch.cat([kp[:, :, :n_prefix].repeat_interleave(G, 0), ks[:, :, :n_suffix]], dim=2).double()
    v = torch.cat([vp[:, :, :n_prefix].repeat_interleave(G, 0), vs[:, :, :n_suffix]], dim=2).double()
    s = torch.einsum("bhd,bhtd->bht", q.view(B, H, hs).double(), k) * scale
    o = torch.einsum("bht,bhtd->bhd", torch.softmax(s, dim=-1), v).reshape(B, H * hs)
    return o, torch.logsumexp(s, dim=-1)


def _run(c, P, H, G, hs, n_prefix, n_suffix, splits=(0, 0), **kw):
    q = kw.pop("q") if "q" in kw else c["q"].to(DEV)
    prefix = kw.pop("prefix") if "prefix" in kw else c["prefix"]
    suffix = kw.pop("suffix") if "suffix" in kw else c["suffix"]
    return ops().attn_decode_shared(q, prefix, P, T_PRE, n_prefix, suffix, G, T_SUF, n_suffix, H, hs, 8.0 / (H * hs), prefix_splits=splits[0],
                                    suffix_splits=splits[1], **kw)


# =================================================================================================== attention against float64
# (P, H, G, n_prefix, n_suffix): every G of {1, 3, 32, 33, 40} (the query-tile edge, padding queries), every n_prefix of {1, 31, 33, 130,
# 700} (the 32-key tile, the 4-wave stride of 128, several splits), every n_suffix of {0, 1, 2, 65}, both P and both H
CASES = [(1, 1, 1, 1, 0), (1, 2, 3, 31, 1), (3, 2, 32, 33, 2), (3, 1, 33, 130, 65), (1, 2, 40, 700, 65), (3, 2, 40, 130, 0), (1, 1, 3, 700, 2),
         (3, 2, 3, 1, 1), (1, 2, 33, 31, 65), (3, 2, 1, 700, 1), (1, 1, 32, 700, 0)]


@pytest.mark.parametrize("hs", [64, 128])
@pytest.mark.parametrize("P,H,G,n_prefix,n_suffix", CASES)
def test_attn_decode_shared_against_float64(hs, P, H, G, n_prefix, n_suffix):
    """The library's split counts and forced ones that leave splits empty at the small key counts; as a control obte_attn_decode on the
    replicated, concatenated cache meets the same bar."""
    o = ops()
    c = _case(hs, P, H, G)
    B, scale = P * G, 8.0 / (H * hs)
    ref_o, ref_lse = _reference(c["q"], c["kp"], c["vp"], c["ks"], c["vs"], G, n_prefix, n_suffix, scale)
    for splits in SPLITS:
        got, lse = _run(c, P, H, G, hs, n_prefix, n_suffix, splits)
        err = (got.float().cpu() - ref_o.float()).abs()
        print(f"attn_decode_shared hs={hs} P={P} H={H} G={G} n_prefix={n_prefix} n_suffix={n_suffix} splits={splits}: worst error / bar "
              f"{(err / (2.0 ** -7 * ref_o.float().abs() + 6e-3)).max().item():.3f}, lse error {(lse.cpu() - ref_lse.float()).abs().max().item():.3g}")
        close(got, ref_o, atol=6e-3, what=f"attn_decode_shared {(hs, P, H, G, n_prefix, n_suffix, splits)}")
        close(lse, ref_lse, atol=2e-3, rtol=1e-3, what=f"lse {(hs, P, H, G, n_prefix, n_suffix, splits)}")
        assert _same((got, lse), _run(c, P, H, G, hs, n_prefix, n_suffix, splits))                       # two calls, the same bytes
    n = n_prefix + n_suffix
    k = torch.cat([c["kp"][:, :, :n_prefix].repeat_interleave(G, 0), c["ks"][:, :, :n_suffix]], dim=2)
    v = torch.cat([c["vp"][:, :, :n_prefix].repeat_interleave(G, 0), c["vs"][:, :, :n_suffix]], dim=2)
    got, lse = o.attn_decode(c["q"].to(DEV), _cache_of(k, v), B, n, n, H, hs, scale)
    close(got, ref_o, atol=6e-3, what="control: obte_attn_decode on the replicated cache")
    close(lse, ref_lse, atol=2e-3, rtol=1e-3, what="control: lse")


def test_attn_decode_shared_without_a_suffix_cache():
    """n_suffix = 0: the suffix contributes exactly nothing, whether a suffix cache is handed over or not"""
    hs, P, H, G = 128, 3, 2, 33
    c = _case(hs, P, H, G)
    for splits in SPLITS:
        want = _run(c, P, H, G, hs, 130, 0, splits)
        got = ops().attn_decode_shared(c["q"].to(DEV), c["prefix"], P, T_PRE, 130, None, G, 0, 0, H, hs, 8.0 / (H * hs), prefix_splits=splits[0],
                                       suffix_splits=splits[1])
        assert _same(got, want), splits


# =================================================================================================== bitwise properties
@pytest.mark.parametrize("hs", [64, 128])
def test_a_row_has_the_same_bits_at_every_group_size_and_prompt_count(hs):
    """forced splits: row (p, g) of (P, G) = (3, 40) against the same query, prefix and suffix row in (3, 3), (1, 40) and (1, 3)"""
    H, n_prefix, n_suffix = 2, 130, 65
    big = _case(hs, 3, H, 40)

    def sub(ps, gs):
        rows = [p * 40 + g for p in ps for g in gs]
        return dict(q=big["q"][rows].to(DEV), prefix=_cache_of(big["kp"][ps], big["vp"][ps]), suffix=_cache_of(big["ks"][rows], big["vs"][rows])), rows
    for splits in ((3, 2), (1, 1), (MAX, 7)):
        want = _run(big, 3, H, 40, hs, n_prefix, n_suffix, splits)
        for ps, gs in (([0, 1, 2], [0, 1, 2]), ([1], list(range(40))), ([2], [37, 38, 39]), ([0, 1, 2], list(range(7, 40)))):
            kw, rows = sub(ps, gs)
            got = _run(None, len(ps), H, len(gs), hs, n_prefix, n_suffix, splits, **kw)
            assert torch.equal(_bits(got[0]), _bits(want[0][rows])) and torch.equal(_bits(got[1]), _bits(want[1][rows])), (hs, splits, ps, len(gs))


@pytest.mark.parametrize("hs", [64, 128])
@pytest.mark.parametrize("G,n_prefix,n_suffix", [(3, 1, 0), (33, 33, 2), (40, 130, 65), (3, 700, 1)])
def test_stale_positions_never_reach_a_result(hs, G, n_prefix, n_suffix):
    """prefix positions >= n_prefix and suffix slots >= n_suffix hold zeros, then the bf16 NaN pattern 0x7FC0: finite, the same bits"""
    P, H = 3, 2
    c = _case(hs, P, H, G)
    res = {}
    for pattern in (0, NAN):
        prefix, suffix = c["prefix"].clone(), c["suffix"].clone()
        prefix.view(torch.int16).view(2, P, H, T_PRE, hs)[:, :, :, n_prefix:] = pattern
        suffix.view(torch.int16).view(2, P * G, H, T_SUF, hs)[:, :, :, n_suffix:] = pattern
        if pattern:
            assert torch.isnan(prefix.view(2, P, H, T_PRE, hs)[:, :, :, n_prefix:]).all() and torch.isnan(suffix.view(2, P * G, H, T_SUF, hs)[:, :, :, n_suffix:]).all()
        res[pattern] = [_run(c, P, H, G, hs, n_prefix, n_suffix, splits, prefix=prefix, suffix=suffix) for splits in SPLITS]
    for a, b in zip(res[0], res[NAN]):
        assert torch.isfinite(b[0]).all() and torch.isfinite(b[1]).all() and _same(a, b), (hs, G, n_prefix, n_suffix)


@pytest.mark.parametrize("hs", [64, 128])
def test_a_row_depends_on_nothing_but_its_own_prompt_and_suffix(hs):
    """every other prompt's prefix, every other row's suffix and every other row's query replaced by NaN: row (1, 1) keeps its bits"""
    P, H, G, n_prefix, n_suffix = 3, 2, 33, 130, 65
    c = _case(hs, P, H, G)
    b0 = 1 * G + 1
    prefix, suffix, q = c["prefix"].clone(), c["suffix"].clone(), c["q"].to(DEV).clone()
    pv, sv = prefix.view(torch.int16).view(2, P, H, T_PRE, hs), suffix.view(torch.int16).view(2, P * G, H, T_SUF, hs)
    pv[:, 0], pv[:, 2] = NAN, NAN
    sv[:, :b0], sv[:, b0 + 1:] = NAN, NAN
    q.view(torch.int16)[:b0], q.view(torch.int16)[b0 + 1:] = NAN, NAN
    for splits in SPLITS:
        want = _run(c, P, H, G, hs, n_prefix, n_suffix, splits)
        got = _run(c, P, H, G, hs, n_prefix, n_suffix, splits, q=q, prefix=prefix, suffix=suffix)
        assert torch.isfinite(got[0][b0]).all() and torch.equal(_bits(got[0][b0]), _bits(want[0][b0])) and torch.equal(_bits(got[1][b0]), _bits(want[1][b0])), splits
        assert not torch.isfinite(got[0][:G]).any()                                                      # the poison was one


# =================================================================================================== peaked softmax across the parts
@pytest.mark.parametrize("hs", [64, 128])
@pytest.mark.parametrize("where", ["first prefix split", "last prefix tile", "suffix"])
def test_peaked_softmax_across_the_parts(hs, where):
    """One key whose scaled score exceeds every other of row (0, 1) by about 60 while the others span +-30 — in the first prefix split,
    in the prefix's last 32-key tile, in the row's suffix — so that the partials of the other part, splits and waves carry weights of
    e^-60 against a maximum they never saw.  Every row against float64, lse too."""
    P, H, G, n_prefix, n_suffix, row = 1, 2, 3, 700, 65, 1
    scale = 8.0 / (H * hs)
    c = _case(hs, P, H, G, seed=50)
    q, kp, ks = c["q"].clone(), c["kp"].clone(), c["ks"].clone()
    qr = q[row].view(H, hs).float()
    keys = torch.cat([kp[0, :, :n_prefix], ks[row, :, :n_suffix]], dim=1).float()                      # [H, n, hs]
    others = torch.einsum("hd,htd->ht", qr, keys) * scale
    qr = (qr * (30.0 / others.abs().amax(dim=-1, keepdim=True))).to(BF)                                  # the other scores now span +-30
    qf = qr.float()
    kstar = (qf * ((30.0 + 60.0) / (scale * qf.square().sum(-1, keepdim=True)))).to(BF)                 # q . k* scale = 90
    q[row] = qr.reshape(-1)
    if where == "suffix":
        ks[row, :, 1] = kstar
    else:
        kp[0, :, 5 if where == "first prefix split" else n_prefix - 3] = kstar
    s = torch.einsum("hd,htd->ht", q[row].view(H, hs).float(), torch.cat([kp[0, :, :n_prefix], ks[row, :, :n_suffix]], dim=1).float()) * scale
    top = s.max(dim=-1).values
    rest = s.masked_fill(s == top.unsqueeze(-1), float("-inf")).amax(dim=-1)
    assert (top - rest > 55).all() and (top > 85).all()
    ref_o, ref_lse = _reference(q, kp, c["vp"], ks, c["vs"], G, n_prefix, n_suffix, scale)
    assert torch.isfinite(ref_o).all() and torch.isfinite(ref_lse).all()
    for splits in ((3, 2), (0, 0), (1, 1), (MAX, 7)):
        got, lse = _run(None, P, H, G, hs, n_prefix, n_suffix, splits, q=q.to(DEV), prefix=_cache_of(kp, c["vp"]), suffix=_cache_of(ks, c["vs"]))
        close(got, ref_o, atol=6e-3, what=f"peaked softmax in the {where}, splits={splits}")
        close(lse, ref_lse, atol=2e-3, rtol=1e-3, what=f"peaked lse in the {where}, splits={splits}")


# =================================================================================================== guard bands
@pytest.mark.parametrize("hs,G,n_prefix,n_suffix", [(64, 33, 33, 2), (128, 3, 130, 65)])
def test_attn_decode_shared_stays_inside_its_buffers(hs, G, n_prefix, n_suffix):
    """q (packed rows, q_ld = 3C), both caches (exactly n_prefix positions and n_suffix slots), o, lse and the workspace (exactly the bytes
    asked for) in poisoned buffers that start 16 bytes behind a 512-byte boundary: the plain call's bits, and no guard byte written"""
    o = ops()
    P, H = 3, 2
    B, Cc, scale = P * G, H * hs, 8.0 / (H * hs)
    c = _case(hs, P, H, G)
    kp, vp, ks, vs = c["kp"][:, :, :n_prefix], c["vp"][:, :, :n_prefix], c["ks"][:, :, :n_suffix], c["vs"][:, :, :n_suffix]
    prefix, suffix, q = _cache_of(kp, vp), _cache_of(ks, vs), c["q"].to(DEV)
    for splits in ((0, 0), (3, 2)):
        want = o.attn_decode_shared(q, prefix, P, n_prefix, n_prefix, suffix, G, n_suffix, n_suffix, H, hs, scale, prefix_splits=splits[0], suffix_splits=splits[1])
        fq, hq = fenced(q, poison="nan", ld=3 * Cc)
        fp, hp = fenced(prefix, poison="nan")
        fs, hsuf = fenced(suffix, poison="nan")
        fo, ho = fenced((B, Cc), BF, "mark")
        fl, hl = fenced((B, H), torch.float32, "mark")
        fw, hw = fenced((int(L().lib().obte_attn_decode_shared_ws_bytes(P, G, H, hs, *splits)),), torch.uint8, "mark")
        got = o.attn_decode_shared(fq, fp, P, n_prefix, n_prefix, fs, G, n_suffix, n_suffix, H, hs, scale, prefix_splits=splits[0], suffix_splits=splits[1],
                                   q_ld=3 * Cc, ws=fw, out=fo, lse=fl)
        torch.cuda.synchronize()
        assert_same_bits(got[0], want[0], f"o, splits={splits}")
        assert_same_bits(got[1], want[1], f"lse, splits={splits}")
        assert_guards(hq, hp, hsuf, ho, hl, hw)


# =================================================================================================== block
@pytest.mark.parametrize("C,H", [(128, 2), (256, 2)])
def test_block_decode_shared_against_block_decode_on_a_replicated_cache(C, H):
    """P = 2 prompts of 37 positions, G = 3 rows each with inputs of their own, 4 steps: the shared step against obte_block_decode on a
    cache that holds the prompt once per row, within twice the block bar; on the weight-streaming products and with them off."""
    T0, T, P, G, steps = 37, 48, 2, 3, 4
    c = _block_setup(C, H, T)
    o, hs, B = c["o"], C // H, P * G
    x0 = c["x"][:, :T0].contiguous().to(DEV)                                                             # (P, T0, C)
    xs = rnd(steps, B, C, seed=C).to(DEV)
    prefix = o.kv_cache_buffer(P, T0, H, hs, DEV)
    o.block_prefill(x0, c["params"], c["rope"], H, c["causal"](T0), prefix, T0)
    from omnibiote_amd.masks import RangeMask
    rep = o.kv_cache_buffer(B, T, H, hs, DEV)
    o.block_prefill(x0.repeat_interleave(G, 0).contiguous(), c["params"], c["rope"], H, o.MaskSpec.from_user(RangeMask.causal(B, T0, DEV), B, T0, H, DEV), rep, T)
    for limit in (L().lib().obte_small_m_max(), 0):
        suffix = o.kv_cache_buffer(B, steps, H, hs, DEV)
        suffix.view(torch.int16).fill_(NAN)
        cache = rep.clone()
        ws = o.block_decode_shared_workspace(P, G, C, H, DEV)
        with o.small_m_max(limit):
            for i in range(steps):
                want = o.block_decode(xs[i], c["params"], c["rope"], H, cache, T, T0 + i)
                got = o.block_decode_shared(xs[i], c["params"], c["rope"], H, prefix, P, T0, T0, suffix, steps, i, ws=ws)
                assert torch.isfinite(got).all()
                d = (got.float() - want.float()).abs()
                assert (d <= 2 * (3e-2 + 2.0 ** -6 * want.float().abs())).all(), (limit, i, d.max().item())
                if i == 0:                                                                               # y may alias x
                    xt = xs[0].clone()
                    assert torch.equal(o.block_decode_shared(xt, c["params"], c["rope"], H, prefix, P, T0, T0, suffix, steps, 0, ws=ws, out=xt), got)
        # the suffix holds what the replicated cache holds at the rows' own positions (the same rotation row, the same store)
        K, Kr = suffix.view(2, B, H, steps, hs), cache.view(2, B, H, T, hs)[:, :, :, T0:T0 + steps]
        assert torch.equal(_bits(K), _bits(Kr.contiguous()))


# =================================================================================================== model
_teacher = {}


def _teacher_case(C):
    """P = 2 prompts of 37 tokens, G = 3 continuations of 6 given tokens each, and the oracle's causal logits of the six full rows"""
    if C not in _teacher:
        c = _gen_case(C)
        P, G, T0, steps = 2, 3, 37, 6
        rng = np.random.default_rng(C + 1)
        prompts = torch.from_numpy(rng.integers(4, c["cfg"].vocab_size, size=(P, T0)).astype(np.int64))
        tails = torch.from_numpy(rng.integers(4, c["cfg"].vocab_size, size=(P * G, steps)).astype(np.int64))
        rows = torch.cat([prompts.repeat_interleave(G, 0), tails], dim=1)
        wb = {k: v.to(BF).float() for k, v in R.hash_weights(c["cfg"]).items()}
        rope = R.cast_rope_table(R.rope_table(c["cfg"].n_embd // c["cfg"].n_head, T0 + steps), BF)
        with torch.no_grad():
            logits = R.model_forward(wb, c["cfg"], rows, _add(_tril(T0 + steps)), rope=rope)
        _teacher[C] = dict(m=c["m"], prompts=prompts, tails=tails, rows=rows, logits=logits, P=P, G=G, T0=T0, steps=steps)
    return _teacher[C]


@pytest.mark.parametrize("C", [128, 256])
def test_teacher_forced_shared_decode_matches_the_oracle_and_the_replicated_cache(C):
    from omnibiote_amd.model import KVCache, SharedPrefixCache
    t = _teacher_case(C)
    m, P, G, T0, steps = t["m"], t["P"], t["G"], t["T0"], t["steps"]
    prompts, tails = t["prompts"].to(DEV), t["tails"].to(DEV)
    shared = SharedPrefixCache(m, P, G, T0, steps)
    rep = KVCache(m, P * G, T0 + steps)
    got, want = [m.prefill(prompts, shared)], [m.prefill(prompts.repeat_interleave(G, 0), rep)]
    assert got[0].shape == (P * G, m.config.vocab_size) and shared.pos == T0 and shared.n_prefix == T0
    assert torch.equal(got[0].view(P, G, -1), got[0].view(P, G, -1)[:, :1].expand(P, G, -1))             # row p, G times
    for i in range(steps):
        assert shared.pos == T0 + i
        got.append(m.decode_step(tails[:, i], shared))
        want.append(m.decode_step(tails[:, i], rep))
    with pytest.raises(ValueError, match="full"):
        m.decode_step(tails[:, 0], shared)
    got, want = torch.stack(got, dim=1).float().cpu(), torch.stack(want, dim=1).float().cpu()            # positions T0 - 1 .. T0 + steps - 1
    assert torch.isfinite(got).all()
    d = (got - t["logits"][:, T0 - 1:]).abs()
    print(f"shared decode vs the oracle, C={C}: max {d.max().item():.4g}, mean {d.mean().item():.4g}")
    assert d.max().item() <= 5e-3 and d.mean().item() <= 1e-3, (d.max().item(), d.mean().item())
    d = (got - want).abs()
    print(f"shared decode vs the replicated cache, C={C}: max {d.max().item():.4g}, mean {d.mean().item():.4g}")
    assert d.max().item() <= 1e-2 and d.mean().item() <= 2e-3, (d.max().item(), d.mean().item())


def test_generate_num_samples():
    c = _gen_case(256)
    m = c["m"]
    P, G, T0, n = 2, 5, 37, 12
    idx = c["ids"][:, :T0].to(DEV)
    out = m.generate(idx, n, top_k=1, num_samples=G)
    assert out.shape == (P * G, T0 + n) and out.dtype == torch.int64
    assert torch.equal(out[:, :T0], idx.repeat_interleave(G, 0))                                         # row p G + g starts with prompt p
    assert torch.equal(out.view(P, G, -1), out.view(P, G, -1)[:, :1].expand(P, G, -1))                   # greedy: the same bits at every g
    assert torch.equal(m.generate(idx, 0, num_samples=G), idx.repeat_interleave(G, 0))

    def seeded(seed, **kw):
        return m.generate(idx, n, temperature=1.0, top_k=50, top_p=0.95, sampler="device", generator=torch.Generator(device=DEV).manual_seed(seed),
                          num_samples=G, **kw)
    a, b, other = seeded(11), seeded(11), seeded(12)
    assert a.shape == (P * G, T0 + n) and torch.equal(a, b) and not torch.equal(a, other)
    for p in range(P):
        assert len({tuple(r) for r in a[p * G:(p + 1) * G, T0:].tolist()}) > 1                          # the samples of a prompt differ
    t = m.generate(idx, n, temperature=0.9, top_k=50, generator=torch.Generator(device=DEV).manual_seed(3), num_samples=G)      # the torch sampler
    assert t.shape == (P * G, T0 + n) and torch.equal(t[:, :T0], idx.repeat_interleave(G, 0))
    eos = int(out[0, T0])                                                                                # prompt 0's first greedy token
    e = m.generate(idx, n, top_k=1, eos_token=eos, num_samples=G)
    gen = e[:, T0:]
    assert (gen[:G] == eos).all()                                                                        # a finished row keeps producing it
    for r in range(P * G):
        hit = (gen[r] == eos).nonzero().flatten()
        if hit.numel():
            assert (gen[r, int(hit[0]):] == eos).all()
    assert torch.equal(gen[G:, :1], out[G:, T0:T0 + 1])


def test_shared_cache_buffers_and_refusals():
    from omnibiote_amd.model import SharedPrefixCache
    c = _gen_case(256)
    m, cfg = c["m"], c["cfg"]
    P, G, T0, n = 2, 5, 37, 12
    hs = cfg.n_embd // cfg.n_head
    cache = SharedPrefixCache(m, P, G, T0, n)
    assert (cache.batch, cache.max_len, cache.group, cache.prompts, cache.dtype) == (P * G, T0 + n, G, P, "bf16") and len(cache.layers) == cfg.n_layer
    f = L().lib().obte_kv_cache_bytes
    for prefix, suffix in cache.layers:
        assert prefix.numel() * 2 + suffix.numel() * 2 == f(P, T0, cfg.n_head, hs) + f(P * G, n, cfg.n_head, hs)
        assert prefix.numel() * 2 == f(P, T0, cfg.n_head, hs)
    idx = c["ids"][:, :T0].to(DEV)
    with pytest.raises(ValueError, match="lengths"):
        m.prefill(idx, cache, lengths=[T0, T0])
    with pytest.raises(ValueError, match="chunk"):
        m.prefill(idx, cache, chunk=16)
    with pytest.raises(ValueError, match="empty"):
        m.decode_step(idx.repeat_interleave(G, 0)[:, 0], cache)
    m.prefill(idx, cache)
    with pytest.raises(NotImplementedError, match="SharedPrefixCache"):
        m.extend(idx.repeat_interleave(G, 0)[:, :4], cache)
    with pytest.raises(NotImplementedError, match="SharedPrefixCache"):
        m.generate_speculative(idx, 4, m, num_samples=G)
    with pytest.raises(ValueError, match="num_samples"):
        m.generate(idx, 4, num_samples=G, lengths=[T0, T0])
    with pytest.raises(ValueError, match="num_samples"):
        m.generate(idx, 4, num_samples=G, kv_dtype="fp8")
    assert cache.pos == T0
    with pytest.raises(ValueError, match="prefix"):
        cache.rewind(1)
    m.decode_step(idx.repeat_interleave(G, 0)[:, 0], cache)
    m.decode_step(idx.repeat_interleave(G, 0)[:, 1], cache)
    cache.rewind(1)
    assert cache.pos == T0 + 1
