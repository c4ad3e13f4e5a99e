"""Continuing a filled key/value cache by several positions per row on the GPU (include/omnibiote_hip_extend.h): obte_attn_extend under
every split count against the CPU oracle (oracle/omnibiote_ref.py, fp32) and bit for bit against itself (repeats, stale cache
positions, later rows of the chunk, the rows form row by row), the chunk's rotate-and-store against the GEMM's RoPE epilogue +
obte_kv_cache_store, guard bands, the block, OmniBioTA.extend / KVCache.rewind and the chunked prefill — at the bars of
tests/test_hip_generate.py for the same quantities: attention forward 2^-7 |ref| + 6e-3, lse atol 2e-3 / rtol 1e-3, block forward
atol 3e-2 / rtol 2^-6, model logits max <= 5e-3 / mean <= 1e-3."""
import ctypes as C

import numpy as np
import pytest
import torch

import omnibiote_ref as R
from fenced import assert_guards, assert_same_bits, fenced
from test_hip_causal import _add, _model, _tril
from test_hip_generate import L, _block_setup, _decode_case, _gen_case, _views, ops
from test_hip_ops import BF, DEV, close, rnd

pytestmark = pytest.mark.gpu

MAX = 32                      # OBTE_ATTN_EXTEND_MAX_SPLITS
SPLITS = (0, 1, 2, 7, MAX)
NEG_INF = float("-inf")
NAN = 0x7FC0
CASES = [(0, 1), (0, 5), (0, 33), (1, 2), (31, 2), (63, 3), (64, 32), (250, 7), (299, 64), (600, 100), (1000, 100)]


def _i32(values):
    return torch.tensor(list(values), dtype=torch.int32, device=DEV)


def _resolved(splits, B, H, hs, n, keys):
    return splits if splits else int(L().lib().obte_attn_extend_splits(B, H, hs, n, keys))


def _chunk_oracle(q, k, v, pos, n, scale):
    """o (B * n, C) and lse (B, H, n) of the queries at positions pos .. pos + n - 1 over keys [0, pos + j + 1)"""
    B, H = q.shape[:2]
    mask = _add(_tril(pos + n)[pos:pos + n])
    qq, kk, vv = q[:, :, pos:pos + n], k[:, :, :pos + n], v[:, :, :pos + n]
    out = R.attention(qq, kk, vv, scale, mask).transpose(1, 2).reshape(B * n, -1)
    lse = torch.logsumexp((qq @ kk.transpose(-2, -1)) * scale + mask, dim=-1)
    return out, lse


def _bits(t):
    return t.view(torch.int16) if t.dtype == BF else t.view(torch.int32)


def _same(a, b):
    return torch.equal(_bits(a[0]), _bits(b[0])) and torch.equal(_bits(a[1]), _bits(b[1]))


# =================================================================================================== attention against the oracle
@pytest.mark.parametrize("hs", [64, 128])
@pytest.mark.parametrize("pos,n", CASES)
def test_attn_extend_against_the_oracle(hs, pos, n):
    """Every split count: the library's own, 1, and forced counts that leave splits empty at the small key counts.  The queries read in
    place from packed rows (q_ld = 3C) and from a dense [B n, C] give the same bytes; as a control, obte_attn_fwd with the causal tables
    over [0, pos + n) meets the same bar on the same rows."""
    o = ops()
    B, H, T_max = 2, 2, 1100
    Cc = H * hs
    scale = 8.0 / Cc
    c = _decode_case(B, H, hs, T_max)
    ref_o, ref_lse = _chunk_oracle(c["q"], c["k"], c["v"], pos, n, scale)
    packed = c["qkv"][:, pos:pos + n].contiguous().to(DEV)          # [B, n, 3C]
    dense = packed[..., :Cc].contiguous()
    for splits in SPLITS:
        got, lse = o.attn_extend(packed, c["cache"], B, T_max, n, pos, H, hs, scale, splits=splits)
        err = (got.float().cpu() - ref_o).abs()
        print(f"attn_extend hs={hs} pos={pos} n={n} splits={splits}: worst error / bar {(err / (2.0 ** -7 * ref_o.abs() + 6e-3)).max().item():.3f}, "
              f"lse error {(lse.cpu() - ref_lse).abs().max().item():.3g}")
        close(got, ref_o, atol=6e-3, what=f"attn_extend hs={hs} pos={pos} n={n} splits={splits}")
        close(lse, ref_lse, atol=2e-3, rtol=1e-3, what=f"lse hs={hs} pos={pos} n={n} splits={splits}")
        assert _same((got, lse), o.attn_extend(dense, c["cache"], B, T_max, n, pos, H, hs, scale, splits=splits))
    from omnibiote_amd.masks import RangeMask
    T = pos + n
    full, _ = o.attn_fwd(c["qkv"][:, :T].contiguous().to(DEV), B, T, H, hs, scale, mask=o.MaskSpec.from_user(RangeMask.causal(B, T, DEV), B, T, H, DEV))[:2]
    close(full.view(B, T, Cc)[:, pos:].reshape(B * n, Cc), ref_o, atol=6e-3, what="control: obte_attn_fwd under the causal tables")


def test_attn_extend_one_sequence_one_head():
    o = ops()
    B, H, hs, T_max, pos, n = 1, 1, 128, 300, 230, 70
    scale = 8.0 / (H * hs)
    c = _decode_case(B, H, hs, T_max)
    ref_o, ref_lse = _chunk_oracle(c["q"], c["k"], c["v"], pos, n, scale)
    for splits in (0, 1, 7):
        got, lse = o.attn_extend(c["qkv"][:, pos:pos + n].contiguous().to(DEV), c["cache"], B, T_max, n, pos, H, hs, scale, splits=splits)
        close(got, ref_o, atol=6e-3, what=f"B=H=1 splits={splits}")
        close(lse, ref_lse, atol=2e-3, rtol=1e-3, what="lse")


# =================================================================================================== bitwise properties
@pytest.mark.parametrize("hs", [64, 128])
def test_attn_extend_is_bitwise_repeatable(hs):
    o = ops()
    B, H, T_max, pos, n = 2, 2, 1100, 600, 100
    c = _decode_case(B, H, hs, T_max)
    q = c["qkv"][:, pos:pos + n].contiguous().to(DEV)
    for splits in SPLITS:
        a = o.attn_extend(q, c["cache"], B, T_max, n, pos, H, hs, 8.0 / (H * hs), splits=splits)
        b = o.attn_extend(q, c["cache"], B, T_max, n, pos, H, hs, 8.0 / (H * hs), splits=splits)
        assert _same(a, b), (hs, splits)


@pytest.mark.parametrize("hs", [64, 128])
@pytest.mark.parametrize("pos,n", [(0, 5), (63, 3), (299, 64), (600, 100)])
def test_attn_extend_never_reads_stale_positions_into_the_result(hs, pos, n):
    """every cache position >= pos + n holds the bf16 NaN pattern 0x7FC0: finite, and no byte of o or lse changes"""
    o = ops()
    B, H, T_max = 2, 2, 1100
    c = _decode_case(B, H, hs, T_max)
    q = c["qkv"][:, pos:pos + n].contiguous().to(DEV)
    dirty = c["cache"].clone()
    dirty.view(torch.int16).view(2, B, H, T_max, hs)[:, :, :, pos + n:] = NAN
    assert torch.isnan(dirty.view(2, B, H, T_max, hs)[:, :, :, pos + n:]).all()
    for splits in SPLITS:
        clean = o.attn_extend(q, c["cache"], B, T_max, n, pos, H, hs, 8.0 / (H * hs), splits=splits)
        got = o.attn_extend(q, dirty, B, T_max, n, pos, H, hs, 8.0 / (H * hs), splits=splits)
        assert torch.isfinite(got[0]).all() and torch.isfinite(got[1]).all() and _same(got, clean), (hs, pos, n, splits)


@pytest.mark.parametrize("hs", [64, 128])
def test_attn_extend_rows_do_not_depend_on_later_rows_of_the_chunk(hs):
    """rows j' > j of the chunk — their q, and their k and v in the cache — replaced by other finite values: rows <= j bit for bit"""
    o = ops()
    B, H, T_max, pos, n = 2, 2, 320, 250, 40
    Cc = H * hs
    scale = 8.0 / Cc
    qkv = rnd(B, T_max, 3 * Cc, seed=hs + 9).to(DEV)
    other = rnd(B, T_max, 3 * Cc, seed=hs + 10, scale=3.0).to(DEV)
    cache = o.kv_cache_buffer(B, T_max, H, hs, DEV)
    for splits in (1, 3):
        o.kv_cache_store(qkv, B, T_max, H, hs, cache, T_max, 0)
        want = o.attn_extend(qkv[:, pos:pos + n].contiguous(), cache, B, T_max, n, pos, H, hs, scale, splits=splits)
        for j in (0, 17, 31, 32):
            changed = qkv.clone()
            changed[:, pos + j + 1:] = other[:, pos + j + 1:]
            o.kv_cache_store(changed, B, T_max, H, hs, cache, T_max, 0)
            got = o.attn_extend(changed[:, pos:pos + n].contiguous(), cache, B, T_max, n, pos, H, hs, scale, splits=splits)
            keep = slice(0, j + 1)
            assert torch.equal(_bits(got[0].view(B, n, Cc)[:, keep]), _bits(want[0].view(B, n, Cc)[:, keep])), (hs, splits, j)
            assert torch.equal(_bits(got[1][:, :, keep]), _bits(want[1][:, :, keep])), (hs, splits, j)
            assert not torch.equal(got[0].view(B, n, Cc)[:, j + 1:], want[0].view(B, n, Cc)[:, j + 1:])      # the change was one


@pytest.mark.parametrize("star", [5, 590])
def test_attn_extend_peaked_softmax_across_splits(star):
    """The chunk's last query (position 599) has one key — in the first split or in the last — whose scaled score exceeds every other
    by more than 40 while the others span +-30: the partials of the other splits and waves carry weights of e^-40 and below against a
    maximum they never saw.  Every row of the chunk against the oracle."""
    o = ops()
    B, H, hs, T_max, pos, n = 2, 2, 128, 600, 560, 40
    Cc = H * hs
    scale = 8.0 / Cc
    qkv = rnd(B, T_max, 3 * Cc, seed=5)
    q = qkv[:, -1, :Cc].reshape(B, H, hs).float()
    k = qkv[:, :, Cc:2 * Cc].reshape(B, T_max, H, hs).transpose(1, 2).float()
    others = torch.einsum("bhd,bhtd->bht", q, k) * scale
    q = (q * (30.0 / others.abs().amax(dim=-1, keepdim=True))).to(BF)
    qf = q.float()
    kstar = (qf * ((30.0 + 50.0) / (scale * qf.square().sum(-1, keepdim=True)))).to(BF)   # q . k* scale = 80
    qkv[:, -1, :Cc] = q.reshape(B, Cc)
    qkv[:, star, Cc:2 * Cc] = kstar.reshape(B, Cc)
    qq, kk, vv = [t.reshape(B, T_max, H, hs).transpose(1, 2).float() for t in qkv.split(Cc, dim=2)]
    s = (qq[:, :, -1:] @ kk.transpose(-2, -1)).squeeze(2) * scale
    rest = torch.cat([s[..., :star], s[..., star + 1:]], dim=-1)
    assert (s[..., star] - rest.amax(dim=-1) > 40).all() and (rest.abs().amax(dim=-1) > 25).all() and (rest.abs().amax(dim=-1) < 35).all()
    ref_o, ref_lse = _chunk_oracle(qq, kk, vv, pos, n, scale)
    assert torch.isfinite(ref_o).all() and torch.isfinite(ref_lse).all()
    cache = o.kv_cache_buffer(B, T_max, H, hs, DEV)
    o.kv_cache_store(qkv.to(DEV), B, T_max, H, hs, cache, T_max, 0)
    for splits in (7, 0, 1, MAX):
        got, lse = o.attn_extend(qkv[:, pos:].contiguous().to(DEV), cache, B, T_max, n, pos, H, hs, scale, splits=splits)
        close(got, ref_o, atol=6e-3, what=f"peaked softmax, star={star} splits={splits}")
        close(lse, ref_lse, atol=2e-3, rtol=1e-3, what=f"peaked lse, star={star} splits={splits}")


# =================================================================================================== rows form
@pytest.mark.parametrize("hs", [64, 128])
@pytest.mark.parametrize("n", [5, 40])
def test_attn_extend_rows_is_the_uniform_call_row_by_row(hs, n):
    o = ops()
    B, H, T_max = 4, 2, 1100
    starts = (0, 37, 600, 1000)
    Cc = H * hs
    scale = 8.0 / Cc
    c = _decode_case(B, H, hs, T_max)
    q = torch.stack([c["qkv"][b, p:p + n] for b, p in enumerate(starts)]).contiguous().to(DEV)
    bound = max(starts)
    for splits in SPLITS:
        got, lse = o.attn_extend(q, c["cache"], B, T_max, n, bound, H, hs, scale, splits=splits, pos_rows=_i32(starts))
        forced = _resolved(splits, B, H, hs, n, bound + n)
        for b, p in enumerate(starts):
            want, want_lse = o.attn_extend(q, c["cache"], B, T_max, n, p, H, hs, scale, splits=forced)
            assert torch.equal(_bits(got.view(B, n, Cc)[b]), _bits(want.view(B, n, Cc)[b])) and torch.equal(_bits(lse[b]), _bits(want_lse[b])), (hs, splits, b)
        if splits in (0, 7):
            for b, p in enumerate(starts):
                ref_o, ref_lse = _chunk_oracle(c["q"][b:b + 1], c["k"][b:b + 1], c["v"][b:b + 1], p, n, scale)
                close(got.view(B, n, Cc)[b], ref_o, atol=6e-3, what=f"attn_extend rows hs={hs} row {b} splits={splits}")
                close(lse[b:b + 1], ref_lse, atol=2e-3, rtol=1e-3, what=f"lse rows hs={hs} row {b} splits={splits}")


@pytest.mark.parametrize("hs", [64, 128])
def test_attn_extend_rows_inactive_rows(hs):
    """positions of -1, bound + 1 (inside the cache, outside the bound) and T_max beside a valid row: zeros and lse = -inf for those,
    the valid row bit for bit the uniform call's.  The inactive rows' whole cache is NaN: none of it is read into anything."""
    o = ops()
    B, H, T_max, bound, n = 4, 2, 1100, 600, 5
    Cc = H * hs
    scale = 8.0 / Cc
    c = _decode_case(B, H, hs, T_max)
    for n in (5, 40):
        for starts in ((-1, 65, bound + 1, T_max), (600, -(2 ** 31), 0, 2 ** 31 - 1)):
            active = [0 <= p <= bound for p in starts]
            q = torch.stack([c["qkv"][b, (p if active[b] else 0):(p if active[b] else 0) + n] for b, p in enumerate(starts)]).contiguous().to(DEV)
            cache = c["cache"].clone()
            kv = cache.view(torch.int16).view(2, B, H, T_max, hs)
            for b in range(B):
                if not active[b]:
                    kv[:, b] = NAN
            for splits in SPLITS:
                got, lse = o.attn_extend(q, cache, B, T_max, n, bound, H, hs, scale, splits=splits, pos_rows=_i32(starts))
                forced = _resolved(splits, B, H, hs, n, bound + n)
                for b, p in enumerate(starts):
                    if active[b]:
                        want, want_lse = o.attn_extend(q, c["cache"], B, T_max, n, p, H, hs, scale, splits=forced)
                        assert torch.equal(_bits(got.view(B, n, Cc)[b]), _bits(want.view(B, n, Cc)[b])) and torch.equal(_bits(lse[b]), _bits(want_lse[b]))
                    else:
                        assert (got.view(B, n, Cc)[b].view(torch.int16) == 0).all(), (hs, splits, b, p)      # +0.0 in every element
                        assert (lse[b] == NEG_INF).all(), (hs, splits, b, p)


# =================================================================================================== rotate and store
def _gemm_plain(a, w, M, N, K):
    d = torch.empty((M, N), dtype=BF, device=DEV)
    g = L().GemmArgs(a.data_ptr(), w.data_ptr(), d.data_ptr(), None, None, M, N, K, K, K, N, 1, 1, L().EPI_NONE, 1.0, 0.0, 0, 0)
    L().check(L().lib().obte_gemm_bf16(C.byref(g), torch.cuda.current_stream().cuda_stream), "obte_gemm_bf16")
    return d


@pytest.mark.parametrize("hs", [64, 128])
@pytest.mark.parametrize("n", [3, 34])
def test_rope_store_chunk_is_the_uniform_epilogue_and_store(hs, n):
    from omnibiote_amd.model import rope_tables
    o = ops()
    B, H, T_max, marker = 4, 2, 77, 0x1234
    Cc = H * hs
    bound = T_max - n
    rope = rope_tables(R.cast_rope_table(R.rope_table(hs, T_max), BF).to(DEV))
    h1 = rnd(B * n, Cc, seed=hs).to(DEV)
    w = rnd(3 * Cc, Cc, seed=hs + 1, scale=Cc ** -0.5).to(DEV)
    plain = _gemm_plain(h1, w, B * n, 3 * Cc, Cc)

    def uniform(p):
        want = o.gemm(h1, w, B * n, 3 * Cc, Cc, epilogue=L().EPI_ROPE_QK, rope=(rope[0][p:], rope[1][p:], n, hs))
        mine = o.kv_cache_buffer(B, T_max, H, hs, DEV)
        mine.view(torch.int16).fill_(marker)
        o.kv_cache_store(want, B, n, H, hs, mine, T_max, p)
        return want, mine

    # equal positions: the bytes of qkv and of the whole cache
    for p in (0, 20, bound):
        qkv = plain.clone()
        cache = o.kv_cache_buffer(B, T_max, H, hs, DEV)
        cache.view(torch.int16).fill_(marker)
        o.kv_cache_rope_store_chunk(qkv, rope, _i32((p,) * B), bound, B, n, H, hs, cache, T_max)
        want, mine = uniform(p)
        assert torch.equal(qkv.view(torch.int16), want.view(torch.int16)), (hs, n, p)
        assert torch.equal(cache.view(torch.int16), mine.view(torch.int16)), (hs, n, p)
    # ragged positions, inactive rows among them: row by row, and every other cache position keeps the marker
    for pos in ((0, 37 if 37 <= bound else 7, bound, -1), (bound + 1, 5, T_max, -7)):
        qkv = plain.clone()
        cache = o.kv_cache_buffer(B, T_max, H, hs, DEV)
        cache.view(torch.int16).fill_(marker)
        o.kv_cache_rope_store_chunk(qkv, rope, _i32(pos), bound, B, n, H, hs, cache, T_max)
        K, V = [z.view(torch.int16) for z in _views(cache, B, H, T_max, hs)]
        touched = torch.zeros(B, T_max, dtype=torch.bool)
        for b, p in enumerate(pos):
            rows = slice(b * n, (b + 1) * n)
            if not 0 <= p <= bound:
                assert torch.equal(qkv[rows], plain[rows])                                   # neither rotated nor stored
                continue
            touched[b, p:p + n] = True
            want, mine = uniform(p)
            assert torch.equal(qkv[rows].view(torch.int16), want[rows].view(torch.int16)), (hs, n, b, p)
            assert not torch.equal(qkv[rows, :2 * Cc], plain[rows, :2 * Cc])                 # it did rotate
            wk, wv = [z.view(torch.int16) for z in _views(mine, B, H, T_max, hs)]
            assert torch.equal(K[b, :, p:p + n], wk[b, :, p:p + n]) and torch.equal(V[b, :, p:p + n], wv[b, :, p:p + n]), (hs, n, b, p)
        untouched = ~touched.to(DEV)
        assert (K.transpose(1, 2)[untouched] == marker).all() and (V.transpose(1, 2)[untouched] == marker).all()


# =================================================================================================== guard bands
@pytest.mark.parametrize("hs", [64, 128])
@pytest.mark.parametrize("n", [5, 33])
@pytest.mark.parametrize("splits", [1, 3])
def test_attn_extend_inside_guard_bands(hs, n, splits):
    """q (an ld larger than its row), the cache, o and lse 16 bytes into buffers that are NaN (inputs) or a marker (outputs) everywhere
    else: the plain call's bits, and every guard intact"""
    o = ops()
    B, H, T_max, pos = 2, 2, 200, 150
    Cc = H * hs
    scale = 8.0 / Cc
    qkv = rnd(B, T_max, 3 * Cc, seed=hs + n).to(DEV)
    cache = o.kv_cache_buffer(B, T_max, H, hs, DEV)
    o.kv_cache_store(qkv, B, T_max, H, hs, cache, T_max, 0)
    cache.view(torch.int16).view(2, B, H, T_max, hs)[:, :, :, pos + n:] = NAN
    q = qkv[:, pos:pos + n, :Cc].reshape(B * n, Cc).contiguous()
    plain = o.attn_extend(q, cache, B, T_max, n, pos, H, hs, scale, splits=splits)
    fq, hq = fenced(q, poison="nan", ld=Cc + 8)
    fc, hc = fenced(cache.view(-1, hs), poison="nan")
    fo, ho = fenced((B * n, Cc), dtype=BF, poison="mark")
    fl, hl = fenced((B * H, n), dtype=torch.float32, poison="mark")
    ws, hw = fenced((max(int(L().lib().obte_attn_extend_ws_bytes(B, H, hs, n, splits)), 16),), dtype=torch.uint8, poison="mark")
    got = o.attn_extend(fq, fc.view(-1), B, T_max, n, pos, H, hs, scale, splits=splits, q_ld=Cc + 8, ws=ws, out=fo, lse=fl.view(B, H, n))
    assert_same_bits(got[0], plain[0], "o")
    assert_same_bits(got[1], plain[1], "lse")
    assert_guards(hq, hc, ho, hl, hw)


# =================================================================================================== block
_blocks = {}


def _block_case(Cc, H):
    if (Cc, H) not in _blocks:
        c = _block_setup(Cc, H, 180)
        c["ref"] = R.block_forward(c["x"].float(), {k: v.float() for k, v in c["w"].items()}, c["pre"], c["cfg"], c["tab"], _add(_tril(180)))
        _blocks[(Cc, H)] = c
    return _blocks[(Cc, H)]


def _prefilled(c, Cc, H, T0=130, T=180):
    o = c["o"]
    cache = o.kv_cache_buffer(c["B"], T, H, Cc // H, DEV)
    cache.view(torch.int16).fill_(0x1234)
    o.block_prefill(c["x"][:, :T0].contiguous().to(DEV), c["params"], c["rope"], H, c["causal"](T0), cache, T)
    return cache


@pytest.mark.parametrize("Cc,H", [(128, 2), (256, 2)])
def test_block_extend_vs_oracle_and_block_infer(Cc, H):
    """prefill x[:, :130], then 7 more positions (B n = 14: the weight-streaming products) and 40 more (B n = 80: the tile path): every
    row against the oracle's causal block forward of the whole x (the block bar) and within twice that bar of block_infer's rows; out = x
    gives the same bits; the rows form with all positions equal is the uniform form."""
    T0, T = 130, 180
    c = _block_case(Cc, H)
    o, B = c["o"], c["B"]
    x = c["x"].to(DEV)
    full = o.block_infer(x, c["params"], c["rope"], H, c["causal"](T))
    cache, twin = _prefilled(c, Cc, H), _prefilled(c, Cc, H)
    at = T0
    for n in (7, 40):
        assert (B * n <= L().lib().obte_small_m_max()) == (n == 7)
        xt = x[:, at:at + n].contiguous()
        y = o.block_extend(xt, c["params"], c["rope"], H, cache, T, at)
        close(y, c["ref"][:, at:at + n], atol=3e-2, rtol=2.0 ** -6, what=f"block_extend C={Cc} positions {at}..{at + n - 1}")
        d = (y.float() - full[:, at:at + n].float()).abs()
        print(f"block_extend vs block_infer rows, C={Cc} n={n}: largest distance {d.max().item():.4g}")
        assert (d <= 2 * (3e-2 + 2.0 ** -6 * full[:, at:at + n].float().abs())).all()
        yr = o.block_extend(xt, c["params"], c["rope"], H, twin, T, at, pos_rows=_i32((at,) * B))
        assert torch.equal(yr, y), (Cc, n)
        assert torch.equal(cache.view(torch.int16), twin.view(torch.int16)), (Cc, n)
        alias = xt.clone()
        assert torch.equal(o.block_extend(alias, c["params"], c["rope"], H, cache, T, at, out=alias), y) and alias.data_ptr() != xt.data_ptr()
        at += n
    assert (_views(cache, B, H, T, Cc // H)[0][:, :, at:].view(torch.int16) == 0x1234).all()     # nothing beyond the last new position


@pytest.mark.parametrize("Cc,H", [(128, 2), (256, 2)])
def test_block_extend_rows_ragged_vs_oracle(Cc, H):
    T = 180
    c = _block_case(Cc, H)
    o, B = c["o"], c["B"]
    x = c["x"].to(DEV)
    cache = _prefilled(c, Cc, H)
    for starts, n in (((97, 130), 7), ((104, 137), 40)):
        xt = torch.stack([x[b, p:p + n] for b, p in enumerate(starts)]).contiguous()
        y = o.block_extend(xt, c["params"], c["rope"], H, cache, T, max(starts), pos_rows=_i32(starts))
        want = torch.stack([c["ref"][b, p:p + n] for b, p in enumerate(starts)])
        close(y, want, atol=3e-2, rtol=2.0 ** -6, what=f"block_extend rows C={Cc}, positions from {starts}, n={n}")


# =================================================================================================== model
CHUNKS = (1, 2, 5, 32, 33, 26)


@pytest.mark.parametrize("Cc", [256, 128])
def test_extend_teacher_forced_matches_the_oracle(Cc):
    from omnibiote_amd.model import KVCache
    c = _gen_case(Cc)
    m, idx = c["m"], c["ids"].to(DEV)
    for mode in ("all", "last"):
        cache = KVCache(m, 2)
        got, where = [m.prefill(idx[:, :100], cache).unsqueeze(1)], [99]
        at = 100
        for n in CHUNKS:
            out = m.extend(idx[:, at:at + n], cache, logits=mode)
            at += n
            assert cache.pos == at and cache.positions is None
            if mode == "all":
                assert out.shape == (2, n, c["cfg"].vocab_size)
                got.append(out); where += list(range(at - n, at))
            else:
                assert out.shape == (2, c["cfg"].vocab_size)
                got.append(out.unsqueeze(1)); where.append(at - 1)
        assert at == 199
        got = torch.cat(got, dim=1).float().cpu()
        assert torch.isfinite(got).all()
        if mode == "all":
            assert where == list(range(99, 199))
        d = (got - c["logits"][:, where]).abs()
        print(f"extend teacher-forced, C={Cc} logits={mode}: max {d.max().item():.4g} mean {d.mean().item():.4g}")
        assert d.max().item() <= 5e-3 and d.mean().item() <= 1e-3, (d.max().item(), d.mean().item())
    with pytest.raises(ValueError, match="positions are full"):
        m.extend(idx[:, :2], cache)


@pytest.mark.parametrize("Cc", [256, 128])
def test_extend_by_a_smaller_chunk_that_needs_the_larger_workspace(Cc):
    """The workspace is not monotone in n: at B * H = 4, n = 65 (three splits per tile) asks for fewer bytes than n = 64 (sixteen).  The
    buffer kept on the cache by the first call must not be taken for the second on the strength of its n."""
    from omnibiote_amd.model import KVCache
    c = _gen_case(Cc)
    m, idx, cfg = c["m"], c["ids"].to(DEV), c["cfg"]
    need = [int(L().lib().obte_block_extend_ws_bytes(2, n, cfg.n_embd, cfg.n_head)) for n in (65, 64)]
    assert 0 < need[0] < need[1], need                              # (what makes this the case to test)
    cache = KVCache(m, 2)
    m.prefill(idx[:, :60], cache)
    got = [m.extend(idx[:, 60:125], cache, logits="all")]
    assert need[0] <= cache.extend_ws.numel() < need[1]
    got.append(m.extend(idx[:, 125:189], cache, logits="all"))
    assert cache.pos == 189 and cache.extend_ws.numel() >= need[1]
    kept = cache.extend_ws
    cache.rewind(64)
    m.extend(idx[:, 125:190], cache)                                # 65 again: the larger buffer stays
    assert cache.extend_ws is kept and cache.pos == 190
    got = torch.cat(got, dim=1).float().cpu()
    d = (got - c["logits"][:, 60:189]).abs()
    print(f"extend by 65, then by 64, C={Cc}: max {d.max().item():.4g} mean {d.mean().item():.4g}")
    assert torch.isfinite(got).all() and d.max().item() <= 5e-3 and d.mean().item() <= 1e-3, (d.max().item(), d.mean().item())


def test_extend_by_one_is_decode_step():
    from omnibiote_amd.model import KVCache
    c = _gen_case(256)
    m, idx = c["m"], c["ids"].to(DEV)
    a, b = KVCache(m, 2), KVCache(m, 2)
    m.prefill(idx[:, :100], a); m.prefill(idx[:, :100], b)
    want = m.decode_step(idx[:, 100], b)
    assert torch.equal(m.extend(idx[:, 100:101], a), want) and a.pos == b.pos == 101
    want = m.decode_step(idx[:, 101], b)
    assert torch.equal(m.extend(idx[:, 101:102], a, logits="all"), want.unsqueeze(1))


@pytest.mark.parametrize("Cc", [256, 128])
def test_extend_rewind_extend(Cc):
    """extend by 8, rewind 5, extend by 5 OTHER tokens: the logits against the oracle of the sequence actually kept; the same on a
    cache whose layers held the NaN pattern first gives the same bits (nothing stale is read)."""
    from omnibiote_amd.model import KVCache
    c = _gen_case(Cc)
    cfg, m, ids = c["cfg"], c["m"], c["ids"]
    alt = (ids[:, 103:108] + 7) % (cfg.vocab_size - 4) + 4
    kept = torch.cat([ids[:, :103], alt], dim=1)
    wb = {k: v.to(BF).float() for k, v in R.hash_weights(cfg).items()}
    with torch.no_grad():
        want = R.model_forward(wb, cfg, kept, _add(_tril(108)), rope=R.cast_rope_table(R.rope_table(cfg.n_embd // cfg.n_head, 108), BF))
    runs = []
    for dirty in (False, True):
        cache = KVCache(m, 2)
        if dirty:
            for kv in cache.layers:
                kv.view(torch.int16).fill_(NAN)
        m.prefill(ids[:, :100].to(DEV), cache)
        first = m.extend(ids[:, 100:108].to(DEV), cache, logits="all")
        assert cache.pos == 108
        cache.rewind(5)
        assert cache.pos == 103
        second = m.extend(alt.to(DEV), cache, logits="all")
        assert cache.pos == 108
        runs.append((first, second))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    first, second = [t.float().cpu() for t in runs[0]]
    assert torch.isfinite(first).all() and torch.isfinite(second).all()
    for got, ref, what in ((first, c["logits"][:, 100:108], "the drafted block"), (second, want[:, 103:108], "after the rewind")):
        d = (got - ref).abs()
        print(f"extend / rewind / extend, C={Cc}, {what}: max {d.max().item():.4g} mean {d.mean().item():.4g}")
        assert d.max().item() <= 5e-3 and d.mean().item() <= 1e-3, (what, d.max().item(), d.mean().item())
    with pytest.raises(ValueError, match="fewer than one"):
        cache.rewind(108)


LENS = (97, 130)


def _ragged_prompt(c):
    idx = c["ids"][:, :max(LENS)].clone()
    idx[0, LENS[0]:] = 7                                           # padding
    return idx.to(DEV)


@pytest.mark.parametrize("Cc", [256, 128])
def test_extend_after_a_ragged_prefill(Cc):
    from omnibiote_amd.model import KVCache
    c = _gen_case(Cc)
    m, ids = c["m"], c["ids"]
    cache = KVCache(m, 2)
    m.prefill(_ragged_prompt(c), cache, lengths=LENS)
    tok = torch.stack([ids[b, n:n + 6] for b, n in enumerate(LENS)]).to(DEV)
    got = m.extend(tok, cache, logits="all").float().cpu()
    assert cache.positions.dtype == torch.int32 and cache.positions.tolist() == [n + 6 for n in LENS] and cache.max_pos == cache.pos == max(LENS) + 6
    want = torch.stack([c["logits"][b, n:n + 6] for b, n in enumerate(LENS)])
    d = (got - want).abs()
    print(f"extend after a ragged prefill, C={Cc}: max {d.max().item():.4g} mean {d.mean().item():.4g}")
    assert torch.isfinite(got).all() and d.max().item() <= 5e-3 and d.mean().item() <= 1e-3, (d.max().item(), d.mean().item())
    cache.park(_i32((0, 1)) == 0)                                                          # park row 0
    m.extend(tok[:, :3], cache)
    assert cache.positions.tolist() == [-1, LENS[1] + 9] and cache.max_pos == max(LENS) + 9
    cache.rewind(2)
    assert cache.positions.tolist() == [-1, LENS[1] + 7] and cache.max_pos == cache.pos == max(LENS) + 7


# =================================================================================================== chunked prefill
@pytest.mark.parametrize("Cc", [256, 128])
def test_chunked_prefill_matches_the_oracle(Cc):
    from omnibiote_amd.model import KVCache
    c = _gen_case(Cc)
    m, idx = c["m"], c["ids"].to(DEV)
    plain_cache = KVCache(m, 2)
    plain = m.prefill(idx[:, :130], plain_cache)
    for chunk in (130, 500):
        cache = KVCache(m, 2)
        assert torch.equal(m.prefill(idx[:, :130], cache, chunk=chunk), plain) and cache.pos == 130 and cache.positions is None
        for a, b in zip(cache.layers, plain_cache.layers):
            assert torch.equal(a.view(2, 2, 2, 200, -1)[:, :, :, :130], b.view(2, 2, 2, 200, -1)[:, :, :, :130])
    for chunk in (32, 50):
        cache = KVCache(m, 2)
        got = [m.prefill(idx[:, :130], cache, chunk=chunk)]
        assert cache.pos == 130 and cache.positions is None and cache.max_pos == 0
        for t in range(130, 140):
            got.append(m.decode_step(idx[:, t], cache))
        got = torch.stack(got, dim=1).float().cpu()
        d = (got - c["logits"][:, 129:140]).abs()
        print(f"prefill(chunk={chunk}) + 10 decode steps, C={Cc}: max {d.max().item():.4g} mean {d.mean().item():.4g}")
        assert torch.isfinite(got).all() and d.max().item() <= 5e-3 and d.mean().item() <= 1e-3, (chunk, d.max().item(), d.mean().item())
    # right-padded prompts
    want_cache = KVCache(m, 2)
    m.prefill(_ragged_prompt(c), want_cache, lengths=LENS)
    cache = KVCache(m, 2)
    got = m.prefill(_ragged_prompt(c), cache, lengths=LENS, chunk=32).float().cpu()
    assert cache.positions.dtype == torch.int32 and torch.equal(cache.positions, want_cache.positions)
    assert cache.max_pos == want_cache.max_pos == cache.pos == want_cache.pos
    want = torch.stack([c["logits"][b, n - 1] for b, n in enumerate(LENS)])
    d = (got - want).abs()
    assert d.max().item() <= 5e-3 and d.mean().item() <= 1e-3, (d.max().item(), d.mean().item())


@pytest.mark.parametrize("Cc", [256, 128])
def test_chunked_prefill_whose_last_chunk_needs_more_workspace(Cc):
    """chunk = 66 on the 130-token prompt: chunks of 66 and 64, and the shorter one asks for the larger workspace"""
    from omnibiote_amd.model import KVCache
    c = _gen_case(Cc)
    m, idx, cfg = c["m"], c["ids"].to(DEV), c["cfg"]
    need = [int(L().lib().obte_block_extend_ws_bytes(2, n, cfg.n_embd, cfg.n_head)) for n in (66, 64)]
    assert 0 < need[0] < need[1], need
    cache = KVCache(m, 2)
    got = [m.prefill(idx[:, :130], cache, chunk=66)]
    assert cache.pos == 130 and cache.positions is None and cache.extend_ws.numel() >= need[1]
    for t in range(130, 133):
        got.append(m.decode_step(idx[:, t], cache))
    got = torch.stack(got, dim=1).float().cpu()
    d = (got - c["logits"][:, 129:133]).abs()
    print(f"prefill(chunk=66) + 3 decode steps, C={Cc}: max {d.max().item():.4g} mean {d.mean().item():.4g}")
    assert torch.isfinite(got).all() and d.max().item() <= 5e-3 and d.mean().item() <= 1e-3, (d.max().item(), d.mean().item())


def test_chunked_prefill_across_the_second_query_tile_boundary():
    """chunk = 257 on a 513-token prompt (one layer, B * H = 4): chunks of 257 and 256, nine partial units against sixteen"""
    from omnibiote_amd.model import KVCache
    cfg = R.RefConfig(block_size=1024, vocab_size=512, n_layer=1, n_head=2, n_embd=256)
    m = _model(cfg, R.hash_weights(cfg), True)
    idx = torch.from_numpy(np.random.default_rng(1).integers(4, cfg.vocab_size, size=(2, 513)).astype(np.int64)).to(DEV)
    need = [int(L().lib().obte_block_extend_ws_bytes(2, n, 256, 2)) for n in (257, 256)]
    assert 0 < need[0] < need[1], need
    plain_cache, cache = KVCache(m, 2), KVCache(m, 2)
    plain = m.prefill(idx, plain_cache)
    got = m.prefill(idx, cache, chunk=257)
    assert cache.pos == 513 and cache.extend_ws.numel() >= need[1]
    d = (got.float() - plain.float()).abs()
    assert torch.isfinite(got).all() and d.max().item() <= 1e-2 and d.mean().item() <= 2e-3      # both within the model bar of the same exact logits


def test_chunked_prefill_peak_memory():
    """one layer, C = 256, B = 2, T0 = 1024: the unchunked call holds about 8 units of B T0 C bf16 (x and the 7 of its workspace), the
    chunked one about 1 unit plus the attention partials — at most half, measured."""
    from omnibiote_amd.model import KVCache
    cfg = R.RefConfig(block_size=1024, vocab_size=512, n_layer=1, n_head=2, n_embd=256)
    m = _model(cfg, R.hash_weights(cfg), True)
    idx = torch.from_numpy(np.random.default_rng(0).integers(4, cfg.vocab_size, size=(2, 1024)).astype(np.int64)).to(DEV)
    peaks, outs = {}, {}
    for chunk in (None, 128):
        cache = KVCache(m, 2)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        outs[chunk] = m.prefill(idx, cache, chunk=chunk)
        torch.cuda.synchronize()
        peaks[chunk] = torch.cuda.max_memory_allocated() - before
        assert cache.pos == 1024
        del cache
    print(f"prefill peak above the level before the call: unchunked {peaks[None]} bytes, chunk=128 {peaks[128]} bytes")
    assert peaks[128] * 2 <= peaks[None], peaks
    d = (outs[128].float() - outs[None].float()).abs()
    assert d.max().item() <= 1e-2 and d.mean().item() <= 2e-3        # both within the model bar of the same exact logits
