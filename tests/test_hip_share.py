"""Prompt pages shared between the rows of a paged cache, on the GPU (include/omnibiote_hip_paged_extend.h): obte_attn_extend_paged bit for bit
against obte_attn_extend's rows form on the same vectors, missing pages against float64 softmax over the keys that are left, the chunk's
rotate-and-store through the table inside guard bands against the rectangular store's bits, the block bit for bit against
obte_block_extend, then OmniBioTA.prefill(shared_pages=) against the oracle and generate_many(share_prefix=True) against the model's own
causal forward.  Shapes: tests/test_hip_paged.py's — B = 3, H = 2, T = 256, 16 pages in seeded random order, every page no row holds
filled with bf16 NaN; the model tests use the small generation fixtures (block size 200: at most 4 pages per row)."""
import pytest
import torch

from fenced import MARK, assert_guards, fenced
from omnibiote_amd.paged import paged_gather_reference, paged_scatter_reference
from test_hip_generate import _block_setup, _decode_case, _gen_case, _views, ops
from test_hip_ops import BF, DEV, close, rnd
from test_hip_paged import _gaps

pytestmark = pytest.mark.gpu

B, H, T, N_PAGES = 3, 2, 256, 16
SPLITS = (0, 1, 2, 7, 32)
NEG_INF = float("-inf")


def _i32(values):
    return torch.tensor(list(values), dtype=torch.int32, device=DEV)


_pools = {}


def _paged_case(hs):
    """_decode_case's rectangular cache of T positions, and the same vectors in a pool whose 16 pages are in random order, every page
    no row holds filled with bf16 NaN (computed once, never modified)"""
    if hs not in _pools:
        c = _decode_case(B, H, hs, T)
        K, V = _views(c["cache"], B, H, T, hs)
        table = torch.randperm(N_PAGES, generator=torch.Generator().manual_seed(hs + 1))[:B * T // 64].view(B, T // 64).to(torch.int32).to(DEV)
        pool = paged_scatter_reference(K, V, table, N_PAGES)
        assert int(torch.isnan(pool.view(2, N_PAGES, -1)).all(dim=-1).sum()) == 2 * (N_PAGES - B * T // 64)
        _pools[hs] = dict(c=c, table=table, pool=pool)
    return _pools[hs]


def _chunk(c, starts, n):
    """packed [B, n, 3C]: row b holds the rows of positions starts[b] .. starts[b] + n - 1 (from position 0 where the start is no position)"""
    return torch.stack([c["qkv"][b, (p if 0 <= p <= T - n else 0):(p if 0 <= p <= T - n else 0) + n] for b, p in enumerate(starts)]).contiguous().to(DEV)


# =================================================================================================== attention
@pytest.mark.parametrize("hs", [64, 128])
def test_attn_extend_paged_is_attn_extend_rows_bit_for_bit(hs):
    """starts on, before and behind the page edges, chunks of one query, of one tile and of two, every split count (7 and 32 leave splits
    empty): the rectangle's bits, row by row"""
    o = ops()
    p = _paged_case(hs)
    scale = 8.0 / (H * hs)
    for starts in ((0, 1, 63), (64, 65, 128), (191, 128, 0)):
        bound = max(starts)
        for n in (1, 2, 32, 33, 64):
            assert bound + n <= T
            q, rows = _chunk(p["c"], starts, n), _i32(starts)
            for splits in SPLITS:
                want, want_lse = o.attn_extend(q, p["c"]["cache"], B, T, n, bound, H, hs, scale, splits=splits, pos_rows=rows)
                got, lse = o.attn_extend_paged(q, p["pool"], N_PAGES, p["table"], B, n, bound, H, hs, scale, rows, splits=splits)
                assert torch.isfinite(got).all() and torch.isfinite(lse).all(), (hs, starts, n, splits)
                assert torch.equal(got, want) and torch.equal(lse, want_lse), (hs, starts, n, splits)


@pytest.mark.parametrize("hs", [64, 128])
def test_attn_extend_paged_missing_pages(hs):
    """An entry of -1, of n_pages or of 2^30 in the middle of a row removes exactly those 64 keys — the chunk's own among them: float64
    softmax over the keys that are left, at the bars of tests/test_hip_extend.py for this kernel (o atol 6e-3, lse atol 2e-3 / rtol 1e-3).
    A row with every entry missing, or with a start outside [0, pos], gives exact zeros and lse = -inf, and the row beside keeps its bits."""
    o = ops()
    p = _paged_case(hs)
    c = p["c"]
    Cc = H * hs
    scale = 8.0 / Cc
    starts, n = (100, 64, 191), 33
    bound = max(starts)
    gone = ((0, 1, -1), (1, 0, N_PAGES), (2, 2, 2 ** 30))               # (row, entry, what stands there)
    table = p["table"].clone()
    keep = torch.ones(B, T, dtype=torch.bool)
    for b, j, v in gone:
        table[b, j] = v
        keep[b, 64 * j:64 * j + 64] = False
    q, rows = _chunk(c, starts, n), _i32(starts)
    ref_o, ref_lse = [], []
    for b, s0 in enumerate(starts):
        qb, kb, vb = c["q"][b, :, s0:s0 + n].double(), c["k"][b, :, :s0 + n].double(), c["v"][b, :, :s0 + n].double()
        s = (qb @ kb.transpose(-2, -1)) * scale                          # [H, n, s0 + n]
        seen = keep[b, :s0 + n].view(1, 1, -1) & (torch.arange(s0 + n).view(1, 1, -1) <= (s0 + torch.arange(n)).view(1, n, 1))
        assert seen.any(dim=-1).all()                                   # (every query keeps a key)
        s = s.masked_fill(~seen, NEG_INF)
        ref_o.append((torch.softmax(s, dim=-1) @ vb).transpose(0, 1).reshape(n, Cc))
        ref_lse.append(torch.logsumexp(s, dim=-1))
    ref_o, ref_lse = torch.cat(ref_o), torch.stack(ref_lse)
    for splits in SPLITS:
        got, lse = o.attn_extend_paged(q, p["pool"], N_PAGES, table, B, n, bound, H, hs, scale, rows, splits=splits)
        close(got, ref_o, atol=6e-3, what=f"attn_extend_paged, missing pages, hs={hs} splits={splits}")
        close(lse, ref_lse, atol=2e-3, rtol=1e-3, what=f"lse, missing pages, hs={hs} splits={splits}")
    # row 0: no page at all; row 1: a start outside [0, pos]; row 2 stays and keeps its bits
    table = p["table"].clone()
    table[0] = _i32((-1, N_PAGES, 2 ** 30, -7))
    for p1 in (-1, bound + 1, 2 ** 31 - 1):
        starts = (100, p1, 191)
        q, rows = _chunk(c, starts, n), _i32(starts)
        for splits in (0, 1, 3):
            got, lse = o.attn_extend_paged(q, p["pool"], N_PAGES, table, B, n, bound, H, hs, scale, rows, splits=splits)
            want, want_lse = o.attn_extend(q, c["cache"], B, T, n, bound, H, hs, scale, splits=splits, pos_rows=rows)
            for b in (0, 1):
                assert (got.view(B, n, Cc)[b].view(torch.int16) == 0).all() and (lse[b] == NEG_INF).all(), (hs, p1, splits, b)
            assert torch.equal(got.view(B, n, Cc)[2], want.view(B, n, Cc)[2]) and torch.equal(lse[2], want_lse[2]), (hs, p1, splits)


# =================================================================================================== the store
@pytest.mark.parametrize("hs", [64, 128])
def test_kv_paged_rope_store_chunk_is_the_rectangular_chunk_store(hs):
    """10 positions per row from 60 (across a page edge), 64, 100 (a row whose other entries are no pages), a parked row, and 120 (its
    positions 128 and 129 have no page): qkv in place and the stored vectors have kv_cache_rope_store_chunk's bits, a position without a
    page is rotated and not stored, and every other byte of the pool and the guards still holds the marker"""
    import omnibiote_ref as R
    from omnibiote_amd.model import rope_tables
    o = ops()
    Bn, n, Tt, C_ = 5, 10, 192, H * hs
    pos, bound = (60, 64, 100, -1, 120), 130
    rope = rope_tables(R.cast_rope_table(R.rope_table(hs, Tt), BF).to(DEV))
    plain = rnd(Bn * n, 3 * C_, seed=hs + 13).to(DEV)
    rect = o.kv_cache_buffer(Bn, Tt, H, hs, DEV)
    rect.view(torch.int16).fill_(MARK[2])
    want_qkv = plain.clone()
    o.kv_cache_rope_store_chunk(want_qkv, rope, _i32(pos), bound, Bn, n, H, hs, rect, Tt)
    size = o.kv_paged_buffer(N_PAGES, H, hs, DEV).numel()
    pool, fence = fenced((size,), BF, poison="mark")
    table = torch.tensor([[3, 12, -1], [8, 0, -1], [-1, 11, N_PAGES], [6, 7, 5], [4, 9, 2 ** 30]], dtype=torch.int32).to(DEV)
    qkv = plain.clone()
    o.kv_paged_rope_store_chunk(qkv, rope, _i32(pos), bound, Bn, n, H, hs, pool, N_PAGES, table)
    assert_guards(fence)
    assert torch.equal(qkv.view(torch.int16), want_qkv.view(torch.int16))
    q3 = qkv.view(Bn, n, 3 * C_)
    assert torch.equal(q3[3], plain.view(Bn, n, 3 * C_)[3])             # parked: untouched
    assert not torch.equal(q3[4, 8:, :2 * C_], plain.view(Bn, n, 3 * C_)[4, 8:, :2 * C_])   # no page: rotated all the same
    mark = torch.tensor(MARK[2], dtype=torch.int16).view(BF).item()
    gk, gv = paged_gather_reference(pool, table, N_PAGES, H, hs, fill=mark)
    wrote = torch.zeros(Bn, Tt, dtype=torch.bool)
    for b, s0 in enumerate(pos):
        if s0 >= 0:
            wrote[b, s0:s0 + n] = True
    wrote[4, 128:] = False                                              # (entry 2 of row 4 is no page)
    wrote = wrote.to(DEV)
    wk, wv = _views(rect, Bn, H, Tt, hs)
    for got, want in ((gk, wk), (gv, wv)):
        got, want = got.view(torch.int16).transpose(1, 2), want.view(torch.int16).transpose(1, 2)   # [B, T, H, hs]
        assert torch.equal(got[wrote], want[wrote]) and (want[wrote] != MARK[2]).any(), hs
        assert (got[~wrote] == MARK[2]).all(), hs
    kv = pool.view(torch.int16).view(2, N_PAGES, H, 64, hs)
    unnamed = torch.ones(N_PAGES, dtype=torch.bool)
    unnamed[[3, 12, 8, 0, 11, 6, 7, 5, 4, 9]] = False
    assert (kv[:, unnamed.to(DEV)] == MARK[2]).all() and (kv[:, [6, 7, 5]] == MARK[2]).all(), hs   # the parked row's pages too


# =================================================================================================== the block
@pytest.mark.parametrize("C_", [256, 128])
def test_block_extend_paged_is_block_extend_rows_bit_for_bit(C_):
    """ragged starts (64, 128, 0), n = 37: y and what the pool holds afterwards are obte_block_extend's rows form on the gathered rectangle"""
    c = _block_setup(C_, H, 200)
    o, hs, Tt, n = c["o"], C_ // H, 192, 37
    starts = (64, 128, 0)
    bound = max(starts)
    rect = o.kv_cache_buffer(B, Tt, H, hs, DEV)
    o.kv_cache_store(rnd(B, Tt, 3 * C_, seed=C_ + 5).to(DEV), B, Tt, H, hs, rect, Tt, 0)
    table = torch.randperm(N_PAGES, generator=torch.Generator().manual_seed(C_))[:B * 3].view(B, 3).to(torch.int32).to(DEV)
    K, V = _views(rect, B, H, Tt, hs)
    pool = paged_scatter_reference(K, V, table, N_PAGES)
    x = rnd(B, n, C_, seed=C_ + 6).to(DEV)
    want = o.block_extend(x, c["params"], c["rope"], H, rect, Tt, bound, pos_rows=_i32(starts))
    got = o.block_extend_paged(x, c["params"], c["rope"], H, pool, N_PAGES, table, bound, _i32(starts))
    assert torch.isfinite(got).all() and torch.equal(got, want), C_
    gk, gv = paged_gather_reference(pool, table, N_PAGES, H, hs)
    assert torch.equal(gk.view(torch.int16), K.view(torch.int16)) and torch.equal(gv.view(torch.int16), V.view(torch.int16)), C_
    alias = x.clone()
    assert torch.equal(o.block_extend_paged(alias, c["params"], c["rope"], H, pool, N_PAGES, table, bound, _i32(starts), out=alias), want)


# =================================================================================================== the model
def _bar(got, want, what):
    d = (got.float().cpu() - want).abs()
    print(f"{what}: max {d.max().item():.4g} mean {d.mean().item():.4g}")
    assert torch.isfinite(got).all()
    assert d.max().item() <= 5e-3 and d.mean().item() <= 1e-3, (what, d.max().item(), d.mean().item())


@pytest.mark.parametrize("C_", [256, 128])
def test_prefill_with_shared_pages_matches_the_oracle(C_):
    """Row 0 holds ids[0, :150]; row 1 takes its first two pages and computes positions 128 .. 189 of ids[0, :190] against them: the
    logits of position 189 and, after row 0 has been released, of 8 teacher-forced decode steps at the project's bar against the oracle
    (max 5e-3, mean 1e-3: tests/test_hip_extend.py) — the shared pages survive their first owner."""
    from omnibiote_amd.model import PagedKVCache
    c = _gen_case(C_)
    m, ids = c["m"], c["ids"].to(DEV)
    order = torch.randperm(8, generator=torch.Generator().manual_seed(C_)).tolist()
    cache = PagedKVCache(m, 2, 8, free_order=order)
    m.prefill(ids[0:1, :150], cache, rows=[0])
    first = list(cache.book.row_pages[0])
    assert first == order[:3] and cache.pages_in_use == 3
    logits = m.prefill(ids[0:1, :190], cache, rows=[1], shared_pages=[first[:2]])
    assert cache.table.tolist() == [first + [-1], first[:2] + [order[3], -1]]
    assert [cache.book.refs[p] for p in order[:4]] == [2, 2, 1, 1] and cache.positions.tolist() == [150, 190]
    assert cache.pages_in_use == 4                                      # unshared: 3 + 3; the two shared pages are held once
    _bar(logits[0], c["logits"][0, 189], f"prefill(shared_pages=), C={C_}, position 189")
    cache.release(0)
    assert cache.pages_in_use == 3 and cache.book.free[-1] == first[2] and cache.positions.tolist() == [-1, 190]
    got = []
    for t in range(190, 198):
        got.append(m.decode_step(torch.stack([ids[0, 0], ids[0, t]]), cache)[1])
    _bar(torch.stack(got), c["logits"][0, 190:198], f"decode behind shared pages, C={C_}, positions 190..197")
    cache.release(1)
    assert cache.pages_in_use == 0 and sorted(cache.book.free) == list(range(8)) and cache.book.refs == [0] * 8


@pytest.mark.parametrize("C_", [256, 128])
def test_prefill_with_shared_pages_splits_what_does_not_fit_one_call(C_):
    """block size 200: a start of 128 with a tail of 10 beside a start of 64 with a tail of 130 — 128 + 130 positions are more than the
    RoPE tables hold, so the host makes two calls, sorted by start; both rows' logits meet the oracle"""
    from omnibiote_amd.model import PagedKVCache
    c = _gen_case(C_)
    m, ids = c["m"], c["ids"].to(DEV)
    assert m._tail_calls([128, 64], [10, 130], 200) == [[1], [0]] and m._tail_calls([128, 64], [10, 72], 200) == [[1, 0]]
    assert m._tail_calls([64, 64, 128, 0], [136, 1, 72, 200], 200) == [[3], [0, 1], [2]]
    cache = PagedKVCache(m, 3, 12)
    m.prefill(ids[0:1, :150], cache, rows=[0])
    first = list(cache.book.row_pages[0])
    idx = ids[0:1, :194].repeat(2, 1)
    idx[0, 138:] = 9                                                    # padding
    logits = m.prefill(idx, cache, lengths=[138, 194], rows=[1, 2], shared_pages=[first[:2], first[:1]])
    assert cache.positions.tolist() == [150, 138, 194] and cache.pages_in_use == 3 + 1 + 3
    assert cache.book.refs[first[0]] == 3 and cache.book.refs[first[1]] == 2
    _bar(logits, torch.stack([c["logits"][0, 137], c["logits"][0, 193]]), f"prefill(shared_pages=) in two calls, C={C_}")
    # a round of one plain row and one sharer: the plain row through the prefill kernels
    cache.release(1), cache.release(2)
    logits = m.prefill(torch.stack([ids[1, :70], ids[0, :70]]), cache, rows=[1, 2], shared_pages=[[], first[:1]])
    assert cache.pages_in_use == 3 + 2 + 1
    _bar(logits, torch.stack([c["logits"][1, 69], c["logits"][0, 69]]), f"prefill(shared_pages=), a plain row beside a sharer, C={C_}")


def _prompts(c, tails):
    """two 128-token prefixes (the fixture's two rows) in turn, each followed by a tail of its own"""
    ids = c["ids"]
    return [torch.cat([ids[i % 2, :128], ids[(i + 1) % 2, 130 + i:130 + i + n]]).to(DEV) for i, n in enumerate(tails)]


@pytest.mark.parametrize("C_", [256, 128])
def test_generate_many_share_prefix(C_):
    """Without a common full page share_prefix=True runs the same path: the same tokens.  With two 128-token prefixes under six requests
    and batch = 3: every output starts with its prompt and has the right length, positions were shared and the two counts add up to the
    prompts' lengths, two runs agree, and in one causal forward over each finished sequence every generated token's logit lies within
    2 x 5e-3 of its position's maximum — the shared path and the full forward are each within 5e-3 of the oracle.  Two requests with one
    prefix admitted in the same round share it too."""
    c = _gen_case(C_)
    m, ids = c["m"], c["ids"]
    n = 12
    apart = [ids[i % 2, 3 * i:3 * i + a].clone().to(DEV) for i, a in enumerate((130, 5, 64, 97, 150))]
    stats = {}
    want = m.generate_many(apart, n, batch=2, top_k=1)
    got = m.generate_many(apart, n, batch=2, top_k=1, share_prefix=True, stats=stats)
    assert all(torch.equal(a, b) for a, b in zip(got, want)) and stats["shared_positions"] == 0
    assert stats["prefill_positions"] == 130 + 5 + 64 + 97 + 150 and stats["decode_steps"] > 0 and stats["peak_pages"] > 0

    tails = (5, 40, 17, 33, 1, 26)
    prompts = _prompts(c, tails)
    runs = []
    for _ in range(2):
        stats = {}
        runs.append(m.generate_many(prompts, n, batch=3, top_k=1, share_prefix=True, stats=stats))
        print(f"generate_many(share_prefix=True), C={C_}: {stats}")
        assert stats["shared_positions"] > 0 and stats["shared_positions"] % 64 == 0
        assert stats["prefill_positions"] + stats["shared_positions"] == sum(p.numel() for p in prompts)
    plain = {}
    m.generate_many(prompts, n, batch=3, top_k=1, stats=plain)
    assert plain["shared_positions"] == 0 and plain["prefill_positions"] == sum(p.numel() for p in prompts) and plain["peak_pages"] >= stats["peak_pages"]
    for r, (a, b_) in enumerate(zip(*runs)):
        assert torch.equal(a, b_), (C_, r)
        assert a.dtype == torch.int64 and a.numel() == prompts[r].numel() + n and torch.equal(a[:prompts[r].numel()], prompts[r]), (C_, r)
        gap = _gaps(m, a, prompts[r].numel())
        print(f"generate_many(share_prefix=True), C={C_}, request {r}: largest gap {gap.max().item():.4g}")
        assert (gap <= 2 * 5e-3).all(), (C_, r, gap.max().item())
    # the same round: both admitted at once, the second waits for the first one's prefill call and takes its two pages
    stats = {}
    pair = m.generate_many(prompts[0:3:2], n, batch=2, top_k=1, share_prefix=True, stats=stats)
    assert stats["shared_positions"] == 128 and stats["prefill_positions"] == prompts[0].numel() + prompts[2].numel() - 128
    for a, p in zip(pair, prompts[0:3:2]):
        assert a.numel() == p.numel() + n and torch.equal(a[:p.numel()], p)
        gap = _gaps(m, a, p.numel())
        print(f"generate_many(share_prefix=True), C={C_}, same round: largest gap {gap.max().item():.4g}")
        assert (gap <= 2 * 5e-3).all(), (C_, gap.max().item())
