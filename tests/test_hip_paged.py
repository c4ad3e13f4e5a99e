"""The paged key/value cache on the GPU (include/omnibiote_hip_paged.h): obte_attn_decode_paged bit for bit against obte_attn_decode_rows on
the same vectors, missing pages against float64 softmax over the keys that are left, the two stores inside guard bands against the
rectangular stores' bits, the block and model paths (prefill, decode_step, release, prefill(rows=)) bit for bit against a KVCache, and
OmniBioTA.generate_many against generate and as a queue.  Shapes: the small generation fixtures of tests/test_hip_generate.py (block
size 200: at most 4 pages per row); the kernel tests use B = 3, H = 2."""
import pytest
import torch

from fenced import MARK, assert_guards, fenced
from omnibiote_amd.paged import paged_gather_reference, paged_scatter_reference, pages_for
from test_hip_generate import _decode_case, _gen_case, _views, ops
from test_hip_ops import BF, DEV, close, rnd

pytestmark = pytest.mark.gpu

B, H, T, N_PAGES = 3, 2, 256, 16        # 4 pages per row, 12 of the pool's 16 in use
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
        table = torch.randperm(N_PAGES, generator=torch.Generator().manual_seed(hs))[:B * T // 64].view(B, T // 64).to(torch.int32).to(DEV)
        pool = paged_scatter_reference(K, V, table, N_PAGES)
        assert int(torch.isnan(pool.view(2, N_PAGES, -1)).all(dim=-1).sum()) == 2 * (N_PAGES - B * T // 64)
        _pools[hs] = dict(c=c, table=table, pool=pool)
    return _pools[hs]


def _queries(c, counts):
    """packed [B, 3C]: row b is the row of position counts[b] - 1; position 0 where the count is not a valid one"""
    return torch.stack([c["qkv"][b, n - 1 if 1 <= n <= T else 0] for b, n in enumerate(counts)]).contiguous().to(DEV)


# =================================================================================================== one-query attention
@pytest.mark.parametrize("hs", [64, 128])
def test_attn_decode_paged_is_attn_decode_rows_bit_for_bit(hs):
    """64 / 65 / 128 / 129 are the page and split edges, 1 the smallest row; 3 and 5 splits leave splits empty"""
    o = ops()
    p = _paged_case(hs)
    scale = 8.0 / (H * hs)
    for counts in ((1, 64, 65), (130, 191, 128), (200, 63, 129)):
        q, n_dev = _queries(p["c"], counts), _i32(counts)
        for splits in (1, 2, 3, 5, 0):
            want, want_lse = o.attn_decode_rows(q, p["c"]["cache"], B, T, n_dev, T, H, hs, scale, splits=splits)
            got, lse = o.attn_decode_paged(q, p["pool"], N_PAGES, p["table"], B, n_dev, T, H, hs, scale, splits=splits)
            assert torch.isfinite(got).all() and torch.isfinite(lse).all(), (hs, counts, splits)
            assert torch.equal(got, want) and torch.equal(lse, want_lse), (hs, counts, splits)


@pytest.mark.parametrize("hs", [64, 128])
def test_attn_decode_paged_missing_pages(hs):
    """An entry of -1, of n_pages or of 2^30 in the middle of a row removes exactly those 64 keys: float64 softmax over the keys that are
    left, at the bars of tests/test_hip_generate_rows.py for this kernel.  A row with every entry missing, or with a count outside
    [1, max_keys], gives exact zeros and lse = -inf."""
    o = ops()
    p = _paged_case(hs)
    c = p["c"]
    scale = 8.0 / (H * hs)
    counts = (200, 130, 256)
    gone = ((0, 1, -1), (1, 0, N_PAGES), (2, 2, 2 ** 30))               # (row, entry, what stands there)
    table = p["table"].clone()
    keep = torch.ones(B, T, dtype=torch.bool)
    for b, j, v in gone:
        table[b, j] = v
        keep[b, 64 * j:64 * j + 64] = False
    q, n_dev = _queries(c, counts), _i32(counts)
    ref_o, ref_lse = [], []
    for b, n in enumerate(counts):
        qb, kb, vb = c["q"][b, :, n - 1:n].double(), c["k"][b, :, :n].double(), c["v"][b, :, :n].double()
        s = (qb @ kb.transpose(-2, -1)) * scale                          # [H, 1, n]
        s = s.masked_fill(~keep[b, :n].view(1, 1, n), NEG_INF)
        ref_o.append((torch.softmax(s, dim=-1) @ vb).reshape(-1))
        ref_lse.append(torch.logsumexp(s, dim=-1).reshape(-1))
    ref_o, ref_lse = torch.stack(ref_o), torch.stack(ref_lse)
    for splits in (0, 1, 2, 3, 5):
        got, lse = o.attn_decode_paged(q, p["pool"], N_PAGES, table, B, n_dev, T, H, hs, scale, splits=splits)
        close(got, ref_o, atol=6e-3, what=f"attn_decode_paged, missing pages, hs={hs} splits={splits}")
        close(lse, ref_lse, atol=2e-3, rtol=1e-3, what=f"lse, missing pages, hs={hs} splits={splits}")
    # row 0: no page at all; row 1: counts outside [1, max_keys]; row 2 stays and keeps its bits
    table = p["table"].clone()
    table[0] = _i32((-1, N_PAGES, 2 ** 30, -7))
    max_keys = 200
    for n1 in (0, -1, max_keys + 1, 2 ** 31 - 1):
        counts = (200, n1, 129)
        q, n_dev = _queries(c, counts), _i32(counts)
        for splits in (0, 1, 3):
            got, lse = o.attn_decode_paged(q, p["pool"], N_PAGES, table, B, n_dev, max_keys, H, hs, scale, splits=splits)
            want, want_lse = o.attn_decode_rows(q, c["cache"], B, T, n_dev, max_keys, H, hs, scale, splits=splits)
            for b in (0, 1):
                assert (got[b].view(torch.int16) == 0).all() and (lse[b] == NEG_INF).all(), (hs, n1, splits, b)
            assert torch.equal(got[2], want[2]) and torch.equal(lse[2], want_lse[2]), (hs, n1, splits)


# =================================================================================================== the stores
def _fenced_pool(o, hs):
    """a pool inside guard bands, payload and guards holding the marker"""
    n = o.kv_paged_buffer(N_PAGES, H, hs, DEV).numel()
    view, h = fenced((n,), BF, poison="mark")
    assert (view.view(torch.int16) == MARK[2]).all()
    return view, h


@pytest.mark.parametrize("hs", [64, 128])
def test_kv_paged_store_is_kv_cache_store_through_the_table(hs):
    """t = 130 over rows with pages for 130, 64 and 0 positions: the positions that have a page hold the rectangular store's bits, every
    other byte of the pool and the guards still holds the marker"""
    o = ops()
    t, C_ = 130, H * hs
    qkv = rnd(B, t, 3 * C_, seed=hs + 7).to(DEV)
    rect = o.kv_cache_buffer(B, T, H, hs, DEV)
    rect.view(torch.int16).fill_(MARK[2])
    o.kv_cache_store(qkv, B, t, H, hs, rect, T, 0)
    pool, fence = _fenced_pool(o, hs)
    table = torch.full((B, 3), -1, dtype=torch.int32)
    table[0] = torch.tensor([9, 2, 14])
    table[1, 0] = 5
    table[2] = torch.tensor([N_PAGES, -1, 2 ** 30])                     # (no page of the pool)
    table = table.to(DEV)
    o.kv_paged_store(qkv, B, t, H, hs, pool, N_PAGES, table)
    assert_guards(fence)
    mark = torch.tensor(MARK[2], dtype=torch.int16).view(BF).item()
    gk, gv = paged_gather_reference(pool, table, N_PAGES, H, hs, fill=mark)
    has = torch.zeros(B, 192, dtype=torch.bool)
    has[0, :130], has[1, :64] = True, True                              # stored: a page is there and the position lies below t
    has = has.to(DEV)
    wk, wv = _views(rect, B, H, T, hs)
    for got, want in ((gk, wk), (gv, wv)):
        got, want = got.view(torch.int16).transpose(1, 2), want[:, :, :192].view(torch.int16).transpose(1, 2)   # [B, 192, H, hs]
        assert torch.equal(got[has], want[has]), hs
        assert (got[~has] == MARK[2]).all(), hs
    kv = pool.view(torch.int16).view(2, N_PAGES, H, 64, hs)
    unused = torch.ones(N_PAGES, dtype=torch.bool)
    unused[[9, 2, 14, 5]] = False
    assert (kv[:, unused.to(DEV)] == MARK[2]).all(), hs


@pytest.mark.parametrize("hs", [64, 128])
def test_kv_paged_rope_store_rows_is_the_rectangular_rows_store(hs):
    """positions 63, 64, 127, one parked row, one row with no page: qkv and the stored vectors have kv_cache_rope_store_rows's bits, and
    every other byte of the pool and the guards still holds the marker"""
    import omnibiote_ref as R
    from omnibiote_amd.model import rope_tables
    o = ops()
    Bn, C_ = 5, H * hs
    pos = (63, 64, 127, -1, 70)
    rope = rope_tables(R.cast_rope_table(R.rope_table(hs, 128), BF).to(DEV))
    plain = rnd(Bn, 3 * C_, seed=hs + 11).to(DEV)
    rect = o.kv_cache_buffer(Bn, 128, H, hs, DEV)
    rect.view(torch.int16).fill_(MARK[2])
    want_qkv = plain.clone()
    o.kv_cache_rope_store_rows(want_qkv, rope, _i32(pos), 127, Bn, H, hs, rect, 128)
    pool, fence = _fenced_pool(o, hs)
    table = torch.tensor([[3, -1], [8, 0], [-1, 11], [6, 7], [4, N_PAGES]], dtype=torch.int32).to(DEV)   # row 4: position 70 has no page
    qkv = plain.clone()
    o.kv_paged_rope_store_rows(qkv, rope, _i32(pos), 127, Bn, H, hs, pool, N_PAGES, table)
    assert_guards(fence)
    assert torch.equal(qkv.view(torch.int16), want_qkv.view(torch.int16))
    assert torch.equal(qkv[3], plain[3]) and not torch.equal(qkv[4, :2 * C_], plain[4, :2 * C_])   # parked: untouched; no page: rotated all the same
    kv = pool.view(torch.int16).view(2, N_PAGES, H, 64, hs)
    wk, wv = [z.view(torch.int16) for z in _views(rect, Bn, H, 128, hs)]
    wrote = torch.zeros(N_PAGES, 64, dtype=torch.bool)
    for b, (page, slot) in {0: (3, 63), 1: (0, 0), 2: (11, 63)}.items():
        wrote[page, slot] = True
        assert torch.equal(kv[0, page, :, slot], wk[b, :, pos[b]]) and torch.equal(kv[1, page, :, slot], wv[b, :, pos[b]]), (hs, b)
        assert (kv[0, page, :, slot] != MARK[2]).any()
    untouched = ~wrote.to(DEV)
    assert (kv[0].transpose(1, 2)[untouched] == MARK[2]).all() and (kv[1].transpose(1, 2)[untouched] == MARK[2]).all()


# =================================================================================================== block and model
LENS = (61, 130)
STEPS = 70


def _token(ids, b, t):
    return ids[b, t % ids.shape[1]]                                     # (teacher forcing needs some token, not a meaningful one)


def _forced(m, cache, ids, lens, first, steps, check=None):
    """`steps` decode steps feeding row b the token behind its position (the `first`-th step onwards): the logits, (B, steps, vocab)"""
    got = []
    for i in range(first, first + steps):
        tok = torch.stack([_token(ids, b, n + i) for b, n in enumerate(lens)])
        got.append(m.decode_step(tok, cache))
        if check is not None:
            check(i + 1)
    return torch.stack(got, dim=1)


@pytest.mark.parametrize("C_", [256, 128])
def test_paged_prefill_and_decode_are_the_kv_cache_s_bit_for_bit(C_):
    """prefill(lengths=(61, 130)), then 70 teacher-forced decode steps — row 0 crosses positions 64 and 128, row 1 ends on the cache's
    last position — on a PagedKVCache with a shuffled free list and on a KVCache: every logit is the same bits, and the pages in use
    after each step are sum_b ceil(pos_b / 64).

    Then release, rows= and decode_step together.  Row 1 has no position left behind the 70 steps (130 + 70 = block_size), so this
    part starts over and interrupts the run after 30 steps: release(0), prefill(another prompt, rows=[0]), 10 more steps.  Row 1's
    logits are the uninterrupted run's steps 30 .. 39 bit for bit; row 0's are those of a fresh paged run in which that prompt was
    prefilled into row 0 the same way (a one-row launch: a product of other M may take another plan, so only launches of one shape
    are comparable bit for bit)."""
    from omnibiote_amd.model import KVCache, PagedKVCache
    c = _gen_case(C_)
    m, ids = c["m"], c["ids"].to(DEV)
    prompt = ids[:, :max(LENS)].clone()
    prompt[0, LENS[0]:] = 9                                            # padding
    plain = KVCache(m, 2)
    want = torch.cat([m.prefill(prompt, plain, lengths=LENS).unsqueeze(1), _forced(m, plain, ids, LENS, 0, STEPS)], dim=1)
    order = torch.randperm(7, generator=torch.Generator().manual_seed(C_)).tolist()
    paged = PagedKVCache(m, 2, 7, free_order=order)                     # 3 + 4 pages: what the two rows come to hold
    first = m.prefill(prompt, paged, lengths=LENS)
    assert paged.positions.tolist() == list(LENS) and paged.pos == paged.max_pos == 130 and paged.pages_in_use == 1 + 3
    assert paged.table.tolist() == [order[:1] + [-1] * 3, order[1:4] + [-1]]

    def pages(i):
        assert paged.pages_in_use == sum(pages_for(n + i) for n in LENS), i
        assert paged.positions.tolist() == [n + i for n in LENS] == paged.book.row_pos

    got = torch.cat([first.unsqueeze(1), _forced(m, paged, ids, LENS, 0, STEPS, pages)], dim=1)
    assert torch.isfinite(got).all() and torch.equal(got, want), C_
    assert paged.pages_in_use == 7 and paged.pos == 200
    with pytest.raises(ValueError, match="full"):
        m.decode_step(ids[:, 0], paged)
    # what the pool holds is what the rectangle holds, layer by layer, at the positions the rows have filled
    hs = C_ // 2
    for pool, rect in zip(paged.layers, plain.layers):
        gk, gv = paged_gather_reference(pool, paged.table, 7, 2, hs, T=200)
        wk, wv = _views(rect, 2, 2, 200, hs)
        for b, n in enumerate(LENS):
            assert torch.equal(gk[b, :, :n + STEPS], wk[b, :, :n + STEPS]) and torch.equal(gv[b, :, :n + STEPS], wv[b, :, :n + STEPS])

    # ---- release, rows= and decode_step together
    other, other_len = ids[1:2, 20:20 + 77].contiguous(), 77
    paged = PagedKVCache(m, 2, 7, free_order=order[::-1])
    m.prefill(prompt, paged, lengths=LENS)
    _forced(m, paged, ids, LENS, 0, 30)
    held = list(paged.book.row_pages[0])
    paged.release(0)
    assert paged.positions.tolist() == [-1, 160] and paged.table.tolist()[0] == [-1] * 4 and paged.book.free[-len(held):] == held
    logits0 = m.prefill(other, paged, rows=[0])
    assert paged.positions.tolist() == [other_len, 160] and paged.pages_in_use == 2 + 3
    now = (other_len - 30, LENS[1])                                     # (so that step 30 + i feeds row 0 the token behind position 77 + i)
    tail = _forced(m, paged, ids, now, 30, 10)
    assert torch.equal(tail[1], want[1, 31:41]), C_
    fresh = PagedKVCache(m, 2, 7)
    m.prefill(prompt[1:2], fresh, rows=[1])
    fresh_logits0 = m.prefill(other, fresh, rows=[0])
    assert fresh.positions.tolist() == [other_len, LENS[1]]
    fresh_tail = _forced(m, fresh, ids, now, 30, 10)
    assert torch.equal(logits0, fresh_logits0) and torch.equal(tail[0], fresh_tail[0]), C_
    paged.release(0), paged.release(1)
    assert paged.pages_in_use == 0 and sorted(paged.book.free) == list(range(7))


def _ragged(c, lens):
    """right-padded prompts of the fixture's tokens, (len(lens), max(lens)) on the device, and the same as a list of 1-D tensors"""
    ids = c["ids"]
    rows = [ids[i % 2, 3 * i:3 * i + n].clone() for i, n in enumerate(lens)]
    idx = torch.full((len(lens), max(lens)), 7, dtype=torch.int64)
    for i, r in enumerate(rows):
        idx[i, :r.numel()] = r
    return idx.to(DEV), [r.to(DEV) for r in rows]


@pytest.mark.parametrize("C_", [256, 128])
@pytest.mark.parametrize("how", [dict(top_k=1), dict(temperature=0.9, top_k=50)])
def test_generate_many_with_every_request_admitted_is_generate(C_, how):
    """batch == len(prompts), enough pages, no eos_token: the tokens of generate(lengths=, sampler="device") under the same seed"""
    c = _gen_case(C_)
    m = c["m"]
    lens, n = (61, 130, 5), 40
    idx, prompts = _ragged(c, lens)
    want, want_n = m.generate(idx, n, lengths=lens, sampler="device", generator=torch.Generator(device=DEV).manual_seed(5), **how)
    got = m.generate_many(prompts, n, batch=3, generator=torch.Generator(device=DEV).manual_seed(5), **how)
    assert want_n.tolist() == [a + n for a in lens] and len(got) == 3
    for b, a in enumerate(lens):
        assert got[b].dtype == torch.int64 and torch.equal(got[b], want[b, :a + n]), (C_, how, b)


QUEUE_LENS = (130, 5, 64, 97, 33, 128, 70)


def _gaps(m, seq, a):
    """in one causal forward over the finished sequence: every generated token's logit below its position's maximum"""
    with torch.no_grad():
        logits = m(seq.unsqueeze(0)).float()[0]
    at = logits[a - 1:seq.numel() - 1]                                  # position t predicts token t + 1
    return at.max(dim=-1).values - at.gather(-1, seq[a:].unsqueeze(-1)).squeeze(-1)


@pytest.mark.parametrize("C_", [256, 128])
def test_generate_many_as_a_queue(C_, monkeypatch):
    """7 prompts of 5 to 130 tokens through batch = 2 and just the pages of the two largest needs, top_k = 1, 30 new tokens, without
    and with an eos_token (row 0's first greedy token, as test_generate_ragged_eos_parks_a_row_and_sampling_is_seeded takes it).  For
    every request: the prompt is intact, the length is right, and in one causal forward over the finished sequence every generated
    token's logit lies within 2e-2 of its position's maximum — the bound and the argument of
    test_generate_ragged_greedy_follows_the_full_forward; the plain generate of these prompts is held to it first, so the bar is the
    reference's own.  All pages are free at the end: the cache generate_many builds is caught as it is made and looked at afterwards."""
    import omnibiote_amd.model as model
    made = []

    class Caught(model.PagedKVCache):
        def __init__(self, *a, **k):
            super().__init__(*a, **k)
            made.append(self)

    monkeypatch.setattr(model, "PagedKVCache", Caught)
    c = _gen_case(C_)
    m = c["m"]
    n = 30
    idx, prompts = _ragged(c, QUEUE_LENS)
    ref, ref_n = m.generate(idx, n, top_k=1, lengths=QUEUE_LENS)
    for b, a in enumerate(QUEUE_LENS):
        gap = _gaps(m, ref[b, :a + n], a)
        print(f"generate, C={C_}, request {b}: largest gap {gap.max().item():.4g}")
        assert (gap <= 2e-2).all(), (b, gap.max().item())
    needs = sorted(pages_for(a + n) for a in QUEUE_LENS)
    n_pages = needs[-1] + needs[-2]
    eos = int(ref[0, QUEUE_LENS[0]])
    for eos_token in (None, eos):
        got = m.generate_many(prompts, n, batch=2, n_pages=n_pages, top_k=1, eos_token=eos_token)
        assert len(got) == len(prompts)
        for b, a in enumerate(QUEUE_LENS):
            new = got[b][a:]
            assert torch.equal(got[b][:a], prompts[b]), (C_, eos_token, b)
            if eos_token is None:
                assert new.numel() == n
            else:
                hit = (new == eos).nonzero().flatten()
                assert 1 <= new.numel() <= n and (new.numel() == n if hit.numel() == 0 else int(hit[0]) == new.numel() - 1), (C_, b, new.tolist())
            gap = _gaps(m, got[b], a)
            print(f"generate_many, C={C_}, eos {eos_token}, request {b}: {new.numel()} tokens, largest gap {gap.max().item():.4g}")
            assert (gap <= 2e-2).all(), (C_, eos_token, b, gap.max().item())
        cache = made.pop()
        assert not made and cache.batch == 2 and cache.n_pages == n_pages
        assert cache.pages_in_use == 0 and sorted(cache.book.free) == list(range(n_pages)) and cache.book.row_pos == [-1, -1]
        assert (cache.table == -1).all()
