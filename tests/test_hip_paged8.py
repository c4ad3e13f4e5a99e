"""The paged key/value cache in OCP e4m3 on the GPU (include/omnibiote_hip_paged8.h): the two stores against obte_kv8_cache_store's and
obte_kv8_cache_rope_store_rows's codes and scales, obte_attn_decode_paged8 bit for bit against obte_attn_decode_kv8's rows form on the
same codes and scales, missing pages against float64 softmax over the keys that are left of the dequantised pool (the bars of
tests/test_hip_kv8.py for obte_attn_decode_kv8: 2^-7 |ref| + 6e-3, lse atol 2e-3 / rtol 1e-3), the three kernels inside guard bands, the
model path bit for bit against KVCache(dtype="fp8"), and generate_many(kv_dtype="fp8").  The kernel tests use B = 3, H = 2, rows of up to
640 positions in a pool of 40 pages; the model tests the small generation fixtures (block size 200)."""
import pytest
import torch

import omnibiote_ref as R
from fenced import MARK, assert_guards, assert_same_bits, fenced
from omnibiote_amd.kvquant import split_cache
from omnibiote_amd.paged import paged8_gather_reference, paged8_scatter_reference, pages_for
from test_hip_generate import _gen_case, ops
from test_hip_kv8 import _decode_case as _kv8_case
from test_hip_kv8 import _store_inputs
from test_hip_ops import BF, DEV, close, rnd
from test_hip_paged import LENS, QUEUE_LENS, STEPS, _forced, _gaps, _i32, _ragged

pytestmark = pytest.mark.gpu

B, H, T, LD, N_PAGES = 3, 2, 640, 10, 40        # 10 pages per row, 30 of the pool's 40 in use
NEG_INF = float("-inf")
MARK_F32 = torch.tensor(0x5A5A5A5A, dtype=torch.int32).view(torch.float32).item()   # the byte marker 0x5A as the scale a gather fills with


def _rect_parts(cache, B_, T_, hs):
    """a rectangular e4m3 cache as (codes uint8 [2, B, H, T, hs], scales fp32 [2, B, H, T]) on its device"""
    kc, vc, ks, vs = split_cache(cache, B_, T_, H, hs)
    return torch.stack([kc, vc]), torch.stack([ks, vs])


_pools = {}


def _paged_case(hs):
    """tests/test_hip_kv8.py's attention case (a per-key factor 2^[-6, 6] drawn independently for K and V) at B = 3, T = 640: its
    rectangular e4m3 cache, and the same codes and scales in a pool whose pages 1 .. 39 are in random order, every page no row holds filled
    with the NaN code 0x7F and NaN scales (computed once, never modified).  Page 0, where the loads of a missing page go, is one of
    those: a V scale of it that reached a product would leave a NaN."""
    if hs not in _pools:
        c = _kv8_case(B, H, hs, T)
        codes, scales = _rect_parts(c["cache"], B, T, hs)
        table = 1 + torch.randperm(N_PAGES - 1, generator=torch.Generator().manual_seed(hs))[:B * LD]
        table = table.view(B, LD).to(torch.int32).to(DEV)
        pool = paged8_scatter_reference(codes, scales, table, N_PAGES)
        n = N_PAGES * H * 64
        unused = torch.ones(N_PAGES, dtype=torch.bool)
        unused[table.flatten().cpu().long()] = False
        assert int(unused.sum()) == N_PAGES - B * LD and bool(unused[0])
        assert (pool[:2 * n * hs].view(2, N_PAGES, -1)[:, unused.to(DEV)] == 0x7F).all()
        assert torch.isnan(pool[2 * n * hs:].view(torch.float32).view(2, N_PAGES, -1)[:, unused.to(DEV)]).all()
        _pools[hs] = dict(c=c, table=table, pool=pool)
    return _pools[hs]


def _queries(c, counts):
    """packed [B, 3C]: row b is the row of position counts[b] - 1; position 0 where the count is not a valid one"""
    return torch.stack([c["qkv"][b, n - 1 if 1 <= n <= T else 0] for b, n in enumerate(counts)]).contiguous().to(DEV)


# =================================================================================================== the stores
def _fenced_pool(o, hs, poison="mark"):
    """an e4m3 pool inside guard bands, payload and guards holding the poison"""
    n = o.kv8_paged_buffer(N_PAGES, H, hs, DEV).numel()
    assert n == 2 * N_PAGES * H * 64 * (hs + 4)
    view, h = fenced((n,), torch.uint8, poison=poison, back_rows=1)
    assert (view == h.poison).all()
    return view, h


def _pool_views(pool, hs):
    """codes [2, N_PAGES, H, 64, hs] uint8 and scales [2, N_PAGES, H, 64] as int32 bit patterns"""
    n = 2 * N_PAGES * H * 64
    return pool[:n * hs].view(2, N_PAGES, H, 64, hs), pool[n * hs:].view(torch.int32).view(2, N_PAGES, H, 64)


@pytest.mark.parametrize("hs", [64, 128])
def test_kv8_paged_store_is_kv8_cache_store_through_the_table(hs):
    """t = 130 over rows with pages for 130, 64 and 0 positions, the spread-magnitude activation of tests/test_hip_kv8.py (a zero vector,
    maxima exactly at and one ulp above 448 * 2^j): the positions that have a page hold obte_kv8_cache_store's codes and scales, every
    other byte of the pool and the guards still holds the marker"""
    o = ops()
    t, T_ = 130, 192
    qkv = _store_inputs(B, t, H, hs, hs + 7).to(DEV)
    rect = o.kv8_cache_buffer(B, T_, H, hs, DEV)
    rect.fill_(MARK[1])
    o.kv8_cache_store(qkv, B, t, H, hs, rect, T_, 0)
    pool, fence = _fenced_pool(o, hs)
    table = torch.full((B, 3), -1, dtype=torch.int32)
    table[0] = torch.tensor([9, 2, 14])
    table[1, 0] = 5
    table[2] = torch.tensor([N_PAGES, -1, 2 ** 30])                     # (no page of the pool)
    table = table.to(DEV)
    o.kv8_paged_store(qkv, B, t, H, hs, pool, N_PAGES, table)
    assert_guards(fence)
    got_c, got_s = paged8_gather_reference(pool, table, N_PAGES, H, hs, fill_code=MARK[1], fill_scale=MARK_F32)
    want_c, want_s = _rect_parts(rect, B, T_, hs)
    has = torch.zeros(B, T_, dtype=torch.bool)
    has[0, :130], has[1, :64] = True, True                              # stored: a page is there and the position lies below t
    has = has.to(DEV)
    got_c, want_c = got_c.permute(1, 3, 0, 2, 4), want_c.permute(1, 3, 0, 2, 4)                       # [B, T, 2, H, hs]
    got_s, want_s = got_s.view(torch.int32).permute(1, 3, 0, 2), want_s.view(torch.int32).permute(1, 3, 0, 2)
    assert torch.equal(got_c[has], want_c[has]) and torch.equal(got_s[has], want_s[has]), hs
    assert (got_c[~has] == MARK[1]).all() and (got_s[~has] == 0x5A5A5A5A).all(), hs
    assert (want_c[has] != MARK[1]).any() and len(set(want_s[has].flatten().tolist())) > 30           # the spread of scales was there
    codes, scales = _pool_views(pool, hs)
    unused = torch.ones(N_PAGES, dtype=torch.bool)
    unused[[9, 2, 14, 5]] = False
    assert (codes[:, unused.to(DEV)] == MARK[1]).all() and (scales[:, unused.to(DEV)] == 0x5A5A5A5A).all(), hs


@pytest.mark.parametrize("hs", [64, 128])
def test_kv8_paged_rope_store_rows_is_the_rectangular_rows_store(hs):
    """positions 63, 64, 127, one parked row, one row whose position has no page: qkv has obte_kv_cache_rope_store_rows's bits, the stored
    codes and scales are obte_kv8_cache_rope_store_rows's, and every other byte of the pool and the guards still holds the marker"""
    from omnibiote_amd.model import rope_tables
    o = ops()
    Bn, C_ = 5, H * hs
    pos = (63, 64, 127, -1, 70)
    rope = rope_tables(R.cast_rope_table(R.rope_table(hs, 128), BF).to(DEV))
    plain = _store_inputs(Bn, 1, H, hs, hs + 11).reshape(Bn, 3 * C_).to(DEV)
    bf = o.kv_cache_buffer(Bn, 128, H, hs, DEV)
    want_qkv = o.kv_cache_rope_store_rows(plain.clone(), rope, _i32(pos), 127, Bn, H, hs, bf, 128)
    rect = o.kv8_cache_buffer(Bn, 128, H, hs, DEV)
    rect.fill_(MARK[1])
    o.kv8_cache_rope_store_rows(plain.clone(), rope, _i32(pos), 127, Bn, H, hs, rect, 128)
    pool, fence = _fenced_pool(o, hs)
    table = torch.tensor([[3, -1], [8, 0], [-1, 11], [6, 7], [4, N_PAGES]], dtype=torch.int32).to(DEV)   # row 4: position 70 has no page
    qkv = plain.clone()
    o.kv8_paged_rope_store_rows(qkv, rope, _i32(pos), 127, Bn, H, hs, pool, N_PAGES, table)
    assert_guards(fence)
    assert torch.equal(qkv.view(torch.int16), want_qkv.view(torch.int16))
    assert torch.equal(qkv[3], plain[3]) and not torch.equal(qkv[4, :2 * C_], plain[4, :2 * C_])   # parked: untouched; no page: rotated all the same
    codes, scales = _pool_views(pool, hs)
    want_c, want_s = _rect_parts(rect, Bn, 128, hs)
    want_s = want_s.view(torch.int32)
    wrote = torch.zeros(N_PAGES, 64, dtype=torch.bool)
    for b, (page, slot) in {0: (3, 63), 1: (0, 0), 2: (11, 63)}.items():
        wrote[page, slot] = True
        for which in (0, 1):
            assert torch.equal(codes[which, page, :, slot], want_c[which, b, :, pos[b]]), (hs, b, which)
            assert torch.equal(scales[which, page, :, slot], want_s[which, b, :, pos[b]]), (hs, b, which)
            assert (scales[which, page, :, slot] != 0x5A5A5A5A).all()
    untouched = ~wrote.to(DEV)
    assert (codes.transpose(2, 3)[:, untouched] == MARK[1]).all() and (scales.transpose(2, 3)[:, untouched] == 0x5A5A5A5A).all()


# =================================================================================================== one-query attention
@pytest.mark.parametrize("hs", [64, 128])
def test_attn_decode_paged8_is_attn_decode_kv8_rows_bit_for_bit(hs):
    """64 / 65, 128 / 129 and 256 / 257 are the page and round edges (a workgroup round is 128 keys at head size 128, 256 at 64), 1 the
    smallest row; the counts above 512 run two full rounds and a tail at head size 64, the least that hands the table entries fetched one
    round ahead over twice; 3 and 5 splits leave splits empty at the small counts.  Every page no row holds is NaN."""
    o = ops()
    p = _paged_case(hs)
    c = p["c"]
    scale = 8.0 / (H * hs)
    for counts in ((1, 64, 65), (128, 129, 257), (513, 600, 256)):
        q, n_dev = _queries(c, counts), _i32(counts)
        for splits in (1, 2, 3, 5, 0):
            want, want_lse = o.attn_decode_kv8(q, c["cache"], B, T, T, H, hs, scale, splits=splits, n_keys_rows=n_dev)
            got, lse = o.attn_decode_paged8(q, p["pool"], N_PAGES, p["table"], B, n_dev, T, H, hs, scale, splits=splits)
            assert torch.isfinite(got).all() and torch.isfinite(lse).all(), (hs, counts, splits)
            assert torch.equal(got, want) and torch.equal(lse, want_lse), (hs, counts, splits)


@pytest.mark.parametrize("hs", [64, 128])
def test_attn_decode_paged8_missing_pages(hs):
    """An entry of -1, of n_pages or of 2^30 in the middle of a row removes exactly those 64 keys: float64 softmax over the remaining keys
    of the dequantised pool, at the bars tests/test_hip_kv8.py holds obte_attn_decode_kv8 to.  With the per-key factors 2^[-6, 6] a
    dropped or swapped scale misses them by orders of magnitude.  Page 0 — where a missing page's loads go — holds what reaches no
    result: the NaN code 0x7F with NaN scales (a page nobody holds), with scales of +inf and -inf, and another row's vectors (row 2's
    first page moved there).  A row with every entry missing, or with a count outside [1, max_keys], gives exact zeros and lse = -inf,
    over each of the three."""
    o = ops()
    p = _paged_case(hs)
    c = p["c"]
    scale = 8.0 / (H * hs)
    counts = (600, 130, 640)
    gone = ((0, 1, -1), (1, 0, N_PAGES), (2, 6, 2 ** 30))               # (row, entry, what stands there)
    page0 = {"nan": (p["pool"], p["table"])}
    pool = p["pool"].clone()
    _pool_views(pool, hs)[1].view(torch.float32)[:, 0] = torch.tensor([float("inf"), NEG_INF], device=DEV).view(1, 2, 1)   # K and V, by head
    page0["inf"] = (pool, p["table"])
    pool, moved = p["pool"].clone(), p["table"].clone()
    was = int(moved[2, 0])
    for part in _pool_views(pool, hs):
        part[:, 0], part[:, was] = part[:, was].clone(), part[:, 0].clone()
    moved[2, 0] = 0
    page0["held"] = (pool, moved)
    keep = torch.ones(B, T, dtype=torch.bool)
    for b, j, v in gone:
        keep[b, 64 * j:64 * j + 64] = False
    q, n_dev = _queries(c, counts), _i32(counts)
    ref_o, ref_lse = [], []
    for b, n in enumerate(counts):
        qb = c["qkv"][b, n - 1, :H * hs].reshape(H, 1, hs).double()
        s = (qb @ c["K"][b, :, :n].transpose(-2, -1)) * scale            # [H, 1, n], on the dequantised codes
        s = s.masked_fill(~keep[b, :n].view(1, 1, n), NEG_INF)
        ref_o.append((torch.softmax(s, dim=-1) @ c["V"][b, :, :n]).reshape(-1))
        ref_lse.append(torch.logsumexp(s, dim=-1).reshape(-1))
    ref_o, ref_lse = torch.stack(ref_o), torch.stack(ref_lse)
    for name, (pool, whole) in page0.items():
        table = whole.clone()
        for b, j, v in gone:
            table[b, j] = v
        for splits in (0, 1, 2, 3, 5):
            got, lse = o.attn_decode_paged8(q, pool, N_PAGES, table, B, n_dev, T, H, hs, scale, splits=splits)
            close(got, ref_o, atol=6e-3, what=f"attn_decode_paged8, missing pages, page 0 {name}, hs={hs} splits={splits}")
            close(lse, ref_lse, atol=2e-3, rtol=1e-3, what=f"lse, missing pages, page 0 {name}, hs={hs} splits={splits}")
    # row 0: no page at all; row 1: counts outside [1, max_keys]; row 2 stays and keeps its bits
    max_keys = 600
    for name, (pool, whole) in page0.items():
        table = whole.clone()
        table[0] = _i32((-1, N_PAGES, 2 ** 30, -7, -1, N_PAGES + 1, -2 ** 31, 2 ** 31 - 1, -1, N_PAGES))
        for n1 in (0, -1, max_keys + 1, 2 ** 31 - 1):
            counts = (600, n1, 129)
            q, n_dev = _queries(c, counts), _i32(counts)
            for splits in (0, 1, 3):
                got, lse = o.attn_decode_paged8(q, pool, N_PAGES, table, B, n_dev, max_keys, H, hs, scale, splits=splits)
                want, want_lse = o.attn_decode_kv8(q, c["cache"], B, T, max_keys, H, hs, scale, splits=splits, n_keys_rows=n_dev)
                for b in (0, 1):
                    assert (got[b].view(torch.int16) == 0).all() and (lse[b] == NEG_INF).all(), (name, hs, n1, splits, b)
                assert torch.equal(got[2], want[2]) and torch.equal(lse[2], want_lse[2]), (name, hs, n1, splits)


# =================================================================================================== guard bands
@pytest.mark.parametrize("hs", [64, 128])
def test_paged8_kernels_inside_guard_bands(hs):
    """the three kernels with their operands 16 bytes into buffers that are NaN (inputs: bf16 NaN, the NaN code 0x7F) or a marker (outputs,
    integers) everywhere else: the plain call's bits, and every guard intact"""
    from omnibiote_amd._lib import lib
    from omnibiote_amd.model import rope_tables
    o = ops()
    Bn, t, ld = 2, 150, 3
    C_ = H * hs
    scale = 8.0 / C_
    table = torch.tensor([[7, 31, 0], [12, 39, 20]], dtype=torch.int32, device=DEV)
    qkv = rnd(Bn, t, 3 * C_, seed=hs).to(DEV)
    plain = o.kv8_paged_buffer(N_PAGES, H, hs, DEV)
    plain.fill_(0x7F)
    o.kv8_paged_store(qkv, Bn, t, H, hs, plain, N_PAGES, table)
    fq, hq = fenced(qkv.view(Bn * t, 3 * C_), poison="nan")
    fc, hc = _fenced_pool(o, hs, poison=0x7F)
    ft, ht = fenced(table, poison="mark")
    o.kv8_paged_store(fq, Bn, t, H, hs, fc, N_PAGES, ft)
    assert_same_bits(fc, plain, "pool after the store")
    assert_guards(hq, hc, ht)
    # one step's rotate-and-store at positions 150 and 151
    rope = rope_tables(R.rope_table(hs, 192).to(DEV))
    pos = _i32((150, 151))
    step = rnd(Bn, 3 * C_, seed=hs + 1).to(DEV)
    want_step = o.kv8_paged_rope_store_rows(step.clone(), rope, pos, 151, Bn, H, hs, plain, N_PAGES, table)
    fs, hs_ = fenced(step, poison="nan")
    fcos, hcos = fenced(rope[0][:152].contiguous(), poison="nan")
    fsin, hsin = fenced(rope[1][:152].contiguous(), poison="nan")
    fp, hp = fenced(pos, poison="mark")
    o.kv8_paged_rope_store_rows(fs, (fcos, fsin), fp, 151, Bn, H, hs, fc, N_PAGES, ft)
    assert_same_bits(fs, want_step, "qkv after the rotation")
    assert_same_bits(fc, plain, "pool after the step")
    assert_guards(hs_, hcos, hsin, hp, hc, ht)
    # attention over the positions the rows hold (row 0: 0 .. 150), 152 the host's bound
    q = want_step[:, :C_].contiguous()
    rows = _i32((151, 77))
    for splits in (1, 3):
        want = o.attn_decode_paged8(q, plain, N_PAGES, table, Bn, rows, 152, H, hs, scale, splits=splits)
        assert torch.isfinite(want[0]).all() and torch.isfinite(want[1]).all()
        fqq, hqq = fenced(q, poison="nan", ld=C_ + 8)
        fo, ho = fenced((Bn, C_), dtype=BF, poison="mark")
        fl, hl = fenced((Bn, H), dtype=torch.float32, poison="mark")
        ws, hw = fenced((int(lib().obte_attn_decode_ws_bytes(Bn, H, hs)),), dtype=torch.uint8, poison="mark", back_rows=1)
        fr, hr = fenced(rows, poison="mark")
        got = o.attn_decode_paged8(fqq, fc, N_PAGES, ft, Bn, fr, 152, H, hs, scale, splits=splits, q_ld=C_ + 8, ws=ws, out=fo, lse=fl)
        assert_same_bits(got[0], want[0], "o")
        assert_same_bits(got[1], want[1], "lse")
        assert_guards(hqq, hc, ht, ho, hl, hr, hw)
        used = Bn * H * splits * (hs + 4) * 4 if splits > 1 else 0
        assert bool((ws[used:] == 0x5A).all())                         # the workspace: nothing beyond the partials of `splits` splits


# =================================================================================================== block and model
@pytest.mark.parametrize("C_", [256, 128])
def test_paged_fp8_prefill_and_decode_are_the_fp8_kv_cache_s_bit_for_bit(C_):
    """tests/test_hip_paged.py's model test on the e4m3 formats: prefill(lengths=(61, 130)), then 70 teacher-forced decode steps, on a
    PagedKVCache(dtype="fp8") with a shuffled free list and on a KVCache(dtype="fp8"): every logit is the same bits, the pages in use
    after each step are sum_b ceil(pos_b / 64), and the pool holds the rectangle's codes and scales.  Then that test's interruption, with
    its two deviations for the same reasons (row 1 has no position left behind the 70 steps, so this part starts over and interrupts
    after 30; row 0's fresh run prefills it alone, since only launches of one shape compare bit for bit): release(0),
    prefill(another prompt, rows=[0]), 10 more steps."""
    from omnibiote_amd.model import KVCache, PagedKVCache
    c = _gen_case(C_)
    m, ids = c["m"], c["ids"].to(DEV)
    hs = C_ // 2
    prompt = ids[:, :max(LENS)].clone()
    prompt[0, LENS[0]:] = 9                                            # padding
    plain = KVCache(m, 2, dtype="fp8")
    want = torch.cat([m.prefill(prompt, plain, lengths=LENS).unsqueeze(1), _forced(m, plain, ids, LENS, 0, STEPS)], dim=1)
    order = torch.randperm(7, generator=torch.Generator().manual_seed(C_)).tolist()
    paged = PagedKVCache(m, 2, 7, free_order=order, dtype="fp8")       # 3 + 4 pages: what the two rows come to hold
    assert paged.dtype == "fp8" and all(p.dtype == torch.uint8 and p.numel() == 2 * 7 * 2 * 64 * (hs + 4) for p in paged.layers)
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
    for pool, rect in zip(paged.layers, plain.layers):
        got_c, got_s = paged8_gather_reference(pool, paged.table, 7, 2, hs, T=200)
        want_c, want_s = _rect_parts(rect, 2, 200, hs)
        for b, n in enumerate(LENS):
            assert torch.equal(got_c[:, b, :, :n + STEPS], want_c[:, b, :, :n + STEPS])
            assert torch.equal(got_s[:, b, :, :n + STEPS].view(torch.int32), want_s[:, b, :, :n + STEPS].view(torch.int32))

    # ---- release, rows= and decode_step together
    other, other_len = ids[1:2, 20:20 + 77].contiguous(), 77
    paged = PagedKVCache(m, 2, 7, free_order=order[::-1], dtype="fp8")
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
    fresh = PagedKVCache(m, 2, 7, dtype="fp8")
    m.prefill(prompt[1:2], fresh, rows=[1])
    fresh_logits0 = m.prefill(other, fresh, rows=[0])
    assert fresh.positions.tolist() == [other_len, LENS[1]]
    fresh_tail = _forced(m, fresh, ids, now, 30, 10)
    assert torch.equal(logits0, fresh_logits0) and torch.equal(tail[0], fresh_tail[0]), C_
    paged.release(0), paged.release(1)
    assert paged.pages_in_use == 0 and sorted(paged.book.free) == list(range(7))


@pytest.mark.parametrize("C_", [256, 128])
@pytest.mark.parametrize("how", [dict(top_k=1), dict(temperature=0.9, top_k=50)])
def test_generate_many_fp8_with_every_request_admitted_is_generate_fp8(C_, how):
    """batch == len(prompts), enough pages, no eos_token: the tokens of generate(lengths=, sampler="device", kv_dtype="fp8") under the
    same seed"""
    c = _gen_case(C_)
    m = c["m"]
    lens, n = (61, 130, 5), 40
    idx, prompts = _ragged(c, lens)
    want, want_n = m.generate(idx, n, lengths=lens, sampler="device", kv_dtype="fp8", generator=torch.Generator(device=DEV).manual_seed(5), **how)
    got = m.generate_many(prompts, n, batch=3, kv_dtype="fp8", generator=torch.Generator(device=DEV).manual_seed(5), **how)
    assert want_n.tolist() == [a + n for a in lens] and len(got) == 3
    for b, a in enumerate(lens):
        assert got[b].dtype == torch.int64 and torch.equal(got[b], want[b, :a + n]), (C_, how, b)


@pytest.mark.parametrize("C_", [256, 128])
def test_generate_many_fp8_as_a_queue(C_, monkeypatch):
    """test_generate_many_as_a_queue on the e4m3 pool: 7 prompts of 5 to 130 tokens through batch = 2 and just the pages of the two
    largest needs, top_k = 1, 30 new tokens.  For every request: the prompt is intact, the length is right, and in one causal forward
    over the finished sequence every generated token's logit lies within 2e-2 of its position's maximum; the plain
    generate(kv_dtype="fp8") of these prompts is held to the bound first, so the bar is the reference path's own.  All pages are free at
    the end, and the cache the call built was an e4m3 one."""
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
    ref, ref_n = m.generate(idx, n, top_k=1, lengths=QUEUE_LENS, kv_dtype="fp8")
    for b, a in enumerate(QUEUE_LENS):
        gap = _gaps(m, ref[b, :a + n], a)
        print(f"generate fp8, C={C_}, request {b}: largest gap {gap.max().item():.4g}")
        assert (gap <= 2e-2).all(), (b, gap.max().item())
    needs = sorted(pages_for(a + n) for a in QUEUE_LENS)
    n_pages = needs[-1] + needs[-2]
    got = m.generate_many(prompts, n, batch=2, n_pages=n_pages, top_k=1, kv_dtype="fp8")
    assert len(got) == len(prompts)
    for b, a in enumerate(QUEUE_LENS):
        assert torch.equal(got[b][:a], prompts[b]) and got[b].numel() == a + n, (C_, b)
        gap = _gaps(m, got[b], a)
        print(f"generate_many fp8, C={C_}, request {b}: largest gap {gap.max().item():.4g}")
        assert (gap <= 2e-2).all(), (C_, b, gap.max().item())
    cache = made.pop()
    assert not made and cache.batch == 2 and cache.n_pages == n_pages and cache.dtype == "fp8" and cache.layers[0].dtype == torch.uint8
    assert cache.pages_in_use == 0 and sorted(cache.book.free) == list(range(n_pages)) and cache.book.row_pos == [-1, -1]
    assert (cache.table == -1).all()
