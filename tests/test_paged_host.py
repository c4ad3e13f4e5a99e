"""Host-side tests (no GPU) of the paged key/value cache and of continuous batching: the scheduler object alone over random seeded
workloads, the cache's bookkeeping without buffers, the new refusals on a fake paged cache, the reference's gather / scatter as pure
functions, the paged entry points' argument checks that return before a launch, and the symbol table."""
import ctypes as C
import random

import pytest
import torch

from omnibiote_amd import _lib
from omnibiote_amd.paged import KV_PAGE, PageBook, PagedSchedule, paged_gather_reference, paged_scatter_reference, pages_for, pool_bytes

EINVAL = -1
P = 4096   # a non-null, 16-byte aligned "pointer" for calls that must return before they touch it


def _err():
    return _lib.lib().obte_last_error().decode()


# ------------------------------------------------------------------------------------------------------- the scheduler alone
def _drive(lengths, max_new, batch, n_pages, rng):
    """Run a PagedSchedule to its end with random end times, a PageBook taking the pages as generate_many's cache would (pages for the
    prompt at admission, one more whenever a position opens a page), and check the invariants at every step.  Returns the admission
    order and the largest number of pages in use."""
    s = PagedSchedule(lengths, max_new, batch, n_pages, block_size=None)
    pages = PageBook(batch, s.n_pages, max(lengths) + max_new, free_order=rng.sample(range(s.n_pages), s.n_pages))
    ends = [rng.randint(1, max_new) for _ in lengths]                   # the token at which each request meets its eos_token
    made, order, running, peak = [0] * len(lengths), [], {}, 0
    guard = 0
    while not s.done:
        guard += 1
        assert guard < 10 * (sum(ends) + len(lengths)), "the schedule does not end"
        for r, slot in s.admit():
            assert slot not in running.values() and r not in running and 0 <= slot < batch
            running[r] = slot
            order.append(r)
            pages.assign(slot, lengths[r])                              # (never raises: the promise covers it)
            pages.place(slot, lengths[r])
        assert running, "nothing runs and nothing was admitted"
        # the invariants
        assert s.promised == sum(s.need[r] for r in running) <= s.n_pages
        owned = [p for slot in running.values() for p in pages.row_pages[slot]]
        assert len(owned) == len(set(owned)) == pages.pages_in_use and not set(owned) & set(pages.free)
        for r, slot in running.items():
            assert len(pages.row_pages[slot]) <= s.need[r]
            assert pages.table[slot, :len(pages.row_pages[slot])].tolist() == pages.row_pages[slot]
            assert (pages.table[slot, len(pages.row_pages[slot]):] == -1).all()
        peak = max(peak, pages.pages_in_use)
        # one token per running request; the finished ones leave at once
        for r in list(running):
            made[r] += 1
            if made[r] == ends[r]:
                pages.release(s.finish(r))
                del running[r]
        if running:
            pages.grow_for_step()                                       # (never raises either)
            pages.step()
    assert made == ends and not running
    assert pages.pages_in_use == 0 and sorted(pages.free) == list(range(s.n_pages)) and s.promised == 0
    assert sorted(s.free_slots) == list(range(batch)) and (pages.table == -1).all() and pages.row_pos == [-1] * batch
    return order, peak


@pytest.mark.parametrize("seed", range(8))
def test_schedule_random_workloads(seed):
    rng = random.Random(seed)
    n = rng.randint(1, 40)
    max_new = rng.randint(1, 200)
    lengths = [rng.randint(1, 700) for _ in range(n)]
    batch = rng.randint(1, 9)
    largest = max(pages_for(a + max_new) for a in lengths)
    n_pages = rng.choice([None, largest, largest + rng.randint(0, 3 * largest)])
    order, peak = _drive(lengths, max_new, batch, n_pages, rng)
    assert order == list(range(n))                                      # first in, first out, each exactly once
    assert peak <= (batch * largest if n_pages is None else n_pages)


def test_schedule_is_strictly_fifo_and_promises_by_need():
    # needs at 10 new tokens: 1, 3, 1 pages; a pool of 3: request 1 has to wait for request 0, and request 2 is not let past it
    s = PagedSchedule([5, 130, 5], 10, batch=3, n_pages=3)
    assert s.need == [1, 3, 1]
    assert s.admit() == [(0, 0)] and s.admit() == [] and s.promised == 1
    assert s.finish(0) == 0 and s.promised == 0
    assert s.admit() == [(1, 0)] and s.admit() == [] and s.promised == 3
    s.finish(1)
    assert s.admit() == [(2, 0)] and not s.done
    s.finish(2)
    assert s.done and s.admit() == []
    # slots: the lowest free one first; n_pages=None is batch times the largest need
    s = PagedSchedule([64, 1, 1, 1], 1, batch=2)
    assert s.n_pages == 4 and s.admit() == [(0, 0), (1, 1)]
    s.finish(0)
    assert s.admit() == [(2, 0)]


def test_schedule_refuses_what_can_never_fit_before_the_first_admission():
    with pytest.raises(ValueError, match=r"request 1: 190 prompt tokens \+ 11 new ones exceed block_size = 200"):
        PagedSchedule([5, 190], 11, batch=2, block_size=200)
    with pytest.raises(ValueError, match=r"request 1 needs 3 pages .* n_pages = 2"):
        PagedSchedule([5, 130], 10, batch=2, n_pages=2)
    with pytest.raises(ValueError, match="empty"):
        PagedSchedule([5, 0], 10, batch=2)
    with pytest.raises(ValueError, match="batch"):
        PagedSchedule([5], 10, batch=0)
    with pytest.raises(ValueError, match="max_new_tokens"):
        PagedSchedule([5], 0, batch=1)
    assert PagedSchedule([], 4, batch=2).done


# ------------------------------------------------------------------------------------------------------- the bookkeeping without buffers
def _fake(batch=3, n_pages=6, max_len=200, free_order=None):
    """a paged cache's position and page state (the host-only class PagedKVCache is built on) with no buffer behind it"""
    from omnibiote_amd.model import PagedPositions
    c = PagedPositions(batch, n_pages, max_len, free_order)
    c.layers, c.decode_ws, c.extend_ws = [None], None, None
    return c


def test_paged_positions_assign_release_and_growth():
    from omnibiote_amd.model import CachePositions, PagedKVCache, PagedPositions
    assert issubclass(PagedKVCache, PagedPositions) and issubclass(PagedPositions, CachePositions)
    c = _fake(free_order=[4, 2, 5, 0, 1, 3])
    assert c.table.shape == (3, 4) and c.table.dtype == torch.int32 and (c.table == -1).all()
    assert c.positions.tolist() == [-1, -1, -1] and c.positions.dtype == torch.int32 and c.pos == c.max_pos == 0 and c.pages_in_use == 0
    c.start_rows([0, 2], [63, 130])
    assert c.table.tolist() == [[4, -1, -1, -1], [-1, -1, -1, -1], [2, 5, 0, -1]]
    assert c.positions.tolist() == [63, -1, 130] and c.pos == c.max_pos == 130 and c.min_pos == 63 and c.pages_in_use == 4
    c.prepare_step()                                                    # positions 63 and 130 lie in pages the rows hold
    assert c.pages_in_use == 4
    c.advance(1)
    assert c.positions.tolist() == [64, -1, 131] and c.book.row_pos == [64, -1, 131] and c.pos == 131
    old = c.table
    c.prepare_step()                                                    # 63 -> 64: row 0 opens its second page
    assert c.table.tolist()[0] == [4, 1, -1, -1] and c.pages_in_use == 5 and c.table is not old and old.tolist()[0] == [4, -1, -1, -1]
    c.assign(1, 64)                                                     # by hand: the last free page
    assert c.pages_in_use == 6 and c.table.tolist()[1] == [3, -1, -1, -1] and c.positions.tolist() == [64, -1, 131]
    c = _fake(n_pages=3)
    c.start_rows([0, 1], [64, 64])
    c.assign(2, 10)
    with pytest.raises(ValueError, match="free"):
        c.assign(2, 65)
    assert c.pages_in_use == 3 and c.table.tolist()[2] == [2, -1, -1, -1]
    c = _fake(n_pages=2)
    c.start_rows([0, 1], [64, 64])
    before = c.table.clone()
    with pytest.raises(ValueError, match="opens 2 new pages"):
        c.prepare_step()                                                # an empty free list: raised with nothing changed
    assert torch.equal(c.table, before) and c.positions.tolist() == [64, 64, -1]
    c.release(0)
    assert c.pages_in_use == 1 and c.table.tolist()[0] == [-1] * 4 and c.positions.tolist() == [-1, 64, -1] and c.pos == 64
    c.prepare_step()                                                    # row 1 takes the page row 0 gave back
    assert c.table.tolist()[1] == [1, 0, -1, -1]
    c.park_rows([1])
    assert c.positions.tolist() == [-1, -1, -1] and c.pages_in_use == 2 and c.pos == 0
    with pytest.raises(ValueError, match="free"):
        c.start_rows([0, 2], [64, 1])                                   # two pages wanted, none free: nothing changes
    assert c.pages_in_use == 2 and c.positions.tolist() == [-1, -1, -1]


def test_paged_positions_refuse_what_needs_the_device_s_word():
    c = _fake()
    c.start_rows([0, 1, 2], [5, 6, 7])
    for call in (lambda: c.park(torch.zeros(3, dtype=torch.bool)), lambda: c.rewind(1), lambda: c.rewind_rows([1, 1, 1]), lambda: c.reset(4),
                 lambda: c.advanced_on_device(1), lambda: c.advance(2)):
        with pytest.raises(ValueError, match="PagedKVCache"):
            call()
    assert c.positions.tolist() == [5, 6, 7] and c.pages_in_use == 3


def test_page_book_checks():
    with pytest.raises(ValueError, match="free_order"):
        PageBook(2, 4, 100, free_order=[0, 1, 1, 3])
    b = PageBook(2, 4, 100)
    assert b.table_ld == 2 and b.assign(0, 100) == [0, 1] and b.assign(0, 100) == []
    with pytest.raises(ValueError, match="max_len"):
        b.assign(1, 101)
    with pytest.raises(ValueError, match="row 2"):
        b.assign(2, 1)
    b.place(0, 100)
    with pytest.raises(ValueError, match="last position"):
        b.grow_for_step()


# ------------------------------------------------------------------------------------------------------- the new refusals
def _cpu_model(block_size=200):
    from omnibiote_amd.model import OmniBioTA, OmniBioTAConfig
    c = OmniBioTAConfig()
    c.block_size, c.vocab_size, c.n_layer, c.n_head, c.n_embd, c.dropout, c.flash = block_size, 64, 1, 2, 128, 0.0, True
    c.autoregressive = True
    return OmniBioTA(c)


def test_paged_cache_refuses_before_any_state_changes():
    from omnibiote_amd.model import CachePositions, DecodeLoop, QuantizedWeights
    m = _cpu_model()
    c = _fake()
    c.start_rows([0, 1, 2], [5, 6, 7])
    state = lambda: (c.positions.tolist(), c.table.tolist(), c.pages_in_use, c.pos)   # noqa: E731
    before = state()
    tok = torch.zeros(3, 4, dtype=torch.int64)
    w = QuantizedWeights.__new__(QuantizedWeights)                     # (refused before it is looked at)
    with pytest.raises(NotImplementedError, match=r"extend: the cache is a paged cache"):
        m.extend(tok, c)
    with pytest.raises(NotImplementedError, match=r"prefill\(chunk=\): the cache is a paged cache"):
        m.prefill(tok, c, chunk=2)
    with pytest.raises(NotImplementedError, match=r"draft_and_verify: the cache is a paged cache"):
        m.draft_and_verify(m, tok[:, 0], c, _fake(), 2)
    plain = CachePositions(3, 32)
    plain.reset(8)
    plain.layers, plain.decode_ws, plain.extend_ws = [None], None, None
    with pytest.raises(NotImplementedError, match=r"draft_and_verify: the cache is a paged cache"):
        m.draft_and_verify(m, tok[:, 0], plain, c, 2)                   # (the draft's cache: it could not step back)
    with pytest.raises(NotImplementedError, match=r"prefill: weights= .* paged cache"):
        m.prefill(tok, c, weights=w)
    with pytest.raises(NotImplementedError, match=r"decode_step: weights= .* paged cache"):
        m.decode_step(tok[:, 0], c, weights=w)
    with pytest.raises(NotImplementedError, match=r"DecodeLoop: the cache is a paged cache"):
        DecodeLoop(m, c, max_steps=4)
    assert state() == before
    # rows= belongs to a paged cache, and is checked on one before anything is assigned
    plain = CachePositions(3, 32)
    with pytest.raises(ValueError, match="rows= names the rows of a PagedKVCache"):
        m.prefill(tok, plain, rows=[0, 1, 2])
    for rows in ([0, 1], [0, 1, 1], [0, 1, 3]):
        with pytest.raises(ValueError, match="distinct rows"):
            m.prefill(tok, c, rows=rows)
    with pytest.raises(ValueError, match="3 lengths for a batch of 2|2 lengths for a batch of 3"):
        m.prefill(tok, c, lengths=[1, 2])
    assert state() == before


def test_generate_many_refuses_before_anything_is_launched():
    m = _cpu_model()
    p = [torch.zeros(5, dtype=torch.int64), torch.zeros(190, dtype=torch.int64)]
    with pytest.raises(ValueError, match="exceed block_size = 200"):
        m.generate_many(p, 11, batch=2)
    with pytest.raises(ValueError, match="n_pages = 1"):
        m.generate_many(p, 5, batch=2, n_pages=1)
    with pytest.raises(ValueError, match="1-D int64"):
        m.generate_many([torch.zeros(2, 2, dtype=torch.int64)], 5, batch=2)
    with pytest.raises(ValueError, match="top_p"):
        m.generate_many(p, 5, batch=2, top_p=0.0)
    assert m.generate_many([], 5, batch=2) == []
    enc = _cpu_model()
    enc.config.autoregressive = False
    with pytest.raises(ValueError, match="not autoregressive"):
        enc.generate_many(p, 5, batch=2)


# ------------------------------------------------------------------------------------------------------- the format in plain torch
def test_gather_and_scatter_reference_are_inverse():
    g = torch.Generator().manual_seed(3)
    B, H, hs, n_pages = 3, 2, 8, 16
    K, V = [torch.randn(B, H, 256, hs, generator=g).to(torch.bfloat16) for _ in range(2)]
    table = torch.randperm(n_pages, generator=g)[:12].view(B, 4).to(torch.int32)
    pool = paged_scatter_reference(K, V, table, n_pages)
    assert pool.numel() * 2 == pool_bytes(n_pages, H, hs) and pages_for(64) == 1 and pages_for(65) == 2 and KV_PAGE == _lib.KV_PAGE == 64
    kv = pool.view(2, n_pages, H, 64, hs)
    used = torch.zeros(n_pages, dtype=torch.bool)
    used[table.flatten().long()] = True
    assert torch.isnan(kv[:, ~used]).all() and not torch.isnan(kv[:, used]).any()
    assert torch.equal(kv[0, table[1, 2].item(), 1], K[1, 1, 128:192])      # page table[b][j], head h: positions [64 j, 64 j + 64)
    gk, gv = paged_gather_reference(pool, table, n_pages, H, hs)
    assert torch.equal(gk, K) and torch.equal(gv, V)
    table[0, 1], table[2, 3] = -1, n_pages                                   # no page: the fill
    gk, gv = paged_gather_reference(pool, table, n_pages, H, hs, T=200, fill=7.0)
    assert gk.shape == (B, H, 200, hs) and (gk[0, :, 64:128] == 7).all() and (gv[2, :, 192:] == 7).all()
    assert torch.equal(gk[1], K[1, :, :200]) and torch.equal(gk[0, :, :64], K[0, :, :64])


# ------------------------------------------------------------------------------------------------------- entry points and symbols
def test_paged_symbols_and_abi():
    names = ["obte_kv_paged_bytes", "obte_kv_paged_store", "obte_kv_paged_rope_store_rows", "obte_attn_decode_paged", "obte_block_fwd_prefill_paged",
             "obte_block_decode_paged"]
    assert list(_lib.SYMBOLS_PAGED) == names
    lib = _lib.lib()
    for n in names:
        assert getattr(lib, n).argtypes == _lib.SYMBOLS_PAGED[n][1]
    assert lib.obte_abi_version() == 1
    sizes = (C.c_int64 * 8)()
    assert lib.obte_struct_sizes(sizes, 8) == 6
    header = open(__file__.rsplit("/tests/", 1)[0] + "/include/omnibiote_hip_paged.h").read()
    for n in names:
        assert n + "(" in header
    assert "#define OBTE_KV_PAGE 64" in header
    assert lib.obte_kv_paged_bytes(16, 2, 128) == pool_bytes(16, 2, 128) == 16 * 2 * 64 * 128 * 4
    assert lib.obte_kv_paged_bytes(16, 2, 32) == 0 and lib.obte_kv_paged_bytes(0, 2, 64) == 0


def _call_store(qkv=P, B=1, t=10, H=1, hs=128, pool=P, n_pages=4, table=P, ld=2):
    return _lib.lib().obte_kv_paged_store(qkv, B, t, H, hs, pool, n_pages, table, ld, None)


def _call_rope(qkv=P, cos=P, sin=P, pos=P, max_pos=5, B=1, H=1, hs=128, pool=P, n_pages=4, table=P, ld=2):
    return _lib.lib().obte_kv_paged_rope_store_rows(qkv, cos, sin, pos, max_pos, B, H, hs, pool, n_pages, table, ld, None)


def _call_decode(q=P, q_ld=128, pool=P, n_pages=4, table=P, ld=2, o=P, lse=None, B=1, n_keys=P, max_keys=10, H=1, hs=128, splits=1, ws=None, ws_bytes=0):
    return _lib.lib().obte_attn_decode_paged(q, q_ld, pool, n_pages, table, ld, o, lse, B, n_keys, max_keys, H, hs, 1.0, splits, ws, ws_bytes, None)


@pytest.mark.parametrize("call,name,kw,word", [
    (_call_store, "obte_kv_paged_store", dict(qkv=None), "null"), (_call_store, "obte_kv_paged_store", dict(table=None), "null"),
    (_call_store, "obte_kv_paged_store", dict(t=129), "do not fit"), (_call_store, "obte_kv_paged_store", dict(t=0), "do not fit"),
    (_call_store, "obte_kv_paged_store", dict(hs=32), "head_dim"), (_call_store, "obte_kv_paged_store", dict(n_pages=0), "shape"),
    (_call_store, "obte_kv_paged_store", dict(pool=P + 8), "aligned"),
    (_call_rope, "obte_kv_paged_rope_store_rows", dict(pos=None), "null"), (_call_rope, "obte_kv_paged_rope_store_rows", dict(pool=None), "null"),
    (_call_rope, "obte_kv_paged_rope_store_rows", dict(max_pos=128), "max_pos"), (_call_rope, "obte_kv_paged_rope_store_rows", dict(max_pos=-1), "max_pos"),
    (_call_rope, "obte_kv_paged_rope_store_rows", dict(ld=0), "shape"), (_call_rope, "obte_kv_paged_rope_store_rows", dict(table=P + 2), "aligned"),
    (_call_decode, "obte_attn_decode_paged", dict(q=None), "null"), (_call_decode, "obte_attn_decode_paged", dict(table=None), "null"),
    (_call_decode, "obte_attn_decode_paged", dict(n_keys=None), "null"), (_call_decode, "obte_attn_decode_paged", dict(max_keys=129), "max_keys"),
    (_call_decode, "obte_attn_decode_paged", dict(max_keys=0), "max_keys"), (_call_decode, "obte_attn_decode_paged", dict(splits=-1), "splits"),
    (_call_decode, "obte_attn_decode_paged", dict(splits=2, ws=P, ws_bytes=64), "workspace"), (_call_decode, "obte_attn_decode_paged", dict(hs=32), "head_dim"),
    (_call_decode, "obte_attn_decode_paged", dict(q_ld=64), "q_ld"),
])
def test_paged_entry_points_reject_before_any_launch(call, name, kw, word):
    assert call(**kw) == EINVAL
    assert _err().startswith(name + ":") and word in _err(), _err()


def test_paged_block_entry_points_reject_before_any_launch():
    lib = _lib.lib()
    d = _lib.BlockDesc(B=2, T=1, n_embd=256, n_head=2, ln1_w=P, attn_w=P, proj_w=P, ln2_w=P, fc_w=P, mlp_w=P, rope_cos=P, rope_sin=P)
    need = lib.obte_block_decode_ws_bytes(2, 256, 2)
    assert lib.obte_block_decode_paged(C.byref(d), P, P, None, 4, P, 2, P, 5, P, need, None) == EINVAL and "obte_block_decode_paged: null" in _err()
    assert lib.obte_block_decode_paged(C.byref(d), P, P, P, 4, None, 2, P, 5, P, need, None) == EINVAL and "null" in _err()
    assert lib.obte_block_decode_paged(C.byref(d), P, P, P, 4, P, 2, P, 128, P, need, None) == EINVAL and "max_pos = 128" in _err()
    assert lib.obte_block_decode_paged(C.byref(d), P, P, P, 4, P, 2, P, 5, P, need - 1, None) == EINVAL and "workspace" in _err()
    assert lib.obte_block_decode_paged(C.byref(d), P, P, P, 0, P, 2, P, 5, P, need, None) == EINVAL and "n_pages" in _err()
    d.T = 130
    need = lib.obte_block_infer_ws_bytes(2, 130, 256, 2)
    assert lib.obte_block_fwd_prefill_paged(C.byref(d), P, P, P, need, P, 4, P, 2, None) == EINVAL and "130 positions do not fit the table's 128" in _err()
    assert lib.obte_block_fwd_prefill_paged(C.byref(d), P, P, P, need, None, 4, P, 3, None) == EINVAL and "obte_block_fwd_prefill_paged: null" in _err()
    assert lib.obte_block_fwd_prefill_paged(C.byref(d), P, P, P, need - 1, P, 4, P, 3, None) == EINVAL and "workspace" in _err()
