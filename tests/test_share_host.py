"""Host-side tests (no GPU) of prompt pages shared between the rows of a paged cache: the PageBook's reference counts, the PrefixIndex
(exact content of whole pages, chained from position 0), the schedule's invariant over seeded random workloads with shared prefixes, the
argument checks of the three entry points of include/omnibiote_hip_paged_extend.h that return before a launch, and the refusals of
prefill(shared_pages=) and generate_many(share_prefix=True)."""
import ctypes as C
import random

import pytest
import torch

from omnibiote_amd import _lib
from omnibiote_amd.paged import PageBook, PagedSchedule, PrefixIndex, pages_for

EINVAL = -1
P = 4096   # a non-null, 16-byte aligned "pointer" for calls that must return before they touch it


def _err():
    return _lib.lib().obte_last_error().decode()


# ------------------------------------------------------------------------------------------------------- the book's counts
def test_page_book_counts_share_and_release_in_either_order():
    for owner_first in (True, False):
        b = PageBook(3, 8, 256, free_order=[5, 1, 7, 0, 2, 3, 4, 6])
        assert b.assign(0, 150) == [5, 1, 7] and b.refs[5] == b.refs[1] == b.refs[7] == 1
        assert b.assign_shared(1, [5, 1]) == [] and b.refs[5] == b.refs[1] == 2 and b.refs[7] == 1
        assert b.table[1].tolist() == [5, 1, -1, -1] and b.row_pages[1] == [5, 1] and b.pages_in_use == 3
        assert b.assign(1, 190) == [0] and b.table[1].tolist() == [5, 1, 0, -1] and b.pages_in_use == 4   # its own page behind the shared ones
        first, second = (0, 1) if owner_first else (1, 0)
        gone = b.release(first)
        assert gone == ([7] if owner_first else [0])                    # only what reached zero
        assert b.refs[5] == b.refs[1] == 1 and b.pages_in_use == 3 and b.free == [2, 3, 4, 6] + gone
        assert (b.table[first] == -1).all() and b.row_pos[first] == -1
        assert b.table[second, :2].tolist() == [5, 1]                   # the other row still names them
        rest = b.release(second)
        assert rest == ([5, 1, 0] if owner_first else [5, 1, 7])        # in the row's order, behind what was free
        assert b.free == [2, 3, 4, 6] + gone + rest and b.pages_in_use == 0 and b.refs == [0] * 8 and (b.table == -1).all()


def test_page_book_revives_a_released_page_and_tells_who_asks_when_one_is_handed_out():
    b = PageBook(2, 4, 256)
    told = []
    b.on_hand_out = told.append
    assert b.assign(0, 128) == [0, 1] and told == [0, 1]
    assert b.release(0) == [0, 1] and b.free == [2, 3, 0, 1] and b.pages_in_use == 0
    assert b.assign_shared(1, [1]) == [1] and told == [0, 1]            # revived: off the free list, its content stays, nobody is told
    assert b.free == [2, 3, 0] and b.refs == [0, 1, 0, 0] and b.pages_in_use == 1 and b.table[1].tolist() == [1, -1, -1, -1]
    assert b.assign(1, 100) == [2] and told == [0, 1, 2]                # the rest of the row from the front of the list
    assert b.assign(0, 128) == [3, 0] and told == [0, 1, 2, 3, 0]       # page 0 gets new content
    assert b.release(1) == [1, 2] and b.release(0) == [3, 0] and b.free == [1, 2, 3, 0]


def test_page_book_refuses_sharing_into_a_row_that_holds_pages():
    b = PageBook(2, 4, 256)
    b.assign(0, 64), b.assign(1, 10)
    before = (b.table.clone(), list(b.free), list(b.refs))
    with pytest.raises(ValueError, match="row 1 still holds 1 pages"):
        b.assign_shared(1, [0])
    b.release(1)
    before = (b.table.clone(), list(b.free), list(b.refs))
    for pages, word in (([4], "outside the pool"), ([-1], "outside the pool"), ([0, 0], "distinct"), ([0, 1, 2, 3, 0], "at most 4")):
        with pytest.raises(ValueError, match=word):
            b.assign_shared(1, pages)
    with pytest.raises(ValueError, match="row 2"):
        b.assign_shared(2, [0])
    assert torch.equal(b.table, before[0]) and b.free == before[1] and b.refs == before[2]


# ------------------------------------------------------------------------------------------------------- the index
def _toks(rng, n):
    return [rng.randrange(4, 512) for _ in range(n)]


def test_prefix_index_longest_match_and_never_the_whole_prompt():
    rng = random.Random(0)
    base = _toks(rng, 200)
    ix = PrefixIndex()
    ix.register(base, [7, 3, 9, 11])                                   # 200 tokens cover 3 pages; the fourth id is not looked at
    assert len(ix) == 3
    assert ix.lookup(base) == [7, 3, 9] and ix.lookup(base[:193]) == [7, 3, 9] and ix.lookup(base[:192]) == [7, 3]
    # never the whole prompt: one token at least is left to compute
    assert ix.lookup(base[:64]) == [] and ix.lookup(base[:65]) == [7] and ix.lookup(base[:128]) == [7] and ix.lookup(base[:129]) == [7, 3]
    assert ix.lookup([]) == [] and ix.lookup(base[:1]) == []
    # the longest chain: a prompt that leaves the base inside its third page
    other = base[:150] + _toks(rng, 100)
    assert ix.lookup(other) == [7, 3]
    ix.register(other, [7, 3, 20])
    assert ix.lookup(other) == [7, 3, 20] and ix.lookup(base) == [7, 3, 9] and len(ix) == 4
    assert ix.lookup(torch.tensor(other)) == [7, 3, 20]                 # a 1-D tensor is read as its tokens
    # a chain that is recorded keeps its page
    ix.register(base, [30, 31, 32])
    assert ix.lookup(base) == [7, 3, 9]
    with pytest.raises(ValueError, match="cover 3 pages"):
        ix.register(base, [1, 2])


def test_prefix_index_matches_exact_content_only():
    rng = random.Random(1)
    a = _toks(rng, 130)
    b = [a[0] + 1] + a[1:]                                              # the same last 63 tokens of page 0, the same page 1
    ix = PrefixIndex()
    ix.register(a, [0, 1])
    assert ix.lookup(a) == [0, 1] and ix.lookup(b) == []                # nothing: the chain starts at position 0
    c = a[:64] + [a[64] + 1] + a[65:]                                   # page 1 differs in its first token
    assert ix.lookup(c) == [0]
    d = a[64:] + a[:64] + [5]                                           # page 1's content at position 0: another key (its parent differs)
    assert ix.lookup(d) == []


def test_prefix_index_forgets_what_is_handed_out_again():
    rng = random.Random(2)
    a = _toks(rng, 200)
    book = PageBook(2, 4, 256)
    ix = PrefixIndex(book)
    assert book.assign(0, 200) == [0, 1, 2, 3]
    ix.register(a, book.row_pages[0])
    assert ix.lookup(a) == [0, 1, 2]
    book.release(0)
    assert ix.lookup(a) == [0, 1, 2]                                    # released and still findable: the free list keeps it
    assert book.assign(1, 10) == [0] and ix.lookup(a) == []             # page 0 handed out again: the chain starts with it
    book.release(1)
    ix.register(a, [0, 1, 2])                                           # (page 0 refilled with the same tokens)
    assert ix.lookup(a) == [0, 1, 2]
    ix.forget(1)                                                        # a middle page: the chain stops there
    assert ix.lookup(a) == [0]
    ix.register(a, [0, 3, 2])                                           # a new middle page is a new node: what lay behind the old one stays lost
    assert ix.lookup(a) == [0, 3, 2] and len(ix) == 3
    ix.forget(17)                                                       # (a page the index does not know)


# ------------------------------------------------------------------------------------------------------- the schedule's invariant
def _drive_shared(prompts, max_new, batch, n_pages, rng):
    """generate_many(share_prefix=True)'s host side without a model: PagedSchedule admits, every admitted request takes the longest
    chain the PrefixIndex finds (assign_shared) and pages of its own for the rest (assign: must never fail), registers its prompt, grows
    by one position per step and is released at a random end.  Returns (shared positions, peak pages in use)."""
    lengths = [len(p) for p in prompts]
    s = PagedSchedule(lengths, max_new, batch, n_pages, block_size=None)
    book = PageBook(batch, s.n_pages, max(lengths) + max_new, free_order=rng.sample(range(s.n_pages), s.n_pages))
    ix = PrefixIndex(book)
    ends = [rng.randint(1, max_new) for _ in prompts]
    made, running, shared, peak = [0] * len(prompts), {}, 0, 0
    guard = 0
    while not s.done:
        guard += 1
        assert guard < 10 * (sum(ends) + len(prompts)), "the schedule does not end"
        for r, slot in s.admit():
            found = ix.lookup(prompts[r])
            assert 64 * len(found) < lengths[r]
            book.assign_shared(slot, found)
            book.assign(slot, lengths[r])                               # (never raises: the promise covers it)
            book.place(slot, lengths[r])
            ix.register(prompts[r], book.row_pages[slot])
            running[r] = slot
            shared += 64 * len(found)
        assert running, "nothing runs and nothing was admitted"
        # the invariants: distinct pages in use never exceed the promise, the counts are the number of rows that name each page
        assert s.promised == sum(s.need[r] for r in running) <= s.n_pages
        assert book.pages_in_use <= s.promised
        named = [p for slot in running.values() for p in book.row_pages[slot]]
        assert [named.count(p) for p in range(s.n_pages)] == book.refs
        assert book.pages_in_use == len(set(named)) and not set(named) & set(book.free)
        for r, slot in running.items():
            assert len(book.row_pages[slot]) <= s.need[r]
            assert book.table[slot, :len(book.row_pages[slot])].tolist() == book.row_pages[slot]
        for page in ix.key_of:                                          # an indexed page is in use or waits on the free list with its content
            assert book.refs[page] > 0 or page in book.free
        peak = max(peak, book.pages_in_use)
        for r in list(running):
            made[r] += 1
            if made[r] == ends[r]:
                book.release(s.finish(r))
                del running[r]
        if running:
            book.grow_for_step()                                        # (never raises either)
            book.step()
    assert made == ends and book.pages_in_use == 0 and sorted(book.free) == list(range(s.n_pages)) and book.refs == [0] * s.n_pages
    assert s.promised == 0 and (book.table == -1).all()
    return shared, peak


@pytest.mark.parametrize("seed", range(8))
def test_schedule_invariant_with_shared_prefixes(seed):
    rng = random.Random(seed)
    prefixes = [_toks(rng, rng.choice([64, 100, 128, 200, 300])) for _ in range(rng.randint(1, 3))]
    prompts = [rng.choice(prefixes) + _toks(rng, rng.randint(1, 150)) for _ in range(rng.randint(2, 40))]
    max_new = rng.randint(1, 200)
    batch = rng.randint(1, 9)
    largest = max(pages_for(len(p) + max_new) for p in prompts)
    n_pages = rng.choice([None, largest, largest + rng.randint(0, 3 * largest)])
    shared, peak = _drive_shared(prompts, max_new, batch, n_pages, rng)
    assert peak <= (batch * largest if n_pages is None else n_pages)
    if batch > 1 and n_pages is None and len(prompts) > len(prefixes):
        assert shared > 0                                               # (some request ran beside, or soon after, one with its prefix)


# ------------------------------------------------------------------------------------------------------- entry points and symbols
def test_paged_extend_symbols_and_abi():
    names = ["obte_attn_extend_paged", "obte_kv_paged_rope_store_chunk", "obte_block_extend_paged"]
    assert list(_lib.SYMBOLS_PAGED_EXTEND) == names
    lib = _lib.lib()
    header = open(__file__.rsplit("/tests/", 1)[0] + "/include/omnibiote_hip_paged_extend.h").read()
    for n in names:
        assert getattr(lib, n).argtypes == _lib.SYMBOLS_PAGED_EXTEND[n][1]
        assert n + "(" in header
    at = [header.index("int " + n + "(") for n in names]
    assert at == sorted(at)                                             # the table keeps the header's order
    assert "kind 120" in header and lib.obte_abi_version() == 1


def _call_attn(q=P, q_ld=128, pool=P, n_pages=4, table=P, ld=2, o=P, lse=None, B=1, n=5, pos=10, pos_rows=P, H=1, hs=128, splits=1, ws=None, ws_bytes=0):
    return _lib.lib().obte_attn_extend_paged(q, q_ld, pool, n_pages, table, ld, o, lse, B, n, pos, pos_rows, H, hs, 1.0, splits, ws, ws_bytes, None)


def _call_store(qkv=P, cos=P, sin=P, pos_rows=P, max_pos=10, B=1, n=5, H=1, hs=128, pool=P, n_pages=4, table=P, ld=2):
    return _lib.lib().obte_kv_paged_rope_store_chunk(qkv, cos, sin, pos_rows, max_pos, B, n, H, hs, pool, n_pages, table, ld, None)


@pytest.mark.parametrize("call,name,kw,word", [
    (_call_attn, "obte_attn_extend_paged", dict(q=None), "null"), (_call_attn, "obte_attn_extend_paged", dict(table=None), "null"),
    (_call_attn, "obte_attn_extend_paged", dict(pos_rows=None), "null"), (_call_attn, "obte_attn_extend_paged", dict(pool=None), "null"),
    (_call_attn, "obte_attn_extend_paged", dict(hs=32), "head_dim"), (_call_attn, "obte_attn_extend_paged", dict(n_pages=0), "shape"),
    (_call_attn, "obte_attn_extend_paged", dict(pos=124), "[124, 129) do not fit the table's [0, 64 * table_ld = 128)"),
    (_call_attn, "obte_attn_extend_paged", dict(pos=-1), "do not fit"), (_call_attn, "obte_attn_extend_paged", dict(n=0), "n_new"),
    (_call_attn, "obte_attn_extend_paged", dict(pool=P + 8), "aligned"), (_call_attn, "obte_attn_extend_paged", dict(table=P + 2), "aligned"),
    (_call_attn, "obte_attn_extend_paged", dict(q_ld=64), "q_ld"), (_call_attn, "obte_attn_extend_paged", dict(splits=33), "splits"),
    (_call_attn, "obte_attn_extend_paged", dict(splits=2, ws=P, ws_bytes=64), "workspace"),
    (_call_store, "obte_kv_paged_rope_store_chunk", dict(qkv=None), "null"), (_call_store, "obte_kv_paged_rope_store_chunk", dict(table=None), "null"),
    (_call_store, "obte_kv_paged_rope_store_chunk", dict(hs=32), "head_dim"), (_call_store, "obte_kv_paged_rope_store_chunk", dict(n=0), "shape"),
    (_call_store, "obte_kv_paged_rope_store_chunk", dict(max_pos=124), "124 + 5 do not fit the table's [0, 64 * table_ld = 128)"),
    (_call_store, "obte_kv_paged_rope_store_chunk", dict(max_pos=-1), "do not fit"),
    (_call_store, "obte_kv_paged_rope_store_chunk", dict(pool=P + 8), "aligned"), (_call_store, "obte_kv_paged_rope_store_chunk", dict(pos_rows=P + 2), "aligned"),
])
def test_paged_extend_entry_points_reject_before_any_launch(call, name, kw, word):
    assert call(**kw) == EINVAL
    assert _err().startswith(name + ":") and word in _err(), _err()


def test_paged_block_extend_rejects_before_any_launch():
    lib = _lib.lib()
    d = _lib.BlockDesc(B=2, T=5, n_embd=256, n_head=2, ln1_w=P, attn_w=P, proj_w=P, ln2_w=P, fc_w=P, mlp_w=P, rope_cos=P, rope_sin=P)
    need = lib.obte_block_extend_ws_bytes(2, 5, 256, 2)
    call = lambda pool=P, n_pages=4, table=P, ld=2, pos=10, pos_rows=P, ws=P, nbytes=need: lib.obte_block_extend_paged(   # noqa: E731
        C.byref(d), P, P, pool, n_pages, table, ld, pos, pos_rows, ws, nbytes, None)
    for kw, word in ((dict(pool=None), "obte_block_extend_paged: null"), (dict(table=None), "null"), (dict(pos_rows=None), "null"),
                     (dict(pos=124), "[124, 129) (d->T = 5 new ones) do not fit the cache's [0, 128)"), (dict(pos=-1), "do not fit"),
                     (dict(nbytes=need - 1), "workspace"), (dict(n_pages=0), "n_pages"), (dict(pool=P + 8), "aligned"), (dict(table=P + 2), "aligned")):
        assert call(**kw) == EINVAL and _err().startswith("obte_block_extend_paged:") and word in _err(), (kw, _err())
    d.n_embd, d.n_head = 64, 2                                          # head_dim 32
    assert call() != 0 and "obte_block_extend_paged" in _err(), _err()


# ------------------------------------------------------------------------------------------------------- the refusals
def _cpu_model(block_size=200):
    from omnibiote_amd.model import OmniBioTA, OmniBioTAConfig
    c = OmniBioTAConfig()
    c.block_size, c.vocab_size, c.n_layer, c.n_head, c.n_embd, c.dropout, c.flash = block_size, 64, 1, 2, 128, 0.0, True
    c.autoregressive = True
    return OmniBioTA(c)


def _fake(batch=3, n_pages=6, max_len=200):
    from omnibiote_amd.model import PagedPositions
    c = PagedPositions(batch, n_pages, max_len)
    c.layers, c.decode_ws, c.extend_ws = [None], None, None
    return c


def test_start_rows_with_shared_pages_is_all_or_nothing_and_counts_what_the_free_list_must_give():
    c = _fake(n_pages=4)
    c.start_rows([0], [130])                                            # pages 0, 1, 2
    assert c.table.tolist()[0] == [0, 1, 2, -1]
    c.start_rows([1], [190], shared=[[0, 1]])                           # one page of its own: the last free one
    assert c.table.tolist()[1] == [0, 1, 3, -1] and c.pages_in_use == 4 and c.positions.tolist() == [130, 190, -1] and c.book.refs == [2, 2, 1, 1]
    c.release(0)                                                        # page 2 is free; 0 and 1 live on in row 1
    assert c.pages_in_use == 3 and c.book.free == [2]
    state = lambda: (c.table.tolist(), c.positions.tolist(), list(c.book.free), list(c.book.refs))   # noqa: E731
    before = state()
    with pytest.raises(ValueError, match="need 2 more pages and 1 of 4 are free"):
        c.start_rows([0, 2], [100, 70], shared=[[0], [0]])              # each needs a page of its own behind page 0
    with pytest.raises(ValueError, match="cover the whole prompt"):
        c.start_rows([0], [128], shared=[[0, 1]])
    with pytest.raises(ValueError, match="outside the pool"):
        c.start_rows([0], [100], shared=[[4]])
    with pytest.raises(ValueError, match="row 1 still holds"):
        c.start_rows([1], [100], shared=[[0]])
    assert state() == before
    c.release(1)                                                        # everything free: [2, 0, 1, 3]
    # a revived page is not counted twice: row 0 revives 0 and 1 and needs one more, row 2 needs one: two of the two that stay free
    c.start_rows([0, 2], [150, 10], shared=[[0, 1], []])
    assert c.table.tolist()[0] == [0, 1, 2, -1] and c.table.tolist()[2] == [3, -1, -1, -1] and c.book.free == []


def test_shared_pages_and_share_prefix_refuse_before_any_state_changes():
    from omnibiote_amd.model import CachePositions, QuantizedWeights
    m = _cpu_model()
    c = _fake()
    c.start_rows([0], [150])
    state = lambda: (c.positions.tolist(), c.table.tolist(), c.pages_in_use, c.pos, list(c.book.free), list(c.book.refs))   # noqa: E731
    before = state()
    tok = torch.zeros(1, 190, dtype=torch.int64)
    w = QuantizedWeights.__new__(QuantizedWeights)
    with pytest.raises(NotImplementedError, match=r"prefill: weights= .* paged cache"):
        m.prefill(tok, c, rows=[1], shared_pages=[[0, 1]], weights=w)
    c.dtype = "fp8"
    with pytest.raises(NotImplementedError, match=r"shared_pages= on an fp8 pool"):
        m.prefill(tok, c, rows=[1], shared_pages=[[0, 1]])
    del c.dtype
    plain = CachePositions(1, 200)
    with pytest.raises(NotImplementedError, match=r"shared_pages= names pages of a PagedKVCache"):
        m.prefill(tok, plain, shared_pages=[[0, 1]])
    with pytest.raises(ValueError, match="outside the pool"):
        m.prefill(tok, c, rows=[1], shared_pages=[[0, 6]])
    with pytest.raises(ValueError, match="cover the whole prompt"):
        m.prefill(tok[:, :128], c, rows=[1], shared_pages=[[0, 1]])
    with pytest.raises(ValueError, match="cover the whole prompt"):
        m.prefill(tok, c, rows=[1], lengths=[64], shared_pages=[[0]])
    with pytest.raises(ValueError, match="row 0 still holds 3 pages"):
        m.prefill(tok, c, rows=[0], shared_pages=[[0, 1]])
    with pytest.raises(ValueError, match="2 lists of shared pages for 1 rows"):
        m.prefill(tok, c, rows=[1], shared_pages=[[0], [1]])
    assert state() == before
    # the old refusals of a paged cache stand beside the new keyword
    with pytest.raises(NotImplementedError, match=r"extend: the cache is a paged cache"):
        m.extend(tok[:, :4], _fake(batch=1))
    with pytest.raises(NotImplementedError, match=r"prefill\(chunk=\): the cache is a paged cache"):
        m.prefill(tok, c, rows=[1], chunk=64, shared_pages=[[0, 1]])
    assert state() == before
    p = [torch.zeros(70, dtype=torch.int64), torch.zeros(90, dtype=torch.int64)]
    with pytest.raises(NotImplementedError, match=r"share_prefix=True needs kv_dtype='bf16'"):
        m.generate_many(p, 5, batch=2, kv_dtype="fp8", share_prefix=True)
    with pytest.raises(ValueError, match="exceed block_size = 200"):
        m.generate_many(p, 120, batch=2, share_prefix=True)
    assert m.generate_many([], 5, batch=2, share_prefix=True, stats={}) == []
