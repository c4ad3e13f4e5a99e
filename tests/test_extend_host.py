"""Host-side tests (no GPU) of continuing a filled key/value cache by several positions per row (include/omnibiote_hip_extend.h): the
symbol table against the header, the pins of the ABI, the default split rule of obte_attn_extend, the workspace sizes, every argument
check that returns before a launch, and the validation of OmniBioTA.extend / KVCache.rewind / prefill(chunk=) on a CPU model with a
cache's position state alone, and that state's own transitions."""
import ctypes as C
import os
import re

import pytest
import torch

from omnibiote_amd import _lib

EINVAL, EUNSUPPORTED = -1, -3
MAX = _lib.ATTN_EXTEND_MAX_SPLITS
P = 4096   # a non-null, 16-byte aligned "pointer" for calls that must return before they touch it
NAMES = ("obte_attn_extend_splits", "obte_attn_extend_ws_bytes", "obte_kv_cache_rope_store_chunk", "obte_attn_extend", "obte_block_extend_ws_bytes",
         "obte_block_extend")


def _err():
    return _lib.lib().obte_last_error().decode()


def test_symbols_are_what_the_header_declares():
    assert tuple(_lib.SYMBOLS_EXTEND) == NAMES
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "omnibiote_hip_extend.h")).read()
    body = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    assert tuple(re.findall(r"\b(obte_\w+)\s*\(", body)) == NAMES                  # the declarations, in order
    assert '#include "omnibiote_hip.h"' in header
    assert re.search(r"#define\s+OBTE_ATTN_EXTEND_MAX_SPLITS\s+%d\b" % MAX, header)
    for name in NAMES:
        assert name not in _lib.SYMBOLS and name not in _lib.SYMBOLS_ROWS and name not in _lib.SYMBOLS_SMALL_M and name not in _lib.SYMBOLS_SAMPLE
        assert hasattr(_lib.lib(), name)
    assert len(_lib.SYMBOLS) == 70 and len(_lib.SYMBOLS_ROWS) == 3 and len(_lib.SYMBOLS_SMALL_M) == 3 and len(_lib.SYMBOLS_SAMPLE) == 1


def test_abi_pins_hold():
    lib = _lib.lib()
    assert lib.obte_abi_version() == 1
    sizes = (C.c_int64 * 16)()
    assert lib.obte_struct_sizes(sizes, 16) == 6


def test_default_split_rule():
    lib = _lib.lib()
    keys = [1, 2, 31, 32, 33, 64, 128, 255, 256, 257, 600, 1024, 1100, 2048, 4096, 65536]
    heads = [(1, 1), (1, 8), (2, 2), (8, 8), (64, 8), (256, 16)]
    for hs in (64, 128):
        for n in (1, 2, 8, 32, 33, 64, 128, 1000):
            table = {}
            for B, H in heads:
                row = [lib.obte_attn_extend_splits(B, H, hs, n, k) for k in keys]
                assert all(1 <= v <= MAX for v in row), row
                assert row == [lib.obte_attn_extend_splits(B, H, hs, n, k) for k in keys]   # a pure function
                assert all(a <= b for a, b in zip(row, row[1:])), row                        # never fewer splits for more keys
                table[B * H] = row
                # the workspace at splits = 0 serves whatever the rule returns for these (B, H, hs, n)
                assert lib.obte_attn_extend_ws_bytes(B, H, hs, n, 0) >= lib.obte_attn_extend_ws_bytes(B, H, hs, n, max(row))
            order = sorted(table)
            for lo, hi in zip(order, order[1:]):                                             # never more splits for more (b, h)
                assert all(a >= b for a, b in zip(table[lo], table[hi])), (lo, hi)
    # below the rule's own minimum of keys per split there is nothing to split
    smallest = min(k for k in range(1, 4097) if lib.obte_attn_extend_splits(1, 1, 128, 8, k) > 1)
    assert smallest >= 64
    for k in (1, smallest // 2, smallest - 1):
        for B, H in heads:
            assert lib.obte_attn_extend_splits(B, H, 128, 8, k) == 1
    assert lib.obte_attn_extend_splits(1, 1, 128, 8, 65536) > 1                              # and it does split
    assert lib.obte_attn_extend_splits(1, 1, 32, 8, 65536) == 1 and lib.obte_attn_extend_splits(0, 1, 128, 8, 65536) == 1


def test_workspace_sizes():
    lib = _lib.lib()
    for B, H, hs, n in [(2, 2, 64, 5), (8, 8, 128, 33), (1, 1, 128, 1), (2, 2, 128, 128)]:
        one = lib.obte_attn_extend_ws_bytes(B, H, hs, n, 1)
        assert one >= B * H * n * (hs + 2) * 4                     # fp32 (O, m, l) of every query at least
        assert lib.obte_attn_extend_ws_bytes(B, H, hs, n, 7) == 7 * one
        assert lib.obte_attn_extend_ws_bytes(B, H, hs, n, 0) >= one
        total = lib.obte_block_extend_ws_bytes(B, n, H * hs, H)
        assert total >= lib.obte_block_infer_ws_bytes(B, n, H * hs, H) + lib.obte_attn_extend_ws_bytes(B, H, hs, n, 0) > 0
    assert lib.obte_attn_extend_ws_bytes(2, 2, 32, 5, 0) == 0      # head size 32
    assert lib.obte_attn_extend_ws_bytes(0, 2, 64, 5, 0) == 0
    assert lib.obte_attn_extend_ws_bytes(2, 2, 64, 0, 0) == 0
    assert lib.obte_attn_extend_ws_bytes(2, 2, 64, 5, MAX + 1) == 0
    assert lib.obte_block_extend_ws_bytes(2, 5, 128, 4) == 0       # head size 32
    assert lib.obte_block_extend_ws_bytes(0, 5, 256, 2) == 0 and lib.obte_block_extend_ws_bytes(2, 0, 256, 2) == 0


def _call_extend(q=P, q_ld=128, cache=P, o=P, lse=None, B=1, T_max=100, n=4, pos=10, pos_rows=None, H=1, hs=128, splits=1, ws=None, ws_bytes=0):
    return _lib.lib().obte_attn_extend(q, q_ld, cache, o, lse, B, T_max, n, pos, pos_rows, H, hs, 1.0, splits, ws, ws_bytes, None)


@pytest.mark.parametrize("kw,word", [
    (dict(q=None), "null"), (dict(cache=None), "null"), (dict(o=None), "null"),
    (dict(n=0), "n_new"), (dict(pos=97), "fit"), (dict(pos=-1), "fit"), (dict(pos=100, n=1), "fit"),
    (dict(splits=-1), "splits"), (dict(splits=MAX + 1), "splits"),
    (dict(splits=2), "workspace"), (dict(splits=2, ws=P, ws_bytes=64), "workspace"), (dict(splits=2, ws=P + 4, ws_bytes=1 << 30), "workspace"),
    (dict(hs=32, q_ld=32), "head_dim"), (dict(q_ld=132), "q_ld"), (dict(q_ld=64), "q_ld"), (dict(q=P + 8), "aligned"),
    (dict(B=0), "shape"), (dict(pos_rows=P + 2), "aligned"),
])
def test_attn_extend_rejects_before_any_launch(kw, word):
    assert _call_extend(**kw) == EINVAL
    assert _err().startswith("obte_attn_extend:") and word in _err(), _err()


def test_rope_store_chunk_rejects_before_any_launch():
    lib = _lib.lib()

    def store(qkv=P, cos=P, sin=P, pos=P, max_pos=10, B=2, n=4, H=2, hs=64, cache=P, T_max=100):
        return lib.obte_kv_cache_rope_store_chunk(qkv, cos, sin, pos, max_pos, B, n, H, hs, cache, T_max, None)
    for kw, word in [(dict(qkv=None), "null"), (dict(pos=None), "null"), (dict(cache=None), "null"), (dict(cos=None), "null"), (dict(n=0), "shape"),
                     (dict(hs=32), "shape"), (dict(max_pos=97), "fit"), (dict(max_pos=-1), "fit"), (dict(pos=P + 2), "aligned"), (dict(qkv=P + 8), "aligned")]:
        assert store(**kw) == EINVAL, kw
        assert _err().startswith("obte_kv_cache_rope_store_chunk:") and word in _err(), (kw, _err())


def _desc(B=2, T=4, C_=256, H=2, **over):
    f = dict(B=B, T=T, n_embd=C_, n_head=H, ln1_w=P, attn_w=P, proj_w=P, ln2_w=P, fc_w=P, mlp_w=P, rope_cos=P, rope_sin=P)
    f.update(over)
    return _lib.BlockDesc(**f)


def test_block_extend_rejects_before_any_launch():
    lib = _lib.lib()
    big = 1 << 30

    def extend(d, x=P, y=P, kv=P, T_max=100, pos=5, pos_rows=None, ws=P, ws_bytes=big):
        return lib.obte_block_extend(C.byref(d) if d is not None else None, x, y, kv, T_max, pos, pos_rows, ws, ws_bytes, None)
    assert extend(None) == EINVAL and "obte_block_extend" in _err() and "null" in _err()
    for over in (dict(key_ranges=P), dict(out_rows=P, n_out_rows=1), dict(dropout_p=0.1), dict(mask=P), dict(query_bounds=P)):
        assert extend(_desc(**over)) == EUNSUPPORTED, over
        assert _err().startswith("obte_block_extend:"), _err()
    assert extend(_desc(), x=None) == EINVAL and "null" in _err()
    assert extend(_desc(), kv=None) == EINVAL and "null" in _err()
    assert extend(_desc(), ws=None) == EINVAL and "null" in _err()
    assert extend(_desc(T=0)) == EINVAL
    assert extend(_desc(T=96)) == EINVAL                                 # d->T new positions from 5 on do not fit 100
    assert _err().startswith("obte_block_extend:") and "d->T" in _err(), _err()
    assert extend(_desc(), pos=97) == EINVAL and "fit" in _err()
    assert extend(_desc(), pos=-1) == EINVAL and "fit" in _err()
    assert extend(_desc(), ws_bytes=lib.obte_block_extend_ws_bytes(2, 4, 256, 2) - 1) == EINVAL
    assert _err().startswith("obte_block_extend:") and "workspace" in _err(), _err()
    assert extend(_desc(C_=128, H=4)) == EINVAL                          # head size 32


# ------------------------------------------------------------------------------------------------------- the model surface
def _cpu_model(autoregressive=True, block_size=32):
    from omnibiote_amd.model import OmniBioTA, OmniBioTAConfig
    c = OmniBioTAConfig()
    c.block_size, c.vocab_size, c.n_layer, c.n_head, c.n_embd, c.dropout, c.flash = block_size, 64, 1, 2, 128, 0.0, True
    c.autoregressive = autoregressive
    return OmniBioTA(c)


def _fake(pos=8, batch=2, max_len=32, positions=None, min_pos=0):
    """a cache's position state (the host-only class KVCache is built on) with no buffer behind it"""
    from omnibiote_amd.model import CachePositions
    c = CachePositions(batch, max_len)
    c.reset(pos, positions, min_pos)
    c.layers, c.decode_ws, c.extend_ws = [None], None, None
    return c


def test_extend_validates_before_any_device_work():
    m = _cpu_model()
    tok = torch.zeros(2, 4, dtype=torch.int64)
    with pytest.raises(ValueError, match=r"\(B, n\)"):
        m.extend(torch.zeros(2, dtype=torch.int64), _fake())
    with pytest.raises(ValueError, match=r"\(B, n\)"):
        m.extend(torch.zeros(2, 4, 1, dtype=torch.int64), _fake())
    with pytest.raises(ValueError, match="n = 0"):
        m.extend(torch.zeros(2, 0, dtype=torch.int64), _fake())
    with pytest.raises(ValueError, match="batch"):
        m.extend(tok, _fake(batch=3))
    with pytest.raises(ValueError, match="empty"):
        m.extend(tok, _fake(pos=0))
    with pytest.raises(ValueError, match="positions are full"):
        m.extend(tok, _fake(pos=29))                                                     # 29 + 4 > 32
    with pytest.raises(ValueError, match="positions are full"):
        m.extend(tok, _fake(pos=29, positions=torch.tensor([20, 29], dtype=torch.int32)))
    with pytest.raises(ValueError, match="logits"):
        m.extend(tok, _fake(), logits="first")
    with pytest.raises(ValueError, match="autoregressive"):
        _cpu_model(False).extend(tok, _fake())
    c = _fake(pos=28)
    with pytest.raises(RuntimeError, match="GPU"):                                       # it fits: the first device-side requirement
        m.extend(tok, c)
    assert c.pos == 28


def test_rewind():
    from omnibiote_amd.model import KVCache
    c = _fake(pos=8)
    KVCache.rewind(c, 5)
    assert c.pos == 3
    KVCache.rewind(c, 0)
    KVCache.rewind(c, 2)
    assert c.pos == 1
    with pytest.raises(ValueError, match="fewer than one"):
        KVCache.rewind(c, 1)
    with pytest.raises(ValueError, match="negative"):
        KVCache.rewind(c, -1)
    assert c.pos == 1
    r = _fake(pos=12, positions=torch.tensor([7, -1, 12], dtype=torch.int32), batch=3)
    KVCache.rewind(r, 5)
    assert r.positions.tolist() == [2, -1, 7] and r.positions.dtype == torch.int32 and r.max_pos == r.pos == 7
    KVCache.rewind(r, 1)
    assert r.positions.tolist() == [1, -1, 6] and r.max_pos == r.pos == 6
    with pytest.raises(ValueError, match="fewer than one"):
        KVCache.rewind(r, 1)                                                             # row 0 would be left empty
    assert r.positions.tolist() == [1, -1, 6] and r.max_pos == 6


def test_rewind_waits_for_the_device_only_where_the_host_bound_does_not_settle_it():
    from omnibiote_amd.model import KVCache

    class Positions:
        """stands for the device tensor: counts the reads that would synchronise"""
        def __init__(self, values):
            self.t, self.reads = torch.tensor(values, dtype=torch.int32), 0
        def tolist(self):
            self.reads += 1
            return self.t.tolist()
        def __sub__(self, other):
            return Positions((self.t - other).tolist())
        def __ge__(self, other):
            return self.t >= other

    r = _fake(pos=20, positions=Positions([12, -1, 20]), batch=3, min_pos=12)            # as prefill(lengths=) and extend leave it
    first = r.positions
    KVCache.rewind(r, 5)
    assert first.reads == 0 and r.positions.t.tolist() == [7, -1, 15] and r.min_pos == 7 and r.max_pos == r.pos == 15
    second = r.positions
    with pytest.raises(ValueError, match="fewer than one"):                              # the bound cannot say: the positions are read
        KVCache.rewind(r, 7)
    assert second.reads == 1 and r.positions is second and r.min_pos == 7 and r.max_pos == 15


def test_extend_workspace_is_judged_by_its_bytes():
    """obte_block_extend_ws_bytes is not monotone in n (the partials follow the default split count): whatever the order of the calls,
    the buffer kept on the cache holds what the call at hand asks for, and is kept while it does"""
    m, lib = _cpu_model(), _lib.lib()
    need = lambda n: lib.obte_block_extend_ws_bytes(2, n, 128, 2)
    sizes = [need(n) for n in range(1, 301)]
    assert min(sizes) > 0
    assert need(65) < need(64) and need(257) < need(256)                                 # (the drops this test is about)
    c = _fake()
    order = [65, 64, 66, 257, 256, 2] + list(range(300, 0, -1)) + list(range(1, 301))
    grown = 0
    for n in order:
        before = getattr(c, "extend_ws", None)
        ws = m._extend_ws(c, "cpu", n)
        assert ws is c.extend_ws and ws.dtype == torch.uint8 and ws.numel() >= need(n), n
        if before is not None and before.numel() >= need(n):
            assert ws is before, n
        grown += ws is not before
    assert c.extend_ws.numel() == max(sizes) and grown < 20
    c = _fake()
    assert m._extend_ws(c, "cpu", 66, 64).numel() == max(need(66), need(64))             # prefill(chunk=66) on 130 tokens: one buffer for both


def test_prefill_and_decode_step_fail_first_at_the_device():
    m = _cpu_model()
    idx = torch.zeros(2, 8, dtype=torch.int64)
    with pytest.raises(ValueError, match="chunk"):
        m.prefill(idx, _fake(pos=0), chunk=0)
    with pytest.raises(ValueError, match="chunk"):
        m.prefill(idx, _fake(pos=0), chunk=-3)
    # every path on a cache state without buffers: its first device-side failure, no AttributeError
    for kw in (dict(), dict(chunk=None), dict(chunk=8), dict(chunk=100), dict(chunk=4), dict(lengths=[3, 8])):
        with pytest.raises(RuntimeError, match="MI355X|GPU"):
            m.prefill(idx, _fake(pos=0), **kw)
    with pytest.raises(RuntimeError, match="GPU"):
        m.decode_step(torch.zeros(2, dtype=torch.int64), _fake())
    with pytest.raises(RuntimeError, match="GPU"):
        m.decode_step(torch.zeros(2, dtype=torch.int64), _fake(positions=torch.tensor([3, 8], dtype=torch.int32)))
    with pytest.raises(RuntimeError, match="GPU"):                                       # n == 1 is decode_step
        m.extend(torch.zeros(2, 1, dtype=torch.int64), _fake())


# ------------------------------------------------------------------------------------------------------- the position state
def _i32(*v):
    return torch.tensor(v, dtype=torch.int32)


def _state(c):
    return c.pos, None if c.positions is None else c.positions.tolist(), c.min_pos, c.max_pos


def test_cache_positions_uniform():
    from omnibiote_amd.model import CachePositions
    c = CachePositions(2, 32)
    assert (c.batch, c.max_len) == (2, 32) and _state(c) == (0, None, 0, 0)
    c.reset(8)
    assert _state(c) == (8, None, 0, 0)                                                  # max_pos: 0 in uniform mode
    c.advance(5)
    c.advance(1)
    assert _state(c) == (14, None, 0, 0)
    c.rewind(6)
    assert _state(c) == (8, None, 0, 0)
    with pytest.raises(AttributeError):
        c.max_pos = 3                                                                    # read-only: pos is the one bound


def test_cache_positions_rows():
    from omnibiote_amd.model import CachePositions
    c = CachePositions(3, 32)
    at = _i32(7, 3, 12)
    c.reset(12, at, min_pos=3)
    assert c.positions is at and _state(c) == (12, [7, 3, 12], 3, 12)                    # the ready tensor is taken as it is; max_pos is pos
    c.advance(4)
    assert c.positions is not at and at.tolist() == [7, 3, 12]                           # a new tensor: queued launches read the old one
    assert c.positions.dtype == torch.int32 and _state(c) == (16, [11, 7, 16], 7, 16)
    c.advance(1)                                                                         # a decode step moves min_pos too
    assert c.positions.dtype == torch.int32 and _state(c) == (17, [12, 8, 17], 8, 17)
    before = c.positions
    c.park(torch.tensor([False, True, False]))
    assert c.positions is not before and c.positions.dtype == torch.int32 and _state(c) == (17, [12, -1, 17], 8, 17)
    c.advance(3)                                                                         # a parked row stays parked
    assert _state(c) == (20, [15, -1, 20], 11, 20)
    c.reset(5)                                                                           # back to uniform
    assert _state(c) == (5, None, 0, 0)


@pytest.mark.parametrize("positions", [None, (7, 3, 12), (7, -1, 12)])
@pytest.mark.parametrize("n", [1, 2, 9])
def test_advance_then_rewind_is_the_identity(positions, n):
    from omnibiote_amd.model import CachePositions
    c = CachePositions(3, 64)
    if positions is None:
        c.reset(12)
    else:
        c.reset(12, _i32(*positions), min_pos=3)
    was = _state(c)
    c.advance(n)
    assert c.pos == 12 + n
    c.rewind(n)
    assert _state(c) == was and (c.positions is None or c.positions.dtype == torch.int32)


def test_require_room_words_the_error_per_caller():
    from omnibiote_amd.model import CachePositions
    c = CachePositions(2, 32)
    c.reset(29, _i32(20, 29))
    c.require_room("extend", 3, detail=True)
    c.require_room("decode_step", 1)
    with pytest.raises(ValueError, match=r"OmniBioTA\.extend: the cache's 32 positions are full: 4 more from 29 do not fit"):
        c.require_room("extend", 4, detail=True)
    c.advance(3)
    with pytest.raises(ValueError, match=r"OmniBioTA\.decode_step: the cache's 32 positions are full$"):
        c.require_room("decode_step", 1)
