"""Host-side tests (no GPU) of the paged key/value cache in OCP e4m3 (include/omnibiote_hip_paged8.h): the symbol table and the pool's
size, the argument checks of every new entry point that return before a launch, the e4m3 gather / scatter references as pure functions,
the two new keywords, and the refusals that stay on a paged cache of either dtype."""
import ctypes as C

import pytest
import torch

from omnibiote_amd import _lib
from omnibiote_amd.paged import KV_PAGE, paged8_gather_reference, paged8_scatter_reference, pool8_bytes, pool_bytes

from test_paged_host import EINVAL, P, _cpu_model, _err, _fake

NAMES = ["obte_kv8_paged_bytes", "obte_kv8_paged_store", "obte_kv8_paged_rope_store_rows", "obte_attn_decode_paged8", "obte_block_fwd_prefill_paged8",
         "obte_block_decode_paged8"]


# ------------------------------------------------------------------------------------------------------- symbols and sizes
def test_paged8_symbols_sizes_and_abi():
    assert list(_lib.SYMBOLS_PAGED8) == NAMES
    lib = _lib.lib()
    for n in NAMES:
        assert getattr(lib, n).argtypes == _lib.SYMBOLS_PAGED8[n][1] and getattr(lib, n).restype == _lib.SYMBOLS_PAGED8[n][0]
    # the argument lists are the bf16 paged family's: only the pool's format differs
    for n8, n in zip(NAMES, _lib.SYMBOLS_PAGED):
        assert _lib.SYMBOLS_PAGED8[n8] == _lib.SYMBOLS_PAGED[n], (n8, n)
    assert lib.obte_abi_version() == 1
    sizes = (C.c_int64 * 8)()
    assert lib.obte_struct_sizes(sizes, 8) == 6
    header = open(__file__.rsplit("/tests/", 1)[0] + "/include/omnibiote_hip_paged8.h").read()
    for n in NAMES:
        assert n + "(" in header
    for n_pages, H, hs in ((16, 2, 128), (1, 1, 64), (40, 8, 64), ((1 << 24) - 1, 3, 128)):
        assert lib.obte_kv8_paged_bytes(n_pages, H, hs) == pool8_bytes(n_pages, H, hs) == 2 * n_pages * H * 64 * (hs + 4)
    assert lib.obte_kv8_paged_bytes(16, 2, 32) == 0 and lib.obte_kv8_paged_bytes(1 << 24, 2, 64) == 0 and lib.obte_kv8_paged_bytes(0, 2, 64) == 0
    assert pool8_bytes(16, 8, 128) / pool_bytes(16, 8, 128) == (128 + 4) / 256 and KV_PAGE == 64


# ------------------------------------------------------------------------------------------------------- rejection before launch
def _call_store(qkv=P, B=1, t=10, H=1, hs=128, pool=P, n_pages=4, table=P, ld=2):
    return _lib.lib().obte_kv8_paged_store(qkv, B, t, H, hs, pool, n_pages, table, ld, None)


def _call_rope(qkv=P, cos=P, sin=P, pos=P, max_pos=5, B=1, H=1, hs=128, pool=P, n_pages=4, table=P, ld=2):
    return _lib.lib().obte_kv8_paged_rope_store_rows(qkv, cos, sin, pos, max_pos, B, H, hs, pool, n_pages, table, ld, None)


def _call_decode(q=P, q_ld=128, pool=P, n_pages=4, table=P, ld=2, o=P, lse=None, B=1, n_keys=P, max_keys=10, H=1, hs=128, splits=1, ws=None, ws_bytes=0):
    return _lib.lib().obte_attn_decode_paged8(q, q_ld, pool, n_pages, table, ld, o, lse, B, n_keys, max_keys, H, hs, 1.0, splits, ws, ws_bytes, None)


def _desc(T=1, H=2):
    return _lib.BlockDesc(B=2, T=T, n_embd=256, n_head=H, ln1_w=P, attn_w=P, proj_w=P, ln2_w=P, fc_w=P, mlp_w=P, rope_cos=P, rope_sin=P)


def _call_block_decode(H=2, pool=P, n_pages=4, table=P, ld=2, pos=P, max_pos=5, short=0):
    lib = _lib.lib()
    d = _desc(1, H)
    return lib.obte_block_decode_paged8(C.byref(d), P, P, pool, n_pages, table, ld, pos, max_pos, P, lib.obte_block_decode_ws_bytes(2, 256, 2) - short, None)


def _call_block_prefill(H=2, T=100, pool=P, n_pages=4, table=P, ld=2, short=0):
    lib = _lib.lib()
    d = _desc(T, H)
    return lib.obte_block_fwd_prefill_paged8(C.byref(d), P, P, P, lib.obte_block_infer_ws_bytes(2, T, 256, 2) - short, pool, n_pages, table, ld, None)


STORE, ROPE, DECODE, BDEC, BPRE = ((_call_store, "obte_kv8_paged_store"), (_call_rope, "obte_kv8_paged_rope_store_rows"), (_call_decode, "obte_attn_decode_paged8"),
                                   (_call_block_decode, "obte_block_decode_paged8"), (_call_block_prefill, "obte_block_fwd_prefill_paged8"))


@pytest.mark.parametrize("entry,kw,word", [
    # a null pointer
    (STORE, dict(qkv=None), "null"), (STORE, dict(pool=None), "null"), (STORE, dict(table=None), "null"),
    (ROPE, dict(pos=None), "null"), (ROPE, dict(pool=None), "null"), (ROPE, dict(table=None), "null"),
    (DECODE, dict(q=None), "null"), (DECODE, dict(pool=None), "null"), (DECODE, dict(table=None), "null"), (DECODE, dict(n_keys=None), "null"),
    (BDEC, dict(pool=None), "null"), (BDEC, dict(table=None), "null"), (BDEC, dict(pos=None), "null"),
    (BPRE, dict(pool=None), "null"), (BPRE, dict(table=None), "null"),
    # a misaligned pool (the scales behind the codes are read as fp32, the codes 16 bytes at a time)
    (STORE, dict(pool=P + 8), "aligned"), (ROPE, dict(pool=P + 8), "aligned"), (DECODE, dict(pool=P + 8), "aligned"),
    (BDEC, dict(pool=P + 8), "aligned"), (BPRE, dict(pool=P + 8), "aligned"),
    (ROPE, dict(table=P + 2), "aligned"), (BDEC, dict(table=P + 2), "aligned"),
    # the table's row length bounds every position and count
    (STORE, dict(t=129), "do not fit"), (STORE, dict(t=0), "do not fit"), (BPRE, dict(T=130), "130 positions do not fit the table's 128"),
    (DECODE, dict(max_keys=129), "max_keys"), (DECODE, dict(max_keys=0), "max_keys"),
    (ROPE, dict(max_pos=128), "max_pos"), (ROPE, dict(max_pos=-1), "max_pos"), (BDEC, dict(max_pos=128), "max_pos = 128"),
    # a bad head size, a bad pool
    (STORE, dict(hs=32), "head_dim"), (ROPE, dict(hs=32), "head_dim"), (DECODE, dict(hs=32), "head_dim"), (BDEC, dict(H=8), "head"), (BPRE, dict(H=8), "head"),
    (STORE, dict(n_pages=0), "shape"), (ROPE, dict(ld=0), "shape"), (DECODE, dict(n_pages=1 << 24), "shape"), (BDEC, dict(n_pages=0), "n_pages"),
    (BPRE, dict(n_pages=1 << 24), "n_pages"),
    # the attention's own, and the workspaces
    (DECODE, dict(splits=-1), "splits"), (DECODE, dict(splits=2, ws=P, ws_bytes=64), "workspace"), (DECODE, dict(q_ld=64), "q_ld"),
    (BDEC, dict(short=1), "workspace"), (BPRE, dict(short=1), "workspace"),
])
def test_paged8_entry_points_reject_before_any_launch(entry, kw, word):
    (call, name) = entry
    assert call(**kw) == EINVAL
    assert _err().startswith(name + ":") and word in _err(), _err()


# ------------------------------------------------------------------------------------------------------- the format in plain torch
def test_paged8_gather_and_scatter_reference_are_inverse():
    g = torch.Generator().manual_seed(5)
    B, H, hs, n_pages = 3, 2, 8, 16
    codes = torch.randint(0, 256, (2, B, H, 256, hs), dtype=torch.uint8, generator=g)
    scales = torch.exp2(torch.randint(-20, 20, (2, B, H, 256), generator=g).float())
    table = torch.randperm(n_pages, generator=g)[:12].view(B, 4).to(torch.int32)
    pool = paged8_scatter_reference(codes, scales, table, n_pages)
    assert pool.dtype == torch.uint8 and pool.numel() == pool8_bytes(n_pages, H, hs)
    # the layout, stated independently: K codes, V codes, K scales, V scales
    n = n_pages * H * 64
    kc, vc = pool[:n * hs].view(n_pages, H, 64, hs), pool[n * hs:2 * n * hs].view(n_pages, H, 64, hs)
    ks, vs = pool[2 * n * hs:2 * n * hs + 4 * n].view(torch.float32).view(n_pages, H, 64), pool[2 * n * hs + 4 * n:].view(torch.float32).view(n_pages, H, 64)
    used = torch.zeros(n_pages, dtype=torch.bool)
    used[table.flatten().long()] = True
    assert (kc[~used] == 0x7F).all() and (vc[~used] == 0x7F).all() and torch.isnan(ks[~used]).all() and torch.isnan(vs[~used]).all()
    assert not torch.isnan(ks[used]).any() and not torch.isnan(vs[used]).any()
    page = table[1, 2].item()                                               # page table[b][j], head h: positions [64 j, 64 j + 64)
    assert torch.equal(kc[page, 1], codes[0, 1, 1, 128:192]) and torch.equal(vc[page, 0], codes[1, 1, 0, 128:192])
    assert torch.equal(ks[page, 1], scales[0, 1, 1, 128:192]) and torch.equal(vs[page, 0], scales[1, 1, 0, 128:192])
    gc, gs = paged8_gather_reference(pool, table, n_pages, H, hs)
    assert torch.equal(gc, codes) and torch.equal(gs, scales)
    table[0, 1], table[2, 3] = -1, n_pages                                  # no page: the fill
    gc, gs = paged8_gather_reference(pool, table, n_pages, H, hs, T=200, fill_code=9, fill_scale=7.0)
    assert gc.shape == (2, B, H, 200, hs) and gs.shape == (2, B, H, 200)
    assert (gc[:, 0, :, 64:128] == 9).all() and (gs[:, 0, :, 64:128] == 7).all() and (gc[:, 2, :, 192:] == 9).all() and (gs[:, 2, :, 192:] == 7).all()
    assert torch.equal(gc[:, 1], codes[:, 1, :, :200]) and torch.equal(gs[:, 0, :, :64], scales[:, 0, :, :64])
    with pytest.raises(ValueError, match="uint8"):
        paged8_gather_reference(pool[:-1], table, n_pages, H, hs)
    with pytest.raises(ValueError, match="multiple of 64"):
        paged8_scatter_reference(codes[:, :, :, :100], scales[:, :, :, :100], table, n_pages)


# ------------------------------------------------------------------------------------------------------- the keywords and the refusals
def test_dtype_keywords_are_checked_before_anything_else():
    from omnibiote_amd.model import PagedKVCache
    m = _cpu_model()
    with pytest.raises(ValueError, match="PagedKVCache: dtype must be 'bf16' or 'fp8', got 'int8'"):
        PagedKVCache(m, 2, 4, dtype="int8")
    p = [torch.zeros(5, dtype=torch.int64), torch.zeros(19, dtype=torch.int64)]
    with pytest.raises(ValueError, match="generate_many: kv_dtype must be 'bf16' or 'fp8', got 'int8'"):
        m.generate_many(p, 5, batch=2, kv_dtype="int8")
    for kv_dtype in ("bf16", "fp8"):                                        # the checks behind it are the same for either
        with pytest.raises(ValueError, match="n_pages = 1"):
            m.generate_many([p[0], torch.zeros(100, dtype=torch.int64)], 5, batch=2, n_pages=1, kv_dtype=kv_dtype)
        assert m.generate_many([], 5, batch=2, kv_dtype=kv_dtype) == []
    with pytest.raises(RuntimeError):                                       # a valid dtype gets as far as the device check: there is no CPU pool
        PagedKVCache(m, 2, 4, dtype="fp8")


def test_paged_fp8_state_keeps_every_refusal():
    from omnibiote_amd.model import CachePositions, DecodeLoop, QuantizedWeights
    m = _cpu_model()
    c = _fake()
    assert c.dtype == "bf16"
    c.dtype = "fp8"                                                         # what PagedKVCache(dtype="fp8") tags its position state with
    c.start_rows([0, 1, 2], [5, 6, 7])
    state = lambda: (c.positions.tolist(), c.table.tolist(), c.pages_in_use, c.pos, c.dtype)   # noqa: E731
    before = state()
    tok = torch.zeros(3, 4, dtype=torch.int64)
    w = QuantizedWeights.__new__(QuantizedWeights)
    draft = _fake()
    draft.dtype = "fp8"
    plain = CachePositions(3, 32)
    plain.reset(8)
    plain.layers, plain.decode_ws, plain.extend_ws = [None], None, None
    for call in (lambda: m.extend(tok, c), lambda: m.prefill(tok, c, chunk=2), lambda: m.draft_and_verify(m, tok[:, 0], c, _fake(), 2),
                 lambda: m.draft_and_verify(m, tok[:, 0], plain, draft, 2), lambda: m.prefill(tok, c, weights=w), lambda: m.decode_step(tok[:, 0], c, weights=w),
                 lambda: DecodeLoop(m, c, max_steps=4)):
        with pytest.raises(NotImplementedError):
            call()
    with pytest.raises(NotImplementedError, match=r"prefill\(chunk=\): the cache is a paged cache"):
        m.prefill(tok, c, chunk=2)
    with pytest.raises(NotImplementedError, match=r"DecodeLoop: the cache is a paged cache"):
        DecodeLoop(m, c, max_steps=4)
    assert state() == before
