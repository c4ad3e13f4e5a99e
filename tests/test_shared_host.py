"""Host-side tests (no GPU) of the shared-prefix key/value cache (include/omnibiote_hip_shared.h): the symbol table against the header,
the pins of the ABI, the default prefix split rule and the workspace sizes, every argument check that returns before a launch, and the
validation of SharedPrefixCache / generate(num_samples=) on a CPU model with the cache's position state alone."""
import ctypes as C
import os
import re

import pytest
import torch

from omnibiote_amd import _lib

EINVAL, EUNSUPPORTED = -1, -3
MAX = _lib.ATTN_SHARED_MAX_SPLITS
P = 4096   # a non-null, 16-byte aligned "pointer" for calls that must return before they touch it
NAMES = ("obte_attn_shared_prefix_splits", "obte_attn_decode_shared_ws_bytes", "obte_attn_decode_shared", "obte_block_decode_shared_ws_bytes",
         "obte_block_decode_shared")


def _err():
    return _lib.lib().obte_last_error().decode()


def test_symbols_are_what_the_header_declares():
    assert tuple(_lib.SYMBOLS_SHARED) == NAMES
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "omnibiote_hip_shared.h")).read()
    body = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    assert tuple(re.findall(r"\b(obte_\w+)\s*\(", body)) == NAMES                  # the declarations, in order
    assert '#include "omnibiote_hip.h"' in header and "struct" not in body
    assert re.search(r"#define\s+OBTE_ATTN_SHARED_MAX_SPLITS\s+%d\b" % MAX, header)
    lib = _lib.lib()
    for name in NAMES:
        for table in (_lib.SYMBOLS, _lib.SYMBOLS_ROWS, _lib.SYMBOLS_SMALL_M, _lib.SYMBOLS_SAMPLE, _lib.SYMBOLS_EXTEND, _lib.SYMBOLS_SPEC, _lib.SYMBOLS_KV8):
            assert name not in table
        res, args = _lib.SYMBOLS_SHARED[name]
        fn = getattr(lib, name)                                                     # the library exports it
        assert fn.restype is res and list(fn.argtypes) == args                      # bound by lib(), in the same loop
    assert len(_lib.SYMBOLS) == 70 and len(_lib.SYMBOLS_ROWS) == 3 and len(_lib.SYMBOLS_SMALL_M) == 3 and len(_lib.SYMBOLS_SAMPLE) == 1
    assert len(_lib.SYMBOLS_EXTEND) == 6 and len(_lib.SYMBOLS_SPEC) == 2 and len(_lib.SYMBOLS_KV8) == 6
    assert lib.obte_abi_version() == 1
    sizes = (C.c_int64 * 16)()
    assert lib.obte_struct_sizes(sizes, 16) == 6


def test_default_prefix_split_rule():
    f = _lib.lib().obte_attn_shared_prefix_splits
    keys = [1, 31, 33, 130, 255, 256, 511, 512, 700, 2048, 4096, 65536]
    for hs in (64, 128):
        for G in (1, 3, 32, 33, 64, 256):
            table = {}
            for Pn, H in [(1, 1), (1, 8), (3, 2), (8, 8), (64, 8)]:
                row = [f(Pn, G, H, hs, k) for k in keys]
                assert all(1 <= v <= MAX for v in row), row
                assert row == [f(Pn, G, H, hs, k) for k in keys]                    # a pure function
                assert all(a <= b for a, b in zip(row, row[1:])), row               # never fewer splits for more keys
                assert _lib.lib().obte_attn_decode_shared_ws_bytes(Pn, G, H, hs, 0, 1) >= _lib.lib().obte_attn_decode_shared_ws_bytes(Pn, G, H, hs, max(row), 1)
                table[Pn * H] = row
            order = sorted(table)
            for lo, hi in zip(order, order[1:]):                                    # never more splits for more (p, h)
                assert all(a >= b for a, b in zip(table[lo], table[hi])), (lo, hi)
    assert f(1, 8, 8, 128, 255) == 1 and f(1, 8, 8, 128, 2048) > 1                  # nothing to split below the rule's minimum; and it does split
    assert f(1, 64, 8, 128, 2048) <= f(1, 8, 8, 128, 2048)                          # a second query tile doubles the workgroups
    for bad in [(0, 8, 8, 128, 2048), (1, 0, 8, 128, 2048), (1, 8, 0, 128, 2048), (1, 8, 8, 32, 2048), (1, 8, 8, 256, 2048), (1, 8, 8, 128, 0),
                (70000, 1, 1, 128, 2048), (1, 70000, 1, 128, 2048), (1, 1 << 20, 1, 64, 2048)]:
        assert f(*bad) == 1, bad


def test_workspace_sizes():
    lib = _lib.lib()
    ws = lib.obte_attn_decode_shared_ws_bytes
    for Pn, G, H, hs in [(1, 1, 1, 64), (3, 33, 2, 64), (2, 40, 2, 128), (1, 64, 8, 128)]:
        B, tiles = Pn * G, (G + 31) // 32
        pre, suf = Pn * H * tiles * (hs // 2 + 2) * 64 * 4, B * H * (hs + 4) * 4    # one partial per (p, h, tile) and per (b, h)
        assert ws(Pn, G, H, hs, 1, 1) == pre + suf
        assert ws(Pn, G, H, hs, 5, 3) == 5 * pre + 3 * suf
        assert ws(Pn, G, H, hs, 5, 3) == ws(Pn, G, H, hs, 5, 3) and ws(Pn, G, H, hs, 1, 1) % 16 == 0
        top = lib.obte_attn_decode_splits(B, H, hs, 1 << 23)
        assert ws(Pn, G, H, hs, 0, 0) >= ws(Pn, G, H, hs, lib.obte_attn_shared_prefix_splits(Pn, G, H, hs, 1 << 23), top)
        total = lib.obte_block_decode_shared_ws_bytes(Pn, G, H * hs, H)
        assert total >= lib.obte_block_infer_ws_bytes(B, 1, H * hs, H) + ws(Pn, G, H, hs, 0, 0) > 0
        assert total == lib.obte_block_decode_shared_ws_bytes(Pn, G, H * hs, H) and total % 256 == 0
    for bad in [(0, 4, 2, 64, 1, 1), (2, 0, 2, 64, 1, 1), (2, 4, 0, 64, 1, 1), (2, 4, 2, 32, 1, 1), (2, 4, 2, 256, 1, 1), (2, 4, 2, 64, -1, 1),
                (2, 4, 2, 64, MAX + 1, 1), (2, 4, 2, 64, 1, -1), (2, 4, 2, 64, 1, _lib.ATTN_DECODE_MAX_SPLITS + 1), (9000, 1, 8, 64, 1, 1),
                (1, 9000, 8, 64, 1, 1)]:
        assert ws(*bad) == 0, bad
    assert lib.obte_block_decode_shared_ws_bytes(2, 4, 128, 4) == 0                 # head size 32
    assert lib.obte_block_decode_shared_ws_bytes(0, 4, 256, 2) == 0 and lib.obte_block_decode_shared_ws_bytes(2, 0, 256, 2) == 0
    assert lib.obte_block_decode_shared_ws_bytes(2, 4, 200, 2) == 0 and lib.obte_block_decode_shared_ws_bytes(9000, 4, 256, 2) == 0


BIG = 1 << 30


def _attn(q=P, q_ld=256, pre=P, Pn=2, T_pre=100, n_prefix=40, suf=P, G=3, T_suf=50, n_suffix=7, o=P, lse=None, H=2, hs=128, ps=1, ss=1, ws=P, ws_bytes=BIG):
    return _lib.lib().obte_attn_decode_shared(q, q_ld, pre, Pn, T_pre, n_prefix, suf, G, T_suf, n_suffix, o, lse, H, hs, 1.0, ps, ss, ws, ws_bytes, None)


@pytest.mark.parametrize("kw,word", [
    (dict(q=None), "null"), (dict(pre=None), "null"), (dict(o=None), "null"), (dict(suf=None), "null"),
    (dict(n_prefix=0), "n_prefix"), (dict(n_prefix=101), "n_prefix"), (dict(n_prefix=-2), "n_prefix"),
    (dict(n_suffix=51), "n_suffix"), (dict(n_suffix=-1), "n_suffix"),
    (dict(hs=32, q_ld=64), "head_dim"), (dict(hs=256, q_ld=512), "head_dim"), (dict(Pn=0), "shape"), (dict(G=0), "shape"), (dict(H=0), "shape"),
    (dict(Pn=40000), "65535"), (dict(G=20000), "65535"), (dict(T_pre=0), "shape"), (dict(T_suf=-1), "shape"),
    (dict(q_ld=260), "q_ld"), (dict(q_ld=128), "q_ld"),
    (dict(q=P + 8), "aligned"), (dict(pre=P + 8), "aligned"), (dict(suf=P + 8), "aligned"), (dict(o=P + 8), "aligned"), (dict(lse=P + 2), "aligned"),
    (dict(ps=-1), "prefix_splits"), (dict(ps=MAX + 1), "prefix_splits"), (dict(ss=-1), "suffix_splits"),
    (dict(ss=_lib.ATTN_DECODE_MAX_SPLITS + 1), "suffix_splits"),
    (dict(ws=None), "workspace"), (dict(ws=P + 4), "workspace"), (dict(ws_bytes=64), "workspace"),
    (dict(ps=3, ss=2, ws_bytes=None), "workspace"),                                     # one byte short of what these counts need
    (dict(ps=0, ss=0, T_pre=4096, n_prefix=4096, T_suf=4096, n_suffix=4096, ws_bytes=None), "workspace"),   # and of what the default counts need
])
def test_attn_decode_shared_rejects_before_any_launch(kw, word):
    if "ws_bytes" in kw and kw["ws_bytes"] is None:
        lib = _lib.lib()
        ps = kw["ps"] or lib.obte_attn_shared_prefix_splits(2, 3, 2, 128, kw["n_prefix"])
        ss = kw["ss"] or lib.obte_attn_decode_splits(6, 2, 128, kw["n_suffix"])
        assert ps > 1 and ss > 1
        kw = dict(kw, ws_bytes=lib.obte_attn_decode_shared_ws_bytes(2, 3, 2, 128, ps, ss) - 1)
    assert _attn(**kw) == EINVAL
    assert _err().startswith("obte_attn_decode_shared:") and word in _err(), _err()


def test_attn_decode_shared_without_a_suffix_takes_a_null_suffix_cache():
    # n_suffix = 0 with suffix_cache NULL passes the pointer check: the next refusal is the workspace's, sized for the prefix alone
    lib = _lib.lib()
    need = lib.obte_attn_decode_shared_ws_bytes(2, 3, 2, 128, 1, 1) - 6 * 2 * 132 * 4
    assert _attn(suf=None, T_suf=0, n_suffix=0, ws_bytes=need - 1) == EINVAL and "workspace" in _err() and str(need) in _err(), _err()


def _desc(B=6, T=1, C_=256, H=2, **over):
    f = dict(B=B, T=T, n_embd=C_, n_head=H, ln1_w=P, attn_w=P, proj_w=P, ln2_w=P, fc_w=P, mlp_w=P, rope_cos=P, rope_sin=P)
    f.update(over)
    return _lib.BlockDesc(**f)


def test_block_decode_shared_rejects_before_any_launch():
    lib = _lib.lib()

    def step(d, x=P, y=P, pre=P, Pn=2, T_pre=100, n_prefix=40, suf=P, T_suf=50, suf_pos=5, ws=P, ws_bytes=BIG):
        return lib.obte_block_decode_shared(C.byref(d) if d is not None else None, x, y, pre, Pn, T_pre, n_prefix, suf, T_suf, suf_pos, ws, ws_bytes, None)
    assert step(None) == EINVAL and "obte_block_decode_shared" in _err() and "null" in _err()
    for over in (dict(key_ranges=P), dict(out_rows=P, n_out_rows=1), dict(dropout_p=0.1), dict(mask=P), dict(query_bounds=P)):
        assert step(_desc(**over)) == EUNSUPPORTED, over
        assert _err().startswith("obte_block_decode_shared:"), _err()
    for kw in (dict(x=None), dict(y=None), dict(pre=None), dict(suf=None), dict(ws=None)):
        assert step(_desc(), **kw) == EINVAL and _err().startswith("obte_block_decode_shared:") and "null" in _err(), (kw, _err())
    assert step(_desc(T=2)) == EINVAL and "T = 1" in _err()
    assert step(_desc(), Pn=4) == EINVAL and "groups" in _err()                      # 6 rows are not 4 groups
    assert step(_desc(), Pn=0) == EINVAL and "groups" in _err()
    for kw in (dict(n_prefix=0), dict(n_prefix=101), dict(T_pre=0)):
        assert step(_desc(), **kw) == EINVAL and "n_prefix" in _err(), (kw, _err())
    for kw in (dict(suf_pos=50), dict(suf_pos=-1), dict(T_suf=0, suf_pos=0)):
        assert step(_desc(), **kw) == EINVAL and "suffix slot" in _err(), (kw, _err())
    assert step(_desc(), pre=P + 8) == EINVAL and "aligned" in _err()
    assert step(_desc(), suf=P + 8) == EINVAL and "aligned" in _err()
    assert step(_desc(B=40000), Pn=1) == EINVAL and "65535" in _err()
    assert step(_desc(), ws_bytes=lib.obte_block_decode_shared_ws_bytes(2, 3, 256, 2) - 1) == EINVAL
    assert _err().startswith("obte_block_decode_shared:") and "workspace" in _err(), _err()
    assert step(_desc(C_=128, H=4)) == EINVAL                                        # head size 32
    assert _err().startswith("obte_block_decode_shared:") and "head" in _err(), _err()


# ------------------------------------------------------------------------------------------------------- the model surface
def _cpu_model(block_size=32, autoregressive=True):
    from omnibiote_amd.model import OmniBioTA, OmniBioTAConfig
    c = OmniBioTAConfig()
    c.block_size, c.vocab_size, c.n_layer, c.n_head, c.n_embd, c.dropout, c.flash = block_size, 64, 1, 2, 128, 0.0, True
    c.autoregressive = autoregressive
    return OmniBioTA(c)


def _fake(prompts=2, samples=3, prefix_len=8, max_new=5, n_prefix=8):
    """a shared-prefix cache's position state with no buffer behind it"""
    from omnibiote_amd.model import CachePositions, SharedPrefixCache
    c = SharedPrefixCache.__new__(SharedPrefixCache)
    CachePositions.__init__(c, prompts * samples, prefix_len + max_new)
    c._shape(prompts, samples, prefix_len, max_new)
    c.layers, c.decode_ws, c.extend_ws = [None], None, None
    c.reset(n_prefix)
    c.n_prefix = n_prefix
    return c


def test_shared_cache_positions():
    from omnibiote_amd.model import CachePositions, SharedPrefixCache
    assert issubclass(SharedPrefixCache, CachePositions)
    c = _fake()
    assert (c.batch, c.max_len, c.group, c.prompts, c.n_prefix, c.pos, c.positions, c.dtype) == (6, 13, 3, 2, 8, 8, None, "bf16")
    with pytest.raises(ValueError, match="prefix"):
        c.rewind(0)                                                                # pos - n < n_prefix + 1: no own token would stay
    c.advance(1)
    assert c.pos == 9 and c.positions is None
    with pytest.raises(ValueError, match="prefix"):
        c.rewind(1)
    c.advance(3)
    c.rewind(2)
    assert c.pos == 10
    with pytest.raises(ValueError, match="prefix"):
        c.rewind(2)
    with pytest.raises(ValueError, match="negative"):
        c.rewind(-1)
    assert c.pos == 10
    c.rewind(1)
    assert c.pos == 9
    with pytest.raises(ValueError, match="uniform"):
        c.park(torch.zeros(6, dtype=torch.bool))
    with pytest.raises(ValueError, match="uniform"):
        c.rewind_rows([0] * 6)
    c.advance(4)                                                                    # slots 0 .. 4 are taken
    c.require_room("decode_step", 0)
    with pytest.raises(ValueError, match="full"):
        c.require_room("decode_step", 1)
    short = _fake(n_prefix=5)                                                       # a prompt shorter than the prefix buffer: the slots still bound it
    short.advance(5)
    with pytest.raises(ValueError, match="full"):
        short.require_room("decode_step", 1)


def test_shared_cache_constructor_checks_its_arguments_first():
    from omnibiote_amd.model import SharedPrefixCache
    m = _cpu_model()
    for args in [(0, 3, 8, 5), (2, 0, 8, 5), (2, 3, 0, 5), (2, 3, 8, 0), (2, 3, 30, 3)]:
        with pytest.raises(ValueError, match="SharedPrefixCache"):
            SharedPrefixCache(m, *args)
    with pytest.raises(ValueError, match="autoregressive"):
        SharedPrefixCache(_cpu_model(autoregressive=False), 2, 3, 8, 5)
    with pytest.raises(RuntimeError, match="GPU"):                                  # valid arguments go on to the first device-side requirement
        SharedPrefixCache(m, 2, 3, 8, 5)


def test_operations_a_shared_cache_refuses():
    m = _cpu_model()
    c = _fake()
    with pytest.raises(NotImplementedError, match="SharedPrefixCache"):
        m.extend(torch.zeros(6, 4, dtype=torch.int64), c)
    with pytest.raises(NotImplementedError, match="SharedPrefixCache"):
        m.extend(torch.zeros(6, 1, dtype=torch.int64), c)
    with pytest.raises(NotImplementedError, match="SharedPrefixCache"):
        m.draft_and_verify(m, torch.zeros(6, dtype=torch.int64), c, _fake(), 2)
    with pytest.raises(NotImplementedError, match="SharedPrefixCache"):
        m.generate_speculative(torch.zeros(2, 4, dtype=torch.int64), 4, m, num_samples=3)
    idx = torch.zeros(2, 8, dtype=torch.int64)
    with pytest.raises(ValueError, match="lengths"):
        m.prefill(idx, c, lengths=[8, 8])
    with pytest.raises(ValueError, match="chunk"):
        m.prefill(idx, c, chunk=4)
    with pytest.raises(ValueError, match="2 prompts"):
        m.prefill(torch.zeros(6, 8, dtype=torch.int64), c)                          # one row per prompt, not per sample
    with pytest.raises(ValueError, match="prefix of 8"):
        m.prefill(torch.zeros(2, 9, dtype=torch.int64), c)
    assert c.pos == 8 and c.n_prefix == 8
    with pytest.raises(RuntimeError, match="GPU"):
        m.prefill(idx, c)
    with pytest.raises(ValueError, match="batch size 6"):
        m.decode_step(torch.zeros(2, dtype=torch.int64), c)                         # one token per sample


def test_generate_num_samples_argument_errors():
    m = _cpu_model()
    idx = torch.zeros(2, 4, dtype=torch.int64)
    for bad in (0, -1, 2.0, True):
        with pytest.raises(ValueError, match="num_samples"):
            m.generate(idx, 4, num_samples=bad)
    with pytest.raises(ValueError, match="num_samples"):
        m.generate(idx, 4, num_samples=3, lengths=[4, 4])
    with pytest.raises(ValueError, match="num_samples"):
        m.generate(idx, 4, num_samples=3, kv_dtype="fp8")
    with pytest.raises(ValueError, match="block_size"):
        m.generate(idx, 40, num_samples=3)
    out = m.generate(idx + torch.arange(2).view(2, 1), 0, num_samples=3)            # nothing to draw: the prompts, once per sample
    assert out.shape == (6, 4) and out[:, 0].tolist() == [0, 0, 0, 1, 1, 1]
    with pytest.raises(RuntimeError, match="GPU"):
        m.generate(idx, 4, num_samples=3)
