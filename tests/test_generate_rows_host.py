"""Host-side tests (no GPU) of generation with one cache position per row: every argument check of the three rows entry points that
returns before a launch, the second symbol table, the validation of ``lengths`` in OmniBioTA.prefill / decode_step / generate, and
the assembly of a ragged generate()'s result as a pure function on CPU tensors."""
import ctypes as C
import os
import re

import pytest
import torch

from omnibiote_amd import _lib

EINVAL, EUNSUPPORTED = -1, -3
MAX = _lib.ATTN_DECODE_MAX_SPLITS
P = 4096   # a non-null, 16-byte aligned "pointer" for calls that must return before they touch it


def _err():
    return _lib.lib().obte_last_error().decode()


# ------------------------------------------------------------------------------------------------------- entry points
def _call_store(qkv=P, cos=P, sin=P, pos=P, max_pos=5, B=1, H=1, hs=128, cache=P, T_max=100):
    return _lib.lib().obte_kv_cache_rope_store_rows(qkv, cos, sin, pos, max_pos, B, H, hs, cache, T_max, None)


@pytest.mark.parametrize("kw,word", [
    (dict(qkv=None), "null"), (dict(cos=None), "null"), (dict(sin=None), "null"), (dict(pos=None), "null"), (dict(cache=None), "null"),
    (dict(max_pos=-1), "max_pos"), (dict(max_pos=100), "max_pos"),
    (dict(hs=32), "head_dim"), (dict(B=0), "shape"),
])
def test_rope_store_rows_rejects_before_any_launch(kw, word):
    assert _call_store(**kw) == EINVAL
    assert _err().startswith("obte_kv_cache_rope_store_rows:") and word in _err(), _err()


def _call_decode(q=P, q_ld=128, cache=P, o=P, lse=None, B=1, T_max=100, n_keys=P, max_keys=10, H=1, hs=128, splits=1, ws=None, ws_bytes=0):
    return _lib.lib().obte_attn_decode_rows(q, q_ld, cache, o, lse, B, T_max, n_keys, max_keys, H, hs, 1.0, splits, ws, ws_bytes, None)


@pytest.mark.parametrize("kw,word", [
    (dict(q=None), "null"), (dict(cache=None), "null"), (dict(o=None), "null"), (dict(n_keys=None), "null"),
    (dict(max_keys=0), "max_keys"), (dict(max_keys=101), "max_keys"),
    (dict(splits=MAX + 1), "splits"), (dict(splits=-1), "splits"),
    (dict(splits=2, ws=P, ws_bytes=64), "workspace"), (dict(splits=2, ws=None, ws_bytes=1 << 20), "workspace"),
    (dict(hs=32), "head_dim"), (dict(q_ld=64), "q_ld"),
])
def test_attn_decode_rows_rejects_before_any_launch(kw, word):
    assert _call_decode(**kw) == EINVAL
    assert _err().startswith("obte_attn_decode_rows:") and word in _err(), _err()


def _desc(B=2, T=1, C_=256, H=2, **over):
    f = dict(B=B, T=T, n_embd=C_, n_head=H, ln1_w=P, attn_w=P, proj_w=P, ln2_w=P, fc_w=P, mlp_w=P, rope_cos=P, rope_sin=P)
    f.update(over)
    return _lib.BlockDesc(**f)


def test_block_decode_rows_rejects_before_any_launch():
    lib = _lib.lib()
    big = 1 << 30

    def decode(d, x=P, y=P, kv=P, T_max=100, pos=P, max_pos=5, ws=P, ws_bytes=big):
        return lib.obte_block_decode_rows(C.byref(d) if d is not None else None, x, y, kv, T_max, pos, max_pos, ws, ws_bytes, None)
    assert decode(None) == EINVAL and "obte_block_decode_rows" in _err() and "null" in _err()
    assert decode(_desc(T=2)) == EINVAL
    assert _err().startswith("obte_block_decode_rows:") and "T = 1" in _err(), _err()
    for over in (dict(key_ranges=P), dict(out_rows=P, n_out_rows=1), dict(dropout_p=0.1), dict(mask=P), dict(query_bounds=P)):
        assert decode(_desc(**over)) == EUNSUPPORTED, over
        assert _err().startswith("obte_block_decode_rows:"), _err()
    for null in ("x", "y", "kv", "pos", "ws"):
        assert decode(_desc(), **{null: None}) == EINVAL
        assert _err().startswith("obte_block_decode_rows:") and "null" in _err(), (null, _err())
    for bad in (-1, 100):
        assert decode(_desc(), max_pos=bad) == EINVAL
        assert _err().startswith("obte_block_decode_rows:") and "max_pos" in _err(), _err()
    assert decode(_desc(), ws_bytes=lib.obte_block_decode_ws_bytes(2, 256, 2) - 1) == EINVAL
    assert _err().startswith("obte_block_decode_rows:") and "workspace" in _err(), _err()
    assert decode(_desc(C_=128, H=4)) == EINVAL                       # head size 32
    assert "obte_block_decode_rows" in _err(), _err()


def test_rows_symbols_have_their_own_table():
    lib = _lib.lib()
    rows = ("obte_kv_cache_rope_store_rows", "obte_attn_decode_rows", "obte_block_decode_rows")
    assert tuple(_lib.SYMBOLS_ROWS) == rows
    for name in rows:
        assert name not in _lib.SYMBOLS
        fn = getattr(lib, name)
        assert fn.restype is C.c_int and list(fn.argtypes) == _lib.SYMBOLS_ROWS[name][1]     # bound by lib(), in the same loop
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "omnibiote_hip_rows.h")).read()
    assert set(re.findall(r"^int (obte_[a-z0-9_]+)\(", header, flags=re.M)) == set(rows)      # what the companion header declares
    assert len(_lib.SYMBOLS) == 70 and list(_lib.SYMBOLS)[-1] == "obte_block_decode" and list(_lib.SYMBOLS)[-8] == "obte_kv_cache_bytes"
    assert lib.obte_abi_version() == 1
    sizes = (C.c_int64 * 16)()
    assert lib.obte_struct_sizes(sizes, 16) == 6


# ------------------------------------------------------------------------------------------------------- lengths
def _cpu_model(block_size=32):
    from omnibiote_amd.model import OmniBioTA, OmniBioTAConfig
    c = OmniBioTAConfig()
    c.block_size, c.vocab_size, c.n_layer, c.n_head, c.n_embd, c.dropout, c.flash = block_size, 64, 1, 2, 128, 0.0, True
    c.autoregressive = True
    return OmniBioTA(c)


def _fake_cache(batch=2, max_len=32, pos=0, positions=None):
    """what prefill / decode_step look at before any device work (a KVCache itself allocates on the GPU)"""
    from omnibiote_amd.model import CachePositions
    c = CachePositions(batch, max_len)
    c.reset(pos, positions)
    c.layers, c.decode_ws, c.extend_ws = [], None, None
    return c


def test_lengths_are_validated_before_any_device_work():
    m = _cpu_model()
    idx = torch.zeros(2, 8, dtype=torch.int64)
    for what in (lambda lengths: m.generate(idx, 4, lengths=lengths), lambda lengths: m.prefill(idx, _fake_cache(), lengths=lengths)):
        with pytest.raises(ValueError, match="3 lengths for a batch of 2"):
            what([3, 4, 5])
        with pytest.raises(ValueError, match=r"\[1, T0 = 8\]"):
            what([0, 8])
        with pytest.raises(ValueError, match=r"\[1, T0 = 8\]"):
            what([9, 8])
        with pytest.raises(ValueError, match=r"\[1, T0 = 8\]"):
            what(torch.tensor([8, -1]))
    with pytest.raises(ValueError, match="block_size"):
        m.generate(idx, 25, lengths=[3, 8])                        # 8 + 25 > 32: the longest row decides
    with pytest.raises(ValueError, match="block_size"):
        m.generate(idx, -1, lengths=[3, 8])
    with pytest.raises(ValueError, match="batch"):
        m.prefill(idx, _fake_cache(batch=3), lengths=[3, 8])
    with pytest.raises(ValueError, match="does not fit"):
        m.prefill(idx, _fake_cache(max_len=7), lengths=[3, 7])


def test_decode_step_refuses_a_full_ragged_cache():
    m = _cpu_model()
    tok = torch.zeros(2, dtype=torch.int64)
    full = _fake_cache(pos=32, positions=torch.tensor([20, 32], dtype=torch.int32))
    with pytest.raises(ValueError, match="full"):
        m.decode_step(tok, full)
    # the uniform rule is untouched: `pos`, not `max_pos`, decides there
    with pytest.raises(ValueError, match="full"):
        m.decode_step(tok, _fake_cache(pos=32))
    with pytest.raises(RuntimeError, match="GPU"):                 # room left: the next thing it notices is the CPU tensor
        m.decode_step(tok, _fake_cache(pos=31, positions=torch.tensor([20, 31], dtype=torch.int32)))


def test_generate_without_new_tokens_returns_the_padded_prompts():
    m = _cpu_model()
    idx = torch.arange(1, 17).view(2, 8)
    out, n = m.generate(idx, 0, lengths=[3, 6], pad_token=63)
    assert out.tolist() == [[1, 2, 3, 63, 63, 63], [9, 10, 11, 12, 13, 14]] and n.tolist() == [3, 6]
    assert out.dtype == torch.int64 and n.dtype == torch.int64


# ------------------------------------------------------------------------------------------------------- layout
def test_ragged_output_layout():
    from omnibiote_amd.model import ragged_output
    idx = torch.tensor([[11, 12, 13, 99, 99], [21, 22, 23, 24, 25], [31, 99, 99, 99, 99]])
    tokens = torch.tensor([[1, 2, 3, 4], [5, 6, 7, 8], [9, 10, 11, 12]])
    # row 0 ran every step; row 1 stopped with its second token (its EOS counts); row 2 stopped with its first
    valid = torch.tensor([[True, True, True, True], [True, True, False, False], [True, False, False, False]])
    out, n = ragged_output(idx, [3, 5, 1], tokens, valid, pad_token=0)
    assert out.shape == (3, 5 + 4) and out.dtype == torch.int64
    assert out.tolist() == [[11, 12, 13, 1, 2, 3, 4, 0, 0],
                            [21, 22, 23, 24, 25, 5, 6, 0, 0],
                            [31, 9, 0, 0, 0, 0, 0, 0, 0]]
    assert n.tolist() == [7, 7, 2] and n.dtype == torch.int64
    # lengths as a tensor, another pad token, a prompt buffer wider than the longest row
    wide = torch.cat([idx, torch.full((3, 2), 77)], dim=1)
    out2, n2 = ragged_output(wide, torch.tensor([3, 5, 1]), tokens, valid, pad_token=7)
    assert torch.equal(n2, n) and torch.equal(out2 == 7, out == 0) and torch.equal(out2[out2 != 7], out[out != 0])
    # no step taken
    out3, n3 = ragged_output(idx, [3, 5, 1], tokens[:, :0], valid[:, :0], pad_token=0)
    assert out3.tolist() == [[11, 12, 13, 0, 0], [21, 22, 23, 24, 25], [31, 0, 0, 0, 0]] and n3.tolist() == [3, 5, 1]
