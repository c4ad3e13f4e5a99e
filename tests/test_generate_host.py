"""Host-side tests (no GPU) of autoregressive generation: the sizes of the key/value cache and of the workspaces, the default split
rule of obte_attn_decode, every argument check that returns before a launch, the sampling helper on CPU tensors and the validation of
OmniBioTA.generate."""
import ctypes as C

import pytest
import torch

from omnibiote_amd import _lib

EINVAL, EUNSUPPORTED = -1, -3
MAX = _lib.ATTN_DECODE_MAX_SPLITS
P = 4096   # a non-null, 16-byte aligned "pointer" for calls that must return before they touch it


def _err():
    return _lib.lib().obte_last_error().decode()


def test_kv_cache_bytes():
    lib = _lib.lib()
    assert lib.obte_kv_cache_bytes(2, 77, 2, 64) == 2 * 2 * 2 * 77 * 64 * 2
    assert lib.obte_kv_cache_bytes(8, 2048, 8, 128) == 2 * 8 * 8 * 2048 * 128 * 2
    assert lib.obte_kv_cache_bytes(2, 77, 2, 32) == 0      # head size 32
    assert lib.obte_kv_cache_bytes(0, 77, 2, 64) == 0
    assert lib.obte_kv_cache_bytes(2, 0, 2, 64) == 0


def test_workspace_sizes():
    lib = _lib.lib()
    for B, H, hs in [(2, 2, 64), (8, 8, 128), (1, 1, 128)]:
        n = lib.obte_attn_decode_ws_bytes(B, H, hs)
        assert n >= B * H * MAX * (hs + 2) * 4 > 0
    assert lib.obte_attn_decode_ws_bytes(2, 2, 32) == 0
    assert lib.obte_block_decode_ws_bytes(2, 256, 2) >= lib.obte_block_infer_ws_bytes(2, 1, 256, 2) + lib.obte_attn_decode_ws_bytes(2, 2, 128)
    assert lib.obte_block_decode_ws_bytes(2, 128, 4) == 0      # head size 32
    assert lib.obte_block_decode_ws_bytes(0, 128, 2) == 0
    assert lib.obte_block_decode_ws_bytes(2, 8192, 64) == 0    # n_embd beyond 4096


def test_default_split_rule():
    lib = _lib.lib()
    keys = [1, 2, 63, 64, 65, 128, 255, 256, 257, 600, 1024, 1100, 2048, 4096, 65536]
    heads = [(1, 1), (1, 8), (2, 2), (8, 8), (64, 8), (256, 16)]
    for hs in (64, 128):
        table = {}
        for B, H in heads:
            row = [lib.obte_attn_decode_splits(B, H, hs, n) for n in keys]
            assert all(1 <= v <= MAX for v in row), row
            assert row[0] == 1                                                     # one key: nothing to split
            assert all(a <= b for a, b in zip(row, row[1:])), row                  # never fewer splits for more keys
            assert row == [lib.obte_attn_decode_splits(B, H, hs, n) for n in keys]  # a pure function
            table[B * H] = row
        order = sorted(table)
        for lo, hi in zip(order, order[1:]):                                       # never more splits for more (b, h)
            assert all(a >= b for a, b in zip(table[lo], table[hi])), (lo, hi)


def _call_decode(q=P, q_ld=128, cache=P, o=P, lse=None, B=1, T_max=100, n_keys=10, H=1, hs=128, splits=1, ws=None, ws_bytes=0):
    return _lib.lib().obte_attn_decode(q, q_ld, cache, o, lse, B, T_max, n_keys, H, hs, 1.0, splits, ws, ws_bytes, None)


@pytest.mark.parametrize("kw,word", [
    (dict(q=None), "null"), (dict(cache=None), "null"), (dict(o=None), "null"),
    (dict(n_keys=0), "n_keys"), (dict(n_keys=101), "n_keys"),
    (dict(splits=MAX + 1), "splits"), (dict(splits=-1), "splits"),
    (dict(splits=2, ws=P, ws_bytes=64), "workspace"), (dict(splits=2, ws=None, ws_bytes=1 << 20), "workspace"),
    (dict(hs=32), "head_dim"),
])
def test_attn_decode_rejects_before_any_launch(kw, word):
    assert _call_decode(**kw) == EINVAL
    assert _err().startswith("obte_attn_decode:") and word in _err(), _err()


def test_kv_cache_store_rejects_before_any_launch():
    lib = _lib.lib()
    assert lib.obte_kv_cache_store(None, 1, 1, 1, 64, P, 10, 0, None) == EINVAL
    assert _err().startswith("obte_kv_cache_store:") and "null" in _err()
    assert lib.obte_kv_cache_store(P, 1, 1, 1, 64, None, 10, 0, None) == EINVAL
    assert lib.obte_kv_cache_store(P, 1, 5, 1, 64, P, 10, 6, None) == EINVAL          # pos0 + t > T_max
    assert _err().startswith("obte_kv_cache_store:") and "T_max" in _err(), _err()
    assert lib.obte_kv_cache_store(P, 1, 11, 1, 64, P, 10, 0, None) == EINVAL
    assert lib.obte_kv_cache_store(P, 1, 1, 1, 32, P, 10, 0, None) == EINVAL


def _desc(B=2, T=1, C_=256, H=2, **over):
    f = dict(B=B, T=T, n_embd=C_, n_head=H, ln1_w=P, attn_w=P, proj_w=P, ln2_w=P, fc_w=P, mlp_w=P, rope_cos=P, rope_sin=P)
    f.update(over)
    return _lib.BlockDesc(**f)


def test_block_decode_and_prefill_reject_before_any_launch():
    lib = _lib.lib()
    big = 1 << 30

    def decode(d, x=P, y=P, kv=P, T_max=100, pos=5, ws=P, ws_bytes=big):
        return lib.obte_block_decode(C.byref(d) if d is not None else None, x, y, kv, T_max, pos, ws, ws_bytes, None)
    assert decode(None) == EINVAL and "obte_block_decode" in _err() and "null" in _err()
    assert decode(_desc(T=2)) == EINVAL
    assert _err().startswith("obte_block_decode:") and "T = 1" in _err(), _err()
    for over in (dict(key_ranges=P), dict(out_rows=P, n_out_rows=1), dict(dropout_p=0.1), dict(mask=P), dict(query_bounds=P)):
        assert decode(_desc(**over)) == EUNSUPPORTED, over
        assert _err().startswith("obte_block_decode:"), _err()
    assert decode(_desc(), x=None) == EINVAL and "null" in _err()
    assert decode(_desc(), kv=None) == EINVAL and "null" in _err()
    assert decode(_desc(), pos=100) == EINVAL and "position" in _err()
    assert decode(_desc(), ws_bytes=lib.obte_block_decode_ws_bytes(2, 256, 2) - 1) == EINVAL
    assert _err().startswith("obte_block_decode:") and "workspace" in _err(), _err()
    assert decode(_desc(C_=128, H=4)) == EINVAL                       # head size 32

    def prefill(d, x=P, y=P, ws=P, ws_bytes=big, kv=P, T_max=100):
        return lib.obte_block_fwd_prefill(C.byref(d) if d is not None else None, x, y, ws, ws_bytes, kv, T_max, None)
    assert prefill(None) == EINVAL and "obte_block_fwd_prefill" in _err()
    assert prefill(_desc(T=64), kv=None) == EINVAL and _err().startswith("obte_block_fwd_prefill:") and "null" in _err()
    assert prefill(_desc(T=101)) == EINVAL and "T_max" in _err()
    assert prefill(_desc(T=64, out_rows=P, n_out_rows=1)) == EUNSUPPORTED and _err().startswith("obte_block_fwd_prefill:")
    assert prefill(_desc(T=64), ws_bytes=16) == EINVAL and "workspace" in _err()


def test_existing_abi_pins_hold():
    lib = _lib.lib()
    assert lib.obte_abi_version() == 1
    sizes = (C.c_int64 * 16)()
    assert lib.obte_struct_sizes(sizes, 16) == 6
    for name in ("obte_kv_cache_bytes", "obte_kv_cache_store", "obte_attn_decode_ws_bytes", "obte_attn_decode_splits", "obte_attn_decode",
                 "obte_block_fwd_prefill", "obte_block_decode_ws_bytes", "obte_block_decode"):
        assert name in _lib.SYMBOLS
    assert list(_lib.SYMBOLS)[-8] == "obte_kv_cache_bytes"      # appended


# ------------------------------------------------------------------------------------------------------- sampling
def test_sample_next_greedy_forms_are_the_argmax():
    from omnibiote_amd.model import sample_next
    logits = torch.randn(5, 97, generator=torch.Generator().manual_seed(0))
    want = logits.argmax(dim=-1)
    assert torch.equal(sample_next(logits, top_k=1), want)
    assert torch.equal(sample_next(logits, temperature=0), want)
    assert torch.equal(sample_next(logits, temperature=0.0, top_k=10), want)
    assert sample_next(logits, top_k=1).dtype == torch.int64 and sample_next(logits).shape == (5,)


def test_sample_next_top_k_stays_in_the_top_k_and_follows_its_generator():
    from omnibiote_amd.model import sample_next
    logits = torch.randn(4, 64, generator=torch.Generator().manual_seed(1))
    k = 5
    top = logits.topk(k, dim=-1).indices
    g = torch.Generator().manual_seed(7)
    draws = [sample_next(logits, temperature=1.3, top_k=k, generator=g) for _ in range(200)]
    for d in draws:
        assert (d.unsqueeze(1) == top).any(dim=1).all()
    assert len({tuple(d.tolist()) for d in draws}) > 1           # it does sample
    a = [sample_next(logits, 0.8, None, torch.Generator().manual_seed(3)) for _ in range(1)]
    ga, gb = torch.Generator().manual_seed(3), torch.Generator().manual_seed(3)
    assert all(torch.equal(sample_next(logits, 0.8, 9, ga), sample_next(logits, 0.8, 9, gb)) for _ in range(20))
    assert torch.equal(a[0], sample_next(logits, 0.8, None, torch.Generator().manual_seed(3)))


def _cpu_model(autoregressive, block_size=32):
    from omnibiote_amd.model import OmniBioTA, OmniBioTAConfig
    c = OmniBioTAConfig()
    c.block_size, c.vocab_size, c.n_layer, c.n_head, c.n_embd, c.dropout, c.flash = block_size, 64, 1, 2, 128, 0.0, True
    c.autoregressive = autoregressive
    return OmniBioTA(c)


def test_generate_validates_before_any_device_work():
    from omnibiote_amd.model import KVCache
    idx = torch.zeros(2, 8, dtype=torch.int64)
    enc, ar = _cpu_model(False), _cpu_model(True)
    with pytest.raises(ValueError, match="autoregressive"):
        enc.generate(idx, 4)
    with pytest.raises(ValueError, match="autoregressive"):
        KVCache(enc, 2)
    with pytest.raises(ValueError, match="block_size"):
        ar.generate(idx, 25)                                       # 8 + 25 > 32
    with pytest.raises(ValueError, match="empty"):
        ar.generate(torch.zeros(2, 0, dtype=torch.int64), 4)
    with pytest.raises(ValueError, match="max_len"):
        KVCache(ar, 2, max_len=33)
