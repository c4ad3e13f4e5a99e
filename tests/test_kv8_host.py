"""Host-side tests (no GPU) of the e4m3 key/value cache (include/omnibiote_hip_kv8.h): the symbol table against the header, the pins of the
ABI, obte_kv8_cache_bytes, every argument check that returns before a launch, the format's yardstick (omnibiote_amd/kvquant.py), and
the operations an fp8 cache refuses, on a CPU model with a cache's position state alone."""
import ctypes as C
import math
import os
import re

import pytest
import torch

from omnibiote_amd import _lib, kvquant

EINVAL, EUNSUPPORTED = -1, -3
P = 4096   # a non-null, 16-byte aligned "pointer" for calls that must return before they touch it
NAMES = ("obte_kv8_cache_bytes", "obte_kv8_cache_store", "obte_kv8_cache_rope_store_rows", "obte_attn_decode_kv8", "obte_block_fwd_prefill_kv8",
         "obte_block_decode_kv8")


def _err():
    return _lib.lib().obte_last_error().decode()


def test_symbols_are_what_the_header_declares():
    assert tuple(_lib.SYMBOLS_KV8) == NAMES
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "omnibiote_hip_kv8.h")).read()
    body = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    assert tuple(re.findall(r"\b(obte_\w+)\s*\(", body)) == NAMES                  # the declarations, in order
    assert '#include "omnibiote_hip.h"' in header and "struct" not in body
    lib = _lib.lib()
    for name in NAMES:
        for table in (_lib.SYMBOLS, _lib.SYMBOLS_ROWS, _lib.SYMBOLS_SMALL_M, _lib.SYMBOLS_SAMPLE, _lib.SYMBOLS_EXTEND, _lib.SYMBOLS_SPEC):
            assert name not in table
        res, args = _lib.SYMBOLS_KV8[name]
        fn = getattr(lib, name)
        assert fn.restype is res and list(fn.argtypes) == args                      # bound by lib(), in the same loop
    assert len(_lib.SYMBOLS) == 70 and len(_lib.SYMBOLS_ROWS) == 3 and len(_lib.SYMBOLS_SMALL_M) == 3 and len(_lib.SYMBOLS_SAMPLE) == 1
    assert len(_lib.SYMBOLS_EXTEND) == 6 and len(_lib.SYMBOLS_SPEC) == 2
    assert lib.obte_abi_version() == 1
    sizes = (C.c_int64 * 16)()
    assert lib.obte_struct_sizes(sizes, 16) == 6


def test_cache_bytes():
    f = _lib.lib().obte_kv8_cache_bytes
    assert f(1, 1, 1, 64) == 2 * 68 and f(2, 77, 2, 128) == 2 * 2 * 2 * 77 * 132 and f(64, 2048, 8, 128) == 2 * 64 * 8 * 2048 * 132
    for B, T, H, hs in [(2, 77, 2, 64), (3, 1100, 5, 128)]:
        assert f(B, T, H, hs) == kvquant.cache_bytes(B, T, H, hs)
        assert f(B, T, H, hs) * 2 * hs == _lib.lib().obte_kv_cache_bytes(B, T, H, hs) * (hs + 4)     # (hs + 4) / (2 hs) of the bf16 cache
    assert f(2, 77, 2, 32) == 0 and f(2, 77, 2, 256) == 0 and f(0, 77, 2, 64) == 0 and f(2, 0, 2, 64) == 0 and f(2, 77, 0, 64) == 0
    assert f(2, 1 << 24, 2, 64) == 0 and f(-1, 77, 2, 64) == 0


def _store(qkv=P, B=2, t=4, H=2, hs=64, cache=P, T_max=100, pos0=5):
    return _lib.lib().obte_kv8_cache_store(qkv, B, t, H, hs, cache, T_max, pos0, None)


@pytest.mark.parametrize("kw,word", [
    (dict(qkv=None), "null"), (dict(cache=None), "null"), (dict(hs=32), "head_dim"), (dict(B=0), "shape"), (dict(t=0), "fit"), (dict(pos0=97), "fit"),
    (dict(pos0=-1), "fit"), (dict(pos0=100, t=1), "fit"), (dict(qkv=P + 8), "aligned"), (dict(cache=P + 8), "aligned"),
])
def test_store_rejects_before_any_launch(kw, word):
    assert _store(**kw) == EINVAL
    assert _err().startswith("obte_kv8_cache_store:") and word in _err(), _err()


def _store_rows(qkv=P, cos=P, sin=P, pos=P, max_pos=10, B=2, H=2, hs=64, cache=P, T_max=100):
    return _lib.lib().obte_kv8_cache_rope_store_rows(qkv, cos, sin, pos, max_pos, B, H, hs, cache, T_max, None)


@pytest.mark.parametrize("kw,word", [
    (dict(qkv=None), "null"), (dict(cos=None), "null"), (dict(sin=None), "null"), (dict(pos=None), "null"), (dict(cache=None), "null"),
    (dict(hs=32), "head_dim"), (dict(B=0), "shape"), (dict(max_pos=100), "max_pos"), (dict(max_pos=-1), "max_pos"), (dict(pos=P + 2), "aligned"),
    (dict(qkv=P + 8), "aligned"), (dict(cache=P + 8), "aligned"), (dict(cos=P + 4), "aligned"),
])
def test_rope_store_rows_rejects_before_any_launch(kw, word):
    assert _store_rows(**kw) == EINVAL
    assert _err().startswith("obte_kv8_cache_rope_store_rows:") and word in _err(), _err()


def _decode(q=P, q_ld=128, cache=P, o=P, lse=None, B=1, T_max=100, n_keys=10, rows=None, H=1, hs=128, splits=1, ws=None, ws_bytes=0):
    return _lib.lib().obte_attn_decode_kv8(q, q_ld, cache, o, lse, B, T_max, n_keys, rows, H, hs, 1.0, splits, ws, ws_bytes, None)


@pytest.mark.parametrize("kw,word", [
    (dict(q=None), "null"), (dict(cache=None), "null"), (dict(o=None), "null"),
    (dict(n_keys=0), "n_keys"), (dict(n_keys=101), "n_keys"), (dict(n_keys=-3), "n_keys"),
    (dict(splits=-1), "splits"), (dict(splits=_lib.ATTN_DECODE_MAX_SPLITS + 1), "splits"),
    (dict(splits=2), "workspace"), (dict(splits=2, ws=P, ws_bytes=64), "workspace"), (dict(splits=2, ws=P + 4, ws_bytes=1 << 30), "workspace"),
    (dict(splits=0, T_max=4096, n_keys=4096), "workspace"),                           # the default count at 4096 keys is above 1
    (dict(hs=32, q_ld=32), "head_dim"), (dict(q_ld=132), "q_ld"), (dict(q_ld=64), "q_ld"), (dict(q=P + 8), "aligned"), (dict(cache=P + 8), "aligned"),
    (dict(o=P + 8), "aligned"), (dict(B=0), "shape"), (dict(rows=P + 2), "aligned"), (dict(B=8192, H=8, q_ld=1024), "B * n_head"),
])
def test_attn_decode_kv8_rejects_before_any_launch(kw, word):
    assert _decode(**kw) == EINVAL
    assert _err().startswith("obte_attn_decode_kv8:") and word in _err(), _err()


def _desc(B=2, T=1, C_=256, H=2, **over):
    f = dict(B=B, T=T, n_embd=C_, n_head=H, ln1_w=P, attn_w=P, proj_w=P, ln2_w=P, fc_w=P, mlp_w=P, rope_cos=P, rope_sin=P)
    f.update(over)
    return _lib.BlockDesc(**f)


def test_block_decode_kv8_rejects_before_any_launch():
    lib = _lib.lib()
    big = 1 << 30

    def step(d, x=P, y=P, kv=P, T_max=100, pos=5, pos_rows=None, ws=P, ws_bytes=big):
        return lib.obte_block_decode_kv8(C.byref(d) if d is not None else None, x, y, kv, T_max, pos, pos_rows, ws, ws_bytes, None)
    assert step(None) == EINVAL and "obte_block_decode_kv8" in _err() and "null" in _err()
    for over in (dict(key_ranges=P), dict(out_rows=P, n_out_rows=1), dict(dropout_p=0.1), dict(mask=P), dict(query_bounds=P)):
        assert step(_desc(**over)) == EUNSUPPORTED, over
        assert _err().startswith("obte_block_decode_kv8:"), _err()
    for kw in (dict(x=None), dict(y=None), dict(kv=None), dict(ws=None)):
        assert step(_desc(), **kw) == EINVAL and _err().startswith("obte_block_decode_kv8:") and "null" in _err(), (kw, _err())
    assert step(_desc(T=2)) == EINVAL and "T = 1" in _err()
    for rows in (None, P):
        assert step(_desc(), pos=100, pos_rows=rows) == EINVAL and "outside the cache" in _err(), _err()     # pos >= T_max
        assert step(_desc(), pos=-1, pos_rows=rows) == EINVAL and "outside the cache" in _err(), _err()
    assert step(_desc(), kv=P + 8) == EINVAL and "aligned" in _err()
    assert step(_desc(), pos_rows=P + 2) == EINVAL and "aligned" in _err()
    assert step(_desc(B=40000)) == EINVAL and "B * n_head" in _err()
    assert step(_desc(), ws_bytes=lib.obte_block_decode_ws_bytes(2, 256, 2) - 1) == EINVAL
    assert _err().startswith("obte_block_decode_kv8:") and "workspace" in _err(), _err()
    assert step(_desc(C_=128, H=4)) == EINVAL                            # head size 32
    assert _err().startswith("obte_block_decode_kv8:") and "head" in _err(), _err()


def test_block_prefill_kv8_rejects_before_any_launch():
    lib = _lib.lib()
    big = 1 << 30

    def prefill(d, x=P, y=P, ws=P, ws_bytes=big, kv=P, T_max=100):
        return lib.obte_block_fwd_prefill_kv8(C.byref(d) if d is not None else None, x, y, ws, ws_bytes, kv, T_max, None)
    assert prefill(None) == EINVAL and "obte_block_fwd_prefill_kv8" in _err() and "null" in _err()
    assert prefill(_desc(T=4, out_rows=P, n_out_rows=1)) == EUNSUPPORTED and _err().startswith("obte_block_fwd_prefill_kv8:")
    for kw in (dict(x=None), dict(y=None), dict(kv=None), dict(ws=None)):
        assert prefill(_desc(T=4), **kw) == EINVAL and _err().startswith("obte_block_fwd_prefill_kv8:") and "null" in _err(), (kw, _err())
    assert prefill(_desc(T=101)) == EINVAL and "fit" in _err()
    assert prefill(_desc(T=4), kv=P + 8) == EINVAL and "aligned" in _err()
    assert prefill(_desc(T=4), ws_bytes=lib.obte_block_infer_ws_bytes(2, 4, 256, 2) - 1) == EINVAL and "workspace" in _err()
    assert prefill(_desc(T=4, C_=128, H=4)) == EINVAL and "head" in _err()        # head size 32


# ------------------------------------------------------------------------------------------------------- the format's yardstick
def _bf16_bits(v):
    return torch.tensor(v, dtype=torch.int32).to(torch.int16).view(torch.bfloat16)


def _vectors(hs=64):
    """bf16 head vectors with per-vector magnitudes over 2^+-30, the zero vector, maxima exactly at 448 * 2^j and one ulp above, bf16's
    largest finite value and its subnormals"""
    g = torch.Generator().manual_seed(5)
    x = torch.randn(70, hs, generator=g) * torch.exp2(torch.randint(-30, 31, (70, 1), generator=g).float())
    x = x.bfloat16()
    x[0] = 0
    for i, j in enumerate((-20, -3, 0, 1, 7, 20)):
        x[1 + i] = (torch.rand(hs, generator=g) * 2 - 1) * 2.0 ** j                # below the maximum planted next
        x[1 + i, 3 * i] = -448.0 * 2.0 ** j
        x[7 + i] = x[1 + i]
        x[7 + i, 3 * i] = (x[1 + i, 3 * i].view(torch.int16) + 1).view(torch.bfloat16)   # one bf16 ulp further from zero
    x[13] = _bf16_bits(0x7F7F)                                                      # bf16 max
    x[14] = _bf16_bits([(1 + 3 * k) % 128 for k in range(hs)])                     # bf16 subnormals (and a zero)
    x[15] = 0
    x[15, 5] = _bf16_bits(0x0001)                                                   # the smallest subnormal alone
    return x


def test_quantize_reference_properties():
    x = _vectors()
    codes, scales = kvquant.quantize_reference(x)
    assert codes.dtype == torch.uint8 and codes.shape == x.shape and scales.dtype == torch.float32 and scales.shape == x.shape[:-1]
    m, e = torch.frexp(scales.double())
    assert bool((m == 0.5).all()) and int((e - 1).min()) >= -126                    # powers of two, at least 2^-126
    assert not bool(((codes & 0x7F) == 0x7F).any())                                 # never a NaN code
    amax = x.double().abs().amax(-1)
    scaled = amax / scales.double()
    assert bool((scaled <= 448).all())
    big = (e - 1) > -126                                                            # where the floor of -126 did not bind
    assert bool((scaled[big] > 224).all()) and bool(big[1:13].all())
    assert float(scales[0]) == 2.0 ** -126 and int(codes[0].max()) == 0             # the zero vector
    for i, j in enumerate((-20, -3, 0, 1, 7, 20)):
        assert float(scales[1 + i]) == 2.0 ** j and float(scales[7 + i]) == 2.0 ** (j + 1)   # 448 * 2^j exactly, and one ulp above
        assert int(codes[1 + i, 3 * i]) == 0xFE                                     # -448: the largest finite code, sign set
    assert float(scales[13]) == 2.0 ** 120 and bool((codes[13] == 0x78).all())      # bf16 max = 255 * 2^120 -> 256 (a tie, to even)
    assert float(scales[14]) == 2.0 ** -126 and float(scales[15]) == 2.0 ** -126
    assert int(codes[15, 5]) == 4 and int(codes[15].sum()) == 4                      # 2^-133 * 2^126 = 2^-7 = 4 * 2^-9, e4m3's smallest subnormal
    assert bool((codes[14].long() == torch.tensor([(1 + 3 * k) % 128 for k in range(64)]).double().mul(2.0 ** -7).float()
                 .to(torch.float8_e4m3fn).view(torch.uint8).long()).all())          # k * 2^-133 -> RNE_e4m3(k * 2^-7)
    back = kvquant.dequantize_reference(codes, scales).double()
    xd = x.double()
    ok = (xd.abs() / scales.double().unsqueeze(-1)) >= 2.0 ** -6                    # e4m3's normal range under this scale
    finite = torch.isfinite(back)                                                   # (256 * 2^120 overflows fp32: row 13 is judged in float64)
    back = torch.where(finite, back, codes.view(torch.float8_e4m3fn).double() * scales.double().unsqueeze(-1))
    assert bool(((back - xd).abs() <= 2.0 ** -4 * xd.abs())[ok].all())
    assert bool(ok[1:13].any(-1).all())


def test_dequantize_then_quantize_is_the_identity_on_representable_vectors():
    g = torch.Generator().manual_seed(6)
    codes = torch.randint(0, 256, (64, 128), generator=g, dtype=torch.int64).to(torch.uint8)
    codes[(codes & 0x7F) == 0x7F] = 0x31                                            # no NaN codes
    codes[:, 0] = 0x7E                                                              # the maximum is 448: the scale stays where it was
    codes[0] = 0                                                                    # (a zero vector comes back at the floor scale)
    scales = torch.exp2(torch.randint(-110, 118, (64,), generator=g).float())       # (2^-9 * 2^-110 is still a bf16)
    scales[0] = 2.0 ** -126
    x = kvquant.dequantize_reference(codes, scales)
    assert bool((x.bfloat16().float() == x).all())                                  # 4 significant bits: every value is a bf16
    c2, s2 = kvquant.quantize_reference(x.bfloat16())
    assert torch.equal(s2, scales) and torch.equal(c2, codes)                       # (the sign of a zero included: -0 stays -0)
    assert math.isclose(float(x[1, 0]), 448.0 * float(scales[1]))


def test_split_cache_views():
    B, T, H, hs = 2, 5, 3, 64
    buf = torch.arange(kvquant.cache_bytes(B, T, H, hs), dtype=torch.int64).to(torch.uint8)
    kc, vc, ks, vs = kvquant.split_cache(buf, B, T, H, hs)
    n = B * H * T
    assert kc.shape == vc.shape == (B, H, T, hs) and ks.shape == vs.shape == (B, H, T) and ks.dtype == torch.float32
    assert kc.data_ptr() == buf.data_ptr() and vc.data_ptr() == buf.data_ptr() + n * hs
    assert ks.data_ptr() == buf.data_ptr() + 2 * n * hs and vs.data_ptr() == ks.data_ptr() + 4 * n
    with pytest.raises(ValueError):
        kvquant.split_cache(buf[:-1], B, T, H, hs)


# ------------------------------------------------------------------------------------------------------- the model surface
def _cpu_model(block_size=32):
    from omnibiote_amd.model import OmniBioTA, OmniBioTAConfig
    c = OmniBioTAConfig()
    c.block_size, c.vocab_size, c.n_layer, c.n_head, c.n_embd, c.dropout, c.flash = block_size, 64, 1, 2, 128, 0.0, True
    c.autoregressive = True
    return OmniBioTA(c)


def _fake(pos=8, batch=2, max_len=32, dtype="fp8"):
    """a cache's position state (the host-only class KVCache is built on) with no buffer behind it"""
    from omnibiote_amd.model import CachePositions
    c = CachePositions(batch, max_len)
    c.reset(pos)
    c.layers, c.decode_ws, c.extend_ws, c.dtype = [None], None, None, dtype
    return c


def test_fp8_cache_refuses_multi_position_operations_before_anything_else():
    from omnibiote_amd.model import CachePositions
    assert CachePositions(2, 8).dtype == "bf16"
    m = _cpu_model()
    c = _fake()
    with pytest.raises(NotImplementedError, match="fp8 cache"):
        m.extend(torch.zeros(2, 4, dtype=torch.int64), c)
    with pytest.raises(NotImplementedError, match="fp8 cache"):
        m.extend(torch.zeros(2, 1, dtype=torch.int64), c)
    with pytest.raises(NotImplementedError, match="fp8 cache"):
        m.prefill(torch.zeros(2, 8, dtype=torch.int64), c, chunk=4)
    with pytest.raises(NotImplementedError, match="fp8 cache"):
        m.draft_and_verify(m, torch.zeros(2, dtype=torch.int64), c, _fake(dtype="bf16"), 2)
    with pytest.raises(NotImplementedError, match="fp8"):
        m.generate_speculative(torch.zeros(2, 4, dtype=torch.int64), 4, m, kv_dtype="fp8")
    assert c.pos == 8 and c.positions is None
    with pytest.raises(ValueError, match="kv_dtype"):
        m.generate_speculative(torch.zeros(2, 4, dtype=torch.int64), 4, m, kv_dtype="int8")
    with pytest.raises(ValueError, match="kv_dtype"):
        m.generate(torch.zeros(2, 4, dtype=torch.int64), 4, kv_dtype="fp16")
    with pytest.raises(RuntimeError, match="GPU"):                                  # a bf16 cache goes on to the first device-side requirement
        m.extend(torch.zeros(2, 4, dtype=torch.int64), _fake(dtype="bf16"))


def test_kvcache_dtype_is_checked_first():
    from omnibiote_amd.model import KVCache
    with pytest.raises(ValueError, match="dtype"):
        KVCache(_cpu_model(), 2, dtype="int8")
