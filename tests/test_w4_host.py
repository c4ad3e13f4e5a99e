"""Host-side tests (no GPU) of the MXFP4 decode-step weights (include/omnibiote_hip_w4.h): the symbol table against the header, the format's
yardstick (omnibiote_amd/w4quant.py), every argument check that returns before a launch, and the model surface —
quantize_weights(format="mxfp4"), the stale snapshot, an unknown format, what refuses weights= — on a CPU model."""
import ctypes as C
import inspect
import os
import re

import pytest
import torch

from omnibiote_amd import _lib, w4quant

EINVAL, EUNSUPPORTED = -1, -3
P = 4096   # a non-null, 16-byte aligned "pointer" for calls that must return before they touch it
NAMES = ("obte_linear_small_m_w4", "obte_block_step_w4")
GRID = (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0)


def _err():
    return _lib.lib().obte_last_error().decode()


def test_symbols_are_what_the_header_declares():
    assert tuple(_lib.SYMBOLS_W4) == NAMES
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "omnibiote_hip_w4.h")).read()
    body = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    assert tuple(re.findall(r"\b(obte_\w+)\s*\(", body)) == NAMES                  # the declarations, in order
    assert '#include "omnibiote_hip.h"' in header and "struct" not in body
    lib = _lib.lib()
    for name in NAMES:
        for table in (getattr(_lib, t) for t in dir(_lib) if t.startswith("SYMBOLS") and t != "SYMBOLS_W4"):
            assert name not in table
        res, args = _lib.SYMBOLS_W4[name]
        fn = getattr(lib, name)
        assert fn.restype is res and list(fn.argtypes) == args                      # bound by lib(), in the same loop
    assert _lib.SYMBOLS_W4["obte_block_step_w4"] == _lib.SYMBOLS_W8["obte_block_step_w8"]          # the w8 step's argument list
    assert len(_lib.SYMBOLS_W8) == 2 and len(_lib.SYMBOLS) == 70                    # the tables beside it as they were
    assert lib.obte_abi_version() == 1
    sizes = (C.c_int64 * 16)()
    assert lib.obte_struct_sizes(sizes, 16) == 6                                    # no new struct
    makefile = open(os.path.join(root, "omnibiote_amd", "csrc", "Makefile")).read()
    assert "omnibiote_hip_w4.h" in makefile


# ------------------------------------------------------------------------------------------------------- the product's checks
def _gemm(M=2, N=16, K=64, epi=0, alpha=1.0, a=P, d=P, aux=None, lda=None, ldd=None, **more):
    return _lib.GemmArgs(a=a, b=None, d=d, aux=aux, M=M, N=N, K=K, lda=K if lda is None else lda, ldb=0, ldd=N if ldd is None else ldd, a_kmajor=1,
                         b_kmajor=1, epilogue=epi, alpha=alpha, **more)


def _product(g, codes=P, ld=None, scales=P, lds=None):
    k = g.K if g is not None else 0
    return _lib.lib().obte_linear_small_m_w4(C.byref(g) if g is not None else None, codes, k // 2 if ld is None else ld, scales, k // 32 if lds is None else lds, None)


@pytest.mark.parametrize("g,kw,rc,word", [
    (None, {}, EINVAL, "null"), (dict(a=None), {}, EINVAL, "null"), (dict(d=None), {}, EINVAL, "null"),
    ({}, dict(codes=None), EINVAL, "null"), ({}, dict(scales=None), EINVAL, "null"),
    (dict(M=0), {}, EINVAL, "M must be"), (dict(M=65), {}, EINVAL, "M must be"), (dict(K=96), {}, EINVAL, "K"), (dict(N=12), {}, EINVAL, "multiples of 8"),
    (dict(lda=56), {}, EINVAL, "leading dimension"), (dict(ldd=8), {}, EINVAL, "leading dimension"),
    ({}, dict(ld=36), EINVAL, "ld_codes"), ({}, dict(ld=24), EINVAL, "ld_codes"), ({}, dict(lds=3), EINVAL, "ld_scales"), (dict(K=128), dict(lds=2), EINVAL, "ld_scales"),
    ({}, dict(codes=P + 4), EINVAL, "aligned"), ({}, dict(scales=P + 1), EINVAL, "aligned"),
    (dict(epi=1), {}, EUNSUPPORTED, "epilogue"), (dict(epi=4), {}, EUNSUPPORTED, "epilogue"), (dict(a_kmajor=0), {}, EUNSUPPORTED, "layout"),
    (dict(epi=2), {}, EINVAL, "aux"), (dict(epi=9, alpha=0.5), {}, EINVAL, "alpha"), (dict(epi=5, N=48), {}, EINVAL, "ROPE"),
])
def test_product_rejects_before_any_launch(g, kw, rc, word):
    if g is not None and "a_kmajor" in g:
        args = _gemm()
        args.a_kmajor = 0
    else:
        args = None if g is None else _gemm(**g)
    assert _product(args, **kw) == rc
    assert _err().startswith("obte_linear_small_m_w4:") and word in _err(), _err()


def test_product_ignores_b_and_ldb():
    """g->b null and ldb 0 pass the checks: the call is refused for something else"""
    assert _product(_gemm(M=65)) == EINVAL and "M must be" in _err()


def _desc(B=2, T=1, C_=256, H=2, **over):
    f = dict(B=B, T=T, n_embd=C_, n_head=H, ln1_w=P, attn_w=P, proj_w=P, ln2_w=P, fc_w=P, mlp_w=P, rope_cos=P, rope_sin=P)
    f.update(over)
    return _lib.BlockDesc(**f)


def test_block_step_w4_rejects_before_any_launch():
    lib = _lib.lib()
    big = 1 << 30
    four = (C.c_void_p * 4)(P, P, P, P)

    def step(d, codes=four, scales=four, x=P, y=P, kv=P, e4m3=0, T_max=100, pos=5, pos_rows=None, ws=P, ws_bytes=big):
        return lib.obte_block_step_w4(C.byref(d) if d is not None else None, codes, scales, x, y, kv, e4m3, T_max, pos, pos_rows, ws, ws_bytes, None)
    assert step(None) == EINVAL and "obte_block_step_w4" in _err() and "null" in _err()
    assert step(_desc(), codes=None) == EINVAL and _err().startswith("obte_block_step_w4:") and "null" in _err()
    assert step(_desc(), scales=None) == EINVAL and "null" in _err()
    assert step(_desc(), codes=(C.c_void_p * 4)(P, P, None, P)) == EINVAL and "codes[2]" in _err()
    assert step(_desc(), codes=(C.c_void_p * 4)(P, P + 4, P, P)) == EINVAL and "aligned" in _err()
    assert step(_desc(), scales=(C.c_void_p * 4)(P, P, P, P + 1)) == EINVAL and "aligned" in _err()
    for over in (dict(key_ranges=P), dict(out_rows=P, n_out_rows=1), dict(dropout_p=0.1), dict(mask=P), dict(query_bounds=P)):
        assert step(_desc(**over)) == EUNSUPPORTED, over
        assert _err().startswith("obte_block_step_w4:"), _err()
    for kw in (dict(x=None), dict(y=None), dict(kv=None), dict(ws=None)):
        assert step(_desc(), **kw) == EINVAL and _err().startswith("obte_block_step_w4:") and "null" in _err(), (kw, _err())
    assert step(_desc(T=2)) == EINVAL and "T = 1" in _err()
    for rows in (None, P):
        for e4m3 in (0, 1):
            assert step(_desc(), pos=100, pos_rows=rows, e4m3=e4m3) == EINVAL and "outside the cache" in _err(), _err()
            assert step(_desc(), pos=-1, pos_rows=rows, e4m3=e4m3) == EINVAL and "outside the cache" in _err(), _err()
    assert step(_desc(), kv=P + 8, e4m3=1) == EINVAL and "aligned" in _err()
    assert step(_desc(), ws_bytes=lib.obte_block_decode_ws_bytes(2, 256, 2) - 1) == EINVAL
    assert _err().startswith("obte_block_step_w4:") and "workspace" in _err(), _err()
    assert step(_desc(C_=128, H=4)) == EINVAL and "head" in _err()                # head size 32


# ------------------------------------------------------------------------------------------------------- the format's yardstick
def _weight(N=40, K=192, seed=5):
    """N(0, 0.02) with a zero row, a row whose blocks differ by 2^12 from one to the next, a row x 2^-20 and a row x 2^10"""
    g = torch.Generator().manual_seed(seed)
    w = (torch.randn(N, K, generator=g) * 0.02).bfloat16()
    w[3] = 0
    w[5] = (w[5].float() * torch.exp2(12.0 * (torch.arange(K // 32) % 2) - 6).repeat_interleave(32)).bfloat16()
    w[6] = (w[6].float() * 2.0 ** -20).bfloat16()
    w[7] = (w[7].float() * 2.0 ** 10).bfloat16()
    return w


def _values(codes_k):
    """the value of each code (k order, one per byte) as float64, -0 for 0x8"""
    t = torch.tensor(GRID + tuple(-g for g in GRID), dtype=torch.float64)
    return t[codes_k.long()]


def test_format_properties():
    w = _weight()
    N, K = w.shape
    codes, scales = w4quant.quantize_weight(w)
    assert codes.dtype == torch.uint8 and codes.shape == (N, K // 2) and scales.dtype == torch.uint8 and scales.shape == (N, K // 32)
    assert codes.numel() == N * K // 2 and scales.numel() == N * K // 32
    plain = w4quant.unpack_codes(codes)
    assert not bool((plain == 8).any()) and int(plain.max()) <= 15                  # never -0
    assert int(scales.min()) >= 2 and int(scales.max()) <= 253                      # never 0, 1 or the NaN byte (nor 254)
    assert int(codes[3].max()) == 0 and bool((scales[3] == 2).all())                # the zero blocks: e = -125
    e = scales.double() - 127
    scaled_max = w.double().reshape(N, -1, 32).abs().amax(-1) * torch.exp2(-e)
    live = scales > 2
    assert bool((scaled_max <= 6).all()) and bool((scaled_max[live] > 3).all())     # the smallest e: nothing saturates, the top binade is used
    assert float(_values(plain).abs().reshape(N, -1, 32).amax(-1)[live].min()) >= 3
    deq = w4quant.dequantize_weight(codes, scales)
    assert deq.dtype == torch.bfloat16 and deq.shape == w.shape
    exact = (_values(plain).reshape(N, -1, 32) * torch.exp2(e).unsqueeze(-1)).reshape(N, K)
    assert torch.equal(deq.double(), exact)                                         # every value survives bf16
    assert torch.equal(deq.float().bfloat16(), deq) and bool(torch.isfinite(deq).all())
    amax = w.double().reshape(N, -1, 32).abs().amax(-1, keepdim=True)
    err = (deq.double() - w.double()).abs().reshape(N, -1, 32)
    assert bool((err[live] < (amax / 3)[live]).all()) and bool((err[~live] == 0).all())


def test_rounding_is_to_nearest_ties_to_the_even_code():
    """one block per row whose maximum 6 pins the scale at 2^0: every grid value, every midpoint and a value on either side of each"""
    mids = [(a + b) / 2 for a, b in zip(GRID, GRID[1:])]
    want_mid = [0.0, 1.0, 1.0, 2.0, 2.0, 4.0, 4.0]                                  # the neighbour whose code is even
    probe = list(GRID) + mids + [m - 2.0 ** -5 for m in mids] + [m + 2.0 ** -5 for m in mids]
    want = list(GRID) + want_mid + list(GRID[:-1]) + list(GRID[1:])
    w = torch.zeros(2, 64, dtype=torch.bfloat16)
    w[0, :len(probe)] = torch.tensor(probe).bfloat16()
    w[1, :len(probe)] = -torch.tensor(probe).bfloat16()
    w[:, 31], w[:, 63] = 6, 6
    assert torch.equal(w[0, :len(probe)].double(), torch.tensor(probe, dtype=torch.float64))      # the probes are bf16 values
    codes, scales = w4quant.quantize_weight(w)
    assert bool((scales == 127).all())
    deq = w4quant.dequantize_weight(codes, scales).double()
    assert deq[0, :len(probe)].tolist() == want and deq[1, :len(probe)].tolist() == [-v for v in want]
    assert not bool((w4quant.unpack_codes(codes) == 8).any())                       # -0.25 and its like round to +0


def test_quantising_a_dequantised_weight_is_a_fixed_point():
    """A block whose scaled maximum lay in (3, 3.5) rounds to a maximum of 3, and the rule — the SMALLEST e — then writes the same values
    one scale lower (3 * 2^e = 6 * 2^(e - 1), and the rest of such a block, multiples of 0.5 up to 3, doubles onto the grid too).  So: every
    other block keeps its codes and its scale at once; such a block keeps its VALUES, bit for bit, under the scale byte below; and from there
    on codes and scales stay as they are."""
    codes, scales = w4quant.quantize_weight(_weight())
    deq = w4quant.dequantize_weight(codes, scales)
    again = w4quant.quantize_weight(deq)
    assert torch.equal(w4quant.dequantize_weight(*again).view(torch.int16), deq.view(torch.int16))
    top = _values(w4quant.unpack_codes(codes)).abs().reshape(codes.shape[0], -1, 32).amax(-1)
    same = (top > 3) | (scales == 2)
    assert bool(same.any()) and bool((~same).any()) and bool((top[~same] == 3).all())
    assert torch.equal(again[1][same], scales[same]) and torch.equal(again[1][~same].long(), scales[~same].long() - 1)
    by_block = lambda c: w4quant.unpack_codes(c).reshape(c.shape[0], -1, 32)
    assert torch.equal(by_block(again[0])[same], by_block(codes)[same])
    third = w4quant.quantize_weight(w4quant.dequantize_weight(*again))
    assert torch.equal(third[0], again[0]) and torch.equal(third[1], again[1])


def test_codes_do_not_depend_on_the_magnitude():
    w = _weight()
    codes, scales = w4quant.quantize_weight(w)
    for j in (-20, 10):
        c2, s2 = w4quant.quantize_weight((w.float() * 2.0 ** j).bfloat16())        # a power of two: exact in bf16
        assert torch.equal(c2, codes)
        live = scales > 2
        assert torch.equal(s2[live].long(), scales[live].long() + j) and bool((s2[~live] == 2).all())


def test_corners_the_largest_values_and_the_floor_scale():
    big = torch.tensor([0x7F7F], dtype=torch.int16).view(torch.bfloat16)            # bf16's largest value
    w = torch.zeros(3, 64, dtype=torch.bfloat16)
    w[0, 0], w[0, 1] = big.item(), 2.0 ** 127
    w[1, 0], w[1, 1], w[1, 2] = 2.0 ** -126, 2.0 ** -127, 1.5 * 2.0 ** -126         # under the floor scale: the grid of 2^-126
    w[2, 0], w[2, 32] = 1.5 * 2.0 ** -124, 3.5 * 2.0 ** -124                       # the largest clamped maximum; the first block above it
    codes, scales = w4quant.quantize_weight(w)
    assert scales[0].tolist() == [253, 2] and scales[1].tolist() == [2, 2] and scales[2].tolist() == [2, 3]
    deq = w4quant.dequantize_weight(codes, scales)
    assert deq[0, 0].item() == float("inf") and deq[0, 1].item() == 2.0 ** 127      # the code of 4 under 2^126 is 2^128
    assert deq[1, :3].double().tolist() == [2.0 ** -126, 0.0, 2.0 ** -125]          # a tie to the even code on either side
    assert deq[2, 0].item() == 1.5 * 2.0 ** -124 and deq[2, 32].item() == 2.0 ** -122
    # what the quantiser never writes, the dequantiser still reads: -0, the NaN scale, the bytes below 2
    c = w4quant.pack_codes(torch.tensor([[8, 1] + [0] * 62], dtype=torch.uint8))
    d = w4quant.dequantize_weight(c, torch.tensor([[127, 255]], dtype=torch.uint8))
    assert d[0, 0].item() == 0 and d.view(torch.int16)[0, 0].item() == -32768 and d[0, 1].item() == 0.5 and bool(torch.isnan(d[0, 32:]).all())
    d = w4quant.dequantize_weight(w4quant.pack_codes(torch.full((1, 64), 7, dtype=torch.uint8)), torch.tensor([[0, 1]], dtype=torch.uint8))
    assert d[0, 0].item() == 6 * 2.0 ** -127 and d[0, 32].item() == 6 * 2.0 ** -126


@pytest.mark.parametrize("K", (64, 192, 320))
def test_pack_round_trip_and_order(K):
    codes = torch.arange(5 * K, dtype=torch.int64).remainder(251).remainder(16).to(torch.uint8).view(5, K)
    packed = w4quant.pack_codes(codes)
    assert packed.shape == (5, K // 2) and packed.is_contiguous()
    assert torch.equal(w4quant.unpack_codes(packed), codes)
    any_bytes = torch.arange(5 * K // 2, dtype=torch.int64).remainder(256).to(torch.uint8).view(5, K // 2)
    assert torch.equal(w4quant.pack_codes(w4quant.unpack_codes(any_bytes)), any_bytes)
    for grp in range(K // 64):                                                      # the order the header states
        for q in range(4):
            for s in range(2):
                for j in range(8):
                    byte = packed[:, 32 * grp + 8 * q + 4 * s + j // 2]
                    assert torch.equal((byte >> 4) if j & 1 else (byte & 15), codes[:, 64 * grp + 32 * s + 8 * q + j])


def test_format_argument_checks():
    with pytest.raises(ValueError, match="bf16"):
        w4quant.quantize_weight(torch.zeros(8, 64))
    with pytest.raises(ValueError, match="multiple of 64"):
        w4quant.quantize_weight(torch.zeros(8, 96, dtype=torch.bfloat16))
    with pytest.raises(ValueError, match="multiple of 64"):
        w4quant.pack_codes(torch.zeros(8, 96, dtype=torch.uint8))
    with pytest.raises(ValueError, match="above 15"):
        w4quant.pack_codes(torch.full((8, 64), 16, dtype=torch.uint8))
    with pytest.raises(ValueError, match="uint8"):
        w4quant.unpack_codes(torch.zeros(8, 32, dtype=torch.int8))
    with pytest.raises(ValueError, match="multiple of 64"):
        w4quant.unpack_codes(torch.zeros(8, 48, dtype=torch.uint8))
    with pytest.raises(ValueError, match="scales"):
        w4quant.dequantize_weight(torch.zeros(8, 32, dtype=torch.uint8), torch.zeros(8, 2))
    with pytest.raises(ValueError, match="scales"):
        w4quant.dequantize_weight(torch.zeros(8, 32, dtype=torch.uint8), torch.zeros(8, 4, dtype=torch.uint8))


def test_quantize_weight_chunks_its_rows(monkeypatch):
    w = _weight(N=40)
    whole = w4quant.quantize_weight(w)
    monkeypatch.setattr(w4quant, "ROW_CHUNK", 16)                                    # 16 + 16 + 8 rows
    parts = w4quant.quantize_weight(w)
    assert torch.equal(whole[0], parts[0]) and torch.equal(whole[1], parts[1])
    assert torch.equal(w4quant.dequantize_weight(*whole), w4quant.dequantize_weight(*parts))


# ------------------------------------------------------------------------------------------------------- the model surface
def _cpu_model(block_size=32, n_layer=2):
    from omnibiote_amd.model import OmniBioTA, OmniBioTAConfig
    c = OmniBioTAConfig()
    c.block_size, c.vocab_size, c.n_layer, c.n_head, c.n_embd, c.dropout, c.flash = block_size, 64, n_layer, 2, 128, 0.0, True
    c.autoregressive = True
    m = OmniBioTA(c)
    for p in m.parameters():
        p.data = p.data.to(torch.bfloat16)
    return m


def _fake(pos=8, batch=2, max_len=32, dtype="bf16"):
    """a cache's position state (the host-only class KVCache is built on) with no buffer behind it"""
    from omnibiote_amd.model import CachePositions
    c = CachePositions(batch, max_len)
    c.reset(pos)
    c.layers, c.decode_ws, c.extend_ws, c.dtype = [None, None], None, None, dtype
    return c


def test_quantize_weights_mxfp4_shapes_and_the_dequantised_model():
    from omnibiote_amd.model import QuantizedWeights
    m = _cpu_model()
    wq = m.quantize_weights(format="mxfp4")
    assert isinstance(wq, QuantizedWeights) and wq.format == "mxfp4" and len(wq.codes) == len(wq.scales) == len(wq.dequantized) == 2
    shapes = [(384, 128), (128, 128), (512, 128), (128, 512)]
    for i, block in enumerate(m.transformer.h):
        assert [tuple(c.shape) for c in wq.codes[i]] == [(n, k // 2) for n, k in shapes] and all(c.dtype == torch.uint8 for c in wq.codes[i])
        assert [tuple(s.shape) for s in wq.scales[i]] == [(n, k // 32) for n, k in shapes] and all(s.dtype == torch.uint8 for s in wq.scales[i])
        assert [c.numel() * c.element_size() for c in wq.codes[i]] == [n * k // 2 for n, k in shapes]          # the bytes a step reads
        assert [s.numel() * s.element_size() for s in wq.scales[i]] == [n * k // 32 for n, k in shapes]
        assert [tuple(d.shape) for d in wq.dequantized[i]] == shapes and all(d.dtype == torch.bfloat16 for d in wq.dequantized[i])
        p = wq.block_params(i)
        assert p[0] is block.ln_1.weight and p[3] is block.ln_2.weight and p[1] is wq.dequantized[i][0] and p[5] is wq.dequantized[i][3]
        assert torch.equal(wq.dequantized[i][2], w4quant.dequantize_weight(*w4quant.quantize_weight(block.mlp.c_fc.weight.detach())))
        assert torch.equal(wq.dequantized[i][2], w4quant.dequantize_weight(wq.codes[i][2], wq.scales[i][2]))
    assert wq.head_codes.shape == (64, 64) and wq.head_codes.dtype == torch.uint8 and wq.head_scales.shape == (64, 4) and wq.head_scales.dtype == torch.uint8
    assert wq.head_dequantized.shape == (64, 128) and wq.head_dequantized.dtype == torch.bfloat16
    dm = wq.dequantized_model()
    assert dm is not m and torch.equal(dm.transformer.wte.weight, m.transformer.wte.weight)
    for a, b, d, c, s in zip(dm.transformer.h, m.transformer.h, wq.dequantized, wq.codes, wq.scales):
        assert torch.equal(a.ln_1.weight, b.ln_1.weight) and torch.equal(a.ln_2.weight, b.ln_2.weight)
        for got, i in ((a.attn.c_attn.weight, 0), (a.attn.c_proj.weight, 1), (a.mlp.c_fc.weight, 2), (a.mlp.c_proj.weight, 3)):
            assert torch.equal(got, d[i]) and torch.equal(got, w4quant.dequantize_weight(c[i], s[i]))
        assert not torch.equal(a.mlp.c_fc.weight, b.mlp.c_fc.weight)
    assert torch.equal(dm.lm_head.weight, w4quant.dequantize_weight(wq.head_codes, wq.head_scales))
    again = dm.quantize_weights(format="mxfp4")                                     # the dequantised model is a fixed point: in its values
    assert all(torch.equal(x.view(torch.int16), y.view(torch.int16)) for i in range(2) for x, y in zip(again.dequantized[i], wq.dequantized[i]))
    assert torch.equal(again.head_dequantized.view(torch.int16), wq.head_dequantized.view(torch.int16))
    with pytest.raises(ValueError, match="bfloat16"):
        from omnibiote_amd.model import OmniBioTA
        OmniBioTA(m.config).quantize_weights(format="mxfp4")                        # fp32 parameters


def test_the_format_keyword():
    from omnibiote_amd.model import OmniBioTA, QuantizedWeights
    m = _cpu_model()
    default, named = m.quantize_weights(), m.quantize_weights(format="e4m3")
    assert default.format == named.format == "e4m3" and QuantizedWeights(m).format == "e4m3" and QuantizedWeights(m, format="mxfp4").format == "mxfp4"
    assert default.head_scales.dtype == torch.float32 and default.head_codes.shape == (64, 128)     # e4m3 as it was
    assert torch.equal(default.head_codes, named.head_codes) and torch.equal(default.codes[1][3], named.codes[1][3])
    for bad in ("fp4", "MXFP4", None, 4):
        with pytest.raises(ValueError, match="format"):
            m.quantize_weights(format=bad)
        with pytest.raises(ValueError, match="format"):
            QuantizedWeights(m, bad)
    assert inspect.signature(OmniBioTA.quantize_weights).parameters["format"].default == "e4m3"
    assert inspect.signature(QuantizedWeights.__init__).parameters["format"].default == "e4m3"


def test_a_stale_snapshot_is_refused():
    m = _cpu_model()
    wq = m.quantize_weights(format="mxfp4")
    idx = torch.zeros(2, 4, dtype=torch.int64)
    with pytest.raises(RuntimeError, match="GPU"):                                  # current: on to the first device requirement
        m.generate(idx, 4, weights=wq)
    with torch.no_grad():
        m.transformer.h[1].attn.c_proj.weight.add_(1)
    for call in (lambda: m.generate(idx, 4, weights=wq), lambda: m.prefill(idx, _fake(), weights=wq), lambda: m.decode_step(idx[:, 0], _fake(), weights=wq)):
        with pytest.raises(ValueError, match="quantize_weights again"):
            call()
    wq = m.quantize_weights(format="mxfp4")
    m.lm_head.weight.data = m.lm_head.weight.data.clone()                           # moved
    with pytest.raises(ValueError, match="quantize_weights again"):
        m.decode_step(idx[:, 0], _fake(), weights=wq)
    with pytest.raises(ValueError, match="another model"):
        _cpu_model().generate(idx, 4, weights=wq)


def test_what_refuses_weights_refuses_mxfp4_with_nothing_changed():
    from omnibiote_amd.model import DecodeLoop, SharedPrefixCache
    m = _cpu_model()
    wq = m.quantize_weights(format="mxfp4")
    idx = torch.zeros(2, 4, dtype=torch.int64)
    c = _fake()
    with pytest.raises(NotImplementedError, match=r"OmniBioTA\.generate: weights="):
        m.generate(idx, 4, num_samples=2, weights=wq)
    with pytest.raises(NotImplementedError, match=r"OmniBioTA\.extend: weights="):
        m.extend(idx, c, weights=wq)
    with pytest.raises(NotImplementedError, match=r"OmniBioTA\.generate_speculative: weights="):
        m.generate_speculative(idx, 4, m, weights=wq)
    with pytest.raises(NotImplementedError, match=r"OmniBioTA\.generate_speculative: weights="):
        m.generate_speculative(idx, 4, m, draft_weights=wq)
    with pytest.raises(NotImplementedError, match=r"OmniBioTA\.draft_and_verify: weights="):
        m.draft_and_verify(m, idx[:, 0], c, _fake(), 2, weights=wq)
    shared = SharedPrefixCache.__new__(SharedPrefixCache)                           # (no buffer: the refusal comes first)
    for call, name in ((lambda: m.prefill(idx, shared, weights=wq), "prefill"), (lambda: m.decode_step(idx[:, 0], shared, weights=wq), "decode_step"),
                       (lambda: DecodeLoop(m, shared, max_steps=4, weights=wq), "DecodeLoop")):
        with pytest.raises(NotImplementedError, match=rf"OmniBioTA\.{name}: weights="):
            call()
    assert c.pos == 8 and c.positions is None


def test_valid_calls_on_a_cpu_model_reach_the_device_requirement():
    m = _cpu_model()
    wq = m.quantize_weights(format="mxfp4")
    idx = torch.zeros(2, 4, dtype=torch.int64)
    for kw in (dict(), dict(lengths=[4, 2]), dict(kv_dtype="fp8"), dict(sampler="device", loop="graph"), dict(allowed_tokens=[1, 2, 3], eos_token=3, min_new_tokens=2)):
        with pytest.raises(RuntimeError, match="GPU"):
            m.generate(idx, 4, weights=wq, **kw)
    with pytest.raises(RuntimeError, match="GPU"):
        m.prefill(idx, _fake(), weights=wq)
    with pytest.raises(RuntimeError, match="GPU"):
        m.decode_step(idx[:, 0], _fake(), weights=wq)
    from omnibiote_amd import ops
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.linear_small_m_w4(torch.zeros(2, 128, dtype=torch.bfloat16), wq.head_codes, wq.head_scales)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.block_step_w4(torch.zeros(2, 128, dtype=torch.bfloat16), wq.block_params(0), (wq.codes[0], wq.scales[0]), (None, None), 2, None, 32, 8)
    with pytest.raises(ValueError, match="four"):
        ops.block_step_w4(torch.zeros(2, 128, dtype=torch.bfloat16), wq.block_params(0), (wq.codes[0][:3], wq.scales[0]), (None, None), 2, None, 32, 8)
