"""Host-side tests (no GPU) of the e4m3 decode-step weights (include/omnibiote_hip_w8.h): the symbol table against the header, the pins of
the ABI, the format's yardstick (omnibiote_amd/w8quant.py), every argument check that returns before a launch, and the model surface —
quantize_weights, the stale snapshot, what refuses weights= — on a CPU model."""
import ctypes as C
import inspect
import os
import re

import pytest
import torch

from omnibiote_amd import _lib, kvquant, w8quant

EINVAL, EUNSUPPORTED = -1, -3
P = 4096   # a non-null, 16-byte aligned "pointer" for calls that must return before they touch it
NAMES = ("obte_linear_small_m_w8", "obte_block_step_w8")


def _err():
    return _lib.lib().obte_last_error().decode()


def test_symbols_are_what_the_header_declares():
    assert tuple(_lib.SYMBOLS_W8) == NAMES
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "omnibiote_hip_w8.h")).read()
    body = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    assert tuple(re.findall(r"\b(obte_\w+)\s*\(", body)) == NAMES                  # the declarations, in order
    assert '#include "omnibiote_hip.h"' in header and "struct" not in body
    lib = _lib.lib()
    others = (_lib.SYMBOLS, _lib.SYMBOLS_ROWS, _lib.SYMBOLS_SMALL_M, _lib.SYMBOLS_SAMPLE, _lib.SYMBOLS_EXTEND, _lib.SYMBOLS_SPEC, _lib.SYMBOLS_KV8,
              _lib.SYMBOLS_SHARED, _lib.SYMBOLS_LOOP, _lib.SYMBOLS_CONSTRAIN)
    for name in NAMES:
        for table in others:
            assert name not in table
        res, args = _lib.SYMBOLS_W8[name]
        fn = getattr(lib, name)
        assert fn.restype is res and list(fn.argtypes) == args                      # bound by lib(), in the same loop
    assert [len(t) for t in others] == [70, 3, 3, 1, 6, 2, 6, 5, 1, 2]              # the ten tables as they were
    assert lib.obte_abi_version() == 1
    sizes = (C.c_int64 * 16)()
    assert lib.obte_struct_sizes(sizes, 16) == 6
    makefile = open(os.path.join(root, "omnibiote_amd", "csrc", "Makefile")).read()
    assert "omnibiote_hip_w8.h" in makefile


# ------------------------------------------------------------------------------------------------------- the product's checks
def _gemm(M=2, N=16, K=64, epi=0, alpha=1.0, a=P, d=P, aux=None, lda=None, ldd=None, **more):
    return _lib.GemmArgs(a=a, b=None, d=d, aux=aux, M=M, N=N, K=K, lda=K if lda is None else lda, ldb=0, ldd=N if ldd is None else ldd, a_kmajor=1,
                         b_kmajor=1, epilogue=epi, alpha=alpha, **more)


def _product(g, codes=P, ld=None, scales=P):
    return _lib.lib().obte_linear_small_m_w8(C.byref(g) if g is not None else None, codes, g.K if ld is None and g is not None else (ld or 0), scales, None)


@pytest.mark.parametrize("g,kw,rc,word", [
    (None, {}, EINVAL, "null"), (dict(a=None), {}, EINVAL, "null"), (dict(d=None), {}, EINVAL, "null"),
    ({}, dict(codes=None), EINVAL, "null"), ({}, dict(scales=None), EINVAL, "null"),
    (dict(M=0), {}, EINVAL, "M must be"), (dict(M=65), {}, EINVAL, "M must be"), (dict(K=96), {}, EINVAL, "K"), (dict(N=12), {}, EINVAL, "multiples of 8"),
    (dict(lda=56), {}, EINVAL, "leading dimension"), (dict(ldd=8), {}, EINVAL, "leading dimension"),
    ({}, dict(ld=72), EINVAL, "ld_codes"), ({}, dict(ld=48), EINVAL, "ld_codes"), ({}, dict(codes=P + 8), EINVAL, "aligned"), ({}, dict(scales=P + 2), EINVAL, "aligned"),
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
    assert _err().startswith("obte_linear_small_m_w8:") and word in _err(), _err()


def test_product_ignores_b_and_ldb():
    """g->b null and ldb 0 pass the checks: the call is refused for something else"""
    assert _product(_gemm(M=65)) == EINVAL and "M must be" in _err()


def _desc(B=2, T=1, C_=256, H=2, **over):
    f = dict(B=B, T=T, n_embd=C_, n_head=H, ln1_w=P, attn_w=P, proj_w=P, ln2_w=P, fc_w=P, mlp_w=P, rope_cos=P, rope_sin=P)
    f.update(over)
    return _lib.BlockDesc(**f)


def test_block_step_w8_rejects_before_any_launch():
    lib = _lib.lib()
    big = 1 << 30
    four = (C.c_void_p * 4)(P, P, P, P)

    def step(d, codes=four, scales=four, x=P, y=P, kv=P, e4m3=0, T_max=100, pos=5, pos_rows=None, ws=P, ws_bytes=big):
        return lib.obte_block_step_w8(C.byref(d) if d is not None else None, codes, scales, x, y, kv, e4m3, T_max, pos, pos_rows, ws, ws_bytes, None)
    assert step(None) == EINVAL and "obte_block_step_w8" in _err() and "null" in _err()
    assert step(_desc(), codes=None) == EINVAL and _err().startswith("obte_block_step_w8:") and "null" in _err()
    assert step(_desc(), scales=None) == EINVAL and "null" in _err()
    assert step(_desc(), codes=(C.c_void_p * 4)(P, P, None, P)) == EINVAL and "codes[2]" in _err()
    assert step(_desc(), codes=(C.c_void_p * 4)(P, P + 8, P, P)) == EINVAL and "aligned" in _err()
    assert step(_desc(), scales=(C.c_void_p * 4)(P, P, P, P + 2)) == EINVAL and "aligned" in _err()
    for over in (dict(key_ranges=P), dict(out_rows=P, n_out_rows=1), dict(dropout_p=0.1), dict(mask=P), dict(query_bounds=P)):
        assert step(_desc(**over)) == EUNSUPPORTED, over
        assert _err().startswith("obte_block_step_w8:"), _err()
    for kw in (dict(x=None), dict(y=None), dict(kv=None), dict(ws=None)):
        assert step(_desc(), **kw) == EINVAL and _err().startswith("obte_block_step_w8:") and "null" in _err(), (kw, _err())
    assert step(_desc(T=2)) == EINVAL and "T = 1" in _err()
    for rows in (None, P):
        for e4m3 in (0, 1):
            assert step(_desc(), pos=100, pos_rows=rows, e4m3=e4m3) == EINVAL and "outside the cache" in _err(), _err()
            assert step(_desc(), pos=-1, pos_rows=rows, e4m3=e4m3) == EINVAL and "outside the cache" in _err(), _err()
    assert step(_desc(), kv=P + 8, e4m3=1) == EINVAL and "aligned" in _err()
    assert step(_desc(), ws_bytes=lib.obte_block_decode_ws_bytes(2, 256, 2) - 1) == EINVAL
    assert _err().startswith("obte_block_step_w8:") and "workspace" in _err(), _err()
    assert step(_desc(C_=128, H=4)) == EINVAL and "head" in _err()                # head size 32


# ------------------------------------------------------------------------------------------------------- the format's yardstick
def _weight(N=40, K=192, seed=5):
    g = torch.Generator().manual_seed(seed)
    w = (torch.randn(N, K, generator=g) * 0.02).bfloat16()
    w[3] = 0
    return w


def test_format_properties():
    w = _weight()
    codes, scales = w8quant.quantize_weight(w)
    assert codes.dtype == torch.uint8 and codes.shape == w.shape and scales.dtype == torch.float32 and scales.shape == (w.shape[0],)
    m, e = torch.frexp(scales.double())
    assert bool((m == 0.5).all()) and int((e - 1).min()) >= -126                    # powers of two
    assert not bool(((codes & 0x7F) == 0x7F).any())                                 # never a NaN code
    values = codes.view(torch.float8_e4m3fn).float()
    assert float(values.abs().max()) <= 448 and float(values.abs().amax(1)[4]) > 224
    assert int(codes[3].max()) == 0 and float(scales[3]) == 2.0 ** -126             # the zero row
    plain, plain_scales = kvquant.quantize_reference(w)                             # row n is one vector of the cache's rule
    assert torch.equal(w8quant.unpack_codes(codes), plain) and torch.equal(scales, plain_scales)
    deq = w8quant.dequantize_weight(codes, scales)
    assert deq.dtype == torch.bfloat16 and deq.shape == w.shape
    exact = w8quant.unpack_codes(codes).view(torch.float8_e4m3fn).double() * scales.double().unsqueeze(1)
    assert torch.equal(deq.double(), exact)                                         # bf16-exact
    amax = w.double().abs().amax(1, keepdim=True)
    assert bool(((deq.double() - w.double()).abs() <= amax / 14).all())
    worst = ((deq.double() - w.double()).abs() / amax.clamp_min(1e-300)).max()
    assert float(worst) <= 16 / 224


def test_codes_do_not_depend_on_the_rows_magnitude():
    w = _weight()
    codes, scales = w8quant.quantize_weight(w)
    for j in (-20, 10):
        c2, s2 = w8quant.quantize_weight((w.float() * 2.0 ** j).bfloat16())        # a power of two: exact in bf16
        assert torch.equal(c2, codes)
        live = torch.arange(w.shape[0]) != 3                                        # (the zero row stays at the floor scale)
        assert torch.equal(s2[live], scales[live] * 2.0 ** j) and float(s2[3]) == 2.0 ** -126


@pytest.mark.parametrize("K", (64, 192, 320))
def test_pack_round_trip_and_order(K):
    codes = torch.arange(5 * K, dtype=torch.int64).remainder(251).to(torch.uint8).view(5, K)
    packed = w8quant.pack_codes(codes)
    assert packed.shape == codes.shape and packed.is_contiguous()
    assert torch.equal(w8quant.unpack_codes(packed), codes) and torch.equal(w8quant.pack_codes(w8quant.unpack_codes(codes)), codes)
    for grp in range(K // 64):                                                      # the order the header states
        for q in range(4):
            for s in range(2):
                assert torch.equal(packed[:, 64 * grp + 16 * q + 8 * s:64 * grp + 16 * q + 8 * s + 8], codes[:, 64 * grp + 32 * s + 8 * q:64 * grp + 32 * s + 8 * q + 8])
    assert sorted(packed[0].tolist()) == sorted(codes[0].tolist())


def test_format_argument_checks():
    with pytest.raises(ValueError, match="bf16"):
        w8quant.quantize_weight(torch.zeros(8, 64))
    with pytest.raises(ValueError, match="multiple of 64"):
        w8quant.quantize_weight(torch.zeros(8, 96, dtype=torch.bfloat16))
    with pytest.raises(ValueError, match="multiple of 64"):
        w8quant.pack_codes(torch.zeros(8, 96, dtype=torch.uint8))
    with pytest.raises(ValueError, match="uint8"):
        w8quant.unpack_codes(torch.zeros(8, 64, dtype=torch.int8))
    with pytest.raises(ValueError, match="scales"):
        w8quant.dequantize_weight(torch.zeros(8, 64, dtype=torch.uint8), torch.zeros(7))


def test_quantize_weight_chunks_its_rows(monkeypatch):
    w = _weight(N=40)
    whole = w8quant.quantize_weight(w)
    monkeypatch.setattr(w8quant, "ROW_CHUNK", 16)                                    # 16 + 16 + 8 rows
    parts = w8quant.quantize_weight(w)
    assert torch.equal(whole[0], parts[0]) and torch.equal(whole[1], parts[1])
    assert torch.equal(w8quant.dequantize_weight(*whole), w8quant.dequantize_weight(*parts))


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


def test_quantize_weights_shapes_and_the_dequantised_model():
    from omnibiote_amd.model import QuantizedWeights
    m = _cpu_model()
    wq = m.quantize_weights()
    assert isinstance(wq, QuantizedWeights) and len(wq.codes) == len(wq.scales) == len(wq.dequantized) == 2
    shapes = [(384, 128), (128, 128), (512, 128), (128, 512)]
    for i, block in enumerate(m.transformer.h):
        assert [tuple(c.shape) for c in wq.codes[i]] == shapes and all(c.dtype == torch.uint8 for c in wq.codes[i])
        assert [tuple(s.shape) for s in wq.scales[i]] == [(n,) for n, _ in shapes] and all(s.dtype == torch.float32 for s in wq.scales[i])
        assert [tuple(d.shape) for d in wq.dequantized[i]] == shapes and all(d.dtype == torch.bfloat16 for d in wq.dequantized[i])
        p = wq.block_params(i)
        assert p[0] is block.ln_1.weight and p[3] is block.ln_2.weight and p[1] is wq.dequantized[i][0] and p[5] is wq.dequantized[i][3]
        assert torch.equal(wq.dequantized[i][2], w8quant.dequantize_weight(*w8quant.quantize_weight(block.mlp.c_fc.weight.detach())))
    assert wq.head_codes.shape == (64, 128) and wq.head_codes.dtype == torch.uint8 and wq.head_scales.shape == (64,)
    assert wq.head_dequantized.shape == (64, 128) and wq.head_dequantized.dtype == torch.bfloat16
    dm = wq.dequantized_model()
    assert dm is not m and torch.equal(dm.transformer.wte.weight, m.transformer.wte.weight)
    assert dm.transformer.wte.weight.data_ptr() != m.transformer.wte.weight.data_ptr()
    for a, b, d in zip(dm.transformer.h, m.transformer.h, wq.dequantized):
        assert torch.equal(a.ln_1.weight, b.ln_1.weight) and torch.equal(a.ln_2.weight, b.ln_2.weight)
        assert torch.equal(a.attn.c_attn.weight, d[0]) and torch.equal(a.mlp.c_proj.weight, d[3])
        assert not torch.equal(a.mlp.c_fc.weight, b.mlp.c_fc.weight)
    assert torch.equal(dm.transformer.ln_f.weight, m.transformer.ln_f.weight) and torch.equal(dm.lm_head.weight, wq.head_dequantized)
    again = dm.quantize_weights()                                                   # the dequantised model is a fixed point
    assert all(torch.equal(x, y) for i in range(2) for x, y in zip(again.codes[i] + again.scales[i], wq.codes[i] + wq.scales[i]))
    with pytest.raises(ValueError, match="bfloat16"):
        from omnibiote_amd.model import OmniBioTA
        OmniBioTA(m.config).quantize_weights()                                      # fp32 parameters


def test_a_stale_snapshot_is_refused():
    m = _cpu_model()
    wq = m.quantize_weights()
    idx = torch.zeros(2, 4, dtype=torch.int64)
    with pytest.raises(RuntimeError, match="GPU"):                                  # current: on to the first device requirement
        m.generate(idx, 4, weights=wq)
    with torch.no_grad():
        m.transformer.h[1].attn.c_proj.weight.add_(1)
    for call in (lambda: m.generate(idx, 4, weights=wq), lambda: m.prefill(idx, _fake(), weights=wq), lambda: m.decode_step(idx[:, 0], _fake(), weights=wq)):
        with pytest.raises(ValueError, match="quantize_weights again"):
            call()
    wq = m.quantize_weights()
    m.lm_head.weight.data = m.lm_head.weight.data.clone()                           # moved
    with pytest.raises(ValueError, match="quantize_weights again"):
        m.decode_step(idx[:, 0], _fake(), weights=wq)
    with pytest.raises(ValueError, match="another model"):
        _cpu_model().generate(idx, 4, weights=wq)
    with pytest.raises(ValueError, match="quantize_weights"):
        m.generate(idx, 4, weights=object())


def test_what_refuses_weights_does_so_before_anything_else():
    from omnibiote_amd.model import DecodeLoop, SharedPrefixCache
    m = _cpu_model()
    wq = m.quantize_weights()
    idx = torch.zeros(2, 4, dtype=torch.int64)
    c = _fake()
    with pytest.raises(NotImplementedError, match=r"OmniBioTA\.generate: weights="):
        m.generate(idx, 4, num_samples=2, weights=wq)
    with pytest.raises(NotImplementedError, match=r"OmniBioTA\.extend: weights="):
        m.extend(idx, c, weights=wq)
    with pytest.raises(NotImplementedError, match=r"OmniBioTA\.extend: weights="):
        m.extend(idx[:, :1], c, weights=wq)
    with pytest.raises(NotImplementedError, match=r"OmniBioTA\.generate_speculative: weights="):
        m.generate_speculative(idx, 4, m, weights=wq)
    with pytest.raises(NotImplementedError, match=r"OmniBioTA\.generate_speculative: weights="):
        m.generate_speculative(idx, 4, m, draft_weights=wq)
    with pytest.raises(NotImplementedError, match=r"OmniBioTA\.draft_and_verify: weights="):
        m.draft_and_verify(m, idx[:, 0], c, _fake(), 2, weights=wq)
    with pytest.raises(NotImplementedError, match=r"OmniBioTA\.draft_and_verify: weights="):
        m.draft_and_verify(m, idx[:, 0], c, _fake(), 2, draft_weights=wq)
    shared = SharedPrefixCache.__new__(SharedPrefixCache)                           # (no buffer: the refusal comes first)
    for call, name in ((lambda: m.prefill(idx, shared, weights=wq), "prefill"), (lambda: m.decode_step(idx[:, 0], shared, weights=wq), "decode_step"),
                       (lambda: DecodeLoop(m, shared, max_steps=4, weights=wq), "DecodeLoop")):
        with pytest.raises(NotImplementedError, match=rf"OmniBioTA\.{name}: weights="):
            call()
    assert c.pos == 8 and c.positions is None


def test_valid_calls_on_a_cpu_model_reach_the_device_requirement():
    m = _cpu_model()
    wq = m.quantize_weights()
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
        ops.linear_small_m_w8(torch.zeros(2, 128, dtype=torch.bfloat16), wq.head_codes, wq.head_scales)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.block_step_w8(torch.zeros(2, 128, dtype=torch.bfloat16), wq.block_params(0), (wq.codes[0], wq.scales[0]), (None, None), 2, None, 32, 8)
    with pytest.raises(ValueError, match="four"):
        ops.block_step_w8(torch.zeros(2, 128, dtype=torch.bfloat16), wq.block_params(0), (wq.codes[0][:3], wq.scales[0]), (None, None), 2, None, 32, 8)


def test_signatures():
    from omnibiote_amd.model import DecodeLoop, OmniBioTA
    sig = list(inspect.signature(DecodeLoop.__init__).parameters.values())
    assert [p.name for p in sig[-3:]] == ["weights", "allowed", "hold_min"] and all(p.kind is p.KEYWORD_ONLY and p.default in (None, 0) for p in sig[-3:])
    gen = list(inspect.signature(OmniBioTA.generate).parameters)
    assert gen[-1] == "weights" and gen[1:4] == ["idx", "max_new_tokens", "temperature"] and gen[-3:-1] == ["allowed_tokens", "min_new_tokens"]
    for f in (OmniBioTA.prefill, OmniBioTA.decode_step, OmniBioTA.generate, OmniBioTA._step_blocks):   # (generate carries it for ragged prompts too)
        assert inspect.signature(f).parameters["weights"].default is None
