"""The decode step's products and readout on MXFP4 weights (include/omnibiote_hip_w4.h, csrc/gemm_small_m.hip's WMxfp4 policy) on the GPU.
The contract is equality of BITS with the bf16 path on the dequantised weights (w4quant.dequantize_weight): the conversion alone against
the dequantised weight itself, the product against ops.linear_small_m at every epilogue, the block step against ops.block_decode /
block_decode_rows / block_decode_kv8, the model against QuantizedWeights.dequantized_model().  No test compares against the unquantised
model with a bar (DESIGN.md 14.20 records that deviation)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import fenced as F
import omnibiote_ref as R
from test_hip_causal import _model
from test_hip_ops import BF, DEV, rnd
from test_hip_small_m import Profile

pytestmark = pytest.mark.gpu

MS = (1, 2, 7, 16, 17, 33, 64)
EINVAL, EUNSUPPORTED = -1, -3
# test_hip_w8.py's shapes, the smallest that reach every branch: (24, 64): N % 16 == 8 and three waves without a chunk; (200, 320): the unrolled
# chunk loop's tail; N > 8192 at K = 256 / 512 / 1024: the x-stationary kernel at every chunk count, the last strip a half one; (8200, 768): as
# many strips on the one-strip kernel
SHAPES = [(24, 64), (136, 192), (384, 128), (200, 320), (1024, 4096), (8200, 256), (8216, 512), (8208, 1024), (8200, 768)]


def ops():
    from omnibiote_amd import ops as o
    return o


def L():
    from omnibiote_amd import _lib
    return _lib


def Q():
    from omnibiote_amd import w4quant
    return w4quant


def _bits(t):
    return t.contiguous().view(torch.int16)


@functools.lru_cache(maxsize=None)
def _case(N, K):
    """x [64, K], aux [64, N], W [N, K] ~ N(0, 0.02) with a zero row, a row x 2^-20, a row x 2^10 and a row whose blocks differ by 2^12 from
    one to the next, quantised; the dequantised weight (computed once, never modified)"""
    x, aux = rnd(64, K, seed=N + K), rnd(64, N, seed=N + K + 2)
    w = rnd(N, K, seed=N + K + 1, scale=0.02)
    w[1] = 0
    w[N // 2] = (w[N // 2].float() * 2.0 ** -20).to(BF)
    w[N - 1] = (w[N - 1].float() * 2.0 ** 10).to(BF)
    step = torch.exp2(12.0 * (torch.arange(K // 32) % 2) - 6).repeat_interleave(32)
    w[2] = (w[2].float() * step).to(BF)
    codes, scales = Q().quantize_weight(w.to(DEV))
    return dict(x=x.to(DEV), aux=aux.to(DEV), codes=codes, scales=scales, deq=Q().dequantize_weight(codes, scales))


# =================================================================================================== the conversion alone
def test_w4_conversion_alone():
    """Through no other kernel: W (32, 256) built by hand — the code of (n, k) is (n + k) % 16, so all 16 nibbles stand at every nibble
    position of every chunk, and the scale bytes sweep 2 .. 253 over rows and blocks — against 64 one-hot rows of x, row m selecting
    k = 4 m + r: both k-steps, all four lane groups and all four chunks in each of the four rounds r, every k of the row once.  Then
    d[m, n] is dequantize_weight(...)[n, k_m], bit for bit.  Two things follow from the sum the selected value passes through: every other
    term is 0 * W, so under the scale byte 253 the codes of 4 and 6, whose values are +-inf (w4quant's corner), are replaced by the codes
    of 2 and 3 (0 * inf is NaN); and a sum that starts at +0 gives +0 for a selected -0 (+0 + -0 = +0), so the expected bits are those
    of W + 0.0 — the code 0x8 must still come out as a zero."""
    o, q = ops(), Q()
    N, K = 32, 256
    n, k = torch.arange(N).unsqueeze(1), torch.arange(K).unsqueeze(0)
    scales = (2 + (n * (K // 32) + torch.arange(K // 32).unsqueeze(0)) % 252).to(torch.uint8)
    assert set(scales.flatten().tolist()) == set(range(2, 254))
    codes = ((n + k) % 16).to(torch.uint8)
    top = (scales == 253).repeat_interleave(32, dim=1) & ((codes & 7) >= 6)
    codes = torch.where(top, codes - 2, codes)
    for pos in range(64):                                                           # every nibble at every nibble position of a chunk
        assert set(codes[:, pos::64].flatten().tolist()) == set(range(16)), pos
    packed = q.pack_codes(codes).to(DEV)
    deq = q.dequantize_weight(packed, scales.to(DEV))
    assert torch.isfinite(deq).all() and int((_bits(deq) == -32768).sum()) > 0      # -0 is among the weights
    want_all = (deq.float() + 0.0).to(BF)
    seen = torch.zeros(K, dtype=torch.int64)
    for r in range(4):
        km = 4 * torch.arange(64) + r
        seen[km] += 1
        x = torch.zeros(64, K, dtype=BF)
        x[torch.arange(64), km] = 1
        got = o.linear_small_m_w4(x.to(DEV), packed, scales.to(DEV))
        want = want_all[:, km.to(DEV)].t()
        bad = _bits(got) != _bits(want)
        assert not bad.any(), (r, int(bad.sum()), [tuple(int(v) for v in i) for i in bad.nonzero()[:4]], got[bad][:4], want[bad][:4])
    assert (seen == 1).all()


# =================================================================================================== the product, bit for bit
@pytest.mark.parametrize("N,K", SHAPES)
def test_w4_product_has_the_bits_of_the_bf16_product_on_the_dequantised_weight(N, K):
    o, Lm, c = ops(), L(), _case(N, K)
    assert bool((c["scales"][1] == 2).all()) and int(c["codes"][1].max()) == 0           # the zero row: e = -125
    for M in MS:
        x, aux = c["x"][:M].contiguous(), c["aux"][:M].contiguous()
        for alpha in (1.0, 0.37):
            want = o.linear_small_m(x, c["deq"], alpha=alpha)
            got = o.linear_small_m_w4(x, c["codes"], c["scales"], alpha=alpha)
            assert got.shape == (M, N) and torch.equal(_bits(got), _bits(want)), ("NONE", M, N, K, alpha)
            want = o.linear_small_m(x, c["deq"], epilogue=Lm.EPI_ADD, aux=aux, alpha=alpha)
            out = aux.clone()                                                               # aux aliased to out
            assert o.linear_small_m_w4(x, c["codes"], c["scales"], epilogue=Lm.EPI_ADD, aux=out, alpha=alpha, out=out) is out
            assert torch.equal(_bits(out), _bits(want)), ("ADD", M, N, K, alpha)
        want = o.linear_small_m(x, c["deq"], epilogue=Lm.EPI_GELU_ACT)
        got = o.linear_small_m_w4(x, c["codes"], c["scales"], epilogue=Lm.EPI_GELU_ACT)
        assert torch.equal(_bits(got), _bits(want)), ("GELU_ACT", M, N, K)
    assert torch.isfinite(want).all() and float(want.float().abs().max()) > 0


@pytest.mark.parametrize("hs,H,K", [(64, 2, 128), (128, 2, 256), (128, 22, 256)])
def test_w4_rope_epilogue(hs, H, K):
    """c_attn's epilogue (N = 3 H hs): rope_T = 1 at table row 5 at every M, rope_T = 4 at M = 7; 22 heads: the x-stationary kernel's"""
    o, Lm = ops(), L()
    N = 3 * H * hs
    c = _case(N, K)
    g = torch.Generator().manual_seed(hs)
    cos, sin = [torch.rand(9, hs // 2, generator=g).mul(2).sub(1).to(DEV) for _ in range(2)]
    for M, T, row in [(M, 1, 5) for M in MS] + [(7, 4, 0), (7, 4, 3)]:
        x = c["x"][:M].contiguous()
        rope = (cos[row:], sin[row:], T, hs)
        want = o.linear_small_m(x, c["deq"], epilogue=Lm.EPI_ROPE_QK, rope=rope)
        got = o.linear_small_m_w4(x, c["codes"], c["scales"], epilogue=Lm.EPI_ROPE_QK, rope=rope)
        assert torch.equal(_bits(got), _bits(want)), (hs, H, M, T, row)
        assert not torch.equal(_bits(got), _bits(o.linear_small_m_w4(x, c["codes"], c["scales"])))       # it did rotate


@pytest.mark.parametrize("N,K", [(136, 192), (8200, 256)])
def test_w4_leading_dimensions(N, K):
    """ldd > N, ld_codes > K / 2 and ld_scales > K / 32: codes and scales as row-strided views whose padding is 0xFF (the codes of -6 under
    the NaN scale), d inside a marked buffer"""
    o, c = ops(), _case(N, K)
    wide = torch.full((N, K // 2 + 24), 0xFF, dtype=torch.uint8, device=DEV)
    wide[:, :K // 2] = c["codes"]
    swide = torch.full((N, K // 32 + 6), 0xFF, dtype=torch.uint8, device=DEV)
    swide[:, :K // 32] = c["scales"]
    for M in (1, 17, 64):
        want = o.linear_small_m(c["x"][:M], c["deq"])
        buf = torch.full((M + 3, N + 8), 0x1234, dtype=torch.int16, device=DEV)
        got = o.linear_small_m_w4(c["x"][:M], wide[:, :K // 2], swide[:, :K // 32], out=buf.view(BF)[:M, :N])
        assert torch.equal(_bits(got), _bits(want)), (M, N, K)
        assert (buf[M:] == 0x1234).all() and (buf[:M, N:] == 0x1234).all()


@pytest.mark.parametrize("N,K", [(24, 64), (200, 320), (1024, 4096), (8216, 512)])
def test_w4_exact_integer_products(N, K):
    """ternary x, weights from {0, +-1, +-2} * 2^e with one e per row, every one an e2m1 value under its block's scale (a block's scale
    follows its own maximum; an all-zero block has none to follow): the quantisation is exact and the result is bf16(the int64 product
    * 2^e), bit for bit"""
    o = ops()
    g = torch.Generator().manual_seed(N + K)
    x = torch.randint(-1, 2, (64, K), generator=g)
    wi = torch.randint(-2, 3, (N, K), generator=g)
    e = torch.randint(-6, 7, (N,), generator=g)
    w = (wi.double() * torch.exp2(e.double()).unsqueeze(1)).to(BF)
    codes, scales = Q().quantize_weight(w.to(DEV))
    assert torch.equal(Q().dequantize_weight(codes, scales).cpu(), w)
    acc = (x @ wi.t()).double() * torch.exp2(e.double())
    for M in MS:
        got = o.linear_small_m_w4(x[:M].to(BF).to(DEV), codes, scales)
        assert torch.equal(got.cpu(), acc[:M].to(BF)), (M, N, K)


@pytest.mark.parametrize("N,K", [(1024, 4096), (384, 128), (8216, 512)])
def test_w4_rows_are_independent_and_calls_repeat(N, K):
    o, c = ops(), _case(N, K)
    full = o.linear_small_m_w4(c["x"], c["codes"], c["scales"])
    assert torch.equal(_bits(full), _bits(o.linear_small_m_w4(c["x"], c["codes"], c["scales"])))
    for m in (0, 15, 16, 63):
        one = o.linear_small_m_w4(c["x"][m:m + 1], c["codes"], c["scales"])
        assert torch.equal(_bits(one[0]), _bits(full[m])), (N, K, m)
    for M in (2, 7, 17, 33):
        assert torch.equal(_bits(o.linear_small_m_w4(c["x"][:M], c["codes"], c["scales"])), _bits(full[:M])), (N, K, M)


@pytest.mark.parametrize("N,K", [(136, 192), (8200, 256)])
@pytest.mark.parametrize("M", (1, 17, 64))
def test_w4_fenced(M, N, K):
    """x, codes, scales, aux and d in poisoned buffers aligned as far as the call asks and no further (x, aux, d: 16 bytes; codes: 8;
    scales: 2): guards intact, the unfenced bits.  The poison of codes and scales is 0xFF: two codes of -6, the NaN scale."""
    o, Lm, c = ops(), L(), _case(N, K)
    want = o.linear_small_m_w4(c["x"][:M], c["codes"], c["scales"], epilogue=Lm.EPI_ADD, aux=c["aux"][:M].contiguous())
    x, hx = F.fenced(c["x"][:M], poison="nan")
    c8, hc = F.fenced(torch.cat([torch.full((8,), 0xFF, dtype=torch.uint8, device=DEV), c["codes"].flatten()]), poison=0xFF)
    codes = c8[8:].view(N, K // 2)
    s14, hs_ = F.fenced(torch.cat([torch.full((14,), 0xFF, dtype=torch.uint8, device=DEV), c["scales"].flatten()]), poison=0xFF)
    scales = s14[14:].view(N, K // 32)
    assert codes.data_ptr() % 16 == 8 and scales.data_ptr() % 16 == 14
    aux, ha = F.fenced(c["aux"][:M], poison="nan")
    d, hd = F.fenced((M, N), BF, poison="mark")
    got = o.linear_small_m_w4(x, codes, scales, epilogue=Lm.EPI_ADD, aux=aux, out=d)
    torch.cuda.synchronize()
    F.assert_guards(hx, hc, hs_, ha, hd)
    assert bool((c8[:8] == 0xFF).all()) and bool((s14[:14] == 0xFF).all())
    F.assert_same_bits(got, want, f"fenced w4 product {M}x{N}x{K}")
    plain, hp = F.fenced((M, N), BF, poison="mark")
    F.assert_same_bits(o.linear_small_m_w4(x, codes, scales, out=plain), o.linear_small_m_w4(c["x"][:M], c["codes"], c["scales"]), "EPI_NONE")
    F.assert_guards(hp)


def test_w4_refusals_name_the_call():
    lib, Lm = L().lib(), L()
    x, codes, scales, d = (torch.zeros(4096, dtype=torch.uint8, device=DEV) for _ in range(4))
    scales.fill_(127)

    def call(M=2, N=16, K=64, epi=0, codes_at=0, scales_at=0, ld=None, lds=None, alpha=1.0):
        g = Lm.GemmArgs(x.data_ptr(), None, d.data_ptr(), None, None, M, N, K, K, K, N, 1, 1, epi, alpha, 0.0, 0, 0)
        return lib.obte_linear_small_m_w4(C.byref(g), codes.data_ptr() + codes_at, K // 2 if ld is None else ld, scales.data_ptr() + scales_at,
                                          K // 32 if lds is None else lds, None)

    for kw, rc, word in [(dict(K=96), EINVAL, "K"), (dict(M=65), EINVAL, "M must be"), (dict(codes_at=4), EINVAL, "aligned"), (dict(scales_at=1), EINVAL, "aligned"),
                         (dict(epi=1), EUNSUPPORTED, "epilogue"), (dict(ld=36), EINVAL, "ld_codes"), (dict(ld=24), EINVAL, "ld_codes"), (dict(lds=3), EINVAL, "ld_scales"),
                         (dict(K=128, lds=2), EINVAL, "ld_scales"), (dict(epi=9, alpha=0.5), EINVAL, "alpha")]:
        assert call(**kw) == rc, kw
        err = lib.obte_last_error().decode()
        assert err.startswith("obte_linear_small_m_w4:") and word in err, (kw, err)
    assert call() == 0
    torch.cuda.synchronize()


# =================================================================================================== the block step
NAMES = ["ln_1.weight", "attn.c_attn.weight", "attn.c_proj.weight", "ln_2.weight", "mlp.c_fc.weight", "mlp.c_proj.weight"]


@functools.lru_cache(maxsize=None)
def _block_case(Cc, H):
    """one block's hash weights quantised: the dequantised parameters, the (codes, scales) pair, tables and inputs for 5 rows"""
    from omnibiote_amd.model import rope_tables
    T = 48
    cfg = R.RefConfig(block_size=T, vocab_size=256, n_layer=1, n_head=H, n_embd=Cc)
    w = {k: v.to(BF) for k, v in R.hash_weights(cfg).items()}
    p = [w["transformer.h.0." + n].to(DEV) for n in NAMES]
    q = [Q().quantize_weight(p[i]) for i in (1, 2, 4, 5)]
    deq = [Q().dequantize_weight(c, s) for c, s in q]
    params = (p[0], deq[0], deq[1], p[3], deq[2], deq[3])
    tab = R.cast_rope_table(R.rope_table(Cc // H, T), BF)
    return dict(T=T, params=params, w4=([c for c, _ in q], [s for _, s in q]), rope=rope_tables(tab.to(DEV)), x=rnd(5, T, Cc, seed=Cc).to(DEV))


@pytest.mark.parametrize("B", (1, 5))
@pytest.mark.parametrize("Cc,H", [(128, 2), (256, 2)])
@pytest.mark.parametrize("kv8", (False, True))
def test_block_step_w4_has_the_bits_of_the_bf16_step(kv8, Cc, H, B):
    """behind a prefill of 20 positions: three uniform steps, then two with one position per row (a parked row among five), on a bf16 and
    an e4m3 cache — y and the cache's bytes equal those of the bf16 entry point on the dequantised parameters; four structure-10
    launches per step.  With the weight-streaming product off, the tile path on the dequantised weights, bit for bit again."""
    from omnibiote_amd.masks import RangeMask
    o, c = ops(), _block_case(Cc, H)
    T, T0, hs = c["T"], 20, Cc // H
    x = c["x"][:B]
    first = (o.kv8_cache_buffer if kv8 else o.kv_cache_buffer)(B, T, H, hs, DEV)
    first.zero_()
    (o.block_prefill_kv8 if kv8 else o.block_prefill)(x[:, :T0].contiguous(), c["params"], c["rope"], H,
                                                      o.MaskSpec.from_user(RangeMask.causal(B, T0, DEV), B, T0, H, DEV), first, T)

    def bf16_step(xt, cache, pos, rows):
        if kv8:
            return o.block_decode_kv8(xt, c["params"], c["rope"], H, cache, T, pos, rows)
        return o.block_decode(xt, c["params"], c["rope"], H, cache, T, pos) if rows is None else o.block_decode_rows(xt, c["params"], c["rope"], H, cache, T, rows, pos)

    for limit in (64, 0):
        a, b = first.clone(), first.clone()
        with o.small_m_max(limit), Profile() as p:
            for t in range(T0, T0 + 3):
                xt = x[:, t].contiguous()
                ya = o.block_step_w4(xt, c["params"], c["w4"], c["rope"], H, a, T, t, kv8=kv8)
                assert torch.equal(_bits(ya), _bits(bf16_step(xt, b, t, None))), ("uniform", limit, t)
            for i in range(2):
                at = [T0 + 3 + i - (r % 3) for r in range(B)]
                if B > 1:
                    at[1] = -1                                                      # a parked row
                rows = torch.tensor(at, dtype=torch.int32, device=DEV)
                xt = x[:, T0 + 3 + i].contiguous()
                ya = o.block_step_w4(xt, c["params"], c["w4"], c["rope"], H, a, T, max(at), rows, kv8=kv8)
                yb = bf16_step(xt, b, max(at), rows)
                live = rows >= 0
                assert torch.equal(_bits(ya[live]), _bits(yb[live])), ("rows", limit, i)
        assert torch.equal(a.view(torch.uint8), b.view(torch.uint8)), limit
        ten = [k for k in p.gemm if k // 1000 == 10]
        assert len(ten) == (4 * 5 if limit else 0) and len(p.gemm) == 2 * 4 * 5, p.gemm


def test_block_step_w4_refusals_name_the_call():
    o, c = ops(), _block_case(128, 2)
    cache = o.kv_cache_buffer(1, c["T"], 2, 64, DEV)
    xt = c["x"][:1, 0].contiguous()
    codes, scales = c["w4"]
    with pytest.raises(ValueError, match="block_step_w4"):
        o.block_step_w4(xt, c["params"], (codes[:3], scales), c["rope"], 2, cache, c["T"], 0)
    with pytest.raises(ValueError, match="block_step_w4: codes1"):
        o.block_step_w4(xt, c["params"], ([codes[0], codes[0], codes[2], codes[3]], scales), c["rope"], 2, cache, c["T"], 0)
    off = torch.cat([torch.zeros(4, dtype=torch.uint8, device=DEV), codes[0].flatten()])[4:].view(codes[0].shape)   # 4 bytes past a 16-byte boundary
    with pytest.raises(RuntimeError, match=r"obte_block_step_w4: codes\[0\] must be 8-byte aligned"):
        o.block_step_w4(xt, c["params"], ([off] + list(codes[1:]), scales), c["rope"], 2, cache, c["T"], 0)


# =================================================================================================== the model
@functools.lru_cache(maxsize=None)
def _gen():
    """2 layers, C = 128, V = 512, block_size 64: the model, its MXFP4 snapshot, the dequantised model and two prompts of 20 tokens"""
    cfg = R.RefConfig(block_size=64, vocab_size=512, n_layer=2, n_head=2, n_embd=128)
    m = _model(cfg, R.hash_weights(cfg), True)
    wq = m.quantize_weights(format="mxfp4")
    ids = torch.from_numpy(np.random.default_rng(128).integers(4, cfg.vocab_size, size=(2, 20)).astype(np.int64)).to(DEV)
    return m, wq, wq.dequantized_model(), ids


def test_decode_step_with_weights_is_the_dequantised_model():
    from omnibiote_amd.model import KVCache
    m, wq, dm, ids = _gen()
    assert wq.format == "mxfp4" and wq.head_scales.dtype == torch.uint8 and tuple(wq.head_codes.shape) == (512, 64)
    for kv in ("bf16", "fp8"):
        ca, cb = KVCache(m, 2, dtype=kv), KVCache(dm, 2, dtype=kv)
        la, lb = m.prefill(ids, ca, weights=wq), dm.prefill(ids, cb)
        assert torch.equal(_bits(la), _bits(lb)), kv
        with Profile() as p:
            for i in range(6):
                tok = la.float().argmax(-1)
                la, lb = m.decode_step(tok, ca, weights=wq), dm.decode_step(tok, cb)
                assert torch.equal(_bits(la), _bits(lb)), (kv, i)
        # four products per block and the readout: structure 10 from the codes, structure 8 in the dequantised model, no e4m3 product
        assert sum(1 for k in p.gemm if k // 1000 == 10) == 6 * (4 * 2 + 1) and sum(1 for k in p.gemm if k // 1000 == 8) == 6 * (4 * 2 + 1)
        assert not [k for k in p.gemm if k // 1000 == 9]


def test_above_the_row_limit_the_tile_path_runs_on_the_dequantised_weights():
    """65 rows: the blocks' products and the readout leave the weight-streaming product in both models, and agree bit for bit"""
    from omnibiote_amd.model import KVCache
    m, wq, dm, ids = _gen()
    wide = ids[:1].repeat(65, 1).contiguous()
    wide[:, 5] = torch.arange(65, device=DEV) + 4
    ca, cb = KVCache(m, 65), KVCache(dm, 65)
    la, lb = m.prefill(wide, ca, weights=wq), dm.prefill(wide, cb)
    assert torch.equal(_bits(la), _bits(lb))
    with Profile() as p:
        for i in range(2):
            tok = lb.float().argmax(-1)
            la, lb = m.decode_step(tok, ca, weights=wq), dm.decode_step(tok, cb)
            assert torch.equal(_bits(la), _bits(lb)), i
    assert not [k for k in p.gemm if k // 1000 in (8, 9, 10)]


GENERATE = [                                                                        # test_hip_w8.py's keyword sets
    dict(top_k=1),
    dict(sampler="device", top_k=40, top_p=0.9, temperature=0.8),
    dict(top_k=1, lengths=[20, 13]),
    dict(sampler="device", top_k=40, kv_dtype="fp8"),
    dict(sampler="device", top_k=40, allowed_tokens=list(range(3, 200)), min_new_tokens=5, eos_token=3),
    dict(sampler="device", top_k=40, top_p=0.9, loop="device", eos_token=3),
    dict(sampler="device", top_k=40, loop="graph"),
    dict(sampler="device", top_k=40, loop="graph", lengths=[20, 13], kv_dtype="fp8"),
]


@pytest.mark.parametrize("kw", GENERATE, ids=lambda kw: "-".join(f"{k}" for k in kw))
def test_generate_with_weights_gives_the_dequantised_models_tokens(kw):
    m, wq, dm, ids = _gen()

    def run(model, **more):
        return model.generate(ids, 12, generator=torch.Generator(device=DEV).manual_seed(7), **kw, **more)
    got, want = run(m, weights=wq), run(dm)
    if "lengths" in kw:
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
        got = got[0]
    else:
        assert torch.equal(got, want)
    assert got.shape[1] > 20


def test_weights_none_is_the_call_without_the_keyword():
    m, wq, dm, ids = _gen()
    for kw in (dict(top_k=1), dict(sampler="device", top_k=40, loop="graph")):
        a = m.generate(ids, 8, generator=torch.Generator(device=DEV).manual_seed(3), weights=None, **kw)
        b = m.generate(ids, 8, generator=torch.Generator(device=DEV).manual_seed(3), **kw)
        assert torch.equal(a, b)
    with Profile() as p:
        m.generate(ids, 4, top_k=1)
    assert not [k for k in p.gemm if k // 1000 in (9, 10)]                          # and no quantised product in it


def test_stale_snapshot_and_refusals_on_the_device():
    from omnibiote_amd.model import KVCache, SharedPrefixCache
    m, wq, dm, ids = _gen()
    with pytest.raises(NotImplementedError, match="generate"):
        m.generate(ids, 4, num_samples=2, weights=wq)
    shared = SharedPrefixCache(m, 2, 2, 20, 4)
    with pytest.raises(NotImplementedError, match="prefill"):
        m.prefill(ids, shared, weights=wq)
    cache = KVCache(m, 2)
    m.prefill(ids, cache, weights=wq)
    with pytest.raises(NotImplementedError, match="extend"):
        m.extend(ids[:, :3], cache, weights=wq)
    assert cache.pos == 20
    with pytest.raises(ValueError, match="another model"):
        dm.decode_step(ids[:, 0], KVCache(dm, 2), weights=wq)
    other = dm.quantize_weights(format="mxfp4")
    with torch.no_grad():
        dm.transformer.h[1].mlp.c_fc.weight.mul_(1.0)                               # same values, a new version
    with pytest.raises(ValueError, match="quantize_weights again"):
        dm.generate(ids, 4, weights=other)
