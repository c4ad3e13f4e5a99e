"""The decode step's products and readout on e4m3 weights (include/omnibiote_hip_w8.h, csrc/gemm_small_m.hip's WE4m3 policy) on the GPU.
The contract is equality of BITS with the bf16 path on the dequantised weights (w8quant.dequantize_weight): the product against
ops.linear_small_m at every epilogue, the block step against ops.block_decode / block_decode_rows / block_decode_kv8, the model against
QuantizedWeights.dequantized_model().  No test compares against the unquantised model with a bar (DESIGN.md 14.11 records that
deviation)."""
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
# (24, 64): N % 16 == 8 and three waves without a chunk; (200, 320): the unrolled chunk loop's tail; N > 8192 at K = 256 / 512 / 1024: the
# x-stationary kernel at every chunk count, the last strip a half one; (8200, 768): as many strips on the one-strip kernel
SHAPES = [(24, 64), (136, 192), (384, 128), (200, 320), (1024, 4096), (8200, 256), (8216, 512), (8208, 1024), (8200, 768)]


def ops():
    from omnibiote_amd import ops as o
    return o


def L():
    from omnibiote_amd import _lib
    return _lib


def Q():
    from omnibiote_amd import w8quant
    return w8quant


def _bits(t):
    return t.contiguous().view(torch.int16)


@functools.lru_cache(maxsize=None)
def _case(N, K):
    """x [64, K], aux [64, N], W [N, K] ~ N(0, 0.02) with a zero row, a row x 2^-20 and a row x 2^10, quantised; the dequantised weight
    (computed once, never modified)"""
    x, aux = rnd(64, K, seed=N + K), rnd(64, N, seed=N + K + 2)
    w = rnd(N, K, seed=N + K + 1, scale=0.02)
    w[1] = 0
    w[N // 2] = (w[N // 2].float() * 2.0 ** -20).to(BF)
    w[N - 1] = (w[N - 1].float() * 2.0 ** 10).to(BF)
    codes, scales = Q().quantize_weight(w.to(DEV))
    return dict(x=x.to(DEV), aux=aux.to(DEV), codes=codes, scales=scales, deq=Q().dequantize_weight(codes, scales))


# =================================================================================================== the product, bit for bit
@pytest.mark.parametrize("N,K", SHAPES)
def test_w8_product_has_the_bits_of_the_bf16_product_on_the_dequantised_weight(N, K):
    o, Lm, c = ops(), L(), _case(N, K)
    assert int((c["scales"][1] == 2.0 ** -126)) and int(c["codes"][1].max()) == 0          # the zero row
    for M in MS:
        x, aux = c["x"][:M].contiguous(), c["aux"][:M].contiguous()
        for alpha in (1.0, 0.37):
            want = o.linear_small_m(x, c["deq"], alpha=alpha)
            got = o.linear_small_m_w8(x, c["codes"], c["scales"], alpha=alpha)
            assert got.shape == (M, N) and torch.equal(_bits(got), _bits(want)), ("NONE", M, N, K, alpha)
            want = o.linear_small_m(x, c["deq"], epilogue=Lm.EPI_ADD, aux=aux, alpha=alpha)
            out = aux.clone()                                                               # aux aliased to out
            assert o.linear_small_m_w8(x, c["codes"], c["scales"], epilogue=Lm.EPI_ADD, aux=out, alpha=alpha, out=out) is out
            assert torch.equal(_bits(out), _bits(want)), ("ADD", M, N, K, alpha)
        want = o.linear_small_m(x, c["deq"], epilogue=Lm.EPI_GELU_ACT)
        got = o.linear_small_m_w8(x, c["codes"], c["scales"], epilogue=Lm.EPI_GELU_ACT)
        assert torch.equal(_bits(got), _bits(want)), ("GELU_ACT", M, N, K)
    assert torch.isfinite(want).all() and float(want.float().abs().max()) > 0


@pytest.mark.parametrize("hs,H,K", [(64, 2, 128), (128, 2, 256), (128, 22, 256)])
def test_w8_rope_epilogue(hs, H, K):
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
        got = o.linear_small_m_w8(x, c["codes"], c["scales"], epilogue=Lm.EPI_ROPE_QK, rope=rope)
        assert torch.equal(_bits(got), _bits(want)), (hs, H, M, T, row)
        assert not torch.equal(_bits(got), _bits(o.linear_small_m_w8(x, c["codes"], c["scales"])))       # it did rotate


@pytest.mark.parametrize("N,K", [(136, 192), (8200, 256)])
def test_w8_leading_dimensions(N, K):
    """ldd > N and ld_codes > K: codes as a row-strided view whose padding is 0x7F (the NaN code), d inside a marked buffer"""
    o, c = ops(), _case(N, K)
    wide = torch.full((N, K + 48), 0x7F, dtype=torch.uint8, device=DEV)
    wide[:, :K] = c["codes"]
    for M in (1, 17, 64):
        want = o.linear_small_m(c["x"][:M], c["deq"])
        buf = torch.full((M + 3, N + 8), 0x1234, dtype=torch.int16, device=DEV)
        got = o.linear_small_m_w8(c["x"][:M], wide[:, :K], c["scales"], out=buf.view(BF)[:M, :N])
        assert torch.equal(_bits(got), _bits(want)), (M, N, K)
        assert (buf[M:] == 0x1234).all() and (buf[:M, N:] == 0x1234).all()


@pytest.mark.parametrize("N,K", [(24, 64), (200, 320), (1024, 4096), (8216, 512)])
def test_w8_exact_integer_products(N, K):
    """ternary x, weights from {0, +-1, +-2} * 2^e with one e per row, every one an e4m3 value under the row's scale: the quantisation is
    exact and the result is bf16(the int64 product * 2^e), bit for bit"""
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
        got = o.linear_small_m_w8(x[:M].to(BF).to(DEV), codes, scales)
        assert torch.equal(got.cpu(), acc[:M].to(BF)), (M, N, K)


@pytest.mark.parametrize("N,K", [(1024, 4096), (384, 128), (8216, 512)])
def test_w8_rows_are_independent_and_calls_repeat(N, K):
    o, c = ops(), _case(N, K)
    full = o.linear_small_m_w8(c["x"], c["codes"], c["scales"])
    assert torch.equal(_bits(full), _bits(o.linear_small_m_w8(c["x"], c["codes"], c["scales"])))
    for m in (0, 15, 16, 63):
        one = o.linear_small_m_w8(c["x"][m:m + 1], c["codes"], c["scales"])
        assert torch.equal(_bits(one[0]), _bits(full[m])), (N, K, m)
    for M in (2, 7, 17, 33):
        assert torch.equal(_bits(o.linear_small_m_w8(c["x"][:M], c["codes"], c["scales"])), _bits(full[:M])), (N, K, M)


@pytest.mark.parametrize("N,K", [(136, 192), (8200, 256)])
@pytest.mark.parametrize("M", (1, 17, 64))
def test_w8_fenced(M, N, K):
    """x, codes, scales, aux and d in poisoned buffers aligned to 16 bytes (scales: 4) and no more: guards intact, the unfenced bits"""
    o, Lm, c = ops(), L(), _case(N, K)
    want = o.linear_small_m_w8(c["x"][:M], c["codes"], c["scales"], epilogue=Lm.EPI_ADD, aux=c["aux"][:M].contiguous())
    x, hx = F.fenced(c["x"][:M], poison="nan")
    codes, hc = F.fenced(c["codes"], poison=0x7F)                                   # the NaN code
    s16, hs_ = F.fenced(torch.cat([torch.zeros(3, device=DEV), c["scales"]]), poison="nan")
    scales = s16[3:]                                                                # 16 + 12 bytes: aligned to 4 and no more
    assert scales.data_ptr() % 16 == 12
    s16[:3] = float("nan")
    aux, ha = F.fenced(c["aux"][:M], poison="nan")
    d, hd = F.fenced((M, N), BF, poison="mark")
    got = o.linear_small_m_w8(x, codes, scales, epilogue=Lm.EPI_ADD, aux=aux, out=d)
    torch.cuda.synchronize()
    F.assert_guards(hx, hc, ha, hd)
    assert bool(torch.isnan(s16[:3]).all())
    F.assert_same_bits(got, want, f"fenced w8 product {M}x{N}x{K}")
    plain, hp = F.fenced((M, N), BF, poison="mark")
    F.assert_same_bits(o.linear_small_m_w8(x, codes, scales, out=plain), o.linear_small_m_w8(c["x"][:M], c["codes"], c["scales"]), "EPI_NONE")
    F.assert_guards(hp)


def test_w8_refusals_name_the_call():
    lib, Lm = L().lib(), L()
    x, codes, scales, d = (torch.zeros(4096, dtype=torch.uint8, device=DEV) for _ in range(4))

    def call(M=2, N=16, K=64, epi=0, codes_at=0, ld=None, alpha=1.0):
        g = Lm.GemmArgs(x.data_ptr(), None, d.data_ptr(), None, None, M, N, K, K, K, N, 1, 1, epi, alpha, 0.0, 0, 0)
        return lib.obte_linear_small_m_w8(C.byref(g), codes.data_ptr() + codes_at, K if ld is None else ld, scales.data_ptr(), None)

    for kw, rc, word in [(dict(K=96), EINVAL, "K"), (dict(M=65), EINVAL, "M must be"), (dict(codes_at=8), EINVAL, "aligned"), (dict(epi=1), EUNSUPPORTED, "epilogue"),
                         (dict(ld=72), EINVAL, "ld_codes"), (dict(ld=48), EINVAL, "ld_codes"), (dict(epi=9, alpha=0.5), EINVAL, "alpha")]:
        assert call(**kw) == rc, kw
        err = lib.obte_last_error().decode()
        assert err.startswith("obte_linear_small_m_w8:") and word in err, (kw, err)
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
    return dict(T=T, params=params, w8=([c for c, _ in q], [s for _, s in q]), rope=rope_tables(tab.to(DEV)), x=rnd(5, T, Cc, seed=Cc).to(DEV))


@pytest.mark.parametrize("B", (1, 5))
@pytest.mark.parametrize("Cc,H", [(128, 2), (256, 2)])
@pytest.mark.parametrize("kv8", (False, True))
def test_block_step_w8_has_the_bits_of_the_bf16_step(kv8, Cc, H, B):
    """behind a prefill of 20 positions: three uniform steps, then two with one position per row (a parked row among five), on a bf16 and
    an e4m3 cache — y and the cache's bytes equal those of the bf16 entry point on the dequantised parameters; four structure-9
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
                ya = o.block_step_w8(xt, c["params"], c["w8"], c["rope"], H, a, T, t, kv8=kv8)
                assert torch.equal(_bits(ya), _bits(bf16_step(xt, b, t, None))), ("uniform", limit, t)
            for i in range(2):
                at = [T0 + 3 + i - (r % 3) for r in range(B)]
                if B > 1:
                    at[1] = -1                                                      # a parked row
                rows = torch.tensor(at, dtype=torch.int32, device=DEV)
                xt = x[:, T0 + 3 + i].contiguous()
                ya = o.block_step_w8(xt, c["params"], c["w8"], c["rope"], H, a, T, max(at), rows, kv8=kv8)
                yb = bf16_step(xt, b, max(at), rows)
                live = rows >= 0
                assert torch.equal(_bits(ya[live]), _bits(yb[live])), ("rows", limit, i)
        assert torch.equal(a.view(torch.uint8), b.view(torch.uint8)), limit
        nine = [k for k in p.gemm if k // 1000 == 9]
        assert len(nine) == (4 * 5 if limit else 0) and len(p.gemm) == 2 * 4 * 5, p.gemm


# =================================================================================================== the model
@functools.lru_cache(maxsize=None)
def _gen():
    """2 layers, C = 128, V = 512, block_size 64: the model, its snapshot, the dequantised model and two prompts of 20 tokens"""
    cfg = R.RefConfig(block_size=64, vocab_size=512, n_layer=2, n_head=2, n_embd=128)
    m = _model(cfg, R.hash_weights(cfg), True)
    wq = m.quantize_weights()
    ids = torch.from_numpy(np.random.default_rng(128).integers(4, cfg.vocab_size, size=(2, 20)).astype(np.int64)).to(DEV)
    return m, wq, wq.dequantized_model(), ids


def test_decode_step_with_weights_is_the_dequantised_model():
    from omnibiote_amd.model import KVCache
    m, wq, dm, ids = _gen()
    for kv in ("bf16", "fp8"):
        ca, cb = KVCache(m, 2, dtype=kv), KVCache(dm, 2, dtype=kv)
        la, lb = m.prefill(ids, ca, weights=wq), dm.prefill(ids, cb)
        assert torch.equal(_bits(la), _bits(lb)), kv
        with Profile() as p:
            for i in range(6):
                tok = la.float().argmax(-1)
                la, lb = m.decode_step(tok, ca, weights=wq), dm.decode_step(tok, cb)
                assert torch.equal(_bits(la), _bits(lb)), (kv, i)
        # four products per block and the readout: structure 9 from the codes, structure 8 in the dequantised model
        assert sum(1 for k in p.gemm if k // 1000 == 9) == 6 * (4 * 2 + 1) and sum(1 for k in p.gemm if k // 1000 == 8) == 6 * (4 * 2 + 1)


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
    assert not [k for k in p.gemm if k // 1000 in (8, 9)]


GENERATE = [
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
    assert not [k for k in p.gemm if k // 1000 == 9]                                # and no e4m3 product in it


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
    other = dm.quantize_weights()
    with torch.no_grad():
        dm.transformer.h[1].mlp.c_fc.weight.mul_(1.0)                               # same values, a new version
    with pytest.raises(ValueError, match="quantize_weights again"):
        dm.generate(ids, 4, weights=other)
