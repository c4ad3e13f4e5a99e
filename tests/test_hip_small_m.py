"""The weight-streaming product for 1 <= M <= 64 rows (obte_linear_small_m_bf16, csrc/gemm_small_m.hip) on the GPU: exact integer
products, its four epilogues bit for bit against the tile structures (ops.gemm) on equal products, random data at the project's GEMM
bar (tests/test_hip_ops.py: RTOL = 2^-7, atol = 0.02 sqrt(K)), row independence, repeatability, nothing read or written outside the
problem; then the decode forms of the block and generate() with the product on and off (ops.small_m_max), at the bars of
tests/test_hip_generate.py for the same quantities."""
import ctypes as C
import functools
import math

import numpy as np
import pytest
import torch

import omnibiote_ref as R
from test_hip_causal import _add, _model, _tril
from test_hip_ops import BF, DEV, RTOL, close, rnd

pytestmark = pytest.mark.gpu

MS = (1, 2, 7, 16, 17, 33, 64)
NAMES = ["ln_1.weight", "attn.c_attn.weight", "attn.c_proj.weight", "ln_2.weight", "mlp.c_fc.weight", "mlp.c_proj.weight"]


def ops():
    from omnibiote_amd import ops as o
    return o


def L():
    from omnibiote_amd import _lib
    return _lib


def tern(*shape, seed):
    """values drawn from {-1, 0, 1}, int64"""
    return torch.randint(-1, 2, shape, generator=torch.Generator().manual_seed(seed))


@functools.lru_cache(maxsize=None)
def _int_case(N, K):
    """x [64, K], W [N, K], aux [64, N] from {-1, 0, 1} and the exact int64 product of all 64 rows (computed once, never modified)"""
    x, w, aux = tern(64, K, seed=N + K), tern(N, K, seed=N + K + 1), tern(64, N, seed=N + K + 2)
    acc = x @ w.t()
    return dict(x=x.to(BF).to(DEV), w=w.to(BF).to(DEV), aux=aux.to(BF).to(DEV), acc=acc, aux_i=aux)


def _bits(t):
    return t.contiguous().view(torch.int16)


# =================================================================================================== exact
@pytest.mark.parametrize("N,K", [(16, 64), (24, 64), (136, 192), (384, 128), (1024, 4096), (512, 1024), (8200, 256), (8216, 512), (8208, 1024), (8200, 768)])
def test_small_m_exact_integer_products(N, K):
    """Every partial sum is an exact fp32 integer in any order: the result is bf16(alpha * the int64 sum), bit for bit.  K = 64 and 192
    leave waves without a chunk, N = 24 and 136 a half strip, N = 16 a single strip; (1024, 4096) is the mlp shape.  More than 512
    strips (N > 8192) at K = 256, 512, 1024 take the x-stationary kernel, two strips per workgroup, the last workgroup one (and a half
    strip at 8200 and 8216); K = 768 at that width stays on the first kernel."""
    o, c = ops(), _int_case(N, K)
    for M in MS:
        for alpha in (1.0, 0.5):
            got = o.linear_small_m(c["x"][:M], c["w"], alpha=alpha)
            want = (c["acc"][:M].double() * alpha).to(BF)
            assert got.shape == (M, N) and torch.equal(got.cpu(), want), (M, N, K, alpha)


# =================================================================================================== epilogues
@pytest.mark.parametrize("N,K", [(24, 64), (384, 128), (512, 1024), (8200, 256)])
def test_small_m_add_and_gelu_equal_the_tile_path(N, K):
    o, c, Lm = ops(), _int_case(N, K), L()
    for M in MS:
        x, aux = c["x"][:M].contiguous(), c["aux"][:M].contiguous()
        for alpha in (1.0, 0.5):
            want = o.gemm(x, c["w"], M, N, K, epilogue=Lm.EPI_ADD, aux=aux, alpha=alpha)
            got = o.linear_small_m(x, c["w"], epilogue=Lm.EPI_ADD, aux=aux, alpha=alpha)
            assert torch.equal(_bits(got), _bits(want)), ("ADD", M, N, K, alpha)
            assert torch.equal(got.cpu(), ((c["acc"][:M].double() * alpha).to(BF).float() + c["aux_i"][:M].float()).to(BF))
            out = aux.clone()                                                        # aux aliased to out
            assert o.linear_small_m(x, c["w"], epilogue=Lm.EPI_ADD, aux=out, alpha=alpha, out=out) is out
            assert torch.equal(_bits(out), _bits(want)), ("ADD in place", M, N, K, alpha)
        want = o.gemm(x, c["w"], M, N, K, epilogue=Lm.EPI_GELU_ACT)
        got = o.linear_small_m(x, c["w"], epilogue=Lm.EPI_GELU_ACT)
        assert torch.equal(_bits(got), _bits(want)), ("GELU_ACT", M, N, K)
        assert not torch.equal(_bits(got), _bits(o.linear_small_m(x, c["w"])))      # it did something


@pytest.mark.parametrize("hs,H,K", [(64, 2, 128), (128, 2, 256), (128, 22, 256)])
def test_small_m_rope_equals_the_tile_path(hs, H, K):
    """c_attn's epilogue at C = 2 hs (N = 3 C, K = C): rope_T = 1 at table row 5 (a decode step's form) at every M, rope_T = 4 at
    M = 7 (position = row % 4); the v third is the plain product, bit for bit.  22 heads of 128 (N = 8448) over K = 256: the
    x-stationary kernel's epilogue."""
    o, Lm = ops(), L()
    Cc = H * hs
    N = 3 * Cc
    c = _int_case(N, K)
    g = torch.Generator().manual_seed(hs)
    cos, sin = [torch.rand(9, hs // 2, generator=g).mul(2).sub(1).to(DEV) for _ in range(2)]
    for M, T, row in [(M, 1, 5) for M in MS] + [(7, 4, 0), (7, 4, 3)]:
        x = c["x"][:M].contiguous()
        rope = (cos[row:], sin[row:], T, hs)
        want = o.gemm(x, c["w"], M, N, K, epilogue=Lm.EPI_ROPE_QK, rope=rope)
        got = o.linear_small_m(x, c["w"], epilogue=Lm.EPI_ROPE_QK, rope=rope)
        plain = o.linear_small_m(x, c["w"])
        assert torch.equal(_bits(got), _bits(want)), (hs, M, T, row)
        assert torch.equal(_bits(got[:, 2 * Cc:]), _bits(plain[:, 2 * Cc:]))
        assert not torch.equal(_bits(got[:, :2 * Cc]), _bits(plain[:, :2 * Cc]))    # it did rotate


# =================================================================================================== random data
@pytest.mark.parametrize("N,K", [(136, 192), (384, 128), (1024, 4096), (4096, 1024), (8200, 512)])
def test_small_m_random_data_against_fp32(N, K):
    o = ops()
    x, w = rnd(64, K, seed=N), rnd(N, K, seed=K + 1)
    ref = x.float() @ w.float().t()
    wd = w.to(DEV)
    for M in MS:
        got = o.linear_small_m(x[:M].to(DEV), wd)
        close(got, ref[:M], atol=0.02 * math.sqrt(K), what=f"small M {M}x{N}x{K}")


def test_small_m_readout_shape():
    """the readout as decode_step calls it: 2 rows (and 64), 65 536 x 1024 weights (134 MB: offsets beyond 2^26 elements), alpha = 1 / 42"""
    o = ops()
    N, K, alpha = 65536, 1024, 1 / 42.0
    x, w = rnd(64, K, seed=3), rnd(N, K, seed=4)
    ref = (x.float() @ w.float().t()) * alpha
    wd = w.to(DEV)
    for M in (2, 64):
        got = o.linear_small_m(x[:M].to(DEV), wd, alpha=alpha)
        close(got, ref[:M], atol=0.02 * math.sqrt(K) * alpha, what=f"readout shape, M = {M}")


# =================================================================================================== rows, repeatability
@pytest.mark.parametrize("N,K", [(1024, 4096), (384, 128), (8200, 512)])
def test_small_m_rows_are_independent_and_calls_repeat(N, K):
    """the summation order is a function of (N, K) alone: a row has the same bits alone and inside 64 rows, and in every call"""
    o = ops()
    x, w = rnd(64, K, seed=11).to(DEV), rnd(N, K, seed=12).to(DEV)
    full = o.linear_small_m(x, w)
    assert torch.equal(_bits(full), _bits(o.linear_small_m(x, w)))
    for m in (0, 15, 16, 63):
        one = o.linear_small_m(x[m:m + 1], w)
        assert torch.equal(_bits(one[0]), _bits(full[m])), (N, K, m)
    for M in (17, 33):                                                               # and inside every MFMA count in between
        assert torch.equal(_bits(o.linear_small_m(x[:M], w)), _bits(full[:M])), (N, K, M)


# =================================================================================================== nothing outside the problem
@pytest.mark.parametrize("N,K", [(136, 192), (8200, 256)])
@pytest.mark.parametrize("M", MS)
def test_small_m_touches_nothing_outside_the_problem(M, N, K):
    o, Lm = ops(), L()
    marker = 0x1234
    c = _int_case(N, K)
    want = o.linear_small_m(c["x"][:M], c["w"])
    # out: [M, N] inside a [M + 3, N + 8] buffer (ldd = N + 8, three guard rows behind row M)
    buf = torch.full((M + 3, N + 8), marker, dtype=torch.int16, device=DEV)
    view = buf.view(BF)[:M, :N]
    # x: [M, K] inside a [66, K + 8] buffer whose every other element is the bf16 NaN 0x7FC0, then zero
    res = []
    for pattern in (0x7FC0, 0):
        xb = torch.full((66, K + 8), pattern, dtype=torch.int16, device=DEV).view(BF)
        xb[:M, :K] = c["x"][:M]
        if pattern:
            assert torch.isnan(xb[M:]).all() and torch.isnan(xb[:, K:]).all()
        for epi, aux in ((Lm.EPI_NONE, None), (Lm.EPI_ADD, view)):
            buf.fill_(marker)
            got = o.linear_small_m(xb[:M, :K], c["w"], epilogue=epi, aux=aux, out=view)
            assert torch.isfinite(got).all()
            assert (buf[M:] == marker).all() and (buf[:M, N:] == marker).all(), (M, epi)
            res.append(got.clone())
    assert torch.equal(_bits(res[0]), _bits(want))
    assert torch.equal(_bits(res[0]), _bits(res[2])) and torch.equal(_bits(res[1]), _bits(res[3]))


# =================================================================================================== block
class Profile:
    """the launch profiler (obte_profile_enable / obte_profile_collect) around a with-block: .kinds and .dims of every record"""

    def __enter__(self):
        L().lib().obte_profile_enable(1)
        return self

    def __exit__(self, *exc):
        lib, cap = L().lib(), 4096
        torch.cuda.synchronize()
        ms, dims, kind = (C.c_double * cap)(), (C.c_int64 * (3 * cap))(), (C.c_int32 * cap)()
        n = lib.obte_profile_collect(ms, dims, kind, cap)
        lib.obte_profile_enable(0)
        self.kinds = [kind[i] for i in range(n)]
        self.dims = [tuple(dims[3 * i:3 * i + 3]) for i in range(n)]
        self.gemm = [k for k in self.kinds if k % 1000 < 100]           # 4 x layout + epilogue + 1000 x structure; 102: attention decode
        return False


@functools.lru_cache(maxsize=None)
def _block_case(Cc, H):
    """three rows of 160 positions through one block: parameters, the oracle's causal forward (computed once, never modified)"""
    from omnibiote_amd.model import rope_tables
    B, T = 3, 160
    cfg = R.RefConfig(block_size=T, vocab_size=256, n_layer=1, n_head=H, n_embd=Cc)
    w = {k: v.to(BF) for k, v in R.hash_weights(cfg).items()}
    pre = "transformer.h.0."
    tab = R.cast_rope_table(R.rope_table(Cc // H, T), BF)
    x = rnd(B, T, Cc, seed=1)
    ref = R.block_forward(x.float(), {k: v.float() for k, v in w.items()}, pre, cfg, tab, _add(_tril(T)))
    return dict(B=B, T=T, params=tuple(w[pre + n].to(DEV) for n in NAMES), rope=rope_tables(tab.to(DEV)), x=x.to(DEV), ref=ref)


def _prefilled(c, Cc, H, T0):
    from omnibiote_amd.masks import RangeMask
    o, B, T = ops(), c["B"], c["T"]
    cache = o.kv_cache_buffer(B, T, H, Cc // H, DEV)
    o.block_prefill(c["x"][:, :T0].contiguous(), c["params"], c["rope"], H, o.MaskSpec.from_user(RangeMask.causal(B, T0, DEV), B, T0, H, DEV), cache, T)
    return cache


def _bar(ref):
    return 3e-2 + 2.0 ** -6 * ref.abs()          # the block bar of test_block_decode_step_by_step_vs_oracle


def _check_kinds(p, on, steps):
    if on:
        assert len(p.gemm) == 4 * steps and all(k // 1000 == 8 for k in p.gemm), p.gemm
    else:
        assert len(p.gemm) == 4 * steps and all(k // 1000 != 8 for k in p.gemm), p.gemm


@pytest.mark.parametrize("Cc,H", [(128, 2), (256, 2)])
def test_block_decode_on_and_off(Cc, H):
    """positions 130 .. 137 one at a time from copies of one prefilled cache, with the product on (64) and off (0): each run at the
    block bar of the oracle's row, the two within twice that bar of each other; four structure-8 launches per step, or none."""
    o, c = ops(), _block_case(Cc, H)
    T0, steps, T = 130, 8, c["T"]
    first = _prefilled(c, Cc, H, T0)
    ws = o.block_decode_workspace(c["B"], Cc, H, DEV)
    ys = {}
    for limit in (64, 0):
        cache = first.clone()
        with o.small_m_max(limit), Profile() as p:
            ys[limit] = [o.block_decode(c["x"][:, t].contiguous(), c["params"], c["rope"], H, cache, T, t, ws=ws) for t in range(T0, T0 + steps)]
        _check_kinds(p, limit > 0, steps)
        for i, y in enumerate(ys[limit]):
            close(y, c["ref"][:, T0 + i], atol=3e-2, rtol=2.0 ** -6, what=f"block_decode, small_m_max {limit}, position {T0 + i}")
    for i, (a, b) in enumerate(zip(ys[64], ys[0])):
        d = (a.float() - b.float()).abs().cpu()
        assert (d <= 2 * _bar(c["ref"][:, T0 + i])).all(), (i, d.max().item())
    with o.small_m_max(2), Profile() as p:                                   # three rows against a limit of two: the tile path
        o.block_decode(c["x"][:, T0].contiguous(), c["params"], c["rope"], H, first.clone(), T, T0, ws=ws)
    _check_kinds(p, False, 1)


@pytest.mark.parametrize("Cc,H", [(128, 2), (256, 2)])
def test_block_decode_rows_on_and_off(Cc, H):
    """the same for one position per row: row 0 through 97 .. 104, row 1 through 130 .. 137, row 2 parked (-1)"""
    o, c = ops(), _block_case(Cc, H)
    T0, steps, T, start = 130, 8, c["T"], (97, 130)
    first = _prefilled(c, Cc, H, T0)
    ws = o.block_decode_workspace(c["B"], Cc, H, DEV)
    ys = {}
    for limit in (64, 0):
        cache = first.clone()
        ys[limit] = []
        with o.small_m_max(limit), Profile() as p:
            for i in range(steps):
                at = [s + i for s in start]
                xt = torch.stack([c["x"][b, t] for b, t in enumerate(at)] + [c["x"][2, T0]]).contiguous()
                pos = torch.tensor(at + [-1], dtype=torch.int32, device=DEV)
                ys[limit].append(o.block_decode_rows(xt, c["params"], c["rope"], H, cache, T, pos, max(at), ws=ws))
        _check_kinds(p, limit > 0, steps)
        for i, y in enumerate(ys[limit]):
            want = torch.stack([c["ref"][b, s + i] for b, s in enumerate(start)])
            close(y[:2], want, atol=3e-2, rtol=2.0 ** -6, what=f"block_decode_rows, small_m_max {limit}, step {i}")
            assert torch.isfinite(y[2]).all()
    for i, (a, b) in enumerate(zip(ys[64], ys[0])):
        want = torch.stack([c["ref"][b_, s + i] for b_, s in enumerate(start)])
        d = (a[:2].float() - b[:2].float()).abs().cpu()
        assert (d <= 2 * _bar(want)).all(), (i, d.max().item())


# =================================================================================================== model
@functools.lru_cache(maxsize=None)
def _gen_model():
    """the 2-layer model of tests/test_hip_generate.py: block 200, vocab 512, 2 heads, n_embd 256"""
    cfg = R.RefConfig(block_size=200, vocab_size=512, n_layer=2, n_head=2, n_embd=256)
    ids = torch.from_numpy(np.random.default_rng(256).integers(4, cfg.vocab_size, size=(2, 130)).astype(np.int64))
    return _model(cfg, R.hash_weights(cfg), True), ids.to(DEV)


def test_generate_greedy_on_and_off():
    """generate(idx, 20, top_k=1) with the product off and at the default: in one causal forward over its own output each run's
    chosen logits lie within 2e-2 of their positions' maxima (the bound of test_generate_greedy_follows_the_full_forward).  At the
    default the readout and the blocks' products are structure-8 launches, with it off none is."""
    o = ops()
    m, idx = _gen_model()
    default = L().lib().obte_small_m_max()
    vocab, n_new = m.config.vocab_size, 20
    for limit in (0, default):
        with o.small_m_max(limit), Profile() as p:
            out = m.generate(idx, n_new, top_k=1)
        assert out.shape == (2, 130 + n_new) and torch.equal(out[:, :130], idx)
        eight = [d for k, d in zip(p.kinds, p.dims) if k // 1000 == 8]
        if limit >= 2:
            assert sum(1 for d in eight if d[1] == vocab) == n_new                       # the prefill's last-position readout and n_new - 1 steps'
            assert sum(1 for d in eight if d[1] != vocab) == 4 * 2 * (n_new - 1)         # four products per block and decode step
        else:
            assert not eight
        with torch.no_grad():
            logits = m(out).float()
        at = logits[:, 129:129 + n_new]
        gap = at.max(dim=-1).values - at.gather(-1, out[:, 130:].unsqueeze(-1)).squeeze(-1)
        print(f"greedy generate, small_m_max {limit}: largest logit gap to the full forward's maximum {gap.max().item():.4g}")
        assert (gap <= 2e-2).all(), (limit, gap.max().item())
