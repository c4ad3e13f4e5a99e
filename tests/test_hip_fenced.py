"""Guard-band tests of the training kernels (tests/fenced.py): every entry point runs once on plain stand-alone tensors and once with
every operand inside a poisoned buffer that starts 16 bytes behind a 512-byte boundary — NaN around the inputs and in the scratch whose
contents are documented as irrelevant, a marker pattern around the outputs.  Each case asserts (a) every guard byte is intact, (b) the
output is finite wherever the plain call's is, (c) the output equals the plain call's bit for bit, under the same forced plan where a
plan applies (the atomic sums of squares keep the relative bar of test_adamw_matches_fp32_formula).  The C ABI is called directly
through _lib's argument structs.  Bars against the oracle are those of tests/test_hip_ops.py for the same quantities."""
import ctypes as C
import functools
import math

import numpy as np
import pytest
import torch

import omnibiote_ref as R
from fenced import assert_finite_where, assert_guards, assert_same_bits, fenced, filled
from test_hip_ops import BF, DEV, _blocks_to_masks, close, rnd

pytestmark = pytest.mark.gpu

F32, I32, I64, U8 = torch.float32, torch.int32, torch.int64, torch.uint8
LAYOUTS = {"nt": (1, 1), "nn": (1, 0), "tn": (0, 0)}     # x W^T, dy W, dy^T x: (a_kmajor, b_kmajor)
SEED = 0x1234_5678_9ABC


def L():
    from omnibiote_amd import _lib
    return _lib


def lib():
    return L().lib()


def st():
    return torch.cuda.current_stream().cuda_stream


def ptr(t):
    return None if t is None else t.data_ptr()


def chk(rc, what):
    L().check(rc, what)


class Plain:
    """stand-alone tensors, exactly as large as the problem"""
    fenced = False

    def __init__(self):
        self.handles = []

    def inp(self, t, ld=None):
        return t.to(DEV).contiguous().clone()

    def out(self, shape, dtype=BF, ld=None, fill=None):
        return filled(shape, dtype, "mark" if fill is None else fill, DEV)

    def scratch(self, shape, dtype=F32, front_bytes=16):
        return filled(shape, dtype, "nan", DEV)


class Fenced(Plain):
    """the same operands inside poisoned buffers"""
    fenced = True

    def _keep(self, pair):
        self.handles.append(pair[1])
        return pair[0]

    def inp(self, t, ld=None):
        return self._keep(fenced(t, poison="nan", ld=ld, device=DEV))

    def out(self, shape, dtype=BF, ld=None, fill=None):
        return self._keep(fenced(shape, dtype, "mark", ld=ld, device=DEV, fill=fill))

    def scratch(self, shape, dtype=F32, front_bytes=16):
        return self._keep(fenced(shape, dtype, "nan", front_bytes=front_bytes, device=DEV))


def both(case, loose=()):
    """case(A) -> {name: output}: run on plain and on fenced operands; (a), (b), (c).  Returns (plain outputs, fenced outputs)."""
    plain, fence = Plain(), Fenced()
    want = case(plain)
    got = case(fence)
    torch.cuda.synchronize()
    assert fence.handles
    assert_guards(*fence.handles)
    assert set(got) == set(want)
    for k in want:
        if k in loose:
            assert_finite_where(got[k], want[k], k)
        else:
            assert_same_bits(got[k], want[k], k)
    return want, got


def ld(t):
    return t.stride(-2)


def test_the_fence_itself_on_the_device():
    """tests/test_fenced_host.py on the device the kernels see: alignment, poison, and a torch store one element outside the payload"""
    x = rnd(5, 24)
    for ldx in (None, 32):
        v, h = fenced(x, poison="nan", ld=ldx, device=DEV)
        assert v.data_ptr() % 512 == 16 and torch.equal(v.cpu(), x)
        assert_guards(h)
        typed = h.whole.view(BF)
        assert torch.isnan(typed[:h.first]).all() and torch.isnan(typed[h.first + 5 * (ldx or 24):]).all()
        for at in (h.first - 1, h.first + 5 * (ldx or 24), h.whole.numel() - 1) + ((h.first + 24,) if ldx else ()):
            keep = h.whole[at].clone()
            h.whole[at] = 0
            with pytest.raises(AssertionError, match="guard overwritten"):
                assert_guards(h)
            h.whole[at] = keep
        assert_guards(h)


# ========================================================================================================= GEMM
@functools.lru_cache(maxsize=None)
def _gemm_data(lay, M, N, K):
    ak, bk = LAYOUTS[lay]
    a = rnd(M, K, seed=M + K) if ak else rnd(K, M, seed=M + K)
    b = rnd(N, K, seed=N + K + 1, scale=0.2) if bk else rnd(K, N, seed=N + K + 1, scale=0.2)
    ref = (a.float() if ak else a.float().t()) @ (b.float().t() if bk else b.float())
    return a, b, ref, rnd(M, N, seed=M + N + 2)


def _args(a, b, d, M, N, K, lay, epi=0, aux=None, d2=None, alpha=1.0, ldd=None):
    ak, bk = LAYOUTS[lay]
    return L().GemmArgs(ptr(a), ptr(b), ptr(d), ptr(aux), ptr(d2), M, N, K, ld(a), ld(b), ldd if ldd is not None else (ld(d) if d is not None else N),
                        ak, bk, epi, float(alpha), 0.0, 0, 0)


def _launch(g, ws=None):
    if ws is not None:
        chk(lib().obte_gemm_bf16_ws(C.byref(g), ptr(ws), ws.numel() * ws.element_size(), st()), "obte_gemm_bf16_ws")
    else:
        chk(lib().obte_gemm_bf16(C.byref(g), st()), "obte_gemm_bf16")


class Plans:
    """plans forced through the plan table, cleared on exit"""

    def __enter__(self):
        return self

    def set(self, lay, epi, M, N, K, structure, width, splits=1):
        ak, bk = LAYOUTS[lay]
        chk(lib().obte_gemm_plan_set(ak, bk, epi, M, N, K, structure, width, splits), "obte_gemm_plan_set")

    def __exit__(self, *exc):
        chk(lib().obte_gemm_plan_clear(), "obte_gemm_plan_clear")
        return False


class Launches:
    """the launch profiler around a with-block: .kinds of every record (a GEMM's is 1000 x structure + 4 x layout + epilogue)"""

    def __enter__(self):
        lib().obte_profile_enable(1)
        return self

    def __exit__(self, *exc):
        cap = 64
        torch.cuda.synchronize()
        ms, dims, kind = (C.c_double * cap)(), (C.c_int64 * (3 * cap))(), (C.c_int32 * cap)()
        n = lib().obte_profile_collect(ms, dims, kind, cap)
        lib().obte_profile_enable(0)
        self.kinds = [kind[i] for i in range(n)]
        return False


STRUCTURES = [(1, 128), (2, 128), (2, 256), (3, 256), (4, 128)]


@pytest.mark.parametrize("lay", list(LAYOUTS))
@pytest.mark.parametrize("structure,width", STRUCTURES)
def test_gemm_edge_tiles_and_leading_dimensions(structure, width, lay):
    """One full tile plus 8 rows and 8 columns; K of one and of three K-tiles (k-major operands) or ragged (the weight-gradient layout);
    dense, then ldd, lda, ldb each 8 elements longer than the row."""
    MN = width + 8
    with Plans() as plans:
        for K in ((64, 192) if lay != "tn" else (77, 300)):
            plans.set(lay, L().EPI_NONE, MN, MN, K, structure, width)
            a, b, ref, _ = _gemm_data(lay, MN, MN, K)
            for pa, pb, pd in ((0, 0, 0), (0, 0, 8), (8, 0, 0), (0, 8, 0)):
                def case(A):
                    ad, bd = A.inp(a, ld=a.shape[1] + pa), A.inp(b, ld=b.shape[1] + pb)
                    d = A.out((MN, MN), ld=MN + pd)
                    _launch(_args(ad, bd, d, MN, MN, K, lay))
                    return dict(d=d)
                with Launches() as seen:
                    want, _ = both(case)
                # the forced structure ran (the half-tile rings hand a K of one K-tile to structure 2: include/omnibiote_hip.h, plans)
                expect = 2 if structure in (3, 4) and K <= 64 else structure
                assert seen.kinds and all(k // 1000 == expect for k in seen.kinds), (seen.kinds, expect)
                close(want["d"], ref, atol=0.02 * math.sqrt(K) * 0.2, what=f"gemm {lay} structure {structure} K {K}")


@pytest.mark.parametrize("structure,width", [(2, 128), (2, 256), (3, 256)])
def test_gemm_strided_forms_of_the_rows_block(structure, width):
    """The strides the rows form of the block runs (C = 128): the k and v thirds written into a packed [M, 3C] buffer (N = 2C, ldd = 3C,
    column offset C; the q third keeps its marker), a k-major A of K = 2C read from such a buffer, and a k-strided A of M = 2C."""
    Cc, rows = 128, 154
    with Plans() as plans:
        # N = 2C into ldd = 3C
        plans.set("nt", L().EPI_NONE, rows, 2 * Cc, Cc, structure, width)
        a, b, ref, _ = _gemm_data("nt", rows, 2 * Cc, Cc)

        def case(A):
            ad, bd, buf = A.inp(a), A.inp(b), A.out((rows, 3 * Cc))
            _launch(_args(ad, bd, buf[:, Cc:], rows, 2 * Cc, Cc, "nt", ldd=3 * Cc))
            return dict(buf=buf)
        want, _ = both(case)
        assert torch.equal(want["buf"][:, :Cc], filled((rows, Cc), BF, "mark", DEV)), "the q third was written"
        close(want["buf"][:, Cc:], ref, atol=0.02 * math.sqrt(Cc) * 0.2, what="N = 2C into ldd = 3C")
        # lda = 3C, K = 2C: dx = d(kv) W_kv
        plans.set("nn", L().EPI_NONE, rows, Cc, 2 * Cc, structure, width)
        packed, w = rnd(rows, 3 * Cc, seed=3), rnd(2 * Cc, Cc, seed=4, scale=0.2)

        def case(A):
            pk, wd, d = A.inp(packed), A.inp(w), A.out((rows, Cc))
            g = _args(pk, wd, d, rows, Cc, 2 * Cc, "nn")
            g.a = pk[:, Cc:].data_ptr()
            _launch(g)
            return dict(d=d)
        want, _ = both(case)
        close(want["d"], packed[:, Cc:].float() @ w.float(), atol=0.02 * math.sqrt(2 * Cc) * 0.2, what="lda = 3C, K = 2C")
        # a_kmajor = 0, lda = 3C, M = 2C: dW_kv = d(kv)^T x
        plans.set("tn", L().EPI_NONE, 2 * Cc, Cc, rows, structure, width)
        x = rnd(rows, Cc, seed=5)

        def case(A):
            pk, xd, d = A.inp(packed), A.inp(x), A.out((2 * Cc, Cc))
            g = _args(pk, xd, d, 2 * Cc, Cc, rows, "tn")
            g.a = pk[:, Cc:].data_ptr()
            _launch(g)
            return dict(d=d)
        want, _ = both(case)
        close(want["d"], packed[:, Cc:].float().t() @ x.float(), atol=0.02 * math.sqrt(rows), what="a_kmajor = 0, lda = 3C, M = 2C")


def test_gemm_192_wide_tile_fenced():
    M, N, K = 264, 200, 192
    with Plans() as plans:
        plans.set("nt", L().EPI_NONE, M, N, K, 2, 192)
        a, b, ref, _ = _gemm_data("nt", M, N, K)
        for pa, pb, pd in ((0, 0, 0), (8, 8, 8)):
            def case(A):
                ad, bd, d = A.inp(a, ld=K + pa), A.inp(b, ld=K + pb), A.out((M, N), ld=N + pd)
                _launch(_args(ad, bd, d, M, N, K, "nt"))
                return dict(d=d)
            want, _ = both(case)
            close(want["d"], ref, atol=0.02 * math.sqrt(K) * 0.2, what="gemm 192 wide")


def test_gemm_persistent_structure_fenced():
    """Structure 7 at the smallest shape it accepts, fenced; bit for bit structure 3's result (as test_gemm_persistent_continuous_ring_structure)."""
    M, N, K = 8192, 2048, 256
    a, b = rnd(M, K, seed=61), rnd(N, K, seed=62, scale=0.2)
    outs = {}
    with Plans() as plans:
        for structure in (7, 3):
            plans.set("nt", L().EPI_NONE, M, N, K, structure, 256)
            A = Fenced()
            ad, bd, d = A.inp(a), A.inp(b), A.out((M, N))
            _launch(_args(ad, bd, d, M, N, K, "nt"))
            torch.cuda.synchronize()
            assert_guards(*A.handles)
            assert torch.isfinite(d).all()
            outs[structure] = d
    assert_same_bits(outs[7], outs[3], "structure 7 vs 3")
    rows = torch.arange(0, M, 257)
    close(outs[7][rows.to(DEV)], a[rows].float() @ b.float().t(), atol=0.02 * math.sqrt(K) * 0.2, what="structure 7")


@pytest.mark.parametrize("structure", [2, 3])
def test_gemm_epilogues_fenced(structure):
    M, N, K = 264, 264, 128
    Lm = L()
    with Plans() as plans:
        a, b, ref, r = _gemm_data("nt", M, N, K)
        for epi in (Lm.EPI_NONE, Lm.EPI_ADD, Lm.EPI_GELU, Lm.EPI_ADD_DROPOUT, Lm.EPI_GELU_ACT):
            plans.set("nt", epi, M, N, K, structure, 256)
        # ADD with aux aliasing d
        def case(A):
            ad, bd, d = A.inp(a), A.inp(b), A.inp(r)
            _launch(_args(ad, bd, d, M, N, K, "nt", Lm.EPI_ADD, aux=d))
            return dict(d=d)
        want, _ = both(case)
        close(want["d"], r.float() + ref.to(BF).float(), atol=0.03, what="add in place")
        # GELU: d and d2
        def case(A):
            ad, bd, d, d2 = A.inp(a), A.inp(b), A.out((M, N)), A.out((M, N))
            _launch(_args(ad, bd, d, M, N, K, "nt", Lm.EPI_GELU, d2=d2))
            return dict(d=d, d2=d2)
        want, _ = both(case)
        close(want["d2"], R.gelu_erf(ref.to(BF).float()), atol=0.03, what="gelu act")
        gelu_act = want["d2"]
        # ADD_DROPOUT
        def case(A):
            ad, bd, d, aux = A.inp(a), A.inp(b), A.out((M, N)), A.inp(r)
            g = _args(ad, bd, d, M, N, K, "nt", Lm.EPI_ADD_DROPOUT, aux=aux)
            g.dropout_p, g.dropout_site, g.dropout_seed = 0.1, 2, SEED
            _launch(g)
            return dict(d=d)
        want, _ = both(case)
        kept = (want["d"] != r.to(DEV)).float().mean().item()
        assert 0.85 < kept < 0.95, kept
        # GELU_ACT: EPI_GELU's d2
        def case(A):
            ad, bd, d = A.inp(a), A.inp(b), A.out((M, N))
            _launch(_args(ad, bd, d, M, N, K, "nt", Lm.EPI_GELU_ACT))
            return dict(d=d)
        want, _ = both(case)
        assert_same_bits(want["d"], gelu_act, "GELU_ACT vs GELU's d2")
        # GELU_BWD in the dy W layout, aux fenced
        plans.set("nn", Lm.EPI_GELU_BWD, M, N, K, structure, 256)
        a2, b2, ref2, h = _gemm_data("nn", M, N, K)

        def case(A):
            ad, bd, d, aux = A.inp(a2), A.inp(b2), A.out((M, N)), A.inp(h)
            _launch(_args(ad, bd, d, M, N, K, "nn", Lm.EPI_GELU_BWD, aux=aux))
            return dict(d=d)
        want, _ = both(case)
        close(want["d"], ref2.to(BF).float() * h.float(), atol=0.03, what="gelu bwd")
        # ROPE_QK: B T = 154, C = 128, hs = 64, the tables fenced
        Bb, T, Cc, hs = 2, 77, 128, 64
        for epi in (Lm.EPI_NONE, Lm.EPI_ROPE_QK):
            plans.set("nt", epi, Bb * T, 3 * Cc, Cc, structure, 256)
        x, w = rnd(Bb * T, Cc, seed=61), rnd(3 * Cc, Cc, seed=62, scale=0.1)
        tab = torch.randn(T, hs // 2, generator=torch.Generator().manual_seed(1))

        def case(A):
            xd, wd, d, cos, sin = A.inp(x), A.inp(w), A.out((Bb * T, 3 * Cc)), A.inp(torch.cos(tab)), A.inp(torch.sin(tab))
            g = _args(xd, wd, d, Bb * T, 3 * Cc, Cc, "nt", Lm.EPI_ROPE_QK)
            g.rope_cos, g.rope_sin, g.rope_T, g.rope_head_dim = cos.data_ptr(), sin.data_ptr(), T, hs
            _launch(g)
            plain = A.out((Bb * T, 3 * Cc))
            _launch(_args(xd, wd, plain, Bb * T, 3 * Cc, Cc, "nt"))
            chk(lib().obte_rope_qk_inplace(ptr(plain), ptr(cos), ptr(sin), Bb, T, Cc // hs, hs, 0, st()), "obte_rope_qk_inplace")
            return dict(d=d, plain=plain)
        want, _ = both(case)
        assert_same_bits(want["d"], want["plain"], "RoPE epilogue vs projection then RoPE")
        # ACC32: FIRST then LAST, the fp32 buffer fenced
        plans.set("tn", Lm.EPI_NONE, M, N, K, structure, 256)
        a3, b3, ref3, _ = _gemm_data("tn", M, N, K)

        def case(A):
            ad, bd, d, acc = A.inp(a3), A.inp(b3), A.out((M, N)), A.out((M, N), F32)
            for mode, dd in ((Lm.ACC32_FIRST, None), (Lm.ACC32_LAST, d)):
                g = _args(ad, bd, dd, M, N, K, "tn", Lm.EPI_ACC32, ldd=N)
                g.acc32, g.acc32_mode = acc.data_ptr(), mode
                _launch(g)
            return dict(d=d, acc=acc)
        want, _ = both(case)
        close(want["acc"], 2.0 * ref3, atol=1e-3, rtol=1e-4, what="acc32 buffer")
        assert torch.equal(want["d"], want["acc"].to(BF))


@pytest.mark.parametrize("structure,width", [(2, 128), (2, 256), (3, 256)])
def test_gemm_split_k_fenced(structure, width):
    """the weight-gradient layout, 4 splits, the workspace full of NaN inside its own fence"""
    M, N, K, splits = 384, 256, 4096, 4
    a, b, ref, r = _gemm_data("tn", M, N, K)
    Lm = L()
    with Plans() as plans:
        plans.set("tn", Lm.EPI_NONE, M, N, K, structure, width, splits)
        for epi in (Lm.EPI_NONE, Lm.EPI_ADD):
            def case(A):
                ad, bd = A.inp(a), A.inp(b)
                d = A.inp(r) if epi == Lm.EPI_ADD else A.out((M, N))
                ws = A.scratch((splits * M * N,), F32)
                _launch(_args(ad, bd, d, M, N, K, "tn", epi, aux=d if epi == Lm.EPI_ADD else None), ws=ws)
                return dict(d=d)
            want, _ = both(case)
            close(want["d"], ref + (r.float() if epi == Lm.EPI_ADD else 0.0), atol=0.01 * math.sqrt(K) + 0.03, what=f"split-K epilogue {epi}")


def test_gemm_grouped_fenced():
    """three problems of mixed layout in one grouped launch, one of them accumulating; every operand and output fenced"""
    Lm = L()
    probs = [("tn", 264, 264, 300, True), ("tn", 256, 136, 300, False), ("nn", 200, 136, 128, False)]
    data = [_gemm_data(lay, M, N, K) for lay, M, N, K, _ in probs]

    def case(A):
        arr = (Lm.GemmArgs * len(probs))()
        outs, held = {}, []
        for i, ((lay, M, N, K, acc), (a, b, _, r)) in enumerate(zip(probs, data)):
            ad, bd = A.inp(a), A.inp(b)
            held += [ad, bd]                                                  # (alive until the launch has been enqueued)
            d = A.inp(r) if acc else A.out((M, N))
            arr[i] = _args(ad, bd, d, M, N, K, lay, Lm.EPI_ADD if acc else Lm.EPI_NONE, aux=d if acc else None)
            outs[f"d{i}"] = d
        chk(lib().obte_gemm_grouped_bf16(arr, len(probs), st()), "obte_gemm_grouped_bf16")
        return outs
    want, _ = both(case)
    for i, ((lay, M, N, K, acc), (_, _, ref, r)) in enumerate(zip(probs, data)):
        close(want[f"d{i}"], (r.float() + ref.to(BF).float()) if acc else ref, atol=0.01 * math.sqrt(K) + 0.03, what=f"grouped problem {i}")


# ==================================================================================================== attention
def _tokens(B, T):
    tok = np.random.default_rng(T).integers(20, 100, size=(B, T))
    tok[0, [(T // 3) % T, (T // 2) % T]] = R.EOS_TOKEN
    tok[1, [5 % T, (T - 10) % T]] = R.EOS_TOKEN
    return tok


@functools.lru_cache(maxsize=None)
def _attn_inputs(hs, T, mode):
    """qkv, d_o, the mask tables of `mode` and the oracle's o, lse, dqkv for B = 2, H = 2 (computed once, never modified)"""
    B, H = 2, 2
    Cc = H * hs
    scale = 8.0 / Cc
    qkv, d_o = rnd(B, T, 3 * Cc, seed=hs + T), rnd(B, T, Cc, seed=99)
    q, k, v = [t.reshape(B, T, H, hs).transpose(1, 2).float().requires_grad_(True) for t in qkv.split(Cc, dim=2)]
    dense, ranges = _blocks_to_masks(_tokens(B, T), T)
    mask_add = None
    if mode in ("ranges", "dense", "dense_exact"):
        mask_add = dense.unsqueeze(1)
    elif mode == "causal":
        mask_add = torch.where(torch.tril(torch.ones(T, T, dtype=torch.bool)), 0.0, R.MASKED_VALUE).view(1, 1, T, T)
    ref = R.attention(q, k, v, scale, mask_add)
    ref.backward(d_o.reshape(B, T, H, hs).transpose(1, 2).float())
    att = (q.detach() @ k.detach().transpose(-2, -1)) * scale
    if mask_add is not None:
        att = att + mask_add
    dref = torch.cat([g.grad.transpose(1, 2).reshape(B, T, Cc) for g in (q, k, v)], dim=2)
    tab = torch.randn(T, hs // 2, generator=torch.Generator().manual_seed(1))
    return dict(qkv=qkv, d_o=d_o, ranges=ranges.to(I32), dense=dense.to(BF).unsqueeze(1).contiguous(), scale=scale, cos=torch.cos(tab), sin=torch.sin(tab),
                o=ref.detach().transpose(1, 2).reshape(B, T, Cc), lse=torch.logsumexp(att, dim=-1), dqkv=dref)


def _attn_case(c, B, T, H, hs, mode, p=0.0):
    """forward, then the backward as the kernel pair (plain and with the inverse RoPE) and, where it applies, as one kernel"""
    Lm = L()
    Cc = H * hs
    one_kernel = hs == 128 and mode not in ("dense", "dense_exact")

    def case(A):
        qkv, d_o = A.inp(c["qkv"][:B]), A.inp(c["d_o"][:B])
        kr = qb = mask = exact = None
        sb = sh = sq = 0
        if mode == "ranges":
            kr = A.inp(c["ranges"][:B])
        elif mode == "causal":
            kr, qb = A.out((B, T, 2), I32), A.out((B, T, 2), I32)
            chk(lib().obte_causal_bounds(None, B, T, ptr(kr), ptr(qb), st()), "obte_causal_bounds")
        elif mode in ("dense", "dense_exact"):
            mask = A.inp(c["dense"][:B])                                  # [B, 1, T, T]: the reference's expand() view, head stride 0
            sb, sh, sq = T * T, 0, T
            kr, qb, flag = A.out((B, T, 2), I32), A.out((B, T, 2), I32), A.out((1,), I32)
            rows, cols = A.out((B * T,), U8), A.out((B * T,), I32)
            chk(lib().obte_mask_bounds(ptr(mask), sb, sh, sq, B, H, T, ptr(kr), ptr(qb), ptr(rows), ptr(flag), ptr(cols), st()), "obte_mask_bounds")
            exact = flag if mode == "dense_exact" else None
        o, lse = A.out((B, T, Cc)), A.out((B, H, T), F32)
        bits = None
        if p > 0.0:
            bits = A.out((int(lib().obte_attn_drop_bits_bytes(B, T, H)) // 4,), I32, fill=0)
        fa = Lm.AttnFwdArgs(ptr(qkv), ptr(o), ptr(lse), ptr(kr), ptr(mask), sb, sh, sq, B, T, H, hs, c["scale"], p, SEED, ptr(exact), ptr(bits))
        chk(lib().obte_attn_fwd(C.byref(fa), st()), "obte_attn_fwd")
        outs = dict(o=o, lse=lse)
        if bits is not None:
            outs["bits"] = bits
        o_in, lse_in = A.inp(o), A.inp(lse)                               # the forward's results as the backward's inputs, behind NaN
        cos, sin = A.inp(c["cos"]), A.inp(c["sin"])
        forms = [("pair", False, False, None), ("pair_rope", False, True, None)]
        if p > 0.0:
            forms = [("pair", False, False, None), ("pair_bits", False, False, bits)]
        if one_kernel:
            forms += [("one", True, False, bits), ("one_rope", True, True, bits)]
        for name, one, rope, use_bits in forms:
            delta, dqkv = A.out((B, H, T), F32), A.out((B, T, 3 * Cc))
            ws_bytes = int(lib().obte_attn_bwd_ws_bytes(B, T, H, hs)) if one else 0
            ws = torch.empty(ws_bytes, dtype=U8, device=DEV) if ws_bytes > 0 else None      # the hand-off scratch: allocated as ops.attn_bwd does
            ba = Lm.AttnBwdArgs(ptr(qkv), ptr(o_in), ptr(d_o), ptr(lse_in), ptr(delta), ptr(dqkv), ptr(cos) if rope else None, ptr(sin) if rope else None,
                                ptr(kr), ptr(mask), sb, sh, sq, B, T, H, hs, c["scale"], p, SEED, ptr(qb), ptr(exact), ptr(ws), ws_bytes, ptr(use_bits))
            chk(lib().obte_attn_bwd(C.byref(ba), st()), "obte_attn_bwd")
            outs["dqkv_" + name], outs["delta_" + name] = dqkv, delta
        return outs
    return case


def _attn_check(hs, T, mode, p=0.0):
    B, H = 2, 2
    c = _attn_inputs(hs, T, mode if mode != "dense_exact" else "dense")
    want, got = both(_attn_case(c, B, T, H, hs, mode, p))
    # batch independence: element 0 alone, with poison directly behind its last row
    alone = Fenced()
    one = _attn_case(c, 1, T, H, hs, mode, p)(alone)
    torch.cuda.synchronize()
    assert_guards(*alone.handles)
    for k in want:
        if k.startswith("dqkv") or k in ("o", "lse"):
            assert_same_bits(one[k][0], got[k][0], f"{k}: batch element 0 alone vs inside B = 2")
    return c, want


@pytest.mark.parametrize("mode", ["none", "ranges", "dense", "dense_exact", "causal"])
@pytest.mark.parametrize("T", [1, 33, 77, 257, 333, 600])
@pytest.mark.parametrize("hs", [64, 128])
def test_attention_fenced(hs, T, mode):
    c, want = _attn_check(hs, T, mode)
    close(want["o"], c["o"], atol=6e-3, what=f"attn fwd {mode}")
    close(want["lse"], c["lse"], atol=2e-3, rtol=1e-3, what="lse")
    for k in ("dqkv_pair", "dqkv_one"):
        if k in want:
            close(want[k], c["dqkv"], atol=1.5e-2, rtol=2.0 ** -6, what=f"attn bwd {mode} {k}")


@pytest.mark.parametrize("hs", [64, 128])
def test_attention_dropout_fenced(hs):
    """p = 0.1 at T = 333 under key ranges: the keep bits zero-filled inside their fence; the backward hashed and from the bits"""
    c, want = _attn_check(hs, 333, "ranges", p=0.1)
    assert_same_bits(want["dqkv_pair_bits"], want["dqkv_pair"], "backward from the keep bits vs hashed")
    assert bool((want["bits"] != 0).any().item()) == (hs == 128)         # head size 64 writes no keep bits


# ==================================================================================================== LayerNorm
@functools.lru_cache(maxsize=None)
def _ln_data(rows, cols):
    x, w = rnd(rows, cols, seed=1, scale=2.0), (1 + 0.3 * rnd(cols, seed=2).float()).to(BF)
    return x, w, rnd(rows, cols, seed=3), rnd(rows, cols, seed=4), rnd(cols, seed=5)


@pytest.mark.parametrize("cols", [8, 136, 1024, 1032, 2560, 4088, 4096])
@pytest.mark.parametrize("rows", [1, 5, 37, 1029])
def test_layernorm_fenced(rows, cols):
    """forward; backward plain, accumulating with the residual gradient, through fp32 partials (FIRST then LAST) and with the dropped
    second output.  cols 2560, 4088 and 4096 are the eight-chunk instantiations: also against the oracle."""
    x, w, dy, dres, old = _ln_data(rows, cols)
    Lm = L()
    ws_rows = lib().obte_layernorm_bwd_ws_rows()
    p, site = 0.1, 2

    def case(A):
        xd, wd, dyd, dresd = A.inp(x), A.inp(w), A.inp(dy), A.inp(dres)
        y, mean, rstd = A.out((rows, cols)), A.out((rows,), F32), A.out((rows,), F32)
        chk(lib().obte_layernorm_fwd(ptr(xd), ptr(wd), ptr(y), ptr(mean), ptr(rstd), rows, cols, 1e-5, st()), "obte_layernorm_fwd")
        mi, ri = A.inp(mean), A.inp(rstd)
        outs = dict(y=y, mean=mean, rstd=rstd)
        dx, dw, ws = A.out((rows, cols)), A.out((cols,)), A.scratch((ws_rows * cols,))
        chk(lib().obte_layernorm_bwd(ptr(dyd), ptr(xd), ptr(wd), ptr(mi), ptr(ri), None, ptr(dx), ptr(dw), ptr(ws), rows, cols, st()), "obte_layernorm_bwd")
        outs.update(dx=dx, dw=dw)
        dx, dw, ws = A.out((rows, cols)), A.inp(old), A.scratch((ws_rows * cols,))
        chk(lib().obte_layernorm_bwd_acc(ptr(dyd), ptr(xd), ptr(wd), ptr(mi), ptr(ri), ptr(dresd), ptr(dx), ptr(dw), ptr(ws), rows, cols, 1, st()),
            "obte_layernorm_bwd_acc")
        outs.update(dx_acc=dx, dw_acc=dw)
        part, dw = A.out((ws_rows * cols,), F32), A.out((cols,))
        for mode in (Lm.LN_PARTIAL_FIRST, Lm.LN_PARTIAL_LAST):
            dx = A.out((rows, cols))
            chk(lib().obte_layernorm_bwd_partial(ptr(dyd), ptr(xd), ptr(wd), ptr(mi), ptr(ri), ptr(dresd), ptr(dx), ptr(dw) if mode == Lm.LN_PARTIAL_LAST else None,
                                                 ptr(part), rows, cols, mode, st()), "obte_layernorm_bwd_partial")
            outs[f"dx_partial{mode}"] = dx
        outs.update(partials=part, dw_partial=dw)
        dx, dxd, dw, ws = A.out((rows, cols)), A.out((rows, cols)), A.out((cols,)), A.scratch((ws_rows * cols,))
        chk(lib().obte_layernorm_bwd_dropout(ptr(dyd), ptr(xd), ptr(wd), ptr(mi), ptr(ri), ptr(dresd), ptr(dx), ptr(dxd), ptr(dw), ptr(ws), rows, cols, 0, 0,
                                             p, SEED, site, st()), "obte_layernorm_bwd_dropout")
        outs.update(dx_drop=dx, dxd=dxd, dw_drop=dw)
        return outs
    want, _ = both(case)
    assert_same_bits(want["dx_drop"], want["dx_acc"], "dx with and without the dropped output")
    assert_same_bits(want[f"dx_partial{Lm.LN_PARTIAL_LAST}"], want["dx_acc"], "dx in partial mode")
    assert torch.equal(want["dw_acc"].cpu(), (old.float() + want["dw_drop"].cpu().float()).to(BF))
    if cols >= 2560:
        xf, wf = x.float().requires_grad_(True), w.float().requires_grad_(True)
        yref = R.layer_norm(xf, wf)
        yref.backward(dy.float())
        close(want["y"], yref, atol=2e-3, what="ln fwd")
        close(want["mean"], x.float().mean(1), atol=1e-5, rtol=1e-5, what="ln mean")
        close(want["dx"], xf.grad, atol=4e-3, what="ln dx")
        close(want["dw"], wf.grad, atol=0.02 * math.sqrt(rows), what="ln dw")
        close(want["dx_acc"], xf.grad + dres.float(), atol=8e-3, what="ln dx+resid")


# ==================================================================================================== masked CE
@functools.lru_cache(maxsize=None)
def _ce_data(vocab, n):
    M = n + 15
    logits = rnd(M, vocab, seed=3, scale=2.0)
    tgt = torch.from_numpy(np.random.default_rng(3).integers(0, vocab, size=M))
    tgt[0], tgt[1] = 0, vocab - 1
    rows = torch.from_numpy(np.sort(np.random.default_rng(4).choice(M, size=n, replace=False))).to(I64)
    lf = logits[rows].float().requires_grad_(True)
    ref = R.masked_lm_loss(lf, tgt[rows], torch.ones(n, dtype=torch.bool), 4)
    ref.backward()
    return logits, tgt, rows, ref.detach(), lf.grad


@pytest.mark.parametrize("vocab,n", [(8, 9), (16384, 9), (16392, 9), (65536, 9), (65544, 9), (65536, 257)])
def test_masked_ce_fenced(vocab, n):
    """the two register kernels on both sides of their boundary, the two-pass kernel, and (257 rows of 65 536) the persistent LDS-DMA
    kernel: with and without a row list, with and without per-row weights; the dense forms with a mask and a previous mask"""
    logits, tgt, rows, ref_loss, ref_grad = _ce_data(vocab, n)
    M, n_accum = logits.shape[0], 4
    weights = torch.full((n,), 1.0 / n)
    mask = torch.zeros(M, dtype=U8)
    mask[rows] = 1
    prev = torch.zeros(M, dtype=U8)
    prev[::2] = 1

    def case(A):
        lg, tg, rw, wv = A.inp(logits), A.inp(tgt), A.inp(rows), A.inp(weights)
        lg_c, tg_c = A.inp(logits[rows]), A.inp(tgt[rows])
        outs = {}
        for name, lgx, tgx, rwx, wvx, total in (("list", lg, tg, rw, None, M), ("list_w", lg, tg, rw, wv, M), ("compact", lg_c, tg_c, None, None, n),
                                                ("compact_w", lg_c, tg_c, None, wv, n)):
            loss, dl = A.out((n,), F32), A.out((n, vocab))
            scale = (1.0 if wvx is not None else 1.0 / n) / n_accum
            chk(lib().obte_masked_ce_rows(ptr(lgx), ptr(tgx), ptr(rwx), None, scale, ptr(wvx), ptr(loss), ptr(dl), n, total, vocab, st()), "obte_masked_ce_rows")
            outs["loss_" + name], outs["dl_" + name] = loss, dl
        mk, pv, gs = A.inp(mask), A.inp(prev), A.inp(torch.tensor([1.0 / n]))
        loss, dl = A.out((M,), F32), A.out((M, vocab))
        chk(lib().obte_masked_ce_fwd_bwd(ptr(lg), ptr(tg), ptr(mk), ptr(gs), 1.0 / n_accum, None, ptr(loss), ptr(dl), M, vocab, st()), "obte_masked_ce_fwd_bwd")
        outs.update(loss_dense=loss, dl_dense=dl)
        loss, dl = A.out((M,), F32), A.out((M, vocab), fill=0)
        chk(lib().obte_masked_ce_fwd_bwd_reuse(ptr(lg), ptr(tg), ptr(mk), ptr(pv), ptr(gs), 1.0 / n_accum, ptr(loss), ptr(dl), M, vocab, st()),
            "obte_masked_ce_fwd_bwd_reuse")
        outs.update(loss_reuse=loss, dl_reuse=dl)
        return outs
    want, _ = both(case)
    for name in ("list", "list_w", "compact", "compact_w"):
        loss = want["loss_" + name].sum().item()
        assert abs(loss - ref_loss.item()) <= 1e-4 * abs(ref_loss.item()) + 1e-6, (name, loss, ref_loss.item())
        close(want["dl_" + name], ref_grad, atol=2e-7, rtol=2.0 ** -7, what="dlogits " + name)
    assert_same_bits(want["dl_compact"], want["dl_list"], "with and without a row list")
    dense = torch.zeros(M, vocab)
    dense[rows] = ref_grad
    close(want["dl_dense"], dense, atol=2e-7, rtol=2.0 ** -7, what="dlogits dense")
    keep = (mask == 0) & (prev == 0)                       # rows unmasked then and now are not touched
    assert torch.equal(want["dl_reuse"].cpu()[~keep], want["dl_dense"].cpu()[~keep]) and (want["dl_reuse"].cpu()[keep] == 0).all()


# ==================================================================================== embedding, dropout, rows, RoPE
@pytest.mark.parametrize("vocab", [64, 512])
@pytest.mark.parametrize("cols", [8, 128])
@pytest.mark.parametrize("rows", [1, 33, 1000])
def test_embedding_fenced(rows, cols, vocab):
    rng = np.random.default_rng(rows + cols)
    idx = rng.integers(0, vocab, size=rows)
    idx[rng.random(rows) < 0.3] = 2                       # one id repeated over many 32-row chunks
    idx = torch.from_numpy(idx)
    order = torch.sort(idx, stable=True).indices.to(I32)
    wte, dout, old = rnd(vocab, cols, seed=1), rnd(rows, cols, seed=2), rnd(vocab, cols, seed=3)
    Lm = L()
    ws_elems = max(int(lib().obte_embedding_bwd_ws_bytes(rows, cols)), 16) // 4
    p = 0.1

    def case(A):
        ix, od, wt, do_ = A.inp(idx), A.inp(order), A.inp(wte), A.inp(dout)
        outs = {}
        out = A.out((rows, cols))
        chk(lib().obte_embedding_fwd(ptr(ix), ptr(wt), ptr(out), rows, cols, vocab, st()), "obte_embedding_fwd")
        outs["fwd"] = out
        out = A.out((rows, cols))
        chk(lib().obte_embedding_fwd_dropout(ptr(ix), ptr(wt), ptr(out), rows, cols, vocab, p, SEED, st()), "obte_embedding_fwd_dropout")
        outs["fwd_drop"] = out
        dw, ws = A.out((vocab, cols)), A.scratch((ws_elems,))
        chk(lib().obte_embedding_bwd(ptr(ix), ptr(od), ptr(do_), ptr(dw), ptr(ws), rows, cols, vocab, st()), "obte_embedding_bwd")
        outs["bwd"] = dw
        dw, ws = A.inp(old), A.scratch((ws_elems,))
        chk(lib().obte_embedding_bwd_acc(ptr(ix), ptr(od), ptr(do_), ptr(dw), ptr(ws), rows, cols, vocab, 1, st()), "obte_embedding_bwd_acc")
        outs["bwd_acc"] = dw
        dw, ws = A.out((vocab, cols)), A.scratch((ws_elems,))
        chk(lib().obte_embedding_bwd_dropout(ptr(ix), ptr(od), ptr(do_), ptr(dw), ptr(ws), rows, cols, vocab, 0, p, SEED, st()), "obte_embedding_bwd_dropout")
        outs["bwd_drop"] = dw
        acc, dw = A.out((vocab, cols), F32), A.out((vocab, cols))
        for mode in (Lm.ACC32_FIRST, Lm.ACC32_LAST):
            ws = A.scratch((ws_elems,))
            chk(lib().obte_embedding_bwd_acc32(ptr(ix), ptr(od), ptr(do_), ptr(acc), ptr(dw) if mode == Lm.ACC32_LAST else None, ptr(ws), rows, cols, vocab, mode,
                                               0.0, 0, st()), "obte_embedding_bwd_acc32")
        outs.update(acc32=acc, bwd_acc32=dw)
        return outs
    want, _ = both(case)
    assert torch.equal(want["fwd"].cpu(), wte[idx])
    ref = torch.zeros(vocab, cols).index_add_(0, idx, dout.float())
    close(want["bwd"], ref, atol=2e-2, what="embedding bwd")
    assert torch.equal(want["bwd_acc"].cpu(), (old.float() + want["bwd"].cpu().float()).to(BF))
    assert torch.equal(want["bwd_acc32"], want["acc32"].to(BF))
    close(want["bwd_acc32"], 2.0 * ref, atol=4e-2, what="embedding bwd, two passes summed in fp32")


@pytest.mark.parametrize("rows,cols", [(1, 8), (33, 136), (1000, 128)])
def test_dropout_rows_and_accumulate_fenced(rows, cols):
    """obte_dropout_bf16 (out of place and in place), obte_rows_gather_bf16 / _scatter_bf16, obte_acc32_add_bf16 FIRST / MORE / LAST"""
    x, y = rnd(rows, cols, seed=1), rnd(rows, cols, seed=2)
    total = rows + 7
    sel = torch.from_numpy(np.sort(np.random.default_rng(rows).choice(total, size=rows, replace=False))).to(I64)
    big = rnd(total, cols, seed=3)
    Lm = L()

    def case(A):
        xd = A.inp(x)
        out = A.out((rows, cols))
        chk(lib().obte_dropout_bf16(ptr(xd), ptr(out), rows * cols, cols, 0.1, SEED, 7, st()), "obte_dropout_bf16")
        inplace = A.inp(x)
        chk(lib().obte_dropout_bf16(ptr(inplace), ptr(inplace), rows * cols, cols, 0.1, SEED, 7, st()), "obte_dropout_bf16")
        sd, bd = A.inp(sel), A.inp(big)
        gathered, scattered = A.out((rows, cols)), A.out((total, cols))
        chk(lib().obte_rows_gather_bf16(ptr(bd), ptr(sd), ptr(gathered), rows, total, cols, st()), "obte_rows_gather_bf16")
        chk(lib().obte_rows_scatter_bf16(ptr(xd), ptr(sd), ptr(scattered), rows, total, cols, st()), "obte_rows_scatter_bf16")
        acc, yd, o16 = A.out((rows * cols,), F32), A.inp(y), A.out((rows, cols))
        chk(lib().obte_acc32_add_bf16(ptr(acc), ptr(xd), None, rows * cols, Lm.ACC32_FIRST, st()), "obte_acc32_add_bf16")
        chk(lib().obte_acc32_add_bf16(ptr(acc), ptr(yd), None, rows * cols, Lm.ACC32_MORE, st()), "obte_acc32_add_bf16")
        chk(lib().obte_acc32_add_bf16(ptr(acc), ptr(xd), ptr(o16), rows * cols, Lm.ACC32_LAST, st()), "obte_acc32_add_bf16")
        return dict(out=out, inplace=inplace, gathered=gathered, scattered=scattered, acc=acc, o16=o16)
    want, _ = both(case)
    assert_same_bits(want["inplace"], want["out"], "dropout in place")
    assert torch.equal(want["gathered"].cpu(), big[sel])
    ref = torch.zeros(total, cols, dtype=BF)
    ref[sel] = x
    assert torch.equal(want["scattered"].cpu(), ref)
    assert torch.equal(want["acc"].cpu(), (x.float() + y.float() + x.float()).reshape(-1))


@pytest.mark.parametrize("hs", [64, 128])
def test_rope_fenced(hs):
    B, T, H = 2, 37, 2
    Cc = H * hs
    qkv = rnd(B, T, 3 * Cc, seed=5)
    tab = torch.randn(T, hs // 2, generator=torch.Generator().manual_seed(2))

    def case(A):
        cos, sin = A.inp(torch.cos(tab)), A.inp(torch.sin(tab))
        fwd, inv = A.inp(qkv), A.inp(qkv)
        chk(lib().obte_rope_qk_inplace(ptr(fwd), ptr(cos), ptr(sin), B, T, H, hs, 0, st()), "obte_rope_qk_inplace")
        chk(lib().obte_rope_qk_inplace(ptr(inv), ptr(cos), ptr(sin), B, T, H, hs, 1, st()), "obte_rope_qk_inplace")
        return dict(fwd=fwd, inv=inv)
    want, _ = both(case)
    assert torch.equal(want["fwd"].cpu()[..., 2 * Cc:], qkv[..., 2 * Cc:]) and torch.equal(want["inv"].cpu()[..., 2 * Cc:], qkv[..., 2 * Cc:])
    assert not torch.equal(want["fwd"].cpu()[..., :2 * Cc], qkv[..., :2 * Cc])


# ==================================================================================================== optimizer
SIZES = (8, 4104, 65544)


def _opt_data():
    return [dict(p=rnd(n, seed=10 + i), g=rnd(n, seed=20 + i, scale=0.1), m=rnd(n, seed=30 + i, scale=0.01),
                 v=(rnd(n, seed=40 + i, scale=0.01).float() ** 2).to(BF)) for i, n in enumerate(SIZES)]


def _mt(A, data, state=True):
    t = L().MtArgs()
    held = []
    for i, d in enumerate(data):
        for f in ("p", "g", "m", "v") if state else ("g",):
            x = A.inp(d[f])
            held.append(x)
            getattr(t, f)[i] = x.data_ptr()
        t.n[i], t.lr[i], t.weight_decay[i], t.step[i] = d["g"].numel(), 1e-2, 1e-2, 3
    t.count = len(data)
    return t, held


def test_adamw_fenced():
    """obte_adamw_bf16 per tensor and the three multi-tensor steps over tensors of 8, 4104 and 65544 elements, each tensor in a fence of its own"""
    data = _opt_data()
    hyper = (1e-2, 0.9, 0.999, 1e-8, 1e-2)

    def case(A):
        outs = {}
        clip = A.inp(torch.tensor([0.5]))
        for i, d in enumerate(data):
            p, g, m, v = (A.inp(d[f]) for f in ("p", "g", "m", "v"))
            chk(lib().obte_adamw_bf16(ptr(p), ptr(g), ptr(m), ptr(v), p.numel(), *hyper, 3, ptr(clip), st()), "obte_adamw_bf16")
            outs.update({f"single_p{i}": p, f"single_m{i}": m, f"single_v{i}": v})
        t, held = _mt(A, data)
        chk(lib().obte_adamw_multi_bf16(C.byref(t), 0.9, 0.999, 1e-8, ptr(clip), st()), "obte_adamw_multi_bf16")
        outs.update({f"multi{j}": x for j, x in enumerate(held)})
        t, held = _mt(A, data)
        chk(lib().obte_adamw_multi_bf16_ref(C.byref(t), 0.9, 0.999, 1e-8, ptr(clip), st()), "obte_adamw_multi_bf16_ref")
        outs.update({f"ref{j}": x for j, x in enumerate(held)})
        tm = L().MtMasterArgs()
        for i, d in enumerate(data):
            p, g = A.out((d["p"].numel(),)), A.inp(d["g"])
            w, m, v = A.inp(d["p"].float()), A.inp(d["m"].float()), A.inp(d["v"].float())
            tm.p[i], tm.g[i], tm.master[i], tm.m[i], tm.v[i] = (x.data_ptr() for x in (p, g, w, m, v))
            tm.n[i], tm.lr[i], tm.weight_decay[i], tm.step[i] = p.numel(), 1e-2, 1e-2, 3
            outs.update({f"master_p{i}": p, f"master_w{i}": w, f"master_m{i}": m, f"master_v{i}": v, f"master_g{i}": g})
        tm.count = len(data)
        chk(lib().obte_adamw_multi_master(C.byref(tm), 0.9, 0.999, 1e-8, ptr(clip), st()), "obte_adamw_multi_master")
        return outs
    want, _ = both(case)
    for i in range(len(SIZES)):                           # the multi-tensor kernel is the single-tensor kernel (p, g, m, v per tensor)
        assert_same_bits(want[f"multi{4 * i}"], want[f"single_p{i}"], "multi vs single p")
        assert_same_bits(want[f"multi{4 * i + 2}"], want[f"single_m{i}"], "multi vs single m")
        assert torch.equal(want[f"master_p{i}"], want[f"master_w{i}"].to(BF))


def test_sumsq_and_clip_coefficient_fenced():
    """The fixed-order partials and the coefficient: bitwise.  The three atomic sums (documented as order-dependent in the last fp32
    bits): the relative bar test_adamw_matches_fp32_formula uses for the sum."""
    data = _opt_data()
    exact = [(d["g"].float() ** 2).sum().item() for d in data]

    def case(A):
        t, _ = _mt(A, data, state=False)
        n_part = int(lib().obte_sumsq_multi_partials_count(C.byref(t)))
        assert n_part == sum((n + 16383) // 16384 for n in SIZES)
        partials, coef = A.out((n_part,), F32), A.out((2,), F32)
        chk(lib().obte_sumsq_multi_bf16_partials(C.byref(t), ptr(partials), st()), "obte_sumsq_multi_bf16_partials")
        pin = A.inp(partials)
        chk(lib().obte_clip_coef_from_partials(ptr(pin), n_part, 1.0, ptr(coef), st()), "obte_clip_coef_from_partials")
        one, all_, each = A.inp(torch.zeros(1)), A.inp(torch.zeros(1)), A.inp(torch.zeros(len(data)))
        g2 = A.inp(data[2]["g"])
        chk(lib().obte_sumsq_bf16(ptr(g2), g2.numel(), ptr(one), st()), "obte_sumsq_bf16")
        chk(lib().obte_sumsq_multi_bf16(C.byref(t), ptr(all_), st()), "obte_sumsq_multi_bf16")
        chk(lib().obte_sumsq_multi_bf16_each(C.byref(t), ptr(each), st()), "obte_sumsq_multi_bf16_each")
        return dict(partials=partials, coef=coef, one=one, all=all_, each=each)
    want, got = both(case, loose=("one", "all", "each"))
    for outs in (want, got):
        assert abs(outs["one"].item() - exact[2]) <= 1e-4 * outs["one"].item()
        assert abs(outs["all"].item() - sum(exact)) <= 1e-4 * outs["all"].item()
        for i, e in enumerate(exact):
            assert abs(outs["each"][i].item() - e) <= 1e-4 * outs["each"][i].item()
    assert abs(want["coef"][0].item() - sum(exact)) <= 1e-4 * sum(exact)
    assert abs(want["coef"][1].item() - min(1.0, 1.0 / (math.sqrt(sum(exact)) + 1e-6))) <= 1e-4


# ============================================================================================== integer prelude
@pytest.mark.parametrize("T", [1, 65, 1000])
def test_prelude_fenced(T):
    """key ranges from token ids, the causal pair with and without document ranges, the embedding sort order (two and three radix passes,
    the workspace full of NaN behind a 256-byte front guard: its documented alignment), and the bounds of a dense mask"""
    B, H = 3, 2
    ids = torch.from_numpy(np.random.default_rng(T).integers(0, 500, size=(B, T)).astype(np.int64))
    ids[:, ::7] = 3
    wide = torch.from_numpy(np.random.default_rng(T + 1).integers(0, 70000, size=(B, T)).astype(np.int64))
    blocks = R.document_blocks(ids.numpy())
    dense = R.dense_mask_from_blocks(blocks, T).to(BF).unsqueeze(1).contiguous()

    def case(A):
        outs = {}
        idd = A.inp(ids)
        for padding in (0, 1):
            kr = A.out((B, T, 2), I32)
            chk(lib().obte_key_ranges_from_tokens(ptr(idd), B, T, 3, padding, 0, ptr(kr), st()), "obte_key_ranges_from_tokens")
            outs[f"kr{padding}"] = kr
        doc = A.inp(outs["kr0"])
        for name, d in (("doc", doc), ("plain", None)):
            kr, qb = A.out((B, T, 2), I32), A.out((B, T, 2), I32)
            chk(lib().obte_causal_bounds(ptr(d), B, T, ptr(kr), ptr(qb), st()), "obte_causal_bounds")
            outs["ckr_" + name], outs["cqb_" + name] = kr, qb
        for name, src, vocab in (("order2", idd, 500), ("order3", A.inp(wide), 70000)):
            order = A.out((B, T), I32)
            ws = A.scratch((int(lib().obte_token_order_ws_bytes(B, T, vocab)) // 4,), F32, front_bytes=256)
            chk(lib().obte_token_order(ptr(src), B, T, vocab, ptr(order), ptr(ws), st()), "obte_token_order")
            outs[name] = order
        mask = A.inp(dense)
        kb, qb, flag = A.out((B, T, 2), I32), A.out((B, T, 2), I32), A.out((1,), I32)
        rows, cols = A.out((B * T,), U8), A.out((B * T,), I32)
        chk(lib().obte_mask_bounds(ptr(mask), T * T, 0, T, B, H, T, ptr(kb), ptr(qb), ptr(rows), ptr(flag), ptr(cols), st()), "obte_mask_bounds")
        outs.update(kb=kb, mqb=qb, flag=flag)
        return outs
    want, _ = both(case)
    assert torch.equal(want["order2"].cpu(), torch.sort(ids, dim=1, stable=True).indices.to(I32))
    assert torch.equal(want["order3"].cpu(), torch.sort(wide, dim=1, stable=True).indices.to(I32))
    assert want["flag"].item() == 1
    t = torch.arange(T, dtype=I32)
    assert torch.equal(want["ckr_plain"].cpu()[0], torch.stack([torch.zeros_like(t), t + 1], dim=1))
