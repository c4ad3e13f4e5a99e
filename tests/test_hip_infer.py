"""GPU tests of the forward-only block path: the activation-only GELU epilogue (OBTE_EPI_GELU_ACT) against the two-output one,
obte_block_fwd_infer against obte_block_fwd, and the model's choice between the two.  Every comparison is bitwise: the path
that keeps nothing for a backward runs the same kernels on the same values, so any difference is a bug, not rounding."""
import ctypes
import warnings

import numpy as np
import pytest
import torch

import omnibiote_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16


def ops():
    from omnibiote_amd import ops as o
    return o


def L():
    from omnibiote_amd import _lib
    return _lib


def collect_kinds():
    cap = 64
    ms = np.zeros(cap, dtype=np.float64)
    dims = np.zeros(3 * cap, dtype=np.int64)
    kind = np.zeros(cap, dtype=np.int32)
    n = L().lib().obte_profile_collect(ms.ctypes.data_as(ctypes.c_void_p), dims.ctypes.data_as(ctypes.c_void_p),
                                       kind.ctypes.data_as(ctypes.c_void_p), cap)
    return [int(k) for k in kind[:n]]


# ---------------------------------------------------------------------------------------------------------------- 1. the epilogue
# structure / width / (M, N, K): ragged edges in both directions on the structures that take them; whole tiles, one per CU, for 7
GEMM_CASES = [(1, 128, (300, 384, 192)), (2, 128, (300, 384, 192)), (2, 192, (300, 384, 192)), (2, 256, (300, 384, 192)),
              (3, 256, (300, 384, 192)), (4, 128, (300, 384, 192)), (7, 256, (4096, 4096, 256))]


@pytest.mark.parametrize("structure,width,shape", GEMM_CASES, ids=[f"s{s}w{w}" for s, w, _ in GEMM_CASES])
def test_gelu_act_is_the_activation_of_the_two_output_epilogue_bit_for_bit(structure, width, shape):
    M, N, K = shape
    Lm, lib = L(), L().lib()
    g = torch.Generator(device=DEV).manual_seed(1000 * structure + width)
    x = torch.randn(M, K, device=DEV, generator=g).to(BF)
    w = (torch.randn(N, K, device=DEV, generator=g) * (2.0 / K ** 0.5)).to(BF)     # acc ~ N(0, 2^2): |acc| from 0 past 6, both tails of the erf fit
    acc = (x.float() @ w.float().t()).abs()
    assert acc.max().item() >= 6.0 and acc.min().item() <= 0.05
    try:
        for epi in (Lm.EPI_GELU, Lm.EPI_GELU_ACT):
            Lm.check(lib.obte_gemm_plan_set(1, 1, epi, M, N, K, structure, width, 1), "obte_gemm_plan_set")
        lib.obte_profile_enable(1)
        collect_kinds()                                   # (records an earlier user may have left)
        try:
            _, act2 = ops().linear_fwd(x, w, epilogue=Lm.EPI_GELU)
            act1 = ops().linear_fwd(x, w, epilogue=Lm.EPI_GELU_ACT)
            torch.cuda.synchronize()
            kinds = collect_kinds()
        finally:
            lib.obte_profile_enable(0)
    finally:
        Lm.check(lib.obte_gemm_plan_clear(), "obte_gemm_plan_clear")
    # both launches on the structure asked for: a resolver fallback must not make this compare a structure with itself
    assert kinds == [1000 * structure + 12 + Lm.EPI_GELU, 1000 * structure + 12 + Lm.EPI_GELU_ACT], kinds
    assert torch.equal(act1, act2)
    ref = R.gelu_erf((x.float() @ w.float().t()).to(BF).float())
    # (and it is a GELU at all: one bf16 ulp below 16 is 0.0625, for an accumulator that rounds the other way than torch's product)
    assert (act1.float() - ref).abs().max().item() <= 0.0625 + 1e-3


def test_gelu_act_without_a_plan_of_its_own_takes_the_gelu_plan():
    M, N, K = 300, 384, 192
    Lm, lib = L(), L().lib()
    g = torch.Generator(device=DEV).manual_seed(5)
    x = torch.randn(M, K, device=DEV, generator=g).to(BF)
    w = (torch.randn(N, K, device=DEV, generator=g) * 0.1).to(BF)
    try:
        Lm.check(lib.obte_gemm_plan_set(1, 1, Lm.EPI_GELU, M, N, K, 4, 128, 1), "obte_gemm_plan_set")
        lib.obte_profile_enable(1)
        collect_kinds()
        try:
            a = ops().linear_fwd(x, w, epilogue=Lm.EPI_GELU_ACT)
            Lm.check(lib.obte_gemm_plan_set(1, 1, Lm.EPI_GELU_ACT, M, N, K, 1, 128, 1), "obte_gemm_plan_set")
            b = ops().linear_fwd(x, w, epilogue=Lm.EPI_GELU_ACT)
            torch.cuda.synchronize()
            kinds = collect_kinds()
        finally:
            lib.obte_profile_enable(0)
    finally:
        Lm.check(lib.obte_gemm_plan_clear(), "obte_gemm_plan_clear")
    assert [k // 1000 for k in kinds] == [4, 1], kinds
    assert torch.equal(a, b)


def test_gelu_act_is_refused_outside_its_layout():
    x = torch.zeros(256, 128, device=DEV, dtype=BF)
    w = torch.zeros(128, 256, device=DEV, dtype=BF)
    Lm = L()
    d = torch.empty(256, 256, device=DEV, dtype=BF)
    g = Lm.GemmArgs(x.data_ptr(), w.data_ptr(), d.data_ptr(), None, None, 256, 256, 128, 128, 256, 256, 1, 0, Lm.EPI_GELU_ACT, 1.0, 0.0, 0, 0)
    assert Lm.lib().obte_gemm_bf16(ctypes.byref(g), None) == -1
    assert "EPI_GELU_ACT" in Lm.lib().obte_last_error().decode()


# ------------------------------------------------------------------------------------------------------------------- 2. the block
def block_params(C, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    rn = lambda *s, scale=1.0: torch.randn(*s, device=DEV, generator=g) * scale
    return ((1.0 + rn(C, scale=0.1)).to(BF), rn(3 * C, C, scale=C ** -0.5).to(BF), rn(C, C, scale=C ** -0.5).to(BF),
            (1.0 + rn(C, scale=0.1)).to(BF), rn(4 * C, C, scale=C ** -0.5).to(BF), rn(C, 4 * C, scale=(4 * C) ** -0.5).to(BF))


def rope_for(T, hs):
    from omnibiote_amd.model import precompute_freqs_cis, rope_tables
    return rope_tables(precompute_freqs_cis(hs, T).to(DEV))


def documents(B, T):
    tok = torch.full((B, T), 7, dtype=torch.int64)
    for b in range(B):
        for e in (T // 5 + 3 * b, T // 2 + 1, T - 9):
            tok[b, e] = 3
    return tok.to(DEV)


def mask_of(kind, B, T, H):
    from omnibiote_amd.masks import RangeMask
    o = ops()
    if kind == "none":
        return o.MaskSpec()
    if kind == "ranges":
        return o.MaskSpec.from_user(RangeMask.from_tokens(documents(B, T)), B, T, H, DEV)
    if kind == "dense_two_runs":   # not a range mask: every row allows two disjoint runs of keys
        k = torch.arange(T).view(1, 1, T)
        q = torch.arange(T).view(1, T, 1)
        lo = (q // 16) * 16
        allowed = ((k >= lo) & (k < lo + 16)) | ((k >= (lo + T // 2) % T) & (k < (lo + T // 2) % T + 8))
        m = torch.where(allowed, 0.0, -1e9).to(BF).expand(B, T, T).contiguous().to(DEV)
        spec = o.MaskSpec.from_user(m.unsqueeze(1), B, T, H, DEV)
        assert spec.dense is not None
        return spec
    assert kind == "dense_expand"  # the reference's expand() view of a block-diagonal mask: the gated launch
    m = RangeMask.from_tokens(documents(B, T)).dense(BF).unsqueeze(1).expand(-1, H, -1, -1)
    spec = o.MaskSpec.from_user(m, B, T, H, DEV)
    assert spec.dense is not None and spec.exact is not None and spec.sh == 0
    return spec


_block_ref = {}


def block_reference(B, T, C, H, kind, p):
    """(x, params of two blocks, rope, mask, y after block 1, y after block 2) through ops.block_fwd; computed once per case."""
    key = (B, T, C, H, kind, p)
    if key not in _block_ref:
        g = torch.Generator(device=DEV).manual_seed(17)
        x = torch.randn(B, T, C, device=DEV, generator=g).to(BF)
        pa, pb = block_params(C, 1), block_params(C, 2)
        rope = rope_for(T, C // H)
        mask = mask_of(kind, B, T, H)
        y1, _ = ops().block_fwd(x, pa, rope, H, mask, p, 1234)
        y2, _ = ops().block_fwd(y1, pb, rope, H, mask, p, 99)
        _block_ref[key] = (x, pa, pb, rope, mask, y1, y2)
    return _block_ref[key]


BLOCK_SHAPES = [(2, 128, 128, 2), (1, 320, 256, 2)]   # head size 64; head size 128 with T no multiple of the 256-query tile


@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("kind", ["none", "ranges", "dense_two_runs", "dense_expand"])
@pytest.mark.parametrize("B,T,C,H", BLOCK_SHAPES)
def test_block_infer_equals_block_fwd_bit_for_bit(B, T, C, H, kind, p):
    x, pa, pb, rope, mask, y1, y2 = block_reference(B, T, C, H, kind, p)
    o = ops()
    ws = o.block_infer_workspace(B, T, C, H, DEV)
    ws.fill_(0xFF)                                     # its contents are irrelevant before the call (NaN patterns if anything read them)
    z1 = o.block_infer(x, pa, rope, H, mask, p, 1234, ws=ws)
    z2 = o.block_infer(z1, pb, rope, H, mask, p, 99, ws=ws)   # the next block through the same workspace
    assert torch.isfinite(y2.float()).all()
    assert torch.equal(z1, y1)
    assert torch.equal(z2, y2)


def test_block_infer_allocates_its_workspace_and_refuses_a_short_one():
    B, T, C, H = BLOCK_SHAPES[0]
    x, pa, _, rope, mask, y1, _ = block_reference(B, T, C, H, "ranges", 0.0)
    o = ops()
    assert torch.equal(o.block_infer(x, pa, rope, H, mask), y1)
    short = torch.empty(o.block_infer_workspace(B, T, C, H, DEV).numel() - 256, dtype=torch.uint8, device=DEV)
    with pytest.raises(RuntimeError, match="workspace"):
        o.block_infer(x, pa, rope, H, mask, ws=short)


def test_block_fwd_infer_leaves_the_rows_form_to_block_fwd():
    B, T, C, H = BLOCK_SHAPES[0]
    x, pa, _, rope, mask, _, _ = block_reference(B, T, C, H, "none", 0.0)
    o, Lm = ops(), L()
    rows = torch.arange(0, B * T, 3, device=DEV)
    d = o._block_desc(B, T, C, H, pa, rope, mask, out_rows=rows)
    ws = o.block_infer_workspace(B, T, C, H, DEV)
    y = torch.empty_like(x)
    assert Lm.lib().obte_block_fwd_infer(ctypes.byref(d), x.data_ptr(), y.data_ptr(), ws.data_ptr(), ws.numel(), None) == -3
    assert "rows" in Lm.lib().obte_last_error().decode()


# ------------------------------------------------------------------------------------------------------------------- 3. aliasing
@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("B,T,C,H", BLOCK_SHAPES)
def test_block_infer_may_write_its_output_over_its_input(B, T, C, H, p):
    x, pa, _, rope, mask, y1, _ = block_reference(B, T, C, H, "ranges", p)
    xin = x.clone()
    out = ops().block_infer(xin, pa, rope, H, mask, p, 1234, out=xin)
    assert out.data_ptr() == xin.data_ptr()
    assert torch.equal(xin, y1)


# --------------------------------------------------------------------------------------------------------------------- 4. the model
def build_model(n_layer, C, H, V, T, dropout):
    from omnibiote_amd.model import OmniBioTA, OmniBioTAConfig
    from omnibiote_amd.mup_compat import set_base_shapes
    c = OmniBioTAConfig()
    c.block_size, c.vocab_size, c.n_layer, c.n_head, c.n_embd, c.dropout, c.flash = T, V, n_layer, H, C, dropout, True
    m = OmniBioTA(c)
    cb = OmniBioTAConfig(); cb.block_size, cb.vocab_size, cb.n_layer, cb.dropout, cb.flash = T, V, n_layer, dropout, True
    cb.n_embd, cb.n_head = 24, 3
    base = OmniBioTA(cb)
    cb.n_embd, cb.n_head = 48, 12
    delta = OmniBioTA(cb)
    set_base_shapes(m, base, delta=delta, rescale_params=False)
    m.load_state_dict(R.hash_weights(R.RefConfig(block_size=T, vocab_size=V, n_layer=n_layer, n_head=H, n_embd=C)), strict=False)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        m.to(BF)
    return m.to(DEV)


@pytest.fixture(scope="module")
def model4():
    return build_model(4, 256, 2, 512, 192, 0.1)


def model_inputs(B=2, T=192, V=512):
    from omnibiote_amd.masks import RangeMask
    tok = torch.from_numpy(np.random.default_rng(3).integers(20, V, size=(B, T)))
    tok[0, 50] = 3; tok[1, [20, 130]] = 3
    tok = tok.to(DEV)
    return tok, RangeMask.from_tokens(tok)


class Calls:
    """Counts the calls of the two block entry points of omnibiote_amd.ops."""

    def __init__(self, monkeypatch):
        o = ops()
        self.infer = self.fwd = 0
        real_infer, real_fwd = o.block_infer, o.block_fwd

        def infer(*a, **k):
            self.infer += 1
            return real_infer(*a, **k)

        def fwd(*a, **k):
            self.fwd += 1
            return real_fwd(*a, **k)
        monkeypatch.setattr(o, "block_infer", infer)
        monkeypatch.setattr(o, "block_fwd", fwd)


@pytest.mark.parametrize("mode", ["eval", "train"])
def test_no_grad_forward_equals_the_grad_enabled_forward(model4, mode, monkeypatch):
    monkeypatch.delenv("OBTE_INFER", raising=False)
    m = model4
    m.train(mode == "train")       # train(): dropout 0.1 in every block, the seeds drawn from torch's generator
    idx, mask = model_inputs()
    calls = Calls(monkeypatch)
    try:
        for emb in (False, True):
            torch.manual_seed(11)
            want = m(idx, attn_mask=mask, return_embeddings=emb)
            assert want.requires_grad and calls.fwd == 4 and calls.infer == 0
            with torch.no_grad():
                torch.manual_seed(11)
                got = m(idx, attn_mask=mask, return_embeddings=emb)
                assert calls.infer == 4 and calls.fwd == 4
                monkeypatch.setenv("OBTE_INFER", "0")
                torch.manual_seed(11)
                old = m(idx, attn_mask=mask, return_embeddings=emb)
                assert calls.infer == 4 and calls.fwd == 8
                monkeypatch.delenv("OBTE_INFER")
            assert not got.requires_grad
            assert torch.equal(got, want.detach())
            assert torch.equal(old, want.detach())
            calls.infer = calls.fwd = 0
    finally:
        m.eval()


def test_encode_is_the_same_under_both_settings_of_the_switch(model4, monkeypatch):
    m = model4.eval()
    idx, _ = model_inputs()
    for method in ("mean", "first", "last", "max", "all"):
        with torch.no_grad():
            monkeypatch.setenv("OBTE_INFER", "1")
            a = m.encode(idx, method)
            monkeypatch.setenv("OBTE_INFER", "0")
            b = m.encode(idx, method)
        assert torch.equal(a, b), method
        assert torch.equal(a, m.encode(idx, method).detach()), method


def test_standalone_mlp_uses_the_activation_only_epilogue_without_a_gradient(model4, monkeypatch):
    monkeypatch.delenv("OBTE_INFER", raising=False)
    mlp = model4.eval().transformer.h[0].mlp
    o, Lm = ops(), L()
    seen = []
    real = o.linear_fwd
    monkeypatch.setattr(o, "linear_fwd", lambda *a, **k: (seen.append(k.get("epilogue", Lm.EPI_NONE)), real(*a, **k))[1])
    x = torch.randn(2, 64, 256, device=DEV, generator=torch.Generator(device=DEV).manual_seed(2)).to(BF)
    want = mlp(x)
    assert seen == [Lm.EPI_GELU, Lm.EPI_NONE] and want.requires_grad
    del seen[:]
    with torch.no_grad():
        got = mlp(x)
    assert seen == [Lm.EPI_GELU_ACT, Lm.EPI_NONE]
    assert torch.equal(got, want.detach())


# ---------------------------------------------------------------------------------------------------------------- 5. path selection
def test_path_selection(model4, monkeypatch):
    monkeypatch.delenv("OBTE_INFER", raising=False)
    m = model4.eval()
    idx, mask = model_inputs()
    calls = Calls(monkeypatch)
    # grad enabled, trainable weights: the training forward, and a backward runs
    y = m(idx, attn_mask=mask, return_embeddings=True)
    assert calls.fwd == 4 and calls.infer == 0 and y.grad_fn is not None
    y.backward(torch.ones_like(y))
    assert m.transformer.h[0].attn.c_attn.weight.grad is not None
    m.zero_grad(set_to_none=True)
    calls.fwd = calls.infer = 0
    # rows= under no_grad: the last block stays with obte_block_fwd, the others keep nothing
    rows = torch.arange(5, idx.numel(), 7, device=DEV)
    want = m(idx, attn_mask=mask, return_embeddings=True, rows=rows).detach()
    assert calls.fwd == 4 and calls.infer == 0
    with torch.no_grad():
        got = m(idx, attn_mask=mask, return_embeddings=True, rows=rows)
    assert calls.fwd == 5 and calls.infer == 3
    assert torch.equal(got, want)
    calls.fwd = calls.infer = 0
    # a block: frozen parameters need no saved activations unless the input wants its gradient
    blk = m.transformer.h[1]
    g = torch.Generator(device=DEV).manual_seed(4)
    x = torch.randn(2, 192, 256, device=DEV, generator=g).to(BF)
    dy = torch.randn(2, 192, 256, device=DEV, generator=g).to(BF)
    xa = x.clone().requires_grad_(True)
    ya = blk(xa, attn_mask=mask)
    ya.backward(dy)
    assert calls.fwd == 1 and calls.infer == 0
    try:
        for prm in blk.parameters():
            prm.requires_grad_(False)
        x0 = x.clone()
        y0 = blk(x0, attn_mask=mask)                      # grad mode on, nothing to differentiate
        assert calls.fwd == 1 and calls.infer == 1 and y0.grad_fn is None
        assert torch.equal(y0, ya.detach()) and torch.equal(x0, x)      # (a direct call leaves its input alone)
        xb = x.clone().requires_grad_(True)
        yb = blk(xb, attn_mask=mask)                      # frozen, but dx is wanted
        assert calls.fwd == 2 and calls.infer == 1 and yb.grad_fn is not None
        yb.backward(dy)
        assert torch.equal(xb.grad, xa.grad)
    finally:
        for prm in blk.parameters():
            prm.requires_grad_(True)
        m.zero_grad(set_to_none=True)


# ------------------------------------------------------------------------------------------------------------------------ 6. memory
def test_no_grad_forward_stays_within_twelve_activation_units(monkeypatch):
    """A condition, not a measurement.  Per block the training forward holds its input, its output and the 15-unit activation
    buffer (unit = M C 2 bytes: 17 at least); the forward-only path holds the embedding it overwrites, the 7-unit workspace with
    its small fp32 rows and ln_f's output: about 10."""
    B, T, C, H = 4, 512, 512, 4
    unit = B * T * C * 2
    m = build_model(4, C, H, 512, T, 0.0).eval()
    idx, mask = model_inputs(B, T)

    def peak_over_level():
        with torch.no_grad():
            m(idx, attn_mask=mask, return_embeddings=True)           # warm-up
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            level = torch.cuda.memory_allocated()
            emb = m(idx, attn_mask=mask, return_embeddings=True)
            torch.cuda.synchronize()
            peak = torch.cuda.max_memory_allocated()
        del emb
        return peak - level
    monkeypatch.setenv("OBTE_INFER", "0")
    old = peak_over_level()
    monkeypatch.delenv("OBTE_INFER")
    new = peak_over_level()
    print(f"peak over level, in units of M C 2 bytes: forward-only {new / unit:.2f}, training forward {old / unit:.2f}")
    assert old > 15 * unit, old / unit          # the test can see the difference
    assert new <= 12 * unit, new / unit
