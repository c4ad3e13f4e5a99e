"""GPU tests of the optional fp32 accumulation of weight gradients over the passes of one optimizer step
(include/omnibiote_hip.h: OBTE_EPI_ACC32, obte_embedding_bwd_acc32, obte_acc32_add_bf16; TrainStep(grad_accum="fp32")).

The semantics define the bits — pass 0: acc32 = c; middle passes: acc32 = fl32(acc32 + c); last pass: the same add, then the
gradient is bf16(acc32); c = fl32(alpha * the fp32 accumulator), formed before any rounding to bf16 — so every check but one
is bitwise.  The one that is not (the train step against the fp64 sum of separately computed micro-batch gradients) asserts
an ordering of two errors, not a bound."""
import os
import socket
import subprocess
import sys
import warnings

import numpy as np
import pytest
import torch

import omnibiote_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_OUT, K_IN = 320, 328     # dW [320, 328]: one full 256 x 256 tile plus edges of 64 and 72
FORMS = ["single_k128", "single_k40", "splitk3", "group1", "group2"]


def ops():
    from omnibiote_amd import ops as o
    return o


def Lm():
    from omnibiote_amd import _lib
    return _lib


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(BF)


def tokens_of(form):
    return {"single_k128": 128, "single_k40": 40, "splitk3": 192, "group1": 128, "group2": 128}[form]


class Form:
    """One launch form of the weight gradient dW = alpha dy^T x, with and without the fp32 sum."""

    def __init__(self, form):
        self.form = form
        self.tokens = tokens_of(form)
        # the plain problem beside the fp32-summed one in the group of two: a dy W product (other layout), EPI_NONE
        self.side_a, self.side_b = rnd(128, 128, seed=90).to(DEV), rnd(128, 256, seed=91).to(DEV)

    def __enter__(self):
        if self.form == "splitk3":   # three K-tiles of 64 tokens, one per split; the fp32 form borrows the NONE plan
            Lm().check(Lm().lib().obte_gemm_plan_set(0, 0, Lm().EPI_NONE, N_OUT, K_IN, self.tokens, 2, 128, 3), "obte_gemm_plan_set")
            assert Lm().lib().obte_gemm_workspace_bytes(N_OUT, K_IN, self.tokens) == 3 * N_OUT * K_IN * 4
        return self

    def __exit__(self, *exc):
        if self.form == "splitk3":
            Lm().check(Lm().lib().obte_gemm_plan_clear(), "obte_gemm_plan_clear")
        return False

    def side(self, out=None):
        return dict(a=self.side_a, b=self.side_b, M=128, N=256, K=128, a_kmajor=True,
                    out=torch.empty(128, 256, dtype=BF, device=DEV) if out is None else out)

    def plain(self, dy, x, alpha=1.0):
        """The existing overwrite-form gradient under the same plan / kernel structure."""
        if self.form.startswith("group"):
            out = torch.empty(N_OUT, K_IN, dtype=BF, device=DEV)
            ops().gemm_grouped([dict(a=dy, b=x, M=N_OUT, N=K_IN, K=self.tokens, out=out, alpha=alpha)])
            return out
        return ops().linear_wgrad(dy, x, alpha=alpha)

    def acc(self, dy, x, acc32, mode, alpha=1.0):
        if self.form == "group1":
            return ops().gemm_grouped([dict(a=dy, b=x, M=N_OUT, N=K_IN, K=self.tokens, acc32=acc32, acc32_mode=mode, alpha=alpha)])[0]
        if self.form == "group2":
            alone = ops().gemm_grouped([self.side()])[0]
            outs = ops().gemm_grouped([dict(a=dy, b=x, M=N_OUT, N=K_IN, K=self.tokens, acc32=acc32, acc32_mode=mode, alpha=alpha), self.side()])
            assert torch.equal(outs[1], alone), "the plain problem of a mixed group differs from its stand-alone result"
            return outs[0]
        return ops().linear_wgrad(dy, x, alpha=alpha, acc32=acc32, acc32_mode=mode)


# ------------------------------------------------------------------------------------------------ 1. exact swamping case
@pytest.mark.parametrize("form", FORMS)
def test_small_contributions_survive_where_a_bf16_running_sum_drops_them(form):
    """Pass 0 contributes 256 c[n,k], c in {1,2,3}; sixteen more passes contribute s[n,k] in {-1,+1} each.  Every product and
    sum is an exact small integer, so the buffer must be exactly 256 c + 16 s and the last pass's output that value in bf16
    (all nine values have at most 8 significant bits).  A running bf16 sum stays at 256 c wherever s = +1: 256 c + 1 rounds back."""
    L = Lm()
    with Form(form) as f:
        Kt = f.tokens
        n, k = torch.arange(N_OUT), torch.arange(K_IN)
        a, b = (n % 2).float(), (k % 3 == 0).float()
        c = 1 + a[:, None] + b[None, :]                                   # {1,2,3}, not symmetric in n and k
        sa, sb = torch.where(n % 3 == 0, -1.0, 1.0), torch.where(k % 5 < 2, 1.0, -1.0)
        s = sa[:, None] * sb[None, :]
        dy0, x0 = torch.zeros(Kt, N_OUT), torch.zeros(Kt, K_IN)
        dy0[0], x0[0] = 16 * (1 + a), 16.0                                # token 0: 256 (1 + a[n])
        dy0[Kt - 1], x0[Kt - 1] = 16.0, 16 * b                            # last token (the zero-filled K tail of K = 40): 256 b[k]
        dy1, x1 = torch.zeros(Kt, N_OUT), torch.zeros(Kt, K_IN)
        dy1[Kt // 2], x1[Kt // 2] = sa, sb
        dy0, x0, dy1, x1 = (t.to(BF).to(DEV) for t in (dy0, x0, dy1, x1))
        acc32 = torch.full((N_OUT, K_IN), float("nan"), dtype=torch.float32, device=DEV)   # FIRST must overwrite whatever is there
        assert f.acc(dy0, x0, acc32, L.ACC32_FIRST) is None
        assert torch.equal(acc32.cpu(), 256 * c)
        for i in range(16):
            out = f.acc(dy1, x1, acc32, L.ACC32_LAST if i == 15 else L.ACC32_MORE)
            assert (out is None) == (i < 15)
        want = 256 * c + 16 * s
        assert torch.equal(acc32.cpu(), want), (acc32.cpu() - want).abs().max().item()
        assert torch.equal(out.float().cpu(), want) and out.dtype == BF
        if form == "single_k128":   # what the default arithmetic does with the same contributions
            g = ops().linear_wgrad(dy0, x0)
            for i in range(16):
                ops().linear_wgrad(dy1, x1, accumulate_into=g)
            g = g.float().cpu()   # +1 on 256 c is half a bf16 step or less and rounds back every time (-1 below 256 is representable)
            assert torch.equal(g[s > 0], (256 * c)[s > 0]) and not torch.equal(g, want)


# ----------------------------------------------------------------------------- 2. / 3. one pass, several passes (random)
@pytest.mark.parametrize("alpha", [1.0, 3.0 / 128.0])
@pytest.mark.parametrize("form", FORMS)
def test_one_pass_is_the_existing_kernel_and_three_passes_are_the_fp32_sum(form, alpha):
    L = Lm()
    with Form(form) as f:
        Kt = f.tokens
        dys = [rnd(Kt, N_OUT, seed=10 + i).to(DEV) for i in range(3)]
        xs = [rnd(Kt, K_IN, seed=20 + i).to(DEV) for i in range(3)]
        singles = []
        for dy, x in zip(dys, xs):   # after FIRST the buffer, rounded, is the existing overwrite-form gradient bit for bit
            b = torch.full((N_OUT, K_IN), float("nan"), dtype=torch.float32, device=DEV)
            f.acc(dy, x, b, L.ACC32_FIRST, alpha)
            assert torch.equal(b.to(BF), f.plain(dy, x, alpha)), "one pass differs from the existing kernel"
            singles.append(b)
        runs = []
        for _ in range(2):
            acc32 = torch.empty(N_OUT, K_IN, dtype=torch.float32, device=DEV)
            f.acc(dys[0], xs[0], acc32, L.ACC32_FIRST, alpha)
            f.acc(dys[1], xs[1], acc32, L.ACC32_MORE, alpha)
            out = f.acc(dys[2], xs[2], acc32, L.ACC32_LAST, alpha)
            runs.append((acc32.clone(), out.clone()))
        want = (singles[0] + singles[1]) + singles[2]           # fp32, each add rounded: what the protocol defines
        assert torch.equal(runs[0][0], want), (runs[0][0] - want).abs().max().item()
        assert torch.equal(runs[0][1], want.to(BF))
        assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])


def test_plans_and_arguments_the_fp32_form_does_not_have_are_refused():
    L = Lm()
    lib = L.lib()
    assert lib.obte_gemm_plan_set(0, 0, L.EPI_ACC32, 512, 512, 512, 3, 256, 1) == 0
    assert lib.obte_gemm_plan_set(0, 0, L.EPI_ACC32, 512, 512, 512, 2, 128, 4) == 0
    assert lib.obte_gemm_plan_set(0, 0, L.EPI_ACC32, 512, 512, 512, 1, 128, 1) != 0      # structure 1 has no fp32 form
    assert lib.obte_gemm_plan_set(1, 1, L.EPI_ACC32, 512, 512, 512, 3, 256, 1) != 0      # the weight-gradient layout only
    L.check(lib.obte_gemm_plan_clear())
    dy, x = rnd(128, 64, seed=1).to(DEV), rnd(128, 64, seed=2).to(DEV)
    with pytest.raises((RuntimeError, ValueError)):
        ops().linear_wgrad(dy, x, acc32=torch.empty(64, 64, dtype=torch.float32, device=DEV), acc32_mode=0)
    with pytest.raises(RuntimeError):
        ops().linear_wgrad(dy, x, acc32=torch.empty(64, 32, dtype=torch.float32, device=DEV), acc32_mode=L.ACC32_FIRST)


def test_acc32_add_is_the_unfused_form_of_the_same_sum():
    L = Lm()
    srcs = [rnd(24, 40, seed=i).to(DEV) for i in range(3)]
    acc32 = torch.full((24, 40), float("nan"), dtype=torch.float32, device=DEV)
    assert ops().acc32_add_(acc32, srcs[0], L.ACC32_FIRST) is None
    assert ops().acc32_add_(acc32, None, L.ACC32_MORE) is None
    assert ops().acc32_add_(acc32, srcs[1], L.ACC32_MORE) is None
    out = ops().acc32_add_(acc32, srcs[2], L.ACC32_LAST)
    want = (srcs[0].float() + srcs[1].float()) + srcs[2].float()
    assert torch.equal(acc32, want) and torch.equal(out, want.to(BF))
    assert torch.equal(ops().acc32_add_(acc32, None, L.ACC32_LAST), want.to(BF)) and torch.equal(acc32, want)
    ops().acc32_add_(acc32, None, L.ACC32_FIRST)
    assert torch.equal(acc32, torch.zeros_like(acc32))


# -------------------------------------------------------------------------------------------------------- 4. block level
def _block_setup(C, H, T, B=2):
    from omnibiote_amd.model import rope_tables
    hs = C // H
    cfg = R.RefConfig(block_size=T, vocab_size=256, n_layer=1, n_head=H, n_embd=C)
    w = {k: v.to(BF) for k, v in R.hash_weights(cfg).items()}
    pre = "transformer.h.0."
    names = ["ln_1.weight", "attn.c_attn.weight", "attn.c_proj.weight", "ln_2.weight", "mlp.c_fc.weight", "mlp.c_proj.weight"]
    params = tuple(w[pre + n].to(DEV) for n in names)
    rope = rope_tables(R.cast_rope_table(R.rope_table(hs, T), BF).to(DEV))
    tokens = np.random.default_rng(3).integers(20, 100, size=(B, T))
    tokens[0, T // 2] = R.EOS_TOKEN
    ranges = ops().key_ranges_from_tokens(torch.from_numpy(tokens).to(DEV))
    return params, rope, ops().MaskSpec(ranges=ranges)


@pytest.mark.parametrize("C,H", [(128, 2), (256, 2)])
@pytest.mark.parametrize("form", ["grouped", "separate", "rows"])
def test_block_backward_sums_its_four_matrices_in_fp32(monkeypatch, C, H, form):
    """ops.block_bwd over three passes with different dy: after FIRST alone each of the four buffers, rounded, is the existing
    block_bwd's gradient; after FIRST / MORE / LAST they are the fp32 sum of the three and the returned gradients their
    rounding; dx and the LayerNorm weight gradients are the existing path's in every pass.  All bitwise."""
    L = Lm()
    o = ops()
    monkeypatch.setenv("OBTE_GROUPED_WGRAD", "1" if form == "grouped" else "0")
    B, T = 2, 64
    params, rope, spec = _block_setup(C, H, T, B)
    x = rnd(B, T, C, seed=1).to(DEV)
    rows_d = None
    n_dy = B * T
    if form == "rows":
        rows_d = torch.sort(torch.randperm(B * T, generator=torch.Generator().manual_seed(5))[:24]).values.to(DEV)
        n_dy = 24
    y, act = o.block_fwd(x, params, rope, H, spec, out_rows=rows_d)
    dys = [rnd(n_dy, C, seed=40 + i, scale=0.1).to(DEV).reshape((B, T, C) if rows_d is None else (n_dy, C)) for i in range(3)]
    mats = (1, 2, 4, 5)
    new = lambda: tuple(torch.full(params[i].shape, float("nan"), dtype=torch.float32, device=DEV) for i in mats)
    plain, singles = [], []
    for dy in dys:
        dx, grads = o.block_bwd(x, dy, act, params, rope, H, spec, out_rows=rows_d)
        plain.append((dx, grads))
        bufs = new()
        dx1, g1 = o.block_bwd(x, dy, act, params, rope, H, spec, out_rows=rows_d, acc32=bufs, acc32_mode=L.ACC32_FIRST)
        assert torch.equal(dx1, dx)
        for j, i in enumerate(mats):
            assert g1[i] is None
            assert torch.equal(bufs[j].to(BF), grads[i]), f"matrix {i}: one pass differs from the existing kernel"
        for i in (0, 3):
            assert torch.equal(g1[i], grads[i])
        singles.append(bufs)
    bufs = new()
    for p, (dy, mode) in enumerate(zip(dys, (L.ACC32_FIRST, L.ACC32_MORE, L.ACC32_LAST))):
        dxp, gp = o.block_bwd(x, dy, act, params, rope, H, spec, out_rows=rows_d, acc32=bufs, acc32_mode=mode)
        assert torch.equal(dxp, plain[p][0]), f"dx of pass {p}"
        for i in (0, 3):
            assert torch.equal(gp[i], plain[p][1][i]), f"LayerNorm weight gradient {i} of pass {p}"
    for j, i in enumerate(mats):
        want = (singles[0][j] + singles[1][j]) + singles[2][j]
        assert torch.equal(bufs[j], want), (i, (bufs[j] - want).abs().max().item())
        assert torch.equal(gp[i], want.to(BF)), i


# ---------------------------------------------------------------------------------------------------- 5. embedding level
@pytest.mark.parametrize("p", [0.0, 0.1])
def test_embedding_backward_sums_in_fp32(p):
    L = Lm()
    o = ops()
    rows, cols, vocab, seed = 300, 64, 50, 1234
    rng = np.random.default_rng(7)
    idxs, douts = [], []
    for i in range(3):
        t = rng.integers(0, 40, size=rows)            # ids 40 .. 49 are never touched
        t[rng.permutation(rows)[:80]] = 7             # a run of 80 equal tokens: spans three 32-position chunks of the sorted order
        idxs.append(torch.from_numpy(t).to(DEV))
        douts.append(rnd(rows, cols, seed=60 + i).to(DEV))
    singles = []
    for idx, dout in zip(idxs, douts):
        b = torch.full((vocab, cols), float("nan"), dtype=torch.float32, device=DEV)
        assert o.embedding_bwd(idx, dout, vocab, dropout_p=p, dropout_seed=seed, acc32=b, acc32_mode=L.ACC32_FIRST) is None
        assert torch.equal(b.to(BF), o.embedding_bwd(idx, dout, vocab, dropout_p=p, dropout_seed=seed))
        singles.append(b)
    runs = []
    for _ in range(2):
        acc32 = torch.full((vocab, cols), float("nan"), dtype=torch.float32, device=DEV)
        o.embedding_bwd(idxs[0], douts[0], vocab, dropout_p=p, dropout_seed=seed, acc32=acc32, acc32_mode=L.ACC32_FIRST)
        o.embedding_bwd(idxs[1], douts[1], vocab, dropout_p=p, dropout_seed=seed, acc32=acc32, acc32_mode=L.ACC32_MORE)
        out = o.embedding_bwd(idxs[2], douts[2], vocab, dropout_p=p, dropout_seed=seed, acc32=acc32, acc32_mode=L.ACC32_LAST)
        runs.append((acc32.clone(), out))
    want = (singles[0] + singles[1]) + singles[2]
    assert torch.equal(runs[0][0], want) and torch.equal(runs[0][1], want.to(BF))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    assert torch.equal(runs[0][0][40:], torch.zeros(10, cols, device=DEV)) and torch.equal(runs[0][1][40:].float(), torch.zeros(10, cols, device=DEV))
    assert want[:40].abs().sum().item() > 0


# -------------------------------------------------------------------------------------------------------- 6. train step
C_, H_, LYR_, V_, T_ = 128, 2, 2, 512, 64


def _tiny_model():
    from omnibiote_amd.model import OmniBioTA, OmniBioTAConfig
    from omnibiote_amd.mup_compat import set_base_shapes
    c = OmniBioTAConfig(); c.block_size, c.vocab_size, c.n_layer, c.n_head, c.n_embd, c.dropout, c.flash = T_, V_, LYR_, H_, C_, 0.0, True
    m = OmniBioTA(c)
    cb = OmniBioTAConfig(); cb.block_size, cb.vocab_size, cb.n_layer, cb.dropout, cb.flash = T_, V_, LYR_, 0.0, True
    cb.n_embd, cb.n_head = 24, 3
    base = OmniBioTA(cb)
    cb.n_embd, cb.n_head = 48, 12
    delta = OmniBioTA(cb)
    set_base_shapes(m, base, delta=delta, rescale_params=False)
    m.load_state_dict(R.hash_weights(R.RefConfig(block_size=T_, vocab_size=V_, n_layer=LYR_, n_head=H_, n_embd=C_)), strict=False)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        m.to(BF)
    return m.to(DEV)


def _step(m, ids, mlm, mini=4, **kw):
    """One optimizer step at lr 0 (the weights stay): (loss, {name: gradient}, the TrainStep)."""
    from omnibiote_amd import train_encoder as TE
    step = TE.TrainStep(m, torch.optim.SGD(m.parameters(), lr=0.0), None, mini_batch_size=mini, n_head=H_, max_grad_norm=1e9, **kw)
    out = step(ids, mlm_mask=mlm)
    for k, p in m.named_parameters():
        assert p.grad is not None and p.grad.dtype == BF, k
    return out["loss"].item(), {k: p.grad.detach().clone() for k, p in m.named_parameters()}, step


def test_train_step_with_fp32_sums_is_closer_to_the_exact_sum_than_the_bf16_running_sum():
    """16 micro-batches of 4 rows.  S = the fp64 sum of the gradients of 16 separate single-micro-batch steps through the
    existing path, each divided by 16 (exact: a power of two).  For every parameter the gradient of grad_accum="fp32" must be
    closer to S (relative L2) than that of the default "bf16".  Also: two streams give the bits of one, and two micro-batches
    per pass the same loss."""
    from omnibiote_amd import train_encoder as TE
    rows, mini = 64, 4
    m = _tiny_model()
    ids = torch.from_numpy(TE.synthetic_rows(rows, T_, V_, np.random.default_rng(3), single_document=False)).to(DEV)
    mlm = torch.from_numpy(np.random.default_rng(4).random((rows, T_)) < 0.15).to(DEV)
    S = None
    for j in range(rows // mini):
        sl = slice(j * mini, (j + 1) * mini)
        _, g, _ = _step(m, ids[sl], mlm[sl], mini)
        S = {k: v.double() / 16 for k, v in g.items()} if S is None else {k: S[k] + g[k].double() / 16 for k in S}
    loss32, g32, st = _step(m, ids, mlm, mini, grad_accum="fp32")
    assert len(st._acc32_store) == 2 + 4 * LYR_                       # wte, lm_head and the blocks' four matrices each
    loss16, g16, _ = _step(m, ids, mlm, mini)
    assert abs(loss32 - loss16) <= 1e-5 * abs(loss16)
    rel = lambda g, k: ((g[k].double() - S[k]).norm() / S[k].norm()).item()
    report = {k: (rel(g32, k), rel(g16, k)) for k in S}
    print("relative L2 distance to the fp64 sum, (fp32 mode, bf16 mode):")
    for k, (e32, e16) in report.items():
        print(f"  {k}: {e32:.3e} {e16:.3e}  ratio {e32 / e16:.2f}")
    worse = {k: v for k, v in report.items() if not v[0] < v[1]}
    assert not worse, f"fp32 mode not closer to the exact sum than bf16 mode for {worse}; all (fp32, bf16): {report}"
    _, g32_2, _ = _step(m, ids, mlm, mini, grad_accum="fp32", pipeline_streams=2)
    for k in g32:
        assert torch.equal(g32_2[k], g32[k]), f"pipeline_streams=2 differs from 1 in {k}"
    _, g32_p, _ = _step(m, ids, mlm, mini, grad_accum="fp32", pipeline_streams=3, backward_order="pass")
    for k in g32:
        assert torch.equal(g32_p[k], g32[k]), f"pipeline_streams=3, backward_order='pass' differs in {k}"
    loss_k2, _, _ = _step(m, ids, mlm, mini, grad_accum="fp32", micro_batches_per_pass=2)
    assert abs(loss_k2 - loss32) <= 1e-5 * abs(loss32)
    # a step of a single pass runs the plain path: the bits of the default mode
    _, ga, sta = _step(m, ids[:mini], mlm[:mini], mini, grad_accum="fp32")
    _, gb, _ = _step(m, ids[:mini], mlm[:mini], mini)
    assert sta._acc32_store is None and all(torch.equal(ga[k], gb[k]) for k in ga)


# ------------------------------------------------------------------------------- 7. a micro-batch with nothing masked
@pytest.mark.parametrize("lm_head_impl", ["masked", "dense"])
def test_a_pass_with_nothing_masked_contributes_zero_wherever_it_falls(lm_head_impl):
    """Three micro-batches A, B, C.  With only one of them masked, the readout weight's buffer after the step is that pass's
    contribution (0 + c exactly) and its gradient the bits the default mode gives for the same mask.  With one of them NOT
    masked — first, middle or last — the readout weight's gradient is the fp32 sum of the other two buffers rounded once, and
    every parameter has a gradient."""
    from omnibiote_amd import train_encoder as TE
    rows, mini = 12, 4
    m = _tiny_model()
    w = m.lm_head.weight
    ids = torch.from_numpy(TE.synthetic_rows(rows, T_, V_, np.random.default_rng(3), single_document=False)).to(DEV)
    mlm = torch.from_numpy(np.random.default_rng(4).random((rows, T_)) < 0.15).to(DEV)

    def only(keep):
        mk = torch.zeros_like(mlm)
        for j in keep:
            mk[j * mini:(j + 1) * mini] = mlm[j * mini:(j + 1) * mini]
        return mk

    solo = []
    for j in range(3):
        _, g, st = _step(m, ids, only([j]), mini, grad_accum="fp32", lm_head_impl=lm_head_impl)
        buf = st._acc32_store.get(w).clone()
        assert torch.equal(g["lm_head.weight"], buf.to(BF)) and buf.abs().sum().item() > 0
        _, g16, _ = _step(m, ids, only([j]), mini, lm_head_impl=lm_head_impl)
        assert torch.equal(g["lm_head.weight"], g16["lm_head.weight"])
        solo.append(buf)
    for empty in range(3):
        keep = [j for j in range(3) if j != empty]
        _, g, st = _step(m, ids, only(keep), mini, grad_accum="fp32", lm_head_impl=lm_head_impl)
        want = solo[keep[0]] + solo[keep[1]]
        assert torch.equal(st._acc32_store.get(w), want), f"buffer with micro-batch {empty} empty"
        assert torch.equal(g["lm_head.weight"], want.to(BF)), f"gradient with micro-batch {empty} empty"


# ---------------------------------------------------------------------------------------------------------------- 8. DDP
def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _run_workers(world, backend, out_path, gpus):
    import time
    port = _free_port()
    procs, logs = [], []
    for r in range(world):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE=str(world), LOCAL_RANK=str(r), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
                   HSA_ENABLE_IPC_MODE_LEGACY="0", OMP_NUM_THREADS="2")
        log = open(f"{out_path}.rank{r}.log", "w+")
        logs.append(log)
        procs.append(subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "ddp_hip_fp32_worker.py"), backend, out_path, str(gpus)],
                                      env=env, stdout=log, stderr=subprocess.STDOUT))
    deadline = time.time() + 300
    try:
        while any(p.poll() is None for p in procs):
            if time.time() > deadline or any(p.poll() not in (None, 0) for p in procs):
                break
            time.sleep(0.2)
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
                p.wait()
    outs = []
    for log in logs:
        log.seek(0)
        outs.append(log.read())
        log.close()
    for r, (p, o) in enumerate(zip(procs, outs)):
        assert p.returncode == 0, f"rank {r} exited with {p.returncode}:\n" + o[-3000:]
    return torch.load(out_path, weights_only=False)


def _check_ddp(res):
    assert res["steps"] >= 2
    for s, rounds in enumerate(res["bucket_calls"]):
        assert rounds == list(range(res["n_buckets"])) and res["n_buckets"] >= 1, f"step {s}: buckets all-reduced {rounds}"   # each bucket once
    for k in res["plain"]["g"]:
        assert torch.equal(res["ddp"]["g"][k], res["plain"]["g"][k]), f"gradient {k}"
        assert torch.equal(res["ddp"]["w"][k], res["plain"]["w"][k]), f"weight {k}"
    assert res["ddp"]["losses"] == res["plain"]["losses"]


@pytest.mark.timeout(600)
def test_ddp_step_in_fp32_mode_is_the_unwrapped_step_with_one_all_reduce_round(tmp_path):
    _check_ddp(_run_workers(1, "gloo", str(tmp_path / "one.pt"), 1))


@pytest.mark.timeout(600)
def test_two_rccl_ranks_in_fp32_mode_are_the_unwrapped_step(tmp_path):
    n = torch.cuda.device_count()
    if n < 2:
        pytest.skip("needs two GPUs (RCCL refuses two ranks on one device); the one-rank gloo form above covers the one-GPU box")
    _check_ddp(_run_workers(2, "nccl", str(tmp_path / "two.pt"), n))


# ---------------------------------------------------------------------------------------------------------- 9. refusals
def test_combinations_that_would_sum_in_bf16_unnoticed_are_refused(monkeypatch):
    from omnibiote_amd import train_encoder as TE
    m = _tiny_model()
    mk = lambda **kw: TE.TrainStep(m, torch.optim.SGD(m.parameters(), lr=0.0), None, mini_batch_size=4, n_head=H_, grad_accum="fp32", **kw)
    with pytest.raises(ValueError, match="sync_every_micro_step"):
        mk(sync_every_micro_step=True)
    with pytest.raises(ValueError, match="fused_loss_fn"):
        mk(fused_loss_fn=lambda *a: None)
    with pytest.raises(ValueError, match="loss_impl"):
        mk(loss_impl="torch")
    m.config.checkpoint_freq = 1
    with pytest.raises(ValueError, match="checkpoint_freq"):
        mk()
    m.config.checkpoint_freq = 0
    step = mk()
    monkeypatch.setenv("OBTE_NO_INPLACE_ACCUM", "1")
    with pytest.raises(ValueError, match="OBTE_NO_INPLACE_ACCUM"):
        mk()
    ids = torch.from_numpy(TE.synthetic_rows(8, T_, V_, np.random.default_rng(3), single_document=False)).to(DEV)
    with pytest.raises(ValueError, match="OBTE_NO_INPLACE_ACCUM"):   # set after construction: refused at the call
        step(ids, mlm_mask=torch.from_numpy(np.random.default_rng(4).random((8, T_)) < 0.15).to(DEV))
    with pytest.raises(ValueError, match="grad_accum"):
        TE.TrainStep(m, torch.optim.SGD(m.parameters(), lr=0.0), None, mini_batch_size=4, n_head=H_, grad_accum="fp16")
