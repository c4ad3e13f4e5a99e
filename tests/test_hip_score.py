"""GPU tests of sequence scoring (include/omnibiote_hip_score.h): obte_readout_score_bf16 through ops.readout_score against
scoring.score_reference (float64, evaluated on the device), and OmniBioTA.score / token_logprobs against the model's own logits.
Every run carries targets of -1 (0 in both outputs) and one target out of range (NaN in both)."""

import numpy as np
import pytest
import torch

import omnibiote_ref as R_
from fenced import assert_guards, assert_same_bits, fenced
from omnibiote_amd import _lib
from omnibiote_amd.scoring import score_reference

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16
LSE_TOL = 1e-5    # the project's bar for an fp32 normaliser against float64 (the sampler's)


def _ops():
    from omnibiote_amd import ops
    return ops


def _targets(R, K, V, seed, bad=None):
    """(R, K) int64 on the device: random ids, a fifth of them -1, the first and the last column of the vocabulary, one value out of range"""
    g = torch.Generator().manual_seed(seed)
    t = torch.randint(0, V, (R, K), generator=g)
    t[torch.rand(R, K, generator=g) < 0.2] = -1
    t[0, 0] = V - 1
    t[-1, -1] = 0
    if R * K >= 3:
        t.view(-1)[1] = -1
    t[R // 2, K - 1] = (V if seed % 2 else -7) if bad is None else bad
    return t.to(DEV)


def _check_marks(t, V, lp, at):
    """-1: 0 in both; anything else outside [0, V): NaN in both; returns the mask of the targets inside"""
    t = t.reshape(lp.shape)
    none, inside = t == -1, (t >= 0) & (t < V)
    outside = ~none & ~inside
    assert bool(outside.any()) and bool((lp[none] == 0).all()) and bool((at[none] == 0).all())
    assert bool(torch.isnan(lp[outside]).all()) and bool(torch.isnan(at[outside]).all())
    assert bool(torch.isfinite(lp[inside]).all()) and bool(torch.isfinite(at[inside]).all())
    return inside


# =================================================================================================== 1. exact data
@pytest.mark.parametrize("V", [5, 128, 1000, 65536 + 40])
@pytest.mark.parametrize("R", [1, 127, 129, 257])
def test_exact_data_is_scored_exactly(R, V):
    """x, w in {-1, 0, 1} and alpha = 2^-3: every logit is a multiple of 1/8 of magnitude <= 24, exact in fp32 under every summation order
    and exact in bf16 (tests/test_score_host.py), so logits_at must equal the float64 value bit for bit: any wrong index, tail or
    slice shows.  C = 64, 128, 192: one, two and an odd number of K steps."""
    ops = _ops()
    for Cc in (64, 128, 192):
        g = torch.Generator(device=DEV).manual_seed(R * 7 + V + Cc)
        x = torch.randint(-1, 2, (R, Cc), generator=g, device=DEV).to(BF)
        w = torch.randint(-1, 2, (V, Cc), generator=g, device=DEV).to(BF)
        for K in (1, 3):
            t = _targets(R, K, V, R + V + Cc + K)
            t = t[:, 0].contiguous() if K == 1 and Cc == 128 else t                  # the (R,) form as well
            rlp, rlse, rat, _ = score_reference(x, w, t, 0.125)
            for slices in (0, 1, 3):
                tt = t.to(torch.int32) if slices == 1 else t
                lp, lse, at = ops.readout_score(x, w, tt, alpha=0.125, slices=slices)
                assert lp.shape == at.shape == t.shape and lse.shape == (R,) and lp.dtype == lse.dtype == at.dtype == torch.float32
                inside = _check_marks(t, V, lp, at)
                what = (R, V, Cc, K, slices)
                assert torch.equal(at[inside].double(), rat[inside]), what
                err = (lse.double() - rlse).abs().max().item()
                assert err <= LSE_TOL, (what, err)
                lse_k = lse if t.dim() == 1 else lse.unsqueeze(1).expand(t.shape)
                assert torch.equal(lp[inside], (at - lse_k)[inside]), what           # one fp32 subtraction


def test_exact_data_with_a_weight_beyond_four_gibibytes():
    """V = 2^25 + 40 rows of C = 64: the last tiles of w start more than 2^32 bytes into it (the buffer descriptors are re-based per tile
    and their size clipped to 32 bits), a slice is 4096 tiles long, and the normaliser sums 33 million terms.  The same exact data and
    the same bars; the reference is evaluated in chunks (fp32 products of this data are exact)."""
    ops = _ops()
    R, V, Cc, CH = 2, 2 ** 25 + 40, 64, 2 ** 21
    g = torch.Generator(device=DEV).manual_seed(25)
    x = torch.randint(-1, 2, (R, Cc), generator=g, device=DEV).to(BF)
    w = torch.empty(V, Cc, dtype=BF, device=DEV)
    parts = []
    for a in range(0, V, CH):
        b = min(a + CH, V)
        w[a:b] = torch.randint(-1, 2, (b - a, Cc), generator=g, device=DEV).to(BF)
        parts.append(torch.logsumexp(0.125 * (x.float() @ w[a:b].float().t()).double(), dim=1))
    rlse = torch.logsumexp(torch.stack(parts, dim=1), dim=1)
    assert w.numel() * 2 > 2 ** 32
    t = torch.tensor([[V - 1, -1, 2 ** 25 + 3], [0, V, 2 ** 24 + 129]], device=DEV)
    rat = 0.125 * (x.float().unsqueeze(1) * w[t.clamp(0, V - 1)].float()).sum(dim=2).double()
    lp, lse, at = ops.readout_score(x, w, t, alpha=0.125)
    inside = _check_marks(t, V, lp, at)
    assert torch.equal(at[inside].double(), rat[inside])
    err = (lse.double() - rlse).abs().max().item()
    print(f"V = 2^25 + 40: |lse - reference| = {err:.2e}")
    assert err <= LSE_TOL, err
    assert torch.equal(lp[inside], (at - lse.unsqueeze(1))[inside])


# =================================================================================================== 2. random data
@pytest.mark.parametrize("V", [8192, 65536])
def test_random_data_stays_inside_zbound(V):
    ops = _ops()
    R, Cc, K = 129, 1024, 3
    g = torch.Generator(device=DEV).manual_seed(V)
    x = torch.randn(R, Cc, generator=g, device=DEV).to(BF)
    w = (0.02 * torch.randn(V, Cc, generator=g, device=DEV)).to(BF)
    t = _targets(R, K, V, V)
    rlp, rlse, rat, zb = score_reference(x, w, t, 1.0)
    lp, lse, at = ops.readout_score(x, w, t)
    inside = _check_marks(t, V, lp, at)
    zb_t = zb.gather(1, t.clamp(0, V - 1))
    zb_max = zb.max(dim=1).values
    e_at = ((at.double() - rat).abs() / zb_t)[inside].max().item()
    e_lse = ((lse.double() - rlse).abs() / (zb_max + LSE_TOL)).max().item()
    e_lp = ((lp.double() - rlp).abs() / (zb_t + zb_max.unsqueeze(1) + LSE_TOL))[inside].max().item()
    print(f"V={V}: errors as fractions of their bounds: logits_at {e_at:.3f}, lse {e_lse:.3f}, logprobs {e_lp:.3f}")
    assert e_at <= 1 and e_lse <= 1 and e_lp <= 1, (e_at, e_lse, e_lp)
    assert torch.equal(at[inside].to(BF).float(), at[inside])                        # a bf16 value: one of the row's logits as the readout rounds them
    assert torch.equal(lp[inside], (at - lse.unsqueeze(1))[inside])


# =================================================================================================== 3. normalisation
def test_the_whole_vocabulary_as_candidates_sums_to_one():
    ops = _ops()
    R, V, Cc = 130, 40, 128
    g = torch.Generator(device=DEV).manual_seed(3)
    x = torch.randn(R, Cc, generator=g, device=DEV).to(BF)
    w = (0.3 * torch.randn(V, Cc, generator=g, device=DEV)).to(BF)
    t = torch.arange(V, device=DEV).expand(R, V).contiguous()
    lp, lse, at = ops.readout_score(x, w, t, alpha=0.5)
    assert (torch.exp(lp.double()).sum(dim=1) - 1).abs().max().item() <= 1e-5
    assert (lse.double() - torch.logsumexp(at.double(), dim=1)).abs().max().item() <= LSE_TOL
    t2 = t.clone()
    t2[7, 3] = V                                                                      # and the out-of-range mark in this shape too
    lp2, lse2, at2 = ops.readout_score(x, w, t2, alpha=0.5)
    assert torch.isnan(lp2[7, 3]) and torch.isnan(at2[7, 3]) and torch.equal(lse2, lse)
    lp2[7, 3], at2[7, 3] = lp[7, 3], at[7, 3]
    assert torch.equal(lp2, lp) and torch.equal(at2, at)


# =================================================================================================== 4. rows are independent
def test_a_row_has_the_same_bits_alone_and_twice():
    ops = _ops()
    R, V, Cc, K, S = 257, 1000, 128, 3, 3
    g = torch.Generator(device=DEV).manual_seed(4)
    x = torch.randn(R, Cc, generator=g, device=DEV).to(BF)
    w = (0.1 * torch.randn(V, Cc, generator=g, device=DEV)).to(BF)
    t = _targets(R, K, V, 4)
    a = ops.readout_score(x, w, t, slices=S)
    b = ops.readout_score(x, w, t, slices=S)
    for u, v in zip(a, b):
        assert_same_bits(u, v, "the second call")
    _check_marks(t, V, a[0], a[2])
    for r in (5, 128, 256):                                                           # three tiles, three places in a tile
        one = ops.readout_score(x[r:r + 1], w, t[r:r + 1], slices=S)
        for u, v, name in zip(one, a, ("logprobs", "lse", "logits_at")):
            assert_same_bits(u, v[r:r + 1], f"row {r} alone: {name}")
    x2 = x.clone()
    x2[:130] = float("nan")                                                           # whatever the other rows hold, in its own tile too
    c = ops.readout_score(x2, w, t, slices=S)
    for u, v in zip(c, a):
        assert_same_bits(u[130:], v[130:], "rows beside NaN rows")


# =================================================================================================== 5. fenced
@pytest.mark.parametrize("R,V,Cc,K,S", [(129, 1000, 128, 3, 3), (1, 5, 64, 1, 0), (130, 257, 192, 2, 1)])
def test_fenced_buffers(R, V, Cc, K, S):
    """x, w, targets, the outputs and the workspace in poisoned buffers at 16-byte alignment and no more, ldx and ldw larger than C: the
    plain call's bits, and not a byte written outside the payloads"""
    ops, lib = _ops(), _lib.lib()
    g = torch.Generator(device=DEV).manual_seed(R + V)
    x = torch.randn(R, Cc, generator=g, device=DEV).to(BF)
    w = (0.1 * torch.randn(V, Cc, generator=g, device=DEV)).to(BF)
    t = _targets(R, K, V, R + V).to(torch.int32)
    plain = ops.readout_score(x, w, t, alpha=0.5, slices=S)
    _check_marks(t, V, plain[0], plain[2])
    fx, hx = fenced(x, poison="nan", ld=Cc + 8)
    fw, hw = fenced(w, poison="nan", ld=Cc + 24)
    ft, ht = fenced(t)
    lp, hlp = fenced((R, K), torch.float32)
    at, hat = fenced((R, K), torch.float32)
    lse, hlse = fenced((R,), torch.float32)
    ws_bytes = lib.obte_readout_score_ws_bytes(R, V, S)
    ws, hws = fenced((R, ws_bytes // (4 * R)), torch.float32)
    assert fx.stride(0) == Cc + 8 and fw.stride(0) == Cc + 24 and ws.numel() * 4 == ws_bytes
    _lib.check(lib.obte_readout_score_bf16(fx.data_ptr(), Cc + 8, fw.data_ptr(), Cc + 24, R, V, Cc, 0.5, ft.data_ptr(), K, lp.data_ptr(), lse.data_ptr(),
                                           at.data_ptr(), S, ws.data_ptr(), ws_bytes, torch.cuda.current_stream().cuda_stream), "obte_readout_score_bf16")
    torch.cuda.synchronize()
    for got, want, name in zip((lp, lse, at), plain, ("logprobs", "lse", "logits_at")):
        assert_same_bits(got, want, name)
    assert_guards(hx, hw, ht, hlp, hat, hlse, hws)
    # the same through the wrapper on the strided views
    again = ops.readout_score(fx, fw, ft, alpha=0.5, slices=S)
    for got, want in zip(again, plain):
        assert_same_bits(got, want, "strided views")


# =================================================================================================== 6. no logits tensor
def test_no_logits_sized_allocation():
    ops = _ops()
    R, V, Cc = 2048, 65536, 1024
    x = torch.randn(R, Cc, device=DEV).to(BF)
    w = (0.02 * torch.randn(V, Cc, device=DEV)).to(BF)
    t = torch.randint(0, V, (R,), device=DEV)
    t[3], t[4] = -1, V
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    lp, lse, at = ops.readout_score(x, w, t)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    assert peak < R * V * 2 // 16, peak                                               # the logits alone are 256 MiB
    assert lp[3] == 0 and torch.isnan(lp[4]) and bool(torch.isfinite(lp[5:]).all())


# =================================================================================================== 7. through the model
_models = {}


def _model_case(H, autoregressive):
    """config {block 48, vocabulary 512, 2 layers, H heads, n_embd 128} with the oracle's hashed weights, and 3 x 48 tokens"""
    from test_hip_causal import _model
    key = (H, autoregressive)
    if key not in _models:
        cfg = R_.RefConfig(block_size=48, vocab_size=512, n_layer=2, n_head=H, n_embd=128)
        ids = torch.from_numpy(np.random.default_rng(H).integers(4, cfg.vocab_size, size=(3, 48)).astype(np.int64)).to(DEV)
        _models[key] = (_model(cfg, R_.hash_weights(cfg), autoregressive), ids)
    return _models[key]


def _model_bound(m, emb_rows, targets):
    """How far log p from the fused call may lie from log-softmax of the model's bf16 logits: both round alpha x w^T of the same ln_f
    output to bf16 once, from fp32 sums in different orders, so each logit of either side is within zbound of the exact product — the
    two differ by at most 2 zbound at the target and 2 max_v zbound in the normaliser, plus the fp32 normaliser's 1e-5 (case 2's bound,
    once per side)."""
    alpha = float(m.lm_head.output_mult) / float(m.lm_head.width_mult())
    zb = score_reference(emb_rows, m.lm_head.weight, targets, alpha)[3]
    return 2 * (zb.gather(1, targets.clamp(0, zb.shape[1] - 1).reshape(zb.shape[0], -1)) + zb.max(dim=1, keepdim=True).values) + LSE_TOL


@pytest.mark.parametrize("H", [2, 1])
def test_score_matches_the_models_own_logits(H):
    m, idx = _model_case(H, True)
    B, T = idx.shape
    lengths = [48, 17, 2]
    with torch.no_grad():
        logits = m(idx)
        ref = torch.log_softmax(logits.double(), dim=-1)[:, :-1].gather(2, idx[:, 1:].unsqueeze(-1)).squeeze(-1)          # (B, T - 1)
        emb = m(idx, return_embeddings=True)
    bound = _model_bound(m, emb[:, :-1].reshape(-1, emb.shape[-1]), idx[:, 1:].reshape(-1)).view(B, T - 1)
    s = m.score(idx, lengths)
    assert s.token_logprobs.shape == (B, T - 1) and s.token_logprobs.dtype == torch.float32 and s.total.shape == (B,) and s.total.dtype == torch.float32
    assert s.count.dtype == torch.int64 and s.count.tolist() == [47, 16, 1]
    real = torch.arange(T - 1, device=DEV).view(1, -1) < s.count.view(-1, 1)
    assert bool((s.token_logprobs[~real] == 0).all()) and bool((s.token_logprobs[real] < 0).all())
    frac = ((s.token_logprobs.double() - ref).abs() / bound)[real].max().item()
    print(f"H={H}: the largest error is {frac:.3f} of its bound (bounds {bound[real].min().item():.2e} .. {bound[real].max().item():.2e})")
    assert frac <= 1, frac
    assert torch.equal(s.total, s.token_logprobs.sum(dim=1))
    # padding does not reach a real position: the short rows alone, and the long one unchanged by its neighbours' lengths
    full = m.score(idx)
    assert full.count.tolist() == [47] * 3
    assert ((full.token_logprobs - s.token_logprobs).abs().double() <= bound)[real].all()
    # the mean next-token loss of the equal-length batch
    with torch.no_grad():
        loss = _ops().next_token_loss(logits, idx).item()
    mine = (-full.total.double().sum() / full.count.sum()).item()
    assert abs(mine - loss) <= bound.mean().item() + LSE_TOL, (mine, loss, bound.mean().item())
    # no dropout whatever the mode says, and the mode is left alone
    was = m.training
    m.train()
    try:
        again = m.score(idx, lengths)
        assert m.training
    finally:
        m.train(was)
    assert_same_bits(again.token_logprobs, s.token_logprobs, "train mode")


def test_token_logprobs_on_an_encoder():
    m, idx = _model_case(2, False)
    B, T = idx.shape
    V = m.config.vocab_size
    rows = torch.tensor([0, 3, 47, 48, 60, 95, 96, 120, 143], device=DEV)
    g = torch.Generator().manual_seed(9)
    cand = torch.randint(0, V, (9, 4), generator=g)
    cand[1, 2], cand[8, 0], cand[4, 3] = -1, -1, -1
    cand[0, 0], cand[8, 3] = V - 1, 0
    cand = cand.to(DEV)
    with torch.no_grad():
        ref_all = torch.log_softmax(m(idx, rows=rows).double(), dim=-1)                   # (9, V)
        emb = m(idx, return_embeddings=True, rows=rows)
    ref = ref_all.gather(1, cand.clamp(0, V - 1))
    bound = _model_bound(m, emb, cand)
    lp = m.token_logprobs(idx, rows, cand)
    assert lp.shape == (9, 4) and lp.dtype == torch.float32
    none = cand == -1
    assert bool((lp[none] == 0).all())
    frac = ((lp.double() - ref).abs() / bound)[~none].max().item()
    print(f"encoder: the largest error is {frac:.3f} of its bound")
    assert frac <= 1, frac
    one = m.token_logprobs(idx, rows, cand[:, 1].contiguous().to(torch.int32))            # (n,) in, (n,) out
    assert one.shape == (9,)
    assert_same_bits(one, lp[:, 1].contiguous(), "one candidate per row")
