"""GPU tests of encoder infilling (include/omnibiote_hip_fill.h): obte_readout_sample_bf16 through ops.readout_sample against the float64
rule (sampling.readout_sample_reference, evaluated on the device), obte_fill_commit through ops.fill_commit against
sampling.fill_commit_reference, and OmniBioTA.sample_tokens / infill on a tiny encoder.

The draw's data is test_hip_score.py's: x, w in {-1, 0, 1}, alpha = 2^-3, C = 64 — every logit z is exact in fp32 and in bf16 under any
summation order, so the kernel's z is the reference's and what is compared is the noise arithmetic and the selection."""
import math

import numpy as np
import pytest
import torch

import omnibiote_ref as R_
from fenced import assert_guards, assert_same_bits, fenced
from omnibiote_amd import _lib, sampling
from omnibiote_amd.sampling import GUMBEL_EPS

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16
LSE_TOL = 1e-5    # the project's bar for an fp32 normaliser against float64 (test_hip_score.py's)
ALPHA, CC = 0.125, 64


def _ops():
    from omnibiote_amd import ops
    return ops


def _data(R, V, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randint(-1, 2, (R, CC), generator=g).to(BF)
    w = torch.randint(-1, 2, (V, CC), generator=g).to(BF)
    keys = torch.randint(0, 2 ** 40, (R,), generator=g)
    return x.to(DEV), w.to(DEV), keys.to(DEV)


def _check_draw(x, w, temperature, seed, keys, allowed, got, what):
    """the eps-argmax comparison of one call's (tokens, logprob, lse) with the float64 rule; returns the number of near-tie rows"""
    tok, lp, lse = got
    R, V = x.shape[0], w.shape[0]
    assert tok.shape == lp.shape == lse.shape == (R,) and tok.dtype == torch.int64 and lp.dtype == lse.dtype == torch.float32
    rtok, _, rlse, P, y = sampling.readout_sample_reference(x, w, temperature, seed, keys=keys, allowed=allowed, alpha=ALPHA)
    live = rtok >= 0
    assert bool((tok[~live] == -1).all()) and bool((lp[~live] == -math.inf).all()) and bool((lse[~live] == -math.inf).all()), what
    assert bool(((tok >= 0) & (tok < V))[live].all()), what
    if V > 1 and temperature > 0:                                            # (a greedy call has no noise: the first maximum, exactly)
        top = torch.topk(P, 2, dim=1).values
        clear = live & ~((top[:, 0] - top[:, 1]) < 2 * GUMBEL_EPS)
    else:
        clear = live
    near = int((live & ~clear).sum())
    assert near <= 0.01 * R, (what, near)                                    # on the reference alone: near ties are rare
    assert torch.equal(tok[clear], rtok[clear]), (what, int((tok != rtok)[clear].sum()))
    at = P.gather(1, tok.clamp(min=0).unsqueeze(1)).squeeze(1)
    assert bool((at >= P.max(dim=1).values - GUMBEL_EPS)[live].all()), what
    e_lse = (lse.double() - rlse)[live].abs().max().item()
    e_lp = (lp.double() - (y.gather(1, tok.clamp(min=0).unsqueeze(1)).squeeze(1) - rlse))[live].abs().max().item()
    print(f"{what}: {near} near-tie rows of {R}, |lse - ref| {e_lse:.2e}, |logprob - ref| {e_lp:.2e}")
    assert e_lse <= LSE_TOL and e_lp <= LSE_TOL + GUMBEL_EPS, (what, e_lse, e_lp)
    if allowed is not None:
        a = allowed.expand(R, V)
        assert bool(a.gather(1, tok.clamp(min=0).unsqueeze(1)).squeeze(1)[live].all()), what
    return near


# =================================================================================================== 1. eps-argmax against float64
@pytest.mark.parametrize("R,V,S", [(1, 5, 0), (127, 129, 0), (300, 1000, 0), (129, 65576, 3)])
def test_draw_matches_the_float64_rule(R, V, S):
    """Every row whose two largest perturbed values lie 2 GUMBEL_EPS apart returns the rule's argmax exactly; the others a token within
    GUMBEL_EPS of the maximum.  lse within 1e-5, logprob within 1e-5 + GUMBEL_EPS of the rule's value at the returned token."""
    ops = _ops()
    x, w, keys = _data(R, V, R * 3 + V)
    for temperature in (1.0, 0.7):
        got = ops.readout_sample(x, w, temperature, 77 + R, keys=keys, alpha=ALPHA, slices=S)
        _check_draw(x, w, temperature, 77 + R, keys, None, got, (R, V, S, temperature))
    got = ops.readout_sample(x, w, 1.0, 5, alpha=ALPHA, slices=S)                                    # no keys: the row numbers
    _check_draw(x, w, 1.0, 5, torch.arange(R, device=DEV), None, got, (R, V, S, "row numbers"))


# =================================================================================================== 2. greedy
@pytest.mark.parametrize("R,V", [(1, 5), (127, 129), (300, 1000), (129, 65576)])
def test_greedy_is_the_first_maximum_with_the_score_kernels_bits(R, V):
    ops = _ops()
    x, w, keys = _data(R, V, R + V)
    z = ALPHA * (x.double() @ w.double().t())
    first = torch.where(z == z.max(dim=1, keepdim=True).values, torch.arange(V, device=DEV).unsqueeze(0), V).min(dim=1).values
    assert V < 100 or int((z == z.max(dim=1, keepdim=True).values).sum()) > R                           # heavily tied data
    for S in (0, 1, 3):
        tok, lp, lse = ops.readout_sample(x, w, 0, 9, keys=keys, alpha=ALPHA, slices=S)
        assert torch.equal(tok, first), (R, V, S)
        slp, slse, _ = ops.readout_score(x, w, tok, alpha=ALPHA, slices=S or _lib.lib().obte_readout_sample_slices(R, V))   # the same split
        assert_same_bits(lse, slse, f"lse {(R, V, S)}")
        assert_same_bits(lp, slp, f"logprob {(R, V, S)}")


# =================================================================================================== 3. invariance
def test_the_draw_depends_on_key_logits_and_seed_alone():
    ops = _ops()
    R, V, S = 257, 1000, 3
    x, w, keys = _data(R, V, 31)
    a = ops.readout_sample(x, w, 0.7, 12, keys=keys, alpha=ALPHA, slices=S)
    b = ops.readout_sample(x, w, 0.7, 12, keys=keys, alpha=ALPHA, slices=S)
    for u, v in zip(a, b):
        assert_same_bits(u, v, "the second call")
    for other in (1, 2, 5, 0):
        t = ops.readout_sample(x, w, 0.7, 12, keys=keys, alpha=ALPHA, slices=other)[0]
        assert torch.equal(t, a[0]), other
    for r in (5, 128, 256):                                                                             # three tiles, three places in a tile
        one = ops.readout_sample(x[r:r + 1], w, 0.7, 12, keys=keys[r:r + 1], alpha=ALPHA, slices=S)
        for u, v, name in zip(one, a, ("tokens", "logprob", "lse")):
            assert_same_bits(u, v[r:r + 1], f"row {r} alone: {name}")
    perm = torch.randperm(R, generator=torch.Generator().manual_seed(3)).to(DEV)
    c = ops.readout_sample(x[perm].contiguous(), w, 0.7, 12, keys=keys[perm].contiguous(), alpha=ALPHA, slices=S)
    for u, v, name in zip(c, a, ("tokens", "logprob", "lse")):
        assert_same_bits(u, v[perm], f"permuted rows: {name}")
    assert not torch.equal(ops.readout_sample(x, w, 0.7, 13, keys=keys, alpha=ALPHA, slices=S)[0], a[0])   # the seed matters
    assert not torch.equal(ops.readout_sample(x, w, 0.7, 12, keys=keys + 1, alpha=ALPHA, slices=S)[0], a[0])   # and the keys


# =================================================================================================== 4. token mask
@pytest.mark.parametrize("V", [129, 1000])
def test_token_mask_shared_and_per_row(V):
    ops = _ops()
    R = 131
    x, w, keys = _data(R, V, V)
    g = torch.Generator(device=DEV).manual_seed(V + 1)
    shared = torch.rand(V, generator=g, device=DEV) < 0.5
    shared[V - 1] = True
    rowwise = torch.rand(R, V, generator=g, device=DEV) < 0.5
    rowwise[3] = False
    rowwise[3, V - 2] = True                                                                            # one allowed token
    rowwise[70] = False                                                                                 # nothing allowed
    rowwise[129] = False
    rowwise[129, 0] = True
    free = ops.readout_sample(x, w, 0.7, 21, keys=keys, alpha=ALPHA)
    for name, allowed in (("shared", shared), ("per row", rowwise)):
        for temperature in (0.7, 0):
            got = ops.readout_sample(x, w, temperature, 21, keys=keys, allowed=allowed, alpha=ALPHA)
            _check_draw(x, w, temperature, 21, keys, allowed, got, (V, name, temperature))
            packed = ops.pack_token_mask(allowed)
            again = ops.readout_sample(x, w, temperature, 21, keys=keys, allowed_packed=packed, alpha=ALPHA)
            for u, v in zip(again, got):
                assert_same_bits(u, v, "the packed form")
    tok, lp, lse = ops.readout_sample(x, w, 0.7, 21, keys=keys, allowed=rowwise, alpha=ALPHA)
    assert tok[3] == V - 2 and lp[3] == 0 and tok[129] == 0 and lp[129] == 0
    assert tok[70] == -1 and lp[70] == -math.inf and lse[70] == -math.inf
    only = rowwise.clone()
    only[70] = True                                                                                     # the neighbours of the empty row are untouched
    t2, lp2, lse2 = ops.readout_sample(x, w, 0.7, 21, keys=keys, allowed=only, alpha=ALPHA)
    keep = torch.arange(R, device=DEV) != 70
    assert torch.equal(t2[keep], tok[keep]) and torch.equal(lp2[keep], lp[keep]) and torch.equal(lse2[keep], lse[keep])
    assert_same_bits(t2[70:71], free[0][70:71], "a row that allows everything")
    full = ops.readout_sample(x, w, 0.7, 21, keys=keys, allowed=torch.ones(V, dtype=torch.bool, device=DEV), alpha=ALPHA)
    for u, v in zip(full, free):
        assert_same_bits(u, v, "a mask that allows everything")


# =================================================================================================== 5. distribution
@pytest.mark.parametrize("V", [5, 40])
def test_tokens_follow_the_softmax(V):
    """65 536 rows of one x with the keys 0 .. 65535 under seed 2024 at temperature 1: Pearson's chi^2 of the token counts against the
    float64 softmax stays below (V - 1) + 6 sqrt(2 (V - 1)) = 20.97 (V = 5) and 91.99 (V = 40).  The float64 rule alone, on the CPU, on
    this data and seed: 1.07 and 35.88 — under half the bar — with 5 near-tie rows each."""
    ops = _ops()
    n = 65536
    g = torch.Generator().manual_seed(V)
    x = torch.randint(-1, 2, (1, CC), generator=g).to(BF).to(DEV)
    w = torch.randint(-1, 2, (V, CC), generator=g).to(BF).to(DEV)
    tok, lp, lse = ops.readout_sample(x.expand(n, CC).contiguous(), w, 1.0, 2024, keys=torch.arange(n, device=DEV), alpha=ALPHA)
    z = ALPHA * (x.double() @ w.double().t())[0]
    p = torch.softmax(z, dim=0)
    counts = torch.bincount(tok, minlength=V).double()
    chi2 = (((counts - n * p) ** 2) / (n * p)).sum().item()
    bar = (V - 1) + 6 * math.sqrt(2 * (V - 1))
    print(f"V = {V}: chi^2 = {chi2:.2f} against {bar:.2f}")
    assert counts.numel() == V and chi2 < bar, (chi2, bar)
    assert (lp.double() - torch.log(p)[tok]).abs().max().item() <= LSE_TOL + GUMBEL_EPS


# =================================================================================================== 6. fenced
@pytest.mark.parametrize("R,V,Cc,S", [(129, 1000, 128, 3), (1, 5, 64, 0), (130, 129, 192, 1)])
def test_fenced_buffers_of_the_draw(R, V, Cc, S):
    """every operand in a poisoned buffer at 16-byte alignment and no more, ldx and ldw larger than C, a per-row mask of exactly
    ceil(V / 8) bytes a row — odd row addresses, the last row ending at the fence, the padding bits of every row's last byte set: the
    plain call's bits, and not a byte written outside the payloads"""
    ops, lib = _ops(), _lib.lib()
    g = torch.Generator(device=DEV).manual_seed(R + V)
    x = torch.randn(R, Cc, generator=g, device=DEV).to(BF)
    w = (0.1 * torch.randn(V, Cc, generator=g, device=DEV)).to(BF)
    keys = torch.randint(0, 2 ** 62, (R,), generator=g, device=DEV)
    allowed = torch.rand(R, V, generator=g, device=DEV) < 0.6
    allowed[:, V - 1] = True
    plain = ops.readout_sample(x, w, 0.8, 99, keys=keys, allowed=allowed, alpha=0.5, slices=S)
    assert bool((plain[0] >= 0).all()) and bool(allowed.gather(1, plain[0].unsqueeze(1)).all())
    nb = (V + 7) // 8
    packed = ops.pack_token_mask(allowed)
    if V % 8:
        packed[:, -1] |= (0xFF << (V % 8)) & 0xFF                                                       # bits of columns >= V: ignored
    fx, hx = fenced(x, poison="nan", ld=Cc + 8)
    fw, hw = fenced(w, poison="nan", ld=Cc + 24)
    fk, hk = fenced(keys)
    fm, hm = fenced(packed)
    tok, htok = fenced((R,), torch.int32)
    lp, hlp = fenced((R,), torch.float32)
    lse, hlse = fenced((R,), torch.float32)
    ws_bytes = lib.obte_readout_sample_ws_bytes(R, V, S)
    ws, hws = fenced((ws_bytes // 4,), torch.float32)
    assert fm.stride(0) == nb and fm.is_contiguous() and ws.numel() * 4 == ws_bytes
    _lib.check(lib.obte_readout_sample_bf16(fx.data_ptr(), Cc + 8, fw.data_ptr(), Cc + 24, R, V, Cc, 0.5, sampling.inv_temperature(0.8), 99, fk.data_ptr(),
                                            fm.data_ptr(), nb if R > 1 else 0, tok.data_ptr(), lp.data_ptr(), lse.data_ptr(), S, ws.data_ptr(), ws_bytes,
                                            torch.cuda.current_stream().cuda_stream), "obte_readout_sample_bf16")
    torch.cuda.synchronize()
    for got, want, name in zip((tok.long(), lp, lse), plain, ("tokens", "logprob", "lse")):
        assert_same_bits(got, want, name)
    assert_guards(hx, hw, hk, hm, htok, hlp, hlse, hws)
    again = ops.readout_sample(fx, fw, 0.8, 99, keys=fk, allowed_packed=fm, alpha=0.5, slices=S)           # the same through the wrapper
    for got, want in zip(again, plain):
        assert_same_bits(got, want, "strided views")


def _commit_case(seed, sizes, T, take_kind):
    """rows of B sequences of ``sizes`` masked positions in (B, T), tokens, log-probabilities from a few values (ties, a NaN), takes"""
    g = torch.Generator().manual_seed(seed)
    B = len(sizes)
    rows = torch.cat([b * T + torch.randperm(T, generator=g)[:n].sort().values for b, n in enumerate(sizes)])
    seg = [0]
    for n in sizes:
        seg.append(seg[-1] + n)
    n = rows.numel()
    tokens = torch.randint(4, 300, (n,), generator=g)
    lp = torch.tensor([-0.25, -0.5, -0.5, -1.0, -2.0, -8.0])[torch.randint(0, 6, (n,), generator=g)]
    lp[n // 2] = float("nan")
    take = [dict(zero=0, one=1, all=m, over=m + 1)[take_kind] for m in sizes]
    nxt = [0]
    for m, k in zip(sizes, take):
        nxt.append(nxt[-1] + m - (k if 0 <= k <= m else 0))
    idx = torch.randint(4, 300, (B * T,), generator=g)
    out = torch.full((B * T,), 7.0)
    return rows, seg, tokens, lp, take, nxt, idx, out


def _i32(v):
    return torch.tensor(v, dtype=torch.int32, device=DEV)


# =================================================================================================== 7. the commit kernel
@pytest.mark.parametrize("order", ["confidence", "random", "left"])
def test_commit_matches_the_reference(order):
    """B = 4 with 0, 1, 33 and 300 entries, take 0, 1, n_b and n_b + 1 (a no-op): idx, out_logprob and rows_next bit for bit the plain-torch
    rule's — equal log-probabilities to the lower position, rows_next ascending at the given offsets, nothing else touched"""
    ops = _ops()
    sizes, T = [0, 1, 33, 300], 400
    for kind in ("zero", "one", "all", "over"):
        rows, seg, tokens, lp, take, nxt, idx, out = _commit_case(len(kind), sizes, T, kind)
        want = sampling.fill_commit_reference(rows, seg, tokens, lp, take, order, 5, idx, out, nxt)
        d_idx, d_out = idx.to(DEV), out.to(DEV)
        d_next = torch.full((nxt[-1] + 3,), -1, dtype=torch.int64, device=DEV)
        ops.fill_commit(rows.to(DEV), _i32(seg), tokens.to(DEV), lp.to(DEV), _i32(take), order, 5, d_idx, d_out, d_next, _i32(nxt), max(sizes))
        assert torch.equal(d_idx.cpu(), want[0]), (order, kind)
        assert_same_bits(d_out.cpu(), want[1], f"out_logprob {(order, kind)}")
        assert torch.equal(d_next[:nxt[-1]].cpu(), want[2]) and bool((d_next[nxt[-1]:] == -1).all()), (order, kind)
        for b in range(4):
            run = d_next[nxt[b]:nxt[b + 1]]
            assert bool((run[1:] > run[:-1]).all()) and bool(((run >= b * T) & (run < (b + 1) * T)).all())
        changed = (d_idx.cpu() != idx) | (d_out.cpu() != out)
        sel = torch.zeros(4 * T, dtype=torch.bool)
        sel[rows] = True
        assert not bool((changed & ~sel).any())
        if kind in ("zero", "over"):
            assert torch.equal(d_idx.cpu(), idx) and torch.equal(d_next[:nxt[-1]].cpu(), rows)
    # a tie across the whole sequence: the lowest positions win
    rows, seg, tokens, lp, take, nxt, idx, out = _commit_case(1, [0, 1, 33, 300], T, "one")
    lp[:] = -1.5
    take, nxt = [0, 0, 5, 7], [0, 0, 1, 29, 322]
    d_idx, d_out, d_next = idx.to(DEV), out.to(DEV), torch.empty(322, dtype=torch.int64, device=DEV)
    ops.fill_commit(rows.to(DEV), _i32(seg), tokens.to(DEV), lp.to(DEV), _i32(take), "confidence", 5, d_idx, d_out, d_next, _i32(nxt), 300)
    assert torch.equal(d_next.cpu(), torch.cat([rows[:1], rows[1 + 5:34], rows[34 + 7:]]))
    # a run longer than max_seg says: that sequence does nothing at all
    d_idx, d_next = idx.to(DEV), torch.full((322,), -1, dtype=torch.int64, device=DEV)
    ops.fill_commit(rows.to(DEV), _i32(seg), tokens.to(DEV), lp.to(DEV), _i32(take), "left", 5, d_idx, d_out, d_next, _i32(nxt), 33)
    assert bool((d_next[29:] == -1).all()) and torch.equal(d_next[:29].cpu(), torch.cat([rows[:1], rows[1 + 5:34]]))
    assert torch.equal(d_idx[3 * T:].cpu(), idx[3 * T:])


def test_fenced_buffers_of_the_commit():
    ops, lib = _ops(), _lib.lib()
    sizes, T = [3, 0, 33, 130], 200
    rows, seg, tokens, lp, _, _, idx, out = _commit_case(8, sizes, T, "one")
    take, nxt = [2, 0, 33, 40], [0, 1, 1, 1, 91]
    plain_idx, plain_out, plain_next = idx.to(DEV), out.to(DEV), torch.empty(91, dtype=torch.int64, device=DEV)
    ops.fill_commit(rows.to(DEV), _i32(seg), tokens.to(DEV), lp.to(DEV), _i32(take), "confidence", 5, plain_idx, plain_out, plain_next, _i32(nxt), 130)
    bufs = [fenced(t.to(DEV)) for t in (rows, _i32(seg), tokens.to(torch.int32), lp, _i32(take), idx, out, _i32(nxt))]
    (f_rows, f_seg, f_tok, f_lp, f_take, f_idx, f_out, f_nxt), handles = [b[0] for b in bufs], [b[1] for b in bufs]
    f_next, h_next = fenced((91,), torch.int64)
    _lib.check(lib.obte_fill_commit(f_rows.data_ptr(), f_seg.data_ptr(), rows.numel(), 4, 130, f_tok.data_ptr(), f_lp.data_ptr(), f_take.data_ptr(),
                                    _lib.FILL_CONFIDENCE, 5, f_idx.data_ptr(), f_out.data_ptr(), 4 * T, f_next.data_ptr(), f_nxt.data_ptr(), 91,
                                    torch.cuda.current_stream().cuda_stream), "obte_fill_commit")
    torch.cuda.synchronize()
    assert_same_bits(f_idx, plain_idx, "idx")
    assert_same_bits(f_out, plain_out, "out_logprob")
    assert_same_bits(f_next, plain_next, "rows_next")
    assert_guards(*handles, h_next)


# =================================================================================================== 8. no logits tensor
def test_no_logits_sized_allocation():
    ops = _ops()
    R, V, Cc = 2048, 65536, 1024
    x = torch.randn(R, Cc, device=DEV).to(BF)
    w = (0.02 * torch.randn(V, Cc, device=DEV)).to(BF)
    keys = torch.arange(R, device=DEV)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    tok, lp, lse = ops.readout_sample(x, w, 1.0, 4, keys=keys)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    assert peak < R * V * 2 // 16, peak                                                                 # the logits alone are 256 MiB
    assert bool(((tok >= 0) & (tok < V)).all()) and bool(torch.isfinite(lp).all()) and bool((lp <= 0).all())


# =================================================================================================== 9. through the model
_case = {}
MASK = 2


def _model_case():
    """a tiny encoder {block 40, vocabulary 300, 2 layers, 2 heads of 64} with the oracle's hashed weights, 3 x 40 tokens and masked
    positions: 9 in the first sequence, none in the second, 17 in the third"""
    from test_hip_causal import _model
    if not _case:
        cfg = R_.RefConfig(block_size=40, vocab_size=300, n_layer=2, n_head=2, n_embd=128)
        rng = np.random.default_rng(40)
        ids = torch.from_numpy(rng.integers(4, cfg.vocab_size, size=(3, 40)).astype(np.int64)).to(DEV)
        masked = torch.zeros(3, 40, dtype=torch.bool)
        masked[0, rng.choice(40, 9, replace=False)] = True
        masked[2, rng.choice(40, 17, replace=False)] = True
        _case["v"] = (_model(cfg, R_.hash_weights(cfg), False), ids, masked.to(DEV))
    return _case["v"]


def test_infill_in_one_step_is_sample_tokens():
    from test_hip_score import _model_bound
    m, idx, masked = _model_case()
    rows = masked.flatten().nonzero().flatten()
    start = idx.masked_fill(masked, MASK)
    out, lps = m.infill(idx, masked, steps=1, temperature=1.0, seed=11, mask_token=MASK)
    tok, lp = m.sample_tokens(start, rows, temperature=1.0, seed=11)
    assert out.shape == idx.shape and out.dtype == torch.int64 and lps.shape == idx.shape and lps.dtype == torch.float32
    assert tok.shape == lp.shape == (26,) and tok.dtype == torch.int64 and lp.dtype == torch.float32
    assert torch.equal(out.flatten()[rows], tok)
    assert_same_bits(lps.flatten()[rows], lp, "log-probabilities")
    assert torch.equal(out[~masked], idx[~masked]) and bool((lps[~masked] == 0).all())
    with torch.no_grad():
        emb = m(start, return_embeddings=True, rows=rows)
    bound = _model_bound(m, emb, tok).squeeze(1)
    ref = m.token_logprobs(start, rows, tok)
    frac = ((lp.double() - ref.double()).abs() / bound).max().item()
    print(f"the largest difference from token_logprobs is {frac:.3f} of its bound")
    assert frac <= 1, frac
    # with a set and a temperature: the same identity, inside the set
    allowed = list(range(10, 60))
    out2, lps2 = m.infill(idx, masked, steps=1, temperature=0.7, seed=11, allowed_tokens=allowed, mask_token=MASK)
    tok2, lp2 = m.sample_tokens(start, rows, temperature=0.7, seed=11, allowed_tokens=allowed)
    assert torch.equal(out2.flatten()[rows], tok2) and bool(((tok2 >= 10) & (tok2 < 60)).all())
    assert_same_bits(lps2.flatten()[rows], lp2, "log-probabilities over a set")


@pytest.mark.parametrize("order", ["confidence", "random", "left"])
def test_infill_over_several_steps(order):
    m, idx, masked = _model_case()
    allowed = torch.zeros(300, dtype=torch.bool)
    allowed[20:120] = True
    was = m.training
    m.train()
    try:
        for steps in (4, 100):
            out, lps = m.infill(idx, masked, steps=steps, temperature=0.9, order=order, seed=5, allowed_tokens=allowed, mask_token=MASK)
            assert torch.equal(out[~masked], idx[~masked]) and not bool((out[masked] == MASK).any())
            assert bool(((out[masked] >= 20) & (out[masked] < 120)).all())
            assert bool((lps[~masked] == 0).all()) and bool(torch.isfinite(lps[masked]).all()) and bool((lps[masked] <= 0).all())
            again = m.infill(idx, masked, steps=steps, temperature=0.9, order=order, seed=5, allowed_tokens=allowed, mask_token=MASK)
            assert_same_bits(again[0], out, "the same seed: tokens")
            assert_same_bits(again[1], lps, "the same seed: log-probabilities")
            other = m.infill(idx, masked, steps=steps, temperature=0.9, order=order, seed=6, allowed_tokens=allowed, mask_token=MASK)
            assert not torch.equal(other[0], out)
        assert m.training
    finally:
        m.train(was)


def test_infill_left_to_right_greedy_is_a_plain_loop():
    """order "left", steps >= the largest masked count, temperature 0: one position per sequence and iteration, the lowest first — the
    same kernels on the same states as this loop over sample_tokens, so the match is exact"""
    m, idx, masked = _model_case()
    out, lps = m.infill(idx, masked, steps=17, temperature=0, order="left", seed=1, mask_token=MASK)
    cur = idx.masked_fill(masked, MASK)
    want_lp = torch.zeros(idx.shape, dtype=torch.float32, device=DEV)
    left = masked.clone()
    T = idx.shape[1]
    while bool(left.any()):
        rows = left.flatten().nonzero().flatten()
        tok, lp = m.sample_tokens(cur, rows, temperature=0, seed=1)
        firsts = [int(left[b].nonzero()[0]) + b * T for b in range(idx.shape[0]) if bool(left[b].any())]
        for pos in firsts:
            at = int((rows == pos).nonzero()[0])
            cur.view(-1)[pos] = tok[at]
            want_lp.view(-1)[pos] = lp[at]
            left.view(-1)[pos] = False
    assert torch.equal(out, cur)
    assert_same_bits(lps, want_lp, "log-probabilities")
