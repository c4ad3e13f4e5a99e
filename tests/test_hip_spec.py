"""obte_spec_verify_bf16 (csrc/spec_verify.hip) against the rule's plain-torch statement, sampling.verify_reference, in float64, and
OmniBioTA.generate_speculative on top of it.

The kernel's integers are exact; what is bounded is their distance from the float64 reference, by test_hip_sample.py's DELTA = 1e-5 and
its derivation (2^-40 fixed-point weights, a hardware exp2 good to about one fp32 ulp):
  kept sets   the kernel's kept count of a row is what ops.sample_logits reports for it (the same integers).  Top-k alone: equal to the
              reference's; with top-p bracketed by the reference's at p -+ DELTA.  The reference distributions P_j, Q_j are then rebuilt
              from the kernel's own counts.
  accepted    every accepted position j has u_accept[j] <= P_j(x_j) / Q_j(x_j) + DELTA, the first rejected one u_accept[j] >= ratio - DELTA.
  token       at the kernel's own a, u_draw lies in the reference's interval of the token: within DELTA for the bonus draw (a == k) and
              within DELTA / Z for a residual draw, Z = sum max(0, P_a - Q_a) the reference's residual mass — the residual renormalises
              by it.  The inputs are built so that Z >= 0.05 in every row, which is asserted.
The largest deviations seen are printed (DESIGN 14.6 records them)."""
import pytest
import torch

from fenced import assert_guards, assert_same_bits, fenced

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16
DELTA = 1e-5
MIN_Z = 0.05
NAN, INF = float("nan"), float("inf")
SETTINGS = [dict(), dict(T=0.8), dict(k=50), dict(p=0.9), dict(T=0.8, k=50, p=0.9), dict(k=1)]


def _ops():
    from omnibiote_amd import ops
    return ops


def _S():
    from omnibiote_amd import sampling
    return sampling


def _in_ld(x):
    """x (B, r, V) copied into rows of ld = V rounded up to 8, the columns behind V holding 100, above every logit: a (B, r, V) view"""
    B, r, V = x.shape
    buf = torch.full((B * r, (V + 7) // 8 * 8), 100.0, dtype=BF, device=DEV)
    buf[:, :V] = x.reshape(B * r, V).to(DEV)
    return buf[:, :V].unflatten(0, (B, r))


def _raw_inputs(B, k, V, seed, related=False, s=2.0):
    """p (B, k + 1, V), q (B, k, V) bf16 and the uniforms (draws (k, B), u_accept (B, k), u_draw (B,)) from a CPU generator, on the CPU:
    q independent of p, or with ``related`` p's first k rows plus noise of half their spread — drafts that are often accepted.  In every
    draft row the column of the target's maximum then trades places with the row's own minimum: the residual keeps at least about the
    target's largest probability, whatever the cuts leave of either row (Z >= 0.05 was checked on the CPU for every case below)"""
    g = torch.Generator().manual_seed(seed)
    p = torch.randn(B, k + 1, V, generator=g) * s
    q = torch.randn(B, k, V, generator=g) * s
    if related:
        q = p[:, :k] + 0.5 * q
    p, q = p.to(BF), q.to(BF)
    c, d = p[:, :k].float().argmax(dim=2, keepdim=True), q.float().argmin(dim=2, keepdim=True)
    qc, qd = q.gather(2, c), q.gather(2, d)
    q = q.scatter(2, c, qd).scatter(2, d, torch.where(c == d, qd, qc))
    return p, q, torch.rand(k, B, generator=g), torch.rand(B, k, generator=g), torch.rand(B, generator=g)


def _inputs(*a, **kw):
    """_raw_inputs on the device, the logits inside rows of ld = V rounded up to 8"""
    p, q, *us = _raw_inputs(*a, **kw)
    return (_in_ld(p), _in_ld(q)) + tuple(u.to(DEV) for u in us)


def _drafts(q, draws, T=1.0, k=None, p=None):
    """x (B, k): position j drawn from q[:, j] by the device sampler under the same settings"""
    return torch.stack([_ops().sample_logits(q[:, j], draws[j], T, k, p) for j in range(q.shape[1])], dim=1)


def _lowest_argmax(x):
    """(rows, V) -> the lowest index of every row's maximum over its entries above -inf that are not NaN (0 for a row with none)"""
    xs = x.float()
    xs = torch.where(torch.isnan(xs), torch.full_like(xs, -INF), xs)
    m = xs.max(dim=1, keepdim=True).values
    return torch.where(m.squeeze(1) > -INF, ((xs == m) & (xs > -INF)).to(torch.uint8).argmax(dim=1), 0)


def _greedy_walk(p, x):
    B, k = x.shape
    top = _lowest_argmax(p.reshape(B * (k + 1), -1)).view(B, k + 1)
    a = (x == top[:, :k]).long().cumprod(dim=1).sum(dim=1)
    return a, top[torch.arange(B, device=p.device), a]


def _check(p, q, x, ua, ud, T=1.0, k=None, p_=None, what="", min_z=MIN_Z):
    """one call against the reference; returns (largest excess of u_accept over its bound, largest deviation of u_draw from the token's
    reference interval in units of the allowance's numerator: times Z for a residual draw)"""
    S = _S()
    B, K, V = p.shape[0], p.shape[1] - 1, p.shape[2]
    n_acc, tok = _ops().spec_verify(p, q, x, ua, ud, T, k, p_)
    assert n_acc.dtype == torch.int32 and tok.dtype == torch.int64 and n_acc.shape == tok.shape == (B,), what
    assert ((n_acc >= 0) & (n_acc <= K)).all() and ((tok >= 0) & (tok < V)).all(), what
    a = n_acc.long()
    rows = torch.arange(B, device=DEV)
    if ua is None or k == 1 or T == 0:
        want_a, want_tok = _greedy_walk(p, x)
        assert torch.equal(a, want_a) and torch.equal(tok, want_tok), what
        return 0.0, 0.0
    # the kernel's kept sets, bracketed by the reference's
    p2, q2 = p.flatten(0, 1), q.flatten(0, 1)
    half = torch.full((B * (K + 1),), 0.5, device=DEV)
    counts = []
    for rows2 in (p2, q2):
        n = _ops().sample_logits(rows2, half[:rows2.shape[0]], T, k, p_, return_kept=True)[1].long()
        if p_ is None or p_ >= 1:
            assert torch.equal(n, S.sample_reference(rows2, 0.5, T, k, None)[1]), what
        else:
            lo, hi = S.sample_reference(rows2, 0.5, T, k, max(p_ - DELTA, 1e-300))[1], S.sample_reference(rows2, 0.5, T, k, min(p_ + DELTA, 1.0))[1]
            assert ((lo <= n) & (n <= hi)).all(), what
        counts.append(n)
    P, Q = S.verify_distributions(p, q, T, n_kept_p=counts[0].view(B, K + 1), n_kept_q=counts[1].view(B, K))
    inside = (x >= 0) & (x < V)
    xc = x.clamp(0, V - 1).unsqueeze(2)
    px = torch.where(inside, P[:, :K].gather(2, xc).squeeze(2), 0.0)
    qx = torch.where(inside, Q.gather(2, xc).squeeze(2), 0.0)
    ratio = torch.where(px > 0, torch.where(qx > 0, px / qx.clamp(min=1e-300), INF), 0.0)
    uac = ua.double()
    uac = torch.where(uac > 0, uac, torch.zeros_like(uac))
    j = torch.arange(K, device=DEV).unsqueeze(0)
    acc, rej = j < a.unsqueeze(1), j == a.unsqueeze(1)
    over = torch.where(acc, uac - ratio, torch.where(rej, ratio - uac, -INF)).max()
    assert over <= DELTA, (what, float(over))
    # the token, in the reference's distribution at the kernel's own a
    pa = P[rows, a]
    res = torch.where((a < K).unsqueeze(1), (pa - Q[rows, a.clamp(max=K - 1)]).clamp(min=0), 0.0)
    z = res.sum(dim=1)
    if min_z is not None:
        assert (z[a < K] >= min_z).all(), (what, float(z[a < K].min()))
    w = torch.where((z > 0).unsqueeze(1), res, pa)
    cdf = w.cumsum(dim=1) / w.sum(dim=1, keepdim=True).clamp(min=1e-300)
    some = w.sum(dim=1) > 0
    assert (tok[~some] == 0).all() and (w.gather(1, tok.unsqueeze(1)).squeeze(1) > 0)[some].all(), what   # an entry of non-zero reference weight
    udc = ud.double()
    udc = torch.where(udc > 0, udc, torch.zeros_like(udc)).clamp(max=1.0)
    above = cdf.gather(1, tok.unsqueeze(1)).squeeze(1)
    below = torch.where(tok > 0, cdf.gather(1, (tok - 1).clamp(min=0).unsqueeze(1)).squeeze(1), torch.zeros_like(above))
    dev = torch.maximum(below - udc, udc - above).clamp(min=0) * torch.where(z > 0, z, torch.ones_like(z))
    dev = dev[some]
    worst = float(dev.max()) if dev.numel() else 0.0
    assert worst <= DELTA, (what, worst)
    return max(float(over), 0.0), worst


def _run_settings(B, k, V, seed, related):
    p, q, draws, ua, ud = _inputs(B, k, V, seed, related)
    worst, accepted = [0.0, 0.0], 0
    for kw in SETTINGS:
        T, tk, tp = kw.get("T", 1.0), kw.get("k"), kw.get("p")
        x = _drafts(q, draws, T, tk, tp)
        if tk == 1:
            x[::2] = _lowest_argmax(p.flatten(0, 1)).view(B, k + 1)[::2, :k]   # every other row drafts the target's own argmax: it stands
        got = _check(p, q, x, ua, ud, T, tk, tp, what=f"B={B} k={k} V={V} related={related} {kw}")
        worst = [max(a, b) for a, b in zip(worst, got)]
        accepted += int(_ops().spec_verify(p, q, x, ua, ud, T, tk, tp)[0].sum())
    return worst, accepted


@pytest.mark.parametrize("k", [1, 4, 31])
@pytest.mark.parametrize("B", [1, 3, 65])
@pytest.mark.parametrize("V", [8, 1003, 2049])
def test_spec_verify_matches_the_reference(V, B, k):
    w1, a1 = _run_settings(B, k, V, 100 * V + 10 * B + k, False)
    w2, a2 = _run_settings(B, k, V, 100 * V + 10 * B + k + 5, True)
    print(f"spec_verify V={V} B={B} k={k}: u_accept over its bound by at most {max(w1[0], w2[0]):.3g}, u_draw outside the token's interval by "
          f"at most {max(w1[1], w2[1]):.3g} (x Z); accepted {a1} (independent q) and {a2} (related q) of {6 * B * k} each")


@pytest.mark.parametrize("B,k", [(1, 4), (3, 31), (65, 1)])
def test_spec_verify_at_the_widest_vocabulary(B, k):
    w1, a1 = _run_settings(B, k, 65536, 7 * B + k, False)
    w2, a2 = _run_settings(B, k, 65536, 7 * B + k + 1, True)
    print(f"spec_verify V=65536 B={B} k={k}: u_accept over its bound by at most {max(w1[0], w2[0]):.3g}, u_draw outside the token's interval "
          f"by at most {max(w1[1], w2[1]):.3g} (x Z); accepted {a1} and {a2} of {6 * B * k}")


# =================================================================================================== exact cases
@pytest.mark.parametrize("V,B,k", [(1003, 3, 4), (2049, 65, 1), (65536, 2, 31), (8, 5, 31)])
def test_a_draft_that_is_the_target_is_accepted_whole_and_the_bonus_is_the_samplers_token(V, B, k):
    ops = _ops()
    p, _, draws, ua, ud = _inputs(B, k, V, V + k)
    q = _in_ld(p[:, :k])                                                 # a bitwise copy of p's first k rows
    for kw in SETTINGS[:5]:
        T, tk, tp = kw.get("T", 1.0), kw.get("k"), kw.get("p")
        x = _drafts(q, draws, T, tk, tp)
        for u in (ua, torch.full_like(ua, 0.99999994), torch.zeros_like(ua)):
            n, tok = ops.spec_verify(p, q, x, u, ud, T, tk, tp)
            assert (n == k).all(), (kw, n.tolist())
            assert_same_bits(tok, ops.sample_logits(p[:, k], ud, T, tk, tp), f"bonus token {kw}")
    n, tok = ops.spec_verify(p, q, x, torch.ones_like(ua), ud)           # ratio 1 exactly: u = 1 is not below it; Z = 0, the draw is from P_0
    assert (n == 0).all()
    assert_same_bits(tok, ops.sample_logits(p[:, 0], ud), "P_0 when the residual is empty")


def test_tokens_the_target_does_not_keep_and_tokens_out_of_range_are_rejected():
    ops = _ops()
    B, k, V = 4, 6, 1003
    p, q, draws, ua, ud = _inputs(B, k, V, 77)
    zero = torch.zeros_like(ua)                                          # u = 0: whatever the target keeps stands
    x = _lowest_argmax(p.flatten(0, 1)).view(B, k + 1)[:, :k].clone()    # the target's favourites
    n, _ = ops.spec_verify(p, q, x, zero, ud, 1.0, 50)
    assert (n == k).all()
    at = [0, 2, 5, 3]
    order = p[:, :k].float().argsort(dim=2, descending=True)
    for rank, want_in in ((49, True), (99, False), (V - 1, False)):
        y = x.clone()
        for b, j in enumerate(at):
            y[b, j] = order[b, j, rank]
        n, tok = ops.spec_verify(p, q, y, zero, ud, 1.0, 50)
        assert n.tolist() == ([k] * B if want_in else at), (rank, n.tolist())
        if not want_in:
            assert (tok != y[torch.arange(B), at]).all()                 # and what the target does not keep is not drawn in its place
    for bad in (-1, V, V + 7, 2 ** 62, -2 ** 63):
        y = x.clone()
        for b, j in enumerate(at):
            y[b, j] = bad
        for kw in (dict(), dict(top_k=50), dict(temperature=0.8, top_p=0.9)):
            n, tok = ops.spec_verify(p, q, y, zero, ud, **kw)
            assert n.tolist() == at and ((tok >= 0) & (tok < V)).all(), (bad, kw)
        n, tok = ops.spec_verify(p, None, y)                             # greedy
        assert n.tolist() == at and torch.equal(tok, _lowest_argmax(p[torch.arange(B), at]))


@pytest.mark.parametrize("V", [8, 1003, 2049, 65536])
def test_greedy_is_the_lowest_argmax_walk(V):
    ops = _ops()
    B, k = 5, 4
    p, q, draws, ua, ud = _inputs(B, k, V, 3 * V)
    if V > 8:
        p[0, 1, 3] = p[0, 1, V - 1] = 50.0                               # ties for the maximum: the lower index is the argmax
        p[1, 4, V // 2] = p[1, 4, V // 2 + 1] = 50.0
        p[2, 2, :] = -3.0
    p[3, 0, :] = NAN                                                     # nothing to take a maximum of: index 0
    top = _lowest_argmax(p.flatten(0, 1)).view(B, k + 1)
    x = top[:, :k].clone()
    x[0, 3] += 1                                                         # row 0: three stand
    if V > 8:
        x[1, 1] = V - 1
        x[0, 1] = 3
    want = _greedy_walk(p, x)
    for kw in (dict(), dict(u_accept=ua, u_draw=ud, top_k=1), dict(u_accept=ua, u_draw=ud, temperature=0), dict(top_k=7, top_p=0.3)):
        for qq in (q, None):
            n, tok = ops.spec_verify(p, qq, x, **kw)
            assert torch.equal(n.long(), want[0]) and torch.equal(tok, want[1]), (V, kw)
    assert int(want[0][0]) == 3 and int(want[0][4]) == k


# =================================================================================================== robustness
@pytest.mark.parametrize("B,k,V", [(64, 3, 1003), (3, 4, 65536), (5, 31, 12000)])
def test_any_bit_pattern_is_safe(B, k, V):
    ops = _ops()
    g = torch.Generator(device=DEV).manual_seed(B + V)
    ld = (V + 7) // 8 * 8

    def bits16(r):
        return torch.randint(-32768, 32768, (B * r, ld), device=DEV, generator=g, dtype=torch.int32).to(torch.int16).view(BF)[:, :V].unflatten(0, (B, r))

    def bits32(*shape):
        return torch.randint(-2 ** 31, 2 ** 31, shape, device=DEV, generator=g, dtype=torch.int64).to(torch.int32).view(torch.float32)

    p, q, ua, ud = bits16(k + 1), bits16(k), bits32(B, k), bits32(B)
    p[0, 1] = NAN
    q[0, 0] = -INF
    p[-1] = -INF
    x = torch.randint(-2 ** 63, 2 ** 63 - 1, (B, k), device=DEV, generator=g, dtype=torch.int64)
    x[:, ::2] = torch.randint(0, V, (B, (k + 1) // 2), device=DEV, generator=g)
    for kw in (dict(), dict(top_k=40), dict(top_p=0.7), dict(top_k=300, top_p=0.2, temperature=0.01), dict(temperature=1e-30), dict(temperature=1e30, top_p=0.5),
               dict(top_k=1)):
        n, tok = ops.spec_verify(p, q, x, ua, ud, **kw)
        assert ((n >= 0) & (n <= k)).all() and ((tok >= 0) & (tok < V)).all(), kw
        assert int(n[0]) <= 1 or kw == dict(top_k=1)                     # nothing of an all-NaN target row is kept
        n2, tok2 = ops.spec_verify(p, q, x, ua, ud, **kw)
        assert torch.equal(n, n2) and torch.equal(tok, tok2), kw


def test_repeatable_and_a_row_depends_on_itself_alone():
    ops = _ops()
    for V, k in ((1003, 4), (65536, 2)):
        B = 65
        p, q, draws, ua, ud = _inputs(B, k, V, 31, related=True)
        for kw in (dict(), dict(top_k=50), dict(temperature=0.8, top_k=200, top_p=0.5), dict(top_k=1)):
            x = _drafts(q, draws, kw.get("temperature", 1.0), kw.get("top_k"), kw.get("top_p"))
            a = ops.spec_verify(p, q, x, ua, ud, **kw)
            b = ops.spec_verify(p, q, x, ua, ud, **kw)
            assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), (V, kw)
            for r in (0, 17, 64):
                one = ops.spec_verify(p[r:r + 1], q[r:r + 1], x[r:r + 1], ua[r:r + 1], ud[r:r + 1], **kw)
                assert int(one[0]) == int(a[0][r]) and int(one[1]) == int(a[1][r]), (V, kw, r)


def test_fenced_buffers_are_respected():
    """p and q at 16-byte-and-no-more alignment, V = 1003 in ld = 1008, NaN poison behind every row and around the payloads; the drafts,
    the uniforms, both outputs and the workspace inside marked guards: bit-equal to the plain call, guards untouched, and the workspace
    written inside obte_spec_verify_ws_bytes alone"""
    from omnibiote_amd import _lib
    B, k, V, ld = 9, 4, 1003, 1008
    p, q, draws, ua, ud = _inputs(B, k, V, 51, related=True)
    x = _drafts(q, draws)
    x[1, 2], x[3, 0] = V, -1
    pf, hp = fenced(p.flatten(0, 1), poison="nan", ld=ld)
    qf, hq = fenced(q.flatten(0, 1), poison="nan", ld=ld)
    xf, hx = fenced(x, poison="mark")
    af, ha = fenced(ua, poison="nan")
    df, hd = fenced(ud, poison="nan")
    assert pf.data_ptr() % 32 == 16 and pf.stride(0) == ld and qf.data_ptr() % 32 == 16
    need = _lib.lib().obte_spec_verify_ws_bytes(B, k)
    assert need == B * (2 * k + 1) * 32
    for T, tk, tp in ((1.0, 0, 1.0), (0.8, 50, 1.0), (1.0, 0, 0.9), (0.8, 200, 0.5), (1.0, 1, 1.0)):
        nf, hn = fenced((B,), dtype=torch.int32, poison="mark")
        tf, ht = fenced((B,), dtype=torch.int64, poison="mark")
        wf, hw = fenced((need,), dtype=torch.uint8, poison="mark")
        _lib.check(_lib.lib().obte_spec_verify_bf16(pf.data_ptr(), ld, qf.data_ptr(), ld, xf.data_ptr(), B, k, V, af.data_ptr(), df.data_ptr(), T, tk, tp,
                                                    nf.data_ptr(), tf.data_ptr(), wf.data_ptr(), need, torch.cuda.current_stream().cuda_stream),
                   "obte_spec_verify_bf16")
        n, tok = _ops().spec_verify(p, q, x, ua, ud, T, tk or None, tp)
        assert_same_bits(nf, n, f"n_accept {T} {tk} {tp}")
        assert_same_bits(tf, tok, f"token {T} {tk} {tp}")
        assert_guards(hp, hq, hx, ha, hd, hn, ht, hw)


# =================================================================================================== the distribution
DIST_SEED = 4


def _dist_case(device):
    """V = 16, k = 2, N = 16 384 batch rows sharing one (p, q); every uniform from one seeded CPU generator"""
    V, k, N = 16, 2, 16384
    g = torch.Generator().manual_seed(DIST_SEED)
    p = (torch.randn(1, k + 1, V, generator=g) * 1.5).to(BF)
    q = (torch.randn(1, k, V, generator=g) * 1.5).to(BF)
    draws, ua, ud = torch.rand(k, N, generator=g), torch.rand(N, k, generator=g), torch.rand(N, generator=g)
    p, q = p.expand(N, k + 1, V).contiguous(), q.expand(N, k, V).contiguous()
    return tuple(t.to(device) for t in (p, q, draws, ua, ud))


def _first_token_frequencies_are_the_targets(x0, a, tok, p):
    N, V = x0.shape[0], p.shape[2]
    first = torch.where(a >= 1, x0, tok)
    f = torch.bincount(first, minlength=V).double() / N
    P0 = torch.softmax(p[0, 0].double(), dim=0)
    bound = 5 * torch.sqrt(P0 * (1 - P0) / N) + 1.0 / N
    return (f - P0).abs(), bound


def test_the_first_emitted_token_has_the_targets_distribution():
    """x_0 if it stands, else the verified token, is distributed as P_0 whatever the draft: |f_i - P_0(i)| <= 5 sqrt(P_0(i) (1 - P_0(i)) / N)
    + 1 / N in every bin.  DIST_SEED is one for which the reference itself, run on the CPU on the same uniforms, is inside the bound."""
    S = _S()
    p, q, draws, ua, ud = _dist_case("cpu")
    x = torch.stack([S.sample_reference(q[:, j], draws[j])[0] for j in range(2)], dim=1)
    a, tok, _ = S.verify_reference(p, q, x, ua, ud)
    d, bound = _first_token_frequencies_are_the_targets(x[:, 0], a, tok, p)
    assert (d <= bound).all(), "the reference itself misses the bound under this seed"
    p, q, draws, ua, ud = _dist_case(DEV)
    x = _drafts(q, draws)
    n, tok = _ops().spec_verify(p, q, x, ua, ud)
    d, bound = _first_token_frequencies_are_the_targets(x[:, 0], n.long(), tok, p)
    print(f"first emitted token over 16384 rows: largest |f - P_0| {float(d.max()):.3g}, the tightest bound {float(bound.min()):.3g}; "
          f"accepted {float(n.float().mean()):.3f} of 2 on average")
    assert (d <= bound).all(), (d / bound).max()


# =================================================================================================== the loop
LOGITS_BAR = 5e-3                                                         # the generation tests' bar on logits


def _case(C=256):
    from test_hip_generate import _gen_case
    return _gen_case(C)                                                  # block 200, vocabulary 512, 2 layers: built once per session


_small = {}


def _one_layer_draft():
    """a 1-layer model of width 128 with weights of its own over the same vocabulary"""
    if not _small:
        import omnibiote_ref as R
        from test_hip_causal import _model
        cfg = R.RefConfig(block_size=200, vocab_size=512, n_layer=1, n_head=2, n_embd=128)
        _small["m"] = _model(cfg, R.hash_weights(cfg, seed=3), True)
    return _small["m"]


def _gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


def _teacher_forced(m, out, t0, steps):
    """the target's logits behind positions t0 - 1 .. t0 + steps - 2 from ONE full causal forward over `out`: entry i predicts token t0 + i"""
    with torch.no_grad():
        return m(out[:, :t0 + steps]).float()[:, t0 - 1:t0 + steps - 1]


@pytest.mark.parametrize("C", [256, 128])
def test_greedy_self_draft_follows_the_full_forward(C):
    from omnibiote_amd.model import KVCache
    c = _case(C)
    m, idx = c["m"], c["ids"][:, :100].to(DEV)
    out, stats = m.generate_speculative(idx, 24, m, k=4, top_k=1, return_stats=True)
    assert out.shape == (2, 124) and out.dtype == torch.int64 and torch.equal(out[:, :100], idx)
    at = _teacher_forced(m, out, 100, 24)
    gap = at.max(dim=-1).values - at.gather(-1, out[:, 100:].unsqueeze(-1)).squeeze(-1)
    print(f"greedy self-draft, C={C}: largest logit gap to the full forward's maximum {gap.max().item():.4g}; {stats}")
    assert (gap <= 2 * LOGITS_BAR).all(), gap.max().item()
    assert 4 * stats["rounds"] <= stats["drafted"] <= 2 * 4 * stats["rounds"] and 2 * stats["accepted"] >= stats["drafted"], stats
    assert 2 * 24 <= stats["accepted"] + 2 * (stats["rounds"] + 1), stats   # a row emits its first token, then per round what stood and one more
    # one round by hand: both caches end at prompt + emitted - 1 (the last emitted token is pending, in neither cache)
    cache, dcache = KVCache(m, 2), KVCache(m, 2)
    pending = _ops().sample_logits(m.prefill(idx, cache, lengths=[100, 100]), None)
    m.prefill(idx, dcache, lengths=[100, 100])
    emitted = [1, 1]
    for _ in range(2):
        x, n, tok = m.draft_and_verify(m, pending, cache, dcache, 4)
        assert cache.positions.tolist() == dcache.positions.tolist() == [100 + e - 1 + 5 for e in emitted]
        a = n.tolist()
        for kv in (cache, dcache):
            kv.rewind_rows([4 - v for v in a], now=[100 + e - 1 + 5 for e in emitted])
        emitted = [e + v + 1 for e, v in zip(emitted, a)]
        assert cache.positions.tolist() == dcache.positions.tolist() == [100 + e - 1 for e in emitted]
        assert cache.pos == dcache.pos == max(cache.positions.tolist()) and cache.min_pos == min(cache.positions.tolist())
        pending = tok
    assert sum(emitted) >= 2 + 8 + 4                                     # (at least half of the 16 drafted stood, and one more per row and round)


def _kept(logits, T, k, bar):
    """the reference's kept set of every row, the threshold loosened by `bar`: what a path whose logits lie within bar / 2 of these may keep"""
    n = _S().sample_reference(logits, 0.5, T, k, None)[1]
    xd = logits.double()
    thr = xd.sort(dim=1, descending=True).values.gather(1, (n - 1).unsqueeze(1))
    return xd >= thr - bar


def test_sampled_run_with_a_smaller_draft_is_seeded_and_stays_in_the_targets_kept_set():
    c = _case(256)
    m, d, idx = c["m"], _one_layer_draft(), c["ids"][:, :100].to(DEV)
    kw = dict(k=4, temperature=0.9, top_k=50, return_stats=True)
    a, sa = m.generate_speculative(idx, 24, d, generator=_gen(11), **kw)
    b, sb = m.generate_speculative(idx, 24, d, generator=_gen(11), **kw)
    other, _ = m.generate_speculative(idx, 24, d, generator=_gen(12), **kw)
    assert a.shape == (2, 124) and a.dtype == torch.int64 and torch.equal(a, b) and sa == sb and torch.equal(a[:, :100], idx)
    assert not torch.equal(a, other)
    at = _teacher_forced(m, a, 100, 24)
    for i in range(24):
        assert _kept(at[:, i], 0.9, 50, 2 * LOGITS_BAR).gather(1, a[:, 100 + i].unsqueeze(1)).all(), i
    print(f"sampled run, 1-layer draft: {sa}")
    assert 4 * sa["rounds"] <= sa["drafted"] <= 2 * 4 * sa["rounds"] and 0 <= sa["accepted"] <= sa["drafted"]
    assert 2 * 24 <= sa["accepted"] + 2 * (sa["rounds"] + 1), sa            # accepted + one per row and round (and the first) >= tokens emitted
    assert sa["rounds"] >= 5                                             # at most k + 1 = 5 tokens per round behind the first


def test_ragged_prompts_eos_and_the_trim():
    from test_hip_generate_rows import LENS, _ragged_prompt
    c = _case(256)
    m, d, idx = c["m"], _one_layer_draft(), _ragged_prompt(c)
    kw = dict(k=4, temperature=0.9, top_k=50, lengths=LENS)
    free, nf = m.generate_speculative(idx, 24, d, generator=_gen(11), **kw)
    again, _ = m.generate_speculative(idx, 24, d, generator=_gen(11), **kw)
    assert free.shape == (2, max(LENS) + 24) and free.dtype == torch.int64 and nf.tolist() == [a + 24 for a in LENS] and torch.equal(free, again)
    for b, a in enumerate(LENS):
        assert torch.equal(free[b, :a], idx[b, :a]) and (free[b, a + 24:] == 0).all()
        at = _teacher_forced(m, free[b:b + 1], a, 24)
        for i in range(24):
            assert _kept(at[:, i], 0.9, 50, 2 * LOGITS_BAR)[0, int(free[b, a + i])], (b, i)
    # EOS: row 0's fourth token — with k = 4 it falls inside a round, or is that round's last
    eos = int(free[0, LENS[0] + 3])
    first = [int((free[b, a:a + 24] == eos).nonzero().flatten()[0]) + 1 if (free[b, a:a + 24] == eos).any() else 24 for b, a in enumerate(LENS)]
    out, n, stats = m.generate_speculative(idx, 24, d, generator=_gen(11), eos_token=eos, pad_token=3, return_stats=True, **kw)
    assert n.tolist() == [a + f for a, f in zip(LENS, first)] and first[0] <= 4      # the same stream up to each row's EOS
    assert out.shape == (2, max(LENS) + max(first))
    for b, a in enumerate(LENS):
        assert torch.equal(out[b, :a + first[b]], free[b, :a + first[b]]) and (out[b, a + first[b]:] == 3).all()
    # equal lengths: a finished row is filled with the EOS, the other runs to max_new_tokens; 7 = 1 + 5 + 1 is trimmed inside a round
    idx2 = c["ids"][:, :100].to(DEV)
    for new in (7, 24):
        plain = m.generate_speculative(idx2, new, d, k=4, temperature=0.9, top_k=50, generator=_gen(5))
        assert plain.shape == (2, 100 + new)
        if new == 24:
            assert torch.equal(plain[:, :107], short)                    # the trim cuts the stream, it does not change it
        short = plain
    eos = int(plain[1, 102])
    got = m.generate_speculative(idx2, 24, d, k=4, temperature=0.9, top_k=50, generator=_gen(5), eos_token=eos)
    assert got.shape == (2, 124)
    for b in range(2):
        hit = (plain[b, 100:] == eos).nonzero().flatten()
        end = 100 + int(hit[0]) + 1 if hit.numel() else 124
        assert torch.equal(got[b, :end], plain[b, :end]) and (got[b, end:] == eos).all()
