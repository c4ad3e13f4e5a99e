"""obte_sample_logits_bf16 (csrc/sample.hip) against the rule's plain-torch statement, sampling.sample_reference, in float64.

The comparison is exact in its integers and bounded in its one floating-point quantity:
  kept count  top-k alone: equal to the reference's.  With top-p the threshold is monotone in p, so n_ref(p - DELTA) <= n_kept <=
              n_ref(p + DELTA) — a row's deciding mass may lie closer to p than either side's rounding (5e-7 was seen), so equality
              would be the wrong test.
  token       with the kept set rebuilt from the kernel's own count, token t satisfies cdf_ref[t - 1] - DELTA <= u <= cdf_ref[t] + DELTA
              and is a kept entry of non-zero reference weight.
DELTA = 1e-5 is derived, not tuned: 40-bit fixed-point weights and a hardware exp2 good to about one fp32 ulp bound a cumulative
probability's error by about 65536 * 2^-40 + 1.2e-7 = 2e-7 (fp32 tree sums of 65 536 terms would stay near 1e-6); DELTA leaves an order
of magnitude over either.  The largest deviation seen is printed by every test (DESIGN 14.3 records it)."""
import pytest
import torch

from fenced import assert_guards, assert_same_bits, fenced

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16
DELTA = 1e-5
NAN, INF = float("nan"), float("inf")


def _ops():
    from omnibiote_amd import ops
    return ops


def _ref(*a, **kw):
    from omnibiote_amd.sampling import sample_reference
    return sample_reference(*a, **kw)


def _logits(B, V, s, seed):
    """randn * s rounded to bf16, (B, V) inside rows of ld = V rounded up to 8; the columns behind V hold 100, above every logit"""
    ld = (V + 7) // 8 * 8
    buf = (torch.randn(B, ld, device=DEV, generator=torch.Generator(device=DEV).manual_seed(seed)) * s).to(BF)
    buf[:, V:] = 100.0
    return buf[:, :V]


def _in_ld(x):
    """x (B, V) copied into rows of ld = V rounded up to 8"""
    B, V = x.shape
    buf = torch.full((B, (V + 7) // 8 * 8), 100.0, dtype=BF, device=DEV)
    buf[:, :V] = x
    return buf[:, :V]


def _rand(B, seed):
    return torch.rand(B, device=DEV, generator=torch.Generator(device=DEV).manual_seed(seed))


def _lowest_argmax(x):
    xs = x.float().cpu()
    xs = torch.where(torch.isnan(xs), torch.full_like(xs, -INF), xs)
    return (xs == xs.max(dim=1, keepdim=True).values).to(torch.uint8).argmax(dim=1)


def _check(x, u, T=1.0, k=None, p=None, what=""):
    """one launch against the reference; returns the largest deviation of u from the token's reference interval"""
    B, V = x.shape
    tok, n = _ops().sample_logits(x, u, T, k, p, return_kept=True)
    assert tok.dtype == torch.int64 and n.dtype == torch.int32 and tok.shape == n.shape == (B,)
    assert ((tok >= 0) & (tok < V)).all() and ((n >= 0) & (n <= V)).all(), what
    n = n.long()
    xd = x.double()
    valid = ~torch.isnan(xd) & (xd > -INF)
    some = valid.any(dim=1)
    assert torch.equal(n > 0, some) and (tok[~some] == 0).all(), what
    if u is None or k == 1 or T == 0:
        assert torch.equal(tok.cpu()[some.cpu()], _lowest_argmax(x)[some.cpu()]) and (n[some] == 1).all(), what
        return 0.0
    if p is None or p >= 1:
        assert torch.equal(n, _ref(x, u, T, k, None)[1]), what
    else:
        lo, hi = _ref(x, u, T, k, max(p - DELTA, 1e-300))[1], _ref(x, u, T, k, min(p + DELTA, 1.0))[1]
        assert ((lo <= n) & (n <= hi)).all(), (what, n.tolist()[:8], lo.tolist()[:8], hi.tolist()[:8])
    _, n2, cdf = _ref(x, u, T, n_kept=n)
    assert torch.equal(n2, n), what                                     # the count takes the threshold's tie whole
    xs = torch.where(valid, xd, torch.full_like(xd, -INF))
    thr = xs.sort(dim=1, descending=True).values.gather(1, (n - 1).clamp(min=0).unsqueeze(1)).squeeze(1)
    at = xs.gather(1, tok.unsqueeze(1)).squeeze(1)
    m = xs.max(dim=1).values
    weight = torch.where(at == m, torch.ones_like(at), torch.exp((at - m) / T))
    assert ((at >= thr) & (weight > 0))[some].all(), what               # a kept entry of non-zero reference weight
    uc = u.double()
    uc = torch.where(uc > 0, uc, torch.zeros_like(uc)).clamp(max=1.0)   # the rule's clamp (NaN: the first)
    above = cdf.gather(1, tok.unsqueeze(1)).squeeze(1)
    below = torch.where(tok > 0, cdf.gather(1, (tok - 1).clamp(min=0).unsqueeze(1)).squeeze(1), torch.zeros_like(above))
    dev = torch.maximum(below - uc, uc - above).clamp(min=0)[some]
    worst = float(dev.max()) if dev.numel() else 0.0
    assert worst <= DELTA, (what, worst)
    return worst


def _settings(V):
    return [dict(), dict(T=0.8), dict(k=1), dict(k=50), dict(k=V), dict(k=V + 5), dict(p=0.9), dict(p=1e-6), dict(k=200, p=0.5, T=0.8),
            dict(p=0.95, T=1.3)]


@pytest.mark.parametrize("B", [1, 3, 64, 65])
@pytest.mark.parametrize("V", [1, 7, 8, 1003, 4096, 65536])
def test_sample_logits_matches_the_reference(V, B):
    worst = 0.0
    for s in (2, 4):
        x = _logits(B, V, float(s), 1000 * s + V + B)
        for i, kw in enumerate(_settings(V)):
            u = _rand(B, 7 * V + 13 * B + i)
            worst = max(worst, _check(x, u, what=f"V={V} B={B} s={s} {kw}", **kw))
    print(f"sample_logits V={V} B={B}: largest deviation of u from the token's reference interval {worst:.3g}")


@pytest.mark.parametrize("V", [2041, 2048, 2049, 16377, 16384, 16385, 65529])
def test_widths_on_either_side_of_a_kernel_choice(V):
    """256 threads hold 2048 columns, 1024 threads 16 384 with two register groups and 65 536 with eight"""
    worst = 0.0
    x = _logits(3, V, 2.0, V)
    x[1, V - 1] = 40.0                                                   # the last column matters; the ones behind it (100) do not
    for i, kw in enumerate((dict(), dict(k=1), dict(k=50), dict(p=0.9), dict(k=200, p=0.5, T=0.8))):
        worst = max(worst, _check(x, _rand(3, V + i), what=f"V={V} {kw}", **kw))
    assert int(_ops().sample_logits(x, None)[1]) == V - 1
    print(f"sample_logits V={V}: largest deviation {worst:.3g}")


def test_u_grid_walks_the_whole_distribution():
    """one row, top_k = 16, u = (i + 1/2) / 4096: every kept entry of visible weight is drawn, in index order"""
    V, N = 1003, 4096
    x = _in_ld(_logits(1, V, 2.0, 5).expand(N, V))
    u = ((torch.arange(N, device=DEV, dtype=torch.float64) + 0.5) / N).float()
    worst = _check(x, u, k=16, what="u grid")
    tok = _ops().sample_logits(x, u, 1.0, 16)
    assert (tok[1:] >= tok[:-1]).all()                                   # the draw is monotone in u
    _, n, cdf = _ref(x[0], 0.5, top_k=16)
    w = torch.diff(cdf, prepend=torch.zeros(1, dtype=torch.float64, device=DEV))
    drawn = set(tok.tolist())
    assert set((w > 2.0 / N).nonzero().flatten().tolist()) <= drawn and len(drawn) <= int(n)   # an interval two grid steps long holds a grid point
    print(f"u grid: {len(set(tok.tolist()))} of {int(n)} kept entries drawn, largest deviation {worst:.3g}")


def _special_rows(V=1003):
    g = torch.Generator().manual_seed(17)
    rows = {}
    rows["one value"] = torch.full((V,), 1.5)
    r = torch.randn(V, generator=g) - 6.0
    r[:10] = 2.0
    r[100:400] = 1.0                                                     # the 11th .. 310th largest are one value
    rows["kth value shared by 300"] = r
    rows["all negative"] = -torch.rand(V, generator=g) * 30 - 1
    r = torch.randn(V, generator=g) * 2
    r[::3] = NAN
    r[1::7] = -INF
    rows["-inf and NaN entries"] = r
    rows["all NaN"] = torch.full((V,), NAN)
    rows["all -inf"] = torch.full((V,), -INF)
    r = torch.randn(V, generator=g) * 2
    r[[40, 900]] = INF
    rows["+inf twice"] = r
    r = -torch.rand(V, generator=g) * 5 - 1
    r[5] = 0.0
    r[6] = -0.0                                                          # one value: -0 counts as +0
    rows["zero of both signs on top"] = r
    return rows


def test_ties_and_special_rows():
    rows = _special_rows()
    names = list(rows)
    x = _in_ld(torch.stack([rows[k] for k in names]).to(BF).to(DEV))
    assert x.view(torch.int16)[names.index("zero of both signs on top"), 5:7].tolist() == [0, -32768]
    B, V = x.shape
    worst = 0.0
    us = [_rand(B, 3), _rand(B, 4)] + [torch.full((B,), v, device=DEV) for v in (0.0, 0.99999994, 1.0, -1.0, NAN, 0.5)]
    for u in us:
        for kw in (dict(), dict(T=0.7), dict(k=11), dict(k=200), dict(k=1), dict(p=0.9), dict(p=1e-6), dict(k=11, p=0.6), dict(k=400, p=0.999)):
            worst = max(worst, _check(x, u, what=f"special rows u={u[0].item()} {kw}", **kw))
    tok, n = _ops().sample_logits(x, us[0], 1.0, None, None, return_kept=True)
    got = dict(zip(names, zip(tok.tolist(), n.tolist())))
    assert got["one value"][1] == V and got["all NaN"] == (0, 0) and got["all -inf"] == (0, 0)
    r = rows["-inf and NaN entries"]
    assert got["+inf twice"][0] in (40, 900) and got["-inf and NaN entries"][1] == int((~torch.isnan(r) & (r > -INF)).sum())
    tok, n = _ops().sample_logits(x, us[0], 1.0, 11, None, return_kept=True)
    assert int(n[names.index("kth value shared by 300")]) == 310 and int(n[names.index("one value")]) == V
    tok, n = _ops().sample_logits(x, us[0], 1.0, None, 1e-6, return_kept=True)
    assert int(n[names.index("zero of both signs on top")]) == 2 and int(tok[names.index("zero of both signs on top")]) in (5, 6)
    # one value everywhere: the draw is uniform by the interval rule, token = floor(u V) up to the fixed point's last place
    u = _rand(B, 9)
    t = _ops().sample_logits(_in_ld(x[:1].expand(B, V)), u)
    assert ((t.double() - torch.floor(u.double() * V)).abs() <= 1).all()
    print(f"special rows: largest deviation {worst:.3g}")


@pytest.mark.parametrize("B,V", [(64, 1003), (3, 65536), (5, 12000)])
def test_any_bit_pattern_is_safe(B, V):
    g = torch.Generator(device=DEV).manual_seed(B + V)
    ld = (V + 7) // 8 * 8
    x = torch.randint(-32768, 32768, (B, ld), device=DEV, generator=g, dtype=torch.int32).to(torch.int16).view(BF)[:, :V]
    u = torch.randint(-2 ** 31, 2 ** 31, (B,), device=DEV, generator=g, dtype=torch.int64).to(torch.int32).view(torch.float32)
    for kw in (dict(), dict(k=40), dict(p=0.7), dict(k=300, p=0.2, T=0.01), dict(T=1e-30), dict(T=1e30, p=0.5)):
        _check(x, u, what=f"bits B={B} V={V} {kw}", **kw)


def test_repeatable_and_a_row_depends_on_itself_alone():
    ops = _ops()
    for V in (1003, 65536):
        x, u = _logits(64, V, 2.0, 31), _rand(64, 32)
        for kw in (dict(), dict(top_k=50), dict(top_p=0.9), dict(temperature=0.8, top_k=200, top_p=0.5)):
            a = ops.sample_logits(x, u, return_kept=True, **kw)
            b = ops.sample_logits(x, u, return_kept=True, **kw)
            assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), (V, kw)
            for r in (0, 17, 63):
                one = ops.sample_logits(x[r:r + 1], u[r:r + 1], return_kept=True, **kw)
                assert int(one[0]) == int(a[0][r]) and int(one[1]) == int(a[1][r]), (V, kw, r)


@pytest.mark.parametrize("V", [1, 7, 1003, 4096, 65536])
def test_greedy_is_the_lowest_index_argmax(V):
    ops = _ops()
    x = _logits(5, V, 2.0, 41 + V)
    if V > 7:
        x[0, 3] = x[0, V - 1] = 50.0                                     # ties for the maximum
        x[1, V // 2] = x[1, V // 2 + 1] = 50.0
        x[2, :] = -3.0
    want = _lowest_argmax(x)
    u = _rand(5, 1)
    for kw in (dict(u=None), dict(u=u, top_k=1), dict(u=u, temperature=0), dict(u=None, top_k=9, top_p=0.3)):
        tok, n = ops.sample_logits(x, return_kept=True, **kw)
        assert torch.equal(tok.cpu(), want) and (n == 1).all(), (V, kw)


def test_fenced_buffers_are_respected():
    """logits at 16-byte-and-no-more alignment, V = 1003 in ld = 1008, NaN poison behind every row and around the payload; u, token and
    n_kept inside marked guards: bit-equal to the plain call, guards untouched"""
    from omnibiote_amd import _lib
    B, V, ld = 9, 1003, 1008
    x, u = _logits(B, V, 2.0, 51), _rand(B, 52)
    xf, hx = fenced(x, poison="nan", ld=ld)
    uf, hu = fenced(u, poison="nan")
    assert xf.data_ptr() % 32 == 16 and xf.stride(0) == ld
    for T, k, p in ((1.0, 0, 1.0), (0.8, 50, 1.0), (1.0, 0, 0.9), (0.8, 200, 0.5), (1.0, 1, 1.0)):
        tf, ht = fenced((B,), dtype=torch.int64, poison="mark")
        nf, hn = fenced((B,), dtype=torch.int32, poison="mark")
        _lib.check(_lib.lib().obte_sample_logits_bf16(xf.data_ptr(), ld, B, V, uf.data_ptr(), T, k, p, tf.data_ptr(), nf.data_ptr(),
                                                      torch.cuda.current_stream().cuda_stream), "obte_sample_logits_bf16")
        tok, n = _ops().sample_logits(x, u, T, k or None, p, return_kept=True)
        assert_same_bits(tf, tok, f"token {T} {k} {p}")
        assert_same_bits(nf, n, f"n_kept {T} {k} {p}")
        assert_guards(hx, hu, ht, hn)


# =================================================================================================== through the model
def _case():
    from test_hip_generate import _gen_case
    return _gen_case(256)                                                # block 200, vocabulary 512, 2 layers: built once per session


def _gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


def _kept_sets(m, idx, out, t0, T, k, p):
    """the reference's kept set of every generated token's row, from the logits decode_step itself returns along `out`"""
    from omnibiote_amd.model import KVCache
    steps = out.shape[1] - t0
    cache = KVCache(m, idx.shape[0], t0 + steps)
    logits = m.prefill(idx, cache)
    for i in range(steps):
        n = _ref(logits, 0.5, T, k, p)[1]
        xd = logits.double()
        thr = xd.sort(dim=1, descending=True).values.gather(1, (n - 1).unsqueeze(1))
        yield i, logits, xd >= thr
        if i + 1 < steps:
            logits = m.decode_step(out[:, t0 + i], cache)


def test_generate_on_the_device_sampler_is_seeded_and_stays_in_the_kept_set():
    c = _case()
    m, idx = c["m"], c["ids"][:, :130].to(DEV)
    kw = dict(temperature=0.9, top_k=50, sampler="device")
    a = m.generate(idx, 20, generator=_gen(11), **kw)
    b = m.generate(idx, 20, generator=_gen(11), **kw)
    other = m.generate(idx, 20, generator=_gen(12), **kw)
    assert a.shape == (2, 150) and a.dtype == torch.int64 and torch.equal(a, b) and torch.equal(a[:, :130], idx)
    assert not torch.equal(a, other)
    for i, _, kept in _kept_sets(m, idx, a, 130, 0.9, 50, None):
        assert kept.gather(1, a[:, 130 + i].unsqueeze(1)).all(), i
    ap = m.generate(idx, 20, generator=_gen(11), temperature=0.9, top_k=50, top_p=0.6, sampler="device")
    for i, _, kept in _kept_sets(m, idx, ap, 130, 0.9, 50, 0.6 + DELTA):   # (the kernel's own count lies between the references at p -+ DELTA)
        assert kept.gather(1, ap[:, 130 + i].unsqueeze(1)).all(), i
    with pytest.raises(ValueError, match="sampler"):
        m.generate(idx, 2, sampler="hip")


def test_a_tiny_top_p_is_the_greedy_stream_on_the_device():
    """top_p = 1e-6 keeps the maximal value's ties alone: every token is a maximum of its row's logits, and the stream is top_k = 1's
    for as long as no maximum was tied"""
    c = _case()
    m, idx = c["m"], c["ids"][:, :130].to(DEV)
    tiny = m.generate(idx, 20, top_p=1e-6, sampler="device", generator=_gen(3))
    greedy = m.generate(idx, 20, top_k=1, sampler="device")
    for i, logits, _ in _kept_sets(m, idx, greedy, 130, 1.0, None, None):
        assert torch.equal(greedy[:, 130 + i].cpu(), _lowest_argmax(logits)), i
    tied = False
    for i, logits, _ in _kept_sets(m, idx, tiny, 130, 1.0, None, None):
        top = logits.float().max(dim=1, keepdim=True).values
        assert (logits.float().gather(1, tiny[:, 130 + i].unsqueeze(1)) == top).all(), i
        tied = tied or bool(((logits.float() == top).sum(dim=1) > 1).any())
        if not tied:
            assert torch.equal(tiny[:, 130 + i], greedy[:, 130 + i]), i
    if not tied:
        assert torch.equal(greedy, m.generate(idx, 20, top_k=1))         # and the torch sampler's argmax


def test_ragged_generate_on_the_device_sampler():
    """lengths= and eos_token=: the shapes and out_lengths invariants of the torch path; a parked row does not disturb the other, which
    runs on under its own column of the call's uniforms as it does beside a row that never stops"""
    from test_hip_generate_rows import LENS, _ragged_prompt
    c = _case()
    m, idx = c["m"], _ragged_prompt(c)
    kw = dict(temperature=0.9, top_k=50, lengths=LENS, sampler="device")
    free, nf = m.generate(idx, 20, generator=_gen(11), **kw)
    again, _ = m.generate(idx, 20, generator=_gen(11), **kw)
    assert free.shape == (2, max(LENS) + 20) and free.dtype == torch.int64 and nf.tolist() == [a + 20 for a in LENS] and torch.equal(free, again)
    ref, nr = m.generate(idx, 20, temperature=0.9, top_k=50, lengths=LENS, generator=_gen(11))
    assert ref.shape == free.shape and nr.tolist() == nf.tolist()        # the torch path: the same shapes, another stream
    for b, a in enumerate(LENS):
        assert torch.equal(free[b, :a], idx[b, :a]) and (free[b, a + 20:] == 0).all()
    eos = int(free[0, LENS[0]])                                          # row 0's first token
    out, n = m.generate(idx, 20, generator=_gen(11), eos_token=eos, pad_token=3, **kw)
    assert int(n[0]) == LENS[0] + 1 and int(out[0, LENS[0]]) == eos and (out[0, LENS[0] + 1:] == 3).all()
    assert torch.equal(out[0, :LENS[0]], idx[0, :LENS[0]])
    n1 = int(n[1])
    hit = (free[1, LENS[1]:] == eos).nonzero().flatten()
    assert n1 == (LENS[1] + int(hit[0]) + 1 if hit.numel() else LENS[1] + 20)
    assert torch.equal(out[1, :n1], free[1, :n1]) and (out[1, n1:] == 3).all()
    assert out.shape[1] == n1                                            # returned right after the step at which the last row finished


def test_the_device_sampler_refuses_other_logits():
    from omnibiote_amd import model
    x = torch.zeros(2, 16, device=DEV)                                   # fp32 on the GPU
    with pytest.raises(ValueError, match="sampler"):
        model._next_tokens("generate", x, 1.0, None, None, None, _rand(2, 1))
    with pytest.raises(ValueError, match="sampler"):
        model._next_tokens("generate", x.to(BF).cpu(), 1.0, None, None, None, torch.rand(2))
