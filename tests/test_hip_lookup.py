"""Speculative decoding without a draft model on the GPU (include/omnibiote_hip_lookup.h): obte_lookup_draft against the rule's plain loop
(sampling.lookup_reference) — integers, so exact equality; obte_spec_verify_point_bf16 bit for bit against obte_spec_verify_bf16 on the
one-hot q it stands for; and OmniBioTA.lookup_and_verify / generate_lookup on top of both, under the generation tests' bars
(LOGITS_BAR of tests/test_hip_spec.py: no new tolerance)."""
import pytest
import torch

from fenced import assert_guards, assert_same_bits, fenced

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16
INF = float("inf")
EINVAL, EUNSUPPORTED = -1, -3
W = 8192                                                                  # OBTE_LOOKUP_MAX_HISTORY
NGRAMS = [(1, 4), (3, 3), (2, 16)]


def _ops():
    from omnibiote_amd import ops
    return ops


def _S():
    from omnibiote_amd import sampling
    return sampling


# =================================================================================================== obte_lookup_draft
def _lens(g_max, width=W):
    """1, 2, g_max + 1 and the lengths around the 256-thread stride: one candidate end, the last of a pass, the first of the next"""
    return [1, 2, g_max + 1, 255, 256, 257, 513, width]


_rows = {}


def _hist(kind):
    """the histories of one kind on the CPU, built once: (hist (rows, width) int64, V)
      four     a 4-symbol vocabulary: ties everywhere, matches of every length up to 16, periodic wraps; the last two rows are tandem
               repeats of period 3 and 12 throughout
      wide     V = 65536, random tokens: fallbacks
      odd      the 4-symbol rows in a history of 523 columns
      bad      4 symbols with every seventh token outside [0, V): negative, V itself, and values whose low 32 bits are a valid token"""
    if kind not in _rows:
        g = torch.Generator().manual_seed(len(kind) + 40)
        if kind == "four":
            h = torch.randint(0, 4, (10, W), generator=g)
            h[8] = torch.arange(W) % 3
            h[9] = h[9, :12].repeat(W // 12 + 1)[:W]
            V = 4
        elif kind == "wide":
            h, V = torch.randint(0, 65536, (8, W), generator=g), 65536
        elif kind == "odd":
            h, V = torch.randint(0, 4, (8, 523), generator=g), 4
        else:
            h, V = torch.randint(0, 4, (8, W), generator=g), 4
            junk = torch.tensor([-1, 4, 2 ** 32 + 1, -2 ** 63, 2 ** 62, 65536, 2 ** 40 + 3, -4])
            h[:, ::7] = junk[torch.randint(0, 8, h[:, ::7].shape, generator=g)]
        _rows[kind] = (h, V)
    return _rows[kind]


_refs = {}


def _reference(kind, ngram):
    """(lens, draft for k = 31, match_len) of every row of a kind under an n-gram range, computed once: the draft for a smaller k is its prefix"""
    if (kind, ngram) not in _refs:
        h, V = _hist(kind)
        lens = _lens(ngram[1], h.shape[1])
        lens = (lens + [257, 8000])[:h.shape[0]]
        d, m = _S().lookup_reference(h, lens, 31, ngram[0], ngram[1], V)
        _refs[(kind, ngram)] = (torch.tensor(lens, dtype=torch.int32), d, m)
    return _refs[(kind, ngram)]


@pytest.mark.parametrize("ngram", NGRAMS)
@pytest.mark.parametrize("k", [1, 8, 31])
@pytest.mark.parametrize("B", [1, 5])
def test_lookup_draft_is_the_reference(B, k, ngram):
    ops = _ops()
    matched = 0
    for kind in ("four", "wide", "odd", "bad"):
        h, V = _hist(kind)
        lens, want_d, want_m = _reference(kind, ngram)
        hd, ld = h.to(DEV), lens.to(DEV)
        for r in range(0, h.shape[0], B):                                # batches of B consecutive rows; the last one overlaps the one before
            r = min(r, h.shape[0] - B)
            d, m = ops.lookup_draft(hd[r:r + B], ld[r:r + B], k, ngram, V)
            assert d.dtype == torch.int64 and d.shape == (B, k) and m.dtype == torch.int32 and m.shape == (B,)
            assert torch.equal(m.cpu(), want_m[r:r + B]), (kind, r, m.tolist(), want_m[r:r + B].tolist())
            assert torch.equal(d.cpu(), want_d[r:r + B, :k]), (kind, r)
        matched += int((want_m > 0).sum())
    assert matched > 0


def test_the_cases_cover_what_they_are_meant_to():
    """on the CPU alone: the 4-symbol rows hold full-length matches, ties and periodic wraps, the wide rows mostly fallbacks"""
    lens, d, m = _reference("four", (2, 16))
    assert m[8] == 16 and m[9] == 16 and (m[3:8] >= 2).all() and m[0] == 0
    assert d[8].tolist() == [(int(lens[8]) + j) % 3 for j in range(31)]   # the period-3 row goes on past its end
    h, _ = _hist("four")
    n = int(lens[9])
    assert d[9].tolist() == [int(h[9, (n + j) % 12]) for j in range(31)]
    lens, d, m = _reference("four", (1, 4))
    assert (m[6:] == 4).all()                                            # several ends share the longest match: the largest one decides
    lens, d, m = _reference("wide", (1, 4))
    assert (m == 0).sum() >= 4 and (m <= 2).all()
    lens, d, m = _reference("wide", (3, 3))
    assert (m == 0).all()
    lens, d, m = _reference("bad", (1, 4))
    h, V = _hist("bad")
    assert ((d < 0) | (d >= V)).any()                                    # a token outside the vocabulary is drafted as it stands


def test_inactive_rows_get_zeros():
    ops = _ops()
    h, V = _hist("four")
    lens = torch.tensor([0, -1, W + 1, 2 ** 31 - 1, -2 ** 31, 300], dtype=torch.int32)
    want_d, want_m = _S().lookup_reference(h[:6], lens, 8, 1, 4, V)
    assert (want_d[:5] == 0).all() and (want_m[:5] == 0).all() and want_m[5] > 0
    d, m = ops.lookup_draft(h[:6].to(DEV), lens.to(DEV), 8, (1, 4), V)
    assert torch.equal(d.cpu(), want_d) and torch.equal(m.cpu(), want_m)
    narrow = h[:6, :200].contiguous()                                    # 300 > hist_ld = 200: inactive here
    d, m = ops.lookup_draft(narrow.to(DEV), lens.to(DEV), 8, (1, 4), V)
    assert (d == 0).all() and (m == 0).all()


def test_repeatable_and_a_row_depends_on_itself_alone():
    ops = _ops()
    for kind in ("four", "bad"):
        h, V = _hist(kind)
        lens, _, _ = _reference(kind, (1, 4))
        hd, ld = h.to(DEV), lens.to(DEV)
        a = ops.lookup_draft(hd, ld, 31, (1, 4), V)
        b = ops.lookup_draft(hd, ld, 31, (1, 4), V)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
        for r in range(h.shape[0]):
            one = ops.lookup_draft(hd[r:r + 1], ld[r:r + 1], 31, (1, 4), V)
            assert torch.equal(one[0][0], a[0][r]) and int(one[1]) == int(a[1][r]), (kind, r)


def test_lookup_draft_inside_guard_bands():
    """hist and lens inside marked guards (a read past a row cannot be seen, a write can), both outputs inside marked guards: the plain
    call's bits, guards untouched"""
    from omnibiote_amd import _lib
    h, V = _hist("odd")
    lens, want_d, want_m = _reference("odd", (1, 4))
    B, width, k = h.shape[0], h.shape[1], 31
    hf, hh = fenced(h.to(DEV), poison="mark")
    lf, hl = fenced(lens.to(DEV), poison="mark")
    df, hd = fenced((B, k), dtype=torch.int64, poison="mark")
    mf, hm = fenced((B,), dtype=torch.int32, poison="mark")
    _lib.check(_lib.lib().obte_lookup_draft(hf.data_ptr(), width, lf.data_ptr(), B, k, 1, 4, V, df.data_ptr(), mf.data_ptr(),
                                            torch.cuda.current_stream().cuda_stream), "obte_lookup_draft")
    d, m = _ops().lookup_draft(h.to(DEV), lens.to(DEV), k, (1, 4), V)
    assert_same_bits(df, d, "draft")
    assert_same_bits(mf, m, "match_len")
    assert torch.equal(df.cpu(), want_d) and torch.equal(mf.cpu(), want_m)
    assert_guards(hh, hl, hd, hm)


def test_lookup_draft_refuses_on_the_device_too():
    from omnibiote_amd import _lib
    lib = _lib.lib()
    h = torch.zeros(2, W + 1, dtype=torch.int64, device=DEV)
    lens = torch.ones(2, dtype=torch.int32, device=DEV)
    d = torch.full((2, 32), 77, dtype=torch.int64, device=DEV)
    m = torch.full((2,), 77, dtype=torch.int32, device=DEV)
    st = torch.cuda.current_stream().cuda_stream

    def call(hist=h.data_ptr(), hist_ld=W, ln=lens.data_ptr(), k=4, draft=d.data_ptr(), match=m.data_ptr()):
        return lib.obte_lookup_draft(hist, hist_ld, ln, 2, k, 1, 4, 512, draft, match, st)

    assert call(hist_ld=W + 1) == EUNSUPPORTED and "8193" in lib.obte_last_error().decode()
    assert call(k=32) == EUNSUPPORTED and "k = 32" in lib.obte_last_error().decode()
    for kw in (dict(hist=None), dict(ln=None), dict(draft=None), dict(match=None)):
        assert call(**kw) == EINVAL and "null" in lib.obte_last_error().decode()
    torch.cuda.synchronize()
    assert (d == 77).all() and (m == 77).all()                           # nothing was launched
    with pytest.raises(ValueError, match="8193"):
        _ops().lookup_draft(h, lens, 4)
    with pytest.raises(ValueError, match="k must"):
        _ops().lookup_draft(h[:, :64].contiguous(), lens, 32)
    with pytest.raises(ValueError, match="apart"):
        _ops().lookup_draft(h[:, :64], lens, 4)


# =================================================================================================== obte_spec_verify_point_bf16
SAMPLED = dict(temperature=0.8, top_k=50, top_p=0.9)


def _in_ld(x, fill=100.0):
    """x (B, r, V) copied into rows of ld = V rounded up to 8, the columns behind V holding `fill`: a (B, r, V) view"""
    B, r, V = x.shape
    buf = torch.full((B * r, (V + 7) // 8 * 8), fill, dtype=BF, device=DEV)
    buf[:, :V] = x.reshape(B * r, V).to(DEV)
    return buf[:, :V].unflatten(0, (B, r))


def _one_hot(x, V):
    """the q the point form stands for: row (b, j) is 0 at x[b, j] and -inf elsewhere, all -inf for a token outside [0, V)"""
    inside = (x >= 0) & (x < V)
    q = torch.full(tuple(x.shape) + (V,), -INF, dtype=BF, device=x.device)
    q.scatter_(2, x.clamp(0, V - 1).unsqueeze(2), torch.where(inside, 0.0, -INF).to(BF).unsqueeze(2))
    return _in_ld(q, -INF)


def _point_case(B, k, V, seed):
    """p (B, k + 1, V) in rows of ld, drafts that mix the target's argmax, random tokens, tokens the target does not keep (each row's
    minimum) and tokens out of range, and uniforms of which a quarter are 0 (whatever the target keeps stands)"""
    g = torch.Generator().manual_seed(seed)
    p = (torch.randn(B, k + 1, V, generator=g) * 2.0).to(BF)
    pf = p[:, :k].float()
    kinds = torch.randint(0, 8, (B, k), generator=g)
    x = torch.randint(0, V, (B, k), generator=g)
    x = torch.where(kinds < 4, pf.argmax(dim=2), x)                      # half: the favourite
    x = torch.where(kinds == 6, pf.argmin(dim=2), x)
    junk = torch.tensor([-1, V, V + 7, 2 ** 62, -2 ** 63, 2 ** 32])
    x = torch.where(kinds == 7, junk[torch.randint(0, 6, (B, k), generator=g)], x)
    ua, ud = torch.rand(B, k, generator=g), torch.rand(B, generator=g)
    ua = torch.where(torch.rand(B, k, generator=g) < 0.25, torch.zeros(()), ua)
    if k > 1:                                                            # row 0 gets past position 0 and not past the last
        x[0, 0], x[0, k - 1] = int(pf[0, 0].argmax()), int(pf[0, k - 1].argmin())
        ua[0, 0], ua[0, k - 1] = 0.0, 0.5
    return _in_ld(p), x.to(DEV), ua.to(DEV), ud.to(DEV)


@pytest.mark.parametrize("k", [1, 4, 31])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("V", [512, 1001, 65536])
def test_spec_verify_point_is_spec_verify_on_the_one_hot_q(V, B, k):
    ops = _ops()
    p, x, ua, ud = _point_case(B, k, V, 1000 * k + 10 * B + V % 97)
    assert p.stride(1) == (V + 7) // 8 * 8
    q = _one_hot(x, V)
    seen = []
    for kw in (dict(), dict(top_k=1), SAMPLED, dict(temperature=0.8), dict(top_k=50), dict(top_p=0.9)):
        uniforms = (None, None) if not kw else (ua, ud)                  # greedy without uniforms, and greedy by top_k = 1
        n, tok = ops.spec_verify_point(p, x, *uniforms, **kw)
        want_n, want_tok = ops.spec_verify(p, q, x, *uniforms, **kw)
        assert_same_bits(n, want_n, f"n_accept {kw}")
        assert_same_bits(tok, want_tok, f"token {kw}")
        n2, tok2 = ops.spec_verify_point(p, x, *uniforms, **kw)          # repeatable
        assert torch.equal(n, n2) and torch.equal(tok, tok2), kw
        assert ((tok >= 0) & (tok < V)).all()
        seen += n.tolist()
    if k > 1:
        assert max(seen) >= 1 and min(seen) < k, seen                    # the cases are neither all rejections nor all acceptances


def test_spec_verify_point_against_the_float64_rule():
    """the contract's other side, away from the rounding of the fixed-point weights: under u_accept = 0 what the target keeps stands and
    nothing else does, exactly as sampling.verify_point_reference has it; the token behind a rejection is never the rejected one"""
    ops = _ops()
    B, k, V = 6, 4, 1001
    p, x, ua, ud = _point_case(B, k, V, 5)
    zero = torch.zeros_like(ua)
    for kw in (dict(), dict(top_k=50), dict(top_k=1)):
        n, tok = ops.spec_verify_point(p, x, zero, ud, **kw)
        want = _S().verify_point_reference(p.cpu(), x.cpu(), zero.cpu(), ud.cpu(), **kw)
        assert torch.equal(n.cpu().long(), want[0]), kw
        if kw.get("top_k") == 1:
            assert torch.equal(tok.cpu(), want[1])
        rej = n.long() < k
        xa = x.gather(1, n.long().clamp(max=k - 1).unsqueeze(1)).squeeze(1)
        assert (tok[rej] != xa[rej]).all(), kw


def test_spec_verify_point_inside_guard_bands():
    """p at 16-byte-and-no-more alignment, V = 1001 in ld = 1008 with NaN behind every row and around the payload; the drafts, the
    uniforms, both outputs and the workspace inside marked guards: bit-equal to the plain call, guards untouched, and the workspace
    written inside obte_spec_verify_point_ws_bytes alone"""
    from omnibiote_amd import _lib
    B, k, V, ld = 9, 4, 1001, 1008
    p, x, ua, ud = _point_case(B, k, V, 51)
    pf, hp = fenced(p.flatten(0, 1), poison="nan", ld=ld)
    xf, hx = fenced(x, poison="mark")
    af, ha = fenced(ua, poison="nan")
    df, hd = fenced(ud, poison="nan")
    assert pf.data_ptr() % 32 == 16 and pf.stride(0) == ld
    need = _lib.lib().obte_spec_verify_point_ws_bytes(B, k)
    assert need == B * (k + 1) * 32
    for T, tk, tp in ((1.0, 0, 1.0), (0.8, 50, 0.9), (1.0, 0, 0.9), (1.0, 1, 1.0)):
        nf, hn = fenced((B,), dtype=torch.int32, poison="mark")
        tf, ht = fenced((B,), dtype=torch.int64, poison="mark")
        wf, hw = fenced((need,), dtype=torch.uint8, poison="mark")
        _lib.check(_lib.lib().obte_spec_verify_point_bf16(pf.data_ptr(), ld, xf.data_ptr(), B, k, V, af.data_ptr(), df.data_ptr(), T, tk, tp, nf.data_ptr(),
                                                          tf.data_ptr(), wf.data_ptr(), need, torch.cuda.current_stream().cuda_stream),
                   "obte_spec_verify_point_bf16")
        n, tok = _ops().spec_verify_point(p, x, ua, ud, T, tk or None, tp)
        assert_same_bits(nf, n, f"n_accept {T} {tk} {tp}")
        assert_same_bits(tf, tok, f"token {T} {tk} {tp}")
        assert_guards(hp, hx, ha, hd, hn, ht, hw)


# =================================================================================================== the distribution
DIST_SEED = 2


def _dist_case(device):
    """V = 16, k = 2, N = 16 384 batch rows sharing one p; an arbitrary point draft — uniform tokens, whatever the target thinks of them —
    and every uniform from one seeded CPU generator"""
    V, k, N = 16, 2, 16384
    g = torch.Generator().manual_seed(DIST_SEED)
    p = (torch.randn(1, k + 1, V, generator=g) * 1.5).to(BF)
    x = torch.randint(0, V, (N, k), generator=g)
    ua, ud = torch.rand(N, k, generator=g), torch.rand(N, generator=g)
    return tuple(t.to(device) for t in (p.expand(N, k + 1, V).contiguous(), x, ua, ud))


def _first_token_frequencies_are_the_targets(x0, a, tok, p):
    N, V = x0.shape[0], p.shape[2]
    first = torch.where(a >= 1, x0, tok)
    f = torch.bincount(first, minlength=V).double() / N
    P0 = torch.softmax(p[0, 0].double(), dim=0)
    bound = 5 * torch.sqrt(P0 * (1 - P0) / N) + 1.0 / N
    return (f - P0).abs(), bound


def test_the_first_emitted_token_has_the_targets_distribution():
    """x_0 if it stands, else the verified token, is distributed as P_0 whatever the drafted token: |f_i - P_0(i)| <= 5 sqrt(P_0(i) (1 -
    P_0(i)) / N) + 1 / N in every bin.  DIST_SEED is one for which verify_point_reference itself, run on the CPU on the same uniforms,
    is inside the bound (at 0.39 of it in its worst bin)."""
    p, x, ua, ud = _dist_case("cpu")
    a, tok, _ = _S().verify_point_reference(p, x, ua, ud)
    d, bound = _first_token_frequencies_are_the_targets(x[:, 0], a, tok, p)
    assert (d <= bound).all(), "the reference itself misses the bound under this seed"
    p, x, ua, ud = _dist_case(DEV)
    n, tok = _ops().spec_verify_point(p, x, ua, ud)
    d, bound = _first_token_frequencies_are_the_targets(x[:, 0], n.long(), tok, p)
    print(f"first emitted token over 16384 rows, point drafts: largest |f - P_0| {float(d.max()):.3g}, the tightest bound {float(bound.min()):.3g}; "
          f"accepted {float(n.float().mean()):.3f} of 2 on average")
    assert (d <= bound).all(), (d / bound).max()


# =================================================================================================== the loop
LOGITS_BAR = 5e-3                                                         # the generation tests' bar on logits (tests/test_hip_spec.py)
PLANT_C, PLANT_T0, PLANT_AT, PLANT_K = 128, 110, 114, 4                   # the planted round: the model's width, the prompt, the pending token's index, k


def _case(C=256):
    from test_hip_generate import _gen_case
    return _gen_case(C)                                                  # block 200, vocabulary 512, 2 layers: built once per session


def _gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


def _teacher_forced(m, out, t0, steps):
    """the target's logits behind positions t0 - 1 .. t0 + steps - 2 from ONE full causal forward over `out`: entry i predicts token t0 + i"""
    with torch.no_grad():
        return m(out[:, :t0 + steps]).float()[:, t0 - 1:t0 + steps - 1]


def _kept(logits, T, k, bar):
    """the reference's kept set of every row, the threshold loosened by `bar`: what a path whose logits lie within bar / 2 of these may keep
    (the rule of tests/test_hip_spec.py's helper of the same name)"""
    n = _S().sample_reference(logits, 0.5, T, k, None)[1]
    xd = logits.double()
    thr = xd.sort(dim=1, descending=True).values.gather(1, (n - 1).unsqueeze(1))
    return xd >= thr - bar


def _by_hand(m, idx, new, k, ngram=(1, 4)):
    """generate_lookup's greedy loop replayed through lookup_and_verify with the caller's own history and per-row account — a row is parked
    once it has its `new` tokens, as the loop parks it: (tokens (B, new), stats)"""
    from omnibiote_amd.model import KVCache
    B, t0 = idx.shape
    cache = KVCache(m, B, t0 + new + k)
    pending = _ops().sample_logits(m.prefill(idx, cache, lengths=[t0] * B), None)
    hist = torch.zeros((B, t0 + new + k + 1), dtype=torch.int64, device=DEV)
    hist[:, :t0] = idx
    hist[:, t0] = pending
    n = [t0 + 1] * B                                                     # every row's tokens so far; n - 1 of them are in the cache
    parked = [False] * B
    stats = dict(rounds=0, drafted=0, accepted=0, matched=0)
    while min(n) < t0 + new:
        done = [v >= t0 + new for v in n]
        if done != parked:
            cache.park(torch.tensor([d and not q for d, q in zip(done, parked)], device=DEV))
            parked = done
        x, a, tok, match = m.lookup_and_verify(pending, cache, hist, torch.tensor(n, dtype=torch.int32, device=DEV), k, ngram=ngram)
        now = [-1 if d else v - 1 + k + 1 for v, d in zip(n, done)]
        assert cache.positions.tolist() == now
        a, match = a.tolist(), match.tolist()
        counted = [0 if d else min(v + 1, t0 + new - c) for v, c, d in zip(a, n, done)]
        cache.rewind_rows([0 if d else k + 1 - c for c, d in zip(counted, done)], now=now)
        stats["rounds"] += 1
        for b in range(B):
            if done[b]:
                continue
            stats["drafted"] += k
            stats["accepted"] += a[b]
            stats["matched"] += match[b] > 0
            row = x[b, :a[b]].tolist() + [int(tok[b])]                   # what the round emitted; the first counted[b] of it count
            hist[b, n[b]:n[b] + counted[b]] = torch.tensor(row[:counted[b]], device=DEV)
            n[b] += counted[b]
        assert cache.positions.tolist() == [-1 if d else v - 1 for v, d in zip(n, done)]
        pending = tok
    assert n == [t0 + new] * B                                           # per row: 1 + the sum over its rounds of what counted
    return hist[:, t0:t0 + new], stats


def test_greedy_lookup_follows_the_full_forward_and_its_account_adds_up():
    c = _case(256)
    m, idx = c["m"], c["ids"][:, :100].to(DEV)
    out, stats = m.generate_lookup(idx, 24, k=4, top_k=1, return_stats=True)
    assert out.shape == (2, 124) and out.dtype == torch.int64 and torch.equal(out[:, :100], idx)
    at = _teacher_forced(m, out, 100, 24)
    gap = at.max(dim=-1).values - at.gather(-1, out[:, 100:].unsqueeze(-1)).squeeze(-1)
    print(f"greedy lookup: largest logit gap to the full forward's maximum {gap.max().item():.4g}; {stats}")
    assert (gap <= 2 * LOGITS_BAR).all(), gap.max().item()
    rr = stats["drafted"] // 4                                           # running row-rounds
    assert stats["drafted"] == 4 * rr and stats["rounds"] <= rr <= 2 * stats["rounds"] and 0 <= stats["accepted"] <= stats["drafted"]
    assert 0 <= stats["matched"] <= rr
    # per row: tokens emitted = 1 + the sum over its rounds of what counted, min(a + 1, what was left); so over both rows
    assert rr <= 2 * 23 <= stats["accepted"] + rr, stats
    tokens, mine = _by_hand(m, idx, 24, 4)                               # the same rounds, the account kept here: the identities hold exactly
    assert torch.equal(tokens, out[:, 100:]) and mine == stats, (mine, stats)
    again = m.generate_lookup(idx, 24, k=4, top_k=1)
    assert torch.equal(again, out)
    assert torch.equal(m.generate_lookup(idx, 24, k=4, temperature=0, generator=_gen(3)), out)
    wide = m.generate_lookup(idx, 7, k=31, ngram=(2, 16), top_k=1)       # 7 = 1 + at most 32 a round: trimmed inside the first round
    assert wide.shape == (2, 107)
    gap = _teacher_forced(m, wide, 100, 7)
    gap = gap.max(dim=-1).values - gap.gather(-1, wide[:, 100:].unsqueeze(-1)).squeeze(-1)
    assert (gap <= 2 * LOGITS_BAR).all(), gap.max().item()


def test_one_round_with_a_planted_history_accepts_the_true_continuation():
    """The greedy stream `out` of generate() behind a prompt of PLANT_T0 tokens; out[:, :PLANT_AT] prefilled, out[:, PLANT_AT] pending.  The
    history holds out[:, PLANT_AT - 3 : PLANT_AT + 1 + k] in front of the real tokens: the row's last four tokens occur there, followed by
    the true continuation, and nowhere later (asserted with lookup_reference).  The round must accept all k — up to the first position
    at which the fp32 oracle's top two logits lie within 4 LOGITS_BAR of each other, where two paths within the bar of the oracle may
    disagree about the argmax; at most one such position may occur over the case.  The hash-weight models' logits lie close together
    (the oracle's margin over this stream is below 4 LOGITS_BAR at every second position); the width-128 model, this prompt length and
    this offset are the choice at which the oracle, run on the CPU over the stream, has no such position: its smallest margin behind
    positions 114 .. 117 is 0.0234.  The margins are printed."""
    import omnibiote_ref as R
    from test_hip_generate import _add, _tril
    from omnibiote_amd.model import KVCache
    c = _case(PLANT_C)
    m, cfg, k, at = c["m"], c["cfg"], PLANT_K, PLANT_AT
    out = m.generate(c["ids"][:, :PLANT_T0].to(DEV), 60, top_k=1)[:, :at + k + 1]
    history = torch.cat([out[:, at - 3:at + 1 + k], out[:, :at + 1]], dim=1).contiguous()
    n = history.shape[1]
    want_x, want_m = _S().lookup_reference(history.cpu(), [n, n], k, 1, 4, cfg.vocab_size)
    assert torch.equal(want_x, out[:, at + 1:at + 1 + k].cpu()) and want_m.tolist() == [4, 4], "the planted match is not the one found"
    # the oracle over the stream: the margin between its top two logits behind positions at .. at + k - 1
    w = {name: v.to(BF).float() for name, v in R.hash_weights(cfg).items()}
    T = at + k
    with torch.no_grad():
        ref = R.model_forward(w, cfg, out[:, :T].cpu(), _add(_tril(T)), rope=R.cast_rope_table(R.rope_table(cfg.n_embd // cfg.n_head, T), BF))[:, at:]
    top = ref.topk(2, dim=-1).values
    close = (top[..., 0] - top[..., 1]) < 4 * LOGITS_BAR                 # (2, k)
    print(f"planted round: the oracle's top-two margins behind positions {at} .. {at + k - 1}: {(top[..., 0] - top[..., 1]).tolist()}")
    assert int(close.sum()) <= 1, "more than one near-tie over the case: choose another PLANT_AT"
    cache = KVCache(m, 2)
    m.prefill(out[:, :at].contiguous(), cache, lengths=[at, at])
    lengths = torch.full((2,), n, dtype=torch.int32, device=DEV)
    x, a, tok, match = m.lookup_and_verify(out[:, at].contiguous(), cache, history, lengths, k)
    assert torch.equal(x.cpu(), want_x) and match.tolist() == [4, 4]
    assert x.dtype == tok.dtype == torch.int64 and a.dtype == match.dtype == torch.int32 and tok.shape == a.shape == (2,)
    assert cache.positions.tolist() == [at + k + 1] * 2
    for b in range(2):
        sure = int(close[b].to(torch.uint8).argmax()) if close[b].any() else k
        assert int(a[b]) >= sure, (b, a.tolist(), close.tolist())
        assert int(a[b]) == k or close[b, int(a[b])], (b, a.tolist(), close.tolist())
    acc = a.tolist()
    cache.rewind_rows([k - v for v in acc], now=[at + k + 1] * 2)
    assert cache.positions.tolist() == [at + v + 1 for v in acc]         # the pending token and what stood; `tok` is pending, in no cache
    assert cache.pos == max(cache.positions.tolist()) and cache.min_pos == min(cache.positions.tolist())


def test_sampled_lookup_is_seeded_and_stays_in_the_targets_kept_set():
    c = _case(256)
    m, idx = c["m"], c["ids"][:, :100].to(DEV)
    kw = dict(k=4, temperature=0.9, top_k=50, return_stats=True)
    a, sa = m.generate_lookup(idx, 24, generator=_gen(11), **kw)
    b, sb = m.generate_lookup(idx, 24, generator=_gen(11), **kw)
    other, _ = m.generate_lookup(idx, 24, generator=_gen(12), **kw)
    assert a.shape == (2, 124) and a.dtype == torch.int64 and torch.equal(a, b) and sa == sb and torch.equal(a[:, :100], idx)
    assert not torch.equal(a, other)
    at = _teacher_forced(m, a, 100, 24)
    for i in range(24):
        assert _kept(at[:, i], 0.9, 50, 2 * LOGITS_BAR).gather(1, a[:, 100 + i].unsqueeze(1)).all(), i
    print(f"sampled lookup run: {sa}")
    rr = sa["drafted"] // 4
    assert sa["drafted"] == 4 * rr and sa["rounds"] <= rr <= 2 * sa["rounds"] and 0 <= sa["accepted"] <= sa["drafted"] and sa["matched"] <= rr
    assert rr <= 2 * 23 <= sa["accepted"] + rr, sa
    assert sa["rounds"] >= 5                                             # at most k + 1 = 5 tokens per round behind the first


def test_ragged_prompts_eos_and_the_trim():
    from test_hip_generate_rows import LENS, _ragged_prompt
    c = _case(256)
    m, idx = c["m"], _ragged_prompt(c)
    kw = dict(k=4, temperature=0.9, top_k=50, lengths=LENS)
    free, nf = m.generate_lookup(idx, 24, generator=_gen(11), **kw)
    again, _ = m.generate_lookup(idx, 24, generator=_gen(11), **kw)
    assert free.shape == (2, max(LENS) + 24) and free.dtype == torch.int64 and nf.tolist() == [a + 24 for a in LENS] and torch.equal(free, again)
    for b, a in enumerate(LENS):
        assert torch.equal(free[b, :a], idx[b, :a]) and (free[b, a + 24:] == 0).all()
        at = _teacher_forced(m, free[b:b + 1], a, 24)
        for i in range(24):
            assert _kept(at[:, i], 0.9, 50, 2 * LOGITS_BAR)[0, int(free[b, a + i])], (b, i)
    # EOS: row 0's fourth token — with k = 4 it falls inside a round, or is that round's last
    eos = int(free[0, LENS[0] + 3])
    first = [int((free[b, a:a + 24] == eos).nonzero().flatten()[0]) + 1 if (free[b, a:a + 24] == eos).any() else 24 for b, a in enumerate(LENS)]
    out, n, stats = m.generate_lookup(idx, 24, generator=_gen(11), eos_token=eos, pad_token=3, return_stats=True, **kw)
    assert n.tolist() == [a + f for a, f in zip(LENS, first)] and first[0] <= 4      # the same stream up to each row's EOS
    assert out.shape == (2, max(LENS) + max(first))
    for b, a in enumerate(LENS):
        assert torch.equal(out[b, :a + first[b]], free[b, :a + first[b]]) and (out[b, a + first[b]:] == 3).all()
    # equal lengths: a finished row is filled with the EOS, the other runs to max_new_tokens; 7 = 1 + 5 + 1 is trimmed inside a round
    idx2 = c["ids"][:, :100].to(DEV)
    for new in (7, 24):
        plain = m.generate_lookup(idx2, new, k=4, temperature=0.9, top_k=50, generator=_gen(5))
        assert plain.shape == (2, 100 + new)
        if new == 24:
            assert torch.equal(plain[:, :107], short)                    # the trim cuts the stream, it does not change it
        short = plain
    eos = int(plain[1, 102])
    got = m.generate_lookup(idx2, 24, k=4, temperature=0.9, top_k=50, generator=_gen(5), eos_token=eos)
    assert got.shape == (2, 124)
    for b in range(2):
        hit = (plain[b, 100:] == eos).nonzero().flatten()
        end = 100 + int(hit[0]) + 1 if hit.numel() else 124
        assert torch.equal(got[b, :end], plain[b, :end]) and (got[b, end:] == eos).all()
