"""obte_sample_logits_constrained_bf16 and obte_spec_verify_constrained_bf16 (include/omnibiote_hip_constrain.h) on the device.

The main test has no tolerance: an excluded column is treated exactly as an entry holding -inf, so the constrained call's integers are,
bit for bit, those of the unrestricted call on a copy of the logits whose excluded columns were overwritten with -inf
(sampling.constrain_reference makes the copy).  Against the float64 rule the criterion and the bound are those of tests/test_hip_sample.py
and tests/test_hip_spec.py, used as they stand: their ``_check`` runs with the constrained call on the untouched logits in the kernel's
place and the reference on the -inf copy.  The verification's inputs keep the residual mass Z >= 0.05 at every drafted position of every
row under the restriction, which the test asserts for the seeds it uses on the reference alone, before the kernel runs."""
import pytest
import torch

import test_hip_sample as THS
import test_hip_spec as THV
from fenced import assert_guards, assert_same_bits, fenced

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16
INF = float("inf")
VS = [5, 250, 2048, 2056, 16384, 16392, 65536]
MODES = [dict(T=0.0), dict(T=0.8), dict(k=50), dict(p=0.9), dict(T=0.8, k=200, p=0.9)]      # greedy, plain, top_k, top_p, both
I32 = torch.int32


def _ops():
    from omnibiote_amd import ops
    return ops


def _S():
    from omnibiote_amd import sampling
    return sampling


def _gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


def _half(shape, seed):
    return torch.rand(shape, device=DEV, generator=_gen(seed)) < 0.5


def _sample(x, u, mode, **con):
    return _ops().sample_logits(x, u, mode.get("T", 1.0), mode.get("k"), mode.get("p"), return_kept=True, **con)


def _minus_inf_copy(x, allowed=None, hold=None, emitted=None, min_emitted=0, offset=0):
    """the logits with the excluded columns overwritten with -inf, in rows of ld = V rounded up to 8 like the original's"""
    y = _S().constrain_reference(x, allowed, hold, emitted, min_emitted, offset)
    return THS._in_ld(y) if y.dim() == 2 else THV._in_ld(y)


def _same(got, want, what):
    for g, w, name in zip(got, want, ("token", "count")):
        assert g.dtype == w.dtype and torch.equal(g, w), (what, name, g.tolist()[:4], w.tolist()[:4])


# =================================================================================================== 1. exact equivalence: the sampler
def _mask_cases(x):
    """(name, the call's keywords, the bool (B, V) or (V,) mask they mean)"""
    B, V = x.shape
    pack = _ops().pack_token_mask
    nb = (V + 7) // 8
    top = x.float().argmax(dim=1)
    cases = []
    everything = torch.ones(V, dtype=torch.bool, device=DEV)
    cases.append(("everything", dict(allowed=everything), everything))
    one = torch.zeros(V, dtype=torch.bool, device=DEV)
    one[V // 2] = True
    cases.append(("one token", dict(allowed=one), one))
    no_max = torch.ones(B, V, dtype=torch.bool, device=DEV)
    no_max[torch.arange(B), top] = False
    cases.append(("row maximum excluded", dict(allowed=no_max), no_max))
    half = _half((V,), V)
    half[V // 3] = True
    cases.append(("random half, shared", dict(allowed_packed=pack(half)), half))
    rows = _half((B, V), V + 1)
    rows[:, 0] = True
    cases.append(("per-row masks", dict(allowed=rows), rows))
    wide = torch.full((B, nb + 5), 0xA5, dtype=torch.uint8, device=DEV)          # allowed_ld = nb + 5, odd; junk between the rows
    wide[:, :nb] = pack(rows)
    cases.append(("allowed_ld larger than needed", dict(allowed_packed=wide), rows))
    odd = torch.full((nb + 3,), 0xFF, dtype=torch.uint8, device=DEV)
    odd[1:1 + nb] = pack(half)
    assert odd[1:1 + nb].data_ptr() % 2 == 1
    cases.append(("odd byte address", dict(allowed_packed=odd[1:1 + nb]), half))
    if V % 8:
        dirty = pack(rows)
        dirty[:, -1] |= 0xFF & ~((1 << (V % 8)) - 1)
        cases.append(("bits set beyond V", dict(allowed_packed=dirty), rows))
    edge = torch.ones(V, dtype=torch.bool, device=DEV)
    edge[[c for c in (7, 8) if c < V] or [V - 1]] = False
    cases.append(("columns 7 and 8", dict(allowed=edge), edge))
    last = torch.ones(V, dtype=torch.bool, device=DEV)
    last[V - 1] = False
    cases.append(("the last column, in the last partial byte", dict(allowed=last), last))
    return cases


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("V", VS)
def test_sampler_equals_the_unrestricted_call_on_a_minus_inf_copy(V, B):
    x = THS._logits(B, V, 2.0, 31 * V + B)
    x[0, V - 1] = 30.0                                                           # row 0's maximum is the last column
    x[:, 7 % V] = 9.0                                                            # and column 7 stands out in every row
    for i, mode in enumerate(MODES):
        u = THS._rand(B, V + 17 * i)
        plain = _sample(x, u, mode)
        for name, kw, mask in _mask_cases(x):
            want = _sample(_minus_inf_copy(x, mask), u, mode)
            _same(_sample(x, u, mode, **kw), want, (V, B, mode, name))
            if name == "everything":
                _same(want, plain, (V, B, mode, "everything allowed is the plain call"))
                _same(_sample(x, u, mode, hold_token=None, min_emitted=0, emitted=torch.zeros(B, dtype=I32, device=DEV)), plain, (V, B, mode, "no mask"))
            if name == "row maximum excluded" and V > 1:
                assert (_sample(x, u, mode, **kw)[0] != x.float().argmax(dim=1)).all()
    # the only finite entries excluded: token 0, nothing kept
    y = THS._in_ld(torch.full((B, V), -INF, dtype=BF, device=DEV))
    cols = sorted({V // 2, V - 1})
    y[:, cols] = 1.5
    gone = torch.ones(V, dtype=torch.bool, device=DEV)
    gone[cols] = False
    for mode in MODES:
        tok, n = _sample(y, THS._rand(B, 5), mode, allowed=gone)
        assert tok.tolist() == [0] * B and n.tolist() == [0] * B, (V, mode)
        tok, n = _sample(y, THS._rand(B, 5), mode, allowed=~gone)
        assert all(t in cols for t in tok.tolist()) and n.tolist() == [1 if mode.get("T") == 0.0 else len(cols)] * B, (V, mode)


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("V", VS)
def test_held_token_equals_the_unrestricted_call_on_a_minus_inf_copy(V, B):
    x = THS._logits(B, V, 2.0, 77 * V + B)
    hold = (V - 1) if V % 8 else V // 2 + 3
    x[:, hold] = 25.0                                                            # the held token is every row's maximum
    half = _half((B, V), V + 9)
    half[:, [0, hold]] = True
    MIN = 5
    below_at_above = torch.tensor([MIN - 1, MIN, MIN + 1][:B], dtype=I32, device=DEV)
    wild = torch.tensor([-2 ** 31, 2 ** 31 - 1, -1][:B], dtype=I32, device=DEV)
    for i, mode in enumerate(MODES):
        u = THS._rand(B, V + 29 * i)
        plain = _sample(x, u, mode)
        for emitted, mn in ((below_at_above, MIN), (None, 0), (None, 1), (None, MIN), (wild, 2 ** 31 - 1), (wild, 0)):
            for allowed in (None, half):
                kw = dict(hold_token=hold, emitted=emitted, min_emitted=mn)
                got = _sample(x, u, mode, allowed=allowed, **kw)
                _same(got, _sample(_minus_inf_copy(x, allowed, **{"hold": hold, "emitted": emitted, "min_emitted": mn}), u, mode), (V, B, mode, mn))
                e = torch.zeros(B, dtype=torch.int64, device=DEV) if emitted is None else emitted.long()
                held = e < mn
                assert (got[0][held] != hold).all(), (V, B, mode, mn)            # a held token is never drawn
                if mode.get("T") == 0.0 and allowed is None:
                    assert (got[0][~held] == hold).all()                          # and comes at once when it may: it is the maximum
        for outside in (-1, V, V + 7, 2 ** 40, -2 ** 40):                        # holds nothing
            _same(_sample(x, u, mode, hold_token=outside, min_emitted=3), plain, (V, B, mode, outside))


# =================================================================================================== 1. exact equivalence: the verification
def _verify(p, q, x, ua, ud, mode, **con):
    greedy = mode.get("T") == 0.0
    return _ops().spec_verify(p, None if greedy else q, x, None if greedy else ua, None if greedy else ud, mode.get("T", 1.0), mode.get("k"), mode.get("p"),
                              **con)


def _verify_copy(p, q, allowed, hold, emitted, mn):
    k = q.shape[1]
    pc = torch.stack([_S().constrain_reference(p[:, j], allowed, hold, emitted, mn, j) for j in range(k + 1)], dim=1)
    qc = torch.stack([_S().constrain_reference(q[:, j], allowed, hold, emitted, mn, j) for j in range(k)], dim=1)
    return THV._in_ld(pc), THV._in_ld(qc)


@pytest.mark.parametrize("k", [1, 4])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("V", VS)
def test_verification_equals_the_unrestricted_call_on_minus_inf_copies(V, B, k):
    p, q, draws, ua, ud = THV._inputs(B, k, V, 13 * V + 5 * B + k, related=True)
    hold = (V - 1) if V % 8 else V // 2 + 3
    p[:, :, hold] += 6.0                                                         # the held token is likely wherever it may be drawn
    q[:, :, hold] += 6.0
    rows = _half((B, V), V + k)
    rows[:, [0, hold]] = True
    MIN = 6
    crossing = torch.tensor([MIN - 2, MIN - 1, 0][:B], dtype=I32, device=DEV)    # emitted + j reaches MIN inside the block (k = 4), at once, never
    seen_excluded = seen_hold_change = False
    for i, mode in enumerate(MODES):
        for allowed, emitted, mn in ((None, None, 0), (rows, None, 0), (rows[0], crossing, MIN), (None, crossing, MIN), (rows, None, MIN)):
            pc, qc = _verify_copy(p, q, allowed, hold, emitted, mn)
            # drafts as the restricted draft would draw them; then one of them is replaced by a token the restriction excludes
            x = torch.stack([_ops().sample_logits(qc[:, j], None if mode.get("T") == 0.0 else draws[j], mode.get("T", 1.0), mode.get("k"), mode.get("p"))
                             for j in range(k)], dim=1)
            j = (k - 1) // 2
            if allowed is not None:
                a = allowed.expand(B, V)
                x[0, j] = int((~a[0]).nonzero()[0])
            elif mn > 0:
                x[0, j] = hold                                                   # held at position j of row 0 (emitted[0] + j < MIN)
            kw = dict(allowed=allowed, hold_token=hold, emitted=emitted, min_emitted=mn)
            got = _verify(p, q, x, ua, ud, mode, **kw)
            want = _verify(pc, qc, x, ua, ud, mode)
            _same(got, want, (V, B, k, mode, mn))
            _same(_verify(p, q, x, ua, ud, mode, **kw), got, "repeatable")
            if allowed is not None or mn > 0:
                assert int(got[0][0]) <= j, (V, B, k, mode)                       # the excluded draft never stands
                seen_excluded = True
                excl = torch.isneginf(pc[torch.arange(B), got[0].long()].float().gather(1, got[1].unsqueeze(1)))
                assert not excl.any()                                            # and the token behind the accepted ones is not excluded
            if allowed is None and mn == 0:
                _same(got, _verify(p, q, x, ua, ud, mode), "nothing restricted is the plain call")
            if emitted is not None and k == 4:
                seen_hold_change = seen_hold_change or bool(torch.isneginf(pc[0, 0, hold].float()) and not torch.isneginf(pc[0, k, hold].float()))
    assert seen_excluded and (seen_hold_change or k < 4)


# =================================================================================================== 2. against the float64 rule
class _Shim:
    """``ops`` for the existing tests' ``_check``: the call under test runs constrained on the untouched logits, whatever -inf copy it is handed"""

    def __init__(self, **replace):
        self._replace = replace

    def __getattr__(self, name):
        return self._replace.get(name) or getattr(_ops(), name)


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("V", VS)
def test_sampler_against_the_float64_rule(V, B, monkeypatch):
    x = THS._logits(B, V, 2.0, 5 * V + B)
    hold = V // 2
    x[:, hold] += 4.0
    rows = _half((B, V), V + 2)
    rows[:, [0, hold]] = True
    emitted = torch.tensor([1, 3, 2][:B], dtype=I32, device=DEV)
    con = dict(allowed=rows, hold_token=hold, emitted=emitted, min_emitted=3)
    xc = _minus_inf_copy(x, rows, hold, emitted, 3)
    monkeypatch.setattr(THS, "_ops", lambda: _Shim(sample_logits=lambda _, u, T, k, p, return_kept: _ops().sample_logits(x, u, T, k, p, return_kept=True, **con)))
    worst = 0.0
    for i, kw in enumerate(THS._settings(V)):
        worst = max(worst, THS._check(xc, THS._rand(B, 3 * V + i), what=f"V={V} B={B} {kw}", **kw))
    print(f"constrained sample_logits V={V} B={B}: largest deviation of u from the token's reference interval {worst:.3g}")


def _verify_case(B, k, V, seed, device):
    """p, q, uniforms, the restriction and the -inf copies; the copies' draft rows are re-shaped as tests/test_hip_spec.py shapes its own, so
    that the residual keeps mass: the column of the restricted target's maximum trades places with the restricted draft row's minimum"""
    S = _S()
    p, q, draws, ua, ud = THV._raw_inputs(B, k, V, seed, related=True)
    g = torch.Generator().manual_seed(seed + 1)
    rows = torch.rand(B, V, generator=g) < 0.5
    hold = V // 2
    rows[:, [0, hold]] = True
    emitted = torch.tensor([4, 5, 0][:B], dtype=I32)
    MIN = 6
    excluded = torch.stack([torch.isneginf(S.constrain_reference(torch.zeros(B, V), rows, hold, emitted, MIN, j)) for j in range(k + 1)], dim=1)
    c = p[:, :k].float().masked_fill(excluded[:, :k], -INF).argmax(dim=2, keepdim=True)
    d = q.float().masked_fill(excluded[:, :k], INF).argmin(dim=2, keepdim=True)
    qc_, qd_ = q.gather(2, c), q.gather(2, d)
    q = q.scatter(2, c, qd_).scatter(2, d, torch.where(c == d, qd_, qc_))
    con = dict(allowed=rows.to(device), hold_token=hold, emitted=emitted.to(device), min_emitted=MIN)
    pc = p.masked_fill(excluded, -INF)
    qc = q.masked_fill(excluded[:, :k], -INF)
    return p, q, pc, qc, draws, ua, ud, con


@pytest.mark.parametrize("k", [1, 4])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("V", VS)
def test_verification_against_the_float64_rule(V, B, k, monkeypatch):
    S = _S()
    p, q, pc, qc, draws, ua, ud, con = _verify_case(B, k, V, 3 * V + 7 * B + k + 9, DEV)
    for kw in THV.SETTINGS:                                                      # the reference alone, before the kernel: Z >= MIN_Z at every position
        if kw.get("k") == 1:
            continue
        P, Q = S.verify_distributions(pc, qc, kw.get("T", 1.0), kw.get("k"), kw.get("p"))
        z = (P[:, :k] - Q).clamp(min=0).sum(dim=2)
        assert (z >= THV.MIN_Z).all(), (kw, float(z.min()))
    pd, qd = THV._in_ld(p), THV._in_ld(q)
    pcd, qcd = THV._in_ld(pc), THV._in_ld(qc)
    draws, ua, ud = draws.to(DEV), ua.to(DEV), ud.to(DEV)
    monkeypatch.setattr(THV, "_ops", lambda: _Shim(spec_verify=lambda _p, _q, x, a, d, T, tk, tp: _ops().spec_verify(pd, qd, x, a, d, T, tk, tp, **con)))
    worst = [0.0, 0.0]
    for kw in THV.SETTINGS:
        T, tk, tp = kw.get("T", 1.0), kw.get("k"), kw.get("p")
        x = THV._drafts(qcd, draws, T, tk, tp)
        got = THV._check(pcd, qcd, x, ua, ud, T, tk, tp, what=f"B={B} k={k} V={V} {kw}")
        worst = [max(a, b) for a, b in zip(worst, got)]
    print(f"constrained spec_verify V={V} B={B} k={k}: u_accept over its bound by at most {worst[0]:.3g}, u_draw outside the token's interval by at most "
          f"{worst[1]:.3g} (x Z)")


# =================================================================================================== 3. nothing outside the problem
@pytest.mark.parametrize("V", [250, 2056, 65536])
def test_mask_and_emitted_in_fenced_buffers(V):
    """the mask rows (ceil(V / 8) bytes each, allowed_ld 3 more) and emitted inside poisoned buffers at 16-byte-and-no-more alignment: the
    results are those of the call on plain tensors whatever the poison is — zeros would exclude, ones allow — and nothing is written"""
    B, k = 3, 4
    nb = (V + 7) // 8
    x, u = THS._logits(B, V, 2.0, V + 41), THS._rand(B, V + 42)
    p, q, draws, ua, ud = THV._inputs(B, k, V, V + 43, related=True)
    hold = V - 1
    x[:, hold] = 20.0
    rows = _half((B, V), V + 44)
    rows[:, [0, hold]] = True
    packed = _ops().pack_token_mask(rows)
    emitted = torch.tensor([1, 2, 3], dtype=I32, device=DEV)
    xd = torch.stack([_ops().sample_logits(q[:, j], draws[j]) for j in range(k)], dim=1)
    for mode in (MODES[0], MODES[4]):
        want_s = _sample(x, u, mode, allowed_packed=packed, hold_token=hold, emitted=emitted, min_emitted=3)
        want_v = _verify(p, q, xd, ua, ud, mode, allowed_packed=packed, hold_token=hold, emitted=emitted, min_emitted=3)
        for poison in (0x00, 0xFF):
            mf, hm = fenced(packed, poison=poison, ld=nb + 3)
            ef, he = fenced(emitted, poison=0x7FFFFFFF if poison else 0)
            tf, ht = fenced((B,), dtype=torch.int64, poison="mark")
            assert mf.data_ptr() % 32 == 16 and mf.stride(0) == nb + 3 and ef.data_ptr() % 32 == 16
            got = _ops().sample_logits(x, u, mode.get("T", 1.0), mode.get("k"), mode.get("p"), return_kept=True, out=tf, allowed_packed=mf, hold_token=hold,
                                       emitted=ef, min_emitted=3)
            assert_same_bits(got[0], want_s[0], f"token {V} {mode}")
            assert_same_bits(got[1], want_s[1], f"n_kept {V} {mode}")
            gv = _verify(p, q, xd, ua, ud, mode, allowed_packed=mf, hold_token=hold, emitted=ef, min_emitted=3)
            assert_same_bits(gv[0], want_v[0], f"n_accept {V} {mode}")
            assert_same_bits(gv[1], want_v[1], f"verified token {V} {mode}")
            assert_guards(hm, he, ht)
            assert torch.equal(mf, packed) and torch.equal(ef, emitted)


# =================================================================================================== 4. rows and repeatability
@pytest.mark.parametrize("V", [250, 16392])
def test_a_row_depends_on_itself_alone_and_calls_repeat(V):
    B, k = 3, 4
    x, u = THS._logits(B, V, 2.0, V + 51), THS._rand(B, V + 52)
    p, q, draws, ua, ud = THV._inputs(B, k, V, V + 53, related=True)
    hold = V // 2
    rows = _half((B, V), V + 54)
    rows[:, [0, hold]] = True
    packed = _ops().pack_token_mask(rows)
    emitted = torch.tensor([0, 4, 9], dtype=I32, device=DEV)
    xd = torch.stack([_ops().sample_logits(q[:, j], draws[j]) for j in range(k)], dim=1)
    for mode in MODES:
        kw = dict(hold_token=hold, min_emitted=5)
        s3 = _sample(x, u, mode, allowed_packed=packed, emitted=emitted, **kw)
        v3 = _verify(p, q, xd, ua, ud, mode, allowed_packed=packed, emitted=emitted, **kw)
        _same(_sample(x, u, mode, allowed_packed=packed, emitted=emitted, **kw), s3, "repeatable")
        _same(_verify(p, q, xd, ua, ud, mode, allowed_packed=packed, emitted=emitted, **kw), v3, "repeatable")
        for b in range(B):
            s1 = _sample(THS._in_ld(x[b:b + 1]), u[b:b + 1], mode, allowed_packed=packed[b:b + 1], emitted=emitted[b:b + 1].clone(), **kw)
            v1 = _verify(THV._in_ld(p[b:b + 1]), THV._in_ld(q[b:b + 1]), xd[b:b + 1], ua[b:b + 1].clone(), ud[b:b + 1].clone(), mode,
                         allowed_packed=packed[b], emitted=emitted[b:b + 1].clone(), **kw)
            _same(s1, (s3[0][b:b + 1], s3[1][b:b + 1]), (V, mode, b))
            _same(v1, (v3[0][b:b + 1], v3[1][b:b + 1]), (V, mode, b))


def test_ops_shape_errors_are_value_errors_in_the_functions_name():
    x = THS._logits(2, 64, 1.0, 1)
    ok = torch.ones(64, dtype=torch.bool, device=DEV)
    for kw in (dict(allowed=ok[:63]), dict(allowed=ok.expand(3, 64)), dict(allowed=ok, allowed_packed=_ops().pack_token_mask(ok)),
               dict(allowed_packed=torch.zeros(7, dtype=torch.uint8, device=DEV)), dict(allowed_packed=torch.zeros(3, 8, dtype=torch.uint8, device=DEV)),
               dict(allowed_packed=torch.zeros(2, 16, dtype=torch.uint8, device=DEV)[:, ::2]), dict(emitted=torch.zeros(3, dtype=I32, device=DEV)),
               dict(min_emitted=-1), dict(min_emitted=2 ** 31), dict(min_emitted=1.5)):
        with pytest.raises(ValueError, match="sample_logits"):
            _ops().sample_logits(x, None, **kw)
    p = torch.zeros(2, 3, 64, dtype=BF, device=DEV)
    d = torch.zeros(2, 2, dtype=torch.int64, device=DEV)
    for kw in (dict(allowed=ok[:63]), dict(emitted=torch.zeros(2, 1, dtype=I32, device=DEV)), dict(min_emitted=-1)):
        with pytest.raises(ValueError, match="spec_verify"):
            _ops().spec_verify(p, None, d, **kw)


# =================================================================================================== 5. through the model
T0, NEW, MIN = 130, 10, 6
LENS = (97, 130)


def _model_case():
    """the generation tests' model (block 200, vocabulary 512, 2 layers), and from the oracle's own logits behind the prompts: an eos that
    is likely in every row, and per output row four unlikely tokens — row r may emit its four and eos, nothing else"""
    c = THS._case()
    at = torch.stack([c["logits"][0, T0 - 1], c["logits"][1, T0 - 1], c["logits"][0, LENS[0] - 1]]).float()
    eos = int(at.min(dim=0).values.argmax())
    low = at.max(dim=0).values.argsort()[:16].tolist()
    V = at.shape[1]
    rows = torch.zeros(4, V, dtype=torch.bool)
    for r in range(4):
        rows[r, low[4 * r:4 * r + 4]] = True
    rows[:, eos] = True
    return c["m"], c["ids"][:, :T0].to(DEV), eos, rows.to(DEV)


def _new_tokens(out, t0s, lens=None):
    """row r's new tokens up to and including its first eos-or-end"""
    return [out[r, t0:(int(lens[r]) if lens is not None else out.shape[1])] for r, t0 in enumerate(t0s)]


def _assert_constrained(tokens, rows, eos, must_hold):
    for r, t in enumerate(tokens):
        assert t.numel() > 0 and bool(rows[r][t].all()), (r, t.tolist())          # every token in the row's set
        first = (t == eos).nonzero().flatten()
        n_before = int(first[0]) if first.numel() else t.numel()
        if must_hold:
            assert n_before >= min(MIN, t.numel()), (r, t.tolist())              # no eos among the first MIN
        else:
            assert n_before < MIN, (r, t.tolist())                               # the run that may emit it early does: the test is not vacuous


PATHS = [dict(sampler="torch"), dict(sampler="device"), dict(sampler="device", lengths=LENS), dict(sampler="device", kv_dtype="fp8"),
         dict(sampler="torch", num_samples=2), dict(sampler="device", loop="device"), dict(sampler="device", loop="graph"),
         dict(sampler="device", loop="graph", lengths=LENS)]


@pytest.mark.parametrize("path", PATHS, ids=lambda d: "-".join(f"{k}={v}" for k, v in d.items()))
def test_generate_stays_in_the_allowed_set_and_holds_eos(path):
    m, idx, eos, rows = _model_case()
    n_rows = 4 if path.get("num_samples") else 2
    allowed = rows[:n_rows]
    if "lengths" in path:
        from test_hip_generate_rows import _ragged_prompt
        idx = _ragged_prompt(THS._case())
    t0s = list(path.get("lengths", [T0] * n_rows))
    kw = dict(temperature=0.5, eos_token=eos, allowed_tokens=allowed, **path)
    for min_new in (0, MIN):
        out = m.generate(idx, NEW, generator=_gen(21), min_new_tokens=min_new, **kw)
        lens = None
        if "lengths" in path:
            out, lens = out
        assert out.shape[0] == n_rows
        _assert_constrained(_new_tokens(out, t0s, lens), allowed, eos, must_hold=min_new > 0)
    again = m.generate(idx, NEW, generator=_gen(21), min_new_tokens=MIN, **kw)
    assert torch.equal(again[0] if "lengths" in path else again, out)            # seeded: repeatable
    ids = allowed[0].nonzero().flatten().tolist()                                # the same set as a list of ids, for every row
    if "lengths" not in path:
        out_ids = m.generate(idx, NEW, generator=_gen(21), min_new_tokens=MIN, **dict(kw, allowed_tokens=ids))
        _assert_constrained(_new_tokens(out_ids, t0s), allowed[:1].expand(n_rows, -1), eos, must_hold=True)


def test_the_device_loop_and_the_graph_agree_bit_for_bit():
    m, idx, eos, rows = _model_case()
    kw = dict(temperature=0.5, eos_token=eos, allowed_tokens=rows[:2], min_new_tokens=MIN, sampler="device")
    a = m.generate(idx, NEW, generator=_gen(5), loop="device", **kw)
    b = m.generate(idx, NEW, generator=_gen(5), loop="graph", **kw)
    assert torch.equal(a, b)
    only_len = dict(kw, allowed_tokens=None)
    assert torch.equal(m.generate(idx, NEW, generator=_gen(5), loop="device", **only_len), m.generate(idx, NEW, generator=_gen(5), loop="graph", **only_len))


@pytest.mark.parametrize("path", [dict(sampler="torch"), dict(sampler="device"), dict(sampler="device", loop="graph"), dict(sampler="torch", num_samples=2)],
                         ids=lambda d: "-".join(f"{k}={v}" for k, v in d.items()))
def test_the_whole_vocabulary_and_no_minimum_change_nothing(path):
    m, idx, eos, rows = _model_case()
    kw = dict(temperature=0.9, top_k=50, eos_token=eos, **path)
    want = m.generate(idx, NEW, generator=_gen(9), **kw)
    everything = torch.ones(rows.shape[1], dtype=torch.bool, device=DEV)
    assert torch.equal(m.generate(idx, NEW, generator=_gen(9), allowed_tokens=everything, min_new_tokens=0, **kw), want)
    assert torch.equal(m.generate(idx, NEW, generator=_gen(9), allowed_tokens=list(range(rows.shape[1])), **kw), want)


@pytest.mark.parametrize("lengths", [None, LENS])
def test_generate_speculative_stays_in_the_allowed_set_and_holds_eos(lengths):
    m, idx, eos, rows = _model_case()
    draft = THV._one_layer_draft()
    allowed = rows[:2]
    if lengths is not None:
        from test_hip_generate_rows import _ragged_prompt
        idx = _ragged_prompt(THS._case())
    t0s = list(lengths or [T0, T0])
    kw = dict(k=4, temperature=0.5, eos_token=eos, allowed_tokens=allowed, lengths=lengths)
    for min_new in (0, MIN):
        out = m.generate_speculative(idx, NEW, draft, generator=_gen(31), min_new_tokens=min_new, **kw)
        lens = None
        if lengths is not None:
            out, lens = out
        _assert_constrained(_new_tokens(out, t0s, lens), allowed, eos, must_hold=min_new > 0)
    again = m.generate_speculative(idx, NEW, draft, generator=_gen(31), min_new_tokens=MIN, **kw)
    assert torch.equal(again[0] if lengths is not None else again, out)
    greedy = m.generate_speculative(idx, NEW, draft, top_k=1, eos_token=eos, allowed_tokens=allowed, min_new_tokens=MIN, lengths=lengths)
    greedy, lens = greedy if lengths is not None else (greedy, None)
    _assert_constrained(_new_tokens(greedy, t0s, lens), allowed, eos, must_hold=True)
