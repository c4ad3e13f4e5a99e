"""Host-side tests (no GPU) of speculative decoding: the symbol table of the verification kernel against its companion header, every
argument check of obte_spec_verify_bf16 that returns before a launch, the rule's plain-torch statement (sampling.verify_reference) on
its edge cases, CachePositions.rewind_rows, and the validation of generate_speculative."""
import ctypes as C
import os
import re

import pytest
import torch

from omnibiote_amd import _lib

EINVAL, EUNSUPPORTED = -1, -3
P = 4096   # a non-null, 16-byte aligned "pointer" for calls that must return before they touch it
NAMES = ("obte_spec_verify_ws_bytes", "obte_spec_verify_bf16")
BF = torch.bfloat16
INF, NAN = float("inf"), float("nan")


def _err():
    return _lib.lib().obte_last_error().decode()


def test_spec_symbols_have_their_own_table():
    lib = _lib.lib()
    assert tuple(_lib.SYMBOLS_SPEC) == NAMES
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "omnibiote_hip_spec.h")).read()
    assert set(re.findall(r"^(?:int|int64_t|void|const char\*) +(obte_[a-z0-9_]+)\(", header, flags=re.M)) == set(NAMES)
    assert len(re.findall(r"^[a-z0-9_\* ]+\bobte_[a-z0-9_]+\(", header, flags=re.M)) == len(NAMES)      # and nothing else
    for name in NAMES:
        for table in (_lib.SYMBOLS, _lib.SYMBOLS_ROWS, _lib.SYMBOLS_SMALL_M, _lib.SYMBOLS_SAMPLE, _lib.SYMBOLS_EXTEND):
            assert name not in table
        fn = getattr(lib, name)
        res, args = _lib.SYMBOLS_SPEC[name]
        assert fn.restype is res and list(fn.argtypes) == args                                            # bound by lib(), in the same loop
    assert len(_lib.SYMBOLS) == 70 and len(_lib.SYMBOLS_SAMPLE) == 1
    assert lib.obte_abi_version() == 1
    sizes = (C.c_int64 * 16)()
    assert lib.obte_struct_sizes(sizes, 16) == 6


def test_workspace_size():
    ws = _lib.lib().obte_spec_verify_ws_bytes
    assert ws(1, 1) == 3 * 32 and ws(8, 4) == 8 * 9 * 32 and ws(64, 31) == 64 * 63 * 32
    assert ws(0, 4) == 0 and ws(2, 0) == 0 and ws(2, 32) == 0


def _call(p=P, ld_p=1008, q=P, ld_q=1008, draft=P, B=2, k=4, V=1003, u_accept=P, u_draw=P, temperature=1.0, top_k=0, top_p=1.0, n_accept=P, token=P,
          ws=P, ws_bytes=1 << 20):
    return _lib.lib().obte_spec_verify_bf16(p, ld_p, q, ld_q, draft, B, k, V, u_accept, u_draw, temperature, top_k, top_p, n_accept, token, ws, ws_bytes, None)


@pytest.mark.parametrize("kw,rc,word", [
    (dict(p=None), EINVAL, "null"), (dict(draft=None), EINVAL, "null"), (dict(n_accept=None), EINVAL, "null"), (dict(token=None), EINVAL, "null"),
    (dict(ws=None), EINVAL, "null"), (dict(q=None), EINVAL, "null pointer (q)"),
    (dict(p=P + 8), EINVAL, "p must be 16-byte"), (dict(q=P + 2), EINVAL, "q must be 16-byte"),
    (dict(ld_p=1004), EINVAL, "ld_p"), (dict(ld_p=1000), EINVAL, "ld_p"), (dict(ld_q=1012), EINVAL, "ld_q"), (dict(ld_q=1000), EINVAL, "ld_q"),
    (dict(B=0), EINVAL, "B"), (dict(B=-3), EINVAL, "B"), (dict(k=0), EINVAL, "k"), (dict(k=-1), EINVAL, "k"), (dict(V=0, ld_p=8, ld_q=8), EINVAL, "V"),
    (dict(temperature=-0.5), EINVAL, "temperature"), (dict(temperature=INF), EINVAL, "temperature"), (dict(temperature=NAN), EINVAL, "temperature"),
    (dict(top_p=0.0), EINVAL, "top_p"), (dict(top_p=-0.1), EINVAL, "top_p"), (dict(top_p=1.0001), EINVAL, "top_p"), (dict(top_p=NAN), EINVAL, "top_p"),
    (dict(u_accept=P + 2), EINVAL, "u_accept must be 4-byte"), (dict(u_draw=P + 1), EINVAL, "u_draw must be 4-byte"),
    (dict(n_accept=P + 2), EINVAL, "n_accept must be 4-byte"), (dict(token=P + 4), EINVAL, "token must be 8-byte"),
    (dict(draft=P + 4), EINVAL, "draft must be 8-byte"), (dict(ws=P + 4), EINVAL, "ws must be 8-byte"),
    (dict(ws_bytes=2 * 9 * 32 - 1), EINVAL, "workspace"), (dict(ws_bytes=0), EINVAL, "workspace"),
    (dict(k=32), EUNSUPPORTED, "k = 32"), (dict(k=1000), EUNSUPPORTED, "k"),
    (dict(V=65537, ld_p=65544, ld_q=65544), EUNSUPPORTED, "65537"), (dict(V=1 << 20, ld_p=1 << 20, ld_q=1 << 20), EUNSUPPORTED, "V"),
])
def test_spec_verify_rejects_before_any_launch(kw, rc, word):
    assert _call(**kw) == rc
    assert _err().startswith("obte_spec_verify_bf16:") and word in _err(), _err()


def test_a_greedy_call_needs_no_draft_logits_but_the_other_checks_hold():
    """q = NULL passes the q checks when the call is greedy (no uniforms, T = 0 or top_k = 1): the next check is the one that answers"""
    for kw in (dict(u_accept=None, u_draw=None), dict(temperature=0.0), dict(top_k=1), dict(u_draw=None)):
        assert _call(q=None, ld_q=0, ws_bytes=0, **kw) == EINVAL and "workspace" in _err(), (kw, _err())


def test_ops_spec_verify_refuses_cpu_tensors_and_bad_shapes():
    from omnibiote_amd import ops
    p, q, x = torch.zeros(2, 5, 16, dtype=BF), torch.zeros(2, 4, 16, dtype=BF), torch.zeros(2, 4, dtype=torch.int64)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.spec_verify(p, q, x, torch.zeros(2, 4), torch.zeros(2))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.spec_verify(p, None, x)


# ----------------------------------------------------------------------------------------------- the rule in plain torch
def _rows(b, r, v, seed, s=2.0):
    return (torch.randn(b, r, v, generator=torch.Generator().manual_seed(seed)) * s).to(BF)


def _ref(*a, **kw):
    from omnibiote_amd.sampling import verify_reference
    return verify_reference(*a, **kw)


def test_reference_accepts_everything_when_the_draft_is_the_target():
    from omnibiote_amd.sampling import sample_reference
    B, k, V = 3, 4, 300
    p = _rows(B, k + 1, V, 1)
    g = torch.Generator().manual_seed(2)
    for kw in (dict(), dict(temperature=0.8, top_k=20), dict(top_p=0.9)):
        x = torch.stack([sample_reference(p[:, j], torch.rand(B, generator=g), **kw)[0] for j in range(k)], dim=1)   # drawn from q = p
        for ua in (torch.rand(B, k, generator=g), torch.full((B, k), 0.99999994)):
            ud = torch.rand(B, generator=g)
            a, tok, cdf = _ref(p, p[:, :k], x, ua, ud, **kw)
            bonus = sample_reference(p[:, k], ud, **kw)
            assert a.tolist() == [k] * B and torch.equal(tok, bonus[0]) and torch.equal(cdf, bonus[2]), kw
    # u = 1 accepts nothing (1 < 1 fails); then Z = 0 and the token comes from P_0
    a, tok, cdf = _ref(p, p[:, :k], x, torch.ones(B, k), ud)
    first = sample_reference(p[:, 0], ud)
    assert a.tolist() == [0] * B and torch.equal(tok, first[0]) and torch.allclose(cdf, first[2], atol=1e-15, rtol=0)


def test_reference_rejects_what_the_target_does_not_keep():
    B, k, V = 2, 3, 200
    p, q = _rows(B, k + 1, V, 3), _rows(B, k, V, 4)
    x = p[:, :k].float().argmax(dim=2)                                   # the target's favourites: kept under any top-k
    low = p[:, 1].float().argmin(dim=1)
    x[:, 1] = low                                                        # position 1: outside the target's top 20
    ua, ud = torch.zeros(B, k), torch.full((B,), 0.5)
    a, tok, cdf = _ref(p, q, x, ua, ud, top_k=20)
    assert a.tolist() == [1, 1]                                          # u = 0 accepts anything the target keeps, and nothing else
    assert (cdf.gather(1, low.unsqueeze(1)) - torch.where(low > 0, cdf.gather(1, (low - 1).clamp(min=0).unsqueeze(1)), torch.zeros(B, 1).double())
            == 0).all()                                                  # and the rejected token is not drawn in its place
    assert _ref(p, q, x, ua, ud)[0].tolist() == [k, k]                   # without the cut everything has P > 0
    for bad in (-1, V, 2 ** 62):                                         # outside [0, V): P = 0
        y = x.clone()
        y[0, 0] = bad
        y[1, 2] = bad
        assert _ref(p, q, y, ua, ud)[0].tolist() == [0, 2], bad


def test_reference_q_zero_and_z_zero():
    V = 8
    p = torch.full((1, 3, V), -INF)
    q = torch.full((1, 2, V), -INF)
    p[0, :, :4] = 0.0                                                    # P uniform on 0..3
    q[0, 0, 4:] = 0.0                                                    # Q_0 on 4..7: Q_0(x) = 0 wherever P_0 > 0
    q[0, 1, :4] = 0.0                                                    # Q_1 = P_1
    x = torch.tensor([[2, 3]])
    a, tok, cdf = _ref(p, q, x, torch.tensor([[0.999, 1.0]]), torch.tensor([0.6]))
    assert int(a) == 1                                                   # Q(x) = 0 < P(x) stands at any u; then ratio 1 fails at u = 1
    assert int(tok) == 2 and torch.allclose(cdf[0], torch.tensor([0.25, 0.5, 0.75, 1, 1, 1, 1, 1]).double())   # Z = 0: the draw is from P_1
    a, tok, _ = _ref(p, q, torch.tensor([[5, 0]]), torch.zeros(1, 2), torch.tensor([0.6]))
    assert int(a) == 0 and int(tok) == 2                                 # P(5) = 0 falls at u = 0; residual max(0, P_0 - Q_0) = P_0
    # a proper residual: P = (1/2, 1/2, 0, ..), Q = (3/4, 1/4, 0, ..): max(0, P - Q) puts everything on index 1
    p2 = torch.full((1, 2, V), -INF)
    q2 = torch.full((1, 1, V), -INF)
    p2[0, :, :2] = 0.0
    q2[0, 0, 0], q2[0, 0, 1] = float(torch.log(torch.tensor(3.0))), 0.0
    a, tok, cdf = _ref(p2, q2, torch.tensor([[0]]), torch.tensor([[0.7]]), torch.tensor([0.01]))       # ratio (1/2) / (3/4) = 2/3 < 0.7
    assert int(a) == 0 and int(tok) == 1 and cdf[0, 0] == 0 and cdf[0, 1] == 1
    assert int(_ref(p2, q2, torch.tensor([[0]]), torch.tensor([[0.6]]), torch.tensor([0.01]))[0]) == 1


def test_reference_greedy_and_nan_uniforms():
    B, k, V = 2, 3, 50
    p, q = _rows(B, k + 1, V, 7), _rows(B, k, V, 8)
    p[0, 1, 7] = p[0, 1, 30] = 40.0                                      # a tie for the maximum: the lower index
    top = p.float().argmax(dim=2)
    top[0, 1] = 7
    x = top[:, :k].clone()
    x[1, 2] = (x[1, 2] + 1) % V
    for kw in (dict(), dict(u_accept=torch.rand(B, k), u_draw=torch.rand(B), top_k=1), dict(u_accept=torch.rand(B, k), u_draw=torch.rand(B), temperature=0)):
        a, tok, cdf = _ref(p, None, x, **kw)
        assert a.tolist() == [k, 2] and tok.tolist() == [int(top[0, k]), int(top[1, 2])]
        assert cdf.shape == (B, V) and cdf[1, int(tok[1])] == 1 and cdf[1, :int(tok[1])].sum() == 0
    y = x.clone()
    y[0, 1] = 30                                                         # the tie's higher index is not the argmax
    assert _ref(p, None, y)[0].tolist() == [1, 2]
    # NaN or negative u_accept counts as 0 (everything the target keeps stands); NaN u_draw draws the first entry
    xs = p[:, :k].float().argmax(dim=2)
    for bad in (NAN, -3.0):
        a, tok, cdf = _ref(p, q, xs, torch.full((B, k), bad), torch.full((B,), NAN))
        assert a.tolist() == [k, k] and tok.tolist() == [0, 0]
    a1, t1, c1 = _ref(p[0], q[0], xs[0], torch.full((k,), 0.3), 0.4)     # one row in, scalars out
    a2, t2, c2 = _ref(p, q, xs, torch.full((B, k), 0.3), torch.full((B,), 0.4))
    assert int(a1) == int(a2[0]) and int(t1) == int(t2[0]) and torch.equal(c1, c2[0]) and c1.shape == (V,)


def test_reference_first_token_is_distributed_as_the_target():
    """the point of the rule: x_0 if it stands, else the residual's draw, has the target's distribution P_0 whatever Q_0 is — exactly, by
    summing over every drafted token: P(i) = Q(i) min(1, P(i) / Q(i)) + (1 - sum_x Q(x) min(1, P(x) / Q(x))) R(i)"""
    from omnibiote_amd.sampling import verify_distributions
    V = 16
    p, q = _rows(1, 2, V, 11), _rows(1, 1, V, 12)
    P, Q = verify_distributions(p, q, top_k=10)
    P0, Q0 = P[0, 0], Q[0, 0]
    out = torch.zeros(V, dtype=torch.float64)
    for x in range(V):
        if Q0[x] == 0:
            continue
        ratio = min(1.0, float(P0[x] / Q0[x]))
        a_lo = int(_ref(p, q, torch.tensor([[x]]), torch.tensor([[ratio * 0.999]]), torch.tensor([0.5]), top_k=10)[0])
        a_hi = int(_ref(p, q, torch.tensor([[x]]), torch.tensor([[ratio * 1.001 + 1e-9]]), torch.tensor([0.5]), top_k=10)[0])
        assert a_lo == (1 if P0[x] > 0 else 0) and (a_hi == 0 or ratio == 1.0), x
        out[x] += Q0[x] * ratio
        cdf = _ref(p, q, torch.tensor([[x]]), torch.tensor([[1.0]]), torch.tensor([0.5]), top_k=10)[2][0]   # u = 1: rejected (ratio <= 1 here or not)
        if ratio < 1.0:
            out += Q0[x] * (1 - ratio) * torch.diff(cdf, prepend=torch.zeros(1, dtype=torch.float64))
    assert torch.allclose(out, P0, atol=1e-12, rtol=0), (out - P0).abs().max()


# ----------------------------------------------------------------------------------------------- CachePositions.rewind_rows
def test_rewind_rows_on_bare_positions():
    from omnibiote_amd.model import CachePositions
    c = CachePositions(4, 64)
    with pytest.raises(ValueError, match="uniform"):
        c.rewind_rows([0, 0, 0, 0])
    c.reset(30, torch.tensor([30, 12, -1, 20], dtype=torch.int32), 12)   # row 2 parked
    c.advance(5)
    assert c.positions.tolist() == [35, 17, -1, 25] and (c.pos, c.min_pos) == (35, 17)
    c.rewind_rows([4, 0, 3, 1])
    assert c.positions.tolist() == [31, 17, -1, 24] and (c.pos, c.min_pos) == (31, 17) and c.positions.dtype == torch.int32
    c.rewind_rows([10, 0, 0, 2], now=[31, 17, -1, 24])                   # the caller's own account: nothing is read back
    assert c.positions.tolist() == [21, 17, -1, 22] and (c.pos, c.min_pos) == (22, 17)
    c.rewind_rows(torch.tensor([0, 16, 99, 0]))                          # down to one position; a parked row's count is not looked at
    assert c.positions.tolist() == [21, 1, -1, 22] and (c.pos, c.min_pos) == (22, 1)
    before = c.positions
    for bad, word in (([0, 1, 0, 0], "fewer than one"), ([22, 0, 0, 0], "fewer than one"), ([0, 0, 0], "counts for"), ([0, -1, 0, 0], "negative"),
                      (3, "sequence")):
        with pytest.raises(ValueError, match=word):
            c.rewind_rows(bad)
    assert c.positions is before and (c.pos, c.min_pos) == (22, 1)       # a refused call changes nothing
    c.park(torch.tensor([True, True, True, True]))
    c.rewind_rows([5, 5, 5, 5])
    assert c.positions.tolist() == [-1] * 4 and (c.pos, c.min_pos) == (22, 1)
    u = CachePositions(2, 16)
    u.reset(9)
    with pytest.raises(ValueError, match="uniform"):
        u.rewind_rows([1, 1])
    assert u.pos == 9


# ----------------------------------------------------------------------------------------------- generate_speculative's checks
def _model(vocab=64, block=32, layers=1, autoregressive=True):
    from omnibiote_amd.model import OmniBioTA, OmniBioTAConfig
    c = OmniBioTAConfig()
    c.block_size, c.vocab_size, c.n_layer, c.n_head, c.n_embd, c.dropout, c.flash = block, vocab, layers, 2, 128, 0.0, True
    c.autoregressive = autoregressive
    return OmniBioTA(c)


def test_generate_speculative_validates_before_any_device_work():
    m, d = _model(), _model(block=24)
    idx = torch.zeros(2, 8, dtype=torch.int64)
    for kw, word in ((dict(draft=_model(vocab=72)), "vocab_size"), (dict(draft=_model(autoregressive=False)), "autoregressive"),
                     (dict(draft=None), "draft"), (dict(draft=d, k=0), "k must"), (dict(draft=d, k=32), "k must"),
                     (dict(draft=d, top_p=0.0), "top_p"), (dict(draft=d, top_k=0), "top_k"), (dict(draft=d, temperature=-1.0), "temperature"),
                     (dict(draft=d, lengths=[8, 9]), "length"), (dict(draft=d, lengths=[8]), "lengths"),
                     (dict(draft=d, k=4, max_new_tokens=13), "block_size = 24"),          # 8 + 13 + 4 > the draft's 24
                     (dict(draft=m, k=4, max_new_tokens=21), "block_size = 32"),
                     (dict(draft=d, k=4, max_new_tokens=-1), "block_size")):
        kw = dict(dict(max_new_tokens=4), **kw)
        with pytest.raises(ValueError, match=word):
            m.generate_speculative(idx, **kw)
    with pytest.raises(ValueError, match="autoregressive"):
        _model(autoregressive=False).generate_speculative(idx, 4, d)
    with pytest.raises(ValueError, match="idx must be"):
        m.generate_speculative(idx[0], 4, d)
    # the bound is longest + new + k <= block_size exactly: 8 + 12 + 4 = 24 passes the checks and reaches the device code, which a CPU model refuses
    with pytest.raises(RuntimeError):
        m.generate_speculative(idx, 12, d, k=4)
    out, stats = m.generate_speculative(idx, 0, d, return_stats=True)    # nothing to generate: no device work at all
    assert torch.equal(out, idx) and stats == dict(rounds=0, drafted=0, accepted=0)
    out, n = m.generate_speculative(idx, 0, d, lengths=[8, 5])
    assert out.shape == (2, 8) and n.tolist() == [8, 5] and (out[1, 5:] == 0).all()
