"""obte_sample_logits_penalized_bf16 (include/omnibiote_hip_penalty.h) on the device, and the penalties of generate() / DecodeLoop.

The kernel tests have no tolerance: a penalised call returns, bit for bit, what the existing sampler returns on a bf16 copy of the logits
whose history columns were rewritten (sampling.penalize_reference makes the copy, in fp32 operations rounded one by one).  No case is
excluded from that comparison.  The model-level tests compare tokens with a hand-written loop of decode_step + penalize_reference +
ops.sample_logits, the loops with each other, and check a property that holds whatever the summation order: with 8 allowed ids, greedy
and a presence penalty above every logit, 8 new tokens are a permutation of the 8 ids."""
import pytest
import torch

import test_hip_sample as THS
from fenced import assert_guards, assert_same_bits, fenced
from test_hip_generate import _gen_case

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16
INF, NAN = float("inf"), float("nan")
I32, I64 = torch.int32, torch.int64
B = 3
VS = [5, 2048, 2049, 16384, 16385, 65536]                                        # both sides of the three launch shapes
MODES = [dict(T=0.0), dict(T=0.8, k=50, p=0.9), dict(T=1.0)]                     # greedy; top-k = 50 with top-p = 0.9; plain sampling
NUMBERS = [dict(repetition=1.3, presence=0.5, frequency=0.25), dict(repetition=0.7, presence=-0.75, frequency=1.5)]


def _ops():
    from omnibiote_amd import ops
    return ops


def _S():
    from omnibiote_amd import sampling
    return sampling


def _sample(x, u, mode, **kw):
    return _ops().sample_logits(x, u, mode.get("T", 1.0), mode.get("k"), mode.get("p"), return_kept=True, **kw)


def _pen(prompt=None, prompt_len=None, gen=None, n_gen=None, **numbers):
    return _ops().Penalty(prompt, prompt_len, gen, n_gen, **numbers)


def _copy(x, pen, prompt=None, gen=None):
    """the penalised bf16 copy of x in rows of ld = V rounded up to 8 like the original's; ``prompt`` / ``gen``: the lists the reference
    is to see in the penalty's place"""
    y = _S().penalize_reference(x, pen.prompt if prompt is None else prompt, pen.prompt_len, pen.gen if gen is None else gen, pen.n_gen,
                                pen.repetition, pen.presence, pen.frequency)
    assert y.dtype == BF and y.shape == x.shape
    return THS._in_ld(y)


def _same(got, want, what):
    for g, w, name in zip(got, want, ("token", "n_kept")):
        assert g.dtype == w.dtype and torch.equal(g, w), (what, name, g.tolist(), w.tolist())


def _logits(V, seed):
    """random bf16 of both signs; among each row's 8 largest columns — the ones every history below names — a -inf, a NaN and a 0 are
    planted, and in row 2 a +inf"""
    x = THS._logits(B, V, 2.0, seed)
    top = x.float().topk(min(8, V), dim=1).indices                              # (B, <= 8), the largest first
    n = top.shape[1]
    rows = torch.arange(B, device=DEV)
    x[rows, top[:, 1 % n]] = -INF
    x[rows, top[:, 2 % n]] = NAN
    x[rows, top[:, 3 % n]] = 0.0
    x[2, top[2, 4 % n]] = INF
    return x, top


def _histories(x, top):
    """(name, prompt, prompt_len, gen, n_gen) — the lists int64 (B, n) on the device, the counts None, a host integer or int32 (B,)"""
    V = x.shape[1]
    g = torch.Generator(device=DEV).manual_seed(V)
    n = top.shape[1]
    few = top[:, :min(4, n)]
    cases = []
    nothing = torch.zeros((B, 4), dtype=I64, device=DEV)
    cases.append(("empty, counted by the kernel", nothing, torch.zeros(B, dtype=I32, device=DEV), nothing, 0))
    cases.append(("length 1, prompt only", top[:, :1].contiguous(), None, None, None))
    cases.append(("length 1, generated only", None, None, top[:, :1].contiguous(), None))
    ends = torch.tensor([[0, V - 1, 0]] * B, dtype=I64, device=DEV)
    cases.append(("tokens 0 and V - 1", ends[:, :2].contiguous(), None, ends, None))
    dup = few.gather(1, torch.randint(0, few.shape[1], (B, 600), device=DEV, generator=g))
    wide = torch.cat([top, torch.randint(0, V, (B, 300), device=DEV, generator=g)], dim=1)
    cases.append(("heavy duplicates", wide, None, dup, None))
    cases.append(("host counts", wide, 9, dup, 411))
    cases.append(("per-row counts", wide, torch.tensor([0, 7, 308], dtype=I32, device=DEV), dup, torch.tensor([600, 1, 0], dtype=I32, device=DEV)))
    cases.append(("counts outside the width", wide, torch.tensor([-5, 2 ** 31 - 1, 309], dtype=I32, device=DEV), dup,
                  torch.tensor([-2 ** 31, 601, 2 ** 31 - 1], dtype=I32, device=DEV)))
    junk = torch.tensor([-1, V, 2 ** 40, -2 ** 63, 2 ** 63 - 1, 2 ** 32, V + 7, -V], dtype=I64, device=DEV)
    mixed = torch.cat([junk.expand(B, -1), top, junk.expand(B, -1)], dim=1)
    cases.append(("ids out of range", mixed, None, mixed.flip(1).contiguous(), None))
    strided = torch.full((B, 640), -7, dtype=I64, device=DEV)
    strided[:, :600] = dup
    cases.append(("strided rows", torch.cat([wide, wide], dim=1)[:, :308], None, strided[:, :600], torch.tensor([3, 600, 77], dtype=I32, device=DEV)))
    return cases


# =================================================================================================== 1. bit-for-bit equality
@pytest.mark.parametrize("V", VS)
def test_penalized_sampler_equals_the_sampler_on_the_penalized_copy(V):
    x, top = _logits(V, 13 * V + 1)
    keep = x.clone()
    changed = 0
    for name, prompt, plen, gen, ngen in _histories(x, top):
        for numbers in NUMBERS:
            pen = _pen(prompt, plen, gen, ngen, **numbers)
            y = _copy(x, pen)
            changed += int(not torch.equal(y.view(torch.int16), x.view(torch.int16)))
            for i, mode in enumerate(MODES):
                u = THS._rand(B, V + 17 * i)
                _same(_sample(x, u, mode, penalty=pen), _sample(y, u, mode), (V, name, numbers, mode))
    assert changed >= 2 * 8                                                     # every history but the empty one rewrites something
    assert_same_bits(x, keep, "the logits are read only")


def test_penalty_moves_the_argmax_and_the_kept_set():
    """the comparison above is not between two calls that ignore the history: the penalised token differs from the plain one"""
    V = 2049
    x = THS._logits(B, V, 1.0, 5)
    best = x.float().argmax(dim=1)
    pen = _pen(gen=best.view(B, 1).contiguous(), repetition=1.0, presence=50.0, frequency=0.0)
    tok, n = _sample(x, None, dict(T=0.0), penalty=pen)
    assert (tok != best).all() and torch.equal(tok, _S().penalize_reference(x, None, None, best.view(B, 1), None, 1.0, 50.0, 0.0).float().argmax(dim=1))


# =================================================================================================== 2. nothing beyond the counts is read
@pytest.mark.parametrize("V", [2049, 65536])
def test_entries_behind_the_counts_are_not_read(V):
    x = THS._logits(B, V, 2.0, 3 * V)
    top = x.float().topk(5, dim=1).indices
    g = torch.Generator(device=DEV).manual_seed(V)
    np_, ng = [4, 0, 33], [0, 65, 2]
    prompt, gen = torch.randint(0, V, (B, 40), device=DEV, generator=g), torch.randint(0, V, (B, 70), device=DEV, generator=g)
    seen_p, seen_g = prompt.clone(), gen.clone()
    for b in range(B):                                                          # behind the counts: the row's largest logits / nothing at all
        prompt[b, np_[b]:] = top[b, torch.arange(40 - np_[b], device=DEV) % 5]
        gen[b, ng[b]:] = top[b, torch.arange(70 - ng[b], device=DEV) % 5]
        seen_p[b, np_[b]:], seen_g[b, ng[b]:] = -1, -1
    fp, hp = fenced(prompt, poison="mark")
    fg, hg = fenced(gen, poison="mark")
    out, ho = fenced((B,), I64)
    numbers = dict(repetition=1.5, presence=2.0, frequency=0.5)
    per_row = _pen(fp, torch.tensor(np_, dtype=I32, device=DEV), fg, torch.tensor(ng, dtype=I32, device=DEV), **numbers)
    whole = _copy(x, _pen(prompt, None, gen, None, **numbers))                  # a call that read the tails would see this row instead
    assert not torch.equal(whole.view(torch.int16), _copy(x, per_row, seen_p, seen_g).view(torch.int16))
    for mode in MODES:
        u = THS._rand(B, V + 1)
        want = _sample(_copy(x, per_row, seen_p, seen_g), u, mode)
        _same(_sample(x, u, mode, penalty=per_row), want, (V, mode, "per-row counts"))
        _ops().sample_logits(x, u, mode.get("T", 1.0), mode.get("k"), mode.get("p"), out=out, penalty=per_row)
        assert torch.equal(out, want[0])
    # the host counts: every row's first 3 / first 2 entries
    prompt[:, 3:], gen[:, 2:] = top[:, :1], top[:, 1:2]
    seen_p, seen_g = prompt.clone(), gen.clone()
    seen_p[:, 3:], seen_g[:, 2:] = -1, -1
    host = _pen(prompt, 3, gen, 2, **numbers)
    for mode in MODES:
        u = THS._rand(B, V + 2)
        _same(_sample(x, u, mode, penalty=host), _sample(_copy(x, host, seen_p, seen_g), u, mode), (V, mode, "host counts"))
    assert_guards(hp, hg, ho)


# =================================================================================================== 3. the count's whole range
def test_a_token_repeated_32767_times():
    V = 16385
    x = THS._logits(B, V, 2.0, 99)
    t = x.float().argmax(dim=1)
    gen = t.view(B, 1).expand(B, 32767).contiguous()
    gen[1, 30000:] = (t[1] + 1) % V                                             # row 1: 30000 of one, 2767 of its neighbour
    pen = _pen(None, None, gen, None, repetition=1.0, presence=0.0, frequency=2.0 ** -12)
    for mode in MODES:
        u = THS._rand(B, 7)
        _same(_sample(x, u, mode, penalty=pen), _sample(_copy(x, pen), u, mode), mode)
    y = _S().penalize_reference(x, None, None, gen, None, 1.0, 0.0, 2.0 ** -12)
    assert float(y[0, t[0]]) == float((x[0, t[0]].float() - 32767 * 2.0 ** -12).to(BF))   # 32767 2^-12 is exact in fp32
    with pytest.raises(ValueError, match="32767"):
        _sample(x, None, MODES[0], penalty=_pen(gen=torch.zeros((B, 32768), dtype=I64, device=DEV), frequency=1.0))


# =================================================================================================== 4. together with the restriction
@pytest.mark.parametrize("V", [250, 16385])
def test_mask_and_held_token_apply_to_the_penalized_row(V):
    x, top = _logits(V, V + 4)
    allowed = torch.rand((B, V), device=DEV, generator=torch.Generator(device=DEV).manual_seed(V)) < 0.5
    allowed[torch.arange(B, device=DEV).view(B, 1), top[:, :6]] = True
    hold = int(top[0, 0])
    emitted = torch.tensor([0, 2, 3], dtype=I32, device=DEV)
    pen = _pen(top[:, 4:].contiguous(), None, top[:, :5].repeat(1, 3), torch.tensor([15, 4, 9], dtype=I32, device=DEV), **NUMBERS[0])
    y = _copy(x, pen)
    for con in (dict(allowed=allowed), dict(hold_token=hold, emitted=emitted, min_emitted=3), dict(allowed=allowed, hold_token=hold, emitted=emitted, min_emitted=3),
                dict(allowed_packed=_ops().pack_token_mask(allowed[1]))):
        for mode in MODES:
            u = THS._rand(B, V + 3)
            _same(_sample(x, u, mode, penalty=pen, **con), _sample(y, u, mode, **con), (V, mode, sorted(con)))


# =================================================================================================== 5. neutral, independent, repeatable
def test_neutral_numbers_give_the_unpenalized_bits():
    for V in (5, 2049, 65536):
        x, top = _logits(V, V + 8)
        lists = dict(prompt=top.contiguous(), gen=top.repeat(1, 4))
        for mode in MODES:
            u = THS._rand(B, V)
            plain = _sample(x, u, mode)
            _same(_sample(x, u, mode, penalty=_pen(**lists)), plain, (V, mode, "1, 0, 0"))
            _same(_sample(x, u, mode, penalty=_pen(**lists, repetition=1.0, presence=-0.0, frequency=0.0)), plain, (V, mode, "-0"))
            _same(_sample(x, u, mode, penalty=_pen(None, None, None, None, **NUMBERS[0])), plain, (V, mode, "no lists"))
            _same(_sample(x, u, mode, penalty=_pen(top.contiguous(), 0, top.contiguous(), 0, **NUMBERS[0])), plain, (V, mode, "two empty lists"))
            # the penalised kernel itself on lists that hold nothing inside [0, V)
            outside = torch.full((B, 9), V, dtype=I64, device=DEV)
            _same(_sample(x, u, mode, penalty=_pen(outside, None, outside - V - 1, None, **NUMBERS[0])), plain, (V, mode, "ids outside"))
            _same(_sample(x, u, mode, penalty=_pen(outside, torch.zeros(B, dtype=I32, device=DEV), None, None, **NUMBERS[0])), plain, (V, mode, "counts 0"))


@pytest.mark.parametrize("V", [2048, 16385, 65536])
def test_rows_are_independent_and_calls_repeat(V):
    x, top = _logits(V, V + 21)
    _, prompt, plen, gen, ngen = _histories(x, top)[6]                          # per-row counts
    pen = _pen(prompt, plen, gen, ngen, **NUMBERS[0])
    con = dict(hold_token=int(top[1, 0]), emitted=torch.tensor([0, 0, 9], dtype=I32, device=DEV), min_emitted=2)
    for mode in MODES:
        u = THS._rand(B, V + 5)
        all_rows = _sample(x, u, mode, penalty=pen, **con)
        _same(_sample(x, u, mode, penalty=pen, **con), all_rows, (V, mode, "twice"))
        for b in range(B):
            alone = _pen(prompt[b:b + 1].contiguous(), plen[b:b + 1].contiguous(), gen[b:b + 1].contiguous(), ngen[b:b + 1].contiguous(), **NUMBERS[0])
            one = _sample(THS._in_ld(x[b:b + 1]), u[b:b + 1].contiguous(), mode, penalty=alone, hold_token=con["hold_token"],
                          emitted=con["emitted"][b:b + 1].contiguous(), min_emitted=2)
            _same(one, tuple(t[b:b + 1] for t in all_rows), (V, mode, "row", b))


def test_wrapper_checks_on_the_device():
    x = THS._logits(B, 64, 1.0, 1)
    ids = torch.zeros((B, 4), dtype=I64, device=DEV)
    for bad, word in ((_pen(ids[:2], frequency=1.0), "prompt"), (_pen(gen=ids.int(), frequency=1.0), "dtype"), (_pen(gen=ids, n_gen=5, frequency=1.0), "count"),
                      (_pen(gen=ids, n_gen=torch.zeros(B, dtype=I64, device=DEV), frequency=1.0), "dtype"), (_pen(gen=ids.t()[:B, :3], frequency=1.0), "stride"),
                      (_pen(n_gen=2, frequency=1.0), "None"), (_pen(gen=ids, repetition=0.0), "repetition"), (_pen(gen=ids, presence=INF), "finite"),
                      (_pen(gen=ids, frequency=1e39), "finite")):
        with pytest.raises((ValueError, RuntimeError), match=word):
            _sample(x, None, MODES[0], penalty=bad)
    with pytest.raises(TypeError):
        _sample(x, None, MODES[0], penalty=dict(gen=ids))


# =================================================================================================== 6. the model
NEW, T0 = 16, 12
LENS = [12, 8]
SET = dict(temperature=0.9, top_k=50, top_p=0.95)
PEN = dict(repetition_penalty=1.3, frequency_penalty=0.2)


def _case():
    c = _gen_case(128)
    return c["m"], c["ids"][:, :T0].to(DEV)


def _by_hand(m, idx, lens, draw):
    """decode_step + penalize_reference + ``draw(logits, i)``, token for token: (B, NEW) int64"""
    from omnibiote_amd.model import KVCache
    b = idx.shape[0]
    cache = KVCache(m, b, T0 + NEW)
    logits = m.prefill(idx, cache) if lens is None else m.prefill(idx, cache, lengths=lens)
    gen = torch.zeros((b, NEW), dtype=I64, device=DEV)
    plen = None if lens is None else torch.tensor(lens, dtype=I32, device=DEV)
    for i in range(NEW):
        y = _S().penalize_reference(logits, idx, plen, gen, i, PEN["repetition_penalty"], 0.0, PEN["frequency_penalty"])
        gen[:, i] = draw(y, i)
        if i + 1 < NEW:
            logits = m.decode_step(gen[:, i].contiguous(), cache)
    return gen


@pytest.mark.parametrize("ragged", [False, True])
def test_generate_with_the_device_sampler_is_the_hand_written_loop(ragged):
    m, idx = _case()
    lens = LENS if ragged else None
    us = torch.rand((NEW, idx.shape[0]), device=DEV, generator=torch.Generator(device=DEV).manual_seed(3))
    want = _by_hand(m, idx, lens, lambda y, i: _ops().sample_logits(y, us[i], SET["temperature"], SET["top_k"], SET["top_p"]))
    kw = dict(sampler="device", generator=torch.Generator(device=DEV).manual_seed(3), **SET, **PEN)
    if ragged:
        out, out_lens = m.generate(idx, NEW, lengths=lens, **kw)
        assert out_lens.tolist() == [n + NEW for n in lens]
        got = torch.stack([out[b, n:n + NEW] for b, n in enumerate(lens)])
    else:
        got = m.generate(idx, NEW, **kw)[:, T0:]
    assert torch.equal(got, want), (got.tolist(), want.tolist())
    plain = m.generate(idx, NEW, lengths=lens, **{**kw, **dict(repetition_penalty=1.0, frequency_penalty=0.0, generator=torch.Generator(device=DEV).manual_seed(3))})
    plain = plain[0] if ragged else plain
    assert plain.shape[1] == (max(LENS) if ragged else T0) + NEW                # neutral numbers: the call as it was


def test_generate_with_the_torch_sampler_draws_from_the_penalized_logits():
    from omnibiote_amd.model import sample_next
    m, idx = _case()
    g = torch.Generator(device=DEV).manual_seed(9)
    want = _by_hand(m, idx, None, lambda y, i: sample_next(y, SET["temperature"], SET["top_k"], g, SET["top_p"]))
    got = m.generate(idx, NEW, sampler="torch", generator=torch.Generator(device=DEV).manual_seed(9), **SET, **PEN)[:, T0:]
    assert torch.equal(got, want), (got.tolist(), want.tolist())


@pytest.mark.parametrize("ragged", [False, True])
def test_device_loop_and_captured_graph_agree_bit_for_bit(ragged):
    m, idx = _case()
    kw = dict(sampler="device", **SET, **PEN, presence_penalty=0.1)
    if ragged:
        kw["lengths"] = LENS
    outs = [m.generate(idx, NEW, loop=loop, generator=torch.Generator(device=DEV).manual_seed(4), **kw) for loop in ("device", "graph")]
    a, b = (o[0] if ragged else o for o in outs)
    assert torch.equal(a, b), (a.tolist(), b.tolist())


def test_a_presence_penalty_above_every_logit_walks_through_the_allowed_ids():
    m, idx = _case()
    ids = [17, 3, 400, 511, 64, 65, 250, 8]
    base = dict(allowed_tokens=ids, presence_penalty=1e4, temperature=0.0)
    paths = [dict(sampler="device"), dict(sampler="torch"), dict(sampler="device", lengths=LENS), dict(sampler="torch", lengths=LENS),
             dict(sampler="device", kv_dtype="fp8"), dict(sampler="device", loop="device"), dict(sampler="device", loop="graph"),
             dict(sampler="device", loop="graph", lengths=LENS), dict(sampler="device", num_samples=2), dict(sampler="torch", num_samples=2),
             dict(sampler="device", weights=m.quantize_weights())]
    for path in paths:
        res = m.generate(idx, 8, **base, **path)
        out = res[0] if "lengths" in path else res
        lens = path["lengths"] if "lengths" in path else [T0] * out.shape[0]
        assert out.shape[0] == idx.shape[0] * path.get("num_samples", 1)
        for b, n in enumerate(lens):
            assert sorted(out[b, n:n + 8].tolist()) == sorted(ids), (path, b, out[b, n:n + 8].tolist())
    free = m.generate(idx, 8, allowed_tokens=ids, temperature=0.0, sampler="device")[:, T0:]
    assert any(len(set(r)) < 8 for r in free.tolist())                          # without the penalty the greedy rows repeat themselves


def test_decode_loop_keeps_its_penalty_across_a_second_prefill():
    from omnibiote_amd.model import DecodeLoop, KVCache, TokenPenalty
    m, idx = _case()
    cache = KVCache(m, idx.shape[0], T0 + NEW)
    logits = m.prefill(idx, cache)
    pen = TokenPenalty.of("test", 1.3, 0.0, 0.2, NEW).bind(idx, None, own_buffer=False)
    loop = DecodeLoop(m, cache, max_steps=NEW, capture=True, penalty=pen)       # greedy
    runs = []
    for prompt in (idx, idx.flip(1).contiguous(), idx):
        if runs:
            logits = loop.prefill(prompt)
        loop.start(logits)
        loop.run(NEW - 1)
        runs.append(loop.result()[0])
    assert torch.equal(runs[0], runs[2]) and not torch.equal(runs[0], runs[1])
    want = m.generate(idx, NEW, temperature=0.0, sampler="device", loop="device", **PEN)[:, T0:]
    assert torch.equal(runs[0], want)
    with pytest.raises(ValueError, match="TokenPenalty"):
        DecodeLoop(m, cache, max_steps=NEW, penalty=TokenPenalty.of("test", 1.3, 0.0, 0.2, NEW))      # not bound
