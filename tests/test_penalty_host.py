"""Host-side tests (no GPU) of penalised generation: the symbol table of the penalised entry point against its companion header, every
argument check that returns before a launch, the rule's plain-torch statement (sampling.penalize_reference) against hand-computed cases
and against the same formulas in float64, the validation of TokenPenalty / generate / ops.sample_logits, and the routing of neutral
penalties to the entry points the call took before, on a stub of the library's function table."""
import ctypes as C
import inspect
import math
import os
import re

import pytest
import torch

from omnibiote_amd import _lib
from omnibiote_amd.sampling import penalize_reference, penalty_numbers

EINVAL, EUNSUPPORTED = -1, -3
P = 4096   # a non-null, 16-byte aligned "pointer" for calls that must return before they touch it
NAME = "obte_sample_logits_penalized_bf16"
INF, NAN = float("inf"), float("nan")
BF, I32, I64 = torch.bfloat16, torch.int32, torch.int64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _err():
    return _lib.lib().obte_last_error().decode()


def _header():
    return open(os.path.join(ROOT, "include", "omnibiote_hip_penalty.h")).read()


def test_penalty_symbol_has_its_own_table_and_header():
    lib = _lib.lib()
    assert tuple(_lib.SYMBOLS_PENALTY) == (NAME,)
    header = _header()
    assert tuple(re.findall(r"^(?:int|int64_t|void|const char\*) +(obte_[a-z0-9_]+)\(", header, flags=re.M)) == (NAME,)
    assert len(re.findall(r"^[a-z0-9_\* ]+\bobte_[a-z0-9_]+\(", header, flags=re.M)) == 1
    assert '#include "omnibiote_hip.h"' in header and not re.search(r"\bstruct\b", header)
    others = (_lib.SYMBOLS, _lib.SYMBOLS_ROWS, _lib.SYMBOLS_SMALL_M, _lib.SYMBOLS_SAMPLE, _lib.SYMBOLS_EXTEND, _lib.SYMBOLS_SPEC, _lib.SYMBOLS_KV8,
              _lib.SYMBOLS_SHARED, _lib.SYMBOLS_LOOP, _lib.SYMBOLS_CONSTRAIN, _lib.SYMBOLS_W8, _lib.SYMBOLS_SCORE, _lib.SYMBOLS_FILL)
    assert [len(t) for t in others] == [70, 3, 3, 1, 6, 2, 6, 5, 1, 2, 2, 3, 4] and all(NAME not in t for t in others)   # the other tables as they were
    res, args = _lib.SYMBOLS_PENALTY[NAME]
    fn = getattr(lib, NAME)
    assert fn.restype is res and list(fn.argtypes) == args                                                               # bound by lib()
    makefile = open(os.path.join(ROOT, "omnibiote_amd", "csrc", "Makefile")).read()
    assert "../../include/omnibiote_hip_penalty.h" in re.search(r"^HDRS\s*=(.*)$", makefile, flags=re.M).group(1)
    assert lib.obte_abi_version() == 1 and lib.obte_struct_sizes((C.c_int64 * 16)(), 16) == 6


def test_argtypes_are_the_constrained_ones_with_the_thirteen_arguments_inserted():
    new = [C.c_void_p, C.c_int64, C.c_void_p, C.c_int32,                     # prompt, prompt_ld, prompt_len, prompt_max
           C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int32,          # gen, gen_ld, n_gen, n_gen_all, gen_max
           C.c_float, C.c_float, C.c_float, C.c_float]                       # repetition, inv_repetition, presence, frequency
    res, args = _lib.SYMBOLS_CONSTRAIN["obte_sample_logits_constrained_bf16"]
    assert _lib.SYMBOLS_PENALTY[NAME] == (res, args[:13] + new + args[13:])  # before token
    proto = re.search(NAME + r"\((.*?)\);", _header(), flags=re.S).group(1)
    names = [a.split()[-1].lstrip("*") for a in proto.replace("\n", " ").split(",")]
    assert names[13:26] == ["prompt", "prompt_ld", "prompt_len", "prompt_max", "gen", "gen_ld", "n_gen", "n_gen_all", "gen_max", "repetition",
                            "inv_repetition", "presence", "frequency"] and names[-3:] == ["token", "n_kept", "s"] and len(names) == len(args) + 13


# ----------------------------------------------------------------------------------------------- OBTE_EINVAL before any launch
def _call(logits=P, ld=1008, B=2, V=1003, u=P, temperature=1.0, top_k=0, top_p=1.0, allowed=P, allowed_ld=126, hold_token=3, emitted=P, min_emitted=2,
          prompt=P, prompt_ld=40, prompt_len=P, prompt_max=40, gen=P, gen_ld=64, n_gen=P, n_gen_all=0, gen_max=64, repetition=1.25, inv_repetition=0.8,
          presence=0.5, frequency=0.25, token=P, n_kept=P):
    return _lib.lib().obte_sample_logits_penalized_bf16(logits, ld, B, V, u, temperature, top_k, top_p, allowed, allowed_ld, hold_token, emitted, min_emitted,
                                                        prompt, prompt_ld, prompt_len, prompt_max, gen, gen_ld, n_gen, n_gen_all, gen_max, repetition,
                                                        inv_repetition, presence, frequency, token, n_kept, None)


@pytest.mark.parametrize("kw,rc,word", [
    # whatever the constrained function rejects
    (dict(logits=None), EINVAL, "null"), (dict(token=None), EINVAL, "null"), (dict(logits=P + 8), EINVAL, "logits must be 16-byte"),
    (dict(ld=1004), EINVAL, "ld"), (dict(ld=1000), EINVAL, "ld"), (dict(B=0), EINVAL, "B"), (dict(V=0, ld=8, allowed_ld=0), EINVAL, "V"),
    (dict(temperature=-0.5), EINVAL, "temperature"), (dict(temperature=NAN), EINVAL, "temperature"), (dict(top_p=0.0), EINVAL, "top_p"),
    (dict(u=P + 2), EINVAL, "u must be 4-byte"), (dict(n_kept=P + 2), EINVAL, "n_kept must be 4-byte"), (dict(token=P + 4), EINVAL, "token must be 8-byte"),
    (dict(V=65537, ld=65544, allowed_ld=0), EUNSUPPORTED, "65537"), (dict(allowed_ld=-1), EINVAL, "allowed_ld"), (dict(allowed_ld=125), EINVAL, "allowed_ld"),
    (dict(emitted=P + 2), EINVAL, "emitted must be 4-byte"), (dict(min_emitted=-1), EINVAL, "min_emitted"),
    # the bounds
    (dict(gen_max=32768, gen_ld=40000), EINVAL, "32767"), (dict(gen_max=65, gen_ld=64), EINVAL, "gen_ld"), (dict(gen_max=-1), EINVAL, "negative"),
    (dict(prompt_max=41), EINVAL, "prompt_ld"), (dict(prompt_max=2 ** 24, prompt_ld=2 ** 25), EINVAL, "2^24"), (dict(prompt_max=-1), EINVAL, "negative"),
    (dict(gen_max=1, gen_ld=0), EINVAL, "gen_ld"), (dict(gen_ld=-64), EINVAL, "gen_ld"),
    # the pointers
    (dict(prompt=None), EINVAL, "null pointer (prompt)"), (dict(gen=None), EINVAL, "null pointer (gen)"),
    (dict(prompt=P + 4), EINVAL, "prompt must be 8-byte"), (dict(gen=P + 4), EINVAL, "gen must be 8-byte"),
    (dict(prompt_len=P + 2), EINVAL, "prompt_len must be 4-byte"), (dict(n_gen=P + 1), EINVAL, "n_gen must be 4-byte"),
    # the numbers
    (dict(repetition=0.0), EINVAL, "repetition must be positive"), (dict(repetition=-1.5), EINVAL, "repetition must be positive"),
    (dict(repetition=INF), EINVAL, "finite"), (dict(repetition=NAN), EINVAL, "finite"), (dict(inv_repetition=INF), EINVAL, "finite"),
    (dict(presence=NAN), EINVAL, "finite"), (dict(presence=-INF), EINVAL, "finite"), (dict(frequency=INF), EINVAL, "finite"),
])
def test_penalized_sampler_rejects_before_any_launch(kw, rc, word):
    assert _call(**kw) == rc
    assert _err().startswith(NAME + ":") and word in _err(), _err()


def test_the_other_samplers_still_answer_in_their_own_name():
    lib = _lib.lib()
    assert lib.obte_sample_logits_bf16(None, 8, 1, 8, None, 1.0, 0, 1.0, P, None, None) == EINVAL and _err().startswith("obte_sample_logits_bf16:")
    assert lib.obte_sample_logits_constrained_bf16(None, 8, 1, 8, None, 1.0, 0, 1.0, None, 0, -1, None, 0, P, None, None) == EINVAL
    assert _err().startswith("obte_sample_logits_constrained_bf16:")


# ----------------------------------------------------------------------------------------------- the rule in plain torch
def _bf(v):
    return float(torch.tensor(v, dtype=torch.float32).to(BF))


def _f32(v):
    return float(torch.tensor(v, dtype=torch.float32))


def test_penalize_reference_on_hand_computed_cases():
    V = 12
    #         0     1     2    3     4     5     6    7     8     9    10   11
    row = [2.0, -1.5, 0.0, 3.0, -INF, INF, NAN, 0.75, -2.5, 1.25, 4.0, -0.0]
    x = torch.tensor([row, row], dtype=BF)
    prompt = torch.tensor([[0, 1, 2, 0, 0, -1, V, 2 ** 40, 4, 6], [3, 3, 3, 3, 3, 3, 3, 3, 3, 3]])
    gen = torch.tensor([[7, 7, 7, 8, 1, 5, -1, V, 2 ** 40, 9, 9], [10] * 11])
    r, pp, fp = 1.5, 0.25, 0.5
    inv = _f32(1.0 / 1.5)
    y = penalize_reference(x, prompt, None, gen, torch.tensor([9, 4]), r, pp, fp)
    assert y.dtype == BF and y.shape == x.shape and x[0, 0] == 2.0                          # a copy
    want0 = {0: _bf(_f32(2.0 * inv)),                                      # positive, prompt only (three times over: once)
             1: _bf(_f32(_f32(-1.5 * r) - _f32(pp + _f32(fp * 1.0)))),     # negative, in both lists, generated once
             2: 0.0,                                                       # zero, prompt only: 0 * inv
             7: _bf(_f32(_f32(0.75 * inv) - _f32(pp + _f32(fp * 3.0)))),   # generated only, three times
             8: _bf(_f32(_f32(-2.5 * r) - _f32(pp + fp))),
             9: 1.25}                                                      # behind n_gen = 9: gen[0, 9:] is not read
    for col, v in want0.items():
        assert float(y[0, col]) == v, (col, float(y[0, col]), v)
    assert float(y[0, 4]) == -INF and float(y[0, 5]) == INF and math.isnan(float(y[0, 6]))   # -inf and NaN stay, +inf / r - finite is +inf
    for col in (3, 10, 11):                                                                   # in no list: the bits stay (-0 included)
        assert y[0, col].view(torch.int16) == x[0, col].view(torch.int16)
    assert float(y[1, 3]) == _bf(_f32(3.0 * inv)) and float(y[1, 10]) == _bf(_f32(_f32(4.0 * inv) - _f32(pp + _f32(fp * 4.0))))   # counts clipped by n_gen = 4
    rest = [c for c in range(V) if c not in (3, 10)]
    assert torch.equal(y[1, rest].view(torch.int16), x[1, rest].view(torch.int16))
    # +inf with an infinite-looking difference follows IEEE; -inf stays -inf under every penalty
    z = penalize_reference(torch.tensor([INF, -INF, NAN], dtype=BF), None, None, torch.tensor([0, 1, 2, 0]), None, 0.5, -3.0, 100.0)
    assert float(z[0]) == INF and float(z[1]) == -INF and math.isnan(float(z[2]))
    # one row in, one row out; counts as numbers; None lists; a float32 input is rounded to bf16 first
    assert torch.equal(penalize_reference(x[0], prompt[0], None, gen[0], 9, r, pp, fp).view(torch.int16), y[0].view(torch.int16))
    assert torch.equal(penalize_reference(x, None, None, None, None, r, pp, fp).view(torch.int16), x.view(torch.int16))
    assert torch.equal(penalize_reference(x, prompt, 0, gen, 0, r, pp, fp).view(torch.int16), x.view(torch.int16))
    assert penalize_reference(torch.tensor([[1.00390625, 2.0]]), torch.tensor([[1]]), None, None, None, 2.0)[0].tolist() == [1.0, 1.0]
    # neutral numbers change nothing, whatever the lists hold
    assert torch.equal(penalize_reference(x, prompt, None, gen, None, 1.0, 0.0, 0.0).view(torch.int16)[:, [c for c in range(V) if c != 6]],
                       x.view(torch.int16)[:, [c for c in range(V) if c != 6]])
    for bad in (dict(repetition=0.0), dict(repetition=-1.0), dict(presence=INF), dict(frequency=NAN), dict(repetition=1e-40)):
        with pytest.raises(ValueError):
            penalize_reference(x, prompt, None, gen, None, **bad)
    with pytest.raises(ValueError, match="gen"):
        penalize_reference(x, prompt, None, gen[:1].repeat(3, 1), None, 2.0)
    with pytest.raises(ValueError, match="prompt"):
        penalize_reference(x, prompt.float(), None, gen, None, 2.0)


def test_penalty_numbers_are_fp32_and_the_reciprocal_comes_from_float64():
    r, inv, pp, fp = penalty_numbers(1.3, 0.1, 0.2)
    assert (r, pp, fp) == (_f32(1.3), _f32(0.1), _f32(0.2)) and inv == _f32(1.0 / _f32(1.3)) and penalty_numbers() == (1.0, 1.0, 0.0, 0.0)
    assert penalty_numbers(3)[1] == _f32(1.0 / 3.0)


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_penalize_reference_agrees_with_the_formulas_in_float64(seed):
    """within one bf16 rounding of the float64 value: |y - y64| <= ulp_bf16(y64) / 2 + the fp32 operations' error, which is below 2^-16 of
    the bf16 step — so y is one of the two bf16 neighbours of y64, or y64's own rounding: |y - y64| <= one bf16 step of |y64|"""
    g = torch.Generator().manual_seed(seed)
    Bn, V = 4, 300
    x = (torch.randn(Bn, V, generator=g) * 3).to(BF)
    prompt = torch.randint(-5, V + 5, (Bn, 50), generator=g)
    gen = torch.randint(-5, V + 5, (Bn, 400), generator=g) // 3                # many duplicates
    plen, ngen = torch.tensor([0, 50, 17, 33]), torch.tensor([400, 0, 123, 9])
    r, pp, fp = [(1.3, 0.5, 0.25), (0.8, -0.3, 0.01), (2.5, 0.0, 1.0)][seed]
    y = penalize_reference(x, prompt, plen, gen, ngen, r, pp, fp).double()
    r32, inv, pp32, fp32 = penalty_numbers(r, pp, fp)
    w = x.double()
    for b in range(Bn):
        ctx = {int(t) for t in prompt[b, :int(plen[b])].tolist() + gen[b, :int(ngen[b])].tolist() if 0 <= t < V}
        cnt = {}
        for t in gen[b, :int(ngen[b])].tolist():
            cnt[t] = cnt.get(t, 0) + 1
        for i in range(V):
            if i not in ctx:
                assert float(y[b, i]) == float(w[b, i])
                continue
            v = float(w[b, i])
            v = v * r32 if v < 0 else v / r32
            if cnt.get(i, 0) > 0:
                v = v - (pp32 + fp32 * cnt[i])
            step = 2.0 ** (math.floor(math.log2(abs(v))) - 7) if v != 0 else 0.0   # the bf16 step at v: 8 bits of significand
            assert abs(float(y[b, i]) - v) <= step, (b, i, float(y[b, i]), v)


# ----------------------------------------------------------------------------------------------- TokenPenalty and generate's checks
def _model(vocab=64, block=32):
    from omnibiote_amd.model import OmniBioTA, OmniBioTAConfig
    c = OmniBioTAConfig()
    c.block_size, c.vocab_size, c.n_layer, c.n_head, c.n_embd, c.dropout, c.flash = block, vocab, 1, 2, 128, 0.0, True
    c.autoregressive = True
    return OmniBioTA(c)


BAD = [(dict(repetition_penalty=0.0), "repetition_penalty"), (dict(repetition_penalty=-2.0), "repetition_penalty"), (dict(repetition_penalty=INF), "finite"),
       (dict(repetition_penalty=NAN), "finite"), (dict(presence_penalty=INF), "finite"), (dict(frequency_penalty=NAN), "finite"),
       (dict(frequency_penalty=1e39), "finite"), (dict(presence_penalty="1"), "must be a number"), (dict(repetition_penalty=None), "must be a number"),
       (dict(frequency_penalty=True), "must be a number"), (dict(repetition_penalty=1e-40), "repetition_penalty")]


@pytest.mark.parametrize("kw,word", BAD)
def test_generate_validates_the_penalties_before_any_device_work(kw, word):
    m = _model()
    idx = torch.zeros(2, 8, dtype=I64)
    for extra in (dict(), dict(sampler="device"), dict(lengths=[8, 5]), dict(sampler="device", loop="graph"), dict(kv_dtype="fp8"), dict(num_samples=2)):
        with pytest.raises(ValueError, match=word):
            m.generate(idx, 4, **extra, **kw)


def test_generate_refuses_more_new_tokens_than_a_count_holds():
    m = _model(block=40000)
    idx = torch.zeros(1, 8, dtype=I64)
    with pytest.raises(ValueError, match="32767"):
        m.generate(idx, 32768, frequency_penalty=0.5)
    from omnibiote_amd.model import TokenPenalty
    assert TokenPenalty.of("t", 1.0, 0.0, 0.0, 10 ** 6) is None and TokenPenalty.of("t", 1.0, 0.0, 0.5, 32767).max_new == 32767


def test_valid_penalties_reach_the_device_code_and_neutral_ones_change_nothing():
    m = _model()
    idx = torch.zeros(2, 8, dtype=I64)
    for kw in (dict(repetition_penalty=1.3), dict(presence_penalty=-0.5, lengths=[8, 5]), dict(frequency_penalty=0.2, num_samples=2),
               dict(repetition_penalty=2, sampler="device", loop="graph")):
        with pytest.raises(RuntimeError):
            m.generate(idx, 4, **kw)
    assert torch.equal(m.generate(idx, 0, repetition_penalty=1.3), idx)


def test_signatures_take_the_new_keywords_where_the_issue_puts_them():
    from omnibiote_amd.model import DecodeLoop, OmniBioTA
    gen = list(inspect.signature(OmniBioTA.generate).parameters)
    at = gen.index("loop")
    assert gen[at + 1:at + 4] == ["repetition_penalty", "presence_penalty", "frequency_penalty"] and gen[-3:] == ["allowed_tokens", "min_new_tokens", "weights"]
    p = inspect.signature(OmniBioTA.generate).parameters
    assert (p["repetition_penalty"].default, p["presence_penalty"].default, p["frequency_penalty"].default) == (1.0, 0.0, 0.0)
    sig = inspect.signature(DecodeLoop.__init__).parameters
    assert list(sig)[-4:] == ["penalty", "weights", "allowed", "hold_min"] and sig["penalty"].kind is sig["penalty"].KEYWORD_ONLY and sig["penalty"].default is None
    for f in (OmniBioTA.generate_speculative, OmniBioTA.draft_and_verify):                   # out of scope: no such keywords
        assert not any("penalty" in name for name in inspect.signature(f).parameters)


def test_token_penalty_binds_records_and_hands_out_the_arguments():
    from omnibiote_amd import ops
    from omnibiote_amd.model import TokenPenalty
    pen = TokenPenalty.of("generate", 1.5, 0.25, 0.5, 6)
    prompt = torch.tensor([[3, 4, 5, 3], [7, 7, 0, 0]])
    assert pen.bind(prompt, [4, 2]) is pen
    assert pen.prompt is not prompt and torch.equal(pen.prompt, prompt) and pen.prompt_len.tolist() == [4, 2] and pen.prompt_len.dtype == I32
    assert pen.gen.shape == (2, 6) and pen.gen.dtype == I64
    pen.record(0, torch.tensor([9, 7]))
    pen.record(1, torch.tensor([9, 1]))
    a = pen.device_args(2)
    assert isinstance(a, ops.Penalty) and a.gen is pen.gen and a.n_gen == 2 and a.prompt is pen.prompt and a.prompt_len is pen.prompt_len
    assert (a.repetition, a.presence, a.frequency) == (1.5, 0.25, 0.5)
    x = torch.ones(2, 12, dtype=BF)
    y = pen.apply(x, 2)
    want = penalize_reference(x, prompt, [4, 2], torch.tensor([[9, 9], [7, 1]]), None, 1.5, 0.25, 0.5)
    assert torch.equal(y, want) and float(y[0, 9]) == _bf(_f32(1.0 / 1.5) - 1.25) and float(y[1, 0]) == 1.0 and float(y[1, 7]) == _bf(_f32(1.0 / 1.5) - 0.75)
    assert torch.equal(pen.apply(x, 0), penalize_reference(x, prompt, [4, 2], None, None, 1.5))
    out, n_new = torch.zeros(2, 6, dtype=I64), torch.zeros(2, dtype=I32)
    la = pen.loop_args(out, n_new)
    assert la.gen is out and la.n_gen is n_new and la.prompt is pen.prompt
    keep = pen.prompt
    pen.rebind(torch.tensor([[1, 2], [3, 4]]))
    assert pen.prompt is keep and pen.prompt[:, :2].tolist() == [[1, 2], [3, 4]] and pen.prompt_len.tolist() == [2, 2]
    with pytest.raises(ValueError, match="rebind"):
        pen.rebind(torch.zeros(2, 5, dtype=I64))
    assert TokenPenalty.of("generate", 1.3, 0.0, 0.0, 4).bind(prompt, None, own_buffer=False).gen is None


# ----------------------------------------------------------------------------------------------- ops.sample_logits on a stub of the library
class _Stub:
    """the library's function table: every entry point records its name and arguments and returns OBTE_OK"""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        if not name.startswith("obte_"):
            raise AttributeError(name)
        return lambda *a: (self.calls.append((name, a)), 0)[1]


@pytest.fixture
def stub(monkeypatch):
    from omnibiote_amd import ops
    s = _Stub()
    monkeypatch.setattr(ops.L, "lib", lambda: s)
    monkeypatch.setattr(ops, "_stream", lambda: 0)
    real = ops._need

    def need(t, name, dtype=ops.bf16, contiguous=True):                                      # the wrapper's checks but the device's
        if isinstance(t, torch.Tensor) and not t.is_cuda:
            if dtype is not None and t.dtype != dtype:
                raise RuntimeError(f"{name}: expected dtype {dtype}, got {t.dtype}")
            return
        real(t, name, dtype, contiguous)
    monkeypatch.setattr(ops, "_need", need)
    return s


def test_neutral_penalties_take_the_entry_point_the_call_took_before(stub):
    from omnibiote_amd import ops
    x = torch.zeros(3, 64, dtype=BF)
    ids = torch.zeros((3, 5), dtype=I64)
    mask = torch.ones(8, dtype=torch.uint8)
    neutral = [None, ops.Penalty(), ops.Penalty(ids, None, ids, None), ops.Penalty(ids, None, ids, 2, 1.0, -0.0, 0.0), ops.Penalty(None, None, None, None, 1.3, 0.5, 0.1),
               ops.Penalty(ids, 0, ids, 0, 1.3, 0.5, 0.1), ops.Penalty(ids[:, :0], None, None, None, 2.0)]
    for pen in neutral:
        stub.calls.clear()
        ops.sample_logits(x, penalty=pen)
        ops.sample_logits(x, penalty=pen, allowed_packed=mask)
        assert [c[0] for c in stub.calls] == ["obte_sample_logits_bf16", "obte_sample_logits_constrained_bf16"], pen
        assert len(stub.calls[0][1]) == 11 and len(stub.calls[1][1]) == 16                  # and their arguments as they were
    stub.calls.clear()
    n = torch.tensor([1, 2, 3], dtype=I32)
    ops.sample_logits(x, penalty=ops.Penalty(ids, n, ids[:, :4], 3, 1.3, 0.5, 0.25), hold_token=7, min_emitted=2)
    ops.sample_logits(x, penalty=ops.Penalty(None, None, ids, n, 2.0))
    assert [c[0] for c in stub.calls] == [NAME, NAME]
    a = stub.calls[0][1]
    assert len(a) == 29 and a[8:13] == (None, 0, 7, None, 2)
    assert a[13:26] == (ids.data_ptr(), 5, n.data_ptr(), 5, ids.data_ptr(), 5, None, 3, 3) + penalty_numbers(1.3, 0.5, 0.25)
    b = stub.calls[1][1]
    assert b[8:13] == (None, 0, -1, None, 0) and b[13:22] == (None, 0, None, 0, ids.data_ptr(), 5, n.data_ptr(), 0, 5) and b[22:26] == (2.0, 0.5, 0.0, 0.0)


def test_spec_verify_takes_the_constrained_entry_point_only_when_a_restriction_is_given(stub):
    """what lets the speculative loop pass an empty keyword dict for a call that restricts nothing"""
    from omnibiote_amd import ops
    p, x = torch.zeros((3, 3, 64), dtype=BF), torch.zeros((3, 2), dtype=I64)

    def verified(**kw):                                                                      # (the workspace query is a call of the table too)
        stub.calls.clear()
        ops.spec_verify(p, None, x, **kw)
        return [(name, len(args)) for name, args in stub.calls if name != "obte_spec_verify_ws_bytes"]
    assert verified() == [("obte_spec_verify_bf16", 18)]
    assert verified(allowed=None, allowed_packed=None, hold_token=None, emitted=None, min_emitted=0) == [("obte_spec_verify_bf16", 18)]
    for kw in (dict(allowed=torch.ones(64, dtype=torch.bool)), dict(allowed_packed=torch.ones(8, dtype=torch.uint8)), dict(hold_token=7),
               dict(emitted=torch.zeros(3, dtype=I32)), dict(min_emitted=2)):
        assert verified(**kw) == [("obte_spec_verify_constrained_bf16", 23)], kw


def test_sample_logits_validates_the_penalty(stub):
    from omnibiote_amd import ops
    x = torch.zeros(3, 64, dtype=BF)
    ids = torch.zeros((3, 5), dtype=I64)
    bad = [(ops.Penalty(ids[:2], frequency=1.0), ValueError, "prompt"), (ops.Penalty(gen=ids.int(), frequency=1.0), RuntimeError, "dtype"),
           (ops.Penalty(gen=ids, n_gen=6, frequency=1.0), ValueError, "count"), (ops.Penalty(gen=ids, n_gen=-1, frequency=1.0), ValueError, "count"),
           (ops.Penalty(gen=ids, n_gen=True, frequency=1.0), ValueError, "count"), (ops.Penalty(gen=ids, n_gen=torch.zeros(3, dtype=I64), frequency=1.0), RuntimeError, "dtype"),
           (ops.Penalty(gen=ids, n_gen=torch.zeros(2, dtype=I32), frequency=1.0), ValueError, "count"), (ops.Penalty(gen=ids.t()[:3, :3], frequency=1.0), ValueError, "stride"),
           (ops.Penalty(n_gen=2, frequency=1.0), ValueError, "None"), (ops.Penalty(prompt_len=2, frequency=1.0), ValueError, "None"),
           (ops.Penalty(gen=ids, repetition=0.0), ValueError, "repetition"), (ops.Penalty(gen=ids, presence=INF), ValueError, "finite"),
           (ops.Penalty(gen=torch.zeros((3, 32768), dtype=I64), frequency=1.0), ValueError, "32767"),
           (ops.Penalty(gen=ids.view(15)[:5].view(1, 5).expand(3, 5), frequency=1.0), ValueError, "apart"), (dict(gen=ids), TypeError, "ops.Penalty")]
    for pen, exc, word in bad:
        with pytest.raises(exc, match=word):
            ops.sample_logits(x, penalty=pen)
    assert stub.calls == []                                                                  # nothing was launched
    ops.sample_logits(x, penalty=ops.Penalty(gen=torch.zeros((3, 32768), dtype=I64), n_gen=32767, frequency=1.0))   # the host count is the bound
    ops.sample_logits(x, penalty=ops.Penalty(gen=torch.zeros((3, 32767), dtype=I64), n_gen=torch.zeros(3, dtype=I32), frequency=1.0))
    assert [c[0] for c in stub.calls] == [NAME, NAME] and stub.calls[0][1][19:22] == (None, 32767, 32767)


def test_ops_refuse_cpu_tensors():
    from omnibiote_amd import ops
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.sample_logits(torch.zeros(2, 16, dtype=BF), penalty=ops.Penalty(gen=torch.zeros((2, 3), dtype=I64), frequency=1.0))
