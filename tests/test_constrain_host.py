"""Host-side tests (no GPU) of constrained generation: the symbol table of the two constrained entry points against their companion
header, every argument check that returns before a launch, the mask helpers and the rule's plain-torch statement
(sampling.constrain_reference), the validation of generate / generate_speculative / DecodeLoop, and the device loop's use of the
restriction on a CPU stub (sampling.advance_reference, as tests/test_loop_host.py drives it)."""
import ctypes as C
import os
import re

import pytest
import torch

from omnibiote_amd import _lib
from omnibiote_amd.sampling import advance_reference, constrain_reference, pack_token_mask, sample_reference, unpack_token_mask

EINVAL, EUNSUPPORTED = -1, -3
P = 4096   # a non-null, 16-byte aligned "pointer" for calls that must return before they touch it
NAMES = ("obte_sample_logits_constrained_bf16", "obte_spec_verify_constrained_bf16")
INF, NAN = float("inf"), float("nan")
I32 = torch.int32


def _err():
    return _lib.lib().obte_last_error().decode()


def _header():
    return open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "omnibiote_hip_constrain.h")).read()


def test_constrain_symbols_have_their_own_table():
    lib = _lib.lib()
    assert tuple(_lib.SYMBOLS_CONSTRAIN) == NAMES
    header = _header()
    assert tuple(re.findall(r"^(?:int|int64_t|void|const char\*) +(obte_[a-z0-9_]+)\(", header, flags=re.M)) == NAMES   # in the header's order
    assert len(re.findall(r"^[a-z0-9_\* ]+\bobte_[a-z0-9_]+\(", header, flags=re.M)) == len(NAMES)                       # and nothing else
    assert '#include "omnibiote_hip.h"' in header and not re.search(r"\bstruct\b", header)
    others = (_lib.SYMBOLS, _lib.SYMBOLS_ROWS, _lib.SYMBOLS_SMALL_M, _lib.SYMBOLS_SAMPLE, _lib.SYMBOLS_EXTEND, _lib.SYMBOLS_SPEC, _lib.SYMBOLS_KV8,
              _lib.SYMBOLS_SHARED, _lib.SYMBOLS_LOOP)
    for name in NAMES:
        for table in others:
            assert name not in table
        fn = getattr(lib, name)
        res, args = _lib.SYMBOLS_CONSTRAIN[name]
        assert fn.restype is res and list(fn.argtypes) == args                                                             # bound by lib()
    assert [len(t) for t in others[:8]] == [70, 3, 3, 1, 6, 2, 6, 5] and tuple(_lib.SYMBOLS_LOOP) == ("obte_gen_advance",)
    assert lib.obte_abi_version() == 1
    sizes = (C.c_int64 * 16)()
    assert lib.obte_struct_sizes(sizes, 16) == 6


def test_argtypes_are_the_unrestricted_ones_with_the_five_arguments_inserted():
    five = [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_int32]                # allowed, allowed_ld, hold_token, emitted, min_emitted
    res, args = _lib.SYMBOLS_SAMPLE["obte_sample_logits_bf16"]
    assert _lib.SYMBOLS_CONSTRAIN[NAMES[0]] == (res, args[:8] + five + args[8:])    # before token
    res, args = _lib.SYMBOLS_SPEC["obte_spec_verify_bf16"]
    assert _lib.SYMBOLS_CONSTRAIN[NAMES[1]] == (res, args[:13] + five + args[13:])  # before n_accept


# ----------------------------------------------------------------------------------------------- OBTE_EINVAL before any launch
def _sample(logits=P, ld=1008, B=2, V=1003, u=P, temperature=1.0, top_k=0, top_p=1.0, allowed=P, allowed_ld=126, hold_token=3, emitted=P, min_emitted=2,
            token=P, n_kept=P):
    return _lib.lib().obte_sample_logits_constrained_bf16(logits, ld, B, V, u, temperature, top_k, top_p, allowed, allowed_ld, hold_token, emitted,
                                                          min_emitted, token, n_kept, None)


def _verify(p=P, ld_p=1008, q=P, ld_q=1008, draft=P, B=2, k=4, V=1003, u_accept=P, u_draw=P, temperature=1.0, top_k=0, top_p=1.0, allowed=P, allowed_ld=126,
            hold_token=3, emitted=P, min_emitted=2, n_accept=P, token=P, ws=P, ws_bytes=1 << 20):
    return _lib.lib().obte_spec_verify_constrained_bf16(p, ld_p, q, ld_q, draft, B, k, V, u_accept, u_draw, temperature, top_k, top_p, allowed, allowed_ld,
                                                        hold_token, emitted, min_emitted, n_accept, token, ws, ws_bytes, None)


NEW = [(dict(allowed_ld=-1), EINVAL, "allowed_ld"), (dict(allowed_ld=125), EINVAL, "allowed_ld"), (dict(allowed_ld=1), EINVAL, "allowed_ld"),
       (dict(emitted=P + 2), EINVAL, "emitted must be 4-byte"), (dict(emitted=P + 1), EINVAL, "emitted must be 4-byte"),
       (dict(min_emitted=-1), EINVAL, "min_emitted"), (dict(min_emitted=-2 ** 31), EINVAL, "min_emitted"),
       (dict(allowed=None, allowed_ld=-8), EINVAL, "allowed_ld")]


@pytest.mark.parametrize("kw,rc,word", NEW + [
    (dict(logits=None), EINVAL, "null"), (dict(token=None), EINVAL, "null"), (dict(logits=P + 8), EINVAL, "logits must be 16-byte"),
    (dict(ld=1004), EINVAL, "ld"), (dict(ld=1000), EINVAL, "ld"), (dict(B=0), EINVAL, "B"), (dict(V=0, ld=8, allowed_ld=0), EINVAL, "V"),
    (dict(temperature=-0.5), EINVAL, "temperature"), (dict(temperature=NAN), EINVAL, "temperature"), (dict(top_p=0.0), EINVAL, "top_p"),
    (dict(top_p=NAN), EINVAL, "top_p"), (dict(u=P + 2), EINVAL, "u must be 4-byte"), (dict(n_kept=P + 2), EINVAL, "n_kept must be 4-byte"),
    (dict(token=P + 4), EINVAL, "token must be 8-byte"), (dict(V=65537, ld=65544, allowed_ld=0), EUNSUPPORTED, "65537"),
])
def test_constrained_sampler_rejects_before_any_launch(kw, rc, word):
    assert _sample(**kw) == rc
    assert _err().startswith("obte_sample_logits_constrained_bf16:") and word in _err(), _err()


@pytest.mark.parametrize("kw,rc,word", NEW + [
    (dict(p=None), EINVAL, "null"), (dict(draft=None), EINVAL, "null"), (dict(n_accept=None), EINVAL, "null"), (dict(ws=None), EINVAL, "null"),
    (dict(q=None), EINVAL, "null pointer (q)"), (dict(p=P + 8), EINVAL, "p must be 16-byte"), (dict(q=P + 2), EINVAL, "q must be 16-byte"),
    (dict(ld_p=1004), EINVAL, "ld_p"), (dict(ld_q=1000), EINVAL, "ld_q"), (dict(B=0), EINVAL, "B"), (dict(k=0), EINVAL, "k"),
    (dict(temperature=INF), EINVAL, "temperature"), (dict(top_p=1.0001), EINVAL, "top_p"), (dict(u_accept=P + 2), EINVAL, "u_accept must be 4-byte"),
    (dict(u_draw=P + 1), EINVAL, "u_draw must be 4-byte"), (dict(n_accept=P + 2), EINVAL, "n_accept must be 4-byte"),
    (dict(token=P + 4), EINVAL, "token must be 8-byte"), (dict(draft=P + 4), EINVAL, "draft must be 8-byte"), (dict(ws=P + 4), EINVAL, "ws must be 8-byte"),
    (dict(ws_bytes=2 * 9 * 32 - 1), EINVAL, "workspace"), (dict(k=32), EUNSUPPORTED, "k = 32"),
    (dict(V=65537, ld_p=65544, ld_q=65544, allowed_ld=0), EUNSUPPORTED, "65537"),
])
def test_constrained_verification_rejects_before_any_launch(kw, rc, word):
    assert _verify(**kw) == rc
    assert _err().startswith("obte_spec_verify_constrained_bf16:") and word in _err(), _err()


def test_the_unrestricted_entry_points_still_answer_in_their_own_name():
    lib = _lib.lib()
    assert lib.obte_sample_logits_bf16(None, 8, 1, 8, None, 1.0, 0, 1.0, P, None, None) == EINVAL and _err().startswith("obte_sample_logits_bf16:")
    assert lib.obte_spec_verify_bf16(None, 8, P, 8, P, 1, 1, 8, P, P, 1.0, 0, 1.0, P, P, P, 1 << 10, None) == EINVAL
    assert _err().startswith("obte_spec_verify_bf16:")


def test_ops_refuse_cpu_tensors():
    from omnibiote_amd import ops
    x = torch.zeros(2, 16, dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.sample_logits(x, allowed=torch.ones(16, dtype=torch.bool))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.pack_token_mask(torch.ones(16, dtype=torch.bool))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.spec_verify(torch.zeros(2, 3, 16, dtype=torch.bfloat16), None, torch.zeros(2, 2, dtype=torch.int64), hold_token=1, min_emitted=1)


# ----------------------------------------------------------------------------------------------- masks and the rule in plain torch
@pytest.mark.parametrize("V", [5, 8, 9, 250, 65536])
def test_pack_token_mask_round_trips(V):
    g = torch.Generator().manual_seed(V)
    for shape in ((V,), (3, V), (2, 2, V)):
        m = torch.rand(shape, generator=g) < 0.5
        m[..., V - 1] = True
        packed = pack_token_mask(m)
        assert packed.dtype == torch.uint8 and packed.shape == shape[:-1] + ((V + 7) // 8,)
        assert torch.equal(unpack_token_mask(packed, V), m)
        flat, pf = m.reshape(-1, V), packed.reshape(-1, packed.shape[-1])
        for i in (0, 1, V // 2, V - 1):                                          # the layout: bit i & 7 of byte i >> 3
            assert torch.equal((pf[:, i >> 3] >> (i & 7)) & 1, flat[:, i].to(torch.uint8))
        if V % 8:
            assert int(pf[:, -1].max()) < (1 << (V % 8))                         # the padding bits are clear
    wide = torch.cat([packed, torch.full_like(packed, 255)], dim=-1)             # more bytes than needed, bits set beyond V: ignored
    assert torch.equal(unpack_token_mask(wide, V), m)
    if V % 8:
        dirty = packed.clone()
        dirty[..., -1] |= 0xFF & ~((1 << (V % 8)) - 1)
        assert torch.equal(unpack_token_mask(dirty, V), m)
    for bad in (torch.zeros(V), torch.zeros(0, dtype=torch.bool)):
        with pytest.raises(ValueError, match="pack_token_mask"):
            pack_token_mask(bad)
    with pytest.raises(ValueError, match="unpack_token_mask"):
        unpack_token_mask(torch.zeros((V + 7) // 8 - 1 if V > 8 else 0, dtype=torch.uint8), V)


def test_constrain_reference_excludes_exactly_the_stated_columns():
    B, V = 3, 21
    x = torch.randn(B, V, generator=torch.Generator().manual_seed(1)).to(torch.bfloat16)
    assert torch.equal(constrain_reference(x), x)
    one = torch.rand(V, generator=torch.Generator().manual_seed(2)) < 0.5
    rows = torch.rand(B, V, generator=torch.Generator().manual_seed(3)) < 0.5
    for allowed in (one, rows):
        y = constrain_reference(x, allowed)
        a = allowed.expand(B, V)
        assert y.dtype == x.dtype and torch.equal(y[a], x[a]) and bool(torch.isneginf(y[~a].float()).all())
    assert torch.equal(constrain_reference(x[1], rows[1]), constrain_reference(x, rows)[1])           # one row in, one row out
    # what reaches the kernels is the packed mask: bits of columns >= V mean nothing
    dirty = pack_token_mask(rows)
    dirty[:, -1] |= 0xE0
    assert torch.equal(constrain_reference(x, unpack_token_mask(dirty, V)), constrain_reference(x, rows))
    for bad in (torch.ones(V + 1, dtype=torch.bool), torch.ones(B + 1, V, dtype=torch.bool), torch.ones(V)):
        with pytest.raises(ValueError, match="constrain_reference"):
            constrain_reference(x, bad)
    with pytest.raises(ValueError, match="min_emitted"):
        constrain_reference(x, None, 2, None, -1)


def test_constrain_reference_holds_the_token_iff_emitted_plus_offset_is_below_the_minimum():
    B, V, T = 4, 12, 5
    x = torch.zeros(B, V)
    emitted = torch.tensor([0, 2, 3, 7], dtype=I32)
    for offset in (0, 1, 2):
        y = constrain_reference(x, None, T, emitted, 3, offset)
        held = torch.isneginf(y[:, T])
        assert held.tolist() == [int(e) + offset < 3 for e in emitted.tolist()]
        y[:, T] = 0
        assert torch.equal(y, x)                                                 # and no other column
    assert torch.isneginf(constrain_reference(x, None, T, None, 1)[:, T]).all()  # emitted None: 0
    assert not torch.isneginf(constrain_reference(x, None, T, None, 0)).any()
    assert not torch.isneginf(constrain_reference(x, None, T, 5, 5)).any() and torch.isneginf(constrain_reference(x, None, T, 4, 5)[:, T]).all()
    for outside in (-1, V, 2 ** 40, None):                                       # holds nothing
        assert torch.equal(constrain_reference(x, None, outside, emitted, 3), x)
    big = torch.tensor([2 ** 31 - 1] * B, dtype=I32)                             # the sum cannot overflow
    assert torch.equal(constrain_reference(x, None, T, big, 2 ** 31 - 1, 31), x)
    # both at once, and the sampler's rule on the result: an excluded maximum is never the token
    allowed = torch.ones(V, dtype=torch.bool)
    allowed[[7, 8]] = False
    x2 = x.clone()
    x2[:, 7], x2[:, T] = 9.0, 8.0
    tok, kept, _ = sample_reference(constrain_reference(x2, allowed, T, emitted, 3), None)
    assert (tok == T).tolist() == [False, False, True, True] and (tok != 7).all()
    tok, kept, _ = sample_reference(constrain_reference(x2, torch.zeros(V, dtype=torch.bool)), 0.5)
    assert tok.tolist() == [0] * B and kept.tolist() == [0] * B                  # nothing left: token 0, nothing kept


# ----------------------------------------------------------------------------------------------- generate's checks
def _model(vocab=64, block=32):
    from omnibiote_amd.model import OmniBioTA, OmniBioTAConfig
    c = OmniBioTAConfig()
    c.block_size, c.vocab_size, c.n_layer, c.n_head, c.n_embd, c.dropout, c.flash = block, vocab, 1, 2, 128, 0.0, True
    c.autoregressive = True
    return OmniBioTA(c)


BAD = [
    (dict(allowed_tokens=[1, 2, 64]), "outside"), (dict(allowed_tokens=[-1, 2]), "outside"), (dict(allowed_tokens=torch.tensor([5, 70])), "outside"),
    (dict(allowed_tokens=[]), "allows nothing"), (dict(allowed_tokens=torch.zeros(64, dtype=torch.bool)), "allows nothing"),
    (dict(allowed_tokens=torch.eye(64, dtype=torch.bool)[:2] & (torch.arange(2).view(2, 1) == 0)), "allows nothing"),      # row 1 of 2 is empty
    (dict(allowed_tokens=torch.ones(63, dtype=torch.bool)), "allowed_tokens must be"), (dict(allowed_tokens=torch.ones(3, 64, dtype=torch.bool)), "one row per"),
    (dict(allowed_tokens=torch.ones(2, 2)), "allowed_tokens must be"), (dict(allowed_tokens=[[1, 2]]), "allowed_tokens must be"),
    (dict(min_new_tokens=-1, eos_token=3), "min_new_tokens"), (dict(min_new_tokens=5, eos_token=3), "min_new_tokens"),
    (dict(min_new_tokens=1.0, eos_token=3), "min_new_tokens"), (dict(min_new_tokens=2), "no eos_token"),
    (dict(min_new_tokens=2, eos_token=3, allowed_tokens=[3]), "nothing else"),
    (dict(min_new_tokens=1, eos_token=3, allowed_tokens=torch.eye(64, dtype=torch.bool)[[5, 3]]), "nothing else"),
]


@pytest.mark.parametrize("kw,word", BAD)
def test_generate_validates_the_restriction_before_any_device_work(kw, word):
    m = _model()
    idx = torch.zeros(2, 8, dtype=torch.int64)
    for extra in (dict(), dict(sampler="device"), dict(lengths=[8, 5]), dict(sampler="device", loop="graph"), dict(kv_dtype="fp8")):
        with pytest.raises(ValueError, match=word):
            m.generate(idx, 4, **extra, **kw)
    with pytest.raises(ValueError, match=word):
        m.generate_speculative(idx, 4, _model(), **kw)
    a = kw.get("allowed_tokens")
    if isinstance(a, torch.Tensor) and a.dtype == torch.bool and a.dim() == 2 and a.shape[0] == 2:
        with pytest.raises(ValueError, match="one row per"):                      # P * G = 4 output rows
            m.generate(idx, 4, num_samples=2, **kw)


def test_a_valid_restriction_reaches_the_device_code():
    """the checks pass and the call goes on to the device work, which a CPU model refuses; nothing to generate needs no device at all"""
    m = _model()
    idx = torch.zeros(2, 8, dtype=torch.int64)
    rows4 = torch.ones(4, 64, dtype=torch.bool)
    for kw in (dict(allowed_tokens=[1, 2, 3]), dict(allowed_tokens=torch.ones(2, 64, dtype=torch.bool), min_new_tokens=4, eos_token=3),
               dict(allowed_tokens=rows4, num_samples=2), dict(min_new_tokens=2, eos_token=99)):
        with pytest.raises(RuntimeError):
            m.generate(idx, 4, **kw)
    assert torch.equal(m.generate(idx, 0, allowed_tokens=[1, 2]), idx)
    assert torch.equal(m.generate_speculative(idx, 0, _model(), allowed_tokens=[1, 2], min_new_tokens=0), idx)


def test_token_constraint_packs_once_and_counts_down():
    from omnibiote_amd.model import TokenConstraint
    assert TokenConstraint.of("generate", None, 0, 8, None, 2, 64, "cpu") is None
    con = TokenConstraint.of("generate", [1, 5, 9], 3, 8, 5, 2, 64, "cpu")
    assert con.allowed.shape == (64,) and con.allowed.nonzero().flatten().tolist() == [1, 5, 9]
    assert torch.equal(con.packed, pack_token_mask(con.allowed)) and con.hold == 5 and con.min_new == 3
    assert [con.device_args(s)["min_emitted"] for s in range(5)] == [3, 2, 1, 0, 0]
    x = torch.zeros(2, 64)
    assert constrain_reference(x, con.allowed, 5, None, 1).isfinite().sum(dim=1).tolist() == [2, 2]
    assert con.restrict(x, 2).isfinite().nonzero()[:, 1].tolist() == [1, 9, 1, 9] and con.restrict(x, 3).isfinite().sum().item() == 6
    only_len = TokenConstraint.of("generate", None, 2, 8, 5, 2, 64, "cpu")
    assert only_len.allowed is None and only_len.packed is None and only_len.hold == 5
    only_mask = TokenConstraint.of("generate", torch.ones(2, 64, dtype=torch.bool), 0, 8, None, 2, 64, "cpu")
    assert only_mask.hold is None and only_mask.packed.shape == (2, 8)


def test_decode_loop_takes_the_restriction_as_its_last_keywords():
    import inspect
    from omnibiote_amd.model import DecodeLoop
    sig = inspect.signature(DecodeLoop.__init__).parameters
    assert sig["allowed"].default is None and sig["hold_min"].default == 0
    assert list(sig)[-2:] == ["allowed", "hold_min"]


# ----------------------------------------------------------------------------------------------- the device loop on a CPU stub
def test_no_eos_before_the_minimum_on_a_stub_of_the_loop():
    """DecodeLoop's step with the kernels replaced by their plain-torch statements: the sampler sees the mask, eos as the held token and
    the loop's own n_new as the rows' emitted counts (start: commit 0 on n_new = 0).  The logits favour eos heavily: without the hold
    every row ends at once."""
    B, V, EOS, STEPS, MIN = 4, 40, 7, 10, 6
    g = torch.Generator().manual_seed(5)
    allowed = torch.zeros(B, V, dtype=torch.bool)
    allowed[:, EOS] = True
    for b in range(B):
        allowed[b, 10 + 5 * b:15 + 5 * b] = True                                 # row b: its own five tokens, and eos
    wte, us = torch.randn(V, 8, generator=g), torch.rand(STEPS, B, generator=g)

    def run(hold_min):
        st = dict(pos=torch.tensor([9, 4, 6, 11], dtype=I32), count=torch.zeros(B, dtype=I32), out=torch.zeros(B, STEPS, dtype=torch.int64),
                  n_new=torch.zeros(B, dtype=I32), token=torch.zeros(B, dtype=torch.int64))
        gl = torch.Generator().manual_seed(6)
        u = us[0]
        for i in range(STEPS):
            logits = torch.randn(B, V, generator=gl)
            logits[:, EOS] += 12.0
            x = constrain_reference(logits, allowed, EOS if hold_min > 0 else None, st["n_new"], hold_min)
            sampled = sample_reference(x, u, 0.8)[0]
            st["pos"], st["count"], st["out"], st["n_new"], st["token"], _, u = advance_reference(
                sampled, st["pos"], st["count"], st["out"], st["n_new"], st["token"], wte, us, eos=EOS, commit=0 if i == 0 else 1)
        return st["out"], st["n_new"]

    out, n_new = run(0)
    assert n_new.tolist() == [1] * B and (out[:, 0] == EOS).all()                # the bias works: unconstrained rows end at once
    out, n_new = run(MIN)
    live = torch.arange(STEPS).view(1, -1) < n_new.view(-1, 1)
    assert (n_new >= MIN + 1).all() or (n_new == STEPS).all()
    assert not (out[:, :MIN] == EOS).any() and (n_new >= MIN).all()
    assert (out[:, MIN] == EOS).all() and n_new.tolist() == [MIN + 1] * B        # and it comes as soon as it may
    assert bool(allowed.gather(1, out)[live].all())                              # every token in its row's set
