"""Host-side tests (no GPU) of the device-resident generation loop (include/omnibiote_hip_loop.h): the symbol table against the header,
the argument checks that return before a launch, sampling.advance_reference against the bookkeeping of the eager generate loops for the
same token stream, CachePositions.advanced_on_device, and the validation of generate(loop=) on a CPU model."""
import ctypes as C
import os
import re

import pytest
import torch

from omnibiote_amd import _lib
from omnibiote_amd.model import CachePositions, ragged_output
from omnibiote_amd.sampling import advance_reference

EINVAL = -1
P = 4096   # a non-null, 16-byte aligned "pointer" for calls that must return before they touch it
NAMES = ("obte_gen_advance",)
I32 = torch.int32


def _err():
    return _lib.lib().obte_last_error().decode()


def test_symbols_are_what_the_header_declares():
    assert tuple(_lib.SYMBOLS_LOOP) == NAMES
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "omnibiote_hip_loop.h")).read()
    body = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    assert tuple(re.findall(r"\b(obte_\w+)\s*\(", body)) == NAMES                  # the declarations, in order
    assert '#include "omnibiote_hip.h"' in header and "struct" not in body
    lib = _lib.lib()
    others = (_lib.SYMBOLS, _lib.SYMBOLS_ROWS, _lib.SYMBOLS_SMALL_M, _lib.SYMBOLS_SAMPLE, _lib.SYMBOLS_EXTEND, _lib.SYMBOLS_SPEC, _lib.SYMBOLS_KV8,
              _lib.SYMBOLS_SHARED)
    for name in NAMES:
        for table in others:
            assert name not in table
        res, args = _lib.SYMBOLS_LOOP[name]
        fn = getattr(lib, name)                                                     # the library exports it
        assert fn.restype is res and list(fn.argtypes) == args                      # bound by lib(), in the same loop
    assert _lib.SYMBOLS_LOOP["obte_gen_advance"] == (C.c_int, [C.c_void_p] * 4 + [C.c_int64] + [C.c_void_p] * 3 + [C.c_int64, C.c_int32, C.c_void_p,
                                                               C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int32, C.c_int64, C.c_void_p])
    assert [len(t) for t in others] == [70, 3, 3, 1, 6, 2, 6, 5]                   # the other tables stay as they were
    assert lib.obte_abi_version() == 1
    sizes = (C.c_int64 * 16)()
    assert lib.obte_struct_sizes(sizes, 16) == 6                                    # no new struct


def _call(sampled=P, pos=P, count=P, out=P, out_ld=4, n_new=P, token=P, wte=P, vocab=10, cols=64, x=P, us=None, us_steps=0, u=None, eos=-1, commit=1, B=2):
    return _lib.lib().obte_gen_advance(sampled, pos, count, out, out_ld, n_new, token, wte, vocab, cols, x, us, us_steps, u, eos, commit, B, None)


@pytest.mark.parametrize("kw,word", [
    (dict(sampled=None), "null"), (dict(pos=None), "null"), (dict(count=None), "null"), (dict(out=None), "null"), (dict(n_new=None), "null"),
    (dict(token=None), "null"), (dict(wte=None), "null"), (dict(x=None), "null"), (dict(us=P, us_steps=3), "null"),
    (dict(wte=P + 8), "aligned"), (dict(x=P + 8), "aligned"), (dict(sampled=P + 4), "aligned"), (dict(out=P + 4), "aligned"),
    (dict(token=P + 4), "aligned"), (dict(pos=P + 2), "aligned"), (dict(count=P + 2), "aligned"), (dict(n_new=P + 2), "aligned"),
    (dict(us=P + 2, us_steps=3, u=P), "aligned"), (dict(us=P, us_steps=3, u=P + 2), "aligned"),
    (dict(cols=60), "cols"), (dict(cols=0), "cols"), (dict(cols=-8), "cols"), (dict(B=0), "B"), (dict(B=1 << 31), "B"),
    (dict(vocab=0), "vocab"), (dict(out_ld=0), "out_ld"), (dict(us=P, us_steps=0, u=P), "us_steps"),
])
def test_gen_advance_rejects_before_any_launch(kw, word):
    assert _call(**kw) == EINVAL
    assert _err().startswith("obte_gen_advance:") and word in _err(), _err()


# ------------------------------------------------------------------------------------------- the rule against the eager loops' bookkeeping
B, STEPS, EOS, VOCAB = 5, 12, 7, 40
LENS = [9, 4, 6, 4, 11]


def _stream(seed):
    """(STEPS, B) tokens in which EOS hits row 1 at step 0, row 3 at step 5 and row 0 at step 8; rows 2 and 4 never draw it"""
    g = torch.Generator().manual_seed(seed)
    t = torch.randint(8, VOCAB, (STEPS, B), generator=g)
    t[0, 1], t[5, 3], t[8, 0] = EOS, EOS, EOS
    t[9, 1] = EOS                                                                   # (behind row 1's end: never seen)
    return t


def _state(pos):
    g = torch.Generator().manual_seed(1)
    return dict(pos=torch.tensor(pos, dtype=I32), count=torch.zeros(B, dtype=I32), out=torch.zeros(B, STEPS, dtype=torch.int64),
                n_new=torch.zeros(B, dtype=I32), token=torch.zeros(B, dtype=torch.int64), wte=torch.randn(VOCAB, 8, generator=g),
                us=torch.rand(STEPS, B, generator=g))


def _advance(st, sampled, eos, commit):
    st["pos"], st["count"], st["out"], st["n_new"], st["token"], st["x"], st["u"] = advance_reference(
        sampled, st["pos"], st["count"], st["out"], st["n_new"], st["token"], st["wte"], st["us"], eos=eos, commit=commit)


def _result(st, steps_run, eos):
    """DecodeLoop.result's width rule on a reference state"""
    width = 1 + steps_run
    if eos is not None and not bool((st["pos"] >= 0).any()):
        width = int(st["n_new"].max())
    return st["out"][:, :width], st["n_new"]


@pytest.mark.parametrize("eos,n_steps", [(EOS, STEPS), (None, STEPS), (EOS, 4)])
def test_reference_reproduces_the_ragged_loop(eos, n_steps):
    stream = _stream(3)
    if n_steps == STEPS and eos is not None:
        stream[6, 2], stream[7, 4] = EOS, EOS                                       # every row finishes: the loop stops at step 8
    # the bookkeeping of generate's host loop behind ragged prompts, restated: tokens, valid, park, and decode_step's advance
    cache = CachePositions(B, 64)
    cache.reset(max(LENS), torch.tensor(LENS, dtype=I32), min(LENS))
    tokens, valid, done, seen = [], [], torch.zeros(B, dtype=torch.bool), {}
    for i in range(n_steps):
        nxt = stream[i]
        tokens.append(nxt)
        valid.append(~done)
        if eos is not None:
            done = done | (nxt == eos)
        if i + 1 == n_steps or (eos is not None and bool(done.all())):
            break
        if eos is not None:
            cache.park(done)
        seen[i] = cache.positions.clone()                                           # where token i's decode_step stores
        cache.advance(1)
    idx = torch.arange(B * max(LENS)).view(B, -1) % VOCAB
    want, want_len = ragged_output(idx, LENS, torch.stack(tokens, dim=1), torch.stack(valid, dim=1), 0)
    # the device loop: start is commit = 0 on token 0, every body commit = 1 on the next token
    st = _state(LENS)
    _advance(st, stream[0], eos, 0)
    for i in range(1, n_steps):
        assert torch.equal(st["pos"], seen[i - 1]) if i - 1 in seen else not bool((st["pos"] >= 0).any())
        assert torch.equal(st["u"], st["us"][i]) and torch.equal(st["x"], st["wte"][st["token"]])
        _advance(st, stream[i], eos, 1)
    assert st["count"].tolist() == [n_steps] * B
    toks, n_new = _result(st, n_steps - 1, eos)
    got, got_len = ragged_output(idx, LENS, toks, torch.arange(toks.shape[1]).view(1, -1) < n_new.view(-1, 1), 0)
    assert torch.equal(got, want) and torch.equal(got_len, want_len)
    assert toks.shape[1] == len(tokens)                                             # the same width as the eager loop's


@pytest.mark.parametrize("every_row_finishes", [False, True])
def test_reference_reproduces_the_uniform_loop(every_row_finishes):
    stream = _stream(4)
    if every_row_finishes:
        stream[6, 2], stream[7, 4] = EOS, EOS
    out, done = [], None                                                            # generate's bookkeeping, restated
    for i in range(STEPS):
        nxt = stream[i]
        if done is not None:
            nxt = torch.where(done, torch.full_like(nxt, EOS), nxt)
        done = (nxt == EOS) if done is None else (done | (nxt == EOS))
        out.append(nxt.unsqueeze(1))
        if i + 1 == STEPS or bool(done.all()):
            break
    want = torch.cat(out, dim=1)
    st = _state([6] * B)
    _advance(st, stream[0], EOS, 0)
    for i in range(1, STEPS):
        _advance(st, stream[i], EOS, 1)
    toks, n_new = _result(st, STEPS - 1, EOS)
    live = torch.arange(toks.shape[1]).view(1, -1) < n_new.view(-1, 1)
    assert torch.equal(torch.where(live, toks, torch.full_like(toks, EOS)), want)   # a finished row keeps producing EOS
    running = st["pos"] >= 0
    assert st["pos"][running].tolist() == [6 + STEPS - 1] * int(running.sum())      # one position per step behind the first token


def test_reference_edge_cases():
    st = _state([3, -1, 5, 0, 2])                                                   # row 1 is parked from the start
    before = {k: v.clone() for k, v in st.items()}
    sampled = torch.tensor([9, 9, EOS, -5, VOCAB + 7])
    _advance(st, sampled, EOS, 0)
    assert st["pos"].tolist() == [3, -1, -1, 0, 2]                                  # commit = 0: nobody moves; row 2 drew EOS
    assert st["n_new"].tolist() == [1, 0, 1, 1, 1] and st["count"].tolist() == [1] * B
    assert st["token"].tolist() == [9, 0, EOS, -5, VOCAB + 7]                       # tokens are stored as drawn ...
    assert torch.equal(st["x"], st["wte"][torch.tensor([9, 0, EOS, 0, VOCAB - 1])])  # ... and clamped where they index the table
    assert st["out"][:, 0].tolist() == [9, 0, EOS, -5, VOCAB + 7] and not st["out"][:, 1:].any()
    assert torch.equal(st["u"], st["us"][1])
    assert torch.equal(before["pos"], torch.tensor([3, -1, 5, 0, 2], dtype=I32))    # nothing is changed in place
    _advance(st, sampled, EOS, 1)
    assert st["pos"].tolist() == [4, -1, -1, 1, 3] and st["n_new"].tolist() == [2, 0, 1, 2, 2]
    assert st["out"][1].tolist() == [0] * STEPS and st["out"][2].tolist() == [EOS] + [0] * (STEPS - 1)
    # count >= out_ld: the row runs on, unrecorded; a negative count records nothing either; the uniforms' row is clamped both ways
    st["count"] = torch.tensor([STEPS, STEPS + 5, STEPS - 1, -3, 2 ** 31 - 1], dtype=I32)
    st["pos"] = torch.tensor([4, 7, 7, 1, 3], dtype=I32)
    was_out, was_n = st["out"].clone(), st["n_new"].clone()
    _advance(st, torch.tensor([11, 12, 13, 14, 15]), EOS, 1)
    assert st["pos"].tolist() == [5, 8, 8, 2, 4]
    assert (st["n_new"] - was_n).tolist() == [0, 0, 1, 0, 0] and st["out"][2, STEPS - 1] == 13
    was_out[2, STEPS - 1] = 13
    assert torch.equal(st["out"], was_out)
    assert st["count"].tolist() == [STEPS + 1, STEPS + 6, STEPS, -2, -2 ** 31]
    assert st["u"].tolist() == [st["us"][STEPS - 1, 0].item(), st["us"][STEPS - 1, 1].item(), st["us"][STEPS - 1, 2].item(), st["us"][0, 3].item(),
                                st["us"][STEPS - 1, 4].item()]
    # no uniforms: u is None; eos None or negative: nobody is parked
    r = advance_reference(torch.tensor([EOS] * B), st["pos"], torch.zeros(B, dtype=I32), st["out"], st["n_new"], st["token"], st["wte"], None, eos=None)
    assert r[6] is None and r[0].tolist() == [6, 9, 9, 3, 5]
    assert advance_reference(torch.tensor([EOS] * B), st["pos"], torch.zeros(B, dtype=I32), st["out"], st["n_new"], st["token"], st["wte"], eos=-1)[0].tolist() == [6, 9, 9, 3, 5]
    with pytest.raises(ValueError, match="commit"):
        advance_reference(sampled, st["pos"], st["count"], st["out"], st["n_new"], st["token"], st["wte"], commit=2)


def test_advanced_on_device_moves_the_host_bounds_alone():
    c = CachePositions(3, 32)
    with pytest.raises(ValueError, match="uniform"):
        c.advanced_on_device(1)
    at = torch.tensor([4, -1, 7], dtype=I32)
    c.reset(7, at, 4)
    c.advanced_on_device(1)
    assert (c.pos, c.min_pos) == (8, 5) and c.positions is at and at.tolist() == [4, -1, 7]
    c.advanced_on_device(3)
    assert (c.pos, c.min_pos) == (11, 8) and c.positions is at and c.max_pos == 11
    c.advance(1)                                                                    # the eager writer still makes a new tensor
    assert c.positions is not at and c.positions.tolist() == [5, -1, 8] and c.pos == 12


def _cpu_model():
    from omnibiote_amd.model import OmniBioTA, OmniBioTAConfig
    c = OmniBioTAConfig()
    c.block_size, c.vocab_size, c.n_layer, c.n_head, c.n_embd, c.dropout, c.flash = 32, 64, 1, 2, 128, 0.0, True
    c.autoregressive = True
    return OmniBioTA(c)


def test_generate_loop_argument_errors():
    m = _cpu_model()
    idx = torch.zeros(2, 4, dtype=torch.int64)
    for bad in ("eager", "host", True, 1):
        with pytest.raises(ValueError, match="loop"):
            m.generate(idx, 4, sampler="device", loop=bad)
    for loop in ("device", "graph"):
        with pytest.raises(ValueError, match="sampler"):
            m.generate(idx, 4, loop=loop)                                           # the default sampler is torch's
        with pytest.raises(ValueError, match="sampler"):
            m.generate(idx, 4, sampler="torch", loop=loop, lengths=[4, 3])
        with pytest.raises(ValueError, match="num_samples"):
            m.generate(idx, 4, sampler="device", loop=loop, num_samples=3)
        assert torch.equal(m.generate(idx, 0, sampler="device", loop=loop), idx)    # nothing to draw
        with pytest.raises(RuntimeError, match="GPU"):                              # valid arguments go on to the first device-side requirement
            m.generate(idx, 4, sampler="device", loop=loop)
    with pytest.raises(RuntimeError, match="GPU"):
        m.generate(idx, 4, sampler="device", loop=None)


def test_decode_loop_refuses_a_shared_prefix_cache():
    from omnibiote_amd.model import DecodeLoop, SharedPrefixCache
    c = SharedPrefixCache.__new__(SharedPrefixCache)
    CachePositions.__init__(c, 6, 13)
    with pytest.raises(ValueError, match="SharedPrefixCache"):
        DecodeLoop(_cpu_model(), c, max_steps=4)
