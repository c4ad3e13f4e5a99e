"""Host-side tests (no GPU) of speculative decoding without a draft model (include/omnibiote_hip_lookup.h): the symbol table against the
companion header, every argument check of obte_lookup_draft and obte_spec_verify_point_bf16 that returns before a launch, the lookup
rule's plain loop (sampling.lookup_reference) on hand-written rows, sampling.verify_point_reference against verify_reference on the
one-hot q it stands for, and the validation of lookup_and_verify and generate_lookup."""
import ctypes as C
import os
import re

import pytest
import torch

from omnibiote_amd import _lib

EINVAL, EUNSUPPORTED = -1, -3
P = 4096   # a non-null, 16-byte aligned "pointer" for calls that must return before they touch it
NAMES = ("obte_lookup_draft", "obte_spec_verify_point_ws_bytes", "obte_spec_verify_point_bf16")
BF = torch.bfloat16
INF, NAN = float("inf"), float("nan")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _err():
    return _lib.lib().obte_last_error().decode()


def test_lookup_symbols_are_what_the_header_declares():
    assert tuple(_lib.SYMBOLS_LOOKUP) == NAMES
    header = open(os.path.join(ROOT, "include", "omnibiote_hip_lookup.h")).read()
    body = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    assert tuple(re.findall(r"\b(obte_\w+)\s*\(", body)) == NAMES                  # the declarations, in order
    assert '#include "omnibiote_hip.h"' in header and "struct" not in body
    assert "OBTE_LOOKUP_MAX_HISTORY 8192" in body and _lib.LOOKUP_MAX_HISTORY == 8192 and _lib.LOOKUP_MAX_NGRAM == 16
    lib = _lib.lib()
    for name in NAMES:
        for table in (getattr(_lib, t) for t in dir(_lib) if t.startswith("SYMBOLS") and t != "SYMBOLS_LOOKUP"):
            assert name not in table
        res, args = _lib.SYMBOLS_LOOKUP[name]
        fn = getattr(lib, name)
        assert fn.restype is res and list(fn.argtypes) == args                      # bound by lib(), in the same loop
    res, args = _lib.SYMBOLS_SPEC["obte_spec_verify_bf16"]
    assert _lib.SYMBOLS_LOOKUP["obte_spec_verify_point_bf16"] == (res, args[:2] + args[4:])       # obte_spec_verify_bf16 without q and ld_q
    assert _lib.SYMBOLS_LOOKUP["obte_spec_verify_point_ws_bytes"] == _lib.SYMBOLS_SPEC["obte_spec_verify_ws_bytes"]
    assert len(_lib.SYMBOLS_SPEC) == 2 and len(_lib.SYMBOLS) == 70                  # the tables beside it as they were
    assert lib.obte_abi_version() == 1
    sizes = (C.c_int64 * 16)()
    assert lib.obte_struct_sizes(sizes, 16) == 6                                    # no new struct
    makefile = open(os.path.join(ROOT, "omnibiote_amd", "csrc", "Makefile")).read()
    assert "omnibiote_hip_lookup.h" in makefile and "lookup_draft.hip" in makefile
    assert "kind 122" in header and "kind 123" in header                            # the launch profiler's kinds, stated where they are taken


def test_point_workspace_is_one_summary_per_target_row():
    ws = _lib.lib().obte_spec_verify_point_ws_bytes
    assert ws(1, 1) == 2 * 32 and ws(8, 4) == 8 * 5 * 32 and ws(64, 31) == 64 * 32 * 32
    assert ws(0, 4) == 0 and ws(2, 0) == 0 and ws(2, 32) == 0


# ------------------------------------------------------------------------------------------------------- the C checks
def _lookup(hist=P, hist_ld=64, lens=P, B=2, k=4, g_min=1, g_max=4, V=512, draft=P, match_len=P):
    return _lib.lib().obte_lookup_draft(hist, hist_ld, lens, B, k, g_min, g_max, V, draft, match_len, None)


@pytest.mark.parametrize("kw,rc,word", [
    (dict(hist=None), EINVAL, "null"), (dict(lens=None), EINVAL, "null"), (dict(draft=None), EINVAL, "null"), (dict(match_len=None), EINVAL, "null"),
    (dict(B=0), EINVAL, "B"), (dict(B=-2), EINVAL, "B"), (dict(B=1 << 24), EINVAL, "B"), (dict(hist_ld=0), EINVAL, "hist_ld"), (dict(k=0), EINVAL, "k"),
    (dict(k=-1), EINVAL, "k"), (dict(hist_ld=8193), EUNSUPPORTED, "8193"), (dict(hist_ld=1 << 40), EUNSUPPORTED, "hist_ld"),
    (dict(k=32), EUNSUPPORTED, "k = 32"), (dict(g_min=0), EINVAL, "g_min"), (dict(g_min=5), EINVAL, "g_min"), (dict(g_max=17), EINVAL, "g_max"),
    (dict(g_min=-1, g_max=-1), EINVAL, "g_min"), (dict(V=0), EINVAL, "V"), (dict(V=65537), EINVAL, "V"), (dict(V=-4), EINVAL, "V"),
    (dict(hist=P + 4), EINVAL, "hist must be 8-byte"), (dict(draft=P + 4), EINVAL, "draft must be 8-byte"), (dict(lens=P + 2), EINVAL, "lens must be 4-byte"),
    (dict(match_len=P + 1), EINVAL, "match_len must be 4-byte"),
])
def test_lookup_draft_rejects_before_any_launch(kw, rc, word):
    assert _lookup(**kw) == rc
    assert _err().startswith("obte_lookup_draft:") and word in _err(), _err()


def _point(p=P, ld_p=1008, draft=P, B=2, k=4, V=1003, u_accept=P, u_draw=P, temperature=1.0, top_k=0, top_p=1.0, n_accept=P, token=P, ws=P,
           ws_bytes=1 << 20):
    return _lib.lib().obte_spec_verify_point_bf16(p, ld_p, draft, B, k, V, u_accept, u_draw, temperature, top_k, top_p, n_accept, token, ws, ws_bytes, None)


@pytest.mark.parametrize("kw,rc,word", [
    (dict(p=None), EINVAL, "null"), (dict(draft=None), EINVAL, "null"), (dict(n_accept=None), EINVAL, "null"), (dict(token=None), EINVAL, "null"),
    (dict(ws=None), EINVAL, "null"), (dict(p=P + 8), EINVAL, "p must be 16-byte"), (dict(ld_p=1004), EINVAL, "ld_p"), (dict(ld_p=1000), EINVAL, "ld_p"),
    (dict(B=0), EINVAL, "B"), (dict(k=0), EINVAL, "k"), (dict(V=0, ld_p=8), EINVAL, "V"),
    (dict(temperature=-0.5), EINVAL, "temperature"), (dict(temperature=NAN), EINVAL, "temperature"), (dict(top_p=0.0), EINVAL, "top_p"),
    (dict(top_p=NAN), EINVAL, "top_p"), (dict(u_accept=P + 2), EINVAL, "u_accept must be 4-byte"), (dict(u_draw=P + 1), EINVAL, "u_draw must be 4-byte"),
    (dict(n_accept=P + 2), EINVAL, "n_accept must be 4-byte"), (dict(token=P + 4), EINVAL, "token must be 8-byte"),
    (dict(draft=P + 4), EINVAL, "draft must be 8-byte"), (dict(ws=P + 4), EINVAL, "ws must be 8-byte"),
    (dict(ws_bytes=2 * 5 * 32 - 1), EINVAL, "obte_spec_verify_point_ws_bytes"), (dict(ws_bytes=0), EINVAL, "workspace"),
    (dict(k=32), EUNSUPPORTED, "k = 32"), (dict(V=65537, ld_p=65544), EUNSUPPORTED, "65537"),
])
def test_spec_verify_point_rejects_before_any_launch(kw, rc, word):
    assert _point(**kw) == rc
    assert _err().startswith("obte_spec_verify_point_bf16:") and word in _err(), _err()


def test_ops_refuse_bad_arguments_and_cpu_tensors():
    from omnibiote_amd import ops
    hist, lens = torch.zeros(2, 16, dtype=torch.int64), torch.ones(2, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.lookup_draft(hist, lens, 4)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.spec_verify_point(torch.zeros(2, 5, 16, dtype=BF), torch.zeros(2, 4, dtype=torch.int64))
    for bad in ((0, 4), (3, 2), (1, 17), (1,), "14", (1.0, 4), None, (True, 4)):
        with pytest.raises(ValueError, match="ngram"):
            ops._ngram("here", bad)
    assert ops._ngram("here", [2, 16]) == (2, 16)


# ------------------------------------------------------------------------------------------------------- the lookup rule
def _look(row, k, ngram=(1, 4), V=100, n=None):
    from omnibiote_amd.sampling import lookup_reference
    d, m = lookup_reference(torch.tensor([row]), torch.tensor([len(row) if n is None else n]), k, ngram[0], ngram[1], V)
    assert d.shape == (1, k) and d.dtype == torch.int64 and m.shape == (1,) and m.dtype == torch.int32
    return d[0].tolist(), int(m[0])


def test_lookup_reference_on_hand_written_rows():
    # the longest match wins over a more recent shorter one: "1 2 3" ended at 3, "2 3" at 7, "3" at 9
    assert _look([1, 2, 3, 40, 41, 2, 3, 50, 3, 60, 1, 2, 3], 3) == ([40, 41, 2], 3)
    # among equal lengths the most recent wins
    assert _look([1, 2, 30, 31, 1, 2, 40, 41, 9, 1, 2], 2) == ([40, 41], 2)
    # g_max caps the comparison: two occurrences of five tokens count as equal at four, the later one is taken
    assert _look([5, 6, 7, 8, 9, 30, 4, 6, 7, 8, 9, 40, 5, 6, 7, 8, 9], 1) == ([40], 4)
    assert _look([5, 6, 7, 8, 9, 30, 4, 6, 7, 8, 9, 40, 5, 6, 7, 8, 9], 1, ngram=(1, 5)) == ([30], 5)
    # a period-3 repeat is drafted periodically past the end of the history: e* = 5, d = 3
    assert _look([7, 8, 9, 7, 8, 9, 7, 8], 8) == ([9, 7, 8, 9, 7, 8, 9, 7], 4)
    assert _look([4, 4, 4], 5) == ([4] * 5, 2)                                     # period 1
    # no match, and n = 1: the last token repeated
    assert _look([1, 2, 3, 4], 3) == ([4, 4, 4], 0)
    assert _look([9], 4) == ([9] * 4, 0)
    assert _look([3, 5, 8, 2, 7, 7, 7], 2, n=4) == ([2, 2], 0)                     # only the first lens[b] tokens are the row
    # an out-of-range token matches nothing, not even itself — but it is drafted as it stands
    assert _look([200, 1, 200, 1, 200], 2) == ([200, 200], 0)
    assert _look([1, 200, 5, 1, 200, 5], 2) == ([1, 200], 1)                       # "5" alone: the comparison stops at 200
    assert _look([-1, 2, -1, 2], 3) == ([-1, 2, -1], 1)
    assert _look([1, 200, 5, 1, 200, 5], 2, V=201) == ([1, 200], 3)
    # g_min above the best match falls back
    assert _look([1, 2, 30, 31, 1, 2], 2, ngram=(3, 4)) == ([2, 2], 0)
    assert _look([1, 2, 30, 31, 1, 2], 2, ngram=(2, 4)) == ([30, 31], 2)
    # a match may not be longer than what lies before its end: e = 1 compares one token
    assert _look([6, 6], 3) == ([6, 6, 6], 1)


def test_lookup_reference_inactive_rows_and_batches():
    from omnibiote_amd.sampling import lookup_reference
    hist = torch.tensor([[1, 2, 1, 2, 0, 0], [3, 3, 3, 3, 3, 3], [1, 2, 1, 2, 0, 0], [5, 4, 5, 4, 5, 4]])
    d, m = lookup_reference(hist, torch.tensor([4, 0, -3, 7]), 3, 1, 4, 10)
    assert d.tolist() == [[1, 2, 1], [0, 0, 0], [0, 0, 0], [0, 0, 0]] and m.tolist() == [2, 0, 0, 0]
    d6, m6 = lookup_reference(hist, torch.tensor([6, 6, 6, 6]), 3, 1, 4, 10)
    assert d6.tolist() == [[0, 0, 0], [3, 3, 3], [0, 0, 0], [5, 4, 5]] and m6.tolist() == [1, 4, 1, 4]


# ------------------------------------------------------------------------------------------------------- the point rule
def _one_hot(x, V, dtype):
    q = torch.full(tuple(x.shape) + (V,), -INF, dtype=dtype)
    for b in range(x.shape[0]):
        for j in range(x.shape[1]):
            if 0 <= int(x[b, j]) < V:
                q[b, j, int(x[b, j])] = 0.0
    return q


def test_verify_point_reference_is_verify_reference_on_the_one_hot_q():
    from omnibiote_amd.sampling import sample_reference, verify_point_reference, verify_reference
    B, k, V = 48, 4, 96
    g = torch.Generator().manual_seed(21)
    p = (torch.randn(B, k + 1, V, generator=g) * 2.0).to(BF)
    x = torch.randint(0, V, (B, k), generator=g)
    x[::2] = p[::2, :k].float().argmax(dim=2)                            # every other row drafts the target's favourites
    x[1, 0], x[3, 2], x[5, 3], x[7, 1] = -1, V, 2 ** 62, -2 ** 63
    ua, ud = torch.rand(B, k, generator=g), torch.rand(B, generator=g)
    ua[2] = 0.0                                                          # whatever the target keeps stands
    ua[6, :2], ua[6, 2] = 0.0, 1.0                                       # and u = 1 is below no probability: two stand
    seen = set()
    for kw in (dict(), dict(temperature=0.8, top_k=50, top_p=0.9), dict(top_k=5), dict(top_k=1), dict(temperature=0)):
        for uniforms in ((ua, ud), (None, None)):
            got = verify_point_reference(p, x, *uniforms, **kw)
            want = verify_reference(p, _one_hot(x, V, BF), x, *uniforms, **kw)
            for a, b in zip(got, want):
                assert torch.equal(a, b), kw
            seen.update(got[0].tolist())
    assert seen == set(range(k + 1))                                     # every acceptance count occurs
    # in words: x_0 stands iff u < P_0(x_0); behind a rejection the token is never x_0; behind k acceptances it is the draw on p[k]
    a, tok, _ = verify_point_reference(p, x, ua, ud)
    P0 = torch.softmax(p[:, 0].double(), dim=1)
    inside = (x[:, 0] >= 0) & (x[:, 0] < V)
    px = torch.where(inside, P0.gather(1, x[:, :1].clamp(0, V - 1)).squeeze(1), torch.zeros(B, dtype=torch.float64))
    assert torch.equal(a >= 1, ua[:, 0].double() < px)
    assert (tok[a == 0] != x[a == 0, 0]).all() and (a == 0).any()
    full = a == k
    assert full.any() and torch.equal(tok[full], sample_reference(p[full, k], ud[full])[0])
    one = verify_point_reference(p[4], x[4], ua[4], float(ud[4]))       # one row in, scalars out
    assert int(one[0]) == int(a[4]) and int(one[1]) == int(tok[4]) and one[2].shape == (V,)


# ------------------------------------------------------------------------------------------------------- the model's checks
def _model(vocab=64, block=32, autoregressive=True):
    from omnibiote_amd.model import OmniBioTA, OmniBioTAConfig
    c = OmniBioTAConfig()
    c.block_size, c.vocab_size, c.n_layer, c.n_head, c.n_embd, c.dropout, c.flash = block, vocab, 1, 2, 128, 0.0, True
    c.autoregressive = autoregressive
    return OmniBioTA(c)


def test_generate_lookup_validates_before_any_device_work():
    m = _model()
    idx = torch.zeros(2, 8, dtype=torch.int64)
    for kw, word in ((dict(k=0), "k must"), (dict(k=32), "k must"), (dict(k=-3), "k must"), (dict(k=2.0), "k must"),
                     (dict(ngram=(0, 4)), "ngram"), (dict(ngram=(5, 4)), "ngram"), (dict(ngram=(1, 17)), "ngram"), (dict(ngram=3), "ngram"),
                     (dict(top_p=0.0), "top_p"), (dict(top_k=0), "top_k"), (dict(temperature=-1.0), "temperature"),
                     (dict(lengths=[8, 9]), "length"), (dict(lengths=[8]), "lengths"),
                     (dict(k=4, max_new_tokens=21), "block_size = 32"),                  # 8 + 21 + 4 > 32
                     (dict(k=31, max_new_tokens=1), "k = 31 drafted"), (dict(max_new_tokens=-1), "block_size")):
        kw = dict(dict(max_new_tokens=4), **kw)
        with pytest.raises(ValueError, match=word) as e:
            m.generate_lookup(idx, **kw)
        assert "generate_lookup" in str(e.value) and "two models" not in str(e.value)
    with pytest.raises(ValueError, match="autoregressive"):
        _model(autoregressive=False).generate_lookup(idx, 4)
    with pytest.raises(ValueError, match="idx must be"):
        m.generate_lookup(idx[0], 4)
    with pytest.raises(ValueError, match="history of 8205"):            # 8000 + 192 + 12 + 1 columns: more than the lookup takes
        _model(block=8300).generate_lookup(torch.zeros(1, 8000, dtype=torch.int64), 192, k=12)
    # the bound is longest + new + k <= block_size exactly: 8 + 20 + 4 = 32 passes the checks and reaches the device code, which a CPU model refuses
    with pytest.raises(RuntimeError):
        m.generate_lookup(idx, 20, k=4)
    out, stats = m.generate_lookup(idx, 0, return_stats=True)            # nothing to generate: no device work at all
    assert torch.equal(out, idx) and stats == dict(rounds=0, drafted=0, accepted=0, matched=0)
    out, n = m.generate_lookup(idx, 0, lengths=[8, 5])
    assert out.shape == (2, 8) and n.tolist() == [8, 5] and (out[1, 5:] == 0).all()


def test_lookup_and_verify_refuses_caches_and_arguments_before_any_launch():
    from omnibiote_amd.model import CachePositions, PagedPositions, SharedPrefixCache
    m = _model()
    pending, hist, lens = torch.zeros(2, dtype=torch.int64), torch.zeros(2, 16, dtype=torch.int64), torch.ones(2, dtype=torch.int32)

    class Bf16(CachePositions):
        dtype = "bf16"

    class Fp8(CachePositions):
        dtype = "fp8"

    with pytest.raises(NotImplementedError, match="lookup_and_verify: the cache is an fp8 cache"):
        m.lookup_and_verify(pending, Fp8(2, 32), hist, lens, 4)
    shared = SharedPrefixCache.__new__(SharedPrefixCache)                # the refusal looks at the type and the dtype alone
    shared.dtype = "bf16"
    with pytest.raises(NotImplementedError, match="lookup_and_verify: the cache is a shared-prefix cache"):
        m.lookup_and_verify(pending, shared, hist, lens, 4)
    paged = PagedPositions.__new__(PagedPositions)
    paged.dtype = "bf16"
    with pytest.raises(NotImplementedError, match="lookup_and_verify: the cache is a paged cache"):
        m.lookup_and_verify(pending, paged, hist, lens, 4)
    for kw, word in ((dict(k=0), "k must"), (dict(k=32), "k must"), (dict(k=4, ngram=(2, 1)), "ngram"), (dict(k=4, ngram=(1, 40)), "ngram")):
        with pytest.raises(ValueError, match=word):
            m.lookup_and_verify(pending, Bf16(2, 32), hist, lens, **kw)
    with pytest.raises(RuntimeError, match="no CPU fallback"):           # the checks passed: the first launch refuses CPU tensors
        m.lookup_and_verify(pending, Bf16(2, 32), hist, lens, 4)
