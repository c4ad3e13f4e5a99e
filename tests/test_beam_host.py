"""Host-side tests (no GPU) of beam search (include/omnibiote_hip_beam.h): the symbol table against the header, the pins of the ABI, the
workspace sizes, every argument check of the three entry points that returns before a launch, the float64 rule
(sampling.beam_step_reference) on hand-made cases, sampling.beam_sequences_reference against parent-pointer backtracking, and the
validation of OmniBioTA.generate_beam on a CPU model."""
import ctypes as C
import math
import os
import re

import pytest
import torch

from omnibiote_amd import _lib
from omnibiote_amd.sampling import beam_sequences_reference, beam_step_reference

EINVAL, EUNSUPPORTED = -1, -3
P = 4096   # a non-null, 16-byte aligned "pointer" for calls that must return before they touch it
Q = 1 << 20   # another one, far enough away that no two buffers overlap
BIG = 1 << 30
NAMES = ("obte_beam_select_ws_bytes", "obte_beam_select_bf16", "obte_attn_decode_beam", "obte_block_decode_beam_ws_bytes", "obte_block_decode_beam")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = float("inf")


def _err():
    return _lib.lib().obte_last_error().decode()


def test_symbols_are_what_the_header_declares():
    assert tuple(_lib.SYMBOLS_BEAM) == NAMES
    header = open(os.path.join(ROOT, "include", "omnibiote_hip_beam.h")).read()
    body = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    assert tuple(re.findall(r"\b(obte_\w+)\s*\(", body)) == NAMES                  # the declarations, in order
    assert '#include "omnibiote_hip.h"' in header and "struct" not in body
    assert re.search(r"#define\s+OBTE_BEAM_MAX_WIDTH\s+%d\b" % _lib.BEAM_MAX_WIDTH, header) and _lib.BEAM_MAX_WIDTH == 32
    make = open(os.path.join(ROOT, "omnibiote_amd", "csrc", "Makefile")).read()
    assert re.search(r"^HDRS\s*=.*include/omnibiote_hip_beam\.h", make, flags=re.M) and re.search(r"^SRCS\s*=.*\bbeam\.hip\b", make, flags=re.M)
    lib = _lib.lib()
    for name in NAMES:
        for table in (_lib.SYMBOLS, _lib.SYMBOLS_SHARED, _lib.SYMBOLS_SAMPLE, _lib.SYMBOLS_CONSTRAIN):
            assert name not in table
        res, args = _lib.SYMBOLS_BEAM[name]
        fn = getattr(lib, name)                                                     # the library exports it
        assert fn.restype is res and list(fn.argtypes) == args                      # bound by lib(), in the same loop
    assert len(_lib.SYMBOLS) == 70 and len(_lib.SYMBOLS_SHARED) == 5
    assert lib.obte_abi_version() == 1
    sizes = (C.c_int64 * 16)()
    assert lib.obte_struct_sizes(sizes, 16) == 6


def test_workspace_sizes():
    lib = _lib.lib()
    ws = lib.obte_beam_select_ws_bytes
    for Pn, W in [(1, 1), (1, 8), (3, 5), (8, 8), (2, 32)]:
        B = Pn * W
        assert ws(Pn, W) == (B * W * 4 + 15) // 16 * 16 + B * 16 and ws(Pn, W) % 16 == 0      # W packed words and one 16-byte record per row
    for bad in [(0, 4), (1, 0), (1, 33), (-1, 4), (1 << 40, 4)]:
        assert ws(*bad) == 0, bad
    for Pn, G, Cc, H in [(1, 1, 128, 2), (3, 5, 256, 2), (2, 32, 256, 4)]:
        assert lib.obte_block_decode_beam_ws_bytes(Pn, G, Cc, H) == lib.obte_block_decode_shared_ws_bytes(Pn, G, Cc, H) > 0
    assert lib.obte_block_decode_beam_ws_bytes(2, 4, 128, 4) == 0 and lib.obte_block_decode_beam_ws_bytes(0, 4, 256, 2) == 0


def _select(logits=P, ld=512, Pn=2, W=4, V=500, score_in=P, done_in=P, eos=-1, allowed=None, allowed_ld=0, anc_in=P, T_suf=16, slot=3, parent=P, token=P,
            score_out=P, done_out=P, anc_out=Q, hist=P, ws=P, ws_bytes=BIG):
    return _lib.lib().obte_beam_select_bf16(logits, ld, Pn, W, V, score_in, done_in, eos, allowed, allowed_ld, anc_in, T_suf, slot, parent, token, score_out,
                                            done_out, anc_out, hist, ws, ws_bytes, None)


@pytest.mark.parametrize("kw,word", [
    (dict(logits=None), "null"), (dict(score_in=None), "null"), (dict(done_in=None), "null"), (dict(anc_in=None), "null"), (dict(parent=None), "null"),
    (dict(token=None), "null"), (dict(score_out=None), "null"), (dict(done_out=None), "null"), (dict(anc_out=None), "null"), (dict(hist=None), "null"),
    (dict(W=0), "W = 0"), (dict(W=33), "W = 33"), (dict(W=-1), "W"), (dict(Pn=0), "P"), (dict(V=0), "V"),
    (dict(ld=508), "ld"), (dict(ld=496), "ld"), (dict(logits=P + 8), "logits"),
    (dict(eos=-2), "eos_token"), (dict(eos=500), "eos_token"),
    (dict(allowed=P, allowed_ld=-1), "allowed_ld"), (dict(allowed=P, allowed_ld=62), "allowed_ld"),
    (dict(T_suf=0), "T_suf"), (dict(slot=16), "slot = 16"), (dict(slot=-1), "slot"),
    (dict(score_in=P + 2), "score_in"), (dict(score_out=P + 2), "score_out"), (dict(parent=P + 2), "parent"), (dict(anc_in=P + 2), "ancestry_in"),
    (dict(anc_out=Q + 2), "ancestry_out"), (dict(token=P + 4), "token"), (dict(hist=P + 4), "token_hist"),
    (dict(anc_out=P), "overlap"), (dict(anc_out=P + 4 * 8 * 16 - 4), "overlap"),       # the same buffer; the last entry of one on the first of the other
    (dict(ws=None), "workspace"), (dict(ws=P + 8), "workspace"), (dict(ws_bytes=None), "workspace"),
])
def test_beam_select_rejects_before_any_launch(kw, word):
    if "ws_bytes" in kw and kw["ws_bytes"] is None:
        kw = dict(kw, ws_bytes=_lib.lib().obte_beam_select_ws_bytes(2, 4) - 1)           # one byte short
    assert _select(**kw) == EINVAL
    assert _err().startswith("obte_beam_select_bf16:") and word in _err(), _err()


def test_beam_select_vocabulary_bound():
    assert _select(V=65537, ld=65544) == EUNSUPPORTED
    assert _err().startswith("obte_beam_select_bf16:") and "65536" in _err(), _err()
    assert _select(anc_out=P + 4 * 8 * 16, ws_bytes=1) == EINVAL and "workspace" in _err()   # adjacent ancestry buffers do not overlap: the next refusal


def _attn(q=P, q_ld=256, pre=P, Pn=2, T_pre=100, n_prefix=40, suf=P, G=3, T_suf=50, n_suffix=7, anc=P, o=P, lse=None, H=2, hs=128, ps=1, ss=1, ws=P, ws_bytes=BIG):
    return _lib.lib().obte_attn_decode_beam(q, q_ld, pre, Pn, T_pre, n_prefix, suf, G, T_suf, n_suffix, anc, o, lse, H, hs, 1.0, ps, ss, ws, ws_bytes, None)


@pytest.mark.parametrize("kw,word", [
    (dict(q=None), "null"), (dict(pre=None), "null"), (dict(o=None), "null"), (dict(suf=None), "null"), (dict(anc=None), "null"),
    (dict(n_prefix=0), "n_prefix"), (dict(n_prefix=101), "n_prefix"), (dict(n_suffix=51), "n_suffix"), (dict(n_suffix=-1), "n_suffix"),
    (dict(hs=32, q_ld=64), "head_dim"), (dict(hs=256, q_ld=512), "head_dim"), (dict(Pn=0), "shape"), (dict(G=0), "shape"), (dict(H=0), "shape"),
    (dict(Pn=40000), "65535"), (dict(G=20000), "65535"), (dict(T_pre=0), "shape"), (dict(T_suf=-1), "shape"),
    (dict(q_ld=260), "q_ld"), (dict(q_ld=128), "q_ld"),
    (dict(q=P + 8), "aligned"), (dict(pre=P + 8), "aligned"), (dict(suf=P + 8), "aligned"), (dict(o=P + 8), "aligned"), (dict(lse=P + 2), "aligned"),
    (dict(anc=P + 2), "ancestry"),
    (dict(ps=-1), "prefix_splits"), (dict(ps=_lib.ATTN_SHARED_MAX_SPLITS + 1), "prefix_splits"), (dict(ss=-1), "suffix_splits"),
    (dict(ss=_lib.ATTN_DECODE_MAX_SPLITS + 1), "suffix_splits"),
    (dict(ws=None), "workspace"), (dict(ws=P + 4), "workspace"), (dict(ws_bytes=64), "workspace"),
    (dict(ps=3, ss=2, ws_bytes=None), "workspace"),
])
def test_attn_decode_beam_rejects_before_any_launch(kw, word):
    if "ws_bytes" in kw and kw["ws_bytes"] is None:
        kw = dict(kw, ws_bytes=_lib.lib().obte_attn_decode_shared_ws_bytes(2, 3, 2, 128, kw["ps"], kw["ss"]) - 1)
    assert _attn(**kw) == EINVAL
    assert _err().startswith("obte_attn_decode_beam:") and word in _err(), _err()


def _desc(B=6, T=1, C_=256, H=2, **over):
    f = dict(B=B, T=T, n_embd=C_, n_head=H, ln1_w=P, attn_w=P, proj_w=P, ln2_w=P, fc_w=P, mlp_w=P, rope_cos=P, rope_sin=P)
    f.update(over)
    return _lib.BlockDesc(**f)


def test_block_decode_beam_rejects_before_any_launch():
    lib = _lib.lib()

    def step(d, x=P, y=P, pre=P, Pn=2, T_pre=100, n_prefix=40, suf=P, T_suf=50, suf_pos=5, anc=P, ws=P, ws_bytes=BIG):
        return lib.obte_block_decode_beam(C.byref(d) if d is not None else None, x, y, pre, Pn, T_pre, n_prefix, suf, T_suf, suf_pos, anc, ws, ws_bytes, None)
    assert step(None) == EINVAL and "obte_block_decode_beam" in _err() and "null" in _err()
    for over in (dict(key_ranges=P), dict(out_rows=P, n_out_rows=1), dict(dropout_p=0.1), dict(mask=P), dict(query_bounds=P)):
        assert step(_desc(**over)) == EUNSUPPORTED, over
        assert _err().startswith("obte_block_decode_beam:"), _err()
    for kw in (dict(x=None), dict(y=None), dict(pre=None), dict(suf=None), dict(ws=None), dict(anc=None)):
        assert step(_desc(), **kw) == EINVAL and _err().startswith("obte_block_decode_beam:") and "null" in _err(), (kw, _err())
    assert step(_desc(T=2)) == EINVAL and "T = 1" in _err()
    assert step(_desc(), Pn=4) == EINVAL and "groups" in _err()
    for kw in (dict(n_prefix=0), dict(n_prefix=101), dict(T_pre=0)):
        assert step(_desc(), **kw) == EINVAL and "n_prefix" in _err(), (kw, _err())
    for kw in (dict(suf_pos=50), dict(suf_pos=-1), dict(T_suf=0, suf_pos=0)):
        assert step(_desc(), **kw) == EINVAL and "suffix slot" in _err(), (kw, _err())
    assert step(_desc(), pre=P + 8) == EINVAL and "aligned" in _err()
    assert step(_desc(), suf=P + 8) == EINVAL and "aligned" in _err()
    assert step(_desc(), anc=P + 2) == EINVAL and "ancestry" in _err() and "aligned" in _err()
    assert step(_desc(B=40000), Pn=1) == EINVAL and "65535" in _err()
    assert step(_desc(), ws_bytes=lib.obte_block_decode_beam_ws_bytes(2, 3, 256, 2) - 1) == EINVAL
    assert _err().startswith("obte_block_decode_beam:") and "workspace" in _err() and "obte_block_decode_beam_ws_bytes" in _err(), _err()
    assert step(_desc(C_=128, H=4)) == EINVAL and _err().startswith("obte_block_decode_beam:") and "head" in _err(), _err()


# ------------------------------------------------------------------------------------------------------- the float64 rule
def _lsm(row):
    return torch.log_softmax(torch.tensor(row, dtype=torch.float64), dim=0)


def test_reference_picks_the_best_of_all_beams_and_inherits_the_ancestry():
    W, V = 2, 4
    logits = torch.tensor([[0.0, 1.0, 2.0, 3.0], [3.0, 0.0, 0.0, 0.0]])
    score = torch.tensor([-1.0, -0.5])
    anc = torch.tensor([[1, 0, 7], [0, 1, 7]])
    parent, token, s, done, a, ranked = beam_step_reference(logits, score, [0, 0], anc, 2, W)
    l0, l1 = _lsm(logits[0].tolist()), _lsm(logits[1].tolist())
    cands = sorted([(-1.0 + l0[v].item(), 0, v) for v in range(V)] + [(-0.5 + l1[v].item(), 1, v) for v in range(V)], key=lambda c: (-c[0], c[1], c[2]))
    assert parent.tolist() == [cands[0][1], cands[1][1]] and token.tolist() == [cands[0][2], cands[1][2]]
    assert (parent.tolist(), token.tolist()) == ([1, 0], [0, 3])
    assert torch.allclose(s, torch.tensor([cands[0][0], cands[1][0]], dtype=torch.float64), atol=1e-12) and done.tolist() == [False, False]
    assert a.tolist() == [[0, 1, 0], [1, 0, 1]]                                       # the parent's entries below the slot, then the row's own beam
    assert len(ranked) == 1 and torch.allclose(ranked[0], torch.tensor([c[0] for c in cands[:3]], dtype=torch.float64), atol=1e-12)
    assert s.dtype == torch.float64 and parent.dtype == torch.int64


def test_reference_tie_order_is_beam_then_token():
    W = 3
    row = [0.0, 2.0, 2.0, -1.0, 2.0]
    logits = torch.tensor([row, row, row, [5.0, 0, 0, 0, 0], [0.0] * 5, [0.0] * 5])    # group 1: one peaked row, two dead ones
    score = torch.tensor([-1.0, -1.0, -2.0, 0.0, -INF, -INF])
    parent, token, s, done, a, _ = beam_step_reference(logits, score, [0] * 6, torch.zeros(6, 1, dtype=torch.int64), 0, W)
    assert parent[:3].tolist() == [0, 0, 0] and token[:3].tolist() == [1, 2, 4]        # equal S: the lower beam first, inside it the lower token
    assert s[0] == s[1] == s[2]
    assert parent[3:].tolist() == [3, 3, 3] and token[3].item() == 0 and sorted(token[4:].tolist()) == [1, 2]
    assert token[4:].tolist() == [1, 2]                                               # equal logits inside a row: the lower token
    assert a[:, 0].tolist() == [0, 1, 2, 0, 1, 2]
    two = beam_step_reference(torch.tensor([row, row]), torch.tensor([-1.0, -1.0]), [0, 0], torch.zeros(2, 1, dtype=torch.int64), 0, 2)
    assert two[0].tolist() == [0, 0] and two[1].tolist() == [1, 2]
    four = beam_step_reference(torch.tensor([row] * 4), torch.tensor([-1.0] * 4), [0] * 4, torch.zeros(4, 1, dtype=torch.int64), 0, 4)
    assert four[0].tolist() == [0, 0, 0, 1] and four[1].tolist() == [1, 2, 4, 1]       # beam 0's three ties, then beam 1's first


def test_reference_done_dead_and_short_groups():
    W, V, eos = 3, 6, 4
    g = torch.Generator().manual_seed(0)
    logits = torch.randn(2 * W, V, generator=g)
    logits[1] = float("nan")                                                         # live, but no candidate column
    score = torch.tensor([-0.25, -0.5, -INF, -3.0, float("nan"), -1.0])
    done = [1, 0, 0, 0, 0, 1]
    anc = torch.arange(2 * W * 2).view(2 * W, 2) % W
    parent, token, s, d, a, ranked = beam_step_reference(logits, score, done, anc, 1, W, eos_token=eos)
    # group 0: the done row's single candidate alone
    assert parent[:W].tolist() == [0, 1, 2] and token[:W].tolist() == [eos, eos, eos] and d[:W].tolist() == [True, True, True]
    assert s[0].item() == -0.25 and s[1].item() == -INF and s[2].item() == -INF and ranked[0].tolist() == [-0.25]
    assert a[0].tolist() == [anc[0, 0].item(), 0] and a[1].tolist() == [anc[1, 0].item(), 1]      # a dead rank copies its own row
    # group 1: the done row 5 (frozen at -1) against the live row 3's columns
    l3 = _lsm(logits[3].tolist()) - 3.0
    top = torch.sort(l3, descending=True)
    cands = sorted([(-1.0, 2, eos)] + [(top.values[i].item(), 0, top.indices[i].item()) for i in range(V)], key=lambda c: (-c[0], c[1], c[2]))[:W]
    assert parent[W:].tolist() == [W + c[1] for c in cands] and token[W:].tolist() == [c[2] for c in cands]
    assert (5 in parent[W:].tolist()) and s[W:][parent[W:] == 5].item() == -1.0              # a finished beam's score is frozen
    assert d[W:].tolist() == [c[1] == 2 or c[2] == eos for c in cands]
    assert all(a[W + r].tolist() == [anc[parent[W + r], 0].item(), r] for r in range(W))
    none = beam_step_reference(logits, score, done, anc, 1, W)                       # without an eos_token a done row proposes token 0
    assert none[1][0].item() == 0 and none[3][:W].tolist() == [True, True, True]


def test_reference_mask_and_special_values():
    W = 2
    logits = torch.tensor([[1.0, -INF, 3.0, float("nan"), 2.0], [0.0, 0.0, 0.0, 0.0, 0.0]])
    allowed = torch.tensor([[True, True, False, True, True], [False, False, False, True, False]])
    parent, token, s, d, a, _ = beam_step_reference(logits, [0.0, 0.0], [0, 0], torch.zeros(2, 1, dtype=torch.int64), 0, W, allowed=allowed)
    assert (parent.tolist(), token.tolist()) == ([1, 0], [3, 4])                     # row 1's single column has log p = 0
    assert s[0].item() == 0.0 and math.isclose(s[1].item(), 2.0 - math.log(math.exp(1.0) + math.exp(2.0)), rel_tol=1e-12)
    shared = beam_step_reference(logits, [0.0, -INF], [0, 0], torch.zeros(2, 1, dtype=torch.int64), 0, W, allowed=allowed[0])
    assert shared[0].tolist() == [0, 0] and shared[1].tolist() == [4, 0]
    inf = beam_step_reference(torch.tensor([[INF, 0.0, INF], [0.0, 0.0, 0.0]]), [0.0, -INF], [0, 0], torch.zeros(2, 1, dtype=torch.int64), 0, W)
    assert inf[1].tolist() == [0, 2] and torch.allclose(inf[2], torch.full((2,), -math.log(2.0), dtype=torch.float64))


def test_sequences_reference_against_backtracking():
    g = torch.Generator().manual_seed(3)
    Pn, W, n, V, eos = 3, 4, 7, 11, 5
    B = Pn * W
    hist = torch.zeros(n, B, dtype=torch.int64)
    parents = torch.zeros(n, B, dtype=torch.int64)
    tables = [torch.full((B, n), -7, dtype=torch.int64), torch.full((B, n), -7, dtype=torch.int64)]
    for i in range(n):
        logits = torch.randn(B, V, generator=g)
        score = -torch.rand(B, generator=g)
        parent, token, _, _, a, _ = beam_step_reference(logits, score, [0] * B, tables[i & 1], i, W)
        hist[i], parents[i] = token, parent
        tables[(i + 1) & 1][:, :i + 1] = a
    final = tables[n & 1]
    seq, lengths = beam_sequences_reference(hist, final, n, W)
    for b in range(B):                                                               # follow the parent pointers back from the last step
        row, want = b, []
        for i in range(n - 1, -1, -1):
            want.append(hist[i, row].item())
            row = parents[i, row].item()
        assert seq[b].tolist() == want[::-1], b
    assert lengths.tolist() == [n] * B
    seq_e, len_e = beam_sequences_reference(hist, final, n, W, eos_token=eos, pad_token=99)
    for b in range(B):
        row = seq[b].tolist()
        k = row.index(eos) + 1 if eos in row else n
        assert len_e[b].item() == k and seq_e[b].tolist() == row[:k] + [99] * (n - k)
    assert beam_sequences_reference(hist, final, n, W, eos_token=eos)[0][len_e < n][:, -1].eq(eos).all()     # the default padding is the eos_token
    short, _ = beam_sequences_reference(hist, tables[1], 1, W)                       # one step: the first table's first column
    assert short.shape == (B, 1)


# ------------------------------------------------------------------------------------------------------- the model surface
def _cpu_model(block_size=32, autoregressive=True):
    from omnibiote_amd.model import OmniBioTA, OmniBioTAConfig
    c = OmniBioTAConfig()
    c.block_size, c.vocab_size, c.n_layer, c.n_head, c.n_embd, c.dropout, c.flash = block_size, 64, 1, 2, 128, 0.0, True
    c.autoregressive = autoregressive
    return OmniBioTA(c)


def test_generate_beam_argument_errors():
    from omnibiote_amd.model import BeamResult
    m = _cpu_model()
    idx = torch.zeros(2, 4, dtype=torch.int64)
    with pytest.raises(ValueError, match="autoregressive"):
        _cpu_model(autoregressive=False).generate_beam(idx, 4, num_beams=2)
    for bad in (0, 33, -1, 2.0, True):
        with pytest.raises(ValueError, match="num_beams"):
            m.generate_beam(idx, 4, num_beams=bad)
    with pytest.raises(ValueError, match="block_size"):
        m.generate_beam(idx, 29, num_beams=2)
    with pytest.raises(ValueError, match="allows nothing"):
        m.generate_beam(idx, 4, num_beams=2, allowed_tokens=[])
    with pytest.raises(ValueError, match="allows nothing"):
        m.generate_beam(idx, 4, num_beams=2, allowed_tokens=torch.zeros(64, dtype=torch.bool))
    with pytest.raises(ValueError, match="vocab_size"):
        m.generate_beam(idx, 4, num_beams=2, allowed_tokens=[64])
    with pytest.raises(ValueError, match="eos_token"):
        m.generate_beam(idx, 4, num_beams=2, eos_token=64)
    with pytest.raises(ValueError, match="length_penalty"):
        m.generate_beam(idx, 4, num_beams=2, length_penalty=float("nan"))
    with pytest.raises(ValueError, match="idx"):
        m.generate_beam(idx[0], 4, num_beams=2)
    out = m.generate_beam(idx + torch.arange(2).view(2, 1), 0, num_beams=3)          # nothing to search: the prompts, once per beam
    assert isinstance(out, BeamResult) and out.sequences.shape == (2, 3, 4) and out.sequences[:, :, 0].tolist() == [[0, 0, 0], [1, 1, 1]]
    assert out.scores.tolist() == [[0.0, -INF, -INF]] * 2 and out.lengths.tolist() == [[0, 0, 0]] * 2
    with pytest.raises(RuntimeError, match="GPU"):                                   # valid arguments go on to the first device-side requirement
        m.generate_beam(idx, 4, num_beams=2, allowed_tokens=[1, 2, 3], eos_token=3)
