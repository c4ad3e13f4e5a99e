"""Host-side tests (no GPU) of sequence scoring: the symbol table of the three entry points against their companion header, the choice of
the split over V and the workspace size, every argument check that returns before a launch, the rule's plain-torch statement
(scoring.score_reference), and the validation of ops.readout_score, OmniBioTA.score and OmniBioTA.token_logprobs."""
import ctypes as C
import math
import os
import re

import pytest
import torch

from omnibiote_amd import _lib
from omnibiote_amd.scoring import score_reference

EINVAL = -1
P = 4096   # a non-null, 16-byte aligned "pointer" for calls that must return before they touch it
NAMES = ("obte_readout_score_slices", "obte_readout_score_ws_bytes", "obte_readout_score_bf16")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _err():
    return _lib.lib().obte_last_error().decode()


def test_score_symbols_have_their_own_table():
    lib = _lib.lib()
    assert tuple(_lib.SYMBOLS_SCORE) == NAMES
    header = open(os.path.join(ROOT, "include", "omnibiote_hip_score.h")).read()
    assert tuple(re.findall(r"^(?:int|int32_t|int64_t|void|const char\*) +(obte_[a-z0-9_]+)\(", header, flags=re.M)) == NAMES   # in the header's order
    assert len(re.findall(r"^[a-z0-9_\* ]+\bobte_[a-z0-9_]+\(", header, flags=re.M)) == len(NAMES)                               # and nothing else
    assert '#include "omnibiote_hip.h"' in header and not re.search(r"\bstruct\b", header)
    others = (_lib.SYMBOLS, _lib.SYMBOLS_ROWS, _lib.SYMBOLS_SMALL_M, _lib.SYMBOLS_SAMPLE, _lib.SYMBOLS_EXTEND, _lib.SYMBOLS_SPEC, _lib.SYMBOLS_KV8,
              _lib.SYMBOLS_SHARED, _lib.SYMBOLS_LOOP, _lib.SYMBOLS_CONSTRAIN, _lib.SYMBOLS_W8)
    for name in NAMES:
        for table in others:
            assert name not in table
        fn = getattr(lib, name)
        res, args = _lib.SYMBOLS_SCORE[name]
        assert fn.restype is res and list(fn.argtypes) == args                                                                    # bound by lib()
    assert [len(t) for t in others] == [70, 3, 3, 1, 6, 2, 6, 5, 1, 2, 2]
    assert lib.obte_abi_version() == 1
    sizes = (C.c_int64 * 16)()
    assert lib.obte_struct_sizes(sizes, 16) == 6
    makefile = open(os.path.join(ROOT, "omnibiote_amd", "csrc", "Makefile")).read()
    assert "omnibiote_hip_score.h" in makefile and "readout_score.hip" in makefile


def test_slices_and_workspace():
    lib = _lib.lib()
    for R in (1, 127, 129, 1024, 8192, 65536, 2 ** 31 - 1):
        for V in (1, 5, 128, 129, 1000, 65536, 2 ** 31 - 1):
            s = lib.obte_readout_score_slices(R, V)
            assert 1 <= s <= 64 and s <= (V + 127) // 128, (R, V, s)
            assert lib.obte_readout_score_ws_bytes(R, V, 0) == lib.obte_readout_score_ws_bytes(R, V, s) == 8 * R * s
            sizes = [lib.obte_readout_score_ws_bytes(R, V, k) for k in range(1, 65)]
            assert sizes == sorted(sizes) and sizes[0] == 8 * R and sizes[-1] == 8 * R * 64                                      # O(R slices)
    assert lib.obte_readout_score_slices(1024, 65536) * 8 >= 256                       # row tiles x slices covers the device
    assert lib.obte_readout_score_slices(8192, 65536) * 64 <= 4 * 256                  # and does not shred a launch that fills it already
    for bad in ((0, 5, 1), (4, 0, 1), (4, 2 ** 31, 1), (4, 5, -1), (4, 5, 65)):
        assert lib.obte_readout_score_ws_bytes(*bad) == -1
    assert lib.obte_readout_score_slices(0, 5) == 1 and lib.obte_readout_score_slices(5, 0) == 1


def _score(x=P, ldx=64, w=P, ldw=64, R=4, V=100, Cc=64, alpha=1.0, targets=P, K=1, logprobs=P, lse=P, logits_at=P, slices=0, ws=P, ws_bytes=1 << 20):
    return _lib.lib().obte_readout_score_bf16(x, ldx, w, ldw, R, V, Cc, alpha, targets, K, logprobs, lse, logits_at, slices, ws, ws_bytes, None)


@pytest.mark.parametrize("kw,word", [
    (dict(Cc=96, ldx=96, ldw=96), "C must"), (dict(Cc=0), "C must"), (dict(K=0), "K must"), (dict(K=65), "K must"), (dict(V=0), "V must"),
    (dict(V=2 ** 31), "V must"), (dict(R=0), "R must"), (dict(ws_bytes=4 * 8 - 1), "ws_bytes"), (dict(slices=3, ws_bytes=3 * 4 * 8 - 1), "ws_bytes"),
    (dict(slices=-1), "slices"), (dict(slices=65), "slices"), (dict(ldx=68), "ldx"), (dict(ldw=68), "ldw"), (dict(ldx=56), "ldx"),
    (dict(x=None), "null"), (dict(w=None), "null"), (dict(targets=None), "null"), (dict(logprobs=None), "null"), (dict(lse=None), "null"),
    (dict(logits_at=None), "null"), (dict(ws=None), "null"), (dict(x=P + 8), "x must be 16-byte"), (dict(w=P + 2), "w must be 16-byte"),
    (dict(ws=P + 4), "ws must be 8-byte"), (dict(targets=P + 2), "targets must be 4-byte"), (dict(lse=P + 1), "lse must be 4-byte"),
])
def test_score_rejects_before_any_launch(kw, word):
    assert _score(**kw) == EINVAL
    assert _err().startswith("obte_readout_score_bf16:") and word in _err(), _err()


# ----------------------------------------------------------------------------------------------- the rule in plain torch
def test_score_reference_is_a_distribution_and_marks_its_targets():
    g = torch.Generator().manual_seed(3)
    R, V, Cc = 6, 7, 64
    x, w = torch.randn(R, Cc, generator=g), torch.randn(V, Cc, generator=g)
    lp, lse, at, zb = score_reference(x, w, torch.arange(V).expand(R, V).contiguous(), 0.25)
    assert lp.dtype == lse.dtype == at.dtype == zb.dtype == torch.float64 and lp.shape == at.shape == zb.shape == (R, V) and lse.shape == (R,)
    assert (torch.exp(lp).sum(dim=1) - 1).abs().max().item() <= 1e-12
    z = 0.25 * x.double() @ w.double().t()
    assert torch.equal(at, z) and torch.equal(lp, z - lse.unsqueeze(1))
    assert torch.allclose(zb, 2.0 ** -8 * z.abs() + Cc * 2.0 ** -24 * 0.25 * (x.double().abs() @ w.double().abs().t()), rtol=1e-15, atol=0)
    t = torch.tensor([[0, -1], [-1, 6], [7, 1], [-2, 2], [3, 3], [2 ** 31 - 1, -1]])
    lp, _, at, _ = score_reference(x, w, t, 0.25)
    assert lp[0, 1] == 0 and at[0, 1] == 0 and lp[1, 0] == 0 and at[5, 1] == 0                        # -1: no candidate
    for r, k in ((2, 0), (3, 0), (5, 0)):                                                             # anything else out of range: NaN in both
        assert math.isnan(lp[r, k]) and math.isnan(at[r, k])
    assert lp[4, 0] == lp[4, 1] == z[4, 3] - lse[4]
    lp1, lse1, at1, _ = score_reference(x, w, t[:, 1].contiguous().to(torch.int32), 0.25)             # (R,) in, (R,) out
    assert lp1.shape == at1.shape == (R,) and torch.equal(lp1, lp[:, 1]) and torch.equal(lse1, lse)
    # uniform logits: lse = log V, whatever their value
    lp, lse, at, _ = score_reference(torch.ones(3, 64), torch.ones(50, 64), torch.zeros(3, dtype=torch.int64), 0.5)
    assert torch.equal(at, torch.full((3,), 32.0, dtype=torch.float64)) and (lse - 32.0 - math.log(50)).abs().max().item() <= 1e-12
    for bad in (dict(x=torch.zeros(3, 32)), dict(targets=torch.zeros(4, dtype=torch.int64)), dict(targets=torch.zeros(3))):
        kw = dict(x=torch.zeros(3, 64), w=torch.zeros(5, 64), targets=torch.zeros(3, dtype=torch.int64))
        kw.update(bad)
        with pytest.raises(ValueError, match="score_reference"):
            score_reference(kw["x"], kw["w"], kw["targets"], 1.0)


def test_exact_data_is_exact_in_fp32_and_bf16():
    """the GPU test's exact data: x, w in {-1, 0, 1} and alpha = 2^-3 make every logit a multiple of 1/8 of magnitude <= C / 8 = 24: the
    fp32 product, under any summation order, and its bf16 rounding equal the float64 value"""
    g = torch.Generator().manual_seed(5)
    x = torch.randint(-1, 2, (33, 192), generator=g).float()
    w = torch.randint(-1, 2, (65576, 192), generator=g).float()
    z32 = 0.125 * (x @ w.t())
    z64 = 0.125 * (x.double() @ w.double().t())
    assert torch.equal(z32.double(), z64) and torch.equal(z32.to(torch.bfloat16).double(), z64) and z64.abs().max().item() <= 24
    lse32 = torch.logsumexp(z32, dim=1)
    assert (lse32.double() - torch.logsumexp(z64, dim=1)).abs().max().item() <= 8e-7                 # a plain fp32 evaluation of the normaliser


def test_random_data_stays_inside_the_looser_bound():
    """x ~ N(0, 1), w ~ 0.02 N(0, 1) in bf16 at C = 1024: the bf16-rounded fp32 product (torch's summation order, not the kernel's) stays
    within 0.72 of 2^-7 |z| plus twice the accumulation term — zbound itself is the worst case over orders, with room to spare"""
    g = torch.Generator().manual_seed(7)
    R, V, Cc = 64, 8192, 1024
    x = torch.randn(R, Cc, generator=g).to(torch.bfloat16)
    w = (0.02 * torch.randn(V, Cc, generator=g)).to(torch.bfloat16)
    _, _, _, zb = score_reference(x, w, torch.zeros(R, dtype=torch.int64), 1.0)
    z64 = x.double() @ w.double().t()
    z = (x.float() @ w.float().t()).to(torch.bfloat16).double()
    loose = 2.0 ** -7 * z64.abs() + 2 * (zb - 2.0 ** -8 * z64.abs())
    assert ((z - z64).abs() / loose).max().item() <= 0.72


# ----------------------------------------------------------------------------------------------- ops and the model
def test_ops_refuse_cpu_tensors_and_bad_shapes():
    from omnibiote_amd import ops
    x, w = torch.zeros(4, 64, dtype=torch.bfloat16), torch.zeros(10, 64, dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.readout_score(x, w, torch.zeros(4, dtype=torch.int64))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.readout_score(x, w, torch.zeros(4, 3, dtype=torch.int32), alpha=0.5, slices=3)
    with pytest.raises(ValueError, match="workspace"):
        ops.readout_score_workspace(4, 10, 65)


def _model(autoregressive, vocab=64, block=32):
    from omnibiote_amd.model import OmniBioTA, OmniBioTAConfig
    c = OmniBioTAConfig()
    c.block_size, c.vocab_size, c.n_layer, c.n_head, c.n_embd, c.dropout, c.flash = block, vocab, 1, 2, 128, 0.0, True
    c.autoregressive = autoregressive
    return OmniBioTA(c)


def test_score_validates_before_any_device_work():
    idx = torch.zeros(3, 8, dtype=torch.int64)
    with pytest.raises(ValueError, match="not autoregressive"):
        _model(False).score(idx)
    m = _model(True)
    for lengths, word in (([8, 1, 5], r"\[2, T = 8\]"), ([8, 9, 5], "every length"), ([0, 4, 5], "every length"), ([8, 8], "2 lengths"),
                          (7, "sequence of 3")):
        with pytest.raises(ValueError, match=word):
            m.score(idx, lengths)
    with pytest.raises(ValueError, match="T >= 2"):
        m.score(idx[:, :1])
    with pytest.raises(ValueError, match=r"\(B, T\)"):
        m.score(idx[0])
    for lengths in (None, [8, 2, 5], torch.tensor([2, 2, 8])):                    # valid: reaches the device requirement
        with pytest.raises(RuntimeError):
            m.score(idx, lengths)


def test_token_logprobs_validates_before_any_device_work():
    m = _model(False)
    idx = torch.zeros(2, 8, dtype=torch.int64)
    rows = torch.tensor([1, 9])
    for cand in (torch.zeros(2), torch.zeros(3, dtype=torch.int64), torch.zeros(2, 65, dtype=torch.int64), torch.zeros(2, 0, dtype=torch.int64),
                 torch.zeros(2, 2, 2, dtype=torch.int64), [0, 1]):
        with pytest.raises(ValueError, match="token_logprobs"):
            m.token_logprobs(idx, rows, cand)
    m.train()
    with pytest.raises(RuntimeError):                                            # valid: reaches the device requirement ...
        m.token_logprobs(idx, rows, torch.zeros(2, 4, dtype=torch.int64))
    assert m.training and all(mod.training for mod in m.modules())               # ... and leaves the modules' mode as it found it
