"""Host-side tests (no GPU) of encoder infilling (include/omnibiote_hip_fill.h): the symbol table against the header, the argument checks
that return before a launch, the noise rule and the loop's rules in plain torch (sampling.gumbel_noise, fill_schedule,
fill_commit_reference, readout_sample_reference), and the validation of OmniBioTA.sample_tokens and OmniBioTA.infill."""
import math
import os
import re

import pytest
import torch

from omnibiote_amd import _lib, sampling

EINVAL = -1
P = 4096   # a non-null, 16-byte aligned "pointer" for calls that must return before they touch it
NAMES = ("obte_readout_sample_slices", "obte_readout_sample_ws_bytes", "obte_readout_sample_bf16", "obte_fill_commit")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _err():
    return _lib.lib().obte_last_error().decode()


def test_fill_symbols_have_their_own_table():
    lib = _lib.lib()
    assert tuple(_lib.SYMBOLS_FILL) == NAMES
    header = open(os.path.join(ROOT, "include", "omnibiote_hip_fill.h")).read()
    assert tuple(re.findall(r"^(?:int|int32_t|int64_t|void|const char\*) +(obte_[a-z0-9_]+)\(", header, flags=re.M)) == NAMES   # in the header's order
    assert len(re.findall(r"^[a-z0-9_\* ]+\bobte_[a-z0-9_]+\(", header, flags=re.M)) == len(NAMES)                               # and nothing else
    assert '#include "omnibiote_hip.h"' in header and not re.search(r"\bstruct\b", header)
    others = (_lib.SYMBOLS, _lib.SYMBOLS_ROWS, _lib.SYMBOLS_SMALL_M, _lib.SYMBOLS_SAMPLE, _lib.SYMBOLS_EXTEND, _lib.SYMBOLS_SPEC, _lib.SYMBOLS_KV8,
              _lib.SYMBOLS_SHARED, _lib.SYMBOLS_LOOP, _lib.SYMBOLS_CONSTRAIN, _lib.SYMBOLS_W8, _lib.SYMBOLS_SCORE)
    for name in NAMES:
        for table in others:
            assert name not in table
        fn = getattr(lib, name)
        res, args = _lib.SYMBOLS_FILL[name]
        assert fn.restype is res and list(fn.argtypes) == args                                                                    # bound by lib()
    for name, (res, args) in _lib.SYMBOLS_FILL.items():                                                                           # as many arguments as declared
        decl = re.search(name + r"\(([^;]*)\);", header, flags=re.S).group(1)
        assert len(decl.split(",")) == len(args), name
    assert lib.obte_abi_version() == 1
    makefile = open(os.path.join(ROOT, "omnibiote_amd", "csrc", "Makefile")).read()
    assert "omnibiote_hip_fill.h" in makefile
    assert (_lib.SITE_FILL, sampling.SITE_FILL) == (8, 8) and "OBTE_SITE_FILL = 8" in header
    assert (_lib.FILL_CONFIDENCE, _lib.FILL_RANDOM, _lib.FILL_LEFT) == (0, 1, 2) and _lib.FILL_MAX_SEG == 8192


def test_sample_split_and_workspace():
    lib = _lib.lib()
    for R in (1, 129, 1024, 8192, 19200, 2 ** 31 - 1):
        for V in (1, 129, 1000, 65536):
            s = lib.obte_readout_sample_slices(R, V)
            tiles_m, tiles_n = (R + 127) // 128, (V + 127) // 128
            assert 1 <= s <= 64 and s <= tiles_n, (R, V, s)
            cost = {k: -(-tiles_m * k // 512) * -(-tiles_n // k) for k in range(1, min(64, tiles_n) + 1)}
            assert cost[s] == min(cost.values()) and all(cost[k] > cost[s] for k in range(1, s))                                      # the fewest among the best
            assert lib.obte_readout_sample_ws_bytes(R, V, 0) == lib.obte_readout_sample_ws_bytes(R, V, s) == 20 * R * s              # O(R slices)
    assert lib.obte_readout_sample_slices(1024, 65536) == lib.obte_readout_score_slices(1024, 65536) == 64
    assert lib.obte_readout_sample_slices(8192, 65536) == lib.obte_readout_score_slices(8192, 65536) == 8
    assert lib.obte_readout_sample_slices(19200, 65536) == 27                          # 150 row tiles: 8 rounds of 19 tiles, not 2 of 128
    for bad in ((0, 5, 1), (4, 0, 1), (4, 2 ** 31, 1), (4, 5, -1), (4, 5, 65)):
        assert lib.obte_readout_sample_ws_bytes(*bad) == -1
    assert lib.obte_readout_sample_slices(0, 5) == 1 and lib.obte_readout_sample_slices(5, 0) == 1


def _sample(x=P, ldx=64, w=P, ldw=64, R=4, V=100, Cc=64, alpha=1.0, inv_temp=1.0, seed=1, keys=P, allowed=None, allowed_ld=0, tokens=P, logprob=P, lse=P,
            slices=0, ws=P, ws_bytes=1 << 20):
    return _lib.lib().obte_readout_sample_bf16(x, ldx, w, ldw, R, V, Cc, alpha, inv_temp, seed, keys, allowed, allowed_ld, tokens, logprob, lse, slices, ws,
                                               ws_bytes, None)


@pytest.mark.parametrize("kw,word", [
    (dict(Cc=96, ldx=96, ldw=96), "C must"), (dict(V=0), "V must"), (dict(V=2 ** 31), "V must"), (dict(R=0), "R must"), (dict(ws_bytes=4 * 20 - 1), "ws_bytes"),
    (dict(slices=65), "slices"), (dict(ldx=68), "ldx"), (dict(ldw=56), "ldw"), (dict(x=None), "null"), (dict(w=None), "null"), (dict(tokens=None), "null"),
    (dict(logprob=None), "null"), (dict(lse=None), "null"), (dict(ws=None), "null"), (dict(inv_temp=-1.0), "inv_temp"), (dict(inv_temp=math.inf), "inv_temp"),
    (dict(inv_temp=math.nan), "inv_temp"), (dict(allowed=P, allowed_ld=-1), "allowed_ld"), (dict(allowed=P, allowed_ld=12), "allowed_ld"),
    (dict(x=P + 8), "x must be 16-byte"), (dict(ws=P + 4), "ws must be 8-byte"), (dict(keys=P + 4), "keys must be 8-byte"),
    (dict(tokens=P + 2), "tokens must be 4-byte"), (dict(logprob=P + 1), "logprob must be 4-byte"),
])
def test_sample_rejects_before_any_launch(kw, word):
    assert _sample(**kw) == EINVAL
    assert _err().startswith("obte_readout_sample_bf16:") and word in _err(), _err()


def _commit(rows=P, seg_off=P, n=4, B=2, max_seg=4, tokens=P, logprob=P, take=P, order=0, seed=1, idx=P, out_logprob=P, n_idx=16, rows_next=2 * P,
            seg_off_next=P, n_next=4):
    return _lib.lib().obte_fill_commit(rows, seg_off, n, B, max_seg, tokens, logprob, take, order, seed, idx, out_logprob, n_idx, rows_next, seg_off_next,
                                       n_next, None)


@pytest.mark.parametrize("kw,word", [
    (dict(rows=None), "null"), (dict(take=None), "null"), (dict(rows_next=None), "null"), (dict(B=0), "B must"), (dict(n=-1), "n and n_next"),
    (dict(n_idx=0), "n_idx"), (dict(max_seg=8193), "max_seg"), (dict(max_seg=-1), "max_seg"), (dict(order=3), "order"), (dict(order=-1), "order"),
    (dict(rows_next=P), "rows_next must not be rows"), (dict(rows=P + 4), "rows must be 8-byte"), (dict(idx=P + 4), "idx must be 8-byte"),
    (dict(take=P + 2), "take must be 4-byte"), (dict(out_logprob=P + 1), "out_logprob must be 4-byte"),
])
def test_commit_rejects_before_any_launch(kw, word):
    assert _commit(**kw) == EINVAL
    assert _err().startswith("obte_fill_commit:") and word in _err(), _err()


# ----------------------------------------------------------------------------------------------- the noise rule
def _hash32(x):
    x &= 0xFFFFFFFF
    x ^= x >> 16; x = (x * 0x7FEB352D) & 0xFFFFFFFF
    x ^= x >> 15; x = (x * 0x846CA68B) & 0xFFFFFFFF
    return x ^ (x >> 16)


def test_gumbel_noise_is_finite_at_both_ends_and_matches_a_hand_computation():
    g = sampling.gumbel_of_hash(torch.tensor([0, 2 ** 32 - 1, 2 ** 31]))
    assert bool(torch.isfinite(g).all())
    # h = 0: w = 2^-33, E = w (1 + w / 2 + ...), g = 33 ln 2 - ln(1 + 2^-34 + ...); h = 2^32 - 1: 1 - w = 2^-33, E = 33 ln 2, g = -ln(33 ln 2)
    assert abs(g[0].item() - 33 * math.log(2)) <= 1e-9 and abs(g[1].item() + math.log(33 * math.log(2))) <= 1e-12
    assert abs(g[2].item() + math.log(-math.log(0.5 - 2.0 ** -33))) <= 1e-12
    # one fixed (seed, key, v) in plain integers: make_drop's two words, drop_rowkey, the column's hash, the rule
    seed, key, v, site = 0x0123456789ABCDEF, (5 << 32) + 77, 41, 8
    s0 = (seed & 0xFFFFFFFF) ^ ((site * 0x632BE5AB) & 0xFFFFFFFF)
    s1 = ((seed >> 32) + site * 0x9E3779B9) & 0xFFFFFFFF
    rowkey = _hash32((_hash32((key & 0xFFFFFFFF) ^ s0) + ((key >> 32) * 0x9E3779B1) + s1) & 0xFFFFFFFF)
    h = _hash32(rowkey ^ v)
    want = -math.log(-math.log1p(-(h + 0.5) * 2.0 ** -32))
    got = sampling.gumbel_noise(seed, torch.tensor([3, key]), 64)
    assert got.shape == (2, 64) and got.dtype == torch.float64
    assert abs(got[1, v].item() - want) <= 1e-12 * max(1.0, abs(want)), (got[1, v].item(), want)
    assert sampling.GUMBEL_EPS <= 2.0 ** -10
    # the noise is Gumbel: mean = Euler's constant, variance = pi^2 / 6, over 2^20 values
    big = sampling.gumbel_noise(7, torch.arange(16), 65536)
    assert abs(big.mean().item() - 0.5772156649) <= 5e-3 and abs(big.var().item() - math.pi ** 2 / 6) <= 2e-2
    assert not torch.equal(big[0], big[1]) and not torch.equal(big[:1], sampling.gumbel_noise(8, torch.arange(1), 65536))
    with pytest.raises(ValueError, match="gumbel_noise"):
        sampling.gumbel_noise(1, torch.zeros(2, 2, dtype=torch.int64), 5)


def test_readout_sample_reference_draws_from_the_softmax():
    g = torch.Generator().manual_seed(11)
    V, n = 6, 40000
    x = torch.randint(-1, 2, (1, 64), generator=g).float()
    w = torch.randint(-1, 2, (V, 64), generator=g).float()
    allowed = torch.tensor([True, True, False, True, True, True])
    tok, lp, lse, pert, y = sampling.readout_sample_reference(x.expand(n, 64), w, 0.7, 5, keys=torch.arange(n), allowed=allowed, alpha=0.125)
    assert tok.dtype == torch.int64 and lp.dtype == lse.dtype == pert.dtype == torch.float64 and pert.shape == (n, V)
    z = 0.125 * (x.double() @ w.double().t())[0]
    it = sampling.inv_temperature(0.7)
    assert it == float(torch.tensor(1 / 0.7).float()) and torch.equal(y[0][allowed], (z * it)[allowed]) and y[0, 2] == -math.inf
    p = torch.softmax(y[0], dim=0)
    assert p[2] == 0 and not bool((tok == 2).any())
    counts = torch.bincount(tok, minlength=V).double()
    chi2 = (((counts - n * p) ** 2) / (n * p))[allowed].sum().item()
    assert chi2 <= (V - 2) + 6 * math.sqrt(2 * (V - 2)), chi2
    assert torch.equal(lp, (y - lse.unsqueeze(1)).gather(1, tok.unsqueeze(1)).squeeze(1))
    # greedy: the first index of the maximum, lse and logprob at temperature 1; a row that allows nothing
    tok0, lp0, lse0, _, y0 = sampling.readout_sample_reference(x, w, 0, 5, alpha=0.125)
    assert tok0.item() == int(torch.where(z == z.max())[0][0]) and torch.equal(y0[0], z) and abs(lse0.item() - torch.logsumexp(z, 0).item()) <= 1e-12
    none = sampling.readout_sample_reference(x, w, 1.0, 5, allowed=torch.zeros(V, dtype=torch.bool), alpha=0.125)
    assert none[0].item() == -1 and none[1].item() == -math.inf and none[2].item() == -math.inf
    for bad in (-1.0, math.inf, math.nan, 1e-40):
        with pytest.raises(ValueError, match="temperature"):
            sampling.inv_temperature(bad)


# ----------------------------------------------------------------------------------------------- the loop's rules
def test_fill_schedule_properties():
    for m in (0, 1, 2, 7, 40, 300):
        for steps in (1, 2, 3, 4, 7, 100, 301):
            sch = sampling.fill_schedule(m, steps)
            assert len(sch) == steps and sum(sch) == m and all(a >= b for a, b in zip(sch, sch[1:])) and all(k >= 0 for k in sch)
            rem = m
            for s, k in enumerate(sch):
                assert k == -(-rem // (steps - s))
                rem -= k
            if steps > m:
                assert sch == [1] * m + [0] * (steps - m)
    assert sampling.fill_schedule(10, 4) == [3, 3, 2, 2] and sampling.fill_schedule(5, 1) == [5]
    for bad in ((-1, 2), (3, 0), (3.0, 2), (3, True)):
        with pytest.raises(ValueError, match="fill_schedule"):
            sampling.fill_schedule(*bad)
    assert sampling.fill_iteration_seed(9, 0) == 9 and sampling.fill_iteration_seed(2 ** 64 - 1, 1) == 0x9E3779B97F4A7C14
    assert len({sampling.fill_iteration_seed(9, s) for s in range(100)}) == 100


def test_fill_commit_reference_on_ties_and_edge_takes():
    T = 10
    rows = torch.tensor([1, 3, 4, 8, 12, 15, 16, 27])                      # sequence 0: 4 entries, 1: 3 entries, 2: 1 entry, 3: none
    seg = [0, 4, 7, 8, 8]
    tokens = torch.arange(100, 108)
    lp = torch.tensor([-1.0, -0.5, -0.5, float("nan"), -2.0, -2.0, -2.0, -0.25])
    idx = torch.zeros(4 * T, dtype=torch.int64)
    out = torch.zeros(4 * T)

    def run(take, order, seed=3):
        nxt = [0]
        for b in range(4):
            nb = seg[b + 1] - seg[b]
            nxt.append(nxt[-1] + nb - (take[b] if 0 <= take[b] <= nb else 0))
        return sampling.fill_commit_reference(rows, seg, tokens, lp, take, order, seed, idx, out, nxt), nxt

    (i2, o2, nx), off = run([2, 1, 1, 0], "confidence")
    assert off == [0, 2, 4, 4, 4] and nx.tolist() == [1, 8, 15, 16]       # -0.5 twice: both; -2 three times: the lowest position; NaN last
    assert i2[3] == 101 and i2[4] == 102 and i2[12] == 104 and i2[27] == 107 and int((i2 != 0).sum()) == 4
    assert o2[3] == -0.5 and o2[12] == -2.0 and o2[27] == -0.25 and int((o2 != 0).sum()) == 4
    (i2, o2, nx), off = run([1, 0, 0, 0], "confidence")
    assert i2[3] == 101 and int((i2 != 0).sum()) == 1 and nx.tolist() == [1, 4, 8, 12, 15, 16, 27]   # the tie at the top: the lower position
    (i2, o2, nx), off = run([4, 3, 1, 0], "confidence")                     # take = n_b: everything, NaN included
    assert nx.numel() == 0 and int((i2 != 0).sum()) == 8 and math.isnan(o2[8])
    (i2, o2, nx), off = run([5, -1, 2, 1], "left")                         # outside [0, n_b]: a no-op, everything copied
    assert torch.equal(i2, idx) and torch.equal(o2, out) and torch.equal(nx, rows)
    (i2, o2, nx), off = run([3, 2, 0, 0], "left")
    assert nx.tolist() == [8, 16, 27] and i2[1] == 100 and i2[4] == 102 and i2[15] == 105
    (i2, o2, nx), off = run([2, 2, 1, 0], "random")
    key = sampling._rowkey(rows, 3)
    for b in range(3):
        k = key[seg[b]:seg[b + 1]]
        first = torch.sort(k, stable=True).indices[:[2, 2, 1][b]]
        assert all(i2[rows[seg[b] + int(j)]] == tokens[seg[b] + int(j)] for j in first)
    assert nx.tolist() == sorted(nx.tolist()) and nx.numel() == 3
    a = run([2, 2, 1, 0], "random", seed=4)[0][2]
    b_ = run([2, 2, 1, 0], "random", seed=5)[0][2]
    c = run([2, 2, 1, 0], "random", seed=6)[0][2]
    assert not (torch.equal(a, nx) and torch.equal(b_, nx) and torch.equal(c, nx))     # the seed matters
    with pytest.raises(ValueError, match="order"):
        run([0, 0, 0, 0], "best")


# ----------------------------------------------------------------------------------------------- ops and the model
def test_ops_refuse_cpu_tensors_and_bad_arguments():
    from omnibiote_amd import ops
    x, w = torch.zeros(4, 64, dtype=torch.bfloat16), torch.zeros(10, 64, dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.readout_sample(x, w, 1.0, 3)
    with pytest.raises(ValueError, match="workspace"):
        ops.readout_sample_workspace(4, 10, 65)
    with pytest.raises(ValueError, match="order"):
        ops.fill_commit(*([torch.zeros(1)] * 5), "best", 1, *([torch.zeros(1)] * 4), 4)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.fill_commit(*([torch.zeros(1, dtype=torch.int64)] * 5), "left", 1, *([torch.zeros(1)] * 4), 4)


def _model(vocab=64, block=32):
    from omnibiote_amd.model import OmniBioTA, OmniBioTAConfig
    c = OmniBioTAConfig()
    c.block_size, c.vocab_size, c.n_layer, c.n_head, c.n_embd, c.dropout, c.flash = block, vocab, 1, 2, 128, 0.0, True
    return OmniBioTA(c)


def test_infill_and_sample_tokens_validate_before_any_device_work():
    m = _model()
    idx = torch.zeros(2, 8, dtype=torch.int64)
    masked = torch.zeros(2, 8, dtype=torch.bool)
    masked[0, 3] = masked[1, 5] = True
    rows = torch.tensor([3, 13])
    bad_infill = [
        (dict(idx=idx[0]), r"\(B, T\)"), (dict(idx=idx.float()), r"\(B, T\)"), (dict(idx=torch.zeros(2, 33, dtype=torch.int64)), "block size"),
        (dict(masked=masked[:, :7]), "masked"), (dict(masked=masked.long()), "masked"), (dict(steps=0), "steps"), (dict(steps=1.5), "steps"),
        (dict(temperature=-0.5), "temperature"), (dict(temperature=math.nan), "temperature"), (dict(allowed_tokens=[]), "empty"),
        (dict(allowed_tokens=torch.zeros(64, dtype=torch.bool)), "empty"), (dict(allowed_tokens=[64]), "allowed_tokens"),
        (dict(allowed_tokens=torch.ones(63, dtype=torch.bool)), "allowed_tokens"), (dict(masked=torch.zeros(2, 8, dtype=torch.bool)), "nothing is masked"),
        (dict(order="best"), "order"), (dict(seed=-1), "seed"), (dict(seed=2 ** 64), "seed"), (dict(mask_token=64), "mask_token"),
    ]
    for kw, word in bad_infill:
        args = dict(idx=idx, masked=masked)
        args.update(kw)
        with pytest.raises(ValueError, match=word):
            m.infill(**args)
    bad_sample = [
        (dict(idx=idx[0]), r"\(B, T\)"), (dict(rows=torch.zeros(0, dtype=torch.int64)), "rows"), (dict(rows=rows.float()), "rows"),
        (dict(rows=rows.view(1, 2)), "rows"), (dict(temperature=-1), "temperature"), (dict(allowed_tokens=[]), "empty"), (dict(seed=1.5), "seed"),
        (dict(allowed_tokens=[-1]), "allowed_tokens"),
    ]
    for kw, word in bad_sample:
        args = dict(idx=idx, rows=rows)
        args.update(kw)
        with pytest.raises(ValueError, match=word):
            m.sample_tokens(**args)
    m.train()
    for call in (lambda: m.infill(idx, masked, steps=3, order="random", allowed_tokens=[4, 5], seed=7),
                 lambda: m.sample_tokens(idx, rows, temperature=0, allowed_tokens=torch.ones(64, dtype=torch.bool))):
        with pytest.raises(RuntimeError):                                        # valid: reaches the device requirement ...
            call()
    assert m.training and all(mod.training for mod in m.modules())               # ... and leaves the modules' mode as it found it
