"""Beam search on the GPU (include/omnibiote_hip_beam.h): obte_beam_select_bf16 against the float64 rule (sampling.beam_step_reference) —
parents, tokens, done flags, ancestry and token history exactly, scores within eps = 1e-5 + 2^-23 |S| (the bar readout_score holds for
its lse against float64, plus one fp32 rounding of the sum) — exact ties, repeatability, guard bands; obte_attn_decode_beam bit for bit
against obte_attn_decode_shared (the identity table; a valid table against the physically gathered suffix cache) and against float64 with
entries that name no row, at tests/test_hip_shared.py's bars (attention 2^-7 |ref| + 6e-3, lse atol 2e-3 / rtol 1e-3);
obte_block_decode_beam against obte_block_decode_shared; OmniBioTA.generate_beam against generate and model.score."""
import math

import pytest
import torch

from fenced import assert_guards, assert_same_bits, fenced, filled
from omnibiote_amd.sampling import beam_step_reference, pack_token_mask
from test_hip_generate import L, _block_setup, _gen_case, ops
from test_hip_ops import BF, DEV, close, rnd

pytestmark = pytest.mark.gpu

INF = float("inf")
T_SUF, SLOT = 6, 3            # the selection tests' ancestry tables: 6 slots, the step writes slot 3
POISON32 = 0x12341234


def _eps(s):
    return 1e-5 + 2.0 ** -23 * abs(s)


# =================================================================================================== the selection
# The seed of every case: the first for which the REFERENCE ALONE shows that the device can be held to exact equality — found on the CPU
# with _margins_ok below, which the test asserts again.  (V, W, P, masked) -> seed; a case not listed uses 0.
SEEDS = {(4104, 5, 1, False): 1}


def _inputs(V, W, Pn, masked, seed):
    """randn * 2 logits in bf16 with a few NaN and -inf entries, rows that are live (about 60 %), done and dead, a per-row mask or none"""
    g = torch.Generator().manual_seed(1000 * seed + 7 * V + 3 * W + Pn + (500 if masked else 0))
    B = Pn * W
    logits = (torch.randn(B, V, generator=g) * 2).to(BF)
    holes = torch.rand(B, V, generator=g)
    logits[holes < 0.01] = float("nan")
    logits[(holes >= 0.01) & (holes < 0.02)] = -INF
    state = torch.rand(B, generator=g)
    score = -3 * torch.rand(B, generator=g)
    done = ((state > 0.6) & (state <= 0.8)).to(torch.uint8)
    score[state > 0.8] = -INF
    if B > 2:
        score[1] = float("nan")                                                     # a NaN score counts as dead
    allowed = (torch.rand(B, V, generator=g) < 0.5) if masked else None
    anc = torch.randint(0, W, (B, T_SUF), generator=g, dtype=torch.int32)
    return dict(logits=logits, score=score, done=done, allowed=allowed, anc=anc, eos=V // 2)


_refs = {}


def _reference(V, W, Pn, masked):
    key = (V, W, Pn, masked)
    if key not in _refs:
        c = _inputs(V, W, Pn, masked, SEEDS.get(key, 0))
        c["ref"] = beam_step_reference(c["logits"], c["score"], c["done"], c["anc"], SLOT, W, eos_token=c["eos"], allowed=c["allowed"])
        _refs[key] = c
    return _refs[key]


def _margins_ok(ref, W):
    """Inside every group: the W-th and the (W + 1)-th candidate lie more than 4 eps apart, and so do two neighbours among the first W
    unless they are an exact tie of one beam (the same row, the same bf16 value: the same S on the device too, ordered by token)."""
    parent, ranked = ref[0], ref[5]
    for p, vals in enumerate(ranked):
        vals = vals.tolist()
        for r in range(min(len(vals), W + 1) - 1):
            gap = vals[r] - vals[r + 1]
            if gap > 4 * _eps(vals[r + 1]):
                continue
            if r + 1 < W and gap == 0.0 and parent[p * W + r] == parent[p * W + r + 1]:
                continue
            return False
    return True


def _run_select(c, W, ld=None, **kw):
    """the call on fresh device copies; returns (parent, token, score, done, ancestry_out, token_hist) on the CPU"""
    o = ops()
    B, V = c["logits"].shape
    if ld is None:                                                                   # rows of 16 bytes: the row stride is V rounded up to 8
        logits = torch.zeros((B, (V + 7) // 8 * 8), dtype=BF, device=DEV)[:, :V]
        logits.copy_(c["logits"])
    else:
        logits = fenced(c["logits"], poison="nan", ld=ld)[0]
    packed = None if c["allowed"] is None else pack_token_mask(c["allowed"]).to(DEV)
    anc_out = filled((B, T_SUF), torch.int32, POISON32)
    hist = filled((T_SUF, B), torch.int64, "mark")
    parent, token, score, done = o.beam_select(logits, c["score"].to(DEV), c["done"].to(DEV), c["anc"].to(DEV), anc_out, hist, SLOT, W, eos_token=c["eos"],
                                               allowed_packed=packed, **kw)
    return [t.cpu() for t in (parent, token, score, done, anc_out, hist)]


def _raw(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def _check_against(got, ref, W, what):
    parent, token, score, done, anc_out, hist = got
    rp, rt, rs, rd, ra, _ = ref
    assert torch.equal(parent.long(), rp), (what, parent.tolist(), rp.tolist())
    assert torch.equal(token, rt), (what, token.tolist(), rt.tolist())
    assert torch.equal(done.bool(), rd), what
    assert torch.equal(anc_out[:, :SLOT + 1].long(), ra), what
    assert (anc_out[:, SLOT + 1:] == POISON32).all(), f"{what}: ancestry entries behind the slot were written"
    assert torch.equal(hist[SLOT], rt) and (hist[:SLOT] == 0x1234123412341234).all() and (hist[SLOT + 1:] == 0x1234123412341234).all(), what
    worst = 0.0
    for b in range(rs.numel()):
        s = rs[b].item()
        if s == -INF:
            assert score[b].item() == -INF, (what, b)
        else:
            err = abs(score[b].double().item() - s)
            worst = max(worst, err / _eps(s))
            assert err <= _eps(s), (what, b, score[b].item(), s)
    return worst


@pytest.mark.parametrize("Pn", [1, 3])
@pytest.mark.parametrize("W", [1, 2, 5, 32])
@pytest.mark.parametrize("V", [5, 100, 4104, 65536])
def test_beam_select_against_the_float64_rule(V, W, Pn):
    ld = (V + 7) // 8 * 8 + 8                                                        # ld > V: the columns behind the row hold NaN
    for masked in (False, True):
        c = _reference(V, W, Pn, masked)
        assert _margins_ok(c["ref"], W), "the case's seed does not separate the reference's candidates: choose another (SEEDS)"
        got = _run_select(c, W, ld=ld)
        worst = _check_against(got, c["ref"], W, (V, W, Pn, masked))
        print(f"beam_select V={V} W={W} P={Pn} masked={masked}: worst score error / eps {worst:.3f}")
        again = _run_select(c, W, ld=ld)
        assert all(torch.equal(_raw(a), _raw(b)) for a, b in zip(got, again)), "two calls, other bytes"


def test_exact_ties_resolve_by_beam_then_token():
    """two live beams with equal scores and identical rows, equal bf16 logits inside the row: (beam, token) decides; a third beam below them"""
    W, V = 4, 100
    row = torch.zeros(V)
    row[[7, 20, 63]] = 3.0                                                           # three equal maxima
    row[[5, 90]] = 2.5
    logits = torch.stack([row, row, row - 1.0, row]).to(BF)
    c = dict(logits=logits, score=torch.tensor([-1.0, -1.0, -1.5, -INF]), done=torch.zeros(4, dtype=torch.uint8), allowed=None,
             anc=torch.zeros(4, T_SUF, dtype=torch.int32), eos=0)
    ref = beam_step_reference(c["logits"], c["score"], c["done"], c["anc"], SLOT, W, eos_token=0)
    assert ref[0].tolist() == [0, 0, 0, 1] and ref[1].tolist() == [7, 20, 63, 7]
    _check_against(_run_select(c, W), ref, W, "ties")
    row2 = torch.zeros(V)                                                            # one beam, a tie wider than W at the threshold: the lowest columns
    c2 = dict(logits=torch.stack([row2] * 4).to(BF), score=torch.tensor([0.0, -INF, -INF, -INF]), done=torch.zeros(4, dtype=torch.uint8), allowed=None,
              anc=torch.zeros(4, T_SUF, dtype=torch.int32), eos=None)
    ref2 = beam_step_reference(c2["logits"], c2["score"], c2["done"], c2["anc"], SLOT, W)
    assert ref2[1].tolist() == [0, 1, 2, 3]
    _check_against(_run_select(c2, W), ref2, W, "a tie wider than W")


@pytest.mark.parametrize("V,W", [(100, 5), (65536, 32), (4104, 2)])
def test_a_group_has_the_same_bits_at_every_prompt_count(V, W):
    c = _reference(V, W, 3, True)
    whole = _run_select(c, W)
    for p in range(3):
        rows = slice(p * W, (p + 1) * W)
        sub = dict(logits=c["logits"][rows], score=c["score"][rows], done=c["done"][rows], allowed=c["allowed"][rows], anc=c["anc"][rows], eos=c["eos"])
        part = _run_select(sub, W)
        assert torch.equal(part[0] + p * W, whole[0][rows]) and torch.equal(part[1], whole[1][rows])
        assert torch.equal(part[2].view(torch.int32), whole[2][rows].view(torch.int32)) and torch.equal(part[3], whole[3][rows])
        assert torch.equal(part[4], whole[4][rows]) and torch.equal(part[5], whole[5][:, rows])


@pytest.mark.parametrize("V,W,Pn", [(100, 5, 3), (4104, 32, 1), (65536, 2, 3)])
def test_beam_select_stays_inside_its_buffers(V, W, Pn):
    """every operand in a poisoned buffer that starts 16 bytes behind a 512-byte boundary: logits with NaN behind every row, the ancestry
    input with poison behind the slot, the workspace exactly the bytes asked for; a row of NaN and a row of -inf propose nothing"""
    o = ops()
    c = dict(_reference(V, W, Pn, True))
    B = Pn * W
    logits = c["logits"].clone()
    logits[0] = float("nan")
    logits[B - 1] = -INF
    c["logits"] = logits
    ref = beam_step_reference(logits, c["score"], c["done"], c["anc"], SLOT, W, eos_token=c["eos"], allowed=c["allowed"])
    plain = _run_select(c, W)
    for b in (0, B - 1):                                                             # a live row of NaN or of -inf proposes nothing
        if math.isfinite(c["score"][b].item()) and not c["done"][b]:
            assert not (plain[0][plain[2] > -INF] == b).any(), b
    ld = (V + 7) // 8 * 8 + 16
    fl, hl = fenced(logits, poison="nan", ld=ld)
    fs, hs_ = fenced(c["score"], poison="nan")
    fd, hd = fenced(c["done"], poison="mark")
    anc_in = c["anc"].clone()
    anc_in[:, SLOT:] = POISON32                                                      # entries j >= slot of the input are not read
    fa, ha = fenced(anc_in, poison=POISON32)
    fm, hm = fenced(pack_token_mask(c["allowed"]), poison="mark")
    fao, hao = fenced((B, T_SUF), torch.int32, POISON32)
    fh, hh = fenced((T_SUF, B), torch.int64, "mark")
    fp, hp = fenced((B,), torch.int32, "mark")
    ft, ht = fenced((B,), torch.int64, "mark")
    fso, hso = fenced((B,), torch.float32, "mark")
    fdo, hdo = fenced((B,), torch.uint8, "mark")
    fw, hw = fenced((int(L().lib().obte_beam_select_ws_bytes(Pn, W)),), torch.uint8, "mark")
    o.beam_select(fl, fs, fd, fa, fao, fh, SLOT, W, eos_token=c["eos"], allowed_packed=fm, parent=fp, token=ft, score_out=fso, done_out=fdo, ws=fw)
    torch.cuda.synchronize()
    got = [t.cpu() for t in (fp, ft, fso, fdo, fao, fh)]
    for a, b, name in zip(got, plain, ("parent", "token", "score", "done")):
        assert_same_bits(a, b, name)
    assert torch.equal(got[4][:, :SLOT + 1], plain[4][:, :SLOT + 1]) and (got[4][:, SLOT + 1:] == POISON32).all()
    assert torch.equal(got[5][SLOT], plain[5][SLOT])
    assert (got[5][:SLOT] == 0x1234123412341234).all() and (got[5][SLOT + 1:] == 0x1234123412341234).all()
    assert_guards(hl, hs_, hd, ha, hm, hao, hh, hp, ht, hso, hdo, hw)
    if _margins_ok(ref, W):
        _check_against(plain, ref, W, "with a NaN row and a -inf row")


# =================================================================================================== the attention
A_PRE, A_SUF, A_P, A_H = 130, 300, 2, 2
SPLITS = ((0, 0), (3, 2), (1, 1), (2, 7))
_acases = {}


def _cache_of(k, v):
    return torch.stack([k, v]).contiguous().view(-1).to(DEV)


def _acase(hs, G):
    key = (hs, G)
    if key not in _acases:
        B = A_P * G
        c = dict(q=rnd(B, A_H * hs, seed=hs + G), kp=rnd(A_P, A_H, A_PRE, hs, seed=2), vp=rnd(A_P, A_H, A_PRE, hs, seed=3),
                 ks=rnd(B, A_H, A_SUF, hs, seed=4), vs=rnd(B, A_H, A_SUF, hs, seed=5))
        g = torch.Generator().manual_seed(hs * 100 + G)
        c["table"] = torch.randint(0, G, (B, A_SUF), generator=g, dtype=torch.int32)
        src = (torch.arange(B) // G * G).view(B, 1) + c["table"].long()                                  # (B, T): the row that slot j of row b is read from
        idx = src.view(B, 1, A_SUF, 1).expand(B, A_H, A_SUF, hs)
        c["ks_g"], c["vs_g"] = c["ks"].gather(0, idx), c["vs"].gather(0, idx)
        c["identity"] = (torch.arange(B, dtype=torch.int32) % G).view(B, 1).expand(B, A_SUF).contiguous()
        c["prefix"], c["suffix"], c["suffix_g"] = _cache_of(c["kp"], c["vp"]), _cache_of(c["ks"], c["vs"]), _cache_of(c["ks_g"], c["vs_g"])
        _acases[key] = c
    return _acases[key]


def _bits(t):
    return t.view(torch.int16) if t.dtype == BF else t.view(torch.int32)


def _same(a, b):
    return torch.equal(_bits(a[0]), _bits(b[0])) and torch.equal(_bits(a[1]), _bits(b[1]))


def _shared(c, hs, G, n_suffix, splits, suffix):
    return ops().attn_decode_shared(c["q"].to(DEV), c["prefix"], A_P, A_PRE, A_PRE, suffix, G, A_SUF, n_suffix, A_H, hs, 8.0 / (A_H * hs), prefix_splits=splits[0],
                                    suffix_splits=splits[1])


def _beam(c, hs, G, n_suffix, splits, table, suffix=None, **kw):
    return ops().attn_decode_beam(c["q"].to(DEV), c["prefix"], A_P, A_PRE, A_PRE, c["suffix"] if suffix is None else suffix, G, A_SUF, n_suffix, table, A_H, hs,
                                  8.0 / (A_H * hs), prefix_splits=splits[0], suffix_splits=splits[1], **kw)


@pytest.mark.parametrize("n_suffix", [0, 1, 63, 65, 300])
@pytest.mark.parametrize("G", [1, 5, 32, 33])
@pytest.mark.parametrize("hs", [64, 128])
def test_attn_decode_beam_bit_for_bit(hs, G, n_suffix):
    """the identity table: obte_attn_decode_shared's bits; a random valid table: its bits on the physically gathered suffix cache; slots and
    table entries at j >= n_suffix hold NaN / poison"""
    c = _acase(hs, G)
    B = A_P * G
    stale = c["suffix"].clone()
    stale.view(torch.int16).view(2, B, A_H, A_SUF, hs)[:, :, :, n_suffix:] = 0x7FC0
    for splits in SPLITS:
        want = _shared(c, hs, G, n_suffix, splits, c["suffix"])
        assert _same(_beam(c, hs, G, n_suffix, splits, c["identity"].to(DEV)), want), ("identity", splits)
        table = c["table"].clone()
        table[:, n_suffix:] = POISON32
        got = _beam(c, hs, G, n_suffix, splits, table.to(DEV), suffix=stale)
        assert torch.isfinite(got[0]).all() and torch.isfinite(got[1]).all()
        assert _same(got, _shared(c, hs, G, n_suffix, splits, c["suffix_g"])), ("gathered", splits)
        assert _same(got, _beam(c, hs, G, n_suffix, splits, table.to(DEV), suffix=stale)), "two calls, other bytes"


@pytest.mark.parametrize("G,n_suffix", [(1, 1), (5, 63), (32, 65), (33, 300)])
@pytest.mark.parametrize("hs", [64, 128])
def test_entries_that_name_no_row_contribute_nothing(hs, G, n_suffix):
    """a third of the entries are -1, G, INT_MIN or INT_MAX (row 1: every one of them): float64 softmax over the remaining keys; q, both
    caches, the table, o, lse and the workspace inside guard bands, the caches' poison NaN — an address formed from such an entry would
    show as NaN or as a wrong value"""
    o = ops()
    c = _acase(hs, G)
    B, scale = A_P * G, 8.0 / (A_H * hs)
    g = torch.Generator().manual_seed(G)
    table = c["table"][:, :n_suffix].clone()
    bad = torch.rand(B, n_suffix, generator=g) < 0.33
    if B > 1:
        bad[1] = True
    junk = torch.tensor([-1, G, -2 ** 31, 2 ** 31 - 1], dtype=torch.int32)[torch.randint(0, 4, (B, n_suffix), generator=g)]
    table = torch.where(bad, junk, table)
    k = torch.cat([c["kp"].repeat_interleave(G, 0), c["ks_g"][:, :, :n_suffix]], dim=2).double()
    v = torch.cat([c["vp"].repeat_interleave(G, 0), c["vs_g"][:, :, :n_suffix]], dim=2).double()
    s = torch.einsum("bhd,bhtd->bht", c["q"].view(B, A_H, hs).double(), k) * scale
    s[:, :, A_PRE:] = s[:, :, A_PRE:].masked_fill(bad.view(B, 1, n_suffix), -INF)
    ref_o = torch.einsum("bht,bhtd->bhd", torch.softmax(s, dim=-1), v).reshape(B, A_H * hs)
    ref_lse = torch.logsumexp(s, dim=-1)
    fq, hq = fenced(c["q"], poison="nan", ld=3 * A_H * hs)
    fp, hp = fenced(c["prefix"], poison="nan")
    fs, hsuf = fenced(_cache_of(c["ks"][:, :, :n_suffix], c["vs"][:, :, :n_suffix]), poison="nan")
    ft, htab = fenced(table, poison=POISON32)
    for splits in SPLITS:
        fo, ho = fenced((B, A_H * hs), BF, "mark")
        fl, hl = fenced((B, A_H), torch.float32, "mark")
        fw, hw = fenced((int(L().lib().obte_attn_decode_shared_ws_bytes(A_P, G, A_H, hs, *splits)),), torch.uint8, "mark")
        got, lse = o.attn_decode_beam(fq, fp, A_P, A_PRE, A_PRE, fs, G, n_suffix, n_suffix, ft, A_H, hs, scale, prefix_splits=splits[0], suffix_splits=splits[1],
                                      q_ld=3 * A_H * hs, ws=fw, out=fo, lse=fl)
        torch.cuda.synchronize()
        close(got, ref_o, atol=6e-3, what=f"attn_decode_beam {(hs, G, n_suffix, splits)}")
        close(lse, ref_lse, atol=2e-3, rtol=1e-3, what=f"lse {(hs, G, n_suffix, splits)}")
        assert_guards(hq, hp, hsuf, htab, ho, hl, hw)
        if B > 1:                                                                    # row 1 has no suffix key left: the prefix alone, bit for bit
            alone = o.attn_decode_shared(c["q"].to(DEV), c["prefix"], A_P, A_PRE, A_PRE, None, G, 0, 0, A_H, hs, scale, prefix_splits=splits[0])
            assert torch.equal(_bits(got[1]), _bits(alone[0][1])) and torch.equal(_bits(lse[1]), _bits(alone[1][1]))


# =================================================================================================== the block
@pytest.mark.parametrize("C,H", [(128, 2), (256, 2)])
def test_block_decode_beam_with_the_identity_table_is_block_decode_shared(C, H):
    T0, T, Pn, G, steps = 37, 48, 2, 3, 4
    c = _block_setup(C, H, T)
    o, hs, B = c["o"], C // H, Pn * G
    x0 = c["x"][:, :T0].contiguous().to(DEV)
    xs = rnd(steps, B, C, seed=C).to(DEV)
    prefix = o.kv_cache_buffer(Pn, T0, H, hs, DEV)
    o.block_prefill(x0, c["params"], c["rope"], H, c["causal"](T0), prefix, T0)
    table = filled((B, steps), torch.int32, POISON32)
    suf_a, suf_b = o.kv_cache_buffer(B, steps, H, hs, DEV), o.kv_cache_buffer(B, steps, H, hs, DEV)
    for s in (suf_a, suf_b):
        s.view(torch.int16).fill_(0x7FC0)
    ws = o.block_decode_beam_workspace(Pn, G, C, H, DEV)
    for i in range(steps):
        table[:, i] = torch.arange(B, dtype=torch.int32, device=DEV) % G             # column i names the row itself; the columns behind it stay poison
        want = o.block_decode_shared(xs[i], c["params"], c["rope"], H, prefix, Pn, T0, T0, suf_a, steps, i)
        got = o.block_decode_beam(xs[i], c["params"], c["rope"], H, prefix, Pn, T0, T0, suf_b, steps, i, table, ws=ws)
        assert torch.isfinite(got).all() and torch.equal(_bits(got), _bits(want)), i
    assert torch.equal(suf_a.view(torch.int16), suf_b.view(torch.int16))


# =================================================================================================== the model
def _delta(m, idx, n):
    """The largest |log-softmax of decode_step's logits at the chosen token - model.score's value| over a greedy run of n tokens on the
    shared-prefix cache with one row per prompt: how far two unchanged paths to one log-probability lie apart"""
    from omnibiote_amd.model import SharedPrefixCache
    Pn, T0 = idx.shape
    cache = SharedPrefixCache(m, Pn, 1, T0, n)
    logits, toks, lps = m.prefill(idx, cache), [], []
    for i in range(n):
        lp = torch.log_softmax(logits.float(), dim=-1)
        tok = lp.argmax(dim=-1)
        toks.append(tok)
        lps.append(lp.gather(1, tok.view(-1, 1)).view(-1))
        if i + 1 < n:
            logits = m.decode_step(tok, cache)
    seq = torch.cat([idx, torch.stack(toks, dim=1)], dim=1)
    scored = m.score(seq).token_logprobs[:, T0 - 1:]
    return (torch.stack(lps, dim=1) - scored).abs().max().item()


def test_generate_beam_of_one_is_greedy_generate():
    c = _gen_case(256)
    m, T0, n = c["m"], 37, 12
    idx = c["ids"][:, :T0].to(DEV)
    want = m.generate(idx, n, top_k=1, num_samples=1)
    got = m.generate_beam(idx, n, num_beams=1)
    assert got.sequences.shape == (2, 1, T0 + n) and torch.equal(got.sequences[:, 0], want)
    assert got.lengths.tolist() == [[n], [n]] and got.scores.shape == (2, 1) and got.scores.dtype == torch.float32
    total = m.score(want).token_logprobs[:, T0 - 1:].sum(dim=1)
    bar = 2 * n * _delta(m, idx, n) + n * 1e-5
    assert ((got.scores[:, 0] - total).abs() <= bar).all(), (got.scores.tolist(), total.tolist(), bar)


def test_generate_beam_exhausts_a_small_vocabulary():
    """allowed_tokens of 2 ids, n = 4, W = 16: the 16 beams are all 16 sequences.  Their scores are sums of log-probabilities normalised over
    the two allowed columns (an excluded column counts as -inf: the rule of the header), so model.score's values — normalised over the whole
    vocabulary — are renormalised here from themselves: the restricted log p of a token is lp - logaddexp(lp, lp of the sibling sequence
    that differs in that token), both read from model.score of the 16 sequences."""
    c = _gen_case(256)
    m, T0, n, W = c["m"], 37, 4, 16
    idx = c["ids"][:, :T0].to(DEV)
    ids = [17, 300]
    out = m.generate_beam(idx, n, num_beams=W, allowed_tokens=ids)
    assert out.sequences.shape == (2, W, T0 + n) and torch.isfinite(out.scores).all() and (out.lengths == n).all()
    bar = 2 * n * _delta(m, idx, n) + n * 1e-5
    for p in range(2):
        new = out.sequences[p, :, T0:].tolist()
        assert sorted(new) == sorted([[ids[(r >> j) & 1] for j in range(n)] for r in range(W)]), "not all 16 sequences, once each"
        lp = m.score(out.sequences[p]).token_logprobs[:, T0 - 1:].double().cpu()      # (16, n), over the whole vocabulary
        at = {tuple(s): r for r, s in enumerate(new)}
        for r, s in enumerate(new):
            want = 0.0
            for j in range(n):
                sib = list(s)
                sib[j] = ids[0] + ids[1] - s[j]
                a, b = lp[r, j].item(), lp[at[tuple(sib)], j].item()
                want += a - (max(a, b) + math.log1p(math.exp(-abs(a - b))))
            assert abs(out.scores[p, r].item() - want) <= bar, (p, r, out.scores[p, r].item(), want, bar)
        assert (out.scores[p, :-1] >= out.scores[p, 1:]).all()


def test_generate_beam_scores_are_the_models_own():
    """W = 4, no mask, n = 12, P = 2: every returned sequence's score against model.score — what a wrong ancestry breaks"""
    c = _gen_case(256)
    m, T0, n, W = c["m"], 37, 12, 4
    idx = c["ids"][:, :T0].to(DEV)
    out = m.generate_beam(idx, n, num_beams=W)
    assert out.sequences.shape == (2, W, T0 + n) and torch.equal(out.sequences[:, :, :T0], idx.unsqueeze(1).expand(2, W, T0))
    bar = 2 * n * _delta(m, idx, n) + n * 1e-5
    total = m.score(out.sequences.view(2 * W, -1)).token_logprobs[:, T0 - 1:].sum(dim=1).view(2, W)
    print(f"generate_beam: worst |score - model.score| {(out.scores - total).abs().max().item():.3g}, bar {bar:.3g}")
    assert ((out.scores - total).abs() <= bar).all(), ((out.scores - total).abs().max().item(), bar)
    assert (out.scores[:, :-1] >= out.scores[:, 1:]).all()                           # non-increasing at length_penalty = 0
    assert len({tuple(s) for s in out.sequences[0].tolist()}) == W                   # the beams of a prompt differ
    again = m.generate_beam(idx, n, num_beams=W)
    assert torch.equal(again.sequences, out.sequences) and torch.equal(again.scores.view(torch.int32), out.scores.view(torch.int32))


def test_generate_beam_with_an_eos_token():
    c = _gen_case(256)
    m, T0, n, W = c["m"], 37, 12, 4
    idx = c["ids"][:, :T0].to(DEV)
    free = m.generate_beam(idx, n, num_beams=W)
    eos = int(free.sequences[0, 0, T0 + 2])                                          # the best beam of prompt 0 reaches it at its third token
    out = m.generate_beam(idx, n, num_beams=W, eos_token=eos, pad_token=3)
    steps = out.sequences.shape[2] - T0
    assert 1 <= steps <= n and (out.lengths <= steps).all() and (out.lengths >= 1).all()
    bar = 2 * n * _delta(m, idx, n) + n * 1e-5
    ended = 0
    for p in range(2):
        for r in range(W):
            k, new = int(out.lengths[p, r]), out.sequences[p, r, T0:].tolist()
            assert eos not in new[:k - 1] and new[k:] == [3] * (steps - k), (p, r, new, k)
            if k < steps:
                assert new[k - 1] == eos
            if new[k - 1] == eos:                                                    # a finished beam's score is frozen at its EOS
                ended += 1
                total = m.score(out.sequences[p, r:r + 1, :T0 + k]).token_logprobs[0, T0 - 1:].sum().item()
                assert abs(out.scores[p, r].item() - total) <= bar, (p, r, out.scores[p, r].item(), total)
    assert ended >= 1 and (out.lengths[0] < n).any()
    assert (out.scores[:, :-1] >= out.scores[:, 1:]).all()
    pen = m.generate_beam(idx, n, num_beams=W, eos_token=eos, pad_token=3, length_penalty=1.0)
    key = pen.scores / pen.lengths.float()
    assert (key[:, :-1] >= key[:, 1:]).all() and torch.equal(pen.scores.sort(dim=1).values, out.scores.sort(dim=1).values)
    only = m.generate_beam(idx, n, num_beams=W, eos_token=eos, allowed_tokens=[eos])     # every live beam must end at once: the loop stops after one step
    assert only.sequences.shape == (2, W, T0 + 1) and (only.sequences[:, :, T0] == eos).all() and only.lengths.tolist() == [[1] * W] * 2
    assert torch.isfinite(only.scores[:, 0]).all() and (only.scores[:, 1:] == -INF).all() and (only.scores[:, 0].abs() <= 1e-6).all()
