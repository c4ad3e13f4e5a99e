"""Generation from prompts of different lengths on the GPU: one cache position per row.  obte_attn_decode_rows row by row against
obte_attn_decode (bit for bit: a row's keys are partitioned and summed as the uniform entry point does it) and against the CPU oracle,
inactive rows, the rotate-and-store launch against the GEMM's RoPE epilogue + obte_kv_cache_store (bit for bit), the block, and
OmniBioTA.prefill / decode_step / generate with ``lengths`` — at the bars of tests/test_hip_generate.py for the same quantities."""
import ctypes as C

import pytest
import torch

import omnibiote_ref as R
from test_hip_causal import _add, _tril
from test_hip_generate import L, _block_setup, _decode_case, _gen_case, _oracle, _views, ops
from test_hip_ops import BF, DEV, close, rnd

pytestmark = pytest.mark.gpu

SPLITS = (0, 1, 2, 7, 64)
NEG_INF = float("-inf")


def _i32(values):
    return torch.tensor(list(values), dtype=torch.int32, device=DEV)


def _resolved(splits, B, H, hs, max_keys):
    """the split count a rows call takes: the forced one, or the library's choice at max_keys"""
    return splits if splits else int(L().lib().obte_attn_decode_splits(B, H, hs, max_keys))


def _queries(c, counts):
    """packed [B, 3C]: row b is the row of position counts[b] - 1 (the query the oracle of counts[b] keys is for); position 0 where
    the count is not a valid one"""
    qkv = c["qkv"]
    T = qkv.shape[1]
    return torch.stack([qkv[b, n - 1 if 1 <= n <= T else 0] for b, n in enumerate(counts)]).contiguous().to(DEV)


# =================================================================================================== one-query attention
@pytest.mark.parametrize("hs", [64, 128])
def test_attn_decode_rows_ragged_is_the_uniform_call_row_by_row(hs):
    o = ops()
    B, H, T_max = 4, 2, 1100
    counts = (1, 65, 600, 1100)
    C_ = H * hs
    scale = 8.0 / C_
    c = _decode_case(B, H, hs, T_max)
    q = _queries(c, counts)
    n_dev = _i32(counts)
    for splits in SPLITS:
        got, lse = o.attn_decode_rows(q, c["cache"], B, T_max, n_dev, T_max, H, hs, scale, splits=splits)
        forced = _resolved(splits, B, H, hs, T_max)
        for b, n in enumerate(counts):
            want, want_lse = o.attn_decode(q, c["cache"], B, T_max, n, H, hs, scale, splits=forced)
            assert torch.equal(got[b], want[b]) and torch.equal(lse[b], want_lse[b]), (hs, splits, b, n)
            ref_o, ref_lse = _oracle(c, n, scale)
            close(got[b], ref_o[b], atol=6e-3, what=f"attn_decode_rows hs={hs} row {b} n_keys={n} splits={splits}")
            close(lse[b], ref_lse[b], atol=2e-3, rtol=1e-3, what=f"lse hs={hs} row {b} n_keys={n} splits={splits}")
    # every count the same: the uniform entry point's bytes
    q = _queries(c, (257,) * B)
    for splits in SPLITS:
        got, lse = o.attn_decode_rows(q, c["cache"], B, T_max, _i32((257,) * B), 257, H, hs, scale, splits=splits)
        want, want_lse = o.attn_decode(q, c["cache"], B, T_max, 257, H, hs, scale, splits=splits)
        assert torch.equal(got, want) and torch.equal(lse, want_lse), (hs, splits)


@pytest.mark.parametrize("hs", [64, 128])
def test_attn_decode_rows_never_reads_a_row_s_tail(hs):
    """positions at and beyond each row's OWN count hold the bf16 NaN pattern 0x7FC0: the same bytes as with the clean cache, finite"""
    o = ops()
    B, H, T_max = 4, 2, 1100
    counts = (1, 65, 600, 1100)
    scale = 8.0 / (H * hs)
    c = _decode_case(B, H, hs, T_max)
    q = _queries(c, counts)
    n_dev = _i32(counts)
    dirty = c["cache"].clone()
    kv = dirty.view(torch.int16).view(2, B, H, T_max, hs)
    for b, n in enumerate(counts):
        kv[:, b, :, n:] = 0x7FC0
    assert torch.isnan(dirty.view(2, B, H, T_max, hs)[:, 0, :, 1:]).all()
    for splits in SPLITS:
        clean = o.attn_decode_rows(q, c["cache"], B, T_max, n_dev, T_max, H, hs, scale, splits=splits)
        got = o.attn_decode_rows(q, dirty, B, T_max, n_dev, T_max, H, hs, scale, splits=splits)
        for a, b_ in zip(got, clean):
            assert torch.isfinite(a).all() and torch.equal(a, b_), (hs, splits)


@pytest.mark.parametrize("hs", [64, 128])
def test_attn_decode_rows_inactive_rows(hs):
    """counts of 0, -1, max_keys + 1 (inside the cache, outside the bound) and INT32_MAX beside valid rows: zeros and lse = -inf for
    those, the valid rows bit for bit the uniform call's.  The inactive rows' whole cache is NaN: none of it is read into anything."""
    o = ops()
    B, H, T_max, max_keys = 4, 2, 1100, 600
    scale = 8.0 / (H * hs)
    c = _decode_case(B, H, hs, T_max)
    for counts in ((0, 65, -1, 600), (1, max_keys + 1, 600, 2 ** 31 - 1)):
        active = [1 <= n <= max_keys for n in counts]
        q = _queries(c, counts)
        n_dev = _i32(counts)
        cache = c["cache"].clone()
        kv = cache.view(torch.int16).view(2, B, H, T_max, hs)
        for b in range(B):
            if not active[b]:
                kv[:, b] = 0x7FC0
        for splits in SPLITS:
            got, lse = o.attn_decode_rows(q, cache, B, T_max, n_dev, max_keys, H, hs, scale, splits=splits)
            forced = _resolved(splits, B, H, hs, max_keys)
            for b, n in enumerate(counts):
                if active[b]:
                    want, want_lse = o.attn_decode(q, c["cache"], B, T_max, n, H, hs, scale, splits=forced)
                    assert torch.equal(got[b], want[b]) and torch.equal(lse[b], want_lse[b]), (hs, splits, b, n)
                else:
                    assert (got[b].view(torch.int16) == 0).all(), (hs, splits, b, n)          # +0.0 in every element
                    assert (lse[b] == NEG_INF).all(), (hs, splits, b, n, lse[b])
            if splits in (1, 7):
                again = o.attn_decode_rows(q, cache, B, T_max, n_dev, max_keys, H, hs, scale, splits=splits)
                assert torch.equal(got.view(torch.int16), again[0].view(torch.int16)) and torch.equal(lse, again[1])


# =================================================================================================== rotate and store
def _gemm_plain(o, a, w, M, N, K):
    """a W^T with OBTE_EPI_NONE through obte_gemm_bf16 (no workspace: one pass over K, as the block's c_attn runs it)"""
    d = torch.empty((M, N), dtype=BF, device=DEV)
    g = L().GemmArgs(a.data_ptr(), w.data_ptr(), d.data_ptr(), None, None, M, N, K, K, K, N, 1, 1, L().EPI_NONE, 1.0, 0.0, 0, 0)
    L().check(L().lib().obte_gemm_bf16(C.byref(g), torch.cuda.current_stream().cuda_stream), "obte_gemm_bf16")
    return d


@pytest.mark.parametrize("hs", [64, 128])
def test_rope_store_rows_is_the_uniform_step_s_epilogue_and_store(hs):
    from omnibiote_amd.model import rope_tables
    o = ops()
    B, H, T_max, marker = 4, 2, 77, 0x1234
    C_ = H * hs
    pos = (0, 37, T_max - 1, -1)
    rope = rope_tables(R.cast_rope_table(R.rope_table(hs, T_max), BF).to(DEV))
    h1 = rnd(B, C_, seed=hs).to(DEV)
    w = rnd(3 * C_, C_, seed=hs + 1, scale=C_ ** -0.5).to(DEV)
    plain = _gemm_plain(o, h1, w, B, 3 * C_, C_)
    qkv = plain.clone()
    cache = o.kv_cache_buffer(B, T_max, H, hs, DEV)
    cache.view(torch.int16).fill_(marker)
    o.kv_cache_rope_store_rows(qkv, rope, _i32(pos), T_max - 1, B, H, hs, cache, T_max)
    K, V = [z.view(torch.int16) for z in _views(cache, B, H, T_max, hs)]
    touched = torch.zeros(B, T_max, dtype=torch.bool)
    for b, p in enumerate(pos):
        if p < 0:
            continue
        touched[b, p] = True
        # the uniform decode's own form: c_attn with the RoPE epilogue at table row p (rope_T = 1), then the store at pos0 = p
        want = o.gemm(h1, w, B, 3 * C_, C_, epilogue=L().EPI_ROPE_QK, rope=(rope[0][p:], rope[1][p:], 1, hs))
        mine = o.kv_cache_buffer(B, T_max, H, hs, DEV)
        o.kv_cache_store(want, B, 1, H, hs, mine, T_max, p)
        assert torch.equal(qkv[b].view(torch.int16), want[b].view(torch.int16)), (hs, b, p)
        if p > 0:
            assert not torch.equal(qkv[b, :2 * C_], plain[b, :2 * C_])                      # it did rotate
        wk, wv = [z.view(torch.int16) for z in _views(mine, B, H, T_max, hs)]
        assert torch.equal(K[b, :, p], wk[b, :, p]) and torch.equal(V[b, :, p], wv[b, :, p]), (hs, b, p)
    untouched = ~touched.to(DEV)
    assert (K.transpose(1, 2)[untouched] == marker).all() and (V.transpose(1, 2)[untouched] == marker).all()
    assert torch.equal(qkv[3], plain[3])                                                     # the inactive row: neither rotated nor stored


# =================================================================================================== block
@pytest.mark.parametrize("C_,H", [(128, 2), (256, 2)])
def test_block_decode_rows_equal_positions_is_block_decode(C_, H):
    T = 160
    c = _block_setup(C_, H, T)
    o, B, hs = c["o"], c["B"], C_ // H
    x = c["x"].to(DEV)
    ws = o.block_decode_workspace(B, C_, H, DEV)
    for t in (130, 159):
        caches = []
        for _ in range(2):
            cache = o.kv_cache_buffer(B, T, H, hs, DEV)
            cache.view(torch.int16).fill_(0x1234)
            o.block_prefill(x[:, :t].contiguous(), c["params"], c["rope"], H, c["causal"](t), cache, T)
            caches.append(cache)
        xt = x[:, t].contiguous()
        want = o.block_decode(xt, c["params"], c["rope"], H, caches[0], T, t, ws=ws)
        got = o.block_decode_rows(xt, c["params"], c["rope"], H, caches[1], T, _i32((t, t)), t, ws=ws)
        assert torch.equal(got, want), (C_, t)
        assert torch.equal(caches[0].view(torch.int16), caches[1].view(torch.int16)), (C_, t)


@pytest.mark.parametrize("C_,H", [(128, 2), (256, 2)])
def test_block_decode_rows_ragged_vs_oracle(C_, H):
    """prefill x[:, :130], then row 0 through positions 97 .. 126 and row 1 through 130 .. 159 in the same 30 calls: each y row against
    the oracle's causal block forward of the whole x at that row's own position (the block bar)."""
    T0, T, start, steps = 130, 160, (97, 130), 30
    c = _block_setup(C_, H, T)
    o, B, hs = c["o"], c["B"], C_ // H
    ref = R.block_forward(c["x"].float(), {k: v.float() for k, v in c["w"].items()}, c["pre"], c["cfg"], c["tab"], _add(_tril(T)))
    x = c["x"].to(DEV)
    cache = o.kv_cache_buffer(B, T, H, hs, DEV)
    o.block_prefill(x[:, :T0].contiguous(), c["params"], c["rope"], H, c["causal"](T0), cache, T)
    ws = o.block_decode_workspace(B, C_, H, DEV)
    for i in range(steps):
        at = [s + i for s in start]
        xt = torch.stack([x[b, t] for b, t in enumerate(at)]).contiguous()
        yt = o.block_decode_rows(xt, c["params"], c["rope"], H, cache, T, _i32(at), max(at), ws=ws)
        want = torch.stack([ref[b, t] for b, t in enumerate(at)])
        close(yt, want, atol=3e-2, rtol=2.0 ** -6, what=f"block_decode_rows C={C_}, positions {at}")
        if i == 0:                                    # y may alias x (the store of these positions repeats itself bit for bit)
            assert torch.equal(o.block_decode_rows(xt, c["params"], c["rope"], H, cache, T, _i32(at), max(at), ws=ws, out=xt), yt)


# =================================================================================================== model
LENS = (97, 130)


def _teacher_forced(m, prompt, ids, lengths, steps):
    """prefill(prompt, lengths), then `steps` decode steps feeding each row its own next token of ids: logits (B, 1 + steps, vocab), row
    b's entry i at position lengths[b] - 1 + i"""
    from omnibiote_amd.model import KVCache
    cache = KVCache(m, prompt.shape[0])
    got = [m.prefill(prompt, cache, lengths=lengths)]
    assert cache.positions.dtype == torch.int32 and cache.positions.tolist() == list(lengths) and cache.max_pos == cache.pos == max(lengths)
    for i in range(steps):
        tok = torch.stack([ids[b, n + i] for b, n in enumerate(lengths)])
        got.append(m.decode_step(tok, cache))
    assert cache.positions.tolist() == [n + steps for n in lengths] and cache.max_pos == cache.pos == max(lengths) + steps
    return torch.stack(got, dim=1)


@pytest.mark.parametrize("C_", [256, 128])
def test_teacher_forced_ragged_decode_matches_the_oracle(C_):
    from omnibiote_amd.model import KVCache
    c = _gen_case(C_)
    m, ids = c["m"], c["ids"].to(DEV)
    steps, T0 = 60, max(LENS)
    runs = []
    for filler in (5, 300):                                        # row 0's padding columns: two different token ids
        prompt = ids[:, :T0].clone()
        prompt[0, LENS[0]:] = filler
        runs.append(_teacher_forced(m, prompt, ids, LENS, steps))
    assert torch.equal(runs[0], runs[1])                           # the padding reaches nothing
    got = runs[0].float().cpu()
    assert torch.isfinite(got).all()
    want = torch.stack([c["logits"][b, n - 1:n + steps] for b, n in enumerate(LENS)])
    d = (got - want).abs()
    print(f"ragged teacher-forced decode, C={C_}: max {d.max().item():.4g} mean {d.mean().item():.4g}")
    assert d.max().item() <= 5e-3 and d.mean().item() <= 1e-3, (d.max().item(), d.mean().item())
    # all lengths equal: the uniform path's logits
    same = _teacher_forced(m, ids[:, :T0].contiguous(), ids, (T0, T0), 10)
    cache = KVCache(m, 2)
    uni = [m.prefill(ids[:, :T0].contiguous(), cache)]
    assert cache.positions is None
    for t in range(T0, T0 + 10):
        uni.append(m.decode_step(ids[:, t], cache))
    assert torch.equal(same, torch.stack(uni, dim=1))


def _ragged_prompt(c):
    idx = c["ids"][:, :max(LENS)].clone()
    idx[0, LENS[0]:] = 7                                           # padding
    return idx.to(DEV)


def test_generate_ragged_greedy_follows_the_full_forward():
    """top_k = 1, 30 new tokens behind prompts of 97 and 130 tokens.  In ONE causal forward over each finished row, truncated to its own
    length, the logit of every generated token lies within 2e-2 of its position's maximum: the decode path and the full forward are
    each within 5e-3 of the oracle, hence within 1e-2 of each other, and an argmax taken on one side can lose at most twice that on
    the other (the bound and the argument of test_generate_greedy_follows_the_full_forward)."""
    c = _gen_case(256)
    m, idx = c["m"], _ragged_prompt(c)
    out, n = m.generate(idx, 30, top_k=1, lengths=LENS)
    assert out.shape == (2, 160) and out.dtype == torch.int64 and n.dtype == torch.int64
    assert n.tolist() == [a + 30 for a in LENS]
    for b, a in enumerate(LENS):
        assert torch.equal(out[b, :a], idx[b, :a])
        assert (out[b, a + 30:] == 0).all()                        # pad_token's default without an eos_token
        with torch.no_grad():
            logits = m(out[b:b + 1, :a + 30]).float()[0]
        at = logits[a - 1:a + 29]                                  # position t predicts token t + 1
        chosen = at.gather(-1, out[b, a:a + 30].unsqueeze(-1)).squeeze(-1)
        gap = at.max(dim=-1).values - chosen
        print(f"ragged greedy generate, row {b}: largest logit gap to the full forward's maximum {gap.max().item():.4g}")
        assert (gap <= 2e-2).all(), (b, gap.max().item())


def test_generate_ragged_eos_parks_a_row_and_sampling_is_seeded():
    c = _gen_case(256)
    m, idx = c["m"], _ragged_prompt(c)
    free, _ = m.generate(idx, 30, top_k=1, lengths=LENS)
    eos = int(free[0, LENS[0]])                                    # row 0's first greedy token
    out, n = m.generate(idx, 30, top_k=1, lengths=LENS, eos_token=eos, pad_token=3)
    assert int(n[0]) == LENS[0] + 1 and int(out[0, LENS[0]]) == eos
    assert (out[0, LENS[0] + 1:] == 3).all()
    assert torch.equal(out[0, :LENS[0]], idx[0, :LENS[0]])
    n1 = int(n[1])                                                 # row 1 runs on as if alone, up to its own stop
    hit = (free[1, LENS[1]:] == eos).nonzero().flatten()
    assert n1 == (LENS[1] + int(hit[0]) + 1 if hit.numel() else LENS[1] + 30)
    assert torch.equal(out[1, :n1], free[1, :n1]) and (out[1, n1:] == 3).all()
    assert out.shape[1] == n1                                      # returned right after the step at which the last row finished
    dflt, _ = m.generate(idx, 30, top_k=1, lengths=LENS, eos_token=eos)
    assert (dflt[0, LENS[0] + 1:] == eos).all()                    # pad_token defaults to eos_token
    a = m.generate(idx, 20, temperature=0.9, top_k=50, generator=torch.Generator(device=DEV).manual_seed(11), lengths=LENS)
    b = m.generate(idx, 20, temperature=0.9, top_k=50, generator=torch.Generator(device=DEV).manual_seed(11), lengths=LENS)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and a[1].tolist() == [x + 20 for x in LENS]


def test_generate_without_lengths_is_unchanged():
    from omnibiote_amd.model import KVCache
    c = _gen_case(256)
    m, idx = c["m"], c["ids"][:, :130].to(DEV)
    out = m.generate(idx, 5, top_k=1)
    assert isinstance(out, torch.Tensor) and out.shape == (2, 135) and out.dtype == torch.int64
    cache = KVCache(m, 2, 135)                                     # what generate() does today, by hand
    want = [idx]
    logits = m.prefill(idx, cache)
    for i in range(5):
        nxt = logits.argmax(dim=-1)
        want.append(nxt.unsqueeze(1))
        if i < 4:
            logits = m.decode_step(nxt, cache)
    assert cache.positions is None and cache.pos == 134
    assert torch.equal(out, torch.cat(want, dim=1))
