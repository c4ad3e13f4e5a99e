"""The device-resident generation loop on the GPU: obte_gen_advance against sampling.advance_reference bit for bit inside guard bands,
DecodeLoop captured against DecodeLoop eager on twin caches, generate(loop="graph") against generate(loop="device"), both against the
model's own full forward at the bound of tests/test_hip_generate_rows.py, and the reuse of a captured loop."""
import pytest
import torch

from fenced import assert_guards, assert_same_bits, fenced
from omnibiote_amd import ops
from omnibiote_amd.sampling import advance_reference
from test_hip_generate import _gen_case
from test_hip_generate_rows import LENS, _ragged_prompt
from test_hip_ops import BF, DEV

pytestmark = pytest.mark.gpu

I32, I64, F32 = torch.int32, torch.int64, torch.float32
WIDTH, US_STEPS, EOS = 6, 5, 11
_tables = {}


def _wte(vocab, cols):
    if (vocab, cols) not in _tables:
        _tables[(vocab, cols)] = torch.randn(vocab, cols, generator=torch.Generator().manual_seed(vocab + cols)).to(BF)
    return _tables[(vocab, cols)]


def _rows(B, vocab):
    """per-row state that walks through every case of the rule, row b taking pattern b mod 8: running, parked, a full out, a negative
    count, the last step of the uniforms, tokens outside the table, positions at the ends of int32"""
    pos = [5, -1, 0, 2 ** 31 - 1, 17, -7, 3, 9]
    count = [0, 2, WIDTH - 1, WIDTH, US_STEPS - 1, 1, -2, WIDTH + 3]
    sampled = [vocab - 1, EOS, EOS, -5, vocab + 7, 8, 4, EOS]
    token = [1, vocab + 100, 2, 3, -9, vocab - 1, 5, 6]
    n_new = [0, 2, WIDTH - 1, WIDTH, 4, 1, 0, WIDTH]
    pick = lambda v, dt: torch.tensor([v[b % 8] for b in range(B)], dtype=dt)   # noqa: E731
    g = torch.Generator().manual_seed(B)
    return dict(sampled=pick(sampled, I64), pos=pick(pos, I32), count=pick(count, I32), n_new=pick(n_new, I32), token=pick(token, I64),
                out=torch.randint(0, vocab, (B, WIDTH), generator=g), us=torch.rand(US_STEPS, B, generator=g), u=torch.rand(B, generator=g))


@pytest.mark.parametrize("B,cols,vocab", [(B, cols, 300) for B in (1, 3, 65) for cols in (64, 1024, 4096)] + [(3, 64, 65536)])
def test_gen_advance_is_the_reference_bit_for_bit_inside_guard_bands(B, cols, vocab):
    wte = _wte(vocab, cols)
    for commit, eos, with_us in [(1, EOS, True), (0, EOS, True), (1, None, False), (0, None, True), (1, EOS, False)]:
        cpu = _rows(B, vocab)
        want = advance_reference(cpu["sampled"], cpu["pos"], cpu["count"], cpu["out"], cpu["n_new"], cpu["token"], wte, cpu["us"] if with_us else None,
                                 eos=eos, commit=commit)
        dev, hs = {}, {}
        for k, v in cpu.items():
            dev[k], hs[k] = fenced(v.to(DEV), poison="nan" if k == "us" else "mark")
        dev["wte"], hs["wte"] = fenced(wte.to(DEV), poison="nan")
        dev["x"], hs["x"] = fenced((B, cols), BF)
        ops.gen_advance(dev["sampled"], dev["pos"], dev["count"], dev["out"], dev["n_new"], dev["token"], dev["wte"], dev["x"],
                        us=dev["us"] if with_us else None, u=dev["u"] if with_us else None, eos=eos, commit=commit)
        what = f"commit {commit} eos {eos} us {with_us}"
        for name, ref in zip(("pos", "count", "out", "n_new", "token", "x"), want):
            assert_same_bits(dev[name].cpu(), ref, f"{name} ({what})")
        assert_same_bits(dev["u"].cpu(), want[6] if with_us else cpu["u"], f"u ({what})")   # not touched without us
        for name in ("sampled", "us"):
            assert_same_bits(dev[name].cpu(), cpu[name], f"{name} is read only ({what})")
        assert_same_bits(dev["wte"].cpu(), wte, "wte is read only")
        assert_guards(*hs.values())
        assert_same_bits(dev["x"], ops.embedding_fwd(dev["token"], dev["wte"]), f"x against obte_embedding_fwd ({what})")
        assert int(want[4][0]) == vocab - 1 and torch.equal(want[5][0], wte[vocab - 1])   # row 0 drew the table's last row


def test_gen_advance_wrapper_checks():
    r = {k: v.to(DEV) for k, v in _rows(3, 300).items()}
    wte, x = _wte(300, 64).to(DEV), torch.empty(3, 64, dtype=BF, device=DEV)
    args = lambda **kw: {**dict(sampled=r["sampled"], pos=r["pos"], count=r["count"], out=r["out"], n_new=r["n_new"], token=r["token"], wte=wte, x=x), **kw}   # noqa: E731
    with pytest.raises(RuntimeError, match="dtype"):
        ops.gen_advance(**args(pos=r["pos"].long()))
    with pytest.raises(ValueError, match="count"):
        ops.gen_advance(**args(count=r["count"][:2]))
    with pytest.raises(ValueError, match="out"):
        ops.gen_advance(**args(out=r["out"][:2]))
    with pytest.raises(ValueError, match="x"):
        ops.gen_advance(**args(x=x[:, :32].contiguous()))
    with pytest.raises(ValueError, match="commit"):
        ops.gen_advance(**args(commit=2))
    with pytest.raises(ValueError, match="us"):
        ops.gen_advance(**args(us=r["us"][:, :2].contiguous(), u=r["u"]))
    with pytest.raises(TypeError):
        ops.gen_advance(**args(us=r["us"]))                                         # us without u


# =================================================================================================== the loop
def _twin(kv_dtype, capture, settings, zero=True):
    """a prefilled cache (its bytes zeroed first, so that two of them can be compared whole) and a loop on it, not started"""
    from omnibiote_amd.model import DecodeLoop, KVCache
    c = _gen_case(256)
    m = c["m"]
    cache = KVCache(m, 2, dtype=kv_dtype)
    if zero:
        for kv in cache.layers:
            kv.zero_()
    logits = m.prefill(_ragged_prompt(c), cache, lengths=LENS)
    return m, cache, DecodeLoop(m, cache, max_steps=13, capture=capture, **settings), logits


def _sampled_settings():
    return dict(temperature=0.9, top_k=50, top_p=0.9, uniforms=torch.rand((13, 2), device=DEV, generator=torch.Generator(device=DEV).manual_seed(5)))


def _same_state(a, b, what):
    for name in ("logits", "token", "positions", "count", "n_new"):
        assert_same_bits(getattr(a, name), getattr(b, name), f"{name} {what}")


@pytest.mark.parametrize("kv_dtype,sampled", [("bf16", False), ("bf16", True), ("fp8", True)])
def test_graph_loop_is_the_eager_loop_bit_for_bit(kv_dtype, sampled):
    settings = _sampled_settings() if sampled else {}
    _, cache_e, eager, logits_e = _twin(kv_dtype, False, settings)
    _, cache_g, graph, logits_g = _twin(kv_dtype, True, settings)
    assert graph.graph is not None and eager.graph is None
    assert_same_bits(logits_g, logits_e, "prefill logits")
    assert graph.positions.tolist() == list(LENS)                                   # the warm-up left the loop's state as it found it
    eager.start(logits_e)
    graph.start(logits_g)
    _same_state(graph, eager, "after start")
    assert eager.count.tolist() == [1, 1] and eager.positions.tolist() == list(LENS)   # one token recorded, no position consumed
    for i in range(12):
        assert eager.run(1) == 1 and graph.run(1) == 1
        _same_state(graph, eager, f"after step {i + 1}")
    assert eager.positions is cache_e.positions and graph.positions is cache_g.positions
    assert eager.positions.tolist() == [n + 12 for n in LENS] and cache_g.pos == max(LENS) + 12 and cache_g.min_pos == min(LENS) + 12
    assert_same_bits(graph.out, eager.out, "out")
    assert eager.n_new.tolist() == [13, 13]
    for i, (a, b) in enumerate(zip(cache_g.layers, cache_e.layers)):
        assert_same_bits(a, b, f"layer {i}'s cache")
    (tg, ng), (te, ne) = graph.result(), eager.result()
    assert tg.shape == (2, 13) and torch.equal(tg, te) and torch.equal(ng, ne)
    with pytest.raises(ValueError, match="max_steps"):
        graph.run(1)


def test_graph_capture_needs_the_weight_streaming_row_limit():
    with ops.small_m_max(1):
        with pytest.raises(ValueError, match="capture"):
            _twin("bf16", True, {}, zero=False)
        _twin("bf16", False, {}, zero=False)                                        # the eager body takes any batch


def _uniform_prompt(c):
    return c["ids"][:, :130].to(DEV)


def _seeded(m, idx, loop, **kw):
    return m.generate(idx, 20, temperature=0.9, top_k=50, top_p=0.9, generator=torch.Generator(device=DEV).manual_seed(11), sampler="device", loop=loop, **kw)


def _eos_semantics(m, loop):
    """generate(loop=) with an eos_token, in both forms, checked against the same loop's free run: (ragged out, lengths, uniform out)"""
    c = _gen_case(256)
    idx = _ragged_prompt(c)
    free, _ = m.generate(idx, 30, top_k=1, lengths=LENS, sampler="device", loop=loop)
    eos = int(free[0, LENS[0]])                                                     # row 0's first greedy token
    out, n = m.generate(idx, 30, top_k=1, lengths=LENS, eos_token=eos, pad_token=3, sampler="device", loop=loop)
    assert int(n[0]) == LENS[0] + 1 and int(out[0, LENS[0]]) == eos and (out[0, LENS[0] + 1:] == 3).all()
    assert torch.equal(out[0, :LENS[0]], idx[0, :LENS[0]])
    n1 = int(n[1])                                                                  # row 1 runs on as if alone, up to its own stop
    hit = (free[1, LENS[1]:] == eos).nonzero().flatten()
    assert n1 == (LENS[1] + int(hit[0]) + 1 if hit.numel() else LENS[1] + 30)
    assert torch.equal(out[1, :n1], free[1, :n1]) and (out[1, n1:] == 3).all()
    assert out.shape[1] == n1 if hit.numel() else out.shape[1] == max(LENS) + 30   # the width of the eager loop: the longest row's end
    dflt, _ = m.generate(idx, 30, top_k=1, lengths=LENS, eos_token=eos, sampler="device", loop=loop)
    assert (dflt[0, LENS[0] + 1:] == eos).all()                                     # pad_token defaults to eos_token
    uidx = _uniform_prompt(c)
    ufree = m.generate(uidx, 20, top_k=1, sampler="device", loop=loop)
    assert ufree.shape == (2, 150) and torch.equal(ufree[:, :130], uidx)
    ueos = int(ufree[0, 130])
    uout = m.generate(uidx, 20, top_k=1, eos_token=ueos, sampler="device", loop=loop)
    assert (uout[0, 130:] == ueos).all()                                            # a finished row keeps producing EOS
    uhit = (ufree[1, 130:] == ueos).nonzero().flatten()
    w = 130 + (int(uhit[0]) + 1 if uhit.numel() else 20)
    assert uout.shape == (2, w) and torch.equal(uout[1], ufree[1, :w])
    return out, n, uout


def test_generate_device_loop_eos_and_seeding():
    c = _gen_case(256)
    m = c["m"]
    _eos_semantics(m, "device")
    a, b = _seeded(m, _ragged_prompt(c), "device", lengths=LENS), _seeded(m, _ragged_prompt(c), "device", lengths=LENS)
    assert torch.equal(a[0], b[0]) and a[1].tolist() == [x + 20 for x in LENS]


def test_generate_graph_equals_generate_device():
    c = _gen_case(256)
    m = c["m"]
    for g, d in zip(_eos_semantics(m, "graph"), _eos_semantics(m, "device")):
        assert g.shape == d.shape and torch.equal(g, d)
    for kw, idx in ((dict(lengths=LENS), _ragged_prompt(c)), ({}, _uniform_prompt(c))):
        g1, g2, d = _seeded(m, idx, "graph", **kw), _seeded(m, idx, "graph", **kw), _seeded(m, idx, "device", **kw)
        if kw:
            assert torch.equal(g1[0], g2[0]) and torch.equal(g1[0], d[0]) and torch.equal(g1[1], d[1])
        else:
            assert g1.shape == (2, 150) and torch.equal(g1, g2) and torch.equal(g1, d)
    f8g, f8d = _seeded(m, _uniform_prompt(c), "graph", kv_dtype="fp8"), _seeded(m, _uniform_prompt(c), "device", kv_dtype="fp8")
    assert torch.equal(f8g, f8d)


@pytest.mark.parametrize("loop", ["device", "graph"])
def test_generate_loop_greedy_follows_the_full_forward(loop):
    """top_k = 1, 30 new tokens behind prompts of 97 and 130 tokens.  In ONE causal forward over each finished row, truncated to its own
    length, the logit of every generated token lies within 2e-2 of its position's maximum: the bound and the argument of
    test_generate_ragged_greedy_follows_the_full_forward — it rests on the decode path's distance to the oracle, which no split
    count of the attention changes, so it holds under the loop's fixed bound as it does under decode_step's."""
    c = _gen_case(256)
    m, idx = c["m"], _ragged_prompt(c)
    out, n = m.generate(idx, 30, top_k=1, lengths=LENS, sampler="device", loop=loop)
    assert out.shape == (2, 160) and out.dtype == torch.int64 and n.dtype == torch.int64
    assert n.tolist() == [a + 30 for a in LENS]
    for b, a in enumerate(LENS):
        assert torch.equal(out[b, :a], idx[b, :a])
        assert (out[b, a + 30:] == 0).all()                                         # pad_token's default without an eos_token
        with torch.no_grad():
            logits = m(out[b:b + 1, :a + 30]).float()[0]
        at = logits[a - 1:a + 29]                                                   # position t predicts token t + 1
        chosen = at.gather(-1, out[b, a:a + 30].unsqueeze(-1)).squeeze(-1)
        gap = at.max(dim=-1).values - chosen
        print(f"generate(loop={loop!r}), row {b}: largest logit gap to the full forward's maximum {gap.max().item():.4g}")
        assert (gap <= 2e-2).all(), (b, gap.max().item())


def test_graph_loop_runs_again_behind_a_second_prefill():
    from omnibiote_amd.model import DecodeLoop, KVCache
    c = _gen_case(256)
    m, cache, loop, logits = _twin("bf16", True, _sampled_settings(), zero=False)
    loop.start(logits)
    assert loop.run(12) == 12
    first = loop.result()
    second = c["ids"][:, 20:120].to(DEV)                                            # another prompt, now of one length: uniform mode
    m.prefill(second, cache)
    with pytest.raises(ValueError, match="positions"):
        loop.start(logits)                                                          # a plain prefill took the loop's tensor off the cache
    logits2 = loop.prefill(second)
    assert cache.positions is loop.positions and loop.positions.tolist() == [100, 100] and (cache.pos, cache.min_pos) == (100, 100)
    with pytest.raises(ValueError, match="start"):
        loop.run(1)
    loop.start(logits2)
    loop.run(12)
    again = loop.result()
    fresh_cache = KVCache(m, 2)
    fresh_logits = m.prefill(second, fresh_cache)
    fresh = DecodeLoop(m, fresh_cache, max_steps=13, **_sampled_settings())
    assert fresh_cache.positions is fresh.positions and fresh.positions.tolist() == [100, 100]   # uniform mode was put into the rows form
    fresh.start(fresh_logits)
    fresh.run(12)
    want = fresh.result()
    assert torch.equal(again[0], want[0]) and torch.equal(again[1], want[1]) and not torch.equal(again[0], first[0])
    assert_same_bits(loop.logits, fresh.logits, "the last step's logits")
    # an eager step replaces cache.positions: the loop refuses to start on it
    logits3 = loop.prefill(second)
    m.decode_step(logits3.argmax(dim=-1), cache)
    assert cache.positions is not loop.positions
    with pytest.raises(ValueError, match="positions"):
        loop.start(logits3)
