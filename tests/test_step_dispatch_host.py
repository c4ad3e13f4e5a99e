"""Host-side test (no GPU) of the one place that chooses a cached step's block op, OmniBioTA._step_blocks: the six ops replaced by
recorders, a CPU model, caches that are position state alone — every row of the table

    SharedPrefixCache, no ancestry -> block_decode_shared(prefix, prompts, prefix_len, n_prefix, suffix, max_new, pos - n_prefix)
    SharedPrefixCache, ancestry    -> block_decode_beam(the same, then the table)
    KVCache, weights given         -> block_step_w8(kv, max_len, pos, pos_rows, kv8=(dtype == "fp8"))
    KVCache fp8                    -> block_decode_kv8(kv, max_len, pos, pos_rows)
    KVCache bf16, rows mode        -> block_decode_rows(kv, max_len, pos_rows, pos)
    KVCache bf16, uniform          -> block_decode(kv, max_len, pos)

per layer, with ws = the cache's workspace and out = x; and decode_step reaches the same calls and then advances the cache by one."""
import pytest
import torch

from omnibiote_amd import ops
from omnibiote_amd.model import CachePositions, SharedPrefixCache
from test_w8_host import _cpu_model, _fake

OPS = ("block_decode", "block_decode_rows", "block_decode_kv8", "block_step_w8", "block_decode_shared", "block_decode_beam")
I32 = torch.int32


@pytest.fixture
def calls(monkeypatch):
    seen = []
    for name in OPS:
        monkeypatch.setattr(ops, name, lambda *a, _name=name, **kw: seen.append((_name, a, kw)))
    return seen


def _kv(dtype, rows):
    c = _fake(pos=8, batch=2, max_len=32, dtype=dtype)
    if rows:
        c.reset(8, torch.tensor([8, 5], dtype=I32), 5)
    c.layers, c.decode_ws = ["kv0", "kv1"], "ws"
    return c


def _shared():
    """3 prompts of 9 tokens (a prefix buffer of 12) with 2 samples each, 2 of 8 suffix slots filled"""
    c = SharedPrefixCache.__new__(SharedPrefixCache)
    CachePositions.__init__(c, 6, 20)
    c._shape(3, 2, 12, 8)
    c.reset(11)
    c.n_prefix = 9
    c.layers, c.decode_ws = [("pre0", "suf0"), ("pre1", "suf1")], "ws"
    return c


TABLE = torch.zeros((6, 8), dtype=I32)
# (the cache, an ancestry table or None) -> (the op without weights, the op with weights, its position arguments for layer i at (pos, pos_rows))
CASES = {
    "shared": (lambda: (_shared(), None), "block_decode_shared", "block_decode_shared", lambda i, pos, rows: (f"pre{i}", 3, 12, 9, f"suf{i}", 8, pos - 9)),
    "beam": (lambda: (_shared(), TABLE), "block_decode_beam", "block_decode_beam", lambda i, pos, rows: (f"pre{i}", 3, 12, 9, f"suf{i}", 8, pos - 9, TABLE)),
    "bf16-uniform": (lambda: (_kv("bf16", False), None), "block_decode", "block_step_w8", lambda i, pos, rows: (f"kv{i}", 32, pos)),
    "bf16-rows": (lambda: (_kv("bf16", True), None), "block_decode_rows", "block_step_w8", lambda i, pos, rows: (f"kv{i}", 32, rows, pos)),
    "fp8-uniform": (lambda: (_kv("fp8", False), None), "block_decode_kv8", "block_step_w8", lambda i, pos, rows: (f"kv{i}", 32, pos, rows)),
    "fp8-rows": (lambda: (_kv("fp8", True), None), "block_decode_kv8", "block_step_w8", lambda i, pos, rows: (f"kv{i}", 32, pos, rows)),
}


def _same(got, want):
    return len(got) == len(want) and all(g is w if isinstance(w, torch.Tensor) else g == w for g, w in zip(got, want))


def _check(calls, m, wq, case, cache, x, pos, rows):
    """the recorded calls are the table's for ``case``: per layer the op, the block's parameters and tables, the position arguments, ws and out"""
    _, plain, quantized, at = CASES[case]
    shared = isinstance(cache, SharedPrefixCache)
    assert [c[0] for c in calls] == [quantized if wq is not None else plain] * 2
    for i, (name, a, kw) in enumerate(calls):
        block = m.transformer.h[i]
        assert a[0] is x and kw["out"] is x and kw["ws"] == "ws"
        if name == "block_step_w8":
            assert a[1] is wq.block_params(i) and a[2][0] is wq.codes[i] and a[2][1] is wq.scales[i]
            assert a[3] is block.attn.rope() and a[4] == 2 and _same(a[5:], (f"kv{i}", 32, pos, rows))
            assert kw == dict(kv8=cache.dtype == "fp8", ws="ws", out=x)
        else:
            assert all(p is q for p, q in zip(a[1], m._block_params(block))) and len(a[1]) == 6
            assert a[2] is block.attn.rope() and a[3] == 2 and _same(a[4:], at(i, pos, rows))
            assert kw == dict(ws="ws", out=x)
        assert not (shared and name == "block_step_w8")


@pytest.mark.parametrize("quantized", [False, True], ids=["bf16-weights", "e4m3-weights"])
@pytest.mark.parametrize("case", list(CASES))
def test_every_row_of_the_table(calls, case, quantized):
    m = _cpu_model()
    wq = m.quantize_weights() if quantized else None
    cache, table = CASES[case][0]()
    x = torch.zeros((cache.batch, 128), dtype=torch.bfloat16)
    # decode_step's arguments (cache.pos, cache.positions), then a DecodeLoop's: a fixed bound with the loop's own tensor
    rows = cache.positions
    m._step_blocks(x, cache, cache.pos, rows, weights=wq, ancestry=table)
    _check(calls, m, None if isinstance(cache, SharedPrefixCache) else wq, case, cache, x, cache.pos, rows)
    if rows is not None:
        calls.clear()
        m._step_blocks(x, cache, cache.max_len - 1, rows, weights=wq)
        _check(calls, m, wq, case, cache, x, 31, rows)
    assert cache.pos == (11 if isinstance(cache, SharedPrefixCache) else 8)                     # the dispatch does not advance the cache


class _OnGpu(torch.Tensor):
    """a CPU tensor that says it is on the GPU: decode_step's device check passes, and every op behind it is a recorder here"""
    is_cuda = True


@pytest.mark.parametrize("quantized", [False, True], ids=["bf16-weights", "e4m3-weights"])
@pytest.mark.parametrize("case", [c for c in CASES if c != "beam"])
def test_decode_step_reaches_the_same_calls_and_advances_the_cache(calls, monkeypatch, case, quantized):
    m = _cpu_model()
    wq = m.quantize_weights() if quantized else None
    cache, _ = CASES[case][0]()
    tokens = torch.zeros(cache.batch, dtype=torch.int64).as_subclass(_OnGpu)
    if quantized and isinstance(cache, SharedPrefixCache):
        with pytest.raises(NotImplementedError, match=r"OmniBioTA\.decode_step: weights="):
            m.decode_step(tokens, cache, weights=wq)
        assert calls == [] and cache.pos == 11
        return
    x = torch.zeros((cache.batch, 128), dtype=torch.bfloat16)
    read = []
    monkeypatch.setattr(ops, "embedding_fwd", lambda ids, wte: x)
    monkeypatch.setattr(m.transformer.ln_f, "forward", lambda h: h)
    monkeypatch.setattr(m, "_readout_rows", lambda h, out=None, weights=None: read.append((h, out, weights)) or "logits")
    pos, rows = cache.pos, cache.positions
    assert m.decode_step(tokens, cache, weights=wq) == "logits"
    _check(calls, m, wq, case, cache, x, pos, rows)
    assert len(read) == 1 and read[0][0] is x and read[0][1] is None and read[0][2] is wq
    assert cache.pos == pos + 1
    if rows is not None:
        assert cache.positions.tolist() == [9, 6] and cache.min_pos == 6
