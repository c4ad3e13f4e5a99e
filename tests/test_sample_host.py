"""Host-side tests (no GPU) of next-token sampling: the symbol table of the device sampler against its companion header, every argument
check of obte_sample_logits_bf16 that returns before a launch, the rule's plain-torch statement (sampling.sample_reference) on its edge
cases, top-p in model.sample_next, and the validation of generate(sampler=)."""
import ctypes as C
import os
import re

import pytest
import torch

from omnibiote_amd import _lib

EINVAL, EUNSUPPORTED = -1, -3
P = 4096   # a non-null, 16-byte aligned "pointer" for calls that must return before they touch it
NAMES = ("obte_sample_logits_bf16",)
BF = torch.bfloat16
INF = float("inf")


def _err():
    return _lib.lib().obte_last_error().decode()


def test_sample_symbols_have_their_own_table():
    lib = _lib.lib()
    assert tuple(_lib.SYMBOLS_SAMPLE) == NAMES
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "omnibiote_hip_sample.h")).read()
    assert set(re.findall(r"^(?:int|int64_t|void|const char\*) +(obte_[a-z0-9_]+)\(", header, flags=re.M)) == set(NAMES)
    assert len(re.findall(r"^[a-z0-9_\* ]+\bobte_[a-z0-9_]+\(", header, flags=re.M)) == len(NAMES)      # and nothing else
    for name in NAMES:
        assert name not in _lib.SYMBOLS and name not in _lib.SYMBOLS_ROWS and name not in _lib.SYMBOLS_SMALL_M
        fn = getattr(lib, name)
        res, args = _lib.SYMBOLS_SAMPLE[name]
        assert fn.restype is res and list(fn.argtypes) == args                                            # bound by lib(), in the same loop
    assert len(_lib.SYMBOLS) == 70 and len(_lib.SYMBOLS_ROWS) == 3 and len(_lib.SYMBOLS_SMALL_M) == 3
    assert lib.obte_abi_version() == 1
    sizes = (C.c_int64 * 16)()
    assert lib.obte_struct_sizes(sizes, 16) == 6


def _call(logits=P, ld=1008, B=2, V=1003, u=P, temperature=1.0, top_k=0, top_p=1.0, token=P, n_kept=P):
    return _lib.lib().obte_sample_logits_bf16(logits, ld, B, V, u, temperature, top_k, top_p, token, n_kept, None)


@pytest.mark.parametrize("kw,rc,word", [
    (dict(logits=None), EINVAL, "null"), (dict(token=None), EINVAL, "null"),
    (dict(logits=P + 8), EINVAL, "logits"), (dict(logits=P + 2), EINVAL, "16-byte"),
    (dict(ld=1004), EINVAL, "ld"), (dict(ld=1000), EINVAL, "ld"), (dict(ld=1012), EINVAL, "ld"),
    (dict(B=0), EINVAL, "B"), (dict(B=-3), EINVAL, "B"), (dict(V=0, ld=8), EINVAL, "V"),
    (dict(temperature=-0.5), EINVAL, "temperature"), (dict(temperature=INF), EINVAL, "temperature"),
    (dict(temperature=float("nan")), EINVAL, "temperature"),
    (dict(top_p=0.0), EINVAL, "top_p"), (dict(top_p=-0.1), EINVAL, "top_p"), (dict(top_p=1.0001), EINVAL, "top_p"),
    (dict(top_p=float("nan")), EINVAL, "top_p"),
    (dict(u=P + 2), EINVAL, "u must be 4-byte"), (dict(n_kept=P + 1), EINVAL, "n_kept must be 4-byte"),
    (dict(token=P + 4), EINVAL, "token must be 8-byte"),
    (dict(V=65537, ld=65544), EUNSUPPORTED, "65537"), (dict(V=1 << 20, ld=1 << 20), EUNSUPPORTED, "V"),
])
def test_sample_logits_rejects_before_any_launch(kw, rc, word):
    assert _call(**kw) == rc
    assert _err().startswith("obte_sample_logits_bf16:") and word in _err(), _err()


def test_ops_sample_logits_refuses_cpu_tensors():
    from omnibiote_amd import ops
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.sample_logits(torch.zeros(2, 16, dtype=BF))


# ----------------------------------------------------------------------------------------------- the rule in plain torch
def _rows(b=4, v=65536, s=2.0, seed=0):
    return (torch.randn(b, v, generator=torch.Generator().manual_seed(seed)) * s).to(BF)


def test_reference_top_k_1_is_the_lowest_argmax():
    from omnibiote_amd.sampling import sample_reference
    x = _rows(3, 500)
    x[0, 17] = x[0, 400] = 30.0                     # a tie for the maximum: the lower index
    x[1, 0] = 30.0
    for kw in (dict(u=0.7, top_k=1), dict(u=None), dict(u=0.7, temperature=0)):
        tok, n, cdf = sample_reference(x, **kw)
        assert tok.tolist() == [17, 0, int(x[2].float().argmax())] and n.tolist() == [1, 1, 1]
        assert cdf.shape == (3, 500) and cdf[0, 16] == 0 and cdf[0, 17] == 1
    tok, n, cdf = sample_reference(x[0], 0.3, top_k=1)      # one row in, scalars out
    assert int(tok) == 17 and int(n) == 1 and cdf.shape == (500,)


def test_reference_keeps_a_tie_at_the_kth_value_whole():
    from omnibiote_amd.sampling import sample_reference
    x = _rows()
    _, n, cdf = sample_reference(x, 0.5, top_k=50)
    kth = x.float().topk(50, dim=1).values[:, -1:]
    assert torch.equal(n, (x.float() >= kth).sum(dim=1)) and (n >= 50).all() and (n <= 60).all(), n.tolist()
    print("kept at k = 50:", n.tolist())
    y = torch.full((1, 1000), -3.0, dtype=BF)
    y[0, :10] = 2.0
    y[0, 100:400] = 1.0                              # the 11th .. 310th largest are one value
    for k, want in ((10, 10), (11, 310), (200, 310), (310, 310), (311, 1000)):
        assert int(sample_reference(y, 0.5, top_k=k)[1]) == want, k
        assert int(sample_reference(y, 0.5, n_kept=k)[1]) == want, k          # the kept set rebuilt from a count


def test_reference_no_ops_and_tiny_top_p():
    from omnibiote_amd.sampling import sample_reference
    x = _rows(3, 4096)
    u = torch.tensor([0.1, 0.5, 0.9])
    plain = sample_reference(x, u, 0.8)
    assert plain[1].tolist() == [4096] * 3
    for kw in (dict(top_p=1.0), dict(top_k=4096), dict(top_k=5000), dict(top_k=4096, top_p=1.0)):
        got = sample_reference(x, u, 0.8, **kw)
        assert all(torch.equal(a, b) for a, b in zip(got, plain)), kw
    x[1, 5] = x[1, 77] = x[1, 4000] = 30.0                                   # the maximum three times in row 1
    tok, n, _ = sample_reference(x, u, 0.8, top_p=1e-6)
    assert n.tolist() == [1, 3, 1]
    assert tok.tolist() == [int(x[0].float().argmax()), 77, int(x[2].float().argmax())]   # u = 0.5 of three equal weights: the second


def test_reference_u_ends_and_top_p_order():
    from omnibiote_amd.sampling import sample_reference
    x = _rows(2, 1003, s=4.0, seed=3)
    for kw in (dict(top_k=16), dict(top_p=0.9), dict(top_k=200, top_p=0.5, temperature=0.8)):
        _, n, cdf = sample_reference(x, 0.5, **kw)
        w = torch.diff(cdf, dim=1, prepend=torch.zeros(2, 1, dtype=torch.float64))
        for r in range(2):
            nz = (w[r] > 0).nonzero().flatten()
            assert int(sample_reference(x[r], 0.0, **kw)[0]) == int(nz[0])
            assert int(sample_reference(x[r], -1.0, **kw)[0]) == int(nz[0])
            assert int(sample_reference(x[r], float("nan"), **kw)[0]) == int(nz[0])
            assert int(sample_reference(x[r], 0.99999994, **kw)[0]) == int(nz[-1])
            assert int(sample_reference(x[r], 1.0, **kw)[0]) == int(nz[-1])
            assert int(sample_reference(x[r], 7.0, **kw)[0]) == int(nz[-1])
            assert 1 <= nz.numel() <= int(n[r])
    # top-p: the kept mass reaches p, and without the lowest kept value it does not; it is applied to what top-k kept
    p = torch.softmax(x.double(), dim=1)
    _, n, _ = sample_reference(x, 0.5, top_p=0.9)
    for r in range(2):
        sv = x[r].double().sort(descending=True).values
        thr = sv[int(n[r]) - 1]
        assert p[r][x[r].double() >= thr].sum() >= 0.9 > p[r][x[r].double() > thr].sum()
    n_k = sample_reference(x, 0.5, top_k=20)[1]
    n_kp = sample_reference(x, 0.5, top_k=20, top_p=0.5)[1]
    assert (n_kp <= n_k).all() and (n_kp >= 1).all() and (n_kp < n_k).any()


def test_reference_never_returns_nan_or_minus_inf_entries():
    from omnibiote_amd.sampling import sample_reference
    x = _rows(4, 300, seed=5)
    x[0, ::2] = float("nan")
    x[0, 1::4] = -INF
    x[1, :] = -INF                                   # nothing to sample
    x[2, :] = float("nan")
    x[3, 40] = x[3, 200] = INF
    for u in (0.0, 0.3, 0.999, 1.0):
        for kw in (dict(), dict(top_k=7), dict(top_p=0.8), dict(top_k=1)):
            tok, n, cdf = sample_reference(x, u, **kw)
            assert torch.isfinite(x[0, int(tok[0])].float())
            assert (int(tok[1]), int(n[1]), int(tok[2]), int(n[2])) == (0, 0, 0, 0)
            assert float(cdf[1].abs().sum()) == 0 and float(cdf[2].abs().sum()) == 0
            assert int(tok[3]) in (40, 200)              # the rest of a +inf row is kept at weight zero unless a cut removes it
            want = {(): 300, ("top_k", 7): 7, ("top_p", 0.8): 2, ("top_k", 1): 1}[tuple(kw.items())[0] if kw else ()]
            assert int(n[3]) == want or (kw == dict(top_k=7) and int(n[3]) > 7), (kw, int(n[3]))      # (a tie at the 7th value)
    assert int(sample_reference(x[0], 0.5)[1]) == 75                          # 300 - 150 NaN - 75 -inf
    assert int(sample_reference(x[3], 0.25)[0]) == 40 and int(sample_reference(x[3], 0.75)[0]) == 200


# ----------------------------------------------------------------------------------------------- model.sample_next(top_p=)
def _parent_sample_next(logits, temperature=1.0, top_k=None, generator=None):
    """the function as it stood before top_p, operation for operation"""
    if top_k == 1 or temperature == 0:
        return torch.argmax(logits, dim=-1)
    logits = logits.float() / temperature
    if top_k is not None:
        v, _ = torch.topk(logits, min(top_k, logits.size(-1)))
        logits = logits.masked_fill(logits < v[:, [-1]], float("-inf"))
    probs = torch.softmax(logits, dim=-1)
    return torch.multinomial(probs, num_samples=1, generator=generator).squeeze(1)


def test_sample_next_top_p_stays_in_the_reference_kept_set():
    from omnibiote_amd.model import sample_next
    from omnibiote_amd.sampling import sample_reference
    x = _rows(4, 512, seed=9)
    for kw in (dict(top_p=0.5), dict(top_p=0.5, top_k=40, temperature=1.3)):
        n = sample_reference(x, 0.5, kw.get("temperature", 1.0), kw.get("top_k"), kw["top_p"])[1]
        sv = x.double().sort(dim=1, descending=True).values
        kept = x.double() >= sv.gather(1, (n - 1).unsqueeze(1))
        assert (n < 512).all() and (n >= 1).all()
        g = torch.Generator().manual_seed(21)
        seen = torch.zeros_like(kept)
        for _ in range(2000 // 4):                   # 2000 draws, four rows at a time
            tok = sample_next(x, generator=g, **kw)
            assert kept.gather(1, tok.unsqueeze(1)).all()
            seen[torch.arange(4), tok] = True
        assert (seen.sum(dim=1) > 1).any()           # it does sample


def test_sample_next_without_top_p_keeps_its_stream():
    from omnibiote_amd.model import sample_next
    x = _rows(3, 700, seed=13)
    for kw in (dict(), dict(temperature=0.8), dict(temperature=1.2, top_k=30), dict(top_k=1), dict(temperature=0)):
        ga, gb, gc = (torch.Generator().manual_seed(5) for _ in range(3))
        for _ in range(10):
            want = _parent_sample_next(x, generator=ga, **kw)
            assert torch.equal(sample_next(x, generator=gb, **kw), want)
            assert torch.equal(sample_next(x, generator=gc, top_p=None, **kw), want)
    ga, gb = torch.Generator().manual_seed(5), torch.Generator().manual_seed(5)
    assert torch.equal(sample_next(x, 0.8, 30, ga, 1.0), _parent_sample_next(x, 0.8, 30, gb))     # top_p = 1 cuts nothing


@pytest.mark.parametrize("bad", [0.0, -0.2, 1.5, float("nan")])
def test_invalid_top_p_raises(bad):
    from omnibiote_amd.model import sample_next
    from omnibiote_amd.sampling import sample_reference
    x = _rows(2, 64)
    with pytest.raises(ValueError, match="top_p"):
        sample_next(x, top_p=bad)
    with pytest.raises(ValueError, match="top_p"):
        sample_reference(x, 0.5, top_p=bad)


def test_generate_validates_sampler_before_any_device_work():
    from omnibiote_amd.model import OmniBioTA, OmniBioTAConfig
    c = OmniBioTAConfig()
    c.block_size, c.vocab_size, c.n_layer, c.n_head, c.n_embd, c.dropout, c.flash = 32, 64, 1, 2, 128, 0.0, True
    c.autoregressive = True
    m = OmniBioTA(c)
    idx = torch.zeros(2, 8, dtype=torch.int64)
    with pytest.raises(ValueError, match="sampler"):
        m.generate(idx, 4, sampler="nonsense")
    with pytest.raises(ValueError, match="sampler"):
        m.generate(idx, 4, lengths=[8, 5], sampler="Device")
    with pytest.raises(ValueError, match="top_p"):
        m.generate(idx, 4, top_p=0.0, sampler="device")
    with pytest.raises(ValueError, match="block_size"):
        m.generate(idx, 25, top_p=0.9, sampler="device")           # the existing checks still come first
