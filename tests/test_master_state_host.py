"""CPU tests of FusedAdamW(master_weights=True)'s host side: construction, the fp32 state through state_dict /
load_state_dict (torch's own load_state_dict casts floating-point state to the parameter's dtype, bf16), the two conversions
between bf16-mode and master-mode state, and the trainer flag.  Only step() needs the GPU (tests/test_hip_master_adamw.py)."""
import io
import warnings

import pytest
import torch

from omnibiote_amd import train_encoder as TE

BF = torch.bfloat16
SHAPES = [(16, 8), (64,), (8,)]


def _params(seed=0):
    g = torch.Generator().manual_seed(seed)
    return [torch.nn.Parameter(torch.randn(s, generator=g).to(BF)) for s in SHAPES]


def _groups(ps):
    return [{"params": ps[:2], "lr": 2.5e-4, "weight_decay": 0.04}, {"params": ps[2:]}]


def _through_a_file(obj):
    f = io.BytesIO()
    torch.save(obj, f)
    f.seek(0)
    return torch.load(f, weights_only=False)


def _fill_master_state(opt, ps, seed=1):
    """fp32 state that bf16 cannot hold: a cast to the parameter's dtype anywhere on the way would change every tensor"""
    g = torch.Generator().manual_seed(seed)
    for i, p in enumerate(ps):
        master = torch.randn(p.shape, generator=g)
        master.view(-1)[0] = 1.0 + 2.0 ** -12
        st = opt.state[p]
        st["step"] = 5 + i
        st["master"] = master
        st["exp_avg"] = torch.randn(p.shape, generator=g) * 1e-2
        st["exp_avg_sq"] = torch.rand(p.shape, generator=g) * 1e-4
        for k in ("master", "exp_avg", "exp_avg_sq"):
            assert not torch.equal(st[k].to(BF).float(), st[k])


def test_master_state_survives_state_dict_save_load_bit_for_bit():
    ps = _params()
    opt = TE.FusedAdamW(_groups(ps), lr=1e-3, weight_decay=1e-2, master_weights=True)
    assert opt.master_weights and all(p.dtype == BF for p in ps)
    _fill_master_state(opt, ps)
    opt.param_groups[0]["lr"] = 1.25e-4   # what a scheduler leaves behind
    sd = _through_a_file(opt.state_dict())
    qs = _params(seed=9)
    fresh = TE.FusedAdamW(_groups(qs), lr=1e-3, weight_decay=1e-2, master_weights=True)
    fresh.load_state_dict(sd)
    assert fresh.param_groups[0]["lr"] == 1.25e-4
    for p, q in zip(ps, qs):
        a, b = opt.state[p], fresh.state[q]
        assert b["step"] == a["step"]
        for k in ("master", "exp_avg", "exp_avg_sq"):
            assert b[k].dtype == torch.float32, (k, b[k].dtype)
            assert torch.equal(a[k], b[k]), k
    assert fresh.state[qs[0]]["master"].view(-1)[0].item() == 1.0 + 2.0 ** -12
    # and once more: what the fresh instance writes is what it read
    again = _through_a_file(fresh.state_dict())
    for k, v in sd["state"].items():
        for name in ("master", "exp_avg", "exp_avg_sq"):
            assert torch.equal(again["state"][k][name], v[name])


def test_bf16_mode_state_converts_into_master_mode_with_a_warning_and_the_reverse_is_refused():
    ps = _params()
    bf = TE.FusedAdamW(_groups(ps), lr=1e-3)
    g = torch.Generator().manual_seed(2)
    for p in ps:
        bf.state[p].update(step=3, exp_avg=(torch.randn(p.shape, generator=g) * 1e-2).to(BF),
                           exp_avg_sq=(torch.rand(p.shape, generator=g) * 1e-4).to(BF))
    sd = _through_a_file(bf.state_dict())
    qs = _params(seed=4)
    master = TE.FusedAdamW(_groups(qs), lr=1e-3, master_weights=True)
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        master.load_state_dict(sd)
    assert len(caught) == 1 and "master" in str(caught[0].message), [str(w.message) for w in caught]
    for p, q in zip(ps, qs):
        st = master.state[q]
        assert st["step"] == 3
        for k in ("exp_avg", "exp_avg_sq"):
            assert st[k].dtype == torch.float32 and torch.equal(st[k], bf.state[p][k].float()), k
        assert st["master"].dtype == torch.float32 and torch.equal(st["master"], q.detach().float())
    # the other direction would drop the masters without a word: refused
    _fill_master_state(master, qs)
    msd = _through_a_file(master.state_dict())
    for rounding in ("reference", "single"):
        with pytest.raises(ValueError, match="master"):
            TE.FusedAdamW(_groups(_params()), lr=1e-3, rounding=rounding).load_state_dict(msd)
    # the bf16 modes among themselves load as before
    other = TE.FusedAdamW(_groups(_params(seed=5)), lr=1e-3)
    other.load_state_dict(sd)
    assert all(st["exp_avg"].dtype == BF for st in other.state.values())


def test_trainer_flag_and_the_cpu_route_refuses_it():
    assert TE.parse_args([]).master_weights is False
    args = TE.parse_args(["--master_weights"])
    assert args.master_weights is True
    model = torch.nn.Linear(8, 8).to(BF)
    with pytest.raises(ValueError, match="master_weights"):
        TE.build_optimizer(model, args, 10, fused=False)
    with pytest.raises(ValueError, match="master_weights"):
        TE.build_optimizer(model, TE.parse_args([]), 10, fused=False, master_weights=True)
    # past the refusal (--force_lr: one plain group, no muP shapes needed on this stand-in model); the fused route constructs without a GPU
    opt, _ = TE.build_optimizer(model, TE.parse_args(["--master_weights", "--force_lr"]), 10)
    assert isinstance(opt, TE.FusedAdamW) and opt.master_weights
    opt, _ = TE.build_optimizer(model, TE.parse_args(["--force_lr"]), 10)
    assert isinstance(opt, TE.FusedAdamW) and not opt.master_weights
    opt, _ = TE.build_optimizer(model, TE.parse_args(["--force_lr"]), 10, fused=False)
    assert isinstance(opt, torch.optim.AdamW)


def test_master_mode_has_one_arithmetic():
    with pytest.raises(ValueError, match="rounding"):
        TE.FusedAdamW(_params(), master_weights=True, rounding="single")
    assert TE.FusedAdamW(_params(), master_weights=True, rounding="reference").master_weights
    assert not TE.FusedAdamW(_params()).master_weights
