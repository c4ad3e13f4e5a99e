"""GPU tests of FusedAdamW(master_weights=True): fp32 master weights and fp32 moments behind the bf16 parameters
(obte_adamw_multi_master, the fixed-order gradient norm).  The reference for the arithmetic is torch.optim.AdamW itself on
fp32 CPU tensors — the optimizer, not a formula typed into the test.

Bar for "the same fp32 number" (taken from test_fused_adamw_reference_rounding_is_torch_adamw_on_bf16_tensors in
tests/test_hip_ops.py and tightened from the width of bf16 to the width of the state, 2^-7 -> 2^-23): at least 99.9 % of the
elements bit-identical and none further than 2 fp32 ulps, an ulp being max(|a|, |b|) * 2^-23; masters get the same absolute
allowance as the parameters there, scaled by the same 2^-16 (0.02 * lr * 2^-16: a master near zero is a running sum of
lr-sized updates, and its own ulp is far finer than one ulp of an update)."""
import contextlib
import io
import math
import warnings

import numpy as np
import pytest
import torch

import omnibiote_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF = torch.bfloat16
ULP = 2.0 ** -23
KEYS = ("master", "exp_avg", "exp_avg_sq")


def TE():
    from omnibiote_amd import train_encoder
    return train_encoder


class Tally:
    """bit-identical count and the worst distance in units of the bar (2 ulps + the masters' allowance)"""

    def __init__(self, lr):
        self.total = self.same = 0
        self.worst = {k: 0.0 for k in KEYS}
        self.lr = lr

    def add(self, kind, ref, got):
        a, b = ref.detach().float().cpu(), got.detach().float().cpu()
        assert a.shape == b.shape and torch.isfinite(b).all()
        self.total += a.numel()
        self.same += int((a == b).sum())
        ulp = torch.maximum(a.abs(), b.abs()) * ULP + 1e-45
        slack = 0.02 * self.lr * 2.0 ** -16 if kind == "master" else 0.0
        self.worst[kind] = max(self.worst[kind], ((a - b).abs() / (2.0 * ulp + slack)).max().item())

    def add_state(self, ref_opt, q, fused, r):
        self.add("master", q.data, fused.state[r]["master"])
        self.add("exp_avg", ref_opt.state[q]["exp_avg"], fused.state[r]["exp_avg"])
        self.add("exp_avg_sq", ref_opt.state[q]["exp_avg_sq"], fused.state[r]["exp_avg_sq"])

    def check(self, what):
        print(f"{what}: {self.same} of {self.total} fp32 elements identical; worst / bar: {self.worst}")
        assert max(self.worst.values()) <= 1.0, self.worst
        assert self.same >= 0.999 * self.total, (self.same, self.total)


def _params_are_rounded_masters(fused, ps):
    for p in ps:
        st = fused.state[p]
        assert st["master"].dtype == torch.float32 and st["exp_avg"].dtype == torch.float32 and st["exp_avg_sq"].dtype == torch.float32
        assert p.dtype == BF and torch.equal(p.detach(), st["master"].to(BF))


SHAPES = [(256, 128), (1024,), (64, 512), (8,)]
STEPS = 12
LR, WD, BETAS, EPS = 3e-3, 1e-2, (0.9, 0.999), 1e-8


def _stream():
    """the inputs of test_fused_adamw_reference_rounding_is_torch_adamw_on_bf16_tensors"""
    gen = torch.Generator().manual_seed(5)
    p0 = [torch.randn(s, generator=gen).to(BF) for s in SHAPES]
    grads = [[(torch.randn(s, generator=gen) * (0.3 if t % 3 else 3.0)).to(BF) for s in SHAPES] for t in range(STEPS)]   # some steps clip, some do not
    return p0, grads


def _groups(ps):
    return [{"params": ps[:2], "lr": LR / 4, "weight_decay": WD * 4}, {"params": ps[2:], "lr": LR, "weight_decay": WD}]


def _pair(p0):
    cpu = [torch.nn.Parameter(x.float()) for x in p0]
    gpu = [torch.nn.Parameter(x.clone().to(DEV)) for x in p0]
    ref = torch.optim.AdamW(_groups(cpu), lr=LR, betas=BETAS, eps=EPS, weight_decay=WD)
    fused = TE().FusedAdamW(_groups(gpu), lr=LR, betas=BETAS, eps=EPS, weight_decay=WD, master_weights=True)
    sched_r = torch.optim.lr_scheduler.LinearLR(ref, start_factor=1.0, end_factor=0.0, total_iters=40)
    sched_f = torch.optim.lr_scheduler.LinearLR(fused, start_factor=1.0, end_factor=0.0, total_iters=40)
    return cpu, gpu, ref, fused, sched_r, sched_f


def _norm64(gs):
    return math.sqrt(sum((g.double() ** 2).sum().item() for g in gs))


@contextlib.contextmanager
def _reference_sqrt_correctly_rounded():
    """torch.optim.AdamW on fp32 CPU tensors calls the HOST math library's vector sqrt for `exp_avg_sq.sqrt()`, and that one op
    is not the same function on every CPU: exact on some, one ulp off for 0.7 % of its arguments on others, for 19 % on the MI355X
    hosts (12659 of 66568 second moments of the first test below) — every other op of the update is an IEEE operation and the
    same everywhere.  A reference that moves with the CPU it runs on cannot be met bit for bit by anything, so inside this
    context the optimizer's fp32 CPU sqrt returns the correctly rounded root (through float64: 53 bits >= 2 * 24 + 2), which is
    what IEEE 754 defines and what the exact hosts return anyway.  Everything else — the optimizer's own code, its op order, the
    bar — is untouched.  Yields the call counter: a test asserts that the optimizer did go through it."""
    calls = [0]
    host_sqrt = torch.Tensor.sqrt

    def sqrt(self):
        if self.dtype == torch.float32 and not self.is_cuda:
            calls[0] += 1
            return host_sqrt(self.double()).float()
        return host_sqrt(self)

    torch.Tensor.sqrt = sqrt
    try:
        yield calls
    finally:
        torch.Tensor.sqrt = host_sqrt


def test_master_step_is_torch_adamw_on_fp32_tensors():
    """The update arithmetic alone: torch.optim.AdamW on fp32 copies, fed g_bf16.float() * coef (an fp32 multiply), against the
    kernel fed the bf16 gradients and the SAME coefficient through its device clip_coef pointer.  The coefficient of each step is
    formed once, here (float64 norm of the bf16 gradients -> min(1, 1 / (norm + 1e-6)) -> fp32).  12 steps, two groups, LinearLR.

    Measured on the MI355X: moments all identical; masters see the count printed below.  With the host's own sqrt in the reference
    the result moves with the CPU (199704 of 199704 identical where it is exact, 199244 = 99.77 % and 3.4 ulps at worst where
    19 % of its roots are one ulp off): see _reference_sqrt_correctly_rounded; how far this host's sqrt is off is printed."""
    p0, grads = _stream()
    cpu, gpu, ref, fused, sched_r, sched_f = _pair(p0)
    for t in range(STEPS):
        coef = torch.tensor([min(1.0, 1.0 / (_norm64(grads[t]) + 1e-6))], dtype=torch.float32)
        for q, r, g in zip(cpu, gpu, grads[t]):
            q.grad = g.float() * coef
            r.grad = g.clone().to(DEV)
        with _reference_sqrt_correctly_rounded() as calls:
            ref.step()
        assert calls[0] == len(cpu)
        sched_r.step()
        assert fused.step(clip_coef=coef.to(DEV)) is None
        sched_f.step()
    tally = Tally(LR)
    for q, r in zip(cpu, gpu):
        tally.add_state(ref, q, fused, r)
    _params_are_rounded_masters(fused, gpu)
    v_all = torch.cat([ref.state[q]["exp_avg_sq"].flatten() for q in cpu])
    print(f"this host's torch sqrt is not the correctly rounded one for {_host_sqrt_off(v_all)} of {v_all.numel()} second moments")
    tally.check("master AdamW vs torch.optim.AdamW on fp32 CPU tensors")


def _host_sqrt_off(t):
    """elements whose fp32 square root, as THIS host's torch computes it, is not the correctly rounded one (the CPU math library's
    vector sqrt is exact on some CPUs and up to one ulp off on others; the GPU's is correctly rounded)"""
    exact = t.double().sqrt().float()   # 53 bits >= 2 * 24 + 2: rounding the double root gives the correctly rounded fp32 root
    return int((t.sqrt() != exact).sum())


def _ieee_step(w, m, v, g, cc, lr, wd, b1, b2, eps, step):
    """torch.optim.AdamW's fp32 op sequence in NumPy, every op correctly rounded (fma through float64: the product of two fp32
    numbers is exact there, the sum is rounded to 53 bits and then to 24 — a double rounding that differs from a true fma for
    about one operand pair in 2^29)"""
    f32 = np.float32
    fma = lambda a, b, c: (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(f32)
    decay, step_size, bc2s = f32(1.0 - lr * wd), f32(lr / (1.0 - b1 ** step)), f32((1.0 - b2 ** step) ** 0.5)
    w1, w2 = f32(1.0 - b1), f32(1.0 - b2)
    g = g * f32(cc)
    w = w * decay
    m = fma(np.full_like(m, w1), g - m, m)
    v = fma(w2 * g, g, v * f32(b2))
    d = np.sqrt(v) / bc2s + f32(eps)
    return w + (-step_size * m) / d, m, v


def test_master_step_is_the_correctly_rounded_evaluation_of_torchs_op_sequence():
    """Beside the comparison with torch.optim.AdamW itself (the test above), which inherits the host's vector sqrt: the same inputs
    against the op sequence evaluated in NumPy with every operation correctly rounded.  This one does not depend on the CPU the
    test runs on.  Bar: all elements identical but for the emulated fma's double rounding (2^-29 per element and step, i.e. none
    expected in 2.4 M element-steps: at most 2 elements allowed, none further than 1 ulp)."""
    p0, grads = _stream()
    gpu = [torch.nn.Parameter(x.clone().to(DEV)) for x in p0]
    fused = TE().FusedAdamW(_groups(gpu), lr=LR, betas=BETAS, eps=EPS, weight_decay=WD, master_weights=True)
    sched = torch.optim.lr_scheduler.LinearLR(fused, start_factor=1.0, end_factor=0.0, total_iters=40)
    state = [(x.float().numpy().copy(), np.zeros(x.shape, np.float32), np.zeros(x.shape, np.float32)) for x in p0]
    for t in range(STEPS):
        coef = np.float32(min(1.0, 1.0 / (_norm64(grads[t]) + 1e-6)))
        for i, g in enumerate(grads[t]):
            grp = fused.param_groups[i // 2]
            state[i] = _ieee_step(*state[i], g.float().numpy(), coef, grp["lr"], grp["weight_decay"], *BETAS, EPS, t + 1)
            gpu[i].grad = g.clone().to(DEV)
        fused.step(clip_coef=torch.tensor([coef], dtype=torch.float32, device=DEV))
        sched.step()
    off = total = 0
    for (w, m, v), r in zip(state, gpu):
        for want, key in ((w, "master"), (m, "exp_avg"), (v, "exp_avg_sq")):
            got = fused.state[r][key].cpu().numpy()
            total += want.size
            off += int((got != want).sum())
            assert (np.abs(got - want) <= np.spacing(np.maximum(np.abs(got), np.abs(want)))).all(), key
    print(f"master AdamW vs the correctly rounded op sequence: {total - off} of {total} identical")
    assert off <= 2, (off, total)


@pytest.mark.parametrize("lr", [1e-3, 2.3e-4, 1e-4])
def test_weights_at_one_keep_learning_below_the_bf16_step(lr):
    """The capability.  A LayerNorm weight sits at 1.0, where one bf16 step is 2^-8 downwards and 2^-7 upwards, and Adam moves it
    by about lr per step: in the default mode (torch.optim.AdamW on bf16 tensors, bit for bit) 64 steps of a constant-sign
    gradient leave every element at exactly 1.0 at these learning rates.  With fp32 masters the weight moves by 64 * lr, as
    torch.optim.AdamW on fp32 tensors moves it, and the bf16 parameter follows as bf16(master)."""
    steps, n = 64, 1024
    g = (torch.randn(n, generator=torch.Generator().manual_seed(0)).sign() * 0.01).to(BF)
    frozen = torch.nn.Parameter(torch.ones(n, dtype=BF, device=DEV))
    moving = torch.nn.Parameter(torch.ones(n, dtype=BF, device=DEV))
    q = torch.nn.Parameter(torch.ones(n))
    kw = dict(lr=lr, betas=BETAS, eps=EPS, weight_decay=0.0)
    default, master, ref = TE().FusedAdamW([frozen], **kw), TE().FusedAdamW([moving], master_weights=True, **kw), torch.optim.AdamW([q], **kw)
    for _ in range(steps):
        frozen.grad, moving.grad, q.grad = g.to(DEV), g.to(DEV), g.float()
        assert default.step() is None and master.step() is None
        with _reference_sqrt_correctly_rounded() as calls:
            ref.step()
        assert calls[0] == 1
    assert bool((frozen.detach() == 1.0).all()), "the bf16 regime was expected to lose every update at this lr"
    tally = Tally(lr)
    tally.add_state(ref, q, master, moving)
    w = master.state[moving]["master"]
    moved = (w - 1.0).abs().mean().item()
    print(f"lr {lr}: mean |master - 1| = {moved:.6g} (64 lr = {64 * lr:.6g}); bf16 parameters off 1.0: {int((moving.detach() != 1.0).sum())} of {n}")
    tally.check(f"lr {lr}")
    assert abs(moved - steps * lr) <= 0.01 * steps * lr
    _params_are_rounded_masters(master, [moving])
    if lr == 1e-3:   # 0.064 is sixteen bf16 steps below 1.0 and eight above it
        assert bool((moving.detach() != 1.0).all())


def _run_with_own_clipping(p0, grads):
    gpu = [torch.nn.Parameter(x.clone().to(DEV)) for x in p0]
    fused = TE().FusedAdamW(_groups(gpu), lr=LR, betas=BETAS, eps=EPS, weight_decay=WD, master_weights=True)
    sched = torch.optim.lr_scheduler.LinearLR(fused, start_factor=1.0, end_factor=0.0, total_iters=40)
    norms = []
    for t in range(STEPS):
        for r, g in zip(gpu, grads[t]):
            r.grad = g.clone().to(DEV)
        out = fused.step(max_norm=1.0)
        assert out.shape == () and out.dtype == torch.float32 and torch.equal(out, fused._clip_out[0])   # the device's own value
        norms.append(out)
        sched.step()
    return gpu, fused, [x.item() for x in norms]


def test_master_step_with_its_own_clipping_end_to_end():
    """step(max_norm=1.0) against clip_grad_norm_ + torch.optim.AdamW on fp32 CPU tensors.  The two norms differ by fp32 summation
    order only.  A relative norm error d scales a step's gradient by (1 + d): m moves by <= d, v by <= 2 d relatively, the update
    by <= 2 d lr.  Device: 64 squares per lane in order, then trees: worst case about 78 * 2^-24 < 2^-17 (asserted against the
    float64 norm of the same gradients).  torch: clip_grad_norm_'s fp32 norm is 2.7e-6 ~ 2^-18.5 off the float64 norm on these
    inputs.  Together 2 (d + d') < 2^-15 per step, so per element |master_hip - master_torch| <= steps * lr * 2^-15 + 2 fp32 ulps,
    lr being the element's group's.  Two identical runs must agree bit for bit: the norm is summed in a fixed order."""
    p0, grads = _stream()
    cpu = [torch.nn.Parameter(x.float()) for x in p0]
    ref = torch.optim.AdamW(_groups(cpu), lr=LR, betas=BETAS, eps=EPS, weight_decay=WD)
    sched_r = torch.optim.lr_scheduler.LinearLR(ref, start_factor=1.0, end_factor=0.0, total_iters=40)
    for t in range(STEPS):
        for q, g in zip(cpu, grads[t]):
            q.grad = g.float()
        torch.nn.utils.clip_grad_norm_(cpu, 1.0)
        ref.step(); sched_r.step()
    gpu, fused, norm_sq = _run_with_own_clipping(p0, grads)
    for t in range(STEPS):
        n64 = _norm64(grads[t])
        rel = abs(math.sqrt(norm_sq[t]) - n64) / n64
        print(f"step {t}: device norm {math.sqrt(norm_sq[t]):.9g}, float64 norm {n64:.9g}, relative error {rel:.3g} (bar 2^-17 = {2.0 ** -17:.3g})")
        assert rel <= 2.0 ** -17
    worst = 0.0
    for i, (q, r) in enumerate(zip(cpu, gpu)):
        a, b = q.data, fused.state[r]["master"].cpu()
        lr = LR / 4 if i < 2 else LR
        bound = STEPS * lr * 2.0 ** -15 + 2.0 * torch.maximum(a.abs(), b.abs()) * ULP
        err = (a - b).abs()
        worst = max(worst, (err / bound).max().item())
        print(f"tensor {i}: max |master_hip - master_torch| = {err.max().item():.3g}; identical {int((a == b).sum())} of {a.numel()}; "
              f"moments identical {int((ref.state[q]['exp_avg'] == fused.state[r]['exp_avg'].cpu()).sum())} / "
              f"{int((ref.state[q]['exp_avg_sq'] == fused.state[r]['exp_avg_sq'].cpu()).sum())}")
        assert bool((err <= bound).all()), (i, err.max().item())
    print("worst / bar:", worst)
    _params_are_rounded_masters(fused, gpu)
    gpu2, fused2, norm_sq2 = _run_with_own_clipping(p0, grads)
    assert norm_sq2 == norm_sq
    for r, r2 in zip(gpu, gpu2):
        assert torch.equal(r.detach(), r2.detach())
        for k in KEYS:
            assert torch.equal(fused.state[r][k], fused2.state[r2][k]), k


def test_a_parameter_written_through_torch_reseeds_its_master_with_one_warning():
    """The kernel writes p through a raw pointer, which torch's version counter does not see; a write through torch
    (model.load_state_dict, p.copy_ under no_grad) bumps it, and the next step takes that parameter's master from the new bf16
    values, warning once.  The other masters are left alone.  (A write through ``p.data`` runs on a detached alias with a version
    counter of its own — p._version does not move, nothing can notice it from the host — so it is followed by reseed_masters().)"""
    gen = torch.Generator().manual_seed(11)
    p0 = [torch.randn(s, generator=gen).to(BF) for s in [(64, 32), (512,), (8,)]]
    grads = [[(torch.randn(x.shape, generator=gen) * 0.1).to(BF) for x in p0] for _ in range(5)]
    other = (p0[1].float() + 1.0).to(BF)
    cpu = [torch.nn.Parameter(x.float()) for x in p0]
    gpu = [torch.nn.Parameter(x.clone().to(DEV)) for x in p0]
    kw = dict(lr=LR, betas=BETAS, eps=EPS, weight_decay=WD)
    ref, fused = torch.optim.AdamW(cpu, **kw), TE().FusedAdamW(gpu, master_weights=True, **kw)

    def step(t):
        for q, r, g in zip(cpu, gpu, grads[t]):
            q.grad, r.grad = g.float(), g.clone().to(DEV)
        with _reference_sqrt_correctly_rounded() as calls:
            ref.step()
        assert calls[0] == len(cpu)
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            fused.step()
        return [str(w.message) for w in caught]

    assert step(0) == [] and step(1) == []
    with torch.no_grad():
        gpu[1].copy_(other.to(DEV))
        cpu[1].copy_(other.float())
    said = step(2)
    assert len(said) == 1 and "re-seeded" in said[0], said
    tally = Tally(LR)
    for q, r in zip(cpu, gpu):
        tally.add_state(ref, q, fused, r)
    tally.check("after a foreign write")
    assert not torch.equal(fused.state[gpu[0]]["master"], gpu[0].detach().float())   # still an fp32 number, not its own rounding
    assert step(3) == []                                                              # the kernel's own writes are no foreign write
    # through .data nothing moves the version: the explicit way
    gpu[2].data.copy_(other[:8].to(DEV))
    with torch.no_grad():
        cpu[2].copy_(other[:8].float())
    fused.reseed_masters([gpu[2]])
    assert torch.equal(fused.state[gpu[2]]["master"], other[:8].float().to(DEV))
    assert step(4) == []
    tally = Tally(LR)
    for q, r in zip(cpu, gpu):
        tally.add_state(ref, q, fused, r)
    tally.check("after reseed_masters")
    _params_are_rounded_masters(fused, gpu)


def _tiny_train_step(total_iters=10):
    """the tiny configuration of tests/test_hip_model.py's TrainStep tests, dropout 0, muP groups, master weights, LinearLR"""
    from omnibiote_amd.mup_compat import mu_param_groups, set_base_shapes
    from omnibiote_amd.model import OmniBioTA, OmniBioTAConfig
    C, H, Lyr, V, T, mini = 128, 2, 2, 512, 64, 4
    cfg = R.RefConfig(block_size=T, vocab_size=V, n_layer=Lyr, n_head=H, n_embd=C)
    c = OmniBioTAConfig(); c.block_size, c.vocab_size, c.n_layer, c.n_head, c.n_embd, c.dropout, c.flash = T, V, Lyr, H, C, 0.0, True
    m = OmniBioTA(c)
    cb = OmniBioTAConfig(); cb.block_size, cb.vocab_size, cb.n_layer, cb.dropout, cb.flash = T, V, Lyr, 0.0, True
    cb.n_embd, cb.n_head = 24, 3
    base = OmniBioTA(cb)
    cb.n_embd, cb.n_head = 48, 12
    delta = OmniBioTA(cb)
    set_base_shapes(m, base, delta=delta, rescale_params=False)
    m.load_state_dict(R.hash_weights(cfg), strict=False)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        m.to(BF)
    m.to(DEV)
    lr, wd = 1e-2, 1e-2
    opt = TE().FusedAdamW(mu_param_groups(list(m.parameters()), lr, wd), lr=lr, betas=BETAS, eps=EPS, weight_decay=wd, master_weights=True)
    sched = torch.optim.lr_scheduler.LinearLR(opt, start_factor=1.0, end_factor=0.0, total_iters=total_iters)
    return m, opt, sched, TE().TrainStep(m, opt, sched, mini_batch_size=mini, n_head=H)


def test_resume_from_saved_state_is_bitwise():
    """Four steps straight against two steps, the state_dicts of model, optimizer and scheduler through torch.save / torch.load
    into freshly built objects (model first, then optimizer, as run() resumes), two more steps on the same batches: parameters,
    masters and moments bit for bit.  torch's own Optimizer.load_state_dict would hand the masters back rounded to bf16."""
    V, T, rows = 512, 64, 8
    rng = np.random.default_rng(7)
    batches = []
    for _ in range(4):
        ids = torch.from_numpy(TE().synthetic_rows(rows, T, V, rng, single_document=False))
        batches.append((ids.to(DEV), torch.from_numpy(rng.random((rows, T)) < 0.15).to(DEV)))
    m1, opt1, _, step1 = _tiny_train_step()
    losses = [step1(ids, mlm_mask=mask)["loss"].item() for ids, mask in batches]
    m2, opt2, sched2, step2 = _tiny_train_step()
    losses2 = [step2(ids, mlm_mask=mask)["loss"].item() for ids, mask in batches[:2]]
    f = io.BytesIO()
    torch.save({"model": m2.state_dict(), "optimizer": opt2.state_dict(), "scheduler": sched2.state_dict()}, f)
    f.seek(0)
    saved = torch.load(f, map_location=DEV, weights_only=False)
    assert all(st["master"].dtype == torch.float32 for st in saved["optimizer"]["state"].values())
    m3, opt3, sched3, step3 = _tiny_train_step()
    m3.load_state_dict(saved["model"])
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        opt3.load_state_dict(saved["optimizer"])
        sched3.load_state_dict(saved["scheduler"])
        losses2 += [step3(ids, mlm_mask=mask)["loss"].item() for ids, mask in batches[2:]]
    # a restored master must not be taken for a stale one and re-seeded from its own rounding, nor anything be converted
    assert not [str(w.message) for w in caught if "FusedAdamW" in str(w.message)]
    assert all(math.isfinite(x) for x in losses + losses2), (losses, losses2)
    assert losses2 == losses, (losses, losses2)
    assert [g["lr"] for g in opt3.param_groups] == [g["lr"] for g in opt1.param_groups]
    lossy = 0
    for (k, a), (_, b) in zip(m1.named_parameters(), m3.named_parameters()):
        assert torch.equal(a.detach(), b.detach()), k
        sa, sb = opt1.state[a], opt3.state[b]
        assert sa["step"] == sb["step"] == 4
        for key in KEYS:
            assert sb[key].dtype == torch.float32 and torch.equal(sa[key], sb[key]), (k, key)
        lossy += int((sa["master"].to(BF).float() != sa["master"]).sum())
    _params_are_rounded_masters(opt3, list(m3.parameters()))
    assert lossy > 0   # the masters do hold more than bf16 can: a load that rounded them could not have passed


def test_multi_tensor_packing_gives_what_each_tensor_alone_gives():
    """40 tensors in one group (two launches of <= 32), sizes around the chunk boundaries of the multi-tensor walk among them:
    every master, moment and parameter equals the same tensor stepped by an optimizer of its own."""
    from omnibiote_amd import _lib
    chunk = _lib.MT_CHUNK
    rng = np.random.default_rng(3)
    sizes = [8, chunk - 8, chunk, chunk + 8] + [8 * int(k) for k in rng.integers(1, 700, size=35)] + [3 * chunk + 16]
    assert len(sizes) == 40
    gen = torch.Generator().manual_seed(13)
    p0 = [torch.randn(n, generator=gen).to(BF) for n in sizes]
    grads = [[(torch.randn(n, generator=gen) * 0.2).to(BF) for n in sizes] for _ in range(3)]
    kw = dict(lr=LR, betas=BETAS, eps=EPS, weight_decay=WD, master_weights=True)
    together = [torch.nn.Parameter(x.clone().to(DEV)) for x in p0]
    alone = [torch.nn.Parameter(x.clone().to(DEV)) for x in p0]
    opt = TE().FusedAdamW(together, **kw)
    opts = [TE().FusedAdamW([p], **kw) for p in alone]
    coef = torch.tensor([0.75], dtype=torch.float32, device=DEV)
    for t in range(3):
        for p, q, g in zip(together, alone, grads[t]):
            p.grad, q.grad = g.clone().to(DEV), g.clone().to(DEV)
        opt.step(clip_coef=coef if t == 1 else None)
        for o in opts:
            o.step(clip_coef=coef if t == 1 else None)
    for n, p, q, o in zip(sizes, together, alone, opts):
        assert torch.equal(p.detach(), q.detach()), n
        for k in KEYS:
            assert torch.equal(opt.state[p][k], o.state[q][k]), (n, k)
    _params_are_rounded_masters(opt, together)
    # the fixed-order norm over the same 40 tensors: one partial per chunk of every tensor, and the same bits twice
    norms = []
    for _ in range(2):
        for p, g in zip(together, grads[0]):
            p.grad = g.clone().to(DEV)
        norms.append(opt.step(max_norm=1.0).item())
    assert norms[0] == norms[1]
    n64 = _norm64(grads[0])
    assert abs(math.sqrt(norms[0]) - n64) / n64 <= 2.0 ** -17
