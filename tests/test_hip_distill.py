"""obte_distill_ce_rows (include/omnibiote_hip_distill.h, ops.distill_ce_rows) against the float64 rule distill.distill_reference on
the same bf16 inputs, at the shapes where the CE family can go wrong: test_masked_ce's (rows, V) — 512 (one chunk per thread, most
threads idle past it), 1000 (no multiple of the chunk stride, a last wave without elements), 65 536 (the full register form) — and
65 536 + 4096, the streamed form that reads both rows twice.

Bars.  row_loss, row_ce, row_kl and the summed loss: test_masked_ce's, 1e-4 |ref| + 1e-6.  dlogits at alpha = 1: test_masked_ce's,
literally (atol 2e-7, rtol 2^-7) — the KL term is multiplied by an exact zero, the arithmetic is that kernel's.  dlogits with a KL
term: p - q cancels, so a relative bar alone cannot hold where the two are close; the bar is 2^-7 |ref| (bf16's rounding with the
existing margin) + EPS w (ce_weight + 2 kl_weight b), the absolute error of the three fp32 softmax values (each <= 1) scaled as the
gradient scales them.  EPS is measured against distill_reference on these inputs: the largest observed value of
(|got - ref| - 2^-7 |ref|) / (w (ce_weight + 2 kl_weight b)) is EPS_OBSERVED; the bar is four times it (the fast exponential's error
depends on its argument, the margin covers other seeds).  Every case prints its own figure before asserting.
Measured: 2.384e-7 (= 2^-22), in test_the_student_as_its_own_teacher at temperature 1, where the reference gradient is an exact zero and
the two log-sum-exps of the same row differ by an fp32 rounding; 6.5e-9 there at temperature 2; at most 1.3e-9 over the 32 cases of
test_distill_ce_rows_against_the_float64_rule that have a KL term (elsewhere the relative part covers the error).  Bar: 9.54e-7."""
import numpy as np
import pytest
import torch

from omnibiote_amd.distill import distill_reference, distill_weights

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF = torch.bfloat16
N_ACCUM = 4
SHAPES = [(64, 512), (33, 1000), (50, 65536), (6, 65536 + 4096)]
EPS_OBSERVED = 2.384e-7   # measured: see the module docstring
EPS = 4 * EPS_OBSERVED


def ops():
    from omnibiote_amd import ops as o
    return o


def L():
    from omnibiote_amd import _lib
    return _lib


_inputs = {}


def inputs(rows, V):
    """Student and teacher logits (bf16), labels and row weights on the GPU, made once per shape and left unchanged.  Even rows: an
    unrelated teacher (p and q far apart); odd rows: the student plus a little noise (p - q cancels)."""
    if (rows, V) not in _inputs:
        g = torch.Generator().manual_seed(1000 + V + rows)
        s = (torch.randn(rows, V, generator=g) * 2.0).to(BF)
        far = torch.randn(rows, V, generator=g) * 2.0
        near = s.float() + 0.25 * torch.randn(rows, V, generator=g)
        odd = (torch.arange(rows) % 2 == 1).view(rows, 1)
        t = torch.where(odd, near, far).to(BF)
        tgt = torch.from_numpy(np.random.default_rng(V + rows).integers(0, V, size=rows))
        tgt[0], tgt[-1] = 0, V - 1
        w = (torch.rand(rows, generator=g) + 0.5) / rows
        _inputs[(rows, V)] = tuple(x.to(DEV) for x in (s, t, tgt, w.float()))
    return _inputs[(rows, V)]


def loss_close(got, ref, what):
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    assert torch.isfinite(got).all(), what
    err, bound = (got - ref).abs(), 1e-4 * ref.abs() + 1e-6
    assert (err <= bound).all(), f"{what}: max err {err.max():.3g}, worst margin {(err - bound).max():.3g}"


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("alpha", [0.0, 0.5, 1.0])
@pytest.mark.parametrize("temperature", [1.0, 2.0])
@pytest.mark.parametrize("rows,V", SHAPES)
def test_distill_ce_rows_against_the_float64_rule(rows, V, temperature, alpha, weighted):
    s, t, tgt, w = inputs(rows, V)
    rw = w if weighted else None
    ref = distill_reference(s, t, tgt, N_ACCUM, rw, alpha, temperature)
    row_loss, dl, row_ce, row_kl = ops().distill_ce_rows_per_row(s, t, tgt, N_ACCUM, rw, alpha, temperature)
    loss, dl2, row_ce2, row_kl2 = ops().distill_ce_rows(s, t, tgt, N_ACCUM, rw, alpha, temperature)
    assert torch.equal(dl, dl2) and torch.equal(row_ce, row_ce2) and torch.equal(row_kl, row_kl2)      # bitwise repeatable
    assert dl.dtype == BF and dl.shape == s.shape and row_loss.dtype == torch.float32
    loss_close(row_loss, ref.row_loss, "row_loss")
    loss_close(row_ce, ref.row_ce, "row_ce")
    loss_close(row_kl, ref.row_kl, "row_kl")
    loss_close(loss, ref.loss, "loss")
    assert (row_kl >= -1e-6).all()
    cw, kw, b = distill_weights(alpha, temperature)
    err = (dl.double() - ref.dlogits).abs()
    assert torch.isfinite(dl.float()).all()
    scale = ref.row_weight.view(-1, 1) * (cw + 2 * kw * b)
    eps_seen = ((err - 2.0 ** -7 * ref.dlogits.abs()).clamp_min(0) / scale).max().item()
    print(f"distill rows {rows} V {V} T {temperature} alpha {alpha} weighted {weighted}: eps observed {eps_seen:.3e}, "
          f"max |err| {err.max().item():.3e}, max |ref| {ref.dlogits.abs().max().item():.3e}")
    if alpha == 1.0:
        bound = 2.0 ** -7 * ref.dlogits.abs() + 2e-7
    else:
        bound = 2.0 ** -7 * ref.dlogits.abs() + EPS * scale
    bad = err > bound
    assert not bad.any(), f"dlogits: {int(bad.sum())}/{bad.numel()} off; max err {err.max():.4g}, eps observed {eps_seen:.3e} (bar {EPS:.3e})"
    # gradient rows sum to ~0 (softmax - onehot, and a difference of two softmaxes)
    assert dl.float().sum(1).abs().max().item() < 1e-3


@pytest.mark.parametrize("temperature", [1.0, 2.0])
@pytest.mark.parametrize("rows,V", SHAPES)
def test_a_row_does_not_depend_on_the_other_rows(rows, V, temperature):
    """A row's four results are identical when the call holds only that row (its weight handed over, so that w is the same)."""
    s, t, tgt, w = inputs(rows, V)
    row_loss, dl, row_ce, row_kl = ops().distill_ce_rows_per_row(s, t, tgt, N_ACCUM, w, 0.5, temperature)
    for r in (0, rows // 2, rows - 1):
        one = ops().distill_ce_rows_per_row(s[r:r + 1].contiguous(), t[r:r + 1].contiguous(), tgt[r:r + 1], N_ACCUM, w[r:r + 1].contiguous(), 0.5, temperature)
        assert torch.equal(one[0], row_loss[r:r + 1]) and torch.equal(one[1], dl[r:r + 1])
        assert torch.equal(one[2], row_ce[r:r + 1]) and torch.equal(one[3], row_kl[r:r + 1])


@pytest.mark.parametrize("temperature", [1.0, 2.0])
def test_the_student_as_its_own_teacher(temperature):
    s, _, tgt, _ = inputs(64, 512)
    _, dl, row_ce, row_kl = ops().distill_ce_rows_per_row(s, s.clone(), tgt, 1, None, 0.0, temperature)
    assert row_kl.abs().max().item() <= 1e-6
    # the reference gradient is an exact zero: what is left is the two softmaxes' own fp32 error, the case EPS is there for
    cw, kw, b = distill_weights(0.0, temperature)
    scale = (1.0 / 64) * (cw + 2 * kw * b)
    eps_seen = dl.float().abs().max().item() / scale
    print(f"distill student = teacher T {temperature}: eps observed {eps_seen:.3e}")
    assert eps_seen <= EPS
    loss_close(row_ce, torch.nn.functional.cross_entropy(s.double(), tgt, reduction="none"), "row_ce")


def test_bad_arguments_are_refused_before_any_launch():
    lib = L().lib()
    n, V = 4, 512
    s, t = torch.zeros(n, V, dtype=BF, device=DEV), torch.zeros(n, V, dtype=BF, device=DEV)
    tgt = torch.zeros(n, dtype=torch.int64, device=DEV)
    out = torch.full((3, n), 7.0, dtype=torch.float32, device=DEV)
    dl = torch.full((n, V), 3.0, dtype=BF, device=DEV)

    def call(logits=s, teacher=t, target=tgt, inv_t=1.0, row_loss=out[0], dlogits=dl, rows=n, vocab=V):
        p = lambda x: None if x is None else (x if isinstance(x, int) else x.data_ptr())
        return lib.obte_distill_ce_rows(p(logits), p(teacher), p(target), 1.0, None, 0.5, 0.5, inv_t, p(row_loss), p(out[1]), p(out[2]), p(dlogits),
                                        rows, vocab, torch.cuda.current_stream().cuda_stream)

    bad = [dict(vocab=V - 4), dict(vocab=0), dict(vocab=131072 + 8), dict(rows=0), dict(dlogits=s), dict(dlogits=t), dict(teacher=None),
           dict(logits=None), dict(target=None), dict(row_loss=None), dict(dlogits=None), dict(inv_t=0.0), dict(inv_t=float("nan")),
           dict(logits=s.data_ptr() + 2), dict(dlogits=s.data_ptr() + V)]   # misaligned; overlapping without being equal
    for kw in bad:
        assert call(**kw) != 0, kw
        assert b"obte_distill_ce_rows" in lib.obte_last_error(), (kw, lib.obte_last_error())
    torch.cuda.synchronize()
    assert (out == 7.0).all() and (dl.float() == 3.0).all()          # nothing was launched
    assert call() == 0
    torch.cuda.synchronize()
    assert (dl.float() != 3.0).all()
    with pytest.raises(RuntimeError):
        ops().distill_ce_rows(s, t[:, :256].contiguous(), tgt, 1)
    with pytest.raises(RuntimeError):
        ops().distill_ce_rows(s.float(), t, tgt, 1)
    with pytest.raises(ValueError):
        ops().distill_ce_rows(s, t, tgt, 1, alpha=2.0)
