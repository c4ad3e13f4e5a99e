"""Causal-LM training, the host side (no GPU): which positions the next-token objective scores (train_encoder.next_token_rows and its
tensor-op fallback), the step plan under objective="clm", the float64 distillation rule (distill.distill_reference) and the refusals
of TrainStep(objective="clm") / a teacher — all of which raise before anything could be launched."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from omnibiote_amd import train_encoder as TE
from omnibiote_amd.distill import distill_loss_float64, distill_reference

EOS, PAD, TAG = TE.EOS_TOKEN, TE.PAD_TOKEN, TE.DNA_TAG


# ----------------------------------------------------------------------------------------------- scored positions
def test_two_documents_and_a_pad_tail():
    #             t:  0    1   2   3    4    5   6    7    8    9
    ids = np.array([[TAG, 20, 21, EOS, TAG, 30, 31, EOS, PAD, PAD]])
    rows, labels = TE.next_token_rows(ids, 1, 1)
    # 3 (an EOS: its successor opens another document) is not scored; 7 is an EOS AND stands before the PAD tail; 8, 9 are PAD / last
    assert rows[0].tolist() == [0, 1, 2, 4, 5, 6]
    assert labels[0].tolist() == [20, 21, EOS, 30, 31, EOS]          # EOS is a label at a document's last real token
    assert rows[0].dtype == np.int64 and labels[0].dtype == np.int64
    # a document cut by the PAD tail: the position before the first PAD is not scored
    ids = np.array([[TAG, 20, 21, 22, PAD, PAD]])
    rows, labels = TE.next_token_rows(ids, 1, 1)
    assert rows[0].tolist() == [0, 1, 2] and labels[0].tolist() == [20, 21, 22]


def test_all_pad_and_no_eos_rows():
    T = 9
    rows, labels = TE.next_token_rows(np.full((1, T), PAD), 1, 1)
    assert rows[0].size == 0 and labels[0].size == 0
    ids = np.arange(20, 20 + T).reshape(1, T)
    rows, labels = TE.next_token_rows(ids, 1, 1)
    assert rows[0].tolist() == list(range(T - 1)) and labels[0].tolist() == ids[0, 1:].tolist()


def _mixed_batch(rows=6, T=17, seed=0):
    rng = np.random.default_rng(seed)
    ids = rng.integers(20, 200, size=(rows, T))
    ids[0, 5] = EOS; ids[0, 6] = TAG
    ids[1, :] = PAD
    ids[2, 9] = EOS; ids[2, 10:] = PAD
    ids[3, T - 1] = EOS
    ids[4, 0] = EOS
    ids[5, 3] = EOS; ids[5, 4] = EOS
    return ids


def test_lists_are_ascending_per_micro_batch_with_labels_in_list_order():
    ids = _mixed_batch()
    T, mini, n_accum = ids.shape[1], 2, 3
    rows, labels = TE.next_token_rows(ids, mini, n_accum)
    assert len(rows) == len(labels) == n_accum
    for j in range(n_accum):
        mb = ids[j * mini:(j + 1) * mini]
        want = [b * T + t for b in range(mini) for t in range(T - 1)
                if mb[b, t] != EOS and mb[b, t] != PAD and mb[b, t + 1] != PAD]
        assert rows[j].tolist() == want                                 # ascending flat positions, counted within the micro-batch
        assert (np.diff(rows[j]) > 0).all()
        assert labels[j].tolist() == [int(mb[p // T, p % T + 1]) for p in want]
    # more rows than mini * n_accum: the tail is ignored, as TrainStep drops it
    rows2, _ = TE.next_token_rows(ids, mini, 2)
    assert [r.tolist() for r in rows2] == [r.tolist() for r in rows[:2]]
    with pytest.raises(ValueError):
        TE.next_token_rows(ids, 4, 2)


def test_tensor_op_fallback_gives_the_same_integers():
    ids = _mixed_batch(seed=3)
    rows, labels = TE.next_token_rows(ids, 2, 3)
    rows_t, labels_t = TE.next_token_rows_device(torch.from_numpy(ids), 2, 3)
    for j in range(3):
        assert rows_t[j].dtype == torch.int64 and labels_t[j].dtype == torch.int64
        assert rows_t[j].tolist() == rows[j].tolist() and labels_t[j].tolist() == labels[j].tolist()


# ------------------------------------------------------------------------------------------------------ step plan
def _attrs(**kw):
    d = dict(mini=4, per_pass=1, lm_head_impl="masked", loss_impl="fused", fused_loss_fn=None, mask_impl="ranges", pipeline_streams=2,
             backward_order="layer", sync_every=False, rows_forward=True, grad_accum="bf16")
    d.update(kw)
    return SimpleNamespace(**d)


@pytest.mark.parametrize("kw", [dict(), dict(per_pass=2), dict(lm_head_impl="dense", pipeline_streams=1), dict(grad_accum="fp32", per_pass=4)])
def test_step_plan_of_clm_is_the_mlm_plan(kw):
    old = TE.resolve_step_plan(_attrs(**kw), 32, True, False, True, env={})            # an object without the new attributes
    mlm = TE.resolve_step_plan(_attrs(objective="mlm", teacher=None, **kw), 32, True, False, True, env={})
    clm = TE.resolve_step_plan(_attrs(objective="clm", teacher=None, **kw), 32, True, True, True, env={})
    assert old == mlm
    assert clm == TE.resolve_step_plan(_attrs(**kw), 32, True, True, True, env={})
    assert TE.StepPlan._fields[:5] == ("rows", "n_accum", "sparse_rows", "readout", "rows_forward") and len(TE.StepPlan._fields) == 18


@pytest.mark.parametrize("kw", [dict(lm_head_impl="dense_full"), dict(loss_impl="torch"), dict(fused_loss_fn=lambda *a: None)])
def test_step_plan_refuses_clm_without_the_row_compact_readout(kw):
    with pytest.raises(ValueError, match="clm"):
        TE.resolve_step_plan(_attrs(objective="clm", **kw), 32, True, False, True, env={})
    assert not TE.resolve_step_plan(_attrs(objective="mlm", **kw), 32, True, False, True, env={}).sparse_rows


# ------------------------------------------------------------------------------------------- the float64 rule
def _rows(n=7, V=40, seed=0):
    g = torch.Generator().manual_seed(seed)
    s = (torch.randn(n, V, generator=g) * 2).to(torch.bfloat16)
    t = (torch.randn(n, V, generator=g) * 2).to(torch.bfloat16)
    tgt = torch.randint(0, V, (n,), generator=g)
    w = torch.rand(n, generator=g) + 0.1
    return s, t, tgt, w


def test_reference_at_alpha_one_is_cross_entropy():
    s, t, tgt, w = _rows()
    ref = distill_reference(s, t, tgt, n_accum=4, alpha=1.0, temperature=2.0)
    ce = torch.nn.functional.cross_entropy(s.double(), tgt, reduction="none")
    assert torch.allclose(ref.row_ce, ce, rtol=1e-12, atol=1e-12)
    assert torch.allclose(ref.loss, ce.mean() / 4, rtol=1e-12, atol=1e-12)
    sd = s.double().requires_grad_(True)
    (torch.nn.functional.cross_entropy(sd, tgt, reduction="mean") / 4).backward()
    assert torch.allclose(ref.dlogits, sd.grad, rtol=1e-10, atol=1e-14)
    refw = distill_reference(s, t, tgt, n_accum=4, row_weights=w, alpha=1.0)
    assert torch.allclose(refw.row_loss, w.double() * ce / 4, rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("temperature", [1.0, 2.0])
def test_reference_with_the_student_as_teacher_has_no_kl(temperature):
    s, _, tgt, _ = _rows(seed=1)
    ref = distill_reference(s, s.clone(), tgt, alpha=0.0, temperature=temperature)
    assert ref.row_kl.abs().max().item() <= 1e-14
    assert ref.dlogits.abs().max().item() == 0.0 and ref.loss.abs().item() <= 1e-14
    other = distill_reference(s, _rows(seed=2)[1], tgt, alpha=0.0, temperature=temperature)
    assert (other.row_kl > 0).all()                                    # (and a different teacher does have one)


@pytest.mark.parametrize("alpha,temperature,weighted", [(0.5, 1.0, False), (0.5, 2.0, True), (0.0, 2.0, False), (0.3, 0.7, True)])
def test_reference_gradient_is_autograds(alpha, temperature, weighted):
    s, t, tgt, w = _rows(seed=4)
    n_accum = 4
    ref = distill_reference(s, t, tgt, n_accum=n_accum, row_weights=w if weighted else None, alpha=alpha, temperature=temperature)
    sd = s.double().requires_grad_(True)
    row_loss, ce, kl = distill_loss_float64(sd, t, tgt, ref.row_weight, alpha, temperature)
    row_loss.sum().backward()
    assert torch.allclose(ref.dlogits, sd.grad, rtol=1e-9, atol=1e-15)
    assert torch.allclose(ref.row_loss, row_loss.detach(), rtol=1e-12, atol=0) and torch.allclose(ref.loss, row_loss.sum().detach(), rtol=1e-12, atol=0)
    want_w = w.double() / n_accum if weighted else torch.full((s.shape[0],), 1.0 / (s.shape[0] * n_accum), dtype=torch.float64)
    assert torch.allclose(ref.row_weight, want_w, rtol=1e-15, atol=0)
    # the KL of the rule is torch's own kl_div of the two softened distributions
    kd = torch.nn.functional.kl_div(torch.log_softmax(s.double() / temperature, -1), torch.softmax(t.double() / temperature, -1), reduction="none").sum(-1)
    assert torch.allclose(ref.row_kl, kd, rtol=1e-10, atol=1e-14)
    assert ref.dlogits.sum(dim=1).abs().max().item() <= 1e-15


def test_reference_refuses_bad_settings():
    s, t, tgt, _ = _rows()
    for kw in (dict(alpha=-0.1), dict(alpha=1.5), dict(temperature=0.0), dict(temperature=float("inf"))):
        with pytest.raises(ValueError):
            distill_reference(s, t, tgt, **kw)
    with pytest.raises(ValueError):
        distill_reference(s, t[:, :8], tgt)


# ------------------------------------------------------------------------------------------------------ refusals
def _model(autoregressive=True, vocab=64, n_embd=32):
    from omnibiote_amd.model import OmniBioTA, OmniBioTAConfig
    c = OmniBioTAConfig()
    c.block_size, c.vocab_size, c.n_layer, c.n_head, c.n_embd, c.dropout, c.flash = 16, vocab, 1, 2, n_embd, 0.0, True
    c.autoregressive = autoregressive
    return OmniBioTA(c)


def _step(model, **kw):
    return TE.TrainStep(model, torch.optim.SGD(model.parameters(), lr=0.0), None, mini_batch_size=2, n_head=2, **kw)


def test_refusals_raise_before_anything_runs():
    student = _model()
    assert _step(student, objective="clm").objective == "clm"                       # the accepted forms construct (nothing is launched)
    teacher = _model(n_embd=64)
    teacher.train()
    st = _step(student, objective="clm", teacher=teacher, distill_alpha=0.25, distill_temperature=2.0)
    assert st.teacher is teacher and not teacher.training                          # put in eval()
    assert _step(_model(autoregressive=False)).objective == "mlm"
    with pytest.raises(ValueError, match="objective"):
        _step(student, objective="lm")
    with pytest.raises(ValueError, match="teacher"):                               # a teacher with objective="mlm"
        _step(student, teacher=teacher)
    with pytest.raises(ValueError, match="vocabulary"):
        _step(student, objective="clm", teacher=_model(vocab=128))
    with pytest.raises(ValueError, match="teacher"):                               # a teacher that is not autoregressive
        _step(student, objective="clm", teacher=_model(autoregressive=False))
    with pytest.raises(ValueError, match="dense_full"):
        _step(student, objective="clm", lm_head_impl="dense_full")
    with pytest.raises(ValueError, match="fused"):                                 # a stub loss
        _step(student, objective="clm", fused_loss_fn=lambda *a: None)
    with pytest.raises(ValueError, match="fused"):
        _step(student, objective="clm", loss_impl="torch")
    with pytest.raises(ValueError, match="autoregressive"):
        _step(_model(autoregressive=False), objective="clm")
    with pytest.raises(ValueError):
        _step(student, objective="clm", teacher=teacher, distill_alpha=1.5)
    with pytest.raises(ValueError):
        _step(student, objective="clm", teacher=teacher, distill_temperature=0.0)


def test_a_live_object_is_checked_again_at_the_call():
    """The public attributes may be reassigned between steps: the refusals hold at the first call too, before any launch (the batch is
    a CPU tensor here: anything launched would fail differently)."""
    ids = torch.randint(20, 60, (4, 16))
    st = _step(_model(), objective="clm")
    st.lm_head_impl = "dense_full"
    with pytest.raises(ValueError, match="dense_full"):
        st(ids)
    st = _step(_model(), objective="clm")
    st.teacher = _model(vocab=128)
    with pytest.raises(ValueError, match="vocabulary"):
        st(ids)
    st = _step(_model())
    st.objective = "clm"
    st._core.config.autoregressive = False
    with pytest.raises(ValueError, match="autoregressive"):
        st(ids)
    with pytest.raises(ValueError, match="mlm_mask"):
        _step(_model(), objective="clm")(ids, mlm_mask=torch.zeros(4, 16, dtype=torch.bool))


def test_trainer_flags():
    a = TE.parse_args([])
    assert (a.objective, a.distill_from, a.teacher_n_layer, a.teacher_n_embd, a.teacher_n_head, a.distill_alpha, a.distill_temperature) == \
        ("mlm", "", 0, 0, 0, 0.5, 1.0)
    a = TE.parse_args(["--objective", "clm", "--distill_from", "t.pt", "--teacher_n_layer", "12", "--distill_alpha", "0.1", "--distill_temperature", "2"])
    assert (a.objective, a.distill_from, a.teacher_n_layer, a.distill_alpha, a.distill_temperature) == ("clm", "t.pt", 12, 0.1, 2.0)
    with pytest.raises(SystemExit):
        TE.parse_args(["--objective", "prefix"])
    small = ["--n_embd", "48", "--n_head", "2", "--n_layer", "1", "--ctx_len", "16"]
    assert TE.build_model(TE.parse_args(small + ["--objective", "clm"]), "cpu", vocab_size=64).config.autoregressive is True
    assert TE.build_model(TE.parse_args(small), "cpu", vocab_size=64).config.autoregressive is False
    with pytest.raises(ValueError, match="clm"):
        TE.load_teacher(TE.parse_args(["--distill_from", "t.pt"]), None, "cpu")
