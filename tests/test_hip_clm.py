"""Causal-LM training on the GPU: TrainStep(objective="clm") and its distillation form against the CPU oracle, the relations the MLM
step's tests assert (pipelined = single stream bitwise, k micro-batches per pass = separate passes, host copy or not), evaluate()
under --objective clm, and the loop the objective exists for: train a model, then generate from it.
All at test_readout_paths_match_the_oracle_loss_and_gradients's shape: C 128, H 2, 2 layers, V 512, T 64, 8 rows, micro-batch 4, rows
that pack several documents.  (The pipelining relation also runs at micro-batch 2: a step of two passes is never pipelined.)"""
import warnings
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import omnibiote_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF = torch.bfloat16
C, H, LYR, V, T, ROWS, MINI = 128, 2, 2, 512, 64, 8, 4
LOSS_BAR, REL_BAR, COS_BAR = 0.02, 0.05, 0.998      # that test's own


def TE():
    from omnibiote_amd import train_encoder
    return train_encoder


def build(w, n_embd=C, n_head=H, n_layer=LYR, autoregressive=True):
    from omnibiote_amd.model import OmniBioTA, OmniBioTAConfig
    from omnibiote_amd.mup_compat import set_base_shapes
    c = OmniBioTAConfig(); c.block_size, c.vocab_size, c.n_layer, c.n_head, c.n_embd, c.dropout, c.flash = T, V, n_layer, n_head, n_embd, 0.0, True
    c.autoregressive = autoregressive
    m = OmniBioTA(c)
    cb = OmniBioTAConfig(); cb.block_size, cb.vocab_size, cb.n_layer, cb.dropout, cb.flash = T, V, n_layer, 0.0, True
    cb.autoregressive = autoregressive
    cb.n_embd, cb.n_head = 24, 3
    base = OmniBioTA(cb)
    cb.n_embd, cb.n_head = 48, 12
    delta = OmniBioTA(cb)
    set_base_shapes(m, base, delta=delta, rescale_params=False)
    m.load_state_dict(w, strict=False)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        m.to(BF)
    return m.to(DEV)


def sgd_step(m, **kw):
    kw.setdefault("mini_batch_size", MINI)
    return TE().TrainStep(m, torch.optim.SGD(m.parameters(), lr=0.0), None, n_head=H, max_grad_norm=1e9, objective="clm", **kw)


def grads(m):
    return {k: p.grad.clone() for k, p in m.named_parameters()}


_shared = {}


def batch():
    """The batch of every test here (made once): multi-document rows, with documents that certainly end inside rows."""
    if "ids" not in _shared:
        ids = TE().synthetic_rows(ROWS, T, V, np.random.default_rng(0), single_document=False)
        ids[1, 20] = R.EOS_TOKEN; ids[1, 21] = 4
        ids[5, 40] = R.EOS_TOKEN
        ids[6, 10] = R.EOS_TOKEN; ids[6, 30] = R.EOS_TOKEN
        assert (ids[:, 1:-1] == R.EOS_TOKEN).any(axis=1).sum() >= 3
        _shared["ids"] = ids
    return _shared["ids"]


def weights():
    if "w" not in _shared:
        _shared["w"] = R.hash_weights(R.RefConfig(block_size=T, vocab_size=V, n_layer=LYR, n_head=H, n_embd=C))
    return _shared["w"]


CT, HT = 256, 2          # the teacher: another width, hash weights from another seed


def teacher_weights():
    if "wt" not in _shared:
        _shared["wt"] = R.hash_weights(R.RefConfig(block_size=T, vocab_size=V, n_layer=LYR, n_head=HT, n_embd=CT), seed=1)
    return _shared["wt"]


def oracle(distill=None):
    """(loss, {name: gradient}) of the oracle route, computed once per form and left unchanged: R.model_forward under the dense form of
    the same document-causal mask, R.readout, the next-token loss over next_token_rows' positions in fp32 — or, distill = (alpha,
    temperature), both forwards in fp32 and the float64 rule's loss — accumulated over the micro-batches."""
    key = ("oracle", distill)
    if key in _shared:
        return _shared[key]
    from omnibiote_amd.distill import distill_loss_float64
    from omnibiote_amd.masks import RangeMask
    ids = torch.from_numpy(batch())
    cfg = R.RefConfig(block_size=T, vocab_size=V, n_layer=LYR, n_head=H, n_embd=C)
    wb = {k: v.to(BF).float().requires_grad_(True) for k, v in weights().items()}
    rope = R.cast_rope_table(R.rope_table(C // H, T), BF)
    n_accum = ROWS // MINI
    rows, labels = TE().next_token_rows(batch(), MINI, n_accum)
    total = 0.0
    for j in range(n_accum):
        sl = slice(j * MINI, (j + 1) * MINI)
        dense = RangeMask.from_tokens(ids[sl], causal=True).dense(torch.float32).unsqueeze(1)
        logits = R.model_forward(wb, cfg, ids[sl], dense, rope=rope)
        pos, lab = torch.from_numpy(rows[j]), torch.from_numpy(labels[j])
        if distill is None:
            scored = torch.zeros(MINI * T, dtype=torch.bool)
            scored[pos] = True
            target = torch.zeros(MINI * T, dtype=torch.int64)
            target[pos] = lab
            lj = R.masked_lm_loss(logits, target, scored, n_accum)
        else:
            cfg_t = R.RefConfig(block_size=T, vocab_size=V, n_layer=LYR, n_head=HT, n_embd=CT)
            wt = {k: v.to(BF).float() for k, v in teacher_weights().items()}
            with torch.no_grad():
                t_logits = R.model_forward(wt, cfg_t, ids[sl], dense, rope=R.cast_rope_table(R.rope_table(CT // HT, T), BF))
            w_row = torch.full((pos.numel(),), 1.0 / (n_accum * pos.numel()), dtype=torch.float64)
            row_loss, _, _ = distill_loss_float64(logits.reshape(-1, V)[pos], t_logits.reshape(-1, V)[pos], lab, w_row, *distill)
            lj = row_loss.sum()
        lj.backward()
        total += lj.item()
    _shared[key] = (total, {k: v.grad.clone() for k, v in wb.items()})
    return _shared[key]


def assert_matches(m, loss, want_loss, want_grads, what):
    assert abs(loss - want_loss) <= LOSS_BAR, (what, loss, want_loss)
    for k, p in m.named_parameters():
        got, want = p.grad.float().cpu().flatten(), want_grads[k].float().cpu().flatten()
        rel = (got - want).norm().item() / (want.norm().item() + 1e-12)
        cos = torch.dot(got, want).item() / (got.norm().item() * want.norm().item() + 1e-30)
        assert rel <= REL_BAR and cos >= COS_BAR, (what, k, rel, cos)


# ---------------------------------------------------------------------------------------------------- oracle parity
@pytest.mark.parametrize("impl", ["masked", "dense"])
def test_clm_step_matches_the_oracle_loss_and_gradients(impl):
    ref_loss, ref_grads = oracle()
    m = build(weights())
    step = sgd_step(m, lm_head_impl=impl)
    out = step(torch.from_numpy(batch()).to(DEV), input_ids_host=batch())
    assert set(out) == {"loss", "tokens"}
    assert_matches(m, out["loss"].item(), ref_loss, ref_grads, impl)
    # the lists the step worked from are next_token_rows'
    rows, _ = TE().next_token_rows(batch(), MINI, ROWS // MINI)
    assert [r.tolist() for r in step._mask_rows_host] == [r.tolist() for r in rows]


def test_clm_step_of_an_empty_micro_batch_gives_every_parameter_a_gradient():
    ids = batch().copy()
    ids[MINI:] = TE().EOS_TOKEN                      # nothing to score in the second micro-batch
    m = build(weights())
    out = sgd_step(m)(torch.from_numpy(ids).to(DEV), input_ids_host=ids)
    assert torch.isfinite(out["loss"]).item()
    assert all(p.grad is not None and torch.isfinite(p.grad.float()).all() for p in m.parameters())


# -------------------------------------------------------------------------------- the relations the MLM tests assert
@pytest.mark.parametrize("mini,distill", [(4, False), (2, False), (2, True)])
def test_clm_pipelined_step_is_bitwise_the_single_stream_step(mini, distill):
    ids = torch.from_numpy(batch()).to(DEV)
    out = {}
    for streams in (1, 2):
        m = build(weights())
        kw = dict(teacher=build(teacher_weights(), CT, HT), distill_alpha=0.5, distill_temperature=2.0) if distill else {}
        step = sgd_step(m, mini_batch_size=mini, pipeline_streams=streams, **kw)
        res = step(ids, input_ids_host=batch())
        torch.cuda.synchronize()
        out[streams] = ({k: v.clone() for k, v in res.items()}, grads(m))
    assert torch.equal(out[1][0]["tokens"], out[2][0]["tokens"])
    for k in set(out[1][0]) - {"tokens"}:   # the reported scalars are summed per stream first: equal up to fp32 rounding, as in the MLM test
        a, b = out[1][0][k].item(), out[2][0][k].item()
        assert abs(a - b) <= 1e-5 * abs(a), (k, a, b)
    for k in out[1][1]:
        assert torch.equal(out[1][1][k], out[2][1][k]), k


def test_clm_micro_batches_per_pass_gives_the_step_of_separate_passes():
    ref_loss, ref_grads = oracle()
    ids = torch.from_numpy(batch()).to(DEV)
    out = {}
    for k in (1, 2):
        m = build(weights())
        loss = sgd_step(m, micro_batches_per_pass=k)(ids, input_ids_host=batch())["loss"].item()
        out[k] = (loss, {n: p.grad.float().cpu().clone() for n, p in m.named_parameters()})
    assert abs(out[1][0] - out[2][0]) <= 2e-3 and abs(out[2][0] - ref_loss) <= LOSS_BAR, (out[1][0], out[2][0], ref_loss)
    for n in out[1][1]:
        a, b, ref = out[2][1][n].flatten(), out[1][1][n].flatten(), ref_grads[n].flatten()
        assert ((a - b).norm() / (b.norm() + 1e-12)).item() <= 0.02, n
        cos = (torch.dot(a, ref) / (a.norm() * ref.norm() + 1e-30)).item()
        assert cos >= COS_BAR and ((a - ref).norm() / (ref.norm() + 1e-12)).item() <= REL_BAR, (n, cos)


def test_clm_step_with_and_without_the_host_copy_is_the_same():
    out = {}
    for tag in ("device", "host"):
        m = build(weights())
        step = sgd_step(m)
        losses = []
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")           # (the one-time "no input_ids_host" warning)
            for _ in range(2):                        # twice: the pinned buffers are reused
                losses.append(step(torch.from_numpy(batch()).to(DEV), input_ids_host=batch() if tag == "host" else None)["loss"].item())
        out[tag] = (losses, grads(m))
    assert out["device"][0] == out["host"][0]
    for k in out["device"][1]:
        assert torch.equal(out["device"][1][k], out["host"][1][k]), k


# ------------------------------------------------------------------------------------------ distillation through the step
@pytest.mark.parametrize("impl", ["masked", "dense"])
def test_distilled_step_matches_the_oracle(impl):
    alpha, temperature = 0.5, 2.0
    ref_loss, ref_grads = oracle((alpha, temperature))
    m, teacher = build(weights()), build(teacher_weights(), CT, HT)
    step = sgd_step(m, lm_head_impl=impl, teacher=teacher, distill_alpha=alpha, distill_temperature=temperature)
    out = step(torch.from_numpy(batch()).to(DEV), input_ids_host=batch())
    assert_matches(m, out["loss"].item(), ref_loss, ref_grads, impl)
    assert all(p.grad is None for p in teacher.parameters()) and not teacher.training
    # "ce" and "kl" are normalised like "loss": loss = alpha ce + (1 - alpha) temperature^2 kl
    ce, kl = out["ce"].item(), out["kl"].item()
    assert abs(alpha * ce + (1 - alpha) * temperature ** 2 * kl - out["loss"].item()) <= 1e-4 * abs(out["loss"].item()) + 1e-6
    assert abs(ce - oracle()[0]) <= LOSS_BAR and kl > 0


def test_distill_alpha_one_gives_the_gradients_of_no_teacher():
    ids = torch.from_numpy(batch()).to(DEV)
    plain = build(weights())
    loss_plain = sgd_step(plain)(ids, input_ids_host=batch())["loss"].item()
    m, teacher = build(weights()), build(teacher_weights(), CT, HT)
    out = sgd_step(m, teacher=teacher, distill_alpha=1.0, distill_temperature=2.0)(ids, input_ids_host=batch())
    assert_matches(m, out["loss"].item(), loss_plain, {k: p.grad for k, p in plain.named_parameters()}, "alpha = 1")
    assert abs(out["ce"].item() - loss_plain) <= LOSS_BAR
    assert all(p.grad is None for p in teacher.parameters())


# -------------------------------------------------------------------------------------------------------- evaluate
def test_evaluate_under_clm_is_the_next_token_loss():
    from omnibiote_amd import ops
    m = build(weights())
    ids = torch.from_numpy(TE().synthetic_rows(MINI, T, V, np.random.default_rng(7), single_document=True)).to(DEV)
    args = SimpleNamespace(mini_batch_size=MINI, use_padding=False, objective="clm")
    got = TE().evaluate(m, [("held_out", lambda n: ids[:n])], args, 1, DEV)["held_out"]
    with torch.no_grad():
        want = ops.next_token_loss(m(ids), ids).item()
    assert abs(got - want) <= LOSS_BAR, (got, want)
    assert m.training                                 # evaluate() puts the mode back


# ------------------------------------------------------------------------------------------- train, then generate
N_BODY, FIRST_BODY = 64, 20
TRAIN_STEPS = 8            # twice the measured 4: see the test's docstring
TRAIN_LR = 1e-2


def permutation_rows(rng, f, rows):
    """Rows of packed documents ``tag, x0, f(x0), f(f(x0)), ..., EOS`` with 24-40 body tokens each (more than the test generates, so
    that a document's end is never the next token within the generated stretch)."""
    out = np.empty((rows, T), dtype=np.int64)
    for r in range(rows):
        pos = 0
        while pos < T:
            n = int(rng.integers(24, 41))
            doc = np.empty(n + 2, dtype=np.int64)
            doc[0], doc[-1] = TE().DNA_TAG, TE().EOS_TOKEN
            x = FIRST_BODY + int(rng.integers(N_BODY))
            for i in range(n):
                doc[1 + i] = x
                x = f[x - FIRST_BODY]
            take = min(len(doc), T - pos)
            out[r, pos:pos + take] = doc[:take]
            pos += take
    return out


def train_then_generate(steps, check_every=None):
    """Trains for `steps` steps; returns the first step count at which the generation follows f exactly (checked every `check_every`
    steps, and at the end), or None."""
    from omnibiote_amd.mup_compat import mu_param_groups
    rng = np.random.default_rng(11)
    f = FIRST_BODY + rng.permutation(N_BODY)
    m = build(weights())
    opt = TE().FusedAdamW(mu_param_groups(list(m.parameters()), TRAIN_LR, 0.0), lr=TRAIN_LR, betas=(0.9, 0.99), eps=1e-8, weight_decay=0.0)
    step = TE().TrainStep(m, opt, None, mini_batch_size=MINI, n_head=H, objective="clm")
    prompt = torch.from_numpy(FIRST_BODY + rng.choice(N_BODY, size=8, replace=False)).view(8, 1).to(DEV)
    want = np.empty((8, 17), dtype=np.int64)
    want[:, 0] = prompt.view(-1).cpu().numpy()
    for t in range(16):
        want[:, t + 1] = f[want[:, t] - FIRST_BODY]

    def follows():
        return np.array_equal(m.generate(prompt, 16, top_k=1).cpu().numpy(), want)

    for s in range(1, steps + 1):
        host = permutation_rows(rng, f, ROWS)
        step(torch.from_numpy(host).to(DEV), input_ids_host=host)
        if (check_every and s % check_every == 0 or s == steps) and follows():
            return s
    return None


def test_train_with_the_next_token_objective_then_generate():
    """The loop the objective closes: documents follow a fixed permutation f of 64 body ids (tok[t + 1] = f(tok[t])); after training
    the 2-layer model with TrainStep(objective="clm"), greedy generation from eight one-token prompts follows f for 16 tokens.
    Measured (checked after every step): the generation first follows f after 4 optimizer steps of 8 rows at lr 1e-2 — Adam's
    sign-like first updates are enough for a 64-entry lookup; TRAIN_STEPS is twice that."""
    assert train_then_generate(TRAIN_STEPS) == TRAIN_STEPS
