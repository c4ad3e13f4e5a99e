"""Drop-in replacement for the reference's ``training/model.py`` class surface, computed by hand-written HIP.

Same names, constructor RNG order, attribute tree and state_dict keys as the reference
(training/model.py:63-277), so ``train_encoder.py`` and the eval scripts can ``from model import OmniBioTA,
OmniBioTAConfig`` unchanged (``training/model.py`` in this repo re-exports this module).  What differs is what
runs underneath: every block forward/backward is one call into ``libomnibiote_hip.so``.

Contract notes (each mirrors a reference behaviour):
  * ``OmniBioTAConfig`` has no ``flash`` field; callers assign it ad hoc (train_encoder.py:152).  Reading it
    when absent raises AttributeError exactly like the reference.
  * ``freqs_cis`` is a persistent complex64 buffer.  ``module.to(torch.bfloat16)`` turns it into a real bf16
    tensor holding cos only (PyTorch semantics), and the reference then *scales* pairs instead of rotating
    them.  This module reproduces both modes from the buffer's dtype: complex -> rotation, real -> cos-only.
  * softmax scale is 8 / n_embd (model.py:119), GELU uses erf(x / 1.41421) (model.py:25), LayerNorm eps 1e-5.
  * The HIP path computes in bf16 with fp32 accumulation — the regime the reference trains and evaluates in
    (train_encoder.py:21,170).  Parameters must be bf16 on a GPU at forward time; anything else raises.
  * dropout (embedding, attention probabilities, both residual projections; model.py:83-84,160,204) is fused
    into the kernels with a counter-based mask: same distribution and scaling as nn.Dropout, but necessarily a
    different random stream than PyTorch's generator.  Each forward draws its seeds from torch's CPU generator, so
    ``torch.manual_seed`` makes runs reproducible and activation checkpointing recomputes identical masks.
  * ``OmniBioTAConfig.autoregressive`` follows the reference, quirk included (model.py:115-146): without an ``attn_mask`` the
    attention is causal (SDPA's is_causal=True / the tril ``bias``) — here the causal RANGE mask, a pair of int32 tables that
    ``OmniBioTA.forward`` builds once per call (one launch, shared by all layers); WITH an ``attn_mask`` the reference applies that
    mask alone and is NOT causal (is_causal=False), and so is this module, with a warning.  A caller who wants a document mask
    and causality passes ``masks.RangeMask.from_tokens(ids, causal=True)``, under either setting of the flag.
"""
from __future__ import annotations

import math
import operator
import warnings
import weakref
from dataclasses import dataclass
from typing import Optional, Tuple

import torch
import torch.nn as nn
from torch.utils.checkpoint import checkpoint

from . import _lib as L
from . import ops
from .generation import (  # noqa: F401  (the generation state lives there; every name stays importable from this module)
    BeamResult, CachePositions, DecodeLoop, KVCache, PagedKVCache, PagedPositions, QuantizedWeights, SequenceScore, SharedPrefixCache, TokenConstraint,
    TokenPenalty, _check_lengths, _check_prompt, _check_room, _check_top_p, _checked_weights, _default_pad, _device_uniforms, _live, _next_tokens,
    _refuse_paged, _refuse_weights, _require_hip, _restriction, _round_restriction, _step_restriction, ragged_output, sample_next)

try:  # the real package, if the environment has it (README.md:16 pins mup==1.0.0)
    from mup import MuReadout as _MuReadoutBase  # type: ignore
    _HAVE_MUP = True
except Exception:  # not installed here: restated semantics, see mup_compat.py
    from .mup_compat import MuReadout as _MuReadoutBase
    _HAVE_MUP = False


# ------------------------------------------------------------------------------------------------ helper functions
def fused_gelu(x: torch.Tensor) -> torch.Tensor:
    """x * 0.5 * (1 + erf(x / 1.41421))  (model.py:23-25).  Tensor-level helper kept for API parity; inside the
    block the same formula runs in the c_fc GEMM epilogue."""
    return x * 0.5 * (1.0 + torch.erf(x / 1.41421))


def precompute_freqs_cis(dim: int, end: int, theta: float = 10000.0) -> torch.Tensor:
    """complex64 (end, dim/2) table of unit phasors exp(i t theta^(-2j/dim))  (model.py:53-61)."""
    inv_freq = 1.0 / (theta ** (torch.arange(0, dim, 2)[: dim // 2].float() / dim))
    angles = torch.outer(torch.arange(end), inv_freq).float()
    return torch.polar(torch.ones_like(angles), angles)


def reshape_for_broadcast(freqs_cis: torch.Tensor, x: torch.Tensor) -> torch.Tensor:
    """(model.py:28-35) view the first x.shape[1] rows of the table as (1, T, 1, hs/2)."""
    assert freqs_cis.shape[-1] == x.shape[-1]
    f = freqs_cis[: x.shape[1]]
    return f.view(*[d if i in (1, x.ndim - 1) else 1 for i, d in enumerate(x.shape)])


def rope_tables(freqs_cis: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """fp32 (cos, sin) tables the kernels consume.  A real-valued buffer (after ``.to(bfloat16)``) yields
    sin = 0: the reference's degenerate cos-only scaling, including the bf16 rounding of cos."""
    if freqs_cis.is_complex():
        return freqs_cis.real.float().contiguous(), freqs_cis.imag.float().contiguous()
    c = freqs_cis.float().contiguous()
    return c, torch.zeros_like(c)


def apply_rotary_emb(xq: torch.Tensor, xk: torch.Tensor, freqs_cis: torch.Tensor):
    """(model.py:39-50) on (B, T, H, hs) tensors; runs the HIP RoPE kernel on a packed copy."""
    B, T, H, hs = xq.shape
    cos, sin = rope_tables(freqs_cis.to(xq.device))
    packed = torch.cat([xq.reshape(B, T, H * hs), xk.reshape(B, T, H * hs), torch.zeros_like(xq).reshape(B, T, H * hs)], dim=2)
    packed = packed.to(torch.bfloat16).contiguous()
    ops.rope_qk_(packed, cos, sin, B, T, H, hs)
    q, k, _ = packed.split(H * hs, dim=2)
    return q.reshape(B, T, H, hs).type_as(xq), k.reshape(B, T, H, hs).type_as(xk)


def _warn_mask_not_causal() -> None:
    """One place, so that Python's default filter shows it once per process."""
    warnings.warn("autoregressive=True with an explicit attn_mask: the mask alone is applied and the attention is NOT causal, as in "
                  "the reference (model.py:131-145, is_causal=False). Pass masks.RangeMask.from_tokens(ids, causal=True) for a "
                  "document mask and causality.", UserWarning)


def _autoregressive_mask(autoregressive: bool, attn_mask, B: int, T: int, device):
    """What an autoregressive module attends under (the reference's rule): no mask given -> the causal range mask, built here;
    a mask given -> that mask alone.  ``attn_mask`` may already be a resolved ops.MaskSpec (OmniBioTA.forward hands its blocks one)."""
    if not autoregressive:
        return attn_mask
    if attn_mask is None:
        from .masks import RangeMask
        return RangeMask.causal(B, T, device)
    if not isinstance(attn_mask, ops.MaskSpec):
        _warn_mask_not_causal()
    return attn_mask


# ------------------------------------------------------------------------------------------ in-place grad accumulation
# How the backward of a micro-batch delivers its weight gradients is a property of the TRAINING STEP that built the graph,
# not of the process: each autograd node below captures the active ``GradPolicy`` snapshot at FORWARD time (``ctx.pol``) and
# its backward — which PyTorch runs on an autograd-engine thread — reads only that.  Two TrainSteps on two models in one
# process, or forward passes issued from different threads, therefore cannot see each other's switches (a context variable
# selects the snapshot; nothing here is a mutable module global).
#   accumulate: the backward of the big matrices adds straight into an existing ``param.grad`` (the wgrad GEMM's epilogue /
#       the embedding scatter do the read-modify-write) and hands autograd ``None`` for them, which removes the separate
#       ``grad += new`` pass over 470 MB per micro-batch.  The arithmetic is the one autograd would do (bf16(old +
#       bf16(new))).  Only valid while nothing needs to observe per-micro-batch gradients: the harness sets it for the
#       micro-batches that run under DDP's no_sync(), never for the last one (whose AccumulateGrad hooks feed the reducer).
#   ln_mode: LayerNorm weight gradients over micro-batches: instead of one reduction launch + one bf16 ``grad += new`` per
#       LayerNorm and micro-batch (17 LayerNorms x 16 micro-batches on the small config), the per-workgroup partial sums are
#       carried in a persistent fp32 buffer per weight (L.LN_PARTIAL_FIRST on the first such micro-batch, _MORE after it) and
#       reduced ONCE, by the micro-batch that runs with L.LN_PARTIAL_LAST and hands the total to autograd.  0 = off.  The
#       total is bf16(sum in fp32) — closer to the exact gradient than autograd's running bf16 sum, not bitwise equal to it.
#   store: who owns those fp32 buffers (one ``LnPartialStore`` per TrainStep; a process-wide default for bare uses of the
#       context manager).
#   acc32_mode: every WEIGHT gradient (the blocks' four matrices, the readout, the embedding) summed in fp32 over the passes of one
#       optimizer step, opt-in: each weight has a persistent fp32 buffer of its own shape in ``acc32_store`` (a ``Fp32GradStore``);
#       the pass with L.ACC32_FIRST stores its contribution there before any rounding to bf16, L.ACC32_MORE adds, L.ACC32_LAST
#       adds and hands bf16(buffer) to autograd — ``param.grad`` stays None until then and is rounded once.  0 = off.  Replaces
#       ``accumulate`` (both at once is an error); the LayerNorm weights go with ``ln_mode``, which the harness starts at the
#       first pass in this mode.
import contextvars
import os


class _ParamKeyedStore:
    """fp32 scratch buffers keyed by a parameter's identity (not an attribute of the parameter or the module: whole-object pickles
    of the model — the reference's checkpoint format — must not carry them), one weak reference per entry, released when the
    parameter dies.  A subclass supplies the buffer (``_new``) and whether an existing one still serves (``_fits``)."""

    def __init__(self):
        self._bufs = {}   # id(weight) -> (weak reference to it, buffer)

    def get(self, param):
        key = id(param)
        ent = self._bufs.get(key)
        if ent is not None and ent[0]() is param and ent[1].device == param.device and self._fits(ent[1], param):
            return ent[1]
        buf = self._new(param)
        bufs = self._bufs
        self._bufs[key] = (weakref.ref(param, lambda _r, k=key: bufs.pop(k, None)), buf)
        return buf

    def __len__(self):
        return len(self._bufs)


class LnPartialStore(_ParamKeyedStore):
    """fp32 partial-sum buffers of LayerNorm weights (2 MB of scratch per weight)."""

    def _new(self, param):
        return ops.ln_partials_buffer(param.numel(), param.device)

    def _fits(self, buf, param):
        return buf.numel() == L.lib().obte_layernorm_bwd_ws_rows() * param.numel()


class Fp32GradStore(_ParamKeyedStore):
    """fp32 buffers of the weights whose gradients are summed in fp32 over the passes of a step (GradPolicy.acc32_mode), one of
    the parameter's shape each (4 bytes per parameter).  Scratch within one optimizer step: the first pass overwrites, nothing
    reads it later."""

    def _new(self, param):
        return torch.empty(param.shape, dtype=torch.float32, device=param.device)

    def _fits(self, buf, param):
        return buf.shape == param.shape


class BackwardOrder:
    """Cross-stream ordering of the backward passes of consecutive micro-batches, PER PARAMETER GROUP instead of per pass.
    Backward passes that run on different HIP streams read-modify-write the same gradient buffers (in-place accumulation, the
    LayerNorm partial sums); what has to be ordered is each buffer's own sequence of updates, not the passes as wholes.  Every
    autograd node that owns parameters waits — on the stream it runs on — for the event the SAME node of the previous
    micro-batch recorded (``wait``), does its work, and records its own (``done``).  The backward of micro-batch j+1 can then
    follow that of micro-batch j one layer behind instead of starting after its last kernel; every buffer still sees the
    updates in micro-batch order, so results are bitwise those of one stream.  ``prev_events``: the ``events`` of the previous
    micro-batch's object (complete on the host by the time this pass's backward is issued: the harness issues backward passes
    in order); ``fallback``: an event that covers the whole previous backward, for a node the previous pass did not run."""
    __slots__ = ("prev_events", "fallback", "events")

    def __init__(self, prev_events=None, fallback=None):
        self.prev_events, self.fallback, self.events = prev_events, fallback, {}

    def wait(self, key):
        ev = None if self.prev_events is None else self.prev_events.get(key)
        if ev is None:
            ev = self.fallback
        if ev is not None:
            torch.cuda.current_stream().wait_event(ev)

    def done(self, key):
        self.events[key] = torch.cuda.current_stream().record_event()


class GradPolicy:
    """Immutable snapshot of the switches above; what an autograd node keeps in ``ctx.pol``."""
    __slots__ = ("accumulate", "ln_mode", "store", "order", "acc32_mode", "acc32_store")

    def __init__(self, accumulate: bool = False, ln_mode: int = 0, store: Optional[LnPartialStore] = None, order: Optional[BackwardOrder] = None,
                 acc32_mode: int = 0, acc32_store: Optional[Fp32GradStore] = None):
        if acc32_mode and accumulate:
            raise ValueError("GradPolicy: acc32_mode (the fp32 sum) replaces accumulate (the bf16 sum in param.grad)")
        if acc32_mode not in (0, L.ACC32_FIRST, L.ACC32_MORE, L.ACC32_LAST):
            raise ValueError(f"GradPolicy: acc32_mode must be 0 or L.ACC32_*, got {acc32_mode}")
        object.__setattr__(self, "accumulate", bool(accumulate))
        object.__setattr__(self, "ln_mode", int(ln_mode))
        object.__setattr__(self, "store", store)
        object.__setattr__(self, "order", order)
        object.__setattr__(self, "acc32_mode", int(acc32_mode))
        object.__setattr__(self, "acc32_store", acc32_store)

    def __setattr__(self, *a):
        raise AttributeError("GradPolicy is immutable: enter accumulate_grads_inplace(...) for different switches")


_NO_POLICY = GradPolicy()
_policy = contextvars.ContextVar("obte_grad_policy", default=_NO_POLICY)
_default_store = LnPartialStore()
_default_acc32_store = Fp32GradStore()
_embedding_order = contextvars.ContextVar("obte_embedding_order", default=None)


def current_grad_policy() -> GradPolicy:
    """The snapshot an autograd node should capture in its forward (``ctx.pol = current_grad_policy()``)."""
    return _policy.get()


class accumulate_grads_inplace:
    """``with accumulate_grads_inplace(enabled, ln_partial_mode, store=...)``: graphs BUILT inside deliver their gradients
    that way when they run backward (inside the block or later, on whatever thread).  acc32_mode (L.ACC32_*) + acc32_store: the
    weight gradients are summed in fp32 instead (``enabled`` must then be False)."""

    def __init__(self, enabled: bool = True, ln_partial_mode: int = 0, store: Optional[LnPartialStore] = None, order: Optional[BackwardOrder] = None,
                 acc32_mode: int = 0, acc32_store: Optional[Fp32GradStore] = None):
        self.pol = GradPolicy(enabled, ln_partial_mode, store if store is not None else _default_store, order, acc32_mode,
                              (acc32_store if acc32_store is not None else _default_acc32_store) if acc32_mode else None)

    def __enter__(self):
        self.token = _policy.set(self.pol)
        return self

    def __exit__(self, *exc):
        _policy.reset(self.token)
        return False


class embedding_order:
    """``with embedding_order(order)``: the next OmniBioTA.forward in this context takes ``order`` (int32, a stable argsort of
    its flattened token ids) for its embedding backward instead of sorting the ids itself — a harness that sorts a whole
    optimizer step's ids in one call hands each micro-batch its slice this way.  Consumed by that forward."""

    def __init__(self, order):
        self.box = [order]

    def __enter__(self):
        self.token = _embedding_order.set(self.box)
        return self

    def __exit__(self, *exc):
        _embedding_order.reset(self.token)
        return False


def _ln_partials(param, pol: GradPolicy):
    """The persistent fp32 partial-sum buffer of a LayerNorm weight in the policy's store (created on first use)."""
    return (pol.store if pol.store is not None else _default_store).get(param)


def _grad_slot(param, pol: Optional[GradPolicy] = None):
    """The existing gradient of ``param`` if the node's policy says accumulate in place and that is applicable, else None.
    (The HIP entry points that receive it insist on bf16 themselves; the protocol is dtype-agnostic so that the CPU
    multi-process tests can drive it with a stub model.)"""
    if pol is None or not pol.accumulate:
        return None
    g = getattr(param, "grad", None)
    if g is None or g.dtype != param.dtype or not g.is_contiguous() or g.shape != param.shape:
        return None
    return g


def _acc32(param, pol: Optional[GradPolicy]):
    """(fp32 buffer of ``param``, mode) as the ops take them when the node's policy sums weight gradients in fp32, else (None, 0)."""
    if pol is None or not pol.acc32_mode:
        return None, 0
    return (pol.acc32_store if pol.acc32_store is not None else _default_acc32_store).get(param), pol.acc32_mode


class _ordered:
    """``with _ordered(pol, key)``: a node's update of the parameter group ``key`` under the policy's BackwardOrder, if it has one —
    wait for the previous pass's update of the group on entry, record this one's event on leaving (not when the body raised)."""
    __slots__ = ("order", "key")

    def __init__(self, pol: Optional[GradPolicy], key):
        self.order, self.key = (pol.order if pol is not None else None), key

    def __enter__(self):
        if self.order is not None:
            self.order.wait(self.key)

    def __exit__(self, exc_type, exc, tb):
        if self.order is not None and exc_type is None:
            self.order.done(self.key)


# ------------------------------------------------------------------------------------------------- autograd glue
class _LayerNormFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w):
        y, mean, rstd = ops.layernorm_fwd(x.contiguous(), w)
        ctx.save_for_backward(x, w, mean, rstd)
        ctx.w_param = w
        ctx.pol = current_grad_policy()
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w, mean, rstd = ctx.saved_tensors
        pol = ctx.pol
        with _ordered(pol, id(ctx.w_param)):
            if pol.ln_mode:
                return ops.layernorm_bwd(dy.contiguous(), x.contiguous(), w, mean, rstd, partials=_ln_partials(ctx.w_param, pol),
                                         partial_mode=pol.ln_mode)
            return ops.layernorm_bwd(dy.contiguous(), x.contiguous(), w, mean, rstd, accumulate_into=_grad_slot(ctx.w_param, pol))


class _LinearFn(torch.autograd.Function):
    """y = alpha * x W^T (bias-free nn.Linear; alpha = 1/width_mult for the muP readout)."""

    @staticmethod
    def forward(ctx, x, w, alpha):
        ctx.save_for_backward(x, w)
        ctx.alpha = alpha
        ctx.w_param = w
        ctx.pol = current_grad_policy()
        x2 = x.reshape(-1, x.shape[-1])
        y = ops.linear_fwd(x2.contiguous(), w, alpha=alpha)
        return y.view(*x.shape[:-1], w.shape[0])

    @staticmethod
    def backward(ctx, dy):
        x, w = ctx.saved_tensors
        dy2 = dy.reshape(-1, dy.shape[-1]).contiguous()
        x2 = x.reshape(-1, x.shape[-1]).contiguous()
        dx = dw = None
        with _ordered(ctx.pol, id(ctx.w_param)):
            a32, a32_mode = _acc32(ctx.w_param, ctx.pol)
            if ctx.needs_input_grad[0] and ctx.needs_input_grad[1]:
                dx, dw = ops.linear_bwd(dy2, x2, w, alpha=ctx.alpha, accumulate_into=_grad_slot(ctx.w_param, ctx.pol), acc32=a32, acc32_mode=a32_mode)
                return dx.view_as(x), dw, None
            if ctx.needs_input_grad[0]:
                dx = ops.linear_dgrad(dy2, w, alpha=ctx.alpha).view_as(x)
            if ctx.needs_input_grad[1]:
                slot = _grad_slot(ctx.w_param, ctx.pol)
                dw = ops.linear_wgrad(dy2, x2, alpha=ctx.alpha, accumulate_into=slot, acc32=a32, acc32_mode=a32_mode)
                if slot is not None:
                    dw = None
        return dx, dw, None


class _LinearGeluFn(torch.autograd.Function):
    """gelu_erf_1.41421(x W^T) (model.py:163-165) through the c_fc GEMM's fused epilogue — the same kernel, rounding and
    saved derivative as inside ``Block`` (one erf evaluation yields the activation and gelu'(h))."""

    @staticmethod
    def forward(ctx, x, w):
        x2 = x.reshape(-1, x.shape[-1]).contiguous()
        der, act = ops.linear_fwd(x2, w, epilogue=L.EPI_GELU)
        ctx.save_for_backward(x, w, der)
        ctx.w_param = w
        ctx.pol = current_grad_policy()
        return act.view(*x.shape[:-1], w.shape[0])

    @staticmethod
    def backward(ctx, dact):
        x, w, der = ctx.saved_tensors
        dh = dact.reshape(-1, dact.shape[-1]) * der            # bf16(dact * gelu'(h)), as OBTE_EPI_GELU_BWD forms it
        x2 = x.reshape(-1, x.shape[-1]).contiguous()
        with _ordered(ctx.pol, id(ctx.w_param)):
            a32, a32_mode = _acc32(ctx.w_param, ctx.pol)
            dx, dw = ops.linear_bwd(dh.contiguous(), x2, w, accumulate_into=_grad_slot(ctx.w_param, ctx.pol), acc32=a32, acc32_mode=a32_mode)
        return dx.view_as(x), dw


class _ReadoutRowsGradFn(torch.autograd.Function):
    """Backward-only node of the readout for a loss that looks at a subset of the positions (the masked-LM loss:
    train_encoder.py:301-305).  ``emb_rows`` [n, C] are the final embeddings of those positions, ``dlogits_rows`` [n, V]
    the rows of d(loss)/d(logits) that are not exact zeros (ops.masked_ce_rows on the DENSE logits).  forward() returns a
    zero scalar that stands for the loss in the graph; backward() contracts over the n rows only:
    d emb_rows = alpha dlogits_rows W, dW = alpha dlogits_rows^T emb_rows — exactly what the dense products give, the
    rows left out being all zero."""

    @staticmethod
    def forward(ctx, emb_rows, w, alpha, dlogits_rows):
        ctx.save_for_backward(emb_rows, w, dlogits_rows)
        ctx.alpha = alpha
        ctx.w_param = w
        ctx.pol = current_grad_policy()
        return torch.zeros((), dtype=torch.float32, device=emb_rows.device)

    @staticmethod
    def backward(ctx, dloss):
        emb_rows, w, dl = ctx.saved_tensors
        with _ordered(ctx.pol, id(ctx.w_param)):
            slot = _grad_slot(ctx.w_param, ctx.pol)
            a32, a32_mode = _acc32(ctx.w_param, ctx.pol)
            dx, dw = ops.linear_bwd(dl, emb_rows.contiguous(), w, alpha=ctx.alpha, accumulate_into=slot, acc32=a32, acc32_mode=a32_mode)
        return dx, dw, None, None


class _Acc32FlushFn(torch.autograd.Function):
    """Backward-only node for a weight whose own node does not run in a pass while its gradient is summed in fp32 (the readout
    weight in a pass with nothing masked): the zero contribution by the pass's mode — FIRST zeroes the buffer, MORE leaves it,
    LAST hands bf16(buffer), the total of the other passes, to autograd (and through it to DDP's reducer).  forward() returns a
    zero scalar to add to whatever the pass runs backward from."""

    @staticmethod
    def forward(ctx, w):
        ctx.w_param = w
        ctx.pol = current_grad_policy()
        return torch.zeros((), dtype=torch.float32, device=w.device)

    @staticmethod
    def backward(ctx, dloss):
        with _ordered(ctx.pol, id(ctx.w_param)):
            a32, a32_mode = _acc32(ctx.w_param, ctx.pol)
            return ops.acc32_add_(a32, None, a32_mode)


class _EmbeddingFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, idx, wte, dropout_p, dropout_seed, order):
        ctx.save_for_backward(idx)
        ctx.vocab = wte.shape[0]
        ctx.w_param = wte
        ctx.drop = (dropout_p, dropout_seed)
        ctx.order = order   # optional: a stable argsort of idx.reshape(-1) (int32) the caller already has
        ctx.pol = current_grad_policy()
        return ops.embedding_fwd(idx.contiguous(), wte, dropout_p, dropout_seed)

    @staticmethod
    def backward(ctx, dout):
        (idx,) = ctx.saved_tensors
        with _ordered(ctx.pol, id(ctx.w_param)):
            a32, a32_mode = _acc32(ctx.w_param, ctx.pol)
            dw = ops.embedding_bwd(idx.contiguous(), dout.contiguous(), ctx.vocab, accumulate_into=_grad_slot(ctx.w_param, ctx.pol),
                                   dropout_p=ctx.drop[0], dropout_seed=ctx.drop[1], order=ctx.order, acc32=a32, acc32_mode=a32_mode)
        return None, dw, None, None, None


class _GradHandOff:
    """The hand-off of the dropout-masked gradient between consecutive blocks' backward passes (ops.block_bwd, dy_masked): block
    i + 1's backward leaves dropout(dx) under block i's MLP-projection mask here, block i's backward takes it instead of spending
    a pass on masking dy.  ONE object per forward call (OmniBioTA.forward creates it and every _BlockFn node of that call holds
    it on its ctx), slots keyed by block index: nothing process-wide, two models or two passes never see each other's entries.
    The taker uses the entry only if the gradient it received IS the dx the entry was made for and nobody touched it since —
    same storage and shape, the same version counter (autograd's in-place accumulation of a second contribution, a tensor hook
    that edits the gradient: both bump it), its own probability and seed; otherwise it masks dy itself."""

    __slots__ = ("slots",)

    def __init__(self):
        self.slots = {}

    def put(self, index, dx, dx_masked, p, seed):
        if dx_masked is not None:
            self.slots[index] = (dx_masked, dx, dx._version, float(p), int(seed))

    def take(self, index, dy, drop):
        ent = self.slots.pop(index, None)
        if ent is None or os.environ.get("OBTE_DROPOUT_HANDOFF") == "0":   # (A/B and tests: every block masks its own dy)
            return None
        dx_masked, dx, version, p, seed = ent
        if (dy.data_ptr() != dx.data_ptr() or dy.shape != dx.shape or dy._version != version or p != float(drop[0])
                or seed != int(drop[1])):
            return None
        return dx_masked


class _BlockFn(torch.autograd.Function):
    """One pre-LN transformer block (model.py:170-181): a single C call per pass."""

    @staticmethod
    def forward(ctx, x, ln1, attn_w, proj_w, ln2, fc_w, mlp_w, rope_cos, rope_sin, n_head, mask, dropout_p, dropout_seed, out_rows=None,
                below_seed=None, handoff=None, index=0):
        x = x.contiguous()
        ctx.below_seed = below_seed if (dropout_p > 0 and handoff is not None) else None   # the dropout seed of the block below (None: no block there)
        ctx.handoff, ctx.index = handoff, index   # this forward call's _GradHandOff and the block's place in it
        params = (ln1, attn_w, proj_w, ln2, fc_w, mlp_w)
        y, act = ops.block_fwd(x, params, (rope_cos, rope_sin), n_head, mask, dropout_p, dropout_seed, out_rows=out_rows)
        ctx.save_for_backward(x, act, rope_cos, rope_sin, *params)
        ctx.n_head, ctx.mask = n_head, mask
        ctx.out_rows = out_rows   # the rows form: y is [n, C], the positions the caller wants (ops.block_fwd)
        ctx.drop = (dropout_p, dropout_seed)
        ctx.w_params = params
        ctx.pol = current_grad_policy()
        return y

    @staticmethod
    def backward(ctx, dy):
        x, act, rope_cos, rope_sin, *params = ctx.saved_tensors
        pol = ctx.pol
        with _ordered(pol, id(ctx.w_params[0])):   # one group per block: its six weights are updated by this one call
            slots = [_grad_slot(w, pol) for w in ctx.w_params]
            lnp = (_ln_partials(ctx.w_params[0], pol), _ln_partials(ctx.w_params[3], pol)) if pol.ln_mode else None
            dy = dy.contiguous()
            # dropout: the block above may have left dropout(dy) under this block's MLP-projection mask (one pass less per block)
            dy_masked = ctx.handoff.take(ctx.index, dy, ctx.drop) if (ctx.drop[0] > 0 and ctx.handoff is not None) else None
            res = ops.block_bwd(x, dy, act, tuple(params), (rope_cos, rope_sin), ctx.n_head, ctx.mask,
                                accumulate_into=slots, dropout_p=ctx.drop[0], dropout_seed=ctx.drop[1], ln_partials=lnp,
                                ln_partial_mode=pol.ln_mode, out_rows=ctx.out_rows, dy_masked=dy_masked, dx_mask_seed=ctx.below_seed,
                                acc32=tuple(_acc32(ctx.w_params[i], pol)[0] for i in (1, 2, 4, 5)) if pol.acc32_mode else None,
                                acc32_mode=pol.acc32_mode)
            dx, grads = res[0], res[1]
            if ctx.below_seed is not None:
                ctx.handoff.put(ctx.index - 1, dx, res[2], ctx.drop[0], ctx.below_seed)
        return (dx, *grads, None, None, None, None, None, None, None, None, None, None)


class _AttnCoreFn(torch.autograd.Function):
    """rope + fused attention on a packed qkv activation (used by the standalone SelfAttention module)."""

    @staticmethod
    def forward(ctx, qkv, rope_cos, rope_sin, n_head, scale, mask, dropout_p, dropout_seed):
        B, T, C3 = qkv.shape
        hs = C3 // 3 // n_head
        qkv = qkv.contiguous().clone()
        ops.rope_qk_(qkv, rope_cos, rope_sin, B, T, n_head, hs)
        o, lse = ops.attn_fwd(qkv, B, T, n_head, hs, scale, mask, dropout_p, dropout_seed)
        ctx.save_for_backward(qkv, o, lse, rope_cos, rope_sin)
        ctx.meta = (B, T, n_head, hs, scale, mask, dropout_p, dropout_seed)
        return o

    @staticmethod
    def backward(ctx, d_o):
        qkv, o, lse, rope_cos, rope_sin = ctx.saved_tensors
        B, T, H, hs, scale, mask, dp, dseed = ctx.meta
        dqkv = ops.attn_bwd(qkv, o, d_o.contiguous(), lse, B, T, H, hs, scale, mask, rope=(rope_cos, rope_sin),
                            dropout_p=dp, dropout_seed=dseed)
        return dqkv, None, None, None, None, None, None, None


class _DropoutFn(torch.autograd.Function):
    """Elementwise dropout with the library's counter-based mask (used by the standalone SelfAttention / MLP modules;
    inside Block the same masks are applied in the GEMM epilogues)."""

    @staticmethod
    def forward(ctx, x, p, seed, site):
        ctx.cfg = (p, seed, site)
        return ops.dropout(x.contiguous(), p, seed, site)

    @staticmethod
    def backward(ctx, dy):
        p, seed, site = ctx.cfg
        return ops.dropout(dy.contiguous(), p, seed, site), None, None, None


def _new_seed() -> int:
    """62-bit seed from torch's CPU generator: reproducible under torch.manual_seed, restored by checkpoint()'s RNG
    preservation, and no GPU synchronisation."""
    return int(torch.randint(0, 2 ** 62, (1,), dtype=torch.int64).item())


def _active_p(module: nn.Module, p: float) -> float:
    p = float(p)
    if not 0.0 <= p < 1.0:
        raise ValueError(f"dropout probability has to be in [0, 1), got {p}")
    return p if module.training else 0.0


def _no_gradient_possible(*tensors) -> bool:
    """No gradient can be asked of a call on these tensors: autograd is off, or none of them requires one.  Such a forward keeps
    nothing for a backward (ops.block_infer, EPI_GELU_ACT) unless OBTE_INFER=0 selects the training forward (same results)."""
    return not torch.is_grad_enabled() or not any(t.requires_grad for t in tensors)


# ------------------------------------------------------------------------------------------------------- modules
class LayerNorm(nn.Module):
    """LayerNorm with optional bias (model.py:63-72).  The reference always builds it with bias=False."""

    def __init__(self, ndim, bias):
        super().__init__()
        self.weight = nn.Parameter(torch.ones(ndim))
        self.bias = nn.Parameter(torch.zeros(ndim)) if bias else None

    def forward(self, input):
        if self.bias is not None:
            raise NotImplementedError("bias=True is not used by the reference (model.py:191) and not implemented")
        _require_hip(input, "LayerNorm")
        return _LayerNormFn.apply(input, self.weight)


class SelfAttention(nn.Module):
    def __init__(self, config):
        super().__init__()
        assert config.n_embd % config.n_head == 0
        self.c_attn = nn.Linear(config.n_embd, 3 * config.n_embd, bias=config.bias)
        self.c_proj = nn.Linear(config.n_embd, config.n_embd, bias=config.bias)
        self.attn_dropout = nn.Dropout(config.dropout, inplace=True)
        self.resid_dropout = nn.Dropout(config.dropout, inplace=True)
        self.n_head = config.n_head
        self.n_embd = config.n_embd
        self.dropout = config.dropout
        self.autoregressive = config.autoregressive
        self.flash = config.flash  # AttributeError if the caller never set it, as in the reference (model.py:89)
        self.register_buffer("freqs_cis", precompute_freqs_cis(self.n_embd // self.n_head, config.block_size))
        if not self.flash:
            # state_dict parity with the reference's non-flash modules (model.py:92-96); the buffer is unused here:
            # both settings run the same fused kernel, which is exact attention either way, and the causal mask of an
            # autoregressive model is a pair of range tables (masks.RangeMask.causal), not this T x T matrix.
            self.register_buffer("bias", torch.tril(torch.ones(config.block_size, config.block_size))
                                 .view(1, 1, config.block_size, config.block_size))
        self._rope_key = None
        self._rope_val = None

    def __getstate__(self):
        state = self.__dict__.copy()
        state["_rope_key"] = None
        state["_rope_val"] = None
        return state

    def rope(self) -> Tuple[torch.Tensor, torch.Tensor]:
        """fp32 cos/sin tables derived from the (possibly dtype-cast) ``freqs_cis`` buffer, cached."""
        f = self.freqs_cis
        key = (f.data_ptr(), f.dtype, f.device, f._version)
        if self._rope_key != key:
            self._rope_val = rope_tables(f)
            self._rope_key = key
        return self._rope_val

    def forward(self, x, attn_mask=None):
        _require_hip(x, "SelfAttention")
        B, T, C = x.size()
        attn_mask = _autoregressive_mask(self.autoregressive, attn_mask, B, T, x.device)
        mask = ops.MaskSpec.from_user(attn_mask, B, T, self.n_head, x.device)
        cos, sin = self.rope()
        p = _active_p(self, self.dropout)
        seed = _new_seed() if p > 0 else 0
        qkv = _LinearFn.apply(x, self.c_attn.weight, 1.0)
        y = _AttnCoreFn.apply(qkv, cos, sin, self.n_head, 8.0 / self.n_embd, mask, p, seed)
        y = _LinearFn.apply(y, self.c_proj.weight, 1.0)
        return _DropoutFn.apply(y, p, seed, L.SITE_RESID) if p > 0 else y


class MLP(nn.Module):
    def __init__(self, config):
        super().__init__()
        self.c_fc = nn.Linear(config.n_embd, 4 * config.n_embd, bias=config.bias)
        self.c_proj = nn.Linear(4 * config.n_embd, config.n_embd, bias=config.bias)
        self.dropout = nn.Dropout(config.dropout, inplace=True)

    def forward(self, x):
        _require_hip(x, "MLP")
        p = _active_p(self, self.dropout.p)
        if _no_gradient_possible(x, self.c_fc.weight) and ops.infer_enabled():   # the activation alone: no derivative for a backward that cannot come
            h = ops.linear_fwd(x.reshape(-1, x.shape[-1]).contiguous(), self.c_fc.weight, epilogue=L.EPI_GELU_ACT)
            h = h.view(*x.shape[:-1], self.c_fc.weight.shape[0])
        else:
            h = _LinearGeluFn.apply(x, self.c_fc.weight)
        y = _LinearFn.apply(h, self.c_proj.weight, 1.0)
        return _DropoutFn.apply(y, p, _new_seed(), L.SITE_MLP) if p > 0 else y


class Block(nn.Module):
    def __init__(self, config):
        super().__init__()
        self.ln_1 = LayerNorm(config.n_embd, bias=config.bias)
        self.attn = SelfAttention(config)
        self.ln_2 = LayerNorm(config.n_embd, bias=config.bias)
        self.mlp = MLP(config)
        if config.bias:
            raise NotImplementedError("bias=True is not used by the reference (model.py:191) and not implemented")

    def forward(self, x, attn_mask=None, out_rows=None, below_seed=None, seed=None, handoff=None, index=0, infer=None):
        """infer (internal, OmniBioTA.forward): a one-element list that holds the workspace of the forward call's blocks on the
        path that keeps nothing for a backward (allocated by the first block that takes it); with it, and autograd off, the block
        writes its output over x (the caller's x is the previous block's output or the fresh embedding).  A direct call leaves x alone.
        below_seed, seed, handoff, index (internal, OmniBioTA.forward): the dropout seed the block BELOW uses in this forward —
        this block's backward then also writes its dx under that block's MLP-projection mask (ops.block_bwd) and leaves it in
        `handoff` (the forward call's _GradHandOff) for block index - 1; `seed` is this block's own, drawn by the caller so that it
        can hand it on (None: drawn here).
        out_rows (optional, int64 (n,), ascending distinct rows of the flattened (b*t, n_embd) activation): the caller
        wants the block's output at those positions alone and gets it as (n, n_embd) — the attention half runs on every
        position, the MLP half on the listed ones (per-position arithmetic: the same values there; in training mode the
        dropout mask of the MLP projection is drawn for the (n, n_embd) output)."""
        _require_hip(x, "Block")
        _require_hip(self.attn.c_attn.weight, "Block parameters")
        B, T, C = x.shape
        if out_rows is not None:
            _check_rows(out_rows, B * T, 1)
        attn_mask = _autoregressive_mask(self.attn.autoregressive, attn_mask, B, T, x.device)
        mask = ops.MaskSpec.from_user(attn_mask, B, T, self.attn.n_head, x.device)
        cos, sin = self.attn.rope()
        # one dropout probability per block, as in the reference (config.dropout feeds all three nn.Dropout modules)
        p = _active_p(self, self.attn.dropout)
        if p > 0:
            seed = _new_seed() if seed is None else seed
        else:
            seed = 0
        params = (self.ln_1.weight, self.attn.c_attn.weight, self.attn.c_proj.weight, self.ln_2.weight, self.mlp.c_fc.weight, self.mlp.c_proj.weight)
        if out_rows is None and _no_gradient_possible(x, *params) and ops.infer_enabled():
            # nobody can differentiate this call: the forward that saves nothing (the rows form stays with obte_block_fwd)
            x = x.contiguous()
            ws = infer[0] if infer is not None else None
            if ws is None:
                ws = ops.block_infer_workspace(B, T, C, self.attn.n_head, x.device)
                if infer is not None:
                    infer[0] = ws
            over = infer is not None and not torch.is_grad_enabled()
            return ops.block_infer(x, params, (cos, sin), self.attn.n_head, mask, p, seed, ws=ws, out=x if over else None)
        return _BlockFn.apply(x, self.ln_1.weight, self.attn.c_attn.weight, self.attn.c_proj.weight, self.ln_2.weight,
                              self.mlp.c_fc.weight, self.mlp.c_proj.weight, cos, sin, self.attn.n_head, mask, p, seed, out_rows,
                              below_seed if p > 0 else None, handoff if p > 0 else None, index)


def _check_rows(rows, total: int, n_blocks: int) -> None:
    """The contract of ``OmniBioTA.forward(rows=)`` / ``Block.forward(out_rows=)``: a non-empty int64 vector on the GPU of
    ASCENDING, DISTINCT positions in [0, total).  Shape, dtype and device are checked on every call (no device read).  The
    values are the caller's responsibility — duplicates are unsupported (the scatter of the block backward would keep one of
    the contributions instead of their sum) and the gather clamps an out-of-range index instead of faulting — unless
    OBTE_CHECK_ROWS=1, which verifies bounds and strict monotonicity at the price of a device round trip per call."""
    if not torch.is_tensor(rows) or rows.dtype != torch.int64 or rows.dim() != 1 or not rows.is_cuda:
        raise ValueError("OmniBioTA.forward: rows must be a 1-D int64 tensor on the GPU")
    if rows.numel() == 0 or n_blocks == 0:
        raise ValueError("OmniBioTA.forward: rows must list at least one position (and the model needs a block)")
    if rows.numel() > total:
        raise ValueError(f"OmniBioTA.forward: {rows.numel()} rows listed, the batch has {total} positions")
    if os.environ.get("OBTE_CHECK_ROWS") == "1":
        r = rows.detach().cpu()
        if int(r[0]) < 0 or int(r[-1]) >= total or (r.numel() > 1 and not bool((r[1:] > r[:-1]).all())):
            raise ValueError(f"OmniBioTA.forward: rows must be strictly ascending positions in [0, {total})")


@dataclass
class OmniBioTAConfig:
    block_size: int = 2048
    vocab_size: int = 2 ** 16
    n_layer: int = 12
    n_head: int = 12
    n_embd: int = 1024
    dropout: float = 0.1
    bias: bool = False
    autoregressive: bool = False
    checkpoint_freq: int = 0


class MuReadout(_MuReadoutBase):
    """The readout layer (model.py:208).  With the real ``mup`` package this is its MuReadout with the matmul
    swapped for the HIP GEMM; without it, the restated class from mup_compat."""

    def forward(self, x):
        _require_hip(x, "MuReadout")
        wm = self.width_mult()
        return _LinearFn.apply(x, self.weight, float(self.output_mult) / float(wm))


class OmniBioTA(nn.Module):
    def __init__(self, config):
        super().__init__()
        assert config.vocab_size is not None
        assert config.block_size is not None
        self.config = config
        self.transformer = nn.ModuleDict(dict(
            wte=nn.Embedding(config.vocab_size, config.n_embd),
            drop=nn.Dropout(config.dropout, inplace=True),
            h=nn.ModuleList([Block(config) for _ in range(config.n_layer)]),
            ln_f=LayerNorm(config.n_embd, bias=config.bias),
        ))
        self.lm_head = MuReadout(config.n_embd, config.vocab_size, bias=False)
        print("number of parameters: %.2fM" % (self.get_num_params() / 1e6,))

    def get_num_params(self, non_embedding=True):
        """All parameters, minus the token embedding when non_embedding (model.py:213-223; lm_head is counted)."""
        n_params = sum(p.numel() for p in self.parameters())
        if non_embedding:
            n_params -= self.transformer.wte.weight.numel()
        return n_params

    def forward(self, idx, attn_mask=None, return_embeddings=False, rows=None):
        """idx (b, t) int64 -> logits (b, t, vocab) or, with return_embeddings, emb (b, t, n_embd)
        (model.py:225-254).  ``attn_mask``: None, the reference's additive (b, n_head, t, t) tensor (any strides,
        expand() views included), or a ``masks.RangeMask`` (per-query key ranges; the fast path).  With
        ``config.autoregressive`` and no mask the attention is causal; with a mask it is that mask alone (the reference's rule).
        ``rows`` (an extension, not in the reference; int64 (n,), ascending positions of the flattened (b*t) batch): the
        caller needs the result at those positions only — a masked-LM loss looks at ~15 % of them (train_encoder.py:304) —
        and gets (n, n_embd) embeddings or (n, vocab) logits.  Nothing after the last block's attention mixes positions, so
        that block's MLP half, ln_f and the readout run on the listed positions alone; every value returned is the one the full
        forward computes there (the same arithmetic per position; few-tile projections may sum their K range in split-K order)."""
        _, t = idx.size()
        assert t <= self.config.block_size, f"Cannot forward sequence of length {t}, block size is only {self.config.block_size}"
        wte = self.transformer.wte.weight
        _require_hip(wte, "OmniBioTA")
        if not idx.is_cuda:
            raise RuntimeError("OmniBioTA.forward: idx must be on the GPU")
        b = idx.shape[0]
        # autoregressive: the causal pair of tables, built once per call for all layers (nothing kept on a module)
        attn_mask = _autoregressive_mask(self.config.autoregressive, attn_mask, b, t, idx.device)
        mask = ops.MaskSpec.from_user(attn_mask, b, t, self.config.n_head, idx.device)
        p = _active_p(self, self.transformer.drop.p)
        # a training harness that sorts the token ids of a whole optimizer step in one call (the embedding backward sums
        # gradient rows in sorted-id order) hands this micro-batch's order through `with embedding_order(...)`; consumed once
        box = _embedding_order.get()
        order = None
        if box is not None:
            order, box[0] = box[0], None
        if order is not None and (order.numel() != idx.numel() or order.dtype != torch.int32 or order.device != idx.device):
            order = None
        x = _EmbeddingFn.apply(idx, wte, p, _new_seed() if p > 0 else 0, order)
        n_blocks = len(self.transformer.h)
        if rows is not None:
            _check_rows(rows, b * t, n_blocks)
        # dropout: the seed of the block just run is handed to the next one, whose backward masks its dx for the block below and
        # leaves it in this call's hand-off object (nothing of this lives on the modules or in the process)
        below = None
        handoff = _GradHandOff()
        infer = [None]   # the workspace of the blocks that run without a backward to come: one per call, filled by the first of them
        for i, block in enumerate(self.transformer.h):
            last_rows = rows if (rows is not None and i == n_blocks - 1) else None
            if self.config.checkpoint_freq > 0 and i % self.config.checkpoint_freq == 0:
                x = checkpoint(block, x, mask, last_rows, use_reentrant=False)
                below = None   # (a recomputed block redraws nothing, but keep the hand-off out of checkpointed segments)
            else:
                bp = _active_p(block, block.attn.dropout)
                seed = _new_seed() if bp > 0 else None
                x = block(x, attn_mask=mask, out_rows=last_rows, below_seed=below, seed=seed, handoff=handoff, index=i, infer=infer)
                below = seed
        emb = self.transformer.ln_f(x)
        if return_embeddings:
            return emb
        return self.lm_head(emb)

    def encode(self, idx, method="mean"):
        """Pooled sequence embedding (model.py:256-277)."""
        assert method in ["mean", "first", "last", "max", "all"], f"Unknown pooling method {method}"
        emb = self.forward(idx, return_embeddings=True)
        if method == "mean":
            return emb.mean(dim=1)
        elif method == "first":
            return emb[:, 0]
        elif method == "last":
            return emb[:, -1]
        elif method == "max":
            return emb.max(dim=1)[0]
        return emb

    # ---- scoring (beyond the reference): log-probabilities without a logits tensor -------------------------------------------------------
    @torch.no_grad()
    def token_logprobs(self, idx, rows, candidates, attn_mask=None):
        """log p(candidate) under the model at listed positions, fp32: ``rows`` int64 (n,), ascending flat positions of the (b*t) batch
        as in ``forward(rows=)``; ``candidates`` int64 or int32 (n, K) — K token ids per position, 1 <= K <= 64, or -1 for "none", which
        gives 0 — or (n,), which returns (n,).  Any model: for an encoder the caller places the MASK id in ``idx`` itself (a variant-effect
        score is then the difference of two entries of one row); for an autoregressive one position t scores token t + 1.
        ``forward(idx, attn_mask, return_embeddings=True, rows=rows)`` and then ``ops.readout_score`` with the readout's alpha: the last
        block's MLP half and ln_f run on the listed rows alone, and no (n, vocab) logits exist.  The values are those of
        ``log_softmax(model(idx, rows=rows).float())`` at the candidates, up to the fp32 summation order.  No gradient, and no dropout
        whatever ``self.training`` says."""
        if not torch.is_tensor(candidates) or candidates.dtype not in (torch.int64, torch.int32) or candidates.dim() not in (1, 2):
            raise ValueError("OmniBioTA.token_logprobs: candidates must be an int64 or int32 tensor of shape (n,) or (n, K)")
        if not torch.is_tensor(rows) or rows.dim() != 1 or candidates.shape[0] != rows.numel():
            raise ValueError("OmniBioTA.token_logprobs: rows must be 1-D with one entry per row of candidates")
        if candidates.dim() == 2 and not 1 <= candidates.shape[1] <= L.READOUT_SCORE_MAX_K:
            raise ValueError(f"OmniBioTA.token_logprobs: 1 <= K <= {L.READOUT_SCORE_MAX_K} candidates per position, got {candidates.shape[1]}")
        modes = [(m, m.training) for m in self.modules()]
        try:
            self.eval()
            emb = self.forward(idx, attn_mask, return_embeddings=True, rows=rows)
        finally:
            for m, was in modes:
                m.training = was
        alpha = float(self.lm_head.output_mult) / float(self.lm_head.width_mult())
        return ops.readout_score(emb, self.lm_head.weight, candidates, alpha=alpha)[0]

    # ---- attention maps: what a forward hook on the reference's attn_dropout sees with flash=False ------------------------------------------
    @torch.no_grad()
    def attention_maps(self, idx, attn_mask=None, layers=None, heads="all", dtype=torch.float32):
        """The softmax weights of the attention of chosen layers: (B, len(layers), n_head, T, T), or (B, len(layers), T, T) with
        ``heads="mean"`` (the heads' mean, summed in fp32), as ``dtype`` (torch.float32, or torch.bfloat16: the rounded fp32 value).
        ``layers``: ascending distinct block indices in [0, n_layer), None for all.  ``attn_mask`` as in ``forward`` (None, the
        reference's additive tensor, a ``masks.RangeMask``; an autoregressive model is causal without one).  The hidden states are
        those of ``model(idx, attn_mask)`` without a gradient: the blocks run as ``forward`` runs them, up to the last requested layer
        and no further.  For a requested layer the packed, rotated qkv is formed from the block's input by ``ops.layernorm_fwd`` and
        the c_attn product with its RoPE epilogue — before the block runs, which may write its output over its input — and
        ``ops.attn_probs`` writes that layer's slice of the result, allocated once.  The rule: attnmaps.attention_probs_reference.
        No gradient, and no dropout whatever ``self.training`` says.  Argument errors are ValueError, raised before anything is launched."""
        n_layer = len(self.transformer.h)
        if layers is None:
            layers = list(range(n_layer))
        else:
            try:
                layers = [operator.index(v) for v in layers]
            except TypeError:
                layers = []
            if not layers:
                raise ValueError("OmniBioTA.attention_maps: layers must be a non-empty sequence of ints, or None for every layer")
            if any(not 0 <= v < n_layer for v in layers):
                raise ValueError(f"OmniBioTA.attention_maps: layers must lie in [0, {n_layer}), got {layers}")
            if any(b <= a for a, b in zip(layers, layers[1:])):
                raise ValueError(f"OmniBioTA.attention_maps: layers must be ascending and distinct, got {layers}")
        if not layers:
            raise ValueError("OmniBioTA.attention_maps: the model has no block")
        if not isinstance(heads, str) or heads not in ("all", "mean"):
            raise ValueError(f"OmniBioTA.attention_maps: heads must be \"all\" or \"mean\", got {heads!r}")
        if dtype not in (torch.float32, torch.bfloat16):
            raise ValueError(f"OmniBioTA.attention_maps: dtype must be torch.float32 or torch.bfloat16, got {dtype}")
        if not torch.is_tensor(idx) or idx.dim() != 2 or idx.dtype != torch.int64:
            raise ValueError("OmniBioTA.attention_maps: idx must be a (b, t) int64 tensor")
        b, t = idx.shape
        if not 1 <= t <= self.config.block_size or b < 1:
            raise ValueError(f"OmniBioTA.attention_maps: idx is {tuple(idx.shape)}, the block size is {self.config.block_size}")
        wte = self.transformer.wte.weight
        _require_hip(wte, "OmniBioTA.attention_maps")
        if not idx.is_cuda:
            raise RuntimeError("OmniBioTA.attention_maps: idx must be on the GPU")
        H, C = self.config.n_head, self.config.n_embd
        hs = C // H
        modes = [(m, m.training) for m in self.modules()]
        try:
            self.eval()
            attn_mask = _autoregressive_mask(self.config.autoregressive, attn_mask, b, t, idx.device)
            mask = ops.MaskSpec.from_user(attn_mask, b, t, H, idx.device)
            x = _EmbeddingFn.apply(idx, wte, 0.0, 0, None)
            out = torch.empty((b, len(layers)) + ((t, t) if heads == "mean" else (H, t, t)), dtype=dtype, device=idx.device)
            ws = ops.attn_probs_workspace(b, t, H, idx.device)
            handoff = _GradHandOff()
            infer = [None]
            slot = {layer: j for j, layer in enumerate(layers)}
            for i, block in enumerate(self.transformer.h):
                if i in slot:
                    h1 = ops.layernorm_fwd(x.contiguous(), block.ln_1.weight)[0]
                    cos, sin = block.attn.rope()
                    qkv = ops.gemm(h1.view(b * t, C), block.attn.c_attn.weight, b * t, 3 * C, C, epilogue=L.EPI_ROPE_QK, rope=(cos, sin, t, hs))
                    ops.attn_probs(qkv, b, t, H, hs, 8.0 / C, mask, heads=heads, dtype=dtype, out=out[:, slot[i]], ws=ws)
                if i == layers[-1]:
                    break
                x = block(x, attn_mask=mask, handoff=handoff, index=i, infer=infer)
        finally:
            for m, was in modes:
                m.training = was
        return out

    @torch.no_grad()
    def score(self, idx, lengths=None):
        """The model's log-likelihood of the sequences ``idx`` (B, T) int64, T >= 2, autoregressive models only.  Returns a
        ``SequenceScore``: ``token_logprobs`` fp32 (B, T - 1) with entry [b, t] = log p(idx[b, t + 1] | idx[b, :t + 1]), ``total`` fp32
        (B,) its row sums, ``count`` int64 (B,) the number of scored tokens, so that ``-total.sum() / count.sum()`` is the mean
        next-token loss.  ``lengths`` (a host sequence of B ints, 2 <= len_b <= T; None: all T): rows of different lengths, right-padded;
        entries at t + 1 >= lengths[b] are 0 and count is lengths - 1.  Under the causal mask padding cannot reach a real position.
        Only the sum(lengths - 1) real positions go through the last block's MLP half, ln_f and the readout (``token_logprobs``), and no
        logits tensor exists.  ``score(model.generate(...))`` is the model's own log-likelihood of its samples at temperature 1 and
        without truncation (no top_k, top_p or allowed_tokens), whatever they were drawn with; a ragged ``generate`` returns the
        ``lengths`` to pass.  No gradient and no dropout."""
        if not torch.is_tensor(idx) or idx.dim() != 2:
            raise ValueError("OmniBioTA.score: idx must be a (B, T) tensor")
        b, t = idx.shape
        self._check_generation("score", b)
        if t < 2:
            raise ValueError(f"OmniBioTA.score: nothing to score in sequences of length {t}: T >= 2")
        lens = [t] * b if lengths is None else _check_lengths("score", lengths, b, t)
        if min(lens) < 2:
            raise ValueError(f"OmniBioTA.score: every length must lie in [2, T = {t}], got {lens}")
        dev = idx.device
        if min(lens) == t:                                                              # every (b, t): nothing to work out on the host
            at = torch.arange(b * (t - 1), device=dev)
            count = torch.full((b,), t - 1, dtype=torch.int64, device=dev)
        else:
            def up(h):   # from pinned memory, so that the copy does not make the host wait for the stream
                return h.pin_memory().to(dev, non_blocking=True) if dev.type == "cuda" else h.to(dev)
            count = torch.tensor(lens, dtype=torch.int64) - 1
            real = torch.arange(t - 1).view(1, -1) < count.view(-1, 1)                   # host: which (b, t) have a real token t + 1
            at = up(real.flatten().nonzero().flatten())                                 # into (B, T - 1), ascending
            count = up(count)
        rows = at // (t - 1) * t + at % (t - 1)                                          # the same positions in (B, T)
        lp = self.token_logprobs(idx, rows, idx[:, 1:].reshape(-1).index_select(0, at))
        out = torch.zeros(b * (t - 1), dtype=torch.float32, device=dev)
        out.index_copy_(0, at, lp)
        out = out.view(b, t - 1)
        return SequenceScore(out, out.sum(dim=1), count)

    # ---- infilling (beyond the reference): tokens drawn at listed positions without a logits tensor ------------------------------------
    def _check_draw(self, what, idx, temperature, seed, allowed_tokens):
        """The arguments ``sample_tokens`` and ``infill`` share, checked on the host before any device work: returns
        ``(seed, allowed)`` with a drawn seed for None and ``allowed`` None or a bool (V,) tensor on the CPU."""
        from .sampling import inv_temperature
        who = f"OmniBioTA.{what}"
        if not torch.is_tensor(idx) or idx.dim() != 2 or idx.dtype != torch.int64 or idx.numel() == 0:
            raise ValueError(f"{who}: idx must be a non-empty (B, T) int64 tensor")
        if idx.shape[1] > self.config.block_size:
            raise ValueError(f"{who}: sequences of length {idx.shape[1]}, the block size is {self.config.block_size}")
        try:
            inv_temperature(temperature)
        except (TypeError, ValueError) as e:
            raise ValueError(f"{who}: {e}") from None
        if seed is not None and (isinstance(seed, bool) or not isinstance(seed, int) or not 0 <= seed < 2 ** 64):
            raise ValueError(f"{who}: seed must be None or an integer in [0, 2^64), got {seed!r}")
        V = self.config.vocab_size
        allowed = None
        if allowed_tokens is not None:
            a = torch.as_tensor(allowed_tokens).detach().cpu()
            if a.numel() == 0:
                raise ValueError(f"{who}: allowed_tokens is empty: there is nothing to draw")
            if a.dtype == torch.bool:
                if a.shape != (V,):
                    raise ValueError(f"{who}: a bool allowed_tokens must be ({V},), one set for all rows, got {tuple(a.shape)}")
                allowed = a.clone()
            else:
                if a.dim() != 1 or a.dtype not in (torch.int64, torch.int32) or (a.numel() and (int(a.min()) < 0 or int(a.max()) >= V)):
                    raise ValueError(f"{who}: allowed_tokens must be a bool ({V},) mask or a 1-D list of token ids in [0, {V})")
                allowed = torch.zeros(V, dtype=torch.bool)
                allowed[a.long()] = True
            if not bool(allowed.any()):
                raise ValueError(f"{who}: allowed_tokens is empty: there is nothing to draw")
        return (_new_seed() if seed is None else seed), allowed

    def _draw_rows(self, idx, rows, temperature, seed, allowed_packed, attn_mask):
        """(tokens, logprob, lse) at ``rows``: the forward on those rows alone, then the fused readout + draw with keys = rows"""
        emb = self.forward(idx, attn_mask, return_embeddings=True, rows=rows)
        alpha = float(self.lm_head.output_mult) / float(self.lm_head.width_mult())
        return ops.readout_sample(emb, self.lm_head.weight, temperature, seed, keys=rows, allowed_packed=allowed_packed, alpha=alpha)

    @torch.no_grad()
    def sample_tokens(self, idx, rows, temperature=1.0, seed=None, allowed_tokens=None, attn_mask=None):
        """One token drawn from the model's distribution at each listed position: ``rows`` int64 (n,), ascending flat positions of the
        (b*t) batch as in ``forward(rows=)``.  Returns ``(tokens (n,) int64, logprobs (n,) fp32)``: the log-probability each token was
        drawn with, at ``temperature`` and over ``allowed_tokens`` (None, token ids, or a bool (V,) mask: one non-empty set for all rows;
        the distribution is renormalised over it).  ``temperature`` 0: the most likely allowed token, its log-probability at temperature 1.
        Any model; ``token_logprobs``' conventions: for an encoder the caller places the MASK id in ``idx`` itself, no gradient, no dropout
        whatever ``self.training`` says.  ``forward(idx, attn_mask, return_embeddings=True, rows=rows)`` and then ``ops.readout_sample`` with
        the readout's alpha and keys = rows: no (n, vocab) logits exist, and a position's draw depends on the seed, its flat position and
        its logits alone.  ``seed`` None draws one from torch's generator."""
        seed, allowed = self._check_draw("sample_tokens", idx, temperature, seed, allowed_tokens)
        if not torch.is_tensor(rows) or rows.dim() != 1 or rows.dtype != torch.int64 or rows.numel() == 0 or rows.numel() > idx.numel():
            raise ValueError("OmniBioTA.sample_tokens: rows must be a non-empty 1-D int64 tensor of positions of the batch")
        packed = None if allowed is None else ops.pack_token_mask(allowed.to(idx.device))
        modes = [(m, m.training) for m in self.modules()]
        try:
            self.eval()
            tokens, logprob, _ = self._draw_rows(idx, rows, temperature, seed, packed, attn_mask)
        finally:
            for m, was in modes:
                m.training = was
        return tokens, logprob

    @torch.no_grad()
    def infill(self, idx, masked, steps=1, temperature=1.0, order="confidence", seed=None, allowed_tokens=None, mask_token=2, attn_mask=None):
        """Fill the positions ``masked`` (bool (B, T)) of ``idx`` (B, T) int64 with tokens drawn from the model, unmasking over ``steps``
        iterations (mask-predict).  Returns ``(out (B, T) int64, logprobs (B, T) fp32)``: ``idx`` with every masked position filled, and
        the log-probability — at ``temperature``, over ``allowed_tokens`` — each token was drawn with in the context of its iteration; 0 at
        positions that were not masked.  ``idx`` is copied and ``mask_token`` written at the masked positions.  Iteration s runs the
        forward on the still-masked rows, draws a token at each (``ops.readout_sample``, keys = the flat positions, the seed of
        ``sampling.fill_iteration_seed(seed, s)``) and commits ``sampling.fill_schedule(m_b, steps)[s]`` of sequence b's — by ``order``:
        "confidence" (largest log-probability first), "random", or "left" (lowest position first); the rest stay masked and are drawn
        again.  ``steps`` 1 draws all positions independently at once; ``steps`` >= the largest masked count unmasks one position per
        sequence and iteration.  ``masked`` is read on the host once, up front (the schedule and every iteration's offsets); the loop
        itself reads nothing back.  At most 8192 masked positions per sequence.  ``allowed_tokens``, ``seed``, ``attn_mask``, modes and
        gradients as ``sample_tokens``."""
        from .sampling import fill_iteration_seed, fill_schedule
        seed, allowed = self._check_draw("infill", idx, temperature, seed, allowed_tokens)
        who = "OmniBioTA.infill"
        if not torch.is_tensor(masked) or masked.dtype != torch.bool or masked.shape != idx.shape:
            raise ValueError(f"{who}: masked must be a bool tensor of idx's shape {tuple(idx.shape)}")
        if isinstance(steps, bool) or not isinstance(steps, int) or steps < 1:
            raise ValueError(f"{who}: steps must be an integer >= 1, got {steps!r}")
        if order not in ops.FILL_ORDERS:
            raise ValueError(f"{who}: order must be one of {tuple(ops.FILL_ORDERS)}, got {order!r}")
        if isinstance(mask_token, bool) or not isinstance(mask_token, int) or not 0 <= mask_token < self.config.vocab_size:
            raise ValueError(f"{who}: mask_token must be a token id in [0, {self.config.vocab_size}), got {mask_token!r}")
        B, T = idx.shape
        held = masked.detach().cpu()                                                      # the one host read
        counts = held.sum(dim=1).tolist()
        if sum(counts) == 0:
            raise ValueError(f"{who}: nothing is masked")
        if max(counts) > L.FILL_MAX_SEG:
            raise ValueError(f"{who}: at most {L.FILL_MAX_SEG} masked positions per sequence, got {max(counts)}")
        # every iteration's takes and offsets, from the counts alone
        per_seq = [fill_schedule(m, steps) for m in counts]
        takes, offs, rem = [], [], list(counts)
        for s in range(steps):
            if sum(rem) == 0:
                break
            offs.append([sum(rem[:b]) for b in range(B + 1)])
            takes.append([per_seq[b][s] for b in range(B)])
            rem = [rem[b] - takes[-1][b] for b in range(B)]
        offs.append([0] * (B + 1))
        dev = idx.device
        _require_hip(self.transformer.wte.weight, "OmniBioTA")
        if not idx.is_cuda:
            raise RuntimeError("OmniBioTA.infill: idx must be on the GPU")

        def up(h):
            return h.pin_memory().to(dev, non_blocking=True)
        take_d, off_d = up(torch.tensor(takes, dtype=torch.int32)), up(torch.tensor(offs, dtype=torch.int32))
        rows = up(held.flatten().nonzero().flatten())
        out = idx.clone().masked_fill_(up(held), mask_token)
        logprobs = torch.zeros(B, T, dtype=torch.float32, device=dev)
        packed = None if allowed is None else ops.pack_token_mask(up(allowed))
        modes = [(m, m.training) for m in self.modules()]
        try:
            self.eval()
            for s in range(len(takes)):
                tokens, logprob, _ = self._draw_rows(out, rows, temperature, fill_iteration_seed(seed, s), packed, attn_mask)
                rows_next = torch.empty(offs[s + 1][B], dtype=torch.int64, device=dev)
                ops.fill_commit(rows, off_d[s], tokens, logprob, take_d[s], order, seed, out, logprobs, rows_next, off_d[s + 1], max(counts))
                rows = rows_next
        finally:
            for m, was in modes:
                m.training = was
        return out, logprobs

    # ---- generation (beyond the reference, whose model.py strikes nanoGPT's generate() out) -----------------------------------------
    # Dropout is never applied on these paths, whatever ``training`` says: a sample is drawn from the model, not from a thinned one.
    def _block_params(self, block):
        return (block.ln_1.weight, block.attn.c_attn.weight, block.attn.c_proj.weight, block.ln_2.weight, block.mlp.c_fc.weight,
                block.mlp.c_proj.weight)

    def _check_generation(self, what, batch, cache=None):
        if not self.config.autoregressive:
            raise ValueError(f"OmniBioTA.{what}: the model is not autoregressive (config.autoregressive): an encoder has no next token")
        if cache is not None and cache.batch != batch:
            raise ValueError(f"OmniBioTA.{what}: the cache was built for batch size {cache.batch}, got {batch}")

    @staticmethod
    def _refuse_fp8(what, cache):
        """NotImplementedError in ``OmniBioTA.what``'s name on an fp8 cache: before anything is launched or any state changes"""
        if cache.dtype == "fp8":
            raise NotImplementedError(f"OmniBioTA.{what}: the cache is an fp8 cache (KVCache(dtype='fp8')), over which only one new position per "
                                      "row attends (prefill, decode_step, generate); several new positions in one call need a bf16 cache")

    @staticmethod
    def _refuse_shared(what, cache):
        """NotImplementedError in ``OmniBioTA.what``'s name on a shared-prefix cache: before anything is launched or any state changes"""
        if isinstance(cache, SharedPrefixCache):
            raise NotImplementedError(f"OmniBioTA.{what}: the cache is a shared-prefix cache (SharedPrefixCache), on which every row takes one new "
                                      "position at a time (prefill, decode_step, generate(num_samples=)); several new positions per row in one "
                                      "call need a KVCache")

    def quantize_weights(self, format="e4m3"):
        """This model's four matrices per block and its readout as e4m3 codes with a power-of-two scale per output row, together with
        their dequantised bf16 form: a ``QuantizedWeights`` for ``weights=`` of ``prefill``, ``decode_step``, ``generate`` and
        ``DecodeLoop``.  Runs in plain torch on the parameters' device, once; a snapshot — after an optimizer step, a ``load_state_dict``
        or a ``.to(...)`` call it again.  It holds 3 bytes per parameter beside the model's 2 (the bf16 copies serve the prompt and
        batches above the weight-streaming product's row limit; dropping them is not built).  ``format="mxfp4"``: OCP MXFP4 instead, e2m1
        codes with a power-of-two scale per 32 elements of a row (w4quant.py): a quarter of the bf16 bytes and a sixteenth, about 2.53
        bytes per parameter held."""
        return QuantizedWeights(self, format)

    def _readout_rows(self, x, out=None, weights=None):
        """The readout of a generation step's (B, C) rows: at most ops' small_m_max of them, bf16 on the GPU, through the
        weight-streaming product with MuReadout.forward's alpha; anything else through the module.  ``out``: a (B, vocab) buffer of the
        caller's that takes the logits (a ``DecodeLoop``'s, whose address must not change).  ``weights``: the readout's codes (e4m3 or
        MXFP4, by ``weights.format``) on that product, the tile product on the dequantised readout above its row limit."""
        if weights is not None:
            _require_hip(x, "OmniBioTA")
            alpha = float(self.lm_head.output_mult) / float(self.lm_head.width_mult())
            if x.shape[0] <= L.lib().obte_small_m_max():
                product = ops.linear_small_m_w4 if weights.format == "mxfp4" else ops.linear_small_m_w8
                return product(x, weights.head_codes, weights.head_scales, alpha=alpha, out=out)
            y = ops.linear_fwd(x, weights.head_dequantized, alpha=alpha)
            return y if out is None else out.copy_(y)
        w = self.lm_head.weight
        if x.is_cuda and x.dtype == torch.bfloat16 and w.dtype == torch.bfloat16 and x.shape[0] <= L.lib().obte_small_m_max():
            return ops.linear_small_m(x, w, alpha=float(self.lm_head.output_mult) / float(self.lm_head.width_mult()), out=out)
        return self.lm_head(x) if out is None else out.copy_(self.lm_head(x))

    @torch.no_grad()
    def prefill(self, idx, cache, lengths=None, chunk=None, weights=None, rows=None, shared_pages=None):
        """The prompt ``idx`` (B, T0) through every block under the causal mask, its keys and values left in ``cache`` (started
        over: ``cache.pos = T0``); returns the logits of the last position, (B, vocab).  ln_f and the readout run on that row alone.

        ``lengths`` (a host sequence of B ints, 1 <= len_b <= T0): the prompts are right-padded, columns >= len_b of row b hold any
        valid id.  The same kernels run over T0 — under the causal mask a real position never sees a later one, so the padding reaches
        nothing, and the cache positions it fills are overwritten by the row's own new tokens before they are read.  Row b's logits
        come from position len_b - 1; ``cache.positions`` = lengths and ``cache.pos`` = max(lengths) put ``decode_step`` on the
        one-position-per-row path.

        ``chunk`` (an int >= 1; None or >= T0: the call above, bit for bit): the first ``chunk`` columns go through the prefill kernels,
        every further ``chunk`` of them through ``extend``'s block path at uniform positions (right padding stays harmless under the
        causal rule), each embedded on its own — the activation workspace is sized by the chunk, no (B, T0, C) tensor exists — and
        row b's last hidden state is picked up in the chunk that holds it.  The cache ends in the same state.

        ``weights`` (``quantize_weights()``): the prompt runs through the same kernels on the DEQUANTISED weights, so that it and a
        continuation by ``decode_step(weights=)`` see one model; the readout of the last position reads the e4m3 codes.

        On a ``PagedKVCache``: ``rows`` is a host list of the cache rows the prompts go to, ``idx`` (len(rows), T0); the default is every
        row.  Only those rows are started over — each gets pages for its ``len_b`` positions unless it holds them — and the others keep
        their state.  The same causal kernels run over the right-padded prompts (``ops.block_prefill_paged``, on an fp8 pool
        ``ops.block_prefill_paged8``, with the gathered table rows: the padding beyond a row's own pages is not stored).  ``chunk=`` and ``weights=`` raise NotImplementedError there: several new
        positions per row over pages and e4m3 weights on pages are not built.

        ``shared_pages`` (a bf16 ``PagedKVCache`` only): a host list with one list of page ids per prompt.  The caller vouches that the
        m_i pages of ``shared_pages[i]`` hold positions [0, 64 m_i) of row i's prompt — another row computed them from the same tokens —
        and 64 m_i < len_i.  Row i then NAMES those pages (``PageBook.assign_shared``) instead of computing and storing them again, gets
        pages of its own for the rest, and only its remaining len_i - 64 m_i tokens run, right-padded to the longest tail, through
        ``ops.block_extend_paged`` at positions 64 m_i on; its logits come from its last tail row.  Rows with an empty list go through the
        path above — with every list empty, the same kernels and the same bits.  Where the rows' starts and tails do not fit one call
        (max start + longest tail > ``cache.max_len``: a long start with a short tail beside a short start with a long tail) the host
        makes several, sorted by start.  Shared pages are read-only by construction: a sharer's first store is at position 64 m_i, in a
        page of its own, and the owner's later stores are at positions >= its prompt length >= 64 m_i; nothing copies on write.
        NotImplementedError on an fp8 pool, on any other cache or with ``weights=``; ValueError for a page id outside the pool,
        64 m_i >= len_i or a row that still holds pages — all before any state changes."""
        if isinstance(cache, PagedPositions):
            return self._prefill_paged(idx, cache, lengths, chunk, weights, rows, shared_pages)
        if shared_pages is not None:
            raise NotImplementedError("OmniBioTA.prefill: shared_pages= names pages of a PagedKVCache; no other cache shares positions between rows")
        if rows is not None:
            raise ValueError("OmniBioTA.prefill: rows= names the rows of a PagedKVCache; every other cache is prefilled as a whole")
        if isinstance(cache, SharedPrefixCache):
            _refuse_weights("prefill", weights, "do not run on a shared-prefix cache (SharedPrefixCache)")
            return self._prefill_shared(idx, cache, lengths, chunk)
        if weights is not None:
            _checked_weights(self, "OmniBioTA.prefill", weights)
        if chunk is not None:
            self._refuse_fp8("prefill(chunk=)", cache)
        if idx.dim() != 2:
            raise ValueError(f"OmniBioTA.prefill: idx must be (B, T0), got {tuple(idx.shape)}")
        if chunk is not None and int(chunk) < 1:
            raise ValueError(f"OmniBioTA.prefill: chunk must be at least 1, got {chunk}")
        b, t = idx.shape
        self._check_generation("prefill", b, cache)
        if t == 0:
            raise ValueError("OmniBioTA.prefill: the prompt is empty")
        if t > cache.max_len:
            raise ValueError(f"OmniBioTA.prefill: a prompt of {t} tokens does not fit the cache's {cache.max_len} positions")
        lens = None if lengths is None else _check_lengths("prefill", lengths, b, t)
        wte = self.transformer.wte.weight
        _require_hip(wte, "OmniBioTA")
        if not idx.is_cuda:
            raise RuntimeError("OmniBioTA.prefill: idx must be on the GPU")
        if chunk is not None and int(chunk) < t:
            return self._prefill_chunked(idx, cache, lens, int(chunk), weights)
        params = self._params_for(weights)
        mask = ops.MaskSpec.from_user(_autoregressive_mask(True, None, b, t, idx.device), b, t, self.config.n_head, idx.device)
        x = ops.embedding_fwd(idx.contiguous(), wte)
        ws = ops.block_infer_workspace(b, t, self.config.n_embd, self.config.n_head, idx.device)
        block_prefill = ops.block_prefill_kv8 if cache.dtype == "fp8" else ops.block_prefill
        for i, (block, kv) in enumerate(zip(self.transformer.h, cache.layers)):
            block_prefill(x, params(i, block), block.attn.rope(), self.config.n_head, mask, kv, cache.max_len, ws=ws, out=x)
        self._prefilled(cache, t, lens, idx.device)
        if lens is None:
            return self._readout_rows(self.transformer.ln_f(x[:, -1].contiguous()), weights=weights)
        last = x[torch.arange(b, device=idx.device), (cache.positions - 1).long()]          # (B, C): row b at its own last position
        return self._readout_rows(self.transformer.ln_f(last.contiguous()), weights=weights)

    def _prefill_paged(self, idx, cache, lengths, chunk, weights, rows, shared_pages=None):
        """``prefill`` on a ``PagedKVCache``: the prompts ``idx`` (len(rows), T0) into the cache rows ``rows``; (len(rows), vocab)"""
        if chunk is not None:
            _refuse_paged("prefill(chunk=)", cache)
        _refuse_weights("prefill", weights, "do not run on a paged cache (PagedKVCache)")
        if shared_pages is not None and cache.dtype == "fp8":
            raise NotImplementedError("OmniBioTA.prefill: shared_pages= on an fp8 pool: several new positions per row over pages need a bf16 PagedKVCache")
        if idx.dim() != 2:
            raise ValueError(f"OmniBioTA.prefill: idx must be (B, T0), got {tuple(idx.shape)}")
        b, t = idx.shape
        self._check_generation("prefill", b)
        whole = rows is None
        rows = list(range(cache.batch)) if whole else [int(r) for r in rows]
        if len(rows) != b or len(set(rows)) != b or (rows and not 0 <= min(rows) <= max(rows) < cache.batch):
            raise ValueError(f"OmniBioTA.prefill: rows must be {b} distinct rows of the cache's {cache.batch} (one per prompt), got {rows}")
        if t == 0:
            raise ValueError("OmniBioTA.prefill: the prompt is empty")
        if t > cache.max_len:
            raise ValueError(f"OmniBioTA.prefill: a prompt of {t} tokens does not fit the cache's {cache.max_len} positions")
        lens = [t] * b if lengths is None else _check_lengths("prefill", lengths, b, t)
        if shared_pages is not None:
            shared_pages = cache.check_shared(rows, lens, shared_pages)  # (ValueError with nothing changed)
            if not any(shared_pages):
                shared_pages = None                                     # nothing is shared: the call below, bit for bit
        wte = self.transformer.wte.weight
        _require_hip(wte, "OmniBioTA")
        if not idx.is_cuda:
            raise RuntimeError("OmniBioTA.prefill: idx must be on the GPU")
        cache.start_rows(rows, lens, shared_pages)                      # (ValueError with nothing changed when the free list cannot, or for bad pages)
        if shared_pages is not None:
            return self._prefill_paged_tails(idx, cache, lens, rows, shared_pages)
        table = cache.table if whole else cache.table[torch.tensor(rows, device=idx.device)]
        last = self._prefill_paged_rows(idx, cache, lens, table)
        return self._readout_rows(self.transformer.ln_f(last.contiguous()))

    def _prefill_paged_rows(self, idx, cache, lens, table):
        """the prompts ``idx`` (b, t) under the causal mask into the pages of ``table`` (b, table_ld): (b, C), row i at its own last position"""
        b, t = idx.shape
        mask = ops.MaskSpec.from_user(_autoregressive_mask(True, None, b, t, idx.device), b, t, self.config.n_head, idx.device)
        x = ops.embedding_fwd(idx.contiguous(), self.transformer.wte.weight)
        ws = ops.block_infer_workspace(b, t, self.config.n_embd, self.config.n_head, idx.device)
        block_prefill = ops.block_prefill_paged8 if cache.dtype == "fp8" else ops.block_prefill_paged
        for block, pool in zip(self.transformer.h, cache.layers):
            block_prefill(x, self._block_params(block), block.attn.rope(), self.config.n_head, mask, pool, cache.n_pages, table, ws=ws, out=x)
        return x[torch.arange(b, device=idx.device), torch.tensor(lens, device=idx.device) - 1]

    @staticmethod
    def _tail_calls(starts, tails, max_len):
        """The rows (indices into ``starts``) of each ``block_extend_paged`` call: sorted by start, a call takes rows while its largest
        start and its longest tail together stay within ``max_len`` (the RoPE tables' and the kernels' bound: pos + n).  A row alone
        always fits: start + tail is its prompt length."""
        calls = []
        for i in sorted(range(len(starts)), key=lambda i: (starts[i], i)):
            if calls and starts[i] + max(tails[i], max(tails[j] for j in calls[-1])) <= max_len:   # (sorted: starts[i] is the call's largest)
                calls[-1].append(i)
            else:
                calls.append([i])
        return calls

    def _prefill_paged_tails(self, idx, cache, lens, rows, shared_pages):
        """``prefill(shared_pages=)`` behind ``start_rows``: the rows without shared pages through the prefill kernels, the others'
        tails through ``ops.block_extend_paged``; (len(rows), vocab)"""
        from .paged import KV_PAGE
        dev, H = idx.device, self.config.n_head
        last = torch.empty((len(rows), self.config.n_embd), dtype=torch.bfloat16, device=dev)
        plain = [i for i, p in enumerate(shared_pages) if not p]
        if plain:
            at = torch.tensor(plain, device=dev)
            t = max(lens[i] for i in plain)
            last[at] = self._prefill_paged_rows(idx[at, :t], cache, [lens[i] for i in plain], cache.table[torch.tensor([rows[i] for i in plain], device=dev)])
        tailed = [i for i, p in enumerate(shared_pages) if p]
        starts = [KV_PAGE * len(shared_pages[i]) for i in tailed]
        tails = [lens[i] - s for i, s in zip(tailed, starts)]
        for call in self._tail_calls(starts, tails, cache.max_len):
            n, g = max(tails[k] for k in call), len(call)
            tokens = torch.zeros((g, n), dtype=torch.int64, device=dev)          # right padding: any valid id; no real position sees it
            for j, k in enumerate(call):
                tokens[j, :tails[k]] = idx[tailed[k], starts[k]:starts[k] + tails[k]]
            table = cache.table[torch.tensor([rows[tailed[k]] for k in call], device=dev)]
            pos_rows = torch.tensor([starts[k] for k in call], dtype=torch.int32, device=dev)
            bound = max(starts[k] for k in call)
            ws = ops.block_extend_workspace(g, n, self.config.n_embd, H, dev)
            x = ops.embedding_fwd(tokens, self.transformer.wte.weight)
            for block, pool in zip(self.transformer.h, cache.layers):
                ops.block_extend_paged(x, self._block_params(block), block.attn.rope(), H, pool, cache.n_pages, table, bound, pos_rows, ws=ws, out=x)
            last[torch.tensor([tailed[k] for k in call], device=dev)] = x[torch.arange(g, device=dev), torch.tensor([tails[k] - 1 for k in call], device=dev)]
        return self._readout_rows(self.transformer.ln_f(last))

    def _params_for(self, weights):
        """(index, block) -> the block's six parameters: the model's own, or with the four matrices dequantised from ``weights``"""
        return (lambda i, block: self._block_params(block)) if weights is None else (lambda i, block: weights.block_params(i))

    def _prefill_shared(self, idx, cache, lengths, chunk):
        """``prefill`` on a ``SharedPrefixCache``: ``idx`` (P, T0), one row per prompt, through the same kernels into the prefix buffers;
        the logits of the last position come back once per sample, (P * G, vocab), row p repeated G times"""
        if lengths is not None or chunk is not None:
            raise ValueError("OmniBioTA.prefill: a shared-prefix cache takes prompts of one length in one piece (no lengths=, no chunk=)")
        if idx.dim() != 2:
            raise ValueError(f"OmniBioTA.prefill: idx must be (P, T0), got {tuple(idx.shape)}")
        p, t = idx.shape
        self._check_generation("prefill", p)
        if p != cache.prompts:
            raise ValueError(f"OmniBioTA.prefill: the shared-prefix cache was built for {cache.prompts} prompts, got {p}")
        if t == 0:
            raise ValueError("OmniBioTA.prefill: the prompt is empty")
        if t > cache.prefix_len:
            raise ValueError(f"OmniBioTA.prefill: a prompt of {t} tokens does not fit the cache's prefix of {cache.prefix_len} positions")
        wte = self.transformer.wte.weight
        _require_hip(wte, "OmniBioTA")
        if not idx.is_cuda:
            raise RuntimeError("OmniBioTA.prefill: idx must be on the GPU")
        mask = ops.MaskSpec.from_user(_autoregressive_mask(True, None, p, t, idx.device), p, t, self.config.n_head, idx.device)
        x = ops.embedding_fwd(idx.contiguous(), wte)
        ws = ops.block_infer_workspace(p, t, self.config.n_embd, self.config.n_head, idx.device)
        for block, (prefix, _) in zip(self.transformer.h, cache.layers):
            ops.block_prefill(x, self._block_params(block), block.attn.rope(), self.config.n_head, mask, prefix, cache.prefix_len, ws=ws, out=x)
        cache.reset(t)
        cache.n_prefix = t
        logits = self._readout_rows(self.transformer.ln_f(x[:, -1].contiguous()))
        return logits.repeat_interleave(cache.group, dim=0)

    @staticmethod
    def _prefilled(cache, t, lens, device):
        """the cache's state behind a prompt of ``t`` columns: uniform, or row b at ``lens[b]`` (the tensor the kernels read is made here)"""
        if lens is None:
            cache.reset(t)
        else:
            cache.reset(max(lens), torch.tensor(lens, dtype=torch.int32, device=device), min(lens))

    def _extend_ws(self, cache, device, *ns):
        """The workspace of ``n`` new positions per row for every ``n`` of ``ns``, kept on the cache object and replaced when a call
        needs more BYTES than it has.  The size is not monotone in n — the attention partials shrink where the default split count drops
        (n = 65 asks for less than n = 64 at small B * H) — so the buffer's own size is compared, never the n that made it."""
        need = max(ops.block_extend_ws_bytes(cache.batch, n, self.config.n_embd, self.config.n_head) for n in ns)
        if cache.extend_ws is None or cache.extend_ws.numel() < need:
            cache.extend_ws = None   # (the old buffer goes before the new one comes)
            cache.extend_ws = torch.empty(need, dtype=torch.uint8, device=device)
        return cache.extend_ws

    def _extend_hidden(self, tokens, cache, pos, pos_rows, weights=None):
        """``tokens`` (B, n) through every block against the cache at positions ``pos`` (or ``pos_rows``) on: the hidden states (B, n, C).
        ``weights``: on their dequantised matrices (a chunked prefill's later chunks)"""
        ws = self._extend_ws(cache, tokens.device, tokens.shape[1])
        x = ops.embedding_fwd(tokens.contiguous(), self.transformer.wte.weight)
        params = self._params_for(weights)
        for i, (block, kv) in enumerate(zip(self.transformer.h, cache.layers)):
            ops.block_extend(x, params(i, block), block.attn.rope(), self.config.n_head, kv, cache.max_len, pos, pos_rows=pos_rows, ws=ws, out=x)
        return x

    def _prefill_chunked(self, idx, cache, lens, chunk, weights=None):
        b, t = idx.shape
        params = self._params_for(weights)
        dev = idx.device
        # one buffer for every chunk size to come (the last chunk may be shorter and still ask for more bytes); it is at least the
        # prefill kernels' workspace for the first chunk's rows, so it serves them too
        ws = self._extend_ws(cache, dev, *{min(chunk, t - start) for start in range(0, t, chunk)})
        last_at = [t - 1] * b if lens is None else [n - 1 for n in lens]
        last = torch.empty((b, self.config.n_embd), dtype=torch.bfloat16, device=dev)
        for start in range(0, t, chunk):
            n = min(chunk, t - start)
            part = idx[:, start:start + n]
            if start == 0:
                mask = ops.MaskSpec.from_user(_autoregressive_mask(True, None, b, n, dev), b, n, self.config.n_head, dev)
                x = ops.embedding_fwd(part.contiguous(), self.transformer.wte.weight)
                for i, (block, kv) in enumerate(zip(self.transformer.h, cache.layers)):
                    ops.block_prefill(x, params(i, block), block.attn.rope(), self.config.n_head, mask, kv, cache.max_len, ws=ws, out=x)
            else:
                x = self._extend_hidden(part, cache, start, None, weights)
            rows = [r for r in range(b) if start <= last_at[r] < start + n]
            if rows:
                rt = torch.tensor(rows, device=dev)
                last[rt] = x[rt, torch.tensor([last_at[r] - start for r in rows], device=dev)]
        self._prefilled(cache, t, lens, dev)
        return self._readout_rows(self.transformer.ln_f(last), weights=weights)

    @torch.no_grad()
    def extend(self, tokens, cache, logits="last", weights=None):
        """``tokens`` (B, n) int64: n new tokens per row in one call, row b's at positions ``cache.pos .. cache.pos + n - 1`` (after a
        prefill with ``lengths``: ``cache.positions[b] + j``, read on the device).  Their keys and values join the cache; position j's
        logits predict token j + 1.  Returns (B, vocab), the logits behind the last token, for ``logits="last"`` or (B, n, vocab) for
        ``"all"`` — what verifying a block of drafted tokens or scoring a continuation needs.  ``pos`` / ``positions`` advance
        by n; parked rows stay parked.  n == 1 is ``decode_step``.  ``KVCache.rewind`` steps back over tokens that are not kept.
        ``weights`` must be None: there is no e4m3-weight form of several new positions per row (NotImplementedError)."""
        _refuse_weights("extend", weights, "have no form for several new positions per row")
        self._refuse_fp8("extend", cache)
        self._refuse_shared("extend", cache)
        _refuse_paged("extend", cache)
        if tokens.dim() != 2:
            raise ValueError(f"OmniBioTA.extend: tokens must be (B, n), got {tuple(tokens.shape)}")
        b, n = tokens.shape
        if n == 0:
            raise ValueError("OmniBioTA.extend: no tokens (n = 0)")
        if logits not in ("last", "all"):
            raise ValueError(f"OmniBioTA.extend: logits must be 'last' or 'all', got {logits!r}")
        self._check_generation("extend", b, cache)
        if cache.pos == 0:
            raise ValueError("OmniBioTA.extend: the cache is empty: prefill a prompt first")
        cache.require_room("extend", n, detail=True)
        if n == 1:
            out = self.decode_step(tokens[:, 0], cache)
            return out if logits == "last" else out.unsqueeze(1)
        if not tokens.is_cuda:
            raise RuntimeError("OmniBioTA.extend: tokens must be on the GPU")
        x = self._extend_hidden(tokens, cache, cache.pos, cache.positions)
        cache.advance(n)
        if logits == "last":
            return self._readout_rows(self.transformer.ln_f(x[:, -1].contiguous()))
        return self._readout_rows(self.transformer.ln_f(x.view(b * n, -1))).view(b, n, -1)

    @torch.no_grad()
    def decode_step(self, tokens, cache, weights=None):
        """One new token per row, ``tokens`` (B,) int64, at position ``cache.pos`` of every row: its keys and values join the cache
        and the logits of the token after it come back, (B, vocab).  O(1) in projections, one read of the cache per layer.
        After a prefill with ``lengths`` row b's token goes to position ``cache.positions[b]``, read on the device; the positions of
        the rows not parked (>= 0) then advance by one there, ``cache.pos`` on the host.  A parked row's logits mean nothing.

        ``weights`` (``quantize_weights()``): every block's four products and the readout read e4m3 codes (``ops.block_step_w8``,
        ``ops.linear_small_m_w8``) — half the weight bytes — and give, bit for bit, this step of ``weights.dequantized_model()``.  On a
        ``KVCache`` of either dtype, uniform or per-row positions; not on a ``SharedPrefixCache`` (NotImplementedError).

        On a ``PagedKVCache`` every active row whose position opens a new page first gets one from the free list — ValueError, before
        anything is launched, if none is left — and the step reads and writes through the table (``ops.block_decode_paged``, on an fp8
        pool ``ops.block_decode_paged8``); ``weights=``
        raises NotImplementedError there."""
        if weights is not None:
            _refuse_weights("decode_step", weights if isinstance(cache, SharedPrefixCache) else None, "do not run on a shared-prefix cache (SharedPrefixCache)")
            _refuse_weights("decode_step", weights if isinstance(cache, PagedPositions) else None, "do not run on a paged cache (PagedKVCache)")
            _checked_weights(self, "OmniBioTA.decode_step", weights)
        if tokens.dim() != 1:
            raise ValueError(f"OmniBioTA.decode_step: tokens must be (B,), got {tuple(tokens.shape)}")
        b = tokens.shape[0]
        self._check_generation("decode_step", b, cache)
        if cache.pos == 0:
            raise ValueError("OmniBioTA.decode_step: the cache is empty: prefill a prompt first")
        cache.require_room("decode_step", 1)
        wte = self.transformer.wte.weight
        if not tokens.is_cuda:
            raise RuntimeError("OmniBioTA.decode_step: tokens must be on the GPU")
        if isinstance(cache, PagedPositions):                          # every active row whose position opens a new page gets one: ValueError
            cache.prepare_step()                                        # before anything is launched when none is left
        x = ops.embedding_fwd(tokens.contiguous(), wte)
        self._step_blocks(x, cache, cache.pos, cache.positions, weights)
        cache.advance(1)
        return self._readout_rows(self.transformer.ln_f(x), weights=weights)

    def _step_blocks(self, x, cache, pos, pos_rows, weights=None, ancestry=None):
        """``x`` (B, C), one new position per row, through every block against ``cache``, in place: the one place that chooses a cached
        step's op.  ``pos``: the position of every row, or with ``pos_rows`` (int32 (B,) on the device: rows mode, every row at its own
        position, read there) the host's bound on it.  A ``SharedPrefixCache`` — the group's prefix and the row's own slots, two buffers
        per layer — steps at suffix slot ``pos - n_prefix``, read through ``ancestry`` (beam search's table) when one is given; a
        ``PagedKVCache`` through its page table, by its dtype; a ``KVCache`` on the e4m3 codes of ``weights``, else by its dtype, else by its mode.  The
        cache is not advanced."""
        H = self.config.n_head
        for i, (block, kv) in enumerate(zip(self.transformer.h, cache.layers)):
            params, rope, to = self._block_params(block), block.attn.rope(), dict(ws=cache.decode_ws, out=x)
            if isinstance(cache, PagedPositions):                      # rows mode always: every row at its own position, its keys in its own pages
                step = ops.block_decode_paged8 if cache.dtype == "fp8" else ops.block_decode_paged
                step(x, params, rope, H, kv, cache.n_pages, cache.table, pos_rows, pos, **to)
            elif isinstance(cache, SharedPrefixCache):
                at = (kv[0], cache.prompts, cache.prefix_len, cache.n_prefix, kv[1], cache.max_new, pos - cache.n_prefix)
                if ancestry is None:
                    ops.block_decode_shared(x, params, rope, H, *at, **to)
                else:
                    ops.block_decode_beam(x, params, rope, H, *at, ancestry, **to)
            elif weights is not None:
                step = ops.block_step_w4 if weights.format == "mxfp4" else ops.block_step_w8
                step(x, weights.block_params(i), (weights.codes[i], weights.scales[i]), rope, H, kv, cache.max_len, pos, pos_rows, kv8=cache.dtype == "fp8", **to)
            elif cache.dtype == "fp8":
                ops.block_decode_kv8(x, params, rope, H, kv, cache.max_len, pos, pos_rows, **to)
            elif pos_rows is not None:
                ops.block_decode_rows(x, params, rope, H, kv, cache.max_len, pos_rows, pos, **to)
            else:
                ops.block_decode(x, params, rope, H, kv, cache.max_len, pos, **to)

    @torch.no_grad()
    def generate(self, idx, max_new_tokens, temperature=1.0, top_k=None, generator=None, eos_token=None, lengths=None, pad_token=None, top_p=None,
                 sampler="torch", kv_dtype="bf16", num_samples=None, loop=None, repetition_penalty=1.0, presence_penalty=0.0, frequency_penalty=0.0,
                 allowed_tokens=None, min_new_tokens=0, weights=None):
        """nanoGPT's generate(): ``idx`` (B, T0) int64 continued by up to ``max_new_tokens`` sampled tokens (``sample_next``); returns
        (B, T0 + n) int64.  The prompt runs once (``prefill``), every new token costs one ``decode_step``.  Where nanoGPT crops the
        context to block_size, this raises: T0 + max_new_tokens must fit.  ``eos_token``: a row that has produced it keeps producing
        it, and generation stops once every row has — the loop's only host synchronisation (none when ``eos_token is None``).
        Dropout is not applied, whatever ``self.training`` says.

        ``lengths`` (a host sequence of B ints, 1 <= len_b <= T0): prompts of different lengths, right-padded in ``idx``.  Every row
        gets up to ``max_new_tokens`` new tokens directly behind its own prompt; max(lengths) + max_new_tokens must fit block_size.
        Returns ``(out, out_lengths)``: out (B, max(lengths) + steps taken) int64, row b its prompt, its new tokens, then ``pad_token``
        (default: ``eos_token`` if given, else 0); out_lengths (B,) int64.  With ``eos_token`` a row that produced it is parked — its
        out_lengths ends with the EOS — and the loop stops once every row is: the same single host synchronisation as above.

        ``top_p``: nucleus sampling (``sample_next``).  ``sampler``: "torch" (``sample_next`` under ``generator``, as ever) or "device":
        the uniforms of the whole call are drawn once, ``torch.rand((max_new_tokens, B), generator=generator)``, and every step's
        tokens come from one launch on the step's bf16 logits (``ops.sample_logits``: the same rule, another random stream).

        ``kv_dtype``: "bf16" or "fp8", the ``KVCache`` the call builds (``KVCache``: the e4m3 cache, about half the bytes).

        ``num_samples`` (an int G >= 1; None: everything above): G samples of every prompt.  ``idx`` is (P, T0), the result
        (P * G, T0 + n) int64 with row p * G + g prompt p followed by its g-th sample — what ``generate(idx.repeat_interleave(G, 0), ...)``
        returns, drawn the same way (the device sampler's uniforms are ``torch.rand((max_new_tokens, P * G), generator=generator)``), but
        on a ``SharedPrefixCache``: the prompt is prefilled and stored once per prompt and read once per 32 samples.  Prompts of one
        length and a bf16 cache only: with ``lengths`` or ``kv_dtype="fp8"`` it raises ValueError.

        ``loop``: None (everything above), "device" or "graph": the token loop runs as a ``DecodeLoop`` — its state lives on the device,
        finished rows are parked there, and the host looks at the rows once every 16 tokens (never without ``eos_token``); "graph" also
        replays every step as one captured graph (B <= 64).  Same arguments, same shape of result, the device sampler's rule and uniforms;
        the tokens are those of ``loop=None, sampler="device"`` except where two logits lie closer than the attention's summation order
        resolves (``DecodeLoop``: the fixed bound).  Needs ``sampler="device"``; not with ``num_samples``: both raise ValueError.

        ``allowed_tokens``: what may be generated — a 1-D sequence or tensor of token ids, a bool (V,) mask, or a bool (rows, V) mask with
        one row per output row (P * G rows with ``num_samples=G``).  Everything else is treated as a logit of -inf at every step
        (``sampling.constrain_reference``; on the device the sampler reads the packed mask itself).  ``eos_token`` is not added: list it
        if rows are to end.  The prompt and ``pad_token`` are not restricted.  ``min_new_tokens``: ``eos_token`` is excluded as well until a
        row has that many new tokens.  Both work with every sampler, cache and loop above; with neither given nothing changes.
        ValueError before anything is launched: an id outside [0, V), a row that allows nothing, ``min_new_tokens`` outside
        [0, max_new_tokens] or without an ``eos_token``, a row that allows nothing but the held ``eos_token``.

        ``repetition_penalty`` (> 0), ``presence_penalty``, ``frequency_penalty``: damp repeats (``TokenPenalty``; the rule:
        include/omnibiote_hip_penalty.h, ``sampling.penalize_reference``).  At every step the logit x of a token of the row's prompt or of
        its output so far becomes x / repetition_penalty (x * repetition_penalty if x < 0), once per distinct token, and a token the row
        has generated c > 0 times loses presence_penalty + frequency_penalty * c; the restriction above applies to the result.  The
        device sampler reads the row's history itself, in its one launch (``ops.sample_logits(penalty=...)``: with ``loop=`` the loop's own
        token buffer, so a captured graph carries the penalties); the torch sampler draws from the rewritten copy.  With every
        sampler, cache, loop, ``lengths``, ``num_samples`` and ``weights``; with 1, 0, 0 nothing changes.  ValueError before anything is
        launched: a penalty that is not a finite number, ``repetition_penalty <= 0``, ``max_new_tokens > 32767`` with a penalty set.  Not
        part of ``generate_speculative`` / ``draft_and_verify`` (the verification would need the history to grow inside a drafted block),
        and there are no no-repeat n-grams or stop sequences.

        ``weights`` (``quantize_weights()``): the prompt runs on the dequantised weights and every new token's step reads the e4m3 codes:
        the tokens are those of ``weights.dequantized_model().generate(...)`` with the same arguments.  With every sampler, ``lengths``,
        ``kv_dtype``, ``eos_token``, ``allowed_tokens`` / ``min_new_tokens`` and ``loop``; not with ``num_samples`` (NotImplementedError)."""
        if weights is not None:
            _refuse_weights("generate", weights if num_samples is not None else None, "do not run on the shared-prefix cache of num_samples")
            _checked_weights(self, "OmniBioTA.generate", weights)
        if sampler not in ("torch", "device"):
            raise ValueError(f"OmniBioTA.generate: sampler must be 'torch' or 'device', got {sampler!r}")
        if loop not in (None, "device", "graph"):
            raise ValueError(f"OmniBioTA.generate: loop must be None, 'device' or 'graph', got {loop!r}")
        if loop is not None and sampler != "device":
            raise ValueError("OmniBioTA.generate: loop= draws with the device sampler (sampler='device'); torch.multinomial's stream is not part of it")
        if loop is not None and num_samples is not None:
            raise ValueError("OmniBioTA.generate: loop= does not run on the shared-prefix cache of num_samples")
        if kv_dtype not in ("bf16", "fp8"):
            raise ValueError(f"OmniBioTA.generate: kv_dtype must be 'bf16' or 'fp8', got {kv_dtype!r}")
        if num_samples is not None:
            if isinstance(num_samples, bool) or not isinstance(num_samples, int) or num_samples < 1:
                raise ValueError(f"OmniBioTA.generate: num_samples must be an integer of at least 1, got {num_samples!r}")
            if lengths is not None or kv_dtype != "bf16":
                raise ValueError("OmniBioTA.generate: num_samples needs prompts of one length (no lengths=) and the bf16 cache (no kv_dtype='fp8')")
        _check_top_p("OmniBioTA.generate", top_p)
        self._check_generation("generate", idx.shape[0] if idx.dim() == 2 else 0)
        b, t0 = _check_prompt("generate", idx)
        con = TokenConstraint.of("generate", allowed_tokens, min_new_tokens, max_new_tokens, eos_token, b * (num_samples or 1), self.config.vocab_size,
                                 idx.device)
        pen = TokenPenalty.of("OmniBioTA.generate", repetition_penalty, presence_penalty, frequency_penalty, max_new_tokens)
        lens = None if lengths is None else _check_lengths("generate", lengths, b, t0)
        longest = t0 if lens is None else max(lens)
        _check_room("generate", longest, max_new_tokens, self.config.block_size, longest=lens is not None)
        idx = idx[:, :longest]                                          # (ragged: without the columns every row counts as padding)
        if num_samples is None:
            rows = idx
        else:                                                               # row p G + g: prompt p, sample g
            rows, b = idx.repeat_interleave(num_samples, dim=0), b * num_samples
        dev = idx.device
        # (tokens (B, S), live (B, S) bool: the columns that hold a row's own tokens, a prefix of the row) — from nothing, the
        # device-resident loop or the host-driven one
        if max_new_tokens == 0:
            tokens = torch.zeros((b, 0), dtype=torch.int64, device=dev)
            live = tokens.bool()
        else:
            cache = KVCache(self, b, longest + max_new_tokens, dtype=kv_dtype) if num_samples is None else SharedPrefixCache(self, idx.shape[0], num_samples,
                                                                                                                           t0, max_new_tokens)
            logits = self.prefill(idx, cache, lengths=lens, weights=weights)
            us = _device_uniforms(sampler, max_new_tokens, b, temperature, top_k, dev, generator)
            if pen is not None:
                pen.bind(rows, lens, own_buffer=loop is None)
            if loop is not None:
                run = DecodeLoop(self, cache, max_steps=max_new_tokens, temperature=temperature, top_k=top_k, top_p=top_p,
                                 uniforms=us if isinstance(us, torch.Tensor) else None, eos_token=eos_token, capture=loop == "graph", penalty=pen,
                                 weights=weights, allowed=None if con is None else con.packed, hold_min=0 if con is None else con.min_new)
                run.start(logits)
                run.run(max_new_tokens - 1)
                tokens, n_new = run.result()
                live = _live(n_new, tokens.shape[1], dev)
            else:
                # one sampler call and one decode_step per token; with an eos_token one host read per step (has every row finished?), none
                # without.  A finished row is fed eos_token from then on; behind ragged prompts it is parked as well
                tokens, done = [], torch.zeros(b, dtype=torch.bool, device=dev)
                for i in range(max_new_tokens):
                    nxt = _next_tokens("generate", logits, temperature, top_k, top_p, generator, None if us is None else us[i], con, i, pen)
                    if eos_token is not None:
                        nxt = torch.where(done, torch.full_like(nxt, eos_token), nxt)
                        done = done | (nxt == eos_token)
                    if pen is not None:
                        pen.record(i, nxt)
                    tokens.append(nxt)
                    if i + 1 == max_new_tokens or (eos_token is not None and bool(done.all())):
                        break
                    if lens is not None and eos_token is not None:          # they store nothing and read nothing from here on
                        cache.park(done)
                    logits = self.decode_step(nxt, cache, weights=weights)
                tokens = torch.stack(tokens, dim=1)
                ended = tokens == (-1 if eos_token is None else eos_token)  # (no token is -1: without an eos_token no row ends)
                live = ended.cumsum(dim=1) - ended.to(torch.int64) == 0     # a row's own tokens: up to and including its first EOS
        if lens is not None:
            return ragged_output(idx, lens, tokens, live, _default_pad(pad_token, eos_token))
        if eos_token is not None:                                       # a finished row keeps producing EOS
            tokens = torch.where(live, tokens, torch.full_like(tokens, eos_token))
        return torch.cat([rows, tokens], dim=1)

    @torch.no_grad()
    def generate_many(self, prompts, max_new_tokens, batch, n_pages=None, temperature=1.0, top_k=None, top_p=None, eos_token=None, generator=None,
                      kv_dtype="bf16", share_prefix=False, stats=None):
        """Continuous batching: ``prompts``, a sequence of 1-D int64 tensors of any lengths, each continued by up to ``max_new_tokens``
        tokens, ``batch`` of them at a time on a ``PagedKVCache`` of ``n_pages`` pages.  Returns a list in the same order, each entry the
        prompt followed by its new tokens up to and including its first ``eos_token``, int64 on the model's device.  A row that ends —
        with its ``eos_token`` or after ``max_new_tokens`` — is released at once, and its slot and its pages serve the next waiting
        prompt while the other rows go on: no row waits for the longest, and memory follows what the rows hold.

        The rule (``paged.PagedSchedule``, which is all of it, without tensors): requests wait in the given order; a request needs
        ceil((len + max_new_tokens) / 64) pages and is admitted when a slot is free and the pages not yet promised to running requests
        cover its need — strictly first-in first-out, nothing is skipped.  ``n_pages=None``: enough for ``batch`` requests of the largest
        need.  ValueError before anything is launched for a request that can never fit: ``len + max_new_tokens > block_size``, or a need
        above ``n_pages``.  The requests admitted in one round are prefilled together, right-padded (``prefill(rows=)``), and each draws
        its first token from the prefill's logits.

        The device sampler only (``ops.sample_logits``: ``temperature``, ``top_k``, ``top_p`` as in ``generate``).  The uniforms are
        ``torch.rand((max_new_tokens, len(prompts)), generator=generator)`` on the model's device, drawn once: request r draws its k-th
        token against [k, r], wherever and whenever it runs; a greedy setting draws nothing.  With an ``eos_token`` the host reads the
        step's tokens once per step, as ``generate``'s loop does; without one it reads nothing until the end.

        ``kv_dtype``: "bf16" or "fp8", the ``PagedKVCache`` the call builds (``PagedKVCache``: the e4m3 pool, the same pages at about half
        the bytes).  The schedule, the promise rule, the uniforms and the default ``n_pages`` do not depend on it.

        ``share_prefix`` (bf16 only; False: nothing below happens): every admitted request is looked up in a ``paged.PrefixIndex`` kept
        for the call — exact token content of whole 64-token pages, chained from position 0 — takes the longest chain of pages it finds,
        names them instead of computing them (``prefill(shared_pages=)``) and computes the rest of its prompt, at least one token,
        against them.  Its own full prompt pages are registered once its prefill is enqueued: later readers are ordered behind it on the
        stream.  Requests admitted in the same round share too: one that has a page in common with an earlier request of the round
        waits for that request's prefill call, so a round may make several.  A finished request's prompt pages stay findable while the
        free list keeps them.  The promise rule is unchanged: sharing makes a request hold fewer pages than promised, never more.
        ``share_prefix=True`` with ``kv_dtype="fp8"`` raises NotImplementedError before anything is launched.

        ``stats`` (an optional dict, filled by the call): ``prefill_positions`` (prompt positions computed), ``shared_positions`` (prompt
        positions taken from shared pages), ``peak_pages`` (the most pages in use at once) and ``decode_steps``.

        Not built: speculative decoding, the device-resident loop and graph capture, sharing of generated (non-prompt) pages and
        copy-on-write, admission that counts shared pages against the promise, preemption or swapping of running requests, penalties
        and token restrictions, the torch sampler."""
        from .paged import KV_PAGE, PagedSchedule, PrefixIndex
        self._check_generation("generate_many", 0)
        if kv_dtype not in ("bf16", "fp8"):
            raise ValueError(f"OmniBioTA.generate_many: kv_dtype must be 'bf16' or 'fp8', got {kv_dtype!r}")
        if share_prefix and kv_dtype == "fp8":
            raise NotImplementedError("OmniBioTA.generate_many: share_prefix=True needs kv_dtype='bf16': several new positions per row over the pages "
                                      "of an e4m3 pool are not built")
        _check_top_p("OmniBioTA.generate_many", top_p)
        if temperature < 0:
            raise ValueError(f"OmniBioTA.generate_many: temperature must not be negative, got {temperature}")
        if top_k is not None and top_k < 1:
            raise ValueError(f"OmniBioTA.generate_many: top_k must be at least 1, got {top_k}")
        prompts = list(prompts)
        for r, p in enumerate(prompts):
            if not isinstance(p, torch.Tensor) or p.dim() != 1 or p.dtype != torch.int64:
                raise ValueError(f"OmniBioTA.generate_many: prompts must be 1-D int64 tensors, prompts[{r}] is not")
        sched = PagedSchedule([p.numel() for p in prompts], max_new_tokens, batch, n_pages, self.config.block_size)
        if not prompts:
            return []
        wte = self.transformer.wte.weight
        _require_hip(wte, "OmniBioTA")
        dev, R, steps, B = wte.device, len(prompts), sched.max_new, sched.batch
        prompts = [p.to(dev) for p in prompts]
        cache = PagedKVCache(self, B, sched.n_pages, max(p.numel() for p in prompts) + steps, dtype=kv_dtype)
        greedy = top_k == 1 or temperature == 0
        # one column more than there are requests: what an idle slot draws against and writes to
        us = None if greedy else torch.cat([torch.rand((steps, R), device=dev, generator=generator), torch.zeros((steps, 1), device=dev)], dim=1)
        out = torch.zeros((R + 1, steps), dtype=torch.int64, device=dev)
        logits = torch.zeros((B, self.config.vocab_size), dtype=torch.bfloat16, device=dev)
        slot_req, slot_k = [R] * B, [0] * B                            # the host's account: the slot's request (R: idle) and its tokens so far
        n_new = [0] * R
        at, changed = None, True                                        # the same on the device, int64 (2, B): uploaded when a slot changes hands
        count = dict(prefill_positions=0, shared_positions=0, peak_pages=0, decode_steps=0)
        index = PrefixIndex(cache.book) if share_prefix else None
        host = [p.tolist() for p in prompts] if share_prefix else None  # (the prompts' tokens on the host: what the index compares)

        def prefill_round(admitted, shared=None):
            rows = [slot for _, slot in admitted]
            lens = [prompts[r].numel() for r, _ in admitted]
            idx = torch.nn.utils.rnn.pad_sequence([prompts[r] for r, _ in admitted], batch_first=True)
            more = {} if shared is None else dict(shared_pages=shared)
            logits[torch.tensor(rows, device=dev)] = self.prefill(idx, cache, lengths=lens, rows=rows, **more)
            taken = 0 if shared is None else KV_PAGE * sum(len(p) for p in shared)
            count["prefill_positions"] += sum(lens) - taken
            count["shared_positions"] += taken

        while not sched.done:
            admitted = sched.admit()
            if admitted and not share_prefix:
                prefill_round(admitted)
            waiting = admitted if share_prefix else []
            while waiting:                                              # one prefill call per pass: whoever shares with a request of this pass waits for the next
                now, later, seen_now = [], [], PrefixIndex()
                for r, slot in waiting:
                    found = index.lookup(host[r])
                    if len(seen_now.lookup(host[r])) > len(found):
                        later.append((r, slot))
                    else:
                        now.append((r, slot, found))
                        seen_now.register(host[r], range(len(seen_now), len(seen_now) + len(host[r]) // KV_PAGE))   # (stand-in page numbers, each once)
                prefill_round([(r, slot) for r, slot, _ in now], [found for _, _, found in now])
                for r, slot, _ in now:
                    index.register(host[r], cache.book.row_pages[slot])
                waiting = later
            if admitted:
                count["peak_pages"] = max(count["peak_pages"], cache.pages_in_use)
                for r, slot in admitted:
                    slot_req[slot], slot_k[slot] = r, 0
                changed = True
            if changed:
                at, changed = torch.tensor([slot_req, slot_k], dtype=torch.int64).to(dev), False
            nxt = ops.sample_logits(logits, None if greedy else us[at[1], at[0]], temperature, top_k, top_p)
            out[at[0], at[1]] = nxt
            seen = nxt.tolist() if eos_token is not None else None      # (the step's one host read)
            for slot, r in enumerate(slot_req):
                if r == R:
                    continue
                slot_k[slot] += 1
                if slot_k[slot] == steps or (seen is not None and seen[slot] == eos_token):
                    n_new[r] = slot_k[slot]
                    sched.finish(r)
                    cache.release(slot)
                    slot_req[slot], slot_k[slot], changed = R, 0, True
            if any(r != R for r in slot_req):
                logits = self.decode_step(nxt, cache)
                count["decode_steps"] += 1
                count["peak_pages"] = max(count["peak_pages"], cache.pages_in_use)
                if not changed:
                    at[1] += at[0] < R                                  # (no slot changed hands: the running ones count on, on the device)
        if stats is not None:
            stats.update(count)
        return [torch.cat([p, out[r, :n_new[r]]]) for r, p in enumerate(prompts)]

    @torch.no_grad()
    def generate_beam(self, idx, max_new_tokens, num_beams=4, eos_token=None, pad_token=None, length_penalty=0.0, allowed_tokens=None):
        """Beam search: the ``num_beams`` = W most probable continuations of every prompt of ``idx`` (P, T0) int64 that a beam of that width
        finds, deterministic.  Returns a ``BeamResult`` (sequences (P, W, T0 + n), scores (P, W), lengths (P, W)), n the steps taken.

        The W beams of a prompt are the rows of one group of a ``SharedPrefixCache(self, P, W, T0, max_new_tokens)``: the prompt is
        prefilled and stored once and read once per step.  After the prefill the beams are identical, so beam 0 starts at score 0 and
        the others at -inf.  Every step is one ``ops.beam_select`` (include/omnibiote_hip_beam.h: per prompt the W best of the W * V
        candidates ``score + log_softmax``, equal scores to the lower beam, then the lower token), the embedding of the chosen tokens,
        ``ops.block_decode_beam`` per layer and the readout.  No key or value is moved when a beam continues another: the selection
        keeps an ancestry table — which row wrote suffix slot j of the history beam b now continues — in two (P * W, max_new_tokens)
        int32 buffers used in turn, and the attention reads through it.  The result is one gather through the last table.

        The rule: the selection inside the loop compares RAW sums of log-probabilities; a beam that has produced ``eos_token`` is finished,
        keeps its slot and its frozen score and competes with it against the running beams (it proposes itself as its only
        continuation).  With an ``eos_token`` the loop reads ``done.all()`` once per step — the only host synchronisation — and stops
        once every beam of every prompt is finished; without one nothing is read.  ``lengths`` counts a beam's new tokens up to and
        including its first EOS, the positions behind it hold ``pad_token`` (default: ``eos_token`` if given, else 0).  The beams of a
        prompt come back ordered by ``scores / lengths ** length_penalty``, descending, by a stable sort of the finished result
        (``length_penalty = 0``: by raw score, the order the last selection left); a dead beam — fewer than W candidates existed, as
        under a small ``allowed_tokens`` — has score -inf and comes last.

        ``allowed_tokens``: token ids, a bool (V,) mask or a bool (P, V) mask, one row per prompt; everything else never enters a beam.
        ``eos_token`` is not added.  ValueError before anything is launched: a model that is not autoregressive, ``num_beams`` outside
        [1, 32], T0 + max_new_tokens > block_size, an ``eos_token`` outside the vocabulary, an allowed set that is empty.  Not built:
        ``lengths=``, the fp8 cache, ``weights=``, penalties, ``min_new_tokens``, a temperature, ``loop=``, diverse or length-pruned beams,
        more than 32 beams, a vocabulary above 65 536."""
        self._check_generation("generate_beam", 0)
        W = num_beams
        if isinstance(W, bool) or not isinstance(W, int) or not 1 <= W <= ops.BEAM_MAX_WIDTH:
            raise ValueError(f"OmniBioTA.generate_beam: num_beams must be an integer in [1, {ops.BEAM_MAX_WIDTH}], got {W!r}")
        P, t0 = _check_prompt("generate_beam", idx, "(P, T0)", min_rows=1)
        n = int(max_new_tokens)
        _check_room("generate_beam", t0, n, self.config.block_size)
        V = self.config.vocab_size
        if eos_token is not None and not 0 <= int(eos_token) < V:
            raise ValueError(f"OmniBioTA.generate_beam: eos_token {eos_token} outside [0, vocab_size = {V})")
        if not math.isfinite(float(length_penalty)):
            raise ValueError(f"OmniBioTA.generate_beam: length_penalty must be a finite number, got {length_penalty!r}")
        con = TokenConstraint.of("generate_beam", allowed_tokens, 0, n, eos_token, P, V, idx.device)
        dev, B = idx.device, P * W
        score = torch.zeros((P, W), dtype=torch.float32, device=dev)
        score[:, 1:] = float("-inf")
        score = score.view(B)
        if n == 0:
            return BeamResult(idx.unsqueeze(1).repeat(1, W, 1), score.view(P, W), torch.zeros((P, W), dtype=torch.int64, device=dev))
        cache = SharedPrefixCache(self, P, W, t0, n)
        logits = self.prefill(idx, cache)
        packed = None if con is None else (con.packed if con.packed.dim() == 1 else con.packed.repeat_interleave(W, dim=0))
        done = torch.zeros(B, dtype=torch.uint8, device=dev)
        ancestry = [torch.zeros((B, n), dtype=torch.int32, device=dev) for _ in range(2)]
        hist = torch.zeros((n, B), dtype=torch.int64, device=dev)
        parent = torch.empty(B, dtype=torch.int32, device=dev)
        token = torch.empty(B, dtype=torch.int64, device=dev)
        ws = ops.beam_select_workspace(P, W, dev)
        wte = self.transformer.wte.weight
        steps = 0
        for i in range(n):
            table = ancestry[(i + 1) & 1]
            ops.beam_select(logits, score, done, ancestry[i & 1], table, hist, i, W, eos_token=eos_token, allowed_packed=packed, parent=parent, token=token,
                            score_out=score, done_out=done, ws=ws)
            steps = i + 1
            if steps == n or (eos_token is not None and bool(done.all())):
                break
            x = ops.embedding_fwd(token, wte)
            self._step_blocks(x, cache, cache.pos, None, ancestry=table)    # (suffix slot i)
            cache.advance(1)
            logits = self._readout_rows(self.transformer.ln_f(x))
        from .sampling import beam_sequences_reference
        new, lengths = beam_sequences_reference(hist, ancestry[steps & 1], steps, W, eos_token, _default_pad(pad_token, eos_token))
        score, lengths, new = score.view(P, W), lengths.view(P, W), new.view(P, W, steps)
        key = score / lengths.clamp(min=1).to(torch.float32) ** float(length_penalty)
        order = torch.sort(key, dim=1, descending=True, stable=True).indices
        seq = torch.cat([idx.unsqueeze(1).expand(P, W, t0), new.gather(1, order.unsqueeze(2).expand(P, W, steps))], dim=2)
        return BeamResult(seq, score.gather(1, order), lengths.gather(1, order))

    @torch.no_grad()
    def draft_and_verify(self, draft, pending, cache, draft_cache, k, uniforms=None, temperature=1.0, top_k=None, top_p=None, allowed=None, hold_token=None,
                         emitted=None, min_emitted=0, weights=None, draft_weights=None):
        """One round of speculative decoding, everything but the step back.  ``pending`` (B,) int64 is every row's last emitted token,
        in neither cache yet; ``cache`` (this model's) and ``draft_cache`` (``draft``'s) stand at the same per-row positions.  The draft
        runs k ``decode_step``s, drawing x_0 .. x_{k-1} with ``ops.sample_logits`` from its logits q_0 .. q_{k-1}, and one more that
        only ingests x_{k-1}; this model runs ``extend([pending, x_0 .. x_{k-1}], logits="all")``; ``ops.spec_verify`` decides.  Both
        caches then hold k + 1 new positions per row.  ``uniforms``: None (greedy: the draft proposes its argmax, q is not kept) or the
        round's ``(draws (k, B), u_accept (B, k), u_draw (B,))`` float32 on the device.  Returns ``(x (B, k) int64, n_accept (B,) int32,
        token (B,) int64)`` on the device; nothing waits for them.  The caller reads n_accept and steps both caches back by
        ``k - n_accept[b]`` (``rewind_rows``): row b has emitted x_0 .. x_{a-1} and ``token``, its new pending token.

        ``allowed`` (a packed mask, uint8 (n,) or (B, n) on the device), ``hold_token``, ``emitted`` (B,) int32 — what every row has emitted,
        the pending token included — and ``min_emitted`` restrict the draft's draws and the verification alike
        (include/omnibiote_hip_constrain.h): the draft's j-th draw and the verification's position j hold ``hold_token`` while
        ``emitted[b] + j < min_emitted``.  With none given the round runs the unrestricted entry points.  ``weights`` / ``draft_weights``
        must be None: e4m3 weights are not built for either model of a round (NotImplementedError)."""
        _refuse_weights("draft_and_verify", weights if weights is not None else draft_weights,
                        "are not built for speculative decoding, for the target (several new positions per row) or the draft")
        self._refuse_fp8("draft_and_verify", cache)         # (the draft only takes decode steps: its cache may be either)
        self._refuse_shared("draft_and_verify", cache)
        _refuse_paged("draft_and_verify", cache)
        _refuse_paged("draft_and_verify", draft_cache, "which cannot step back over rejected tokens")
        b = pending.shape[0]
        greedy = uniforms is None or temperature == 0 or top_k == 1
        draws, u_accept, u_draw = (None, None, None) if greedy else uniforms
        q = None if greedy else torch.empty((b, k, self.config.vocab_size), dtype=torch.bfloat16, device=pending.device)
        xs, tok = [], pending
        for j in range(k):
            ql = draft.decode_step(tok, draft_cache)
            if q is not None:
                q[:, j] = ql
            tok = ops.sample_logits(ql, None if greedy else draws[j], temperature, top_k, top_p, **_restriction(allowed, hold_token, emitted, min_emitted, j))
            xs.append(tok)
        draft.decode_step(tok, draft_cache)                             # x_{k-1} joins the draft's cache as it joins the target's below
        x = torch.stack(xs, dim=1)
        p = self.extend(torch.cat([pending.unsqueeze(1), x], dim=1), cache, logits="all")
        n_accept, token = ops.spec_verify(p, q, x, u_accept, u_draw, temperature, top_k, top_p, **_restriction(allowed, hold_token, emitted, min_emitted))
        return x, n_accept, token

    @torch.no_grad()
    def generate_speculative(self, idx, max_new_tokens, draft, k=4, temperature=1.0, top_k=None, top_p=None, generator=None, eos_token=None,
                             lengths=None, pad_token=None, return_stats=False, kv_dtype="bf16", num_samples=None, allowed_tokens=None, min_new_tokens=0,
                             weights=None, draft_weights=None):
        """``generate`` by draft and verify: ``draft`` — any autoregressive OmniBioTA on the same device with the same vocabulary, a smaller
        model in practice, this model itself for a self-check — proposes ``k`` tokens per round (1 <= k <= 31), this model scores them in
        one ``extend`` and ``ops.spec_verify`` keeps a prefix of them and adds one token of its own, so that every emitted token is
        distributed as this model's own sampling under ``temperature`` / ``top_k`` / ``top_p`` would have it (the rule:
        ``sampling.verify_reference``; with ``top_k == 1`` or ``temperature == 0`` the output is this model's greedy stream up to the
        two paths' rounding).  A round (``draft_and_verify``) emits between 1 and k + 1 tokens per row.

        Both models get a ``KVCache`` of their own with one position per row; ``lengths``, ``eos_token`` and ``pad_token`` as in
        ``generate``.  The last round may write k positions it does not keep: longest prompt + max_new_tokens + k must fit the
        block_size of both models.  All uniforms come from ``generator`` on the device, one ``torch.rand`` per round, so a seeded call
        is repeatable.  One host synchronisation per round (how many tokens stood, and where an EOS lies) and one for the first token
        when ``eos_token`` is given; rows that have their ``max_new_tokens`` or have emitted ``eos_token`` are parked, and the loop ends
        when every row is.

        Returns (B, T0 + max_new_tokens) int64, a row that emitted ``eos_token`` filled with it to the end; with ``lengths``
        ``(out, out_lengths)`` as ``generate`` does (``ragged_output``).  ``return_stats`` appends a dict of host ints: ``rounds``, and
        over all rows and rounds ``drafted`` (k per running row) and ``accepted`` (the drafted tokens that stood).

        ``allowed_tokens`` and ``min_new_tokens`` as in ``generate``: the draft's draws and the verification take the same mask and the same
        held ``eos_token``, so the emitted tokens are distributed as this model's own restricted sampling; the rows' emitted counts reach
        the device once per round, behind the round's host synchronisation.  ``weights`` / ``draft_weights`` must be None: e4m3 weights
        are not built for either model (NotImplementedError)."""
        what = "generate_speculative"
        _refuse_weights(what, weights if weights is not None else draft_weights,
                        "are not built for speculative decoding, for the target (several new positions per row) or the draft")
        if num_samples is not None:
            raise NotImplementedError(f"OmniBioTA.{what}: num_samples: verifying a drafted block attends from several new positions per row, which "
                                      "is not built over a shared-prefix cache (SharedPrefixCache); repeat the prompts instead")
        if kv_dtype == "fp8":
            raise NotImplementedError(f"OmniBioTA.{what}: kv_dtype 'fp8': verifying a drafted block attends from several new positions per row, "
                                      "which is not built over an fp8 cache; use the bf16 cache")
        if kv_dtype != "bf16":
            raise ValueError(f"OmniBioTA.{what}: kv_dtype must be 'bf16' or 'fp8', got {kv_dtype!r}")
        _check_top_p(f"OmniBioTA.{what}", top_p)
        self._check_generation(what, idx.shape[0] if idx.dim() == 2 else 0)
        if not isinstance(draft, OmniBioTA) or not draft.config.autoregressive:
            raise ValueError(f"OmniBioTA.{what}: draft must be an autoregressive OmniBioTA")
        if draft.config.vocab_size != self.config.vocab_size:
            raise ValueError(f"OmniBioTA.{what}: the draft's vocab_size {draft.config.vocab_size} is not this model's {self.config.vocab_size}")
        if draft.transformer.wte.weight.device != self.transformer.wte.weight.device:
            raise ValueError(f"OmniBioTA.{what}: the draft is on {draft.transformer.wte.weight.device}, this model on {self.transformer.wte.weight.device}")
        b, t0 = _check_prompt(what, idx)
        if not 1 <= int(k) <= L.SPEC_VERIFY_MAX_K:
            raise ValueError(f"OmniBioTA.{what}: k must lie in [1, {L.SPEC_VERIFY_MAX_K}], got {k}")
        k = int(k)
        if temperature < 0:
            raise ValueError(f"OmniBioTA.{what}: temperature must not be negative, got {temperature}")
        if top_k is not None and top_k < 1:
            raise ValueError(f"OmniBioTA.{what}: top_k must be at least 1, got {top_k}")
        lens = [t0] * b if lengths is None else _check_lengths(what, lengths, b, t0)
        longest = max(lens)
        _check_room(what, longest, max_new_tokens, min(self.config.block_size, draft.config.block_size), longest=True, drafted=k)
        con = TokenConstraint.of(what, allowed_tokens, min_new_tokens, max_new_tokens, eos_token, b, self.config.vocab_size, idx.device)
        pad = _default_pad(pad_token, eos_token)
        idx = idx[:, :longest]
        dev = idx.device
        stats = dict(rounds=0, drafted=0, accepted=0)

        def result(tokens, counts):
            if lengths is None:
                out = (torch.cat([idx, tokens], dim=1),)
            else:
                out = ragged_output(idx, lens, tokens, _live(torch.tensor(counts, device=dev), tokens.shape[1], dev), pad)
            out = out + (stats,) if return_stats else out
            return out[0] if len(out) == 1 else out

        if max_new_tokens == 0:
            return result(torch.zeros((b, 0), dtype=torch.int64, device=dev), [0] * b)
        greedy = top_k == 1 or temperature == 0
        cache, draft_cache = KVCache(self, b, longest + max_new_tokens + k), KVCache(draft, b, longest + max_new_tokens + k)
        logits = self.prefill(idx, cache, lengths=lens)
        draft.prefill(idx, draft_cache, lengths=lens)
        pending = ops.sample_logits(logits, None if greedy else torch.rand(b, device=dev, generator=generator), temperature, top_k, top_p,
                                    **_step_restriction(con))
        # the host's account: where the rows stand in both caches (-1: parked), what each has emitted and where in `cols` it lies
        at = list(lens)
        cols, width = [pending.unsqueeze(1)], 1
        where = [[0] for _ in range(b)]
        first = pending.tolist() if eos_token is not None else None
        done = [max_new_tokens == 1 or (first is not None and first[r] == eos_token) for r in range(b)]
        newly = list(done)
        col = torch.arange(k + 1, device=dev).view(1, -1)
        while not all(done):
            if any(newly):                                              # park what the last round finished: it stores and reads nothing
                mask = torch.tensor(newly, device=dev)
                cache.park(mask)
                draft_cache.park(mask)
                at = [-1 if d else p for p, d in zip(at, done)]
            us = None
            if not greedy:
                r = torch.rand(b * (2 * k + 1), device=dev, generator=generator)
                us = r[:k * b].view(k, b), r[k * b:2 * k * b].view(b, k), r[2 * k * b:]
            x, n_accept, token = self.draft_and_verify(draft, pending, cache, draft_cache, k, us, temperature, top_k, top_p,
                                                       **_round_restriction(con, [len(w) for w in where], dev))   # (as of the last round's read)
            a_dev = n_accept.long().unsqueeze(1)
            emitted = torch.cat([x, token.unsqueeze(1)], dim=1).scatter(1, a_dev, token.unsqueeze(1))   # x_0 .. x_{a-1}, token, (stale)
            if eos_token is None:
                read = [(a, k + 1) for a in n_accept.tolist()]         # the round's host synchronisation
            else:
                hit = (emitted == eos_token) & (col <= a_dev)
                eos_at = torch.where(hit.any(dim=1), hit.to(torch.uint8).argmax(dim=1), torch.full((b,), k + 1, device=dev))
                read = torch.stack([a_dev.squeeze(1), eos_at], dim=1).tolist()   # the round's host synchronisation
            stats["rounds"] += 1
            back, now, newly = [0] * b, [p + k + 1 if p >= 0 else -1 for p in at], [False] * b
            for r in range(b):
                if done[r]:
                    continue
                a, e = read[r]
                n = min(a + 1, e + 1, max_new_tokens - len(where[r]))   # tokens of this round that count
                stats["drafted"] += k
                stats["accepted"] += a
                where[r] += range(width, width + n)
                back[r] = k + 1 - n                                     # the pending token and the first n - 1 of this round's stay
                newly[r] = done[r] = len(where[r]) >= max_new_tokens or e < n
            cache.rewind_rows(back, now)
            draft_cache.rewind_rows(back, now)
            at = [p - n if p >= 0 else -1 for p, n in zip(now, back)]
            cols.append(emitted)
            width += k + 1
            pending = token
        counts = [len(w) for w in where]
        steps = max_new_tokens if lengths is None else max(counts)
        fill = eos_token if lengths is None and eos_token is not None else pad
        every = torch.cat(cols + [torch.full((b, 1), int(fill), dtype=torch.int64, device=dev)], dim=1)
        gather = torch.tensor([w[:steps] + [width] * (steps - len(w)) for w in where], device=dev)
        return result(every.gather(1, gather), counts)

    @torch.no_grad()
    def lookup_and_verify(self, pending, cache, history, lengths, k, uniforms=None, temperature=1.0, top_k=None, top_p=None, ngram=(1, 4)):
        """One round of speculative decoding without a draft model, everything but the step back: ``draft_and_verify`` with an n-gram
        lookup in every row's own tokens as the draft.  ``pending`` (B,) int64 is every row's last emitted token, not in ``cache`` yet;
        ``history`` (B, W) int64 and ``lengths`` (B,) int32, both on the device, hold every row's tokens so far, the pending one last:
        ``history[b, :lengths[b]]``.  ``ops.lookup_draft`` proposes x_0 .. x_{k-1} — what followed the most recent longest earlier
        occurrence of the row's last ``ngram`` = (g_min, g_max) tokens, or the last token repeated — at the cost of no model
        evaluation; this model runs ``extend([pending, x_0 .. x_{k-1}], logits="all")``; ``ops.spec_verify_point`` decides, the draft
        distribution of a position being the point mass on its token.  The cache then holds k + 1 new positions per row.  ``uniforms``:
        None (greedy) or the round's ``(u_accept (B, k), u_draw (B,))`` float32 on the device.  Returns ``(x (B, k) int64, n_accept (B,)
        int32, token (B,) int64, match_len (B,) int32)`` on the device; nothing waits for them.  The caller reads n_accept and steps the
        cache back by ``k - n_accept[b]`` (``rewind_rows``): row b has emitted x_0 .. x_{a-1} and ``token``, its new pending token."""
        what = "lookup_and_verify"
        self._refuse_fp8(what, cache)
        self._refuse_shared(what, cache)
        _refuse_paged(what, cache)
        if isinstance(k, bool) or not isinstance(k, int) or not 1 <= k <= L.SPEC_VERIFY_MAX_K:
            raise ValueError(f"OmniBioTA.{what}: k must lie in [1, {L.SPEC_VERIFY_MAX_K}], got {k!r}")
        ngram = ops._ngram(f"OmniBioTA.{what}", ngram)
        greedy = uniforms is None or temperature == 0 or top_k == 1
        u_accept, u_draw = (None, None) if greedy else uniforms
        x, match_len = ops.lookup_draft(history, lengths, k, ngram, self.config.vocab_size)
        p = self.extend(torch.cat([pending.unsqueeze(1), x], dim=1), cache, logits="all")
        n_accept, token = ops.spec_verify_point(p, x, u_accept, u_draw, temperature, top_k, top_p)
        return x, n_accept, token, match_len

    @torch.no_grad()
    def generate_lookup(self, idx, max_new_tokens, k=8, ngram=(1, 4), temperature=1.0, top_k=None, top_p=None, generator=None, eos_token=None,
                        lengths=None, pad_token=None, return_stats=False):
        """``generate_speculative`` without a draft model: every round (``lookup_and_verify``) drafts ``k`` tokens per row (1 <= k <= 31)
        by an n-gram lookup in the row's own prompt and output — the tokens that followed the most recent longest earlier occurrence
        of its last ``ngram`` = (g_min, g_max) tokens, 1 <= g_min <= g_max <= 16 — scores them in one ``extend`` and keeps a prefix of
        them plus one token of its own, so that every emitted token is distributed as this model's own sampling under ``temperature``
        / ``top_k`` / ``top_p`` would have it (the rule: ``sampling.verify_point_reference``; with ``top_k == 1`` or ``temperature == 0``
        the output is this model's greedy stream up to the two paths' rounding).  The draft costs no model evaluation: sequences with
        tandem repeats, repeated motifs or continuations that copy the prompt gain up to k + 1 tokens per round, others pay the
        wider ``extend`` for one.

        ``lengths``, ``eos_token``, ``pad_token``, the return forms and ``return_stats`` as in ``generate_speculative``; the stats gain
        ``matched``, the running row-rounds whose lookup found a match.  The last round may write k positions it does not keep: longest
        prompt + max_new_tokens + k must fit block_size.  The call owns a history buffer (B, longest + max_new_tokens + k + 1) int64 —
        at most 8192 columns — and a device int32 length vector: a round's k + 1 emitted columns are written behind each row's length
        on the device before the round's one host synchronisation, the lengths then advance by the tokens that count, and the next
        round overwrites the rest.  All uniforms come from ``generator`` on the device, one ``torch.rand(B * (k + 1))`` per round and one
        draw for the first token, so a seeded call is repeatable.

        Not built: ``allowed_tokens`` / ``min_new_tokens`` and the penalties, ``kv_dtype="fp8"``, ``num_samples``, ``weights=``, paged caches,
        the device-resident loop and graph capture."""
        what = "generate_lookup"
        _check_top_p(f"OmniBioTA.{what}", top_p)
        self._check_generation(what, idx.shape[0] if idx.dim() == 2 else 0)
        b, t0 = _check_prompt(what, idx)
        if isinstance(k, bool) or not isinstance(k, int) or not 1 <= k <= L.SPEC_VERIFY_MAX_K:
            raise ValueError(f"OmniBioTA.{what}: k must lie in [1, {L.SPEC_VERIFY_MAX_K}], got {k!r}")
        ngram = ops._ngram(f"OmniBioTA.{what}", ngram)
        if temperature < 0:
            raise ValueError(f"OmniBioTA.{what}: temperature must not be negative, got {temperature}")
        if top_k is not None and top_k < 1:
            raise ValueError(f"OmniBioTA.{what}: top_k must be at least 1, got {top_k}")
        lens = [t0] * b if lengths is None else _check_lengths(what, lengths, b, t0)
        longest = max(lens)
        _check_room(what, longest, max_new_tokens, self.config.block_size, longest=True, drafted=k, draft_model=False)
        width = longest + max_new_tokens + k + 1
        if width > L.LOOKUP_MAX_HISTORY:
            raise ValueError(f"OmniBioTA.{what}: a history of {width} tokens per row (the longest prompt + max_new_tokens + k + 1) exceeds the "
                             f"{L.LOOKUP_MAX_HISTORY} the lookup takes")
        pad = _default_pad(pad_token, eos_token)
        idx = idx[:, :longest]
        dev = idx.device
        stats = dict(rounds=0, drafted=0, accepted=0, matched=0)

        def result(tokens, counts):
            if lengths is None:
                out = (torch.cat([idx, tokens], dim=1),)
            else:
                out = ragged_output(idx, lens, tokens, _live(torch.tensor(counts, device=dev), tokens.shape[1], dev), pad)
            out = out + (stats,) if return_stats else out
            return out[0] if len(out) == 1 else out

        if max_new_tokens == 0:
            return result(torch.zeros((b, 0), dtype=torch.int64, device=dev), [0] * b)
        greedy = top_k == 1 or temperature == 0
        cache = KVCache(self, b, longest + max_new_tokens + k)
        logits = self.prefill(idx, cache, lengths=lens)
        pending = ops.sample_logits(logits, None if greedy else torch.rand(b, device=dev, generator=generator), temperature, top_k, top_p)
        # the device's account: every row's tokens so far, the pending one last
        start = torch.tensor(lens, dtype=torch.int64, device=dev).unsqueeze(1)
        hist = torch.zeros((b, width), dtype=torch.int64, device=dev)
        hist[:, :longest] = idx
        hist.scatter_(1, start, pending.unsqueeze(1))
        hlen = (start.squeeze(1) + 1).to(torch.int32)
        # the host's account: where the rows stand in the cache (-1: parked) and how many tokens each has emitted
        at = list(lens)
        counts = [1] * b
        first = pending.tolist() if eos_token is not None else None
        done = [max_new_tokens == 1 or (first is not None and first[r] == eos_token) for r in range(b)]
        newly = list(done)
        col = torch.arange(k + 1, device=dev).view(1, -1)
        while not all(done):
            if any(newly):                                              # park what the last round finished: it stores and reads nothing
                cache.park(torch.tensor(newly, device=dev))
                at = [-1 if d else p for p, d in zip(at, done)]
            us = None
            if not greedy:
                r = torch.rand(b * (k + 1), device=dev, generator=generator)
                us = r[:b * k].view(b, k), r[b * k:]
            x, n_accept, token, match_len = self.lookup_and_verify(pending, cache, hist, hlen, k, us, temperature, top_k, top_p, ngram)
            a_dev = n_accept.long().unsqueeze(1)
            emitted = torch.cat([x, token.unsqueeze(1)], dim=1).scatter(1, a_dev, token.unsqueeze(1))   # x_0 .. x_{a-1}, token, (stale)
            hist.scatter_(1, hlen.long().unsqueeze(1) + col, emitted)   # behind the row's length: at most column width - 2
            if eos_token is None:
                eos_at = torch.full((b,), k + 1, device=dev)
            else:
                hit = (emitted == eos_token) & (col <= a_dev)
                eos_at = torch.where(hit.any(dim=1), hit.to(torch.uint8).argmax(dim=1), torch.full((b,), k + 1, device=dev))
            read = torch.stack([a_dev.squeeze(1), eos_at, match_len.long()], dim=1).tolist()   # the round's host synchronisation
            stats["rounds"] += 1
            back, now, newly, grow = [0] * b, [p + k + 1 if p >= 0 else -1 for p in at], [False] * b, [0] * b
            for r in range(b):
                if done[r]:
                    continue
                a, e, m = read[r]
                n = min(a + 1, e + 1, max_new_tokens - counts[r])       # tokens of this round that count
                stats["drafted"] += k
                stats["accepted"] += a
                stats["matched"] += m > 0
                counts[r] += n
                grow[r] = n
                back[r] = k + 1 - n                                     # the pending token and the first n - 1 of this round's stay
                newly[r] = done[r] = counts[r] >= max_new_tokens or e < n
            cache.rewind_rows(back, now)
            at = [p - n if p >= 0 else -1 for p, n in zip(now, back)]
            hlen += torch.tensor(grow, dtype=torch.int32, device=dev)
            pending = token
        steps = max_new_tokens if lengths is None else max(counts)
        fill = eos_token if lengths is None and eos_token is not None else pad
        tokens = hist.gather(1, start + torch.arange(steps, device=dev).view(1, -1))    # row b's counts[b] tokens lie behind its prompt
        tokens = torch.where(_live(torch.tensor(counts, device=dev), steps, dev), tokens, torch.full((), int(fill), dtype=torch.int64, device=dev))
        return result(tokens, counts)


def next_token_loss(logits, idx):
    """Mean cross entropy of position t's logits against token t + 1 over every row's first T - 1 positions — the loss of an
    autoregressive model on its own input (ops.next_token_loss: obte_masked_ce_rows with a row list).  Differentiable."""
    return ops.next_token_loss(logits, idx)
