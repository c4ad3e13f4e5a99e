"""Data-parallel masked-LM training harness: the counterpart of the reference's ``training/train_encoder.py``
for the MI355X path (one process per GPU under torchrun, DDP over RCCL).

Kept from the reference (file:line = training/train_encoder.py):
  * flags --batch_size / --mini_batch_size / --n_head / --n_embd / --n_layer / --ctx_len / --dropout / --lr / betas /
    --epsilon / --weight_decay / --token_budget / --disable_flash / --force_lr / --checkpoint_freq / --use_padding /
    --batch_ramp / --warmup_period (:438-467), global batch split evenly over ranks (:115-118);
  * model + muP set-up: target, base (n_embd 24 / n_head 3) and delta (48 / 12) models, set_base_shapes, bf16 (:145-170);
  * lr = args.lr * sqrt(batch_size) / 32, MuAdamW (or AdamW with --force_lr), LinearLR 1 -> 0 (:195-201);
  * MLM corruption with the host NumPy RNG, 15 %, every selected token -> MASK (:273-279);
  * gradient accumulation over rows/mini_batch_size micro-batches with loss / n_accum, masked-only CE averaged over
    the masked tokens of the micro-batch (:284-305); clip_grad_norm_(1.0), optimizer, scheduler (:316-318);
  * tokens/s = non-PAD tokens of all ranks / wall time, MFU formula 6N + 12 L C T (:350-364).
Changed on purpose (same mathematics, MI355X-first mechanics):
  * the attention mask travels as per-query key ranges built on the device (masks.RangeMask) instead of a dense
    (B, H, T, T) tensor built by a Python loop behind a nonzero() host sync (:290-292);
  * gradients are all-reduced once per optimizer step — DDP ``no_sync()`` on all but the last micro-batch — instead
    of after every micro-batch (the reference never calls no_sync, :284-311); averaging already-averaged sums is
    idempotent, so the result is the same while 1/n_accum of the bytes cross xGMI, in buckets that overlap with the
    last micro-batch's backward;
  * loss: fused CE forward+backward kernel (one pass over the logits); the per-step scalars (loss, token count) are
    reduced with one small device all-reduce instead of two pickled gloo all_gather_object calls (:335,354);
  * clip + AdamW run as fused kernels without a host sync (the clip coefficient stays on the device).
Added beyond the reference, off by default: ``--master_weights`` — fp32 master weights and fp32 moments behind the bf16 parameters
(FusedAdamW(master_weights=True)); the masters travel inside the optimizer checkpoint and ``--resume_from`` restores them;
``--fp32_grad_accum`` — every weight gradient summed over the micro-batches of a step in fp32 and rounded to bf16 once
(TrainStep(grad_accum="fp32")) instead of after every micro-batch, as autograd's ``grad += new`` does (:284-311).
``--objective clm`` — the next-token objective for autoregressive models (TrainStep(objective="clm"): the batch itself under the
document-causal mask, the row-compact readout over next_token_rows' positions, the reference's per-micro-batch normalisation carried
over) and ``--distill_from`` — the same step against a teacher's logits (ops.distill_ce_rows: one kernel for alpha * CE +
(1 - alpha) * T^2 * KL and its gradient), the loss a speculative-decoding draft is trained with.
Data: with ``--base_dir`` pointing at the reference's directory layout (``genbank/train``, ``uniref100/train`` ... of
``.npy`` token shards, train_encoder.py:70-99) batches come from ``omnibiote_amd.loader`` (same packing and mixing as the
reference loader, loader thread + bounded queue, pinned-memory copies on their own stream); otherwise from synthetic rows
of the same contract.  Checkpoints follow the reference's convention (whole-object model pickle every
``--save_freq`` tokens, previous one removed, train_encoder.py:412-423); optimizer and scheduler are saved as state_dicts.
wandb logging is replaced by one line per step on rank 0.
"""
from __future__ import annotations

import argparse
import contextlib
import math
import os
import time
from collections import namedtuple
from types import SimpleNamespace
from typing import Callable, Dict, Iterable, List, Optional

import numpy as np
import torch
import torch.distributed as dist
import torch.nn.functional as F

EOS_TOKEN, MASK_TOKEN, PAD_TOKEN = 3, 2, 1   # training/loader.py:4-6
DNA_TAG, PROTEIN_TAG = 4, 18                   # tokenizer ids
BANNED_MIXED = 65533                           # train_encoder.py:62-67


# ----------------------------------------------------------------------------------------------- synthetic data
def synthetic_rows(rows: int, ctx_len: int, vocab: int, rng: np.random.Generator, single_document: bool = True,
                   nucleotide_fraction: float = 0.8) -> np.ndarray:
    """int64 (rows, ctx_len) in the packed, un-padded format get_sequence(..., USE_PADDING=False) yields
    (loader.py:118-163): documents ``tag, body..., EOS`` concatenated and truncated at ctx_len; 80 % of the rows
    nucleotide (tag 4), 20 % peptide (tag 18) as the 'mixed' split (train_encoder.py:82-86); body ids uniform over
    [20, vocab) minus the banned id.  single_document=True makes every row one document longer than ctx_len (no
    interior EOS -> full attention), the variant the FLOP formula assumes."""
    out = np.empty((rows, ctx_len), dtype=np.int64)
    hi = min(vocab, 65536)
    for r in range(rows):
        nucleotide = rng.random() < nucleotide_fraction
        tag = DNA_TAG if nucleotide else PROTEIN_TAG
        pos = 0
        while pos < ctx_len:
            if single_document:
                n = ctx_len
            else:
                lo_len, hi_len = (256, 8192) if nucleotide else (32, 512)
                n = int(math.exp(rng.uniform(math.log(lo_len), math.log(hi_len))))
            doc = rng.integers(20, hi, size=n + 2)
            doc[doc == BANNED_MIXED] = 20
            doc[0] = tag
            doc[-1] = EOS_TOKEN
            take = min(len(doc), ctx_len - pos)
            out[r, pos:pos + take] = doc[:take]
            pos += take
    rng.shuffle(out, axis=0)   # loader.py:176
    return out


def mlm_corrupt(input_ids: torch.Tensor, mask_prob: float = 0.15):
    """train_encoder.py:273-279: host NumPy Bernoulli, minus PAD and EOS positions, all selected -> MASK_TOKEN."""
    draw = np.random.binomial(1, mask_prob, tuple(input_ids.shape))
    mask = torch.as_tensor(draw, dtype=torch.bool, device=input_ids.device)
    mask = mask & (input_ids != PAD_TOKEN) & (input_ids != EOS_TOKEN)
    return input_ids.masked_fill(mask, MASK_TOKEN), mask


def _next_token_scored(ids):
    """The positions a next-token objective scores, as a bool (rows, T) of ``ids``'s kind (a numpy array or a tensor): (b, t) with
    t + 1 < T, ids[b, t] neither EOS (the pair "end of one document -> first token of the next" is no label pair) nor PAD, and
    ids[b, t + 1] not PAD."""
    scored = torch.zeros(ids.shape, dtype=torch.bool, device=ids.device) if torch.is_tensor(ids) else np.zeros(ids.shape, dtype=bool)
    scored[:, :-1] = (ids[:, :-1] != EOS_TOKEN) & (ids[:, :-1] != PAD_TOKEN) & (ids[:, 1:] != PAD_TOKEN)
    return scored


def next_token_rows(ids_host, mini: int, n_accum: int):
    """Which positions the causal-LM objective scores, from the host copy of the batch (numpy only, no device round trip):
    ``(rows, labels)``, each a list of n_accum int64 arrays — per micro-batch of ``mini`` rows the ascending flat positions b T + t
    (b counted within the micro-batch) that are scored (_next_token_scored) and, in the same order, their labels ids[b, t + 1].  EOS IS a
    label, at a document's last real token, so that stopping at ``eos_token`` is learnt."""
    ids = np.asarray(ids_host)[:mini * n_accum]
    if ids.ndim != 2 or ids.shape[0] != mini * n_accum:
        raise ValueError(f"next_token_rows: a (rows, T) batch of at least mini * n_accum = {mini * n_accum} rows is needed, got shape {np.shape(ids_host)}")
    per = _next_token_scored(ids).reshape(n_accum, -1)
    nxt = np.roll(ids, -1, axis=1).reshape(n_accum, -1)     # (the wrapped last column is never scored)
    rows = [np.flatnonzero(per[j]).astype(np.int64) for j in range(n_accum)]
    return rows, [nxt[j][rows[j]].astype(np.int64) for j in range(n_accum)]


def next_token_rows_device(input_ids: torch.Tensor, mini: int, n_accum: int):
    """next_token_rows without a host copy of the batch: the same integers from tensor ops and ONE blocking device-to-host copy (of the
    bool table); lists of int64 tensors on ``input_ids``'s device."""
    ids = input_ids[:mini * n_accum]
    scored = _next_token_scored(ids).reshape(n_accum, -1)
    nxt = torch.roll(ids, shifts=-1, dims=1).reshape(n_accum, -1)
    sh = scored.cpu()
    rows = [torch.nonzero(sh[j], as_tuple=False).reshape(-1).to(ids.device) for j in range(n_accum)]
    return rows, [nxt[j].index_select(0, rows[j]) for j in range(n_accum)]


# ---------------------------------------------------------------------------------------------------- optimizer
class FusedAdamW(torch.optim.Optimizer):
    """AdamW over bf16 parameters with bf16 moments (the reference's pure-bf16 regime) on the fused HIP kernels.
    ``step(max_norm=...)`` also applies clip_grad_norm_ semantics (train_encoder.py:316) without a host sync: the
    squared norm is accumulated on the device and the coefficient min(1, max_norm/(norm+1e-6)) is consumed by the
    update kernel directly.

    ``master_weights=True`` (off by default; NOT the reference's regime, which keeps no fp32 state): the optimizer owns an fp32
    master copy of every weight and fp32 moments, runs torch.optim.AdamW's fp32 arithmetic on them (obte_adamw_multi_master) and
    writes ``p = bf16(master)`` each step, so updates smaller than half a bf16 step of the weight are kept instead of rounded
    away.  The parameters stay bf16: the model, DDP and the checkpoints see what they see without it."""

    _MASTER_KEYS = ("master", "exp_avg", "exp_avg_sq")

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, rounding: str = "reference",
                 master_weights: bool = False):
        """rounding="reference" (default): every tensor op of torch.optim.AdamW's bf16 update is rounded to bf16 exactly
        where the reference's optimizer rounds it (obte_adamw_multi_bf16_ref), so trajectories track the reference's;
        "single": fp32 arithmetic per element with one rounding per state (more accurate, not the reference's numbers).
        master_weights=True has one arithmetic of its own: rounding must then be left at its default."""
        assert rounding in ("reference", "single")
        if master_weights and rounding != "reference":
            raise ValueError("FusedAdamW(master_weights=True) has one arithmetic (torch.optim.AdamW on fp32 state): "
                             f"leave rounding at its default (got rounding={rounding!r})")
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay))
        self.rounding = rounding
        self.master_weights = bool(master_weights)
        self._norm_sq = None
        self._partials = None        # master mode: one fp32 partial sum of squares per workgroup, and [norm_sq, coefficient]
        self._clip_out = None
        self._seen_version = {}      # master mode: each parameter's _version as the last step (or load_state_dict) left it
        self._warned_foreign = False

    # ---- fp32 state through state_dict() / load_state_dict() -----------------------------------------------------------------
    def load_state_dict(self, state_dict):
        """torch.optim.Optimizer.load_state_dict casts every floating-point state tensor to the PARAMETER's dtype, which would
        round the fp32 masters and moments to bf16.  In master mode they are taken from the given state dict as they are (fp32,
        bit for bit).  A state dict written by the bf16 modes is converted with a warning: moments upcast exactly, masters
        seeded from the live parameters.  A master-mode state dict is refused by a bf16-mode optimizer (it would drop the
        masters silently).  The parameters' versions are recorded as they are NOW, so load the model first, as run() does."""
        import warnings
        from itertools import chain
        saved = state_dict["state"]
        has_master = any(isinstance(v, dict) and "master" in v for v in saved.values())
        if not self.master_weights:
            if has_master:
                raise ValueError("this optimizer state was written with master_weights=True (fp32 master weights and moments); "
                                 "loading it into FusedAdamW(master_weights=False) would drop the masters: build the optimizer "
                                 "with master_weights=True (--master_weights)")
            return super().load_state_dict(state_dict)
        super().load_state_dict(state_dict)   # validates the groups, restores their hyper-parameters and every step count
        saved_ids = chain.from_iterable(g["params"] for g in state_dict["param_groups"])
        params = chain.from_iterable(g["params"] for g in self.param_groups)
        converted = 0
        self._seen_version = {}
        for k, p in zip(saved_ids, params):
            src = saved.get(k)
            if not src:
                continue
            st = self.state[p]
            for key in ("exp_avg", "exp_avg_sq"):
                st[key] = src[key].to(device=p.device, dtype=torch.float32, copy=True)
            if "master" in src:
                st["master"] = src["master"].to(device=p.device, dtype=torch.float32, copy=True)
            else:
                st["master"] = p.detach().float()
                converted += 1
            self._seen_version[p] = p._version
        if converted:
            warnings.warn(f"FusedAdamW(master_weights=True): the loaded optimizer state holds no master weights (written by a "
                          f"bf16 mode): {converted} masters seeded from the current bf16 parameters, moments upcast to fp32")

    def reseed_masters(self, params=None):
        """Take the masters of `params` (default: all) from the bf16 parameters as they are now.  For writes that torch's version
        counter does not see (``p.data.copy_(...)``, a kernel writing through a raw pointer): writes through torch proper
        (``p.copy_`` under no_grad, ``model.load_state_dict``) are noticed by step() itself."""
        for p in (params if params is not None else [p for g in self.param_groups for p in g["params"]]):
            st = self.state.get(p)
            if st and "master" in st:
                st["master"].copy_(p.detach())
                self._seen_version[p] = p._version

    def _step_master(self, max_norm, clip_coef):
        import ctypes as C
        import warnings
        from . import _lib as L
        lib = L.lib()
        stream = torch.cuda.current_stream().cuda_stream
        batches, stepped, foreign = [], [], 0   # (MtMasterArgs, MtArgs, betas, eps)
        for group in self.param_groups:
            ps = [p for p in group["params"] if p.grad is not None]
            lr, wd = float(group["lr"]), float(group["weight_decay"])
            for i in range(0, len(ps), L.MT_MAX):
                chunk = ps[i:i + L.MT_MAX]
                a, ga = L.MtMasterArgs(), L.MtArgs()
                a.count = ga.count = len(chunk)
                for j, p in enumerate(chunk):
                    if p.dtype != torch.bfloat16 or p.numel() % 8 or not p.is_cuda:
                        raise RuntimeError("FusedAdamW needs bf16 GPU parameters with numel % 8 == 0")
                    st = self.state[p]
                    if not st:
                        st["step"] = 0
                        st["master"] = p.detach().float()
                        st["exp_avg"] = torch.zeros_like(p, dtype=torch.float32)
                        st["exp_avg_sq"] = torch.zeros_like(p, dtype=torch.float32)
                    elif self._seen_version.get(p) != p._version:
                        # the kernel writes p through a raw pointer, which does not count as a version: a different one means
                        # torch wrote the parameter (model.load_state_dict, a manual copy_) and the master no longer stands for it
                        st["master"].copy_(p.detach())
                        foreign += 1
                    st["step"] += 1
                    a.p[j], a.g[j] = p.data_ptr(), p.grad.data_ptr()
                    a.master[j], a.m[j], a.v[j] = st["master"].data_ptr(), st["exp_avg"].data_ptr(), st["exp_avg_sq"].data_ptr()
                    a.n[j], a.lr[j], a.weight_decay[j], a.step[j] = p.numel(), lr, wd, st["step"]
                    ga.g[j], ga.n[j] = a.g[j], a.n[j]
                stepped.extend(chunk)
                batches.append((a, ga, group["betas"], group["eps"]))
        if foreign and not self._warned_foreign:
            self._warned_foreign = True
            warnings.warn(f"FusedAdamW(master_weights=True): {foreign} parameters were written outside the optimizer since its last "
                          "step; their fp32 masters were re-seeded from the bf16 parameters (this warning is given once)")
        if not batches:
            return None
        clip_ptr, norm_sq = None, None
        if max_norm is not None:
            # the fixed-order norm: one partial per workgroup, every launch its own stretch, one small kernel adds them in index
            # order and forms the coefficient on the device (no atomics: two runs and two replicas get the same bits)
            dev = torch.device("cuda", torch.cuda.current_device())
            counts = [int(lib.obte_sumsq_multi_partials_count(C.byref(ga))) for _, ga, _, _ in batches]
            if min(counts) < 0:
                L.check(min(counts), "obte_sumsq_multi_partials_count")
            total = sum(counts)
            if self._partials is None or self._partials.device != dev or self._partials.numel() < total:
                self._partials = torch.empty(total, dtype=torch.float32, device=dev)
            if self._clip_out is None or self._clip_out.device != dev:
                self._clip_out = torch.empty(2, dtype=torch.float32, device=dev)
            off = 0
            for (_, ga, _, _), c in zip(batches, counts):
                L.check(lib.obte_sumsq_multi_bf16_partials(C.byref(ga), self._partials.data_ptr() + 4 * off, stream), "obte_sumsq_multi_bf16_partials")
                off += c
            L.check(lib.obte_clip_coef_from_partials(self._partials.data_ptr(), total, float(max_norm), self._clip_out.data_ptr(), stream),
                    "obte_clip_coef_from_partials")
            clip_ptr = self._clip_out.data_ptr() + 4
        elif clip_coef is not None:
            if clip_coef.dtype != torch.float32 or not clip_coef.is_cuda or clip_coef.numel() != 1:
                raise ValueError("clip_coef must be one fp32 element on the GPU")
            clip_ptr = clip_coef.data_ptr()
        for a, _, (b1, b2), eps in batches:
            L.check(lib.obte_adamw_multi_master(C.byref(a), b1, b2, eps, clip_ptr, stream), "obte_adamw_multi_master")
        for p in stepped:
            self._seen_version[p] = p._version
        return None if max_norm is None else self._clip_out[0].clone()

    @torch.no_grad()
    def step(self, max_norm: Optional[float] = None, clip_coef: Optional[torch.Tensor] = None):
        """Multi-tensor launches: <= 32 tensors per kernel (per parameter group, since betas/eps are per group).
        clip_coef (master mode only, instead of max_norm): one fp32 element on the device that the update kernel multiplies
        every gradient by — a coefficient the caller formed."""
        if clip_coef is not None and (max_norm is not None or not self.master_weights):
            raise ValueError("clip_coef is for master_weights=True and replaces max_norm")
        if self.master_weights:
            return self._step_master(max_norm, clip_coef)
        import ctypes as C
        from . import _lib as L
        from . import ops
        lib = L.lib()
        stream = torch.cuda.current_stream().cuda_stream
        batches = []   # (MtArgs, betas, eps)
        for group in self.param_groups:
            ps = [p for p in group["params"] if p.grad is not None]
            for i in range(0, len(ps), L.MT_MAX):
                chunk = ps[i:i + L.MT_MAX]
                a = L.MtArgs()
                a.count = len(chunk)
                for j, p in enumerate(chunk):
                    st = self.state[p]
                    if not st:
                        st["step"] = 0
                        st["exp_avg"] = torch.zeros_like(p)
                        st["exp_avg_sq"] = torch.zeros_like(p)
                    st["step"] += 1
                    if p.dtype != torch.bfloat16 or p.numel() % 8 or not p.is_cuda:
                        raise RuntimeError("FusedAdamW needs bf16 GPU parameters with numel % 8 == 0")
                    a.p[j], a.g[j], a.m[j], a.v[j] = p.data_ptr(), p.grad.data_ptr(), st["exp_avg"].data_ptr(), st["exp_avg_sq"].data_ptr()
                    a.n[j], a.lr[j], a.weight_decay[j], a.step[j] = p.numel(), float(group["lr"]), float(group["weight_decay"]), st["step"]
                    a.lr64[j], a.weight_decay64[j] = float(group["lr"]), float(group["weight_decay"])   # un-rounded, for the _ref kernel's double-formed scalars
                batches.append((a, group["betas"], group["eps"]))
        if not batches:
            return None
        clip = None
        if max_norm is not None and self.rounding == "reference":
            # clip_grad_norm_ on bf16 gradients (train_encoder.py:316): per-tensor norms rounded to bf16, their 2-norm
            # rounded to bf16, the coefficient max_norm / (total + 1e-6) formed and clamped in bf16
            dev = torch.device("cuda", torch.cuda.current_device())
            n_tensors = sum(a.count for a, _, _ in batches)
            if self._norm_sq is None or self._norm_sq.device != dev or self._norm_sq.numel() != n_tensors:
                self._norm_sq = torch.zeros(n_tensors, dtype=torch.float32, device=dev)
            self._norm_sq.zero_()
            off = 0
            for a, _, _ in batches:
                L.check(lib.obte_sumsq_multi_bf16_each(C.byref(a), self._norm_sq.data_ptr() + 4 * off, stream), "obte_sumsq_multi_bf16_each")
                off += a.count
            total = torch.linalg.vector_norm(self._norm_sq.sqrt().to(torch.bfloat16))
            clip = torch.clamp(max_norm / (total + 1e-6), max=1.0).float().reshape(1)
        elif max_norm is not None:
            dev = torch.device("cuda", torch.cuda.current_device())
            if self._norm_sq is None or self._norm_sq.device != dev or self._norm_sq.numel() != 1:
                self._norm_sq = torch.zeros(1, dtype=torch.float32, device=dev)
            self._norm_sq.zero_()
            for a, _, _ in batches:
                L.check(lib.obte_sumsq_multi_bf16(C.byref(a), self._norm_sq.data_ptr(), stream), "obte_sumsq_multi_bf16")
            clip = torch.clamp(max_norm / (self._norm_sq.sqrt() + 1e-6), max=1.0)
        fn = lib.obte_adamw_multi_bf16_ref if self.rounding == "reference" else lib.obte_adamw_multi_bf16
        for a, (b1, b2), eps in batches:
            L.check(fn(C.byref(a), b1, b2, eps, None if clip is None else clip.data_ptr(), stream), "obte_adamw_multi_bf16")
        return None if clip is None else self._norm_sq.sum()


# --------------------------------------------------------------------------------------------------- train step
# What one TrainStep call does, resolved once at its top (resolve_step_plan) from the object's public attributes AS THEY ARE AT THAT
# CALL — callers reassign them on a live object between steps — and the call's own facts; plain Python values only.  rows: of the
# batch, a multiple of the micro-batch; n_accum micro-batches in n_pass passes of k micro-batches (span rows) each; sparse_rows: one
# of the two row-compact readouts (`readout`; they need the HIP kernels); fp32_sum: every weight gradient summed in fp32 over the
# passes; ns: streams in flight; has_reducer: the model is DDP-wrapped (no_sync); layer_order: side passes order their backward per
# parameter group (model.BackwardOrder); bf16 path: inplace — a gradient policy is entered at all, ln_partials — LayerNorm weight
# gradients as fp32 partial sums from pass 1 on; emb_sort: one segmented id sort per step for the embedding backward.
StepPlan = namedtuple("StepPlan", "rows n_accum sparse_rows readout rows_forward mask_impl k n_pass span fp32_sum pipelined ns has_reducer "
                                  "layer_order sync_every inplace ln_partials emb_sort")
# Pass j of a plan (pass_record).  isolate_last: the last pass of a DDP-wrapped model, on the caller's stream after everything, else
# `side`: on side stream `slot`; ordered: a BackwardOrder is attached; join_side: its backward waits for every side stream instead of
# the previous backward; delivery: the arguments (accumulate, ln_mode, acc32_mode) of model.accumulate_grads_inplace, or None — no
# policy entered (autograd's own `grad += new`).
PassRecord = namedtuple("PassRecord", "j last isolate_last side slot no_sync ordered join_side delivery")
# The corrupted batch of one step; rows / targets: per micro-batch, the masked positions and (host prelude only) their labels, or None
# labels (objective="clm" only): the batch shifted left by one, what the dense readout's CE indexes by position; None: the batch itself
_Batch = namedtuple("_Batch", "masked_ids mask rows targets labels", defaults=(None,))


def resolve_step_plan(s, rows: int, on_gpu: bool, has_reducer: bool, has_transformer: bool, env=os.environ) -> StepPlan:
    """s: a TrainStep, or anything with its public attributes.  env: the two A/B switches are read here, once per call.
    OBTE_NO_INPLACE_ACCUM=1: every gradient is delivered through autograd's AccumulateGrad (`grad += new`, issued by the engine AFTER
    a node's backward returned), so no per-group event a node records can cover it: pipelined passes are then ordered as wholes.
    OBTE_NO_LN_PARTIALS=1: no fp32 LayerNorm partial sums."""
    stub = s.fused_loss_fn is not None          # a stub model / torch loss (CPU tests) takes the generic graph
    no_inplace = env.get("OBTE_NO_INPLACE_ACCUM") == "1"
    fused = s.loss_impl == "fused"
    rows = rows // s.mini * s.mini
    n_accum = rows // s.mini
    sparse_rows = s.lm_head_impl in ("dense", "masked") and fused and not stub
    # objective="clm" (read with a default: callers hand any object with the older attributes) runs on the row-compact readout alone, so
    # its plan is the MLM plan of the same settings; the attributes may have been reassigned on a live object since the constructor checked
    if getattr(s, "objective", "mlm") == "clm" and not sparse_rows:
        raise ValueError('TrainStep(objective="clm") needs lm_head_impl "masked" or "dense", loss_impl="fused" and no fused_loss_fn; got '
                         f"lm_head_impl={s.lm_head_impl!r}, loss_impl={s.loss_impl!r}, fused_loss_fn {'set' if stub else 'None'}")
    k = s.per_pass if (sparse_rows and n_accum % s.per_pass == 0) else 1
    n_pass = n_accum // k
    pipelined = s.pipeline_streams >= 2 and on_gpu and fused and n_pass > 2 and not s.sync_every
    return StepPlan(rows=rows, n_accum=n_accum, sparse_rows=sparse_rows, readout=s.lm_head_impl, rows_forward=s.rows_forward,
                    mask_impl=s.mask_impl, k=k, n_pass=n_pass, span=k * s.mini,
                    fp32_sum=s.grad_accum == "fp32" and n_pass >= 2,   # (a single pass: the plain path, its gradient is rounded once anyway)
                    pipelined=pipelined, ns=s.pipeline_streams if pipelined else 1, has_reducer=has_reducer,
                    layer_order=s.backward_order == "layer" and not stub and not no_inplace, sync_every=bool(s.sync_every),
                    inplace=fused and not no_inplace,
                    ln_partials=n_pass > 2 and not s.sync_every and not stub and env.get("OBTE_NO_LN_PARTIALS") != "1",
                    emb_sort=on_gpu and fused and not stub and has_transformer)


def pass_record(plan: StepPlan, j: int) -> PassRecord:
    """Pass j of the plan; the ONE place that decides how a pass delivers its gradients.
    bf16 path: all but the last pass of a DDP-wrapped model accumulate in place — nobody observes the per-micro-batch gradients,
    so the wgrad epilogues add into param.grad themselves (the last pass too when no reducer is attached: nothing observes its
    gradients before the optimizer does).  LayerNorm weights: pass 0 delivers through autograd (there is no .grad yet), 1 .. n-2
    carry fp32 partial sums (first / more), the last folds them in and delivers the total through autograd.
    fp32 sum: every weight gradient, the LayerNorm weights included, from pass 0 on — first / more / last."""
    from . import _lib as L
    last = j == plan.n_pass - 1
    isolate_last = last and plan.has_reducer
    side = plan.pipelined and not isolate_last
    if plan.fp32_sum:
        ln_mode, acc32_mode = ((L.LN_PARTIAL_FIRST, L.ACC32_FIRST) if j == 0 else
                               (L.LN_PARTIAL_LAST, L.ACC32_LAST) if last else (L.LN_PARTIAL_MORE, L.ACC32_MORE))
        delivery = (False, ln_mode, acc32_mode)
    elif not plan.inplace:
        delivery = None
    else:
        ln_mode = 0
        if plan.ln_partials and j >= 1:
            ln_mode = L.LN_PARTIAL_FIRST if j == 1 else (L.LN_PARTIAL_LAST if last else L.LN_PARTIAL_MORE)
        delivery = (not isolate_last and not plan.sync_every, ln_mode, 0)
    return PassRecord(j=j, last=last, isolate_last=isolate_last, side=side, slot=(j % plan.ns) if side else 0,
                      no_sync=plan.has_reducer and not last and not plan.sync_every, ordered=side and plan.layer_order,
                      join_side=plan.pipelined and isolate_last, delivery=delivery)


def _pass_rows(batch: _Batch, j: int, k: int, rows_per_mb: int):
    """Masked positions of pass j (micro-batches j*k .. j*k + k-1) as row indices into the pass's k * mini rows; for k > 1 the
    weight 1 / (masked tokens of its own micro-batch) of each; their labels in the same order when the host prelude shipped them."""
    lists = batch.rows[j * k:(j + 1) * k]
    tgts = batch.targets[j * k:(j + 1) * k] if batch.targets is not None else None
    keep = [i for i, r in enumerate(lists) if r.numel() > 0]
    if k == 1 or not keep:
        return lists[0], None, None if tgts is None else tgts[0]
    rows = torch.cat([lists[i] + i * rows_per_mb for i in keep])
    w = torch.cat([torch.full((lists[i].numel(),), 1.0 / lists[i].numel(), dtype=torch.float32, device=rows.device) for i in keep])
    return rows, w, None if tgts is None else torch.cat([tgts[i] for i in keep])


class TrainStep:
    """One optimizer step of train_encoder.py:241-323 over a (rows, ctx_len) batch of this rank's rows."""
    _warned_no_host_copy = False

    def __init__(self, model, optimizer, scheduler=None, *, mini_batch_size: int, n_head: int, use_padding: bool = False,
                 loss_impl: str = "fused", mask_impl: str = "ranges", sync_every_micro_step: bool = False,
                 max_grad_norm: float = 1.0, lm_head_impl: str = "masked", pipeline_streams: int = 1,
                 fused_loss_fn: Optional[Callable] = None, micro_batches_per_pass: int = 1, backward_order: str = "layer",
                 rows_forward: bool = True, grad_accum: str = "bf16", objective: str = "mlm", teacher=None, distill_alpha: float = 0.5,
                 distill_temperature: float = 1.0):
        """objective: "mlm" (default) — the reference's masked-LM step; "clm" — the next-token objective of an autoregressive model
        (config.autoregressive): no corruption, the document-causal mask, and the row-compact readout over the positions
        next_token_rows lists, every one weighted 1 / (n_accum * scored positions of its own micro-batch).  teacher (clm only): an
        autoregressive OmniBioTA with the student's vocabulary, any depth and width; put in eval(), run under no_grad on the listed
        rows, and the loss becomes distill_alpha * CE + (1 - distill_alpha) * distill_temperature^2 * KL(teacher || student) at that
        temperature (ops.distill_ce_rows); the result dict then also carries "ce" and "kl", normalised like "loss".
        grad_accum: "bf16" (default) — the reference's arithmetic: every micro-batch's weight gradient is rounded to bf16 and
        added to a bf16 running sum (autograd's ``grad += new``; here the wgrad epilogues do it in place).  "fp32" (beyond the
        reference, --fp32_grad_accum): over the passes of a step every weight gradient is summed in a persistent fp32 buffer of
        the weight's shape (model.Fp32GradStore, owned by this object: +4 bytes per parameter) from the contributions BEFORE
        their rounding to bf16 — pass 0 stores, the middle passes add, the last adds and hands bf16(sum) to autograd.
        ``param.grad`` is None until then; the optimizer, clipping, DDP buckets and checkpoints see bf16 gradients rounded once.
        A step of a single pass runs the plain path.  Refused (ValueError, never a silent bf16 sum) with sync_every_micro_step,
        OBTE_NO_INPLACE_ACCUM=1 / OBTE_NO_LN_PARTIALS=1, a stub or torch loss and activation checkpointing.
        fused_loss_fn: ``(logits, targets, mlm_mask, n_accum) -> (loss, dlogits)`` used by loss_impl="fused" instead of
        the HIP kernel (ops.masked_ce) — lets the CPU multi-process tests drive the product scheduling (in-place
        accumulation, no_sync, hand-delivered d(logits)) with a stub model and a torch loss."""
        self.fused_loss_fn = fused_loss_fn
        if objective not in ("mlm", "clm"):
            raise ValueError(f'objective must be "mlm" or "clm", got {objective!r}')
        self.objective = objective
        self.teacher, self.distill_alpha, self.distill_temperature = teacher, float(distill_alpha), float(distill_temperature)
        # micro_batches_per_pass = k > 1 (the two row-compact readout paths): k consecutive micro-batches go through the model in ONE
        # forward/backward of k * mini_batch_size rows.  Rows never interact across a batch (attention is per row, the mask
        # builder's per-micro-batch quirk is kept), and the loss keeps the reference's normalisation — every masked row is
        # weighted 1 / (n_accum * masked tokens of ITS micro-batch), train_encoder.py:301-305 — so loss and gradients are those
        # of k separate passes up to summation order; every kernel simply sees k times the rows per launch.  An execution
        # option like pipeline_streams, off by default: --mini_batch_size keeps its meaning either way.
        self.per_pass = max(1, int(micro_batches_per_pass))
        self.model, self.optimizer, self.scheduler = model, optimizer, scheduler
        self.mini, self.n_head, self.use_padding = mini_batch_size, n_head, use_padding
        self.loss_impl, self.mask_impl = loss_impl, mask_impl
        self.sync_every = sync_every_micro_step
        self.max_grad_norm = max_grad_norm
        # "masked" (default): the loss multiplies the unmasked ~85 % of the positions by zero
        #     (train_encoder.py:304), so the readout (model.py:253, reached through forward(return_embeddings=True)) and the
        #     cross entropy run on the MLM-masked positions alone: logits [n_masked, V] instead of [B*T, V], CE over those rows
        #     (ops.masked_ce_rows), the two backward products over those rows (model._ReadoutRowsGradFn).  Same loss, same
        #     gradients — the positions left out contribute exact zeros — for 1/6.7 of the lm_head work.
        # "dense": the forward computes the logits of EVERY position, as the reference does (train_encoder.py:296); d(logits)
        #     has exact-zero rows outside the mask, so the readout's backward contracts over the masked rows only.
        # "dense_full": the same forward, and the backward through the dense [M, V] d(logits) tensor — the literal
        #     translation of the reference's graph (logits.backward(dlogits)); kept for A/B and for callers of model(x).
        assert lm_head_impl in ("dense", "dense_full", "masked")
        self.lm_head_impl = lm_head_impl
        # pipeline_streams = 2: micro-batches alternate between two HIP streams so that the forward of micro-batch j+1
        # runs beside the backward of micro-batch j (kernel tails and half-filled grids of one fill with work of the
        # other).  The backward passes stay strictly ordered (an event per micro-batch), so every gradient buffer sees
        # the same read-modify-write sequence as on one stream: results are bitwise those of pipeline_streams = 1.
        assert pipeline_streams in (1, 2, 3)
        self.pipeline_streams = pipeline_streams
        # backward_order (pipeline_streams = 2): "pass" — the backward of micro-batch j+1 starts after the LAST kernel of micro-batch
        # j's backward (one event per pass); "layer" (default) — every parameter group's update waits for the same group's update
        # of the previous micro-batch only (model.BackwardOrder: one event per block / LayerNorm / embedding / readout), so the
        # next backward follows one layer behind and both streams stay busy.  Each gradient buffer sees the same sequence of
        # read-modify-writes either way: bitwise the same results (tested against pipeline_streams = 1).
        assert backward_order in ("layer", "pass")
        self.backward_order = backward_order
        # lm_head_impl="masked": hand the list of masked positions to model.forward(rows=...) so that everything after the last
        # block's attention (its MLP half, ln_f, the readout) is computed for those positions only; False: forward(return_
        # embeddings=True) on every position, rows gathered afterwards (the reference's forward contract to the letter)
        self.rows_forward = bool(rows_forward) and hasattr(self._core, "transformer")
        # caches that outlive a call (nothing that describes a pass does)
        self._streams = None
        self._host_bufs = {}
        self._order_ws = {}
        self._dlogits = {}
        self._ln_store = None
        self._acc32_store = None
        self._mask_rows_host = None   # the last call's per-micro-batch masked-row lists (read by tests)
        self._clm_bufs = {}
        self._check_objective()
        if grad_accum not in ("bf16", "fp32"):
            raise ValueError(f'grad_accum must be "bf16" or "fp32", got {grad_accum!r}')
        self.grad_accum = grad_accum
        if grad_accum == "fp32":
            if sync_every_micro_step:
                raise ValueError('grad_accum="fp32" (--fp32_grad_accum) cannot be combined with sync_every_micro_step=True: the gradient exists '
                                 "only after the last micro-batch, there is nothing to exchange before it")
            if loss_impl != "fused" or fused_loss_fn is not None:
                raise ValueError('grad_accum="fp32" (--fp32_grad_accum) needs the HIP model and loss (loss_impl="fused", no fused_loss_fn): a '
                                 "stub model or a torch loss delivers its gradients through autograd's bf16 `grad += new`")
            if int(getattr(getattr(self._core, "config", None), "checkpoint_freq", 0) or 0) > 0:
                raise ValueError('grad_accum="fp32" (--fp32_grad_accum) cannot be combined with checkpoint_freq > 0: a recomputed block captures '
                                 "its gradient policy on the autograd thread, outside the step's context, and would sum in bf16 unnoticed")
            self._refuse_env_switches()

    @property
    def _core(self):
        """The model itself, out of a DDP wrapper."""
        return self.model.module if hasattr(self.model, "module") else self.model

    def _check_objective(self) -> None:
        """The refusals of objective="clm" and of a teacher: in the constructor and again at the top of every call (the public
        attributes may be reassigned on a live object), before anything is launched."""
        if self.objective != "clm":
            if self.teacher is not None:
                raise ValueError('TrainStep: a teacher needs objective="clm" (distillation is a next-token loss)')
            return
        if self.lm_head_impl == "dense_full":
            raise ValueError('TrainStep(objective="clm"): lm_head_impl="dense_full" is not available (the next-token loss runs on the row-compact '
                             'readout: "masked" or "dense")')
        if self.fused_loss_fn is not None or self.loss_impl != "fused":
            raise ValueError('TrainStep(objective="clm") needs the HIP loss (loss_impl="fused", no fused_loss_fn)')
        if not bool(getattr(getattr(self._core, "config", None), "autoregressive", False)):
            raise ValueError('TrainStep(objective="clm"): the model is not autoregressive (config.autoregressive): a bidirectional model sees the '
                             "token it is asked to predict")
        if self.teacher is not None:
            from .distill import distill_weights
            from .model import OmniBioTA
            t = self.teacher
            if not isinstance(t, OmniBioTA) or not t.config.autoregressive:
                raise ValueError("TrainStep: teacher must be an autoregressive OmniBioTA")
            if t.config.vocab_size != self._core.config.vocab_size:
                raise ValueError(f"TrainStep: the teacher's vocabulary ({t.config.vocab_size}) differs from the student's ({self._core.config.vocab_size})")
            distill_weights(self.distill_alpha, self.distill_temperature)
            t.eval()

    @staticmethod
    def _refuse_env_switches() -> None:
        for var in ("OBTE_NO_INPLACE_ACCUM", "OBTE_NO_LN_PARTIALS"):
            if os.environ.get(var) == "1":
                raise ValueError(f'grad_accum="fp32" (--fp32_grad_accum) cannot be combined with {var}=1: that switch sends gradients through '
                                 "autograd's bf16 `grad += new`")

    def _resolve(self, n_rows: int, on_gpu: bool) -> StepPlan:
        return resolve_step_plan(self, n_rows, on_gpu, hasattr(self.model, "no_sync"), hasattr(self._core, "transformer"))

    def _delivery(self, rec: PassRecord, order):
        """The gradient policy of the pass (pass_record decided it) over this object's own fp32 stores."""
        if rec.delivery is None:   # CPU-oracle tests / A-B switch
            return contextlib.nullcontext()
        from .model import Fp32GradStore, LnPartialStore, accumulate_grads_inplace
        accumulate, ln_mode, acc32_mode = rec.delivery
        if self._ln_store is None:
            self._ln_store = LnPartialStore()     # fp32 LayerNorm partial sums
        if acc32_mode and self._acc32_store is None:
            self._acc32_store = Fp32GradStore()   # fp32 gradient sums
        return accumulate_grads_inplace(accumulate, ln_mode, store=self._ln_store, order=order, acc32_mode=acc32_mode,
                                        acc32_store=self._acc32_store if acc32_mode else None)

    def _token_order_ws(self, segments: int, seg_len: int, vocab: int, dev) -> torch.Tensor:
        """The workspace of ops.token_order: allocated once per shape and reused (every use is on the caller's stream)."""
        key = (segments, seg_len, vocab, dev)
        ws = self._order_ws.get(key)
        if ws is None:
            from . import ops
            if len(self._order_ws) >= 4:           # like _host_bufs: --batch_ramp walks through many row counts
                self._order_ws.pop(next(iter(self._order_ws)))
            ws = self._order_ws[key] = ops.token_order_workspace(segments, seg_len, vocab, dev)
        return ws

    def _embedding_orders(self, plan: StepPlan, masked_ids):
        """The embedding backward sums gradient rows in sorted-token order: ONE segmented sort for all passes of the step instead
        of a radix sort (four launches) per pass.  None: every forward sorts its own ids."""
        if not plan.emb_sort:
            return None
        from . import ops
        seg = masked_ids.reshape(plan.n_pass, -1)
        if not ops.prelude_hip():
            return torch.sort(seg, dim=1, stable=True).indices.to(torch.int32)
        seg = seg.contiguous()
        vocab = self._core.transformer.wte.weight.shape[0]
        return ops.token_order(seg, vocab, ws=self._token_order_ws(plan.n_pass, seg.shape[1], vocab, seg.device))

    def _mask(self, plan: StepPlan, ranges, j: int, dtype):
        """The attention mask of pass j out of the range tables (a masks.RangeMask) built once per optimizer step for every micro-batch."""
        from . import masks
        sl = slice(j * plan.span, (j + 1) * plan.span)
        rm = masks.RangeMask(ranges.key_ranges[sl], None if ranges.query_bounds is None else ranges.query_bounds[sl])
        if plan.mask_impl == "ranges":
            if rm.query_bounds is not None:   # objective="clm": resolved here, so that the model does not take it for a mask without causality
                from . import ops
                B, T, _ = rm.key_ranges.shape
                return ops.MaskSpec.from_user(rm, B, T, self.n_head, rm.key_ranges.device)
            return rm
        return rm.dense(dtype).unsqueeze(1).expand(-1, self.n_head, -1, -1)   # train_encoder.py:292

    def _loss_backward(self, rec: PassRecord, chain, logits, targets, mask, n_accum):
        if self.loss_impl == "fused":
            if self.fused_loss_fn is not None:
                loss, dlogits = self.fused_loss_fn(logits, targets, mask, n_accum)
            else:
                from . import ops
                if rec.slot not in self._dlogits:   # one reusable d(logits) buffer per stream in flight
                    self._dlogits[rec.slot] = ops.DLogitsBuffer()
                loss, dlogits = ops.masked_ce(logits, targets, mask, n_accum, reuse=self._dlogits[rec.slot])
            self._order_backward(rec, chain)
            logits.backward(dlogits)
            return loss.detach()
        # the reference's own three lines (train_encoder.py:301-305)
        loss = F.cross_entropy(logits.view(-1, logits.size(-1)), targets.reshape(-1), reduction="none") / n_accum
        loss *= mask.reshape(-1).float()
        loss = loss.sum() / mask.reshape(-1).sum()
        loss.backward()
        return loss.detach().float()

    def _order_backward(self, rec: PassRecord, chain, whole_pass: bool = False):
        """Pipelined micro-batches: this backward may start only after the previous micro-batch's backward finished.
        whole_pass: wait for the previous backward as a whole even under per-group ordering — for a graph whose gradients
        reach the readout weight through AccumulateGrad instead of a node that carries the BackwardOrder (the zero
        gradients of a pass with nothing masked)."""
        if rec.join_side:   # the isolated last pass of a DDP-wrapped model: everything before it is done
            for st in self._streams:
                torch.cuda.current_stream().wait_stream(st)
            return
        if chain.order is not None and not whole_pass:   # per-group events instead (model.BackwardOrder); prev_done is its fallback
            return
        if chain.prev_done is not None:
            torch.cuda.current_stream().wait_event(chain.prev_done)

    def _rows_loss_backward(self, plan: StepPlan, rec: PassRecord, chain, batch: _Batch, x, y, attn_mask):
        """The two row-compact readouts (see __init__): the CE kernel turns logits into d(logits) rows of the masked positions — the
        row indices come from the host-side MLM draw, no device sync — and the two backward products contract over those rows.
        "dense": logits of every position in the forward, as model.py:253 computes them.  "masked" (SURVEY.md §8f rank 1): logits
        for the listed rows alone ([n_masked, V]), forward included."""
        from . import ops
        from .model import _Acc32FlushFn, _ReadoutRowsGradFn
        core = self._core
        rows, weights, tg = _pass_rows(batch, rec.j, plan.k, self.mini * x.shape[1])
        if rows.numel() == 0:
            # nothing masked in this pass (the reference would produce 0/0 = NaN here): still hand EVERY parameter a (zero)
            # gradient — lm_head included — or DDP's reducer would wait for it forever when this is the synchronising pass.
            # The readout's own node does not run in such a pass; with the fp32 sum its weight takes the zero contribution by
            # the pass's mode instead (model._Acc32FlushFn: the first pass zeroes the buffer, the last hands the other passes'
            # total to autograd and DDP's reducer).
            emb = self.model(x, attn_mask=attn_mask, return_embeddings=True)
            self._order_backward(rec, chain, whole_pass=True)
            head = _Acc32FlushFn.apply(core.lm_head.weight) if plan.fp32_sum else core.lm_head.weight.sum() * 0
            (emb.sum() * 0 + head).backward()
            return torch.zeros((), dtype=torch.float32, device=x.device)
        if self.teacher is not None:
            return self._distill_loss_backward(plan, rec, chain, x, y, attn_mask, rows, weights, tg)
        dense = plan.readout == "dense"
        if not dense and plan.rows_forward:
            # the model is told which positions are wanted: the last block's MLP half and ln_f run on them alone (model.forward(rows=))
            emb_rows = self.model(x, attn_mask=attn_mask, return_embeddings=True, rows=rows)
        else:
            emb = self.model(x, attn_mask=attn_mask, return_embeddings=True)
            emb_rows = None if dense else emb.reshape(-1, emb.shape[-1]).index_select(0, rows)
        with torch.no_grad():
            if dense:
                logits = core.lm_head(emb)                     # (B, T, V)
                loss, dl = ops.masked_ce_rows(logits, y.reshape(-1), rows, plan.n_accum, row_weights=weights)
            else:
                logits = core.lm_head(emb_rows)                # (n_masked, V): the rows the loss keeps (train_encoder.py:304)
                loss, dl = ops.masked_ce_rows(logits, tg if tg is not None else y.reshape(-1).index_select(0, rows), None, plan.n_accum,
                                              row_weights=weights)
        del logits
        self._order_backward(rec, chain)
        if dense:
            emb_rows = emb.reshape(-1, emb.shape[-1]).index_select(0, rows)
        wm = float(core.lm_head.output_mult) / float(core.lm_head.width_mult())
        _ReadoutRowsGradFn.apply(emb_rows, core.lm_head.weight, wm, dl).backward()
        return loss.detach()

    def _distill_loss_backward(self, plan: StepPlan, rec: PassRecord, chain, x, y, attn_mask, rows, weights, tg):
        """_rows_loss_backward with a teacher: the teacher's logits at the listed positions (no_grad: its blocks take the forward that
        keeps nothing), ops.distill_ce_rows in the place of ops.masked_ce_rows, the same two backward products.  Returns
        [loss, ce, kl], each under the step's normalisation."""
        from . import ops
        from .model import _ReadoutRowsGradFn
        core = self._core
        dense = plan.readout == "dense"
        if not dense and plan.rows_forward:
            emb_rows = self.model(x, attn_mask=attn_mask, return_embeddings=True, rows=rows)
        else:
            emb = self.model(x, attn_mask=attn_mask, return_embeddings=True)
            emb_rows = None if dense else emb.reshape(-1, emb.shape[-1]).index_select(0, rows)
        with torch.no_grad():
            t_mask = attn_mask
            if torch.is_tensor(attn_mask) and attn_mask.shape[1] != self.teacher.config.n_head:   # mask_impl="dense": one (T, T) table for every head
                t_mask = attn_mask[:, :1].expand(-1, self.teacher.config.n_head, -1, -1)
            t_logits = self.teacher.lm_head(self.teacher(x, attn_mask=t_mask, return_embeddings=True, rows=rows))
            if dense:   # logits of every position, as the dense readout computes them; the loss kernel takes the listed ones
                logits = core.lm_head(emb)
                logits = logits.reshape(-1, logits.shape[-1]).index_select(0, rows)
            else:
                logits = core.lm_head(emb_rows)
            labels = tg if tg is not None else y.reshape(-1).index_select(0, rows)
            loss, dl, row_ce, row_kl = ops.distill_ce_rows(logits, t_logits, labels, plan.n_accum, row_weights=weights,
                                                           alpha=self.distill_alpha, temperature=self.distill_temperature)
            if weights is None:
                parts = torch.stack([row_ce.sum(), row_kl.sum()]) / (rows.numel() * plan.n_accum)
            else:
                parts = torch.stack([(row_ce * weights).sum(), (row_kl * weights).sum()]) / plan.n_accum
        del logits, t_logits
        self._order_backward(rec, chain)
        if dense:
            emb_rows = emb.reshape(-1, emb.shape[-1]).index_select(0, rows)
        wm = float(core.lm_head.output_mult) / float(core.lm_head.width_mult())
        _ReadoutRowsGradFn.apply(emb_rows, core.lm_head.weight, wm, dl).backward()
        return torch.cat([loss.detach().reshape(1), parts])

    def _clm_batch(self, plan: StepPlan, input_ids, ids_host) -> _Batch:
        """objective="clm": no corruption — the batch itself, the scored positions per micro-batch and their labels (next_token_rows).
        With the host copy of the batch the lists are formed on the host and travel through reused pinned buffers as asynchronous
        copies, as in _host_prelude; without it they come from tensor ops and one blocking copy (the same one-time warning)."""
        labels = torch.roll(input_ids, shifts=-1, dims=1)
        if ids_host is None or not input_ids.is_cuda:
            if input_ids.is_cuda and not TrainStep._warned_no_host_copy:
                TrainStep._warned_no_host_copy = True
                import warnings
                warnings.warn("TrainStep: no input_ids_host given — the scored-row lists of the readout path need a "
                              "blocking device-to-host copy per optimizer step (pass the loader's host copy of the batch to avoid it)")
            lists, targets = next_token_rows_device(input_ids, self.mini, plan.n_accum)
            return _Batch(input_ids, None, lists, targets, labels)
        dev = input_ids.device
        rows, T = plan.rows, input_ids.shape[1]
        idx, lab = next_token_rows(np.asarray(ids_host)[:rows], self.mini, plan.n_accum)
        st = self._clm_bufs.get((rows, T, dev))
        if st is None:
            st = dict(rows_pin=torch.empty(rows * T, dtype=torch.int64).pin_memory(), rows_dev=torch.empty(rows * T, dtype=torch.int64, device=dev),
                      tgt_pin=torch.empty(rows * T, dtype=torch.int64).pin_memory(), tgt_dev=torch.empty(rows * T, dtype=torch.int64, device=dev), done=None)
            if len(self._clm_bufs) >= 4:           # --batch_ramp walks through many row counts: keep a few
                self._clm_bufs.pop(next(iter(self._clm_bufs)))
            self._clm_bufs[(rows, T, dev)] = st
        if st["done"] is not None:
            st["done"].synchronize()        # the previous step's copies out of these pinned buffers (long finished)
        sizes = [len(v) for v in idx]
        total = int(sum(sizes))
        if total:
            st["rows_pin"].numpy()[:total] = np.concatenate(idx)
            st["rows_dev"][:total].copy_(st["rows_pin"][:total], non_blocking=True)
            st["tgt_pin"].numpy()[:total] = np.concatenate(lab)
            st["tgt_dev"][:total].copy_(st["tgt_pin"][:total], non_blocking=True)
        off = np.concatenate([[0], np.cumsum(sizes)])
        lists = [st["rows_dev"][int(off[j]):int(off[j + 1])] for j in range(plan.n_accum)]
        targets = [st["tgt_dev"][int(off[j]):int(off[j + 1])] for j in range(plan.n_accum)]
        st["done"] = torch.cuda.current_stream().record_event()
        return _Batch(input_ids, None, lists, targets, labels)

    def _host_prelude(self, plan: StepPlan, input_ids, ids_host) -> _Batch:
        """The MLM corruption with every host-side input at hand (train_encoder.py:273-279): the Bernoulli draw AND the
        PAD/EOS exclusions are evaluated on the host copy of the batch, so the final mask — and from it the per-micro-batch
        lists of masked positions — is known without a device round trip.  Mask and lists go to the GPU through reused
        pinned buffers as asynchronous copies; the host never waits for the device here (the `.cpu()` of the device-side
        form stalls the host until the previous optimizer step has drained: 1.5-2 ms of idle GPU per step)."""
        dev = input_ids.device
        rows, n_accum, T = plan.rows, plan.n_accum, input_ids.shape[1]
        ids_h = np.asarray(ids_host)[:rows]
        draw = np.random.binomial(1, 0.15, (rows, T))                                  # same call, same stream as mlm_corrupt
        mask_h = (draw != 0) & (ids_h != PAD_TOKEN) & (ids_h != EOS_TOKEN)
        st = self._host_bufs.get((rows, T, dev))
        if st is None:
            st = dict(mask_pin=torch.empty((rows, T), dtype=torch.bool).pin_memory(), rows_pin=torch.empty(rows * T, dtype=torch.int64).pin_memory(),
                      mask_dev=torch.empty((rows, T), dtype=torch.bool, device=dev), rows_dev=torch.empty(rows * T, dtype=torch.int64, device=dev),
                      tgt_pin=torch.empty(rows * T, dtype=torch.int64).pin_memory(), tgt_dev=torch.empty(rows * T, dtype=torch.int64, device=dev),
                      done=None)
            if len(self._host_bufs) >= 4:          # --batch_ramp walks through many row counts: keep a few
                self._host_bufs.pop(next(iter(self._host_bufs)))
            self._host_bufs[(rows, T, dev)] = st
        if st["done"] is not None:
            st["done"].synchronize()        # the previous step's copies out of these pinned buffers (long finished)
        st["mask_pin"].numpy()[...] = mask_h
        st["mask_dev"].copy_(st["mask_pin"], non_blocking=True)
        lists = targets = None
        if plan.sparse_rows:
            per = mask_h.reshape(n_accum, -1)
            idx = [np.flatnonzero(per[j]) for j in range(n_accum)]
            sizes = [len(v) for v in idx]
            total = int(sum(sizes))
            if total:
                st["rows_pin"].numpy()[:total] = np.concatenate(idx)
                st["rows_dev"][:total].copy_(st["rows_pin"][:total], non_blocking=True)
                # the labels of those positions (the uncorrupted ids), in the same order: the compact CE needs no device-side gather
                per_ids = ids_h.reshape(n_accum, -1)
                st["tgt_pin"].numpy()[:total] = np.concatenate([per_ids[j][idx[j]] for j in range(n_accum)])
                st["tgt_dev"][:total].copy_(st["tgt_pin"][:total], non_blocking=True)
            off = np.concatenate([[0], np.cumsum(sizes)])
            lists = [st["rows_dev"][int(off[j]):int(off[j + 1])] for j in range(n_accum)]
            targets = [st["tgt_dev"][int(off[j]):int(off[j + 1])] for j in range(n_accum)]
        st["done"] = torch.cuda.current_stream().record_event()
        mask = st["mask_dev"]
        return _Batch(input_ids.masked_fill(mask, MASK_TOKEN), mask, lists, targets)

    def _prepare_batch(self, plan: StepPlan, input_ids, mlm_mask, input_ids_host) -> _Batch:
        """The corrupted ids, the mask and — for the row-compact readouts — the masked positions per micro-batch, from the host
        prelude, the host Bernoulli draw (mlm_corrupt) or the caller's mlm_mask.  objective="clm": _clm_batch."""
        if self.objective == "clm":
            if mlm_mask is not None:
                raise ValueError('TrainStep(objective="clm"): there is no corruption, mlm_mask has no meaning')
            return self._clm_batch(plan, input_ids, input_ids_host)
        if mlm_mask is None and input_ids_host is not None and input_ids.is_cuda:
            return self._host_prelude(plan, input_ids, input_ids_host)
        if mlm_mask is None:
            masked_ids, mask = mlm_corrupt(input_ids)
        else:
            mask = mlm_mask[:plan.rows].to(input_ids.device) & (input_ids != PAD_TOKEN) & (input_ids != EOS_TOKEN)
            masked_ids = input_ids.masked_fill(mask, MASK_TOKEN)
        lists = None
        if plan.sparse_rows:
            # per-micro-batch row indices of the masked positions; mlm_corrupt drew the mask on the host, but PAD/EOS
            # exclusions were applied on the device, so fetch the final mask once per optimizer step (one small D2H copy)
            if input_ids.is_cuda and mlm_mask is None and not TrainStep._warned_no_host_copy:
                TrainStep._warned_no_host_copy = True
                import warnings
                warnings.warn("TrainStep: no input_ids_host given — the masked-row lists of the default readout path need a "
                              "blocking device-to-host copy per optimizer step (pass the loader's host copy of the batch to avoid it)")
            mh = mask.reshape(plan.n_accum, -1).cpu()
            lists = [torch.nonzero(mh[j], as_tuple=False).reshape(-1).to(input_ids.device) for j in range(mh.shape[0])]
        return _Batch(masked_ids, mask, lists, None)

    def _fork_streams(self, plan: StepPlan):
        """The caller's stream when the step is pipelined, its side streams made to wait for it; else None."""
        if not plan.pipelined:
            return None
        main = torch.cuda.current_stream()
        if self._streams is None or len(self._streams) != plan.ns:
            self._streams = [torch.cuda.Stream() for _ in range(plan.ns)]
            # gradients are produced on the side streams by design; the engine's cross-stream sync is what we want
            warn_off = getattr(torch.autograd.graph, "set_warn_on_accumulate_grad_stream_mismatch", None)
            if warn_off is not None:
                warn_off(False)
        for st in self._streams:
            st.wait_stream(main)
        return main

    def _run_pass(self, plan: StepPlan, rec: PassRecord, chain, batch: _Batch, input_ids, ranges, emb_orders, dtype):
        """Forward, loss and backward of one pass on the current stream; its share of the step's loss."""
        from .model import BackwardOrder, embedding_order
        sl = slice(rec.j * plan.span, (rec.j + 1) * plan.span)
        x, y = batch.masked_ids[sl], (input_ids if batch.labels is None else batch.labels)[sl]
        attn_mask = self._mask(plan, ranges, rec.j, dtype)
        ctx = self.model.no_sync() if rec.no_sync else contextlib.nullcontext()
        # this pass's slice of the step-wide id sort, for its embedding backward
        ctx_order = embedding_order(emb_orders[rec.j]) if emb_orders is not None else contextlib.nullcontext()
        chain.order = BackwardOrder(chain.prev_events, chain.prev_done) if rec.ordered else None
        with ctx, ctx_order, self._delivery(rec, chain.order):
            if plan.sparse_rows:
                loss = self._rows_loss_backward(plan, rec, chain, batch, x, y, attn_mask)
            else:
                logits = self.model(x, attn_mask=attn_mask)
                loss = self._loss_backward(rec, chain, logits, y, batch.mask[sl], plan.n_accum)
                del logits
        if rec.side:
            chain.prev_done = torch.cuda.current_stream().record_event()
            chain.prev_events = chain.order.events if chain.order is not None else None
        return loss

    def __call__(self, input_ids: torch.Tensor, mlm_mask: Optional[torch.Tensor] = None, input_ids_host=None) -> Dict[str, torch.Tensor]:
        """mlm_mask (optional, bool (rows, T)): the positions to corrupt instead of the host Bernoulli draw of
        train_encoder.py:273-274 (PAD/EOS are still excluded) — lets tests hand two runs the same corruption.
        input_ids_host (optional, the same batch as a host array/tensor, e.g. what the loader produced before its H2D copy):
        lets the step form the MLM mask without waiting for the device (see _host_prelude); results are identical.
        NEEDED for the sync-free path of the default readout (lm_head_impl="dense" / "masked" list the masked rows per
        micro-batch): without it the final mask comes back from the device once per optimizer step — a blocking D2H copy that
        waits for the previous step to drain (a one-time warning says so)."""
        from . import masks
        self._check_objective()   # (the public attributes may have been reassigned since the constructor)
        plan = self._resolve(input_ids.shape[0], input_ids.is_cuda)
        input_ids = input_ids[:plan.rows]
        self.optimizer.zero_grad(set_to_none=True)
        batch = self._prepare_batch(plan, input_ids, mlm_mask, input_ids_host)
        self._mask_rows_host = batch.rows
        if plan.fp32_sum:
            self._refuse_env_switches()
        dtype = next(self.model.parameters()).dtype
        emb_orders = self._embedding_orders(plan, batch.masked_ids)
        ranges = masks.RangeMask.from_tokens(input_ids, padding=self.use_padding, group=self.mini, causal=self.objective == "clm")
        # the loss, summed per stream (with a teacher: [loss, ce, kl])
        partial = [torch.zeros((3,) if self.teacher is not None else (), dtype=torch.float32, device=input_ids.device) for _ in range(plan.ns)]
        main = self._fork_streams(plan)
        # what links the backward passes of this call's side passes: the event after the previous one, that pass's per-group events,
        # and the BackwardOrder of the pass being built
        chain = SimpleNamespace(prev_done=None, prev_events=None, order=None)
        for rec in (pass_record(plan, j) for j in range(plan.n_pass)):
            # an isolated last pass: its forward still runs beside the previous backward passes (it only reads weights); the
            # caller's stream joins the side streams right before its backward (_order_backward)
            with (torch.cuda.stream(self._streams[rec.slot]) if rec.side else contextlib.nullcontext()):
                partial[rec.slot] += self._run_pass(plan, rec, chain, batch, input_ids, ranges, emb_orders, dtype)
        if input_ids.is_cuda and hasattr(self.model, "_obte_timed_hook"):   # measurement only (comm.TimedHook): the step's last backward ends here
            self.backward_end_event = torch.cuda.Event(enable_timing=True)
            self.backward_end_event.record()
        cum_loss = partial[0]
        if plan.pipelined:
            for st in self._streams:   # (a no-op after an isolated last pass: that one already waited for them)
                main.wait_stream(st)
            for extra in partial[1:]:
                cum_loss = cum_loss + extra
        if isinstance(self.optimizer, FusedAdamW):
            self.optimizer.step(max_norm=self.max_grad_norm)
        else:
            torch.nn.utils.clip_grad_norm_(self.model.parameters(), self.max_grad_norm)
            self.optimizer.step()
        if self.scheduler is not None:
            self.scheduler.step()
        tokens = (input_ids != PAD_TOKEN).sum()
        if self.teacher is not None:
            return {"loss": cum_loss[0], "tokens": tokens, "ce": cum_loss[1], "kl": cum_loss[2]}
        return {"loss": cum_loss, "tokens": tokens}


# ------------------------------------------------------------------------------------------------- model set-up
def set_dropout(model, p: float) -> None:
    """Change the dropout probability of a built model (config.dropout feeds four sites: model.py:83-84,160,204)."""
    core = model.module if hasattr(model, "module") else model
    core.config.dropout = p
    core.transformer.drop.p = p
    for blk in core.transformer.h:
        blk.attn.dropout = p
        blk.attn.attn_dropout.p = p
        blk.attn.resid_dropout.p = p
        blk.mlp.dropout.p = p


def build_model(args, device, dtype=torch.bfloat16, vocab_size: int = 2 ** 16):
    """train_encoder.py:145-170: target model, muP base/delta models sharing ONE mutated config object,
    set_base_shapes, cast, move."""
    from .model import OmniBioTA, OmniBioTAConfig
    try:
        from mup import set_base_shapes  # type: ignore
    except Exception:
        from .mup_compat import set_base_shapes
    config = OmniBioTAConfig()
    config.vocab_size = vocab_size
    config.dropout = args.dropout
    config.block_size = args.ctx_len
    config.n_embd = args.n_embd
    config.n_layer = args.n_layer
    config.n_head = args.n_head
    config.flash = not args.disable_flash
    config.checkpoint_freq = args.checkpoint_freq
    config.autoregressive = getattr(args, "objective", "mlm") == "clm"   # --objective clm: a causal model (generate / score / sample serve it)
    m = OmniBioTA(config)
    config.n_embd, config.n_head = 24, 3
    base_model = OmniBioTA(config)
    config.n_embd, config.n_head = 48, 12
    delta_model = OmniBioTA(config)
    set_base_shapes(m, base_model, delta=delta_model)
    del base_model, delta_model
    config.n_embd, config.n_head = args.n_embd, args.n_head   # the reference leaves 48/12 behind; nothing reads it
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")   # "Casting complex values to real": the reference's cos-only RoPE regime
        m.to(dtype)
    m.to(device)
    return m


def build_optimizer(model, args, total_iters: int, fused: bool = True, master_weights: Optional[bool] = None):
    """train_encoder.py:195-201.  master_weights (default: args.master_weights): fp32 master weights and moments behind the bf16
    parameters (FusedAdamW(master_weights=True): beyond the reference, off by default)."""
    if master_weights is None:
        master_weights = bool(getattr(args, "master_weights", False))
    if master_weights and not fused:
        raise ValueError("--master_weights needs the fused HIP optimizer (--device cuda): there is no CPU path for it")
    lr = args.lr * np.sqrt(args.batch_size) / 32
    params = list(model.parameters())
    betas = (args.beta1, args.beta2)
    if args.force_lr:
        groups = [{"params": params}]
    else:
        from .mup_compat import mu_param_groups
        groups = mu_param_groups(params, lr, args.weight_decay)
    if fused:
        opt = FusedAdamW(groups, lr=lr, betas=betas, eps=args.epsilon, weight_decay=args.weight_decay, master_weights=master_weights)
    else:
        opt = torch.optim.AdamW(groups, lr=lr, betas=betas, eps=args.epsilon, weight_decay=args.weight_decay)
    sched = torch.optim.lr_scheduler.LinearLR(opt, start_factor=1.0, end_factor=0.0, total_iters=max(total_iters, 1))
    return opt, sched


def flops_per_token(num_model_params: int, n_layer: int, n_embd: int, ctx_len: int) -> float:
    return 6.0 * num_model_params + 12.0 * n_layer * n_embd * ctx_len   # train_encoder.py:360


def flops_per_token_executed(num_model_params: int, n_layer: int, n_embd: int, ctx_len: int, lm_head_impl: str = "masked",
                             rows_forward: bool = True, vocab: int = 2 ** 16, masked_fraction: float = 0.15,
                             attention_fraction: float = 1.0, rows_attention: Optional[bool] = None) -> float:
    """FLOP per token the step actually EXECUTES: the reference's 6N + 12LCT minus the products the readout form leaves out on
    the (1 - masked_fraction) of the positions the loss multiplies by zero (train_encoder.py:304) — "dense": the two backward
    products of the readout; "masked": all three, and with rows_forward the last block's MLP half (8 C^2 parameters) as well;
    rows_attention (default: as rows_forward; the library takes this form without a dense mask, csrc/block.cpp rows_attn): also the
    last block's attention projection and the q third of its c_attn (C^2 parameters each) and its attention for the queries at
    those positions — keys and values of every position are still formed."""
    skip = 1.0 - masked_fraction
    skipped = {"dense": 4.0 * n_embd * vocab * skip, "dense_full": 0.0, "masked": 6.0 * n_embd * vocab * skip}[lm_head_impl]
    if lm_head_impl == "masked" and rows_forward:
        skipped += 6.0 * 8.0 * n_embd ** 2 * skip
        if rows_attention is None or rows_attention:
            skipped += (2 * 6.0 * n_embd ** 2 + 12.0 * n_embd * ctx_len * attention_fraction) * skip   # c_proj and c_attn's q third: C^2 parameters each
    # attention_fraction < 1 (rows that pack several documents): the share of the 12 L C T attention term the kernels visit
    skipped += 12.0 * n_layer * n_embd * ctx_len * (1.0 - attention_fraction)
    return flops_per_token(num_model_params, n_layer, n_embd, ctx_len) - skipped


def wrap_ddp(model, device_index: Optional[int], bucket_cap_mb: int = 100, grad_exchange: str = "allreduce", timed: bool = False):
    """DDP over RCCL.  Buckets of ~100 MB (a few per all-reduce of small's 470 MB) keep each ring/tree step long
    enough to run at xGMI link rate while still overlapping the tail of backward; gradients are views into the
    buckets, so the reducer never copies.
    grad_exchange: "allreduce" — DDP's own bucketed all-reduce (train_encoder.py:185 as the reference runs it); "all_links" — the
    direct reduce-scatter + all-gather of comm.AllLinksHook (every xGMI link of the mesh at once, fp32 fixed-order reduction: SURVEY
    section 5).  timed: wrap the exchange in comm.TimedHook (per-bucket device events; the wrapper hangs on the returned module as
    ``_obte_timed_hook``) — measurement only."""
    from torch.nn.parallel import DistributedDataParallel as DDP
    from . import comm
    assert grad_exchange in ("allreduce", "all_links"), grad_exchange
    kw = dict(bucket_cap_mb=bucket_cap_mb, gradient_as_bucket_view=True, broadcast_buffers=False)
    ddp = DDP(model, **kw) if device_index is None else DDP(model, device_ids=[device_index], **kw)
    hook = comm.AllLinksHook() if grad_exchange == "all_links" else (comm.allreduce_mean_hook() if timed else None)
    if timed and hook is not None:
        hook = comm.TimedHook(hook)
        ddp._obte_timed_hook = hook
    if hook is not None:
        ddp.register_comm_hook(None, comm.as_ddp_hook(hook, f"obte_{grad_exchange}{'_timed' if timed else ''}_hook"))
    return ddp


def parse_args(argv=None):
    p = argparse.ArgumentParser(description="OmniBioTE masked-LM training on MI355X (synthetic data)")
    p.add_argument("--batch_size", type=int, default=1024)
    p.add_argument("--mini_batch_size", type=int, default=8)
    p.add_argument("--n_head", type=int, default=8)
    p.add_argument("--n_embd", type=int, default=1024)
    p.add_argument("--n_layer", type=int, default=8)
    p.add_argument("--ctx_len", type=int, default=2048)
    p.add_argument("--dropout", type=float, default=0.1)
    p.add_argument("--lr", type=float, default=1e-2)
    p.add_argument("--beta1", type=float, default=0.9)
    p.add_argument("--beta2", type=float, default=0.999)
    p.add_argument("--epsilon", type=float, default=1e-8)
    p.add_argument("--weight_decay", type=float, default=1e-2)
    p.add_argument("--token_budget", type=float, default=20e9)
    p.add_argument("--test_freq", type=int, default=int(1e7))
    p.add_argument("--save_freq", type=int, default=int(1e9))
    p.add_argument("--save_name", type=str, default="omnibiota")
    p.add_argument("--disable_flash", action="store_true", default=False)
    p.add_argument("--wandb_project_name", type=str, default="omnibiota")
    p.add_argument("--base_dir", type=str, default="")
    p.add_argument("--force_lr", action="store_true", default=False)
    p.add_argument("--checkpoint_freq", type=int, default=0)
    p.add_argument("--banned_token", type=int, default=BANNED_MIXED)
    p.add_argument("--warmup_period", type=float, default=0.05)
    p.add_argument("--batch_ramp", action="store_true", default=False)
    p.add_argument("--train_type", type=str, default="mixed")
    p.add_argument("--FSDP", action="store_true", default=False)
    p.add_argument("--use_padding", action="store_true", default=False)
    p.add_argument("--resume_from", type=int, default=0)
    # additions
    p.add_argument("--max_steps", type=int, default=0, help="stop after this many optimizer steps (0 = token budget)")
    p.add_argument("--multi_document", action="store_true", default=False, help="synthetic rows with interior EOS")
    p.add_argument("--pipeline_streams", type=int, default=2, choices=[1, 2, 3],
                   help="2: overlap the forward of micro-batch j+1 with the backward of micro-batch j (same results)")
    p.add_argument("--micro_batches_per_pass", type=int, default=1,
                   help="k > 1: k micro-batches of --mini_batch_size rows per forward/backward pass (masks and loss normalisation stay per "
                        "micro-batch: same loss and gradients; +4-6 %% at k = 2-4 on the small config, bench.py chooses it by measurement)")
    p.add_argument("--grad_exchange", default="allreduce", choices=["allreduce", "all_links"],
                   help="allreduce: DDP's bucketed all-reduce as the reference runs it; all_links: direct reduce-scatter + all-gather over "
                        "every xGMI link of the node at once (comm.AllLinksHook; fp32 fixed-order reduction, one rounding)")
    p.add_argument("--backend", default="nccl", choices=["nccl", "gloo"],
                   help="torch.distributed backend: nccl (= RCCL over xGMI, the production path) or gloo (plumbing runs: "
                        "BASELINE config 1; gradients then cross the host)")
    p.add_argument("--master_weights", action="store_true", default=False,
                   help="fp32 master weights and fp32 moments behind the bf16 parameters (12 instead of 4 bytes of optimizer state per "
                        "parameter; beyond the reference's pure-bf16 regime, so loss curves no longer track the reference's step for "
                        "step); they travel in the optimizer checkpoint and --resume_from restores them")
    p.add_argument("--fp32_grad_accum", action="store_true", default=False,
                   help="sum every weight gradient over the micro-batches of a step in fp32 and round it to bf16 once, instead of after "
                        "every micro-batch (+4 bytes per parameter of scratch; beyond the reference's arithmetic, like --master_weights, whose "
                        "fp32 masters it feeds with a gradient rounded once); not with --checkpoint_freq > 0")
    p.add_argument("--objective", default="mlm", choices=["mlm", "clm"],
                   help="mlm: the reference's masked-LM objective; clm: next-token prediction — the model is built autoregressive "
                        "(config.autoregressive), no corruption, document-causal attention, every position with a successor in its own document scored")
    p.add_argument("--distill_from", type=str, default="",
                   help="--objective clm only: a checkpoint written by checkpoint.save_checkpoint of an autoregressive teacher with the same vocabulary; "
                        "the loss becomes distill_alpha * CE + (1 - distill_alpha) * T^2 * KL(teacher || student) at temperature T")
    p.add_argument("--teacher_n_layer", type=int, default=0, help="the teacher's depth (0: --n_layer)")
    p.add_argument("--teacher_n_embd", type=int, default=0, help="the teacher's width (0: --n_embd)")
    p.add_argument("--teacher_n_head", type=int, default=0, help="the teacher's heads (0: --n_head)")
    p.add_argument("--distill_alpha", type=float, default=0.5, help="weight of the hard-label cross entropy in the distillation loss")
    p.add_argument("--distill_temperature", type=float, default=1.0, help="temperature both distributions are softened by in the KL term")
    p.add_argument("--device", default="cuda", choices=["cuda", "cpu"],
                   help="cpu only exercises the harness plumbing: the model itself has no CPU path and says so at the first forward")
    return p.parse_args(argv)


def effective_batch(i: int, total_iters: int, args, batch_size: int) -> int:
    """Batch-size ramp of train_encoder.py:245-255."""
    mini = args.mini_batch_size
    if args.batch_ramp:
        e = min((int(i / (total_iters * args.warmup_period) * batch_size) // mini) * mini + mini, batch_size)
    else:
        e = batch_size
    return e // mini * mini


TRAIN_TYPES = {   # train_encoder.py:72-93
    "protein": (["uniref100/train"], [1.0]),
    "nucleotide": (["genbank/train"], [1.0]),
    "mixed": (["genbank/train", "uniref100/train"], [0.80, 0.20]),
    "halfnhalf": (["genbank/train", "uniref100/train"], [0.50, 0.50]),
}
TEST_SETS = {     # train_encoder.py:72-93: (test_dirs, test_names)
    "protein": (["uniref100/val"], ["uniref100"]),
    "nucleotide": (["genbank/val"], ["genbank"]),
    "mixed": (["genbank/val", "uniref100/val"], ["genbank", "uniref100"]),
    "halfnhalf": (["genbank/val", "uniref100/val"], ["genbank", "uniref100"]),
}


def make_batch_source(args, batch_size: int, device, rng):
    """``(next_batch, description, close)``: ``next_batch(rows) -> LongTensor (rows, ctx_len)`` on ``device``; real shards
    when --base_dir has them, else synthetic.  ``close()`` stops and joins the loader thread (call it before tearing the
    process group down)."""
    if args.train_type not in TRAIN_TYPES:
        raise ValueError("Invalid train_type. Must be one of 'protein', 'nucleotide', 'mixed', or 'halfnhalf'")
    dirs, props = TRAIN_TYPES[args.train_type]
    dirs = [os.path.join(args.base_dir, d) for d in dirs] if args.base_dir else []
    if dirs and all(os.path.isdir(d) and os.listdir(d) for d in dirs):
        import queue
        import threading
        from . import loader as LD
        files = [sorted(os.path.join(d, f) for f in os.listdir(d)) for d in dirs]
        readers = [LD.line_reader(f, banned_tokens=[args.banned_token]) for f in files]
        gens = [LD.get_sequence(r, args.ctx_len, args.use_padding) for r in readers]
        batches = LD.get_batch(gens, LD.batch_split(batch_size, props), return_pt=True)
        q = queue.Queue(maxsize=2)                                   # train_encoder.py:140-142
        stop = threading.Event()
        th = threading.Thread(target=LD.data_loader_parallel, args=(q, batches, device, stop), daemon=True)
        th.start()
        pool = [q.get(block=True)]

        def real(rows):
            while sum(b.shape[0] for b in pool) < rows:              # the reference's grand_batch top-up (:258-261)
                pool.append(q.get(block=True))
            hosts = [getattr(b, "_obte_host_copy", None) for b in pool]
            cat = torch.cat(pool, dim=0) if len(pool) > 1 else pool[0]
            host = None if any(h is None for h in hosts) else (np.concatenate(hosts) if len(hosts) > 1 else hosts[0])
            rest, out = cat[rows:], cat[:rows]
            if host is not None:      # the host copies travel with the rows they belong to
                rest._obte_host_copy, out._obte_host_copy = host[rows:], host[:rows]
            pool[:] = [rest]
            return out

        def close():
            stop.set()
            while th.is_alive():
                try:
                    q.get_nowait()
                except queue.Empty:
                    pass
                th.join(timeout=0.1)
        return real, "shards under " + args.base_dir, close
    if args.base_dir:
        print(f"note: no token shards under {args.base_dir}; training on synthetic rows")

    def synth(rows):
        host = synthetic_rows(rows, args.ctx_len, 2 ** 16, rng, single_document=not args.multi_document)
        dev_t = torch.from_numpy(host).to(device)
        dev_t._obte_host_copy = host      # lets TrainStep form the MLM mask without a device round trip
        return dev_t
    return synth, "synthetic rows", (lambda: None)


def make_test_sources(args, device, rng):
    """Held-out generators for the periodic evaluation (train_encoder.py:131-133): ``[(name, next_rows)]`` where
    ``next_rows(n) -> LongTensor (n, ctx_len)``.  The ``*/val`` shard directories when --base_dir has them, else one
    synthetic stream from its own RNG."""
    dirs, names = TEST_SETS[args.train_type]
    dirs = [os.path.join(args.base_dir, d) for d in dirs] if args.base_dir else []
    out = []
    if dirs and all(os.path.isdir(d) and os.listdir(d) for d in dirs):
        from . import loader as LD
        for d, name in zip(dirs, names):
            files = sorted(os.path.join(d, f) for f in os.listdir(d))
            gen = LD.get_sequence(LD.line_reader(files, banned_tokens=[args.banned_token]), args.ctx_len, args.use_padding)

            def rows_from(n, gen=gen):
                arr = np.concatenate([np.asarray(next(gen)).reshape(1, -1) for _ in range(n)])   # :376-379
                return torch.as_tensor(arr, dtype=torch.long, device=device)
            out.append((name, rows_from))
        return out
    trng = np.random.default_rng(int(rng.integers(1 << 31)) + 7919)

    def synth(n):
        return torch.from_numpy(synthetic_rows(n, args.ctx_len, 2 ** 16, trng, single_document=not args.multi_document)).to(device)
    return [("synthetic", synth)]


@torch.no_grad()
def evaluate(model, test_sources, args, world: int, device) -> Dict[str, float]:
    """The held-out pass of train_encoder.py:371-410: model.eval(), one mini-batch per test set, the same MLM corruption
    and attention mask as training, loss = sum_masked(CE) / n_masked / world on every rank, summed over ranks.
    --objective clm: the mean next-token loss over the scored positions of the mini-batch (next_token_rows) under the document-causal
    mask, through the row-compact readout; no MLM draw."""
    from . import masks, ops
    core = model.module if hasattr(model, "module") else model
    was_training = core.training
    model.eval()
    out = {}
    clm = getattr(args, "objective", "mlm") == "clm"
    for name, next_rows in test_sources:
        test_batch = next_rows(args.mini_batch_size)
        if clm:
            rows, labels = next_token_rows_device(test_batch, test_batch.shape[0], 1)
            if rows[0].numel() == 0:
                loss = torch.full((), float("nan"), dtype=torch.float32, device=test_batch.device)   # nothing to score: 0 / 0, as the MLM mean gives
            else:
                attn = masks.RangeMask.from_tokens(test_batch, padding=args.use_padding, causal=True)
                attn = ops.MaskSpec.from_user(attn, test_batch.shape[0], test_batch.shape[1], core.config.n_head, test_batch.device)
                emb_rows = model(test_batch, attn_mask=attn, return_embeddings=True, rows=rows[0])
                loss, _ = ops.masked_ce_rows(core.lm_head(emb_rows), labels[0], None, 1)
            loss = loss.float() / world
            if world > 1:
                dist.all_reduce(loss)
            out[name] = float(loss.item())
            continue
        masked_ids, mask = mlm_corrupt(test_batch)
        attn = masks.RangeMask.from_tokens(test_batch, padding=args.use_padding)
        logits = model(masked_ids, attn_mask=attn)
        if logits.is_cuda and logits.dtype == torch.bfloat16:
            loss, _ = ops.masked_ce(logits, test_batch, mask, 1)
        else:
            ce = F.cross_entropy(logits.view(-1, logits.size(-1)).float(), test_batch.view(-1), reduction="none")
            loss = (ce * mask.view(-1).float()).sum() / mask.view(-1).sum()
        loss = loss.float() / world
        if world > 1:
            dist.all_reduce(loss)
        out[name] = float(loss.item())
    model.train(was_training)
    return out


def load_teacher(args, student, device):
    """--distill_from: the teacher out of a checkpoint.save_checkpoint file, in bf16 on ``device``.  Its shape is the one the
    --teacher_n_layer / --teacher_n_embd / --teacher_n_head flags declare (each defaults to the student's value): a checkpoint of
    another shape is refused, so that a mistaken path does not train against the wrong model unnoticed."""
    from .checkpoint import load_checkpoint
    if getattr(args, "objective", "mlm") != "clm":
        raise ValueError("--distill_from needs --objective clm")
    t = load_checkpoint(args.distill_from, map_location=device)
    want = {"n_layer": getattr(args, "teacher_n_layer", 0) or args.n_layer, "n_embd": getattr(args, "teacher_n_embd", 0) or args.n_embd,
            "n_head": getattr(args, "teacher_n_head", 0) or args.n_head}
    have = {k: getattr(t.config, k) for k in want}
    if have != want:
        raise ValueError(f"--distill_from {args.distill_from}: the checkpoint's model has {have}, expected {want} (--teacher_n_layer / --teacher_n_embd / "
                         "--teacher_n_head; each defaults to the student's value)")
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")   # "Casting complex values to real", as in build_model
        t.to(torch.bfloat16)
    return t.to(device).eval()


def run(args):
    if args.FSDP:
        raise NotImplementedError("--FSDP is outside this build's scope (the north star names DDP)")
    backend = getattr(args, "backend", "nccl")
    on_gpu = getattr(args, "device", "cuda") == "cuda"
    if backend == "nccl" and not on_gpu:
        raise SystemExit("--backend nccl (RCCL) needs --device cuda; use --backend gloo for a CPU plumbing run")
    if "RANK" not in os.environ and "WORLD_SIZE" not in os.environ:   # a bare `python train_encoder.py` is a world of one;
        os.environ["RANK"], os.environ["WORLD_SIZE"] = "0", "1"         # a launcher that set only one of the two is a mis-launch
    elif "RANK" not in os.environ or "WORLD_SIZE" not in os.environ:
        raise SystemExit("train_encoder: RANK and WORLD_SIZE must both be set by the launcher (or neither, for a single process)")
    for k, v in (("MASTER_ADDR", "127.0.0.1"), ("MASTER_PORT", "29511")):
        os.environ.setdefault(k, v)
    # torchrun sets LOCAL_RANK; srun / mpirun style launchers set only RANK: then bind like the reference does,
    # rank % GPUs on the node (train_encoder.py:110-111)
    local = int(os.environ.get("LOCAL_RANK", int(os.environ["RANK"]) % max(torch.cuda.device_count(), 1) if on_gpu else 0))
    if on_gpu:
        torch.cuda.set_device(local)
        device = torch.device("cuda", local)
    else:
        device = torch.device("cpu")
    dist.init_process_group(backend, **({"device_id": device} if backend == "nccl" else {}))   # nccl = RCCL on ROCm
    rank, world = dist.get_rank(), dist.get_world_size()
    assert args.batch_size % world == 0, "Batch size must be divisible by the number of processes."
    batch_size = args.batch_size // world
    np.random.seed(1234 + rank)
    torch.manual_seed(1234)   # identical initial weights on every rank (DDP broadcasts rank 0's anyway)
    m = build_model(args, device)
    if args.resume_from > 0:   # train_encoder.py:174-178
        from .checkpoint import load_checkpoint
        m = load_checkpoint(f"{args.save_name}_{args.resume_from}.pt", map_location=device)
        m.to(torch.bfloat16).to(device)
        print(f"Loaded model from {args.resume_from} token checkpoint")
    torch.manual_seed(1234 + rank)   # per-rank dropout streams from here on
    n_params = m.get_num_params()
    if on_gpu:
        from . import tune
        tune.tune_model_shapes(max(1, getattr(args, "micro_batches_per_pass", 1)) * args.mini_batch_size * args.ctx_len, args.n_embd, 2 ** 16,
                               device=device, verbose=(rank == 0))
        if world > 1:   # every rank adopts rank 0's plan table: the replicas then run the same kernels
            box = [tune.export_plans() if rank == 0 else None]
            dist.broadcast_object_list(box, src=0)
            if rank != 0:
                tune.import_plans(box[0])
    model = wrap_ddp(m, local if on_gpu else None, grad_exchange=getattr(args, "grad_exchange", "allreduce")) if world > 1 else m
    total_iters = int(args.token_budget / (world * batch_size * args.ctx_len))
    opt, sched = build_optimizer(m, args, total_iters, fused=on_gpu)
    objective = getattr(args, "objective", "mlm")
    teacher = load_teacher(args, m, device) if getattr(args, "distill_from", "") else None
    step = TrainStep(model, opt, sched, mini_batch_size=args.mini_batch_size, n_head=args.n_head, use_padding=args.use_padding,
                     pipeline_streams=getattr(args, "pipeline_streams", 1), micro_batches_per_pass=getattr(args, "micro_batches_per_pass", 1),
                     grad_accum="fp32" if getattr(args, "fp32_grad_accum", False) else "bf16", objective=objective, teacher=teacher,
                     distill_alpha=getattr(args, "distill_alpha", 0.5), distill_temperature=getattr(args, "distill_temperature", 1.0))
    rng = np.random.default_rng(1234 + rank)
    next_batch, source, close_source = make_batch_source(args, batch_size, device, rng)
    test_sources = make_test_sources(args, device, rng)
    if rank == 0:
        print(f"data: {source}; backend {backend}, world {world}, device {device}")
    trained, last_save, last_test, start = 0, 0, 0, 0
    if args.resume_from > 0:   # train_encoder.py:210-223 (optimizer/scheduler as state_dicts, not whole objects)
        trained = last_save = last_test = args.resume_from
        start = int(total_iters * (trained / args.token_budget))
        st = torch.load(f"{args.save_name}_optimizer_{args.resume_from}.pt", map_location=device, weights_only=False)
        opt.load_state_dict(st["optimizer"]); sched.load_state_dict(st["scheduler"])
    fpt = flops_per_token(n_params, args.n_layer, args.n_embd, args.ctx_len)   # the reference's MFU formula (:360)
    # what this step executes: its default readout runs on the ~15 % MLM-masked positions only (fewer FLOP, same gradients)
    fpt_exec = flops_per_token_executed(n_params, args.n_layer, args.n_embd, args.ctx_len, step.lm_head_impl, step.rows_forward,
                                        rows_attention=step.rows_forward and step.mask_impl == "ranges",
                                        masked_fraction=1.0 if objective == "clm" else 0.15)   # (clm scores nearly every position; a teacher's forward is not counted)
    n_steps = total_iters if args.max_steps <= 0 else min(total_iters, start + args.max_steps)

    def save(tag):
        from .checkpoint import save_checkpoint
        save_checkpoint(model, f"{args.save_name}{tag}.pt")
        torch.save({"optimizer": opt.state_dict(), "scheduler": sched.state_dict()}, f"{args.save_name}_optimizer{tag}.pt")

    history = []
    try:
        for i in range(start, n_steps):
            t0 = time.time()
            rows = effective_batch(i, total_iters, args, batch_size)
            ids = next_batch(rows)
            out = step(ids, input_ids_host=getattr(ids, "_obte_host_copy", None))
            stats = torch.stack([out["loss"], out["tokens"].float()] + ([out["ce"], out["kl"]] if teacher is not None else []))
            if world > 1:
                dist.all_reduce(stats)
            if on_gpu:
                torch.cuda.synchronize()
                from . import _lib
                _lib.check_device_status(f"step {i}")   # a kernel that found its own results invalid says so here, not never
            dt = time.time() - t0
            loss, toks = stats[0].item() / world, int(stats[1].item())
            trained += toks
            history.append(loss)
            if rank == 0:
                lrs = [g["lr"] for g in opt.param_groups]
                parts = f" ce {stats[2].item() / world:.4f} kl {stats[3].item() / world:.4f}" if teacher is not None else ""
                print(f"step {i} loss {loss:.4f}{parts} lr {lrs[0]:.5f}|{lrs[-1]:.5f} tokens/s {toks / dt:,.0f} "
                      f"MFMA-frac(executed FLOP) {toks / dt * fpt_exec / (2.5e15 * world) * 100:.1f}% "
                      f"[reference formula 6N+12LCT: {toks / dt * fpt / (2.5e15 * world) * 100:.1f}%] trained {trained / 1e6:.2f}M", flush=True)
            if trained - last_test > args.test_freq:            # train_encoder.py:371-410
                for name, v in evaluate(model, test_sources, args, world, device).items():
                    if rank == 0:
                        print(f"test_loss/{name} {v:.4f} at {trained / 1e6:.2f}M tokens", flush=True)
                last_test = trained
            if rank == 0 and trained - last_save > args.save_freq:   # train_encoder.py:412-423: keep only the newest
                save(f"_{trained}")
                if last_save > 0:
                    for f in (f"{args.save_name}_{last_save}.pt", f"{args.save_name}_optimizer_{last_save}.pt"):
                        if os.path.exists(f):
                            os.remove(f)
                last_save = trained
        if rank == 0 and args.save_name:
            save("")                                        # train_encoder.py:429-432
    finally:
        close_source()
        dist.destroy_process_group()
    return history


if __name__ == "__main__":
    run(parse_args())
