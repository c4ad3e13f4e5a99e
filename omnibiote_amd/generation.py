"""The state of autoregressive generation: the sampler and what restricts or penalises it, the key/value caches and their positions,
the e4m3 weight snapshot, the device-resident token loop and the result types.  ``OmniBioTA`` (model.py) drives these and re-exports
every name; nothing here imports model.py — ``DecodeLoop`` and the caches reach the model only through the instance they are given.
"""
from __future__ import annotations

import copy
from typing import NamedTuple

import torch

from . import _lib as L
from . import ops
from . import w4quant
from . import w8quant


def _require_hip(t: torch.Tensor, what: str) -> None:
    if not t.is_cuda:
        raise RuntimeError(f"{what}: the OmniBioTE MI355X path needs GPU tensors (got {t.device}); there is no CPU "
                           "fallback in this package. Move the model and inputs to the GPU, e.g. m.to(torch.bfloat16).to('cuda').")
    if t.dtype != torch.bfloat16:
        raise RuntimeError(f"{what}: parameters/activations must be torch.bfloat16 (the reference trains and evaluates "
                           f"in bf16: train_encoder.py:21,170); got {t.dtype}. Call model.to(torch.bfloat16).")
    L.lib()  # raises HipLibraryError if the shared library is missing


def _check_top_p(what, top_p):
    if top_p is not None and not 0 < top_p <= 1:
        raise ValueError(f"{what}: top_p must lie in (0, 1], got {top_p}")


def _check_prompt(what, idx, shape="(B, T0)", min_rows=0):
    """``idx``'s shape, (rows, T0) with T0 >= 1, or a ValueError naming ``OmniBioTA.what``"""
    if idx.dim() != 2 or idx.shape[0] < min_rows:
        raise ValueError(f"OmniBioTA.{what}: idx must be {shape}, got {tuple(idx.shape)}")
    if idx.shape[1] == 0:
        raise ValueError(f"OmniBioTA.{what}: the prompt is empty")
    return idx.shape


def _check_room(what, prompt, max_new_tokens, block_size, longest=False, drafted=0, draft_model=True):
    """ValueError naming ``OmniBioTA.what`` unless ``prompt`` tokens (``longest``: of the longest row), ``max_new_tokens`` new ones and the
    ``drafted`` a speculative round may write beyond them fit ``block_size`` (with a draft model: the smaller of the two models')"""
    if max_new_tokens < 0 or prompt + max_new_tokens + drafted > block_size:
        raise ValueError(f"OmniBioTA.{what}: {prompt} prompt tokens{' (the longest row)' if longest else ''} + {max_new_tokens} new ones"
                         + (f" + k = {drafted} drafted" if drafted else "") + f" exceed block_size = {block_size}"
                         + (" (the smaller of the two models')" if drafted and draft_model else ""))


def _default_pad(pad_token, eos_token):
    """what stands behind a row's last token: ``pad_token``, by default ``eos_token`` if there is one, else 0"""
    return pad_token if pad_token is not None else (eos_token if eos_token is not None else 0)


def _live(n_new, steps, device):
    """bool (B, steps): column i of row b holds one of the row's ``n_new[b]`` tokens"""
    return torch.arange(steps, device=device).view(1, -1) < n_new.view(-1, 1)


def sample_next(logits, temperature=1.0, top_k=None, generator=None, top_p=None):
    """The next token of every row from its (B, vocab) logits: nanoGPT's sampling step.  ``top_k == 1`` or ``temperature == 0`` is the
    argmax; otherwise the logits are divided by the temperature, everything below the row's k-th largest is excluded, and the token
    is drawn from the softmax with ``torch.multinomial`` under ``generator``.  ``top_p`` in (0, 1] (nucleus sampling, after top-k, by
    the rule of ``sampling.sample_reference``): of what is left, walking the distinct values downwards, everything below the first
    value at which the running probability reaches ``top_p`` is excluded too, ties kept whole.  Ordinary torch on any device; returns
    (B,) int64."""
    if logits.dim() != 2:
        raise ValueError(f"sample_next: logits must be (B, vocab), got {tuple(logits.shape)}")
    if top_k is not None and top_k < 1:
        raise ValueError(f"sample_next: top_k must be at least 1, got {top_k}")
    if temperature < 0:
        raise ValueError(f"sample_next: temperature must not be negative, got {temperature}")
    _check_top_p("sample_next", top_p)
    if top_k == 1 or temperature == 0:
        return torch.argmax(logits, dim=-1)
    raw = logits
    logits = logits.float() / temperature
    if top_k is not None:
        v, _ = torch.topk(logits, min(top_k, logits.size(-1)))
        logits = logits.masked_fill(logits < v[:, [-1]], float("-inf"))
    if top_p is not None and top_p < 1:
        # the distinct values' masses from a descending sort, in float64 on the logits as given (the reference's arithmetic)
        x = raw.double().masked_fill(torch.isneginf(logits), float("-inf"))
        sv, _ = torch.sort(x, dim=-1, descending=True)
        csum = torch.exp((sv - sv[:, :1]) / temperature).cumsum(dim=-1)
        end = torch.ones_like(sv, dtype=torch.bool)
        end[:, :-1] = sv[:, :-1] != sv[:, 1:]                            # the last entry of every run of one value
        at = (end & (csum >= top_p * csum[:, -1:])).to(torch.uint8).argmax(dim=-1, keepdim=True)
        logits = logits.masked_fill(x < sv.gather(1, at), float("-inf"))
    probs = torch.softmax(logits, dim=-1)
    return torch.multinomial(probs, num_samples=1, generator=generator).squeeze(1)


class TokenConstraint:
    """``allowed_tokens`` and ``min_new_tokens`` of one generation call, checked and packed once before the prefill (the rule:
    include/omnibiote_hip_constrain.h; in plain torch ``sampling.constrain_reference``).  ``allowed``: bool (V,) or (rows, V) on the
    call's device, or None; ``packed``: the same as ``sampling.pack_token_mask`` makes it; ``hold``: ``eos_token`` while a minimum length is
    asked for, else None; ``min_new``: that length.  ``TokenConstraint.of`` returns None for a call that restricts nothing."""

    @classmethod
    def of(cls, what, allowed_tokens, min_new_tokens, max_new_tokens, eos_token, rows, vocab, device):
        if isinstance(min_new_tokens, bool) or not isinstance(min_new_tokens, int) or not 0 <= min_new_tokens <= max(int(max_new_tokens), 0):
            raise ValueError(f"OmniBioTA.{what}: min_new_tokens must be an integer in [0, max_new_tokens = {max_new_tokens}], got {min_new_tokens!r}")
        if min_new_tokens > 0 and eos_token is None:
            raise ValueError(f"OmniBioTA.{what}: min_new_tokens = {min_new_tokens} holds eos_token back, and there is no eos_token")
        if allowed_tokens is None and min_new_tokens == 0:
            return None
        mask = None
        if allowed_tokens is not None:
            t = allowed_tokens if isinstance(allowed_tokens, torch.Tensor) else torch.as_tensor(allowed_tokens)
            if t.dtype == torch.bool:
                if t.shape not in ((vocab,), (rows, vocab)):
                    raise ValueError(f"OmniBioTA.{what}: a bool allowed_tokens must be ({vocab},) or ({rows}, {vocab}): one row per output row, got "
                                     f"{tuple(t.shape)}")
                mask = t.to(device)
            else:
                if t.dim() == 1 and t.numel() == 0:                     # (an empty list comes as float32)
                    t = t.to(torch.int64)
                if t.dim() != 1 or t.is_floating_point() or t.is_complex():
                    raise ValueError(f"OmniBioTA.{what}: allowed_tokens must be a 1-D sequence of token ids or a bool mask, got {t.dtype} {tuple(t.shape)}")
                if t.numel() > 0 and (int(t.min()) < 0 or int(t.max()) >= vocab):
                    raise ValueError(f"OmniBioTA.{what}: allowed_tokens holds an id outside [0, vocab_size = {vocab})")
                mask = torch.zeros(vocab, dtype=torch.bool, device=device)
                mask[t.to(device=device, dtype=torch.int64)] = True
            if not bool(mask.any(dim=-1).all()):
                raise ValueError(f"OmniBioTA.{what}: allowed_tokens allows nothing" + (" in some row" if mask.dim() == 2 else ""))
            if min_new_tokens > 0 and 0 <= int(eos_token) < vocab:
                other = mask.clone()
                other[..., int(eos_token)] = False
                if not bool(other.any(dim=-1).all()):
                    raise ValueError(f"OmniBioTA.{what}: min_new_tokens = {min_new_tokens} holds eos_token back, and allowed_tokens allows nothing else"
                                     + (" in some row" if mask.dim() == 2 else ""))
        from .sampling import pack_token_mask
        con = cls()
        con.allowed, con.packed = mask, None if mask is None else pack_token_mask(mask)
        con.min_new, con.hold = min_new_tokens, eos_token if min_new_tokens > 0 else None
        return con

    def device_args(self, emitted_by_all=0):
        """the keywords of ``ops.sample_logits`` in a host-driven loop: every running row has emitted ``emitted_by_all`` tokens"""
        return dict(allowed_packed=self.packed, hold_token=self.hold, emitted=None, min_emitted=max(0, self.min_new - emitted_by_all))

    def restrict(self, logits, emitted_by_all=0):
        """``logits`` with the excluded columns at -inf, for the torch sampler"""
        from .sampling import constrain_reference
        return constrain_reference(logits, self.allowed, self.hold, None, max(0, self.min_new - emitted_by_all))


# What restricts a draw reaches ``ops.sample_logits`` / ``ops.spec_verify`` as keywords, and a call that restricts nothing passes none of them:
# the dicts below are empty then, the ops see their defaults and take the unrestricted entry point (a keyword that is given, ``emitted``
# or a ``hold_token`` whose minimum has passed included, selects the constrained one: another kernel instantiation).
def _step_restriction(con, step=0):
    """the restriction keywords of ``ops.sample_logits`` in a host-driven loop whose running rows have emitted ``step`` tokens; ``con``: the
    call's ``TokenConstraint`` or None"""
    return {} if con is None else con.device_args(step)


def _round_restriction(con, counts, device):
    """the restriction keywords of ``OmniBioTA.draft_and_verify`` for one speculative round; ``counts``: what every row has emitted, the
    host's account (sent to the device only while a minimum length holds ``eos_token`` back)"""
    if con is None:
        return {}
    emitted = torch.tensor(counts, dtype=torch.int32, device=device) if con.min_new > 0 else None
    return dict(allowed=con.packed, hold_token=con.hold, emitted=emitted, min_emitted=con.min_new)


def _restriction(allowed, hold_token, emitted, min_emitted, drawn=None):
    """``draft_and_verify``'s four restriction arguments as the keywords of ``ops.spec_verify`` or, ``drawn`` tokens into the round, of the
    draft's ``ops.sample_logits``"""
    if allowed is None and hold_token is None and emitted is None and min_emitted == 0:
        return {}
    return dict(allowed_packed=allowed, hold_token=hold_token, emitted=emitted, min_emitted=min_emitted if drawn is None else max(0, min_emitted - drawn))


class TokenPenalty:
    """``repetition_penalty``, ``presence_penalty`` and ``frequency_penalty`` of one generation call (the rule:
    include/omnibiote_hip_penalty.h; in plain torch ``sampling.penalize_reference``): repetition divides the positive and multiplies the
    negative logits of every token of the row's prompt or output, once per distinct token; presence + frequency * count is subtracted
    from the logits of the tokens the row has generated.  ``TokenPenalty.of`` checks the numbers — ValueError before anything is
    launched — and returns None for a call that penalises nothing; ``bind`` attaches the rows' prompts, (rows, T0) int64 with their
    lengths as (rows,) int32 on the device, and for a host-driven loop the (rows, max_new_tokens) int64 buffer of generated tokens:
    ``record`` writes a step's tokens into it with one device copy and no host read, ``device_args(i)`` is the ``penalty`` of
    ``ops.sample_logits`` at step i and ``apply(logits, i)`` the torch sampler's penalised copy.  ``loop_args`` reads a ``DecodeLoop``'s
    own ``out`` / ``n_new`` instead."""

    @classmethod
    def of(cls, what, repetition_penalty, presence_penalty, frequency_penalty, max_new_tokens):
        from .sampling import penalty_numbers
        for name, v in (("repetition_penalty", repetition_penalty), ("presence_penalty", presence_penalty), ("frequency_penalty", frequency_penalty)):
            if isinstance(v, bool) or not isinstance(v, (int, float)):
                raise ValueError(f"{what}: {name} must be a number, got {v!r}")
        try:
            r, _, pp, fp = penalty_numbers(repetition_penalty, presence_penalty, frequency_penalty)
        except ValueError as e:
            raise ValueError(f"{what}: repetition_penalty must be positive and all three penalties finite in fp32 ({e})") from None
        if r == 1.0 and pp == 0.0 and fp == 0.0:
            return None
        if int(max_new_tokens) > L.PENALTY_MAX_GEN:
            raise ValueError(f"{what}: penalties count a row's generated tokens up to {L.PENALTY_MAX_GEN}, got max_new_tokens = {max_new_tokens}")
        pen = cls()
        pen.repetition, pen.presence, pen.frequency, pen.max_new = r, pp, fp, int(max_new_tokens)
        pen.prompt = pen.prompt_len = pen.gen = None
        return pen

    def bind(self, prompt, lengths=None, own_buffer=True):
        """the rows' prompts ``prompt`` (rows, T0) int64 and their lengths (a host sequence; None: T0 each) — copied, so a loop that is
        prefilled again can rewrite them in place (``rebind``)"""
        rows, t0 = prompt.shape
        self.prompt = prompt.to(torch.int64).contiguous().clone()
        self.prompt_len = torch.tensor([t0] * rows if lengths is None else [int(n) for n in lengths], dtype=torch.int32).to(prompt.device)
        self.gen = torch.zeros((rows, self.max_new), dtype=torch.int64, device=prompt.device) if own_buffer else None
        return self

    def rebind(self, prompt, lengths=None):
        """another prompt into the buffers ``bind`` made: the addresses a captured graph holds stay valid"""
        rows, width = self.prompt.shape
        if prompt.dim() != 2 or prompt.shape[0] != rows or prompt.shape[1] > width:
            raise ValueError(f"TokenPenalty.rebind: the prompt must be ({rows}, at most {width}), got {tuple(prompt.shape)}")
        t0 = prompt.shape[1]
        self.prompt[:, :t0].copy_(prompt)
        self.prompt_len.copy_(torch.tensor([t0] * rows if lengths is None else [int(n) for n in lengths], dtype=torch.int32))

    def record(self, step, tokens):
        self.gen[:, step].copy_(tokens)

    def _numbers(self):
        return dict(repetition=self.repetition, presence=self.presence, frequency=self.frequency)

    def device_args(self, step):
        """the ``penalty`` of ``ops.sample_logits`` in a host-driven loop: every row has ``step`` recorded tokens"""
        return ops.Penalty(self.prompt, self.prompt_len, self.gen, step, **self._numbers())

    def loop_args(self, out, n_new):
        """the same for a ``DecodeLoop``: its ``out`` and ``n_new`` are the generated lists and their counts — addresses only"""
        return ops.Penalty(self.prompt, self.prompt_len, out, n_new, **self._numbers())

    def apply(self, logits, step):
        """``logits`` with the history's columns rewritten (bf16), for the torch sampler"""
        from .sampling import penalize_reference
        return penalize_reference(logits, self.prompt, self.prompt_len, self.gen, step, **self._numbers())


def _next_tokens(what, logits, temperature, top_k, top_p, generator, u, con=None, step=0, pen=None):
    """one step's tokens: ``sample_next`` (u is None: the torch sampler), or one launch of the device sampler against this step's
    uniforms ``u`` (B,) — False: greedy, nothing was drawn.  ``con``: the call's ``TokenConstraint`` or None; ``step``: the tokens every
    running row has emitted so far; ``pen``: the call's ``TokenPenalty`` or None (the caller records the tokens it keeps)"""
    if u is None:
        if pen is not None:
            logits = pen.apply(logits, step)
        return sample_next(logits if con is None else con.restrict(logits, step), temperature, top_k, generator, top_p)
    if not (logits.is_cuda and logits.dtype == torch.bfloat16):
        raise ValueError(f"OmniBioTA.{what}: sampler='device' needs bf16 logits on the GPU, got {logits.dtype} on {logits.device}")
    return ops.sample_logits(logits, None if u is False else u, temperature, top_k, top_p, penalty=None if pen is None else pen.device_args(step),
                             **_step_restriction(con, step))


def _device_uniforms(sampler, steps, batch, temperature, top_k, device, generator):
    """None for the torch sampler; for the device sampler the uniforms of a whole call, (steps, batch) drawn once (False when the
    setting is greedy and nothing is drawn)"""
    if sampler == "torch":
        return None
    if top_k == 1 or temperature == 0:
        return [False] * steps
    return torch.rand((steps, batch), device=device, generator=generator)


def _check_lengths(what, lengths, batch, t0):
    """``lengths`` as a list of ``batch`` ints in [1, t0], or a ValueError naming ``what``"""
    try:
        lens = [int(n) for n in (lengths.tolist() if isinstance(lengths, torch.Tensor) else lengths)]
    except TypeError:
        raise ValueError(f"OmniBioTA.{what}: lengths must be a sequence of {batch} integers") from None
    if len(lens) != batch:
        raise ValueError(f"OmniBioTA.{what}: {len(lens)} lengths for a batch of {batch} rows")
    if min(lens) < 1 or max(lens) > t0:
        raise ValueError(f"OmniBioTA.{what}: every length must lie in [1, T0 = {t0}], got {lens}")
    return lens


def ragged_output(idx, lengths, tokens, valid, pad_token):
    """The result of a ragged ``generate``: row b is its prompt ``idx[b, :lengths[b]]``, then the tokens of the steps it was still
    running at — ``tokens[b, i]`` where ``valid[b, i]``, a prefix of the row — then ``pad_token``.  idx (B, T0) int64, lengths (B,)
    integers, tokens (B, S) int64, valid (B, S) bool.  Returns (out (B, max(lengths) + S) int64, out_lengths (B,) int64).  Ordinary torch
    on any device, no host synchronisation beyond the width (a host integer the caller already has)."""
    b, steps = tokens.shape
    lens = torch.as_tensor(lengths, dtype=torch.int64).to(idx.device).view(b, 1)
    longest = max(lengths.tolist() if isinstance(lengths, torch.Tensor) else lengths)
    n_new = valid.sum(dim=1, keepdim=True).to(torch.int64)
    col = torch.arange(longest + steps, device=idx.device).view(1, -1)
    out = torch.full((b, longest + steps), int(pad_token), dtype=torch.int64, device=idx.device)
    out[:, :longest] = torch.where(col[:, :longest] < lens, idx[:, :longest], out[:, :longest])
    if steps > 0:
        at = col - lens                                                 # the step whose token stands in this column
        new = tokens.gather(1, at.clamp(0, steps - 1))
        out = torch.where((at >= 0) & (at < n_new), new, out)
    return out, (lens + n_new).view(b)


class CachePositions:
    """Where a key/value cache of ``batch`` rows and ``max_len`` positions stands, and the only code that moves it: host integers and one
    device tensor, no buffer, so it can be built and driven without a GPU (``KVCache`` adds the buffers).

    ``pos``: the positions filled, a host integer.  Uniform mode (``positions is None``): the same for every row.  After a prefill with
    ``lengths`` the rows stand at different positions: ``positions`` is then an int32 (B,) device tensor, row b's next position (the
    kernels read it there; a negative value parks a finished row: it stores nothing and attends to nothing), ``pos`` the host's upper
    bound on it — the longest row — and ``min_pos`` a host-side lower bound on the shortest row that is not parked (0: unknown; only
    ``rewind`` reads it).  ``reset``, ``advance``, ``park``, ``rewind`` and ``rewind_rows`` are the only writers of the three — and, for a
    ``DecodeLoop``, ``advanced_on_device``: there the loop's kernel (obte_gen_advance) is the writer of the device tensor, in place, and
    this class moves the host bounds alone."""

    dtype = "bf16"   # what the buffers behind the positions hold (KVCache sets it): no operation here touches a cache byte

    def __init__(self, batch, max_len):
        self.batch, self.max_len = int(batch), int(max_len)
        self.reset(0)

    @property
    def max_pos(self):
        """the host's bound on ``positions`` (0 in uniform mode)"""
        return self.pos if self.positions is not None else 0

    def reset(self, pos, positions=None, min_pos=0):
        """The state after a prefill, or set by hand: ``pos`` positions filled; ``positions`` a ready int32 (B,) tensor on the kernels'
        device with ``pos`` its upper bound, ``min_pos`` a lower bound on its active rows.  Host assignments only, nothing is copied."""
        self.pos, self.positions, self.min_pos = int(pos), positions, int(min_pos)

    def require_room(self, what, n, detail=False):
        """ValueError in ``OmniBioTA.what``'s name unless ``n`` more positions fit"""
        if self.pos + n > self.max_len:
            tail = f": {n} more from {self.pos} do not fit" if detail else ""
            raise ValueError(f"OmniBioTA.{what}: the cache's {self.max_len} positions are full{tail}")

    def advance(self, n):
        """``n`` more positions are filled in every row that is not parked.  ``positions`` becomes a new tensor (launches already queued
        read the old one); the update is queued on the stream and nothing waits for it."""
        self.pos += n
        if self.positions is not None:
            self.positions = torch.add(self.positions, self.positions >= 0, alpha=n)   # int32 + n * bool: int32; parked rows (< 0) stay
            self.min_pos += n

    def advanced_on_device(self, n):
        """``n`` more positions were filled, and ``positions`` has been moved (and finished rows parked) in place by a kernel on the
        stream: only the host bounds follow here.  ``positions`` stays the same tensor — launches recorded against its address, a
        captured graph's among them, keep reading the live state.  Rows mode only."""
        if self.positions is None:
            raise ValueError("KVCache.advanced_on_device: the cache is in uniform mode (no positions tensor for a kernel to move)")
        self.pos += n
        self.min_pos += n

    def park(self, done):
        """Park the rows where ``done`` (bool (B,)) holds: they store nothing and read nothing from here on.  Rows mode only."""
        self.positions = torch.where(done, torch.full_like(self.positions, -1), self.positions)

    def rewind(self, n):
        """Step back by ``n`` positions: ``pos -= n``, and after a prefill with ``lengths`` the rows not parked step back by ``n`` each.
        This is what a caller does with rejected draft tokens: ``extend`` the cache by the drafted block, keep the accepted prefix, rewind
        the rest.  No kernel of the library runs and nothing is cleared — positions beyond ``pos`` are never read, and the next tokens
        overwrite them.  With ``positions`` set, the one elementwise update of that tensor is queued on the stream and the host does not
        wait for it: a draft-and-verify loop (extend by k, rewind by fewer) never synchronises here.  ValueError if a row would be left
        with fewer than one position."""
        n = int(n)
        if n < 0:
            raise ValueError(f"KVCache.rewind: n must not be negative, got {n}")
        if self.positions is None:
            if self.pos - n < 1:
                raise ValueError(f"KVCache.rewind: {n} positions back from {self.pos} leaves fewer than one")
            self.pos -= n
            return
        # The shortest active row, bounded from below on the host (reset sets ``min_pos``, advance and this move it; parked rows only leave
        # it too low, which is safe): while the bound allows the step nothing waits for the device.  Only where it does not — or on a
        # cache whose positions were set without a bound — are the positions themselves read, which synchronises.
        low = self.min_pos
        if self.pos - n < 1:
            raise ValueError(f"KVCache.rewind: {n} positions back leaves a row with fewer than one")
        if low - n < 1:
            active = [p for p in self.positions.tolist() if p >= 0]
            low = min(active) if active else n + 1
            if low - n < 1:
                raise ValueError(f"KVCache.rewind: {n} positions back leaves a row with fewer than one")
        self.positions = self.positions - n * (self.positions >= 0).to(torch.int32)   # (parked rows, < 0, stay as they are)
        self.min_pos = low - n
        self.pos -= n

    def rewind_rows(self, back, now=None):
        """Step every row back by its own count: ``back`` is a host sequence of B non-negative ints, what a draft-and-verify loop knows
        once it has read how many drafted tokens stand in each row.  Rows not parked step back by ``back[b]``, parked rows stay parked;
        ``pos`` becomes the new maximum over the rows not parked and ``min_pos`` their new minimum, both exact.  Rows mode only.
        ``now``: the rows' positions as the caller knows them, a host sequence of B ints (negative: parked) — with it nothing is read
        from the device and nothing waits; without it ``positions`` is read, which synchronises.  As in ``rewind`` no kernel of the
        library runs, nothing is cleared, and the one elementwise update of ``positions`` is queued on the stream.  ValueError if a
        row would keep fewer than one position, or in uniform mode."""
        if self.positions is None:
            raise ValueError("KVCache.rewind_rows: the cache is in uniform mode (no prefill with lengths): use rewind")
        try:
            back = [int(n) for n in (back.tolist() if isinstance(back, torch.Tensor) else back)]
        except TypeError:
            raise ValueError(f"KVCache.rewind_rows: back must be a sequence of {self.batch} integers") from None
        if len(back) != self.batch:
            raise ValueError(f"KVCache.rewind_rows: {len(back)} counts for a cache of {self.batch} rows")
        if min(back) < 0:
            raise ValueError(f"KVCache.rewind_rows: counts must not be negative, got {back}")
        now = self.positions.tolist() if now is None else [int(p) for p in now]
        if len(now) != self.batch:
            raise ValueError(f"KVCache.rewind_rows: {len(now)} positions for a cache of {self.batch} rows")
        left = [p - n for p, n in zip(now, back) if p >= 0]
        if left and min(left) < 1:
            raise ValueError(f"KVCache.rewind_rows: {back} positions back from {now} leaves a row with fewer than one")
        step = torch.tensor(back, dtype=torch.int32).to(self.positions.device, non_blocking=True)
        self.positions = self.positions - step * (self.positions >= 0).to(torch.int32)   # (parked rows, < 0, stay as they are)
        if left:                                                        # (every row parked: the bounds stay, nothing reads them)
            self.pos, self.min_pos = max(left), min(left)


class KVCache(CachePositions):
    """The rotated keys and the values of every layer of ``model`` for ``batch`` sequences of up to ``max_len`` positions
    (default and at most ``config.block_size``): one buffer per layer (include/omnibiote_hip.h, obte_kv_cache_bytes), the workspaces of
    a decode step and of ``extend``, and where the rows stand (``CachePositions``).  ``OmniBioTA.prefill`` starts it over (nothing is
    cleared: positions beyond ``pos`` are never read), ``decode_step`` advances it by one token per row, ``extend`` by several,
    ``rewind`` steps back.

    ``dtype``: "bf16" (the default) or "fp8" — keys and values stored as OCP e4m3 with one power-of-two scale per (row, head, position)
    vector (include/omnibiote_hip_kv8.h, kvquant.py): 2 (hs + 4) bytes per cached vector instead of 4 hs.  ``prefill`` (unchunked),
    ``decode_step`` and ``generate`` run on either; several new positions per row in one call (``extend``, ``prefill(chunk=)``,
    ``generate_speculative``) need a bf16 cache and raise NotImplementedError on an fp8 one."""

    def __init__(self, model, batch, max_len=None, dtype="bf16"):
        if dtype not in ("bf16", "fp8"):
            raise ValueError(f"KVCache: dtype must be 'bf16' or 'fp8', got {dtype!r}")
        cfg = model.config
        if not cfg.autoregressive:
            raise ValueError("KVCache: the model is not autoregressive (config.autoregressive): an encoder has no next token")
        max_len = cfg.block_size if max_len is None else int(max_len)
        if not 1 <= max_len <= cfg.block_size:
            raise ValueError(f"KVCache: max_len {max_len} outside [1, block_size = {cfg.block_size}]")
        if batch < 1:
            raise ValueError(f"KVCache: batch must be at least 1, got {batch}")
        wte = model.transformer.wte.weight
        _require_hip(wte, "KVCache")
        super().__init__(batch, max_len)
        hs = cfg.n_embd // cfg.n_head
        self.dtype = dtype
        new = ops.kv8_cache_buffer if dtype == "fp8" else ops.kv_cache_buffer
        self.layers = [new(self.batch, max_len, cfg.n_head, hs, wte.device) for _ in model.transformer.h]
        self.decode_ws = ops.block_decode_workspace(self.batch, cfg.n_embd, cfg.n_head, wte.device)
        self.extend_ws = None   # OmniBioTA.extend's workspace: allocated by the first call, replaced when a call needs more bytes


class SharedPrefixCache(CachePositions):
    """The cache of ``prompts`` prompts with ``samples`` samples drawn from each (include/omnibiote_hip_shared.h): ``batch = prompts *
    samples`` rows, row p * samples + g the g-th sample of prompt p.  Per layer a PREFIX buffer of ``prompts`` rows and ``prefix_len``
    positions, which ``OmniBioTA.prefill`` fills once per prompt and every row of the group reads, and a SUFFIX buffer of ``batch`` rows
    and ``max_new`` slots for the rows' own tokens, both ``ops.kv_cache_buffer``'s; ``layers[i]`` is the pair.  ``pos`` counts absolute
    positions as on a ``KVCache`` (a token's RoPE row is ``pos``); ``n_prefix`` is the prompt length the last prefill left, and slot
    ``pos - n_prefix`` of the suffix takes the next token.  ``group = samples``.

    Uniform mode only (every prompt of a call has the same length): ``park`` and ``rewind_rows`` raise, and ``rewind`` does not step
    into the prefix.  bf16 only.  ``prefill`` (without ``lengths`` / ``chunk``), ``decode_step`` and ``generate(num_samples=)`` run on
    it; ``extend`` and the speculative loop raise NotImplementedError."""

    def __init__(self, model, prompts, samples, prefix_len, max_new):
        cfg = model.config
        if not cfg.autoregressive:
            raise ValueError("SharedPrefixCache: the model is not autoregressive (config.autoregressive): an encoder has no next token")
        prompts, samples, prefix_len, max_new = int(prompts), int(samples), int(prefix_len), int(max_new)
        if prompts < 1 or samples < 1:
            raise ValueError(f"SharedPrefixCache: prompts and samples must be at least 1, got {prompts} and {samples}")
        if prefix_len < 1 or max_new < 1 or prefix_len + max_new > cfg.block_size:
            raise ValueError(f"SharedPrefixCache: prefix_len {prefix_len} and max_new {max_new} must be at least 1 and together at most "
                             f"block_size = {cfg.block_size}")
        wte = model.transformer.wte.weight
        _require_hip(wte, "SharedPrefixCache")
        super().__init__(prompts * samples, prefix_len + max_new)
        self._shape(prompts, samples, prefix_len, max_new)
        hs = cfg.n_embd // cfg.n_head
        self.layers = [(ops.kv_cache_buffer(prompts, prefix_len, cfg.n_head, hs, wte.device),
                        ops.kv_cache_buffer(self.batch, max_new, cfg.n_head, hs, wte.device)) for _ in model.transformer.h]
        self.decode_ws = ops.block_decode_shared_workspace(prompts, samples, cfg.n_embd, cfg.n_head, wte.device)
        self.extend_ws = None

    def _shape(self, prompts, samples, prefix_len, max_new):
        """host integers only (the position logic below reads nothing else)"""
        self.prompts, self.group, self.prefix_len, self.max_new = prompts, samples, prefix_len, max_new
        self.n_prefix = 0   # set by prefill

    def require_room(self, what, n, detail=False):
        """ValueError in ``OmniBioTA.what``'s name unless ``n`` more suffix slots are free"""
        if self.pos - self.n_prefix + n > self.max_new:
            tail = f": {n} more from slot {self.pos - self.n_prefix} do not fit" if detail else ""
            raise ValueError(f"OmniBioTA.{what}: the shared-prefix cache's {self.max_new} suffix slots are full{tail}")

    def park(self, done):
        raise ValueError("SharedPrefixCache.park: a shared-prefix cache is in uniform mode (rows are not parked)")

    def rewind_rows(self, back, now=None):
        raise ValueError("SharedPrefixCache.rewind_rows: a shared-prefix cache is in uniform mode: use rewind")

    def rewind(self, n):
        """``CachePositions.rewind`` within the rows' own tokens: at least one of them stays (the prefix is the prompt, not a sample)"""
        n = int(n)
        if n < 0:
            raise ValueError(f"SharedPrefixCache.rewind: n must not be negative, got {n}")
        if self.pos - n < self.n_prefix + 1:
            raise ValueError(f"SharedPrefixCache.rewind: {n} positions back from {self.pos} steps into the shared prefix of {self.n_prefix}")
        self.pos -= n


class PagedPositions(CachePositions):
    """Where the rows of a paged cache stand and which pages they hold (include/omnibiote_hip_paged.h): a ``CachePositions`` that is always
    in rows mode, built on a ``paged.PageBook`` — the free list, the table as a CPU tensor and an exact host mirror of every row's
    position, -1 for a parked row.  No buffer: it can be built and driven without a GPU (``device=None``: ``table`` and ``positions`` are
    then CPU tensors); ``PagedKVCache`` adds the pools.

    This class is the only writer of the table and the mirror.  ``assign(row, n_positions)`` gives a row the pages that cover that many
    positions (ValueError when the free list cannot), ``release(row)`` takes them back, clears the row's entries and parks it,
    ``park_rows(rows)`` parks rows that keep their pages, ``pages_in_use`` counts.  ``table`` (int32 (batch, ceil(max_len / 64)), -1: no
    page) and ``positions`` (int32 (batch,)) are what the kernels read; a change of the book reaches them as one small copy each, made
    when they are next read — so any number of changes between two steps cost one copy.  Each copy is a new tensor: launches already
    queued read the old one.  ``pos`` = ``max_pos`` is the largest mirrored position.

    ``park(done_tensor)``, ``rewind``, ``rewind_rows``, ``reset`` and ``advanced_on_device`` raise: the host must know where every row
    stands, and those move rows by device values or by several positions."""

    def __init__(self, batch, n_pages, max_len, free_order=None, device=None):
        from .paged import PageBook
        self.book = PageBook(batch, n_pages, max_len, free_order)
        self.batch, self.max_len, self.n_pages, self.device = self.book.batch, self.book.max_len, self.book.n_pages, device
        self.pos = self.min_pos = 0
        self._positions = self._table = None
        self._stale_positions = self._stale_table = True

    # ---- what the kernels read -----------------------------------------------------------------------------------------------------------
    def _put(self, t):
        return t.clone() if self.device is None else t.to(self.device)

    @property
    def positions(self):
        if self._stale_positions:
            self._positions, self._stale_positions = self._put(torch.tensor(self.book.row_pos, dtype=torch.int32)), False
        return self._positions

    @positions.setter
    def positions(self, value):                                         # (CachePositions.advance: the device's own + 1, the mirror's twin)
        self._positions, self._stale_positions = value, False

    @property
    def table(self):
        if self._stale_table:
            self._table, self._stale_table = self._put(self.book.table), False
        return self._table

    def _moved(self, table=False):
        """the book has changed: the bounds follow now, the kernels' copies when they are next read"""
        active = [p for p in self.book.row_pos if p >= 0]
        self.pos, self.min_pos = max(active, default=0), min(active, default=0)
        self._stale_positions = True
        self._stale_table = self._stale_table or table

    # ---- the writers -----------------------------------------------------------------------------------------------------------------------
    @property
    def pages_in_use(self):
        return self.book.pages_in_use

    def assign(self, row, n_positions):
        """row ``row`` gets the pages that cover ``n_positions`` positions (it keeps those it has); ValueError when the free list cannot"""
        if self.book.assign(row, n_positions):
            self._moved(table=True)

    def release(self, row):
        """row ``row``'s pages go back to the free list, its table entries are cleared and it is parked"""
        self.book.release(row)
        self._moved(table=True)

    def park_rows(self, rows):
        """park the rows of the host list ``rows``: they store nothing and read nothing from here on, and keep their pages until released"""
        self.book.park_rows(rows)
        self._moved()

    def start_rows(self, rows, lengths, shared=None):
        """``prefill``'s bookkeeping: row rows[i] starts over behind a prompt of lengths[i] tokens, with pages for them (those it holds
        count).  ``shared[i]`` (``prefill(shared_pages=)``): the pages that hold row rows[i]'s first 64 * len(shared[i]) positions
        already — the row names them (``PageBook.assign_shared``: it must hold no page, and 64 * len(shared[i]) < lengths[i]) and gets
        pages of its own for the rest.  ValueError, with nothing changed, for a bad ``shared`` or when the free list cannot cover every
        row: only the pages that must come from the free list count, after the shared pages that lie on it (released, still valid) are
        taken off it."""
        from .paged import pages_for
        rows, lengths = [int(r) for r in rows], [int(n) for n in lengths]
        shared = self.check_shared(rows, lengths, shared)
        revived = {p for pages in shared for p in pages if self.book.refs[p] == 0}
        more = sum(max(0, pages_for(n) - len(self.book.row_pages[r]) - len(pages)) for r, n, pages in zip(rows, lengths, shared))
        if more > len(self.book.free) - len(revived):
            raise ValueError(f"PagedKVCache: the prompts of rows {list(rows)} need {more} more pages and {len(self.book.free) - len(revived)} of "
                             f"{self.n_pages} are free")
        for r, pages in zip(rows, shared):
            if pages:
                self.book.assign_shared(r, pages)
        for r, n in zip(rows, lengths):
            self.book.assign(r, n)
            self.book.place(r, n)
        self._moved(table=True)

    def check_shared(self, rows, lengths, shared):
        """``shared`` as ``start_rows`` takes it, one list of ints per row, or a ValueError that changes nothing: a row that still holds
        pages, a page outside the pool, pages that cover a whole prompt (64 * len(shared[i]) >= lengths[i])"""
        from .paged import KV_PAGE
        shared = [[] for _ in rows] if shared is None else [list(p) for p in shared]
        if len(shared) != len(rows):
            raise ValueError(f"PagedKVCache: {len(shared)} lists of shared pages for {len(rows)} rows")
        for i, (r, n) in enumerate(zip(rows, lengths)):
            if shared[i]:
                _, shared[i] = self.book.check_shared(r, shared[i])
                if KV_PAGE * len(shared[i]) >= n:
                    raise ValueError(f"PagedKVCache: row {r}: {len(shared[i])} shared pages cover the whole prompt of {n} tokens (at least one is computed)")
        return shared

    def prepare_step(self):
        """before a decode step is launched: every active row whose position opens a new page gets one (ValueError when none is left)"""
        if self.book.grow_for_step():
            self._moved(table=True)

    def advance(self, n):
        """one more position in every row that is not parked: on the device as ``CachePositions.advance``, and in the mirror"""
        if n != 1:
            raise ValueError(f"PagedKVCache.advance: a paged cache takes one new position per row at a time, got {n}")
        super().advance(1)
        self.book.step()
        active = [p for p in self.book.row_pos if p >= 0]
        self.pos, self.min_pos = max(active, default=0), min(active, default=0)

    def _host_only(self, what):
        raise ValueError(f"PagedKVCache.{what}: the host must know where every row of a paged cache stands: use assign, release, park_rows and "
                         "prefill(rows=)")

    def reset(self, pos, positions=None, min_pos=0):
        self._host_only("reset")

    def advanced_on_device(self, n):
        self._host_only("advanced_on_device")

    def park(self, done):
        self._host_only("park")

    def rewind(self, n):
        self._host_only("rewind")

    def rewind_rows(self, back, now=None):
        self._host_only("rewind_rows")


class PagedKVCache(PagedPositions):
    """The rotated keys and the values of every layer of ``model`` for ``batch`` rows in a pool of ``n_pages`` pages of 64 positions
    (include/omnibiote_hip_paged.h): memory is sized by what the rows hold together, not by ``batch`` times the longest row, and the pages
    and the slot of a finished row serve the next prompt while the others go on.  Per layer one pool (``ops.kv_paged_buffer``); the table,
    the free list and the rows' positions are ``PagedPositions``'s; ``max_len`` (default and at most ``config.block_size``) bounds one row.

    ``OmniBioTA.prefill(idx, cache, lengths=, rows=)`` starts the rows of the host list ``rows`` over (default: all) and leaves the others
    alone; ``decode_step`` gives every active row whose position opens a new page one from the free list, then steps;
    ``OmniBioTA.generate_many`` is the loop that admits, steps and releases.  ``free_order``: the order in which pages are first handed out.

    ``dtype``: "bf16" (the default) or "fp8" — the pools hold OCP e4m3 codes with one power-of-two scale per head vector
    (include/omnibiote_hip_paged8.h, ``ops.kv8_paged_buffer``): ``KVCache(dtype="fp8")``'s vectors in pages, 2 (hs + 4) bytes each instead
    of 4 hs, so the same ``n_pages`` take about half the bytes.  The table, the free list and the positions do not depend on it.

    Not built, each refused before anything is launched, for either dtype: several new positions per row over pages (``extend``,
    ``prefill(chunk=)``, ``draft_and_verify`` and the speculative loop); e4m3 weights (``weights=``); the device-resident loop and graph
    capture (``DecodeLoop``); copy-on-write and sharing of generated (non-prompt) pages; preemption or swapping of running rows.

    Pages shared between rows (bf16 only): ``prefill(..., shared_pages=)`` lets a row name pages another row has filled with the same
    prompt tokens and computes only the rest of its prompt against them (include/omnibiote_hip_paged_extend.h); ``PageBook`` counts the
    rows that name a page and frees it with the last one; ``generate_many(share_prefix=True)`` finds the pages (``paged.PrefixIndex``)."""

    def __init__(self, model, batch, n_pages, max_len=None, free_order=None, dtype="bf16"):
        if dtype not in ("bf16", "fp8"):
            raise ValueError(f"PagedKVCache: dtype must be 'bf16' or 'fp8', got {dtype!r}")
        cfg = model.config
        if not cfg.autoregressive:
            raise ValueError("PagedKVCache: the model is not autoregressive (config.autoregressive): an encoder has no next token")
        max_len = cfg.block_size if max_len is None else int(max_len)
        if not 1 <= max_len <= cfg.block_size:
            raise ValueError(f"PagedKVCache: max_len {max_len} outside [1, block_size = {cfg.block_size}]")
        if batch < 1 or n_pages < 1:
            raise ValueError(f"PagedKVCache: batch and n_pages must be at least 1, got {batch} and {n_pages}")
        wte = model.transformer.wte.weight
        _require_hip(wte, "PagedKVCache")
        super().__init__(batch, n_pages, max_len, free_order, wte.device)
        hs = cfg.n_embd // cfg.n_head
        self.dtype = dtype
        new = ops.kv8_paged_buffer if dtype == "fp8" else ops.kv_paged_buffer
        self.layers = [new(self.n_pages, cfg.n_head, hs, wte.device) for _ in model.transformer.h]
        self.decode_ws = ops.block_decode_workspace(self.batch, cfg.n_embd, cfg.n_head, wte.device)
        self.extend_ws = None


def _refuse_paged(what, cache, why="over which one new position per row attends at a time (prefill, decode_step, generate_many)"):
    """NotImplementedError in ``OmniBioTA.what``'s name on a paged cache: before anything is launched or any state changes"""
    if isinstance(cache, PagedPositions):
        raise NotImplementedError(f"OmniBioTA.{what}: the cache is a paged cache (PagedKVCache), {why}; this call needs a KVCache")


class QuantizedWeights:
    """``model``'s decode-step weights as OCP e4m3 with one power-of-two scale per output row (include/omnibiote_hip_w8.h, w8quant.py):
    what ``prefill``, ``decode_step``, ``generate`` and ``DecodeLoop`` take as ``weights=``.  Per block, in the order c_attn, attention
    c_proj, c_fc, MLP c_proj: ``codes[i]`` (four uint8 (N, K) tensors in w8quant's stored order), ``scales[i]`` (four fp32 (N,)) and
    ``dequantized[i]`` (the four bf16 weights those codes stand for); ``head_codes``, ``head_scales`` and ``head_dequantized`` the same
    three things for ``lm_head.weight``.  The embedding ``wte`` and the LayerNorm weights are read from the model as ever.

    A cached step of at most ``ops.small_m_max`` rows reads the codes — half the bytes — and computes, bit for bit, the bf16 step on the
    dequantised weights; everything else (the prompt, a larger batch) runs the existing kernels on the dequantised weights, so prompt and
    continuation see ONE model: ``dequantized_model()``.

    A snapshot: it remembers every source parameter's ``data_ptr()`` and ``_version``, and every use raises ValueError ("quantize_weights
    again") once a parameter was updated or moved.  It holds 3 bytes per parameter (codes and the bf16 copy) beside the model's 2;
    serving from the codes alone, without the bf16 copies, is not built.

    ``format="mxfp4"`` (``.format`` says which): OCP MXFP4 instead (include/omnibiote_hip_w4.h, w4quant.py) — ``codes[i]`` uint8 (N, K / 2), two
    e2m1 codes per byte in w4quant's stored order, ``scales[i]`` uint8 (N, K / 32), one e8m0 power of two per 32 elements of a row; the
    same attributes under the same names, the same contract, a quarter of the bytes and a sixteenth per cached step, and about 2.53 bytes
    per parameter held beside the model's 2.  Any other format: ValueError."""

    FORMATS = {"e4m3": w8quant, "mxfp4": w4quant}

    def __init__(self, model, format="e4m3"):
        if format not in self.FORMATS:
            raise ValueError(f"quantize_weights: format must be one of {', '.join(map(repr, self.FORMATS))}, got {format!r}")
        self.format, self._quant = format, self.FORMATS[format]
        self.model = model
        self._sources = []
        self.codes, self.scales, self.dequantized, self._params = [], [], [], []
        for block in model.transformer.h:
            p = model._block_params(block)
            c, s, d = zip(*(self._take(w) for w in (p[1], p[2], p[4], p[5])))
            self.codes.append(c); self.scales.append(s); self.dequantized.append(d)
            self._params.append((p[0], d[0], d[1], p[3], d[2], d[3]))
        self.head_codes, self.head_scales, self.head_dequantized = self._take(model.lm_head.weight)

    def _take(self, param):
        if param.dtype != torch.bfloat16:
            raise ValueError(f"quantize_weights: the weights must be torch.bfloat16, got {param.dtype}: call model.to(torch.bfloat16)")
        self._sources.append((param, param.data_ptr(), param._version))
        with torch.no_grad():
            codes, scales = self._quant.quantize_weight(param.detach())
            return codes, scales, self._quant.dequantize_weight(codes, scales)

    def check(self, model, what):
        """ValueError in ``what``'s name unless this is ``model``'s snapshot and every source parameter is where and what it was"""
        if model is not self.model:
            raise ValueError(f"{what}: weights= is the snapshot of another model: call quantize_weights again on this one")
        for p, ptr, version in self._sources:
            if p.data_ptr() != ptr or p._version != version:
                raise ValueError(f"{what}: a parameter was updated or moved since model.quantize_weights(): call quantize_weights again")

    def block_params(self, index):
        """block ``index``'s six parameters with the four matrices dequantised (the LayerNorm weights are the model's own)"""
        return self._params[index]

    def dequantized_model(self):
        """A deep copy of the model whose four matrices per block and readout are the dequantised ones: the bf16 model that ``weights=``
        computes, and the tests' yardstick.  Everything else (``wte``, the LayerNorm weights) is copied as it is."""
        m = copy.deepcopy(self.model)
        for p, src in zip(m.parameters(), self.model.parameters()):    # (a deep copy of a Parameter drops the muP tag set_base_shapes gave it)
            if hasattr(src, "infshape") and not hasattr(p, "infshape"):
                p.infshape = copy.deepcopy(src.infshape)
        with torch.no_grad():
            for block, d in zip(m.transformer.h, self.dequantized):
                for w, dq in zip((block.attn.c_attn.weight, block.attn.c_proj.weight, block.mlp.c_fc.weight, block.mlp.c_proj.weight), d):
                    w.copy_(dq)
            m.lm_head.weight.copy_(self.head_dequantized)
        return m


def _checked_weights(model, what, weights):
    """``weights=`` of a generation call: a QuantizedWeights of this model, still current (ValueError otherwise)"""
    if not isinstance(weights, QuantizedWeights):
        raise ValueError(f"{what}: weights must be what model.quantize_weights() returns, got {type(weights).__name__}")
    weights.check(model, what)


def _refuse_weights(what, weights, why):
    """NotImplementedError in ``OmniBioTA.what``'s name when e4m3 weights are given: before anything is launched or any state changes"""
    if weights is not None:
        raise NotImplementedError(f"OmniBioTA.{what}: weights= (e4m3 weights, QuantizedWeights) {why}; they serve prefill, decode_step, generate and "
                                  "DecodeLoop on a KVCache")


class DecodeLoop:
    """The token loop of ``generate`` with its state on the device: ``model`` stepping a prefilled ``KVCache`` (bf16 or fp8) for up to
    ``max_steps`` tokens per row with no value passing through the host, so that one step is the same sequence of launches with the
    same arguments every time — and, with ``capture=True``, one replay of a captured graph.

    The loop owns buffers whose addresses never change: ``logits`` (B, V) bf16, ``sampled`` and ``token`` (B,) int64, ``u`` (B,) fp32,
    ``x`` (B, C) bf16, ``count`` and ``n_new`` (B,) int32, ``out`` (B, max_steps) int64; the rows' positions are ``cache.positions``,
    moved in place (a cache in uniform mode is put into rows mode here, every row at ``cache.pos``).  One step — the body — is: every
    block's rows-form cached step on ``x`` at ``positions`` under the FIXED bound ``cache.max_len - 1``, ``ln_f``, the readout into
    ``logits``, ``ops.sample_logits`` into ``sampled``, and ``ops.gen_advance``, which records the tokens, parks the rows that drew
    ``eos_token``, fetches the next uniforms and embeds the next tokens (include/omnibiote_hip_loop.h): one launch fewer than a
    ``decode_step`` plus the sampler, the embedding's, and none of the host's small tensor operations.

    ``uniforms``: (steps, B) float32 on the device, row i the draws of the i-th token (as ``generate(sampler="device")`` draws them; steps
    beyond the last row reuse it); None, ``temperature == 0`` or ``top_k == 1``: greedy.

    ``start(prefill_logits)`` draws the first token from the prefill's logits (no cache position is consumed), ``run(k)`` takes k steps,
    ``result()`` returns the tokens.  The loop can be run again on its cache behind another prompt: ``loop.prefill(idx, lengths)`` is
    ``model.prefill`` that keeps the rows' positions in the loop's own tensor.  ``start`` raises when ``cache.positions`` is no longer that
    tensor — an eager ``decode_step``, ``extend``, ``rewind`` or a plain ``model.prefill`` replaces it.

    The fixed bound: a row's attention launch has the split count of ``max_len`` keys whatever the row's position, where ``decode_step``
    uses the count of ``cache.pos + 1`` keys.  Row b's attention is, bit for bit, the uniform call's at the same split count
    (include/omnibiote_hip_rows.h), so the loop's logits equal ``decode_step``'s to the accuracy of another summation order — within the
    generation tests' bounds — not bit for bit.  ``capture=True`` and ``capture=False`` run the same launches and agree bit for bit.

    ``capture=True``: the body runs once eagerly with every row parked — it touches no cache byte by the rows convention, and takes the
    kernels' one-time set-up out of the capture; the loop's state is restored — and is then recorded into a ``torch.cuda.CUDAGraph``,
    one linear stream.  It needs B <= the weight-streaming product's row limit (``obte_small_m_max``): above it the products take
    paths that have not been vetted for capture, and the constructor raises ValueError (the eager body takes any B).

    ``allowed`` (a packed mask, uint8 (n,) or (B, n) on the device as ``ops.pack_token_mask`` makes it) and ``hold_min`` restrict every draw,
    the first token's included (include/omnibiote_hip_constrain.h): the sampler gets the mask, ``eos_token`` as the held token and the
    loop's own ``n_new`` as the rows' emitted counts — addresses and constants, so a captured graph replays it.  Weights, cache
    buffers and tables are captured BY ADDRESS: in-place updates of the parameters are seen by the next replay, but ``model.to(...)``,
    a reloaded parameter or a new cache leave the graph reading freed memory — build a new loop.

    ``weights`` (``model.quantize_weights()``): every block's step and the readout read the e4m3 codes (``QuantizedWeights``); a captured
    graph holds the codes' and scales' addresses like every other.  The snapshot is checked here, in ``prefill``, ``start`` and ``run``.

    ``penalty`` (a ``TokenPenalty`` bound to the prompts the cache was prefilled with, ``TokenPenalty.of(...).bind(idx, lengths,
    own_buffer=False)``): every draw is penalised (include/omnibiote_hip_penalty.h).  The sampler reads the loop's own ``out`` and ``n_new``
    as the rows' generated tokens and the penalty's prompt buffer — addresses and constants again, so a captured graph replays it;
    ``loop.prefill`` rewrites that buffer in place (a prompt no wider than the first).  ``max_steps`` is at most 32767 then."""

    def __init__(self, model, cache, *, max_steps, temperature=1.0, top_k=None, top_p=None, uniforms=None, eos_token=None, capture=False, penalty=None,
                 weights=None, allowed=None, hold_min=0):
        if isinstance(cache, SharedPrefixCache):
            _refuse_weights("DecodeLoop", weights, "do not run on a shared-prefix cache (SharedPrefixCache)")
            raise ValueError("DecodeLoop: a SharedPrefixCache steps at a host suffix position, which changes every step: the device loop needs a KVCache")
        _refuse_paged("DecodeLoop", cache, "whose table and free list the host moves between steps (the device-resident loop and graph capture over pages are not built)")
        model._check_generation("DecodeLoop", cache.batch, cache)
        if weights is not None:
            _checked_weights(model, "DecodeLoop", weights)
        if int(max_steps) < 1:
            raise ValueError(f"DecodeLoop: max_steps must be at least 1, got {max_steps}")
        if temperature < 0:
            raise ValueError(f"DecodeLoop: temperature must not be negative, got {temperature}")
        if top_k is not None and top_k < 1:
            raise ValueError(f"DecodeLoop: top_k must be at least 1, got {top_k}")
        _check_top_p("DecodeLoop", top_p)
        if isinstance(hold_min, bool) or not isinstance(hold_min, int) or hold_min < 0:
            raise ValueError(f"DecodeLoop: hold_min must be an integer of at least 0, got {hold_min!r}")
        if hold_min > 0 and eos_token is None:
            raise ValueError(f"DecodeLoop: hold_min = {hold_min} holds eos_token back, and there is no eos_token")
        if cache.pos == 0:
            raise ValueError("DecodeLoop: the cache is empty: prefill a prompt first")
        if penalty is not None:
            if not isinstance(penalty, TokenPenalty) or penalty.prompt is None or penalty.prompt.shape[0] != cache.batch:
                raise ValueError(f"DecodeLoop: penalty must be a TokenPenalty bound to the prompts of the cache's {cache.batch} rows")
            if int(max_steps) > L.PENALTY_MAX_GEN:
                raise ValueError(f"DecodeLoop: penalties count a row's generated tokens up to {L.PENALTY_MAX_GEN}, got max_steps = {max_steps}")
        cfg = model.config
        b = cache.batch
        wte = model.transformer.wte.weight
        _require_hip(wte, "DecodeLoop")
        dev = wte.device
        greedy = uniforms is None or temperature == 0 or top_k == 1
        if not greedy and (uniforms.dim() != 2 or uniforms.shape[0] < 1 or uniforms.shape[1] != b or uniforms.dtype != torch.float32):
            raise ValueError(f"DecodeLoop: uniforms must be (steps >= 1, {b}) float32, got {tuple(uniforms.shape)} {uniforms.dtype}")
        if capture and b > L.lib().obte_small_m_max():
            raise ValueError(f"DecodeLoop: capture needs a batch of at most {L.lib().obte_small_m_max()} rows (the weight-streaming product's "
                             f"limit), got {b}; capture=False takes any batch")
        self.model, self.cache, self.max_steps, self.eos_token = model, cache, int(max_steps), eos_token
        self.temperature, self.top_k, self.top_p = temperature, top_k, top_p
        self.uniforms = None if greedy else uniforms.contiguous()
        self.allowed, self.hold_min, self.weights = allowed, hold_min, weights
        if cache.positions is None:
            cache.reset(cache.pos, positions=torch.full((b,), cache.pos, dtype=torch.int32, device=dev), min_pos=cache.pos)
        self.positions = cache.positions
        self.logits = torch.zeros((b, cfg.vocab_size), dtype=torch.bfloat16, device=dev)
        self.sampled = torch.zeros(b, dtype=torch.int64, device=dev)
        self.token = torch.zeros(b, dtype=torch.int64, device=dev)
        self.u = torch.zeros(b, dtype=torch.float32, device=dev)
        self.x = torch.zeros((b, cfg.n_embd), dtype=torch.bfloat16, device=dev)
        self.count = torch.zeros(b, dtype=torch.int32, device=dev)
        self.n_new = torch.zeros(b, dtype=torch.int32, device=dev)
        self.out = torch.zeros((b, self.max_steps), dtype=torch.int64, device=dev)
        self.penalty = penalty
        # the sampler's optional keywords, empty where nothing is asked for (``emitted`` alone would select the constrained entry point)
        self._pen = {} if penalty is None else {"penalty": penalty.loop_args(self.out, self.n_new)}
        self._con = {} if allowed is None and hold_min == 0 else dict(allowed_packed=allowed, hold_token=eos_token if hold_min > 0 else None,
                                                                      emitted=self.n_new, min_emitted=hold_min)
        self.steps = 0          # body runs since start
        self.started = False
        self.graph = None
        if capture:
            self._capture()

    def _sample_and_advance(self, commit):
        ops.sample_logits(self.logits, self.u if self.uniforms is not None else None, self.temperature, self.top_k, self.top_p, out=self.sampled,
                          **self._con, **self._pen)
        ops.gen_advance(self.sampled, self.positions, self.count, self.out, self.n_new, self.token, self.model.transformer.wte.weight, self.x,
                        us=self.uniforms, u=self.u if self.uniforms is not None else None, eos=self.eos_token, commit=commit)

    @torch.no_grad()
    def _body(self):
        """one step; no host-dependent value in it: every argument is an address or a constant of the loop"""
        m, x = self.model, self.x
        m._step_blocks(x, self.cache, self.cache.max_len - 1, self.positions, weights=self.weights)
        m._readout_rows(m.transformer.ln_f(x), out=self.logits, weights=self.weights)
        self._sample_and_advance(1)

    def _capture(self):
        state = [self.positions, self.count, self.n_new, self.token, self.u]
        saved = [t.clone() for t in state]
        self.positions.fill_(-1)                                        # every row parked: the warm-up step stores and reads no cache byte
        self._body()
        for t, was in zip(state, saved):
            t.copy_(was)
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph):
            self._body()

    @torch.no_grad()
    def prefill(self, idx, lengths=None):
        """``model.prefill(idx, cache, lengths)`` for a loop that is to run again on its cache: a prefill leaves new positions behind (a new
        tensor, or uniform mode), and this writes them into the loop's own tensor and hands that back to the cache.  Returns the logits
        for ``start``."""
        logits = self.model.prefill(idx, self.cache, lengths=lengths, weights=self.weights)
        c = self.cache
        if c.positions is None:
            self.positions.fill_(c.pos)
            c.reset(c.pos, self.positions, c.pos)
        else:
            self.positions.copy_(c.positions)
            c.reset(c.pos, self.positions, c.min_pos)
        if self.penalty is not None:
            self.penalty.rebind(idx, lengths)
        self.started = False
        return logits

    @torch.no_grad()
    def start(self, prefill_logits):
        """The first token of every row, drawn from the prefill's logits (B, V): recorded, and embedded for the first step; no cache
        position is consumed.  Resets the loop's counters, so a loop may be started again behind another prefill."""
        if self.cache.positions is not self.positions:
            raise ValueError("DecodeLoop.start: cache.positions is no longer the tensor this loop was built on (an eager decode_step, extend, "
                             "rewind or model.prefill replaced it): prefill through loop.prefill, or build a new loop")
        if self.weights is not None:
            self.weights.check(self.model, "DecodeLoop.start")
        if prefill_logits.shape != self.logits.shape:
            raise ValueError(f"DecodeLoop.start: logits must be {tuple(self.logits.shape)}, got {tuple(prefill_logits.shape)}")
        self.logits.copy_(prefill_logits)
        for t in (self.count, self.n_new, self.token, self.out):
            t.zero_()
        if self.uniforms is not None:
            self.u.copy_(self.uniforms[0])
        self._sample_and_advance(0)
        self.steps, self.started = 0, True

    @torch.no_grad()
    def run(self, k, poll=16):
        """``k`` steps (fewer with ``eos_token`` once every row is parked: the positions are read on the host once every ``poll`` steps — the
        loop's only synchronisation, none without ``eos_token``).  Returns the steps taken."""
        if not self.started:
            raise ValueError("DecodeLoop.run: start the loop first")
        if self.cache.positions is not self.positions:
            raise ValueError("DecodeLoop.run: cache.positions is no longer the tensor this loop was built on: build a new loop")
        if self.weights is not None:
            self.weights.check(self.model, "DecodeLoop.run")
        k, poll = int(k), int(poll)
        if k < 0 or poll < 1:
            raise ValueError(f"DecodeLoop.run: k must not be negative and poll at least 1, got {k} and {poll}")
        if 1 + self.steps + k > self.max_steps:
            raise ValueError(f"DecodeLoop.run: {k} more steps behind {self.steps} exceed max_steps = {self.max_steps} (the first token included)")
        self.cache.require_room("DecodeLoop.run", k, detail=True)
        for i in range(k):
            if self.graph is not None:
                self.graph.replay()
            else:
                self._body()
            self.cache.advanced_on_device(1)
            self.steps += 1
            if self.eos_token is not None and (i + 1) % poll == 0 and i + 1 < k and not bool((self.positions >= 0).any()):
                return i + 1
        return k

    def result(self):
        """(tokens (B, S) int64, n_new (B,) int32): row b's first n_new[b] columns are its tokens, the rest means nothing.  S is the
        number of tokens drawn, 1 + the steps run — or, once every row has finished, the longest row's count (with ``eos_token`` this
        reads the positions on the host)."""
        width = 1 + self.steps
        if self.eos_token is not None and not bool((self.positions >= 0).any()):
            width = int(self.n_new.max())
        return self.out[:, :width].clone(), self.n_new.clone()


class SequenceScore(NamedTuple):
    """What ``OmniBioTA.score`` returns: log p of every next token (B, T - 1) fp32 (0 behind a row's length), the row sums (B,) fp32 and
    the number of scored tokens per row (B,) int64."""
    token_logprobs: torch.Tensor
    total: torch.Tensor
    count: torch.Tensor


class BeamResult(NamedTuple):
    """What ``OmniBioTA.generate_beam`` returns: per prompt its beams, best first — ``sequences`` (P, W, T0 + n) int64 (the prompt, the new
    tokens, ``pad_token`` behind a beam's first EOS), ``scores`` (P, W) fp32, the raw sums of the new tokens' log-probabilities (-inf: a
    dead beam), and ``lengths`` (P, W) int64, the new tokens up to and including the first EOS."""
    sequences: torch.Tensor
    scores: torch.Tensor
    lengths: torch.Tensor
