"""The distillation loss of a causal-LM training step as plain torch in float64: the rule that ``obte_distill_ce_rows``
(include/omnibiote_hip_distill.h, ``ops.distill_ce_rows``) implements, and the yardstick of its tests — as ``sampling.py`` and
``scoring.py`` are for their kernels.  Runs on any device; nothing here is on a hot path.

With s, t a row's student and teacher logits, tau the temperature, b = 1 / tau, P = softmax(s), p = softmax(b s), q = softmax(b t):

    CE   = lse(s) - s[target]
    KL   = sum_v q_v (b t_v - b s_v) - lse(b t) + lse(b s)            = KL(q || p)
    loss = w (alpha CE + (1 - alpha) tau^2 KL)
    d loss / d s_v = w (alpha (P_v - [v = target]) + (1 - alpha) tau^2 b (p_v - q_v))

(Hinton et al., "Distilling the Knowledge in a Neural Network", 2015: the tau^2 keeps the soft term's gradient at the scale of the hard
one.)  The row weight w is the training step's normalisation: 1 / (n_accum * rows) without ``row_weights``, else row_weights[r] / n_accum.
"""
from __future__ import annotations

from typing import NamedTuple, Optional

import torch


class DistillReference(NamedTuple):
    loss: torch.Tensor       # () float64: the sum of row_loss
    dlogits: torch.Tensor    # (n, V) float64: d loss / d logits, closed form
    row_ce: torch.Tensor     # (n,) float64, unweighted
    row_kl: torch.Tensor     # (n,) float64, unweighted
    row_loss: torch.Tensor   # (n,) float64: w (alpha CE + (1 - alpha) tau^2 KL)
    row_weight: torch.Tensor  # (n,) float64: w


def distill_weights(alpha: float, temperature: float):
    """(ce_weight, kl_weight, inv_temperature) of the C entry point for the mix ``alpha`` at ``temperature``."""
    alpha, temperature = float(alpha), float(temperature)
    if not 0.0 <= alpha <= 1.0:
        raise ValueError(f"distillation: alpha must lie in [0, 1], got {alpha}")
    if not (temperature > 0.0 and temperature < float("inf")):
        raise ValueError(f"distillation: temperature must be a positive finite number, got {temperature}")
    return alpha, (1.0 - alpha) * temperature * temperature, 1.0 / temperature


def distill_loss_float64(logits, teacher_logits, targets, row_weight, alpha: float = 0.5, temperature: float = 1.0):
    """(row_loss, row_ce, row_kl), float64, differentiable with respect to ``logits``: the rule written with torch's own ops."""
    cw, kw, b = distill_weights(alpha, temperature)
    s = logits.double()
    t = teacher_logits.double()
    ls = torch.log_softmax(s, dim=-1)
    ce = -ls.gather(1, targets.reshape(-1, 1)).reshape(-1)
    lp = torch.log_softmax(b * s, dim=-1)
    lq = torch.log_softmax(b * t, dim=-1)
    kl = (lq.exp() * (lq - lp)).sum(dim=-1)
    return row_weight * (cw * ce + kw * kl), ce, kl


def distill_reference(logits, teacher_logits, targets, n_accum: int = 1, row_weights: Optional[torch.Tensor] = None, alpha: float = 0.5,
                      temperature: float = 1.0) -> DistillReference:
    """logits, teacher_logits (n, V) of any float dtype (used as float64 values), targets int64 (n,).  The arguments of
    ``ops.distill_ce_rows``; every result in float64, the gradient in closed form (tests compare it with autograd's)."""
    if logits.dim() != 2 or teacher_logits.shape != logits.shape or targets.numel() != logits.shape[0]:
        raise ValueError(f"distill_reference: logits and teacher_logits (n, V), targets (n,); got {tuple(logits.shape)}, "
                         f"{tuple(teacher_logits.shape)}, {tuple(targets.shape)}")
    cw, kw, b = distill_weights(alpha, temperature)
    n = logits.shape[0]
    if row_weights is None:
        w = torch.full((n,), 1.0 / (n * n_accum), dtype=torch.float64, device=logits.device)
    else:
        w = row_weights.double().reshape(-1) / n_accum
    with torch.no_grad():
        s = logits.double()
        targets = targets.reshape(-1)
        row_loss, ce, kl = distill_loss_float64(s, teacher_logits, targets, w, alpha, temperature)
        P = torch.softmax(s, dim=-1)
        p = torch.softmax(b * s, dim=-1)
        q = torch.softmax(b * teacher_logits.double(), dim=-1)
        hard = P.clone()
        hard[torch.arange(n, device=s.device), targets] -= 1.0
        d = w.reshape(-1, 1) * (cw * hard + kw * b * (p - q))
    return DistillReference(row_loss.sum(), d, ce, kl, row_loss, w)
