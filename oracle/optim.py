"""Step-tail oracle: gradient clipping, the optimizer update and the dynamic loss scale, restated in float64.

Follows the reference lines the fused kernel (csrc/ww_optim.hip) cites:
  * ``src/training/optimizer_factory.py:165-199`` -- create_optimizer: torch.optim.Adam / AdamW / SGD(nesterov=True)
  * ``src/training/optimizer_factory.py:446-452`` -- clip_gradients: torch.nn.utils.clip_grad_norm_
  * ``src/training/optimizer_factory.py:403-420`` -- create_grad_scaler: torch.amp.GradScaler and its defaults
  * ``src/training/trainer.py:177-193``           -- skip a non-finite loss; scale -> unscale_ -> clip -> step -> update
The formulas are torch.optim's single-tensor ones (bias corrections from the step number), written out on numpy float64
arrays; nothing is modified in place.
PINNED: tests/test_optim_oracle.py (against torch.optim and torch.amp.GradScaler themselves, float64, on the CPU)."""
import math

import numpy as np

KINDS = ("adam", "adamw", "sgd")


def clip_grad_norm(g, max_norm):
    """-> (norm, clipped): torch.nn.utils.clip_grad_norm_ on one tensor, ``c = min(1, max_norm / (norm + 1e-6))``.
    A non-finite norm propagates as torch's does: an inf norm gives c = 0 (and inf * 0 = NaN at the inf element), a NaN norm
    gives c = NaN (the comparison with 1 is false).  ``max_norm <= 0``: the norm only, the gradient unchanged."""
    g = np.asarray(g, dtype=np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        norm = float(np.sqrt((g * g).sum()))
        if not max_norm > 0:
            return norm, g.copy()
        c = max_norm / (norm + 1e-6)
        if c > 1.0:                      # torch.clamp(c, max=1.0); NaN compares false and stays
            c = 1.0
        return norm, g * c


def optim_step(kind, p, g, m, v, t, lr, betas=(0.9, 0.999), eps=1e-8, wd=0.0, momentum=0.0):
    """One update of step number ``t`` (1 = the first) -> (p, m, v), new float64 arrays.
    adam : L2 term in the gradient      (torch.optim.Adam,  weight_decay)
    adamw: decoupled decay              (torch.optim.AdamW: p *= 1 - lr * wd)
    sgd  : nesterov=True, dampening=0   (torch.optim.SGD; ``m`` is the momentum buffer, ``v`` is passed through).  A zero
           buffer reproduces torch's "first step: buf = g"; with momentum == 0 the buffer is not touched."""
    p, g = np.asarray(p, dtype=np.float64), np.asarray(g, dtype=np.float64)
    m = None if m is None else np.asarray(m, dtype=np.float64)
    v = None if v is None else np.asarray(v, dtype=np.float64)
    if kind == "sgd":
        if wd != 0:
            g = g + wd * p
        if momentum != 0:
            m = momentum * m + g
            g = g + momentum * m
        return p - lr * g, m, v
    if kind not in ("adam", "adamw"):
        raise ValueError(f"unknown optimizer kind {kind!r}")
    beta1, beta2 = betas
    if kind == "adamw":
        p = p * (1.0 - lr * wd)
    elif wd != 0:
        g = g + wd * p
    m = m + (1.0 - beta1) * (g - m)                       # exp_avg.lerp_(grad, 1 - beta1)
    v = beta2 * v + (1.0 - beta2) * g * g                 # exp_avg_sq.mul_(beta2).addcmul_(grad, grad, value=1 - beta2)
    bc1, bc2 = 1.0 - beta1 ** t, 1.0 - beta2 ** t
    denom = np.sqrt(v) / math.sqrt(bc2) + eps
    return p - (lr / bc1) * (m / denom), m, v


def grad_scaler_update(scale, tracker, growth=2.0, backoff=0.5, interval=2000, grads_nonfinite=False, skipped=False):
    """-> (scale, tracker) after one step: the rule above ``ww_loss_scale`` in include/wwhip.h, which is
    torch.amp.GradScaler.update().  Non-finite gradients: scale * backoff, tracker 0.  An applied step: tracker + 1, and
    once it reaches the interval scale * growth, tracker 0.  ``skipped`` without non-finite gradients (the batch was
    dropped for its loss or targets before the scaler saw it): both unchanged."""
    if grads_nonfinite:
        return scale * backoff, 0
    if skipped:
        return scale, tracker
    tracker += 1
    if tracker >= interval:
        return scale * growth, 0
    return scale, tracker
