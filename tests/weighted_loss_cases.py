"""Float64 restatement of the weighted 2-class losses (the table in include/wwhip.h above ww_ce2_loss_weighted_fwd_bwd), the fp32
CPU torch formulation whose error against it sizes the tolerances, and the inputs the weighted-loss tests share.

Per sample, l_b and g_b = dl_b/dz_b are the reference's ``LabelSmoothingCrossEntropy`` / ``FocalLoss`` terms
(``src/models/losses.py:66-87``, ``:170-197``); w_b = weight[y_b]:

    mean, "batch"        loss = sum w_b l_b / B            grad = w_b g_b / B            (loss * weight).mean()
    mean, "weight_sum"   loss = sum w_b l_b / sum w_b      grad = w_b g_b / sum w_b      nn.CrossEntropyLoss(weight=...)
    sum                  loss = sum w_b l_b                grad = w_b g_b
    none                 loss = (w_b l_b)_b                grad = w_b g_b * upstream_b

Which divisor a class takes is ``divisor_of``: only the eps == 0 branch of the factory (``nn.CrossEntropyLoss``, ``:256``)
divides by the weights' sum.  tests/golden/g9_weighted_loss.npz, written from the reference itself, is the arbiter."""
import functools

import numpy as np
import torch

FOCAL_EPS = 1e-7
LOSSES = {"ce0": ("ce", dict(eps=0.0)), "ce0.1": ("ce", dict(eps=float(np.float32(0.1)))),
          "focal": ("focal", dict(alpha=0.25, gamma=2.0))}
WEIGHTS = {"w0.55-5": (0.55, 5.0), "w1-1": (1.0, 1.0), "w0-2": (0.0, 2.0)}


def divisor_of(loss_name):
    """What the reference's weighted 'mean' divides by for the class ``create_loss_function`` returns under this name."""
    return "weight_sum" if loss_name == "ce0" else "batch"


def _log_softmax(z):
    m = z.max(axis=-1, keepdims=True)
    return z - m - np.log(np.exp(z - m).sum(axis=-1, keepdims=True))


def per_sample(kind, logits, targets, eps=0.0, alpha=0.25, gamma=2.0):
    """-> (l (B,), g (B,2)) in float64, unweighted and unreduced."""
    z, y = np.asarray(logits, dtype=np.float64), np.asarray(targets)
    lp = _log_softmax(z)
    p = np.exp(lp)
    onehot = np.eye(2)[y]
    if kind == "ce":
        s = onehot * (1.0 - eps) + (1.0 - onehot) * eps
        return -(s * lp).sum(-1), p - s
    pt_raw = (p * onehot).sum(-1)
    pt = np.clip(pt_raw, FOCAL_EPS, 1.0 - FOCAL_EPS)
    fw = (1.0 - pt) ** gamma
    a_t = np.where(y == 1, alpha, 1.0 - alpha)
    ce = -(lp * onehot).sum(-1)
    inside = (pt_raw > FOCAL_EPS) & (pt_raw < 1.0 - FOCAL_EPS)
    with np.errstate(invalid="ignore", divide="ignore"):
        dfw = np.where(inside & (gamma != 0.0), -gamma * (1.0 - pt) ** (gamma - 1.0), 0.0)
    dpt = pt_raw[:, None] * (onehot - p)
    return a_t * fw * ce, a_t[:, None] * (fw[:, None] * (p - onehot) + (dfw * ce)[:, None] * dpt)


def weighted_loss(kind, logits, targets, weight, reduction, divisor="batch", upstream=None, **hyper):
    """-> (loss, dlogits) in float64.  ``weight``: (w_neg, w_pos) or None; ``upstream``: the (B,) gradient arriving at a
    'none' loss (ones if omitted)."""
    y = np.asarray(targets)
    l, g = per_sample(kind, logits, y, **hyper)
    w = np.ones(2) if weight is None else np.asarray(weight, dtype=np.float64)
    wb = w[y]
    wl, wg = wb * l, wb[:, None] * g
    if reduction == "none":
        return wl, wg if upstream is None else wg * np.asarray(upstream, dtype=np.float64)[:, None]
    if reduction == "sum":
        return wl.sum(), wg
    assert reduction == "mean" and divisor in ("batch", "weight_sum")
    den = float(len(y)) if divisor == "batch" else wb.sum()
    with np.errstate(invalid="ignore", divide="ignore"):
        return wl.sum() / den, wg / den


def torch32(kind, logits, targets, weight, reduction, divisor="batch", upstream=None, eps=0.0, alpha=0.25, gamma=2.0):
    """The same quantities from fp32 CPU torch with autograd, written the way the reference writes them -> (loss, dlogits) as
    float64 arrays of fp32 values.  The weighted mean over the weights' sum at eps == 0 is torch's own cross_entropy."""
    F = torch.nn.functional
    z = torch.from_numpy(np.array(logits, dtype=np.float32)).requires_grad_()
    y = torch.from_numpy(np.array(targets, dtype=np.int64))
    w = None if weight is None else torch.tensor([float(weight[0]), float(weight[1])], dtype=torch.float32)
    if kind == "ce" and eps == 0.0 and (reduction != "mean" or divisor == "weight_sum"):
        loss = F.cross_entropy(z, y, weight=w, reduction=reduction)
    else:
        onehot = F.one_hot(y, 2).float()
        if kind == "ce":
            per = -torch.sum((onehot * (1.0 - eps) + (1 - onehot) * eps) * F.log_softmax(z, dim=-1), dim=-1)
        else:
            pt = torch.clamp(torch.sum(F.softmax(z, dim=-1) * onehot, dim=-1), min=FOCAL_EPS, max=1.0 - FOCAL_EPS)
            a_t = torch.where(y == 1, torch.tensor(alpha), torch.tensor(1 - alpha))
            per = a_t * (1 - pt) ** gamma * F.cross_entropy(z, y, reduction="none")
        if w is not None:
            per = per * w[y]
        if reduction == "none":
            loss = per
        elif reduction == "sum":
            loss = per.sum()
        else:
            loss = per.mean() if divisor == "batch" else per.sum() / (w[y].sum() if w is not None else float(len(y)))
    if reduction == "none":
        loss.backward(torch.ones(len(y)) if upstream is None else torch.from_numpy(np.array(upstream, dtype=np.float32)))
    else:
        loss.backward()
    return loss.detach().numpy().astype(np.float64), z.grad.numpy().astype(np.float64)


MARGINS = (0.0,) + tuple(s * a for a in (1e-3, 1.0, 15.0, 17.5, 30.0, 90.0) for s in (1.0, -1.0))


@functools.lru_cache(maxsize=None)
def batch(B, targets="mixed"):
    """(logits (B,2) f32, targets (B,) i64), read-only: every margin z1 - z0 of MARGINS under both labels, in an order with no
    period in common with the block; a margin of 0 is an exact tie, none lies within 0.5 of 16.118, where focal's p_t clamp
    makes the reference's own gradient discontinuous.  ``targets``: "mixed", "zeros" or "ones"."""
    combos = [(mg, y) for mg in MARGINS for y in (0, 1)]
    pick = (np.arange(B) * 7 + 3) % len(combos)
    z0 = np.random.default_rng(1000 + B).normal(0.0, 1.0, B).astype(np.float32)
    z1 = (z0 + np.array([combos[i][0] for i in pick], np.float32)).astype(np.float32)
    z = np.stack([z0, z1], axis=1)
    assert not ((np.abs(np.abs(z[:, 1].astype(np.float64) - z[:, 0]) - 16.118) < 0.5).any())
    y = np.array([combos[i][1] for i in pick], np.int64)
    if targets != "mixed":
        y = np.full(B, {"zeros": 0, "ones": 1}[targets], np.int64)
    z.setflags(write=False)
    y.setflags(write=False)
    return z, y


def counters(logits, targets):
    """(correct, tp, tn, fp, fn): argmax with ties to class 0, weights ignored."""
    z, y = np.asarray(logits), np.asarray(targets)
    pred = (z[:, 1] > z[:, 0]).astype(np.int64)
    tp, tn = int(((pred == 1) & (y == 1)).sum()), int(((pred == 0) & (y == 0)).sum())
    fp, fn = int(((pred == 1) & (y == 0)).sum()), int(((pred == 0) & (y == 1)).sum())
    return tp + tn, tp, tn, fp, fn


def load_g9(golden_dir):
    """-> list of case dicts from g9_weighted_loss.npz (layout: tests/golden/make_golden_weighted_loss.py): name, loss_name,
    reduction, weight, z, y, loss (scalar or (B,)), grad (B,2), upstream ((B,) for 'none', else None)."""
    f = np.load(golden_dir / "g9_weighted_loss.npz")
    weights = {str(n): tuple(float(v) for v in w) for n, w in zip(f["weight_names"], f["weights"])}
    out, il, ig, iu = [], 0, 0, 0
    for name in f["cases"]:
        loss_name, reduction, wname, inputs = str(name).split("|")
        z, y = f["z/" + inputs], f["y/" + inputs]
        B = len(y)
        nl = B if reduction == "none" else 1
        loss = f["loss"][il:il + nl] if reduction == "none" else f["loss"][il]
        up = f["upstream"][iu:iu + B] if reduction == "none" else None
        out.append(dict(name=str(name), loss_name=loss_name, reduction=reduction, weight=weights[wname], z=z, y=y, loss=loss,
                        grad=f["grad"][ig:ig + 2 * B].reshape(B, 2), upstream=up))
        il, ig, iu = il + nl, ig + 2 * B, iu + (B if reduction == "none" else 0)
    assert (il, ig, iu) == (len(f["loss"]), len(f["grad"]), len(f["upstream"]))
    return out
