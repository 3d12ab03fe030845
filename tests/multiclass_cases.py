"""Float64 restatement of the C-class losses (the formulas and the table in include/wwhip.h above ww_cen_loss_fwd_bwd), the fp32
CPU torch formulation whose error against it sizes the tolerances, the inputs the multi-class tests share, and NumPy restatements
of the counters, the confusion matrix and the C-column score stage.

Per sample, with p = softmax(z), lp = log_softmax(z), onehot of the target y (``src/models/losses.py:66-87``, ``:170-197``):

    CE, smoothing eps   s = onehot (1-eps) + (1-onehot) eps/(C-1);  l = -sum s lp;  g = p - s
    focal               pt = clamp(p[y], 1e-7, 1-1e-7), fw = (1-pt)^gamma, a_t = alpha if y == 1 else 1-alpha, ce = -lp[y];
                        l = a_t fw ce;  g = a_t (fw (p - onehot) + dfw ce p[y] (onehot - p)),
                        dfw = -gamma (1-pt)^(gamma-1) strictly inside the clamp and for gamma != 0, else 0

and w_b = weight[y_b] with the reductions of tests/weighted_loss_cases.py.  At C == 2 this is that module's ``per_sample``.
tests/golden/g12_multiclass.npz, written from the reference itself, is the arbiter."""
import functools

import numpy as np
import torch

from tests.weighted_loss_cases import FOCAL_EPS, LOSSES, MARGINS, divisor_of  # noqa: F401  (shared with the tests)

CLAMP_MARGIN = 16.118                    # log((1 - 1e-7) / 1e-7): where p_t meets focal's clamp


def _log_softmax(z):
    m = z.max(axis=-1, keepdims=True)
    return z - m - np.log(np.exp(z - m).sum(axis=-1, keepdims=True))


def per_sample(kind, logits, targets, eps=0.0, alpha=0.25, gamma=2.0):
    """-> (l (B,), g (B,C)) in float64, unweighted and unreduced."""
    z, y = np.asarray(logits, dtype=np.float64), np.asarray(targets)
    C = z.shape[1]
    lp = _log_softmax(z)
    p = np.exp(lp)
    onehot = np.eye(C)[y]
    if kind == "ce":
        s = onehot * (1.0 - eps) + (1.0 - onehot) * (eps / (C - 1))
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
    """-> (loss, dlogits) in float64.  ``weight``: C values or None; ``upstream``: the (B,) gradient arriving at a 'none' loss."""
    y = np.asarray(targets)
    l, g = per_sample(kind, logits, y, **hyper)
    C = g.shape[1]
    w = np.ones(C) if weight is None else np.asarray(weight, dtype=np.float64)
    assert w.shape == (C,)
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
    C = z.shape[1]
    w = None if weight is None else torch.tensor([float(v) for v in weight], dtype=torch.float32)
    if kind == "ce" and eps == 0.0 and (reduction != "mean" or divisor == "weight_sum"):
        loss = F.cross_entropy(z, y, weight=w, reduction=reduction)
    else:
        onehot = F.one_hot(y, C).float()
        if kind == "ce":
            per = -torch.sum((onehot * (1.0 - eps) + (1 - onehot) * (eps / (C - 1))) * F.log_softmax(z, dim=-1), dim=-1)
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


def margins_of(logits, targets):
    """z_y - logsumexp of the other columns, in float64: p_y = sigmoid(margin)."""
    z, y = np.asarray(logits, dtype=np.float64), np.asarray(targets)
    rows = np.arange(len(y))
    zy = z[rows, y]
    others = z.copy()
    others[rows, y] = -np.inf
    m = others.max(axis=1)
    return zy - (m + np.log(np.exp(others - m[:, None]).sum(axis=1)))


TIE_PAIRS = ((0, 2), (1, 2), (0, 1))


@functools.lru_cache(maxsize=None)
def batch_c(B, C, targets="mixed"):
    """(logits (B,C) f32, targets (B,) i64), read-only.  The margin of the target against the logsumexp of the other columns
    runs over MARGINS under every target class, in an order with no period in common with the block.  Every ninth row (from
    row 4) first gets an exact tie between two columns -- (0,2), (1,2), (0,1) in turn, those that exist -- placed above the
    rest of the row, so that the tie decides the argmax wherever the target's margin is not positive.  No realised margin
    lies within 0.5 of +-16.118, where focal's p_t clamp makes the reference's own gradient discontinuous.
    ``targets``: "mixed" or an int (every sample of that class)."""
    combos = [(mg, y) for mg in MARGINS for y in range(C)]
    pick = (np.arange(B) * 11 + 3) % len(combos)             # 11 is coprime to 13 * C for every C the tests use
    z = np.random.default_rng(2000 + 100 * C + B).normal(0.0, 1.0, (B, C)).astype(np.float32)
    y = np.array([combos[i][1] for i in pick], np.int64)
    if targets != "mixed":
        y = np.full(B, int(targets), np.int64)
    pairs = [p for p in TIE_PAIRS if max(p) < C]
    for n, b in enumerate(range(4, B, 9)):
        a, c = pairs[n % len(pairs)]
        z[b, a] = z[b, c] = np.float32(z[b].max() + np.float32(0.25))
    for b in range(B):
        tied = (b >= 4 and (b - 4) % 9 == 0)
        a, c = pairs[((b - 4) // 9) % len(pairs)] if tied else (-1, -1)
        if tied and y[b] in (a, c):
            continue                                          # the target itself is one of the tied columns
        others = np.delete(z[b].astype(np.float64), y[b])
        lse = others.max() + np.log(np.exp(others - others.max()).sum())
        z[b, y[b]] = np.float32(lse + combos[pick[b]][0])
    assert not (np.abs(np.abs(margins_of(z, y)) - CLAMP_MARGIN) < 0.5).any()
    z.setflags(write=False)
    y.setflags(write=False)
    return z, y


def predictions(logits):
    """The loss kernel's predicted class: the first index of the row maximum under ``>``; a NaN never wins."""
    z = np.asarray(logits)
    top, pred = z[:, 0].copy(), np.zeros(len(z), np.int64)
    with np.errstate(invalid="ignore"):
        for j in range(1, z.shape[1]):
            upd = z[:, j] > top
            top = np.where(upd, z[:, j], top)
            pred = np.where(upd, j, pred)
    return pred


def counters(logits, targets):
    """(correct, tp, tn, fp, fn) with the reference's meaning for any C (``src/training/metrics.py:105-116``)."""
    pred, y = predictions(logits), np.asarray(targets)
    tp, tn = int(((pred == 1) & (y == 1)).sum()), int(((pred == 0) & (y == 0)).sum())
    fp, fn = int(((pred == 1) & (y == 0)).sum()), int(((pred == 0) & (y == 1)).sum())
    return int((pred == y).sum()), tp, tn, fp, fn


def confusion(pred, targets, C):
    """int64 (C,C) counts indexed [target, pred]."""
    idx = np.asarray(targets, np.int64) * C + np.asarray(pred, np.int64)
    return np.bincount(idx, minlength=C * C).reshape(C, C).astype(np.int64)


def softmax_conf64(logits):
    """softmax(row)[1] in float64 with the row maximum subtracted."""
    z = np.asarray(logits, dtype=np.float64)
    e = np.exp(z - z.max(axis=1, keepdims=True))
    return e[:, 1] / e.sum(axis=1)


METRIC_FIELDS = ("accuracy", "precision", "recall", "f1_score", "fpr", "fnr", "true_positives", "true_negatives",
                 "false_positives", "false_negatives", "total_samples", "positive_samples", "negative_samples")


def load_g12(golden_dir):
    """-> (loss cases, metrics cases) from g12_multiclass.npz (layout: tests/golden/make_golden_multiclass.py).  A loss case:
    name, loss_name, reduction, weight (C floats or None), z, y, loss (scalar or (B,)), grad (B,C), upstream ((B,) for 'none',
    else None).  A metrics case: name, z, y, results (dict of METRIC_FIELDS), matrix (C,C)."""
    f = np.load(golden_dir / "g12_multiclass.npz")
    out, il, ig, iu = [], 0, 0, 0
    for name in f["cases"]:
        loss_name, reduction, wname, inputs = str(name).split("|")
        z, y = f["z/" + inputs], f["y/" + inputs]
        B, C = z.shape
        weight = None if wname == "none" else tuple(float(v) for v in f[f"w/{wname}/C{C}"])
        nl = B if reduction == "none" else 1
        loss = f["loss"][il:il + nl] if reduction == "none" else f["loss"][il]
        up = f["upstream"][iu:iu + B] if reduction == "none" else None
        out.append(dict(name=str(name), loss_name=loss_name, reduction=reduction, weight=weight, z=z, y=y, loss=loss,
                        grad=f["grad"][ig:ig + C * B].reshape(B, C), upstream=up))
        il, ig, iu = il + nl, ig + C * B, iu + (B if reduction == "none" else 0)
    assert (il, ig, iu) == (len(f["loss"]), len(f["grad"]), len(f["upstream"]))
    metrics = []
    for name in f["metric_cases"]:
        name = str(name)
        vals = f["m/results/" + name]
        res = {k: (float(v) if i < 6 else int(v)) for i, (k, v) in enumerate(zip(METRIC_FIELDS, vals))}
        metrics.append(dict(name=name, z=f["m/z/" + name], y=f["m/y/" + name], results=res, matrix=f["m/matrix/" + name]))
    return out, metrics
