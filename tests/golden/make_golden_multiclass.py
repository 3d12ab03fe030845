"""Generate tests/golden/g12_multiclass.npz from the reference's own loss and metrics modules.

    python tests/golden/make_golden_multiclass.py --reference PATH/TO/wakeword_trainer_home

``src/models/losses.py`` and ``src/training/metrics.py`` are loaded by file path (they import only torch and numpy).

Losses.  Inputs are stored once per batch (``z/<inputs>`` (B,C) float32, ``y/<inputs>``), ``<inputs>`` = ``C<C>B<B>`` or
``C<C>big``, and the weights once per name and width (``w/<weight>/C<C>``, float32 (C,)); the weight name ``none`` means no
weight tensor.  ``cases`` lists ``<loss>|<reduction>|<weight>|<inputs>``; their results lie one after the other, in that
order, in three flat float32 arrays: ``loss`` (1 value, or B for 'none'), ``grad`` (B*C values: autograd's gradient of the
logits) and ``upstream`` (B values for 'none', else nothing: the random vector the per-sample loss was back-propagated with).
Losses: ce0 = cross_entropy with label_smoothing 0 (``nn.CrossEntropyLoss``), ce0.1 = ``LabelSmoothingCrossEntropy(0.1)``,
focal = ``FocalLoss(0.25, 2.0)``.  Every 'mean' case is built by ``create_loss_function(..., num_classes=C, class_weights=w)``;
'sum' and 'none' construct the same classes directly (the factory only offers 'mean').
Cases, for C = 3 and 5 and each loss: B = 65 under mean x {none, generic, zero}, sum x generic, none x {generic, zero};
B = 1 and 3 under the generic weight x mean / sum / none; one batch of 8 with logits at +-88 under the generic weight, mean.
``generic`` gives every class another weight, ``zero`` has a zero entry (class 2).

Metrics.  ``metric_cases`` names two batches of 40 logits rows (C = 3 and 5) with exact ties and targets >= 2:
``m/z/<name>``, ``m/y/<name>``, ``m/results/<name>`` = ``MetricsCalculator.calculate``'s thirteen fields in the order of
``MetricResults`` as float64, ``m/matrix/<name>`` = ``confusion_matrix(..., num_classes=C)`` int64 [target, pred].

tests/multiclass_cases.py:load_g12 is the reader; the tests read only the .npz."""
import argparse
import importlib.util
from pathlib import Path

import numpy as np
import torch

HERE = Path(__file__).resolve().parent
LOSSES = {"ce0": ("cross_entropy", 0.0), "ce0.1": ("cross_entropy", 0.1), "focal": ("focal_loss", 0.0)}
WEIGHTS = {"generic": {3: (0.55, 5.0, 1.75), 5: (0.55, 5.0, 1.75, 0.8, 2.5)}, "zero": {3: (1.5, 2.0, 0.0), 5: (1.5, 2.0, 0.0, 0.7, 1.0)}}
FIELDS = ("accuracy", "precision", "recall", "f1_score", "fpr", "fnr", "true_positives", "true_negatives", "false_positives",
          "false_negatives", "total_samples", "positive_samples", "negative_samples")


def _load(reference, rel, name):
    spec = importlib.util.spec_from_file_location(name, Path(reference).resolve() / rel)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _inputs():
    g = torch.Generator().manual_seed(1212)
    out = {}
    for C in (3, 5):
        out[f"C{C}B65"] = (torch.randn(65, C, generator=g) * 2.5, torch.randint(0, C, (65,), generator=g))
        # the two tiny batches are written out: margins at which p - target does not cancel, so that the reference's own fp32
        # gradient is good to a few ulp of its largest entry and the 1e-6 comparison with a float64 restatement is meaningful
        rows = torch.tensor([[0.5, -1.25, 0.75, -0.5, 1.0], [-2.0, 1.0, 0.25, 0.5, -1.5], [0.25, 0.75, -1.0, 1.25, 0.0]])[:, :C]
        out[f"C{C}B1"] = (rows[:1].clone(), torch.tensor([1]))
        out[f"C{C}B3"] = (rows.clone(), torch.tensor([0, 2, C - 1]))
        big = torch.zeros(8, C)
        big[:, :3] = torch.tensor([[88.0, -88.0, 0.0], [-88.0, 88.0, -88.0], [88.0, -88.0, 88.0], [-88.0, 88.0, 87.0],
                                   [88.0, 87.0, -88.0], [-88.0, -87.5, -88.0], [0.0, 0.0, 0.0], [1.5, -0.5, 88.0]])
        out[f"C{C}big"] = (big, torch.tensor([0, 0, 1, 2, 1, 0, 2, C - 1]))
    return out


def _criterion(ref, loss_name, reduction, w, C):
    name, eps = LOSSES[loss_name]
    if reduction == "mean":
        return ref.create_loss_function(name, num_classes=C, label_smoothing=eps, focal_alpha=0.25, focal_gamma=2.0,
                                        class_weights=w, device="cpu")
    if loss_name == "ce0":
        return torch.nn.CrossEntropyLoss(weight=w, reduction=reduction)
    if loss_name == "ce0.1":
        return ref.LabelSmoothingCrossEntropy(smoothing=eps, weight=w, reduction=reduction)
    return ref.FocalLoss(alpha=0.25, gamma=2.0, weight=w, reduction=reduction)


def _metric_inputs():
    g = torch.Generator().manual_seed(1213)
    out = {}
    for C in (3, 5):
        z = torch.randn(40, C, generator=g)
        y = torch.randint(0, C, (40,), generator=g)
        for b, (a, c) in zip(range(0, 40, 3), [(0, 2), (1, 2), (0, 1)] * 5):      # exact ties at the top of the row
            z[b, a] = z[b, c] = z[b].max() + 0.5
        z[38] = 0.0                                                               # a row of equal logits
        y[:6] = torch.tensor([0, 1, 2, 2, 1, 0])
        out[f"C{C}"] = (z, y)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="checkout of the reference project")
    args = ap.parse_args()
    ref = _load(args.reference, Path("src") / "models" / "losses.py", "reference_losses")
    met = _load(args.reference, Path("src") / "training" / "metrics.py", "reference_metrics")

    inputs = _inputs()
    plan = []
    for C in (3, 5):
        for ln in LOSSES:
            plan += [(ln, "mean", wn, f"C{C}B65") for wn in ("none", "generic", "zero")]
            plan += [(ln, "sum", "generic", f"C{C}B65"), (ln, "none", "generic", f"C{C}B65"), (ln, "none", "zero", f"C{C}B65")]
            plan += [(ln, red, "generic", f"C{C}B{B}") for red in ("mean", "sum", "none") for B in (1, 3)]
            plan += [(ln, "mean", "generic", f"C{C}big")]
    out = {"cases": np.array(["|".join(c) for c in plan])}
    for wn, per_c in WEIGHTS.items():
        for C, w in per_c.items():
            out[f"w/{wn}/C{C}"] = np.array(w, dtype=np.float32)
    for k, (z, y) in inputs.items():
        out["z/" + k], out["y/" + k] = z.numpy(), y.numpy()
    g = torch.Generator().manual_seed(1214)
    losses, grads, ups = [], [], []
    for ln, red, wn, inp in plan:
        z0, y = inputs[inp]
        C = z0.shape[1]
        w = None if wn == "none" else torch.tensor(WEIGHTS[wn][C], dtype=torch.float32)
        z = z0.clone().requires_grad_()
        loss = _criterion(ref, ln, red, w, C)(z, y)
        if red == "none":
            up = torch.randn(len(y), generator=g)
            loss.backward(up)
            ups.append(up.numpy())
        else:
            loss.backward()
        losses.append(loss.detach().numpy().reshape(-1))
        grads.append(z.grad.numpy().reshape(-1))
    out["loss"], out["grad"], out["upstream"] = (np.concatenate(v).astype(np.float32) for v in (losses, grads, ups))

    calc = met.MetricsCalculator(device="cpu")
    names = []
    for name, (z, y) in _metric_inputs().items():
        res = calc.calculate(z, y)
        names.append(name)
        out["m/z/" + name], out["m/y/" + name] = z.numpy(), y.numpy()
        out["m/results/" + name] = np.array([getattr(res, k) for k in FIELDS], dtype=np.float64)
        out["m/matrix/" + name] = calc.confusion_matrix(z, y, num_classes=z.shape[1]).numpy().astype(np.int64)
    out["metric_cases"] = np.array(names)
    np.savez_compressed(HERE / "g12_multiclass.npz", **out)
    print(f"{len(plan)} loss cases, {len(names)} metrics cases -> {HERE / 'g12_multiclass.npz'}")


if __name__ == "__main__":
    main()
