"""Generate tests/golden/g9_weighted_loss.npz from the reference's own loss module.

    python tests/golden/make_golden_weighted_loss.py --reference PATH/TO/wakeword_trainer_home

``src/models/losses.py`` is loaded by file path (it imports only torch).  Inputs are stored once per batch (``z/<inputs>``,
``y/<inputs>``) and the weights once per name (``weight_names``, ``weights``: float32 [w_neg, w_pos]).  ``cases`` lists
``<loss>|<reduction>|<weight>|<inputs>``; their results lie one after the other, in that order, in three flat float32 arrays
(one zip member per case would cost more than the numbers): ``loss`` (1 value, or B for 'none'), ``grad`` (2B values:
autograd's gradient of the logits) and ``upstream`` (B values for 'none', else nothing: the random vector the per-sample loss
was back-propagated with).  tests/weighted_loss_cases.py:load_g9 is the reader.

Losses: ce0 = cross_entropy with label_smoothing 0 (``nn.CrossEntropyLoss``), ce0.1 = ``LabelSmoothingCrossEntropy(0.1)``,
focal = ``FocalLoss(0.25, 2.0)``.  Every 'mean' case is built by ``create_loss_function(..., class_weights=w)``, the call chain
a user takes; 'sum' and 'none' construct the same classes directly (the factory only offers 'mean').
Cases: B = 65 with all three weights x all three reductions; B = 1 and 3 with (0.55, 5.0) x all three reductions; and one batch
of 8 with logits at +-88 (as G1 has) under (0.55, 5.0), mean.  The tests read only the .npz."""
import argparse
import importlib.util
from pathlib import Path

import numpy as np
import torch

HERE = Path(__file__).resolve().parent
LOSSES = {"ce0": ("cross_entropy", 0.0), "ce0.1": ("cross_entropy", 0.1), "focal": ("focal_loss", 0.0)}
WEIGHTS = {"w0.55-5": (0.55, 5.0), "w1-1": (1.0, 1.0), "w0-2": (0.0, 2.0)}


def _inputs():
    g = torch.Generator().manual_seed(909)
    out = {}
    for B in (1, 3, 65):
        z = torch.randn(B, 2, generator=g) * 2.5
        y = (torch.rand(B, generator=g) < 0.35).long()
        out[f"B{B}"] = (z, y)
    # the two tiny batches are written out: margins at which p - target does not cancel, so that the reference's own fp32
    # gradient is good to a few ulp of its largest entry and the 1e-6 comparison with a float64 restatement is meaningful
    out["B1"] = (torch.tensor([[0.5, -1.25]]), torch.tensor([1]))
    out["B3"] = (torch.tensor([[0.5, -1.25], [-2.0, 1.0], [0.25, 0.75]]), torch.tensor([0, 1, 0]))
    big = torch.tensor([[88.0, -88.0], [-88.0, 88.0], [88.0, -88.0], [-88.0, 88.0], [88.0, 87.0], [-88.0, -87.5], [0.0, 0.0],
                        [1.5, -0.5]])
    out["big8"] = (big, torch.tensor([0, 0, 1, 1, 1, 0, 1, 0]))
    return out


def _criterion(ref, loss_name, reduction, w):
    name, eps = LOSSES[loss_name]
    if reduction == "mean":
        return ref.create_loss_function(name, num_classes=2, label_smoothing=eps, focal_alpha=0.25, focal_gamma=2.0,
                                        class_weights=w, device="cpu")
    if loss_name == "ce0":
        return torch.nn.CrossEntropyLoss(weight=w, reduction=reduction)
    if loss_name == "ce0.1":
        return ref.LabelSmoothingCrossEntropy(smoothing=eps, weight=w, reduction=reduction)
    return ref.FocalLoss(alpha=0.25, gamma=2.0, weight=w, reduction=reduction)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="checkout of the reference project (src/models/losses.py is loaded)")
    args = ap.parse_args()
    spec = importlib.util.spec_from_file_location("reference_losses", Path(args.reference).resolve() / "src" / "models" / "losses.py")
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)

    inputs = _inputs()
    plan = [(ln, red, wn, "B65") for ln in LOSSES for red in ("mean", "sum", "none") for wn in WEIGHTS]
    plan += [(ln, red, "w0.55-5", inp) for ln in LOSSES for red in ("mean", "sum", "none") for inp in ("B1", "B3")]
    plan += [(ln, "mean", "w0.55-5", "big8") for ln in LOSSES]
    out = {"cases": np.array(["|".join(c) for c in plan]), "weight_names": np.array(list(WEIGHTS)),
           "weights": np.array(list(WEIGHTS.values()), dtype=np.float32)}
    for k, (z, y) in inputs.items():
        out["z/" + k], out["y/" + k] = z.numpy(), y.numpy()
    g = torch.Generator().manual_seed(910)
    losses, grads, ups = [], [], []
    for ln, red, wn, inp in plan:
        w = torch.tensor(WEIGHTS[wn], dtype=torch.float32)
        z0, y = inputs[inp]
        z = z0.clone().requires_grad_()
        loss = _criterion(ref, ln, red, w)(z, y)
        if red == "none":
            up = torch.randn(len(y), generator=g)
            loss.backward(up)
            ups.append(up.numpy())
        else:
            loss.backward()
        losses.append(loss.detach().numpy().reshape(-1))
        grads.append(z.grad.numpy().reshape(-1))
    out["loss"], out["grad"], out["upstream"] = (np.concatenate(v).astype(np.float32) for v in (losses, grads, ups))
    np.savez_compressed(HERE / "g9_weighted_loss.npz", **out)
    print(f"{len(plan)} cases -> {HERE / 'g9_weighted_loss.npz'}")


if __name__ == "__main__":
    main()
