"""Loss factory of the hot path: same names, constructor arguments and input validation as
the reference (``src/models/losses.py:14-270``); the arithmetic (loss, gradient, batch
counters) is one HIP kernel.  Scope: ``num_classes`` from 2 to ``LOSS_MAX_CLASSES`` (2 by default); optional per-class
``weight`` (``:89-92``, ``:199-202``, ``:256``) and ``reduction`` in mean / sum / none (``:95-102``).

Three C-ABI entries.  With two classes, ``weight=None`` with ``reduction="mean"`` -- what ``Trainer`` builds unless it is handed
class weights (``src/training/trainer.py:78-86`` passes ``class_weights=None``) -- calls ``ww_ce2_loss_fwd_bwd`` and every other
combination calls ``ww_ce2_loss_weighted_fwd_bwd``; with more than two classes every combination calls ``ww_cen_loss_fwd_bwd``,
which can also count the batch into a (C,C) confusion matrix on the device (``track_confusion``).
The weighted mean follows the reference class by class: ``CrossEntropyLoss`` divides
by the sum of the batch's weights as ``nn.CrossEntropyLoss(weight=...)`` does, ``LabelSmoothingCrossEntropy`` and
``FocalLoss`` divide by the batch size (``(loss * weight).mean()``).

Data parallel: each rank normalises by its own batch -- by its own sum of weights under ``CrossEntropyLoss`` -- and the ranks'
gradients are averaged, which is what torch DDP does with a weighted ``nn.CrossEntropyLoss``.  Under that divisor a sharded
run is therefore not the single-process run on the concatenated batch."""
from typing import Optional

import torch
import torch.nn as nn

from .. import _native as nat

_REDUCTIONS = {"mean": nat.REDUCE_MEAN, "sum": nat.REDUCE_SUM, "none": nat.REDUCE_NONE}


class _CE2Fn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, targets, mod):
        loss, vec, dl, stats = mod._launch(logits.contiguous(), targets.contiguous(), mod.found_inf_out)
        mod.last_stats = stats
        ctx.save_for_backward(dl)
        ctx.per_sample = vec is not None
        return vec if ctx.per_sample else loss.reshape(())

    @staticmethod
    def backward(ctx, gout):
        (dl,) = ctx.saved_tensors
        return dl * (gout[:, None] if ctx.per_sample else gout), None, None


class _NativeLoss(nn.Module):
    _kind = nat.LOSS_CE
    _eps, _alpha, _gamma = 0.0, 0.25, 2.0
    _divisor = nat.DIV_BATCH              # what a weighted 'mean' divides by: (loss * weight).mean() of the reference classes

    def __init__(self, weight: Optional[torch.Tensor], reduction: str, num_classes: int = 2):
        super().__init__()
        if isinstance(num_classes, bool) or not isinstance(num_classes, int) or not 2 <= num_classes <= nat.LOSS_MAX_CLASSES:
            raise ValueError(f"num_classes must be an int in [2, {nat.LOSS_MAX_CLASSES}] for the HIP loss kernels, got {num_classes!r}")
        C = num_classes
        if weight is not None and not (torch.is_tensor(weight) and weight.dtype == torch.float32 and tuple(weight.shape) == (C,)):
            what = f"{weight.dtype} {tuple(weight.shape)}" if torch.is_tensor(weight) else type(weight).__name__
            layout = "[w_neg, w_pos] for the 2-class" if C == 2 else f"(one weight per class) for the {C}-class"
            raise ValueError(f"weight must be a float32 tensor of shape ({C},) {layout} HIP loss kernel, got {what}")
        self.num_classes = C
        if reduction not in _REDUCTIONS:
            raise ValueError(f"Invalid reduction: {reduction}")
        # a buffer, so that criterion.to(device) takes it along; the kernel reads it through its pointer at run time, so an
        # in-place change of its values holds from the next step on, eager or replayed from a captured graph
        self.register_buffer("weight", None if weight is None else weight.detach().clone())
        self.reduction = reduction
        self.validate_targets = True      # reference behaviour: raise at once (costs a host sync)
        self.last_stats = None            # device uint8[48] = ww_step_stats of the last call
        self.found_inf_out = None         # float32[1] device tensor that also receives found_inf (data-parallel bucket slot)
        self.loss_scale = None            # device ww_loss_scale (fp16 storage): dL/dlogits leaves the kernel times scale[slot]
        self.loss_scale_slot = 0
        self.confusion = None             # int64 (C,C) device tensor [target, pred] once track_confusion() was called (C > 2)
        self._stats = {}

    def track_confusion(self, device=None):
        """Allocate, once, a zeroed (C,C) int64 device matrix indexed [target, pred]; every launch from then on adds its batch
        to it unless the launch sets found_inf (non-finite loss or a bad target).  The tensor is never replaced, so a captured
        graph keeps counting into it; the caller zeroes it in place (``criterion.confusion.zero_()``) and reads it when it wants.
        Only the C-class entry counts, so this needs num_classes > 2."""
        if self.num_classes == 2:
            raise ValueError("track_confusion needs num_classes > 2: with two classes ww_step_stats' tp/tn/fp/fn are the matrix")
        if self.confusion is None:
            dev = device if device is not None else (self.weight.device if self.weight is not None else "cuda")
            if torch.device(dev).type != "cuda":
                raise nat.NativeError("the confusion matrix lives on an MI355X ('cuda') device -- there is no CPU fallback")
            self.confusion = torch.zeros(self.num_classes, self.num_classes, dtype=torch.int64, device=dev)
        return self.confusion

    def _stats_for(self, dev):
        if dev not in self._stats:
            self._stats[dev] = torch.zeros(nat.STEP_STATS_BYTES, dtype=torch.uint8, device=dev)
        return self._stats[dev]

    def _launch(self, logits, targets, found_inf_out):
        """One kernel launch -> (loss (1,), loss_vec (B,) or None, dlogits, stats).  Two classes: the unweighted mean through
        the entry it always had, everything else through the weighted one.  More than two: the C-class entry."""
        stats = self._stats_for(logits.device)
        if self.num_classes == 2 and self.reduction == "mean" and self.weight is None:
            loss, dl, stats = nat.ce2_loss_fwd_bwd(logits, targets, self._kind, self._eps, self._alpha, self._gamma, stats=stats,
                                                   found_inf_out=found_inf_out, loss_scale=self.loss_scale,
                                                   loss_scale_slot=self.loss_scale_slot)
            return loss, None, dl, stats
        w = self.weight
        if w is not None and (w.device != logits.device or w.dtype != torch.float32):
            # no copy here: a host-to-device copy per step would sync, and could not be captured into a graph
            raise ValueError(f"the loss weight is {w.dtype} on {w.device} but the logits are on {logits.device}: move the "
                             "criterion with .to(device) (it must stay float32)")
        if self.num_classes > 2:
            if self.confusion is not None and self.confusion.device != logits.device:
                raise ValueError(f"the confusion matrix is on {self.confusion.device} but the logits are on {logits.device}")
            return nat.cen_loss_fwd_bwd(logits, targets, self._kind, self._eps, self._alpha, self._gamma, class_weight=w,
                                        reduction=_REDUCTIONS[self.reduction], mean_divisor=self._divisor, stats=stats,
                                        found_inf_out=found_inf_out, loss_scale=self.loss_scale,
                                        loss_scale_slot=self.loss_scale_slot, confusion=self.confusion)
        return nat.ce2_loss_weighted_fwd_bwd(logits, targets, self._kind, self._eps, self._alpha, self._gamma, class_weight=w,
                                             reduction=_REDUCTIONS[self.reduction], mean_divisor=self._divisor, stats=stats,
                                             found_inf_out=found_inf_out, loss_scale=self.loss_scale,
                                             loss_scale_slot=self.loss_scale_slot)

    def native_fwd_bwd(self, logits: torch.Tensor, target: torch.Tensor, found_inf_out=None):
        """Loss kernel without autograd: -> (device ww_step_stats, dL/dlogits).  Target range errors are reported through
        ``stats.bad_target`` (the caller reads the stats once per step).  With ``reduction='none'`` the gradient is that of
        the per-sample losses' sum and ``stats.loss`` their mean."""
        C = self.num_classes
        if logits.dim() != 2 or logits.size(1) != C or target.dim() != 1 or logits.size(0) != target.size(0):
            raise ValueError(f"expected logits (B,{C}) for num_classes = {C} and targets (B,), got {tuple(logits.shape)} and "
                             f"{tuple(target.shape)}")
        _, _, dl, stats = self._launch(logits.contiguous(), target.long().contiguous(), found_inf_out)
        self.last_stats = stats
        return stats, dl

    def forward(self, pred: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
        if pred.dim() != 2:
            raise ValueError(f"Predictions must be 2D (batch, num_classes), got shape {pred.shape}")
        if target.dim() != 1:
            raise ValueError(f"Targets must be 1D (batch,), got shape {target.shape}")
        if pred.size(0) != target.size(0):
            raise ValueError(f"Batch size mismatch: pred={pred.size(0)}, target={target.size(0)}")
        if pred.size(1) != self.num_classes:
            raise ValueError(f"this criterion was built for num_classes = {self.num_classes}, got logits with {pred.size(1)} columns")
        if not pred.is_cuda:
            raise nat.NativeError("the loss runs on a hand-written HIP kernel only; tensors must be on an MI355X "
                                  "('cuda') device -- there is no CPU fallback")
        loss = _CE2Fn.apply(pred.float(), target.long(), self)
        if self.validate_targets:
            st = nat.decode_stats(self.last_stats.cpu())
            if st["bad_target"]:
                raise ValueError(f"Target values must be in [0, {self.num_classes - 1}]")
        return loss


class LabelSmoothingCrossEntropy(_NativeLoss):
    def __init__(self, smoothing: float = 0.1, weight: Optional[torch.Tensor] = None, reduction: str = "mean", *,
                 num_classes: int = 2):
        if not 0.0 <= smoothing <= 1.0:
            raise ValueError(f"Label smoothing must be in [0, 1], got {smoothing}")
        super().__init__(weight, reduction, num_classes)
        self.smoothing, self.confidence = smoothing, 1.0 - smoothing
        self._eps = float(smoothing)


class CrossEntropyLoss(LabelSmoothingCrossEntropy):
    """label_smoothing == 0 branch (the reference returns nn.CrossEntropyLoss there, losses.py:256): its weighted mean divides
    by the sum of the batch's weights, not by the batch size."""
    _divisor = nat.DIV_WEIGHT_SUM

    def __init__(self, weight: Optional[torch.Tensor] = None, reduction: str = "mean", *, num_classes: int = 2):
        super().__init__(0.0, weight, reduction, num_classes=num_classes)


class FocalLoss(_NativeLoss):
    _kind = nat.LOSS_FOCAL
    EPS = 1e-7

    def __init__(self, alpha: float = 0.25, gamma: float = 2.0, weight: Optional[torch.Tensor] = None,
                 reduction: str = "mean", *, num_classes: int = 2):
        if not 0.0 <= alpha <= 1.0:
            raise ValueError(f"Alpha must be in [0, 1], got {alpha}")
        if gamma < 0:
            raise ValueError(f"Gamma must be non-negative, got {gamma}")
        super().__init__(weight, reduction, num_classes)
        self.alpha, self.gamma = alpha, gamma
        self._alpha, self._gamma = float(alpha), float(gamma)


def create_loss_function(loss_name: str, num_classes: int = 2, label_smoothing: float = 0.1,
                         focal_alpha: float = 0.25, focal_gamma: float = 2.0,
                         class_weights: Optional[torch.Tensor] = None, device: str = "cuda") -> nn.Module:
    name = loss_name.lower()
    if class_weights is not None:
        class_weights = class_weights.to(device)
    if name == "cross_entropy":
        if label_smoothing > 0:
            return LabelSmoothingCrossEntropy(smoothing=label_smoothing, weight=class_weights, reduction="mean",
                                              num_classes=num_classes)
        return CrossEntropyLoss(weight=class_weights, reduction="mean", num_classes=num_classes)
    if name == "focal_loss":
        return FocalLoss(alpha=focal_alpha, gamma=focal_gamma, weight=class_weights, reduction="mean", num_classes=num_classes)
    raise ValueError(f"Unknown loss function: {name}. Supported: cross_entropy, focal_loss")
