"""The score stage of evaluation: what happens to a batch of logits.

The reference does it on the host, batch by batch: ``logits.cpu()``, ``probabilities[:, 1].cpu().numpy()``, a comparison with
the threshold (``src/evaluation/evaluator.py:220-222, 305-307``), and for the ROC curve a loop over 100 thresholds
(``:389-408``).  Here one kernel launch per batch (``ww_eval_accumulate``) writes the per-sample confidence, decision and ROC
bin into dataset-long device buffers and adds to integer counters; ``ScoreRun.finish`` reads all of it back once.

Every comparison on the device is ``float64(conf) >= t`` on the float32 confidence.  The reference's three comparison
semantics are then three choices of ``t`` made here, on the host (DESIGN.md "Evaluation"):

* ROC loop: ``float32 array >= np.float64 scalar`` compares in float64 under NumPy 2 -> the linspace itself;
* ``confidences >= threshold`` with a Python float (``evaluate_files`` / ``evaluate_dataset``) compares in float32
  -> ``file_threshold(threshold)`` = ``float64(float32(threshold))``;
* ``confidence.item() >= threshold`` (``evaluate_file``, ``MicrophoneInference._process_chunk``) compares in double
  -> the threshold unchanged.

The host functions of this module restate the device rule in NumPy; the tests hold the kernel to them.
"""
import numpy as np
import torch

from .. import _native as nat

ROC_POINTS = 100


def roc_thresholds() -> np.ndarray:
    """The reference's ROC thresholds (``evaluator.py:389``)."""
    return np.linspace(0, 1, ROC_POINTS)


def file_threshold(threshold: float) -> float:
    """The float64 value whose comparison with a float32 confidence equals NumPy's ``float32_array >= python_float``:
    a Python float is a weak scalar, so NumPy compares in float32, i.e. against the rounded threshold."""
    return float(np.float64(np.float32(threshold)))


def bin_of(conf, thresholds) -> np.ndarray:
    """Number of ``thresholds`` entries ``t`` (ascending float64) with ``float64(conf) >= t``; NaN -> 0.  int32."""
    c = np.asarray(conf, np.float32).astype(np.float64)
    b = np.searchsorted(np.asarray(thresholds, np.float64), c, side="right")
    return np.where(np.isnan(c), 0, b).astype(np.int32)


def histogram(bins, targets, n_thresholds: int) -> np.ndarray:
    """int64 (2, K+1) counts indexed [target][bin]; targets outside {0, 1} are not counted."""
    bins, targets = np.asarray(bins), np.asarray(targets)
    return np.stack([np.bincount(bins[targets == t], minlength=n_thresholds + 1) for t in (0, 1)]).astype(np.int64)


def roc_from_hist(hist):
    """(fpr, tpr) float64 (K,) from the (2, K+1) histogram: a sample is predicted positive at threshold k iff its bin is
    > k, so the counts are suffix sums (int64); a rate whose denominator is 0 is 0.0 (``evaluator.py:402-405``)."""
    hist = np.asarray(hist, np.int64)
    ge = np.cumsum(hist[:, ::-1], axis=1)[:, ::-1][:, 1:]          # [target][k] = samples of that target with bin >= k + 1
    total = hist.sum(axis=1)
    rates = [ge[t] / total[t] if total[t] > 0 else np.zeros(ge.shape[1], np.float64) for t in (0, 1)]
    return rates[0], rates[1]


class ScoreRun:
    """Device accumulators of one pass over ``n`` samples, carved from ONE byte buffer so that ``finish`` is one D2H copy:
    hist i64 (2,K+1) | counters i64 (8) | logits f32 (n,C) | conf f32 (n) | bin i32 (n) | pred u8 (n).  ``num_classes`` = C is
    the width of the logits: 2 scores through ``ww_eval_accumulate`` as always, more through ``ww_eval_accumulate_classes``."""

    def __init__(self, n: int, thresholds, decision: float, device, num_classes: int = 2):
        if isinstance(num_classes, bool) or not isinstance(num_classes, int) or not 2 <= num_classes <= nat.LOSS_MAX_CLASSES:
            raise ValueError(f"num_classes must be an int in [2, {nat.LOSS_MAX_CLASSES}], got {num_classes!r}")
        self.num_classes = num_classes
        thr = np.ascontiguousarray(thresholds, np.float64)
        if thr.ndim != 1 or not 1 <= thr.size <= nat.EVAL_MAX_THRESHOLDS or np.any(np.diff(thr) < 0) or np.isnan(thr).any():
            raise ValueError(f"thresholds must be 1 to {nat.EVAL_MAX_THRESHOLDS} ascending float64 values")
        self.n, self.K, self.decision, self.filled = int(n), thr.size, float(decision), 0
        self.thresholds = torch.from_numpy(thr).to(device)
        fields = (("hist", torch.int64, 2 * (self.K + 1)), ("counters", torch.int64, 8), ("logits", torch.float32, num_classes * self.n),
                  ("conf", torch.float32, self.n), ("bin", torch.int32, self.n), ("pred", torch.uint8, self.n))
        self._layout, off = [], 0
        for name, dt, count in fields:                       # descending element size: every view stays aligned
            nbytes = count * torch.empty((), dtype=dt).element_size()
            self._layout.append((name, dt, off, nbytes))
            off += nbytes
        self._buf = torch.zeros(off, dtype=torch.uint8, device=device)
        for name, dt, start, nbytes in self._layout:
            setattr(self, name, self._buf[start:start + nbytes].view(dt))
        self.logits = self.logits.view(self.n, num_classes)

    def add(self, scores: torch.Tensor, targets=None):
        """Queue one batch: (B,C) logits, or (B,) confidences (their logits slots stay zero).  No host synchronisation."""
        B = scores.shape[0]
        if self.filled + B > self.n:
            raise ValueError(f"ScoreRun holds {self.n} samples; batch of {B} at {self.filled} does not fit")
        scores = scores.detach().float().contiguous()
        if scores.dim() == 2:
            if scores.shape[1] != self.num_classes:
                raise ValueError(f"ScoreRun was built for num_classes = {self.num_classes}, got logits with {scores.shape[1]} columns")
            self.logits[self.filled:self.filled + B].copy_(scores)
        accumulate = nat.eval_accumulate_classes if scores.dim() == 2 and self.num_classes > 2 else nat.eval_accumulate
        accumulate(scores, targets, self.thresholds, self.decision, self.conf, self.pred, self.bin, self.filled, self.hist,
                   self.counters)
        self.filled += B

    def finish(self) -> dict:
        """The single read-back: numpy arrays of the ``filled`` samples plus ``hist`` (2,K+1) and the named counters."""
        host = self._buf.cpu().numpy()
        np_dt = {torch.int64: np.int64, torch.float32: np.float32, torch.int32: np.int32, torch.uint8: np.uint8}
        out = {name: host[start:start + nbytes].view(np_dt[dt]) for name, dt, start, nbytes in self._layout}
        m = self.filled
        res = {"hist": out["hist"].reshape(2, self.K + 1), "logits": out["logits"].reshape(self.n, self.num_classes)[:m],
               "conf": out["conf"][:m], "bin": out["bin"][:m], "pred": out["pred"][:m]}
        res.update({k: int(v) for k, v in zip(nat.EVAL_COUNTERS, out["counters"])})
        return res
