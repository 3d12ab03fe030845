"""Shared by test_evaluation_host.py and test_evaluation_gpu.py: the adversarial confidences and the reference's
evaluation arithmetic restated in this file's own words (threshold by threshold, chunk by chunk)."""
import numpy as np

F32, F64 = np.float32, np.float64
ULP_BOUND = 16 * 2.0 ** -24      # softmax confidence vs float64: two expf of 1-2 ulp each + three roundings, margin ~2x


def roc_thresholds():
    return np.linspace(0, 1, 100)


def adversarial_confidences():
    """float32: every ROC threshold rounded to float32 with both float32 neighbours, then the edges of [0,1], a subnormal,
    NaN and values outside [0,1]."""
    t32 = roc_thresholds().astype(F32)
    vals = np.stack([np.nextafter(t32, F32(-np.inf)), t32, np.nextafter(t32, F32(np.inf))], axis=1).ravel()
    extra = np.array([0.0, -0.0, 1.0, np.nextafter(F32(1), F32(0)), 1e-40, np.nan, 1.5, -0.25], F32)
    return np.concatenate([vals, extra]).astype(F32)


def rounds_down(thresholds):
    """Mask of thresholds whose float32 rounding is below them: there ``float32(t) >= t`` is true in float32, false in float64."""
    return thresholds.astype(F32).astype(F64) < thresholds


def predictions_at(conf, thresholds):
    """bool (K, n): the float64 comparison of every float32 confidence with every threshold (NaN compares false)."""
    return np.asarray(conf, F32).astype(F64)[None, :] >= np.asarray(thresholds, F64)[:, None]


def restated_roc(conf, targets, thresholds):
    """The reference's ROC loop, vectorised over the thresholds: integer counts, float64 rates, 0.0 for an empty class."""
    pred = predictions_at(conf, thresholds)
    targets = np.asarray(targets)
    pos, neg = targets == 1, targets == 0
    tp, fn = (pred & pos).sum(1), (~pred & pos).sum(1)
    fp, tn = (pred & neg).sum(1), (~pred & neg).sum(1)
    with np.errstate(invalid="ignore", divide="ignore"):
        tpr = np.where(tp + fn > 0, tp / (tp + fn), 0.0)
        fpr = np.where(fp + tn > 0, fp / (fp + tn), 0.0)
    return fpr.astype(F64), tpr.astype(F64)


def simulated_chunks(n_samples, chunk, block=17):
    """Start offsets of the chunks a growing buffer yields: samples arrive in blocks; while the buffer holds a chunk, take
    its first ``chunk`` samples and drop ``chunk // 2``.  Returns (starts, samples left in the buffer)."""
    starts, buffered, dropped, arrived = [], 0, 0, 0
    while True:
        while buffered >= chunk:
            starts.append(dropped)
            buffered -= chunk // 2
            dropped += chunk // 2
        if arrived == n_samples:
            return starts, buffered
        step = min(block, n_samples - arrived)
        arrived += step
        buffered += step


def host_windows(wave, chunk):
    """float32 (W, chunk) windows, each divided by its own peak when that is > 0, and the peaks -- NumPy float32 arithmetic."""
    starts, _ = simulated_chunks(len(wave), chunk)
    out, peaks = np.zeros((len(starts), chunk), F32), np.zeros(len(starts), F32)
    for w, s in enumerate(starts):
        piece = wave[s:s + chunk]
        peak = np.max(np.abs(piece))
        peaks[w] = peak
        out[w] = piece / peak if peak > 0 else piece
    return out, peaks


def softmax64(logits):
    """Positive-class probability of float32 (n,2) logits in float64."""
    z = np.asarray(logits, F32).astype(F64)
    m = z.max(axis=1, keepdims=True)
    e = np.exp(z - m)
    return e[:, 1] / e.sum(axis=1)
