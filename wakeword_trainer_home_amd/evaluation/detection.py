"""``DetectionScanner``: the dense detection scan -- how often a model fires on hours of audio without the keyword, and how
many keywords it misses at that rate.  The reference has no counterpart: its ``MicrophoneInference`` (and ``RecordingScanner``
here) decides every half-overlapping window on its own and calls every non-positive window a "false alarm".

A recording of ``S`` samples holds ``num_windows_hop(S, chunk, hop)`` windows.  They are cut by slab on the device
(``ww_wave_windows_at``, or ``ww_feat_windows`` from a feature map computed once), run through the model, scored by ``ScoreRun``,
and ``ww_detect_accumulate`` then smooths the confidences, runs one trigger machine with a refractory period per threshold,
and matches the triggers against labelled keyword occurrences.  One read-back per recording, no per-batch synchronisation.

The law (DESIGN.md "Evaluation"; the functions of this module restate it in NumPy and the tests hold the kernels to them):

* smoothing: ``s_w = float32((0.0 + sum of float64(conf_j), j = max(0, w-M+1) .. w, ascending) / count)``; a NaN propagates;
* triggers, per threshold ``t``: ``next_ok = 0``; for ``w = 0 .. W-1``: if ``w >= next_ok`` and ``float64(s_w) >= t``, trigger
  at ``w`` and set ``next_ok = w + R``.  A NaN never triggers; the comparison is float64 on the float32 value (``scoring.py``);
* matching: events are inclusive window intervals ``[a_e, b_e]``, ``a_e <= b_e < a_{e+1}``.  A trigger inside an event not yet
  hit by this threshold is a hit, inside an event already hit a duplicate, outside every event a false alarm.

Because of the refractory rule false alarms are NOT monotone in the threshold: a lower threshold can trigger earlier, and its
refractory period then swallows a later false alarm the higher threshold raises.  The curve is therefore counted threshold
by threshold, never by suffix sums over a histogram.
"""
import math
from dataclasses import dataclass
from typing import Callable, List, Optional

import numpy as np
import torch
import torch.nn as nn

from .. import _native as nat
from ..config.cuda_utils import enforce_cuda
from ..data.feature_extraction import FeatureExtractor
from .scoring import ScoreRun, roc_thresholds

TRIGGERS, HITS, FALSE_ALARMS, DUPLICATES = range(4)      # columns of every counts array (nat.DETECT_COUNTS)


# ------------------------------------------------------------------------------------------------ host restatement
def num_windows_hop(n_samples: int, chunk: int, hop: int) -> int:
    """Windows of ``chunk`` samples at hop ``hop`` that lie inside ``n_samples`` (host arithmetic only)."""
    if not 1 <= hop <= chunk:
        raise ValueError(f"hop must be in [1, chunk = {chunk}], got {hop}")
    return 0 if n_samples < chunk else (n_samples - chunk) // hop + 1


def window_starts_hop(n_samples: int, chunk: int, hop: int) -> List[int]:
    """First sample of each of those windows."""
    return [w * hop for w in range(num_windows_hop(n_samples, chunk, hop))]


def smooth(conf, M: int) -> np.ndarray:
    """float32 (W,): the mean of the last ``min(M, w + 1)`` confidences, summed in float64 from 0.0 in ascending window
    order, divided in float64, rounded once to float32."""
    if not 1 <= M <= nat.DETECT_MAX_SMOOTH:
        raise ValueError(f"smooth_windows must be in [1, {nat.DETECT_MAX_SMOOTH}], got {M}")
    c = np.asarray(conf, np.float32).astype(np.float64)
    W = c.size
    acc = np.zeros(W, np.float64)
    with np.errstate(invalid="ignore"):
        for k in range(min(M, W) - 1, -1, -1):              # term j = w - k: the oldest first
            acc[k:] += c[:W - k]
    count = np.minimum(np.arange(W) + 1, M).astype(np.float64)
    return (acc / count).astype(np.float32)


def trigger_windows(s, t: float, R: int) -> np.ndarray:
    """int64: the windows at which the machine of threshold ``t`` triggers on the smoothed sequence ``s``."""
    if R < 1:
        raise ValueError(f"the refractory length must be at least one window, got {R}")
    with np.errstate(invalid="ignore"):
        cand = np.flatnonzero(np.asarray(s, np.float32).astype(np.float64) >= np.float64(t))
    if R == 1 or cand.size == 0:
        return cand.astype(np.int64)
    out, next_ok = [], 0
    for w in cand.tolist():
        if w >= next_ok:
            out.append(w)
            next_ok = w + R
    return np.asarray(out, np.int64)


def _checked_events(events) -> np.ndarray:
    ev = np.zeros((0, 2), np.int64) if events is None else np.asarray(events, np.int64).reshape(-1, 2)
    if ev.size and ((ev[:, 0] > ev[:, 1]).any() or (ev[:, 0] < 0).any() or (ev[1:, 0] <= ev[:-1, 1]).any()):
        raise ValueError("events must be inclusive window intervals [a, b] with 0 <= a_e <= b_e < a_{e+1}")
    return ev


def match_triggers(triggers, events) -> np.ndarray:
    """int64 (4,) = triggers, hits, false alarms, duplicates of one machine's trigger windows against the events."""
    tw, ev = np.asarray(triggers, np.int64), _checked_events(events)
    if ev.shape[0] == 0:
        return np.array([tw.size, 0, tw.size, 0], np.int64)
    e = np.searchsorted(ev[:, 0], tw, side="right") - 1            # the last event starting at or before the trigger
    inside = (e >= 0) & (tw <= ev[np.maximum(e, 0), 1])
    hits = np.unique(e[inside]).size
    return np.array([tw.size, hits, int((~inside).sum()), int(inside.sum()) - hits], np.int64)


def detect_counts(conf, M: int, R: int, thresholds, events) -> np.ndarray:
    """int64 (K,4): what ``ww_detect_accumulate`` adds to ``counts`` for one recording."""
    s = smooth(conf, M)
    return np.stack([match_triggers(trigger_windows(s, t, R), events) for t in np.asarray(thresholds, np.float64).reshape(-1)])


def event_windows(events_s, S: int, sample_rate: int, chunk: int, hop: int, tolerance_s: float):
    """Keyword occurrences in seconds -> ``(intervals, n_events)``.  A trigger's time is the END of its window,
    ``(w * hop + chunk) / sample_rate``; the event ``[t0, t1]`` owns the windows whose end time lies in
    ``[t0, t1 + tolerance_s]``, clipped to ``[0, W - 1]``.  Events are sorted by start; a range is cut where the next one's
    begins.  ``intervals`` is int32 (E',2) of the ranges left non-empty, ``n_events`` counts every event: one whose range is
    empty can only be missed.  The comparisons are made on the float64 end time as written above, so a window that ends
    exactly at ``t0`` or at ``t1 + tolerance_s`` belongs to the event."""
    ev = np.zeros((0, 2), np.float64) if events_s is None else np.asarray(events_s, np.float64).reshape(-1, 2)
    if not np.isfinite(ev).all() or (ev[:, 1] < ev[:, 0]).any() or not tolerance_s >= 0:
        raise ValueError("events must be finite (t0, t1) pairs in seconds with t0 <= t1; the tolerance must be >= 0")
    W = num_windows_hop(S, chunk, hop)
    ev = ev[np.lexsort((ev[:, 1], ev[:, 0]))]
    end = lambda w: (w * hop + chunk) / sample_rate
    lo, hi = ev[:, 0], ev[:, 1] + tolerance_s
    a = np.ceil((lo * sample_rate - chunk) / hop)              # within one window of the answer: settle it on end()
    a = np.where(end(a - 1) >= lo, a - 1, a)
    a = np.maximum(np.where(end(a) < lo, a + 1, a), 0.0)
    b = np.floor((hi * sample_rate - chunk) / hop)
    b = np.where(end(b + 1) <= hi, b + 1, b)
    b = np.minimum(np.where(end(b) > hi, b - 1, b), W - 1.0)
    if ev.shape[0] > 1:
        b[:-1] = np.minimum(b[:-1], a[1:] - 1.0)
    keep = a <= b
    return np.stack([a[keep], b[keep]], axis=1).astype(np.int32).reshape(-1, 2), int(ev.shape[0])


def rates(counts, n_events: int, hours: float):
    """``(fa_per_hour, miss_rate)`` float64 from counts (..., 4); a zero denominator gives 0.0, as the reference's ROC does."""
    counts = np.asarray(counts, np.int64)
    fa = counts[..., FALSE_ALARMS] / hours if hours > 0 else np.zeros(counts.shape[:-1], np.float64)
    miss = (n_events - counts[..., HITS]) / n_events if n_events > 0 else np.zeros(counts.shape[:-1], np.float64)
    return np.asarray(fa, np.float64), np.asarray(miss, np.float64)


# ------------------------------------------------------------------------------------------------------ results
@dataclass
class DetectionScan:
    """One recording.  ``conf`` / ``smoothed`` float32 (W,); ``trigger_windows`` int64 and ``trigger_times`` float64 seconds
    (window ends) of the decision threshold's triggers -- the first ``max_triggers`` of ``n_triggers``; ``counts`` int64 (K,4)
    and ``decision_counts`` int64 (4,) in the order of ``nat.DETECT_COUNTS``; ``n_events`` counts every labelled event."""
    conf: np.ndarray
    smoothed: np.ndarray
    trigger_windows: np.ndarray
    trigger_times: np.ndarray
    n_triggers: int
    counts: np.ndarray
    decision_counts: np.ndarray
    n_events: int
    seconds: float


@dataclass
class DetectionResult:
    """Totals over every recording scanned since the last ``reset``."""
    hours: float
    n_events: int
    thresholds: np.ndarray
    counts: np.ndarray                 # int64 (K,4)
    fa_per_hour: np.ndarray            # float64 (K,)
    miss_rate: np.ndarray              # float64 (K,)
    threshold: float
    decision_counts: np.ndarray        # int64 (4,)
    decision_fa_per_hour: float
    decision_miss_rate: float

    def operating_point(self, max_fa_per_hour: float) -> Optional[dict]:
        """Among the thresholds whose false alarms per hour are within the budget, the one with the lowest miss rate; ties
        go to the lowest threshold.  ``None`` when no threshold is within budget."""
        ok = np.flatnonzero(self.fa_per_hour <= max_fa_per_hour)
        if ok.size == 0:
            return None
        k = int(ok[np.argmin(self.miss_rate[ok])])             # argmin returns the first, i.e. lowest, threshold of a tie
        return {"index": k, "threshold": float(self.thresholds[k]), "fa_per_hour": float(self.fa_per_hour[k]),
                "miss_rate": float(self.miss_rate[k])}


# ------------------------------------------------------------------------------------------------------ the scanner
class DetectionScanner:
    """Scan whole recordings at a dense hop and count triggers, hits, false alarms and duplicates per threshold.

    ``features="window"`` (default) computes what the reference's detector computes for a window: each window is cut from
    the waveform, divided by its own peak (``normalize="window"``, the default; ``"none"`` leaves it), and goes through the
    front end on its own -- reflect padding at both window edges included.  With ``hop = chunk // 2``,
    ``smooth_windows = 1`` and a refractory period of one window the confidences and decisions are ``RecordingScanner``'s,
    bit for bit.

    ``features="stream"`` is what a deployed streaming detector computes: the front end runs ONCE over the whole recording
    (one ``ww_logmel_fwd`` call, ``B = 1``), and the windows are cut from the feature map, ``hop / hop_length`` columns apart
    (the hop must be a multiple of ``hop_length``).  Column ``t`` of window ``w`` is centred on the same sample as in window
    mode, so with normalisation off the two modes see the same samples in every frame whose ``n_fft`` support lies inside
    the window; they differ in the ``n_fft / (2 hop_length)`` frames at either edge, where window mode sees samples reflected
    at the window's edge and stream mode the recording's real neighbours.  A window cannot be divided by its own peak in this
    mode (``normalize="window"`` raises): ``"recording"`` (default) divides the recording by its peak, ``"none"`` leaves it.

    False alarms are not monotone in the threshold (module docstring): ``result().fa_per_hour`` can rise with the threshold.

    ``model`` is any module mapping features to ``(B, C)`` logits (the ``Quantized*`` runtime classes included); ``C > 2``
    scores through ``ww_eval_accumulate_classes`` as in ``RecordingScanner``."""

    def __init__(self, model: nn.Module, sample_rate: int = 16000, audio_duration: float = 1.5, hop_seconds: float = 0.1,
                 thresholds=None, threshold: float = 0.5, smooth_windows: int = 1, refractory_seconds: Optional[float] = None,
                 features: str = "window", normalize: Optional[str] = None, tolerance_seconds: Optional[float] = None,
                 device: str = "cuda", callback: Optional[Callable] = None, feature_type: str = "mel", n_mels: int = 128,
                 n_mfcc: int = 40, n_fft: int = 1024, hop_length: int = 160, batch_size: int = 512,
                 num_classes: Optional[int] = None, max_triggers: int = 4096):
        enforce_cuda()
        if features not in ("window", "stream"):
            raise ValueError(f"features must be 'window' or 'stream', got {features!r}")
        if normalize is None:
            normalize = "window" if features == "window" else "recording"
        allowed = ("window", "none") if features == "window" else ("recording", "none")
        if normalize not in allowed:
            raise ValueError(f"features={features!r} takes normalize in {allowed}, got {normalize!r}")
        self.model, self.sample_rate, self.audio_duration = model, sample_rate, audio_duration
        self.chunk_samples = int(sample_rate * audio_duration)
        self.hop_samples = int(round(hop_seconds * sample_rate))
        if not 1 <= self.hop_samples <= self.chunk_samples:
            raise ValueError(f"hop_seconds = {hop_seconds} is {self.hop_samples} samples: must be in [1, {self.chunk_samples}]")
        if features == "stream" and self.hop_samples % hop_length:
            raise ValueError(f"stream features need a window hop ({self.hop_samples} samples) that is a multiple of "
                             f"hop_length = {hop_length}")
        self.features, self.normalize = features, normalize
        thr = roc_thresholds() if thresholds is None else np.ascontiguousarray(thresholds, np.float64)
        if thr.ndim != 1 or not 1 <= thr.size <= nat.EVAL_MAX_THRESHOLDS or np.isnan(thr).any() or np.any(np.diff(thr) < 0):
            raise ValueError(f"thresholds must be 1 to {nat.EVAL_MAX_THRESHOLDS} ascending float64 values")
        self.thresholds, self.threshold = thr, float(threshold)
        if not 1 <= smooth_windows <= nat.DETECT_MAX_SMOOTH:
            raise ValueError(f"smooth_windows must be in [1, {nat.DETECT_MAX_SMOOTH}], got {smooth_windows}")
        self.smooth_windows = int(smooth_windows)
        refractory_seconds = audio_duration if refractory_seconds is None else refractory_seconds
        if not refractory_seconds >= 0:
            raise ValueError(f"refractory_seconds must be >= 0, got {refractory_seconds}")
        # a trigger at w blocks the windows that begin less than the refractory period after it
        self.refractory_windows = min(max(1, math.ceil(int(round(refractory_seconds * sample_rate)) / self.hop_samples)),
                                      2 ** 31 - 1)
        self.tolerance_seconds = audio_duration if tolerance_seconds is None else float(tolerance_seconds)
        self.device, self.callback, self.batch_size, self.num_classes = device, callback, int(batch_size), num_classes
        if self.batch_size < 1 or max_triggers < 0:
            raise ValueError("batch_size must be >= 1 and max_triggers >= 0")
        self.max_triggers = int(max_triggers)
        self.model.to(device)
        self.model.eval()
        self.feature_extractor = FeatureExtractor(sample_rate=sample_rate, feature_type=feature_type, n_mels=n_mels,
                                                  n_mfcc=n_mfcc, n_fft=n_fft, hop_length=hop_length, device=device)
        self._thr_dev = torch.from_numpy(thr).to(device)
        self.reset()

    # ---- geometry
    def num_windows(self, n_samples: int) -> int:
        return num_windows_hop(n_samples, self.chunk_samples, self.hop_samples)

    def window_time(self, w):
        """The time a trigger at window ``w`` is reported at: the end of the window, in seconds."""
        return (np.asarray(w, np.float64) * self.hop_samples + self.chunk_samples) / self.sample_rate

    def event_windows(self, events_s, n_samples: int):
        return event_windows(events_s, n_samples, self.sample_rate, self.chunk_samples, self.hop_samples, self.tolerance_seconds)

    # ---- the two ways to the model's input
    def slab_features(self, audio: torch.Tensor):
        """-> ``(W, slab)``: ``slab(w0, n)`` returns the model input of windows ``w0 .. w0+n-1`` of the float32 device
        recording ``audio``.  Nothing is synchronised."""
        S = audio.shape[0]
        W = self.num_windows(S)
        if self.features == "window":
            def slab(w0, n):
                windows, _ = nat.wave_windows_at(audio, self.chunk_samples, self.hop_samples, w0, n,
                                                 normalize=self.normalize == "window")
                return self.feature_extractor(windows)
            return W, slab
        if W == 0:
            return 0, None
        if self.normalize == "recording":                 # one window of length S in ww_wave_windows' law
            audio = nat.wave_windows_at(audio, S, S, 0, 1, normalize=True)[0][0]
        feat = self.feature_extractor(audio)[0]            # (F, S // hop_length + 1)
        hl = self.feature_extractor.hop_length
        Tw, step = self.chunk_samples // hl + 1, self.hop_samples // hl
        return W, lambda w0, n: nat.feat_windows(feat, Tw, step, w0, n)

    # ---- scanning
    def scan(self, audio_1d, events=None) -> DetectionScan:
        """Scan one recording.  ``events``: (t0, t1) pairs in seconds, the labelled keyword occurrences (None: none).  The
        callback, if any, is called with ``(time_s, smoothed_confidence)`` of every decision-threshold trigger after the
        read-back.  Totals add up over calls."""
        audio = torch.as_tensor(audio_1d)
        if audio.dim() != 1:
            raise ValueError(f"recording must be 1-D, got {tuple(audio.shape)}")
        audio = audio.to(self.device, non_blocking=True).float().contiguous()
        S, K = audio.shape[0], self.thresholds.size
        intervals, n_events = self.event_windows(events, S)
        W, slab = self.slab_features(audio)
        seconds = S / self.sample_rate
        if W == 0:
            z = np.zeros(0, np.float32)
            scan = DetectionScan(z, z.copy(), np.zeros(0, np.int64), np.zeros(0, np.float64), 0, np.zeros((K, 4), np.int64),
                                 np.zeros(4, np.int64), n_events, seconds)
        else:
            run = None
            with torch.no_grad():
                for w0 in range(0, W, self.batch_size):
                    logits = self.model(slab(w0, min(self.batch_size, W - w0)))
                    if run is None:
                        C = self.num_classes if self.num_classes is not None else int(logits.shape[1])
                        run = ScoreRun(W, [self.threshold], self.threshold, self.device, num_classes=C)
                    run.add(logits)
            # the detector's outputs share one byte buffer: smoothed f32 (W) | triggers i32 (max) | n_triggers i32 (1) come
            # after the 64-bit counters, so every view stays aligned and the read-back is one copy
            T = self.max_triggers
            buf = torch.zeros(8 * (4 * K + 4) + 4 * (W + T + 1), dtype=torch.uint8, device=self.device)
            counts, dcounts = buf[:32 * K].view(torch.int64), buf[32 * K:32 * K + 32].view(torch.int64)
            rest = buf[32 * K + 32:].view(torch.int32)
            smoothed, trig, n_trig = rest[:W].view(torch.float32), rest[W:W + T], rest[W + T:]
            ev_dev = torch.from_numpy(intervals).to(self.device) if intervals.shape[0] else None
            nat.detect_accumulate(run.conf, self.smooth_windows, self.refractory_windows, self._thr_dev, self.threshold, ev_dev,
                                  smoothed, counts, dcounts, trig, n_trig)
            host = buf.cpu().numpy()
            conf = run.finish()["conf"].copy()
            h64 = host[:32 * K + 32].view(np.int64)
            h32 = host[32 * K + 32:].view(np.int32)
            n = int(h32[W + T])
            tw = h32[W:W + min(n, T)].astype(np.int64)
            scan = DetectionScan(conf, h32[:W].view(np.float32).copy(), tw, self.window_time(tw), n,
                                 h64[:4 * K].reshape(K, 4).copy(), h64[4 * K:].copy(), n_events, seconds)
        self._counts += scan.counts
        self._decision_counts += scan.decision_counts
        self._n_events += n_events
        self._seconds += seconds
        if self.callback:
            for w, t in zip(scan.trigger_windows, scan.trigger_times):
                self.callback(float(t), float(scan.smoothed[w]))
        return scan

    def result(self) -> DetectionResult:
        hours = self._seconds / 3600.0
        fa, miss = rates(self._counts, self._n_events, hours)
        dfa, dmiss = rates(self._decision_counts, self._n_events, hours)
        return DetectionResult(hours, self._n_events, self.thresholds.copy(), self._counts.copy(), fa, miss, self.threshold,
                               self._decision_counts.copy(), float(dfa), float(dmiss))

    def reset(self):
        self._counts = np.zeros((self.thresholds.size, 4), np.int64)
        self._decision_counts = np.zeros(4, np.int64)
        self._n_events, self._seconds = 0, 0.0
