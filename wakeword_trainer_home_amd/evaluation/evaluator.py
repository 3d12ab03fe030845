"""``ModelEvaluator`` / ``load_model_for_evaluation`` with the reference's names, signatures and result types
(``src/evaluation/evaluator.py``), running on the device from waveform to counters.

Per batch the loop is: log-mel front end (``ww_logmel_fwd``) -> eval-mode model forward -> ``ww_eval_accumulate``.  Nothing is
copied to the host inside the loop; ``ScoreRun.finish`` reads confidences, decisions, logits and counters back once.

Defined by this build, because ``src/data`` (``AudioProcessor``) is absent from the reference snapshot:

* files are read with the standard library's ``wave`` module: 16-bit PCM, mono, at ``sample_rate`` (anything else is a load
  failure); samples are scaled by 1/32768 and zero-padded or cropped at the end to ``audio_duration``;
* ``latency_ms`` is the wall time of the whole pass, read-back included, divided by the number of samples: the reference
  times each asynchronous batch launch without waiting for the device, and no per-batch wait exists here either;
* ``evaluate_files`` returns results in input order (the reference appends a batch's ``"Error"`` results before that
  batch's successful ones).
"""
import logging
import time
import wave as _wave
from dataclasses import dataclass
from pathlib import Path
from typing import Dict, List, Optional, Tuple

import numpy as np
import torch
import torch.nn as nn

from ..config.cuda_utils import enforce_cuda
from ..data.feature_extraction import FeatureExtractor
from ..training.metrics import MetricResults, MetricsCalculator
from .scoring import ScoreRun, file_threshold, roc_from_hist, roc_thresholds

logger = logging.getLogger(__name__)


@dataclass
class EvaluationResult:
    """Single file evaluation result (``evaluator.py:22-29``)."""
    filename: str
    prediction: str      # "Positive" | "Negative" | "Error"
    confidence: float
    latency_ms: float
    logits: np.ndarray


def load_wav(path, sample_rate: int, n_samples: int) -> np.ndarray:
    """16-bit PCM mono WAV at ``sample_rate`` -> float32 (n_samples,) in [-1, 1), zero-padded or cropped at the end."""
    with _wave.open(str(path), "rb") as f:
        if f.getnchannels() != 1 or f.getsampwidth() != 2 or f.getcomptype() != "NONE":
            raise ValueError(f"{path}: need 16-bit PCM mono, got {f.getnchannels()} channel(s) of {8 * f.getsampwidth()} bits")
        if f.getframerate() != sample_rate:
            raise ValueError(f"{path}: sample rate {f.getframerate()} != {sample_rate} (no resampling here)")
        pcm = np.frombuffer(f.readframes(f.getnframes()), dtype="<i2")
    out = np.zeros(n_samples, np.float32)
    m = min(n_samples, pcm.size)
    out[:m] = pcm[:m].astype(np.float32) / np.float32(32768.0)
    return out


def error_result(path) -> EvaluationResult:
    """What the reference records for a file that failed to load (``evaluator.py:186-195``)."""
    return EvaluationResult(filename=Path(path).name, prediction="Error", confidence=0.0, latency_ms=0.0,
                            logits=np.array([0.0, 0.0]))


def load_batch(paths, sample_rate: int, n_samples: int):
    """-> (waves float32 (m, n_samples), indices into ``paths`` of the m files that loaded); failures are logged."""
    waves, ok = [], []
    for i, p in enumerate(paths):
        try:
            waves.append(load_wav(p, sample_rate, n_samples))
            ok.append(i)
        except Exception as e:                     # noqa: BLE001 -- as the reference: any failure is this file's "Error"
            logger.error("Failed to load %s: %s", p, e)
    return (np.stack(waves) if waves else np.zeros((0, n_samples), np.float32)), ok


def _filename(meta, batch_idx: int, i: int) -> str:
    return Path(meta["path"]).name if "path" in meta else f"sample_{batch_idx}_{i}"


def _collate(items):
    """The reference's collate_fn (``evaluator.py:257-266``): stack the first elements, tensor the labels, list the metadata."""
    feats, labels, metas = zip(*items)
    feats = torch.stack([f if isinstance(f, torch.Tensor) else torch.as_tensor(f) for f in feats])
    return feats, torch.tensor(labels), list(metas)


class ModelEvaluator:
    def __init__(self, model: nn.Module, sample_rate: int = 16000, audio_duration: float = 1.5, device: str = "cuda",
                 feature_type: str = "mel", n_mels: int = 128, n_mfcc: int = 40, n_fft: int = 1024, hop_length: int = 160,
                 num_classes: Optional[int] = None):
        enforce_cuda()
        self.model, self.sample_rate, self.audio_duration, self.device = model, sample_rate, audio_duration, device
        self.num_classes = num_classes         # None: the width of the first batch of logits of each pass
        self.n_samples = int(sample_rate * audio_duration)
        self.model.to(device)
        self.model.eval()
        self.feature_extractor = FeatureExtractor(sample_rate=sample_rate, feature_type=feature_type, n_mels=n_mels,
                                                  n_mfcc=n_mfcc, n_fft=n_fft, hop_length=hop_length, device=device)
        self.metrics_calculator = MetricsCalculator(device=device)
        self.last_counters: Dict[str, int] = {}
        logger.info("ModelEvaluator initialized on %s", device)

    # ------------------------------------------------------------------ device loop
    def _logits(self, x: torch.Tensor) -> torch.Tensor:
        with torch.no_grad():
            return self.model(x)

    def _features(self, x: torch.Tensor) -> torch.Tensor:
        """(B,N) waveforms go through the native front end; anything else is a ready feature batch."""
        x = x.to(self.device, non_blocking=True)
        if x.dim() == 2:
            return self.feature_extractor(x)
        return x.float()

    def _add(self, run: Optional[ScoreRun], n: int, thresholds, decision: float, logits: torch.Tensor, targets=None) -> ScoreRun:
        """Queue one batch; the first batch of a pass creates the run, as wide as ``num_classes`` or as these logits."""
        if run is None:
            C = self.num_classes if self.num_classes is not None else int(logits.shape[1])
            run = ScoreRun(n, thresholds, decision, self.device, num_classes=C)
        run.add(logits, targets)
        return run

    def _finish(self, run: ScoreRun, t0: float):
        host = run.finish()
        self.last_counters = {k: host[k] for k in ("tp", "tn", "fp", "fn", "count", "bad_target", "nan_score")}
        if host["bad_target"]:
            logger.warning("%d target(s) outside [0, %d]: counted in total_samples only", host["bad_target"], run.num_classes - 1)
        if host["nan_score"]:
            logger.warning("%d sample(s) with a NaN confidence: predicted Negative", host["nan_score"])
        return host, (time.time() - t0) * 1000.0 / max(run.filled, 1)

    @staticmethod
    def _results(names, host, latency_ms: float) -> List[EvaluationResult]:
        # tolist(): Python floats / ints in one pass each (float(float32) is exact) -- the list of n result objects is the
        # one per-sample host cost of a pass
        return [EvaluationResult(filename=name, prediction="Positive" if p else "Negative", confidence=c,
                                 latency_ms=latency_ms, logits=lg)
                for name, c, p, lg in zip(names, host["conf"].tolist(), host["pred"].tolist(), host["logits"])]

    def _score_waveforms(self, waves, names, decision: float, batch_size: int) -> List[EvaluationResult]:
        if isinstance(waves, np.ndarray):
            waves = torch.from_numpy(waves)
        if waves.dim() != 2:
            raise ValueError(f"waveforms must be (n, N), got {tuple(waves.shape)}")
        if waves.dtype not in (torch.float32, torch.int16):
            raise ValueError(f"waveforms must be float32 or int16, got {waves.dtype}")
        n = waves.shape[0]
        names = [f"sample_{i}" for i in range(n)] if names is None else list(names)
        if len(names) != n:
            raise ValueError(f"{len(names)} names for {n} waveforms")
        if n == 0:
            return []
        t0 = time.time()
        run = None
        for i in range(0, n, batch_size):
            run = self._add(run, n, [decision], decision, self._logits(self._features(waves[i:i + batch_size])))
        host, latency = self._finish(run, t0)
        return self._results(names, host, latency)

    # ------------------------------------------------------------------ public interface
    def evaluate_waveforms(self, waves, names: Optional[List[str]] = None, threshold: float = 0.5,
                           batch_size: int = 32) -> List[EvaluationResult]:
        """``waves`` (n, N) float32 or int16, on the host or the device.  Decision as ``evaluate_files``: the float32
        comparison ``confidences >= threshold`` (``evaluator.py:222``)."""
        return self._score_waveforms(waves, names, file_threshold(threshold), batch_size)

    def evaluate_file(self, audio_path: Path, threshold: float = 0.5) -> EvaluationResult:
        """One file; a load failure raises, as in the reference.  Its decision compares ``confidence.item()`` with the
        Python float in double (``evaluator.py:137-138``), so the threshold is passed unrounded."""
        audio_path = Path(audio_path)
        wave = load_wav(audio_path, self.sample_rate, self.n_samples)
        return self._score_waveforms(wave[None], [audio_path.name], float(threshold), 1)[0]

    def evaluate_files(self, audio_paths: List[Path], threshold: float = 0.5, batch_size: int = 32) -> List[EvaluationResult]:
        paths = [Path(p) for p in audio_paths]
        results: List[Optional[EvaluationResult]] = [None] * len(paths)
        slots = []
        t0 = time.time()
        decision = file_threshold(threshold)
        run = None
        for i in range(0, len(paths), batch_size):
            waves, ok = load_batch(paths[i:i + batch_size], self.sample_rate, self.n_samples)
            slots += [i + k for k in ok]
            if ok:
                run = self._add(run, len(paths), [decision], decision, self._logits(self._features(torch.from_numpy(waves))))
        for i in set(range(len(paths))) - set(slots):
            results[i] = error_result(paths[i])
        if slots:
            host, latency = self._finish(run, t0)
            for i, r in zip(slots, self._results([paths[i].name for i in slots], host, latency)):
                results[i] = r
        return results

    def _run_dataset(self, dataset, thresholds, decision: float, batch_size: int):
        n = len(dataset)
        if n == 0:
            raise ValueError("empty dataset")
        logger.info("Evaluating dataset with %d samples...", n)
        t0 = time.time()
        run, names = None, []
        for batch_idx, i in enumerate(range(0, n, batch_size)):
            inputs, targets, metadata = _collate([dataset[j] for j in range(i, min(i + batch_size, n))])
            names += [_filename(m, batch_idx, k) for k, m in enumerate(metadata)]
            run = self._add(run, n, thresholds, decision, self._logits(self._features(inputs)),
                            targets.to(self.device, non_blocking=True).long())
        host, latency = self._finish(run, t0)
        return host, names, latency

    def evaluate_dataset(self, dataset, threshold: float = 0.5, batch_size: int = 32) -> Tuple[MetricResults, List[EvaluationResult]]:
        """Items are ``(features_or_waveform, label, metadata)``; a 1-D first element is a waveform.  ``MetricResults``
        come from the argmax counters, as ``MetricsCalculator.calculate`` on the collected (n,C) logits does
        (``evaluator.py:321-324``); ``prediction`` is the threshold decision (``:307``).  With more than two classes the
        positive and negative sample counts are the rows of the histogram -- the targets equal to 1 and to 0 -- because a
        sample of either class that is predicted as class 2.. is in none of the four counters."""
        decision = file_threshold(threshold)
        host, names, latency = self._run_dataset(dataset, [decision], decision, batch_size)
        metrics = MetricResults.from_counts(host["tp"], host["tn"], host["fp"], host["fn"])
        metrics.total_samples = host["count"]                 # len(targets): labels outside {0,1} count here only
        metrics.accuracy = (host["tp"] + host["tn"]) / host["count"] if host["count"] > 0 else 0.0
        if host["logits"].shape[1] > 2:
            metrics.positive_samples, metrics.negative_samples = int(host["hist"][1].sum()), int(host["hist"][0].sum())
        logger.info("Evaluation complete: %s", metrics)
        return metrics, self._results(names, host, latency)

    def get_roc_curve_data(self, dataset, batch_size: int = 32) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """(fpr, tpr, thresholds) at the reference's 100 linspace thresholds, from the device histogram."""
        thresholds = roc_thresholds()
        host, _, _ = self._run_dataset(dataset, thresholds, 0.5, batch_size)
        fpr, tpr = roc_from_hist(host["hist"])
        return fpr, tpr, thresholds


def load_model_for_evaluation(checkpoint_path: Path, device: str = "cuda") -> Tuple[nn.Module, Dict]:
    """Model + info from a checkpoint ``Trainer._save_checkpoint`` wrote (``evaluator.py:413-465``), read with the same
    restricted unpickler as ``Trainer.load_checkpoint``: tensors, plain containers, TrainingState and the config dataclasses."""
    from ..models import create_model
    from ..training.trainer import _checkpoint_safe_globals
    logger.info("Loading model from: %s", checkpoint_path)
    with torch.serialization.safe_globals(_checkpoint_safe_globals()):
        checkpoint = torch.load(checkpoint_path, map_location=device, weights_only=True)
    if "config" not in checkpoint:
        raise ValueError("Checkpoint does not contain configuration")
    config = checkpoint["config"]
    model = create_model(architecture=config.model.architecture, num_classes=config.model.num_classes, pretrained=False,
                         dropout=config.model.dropout)
    model.load_state_dict(checkpoint["model_state_dict"])
    model.to(device)
    model.eval()
    logger.info("Model loaded successfully: %s", config.model.architecture)
    info = {"epoch": checkpoint.get("epoch", 0), "val_loss": checkpoint.get("val_loss", 0.0),
            "val_metrics": checkpoint.get("val_metrics", {}), "config": config}
    return model, info
