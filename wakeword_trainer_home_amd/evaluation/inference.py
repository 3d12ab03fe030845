"""``RecordingScanner``: the batch form of the reference's ``MicrophoneInference`` (``src/evaluation/inference.py``) -- the
same detector run over a whole recording that is already in memory.  No sounddevice, no threads, no queues.

The reference's worker appends 100 ms blocks to a buffer and, while it holds ``chunk_samples``, takes the first
``chunk_samples`` as a chunk and drops ``chunk_samples // 2`` (``:150-153``); each chunk is divided by its own peak (``:190-191``),
turned into features, classified, and ``confidence.item() >= threshold`` decides (``:209-210``, a comparison in double).
Over a recording of ``S`` samples that is ``num_windows(S, chunk)`` windows starting at ``window_starts(S, chunk)``; here
``ww_wave_windows`` cuts and normalises all of them in one launch, the windows go through the log-mel front end and the model
in batches, ``ww_eval_accumulate`` takes the decisions with the threshold unrounded, and one read-back returns them.
"""
import logging
from typing import Callable, List, Optional, Tuple

import torch
import torch.nn as nn

from .. import _native as nat
from ..config.cuda_utils import enforce_cuda
from ..data.feature_extraction import FeatureExtractor
from .scoring import ScoreRun

logger = logging.getLogger(__name__)


def num_windows(n_samples: int, chunk: int) -> int:
    """Chunks the reference's buffer loop processes once ``n_samples`` have arrived (host arithmetic only)."""
    if chunk < 2:
        raise ValueError("chunk must be at least 2 samples")
    return 0 if n_samples < chunk else (n_samples - chunk) // (chunk // 2) + 1


def window_starts(n_samples: int, chunk: int) -> List[int]:
    """First sample of each of those chunks."""
    return [w * (chunk // 2) for w in range(num_windows(n_samples, chunk))]


class RecordingScanner:
    def __init__(self, model: nn.Module, sample_rate: int = 16000, audio_duration: float = 1.5, threshold: float = 0.5,
                 device: str = "cuda", callback: Optional[Callable] = None, feature_type: str = "mel", n_mels: int = 128,
                 n_mfcc: int = 40, n_fft: int = 1024, hop_length: int = 160, batch_size: int = 32,
                 num_classes: Optional[int] = None):
        enforce_cuda()
        self.num_classes = num_classes         # None: the width of the first batch of logits of each scan
        self.model, self.sample_rate, self.audio_duration = model, sample_rate, audio_duration
        self.chunk_samples = int(sample_rate * audio_duration)
        self.threshold, self.device, self.callback, self.batch_size = threshold, device, callback, batch_size
        self.model.to(device)
        self.model.eval()
        self.feature_extractor = FeatureExtractor(sample_rate=sample_rate, feature_type=feature_type, n_mels=n_mels,
                                                  n_mfcc=n_mfcc, n_fft=n_fft, hop_length=hop_length, device=device)
        self.detection_count = 0
        self.false_alarm_count = 0
        self.buffer_size = 0
        self.last_peaks: Optional[torch.Tensor] = None     # (W,) device tensor: the peaks of the last scan's windows

    def num_windows(self, n_samples: int) -> int:
        return num_windows(n_samples, self.chunk_samples)

    def window_starts(self, n_samples: int) -> List[int]:
        return window_starts(n_samples, self.chunk_samples)

    def scan(self, audio_1d) -> List[Tuple[float, bool]]:
        """``(confidence, is_positive)`` of every window of the recording, in window order; the callback, if any, is
        called with each pair after the read-back.  Counts add up over calls."""
        audio = torch.as_tensor(audio_1d)
        if audio.dim() != 1:
            raise ValueError(f"recording must be 1-D, got {tuple(audio.shape)}")
        audio = audio.to(self.device, non_blocking=True).float().contiguous()
        S = audio.shape[0]
        windows, peaks = nat.wave_windows(audio, self.chunk_samples)
        W = windows.shape[0]
        self.buffer_size = S - W * (self.chunk_samples // 2)      # what the reference's buffer still holds
        self.last_peaks = peaks
        if W == 0:
            return []
        run = None
        with torch.no_grad():
            for i in range(0, W, self.batch_size):
                logits = self.model(self.feature_extractor(windows[i:i + self.batch_size]))
                if run is None:
                    C = self.num_classes if self.num_classes is not None else int(logits.shape[1])
                    run = ScoreRun(W, [self.threshold], self.threshold, self.device, num_classes=C)
                run.add(logits)
        host = run.finish()
        results = [(float(c), bool(p)) for c, p in zip(host["conf"], host["pred"])]
        for confidence, is_positive in results:
            if self.callback:
                self.callback(confidence, is_positive)
            if is_positive:
                self.detection_count += 1
            else:
                self.false_alarm_count += 1
        return results

    def get_stats(self) -> dict:
        """The reference's keys (``inference.py:301-306``).  As there, ``false_alarm_count`` counts EVERY window that was
        not a detection -- the name is the reference's, the quantity is "non-positive windows"; it is kept as is.
        ``is_recording`` is always False and ``buffer_size`` is what the reference's buffer would still hold after the last
        scanned recording."""
        return {"detection_count": self.detection_count, "false_alarm_count": self.false_alarm_count, "is_recording": False,
                "buffer_size": self.buffer_size}
