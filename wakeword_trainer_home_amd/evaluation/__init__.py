"""Evaluation with the reference's interfaces (``src/evaluation``): ``ModelEvaluator`` / ``load_model_for_evaluation``
(``evaluator.py``) and ``RecordingScanner``, the batch form of ``MicrophoneInference`` (``inference.py``).  The score stage
after the logits runs on the device (``ww_eval_accumulate``, ``ww_wave_windows``); see DESIGN.md "Evaluation".
``DetectionScanner`` (``detection.py``) goes beyond the reference: a dense scan with smoothing, a refractory period and
triggers matched to labelled events -- false alarms per hour against miss rate (``ww_detect_accumulate``)."""
from .detection import (DetectionResult, DetectionScan, DetectionScanner, detect_counts, event_windows, match_triggers,
                        num_windows_hop, rates, smooth, trigger_windows, window_starts_hop)
from .evaluator import EvaluationResult, ModelEvaluator, load_model_for_evaluation, load_wav
from .inference import RecordingScanner, num_windows, window_starts
from .scoring import ScoreRun, bin_of, file_threshold, histogram, roc_from_hist, roc_thresholds

__all__ = ["EvaluationResult", "ModelEvaluator", "load_model_for_evaluation", "load_wav", "RecordingScanner", "num_windows",
           "window_starts", "ScoreRun", "bin_of", "file_threshold", "histogram", "roc_from_hist", "roc_thresholds",
           "DetectionResult", "DetectionScan", "DetectionScanner", "detect_counts", "event_windows", "match_triggers",
           "num_windows_hop", "rates", "smooth", "trigger_windows", "window_starts_hop"]
