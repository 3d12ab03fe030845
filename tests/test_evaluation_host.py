"""CPU: the host half of the evaluation package -- the bin rule and the ROC finish that the device histogram feeds, the
window arithmetic of the recording scan, the WAV loader and the checkpoint loader.  No GPU is touched."""
import ctypes
import wave

import numpy as np
import pytest
import torch

from tests.evaluation_cases import (F32, F64, adversarial_confidences, predictions_at, restated_roc, roc_thresholds,
                                    rounds_down, simulated_chunks)


def _targets(n, kind):
    if kind == "mixed":
        return np.resize(np.array([0, 1, 1, 0, 2, 1, 0, -1, 0, 1, 0], np.int64), n)
    return np.full(n, {"no_positive": 0, "no_negative": 1}[kind], np.int64)


@pytest.mark.parametrize("kind", ["mixed", "no_positive", "no_negative"])
def test_bin_rule_and_roc_finish_equal_the_threshold_loop(kind):
    from wakeword_trainer_home_amd.evaluation import bin_of, histogram, roc_from_hist, roc_thresholds as pkg_thr
    thr = roc_thresholds()
    assert np.array_equal(pkg_thr(), thr)
    conf = adversarial_confidences()
    targets = _targets(conf.size, kind)
    bins = bin_of(conf, thr)
    assert bins.dtype == np.int32
    assert np.array_equal(bins, predictions_at(conf, thr).sum(axis=0))           # "entries t with float64(conf) >= t"
    assert bins[np.isnan(conf)].tolist() == [0]
    hist = histogram(bins, targets, thr.size)
    assert hist.shape == (2, 101) and hist.dtype == np.int64
    assert hist.sum() == np.isin(targets, (0, 1)).sum()
    fpr, tpr = roc_from_hist(hist)
    ref_fpr, ref_tpr = restated_roc(conf, targets, thr)
    assert fpr.dtype == F64 and tpr.dtype == F64
    assert np.array_equal(fpr, ref_fpr) and np.array_equal(tpr, ref_tpr)
    if kind == "no_positive":
        assert not tpr.any() and fpr.any()
    if kind == "no_negative":
        assert not fpr.any() and tpr.any()


def test_the_three_comparison_semantics_differ_at_the_float32_neighbours():
    """51 of the 100 thresholds round downwards in float32; at conf == float32(t) the float32 comparison (what
    ``confidences >= threshold`` does with a Python float) says positive and the float64 one (the ROC loop, ``.item()``)
    says negative.  ``file_threshold`` is the float64 table entry that reproduces the float32 comparison."""
    from wakeword_trainer_home_amd.evaluation import file_threshold
    thr = roc_thresholds()
    down = rounds_down(thr)
    assert down.sum() == 51
    conf = adversarial_confidences()
    for t, d in zip(thr, down):
        c = np.array([F32(t)], F32)
        as_f32 = bool(c[0] >= F32(t))
        as_f64 = bool(predictions_at(c, [t])[0, 0])
        assert as_f32 and as_f64 == (not d)
        ft = file_threshold(float(t))
        assert isinstance(ft, float) and ft == float(F32(t))
        # NumPy's own float32-array >= Python-float comparison, on every adversarial value
        with np.errstate(invalid="ignore"):
            assert np.array_equal(conf >= float(t), predictions_at(conf, [ft])[0])


@pytest.mark.parametrize("chunk", [250, 251])
def test_window_arithmetic_equals_the_buffer_loop(chunk):
    from wakeword_trainer_home_amd import _native
    from wakeword_trainer_home_amd.evaluation import num_windows, window_starts
    for S in range(0, 5 * chunk + 1):
        starts, left = simulated_chunks(S, chunk)
        assert window_starts(S, chunk) == starts, S
        assert num_windows(S, chunk) == len(starts), S
        assert S - len(starts) * (chunk // 2) == left, S
        assert all(s + chunk <= S for s in starts)
    for S in (0, chunk - 1, chunk, 3 * chunk + 1, 5 * chunk):                      # the library's own host rule
        assert _native.wave_num_windows(S, chunk) == num_windows(S, chunk)
    assert _native.wave_num_windows(60000, 24000) == 4


def _write_wav(path, pcm, rate=16000, channels=1, width=2):
    with wave.open(str(path), "wb") as f:
        f.setnchannels(channels)
        f.setsampwidth(width)
        f.setframerate(rate)
        f.writeframes(np.asarray(pcm).tobytes())


def test_wav_loader_pads_crops_and_reports_errors(tmp_path):
    from wakeword_trainer_home_amd.evaluation import load_wav
    from wakeword_trainer_home_amd.evaluation.evaluator import error_result, load_batch
    rng = np.random.default_rng(0)
    short, long_ = rng.integers(-32768, 32768, 100).astype("<i2"), rng.integers(-32768, 32768, 400).astype("<i2")
    short[0], short[1] = -32768, 32767
    _write_wav(tmp_path / "short.wav", short)
    _write_wav(tmp_path / "long.wav", long_)
    _write_wav(tmp_path / "rate.wav", short, rate=8000)
    _write_wav(tmp_path / "stereo.wav", np.repeat(short, 2), channels=2)
    (tmp_path / "broken.wav").write_bytes(b"not a wav file")
    a = load_wav(tmp_path / "short.wav", 16000, 240)
    assert a.dtype == F32 and a.shape == (240,)
    assert np.array_equal(a[:100], short.astype(F32) / F32(32768)) and not a[100:].any()       # zero-padded at the end
    assert a[0] == -1.0 and a[1] == F32(32767 / 32768)
    b = load_wav(tmp_path / "long.wav", 16000, 240)
    assert np.array_equal(b, long_[:240].astype(F32) / F32(32768))                             # cropped at the end
    for bad in ("rate.wav", "stereo.wav", "broken.wav", "missing.wav"):
        with pytest.raises(Exception):
            load_wav(tmp_path / bad, 16000, 240)
    names = ["short.wav", "broken.wav", "long.wav", "missing.wav", "rate.wav"]
    waves, ok = load_batch([tmp_path / n for n in names], 16000, 240)
    assert ok == [0, 2] and waves.shape == (2, 240) and np.array_equal(waves[0], a) and np.array_equal(waves[1], b)
    none, ok = load_batch([tmp_path / "broken.wav"], 16000, 240)
    assert ok == [] and none.shape == (0, 240)
    r = error_result(tmp_path / "broken.wav")
    assert (r.filename, r.prediction, r.confidence, r.latency_ms) == ("broken.wav", "Error", 0.0, 0.0)
    assert np.array_equal(r.logits, np.array([0.0, 0.0]))


def test_checkpoint_without_configuration_is_refused(tmp_path):
    from wakeword_trainer_home_amd.evaluation import load_model_for_evaluation
    path = tmp_path / "no_config.pt"
    torch.save({"epoch": 3, "model_state_dict": {}, "val_loss": 0.5}, path)
    with pytest.raises(ValueError, match="Checkpoint does not contain configuration"):
        load_model_for_evaluation(path, device="cpu")


def test_evaluation_result_and_native_layout():
    import dataclasses
    from wakeword_trainer_home_amd import _native
    from wakeword_trainer_home_amd.evaluation import EvaluationResult
    assert [f.name for f in dataclasses.fields(EvaluationResult)] == ["filename", "prediction", "confidence", "latency_ms",
                                                                      "logits"]
    assert _native.EVAL_COUNTERS[:7] == ("tp", "tn", "fp", "fn", "count", "bad_target", "nan_score")
    assert len(_native.EVAL_COUNTERS) == 8 and _native.ABI_VERSION == 17
    assert (_native.SCORE_LOGITS, _native.SCORE_CONF, _native.EVAL_MAX_THRESHOLDS) == (0, 1, 1024)
    lib = ctypes.CDLL(str(_native.lib_path()))
    assert all(hasattr(lib, n) for n in ("ww_eval_accumulate", "ww_wave_windows", "ww_wave_num_windows"))
