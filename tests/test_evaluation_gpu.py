"""GPU: the evaluation path on the device -- ww_eval_accumulate and ww_wave_windows against the host rules restated in
tests/evaluation_cases.py, then ModelEvaluator / RecordingScanner / load_model_for_evaluation end to end."""
import numpy as np
import pytest
import torch

from tests.evaluation_cases import (F32, F64, ULP_BOUND, adversarial_confidences, host_windows, predictions_at, restated_roc,
                                    roc_thresholds, rounds_down, softmax64)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")


def _bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def _table(K):
    return {1: np.array([0.5]), 100: roc_thresholds(), 1024: np.linspace(0, 1, 1024)}[K]


def _accumulators(n, K):
    z = lambda dt, m, fill=0: torch.full((m,), fill, dtype=dt, device=DEV)
    return dict(conf=z(torch.float32, n, -7.0), pred=z(torch.uint8, n, 9), bins=z(torch.int32, n, -5),
                hist=z(torch.int64, 2 * (K + 1)), counters=z(torch.int64, 8))


def _host_counts(pred_class, targets):
    t, p = np.asarray(targets), np.asarray(pred_class).astype(bool)
    return dict(tp=int((p & (t == 1)).sum()), tn=int((~p & (t == 0)).sum()), fp=int((p & (t == 0)).sum()),
                fn=int((~p & (t == 1)).sum()), bad_target=int((~np.isin(t, (0, 1))).sum()))


@pytest.mark.parametrize("K", [1, 100, 1024])
@pytest.mark.parametrize("B", [1, 63, 64, 65, 1025])
def test_eval_accumulate_confidence_mode(B, K):
    """Three calls into the same accumulators at offsets 0, B, 2B: per-sample outputs land at their offsets, the counters
    hold the sum, all of it equal to the host rule exactly."""
    from wakeword_trainer_home_amd import _native as nat
    from wakeword_trainer_home_amd.evaluation import bin_of, file_threshold, histogram
    thr = _table(K)
    decision = 0.5 if K == 1 else file_threshold(float(thr[np.flatnonzero(rounds_down(thr))[K // 3]]))
    adv = adversarial_confidences()
    pad = 5
    acc = _accumulators(3 * B + pad, K)
    thr_dev = torch.from_numpy(thr).to(DEV)
    confs, targets = [], []
    for call in range(3):
        c = np.resize(np.roll(adv, -101 * call - B), B)
        t = np.resize(np.roll(np.array([0, 1, 1, 0, 2, 1, 0, -1, 0, 1, 0], np.int64), call), B)
        confs.append(c)
        targets.append(t)
        nat.eval_accumulate(torch.from_numpy(c).to(DEV), torch.from_numpy(t).to(DEV), thr_dev, decision, acc["conf"],
                            acc["pred"], acc["bins"], call * B, acc["hist"], acc["counters"])
    conf, t = np.concatenate(confs), np.concatenate(targets)
    got = {k: v.cpu().numpy() for k, v in acc.items()}
    assert np.array_equal(_bits(got["conf"][:3 * B]), _bits(conf))                       # a copy, NaN included
    exp_pred = predictions_at(conf, [decision])[0]
    assert np.array_equal(got["pred"][:3 * B], exp_pred.astype(np.uint8))
    exp_bins = bin_of(conf, thr)
    assert np.array_equal(got["bins"][:3 * B], exp_bins)
    assert np.array_equal(exp_bins, predictions_at(conf, thr).sum(axis=0))
    assert (got["conf"][3 * B:] == -7.0).all() and (got["pred"][3 * B:] == 9).all() and (got["bins"][3 * B:] == -5).all()
    assert np.array_equal(got["hist"].reshape(2, K + 1), histogram(exp_bins, t, K))
    exp = _host_counts(exp_pred, t)                                                      # predicted class = pred in this mode
    c = dict(zip(nat.EVAL_COUNTERS, got["counters"].tolist()))
    assert {k: c[k] for k in exp} == exp
    assert c["count"] == 3 * B and c["nan_score"] == int(np.isnan(conf).sum()) and c["reserved"] == 0


def test_rounded_and_unrounded_decision_thresholds_differ_where_the_host_rule_says():
    """pred with float64(float32(t)) (the float32 comparison of evaluate_files) against pred with t itself (the double
    comparison of .item()): they differ exactly at conf == float32(t) of the 51 thresholds that round downwards."""
    from wakeword_trainer_home_amd import _native as nat
    from wakeword_trainer_home_amd.evaluation import file_threshold
    thr, conf = roc_thresholds(), adversarial_confidences()
    n = conf.size
    conf_dev, thr_dev = torch.from_numpy(conf).to(DEV), torch.from_numpy(thr).to(DEV)
    preds = {}
    for mode, rule in (("f32", file_threshold), ("f64", float)):
        acc = _accumulators(n * thr.size, thr.size)
        for k, t in enumerate(thr):
            nat.eval_accumulate(conf_dev, None, thr_dev, rule(float(t)), acc["conf"], acc["pred"], None, k * n, acc["hist"],
                                acc["counters"])
        preds[mode] = acc["pred"].cpu().numpy().reshape(thr.size, n).astype(bool)
        assert not acc["hist"].any() and (acc["bins"] == -5).all()                       # no targets, no bin buffer
        assert acc["counters"].cpu().tolist()[4:6] == [n * thr.size, 0]
    with np.errstate(invalid="ignore"):
        as_f32 = np.stack([conf >= F32(t) for t in thr])
    assert np.array_equal(preds["f32"], as_f32)
    assert np.array_equal(preds["f64"], predictions_at(conf, thr))
    differ = preds["f32"] != preds["f64"]
    expected = rounds_down(thr)[:, None] & (conf[None, :] == thr.astype(F32)[:, None])
    assert np.array_equal(differ, expected)
    assert (differ.any(axis=1) == rounds_down(thr)).all() and differ.any(axis=1).sum() == 51


def _logit_cases():
    diffs = [0.0] + [s * d for d in (1e-3, 5.0, 16.0, 17.0, 80.0, 120.0) for s in (1.0, -1.0)]
    rows = [(base, base + d) for base in (0.0, 1.5) for d in diffs]
    rng = np.random.default_rng(5)
    rows += [tuple(r) for r in rng.normal(0, 12, (200, 2))]
    special = [(2.0, 2.0), (-3.5, -3.5), (np.nan, 1.0), (1.0, np.nan), (np.nan, np.nan), (np.inf, 0.0), (0.0, np.inf),
               (-np.inf, 0.0), (np.inf, np.inf), (0.0, -np.inf)]
    return np.array(rows, F32), np.array(special, F32), len(diffs)


def test_eval_accumulate_logits_mode():
    """Logit differences 0, +-1e-3, +-5, +-16, +-17, +-80, +-120 on two bases, 200 random pairs, ties, NaN, +-inf.
    Measured on an MI355X: the worst relative error of conf against a float64 softmax over |l1-l0| <= 80 is 1.358e-07
    (2.3 fp32 ulps; bound: 16 fp32 ulps = 9.54e-07)."""
    from wakeword_trainer_home_amd import _native as nat
    from wakeword_trainer_home_amd.evaluation import bin_of, histogram
    finite, special, n_diffs = _logit_cases()
    logits = np.concatenate([finite, special])
    n = len(logits)
    targets = np.resize(np.array([1, 0, 0, 1, 1, 0, 3, 1, 0], np.int64), n)
    thr = roc_thresholds()
    acc = _accumulators(n, thr.size)
    nat.eval_accumulate(torch.from_numpy(logits).to(DEV), torch.from_numpy(targets).to(DEV), torch.from_numpy(thr).to(DEV),
                        0.5, acc["conf"], acc["pred"], acc["bins"], 0, acc["hist"], acc["counters"])
    got = {k: v.cpu().numpy() for k, v in acc.items()}
    conf = got["conf"]
    # argmax counters == torch.argmax on the CPU (tie -> 0, NaN wins, first NaN wins)
    amax = torch.from_numpy(logits).argmax(dim=1).numpy()
    assert amax[len(finite):].tolist() == [0, 0, 0, 1, 0, 0, 1, 1, 0, 0]
    exp = _host_counts(amax, targets)
    c = dict(zip(nat.EVAL_COUNTERS, got["counters"].tolist()))
    assert {k: c[k] for k in exp} == exp and c["count"] == n
    # confidence against a float64 softmax
    d = finite[:, 1].astype(F64) - finite[:, 0].astype(F64)
    ref = softmax64(finite)
    sel = np.abs(d) <= 80
    rel = np.abs(conf[:len(finite)].astype(F64)[sel] - ref[sel]) / ref[sel]
    print(f"softmax confidence: worst relative error over |l1-l0| <= 80: {rel.max():.3e} (bound {ULP_BOUND:.3e})")
    assert rel.max() <= ULP_BOUND
    grid = conf[:2 * n_diffs]
    dg = d[:2 * n_diffs]
    assert (grid[dg >= 17] == 1.0).all() and (dg >= 17).sum() == 6                       # saturated: exactly 1 ...
    assert (grid[dg == -120] == 0.0).all() and (dg == -120).sum() == 2                   # ... and exactly 0
    assert (grid[dg == 0] == 0.5).all()
    assert ((grid[dg == 16] < 1.0) & (grid[dg == 16] > 0.999999)).all()
    # NaN / infinity follow the formula (as torch.softmax does): NaN wherever exp(l - m) meets inf - inf or a NaN
    with np.errstate(invalid="ignore"):
        ref_special = torch.softmax(torch.from_numpy(special), dim=1)[:, 1].numpy()
    assert np.array_equal(np.isnan(conf[len(finite):]), np.isnan(ref_special))
    ok = ~np.isnan(ref_special)
    assert np.array_equal(conf[len(finite):][ok], ref_special[ok])
    assert c["nan_score"] == int(np.isnan(conf).sum()) >= 5
    # decisions, bins and histogram are exact when recomputed from the kernel's own confidences
    assert np.array_equal(got["pred"], predictions_at(conf, [0.5])[0].astype(np.uint8))
    bins = bin_of(conf, thr)
    assert np.array_equal(got["bins"], bins)
    assert np.array_equal(got["hist"].reshape(2, -1), histogram(bins, targets, thr.size))


def _recording(S, chunk, rng):
    wave = (rng.normal(0, 0.2, S) * rng.choice([1e-3, 0.05, 1.0, 30.0], S)).astype(F32)
    half = chunk // 2
    if S >= 5 * half + chunk - half:
        wave[2 * half:2 * half + chunk] = 0.0                # window 2 is all zero
        wave[5 * half + 3] = np.nan                          # only the last window (4) holds the NaN
    return wave


@pytest.mark.parametrize("chunk,W", [(250, 0), (250, 1), (250, 5), (251, 0), (251, 1), (251, 5), (24000, 4)])
def test_wave_windows_equal_numpy_bit_for_bit(chunk, W):
    from wakeword_trainer_home_amd import _native as nat
    from wakeword_trainer_home_amd.evaluation import num_windows
    rng = np.random.default_rng(chunk + W)
    half = chunk // 2
    S = 60000 if chunk == 24000 else (chunk - 1 if W == 0 else chunk + (W - 1) * half + 7)
    assert num_windows(S, chunk) == W and (chunk == 24000 or S < chunk or (S - chunk) % half == 7)   # small sizes leave a remainder
    if W == 1:                                               # a tiny but normal peak: 1e-30
        wave = (rng.uniform(-1, 1, S) * 1e-30).astype(F32)
        wave[11] = F32(1e-30)
    else:
        wave = _recording(S, chunk, rng)
    out, peaks = nat.wave_windows(torch.from_numpy(wave).to(DEV), chunk)
    with np.errstate(invalid="ignore"):
        ref_out, ref_peaks = host_windows(wave, chunk)
    assert out.shape == (W, chunk) and peaks.shape == (W,)
    assert np.array_equal(_bits(out.cpu().numpy()), _bits(ref_out))
    assert np.array_equal(peaks.cpu().numpy(), ref_peaks, equal_nan=True)
    if W == 1:
        assert ref_peaks[0] == F32(1e-30) and np.abs(ref_out).max() == 1.0
    if W == 5:
        assert ref_peaks[2] == 0 and not ref_out[2].any()                                 # all-zero window stays zero
        assert np.isnan(ref_peaks[4]) and not np.isnan(ref_peaks[:4]).any()
        s = 4 * half
        assert np.array_equal(_bits(ref_out[4]), _bits(wave[s:s + chunk]))                # the NaN window is unscaled
        assert np.abs(ref_out[[0, 1, 3]]).max(axis=1).tolist() == [1.0, 1.0, 1.0]
    if chunk == 24000:
        assert np.abs(ref_out).max(axis=1).tolist() == [1.0] * 4


N, N_MELS, N_SAMPLES = 24000, 40, 37


class _Waves(torch.utils.data.Dataset):
    """37 waveforms of config-2 geometry (24000 samples -> 40 x 151 log-mel), every other item without a path."""

    def __init__(self):
        rng = np.random.default_rng(11)
        amp = rng.choice([1e-3, 0.02, 0.3, 1.0], (N_SAMPLES, 1))
        self.waves = torch.from_numpy((rng.normal(0, 1, (N_SAMPLES, N)) * amp).clip(-1, 1).astype(F32))
        self.labels = (rng.random(N_SAMPLES) < 0.4).astype(np.int64)

    def __len__(self):
        return N_SAMPLES

    def __getitem__(self, i):
        meta = {"path": f"/data/clips/clip_{i:03d}.wav"} if i % 2 == 0 else {"label": int(self.labels[i])}
        return self.waves[i], int(self.labels[i]), meta


@pytest.fixture(scope="module")
def model():
    """An untrained cnn_small answers every input alike (logit spread 1e-3): give its BatchNorm layers running statistics of
    the test's own features, then stretch and centre the classifier so that the confidences cover most of (0, 1)."""
    from wakeword_trainer_home_amd import _native as nat
    from wakeword_trainer_home_amd.models import create_model
    torch.manual_seed(4)
    m = create_model("cnn_small", dropout=0.0).to(DEV)
    feats = nat.logmel_fwd(_Waves().waves.to(DEV), nat.make_feat_cfg(n_mels=N_MELS))
    with torch.no_grad():
        m.train()
        for _ in range(30):
            m(feats)
        m.eval()
        m.classifier.weight.mul_(200.0)
        z = m(feats)
        m.classifier.bias[1] -= (z[:, 1] - z[:, 0]).mean()
    return m


@pytest.fixture(scope="module")
def evaluator(model):
    from wakeword_trainer_home_amd.evaluation import ModelEvaluator
    return ModelEvaluator(model, sample_rate=16000, audio_duration=1.5, device=DEV, n_mels=N_MELS)


def test_evaluate_dataset_and_roc_end_to_end(model, evaluator):
    """cnn_small, 37 waveforms at batch_size 16 (batches 16, 16, 5) against model(feats) called directly.
    Measured on an MI355X: worst relative confidence error 7.5e-08 against the float64 softmax of the logits; one batch
    of 37 gives confidences BITWISE EQUAL to the batches of 16 (eval-mode kernels treat every sample on its own)."""
    from wakeword_trainer_home_amd.training import MetricsCalculator
    data = _Waves()
    threshold = 0.5
    metrics, results = evaluator.evaluate_dataset(data, threshold=threshold, batch_size=16)
    fpr, tpr, thr = evaluator.get_roc_curve_data(data, batch_size=16)
    with torch.no_grad():
        direct = torch.cat([model(evaluator.feature_extractor(data.waves[i:i + 16].to(DEV))) for i in (0, 16, 32)]).cpu()
    logits = np.stack([r.logits for r in results])
    conf = np.array([r.confidence for r in results], F32)
    assert logits.dtype == F32 and np.array_equal(logits, direct.numpy())
    ref = softmax64(direct.numpy())
    rel = np.abs(conf.astype(F64) - ref) / ref
    print(f"end to end: worst relative confidence error {rel.max():.3e}; logit spread {np.ptp(direct.numpy()[:, 1] - direct.numpy()[:, 0]):.3f}")
    assert rel.max() <= ULP_BOUND
    assert np.allclose(conf, torch.softmax(direct, dim=1)[:, 1].numpy(), rtol=2 * ULP_BOUND, atol=0)
    targets = torch.from_numpy(data.labels)
    assert metrics == MetricsCalculator(device="cpu").calculate(direct, targets, threshold=threshold)
    assert metrics.total_samples == N_SAMPLES and 0 < metrics.positive_samples < N_SAMPLES
    assert np.array_equal(thr, roc_thresholds())
    ref_fpr, ref_tpr = restated_roc(conf, data.labels, thr)
    assert fpr.dtype == F64 and np.array_equal(fpr, ref_fpr) and np.array_equal(tpr, ref_tpr)
    assert len(np.unique(np.floor(conf * 99))) >= 10 and 0 < fpr[50] < 1 and 0 < tpr[50] < 1   # not a degenerate curve
    names = [f"clip_{i:03d}.wav" if i % 2 == 0 else f"sample_{i // 16}_{i % 16}" for i in range(N_SAMPLES)]
    assert [r.filename for r in results] == names
    assert [r.prediction for r in results] == ["Positive" if c >= F32(threshold) else "Negative" for c in conf]
    assert all(r.latency_ms > 0 for r in results)
    # one batch of 37
    m37, r37 = evaluator.evaluate_dataset(data, threshold=threshold, batch_size=37)
    conf37 = np.array([r.confidence for r in r37], F32)
    bitwise = np.array_equal(conf37, conf)
    print(f"batch_size 37 vs 16: confidences bitwise equal: {bitwise}; worst relative difference "
          f"{(np.abs(conf37.astype(F64) - conf) / conf).max():.3e}")
    assert (np.abs(conf37.astype(F64) - conf.astype(F64)) / ref).max() <= ULP_BOUND
    assert [r.filename for r in r37] == [n if i % 2 == 0 else f"sample_0_{i}" for i, n in enumerate(names)]
    f37, t37, _ = evaluator.get_roc_curve_data(data, batch_size=37)
    r_f37, r_t37 = restated_roc(conf37, data.labels, thr)
    assert np.array_equal(f37, r_f37) and np.array_equal(t37, r_t37)


def test_recording_scanner_equals_host_cut_windows(model, evaluator):
    """A 4.2 s recording: 4 windows of 1.5 s at 50 % overlap, 19200 samples left over."""
    from wakeword_trainer_home_amd.evaluation import RecordingScanner
    rng = np.random.default_rng(21)
    S = int(4.2 * 16000)
    audio = (rng.normal(0, 0.1, S) * np.repeat(rng.choice([0.01, 0.3, 1.0, 3.0], S // 2400), 2400)).astype(F32)
    seen = []
    scanner = RecordingScanner(model, sample_rate=16000, audio_duration=1.5, threshold=0.5, device=DEV, n_mels=N_MELS,
                               callback=lambda c, p: seen.append((c, p)), batch_size=3)
    assert scanner.num_windows(S) == 4 and scanner.window_starts(S) == [0, 12000, 24000, 36000]
    got = scanner.scan(audio)
    windows, peaks = host_windows(audio, 24000)
    ref = evaluator.evaluate_waveforms(windows, threshold=0.5, batch_size=3)
    assert len(got) == 4 and seen == got
    assert [c for c, _ in got] == [r.confidence for r in ref]
    assert [p for _, p in got] == [r.prediction == "Positive" for r in ref]
    assert np.array_equal(scanner.last_peaks.cpu().numpy(), peaks)
    pos = sum(p for _, p in got)
    assert scanner.get_stats() == {"detection_count": pos, "false_alarm_count": 4 - pos, "is_recording": False,
                                   "buffer_size": 19200}
    assert scanner.scan(audio[:23999]) == [] and scanner.get_stats()["buffer_size"] == 23999
    assert [r.filename for r in ref] == [f"sample_{i}" for i in range(4)]
    # int16 waveforms on the device take the same path
    pcm = torch.from_numpy((windows * 32767).astype(np.int16)).to(DEV)
    assert len(evaluator.evaluate_waveforms(pcm, names=list("abcd"), batch_size=4)) == 4


def test_files_go_through_the_same_path(tmp_path, evaluator):
    import wave
    data = _Waves()
    pcm = (data.waves[:3].numpy() * 32767).astype("<i2")
    paths = []
    for i, p in enumerate(pcm):
        paths.append(tmp_path / f"f{i}.wav")
        with wave.open(str(paths[-1]), "wb") as f:
            f.setnchannels(1)
            f.setsampwidth(2)
            f.setframerate(16000)
            f.writeframes(p[:N - 1000 * i].tobytes())                                     # shorter files are zero-padded
    bad = tmp_path / "bad.wav"
    bad.write_bytes(b"junk")
    res = evaluator.evaluate_files([paths[0], bad, paths[1], paths[2]], threshold=0.5, batch_size=2)
    assert [r.filename for r in res] == ["f0.wav", "bad.wav", "f1.wav", "f2.wav"]
    assert res[1].prediction == "Error" and res[1].confidence == 0.0
    waves = np.zeros((3, N), F32)
    for i, p in enumerate(pcm):
        waves[i, :N - 1000 * i] = p[:N - 1000 * i].astype(F32) / F32(32768)
    ref = evaluator.evaluate_waveforms(waves, batch_size=3)
    assert [r.confidence for r in (res[0], res[2], res[3])] == [r.confidence for r in ref]
    one = evaluator.evaluate_file(paths[1], threshold=0.5)
    assert one.filename == "f1.wav" and one.confidence == ref[1].confidence and one.prediction == ref[1].prediction


def test_load_model_for_evaluation_reads_a_trainer_checkpoint(tmp_path):
    from wakeword_trainer_home_amd.config import get_preset
    from wakeword_trainer_home_amd.data import make_synthetic_batch
    from wakeword_trainer_home_amd.evaluation import load_model_for_evaluation
    from wakeword_trainer_home_amd.models import create_model
    from wakeword_trainer_home_amd.training import Trainer
    cfg = get_preset("cnn_small_logmel40")
    cfg.training.epochs, cfg.optimizer.warmup_epochs, cfg.training.batch_size = 1, 0, 8
    cfg.optimizer.mixed_precision = False            # fp32 activation storage, as the loaded model's
    torch.manual_seed(3)
    trained = create_model("cnn_small", dropout=cfg.model.dropout)
    wave, y = make_synthetic_batch(16, N, seed=5)
    y[::3] = 1
    batches = [(wave[i:i + 8], y[i:i + 8], [{"path": "s"}] * 8) for i in (0, 8)]
    t = Trainer(trained, batches, batches[:1], cfg, checkpoint_dir=tmp_path, device=DEV)
    t.train()
    path = tmp_path / "best_model.pt"
    assert path.exists()
    model, info = load_model_for_evaluation(path, device=DEV)
    assert not model.training and info["epoch"] == 0 and info["config"].model.architecture == cfg.model.architecture
    assert set(info) == {"epoch", "val_loss", "val_metrics", "config"} and np.isfinite(info["val_loss"])
    feats = t._features(wave[:8], training=False)
    with torch.no_grad():
        assert torch.equal(model(feats), t.model.eval()(feats))
