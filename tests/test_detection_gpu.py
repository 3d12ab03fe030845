"""GPU: the dense detection scan on the device -- ww_wave_windows_at, ww_feat_windows and ww_detect_accumulate against the
host rules of evaluation/detection.py and tests/detection_cases.py, then DetectionScanner end to end in both feature modes."""
import numpy as np
import pytest
import torch

from oracle import features as OF
from tests.detection_cases import (CUT_CHUNK, CUT_HOPS, CUT_S, F32, bits, cutter_wave, detector_cases, detector_confidences,
                                   detector_events, host_windows_at, table)
from tests.input_stage import assert_logmel_close, logmel_bounds, logmel_t32, oracle_kw, per_clip_err

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N_MELS, N_FFT, HOP_LENGTH, SR = 40, 1024, 160, 16000
DURATION = 0.3
CHUNK = 4800
KW = oracle_kw(n_mels=N_MELS)


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")


@pytest.fixture
def grid_cap():
    """Set the context's grid cap for a test; always back to 0 (no cap) afterwards."""
    from wakeword_trainer_home_amd import _native as nat
    yield lambda n: nat.set_grid_cap(DEV, n)
    nat.set_grid_cap(DEV, 0)


# ------------------------------------------------------------------------------------------------------ the cutter
@pytest.mark.parametrize("cap", [0, 3])
@pytest.mark.parametrize("hop", CUT_HOPS)
def test_wave_windows_at_equal_numpy_bit_for_bit(hop, cap, grid_cap):
    """S = 1000, chunk = 96: the full slab and slabs with w0 > 0 and odd n, both normalize values, a zero window and a NaN
    window; with the grid capped at 3 workgroups every slab of more than 3 windows takes several trips."""
    from wakeword_trainer_home_amd import _native as nat
    from wakeword_trainer_home_amd.evaluation import num_windows_hop
    wave = cutter_wave()
    W = num_windows_hop(CUT_S, CUT_CHUNK, hop)
    assert W == nat.wave_num_windows_hop(CUT_S, CUT_CHUNK, hop) == (CUT_S - CUT_CHUNK) // hop + 1
    dev = torch.from_numpy(wave).to(DEV)
    grid_cap(cap)
    full = {}
    for w0, n in [(0, W), (3, 5), (W - 7, 7), (1, 0)]:
        for normalize in (True, False):
            out, peaks = nat.wave_windows_at(dev, CUT_CHUNK, hop, w0, n, normalize=normalize)
            ref_out, ref_peaks = host_windows_at(wave, CUT_CHUNK, hop, w0, n, normalize)
            assert out.shape == (n, CUT_CHUNK) and peaks.shape == (n,)
            assert np.array_equal(bits(out.cpu().numpy()), bits(ref_out)), (w0, n, normalize)
            assert np.array_equal(peaks.cpu().numpy(), ref_peaks, equal_nan=True), (w0, n, normalize)
            if n == W:
                full[normalize] = (ref_out, ref_peaks)
    ref_out, ref_peaks = full[True]
    zero, nan = np.flatnonzero(ref_peaks == 0), np.flatnonzero(np.isnan(ref_peaks))
    assert zero.size and nan.size and not ref_out[zero].any()                            # a zero window stays zero
    assert np.array_equal(bits(ref_out[nan]), bits(full[False][0][nan]))                 # a NaN window is copied unscaled
    ok = ~np.isnan(ref_peaks) & (ref_peaks > 0)
    assert (np.abs(ref_out[ok]).max(axis=1) == 1.0).all() and not np.array_equal(ref_out[ok], full[False][0][ok])
    if hop == CUT_CHUNK // 2:                                                            # the reference's own hop
        out, peaks = nat.wave_windows_at(dev, CUT_CHUNK, hop, 0, W)
        old_out, old_peaks = nat.wave_windows(dev, CUT_CHUNK)
        assert torch.equal(out.view(torch.int32), old_out.view(torch.int32))
        assert torch.equal(peaks.view(torch.int32), old_peaks.view(torch.int32))
    for w0, n in [(-1, 2), (W - 1, 2), (W, 1)]:
        with pytest.raises(ValueError):
            nat.wave_windows_at(dev, CUT_CHUNK, hop, w0, n)


@pytest.mark.parametrize("over", [0, 1])
def test_wave_windows_at_on_either_side_of_the_split_threshold(over):
    """chunk = WW_WAVE_SPLIT_CHUNK is the longest window one workgroup cuts, one sample more takes the segmented form (five
    segments, the last one of a single sample): four windows at hop 100, the last holding a NaN; an all-zero recording; and
    the whole recording as one window, which is how stream mode divides a recording by its peak."""
    from wakeword_trainer_home_amd import _native as nat
    chunk = nat.WAVE_SPLIT_CHUNK + over
    S = chunk + 300
    rng = np.random.default_rng(chunk)
    wave = (rng.normal(0, 0.2, S) * rng.choice([1e-3, 0.05, 1.0, 30.0], S)).astype(F32)
    wave[33000] = np.nan
    for w, shape in ((wave, (chunk, 100, 0, 4)), (wave, (chunk, 100, 1, 3)), (np.zeros(S, F32), (chunk, 100, 2, 1)),
                     (wave[:32900], (32900, 32900, 0, 1)), (wave, (S, S, 0, 1))):
        dev = torch.from_numpy(w).to(DEV)
        for normalize in (True, False):
            out, peaks = nat.wave_windows_at(dev, *shape, normalize=normalize)
            ref_out, ref_peaks = host_windows_at(w, *shape, normalize)
            assert np.array_equal(bits(out.cpu().numpy()), bits(ref_out)), (shape, normalize)
            assert np.array_equal(bits(peaks.cpu().numpy()), bits(ref_peaks)), (shape, normalize)
    ref_peaks = host_windows_at(wave, chunk, 100, 0, 4, True)[1]
    assert np.isnan(ref_peaks).tolist() == [False, False, False, True]


@pytest.mark.parametrize("cap", [0, 2])
@pytest.mark.parametrize("F", [1, 40])
def test_feat_windows_equal_numpy_slicing_bit_for_bit(F, cap, grid_cap):
    """Ttot = 37, Tw in {1, 7, 16}, step in {1, 3}, from window 0 and from window 2; the map holds arbitrary bit patterns
    (NaN payloads, -0.0, subnormals), so only a bit copy passes."""
    from wakeword_trainer_home_amd import _native as nat
    Ttot = 37
    rng = np.random.default_rng(F)
    feat = rng.integers(0, 2 ** 32, (F, Ttot), dtype=np.uint64).astype(np.uint32)
    dev = torch.from_numpy(feat.view(F32)).to(DEV)
    grid_cap(cap)
    for Tw in (1, 7, 16):
        for step in (1, 3):
            Wmax = (Ttot - Tw) // step + 1
            for w0, n in [(0, Wmax), (2, Wmax - 2), (1, 0)]:
                out = nat.feat_windows(dev, Tw, step, w0, n)
                assert out.shape == (n, 1, F, Tw)
                ref = np.stack([feat[:, (w0 + i) * step:(w0 + i) * step + Tw] for i in range(n)]).reshape(n, 1, F, Tw) \
                    if n else np.zeros((0, 1, F, Tw), np.uint32)
                assert np.array_equal(out.cpu().numpy().view(np.uint32), ref), (Tw, step, w0, n)
            with pytest.raises(ValueError):
                nat.feat_windows(dev, Tw, step, 1, Wmax)                                  # one window past the map


# ------------------------------------------------------------------------------------------------------ the detector
def test_detect_accumulate_equals_the_restatement():
    """W in {0, 1, 2, 300, tile - 1, tile, tile + 1} x a Latin square over K in {1, 100, 1024}, M in {1, 3, 64},
    R in {1, 4, W + 1}, E in {0, 1, 5}: smoothed bitwise, counts exactly; every case is launched twice into the same
    counters; max_triggers alternates between 3 (fewer than most trigger counts) and W + 1."""
    from wakeword_trainer_home_amd import _native as nat
    from wakeword_trainer_home_amd.evaluation import detect_counts, smooth, trigger_windows
    rng = np.random.default_rng(2024)
    z = lambda dt, m, fill=0: torch.full((m,), fill, dtype=dt, device=DEV)
    truncated = 0
    for idx, (W, K, M, R, E) in enumerate(detector_cases(nat.DETECT_TILE)):
        thr = table(K)
        decision = 0.25 if K == 1 else float(thr[K // 3])
        conf, ev = detector_confidences(W, thr, rng), detector_events(W, E)
        T = 3 if idx % 2 else W + 1
        d = dict(conf=torch.from_numpy(conf).to(DEV), thr=torch.from_numpy(thr).to(DEV),
                 ev=torch.from_numpy(ev).to(DEV) if ev.shape[0] else None, smoothed=z(torch.float32, W, -7.0),
                 counts=z(torch.int64, 4 * K), dcounts=z(torch.int64, 4), trig=z(torch.int32, T, -5), n=z(torch.int32, 1, -9))
        for _ in range(2):
            nat.detect_accumulate(d["conf"], M, R, d["thr"], decision, d["ev"], d["smoothed"], d["counts"], d["dcounts"],
                                  d["trig"], d["n"])
        got = {k: v.cpu().numpy() for k, v in d.items() if v is not None}
        tag = (W, K, M, R, E, T)
        if W == 0:
            assert not got["counts"].any() and not got["dcounts"].any() and got["n"][0] == -9 and (got["trig"] == -5).all()
            continue
        s = smooth(conf, M)
        assert np.array_equal(bits(got["smoothed"]), bits(s)), tag
        exp = detect_counts(conf, M, R, thr, ev)
        assert np.array_equal(got["counts"].reshape(K, 4), 2 * exp), tag
        assert (exp[:, 0] == exp[:, 1:].sum(axis=1)).all()
        tw = trigger_windows(s, decision, R)
        assert np.array_equal(got["dcounts"], 2 * detect_counts(conf, M, R, [decision], ev)[0]), tag
        assert got["n"][0] == tw.size and got["dcounts"][0] == 2 * tw.size, tag
        kept = min(T, tw.size)
        assert np.array_equal(got["trig"][:kept], tw[:kept]) and (got["trig"][kept:] == -5).all(), tag
        truncated += tw.size > T
    assert truncated >= 5                              # the list was shorter than the trigger count, and said so, often enough


def test_detect_accumulate_without_a_smoothed_buffer_and_with_bad_arguments():
    from wakeword_trainer_home_amd import _native as nat
    from wakeword_trainer_home_amd.evaluation import detect_counts
    rng = np.random.default_rng(5)
    thr = table(100)
    conf, ev = detector_confidences(300, thr, rng), detector_events(300, 5)
    z = lambda dt, m: torch.zeros(m, dtype=dt, device=DEV)
    args = dict(conf=torch.from_numpy(conf).to(DEV), thr=torch.from_numpy(thr).to(DEV), ev=torch.from_numpy(ev).to(DEV))
    counts, dcounts, trig, n = z(torch.int64, 400), z(torch.int64, 4), z(torch.int32, 0), z(torch.int32, 1)
    nat.detect_accumulate(args["conf"], 3, 4, args["thr"], 0.5, args["ev"], None, counts, dcounts, trig, n)
    assert np.array_equal(counts.cpu().numpy().reshape(100, 4), detect_counts(conf, 3, 4, thr, ev))
    assert n.item() == dcounts[0].item() > 0
    for M, R, decision in [(0, 1, 0.5), (65, 1, 0.5), (1, 0, 0.5), (1, 1, float("nan"))]:
        with pytest.raises(ValueError):
            nat.detect_accumulate(args["conf"], M, R, args["thr"], decision, args["ev"], None, counts, dcounts, trig, n)


# ------------------------------------------------------------------------------------------------------ the scanner
def _recording(seconds, seed):
    rng = np.random.default_rng(seed)
    S = int(seconds * SR)
    return (rng.normal(0, 0.1, S) * np.repeat(rng.choice([0.01, 0.3, 1.0, 3.0], S // 800 + 1), 800)[:S]).astype(F32)


@pytest.fixture(scope="module")
def audio():
    return _recording(2.0, 21)


@pytest.fixture(scope="module")
def model(audio):
    """A seeded cnn_small in eval mode.  Untrained it answers every window alike, so its BatchNorm layers get running
    statistics from the recording's own windows and the classifier is stretched and centred: the confidences then spread
    over (0, 1) and the trigger machines have something to decide."""
    from wakeword_trainer_home_amd import _native as nat
    from wakeword_trainer_home_amd.models import create_model
    torch.manual_seed(4)
    m = create_model("cnn_small", dropout=0.0).to(DEV)
    dev = torch.from_numpy(audio).to(DEV)
    windows, _ = nat.wave_windows_at(dev, CHUNK, 800, 0, (audio.size - CHUNK) // 800 + 1)
    feats = nat.logmel_fwd(windows, nat.make_feat_cfg(n_mels=N_MELS))
    with torch.no_grad():
        m.train()
        for _ in range(30):
            m(feats)
        m.eval()
        m.classifier.weight.mul_(200.0)
        z = m(feats)[::3]                              # the half-overlapping windows: as many of them above 0.5 as below
        m.classifier.bias[1] -= (z[:, 1] - z[:, 0]).median()
    return m


def _scanner(model, **kw):
    from wakeword_trainer_home_amd.evaluation import DetectionScanner
    return DetectionScanner(model, sample_rate=SR, audio_duration=DURATION, device=DEV, n_mels=N_MELS, n_fft=N_FFT,
                            hop_length=HOP_LENGTH, **kw)


def test_scanner_at_half_overlap_is_the_recording_scanner_bit_for_bit(model, audio):
    from wakeword_trainer_home_amd.evaluation import RecordingScanner
    seen = []
    scanner = _scanner(model, hop_seconds=0.15, smooth_windows=1, refractory_seconds=0.15, threshold=0.5,
                       callback=lambda t, c: seen.append((t, c)))
    assert (scanner.hop_samples, scanner.refractory_windows, scanner.chunk_samples) == (2400, 1, CHUNK)
    scan = scanner.scan(audio)
    ref = RecordingScanner(model, sample_rate=SR, audio_duration=DURATION, threshold=0.5, device=DEV, n_mels=N_MELS).scan(audio)
    assert len(ref) == scan.conf.size == 12
    assert np.array_equal(bits(scan.conf), bits(np.array([c for c, _ in ref], F32)))
    assert np.array_equal(bits(scan.smoothed), bits(scan.conf))
    positive = [w for w, (_, p) in enumerate(ref) if p]
    assert scan.trigger_windows.tolist() == positive and scan.n_triggers == len(positive)
    assert 0 < len(positive) < 12, "the fixture's confidences must fall on both sides of the threshold"
    assert scan.trigger_times.tolist() == [(w * 2400 + CHUNK) / SR for w in positive]
    assert seen == [(t, float(scan.smoothed[w])) for w, t in zip(positive, scan.trigger_times)]


def test_scanner_result_equals_the_restatement_on_its_own_confidences(model, audio):
    from wakeword_trainer_home_amd.evaluation import detect_counts, event_windows, rates, smooth, trigger_windows
    events = [(0.5, 0.7), (1.4, 1.5)]
    scanner = _scanner(model, hop_seconds=0.05, smooth_windows=3, tolerance_seconds=0.1)
    assert (scanner.hop_samples, scanner.refractory_windows) == (800, 6)
    scan = scanner.scan(audio, events)
    W = (audio.size - CHUNK) // 800 + 1
    iv, n_events = event_windows(events, audio.size, SR, CHUNK, 800, 0.1)
    assert n_events == 2 and iv.shape == (2, 2) and scan.conf.shape == (W,)
    s = smooth(scan.conf, 3)
    assert np.array_equal(bits(scan.smoothed), bits(s))
    exp = detect_counts(scan.conf, 3, 6, scanner.thresholds, iv)
    print(f"INFO triggers per threshold: {len(np.unique(exp[:, 0]))} distinct counts, {exp[:, 0].min()} .. {exp[:, 0].max()}; "
          f"false alarms rise somewhere along the table: {bool((np.diff(exp[:, 2]) > 0).any())}")
    assert np.array_equal(scan.counts, exp) and len(np.unique(exp[:, 0])) > 1
    assert scan.trigger_windows.tolist() == trigger_windows(s, 0.5, 6).tolist()
    assert np.array_equal(scan.decision_counts, detect_counts(scan.conf, 3, 6, [0.5], iv)[0])
    res = scanner.result()
    hours = audio.size / SR / 3600.0
    fa, miss = rates(exp, 2, hours)
    assert res.hours == hours and res.n_events == 2 and np.array_equal(res.counts, exp)
    assert np.array_equal(res.fa_per_hour, fa) and np.array_equal(res.miss_rate, miss)
    assert np.array_equal(res.fa_per_hour, exp[:, 2] / hours) and np.array_equal(res.miss_rate, (2 - exp[:, 1]) / 2)
    scanner.scan(audio, events)                                                          # totals add up; rates stay
    twice = scanner.result()
    assert np.array_equal(twice.counts, 2 * exp) and twice.n_events == 4 and twice.hours == 2 * hours
    assert np.array_equal(twice.miss_rate, miss)
    scanner.reset()
    assert not scanner.result().counts.any() and scanner.result().hours == 0.0 and scanner.result().fa_per_hour.tolist() == [0.0] * 100
    empty = scanner.scan(audio[:CHUNK - 1], events)                                      # no window: the events are certain misses
    assert empty.conf.size == 0 and empty.n_events == 2 and scanner.result().miss_rate.tolist() == [1.0] * 100


def _interior():
    t = np.arange(CHUNK // HOP_LENGTH + 1)
    return np.flatnonzero((t * HOP_LENGTH >= N_FFT // 2) & (t * HOP_LENGTH <= CHUNK - N_FFT // 2))


def test_stream_features_equal_window_features_where_no_window_edge_is_seen(model, audio):
    """normalize = "none", hop 50 ms: the features of window w at the frames whose n_fft support lies inside the window, from
    the feature map computed once (stream) and from the window cut and transformed on its own (window).  Both are held to
    the float64 oracle features of the window's samples within the front end's own bound (tests/input_stage.py).
    Measured on an MI355X: window mode 2.09e-6 and stream mode 1.50e-6 from the oracle (bound 3.05e-5); the two device
    results are NOT bit-equal on those frames (they differ by up to 2.4e-6: a frame sits at another place of the kernel's
    frame blocks); on the eight edge frames they differ by up to 13.7, reflection against the recording's real neighbours."""
    hop = 800
    W = (audio.size - CHUNK) // hop + 1
    dev = torch.from_numpy(audio).to(DEV)
    feats = {}
    for mode in ("window", "stream"):
        n, slab = _scanner(model, hop_seconds=0.05, features=mode, normalize="none").slab_features(dev)
        assert n == W
        parts = [slab(0, 7), slab(7, W - 7)]                                             # two slabs, the second from w0 = 7
        feats[mode] = torch.cat(parts).cpu().numpy()
        assert feats[mode].shape == (W, 1, N_MELS, CHUNK // HOP_LENGTH + 1)
    x = host_windows_at(audio, CHUNK, hop, 0, W, False)[0]
    ref = OF.logmel(x, **KW)
    bound = logmel_bounds(logmel_t32(x, ref, **KW))
    t = _interior()
    assert t.tolist() == list(range(4, 27))
    for mode in ("window", "stream"):
        err = per_clip_err(feats[mode][..., t], ref[..., t])
        print(f"MEASURED {mode} features, interior frames: max err {err.max():.3e}, worst err/bound {(err / bound).max():.3f}")
        assert (err < bound).all(), (mode, err.max(), bound.min())
    same = np.array_equal(bits(feats["window"][..., t]), bits(feats["stream"][..., t]))
    diff = np.abs(feats["window"][..., t].astype(np.float64) - feats["stream"][..., t]).max()
    print(f"INFO window and stream features bit-equal on the interior frames: {same} (max abs difference {diff:.3e})")
    edge = np.setdiff1d(np.arange(CHUNK // HOP_LENGTH + 1), t)
    print(f"INFO on the edge frames {edge.tolist()} the modes differ by up to "
          f"{np.abs(feats['window'][..., edge].astype(np.float64) - feats['stream'][..., edge]).max():.3e} (reflection against real neighbours)")


def test_stream_front_end_over_four_seconds_in_one_call(model):
    """N = 64000 in a single B = 1 call -- longer than any clip the front-end tests run: the whole map against the float64
    oracle, and the slabs cut from it against NumPy slicing."""
    audio = _recording(4.0, 33)
    dev = torch.from_numpy(audio).to(DEV)
    scanner = _scanner(model, hop_seconds=0.05, features="stream", normalize="none")
    fmap = scanner.feature_extractor(dev)
    assert fmap.shape == (1, N_MELS, 64000 // HOP_LENGTH + 1)
    assert_logmel_close(fmap.cpu().numpy()[None], OF.logmel(audio[None], **KW), audio[None], tag="log-mel 4 s", **KW)
    W, slab = scanner.slab_features(dev)
    assert W == (64000 - CHUNK) // 800 + 1 == 75
    got, host = slab(0, W).cpu().numpy(), fmap.cpu().numpy()[0]
    ref = np.stack([host[:, 5 * w:5 * w + 31] for w in range(W)])[:, None]
    assert np.array_equal(bits(got), bits(ref))
    # "recording" divides by the recording's peak before the one front-end call
    W, slab = _scanner(model, hop_seconds=0.05, features="stream").slab_features(dev)
    normed = scanner.feature_extractor(torch.from_numpy(audio / np.abs(audio).max()).to(DEV)).cpu().numpy()[0]
    assert np.array_equal(bits(slab(3, 1).cpu().numpy()[0, 0]), bits(normed[:, 15:46]))
    scan = _scanner(model, hop_seconds=0.05, features="stream").scan(audio)
    assert scan.conf.shape == (75,) and np.isfinite(scan.conf).all()


def test_scanner_arguments():
    from wakeword_trainer_home_amd.evaluation import DetectionScanner
    stub = torch.nn.Identity()
    for kw in (dict(features="stream", normalize="window"), dict(features="window", normalize="recording"),
               dict(features="stream", hop_seconds=0.105), dict(features="frames"), dict(hop_seconds=0.0),
               dict(hop_seconds=2.0), dict(smooth_windows=65), dict(thresholds=[0.5, 0.4])):
        with pytest.raises(ValueError):
            DetectionScanner(stub, device=DEV, **kw)


class _FixedLogits(torch.nn.Module):
    """Answers every window with the same logits: confidence softmax([0, ln 3])[1] = 0.75."""

    def forward(self, x):
        return torch.tensor([[0.0, float(np.log(3.0))]], device=x.device).expand(x.shape[0], 2).contiguous()


def test_false_alarms_per_hour_and_miss_rate_on_a_figure_worked_out_by_hand():
    """36 s (0.01 h) of a constant, windows of 0.5 s at hop 0.5 s: 72 windows, window w ends at (w + 1) / 2 s.  Every
    confidence is 0.75 and the refractory period is 2 s = 4 windows, so threshold 0.5 triggers at w = 0, 4, ..., 68: 18
    triggers; threshold 0.9 never triggers.  Event [2.4, 2.6] s owns window 4 (ends at 2.5 s): hit.  Event [10.0, 10.1] s
    owns window 19, where no trigger falls: missed.  At 0.5: 1 hit, 17 false alarms = 1700 per hour, miss rate 1/2; at 0.9:
    0 per hour, miss rate 1."""
    from wakeword_trainer_home_amd.evaluation import DetectionScanner
    seen = []
    scanner = DetectionScanner(_FixedLogits(), sample_rate=SR, audio_duration=0.5, hop_seconds=0.5, thresholds=[0.5, 0.9],
                               threshold=0.5, refractory_seconds=2.0, tolerance_seconds=0.0, device=DEV, n_mels=N_MELS,
                               callback=lambda t, c: seen.append((t, c)))
    audio = np.full(36 * SR, 0.25, F32)
    events = [(10.0, 10.1), (2.4, 2.6)]
    scan = scanner.scan(audio, events)
    assert scan.conf.shape == (72,) and np.abs(scan.conf - 0.75).max() < 1e-6 and scanner.refractory_windows == 4
    assert scan.trigger_windows.tolist() == list(range(0, 72, 4)) and scan.n_triggers == 18
    assert scan.trigger_times.tolist() == [(w + 1) / 2 for w in range(0, 72, 4)]
    assert seen == [((w + 1) / 2, float(scan.smoothed[w])) for w in range(0, 72, 4)]
    assert scan.counts.tolist() == [[18, 1, 17, 0], [0, 0, 0, 0]] and scan.decision_counts.tolist() == [18, 1, 17, 0]
    res = scanner.result()
    assert res.hours == pytest.approx(0.01, rel=1e-12) and res.n_events == 2
    assert res.fa_per_hour.tolist() == pytest.approx([1700.0, 0.0], rel=1e-12) and res.miss_rate.tolist() == [0.5, 1.0]
    assert res.decision_fa_per_hour == pytest.approx(1700.0, rel=1e-12) and res.decision_miss_rate == 0.5
    assert res.operating_point(2000.0) == {"index": 0, "threshold": 0.5, "fa_per_hour": res.fa_per_hour[0], "miss_rate": 0.5}
    assert res.operating_point(100.0)["threshold"] == 0.9 and res.operating_point(100.0)["miss_rate"] == 1.0
    assert res.operating_point(-1.0) is None
    scanner.scan(audio, events)
    again = scanner.result()
    assert again.counts.tolist() == [[36, 2, 34, 0], [0, 0, 0, 0]] and again.n_events == 4
    assert again.fa_per_hour.tolist() == pytest.approx([1700.0, 0.0], rel=1e-12) and again.miss_rate.tolist() == [0.5, 1.0]
