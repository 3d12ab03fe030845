"""Throughput of the dense detection scan: a seeded synthetic recording (default 10 minutes) scanned at hop 100 ms by a seeded
cnn_small in both feature modes of DetectionScanner -- "window" (each window cut, peak-normalised and transformed on its own)
and "stream" (the front end once over the recording, windows cut from the feature map).

Two measurements per mode, each after a warm-up scan:
  * whole scans, wall time with the device idle at both ends (median and best of --reps): windows/s and seconds of audio per
    second.  This includes the read-back and the host's result objects.
  * one instrumented pass with a device-event pair around every stage of every slab: cutter (ww_wave_windows_at /
    ww_feat_windows), front end (ww_logmel_fwd), model, score (ScoreRun.add) and the detector launch (ww_detect_accumulate).
    In stream mode "peak" is the division of the whole recording by its peak (ww_wave_windows_at with one window of S samples).
    The sums are device time per stage; what is left of the scan's wall time is launch gaps, the read-back and host work.

    python tools/bench_detect.py [--minutes 10] [--batch 512] [--reps 5] [--out profiles/detect_measured.txt]
"""
import argparse
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import numpy as np
import torch

DEV = "cuda:0"


def wall(fn, reps):
    fn()
    times = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    return statistics.median(times), min(times)


class Stages:
    """Device-event pairs per named stage; ``total()`` synchronises once and sums them."""

    def __init__(self):
        self.pairs = []

    def run(self, name, fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn()
        b.record()
        self.pairs.append((name, a, b))
        return out

    def total(self):
        torch.cuda.synchronize()
        out = {}
        for name, a, b in self.pairs:
            out[name] = out.get(name, 0.0) + a.elapsed_time(b) * 1e-3
        return out


def instrumented_pass(scanner, audio):
    """The launches of DetectionScanner.scan, stage by stage (no events of a recording, no read-back)."""
    from wakeword_trainer_home_amd import _native as nat
    from wakeword_trainer_home_amd.evaluation import ScoreRun
    st = Stages()
    S = audio.shape[0]
    W = scanner.num_windows(S)
    fe, B = scanner.feature_extractor, scanner.batch_size
    run = ScoreRun(W, [scanner.threshold], scanner.threshold, DEV)
    if scanner.features == "stream":
        x = st.run("peak", lambda: nat.wave_windows_at(audio, S, S, 0, 1, normalize=True)[0][0])     # the recording / its peak
        feat = st.run("front end", lambda: fe(x))[0]
        Tw, step = scanner.chunk_samples // fe.hop_length + 1, scanner.hop_samples // fe.hop_length
    with torch.no_grad():
        for w0 in range(0, W, B):
            n = min(B, W - w0)
            if scanner.features == "stream":
                feats = st.run("cutter", lambda: nat.feat_windows(feat, Tw, step, w0, n))
            else:
                windows = st.run("cutter", lambda: nat.wave_windows_at(audio, scanner.chunk_samples, scanner.hop_samples, w0, n)[0])
                feats = st.run("front end", lambda: fe(windows))
            logits = st.run("model", lambda: scanner.model(feats))
            st.run("score", lambda: run.add(logits))
    K = scanner.thresholds.size
    z = lambda dt, m: torch.zeros(m, dtype=dt, device=DEV)
    smoothed, counts, dcounts, trig, ntrig = (z(torch.float32, W), z(torch.int64, 4 * K), z(torch.int64, 4),
                                              z(torch.int32, scanner.max_triggers), z(torch.int32, 1))
    thr = torch.from_numpy(scanner.thresholds).to(DEV)
    st.run("detector", lambda: nat.detect_accumulate(run.conf, scanner.smooth_windows, scanner.refractory_windows, thr,
                                                     scanner.threshold, None, smoothed, counts, dcounts, trig, ntrig))
    return st.total()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--minutes", type=float, default=10.0)
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--smooth", type=int, default=3)
    ap.add_argument("--out", type=Path, default=ROOT / "profiles" / "detect_measured.txt")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_detect.py measures on an MI355X; there is no CPU path"
    from wakeword_trainer_home_amd.config import get_preset
    from wakeword_trainer_home_amd.evaluation import DetectionScanner
    from wakeword_trainer_home_amd.models import create_model
    cfg = get_preset("cnn_small_logmel40")
    sr, dur = cfg.data.sample_rate, cfg.data.audio_duration
    S = int(args.minutes * 60 * sr)
    rng = np.random.default_rng(0)
    # noise whose level changes every 100 ms, so that window peaks differ; the model is untrained: its decisions mean nothing
    audio = (rng.normal(0, 0.1, S) * np.repeat(rng.choice([0.01, 0.3, 1.0, 3.0], S // 1600 + 1), 1600)[:S]).astype(np.float32)
    audio = torch.from_numpy(audio).to(DEV)
    torch.manual_seed(0)
    model = create_model("cnn_small", dropout=0.0)
    lines = [f"tools/bench_detect.py on {torch.cuda.get_device_name(0)}: {args.minutes:g} min of seeded noise at {sr} Hz "
             f"({S} samples), windows of {dur} s at hop 100 ms, seeded cnn_small (fp32 storage, eval), n_mels {cfg.data.n_mels}, "
             f"n_fft {cfg.data.n_fft}, hop_length {cfg.data.hop_length}, slabs of {args.batch} windows, {args.smooth}-window "
             f"smoothing, 100 thresholds", ""]
    walls = {}
    for mode in ("window", "stream"):
        scanner = DetectionScanner(model, sample_rate=sr, audio_duration=dur, hop_seconds=0.1, smooth_windows=args.smooth,
                                   features=mode, device=DEV, n_mels=cfg.data.n_mels, n_fft=cfg.data.n_fft,
                                   hop_length=cfg.data.hop_length, batch_size=args.batch)
        W = scanner.num_windows(S)
        med, best = wall(lambda: scanner.scan(audio), args.reps)
        walls[mode] = med
        instrumented_pass(scanner, audio)
        stages = instrumented_pass(scanner, audio)
        dev_total = sum(stages.values())
        lines.append(f"features = {mode!r}: {W} windows in {-(-W // args.batch)} slabs")
        lines.append(f"  whole scan, wall, median of {args.reps}: {med * 1e3:8.2f} ms (best {best * 1e3:.2f})   "
                     f"{W / med:10.0f} windows/s   {S / sr / med:8.1f} s of audio per second")
        lines.append(f"  device time by stage (event pairs, one pass): {dev_total * 1e3:.2f} ms = {dev_total / med:.2f} of the wall time")
        for name in ("peak", "cutter", "front end", "model", "score", "detector"):
            if name in stages:
                lines.append(f"    {name:10s} {stages[name] * 1e3:8.3f} ms   {stages[name] / dev_total:6.1%}")
        lines.append("")
    lines.append(f"stream / window, whole-scan wall time: {walls['stream'] / walls['window']:.3f}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    args.out.parent.mkdir(parents=True, exist_ok=True)
    args.out.write_text(text)


if __name__ == "__main__":
    main()
