"""Time of the time-stretch / pitch-shift call (ww_audio_tsm) alone at B = 512, N = 24000 over the default preset ranges
(rates 0.8 ... 1.2, -2 ... +2 semitones), with both probabilities at 1.0 and at 0.5, and beside it the existing RIR + noise call
(ww_audio_augment, 4000-tap RIRs through the overlap-save form, as the Trainer runs it) on the same batch in the same process.
HIP events around the launches of one call, device idle before each; the median of --reps passes after --warmup.  Prints
one JSON line.

    python tools/bench_tsm.py [--batch 512] [--samples 24000] [--reps 20] [--warmup 3]
"""
import argparse
import json
import statistics
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import torch

DEV = "cuda:0"


def event_ms(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    times = []
    for _ in range(reps):
        torch.cuda.synchronize()
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return statistics.median(times), min(times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--samples", type=int, default=24000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    from wakeword_trainer_home_amd import _native as nat
    from wakeword_trainer_home_amd.config import AugmentationConfig
    a = AugmentationConfig()
    B, N = args.batch, args.samples
    g = torch.Generator(device=DEV).manual_seed(3)
    x = 0.2 * torch.randn(B, N, device=DEV, generator=g)
    rirs = torch.randn(16, 4000, device=DEV, generator=g) * torch.exp(-torch.arange(4000, device=DEV) / 700.0)
    noises = 0.1 * torch.randn(8, 160000, device=DEV, generator=g)
    spectra = nat.audio_rir_spectra(rirs)
    out = torch.empty_like(x)
    scratch = torch.empty(nat.load().ww_audio_tsm_scratch_bytes(B, N, a.pitch_shift_max) // 4, device=DEV)
    res = {"bench": "audio_tsm", "gpu": torch.cuda.get_device_name(0), "batch": B, "samples_per_wave": N, "reps": args.reps,
           "rate_range": [a.time_stretch_min, a.time_stretch_max], "semis_range": [a.pitch_shift_min, a.pitch_shift_max]}
    for p in (1.0, 0.5):
        def tsm():
            nat.audio_tsm(x, p, a.time_stretch_min, a.time_stretch_max, p, a.pitch_shift_min, a.pitch_shift_max, seed=1, step=9,
                          out=out, scratch=scratch)
        med, best = event_ms(tsm, args.reps, args.warmup)
        res[f"tsm_prob_{p}_ms"], res[f"tsm_prob_{p}_best_ms"] = round(med, 4), round(best, 4)
    # each stage of the selected-clip path alone: a pitch shift of 0 semitones with certain stretch is WSOLA + a resampler that
    # copies z; certain pitch shift without stretch still runs WSOLA (at rho = 1 / f), so the split is read from the 0-semitone run
    def wsola_mostly():
        nat.audio_tsm(x, 1.0, a.time_stretch_min, a.time_stretch_max, 0.0, 0, 0, seed=1, step=9, out=out, scratch=scratch)
    med, _ = event_ms(wsola_mostly, args.reps, args.warmup)
    res["tsm_stretch_only_ms"] = round(med, 4)

    def rir_noise():
        nat.audio_augment(x, rirs, noises, a.rir_prob, a.background_noise_prob, a.noise_snr_min, a.noise_snr_max, seed=1, step=9,
                          rir_spectra=spectra)
    med, best = event_ms(rir_noise, args.reps, args.warmup)
    res["rir_noise_ms"], res["rir_noise_best_ms"] = round(med, 4), round(best, 4)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
