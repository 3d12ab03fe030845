"""Throughput of the evaluation path: samples/s of ModelEvaluator.evaluate_waveforms for cnn_small at batch 512 (waveform ->
log-mel -> model -> ww_eval_accumulate, one read-back per pass, a list of n EvaluationResult objects), the same pass without
building those objects, and beside them Trainer.validate_epoch on the same
device-resident waveforms and batch size (one ww_step_stats read per batch).  Wall time of whole passes, device idle at both
ends; the median of --reps passes after one warm-up pass.  Prints one JSON line.

    python tools/bench_eval.py [--samples 4096] [--batch 512] [--reps 5]
"""
import argparse
import json
import statistics
import sys
import tempfile
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import torch

DEV = "cuda:0"


def passes_per_second(fn, reps):
    fn()
    times = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    return statistics.median(times), min(times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=4096)
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    from wakeword_trainer_home_amd.config import get_preset
    from wakeword_trainer_home_amd.evaluation import ModelEvaluator, ScoreRun
    from wakeword_trainer_home_amd.models import create_model
    from wakeword_trainer_home_amd.training import Trainer
    cfg = get_preset("cnn_small_logmel40")
    cfg.optimizer.mixed_precision = False                      # fp32 activation storage on both sides
    n, B, N = args.samples, args.batch, int(cfg.data.sample_rate * cfg.data.audio_duration)
    torch.manual_seed(0)
    waves = (torch.randn(n, N, device=DEV) * 0.1).clamp_(-1, 1)
    targets = (torch.rand(n, device=DEV) < 0.3).long()
    model = create_model("cnn_small", dropout=cfg.model.dropout)
    ev = ModelEvaluator(model, sample_rate=cfg.data.sample_rate, audio_duration=cfg.data.audio_duration, device=DEV,
                        n_mels=cfg.data.n_mels, n_fft=cfg.data.n_fft, hop_length=cfg.data.hop_length)
    t_eval, t_eval_min = passes_per_second(lambda: ev.evaluate_waveforms(waves, batch_size=B), args.reps)

    def score_pass():                                          # the same pass without building n EvaluationResult objects
        run = ScoreRun(n, [0.5], 0.5, DEV)
        for i in range(0, n, B):
            run.add(ev._logits(ev._features(waves[i:i + B])))
        return run.finish()
    t_score, t_score_min = passes_per_second(score_pass, args.reps)
    batches = [(waves[i:i + B], targets[i:i + B]) for i in range(0, n, B)]
    with tempfile.TemporaryDirectory() as ckpt_dir:
        trainer = Trainer(model, batches[:1], batches, cfg, checkpoint_dir=Path(ckpt_dir), device=DEV)
        t_val, t_val_min = passes_per_second(lambda: trainer.validate_epoch(0), args.reps)
    print(json.dumps({"bench": "evaluation", "model": "cnn_small", "gpu": torch.cuda.get_device_name(0), "samples": n,
                      "batch": B, "samples_per_wave": N, "reps": args.reps,
                      "evaluate_waveforms_samples_per_s": round(n / t_eval, 1),
                      "evaluate_waveforms_best_samples_per_s": round(n / t_eval_min, 1),
                      "score_pass_without_result_objects_samples_per_s": round(n / t_score, 1),
                      "score_pass_without_result_objects_best_samples_per_s": round(n / t_score_min, 1),
                      "validate_epoch_samples_per_s": round(n / t_val, 1),
                      "validate_epoch_best_samples_per_s": round(n / t_val_min, 1)}))


if __name__ == "__main__":
    main()
