"""Throughput of the public call: Trainer.train_epoch() over a DeviceBatchLoader (bench.py drives the private
_prepare_native / _step_native over four resident batches and stays the headline).  One JSON line per geometry:

  config2        cnn_small, B=512, 1.5 s clips, bf16 -- bench.py's geometry, fed by the loader
  large_dataset  the preset's geometry: B=128, 2.5 s clips, RIR p=0.25, noise p=0.4 at 10-20 dB, lr 2e-3, bf16, with cnn_small in
                 place of the out-of-scope resnet18

Each line carries samples/s over whole epochs (drained: the clock stops after the last step's results are read) and the
loader launches by themselves, queued back to back: ms per launch (kernel + in-stream gap) and GB/s over the bytes it must move
(B x n_out x 2 read + written).
--host feeds the same epochs from pinned host int16 batches through a torch DataLoader over ShardedEpochSampler instead: the
H2D-inclusive figure.  Multi-GPU figures are not measured here."""
import argparse
import contextlib
import gc
import json
import sys
import tempfile
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import torch
from wakeword_trainer_home_amd.config import get_preset
from wakeword_trainer_home_amd.data import AudioAugmentation, DeviceBatchLoader, DeviceClipBank, ShardedEpochSampler
from wakeword_trainer_home_amd.models import create_model
from wakeword_trainer_home_amd.training import Trainer

DEV = "cuda:0"


def geometry(name):
    if name == "config2":
        cfg = get_preset("cnn_small_logmel40")
        cfg.optimizer.mixed_precision = True           # bf16 storage, bench.py's default --dtype
    else:
        cfg = get_preset("large_dataset")
        cfg.model.architecture, cfg.model.pretrained = "cnn_small", False
    return cfg


class HostBatches(torch.utils.data.Dataset):
    """Pinned host bank; one item = one batch, gathered into a ring of pinned buffers (batch_size=None DataLoader)."""

    def __init__(self, bank, n_out):
        self.wave = bank.wave[:, :n_out].cpu().pin_memory()
        self.label = bank.labels.cpu().long()
        self.bufs, self.i = {}, 0

    def __len__(self):
        return self.wave.shape[0]

    def __getitem__(self, idx):
        idx = torch.as_tensor(idx)
        key = (self.i % 4, len(idx))
        self.i += 1
        if key not in self.bufs:
            self.bufs[key] = torch.empty((len(idx), self.wave.shape[1]), dtype=torch.int16).pin_memory()
        torch.index_select(self.wave, 0, idx, out=self.bufs[key])
        return self.bufs[key], self.label[idx], {}


def run(name, args):
    cfg = geometry(name)
    B, n_out = cfg.training.batch_size, int(cfg.data.sample_rate * cfg.data.audio_duration)
    cfg.loss.sampler_strategy = args.strategy
    n_clips = B * args.batches
    bank = DeviceClipBank.synthetic(n_clips, n_out, seed=1234, device=DEV)
    if args.strategy == "weighted":
        bank.hard_negative = (torch.arange(n_clips, device=DEV) % 16 == 1) & (bank.labels == 0)
    loader = DeviceBatchLoader.from_config(bank, cfg, drop_last=True)
    if args.host:
        sampler = ShardedEpochSampler(n_clips, cfg.augmentation.seed, 0, 1, args.strategy,
                                      None if args.strategy == "none" else bank.weights(args.strategy, cfg.loss.hard_negative_weight))
        feed = torch.utils.data.DataLoader(HostBatches(bank, n_out), batch_size=None,
                                           sampler=torch.utils.data.BatchSampler(sampler, B, drop_last=True))
        owner = sampler
    else:
        feed = owner = loader
    torch.manual_seed(1234)
    model = create_model("cnn_small", num_classes=2, pretrained=False, dropout=cfg.model.dropout)
    with contextlib.redirect_stdout(sys.stderr):
        trainer = Trainer(model, feed, [], cfg, checkpoint_dir=Path(tempfile.mkdtemp(prefix="wwepoch_")), device=DEV)
    trainer.show_progress = False
    if name == "large_dataset":
        g = torch.Generator(device=DEV).manual_seed(77)
        taps = 4000                                     # 0.25 s at 16 kHz
        rirs = torch.randn(64, taps, device=DEV, generator=g) * torch.exp(-torch.arange(taps, device=DEV) / (taps / 6.0))
        noises = 0.1 * torch.randn(64, 10 * 16000, device=DEV, generator=g)
        a = cfg.augmentation
        trainer.audio_augmentation = AudioAugmentation(
            sample_rate=16000, device=DEV, background_noise_prob=a.background_noise_prob,
            noise_snr_range=(a.noise_snr_min, a.noise_snr_max), rir_prob=a.rir_prob, rirs=rirs, noises=noises, seed=a.seed)

    def epoch(e):
        owner.set_epoch(e)                              # what Trainer.train() does ahead of train_epoch()
        trainer.train_epoch(e)

    gc.collect()
    gc.disable()
    for e in range(args.warmup_epochs):
        epoch(e)
    torch.cuda.synchronize()
    times = []
    for e in range(args.warmup_epochs, args.warmup_epochs + args.epochs):
        t0 = time.perf_counter()
        epoch(e)
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    gc.enable()
    per_epoch = len(feed) * B
    best = min(times)
    out = {"metric": "train_epoch_samples_per_s", "geometry": name, "feed": "host_dataloader" if args.host else "device_loader",
           "value": round(per_epoch / best, 1), "unit": "samples/s", "batch": B, "n_out": n_out, "batches_per_epoch": len(feed),
           "epochs_timed": args.epochs, "epoch_seconds": [round(t, 4) for t in times],
           "ms_per_step": round(1e3 * best / len(feed), 4), "sampler_strategy": args.strategy,
           "act_dtype": "bf16", "gpus": 1, "multi_gpu": "unmeasured"}
    # the loader launches alone.  Python issues one every ~18 us, which is about what the kernel takes, so the launches are queued
    # behind a few milliseconds of copying and the device runs them back to back: kernel + in-stream gap, no host in between
    it, n = iter(loader), min(len(loader), 50)
    for _ in range(3):
        next(it)
    blocker = torch.empty_like(bank.wave)
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(4):
        blocker.copy_(bank.wave)
    a.record()
    for _ in range(n - 3):
        next(it)
    b.record()
    torch.cuda.synchronize()
    ms = a.elapsed_time(b) / (n - 3)
    out["loader_launch_ms"] = round(ms, 5)
    out["loader_gb_per_s"] = round(2 * 2 * B * n_out / (ms * 1e-3) / 1e9, 1)
    print(json.dumps(out), flush=True)
    del trainer, bank, loader, feed
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--geometry", choices=("config2", "large_dataset", "both"), default="both")
    ap.add_argument("--batches", type=int, default=64, help="batches per epoch (the bank holds batches x B clips)")
    ap.add_argument("--epochs", type=int, default=3)
    ap.add_argument("--warmup-epochs", type=int, default=1)
    ap.add_argument("--strategy", choices=("none", "balanced", "weighted"), default="none")
    ap.add_argument("--host", action="store_true", help="feed from pinned host batches through a torch DataLoader")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_epoch.py needs an MI355X: the HIP hot path has no CPU fallback")
    for name in (("config2", "large_dataset") if args.geometry == "both" else (args.geometry,)):
        run(name, args)


if __name__ == "__main__":
    main()
