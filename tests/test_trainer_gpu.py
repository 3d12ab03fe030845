"""GPU: the drop-in Trainer / module API running on the HIP hot path, against the trace captured from the
real reference Trainer (G2) and against the CPU oracle."""
import numpy as np
import pytest
import torch

from tests.golden_util import load_trace, make_inputs

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")


def _cfg_from_meta(meta):
    from wakeword_trainer_home_amd.config import WakewordConfig
    cfg = WakewordConfig()
    for sec in ("loss", "optimizer", "training"):
        for k, v in meta["cfg"][sec].items():
            if hasattr(getattr(cfg, sec), k):
                setattr(getattr(cfg, sec), k, v)
    cfg.model.architecture, cfg.model.pretrained = "cnn_small", False
    return cfg


class _Rec:
    def __init__(self):
        self.loss, self.acc, self.epochs = [], [], []

    def on_batch_end(self, batch_idx, loss, acc):
        self.loss.append(loss)
        self.acc.append(acc)

    def on_epoch_end(self, epoch, train_loss, val_loss, val_metrics):
        self.epochs.append((train_loss, val_loss, val_metrics))


@pytest.mark.parametrize("tag", ["default_b16", "focal_b16", "sgd_b8", "default_b128"])
def test_native_trainer_matches_reference_trace(golden_dir, tmp_path, tag):
    """north_star: per-step loss within 1e-3 (fp32) of the reference PyTorch step on identical inputs."""
    from wakeword_trainer_home_amd.models import create_model
    from wakeword_trainer_home_amd.training import Trainer
    meta, tr = load_trace(golden_dir, tag)
    cfg = _cfg_from_meta(meta)
    model = create_model("cnn_small", dropout=0.0)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in tr["init"].items()})
    xtr, ytr = make_inputs(meta["train_seed"], meta["n_train"])
    xva, yva = make_inputs(meta["val_seed"], meta["n_val"])
    DL, TD = torch.utils.data.DataLoader, torch.utils.data.TensorDataset
    t = Trainer(model, DL(TD(xtr, ytr), batch_size=meta["batch"]), DL(TD(xva, yva), batch_size=meta["batch"]), cfg,
                checkpoint_dir=tmp_path, device=DEV)
    assert t.native and t._native_loss
    rec = _Rec()
    t.add_callback(rec)
    res = t.train()
    d = np.abs(np.array(rec.loss) - tr["step_loss"])
    assert len(rec.loss) == len(tr["step_loss"])
    assert d.max() < 1e-3, f"per-step loss delta max {d.max():.2e} ({d})"
    assert np.abs(np.array(rec.acc) - tr["step_acc"]).max() <= 1.0 / meta["batch"] + 1e-9
    for k in ("train_loss", "val_loss"):
        assert np.abs(np.array(res["history"][k]) - np.array(meta["history"][k])).max() < 1e-3, k
    np.testing.assert_allclose(res["history"]["learning_rates"], meta["history"]["learning_rates"], rtol=2e-3)
    assert sorted(p.name for p in tmp_path.iterdir()) == meta["files"]
    ck = torch.load(tmp_path / "best_model.pt", map_location="cpu", weights_only=False)
    # the reference's key set plus the build's one documented extension (the Philox launched-step counter)
    assert sorted(set(ck.keys()) - {"launched_steps"}) == meta["ckpt_keys"] and "launched_steps" in ck
    # the checkpoint loads into the plain-torch formulation (and would into the reference's consumers)
    from oracle.cnn_small import CNNSmallOracle
    CNNSmallOracle(dropout=0.0).load_state_dict(ck["model_state_dict"])
    assert int(ck["model_state_dict"]["stem.bn.num_batches_tracked"]) == len(tr["step_loss"])
    print(f"{tag}: max |loss_HIP - loss_ref| = {d.max():.2e}")


def test_waveform_batches_run_the_fused_front_end(tmp_path):
    """2-D inputs (B,N): log-mel + SpecAugment + cnn_small step on the device == oracle pipeline on the host."""
    from wakeword_trainer_home_amd.config import get_preset
    from wakeword_trainer_home_amd.models import create_model
    from wakeword_trainer_home_amd.training import Trainer
    from wakeword_trainer_home_amd.data import make_synthetic_batch
    from oracle.cnn_small import CNNSmallOracle
    from oracle.train_step import TorchLoss, frontend, train_step
    cfg = get_preset("cnn_small_logmel40")
    cfg.training.epochs, cfg.optimizer.warmup_epochs, cfg.training.batch_size = 1, 0, 8
    torch.manual_seed(3)
    model = create_model("cnn_small", dropout=0.3, dropout_seed=11)
    sd = {k: v.clone() for k, v in model.state_dict().items()}
    wave, y = make_synthetic_batch(24, 24000, seed=5)
    y[::3] = 1
    batches = [(wave[i:i + 8], y[i:i + 8], [{"path": "s"}] * 8) for i in range(0, 24, 8)]
    t = Trainer(model, batches, batches[:1], cfg, checkpoint_dir=tmp_path, device=DEV)
    rec = _Rec()
    t.add_callback(rec)
    t.train_epoch(0)
    oracle = CNNSmallOracle(dropout=0.3, dropout_seed=11)
    oracle.load_state_dict(sd)
    oracle.train()
    opt = torch.optim.AdamW(oracle.parameters(), lr=cfg.training.learning_rate, weight_decay=cfg.optimizer.weight_decay)
    a = cfg.augmentation
    spec = dict(freq_mask_param=a.freq_mask_param, time_mask_param=a.time_mask_param, n_freq_masks=a.n_freq_masks,
                n_time_masks=a.n_time_masks, freq_mask_prob=a.freq_mask_prob, time_mask_prob=a.time_mask_prob)
    for i, (w, yy, _) in enumerate(batches):
        x, _ = frontend(w.numpy(), spec, seed=a.seed, step=i)
        r = train_step(oracle, TorchLoss("cross_entropy", eps=cfg.loss.label_smoothing), opt, x, yy, 1.0)
        assert abs(r["loss"] - rec.loss[i]) < 1e-3, (i, r["loss"], rec.loss[i])
    loss, m = t.validate_epoch(0)
    assert m.total_samples == 8 and np.isfinite(loss)


def test_module_api_autograd_and_accumulation():
    from wakeword_trainer_home_amd.models import create_model, create_loss_function
    from oracle.cnn_small import CNNSmallOracle
    from oracle.train_step import TorchLoss
    torch.manual_seed(0)
    model = create_model("cnn_small", dropout=0.0).to(DEV)
    oracle = CNNSmallOracle(dropout=0.0)
    oracle.load_state_dict({k: v.cpu() for k, v in model.state_dict().items()})
    x, y = make_inputs(11, 6)
    crit = create_loss_function("cross_entropy", label_smoothing=0.1, device=DEV)
    model.train()
    out = model(x.to(DEV))
    assert out.shape == (6, 2) and out.requires_grad
    loss = crit(out, y.to(DEV))
    (2.0 * loss).backward()                       # upstream scale flows through both custom Functions
    oracle.train()
    lo = TorchLoss("cross_entropy", eps=0.1)(oracle(x), y)
    (2.0 * lo).backward()
    assert abs(loss.item() - lo.item()) < 1e-5
    # API-level check on the whole gradient vector (element-level parity with shared ReLU decisions is
    # test_hip_kernels.py::test_cnn_small_fwd_bwd_matches_oracle; at B=6 a single fp32 ReLU flip moves
    # individual BN gradients by ~1e-2)
    gn = torch.cat([p.grad.flatten().cpu() for p in model.parameters()])
    go = torch.cat([q.grad.flatten() for q in oracle.parameters()])
    assert ((gn - go).norm() / go.norm()).item() < 2e-2
    g1 = {n: p.grad.clone() for n, p in model.named_parameters()}
    crit(model(x.to(DEV)), y.to(DEV)).backward()  # second backward without zero_grad accumulates
    for n, p in model.named_parameters():
        assert torch.allclose(p.grad, 1.5 * g1[n], rtol=2e-3, atol=1e-7), n
    oracle(x)                                     # mirror the second training forward (running statistics)
    model.eval()
    with torch.no_grad():
        e_out = model(x.to(DEV))
    oracle.eval()
    assert (e_out.cpu() - oracle(x)).abs().max() < 1e-3
    with pytest.raises(ValueError, match=r"Target values must be in \[0, 1\]"):
        crit(e_out, torch.full((6,), 3, device=DEV))


def test_feature_extractor_and_specaugment_api():
    """call contracts reconstructed from the reference's call sites."""
    from wakeword_trainer_home_amd.data import FeatureExtractor, SpecAugment
    from oracle import features as OF
    fe = FeatureExtractor(sample_rate=16000, feature_type="mel", n_mels=64, n_mfcc=40, n_fft=1024, hop_length=160,
                          device=DEV)
    wav = torch.from_numpy(np.random.default_rng(0).normal(0, 0.1, 24000).astype(np.float32))
    f = fe(wav)                                    # evaluator.py:125 -> (1, n_mels, T); caller unsqueezes
    assert f.shape == (1, 64, 151) and f.is_cuda
    assert np.abs(f.cpu().numpy() - OF.logmel(wav.numpy()[None], n_mels=64)[0]).max() < 1e-3
    assert FeatureExtractor(feature_type="mfcc", n_mels=40, n_mfcc=13, device=DEV)(wav).shape == (1, 13, 151)
    assert fe(torch.stack([wav, wav])).shape == (2, 1, 64, 151)
    with pytest.raises(ValueError):
        FeatureExtractor(feature_type="chroma")
    sa = SpecAugment(freq_mask_param=15, time_mask_param=35, n_freq_masks=2, n_time_masks=2)
    spec = torch.randn(1, 64, 50, device=DEV)      # test_training_pipeline.py:259-262
    out = sa(spec)
    assert out.shape == spec.shape and (out == 0).any() and not (spec == 0).any()


@pytest.mark.parametrize("deferred", [True, False])
def test_nonfinite_batch_is_skipped_on_the_device(tmp_path, deferred):
    """Reference semantics (trainer.py:177-179, Q5): a batch with a non-finite loss changes no parameter, fires no
    on_batch_end, but still counts in the epoch-loss denominator.  Here the decision reaches the fused optimizer as
    a device flag; with deferred_metrics the callbacks arrive one step late but complete and in order."""
    from wakeword_trainer_home_amd.config import WakewordConfig
    from wakeword_trainer_home_amd.models import create_model
    from wakeword_trainer_home_amd.training import Trainer
    cfg = WakewordConfig()
    cfg.training.epochs, cfg.optimizer.warmup_epochs = 1, 0
    cfg.training.deferred_metrics = deferred
    cfg.model.architecture = "cnn_small"
    torch.manual_seed(1)
    model = create_model("cnn_small", dropout=0.0)
    x, y = make_inputs(21, 32)
    bad = x[8:16].clone()
    bad[3, 0, 5, 7] = float("nan")
    badt = y[16:24].clone()
    badt[2] = 5                                       # invalid target: the reference raises ValueError and skips
    batches = [(x[0:8], y[0:8]), (bad, y[8:16]), (x[16:24], badt), (x[24:32], y[24:32])]
    t = Trainer(model, batches, batches[:1], cfg, checkpoint_dir=tmp_path, device=DEV)
    assert t.deferred_metrics == deferred and t._skip_on_device
    seen = []
    snaps = []

    class CB:
        def on_batch_end(self, idx, loss, acc):
            seen.append(idx)
            assert np.isfinite(loss)
    t.add_callback(CB())
    # step by step, snapshotting parameters after each launched step
    t.model.train()
    t.train_metrics_tracker.reset()
    for i, (xi, yi) in enumerate(batches):
        t._step_native(xi, yi, i)
        torch.cuda.synchronize()
        snaps.append(torch.cat([p.detach().flatten().clone() for p in t.model.parameters()]))
    t._flush_pending()
    assert not torch.equal(snaps[0], snaps[3])
    assert torch.equal(snaps[0], snaps[1]), "NaN batch must not change the parameters"
    assert torch.equal(snaps[1], snaps[2]), "invalid-target batch must not change the parameters"
    assert torch.isfinite(snaps[3]).all()
    # full epoch through the public API: callbacks for the 2 good batches only, denominator = 4
    model2 = create_model("cnn_small", dropout=0.0)
    t2 = Trainer(model2, batches, batches[:1], cfg, checkpoint_dir=tmp_path, device=DEV)
    rec = _Rec()
    t2.add_callback(rec)
    avg, _ = t2.train_epoch(0)
    assert len(rec.loss) == 2 and t2.state.global_step == 2
    assert avg == pytest.approx(sum(rec.loss) / 4)
    # a NaN input reaches the logits as in torch (ReLU propagates NaN): eval forward is NaN, not silently finite
    model2.eval()
    with torch.no_grad():
        assert torch.isnan(model2(bad.to(DEV))).any()


_UNFUSED_RUNS = {}            # (optim, deferred) -> what _unfused_run saw: each arm runs once, the test's cases share it


def _unfused_run(optim, deferred, ckpt_dir):
    """cnn_small's native step under a torch optimizer over four batches of 8 (clean, NaN input, invalid target, clean):
    step by step with the parameters snapshotted after every launched step, then one epoch through train_epoch."""
    if (optim, deferred) in _UNFUSED_RUNS:
        return _UNFUSED_RUNS[optim, deferred]
    from wakeword_trainer_home_amd.config import WakewordConfig
    from wakeword_trainer_home_amd.models import create_model
    from wakeword_trainer_home_amd.training import Trainer
    cfg = WakewordConfig()
    cfg.training.epochs, cfg.optimizer.warmup_epochs = 1, 0
    cfg.training.deferred_metrics = deferred
    cfg.model.architecture = "cnn_small"
    x, y = make_inputs(21, 32)
    bad = x[8:16].clone()
    bad[3, 0, 5, 7] = float("nan")
    badt = y[16:24].clone()
    badt[2] = 5
    batches = [(x[0:8], y[0:8]), (bad, y[8:16]), (x[16:24], badt), (x[24:32], y[24:32])]

    def trainer():
        torch.manual_seed(1)
        model = create_model("cnn_small", dropout=0.0)
        t = Trainer(model, batches, batches[:1], cfg, checkpoint_dir=ckpt_dir, device=DEV)
        if optim == "adam_fused":
            t.optimizer = torch.optim.Adam(model.parameters(), lr=1e-3, fused=True)
        else:
            t.optimizer = torch.optim.SGD(model.parameters(), lr=1e-2, momentum=0.9)
        t._classify_optimizer()
        return t

    def params(t):
        return torch.cat([p.detach().flatten().clone() for p in t.model.parameters()])

    t = trainer()
    r = {"fused": t._fused_optimizer, "skip_on_device": t._skip_on_device, "deferred": t.deferred_metrics}
    t.model.train()
    t.train_metrics_tracker.reset()
    r["snaps"], r["returned"] = [params(t)], []
    for i, (xi, yi) in enumerate(batches):
        r["returned"] += t._step_native(xi, yi, i)
        torch.cuda.synchronize()
        r["snaps"].append(params(t))
    r["returned"] += t._flush_pending()
    t2, fired = trainer(), []

    class CB:
        def on_batch_end(self, idx, loss, acc):
            fired.append((idx, loss, acc))
    t2.add_callback(CB())
    t2.train_epoch(0)                                 # ends with its own _flush_pending()
    r["fired"] = fired
    _UNFUSED_RUNS[optim, deferred] = r
    return r


@pytest.mark.parametrize("deferred", [True, False])
@pytest.mark.parametrize("optim", ["adam_fused", "sgd"])
def test_unfused_native_arms_skip_and_apply(tmp_path, optim, deferred):
    """The native step under a torch optimizer, the two arms no other GPU test runs: one that takes found_inf on the
    device (fused Adam: clip kernel, then optimizer.step() with the flag) and one that cannot (SGD: the host reads the
    stats, then steps or drops the gradients).  The properties of test_nonfinite_batch_is_skipped_on_the_device: a
    skipped batch changes no parameter and reports nothing, and reading the stats one step late changes no update."""
    r = _unfused_run(optim, deferred, tmp_path)
    assert not r["fused"]
    assert r["skip_on_device"] == (optim == "adam_fused")
    assert r["deferred"] == (deferred and optim == "adam_fused")       # the host decides for SGD: nothing to defer
    start, s0, s1, s2, s3 = r["snaps"]
    assert not torch.equal(start, s0), "the first clean batch must be applied"
    assert torch.equal(s0, s1), "NaN batch must not change the parameters"
    assert torch.equal(s1, s2), "invalid-target batch must not change the parameters"
    assert not torch.equal(s2, s3) and not torch.equal(s0, s3), "the last clean batch must be applied"
    assert torch.isfinite(s3).all()
    for what in ("returned", "fired"):               # what the steps handed back / what train_epoch gave on_batch_end
        assert [d[0] for d in r[what]] == [0, 3], (what, r[what])
        assert all(np.isfinite(d[1]) for d in r[what]), (what, r[what])
    if optim == "adam_fused":
        other = _unfused_run(optim, not deferred, tmp_path)
        assert torch.equal(s3, other["snaps"][-1]), "reading the stats one step late must not change the update"


@pytest.mark.parametrize("poison", [False, True], ids=["clean", "with_a_skipped_batch"])
def test_native_resume_continues_like_an_uninterrupted_run(tmp_path, poison):
    """Checkpoint after 2 of 4 epochs (native cnn_small, fused clip+optimizer, dropout on), resume in a fresh Trainer: the
    remaining steps reproduce the uninterrupted run bit for bit -- weights, BatchNorm statistics, optimizer moments and
    step count, scheduler and the dropout stream all continue.  `with_a_skipped_batch`: one batch of every epoch is
    non-finite and skipped; the Philox streams are driven by the LAUNCHED-step counter (saved in the checkpoint), so the
    skipped batches neither make later batches reuse masks nor break the resumed run's match."""
    from wakeword_trainer_home_amd.config import get_preset
    from wakeword_trainer_home_amd.models import create_model
    from wakeword_trainer_home_amd.training import Trainer

    def run(d, stop_after=None, resume=None):
        cfg = get_preset("cnn_small_logmel40")
        cfg.training.epochs, cfg.optimizer.warmup_epochs, cfg.training.batch_size = 4, 0, 8
        cfg.training.checkpoint_frequency = "every_epoch"
        torch.manual_seed(12)
        model = create_model("cnn_small", dropout=0.3, dropout_seed=3)
        x, y = make_inputs(31, 24)
        if poison:
            x = x.clone()
            x[9, 0, 3, 3] = float("inf")                                   # the second batch of every epoch is skipped
        batches = [(x[i:i + 8], y[i:i + 8]) for i in range(0, 24, 8)]
        t = Trainer(model, batches, batches[:1], cfg, checkpoint_dir=d, device=DEV)
        rec = _Rec()
        t.add_callback(rec)
        if stop_after is not None:       # Ctrl-C after the epoch's checkpoint is written (train() catches it)
            class _Stop:
                def on_epoch_end(self, epoch, *a):
                    if epoch + 1 == stop_after:
                        raise KeyboardInterrupt
            t.add_callback(_Stop())
        t.train(resume_from=resume)
        return rec.loss, {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}

    full_loss, full_sd = run(tmp_path / "full")
    run(tmp_path / "a", stop_after=2)
    tail_loss, tail_sd = run(tmp_path / "b", resume=tmp_path / "a" / "checkpoint_epoch_002.pt")
    per_epoch = 2 if poison else 3
    assert len(full_loss) == 4 * per_epoch and len(tail_loss) == 2 * per_epoch
    assert tail_loss == full_loss[2 * per_epoch:]
    bits = lambda t: t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t      # NaN running stats compare bitwise
    for k in full_sd:
        assert torch.equal(bits(full_sd[k]), bits(tail_sd[k])), k


def test_ragged_batches_through_the_native_step(tmp_path):
    """A DataLoader's last batch is short (drop_last=False in the reference): batch sizes 8, 8, 5 and a single-sample batch
    go through the same native step (workspaces are per shape) and track the oracle pipeline step by step."""
    from wakeword_trainer_home_amd.config import get_preset
    from wakeword_trainer_home_amd.models import create_model
    from wakeword_trainer_home_amd.training import Trainer
    from wakeword_trainer_home_amd.data import make_synthetic_batch
    from oracle.cnn_small import CNNSmallOracle
    from oracle.train_step import TorchLoss, frontend, train_step
    cfg = get_preset("cnn_small_logmel40")
    cfg.training.epochs, cfg.optimizer.warmup_epochs, cfg.training.batch_size = 1, 0, 8
    torch.manual_seed(8)
    model = create_model("cnn_small", dropout=0.0)
    sd = {k: v.clone() for k, v in model.state_dict().items()}
    wave, y = make_synthetic_batch(22, 24000, seed=9)
    y[::2] = 1
    cuts = [(0, 8), (8, 16), (16, 21), (21, 22)]
    batches = [(wave[a:b], y[a:b]) for a, b in cuts]
    t = Trainer(model, batches, batches[:1], cfg, checkpoint_dir=tmp_path, device=DEV)
    rec = _Rec()
    t.add_callback(rec)
    loss, acc = t.train_epoch(0)
    assert len(rec.loss) == 4 and np.isfinite(loss) and 0.0 <= acc <= 1.0
    oracle = CNNSmallOracle(dropout=0.0)
    oracle.load_state_dict(sd)
    oracle.train()
    opt = torch.optim.AdamW(oracle.parameters(), lr=cfg.training.learning_rate, weight_decay=cfg.optimizer.weight_decay)
    a = cfg.augmentation
    spec = dict(freq_mask_param=a.freq_mask_param, time_mask_param=a.time_mask_param, n_freq_masks=a.n_freq_masks,
                n_time_masks=a.n_time_masks, freq_mask_prob=a.freq_mask_prob, time_mask_prob=a.time_mask_prob)
    for i, (w, yy) in enumerate(batches):
        x, _ = frontend(w.numpy(), spec, seed=a.seed, step=i)
        r = train_step(oracle, TorchLoss("cross_entropy", eps=cfg.loss.label_smoothing), opt, x, yy, 1.0)
        assert abs(r["loss"] - rec.loss[i]) < 2e-3, (i, r["loss"], rec.loss[i])
    # the epoch's sample-weighted accuracy counts every sample of every batch once
    assert t.train_metrics_tracker.compute().total_samples == 22
