"""Waveform augmentation: oracle self-checks on CPU, HIP parity on the GPU.
The law is the build's own spec (reference source absent -> parity unpinned w.r.t. the reference); what is checked here
is device == oracle: Philox choices bit-exact, waveform within max(m * e32, 16 * 2**-24) absolute per call, the former
flat 1e-4 as ceiling (tests/input_stage.py; tests/test_input_stage_bounds.py shows on the CPU that these bounds
discriminate).  e32 is the error of the fp32 restatement of the law (every array and scalar in float32, on the CPU)
against the float64 oracle on the same inputs; m = 8 for the direct convolution and 32 for the overlap-save form.  For
the direct form e32 is the larger of that restatement and the one whose convolution is one running fp32 sum over the
taps, the device's own order: every dense-RIR direct case rests on the second (1200 taps: 1.3e-6 against numpy's blocked
1.2e-7; 8192 taps: 4.3e-6 against 1.4e-7; the device measured 1.3e-6 and 4.3e-6)."""
import numpy as np
import pytest
import torch

from oracle import audio_augment as oa
from tests import input_stage as S

_banks = S.banks


def test_oracle_choices_ranges_and_rates():
    ch = oa.audio_choices(4096, 24000, 5, 7, 48000, 0.25, 0.5, 5.0, 20.0, seed=3, step=11)
    assert ch["rir"].max() < 5 and ch["noise"].max() < 7
    assert 0 <= ch["offset"].min() and ch["offset"].max() <= 24000
    assert ch["snr_db"].min() >= 5.0 and ch["snr_db"].max() <= 20.0
    assert abs((ch["rir"] >= 0).mean() - 0.25) < 0.03 and abs((ch["noise"] >= 0).mean() - 0.5) < 0.03
    # a different step or sample offset is a different stream; same arguments repeat exactly
    ch2 = oa.audio_choices(4096, 24000, 5, 7, 48000, 0.25, 0.5, 5.0, 20.0, seed=3, step=12)
    assert (ch2["offset"] != ch["offset"]).mean() > 0.9
    ch3 = oa.audio_choices(8, 24000, 5, 7, 48000, 0.25, 0.5, 5.0, 20.0, seed=3, step=11, sample_offset=100)
    assert np.array_equal(ch3["offset"], ch["offset"][100:108])


def test_oracle_signal_law():
    rng = np.random.default_rng(0)
    rirs, noises = _banks(rng)
    x = (0.2 * rng.standard_normal((16, 8000))).astype(np.float32)
    out, ch = oa.audio_augment(x, rirs, noises, 1.0, 1.0, 10.0, 10.0, seed=1)
    assert out.shape == x.shape and np.isfinite(out).all() and np.abs(out).max() <= 1.0
    for b in range(16):       # SNR of the mix is the drawn one (no clipping at this level)
        n = noises[ch["noise"][b]][ch["offset"][b]:ch["offset"][b] + 8000].astype(np.float64)
        y = np.convolve(x[b].astype(np.float64), rirs[ch["rir"][b]].astype(np.float64))[:8000]
        y *= np.sqrt(np.mean(x[b].astype(np.float64) ** 2) / np.mean(y ** 2))
        resid = out[b] - y
        snr = 10 * np.log10(np.mean(y ** 2) / np.mean(resid ** 2))
        assert abs(snr - 10.0) < 1e-6
        assert np.allclose(resid / np.sqrt(np.mean(resid ** 2)), n / np.sqrt(np.mean(n ** 2)), atol=1e-9)
    # probabilities 0 -> identity (up to the clip)
    out0, _ = oa.audio_augment(x, rirs, noises, 0.0, 0.0, 5.0, 20.0)
    assert np.array_equal(out0, np.clip(x.astype(np.float64), -1, 1))
    # no banks -> identity
    out1, ch1 = oa.audio_augment(x, None, None, 1.0, 1.0, 5.0, 20.0)
    assert np.array_equal(out1, out0) and (ch1["rir"] == -1).all() and (ch1["noise"] == -1).all()


# ---------------------------------------------------------------------------------------------------- GPU parity
def _run_device(x, rirs, noises, fft=False, **kw):
    from wakeword_trainer_home_amd import _native as nat
    dev = torch.device("cuda:0")
    t = lambda a: None if a is None else torch.from_numpy(a).to(dev)
    spectra = nat.audio_rir_spectra(t(rirs)) if (fft and rirs is not None) else None
    out, ch = nat.audio_augment(t(x), t(rirs), t(noises), want_choices=True, rir_spectra=spectra, **kw)
    torch.cuda.synchronize()
    return out.cpu().numpy(), ch.cpu().numpy()


def _check(x, rirs, noises, rir_prob, noise_prob, smin, smax, seed=0, step=0, sample_offset=0, atol=None, fft=False, ref=None,
           tag="augment"):
    """Device against the float64 oracle (or a closed-form ``ref``) within input_stage.waveform_bound; choices bit-exact."""
    out, ch = _run_device(x, rirs, noises, fft=fft, rir_prob=rir_prob, noise_prob=noise_prob, snr_min_db=smin, snr_max_db=smax,
                          seed=seed, step=step, sample_offset=sample_offset)
    oref, rch = oa.audio_augment(x, rirs, noises, rir_prob, noise_prob, smin, smax, seed, step, sample_offset)
    f32, _ = oa.audio_augment(x, rirs, noises, rir_prob, noise_prob, smin, smax, seed, step, sample_offset, dtype=np.float32)
    e32 = float(np.abs(f32 - oref).max())
    yard = e32
    if atol is None:
        c = S.aug_call(x, rirs, noises, rir_prob, noise_prob, smin, smax, seed, step, sample_offset)
        yard = e32 if fft else max(e32, S.aug_e_seq(c, oref))
        atol = S.waveform_bound(e32, fft, yard)
    assert np.array_equal(ch[:, 0], rch["rir"]) and np.array_equal(ch[:, 1], rch["noise"])
    assert np.array_equal(ch[:, 2], rch["offset"])
    assert np.allclose(ch[:, 3].copy().view(np.float32), rch["snr_db"], rtol=0, atol=2e-6)
    assert np.isfinite(out).all() and np.abs(out).max() <= 1.0
    err = np.abs(out - (oref if ref is None else ref)).max()
    S.measured(f"{tag} {'fft' if fft else 'direct'}", err, yard, atol)
    assert err <= atol, (err, atol, e32)
    return out, ch


def _check_call(c, fft, **kw):
    return _check(c["x"], c["rirs"], c["noises"], c["rir_prob"], c["noise_prob"], c["smin"], c["smax"], c["seed"], c["step"],
                  c["sample_offset"], fft=fft, **kw)


@pytest.mark.gpu
@pytest.mark.parametrize("fft", [False, True], ids=["direct", "fft"])
@pytest.mark.parametrize("B,N,L", S.MATCH_SHAPES)
def test_device_matches_oracle(B, N, L, fft):
    """Both forms of the convolution: direct time-domain, and overlap-save FFT (1, 2 and 3+ segments per clip)."""
    for c in S.match_calls(B, N, L):
        _check_call(c, fft)


@pytest.mark.gpu
@pytest.mark.parametrize("fft", [False, True], ids=["direct", "fft"])
@pytest.mark.parametrize("N", S.TWO_TAP_N)
@pytest.mark.parametrize("L", S.TWO_TAP_L)
def test_convolution_alone_matches_closed_form(N, L, fft):
    """A two-tap bank h[0] = 1, h[L-1] = 0.5 and no noise: the reference is y[t] = x[t] + 0.5 x[t-L+1] and the loudness scale
    (the oracle equals it exactly, test_input_stage_bounds.py).  A seam one sample off -- a tile's history, a segment's head,
    the padded tail of a length that is no multiple of 8 -- moves a full-size sample here."""
    c = S.two_tap_call(N, L)
    _check_call(c, fft, ref=S.two_tap_closed_form(c["x"], L), tag=f"two-tap N={N} L={L}")


@pytest.mark.gpu
@pytest.mark.parametrize("fft", [False, True], ids=["direct", "fft"])
def test_mix_alone_on_a_planted_noise_bank(fft):
    """No RIR (the FFT form then copies), every clip mixed; a sample of +3 sits just before and one of -3 just after each clip's
    noise segment, so noise statistics over a window one sample off move the output by 1e-2 and more."""
    out, ch = _check_call(S.mix_alone_call(), fft, tag="mix alone")
    assert (ch[:, 0] == -1).all() and (ch[:, 1] >= 0).all()


@pytest.mark.gpu
@pytest.mark.parametrize("fft", [False, True], ids=["direct", "fft"])
def test_saturating_mix(fft):
    """Loud clips under loud noise, both effects on: a fifth of the samples end on the rails, the others do not, and both kinds
    are under the bound (with quiet inputs |out| <= 1 holds trivially)."""
    c = S.saturation_call()
    out, _ = _check_call(c, fft, tag="saturation")
    ref, _ = S.aug_oracle(c)
    share = float(np.mean(np.abs(ref) == 1.0))
    assert 0.1 <= share <= 0.5, share
    assert abs(float(np.mean(np.abs(out) == 1.0)) - share) < 1e-3


@pytest.mark.gpu
@pytest.mark.parametrize("fft", [False, True], ids=["direct", "fft"])
def test_wide_philox_words(fft):
    """Seed, step and sample offset beyond 32 bits: choices bit-exact, waveform within the bound."""
    _check_call(S.wide_philox_call(), fft, tag="wide philox")


@pytest.mark.gpu
def test_fft_and_direct_forms_agree_at_full_batch():
    """BASELINE-sized batch (512 clips x 24000 samples, 4000-tap RIRs): the two device forms against each other
    (the float64 oracle covers the small cases above)."""
    from wakeword_trainer_home_amd import _native as nat
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(3)
    x = 0.2 * torch.randn(512, 24000, device=dev, generator=g)
    rirs = torch.randn(16, 4000, device=dev, generator=g) * torch.exp(-torch.arange(4000, device=dev) / 700.0)
    noises = 0.1 * torch.randn(8, 160000, device=dev, generator=g)
    kw = dict(rir_prob=0.25, noise_prob=0.5, snr_min_db=5.0, snr_max_db=20.0, seed=1, step=9, want_choices=True)
    a, ca = nat.audio_augment(x, rirs, noises, **kw)
    b, cb = nat.audio_augment(x, rirs, noises, rir_spectra=nat.audio_rir_spectra(rirs), **kw)
    assert torch.equal(ca, cb)
    assert 0.15 < (ca[:, 0] >= 0).float().mean() < 0.35 and 0.4 < (ca[:, 1] >= 0).float().mean() < 0.6
    assert torch.isfinite(b).all() and (a - b).abs().max().item() <= 1e-4
    plain = (ca[:, 0] < 0) & (ca[:, 1] < 0)                       # untouched clips are bit-exact copies
    assert torch.equal(b[plain], x[plain].clamp(-1, 1))


@pytest.mark.gpu
def test_device_edge_cases():
    calls = S.edge_case_calls()
    first = calls[0][0]                                         # Nn == N: the only offset is 0
    out, ch = _check_call(first, False)
    assert (ch[:, 2] == 0).all()
    # effects off / banks absent: clipped copy, bit-exact
    x, rirs, noises = first["x"], first["rirs"], first["noises"]
    for args in ((rirs, noises, 0.0, 0.0), (None, None, 1.0, 1.0)):
        o, c = _run_device(x * 5, args[0], args[1], rir_prob=args[2], noise_prob=args[3], snr_min_db=5.0, snr_max_db=20.0)
        assert np.array_equal(o, np.clip(x * 5, -1, 1)) and (c[:, :2] == -1).all()
    # silent clip and silent noise (no NaN from 0/0); only one of the banks
    for c, forms in calls[1:]:
        for fft in forms:
            _check_call(c, fft)


@pytest.mark.gpu
def test_device_rejects_bad_arguments():
    from wakeword_trainer_home_amd import _native as nat
    dev = torch.device("cuda:0")
    x = torch.zeros(2, 4000, device=dev)
    with pytest.raises(nat.NativeError):
        nat.audio_augment(x, torch.zeros(1, 9000, device=dev), None, 1.0, 0.0, 5.0, 20.0)     # RIR too long
    with pytest.raises(ValueError):
        nat.audio_augment(x, None, torch.zeros(1, 3999, device=dev), 0.0, 1.0, 5.0, 20.0)     # noise shorter than N
    with pytest.raises(ValueError):
        nat.audio_augment(x, None, None, 0.0, 0.0, 20.0, 5.0)                                 # snr range reversed
    with pytest.raises(ValueError):
        nat.audio_augment(x.double(), None, None, 0.0, 0.0, 5.0, 20.0)


@pytest.mark.gpu
def test_audio_augmentation_class_and_trainer_hook(tmp_path):
    """Constructor and call contract of tests/test_training_pipeline.py:230-243, then the Trainer applies it ahead of the
    log-mel with the step / sample-offset counters of the batch."""
    from wakeword_trainer_home_amd.data.augmentation import AudioAugmentation
    from wakeword_trainer_home_amd.data.dataset import make_synthetic_batch
    from oracle import features as of
    rng = np.random.default_rng(1)
    aug = AudioAugmentation(sample_rate=16000, device="cuda", time_stretch_range=(0.8, 1.2), pitch_shift_range=(-2, 2),
                            background_noise_prob=0.5)
    a = torch.randn(1, 16000, device="cuda")
    o = aug(a)
    assert o.shape == a.shape and torch.isfinite(o).all()
    rirs, noises = _banks(rng, R=4, L=800, K=3, Nn=30000)
    aug = AudioAugmentation(device="cuda", background_noise_prob=0.7, rir_prob=0.5, rirs=rirs, noises=noises, seed=9)
    x = (0.2 * rng.standard_normal((8, 24000))).astype(np.float32)
    o0 = aug(torch.from_numpy(x), return_choices=True).cpu().numpy()
    ref0, rch = oa.audio_augment(x, rirs, noises, 0.5, 0.7, 5.0, 20.0, seed=9, step=0)
    assert np.array_equal(aug.last_choices[:, 0].cpu().numpy(), rch["rir"]) and np.abs(o0 - ref0).max() <= 1e-4
    o1 = aug(torch.from_numpy(x)).cpu().numpy()                      # the call counter advanced the stream
    ref1, _ = oa.audio_augment(x, rirs, noises, 0.5, 0.7, 5.0, 20.0, seed=9, step=1)
    assert np.abs(o1 - ref1).max() <= 1e-4 and np.abs(o1 - o0).max() > 1e-3
    xi = (x * 32767).astype(np.int16)                                # int16 PCM input
    oi = aug(torch.from_numpy(xi), step=0).cpu().numpy()
    refi, _ = oa.audio_augment(xi.astype(np.float32) / 32768.0, rirs, noises, 0.5, 0.7, 5.0, 20.0, seed=9, step=0)
    assert np.abs(oi - refi).max() <= 1e-4

    # Trainer hook: features of step 2 == log-mel(waveform augmented with step=2, offset=rank*B); SpecAugment off
    from wakeword_trainer_home_amd.config import get_preset
    from wakeword_trainer_home_amd.models import create_model
    from wakeword_trainer_home_amd.training import Trainer
    cfg = get_preset("cnn_small_logmel40")
    cfg.training.epochs, cfg.optimizer.warmup_epochs, cfg.training.batch_size = 1, 0, 8
    cfg.augmentation.n_freq_masks = cfg.augmentation.n_time_masks = 0
    y = torch.zeros(8, dtype=torch.long)
    batches = [(torch.from_numpy(x), y, [{"path": "s"}] * 8)]
    tr = Trainer(create_model("cnn_small"), batches, batches, cfg, checkpoint_dir=tmp_path, device="cuda")
    tr.audio_augmentation = aug
    feats = tr._features(torch.from_numpy(x), training=True, step=2).cpu().numpy()
    w2 = aug(torch.from_numpy(x), step=2).cpu().numpy()
    ref2, _ = oa.audio_augment(x, rirs, noises, 0.5, 0.7, 5.0, 20.0, seed=9, step=2)
    assert np.abs(w2 - ref2).max() <= 1e-4
    lm = of.logmel(w2)
    assert np.abs(feats.reshape(lm.shape) - lm).max() <= 2e-3
    ev = tr._features(torch.from_numpy(x), training=False).cpu().numpy()      # evaluation: no augmentation
    assert np.abs(ev.reshape(lm.shape) - of.logmel(x)).max() <= 2e-3
    tr.train_epoch(0)                                                          # and a full step runs through it
    assert np.isfinite(tr.train_metrics_tracker.compute().accuracy)
