"""Time-stretch / pitch-shift on the GPU (ww_audio_tsm) against the restated law of tests/tsm_cases.py.

The search is a chain of argmax decisions, so the device is held in three ways.  Teacher-forced synthesis: its waveform
against the float64 law run with the device's own offsets, under the fp32 round-off bound ``tsm_cases.waveform_bound``.
Teacher-forced search: every offset it chose is, by the float64 correlations, within the round-off of an fp32 dot product of
the best one.  Free-running: on the clips whose margins exceed that round-off (tests/test_tsm_host.py shows the noise clips
do), its offsets ARE the law's."""
import functools

import numpy as np
import pytest
import torch

from oracle import audio_augment as OA
from tests import input_stage as S
from tests import tsm_cases as T

UNTOUCHED = 32000          # no offset has this value: what delta_out holds before the call


def _run(c):
    """-> (out (B,N), choices (B,3) int32, delta (B, max_grains) int16) of one device call."""
    from wakeword_trainer_home_amd import _native as nat
    dev = torch.device("cuda:0")
    x = torch.from_numpy(c["x"]).to(dev)
    B, N = x.shape
    delta = torch.full((B, nat.audio_tsm_max_grains(N, c["pmax"])), UNTOUCHED, dtype=torch.int16, device=dev)
    out, ch = nat.audio_tsm(x, c["stretch_prob"], c["rmin"], c["rmax"], c["pitch_prob"], c["pmin"], c["pmax"], seed=c["seed"],
                            step=c["step"], sample_offset=c["sample_offset"], want_choices=True, delta_out=delta)
    return out.cpu().numpy(), ch.cpu().numpy(), delta.cpu().numpy()


@functools.lru_cache(maxsize=None)
def _fixed(B, N, rate, semis):
    c = T.fixed_call(B, N, rate, semis)
    return c, _run(c)


def _selected(ref):
    return ref["stretch"] | (ref["semis"] != 0)


def _check_choices(c, ch):
    ref = T.choices(len(c["x"]), *T.call_args(c))
    assert np.array_equal(ch[:, 0], ref["stretch"].astype(np.int32))
    assert np.array_equal(ch[:, 1].view(np.float32).view(np.uint32), ref["rate"].view(np.uint32))
    assert np.array_equal(ch[:, 2], ref["semis"])
    return ref


def _check_delta_shape(c, ref, delta):
    """Offsets of the selected clips lie in [-DELTA, DELTA]; whatever lies past a clip's last grain, and every row of a
    copied clip, is untouched."""
    N = c["x"].shape[1]
    for b, on in enumerate(_selected(ref)):
        G = T.fixed_point(N, ref["rate"][b], ref["semis"][b])["G"] if on else 0
        assert (np.abs(delta[b, :G].astype(np.int64)) <= T.DELTA).all(), (b, delta[b, :G])
        assert (delta[b, G:] == UNTOUCHED).all(), b


def _check_synthesis(c, out, delta, tag):
    ref64, ch, _ = T.tsm(c["x"], *T.call_args(c), forced=delta)
    ref32, _, _ = T.tsm(c["x"], *T.call_args(c), forced=delta, dtype=np.float32)
    on = _selected(ch)
    assert np.array_equal(out[~on], c["x"][~on]), "a clip with neither effect must be a bit-exact copy"
    if on.any():
        e32 = S.per_clip_err(ref32[on], ref64[on])
        err = S.per_clip_err(out[on], ref64[on])
        bound = np.array([T.waveform_bound(e) for e in e32])
        S.measured(tag, err, e32, bound)
        for b, e, bd in zip(np.flatnonzero(on), err, bound):
            assert e < bd, f"{tag} clip {b}: max abs err {e:.3e} (bound {bd:.2e})"


def _check_search(c, ref, delta):
    """No grain is exempt: with the device's own p_{m-1}, max c - c(d_dev) <= gamma, and d_dev = -DELTA where every c is 0."""
    N = c["x"].shape[1]
    for b in np.flatnonzero(_selected(ref)):
        x64 = c["x"][b].astype(np.float64)
        fx = T.fixed_point(N, ref["rate"][b], ref["semis"][b])
        p_prev = 0
        for m in range(1, fx["G"] + 1):
            a = T.grain_anchor(m, fx)
            cc, s = T.grain_scores(x64, p_prev, a)
            jd, jb = int(delta[b, m - 1]) + T.DELTA, int(np.argmax(cc))
            if not cc.any():
                assert jd == 0, f"clip {b} grain {m}: every correlation is 0, d must be -DELTA, got {jd - T.DELTA}"
            assert cc[jb] - cc[jd] <= T.gamma(s[jb], s[jd]), (b, m, jd - T.DELTA, jb - T.DELTA, cc[jb] - cc[jd])
            p_prev = a + jd - T.DELTA


@pytest.mark.gpu
@pytest.mark.parametrize("rate,semis", T.FIXED)
@pytest.mark.parametrize("B,N", T.SHAPES)
def test_fixed_cases_teacher_forced(B, N, rate, semis):
    """Choices bit-exact; the waveform against the law run with the device's offsets; every offset within round-off of the best."""
    c, (out, ch, delta) = _fixed(B, N, rate, semis)
    ref = _check_choices(c, ch)
    assert ref["stretch"].all() and (ref["rate"] == np.float32(rate)).all() and (ref["semis"] == semis).all()
    _check_delta_shape(c, ref, delta)
    _check_synthesis(c, out, delta, f"tsm ({B},{N}) rate {rate} semis {semis}")
    _check_search(c, ref, delta)


@pytest.mark.gpu
@pytest.mark.parametrize("rate,semis", T.FIXED)
@pytest.mark.parametrize("B,N", T.SHAPES)
def test_fixed_cases_free_running(B, N, rate, semis):
    """On the clips that pass the precondition -- the noise clips all do -- the device's offsets are the law's outright."""
    c, (_, _, delta) = _fixed(B, N, rate, semis)
    free = [b for b in range(B + 1) if T.free_running_ok(c["x"][b], rate, semis) > 1.0]
    assert set(range(B)) <= set(free)
    for b in free:
        d = T.tsm_clip(c["x"][b], rate, semis)[1]
        assert np.array_equal(delta[b, :len(d)], d), (b, delta[b, :len(d)], d)


@pytest.mark.gpu
def test_wide_philox_words_and_full_ranges():
    """Seed, step and sample offset beyond 32 bits, rates over [0.5, 2] and every semitone of [-12, 12]."""
    c = T.wide_philox_call()
    out, ch, delta = _run(c)
    ref = _check_choices(c, ch)
    assert 0 < _selected(ref).sum()
    _check_delta_shape(c, ref, delta)
    _check_synthesis(c, out, delta, "tsm wide philox")
    _check_search(c, ref, delta)


@pytest.mark.gpu
def test_mixed_probabilities():
    """Half the clips stretched, half shifted: the clips with neither effect are bit-exact copies, the others within the bound."""
    c = T.mixed_call()
    out, ch, delta = _run(c)
    ref = _check_choices(c, ch)
    on = _selected(ref)
    assert 8 <= (~on).sum() <= 40 and 0.3 < ref["stretch"].mean() < 0.7
    _check_delta_shape(c, ref, delta)
    _check_synthesis(c, out, delta, "tsm mixed")
    _check_search(c, ref, delta)


@pytest.mark.gpu
def test_probabilities_zero_copy():
    c = dict(T.mixed_call(B=5, N=700), stretch_prob=0.0, pitch_prob=0.0)
    out, ch, delta = _run(c)
    assert np.array_equal(out, c["x"]) and (delta == UNTOUCHED).all()
    assert not ch[:, 0].any() and (ch[:, 1].view(np.float32) == 1.0).all() and not ch[:, 2].any()


@pytest.mark.gpu
def test_device_rejects_bad_arguments():
    from wakeword_trainer_home_amd import _native as nat
    dev = torch.device("cuda:0")
    x = torch.zeros(2, 700, device=dev)
    for args in ((1.0, 0.4, 1.2, 1.0, -2, 2), (1.0, 0.8, 2.5, 1.0, -2, 2), (1.0, 1.2, 0.8, 1.0, -2, 2),
                 (1.0, 0.8, 1.2, 1.0, -13, 2), (1.0, 0.8, 1.2, 1.0, -2, 13), (1.0, 0.8, 1.2, 1.0, 2, -2),
                 (1.5, 0.8, 1.2, 1.0, -2, 2), (1.0, 0.8, 1.2, -0.5, -2, 2)):
        with pytest.raises(ValueError):
            nat.audio_tsm(x, *args)
    with pytest.raises(ValueError):
        nat.audio_tsm(x, 1.0, 0.8, 1.2, 1.0, -2, 2, out=x)                                   # in place
    with pytest.raises(ValueError):
        nat.audio_tsm(x.double(), 1.0, 0.8, 1.2, 1.0, -2, 2)
    with pytest.raises(ValueError):
        nat.audio_tsm(x[:, :0].contiguous(), 1.0, 0.8, 1.2, 1.0, -2, 2)                      # N < 1
    with pytest.raises(ValueError):
        nat.audio_tsm(x, 1.0, 0.8, 1.2, 1.0, -2, 2, delta_out=torch.zeros(2, 1, dtype=torch.int16, device=dev))
    with pytest.raises(nat.NativeError):
        nat.audio_tsm(x, 1.0, 0.8, 1.2, 1.0, -2, 2, scratch=torch.zeros(64, device=dev))   # scratch too small
    assert torch.equal(nat.audio_tsm(x + 0.25, 0.0, 0.8, 1.2, 0.0, -2, 2), x + 0.25)


@pytest.mark.gpu
def test_class_runs_stretch_and_pitch_ahead_of_rir_and_noise(tmp_path):
    """AudioAugmentation with both probabilities 1 equals oracle.audio_augment applied to the restated stretch output (clips
    that pass the free-running precondition); int16 input; from_config; probabilities 0 is today's result; a Trainer epoch."""
    from wakeword_trainer_home_amd import _native as nat
    from wakeword_trainer_home_amd.config import get_preset
    from wakeword_trainer_home_amd.data.augmentation import AudioAugmentation
    from wakeword_trainer_home_amd.models import create_model
    from wakeword_trainer_home_amd.training import Trainer
    c = T.class_call()
    x, rirs, noises = c["x"], c["rirs"], c["noises"]
    aug = AudioAugmentation(device="cuda", time_stretch_prob=1.0, pitch_shift_prob=1.0, background_noise_prob=0.7, rir_prob=0.5,
                            rirs=rirs, noises=noises, seed=c["seed"])
    out = aug(torch.from_numpy(x), step=0, return_choices=True).cpu().numpy()
    mid, ch, _ = T.tsm(x, *T.call_args(c))
    tc = aug.last_tsm_choices.cpu().numpy()
    assert np.array_equal(tc[:, 1].view(np.float32), ch["rate"]) and np.array_equal(tc[:, 2], ch["semis"]) and tc[:, 0].all()
    ref, rch = OA.audio_augment(mid, rirs, noises, 0.5, 0.7, 5.0, 20.0, seed=c["seed"], step=0)
    assert np.array_equal(aug.last_choices[:, 0].cpu().numpy(), rch["rir"])
    err = np.abs(out - ref).max()
    print(f"MEASURED class chain: max err {err:.3e} (bound 1e-4)")
    assert err <= 1e-4
    xi = (x * 32767).astype(np.int16)                                # int16 PCM input
    oi = aug(torch.from_numpy(xi), step=0).cpu().numpy()
    mid_i, _, deltas = T.tsm(xi.astype(np.float32) / 32768.0, *T.call_args(c))
    ref_i, _ = OA.audio_augment(mid_i, rirs, noises, 0.5, 0.7, 5.0, 20.0, seed=c["seed"], step=0)
    assert np.abs(oi - ref_i).max() <= 1e-4

    # both probabilities 0: nothing new runs, the result is bit-equal to the RIR + noise call alone
    plain = AudioAugmentation(device="cuda", background_noise_prob=0.7, rir_prob=0.5, rirs=rirs, noises=noises, seed=c["seed"])
    xd = torch.from_numpy(x).cuda()
    today = nat.audio_augment(xd, plain.rirs, plain.noises, 0.5, 0.7, 5.0, 20.0, seed=c["seed"], step=3, sample_offset=8,
                              rir_spectra=plain.rir_spectra)
    assert torch.equal(plain(xd, step=3, sample_offset=8, return_choices=True), today) and plain.last_tsm_choices is None

    # from_config carries all six knobs
    cfg = get_preset("cnn_small_logmel40")
    a = cfg.augmentation
    a.time_stretch_min, a.time_stretch_max, a.pitch_shift_min, a.pitch_shift_max = 0.9, 1.1, -1, 3
    a.time_stretch_prob, a.pitch_shift_prob = 1.0, 1.0
    fc = AudioAugmentation.from_config(cfg, "cuda", rirs=rirs, noises=noises, seed=c["seed"])
    assert (fc.time_stretch_range, fc.pitch_shift_range, fc.time_stretch_prob, fc.pitch_shift_prob) == ((0.9, 1.1), (-1, 3), 1.0, 1.0)
    fc(torch.from_numpy(x), step=0, return_choices=True)
    want = T.choices(len(x), 1.0, 0.9, 1.1, 1.0, -1, 3, seed=c["seed"])
    got = fc.last_tsm_choices.cpu().numpy()
    assert np.array_equal(got[:, 1].view(np.float32), want["rate"]) and np.array_equal(got[:, 2], want["semis"])

    # a Trainer epoch with the augmentor attached
    cfg.training.epochs, cfg.optimizer.warmup_epochs, cfg.training.batch_size = 1, 0, 8
    rng = np.random.default_rng(2)
    xb = torch.from_numpy((0.2 * rng.standard_normal((8, 24000))).astype(np.float32))
    batches = [(xb, torch.zeros(8, dtype=torch.long), [{"path": "s"}] * 8)]
    tr = Trainer(create_model("cnn_small"), batches, batches, cfg, checkpoint_dir=tmp_path, device="cuda")
    tr.audio_augmentation = AudioAugmentation.from_config(cfg, "cuda", rirs=rirs, noises=np.tile(noises, (1, 5)), seed=1)
    tr.train_epoch(0)
    assert np.isfinite(tr.train_metrics_tracker.compute().accuracy)
