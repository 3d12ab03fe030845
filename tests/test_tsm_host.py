"""Time-stretch / pitch-shift on the CPU: the restated law (tests/tsm_cases.py) means what DESIGN.md says, its choices
follow the Philox stream, the waveform bound of the GPU tests discriminates (defect catalogue), the clips the free-running
GPU test uses pass its precondition, and the library exports the new entry points."""
import ctypes
import functools
import math

import numpy as np
import pytest

from oracle.philox import philox4x32_10, make_ctr, make_key
from oracle import audio_augment as OA
from tests import tsm_cases as T

SR = 16000


# ----------------------------------------------------------------------------------------------------------- meaning
def _tone(f, N=16000, amp=0.5):
    return (amp * np.sin(2 * np.pi * f * np.arange(N) / SR)).astype(np.float32)


def _peak_hz(seg):
    sp = np.abs(np.fft.rfft(seg * np.hanning(len(seg))))
    return np.argmax(sp) * SR / len(seg)


@pytest.mark.parametrize("semis", [-2, 3, 12, -12])
def test_pitch_shift_moves_a_tone_by_the_semitones(semis):
    out, _ = T.tsm_clip(_tone(440.0), 1.0, semis)
    seg = out[2000:10000]                                     # 8000 samples: 2 Hz bins
    want = 440.0 * 2.0 ** (semis / 12.0)
    assert abs(_peak_hz(seg) - want) <= SR / len(seg), (semis, _peak_hz(seg), want)
    assert np.sqrt(np.mean(seg ** 2)) == pytest.approx(0.5 / math.sqrt(2), rel=5e-3)


def test_time_stretch_keeps_pitch_and_level():
    out, _ = T.tsm_clip(_tone(440.0), 0.8, 0)
    seg = out[2000:10000]
    assert _peak_hz(seg) == 440.0
    assert abs(np.sqrt(np.mean(seg ** 2)) - 0.5 / math.sqrt(2)) <= 1e-3


@pytest.mark.parametrize("rate", [0.8, 1.25])
def test_time_stretch_moves_a_burst_to_t0_over_rate(rate):
    """The search may move a grain by DELTA = 128 samples = 8 ms; two grains overlap: 16 ms."""
    N, t0 = 12000, 0.25
    t = np.arange(N) / SR
    rng = np.random.default_rng(4)
    x = (0.5 * rng.standard_normal(N) * np.exp(-0.5 * ((t - t0) / 0.004) ** 2)).astype(np.float32)
    out, _ = T.tsm_clip(x, rate, 0)
    centroid = float(np.sum(t * out ** 2) / np.sum(out ** 2))
    assert abs(centroid - t0 / rate) <= 0.016, (centroid, t0 / rate)


def test_unit_rate_with_zero_offsets_is_the_identity():
    x = T.noise_clips(3, 2048)[0]
    fx = T.fixed_point(len(x), 1.0, 0)
    assert (fx["f_q"], fx["rho_q"], fx["half"], fx["Z"], fx["G"]) == (1 << 20, 65536, 8, 2047 + 10, 8)
    z, d = T.wsola(x, fx, forced=np.zeros(fx["G"], np.int64))
    assert np.abs(z[:len(x)] - x).max() <= 2.0 ** -52 and not z[len(x):].any()     # w[i] + w[i+256] = 1 to one rounding
    out = T.resample(z, fx)
    assert np.array_equal(out, z[:len(x)])                    # semis = 0: the resampler copies z
    # the first hop is x itself, at any rate and pitch (grains -1 and 0)
    fx = T.fixed_point(len(x), 0.7, 5)
    z, _ = T.wsola(x, fx)
    assert np.abs(z[:T.HS] - x[:T.HS]).max() <= 2.0 ** -52


def test_fixed_point_and_sizes():
    assert T.f_q_of(0) == 1 << 20 and T.f_q_of(12) == 1 << 21 and T.f_q_of(-12) == 1 << 19
    assert [T.f_q_of(s) for s in range(-12, 13)] == sorted(T.f_q_of(s) for s in range(-12, 13))
    for s in range(-12, 13):                                  # no f_q sits near a rounding tie, so exp2 and pow agree on it
        v = 2.0 ** (s / 12.0) * 1048576.0
        assert abs(v - math.floor(v) - 0.5) > 1e-6 or s % 12 == 0
    fx = T.fixed_point(24000, 2.0, 12)
    assert (fx["rho_q"], fx["half"], fx["Z"], fx["G"]) == (65536, 16, 2 * 23999 + 18, (2 * 23999 + 17) // 256)
    assert T.max_grains(24000, -3) == T.max_grains(24000, 0) == T.fixed_point(24000, 1.0, 0)["G"]


# ----------------------------------------------------------------------------------------------------------- choices
def test_choices_come_from_draw_2_alone():
    kw = dict(seed=2 ** 40 + 17, step=2 ** 33 + 5, sample_offset=1000)
    ch = T.choices(64, 0.5, 0.8, 1.2, 0.5, -2, 2, **kw)
    g = np.arange(64, dtype=np.uint64) + np.uint64(1000)
    r = philox4x32_10(make_ctr(kw["step"], g, OA.TAG_AUDIO, 2), make_key(kw["seed"])).astype(np.uint64)
    assert np.array_equal(ch["stretch"], r[:, 0] < 2 ** 31) and np.array_equal(ch["pitch"], r[:, 2] < 2 ** 31)
    assert np.array_equal(ch["semis"], np.where(ch["pitch"], -2 + (r[:, 3] % 5).astype(np.int64), 0))
    u = (r[:, 1] >> 8).astype(np.float64) * 2.0 ** -24
    lo, hi = float(np.float32(0.8)), float(np.float32(1.2))
    want = np.where(ch["stretch"], (u * (hi - lo) + lo).astype(np.float32), np.float32(1.0))
    assert ch["rate"].dtype == np.float32 and np.array_equal(ch["rate"], want)
    # draws 0 and 1 (RIR, noise) are what they were: the audio choices do not move when stretch / pitch are configured
    again = T.choices(64, 0.5, 0.8, 1.2, 0.5, -2, 2, **kw)
    assert all(np.array_equal(ch[k], again[k]) for k in ch)
    other_step = T.choices(64, 0.5, 0.8, 1.2, 0.5, -2, 2, **dict(kw, step=kw["step"] + 1))
    assert not np.array_equal(ch["rate"], other_step["rate"])
    shifted = T.choices(64, 0.5, 0.8, 1.2, 0.5, -2, 2, **dict(kw, sample_offset=1003))
    assert not np.array_equal(ch["rate"], shifted["rate"])
    assert all(np.array_equal(ch[k][3:], shifted[k][:-3]) for k in ch)        # clip g is clip g, whatever the batch it is in


def test_choice_rates_and_ranges():
    ch = T.choices(4096, 0.3, 0.7, 1.3, 0.6, -3, 4, seed=1)
    assert abs(ch["stretch"].mean() - 0.3) <= 0.03 and abs(ch["pitch"].mean() - 0.6) <= 0.03
    assert (ch["rate"][~ch["stretch"]] == 1.0).all() and (ch["semis"][~ch["pitch"]] == 0).all()
    r = ch["rate"][ch["stretch"]]
    assert r.min() >= np.float32(0.7) and r.max() <= np.float32(1.3) and r.std() > 0.1
    s = ch["semis"][ch["pitch"]]
    assert set(s.tolist()) == set(range(-3, 5))
    ch = T.choices(256, 1.0, 1.1, 1.1, 1.0, 7, 7, seed=2)
    assert (ch["rate"] == np.float32(1.1)).all() and (ch["semis"] == 7).all() and ch["stretch"].all()
    ch = T.choices(256, 0.0, 0.8, 1.2, 0.0, -2, 2, seed=2)
    assert not ch["stretch"].any() and (ch["rate"] == 1.0).all() and not ch["semis"].any()


def test_a_clip_with_neither_effect_is_a_copy():
    c = T.mixed_call()
    out, ch, deltas = T.tsm(c["x"], *T.call_args(c))
    plain = ~ch["stretch"] & (ch["semis"] == 0)
    assert 4 <= plain.sum() <= 40
    assert np.array_equal(out[plain], c["x"][plain].astype(np.float64)) and all(deltas[b] is None for b in np.flatnonzero(plain))
    # (a clip this short that is only stretched can come out unchanged: the search follows the natural continuation while the
    # drift stays within DELTA; a pitch shift always shows)
    assert all(np.abs(out[b] - c["x"][b]).max() > 1e-3 for b in np.flatnonzero(ch["semis"] != 0))


# --------------------------------------------------------------------------------------------------- defect catalogue
# which shapes catch which defect (computed below, stated here).  A late template and a last-tie need a searched grain, the
# last-tie one whose template or region is empty (a clip end inside the search); the float anchor differs from the fixed point
# only once m HS is large; the missing cutoff shows at the two cases that shift up.
CAUGHT = {
    "template_late": {(3, 300), (4, 700), (3, 2048), (5, 5000), (2, 24000)},
    "hann_symmetric": {(3, 300), (4, 700), (3, 2048), (5, 5000), (2, 24000)},
    "last_tie": {(4, 700), (3, 2048), (5, 5000), (2, 24000)},
    "first_hop_faded": {(3, 300), (4, 700), (3, 2048), (5, 5000), (2, 24000)},
    "a_float": {(2, 24000)},
    "no_cutoff": {(3, 300), (4, 700), (3, 2048), (5, 5000), (2, 24000)},
}


@functools.lru_cache(maxsize=None)
def _shape_rows(B, N):
    """Per fixed case and clip of a shape: the law's output and offsets, the fp32 restatement's error, the bound, the margin."""
    rows = []
    for rate, semis in T.FIXED:
        x = T.fixed_call(B, N, rate, semis)["x"]
        for b in range(B + 1):
            trace = []
            o64, d = T.tsm_clip(x[b], rate, semis, trace=trace)
            o32, _ = T.tsm_clip(x[b], rate, semis, forced=d, dtype=np.float32)
            e32 = float(np.abs(o32 - o64).max())
            rows.append(dict(rate=rate, semis=semis, b=b, x=x[b], out=o64, d=d, e32=e32, bound=T.waveform_bound(e32),
                             margin=min((T.margin_ratio(c, s) for c, s in trace), default=math.inf), harmonic=b == B))
    return rows


@pytest.mark.parametrize("shape", T.SHAPES, ids=str)
def test_fp32_restatement_clears_the_bound_eightfold(shape):
    """The bound rests on the fp32 restatement alone: 8 x its error, floored at 16 * 2**-24 and capped at 1e-4."""
    for r in _shape_rows(*shape):
        assert 1e-8 <= r["e32"] <= 4e-7, (shape, r["rate"], r["semis"], r["e32"])
        assert 8.0 * r["e32"] <= r["bound"] <= 4e-6


@pytest.mark.parametrize("shape", T.SHAPES, ids=str)
def test_every_defect_misses_the_waveform_bound(shape):
    """Each planted mistake stands in for the device: its output misses the bound by a factor of two at least (thousands, in
    fact) at the shapes CAUGHT names, every defect is caught somewhere and every shape catches four or more."""
    worst = {}
    for r in _shape_rows(*shape):
        for name, (_, mode) in T.DEFECTS.items():
            od, dd = T.tsm_clip(r["x"], r["rate"], r["semis"], defect=name)
            ref = r["out"] if mode == "free" else T.tsm_clip(r["x"], r["rate"], r["semis"], forced=dd)[0]
            worst[name] = max(worst.get(name, 0.0), float(np.abs(od - ref).max()) / r["bound"])
    for name, w in worst.items():
        print(f"{name} at {shape}: err / bound up to {w:.3g}")
        assert (w >= 2.0) == (shape in CAUGHT[name]), (name, shape, w)
        assert w >= 1000.0 or w == 0.0, (name, shape, w)       # caught a thousandfold, or not at all
    assert sum(shape in s for s in CAUGHT.values()) >= 4
    assert all(CAUGHT[name] for name in T.DEFECTS) and set(CAUGHT) == set(T.DEFECTS)


def test_unknown_defect_changes_nothing():
    x = T.noise_clips(3, 300)[0]
    assert np.array_equal(T.tsm_clip(x, 0.8, 2, defect=None)[0], T.tsm_clip(x, 0.8, 2)[0])


# ------------------------------------------------------------------------------------------- free-running precondition
@pytest.mark.parametrize("shape", T.SHAPES, ids=str)
def test_noise_clips_pass_the_free_running_precondition(shape):
    """Every grain's margin between the best and the second-best correlation exceeds 2 gamma, gamma = LW * 2**-24 * (S_best +
    S_second): whatever order the device sums in, it finds the same offset.  The harmonic clip need not (and mostly does not)."""
    rows = _shape_rows(*shape)
    worst = min(r["margin"] for r in rows if not r["harmonic"])
    print(f"{shape}: smallest margin / (2 gamma) over the noise clips {worst:.3g}; harmonic clip "
          f"{min(r['margin'] for r in rows if r['harmonic']):.3g}")
    assert worst > 1.0


def test_class_call_clips_pass_the_precondition():
    c = T.class_call()
    ch = T.choices(len(c["x"]), *T.call_args(c))
    assert ch["stretch"].all() and len(set(ch["semis"].tolist())) >= 2
    assert min(T.free_running_ok(c["x"][b], ch["rate"][b], ch["semis"][b]) for b in range(len(c["x"]))) > 1.0


def test_gamma_bounds_fp32_dot_products_in_any_order():
    """The premise of the search tests, on the data they use: fp32 sums of the 512 products, forward, backward and pairwise,
    stay within LW * 2**-24 * sum |x_i tau_i| of float64."""
    x = T.noise_clips(5, 5000)[1]
    tau, region = T._seg(x, 256, T.LW), T._seg(x, 700, T.LW)
    exact = float(np.dot(region.astype(np.float64), tau.astype(np.float64)))
    bound = T.gamma(np.abs(region.astype(np.float64) * tau).sum(), 0.0)
    prod = region * tau
    sums = [np.cumsum(prod, dtype=np.float32)[-1], np.cumsum(prod[::-1], dtype=np.float32)[-1], np.sum(prod, dtype=np.float32)]
    assert all(abs(float(s) - exact) <= bound for s in sums)


# ------------------------------------------------------------------------------------------------- library and class
def test_library_exports_the_tsm_entry_points():
    from wakeword_trainer_home_amd import _native as nat
    names = ("ww_audio_tsm", "ww_audio_tsm_max_grains", "ww_audio_tsm_scratch_bytes")
    lib = ctypes.CDLL(str(nat.lib_path()))
    assert all(n in nat.EXPORTS and hasattr(lib, n) for n in names)
    lib = nat.load()
    assert lib.ww_abi_version() == 17 == nat.ABI_VERSION
    assert ctypes.sizeof(nat.AudioTsmCfg) == 24
    for N in (1, 300, 700, 2048, 5000, 24000, 40000):         # host-only sizes follow the restatement
        for smax in (-12, -3, 0, 2, 7, 12):
            G = T.max_grains(N, smax)
            assert nat.audio_tsm_max_grains(N, smax) == G
            Z = T.fixed_point(N, 1.0, max(smax, 0))["Z"]
            assert lib.ww_audio_tsm_scratch_bytes(3, N, smax) == 3 * Z * 4 and G == (Z - 1) // T.HS
    assert lib.ww_audio_tsm_scratch_bytes(0, 300, 0) == 0 and lib.ww_audio_tsm_scratch_bytes(2, 0, 0) == 0
    assert lib.ww_audio_tsm_scratch_bytes(2, 300, 13) == 0 and nat.audio_tsm_max_grains(300, 13) == 0


def test_augmentation_class_validates_and_reads_the_config():
    from wakeword_trainer_home_amd.config import get_default_config, AugmentationConfig
    from wakeword_trainer_home_amd.data.augmentation import AudioAugmentation
    aug = AudioAugmentation(device="cuda")
    assert (aug.time_stretch_prob, aug.pitch_shift_prob) == (0.0, 0.0) and aug.last_tsm_choices is None
    for kw in (dict(time_stretch_range=(0.4, 1.2)), dict(time_stretch_range=(0.8, 2.5)), dict(time_stretch_range=(1.2, 0.8)),
               dict(pitch_shift_range=(-13, 2)), dict(pitch_shift_range=(-2, 13)), dict(pitch_shift_range=(2, -2)),
               dict(pitch_shift_range=(-1.5, 2)), dict(time_stretch_prob=1.5), dict(pitch_shift_prob=-0.1)):
        with pytest.raises(ValueError):
            AudioAugmentation(device="cuda", **kw)
    assert (AugmentationConfig().time_stretch_prob, AugmentationConfig().pitch_shift_prob) == (0.0, 0.0)
    cfg = get_default_config()
    a = cfg.augmentation
    a.time_stretch_min, a.time_stretch_max, a.pitch_shift_min, a.pitch_shift_max = 0.9, 1.1, -1, 3
    a.time_stretch_prob, a.pitch_shift_prob = 0.7, 0.4
    a.background_noise_prob, a.noise_snr_min, a.noise_snr_max, a.rir_prob = 0.6, 3.0, 15.0, 0.2
    aug = AudioAugmentation.from_config(cfg, device="cuda", seed=11)
    assert (aug.time_stretch_range, aug.pitch_shift_range) == ((0.9, 1.1), (-1, 3))
    assert (aug.time_stretch_prob, aug.pitch_shift_prob) == (0.7, 0.4)
    assert (aug.background_noise_prob, aug.noise_snr_range, aug.rir_prob, aug.seed) == (0.6, (3.0, 15.0), 0.2, 11)
    assert aug.sample_rate == cfg.data.sample_rate and aug.rirs is None and aug.noises is None
    assert type(cfg).from_dict(cfg.to_dict()).augmentation.time_stretch_prob == 0.7          # the knobs survive a round trip
