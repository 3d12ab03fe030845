"""The parity bounds of the input stage discriminate (CPU only): for the very inputs the GPU tests feed the device
(tests/input_stage.py), the independent fp32 yardsticks clear the bounds with room to spare and every catalogued defect --
the float64 law with exactly one planted mistake (oracle.features.DEFECTS, oracle.audio_augment.DEFECTS), standing in for
the device output -- misses them by a factor of two or more, on every kernel path.  The bound functions are the ones the GPU
tests call."""
import math

import numpy as np
import pytest

from oracle import audio_augment as OA
from oracle import features as OF
from tests import input_stage as S

PATHS = ("lt1024", "eq1024", "gt1024")     # k_logmel on zero-extended frames, k_logmel as built, k_logmel_any
LOGMEL_DEFECTS = [d for d in OF.DEFECTS if d != "dct_row0_unscaled"]
# The int16-scale defect moves log(mel + 1e-6) by 2 ln(32768/32767) * mel / (mel + 1e-6): twice TIGHT up to the log's
# epsilon, which at a band of power >= 1 is a relative 1e-6.
INT16_FACTOR = 2.0 * (1.0 - 1e-6)


@pytest.fixture(scope="module")
def frontend():
    """Per input set: the oracle, the yardsticks, the bounds and every defect's per-clip error / bound."""
    rows = []
    for s in S.frontend_input_sets():
        x, kw = s["x"], s["kw"]
        x64 = S.as_float(x)
        ref = OF.logmel(x64, **kw)
        t32 = S.logmel_t32(x64, ref, **kw)
        bound = S.logmel_bounds(t32)
        r = dict(s, ref=ref, t32=t32, bound=bound, at_ceiling=bound >= S.old_logmel_bounds(t32), ratio={},
                 silent=np.abs(x64).max(axis=1) == 0)
        for d in LOGMEL_DEFECTS:
            if d == "int16_scale_32767":
                if x.dtype != np.int16:
                    continue
                out = OF.logmel(OF.pcm16_to_float(x, d), **kw)
            else:
                out = OF.logmel(x64, defect=d, **kw)
            r["ratio"][d] = S.per_clip_err(out, ref) / bound
        if s["n_mfcc"]:
            refm = OF.mfcc(x64, n_mfcc=s["n_mfcc"], **kw)
            r["mfcc_bound"] = S.mfcc_bounds(bound, refm, kw.get("n_mels", 40), S.mfcc_ceiling(**kw))
            r["mfcc_t32"] = S.mfcc_t32(x64, refm, s["n_mfcc"], **kw)
            r["ratio"]["dct_row0_unscaled"] = S.per_clip_err(OF.mfcc(x64, n_mfcc=s["n_mfcc"], defect="dct_row0_unscaled", **kw),
                                                             refm) / r["mfcc_bound"]
        rows.append(r)
    return rows


def test_defaults_are_the_spec():
    x = S.waves(3, 3000, seed=1)
    assert np.array_equal(OF.logmel(x, defect=None), OF.logmel(x))
    assert np.array_equal(OF.pcm16_to_float(S.to_int16(x)), S.to_int16(x).astype(np.float64) / 32768.0)
    for d in OF.DEFECTS:
        out = OF.logmel(OF.pcm16_to_float(S.to_int16(x), d), defect=d) if d != "dct_row0_unscaled" else \
            OF.mfcc(x, defect=d)
        ref = OF.logmel(OF.pcm16_to_float(S.to_int16(x))) if d != "dct_row0_unscaled" else OF.mfcc(x)
        assert np.abs(out - ref).max() > 5e-5, d                   # (each knob does change the result)
    with pytest.raises(ValueError):
        OF.logmel(x, defect="no such defect")
    assert np.array_equal(OF.round_to([1.0 + 2.0 ** -9, 1.0 + 2.0 ** -8 + 2.0 ** -9, 65504.0], "bf16"),
                          [1.0, 1.0 + 2.0 ** -7, 65536.0])         # ties to even, carry into the exponent


def test_logmel_yardstick_clears_its_bound_fourfold_and_only_pure_tones_sit_at_the_old_ceiling(frontend):
    """From t32 alone.  bound = min(old, max(TIGHT, 4 t32)): the yardstick has its factor of 4 wherever the old rule is not
    what binds.  The old rule binds only on a clip on the fp32 round-off floor of any fp32 STFT under log(mel + 1e-6): the
    pure sweep (clip 1 of ``waves``), and the two int16 extremes -- a full-scale Nyquist tone and a full-scale DC, pure tones
    too, held by the same function."""
    for r in frontend:
        assert (r["bound"] >= S.TIGHT).all() and (r["bound"] <= S.old_logmel_bounds(r["t32"])).all(), r["id"]
        free = ~r["at_ceiling"]
        assert (4.0 * r["t32"][free] <= r["bound"][free]).all(), r["id"]
        allowed = {"waves": {1}, "nosweep": set(), "tones": {0, 1}}[r["layout"]]
        assert set(np.flatnonzero(r["at_ceiling"])) <= allowed, (r["id"], r["t32"])
        if r["layout"] == "waves":                                 # clip 0 (noise) is held below 1e-4 in every case ...
            assert r["bound"][0] < 1e-4 or r["id"].startswith("fft-512-128-128-5000"), (r["id"], r["bound"])
    # ... and to TIGHT itself in all but the one with one-bin low bands; there only the silent clip is (fine: per path)
    loose = [r["id"] for r in frontend if r["layout"] == "waves" and r["bound"][0] != S.TIGHT]
    assert all(i.startswith("fft-512-128-128-5000") for i in loose), loose


def test_mfcc_yardstick_clears_its_bound_fourfold(frontend):
    """The fp32 torch MFCC against sqrt(n_mels) * bound_b + 4 * 2**-24 * max|ref_b|: a factor of 4 to spare on every clip but
    two kinds.  A clip at the flat 2e-3 / 3e-3 ceiling (the sweep, as in the log-mel; the square of the 128-band corner,
    0.7 % of it) is only asked to pass.  A silent clip has a factor of 2: its c0 = -13.8 sqrt(n_mels) is an fp32 running
    sum of n_mels equal terms, which no term of the bound models (1.1e-4 at 80 bands against 3.0e-4; 40 and 64 bands clear it fourfold as well)."""
    n = 0
    for r in frontend:
        if r["n_mfcc"]:
            ratio = r["mfcc_t32"] / r["mfcc_bound"]
            at_ceiling = r["mfcc_bound"] >= S.mfcc_ceiling(**r["kw"])
            allowed = {1} if r["layout"] == "waves" else {3} if "corner" in r["id"] else set()
            assert set(np.flatnonzero(at_ceiling)) <= allowed, r["id"]
            room = np.where(at_ceiling, 1.0, np.where(r["silent"], 2.0, 4.0))
            assert (room * ratio <= 1.0).all(), (r["id"], ratio)
            n += 1
    assert n >= 3 * len(PATHS)


@pytest.mark.parametrize("defect", list(OF.DEFECTS))
def test_every_frontend_defect_misses_the_bound_on_every_path(frontend, defect):
    factor = INT16_FACTOR if defect == "int16_scale_32767" else 2.0
    for path in PATHS:
        worst = max(((r["ratio"][defect].max(), r) for r in frontend if r["path"] == path and defect in r["ratio"]),
                    key=lambda t: t[0])
        print(f"{defect} on {path}: err / bound up to {worst[0]:.3g} ({worst[1]['id']})")
        assert worst[0] >= factor, (defect, path, worst[0])
        # the negative control through the very helper the GPU tests call
        r = worst[1]
        x64 = S.as_float(r["x"])
        with pytest.raises(AssertionError):
            if defect == "dct_row0_unscaled":
                S.assert_mfcc_close(OF.mfcc(x64, n_mfcc=r["n_mfcc"], defect=defect, **r["kw"]), x64, r["n_mfcc"], **r["kw"])
            else:
                out = OF.logmel(OF.pcm16_to_float(r["x"], defect) if defect == "int16_scale_32767" else x64,
                                defect=None if defect == "int16_scale_32767" else defect, **r["kw"])
                S.assert_logmel_close(out, r["ref"], x64, **r["kw"])


def test_int16_scale_defect_is_caught_on_a_loud_clip_held_to_tight(frontend):
    for path in PATHS:
        hits = [(r["id"], b) for r in frontend if r["path"] == path and "int16_scale_32767" in r["ratio"]
                for b in range(len(r["bound"]))
                if not r["silent"][b] and r["bound"][b] == S.TIGHT and r["ratio"]["int16_scale_32767"][b] >= INT16_FACTOR]
        assert hits, path
    assert abs(S.TIGHT - 3.0518e-5) < 1e-9


def test_the_yardstick_itself_passes_the_gpu_helpers(frontend):
    """The helpers accept an honest fp32 implementation: the fp32 torch.stft formulation in the device's place."""
    for r in frontend[::4]:
        x64 = S.as_float(r["x"])
        S.assert_logmel_close(OF.logmel_torch(x64, **r["kw"]).numpy(), r["ref"], x64, **r["kw"])
        if r["n_mfcc"]:
            S.assert_mfcc_close(OF.logmel_torch(x64, n_mfcc=r["n_mfcc"], **r["kw"]).numpy(), x64, r["n_mfcc"], **r["kw"])


def test_device_order_restatement_is_honest_and_explains_the_nyquist_tone(frontend):
    """oracle.features.logmel_device_order_f32, the fp32 numpy restatement of the device's order of operations, passes the
    bounds wherever the yardstick applies (it is a fair fp32 implementation) and misses TIGHT on the full-scale Nyquist tone
    sevenfold at n_fft 128 -- as the device does (2.268e-4) -- where pocketfft lands on an exact zero in the empty bins.  That
    clip is the stated exception of input_stage.nyquist_tone_bounds; the DC clip beside it keeps the rule."""
    for r in frontend:
        if r["id"] in ("fft-256-64-40-8000", "logmel-4-16000-{'hop': 256, 'n_mels': 64}", "fft-2048-512-64-24000",
                       "fft-128-160-23-24000-i16", "corner"):
            x64 = S.as_float(r["x"])
            S.assert_logmel_close(OF.logmel_device_order_f32(x64, **r["kw"]), r["ref"], x64, tag="restated " + r["id"], **r["kw"])
        if r["layout"] == "tones":
            x64 = S.as_float(r["x"])
            err = S.per_clip_err(OF.logmel_device_order_f32(x64, **r["kw"]), r["ref"])
            assert err[1] < r["bound"][1], (r["id"], err)
            bounds = S.nyquist_tone_bounds(r["x"], r["ref"], **r["kw"])(r["t32"])
            assert bounds[1] == r["bound"][1] and bounds[0] >= S.old_logmel_bounds(r["t32"])[0] and err[0] < bounds[0]
            if r["path"] == "lt1024":
                assert r["t32"][0] < 1e-5 and err[0] > 5.0 * S.TIGHT, (r["t32"], err)
                assert bounds[0] == 1e-3


# -------------------------------------------------------------------------------------------- waveform augmentation
@pytest.fixture(scope="module")
def augment():
    rows = []
    for id_, c, forms in S.aug_input_calls():
        ref, ch = S.aug_oracle(c)
        e32 = float(np.abs(S.aug_oracle(c, dtype=np.float32)[0] - ref).max())
        ratio = {d: float(np.abs(S.aug_oracle(c, defect=d)[0] - ref).max()) for d in OA.DEFECTS}
        e_seq = S.aug_e_seq(c, ref) if False in forms else 0.0
        rows.append(dict(id=id_, call=c, forms=forms, ref=ref, ch=ch, e32=e32, e_seq=e_seq, err=ratio,
                         bound={fft: S.waveform_bound(e32, fft, 0.0 if fft else e_seq) for fft in forms}))
    return rows


def test_fp32_restatements_clear_the_waveform_bound_fourfold(augment):
    for r in augment:
        for fft in r["forms"]:
            yard = r["e32"] if fft else max(r["e32"], r["e_seq"])
            assert 4.0 * yard <= r["bound"][fft] <= S.WAVE_CEILING / 2, (r["id"], fft, yard)
        assert r["e32"] < 5e-7, (r["id"], r["e32"])               # a few ulp of a value below 1
        L = 0 if r["call"]["rirs"] is None else int(np.count_nonzero(r["call"]["rirs"][0]))
        # the running fp32 sum of the direct form: no further off than the blocked one under a handful of taps, and growing
        # with the tap count under a dense RIR (the reason it is a yardstick of its own)
        assert r["e_seq"] <= (3.0 if L <= 8 else 40.0) * max(r["e32"], 2.0 ** -24), (r["id"], r["e_seq"], r["e32"])
    dense = [r["e_seq"] / r["e32"] for r in augment if r["id"].startswith("match-(2, 24000, 8192)")]
    assert min(dense) > 8.0, dense                                 # 8 x the blocked restatement cannot hold an honest running sum
    assert S.waveform_bound(0.0, False) == S.WAVE_FLOOR and S.waveform_bound(1.0, True) == S.WAVE_CEILING
    f32, _ = S.aug_oracle(augment[0]["call"], dtype=np.float32)
    assert f32.dtype == np.float32


@pytest.mark.parametrize("defect", list(OA.DEFECTS))
def test_every_augmentation_defect_misses_the_bound_in_both_forms(augment, defect):
    for fft in (False, True):
        worst = max(((r["err"][defect] / r["bound"][fft], r["id"]) for r in augment if fft in r["forms"]))
        print(f"{defect}, {'fft' if fft else 'direct'} form: err / bound up to {worst[0]:.3g} ({worst[1]})")
        assert worst[0] >= 2.0, (defect, fft, worst)


def test_two_tap_closed_form_is_the_oracle(augment):
    n = 0
    for r in augment:
        if r["id"].startswith("two-tap"):
            L = r["call"]["rirs"].shape[1]
            assert (r["ch"]["rir"] == 0).all() and (r["ch"]["noise"] == -1).all()
            assert np.array_equal(r["ref"], S.two_tap_closed_form(r["call"]["x"], L)), r["id"]
            n += 1
    assert n == len(S.TWO_TAP_N) * len(S.TWO_TAP_L)
    # none of the lengths is a multiple of the direct form's tile or of an overlap-save step; 1, 2 and 3+ segments occur
    for N in S.TWO_TAP_N:
        assert N % 2048
        for L in S.TWO_TAP_L:
            assert N % (16384 - L + 1)
    segs = {-(-N // (16384 - L + 1)) for N in S.TWO_TAP_N for L in S.TWO_TAP_L}
    assert {1, 2, 3} <= segs and max(segs) > 3 and 3001 % 8


def test_planted_noise_bank_shows_a_window_one_sample_off(augment):
    r = next(r for r in augment if r["id"] == "mix-alone")
    c, ch = r["call"], r["ch"]
    N, Nn = c["x"].shape[1], c["noises"].shape[1]
    assert (ch["noise"] >= 0).all() and (ch["rir"] == -1).all()
    assert ((ch["offset"] >= 1).any() and (ch["offset"] + N < Nn).any())           # both plants exist somewhere
    assert r["e32"] < 2e-7
    for d in ("noise_rms_shift_plus", "noise_rms_shift_minus"):
        assert r["err"][d] > 1e-2, (d, r["err"][d])


def test_saturation_case_clips_a_fifth_of_the_samples(augment):
    r = next(r for r in augment if r["id"] == "saturation")
    share = float(np.mean(np.abs(r["ref"]) == 1.0))
    assert 0.1 <= share <= 0.5, share
    assert r["err"]["clip_before_noise"] > 1e-2
    assert (r["ch"]["rir"] >= 0).all() and (r["ch"]["noise"] >= 0).all()


def test_wide_philox_words_reach_the_high_halves():
    c = S.wide_philox_call()
    B, N = c["x"].shape
    args = (B, N, 3, 2, c["noises"].shape[1], 0.6, 0.6, 5.0, 20.0)
    wide = OA.audio_choices(*args, seed=c["seed"], step=c["step"], sample_offset=c["sample_offset"])
    for low in (dict(seed=c["seed"] & 0xFFFFFFFF, step=c["step"], sample_offset=c["sample_offset"]),
                dict(seed=c["seed"], step=c["step"] & 0xFFFFFFFF, sample_offset=c["sample_offset"])):
        assert not np.array_equal(OA.audio_choices(*args, **low)["offset"], wide["offset"])
    assert (wide["rir"] >= 0).any() and (wide["rir"] < 0).any() and (wide["noise"] >= 0).any()
