"""CPU: the claims tests/test_grid_passes_gpu.py rests on.  That a case makes a second pass is asked of the library's own plan
queries (ww_pass_plan / ww_loader_plan, the functions the launch sites take their grids from), so a change of a cap turns these
assertions red instead of silently turning the GPU tests back into one-pass tests; the rest checks what the references need."""
import re
from pathlib import Path

import numpy as np

from tests import data_pipeline_cases as D
from tests import grid_pass_cases as K
from tests.evaluation_cases import host_windows

REPO = Path(__file__).resolve().parent.parent


def test_every_case_is_past_one_pass_and_ends_ragged():
    from wakeword_trainer_home_amd import _native as nat
    for name, (launch, n, whole) in K.pass_cases().items():
        p = nat.plan_passes(launch, n)
        print(f"{name}: {launch} n={n} grid={p['grid']} one pass={p['per_pass']} passes={p['passes']} last={n - (p['passes'] - 1) * p['per_pass']}")
        assert p["passes"] >= 2 and n > p["per_pass"], name
        assert p["passes"] == -(-n // p["per_pass"])
        if whole:                       # (2, 4096, 1024): both counter fields at their limits -- exactly two full passes
            assert n == 2 * p["per_pass"], name
        else:
            assert n % p["per_pass"] != 0, name
    # the figures the cases were chosen by
    assert nat.plan_passes("ew", K.EW_N) == {"grid": 4096, "per_pass": 1 << 20, "passes": 2}
    assert nat.plan_passes("to16_pair", 4_284_416) == {"grid": 4096, "per_pass": 1 << 22, "passes": 2}
    assert nat.plan_passes("wave_windows", K.WINDOW_W) == {"grid": 4096, "per_pass": 4096, "passes": 2}
    assert nat.plan_passes("ew", 4 * 260 * 260 * 16)["passes"] == 5 and nat.plan_passes("dropout_bt", 1_056_000)["passes"] == 2
    # the second trip of k_to16_pair starts at row 65 536 of x = sample 1024, and takes all of W_ih
    Bp, Tp, Ip = K.PROJ_SHAPE
    first = nat.plan_passes("to16_pair", 4_284_416)["per_pass"] // (Ip // 4)
    assert first == 65536 and first // Tp == 1024 and Bp * Tp - first == 1024 and K.PROJ_SAMPLES == (0, 1023, 1024, Bp - 1)
    # the tiny cases and everything the older tests run stay inside one pass
    for launch, n in (("ew", 1), ("ew", 5), ("ew", 25728 // 4), ("ew", 2 * 10 * 9 * 16), ("dropout_bt", 3 * 7 * 2), ("wave_windows", 5),
                      ("to16_pair", (70 * 20 * 256 + 384 * 256) // 4)):
        assert nat.plan_passes(launch, n)["passes"] == 1, (launch, n)
    assert nat.plan_passes("ew", 1) == {"grid": 1, "per_pass": 256, "passes": 1}
    assert nat.plan_passes("to16_pair", 1025) == {"grid": 2, "per_pass": 2048, "passes": 1}


def test_plan_queries_refuse_bad_arguments():
    import ctypes
    import pytest
    from wakeword_trainer_home_amd import _native as nat
    lib = nat.load()
    out = (ctypes.c_long * 2)()
    assert lib.ww_pass_plan(len(nat.PASS_LAUNCHES), 5, out) == -1 and b"unknown launch" in lib.ww_last_error()
    assert lib.ww_pass_plan(-1, 5, out) == -1 and lib.ww_pass_plan(0, 0, out) == -1 and lib.ww_pass_plan(0, 5, None) == -1
    assert lib.ww_loader_plan(0, 8, (ctypes.c_int * 2)()) == -1 and lib.ww_loader_plan(8, 0, (ctypes.c_int * 2)()) == -1
    with pytest.raises(ValueError):
        nat.plan_passes("nothing", 5)


def test_loader_cases_make_unequal_and_three_trips():
    from wakeword_trainer_home_amd import _native as nat
    n_out = K.LOADER["n_out"]
    assert n_out % 2 == 1 and n_out // 8 == 3 * 256
    for B, _ in K.LOADER_RUNS:
        p = nat.plan_loader(B, n_out)
        print(f"loader B={B} n_out={n_out}: S={p['S']} passes={p['passes']} trips={p['trips']}")
        assert p["passes"] == 3 and p["trips"] == K.LOADER_TRIPS[B] and max(p["trips"]) >= 2
    assert nat.plan_loader(1100, n_out)["S"] == 2 and nat.plan_loader(2048, n_out)["S"] == 1
    # the shapes the presets use, for the record: 128 x 40 000 -> 16 of 20 (2 trips), 512 x 24 000 -> 4 of 12 (3 trips)
    assert (nat.plan_loader(128, 40000)["S"], nat.plan_loader(128, 40000)["passes"]) == (16, 20)
    assert nat.plan_loader(512, 24000)["trips"] == (3, 3, 3, 3)
    # every case of test_data_pipeline_gpu.py is one trip per thread
    for B, n in ((24, 8), (24, 250), (24, 4001), (24, 24000), (5, 24000), (9, 24000), (64, 24000), (9, 250)):
        assert set(nat.plan_loader(B, n)["trips"]) <= {0, 1}, (B, n)


def test_loader_case_draws_odd_and_even_crop_offsets_from_every_clip_length():
    c = K.LOADER
    lengths = np.array([0, 1, c["n_out"] - 1, c["n_out"], c["n_out"] + 1, c["L"]] * 4)      # _bank_case's lengths
    cdf = D.cdf_table(D.zero_run_weights(c["n_clips"], seed=3))
    for epoch in c["epochs"]:
        idx = D.indices(c["n_clips"], "weighted", c["seed"], epoch, c["rank"], c["world"], c["k0"], 2048, cdf=cdf)
        off = D.crop_offsets(D.positions(c["rank"], c["world"], c["k0"], 2048), lengths[idx], c["n_out"], c["seed"], epoch, True)
        odd, even = int((off % 2 == 1).sum()), int(((off > 0) & (off % 2 == 0)).sum())
        print(f"loader epoch {epoch}: {odd} odd and {even} even non-zero crop offsets, {len(set(idx))} clips, lengths {sorted(set(lengths[idx]))}")
        assert odd > 0 and even > 0 and off.max() <= c["L"] - c["n_out"]
        assert set(lengths[idx]) == set(lengths)                  # empty, short, exact and long clips are all drawn
        assert (off[:1100] % 2 == 1).any() and ((off[:1100] > 0) & (off[:1100] % 2 == 0)).any()


def test_integer_cases_stay_exact_in_float32():
    B, T, Cin, Cout, k, d = K.DPRE_SHAPE
    dpre, x, w = 4 * K.DPRE_SCALE, 4, 2                              # largest |dy| * scale, |x|, |w| of tcn_cases.layer_inputs
    assert B * T == 16400 and dpre * x == 32
    for bound in (B * T * dpre * x, Cout * k * dpre * w, B * T * dpre):        # dw, dx, db
        assert bound < 2 ** 24
    assert dpre <= 256 and x <= 256                                  # bf16 holds the operands exactly
    assert 4 * 4 < 2 ** 24 and 2 < 2 ** 24                           # max-pool: values in [0, 2], at most four gradients of |4| meet
    assert (B * T * Cout // 4 - (1 << 20)) == 16 * (Cout // 4)      # 16 rows into the second pass


def test_window_recordings_hold_what_they_claim():
    for chunk, order in zip(K.WINDOW_CHUNKS, ("zero_tiny", "tiny_zero")):
        wave = K.window_recording(chunk, order)
        with np.errstate(invalid="ignore"):
            out, peaks = host_windows(wave, chunk)
        assert len(peaks) == K.WINDOW_W and (len(wave) - chunk) % (chunk // 2) == 7
        zero, tiny = (4096, 4097) if order == "zero_tiny" else (4097, 4096)
        assert peaks[zero] == 0 and not out[zero].any()
        assert peaks[tiny] == K.F32(1e-30) and np.abs(out[tiny]).max() == 1.0
        assert np.isnan(peaks[4098]) and not np.isnan(peaks[:4098]).any()
        assert np.isfinite(out[:4098]).all() and (np.abs(out[:4096]).max(axis=1) == 1.0).all() and (peaks[4093:4096] > 1e-4).all()
        # first trip against second trip of workgroups 0, 1: one peak grows, one shrinks; neither repeats
        first, second = peaks[:2], peaks[4096:4098]
        assert (first > 0).all() and (first != second).all() and (second > first).any() and (second < first).any()
        assert 0 < peaks[2] < 1e-30


def test_ew_inputs_plant_every_special_in_both_passes():
    a, b = K.ew_inputs(K.EW_N)
    npair = len(K.SPECIALS) ** 2
    for at in (0, 1 << 20, K.EW_N - npair):
        assert at + npair <= K.EW_N and (at == 0 and npair <= 256 or at >= 1 << 20)
        seg_a, seg_b = a[at:at + npair], b[at:at + npair]
        assert K.same_floats(seg_a, np.repeat(K.SPECIALS, len(K.SPECIALS))) and K.same_floats(seg_b, np.tile(K.SPECIALS, len(K.SPECIALS)))
        ref = K.add_relu_ref(seg_a, seg_b)
        # -0 survives (-0 + -0), negative sums and -inf become +0, NaN and +inf stay, a positive subnormal stays, a negative one goes
        assert np.signbit(ref[(seg_a == 0) & np.signbit(seg_a) & (seg_b == 0) & np.signbit(seg_b)]).all()
        assert np.isnan(ref).sum() >= 17 and np.isinf(ref).any() and not (ref < 0).any()
        assert (ref == K.F32(1e-40)).any() and K.F32(1e-40) > 0 and K.F32(1e-40) < np.finfo(K.F32).tiny
        m = K.relu_mask_ref(seg_a, seg_b)                         # (dy, y)
        assert not m[seg_b == 0].any() and not np.signbit(m[seg_b == 0]).any()
        assert K.same_floats(m[np.isnan(seg_b)], seg_a[np.isnan(seg_b)])
    assert K.same_floats(np.array([np.nan, 1.0, -0.0]), np.array([np.nan, 1.0, -0.0]))
    assert not K.same_floats(np.array([0.0]), np.array([-0.0])) and not K.same_floats(np.array([1.0]), np.array([np.nan]))


def test_dropout_masks_keep_at_the_rate_and_reach_the_field_limits():
    for name, case in (("big", K.DROP_BIG), ("ragged", K.DROP_RAGGED), ("p999", K.DROP_SMALL["p999"])):
        keep = K.dropout_keep_cached(name, case)
        q = 1.0 - K.dropout_p32(case["p"])
        sigma = (q * (1 - q) / keep.size) ** 0.5
        print(f"dropout {name} {case['shape']}: keep rate {keep.mean():.6f}, 1 - p = {q:.6f}, 4 sigma = {4 * sigma:.6f}")
        assert abs(keep.mean() - q) <= 4 * sigma, name
        x = K.dropout_case_x(case["shape"])
        for planted in (np.signbit(x) & (x == 0), np.isnan(x)):
            assert (planted & ~keep).any() and (name == "p999" or (planted & keep).any()), name
    B, T, C = K.DROP_BIG["shape"]
    assert T - 1 == 2 ** 12 - 1 and (C - 1) >> 2 == 2 ** 8 - 1 and K.DROP_BIG["stream_id"] == 2 ** 4 - 1
    B, T, C = K.DROP_RAGGED["shape"]
    assert C % 4 != 0 and B * T * ((C + 3) // 4) == 1_056_000
    # the low word of sample_offset + b wraps inside the batch, and the mask law keeps only that word
    wrap = K.DROP_SMALL["offset_wraps"]
    assert wrap["sample_offset"] < 2 ** 32 <= wrap["sample_offset"] + wrap["shape"][0] - 1
    low = dict(wrap, shape=(3,) + wrap["shape"][1:], sample_offset=0)
    assert np.array_equal(K.dropout_keep(wrap)[3:], K.dropout_keep(low))
    assert np.array_equal(K.dropout_keep(K.DROP_SMALL["offset_2_40"]), K.dropout_keep(dict(wrap, sample_offset=5)))
    assert K.dropout_keep(K.DROP_SMALL["p0"]).all()
    # the reference multiplies once, in float32
    ref = K.dropout_ref(np.array([1.0, -0.0, np.nan, 3.0], dtype=K.F32), np.array([True, True, True, False]), 0.3)
    assert ref[0] == K.F32(1.0 / (1.0 - float(K.F32(0.3)))) and np.signbit(ref[1]) and np.isnan(ref[2]) and ref[3] == 0 and not np.signbit(ref[3])


def test_header_declares_the_plan_queries_under_abi_17():
    from wakeword_trainer_home_amd import _native as nat
    header = (REPO / "include" / "wwhip.h").read_text()
    assert nat.ABI_VERSION == 17 and re.search(r"#define WW_ABI_VERSION 17\b", header) and nat.load().ww_abi_version() == 17
    assert re.search(r"\bint ww_pass_plan\(int launch, long n, long \*out\);", header)
    assert re.search(r"\bint ww_loader_plan\(int B, int n_out, int \*out\);", header)
    for i, name in enumerate(nat.PASS_LAUNCHES):
        assert re.search(rf"#define WW_PASS_{name.upper()} {i}\b", header), name
    assert "ww_pass_plan" in nat.EXPORTS and "ww_loader_plan" in nat.EXPORTS
    # the launch sites take their grids from the functions the queries report (csrc/ww_internal.h)
    csrc = REPO / "wakeword_trainer_home_amd" / "csrc"
    for file, call in (("ww_tap_gemm.h", "ww_pass_ew(n).grid"), ("ww_gru.hip", "ww_pass_dropout_bt("), ("ww_eval.hip", "ww_pass_wave_windows(W).grid"),
                       ("ww_rnn.h", "ww_pass_to16_pair(n4).grid"), ("ww_data.hip", "ww_loader_plan_rows(B, n_out).S")):
        assert call in (csrc / file).read_text(), (file, call)
