"""Host: the detection law restated in evaluation/detection.py, against sequences worked out by hand and against the
window-by-window walk of tests/detection_cases.py; event_windows; the new names of the C ABI."""
import ctypes
import re

import numpy as np
import pytest

from tests.conftest import REPO
from tests.detection_cases import (F32, F64, NAN, RISING, TWELVE, TWELVE_EVENTS, TWELVE_EXPECT, bits, detector_cases,
                                   detector_confidences, detector_events, roc_thresholds, table, walk, walk_smooth)
from wakeword_trainer_home_amd.evaluation import (detect_counts, event_windows, match_triggers, num_windows, num_windows_hop,
                                                  rates, smooth, trigger_windows, window_starts_hop)

NEW_NAMES = {"ww_wave_num_windows_hop", "ww_wave_windows_at", "ww_feat_windows", "ww_detect_accumulate"}


@pytest.mark.parametrize("R", [1, 3])
def test_twelve_windows_by_hand(R):
    exp = TWELVE_EXPECT[R]
    assert trigger_windows(TWELVE, 0.5, R).tolist() == exp["triggers"]
    assert match_triggers(exp["triggers"], TWELVE_EVENTS).tolist() == exp["counts"]
    assert detect_counts(TWELVE, 1, R, [0.5], TWELVE_EVENTS).tolist() == [exp["counts"]]
    s, trig, counts = walk(TWELVE, 1, R, 0.5, TWELVE_EVENTS)
    assert trig == exp["triggers"] and counts == exp["counts"] and np.array_equal(s, TWELVE)
    assert counts[0] == counts[1] + counts[2] + counts[3]


def test_false_alarms_can_rise_with_the_threshold():
    c = detect_counts(RISING["conf"], 1, RISING["R"], RISING["thresholds"], RISING["events"])
    assert c.tolist() == RISING["counts"]
    assert c[1, 2] > c[0, 2]                                   # more false alarms at the HIGHER threshold
    fa, miss = rates(c, n_events=1, hours=0.5)
    assert fa.tolist() == [0.0, 2.0] and miss.tolist() == [0.0, 1.0]
    assert rates(c, 0, 0.0)[0].tolist() == [0.0, 0.0] and rates(c, 0, 0.0)[1].tolist() == [0.0, 0.0]


def test_a_tie_triggers_only_where_the_float32_value_reaches_the_float64_threshold():
    thr = roc_thresholds()
    down = np.flatnonzero(thr.astype(F32).astype(F64) < thr)
    up = np.flatnonzero(thr.astype(F32).astype(F64) > thr)
    assert down.size and up.size
    for k, fires in ((down[3], False), (up[3], True)):
        conf = np.array([0.0, thr[k], 0.0], F32)               # conf == float32(threshold)
        assert trigger_windows(conf, thr[k], 1).tolist() == ([1] if fires else [])
        assert walk(conf, 1, 1, thr[k], [])[1] == ([1] if fires else [])
    assert trigger_windows(np.array([0.5], F32), 0.5, 1).tolist() == [0]       # an exact tie


def test_a_nan_confidence_never_triggers_and_spreads_over_m_windows():
    conf = np.array([0.9, NAN, 0.9, 0.9, 0.9, 0.9], F32)
    assert trigger_windows(conf, 0.0, 1).tolist() == [0, 2, 3, 4, 5]
    s = smooth(conf, 3)
    assert np.isnan(s).tolist() == [False, True, True, True, False, False]
    assert np.array_equal(bits(s[4:]), bits(np.array([0.9, 0.9], F32)))
    assert trigger_windows(s, 0.0, 1).tolist() == [0, 4, 5]
    assert detect_counts(conf, 3, 1, [0.0, 0.95], [(1, 4)]).tolist() == [[3, 1, 2, 0], [0, 0, 0, 0]]


def test_smoothing_over_fewer_than_m_windows_and_in_float64():
    assert smooth(np.array([1.0, 0.0, 0.5], F32), 5).tolist() == [1.0, 0.5, 0.5]       # M larger than w + 1: count = w + 1
    big = np.array([16777216.0, 1.0, 1.0], F32)               # a float32 running sum would lose both ones
    assert smooth(big, 3)[2] == F32(16777218.0 / 3.0) != F32((F32(16777216.0) + F32(1.0) + F32(1.0)) / F32(3.0))
    rng = np.random.default_rng(3)
    conf = rng.random(200).astype(F32)
    conf[[17, 150]] = np.nan
    for M in (1, 2, 3, 64):
        assert np.array_equal(bits(smooth(conf, M)), bits(walk_smooth(conf, M)))
    assert smooth(np.zeros(0, F32), 4).shape == (0,)
    with pytest.raises(ValueError):
        smooth(conf, 65)


def test_the_restatement_equals_the_window_by_window_walk():
    """The vectorised restatement the GPU tests use against the literal walk, on the GPU tests' own small inputs."""
    rng = np.random.default_rng(11)
    for W, K, M, R, E in [c for c in detector_cases(1024) if c[0] <= 300 and c[1] <= 100]:
        thr = table(K)
        conf, ev = detector_confidences(W, thr, rng), detector_events(W, E)
        got = detect_counts(conf, M, R, thr, ev)
        assert got.shape == (K, 4)
        for k in range(0, K, 7):
            assert got[k].tolist() == walk(conf, M, R, thr[k], ev.tolist())[2], (W, K, M, R, E, k)


def test_num_windows_hop_at_half_overlap_is_the_reference_rule():
    for chunk in (2, 3, 96, 251):
        for S in range(0, 4 * chunk + 3):
            assert num_windows_hop(S, chunk, max(1, chunk // 2)) == num_windows(S, chunk), (S, chunk)
    assert num_windows_hop(1000, 96, 7) == 130 and window_starts_hop(1000, 96, 7)[-1] == 903
    assert num_windows_hop(95, 96, 1) == 0 and num_windows_hop(96, 96, 96) == 1
    for hop in (0, 97):
        with pytest.raises(ValueError):
            num_windows_hop(1000, 96, hop)


def test_event_windows():
    sr, chunk, hop = 100, 50, 10                               # window w ends at (10 w + 50) / 100 s; 1000 samples: 96 windows
    S = 1000
    ew = lambda ev, tol=0.0: event_windows(ev, S, sr, chunk, hop, tol)
    iv, n = ew([(1.0, 2.0)])                                   # ends in [1.0, 2.0]: w = 5 .. 15
    assert iv.tolist() == [[5, 15]] and n == 1 and iv.dtype == np.int32
    assert ew([(1.0, 2.0)], 0.5)[0].tolist() == [[5, 20]]      # the tolerance extends the end only
    assert ew([(1.01, 1.09)])[0].tolist() == [] and ew([(1.01, 1.09)])[1] == 1     # no window ends inside: empty, still counted
    # clipping at both ends: the first window ends at 0.5 s, the last (95) at 10.0 s
    assert ew([(0.0, 0.7)])[0].tolist() == [[0, 2]]
    assert ew([(9.8, 12.0)], 3.0)[0].tolist() == [[93, 95]]
    assert ew([(0.0, 0.3)]) [0].tolist() == [] and ew([(10.5, 11.0)])[0].tolist() == []
    # sorted by start; an overlapping range is cut where the next one begins
    iv, n = ew([(3.0, 3.2), (1.0, 2.0)], 1.5)
    assert iv.tolist() == [[5, 24], [25, 42]] and n == 2
    # two events with the same first window: the earlier one is left empty and is a certain miss
    iv, n = ew([(1.0, 1.0), (1.0, 1.5)])
    assert iv.tolist() == [[5, 10]] and n == 2
    assert ew(None) [0].shape == (0, 2) and ew(None)[1] == 0
    assert event_windows([(0.1, 0.2)], 40, sr, chunk, hop, 1.0)[0].shape == (0, 2)           # a recording without windows
    for bad in ([(2.0, 1.0)], [(NAN, 1.0)], [(1.0, NAN)]):
        with pytest.raises(ValueError):
            ew(bad)
    # the intervals satisfy the kernel's precondition and feed the matcher
    iv, _ = ew([(0.0, 0.7), (0.6, 2.0), (2.0, 2.0), (5.0, 5.5)], 0.3)
    assert (iv[:, 0] <= iv[:, 1]).all() and (iv[1:, 0] > iv[:-1, 1]).all()
    assert match_triggers([0, 2, 3, 30, 95], iv).tolist()[0] == 5


def test_header_exports_and_library_agree_on_the_new_names():
    from wakeword_trainer_home_amd import _native
    header = (REPO / "include" / "wwhip.h").read_text()
    declared = set(re.findall(r"\b(ww_[a-z0-9_]+)\s*\(", header))
    assert NEW_NAMES <= declared and NEW_NAMES <= set(_native.EXPORTS)
    lib = ctypes.CDLL(str(_native.lib_path()))
    assert all(hasattr(lib, n) for n in NEW_NAMES)
    assert _native.load().ww_abi_version() == _native.ABI_VERSION == 17
    assert re.search(r"#define WW_ABI_VERSION 17\b", header)
    assert int(re.search(r"#define WW_DETECT_TILE (\d+)", header).group(1)) == _native.DETECT_TILE
    assert int(re.search(r"#define WW_WAVE_SPLIT_CHUNK (\d+)", header).group(1)) == _native.WAVE_SPLIT_CHUNK
    assert int(re.search(r"#define WW_DETECT_MAX_SMOOTH (\d+)", header).group(1)) == _native.DETECT_MAX_SMOOTH
    # the host-only window count follows the restated rule
    for S, chunk, hop in [(1000, 96, 7), (95, 96, 1), (96, 96, 96), (24000 * 40, 24000, 1600), (5, 2, 1)]:
        assert _native.wave_num_windows_hop(S, chunk, hop) == num_windows_hop(S, chunk, hop)
