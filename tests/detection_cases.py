"""Shared by test_detection_host.py and test_detection_gpu.py: the detection law written out once more, window by window
(``walk``: nothing vectorised, nothing shared with ``evaluation/detection.py``), the hand-worked sequences, and the seeded
inputs of the GPU tests."""
import numpy as np

F32, F64 = np.float32, np.float64
NAN = float("nan")


def roc_thresholds():
    return np.linspace(0, 1, 100)


# ------------------------------------------------------------------------------------------------ the law, literally
def walk_smooth(conf, M):
    conf = np.asarray(conf, F32)
    out = np.zeros(conf.size, F32)
    for w in range(conf.size):
        acc = F64(0.0)
        terms = range(max(0, w - M + 1), w + 1)
        for j in terms:
            acc = acc + F64(conf[j])
        out[w] = F32(acc / F64(len(terms)))
    return out


def walk(conf, M, R, t, events):
    """-> (smoothed, trigger windows, [triggers, hits, false alarms, duplicates]) of ONE threshold."""
    s = walk_smooth(conf, M)
    next_ok, trig, hit, counts = 0, [], set(), [0, 0, 0, 0]
    for w in range(s.size):
        if w >= next_ok and F64(s[w]) >= F64(t):
            trig.append(w)
            next_ok = w + R
            counts[0] += 1
            inside = [e for e, (a, b) in enumerate(events) if a <= w <= b]
            if not inside:
                counts[2] += 1
            elif inside[0] in hit:
                counts[3] += 1
            else:
                hit.add(inside[0])
                counts[1] += 1
    return s, trig, counts


# ------------------------------------------------------------------------------------------------ hand-worked sequences
# twelve windows, threshold 0.5, no smoothing.  At or above 0.5: windows 1 2 4 5 7 8 10 11 (window 7 is a tie).
TWELVE = np.array([0.1, 0.6, 0.7, 0.2, 0.9, 0.8, 0.1, 0.5, 0.6, 0.3, 0.7, 0.9], F32)
TWELVE_EVENTS = [(1, 2), (5, 6), (10, 11)]
TWELVE_EXPECT = {
    # R = 1: every such window triggers.  1 hit, 2 duplicate (event 0); 4 false; 5 hit (event 1); 7, 8 false; 10 hit, 11
    # duplicate (event 2)
    1: dict(triggers=[1, 2, 4, 5, 7, 8, 10, 11], counts=[8, 3, 3, 2]),
    # R = 3: 1 triggers (hit, event 0) and blocks 2, 3; 4 triggers (false) and blocks 5, 6 -- event 1 is missed; 7 triggers
    # (false, the tie) and blocks 8, 9; 10 triggers (hit, event 2) and blocks 11
    3: dict(triggers=[1, 4, 7, 10], counts=[4, 2, 2, 0]),
}

# false alarms RISE with the threshold: at 0.5 window 0 triggers (a hit) and its refractory period swallows window 2; at 0.8
# window 0 stays silent and window 2 triggers outside the event
RISING = dict(conf=np.array([0.6, 0.1, 0.9, 0.1, 0.1, 0.1], F32), R=3, events=[(0, 0)], thresholds=[0.5, 0.8],
              counts=[[1, 1, 0, 0], [1, 0, 1, 0]])


# ------------------------------------------------------------------------------------------------ GPU detector inputs
def table(K):
    return {1: np.array([0.5]), 100: roc_thresholds(), 1024: np.linspace(0, 1, 1024)}[K]


def detector_confidences(W, thr, rng):
    """Drawn from a small set: exact table entries rounded to float32 (ties, some of which round below the entry), their
    neighbours, plain values, and now and then a NaN."""
    picks = thr[rng.integers(0, thr.size, 6)].astype(F32)
    pool = np.concatenate([picks, np.nextafter(picks[:2], F32(2)), np.array([0.0, 0.25, 0.5, 0.75, 1.0, 0.05], F32)])
    conf = pool[rng.integers(0, pool.size, W)]
    conf[rng.random(W) < 0.01] = np.nan
    return conf.astype(F32)


def detector_events(W, E):
    """E intervals (fewer when W cannot hold them): one at window 0, one ending at W - 1, two adjacent."""
    if W == 0 or E == 0:
        return np.zeros((0, 2), np.int32)
    if E == 1:
        return np.array([[0, min(2, W - 1)]] if W % 2 else [[max(0, W - 3), W - 1]], np.int32)
    if W < 20:
        return np.array([[w, w] for w in range(min(E, W))], np.int32)
    return np.array([[0, 3], [4, 9], [W // 3, W // 3 + W // 15], [2 * W // 3, 2 * W // 3], [W - 10, W - 1]], np.int32)


def detector_cases(tile):
    """(W, K, M, R, E): every W meets every K x M pair, and every R and E choice, on a 3 x 3 Latin square."""
    cases = []
    for W in (0, 1, 2, 300, tile - 1, tile, tile + 1):
        for i, K in enumerate((1, 100, 1024)):
            for j, M in enumerate((1, 3, 64)):
                cases.append((W, K, M, (1, 4, W + 1)[(i + j) % 3], (0, 1, 5)[(i + 2 * j) % 3]))
    return cases


# ------------------------------------------------------------------------------------------------ cutter inputs
CUT_S, CUT_CHUNK, CUT_HOPS = 1000, 96, (1, 7, 48, 96)


def cutter_wave():
    """1000 samples of mixed scale; samples [192, 300) are zero -- a whole window at every hop of CUT_HOPS starts at 192 or
    196 -- and sample 700 is a NaN."""
    rng = np.random.default_rng(96)
    wave = (rng.normal(0, 0.2, CUT_S) * rng.choice([1e-3, 0.05, 1.0, 30.0], CUT_S)).astype(F32)
    wave[192:300] = 0.0
    wave[700] = np.nan
    return wave


def host_windows_at(wave, chunk, hop, w0, n, normalize):
    out, peaks = np.zeros((n, chunk), F32), np.zeros(n, F32)
    with np.errstate(invalid="ignore"):
        for i in range(n):
            piece = wave[(w0 + i) * hop:(w0 + i) * hop + chunk]
            assert piece.size == chunk
            peak = np.max(np.abs(piece))
            peaks[i] = peak
            out[i] = piece / peak if (normalize and peak > 0) else piece
    return out, peaks


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)
