"""Time-stretch / pitch-shift (DESIGN.md "Time-stretch / pitch-shift spec"): the restatement of the law in numpy, the cases
the GPU tests feed the device (tests/test_tsm_gpu.py) and the bounds they hold it to; tests/test_tsm_host.py shows on the CPU
that the law means what it says and that the bounds discriminate.

The law is time-domain WSOLA followed by a windowed-sinc resampler.  Constants: LW = 512 (grain), HS = 256 (synthesis
hop), DELTA = 128 (search radius), ZC = 8 (sinc zero crossings per side).  Window: periodic Hann w[i] = 0.5 - 0.5 cos(2 pi i /
512), so w[i] + w[i+256] = 1.  x[k] = 0 for k < 0 or k >= N, and z[k] = 0 for k < 0.

Draws.  Per clip b (g = sample_offset + b) one Philox4x32-10 draw, ctr = (step_lo, step_hi, g, TAG_AUDIO<<24 | 2), key = seed:
  stretch = r0 < floor(float32(time_stretch_prob) * 2**32);  u = float32(r1 >> 8) * 2**-24
  rate    = fma(u, rmax - rmin, rmin) in float32, or 1.0f without stretch
  pitch   = r2 < floor(float32(pitch_shift_prob) * 2**32);   semis = pmin + r3 mod (pmax - pmin + 1), or 0 without pitch shift
A clip with neither effect (no stretch and semis == 0) is a bit-exact copy.

Fixed point (host, double):  f_q = llround(exp2(semis / 12) * 2**20);  rho_q = llround(rate / (f_q * 2**-20) * 65536);
  half = ZC if f_q <= 2**20 else (ZC f_q + 2**20 - 1) >> 20;  Z = (((N-1) f_q) >> 20) + half + 2;  G = (Z - 1) // HS.

WSOLA -> z[0 .. Z).  Grain m sits at output m HS and copies x[p_m .. p_m + LW).  p_{-1} = -HS, p_0 = 0.  For m = 1 .. G:
  a_m = (m HS rho_q) >> 16;  tau[i] = x[p_{m-1} + HS + i];  c(d) = sum_{i<LW} x[a_m + d + i] tau[i], d in [-DELTA, DELTA];
  d_m = argmax c (ties: the smallest d);  p_m = a_m + d_m.     z[n] = sum_m w[n - m HS] x[p_m + n - m HS].

Resample.  c = 1 if f_q <= 2**20 else float32(2**20) / float32(f_q).  For n in [0, N): P = n f_q, k0 = P >> 20,
  fr = float32(P & (2**20 - 1)) * 2**-20;  out[n] = sum_{j = -half .. half+1} z[k0 + j] h(fr - j);
  h(u) = c sinc(c u) (0.5 + 0.5 cos(pi c u / ZC)) where |c u| < ZC, else 0;  sinc(v) = sin(pi v) / (pi v), 1 at 0.
The result is not clipped.

``tsm(..., dtype=np.float32)`` is the fp32 RESTATEMENT (synthesis and resampler in float32; the search stays float64, or
takes the offsets it is given): the yardstick of the waveform bound.  ``defect=`` plants exactly one mistake (DEFECTS).
"""
import math

import numpy as np

from oracle.philox import philox4x32_10, make_ctr, make_key, prob_threshold
from tests import input_stage as S

LW, HS, DELTA, ZC = 512, 256, 128, 8
ONE = 1 << 20
TAG_AUDIO = 2
U32 = 2.0 ** -24                       # unit round-off of float32

# name -> (what is wrong, how it shows).  "forced": the output against the law run with the offsets the defective code itself
# reports (what the teacher-forced GPU test sees); "free": against the law's own free-running output (a defect of the search
# changes the offsets, and with them which samples are copied; the GPU tests meet it in the search and free-running tests).
DEFECTS = {
    "template_late": ("template one sample late: tau[i] = x[p_{m-1} + HS + 1 + i]", "free"),
    "hann_symmetric": ("symmetric Hann, cos(2 pi i / 511), instead of the periodic one", "forced"),
    "last_tie": ("ties of the search go to the largest d", "free"),
    "first_hop_faded": ("no grain -1: the first hop is faded in", "forced"),
    "a_float": ("a_m = floor(float32(m HS) * float32(rate / f)) instead of the fixed point", "forced"),
    "no_cutoff": ("resampler without the cutoff: c = 1 at every pitch", "forced"),
}


# ----------------------------------------------------------------------------------------------------------- the law
def choices(B, stretch_prob, rmin, rmax, pitch_prob, pmin, pmax, seed=0, step=0, sample_offset=0):
    """-> dict of arrays: stretch (bool), rate (float32), pitch (bool), semis (int64)."""
    g = (np.arange(B, dtype=np.uint64) + np.uint64(sample_offset)) & np.uint64(0xFFFFFFFF)
    r = philox4x32_10(make_ctr(step, g, TAG_AUDIO, 2), make_key(seed)).astype(np.uint64)
    stretch = r[:, 0] < np.uint64(prob_threshold(stretch_prob))
    u = (r[:, 1] >> np.uint64(8)).astype(np.float32) * np.float32(U32)
    lo, hi = np.float32(rmin), np.float32(rmax)
    rate = (u.astype(np.float64) * float(hi - lo) + float(lo)).astype(np.float32)      # u (hi - lo) is exact in double
    rate = np.where(stretch, rate, np.float32(1.0)).astype(np.float32)
    pitch = r[:, 2] < np.uint64(prob_threshold(pitch_prob))
    semis = np.where(pitch, int(pmin) + (r[:, 3] % np.uint64(int(pmax) - int(pmin) + 1)).astype(np.int64), 0)
    return dict(stretch=stretch, rate=rate, pitch=pitch, semis=semis)


def _llround(v):
    return int(math.floor(v + 0.5))


def f_q_of(semis):
    return _llround(2.0 ** (int(semis) / 12.0) * 1048576.0)


def fixed_point(N, rate, semis):
    f_q = f_q_of(semis)
    rho_q = _llround(float(np.float32(rate)) / (f_q * 2.0 ** -20) * 65536.0)
    half = ZC if f_q <= ONE else (ZC * f_q + ONE - 1) >> 20
    Z = (((N - 1) * f_q) >> 20) + half + 2
    return dict(N=N, rate=float(np.float32(rate)), semis=int(semis), f_q=f_q, rho_q=rho_q, half=half, Z=Z, G=(Z - 1) // HS)


def max_grains(N, semis_max):
    """Columns of delta_out: the grains of the longest z of a call (a clip without pitch shift has semis = 0)."""
    return fixed_point(N, 1.0, max(int(semis_max), 0))["G"]


def _seg(x, start, n):
    """x[start : start + n] with zeros outside the clip."""
    out = np.zeros(n, x.dtype)
    lo, hi = max(start, 0), min(start + n, len(x))
    if hi > lo:
        out[lo - start:hi - start] = x[lo:hi]
    return out


def window(ft=np.float64, defect=None):
    i = np.arange(LW, dtype=np.float64)
    return (0.5 - 0.5 * np.cos(2.0 * np.pi * i / (LW - 1 if defect == "hann_symmetric" else LW))).astype(ft)


def grain_anchor(m, fx, defect=None):
    if defect == "a_float":
        return int(math.floor(float(np.float32(m * HS) * np.float32(fx["rate"] / (fx["f_q"] * 2.0 ** -20)))))
    return (m * HS * fx["rho_q"]) >> 16


def grain_scores(x64, p_prev, a, defect=None):
    """-> (c, S): the 2 DELTA + 1 correlations of a grain in float64 and the sums of |x_i tau_i| behind them."""
    tau = _seg(x64, p_prev + HS + (1 if defect == "template_late" else 0), LW)
    region = _seg(x64, a - DELTA, LW + 2 * DELTA)
    return np.correlate(region, tau, "valid"), np.correlate(np.abs(region), np.abs(tau), "valid")


def wsola(x, fx, forced=None, dtype=np.float64, defect=None, trace=None):
    """One clip -> (z (Z,) ``dtype``, d (G,) int).  ``forced``: offsets to use instead of searching.  ``trace`` (a list)
    receives (c, S) per grain."""
    ft = np.dtype(dtype).type
    x64 = np.asarray(x, np.float64)
    xs = np.asarray(x, ft)
    w = window(ft, defect)
    Z, G = fx["Z"], fx["G"]
    z = np.zeros(Z + LW, ft)
    d = np.zeros(G, np.int64)
    if defect != "first_hop_faded":
        z[:HS] += w[HS:] * _seg(xs, 0, HS)                   # grain -1 at p = -HS
    z[:LW] += w * _seg(xs, 0, LW)                            # grain 0 at p = 0
    p_prev = 0
    for m in range(1, G + 1):
        a = grain_anchor(m, fx, defect)
        if forced is None or trace is not None:
            c, s = grain_scores(x64, p_prev, a, defect)
            if trace is not None:
                trace.append((c, s))
        if forced is None:
            j = (len(c) - 1 - int(np.argmax(c[::-1]))) if defect == "last_tie" else int(np.argmax(c))
            d[m - 1] = j - DELTA
        else:
            d[m - 1] = int(forced[m - 1])
        p_prev = a + int(d[m - 1])
        z[m * HS:m * HS + LW] += w * _seg(xs, p_prev, LW)
    return z[:Z], d


def _sinpi(v, ft):
    k = np.rint(v)
    s = np.sin(ft(np.pi) * (v - k).astype(ft)).astype(ft)
    return np.where(k.astype(np.int64) & 1, -s, s).astype(ft)


def resample(z, fx, dtype=np.float64, defect=None):
    ft = np.dtype(dtype).type
    N, f_q, half = fx["N"], fx["f_q"], fx["half"]
    n = np.arange(N, dtype=np.int64)
    P = n * f_q
    k0 = P >> 20
    fr = ((P & (ONE - 1)).astype(np.float32) * np.float32(2.0 ** -20)).astype(ft)
    c = ft(1.0) if (f_q <= ONE or defect == "no_cutoff") else ft(np.float32(ONE) / np.float32(f_q))
    zp = np.concatenate([np.zeros(half, ft), np.asarray(z, ft)])
    out = np.zeros(N, ft)
    for j in range(-half, half + 2):
        v = (c * (fr - ft(j))).astype(ft)
        safe = np.where(v == 0, ft(1.0), v)
        sinc = np.where(v == 0, ft(1.0), _sinpi(v, ft) / (ft(np.pi) * safe)).astype(ft)
        h = (c * sinc * (ft(0.5) + ft(0.5) * np.cos(ft(np.pi) * v / ft(ZC)).astype(ft))).astype(ft)
        h = np.where(np.abs(v) < ZC, h, ft(0.0)).astype(ft)
        out = (out + zp[k0 + j + half] * h).astype(ft)
    return out


def tsm_clip(x, rate, semis, forced=None, dtype=np.float64, defect=None, trace=None):
    """One selected clip -> (out (N,), d (G,))."""
    fx = fixed_point(len(x), rate, semis)
    z, d = wsola(x, fx, forced, dtype, defect, trace)
    return resample(z, fx, dtype, defect), d


def tsm(x, stretch_prob, rmin, rmax, pitch_prob, pmin, pmax, seed=0, step=0, sample_offset=0, forced=None, dtype=np.float64,
        defect=None):
    """x (B,N) -> (out (B,N) ``dtype``, choices, deltas: per clip the offsets (None for a copied clip)).  ``forced``: a
    (B, max_grains) array whose row b holds the offsets clip b is to use."""
    ft = np.dtype(dtype).type
    x = np.asarray(x)
    B, N = x.shape
    ch = choices(B, stretch_prob, rmin, rmax, pitch_prob, pmin, pmax, seed, step, sample_offset)
    out, deltas = np.empty((B, N), ft), []
    for b in range(B):
        if not ch["stretch"][b] and ch["semis"][b] == 0:
            out[b] = x[b]
            deltas.append(None)
            continue
        o, d = tsm_clip(x[b], ch["rate"][b], ch["semis"][b], None if forced is None else forced[b], dtype, defect)
        out[b] = o
        deltas.append(d)
    return out, ch, deltas


# --------------------------------------------------------------------------------------------------- bounds and margins
def gamma(s_a, s_b):
    """The standard bound on the round-off of a 512-term fp32 dot product, in any order, is LW * 2**-24 * sum |x_i tau_i|;
    this is that bound for two of them together."""
    return LW * U32 * (float(s_a) + float(s_b))


def margin_ratio(c, s):
    """(best - second best) / (2 gamma) of one grain; inf where every product is an exact zero (nothing rounds)."""
    order = np.argsort(-c, kind="stable")
    g = gamma(s[order[0]], s[order[1]])
    return math.inf if g == 0.0 else float(c[order[0]] - c[order[1]]) / (2.0 * g)


def free_running_ok(x, rate, semis):
    """The free-running precondition of one clip: every grain's margin between its best and second-best c exceeds 2 gamma."""
    trace = []
    tsm_clip(x, rate, semis, trace=trace)
    return min((margin_ratio(c, s) for c, s in trace), default=math.inf)


def waveform_bound(e32):
    """max(8 e32, 16 * 2**-24), capped at 1e-4: the direct-form bound of tests/input_stage.py -- short fp32 dot products summed
    in another order.  ``e32``: the fp32 restatement against float64, same offsets."""
    return min(S.WAVE_CEILING, max(S.WAVE_HEADROOM[False] * float(e32), S.WAVE_FLOOR))


# ---------------------------------------------------------------------------------------------------------------- cases
SHAPES = [(3, 300), (4, 700), (3, 2048), (5, 5000), (2, 24000)]
FIXED = [(0.5, -12), (0.8, 2), (1.0, 0), (1.25, -3), (2.0, 12), (1.1, 0)]
# white-noise seeds per shape for which every clip of every fixed case passes the free-running precondition
# (test_tsm_host.py checks it); the harmonic clip is never asked to run free
NOISE_SEED = {(3, 300): 0, (4, 700): 0, (3, 2048): 0, (5, 5000): 0, (2, 24000): 0}


def noise_clips(B, N, seed=None):
    """White noise at 0.2 RMS."""
    rng = np.random.default_rng(NOISE_SEED[(B, N)] if seed is None else seed)
    return (0.2 * rng.standard_normal((B, N))).astype(np.float32)


def harmonic_clip(N):
    """150, 300 and 450 Hz at 16 kHz: the correlation repeats every 106.67 samples, near-ties are the rule."""
    t = np.arange(N) / 16000.0
    return (0.2 * (np.sin(2 * np.pi * 150 * t) + 0.5 * np.sin(2 * np.pi * 300 * t + 0.3)
                   + 0.25 * np.sin(2 * np.pi * 450 * t + 1.1))).astype(np.float32)


def fixed_call(B, N, rate, semis, seed=7, step=3, sample_offset=11):
    """Both probabilities 1 and rmin == rmax: the noise clips of the shape plus one harmonic clip (the last row)."""
    x = np.concatenate([noise_clips(B, N), harmonic_clip(N)[None]])
    return dict(x=x, stretch_prob=1.0, rmin=rate, rmax=rate, pitch_prob=1.0, pmin=semis, pmax=semis, seed=seed, step=step,
                sample_offset=sample_offset)


def call_args(c):
    return (c["stretch_prob"], c["rmin"], c["rmax"], c["pitch_prob"], c["pmin"], c["pmax"], c["seed"], c["step"],
            c["sample_offset"])


def mixed_call(B=64, N=700):
    rng = np.random.default_rng(23)
    x = (0.2 * rng.standard_normal((B, N))).astype(np.float32)
    return dict(x=x, stretch_prob=0.5, rmin=0.8, rmax=1.2, pitch_prob=0.5, pmin=-2, pmax=2, seed=5, step=9, sample_offset=40)


def wide_philox_call(B=6, N=700):
    """Seed, step and sample offset beyond 32 bits."""
    rng = np.random.default_rng(29)
    x = (0.2 * rng.standard_normal((B, N))).astype(np.float32)
    return dict(x=x, stretch_prob=0.6, rmin=0.5, rmax=2.0, pitch_prob=0.6, pmin=-12, pmax=12, seed=2 ** 40 + 17,
                step=2 ** 33 + 5, sample_offset=2 ** 32 + 1000)


def class_call(B=4, N=5000):
    """AudioAugmentation with both effects certain over the default ranges, RIR and noise after them; white-noise clips that
    pass the free-running precondition (test_tsm_host.py), so the device's offsets are the restatement's."""
    rng = np.random.default_rng(37)
    x = (0.2 * rng.standard_normal((B, N))).astype(np.float32)
    rirs, noises = S.banks(rng, R=3, L=400, K=2, Nn=N + 777)
    return dict(x=x, rirs=rirs, noises=noises, stretch_prob=1.0, rmin=0.8, rmax=1.2, pitch_prob=1.0, pmin=-2, pmax=2, seed=9,
                step=0, sample_offset=0)
