"""Waveform augmentation oracle: RIR convolution + background-noise mix (BASELINE config 4).

The reference's ``AudioAugmentation`` source is ABSENT; only its constructor
(``tests/test_training_pipeline.py:230-236``), its shape/finite contract (``:242-243``), the config knobs
(``src/config/defaults.py:81-87``: background_noise_prob, noise_snr_min/max, rir_prob) and the UI guidance
(``src/ui/panel_docs.py:111-122``) survive.  The law below is the BUILD'S OWN SPEC (DESIGN.md "Audio augmentation
spec") -- **parity unpinned** w.r.t. the reference.  Time-stretch / pitch-shift are outside the north_star list.

Per clip b (global sample index g = sample_offset + b), two Philox4x32-10 draws with ctr = (step_lo, step_hi, g,
TAG_AUDIO<<24 | i), key = seed:
  i = 0 (RIR):    apply = r0 < floor(float32(rir_prob) * 2**32);  rir = r1 mod R
  i = 1 (noise):  apply = r0 < floor(float32(noise_prob) * 2**32); noise = r1 mod K;  offset = r2 mod (Nn - N + 1);
                  u = float32(r3 >> 8) * 2**-24;  snr_db = fma(u, snr_max - snr_min, snr_min)          (float32)
Signal law:
  y  = (x * h_rir)[0:N]  (causal linear convolution, zero history) if apply_rir else x
  y *= rms(x) / rms(y)   (RIR keeps the clip's loudness; skipped when rms(y) == 0)
  n  = noise[noise][offset : offset + N];  gain = rms(y) / (rms(n) * 10**(snr_db/20))   (0 if rms(n) == 0)
  out = clip(y + gain * n, -1, 1)         (no noise -> out = clip(y, -1, 1))

``audio_augment(..., dtype=np.float32)`` is the fp32 RESTATEMENT of the same steps (every array and scalar in float32):
the yardstick the device bounds rest on.  ``defect=`` restates the law in float64 with exactly ONE planted mistake
(DEFECTS below), the catalogue tests/test_input_stage_bounds.py holds those bounds against.
"""
import numpy as np

from .philox import philox4x32_10, make_ctr, make_key, prob_threshold

TAG_AUDIO = 2

# name -> what is wrong (everything else stays the spec)
DEFECTS = {
    "noise_rms_shift_plus": "noise RMS over noise[offset+1 : offset+1+N] (the mixed segment is noise[offset : offset+N])",
    "noise_rms_shift_minus": "noise RMS over noise[offset-1 : offset-1+N]",
    "noise_rms_whole_clip": "noise RMS over the whole noise clip",
    "gain_before_loudness": "SNR gain from rms(y) before the loudness scale",
    "loudness_untruncated": "loudness scale from the untruncated N+L-1 convolution",
    "clip_before_noise": "clip applied before the noise is added",
}


def audio_choices(B, N, R, K, Nn, rir_prob, noise_prob, snr_min, snr_max, seed=0, step=0, sample_offset=0):
    """-> dict of arrays: rir (int, -1 = none), noise (int, -1 = none), offset (int), snr_db (float32)."""
    g = (np.arange(B, dtype=np.uint64) + np.uint64(sample_offset))
    key = make_key(seed)
    r_rir = philox4x32_10(make_ctr(step, g, TAG_AUDIO, 0), key).astype(np.uint64)
    r_noi = philox4x32_10(make_ctr(step, g, TAG_AUDIO, 1), key).astype(np.uint64)
    rir = np.full(B, -1, dtype=np.int64)
    if R > 0:
        app = r_rir[:, 0] < np.uint64(prob_threshold(rir_prob))
        rir = np.where(app, (r_rir[:, 1] % np.uint64(R)).astype(np.int64), -1)
    noise = np.full(B, -1, dtype=np.int64)
    offset = np.zeros(B, dtype=np.int64)
    if K > 0:
        app = r_noi[:, 0] < np.uint64(prob_threshold(noise_prob))
        noise = np.where(app, (r_noi[:, 1] % np.uint64(K)).astype(np.int64), -1)
        offset = (r_noi[:, 2] % np.uint64(Nn - N + 1)).astype(np.int64)
    u = (r_noi[:, 3] >> np.uint64(8)).astype(np.float32) * np.float32(2.0 ** -24)
    snr = (u.astype(np.float64) * float(np.float32(snr_max) - np.float32(snr_min)) + float(np.float32(snr_min))).astype(np.float32)
    return dict(rir=rir, noise=noise, offset=offset, snr_db=snr)


def conv_sequential_f32(x, h):
    """(x * h)[0:N] as the device's direct form sums it: one running fp32 sum per output, taps in ascending order, each step
    an fma (product exact in float64, one rounding to float32).  A zero tap adds an exact zero and is skipped."""
    x64, N = np.asarray(x, dtype=np.float32).astype(np.float64), len(x)
    acc = np.zeros(N, np.float32)
    for k in np.flatnonzero(np.asarray(h)[:N]):
        acc[k:] = (acc[k:].astype(np.float64) + float(np.float32(h[k])) * x64[:N - k]).astype(np.float32)
    return acc


def audio_augment(x, rirs, noises, rir_prob, noise_prob, snr_min, snr_max, seed=0, step=0, sample_offset=0,
                  dtype=np.float64, defect=None, conv_order=None):
    """x (B,N) -> (out (B,N) ``dtype``, choices).  ``conv_order="sequential"`` (float32 only) takes the convolution from
    ``conv_sequential_f32``: the restatement of the device's direct form in ITS order of operations."""
    if defect is not None and defect not in DEFECTS:
        raise ValueError(f"unknown augmentation defect {defect!r}")
    ft = np.dtype(dtype).type
    x = np.asarray(x, dtype=ft)
    B, N = x.shape
    R = 0 if rirs is None else rirs.shape[0]
    K, Nn = (0, 0) if noises is None else noises.shape
    ch = audio_choices(B, N, R, K, Nn, rir_prob, noise_prob, snr_min, snr_max, seed, step, sample_offset)
    rms = lambda v: np.sqrt(np.mean(v ** 2, dtype=ft))
    out = np.empty_like(x)
    for b in range(B):
        y = x[b]
        rx = ry = rms(y)
        if ch["rir"][b] >= 0:
            if conv_order == "sequential":
                assert ft is np.float32 and defect is None
                full = conv_sequential_f32(x[b], rirs[ch["rir"][b]])
            else:
                full = np.convolve(x[b], np.asarray(rirs[ch["rir"][b]], dtype=ft))
            y = full[:N]
            ry0 = rms(y)
            rs = rms(full) if defect == "loudness_untruncated" else ry0
            if rs > 0:
                y = y * (rx / rs)
            ry = ry0 if defect == "gain_before_loudness" else rms(y)
        if defect == "clip_before_noise":
            y = np.clip(y, ft(-1.0), ft(1.0))
        if ch["noise"][b] >= 0:
            row, o = np.asarray(noises[ch["noise"][b]], dtype=ft), int(ch["offset"][b])
            n = row[o:o + N]
            if defect == "noise_rms_shift_plus":
                rn = rms(row[min(o + 1, Nn - N):min(o + 1, Nn - N) + N])
            elif defect == "noise_rms_shift_minus":
                rn = rms(row[max(o - 1, 0):max(o - 1, 0) + N])
            elif defect == "noise_rms_whole_clip":
                rn = rms(row)
            else:
                rn = rms(n)
            gain = ry / (rn * ft(10.0) ** (ft(ch["snr_db"][b]) / ft(20.0))) if rn > 0 else ft(0.0)
            y = y + gain * n
        out[b] = np.clip(y, ft(-1.0), ft(1.0))
    return out, ch
