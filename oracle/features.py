"""Log-mel / MFCC oracle (float64 numpy + an fp32 torch.stft variant).

The reference's ``src/data/feature_extraction.py`` is ABSENT from the snapshot
(SURVEY.md F1); its API is known only from call sites
(``src/evaluation/evaluator.py:86-94,122-128``, ``src/evaluation/inference.py:94-102,194-200``)
and its output shape from ``src/export/onnx_exporter.py:316-320``.  The arithmetic
below is therefore the BUILD'S OWN SPEC (DESIGN.md "Feature spec"):
**parity unpinned** with respect to the reference.

Spec: periodic Hann(n_fft); center=True with reflect padding n_fft//2;
T = 1 + N // hop frames; rFFT(n_fft); power |X|^2; HTK mel triangular filterbank
(f_min=0, f_max=sr/2, norm=None), as published for torchaudio 2.1
``functional.melscale_fbanks``; log(mel + 1e-6) natural log.  MFCC = orthonormal
DCT-II of the log-mel over the mel axis, first n_mfcc coefficients.

``defect=`` (default None = the spec) restates the law in float64 with exactly ONE planted mistake, the catalogue
tests/test_input_stage_bounds.py holds the parity bounds against: a bound that accepts one of these is too loose.
"""
import numpy as np

LOG_EPS = 1e-6

# name -> what is wrong (everything else stays the float64 spec)
DEFECTS = {
    "int16_scale_32767": "int16 PCM scaled by 1/32767 instead of 1/32768 (pcm16_to_float)",
    "mel_fp16": "mel weights rounded to fp16",
    "mel_bf16": "mel weights rounded to bf16",
    "window_fp16": "Hann window rounded to fp16",
    "hann_symmetric": "symmetric instead of periodic Hann",
    "pad_symmetric": "symmetric (edge sample repeated) instead of reflect padding",
    "dct_row0_unscaled": "DCT row 0 without its 1/sqrt(2) (MFCC only)",
}


def round_to(a, kind: str) -> np.ndarray:
    """float64 array -> its values after rounding (to nearest even) to "fp16" or "bf16", back in float64."""
    a = np.asarray(a, dtype=np.float64)
    if kind == "fp16":
        return a.astype(np.float16).astype(np.float64)
    u = a.astype(np.float32).view(np.uint32)
    u = (u + np.uint32(0x7FFF) + ((u >> np.uint32(16)) & np.uint32(1))) & np.uint32(0xFFFF0000)
    return u.view(np.float32).astype(np.float64)


def _check_defect(defect):
    if defect is not None and defect not in DEFECTS:
        raise ValueError(f"unknown front-end defect {defect!r}")


def pcm16_to_float(xi, defect=None) -> np.ndarray:
    """int16 PCM -> float64 waveform: x = xi / 32768."""
    _check_defect(defect)
    return np.asarray(xi, dtype=np.float64) / (32767.0 if defect == "int16_scale_32767" else 32768.0)


def hann_periodic(n_fft: int) -> np.ndarray:
    k = np.arange(n_fft, dtype=np.float64)
    return 0.5 - 0.5 * np.cos(2.0 * np.pi * k / n_fft)


def _window(n_fft: int, defect=None) -> np.ndarray:
    if defect == "hann_symmetric":
        k = np.arange(n_fft, dtype=np.float64)
        return 0.5 - 0.5 * np.cos(2.0 * np.pi * k / (n_fft - 1))
    w = hann_periodic(n_fft)
    return round_to(w, "fp16") if defect == "window_fp16" else w


def hz_to_mel_htk(f):
    return 2595.0 * np.log10(1.0 + np.asarray(f, dtype=np.float64) / 700.0)


def mel_to_hz_htk(m):
    return 700.0 * (10.0 ** (np.asarray(m, dtype=np.float64) / 2595.0) - 1.0)


def mel_filterbank(n_freqs: int, n_mels: int, sample_rate: int,
                   f_min: float = 0.0, f_max: float = None) -> np.ndarray:
    """(n_freqs, n_mels) float64 triangular HTK filterbank, norm=None."""
    if f_max is None:
        f_max = sample_rate / 2.0
    all_freqs = np.linspace(0.0, sample_rate / 2.0, n_freqs)
    m_pts = np.linspace(hz_to_mel_htk(f_min), hz_to_mel_htk(f_max), n_mels + 2)
    f_pts = mel_to_hz_htk(m_pts)
    f_diff = f_pts[1:] - f_pts[:-1]
    slopes = f_pts[None, :] - all_freqs[:, None]          # (n_freqs, n_mels+2)
    down = -slopes[:, :-2] / f_diff[:-1]
    up = slopes[:, 2:] / f_diff[1:]
    return np.maximum(0.0, np.minimum(down, up))


def dct_matrix(n_mfcc: int, n_mels: int, defect=None) -> np.ndarray:
    """(n_mfcc, n_mels) orthonormal DCT-II."""
    n = np.arange(n_mels, dtype=np.float64)
    k = np.arange(n_mfcc, dtype=np.float64)[:, None]
    d = np.cos(np.pi / n_mels * (n + 0.5) * k)
    if defect != "dct_row0_unscaled":
        d[0] *= 1.0 / np.sqrt(2.0)
    return d * np.sqrt(2.0 / n_mels)


def frame_signal(x: np.ndarray, n_fft: int, hop: int, defect=None) -> np.ndarray:
    """x (B,N) -> (B,T,n_fft) with center=True reflect padding."""
    pad = n_fft // 2
    xp = np.pad(x, ((0, 0), (pad, pad)), mode="symmetric" if defect == "pad_symmetric" else "reflect")
    T = 1 + x.shape[1] // hop
    idx = np.arange(T)[:, None] * hop + np.arange(n_fft)[None, :]
    return xp[:, idx]


def power_spectrogram(x, n_fft=1024, hop=160, defect=None):
    x = np.asarray(x, dtype=np.float64)
    fr = frame_signal(x, n_fft, hop, defect) * _window(n_fft, defect)
    spec = np.fft.rfft(fr, n=n_fft, axis=-1)              # (B,T,F)
    return (spec.real ** 2 + spec.imag ** 2)


def logmel(x, sample_rate=16000, n_fft=1024, hop=160, n_mels=40,
           f_min=0.0, f_max=None, log_eps=LOG_EPS, defect=None):
    """x (B,N) float -> (B,1,n_mels,T) float64."""
    _check_defect(defect)
    p = power_spectrogram(x, n_fft, hop, defect)          # (B,T,F)
    fb = mel_filterbank(n_fft // 2 + 1, n_mels, sample_rate, f_min, f_max)
    if defect in ("mel_fp16", "mel_bf16"):
        fb = round_to(fb, defect[4:])
    mel = p @ fb                                          # (B,T,M)
    return np.log(mel + log_eps).transpose(0, 2, 1)[:, None]


def mfcc(x, sample_rate=16000, n_fft=1024, hop=160, n_mels=40, n_mfcc=40,
         f_min=0.0, f_max=None, log_eps=LOG_EPS, defect=None):
    lm = logmel(x, sample_rate, n_fft, hop, n_mels, f_min, f_max, log_eps, defect)[:, 0]  # (B,M,T)
    d = dct_matrix(n_mfcc, n_mels, defect)
    return np.einsum("cm,bmt->bct", d, lm)[:, None]


def logmel_torch(x, sample_rate=16000, n_fft=1024, hop=160, n_mels=40,
                 f_min=0.0, f_max=None, log_eps=LOG_EPS, n_mfcc=None):
    """fp32 torch.stft formulation of the same spec (the 'reference-style PyTorch
    CPU path' used for the cpu_baseline timing and as an independent cross-check)."""
    import torch
    x = torch.as_tensor(x, dtype=torch.float32)
    win = torch.hann_window(n_fft, periodic=True, dtype=torch.float32)
    spec = torch.stft(x, n_fft, hop_length=hop, win_length=n_fft, window=win,
                      center=True, pad_mode="reflect", return_complex=True)   # (B,F,T)
    p = spec.real ** 2 + spec.imag ** 2
    fb = torch.from_numpy(mel_filterbank(n_fft // 2 + 1, n_mels, sample_rate, f_min, f_max)).float()
    mel = torch.matmul(fb.t(), p)                         # (B,M,T)
    out = torch.log(mel + log_eps)
    if n_mfcc is not None:
        d = torch.from_numpy(dct_matrix(n_mfcc, n_mels)).float()
        out = torch.matmul(d, out)
    return out[:, None]


def _tw6_f32(tw, base, k):
    """W^(base*k), k = 0..15, as k_logmel forms it: from the fp32 table entries W^(base*b) and W^(4*base*a) (k = 4a + b), the
    nine mixed ones by one complex64 product."""
    a, b = k >> 2, k & 3
    t1, t4 = tw[(base * b) & 1023], tw[(base * 4 * a) & 1023]
    return np.where(a == 0, t1, np.where(b == 0, t4, (t4 * t1).astype(np.complex64))).astype(np.complex64)


def logmel_device_order_f32(x, sample_rate=16000, n_fft=1024, hop=160, n_mels=40, f_min=0.0, f_max=None, log_eps=LOG_EPS):
    """fp32 numpy RESTATEMENT of the device's order of operations (not a yardstick: it exists to show which part of a device
    error is the round-off of its algorithm).  n_fft <= 1024 (k_logmel): the frame under its own Hann in the middle of a
    1024-sample window, two real frames as one complex 1024-point transform factored 16 x 16 x 4 with twiddles W1024^(lane*kb)
    and W64^(q*kc) formed from six fp32 table entries each, the two spectra separated as sums and differences of X[k] and
    X[N-k], 4|X|^2 with the 1/4 in the band weights.  n_fft > 1024 (k_logmel_any): bit-reversed radix-2 stages with the table
    twiddles.  x (B,N) -> (B,1,n_mels,T) float32.  The 16-point transforms inside a pass are matrix products here."""
    c64, f32 = np.complex64, np.float32
    x = np.asarray(x, dtype=f32)
    n_tab = max(n_fft, 1024)
    win = np.zeros(n_tab, f32)
    win[(n_tab - n_fft) // 2:(n_tab - n_fft) // 2 + n_fft] = hann_periodic(n_fft).astype(f32)
    ang = 2.0 * np.pi * np.arange(n_tab) / n_tab
    tw = (np.cos(ang).astype(f32) - 1j * np.sin(ang).astype(f32)).astype(c64)
    T = 1 + x.shape[1] // hop
    xp = np.pad(x, ((0, 0), (n_tab // 2, n_tab // 2)), mode="reflect")
    fr = (xp[:, np.arange(T)[:, None] * hop + np.arange(n_tab)[None, :]] * win).astype(f32)          # (B,T,n_tab)
    fb = mel_filterbank(n_fft // 2 + 1, n_mels, sample_rate, f_min, f_max).astype(f32)
    if n_fft > 1024:
        log2n = n_fft.bit_length() - 1
        rev = np.array([int(format(i, f"0{log2n}b")[::-1], 2) for i in range(n_fft)])
        z = np.empty(fr.shape, c64)
        z[..., rev] = fr
        for s in range(log2n):
            half, tstep = 1 << s, n_fft >> (s + 1)
            z = z.reshape(fr.shape[:2] + (-1, 2, half))
            v = (z[..., 1, :] * tw[np.arange(half) * tstep]).astype(c64)
            z = np.stack([z[..., 0, :] + v, z[..., 0, :] - v], axis=-2).astype(c64).reshape(fr.shape)
        p = (z.real ** 2 + z.imag ** 2).astype(f32)[..., :n_fft // 2 + 1]
        mel = p @ fb
    else:
        if T % 2:
            fr = np.concatenate([fr, np.zeros_like(fr[:, :1])], axis=1)
        z = (fr[:, 0::2] + 1j * fr[:, 1::2]).astype(c64)                                             # frames (a, b) of a wave
        k16 = np.arange(16)
        d16 = np.exp(-2j * np.pi * np.outer(k16, k16) / 16).astype(c64)
        d4 = np.exp(-2j * np.pi * np.outer(np.arange(4), np.arange(4)) / 4).astype(c64)
        y1 = np.einsum("kn,...nl->...kl", d16, z.reshape(z.shape[:2] + (16, 64))).astype(c64)       # [kb, n1 = lane]
        y1 = (y1 * _tw6_f32(tw, np.arange(64)[None, :], k16[:, None])).astype(c64)
        y2 = np.einsum("cm,...kmq->...kcq", d16, y1.reshape(y1.shape[:2] + (16, 16, 4))).astype(c64)  # [kb, kc, q]
        y2 = (y2 * _tw6_f32(tw, 16 * np.arange(4)[None, :], k16[:, None])).astype(c64)
        y3 = np.einsum("dq,...kcq->...kcd", d4, y2).astype(c64)                                      # X[16 kc + 256 kd + kb]
        X = np.empty(z.shape, c64)
        kb, kc, kd = np.meshgrid(k16, k16, np.arange(4), indexing="ij")
        X[..., (16 * kc + 256 * kd + kb).ravel()] = y3.reshape(z.shape[:2] + (-1,))
        Y = X[..., (1024 - np.arange(513)) % 1024]                                                   # X[N - k]
        Xk = X[..., :513]
        pa = ((Xk.real + Y.real) ** 2 + (Xk.imag - Y.imag) ** 2).astype(f32)
        pb = ((Xk.imag + Y.imag) ** 2 + (Xk.real - Y.real) ** 2).astype(f32)
        p = np.stack([pa, pb], axis=2).reshape(x.shape[0], -1, 513)[:, :T]
        r = 1024 // n_fft
        mel = p[..., ::r] @ (f32(0.25) * fb)
    return np.log((mel + f32(log_eps)).astype(f32)).astype(f32).transpose(0, 2, 1)[:, None]
