"""The int8 law of DESIGN.md "Export", restated from its text, and the cases the export tests share.

Nothing here imports the export package's interpreter (``export/reference.py``) or a kernel: convolutions are
``torch.nn.functional.conv2d`` on integer-valued float64 tensors (exact below 2^53), the requantisation is int64 NumPy, the
multiplier encoding is a search over ``fractions.Fraction``.  Tensors come back NHWC, as the bundle's runtimes hold them.
"""
import math
from fractions import Fraction

import numpy as np
import torch
import torch.nn.functional as TF

BLOCKS = 4
CONVS = ["stem"] + [f"{kind}{k}" for k in range(BLOCKS) for kind in ("dw", "pw")]
STAGES = ["xq"] + CONVS + ["pool", "logits"]
A_MAX_FLOOR = 255.0 * 2.0 ** -20
TIE_CH, ZERO_CH = 5, 7                 # channels the hard bundle rigs: exact rounding ties / all-zero weights


# ------------------------------------------------------------------ the law, restated
def r_round_half_even(q: Fraction) -> int:
    f = math.floor(q)
    d = q - f
    return f + (1 if d > Fraction(1, 2) or (d == Fraction(1, 2) and f % 2) else 0)


def r_encode_multiplier(r: float):
    """The (m, sh), 2^30 <= m < 2^31, 1 <= sh <= 62, with m 2^-sh nearest to r; None where no shift puts m in range."""
    if not (math.isfinite(r) and r > 0):
        return None
    R, best = Fraction(r), None
    for sh in range(1, 63):
        m = r_round_half_even(R * 2 ** sh)
        if 2 ** 30 <= m < 2 ** 31:
            err = abs(Fraction(m, 2 ** sh) - R)
            if best is None or err < best[0]:
                best = (err, m, sh)
    return None if best is None else (best[1], best[2])


def r_quantize_input(x, scale, zero):
    x = torch.as_tensor(np.asarray(x, np.float32))
    r = torch.round(x / torch.tensor(float(np.float32(scale)), dtype=torch.float32))      # one fp32 division, half to even
    r = torch.where(torch.isnan(r), torch.zeros_like(r), r).clamp(-1000.0, 1000.0)
    return (r.to(torch.int64) + int(zero)).clamp(-128, 127).to(torch.int8).numpy()


def r_requantize(acc, m, sh):
    acc, m, sh = np.asarray(acc, np.int64), np.asarray(m, np.int64), np.asarray(sh, np.int64)
    assert (np.abs(acc) < 2 ** 31).all(), "the accumulator left int32"
    t = np.right_shift(acc * m + np.left_shift(np.int64(1), sh - 1), sh)                   # arithmetic: floor
    return (np.clip(t, 0, 255) - 128).astype(np.int8)


def _i64(t):
    a = t.numpy()
    assert (a == np.rint(a)).all() and (np.abs(a) < 2.0 ** 53).all()
    return a.astype(np.int64)


def r_forward(arrays, x, want_acc=False):
    """Every stage of the int8 network: {stage: array} (NHWC int8 tensors, pool (B,64), logits float32); with ``want_acc``
    also ``acc/<conv>``, the int64 accumulators (B,H,W,64)."""
    x = np.asarray(x, np.float32)
    x = x[:, 0] if x.ndim == 4 else x
    out = {}
    z = int(arrays["input_zero"][0])
    xq = r_quantize_input(x, arrays["input_scale"][0], z)
    out["xq"] = xq
    d = torch.from_numpy(xq.astype(np.float64) - z)[:, None]                # (B,1,F,T): q - z_in, zero padding = z_in
    for name in CONVS:
        w = torch.from_numpy(arrays[name + ".w"].astype(np.float64))
        if name == "stem":
            c = TF.conv2d(d, w.view(64, 1, 3, 3), stride=2, padding=1)
        elif name.startswith("dw"):
            c = TF.conv2d(d, w.view(64, 1, 3, 3), padding=1, groups=64)
        else:
            c = TF.conv2d(d, w.view(64, 64, 1, 1))
        acc = _i64(c).transpose(0, 2, 3, 1) + arrays[name + ".b"].astype(np.int64)
        q = r_requantize(acc, arrays[name + ".m"], arrays[name + ".sh"])
        out[name] = q
        if want_acc:
            out["acc/" + name] = acc
        d = torch.from_numpy((q.astype(np.float64) + 128.0).transpose(0, 3, 1, 2).copy())
    S = (out[CONVS[-1]].astype(np.int64) + 128).sum(axis=(1, 2))
    p = r_requantize(S, arrays["pool.m"][0], arrays["pool.sh"][0])
    out["pool"] = p
    acc = (p.astype(np.int64) + 128) @ arrays["fc.w"].astype(np.int64).T + arrays["fc.b"].astype(np.int64)
    assert (np.abs(acc) < 2 ** 31).all()
    out["logits"] = acc.astype(np.float32) * arrays["fc.scale"].astype(np.float32)        # one fp32 multiply
    return out


# ------------------------------------------------------------------ the float model and the export derivation, restated
def float_layers(state, eps=1e-5):
    """{name: (W' float64 (C,K), b' float64 (C,))}: BatchNorm folded into its conv, in float64."""
    st = {k: np.asarray(v, np.float64) for k, v in state.items() if np.asarray(v).dtype.kind == "f"}

    def fold(wkey, bn):
        k = st[bn + ".weight"] / np.sqrt(st[bn + ".running_var"] + eps)
        w = st[wkey]
        return w.reshape(w.shape[0], -1) * k[:, None], st[bn + ".bias"] - st[bn + ".running_mean"] * k
    layers = {"stem": fold("stem.conv.weight", "stem.bn")}
    for k in range(BLOCKS):
        layers[f"dw{k}"] = fold(f"blocks.{k}.dw.weight", f"blocks.{k}.dw_bn")
        layers[f"pw{k}"] = fold(f"blocks.{k}.pw.weight", f"blocks.{k}.pw_bn")
    layers["fc"] = (st["classifier.weight"], st["classifier.bias"])
    return layers


def float_forward(state, x, eps=1e-5):
    """The fp32 model's eval forward in float64 -> (logits (B,2), {x_min, x_max, a_max[9], p_max})."""
    L = float_layers(state, eps)
    a = torch.from_numpy(np.asarray(x, np.float64))
    a = a[:, None] if a.dim() == 3 else a
    ranges = {"x_min": float(a.min()), "x_max": float(a.max()), "a_max": []}
    for name in CONVS:
        w, b = (torch.from_numpy(t) for t in L[name])
        if name == "stem":
            a = TF.conv2d(a, w.view(64, 1, 3, 3), b, stride=2, padding=1)
        elif name.startswith("dw"):
            a = TF.conv2d(a, w.view(64, 1, 3, 3), b, padding=1, groups=64)
        else:
            a = TF.conv2d(a, w.view(64, 64, 1, 1), b)
        a = a.clamp_min(0.0)
        ranges["a_max"].append(float(a.max()))
    p = a.mean(dim=(2, 3))
    ranges["p_max"] = float(p.max())
    logits = p @ torch.from_numpy(L["fc"][0]).T + torch.from_numpy(L["fc"][1])
    return logits.numpy(), ranges


def r_quantize_model(state, feature_shape, ranges, eps=1e-5):
    """The arrays of the int8 bundle of ``state`` under calibrated ``ranges``, from the text of the law."""
    F, T = feature_shape
    HW = ((F + 1) // 2) * ((T + 1) // 2)
    L = float_layers(state, eps)
    lo, hi = min(ranges["x_min"], 0.0), max(ranges["x_max"], 0.0)
    if hi - lo <= 0:
        hi = 1.0
    s_x = np.float32((hi - lo) / 255.0)
    z_x = int(np.clip(np.rint(-128.0 - lo / float(s_x)), -128, 127))
    a = {"input_scale": np.array([s_x], np.float32), "input_zero": np.array([z_x], np.int32)}
    s_in = float(s_x)

    def weights(wf):
        amax = np.abs(wf).max(axis=1)
        s_w = np.where(amax > 0, amax / 127.0, 1.0)
        return np.clip(np.rint(wf / s_w[:, None]), -127, 127).astype(np.int8), s_w
    for name, am in zip(CONVS, ranges["a_max"]):
        wf, bf = L[name]
        q_w, s_w = weights(wf)
        s_out = max(am, A_MAX_FLOOR) / 255.0
        ms = [r_encode_multiplier(s_in * s_w[c] / s_out) for c in range(64)]
        a[name + ".w"], a[name + ".b"] = q_w, np.rint(bf / (s_in * s_w)).astype(np.int32)
        a[name + ".m"] = np.array([m for m, _ in ms], np.int32)
        a[name + ".sh"] = np.array([s for _, s in ms], np.int32)
        s_in = s_out
    s_p = max(ranges["p_max"], A_MAX_FLOOR) / 255.0
    m_p, sh_p = r_encode_multiplier(s_in / (HW * s_p))
    a["pool.m"], a["pool.sh"] = np.array([m_p], np.int32), np.array([sh_p], np.int32)
    q_w, s_w = weights(L["fc"][0])
    a["fc.w"], a["fc.b"] = q_w, np.rint(L["fc"][1] / (s_p * s_w)).astype(np.int32)
    a["fc.scale"] = (s_p * s_w).astype(np.float32)
    return a


# ------------------------------------------------------------------ cases
def header_for(F, T, kind="int8"):
    return {"format": "wakeword-bundle", "version": 1, "kind": kind, "architecture": "cnn_small", "num_classes": 2,
            "input_shape": [1, 1, F, T], "feature_shape": [F, T], "layers": CONVS + ["pool", "fc"]}


def random_state(seed=0, dead=None):
    """A cnn_small state_dict (float32 NumPy) with non-trivial BatchNorm statistics; ``dead``: the conv (a CONVS name)
    whose BatchNorm has gamma = 0 and beta = -1, so its ReLU output is 0 everywhere -- a dead layer, a_max = 0."""
    g = np.random.default_rng(seed)
    st = {}

    def bn(prefix, name):
        st[prefix + ".weight"] = g.uniform(0.5, 1.5, 64)
        st[prefix + ".bias"] = g.normal(0.0, 0.3, 64)
        st[prefix + ".running_mean"] = g.normal(0.0, 0.3, 64)
        st[prefix + ".running_var"] = g.uniform(0.3, 2.0, 64)
        if name == dead:
            st[prefix + ".weight"], st[prefix + ".bias"] = np.zeros(64), -np.ones(64)
    st["stem.conv.weight"] = g.normal(0, 0.4, (64, 1, 3, 3))
    bn("stem.bn", "stem")
    for k in range(BLOCKS):
        st[f"blocks.{k}.dw.weight"] = g.normal(0, 0.45, (64, 1, 3, 3))
        bn(f"blocks.{k}.dw_bn", f"dw{k}")
        st[f"blocks.{k}.pw.weight"] = g.normal(0, 0.18, (64, 64, 1, 1))
        bn(f"blocks.{k}.pw_bn", f"pw{k}")
    st["blocks.1.dw.weight"][ZERO_CH] = 0.0                    # an all-zero weight channel: s_w = 1
    st["classifier.weight"] = g.normal(0, 0.3, (2, 64))
    st["classifier.bias"] = g.normal(0, 0.1, 2)
    return {k: np.asarray(v, np.float32) for k, v in st.items()}


def structured_features(n, F=40, T=151, seed=0):
    """Log-mel-like maps (n,1,F,T) float32: a noise floor, a frequency sweep and a burst, each at a level that varies from sample
    to sample, so the logit margin varies across samples by far more than the quantisation error."""
    g = np.random.default_rng(seed)
    f, t = np.arange(F)[:, None], np.arange(T)[None, :]
    x = np.empty((n, 1, F, T), np.float32)
    for i in range(n):
        level = -9.0 + 8.0 * (i % 8) / 7.0
        floor = -11.0 + 5.0 * ((i * 5) % 8) / 7.0
        m = np.full((F, T), floor) + g.normal(0, 0.4, (F, T))
        slope = (0.1 + 0.05 * (i % 5)) * (1 if i % 2 else -1)
        centre = F / 2 + slope * (t - T / 2)
        m += (level - floor) * np.exp(-0.5 * ((f - centre) / (1.0 + i % 3)) ** 2)
        t0, width = int(g.integers(0, max(T - 40, 1))), int(g.integers(8, 40))
        m[:, t0:t0 + width] += (3.0 + i % 4) * np.exp(-0.5 * ((f - g.integers(0, F)) / 4.0) ** 2)
        x[i, 0] = m
    return x


def hard_bundle(F, T, seed=0):
    """(header, arrays): a bundle written integer by integer on which, with ``hard_features``, every hard spot of the law
    occurs; ``assert_hard`` checks that it does.  Weights are random and asymmetric (a transposed pointwise product cannot
    pass); channel TIE_CH of every conv has m = 2^30, sh = 31 -- every odd accumulator is an exact tie -- and weights
    +1, -1, +1, .. that sum to zero, so its accumulators are small and of both signs; channel ZERO_CH has all-zero weights."""
    g = np.random.default_rng(seed)
    a = {"input_scale": np.array([0.0625], np.float32), "input_zero": np.array([37], np.int32)}
    for name in CONVS:
        pw = name.startswith("pw")
        w = g.integers(-127, 128, (64, 64 if pw else 9)).astype(np.int8)
        b = g.integers(-20000, 20001, 64).astype(np.int32)
        m = g.integers(2 ** 30, 2 ** 31, 64).astype(np.int32)
        sh = np.full(64, 38 if pw else 37, np.int32)
        w[TIE_CH] = np.resize([1, -1], w.shape[1])
        w[TIE_CH, -1] = -1 if pw else 0                      # the row sums to zero: accumulators of both signs
        b[TIE_CH], m[TIE_CH], sh[TIE_CH] = 0, 2 ** 30, 31
        w[ZERO_CH], b[ZERO_CH], m[ZERO_CH], sh[ZERO_CH] = 0, 3001, 2 ** 30 + 12345, 36
        a[name + ".w"], a[name + ".b"], a[name + ".m"], a[name + ".sh"] = w, b, m, sh
    HW = ((F + 1) // 2) * ((T + 1) // 2)
    m_p, sh_p = r_encode_multiplier(1.5 / HW)
    a["pool.m"], a["pool.sh"] = np.array([m_p], np.int32), np.array([sh_p], np.int32)
    a["fc.w"] = g.integers(-127, 128, (2, 64)).astype(np.int8)
    a["fc.b"] = g.integers(-5000, 5001, 2).astype(np.int32)
    a["fc.scale"] = np.array([1.25e-4, 2.5e-4], np.float32)
    return header_for(F, T), a


def hard_features(F, T, B, seed=1):
    return np.random.default_rng(seed).uniform(-12.0, 8.0, (B, 1, F, T)).astype(np.float32)


def assert_hard(arrays, ref):
    """``ref = r_forward(arrays, x, want_acc=True)``: the hard spots occur."""
    assert int(arrays["input_zero"][0]) != 0
    assert ref["xq"].min() == -128 and ref["xq"].max() == 127, "the input does not saturate at both ends"
    for name in CONVS:
        q, acc = ref[name], ref["acc/" + name]
        assert q.min() == -128 and q.max() == 127, f"{name}: outputs are not clamped at both ends"
        tie = acc[..., TIE_CH]
        assert ((tie % 2 == 1) & (tie > 0)).any() and ((tie % 2 == 1) & (tie < 0)).any(), f"{name}: no ties of both signs"
        assert not arrays[name + ".w"][ZERO_CH].any()
        assert (np.unique(q[..., ZERO_CH]).size == 1)
    assert np.unique(ref["pool"]).size > 8
