"""The int8 law of an LSTMWakeword bundle (DESIGN.md "Export", subsection "LSTM"), restated from its text, and the cases the LSTM
export tests share.

Nothing here imports the export package or a kernel.  Arithmetic is int64 NumPy with explicit loops over steps and gate rows (a
row's sum over k is one ``np.dot`` of int64 vectors over the batch); the multiplier encoding is ``q8_cases.r_encode_multiplier``,
the search over ``fractions.Fraction``.  The two tables are DATA, taken from the bundle after ``check_tables`` has held every entry
to within 1 of its own float64 value and both to be non-decreasing.  Tensors come back unpadded, per direction.
"""
import math

import numpy as np

from tests.q8_cases import r_encode_multiplier, r_quantize_input, structured_features  # noqa: F401

H = 128
DIRS = ("fwd", "rev")
# name -> (B, T, I, layers, bidirectional, num_classes, gain): ``gain`` scales every LSTM weight and bias of ``random_state``
CASES = {"tiny": (3, 1, 40, 1, True, 2, 1.0), "odd": (13, 7, 40, 2, True, 2, 1.0), "uni": (5, 4, 24, 1, False, 2, 1.0),
         "classes": (4, 5, 40, 1, True, 3, 1.0), "saturating": (4, 40, 40, 2, True, 2, 24.0)}
CLAMPS = ("index_low", "index_high", "u_low", "u_high", "cell_low", "cell_high", "q_h_127")


def lstm_args(I, layers, bidirectional):
    return {"input_size": int(I), "hidden_size": H, "num_layers": int(layers), "bidirectional": bool(bidirectional)}


def dirs(args):
    return DIRS if args["bidirectional"] else DIRS[:1]


def stages(args):
    return ["xq"] + [f"l{k}.{d}.{s}" for k in range(args["num_layers"]) for d in dirs(args) for s in ("u", "y", "c")] + ["hcat", "logits"]


def state_keys(args):
    """[(state key suffix, bundle prefix, layer, K_in)] per layer and direction, in state-dict order."""
    nd = len(dirs(args))
    return [(f"_l{k}" + ("_reverse" if d else ""), f"l{k}.{DIRS[d]}", k, args["input_size"] if k == 0 else nd * H)
            for k in range(args["num_layers"]) for d in range(nd)]


# ------------------------------------------------------------------ the law, restated
def r_R(a, m, sh):
    """R(a, m, sh) = (int64(a) m + 2^(sh-1)) >> sh, arithmetic shift (floor)."""
    a = np.asarray(a, np.int64)
    assert (np.abs(a) < 2 ** 31).all(), "the accumulator left int32"
    return np.right_shift(a * np.int64(m) + (np.int64(1) << np.int64(sh - 1)), np.int64(sh))


def check_tables(arrays):
    """Each entry within 1 of its own float64 value, both tables non-decreasing, int16 (4096,)."""
    x = np.arange(4096, dtype=np.float64) / 256.0 - 8.0
    for name, f in (("tab.sigmoid", 1.0 / (1.0 + np.exp(-x))), ("tab.tanh", np.tanh(x))):
        t = arrays[name]
        assert t.dtype == np.int16 and t.shape == (4096,), name
        assert (np.abs(t.astype(np.float64) - f * 2.0 ** 15) <= 1.0).all(), name
        assert (np.diff(t.astype(np.int64)) >= 0).all(), name


def r_look(tab, a, hits=None):
    if hits is not None:
        hits["index_low"] |= bool((a < -2048).any())
        hits["index_high"] |= bool((a > 2047).any())
    return tab[np.clip(a, -2048, 2047) + 2048].astype(np.int64)


def r_forward(args, arrays, x, hits=None):
    """Every tensor of the int8 network: {stage: array}; ``x`` (B,1,F,T) features or (B,T,F) sequences.  ``hits``: a dict that
    records which clamps of the law were reached (CLAMPS)."""
    a = arrays
    check_tables(a)
    if hits is not None:
        for k in CLAMPS:
            hits.setdefault(k, False)
    sig, tanh = a["tab.sigmoid"], a["tab.tanh"]
    x = np.asarray(x, np.float32)
    if x.ndim == 4:
        x = x[:, 0].transpose(0, 2, 1)
    z_in = int(a["input_zero"][0])
    q_in = np.ascontiguousarray(r_quantize_input(x, a["input_scale"][0], z_in)).astype(np.int64)
    out = {"xq": q_in.astype(np.int8)}
    B, T, _ = q_in.shape
    hcat = []
    for k in range(args["num_layers"]):
        ys = []
        for d in dirs(args):
            p = f"l{k}.{d}"
            wi, bi, mi, shi = (a[p + ".ih" + s].astype(np.int64) for s in (".w", ".b", ".m", ".sh"))
            wh, bh, mh, shh = (a[p + ".hh" + s].astype(np.int64) for s in (".w", ".b", ".m", ".sh"))
            u = np.zeros((B, T, 4 * H), np.int64)
            for n in range(4 * H):
                raw = r_R(np.dot(q_in - z_in, wi[n]) + bi[n], mi[n], shi[n])
                if hits is not None:
                    hits["u_low"] |= bool((raw < -32768).any())
                    hits["u_high"] |= bool((raw > 32767).any())
                u[:, :, n] = np.clip(raw, -32768, 32767)
            y = np.zeros((B, T, H), np.int64)
            q_h, c = np.zeros((B, H), np.int64), np.zeros((B, H), np.int64)
            for t in (range(T) if d == "fwd" else range(T - 1, -1, -1)):
                pre = np.zeros((B, 4 * H), np.int64)
                for n in range(4 * H):
                    pre[:, n] = u[:, t, n] + r_R(np.dot(q_h, wh[n]) + bh[n], mh[n], shh[n])
                i, f = r_look(sig, pre[:, :H], hits), r_look(sig, pre[:, H:2 * H], hits)
                g, o = r_look(tanh, pre[:, 2 * H:3 * H], hits), r_look(sig, pre[:, 3 * H:], hits)
                raw = (f * c + ((i * g + 8) >> 4) + 2 ** 14) >> 15
                c = np.clip(raw, -32768, 32767)
                h16 = (o * r_look(tanh, (c + 4) >> 3) + 2 ** 14) >> 15
                raw_h = (h16 + 128) >> 8
                q_h = np.clip(raw_h, -128, 127)
                if hits is not None:
                    hits["cell_low"] |= bool((raw < -32768).any())
                    hits["cell_high"] |= bool((raw > 32767).any())
                    hits["q_h_127"] |= bool((raw_h > 127).any())
                y[:, t] = q_h
            out[p + ".u"], out[p + ".y"], out[p + ".c"] = u.astype(np.int16), y.astype(np.int8), c.astype(np.int16)
            ys.append(y)
            if k == args["num_layers"] - 1:
                hcat.append(y[:, T - 1] if d == "fwd" else y[:, 0])
        q_in, z_in = np.concatenate(ys, axis=2), 0
    hcat = np.concatenate(hcat, axis=1)
    out["hcat"] = hcat.astype(np.int8)
    acc = hcat @ a["fc.w"].astype(np.int64).T + a["fc.b"].astype(np.int64)
    assert (np.abs(acc) < 2 ** 31).all()
    out["logits"] = acc.astype(np.float32) * a["fc.scale"].astype(np.float32)                    # one fp32 multiply
    return out


# ------------------------------------------------------------------ the export derivation, restated
def r_tables():
    x = np.arange(4096, dtype=np.float64) / 256.0 - 8.0
    sig = np.minimum(np.rint(1.0 / (1.0 + np.exp(-x)) * 2.0 ** 15), 32767).astype(np.int16)
    tanh = np.clip(np.rint(np.tanh(x) * 2.0 ** 15), -32767, 32767).astype(np.int16)
    return sig, tanh


def r_quantize_model(state, args, x_min, x_max):
    """The arrays of the int8 bundle of ``state`` under the calibrated input range, from the text of the law."""
    st = {k: np.asarray(v, np.float64) for k, v in state.items()}
    lo, hi = min(x_min, 0.0), max(x_max, 0.0)
    if hi - lo <= 0:
        hi = 1.0
    s_x = np.float32((hi - lo) / 255.0)
    z_x = int(np.clip(np.rint(-128.0 - lo / float(s_x)), -128, 127))
    a = {"input_scale": np.array([s_x], np.float32), "input_zero": np.array([z_x], np.int32)}

    def rows(name, w, b, s_in):
        amax = np.abs(w).max(axis=1)
        s_w = np.where(amax > 0, amax / 127.0, 1.0)
        a[name + ".w"] = np.clip(np.rint(w / s_w[:, None]), -127, 127).astype(np.int8)
        a[name + ".b"] = np.rint(b / (s_in * s_w)).astype(np.int32)
        ms = [r_encode_multiplier(s_in * s_w[n] * 256.0) for n in range(w.shape[0])]
        a[name + ".m"] = np.array([m for m, _ in ms], np.int32)
        a[name + ".sh"] = np.array([s for _, s in ms], np.int32)
    for sfx, p, k, _ in state_keys(args):
        rows(p + ".ih", st["lstm.weight_ih" + sfx], st["lstm.bias_ih" + sfx], float(s_x) if k == 0 else 2.0 ** -7)
        rows(p + ".hh", st["lstm.weight_hh" + sfx], st["lstm.bias_hh" + sfx], 2.0 ** -7)
    w = st["fc.1.weight"]
    amax = np.abs(w).max(axis=1)
    s_w = np.where(amax > 0, amax / 127.0, 1.0)
    a["fc.w"] = np.clip(np.rint(w / s_w[:, None]), -127, 127).astype(np.int8)
    a["fc.b"] = np.rint(st["fc.1.bias"] / (2.0 ** -7 * s_w)).astype(np.int32)
    a["fc.scale"] = (2.0 ** -7 * s_w).astype(np.float32)
    a["tab.sigmoid"], a["tab.tanh"] = r_tables()
    return a


def float_forward(state, args, x):
    """The fp32 model's eval forward in float64 -> logits (B, nc); ``x`` (B,1,F,T) or (B,T,F)."""
    st = {k: np.asarray(v, np.float64) for k, v in state.items()}
    x = np.asarray(x, np.float64)
    if x.ndim == 4:
        x = x[:, 0].transpose(0, 2, 1)
    B, T, _ = x.shape
    sg = lambda v: 1.0 / (1.0 + np.exp(-v))       # noqa: E731
    nd, last = len(dirs(args)), []
    for k in range(args["num_layers"]):
        ys = []
        for d in range(nd):
            sfx = f"_l{k}" + ("_reverse" if d else "")
            pre = x @ st["lstm.weight_ih" + sfx].T + st["lstm.bias_ih" + sfx] + st["lstm.bias_hh" + sfx]
            h, c, y = np.zeros((B, H)), np.zeros((B, H)), np.zeros((B, T, H))
            for t in (range(T) if d == 0 else range(T - 1, -1, -1)):
                g_in = pre[:, t] + h @ st["lstm.weight_hh" + sfx].T
                c = sg(g_in[:, H:2 * H]) * c + sg(g_in[:, :H]) * np.tanh(g_in[:, 2 * H:3 * H])
                h = sg(g_in[:, 3 * H:]) * np.tanh(c)
                y[:, t] = h
            ys.append(y)
            if k == args["num_layers"] - 1:
                last.append(h)
        x = np.concatenate(ys, axis=2)
    return np.concatenate(last, axis=1) @ st["fc.1.weight"].T + st["fc.1.bias"]


# ------------------------------------------------------------------ cases
def header_for(args, num_classes=2, T=45, kind="int8"):
    F = args["input_size"]
    layers = [f"l{k}.{d}.{part}" for k in range(args["num_layers"]) for d in dirs(args) for part in ("ih", "hh")] + ["fc"]
    return {"format": "wakeword-bundle", "version": 1, "kind": kind, "architecture": "LSTMWakeword", "num_classes": int(num_classes),
            "input_shape": [1, 1, F, T], "feature_shape": [F, T], "layers": layers, "lstm": dict(args)}


def random_state(args, num_classes=2, seed=0, gain=1.0, head_gain=1.0):
    """An LSTMWakeword state_dict (float32 NumPy) under the reference's keys, NumPy's PCG64 stream: lstm.* uniform in
    +-gain/sqrt(128) (nn.LSTM's initialisation times ``gain``), fc.* in +-head_gain/sqrt(in_features); one all-zero gate row
    (row 7 of l0's forward weight_hh)."""
    g = np.random.default_rng(seed)
    st = {}
    bound = gain * H ** -0.5
    for sfx, _, _, K in state_keys(args):
        st["lstm.weight_ih" + sfx] = g.uniform(-bound, bound, (4 * H, K))
        st["lstm.weight_hh" + sfx] = g.uniform(-bound, bound, (4 * H, H))
        st["lstm.bias_ih" + sfx] = g.uniform(-bound, bound, 4 * H)
        st["lstm.bias_hh" + sfx] = g.uniform(-bound, bound, 4 * H)
    st["lstm.weight_hh_l0"][7] = 0.0
    C = len(dirs(args)) * H
    st["fc.1.weight"] = g.uniform(-1, 1, (num_classes, C)) * head_gain * C ** -0.5
    st["fc.1.bias"] = g.uniform(-1, 1, num_classes) * C ** -0.5
    return {k: np.asarray(v, np.float32) for k, v in st.items()}


def features(B, T, I, seed=1, steady=False):
    """(B,1,I,T) float32 in [-12, 8]: wider than the calibrated range of ``case``, so the input saturates at both ends.
    ``steady``: every channel keeps its level over time but for a little noise, so a saturated gate stays saturated from step to
    step and the cell can run into its clamp."""
    g = np.random.default_rng(seed)
    if not steady:
        return g.uniform(-12.0, 8.0, (B, 1, I, T)).astype(np.float32)
    x = g.uniform(-11.7, 7.7, (B, 1, I, 1)) + g.uniform(-0.3, 0.3, (B, 1, I, T))
    return x.astype(np.float32)


_CACHE = {}


def case(name, batch=None):
    """(header, arrays, x, ref, hits) of one of CASES (``batch``: another batch size): the bundle is the restated derivation of
    ``random_state`` at the case's gain, calibrated on [-11, 7] so the input clamps at both ends; the scaled-up case runs on
    ``steady`` features; computed once per process."""
    key = (name, batch)
    if key not in _CACHE:
        B, T, I, layers, bidir, nc, gain = CASES[name]
        B = batch or B
        args = lstm_args(I, layers, bidir)
        state = random_state(args, nc, seed=3 + len(name), gain=gain)
        arrays = r_quantize_model(state, args, -11.0, 7.0)
        x = features(B, T, I, steady=gain > 1.0)
        hits = {}
        ref = r_forward(args, arrays, x, hits)
        assert ref["xq"].min() == -128 and ref["xq"].max() == 127, "the input does not saturate at both ends"
        _CACHE[key] = (header_for(args, nc, T), arrays, x, ref, hits)
    return _CACHE[key]


def clamps_reached():
    """{clamp: [cases that reach it]} over CASES."""
    out = {k: [] for k in CLAMPS}
    for name in CASES:
        for k, v in case(name)[4].items():
            if v:
                out[k].append(name)
    return out


assert math.isclose(2.0 ** -7 * 256.0, 2.0)        # the hidden projection's multiplier is 2 s_wh
