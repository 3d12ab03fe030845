"""The int8 law of a CRNNWakeword bundle (DESIGN.md "Export", subsections "GRU" and "CRNN"), restated from its text, and the cases
the CRNN export tests share.

Nothing here imports the export package or a kernel.  The conv stack is ``tests.q8_cases``' (its ``r_forward`` convs, its
``float_layers`` and the derivation of its ``r_quantize_model``); the frequency mean is int64 NumPy; the GRU stack is int64 NumPy
with explicit loops over steps and gate rows (a row's sum over k is one ``np.dot`` of int64 vectors over the batch); the multiplier
encoding is ``q8_cases.r_encode_multiplier``.  The two tables are DATA, taken from the bundle after ``check_tables`` (the LSTM
cases') has held every entry to within 1 of its own float64 value.  Tensors come back unpadded, per direction.

Two families of cases: GRU-stack cases (``STACK_CASES``: a stack on quantised (B,T,I) rows, which drive the layer kernels directly)
and whole-model cases (``CASES``).
"""
import numpy as np
import torch
import torch.nn.functional as TF

from tests import q8_cases as Q
from tests.q8_cases import r_encode_multiplier, r_quantize_input, structured_features  # noqa: F401
from tests.q8_lstm_cases import check_tables, features, r_R, r_look, r_tables

H = 128
DIRS = ("fwd", "rev")
CONVS = Q.CONVS
# name -> (B, T, I, layers, bidirectional, num_classes, gain): ``gain`` scales every GRU weight and bias of ``random_gru``
STACK_CASES = {"tiny": (3, 1, 40, 1, True, 2, 1.0), "odd": (13, 7, 40, 2, True, 2, 1.0), "uni": (5, 4, 24, 1, False, 2, 1.0),
               "classes": (4, 5, 40, 1, True, 3, 1.0), "saturating": (4, 40, 40, 2, True, 2, 24.0)}
# name -> (B, F, T, layers, bidirectional, num_classes)
CASES = {"tiny": (3, 8, 1, 1, True, 2), "odd": (13, 13, 21, 2, True, 2), "uni": (5, 24, 8, 1, False, 2), "classes": (4, 40, 9, 1, True, 3)}
CLAMPS = ("index_low", "index_high", "u_low", "u_high", "q_h_127")
NARROW = 0.6        # the whole-model cases calibrate every conv maximum and f_max at this fraction of what their inputs reach


def crnn_args(layers, bidirectional):
    return {"hidden_size": H, "num_layers": int(layers), "bidirectional": bool(bidirectional)}


def dirs(args):
    return DIRS if args["bidirectional"] else DIRS[:1]


def stack_stages(args):
    return [f"l{k}.{d}.{s}" for k in range(args["num_layers"]) for d in dirs(args) for s in ("u", "y", "h")]


def stages(args):
    return ["xq"] + ["front." + c for c in CONVS] + ["seq"] + stack_stages(args) + ["hcat", "logits"]


def state_keys(args, input_size):
    """[(state key suffix, bundle prefix, layer, K_in)] per layer and direction, in state-dict order."""
    nd = len(dirs(args))
    return [(f"_l{k}" + ("_reverse" if d else ""), f"l{k}.{DIRS[d]}", k, input_size if k == 0 else nd * H)
            for k in range(args["num_layers"]) for d in range(nd)]


# ------------------------------------------------------------------ the law, restated
def r_gru_stack(args, a, q_in, z_in, hits=None):
    """The GRU stack on int64 rows ``q_in`` (B,T,K) with zero point ``z_in``: ({stage: array}, hcat int64 (B, nd H))."""
    check_tables(a)
    if hits is not None:
        for k in CLAMPS:
            hits.setdefault(k, False)
    sig, tanh = a["tab.sigmoid"], a["tab.tanh"]
    q_in = np.asarray(q_in, np.int64)
    B, T, _ = q_in.shape
    out, hcat = {}, []
    for k in range(args["num_layers"]):
        ys = []
        for d in dirs(args):
            p = f"l{k}.{d}"
            wi, bi, mi, shi = (a[p + ".ih" + s].astype(np.int64) for s in (".w", ".b", ".m", ".sh"))
            wh, bh, mh, shh = (a[p + ".hh" + s].astype(np.int64) for s in (".w", ".b", ".m", ".sh"))
            u = np.zeros((B, T, 3 * H), np.int64)
            for n in range(3 * H):
                raw = r_R(np.dot(q_in - z_in, wi[n]) + bi[n], mi[n], shi[n])
                if hits is not None:
                    hits["u_low"] |= bool((raw < -32768).any())
                    hits["u_high"] |= bool((raw > 32767).any())
                u[:, :, n] = np.clip(raw, -32768, 32767)
            y = np.zeros((B, T, H), np.int64)
            q_h, h16 = np.zeros((B, H), np.int64), np.zeros((B, H), np.int64)
            for t in (range(T) if d == "fwd" else range(T - 1, -1, -1)):
                v = np.zeros((B, 3 * H), np.int64)
                for n in range(3 * H):
                    v[:, n] = r_R(np.dot(q_h, wh[n]) + bh[n], mh[n], shh[n])          # unclamped
                r = r_look(sig, u[:, t, :H] + v[:, :H], hits)
                z = r_look(sig, u[:, t, H:2 * H] + v[:, H:2 * H], hits)
                n_ = r_look(tanh, u[:, t, 2 * H:] + ((r * v[:, 2 * H:] + 2 ** 14) >> 15), hits)
                h16 = ((32768 - z) * n_ + z * h16 + 2 ** 14) >> 15
                assert (np.abs(h16) <= 32767).all(), "the carried state left its stated bound"
                raw_h = (h16 + 128) >> 8
                assert (raw_h >= -128).all()
                q_h = np.clip(raw_h, -128, 127)
                if hits is not None:
                    hits["q_h_127"] |= bool((raw_h > 127).any())
                y[:, t] = q_h
            out[p + ".u"], out[p + ".y"], out[p + ".h"] = u.astype(np.int16), y.astype(np.int8), h16.astype(np.int16)
            ys.append(y)
            if k == args["num_layers"] - 1:
                hcat.append(y[:, T - 1] if d == "fwd" else y[:, 0])
        q_in, z_in = np.concatenate(ys, axis=2), 0
    return out, np.concatenate(hcat, axis=1)


def _head(a, hcat, out):
    out["hcat"] = hcat.astype(np.int8)
    acc = hcat @ a["fc.w"].astype(np.int64).T + a["fc.b"].astype(np.int64)
    assert (np.abs(acc) < 2 ** 31).all()
    out["logits"] = acc.astype(np.float32) * a["fc.scale"].astype(np.float32)                    # one fp32 multiply
    return out


def r_forward_stack(args, arrays, x, hits=None):
    """A GRU stack on quantised features: ``x`` (B,1,I,T) -> {xq (B,T,I), the stack's tensors, hcat, logits}."""
    x = np.asarray(x, np.float32)[:, 0].transpose(0, 2, 1)
    z_in = int(arrays["input_zero"][0])
    q_in = np.ascontiguousarray(r_quantize_input(x, arrays["input_scale"][0], z_in))
    out = {"xq": q_in}
    stack, hcat = r_gru_stack(args, arrays, q_in, z_in, hits)
    out.update(stack)
    return _head(arrays, hcat, out)


def _front_arrays(arrays):
    """The conv arrays under cnn_small's names, with an inert pool and classifier, for ``q8_cases.r_forward``."""
    a = {k[len("front."):]: v for k, v in arrays.items() if k.startswith("front.")}
    a["input_scale"], a["input_zero"] = arrays["input_scale"], arrays["input_zero"]
    a["pool.m"], a["pool.sh"] = np.array([2 ** 30], np.int32), np.array([40], np.int32)
    a["fc.w"], a["fc.b"], a["fc.scale"] = np.zeros((2, 64), np.int8), np.zeros(2, np.int32), np.ones(2, np.float32)
    return a


def r_forward(args, arrays, x, hits=None):
    """Every tensor of the int8 CRNN: {stage: array}; ``x`` (B,1,F,T) features."""
    conv = Q.r_forward(_front_arrays(arrays), x)
    out = {"xq": conv["xq"]}
    for c in CONVS:
        out["front." + c] = conv[c]
    S = (conv[CONVS[-1]].astype(np.int64) + 128).sum(axis=1)                      # over the frequency axis: (B,W',64)
    seq = np.clip(-128 + r_R(S, int(arrays["fmean.m"][0]), int(arrays["fmean.sh"][0])), -128, 127)
    out["seq"] = seq.astype(np.int8)
    stack, hcat = r_gru_stack(args, arrays, seq, -128, hits)
    out.update(stack)
    return _head(arrays, hcat, out)


# ------------------------------------------------------------------ the float model and the export derivation, restated
def _front_state(state):
    st = {k[len("front."):]: v for k, v in state.items() if k.startswith("front.")}
    st["classifier.weight"], st["classifier.bias"] = np.zeros((2, 64), np.float32), np.zeros(2, np.float32)
    return st


def float_front(state, x, eps=1e-5):
    """The float front end in float64: (seq (B,W',64), {x_min, x_max, a_max[9], f_max})."""
    L = Q.float_layers(_front_state(state), eps)
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
    seq = a.mean(dim=2).permute(0, 2, 1).contiguous().numpy()                     # (B,64,H',W') -> (B,W',64)
    ranges["f_max"] = float(seq.max())
    return seq, ranges


def float_gru_stack(st, args, x, prefix=""):
    """The GRU stack and its head in float64 on sequences ``x`` (B,T,K) -> logits (B, nc); ``st`` float64 state."""
    B, T, _ = x.shape
    sg = lambda v: 1.0 / (1.0 + np.exp(-v))       # noqa: E731
    nd, last = len(dirs(args)), []
    for k in range(args["num_layers"]):
        ys = []
        for d in range(nd):
            sfx = f"_l{k}" + ("_reverse" if d else "")
            w_hh, b_hh = st[prefix + "gru.weight_hh" + sfx], st[prefix + "gru.bias_hh" + sfx]
            pre = x @ st[prefix + "gru.weight_ih" + sfx].T + st[prefix + "gru.bias_ih" + sfx]
            h, y = np.zeros((B, H)), np.zeros((B, T, H))
            for t in (range(T) if d == 0 else range(T - 1, -1, -1)):
                gh = h @ w_hh.T + b_hh
                r, z = sg(pre[:, t, :H] + gh[:, :H]), sg(pre[:, t, H:2 * H] + gh[:, H:2 * H])
                n = np.tanh(pre[:, t, 2 * H:] + r * gh[:, 2 * H:])
                h = (1.0 - z) * n + z * h
                y[:, t] = h
            ys.append(y)
            if k == args["num_layers"] - 1:
                last.append(h)
        x = np.concatenate(ys, axis=2)
    return np.concatenate(last, axis=1) @ st[prefix + "fc.1.weight"].T + st[prefix + "fc.1.bias"]


def float_forward(state, args, x):
    """The fp32 CRNN's eval forward in float64 -> logits (B, nc); ``x`` (B,1,F,T)."""
    st = {k: np.asarray(v, np.float64) for k, v in state.items()}
    return float_gru_stack(st, args, float_front(state, x)[0], "rnn.")


def _rows(a, name, w, b, s_in):
    amax = np.abs(w).max(axis=1)
    s_w = np.where(amax > 0, amax / 127.0, 1.0)
    a[name + ".w"] = np.clip(np.rint(w / s_w[:, None]), -127, 127).astype(np.int8)
    a[name + ".b"] = np.rint(b / (s_in * s_w)).astype(np.int32)
    ms = [r_encode_multiplier(s_in * s_w[n] * 256.0) for n in range(w.shape[0])]
    a[name + ".m"] = np.array([m for m, _ in ms], np.int32)
    a[name + ".sh"] = np.array([s for _, s in ms], np.int32)


def r_quantize_stack(a, st, args, input_size, s_in0, prefix=""):
    """The GRU stack, its head and the tables into ``a``, from the text of the law."""
    for sfx, p, k, _ in state_keys(args, input_size):
        _rows(a, p + ".ih", st[prefix + "gru.weight_ih" + sfx], st[prefix + "gru.bias_ih" + sfx], s_in0 if k == 0 else 2.0 ** -7)
        _rows(a, p + ".hh", st[prefix + "gru.weight_hh" + sfx], st[prefix + "gru.bias_hh" + sfx], 2.0 ** -7)
    w = st[prefix + "fc.1.weight"]
    amax = np.abs(w).max(axis=1)
    s_w = np.where(amax > 0, amax / 127.0, 1.0)
    a["fc.w"] = np.clip(np.rint(w / s_w[:, None]), -127, 127).astype(np.int8)
    a["fc.b"] = np.rint(st[prefix + "fc.1.bias"] / (2.0 ** -7 * s_w)).astype(np.int32)
    a["fc.scale"] = (2.0 ** -7 * s_w).astype(np.float32)
    a["tab.sigmoid"], a["tab.tanh"] = r_tables()
    return a


def r_input(x_min, x_max):
    lo, hi = min(x_min, 0.0), max(x_max, 0.0)
    if hi - lo <= 0:
        hi = 1.0
    s_x = np.float32((hi - lo) / 255.0)
    z_x = int(np.clip(np.rint(-128.0 - lo / float(s_x)), -128, 127))
    return s_x, z_x


def r_quantize_stack_model(state, args, input_size, x_min, x_max):
    """The arrays of a GRU stack on quantised features (the stack cases), from the text of the law."""
    st = {k: np.asarray(v, np.float64) for k, v in state.items()}
    s_x, z_x = r_input(x_min, x_max)
    a = {"input_scale": np.array([s_x], np.float32), "input_zero": np.array([z_x], np.int32)}
    return r_quantize_stack(a, st, args, input_size, float(s_x))


def r_quantize_model(state, args, F, ranges, eps=1e-5):
    """The arrays of the int8 CRNN bundle of ``state`` under calibrated ``ranges`` (x_min, x_max, a_max[9], f_max)."""
    st = {k: np.asarray(v, np.float64) for k, v in state.items()}
    conv = Q.r_quantize_model(_front_state(state), (F, 1), dict(ranges, p_max=1.0), eps)
    a = {"input_scale": conv["input_scale"], "input_zero": conv["input_zero"]}
    for c in CONVS:
        for s in (".w", ".b", ".m", ".sh"):
            a["front." + c + s] = conv[c + s]
    s_a = max(ranges["a_max"][-1], Q.A_MAX_FLOOR) / 255.0
    s_f = max(ranges["f_max"], Q.A_MAX_FLOOR) / 255.0
    m_f, sh_f = r_encode_multiplier(s_a / (((F + 1) // 2) * s_f))
    a["fmean.m"], a["fmean.sh"] = np.array([m_f], np.int32), np.array([sh_f], np.int32)
    return r_quantize_stack(a, st, args, 64, s_f, "rnn.")


# ------------------------------------------------------------------ cases
def header_for(args, F, T, num_classes=2, kind="int8"):
    layers = ["front." + c for c in CONVS] + [f"l{k}.{d}.{part}" for k in range(args["num_layers"]) for d in dirs(args)
                                              for part in ("ih", "hh")] + ["fmean", "fc"]
    return {"format": "wakeword-bundle", "version": 1, "kind": kind, "architecture": "crnn", "num_classes": int(num_classes),
            "input_shape": [1, 1, F, T], "feature_shape": [F, T], "layers": layers, "crnn": dict(args)}


def random_gru(g, args, input_size, num_classes=2, gain=1.0, head_gain=1.0, prefix=""):
    """gru.* uniform in +-gain/sqrt(128) (nn.GRU's initialisation times ``gain``), drawn per (layer, direction) in the order w_ih,
    w_hh, b_ih, b_hh; then fc.1.* in +-head_gain/sqrt(in_features); one all-zero gate row (row 7 of l0's forward weight_hh)."""
    st = {}
    bound = gain * H ** -0.5
    for sfx, _, _, K in state_keys(args, input_size):
        st[prefix + "gru.weight_ih" + sfx] = g.uniform(-bound, bound, (3 * H, K))
        st[prefix + "gru.weight_hh" + sfx] = g.uniform(-bound, bound, (3 * H, H))
        st[prefix + "gru.bias_ih" + sfx] = g.uniform(-bound, bound, 3 * H)
        st[prefix + "gru.bias_hh" + sfx] = g.uniform(-bound, bound, 3 * H)
    st[prefix + "gru.weight_hh_l0"][7] = 0.0
    C = len(dirs(args)) * H
    st[prefix + "fc.1.weight"] = g.uniform(-1, 1, (num_classes, C)) * head_gain * C ** -0.5
    st[prefix + "fc.1.bias"] = g.uniform(-1, 1, num_classes) * C ** -0.5
    return {k: np.asarray(v, np.float32) for k, v in st.items()}


def random_state(args, num_classes=2, seed=0, gain=1.0, front_seed=None, head_gain=1.0):
    """A CRNNWakeword state_dict (float32 NumPy): ``q8_cases.random_state(front_seed)`` under ``front.`` (without its classifier),
    then ``random_gru`` under ``rnn.`` from NumPy's PCG64 stream of ``seed``."""
    st = {"front." + k: v for k, v in Q.random_state(seed if front_seed is None else front_seed).items()
          if not k.startswith("classifier.")}
    st.update(random_gru(np.random.default_rng(seed), args, 64, num_classes, gain, head_gain, "rnn."))
    return st


_CACHE = {}


def stack_case(name, batch=None):
    """(args, arrays, x, ref, hits) of one of STACK_CASES (``batch``: another batch size): the restated derivation of
    ``random_gru`` at the case's gain, calibrated on [-11, 7] with inputs over [-12, 8], so the input clamps at both ends; the
    scaled-up case runs on ``steady`` features; computed once per process."""
    key = ("stack", name, batch)
    if key not in _CACHE:
        B, T, I, layers, bidir, nc, gain = STACK_CASES[name]
        B = batch or B
        args = crnn_args(layers, bidir)
        state = random_gru(np.random.default_rng(3 + len(name)), args, I, nc, gain)
        arrays = r_quantize_stack_model(state, args, I, -11.0, 7.0)
        x = features(B, T, I, steady=gain > 1.0)
        hits = {}
        ref = r_forward_stack(args, arrays, x, hits)
        assert ref["xq"].min() == -128 and ref["xq"].max() == 127, "the input does not saturate at both ends"
        _CACHE[key] = (args, arrays, x, ref, hits)
    return _CACHE[key]


def case(name, batch=None):
    """(header, arrays, x, ref) of one of CASES (``batch``: another batch size): the restated derivation of ``random_state``
    (seed 3 + len(name)), its input range calibrated on [-11, 7] with inputs over [-12, 8] and its conv maxima and f_max at NARROW
    times what the float model reaches on those inputs -- so a conv output and ``seq`` reach 127 as well as -128; computed once."""
    key = ("crnn", name, batch)
    if key not in _CACHE:
        B, F, T, layers, bidir, nc = CASES[name]
        _CACHE[key] = build(batch or B, F, T, layers, bidir, nc, seed=3 + len(name))
    return _CACHE[key]


def build(B, F, T, layers, bidir, nc, seed):
    """(header, arrays, x, ref) as ``case`` derives them, for any shape."""
    args = crnn_args(layers, bidir)
    state = random_state(args, nc, seed=seed)
    x = Q.hard_features(F, T, B)
    _, reach = float_front(state, x)
    ranges = {"x_min": -11.0, "x_max": 7.0, "a_max": [NARROW * v for v in reach["a_max"]], "f_max": NARROW * reach["f_max"]}
    arrays = r_quantize_model(state, args, F, ranges)
    ref = r_forward(args, arrays, x)
    assert ref["xq"].min() == -128 and ref["xq"].max() == 127, "the input does not saturate at both ends"
    assert any(ref["front." + c].max() == 127 and ref["front." + c].min() == -128 for c in CONVS), "no conv output clamps"
    assert ref["seq"].max() == 127 and ref["seq"].min() == -128, "seq does not reach both ends"
    return header_for(args, F, T, nc), arrays, x, ref


def clamps_reached():
    """{clamp: [stack cases that reach it]} over STACK_CASES."""
    out = {k: [] for k in CLAMPS}
    for name in STACK_CASES:
        for k, v in stack_case(name)[4].items():
            if v:
                out[k].append(name)
    return out
