"""The int8 law of DESIGN.md 5.6, subsection "MobileNetV3", restated for the tests: explicit sums over taps with in-image tests, int64
NumPy, multipliers found by a search over exact Fractions, the Hardswish table recomputed here entry by entry.  Nothing of the
package's interpreter or quantiser is imported: ``wakeword_trainer_home_amd.export.reference`` / ``quantize`` and the kernels are each
held to THIS text.

Two families of whole-model cases.  ``model``: a seeded ``MobileNetV3Wakeword`` state (BatchNorm running statistics non-trivial),
calibrated by the float64 walk below on the case's own inputs at NARROW of their ranges, quantised by the restated quantiser.
``hard``: synthetic arrays -- random int8 weights with an all-zero channel, random tables with both ends present, multipliers tuned
layer by layer so that every epilogue hits both clamps (``assert_hard`` says where), gates of 0 and 255, residuals that push the sum
past both clamps -- on inputs holding NaN and +-inf.  The stage tensors of a case are also the inputs of the per-layer GPU tests."""
import math
from fractions import Fraction

import numpy as np

from tests.q8_cases import r_quantize_input, r_round_half_even, structured_features  # noqa: F401

CONF = ((16, 3, 16, 16, True, "RE", 2), (16, 3, 72, 24, False, "RE", 2), (24, 3, 88, 24, False, "RE", 1),
        (24, 5, 96, 40, True, "HS", 2), (40, 5, 240, 40, True, "HS", 1), (40, 5, 240, 40, True, "HS", 1),
        (40, 5, 120, 48, True, "HS", 1), (48, 5, 144, 48, True, "HS", 1), (48, 5, 288, 96, True, "HS", 2),
        (96, 5, 576, 96, True, "HS", 1), (96, 5, 576, 96, True, "HS", 1))
SQUEEZE = (8, 0, 0, 24, 64, 64, 32, 40, 72, 144, 144)        # make_divisible(exp // 4, 8) of the blocks with squeeze-excitation
STEM, LAST, HIDDEN = 16, 576, 1024
A_MAX_FLOOR, S_MAX_FLOOR = 255.0 * 2.0 ** -20, 127.0 * 2.0 ** -20
NARROW = 0.6
ZERO_CH = 3                                                   # the all-zero weight channel of every layer of a hard bundle
# name: (family, B, F, T, num_classes, seed).  (16,24): stages 8x12, 4x6, 2x3, 1x2, 1x1 -- 5x5 windows larger than the image, HW = 1
# pools; (13,21): odd at every stride-2 layer; B = 3: pixel counts no multiples of 16, tiles span images; trips: 40 images make every
# persistent kernel take several passes under a grid cap of 1 or 2 (the 1x1 stage's projection has 3 x 2 items for 4 waves).
CASES = {"tiny": ("model", 3, 16, 24, 2, 0), "odd": ("model", 3, 13, 21, 3, 1), "dead": ("model", 2, 16, 24, 2, 2),
         "hard_tiny": ("hard", 3, 16, 24, 2, 3), "hard_odd": ("hard", 3, 13, 21, 3, 4), "trips": ("hard", 40, 16, 24, 2, 5)}
DEAD = {"b1.expand": [0.0, 0.0], "b2.out": [0.0, 0.0], "b4.dw.u": [0.0, 0.0]}      # ranges the dead case overrides: the floors


def half(n):
    return (n - 1) // 2 + 1


def blocks(F, T):
    hw, out = (half(F), half(T)), []
    for (cin, k, exp, cout, se, act, stride), sq in zip(CONF, SQUEEZE):
        nxt = (half(hw[0]), half(hw[1])) if stride == 2 else hw
        out.append(dict(cin=cin, k=k, exp=exp, cout=cout, se=sq if se else 0, hs=act == "HS", stride=stride, expand=exp != cin,
                        res=stride == 1 and cin == cout, hw_in=hw, hw=nxt))
        hw = nxt
    return out


def range_names():
    out = ["stem.u", "stem"]
    for i, b in enumerate(blocks(1, 1)):
        for layer in (["expand"] if b["expand"] else []) + ["dw"]:
            out += ([f"b{i}.{layer}.u"] if b["hs"] else []) + [f"b{i}.{layer}"]
        out += ([f"b{i}.h"] if b["se"] else []) + [f"b{i}.out"]
    return out + ["last.u", "last", "cls0.u", "hidden"]


def stages():
    out = ["xq", "stem"]
    for i, b in enumerate(blocks(1, 1)):
        out += ([f"b{i}.expand"] if b["expand"] else []) + [f"b{i}.dw"]
        out += [f"b{i}.{s}" for s in ("pool", "h", "gate", "y")] if b["se"] else []
        out.append(f"b{i}.out")
    return out + ["last", "pool", "hidden", "logits"]


# ------------------------------------------------------------------ the law
def r_encode_multiplier(r):
    """The (m, sh), 2^30 <= m < 2^31, 1 <= sh <= 62, with m 2^-sh nearest to r, by exact Fractions: only the shifts next to the
    binary exponent of r can put m in range, so the search of tests/q8_cases.py is cut to those (thousands of channels per case)."""
    assert math.isfinite(r) and r > 0
    R, best, e = Fraction(r), None, math.frexp(r)[1]
    for sh in range(max(1, 29 - e), min(62, 33 - e) + 1):
        m = r_round_half_even(R * 2 ** sh)
        if 2 ** 30 <= m < 2 ** 31:
            err = abs(Fraction(m, 2 ** sh) - R)
            if best is None or err < best[0]:
                best = (err, m, sh)
    return best[1], best[2]


def r_R(a, m, sh):
    a = np.asarray(a, np.int64)
    assert (np.abs(a) < 2 ** 31).all(), "an accumulator left int32"
    m, sh = np.asarray(m, np.int64), np.asarray(sh, np.int64)
    return np.right_shift(a * m + np.left_shift(np.int64(1), sh - 1), sh)


def r_clamp(v):
    return np.clip(v, -128, 127).astype(np.int8)


def r_window(q, z, w, k, stride):
    """acc[b,ho,wo,c] = sum over the taps whose source pixel lies inside the image of w[c, kh k + kw] (q[b,hi,wi,c] - z); q has the
    layer's channels, or one (the stem)."""
    B, H, W, _ = q.shape
    p, Ho, Wo = k // 2, (H - 1) // stride + 1, (W - 1) // stride + 1
    d, w = q.astype(np.int64) - z, w.astype(np.int64)
    acc = np.zeros((B, Ho, Wo, w.shape[0]), np.int64)
    for ho in range(Ho):
        for wo in range(Wo):
            for kh in range(k):
                hi = ho * stride - p + kh
                if not 0 <= hi < H:
                    continue
                for kw in range(k):
                    wi = wo * stride - p + kw
                    if 0 <= wi < W:
                        acc[:, ho, wo, :] += w[:, kh * k + kw] * d[:, hi, wi, :]
    return acc


def r_matmul(q, z, w):
    return (q.astype(np.int64) - z) @ w.astype(np.int64).T


def r_table(s_u, z_u, s_out, z_out):
    t = []
    for i in range(256):
        v = (i - 128 - z_u) * float(s_u)
        hs = v * min(max(v + 3.0, 0.0), 6.0) / 6.0
        t.append(min(max(int(np.rint(hs / float(s_out))) + z_out, -128), 127))
    return np.array(t, np.int8)


def r_forward(arrays, x, F, T, want=False, tune=None):
    """Every stage tensor of the law on features ``x``; ``want`` adds ``acc/<layer>`` and ``u/<layer>``.  ``tune(name, acc)`` is called
    before a layer's accumulator is requantised (the hard bundles set its multiplier there)."""
    a, out = arrays, {}

    def finish(name, acc, kind, res=None):
        acc = acc + a[name + ".b"].astype(np.int64)
        if tune:
            tune(name, acc)
        if want:
            out["acc/" + name] = acc
        r = r_R(acc, a[name + ".m"], a[name + ".sh"])
        if kind == "relu":
            return r_clamp(r - 128), -128
        if kind == "signed":
            return r_clamp(r if res is None else r + res), 0
        u = np.clip(int(a[name + ".zu"][0]) + r, -128, 127)
        if want:
            out["u/" + name] = u.astype(np.int8)
        return a[name + ".tab"][u + 128], int(a[name + ".zo"][0])

    def pool(q, z, name):
        S = (q.astype(np.int64) - z).sum(axis=(1, 2))
        return r_clamp(z + r_R(S, a[name + ".m"][0], a[name + ".sh"][0]))
    x = np.asarray(x, np.float32).reshape(-1, F, T)
    z_x = int(a["input_zero"][0])
    xq = r_quantize_input(x, a["input_scale"][0], z_x)
    out["xq"] = xq
    q, z = finish("stem", r_window(xq[..., None], z_x, a["stem.w"], 3, 2), "hs")
    out["stem"] = q
    for i, b in enumerate(blocks(F, T)):
        p, act, q_in = f"b{i}.", "hs" if b["hs"] else "relu", q
        if b["expand"]:
            q, z = finish(p + "expand", r_matmul(q, z, a[p + "expand.w"]), act)
            out[p + "expand"] = q
        q, z = finish(p + "dw", r_window(q, z, a[p + "dw.w"], b["k"], b["stride"]), act)
        out[p + "dw"] = q
        if b["se"]:
            sq = pool(q, z, p + "pool")
            h, _ = finish(p + "fc1", r_matmul(sq, z, a[p + "fc1.w"]), "relu")
            acc2 = r_matmul(h, -128, a[p + "fc2.w"]) + a[p + "fc2.b"].astype(np.int64)
            if tune:
                tune(p + "fc2", acc2)
            gate = np.clip(r_R(acc2, a[p + "fc2.m"], a[p + "fc2.sh"]), 0, 255)
            q = r_clamp(z + r_R((q.astype(np.int64) - z) * gate[:, None, None, :], a[p + "gate.m"][0], a[p + "gate.sh"][0]))
            out[p + "pool"], out[p + "h"], out[p + "gate"], out[p + "y"] = sq, h, gate.astype(np.uint8), q
            if want:
                out["acc/" + p + "fc2"] = acc2
        res = r_R(q_in, a[p + "res.m"][0], a[p + "res.sh"][0]) if b["res"] else None
        q, z = finish(p + "project", r_matmul(q, z, a[p + "project.w"]), "signed", res)
        out[p + "out"] = q
    q, z = finish("last", r_matmul(q, 0, a["last.w"]), "hs")
    out["last"] = q
    pq = pool(q, z, "pool")
    out["pool"] = pq
    hid, z_h = finish("cls0", r_matmul(pq, z, a["cls0.w"]), "hs")
    out["hidden"] = hid
    acc = r_matmul(hid, z_h, a["fc.w"]) + a["fc.b"].astype(np.int64)
    if want:
        out["acc/fc"] = acc
    out["logits"] = acc.astype(np.float32) * a["fc.scale"].astype(np.float32)
    return out


# ------------------------------------------------------------------ the float model (float64 NumPy) and its ranges
def _fold(st, p, eps):
    k = st[p + ".1.weight"] / np.sqrt(st[p + ".1.running_var"] + eps)
    w = st[p + ".0.weight"]
    return w.reshape(w.shape[0], -1) * k[:, None], st[p + ".1.bias"] - st[p + ".1.running_mean"] * k


def float_layers(state, eps=1e-3):
    """{law name: (W' (Cout, K), b')} with BatchNorm folded, in float64; the squeeze-excitation's and the head's as they are."""
    st = {k: np.asarray(v, np.float64) for k, v in state.items() if np.asarray(v).dtype.kind == "f"}
    pre, L = "mobilenet.features.", {}
    L["stem"] = _fold(st, pre + "0", eps)
    for i, b in enumerate(blocks(1, 1)):
        p, j = f"{pre}{i + 1}.block.", 0
        if b["expand"]:
            L[f"b{i}.expand"], j = _fold(st, p + "0", eps), 1
        L[f"b{i}.dw"] = _fold(st, f"{p}{j}", eps)
        j += 1
        if b["se"]:
            for fc in ("fc1", "fc2"):
                w = st[f"{p}{j}.{fc}.weight"]
                L[f"b{i}.{fc}"] = (w.reshape(w.shape[0], -1), st[f"{p}{j}.{fc}.bias"])
            j += 1
        L[f"b{i}.project"] = _fold(st, f"{p}{j}", eps)
    L["last"] = _fold(st, pre + "12", eps)
    L["cls0"] = (st["mobilenet.classifier.0.weight"], st["mobilenet.classifier.0.bias"])
    L["fc"] = (st["mobilenet.classifier.3.weight"], st["mobilenet.classifier.3.bias"])
    return L


def _fwindow(x, w, k, stride):
    B, H, W, _ = x.shape
    p, Ho, Wo = k // 2, (H - 1) // stride + 1, (W - 1) // stride + 1
    d = np.pad(x, ((0, 0), (p, p), (p, p), (0, 0)))
    acc = np.zeros((B, Ho, Wo, w.shape[0]))
    for kh in range(k):
        for kw in range(k):
            acc += d[:, kh:kh + stride * (Ho - 1) + 1:stride, kw:kw + stride * (Wo - 1) + 1:stride, :] * w[:, kh * k + kw]
    return acc


def _hs(v):
    return v * np.clip(v + 3.0, 0.0, 6.0) / 6.0


def float_walk(state, x, eps=1e-3):
    """The eval forward in float64 -> ({x_min, x_max, ranges {name: [min, max]}}, logits (B, num_classes) float64)."""
    L = float_layers(state, eps)
    x = np.asarray(x, np.float64)
    x = x.reshape(x.shape[0], x.shape[-2], x.shape[-1], 1)
    rng = {}

    def see(name, t):
        rng[name] = [float(t.min()), float(t.max())]
        return t

    def act(name, pre, hs):
        return see(name, _hs(see(name + ".u", pre))) if hs else see(name, np.maximum(pre, 0.0))
    w, b = L["stem"]
    h = act("stem", _fwindow(x, w, 3, 2) + b, True)
    for i, blk in enumerate(blocks(1, 1)):
        p, h_in = f"b{i}.", h
        if blk["expand"]:
            w, b = L[p + "expand"]
            h = act(p + "expand", h @ w.T + b, blk["hs"])
        w, b = L[p + "dw"]
        h = act(p + "dw", _fwindow(h, w, blk["k"], blk["stride"]) + b, blk["hs"])
        if blk["se"]:
            (w1, b1), (w2, b2) = L[p + "fc1"], L[p + "fc2"]
            hid = see(p + "h", np.maximum(h.mean(axis=(1, 2)) @ w1.T + b1, 0.0))
            h = h * (np.clip(hid @ w2.T + b2 + 3.0, 0.0, 6.0) / 6.0)[:, None, None, :]
        w, b = L[p + "project"]
        h = see(p + "out", h @ w.T + b + (h_in if blk["res"] else 0.0))
    w, b = L["last"]
    h = act("last", h @ w.T + b, True)
    w, b = L["cls0"]
    hid = _hs(see("cls0.u", h.mean(axis=(1, 2)) @ w.T + b))
    see("hidden", hid)
    w, b = L["fc"]
    return {"x_min": float(x.min()), "x_max": float(x.max()), "ranges": rng}, hid @ w.T + b


# ------------------------------------------------------------------ the quantiser, from the text of the law
def r_asym(lo, hi):
    lo, hi = min(float(lo), 0.0), max(float(hi), 0.0)
    if hi - lo <= 0:
        hi = 1.0
    s = np.float32((hi - lo) / 255.0)
    return s, int(np.clip(np.rint(-128.0 - lo / float(s)), -128, 127))


def r_quantize_model(state, feature_shape, cal, eps=1e-3):
    L, rng = float_layers(state, eps), cal["ranges"]
    s_x, z_x = r_asym(cal["x_min"], cal["x_max"])
    a = {"input_scale": np.array([s_x], np.float32), "input_zero": np.array([z_x], np.int32)}

    def one(name, r):
        m, sh = r_encode_multiplier(r)
        a[name + ".m"], a[name + ".sh"] = np.array([m], np.int32), np.array([sh], np.int32)

    def layer(name, s_in, kind, out_name=None, shift=0.0):
        w, b = L[name]
        amax = np.abs(w).max(axis=1)
        s_w = np.where(amax > 0, amax / 127.0, 1.0)
        r = rng.get(out_name or name)
        if kind == "hs":
            u = rng[name + ".u"]
            s_u, z_u = r_asym(max(u[0], -3.0), u[1])
            s_o, z_o = r_asym(r[0], r[1])
            a[name + ".zu"], a[name + ".zo"] = np.array([z_u], np.int32), np.array([z_o], np.int32)
            a[name + ".tab"] = r_table(s_u, z_u, s_o, z_o)
            s_t, s_o = float(s_u), float(s_o)
        elif kind == "relu":
            s_t = s_o = max(r[1], A_MAX_FLOOR) / 255.0
        elif kind == "signed":
            s_t = s_o = max(abs(r[0]), abs(r[1]), S_MAX_FLOOR) / 127.0
        else:
            s_t, s_o = 6.0 / 255.0, 1.0 / 255.0
        a[name + ".w"] = np.clip(np.rint(w / s_w[:, None]), -127, 127).astype(np.int8)
        a[name + ".b"] = np.rint((b + shift) / (s_in * s_w)).astype(np.int32)
        ms = [r_encode_multiplier(s_in * s_w[c] / s_t) for c in range(w.shape[0])]
        a[name + ".m"] = np.array([m for m, _ in ms], np.int32)
        a[name + ".sh"] = np.array([s for _, s in ms], np.int32)
        return s_o
    s = layer("stem", float(s_x), "hs")
    bl = blocks(*feature_shape)
    for i, b in enumerate(bl):
        p, kind, s_res = f"b{i}.", "hs" if b["hs"] else "relu", s
        if b["expand"]:
            s = layer(p + "expand", s, kind)
        s = layer(p + "dw", s, kind)
        if b["se"]:
            hw = b["hw"][0] * b["hw"][1]
            one(p + "pool", 1.0 / hw)
            a[p + "pool.hw"] = np.array([hw], np.int32)
            s_h = layer(p + "fc1", s, "relu", p + "h")
            layer(p + "fc2", s_h, "gate", shift=3.0)
            one(p + "gate", 1.0 / 255.0)
        s = layer(p + "project", s, "signed", p + "out")
        if b["res"]:
            one(p + "res", s_res / s)
    s = layer("last", s, "hs")
    hw = bl[-1]["hw"][0] * bl[-1]["hw"][1]
    one("pool", 1.0 / hw)
    a["pool.hw"] = np.array([hw], np.int32)
    s_h = layer("cls0", s, "hs", "hidden")
    w, b = L["fc"]
    amax = np.abs(w).max(axis=1)
    s_w = np.where(amax > 0, amax / 127.0, 1.0)
    a["fc.w"] = np.clip(np.rint(w / s_w[:, None]), -127, 127).astype(np.int8)
    a["fc.b"] = np.rint(b / (s_h * s_w)).astype(np.int32)
    a["fc.scale"] = (s_h * s_w).astype(np.float32)
    return a


# ------------------------------------------------------------------ cases
def header_for(F, T, num_classes=2, kind="int8"):
    return {"format": "wakeword-bundle", "version": 1, "kind": kind, "architecture": "mobilenetv3", "num_classes": num_classes,
            "input_shape": [1, 1, F, T], "layers": ["stem"], "feature_shape": [F, T]}


def state_shapes(num_classes=2):
    """[(key, shape)] of ``MobileNetV3Wakeword.state_dict()``, in its order."""
    out, pre = [], "mobilenet.features."

    def cba(p, cout, cin, k):
        out.append((p + ".0.weight", (cout, cin, k, k)))
        out.extend((f"{p}.1.{s}", (cout,)) for s in ("weight", "bias", "running_mean", "running_var"))
        out.append((p + ".1.num_batches_tracked", ()))
    cba(pre + "0", STEM, 1, 3)
    for i, b in enumerate(blocks(1, 1)):
        p, j = f"{pre}{i + 1}.block.", 0
        if b["expand"]:
            cba(p + "0", b["exp"], b["cin"], 1)
            j = 1
        cba(f"{p}{j}", b["exp"], 1, b["k"])
        j += 1
        if b["se"]:
            out += [(f"{p}{j}.fc1.weight", (b["se"], b["exp"], 1, 1)), (f"{p}{j}.fc1.bias", (b["se"],)),
                    (f"{p}{j}.fc2.weight", (b["exp"], b["se"], 1, 1)), (f"{p}{j}.fc2.bias", (b["exp"],))]
            j += 1
        cba(f"{p}{j}", b["cout"], b["exp"], 1)
    cba(pre + "12", LAST, CONF[-1][3], 1)
    return out + [("mobilenet.classifier.0.weight", (HIDDEN, LAST)), ("mobilenet.classifier.0.bias", (HIDDEN,)),
                  ("mobilenet.classifier.3.weight", (num_classes, HIDDEN)), ("mobilenet.classifier.3.bias", (num_classes,))]


def random_state(num_classes=2, seed=0, gain=1.0):
    """A seeded float32 state: He-scaled weights times ``gain``, BatchNorm scales in [0.6, 1.4], shifts and running means ~ N(0, 0.2),
    running variances in [0.5, 1.5] -- running statistics that a folding bug cannot hide behind."""
    g, st = np.random.default_rng(seed), {}
    for key, shape in state_shapes(num_classes):
        leaf = key.rsplit(".", 1)[1]
        if leaf == "num_batches_tracked":
            st[key] = np.array(7, np.int64)
        elif leaf == "running_var":
            st[key] = g.uniform(0.5, 1.5, shape).astype(np.float32)
        elif leaf == "running_mean" or (leaf == "bias" and len(shape) == 1):
            st[key] = g.normal(0.0, 0.2, shape).astype(np.float32)
        elif len(shape) == 1:
            st[key] = g.uniform(0.6, 1.4, shape).astype(np.float32)
        else:
            fan_in = int(np.prod(shape[1:]))
            st[key] = (g.normal(0.0, 1.0, shape) * gain * math.sqrt(2.0 / fan_in)).astype(np.float32)
    return st


def hard_bundle(F, T, x, num_classes=2, seed=0):
    """Synthetic arrays of a whole bundle, built layer by layer while the law runs on ``x``: every multiplier is set from the layer's
    own accumulators so that its epilogue reaches both clamps (see ``assert_hard``)."""
    g = np.random.default_rng(seed)
    a = {"input_scale": np.array([0.07], np.float32), "input_zero": np.array([37], np.int32)}

    def one(name, r):
        m, sh = r_encode_multiplier(r)
        a[name + ".m"], a[name + ".sh"] = np.array([m], np.int32), np.array([sh], np.int32)

    def layer(name, cout, k_in, hs=False):
        w = g.integers(-127, 128, (cout, k_in)).astype(np.int8)
        w[ZERO_CH] = 0
        a[name + ".w"] = w
        a[name + ".b"] = g.integers(-400 * k_in, 400 * k_in + 1, cout).astype(np.int32)
        a[name + ".m"], a[name + ".sh"] = np.full(cout, 2 ** 30, np.int32), np.full(cout, 31, np.int32)
        if hs:
            zu, zo = int(g.integers(-60, 61)), int(g.integers(-100, 101))
            tab = g.integers(-128, 128, 256).astype(np.int8)
            tab[0], tab[255], tab[1], tab[254], tab[zu + 128] = -128, 127, 127, -128, zo
            a[name + ".zu"], a[name + ".zo"], a[name + ".tab"] = np.array([zu], np.int32), np.array([zo], np.int32), tab
    layer("stem", STEM, 9, True)
    bl = blocks(F, T)
    for i, b in enumerate(bl):
        p = f"b{i}."
        if b["expand"]:
            layer(p + "expand", b["exp"], b["cin"], b["hs"])
        layer(p + "dw", b["exp"], b["k"] ** 2, b["hs"])
        if b["se"]:
            hw = b["hw"][0] * b["hw"][1]
            one(p + "pool", 1.0 / hw)
            a[p + "pool.hw"] = np.array([hw], np.int32)
            layer(p + "fc1", b["se"], b["exp"])
            layer(p + "fc2", b["exp"], b["se"])
            one(p + "gate", 1.0 / 255.0)
        layer(p + "project", b["cout"], b["exp"])
        if b["res"]:
            one(p + "res", 1.7)
    layer("last", LAST, CONF[-1][3], True)
    hw = bl[-1]["hw"][0] * bl[-1]["hw"][1]
    one("pool", 1.0 / hw)
    a["pool.hw"] = np.array([hw], np.int32)
    layer("cls0", HIDDEN, LAST, True)
    a["fc.w"] = g.integers(-127, 128, (num_classes, HIDDEN)).astype(np.int8)
    a["fc.b"] = g.integers(-10 ** 6, 10 ** 6, num_classes).astype(np.int32)
    a["fc.scale"] = g.uniform(1e-6, 1e-5, num_classes).astype(np.float32)

    def tune(name, acc):
        # the largest |accumulator| of a channel maps to 300 (ReLU, Hardswish, signed) or 450 (the gate): past 127 / 255 on one side,
        # and, the accumulators being of both signs, past the other
        top = np.abs(acc).reshape(-1, acc.shape[-1]).max(axis=0).astype(np.float64)
        want = 450.0 if name.endswith("fc2") else 300.0
        ms = [r_encode_multiplier(want / max(t, 1.0)) for t in top]
        a[name + ".m"] = np.array([m for m, _ in ms], np.int32)
        a[name + ".sh"] = np.array([s for _, s in ms], np.int32)
    r_forward(a, x, F, T, tune=tune)
    return a


def hard_features(B, F, T, seed):
    x = structured_features(B, F, T, seed=seed)
    x[0, 0, 0, 0], x[0, 0, 1, 2], x[B - 1, 0, 2, 1] = np.nan, np.inf, -np.inf
    return x


def assert_hard(F, T, ref):
    """Both clamps in every epilogue of the last stage with more than a handful of values, u at both ends, gates of 0 and 255."""
    bl = blocks(F, T)
    for i, b in enumerate(bl):
        p = f"b{i}."
        big = b["hw"][0] * b["hw"][1] > 1
        if b["se"]:
            g = ref[p + "gate"]
            assert g.min() == 0 and g.max() == 255, p + "gate"
        o = ref[p + "out"]
        assert o.min() == -128 and o.max() == 127, p + "out"
        if not b["hs"]:
            assert ref[p + "dw"].min() == -128 and (ref[p + "dw"].max() == 127 or not big), p + "dw"
    for name in ["stem", "last", "cls0"] + [f"b{i}.dw" for i, b in enumerate(bl) if b["hs"]]:
        u = ref["u/" + name]
        assert u.min() == -128 and u.max() == 127, name
    assert ref["xq"].min() == -128 and ref["xq"].max() == 127


_CACHE = {}


def case(name):
    """-> (header, arrays, x (B,1,F,T) float32, ref): ``ref`` holds every stage tensor of the restated law, with accumulators and u."""
    if name not in _CACHE:
        family, B, F, T, nc, seed = CASES[name]
        if family == "hard":
            x = hard_features(B, F, T, seed)
            arrays = hard_bundle(F, T, x, nc, seed)
        else:
            x = structured_features(B, F, T, seed=seed)
            state = random_state(nc, seed)
            cal, _ = float_walk(state, x)
            cal["ranges"] = {k: [NARROW * v[0], NARROW * v[1]] for k, v in cal["ranges"].items()}
            if name == "dead":
                cal["ranges"].update(DEAD)
            arrays = r_quantize_model(state, (F, T), cal)
        ref = r_forward(arrays, x, F, T, want=True)
        if family == "hard":
            assert_hard(F, T, ref)
        _CACHE[name] = (header_for(F, T, nc), arrays, x, ref)
    return _CACHE[name]


def dw_layer_case(k, stride, H, W, C, hs, seed=0, B=2):
    """One synthetic depthwise layer on a (B,H,W,C) tensor: -> (q, z, arrays of layer 'dw', restated output).  Both clamps are hit
    where the tensor has enough values."""
    g = np.random.default_rng(seed)
    q, z = g.integers(-128, 128, (B, H, W, C)).astype(np.int8), int(g.integers(-128, 128))
    w = g.integers(-127, 128, (C, k * k)).astype(np.int8)
    w[ZERO_CH] = 0
    a = {"dw.w": w, "dw.b": g.integers(-3000, 3001, C).astype(np.int32)}
    acc = r_window(q, z, w, k, stride) + a["dw.b"]
    top = np.abs(acc).reshape(-1, C).max(axis=0).astype(np.float64)
    ms = [r_encode_multiplier(300.0 / max(t, 1.0)) for t in top]
    a["dw.m"], a["dw.sh"] = np.array([m for m, _ in ms], np.int32), np.array([s for _, s in ms], np.int32)
    r = r_R(acc, a["dw.m"], a["dw.sh"])
    if not hs:
        return q, z, a, r_clamp(r - 128)
    zu = int(g.integers(-60, 61))
    tab = g.integers(-128, 128, 256).astype(np.int8)
    tab[0], tab[255] = -128, 127
    a["dw.zu"], a["dw.tab"] = np.array([zu], np.int32), tab
    return q, z, a, tab[np.clip(zu + r, -128, 127) + 128]
