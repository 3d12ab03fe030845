"""The int8 law of a ResNet18Wakeword bundle (DESIGN.md "Export", subsection "ResNet18"), restated from its text, and the cases the
ResNet18 export tests share.

Nothing here imports the export package or a kernel.  Arithmetic is int64 NumPy; a convolution is an explicit sum over taps and
output positions with an in-image test (no padding with a fill value); each tap's channel sum is a float64 matrix product of
integer-valued operands, exact below 2^53 and checked to be.  The multiplier encoding is ``q8_cases.r_encode_multiplier``, the
search over ``fractions.Fraction``.  Tensors come back NHWC, (B, H, W, C).
"""
import numpy as np

from tests.q8_cases import A_MAX_FLOOR, r_encode_multiplier, r_quantize_input, structured_features  # noqa: F401

PLANES = (64, 128, 256, 512)
TIE_CHS = (5, 13, 21, 29, 37, 45, 53, 61)     # channels the hard bundle rigs in every conv: every odd accumulator is an exact tie
ZERO_CH = 7                                   # ... all-zero weights
DS_MAX_FLOOR = 127.0 * 2.0 ** -20
# name -> (batch, F, T, num_classes): the shapes of tests/test_export_resnet_*.py
#   odd:   every stage at an odd size, 20x17 -> 10x9 -> 5x5 -> 3x3 -> 2x2
#   tiny:  the image is narrower than the stem kernel, 5x3 -> 3x2 -> 2x1 -> 1x1 -> 1x1: only the centre tap is live at the end
#   trips: 1080 stage-1 rows, so capped launches make many trips
CASES = {"odd": (2, 40, 33, 2), "tiny": (3, 9, 6, 2), "tiny3": (3, 9, 6, 3), "trips": (12, 40, 33, 2)}
HARD_SEEDS = {"odd": 0, "tiny": 1, "tiny3": 1, "trips": 0}      # seeds at which ``assert_hard`` holds (tiny: 9 of seeds 0..11 do)


def half(n):
    """floor((n + 2p - k) / 2) + 1 for (k, p) = (7, 3), (3, 1), (1, 0): torch's floor formula of every stride-2 layer here."""
    return (n - 1) // 2 + 1


def blocks():
    """[(name 'l{s}.{b}', Cin, Cout, stride, has a downsample conv)] in execution order."""
    out, cin = [], 64
    for s, planes in enumerate(PLANES):
        for b in range(2):
            first = b == 0 and s > 0
            out.append((f"l{s + 1}.{b}", cin, planes, 2 if first else 1, first))
            cin = planes
    return out


def convs():
    """[(conv name, Cout, Cin, k)] in execution order, the stem first."""
    out = [("stem", 64, 1, 7)]
    for name, cin, cout, _, down in blocks():
        out += [(name + ".conv1", cout, cin, 3)] + ([(name + ".down", cout, cin, 1)] if down else []) + [(name + ".conv2", cout, cout, 3)]
    return out


def stages():
    out = ["xq", "stem", "pool0"]
    for name, _, _, _, down in blocks():
        out += [name + ".h1"] + ([name + ".ds"] if down else []) + [name + ".out"]
    return out + ["pool", "logits"]


def stage_shapes(F, T):
    """[(H, W)] of the stem output, then of stages 1..4."""
    out = [(half(F), half(T))]
    for _ in range(4):
        out.append((half(out[-1][0]), half(out[-1][1])))
    return out


# ------------------------------------------------------------------ the law, restated
def r_R(a, m, sh):
    """R(a, m, sh) = (int64(a) m + 2^(sh-1)) >> sh, arithmetic shift (floor)."""
    a, m, sh = np.asarray(a, np.int64), np.asarray(m, np.int64), np.asarray(sh, np.int64)
    assert (np.abs(a) < 2 ** 31).all(), "the accumulator left int32"
    return np.right_shift(a * m + np.left_shift(np.int64(1), sh - 1), sh)


def r_clamp(v):
    return (np.clip(np.asarray(v, np.int64), 0, 255) - 128).astype(np.int8)        # clamp(-128 + v, -128, 127)


def r_conv(q, z, w, b, stride):
    """acc[b,ho,wo,n] = sum_{kh,kw,c} w[n,c,kh,kw] (q[b, ho s - p + kh, wo s - p + kw, c] - z) + b[n], p = k // 2; a position
    outside the image contributes nothing."""
    B, H, W, _ = q.shape
    cout, _, k, _ = w.shape
    p = k // 2
    Ho, Wo = (H + 2 * p - k) // stride + 1, (W + 2 * p - k) // stride + 1
    x = q.astype(np.float64) - float(z)
    wf = w.astype(np.float64)
    acc = np.zeros((B, Ho, Wo, cout), np.float64)
    for kh in range(k):
        for kw in range(k):
            wt = wf[:, :, kh, kw].T
            for ho in range(Ho):
                hi = ho * stride - p + kh
                if not 0 <= hi < H:
                    continue
                for wo in range(Wo):
                    wi = wo * stride - p + kw
                    if 0 <= wi < W:
                        acc[:, ho, wo] += x[:, hi, wi] @ wt
    assert (acc == np.rint(acc)).all() and (np.abs(acc) < 2.0 ** 53).all()
    return acc.astype(np.int64) + np.asarray(b, np.int64)


def r_maxpool(q):
    """(q_out, number of window positions inside the image): 3x3, stride 2, pad 1, the maximum over the positions inside."""
    B, H, W, C = q.shape
    Ho, Wo = half(H), half(W)
    out = np.empty((B, Ho, Wo, C), np.int8)
    count = np.zeros((Ho, Wo), np.int64)
    for ho in range(Ho):
        for wo in range(Wo):
            inside = [(hi, wi) for hi in range(2 * ho - 1, 2 * ho + 2) for wi in range(2 * wo - 1, 2 * wo + 2) if 0 <= hi < H and 0 <= wi < W]
            assert inside
            count[ho, wo] = len(inside)
            out[:, ho, wo] = np.stack([q[:, hi, wi] for hi, wi in inside]).max(axis=0)
    return out, count


def r_forward(arrays, x, want_acc=False):
    """Every stage of the int8 network: {stage: array}; with ``want_acc`` also ``acc/<conv>`` (int64 accumulators), ``conv/<block>``
    and ``res/<block>`` (the two rounded terms of conv2's add, int64) and ``poolcount`` (in-image positions per max-pool window)."""
    a = arrays
    x = np.asarray(x, np.float32)
    x = x[:, 0] if x.ndim == 4 else x
    out = {}
    z_x = int(a["input_zero"][0])
    xq = r_quantize_input(x, a["input_scale"][0], z_x)
    out["xq"] = xq

    def conv(name, q, z, stride):
        acc = r_conv(q, z, a[name + ".w"], a[name + ".b"], stride)
        if want_acc:
            out["acc/" + name] = acc
        return r_R(acc, a[name + ".m"], a[name + ".sh"])
    q = r_clamp(conv("stem", xq[..., None], z_x, 2))
    out["stem"] = q
    q, count = r_maxpool(q)
    out["pool0"] = q
    for name, _, _, stride, down in blocks():
        h1 = r_clamp(conv(name + ".conv1", q, -128, stride))
        out[name + ".h1"] = h1
        if down:
            res = np.clip(conv(name + ".down", q, -128, stride), -128, 127).astype(np.int8)       # signed: z = 0
            out[name + ".ds"] = res
            z_res = 0
        else:
            res, z_res = q, -128
        c2 = conv(name + ".conv2", h1, -128, 1)
        rr = r_R(res.astype(np.int64) - z_res, a[name + ".res.m"][0], a[name + ".res.sh"][0])
        q = r_clamp(c2 + rr)                                                                      # summed in int64 before the clamp
        out[name + ".out"] = q
        if want_acc:
            out["conv/" + name], out["res/" + name] = c2, rr
    S = (q.astype(np.int64) + 128).sum(axis=(1, 2))
    pool = r_clamp(r_R(S, a["pool.m"][0], a["pool.sh"][0]))
    out["pool"] = pool
    acc = (pool.astype(np.int64) + 128) @ a["fc.w"].astype(np.int64).T + a["fc.b"].astype(np.int64)
    assert (np.abs(acc) < 2 ** 31).all()
    out["logits"] = acc.astype(np.float32) * a["fc.scale"].astype(np.float32)                    # one fp32 multiply
    if want_acc:
        out["poolcount"] = count
    return out


# ------------------------------------------------------------------ the float model and the export derivation, restated
def _state_prefix(name):
    return f"resnet.layer{name[1]}.{name[3]}."


def _folded(st, conv, bn, eps):
    """BatchNorm folded in float64: W' = W g / sqrt(var + eps) per output channel, b' = beta - mean g / sqrt(var + eps)."""
    k = st[bn + ".weight"] / np.sqrt(st[bn + ".running_var"] + eps)
    return st[conv + ".weight"] * k[:, None, None, None], st[bn + ".bias"] - st[bn + ".running_mean"] * k


def float_layers(state, eps=1e-5):
    """{conv name: (W' (Cout,Cin,k,k), b' (Cout,))}, BatchNorm folded, float64; plus ``fc``."""
    st = {k: np.asarray(v, np.float64) for k, v in state.items()}
    layers = {"stem": _folded(st, "resnet.conv1", "resnet.bn1", eps)}
    for name, _, _, _, down in blocks():
        p = _state_prefix(name)
        layers[name + ".conv1"] = _folded(st, p + "conv1", p + "bn1", eps)
        layers[name + ".conv2"] = _folded(st, p + "conv2", p + "bn2", eps)
        if down:
            layers[name + ".down"] = _folded(st, p + "downsample.0", p + "downsample.1", eps)
    layers["fc"] = (st["resnet.fc.1.weight"], st["resnet.fc.1.bias"])
    return layers


def _fconv(x, w, b, stride):
    B, H, W, _ = x.shape
    k = w.shape[2]
    p = k // 2
    Ho, Wo = (H + 2 * p - k) // stride + 1, (W + 2 * p - k) // stride + 1
    xp = np.pad(x, ((0, 0), (p, p), (p, p), (0, 0)))
    y = np.zeros((B, Ho, Wo, w.shape[0])) + b
    for kh in range(k):
        for kw in range(k):
            y += xp[:, kh:kh + stride * (Ho - 1) + 1:stride, kw:kw + stride * (Wo - 1) + 1:stride] @ w[:, :, kh, kw].T
    return y


def float_forward(state, x, eps=1e-5):
    """The model's eval forward in float64 -> (logits (B,nc), {x_min, x_max, stem_max, h1_max[8], ds_max[3], out_max[8], p_max})."""
    L = float_layers(state, eps)
    x = np.asarray(x, np.float64)
    x = x[:, 0] if x.ndim == 4 else x
    r = {"x_min": float(x.min()), "x_max": float(x.max()), "h1_max": [], "ds_max": [], "out_max": []}
    h = np.maximum(_fconv(x[..., None], *L["stem"], 2), 0.0)
    r["stem_max"] = float(h.max())
    B, H, W, C = h.shape
    hp = np.pad(h, ((0, 0), (1, 1), (1, 1), (0, 0)), constant_values=-np.inf)
    Ho, Wo = half(H), half(W)
    h = np.max([hp[:, kh:kh + 2 * (Ho - 1) + 1:2, kw:kw + 2 * (Wo - 1) + 1:2] for kh in range(3) for kw in range(3)], axis=0)
    for name, _, _, stride, down in blocks():
        h1 = np.maximum(_fconv(h, *L[name + ".conv1"], stride), 0.0)
        res = h
        if down:
            res = _fconv(h, *L[name + ".down"], stride)
            r["ds_max"].append(float(np.abs(res).max()))
        h = np.maximum(_fconv(h1, *L[name + ".conv2"], 1) + res, 0.0)
        r["h1_max"].append(float(h1.max()))
        r["out_max"].append(float(h.max()))
    pool = h.mean(axis=(1, 2))
    r["p_max"] = float(pool.max())
    return pool @ L["fc"][0].T + L["fc"][1], r


def torch_ranges(state, x, dtype, eps=1e-5):
    """The calibration ranges as CPU torch computes them in ``dtype``: the module tree in eval mode, BatchNorm not folded."""
    import torch
    import torch.nn.functional as Fn
    st = {k: torch.from_numpy(np.asarray(v)).to(dtype) for k, v in state.items() if not k.endswith("num_batches_tracked")}

    def bn(p, y):
        return Fn.batch_norm(y, st[p + ".running_mean"], st[p + ".running_var"], st[p + ".weight"], st[p + ".bias"], False, 0.1, eps)
    x = torch.from_numpy(np.asarray(x)).to(dtype)
    x = x if x.dim() == 4 else x[:, None]
    r = {"x_min": float(x.min()), "x_max": float(x.max()), "h1_max": [], "ds_max": [], "out_max": []}
    with torch.no_grad():
        h = torch.relu(bn("resnet.bn1", Fn.conv2d(x, st["resnet.conv1.weight"], stride=2, padding=3)))
        r["stem_max"] = float(h.max())
        h = Fn.max_pool2d(h, 3, 2, 1)
        for name, _, _, stride, down in blocks():
            p = _state_prefix(name)
            h1 = torch.relu(bn(p + "bn1", Fn.conv2d(h, st[p + "conv1.weight"], stride=stride, padding=1)))
            res = h
            if down:
                res = bn(p + "downsample.1", Fn.conv2d(h, st[p + "downsample.0.weight"], stride=stride))
                r["ds_max"].append(float(res.abs().max()))
            h = torch.relu(bn(p + "bn2", Fn.conv2d(h1, st[p + "conv2.weight"], padding=1)) + res)
            r["h1_max"].append(float(h1.max()))
            r["out_max"].append(float(h.max()))
        r["p_max"] = float(h.mean(dim=(2, 3)).max())
    return r


def flat_ranges(r):
    """The activation ranges of a calibration in one list: stem, h1 x 8, ds x 3, out x 8, pool."""
    return [r["stem_max"]] + list(r["h1_max"]) + list(r["ds_max"]) + list(r["out_max"]) + [r["p_max"]]


def r_quantize_model(state, feature_shape, ranges, eps=1e-5):
    """The arrays of the int8 bundle of ``state`` under calibrated ``ranges``, from the text of the law."""
    L = float_layers(state, eps)
    lo, hi = min(ranges["x_min"], 0.0), max(ranges["x_max"], 0.0)
    if hi - lo <= 0:
        hi = 1.0
    s_x = np.float32((hi - lo) / 255.0)
    z_x = int(np.clip(np.rint(-128.0 - lo / float(s_x)), -128, 127))
    a = {"input_scale": np.array([s_x], np.float32), "input_zero": np.array([z_x], np.int32)}

    def scale(am):
        return max(am, A_MAX_FLOOR) / 255.0

    def one(m_sh):
        return np.array([m_sh[0]], np.int32), np.array([m_sh[1]], np.int32)

    def conv(name, s_in, s_out):
        w, b = L[name]
        amax = np.abs(w).reshape(w.shape[0], -1).max(axis=1)
        s_w = np.where(amax > 0, amax / 127.0, 1.0)
        a[name + ".w"] = np.clip(np.rint(w / s_w[:, None, None, None]), -127, 127).astype(np.int8)
        a[name + ".b"] = np.rint(b / (s_in * s_w)).astype(np.int32)
        ms = [r_encode_multiplier(s_in * s_w[c] / s_out) for c in range(w.shape[0])]
        a[name + ".m"] = np.array([m for m, _ in ms], np.int32)
        a[name + ".sh"] = np.array([s for _, s in ms], np.int32)
    s_in = scale(ranges["stem_max"])
    conv("stem", float(s_x), s_in)
    n_ds = 0
    for i, (name, _, _, _, down) in enumerate(blocks()):
        s_h1, s_out = scale(ranges["h1_max"][i]), scale(ranges["out_max"][i])
        conv(name + ".conv1", s_in, s_h1)
        s_res = s_in
        if down:
            s_res = max(ranges["ds_max"][n_ds], DS_MAX_FLOOR) / 127.0
            n_ds += 1
            conv(name + ".down", s_in, s_res)
        conv(name + ".conv2", s_h1, s_out)
        a[name + ".res.m"], a[name + ".res.sh"] = one(r_encode_multiplier(s_res / s_out))
        s_in = s_out
    H, W = stage_shapes(*feature_shape)[-1]
    s_p = scale(ranges["p_max"])
    a["pool.m"], a["pool.sh"] = one(r_encode_multiplier(s_in / (H * W * s_p)))
    w, b = L["fc"]
    amax = np.abs(w).max(axis=1)
    s_w = np.where(amax > 0, amax / 127.0, 1.0)
    a["fc.w"] = np.clip(np.rint(w / s_w[:, None]), -127, 127).astype(np.int8)
    a["fc.b"] = np.rint(b / (s_p * s_w)).astype(np.int32)
    a["fc.scale"] = (s_p * s_w).astype(np.float32)
    return a


# ------------------------------------------------------------------ cases
def header_for(F, T, num_classes=2, kind="int8"):
    return {"format": "wakeword-bundle", "version": 1, "kind": kind, "architecture": "ResNet18Wakeword", "num_classes": int(num_classes),
            "input_shape": [1, 1, F, T], "feature_shape": [F, T], "layers": [n for n, *_ in convs()] + ["pool", "fc"]}


def random_state(num_classes=2, seed=0, gain=1.0, dead=None, flat_ds=False):
    """A ResNet18Wakeword state_dict (float32 NumPy) under the reference's 122 keys.  Conv weights are normal with the variance
    2 gain^2 / fan_in, BatchNorm has weights in [0.6, 1.4], small biases and running means and running variances in [0.5, 1.5], so
    a folded BatchNorm is not the identity; one all-zero weight channel (layer1.0.conv2, ZERO_CH).  ``dead``: a conv1 name
    ('l2.1.conv1') whose weights are 0 and whose BatchNorm bias is -1, so its ReLU output is 0 everywhere -- a dead layer,
    a_max = 0.  ``flat_ds``: the downsample of l3.0 has zero weights and a zero BatchNorm shift, max |ds| = 0."""
    g = np.random.default_rng(seed)
    st = {}

    def bn(p, c):
        st[p + ".weight"], st[p + ".bias"] = g.uniform(0.6, 1.4, c), g.normal(0, 0.1, c)
        st[p + ".running_mean"], st[p + ".running_var"] = g.normal(0, 0.1, c), g.uniform(0.5, 1.5, c)
        st[p + ".num_batches_tracked"] = np.array(100, np.int64)

    def conv(p, cout, cin, k):
        st[p + ".weight"] = g.normal(0, gain * np.sqrt(2.0 / (cin * k * k)), (cout, cin, k, k))
    conv("resnet.conv1", 64, 1, 7)
    bn("resnet.bn1", 64)
    for name, cin, cout, _, down in blocks():
        p = _state_prefix(name)
        conv(p + "conv1", cout, cin, 3)
        bn(p + "bn1", cout)
        conv(p + "conv2", cout, cout, 3)
        bn(p + "bn2", cout)
        if down:
            conv(p + "downsample.0", cout, cin, 1)
            bn(p + "downsample.1", cout)
        if dead == name + ".conv1":
            st[p + "conv1.weight"][:] = 0.0
            st[p + "bn1.bias"][:], st[p + "bn1.running_mean"][:] = -1.0, 0.0
    if flat_ds:
        st["resnet.layer3.0.downsample.0.weight"][:] = 0.0
        st["resnet.layer3.0.downsample.1.bias"][:], st["resnet.layer3.0.downsample.1.running_mean"][:] = 0.0, 0.0
    st["resnet.layer1.0.conv2.weight"][ZERO_CH] = 0.0
    st["resnet.fc.1.weight"] = g.uniform(-1, 1, (num_classes, 512)) * gain * 512.0 ** -0.5
    st["resnet.fc.1.bias"] = g.uniform(-1, 1, num_classes) * 512.0 ** -0.5
    return {k: (v if v.dtype == np.int64 else np.asarray(v, np.float32)) for k, v in st.items()}


def hard_bundle(F, T, num_classes=2, seed=0):
    """(header, arrays): a bundle written integer by integer on which, with ``hard_features``, every hard spot of the law
    occurs; ``assert_hard`` checks that it does.  Weights are random and asymmetric; the channels TIE_CHS of every conv have
    m = 2^30, sh = 31 -- every odd accumulator is an exact tie -- a zero bias and weights +1, -1 and 0 in equal numbers, shuffled, so
    their accumulators are small and of both signs; channel ZERO_CH has all-zero weights.  The multipliers of a conv over
    K = k k Cin inputs sit in the binade that brings its accumulators (about 1e4 sqrt(K)) to a few hundred, so outputs clamp at
    both ends; a residual multiplier is 0.5 .. 1 for a block input (0 .. 255) and 1 .. 2 for a signed ds (-128 .. 127)."""
    g = np.random.default_rng(seed)
    a = {"input_scale": np.array([0.0625], np.float32), "input_zero": np.array([37], np.int32)}
    for name, cout, cin, k in convs():
        K = cin * k * k
        w = g.integers(-127, 128, (cout, cin, k, k)).astype(np.int8)
        b = g.integers(-20000, 20001, cout).astype(np.int32)
        m = g.integers(2 ** 30, 2 ** 31, cout).astype(np.int32)
        sh = np.full(cout, 31 + int(np.ceil(np.log2(1.0e4 * np.sqrt(K) / 400.0))), np.int32)
        for c in TIE_CHS:
            pm = np.zeros(K, np.int8)                              # a third +1, a third -1, the rest 0: were every weight odd, all
            pm[:K // 3], pm[K // 3:2 * (K // 3)] = 1, -1           # outputs that see a whole (small) image would share its parity
            w[c] = g.permutation(pm).reshape(cin, k, k)
            b[c], m[c], sh[c] = 0, 2 ** 30, 31
        w[ZERO_CH], b[ZERO_CH], m[ZERO_CH], sh[ZERO_CH] = 0, 3001, 2 ** 30 + 12345, 36
        a[name + ".w"], a[name + ".b"], a[name + ".m"], a[name + ".sh"] = w, b, m, sh
    one = lambda v: np.array([v], np.int32)       # noqa: E731
    for name, _, _, _, down in blocks():
        a[name + ".res.m"], a[name + ".res.sh"] = one(int(g.integers(2 ** 30, 2 ** 31))), one(30 if down else 31)
    H, W = stage_shapes(F, T)[-1]
    m_p, sh_p = r_encode_multiplier(1.5 / (H * W))
    a["pool.m"], a["pool.sh"] = one(m_p), one(sh_p)
    a["fc.w"] = g.integers(-127, 128, (num_classes, 512)).astype(np.int8)
    a["fc.b"] = g.integers(-5000, 5001, num_classes).astype(np.int32)
    a["fc.scale"] = (1.25e-4 * (1.0 + np.arange(num_classes))).astype(np.float32)
    return header_for(F, T, num_classes), a


def hard_features(F, T, B, seed=1):
    return np.random.default_rng(seed).uniform(-12.0, 8.0, (B, 1, F, T)).astype(np.float32)


_CACHE = {}


def hard_case(name):
    """(header, arrays, x, ref) of one of CASES at its committed seed, ``assert_hard`` run; computed once per process and shared
    (callers do not modify it)."""
    if name not in _CACHE:
        B, F, T, nc = CASES[name]
        header, arrays = hard_bundle(F, T, nc, seed=HARD_SEEDS[name])
        x = hard_features(F, T, B)
        ref = r_forward(arrays, x, want_acc=True)
        assert_hard(arrays, ref)
        _CACHE[name] = (header, arrays, x, ref)
    return _CACHE[name]


def assert_hard(arrays, ref):
    """``ref = r_forward(arrays, x, want_acc=True)``: the hard spots occur."""
    assert int(arrays["input_zero"][0]) != 0
    assert ref["xq"].min() == -128 and ref["xq"].max() == 127, "the input does not saturate at both ends"
    tie_pos = tie_neg = False
    for name, *_ in convs():
        acc = ref["acc/" + name]
        r = r_R(acc, arrays[name + ".m"], arrays[name + ".sh"])
        if name.endswith(".down"):
            assert (r < -128).any() and (r > 127).any(), f"{name}: the signed output is not clamped at both ends"
            ds = ref[name[:-5] + ".ds"]
            assert ds.min() == -128 and ds.max() == 127
        else:                                   # (conv2's own term is clamped only after the add; its range is checked all the same)
            assert (r < 0).any() and (r > 255).any(), f"{name}: outputs are not clamped at both ends"
        tie = acc[..., list(TIE_CHS)]
        odd_pos, odd_neg = bool(((tie % 2 == 1) & (tie > 0)).any()), bool(((tie % 2 == 1) & (tie < 0)).any())
        if tie.size >= 64:                      # (a 1x1 image of a small batch has too few accumulators to promise both)
            assert odd_pos and odd_neg, f"{name}: no ties of both signs"
        tie_pos, tie_neg = tie_pos or odd_pos, tie_neg or odd_neg
        assert (arrays[name + ".m"][list(TIE_CHS)] == 2 ** 30).all() and (arrays[name + ".sh"][list(TIE_CHS)] == 31).all()
        assert not arrays[name + ".w"][ZERO_CH].any()
    assert tie_pos and tie_neg
    for stage in ("stem",) + tuple(n + ".h1" for n, *_ in blocks()):
        q = ref[stage]
        assert q.min() == -128 and q.max() == 127 and np.unique(q[..., ZERO_CH]).size == 1, stage
    neg_conv, neg_res, both = False, False, False
    for name, *_ in blocks():
        c2, rr = ref["conv/" + name], ref["res/" + name]
        s = c2 + rr
        assert (s > 255).any(), f"{name}: the add never clamps from above"
        neg_conv |= bool(((c2 < 0) & (rr > 0) & (s > 0) & (s < 255)).any())
        neg_res |= bool(((c2 > 0) & (rr < 0) & (s > 0) & (s < 255)).any())
        both |= bool((s < 0).any() and (s > 255).any())
    assert neg_conv, "no block output with a negative conv term beside a positive residual term"
    assert neg_res, "no block output with a positive conv term beside a negative residual term"
    assert both, "no block output at which both clamps of the add are hit"
    # a max-pool window partly outside the image, where a fill value of 0 would win: the stem's ZERO_CH output is one negative constant
    count = ref["poolcount"]
    border = count < 9
    assert border.any() and count.min() >= 1
    zc = ref["pool0"][..., ZERO_CH]
    assert np.unique(zc).size == 1 and zc.flat[0] < 0 and zc.flat[0] == ref["stem"][..., ZERO_CH].flat[0]
    assert np.unique(ref["pool"]).size > 8
