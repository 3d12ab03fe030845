"""The int8 law of a TCNWakeword bundle (DESIGN.md "Export", subsection "TCN"), restated from its text, and the cases the TCN
export tests share.

Nothing here imports the export package or a kernel.  Arithmetic is int64 NumPy; a convolution is an explicit sum over taps and
times with a ``t' >= 0`` test (no padding with a fill value); each tap's channel sum is a float64 matrix product of
integer-valued operands, exact below 2^53 and checked to be.  The multiplier encoding is ``q8_cases.r_encode_multiplier``, the
search over ``fractions.Fraction``.  Tensors come back as (B, T, C), unpadded.
"""
import numpy as np

from tests.q8_cases import A_MAX_FLOOR, r_encode_multiplier, r_quantize_input, structured_features  # noqa: F401

TIE_CH, ZERO_CH = 5, 7                 # channels the hard bundle rigs in every conv: exact rounding ties / all-zero weights
# (B, F, T, num_channels, kernel_size): the shapes of tests/test_export_tcn_*.py and the seeds at which ``assert_hard`` holds
SHAPES = {"identity": (2, 12, 5, [16, 16, 16], 3), "default": (3, 40, 45, [64, 128, 256], 3), "small": (5, 40, 70, [32, 48], 2)}
HARD_SEEDS = {"identity": 2, "default": 0, "small": 0}


def tcn_args(F, num_channels, k):
    return {"input_size": int(F), "num_channels": [int(c) for c in num_channels], "kernel_size": int(k)}


def block_convs(args):
    """[(block, conv name, Cin, Cout, taps, dilation)] in execution order; ``down`` only where the channel count changes."""
    out, cin = [], args["input_size"]
    for i, c in enumerate(args["num_channels"]):
        out += [(i, "conv1", cin, c, args["kernel_size"], 2 ** i), (i, "conv2", c, c, args["kernel_size"], 2 ** i)]
        if cin != c:
            out.append((i, "down", cin, c, 1, 1))
        cin = c
    return out


def stages(args):
    return ["xq"] + [f"b{i}.{s}" for i in range(len(args["num_channels"])) for s in ("h1", "h2", "out")] + ["pool", "logits"]


# ------------------------------------------------------------------ the law, restated
def r_R(a, m, sh):
    """R(a, m, sh) = (int64(a) m + 2^(sh-1)) >> sh, arithmetic shift (floor)."""
    a, m, sh = np.asarray(a, np.int64), np.asarray(m, np.int64), np.asarray(sh, np.int64)
    assert (np.abs(a) < 2 ** 31).all(), "the accumulator left int32"
    return np.right_shift(a * m + np.left_shift(np.int64(1), sh - 1), sh)


def r_clamp(v):
    return (np.clip(np.asarray(v, np.int64), 0, 255) - 128).astype(np.int8)        # clamp(-128 + v, -128, 127)


def r_conv(q, z, w, b, d):
    """acc[b,t,n] = sum_j sum_c w[n,c,j] (q[b, t - (k-1-j) d, c] - z) + b[n]; a source time below 0 contributes nothing."""
    B, T, _ = q.shape
    cout, _, k = w.shape
    x = q.astype(np.float64) - float(z)
    wf = w.astype(np.float64)
    acc = np.zeros((B, T, cout), np.float64)
    for j in range(k):
        for t in range(T):
            ts = t - (k - 1 - j) * d
            if ts >= 0:
                acc[:, t] += x[:, ts] @ wf[:, :, j].T
    assert (acc == np.rint(acc)).all() and (np.abs(acc) < 2.0 ** 53).all()
    return acc.astype(np.int64) + np.asarray(b, np.int64)


def r_forward(args, arrays, x, want_acc=False):
    """Every stage of the int8 network: {stage: array}; with ``want_acc`` also ``acc/b{i}.conv1|conv2|down`` (int64 accumulators),
    ``skip/b{i}`` and ``add/b{i}`` (the two rounded terms of the add, int64)."""
    a = arrays
    x = np.asarray(x, np.float32)
    x = x[:, 0] if x.ndim == 4 else x
    out = {}
    z = int(a["input_zero"][0])
    q = np.ascontiguousarray(r_quantize_input(x, a["input_scale"][0], z).transpose(0, 2, 1))      # (B, T, F)
    out["xq"] = q
    cin = args["input_size"]
    for i, c in enumerate(args["num_channels"]):
        d, p = 2 ** i, f"b{i}."
        acc1 = r_conv(q, z, a[p + "conv1.w"], a[p + "conv1.b"], d)
        h1 = r_clamp(r_R(acc1, a[p + "conv1.m"], a[p + "conv1.sh"]))
        acc2 = r_conv(h1, -128, a[p + "conv2.w"], a[p + "conv2.b"], d)
        h2 = r_clamp(r_R(acc2, a[p + "conv2.m"], a[p + "conv2.sh"]))
        if cin != c:
            accd = r_conv(q, z, a[p + "down.w"], a[p + "down.b"], 1)
            skip = r_R(accd, a[p + "down.m"], a[p + "down.sh"])
        else:
            accd = None
            skip = r_R(q.astype(np.int64) - z, a[p + "skip.m"][0], a[p + "skip.sh"][0])
        add = r_R(h2.astype(np.int64) + 128, a[p + "add.m"][0], a[p + "add.sh"][0])
        q, z, cin = r_clamp(skip + add), -128, c
        out[p + "h1"], out[p + "h2"], out[p + "out"] = h1, h2, q
        if want_acc:
            out["acc/" + p + "conv1"], out["acc/" + p + "conv2"], out["skip/b%d" % i], out["add/b%d" % i] = acc1, acc2, skip, add
            if accd is not None:
                out["acc/" + p + "down"] = accd
    S = (q.astype(np.int64) + 128).sum(axis=1)
    pool = r_clamp(r_R(S, a["pool.m"][0], a["pool.sh"][0]))
    out["pool"] = pool
    acc = (pool.astype(np.int64) + 128) @ a["fc.w"].astype(np.int64).T + a["fc.b"].astype(np.int64)
    assert (np.abs(acc) < 2 ** 31).all()
    out["logits"] = acc.astype(np.float32) * a["fc.scale"].astype(np.float32)                    # one fp32 multiply
    return out


# ------------------------------------------------------------------ the float model and the export derivation, restated
def _fconv(x, w, b, d):
    B, T, _ = x.shape
    k = w.shape[2]
    y = np.zeros((B, T, w.shape[0])) + b
    for j in range(k):
        off = (k - 1 - j) * d
        if off < T:
            y[:, off:] += x[:, :T - off] @ w[:, :, j].T
    return y


def float_forward(state, args, x):
    """The fp32 model's eval forward in float64 -> (logits (B,nc), {x_min, x_max, a_max[3 per block: h1, h2, out], p_max})."""
    st = {k: np.asarray(v, np.float64) for k, v in state.items()}
    x = np.asarray(x, np.float64)
    x = x[:, 0] if x.ndim == 4 else x
    ranges = {"x_min": float(x.min()), "x_max": float(x.max()), "a_max": []}
    h = x.transpose(0, 2, 1)
    for i in range(len(args["num_channels"])):
        p = f"tcn.network.{i}."
        h1 = np.maximum(_fconv(h, st[p + "conv1.weight"], st[p + "conv1.bias"], 2 ** i), 0.0)
        h2 = np.maximum(_fconv(h1, st[p + "conv2.weight"], st[p + "conv2.bias"], 2 ** i), 0.0)
        res = _fconv(h, st[p + "downsample.weight"], st[p + "downsample.bias"], 1) if p + "downsample.weight" in st else h
        h = np.maximum(h2 + res, 0.0)
        ranges["a_max"] += [float(h1.max()), float(h2.max()), float(h.max())]
    pool = h.mean(axis=1)
    ranges["p_max"] = float(pool.max())
    return pool @ st["fc.3.weight"].T + st["fc.3.bias"], ranges


def r_quantize_model(state, args, feature_shape, ranges):
    """The arrays of the int8 bundle of ``state`` under calibrated ``ranges``, from the text of the law."""
    _, T = feature_shape
    st = {k: np.asarray(v, np.float64) for k, v in state.items()}
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

    def conv(name, w, b, s_in, s_out):
        amax = np.abs(w).reshape(w.shape[0], -1).max(axis=1)
        s_w = np.where(amax > 0, amax / 127.0, 1.0)
        a[name + ".w"] = np.clip(np.rint(w / s_w[:, None, None]), -127, 127).astype(np.int8)
        a[name + ".b"] = np.rint(b / (s_in * s_w)).astype(np.int32)
        ms = [r_encode_multiplier(s_in * s_w[c] / s_out) for c in range(w.shape[0])]
        a[name + ".m"] = np.array([m for m, _ in ms], np.int32)
        a[name + ".sh"] = np.array([s for _, s in ms], np.int32)
    s_in = float(s_x)
    for i in range(len(args["num_channels"])):
        p, q = f"tcn.network.{i}.", f"b{i}."
        s_h1, s_h2, s_out = (scale(v) for v in ranges["a_max"][3 * i:3 * i + 3])
        conv(q + "conv1", st[p + "conv1.weight"], st[p + "conv1.bias"], s_in, s_h1)
        conv(q + "conv2", st[p + "conv2.weight"], st[p + "conv2.bias"], s_h1, s_h2)
        if p + "downsample.weight" in st:
            conv(q + "down", st[p + "downsample.weight"], st[p + "downsample.bias"], s_in, s_out)
        else:
            a[q + "skip.m"], a[q + "skip.sh"] = one(r_encode_multiplier(s_in / s_out))
        a[q + "add.m"], a[q + "add.sh"] = one(r_encode_multiplier(s_h2 / s_out))
        s_in = s_out
    s_p = scale(ranges["p_max"])
    a["pool.m"], a["pool.sh"] = one(r_encode_multiplier(s_in / (T * s_p)))
    w = st["fc.3.weight"]
    amax = np.abs(w).max(axis=1)
    s_w = np.where(amax > 0, amax / 127.0, 1.0)
    a["fc.w"] = np.clip(np.rint(w / s_w[:, None]), -127, 127).astype(np.int8)
    a["fc.b"] = np.rint(st["fc.3.bias"] / (s_p * s_w)).astype(np.int32)
    a["fc.scale"] = (s_p * s_w).astype(np.float32)
    return a


# ------------------------------------------------------------------ cases
def header_for(F, T, args, num_classes=2, kind="int8"):
    layers = [f"b{i}.{n}" for i, n, *_ in block_convs(args)] + ["pool", "fc"]
    return {"format": "wakeword-bundle", "version": 1, "kind": kind, "architecture": "TCNWakeword", "num_classes": int(num_classes),
            "input_shape": [1, 1, F, T], "feature_shape": [F, T], "layers": layers, "tcn": dict(args)}


def random_state(args, num_classes=2, seed=0, gain=1.0, dead=None):
    """A TCNWakeword state_dict (float32 NumPy) under the reference's keys: every tensor uniform in +-gain/sqrt(fan_in), as
    nn.Conv1d and nn.Linear initialise; one all-zero weight channel (block 0, conv2, ZERO_CH).  ``dead``: (block, conv name) whose
    weights are 0 and whose bias is -1, so its ReLU output is 0 everywhere -- a dead layer, a_max = 0."""
    g = np.random.default_rng(seed)
    st = {}
    for i, name, cin, cout, k, _ in block_convs(args):
        key = f"tcn.network.{i}.{'downsample' if name == 'down' else name}"
        bound = gain * float(cin * k) ** -0.5
        st[key + ".weight"] = g.uniform(-bound, bound, (cout, cin, k))
        st[key + ".bias"] = g.uniform(-bound, bound, cout)
        if dead == (i, name):
            st[key + ".weight"][:], st[key + ".bias"][:] = 0.0, -1.0
    st["tcn.network.0.conv2.weight"][ZERO_CH] = 0.0
    c = args["num_channels"][-1]
    st["fc.3.weight"] = g.uniform(-1, 1, (num_classes, c)) * gain * float(c) ** -0.5
    st["fc.3.bias"] = g.uniform(-1, 1, num_classes) * float(c) ** -0.5
    return {k: np.asarray(v, np.float32) for k, v in st.items()}


def hard_bundle(F, T, num_channels, k, num_classes=2, seed=0):
    """(header, arrays): a bundle written integer by integer on which, with ``hard_features``, every hard spot of the law
    occurs; ``assert_hard`` checks that it does.  Weights are random and asymmetric; channel TIE_CH of every conv has
    m = 2^30, sh = 31 -- every odd accumulator is an exact tie -- a zero bias and weights +1, -1, +1, .. that sum to zero, so its
    accumulators are small and of both signs; channel ZERO_CH has all-zero weights.  The multipliers of a conv over K = k Cin
    inputs sit in the binade that brings its accumulators (about 1e4 sqrt(K)) to a few hundred, so outputs clamp at both ends."""
    g = np.random.default_rng(seed)
    args = tcn_args(F, num_channels, k)
    a = {"input_scale": np.array([0.0625], np.float32), "input_zero": np.array([37], np.int32)}
    for i, name, cin, cout, kk, _ in block_convs(args):
        K = cin * kk
        w = g.integers(-127, 128, (cout, cin, kk)).astype(np.int8)
        b = g.integers(-20000, 20001, cout).astype(np.int32)
        m = g.integers(2 ** 30, 2 ** 31, cout).astype(np.int32)
        sh = np.full(cout, 31 + int(np.ceil(np.log2(1.0e4 * np.sqrt(K) / 400.0))), np.int32)
        w[TIE_CH] = np.resize([1, -1], K).reshape(cin, kk)
        b[TIE_CH], m[TIE_CH], sh[TIE_CH] = 0, 2 ** 30, 31
        w[ZERO_CH], b[ZERO_CH], m[ZERO_CH], sh[ZERO_CH] = 0, 3001, 2 ** 30 + 12345, 36
        p = f"b{i}.{name}"
        a[p + ".w"], a[p + ".b"], a[p + ".m"], a[p + ".sh"] = w, b, m, sh
    cin = F
    for i, c in enumerate(num_channels):
        one = lambda v: np.array([v], np.int32)       # noqa: E731
        if cin == c:
            a[f"b{i}.skip.m"], a[f"b{i}.skip.sh"] = one(int(g.integers(2 ** 30, 2 ** 31))), one(31)        # 0.5 .. 1
        a[f"b{i}.add.m"], a[f"b{i}.add.sh"] = one(int(g.integers(2 ** 30, 2 ** 31))), one(30)              # 1 .. 2
        cin = c
    m_p, sh_p = r_encode_multiplier(1.5 / T)
    a["pool.m"], a["pool.sh"] = np.array([m_p], np.int32), np.array([sh_p], np.int32)
    a["fc.w"] = g.integers(-127, 128, (num_classes, cin)).astype(np.int8)
    a["fc.b"] = g.integers(-5000, 5001, num_classes).astype(np.int32)
    a["fc.scale"] = (1.25e-4 * (1.0 + np.arange(num_classes))).astype(np.float32)
    return header_for(F, T, args, num_classes), a


def hard_features(F, T, B, seed=1):
    return np.random.default_rng(seed).uniform(-12.0, 8.0, (B, 1, F, T)).astype(np.float32)


def hard_case(name, num_classes=2, batch=None):
    """(header, arrays, x, ref) of one of SHAPES at its committed seed (``batch``: another batch size), ``assert_hard`` run."""
    B, F, T, ch, k = SHAPES[name]
    B = batch or B
    header, arrays = hard_bundle(F, T, ch, k, num_classes, seed=HARD_SEEDS[name])
    x = hard_features(F, T, B)
    ref = r_forward(header["tcn"], arrays, x, want_acc=True)
    assert_hard(header["tcn"], arrays, ref)
    return header, arrays, x, ref


def assert_hard(args, arrays, ref):
    """``ref = r_forward(args, arrays, x, want_acc=True)``: the hard spots occur."""
    assert int(arrays["input_zero"][0]) != 0
    assert ref["xq"].min() == -128 and ref["xq"].max() == 127, "the input does not saturate at both ends"
    for i, name, *_ in block_convs(args):
        p = f"b{i}.{name}"
        acc = ref["acc/" + p]
        r = r_R(acc, arrays[p + ".m"], arrays[p + ".sh"])
        if name != "down":                                   # (the downsample conv's output is not clamped before the add)
            assert (r < 0).any() and (r > 255).any(), f"{p}: outputs are not clamped at both ends"
            q = ref[f"b{i}.{'h1' if name == 'conv1' else 'h2'}"]
            assert q.min() == -128 and q.max() == 127 and np.unique(q[..., ZERO_CH]).size == 1
        tie = acc[..., TIE_CH]
        assert ((tie % 2 == 1) & (tie > 0)).any() and ((tie % 2 == 1) & (tie < 0)).any(), f"{p}: no ties of both signs"
        assert not arrays[p + ".w"][ZERO_CH].any()
    mixed, both = False, False
    for i in range(len(args["num_channels"])):
        skip, add = ref[f"skip/b{i}"], ref[f"add/b{i}"]
        s = skip + add
        assert (s > 255).any(), f"block {i}: the add never clamps from above"
        mixed |= bool(((skip < 0) & (add > 0)).any())
        both |= bool((s < 0).any() and (s > 255).any())
    assert mixed, "no block output with a negative skip term beside a positive h2 term"
    assert both, "no block output at which both clamps of the add are hit"
    assert np.unique(ref["pool"]).size > 8
