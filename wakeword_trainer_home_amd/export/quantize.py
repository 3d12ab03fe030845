"""The export side of the int8 law (DESIGN.md "Export"): BatchNorm folding, scales, integer weights, biases and multipliers
of ``cnn_small``, ``TCNWakeword``, ``ResNet18Wakeword``, ``LSTMWakeword``, ``CRNNWakeword`` and ``MobileNetV3Wakeword``, all in float64 NumPy on the host.  ``reference.py`` is the other half: what a runtime does
with the result."""
import math
from typing import Dict, Sequence

import numpy as np

from .reference import BLOCKS, CONVS, LSTM_DIRS, LSTM_HIDDEN, LSTM_TABLE, resnet_blocks, resnet_half, tcn_blocks

A_MAX_FLOOR = 255.0 * 2.0 ** -20       # a calibrated maximum at or below zero (a dead layer) counts as this: s_out = 2^-20
ACC_MAX_3X3 = 9 * 127 * 255            # largest |sum q_w (q_in - z_in)| of the stem and the depthwise convs
ACC_MAX_1X1 = 64 * 127 * 255           # ... of the pointwise convs and the classifier
INT32_MAX = 2 ** 31 - 1


class QuantizationError(ValueError):
    """The model or its calibration cannot be expressed in the int8 law; the message names the layer and channel."""


def encode_multiplier(r: float, what: str = "multiplier"):
    """(m, sh) with 2^30 <= m < 2^31, 1 <= sh <= 62 and m * 2^-sh the nearest such value to ``r`` (ties to the even m)."""
    r = float(r)
    if not (math.isfinite(r) and r > 0.0):
        raise QuantizationError(f"{what}: the real multiplier {r!r} is not positive and finite")
    f, e = math.frexp(r)                         # r = f * 2^e, 0.5 <= f < 1
    m = int(np.rint(f * 2.0 ** 31))              # exact product, one rounding
    if m == 2 ** 31:
        m, e = 2 ** 30, e + 1
    sh = 31 - e
    if not 1 <= sh <= 62:
        raise QuantizationError(f"{what}: the real multiplier {r!r} needs a shift of {sh}, outside [1, 62]")
    return m, sh


def fold_bn(w, gamma, beta, mean, var, eps):
    """W' = W g / sqrt(var + eps) per output channel, b' = beta - mean g / sqrt(var + eps); float64."""
    w, gamma, beta, mean, var = (np.asarray(t, np.float64) for t in (w, gamma, beta, mean, var))
    k = gamma / np.sqrt(var + float(eps))
    return w.reshape(w.shape[0], -1) * k[:, None], beta - mean * k


def quantize_weights(wf):
    """wf float64 (C,K) -> (int8 (C,K), s_w float64 (C,)): s_w = max|row| / 127, an all-zero row takes 1."""
    amax = np.abs(wf).max(axis=1)
    s_w = np.where(amax > 0, amax / 127.0, 1.0)
    return np.clip(np.rint(wf / s_w[:, None]), -127, 127).astype(np.int8), s_w


def quantize_bias(bf, s_in, s_w, acc_max, layer, unit="channel"):
    q = np.rint(np.asarray(bf, np.float64) / (s_in * s_w))
    bad = np.nonzero(~(np.abs(q) + acc_max <= INT32_MAX))[0]       # (a NaN is bad too)
    if bad.size:
        c = int(bad[0])
        raise QuantizationError(f"{layer}, {unit} {c}: bias {q[c]!r} plus an accumulator of up to {acc_max} leaves int32")
    return q.astype(np.int32)


def input_qparams(x_min, x_max):
    """(s_x as float32, z_x) from the calibrated range, widened to contain 0; an empty range counts as [0, 1]."""
    lo, hi = min(float(x_min), 0.0), max(float(x_max), 0.0)
    if not (math.isfinite(lo) and math.isfinite(hi)):
        raise QuantizationError(f"input: the calibrated range [{x_min!r}, {x_max!r}] is not finite")
    if hi - lo <= 0.0:
        hi = 1.0
    s = np.float32((hi - lo) / 255.0)
    if not (np.isfinite(s) and s > 0):
        raise QuantizationError(f"input: the scale of the range [{lo!r}, {hi!r}] is not a positive float32")
    z = int(np.clip(np.rint(-128.0 - lo / float(s)), -128, 127))
    return s, z


def out_scale(a_max):
    a = float(a_max)
    if math.isnan(a) or math.isinf(a):
        raise QuantizationError(f"a calibrated maximum of {a!r} is not finite")
    return max(a, A_MAX_FLOOR) / 255.0


def cnn_small_float_layers(state: Dict[str, np.ndarray], eps: float = 1e-5):
    """{conv name: (W' (64,K), b' (64,))} of a cnn_small state_dict, BatchNorm folded; plus ``fc``."""
    def bn(prefix):
        return [state[f"{prefix}.{k}"] for k in ("weight", "bias", "running_mean", "running_var")]
    layers = {"stem": fold_bn(state["stem.conv.weight"], *bn("stem.bn"), eps)}
    for k in range(BLOCKS):
        layers[f"dw{k}"] = fold_bn(state[f"blocks.{k}.dw.weight"], *bn(f"blocks.{k}.dw_bn"), eps)
        layers[f"pw{k}"] = fold_bn(state[f"blocks.{k}.pw.weight"], *bn(f"blocks.{k}.pw_bn"), eps)
    if "classifier.weight" in state:                 # (the CRNN's front end is the conv stack alone)
        layers["fc"] = (np.asarray(state["classifier.weight"], np.float64), np.asarray(state["classifier.bias"], np.float64))
    return layers


def quantize_cnn_small(state: Dict[str, np.ndarray], feature_shape: Sequence[int], x_min: float, x_max: float,
                       a_max: Sequence[float], p_max: float, eps: float = 1e-5):
    """The arrays of an int8 bundle and its scales.  ``a_max``: the calibrated maximum of each conv's post-ReLU output, in
    ``CONVS`` order; ``p_max``: that of the pooled vector.  Raises ``QuantizationError`` where the law refuses."""
    F, T = int(feature_shape[0]), int(feature_shape[1])
    H, W = (F + 1) // 2, (T + 1) // 2
    if len(a_max) != len(CONVS):
        raise QuantizationError(f"{len(a_max)} calibrated maxima for {len(CONVS)} convs")
    layers = cnn_small_float_layers(state, eps)
    if "fc" not in layers or layers["fc"][0].shape != (2, 64):
        shape = layers["fc"][0].shape if "fc" in layers else None
        raise QuantizationError(f"the int8 path has a Linear(64,2) classifier, got weights of shape {shape}")
    s_x, z_x = input_qparams(x_min, x_max)
    arrays = {"input_scale": np.array([s_x], np.float32), "input_zero": np.array([z_x], np.int32)}
    scales = {"input": float(s_x)}
    s_in = float(s_x)
    for name, am in zip(CONVS, a_max):
        wf, bf = layers[name]
        acc_max = ACC_MAX_1X1 if name.startswith("pw") else ACC_MAX_3X3
        q_w, s_w = quantize_weights(wf)
        s_out = out_scale(am)
        ms = [encode_multiplier(s_in * s_w[c] / s_out, f"{name}, channel {c}") for c in range(64)]
        arrays[name + ".w"] = q_w
        arrays[name + ".b"] = quantize_bias(bf, s_in, s_w, acc_max, name)
        arrays[name + ".m"] = np.array([m for m, _ in ms], np.int32)
        arrays[name + ".sh"] = np.array([s for _, s in ms], np.int32)
        scales[name] = s_out
        s_in = s_out
    s_p = out_scale(p_max)
    m_p, sh_p = encode_multiplier(s_in / (H * W * s_p), "pool")
    arrays["pool.m"], arrays["pool.sh"] = np.array([m_p], np.int32), np.array([sh_p], np.int32)
    scales["pool"] = s_p
    wf, bf = layers["fc"]
    q_w, s_w = quantize_weights(wf)
    arrays["fc.w"] = q_w
    arrays["fc.b"] = quantize_bias(bf, s_p, s_w, ACC_MAX_1X1, "classifier")
    arrays["fc.scale"] = (s_p * s_w).astype(np.float32)
    return arrays, scales


DS_MAX_FLOOR = 127.0 * 2.0 ** -20      # a calibrated max|ds| at or below zero counts as this: s_ds = 2^-20
RESNET_MAX_CLASSES = 64


def signed_scale(a_max):
    """The scale of a signed tensor (zero point 0) from its calibrated max |value|: the ResNet's downsample output."""
    a = float(a_max)
    if math.isnan(a) or math.isinf(a):
        raise QuantizationError(f"a calibrated maximum of {a!r} is not finite")
    return max(a, DS_MAX_FLOOR) / 127.0


def _quantize_conv2d(arrays, name, wf, bf, shape, s_in, s_out):
    """One BatchNorm-folded Conv2d of the ResNet: ``wf`` float64 (Cout, Cin k k), ``shape`` = (Cout, Cin, k, k)."""
    cout, cin, k, _ = shape
    q_w, s_w = quantize_weights(wf)
    ms = [encode_multiplier(s_in * s_w[c] / s_out, f"{name}, channel {c}") for c in range(cout)]
    arrays[name + ".w"] = q_w.reshape(shape)
    arrays[name + ".b"] = quantize_bias(bf, s_in, s_w, k * k * cin * 127 * 255, name)
    arrays[name + ".m"] = np.array([m for m, _ in ms], np.int32)
    arrays[name + ".sh"] = np.array([s for _, s in ms], np.int32)


def quantize_resnet18(state: Dict[str, np.ndarray], feature_shape: Sequence[int], ranges: dict, eps: float = 1e-5):
    """The arrays of an int8 ResNet18Wakeword bundle and its scales (the law's subsection "ResNet18").  ``ranges``: ``x_min``,
    ``x_max``, ``stem_max``, per block (eight, in execution order) ``h1_max`` and ``out_max``, ``ds_max`` (max |ds| of the three
    downsample outputs, stages 2-4) and ``p_max``.  Weights keep nn.Conv2d's (Cout,Cin,k,k).  Raises ``QuantizationError`` where
    the law refuses."""
    F, T = int(feature_shape[0]), int(feature_shape[1])
    st = {k: np.asarray(v, np.float64) for k, v in state.items()}
    if "resnet.fc.1.weight" not in st or "resnet.conv1.weight" not in st:
        raise QuantizationError("the state holds no ResNet18Wakeword (resnet.conv1.weight, resnet.fc.1.weight)")
    num_classes = st["resnet.fc.1.weight"].shape[0]
    if not 2 <= num_classes <= RESNET_MAX_CLASSES:
        raise QuantizationError(f"the int8 ResNet18 takes 2..{RESNET_MAX_CLASSES} classes, got {num_classes}")
    blocks = resnet_blocks()
    if len(ranges["h1_max"]) != 8 or len(ranges["out_max"]) != 8 or len(ranges["ds_max"]) != 3:
        raise QuantizationError("the calibrated ranges need eight h1 and block-output maxima and three downsample maxima")

    def folded(conv, bn, shape):
        key = conv + ".weight"
        if key not in st or st[key].shape != shape:
            raise QuantizationError(f"{key}: expected weights of shape {shape}")
        return fold_bn(st[key], *(st[f"{bn}.{k}"] for k in ("weight", "bias", "running_mean", "running_var")), eps)
    s_x, z_x = input_qparams(ranges["x_min"], ranges["x_max"])
    arrays = {"input_scale": np.array([s_x], np.float32), "input_zero": np.array([z_x], np.int32)}
    scales = {"input": float(s_x)}
    s_in = out_scale(ranges["stem_max"])
    _quantize_conv2d(arrays, "stem", *folded("resnet.conv1", "resnet.bn1", (64, 1, 7, 7)), (64, 1, 7, 7), float(s_x), s_in)
    scales["stem"] = s_in                          # (the max pool passes scale and zero point through)
    n_ds = 0
    for i, (name, cin, cout, _, down) in enumerate(blocks):
        p = f"resnet.layer{name[1]}.{name[3]}."
        s_h1, s_out = out_scale(ranges["h1_max"][i]), out_scale(ranges["out_max"][i])
        _quantize_conv2d(arrays, name + ".conv1", *folded(p + "conv1", p + "bn1", (cout, cin, 3, 3)), (cout, cin, 3, 3), s_in, s_h1)
        s_res = s_in
        if down:
            s_res = signed_scale(ranges["ds_max"][n_ds])
            n_ds += 1
            _quantize_conv2d(arrays, name + ".down", *folded(p + "downsample.0", p + "downsample.1", (cout, cin, 1, 1)),
                             (cout, cin, 1, 1), s_in, s_res)
            scales[name + ".ds"] = s_res
        _quantize_conv2d(arrays, name + ".conv2", *folded(p + "conv2", p + "bn2", (cout, cout, 3, 3)), (cout, cout, 3, 3), s_h1, s_out)
        _one_multiplier(arrays, name + ".res", s_res / s_out)
        scales.update({name + ".h1": s_h1, name + ".out": s_out})
        s_in = s_out
    hw = F, T
    for _ in range(5):
        hw = resnet_half(hw[0]), resnet_half(hw[1])
    s_p = out_scale(ranges["p_max"])
    _one_multiplier(arrays, "pool", s_in / (hw[0] * hw[1] * s_p))
    scales["pool"] = s_p
    if st["resnet.fc.1.weight"].shape != (num_classes, 512):
        raise QuantizationError(f"resnet.fc.1.weight: expected weights of shape {(num_classes, 512)}")
    q_w, s_w = quantize_weights(st["resnet.fc.1.weight"])
    arrays["fc.w"] = q_w
    arrays["fc.b"] = quantize_bias(st["resnet.fc.1.bias"], s_p, s_w, 512 * 127 * 255, "classifier")
    arrays["fc.scale"] = (s_p * s_w).astype(np.float32)
    return arrays, scales


TCN_MAX_BLOCKS, TCN_MAX_KERNEL, TCN_MAX_CLASSES = 8, 8, 64


def check_tcn_args(tcn_args, num_classes=2):
    """The limits of the TCN int8 path: the model's own (channel counts multiples of 4, 1 <= k <= 8, at most 8 blocks) and
    2 <= num_classes <= 64.  -> (input_size, [channels], kernel_size) as ints."""
    F, ch, k = int(tcn_args["input_size"]), [int(c) for c in tcn_args["num_channels"]], int(tcn_args["kernel_size"])
    if not 1 <= len(ch) <= TCN_MAX_BLOCKS:
        raise QuantizationError(f"the int8 TCN takes 1..{TCN_MAX_BLOCKS} blocks, got {len(ch)}")
    if not 1 <= k <= TCN_MAX_KERNEL:
        raise QuantizationError(f"the int8 TCN takes 1 <= kernel_size <= {TCN_MAX_KERNEL}, got {k}")
    if any(c < 4 or c % 4 for c in [F] + ch):
        raise QuantizationError(f"the int8 TCN takes channel counts that are positive multiples of 4, got {[F] + ch}")
    if not 2 <= int(num_classes) <= TCN_MAX_CLASSES:
        raise QuantizationError(f"the int8 TCN takes 2..{TCN_MAX_CLASSES} classes, got {num_classes}")
    return F, ch, k


def _quantize_conv1d(arrays, name, wf, bf, s_in, s_out):
    """One Conv1d (Cout, Cin, k) of the TCN: weights, bias with the refusal, one multiplier per output channel."""
    cout, cin, k = wf.shape
    q_w, s_w = quantize_weights(wf.reshape(cout, cin * k))
    ms = [encode_multiplier(s_in * s_w[c] / s_out, f"{name}, channel {c}") for c in range(cout)]
    arrays[name + ".w"] = q_w.reshape(cout, cin, k)
    arrays[name + ".b"] = quantize_bias(bf, s_in, s_w, k * cin * 127 * 255, name)
    arrays[name + ".m"] = np.array([m for m, _ in ms], np.int32)
    arrays[name + ".sh"] = np.array([s for _, s in ms], np.int32)


def _one_multiplier(arrays, name, r):
    m, sh = encode_multiplier(r, name)
    arrays[name + ".m"], arrays[name + ".sh"] = np.array([m], np.int32), np.array([sh], np.int32)


def quantize_tcn(state: Dict[str, np.ndarray], tcn_args: dict, feature_shape: Sequence[int], x_min: float, x_max: float,
                 a_max: Sequence[float], p_max: float):
    """The arrays of an int8 TCNWakeword bundle and its scales (the law's subsection "TCN").  ``tcn_args``: ``input_size``,
    ``num_channels``, ``kernel_size``; ``a_max``: per block the calibrated maxima of h1, h2 and the block output, in that order;
    ``p_max``: that of the pooled vector.  Arrays are unpadded.  Raises ``QuantizationError`` where the law refuses."""
    F, T = int(feature_shape[0]), int(feature_shape[1])
    st = {k: np.asarray(v, np.float64) for k, v in state.items()}
    if "fc.3.weight" not in st:
        raise QuantizationError("the state holds no TCNWakeword classifier (fc.3.weight)")
    num_classes = st["fc.3.weight"].shape[0]
    in_size, channels, k = check_tcn_args(tcn_args, num_classes)
    if in_size != F:
        raise QuantizationError(f"the TCN reads {in_size} features per frame, the feature shape has {F}")
    if len(a_max) != 3 * len(channels):
        raise QuantizationError(f"{len(a_max)} calibrated maxima for {len(channels)} blocks of three tensors")
    s_x, z_x = input_qparams(x_min, x_max)
    arrays = {"input_scale": np.array([s_x], np.float32), "input_zero": np.array([z_x], np.int32)}
    scales = {"input": float(s_x)}
    s_in = float(s_x)
    for i, cin, cout, _, down in tcn_blocks(tcn_args):
        p, q = f"tcn.network.{i}.", f"b{i}."
        for key, shape in ((p + "conv1.weight", (cout, cin, k)), (p + "conv2.weight", (cout, cout, k))):
            if key not in st or st[key].shape != shape:
                raise QuantizationError(f"{key}: expected weights of shape {shape}")
        if down and (p + "downsample.weight" not in st or st[p + "downsample.weight"].shape != (cout, cin, 1)):
            raise QuantizationError(f"{p}downsample.weight: expected weights of shape {(cout, cin, 1)}")
        s_h1, s_h2, s_out = (out_scale(v) for v in a_max[3 * i:3 * i + 3])
        _quantize_conv1d(arrays, q + "conv1", st[p + "conv1.weight"], st[p + "conv1.bias"], s_in, s_h1)
        _quantize_conv1d(arrays, q + "conv2", st[p + "conv2.weight"], st[p + "conv2.bias"], s_h1, s_h2)
        if down:
            _quantize_conv1d(arrays, q + "down", st[p + "downsample.weight"], st[p + "downsample.bias"], s_in, s_out)
        else:
            _one_multiplier(arrays, q + "skip", s_in / s_out)
        _one_multiplier(arrays, q + "add", s_h2 / s_out)
        scales.update({q + "h1": s_h1, q + "h2": s_h2, q + "out": s_out})
        s_in = s_out
    s_p = out_scale(p_max)
    _one_multiplier(arrays, "pool", s_in / (T * s_p))
    scales["pool"] = s_p
    if st["fc.3.weight"].shape != (num_classes, channels[-1]):
        raise QuantizationError(f"fc.3.weight: expected weights of shape {(num_classes, channels[-1])}")
    q_w, s_w = quantize_weights(st["fc.3.weight"])
    arrays["fc.w"] = q_w
    arrays["fc.b"] = quantize_bias(st["fc.3.bias"], s_p, s_w, channels[-1] * 127 * 255, "classifier")
    arrays["fc.scale"] = (s_p * s_w).astype(np.float32)
    return arrays, scales


LSTM_MAX_LAYERS, LSTM_MAX_CLASSES = 8, 64
S_H = 2.0 ** -7                        # the fixed scale of the hidden operand q_h (zero point 0)


def _check_rnn_args(what, args, num_classes, input_size=None):
    """What ``check_lstm_args`` and ``check_crnn_args`` share; ``what`` is the model word of the messages, ``input_size`` is checked
    where the model has one.  -> (num_layers, num_directions)."""
    H, L = int(args["hidden_size"]), int(args["num_layers"])
    if H != LSTM_HIDDEN:
        raise QuantizationError(f"the int8 {what} implements hidden_size == {LSTM_HIDDEN}, got hidden_size {H}")
    if not 1 <= L <= LSTM_MAX_LAYERS:
        raise QuantizationError(f"the int8 {what} takes 1..{LSTM_MAX_LAYERS} layers, got num_layers {L}")
    if input_size is not None and input_size < 1:
        raise QuantizationError(f"the int8 {what} takes a positive input_size, got {input_size}")
    if not 2 <= int(num_classes) <= LSTM_MAX_CLASSES:
        raise QuantizationError(f"the int8 {what} takes 2..{LSTM_MAX_CLASSES} classes, got num_classes {num_classes}")
    return L, 2 if args["bidirectional"] else 1


def check_lstm_args(lstm_args, num_classes=2):
    """The limits of the LSTM int8 path: hidden size 128 (the implemented size of ``LSTMWakeword``), 1..8 layers, a positive
    input size, 2 <= num_classes <= 64.  -> (input_size, num_layers, num_directions) as ints."""
    I = int(lstm_args["input_size"])
    return (I,) + _check_rnn_args("LSTM", lstm_args, num_classes, I)


def lstm_tables():
    """(tab.sigmoid, tab.tanh): int16 (4096,), entry j the function at j / 256 - 8 in Q15, from float64; the sigmoid capped at
    32767, the tanh at +-32767.  Written into the bundle: a runtime reads them, it never recomputes them."""
    x = np.arange(LSTM_TABLE, dtype=np.float64) / 256.0 - 8.0
    sig = np.minimum(np.rint(2.0 ** 15 / (1.0 + np.exp(-x))), 32767)
    tanh = np.clip(np.rint(np.tanh(x) * 2.0 ** 15), -32767, 32767)
    return sig.astype(np.int16), tanh.astype(np.int16)


def _quantize_gates(arrays, name, wf, bf, s_in, acc_max):
    """One weight matrix (4H, K) of an LSTM direction, or (3H, K) of a GRU direction, with its bias: per-row weights, the int32 bias with the refusal, and the
    multiplier that brings the accumulator to Q8 gate pre-activations, m 2^-sh ~ s_in s_w 2^8."""
    if not np.isfinite(wf).all():
        raise QuantizationError(f"{name}: a weight is not finite")
    q_w, s_w = quantize_weights(wf)
    ms = [encode_multiplier(s_in * s_w[n] * 256.0, f"{name}, row {n}") for n in range(wf.shape[0])]
    arrays[name + ".w"] = q_w
    arrays[name + ".b"] = quantize_bias(bf, s_in, s_w, acc_max, name, unit="row")
    arrays[name + ".m"] = np.array([m for m, _ in ms], np.int32)
    arrays[name + ".sh"] = np.array([s for _, s in ms], np.int32)


def _quantize_rnn_stack(arrays, st, gates, rnn, fc, input_size, num_layers, num_directions, s_in0):
    """A recurrent stack of ``gates`` gate blocks per direction (the law's subsections "LSTM": 4, "GRU": 3) into ``arrays``: per
    layer and direction ``l{l}.{fwd|rev}.{ih,hh}.{w,b,m,sh}``, then ``fc.*`` and ``tab.*``.  ``st``: float64 state; ``rnn`` / ``fc``:
    the key prefixes of the stack and of its classifier in it; ``s_in0``: the scale of the layer-0 input.  Raises
    ``QuantizationError`` where the law refuses."""
    H, nd = LSTM_HIDDEN, num_directions
    for layer in range(num_layers):
        K, s_in = (input_size, float(s_in0)) if layer == 0 else (nd * H, S_H)
        for d in range(nd):
            sfx, name = f"_l{layer}" + ("_reverse" if d else ""), f"l{layer}.{LSTM_DIRS[d]}"
            for key, shape in ((f"{rnn}weight_ih{sfx}", (gates * H, K)), (f"{rnn}weight_hh{sfx}", (gates * H, H)),
                               (f"{rnn}bias_ih{sfx}", (gates * H,)), (f"{rnn}bias_hh{sfx}", (gates * H,))):
                if key not in st or st[key].shape != shape:
                    raise QuantizationError(f"{key}: expected a tensor of shape {shape}")
            _quantize_gates(arrays, name + ".ih", st[f"{rnn}weight_ih{sfx}"], st[f"{rnn}bias_ih{sfx}"], s_in, K * 127 * 255)
            _quantize_gates(arrays, name + ".hh", st[f"{rnn}weight_hh{sfx}"], st[f"{rnn}bias_hh{sfx}"], S_H, H * 127 * 128)
    fw, fb = st.get(fc + "weight"), st.get(fc + "bias")
    if fw is None or fb is None or fw.ndim != 2 or fw.shape[1] != nd * H or fb.shape != (fw.shape[0],):
        raise QuantizationError(f"{fc}weight: expected weights of shape (num_classes, {nd * H}) and their bias")
    if not np.isfinite(fw).all():
        raise QuantizationError("classifier: a weight is not finite")
    q_w, s_w = quantize_weights(fw)
    arrays["fc.w"] = q_w
    arrays["fc.b"] = quantize_bias(fb, S_H, s_w, nd * H * 127 * 128, "classifier", unit="row")
    arrays["fc.scale"] = (S_H * s_w).astype(np.float32)
    arrays["tab.sigmoid"], arrays["tab.tanh"] = lstm_tables()


def quantize_lstm(state: Dict[str, np.ndarray], lstm_args: dict, x_min: float, x_max: float):
    """The arrays of an int8 LSTMWakeword bundle and its scales (the law's subsection "LSTM").  ``lstm_args``: ``input_size``,
    ``hidden_size``, ``num_layers``, ``bidirectional``.  Only the input range is calibrated: hidden state, gates and cell have
    fixed power-of-two scales.  Arrays are unpadded.  Raises ``QuantizationError`` where the law refuses."""
    st = {k: np.asarray(v, np.float64) for k, v in state.items()}
    if "fc.1.weight" not in st or "lstm.weight_ih_l0" not in st:
        raise QuantizationError("the state holds no LSTMWakeword (lstm.weight_ih_l0, fc.1.weight)")
    num_classes = st["fc.1.weight"].shape[0]
    I, L, nd = check_lstm_args(lstm_args, num_classes)
    if st["fc.1.weight"].shape != (num_classes, nd * LSTM_HIDDEN):
        raise QuantizationError(f"fc.1.weight: expected weights of shape {(num_classes, nd * LSTM_HIDDEN)}")
    s_x, z_x = input_qparams(x_min, x_max)
    arrays = {"input_scale": np.array([s_x], np.float32), "input_zero": np.array([z_x], np.int32)}
    _quantize_rnn_stack(arrays, st, 4, "lstm.", "fc.1.", I, L, nd, s_x)
    return arrays, {"input": float(s_x), "hidden": S_H}


def check_crnn_args(crnn_args, num_classes=2):
    """The limits of the CRNN int8 path: hidden size 128 (the implemented size of the GRU stack), 1..8 layers,
    2 <= num_classes <= 64.  -> (num_layers, num_directions) as ints."""
    return _check_rnn_args("CRNN", crnn_args, num_classes)


def quantize_gru_stack(arrays, st, prefix, input_size, num_layers, num_directions, s_in0):
    """The GRU stack of the law's subsection "GRU" into ``arrays``: per layer and direction ``l{l}.{fwd|rev}.{ih,hh}.{w,b,m,sh}``
    (gate rows r, z, n), then ``fc.*`` and ``tab.*``.  ``st``: float64 state; ``prefix``: where the stack lives in it (``gru.*`` and
    ``fc.1.*`` below it); ``s_in0``: the scale of the layer-0 input.  Raises ``QuantizationError`` where the law refuses."""
    _quantize_rnn_stack(arrays, st, 3, prefix + "gru.", prefix + "fc.1.", input_size, num_layers, num_directions, s_in0)


def quantize_crnn(state: Dict[str, np.ndarray], crnn_args: dict, F: int, ranges: dict, eps: float = 1e-5):
    """The arrays of an int8 CRNNWakeword bundle and its scales (the law's subsections "GRU" and "CRNN").  ``crnn_args``:
    ``hidden_size``, ``num_layers``, ``bidirectional``; ``F``: the feature rows of the bundle; ``ranges``: ``x_min``, ``x_max``,
    ``a_max`` (the nine conv maxima in ``CONVS`` order) and ``f_max`` (the maximum of the float front end's output sequence).
    Arrays are unpadded: ``front.<conv>.{w,b,m,sh}``, ``fmean.{m,sh}``, the stack's, ``fc.*``, ``tab.*``."""
    st = {k: np.asarray(v, np.float64) for k, v in state.items() if np.asarray(v).dtype.kind == "f"}
    if "front.stem.conv.weight" not in st or "rnn.gru.weight_ih_l0" not in st or "rnn.fc.1.weight" not in st:
        raise QuantizationError("the state holds no CRNNWakeword (front.stem.conv.weight, rnn.gru.weight_ih_l0, rnn.fc.1.weight)")
    L, nd = check_crnn_args(crnn_args, st["rnn.fc.1.weight"].shape[0])
    F = int(F)
    if F < 1:
        raise QuantizationError(f"the int8 CRNN takes a positive number of feature rows, got {F}")
    a_max = list(ranges["a_max"])
    if len(a_max) != len(CONVS):
        raise QuantizationError(f"{len(a_max)} calibrated maxima for {len(CONVS)} convs")
    layers = cnn_small_float_layers({k[len("front."):]: v for k, v in st.items() if k.startswith("front.")}, eps)
    s_x, z_x = input_qparams(ranges["x_min"], ranges["x_max"])
    arrays = {"input_scale": np.array([s_x], np.float32), "input_zero": np.array([z_x], np.int32)}
    scales = {"input": float(s_x), "hidden": S_H}
    s_in = float(s_x)
    for name, am in zip(CONVS, a_max):
        wf, bf = layers[name]
        if not np.isfinite(wf).all():
            raise QuantizationError(f"front.{name}: a weight is not finite")
        q_w, s_w = quantize_weights(wf)
        s_out = out_scale(am)
        ms = [encode_multiplier(s_in * s_w[c] / s_out, f"front.{name}, channel {c}") for c in range(64)]
        arrays[f"front.{name}.w"] = q_w
        arrays[f"front.{name}.b"] = quantize_bias(bf, s_in, s_w, ACC_MAX_1X1 if name.startswith("pw") else ACC_MAX_3X3, "front." + name)
        arrays[f"front.{name}.m"] = np.array([m for m, _ in ms], np.int32)
        arrays[f"front.{name}.sh"] = np.array([s for _, s in ms], np.int32)
        scales["front." + name] = s_out
        s_in = s_out
    s_f = out_scale(ranges["f_max"])
    _one_multiplier(arrays, "fmean", s_in / (((F + 1) // 2) * s_f))
    scales["fmean"] = s_f
    quantize_gru_stack(arrays, st, "rnn.", 64, L, nd, s_f)
    return arrays, scales


MBV3_MAX_CLASSES = 64


def asym_qparams(lo, hi, what):
    """The *input rule* on a calibrated (min, max) for any asymmetric tensor: (s as float32, z); the range is widened to contain 0."""
    try:
        return input_qparams(lo, hi)
    except QuantizationError as e:
        raise QuantizationError(f"{what}: {str(e)[len('input: '):]}") from None


def hardswish_table(s_u, z_u, s_out, z_out):
    """T[i] = clamp(rne(hs((i - 128 - z_u) s_u) / s_out) + z_out, -128, 127), hs(v) = v min(max(v + 3, 0), 6) / 6: int8 (256,), in
    float64.  A runtime reads it from the bundle and never recomputes it."""
    v = (np.arange(256, dtype=np.float64) - 128.0 - float(z_u)) * float(s_u)
    hs = v * np.minimum(np.maximum(v + 3.0, 0.0), 6.0) / 6.0
    return np.clip(np.rint(hs / float(s_out)) + float(z_out), -128, 127).astype(np.int8)


def _quantize_mbv3_layer(arrays, scales, name, wf, bf, s_in, acc_max, kind, rng, rng_u=None, bias_shift=0.0, real=None):
    """One weight matrix ``wf`` (Cout, K) with its float bias under one of the law's epilogues.  ``kind``: ``relu`` (``rng[1]`` is
    the calibrated maximum), ``signed`` (max |.| of ``rng``), ``hs`` (the Hardswish rule: ``rng_u`` is the pre-activation's range,
    ``rng`` the output's) or ``gate`` (fc2 with Hardsigmoid: +3 folded into the bias, the multiplier aims at 255 / 6).
    -> (s_out, z_out) of the tensor the layer writes."""
    wf = np.asarray(wf, np.float64)
    if not (np.isfinite(wf).all() and np.isfinite(np.asarray(bf, np.float64)).all()):
        raise QuantizationError(f"{name}: a weight or folded bias is not finite")
    q_w, s_w = quantize_weights(wf)
    if kind == "hs":
        s_u, z_u = asym_qparams(max(float(rng_u[0]), -3.0), rng_u[1], name + " pre-activation")
        s_o, z_o = asym_qparams(rng[0], rng[1], name + " output")
        arrays[name + ".zu"], arrays[name + ".zo"] = np.array([z_u], np.int32), np.array([z_o], np.int32)
        arrays[name + ".tab"] = hardswish_table(s_u, z_u, s_o, z_o)
        s_t, s_o = float(s_u), float(s_o)
        scales[name + ".u"] = s_t
    elif kind == "relu":
        s_t = s_o = out_scale(rng[1])
        z_o = -128
    elif kind == "signed":
        s_t = s_o = signed_scale(max(abs(float(rng[0])), abs(float(rng[1]))))
        z_o = 0
    else:
        s_t, s_o, z_o = 6.0 / 255.0, 1.0 / 255.0, 0
    ms = [encode_multiplier(s_in * s_w[c] / s_t, f"{name}, channel {c}") for c in range(wf.shape[0])]
    arrays[name + ".w"] = q_w
    arrays[name + ".b"] = quantize_bias(np.asarray(bf, np.float64) + bias_shift, s_in, s_w, acc_max, name)
    arrays[name + ".m"] = np.array([m for m, _ in ms], np.int32)
    arrays[name + ".sh"] = np.array([s for _, s in ms], np.int32)
    scales[real or name] = s_o
    return s_o, z_o


def quantize_mobilenetv3(state: Dict[str, np.ndarray], feature_shape: Sequence[int], cal: dict, eps: float = 1e-3):
    """The arrays of an int8 MobileNetV3Wakeword bundle and its scales (the law's subsection "MobileNetV3").  ``cal``: ``x_min``,
    ``x_max`` and ``ranges``, {name: (min, max)} over ``reference.mbv3_range_names()``.  Arrays are unpadded: ``stem.*``, per block
    ``b{i}.expand|dw|project.{w,b,m,sh}``, ``b{i}.pool.{m,sh,hw}``, ``b{i}.fc1|fc2.{w,b,m,sh}``, ``b{i}.gate.{m,sh}``,
    ``b{i}.res.{m,sh}``; ``last.*``, ``pool.{m,sh,hw}``, ``cls0.*``, ``fc.{w,b,scale}``; every Hardswish layer carries ``.zu``, ``.zo``
    and ``.tab``.  Raises ``QuantizationError`` where the law refuses."""
    from .reference import MBV3_HIDDEN, MBV3_LAST, MBV3_STEM, mbv3_blocks, mbv3_range_names
    F, T = int(feature_shape[0]), int(feature_shape[1])
    st = {k: np.asarray(v, np.float64) for k, v in state.items() if np.asarray(v).dtype.kind == "f"}
    pre = "mobilenet.features."
    if pre + "0.0.weight" not in st or "mobilenet.classifier.3.weight" not in st:
        raise QuantizationError("the state holds no MobileNetV3Wakeword (mobilenet.features.0.0.weight, mobilenet.classifier.3.weight)")
    num_classes = st["mobilenet.classifier.3.weight"].shape[0]
    if not 2 <= num_classes <= MBV3_MAX_CLASSES:
        raise QuantizationError(f"the int8 MobileNetV3 takes 2..{MBV3_MAX_CLASSES} classes, got {num_classes}")
    rng = cal["ranges"]
    missing = [n for n in mbv3_range_names() if n not in rng]
    if missing:
        raise QuantizationError(f"the calibrated ranges lack {missing[:3]}")

    def folded(p, shape):
        key = p + ".0.weight"
        if key not in st or st[key].shape != shape:
            raise QuantizationError(f"{key}: expected weights of shape {shape}")
        return fold_bn(st[key], *(st[f"{p}.1.{k}"] for k in ("weight", "bias", "running_mean", "running_var")), eps)

    def plain(p, shape):
        if p + ".weight" not in st or st[p + ".weight"].shape[:2] != shape or st[p + ".bias"].shape != shape[:1]:
            raise QuantizationError(f"{p}.weight: expected weights of shape {shape} and their bias")
        return st[p + ".weight"].reshape(shape), st[p + ".bias"]
    s_x, z_x = input_qparams(cal["x_min"], cal["x_max"])
    arrays = {"input_scale": np.array([s_x], np.float32), "input_zero": np.array([z_x], np.int32)}
    scales = {"input": float(s_x)}
    s, z = _quantize_mbv3_layer(arrays, scales, "stem", *folded(pre + "0", (MBV3_STEM, 1, 3, 3)), float(s_x), 9 * 127 * 255, "hs",
                                rng["stem"], rng["stem.u"])
    for i, b in enumerate(mbv3_blocks(F, T)):
        p, q, j = f"{pre}{i + 1}.block.", f"b{i}.", 0
        kind, s_res = "hs" if b["hs"] else "relu", s
        if b["expand"]:
            s, z = _quantize_mbv3_layer(arrays, scales, q + "expand", *folded(p + "0", (b["exp"], b["cin"], 1, 1)), s,
                                        b["cin"] * 127 * 255, kind, rng[q + "expand"], rng.get(q + "expand.u"))
            j = 1
        s, z = _quantize_mbv3_layer(arrays, scales, q + "dw", *folded(f"{p}{j}", (b["exp"], 1, b["k"], b["k"])), s,
                                    b["k"] ** 2 * 127 * 255, kind, rng[q + "dw"], rng.get(q + "dw.u"))
        j += 1
        if b["se"]:
            hw = b["hw"][0] * b["hw"][1]
            _one_multiplier(arrays, q + "pool", 1.0 / hw)
            arrays[q + "pool.hw"] = np.array([hw], np.int32)
            s_h, _ = _quantize_mbv3_layer(arrays, scales, q + "fc1", *plain(f"{p}{j}.fc1", (b["se"], b["exp"])), s, b["exp"] * 127 * 255,
                                          "relu", rng[q + "h"], real=q + "h")
            _quantize_mbv3_layer(arrays, scales, q + "fc2", *plain(f"{p}{j}.fc2", (b["exp"], b["se"])), s_h, b["se"] * 127 * 255,
                                 "gate", None, bias_shift=3.0, real=q + "gate")
            _one_multiplier(arrays, q + "gate", 1.0 / 255.0)
            j += 1
        s_y = s
        s, z = _quantize_mbv3_layer(arrays, scales, q + "project", *folded(f"{p}{j}", (b["cout"], b["exp"], 1, 1)), s_y,
                                    b["exp"] * 127 * 255, "signed", rng[q + "out"], real=q + "out")
        if b["res"]:
            _one_multiplier(arrays, q + "res", s_res / s)
    last = mbv3_blocks(F, T)[-1]
    s, z = _quantize_mbv3_layer(arrays, scales, "last", *folded(pre + "12", (MBV3_LAST, last["cout"], 1, 1)), s, last["cout"] * 127 * 255,
                                "hs", rng["last"], rng["last.u"])
    hw = last["hw"][0] * last["hw"][1]
    _one_multiplier(arrays, "pool", 1.0 / hw)
    arrays["pool.hw"] = np.array([hw], np.int32)
    scales["pool"] = s
    s_h, _ = _quantize_mbv3_layer(arrays, scales, "cls0", *plain("mobilenet.classifier.0", (MBV3_HIDDEN, MBV3_LAST)), s, MBV3_LAST * 127 * 255,
                                  "hs", rng["hidden"], rng["cls0.u"], real="hidden")
    fw, fb = plain("mobilenet.classifier.3", (num_classes, MBV3_HIDDEN))
    if not np.isfinite(fw).all():
        raise QuantizationError("classifier: a weight is not finite")
    q_w, s_w = quantize_weights(fw)
    arrays["fc.w"] = q_w
    arrays["fc.b"] = quantize_bias(fb, s_h, s_w, MBV3_HIDDEN * 127 * 255, "classifier")
    arrays["fc.scale"] = (s_h * s_w).astype(np.float32)
    return arrays, scales
