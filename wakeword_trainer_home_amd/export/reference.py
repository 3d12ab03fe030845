"""A pure-NumPy interpreter of an int8 bundle: the int8 law of DESIGN.md "Export", and nothing else.

It imports NumPy and the standard library only -- no torch, no native library, nothing of this package -- so a port of the
bundle to another runtime can be checked against it, tensor by tensor.  It runs on the CPU.

    header, arrays = load_bundle("model_int8.npz")
    out = run_int8(header, arrays, features)          # features (B,1,F,T) or (B,F,T) float32
    out["logits"]                                     # (B,2) float32; the other keys are the int8 tensors of every stage

``run_int8`` dispatches on the header's architecture: ``cnn_small`` (NHWC tensors), ``TCNWakeword`` (``run_int8_tcn``: (B,T,C)
tensors ``xq``, each block's ``b{i}.h1``, ``b{i}.h2``, ``b{i}.out``, then ``pool`` and ``logits`` (B,num_classes)),
``ResNet18Wakeword`` (``run_int8_resnet18``), ``LSTMWakeword`` (``run_int8_lstm``: any number of frames T) or ``crnn``
(``run_int8_crnn``: cnn_small's conv stack, the frequency mean, a GRU stack -- ``run_int8_gru_stack`` --; any T) or ``mobilenetv3``
(``run_int8_mobilenetv3``: Hardswish by table, squeeze-excitation with a uint8 gate, signed bottleneck outputs).
"""
import json

import numpy as np

FORMAT_NAME = "wakeword-bundle"
FORMAT_VERSION = 1
BLOCKS = 4
CONVS = ["stem"] + [f"{kind}{k}" for k in range(BLOCKS) for kind in ("dw", "pw")]     # in execution order
STAGES = ["xq"] + CONVS + ["pool", "logits"]


def load_bundle(path):
    """-> (header dict, {name: array}); ``numpy.load`` without pickle and ``json`` are all a reader needs."""
    with np.load(str(path), allow_pickle=False) as z:
        arrays = {k: z[k] for k in z.files}
    header = json.loads(bytes(arrays.pop("header")).decode("utf-8"))
    return header, arrays


def quantize_input(x, scale, zero):
    """q = clamp(rne(x / s_x) + z_x, -128, 127); the division is one fp32 operation, NaN -> z_x, +-inf saturate."""
    x = np.asarray(x, np.float32)
    with np.errstate(all="ignore"):
        r = np.rint(x / np.float32(scale))                    # float32 / float32: correctly rounded
    r = np.where(np.isnan(r), np.float32(0), np.clip(r, -512, 512))
    return np.clip(r.astype(np.int64) + int(zero), -128, 127).astype(np.int8)


def requantize(acc, mult, shift):
    """clamp(-128 + ((int64(acc) * m + 2^(sh-1)) >> sh), -128, 127): arithmetic shift, round half up."""
    acc = np.asarray(acc, np.int64)
    mult = np.asarray(mult, np.int64)
    shift = np.asarray(shift, np.int64)
    t = (acc * mult + (np.int64(1) << (shift - 1))) >> shift
    return (np.clip(t, 0, 255) - 128).astype(np.int8)


def _wrap32(a):
    return np.asarray(a, np.int64).astype(np.int32).astype(np.int64)


def _conv3x3(q, zero, w, stride):
    """q int8 (B,H,W,C), C == 1 (stem: w (64,9) gives 64 outputs) or 64 (depthwise); pad 1; the padding holds the zero point."""
    B, H, W, _ = q.shape
    d = np.pad(q.astype(np.int64) - int(zero), ((0, 0), (1, 1), (1, 1), (0, 0)))
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    acc = np.zeros((B, Ho, Wo, 64), np.int64)
    for kh in range(3):
        for kw in range(3):
            win = d[:, kh:kh + stride * (Ho - 1) + 1:stride, kw:kw + stride * (Wo - 1) + 1:stride, :]
            acc += win * w[:, kh * 3 + kw].astype(np.int64)
    return acc


def round_shift(a, mult, shift):
    """R(a, m, sh) = (int64(a) * m + 2^(sh-1)) >> sh: arithmetic shift, round half up; no offset, no clamp."""
    a, mult, shift = np.asarray(a, np.int64), np.asarray(mult, np.int64), np.asarray(shift, np.int64)
    return (a * mult + (np.int64(1) << (shift - 1))) >> shift


def _clamp8(v):
    """clamp(-128 + v, -128, 127)"""
    return (np.clip(v, 0, 255) - 128).astype(np.int8)


def tcn_blocks(tcn):
    """[(block, Cin, Cout, dilation, has a downsample conv)] of a header's ``tcn`` entry."""
    out, cin = [], int(tcn["input_size"])
    for i, c in enumerate(tcn["num_channels"]):
        out.append((i, cin, int(c), 2 ** i, cin != int(c)))
        cin = int(c)
    return out


def tcn_stages(tcn):
    return ["xq"] + [f"b{i}.{s}" for i in range(len(tcn["num_channels"])) for s in ("h1", "h2", "out")] + ["pool", "logits"]


def _causal_conv(q, zero, w, dilation):
    """sum_j sum_c w[n,c,j] (q[b, t - (k-1-j) d, c] - zero) -> int64 (B,T,Cout); source times below 0 contribute nothing.
    The channel sums are float64 matrix products of integers below 2^8 -- at most k Cin 127 255 < 2^53 in all, so exact."""
    B, T, _ = q.shape
    k = w.shape[2]
    d = q.astype(np.float64) - float(zero)
    acc = np.zeros((B, T, w.shape[0]), np.float64)
    for j in range(k):
        off = (k - 1 - j) * dilation
        if off < T:
            acc[:, off:] += d[:, :T - off] @ w[:, :, j].astype(np.float64).T
    return acc.astype(np.int64)


def run_int8_tcn(header, arrays, x, want_acc=False):
    """Every stage of an int8 TCNWakeword bundle: ``xq`` (B,T,F), each block's ``b{i}.h1``, ``b{i}.h2``, ``b{i}.out`` (B,T,C),
    ``pool`` (B,C), ``logits`` float32; with ``want_acc`` also the int64 accumulators ``acc/b{i}.conv1|conv2|down``."""
    x = np.asarray(x, np.float32)
    if x.ndim == 4:
        x = x[:, 0]
    F, T = header["feature_shape"]
    if x.ndim != 3 or tuple(x.shape[1:]) != (F, T):
        raise ValueError(f"this bundle is for features of shape ({F},{T}), got {tuple(x.shape)}")
    a, out = arrays, {}
    zero = int(a["input_zero"][0])
    q = np.ascontiguousarray(quantize_input(x, a["input_scale"][0], zero).transpose(0, 2, 1))
    out["xq"] = q
    for i, _, _, d, down in tcn_blocks(header["tcn"]):
        p = f"b{i}."
        acc1 = _wrap32(_causal_conv(q, zero, a[p + "conv1.w"], d) + a[p + "conv1.b"].astype(np.int64))
        h1 = requantize(acc1, a[p + "conv1.m"], a[p + "conv1.sh"])
        acc2 = _wrap32(_causal_conv(h1, -128, a[p + "conv2.w"], d) + a[p + "conv2.b"].astype(np.int64))
        h2 = requantize(acc2, a[p + "conv2.m"], a[p + "conv2.sh"])
        if down:
            accd = _wrap32(_causal_conv(q, zero, a[p + "down.w"], 1) + a[p + "down.b"].astype(np.int64))
            skip = round_shift(accd, a[p + "down.m"], a[p + "down.sh"])
        else:
            skip = round_shift(q.astype(np.int64) - zero, a[p + "skip.m"][0], a[p + "skip.sh"][0])
        q = _clamp8(skip + round_shift(h2.astype(np.int64) + 128, a[p + "add.m"][0], a[p + "add.sh"][0]))
        zero = -128
        out[p + "h1"], out[p + "h2"], out[p + "out"] = h1, h2, q
        if want_acc:
            out["acc/" + p + "conv1"], out["acc/" + p + "conv2"] = acc1, acc2
            if down:
                out["acc/" + p + "down"] = accd
    S = _wrap32((q.astype(np.int64) + 128).sum(axis=1))
    pool = requantize(S, a["pool.m"][0], a["pool.sh"][0])
    out["pool"] = pool
    acc = _wrap32((pool.astype(np.int64) + 128) @ a["fc.w"].astype(np.int64).T + a["fc.b"].astype(np.int64))
    out["logits"] = acc.astype(np.float32) * a["fc.scale"].astype(np.float32)
    return out


RESNET_PLANES = (64, 128, 256, 512)


def resnet_half(n):
    """The output size of a stride-2 layer of the ResNet: floor((n + 2p - k) / 2) + 1 is (n - 1) // 2 + 1 for (k, p) = (7, 3),
    (3, 1) and (1, 0) alike."""
    return (int(n) - 1) // 2 + 1


def resnet_blocks():
    """[(name 'l{s}.{b}', Cin, Cout, stride, has a downsample conv)] of the eight BasicBlocks, in execution order."""
    out, cin = [], 64
    for s, planes in enumerate(RESNET_PLANES):
        for b in range(2):
            first = b == 0 and s > 0
            out.append((f"l{s + 1}.{b}", cin, planes, 2 if first else 1, first))
            cin = planes
    return out


def resnet_stages():
    out = ["xq", "stem", "pool0"]
    for name, _, _, _, down in resnet_blocks():
        out += [name + ".h1"] + ([name + ".ds"] if down else []) + [name + ".out"]
    return out + ["pool", "logits"]


def _conv2d(q, zero, w, stride):
    """sum_{kh,kw,c} w[n,c,kh,kw] (q[b, ho s - p + kh, wo s - p + kw, c] - zero) -> int64 (B,Ho,Wo,Cout), p = k // 2; positions
    outside the image contribute nothing (the padding of q - zero is 0).  The channel sums are float64 matrix products of
    integers below 2^8 -- at most k k Cin 127 255 < 2^53 in all, so exact."""
    B, H, W, _ = q.shape
    k = w.shape[2]
    p = k // 2
    Ho, Wo = (H + 2 * p - k) // stride + 1, (W + 2 * p - k) // stride + 1
    d = np.pad(q.astype(np.float64) - float(zero), ((0, 0), (p, p), (p, p), (0, 0)))
    acc = np.zeros((B, Ho, Wo, w.shape[0]), np.float64)
    for kh in range(k):
        for kw in range(k):
            win = d[:, kh:kh + stride * (Ho - 1) + 1:stride, kw:kw + stride * (Wo - 1) + 1:stride, :]
            acc += win @ w[:, :, kh, kw].astype(np.float64).T
    return acc.astype(np.int64)


def _maxpool3x3s2(q):
    """The maximum of q over the 3x3 stride-2 pad-1 window's positions inside the image (the padding can never win)."""
    B, H, W, C = q.shape
    Ho, Wo = resnet_half(H), resnet_half(W)
    d = np.pad(q.astype(np.int16), ((0, 0), (1, 1), (1, 1), (0, 0)), constant_values=-129)
    out = np.full((B, Ho, Wo, C), -129, np.int16)
    for kh in range(3):
        for kw in range(3):
            out = np.maximum(out, d[:, kh:kh + 2 * (Ho - 1) + 1:2, kw:kw + 2 * (Wo - 1) + 1:2, :])
    return out.astype(np.int8)


def run_int8_resnet18(header, arrays, x, want_acc=False):
    """Every stage of an int8 ResNet18Wakeword bundle, NHWC: ``xq`` (B,F,T), ``stem``, ``pool0``, per block ``l{s}.{b}.h1``,
    ``l{s}.{b}.ds`` (int8 with zero point 0; blocks 0 of stages 2-4) and ``l{s}.{b}.out``, ``pool`` (B,512), ``logits`` float32;
    with ``want_acc`` also the int64 accumulators ``acc/stem`` and ``acc/l{s}.{b}.conv1|conv2|down``."""
    x = np.asarray(x, np.float32)
    if x.ndim == 4:
        x = x[:, 0]
    F, T = header["feature_shape"]
    if x.ndim != 3 or tuple(x.shape[1:]) != (F, T):
        raise ValueError(f"this bundle is for features of shape ({F},{T}), got {tuple(x.shape)}")
    a, out = arrays, {}
    z_x = int(a["input_zero"][0])
    xq = quantize_input(x, a["input_scale"][0], z_x)
    out["xq"] = xq

    def conv(name, q, zero, stride):
        acc = _wrap32(_conv2d(q, zero, a[name + ".w"], stride) + a[name + ".b"].astype(np.int64))
        if want_acc:
            out["acc/" + name] = acc
        return acc
    q = requantize(conv("stem", xq[..., None], z_x, 2), a["stem.m"], a["stem.sh"])
    out["stem"] = q
    q = _maxpool3x3s2(q)
    out["pool0"] = q
    for name, _, _, stride, down in resnet_blocks():
        h1 = requantize(conv(name + ".conv1", q, -128, stride), a[name + ".conv1.m"], a[name + ".conv1.sh"])
        out[name + ".h1"] = h1
        if down:
            r = round_shift(conv(name + ".down", q, -128, stride), a[name + ".down.m"], a[name + ".down.sh"])
            res = np.clip(r, -128, 127).astype(np.int8)
            out[name + ".ds"] = res
            z_res = 0
        else:
            res, z_res = q, -128
        t = round_shift(conv(name + ".conv2", h1, -128, 1), a[name + ".conv2.m"], a[name + ".conv2.sh"])
        q = _clamp8(t + round_shift(res.astype(np.int64) - z_res, a[name + ".res.m"][0], a[name + ".res.sh"][0]))
        out[name + ".out"] = q
    S = _wrap32((q.astype(np.int64) + 128).sum(axis=(1, 2)))
    pool = requantize(S, a["pool.m"][0], a["pool.sh"][0])
    out["pool"] = pool
    acc = _wrap32((pool.astype(np.int64) + 128) @ a["fc.w"].astype(np.int64).T + a["fc.b"].astype(np.int64))
    out["logits"] = acc.astype(np.float32) * a["fc.scale"].astype(np.float32)
    return out


LSTM_HIDDEN, LSTM_TABLE, LSTM_DIRS = 128, 4096, ("fwd", "rev")


def _rnn_stack_stages(args, state):
    """Per layer and direction ``l{l}.{fwd|rev}.u``, ``.y`` and the final state ``.c`` / ``.h``."""
    dirs = LSTM_DIRS if args["bidirectional"] else LSTM_DIRS[:1]
    return [f"l{k}.{d}.{s}" for k in range(int(args["num_layers"])) for d in dirs for s in ("u", "y", state)]


def lstm_stages(lstm):
    """``xq``, per layer and direction ``l{l}.{fwd|rev}.u``, ``.y`` and ``.c``, then ``hcat`` and ``logits``."""
    return ["xq"] + _rnn_stack_stages(lstm, "c") + ["hcat", "logits"]


def look(tab, a):
    """tab[clamp(a, -2048, 2047) + 2048] as int64: the bundle's int16 table is data, never recomputed."""
    return tab[np.clip(a, -2048, 2047) + 2048].astype(np.int64)


def _exact_matmul(q, w):
    """q (.., K) x w (N, K)^T of integers below 2^8 as a float64 matrix product: at most K 127 255 < 2^53, so exact."""
    return (q.astype(np.float64) @ w.astype(np.float64).T).astype(np.int64)


def _lstm_step(sig, tanh, u, v, c):
    """One LSTM step on Q8 pre-activations u + v (B,512), gate order i, f, g, o; the state is the cell c.  -> (c, h16)."""
    H, g_in = LSTM_HIDDEN, u + v
    i, f = look(sig, g_in[:, :H]), look(sig, g_in[:, H:2 * H])
    g, o = look(tanh, g_in[:, 2 * H:3 * H]), look(sig, g_in[:, 3 * H:])
    c = np.clip((f * c + ((i * g + 8) >> 4) + 2 ** 14) >> 15, -32768, 32767)
    return c, (o * look(tanh, (c + 4) >> 3) + 2 ** 14) >> 15


def _gru_step(sig, tanh, u, v, h16):
    """One GRU step on the Q8 input part u and hidden part v (B,384), gate order r, z, n; the state is h16.  -> (h16, h16)."""
    H = LSTM_HIDDEN
    r, z = look(sig, u[:, :H] + v[:, :H]), look(sig, u[:, H:2 * H] + v[:, H:2 * H])
    n = look(tanh, u[:, 2 * H:] + ((r * v[:, 2 * H:] + 2 ** 14) >> 15))
    h16 = ((32768 - z) * n + z * h16 + 2 ** 14) >> 15
    return h16, h16


LSTM_CELL, GRU_CELL = ("c", _lstm_step), ("h", _gru_step)      # the name of the final state among the stages, the step


def run_int8_gru_stack(arrays, q_in, z_in, args, cell=GRU_CELL):
    """The recurrent stack of the law's subsections "GRU" (the default ``cell``) and "LSTM" on int8 rows ``q_in`` (B,T,K) with
    zero point ``z_in``; ``args``: ``num_layers``, ``bidirectional``.  -> ({``l{l}.{fwd|rev}.u`` (B,T,384 | 512) int16 (the input
    projection in Q8, gate order r, z, n | i, f, g, o), ``.y`` (B,T,128) int8 (q_h at every step, in time order), ``.h`` | ``.c``
    (B,128) int16 (h16 | the cell after the direction's last step)}, hcat (B, nd 128) int8)."""
    a, out, H = arrays, {}, LSTM_HIDDEN
    state, step = cell
    dirs = LSTM_DIRS if args["bidirectional"] else LSTM_DIRS[:1]
    sig, tanh = a["tab.sigmoid"], a["tab.tanh"]
    L = int(args["num_layers"])
    q_in, z_in = np.asarray(q_in), int(z_in)
    B, T, _ = q_in.shape
    hcat = []
    for k in range(L):
        ys = []
        for d in dirs:
            p = f"l{k}.{d}"
            acc = _wrap32(_exact_matmul(q_in.astype(np.int64) - z_in, a[p + ".ih.w"]) + a[p + ".ih.b"].astype(np.int64))
            u = np.clip(round_shift(acc, a[p + ".ih.m"], a[p + ".ih.sh"]), -32768, 32767)
            y = np.zeros((B, T, H), np.int8)
            q_h, s = np.zeros((B, H), np.int64), np.zeros((B, H), np.int64)
            for t in (range(T) if d == "fwd" else range(T - 1, -1, -1)):
                acc = _wrap32(_exact_matmul(q_h, a[p + ".hh.w"]) + a[p + ".hh.b"].astype(np.int64))
                s, h16 = step(sig, tanh, u[:, t], round_shift(acc, a[p + ".hh.m"], a[p + ".hh.sh"]), s)
                q_h = np.clip((h16 + 128) >> 8, -128, 127)
                y[:, t] = q_h
            out[p + ".u"], out[p + ".y"], out[f"{p}.{state}"] = u.astype(np.int16), y, s.astype(np.int16)
            ys.append(y)
            if k == L - 1:
                hcat.append(y[:, T - 1] if d == "fwd" else y[:, 0])
        q_in, z_in = np.concatenate(ys, axis=2), 0
    return out, np.concatenate(hcat, axis=1)


def run_int8_lstm(header, arrays, x, want_acc=False):
    """Every stage of an int8 LSTMWakeword bundle on (B,1,F,T) features or (B,T,F) sequences, any T >= 1: ``xq`` (B,T,F) int8; per
    layer and direction ``l{l}.{fwd|rev}.u`` (B,T,512) int16 (the input projection in Q8, gate order i, f, g, o), ``.y`` (B,T,128)
    int8 (q_h at every step, in time order) and ``.c`` (B,128) int16 (the cell after the direction's last step); ``hcat``
    (B, nd 128) int8; ``logits`` float32.  ``want_acc`` adds nothing: the law has no hidden accumulators beyond ``u``."""
    x = np.asarray(x, np.float32)
    F = int(header["lstm"]["input_size"])
    if x.ndim == 4 and x.shape[1] == 1:
        x = x[:, 0].transpose(0, 2, 1)
    if x.ndim != 3 or x.shape[2] != F or x.shape[1] < 1:
        raise ValueError(f"this bundle is for features of shape (B,1,{F},T) or sequences (B,T,{F}), got {tuple(x.shape)}")
    a = arrays
    z_in = int(a["input_zero"][0])
    out = {"xq": np.ascontiguousarray(quantize_input(x, a["input_scale"][0], z_in))}
    stack, hcat = run_int8_gru_stack(a, out["xq"], z_in, header["lstm"], LSTM_CELL)
    out.update(stack)
    out["hcat"] = hcat
    acc = _wrap32(_exact_matmul(hcat, a["fc.w"]) + a["fc.b"].astype(np.int64))
    out["logits"] = acc.astype(np.float32) * a["fc.scale"].astype(np.float32)
    return out


def gru_stack_stages(args):
    """Per layer and direction ``l{l}.{fwd|rev}.u``, ``.y`` and ``.h``."""
    return _rnn_stack_stages(args, "h")


def crnn_stages(crnn):
    return ["xq"] + ["front." + c for c in CONVS] + ["seq"] + gru_stack_stages(crnn) + ["hcat", "logits"]


def run_int8_crnn(header, arrays, x, want_acc=False):
    """Every stage of an int8 CRNNWakeword bundle on (B,1,F,T) or (B,F,T) features, F the bundle's, any T >= 1: ``xq`` (B,F,T)
    int8; the nine conv tensors ``front.<conv>`` (B,H',W',64) int8 NHWC; ``seq`` (B,W',64) int8, the frequency mean; the GRU stack's
    tensors (``run_int8_gru_stack``); ``hcat``; ``logits`` float32.  With ``want_acc`` also ``acc/front.<conv>``."""
    x = np.asarray(x, np.float32)
    if x.ndim == 4 and x.shape[1] == 1:
        x = x[:, 0]
    F = int(header["feature_shape"][0])
    if x.ndim != 3 or x.shape[1] != F or x.shape[2] < 1:
        raise ValueError(f"this bundle is for features of shape (B,1,{F},T), got {tuple(x.shape)}")
    a, out = arrays, {}
    z_x = int(a["input_zero"][0])
    q = quantize_input(x, a["input_scale"][0], z_x)
    out["xq"] = q
    q, zero = q[..., None], z_x
    for name in CONVS:
        w = a[f"front.{name}.w"]
        if name == "stem":
            acc = _conv3x3(q, zero, w, 2)
        elif name.startswith("dw"):
            acc = _conv3x3(q, zero, w, 1)
        else:
            acc = (q.astype(np.int64) - zero) @ w.astype(np.int64).T
        acc = _wrap32(acc + a[f"front.{name}.b"].astype(np.int64))
        q, zero = requantize(acc, a[f"front.{name}.m"], a[f"front.{name}.sh"]), -128
        out["front." + name] = q
        if want_acc:
            out["acc/front." + name] = acc
    S = _wrap32((q.astype(np.int64) + 128).sum(axis=1))                  # over the frequency axis H': (B,W',64)
    seq = requantize(S, a["fmean.m"][0], a["fmean.sh"][0])
    out["seq"] = seq
    stack, hcat = run_int8_gru_stack(a, seq, -128, header["crnn"])
    out.update(stack)
    out["hcat"] = hcat
    acc = _wrap32(_exact_matmul(hcat, a["fc.w"]) + a["fc.b"].astype(np.int64))
    out["logits"] = acc.astype(np.float32) * a["fc.scale"].astype(np.float32)
    return out


MBV3_CONF = ((16, 3, 16, 16, True, "RE", 2), (16, 3, 72, 24, False, "RE", 2), (24, 3, 88, 24, False, "RE", 1),
             (24, 5, 96, 40, True, "HS", 2), (40, 5, 240, 40, True, "HS", 1), (40, 5, 240, 40, True, "HS", 1),
             (40, 5, 120, 48, True, "HS", 1), (48, 5, 144, 48, True, "HS", 1), (48, 5, 288, 96, True, "HS", 2),
             (96, 5, 576, 96, True, "HS", 1), (96, 5, 576, 96, True, "HS", 1))      # mobilenet_v3_small: cin, k, exp, cout, SE, act, stride
MBV3_STEM, MBV3_LAST, MBV3_HIDDEN = 16, 576, 1024
GATE_MULT, GATE_SHIFT = 1077952576, 38         # the encoding of 1 / 255


def mbv3_blocks(F, T):
    """[dict] of the eleven inverted-residual blocks on (F, T) features, in execution order: ``cin``, ``k``, ``exp``, ``cout``,
    ``se`` (its squeeze width, or 0), ``hs`` (Hardswish, else ReLU), ``stride``, ``expand`` (has an expand conv), ``res`` (has a
    skip connection), ``hw_in`` and ``hw`` (the image before and after the depthwise conv)."""
    hw, out = (resnet_half(F), resnet_half(T)), []
    for cin, k, exp, cout, se, act, stride in MBV3_CONF:
        nxt = (resnet_half(hw[0]), resnet_half(hw[1])) if stride == 2 else hw
        sq = max(8, (exp // 4 + 4) // 8 * 8)
        if sq < 0.9 * (exp // 4):
            sq += 8
        out.append({"cin": cin, "k": k, "exp": exp, "cout": cout, "se": sq if se else 0, "hs": act == "HS", "stride": stride,
                    "expand": exp != cin, "res": stride == 1 and cin == cout, "hw_in": hw, "hw": nxt})
        hw = nxt
    return out


def mbv3_stages(want=("expand", "dw", "pool", "h", "gate", "y", "out")):
    """The stage tensors of ``run_int8_mobilenetv3`` in execution order."""
    out = ["xq", "stem"]
    for i, b in enumerate(mbv3_blocks(1, 1)):
        have = {"expand": b["expand"], "dw": True, "pool": b["se"], "h": b["se"], "gate": b["se"], "y": b["se"], "out": True}
        out += [f"b{i}.{s}" for s in want if have[s]]
    return out + ["last", "pool", "hidden", "logits"]


def mbv3_range_names():
    """The calibrated tensors of a MobileNetV3 bundle, in execution order; ``<layer>.u`` is a Hardswish pre-activation."""
    out = ["stem.u", "stem"]
    for i, b in enumerate(mbv3_blocks(1, 1)):
        for layer in (["expand"] if b["expand"] else []) + ["dw"]:
            out += ([f"b{i}.{layer}.u"] if b["hs"] else []) + [f"b{i}.{layer}"]
        out += ([f"b{i}.h"] if b["se"] else []) + [f"b{i}.out"]
    return out + ["last.u", "last", "cls0.u", "hidden"]


def _dwconv(q, zero, w, k, stride):
    """sum_{kh,kw} w[c, kh k + kw] (q[b, ho s - p + kh, wo s - p + kw, c] - zero) -> int64 (B,Ho,Wo,C), p = k // 2; positions outside
    the image contribute nothing.  q has C channels, or one (the stem: every output channel reads it)."""
    B, H, W, _ = q.shape
    p = k // 2
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    d = np.pad(q.astype(np.int64) - int(zero), ((0, 0), (p, p), (p, p), (0, 0)))
    acc = np.zeros((B, Ho, Wo, w.shape[0]), np.int64)
    for kh in range(k):
        for kw in range(k):
            win = d[:, kh:kh + stride * (Ho - 1) + 1:stride, kw:kw + stride * (Wo - 1) + 1:stride, :]
            acc += win * w[:, kh * k + kw].astype(np.int64)
    return acc


def run_int8_mobilenetv3(header, arrays, x, want_acc=False):
    """Every stage of an int8 MobileNetV3Wakeword bundle, NHWC (the law's subsection "MobileNetV3"): ``xq`` (B,F,T), ``stem``, per
    block ``b{i}.expand`` (where the block has one), ``b{i}.dw``, the squeeze-excitation's ``b{i}.pool`` (B,C), ``b{i}.h`` (B,Csq),
    ``b{i}.gate`` (B,C) uint8 and ``b{i}.y``, ``b{i}.out`` (zero point 0); ``last``, ``pool`` (B,576), ``hidden`` (B,1024), ``logits``
    float32.  With ``want_acc`` also the accumulators ``acc/<layer>`` and the Hardswish pre-activations ``u/<layer>``."""
    x = np.asarray(x, np.float32)
    if x.ndim == 4:
        x = x[:, 0]
    F, T = header["feature_shape"]
    if x.ndim != 3 or tuple(x.shape[1:]) != (F, T):
        raise ValueError(f"this bundle is for features of shape ({F},{T}), got {tuple(x.shape)}")
    a, out = arrays, {}

    def finish(name, acc, kind, res=None):
        """the three epilogues: -> (int8 tensor, its zero point)"""
        acc = _wrap32(acc + a[name + ".b"].astype(np.int64))
        if want_acc:
            out["acc/" + name] = acc
        r = round_shift(acc, a[name + ".m"], a[name + ".sh"])
        if kind == "relu":
            return _clamp8(r), -128
        if kind == "signed":
            return np.clip(r if res is None else r + res, -128, 127).astype(np.int8), 0
        u = np.clip(int(a[name + ".zu"][0]) + r, -128, 127)
        if want_acc:
            out["u/" + name] = u.astype(np.int8)
        return a[name + ".tab"][u + 128], int(a[name + ".zo"][0])

    def pool(q, zero, name):
        S = _wrap32((q.astype(np.int64) - zero).sum(axis=(1, 2)))
        return np.clip(zero + round_shift(S, a[name + ".m"][0], a[name + ".sh"][0]), -128, 127).astype(np.int8)
    z_x = int(a["input_zero"][0])
    xq = quantize_input(x, a["input_scale"][0], z_x)
    out["xq"] = xq
    q, z = finish("stem", _dwconv(xq[..., None], z_x, a["stem.w"], 3, 2), "hs")
    out["stem"] = q
    for i, b in enumerate(mbv3_blocks(F, T)):
        p, act, q_in = f"b{i}.", "hs" if b["hs"] else "relu", q
        if b["expand"]:
            q, z = finish(p + "expand", _exact_matmul(q.astype(np.int64) - z, a[p + "expand.w"]), act)
            out[p + "expand"] = q
        q, z = finish(p + "dw", _dwconv(q, z, a[p + "dw.w"], b["k"], b["stride"]), act)
        out[p + "dw"] = q
        if b["se"]:
            sq = pool(q, z, p + "pool")
            h, _ = finish(p + "fc1", _exact_matmul(sq.astype(np.int64) - z, a[p + "fc1.w"]), "relu")
            acc2 = _wrap32(_exact_matmul(h.astype(np.int64) + 128, a[p + "fc2.w"]) + a[p + "fc2.b"].astype(np.int64))
            gate = np.clip(round_shift(acc2, a[p + "fc2.m"], a[p + "fc2.sh"]), 0, 255)
            y = (q.astype(np.int64) - z) * gate[:, None, None, :]
            q = np.clip(z + round_shift(y, a[p + "gate.m"][0], a[p + "gate.sh"][0]), -128, 127).astype(np.int8)
            out[p + "pool"], out[p + "h"], out[p + "gate"], out[p + "y"] = sq, h, gate.astype(np.uint8), q
            if want_acc:
                out["acc/" + p + "fc2"] = acc2
        res = round_shift(q_in.astype(np.int64), a[p + "res.m"][0], a[p + "res.sh"][0]) if b["res"] else None
        q, z = finish(p + "project", _exact_matmul(q.astype(np.int64) - z, a[p + "project.w"]), "signed", res)
        out[p + "out"] = q
    q, z = finish("last", _exact_matmul(q.astype(np.int64), a["last.w"]), "hs")
    out["last"] = q
    pq = pool(q, z, "pool")
    out["pool"] = pq
    hid, z_h = finish("cls0", _exact_matmul(pq.astype(np.int64) - z, a["cls0.w"]), "hs")
    out["hidden"] = hid
    acc = _wrap32(_exact_matmul(hid.astype(np.int64) - z_h, a["fc.w"]) + a["fc.b"].astype(np.int64))
    if want_acc:
        out["acc/fc"] = acc
    out["logits"] = acc.astype(np.float32) * a["fc.scale"].astype(np.float32)
    return out


def run_int8(header, arrays, x, want_acc=False):
    """Every stage of the int8 network on features ``x``, by the bundle's architecture.  ``cnn_small``: dict of STAGES (int8
    NHWC tensors, ``pool`` (B,64), ``logits``); ``TCNWakeword``: ``run_int8_tcn``; ``ResNet18Wakeword``: ``run_int8_resnet18``;
    ``LSTMWakeword``: ``run_int8_lstm``; ``crnn``: ``run_int8_crnn``; ``mobilenetv3``: ``run_int8_mobilenetv3``.  ``want_acc`` adds the
    accumulators."""
    if header.get("architecture") == "crnn":
        return run_int8_crnn(header, arrays, x, want_acc)
    if header.get("architecture") == "mobilenetv3":
        return run_int8_mobilenetv3(header, arrays, x, want_acc)
    if header.get("architecture") == "LSTMWakeword":
        return run_int8_lstm(header, arrays, x, want_acc)
    if header.get("architecture") == "TCNWakeword":
        return run_int8_tcn(header, arrays, x, want_acc)
    if header.get("architecture") == "ResNet18Wakeword":
        return run_int8_resnet18(header, arrays, x, want_acc)
    x = np.asarray(x, np.float32)
    if x.ndim == 4:
        x = x[:, 0]
    F, T = header["feature_shape"]
    if x.ndim != 3 or tuple(x.shape[1:]) != (F, T):
        raise ValueError(f"this bundle is for features of shape ({F},{T}), got {tuple(x.shape)}")
    a = arrays
    out = {}
    z_x = int(a["input_zero"][0])
    q = quantize_input(x, a["input_scale"][0], z_x)
    out["xq"] = q
    q, zero = q[..., None], z_x
    for name in CONVS:
        w = a[name + ".w"]
        if name == "stem":
            acc = _conv3x3(q, zero, w, 2)
        elif name.startswith("dw"):
            acc = _conv3x3(q, zero, w, 1)
        else:
            acc = (q.astype(np.int64) - zero) @ w.astype(np.int64).T
        acc = _wrap32(acc + a[name + ".b"].astype(np.int64))
        q, zero = requantize(acc, a[name + ".m"], a[name + ".sh"]), -128
        out[name] = q
        if want_acc:
            out["acc/" + name] = acc
    S = _wrap32((q.astype(np.int64) + 128).sum(axis=(1, 2)))
    p = requantize(S, a["pool.m"][0], a["pool.sh"][0])
    out["pool"] = p
    acc = _wrap32((p.astype(np.int64) + 128) @ a["fc.w"].astype(np.int64).T + a["fc.b"].astype(np.int64))
    out["logits"] = acc.astype(np.float32) * a["fc.scale"].astype(np.float32)
    return out
