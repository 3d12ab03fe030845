"""The bundle file: one ``.npz`` whose ``header`` entry is UTF-8 JSON (stored as bytes, so nothing in the file is pickled)
and whose other entries are plain arrays.  ``numpy.load`` and ``json`` read it; ``check_bundle`` says whether it is whole."""
import json
from pathlib import Path

import numpy as np

from .reference import (CONVS, FORMAT_NAME, FORMAT_VERSION, LSTM_DIRS, LSTM_HIDDEN, LSTM_TABLE, MBV3_HIDDEN, MBV3_LAST, MBV3_STEM,
                        load_bundle, mbv3_blocks, resnet_blocks)  # noqa: F401  (load_bundle is re-exported)

STATE_PREFIX = "state/"
FP16_MAX = 65504.0


class BundleError(ValueError):
    """A bundle that is not what its header says: a missing array, a wrong shape or dtype, an unknown version, a value out
    of its range."""


def write_bundle(path, header: dict, arrays: dict) -> Path:
    path = Path(path)
    blob = np.frombuffer(json.dumps(header, sort_keys=True).encode("utf-8"), dtype=np.uint8)
    with open(path, "wb") as f:                       # an open file: numpy appends no ".npz" to the name it was given
        np.savez(f, header=blob, **arrays)
    return path


def make_header(kind: str, architecture: str, num_classes: int, input_shape, layers, config=None, **more) -> dict:
    h = {"format": FORMAT_NAME, "version": FORMAT_VERSION, "kind": kind, "architecture": architecture,
         "num_classes": int(num_classes), "input_shape": [int(v) for v in input_shape], "layers": list(layers)}
    if config is not None:
        h.update(opset_version=int(config.opset_version), dynamic_batch=bool(config.dynamic_batch), optimize=bool(config.optimize))
    h.update(more)
    return h


def to_fp16(a: np.ndarray) -> np.ndarray:
    """Round to nearest even, saturating at +-65504 (a NaN stays a NaN)."""
    return np.clip(np.asarray(a, np.float32), -FP16_MAX, FP16_MAX).astype(np.float16)


def float_arrays(state: dict, fp16: bool) -> dict:
    """state_dict (NumPy) -> bundle arrays; with ``fp16`` every floating tensor is narrowed, the others stay as they are."""
    out = {}
    for k, v in state.items():
        v = np.asarray(v)
        out[STATE_PREFIX + k] = to_fp16(v) if fp16 and np.issubdtype(v.dtype, np.floating) else v
    return out


def _need(arrays, name, dtype, shape):
    if name not in arrays:
        raise BundleError(f"array {name!r} is missing")
    a = arrays[name]
    if a.dtype != np.dtype(dtype):
        raise BundleError(f"array {name!r} is {a.dtype}, expected {np.dtype(dtype)}")
    if tuple(a.shape) != tuple(shape):
        raise BundleError(f"array {name!r} has shape {tuple(a.shape)}, expected {tuple(shape)}")
    return a


def _check_mult(arrays, prefix, n):
    m, sh = _need(arrays, prefix + ".m", np.int32, (n,)), _need(arrays, prefix + ".sh", np.int32, (n,))
    if (m < 2 ** 30).any():
        raise BundleError(f"{prefix}.m: a multiplier outside [2^30, 2^31)")
    if (sh < 1).any() or (sh > 62).any():
        raise BundleError(f"{prefix}.sh: a shift outside [1, 62]")


def _check_fc(arrays, nc, K):
    w = _need(arrays, "fc.w", np.int8, (nc, K))
    if (w == -128).any():
        raise BundleError("fc.w holds -128: weights are symmetric, in [-127, 127]")
    _need(arrays, "fc.b", np.int32, (nc,))
    if not np.isfinite(_need(arrays, "fc.scale", np.float32, (nc,))).all():
        raise BundleError("fc.scale is not finite")


def check_tcn_entry(header: dict):
    """The header's ``tcn`` entry as (input_size, [channels], kernel_size), within the limits of the int8 TCN path."""
    tcn = header.get("tcn")
    if not (isinstance(tcn, dict) and all(k in tcn for k in ("input_size", "num_channels", "kernel_size"))):
        raise BundleError(f"the tcn entry {tcn!r} is not {{input_size, num_channels, kernel_size}}")
    F, ch, k = tcn["input_size"], tcn["num_channels"], tcn["kernel_size"]
    if not (isinstance(ch, list) and 1 <= len(ch) <= 8 and all(isinstance(c, int) for c in ch) and isinstance(F, int)
            and isinstance(k, int)):
        raise BundleError(f"the tcn entry {tcn!r}: 1..8 integer channel counts, an integer input_size and kernel_size")
    if any(c < 4 or c % 4 for c in [F] + ch) or not 1 <= k <= 8:
        raise BundleError(f"the tcn entry {tcn!r}: channel counts are positive multiples of 4, 1 <= kernel_size <= 8")
    return F, ch, k


def _check_tcn(header, arrays, fs):
    F, ch, k = check_tcn_entry(header)
    nc = header["num_classes"]
    if not (isinstance(nc, int) and 2 <= nc <= 64):
        raise BundleError(f"num_classes {nc!r} is outside [2, 64]")
    if fs[0] != F:
        raise BundleError(f"feature_shape {fs!r} does not have the TCN's {F} features per frame")
    cin = F
    for i, c in enumerate(ch):
        convs = [("conv1", cin, k), ("conv2", c, k)] + ([("down", cin, 1)] if cin != c else [])
        for name, ci, kk in convs:
            p = f"b{i}.{name}"
            w = _need(arrays, p + ".w", np.int8, (c, ci, kk))
            if (w == -128).any():
                raise BundleError(f"{p}.w holds -128: weights are symmetric, in [-127, 127]")
            _need(arrays, p + ".b", np.int32, (c,))
            _check_mult(arrays, p, c)
        if cin == c:
            _check_mult(arrays, f"b{i}.skip", 1)
        _check_mult(arrays, f"b{i}.add", 1)
        cin = c
    _check_mult(arrays, "pool", 1)
    _check_fc(arrays, nc, cin)


def _check_resnet18(header, arrays):
    nc = header["num_classes"]
    if not (isinstance(nc, int) and 2 <= nc <= 64):
        raise BundleError(f"num_classes {nc!r} is outside [2, 64]")
    convs = [("stem", 64, 1, 7)]
    for name, cin, cout, _, down in resnet_blocks():
        convs += [(name + ".conv1", cout, cin, 3), (name + ".conv2", cout, cout, 3)] + ([(name + ".down", cout, cin, 1)] if down else [])
        _check_mult(arrays, name + ".res", 1)
    for p, cout, cin, k in convs:
        w = _need(arrays, p + ".w", np.int8, (cout, cin, k, k))
        if (w == -128).any():
            raise BundleError(f"{p}.w holds -128: weights are symmetric, in [-127, 127]")
        _need(arrays, p + ".b", np.int32, (cout,))
        _check_mult(arrays, p, cout)
    _check_mult(arrays, "pool", 1)
    _check_fc(arrays, nc, 512)


def _check_rnn_entry(header, key, with_input):
    e = header.get(key)
    keys = (("input_size",) if with_input else ()) + ("hidden_size", "num_layers", "bidirectional")
    if not (isinstance(e, dict) and all(k in e for k in keys)):
        raise BundleError(f"the {key} entry {e!r} is not {{{', '.join(keys)}}}")
    *ints, bi = (e[k] for k in keys)
    if not (all(isinstance(v, int) and not isinstance(v, bool) for v in ints) and isinstance(bi, bool)):
        raise BundleError(f"the {key} entry {e!r}: integer {', '.join(keys[:-2])} and num_layers, a boolean bidirectional")
    *I, H, L = ints
    if H != LSTM_HIDDEN or not 1 <= L <= 8 or any(v < 1 for v in I):
        raise BundleError(f"the {key} entry {e!r}: hidden_size {LSTM_HIDDEN}, 1..8 layers" + (", a positive input_size" if I else ""))
    return (*I, L, 2 if bi else 1)


def check_lstm_entry(header: dict):
    """The header's ``lstm`` entry as (input_size, num_layers, num_directions), within the limits of ``LSTMWakeword``."""
    return _check_rnn_entry(header, "lstm", True)


def check_crnn_entry(header: dict):
    """The header's ``crnn`` entry as (num_layers, num_directions), within the limits of the int8 GRU stack."""
    return _check_rnn_entry(header, "crnn", False)


def _check_rnn_stack(arrays, gates, K0, L, nd):
    """L layers of nd directions of ``gates`` gate blocks (LSTM 4, GRU 3) over K0 input columns, then the two gate tables."""
    G, H = gates * LSTM_HIDDEN, LSTM_HIDDEN
    for layer in range(L):
        for d in LSTM_DIRS[:nd]:
            for part, K in (("ih", K0 if layer == 0 else nd * H), ("hh", H)):
                p = f"l{layer}.{d}.{part}"
                w = _need(arrays, p + ".w", np.int8, (G, K))
                if (w == -128).any():
                    raise BundleError(f"{p}.w holds -128: weights are symmetric, in [-127, 127]")
                _need(arrays, p + ".b", np.int32, (G,))
                _check_mult(arrays, p, G)
    _check_tables(arrays)


def _check_lstm(header, arrays, fs):
    I, L, nd = check_lstm_entry(header)
    nc = header["num_classes"]
    if not (isinstance(nc, int) and 2 <= nc <= 64):
        raise BundleError(f"num_classes {nc!r} is outside [2, 64]")
    if fs[0] != I:
        raise BundleError(f"feature_shape {fs!r} does not have the LSTM's {I} features per frame")
    _check_rnn_stack(arrays, 4, I, L, nd)
    _check_fc(arrays, nc, nd * LSTM_HIDDEN)


def _check_tables(arrays):
    for name, lo in (("tab.sigmoid", 0), ("tab.tanh", -32767)):
        t = _need(arrays, name, np.int16, (LSTM_TABLE,)).astype(np.int64)
        if (np.diff(t) < 0).any() or t.min() < lo or t.max() > 32767:
            raise BundleError(f"{name} is not a non-decreasing table within [{lo}, 32767]")


def _check_crnn(header, arrays):
    L, nd = check_crnn_entry(header)
    nc = header["num_classes"]
    if not (isinstance(nc, int) and 2 <= nc <= 64):
        raise BundleError(f"num_classes {nc!r} is outside [2, 64]")
    for name in CONVS:
        p = "front." + name
        w = _need(arrays, p + ".w", np.int8, (64, 64 if name.startswith("pw") else 9))
        if (w == -128).any():
            raise BundleError(f"{p}.w holds -128: weights are symmetric, in [-127, 127]")
        _need(arrays, p + ".b", np.int32, (64,))
        _check_mult(arrays, p, 64)
    _check_mult(arrays, "fmean", 1)
    _check_rnn_stack(arrays, 3, 64, L, nd)
    _check_fc(arrays, nc, nd * LSTM_HIDDEN)


def _check_mbv3_layer(arrays, p, cout, k_in, hs=False):
    w = _need(arrays, p + ".w", np.int8, (cout, k_in))
    if (w == -128).any():
        raise BundleError(f"{p}.w holds -128: weights are symmetric, in [-127, 127]")
    _need(arrays, p + ".b", np.int32, (cout,))
    _check_mult(arrays, p, cout)
    if hs:
        _need(arrays, p + ".tab", np.int8, (256,))
        for z in (".zu", ".zo"):
            if not -128 <= int(_need(arrays, p + z, np.int32, (1,))[0]) <= 127:
                raise BundleError(f"{p}{z} is outside int8")


def _check_mbv3_pool(arrays, p, hw):
    _check_mult(arrays, p, 1)
    got = int(_need(arrays, p + ".hw", np.int32, (1,))[0])
    if got != hw:
        raise BundleError(f"{p}.hw is {got}: the feature_shape reduces to {hw} pixels there")


def _check_mobilenetv3(header, arrays, fs):
    nc = header["num_classes"]
    if not (isinstance(nc, int) and not isinstance(nc, bool) and 2 <= nc <= 64):
        raise BundleError(f"num_classes {nc!r} is outside [2, 64]")
    _check_mbv3_layer(arrays, "stem", MBV3_STEM, 9, hs=True)
    blocks = mbv3_blocks(*fs)
    for i, b in enumerate(blocks):
        p = f"b{i}."
        if b["expand"]:
            _check_mbv3_layer(arrays, p + "expand", b["exp"], b["cin"], b["hs"])
        _check_mbv3_layer(arrays, p + "dw", b["exp"], b["k"] ** 2, b["hs"])
        if b["se"]:
            _check_mbv3_pool(arrays, p + "pool", b["hw"][0] * b["hw"][1])
            _check_mbv3_layer(arrays, p + "fc1", b["se"], b["exp"])
            _check_mbv3_layer(arrays, p + "fc2", b["exp"], b["se"])
            _check_mult(arrays, p + "gate", 1)
        _check_mbv3_layer(arrays, p + "project", b["cout"], b["exp"])
        if b["res"]:
            _check_mult(arrays, p + "res", 1)
    _check_mbv3_layer(arrays, "last", MBV3_LAST, blocks[-1]["cout"], hs=True)
    _check_mbv3_pool(arrays, "pool", blocks[-1]["hw"][0] * blocks[-1]["hw"][1])
    _check_mbv3_layer(arrays, "cls0", MBV3_HIDDEN, MBV3_LAST, hs=True)
    _check_fc(arrays, nc, MBV3_HIDDEN)


def check_bundle(header: dict, arrays: dict) -> None:
    """Raises ``BundleError`` unless the bundle is complete and every value is in the range its law gives it."""
    if not isinstance(header, dict) or header.get("format") != FORMAT_NAME:
        raise BundleError("not a wakeword bundle (no such format name in the header)")
    if header.get("version") != FORMAT_VERSION:
        raise BundleError(f"format version {header.get('version')!r} is unknown (this reader knows {FORMAT_VERSION})")
    kind = header.get("kind")
    for key in ("architecture", "num_classes", "input_shape", "layers"):
        if key not in header:
            raise BundleError(f"header entry {key!r} is missing")
    if len(header["input_shape"]) != 4:
        raise BundleError(f"input_shape {header['input_shape']!r} is not (1,1,F,T)")
    if kind in ("fp32", "fp16"):
        want = np.float32 if kind == "fp32" else np.float16
        names = [k for k in arrays if k.startswith(STATE_PREFIX)]
        if not names:
            raise BundleError("the bundle holds no state")
        for k in names:
            if np.issubdtype(arrays[k].dtype, np.floating) and arrays[k].dtype != want:
                raise BundleError(f"array {k!r} is {arrays[k].dtype} in a bundle of kind {kind}")
        return
    if kind != "int8":
        raise BundleError(f"unknown bundle kind {kind!r}")
    if header["architecture"] not in ("cnn_small", "crnn", "mobilenetv3", "TCNWakeword", "ResNet18Wakeword", "LSTMWakeword"):
        raise BundleError(f"an int8 bundle of {header['architecture']!r}: only cnn_small, crnn, mobilenetv3, TCNWakeword, "
                          "ResNet18Wakeword and LSTMWakeword have an int8 form")
    fs = header.get("feature_shape")
    if not (isinstance(fs, list) and len(fs) == 2 and all(isinstance(v, int) and v >= 1 for v in fs)):
        raise BundleError(f"feature_shape {fs!r} is not [F, T]")
    s = _need(arrays, "input_scale", np.float32, (1,))
    if not (np.isfinite(s[0]) and s[0] > 0):
        raise BundleError("input_scale is not positive and finite")
    z = _need(arrays, "input_zero", np.int32, (1,))
    if not -128 <= int(z[0]) <= 127:
        raise BundleError("input_zero is outside int8")
    if header["architecture"] == "TCNWakeword":
        return _check_tcn(header, arrays, fs)
    if header["architecture"] == "ResNet18Wakeword":
        return _check_resnet18(header, arrays)
    if header["architecture"] == "LSTMWakeword":
        return _check_lstm(header, arrays, fs)
    if header["architecture"] == "crnn":
        return _check_crnn(header, arrays)
    if header["architecture"] == "mobilenetv3":
        return _check_mobilenetv3(header, arrays, fs)
    for name in CONVS:
        w = _need(arrays, name + ".w", np.int8, (64, 64 if name.startswith("pw") else 9))
        if (w == -128).any():
            raise BundleError(f"{name}.w holds -128: weights are symmetric, in [-127, 127]")
        _need(arrays, name + ".b", np.int32, (64,))
        _check_mult(arrays, name, 64)
    _check_mult(arrays, "pool", 1)
    _need(arrays, "fc.w", np.int8, (2, 64))
    _need(arrays, "fc.b", np.int32, (2,))
    if not np.isfinite(_need(arrays, "fc.scale", np.float32, (2,))).all():
        raise BundleError("fc.scale is not finite")
