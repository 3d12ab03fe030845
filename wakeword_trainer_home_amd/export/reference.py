"""A pure-NumPy interpreter of an int8 bundle: the int8 law of DESIGN.md "Export", and nothing else.

It imports NumPy and the standard library only -- no torch, no native library, nothing of this package -- so a port of the
bundle to another runtime can be checked against it, tensor by tensor.  It runs on the CPU.

    header, arrays = load_bundle("model_int8.npz")
    out = run_int8(header, arrays, features)          # features (B,1,F,T) or (B,F,T) float32
    out["logits"]                                     # (B,2) float32; the other keys are the int8 tensors of every stage
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


def run_int8(header, arrays, x):
    """Every stage of the int8 network on features ``x``; -> dict of STAGES (int8 NHWC tensors, ``pool`` (B,64), ``logits``)."""
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
    S = _wrap32((q.astype(np.int64) + 128).sum(axis=(1, 2)))
    p = requantize(S, a["pool.m"][0], a["pool.sh"][0])
    out["pool"] = p
    acc = _wrap32((p.astype(np.int64) + 128) @ a["fc.w"].astype(np.int64).T + a["fc.b"].astype(np.int64))
    out["logits"] = acc.astype(np.float32) * a["fc.scale"].astype(np.float32)
    return out
