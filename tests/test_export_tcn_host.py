"""The TCN half of the export package without a GPU: the NumPy interpreter and ``quantize_tcn`` against the restated law
(tests/q8_tcn_cases.py) bit for bit, the refusals, the bundle file, the ABI names, and the quantisation error against the
float64 model on the committed fixture."""
import json
import re
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from tests import q8_tcn_cases as TQ
from wakeword_trainer_home_amd.export import bundle as BU
from wakeword_trainer_home_amd.export import quantize as QZ
from wakeword_trainer_home_amd.export import reference as R

REPO = Path(__file__).resolve().parent.parent
GOLDEN = Path(__file__).resolve().parent / "golden"
TQ8_NAMES = ["ww_tq8_conv1d_fwd", "ww_tq8_pool_fc_fwd", "ww_tq8_quantize_bt", "ww_tq8_skip_add_fwd", "ww_tq8_tcn_fwd",
             "ww_tq8_tcn_workspace_bytes"]


@pytest.fixture(scope="module")
def hard_cases():
    """name -> (header, arrays, x, restated stages with accumulators); ``assert_hard`` has run on each."""
    return {name: TQ.hard_case(name) for name in TQ.SHAPES}


# ------------------------------------------------------------------ the interpreter against the restatement
@pytest.mark.parametrize("name", list(TQ.SHAPES))
def test_interpreter_equals_restated_law_on_every_tensor(hard_cases, name):
    header, arrays, x, ref = hard_cases[name]
    out = R.run_int8(header, arrays, x, want_acc=True)
    want = TQ.stages(header["tcn"])
    assert [k for k in out if not k.startswith("acc/")] == want == R.tcn_stages(header["tcn"])
    for stage in want + [k for k in out if k.startswith("acc/")]:
        assert out[stage].dtype == ref[stage].dtype and out[stage].shape == ref[stage].shape, stage
        assert np.array_equal(out[stage], ref[stage]), stage
    assert list(R.run_int8(header, arrays, x)) == want                      # the accumulators come on request only
    B, F, T = x.shape[0], x.shape[2], x.shape[3]
    assert out["xq"].shape == (B, T, F) and out["logits"].shape == (B, 2) and out["logits"].dtype == np.float32
    with pytest.raises(ValueError, match="features of shape"):
        R.run_int8(header, arrays, np.zeros((1, 1, F, T + 1), np.float32))


def test_interpreter_three_classes():
    header, arrays, x, ref = TQ.hard_case("small", num_classes=3)
    out = R.run_int8(header, arrays, x)
    assert out["logits"].shape == (5, 3) and np.array_equal(out["logits"], ref["logits"])


# ------------------------------------------------------------------ the derivation against the restatement
@pytest.mark.parametrize("name,dead", [("identity", None), ("default", None), ("small", None), ("small", (1, "conv1"))])
def test_export_derivation_equals_restated_law(name, dead):
    _, F, T, ch, k = TQ.SHAPES[name]
    args = TQ.tcn_args(F, ch, k)
    state = TQ.random_state(args, 3, seed=4, dead=dead)
    x = TQ.structured_features(6, F, T, seed=4)
    _, ranges = TQ.float_forward(state, args, x[:3])
    arrays, scales = QZ.quantize_tcn(state, args, (F, T), ranges["x_min"], ranges["x_max"], ranges["a_max"], ranges["p_max"])
    want = TQ.r_quantize_model(state, args, (F, T), ranges)
    assert sorted(arrays) == sorted(want)
    for key in want:
        assert arrays[key].dtype == want[key].dtype and np.array_equal(arrays[key], want[key]), key
    assert arrays["b0.conv1.w"].shape == (ch[0], F, k)                          # unpadded
    assert not arrays["b0.conv2.w"][TQ.ZERO_CH].any()                           # the all-zero channel of random_state
    assert ("b1.skip.m" in arrays) == (ch[0] == ch[1]) and ("b1.down.w" in arrays) == (ch[0] != ch[1])
    header = TQ.header_for(F, T, args, 3)
    BU.check_bundle(header, arrays)
    out, ref = R.run_int8(header, arrays, x), TQ.r_forward(args, arrays, x)
    for stage in TQ.stages(args):
        assert np.array_equal(out[stage], ref[stage]), stage
    if dead:                                                                    # the dead-layer floor
        assert ranges["a_max"][3 * dead[0]] == 0.0 and scales["b1.h1"] == 2.0 ** -20 and (out["b1.h1"] == -128).all()


def test_export_refuses_what_the_law_cannot_hold():
    _, F, T, ch, k = TQ.SHAPES["small"]
    args = TQ.tcn_args(F, ch, k)
    state = TQ.random_state(args, 2, seed=4)
    _, r = TQ.float_forward(state, args, TQ.structured_features(2, F, T))
    quantize = lambda st, rr: QZ.quantize_tcn(st, args, (F, T), rr["x_min"], rr["x_max"], rr["a_max"], rr["p_max"])  # noqa: E731
    quantize(state, r)
    bad = dict(state)
    bad["tcn.network.1.conv2.bias"] = state["tcn.network.1.conv2.bias"].copy()
    bad["tcn.network.1.conv2.bias"][11] = 1e12                                    # a bias overflow
    with pytest.raises(QZ.QuantizationError, match=r"b1\.conv2, channel 11"):
        quantize(bad, r)
    bad = dict(state)
    bad["tcn.network.0.downsample.bias"] = state["tcn.network.0.downsample.bias"].copy()
    bad["tcn.network.0.downsample.bias"][3] = -1e12
    with pytest.raises(QZ.QuantizationError, match=r"b0\.down, channel 3"):
        quantize(bad, r)
    # the bound is k * Cin * 127 * 255 for a conv, C_last * 127 * 255 for the classifier
    s_w = np.ones(48)
    assert QZ.quantize_bias(np.full(48, float(2 ** 31 - 1 - 2 * 32 * 127 * 255)), 1.0, s_w, 2 * 32 * 127 * 255, "b1.conv1")[0] > 0
    with pytest.raises(QZ.QuantizationError, match="b1.conv1, channel 0"):
        QZ.quantize_bias(np.full(48, float(2 ** 31 - 2 * 32 * 127 * 255)), 1.0, s_w, 2 * 32 * 127 * 255, "b1.conv1")
    for value in (float("nan"), float("inf")):                                    # a non-finite maximum
        rr = dict(r, a_max=list(r["a_max"]))
        rr["a_max"][4] = value
        with pytest.raises(QZ.QuantizationError, match="not finite"):
            quantize(state, rr)
    bad = dict(state)                                                             # a multiplier that rounds to zero
    bad["tcn.network.0.conv1.weight"] = state["tcn.network.0.conv1.weight"].copy()
    bad["tcn.network.0.conv1.weight"][2] *= 1e-30
    with pytest.raises(QZ.QuantizationError, match=r"b0\.conv1, channel 2"):
        quantize(bad, r)
    with pytest.raises(QZ.QuantizationError, match="b0.add"):
        QZ.encode_multiplier(0.0, "b0.add")
    for broken in (dict(args, kernel_size=9), dict(args, num_channels=[32, 50]), dict(args, num_channels=[8] * 9)):
        with pytest.raises(QZ.QuantizationError):
            QZ.quantize_tcn(state, broken, (F, T), r["x_min"], r["x_max"], r["a_max"], r["p_max"])
    with pytest.raises(QZ.QuantizationError):
        QZ.check_tcn_args(args, num_classes=65)


# ------------------------------------------------------------------ the bundle file
def test_bundle_round_trip_and_plain_readability(tmp_path, hard_cases):
    header, arrays, x, ref = hard_cases["identity"]
    path = BU.write_bundle(tmp_path / "t_int8.npz", header, arrays)
    h2, a2 = BU.load_bundle(path)
    assert h2 == header and sorted(a2) == sorted(arrays)
    for k in arrays:
        assert a2[k].dtype == arrays[k].dtype and np.array_equal(a2[k], arrays[k]), k
    code = ("import sys, json, numpy as np\n"
            "z = np.load(sys.argv[1], allow_pickle=False)\n"
            "h = json.loads(bytes(z['header']).decode('utf-8'))\n"
            "assert not any(m.startswith(('torch', 'wakeword')) for m in sys.modules)\n"
            "print(json.dumps([h['kind'], h['architecture'], h['tcn'], sorted(z.files), int(z['b1.conv2.m'][5])]))\n")
    r = subprocess.run([sys.executable, "-c", code, str(path)], capture_output=True, text=True, cwd=tmp_path)
    assert r.returncode == 0, r.stderr
    kind, arch, tcn, files, m = json.loads(r.stdout)
    assert (kind, arch, m) == ("int8", "TCNWakeword", 2 ** 30) and files == sorted(list(arrays) + ["header"])
    assert tcn == {"input_size": 12, "num_channels": [16, 16, 16], "kernel_size": 3}


def _malformed():
    def drop(a, h):
        del a["b1.conv2.sh"]

    def drop_skip(a, h):
        del a["b0.skip.m"]

    def drop_add(a, h):
        del a["b1.add.sh"]

    def shape(a, h):
        a["b0.conv1.w"] = a["b0.conv1.w"].transpose(0, 2, 1).copy()

    def padded(a, h):
        a["b2.down.w"] = np.zeros((64, 64, 1), np.int8)          # arrays are unpadded: (48, 32, 1)

    def dtype(a, h):
        a["b1.conv1.b"] = a["b1.conv1.b"].astype(np.int64)

    def mult_low(a, h):
        a["b1.add.m"][0] = 2 ** 30 - 1

    def mult_negative(a, h):
        a["b0.conv2.m"][0] = -(2 ** 30)

    def shift_zero(a, h):
        a["b0.skip.sh"][0] = 0

    def shift_high(a, h):
        a["pool.sh"][0] = 63

    def weight_min(a, h):
        a["b1.conv1.w"][1, 1, 0] = -128

    def no_tcn(a, h):
        del h["tcn"]

    def tcn_channels(a, h):
        h["tcn"] = dict(h["tcn"], num_channels=[32, 50])

    def tcn_kernel(a, h):
        h["tcn"] = dict(h["tcn"], kernel_size=9)

    def feature_rows(a, h):
        h["feature_shape"] = [36, h["feature_shape"][1]]

    def classes(a, h):
        h["num_classes"] = 3

    def arch(a, h):
        h["architecture"] = "gru"

    def scale(a, h):
        a["fc.scale"][1] = np.inf
    return [drop, drop_skip, drop_add, shape, padded, dtype, mult_low, mult_negative, shift_zero, shift_high, weight_min, no_tcn,
            tcn_channels, tcn_kernel, feature_rows, classes, arch, scale]


def test_malformed_bundles_are_invalid_not_errors(tmp_path):
    from wakeword_trainer_home_amd.export import validate_exported_model
    # channels [32, 32, 48]: block 0 has an identity skip (F = 32), block 2 a downsample conv
    header, arrays = TQ.hard_bundle(32, 9, [32, 32, 48], 2)
    BU.check_bundle(header, arrays)
    good = validate_exported_model(BU.write_bundle(tmp_path / "good.npz", header, arrays))
    assert good["valid"] is True and good["error"] is None and good["graph"] == len(header["layers"]) == 9
    assert good["inputs"] == [("input", [0, 1, 32, 9])] and good["outputs"] == [("output", [0, 2])]
    for breaker in _malformed():
        a, h = {k: v.copy() for k, v in arrays.items()}, dict(header)
        breaker(a, h)
        with pytest.raises(BU.BundleError):
            BU.check_bundle(h, a)
        res = validate_exported_model(BU.write_bundle(tmp_path / f"{breaker.__name__}.npz", h, a))
        assert res["valid"] is False and res["error"], breaker.__name__


def test_float_bundles_of_a_tcn_carry_the_tcn_entry():
    args = TQ.tcn_args(40, [32, 48], 2)
    state = TQ.random_state(args, 2, seed=1)
    for kind in ("fp32", "fp16"):
        h = BU.make_header(kind, "TCNWakeword", 2, (1, 1, 40, 70), list(state), tcn=args)
        BU.check_bundle(h, BU.float_arrays(state, fp16=kind == "fp16"))
        assert BU.check_tcn_entry(h) == (40, [32, 48], 2)
    with pytest.raises(BU.BundleError):
        BU.check_tcn_entry({"tcn": {"input_size": 40, "num_channels": [], "kernel_size": 2}})


# ------------------------------------------------------------------ interface
def test_header_and_exports_agree_on_the_tq8_entry_points():
    import ctypes
    from wakeword_trainer_home_amd import _native
    header = (REPO / "include" / "wwhip.h").read_text()
    declared = set(re.findall(r"\b(ww_[a-z0-9_]+)\s*\(", header))
    assert declared == set(_native.EXPORTS)
    assert sorted(n for n in declared if n.startswith("ww_tq8_")) == TQ8_NAMES
    assert _native.ABI_VERSION == 17 and _native.load().ww_abi_version() == 17
    assert (_native.TQ8_MAX_BLOCKS, _native.TQ8_BLOCK_NPTR) == (8, 12)
    assert re.search(r"#define\s+WW_TQ8_MAX_BLOCKS\s+8\b", header) and re.search(r"#define\s+WW_TQ8_BLOCK_NPTR\s+12\b", header)
    assert ctypes.sizeof(_native.Tq8Io) == 4 * (8 + 5 * 8)
    makefile = (REPO / "wakeword_trainer_home_amd" / "csrc" / "Makefile").read_text()
    assert "ww_q8_tcn.hip" in makefile
    # the workspace the header describes: xq, then h1, h2, out per block, then pool, each rounded up to 256 bytes
    r256 = lambda n: (n + 255) // 256 * 256       # noqa: E731
    p64 = lambda c: (c + 63) // 64 * 64           # noqa: E731
    for B, F, T, ch, _ in list(TQ.SHAPES.values()) + [(512, 40, 151, [64, 128, 256], 3)]:
        want = r256(B * T * p64(F)) + sum(3 * r256(B * T * p64(c)) for c in ch) + r256(B * ch[-1])
        assert _native.tq8_tcn_workspace_bytes(B, F, T, ch) == want
    assert _native.tq8_tcn_workspace_bytes(0, 40, 45, [64]) == 0 and _native.tq8_tcn_workspace_bytes(1, 40, 45, [4] * 9) == 0


def test_quantized_tcn_refuses_cpu_input_and_other_shapes(hard_cases):
    import torch
    import wakeword_trainer_home_amd.export as E
    from wakeword_trainer_home_amd._native import NativeError
    assert "QuantizedTCN" in E.__all__ and "calibrate_tcn" in E.__all__
    header, arrays, x, _ = hard_cases["identity"]
    model = E.QuantizedTCN(header, arrays)
    assert model.hip_backed and not model.training and not list(model.parameters())
    assert not any(t.requires_grad for t in model.buffers()) and model.num_classes == 2
    assert model.conv(0, "conv1")[0].shape == (64, 3, 64) and model.conv(1, "down") == (None,) * 4
    with pytest.raises(NativeError, match="no CPU fallback"):
        model(torch.from_numpy(x))
    with pytest.raises(ValueError, match="features of shape"):
        model(torch.zeros(1, 1, 12, 6))
    with pytest.raises(RuntimeError):
        model.train()
    with pytest.raises(ValueError):
        E.QuantizedTCN(dict(header, kind="fp32"), arrays)
    from tests import q8_cases as Q
    with pytest.raises(ValueError):
        E.QuantizedTCN(*Q.hard_bundle(13, 21))


def test_device_layout_pads_with_zero_weights_and_neutral_channels(hard_cases):
    from wakeword_trainer_home_amd.export.runtime import device_tcn_conv
    header, arrays, _, _ = hard_cases["small"]
    w, b, m, sh = device_tcn_conv(arrays, "b1.conv1", -128)
    q = arrays["b1.conv1.w"]
    assert w.shape == (64, 2, 64) and np.array_equal(w[:48, :, :32], q.transpose(0, 2, 1))
    assert not w[48:].any() and not w[:, :, 32:].any()
    assert np.array_equal(b[:48], (arrays["b1.conv1.b"].astype(np.int64) + 128 * q.astype(np.int64).sum(axis=(1, 2))).astype(np.int32))
    assert not b[48:].any() and (m[48:] == 2 ** 30).all() and (sh[48:] == 31).all()


# ------------------------------------------------------------------ quantisation error against the float64 model
def test_quantisation_error_on_the_golden_fixture():
    """Interpreter on the exported bundle of the fixture vs. the float64 model, over its 24 structured feature maps.
    Recorded for the restated law (tests/golden/q8_tcn_errors.json): max |dlogit| 0.258, mean 0.119, with logit margins from
    -36.76 to -13.99 across the samples.  The interpreter is held to twice the record; the factor covers a re-seeded fixture."""
    z = np.load(GOLDEN / "g14_q8_tcn.npz")
    rec = json.loads((GOLDEN / "q8_tcn_errors.json").read_text())["TCNWakeword"]
    x = z["x"].astype(np.float32)
    F, T = rec["feature_shape"]
    assert x.shape == (24, 1, F, T) and rec["samples"] == 24 and rec["calibration_samples"] == 12
    args = TQ.tcn_args(F, z["num_channels"].tolist(), int(z["kernel_size"]))
    state = TQ.random_state(args, 2, seed=int(z["param_seed"]), gain=float(z["gain"]))
    for k, v in state.items():                                                    # the regenerated parameters are the fixture's
        idx = np.arange(v.size) if v.size <= 16 else np.linspace(0, v.size - 1, 16).astype(np.int64)
        assert np.array_equal(v.reshape(-1)[idx], z["psamp." + k]), k
    logits, _ = TQ.float_forward(state, args, x)
    assert np.array_equal(logits, z["logits"])
    _, cal = TQ.float_forward(state, args, x[:12])
    assert cal["x_min"] == float(z["x_min"]) and cal["a_max"] == z["a_max"].tolist() and cal["p_max"] == float(z["p_max"])
    arrays, _ = QZ.quantize_tcn(state, args, (F, T), float(z["x_min"]), float(z["x_max"]), z["a_max"].tolist(), float(z["p_max"]))
    q = R.run_int8(TQ.header_for(F, T, args), arrays, x)["logits"]
    d = np.abs(q.astype(np.float64) - logits)
    margin = logits[:, 1] - logits[:, 0]
    print(f"MEASURED max |dlogit| {d.max():.4g} (recorded {rec['max_abs_dlogit']}), mean {d.mean():.4g}; "
          f"margin {margin.min():.4g} .. {margin.max():.4g}")
    assert margin.max() - margin.min() > 20 * rec["max_abs_dlogit"], "the margins vary too little to show a quantisation error"
    assert d.max() <= 2 * rec["max_abs_dlogit"]
