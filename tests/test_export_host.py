"""The export package without a GPU: the int8 law's encodings and refusals, the NumPy interpreter against the restated law
(tests/q8_cases.py) bit for bit, the bundle file, and the quantisation error against the float64 model."""
import ctypes
import dataclasses
import json
import re
import subprocess
import sys
from fractions import Fraction
from pathlib import Path

import numpy as np
import pytest

from tests import q8_cases as Q
from wakeword_trainer_home_amd.export import bundle as BU
from wakeword_trainer_home_amd.export import quantize as QZ
from wakeword_trainer_home_amd.export import reference as R

REPO = Path(__file__).resolve().parent.parent
GOLDEN = Path(__file__).resolve().parent / "golden"


# ------------------------------------------------------------------ multiplier encoding
@pytest.mark.parametrize("r", [0.5, 0.75, 1.0, 2.0 ** -31, 2.0 ** 29, (2 ** 31 - 1) * 2.0 ** -1, 1.0 - 2.0 ** -33, 1.0 - 2.0 ** -32,
                               0.3, 1e-7, 123.456, 2.0 ** -31 * (1 + 2.0 ** -31), np.nextafter(2.0 ** 30, 0.0) / 2,
                               (2 ** 30 + 0.5) * 2.0 ** -40, (2 ** 30 + 1.5) * 2.0 ** -40])
def test_multiplier_encoding_is_the_nearest(r):
    m, sh = QZ.encode_multiplier(r)
    assert 2 ** 30 <= m < 2 ** 31 and 1 <= sh <= 62
    assert (m, sh) == Q.r_encode_multiplier(r)
    # no neighbour in the same binade is nearer
    err = abs(Fraction(m, 2 ** sh) - Fraction(r))
    assert err <= abs(Fraction(m + 1, 2 ** sh) - Fraction(r)) and err <= abs(Fraction(m - 1, 2 ** sh) - Fraction(r))


def test_multiplier_range_ends_and_refusals():
    assert QZ.encode_multiplier(0.5) == (2 ** 30, 31)
    assert QZ.encode_multiplier(2.0 ** -32) == (2 ** 30, 62)                  # the smallest shift-62 multiplier
    assert QZ.encode_multiplier(2.0 ** 29) == (2 ** 30, 1)
    assert QZ.encode_multiplier((2 ** 31 - 1) * 0.5) == (2 ** 31 - 1, 1)      # the largest value there is
    assert QZ.encode_multiplier(1.0 - 2.0 ** -33) == (2 ** 30, 30)            # rounds up into the next binade
    for bad in (0.0, -1.0, float("nan"), float("inf"), 2.0 ** 30, 2.0 ** -33, 1e-30):
        with pytest.raises(QZ.QuantizationError):
            QZ.encode_multiplier(bad, "layer x, channel 3")
        assert Q.r_encode_multiplier(bad) is None or bad == 2.0 ** -33
    with pytest.raises(QZ.QuantizationError, match="layer x, channel 3"):
        QZ.encode_multiplier(0.0, "layer x, channel 3")


def test_bias_refusal_names_layer_and_channel():
    s_w = np.ones(64)
    ok = QZ.quantize_bias(np.full(64, float(2 ** 31 - 1 - QZ.ACC_MAX_3X3)), 1.0, s_w, QZ.ACC_MAX_3X3, "dw1")
    assert ok.dtype == np.int32 and ok[0] == 2 ** 31 - 1 - QZ.ACC_MAX_3X3
    b = np.zeros(64)
    b[9] = -float(2 ** 31 - QZ.ACC_MAX_1X1)
    with pytest.raises(QZ.QuantizationError, match=r"pw2, channel 9"):
        QZ.quantize_bias(b, 1.0, s_w, QZ.ACC_MAX_1X1, "pw2")
    assert QZ.ACC_MAX_3X3 == 9 * 127 * 255 and QZ.ACC_MAX_1X1 == 64 * 127 * 255


def test_weight_quantisation_and_all_zero_channel():
    g = np.random.default_rng(0)
    w = g.normal(0, 1, (64, 9))
    w[7] = 0
    q, s = QZ.quantize_weights(w)
    assert q.dtype == np.int8 and s[7] == 1.0 and not q[7].any()
    assert np.abs(q).max(axis=1)[np.arange(64) != 7].min() == 127 and q.min() >= -127
    assert np.array_equal(q, np.clip(np.rint(w / s[:, None]), -127, 127))


def test_dead_layer_floor():
    assert QZ.out_scale(0.0) == QZ.out_scale(-3.0) == 2.0 ** -20 == QZ.A_MAX_FLOOR / 255.0 == Q.A_MAX_FLOOR / 255.0
    assert QZ.out_scale(51.0) == 0.2
    with pytest.raises(QZ.QuantizationError):
        QZ.out_scale(float("nan"))


# ------------------------------------------------------------------ input quantisation
def test_input_quantisation_special_values():
    s, z = QZ.input_qparams(-12.75, 3.1875)
    assert s.dtype == np.float32 and s == np.float32(0.0625) and z == 76
    x = np.array([np.nan, np.inf, -np.inf, 0.0, -12.75, 3.1875, 1e30, -1e30, 0.03125, 0.09375, -0.03125, 3.4e38, 1e-45],
                 np.float32)
    want = np.array([76, 127, -128, 76, -128, 127, 127, -128, 76, 78, 76, 127, 76], np.int8)      # ties go to the even
    assert np.array_equal(R.quantize_input(x, s, z), want)
    assert np.array_equal(Q.r_quantize_input(x, s, z), want)
    g = np.random.default_rng(3)
    x = (g.normal(0, 6, 20000) * g.choice([1.0, 1e-3, 40.0], 20000)).astype(np.float32)
    for scale, zero in ((s, z), (np.float32(0.1), -128), (np.float32(1.7e-3), 127), (np.float32(3.3), 0)):
        assert np.array_equal(R.quantize_input(x, scale, zero), Q.r_quantize_input(x, scale, zero))


def test_input_range_contains_zero():
    s, z = QZ.input_qparams(2.0, 10.0)                # widened to [0, 10]
    assert z == -128 and s == np.float32(10.0 / 255.0)
    s, z = QZ.input_qparams(-5.0, -1.0)               # widened to [-5, 0]
    assert z == 127
    s, z = QZ.input_qparams(0.0, 0.0)
    assert s == np.float32(1.0 / 255.0) and z == -128
    with pytest.raises(QZ.QuantizationError):
        QZ.input_qparams(float("-inf"), 1.0)


# ------------------------------------------------------------------ the interpreter against the restatement
@pytest.fixture(scope="module")
def hard_cases():
    out = {}
    for B, F, T in ((3, 13, 21), (2, 40, 38)):
        header, arrays = Q.hard_bundle(F, T)
        x = Q.hard_features(F, T, B)
        ref = Q.r_forward(arrays, x, want_acc=True)
        Q.assert_hard(arrays, ref)
        out[(B, F, T)] = (header, arrays, x, ref)
    return out


@pytest.mark.parametrize("shape", [(3, 13, 21), (2, 40, 38)])
def test_interpreter_equals_restated_law_on_every_tensor(hard_cases, shape):
    header, arrays, x, ref = hard_cases[shape]
    out = R.run_int8(header, arrays, x)
    assert list(out) == Q.STAGES == R.STAGES
    for stage in Q.STAGES:
        assert out[stage].dtype == ref[stage].dtype and out[stage].shape == ref[stage].shape, stage
        assert np.array_equal(out[stage], ref[stage]), stage
    with pytest.raises(ValueError, match="features of shape"):
        R.run_int8(header, arrays, np.zeros((1, 1, shape[1] + 1, shape[2]), np.float32))


@pytest.mark.parametrize("dead", [None, "dw2"])
def test_export_derivation_equals_restated_law(dead):
    state = Q.random_state(seed=4, dead=dead)
    x = Q.structured_features(6, 13, 21, seed=4)
    _, ranges = Q.float_forward(state, x[:3])
    if dead:
        assert ranges["a_max"][Q.CONVS.index(dead)] == 0.0
    arrays, scales = QZ.quantize_cnn_small(state, (13, 21), ranges["x_min"], ranges["x_max"], ranges["a_max"], ranges["p_max"])
    want = Q.r_quantize_model(state, (13, 21), ranges)
    assert sorted(arrays) == sorted(want)
    for k in want:
        assert arrays[k].dtype == want[k].dtype and np.array_equal(arrays[k], want[k]), k
    assert not arrays["dw1.w"][Q.ZERO_CH].any()                                   # the all-zero channel of random_state
    header = Q.header_for(13, 21)
    BU.check_bundle(header, arrays)
    out, ref = R.run_int8(header, arrays, x), Q.r_forward(arrays, x)
    for stage in Q.STAGES:
        assert np.array_equal(out[stage], ref[stage]), stage
    if dead:
        assert scales[dead] == 2.0 ** -20 and (out[dead] == -128).all()


def test_export_refuses_what_the_law_cannot_hold():
    state = Q.random_state(seed=4)
    _, r = Q.float_forward(state, Q.structured_features(2, 13, 21))
    state["blocks.3.pw_bn.bias"][11] = 1e12
    with pytest.raises(QZ.QuantizationError, match="pw3, channel 11"):
        QZ.quantize_cnn_small(state, (13, 21), r["x_min"], r["x_max"], r["a_max"], r["p_max"])
    state = Q.random_state(seed=4)
    state["blocks.0.dw.weight"][2] *= 1e12                                   # a multiplier of 2^30 or more
    with pytest.raises(QZ.QuantizationError, match="dw0, channel 2"):
        QZ.quantize_cnn_small(state, (13, 21), r["x_min"], r["x_max"], r["a_max"], r["p_max"])


# ------------------------------------------------------------------ the bundle file
def test_bundle_round_trip_and_plain_readability(tmp_path, hard_cases):
    header, arrays, x, ref = hard_cases[(3, 13, 21)]
    path = BU.write_bundle(tmp_path / "m_int8.npz", header, arrays)
    assert path.name == "m_int8.npz"
    h2, a2 = BU.load_bundle(path)
    assert h2 == header and sorted(a2) == sorted(arrays)
    for k in arrays:
        assert a2[k].dtype == arrays[k].dtype and np.array_equal(a2[k], arrays[k]), k
    # a reader with NumPy and json alone, in a process that never imports the package
    code = ("import sys, json, numpy as np\n"
            "z = np.load(sys.argv[1], allow_pickle=False)\n"
            "h = json.loads(bytes(z['header']).decode('utf-8'))\n"
            "assert not any(m.startswith(('torch', 'wakeword')) for m in sys.modules)\n"
            "print(json.dumps([h['kind'], h['version'], h['feature_shape'], sorted(z.files), int(z['pw3.m'][5])]))\n")
    r = subprocess.run([sys.executable, "-c", code, str(path)], capture_output=True, text=True, cwd=tmp_path)
    assert r.returncode == 0, r.stderr
    kind, version, fs, files, m = json.loads(r.stdout)
    assert (kind, version, fs, m) == ("int8", 1, [13, 21], 2 ** 30) and files == sorted(list(arrays) + ["header"])


def test_float_bundles_and_fp16_rounding(tmp_path):
    state = Q.random_state(seed=2)
    state["stem.bn.num_batches_tracked"] = np.array(7, np.int64)
    state["classifier.bias"] = np.array([1e6, -(1.0 + 2.0 ** -11)], np.float32)          # saturates; a tie: rounds to even
    h = BU.make_header("fp16", "cnn_small", 2, (1, 1, 40, 151), ["stem.conv.weight"])
    path = BU.write_bundle(tmp_path / "m_fp16.npz", h, BU.float_arrays(state, fp16=True))
    h2, a2 = BU.load_bundle(path)
    BU.check_bundle(h2, a2)
    assert a2["state/stem.bn.num_batches_tracked"].dtype == np.int64 and a2["state/stem.conv.weight"].dtype == np.float16
    assert a2["state/classifier.bias"].tolist() == [65504.0, -1.0]
    assert np.array_equal(a2["state/stem.conv.weight"], state["stem.conv.weight"].astype(np.float16))
    assert path.stat().st_size < 0.75 * BU.write_bundle(tmp_path / "m.npz", dict(h, kind="fp32"),
                                                        BU.float_arrays(state, fp16=False)).stat().st_size


def _malformed(arrays, header):
    def drop(a, h):
        del a["pw1.sh"]

    def shape(a, h):
        a["dw0.w"] = a["dw0.w"].T.copy()

    def dtype(a, h):
        a["stem.b"] = a["stem.b"].astype(np.int64)

    def version(a, h):
        h["version"] = 99

    def mult_low(a, h):
        a["pw2.m"][3] = 2 ** 30 - 1

    def mult_negative(a, h):
        a["dw3.m"][0] = -(2 ** 30)

    def shift_zero(a, h):
        a["stem.sh"][63] = 0

    def shift_high(a, h):
        a["pool.sh"][0] = 63

    def weight_min(a, h):
        a["pw0.w"][1, 1] = -128

    def kind(a, h):
        h["kind"] = "int4"

    def arch(a, h):
        h["architecture"] = "gru"

    def scale(a, h):
        a["input_scale"][0] = 0.0
    return [drop, shape, dtype, version, mult_low, mult_negative, shift_zero, shift_high, weight_min, kind, arch, scale]


def test_malformed_bundles_are_invalid_not_errors(tmp_path, hard_cases):
    from wakeword_trainer_home_amd.export import validate_exported_model
    header, arrays, _, _ = hard_cases[(3, 13, 21)]
    good = validate_exported_model(BU.write_bundle(tmp_path / "good.npz", header, arrays))
    assert good["valid"] is True and good["error"] is None and good["graph"] == len(header["layers"]) == 11
    assert good["inputs"] == [("input", [0, 1, 13, 21])] and good["outputs"] == [("output", [0, 2])] and good["file_size_mb"] > 0
    for breaker in _malformed(arrays, header):
        a, h = {k: v.copy() for k, v in arrays.items()}, dict(header)
        breaker(a, h)
        with pytest.raises(BU.BundleError):
            BU.check_bundle(h, a)
        res = validate_exported_model(BU.write_bundle(tmp_path / f"{breaker.__name__}.npz", h, a))
        assert res["valid"] is False and res["error"], breaker.__name__
    (tmp_path / "junk.npz").write_bytes(b"not a zip file")
    res = validate_exported_model(tmp_path / "junk.npz")
    assert res["valid"] is False and res["error"]
    assert validate_exported_model(tmp_path / "absent.npz")["valid"] is False


# ------------------------------------------------------------------ interface
def test_export_config_defaults_equal_the_reference():
    from wakeword_trainer_home_amd.export import ExportConfig
    got = [(f.name, f.default) for f in dataclasses.fields(ExportConfig)]
    assert got == [("output_path", dataclasses.MISSING), ("opset_version", 14), ("dynamic_batch", True), ("quantize_fp16", False),
                   ("quantize_int8", False), ("optimize", True), ("verbose", False)]


def test_aliases_and_public_names():
    import wakeword_trainer_home_amd.export as E
    assert E.ONNXExporter is E.ModelExporter and E.export_model_to_onnx is E.export_model
    assert E.validate_onnx_model is E.validate_exported_model and E.benchmark_onnx_model is E.benchmark_exported_model
    for name in ("ONNXExporter", "ExportConfig", "export_model_to_onnx", "validate_onnx_model", "benchmark_onnx_model"):
        assert name in E.__all__                          # the reference's __all__


def test_header_and_exports_agree_on_the_q8_entry_points():
    from wakeword_trainer_home_amd import _native
    header = (REPO / "include" / "wwhip.h").read_text()
    declared = set(re.findall(r"\b(ww_[a-z0-9_]+)\s*\(", header))
    assert declared == set(_native.EXPORTS)
    q8 = sorted(n for n in declared if n.startswith("ww_q8_"))
    assert q8 == ["ww_q8_cnn_small_fwd", "ww_q8_cnn_small_workspace_bytes", "ww_q8_dwconv3x3_fwd", "ww_q8_dwpw_fwd",
                  "ww_q8_gap_fc_fwd", "ww_q8_pwconv1x1_fwd", "ww_q8_quantize", "ww_q8_stem_fwd"]
    assert _native.ABI_VERSION == 17 and _native.load().ww_abi_version() == 17
    assert re.search(r"#define\s+WW_ABI_VERSION\s+17\b", header)
    assert ctypes.sizeof(_native.Q8Io) == 16 and _native.Q8_NPTR == 39 and _native.Q8_NACT == 9
    # the workspace the header describes
    r256 = lambda n: (n + 255) // 256 * 256       # noqa: E731
    for B, F, T in ((5, 40, 151), (3, 13, 21)):
        H, W = (F + 1) // 2, (T + 1) // 2
        assert _native.q8_cnn_small_workspace_bytes(B, F, T) == r256(B * F * T) + 9 * r256(B * H * W * 64) + r256(B * 64)


def test_quantized_module_refuses_cpu_input_and_other_shapes(hard_cases):
    import torch
    from wakeword_trainer_home_amd._native import NativeError
    from wakeword_trainer_home_amd.export import QuantizedCNNSmall
    header, arrays, x, _ = hard_cases[(3, 13, 21)]
    model = QuantizedCNNSmall(header, arrays)
    assert model.hip_backed and not model.training and not list(model.parameters())
    assert not any(t.requires_grad for t in model.buffers()) and model.form in ("pair", "fused")
    with pytest.raises(NativeError, match="no CPU fallback"):
        model(torch.from_numpy(x))
    with pytest.raises(ValueError, match="features of shape"):
        model(torch.zeros(1, 1, 14, 21))
    with pytest.raises(RuntimeError):
        model.train()
    with pytest.raises(ValueError):
        QuantizedCNNSmall(dict(header, kind="fp32"), arrays)


# ------------------------------------------------------------------ quantisation error against the float64 model
def test_quantisation_error_on_the_golden_fixture():
    """Interpreter on the exported bundle of the fixture vs. the float64 model, over its 32 structured feature maps.
    Recorded for the restated law (tests/golden/q8_errors.json): max |dlogit| 0.723, mean 0.27, with logit margins from
    -45.5 to -25.4 across the samples.  The interpreter is held to twice the record; the factor covers a re-seeded fixture."""
    z = np.load(GOLDEN / "g13_q8_cnn_small.npz")
    rec = json.loads((GOLDEN / "q8_errors.json").read_text())["cnn_small"]
    state = {k[len("state/"):]: z[k] for k in z.files if k.startswith("state/")}
    x = z["x"].astype(np.float32)
    assert x.shape == (32, 1, 40, 151) and rec["samples"] == 32
    logits, ranges = Q.float_forward(state, x)
    _, cal = Q.float_forward(state, x[:16])
    assert cal["x_min"] == float(z["x_min"]) and cal["a_max"] == z["a_max"].tolist() and cal["p_max"] == float(z["p_max"])
    assert min(np.sqrt(state[k]).min() for k in state if k.endswith("running_var")) > 0.5           # non-trivial statistics
    assert max(np.abs(state[k]).max() for k in state if k.endswith("running_mean")) > 0.5
    arrays, _ = QZ.quantize_cnn_small(state, (40, 151), float(z["x_min"]), float(z["x_max"]), z["a_max"].tolist(), float(z["p_max"]))
    q = R.run_int8(Q.header_for(40, 151), arrays, x)["logits"]
    d = np.abs(q.astype(np.float64) - logits)
    margin = logits[:, 1] - logits[:, 0]
    print(f"MEASURED max |dlogit| {d.max():.4g} (recorded {rec['max_abs_dlogit']}), mean {d.mean():.4g}; "
          f"margin {margin.min():.4g} .. {margin.max():.4g}")
    assert margin.max() - margin.min() > 20 * rec["max_abs_dlogit"], "the margins vary too little to show a quantisation error"
    assert d.max() <= 2 * rec["max_abs_dlogit"]
