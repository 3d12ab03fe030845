"""The ResNet18 half of the export package without a GPU: the NumPy interpreter and ``quantize_resnet18`` against the restated law
(tests/q8_resnet_cases.py) bit for bit, the refusals, the floors, the bundle file, the ABI names, and the quantisation error
against the float64 model on the committed fixture."""
import json
import re
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from tests import q8_resnet_cases as RQ
from wakeword_trainer_home_amd.export import bundle as BU
from wakeword_trainer_home_amd.export import quantize as QZ
from wakeword_trainer_home_amd.export import reference as R

REPO = Path(__file__).resolve().parent.parent
GOLDEN = Path(__file__).resolve().parent / "golden"
RQ8_NAMES = ["ww_rq8_conv2d_fwd", "ww_rq8_maxpool_fwd", "ww_rq8_resnet18_fwd", "ww_rq8_resnet18_workspace_bytes", "ww_rq8_stem_fwd"]
F_, T_ = 40, 33


@pytest.fixture(scope="module")
def golden():
    """(fixture arrays, its error record, the regenerated float32 state, float32 features) -- shared, never modified."""
    z = np.load(GOLDEN / "g15_q8_resnet18.npz")
    rec = json.loads((GOLDEN / "q8_resnet18_errors.json").read_text())["ResNet18Wakeword"]
    return z, rec, RQ.random_state(2, seed=int(z["param_seed"]), gain=float(z["gain"])), z["x"].astype(np.float32)


def _ranges(z):
    a = z["a_max"].tolist()
    return {"x_min": float(z["x_min"]), "x_max": float(z["x_max"]), "stem_max": a[0], "h1_max": a[1:9], "ds_max": a[9:12],
            "out_max": a[12:20], "p_max": a[20]}


# ------------------------------------------------------------------ the interpreter against the restatement
@pytest.mark.parametrize("name", list(RQ.CASES))
def test_interpreter_equals_restated_law_on_every_tensor(name):
    header, arrays, x, ref = RQ.hard_case(name)
    B, F, T, nc = RQ.CASES[name]
    out = R.run_int8(header, arrays, x, want_acc=True)
    want = RQ.stages()
    assert [k for k in out if not k.startswith("acc/")] == want == R.resnet_stages()
    assert sorted(k for k in out if k.startswith("acc/")) == sorted("acc/" + n for n, *_ in RQ.convs())
    for stage in want + [k for k in out if k.startswith("acc/")]:
        assert out[stage].dtype == ref[stage].dtype and out[stage].shape == ref[stage].shape, stage
        assert np.array_equal(out[stage], ref[stage]), stage
    assert list(R.run_int8(header, arrays, x)) == want                      # the accumulators come on request only
    hw = RQ.stage_shapes(F, T)
    assert out["xq"].shape == (B, F, T) and out["stem"].shape == (B, *hw[0], 64) and out["pool0"].shape == (B, *hw[1], 64)
    assert out["l4.1.out"].shape == (B, *hw[4], 512) and out["logits"].shape == (B, nc) and out["logits"].dtype == np.float32
    with pytest.raises(ValueError, match="features of shape"):
        R.run_int8(header, arrays, np.zeros((1, 1, F, T + 1), np.float32))


def test_stage_sizes_follow_the_floor_formulas():
    assert RQ.stage_shapes(40, 33) == [(20, 17), (10, 9), (5, 5), (3, 3), (2, 2)]
    assert RQ.stage_shapes(9, 6) == [(5, 3), (3, 2), (2, 1), (1, 1), (1, 1)]
    assert RQ.stage_shapes(40, 151)[2:] == [(5, 19), (3, 10), (2, 5)] and RQ.stage_shapes(128, 251)[-1] == (4, 8)
    for n in range(1, 40):
        assert R.resnet_half(n) == RQ.half(n) == (n + 6 - 7) // 2 + 1 == (n + 2 - 3) // 2 + 1 == (n - 1) // 2 + 1
    assert [(n, s, d) for n, _, _, s, d in R.resnet_blocks()] == [(n, s, d) for n, _, _, s, d in RQ.blocks()]


# ------------------------------------------------------------------ the derivation against the restatement
@pytest.mark.parametrize("variant", ["plain", "dead", "flat_ds"])
def test_export_derivation_equals_restated_law(variant):
    state = RQ.random_state(3, seed=4, gain=0.7, dead="l2.1.conv1" if variant == "dead" else None, flat_ds=variant == "flat_ds")
    x = RQ.structured_features(4, F_, T_, seed=4)
    _, ranges = RQ.float_forward(state, x[:2])
    arrays, scales = QZ.quantize_resnet18(state, (F_, T_), ranges)
    want = RQ.r_quantize_model(state, (F_, T_), ranges)
    assert sorted(arrays) == sorted(want)
    for key in want:
        assert arrays[key].dtype == want[key].dtype and arrays[key].shape == want[key].shape and np.array_equal(arrays[key], want[key]), key
    assert arrays["stem.w"].shape == (64, 1, 7, 7) and arrays["l3.0.down.w"].shape == (256, 128, 1, 1)
    assert arrays["l4.1.conv2.w"].shape == (512, 512, 3, 3) and arrays["fc.w"].shape == (3, 512)
    assert not arrays["l1.0.conv2.w"][RQ.ZERO_CH].any()                         # the all-zero channel of random_state
    assert "l1.0.down.w" not in arrays and "l2.1.down.w" not in arrays and "l2.0.down.w" in arrays
    header = RQ.header_for(F_, T_, 3)
    BU.check_bundle(header, arrays)
    out, ref = R.run_int8(header, arrays, x), RQ.r_forward(arrays, x)
    for stage in RQ.stages():
        assert np.array_equal(out[stage], ref[stage]), stage
    if variant == "dead":                                                       # the dead-layer floor
        assert ranges["h1_max"][3] == 0.0 and scales["l2.1.h1"] == 2.0 ** -20 and (out["l2.1.h1"] == -128).all()
    if variant == "flat_ds":                                                    # the floor of the signed tensor
        assert ranges["ds_max"][1] == 0.0 and scales["l3.0.ds"] == 2.0 ** -20 and (out["l3.0.ds"] == 0).all()
        assert QZ.signed_scale(-1.0) == QZ.signed_scale(0.0) == 2.0 ** -20 and QZ.signed_scale(127.0) == 1.0


def test_export_refuses_what_the_law_cannot_hold(golden):
    z, _, state, _ = golden
    r = _ranges(z)
    QZ.quantize_resnet18(state, (F_, T_), r)

    def with_bias(key, ch, value):
        bad = dict(state)
        bad[key] = state[key].copy()
        bad[key][ch] = value
        return bad
    for key, ch, value, pattern in (("resnet.layer2.1.bn2.bias", 11, 1e12, r"l2\.1\.conv2, channel 11"),
                                    ("resnet.layer3.0.downsample.1.bias", 3, -1e12, r"l3\.0\.down, channel 3"),
                                    ("resnet.bn1.bias", 63, 1e12, r"stem, channel 63"),
                                    ("resnet.fc.1.bias", 1, 1e12, r"classifier, channel 1")):
        with pytest.raises(QZ.QuantizationError, match=pattern):                  # a bias overflow names layer and channel
            QZ.quantize_resnet18(with_bias(key, ch, value), (F_, T_), r)
    # the bound is k k Cin 127 255 for a conv (49 for the stem), 512 127 255 for the classifier
    s_w = np.ones(64)
    for acc_max, layer in ((49 * 127 * 255, "stem"), (9 * 64 * 127 * 255, "l1.0.conv1"), (512 * 127 * 255, "classifier")):
        assert QZ.quantize_bias(np.full(64, float(2 ** 31 - 1 - acc_max)), 1.0, s_w, acc_max, layer)[0] > 0
        with pytest.raises(QZ.QuantizationError, match=f"{layer}, channel 0"):
            QZ.quantize_bias(np.full(64, float(2 ** 31 - acc_max)), 1.0, s_w, acc_max, layer)
    for value in (float("nan"), float("inf")):                                    # a non-finite maximum
        for key, idx in (("h1_max", 4), ("ds_max", 0), ("out_max", 7)):
            rr = dict(r, **{key: list(r[key])})
            rr[key][idx] = value
            with pytest.raises(QZ.QuantizationError, match="not finite"):
                QZ.quantize_resnet18(state, (F_, T_), rr)
    bad = dict(state)                                                             # a multiplier that rounds to zero
    bad["resnet.layer1.0.conv1.weight"] = state["resnet.layer1.0.conv1.weight"].copy()
    bad["resnet.layer1.0.conv1.weight"][2] *= 1e-30
    with pytest.raises(QZ.QuantizationError, match=r"l1\.0\.conv1, channel 2"):
        QZ.quantize_resnet18(bad, (F_, T_), r)
    with pytest.raises(QZ.QuantizationError, match="l2.0.res"):
        QZ.encode_multiplier(0.0, "l2.0.res")
    with pytest.raises(QZ.QuantizationError, match="maxima"):
        QZ.quantize_resnet18(state, (F_, T_), dict(r, ds_max=r["ds_max"][:2]))
    bad = dict(state)
    bad["resnet.fc.1.weight"], bad["resnet.fc.1.bias"] = np.zeros((65, 512), np.float32), np.zeros(65, np.float32)
    with pytest.raises(QZ.QuantizationError, match="classes"):
        QZ.quantize_resnet18(bad, (F_, T_), r)
    with pytest.raises(QZ.QuantizationError, match="ResNet18Wakeword"):
        QZ.quantize_resnet18({"classifier.weight": np.zeros((2, 64))}, (F_, T_), r)


# ------------------------------------------------------------------ the bundle file
def test_bundle_round_trip_and_plain_readability(tmp_path):
    header, arrays, x, ref = RQ.hard_case("tiny")
    path = BU.write_bundle(tmp_path / "r_int8.npz", header, arrays)
    h2, a2 = BU.load_bundle(path)
    assert h2 == header and sorted(a2) == sorted(arrays)
    for k in arrays:
        assert a2[k].dtype == arrays[k].dtype and np.array_equal(a2[k], arrays[k]), k
    code = ("import sys, json, numpy as np\n"
            "z = np.load(sys.argv[1], allow_pickle=False)\n"
            "h = json.loads(bytes(z['header']).decode('utf-8'))\n"
            "assert not any(m.startswith(('torch', 'wakeword')) for m in sys.modules)\n"
            "print(json.dumps([h['kind'], h['architecture'], sorted(z.files), int(z['l3.0.down.m'][5])]))\n")
    r = subprocess.run([sys.executable, "-c", code, str(path)], capture_output=True, text=True, cwd=tmp_path)
    assert r.returncode == 0, r.stderr
    kind, arch, files, m = json.loads(r.stdout)
    assert (kind, arch, m) == ("int8", "ResNet18Wakeword", 2 ** 30) and files == sorted(list(arrays) + ["header"])


def test_float_bundles_round_trip(tmp_path, golden):
    """fp32 and fp16 bundles of the class: written, checked, read back -- fp32 exactly, fp16 as every weight rounded once."""
    _, _, state, _ = golden
    for kind in ("fp32", "fp16"):
        h = BU.make_header(kind, "ResNet18Wakeword", 2, (1, 1, F_, T_), [k for k in state if k.endswith("weight")])
        a = BU.float_arrays(state, fp16=kind == "fp16")
        BU.check_bundle(h, a)
        h2, a2 = BU.load_bundle(BU.write_bundle(tmp_path / f"r_{kind}.npz", h, a))
        BU.check_bundle(h2, a2)
        assert h2 == h and len(a2) == 122
        for k, v in state.items():
            got = a2[BU.STATE_PREFIX + k]
            if v.dtype == np.int64:
                assert got.dtype == np.int64 and np.array_equal(got, v)
            elif kind == "fp32":
                assert got.dtype == np.float32 and np.array_equal(got, v), k
            else:
                assert got.dtype == np.float16 and np.array_equal(got, v.astype(np.float16)), k


def _malformed():
    def drop(a, h):
        del a["l2.1.conv2.sh"]

    def drop_down(a, h):
        del a["l3.0.down.w"]

    def drop_res(a, h):
        del a["l1.1.res.m"]

    def shape(a, h):
        a["l1.0.conv1.w"] = a["l1.0.conv1.w"].reshape(64, 9, 64)           # the device layout is not the bundle's

    def stem_shape(a, h):
        a["stem.w"] = a["stem.w"].reshape(64, 49)

    def dtype(a, h):
        a["l2.0.conv1.b"] = a["l2.0.conv1.b"].astype(np.int64)

    def mult_low(a, h):
        a["l4.0.res.m"][0] = 2 ** 30 - 1

    def mult_negative(a, h):
        a["l1.0.conv2.m"][0] = -(2 ** 30)

    def shift_zero(a, h):
        a["l2.0.down.sh"][0] = 0

    def shift_high(a, h):
        a["pool.sh"][0] = 63

    def weight_min(a, h):
        a["l4.1.conv1.w"][1, 1, 0, 2] = -128

    def fc_weight_min(a, h):
        a["fc.w"][0, 3] = -128

    def classes(a, h):
        h["num_classes"] = 3

    def too_many_classes(a, h):
        h["num_classes"] = 65

    def feature_shape(a, h):
        h["feature_shape"] = [9]

    def arch(a, h):
        h["architecture"] = "gru"

    def scale(a, h):
        a["fc.scale"][1] = np.inf

    def input_zero(a, h):
        a["input_zero"][0] = 128
    return [drop, drop_down, drop_res, shape, stem_shape, dtype, mult_low, mult_negative, shift_zero, shift_high, weight_min,
            fc_weight_min, classes, too_many_classes, feature_shape, arch, scale, input_zero]


def test_malformed_bundles_are_invalid_not_errors(tmp_path):
    from wakeword_trainer_home_amd.export import validate_exported_model
    header, arrays = RQ.hard_bundle(9, 6, 2)
    BU.check_bundle(header, arrays)
    good = validate_exported_model(BU.write_bundle(tmp_path / "good.npz", header, arrays))
    assert good["valid"] is True and good["error"] is None and good["graph"] == len(header["layers"]) == 22
    assert good["inputs"] == [("input", [0, 1, 9, 6])] and good["outputs"] == [("output", [0, 2])]
    for breaker in _malformed():
        a, h = {k: v.copy() for k, v in arrays.items()}, dict(header)
        breaker(a, h)
        with pytest.raises(BU.BundleError):
            BU.check_bundle(h, a)
        if breaker.__name__ in ("drop", "mult_low", "arch"):                   # (written in full 11 MB each: three stand for all)
            res = validate_exported_model(BU.write_bundle(tmp_path / f"{breaker.__name__}.npz", h, a))
            assert res["valid"] is False and res["error"], breaker.__name__


def test_int8_error_wording_for_other_architectures_is_unchanged(tmp_path):
    """``_write_int8`` is reached after the float bundle is written; for an architecture outside the three its message keeps the
    words ``cnn_small only`` (tests/test_export_gpu.py looks for them on a gru)."""
    from wakeword_trainer_home_amd.export.exporter import ExportConfig, ModelExporter
    exporter = ModelExporter.__new__(ModelExporter)
    exporter.calibration = [np.zeros((1, 1, 40, 38), np.float32)]
    with pytest.raises(QZ.QuantizationError, match="cnn_small only") as e:
        exporter._write_int8(tmp_path / "g.npz", {"architecture": "gru"}, {}, ExportConfig(output_path=tmp_path / "g.npz"))
    assert "'gru'" in str(e.value) and "ResNet18Wakeword" in str(e.value)
    with pytest.raises(BU.BundleError, match="int8 form"):
        BU.check_bundle(dict(RQ.header_for(9, 6), architecture="gru"), {})


# ------------------------------------------------------------------ interface
def test_header_and_exports_agree_on_the_rq8_entry_points():
    import ctypes
    from wakeword_trainer_home_amd import _native
    header = (REPO / "include" / "wwhip.h").read_text()
    declared = set(re.findall(r"\b(ww_[a-z0-9_]+)\s*\(", header))
    assert declared == set(_native.EXPORTS)
    assert sorted(n for n in declared if n.startswith("ww_rq8_")) == RQ8_NAMES
    assert _native.ABI_VERSION == 17 and _native.load().ww_abi_version() == 17
    assert (_native.RQ8_NPTR, _native.RQ8_RELU, _native.RQ8_SIGNED, _native.RQ8_ADD) == (103, 0, 1, 2)
    for name, value in (("NPTR", 103), ("RELU", 0), ("SIGNED", 1), ("ADD", 2)):
        assert re.search(rf"#define\s+WW_RQ8_{name}\s+{value}\b", header)
    assert ctypes.sizeof(_native.Rq8Io) == 4 * (5 + 2 * 8)
    makefile = (REPO / "wakeword_trainer_home_amd" / "csrc" / "Makefile").read_text()
    assert "ww_q8_resnet.hip" in makefile
    # the workspace the header describes: xq, stem, pool0, then h1, [ds,] out per block, then pool, each rounded up to 256 bytes
    r256 = lambda n: (n + 255) // 256 * 256       # noqa: E731
    for B, F, T in [(b, f, t) for b, f, t, _ in RQ.CASES.values()] + [(128, 40, 151), (128, 128, 251)]:
        hw = RQ.stage_shapes(F, T)
        want = r256(B * F * T) + r256(B * hw[0][0] * hw[0][1] * 64) + r256(B * hw[1][0] * hw[1][1] * 64) + r256(B * 512)
        for s, planes in enumerate(RQ.PLANES):
            act = r256(B * hw[s + 1][0] * hw[s + 1][1] * planes)
            want += (5 if s else 4) * act
        assert _native.rq8_resnet18_workspace_bytes(B, F, T) == want
    assert _native.rq8_resnet18_workspace_bytes(0, 40, 33) == 0 and _native.rq8_resnet18_workspace_bytes(1, 0, 33) == 0


def test_quantized_resnet18_refuses_cpu_input_and_other_shapes():
    import torch
    import wakeword_trainer_home_amd.export as E
    from wakeword_trainer_home_amd._native import NativeError
    from wakeword_trainer_home_amd.models import create_model
    assert "QuantizedResNet18" in E.__all__ and "calibrate_resnet18" in E.__all__
    header, arrays, x, _ = RQ.hard_case("tiny")
    model = E.QuantizedResNet18(header, arrays)
    assert model.hip_backed and not model.training and not list(model.parameters())
    assert not any(t.requires_grad for t in model.buffers()) and model.num_classes == 2 and model.feature_shape == (9, 6)
    assert model.conv("stem")[0].shape == (64, 64) and model.conv("l2.0.conv1")[0].shape == (128, 9, 64)
    assert model.conv("l2.0.down")[0].shape == (128, 1, 64) and model.conv("l1.0.down") == (None,) * 4
    with pytest.raises(NativeError, match="no CPU fallback"):
        model(torch.from_numpy(x))
    with pytest.raises(ValueError, match="features of shape"):
        model(torch.zeros(1, 1, 9, 7))
    with pytest.raises(RuntimeError):
        model.train()
    with pytest.raises(ValueError):
        E.QuantizedResNet18(dict(header, kind="fp32"), arrays)
    from tests import q8_cases as Q
    with pytest.raises(ValueError):
        E.QuantizedResNet18(*Q.hard_bundle(13, 21))
    with pytest.raises(Exception):                                  # the factory still does not offer the class
        create_model("resnet18")


def test_device_layout_of_a_conv():
    from wakeword_trainer_home_amd.export.runtime import device_resnet_conv
    header, arrays, _, _ = RQ.hard_case("tiny")
    w, b, m, sh = device_resnet_conv(arrays, "l3.0.conv1", -128)
    q = arrays["l3.0.conv1.w"]
    assert w.shape == (256, 9, 128) and w.flags["C_CONTIGUOUS"]
    for kh in range(3):
        for kw in range(3):
            assert np.array_equal(w[:, kh * 3 + kw, :], q[:, :, kh, kw])
    assert np.array_equal(b, (arrays["l3.0.conv1.b"].astype(np.int64) + 128 * q.astype(np.int64).sum(axis=(1, 2, 3))).astype(np.int32))
    assert m is arrays["l3.0.conv1.m"] and sh is arrays["l3.0.conv1.sh"]
    ws, bs, _, _ = device_resnet_conv(arrays, "stem", 37)
    assert ws.shape == (64, 64) and np.array_equal(ws[:, 3 * 7 + 2], arrays["stem.w"][:, 0, 3, 2]) and not ws[:, 49:].any()
    assert np.array_equal(bs, (arrays["stem.b"].astype(np.int64) - 37 * arrays["stem.w"].astype(np.int64).sum(axis=(1, 2, 3))).astype(np.int32))


# ------------------------------------------------------------------ quantisation error against the float64 model
def test_quantisation_error_on_the_golden_fixture(golden):
    """Interpreter on the exported bundle of the fixture vs. the float64 model, over its 16 structured feature maps at (40,33).
    Recorded for the restated law (tests/golden/q8_resnet18_errors.json): max |dlogit| 0.0118, mean 0.00481, with logit margins
    from -0.5141 to -0.268 across the samples (a span of 20.9 times the maximum: the fixture's parameter gain, 0.5, is the one of
    those tried -- 0.4, 0.5, 0.7, 1.0, 1.5 -- at which the span exceeds the required 20 times).  The interpreter is held to twice
    the record; the factor covers a re-seeded fixture."""
    z, rec, state, x = golden
    F, T = rec["feature_shape"]
    assert x.shape == (16, 1, F, T) and rec["samples"] == 16 and rec["calibration_samples"] == 8
    for k, v in state.items():                                                    # the regenerated parameters are the fixture's
        idx = np.arange(v.size) if v.size <= 16 else np.linspace(0, v.size - 1, 16).astype(np.int64)
        assert np.array_equal(v.reshape(-1)[idx], z["psamp." + k]), k
    assert len(state) == 122
    logits, _ = RQ.float_forward(state, x)
    assert np.array_equal(logits, z["logits"])
    _, cal = RQ.float_forward(state, x[:8])
    assert cal["x_min"] == float(z["x_min"]) and RQ.flat_ranges(cal) == z["a_max"].tolist()
    arrays, _ = QZ.quantize_resnet18(state, (F, T), _ranges(z))
    q = R.run_int8(RQ.header_for(F, T), arrays, x)["logits"]
    d = np.abs(q.astype(np.float64) - logits)
    margin = logits[:, 1] - logits[:, 0]
    print(f"MEASURED max |dlogit| {d.max():.4g} (recorded {rec['max_abs_dlogit']}), mean {d.mean():.4g}; "
          f"margin {margin.min():.4g} .. {margin.max():.4g}")
    assert margin.max() - margin.min() > 20 * rec["max_abs_dlogit"], "the margins vary too little to show a quantisation error"
    assert d.max() <= 2 * rec["max_abs_dlogit"]
