"""The int8 ``MobileNetV3Wakeword`` path on the host (no GPU): the interpreter and the quantiser against the restated law of
tests/q8_mobilenet_cases.py, the bundle check, the runtime module's refusals, the interface, and the golden fixture."""
import json
import re
from pathlib import Path

import numpy as np
import pytest
import torch

from tests import q8_mobilenet_cases as MQ
from wakeword_trainer_home_amd.export import bundle as BU
from wakeword_trainer_home_amd.export import quantize as QZ
from wakeword_trainer_home_amd.export import reference as R

REPO = Path(__file__).resolve().parent.parent
GOLDEN = Path(__file__).resolve().parent / "golden"
MQ8_NAMES = ["ww_mq8_conv1x1_fwd", "ww_mq8_dwconv_fwd", "ww_mq8_gate_fwd", "ww_mq8_head_fwd", "ww_mq8_mobilenetv3_fwd",
             "ww_mq8_mobilenetv3_workspace_bytes", "ww_mq8_se_fwd", "ww_mq8_stem_fwd"]


# ------------------------------------------------------------------ the interpreter against the restatement
@pytest.mark.parametrize("name", list(MQ.CASES))
def test_interpreter_equals_restated_law_on_every_tensor(name):
    header, arrays, x, ref = MQ.case(name)
    got = R.run_int8(header, arrays, x, want_acc=True)                  # dispatches on the header's architecture
    assert set(got) == set(ref)
    assert [k for k in got if "/" not in k] == MQ.stages() == R.mbv3_stages()
    for key, want in ref.items():
        assert got[key].shape == want.shape and np.array_equal(got[key], want), key
        if "/" not in key or key.startswith("u/"):
            assert got[key].dtype == want.dtype, key
    plain = R.run_int8_mobilenetv3(header, arrays, x)
    assert list(plain) == MQ.stages() and np.array_equal(plain["logits"], ref["logits"])
    assert plain["logits"].dtype == np.float32 and plain["logits"].shape == (x.shape[0], header["num_classes"])


def test_the_cases_reach_what_they_are_for():
    """The hard bundles assert their own clamps while they are built (``assert_hard``); here: the shapes, the dead layer's floor, the
    non-finite inputs."""
    _, arrays, x, ref = MQ.case("hard_tiny")
    assert np.isnan(x).any() and np.isposinf(x).any() and np.isneginf(x).any()
    assert ref["xq"][0, 0, 0] == arrays["input_zero"][0]               # NaN -> the zero point
    assert [ref[k].shape[1:3] for k in ("stem", "b0.dw", "b1.dw", "b3.dw", "b8.dw")] == [(8, 12), (4, 6), (2, 3), (1, 2), (1, 1)]
    assert all((arrays[f"b{i}.dw.w"][MQ.ZERO_CH] == 0).all() for i in range(11))
    assert [ref[k].shape[1:3] for k in ("stem", "b0.dw", "b1.dw", "b3.dw", "b8.dw")] != \
        [MQ.case("hard_odd")[3][k].shape[1:3] for k in ("stem", "b0.dw", "b1.dw", "b3.dw", "b8.dw")]
    assert MQ.case("hard_odd")[3]["stem"].shape[1:3] == (7, 11)         # odd at every stride-2 layer: 13x21 -> 7x11 -> 4x6 -> 2x3 ..
    _, dead, _, dref = MQ.case("dead")
    m, sh = MQ.r_encode_multiplier(1.0)
    assert (dref["b1.expand"] == 127).any() or (dref["b1.expand"] == -128).all()        # s_out = 2^-20: anything positive saturates
    assert np.abs(dref["b2.out"].astype(int)).max() == 128 or (dref["b2.out"] == 0).all()
    assert (m, sh) == (2 ** 30, 30) and MQ.r_encode_multiplier(1 / 255) == (1077952576, 38) == (R.GATE_MULT, R.GATE_SHIFT)
    for name in ("tiny", "hard_tiny"):
        a = MQ.case(name)[1]
        assert all((int(a[f"b{i}.gate.m"][0]), int(a[f"b{i}.gate.sh"][0])) == (1077952576, 38) for i in (0, 3, 10))
        assert (int(a["pool.m"][0]), int(a["pool.sh"][0]), int(a["pool.hw"][0])) == (2 ** 30, 30, 1)


# ------------------------------------------------------------------ the quantiser
def _fixture():
    z = np.load(GOLDEN / "g18_q8_mobilenetv3.npz")
    meta = json.loads(bytes(z["meta"]).decode())
    state = MQ.random_state(meta["num_classes"], meta["seed"], meta["gain"])
    cal = {"x_min": float(z["x_range"][0]), "x_max": float(z["x_range"][1]),
           "ranges": {n: [float(v[0]), float(v[1])] for n, v in zip(MQ.range_names(), z["ranges"])}}
    return z, meta, state, cal


def test_fixture_parameters_regenerate():
    z, meta, state, _ = _fixture()
    keys = [k for k in z.files if k.startswith("psamp.")]
    assert len(keys) >= 8
    for k in keys:
        flat = np.asarray(state[k[len("psamp."):]], np.float32).reshape(-1)
        assert np.array_equal(z[k], flat[:: max(1, flat.size // 16)][:16]), k
    bn = [k for k in state if k.endswith("running_mean") or k.endswith("running_var")]
    assert bn and all(np.ptp(state[k]) > 0.1 for k in bn)                # non-trivial running statistics


def test_quantize_mobilenetv3_equals_the_restated_quantiser_on_the_fixture():
    z, meta, state, cal = _fixture()
    F, T = meta["feature_shape"]
    got, scales = QZ.quantize_mobilenetv3(state, (F, T), cal)
    want = MQ.r_quantize_model(state, (F, T), cal)
    assert set(got) == set(want)
    for k in want:
        assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), k
    assert all(np.isfinite(v) and v > 0 for v in scales.values())
    assert all(k + ".tab" in got for k in ["stem", "last", "cls0"] + [f"b{i}.{s}" for i in range(3, 11) for s in ("expand", "dw")])
    assert not any(f"b{i}.{s}.tab" in got for i in range(3) for s in ("expand", "dw"))
    BU.check_bundle(MQ.header_for(F, T, meta["num_classes"]), got)


def test_bias_refusal_names_layer_and_channel():
    _, meta, state, cal = _fixture()
    F, T = meta["feature_shape"]
    st = dict(state)
    b = st["mobilenet.features.2.block.1.1.bias"].copy()
    b[5] = 1e30
    st["mobilenet.features.2.block.1.1.bias"] = b
    with pytest.raises(QZ.QuantizationError, match=r"b1\.dw, channel 5"):
        QZ.quantize_mobilenetv3(st, (F, T), cal)
    st = dict(state)
    b = st["mobilenet.features.4.block.2.fc2.bias"].copy()
    b[7] = -1e30
    st["mobilenet.features.4.block.2.fc2.bias"] = b
    with pytest.raises(QZ.QuantizationError, match=r"b3\.fc2, channel 7"):
        QZ.quantize_mobilenetv3(st, (F, T), cal)
    bad = dict(cal, ranges=dict(cal["ranges"], **{"b4.out": [float("nan"), 1.0]}))
    with pytest.raises(QZ.QuantizationError, match="not finite"):
        QZ.quantize_mobilenetv3(state, (F, T), bad)
    with pytest.raises(QZ.QuantizationError, match="lack"):
        QZ.quantize_mobilenetv3(state, (F, T), dict(cal, ranges={}))
    with pytest.raises(QZ.QuantizationError, match="classes"):
        QZ.quantize_mobilenetv3(MQ.random_state(65, 0), (F, T), cal)


def test_hardswish_table_is_the_law():
    for s_u, z_u, s_o, z_o in ((0.05, -20, 0.03, -110), (0.3, 5, 0.2, -128), (2.0 ** -20, 0, 2.0 ** -20, 0)):
        t = QZ.hardswish_table(np.float32(s_u), z_u, np.float32(s_o), z_o)
        assert t.dtype == np.int8 and t.shape == (256,) and np.array_equal(t, MQ.r_table(np.float32(s_u), z_u, np.float32(s_o), z_o))
        assert t[z_u + 128] == z_o                                       # hs(0) = 0: a pad channel comes out as the zero point


def test_export_without_calibration_data_is_refused(tmp_path):
    from wakeword_trainer_home_amd.export.exporter import ExportConfig, ModelExporter
    exporter = ModelExporter.__new__(ModelExporter)
    exporter.calibration = None
    with pytest.raises(QZ.QuantizationError, match="calibration"):
        exporter._write_int8(tmp_path / "m.npz", {"architecture": "mobilenetv3"}, {}, ExportConfig(output_path=tmp_path / "m.npz"))
    exporter.calibration = [np.zeros((1, 1, 40, 38), np.float32)]
    with pytest.raises(QZ.QuantizationError, match="cnn_small only") as e:
        exporter._write_int8(tmp_path / "g.npz", {"architecture": "gru"}, {}, ExportConfig(output_path=tmp_path / "g.npz"))
    assert "mobilenetv3" in str(e.value).split("not 'gru'")[0]          # named among the covered
    with pytest.raises(BU.BundleError, match="int8 form"):
        BU.check_bundle(dict(MQ.header_for(16, 24), architecture="gru"), MQ.case("tiny")[1])


# ------------------------------------------------------------------ the bundle
def test_round_trip_preserves_dtypes_and_values(tmp_path):
    header, arrays, x, ref = MQ.case("odd")
    path = BU.write_bundle(tmp_path / "m_int8.npz", header, arrays)
    h2, a2 = BU.load_bundle(path)
    assert h2 == header and set(a2) == set(arrays)
    for k, v in arrays.items():
        assert a2[k].dtype == v.dtype and np.array_equal(a2[k], v), k
    BU.check_bundle(h2, a2)
    assert np.array_equal(R.run_int8(h2, a2, x)["logits"], ref["logits"])


def _breakers():
    def drop(key):
        return lambda h, a: a.pop(key)

    def put(key, value):
        return lambda h, a: a.__setitem__(key, value(a[key]))

    def head(key, value):
        return lambda h, a: h.__setitem__(key, value)

    def poke(key, idx, value):
        def f(h, a):
            v = a[key].copy()
            v.reshape(-1)[idx] = value
            a[key] = v
        return f
    return {"missing_array": drop("b3.fc1.w"), "missing_table": drop("b5.dw.tab"), "missing_hw": drop("b0.pool.hw"),
            "wrong_dtype": put("b1.expand.w", lambda v: v.astype(np.int16)), "wrong_shape": put("b2.dw.w", lambda v: v[:, :8]),
            "bias_dtype": put("last.b", lambda v: v.astype(np.int64)), "mult_low": poke("b4.project.m", 3, 2 ** 30 - 1),
            "shift_zero": poke("cls0.sh", 100, 0), "shift_63": poke("b0.gate.sh", 0, 63), "res_mult": poke("b2.res.m", 0, 5),
            "weight_m128": poke("b6.fc2.w", 11, -128), "fc_m128": poke("fc.w", 1, -128),
            "table_uint8": put("stem.tab", lambda v: v.view(np.uint8)), "table_short": put("last.tab", lambda v: v[:255]),
            "zu_outside": poke("cls0.zu", 0, 200), "hw_mismatch": poke("b3.pool.hw", 0, 3), "pool_hw": poke("pool.hw", 0, 2),
            "feature_shape": head("feature_shape", [40, 45]), "fc_scale_nan": poke("fc.scale", 0, np.nan),
            "classes_65": head("num_classes", 65), "classes_1": head("num_classes", 1), "input_scale": poke("input_scale", 0, 0.0)}


@pytest.mark.parametrize("name", list(_breakers()))
def test_malformed_bundles_are_rejected_and_reported(name, tmp_path):
    from wakeword_trainer_home_amd.export import validate_exported_model
    header, arrays, _, _ = MQ.case("tiny")
    h, a = json.loads(json.dumps(header)), dict(arrays)
    _breakers()[name](h, a)
    with pytest.raises(BU.BundleError):
        BU.check_bundle(h, a)
    res = validate_exported_model(BU.write_bundle(tmp_path / "bad.npz", h, a))
    assert res["valid"] is False and res["error"], name


def test_check_bundle_accepts_every_case():
    for name in MQ.CASES:
        header, arrays, _, _ = MQ.case(name)
        BU.check_bundle(header, arrays)


# ------------------------------------------------------------------ the runtime module and the interface
def test_quantized_module_refuses_cpu_input_and_other_shapes():
    from wakeword_trainer_home_amd import _native
    from wakeword_trainer_home_amd.export import QuantizedMobileNetV3
    header, arrays, x, _ = MQ.case("tiny")
    net = QuantizedMobileNetV3(header, arrays)
    assert not net.training and net.num_classes == 2 and net.feature_shape == (16, 24) and not list(net.parameters())
    assert len(net._names) == _native.MQ8_NPTR == 260
    with pytest.raises(_native.NativeError):
        net(torch.from_numpy(x))
    with pytest.raises(ValueError, match="features of shape"):
        net(torch.zeros(2, 1, 16, 25))
    with pytest.raises(ValueError, match="float32"):
        net(torch.zeros(2, 1, 16, 24, dtype=torch.float64))
    with pytest.raises(RuntimeError, match="no training mode"):
        net.train()
    with pytest.raises(ValueError, match="mobilenetv3"):
        QuantizedMobileNetV3(dict(header, kind="fp32"), {"state/x": np.zeros(1, np.float32)})
    # the device layout: channel counts padded to 64, zero weights, multipliers that leave the zero point
    w, b, m, sh, tab = net.conv("b1.expand")
    assert tuple(w.shape) == (128, 64) and not w[72:].any() and not w[:, 16:].any() and tab is None
    assert not b[72:].any() and (m[72:] == 2 ** 30).all() and (sh[72:] == 31).all()
    w, b, m, sh, tab = net.conv("b3.dw")
    assert tuple(w.shape) == (25, 128) and not w[:, 96:].any() and tab.dtype == torch.int8 and tab.numel() == 256
    assert tuple(net.conv("stem")[0].shape) == (9, 64) and tuple(net.conv("cls0")[0].shape) == (1024, 576)
    assert tuple(net.conv("b3.fc1")[0].shape) == (24, 96) and net.conv("b0.expand")[0] is None


def test_header_and_exports_agree_on_the_mq8_entry_points():
    import ctypes
    from wakeword_trainer_home_amd import _native
    header = (REPO / "include" / "wwhip.h").read_text()
    declared = set(re.findall(r"\b(ww_[a-z0-9_]+)\s*\(", header))
    assert declared == set(_native.EXPORTS)
    assert sorted(n for n in declared if n.startswith("ww_mq8_")) == MQ8_NAMES
    assert _native.ABI_VERSION == 17 and re.search(r"#define\s+WW_ABI_VERSION\s+17\b", header)
    for name, value in (("BLOCKS", 11), ("BLOCK_NPTR", 22), ("NPTR", 260), ("LAST", 576), ("HIDDEN", 1024), ("RELU", 0), ("HSWISH", 1),
                        ("SIGNED", 2)):
        assert re.search(rf"#define\s+WW_MQ8_{name}\s+{value}\b", header) and getattr(_native, "MQ8_" + name) == value
    assert ctypes.sizeof(_native.Mq8Io) == 4 * (3 + 8 + 10 * 11)
    assert "ww_q8_mobilenet.hip" in (REPO / "wakeword_trainer_home_amd" / "csrc" / "Makefile").read_text()
    import wakeword_trainer_home_amd.export as E
    assert {"QuantizedMobileNetV3", "calibrate_mobilenetv3"} <= set(E.__all__)


# ------------------------------------------------------------------ the golden fixture
def test_fixture_logits_within_the_recorded_loss_and_margins_span_it():
    z, meta, state, cal = _fixture()
    errors = json.loads((GOLDEN / "q8_mobilenetv3_errors.json").read_text())
    F, T = meta["feature_shape"]
    x = z["x"].astype(np.float32)
    arrays, _ = QZ.quantize_mobilenetv3(state, (F, T), cal)
    header = MQ.header_for(F, T, meta["num_classes"])
    BU.check_bundle(header, arrays)                                       # (fails on the parent commit: no int8 form)
    got = R.run_int8(header, arrays, x)["logits"].astype(np.float64)      # (fails on the parent commit: no such interpreter)
    want = z["logits64"]
    loss = np.abs(got - want)
    print(f"max |dlogit| {loss.max():.6f} (recorded {errors['max_abs_dlogit']:.6f}), mean {loss.mean():.6f}")
    assert loss.max() <= 2.0 * errors["max_abs_dlogit"]
    margin = want[:, 1] - want[:, 0]
    span = float(margin.max() - margin.min())
    print(f"margin span {span:.4f}, factor {span / errors['max_abs_dlogit']:.1f} (recorded {errors['factor']:.1f})")
    assert span >= errors["factor"] * errors["max_abs_dlogit"] * (1 - 1e-9)
    assert errors["factor"] >= 20.0 or errors.get("shortfall"), "a factor below 20 must be recorded as a shortfall"
