"""The LSTM half of the export package without a GPU: the NumPy interpreter and ``quantize_lstm`` against the restated law
(tests/q8_lstm_cases.py) bit for bit, the law's symmetries, the refusals, the bundle file, the ABI names, and the quantisation
error against the reference's float64 model on the committed fixture."""
import json
import re
from pathlib import Path

import numpy as np
import pytest

from tests import q8_lstm_cases as LQ
from wakeword_trainer_home_amd.export import bundle as BU
from wakeword_trainer_home_amd.export import quantize as QZ
from wakeword_trainer_home_amd.export import reference as R

REPO = Path(__file__).resolve().parent.parent
GOLDEN = Path(__file__).resolve().parent / "golden"
LQ8_NAMES = ["ww_lq8_head_fwd", "ww_lq8_lstm_fwd", "ww_lq8_lstm_layer_fwd", "ww_lq8_lstm_workspace_bytes", "ww_lq8_proj_fwd"]


# ------------------------------------------------------------------ the interpreter against the restatement
@pytest.mark.parametrize("name", list(LQ.CASES))
def test_interpreter_equals_restated_law_on_every_tensor(name):
    header, arrays, x, ref, _ = LQ.case(name)
    BU.check_bundle(header, arrays)
    out = R.run_int8(header, arrays, x)
    want = LQ.stages(header["lstm"])
    assert list(out) == want == R.lstm_stages(header["lstm"])
    for stage in want:
        assert out[stage].dtype == ref[stage].dtype and out[stage].shape == ref[stage].shape, stage
        assert np.array_equal(out[stage], ref[stage]), stage
    B, T, I, _, bidir, nc, _ = LQ.CASES[name]
    nd = 2 if bidir else 1
    assert out["xq"].shape == (B, T, I) and out["xq"].dtype == np.int8
    assert out["l0.fwd.u"].shape == (B, T, 512) and out["l0.fwd.u"].dtype == np.int16
    assert out["l0.fwd.y"].shape == (B, T, 128) and out["l0.fwd.c"].shape == (B, 128) and out["l0.fwd.c"].dtype == np.int16
    assert out["hcat"].shape == (B, nd * 128) and out["logits"].shape == (B, nc) and out["logits"].dtype == np.float32
    seq = R.run_int8(header, arrays, np.ascontiguousarray(x[:, 0].transpose(0, 2, 1)))     # the (B,T,F) form
    assert all(np.array_equal(seq[k], out[k]) for k in want)
    with pytest.raises(ValueError, match="features of shape"):
        R.run_int8(header, arrays, np.zeros((1, 1, I + 1, T), np.float32))


def test_every_clamp_of_the_law_is_reached():
    reached = LQ.clamps_reached()
    assert set(reached) == set(LQ.CLAMPS)
    for clamp, names in reached.items():
        assert names, f"no case reaches the clamp {clamp}"
    for clamp in ("u_low", "u_high", "cell_low", "cell_high", "q_h_127"):
        assert "saturating" in reached[clamp]
    ref = LQ.case("saturating")[3]
    assert ref["l0.fwd.u"].min() == -32768 and ref["l0.fwd.u"].max() == 32767
    assert max(ref[f"l{k}.{d}.y"].max() for k in (0, 1) for d in LQ.DIRS) == 127


def test_nan_and_infinite_inputs_follow_the_input_rule():
    header, arrays, x, _, _ = LQ.case("uni")
    x = x.copy()
    x[0, 0, 3, 1], x[1, 0, 0, 0], x[2, 0, 5, 2] = np.nan, np.inf, -np.inf
    out = R.run_int8(header, arrays, x)
    ref = LQ.r_forward(header["lstm"], arrays, x)
    assert out["xq"][0, 1, 3] == int(arrays["input_zero"][0]) and out["xq"][1, 0, 0] == 127 and out["xq"][2, 2, 5] == -128
    for stage in LQ.stages(header["lstm"]):
        assert np.array_equal(out[stage], ref[stage]), stage
    assert np.isfinite(out["logits"]).all()


def test_reverse_direction_is_the_forward_direction_on_flipped_time():
    """A bundle whose two directions hold the same parameters: the reverse direction on x equals the forward one on x flipped."""
    header, arrays, x, _, _ = LQ.case("odd")
    a = dict(arrays)
    for key in list(a):
        if ".rev." in key:
            a[key] = a[key.replace(".rev.", ".fwd.")]
    one = dict(header, lstm=dict(header["lstm"], num_layers=1))
    out, flipped = R.run_int8(one, a, x), R.run_int8(one, a, x[..., ::-1].copy())
    assert np.array_equal(out["l0.rev.u"], flipped["l0.fwd.u"][:, ::-1])
    assert np.array_equal(out["l0.rev.y"], flipped["l0.fwd.y"][:, ::-1]) and np.array_equal(out["l0.rev.c"], flipped["l0.fwd.c"])
    assert np.array_equal(out["hcat"][:, 128:], flipped["hcat"][:, :128])
    assert not np.array_equal(out["l0.rev.y"], out["l0.fwd.y"])


def test_rolling_the_batch_rolls_every_output():
    header, arrays, x, ref, _ = LQ.case("odd")
    out = R.run_int8(header, arrays, np.roll(x, 5, axis=0))
    for stage in LQ.stages(header["lstm"]):
        assert np.array_equal(out[stage], np.roll(ref[stage], 5, axis=0)), stage


# ------------------------------------------------------------------ the derivation against the restatement
@pytest.mark.parametrize("name", ["odd", "uni", "classes"])
def test_export_derivation_equals_restated_law(name):
    B, T, I, layers, bidir, nc, gain = LQ.CASES[name]
    args = LQ.lstm_args(I, layers, bidir)
    state = LQ.random_state(args, nc, seed=5, gain=gain)
    arrays, scales = QZ.quantize_lstm(state, args, -9.5, 6.25)
    want = LQ.r_quantize_model(state, args, -9.5, 6.25)
    assert sorted(arrays) == sorted(want)
    for key in want:
        assert arrays[key].dtype == want[key].dtype and arrays[key].shape == want[key].shape, key
        assert np.array_equal(arrays[key], want[key]), key
    nd = 2 if bidir else 1
    assert arrays["l0.fwd.ih.w"].shape == (512, I) and arrays["l0.fwd.ih.w"].dtype == np.int8               # unpadded
    assert arrays["l0.fwd.hh.w"].shape == (512, 128) and arrays["fc.w"].shape == (nc, nd * 128)
    assert arrays["l0.fwd.ih.b"].dtype == arrays["l0.fwd.hh.m"].dtype == arrays["l0.fwd.hh.sh"].dtype == np.int32
    assert arrays["tab.sigmoid"].dtype == arrays["tab.tanh"].dtype == np.int16 and arrays["tab.tanh"].shape == (4096,)
    assert arrays["fc.scale"].dtype == np.float32 and ("l0.rev.ih.w" in arrays) == bidir
    if layers > 1:
        assert arrays["l1.fwd.ih.w"].shape == (512, nd * 128)
    assert not arrays["l0.fwd.hh.w"][7].any() and arrays["l0.fwd.hh.m"][7] == 2 ** 30 and arrays["l0.fwd.hh.sh"][7] == 29  # s_w = 1: r = 2
    assert scales["hidden"] == 2.0 ** -7 and scales["input"] == float(arrays["input_scale"][0])
    LQ.check_tables(arrays)
    assert arrays["tab.sigmoid"][2048] == 16384 and arrays["tab.tanh"][2048] == 0 and arrays["tab.tanh"][2304] == 24956
    assert arrays["tab.sigmoid"].min() == 11 and arrays["tab.sigmoid"].max() == 32757            # sigma(-8), sigma(8 - 1/256) in Q15
    assert arrays["tab.tanh"].min() == -32767 and arrays["tab.tanh"].max() == 32767
    BU.check_bundle(LQ.header_for(args, nc), arrays)


def test_export_refuses_what_the_law_cannot_hold():
    args = LQ.lstm_args(40, 2, True)
    state = LQ.random_state(args, 2, seed=4)
    QZ.quantize_lstm(state, args, -10.0, 5.0)

    def changed(key, index, value):
        bad = dict(state)
        bad[key] = state[key].copy()
        bad[key][index] = value
        return bad
    with pytest.raises(QZ.QuantizationError, match=r"l1\.rev\.hh, row 11"):                 # a bias overflow names layer and row
        QZ.quantize_lstm(changed("lstm.bias_hh_l1_reverse", 11, 1e12), args, -10.0, 5.0)
    with pytest.raises(QZ.QuantizationError, match=r"l0\.fwd\.ih, row 300"):
        QZ.quantize_lstm(changed("lstm.bias_ih_l0", 300, -1e12), args, -10.0, 5.0)
    with pytest.raises(QZ.QuantizationError, match=r"classifier, row 1"):
        QZ.quantize_lstm(changed("fc.1.bias", 1, 1e12), args, -10.0, 5.0)
    # the bounds are K_in 127 255 for the input projection, H 127 128 for the hidden one, nd H 127 128 for the classifier
    s_w = np.ones(512)
    for acc_max in (40 * 127 * 255, 128 * 127 * 128, 256 * 127 * 128):
        assert QZ.quantize_bias(np.full(512, float(2 ** 31 - 1 - acc_max)), 1.0, s_w, acc_max, "l0.fwd.hh", unit="row")[0] > 0
        with pytest.raises(QZ.QuantizationError, match=r"l0\.fwd\.hh, row 0"):
            QZ.quantize_bias(np.full(512, float(2 ** 31 - acc_max)), 1.0, s_w, acc_max, "l0.fwd.hh", unit="row")
    for value in (float("nan"), float("inf")):                                                # a non-finite weight
        with pytest.raises(QZ.QuantizationError, match=r"l0\.rev\.hh.*not finite"):
            QZ.quantize_lstm(changed("lstm.weight_hh_l0_reverse", (5, 5), value), args, -10.0, 5.0)
    bad = dict(state)                                                                         # a multiplier out of range
    bad["lstm.weight_ih_l0"] = state["lstm.weight_ih_l0"].copy()
    bad["lstm.weight_ih_l0"][2] *= 1e-30
    with pytest.raises(QZ.QuantizationError, match=r"l0\.fwd\.ih, row 2"):
        QZ.quantize_lstm(bad, args, -10.0, 5.0)
    with pytest.raises(QZ.QuantizationError, match="hidden_size 64"):                         # hidden size != 128
        QZ.quantize_lstm(state, dict(args, hidden_size=64), -10.0, 5.0)
    with pytest.raises(QZ.QuantizationError, match="num_layers"):
        QZ.quantize_lstm(state, dict(args, num_layers=9), -10.0, 5.0)
    with pytest.raises(QZ.QuantizationError, match="lstm.weight_ih_l0"):                      # another input size than the state's
        QZ.quantize_lstm(state, dict(args, input_size=24), -10.0, 5.0)
    with pytest.raises(QZ.QuantizationError, match="num_classes"):
        QZ.check_lstm_args(args, num_classes=65)
    with pytest.raises(QZ.QuantizationError, match="not finite"):
        QZ.quantize_lstm(state, args, -10.0, float("inf"))
    # the argument and entry checks are shared with the CRNN: every message still names this model
    for changes, nc, text in (({"hidden_size": 64}, 2, "the int8 LSTM implements hidden_size == 128, got hidden_size 64"),
                              ({"num_layers": 9}, 2, "the int8 LSTM takes 1..8 layers, got num_layers 9"),
                              ({"input_size": 0}, 2, "the int8 LSTM takes a positive input_size, got 0"),
                              ({}, 65, "the int8 LSTM takes 2..64 classes, got num_classes 65")):
        with pytest.raises(QZ.QuantizationError) as e:
            QZ.check_lstm_args(dict(args, **changes), num_classes=nc)
        assert str(e.value) == text
    assert QZ.check_lstm_args(args, num_classes=64) == (40, 2, 2)
    for changes, text in (({"hidden_size": 64}, ": hidden_size 128, 1..8 layers, a positive input_size"),
                          ({"num_layers": 9}, ": hidden_size 128, 1..8 layers, a positive input_size"),
                          ({"num_layers": 2.0}, ": integer input_size, hidden_size and num_layers, a boolean bidirectional")):
        with pytest.raises(BU.BundleError) as e:
            BU.check_lstm_entry({"lstm": dict(args, **changes)})
        assert str(e.value).startswith("the lstm entry {") and str(e.value).endswith(text)
    with pytest.raises(BU.BundleError, match=r"the lstm entry None is not \{input_size, hidden_size, num_layers, bidirectional\}"):
        BU.check_lstm_entry({})


# ------------------------------------------------------------------ the bundle file
def _malformed():
    def drop(a, h):
        del a["l1.rev.hh.sh"]

    def drop_table(a, h):
        del a["tab.tanh"]

    def shape(a, h):
        a["l0.fwd.ih.w"] = a["l0.fwd.ih.w"].T.copy()

    def padded(a, h):
        a["l0.fwd.ih.w"] = np.zeros((512, 64), np.int8)           # arrays are unpadded: (512, 40)

    def dtype(a, h):
        a["l1.fwd.hh.b"] = a["l1.fwd.hh.b"].astype(np.int64)

    def mult_low(a, h):
        a["l0.rev.ih.m"][3] = 2 ** 30 - 1

    def shift_zero(a, h):
        a["l1.fwd.hh.sh"][0] = 0

    def shift_high(a, h):
        a["l0.fwd.hh.sh"][511] = 63

    def weight_min(a, h):
        a["l1.rev.ih.w"][1, 1] = -128

    def table_dtype(a, h):
        a["tab.sigmoid"] = a["tab.sigmoid"].astype(np.int32)

    def table_order(a, h):
        a["tab.tanh"][100] = a["tab.tanh"][99] - 1

    def table_range(a, h):
        a["tab.sigmoid"][0] = -1

    def no_lstm(a, h):
        del h["lstm"]

    def hidden(a, h):
        h["lstm"] = dict(h["lstm"], hidden_size=64)

    def layers(a, h):
        h["lstm"] = dict(h["lstm"], num_layers=3)

    def directions(a, h):
        h["lstm"] = dict(h["lstm"], bidirectional=1)

    def feature_rows(a, h):
        h["feature_shape"] = [36, h["feature_shape"][1]]

    def classes(a, h):
        h["num_classes"] = 3

    def arch(a, h):
        h["architecture"] = "gru"

    def scale(a, h):
        a["fc.scale"][1] = np.inf
    return [drop, drop_table, shape, padded, dtype, mult_low, shift_zero, shift_high, weight_min, table_dtype, table_order,
            table_range, no_lstm, hidden, layers, directions, feature_rows, classes, arch, scale]


def test_malformed_bundles_are_invalid_not_errors(tmp_path):
    from wakeword_trainer_home_amd.export import validate_exported_model
    header, arrays, _, _, _ = LQ.case("odd")
    BU.check_bundle(header, arrays)
    path = BU.write_bundle(tmp_path / "good.npz", header, arrays)
    h2, a2 = BU.load_bundle(path)
    assert h2 == header and sorted(a2) == sorted(arrays)
    assert all(a2[k].dtype == arrays[k].dtype and np.array_equal(a2[k], arrays[k]) for k in arrays)
    good = validate_exported_model(path)
    assert good["valid"] is True and good["error"] is None and good["graph"] == len(header["layers"]) == 9
    assert good["inputs"] == [("input", [0, 1, 40, 7])] and good["outputs"] == [("output", [0, 2])]
    for breaker in _malformed():
        a, h = {k: v.copy() for k, v in arrays.items()}, dict(header)
        breaker(a, h)
        with pytest.raises(BU.BundleError):
            BU.check_bundle(h, a)
        res = validate_exported_model(BU.write_bundle(tmp_path / f"{breaker.__name__}.npz", h, a))
        assert res["valid"] is False and res["error"], breaker.__name__


def test_float_bundles_of_an_lstm_carry_the_lstm_entry():
    args = LQ.lstm_args(40, 2, True)
    state = LQ.random_state(args, 2, seed=1)
    for kind in ("fp32", "fp16"):
        h = BU.make_header(kind, "LSTMWakeword", 2, (1, 1, 40, 45), list(state), lstm=args)
        BU.check_bundle(h, BU.float_arrays(state, fp16=kind == "fp16"))
        assert BU.check_lstm_entry(h) == (40, 2, 2)
    assert BU.check_lstm_entry({"lstm": LQ.lstm_args(24, 1, False)}) == (24, 1, 1)
    for broken in ({}, {"lstm": dict(args, hidden_size=256)}, {"lstm": dict(args, num_layers=0)},
                   {"lstm": {"input_size": 40, "num_layers": 2}}):
        with pytest.raises(BU.BundleError):
            BU.check_lstm_entry(broken)


def test_int8_error_wording_keeps_its_words_and_names_the_lstm(tmp_path):
    from wakeword_trainer_home_amd.export.exporter import ExportConfig, ModelExporter
    exporter = ModelExporter.__new__(ModelExporter)
    exporter.calibration = [np.zeros((1, 1, 40, 38), np.float32)]
    with pytest.raises(QZ.QuantizationError, match="cnn_small only") as e:
        exporter._write_int8(tmp_path / "g.npz", {"architecture": "gru"}, {}, ExportConfig(output_path=tmp_path / "g.npz"))
    assert "'gru'" in str(e.value) and "ResNet18Wakeword" in str(e.value) and "LSTMWakeword" in str(e.value)
    exporter.calibration = None                                   # an LSTM without calibration data is refused as the others are
    with pytest.raises(QZ.QuantizationError, match="calibration"):
        exporter._write_int8(tmp_path / "l.npz", {"architecture": "LSTMWakeword"}, {}, ExportConfig(output_path=tmp_path / "l.npz"))


# ------------------------------------------------------------------ interface
def test_header_and_exports_agree_on_the_lq8_entry_points():
    import ctypes
    from wakeword_trainer_home_amd import _native
    header = (REPO / "include" / "wwhip.h").read_text()
    declared = set(re.findall(r"\b(ww_[a-z0-9_]+)\s*\(", header))
    assert declared == set(_native.EXPORTS)
    assert sorted(n for n in declared if n.startswith("ww_lq8_")) == LQ8_NAMES
    assert _native.ABI_VERSION == 17 and re.search(r"#define\s+WW_ABI_VERSION\s+17\b", header)
    assert (_native.LQ8_MAX_LAYERS, _native.LQ8_LAYER_NPTR, _native.LQ8_TAIL_NPTR) == (8, 8, 5)
    for name, value in (("MAX_LAYERS", 8), ("LAYER_NPTR", 8), ("TAIL_NPTR", 5)):
        assert re.search(rf"#define\s+WW_LQ8_{name}\s+{value}\b", header)
    assert ctypes.sizeof(_native.Lq8Io) == 4 * 6
    assert "ww_q8_lstm.hip" in (REPO / "wakeword_trainer_home_amd" / "csrc" / "Makefile").read_text()


def test_native_library_exports_the_lq8_entry_points_and_sizes_the_workspace():
    from wakeword_trainer_home_amd import _native
    lib = _native.load()
    assert lib.ww_abi_version() == 17 and all(hasattr(lib, n) for n in LQ8_NAMES)
    # the workspace the header describes: xq, then u, y, c_n per layer, then hcat, each rounded up to 256 bytes
    r256 = lambda n: (n + 255) // 256 * 256       # noqa: E731
    p64 = lambda c: (c + 63) // 64 * 64           # noqa: E731
    shapes = [(B, T, I, L, 2 if bi else 1) for B, T, I, L, bi, _, _ in LQ.CASES.values()] + [(512, 151, 40, 2, 2)]
    for B, T, I, L, nd in shapes:
        want = r256(B * T * p64(I)) + L * (r256(B * T * nd * 1024) + r256(B * T * nd * 128) + r256(B * nd * 256)) + r256(B * nd * 128)
        assert _native.lq8_lstm_workspace_bytes(B, T, I, L, nd) == want
    assert _native.lq8_lstm_workspace_bytes(0, 45, 40, 2, 2) == 0 and _native.lq8_lstm_workspace_bytes(1, 45, 40, 9, 2) == 0
    assert _native.lq8_lstm_workspace_bytes(1, 45, 40, 2, 3) == 0


def test_quantized_lstm_refuses_cpu_input_and_other_shapes():
    import torch
    import wakeword_trainer_home_amd.export as E
    from wakeword_trainer_home_amd._native import NativeError
    from wakeword_trainer_home_amd.export.runtime import device_lstm_layer
    assert "QuantizedLSTM" in E.__all__ and "calibrate_lstm" in E.__all__
    header, arrays, x, _, _ = LQ.case("odd")
    model = E.QuantizedLSTM(header, arrays)
    assert model.hip_backed and not model.training and not list(model.parameters())
    assert not any(t.requires_grad for t in model.buffers()) and model.num_classes == 2 and model.num_directions == 2
    w_ih, b_ih, _, _, w_hh, b_hh, _, _ = model.layer(0)
    assert w_ih.shape == (1024, 64) and w_hh.shape == (1024, 128) and model.layer(1)[0].shape == (1024, 256)
    assert not w_ih[:, 40:].any() and np.array_equal(w_ih[512:, :40].numpy(), arrays["l0.rev.ih.w"])
    z = int(arrays["input_zero"][0])
    eff = arrays["l0.fwd.ih.b"].astype(np.int64) - z * arrays["l0.fwd.ih.w"].astype(np.int64).sum(axis=1)
    assert z != 0 and np.array_equal(b_ih[:512].numpy(), eff.astype(np.int32)) and np.array_equal(b_hh[512:].numpy(), arrays["l0.rev.hh.b"])
    assert np.array_equal(device_lstm_layer(arrays, 1, 2, 0)[1][:512], arrays["l1.fwd.ih.b"])          # zero point 0: the bias itself
    with pytest.raises(NativeError, match="no CPU fallback"):
        model(torch.from_numpy(x))
    with pytest.raises(ValueError, match="features of shape"):
        model(torch.zeros(1, 1, 12, 6))
    with pytest.raises(ValueError, match="float32"):
        model(torch.zeros(1, 1, 40, 6, dtype=torch.float64))
    with pytest.raises(RuntimeError):
        model.train()
    with pytest.raises(ValueError):
        E.QuantizedLSTM(dict(header, kind="fp32"), arrays)
    from tests import q8_cases as Q
    with pytest.raises(ValueError):
        E.QuantizedLSTM(*Q.hard_bundle(13, 21))


# ------------------------------------------------------------------ quantisation error against the reference's float64 model
def test_quantisation_error_on_the_golden_fixture():
    """Interpreter on the exported bundle of the fixture vs. the float64 logits of the reference's own LSTMWakeword, over its 24
    structured feature maps.  Recorded for the restated law (tests/golden/q8_lstm_errors.json): max |dlogit| 0.00441, mean 0.00142,
    with logit margins from -0.12 to 0.0209 across the samples (span / loss 32).  The interpreter is held to twice the record."""
    z = np.load(GOLDEN / "g16_q8_lstm.npz")
    rec = json.loads((GOLDEN / "q8_lstm_errors.json").read_text())["LSTMWakeword"]
    x = z["x"].astype(np.float32)
    F, T = rec["feature_shape"]
    assert x.shape == (24, 1, F, T) and rec["samples"] == 24 and rec["calibration_samples"] == 12
    args = LQ.lstm_args(F, int(z["num_layers"]), bool(z["bidirectional"]))
    state = LQ.random_state(args, 2, seed=int(z["param_seed"]), head_gain=float(z["head_gain"]))
    for k, v in state.items():                                                    # the regenerated parameters are the fixture's
        idx = np.arange(v.size) if v.size <= 16 else np.linspace(0, v.size - 1, 16).astype(np.int64)
        assert np.array_equal(v.reshape(-1)[idx], z["psamp." + k]), k
    logits = z["logits"]
    assert logits.dtype == np.float64 and np.abs(LQ.float_forward(state, args, x) - logits).max() < 1e-9
    assert float(x[:12].min()) == float(z["x_min"]) and float(x[:12].max()) == float(z["x_max"])
    arrays, _ = QZ.quantize_lstm(state, args, float(z["x_min"]), float(z["x_max"]))
    q = R.run_int8(LQ.header_for(args, 2, T), arrays, x)["logits"]
    d = np.abs(q.astype(np.float64) - logits)
    margin = logits[:, 1] - logits[:, 0]
    print(f"MEASURED max |dlogit| {d.max():.4g} (recorded {rec['max_abs_dlogit']}), mean {d.mean():.4g}; "
          f"margin {margin.min():.4g} .. {margin.max():.4g}")
    assert margin.max() - margin.min() > 20 * rec["max_abs_dlogit"], "the margins vary too little to show a quantisation error"
    assert d.max() <= 2 * rec["max_abs_dlogit"]
