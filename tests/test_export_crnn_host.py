"""The CRNN half of the export package without a GPU: the NumPy interpreter and ``quantize_crnn`` against the restated law
(tests/q8_crnn_cases.py) bit for bit, the law's symmetries, the refusals, the bundle file, the ABI names, and the quantisation
error against the reference's float64 GRU on the committed fixture."""
import json
import re
from pathlib import Path

import numpy as np
import pytest

from tests import q8_crnn_cases as CQ
from wakeword_trainer_home_amd.export import bundle as BU
from wakeword_trainer_home_amd.export import quantize as QZ
from wakeword_trainer_home_amd.export import reference as R

REPO = Path(__file__).resolve().parent.parent
GOLDEN = Path(__file__).resolve().parent / "golden"
CQ8_NAMES = ["ww_cq8_crnn_fwd", "ww_cq8_crnn_workspace_bytes", "ww_cq8_fmean_fwd", "ww_cq8_gru_layer_fwd"]


# ------------------------------------------------------------------ the interpreter against the restatement
@pytest.mark.parametrize("name", list(CQ.CASES))
def test_interpreter_equals_restated_law_on_every_tensor(name):
    header, arrays, x, ref = CQ.case(name)
    BU.check_bundle(header, arrays)
    out = R.run_int8(header, arrays, x)
    want = CQ.stages(header["crnn"])
    assert list(out) == want == R.crnn_stages(header["crnn"])
    for stage in want:
        assert out[stage].dtype == ref[stage].dtype and out[stage].shape == ref[stage].shape, stage
        assert np.array_equal(out[stage], ref[stage]), stage
    B, F, T, _, bidir, nc = CQ.CASES[name]
    nd, Hp, Wp = 2 if bidir else 1, (F + 1) // 2, (T + 1) // 2
    assert out["xq"].shape == (B, F, T) and out["xq"].dtype == np.int8
    assert out["front.dw2"].shape == (B, Hp, Wp, 64) and out["seq"].shape == (B, Wp, 64) and out["seq"].dtype == np.int8
    assert out["l0.fwd.u"].shape == (B, Wp, 384) and out["l0.fwd.u"].dtype == np.int16
    assert out["l0.fwd.y"].shape == (B, Wp, 128) and out["l0.fwd.h"].shape == (B, 128) and out["l0.fwd.h"].dtype == np.int16
    assert out["hcat"].shape == (B, nd * 128) and out["logits"].shape == (B, nc) and out["logits"].dtype == np.float32
    assert all(np.array_equal(v, out[k]) for k, v in R.run_int8(header, arrays, x[:, 0]).items())      # the (B,F,T) form
    with pytest.raises(ValueError, match="features of shape"):
        R.run_int8(header, arrays, np.zeros((1, 1, F + 1, T), np.float32))
    longer = np.concatenate([x, x[..., ::-1]], axis=3)                                                  # any T
    assert np.array_equal(R.run_int8(header, arrays, longer)["logits"], CQ.r_forward(header["crnn"], arrays, longer)["logits"])


@pytest.mark.parametrize("name", list(CQ.STACK_CASES))
def test_stack_interpreter_equals_restated_law(name):
    args, arrays, _, ref, _ = CQ.stack_case(name)
    out, hcat = R.run_int8_gru_stack(arrays, ref["xq"], int(arrays["input_zero"][0]), args)
    assert list(out) == CQ.stack_stages(args) == R.gru_stack_stages(args)
    for stage in out:
        assert out[stage].dtype == ref[stage].dtype and np.array_equal(out[stage], ref[stage]), stage
    assert hcat.dtype == np.int8 and np.array_equal(hcat, ref["hcat"])


def test_every_clamp_of_the_gru_subsection_is_reached():
    reached = CQ.clamps_reached()
    assert set(reached) == set(CQ.CLAMPS)
    for clamp, names in reached.items():
        assert names, f"no case reaches the clamp {clamp}"
        assert "saturating" in names
    assert any(n != "saturating" for n in reached["q_h_127"])                      # the default-gain cases reach it too
    ref = CQ.stack_case("saturating")[3]
    assert ref["l0.fwd.u"].min() == -32768 and ref["l0.fwd.u"].max() == 32767
    assert max(ref[f"l{k}.{d}.y"].max() for k in (0, 1) for d in CQ.DIRS) == 127
    for name in CQ.CASES:                                                          # and the whole-model cases' own clamps
        r = CQ.case(name)[3]
        assert r["seq"].min() == -128 and r["seq"].max() == 127 and r["xq"].min() == -128 and r["xq"].max() == 127


def test_nan_and_infinite_inputs_follow_the_input_rule():
    header, arrays, x, _ = CQ.case("uni")
    x = x.copy()
    x[0, 0, 3, 1], x[1, 0, 0, 0], x[2, 0, 5, 2] = np.nan, np.inf, -np.inf
    out = R.run_int8(header, arrays, x)
    ref = CQ.r_forward(header["crnn"], arrays, x)
    assert out["xq"][0, 3, 1] == int(arrays["input_zero"][0]) and out["xq"][1, 0, 0] == 127 and out["xq"][2, 5, 2] == -128
    for stage in CQ.stages(header["crnn"]):
        assert np.array_equal(out[stage], ref[stage]), stage
    assert np.isfinite(out["logits"]).all()


def test_reverse_direction_is_the_forward_direction_on_the_flipped_sequence():
    """A stack whose two directions hold the same parameters: the reverse direction on a sequence equals the forward one on the
    sequence flipped in time.  (The SEQUENCE: the conv stack in front is not symmetric in time.)"""
    args, arrays, _, ref, _ = CQ.stack_case("odd")
    a = dict(arrays)
    for key in list(a):
        if ".rev." in key:
            a[key] = a[key.replace(".rev.", ".fwd.")]
    one, z = dict(args, num_layers=1), int(arrays["input_zero"][0])
    (out, hcat), (flipped, hcat_f) = R.run_int8_gru_stack(a, ref["xq"], z, one), R.run_int8_gru_stack(a, ref["xq"][:, ::-1], z, one)
    assert np.array_equal(out["l0.rev.u"], flipped["l0.fwd.u"][:, ::-1])
    assert np.array_equal(out["l0.rev.y"], flipped["l0.fwd.y"][:, ::-1]) and np.array_equal(out["l0.rev.h"], flipped["l0.fwd.h"])
    assert np.array_equal(hcat[:, 128:], hcat_f[:, :128])
    assert not np.array_equal(out["l0.rev.y"], out["l0.fwd.y"])


def test_rolling_the_batch_rolls_every_output():
    header, arrays, x, ref = CQ.case("odd")
    out = R.run_int8(header, arrays, np.roll(x, 5, axis=0))
    for stage in CQ.stages(header["crnn"]):
        assert np.array_equal(out[stage], np.roll(ref[stage], 5, axis=0)), stage


# ------------------------------------------------------------------ the derivation against the restatement
def _ranges(state, F, T, seed=4):
    return CQ.float_front(state, CQ.structured_features(3, F, T, seed=seed))[1]


@pytest.mark.parametrize("name", ["odd", "uni", "classes"])
def test_export_derivation_equals_restated_law(name):
    _, F, T, layers, bidir, nc = CQ.CASES[name]
    args = CQ.crnn_args(layers, bidir)
    state = CQ.random_state(args, nc, seed=5)
    ranges = _ranges(state, F, T)
    arrays, scales = QZ.quantize_crnn(state, args, F, ranges)
    want = CQ.r_quantize_model(state, args, F, ranges)
    assert sorted(arrays) == sorted(want)
    for key in want:
        assert arrays[key].dtype == want[key].dtype and arrays[key].shape == want[key].shape, key
        assert np.array_equal(arrays[key], want[key]), key
    nd = 2 if bidir else 1
    assert arrays["front.stem.w"].shape == (64, 9) and arrays["front.pw3.w"].shape == (64, 64) and arrays["fmean.m"].shape == (1,)
    assert arrays["l0.fwd.ih.w"].shape == (384, 64) and arrays["l0.fwd.ih.w"].dtype == np.int8
    assert arrays["l0.fwd.hh.w"].shape == (384, 128) and arrays["fc.w"].shape == (nc, nd * 128)
    assert arrays["l0.fwd.ih.b"].dtype == arrays["l0.fwd.hh.m"].dtype == arrays["l0.fwd.hh.sh"].dtype == np.int32
    assert arrays["tab.sigmoid"].dtype == arrays["tab.tanh"].dtype == np.int16 and arrays["tab.tanh"].shape == (4096,)
    assert arrays["fc.scale"].dtype == np.float32 and ("l0.rev.ih.w" in arrays) == bidir
    if layers > 1:
        assert arrays["l1.fwd.ih.w"].shape == (384, nd * 128)
    assert not arrays["l0.fwd.hh.w"][7].any() and arrays["l0.fwd.hh.m"][7] == 2 ** 30 and arrays["l0.fwd.hh.sh"][7] == 29  # s_w = 1: r = 2
    assert scales["hidden"] == 2.0 ** -7 and scales["input"] == float(arrays["input_scale"][0])
    assert scales["fmean"] == max(ranges["f_max"], 255 * 2.0 ** -20) / 255
    CQ.check_tables(arrays)
    BU.check_bundle(CQ.header_for(args, F, T, nc), arrays)


def test_a_dead_front_end_takes_the_floor():
    args = CQ.crnn_args(1, False)
    state = CQ.random_state(args, 2, seed=5)
    ranges = dict(_ranges(state, 13, 21), f_max=0.0)
    arrays, scales = QZ.quantize_crnn(state, args, 13, ranges)
    assert scales["fmean"] == 2.0 ** -20
    assert np.array_equal(arrays["fmean.m"], CQ.r_quantize_model(state, args, 13, ranges)["fmean.m"])


def test_export_refuses_what_the_law_cannot_hold():
    args = CQ.crnn_args(2, True)
    state = CQ.random_state(args, 2, seed=4)
    ranges = _ranges(state, 13, 21)
    QZ.quantize_crnn(state, args, 13, ranges)

    def changed(key, index, value):
        bad = dict(state)
        bad[key] = state[key].copy()
        bad[key][index] = value
        return bad
    with pytest.raises(QZ.QuantizationError, match=r"l1\.rev\.hh, row 11"):                 # a bias overflow names layer and row
        QZ.quantize_crnn(changed("rnn.gru.bias_hh_l1_reverse", 11, 1e12), args, 13, ranges)
    with pytest.raises(QZ.QuantizationError, match=r"l0\.fwd\.ih, row 300"):
        QZ.quantize_crnn(changed("rnn.gru.bias_ih_l0", 300, -1e12), args, 13, ranges)
    with pytest.raises(QZ.QuantizationError, match=r"classifier, row 1"):
        QZ.quantize_crnn(changed("rnn.fc.1.bias", 1, 1e12), args, 13, ranges)
    with pytest.raises(QZ.QuantizationError, match=r"front\.dw1, channel 3"):
        QZ.quantize_crnn(changed("front.blocks.1.dw_bn.bias", 3, 1e12), args, 13, ranges)
    # the bounds are K_in 127 255 for the input projection, H 127 128 for the hidden one
    s_w = np.ones(384)
    for acc_max in (64 * 127 * 255, 128 * 127 * 128, 256 * 127 * 255):
        assert QZ.quantize_bias(np.full(384, float(2 ** 31 - 1 - acc_max)), 1.0, s_w, acc_max, "l0.fwd.hh", unit="row")[0] > 0
        with pytest.raises(QZ.QuantizationError, match=r"l0\.fwd\.hh, row 0"):
            QZ.quantize_bias(np.full(384, float(2 ** 31 - acc_max)), 1.0, s_w, acc_max, "l0.fwd.hh", unit="row")
    for value in (float("nan"), float("inf")):                                                # a non-finite weight
        with pytest.raises(QZ.QuantizationError, match=r"l0\.rev\.hh.*not finite"):
            QZ.quantize_crnn(changed("rnn.gru.weight_hh_l0_reverse", (5, 5), value), args, 13, ranges)
        with pytest.raises(QZ.QuantizationError, match=r"front\.pw2.*not finite"):
            QZ.quantize_crnn(changed("front.blocks.2.pw.weight", (5, 5, 0, 0), value), args, 13, ranges)
    with pytest.raises(QZ.QuantizationError, match="hidden_size 64"):                         # hidden size != 128
        QZ.quantize_crnn(state, dict(args, hidden_size=64), 13, ranges)
    for layers in (0, 9):
        with pytest.raises(QZ.QuantizationError, match="num_layers"):
            QZ.quantize_crnn(state, dict(args, num_layers=layers), 13, ranges)
    for nc in (1, 65):
        with pytest.raises(QZ.QuantizationError, match="num_classes"):
            QZ.check_crnn_args(args, num_classes=nc)
        with pytest.raises(QZ.QuantizationError, match="num_classes"):
            QZ.quantize_crnn(CQ.random_state(args, nc, seed=4), args, 13, ranges)
    with pytest.raises(QZ.QuantizationError, match="rnn.gru.weight_ih_l1"):                   # another direction count than the state's
        QZ.quantize_crnn(state, dict(args, bidirectional=False), 13, ranges)
    with pytest.raises(QZ.QuantizationError, match="not finite"):
        QZ.quantize_crnn(state, args, 13, dict(ranges, x_max=float("inf")))
    with pytest.raises(QZ.QuantizationError, match="not finite"):
        QZ.quantize_crnn(state, args, 13, dict(ranges, f_max=float("nan")))
    with pytest.raises(QZ.QuantizationError, match="calibrated maxima"):
        QZ.quantize_crnn(state, args, 13, dict(ranges, a_max=ranges["a_max"][:8]))
    # the argument and entry checks are shared with the LSTM: every message still names this model, and no input_size is asked for
    for changes, nc, text in (({"hidden_size": 64}, 2, "the int8 CRNN implements hidden_size == 128, got hidden_size 64"),
                              ({"num_layers": 9}, 2, "the int8 CRNN takes 1..8 layers, got num_layers 9"),
                              ({}, 65, "the int8 CRNN takes 2..64 classes, got num_classes 65")):
        with pytest.raises(QZ.QuantizationError) as e:
            QZ.check_crnn_args(dict(args, **changes), num_classes=nc)
        assert str(e.value) == text
    assert QZ.check_crnn_args(dict(args, input_size=0), num_classes=64) == (2, 2)
    for changes, text in (({"hidden_size": 64}, ": hidden_size 128, 1..8 layers"), ({"num_layers": 9}, ": hidden_size 128, 1..8 layers"),
                          ({"num_layers": 2.0}, ": integer hidden_size and num_layers, a boolean bidirectional")):
        with pytest.raises(BU.BundleError) as e:
            BU.check_crnn_entry({"crnn": dict(args, **changes)})
        assert str(e.value).startswith("the crnn entry {") and str(e.value).endswith(text)
    with pytest.raises(BU.BundleError, match=r"the crnn entry None is not \{hidden_size, num_layers, bidirectional\}"):
        BU.check_crnn_entry({})


# ------------------------------------------------------------------ the bundle file
def _malformed():
    def drop(a, h):
        del a["l1.rev.hh.sh"]

    def drop_table(a, h):
        del a["tab.tanh"]

    def drop_fmean(a, h):
        del a["fmean.m"]

    def drop_conv(a, h):
        del a["front.dw3.b"]

    def shape(a, h):
        a["l0.fwd.ih.w"] = a["l0.fwd.ih.w"].T.copy()

    def lstm_rows(a, h):
        a["l0.fwd.hh.w"] = np.zeros((512, 128), np.int8)          # a GRU direction has 384 gate rows

    def conv_shape(a, h):
        a["front.stem.w"] = a["front.stem.w"].T.copy()

    def dtype(a, h):
        a["l1.fwd.hh.b"] = a["l1.fwd.hh.b"].astype(np.int64)

    def mult_low(a, h):
        a["l0.rev.ih.m"][3] = 2 ** 30 - 1

    def fmean_mult(a, h):
        a["fmean.m"][0] = 5

    def fmean_shift(a, h):
        a["fmean.sh"][0] = 63

    def shift_zero(a, h):
        a["l1.fwd.hh.sh"][0] = 0

    def shift_high(a, h):
        a["l0.fwd.hh.sh"][383] = 63

    def weight_min(a, h):
        a["l1.rev.ih.w"][1, 1] = -128

    def conv_weight_min(a, h):
        a["front.pw0.w"][1, 1] = -128

    def table_dtype(a, h):
        a["tab.sigmoid"] = a["tab.sigmoid"].astype(np.int32)

    def table_order(a, h):
        a["tab.tanh"][100] = a["tab.tanh"][99] - 1

    def table_range(a, h):
        a["tab.sigmoid"][0] = -1

    def no_entry(a, h):
        del h["crnn"]

    def hidden(a, h):
        h["crnn"] = dict(h["crnn"], hidden_size=64)

    def layers(a, h):
        h["crnn"] = dict(h["crnn"], num_layers=3)

    def no_layers(a, h):
        h["crnn"] = dict(h["crnn"], num_layers=0)

    def directions(a, h):
        h["crnn"] = dict(h["crnn"], bidirectional=1)

    def classes(a, h):
        h["num_classes"] = 3

    def arch(a, h):
        h["architecture"] = "gru"

    def scale(a, h):
        a["fc.scale"][1] = np.inf
    return [drop, drop_table, drop_fmean, drop_conv, shape, lstm_rows, conv_shape, dtype, mult_low, fmean_mult, fmean_shift, shift_zero,
            shift_high, weight_min, conv_weight_min, table_dtype, table_order, table_range, no_entry, hidden, layers, no_layers,
            directions, classes, arch, scale]


def test_malformed_bundles_are_invalid_not_errors(tmp_path):
    from wakeword_trainer_home_amd.export import validate_exported_model
    header, arrays, _, _ = CQ.case("odd")
    BU.check_bundle(header, arrays)
    path = BU.write_bundle(tmp_path / "good.npz", header, arrays)
    h2, a2 = BU.load_bundle(path)
    assert h2 == header and sorted(a2) == sorted(arrays)
    assert all(a2[k].dtype == arrays[k].dtype and np.array_equal(a2[k], arrays[k]) for k in arrays)
    good = validate_exported_model(path)
    assert good["valid"] is True and good["error"] is None and good["graph"] == len(header["layers"]) == 9 + 8 + 2
    assert good["inputs"] == [("input", [0, 1, 13, 21])] and good["outputs"] == [("output", [0, 2])]
    for breaker in _malformed():
        a, h = {k: v.copy() for k, v in arrays.items()}, dict(header)
        breaker(a, h)
        with pytest.raises(BU.BundleError):
            BU.check_bundle(h, a)
        res = validate_exported_model(BU.write_bundle(tmp_path / f"{breaker.__name__}.npz", h, a))
        assert res["valid"] is False and res["error"], breaker.__name__


def test_float_bundles_of_a_crnn_carry_and_honour_the_crnn_entry(tmp_path, monkeypatch):
    args = CQ.crnn_args(1, False)
    state = CQ.random_state(args, 3, seed=1)
    for kind in ("fp32", "fp16"):
        h = BU.make_header(kind, "crnn", 3, (1, 1, 40, 45), list(state), crnn=args)
        BU.check_bundle(h, BU.float_arrays(state, fp16=kind == "fp16"))
        assert BU.check_crnn_entry(h) == (1, 1)
    assert BU.check_crnn_entry({"crnn": CQ.crnn_args(8, True)}) == (8, 2)
    for broken in ({}, {"crnn": dict(args, hidden_size=256)}, {"crnn": dict(args, num_layers=0)}, {"crnn": dict(args, num_layers=9)},
                   {"crnn": {"num_layers": 2}}, {"crnn": dict(args, num_layers=True)}):
        with pytest.raises(BU.BundleError):
            BU.check_crnn_entry(broken)
    # the loader builds the model the entry describes, not the factory's default (2 layers, bidirectional)
    import wakeword_trainer_home_amd.models as M
    from wakeword_trainer_home_amd.export import exporter as EX
    built = {}

    class Stop(Exception):
        pass

    def fake_create_model(**kw):
        built.update(kw)
        raise Stop
    monkeypatch.setattr(M, "create_model", fake_create_model)
    path = BU.write_bundle(tmp_path / "c.npz", BU.make_header("fp32", "crnn", 3, (1, 1, 40, 45), list(state), crnn=args),
                           BU.float_arrays(state, fp16=False))
    with pytest.raises(Stop):
        EX.load_exported_model(path, "cpu")
    assert built == {"architecture": "crnn", "num_classes": 3, "pretrained": False, "hidden_size": 128, "num_layers": 1,
                     "bidirectional": False}


def test_int8_error_wording_keeps_its_words_and_names_the_crnn(tmp_path):
    from wakeword_trainer_home_amd.export.exporter import ExportConfig, ModelExporter
    exporter = ModelExporter.__new__(ModelExporter)
    exporter.calibration = [np.zeros((1, 1, 40, 38), np.float32)]
    with pytest.raises(QZ.QuantizationError, match="cnn_small only") as e:
        exporter._write_int8(tmp_path / "g.npz", {"architecture": "gru"}, {}, ExportConfig(output_path=tmp_path / "g.npz"))
    text = str(e.value)
    assert "'gru'" in text and "ResNet18Wakeword" in text and "LSTMWakeword" in text and "TCNWakeword" in text
    assert "crnn" in text.split("not 'gru'")[0]                   # named among the covered
    exporter.calibration = None                                   # a CRNN without calibration data is refused as the others are
    with pytest.raises(QZ.QuantizationError, match="calibration"):
        exporter._write_int8(tmp_path / "c.npz", {"architecture": "crnn"}, {}, ExportConfig(output_path=tmp_path / "c.npz"))
    with pytest.raises(BU.BundleError, match="int8 form"):
        BU.check_bundle(dict(CQ.header_for(CQ.crnn_args(1, True), 13, 21), architecture="gru"), {})


# ------------------------------------------------------------------ interface
def test_header_and_exports_agree_on_the_cq8_entry_points():
    import ctypes
    from wakeword_trainer_home_amd import _native
    header = (REPO / "include" / "wwhip.h").read_text()
    declared = set(re.findall(r"\b(ww_[a-z0-9_]+)\s*\(", header))
    assert declared == set(_native.EXPORTS)
    assert sorted(n for n in declared if n.startswith("ww_cq8_")) == CQ8_NAMES
    assert _native.ABI_VERSION == 17 and re.search(r"#define\s+WW_ABI_VERSION\s+17\b", header)
    consts = (("MAX_LAYERS", 8), ("CONV_NPTR", 36), ("LAYER_NPTR", 8), ("TAIL_NPTR", 5), ("NACT", 5))
    for name, value in consts:
        assert re.search(rf"#define\s+WW_CQ8_{name}\s+{value}\b", header) and getattr(_native, "CQ8_" + name) == value
    assert ctypes.sizeof(_native.Cq8Io) == 4 * 7
    assert "ww_q8_crnn.hip" in (REPO / "wakeword_trainer_home_amd" / "csrc" / "Makefile").read_text()


def test_native_library_exports_the_cq8_entry_points_and_sizes_the_workspace():
    from wakeword_trainer_home_amd import _native
    lib = _native.load()
    assert lib.ww_abi_version() == 17 and all(hasattr(lib, n) for n in CQ8_NAMES)
    # the workspace the header describes: xq, stem and pw0..pw3, seq, then u, y, h_n per layer, then hcat, each rounded up to 256
    r256 = lambda n: (n + 255) // 256 * 256       # noqa: E731
    shapes = [(B, F, T, L, 2 if bi else 1) for B, F, T, L, bi, _ in CQ.CASES.values()] + [(512, 40, 151, 2, 2)]
    for B, F, T, L, nd in shapes:
        Hp, Wp = (F + 1) // 2, (T + 1) // 2
        want = (r256(B * F * T) + 5 * r256(B * Hp * Wp * 64) + r256(B * Wp * 64) +
                L * (r256(B * Wp * nd * 768) + r256(B * Wp * nd * 128) + r256(B * nd * 256)) + r256(B * nd * 128))
        assert _native.cq8_crnn_workspace_bytes(B, F, T, L, nd) == want
    assert _native.cq8_crnn_workspace_bytes(0, 40, 45, 2, 2) == 0 and _native.cq8_crnn_workspace_bytes(1, 40, 45, 9, 2) == 0
    assert _native.cq8_crnn_workspace_bytes(1, 40, 45, 2, 3) == 0 and _native.cq8_crnn_workspace_bytes(1, 40, 0, 2, 2) == 0


def test_quantized_crnn_refuses_cpu_input_and_another_f():
    import torch
    import wakeword_trainer_home_amd.export as E
    from wakeword_trainer_home_amd._native import NativeError
    from wakeword_trainer_home_amd.export.runtime import device_gru_layer
    assert "QuantizedCRNN" in E.__all__ and "calibrate_crnn" in E.__all__
    header, arrays, x, _ = CQ.case("odd")
    model = E.QuantizedCRNN(header, arrays)
    assert model.hip_backed and not model.training and not list(model.parameters())
    assert not any(t.requires_grad for t in model.buffers()) and model.num_classes == 2 and model.num_directions == 2
    w_ih, b_ih, _, _, w_hh, b_hh, _, _ = model.layer(0)
    assert w_ih.shape == (768, 64) and w_hh.shape == (768, 128) and model.layer(1)[0].shape == (768, 256)
    assert np.array_equal(w_ih[384:].numpy(), arrays["l0.rev.ih.w"])
    eff = arrays["l0.fwd.ih.b"].astype(np.int64) + 128 * arrays["l0.fwd.ih.w"].astype(np.int64).sum(axis=1)      # z_in = -128
    assert np.array_equal(b_ih[:384].numpy(), eff.astype(np.int32)) and np.array_equal(b_hh[384:].numpy(), arrays["l0.rev.hh.b"])
    assert np.array_equal(device_gru_layer(arrays, 1, 2, 0)[1][:384], arrays["l1.fwd.ih.b"])          # zero point 0: the bias itself
    assert model.conv("stem")[0].shape == (9, 64) and model.conv("pw3")[0].shape == (64, 64)
    with pytest.raises(NativeError, match="no CPU fallback"):
        model(torch.from_numpy(x))
    with pytest.raises(ValueError, match="features of shape"):
        model(torch.zeros(1, 1, 12, 6))
    with pytest.raises(ValueError, match="float32"):
        model(torch.zeros(1, 1, 13, 6, dtype=torch.float64))
    with pytest.raises(RuntimeError):
        model.train()
    with pytest.raises(ValueError):
        E.QuantizedCRNN(dict(header, kind="fp32"), arrays)
    from tests import q8_cases as Q
    with pytest.raises(ValueError):
        E.QuantizedCRNN(*Q.hard_bundle(13, 21))


# ------------------------------------------------------------------ quantisation error against the reference's float64 GRU
def test_quantisation_error_on_the_golden_fixture():
    """Interpreter on the exported bundle of the fixture vs. the float64 logits of the reference's own GRUWakeword(input_size=64) run
    on the float64 sequence of the restated float front end, over its 24 structured feature maps.  The record is what the restated
    law loses (tests/golden/q8_crnn_errors.json); the interpreter is held to twice the recorded maximum, and the margins must span
    more than 20 times it."""
    z = np.load(GOLDEN / "g17_q8_crnn.npz")
    rec = json.loads((GOLDEN / "q8_crnn_errors.json").read_text())["CRNNWakeword"]
    x = z["x"].astype(np.float32)
    F, T = rec["feature_shape"]
    assert x.shape == (24, 1, F, T) and rec["samples"] == 24 and rec["calibration_samples"] == 12
    args = CQ.crnn_args(int(z["num_layers"]), bool(z["bidirectional"]))
    state = CQ.random_state(args, 2, seed=int(z["gru_seed"]), gain=float(z["gain"]), front_seed=int(z["front_seed"]))
    for k, v in state.items():                                                    # the regenerated parameters are the fixture's
        idx = np.arange(v.size) if v.size <= 16 else np.linspace(0, v.size - 1, 16).astype(np.int64)
        assert np.array_equal(v.reshape(-1)[idx], z["psamp." + k]), k
    logits = z["logits"]
    assert logits.dtype == np.float64 and np.abs(CQ.float_forward(state, args, x) - logits).max() < 1e-9
    ranges = CQ.float_front(state, x[:12])[1]
    assert ranges["x_min"] == float(z["x_min"]) and ranges["x_max"] == float(z["x_max"])
    assert np.array_equal(np.array(ranges["a_max"] + [ranges["f_max"]]), z["maxima"])
    arrays, _ = QZ.quantize_crnn(state, args, F, ranges)
    q = R.run_int8(CQ.header_for(args, F, T), arrays, x)["logits"]
    d = np.abs(q.astype(np.float64) - logits)
    margin = logits[:, 1] - logits[:, 0]
    print(f"MEASURED max |dlogit| {d.max():.4g} (recorded {rec['max_abs_dlogit']}), mean {d.mean():.4g}; "
          f"margin {margin.min():.4g} .. {margin.max():.4g}")
    assert margin.max() - margin.min() > 20 * rec["max_abs_dlogit"], "the margins vary too little to show a quantisation error"
    assert d.max() <= 2 * rec["max_abs_dlogit"]
