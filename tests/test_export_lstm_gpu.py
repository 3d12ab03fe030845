"""The int8 LSTM kernels and the LSTM half of the export package on the GPU.  Integer arithmetic is exact, so every comparison with
the restated law (tests/q8_lstm_cases.py) is bit for bit: no tolerance anywhere in this file but the fp16 bundle's weight
rounding."""
import os

import numpy as np
import pytest
import torch

from tests import q8_crnn_cases as CQ
from tests import q8_lstm_cases as LQ

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TRIPS_BATCH = 40        # ``odd`` at B = 40: 280 rows are five 64-row groups x 16 gate-row tiles = 80 projection items, and three
#                         16-row batch groups of the recurrence: a capped launch walks them in several trips


@pytest.fixture(scope="module")
def cases():
    """name -> (header, arrays, x, restated tensors, QuantizedLSTM on the device); computed once, never modified."""
    from wakeword_trainer_home_amd.export import QuantizedLSTM
    out = {}
    for name in list(LQ.CASES) + ["trips"]:
        case = LQ.case("odd", batch=TRIPS_BATCH) if name == "trips" else LQ.case(name)
        out[name] = case[:4] + (QuantizedLSTM(case[0], case[1]).to(DEV),)
    return out


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _pad(q, fill):
    """(B,T,C) int8 -> the device layout (B,T,Cp), the pad channels holding the tensor's zero point."""
    B, T, C = q.shape
    out = np.full((B, T, (C + 63) // 64 * 64), fill, np.int8)
    out[..., :C] = q
    return out


def _same(got, want, what):
    got = got.cpu().numpy()
    assert got.dtype == want.dtype and got.shape == want.shape, f"{what}: {got.dtype} {got.shape} vs {want.dtype} {want.shape}"
    bad = np.flatnonzero(got.reshape(-1) != want.reshape(-1))
    assert bad.size == 0, f"{what}: {bad.size} of {got.size} differ, first at {np.unravel_index(bad[0], got.shape)}"


def _stacked(ref, args, k, what):
    """The restated law's per-direction tensors of layer ``k`` as the device stacks them: forward channels first."""
    return np.concatenate([ref[f"l{k}.{d}.{what}"] for d in LQ.dirs(args)], axis=-1)


@pytest.fixture
def grid_cap():
    from wakeword_trainer_home_amd import _native as nat
    yield lambda n: nat.set_grid_cap(DEV, n)
    nat.set_grid_cap(DEV, 0)


@pytest.fixture
def global_tables():
    """The recurrence launches that follow read the gate tables through the caches instead of LDS."""
    old = os.environ.get("WW_LQ8_TABLES")
    os.environ["WW_LQ8_TABLES"] = "global"
    yield
    if old is None:
        del os.environ["WW_LQ8_TABLES"]
    else:
        os.environ["WW_LQ8_TABLES"] = old


def _kernels(case):
    """Every kernel alone, each fed the restated law's own input tensor in the device layout."""
    from wakeword_trainer_home_amd import _native as nat
    header, arrays, x, ref, model = case
    args = header["lstm"]
    z_x = int(arrays["input_zero"][0])
    _same(nat.tq8_quantize_bt(_dev(x[:, 0]), arrays["input_scale"][0], z_x), _pad(ref["xq"], z_x), "quantize")
    a_in = _pad(ref["xq"], z_x)
    for k in range(args["num_layers"]):
        w_ih, b_ih, m_i, sh_i, w_hh, b_hh, m_h, sh_h = model.layer(k)
        _same(nat.lq8_proj_fwd(_dev(a_in), w_ih, b_ih, m_i, sh_i), _stacked(ref, args, k, "u"), f"l{k} projection")
        y, c_n = nat.lq8_lstm_layer_fwd(_dev(_stacked(ref, args, k, "u")), w_hh, b_hh, m_h, sh_h, model.tab_sigmoid, model.tab_tanh)
        _same(y, _stacked(ref, args, k, "y"), f"l{k} recurrence, y")
        _same(c_n, _stacked(ref, args, k, "c"), f"l{k} recurrence, c")
        a_in = _stacked(ref, args, k, "y")
    hcat, logits = nat.lq8_head_fwd(_dev(a_in), model.fc_w, model.fc_b, model.fc_scale)
    _same(hcat, ref["hcat"], "hcat")
    _same(logits, ref["logits"], "logits")


def _whole(case, sequences=False):
    """One forward; every stage tensor read back from the workspace, pad channels included."""
    from wakeword_trainer_home_amd import _native as nat
    header, arrays, x, ref, model = case
    args = header["lstm"]
    B, F, T = x.shape[0], x.shape[2], x.shape[3]
    model._ws.clear()                                            # a fresh workspace: what is read below was written by this call
    xd = _dev(x)
    with torch.no_grad():
        logits = model(xd[:, 0].transpose(1, 2) if sequences else xd)
    _same(logits, ref["logits"], "logits")
    views = nat.lq8_workspace_views(model.workspace(B, T), B, T, F, args["num_layers"], len(LQ.dirs(args)))
    _same(views["xq"], _pad(ref["xq"], int(arrays["input_zero"][0])), "xq")
    for k in range(args["num_layers"]):
        for what in ("u", "y", "c"):
            _same(views[f"l{k}.{what}"], _stacked(ref, args, k, what), f"l{k}.{what}")
    _same(views["hcat"], ref["hcat"], "hcat")
    return views


@pytest.mark.parametrize("name", list(LQ.CASES))
def test_each_kernel_alone(cases, name):
    _kernels(cases[name])


@pytest.mark.parametrize("name", list(LQ.CASES))
def test_whole_model_every_tensor_through_both_input_forms(cases, name):
    _whole(cases[name])
    _whole(cases[name], sequences=True)
    _, _, x, ref, model = cases[name]
    assert ref["logits"].shape == (x.shape[0], LQ.CASES[name][5])
    with torch.no_grad():                                        # a batch slice (another base address) takes the same path
        _same(model(_dev(x)[1:]), ref["logits"][1:], "batch slice")


def test_kernels_make_several_trips_under_a_grid_cap(cases, grid_cap):
    """One workgroup walks everything: ``trips`` is 80 projection items in layer 0 and in layer 1 (20 trips of four waves), three
    batch groups per direction of the recurrence, 40 samples of the head; ``odd`` has a last batch group of 13 live rows."""
    for cap in (1, 3):
        grid_cap(cap)
        for name in ("trips", "odd"):
            _kernels(cases[name])
            _whole(cases[name])


def test_global_tables_form_gives_the_same_bits(cases, grid_cap, global_tables):
    for name in LQ.CASES:
        _kernels(cases[name])
    _whole(cases["saturating"])
    grid_cap(1)
    _whole(cases["trips"])


def _gru_layer0(args, arrays):
    """(w_hh, bias, mult, shift, tab_sigmoid, tab_tanh) of layer 0 of a GRU stack case on the device, as ``cq8_gru_layer_fwd`` reads
    them."""
    from wakeword_trainer_home_amd.export.runtime import device_gru_layer
    layer = device_gru_layer(arrays, 0, len(CQ.dirs(args)), int(arrays["input_zero"][0]))
    return tuple(_dev(t) for t in layer[4:] + (arrays["tab.sigmoid"], arrays["tab.tanh"]))


@pytest.mark.parametrize("cell", ["lstm", "gru"])
def test_recurrence_frame_two_trips_one_live_row_one_direction(cases, grid_cap, cell):
    """The edges of the frame both cells share that no other case meets: ``uni`` (one direction, one layer, I = 24, T = 4) at 17
    batch rows under a grid cap of 1 is a launch at gridDim.y = 1 whose one workgroup makes two trips, the second with a single
    live row.  (T = 1 on this shape would need a case builder that takes T; ``tiny`` is T = 1.)"""
    from wakeword_trainer_home_amd import _native as nat
    if cell == "lstm":
        ref, model = LQ.case("uni", batch=17)[3], cases["uni"][4]         # the bundle does not depend on the batch size
        fwd, state = nat.lq8_lstm_layer_fwd, "c"
        params = model.layer(0)[4:] + (model.tab_sigmoid, model.tab_tanh)
    else:
        args, arrays, _, ref = CQ.stack_case("uni", batch=17)[:4]
        fwd, state, params = nat.cq8_gru_layer_fwd, "h", _gru_layer0(args, arrays)
    assert ref["l0.fwd.u"].shape[:2] == (17, 4) and "l0.rev.u" not in ref
    grid_cap(1)
    y, s_n = fwd(_dev(ref["l0.fwd.u"]), *params)
    _same(y, ref["l0.fwd.y"], f"{cell} recurrence, y")
    _same(s_n, ref[f"l0.fwd.{state}"], f"{cell} recurrence, final state")


def test_the_gru_ignores_the_lstm_table_switch(cases, global_tables):
    """WW_LQ8_TABLES=global is the LSTM's switch alone: under it the GRU recurrence gives the restated law's bits, and the LSTM
    recurrence launched right after it gives its own in both table forms."""
    from wakeword_trainer_home_amd import _native as nat
    args, arrays, _, ref = CQ.stack_case("odd")[:4]
    y, h_n = nat.cq8_gru_layer_fwd(_dev(_stacked(ref, args, 0, "u")), *_gru_layer0(args, arrays))
    _same(y, _stacked(ref, args, 0, "y"), "GRU recurrence, y")
    _same(h_n, _stacked(ref, args, 0, "h"), "GRU recurrence, h_n")
    header, _, _, ref, model = cases["odd"]
    got = {}
    for tables in ("global", "lds"):
        os.environ["WW_LQ8_TABLES"] = tables                     # (the fixture puts the old value back)
        got[tables] = nat.lq8_lstm_layer_fwd(_dev(_stacked(ref, header["lstm"], 0, "u")), *model.layer(0)[4:], model.tab_sigmoid,
                                             model.tab_tanh)
        _same(got[tables][0], _stacked(ref, header["lstm"], 0, "y"), f"LSTM recurrence, tables {tables}, y")
        _same(got[tables][1], _stacked(ref, header["lstm"], 0, "c"), f"LSTM recurrence, tables {tables}, c")
    assert all(torch.equal(a, b) for a, b in zip(got["global"], got["lds"]))


def test_nan_and_infinite_inputs_on_the_device(cases):
    from wakeword_trainer_home_amd import _native as nat
    header, arrays, x, _, model = cases["uni"]
    x = x.copy()
    x[0, 0, 3, 1], x[1, 0, 0, 0], x[2, 0, 5, 2] = np.nan, np.inf, -np.inf
    ref = LQ.r_forward(header["lstm"], arrays, x)
    z_x = int(arrays["input_zero"][0])
    assert ref["xq"][0, 1, 3] == z_x and ref["xq"][1, 0, 0] == 127 and ref["xq"][2, 2, 5] == -128
    model._ws.clear()
    with torch.no_grad():
        _same(model(_dev(x)), ref["logits"], "logits")
    B, T = x.shape[0], x.shape[3]
    views = nat.lq8_workspace_views(model.workspace(B, T), B, T, 24, 1, 1)
    _same(views["xq"], _pad(ref["xq"], z_x), "xq")
    _same(views["l0.y"], ref["l0.fwd.y"], "l0.y")


def test_flip_and_roll_identities_device_against_device(cases):
    from wakeword_trainer_home_amd import _native as nat
    from wakeword_trainer_home_amd.export import QuantizedLSTM
    header, arrays, x, _, model = cases["odd"]
    B, T = x.shape[0], x.shape[3]
    views = {k: v.clone() for k, v in _whole(cases["odd"]).items()}
    with torch.no_grad():
        base = model(_dev(x))
        rolled = model(_dev(np.roll(x, 5, axis=0)))
    assert torch.equal(rolled, torch.roll(base, 5, 0))
    got = nat.lq8_workspace_views(model.workspace(B, T), B, T, 40, 2, 2)
    for k, v in views.items():
        assert torch.equal(got[k], torch.roll(v, 5, 0)), k
    # a one-layer bundle whose two directions hold the same parameters: reverse on x is forward on x flipped in time
    a = dict(arrays)
    for key in list(a):
        if ".rev." in key:
            a[key] = a[key.replace(".rev.", ".fwd.")]
    twin = QuantizedLSTM(dict(header, lstm=dict(header["lstm"], num_layers=1)), a).to(DEV)
    with torch.no_grad():
        twin(_dev(x))
        v = {k: t.clone() for k, t in nat.lq8_workspace_views(twin.workspace(B, T), B, T, 40, 1, 2).items()}
        twin(_dev(x[..., ::-1].copy()))
    f = nat.lq8_workspace_views(twin.workspace(B, T), B, T, 40, 1, 2)
    assert torch.equal(v["l0.u"][..., 512:], f["l0.u"][..., :512].flip(1))
    assert torch.equal(v["l0.y"][..., 128:], f["l0.y"][..., :128].flip(1)) and torch.equal(v["l0.c"][:, 128:], f["l0.c"][:, :128])
    assert torch.equal(v["hcat"][:, 128:], f["hcat"][:, :128]) and not torch.equal(v["l0.y"][..., 128:], v["l0.y"][..., :128])


# ------------------------------------------------------------------ the export package
ARGS = LQ.lstm_args(40, 2, True)
F_, T_ = 40, 45


def _trained_like(seed=0):
    from wakeword_trainer_home_amd.models import LSTMWakeword
    model = LSTMWakeword(input_size=40, hidden_size=128, num_layers=2, num_classes=2, bidirectional=True, dropout=0.3)
    state = LQ.random_state(ARGS, 2, seed=seed)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in state.items()})
    return model.to(DEV), state


def test_export_writes_three_bundles_and_loads_them(tmp_path):
    from wakeword_trainer_home_amd.export import (ExportConfig, ModelExporter, QuantizedLSTM, benchmark_exported_model,
                                                  load_exported_model, validate_exported_model)
    from wakeword_trainer_home_amd.export.reference import load_bundle, run_int8
    model, state = _trained_like()
    xs = LQ.structured_features(12, F_, T_, seed=2)
    x = torch.from_numpy(xs).to(DEV)
    exporter = ModelExporter(model, (1, 1, F_, T_), DEV, calibration=[x[:3], x[3:6]])
    model.train()                                                # (the exporter's constructor puts the model in eval mode)
    res = exporter.export(ExportConfig(output_path=tmp_path / "sub" / "lstm.npz", quantize_fp16=True, quantize_int8=True))
    assert model.training, "the training state was not restored"
    assert res["success"] is True and "fp16_error" not in res and "int8_error" not in res, res
    assert res["fp16_path"].endswith("lstm_fp16.npz") and res["int8_path"].endswith("lstm_int8.npz")
    assert res["int8_reduction"] > 65 > res["fp16_reduction"] > 45                # about a quarter and a half of the fp32 bundle
    model.eval()
    with torch.no_grad():
        want = model(x)
    for kind in ("path", "fp16_path", "int8_path"):
        header, _ = load_bundle(res[kind])
        assert header["architecture"] == "LSTMWakeword" and header["lstm"] == ARGS
        v = validate_exported_model(res[kind], model, x, DEV)
        assert v["valid"] and v["error"] is None and v["inference_success"] and tuple(v["output_shape"]) == (12, 2), v
        if kind == "path":
            assert v["max_difference"] == 0.0 and v["numerically_equivalent"]    # the stored state in the same class
        b = benchmark_exported_model(res[kind], model, x, num_runs=2, device=DEV)
        assert b["pytorch_time_ms"] > 0 and b["exported_time_ms"] > 0
    with torch.no_grad():
        loaded = load_exported_model(res["path"], DEV)
        assert type(loaded).__name__ == "LSTMWakeword" and not loaded.training
        assert torch.equal(loaded(x), want)
        got16 = load_exported_model(res["fp16_path"], DEV)(x).cpu().numpy().astype(np.float64)
        q8 = load_exported_model(res["int8_path"], DEV)
        got8 = q8(x)
        got8_long = q8(torch.cat([x, x.flip(3)], dim=3))        # the bundle is not tied to one T
    # fp16: what rounding every weight to fp16 does to the float64 model, up to the fp32 round-off of the device forward (sums of
    # up to 256 products through 45 steps and two layers: a few 1e-6 of gate values below 1; the bound allows 1e-4)
    state16 = {k: v.astype(np.float16).astype(np.float32) for k, v in state.items()}
    f64, f64_16 = LQ.float_forward(state, ARGS, xs), LQ.float_forward(state16, ARGS, xs)
    d16 = np.abs(got16 - want.cpu().numpy().astype(np.float64)).max()
    print(f"MEASURED fp16 bundle vs fp32 model {d16:.4g}; float64 model under fp16 weights {np.abs(f64_16 - f64).max():.4g}; "
          f"device vs float64 under fp16 weights {np.abs(got16 - f64_16).max():.4g}")
    assert np.abs(got16 - f64_16).max() <= 1e-4
    assert 0.0 < d16 <= np.abs(f64_16 - f64).max() + 2e-4
    # int8: the device runs the bundle as the interpreter and the restated law do
    assert isinstance(q8, QuantizedLSTM)
    header, arrays = load_bundle(res["int8_path"])
    _same(got8, run_int8(header, arrays, xs)["logits"], "exported int8 bundle")
    _same(got8, LQ.r_forward(ARGS, arrays, xs)["logits"], "exported int8 bundle, restated")
    _same(got8_long, run_int8(header, arrays, np.concatenate([xs, xs[..., ::-1]], axis=3))["logits"], "twice the frames")
    cal = header["calibration"]
    assert cal == {"x_min": float(xs[:6].min()), "x_max": float(xs[:6].max()), "samples": 6}
    want_arrays = LQ.r_quantize_model(state, ARGS, cal["x_min"], cal["x_max"])
    assert sorted(arrays) == sorted(want_arrays) and all(np.array_equal(arrays[k], want_arrays[k]) for k in want_arrays)


def test_calibrate_lstm_equals_numpy_minimum_and_maximum():
    from wakeword_trainer_home_amd.data.feature_extraction import FeatureExtractor
    from wakeword_trainer_home_amd.export import calibrate_lstm
    from wakeword_trainer_home_amd.export.quantize import QuantizationError
    xs = LQ.structured_features(9, 40, 70, seed=6)
    x = torch.from_numpy(xs).to(DEV)
    seq = torch.from_numpy(np.ascontiguousarray(LQ.features(3, 11, 40, seed=9)[:, 0].transpose(0, 2, 1))).to(DEV)
    cal = calibrate_lstm(None, [x[:4], x[4:], seq], 40, DEV)             # (B,1,F,T) and (B,T,F) batches of different lengths
    both = np.concatenate([xs.reshape(-1), seq.cpu().numpy().reshape(-1)])
    assert cal == {"x_min": float(both.min()), "x_max": float(both.max()), "samples": 12}
    fe = FeatureExtractor(n_mels=40, device=DEV)
    waves = torch.from_numpy(np.random.default_rng(3).normal(0, 0.1, (3, 7040)).astype(np.float32)).to(DEV)
    feats = fe(waves).cpu().numpy()
    cal = calibrate_lstm(None, [waves], 40, DEV, fe)                      # waveforms go through the feature extractor
    assert cal == {"x_min": float(feats.min()), "x_max": float(feats.max()), "samples": 3}
    with pytest.raises(QuantizationError, match="empty"):
        calibrate_lstm(None, [], 40, DEV)
    with pytest.raises(QuantizationError, match="expected"):
        calibrate_lstm(None, [x[:, :, :39]], 40, DEV)
    with pytest.raises(QuantizationError, match="feature_extractor"):
        calibrate_lstm(None, [waves], 40, DEV)


def test_int8_lstm_needs_calibration(tmp_path):
    from wakeword_trainer_home_amd.export import ExportConfig, ModelExporter
    model, _ = _trained_like()
    res = ModelExporter(model, (1, 1, F_, T_), DEV).export(ExportConfig(output_path=tmp_path / "a.npz", quantize_int8=True))
    assert res["success"] is True and "calibration" in res["int8_error"] and "int8_path" not in res


class _Spy(torch.nn.Module):
    """Passes batches to the int8 model and keeps the features it was given."""

    def __init__(self, inner):
        super().__init__()
        self.inner, self.seen = inner, []

    def forward(self, x):
        self.seen.append(x.detach().cpu().numpy())
        return self.inner(x)


class _Replay(torch.nn.Module):
    def __init__(self, logits):
        super().__init__()
        self.logits, self.at = logits, 0

    def forward(self, x):
        self.at += x.shape[0]
        return self.logits[self.at - x.shape[0]:self.at]


def test_evaluator_and_scanner_score_the_int8_lstm_as_the_restated_law(tmp_path, cases):
    """Clips of 7040 samples are 45 frames.  The evaluator and the scanner on the loaded int8 bundle (the one-layer bundle of
    ``tiny``: an LSTM bundle takes any T) against the same tools replaying the restated law's logits of the very features the model
    was given."""
    from wakeword_trainer_home_amd.data import make_synthetic_batch
    from wakeword_trainer_home_amd.evaluation import ModelEvaluator, RecordingScanner
    from wakeword_trainer_home_amd.export import load_exported_model
    from wakeword_trainer_home_amd.export.bundle import write_bundle
    header, arrays = cases["tiny"][:2]
    n, dur = 7040, 7040 / 16000
    spy = _Spy(load_exported_model(write_bundle(tmp_path / "l_int8.npz", header, arrays), DEV))
    waves, _ = make_synthetic_batch(13, n, seed=11)
    ev = ModelEvaluator(spy, sample_rate=16000, audio_duration=dur, device=DEV, n_mels=40)
    got = ev.evaluate_waveforms(waves, threshold=0.5, batch_size=8)
    counters = dict(ev.last_counters)
    feats = np.concatenate(spy.seen)
    assert feats.shape == (13, 1, 40, 45)
    want_logits = torch.from_numpy(LQ.r_forward(header["lstm"], arrays, feats)["logits"]).to(DEV)
    ev2 = ModelEvaluator(_Replay(want_logits), sample_rate=16000, audio_duration=dur, device=DEV, n_mels=40)
    want = ev2.evaluate_waveforms(waves, threshold=0.5, batch_size=8)
    assert len(got) == 13 and counters == ev2.last_counters and counters["count"] == 13
    assert [r.confidence for r in got] == [r.confidence for r in want]
    assert [r.prediction for r in got] == [r.prediction for r in want]
    assert all(np.array_equal(a.logits, b.logits) for a, b in zip(got, want))
    assert len({r.confidence for r in got}) > 4                  # the clips do not all score alike
    # the scanner: a recording of 3.5 windows at 50 % overlap
    rng = np.random.default_rng(21)
    S = int(3.5 * n)
    audio = (rng.normal(0, 0.1, S) * np.repeat(rng.choice([0.01, 0.3, 1.0, 3.0], S // 880), 880)).astype(np.float32)
    spy.seen.clear()
    kw = dict(sample_rate=16000, audio_duration=dur, threshold=0.5, device=DEV, n_mels=40, batch_size=4)
    scanner = RecordingScanner(spy, **kw)
    W = scanner.num_windows(S)
    assert W == 6
    got = scanner.scan(audio)
    feats = np.concatenate(spy.seen)
    assert feats.shape == (W, 1, 40, 45)
    want_logits = torch.from_numpy(LQ.r_forward(header["lstm"], arrays, feats)["logits"]).to(DEV)
    want = RecordingScanner(_Replay(want_logits), **kw).scan(audio)
    assert len(got) == W and got == want and len({c for c, _ in got}) > 1
