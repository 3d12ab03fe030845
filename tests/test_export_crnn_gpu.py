"""The int8 CRNN kernels and the CRNN half of the export package on the GPU.  Integer arithmetic is exact, so every comparison with
the restated law (tests/q8_crnn_cases.py) is bit for bit: no tolerance anywhere in this file but the fp16 bundle's weight rounding
and the calibration's fp32-vs-fp64 check."""
import numpy as np
import pytest
import torch

from tests import q8_crnn_cases as CQ

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TRIPS_BATCH = 40        # ``odd`` at B = 40: three 16-row batch groups of the recurrence; 280 rows of the stack's projection are five
#                         64-row groups x 12 gate-row tiles; 440 rows of the frequency mean are 28 tiles, seven workgroups' worth


class _Stack:
    """A GRU-stack case's tensors on the device, in the layout the layer entry points read."""

    def __init__(self, args, arrays):
        from wakeword_trainer_home_amd.export.runtime import device_gru_layer
        nd = len(CQ.dirs(args))
        z_x = int(arrays["input_zero"][0])
        self.layers = [tuple(_dev(t) for t in device_gru_layer(arrays, k, nd, z_x if k == 0 else 0)) for k in range(args["num_layers"])]
        self.fc = tuple(_dev(arrays[k]) for k in ("fc.w", "fc.b", "fc.scale"))
        self.tables = _dev(arrays["tab.sigmoid"]), _dev(arrays["tab.tanh"])


@pytest.fixture(scope="module")
def stacks():
    """name -> (args, arrays, x, restated tensors, _Stack); computed once, never modified."""
    out = {}
    for name in list(CQ.STACK_CASES) + ["trips"]:
        case = CQ.stack_case("odd", batch=TRIPS_BATCH) if name == "trips" else CQ.stack_case(name)
        out[name] = case[:4] + (_Stack(case[0], case[1]),)
    return out


@pytest.fixture(scope="module")
def cases():
    """name -> (header, arrays, x, restated tensors, QuantizedCRNN on the device); computed once, never modified."""
    from wakeword_trainer_home_amd.export import QuantizedCRNN
    out = {}
    for name in list(CQ.CASES) + ["trips"]:
        case = CQ.case("odd", batch=TRIPS_BATCH) if name == "trips" else CQ.case(name)
        out[name] = case + (QuantizedCRNN(case[0], case[1]).to(DEV),)
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
    return np.concatenate([ref[f"l{k}.{d}.{what}"] for d in CQ.dirs(args)], axis=-1)


@pytest.fixture
def grid_cap():
    from wakeword_trainer_home_amd import _native as nat
    yield lambda n: nat.set_grid_cap(DEV, n)
    nat.set_grid_cap(DEV, 0)


def _stack_kernels(case):
    """The projection, the recurrence and the head alone, each fed the restated law's own input tensor in the device layout."""
    from wakeword_trainer_home_amd import _native as nat
    args, arrays, _, ref, dev = case
    z_x = int(arrays["input_zero"][0])
    a_in = _pad(ref["xq"], z_x)
    G = 384 * len(CQ.dirs(args))
    for k in range(args["num_layers"]):
        w_ih, b_ih, m_i, sh_i, w_hh, b_hh, m_h, sh_h = dev.layers[k]
        assert w_ih.shape[0] == w_hh.shape[0] == G
        _same(nat.lq8_proj_fwd(_dev(a_in), w_ih, b_ih, m_i, sh_i), _stacked(ref, args, k, "u"), f"l{k} projection, G = {G}")
        y, h_n = nat.cq8_gru_layer_fwd(_dev(_stacked(ref, args, k, "u")), w_hh, b_hh, m_h, sh_h, *dev.tables)
        _same(y, _stacked(ref, args, k, "y"), f"l{k} recurrence, y")
        _same(h_n, _stacked(ref, args, k, "h"), f"l{k} recurrence, h_n")
        a_in = _stacked(ref, args, k, "y")
    hcat, logits = nat.lq8_head_fwd(_dev(a_in), *dev.fc)
    _same(hcat, ref["hcat"], "hcat")
    _same(logits, ref["logits"], "logits")


def _fmean(case):
    from wakeword_trainer_home_amd import _native as nat
    _, arrays, _, ref, _ = case
    _same(nat.cq8_fmean_fwd(_dev(ref["front.pw3"]), arrays["fmean.m"][0], arrays["fmean.sh"][0]), ref["seq"], "fmean")


def _views(model, header, x):
    from wakeword_trainer_home_amd import _native as nat
    args = header["crnn"]
    B, F, T = x.shape[0], x.shape[2], x.shape[3]
    return nat.cq8_workspace_views(model.workspace(B, T), B, F, T, args["num_layers"], len(CQ.dirs(args)))


def _whole(case):
    """One forward; every stage tensor the launches write read back from the workspace."""
    header, arrays, x, ref, model = case
    args = header["crnn"]
    model._ws.clear()                                            # a fresh workspace: what is read below was written by this call
    with torch.no_grad():
        logits = model(_dev(x))
    _same(logits, ref["logits"], "logits")
    views = _views(model, header, x)
    _same(views["xq"], ref["xq"], "xq")
    for name in ("front.stem", "front.pw0", "front.pw1", "front.pw2", "front.pw3", "seq"):
        _same(views[name], ref[name], name)
    for k in range(args["num_layers"]):
        for what in ("u", "y", "h"):
            _same(views[f"l{k}.{what}"], _stacked(ref, args, k, what), f"l{k}.{what}")
    _same(views["hcat"], ref["hcat"], "hcat")
    return views


@pytest.mark.parametrize("name", list(CQ.STACK_CASES))
def test_projection_recurrence_and_head_alone(stacks, name):
    """``uni`` is the projection at G = 384, the others at G = 768; the recurrence on all five stack cases."""
    _stack_kernels(stacks[name])


@pytest.mark.parametrize("name", list(CQ.CASES))
def test_frequency_mean_alone(cases, name):
    _fmean(cases[name])


@pytest.mark.parametrize("name", list(CQ.CASES))
def test_whole_model_every_workspace_tensor(cases, name):
    _whole(cases[name])
    _, _, x, ref, model = cases[name]
    assert ref["logits"].shape == (x.shape[0], CQ.CASES[name][5])
    with torch.no_grad():                                        # a batch slice (another base address) takes the same path
        _same(model(_dev(x)[1:]), ref["logits"][1:], "batch slice")


def test_kernels_make_several_trips_under_a_grid_cap(stacks, cases, grid_cap):
    """One or two workgroups walk everything: three batch groups per direction of the recurrence, 60 projection items, 28 tiles of
    the frequency mean; ``odd`` has a last batch group of 13 live rows."""
    for cap in (1, 2):
        grid_cap(cap)
        for name in ("trips", "odd"):
            _stack_kernels(stacks[name])
            _fmean(cases[name])
            _whole(cases[name])


def test_nan_and_infinite_inputs_on_the_device(cases):
    header, arrays, x, _, model = cases["uni"]
    x = x.copy()
    x[0, 0, 3, 1], x[1, 0, 0, 0], x[2, 0, 5, 2] = np.nan, np.inf, -np.inf
    ref = CQ.r_forward(header["crnn"], arrays, x)
    z_x = int(arrays["input_zero"][0])
    assert ref["xq"][0, 3, 1] == z_x and ref["xq"][1, 0, 0] == 127 and ref["xq"][2, 5, 2] == -128
    model._ws.clear()
    with torch.no_grad():
        _same(model(_dev(x)), ref["logits"], "logits")
    views = _views(model, header, x)
    _same(views["xq"], ref["xq"], "xq")
    _same(views["seq"], ref["seq"], "seq")
    _same(views["l0.y"], ref["l0.fwd.y"], "l0.y")
    assert np.isfinite(ref["logits"]).all()


def test_flip_and_roll_identities_device_against_device(cases, stacks):
    from wakeword_trainer_home_amd import _native as nat
    header, arrays, x, _, model = cases["odd"]
    views = {k: v.clone() for k, v in _whole(cases["odd"]).items()}
    with torch.no_grad():
        base = model(_dev(x))
        rolled = model(_dev(np.roll(x, 5, axis=0)))
    assert torch.equal(rolled, torch.roll(base, 5, 0))
    got = _views(model, header, x)
    for k, v in views.items():
        assert torch.equal(got[k], torch.roll(v, 5, 0)), k
    # a layer whose two directions hold the same parameters: its reverse direction on a sequence is its forward direction on the
    # sequence flipped in time (the SEQUENCE: the conv stack is not symmetric in time)
    args, _, _, ref, dev = stacks["odd"]
    w_ih, b_ih, m_i, sh_i, w_hh, b_hh, m_h, sh_h = (torch.cat([t[:384], t[:384]]) for t in dev.layers[0])
    seq = _dev(_pad(ref["xq"], int(stacks["odd"][1]["input_zero"][0])))
    u, uf = nat.lq8_proj_fwd(seq, w_ih, b_ih, m_i, sh_i), nat.lq8_proj_fwd(seq.flip(1).contiguous(), w_ih, b_ih, m_i, sh_i)
    assert torch.equal(u[..., 384:], uf[..., :384].flip(1))
    (y, h), (yf, hf) = (nat.cq8_gru_layer_fwd(t, w_hh, b_hh, m_h, sh_h, *dev.tables) for t in (u, uf))
    assert torch.equal(y[..., 128:], yf[..., :128].flip(1)) and torch.equal(h[:, 128:], hf[:, :128])
    assert not torch.equal(y[..., 128:], y[..., :128])
    _same(y[..., :128], ref["l0.fwd.y"], "the twin's forward direction")


# ------------------------------------------------------------------ the export package
ARGS = CQ.crnn_args(2, True)
F_, T_ = 40, 45


def _trained_like(seed=0, **kw):
    from wakeword_trainer_home_amd.models import create_model
    args = dict(ARGS, **kw)
    model = create_model("crnn", num_classes=2, num_layers=args["num_layers"], bidirectional=args["bidirectional"])
    state = CQ.random_state(args, 2, seed=seed)
    res = model.load_state_dict({k: torch.from_numpy(v) for k, v in state.items()}, strict=False)
    assert not res.unexpected_keys and all(k.endswith("num_batches_tracked") for k in res.missing_keys)
    return model.to(DEV), state


def test_export_writes_three_bundles_and_loads_them(tmp_path):
    from wakeword_trainer_home_amd.export import (ExportConfig, ModelExporter, QuantizedCRNN, load_exported_model,
                                                  validate_exported_model)
    from wakeword_trainer_home_amd.export.reference import load_bundle, run_int8
    model, state = _trained_like()
    xs = CQ.structured_features(12, F_, T_, seed=2)
    x = torch.from_numpy(xs).to(DEV)
    exporter = ModelExporter(model, (1, 1, F_, T_), DEV, calibration=[x[:3], x[3:6]])
    model.train()                                                # (the exporter's constructor puts the model in eval mode)
    res = exporter.export(ExportConfig(output_path=tmp_path / "sub" / "crnn.npz", quantize_fp16=True, quantize_int8=True))
    assert model.training, "the training state was not restored"
    assert res["success"] is True and "fp16_error" not in res and "int8_error" not in res, res
    assert res["fp16_path"].endswith("crnn_fp16.npz") and res["int8_path"].endswith("crnn_int8.npz")
    assert res["int8_reduction"] > 65 > res["fp16_reduction"] > 45                # about a quarter and a half of the fp32 bundle
    model.eval()
    with torch.no_grad():
        want = model(x)
    for kind in ("path", "fp16_path", "int8_path"):
        header, _ = load_bundle(res[kind])
        assert header["architecture"] == "crnn" and header["crnn"] == ARGS
        v = validate_exported_model(res[kind], model, x, DEV)
        assert v["valid"] and v["error"] is None and v["inference_success"] and tuple(v["output_shape"]) == (12, 2), v
        if kind == "path":
            assert v["max_difference"] == 0.0 and v["numerically_equivalent"]    # the stored state in the same class
    with torch.no_grad():
        loaded = load_exported_model(res["path"], DEV)
        assert type(loaded).__name__ == "CRNNWakeword" and not loaded.training
        assert torch.equal(loaded(x), want)
        got16 = load_exported_model(res["fp16_path"], DEV)(x).cpu().numpy().astype(np.float64)
        q8 = load_exported_model(res["int8_path"], DEV)
        got8 = q8(x)
        got8_long = q8(torch.cat([x, x.flip(3)], dim=3))        # the bundle is not tied to one T
    # fp16: what rounding every weight to fp16 does to the float64 model, up to the fp32 round-off of the device forward (nine
    # convs, then sums of up to 256 products through 23 steps and two layers; the bound allows 1e-4 as the LSTM's test does)
    state16 = {k: v.astype(np.float16).astype(np.float32) for k, v in state.items()}
    f64, f64_16 = CQ.float_forward(state, ARGS, xs), CQ.float_forward(state16, ARGS, xs)
    d16 = np.abs(got16 - want.cpu().numpy().astype(np.float64)).max()
    print(f"MEASURED fp16 bundle vs fp32 model {d16:.4g}; float64 model under fp16 weights {np.abs(f64_16 - f64).max():.4g}; "
          f"device vs float64 under fp16 weights {np.abs(got16 - f64_16).max():.4g}")
    assert np.abs(got16 - f64_16).max() <= 1e-4
    assert 0.0 < d16 <= np.abs(f64_16 - f64).max() + 2e-4
    # int8: the device runs the bundle as the interpreter and the restated law do
    assert isinstance(q8, QuantizedCRNN)
    header, arrays = load_bundle(res["int8_path"])
    _same(got8, run_int8(header, arrays, xs)["logits"], "exported int8 bundle")
    _same(got8, CQ.r_forward(ARGS, arrays, xs)["logits"], "exported int8 bundle, restated")
    _same(got8_long, CQ.r_forward(ARGS, arrays, np.concatenate([xs, xs[..., ::-1]], axis=3))["logits"], "twice the frames")
    cal = header["calibration"]
    want_arrays = CQ.r_quantize_model(state, ARGS, F_, cal)
    assert sorted(arrays) == sorted(want_arrays) and all(np.array_equal(arrays[k], want_arrays[k]) for k in want_arrays)


def test_a_non_default_crnn_is_reloaded_from_its_entry(tmp_path):
    from wakeword_trainer_home_amd.export import ExportConfig, ModelExporter, load_exported_model
    from wakeword_trainer_home_amd.export.reference import load_bundle
    model, _ = _trained_like(seed=2, num_layers=1, bidirectional=False)
    x = torch.from_numpy(CQ.structured_features(4, F_, 21, seed=3)).to(DEV)
    res = ModelExporter(model, (1, 1, F_, 21), DEV, calibration=[x]).export(
        ExportConfig(output_path=tmp_path / "c.npz", quantize_fp16=True, quantize_int8=True))
    assert res["success"] is True and "int8_error" not in res and "fp16_error" not in res, res
    assert load_bundle(res["path"])[0]["crnn"] == CQ.crnn_args(1, False)
    with torch.no_grad():
        want = model(x)
        loaded = load_exported_model(res["path"], DEV)
        assert loaded.rnn.num_layers == 1 and not loaded.rnn.bidirectional and torch.equal(loaded(x), want)
        q8 = load_exported_model(res["int8_path"], DEV)
        assert q8.num_layers == 1 and q8.num_directions == 1 and q8(x).shape == (4, 2)


def test_calibrate_crnn_equals_numpy_maxima():
    """The calibration saw the fp32 model: its ranges are the float64 model's up to fp32 round-off (rtol 1e-4, the bound the
    cnn_small calibration is held to); the input range is exact.  Batches of different lengths."""
    from wakeword_trainer_home_amd.export import calibrate_crnn
    from wakeword_trainer_home_amd.export.quantize import QuantizationError
    model, state = _trained_like(seed=1)
    xa, xb = CQ.structured_features(5, F_, 45, seed=6), CQ.structured_features(4, F_, 70, seed=7)
    model.train()                                                # the calibration runs the front end in eval mode and puts this back
    cal = calibrate_crnn(model, [_dev(xa[:2]), _dev(xa[2:]), _dev(xb)], F_, DEV)
    ra, rb = CQ.float_front(state, xa)[1], CQ.float_front(state, xb)[1]
    assert cal["samples"] == 9 and sorted(cal) == ["a_max", "f_max", "samples", "x_max", "x_min"]
    assert cal["x_min"] == float(min(xa.min(), xb.min())) and cal["x_max"] == float(max(xa.max(), xb.max()))
    want = [max(p, q) for p, q in zip(ra["a_max"] + [ra["f_max"]], rb["a_max"] + [rb["f_max"]])]
    np.testing.assert_allclose(cal["a_max"] + [cal["f_max"]], want, rtol=1e-4)
    assert model.front.training and model.training, "the training state was not restored"
    with pytest.raises(QuantizationError, match="empty"):
        calibrate_crnn(model, [], F_, DEV)
    with pytest.raises(QuantizationError, match="expected"):
        calibrate_crnn(model, [_dev(xa[:, :, :39])], F_, DEV)
    with pytest.raises(QuantizationError, match="feature_extractor"):
        calibrate_crnn(model, [torch.zeros(2, 7040, device=DEV)], F_, DEV)


def test_int8_crnn_needs_calibration(tmp_path):
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


def test_evaluator_and_scanner_score_the_int8_crnn_as_the_restated_law(tmp_path):
    """Clips of 7040 samples are 45 frames, the T the bundle was calibrated at; the scanner runs windows of 4800 samples, 31 frames
    (a CRNN bundle takes any T).  Both tools on the loaded int8 bundle against the same tools replaying the restated law's logits
    of the very features the model was given."""
    from wakeword_trainer_home_amd.data import make_synthetic_batch
    from wakeword_trainer_home_amd.evaluation import ModelEvaluator, RecordingScanner
    from wakeword_trainer_home_amd.export import QuantizedCRNN, load_exported_model
    from wakeword_trainer_home_amd.export.bundle import write_bundle
    header, arrays, _, _ = CQ.build(2, 40, 45, 1, True, 2, seed=9)
    args = header["crnn"]
    n, dur = 7040, 7040 / 16000
    inner = load_exported_model(write_bundle(tmp_path / "c_int8.npz", header, arrays), DEV)
    assert isinstance(inner, QuantizedCRNN)
    spy = _Spy(inner)
    waves, _ = make_synthetic_batch(13, n, seed=11)
    ev = ModelEvaluator(spy, sample_rate=16000, audio_duration=dur, device=DEV, n_mels=40)
    got = ev.evaluate_waveforms(waves, threshold=0.5, batch_size=8)
    counters = dict(ev.last_counters)
    feats = np.concatenate(spy.seen)
    assert feats.shape == (13, 1, 40, 45)
    want_logits = torch.from_numpy(CQ.r_forward(args, arrays, feats)["logits"]).to(DEV)
    ev2 = ModelEvaluator(_Replay(want_logits), sample_rate=16000, audio_duration=dur, device=DEV, n_mels=40)
    want = ev2.evaluate_waveforms(waves, threshold=0.5, batch_size=8)
    assert len(got) == 13 and counters == ev2.last_counters and counters["count"] == 13
    assert [r.confidence for r in got] == [r.confidence for r in want]
    assert [r.prediction for r in got] == [r.prediction for r in want]
    assert all(np.array_equal(a.logits, b.logits) for a, b in zip(got, want))
    assert len({r.confidence for r in got}) > 4                  # the clips do not all score alike
    # the scanner: a recording of 3.5 windows at 50 % overlap, the window shorter than the calibration clips
    n2 = 4800
    rng = np.random.default_rng(21)
    S = int(3.5 * n2)
    audio = (rng.normal(0, 0.1, S) * np.repeat(rng.choice([0.01, 0.3, 1.0, 3.0], S // 800), 800)).astype(np.float32)
    spy.seen.clear()
    kw = dict(sample_rate=16000, audio_duration=n2 / 16000, threshold=0.5, device=DEV, n_mels=40, batch_size=4)
    scanner = RecordingScanner(spy, **kw)
    W = scanner.num_windows(S)
    assert W == 6
    got = scanner.scan(audio)
    feats = np.concatenate(spy.seen)
    assert feats.shape == (W, 1, 40, 31)
    want_logits = torch.from_numpy(CQ.r_forward(args, arrays, feats)["logits"]).to(DEV)
    want = RecordingScanner(_Replay(want_logits), **kw).scan(audio)
    assert len(got) == W and got == want and len({c for c, _ in got}) > 1
