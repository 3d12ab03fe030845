"""The int8 TCN kernels and the TCN half of the export package on the GPU.  Integer arithmetic is exact, so every comparison with
the restated law (tests/q8_tcn_cases.py) is bit for bit: no tolerance anywhere in this file but the calibration's fp32-vs-fp64
check and the fp16 bundle's weight rounding."""
import os

import numpy as np
import pytest
import torch

from tests import q8_tcn_cases as TQ

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TRIPS_BATCH = 12        # the default model on 12 x 45 = 540 rows: nine 64-row groups, so a capped conv launch makes several trips
IDENTITY_TRIPS_BATCH = 60   # 300 rows of 64 bytes: 1200 vectors, five passes of one capped workgroup of the identity-skip add


@pytest.fixture(scope="module")
def cases():
    """name -> (header, arrays, x, restated stages, QuantizedTCN on the device); computed once, never modified."""
    from wakeword_trainer_home_amd.export import QuantizedTCN
    out = {}
    for name in list(TQ.SHAPES) + ["small3", "trips", "identity_trips"]:
        if name == "small3":
            case = TQ.hard_case("small", num_classes=3)
        elif name == "trips":
            case = TQ.hard_case("default", batch=TRIPS_BATCH)
        elif name == "identity_trips":
            case = TQ.hard_case("identity", batch=IDENTITY_TRIPS_BATCH)
        else:
            case = TQ.hard_case(name)
        out[name] = case + (QuantizedTCN(case[0], case[1]).to(DEV),)
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


@pytest.fixture
def grid_cap():
    from wakeword_trainer_home_amd import _native as nat
    yield lambda n: nat.set_grid_cap(DEV, n)
    nat.set_grid_cap(DEV, 0)


def _layers(case):
    """Every layer kernel alone, each fed the restated law's own input tensor in the device layout."""
    from wakeword_trainer_home_amd import _native as nat
    header, arrays, x, ref, model = case
    args = header["tcn"]
    z_x = int(arrays["input_zero"][0])
    _same(nat.tq8_quantize_bt(_dev(x[:, 0]), arrays["input_scale"][0], z_x), _pad(ref["xq"], z_x), "quantize")
    prev, zero, cin = ref["xq"], z_x, args["input_size"]
    for i, c in enumerate(args["num_channels"]):
        d, p = 2 ** i, f"b{i}."
        a_in = _dev(_pad(prev, zero))
        _same(nat.tq8_conv1d_fwd(a_in, *model.conv(i, "conv1"), d, zero), _pad(ref[p + "h1"], -128), p + "conv1")
        _same(nat.tq8_conv1d_fwd(_dev(_pad(ref[p + "h1"], -128)), *model.conv(i, "conv2"), d, -128), _pad(ref[p + "h2"], -128),
              p + "conv2")
        h2 = _dev(_pad(ref[p + "h2"], -128))
        m_a, sh_a = int(arrays[p + "add.m"][0]), int(arrays[p + "add.sh"][0])
        if cin != c:
            out = nat.tq8_conv1d_fwd(a_in, *model.conv(i, "down"), 1, zero, residual=h2, res_mult=m_a, res_shift=sh_a)
        else:
            out = nat.tq8_skip_add_fwd(a_in, h2, zero, int(arrays[p + "skip.m"][0]), int(arrays[p + "skip.sh"][0]), m_a, sh_a)
        _same(out, _pad(ref[p + "out"], -128), p + "out")
        prev, zero, cin = ref[p + "out"], -128, c
    pool, logits = nat.tq8_pool_fc_fwd(_dev(_pad(prev, -128)), cin, int(arrays["pool.m"][0]), int(arrays["pool.sh"][0]), model.fc_w,
                                       model.fc_b, model.fc_scale)
    _same(pool, ref["pool"], "pool")
    _same(logits, ref["logits"], "logits")


def _whole(case):
    """One forward; every stage tensor read back from the workspace, pad channels included."""
    from wakeword_trainer_home_amd import _native as nat
    header, arrays, x, ref, model = case
    args = header["tcn"]
    B, F, T = x.shape[0], x.shape[2], x.shape[3]
    model._ws.clear()                                            # a fresh workspace: what is read below was written by this call
    with torch.no_grad():
        logits = model(_dev(x))
    _same(logits, ref["logits"], "logits")
    views = nat.tq8_workspace_views(model.workspace(B), B, F, T, args["num_channels"])
    for stage in TQ.stages(args)[:-1]:
        want = ref[stage] if stage == "pool" else _pad(ref[stage], int(arrays["input_zero"][0]) if stage == "xq" else -128)
        _same(views[stage], want, stage)


@pytest.mark.parametrize("name", list(TQ.SHAPES))
def test_each_layer_kernel_alone(cases, name):
    _layers(cases[name])


@pytest.mark.parametrize("name", list(TQ.SHAPES) + ["small3"])
def test_whole_model_every_tensor(cases, name):
    _whole(cases[name])
    if name == "small3":
        assert cases[name][3]["logits"].shape == (5, 3)
    else:                                                        # a batch slice (another base address) takes the same path
        _, _, x, ref, model = cases[name]
        with torch.no_grad():
            _same(model(_dev(x)[1:]), ref["logits"][1:], "batch slice")


def test_kernels_make_several_trips_under_a_grid_cap(cases, grid_cap):
    """One workgroup of four waves walks everything.  ``small``: 350 rows = six 64-row groups over one channel tile, two trips;
    ``trips`` (the default model at B = 12): nine groups x 1, 2 and 4 channel tiles, three to nine trips per conv, 34 passes of
    the quantize kernel; ``identity_trips``: five 64-row groups, two trips per conv, five passes of the identity-skip add."""
    grid_cap(1)
    for name in ("small", "trips", "identity_trips"):
        _whole(cases[name])
        _layers(cases[name])
    for cap in (2, 3, 4, 9):         # the LDS form of the conv kernel: a workgroup per channel tile where the grid divides, else all tiles
        grid_cap(cap)
        _whole(cases["trips"])


@pytest.fixture
def streamed_weights():
    """The conv launches that follow stream their weights through L2 instead of holding a channel tile's in LDS."""
    old = os.environ.get("WW_TQ8_WEIGHTS")
    os.environ["WW_TQ8_WEIGHTS"] = "stream"
    yield
    if old is None:
        del os.environ["WW_TQ8_WEIGHTS"]
    else:
        os.environ["WW_TQ8_WEIGHTS"] = old


def test_streamed_weights_form_gives_the_same_bits(cases, grid_cap, streamed_weights):
    for name in TQ.SHAPES:
        _layers(cases[name])
        _whole(cases[name])
    grid_cap(1)
    for name in ("small", "trips", "identity_trips"):
        _whole(cases[name])


def test_quantize_special_values_and_odd_shapes():
    from wakeword_trainer_home_amd import _native as nat
    g = np.random.default_rng(2)
    for B, F, T in ((1, 4, 1), (2, 12, 5), (3, 40, 45), (1, 68, 7)):
        x = (g.normal(0, 6, (B, F, T)) * g.choice([1.0, 1e-3, 40.0], (B, F, T))).astype(np.float32)
        flat = x.reshape(-1)
        flat[::7] = np.resize(np.array([np.nan, np.inf, -np.inf, 0.03125, 0.09375, -0.03125, 3.4e38], np.float32), flat[::7].size)
        for scale, zero in ((np.float32(0.0625), 76), (np.float32(1.7e-3), 127), (np.float32(3.3), -128)):
            want = _pad(np.ascontiguousarray(TQ.r_quantize_input(x, scale, zero).transpose(0, 2, 1)), zero)
            _same(nat.tq8_quantize_bt(_dev(x), scale, zero), want, f"{(B, F, T)} zero={zero}")


# ------------------------------------------------------------------ the export package
ARGS = TQ.tcn_args(40, [64, 128, 256], 3)
F_, T_ = 40, 45


def _trained_like(seed=0):
    from wakeword_trainer_home_amd.models import TCNWakeword
    model = TCNWakeword(input_size=40, num_channels=[64, 128, 256], kernel_size=3, num_classes=2, dropout=0.3)
    state = TQ.random_state(ARGS, 2, seed=seed, gain=2.0)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in state.items()})
    return model.to(DEV), state


def test_export_writes_three_bundles_and_loads_them(tmp_path):
    from wakeword_trainer_home_amd.export import (ExportConfig, ModelExporter, QuantizedTCN, benchmark_exported_model,
                                                  load_exported_model, validate_exported_model)
    from wakeword_trainer_home_amd.export.reference import load_bundle, run_int8
    model, state = _trained_like()
    xs = TQ.structured_features(20, F_, T_, seed=2)
    x = torch.from_numpy(xs).to(DEV)
    exporter = ModelExporter(model, (1, 1, F_, T_), DEV, calibration=[x[:6], x[6:12]])
    model.train()                                                # (the exporter's constructor puts the model in eval mode)
    res = exporter.export(
        ExportConfig(output_path=tmp_path / "sub" / "tcn.npz", quantize_fp16=True, quantize_int8=True))
    assert model.training, "the training state was not restored"
    assert res["success"] is True and "fp16_error" not in res and "int8_error" not in res, res
    assert res["fp16_path"].endswith("tcn_fp16.npz") and res["int8_path"].endswith("tcn_int8.npz")
    assert res["int8_reduction"] > res["fp16_reduction"] > 20
    model.eval()
    with torch.no_grad():
        want = model(x)
    for kind in ("path", "fp16_path", "int8_path"):
        header, _ = load_bundle(res[kind])
        assert header["architecture"] == "TCNWakeword" and header["tcn"] == ARGS
        v = validate_exported_model(res[kind], model, x, DEV)
        assert v["valid"] and v["error"] is None and v["inference_success"] and tuple(v["output_shape"]) == (20, 2), v
        b = benchmark_exported_model(res[kind], model, x, num_runs=2, device=DEV)
        assert b["pytorch_time_ms"] > 0 and b["exported_time_ms"] > 0
    # fp32: the stored state in the same class -- the same logits exactly
    with torch.no_grad():
        loaded = load_exported_model(res["path"], DEV)
        assert type(loaded).__name__ == "TCNWakeword" and not loaded.training
        assert torch.equal(loaded(x), want)
        got16 = load_exported_model(res["fp16_path"], DEV)(x).cpu().numpy().astype(np.float64)
        q8 = load_exported_model(res["int8_path"], DEV)
        got8 = q8(x)
    # fp16: what rounding every weight to fp16 does to the float64 model, up to the fp32 round-off of the device forward.  That
    # round-off: products of K <= 768 terms accumulated in fp32 through seven layers, a few 1e-5 of the largest logit; the bound
    # below allows 2e-4 of it.
    state16 = {k: v.astype(np.float16).astype(np.float32) for k, v in state.items()}
    f64, _ = TQ.float_forward(state, ARGS, xs)
    f64_16, _ = TQ.float_forward(state16, ARGS, xs)
    slack = 2e-4 * max(1.0, float(np.abs(f64).max()))
    d16 = np.abs(got16 - want.cpu().numpy().astype(np.float64)).max()
    print(f"MEASURED fp16 bundle vs fp32 model {d16:.4g}; float64 model under fp16 weights {np.abs(f64_16 - f64).max():.4g}; "
          f"device vs float64 under fp16 weights {np.abs(got16 - f64_16).max():.4g} (slack {slack:.4g})")
    assert np.abs(got16 - f64_16).max() <= slack
    assert 0.0 < d16 <= np.abs(f64_16 - f64).max() + 2 * slack
    # int8: the device runs the bundle as the interpreter and the restated law do
    assert isinstance(q8, QuantizedTCN)
    header, arrays = load_bundle(res["int8_path"])
    _same(got8, run_int8(header, arrays, xs)["logits"], "exported int8 bundle")
    _same(got8, TQ.r_forward(ARGS, arrays, xs)["logits"], "exported int8 bundle, restated")
    want_arrays = TQ.r_quantize_model(state, ARGS, (F_, T_), header["calibration"])
    assert all(np.array_equal(arrays[k], want_arrays[k]) for k in want_arrays) and sorted(arrays) == sorted(want_arrays)
    # the calibration saw the fp32 model: its ranges are the float64 model's up to fp32 round-off
    _, ranges = TQ.float_forward(state, ARGS, xs[:12])
    cal = header["calibration"]
    assert cal["samples"] == 12 and cal["x_min"] == ranges["x_min"] and cal["x_max"] == ranges["x_max"]
    np.testing.assert_allclose(cal["a_max"] + [cal["p_max"]], ranges["a_max"] + [ranges["p_max"]], rtol=1e-4)


def test_calibrate_tcn_equals_the_restated_ranges():
    from wakeword_trainer_home_amd.export import calibrate_tcn
    from wakeword_trainer_home_amd.export.quantize import QuantizationError
    from wakeword_trainer_home_amd.models import TCNWakeword
    args = TQ.tcn_args(40, [32, 32, 48], 2)                       # an identity skip in block 1
    state = TQ.random_state(args, 3, seed=5)
    model = TCNWakeword(input_size=40, num_channels=[32, 32, 48], kernel_size=2, num_classes=3, dropout=0.3)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in state.items()})
    model.to(DEV).eval()
    xs = TQ.structured_features(9, 40, 70, seed=6)
    x = torch.from_numpy(xs).to(DEV)
    cal = calibrate_tcn(model, [x[:4], x[4:, 0]], (40, 70), DEV)        # a (B,F,T) batch is taken as well
    _, ranges = TQ.float_forward(state, args, xs)
    assert cal["samples"] == 9 and cal["x_min"] == ranges["x_min"] and cal["x_max"] == ranges["x_max"] and len(cal["a_max"]) == 9
    np.testing.assert_allclose(cal["a_max"] + [cal["p_max"]], ranges["a_max"] + [ranges["p_max"]], rtol=1e-4)
    with pytest.raises(QuantizationError, match="empty"):
        calibrate_tcn(model, [], (40, 70), DEV)
    with pytest.raises(QuantizationError, match="expected"):
        calibrate_tcn(model, [x[:, :, :, :69]], (40, 70), DEV)


def test_int8_tcn_needs_calibration(tmp_path):
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


def test_evaluator_and_scanner_score_the_int8_tcn_as_the_interpreter(tmp_path, cases):
    """Clips of 7040 samples are 45 frames, the default hard bundle's T.  The evaluator and the scanner on the loaded int8
    bundle against the same tools replaying the restated law's logits of the very features the model was given."""
    from wakeword_trainer_home_amd.data import make_synthetic_batch
    from wakeword_trainer_home_amd.evaluation import ModelEvaluator, RecordingScanner
    from wakeword_trainer_home_amd.export import load_exported_model
    from wakeword_trainer_home_amd.export.bundle import write_bundle
    header, arrays = cases["default"][:2]
    n, dur = 7040, 7040 / 16000
    spy = _Spy(load_exported_model(write_bundle(tmp_path / "t_int8.npz", header, arrays), DEV))
    waves, _ = make_synthetic_batch(21, n, seed=11)
    ev = ModelEvaluator(spy, sample_rate=16000, audio_duration=dur, device=DEV, n_mels=40)
    got = ev.evaluate_waveforms(waves, threshold=0.5, batch_size=8)
    counters = dict(ev.last_counters)
    feats = np.concatenate(spy.seen)
    assert feats.shape == (21, 1, 40, 45)
    want_logits = torch.from_numpy(TQ.r_forward(header["tcn"], arrays, feats)["logits"]).to(DEV)
    ev2 = ModelEvaluator(_Replay(want_logits), sample_rate=16000, audio_duration=dur, device=DEV, n_mels=40)
    want = ev2.evaluate_waveforms(waves, threshold=0.5, batch_size=8)
    assert len(got) == 21 and counters == ev2.last_counters and counters["count"] == 21
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
    want_logits = torch.from_numpy(TQ.r_forward(header["tcn"], arrays, feats)["logits"]).to(DEV)
    want = RecordingScanner(_Replay(want_logits), **kw).scan(audio)
    assert len(got) == W and got == want and len({c for c, _ in got}) > 1
