"""The int8 kernels and the export package on the GPU.  Integer arithmetic is exact, so every comparison with the restated law
(tests/q8_cases.py) is bit for bit: no tolerance anywhere in this file but the calibration's fp32-vs-fp64 check."""
import numpy as np
import pytest
import torch

from tests import q8_cases as Q

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LAYER_SHAPES = [(3, 13, 21), (1, 40, 151)]      # stem output 7x11 = 77 pixels, 231 in all: no multiple of 16
MODEL_SHAPES = [(5, 40, 151), (2, 40, 38)]


@pytest.fixture(scope="module")
def cases():
    """shape -> (header, arrays, x, restated stages, QuantizedCNNSmall on the device); computed once, never modified."""
    from wakeword_trainer_home_amd.export import QuantizedCNNSmall
    out = {}
    for B, F, T in LAYER_SHAPES + MODEL_SHAPES:
        header, arrays = Q.hard_bundle(F, T)
        x = Q.hard_features(F, T, B)
        ref = Q.r_forward(arrays, x, want_acc=True)
        Q.assert_hard(arrays, ref)
        out[(B, F, T)] = (header, arrays, x, ref, QuantizedCNNSmall(header, arrays).to(DEV))
    return out


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _same(got, want, what):
    got = got.cpu().numpy()
    assert got.dtype == want.dtype and got.shape == want.shape, what
    bad = np.flatnonzero(got.reshape(-1) != want.reshape(-1))
    assert bad.size == 0, f"{what}: {bad.size} of {got.size} differ, first at {np.unravel_index(bad[0], got.shape)}"


@pytest.fixture
def grid_cap():
    from wakeword_trainer_home_amd import _native as nat
    yield lambda n: nat.set_grid_cap(DEV, n)
    nat.set_grid_cap(DEV, 0)


@pytest.mark.parametrize("shape", LAYER_SHAPES)
def test_each_layer_kernel_alone(cases, shape):
    from wakeword_trainer_home_amd import _native as nat
    _, arrays, x, ref, model = cases[shape]
    xq = nat.q8_quantize(_dev(x[:, 0]), arrays["input_scale"][0], int(arrays["input_zero"][0]))
    _same(xq, ref["xq"], "quantize")
    _same(nat.q8_stem_fwd(_dev(ref["xq"]), *model.conv("stem"), int(arrays["input_zero"][0])), ref["stem"], "stem")
    prev = "stem"
    for k in range(4):
        _same(nat.q8_dwconv3x3_fwd(_dev(ref[prev]), *model.conv(f"dw{k}")), ref[f"dw{k}"], f"dw{k}")
        _same(nat.q8_pwconv1x1_fwd(_dev(ref[f"dw{k}"]), *model.conv(f"pw{k}")), ref[f"pw{k}"], f"pw{k}")
        prev = f"pw{k}"
    pool, logits = nat.q8_gap_fc_fwd(_dev(ref["pw3"]), int(arrays["pool.m"][0]), int(arrays["pool.sh"][0]), model.fc_w, model.fc_b,
                                     model.fc_scale)
    _same(pool, ref["pool"], "pool")
    _same(logits, ref["logits"], "logits")


def test_quantize_special_values_and_odd_lengths():
    from wakeword_trainer_home_amd import _native as nat
    g = np.random.default_rng(2)
    for n in (1, 3, 4, 1023, 4099):
        x = (g.normal(0, 6, n) * g.choice([1.0, 1e-3, 40.0], n)).astype(np.float32)
        x[:: 7] = [np.nan, np.inf, -np.inf, 0.03125, 0.09375, -0.03125, 3.4e38][n % 7]
        for scale, zero in ((np.float32(0.0625), 76), (np.float32(1.7e-3), 127), (np.float32(3.3), -128)):
            _same(nat.q8_quantize(_dev(x), scale, zero), Q.r_quantize_input(x, scale, zero), f"n={n} zero={zero}")


def test_kernels_make_several_trips_under_a_grid_cap(cases, grid_cap):
    """(1,40,151): 1520 pixels = 95 tiles of 16; two workgroups of four waves walk them in twelve trips each."""
    from wakeword_trainer_home_amd import _native as nat
    _, arrays, x, ref, model = cases[(1, 40, 151)]
    assert ref["stem"].size // 64 == 1520
    grid_cap(2)
    _same(nat.q8_pwconv1x1_fwd(_dev(ref["dw1"]), *model.conv("pw1")), ref["pw1"], "pw1")
    _same(nat.q8_dwconv3x3_fwd(_dev(ref["pw0"]), *model.conv("dw1")), ref["dw1"], "dw1")
    _same(nat.q8_dwpw_fwd(_dev(ref["pw0"]), model.conv("dw1"), model.conv("pw1")), ref["pw1"], "dw1+pw1")
    _same(nat.q8_stem_fwd(_dev(ref["xq"]), *model.conv("stem"), int(arrays["input_zero"][0])), ref["stem"], "stem")
    grid_cap(1)
    _same(nat.q8_pwconv1x1_fwd(_dev(ref["dw3"]), *model.conv("pw3")), ref["pw3"], "pw3")


@pytest.mark.parametrize("shape", LAYER_SHAPES)
def test_fused_pair_equals_the_two_launches(cases, shape):
    from wakeword_trainer_home_amd import _native as nat
    _, _, _, ref, model = cases[shape]
    prev = "stem"
    for k in range(4):
        a = _dev(ref[prev])
        pair = nat.q8_pwconv1x1_fwd(nat.q8_dwconv3x3_fwd(a, *model.conv(f"dw{k}")), *model.conv(f"pw{k}"))
        fused = nat.q8_dwpw_fwd(a, model.conv(f"dw{k}"), model.conv(f"pw{k}"))
        assert torch.equal(pair, fused), f"block {k}"
        _same(fused, ref[f"pw{k}"], f"block {k}")
        prev = f"pw{k}"


@pytest.mark.parametrize("shape", MODEL_SHAPES + LAYER_SHAPES[:1])
@pytest.mark.parametrize("form", ["pair", "fused"])
def test_whole_model_every_tensor(cases, shape, form):
    from wakeword_trainer_home_amd import _native as nat
    B, F, T = shape
    _, _, x, ref, model = cases[shape]
    model.set_form(form)
    model._ws.clear()                                            # a fresh workspace: what is read below was written by this call
    with torch.no_grad():
        logits = model(_dev(x))
    _same(logits, ref["logits"], "logits")
    views = nat.q8_workspace_views(model.workspace(B), B, F, T)
    for stage in Q.STAGES[:-1]:
        if form == "fused" and stage.startswith("dw"):
            continue                                             # the fused form keeps the depthwise output in registers
        _same(views[stage], ref[stage], stage)
    # a batch slice whose storage is not 16-byte aligned takes the same path
    if (F * T) % 4:
        with torch.no_grad():
            _same(model(_dev(x)[1:]), ref["logits"][1:], "unaligned slice")


def test_evaluator_scores_the_int8_model_as_the_interpreter(tmp_path, cases):
    """41 synthetic clips at batch size 16 (16 + 16 + 9) through ModelEvaluator on the loaded int8 bundle, against the same
    evaluator scoring the restated law's logits of the same features."""
    from wakeword_trainer_home_amd.data import make_synthetic_batch
    from wakeword_trainer_home_amd.evaluation import ModelEvaluator
    from wakeword_trainer_home_amd.export import load_exported_model
    from wakeword_trainer_home_amd.export.bundle import write_bundle
    header, arrays = cases[(5, 40, 151)][:2]
    model = load_exported_model(write_bundle(tmp_path / "m_int8.npz", header, arrays), DEV)
    waves, _ = make_synthetic_batch(41, 24000, seed=11)
    ev = ModelEvaluator(model, sample_rate=16000, audio_duration=1.5, device=DEV, n_mels=40)
    got = ev.evaluate_waveforms(waves, threshold=0.5, batch_size=16)
    counters = dict(ev.last_counters)
    feats = ev.feature_extractor(waves).cpu().numpy()
    want_logits = torch.from_numpy(Q.r_forward(arrays, feats)["logits"]).to(DEV)

    class Replay(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.at = 0

        def forward(self, x):
            self.at += x.shape[0]
            return want_logits[self.at - x.shape[0]:self.at]
    ev2 = ModelEvaluator(Replay(), sample_rate=16000, audio_duration=1.5, device=DEV, n_mels=40)
    want = ev2.evaluate_waveforms(waves, threshold=0.5, batch_size=16)
    assert len(got) == 41 and counters == ev2.last_counters and counters["count"] == 41
    assert [r.confidence for r in got] == [r.confidence for r in want]
    assert [r.prediction for r in got] == [r.prediction for r in want]
    assert all(np.array_equal(a.logits, b.logits) for a, b in zip(got, want))
    assert len({r.confidence for r in got}) > 8                  # the clips do not all score alike
    # at a threshold inside the confidences both decisions occur, and an exact hit counts as Positive on both sides
    thr = sorted(r.confidence for r in want)[20]
    got = ev.evaluate_waveforms(waves, threshold=thr, batch_size=16)
    ev2.model.at = 0
    want = ev2.evaluate_waveforms(waves, threshold=thr, batch_size=16)
    assert [r.prediction for r in got] == [r.prediction for r in want] and ev.last_counters == ev2.last_counters
    assert {r.prediction for r in got} == {"Positive", "Negative"}


def _trained_like(seed=0):
    from wakeword_trainer_home_amd.models import create_model
    model = create_model("cnn_small", dropout=0.3)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in Q.random_state(seed).items()}, strict=False)
    return model.to(DEV)


def test_export_writes_three_bundles_and_validates_them(tmp_path):
    from wakeword_trainer_home_amd.export import (ExportConfig, ModelExporter, load_exported_model, validate_exported_model)
    from wakeword_trainer_home_amd.export.reference import load_bundle, run_int8
    model = _trained_like()
    model.train()
    x = torch.from_numpy(Q.structured_features(24, 40, 151, seed=2)).to(DEV)
    exporter = ModelExporter(model, (1, 1, 40, 151), DEV, calibration=[x[:8], x[8:16]])
    model.train()
    res = exporter.export(ExportConfig(output_path=tmp_path / "sub" / "model.npz", quantize_fp16=True, quantize_int8=True))
    assert model.training, "the training state was not restored"
    assert res["success"] is True and "fp16_error" not in res and "int8_error" not in res, res
    assert set(res) == {"success", "path", "opset_version", "dynamic_batch", "file_size_mb", "fp16_path", "fp16_size_mb",
                        "fp16_reduction", "int8_path", "int8_size_mb", "int8_reduction"}
    assert res["fp16_path"].endswith("model_fp16.npz") and res["int8_path"].endswith("model_int8.npz")
    assert 20 < res["fp16_reduction"] < 50 and res["int8_reduction"] > res["fp16_reduction"]
    model.eval()
    with torch.no_grad():
        want = model(x)
        assert torch.equal(load_exported_model(res["path"], DEV)(x), want)
    diffs = {}
    for kind in ("path", "fp16_path", "int8_path"):
        v = validate_exported_model(res[kind], model, x, DEV)
        assert v["valid"] and v["error"] is None and v["inference_success"] and tuple(v["output_shape"]) == (24, 2), v
        assert np.isfinite(v["max_difference"]) and v["mean_difference"] <= v["max_difference"]
        assert v["numerically_equivalent"] == (v["max_difference"] < 1e-3)
        diffs[kind] = v["max_difference"]
    print(f"MEASURED max_difference: fp32 {diffs['path']:.4g}, fp16 {diffs['fp16_path']:.4g}, int8 {diffs['int8_path']:.4g} "
          f"(logits span {float(want.min()):.4g} .. {float(want.max()):.4g})")
    assert diffs["path"] == 0.0 and diffs["fp16_path"] > 0.0 and diffs["int8_path"] > 0.0
    # the calibration saw the fp32 model: its ranges are the float64 model's up to fp32 round-off
    header, arrays = load_bundle(res["int8_path"])
    _, ranges = Q.float_forward(Q.random_state(0), x[:16].cpu().numpy())
    cal = header["calibration"]
    assert cal["samples"] == 16 and cal["x_min"] == ranges["x_min"] and cal["x_max"] == ranges["x_max"]
    np.testing.assert_allclose(cal["a_max"] + [cal["p_max"]], ranges["a_max"] + [ranges["p_max"]], rtol=1e-4)
    # and the device runs that bundle as the interpreter does
    with torch.no_grad():
        got = load_exported_model(res["int8_path"], DEV)(x)
    _same(got, run_int8(header, arrays, x.cpu().numpy())["logits"], "exported int8 bundle")
    _same(got, Q.r_forward(arrays, x.cpu().numpy())["logits"], "exported int8 bundle, restated")


def test_int8_needs_calibration_and_cnn_small(tmp_path):
    from wakeword_trainer_home_amd.export import ExportConfig, ModelExporter
    from wakeword_trainer_home_amd.models import create_model
    res = ModelExporter(_trained_like(), (1, 1, 40, 151), DEV).export(
        ExportConfig(output_path=tmp_path / "a.npz", quantize_int8=True))
    assert res["success"] is True and "calibration" in res["int8_error"] and "int8_path" not in res
    torch.manual_seed(0)
    x = torch.randn(4, 1, 40, 38, device=DEV)
    res = ModelExporter(create_model("gru"), (1, 1, 40, 38), DEV, calibration=[x]).export(
        ExportConfig(output_path=tmp_path / "g.npz", quantize_int8=True, quantize_fp16=True))
    assert res["success"] is True and "cnn_small only" in res["int8_error"] and "int8_path" not in res
    assert (tmp_path / "g.npz").exists() and (tmp_path / "g_fp16.npz").exists() and not (tmp_path / "g_int8.npz").exists()


def test_non_finite_model_and_bad_directory_are_reported(tmp_path):
    from wakeword_trainer_home_amd.export import ExportConfig, ModelExporter
    model = _trained_like()
    with torch.no_grad():
        model.classifier.bias[0] = float("nan")
    res = ModelExporter(model, (1, 1, 40, 38), DEV).export(ExportConfig(output_path=tmp_path / "n.npz"))
    assert res == {"success": False, "error": "Model outputs contain NaN or Inf"}
    (tmp_path / "file").write_text("x")
    res = ModelExporter(_trained_like(), (1, 1, 40, 38), DEV).export(ExportConfig(output_path=tmp_path / "file" / "m.npz"))
    assert res["success"] is False and res["error"].startswith("Directory creation failed")


def test_benchmark_returns_its_keys(tmp_path, cases):
    from wakeword_trainer_home_amd.export import benchmark_exported_model
    from wakeword_trainer_home_amd.export.bundle import write_bundle
    header, arrays, x = cases[(2, 40, 38)][:3]
    path = write_bundle(tmp_path / "m_int8.npz", header, arrays)
    res = benchmark_exported_model(path, _trained_like(), torch.from_numpy(x), num_runs=5, device=DEV)
    assert set(res) == {"pytorch_time_ms", "exported_time_ms", "onnx_time_ms", "speedup", "num_runs"}
    assert res["pytorch_time_ms"] > 0 and res["exported_time_ms"] > 0 and res["onnx_time_ms"] == res["exported_time_ms"]
    assert res["num_runs"] == 5 and res["speedup"] == res["pytorch_time_ms"] / res["exported_time_ms"]


def test_export_model_reads_a_trainer_checkpoint(tmp_path):
    from wakeword_trainer_home_amd.config import get_preset
    from wakeword_trainer_home_amd.data import make_synthetic_batch
    from wakeword_trainer_home_amd.export import export_model, load_exported_model
    from wakeword_trainer_home_amd.models import create_model
    from wakeword_trainer_home_amd.training import Trainer
    cfg = get_preset("cnn_small_logmel40")
    cfg.training.epochs, cfg.optimizer.warmup_epochs, cfg.training.batch_size = 1, 0, 8
    cfg.optimizer.mixed_precision = False
    torch.manual_seed(3)
    wave, y = make_synthetic_batch(16, 24000, seed=5)
    y[::3] = 1
    batches = [(wave[i:i + 8], y[i:i + 8], [{"path": "s"}] * 8) for i in (0, 8)]
    t = Trainer(create_model("cnn_small", dropout=cfg.model.dropout), batches, batches[:1], cfg, checkpoint_dir=tmp_path, device=DEV)
    t.train()
    res = export_model(tmp_path / "best_model.pt", tmp_path / "out" / "ww.npz", quantize_int8=True, device=DEV,
                       calibration=[wave[:8], wave[8:]])                      # waveforms: they go through the front end
    assert res["success"] is True and "int8_error" not in res, res
    assert (res["architecture"], res["sample_rate"], res["duration"], res["input_shape"]) == \
        (cfg.model.architecture, cfg.data.sample_rate, cfg.data.audio_duration, (1, 1, 40, 151))
    feats = t._features(wave[:8], training=False)
    with torch.no_grad():
        assert torch.equal(load_exported_model(res["path"], DEV)(feats), t.model.eval()(feats))
        q = load_exported_model(res["int8_path"], DEV)(feats)
    assert q.shape == (8, 2) and torch.isfinite(q).all()
