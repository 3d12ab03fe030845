"""The int8 ResNet18 kernels and the ResNet18 half of the export package on the GPU.  Integer arithmetic is exact, so every
comparison with the restated law (tests/q8_resnet_cases.py) is bit for bit: no tolerance anywhere in this file but the
calibration's fp32-vs-fp64 check and the fp16 bundle's weight rounding."""
import json
import os
from pathlib import Path

import numpy as np
import pytest
import torch

from tests import q8_resnet_cases as RQ

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLDEN = Path(__file__).resolve().parent / "golden"
RELU, SIGNED, ADD = 0, 1, 2
# (B, H, W, Cin, Cout, k, stride) of the conv kernel alone: a 16-row tile that spans two images (15 rows each); 5x5 -> 3x3 at
# stride 2; the 1x1 downsample shape; a 1x1 image (only the centre tap is live); K = 9 x 256 = 2304 bytes a channel, a 144 KB
# channel tile, the largest the LDS form holds; and K = 9 x 512, a 288 KB tile, which is always streamed
CONV_SHAPES = [(2, 5, 3, 64, 64, 3, 1), (3, 5, 5, 64, 128, 3, 2), (3, 5, 5, 64, 128, 1, 2), (5, 1, 1, 128, 128, 3, 1),
               (2, 3, 3, 256, 256, 3, 1), (3, 2, 2, 512, 64, 3, 1)]


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _same(got, want, what):
    got = got.cpu().numpy()
    assert got.dtype == want.dtype and got.shape == want.shape, f"{what}: {got.dtype} {got.shape} vs {want.dtype} {want.shape}"
    bad = np.flatnonzero(got.reshape(-1) != want.reshape(-1))
    assert bad.size == 0, f"{what}: {bad.size} of {got.size} differ, first at {np.unravel_index(bad[0], got.shape)}"


@pytest.fixture(scope="module")
def cases():
    """name -> (header, arrays, x, restated stages, QuantizedResNet18 on the device); computed once, never modified."""
    from wakeword_trainer_home_amd.export import QuantizedResNet18
    out = {}
    for name in RQ.CASES:
        case = RQ.hard_case(name)
        out[name] = case + (QuantizedResNet18(case[0], case[1]).to(DEV),)
    return out


@pytest.fixture(scope="module")
def conv_cases():
    """Per CONV_SHAPES entry: random int8 input, weights and requantisation vectors (a tie channel and an all-zero channel among
    them), a residual tensor, and the restated law's output under each of the three epilogues."""
    out = []
    for i, (B, H, W, cin, cout, k, s) in enumerate(CONV_SHAPES):
        g = np.random.default_rng(100 + i)
        K = cin * k * k
        q = g.integers(-128, 128, (B, H, W, cin)).astype(np.int8)
        w = g.integers(-127, 128, (cout, cin, k, k)).astype(np.int8)
        b = g.integers(-20000, 20001, cout).astype(np.int32)
        m = g.integers(2 ** 30, 2 ** 31, cout).astype(np.int32)
        sh = np.full(cout, 31 + int(np.ceil(np.log2(1.0e4 * np.sqrt(K) / 400.0))), np.int32)
        w[5] = g.permutation(np.resize([1, -1, 0], K)).reshape(cin, k, k)
        b[5], m[5], sh[5] = 0, 2 ** 30, 31
        w[7] = 0
        z_in = -128 if i % 2 == 0 else 23                          # the fill of positions outside the image is the zero point
        acc = RQ.r_conv(q, z_in, w, b, s)
        r = RQ.r_R(acc, m, sh)
        res = g.integers(-128, 128, acc.shape).astype(np.int8)
        z_res, m_r, sh_r = (0, int(g.integers(2 ** 30, 2 ** 31)), 30) if i % 2 else (-128, int(g.integers(2 ** 30, 2 ** 31)), 31)
        total = r + RQ.r_R(res.astype(np.int64) - z_res, m_r, sh_r)
        want = {RELU: RQ.r_clamp(r), SIGNED: np.clip(r, -128, 127).astype(np.int8), ADD: RQ.r_clamp(total)}
        assert (r < -128).any() and (r > 255).any() and (total < 0).any() and (total > 255).any()
        tie = acc[..., 5]
        assert (tie % 2 == 1).any()
        wd = np.ascontiguousarray(w.transpose(0, 2, 3, 1).reshape(cout, k * k, cin))
        b_eff = (b.astype(np.int64) - z_in * w.astype(np.int64).reshape(cout, -1).sum(axis=1)).astype(np.int32)
        out.append(dict(q=q, w=wd, b=b_eff, m=m, sh=sh, k=k, s=s, z_in=z_in, res=res, z_res=z_res, m_r=m_r, sh_r=sh_r, want=want))
    return out


def _conv_alone(conv_cases):
    from wakeword_trainer_home_amd import _native as nat
    for i, c in enumerate(conv_cases):
        args = [_dev(c[key]) for key in ("q", "w", "b", "m", "sh")]
        for ep in (RELU, SIGNED, ADD):
            more = dict(residual=_dev(c["res"]), res_zero=c["z_res"], res_mult=c["m_r"], res_shift=c["sh_r"]) if ep == ADD else {}
            _same(nat.rq8_conv2d_fwd(*args, c["k"], c["s"], c["z_in"], ep, **more), c["want"][ep], f"conv shape {i} epilogue {ep}")


@pytest.fixture
def grid_cap():
    from wakeword_trainer_home_amd import _native as nat
    yield lambda n: nat.set_grid_cap(DEV, n)
    nat.set_grid_cap(DEV, 0)


def _layers(case):
    """Every layer kernel alone, each fed the restated law's own input tensor."""
    from wakeword_trainer_home_amd import _native as nat
    header, arrays, x, ref, model = case
    z_x = int(arrays["input_zero"][0])
    _same(nat.q8_quantize(_dev(x[:, 0]), arrays["input_scale"][0], z_x), ref["xq"], "quantize")
    _same(nat.rq8_stem_fwd(_dev(ref["xq"]), *model.conv("stem"), z_x), ref["stem"], "stem")
    _same(nat.rq8_maxpool_fwd(_dev(ref["stem"])), ref["pool0"], "pool0")
    prev = ref["pool0"]
    for name, _, _, stride, down in RQ.blocks():
        a_in = _dev(prev)
        _same(nat.rq8_conv2d_fwd(a_in, *model.conv(name + ".conv1"), 3, stride), ref[name + ".h1"], name + ".h1")
        res, z_res = a_in, -128
        if down:
            res, z_res = nat.rq8_conv2d_fwd(a_in, *model.conv(name + ".down"), 1, 2, -128, SIGNED), 0
            _same(res, ref[name + ".ds"], name + ".ds")
        out = nat.rq8_conv2d_fwd(_dev(ref[name + ".h1"]), *model.conv(name + ".conv2"), 3, 1, -128, ADD, residual=res, res_zero=z_res,
                                 res_mult=int(arrays[name + ".res.m"][0]), res_shift=int(arrays[name + ".res.sh"][0]))
        _same(out, ref[name + ".out"], name + ".out")
        prev = ref[name + ".out"]
    B, H, W, Cn = prev.shape
    pool, logits = nat.tq8_pool_fc_fwd(_dev(prev.reshape(B, H * W, Cn)), Cn, int(arrays["pool.m"][0]), int(arrays["pool.sh"][0]),
                                       model.fc_w, model.fc_b, model.fc_scale)
    _same(pool, ref["pool"], "pool")
    _same(logits, ref["logits"], "logits")


def _whole(case):
    """One forward; every stage tensor read back from the workspace."""
    from wakeword_trainer_home_amd import _native as nat
    header, arrays, x, ref, model = case
    B, F, T = x.shape[0], x.shape[2], x.shape[3]
    model._ws.clear()                                            # a fresh workspace: what is read below was written by this call
    with torch.no_grad():
        logits = model(_dev(x))
    _same(logits, ref["logits"], "logits")
    views = nat.rq8_workspace_views(model.workspace(B), B, F, T)
    assert list(views) == RQ.stages()[:-1]
    for stage in RQ.stages()[:-1]:
        _same(views[stage], ref[stage], stage)


def test_conv_kernel_alone_each_epilogue(conv_cases):
    _conv_alone(conv_cases)


def test_conv_entry_refuses_what_it_cannot_run(conv_cases):
    from wakeword_trainer_home_amd import _native as nat
    c = conv_cases[0]
    args = [_dev(c[key]) for key in ("q", "w", "b", "m", "sh")]
    with pytest.raises(ValueError):                              # 32 channels: not whole K chunks
        nat.rq8_conv2d_fwd(_dev(c["q"][..., :32]), _dev(c["w"][..., :32]), *args[2:], 3, 1)
    with pytest.raises(ValueError):                              # the add epilogue without its residual
        nat.rq8_conv2d_fwd(*args, 3, 1, -128, ADD)
    with pytest.raises(ValueError):                              # a residual multiplier below 2^30
        nat.rq8_conv2d_fwd(*args, 3, 1, -128, ADD, residual=_dev(c["res"]), res_zero=0, res_mult=5, res_shift=3)
    with pytest.raises(ValueError):                              # stride 3
        nat.rq8_conv2d_fwd(*args, 3, 3)


@pytest.mark.parametrize("name", ["odd", "tiny"])
def test_each_layer_kernel_alone(cases, name):
    _layers(cases[name])


@pytest.mark.parametrize("name", list(RQ.CASES))
def test_whole_model_every_tensor(cases, name):
    _whole(cases[name])
    _, _, x, ref, model = cases[name]
    assert ref["logits"].shape == (x.shape[0], RQ.CASES[name][3])
    with torch.no_grad():                                        # a batch slice: another base address (tiny: one that is not
        _same(model(_dev(x)[1:]), ref["logits"][1:], "batch slice")          # 16-byte aligned, so the module copies it)


def test_kernels_make_several_trips_under_a_grid_cap(cases, conv_cases, grid_cap):
    """One workgroup of four waves walks everything.  ``trips``: 1080 stage-1 rows are 68 16-row groups, 17 trips of the four
    waves per conv (the stem's 4080 pixels are 255 tiles, 64 trips); ``tiny``: three rows at the end, where
    three of the four waves have nothing to do."""
    grid_cap(1)
    for name in ("trips", "tiny"):
        _whole(cases[name])
    _layers(cases["tiny"])
    _conv_alone(conv_cases)
    for cap in (2, 3, 5, 8):         # the LDS form: a workgroup per channel tile where the grid reaches their number, else all tiles
        grid_cap(cap)
        _whole(cases["trips"])
        _whole(cases["tiny"])


@pytest.fixture
def forms():
    """Sets the environment switches of the conv launches that follow (weight form, row tile) and restores them."""
    old = {k: os.environ.get(k) for k in ("WW_RQ8_WEIGHTS", "WW_RQ8_ROWTILE")}

    def use(weights, rowtile):
        for k, v in (("WW_RQ8_WEIGHTS", weights), ("WW_RQ8_ROWTILE", rowtile)):
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    yield use
    for k, v in old.items():
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = v


def test_every_weight_form_and_row_tile_gives_the_same_bits(cases, conv_cases, grid_cap, forms):
    """Weights streamed through L2 or resident in LDS (wherever a channel tile fits, up to the 144 KB of the 256 -> 256 conv; the
    512-channel convs are streamed in every form), 16 or 64 rows a wave (every test shape takes 16 by default)."""
    for weights in ("stream", "lds", None):
        for rowtile in ("1", "4"):
            forms(weights, rowtile)
            grid_cap(0)
            _conv_alone(conv_cases)
            for name in ("odd", "tiny3"):
                _whole(cases[name])
            grid_cap(1)
            _whole(cases["trips"])
            _conv_alone(conv_cases)


# ------------------------------------------------------------------ the export package
F_, T_ = 40, 33


def _golden():
    z = np.load(GOLDEN / "g15_q8_resnet18.npz")
    rec = json.loads((GOLDEN / "q8_resnet18_errors.json").read_text())["ResNet18Wakeword"]
    return z, rec, RQ.random_state(2, seed=int(z["param_seed"]), gain=float(z["gain"]))


def _model_of(state, num_classes=2):
    from wakeword_trainer_home_amd.models import ResNet18Wakeword
    model = ResNet18Wakeword(num_classes=num_classes)
    model.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in state.items()})
    return model.to(DEV)


def _cal_rtol(rec):
    """The existing tests' 1e-4, unless float32 CPU torch's own calibration of this model is further than half of that from
    float64 (recorded by the fixture's generator): then twice that figure."""
    return 1e-4 if rec["calibration_fp32_rel"] <= 0.5e-4 else 2 * rec["calibration_fp32_rel"]


def test_export_writes_three_bundles_and_loads_them(tmp_path):
    from wakeword_trainer_home_amd.export import (ExportConfig, ModelExporter, QuantizedResNet18, load_exported_model,
                                                  validate_exported_model)
    from wakeword_trainer_home_amd.export.reference import load_bundle, run_int8
    z, rec, state = _golden()
    model = _model_of(state)
    xs = z["x"].astype(np.float32)
    x = torch.from_numpy(xs).to(DEV)
    exporter = ModelExporter(model, (1, 1, F_, T_), DEV, calibration=[x[:5], x[5:8]])
    model.train()                                                # (the exporter's constructor puts the model in eval mode)
    res = exporter.export(ExportConfig(output_path=tmp_path / "sub" / "rn.npz", quantize_fp16=True, quantize_int8=True))
    assert model.training, "the training state was not restored"
    assert res["success"] is True and "fp16_error" not in res and "int8_error" not in res, res
    assert res["fp16_path"].endswith("rn_fp16.npz") and res["int8_path"].endswith("rn_int8.npz")
    assert res["int8_reduction"] > res["fp16_reduction"] > 20
    model.eval()
    with torch.no_grad():
        want = model(x)
    for kind in ("path", "fp16_path", "int8_path"):
        header, _ = load_bundle(res[kind])
        assert header["architecture"] == "ResNet18Wakeword"
        v = validate_exported_model(res[kind], model, x, DEV)
        assert v["valid"] and v["error"] is None and v["inference_success"] and tuple(v["output_shape"]) == (16, 2), v
    # fp32: the stored state in the same class -- the same logits exactly
    with torch.no_grad():
        loaded = load_exported_model(res["path"], DEV)
        assert type(loaded).__name__ == "ResNet18Wakeword" and not loaded.training
        assert torch.equal(loaded(x), want)
        got16 = load_exported_model(res["fp16_path"], DEV)(x).cpu().numpy().astype(np.float64)
        q8 = load_exported_model(res["int8_path"], DEV)
        got8 = q8(x)
    # fp16: what rounding every weight to fp16 does to the float64 model, up to the fp32 round-off of the device forward.  That
    # round-off: products of K <= 4608 terms accumulated in fp32 through twenty layers; the bound allows 2e-4 of the largest logit
    # (at least of 1).
    state16 = {k: (v if v.dtype == np.int64 else v.astype(np.float16).astype(np.float32)) for k, v in state.items()}
    f64 = z["logits"]
    f64_16, _ = RQ.float_forward(state16, xs)
    slack = 2e-4 * max(1.0, float(np.abs(f64).max()))
    d16 = np.abs(got16 - want.cpu().numpy().astype(np.float64)).max()
    print(f"MEASURED fp16 bundle vs fp32 model {d16:.4g}; float64 model under fp16 weights {np.abs(f64_16 - f64).max():.4g}; "
          f"device vs float64 under fp16 weights {np.abs(got16 - f64_16).max():.4g} (slack {slack:.4g}); "
          f"fp32 device vs float64 {np.abs(want.cpu().numpy() - f64).max():.4g}")
    assert np.abs(want.cpu().numpy().astype(np.float64) - f64).max() <= slack     # the float bundle reproduces the model
    assert np.abs(got16 - f64_16).max() <= slack
    assert 0.0 < d16 <= np.abs(f64_16 - f64).max() + 2 * slack
    # int8: the device runs the bundle as the interpreter and the restated law do
    assert isinstance(q8, QuantizedResNet18)
    header, arrays = load_bundle(res["int8_path"])
    _same(got8, run_int8(header, arrays, xs)["logits"], "exported int8 bundle")
    _same(got8, RQ.r_forward(arrays, xs)["logits"], "exported int8 bundle, restated")
    want_arrays = RQ.r_quantize_model(state, (F_, T_), header["calibration"])
    assert sorted(arrays) == sorted(want_arrays) and all(np.array_equal(arrays[k], want_arrays[k]) for k in want_arrays)
    # the calibration saw the fp32 model: its ranges are the float64 model's (the fixture's) up to fp32 round-off
    cal = header["calibration"]
    assert cal["samples"] == 8 and cal["x_min"] == float(z["x_min"]) and cal["x_max"] == float(z["x_max"])
    rel = np.abs(np.array(RQ.flat_ranges(cal)) - z["a_max"]) / z["a_max"]
    print(f"MEASURED calibration on the device vs float64: max relative difference {rel.max():.4g} (rtol {_cal_rtol(rec):.4g})")
    np.testing.assert_allclose(RQ.flat_ranges(cal), z["a_max"], rtol=_cal_rtol(rec))


def test_calibrate_resnet18_equals_the_restated_ranges():
    from wakeword_trainer_home_amd.export import calibrate_resnet18
    from wakeword_trainer_home_amd.export.quantize import QuantizationError
    z, rec, _ = _golden()
    state = RQ.random_state(3, seed=5, gain=0.8)
    model = _model_of(state, 3).eval()
    xs = z["x"].astype(np.float32)[:6]
    x = torch.from_numpy(xs).to(DEV)
    cal = calibrate_resnet18(model, [x[:4], x[4:, 0]], (F_, T_), DEV)        # a (B,F,T) batch is taken as well
    _, ranges = RQ.float_forward(state, xs)
    assert cal["samples"] == 6 and cal["x_min"] == ranges["x_min"] and cal["x_max"] == ranges["x_max"]
    assert (len(cal["h1_max"]), len(cal["ds_max"]), len(cal["out_max"])) == (8, 3, 8)
    np.testing.assert_allclose(RQ.flat_ranges(cal), RQ.flat_ranges(ranges), rtol=_cal_rtol(rec))
    with pytest.raises(QuantizationError, match="empty"):
        calibrate_resnet18(model, [], (F_, T_), DEV)
    with pytest.raises(QuantizationError, match="expected"):
        calibrate_resnet18(model, [x[:, :, :, :32]], (F_, T_), DEV)


def test_int8_resnet18_needs_calibration(tmp_path):
    from wakeword_trainer_home_amd.export import ExportConfig, ModelExporter
    from wakeword_trainer_home_amd.models import ResNet18Wakeword
    torch.manual_seed(0)
    res = ModelExporter(ResNet18Wakeword(), (1, 1, F_, T_), DEV).export(ExportConfig(output_path=tmp_path / "a.npz", quantize_int8=True))
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


def test_evaluator_and_scanner_score_the_int8_resnet18_as_the_restated_law(tmp_path, cases):
    """Clips of 5120 samples are 33 frames, the ``odd`` bundle's T.  The evaluator and the scanner on the loaded int8 bundle
    against the same tools replaying the restated law's logits of the very features the model was given."""
    from wakeword_trainer_home_amd.data import make_synthetic_batch
    from wakeword_trainer_home_amd.evaluation import ModelEvaluator, RecordingScanner
    from wakeword_trainer_home_amd.export import load_exported_model
    from wakeword_trainer_home_amd.export.bundle import write_bundle
    header, arrays = cases["odd"][:2]
    n, dur = 5120, 5120 / 16000
    spy = _Spy(load_exported_model(write_bundle(tmp_path / "r_int8.npz", header, arrays), DEV))
    waves, _ = make_synthetic_batch(13, n, seed=11)
    ev = ModelEvaluator(spy, sample_rate=16000, audio_duration=dur, device=DEV, n_mels=40)
    got = ev.evaluate_waveforms(waves, threshold=0.5, batch_size=8)
    counters = dict(ev.last_counters)
    feats = np.concatenate(spy.seen)
    assert feats.shape == (13, 1, 40, 33)
    want_logits = torch.from_numpy(RQ.r_forward(arrays, feats)["logits"]).to(DEV)
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
    audio = (rng.normal(0, 0.1, S) * np.repeat(rng.choice([0.01, 0.3, 1.0, 3.0], S // 640), 640)).astype(np.float32)
    spy.seen.clear()
    kw = dict(sample_rate=16000, audio_duration=dur, threshold=0.5, device=DEV, n_mels=40, batch_size=4)
    scanner = RecordingScanner(spy, **kw)
    W = scanner.num_windows(S)
    assert W == 6
    got = scanner.scan(audio)
    feats = np.concatenate(spy.seen)
    assert feats.shape == (W, 1, 40, 33)
    want_logits = torch.from_numpy(RQ.r_forward(arrays, feats)["logits"]).to(DEV)
    want = RecordingScanner(_Replay(want_logits), **kw).scan(audio)
    assert len(got) == W and got == want and len({c for c, _ in got}) > 1
