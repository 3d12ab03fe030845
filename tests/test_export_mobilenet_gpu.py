"""The int8 MobileNetV3 kernels and the MobileNetV3 half of the export package on the GPU.  Integer arithmetic is exact, so every
comparison with the restated law (tests/q8_mobilenet_cases.py) is bit for bit: no tolerance anywhere in this file but the
calibration's fp32-vs-fp64 check."""
import numpy as np
import pytest
import torch

from tests import q8_mobilenet_cases as MQ

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LAYER_CASES = ("hard_tiny", "hard_odd", "tiny")
# measured: the largest deviation of a device-calibrated range from its float64 recomputation is 3.3e-6 where the largest magnitude
# among the ranges is 27.4, relative 1.2e-7 (one MI355X; fp32 sums of at most 576 terms per output); the bound is twice that
CALIBRATION_REL = 2.4e-7


@pytest.fixture(scope="module")
def cases():
    """name -> (header, arrays, x, restated tensors, QuantizedMobileNetV3 on the device); computed once, never modified."""
    from wakeword_trainer_home_amd.export import QuantizedMobileNetV3
    return {name: MQ.case(name) + (QuantizedMobileNetV3(*MQ.case(name)[:2]).to(DEV),) for name in MQ.CASES}


@pytest.fixture
def grid_cap():
    from wakeword_trainer_home_amd import _native as nat
    yield lambda n: nat.set_grid_cap(DEV, n)
    nat.set_grid_cap(DEV, 0)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _pad(q, fill):
    """(..., C) -> the device layout (..., Cp), the pad channels holding the tensor's zero point."""
    C = q.shape[-1]
    out = np.full(q.shape[:-1] + ((C + 63) // 64 * 64,), fill, q.dtype)
    out[..., :C] = q
    return out


def _same(got, want, fill=None, what=""):
    """``got`` (device, padded) equals ``want`` on the real channels, and holds ``fill`` in the pad channels."""
    got = got.cpu().numpy()
    C = want.shape[-1]
    assert got.shape[:-1] == want.shape[:-1] and np.array_equal(got[..., :C], want), what
    if fill is not None:
        assert (got[..., C:] == fill).all(), what + ": pad channels"


def _zeros(arrays, F, T):
    """{stage name: zero point} of every int8 stage tensor."""
    z = {"xq": int(arrays["input_zero"][0]), "stem": int(arrays["stem.zo"][0]), "last": int(arrays["last.zo"][0])}
    for i, b in enumerate(MQ.blocks(F, T)):
        p = f"b{i}."
        for layer in ("expand", "dw"):
            z[p + layer] = int(arrays[p + layer + ".zo"][0]) if b["hs"] and p + layer + ".zo" in arrays else -128
        z[p + "pool"] = z[p + "y"] = z[p + "dw"]
        z[p + "h"], z[p + "out"] = -128, 0
    z["pool"], z["hidden"] = z["last"], int(arrays["cls0.zo"][0])
    return z


# ------------------------------------------------------------------ the layer entry points
@pytest.mark.parametrize("name", LAYER_CASES)
def test_conv1x1_epilogues(cases, name):
    from wakeword_trainer_home_amd import _native as nat
    header, arrays, x, ref, net = cases[name]
    F, T = header["feature_shape"]
    z = _zeros(arrays, F, T)
    seen = set()
    for i, b in enumerate(MQ.blocks(F, T)):
        p = f"b{i}."
        src = "stem" if i == 0 else f"b{i - 1}.out"
        if b["expand"]:
            w, bias, m, sh, tab = net.conv(p + "expand")
            ep, zu = (nat.MQ8_HSWISH, int(arrays[p + "expand.zu"][0])) if b["hs"] else (nat.MQ8_RELU, 0)
            got = nat.mq8_conv1x1_fwd(_dev(_pad(ref[src], z[src])), w, bias, m, sh, z[src], ep, zu, tab)
            _same(got, ref[p + "expand"], z[p + "expand"], p + "expand")
            seen.add(ep)
        a_in = p + ("y" if b["se"] else "dw")
        w, bias, m, sh, _ = net.conv(p + "project")
        res = _dev(_pad(ref[src], 0)) if b["res"] else None
        rm, rs = (int(arrays[p + "res.m"][0]), int(arrays[p + "res.sh"][0])) if b["res"] else (0, 0)
        got = nat.mq8_conv1x1_fwd(_dev(_pad(ref[a_in], z[a_in])), w, bias, m, sh, z[a_in], nat.MQ8_SIGNED, residual=res, res_mult=rm,
                                  res_shift=rs)
        _same(got, ref[p + "out"], 0, p + "project")
        seen.add((nat.MQ8_SIGNED, b["res"]))
    w, bias, m, sh, tab = net.conv("last")
    got = nat.mq8_conv1x1_fwd(_dev(_pad(ref["b10.out"], 0)), w, bias, m, sh, 0, nat.MQ8_HSWISH, int(arrays["last.zu"][0]), tab)
    _same(got, ref["last"], None, "last")
    assert seen == {nat.MQ8_RELU, nat.MQ8_HSWISH, (nat.MQ8_SIGNED, False), (nat.MQ8_SIGNED, True)}


@pytest.mark.parametrize("name", LAYER_CASES)
def test_depthwise_in_its_four_forms_and_the_stem(cases, name):
    from wakeword_trainer_home_amd import _native as nat
    header, arrays, x, ref, net = cases[name]
    F, T = header["feature_shape"]
    z = _zeros(arrays, F, T)
    w, bias, m, sh, tab = net.conv("stem")
    got = nat.mq8_stem_fwd(_dev(ref["xq"]), w, bias, m, sh, z["xq"], int(arrays["stem.zu"][0]), tab)
    _same(got, ref["stem"], z["stem"], "stem")
    forms = set()
    for i, b in enumerate(MQ.blocks(F, T)):
        p = f"b{i}."
        src = p + "expand" if b["expand"] else "stem"
        w, bias, m, sh, tab = net.conv(p + "dw")
        ep, zu = (nat.MQ8_HSWISH, int(arrays[p + "dw.zu"][0])) if b["hs"] else (nat.MQ8_RELU, 0)
        got = nat.mq8_dwconv_fwd(_dev(_pad(ref[src], z[src])), w, bias, m, sh, b["k"], b["stride"], z[src], ep, zu, tab)
        _same(got, ref[p + "dw"], z[p + "dw"], p + "dw")
        forms.add((b["k"], b["stride"]))
    assert forms == {(3, 1), (3, 2), (5, 1), (5, 2)}


@pytest.mark.parametrize("k,stride,H,W,C,hs", [(5, 2, 1, 1, 40, True), (5, 2, 2, 3, 24, True), (5, 1, 2, 3, 88, False), (3, 2, 5, 7, 16, False),
                                               (3, 1, 3, 3, 72, True), (5, 2, 9, 11, 40, False), (3, 2, 1, 1, 16, True)])
def test_depthwise_on_synthetic_layers(k, stride, H, W, C, hs):
    """Windows larger than the image (5x5 stride 2 on 1x1 and 2x3), every channel count of the model below 96, both epilogues."""
    from wakeword_trainer_home_amd import _native as nat
    q, z, a, want = MQ.dw_layer_case(k, stride, H, W, C, hs, seed=k * 100 + H)
    Cp = (C + 63) // 64 * 64
    w = np.zeros((k * k, Cp), np.int8)
    w[:, :C] = a["dw.w"].T
    bias, m, sh = np.zeros(Cp, np.int32), np.full(Cp, 2 ** 30, np.int32), np.full(Cp, 31, np.int32)
    bias[:C] = (a["dw.b"].astype(np.int64) - z * a["dw.w"].astype(np.int64).sum(axis=1)).astype(np.int32)
    m[:C], sh[:C] = a["dw.m"], a["dw.sh"]
    ep, zu, tab = (nat.MQ8_HSWISH, int(a["dw.zu"][0]), _dev(a["dw.tab"])) if hs else (nat.MQ8_RELU, 0, None)
    got = nat.mq8_dwconv_fwd(_dev(_pad(q, z)), _dev(w), _dev(bias), _dev(m), _dev(sh), k, stride, z, ep, zu, tab)
    _same(got, want, None, f"dw {k}x{k} s{stride} on {H}x{W}x{C}")
    if H * W * C > 500:
        assert want.min() == -128 and want.max() == 127


@pytest.mark.parametrize("name", LAYER_CASES)
def test_squeeze_excitation_gate_pass_and_head(cases, name):
    from wakeword_trainer_home_amd import _native as nat
    header, arrays, x, ref, net = cases[name]
    F, T = header["feature_shape"]
    z = _zeros(arrays, F, T)
    one = lambda key: int(arrays[key][0])        # noqa: E731
    for i, b in enumerate(MQ.blocks(F, T)):
        if not b["se"]:
            continue
        p = f"b{i}."
        a = _dev(_pad(ref[p + "dw"], z[p + "dw"]))
        pool, h, gate = nat.mq8_se_fwd(a, b["exp"], z[p + "dw"], one(p + "pool.m"), one(p + "pool.sh"), net.conv(p + "fc1")[:4],
                                       net.conv(p + "fc2")[:4])
        _same(pool, ref[p + "pool"], z[p + "dw"], p + "pool")
        _same(h, ref[p + "h"], None, p + "h")
        _same(gate, ref[p + "gate"], 0, p + "gate")
        y = nat.mq8_gate_fwd(a, _dev(_pad(ref[p + "gate"], 0)), z[p + "dw"], one(p + "gate.m"), one(p + "gate.sh"))
        _same(y, ref[p + "y"], z[p + "dw"], p + "y")
    pool, hidden, logits = nat.mq8_head_fwd(_dev(ref["last"]), z["last"], one("pool.m"), one("pool.sh"), net.conv("cls0")[:4], one("cls0.zu"),
                                            net.conv("cls0")[4], z["hidden"], net.fc_w, net.fc_b, net.fc_scale)
    _same(pool, ref["pool"], None, "pool")
    _same(hidden, ref["hidden"], None, "hidden")
    assert np.array_equal(logits.cpu().numpy(), ref["logits"])


# ------------------------------------------------------------------ the whole forward
def _check_forward(case, x=None, ref=None, skip=()):
    from wakeword_trainer_home_amd import _native as nat
    header, arrays, x0, ref0, net = case
    x, ref = (x0, ref0) if x is None else (x, ref)
    F, T = header["feature_shape"]
    z = _zeros(arrays, F, T)
    with torch.no_grad():
        logits = net(_dev(x))
    assert np.array_equal(logits.cpu().numpy(), ref["logits"])
    views = nat.mq8_workspace_views(net.workspace(x.shape[0]), x.shape[0], F, T)
    assert list(views) == [s for s in MQ.stages() if s != "logits"]
    for stage, t in views.items():
        if skip and stage.endswith(skip):
            continue
        _same(t, ref[stage], 0 if stage.endswith("gate") else (z[stage] if stage != "xq" else None), stage)


@pytest.mark.parametrize("name", [n for n in MQ.CASES if n != "trips"])
def test_forward_gives_every_workspace_tensor_and_the_logits(cases, name):
    _check_forward(cases[name])


def test_kernels_make_several_trips_under_a_grid_cap(cases, grid_cap):
    for cap in (1, 2, 0):
        grid_cap(cap)
        _check_forward(cases["trips"])


def test_workspace_reuse_and_another_batch_size(cases):
    header, arrays, x, ref, net = cases["hard_tiny"]
    F, T = header["feature_shape"]
    _check_forward(cases["hard_tiny"])
    first = net.workspace(x.shape[0])
    _check_forward(cases["hard_tiny"])                                   # a second forward on the same module and workspace
    assert net.workspace(x.shape[0]) is first
    x2 = np.concatenate([x[1:], x[:1], x[2:]])                           # another batch size (4), another order
    _check_forward(cases["hard_tiny"], x2, MQ.r_forward(arrays, x2, F, T))
    _check_forward(cases["hard_tiny"])                                   # ... and the first size again
    assert set(net._ws) == {3, 4}


def test_fused_gate_form_equals_the_pass_form(cases, grid_cap, monkeypatch):
    """The projection conv that gates its own pixel fragments gives the bits of the gate pass followed by the plain conv: per layer,
    and through the whole forward, which then neither writes nor reads the y tensors."""
    from wakeword_trainer_home_amd import _native as nat
    for name in LAYER_CASES:
        header, arrays, x, ref, net = cases[name]
        F, T = header["feature_shape"]
        z = _zeros(arrays, F, T)
        for i, b in enumerate(MQ.blocks(F, T)):
            if not b["se"]:
                continue
            p, src = f"b{i}.", "stem" if i == 0 else f"b{i - 1}.out"
            w, bias, m, sh, _ = net.conv(p + "project")
            res = _dev(_pad(ref[src], 0)) if b["res"] else None
            rm, rs = (int(arrays[p + "res.m"][0]), int(arrays[p + "res.sh"][0])) if b["res"] else (0, 0)
            got = nat.mq8_conv1x1_fwd(_dev(_pad(ref[p + "dw"], z[p + "dw"])), w, bias, m, sh, z[p + "dw"], nat.MQ8_SIGNED, residual=res,
                                      res_mult=rm, res_shift=rs, gate=_dev(_pad(ref[p + "gate"], 0)), gate_mult=int(arrays[p + "gate.m"][0]),
                                      gate_shift=int(arrays[p + "gate.sh"][0]))
            _same(got, ref[p + "out"], 0, p + "project, fused")
    for name, cap in (("hard_tiny", 0), ("hard_odd", 0), ("tiny", 0), ("trips", 1), ("trips", 0)):
        header, arrays, x, ref, net = cases[name]
        F, T = header["feature_shape"]
        grid_cap(cap)
        monkeypatch.setenv("WW_MQ8_GATE", "pass")
        _check_forward(cases[name])
        ys = [v for k, v in nat.mq8_workspace_views(net.workspace(x.shape[0]), x.shape[0], F, T).items() if k.endswith(".y")]
        for y in ys:
            y.fill_(55)
        monkeypatch.setenv("WW_MQ8_GATE", "fused")
        _check_forward(cases[name], skip=(".y",))
        assert len(ys) == 9 and all(bool((y == 55).all()) for y in ys)       # neither written ...
        for y in ys:
            y.fill_(-77)
        _check_forward(cases[name], skip=(".y",))                            # ... nor read


@pytest.mark.parametrize("form", ["relu", "gated"])
def test_conv1x1_rows_past_the_end_on_a_second_trip(grid_cap, form):
    """64 -> 64 channels over 14 images of 5 pixels, one workgroup: 70 rows are five 16-row tiles for four waves, so one wave makes
    a second trip, to the tile whose last ten rows lie past the end; 5 pixels an image, so every tile spans images and the gated
    form reads up to four gate rows in one tile.  (The model cases reach the ReLU epilogue under a grid cap with whole tiles only.)"""
    from wakeword_trainer_home_amd import _native as nat
    g = np.random.default_rng(7)
    B, HW, C, z = 14, 5, 64, 23
    q = g.integers(-128, 128, (B, 1, HW, C)).astype(np.int8)
    w = g.integers(-127, 128, (C, C)).astype(np.int8)
    b = g.integers(-20000, 20001, C).astype(np.int32)
    m = g.integers(2 ** 30, 2 ** 31, C).astype(np.int32)
    sh = np.full(C, 39, np.int32)                                        # |acc| < 2^21.1 and m / 2^39 > 2^-9: r leaves [-128, 255] both ways
    b_eff = (b.astype(np.int64) - z * w.astype(np.int64).sum(axis=1)).astype(np.int32)
    args = [_dev(v) for v in (w, b_eff, m, sh)]
    grid_cap(1)
    if form == "relu":
        want = MQ.r_clamp(MQ.r_R(MQ.r_matmul(q, z, w) + b, m, sh) - 128)
        got = nat.mq8_conv1x1_fwd(_dev(q), *args, z, nat.MQ8_RELU)
    else:
        gate = g.integers(0, 256, (B, C)).astype(np.uint8)
        gm, gsh = int(g.integers(2 ** 30, 2 ** 31)), 38                  # G / 255 is about R(G, 2^30 .. 2^31, 38)
        y = MQ.r_clamp(z + MQ.r_R((q.astype(np.int64) - z) * gate[:, None, None, :], gm, gsh))
        want = MQ.r_clamp(MQ.r_R(MQ.r_matmul(y, z, w) + b, m, sh))
        got = nat.mq8_conv1x1_fwd(_dev(q), *args, z, nat.MQ8_SIGNED, gate=_dev(gate), gate_mult=gm, gate_shift=gsh)
    assert want.min() == -128 and want.max() == 127
    _same(got, want, None, form)


# ------------------------------------------------------------------ the export package
def _model(num_classes=2, seed=0):
    from wakeword_trainer_home_amd.models import create_model
    torch.manual_seed(seed)
    model = create_model("mobilenetv3", num_classes=num_classes, pretrained=False)
    state = {k: torch.from_numpy(np.asarray(v)) for k, v in MQ.random_state(num_classes, seed).items()}
    model.load_state_dict(state)                                         # (the seeded state carries non-trivial running statistics)
    return model.to(DEV).eval()


def test_export_load_validate_and_evaluate(tmp_path):
    from wakeword_trainer_home_amd.data import make_synthetic_batch
    from wakeword_trainer_home_amd.evaluation import ModelEvaluator
    from wakeword_trainer_home_amd.export import (ExportConfig, ModelExporter, QuantizedMobileNetV3, load_exported_model,
                                                  validate_exported_model)
    from wakeword_trainer_home_amd.export.reference import load_bundle, run_int8
    F, T = 40, 45
    model = _model()
    x = torch.from_numpy(MQ.structured_features(8, F, T, seed=3)).to(DEV)
    exporter = ModelExporter(model, (1, 1, F, T), DEV, calibration=[x[:4], x[4:]])
    model.train()
    res = exporter.export(ExportConfig(output_path=tmp_path / "sub" / "mb.npz", quantize_fp16=True, quantize_int8=True))
    assert model.training, "the training state was not restored"
    assert res["success"] is True and "fp16_error" not in res and "int8_error" not in res, res
    assert res["fp16_path"].endswith("mb_fp16.npz") and res["int8_path"].endswith("mb_int8.npz")
    assert res["int8_reduction"] > 65 > res["fp16_reduction"] > 45            # about a quarter and a half of the fp32 bundle
    model.eval()
    net = load_exported_model(res["int8_path"], DEV)
    assert isinstance(net, QuantizedMobileNetV3) and net.feature_shape == (F, T)
    header, arrays = load_bundle(res["int8_path"])
    assert header["architecture"] == "mobilenetv3" and header["calibration"]["samples"] == 8
    with torch.no_grad():
        got = net(x).cpu().numpy()
    assert np.array_equal(got, run_int8(header, arrays, x.cpu().numpy())["logits"])
    assert np.array_equal(got, MQ.r_forward(arrays, x.cpu().numpy(), F, T)["logits"])
    for key in ("path", "fp16_path", "int8_path"):
        v = validate_exported_model(res[key], model, x, DEV)
        assert v["valid"] is True and v["error"] is None and v["inference_success"] and v["output_shape"] == (8, 2), (key, v)
        print(key, "max_difference", v["max_difference"])
    # without calibration data: the existing refusal
    res = ModelExporter(model, (1, 1, F, T), DEV).export(ExportConfig(output_path=tmp_path / "a.npz", quantize_int8=True))
    assert res["success"] is True and "calibration" in res["int8_error"] and "int8_path" not in res
    # ModelEvaluator scores the int8 module as it scores any other
    n = 7040
    waves, _ = make_synthetic_batch(9, n, seed=11)
    ev = ModelEvaluator(net, sample_rate=16000, audio_duration=n / 16000, device=DEV, n_mels=F)
    out = ev.evaluate_waveforms(waves, threshold=0.5, batch_size=4)
    assert len(out) == 9 and ev.last_counters["count"] == 9 and all(np.isfinite(r.confidence) for r in out)


def test_device_calibration_agrees_with_the_float64_walk():
    from wakeword_trainer_home_amd.export import calibrate_mobilenetv3
    F, T = 16, 24
    model = _model(seed=1)
    x = MQ.structured_features(6, F, T, seed=5)
    got = calibrate_mobilenetv3(model, [torch.from_numpy(x[:3]), torch.from_numpy(x[3:])], (F, T), DEV)
    want, _ = MQ.float_walk(MQ.random_state(2, 1), x)
    assert got["samples"] == 6 and list(got["ranges"]) == MQ.range_names()
    top = max(abs(v) for r in want["ranges"].values() for v in r)
    dev = max(abs(g - w) for n in MQ.range_names() for g, w in zip(got["ranges"][n], want["ranges"][n]))
    print(f"largest range deviation {dev:.3g} of {top:.3g}: relative {dev / top:.3g}")
    assert (got["x_min"], got["x_max"]) == (want["x_min"], want["x_max"])
    assert dev <= CALIBRATION_REL * top
