"""No GPU: the weighted-loss layers above the kernel -- the float64 restatement against the reference's recorded numbers
(tests/golden/g9_weighted_loss.npz), the constructors of the three loss classes, the C ABI's new name, and the helpers that
carry class weights from a clip bank's labels to the Trainer."""
import ctypes
import re
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import weighted_loss_cases as WC

REPO = Path(__file__).resolve().parents[1]
GOLDEN = REPO / "tests" / "golden"
G9 = WC.load_g9(GOLDEN)


def test_g9_covers_what_it_should():
    names = {c["name"] for c in G9}
    for ln in WC.LOSSES:
        for red in ("mean", "sum", "none"):
            assert {f"{ln}|{red}|{wn}|B65" for wn in WC.WEIGHTS} <= names
            assert {f"{ln}|{red}|w0.55-5|B{B}" for B in (1, 3)} <= names
        assert f"{ln}|mean|w0.55-5|big8" in names
    big = next(c for c in G9 if c["name"].endswith("big8"))
    assert np.abs(big["z"]).max() == 88.0


@pytest.mark.parametrize("case", G9, ids=lambda c: c["name"])
def test_restatement_matches_the_reference_recorded_numbers(case):
    """1e-6 of the case's largest value, loss and gradient: the reference computes in fp32, a few 1e-7 from float64.  The
    divisor is ``divisor_of``'s: dividing the eps == 0 mean by B, or the others by the weights' sum, is off by O(1) here."""
    kind, hyper = WC.LOSSES[case["loss_name"]]
    loss, grad = WC.weighted_loss(kind, case["z"], case["y"], case["weight"], case["reduction"], WC.divisor_of(case["loss_name"]),
                                  case["upstream"], **hyper)
    assert np.abs(loss - case["loss"]).max() <= 1e-6 * np.abs(loss).max(), case["name"]
    assert np.abs(grad - case["grad"]).max() <= 1e-6 * np.abs(grad).max(), case["name"]


def test_the_two_divisors_are_far_apart_on_the_fixture():
    """What the divisor test is for: under (0.55, 5.0) at B = 65 the two 'mean' rules differ by far more than any tolerance, and
    the recorded nn.CrossEntropyLoss value sides with the weights' sum."""
    case = next(c for c in G9 if c["name"] == "ce0|mean|w0.55-5|B65")
    by_w, _ = WC.weighted_loss("ce", case["z"], case["y"], case["weight"], "mean", "weight_sum")
    by_b, _ = WC.weighted_loss("ce", case["z"], case["y"], case["weight"], "mean", "batch")
    assert abs(by_w - by_b) > 0.1 * abs(by_w)
    assert abs(by_w - case["loss"]) < 1e-6 * abs(by_w) < abs(by_b - case["loss"])


def test_fp32_formulation_agrees_with_the_restatement():
    """The error measure of the GPU tests is sound: the fp32 CPU formulation sits within 2e-6 of the restatement in every mode."""
    z, y = WC.batch(65)
    up = np.random.default_rng(5).normal(size=65).astype(np.float32)
    for ln, (kind, hyper) in WC.LOSSES.items():
        for red, div in (("mean", "batch"), ("mean", "weight_sum"), ("sum", "batch"), ("none", "batch")):
            u = up if red == "none" else None
            ref = WC.weighted_loss(kind, z, y, np.float32([0.55, 5.0]), red, div, u, **hyper)
            got = WC.torch32(kind, z, y, np.float32([0.55, 5.0]), red, div, u, **hyper)
            for a, b in zip(got, ref):
                assert np.abs(a - b).max() <= 2e-6 * np.abs(b).max(), (ln, red, div)


# --------------------------------------------------------------------------- constructors
def _classes():
    from wakeword_trainer_home_amd.models import losses as L
    return L, [(L.CrossEntropyLoss, {}), (L.LabelSmoothingCrossEntropy, dict(smoothing=0.1)), (L.FocalLoss, dict(alpha=0.25, gamma=2.0))]


def test_weights_and_reductions_are_accepted_by_all_three_classes():
    from wakeword_trainer_home_amd import _native as nat
    L, classes = _classes()
    w = torch.tensor([0.55, 5.0])
    for cls, kw in classes:
        for red in ("mean", "sum", "none"):
            c = cls(weight=w, reduction=red, **kw)
            assert c.reduction == red and torch.equal(c.weight, w)
            assert c.weight is not w                                        # its own copy, registered as a buffer
            assert "weight" in dict(c.named_buffers()) and "weight" in c.state_dict()
            assert c.to("cpu").weight.device.type == "cpu" and c.to(torch.device("meta")).weight.device.type == "meta"
        plain = cls(**kw)
        assert plain.weight is None and plain.reduction == "mean" and not dict(plain.named_buffers())
    assert L.CrossEntropyLoss._divisor == nat.DIV_WEIGHT_SUM
    assert L.LabelSmoothingCrossEntropy(0.1)._divisor == nat.DIV_BATCH and L.FocalLoss()._divisor == nat.DIV_BATCH
    assert (nat.REDUCE_MEAN, nat.REDUCE_SUM, nat.REDUCE_NONE, nat.DIV_BATCH, nat.DIV_WEIGHT_SUM) == (0, 1, 2, 0, 1)


@pytest.mark.parametrize("bad", [torch.ones(3), torch.ones(1, 2), torch.ones(()), torch.ones(2, dtype=torch.float64),
                                 torch.ones(2, dtype=torch.int64), [1.0, 1.0]], ids=["len3", "2d", "0d", "f64", "i64", "list"])
def test_wrong_weight_shape_or_dtype_raises(bad):
    _, classes = _classes()
    for cls, kw in classes:
        with pytest.raises(ValueError, match=r"float32 tensor of shape \(2,\)"):
            cls(weight=bad, **kw)


def test_invalid_reduction_raises_at_construction():
    _, classes = _classes()
    for cls, kw in classes:
        with pytest.raises(ValueError, match="Invalid reduction: nope"):
            cls(reduction="nope", **kw)


def test_negative_weights_are_not_refused():
    L, _ = _classes()
    assert L.FocalLoss(weight=torch.tensor([-1.0, 2.0])).weight[0] == -1.0   # the reference has no sign check either


def test_cpu_tensors_still_raise_no_cpu_fallback():
    from wakeword_trainer_home_amd import _native as nat
    _, classes = _classes()
    for cls, kw in classes:
        for red in ("mean", "none"):
            with pytest.raises(nat.NativeError, match="no CPU fallback"):
                cls(weight=torch.tensor([0.55, 5.0]), reduction=red, **kw)(torch.zeros(4, 2), torch.zeros(4, dtype=torch.long))


def test_factory_passes_class_weights_through_and_moves_them():
    from wakeword_trainer_home_amd.models import losses as L
    w = torch.tensor([0.55, 5.0])
    for name, eps, cls in (("cross_entropy", 0.0, L.CrossEntropyLoss), ("cross_entropy", 0.1, L.LabelSmoothingCrossEntropy),
                           ("focal_loss", 0.1, L.FocalLoss)):
        c = L.create_loss_function(name, label_smoothing=eps, class_weights=w, device="meta")
        assert type(c) is cls and c.reduction == "mean" and c.weight.device.type == "meta" and tuple(c.weight.shape) == (2,)
        assert L.create_loss_function(name, label_smoothing=eps, device="meta").weight is None


# --------------------------------------------------------------------------- C ABI
def test_weighted_entry_is_declared_bound_and_exported():
    from wakeword_trainer_home_amd import _native as nat
    name = "ww_ce2_loss_weighted_fwd_bwd"
    header = (REPO / "include" / "wwhip.h").read_text()
    assert name in set(re.findall(r"\b(ww_[a-z0-9_]+)\s*\(", header))
    assert name in nat.EXPORTS and "ww_ce2_loss_fwd_bwd" in nat.EXPORTS
    assert hasattr(ctypes.CDLL(str(nat.lib_path())), name)
    assert nat.ABI_VERSION == 17 and nat.load().ww_abi_version() == 17
    assert re.search(r"#define WW_ABI_VERSION 17\b", header)
    for macro, value in (("WW_REDUCE_MEAN", 0), ("WW_REDUCE_SUM", 1), ("WW_REDUCE_NONE", 2), ("WW_DIV_BATCH", 0), ("WW_DIV_WEIGHT_SUM", 1)):
        assert re.search(rf"#define {macro} {value}\b", header), macro
    assert len(nat._SIGS[name][1]) == len(nat._SIGS["ww_ce2_loss_fwd_bwd"][1]) + 4


# --------------------------------------------------------------------------- helpers
def _config(mode):
    return SimpleNamespace(loss=SimpleNamespace(class_weights=mode))


def test_class_weights_from_config_branches():
    from wakeword_trainer_home_amd import training
    from wakeword_trainer_home_amd.training import calculate_class_weights, class_weights_from_config
    assert "class_weights_from_config" in training.__all__
    stats = {"positive": 200, "negative": 1800}                              # the reference test's imbalance
    w = class_weights_from_config(_config("balanced"), stats, "cpu")
    assert torch.equal(w, calculate_class_weights(stats, "balanced", "cpu"))
    assert w.dtype == torch.float32 and w.tolist() == [pytest.approx(2000 / 3600), pytest.approx(5.0)]
    assert class_weights_from_config(_config("none"), stats, "cpu") is None
    with pytest.raises(ValueError, match="explicit"):
        class_weights_from_config(_config("custom"), stats, "cpu")
    with pytest.raises(ValueError, match=r"Invalid class weights: sqrt \(valid: \['balanced', 'none', 'custom'\]\)"):
        class_weights_from_config(_config("sqrt"), stats, "cpu")


def test_default_config_field_is_one_of_the_handled_modes():
    from wakeword_trainer_home_amd.config import get_preset
    assert get_preset("cnn_small_logmel40").loss.class_weights in ("balanced", "none", "custom")
