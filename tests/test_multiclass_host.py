"""Host: more than two classes on the native losses -- constructors, factory, exports, the bindings' argument checks, the
confusion-matrix metrics against the reference's recorded numbers (tests/golden/g12_multiclass.npz) and the float64
restatement (tests/multiclass_cases.py) against the reference's recorded losses and gradients.  No GPU."""
import functools
import re
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import multiclass_cases as MC
from tests import weighted_loss_cases as WC

ROOT = Path(__file__).resolve().parent.parent
GOLDEN = Path(__file__).resolve().parent / "golden"
LOSS_CASES, METRIC_CASES = MC.load_g12(GOLDEN)


def _classes():
    from wakeword_trainer_home_amd.models import losses as L
    return {"ce0": L.CrossEntropyLoss, "ce0.1": functools.partial(L.LabelSmoothingCrossEntropy, 0.1), "focal": L.FocalLoss}


# --------------------------------------------------------------------------- 1. classes and factory
@pytest.mark.parametrize("name", ["ce0", "ce0.1", "focal"])
def test_classes_take_num_classes_and_a_weight_of_that_length(name):
    from wakeword_trainer_home_amd import _native as nat
    make = _classes()[name]
    w3 = torch.tensor([0.5, 2.0, 1.0])
    crit = make(weight=w3, num_classes=3)
    assert crit.num_classes == 3 and torch.equal(crit.weight, w3) and crit.confusion is None and crit.reduction == "mean"
    assert make(num_classes=nat.LOSS_MAX_CLASSES).num_classes == 64 and make(reduction="none", num_classes=5).weight is None
    with pytest.raises(ValueError, match=r"float32 tensor of shape \(3,\)"):
        make(weight=torch.ones(2), num_classes=3)
    with pytest.raises(ValueError, match=r"float32 tensor of shape \(3,\)"):
        make(weight=w3.double(), num_classes=3)
    for bad in (1, 65, 0, -3, 2.0, True):
        with pytest.raises(ValueError, match=r"num_classes must be an int in \[2, 64\]"):
            make(num_classes=bad)


@pytest.mark.parametrize("name", ["ce0", "ce0.1", "focal"])
def test_default_is_two_classes_as_before(name):
    make = _classes()[name]
    crit = make()
    assert crit.num_classes == 2 and crit.confusion is None
    assert torch.equal(make(weight=torch.tensor([0.55, 5.0])).weight, torch.tensor([0.55, 5.0]))
    with pytest.raises(ValueError, match=r"float32 tensor of shape \(2,\)"):
        make(weight=torch.ones(3))
    with pytest.raises(ValueError, match="num_classes > 2"):
        crit.track_confusion()
    z, y = torch.zeros(4, 3), torch.zeros(4, dtype=torch.int64)
    with pytest.raises(ValueError, match=r"num_classes = 2.*3 columns"):
        crit(z, y)
    with pytest.raises(ValueError, match=r"\(B,2\) for num_classes = 2"):
        crit.native_fwd_bwd(z, y)


def test_width_mismatch_names_both_numbers_and_there_is_no_cpu_path():
    from wakeword_trainer_home_amd import _native as nat
    from wakeword_trainer_home_amd.models import losses as L
    crit = L.FocalLoss(num_classes=5)
    y = torch.zeros(4, dtype=torch.int64)
    with pytest.raises(ValueError, match=r"num_classes = 5.*2 columns"):
        crit(torch.zeros(4, 2), y)
    with pytest.raises(ValueError, match=r"\(B,5\) for num_classes = 5.*\(4, 3\)"):
        crit.native_fwd_bwd(torch.zeros(4, 3), y)
    with pytest.raises(nat.NativeError, match="no CPU fallback"):
        crit(torch.zeros(4, 5), y)
    with pytest.raises(nat.NativeError, match="no CPU fallback"):
        crit.track_confusion("cpu")


def test_factory_passes_num_classes_on():
    from wakeword_trainer_home_amd.models import losses as L
    w = torch.tensor([0.5, 2.0, 1.0])
    a = L.create_loss_function("cross_entropy", num_classes=3, label_smoothing=0.1, class_weights=w, device="cpu")
    b = L.create_loss_function("cross_entropy", num_classes=3, label_smoothing=0.0, device="cpu")
    c = L.create_loss_function("focal_loss", num_classes=5, device="cpu")
    assert (type(a), a.num_classes, a.reduction) == (L.LabelSmoothingCrossEntropy, 3, "mean") and torch.equal(a.weight, w)
    assert (type(b), b.num_classes, b._divisor) == (L.CrossEntropyLoss, 3, L.nat.DIV_WEIGHT_SUM)
    assert (type(c), c.num_classes, c._divisor) == (L.FocalLoss, 5, L.nat.DIV_BATCH)
    d = L.create_loss_function("cross_entropy", device="cpu")
    assert (type(d), d.num_classes) == (L.LabelSmoothingCrossEntropy, 2)
    for bad in (1, 65):
        with pytest.raises(ValueError, match=r"num_classes must be an int in \[2, 64\]"):
            L.create_loss_function("focal_loss", num_classes=bad, device="cpu")
    with pytest.raises(ValueError, match=r"shape \(3,\)"):
        L.create_loss_function("focal_loss", num_classes=3, class_weights=torch.ones(2), device="cpu")


def test_cnn_small_stays_two_class():
    from wakeword_trainer_home_amd.models import create_model
    with pytest.raises(ValueError, match="num_classes == 2, got 3"):
        create_model("cnn_small", num_classes=3)


# --------------------------------------------------------------------------- 2. C-ABI and bindings
def test_new_entries_are_exported_and_declared_without_an_abi_bump():
    from wakeword_trainer_home_amd import _native as nat
    header = (ROOT / "include" / "wwhip.h").read_text()
    for name in ("ww_cen_loss_fwd_bwd", "ww_eval_accumulate_classes"):
        assert name in nat.EXPORTS and re.search(rf"\bint {name}\(", header), name
    assert "ww_ce2_loss_fwd_bwd" in nat.EXPORTS and "ww_ce2_loss_weighted_fwd_bwd" in nat.EXPORTS and "ww_eval_accumulate" in nat.EXPORTS
    assert nat.ABI_VERSION == 17 and re.search(r"#define WW_ABI_VERSION 17\b", header)
    assert nat.LOSS_MAX_CLASSES == 64 and re.search(r"#define WW_LOSS_MAX_CLASSES 64\b", header)
    assert nat.STEP_STATS_BYTES == 48 and len(nat.EVAL_COUNTERS) == 8
    if nat.lib_path().exists():
        lib = nat.load()
        assert hasattr(lib, "ww_cen_loss_fwd_bwd") and hasattr(lib, "ww_eval_accumulate_classes")


def test_loss_binding_refuses_bad_arguments_before_any_launch():
    from wakeword_trainer_home_amd import _native as nat
    y = torch.zeros(4, dtype=torch.int64)
    for z in (torch.zeros(4, 1), torch.zeros(4, 65), torch.zeros(4), torch.zeros(4, 3, dtype=torch.float64)):
        with pytest.raises(ValueError, match=r"\(B,C\)|outside \[2, 64\]"):
            nat.cen_loss_fwd_bwd(z, y)
    z = torch.zeros(4, 3)
    with pytest.raises(ValueError, match="int64 of shape"):
        nat.cen_loss_fwd_bwd(z, y.int())
    with pytest.raises(ValueError, match="int64 of shape"):
        nat.cen_loss_fwd_bwd(z, y[:3])
    with pytest.raises(ValueError, match=r"class_weight must be float32 of shape \(3,\)"):
        nat.cen_loss_fwd_bwd(z, y, class_weight=torch.ones(2))
    with pytest.raises(ValueError, match=r"confusion must be int64 of shape \(3, 3\)"):
        nat.cen_loss_fwd_bwd(z, y, confusion=torch.zeros(2, 2, dtype=torch.int64))
    with pytest.raises(ValueError, match=r"confusion must be int64 of shape \(3, 3\)"):
        nat.cen_loss_fwd_bwd(z, y, confusion=torch.zeros(3, 3, dtype=torch.int32))
    with pytest.raises(nat.NativeError, match="no CPU fallback"):
        nat.cen_loss_fwd_bwd(z, y)


def test_eval_binding_refuses_bad_arguments_before_any_launch():
    from wakeword_trainer_home_amd import _native as nat
    n, K = 4, 3
    ok = dict(targets=torch.zeros(n, dtype=torch.int64), thresholds=torch.linspace(0, 1, K, dtype=torch.float64), decision=0.5,
              conf=torch.zeros(n), pred=torch.zeros(n, dtype=torch.uint8), bins=torch.zeros(n, dtype=torch.int32), offset=0,
              hist=torch.zeros(2 * (K + 1), dtype=torch.int64), counters=torch.zeros(8, dtype=torch.int64))
    z = torch.zeros(n, 3)
    for bad_z in (torch.zeros(n, 1), torch.zeros(n, 65), torch.zeros(n), z.double()):
        with pytest.raises(ValueError, match=r"\(B,C\)|outside \[2, 64\]"):
            nat.eval_accumulate_classes(bad_z, **ok)
    for key, val, msg in (("targets", ok["targets"].int(), "int64 of shape"), ("thresholds", ok["thresholds"].float(), "float64"),
                          ("conf", ok["conf"].double(), "float32 / uint8 / int32"), ("offset", 1, "offset \\+ B = 5"),
                          ("hist", ok["hist"][:-1], "2\\*\\(K\\+1\\) = 8"), ("counters", ok["counters"][:7], "int64 with 8")):
        with pytest.raises(ValueError, match=msg):
            nat.eval_accumulate_classes(z, **{**ok, key: val})
    with pytest.raises(nat.NativeError, match="no CPU fallback"):
        nat.eval_accumulate_classes(z, **ok)


def test_score_run_checks_its_width_before_allocating():
    from wakeword_trainer_home_amd.evaluation import ScoreRun
    for bad in (1, 65, 2.0):
        with pytest.raises(ValueError, match=r"num_classes must be an int in \[2, 64\]"):
            ScoreRun(4, [0.5], 0.5, "cpu", num_classes=bad)


# --------------------------------------------------------------------------- 3. metrics
@pytest.mark.parametrize("case", METRIC_CASES, ids=lambda c: c["name"])
def test_from_confusion_equals_the_reference_calculator_exactly(case):
    from wakeword_trainer_home_amd.training.metrics import MetricResults, MetricsCalculator, MetricsTracker
    C = case["z"].shape[1]
    assert (case["y"] >= 2).any() and case["matrix"].shape == (C, C)
    pred = torch.from_numpy(case["z"]).argmax(dim=1).numpy()
    assert np.array_equal(MC.predictions(case["z"]), pred)                    # no NaN here: the two argmax rules agree
    assert (np.sort(case["z"], axis=1)[:, -1] == np.sort(case["z"], axis=1)[:, -2]).sum() >= 10      # exact ties at the top
    matrix = MC.confusion(pred, case["y"], C)
    assert np.array_equal(matrix, case["matrix"])
    for m in (matrix, torch.from_numpy(matrix), matrix.tolist()):
        res = MetricResults.from_confusion(m)
        assert res.to_dict() == case["results"]                               # floats included: the same divisions
    assert res.total_samples == 40 > res.true_positives + res.true_negatives + res.false_positives + res.false_negatives
    calc = MetricsCalculator(device="cpu")
    assert calc.calculate(torch.from_numpy(case["z"]), torch.from_numpy(case["y"])).to_dict() == case["results"]
    assert np.array_equal(calc.confusion_matrix(torch.from_numpy(case["z"]), torch.from_numpy(case["y"]), C).numpy(), matrix)
    # the tracker: two halves of the samples give the whole
    tracker = MetricsTracker(device="cpu")
    assert tracker.compute().total_samples == 0
    tracker.update_confusion(MC.confusion(pred[:17], case["y"][:17], C))
    tracker.update_confusion(torch.from_numpy(MC.confusion(pred[17:], case["y"][17:], C)))
    assert tracker.compute().to_dict() == case["results"]
    with pytest.raises(ValueError, match="one size per epoch"):
        tracker.update_confusion(np.zeros((C + 1, C + 1), np.int64))
    tracker.reset()
    tracker.update_counts(1, 2, 3, 4)
    assert tracker.compute().to_dict() == MetricResults.from_counts(1, 2, 3, 4).to_dict()        # the 2-class path, untouched


def test_from_confusion_at_two_classes_is_from_counts_and_rejects_other_shapes():
    from wakeword_trainer_home_amd.training.metrics import MetricResults
    m = np.array([[7, 2], [3, 5]])                                           # [target, pred]: tn fp / fn tp
    assert MetricResults.from_confusion(m).to_dict() == MetricResults.from_counts(5, 7, 2, 3).to_dict()
    assert MetricResults.from_confusion(np.zeros((3, 3), np.int64)).to_dict() == MetricResults.empty().to_dict()
    for bad in (np.zeros((2, 3), np.int64), np.zeros((1, 1), np.int64), np.zeros(4, np.int64), np.zeros((3, 3))):
        with pytest.raises(ValueError, match="square integer matrix"):
            MetricResults.from_confusion(bad)


def test_epoch_reduce_sums_the_matrix_across_ranks():
    """``Trainer._epoch_reduce`` driven on the host with a stand-in for the process group whose all_reduce adds a second
    rank's contribution (here: the same values again).  tests/test_multiclass_dp_gpu.py runs two real ranks on one GPU."""
    from wakeword_trainer_home_amd.training.metrics import MetricsTracker
    from wakeword_trainer_home_amd.training.trainer import Trainer
    case = METRIC_CASES[0]
    C = case["z"].shape[1]
    tracker = MetricsTracker(device="cpu")
    tracker.update_confusion(case["matrix"])
    tracker.update_counts(1, 2, 3, 4)
    seen = []

    def all_reduce(t):
        seen.append(tuple(t.shape))
        t.mul_(2)
    fake = SimpleNamespace(_dist=SimpleNamespace(all_reduce=all_reduce), device="cpu", _dev_type="cpu",
                           _confusion=torch.zeros(C, C, dtype=torch.int64), _num_classes=C)
    loss_sum, n = Trainer._epoch_reduce(fake, tracker, 1.5, 3)
    assert (loss_sum, n) == (3.0, 6) and tracker._c == [2, 4, 6, 8] and (C, C) in seen
    assert tracker._m.dtype == np.int64 and np.array_equal(tracker._m, 2 * case["matrix"])
    assert tracker.compute().total_samples == 80
    # a rank whose epoch gave no matrix (every batch failed) still takes part in the reduce, with zeros
    empty = MetricsTracker(device="cpu")
    Trainer._epoch_reduce(fake, empty, 0.0, 0)
    assert np.array_equal(empty._m, np.zeros((C, C), np.int64))
    # two classes: no matrix is reduced
    seen.clear()
    fake._confusion, fake._num_classes = None, 2
    two = MetricsTracker(device="cpu")
    two.update_counts(1, 1, 1, 1)
    Trainer._epoch_reduce(fake, two, 1.0, 1)
    assert two._m is None and seen == [(5,), (1,)]


# --------------------------------------------------------------------------- 4. the restatement
@pytest.mark.parametrize("B", [1, 65, 1025])
def test_restatement_is_the_two_class_one_at_two_columns(B):
    z, y = WC.batch(B)
    for kind, h in WC.LOSSES.values():
        a, b = WC.per_sample(kind, z, y, **h), MC.per_sample(kind, z, y, **h)
        for u, v in zip(a, b):
            assert np.abs(u - v).max() <= 1e-14 * max(1.0, np.abs(u).max())
    assert MC.counters(z, y) == WC.counters(z, y)


@pytest.mark.parametrize("case", LOSS_CASES, ids=lambda c: c["name"])
def test_restatement_matches_the_recorded_reference_within_fp32_error(case):
    """The recorded numbers are fp32 results of a handful of operations on numbers of the size of the largest entry: 16 ulps
    of that entry, 16 * 2^-24 = 9.5e-7, rounded to 1e-6 as everywhere in these tests."""
    kind, h = MC.LOSSES[case["loss_name"]]
    loss, grad = MC.weighted_loss(kind, case["z"], case["y"], case["weight"], case["reduction"], MC.divisor_of(case["loss_name"]),
                                  case["upstream"], **h)
    rec_l, rec_g = np.asarray(case["loss"], np.float64), case["grad"].astype(np.float64)
    assert np.isfinite(rec_l).all() and np.isfinite(rec_g).all()
    assert np.abs(rec_l - loss).max() <= 1e-6 * np.abs(loss).max()
    assert np.abs(rec_g - grad).max() <= 1e-6 * np.abs(grad).max()
    assert not (np.abs(np.abs(MC.margins_of(case["z"], case["y"])) - MC.CLAMP_MARGIN) < 0.5).any()


def test_fixture_holds_the_cases_the_tests_rely_on():
    names = [c["name"] for c in LOSS_CASES]
    assert len(names) == len(set(names)) == 78
    for C in (3, 5):
        for ln in MC.LOSSES:
            for red in ("mean", "sum", "none"):
                for B in (1, 3, 65):
                    assert f"{ln}|{red}|generic|C{C}B{B}" in names
            assert f"{ln}|mean|none|C{C}B65" in names and f"{ln}|mean|zero|C{C}B65" in names and f"{ln}|mean|generic|C{C}big" in names
    big = next(c for c in LOSS_CASES if c["name"].endswith("C3big"))
    assert np.abs(big["z"]).max() == 88.0
    zero = next(c for c in LOSS_CASES if "|zero|" in c["name"])
    assert 0.0 in zero["weight"] and (zero["y"] == zero["weight"].index(0.0)).any()
    assert (GOLDEN / "g12_multiclass.npz").stat().st_size < 100 * 1024


@pytest.mark.parametrize("C", [2, 3, 5, 12, 63, 64])
def test_shared_batches_cover_margins_targets_and_ties(C):
    z, y = MC.batch_c(1025, C)
    assert z.shape == (1025, C) and z.dtype == np.float32 and not z.flags.writeable
    assert set(y.tolist()) == set(range(C))
    mg = MC.margins_of(z, y)
    for want in MC.MARGINS:
        assert (np.abs(mg - want) <= 1e-5 * max(1.0, abs(want))).any(), want
    top2 = np.sort(z, axis=1)[:, -2:]
    assert (top2[:, 0] == top2[:, 1]).sum() >= 20                            # exact ties that decide the argmax
    pred = MC.predictions(z)
    assert np.array_equal(pred, z.argmax(axis=1)) and MC.confusion(pred, y, C).sum() == 1025
    assert MC.batch_c(65, C, 1)[1].tolist() == [1] * 65
