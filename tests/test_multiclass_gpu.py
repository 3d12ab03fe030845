"""GPU: more than two classes -- ww_cen_loss_fwd_bwd and ww_eval_accumulate_classes from the kernels to the Trainer and the
evaluator.

Float tolerances are those of tests/test_weighted_loss_gpu.py and take nothing from the kernel: every float tensor is compared
with the float64 restatement (tests/multiclass_cases.py) under ``max(1e-6 * max|tensor|, 4 * e32)``, e32 being the error of the
fp32 CPU torch formulation on the same inputs against the same float64 values.  Counters, flags, matrices, power-of-two scalings
and everything said to equal another entry must be exact.  Each parity test prints what it measured
(profiles/multiclass_loss_measured.txt keeps one run's figures)."""
import functools
import logging
from pathlib import Path

import numpy as np
import pytest
import torch

from tests import multiclass_cases as MC
from tests import weighted_loss_cases as WC
from tests.evaluation_cases import F32, F64, ULP_BOUND, predictions_at, restated_roc, roc_thresholds

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLDEN = Path(__file__).resolve().parent / "golden"
MODES = (("mean", "batch"), ("mean", "weight_sum"), ("sum", "batch"), ("none", "batch"), ("none", "weight_sum"))
PARITY_B = (1, 3, 64, 65, 1023, 1024, 1025, 2500)
LOSS_CASES, _ = MC.load_g12(GOLDEN)


@pytest.fixture(scope="module")
def nat():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from wakeword_trainer_home_amd import _native
    _native.load()
    return _native


def _dev(a, dtype=None):
    return torch.from_numpy(np.array(a, dtype=dtype)).to(DEV)


@functools.lru_cache(maxsize=None)
def _weight(C):
    """One weight per class, no two alike among the first seven, as the float32 values the kernel is handed."""
    w = [0.55 + 0.37 * ((5 * j) % 7) for j in range(C)]
    w[1] = 5.0
    return tuple(float(np.float32(v)) for v in w)


def _launch(nat, loss_name, z, y, weight, reduction, divisor, **extra):
    kind, h = MC.LOSSES[loss_name]
    w = None if weight is None else torch.tensor(weight, dtype=torch.float32, device=DEV)
    return nat.cen_loss_fwd_bwd(
        _dev(z, np.float32), _dev(y, np.int64), nat.LOSS_CE if kind == "ce" else nat.LOSS_FOCAL, h.get("eps", 0.0),
        h.get("alpha", 0.25), h.get("gamma", 2.0), class_weight=w,
        reduction={"mean": nat.REDUCE_MEAN, "sum": nat.REDUCE_SUM, "none": nat.REDUCE_NONE}[reduction],
        mean_divisor={"batch": nat.DIV_BATCH, "weight_sum": nat.DIV_WEIGHT_SUM}[divisor], **extra)


def _err(got, ref):
    got = got.detach().cpu().numpy() if torch.is_tensor(got) else got
    return float(np.abs(np.asarray(got, dtype=np.float64) - ref).max())


def _top(a):
    return float(np.abs(a).max())


def _close(what, got, ref, e32, where):
    """max |got - ref| <= max(1e-6 * max|ref|, 4 * e32) over the whole tensor; a NaN on either side fails.  -> err / max|ref|"""
    err, bound = _err(got, ref), max(1e-6 * _top(ref), 4.0 * e32)
    print(f"measured {where}: {what} max abs err {err:.3e} (bound {bound:.3e}, fp32 CPU e32 {e32:.3e}, max|ref| {_top(ref):.3e})")
    assert err <= bound, f"{where}: {what} max abs err {err:.3e} > bound {bound:.3e} (fp32 CPU e32 {e32:.3e}, max|ref| {_top(ref):.3e})"
    return err / _top(ref) if _top(ref) else err


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


@functools.lru_cache(maxsize=None)
def _reference(loss_name, B, C, targets, reduction, divisor):
    """Float64 values and the fp32 CPU formulation's error against them; computed once per case, never modified."""
    kind, h = MC.LOSSES[loss_name]
    z, y = MC.batch_c(B, C, targets)
    W = _weight(C)
    loss, grad = MC.weighted_loss(kind, z, y, W, reduction, divisor, **h)
    l32, g32 = MC.torch32(kind, z, y, W, reduction, divisor, **h)
    out = dict(loss=loss, grad=grad, e_loss=float(np.abs(l32 - loss).max()), e_grad=float(np.abs(g32 - grad).max()))
    if reduction == "none":
        mean, _ = MC.weighted_loss(kind, z, y, W, "mean", divisor, **h)
        m32, _ = MC.torch32(kind, z, y, W, "mean", divisor, **h)
        out.update(mean=mean, e_mean=abs(float(m32) - float(mean)))
    return out


def _check_parity(nat, loss_name, B, C, targets="mixed"):
    z, y = MC.batch_c(B, C, targets)
    W = _weight(C)
    matrix = MC.confusion(MC.predictions(z), y, C)
    conf = torch.zeros(C, C, dtype=torch.int64, device=DEV)
    for n, (reduction, divisor) in enumerate(MODES, 1):
        where = f"{loss_name} C={C} B={B} targets={targets} {reduction}/{divisor}"
        r = _reference(loss_name, B, C, targets, reduction, divisor)
        found = torch.full((1,), 7.0, device=DEV)
        loss, vec, dl, stats = _launch(nat, loss_name, z, y, W, reduction, divisor, found_inf_out=found, confusion=conf)
        assert (vec is not None) == (reduction == "none") and tuple(dl.shape) == (B, C), where
        _close("dlogits", dl, r["grad"], r["e_grad"], where)
        if reduction == "none":
            _close("loss_vec", vec, r["loss"], r["e_loss"], where)
            _close("reported mean", np.float64(loss.item()), np.float64(r["mean"]), r["e_mean"], where)
        else:
            _close("loss", np.float64(loss.item()), np.float64(r["loss"]), r["e_loss"], where)
        st = nat.decode_stats(stats.cpu())
        assert (st["correct"], st["tp"], st["tn"], st["fp"], st["fn"]) == MC.counters(z, y), where      # weights ignored
        assert st["count"] == B and st["nonfinite"] == 0 and st["bad_target"] == 0 and st["reserved"] == 0, where
        assert st["loss"] == loss.item() and st["grad_norm"] == 0.0 and st["found_inf"] == 0.0 and found.item() == 0.0, where
        assert np.array_equal(conf.cpu().numpy(), n * matrix), where                                     # added to, never reset


# --------------------------------------------------------------------------- 1. parity with the float64 restatement
@pytest.mark.parametrize("B", PARITY_B)
@pytest.mark.parametrize("C", [3, 5, 64])
@pytest.mark.parametrize("loss_name", list(MC.LOSSES))
def test_kernel_matches_float64_restatement(nat, loss_name, C, B):
    """One sample, less than a wave, a wave boundary, the block-stride boundary from both sides, a third trip."""
    _check_parity(nat, loss_name, B, C)


@pytest.mark.parametrize("B", [65, 1025])
@pytest.mark.parametrize("C", [2, 12, 63])
@pytest.mark.parametrize("loss_name", list(MC.LOSSES))
def test_kernel_matches_float64_restatement_at_other_widths(nat, loss_name, C, B):
    _check_parity(nat, loss_name, B, C)


@pytest.mark.parametrize("C", [4, 8, 9, 16, 17, 32, 33])
@pytest.mark.parametrize("loss_name", list(MC.LOSSES))
def test_kernel_matches_float64_restatement_around_powers_of_two(nat, loss_name, C):
    """The widths either side of every power of two up to 32, at a batch whose second trip holds one sample.  (The kernel walks
    a row column by column, so no width is special to it today; a mapping of a row onto a group of lanes would change path at
    exactly these widths -- the one that was measured and not kept did, DESIGN.md "Loss scope".)"""
    _check_parity(nat, loss_name, 1025, C)


def test_prediction_rule_with_nan_and_infinite_logits(nat):
    """pred is the first index of the row maximum under > as a scan from column 0 finds it: a NaN never beats a number, a NaN
    in column 0 is never beaten, -inf ties go to the lower index.  Only the counters and the matrix are looked at."""
    nan, inf = np.nan, np.inf
    rows = [[1.0, nan, 0.5], [nan, 3.0, 1.0], [0.0, nan, 2.0], [nan, nan, nan], [-inf, -inf, -inf], [-inf, 1.0, nan],
            [2.0, 2.0, nan], [0.0, inf, inf], [nan, inf, 0.0], [1.0, 0.0, nan], [2.0, 2.0, 1.0], [0.5, 1.5, 1.5]]
    want = [0, 0, 2, 0, 0, 1, 0, 1, 0, 0, 0, 1]
    for C in (3, 5, 12):
        z = np.full((len(rows), C), -inf, F32)                                              # the columns beyond 2 never win
        z[:, :3] = np.array(rows, F32)
        assert MC.predictions(z).tolist() == want
        y = np.resize(np.array([0, 1, 2], np.int64), len(rows))
        conf = torch.zeros(C, C, dtype=torch.int64, device=DEV)
        _, _, _, stats = _launch(nat, "focal", z, y, None, "sum", "batch", confusion=conf)
        st = nat.decode_stats(stats.cpu())
        assert (st["correct"], st["tp"], st["tn"], st["fp"], st["fn"]) == MC.counters(z, y), C
        assert st["nonfinite"] == 1 and st["found_inf"] == 1.0 and not conf.any()            # a NaN loss: the batch is not counted
        ok = np.isfinite(z[:, :3]).all(axis=1)                                                # the finite rows alone are
        _, _, _, stats = _launch(nat, "focal", z[ok], y[ok], None, "sum", "batch", confusion=conf)
        assert nat.decode_stats(stats.cpu())["found_inf"] == 0.0 and ok.sum() == 2
        assert np.array_equal(conf.cpu().numpy(), MC.confusion(MC.predictions(z[ok]), y[ok], C))


@pytest.mark.parametrize("target", [0, 1, 2])
@pytest.mark.parametrize("loss_name", list(MC.LOSSES))
def test_one_class_alone_in_the_weight_sum(nat, loss_name, target):
    _check_parity(nat, loss_name, 65, 3, target)


def test_zero_weight_sum_is_nan_skips_and_leaves_the_matrix_alone(nat):
    z, _ = MC.batch_c(65, 3)
    y = np.full(65, 2, np.int64)
    conf = torch.full((3, 3), 7, dtype=torch.int64, device=DEV)
    found = torch.full((1,), 7.0, device=DEV)
    loss, _, dl, stats = _launch(nat, "ce0", z, y, (1.5, 2.0, 0.0), "mean", "weight_sum", found_inf_out=found, confusion=conf)
    st = nat.decode_stats(stats.cpu())
    assert torch.isnan(loss) and np.isnan(st["loss"])                          # 0/0, as torch's weighted cross_entropy gives
    assert (st["nonfinite"], st["bad_target"], st["found_inf"], st["count"], found.item()) == (1, 0, 1.0, 65, 1.0)
    assert (conf == 7).all()
    # under the batch divisor the same batch is a finite zero, and is counted
    loss, _, dl, stats = _launch(nat, "ce0.1", z, y, (1.5, 2.0, 0.0), "mean", "batch", found_inf_out=found, confusion=conf)
    st = nat.decode_stats(stats.cpu())
    assert loss.item() == 0.0 and not dl.any() and (st["nonfinite"], st["found_inf"], found.item()) == (0, 0.0, 0.0)
    assert np.array_equal(conf.cpu().numpy() - 7, MC.confusion(MC.predictions(z), y, 3))


# --------------------------------------------------------------------------- 2. the confusion matrix
@pytest.mark.parametrize("C", [3, 64])
def test_two_launches_add_into_one_matrix(nat, C):
    (z1, y1), (z2, y2) = MC.batch_c(2500, C), MC.batch_c(1025, C)
    conf = torch.zeros(C, C, dtype=torch.int64, device=DEV)
    _launch(nat, "ce0.1", z1, y1, None, "mean", "batch", confusion=conf)
    _launch(nat, "focal", z2, y2, _weight(C), "sum", "batch", confusion=conf)
    want = MC.confusion(MC.predictions(z1), y1, C) + MC.confusion(MC.predictions(z2), y2, C)
    assert np.array_equal(conf.cpu().numpy(), want) and want.sum() == 3525
    assert (np.diag(want) > 0).all() and (want.sum(axis=1) > 0).all()


@pytest.mark.parametrize("bad", ["C", -1])
@pytest.mark.parametrize("reduction,divisor", MODES)
def test_bad_target_is_clamped_flagged_and_keeps_the_batch_out_of_the_matrix(nat, bad, reduction, divisor):
    """Index 1500 of 2500 is reached on the block's second trip.  Apart from the flags, the outputs are those of the batch with
    the target already clamped -- so the sample took the clamped class's weight."""
    C = 5
    z, y = (np.array(a) for a in MC.batch_c(2500, C))
    y_bad, y_clamped = y.copy(), y.copy()
    y_bad[1500], y_clamped[1500] = (C, C - 1) if bad == "C" else (-1, 0)
    conf = torch.zeros(C, C, dtype=torch.int64, device=DEV)
    found = torch.full((1,), 7.0, device=DEV)
    loss, vec, dl, stats = _launch(nat, "ce0.1", z, y_bad, _weight(C), reduction, divisor, found_inf_out=found, confusion=conf)
    assert not conf.any()
    loss_c, vec_c, dl_c, stats_c = _launch(nat, "ce0.1", z, y_clamped, _weight(C), reduction, divisor, confusion=conf)
    assert np.array_equal(conf.cpu().numpy(), MC.confusion(MC.predictions(z), y_clamped, C))
    assert torch.equal(_bits(loss), _bits(loss_c)) and torch.equal(_bits(dl), _bits(dl_c))
    assert vec is None or torch.equal(_bits(vec), _bits(vec_c))
    st, st_c = nat.decode_stats(stats.cpu()), nat.decode_stats(stats_c.cpu())
    assert (st["bad_target"], st["found_inf"], st["nonfinite"], found.item()) == (1, 1.0, 0, 1.0)
    assert (st_c["bad_target"], st_c["found_inf"]) == (0, 0.0)
    assert all(st[k] == st_c[k] for k in ("correct", "tp", "tn", "fp", "fn", "count", "loss"))


def test_without_a_matrix_the_outputs_are_the_same_and_nothing_else_is_written(nat):
    C = 5
    z, y = MC.batch_c(1025, C)
    near = torch.zeros(2, C, C, dtype=torch.int64, device=DEV)                # [0] is handed over, [1] lies right behind it
    a = _launch(nat, "focal", z, y, _weight(C), "none", "batch", confusion=near[0])
    b = _launch(nat, "focal", z, y, _weight(C), "none", "batch")
    for u, v in zip(a, b):
        assert torch.equal(u.cpu().view(torch.uint8), v.cpu().view(torch.uint8))
    assert near[0].sum().item() == 1025 and not near[1].any()


# --------------------------------------------------------------------------- 3. loss scale, found_inf_out
@functools.lru_cache(maxsize=None)
def _plain_batch(B, C):
    """Logits within a few units: every gradient is a normal float, so scaling by a power of two is exact."""
    rng = np.random.default_rng(77 + B + C)
    z = rng.normal(0.0, 2.0, (B, C)).astype(np.float32)
    y = rng.integers(0, C, B).astype(np.int64)
    return z, y


@pytest.mark.parametrize("B,C", [(65, 3), (1025, 5), (65, 64)])
@pytest.mark.parametrize("loss_name", list(MC.LOSSES))
def test_loss_scale_multiplies_the_gradient_exactly_in_every_reduction(nat, loss_name, B, C):
    z, y = _plain_batch(B, C)
    ls = nat.loss_scale_new(DEV, 2.0 ** 10)
    ls[0:8].view(torch.float32)[1] = 2.0 ** 16
    for reduction, divisor in MODES:
        loss0, vec0, dl0, _ = _launch(nat, loss_name, z, y, _weight(C), reduction, divisor)
        assert np.abs(dl0.cpu().numpy()).min() >= 2.0 ** -100
        for slot, scale in ((0, 2.0 ** 10), (1, 2.0 ** 16)):
            loss, vec, dl, _ = _launch(nat, loss_name, z, y, _weight(C), reduction, divisor, loss_scale=ls, loss_scale_slot=slot)
            where = f"{loss_name} B={B} C={C} {reduction}/{divisor} slot {slot}"
            assert torch.equal(dl.cpu(), dl0.cpu() * scale), where
            assert torch.equal(_bits(loss), _bits(loss0)) and (vec is None or torch.equal(_bits(vec), _bits(vec0))), where
    assert [nat.loss_scale_read(ls, s)["scale"] for s in (0, 1)] == [2.0 ** 10, 2.0 ** 16]


def test_argument_checks_of_the_entry(nat):
    z, y = _plain_batch(3, 3)
    zt, yt = _dev(z), _dev(y)
    with pytest.raises(ValueError, match="unknown reduction 3"):
        nat.cen_loss_fwd_bwd(zt, yt, reduction=3)
    with pytest.raises(ValueError, match="unknown mean_divisor 2"):
        nat.cen_loss_fwd_bwd(zt, yt, mean_divisor=2)
    with pytest.raises(nat.NativeError, match="no CPU fallback"):
        nat.cen_loss_fwd_bwd(zt, yt, class_weight=torch.ones(3))
    lib, none_ptr = nat.load(), None
    args = lambda C, red, vec: (nat.ctx(torch.device(DEV)), zt.data_ptr(), yt.data_ptr(), 3, C, nat.LOSS_CE, 0.0, 0.25, 2.0, none_ptr,
                                red, nat.DIV_BATCH, none_ptr, vec, torch.empty_like(zt).data_ptr(), none_ptr, none_ptr, none_ptr,
                                none_ptr, 0, none_ptr)
    assert lib.ww_cen_loss_fwd_bwd(*args(3, nat.REDUCE_NONE, none_ptr)) == -1 and b"needs loss_vec" in lib.ww_last_error()
    for C in (1, 65, 0, -2):
        assert lib.ww_cen_loss_fwd_bwd(*args(C, nat.REDUCE_MEAN, none_ptr)) == -1 and b"outside [2, 64]" in lib.ww_last_error()
        rc = lib.ww_eval_accumulate_classes(nat.ctx(torch.device(DEV)), zt.data_ptr(), C, none_ptr, 3, zt.data_ptr(), 1, 0.5,
                                            zt.data_ptr(), zt.data_ptr(), none_ptr, 0, zt.data_ptr(), zt.data_ptr(), none_ptr)
        assert rc == -1 and b"outside [2, 64]" in lib.ww_last_error()


# --------------------------------------------------------------------------- 4. the reference's recorded numbers
def _make(loss_name, C, weight, reduction):
    from wakeword_trainer_home_amd.models import losses as L
    cls = {"ce0": L.CrossEntropyLoss, "ce0.1": functools.partial(L.LabelSmoothingCrossEntropy, 0.1), "focal": L.FocalLoss}[loss_name]
    return cls(weight=weight, reduction=reduction, num_classes=C).to(DEV)


@pytest.mark.parametrize("case", LOSS_CASES, ids=lambda c: c["name"])
def test_g12_cases_on_the_device(nat, case):
    """Through the public classes (the factory for 'mean', as the fixture was made; autograd with the recorded upstream vector
    for 'none'), against what the reference recorded; e32 is the recorded fp32 numbers' own distance from the float64
    restatement."""
    from wakeword_trainer_home_amd.models import losses as L
    ln, red = case["loss_name"], case["reduction"]
    kind, h = MC.LOSSES[ln]
    C = case["z"].shape[1]
    ref_l, ref_g = MC.weighted_loss(kind, case["z"], case["y"], case["weight"], red, MC.divisor_of(ln), case["upstream"], **h)
    rec_l, rec_g = np.asarray(case["loss"], dtype=np.float64), np.asarray(case["grad"], dtype=np.float64)
    w = None if case["weight"] is None else torch.tensor(case["weight"], dtype=torch.float32)
    if red == "mean":
        crit = L.create_loss_function({"ce0": "cross_entropy", "ce0.1": "cross_entropy", "focal": "focal_loss"}[ln], num_classes=C,
                                      label_smoothing=h.get("eps", 0.0), focal_alpha=0.25, focal_gamma=2.0, class_weights=w, device=DEV)
        assert crit.num_classes == C and (w is None or crit.weight.device.type == "cuda")
    else:
        crit = _make(ln, C, w, red)
    z = _dev(case["z"], np.float32).requires_grad_()
    loss = crit(z, _dev(case["y"], np.int64))
    loss.backward(_dev(case["upstream"], np.float32) if red == "none" else None)
    assert tuple(loss.shape) == (() if red != "none" else (len(case["y"]),))
    _close("loss", loss, rec_l, float(np.abs(rec_l - ref_l).max()), case["name"])
    _close("dlogits", z.grad, rec_g, float(np.abs(rec_g - ref_g).max()), case["name"])


def test_module_raises_on_a_bad_target_naming_the_range(nat):
    z, y = _plain_batch(65, 3)
    y = y.copy()
    y[7] = 3
    for crit in (_make("focal", 3, torch.tensor(_weight(3)), "mean"), _make("ce0", 3, None, "sum"), _make("ce0.1", 3, None, "none")):
        assert crit.validate_targets is True
        with pytest.raises(ValueError, match=r"Target values must be in \[0, 2\]"):
            crit(_dev(z), _dev(y))


def test_track_confusion_keeps_one_buffer_and_counts_every_launch(nat):
    z, y = MC.batch_c(65, 3)
    crit = _make("ce0.1", 3, None, "mean")
    assert crit.confusion is None
    m = crit.track_confusion()
    assert m.dtype == torch.int64 and tuple(m.shape) == (3, 3) and m.device.type == "cuda" and not m.any()
    assert crit.track_confusion() is m and crit.confusion is m
    ptr = m.data_ptr()
    crit(_dev(z), _dev(y))
    crit.native_fwd_bwd(_dev(z), _dev(y))
    assert crit.confusion.data_ptr() == ptr
    assert np.array_equal(m.cpu().numpy(), 2 * MC.confusion(MC.predictions(z), y, 3))


# --------------------------------------------------------------------------- 5. routing at two classes
@pytest.mark.parametrize("loss_name", list(MC.LOSSES))
def test_two_class_criteria_still_take_the_two_class_entries_bit_for_bit(nat, loss_name, monkeypatch):
    kind, h = MC.LOSSES[loss_name]
    z, y = WC.batch(1025)
    zt, yt = _dev(z), _dev(y)
    args = (nat.LOSS_CE if kind == "ce" else nat.LOSS_FOCAL, h.get("eps", 0.0), h.get("alpha", 0.25), h.get("gamma", 2.0))
    monkeypatch.setattr(nat, "cen_loss_fwd_bwd", lambda *a, **k: pytest.fail("two classes must not take the C-class entry"))
    from wakeword_trainer_home_amd.models import losses as L
    cls = {"ce0": L.CrossEntropyLoss, "ce0.1": functools.partial(L.LabelSmoothingCrossEntropy, 0.1), "focal": L.FocalLoss}[loss_name]
    for kw in ({}, {"num_classes": 2}):
        crit = cls(**kw).to(DEV)
        assert crit.num_classes == 2
        zg = zt.clone().requires_grad_()
        loss = crit(zg, yt)
        loss.backward()
        loss0, dl0, st0 = nat.ce2_loss_fwd_bwd(zt, yt, *args)
        assert torch.equal(_bits(loss), _bits(loss0.reshape(()))) and torch.equal(_bits(zg.grad), _bits(dl0))
        assert torch.equal(crit.last_stats.cpu(), st0.cpu())
    w = torch.tensor([0.55, 5.0])
    crit = _make(loss_name, 2, w, "sum")
    zg = zt.clone().requires_grad_()
    loss = crit(zg, yt)
    loss.backward()
    loss0, _, dl0, st0 = nat.ce2_loss_weighted_fwd_bwd(zt, yt, *args, class_weight=w.to(DEV), reduction=nat.REDUCE_SUM,
                                                       mean_divisor=crit._divisor)
    assert torch.equal(_bits(loss), _bits(loss0.reshape(()))) and torch.equal(_bits(zg.grad), _bits(dl0))
    assert torch.equal(crit.last_stats.cpu(), st0.cpu())


# --------------------------------------------------------------------------- 6. the score stage
def _eval_logits(n, C):
    rng = np.random.default_rng(50 + C)
    z = rng.normal(0.0, 6.0, (n, C)).astype(F32)
    for b, (a, c) in zip(range(2, n, 5), [(0, 2), (1, 2), (0, 1)] * n):       # exact ties at the top of the row
        z[b, a] = z[b, c] = z[b].max() + F32(1.0)
    nan_rows = list(range(7, n, 11))
    for k, b in enumerate(nan_rows):                                          # a NaN column, sometimes two
        z[b, k % C] = np.nan
        if k % 3 == 2:
            z[b, (k + 2) % C] = np.nan
    return z, np.array(nan_rows, np.int64)


@pytest.mark.parametrize("B", [1, 63, 64, 65, 1025])
@pytest.mark.parametrize("C", [3, 12])
def test_eval_accumulate_classes(nat, C, B):
    """Two calls into the same accumulators at offsets 0 and B.  conf against a float64 softmax (16 fp32 ulps, the bound of
    tests/test_evaluation_gpu.py); the argmax counters equal torch.argmax on the CPU; decisions, bins and the histogram are
    exact when recomputed from the kernel's own confidences; targets 2..C-1 stay out of hist, C and -1 are bad."""
    from wakeword_trainer_home_amd.evaluation import bin_of, histogram
    n, thr = 2 * B, roc_thresholds()
    z, nan_rows = _eval_logits(n, C)
    t = np.resize(np.array([0, 1, 2, 1, 0, C - 1, 1, 0, C, 0, 1, -1, 2], np.int64), n)
    acc = dict(conf=torch.full((n + 3,), -7.0, device=DEV), pred=torch.full((n + 3,), 9, dtype=torch.uint8, device=DEV),
               bins=torch.full((n + 3,), -5, dtype=torch.int32, device=DEV), hist=torch.zeros(2 * (thr.size + 1), dtype=torch.int64, device=DEV),
               counters=torch.zeros(8, dtype=torch.int64, device=DEV))
    thr_dev = torch.from_numpy(thr).to(DEV)
    for call in range(2):
        s = slice(call * B, call * B + B)
        nat.eval_accumulate_classes(_dev(z[s]), _dev(t[s]), thr_dev, 0.5, acc["conf"], acc["pred"], acc["bins"], call * B,
                                    acc["hist"], acc["counters"])
    got = {k: v.cpu().numpy() for k, v in acc.items()}
    conf = got["conf"][:n]
    assert (got["conf"][n:] == -7.0).all() and (got["pred"][n:] == 9).all() and (got["bins"][n:] == -5).all()
    finite = np.ones(n, bool)
    finite[nan_rows] = False
    ref = MC.softmax_conf64(z[finite])
    rel = np.abs(conf[finite].astype(F64) - ref) / ref
    print(f"measured eval C={C} B={B}: worst relative confidence error {rel.max():.3e} (bound {ULP_BOUND:.3e})")
    assert rel.max() <= ULP_BOUND
    with np.errstate(invalid="ignore"):
        ref_nan = torch.softmax(torch.from_numpy(z), dim=1)[:, 1].numpy()
    assert np.array_equal(np.isnan(conf), np.isnan(ref_nan)) and np.isnan(conf).sum() == len(nan_rows)
    amax = torch.from_numpy(z).argmax(dim=1).numpy()                          # tie -> first, a NaN wins, the first NaN wins
    if len(nan_rows):
        assert np.isnan(z[nan_rows, amax[nan_rows]]).all()
    c = dict(zip(nat.EVAL_COUNTERS, got["counters"].tolist()))
    want = dict(tp=int(((amax == 1) & (t == 1)).sum()), tn=int(((amax == 0) & (t == 0)).sum()), fp=int(((amax == 1) & (t == 0)).sum()),
                fn=int(((amax == 0) & (t == 1)).sum()), count=n, bad_target=int(((t < 0) | (t >= C)).sum()),
                nan_score=len(nan_rows), reserved=0)
    assert c == want
    assert np.array_equal(got["pred"][:n], predictions_at(conf, [0.5])[0].astype(np.uint8))
    bins = bin_of(conf, thr)
    assert np.array_equal(got["bins"][:n], bins)
    hist = got["hist"].reshape(2, -1)
    assert np.array_equal(hist, histogram(bins, t, thr.size))
    assert hist.sum() == int(np.isin(t, (0, 1)).sum())                        # targets >= 2 are in neither row
    assert B == 1 or hist.sum() < n - want["bad_target"]


# --------------------------------------------------------------------------- 7. the evaluator
N_CLIP, N_CLIPS = 7040, 41


class _Clips(torch.utils.data.Dataset):
    def __init__(self):
        rng = np.random.default_rng(12)
        amp = rng.choice([1e-3, 0.02, 0.3, 1.0], (N_CLIPS, 1))
        self.waves = torch.from_numpy((rng.normal(0, 1, (N_CLIPS, N_CLIP)) * amp).clip(-1, 1).astype(F32))
        self.labels = (np.arange(N_CLIPS) * 5 % 3).astype(np.int64)

    def __len__(self):
        return N_CLIPS

    def __getitem__(self, i):
        return self.waves[i], int(self.labels[i]), {"path": f"/data/clips/clip_{i:03d}.wav"}


def test_evaluator_with_three_classes_end_to_end(nat):
    """TCNWakeword(num_classes=3) on 41 clips of 7040 samples at batch_size 16: metrics equal from_confusion of the matrix
    restated from the model's own logits (and the reference calculator's arithmetic on them), the ROC equals the reference's
    loop restated, and the width comes from the first batch."""
    from wakeword_trainer_home_amd.evaluation import ModelEvaluator, RecordingScanner
    from wakeword_trainer_home_amd.models import TCNWakeword
    from wakeword_trainer_home_amd.training import MetricResults, MetricsCalculator
    data = _Clips()
    torch.manual_seed(5)
    model = TCNWakeword(num_classes=3, dropout=0.0).to(DEV).eval()
    ev = ModelEvaluator(model, sample_rate=16000, audio_duration=N_CLIP / 16000, device=DEV, n_mels=40)
    assert ev.num_classes is None and ev.n_samples == N_CLIP
    with torch.no_grad():                                                     # spread the untrained head's answers over the classes
        feats = ev.feature_extractor(data.waves.to(DEV))
        head = model.fc[3]
        zc = model(feats)
        head.weight.mul_(4.0 / max(float(zc.std(dim=0).mean()), 1e-12))
        head.bias.sub_(model(feats).mean(dim=0))
        direct = torch.cat([model(ev.feature_extractor(data.waves[i:i + 16].to(DEV))) for i in (0, 16, 32)]).cpu()
    metrics, results = ev.evaluate_dataset(data, threshold=0.5, batch_size=16)
    logits = np.stack([r.logits for r in results])
    assert logits.shape == (N_CLIPS, 3) and np.array_equal(logits, direct.numpy())
    pred = direct.argmax(dim=1).numpy()
    print(f"measured evaluator: predicted classes {np.bincount(pred, minlength=3).tolist()}, logit std {direct.std(dim=0).tolist()}")
    assert len(set(pred.tolist())) >= 2
    matrix = MC.confusion(pred, data.labels, 3)
    assert metrics == MetricResults.from_confusion(matrix)
    assert metrics == MetricsCalculator(device="cpu").calculate(direct, torch.from_numpy(data.labels))
    assert metrics.total_samples == N_CLIPS and metrics.positive_samples == int((data.labels == 1).sum())
    conf = np.array([r.confidence for r in results], F32)
    ref = MC.softmax_conf64(direct.numpy())
    assert (np.abs(conf.astype(F64) - ref) / ref).max() <= ULP_BOUND
    assert [r.prediction for r in results] == ["Positive" if c >= F32(0.5) else "Negative" for c in conf]
    assert ev.last_counters["count"] == N_CLIPS and ev.last_counters["bad_target"] == 0
    fpr, tpr, thr = ev.get_roc_curve_data(data, batch_size=16)
    ref_fpr, ref_tpr = restated_roc(conf, data.labels, thr)                   # targets 2 are in neither rate, as in the reference loop
    assert np.array_equal(thr, roc_thresholds()) and np.array_equal(fpr, ref_fpr) and np.array_equal(tpr, ref_tpr)
    # a stated width must be the model's; the scanner takes it from the first batch as well
    with pytest.raises(ValueError, match="num_classes = 2.*3 columns"):
        ModelEvaluator(model, sample_rate=16000, audio_duration=N_CLIP / 16000, device=DEV, n_mels=40,
                       num_classes=2).evaluate_waveforms(data.waves[:4])
    scanner = RecordingScanner(model, sample_rate=16000, audio_duration=N_CLIP / 16000, threshold=0.5, device=DEV, n_mels=40, batch_size=3)
    got = scanner.scan(data.waves[3].repeat(3)[: 2 * N_CLIP])
    assert len(got) == 3 and all(0.0 <= c <= 1.0 for c, _ in got)


# --------------------------------------------------------------------------- 8. the Trainer
def _trainer(tmp_path, name, graph, batches, val, **kw):
    from wakeword_trainer_home_amd.config import get_preset
    from wakeword_trainer_home_amd.models import TCNWakeword
    from wakeword_trainer_home_amd.training import Trainer
    cfg = get_preset("cnn_small_logmel40")
    cfg.training.epochs, cfg.optimizer.warmup_epochs, cfg.training.batch_size = 2, 0, 8
    cfg.loss.label_smoothing = 0.1
    cfg.optimizer.mixed_precision = False
    cfg.training.checkpoint_frequency = "best_only"
    cfg.training.hip_graph, cfg.training.hip_graph_auto = graph, False
    cfg.model.num_classes = 3
    torch.manual_seed(11)
    model = TCNWakeword(num_classes=3, dropout=0.3, dropout_seed=2)
    return Trainer(model, batches, val, cfg, checkpoint_dir=tmp_path / name, device=DEV, **kw), model


def _clips(n, seed):
    from wakeword_trainer_home_amd.data import make_synthetic_batch
    wave, y = make_synthetic_batch(n, N_CLIP, seed=seed)
    y = (torch.arange(n) * 5 % 3).to(y.dtype)
    return [(wave[i:i + 8], y[i:i + 8]) for i in range(0, n, 8)]


def test_trainer_with_three_classes_graph_equals_eager_and_reports_the_matrix(nat, tmp_path):
    """Two epochs of three batches of 8 clips (labels 0, 1, 2), eager and with hip_graph=True.  A forward hook keeps the eager
    run's logits; the graph run, equal bit for bit, must report the same epoch metrics."""
    from wakeword_trainer_home_amd.models.losses import LabelSmoothingCrossEntropy
    from wakeword_trainer_home_amd.training import MetricResults
    batches = _clips(24, seed=6)
    runs = {}
    for name, graph in (("eager", False), ("graph", True)):
        t, model = _trainer(tmp_path, name, graph, batches, batches[:2])
        assert isinstance(t.criterion, LabelSmoothingCrossEntropy) and t.criterion.num_classes == 3 and t._async_autograd
        assert t.criterion.confusion is not None and t._confusion is t.criterion.confusion
        key = dict(t._graph_key((8, 1, 40, 45))[5])
        assert key["num_classes"] == 3 and key["confusion_ptr"] == t.criterion.confusion.data_ptr()
        seen = []
        if not graph:
            model.register_forward_hook(lambda m, i, out: seen.append((m.training, out.detach().cpu().clone())))
        rec, epochs = [], []
        t.add_callback(type("R", (), {"on_batch_end": lambda self, i, l, a: rec.append((i, l, a))})())
        for e in range(2):
            t.train_epoch(e)
            tm = t.train_metrics_tracker.compute()
            _, vm = t.validate_epoch(e)
            epochs.append((tm, vm))
        sd = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
        moments = [torch.as_tensor(v).detach().cpu().clone() for st in t.optimizer.state_dict()["state"].values() for v in st.values()]
        runs[name] = dict(t=t, rec=rec, epochs=epochs, sd=sd, moments=moments, seen=seen)
    a, b = runs["eager"], runs["graph"]
    assert b["t"]._graph is not None and a["t"]._graph is None
    losses = [l for _, l, _ in a["rec"]]
    assert len(losses) == 6 and all(np.isfinite(losses)) and len(set(losses)) > 1
    assert a["rec"] == b["rec"], "loss traces differ"
    for k in a["sd"]:
        assert torch.equal(a["sd"][k], b["sd"][k]), k
    assert len(a["moments"]) == len(b["moments"]) and all(torch.equal(u, v) for u, v in zip(a["moments"], b["moments"]))
    # the matrix, restated from the eager run's own logits: 3 training + 2 validation forwards per epoch
    assert [tr for tr, _ in a["seen"]] == ([True] * 3 + [False] * 2) * 2
    y_train = torch.cat([y for _, y in batches]).numpy()
    y_val = y_train[:16]
    for e in range(2):
        outs = a["seen"][5 * e:5 * e + 5]
        z_train, z_val = torch.cat([o for _, o in outs[:3]]).numpy(), torch.cat([o for _, o in outs[3:]]).numpy()
        want_t = MetricResults.from_confusion(MC.confusion(MC.predictions(z_train), y_train, 3))
        want_v = MetricResults.from_confusion(MC.confusion(MC.predictions(z_val), y_val, 3))
        for run in (a, b):
            tm, vm = run["epochs"][e]
            assert tm == want_t and vm == want_v, (e, tm, want_t, vm, want_v)
        assert want_t.total_samples == 24 and want_v.total_samples == 16
        assert want_t.true_positives + want_t.true_negatives + want_t.false_positives + want_t.false_negatives < 24
    # the per-step accuracy is correct / count over all three classes
    for (i, _, acc), (_, out), (_, y) in zip(a["rec"][:3], a["seen"][:3], batches):
        assert acc == float((MC.predictions(out.numpy()) == y.numpy()).sum()) / 8


def test_trainer_reports_a_target_of_three_against_the_range_and_skips_the_batch(nat, tmp_path, caplog):
    from wakeword_trainer_home_amd.training import MetricResults
    batches = _clips(16, seed=7)
    bad = batches[1][1].clone()
    bad[5] = 3
    batches[1] = (batches[1][0], bad)
    t, model = _trainer(tmp_path, "bad", False, batches, batches[:1])
    rec = []
    t.add_callback(type("R", (), {"on_batch_end": lambda self, i, l, a: rec.append(i)})())
    before = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
    with caplog.at_level(logging.ERROR):
        t.train_epoch(0)
    assert any("Target values must be in [0, 2]" in r.getMessage() for r in caplog.records)
    assert rec == [0]                                                         # the second batch was skipped
    assert t.train_metrics_tracker.compute().total_samples == 8
    assert any(not torch.equal(before[k], v.detach().cpu()) for k, v in model.state_dict().items())
