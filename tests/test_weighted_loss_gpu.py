"""GPU: ww_ce2_loss_weighted_fwd_bwd -- per-class weights and the mean / sum / none reductions -- from the kernel to the Trainer.

Tolerances follow tests/test_step_tail.py and take nothing from the kernel: every float tensor is compared with the float64
restatement (tests/weighted_loss_cases.py) under ``max(1e-6 * max|tensor|, 4 * e32)``, e32 being the error of the fp32 CPU torch
formulation on the same inputs against the same float64 values.  Counters, flags, power-of-two scalings and everything said to
equal the unweighted entry must be exact.  Each parity test prints what it measured (profiles/weighted_loss_parity_measured.txt
keeps one run's figures)."""
import functools
from pathlib import Path

import numpy as np
import pytest
import torch

from tests import weighted_loss_cases as WC

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLDEN = Path(__file__).resolve().parent / "golden"
W = tuple(float(np.float32(v)) for v in (0.55, 5.0))                       # the float32 values the kernel is handed
MODES = (("mean", "batch"), ("mean", "weight_sum"), ("sum", "batch"), ("none", "batch"), ("none", "weight_sum"))
PARITY_B = (1, 3, 64, 65, 1023, 1024, 1025, 2500)


@pytest.fixture(scope="module")
def nat():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from wakeword_trainer_home_amd import _native
    _native.load()
    return _native


def _dev(a, dtype=None):
    return torch.from_numpy(np.array(a, dtype=dtype)).to(DEV)


def _launch(nat, loss_name, z, y, weight, reduction, divisor, **extra):
    kind, h = WC.LOSSES[loss_name]
    w = None if weight is None else torch.tensor(weight, dtype=torch.float32, device=DEV)
    return nat.ce2_loss_weighted_fwd_bwd(
        _dev(z, np.float32), _dev(y, np.int64), nat.LOSS_CE if kind == "ce" else nat.LOSS_FOCAL, h.get("eps", 0.0),
        h.get("alpha", 0.25), h.get("gamma", 2.0), class_weight=w,
        reduction={"mean": nat.REDUCE_MEAN, "sum": nat.REDUCE_SUM, "none": nat.REDUCE_NONE}[reduction],
        mean_divisor={"batch": nat.DIV_BATCH, "weight_sum": nat.DIV_WEIGHT_SUM}[divisor], **extra)


def _old(nat, loss_name, z, y, **extra):
    kind, h = WC.LOSSES[loss_name]
    return nat.ce2_loss_fwd_bwd(_dev(z, np.float32), _dev(y, np.int64), nat.LOSS_CE if kind == "ce" else nat.LOSS_FOCAL,
                                h.get("eps", 0.0), h.get("alpha", 0.25), h.get("gamma", 2.0), **extra)


def _err(got, ref):
    got = got.detach().cpu().numpy() if torch.is_tensor(got) else got
    return float(np.abs(np.asarray(got, dtype=np.float64) - ref).max())


def _top(a):
    return float(np.abs(a).max())


def _close(what, got, ref, e32, where):
    """max |got - ref| <= max(1e-6 * max|ref|, 4 * e32) over the whole tensor; a NaN on either side fails.  -> err / max|ref|"""
    err, bound = _err(got, ref), max(1e-6 * _top(ref), 4.0 * e32)
    assert err <= bound, f"{where}: {what} max abs err {err:.3e} > bound {bound:.3e} (fp32 CPU e32 {e32:.3e}, max|ref| {_top(ref):.3e})"
    return err / _top(ref) if _top(ref) else err


@functools.lru_cache(maxsize=None)
def _reference(loss_name, B, targets, reduction, divisor):
    """Float64 values and the fp32 CPU formulation's error against them; computed once per case, never modified.
    -> dict(loss, grad, e_loss, e_grad [, mean, e_mean]): for 'none', ``loss`` is the vector and ``mean`` the reported scalar."""
    kind, h = WC.LOSSES[loss_name]
    z, y = WC.batch(B, targets)
    loss, grad = WC.weighted_loss(kind, z, y, W, reduction, divisor, **h)
    l32, g32 = WC.torch32(kind, z, y, W, reduction, divisor, **h)
    out = dict(loss=loss, grad=grad, e_loss=float(np.abs(l32 - loss).max()), e_grad=float(np.abs(g32 - grad).max()))
    if reduction == "none":
        mean, _ = WC.weighted_loss(kind, z, y, W, "mean", divisor, **h)
        m32, _ = WC.torch32(kind, z, y, W, "mean", divisor, **h)
        out.update(mean=mean, e_mean=abs(float(m32) - float(mean)))
    return out


def _check_parity(nat, loss_name, B, targets):
    z, y = WC.batch(B, targets)
    for reduction, divisor in MODES:
        where = f"{loss_name} B={B} targets={targets} {reduction}/{divisor}"
        r = _reference(loss_name, B, targets, reduction, divisor)
        found = torch.full((1,), 7.0, device=DEV)
        loss, vec, dl, stats = _launch(nat, loss_name, z, y, W, reduction, divisor, found_inf_out=found)
        assert (vec is not None) == (reduction == "none") and tuple(dl.shape) == (B, 2), where
        rel_g = _close("dlogits", dl, r["grad"], r["e_grad"], where)
        if reduction == "none":
            rel_v = _close("loss_vec", vec, r["loss"], r["e_loss"], where)
            rel_l = _close("reported mean", np.float64(loss.item()), np.float64(r["mean"]), r["e_mean"], where)
        else:
            rel_v = 0.0
            rel_l = _close("loss", np.float64(loss.item()), np.float64(r["loss"]), r["e_loss"], where)
        st = nat.decode_stats(stats.cpu())
        assert (st["correct"], st["tp"], st["tn"], st["fp"], st["fn"]) == WC.counters(z, y), where       # weights ignored
        assert st["count"] == B and st["nonfinite"] == 0 and st["bad_target"] == 0 and st["reserved"] == 0, where
        assert st["loss"] == loss.item() and st["grad_norm"] == 0.0 and st["found_inf"] == 0.0 and found.item() == 0.0, where
        ref_s, e_s = (r["mean"], r["e_mean"]) if reduction == "none" else (r["loss"], r["e_loss"])
        print(f"measured {where}: loss rel {rel_l:.2e} (fp32 CPU {e_s / abs(float(ref_s)):.2e})  loss_vec rel {rel_v:.2e}  "
              f"dlogits rel {rel_g:.2e} (fp32 CPU {r['e_grad'] / _top(r['grad']):.2e})")


# --------------------------------------------------------------------------- 1. parity with the float64 restatement
@pytest.mark.parametrize("B", PARITY_B)
@pytest.mark.parametrize("loss_name", list(WC.LOSSES))
def test_weighted_kernel_matches_float64_restatement(nat, loss_name, B):
    """One thread of work, less than a wave, a wave boundary, the block-stride boundary from both sides, a third trip."""
    _check_parity(nat, loss_name, B, "mixed")


@pytest.mark.parametrize("targets", ["zeros", "ones"])
@pytest.mark.parametrize("loss_name", list(WC.LOSSES))
def test_one_class_alone_in_the_weight_sum(nat, loss_name, targets):
    _check_parity(nat, loss_name, 65, targets)


# --------------------------------------------------------------------------- 2. the reference's recorded numbers
@pytest.mark.parametrize("case", WC.load_g9(GOLDEN), ids=lambda c: c["name"])
def test_g9_cases_on_the_device(nat, case):
    """Through the public classes (the factory for 'mean', as the fixture was made), against what the reference recorded;
    e32 is the recorded fp32 numbers' own distance from the float64 restatement."""
    from wakeword_trainer_home_amd.models import losses as L
    ln, red = case["loss_name"], case["reduction"]
    kind, h = WC.LOSSES[ln]
    ref_l, ref_g = WC.weighted_loss(kind, case["z"], case["y"], case["weight"], red, WC.divisor_of(ln), case["upstream"], **h)
    rec_l, rec_g = np.asarray(case["loss"], dtype=np.float64), np.asarray(case["grad"], dtype=np.float64)
    w = torch.tensor(case["weight"], dtype=torch.float32)
    if red == "mean":
        crit = L.create_loss_function({"ce0": "cross_entropy", "ce0.1": "cross_entropy", "focal": "focal_loss"}[ln],
                                      label_smoothing=h.get("eps", 0.0), focal_alpha=0.25, focal_gamma=2.0, class_weights=w, device=DEV)
        assert crit.weight.device.type == "cuda"
    else:
        cls = {"ce0": L.CrossEntropyLoss, "ce0.1": functools.partial(L.LabelSmoothingCrossEntropy, 0.1), "focal": L.FocalLoss}[ln]
        crit = cls(weight=w, reduction=red).to(DEV)
    z = _dev(case["z"], np.float32).requires_grad_()
    loss = crit(z, _dev(case["y"], np.int64))
    loss.backward(_dev(case["upstream"], np.float32) if red == "none" else None)
    assert tuple(loss.shape) == (() if red != "none" else (len(case["y"]),))
    _close("loss", loss, rec_l, float(np.abs(rec_l - ref_l).max()), case["name"])
    _close("dlogits", z.grad, rec_g, float(np.abs(rec_g - ref_g).max()), case["name"])


# --------------------------------------------------------------------------- 3. exactness against the unweighted entry
@functools.lru_cache(maxsize=None)
def _plain_batch(B):
    """Margins within +-12 or so: every gradient is a normal float, so scaling by a power of two is exact."""
    rng = np.random.default_rng(77 + B)
    z = (rng.normal(0.0, 2.0, (B, 2))).astype(np.float32)
    y = (rng.random(B) < 0.3).astype(np.int64)
    y[0], y[-1] = (0, 1) if B > 1 else (1, 1)
    return z, y


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


@pytest.mark.parametrize("B", [65, 1025])
@pytest.mark.parametrize("loss_name", list(WC.LOSSES))
def test_unit_weights_reproduce_the_unweighted_entry_bit_for_bit(nat, loss_name, B):
    z, y = _plain_batch(B)
    loss0, dl0, st0 = _old(nat, loss_name, z, y)
    st0 = st0.cpu().clone()
    assert np.abs(dl0.cpu().numpy()).min() >= 2.0 ** -100
    for weight in (None, (1.0, 1.0)):
        for divisor in ("batch", "weight_sum"):
            loss, vec, dl, st = _launch(nat, loss_name, z, y, weight, "mean", divisor)
            where = f"{loss_name} B={B} weight={weight} {divisor}"
            assert vec is None and torch.equal(_bits(loss), _bits(loss0)) and torch.equal(_bits(dl), _bits(dl0)), where
            assert torch.equal(st.cpu(), st0), where                          # all 48 bytes of ww_step_stats
    # one power of two on both classes: twice the loss and the gradient over B, cancelled over the weights' sum
    loss, _, dl, _ = _launch(nat, loss_name, z, y, (2.0, 2.0), "mean", "batch")
    assert loss.item() == 2.0 * loss0.item() and torch.equal(dl.cpu(), 2.0 * dl0.cpu())
    loss, _, dl, st = _launch(nat, loss_name, z, y, (2.0, 2.0), "mean", "weight_sum")
    assert torch.equal(_bits(loss), _bits(loss0)) and torch.equal(_bits(dl), _bits(dl0)) and torch.equal(st.cpu(), st0)


# --------------------------------------------------------------------------- 4. flags
def test_zero_weight_sum_is_nan_and_skips_under_weight_sum_but_not_under_batch(nat):
    from wakeword_trainer_home_amd.models import losses as L
    z, _ = _plain_batch(65)
    zt, yt = _dev(z), torch.zeros(65, dtype=torch.int64, device=DEV)
    w = torch.tensor([0.0, 2.0])
    crit = L.CrossEntropyLoss(weight=w).to(DEV)
    crit.found_inf_out = torch.full((1,), 7.0, device=DEV)
    loss = crit(zt, yt)
    st = nat.decode_stats(crit.last_stats.cpu())
    assert torch.isnan(loss) and np.isnan(st["loss"])                          # 0/0, as torch's weighted cross_entropy gives
    assert (st["nonfinite"], st["bad_target"], st["found_inf"], st["count"]) == (1, 0, 1.0, 65)
    assert crit.found_inf_out.item() == 1.0
    crit = L.LabelSmoothingCrossEntropy(0.1, weight=w).to(DEV)
    crit.found_inf_out = torch.full((1,), 7.0, device=DEV)
    zg = zt.clone().requires_grad_()
    loss = crit(zg, yt)
    loss.backward()
    st = nat.decode_stats(crit.last_stats.cpu())
    assert loss.item() == 0.0 and not zg.grad.any()
    assert (st["nonfinite"], st["bad_target"], st["found_inf"]) == (0, 0, 0.0) and crit.found_inf_out.item() == 0.0


@pytest.mark.parametrize("bad", [2, -1])
@pytest.mark.parametrize("reduction,divisor", MODES)
def test_bad_target_is_clamped_weighted_by_its_clamped_class_and_flagged(nat, bad, reduction, divisor):
    """Index 1500 of 2500 is reached on the block's second trip.  Apart from the flags, the outputs are those of the batch
    with the target already clamped -- so the sample took the clamped class's weight."""
    z, y = (np.array(a) for a in WC.batch(2500))
    y_bad, y_clamped = y.copy(), y.copy()
    y_bad[1500], y_clamped[1500] = bad, (1 if bad > 1 else 0)
    found = torch.full((1,), 7.0, device=DEV)
    loss, vec, dl, stats = _launch(nat, "ce0.1", z, y_bad, W, reduction, divisor, found_inf_out=found)
    loss_c, vec_c, dl_c, stats_c = _launch(nat, "ce0.1", z, y_clamped, W, reduction, divisor)
    assert torch.equal(_bits(loss), _bits(loss_c)) and torch.equal(_bits(dl), _bits(dl_c))
    assert vec is None or torch.equal(_bits(vec), _bits(vec_c))
    st, st_c = nat.decode_stats(stats.cpu()), nat.decode_stats(stats_c.cpu())
    assert (st["bad_target"], st["found_inf"], st["nonfinite"], found.item()) == (1, 1.0, 0, 1.0)
    assert (st_c["bad_target"], st_c["found_inf"]) == (0, 0.0)
    assert all(st[k] == st_c[k] for k in ("correct", "tp", "tn", "fp", "fn", "count", "loss"))


def test_module_raises_on_a_bad_target_as_the_unweighted_one_does(nat):
    from wakeword_trainer_home_amd.models import losses as L
    z, y = _plain_batch(65)
    y = y.copy()
    y[7] = 2
    for crit in (L.FocalLoss(weight=torch.tensor(W)), L.CrossEntropyLoss(reduction="sum"), L.LabelSmoothingCrossEntropy(0.1)):
        crit = crit.to(DEV)
        assert crit.validate_targets is True
        with pytest.raises(ValueError, match=r"Target values must be in \[0, 1\]"):
            crit(_dev(z), _dev(y))


@pytest.mark.parametrize("B", [65, 1025])
@pytest.mark.parametrize("loss_name", list(WC.LOSSES))
def test_loss_scale_multiplies_the_gradient_exactly_in_every_reduction(nat, loss_name, B):
    z, y = _plain_batch(B)
    ls = nat.loss_scale_new(DEV, 2.0 ** 10)
    ls[0:8].view(torch.float32)[1] = 2.0 ** 16
    for reduction, divisor in MODES:
        loss0, vec0, dl0, _ = _launch(nat, loss_name, z, y, W, reduction, divisor)
        for slot, scale in ((0, 2.0 ** 10), (1, 2.0 ** 16)):
            loss, vec, dl, _ = _launch(nat, loss_name, z, y, W, reduction, divisor, loss_scale=ls, loss_scale_slot=slot)
            where = f"{loss_name} B={B} {reduction}/{divisor} slot {slot}"
            assert torch.equal(dl.cpu(), dl0.cpu() * scale), where
            assert torch.equal(_bits(loss), _bits(loss0)) and (vec is None or torch.equal(_bits(vec), _bits(vec0))), where
    assert [nat.loss_scale_read(ls, s)["scale"] for s in (0, 1)] == [2.0 ** 10, 2.0 ** 16]


def test_argument_checks(nat):
    z, y = _plain_batch(3)
    zt, yt = _dev(z), _dev(y)
    with pytest.raises(ValueError, match="unknown reduction 3"):
        nat.ce2_loss_weighted_fwd_bwd(zt, yt, reduction=3)
    with pytest.raises(ValueError, match="unknown mean_divisor 2"):
        nat.ce2_loss_weighted_fwd_bwd(zt, yt, mean_divisor=2)
    with pytest.raises(ValueError, match="float32 of shape"):
        nat.ce2_loss_weighted_fwd_bwd(zt, yt, class_weight=torch.ones(3, device=DEV))
    with pytest.raises(nat.NativeError, match="no CPU fallback"):
        nat.ce2_loss_weighted_fwd_bwd(zt, yt, class_weight=torch.ones(2))
    lib, none_ptr = nat.load(), None
    rc = lib.ww_ce2_loss_weighted_fwd_bwd(nat.ctx(torch.device(DEV)), zt.data_ptr(), yt.data_ptr(), 3, nat.LOSS_CE, 0.0, 0.25, 2.0,
                                          none_ptr, nat.REDUCE_NONE, nat.DIV_BATCH, none_ptr, none_ptr, torch.empty_like(zt).data_ptr(),
                                          none_ptr, none_ptr, none_ptr, 0, none_ptr)
    assert rc == -1 and b"needs loss_vec" in lib.ww_last_error()


def test_weight_on_another_device_raises_instead_of_copying(nat):
    from wakeword_trainer_home_amd.models import losses as L
    z, y = _plain_batch(3)
    crit = L.FocalLoss(weight=torch.tensor(W))                                 # never moved: the buffer is still on the CPU
    with pytest.raises(ValueError, match=r"move the criterion with \.to\(device\)"):
        crit(_dev(z), _dev(y))
    with pytest.raises(ValueError, match=r"move the criterion with \.to\(device\)"):
        crit.native_fwd_bwd(_dev(z), _dev(y))


# --------------------------------------------------------------------------- 5. autograd
@pytest.mark.parametrize("loss_name", list(WC.LOSSES))
def test_none_reduction_through_autograd(nat, loss_name):
    from wakeword_trainer_home_amd.models import losses as L
    kind, h = WC.LOSSES[loss_name]
    B = 1025
    z, y = WC.batch(B)
    up = np.random.default_rng(9).normal(size=B).astype(np.float32)
    make = {"ce0": L.CrossEntropyLoss, "ce0.1": functools.partial(L.LabelSmoothingCrossEntropy, 0.1), "focal": L.FocalLoss}[loss_name]
    crit = make(weight=torch.tensor(W), reduction="none").to(DEV)
    zt = _dev(z).requires_grad_()
    loss = crit(zt, _dev(y))
    assert tuple(loss.shape) == (B,)
    loss.backward(_dev(up))
    ref_l, ref_g = WC.weighted_loss(kind, z, y, W, "none", upstream=up, **h)
    l32, g32 = WC.torch32(kind, z, y, W, "none", upstream=up, **h)
    _close("per-sample loss", loss, ref_l, float(np.abs(l32 - ref_l).max()), loss_name)
    _close("w_b g_b gout_b", zt.grad, ref_g, float(np.abs(g32 - ref_g).max()), loss_name)
    # .sum().backward() on the per-sample losses is the 'sum' loss's gradient, bit for bit
    z1 = _dev(z).requires_grad_()
    crit(z1, _dev(y)).sum().backward()
    z2 = _dev(z).requires_grad_()
    total = make(weight=torch.tensor(W), reduction="sum").to(DEV)(z2, _dev(y))
    total.backward()
    assert tuple(total.shape) == () and torch.equal(_bits(z1.grad), _bits(z2.grad))


# --------------------------------------------------------------------------- 6. through a model
def test_weighted_route_reaches_the_model_step(nat):
    """cnn_small, fp32, B = 8: the backward kernels are linear in dlogits, so weights of (2, 2) double the flat gradient
    exactly over B and leave it untouched over the weights' sum."""
    from tests.golden_util import make_inputs
    from wakeword_trainer_home_amd.models import create_model
    from wakeword_trainer_home_amd.models import losses as L
    x, y = make_inputs(41, 8)
    x, y = x.to(DEV), y.to(DEV)
    torch.manual_seed(3)
    model = create_model("cnn_small", dropout=0.3, dropout_seed=5).to(DEV).to(memory_format=torch.channels_last).train()
    two = torch.tensor([2.0, 2.0])

    def flat_grad(crit):
        crit = crit.to(DEV)
        for p in model.parameters():
            p.grad = None
        model.dropout_step = 0                                               # the same dropout masks every time
        flag = torch.full((1,), 7.0, device=DEV)
        stats = model.train_step_native(x, y, crit, found_inf_out=flag)
        st = nat.decode_stats(stats.cpu())
        assert (st["nonfinite"], st["bad_target"], st["found_inf"], st["count"], flag.item()) == (0, 0, 0.0, 8, 0.0)
        return model.flat_grad.detach().cpu().clone(), st

    g_ls, st_ls = flat_grad(L.LabelSmoothingCrossEntropy(0.1))
    g_ls2, st_ls2 = flat_grad(L.LabelSmoothingCrossEntropy(0.1, weight=two))
    assert g_ls.abs().max() > 0 and torch.equal(g_ls2, 2.0 * g_ls) and st_ls2["loss"] == 2.0 * st_ls["loss"]
    g_ce, st_ce = flat_grad(L.CrossEntropyLoss())
    g_ce2, st_ce2 = flat_grad(L.CrossEntropyLoss(weight=two))
    assert g_ce.abs().max() > 0 and torch.equal(_bits(g_ce2), _bits(g_ce)) and st_ce2 == st_ce
    assert all(st_ls[k] == st_ls2[k] for k in ("correct", "tp", "tn", "fp", "fn"))


# --------------------------------------------------------------------------- 7. Trainer
def _trainer(tmp_path, name, graph, **kw):
    from wakeword_trainer_home_amd.config import get_preset
    from wakeword_trainer_home_amd.models import create_model
    from wakeword_trainer_home_amd.training import Trainer
    from tests.golden_util import make_inputs
    cfg = get_preset("cnn_small_logmel40")
    cfg.training.epochs, cfg.training.batch_size, cfg.optimizer.warmup_epochs = 1, 8, 0
    cfg.optimizer.mixed_precision = False
    cfg.model.dropout = 0.3
    cfg.training.hip_graph, cfg.training.hip_graph_auto = graph, False
    cfg.training.checkpoint_frequency = "best_only"
    x, y = make_inputs(17, 8 * 4)
    y[::4] = 1
    batches = [(x[8 * i:8 * i + 8], y[8 * i:8 * i + 8]) for i in range(4)]
    torch.manual_seed(7)
    model = create_model("cnn_small", dropout=cfg.model.dropout, dropout_seed=3)
    t = Trainer(model, batches[:3], batches[:1], cfg, checkpoint_dir=tmp_path / name, device=DEV, **kw)
    rec = []
    t.add_callback(type("R", (), {"on_batch_end": lambda self, i, l, a: rec.append((i, l, a))})())
    return t, model, rec, batches


def _state(model, t):
    sd = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
    moments = [torch.as_tensor(v).detach().cpu().clone() for st in t.optimizer.state_dict()["state"].values() for v in st.values()]
    return sd, moments


def _assert_same_state(a, b):
    bits = lambda v: v.contiguous().view(torch.int32) if v.dtype == torch.float32 else v
    assert a[0].keys() == b[0].keys() and len(a[1]) == len(b[1])
    for k in a[0]:
        assert torch.equal(bits(a[0][k]), bits(b[0][k])), k
    for u, v in zip(a[1], b[1]):
        assert torch.equal(u, v)


def test_trainer_with_class_weights_graph_equals_eager_and_reads_the_weight_at_replay(tmp_path):
    from wakeword_trainer_home_amd.models.losses import LabelSmoothingCrossEntropy
    from wakeword_trainer_home_amd.training import Trainer
    w = torch.tensor(W)
    captures, orig = [], Trainer._graph_capture

    def counting(self, feats):
        captures.append(tuple(feats.shape))
        return orig(self, feats)
    runs = {}
    Trainer._graph_capture = counting
    try:
        for name, graph in (("eager", False), ("graph", True)):
            t, model, rec, batches = _trainer(tmp_path, name, graph, class_weights=w)
            assert isinstance(t.criterion, LabelSmoothingCrossEntropy) and t.criterion.weight.device.type == "cuda"
            assert torch.equal(t.criterion.weight.cpu(), w)
            t.train_epoch(0)                                                 # three steps: eager, eager (captured after it), replayed
            after3 = (_state(model, t), list(rec))
            key = t._graph_key((8, 1, 40, 151))
            t.criterion.weight.fill_(1.0)                                    # in place: same pointer, new values
            assert t._graph_key((8, 1, 40, 151)) == key
            t.train_loader = batches[3:4]
            t.train_epoch(1)                                                 # one more step
            runs[name] = (after3, (_state(model, t), list(rec)), t)
    finally:
        Trainer._graph_capture = orig
    assert captures == [(8, 1, 40, 151)]                                     # the graph run captured once; no recapture for new values
    assert runs["graph"][2]._graph is not None and runs["eager"][2]._graph is None
    for stage in (0, 1):
        assert runs["eager"][stage][1] == runs["graph"][stage][1], "loss traces differ"      # float equality
        _assert_same_state(runs["eager"][stage][0], runs["graph"][stage][0])
    assert len(runs["graph"][1][1]) == 4                                     # (a graph that had baked (0.55, 5) would differ in step 4)


def test_trainer_argument_rules(tmp_path):
    from wakeword_trainer_home_amd.models.losses import CrossEntropyLoss, LabelSmoothingCrossEntropy
    with pytest.raises(ValueError, match="either criterion or class_weights"):
        _trainer(tmp_path, "both", False, criterion=CrossEntropyLoss(), class_weights=torch.tensor(W))
    with pytest.raises(ValueError, match="reduction='none'"):
        _trainer(tmp_path, "none", False, criterion=LabelSmoothingCrossEntropy(0.1, reduction="none"))
    t, _, _, _ = _trainer(tmp_path, "sum", False, criterion=LabelSmoothingCrossEntropy(0.1, reduction="sum"))
    assert t.criterion.reduction == "sum"
    # without the argument nothing changes, whatever config.loss.class_weights says
    t, _, _, _ = _trainer(tmp_path, "plain", False)
    assert t.config.loss.class_weights == "balanced"
    assert type(t.criterion) is LabelSmoothingCrossEntropy and t.criterion.weight is None and t.criterion.reduction == "mean"
    k = dict(t._graph_key((8, 1, 40, 151))[5])
    assert (k["reduction"], k["weight"], k["weight_ptr"]) == ("mean", False, None)
    t2, _, _, _ = _trainer(tmp_path, "weighted", False, class_weights=torch.tensor(W))
    k2 = dict(t2._graph_key((8, 1, 40, 151))[5])
    assert (k2["reduction"], k2["weight"], k2["weight_ptr"]) == ("mean", True, t2.criterion.weight.data_ptr())


def test_clip_bank_class_stats_feed_the_balanced_weights(nat):
    from wakeword_trainer_home_amd.data import DeviceClipBank
    from wakeword_trainer_home_amd.training import class_weights_from_config
    from types import SimpleNamespace
    labels = np.zeros(2000, dtype=np.int64)
    labels[::10] = 1                                                         # 200 positives against 1800 negatives
    bank = DeviceClipBank(torch.zeros(2000, 8, dtype=torch.int16), labels, device=DEV)
    assert bank.class_stats() == {"positive": 200, "negative": 1800}
    w = class_weights_from_config(SimpleNamespace(loss=SimpleNamespace(class_weights="balanced")), bank.class_stats(), DEV)
    assert w.device.type == "cuda" and w.dtype == torch.float32 and w.tolist() == [pytest.approx(2000 / 3600), pytest.approx(5.0)]
    assert DeviceClipBank(torch.zeros(3, 8, dtype=torch.int16), [1, 1, 1], device=DEV).class_stats() == {"positive": 3, "negative": 0}
