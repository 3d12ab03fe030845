"""The step tail every model ends with -- ww_ce2_loss_fwd_bwd, ww_grad_norm_clip, ww_clip_optim_step -- called directly on
plain tensors, per dispatch arm, against the float64 oracles (oracle/optim.py, oracle/losses.py).

ww_clip_optim_step has three arms: one block (n <= 4096), a scalar grid (4096 < n < 65536, or any bucket off the 16-byte
grid) and a float4 grid (n >= 65536); ww_grad_norm_clip switches from one block to block partials above n = 65536; the loss
kernel is one 1024-thread block that strides over the batch.  The sizes below sit on both sides of each switch, on the float4
tail lengths, and far enough out (2 100 003) for a second grid-stride trip and the cap of 256 block partials.

Tolerances.  No bound is taken from the kernels.  Every float tensor is compared with the float64 oracle under
``max(floor, 4 * e32)``: e32 is the error, against the same oracle and on the same inputs, of the fp32 CPU formulation
(torch.optim and clip_grad_norm_ on float32 tensors; torch.nn.functional.cross_entropy and a few-line fp32 focal loss with
autograd), the factor 4 allows for another contraction and reduction order on the device, and the floor is 2e-6 absolute for
parameters of O(1), 1e-5 relative for norms and 1e-6 of the tensor's largest value for moments, clipped gradients, loss
gradients and the loss.  Every hyper-parameter is a float32 value (the C structs hold floats), so the oracle, the fp32
formulation and the kernel are handed the same numbers.  Integer state, flags and the power-of-two scales must be exact."""
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def nat():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from wakeword_trainer_home_amd import _native
    _native.load()
    return _native


def _f32(x):
    return float(np.float32(x))


BETAS = (_f32(0.9), _f32(0.999))
WD, MOM = _f32(1e-2), _f32(0.9)
LRS = (_f32(3e-3), _f32(1e-3), _f32(1e-2), _f32(3e-3))                 # call k runs at LRS[k % 4]: a scheduler at work
# name -> (kind, weight decay, momentum, eps).  Adam's L2 term adds wd * p to the gradient, and among two million elements a
# few of those sums cancel to within fp32 rounding; the first update, lr * g / (|g| + eps), of such an element is decided by
# that rounding when eps is torch's default 1e-8 (measured on the CPU: the fp32 formulation is then 4e-3 off the oracle at
# n = 2 100 003).  So that rule runs at eps = 1e-4, where every element's update is well conditioned and eps carries weight
# in the denominator; the decoupled rules, whose gradients are not sums, keep the default.
RULES = {
    "adam-l2": ("adam", WD, 0.0, _f32(1e-4)),
    "adamw": ("adamw", WD, 0.0, _f32(1e-8)),
    "adamw-nodecay": ("adamw", 0.0, 0.0, _f32(1e-8)),
    "sgd-nesterov": ("sgd", WD, MOM, 0.0),
    "sgd-plain": ("sgd", 0.0, 0.0, 0.0),     # no momentum, exp_avg_sq = None
}
PLANTED = (0.0, 1e-12, -1e-12, 0.0, -1e-12, 1e-12)                     # exact zeros and tiny values at the front of every gradient


def _misaligned(t):
    """A contiguous device copy of ``t`` that starts one float into a larger buffer: never 16-byte aligned."""
    buf = torch.empty(t.numel() + 1, dtype=torch.float32, device=DEV)
    v = buf[1:].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % 16 == 4
    return v


def _torch_opt(rule, q):
    kind, wd, mom, eps = RULES[rule]
    if kind == "adam":
        return torch.optim.Adam([q], lr=LRS[0], betas=BETAS, eps=eps, weight_decay=wd)
    if kind == "adamw":
        return torch.optim.AdamW([q], lr=LRS[0], betas=BETAS, eps=eps, weight_decay=wd)
    return torch.optim.SGD([q], lr=LRS[0], momentum=mom, weight_decay=wd, nesterov=mom > 0)


def _maxabs(a, b):
    return float(np.abs(np.asarray(a, dtype=np.float64) - b).max())


@functools.lru_cache(maxsize=2)
def _reference(rule, n, max_norm, plan="aaaa"):
    """The float64 trajectory of ``len(plan)`` calls ('a' = applied, 's' = skipped: clipped, nothing else) and, beside it, the
    fp32 CPU formulation's error e32 against it.  -> (p0, grads, calls); computed once per case and shared, never modified."""
    from oracle import optim as OO
    kind, wd, mom, eps = RULES[rule]
    gen = torch.Generator().manual_seed(1000 * len(plan) + n % 997)
    p0 = torch.randn(n, generator=gen)
    grads = []
    for k in range(len(plan)):
        g = torch.randn(n, generator=gen) * (3.0 if k % 2 else 0.01)    # under and over the clip threshold in turn
        if n > len(PLANTED):
            g[:len(PLANTED)] = torch.tensor(PLANTED)
        grads.append(g)
    q = torch.nn.Parameter(p0.clone())
    topt = _torch_opt(rule, q)
    p, m, v = p0.numpy().astype(np.float64), np.zeros(n), np.zeros(n)
    t, calls = 0, []
    for k, what in enumerate(plan):
        lr = LRS[k % 4]
        norm, gc = OO.clip_grad_norm(grads[k].numpy(), max_norm)
        q.grad = grads[k].clone()
        n32 = torch.nn.utils.clip_grad_norm_([q], max_norm) if max_norm > 0 else q.grad.norm()
        e32 = {"norm": abs(n32.item() - norm), "g": _maxabs(q.grad.numpy(), gc)}
        if what == "a":
            t += 1
            p, m, v = OO.optim_step(kind, p, gc, m, v, t, lr, BETAS, eps, wd, mom)
            for gp in topt.param_groups:
                gp["lr"] = lr
            topt.step()
        st = topt.state.get(q, {})
        m32 = st.get("exp_avg", st.get("momentum_buffer"))
        v32 = st.get("exp_avg_sq")
        e32["p"] = _maxabs(q.detach().numpy(), p)
        e32["m"] = _maxabs(np.zeros(n) if m32 is None else m32.numpy(), m)
        e32["v"] = _maxabs(np.zeros(n) if v32 is None else v32.numpy(), v)
        calls.append(SimpleNamespace(lr=lr, t=t, norm=norm, g=gc, p=p, m=m, v=v, e32=e32))
    return p0, tuple(grads), tuple(calls)


def _close(what, got, ref, e32, floor, where):
    """max |got - ref| <= max(floor, 4 * e32) over the WHOLE tensor; a NaN on either side fails."""
    err = _maxabs(got.detach().cpu().numpy() if torch.is_tensor(got) else got, ref)
    bound = max(floor, 4.0 * e32)
    assert err <= bound, f"{where}: {what} max abs err {err:.3e} > bound {bound:.3e} (floor {floor:.1e}, fp32 CPU e32 {e32:.3e})"


def _top(a):
    return float(np.abs(a).max())


def _check_call(c, where, p, m, v, bucket=None, norm=None):
    """Device tensors after one call against call record ``c`` of _reference."""
    _close("params", p, c.p, c.e32["p"], 2e-6, where)
    if m is not None:
        _close("exp_avg", m, c.m, c.e32["m"], 1e-6 * _top(c.m), where)
    if v is not None:
        _close("exp_avg_sq", v, c.v, c.e32["v"], 1e-6 * _top(c.v), where)
    if bucket is not None:
        _close("clipped gradients", bucket, c.g, c.e32["g"], 1e-6 * _top(c.g), where)
    if norm is not None:
        _close("grad norm", np.float64(norm), c.norm, c.e32["norm"], 1e-5 * c.norm, where)


def _cfg(nat, rule, lr, max_norm):
    kind, wd, mom, eps = RULES[rule]
    code = {"adam": nat.OPT_ADAM, "adamw": nat.OPT_ADAMW, "sgd": nat.OPT_SGD}[kind]
    return nat.OptimCfg(code, lr, BETAS[0], BETAS[1], eps, wd, mom, max_norm)


def _buffers(rule, p0, misaligned=False):
    n = p0.numel()
    p = _misaligned(p0) if misaligned else p0.to(DEV)
    m = torch.zeros(n, device=DEV)
    v = None if rule == "sgd-plain" else torch.zeros(n, device=DEV)
    return p, m, v


def _stats(nat, found_inf=0.0):
    """A device ww_step_stats as the loss kernel leaves it, with recognisable counters."""
    s = nat.StepStats(0.25, 0.0, 3, 1, 2, 4, 5, 0, 0, 9, found_inf, 0)
    return torch.frombuffer(bytearray(bytes(s)), dtype=torch.uint8).to(DEV)


def _pinned(fill):
    return torch.full((48,), fill, dtype=torch.uint8).pin_memory()


# --------------------------------------------------------------------------- a. optimizer arms x update rules
_FULL = (1025, 4097, 65539)                                             # one size per arm gets every rule
_ONE = ((1, "adam-l2"), (1023, "sgd-nesterov"), (4096, "adamw"), (65535, "adam-l2"), (65536, "sgd-nesterov"),
        (65537, "adamw-nodecay"), (2100003, "adam-l2"))
_OFF_GRID = {(65539, "adamw"), (2100003, "adam-l2")}                    # repeated with the parameter bucket misaligned


def _arm_cases():
    pairs = [(n, r) for n in _FULL for r in RULES] + list(_ONE)
    out = []
    for n, r in sorted(pairs, key=lambda c: c[0]):
        for max_norm in (0.0, 1.0):
            for mis in ((False, True) if (n, r) in _OFF_GRID else (False,)):        # neighbours: they share one reference
                out.append(pytest.param(n, r, max_norm, mis, id=f"{n}-{r}-clip{max_norm:g}" + ("-misaligned" if mis else "")))
    return out


@pytest.mark.parametrize("n,rule,max_norm,misaligned", _arm_cases())
def test_optimizer_arm_matches_float64_oracle(nat, n, rule, max_norm, misaligned):
    p0, grads, calls = _reference(rule, n, max_norm)
    p, m, v = _buffers(rule, p0, misaligned)
    state = torch.zeros(2, dtype=torch.int64, device=DEV)
    norm = torch.zeros(1, device=DEV)
    for k, c in enumerate(calls):
        parity = k & 1
        bucket = grads[k].to(DEV)
        nat.clip_optim_step_(_cfg(nat, rule, c.lr, max_norm), p, bucket, m, v, state, parity, norm_out=norm)
        where = f"n={n} {rule} max_norm={max_norm:g} step {k}"
        st = state.tolist()
        assert st[parity ^ 1] == k + 1 and st[parity] == k, (where, st)      # the slot written, and the slot left alone
        _check_call(c, where, p, m, v, bucket, norm.item())
        if max_norm == 0:
            assert torch.equal(bucket.cpu(), grads[k]), where                # nothing to clip: the bucket is not touched


# --------------------------------------------------------------------------- b. skips, per arm
@pytest.mark.parametrize("cause", ["nan_gradient", "stats_found_inf", "found_inf_extra"])
@pytest.mark.parametrize("n", _FULL)
def test_skipped_step_changes_nothing_and_is_not_counted(nat, n, cause):
    """applied, skipped, applied: the skip leaves parameters, moments and the step count bit-identical, flags the record,
    and the step after it continues from step count t, not t + 1."""
    rule, max_norm = "adamw", 1.0
    p0, grads, calls = _reference(rule, n, max_norm, "asa")
    p, m, v = _buffers(rule, p0)
    state = torch.zeros(2, dtype=torch.int64, device=DEV)
    norm = torch.zeros(1, device=DEV)
    for k, c in enumerate(calls):
        parity, skip = k & 1, k == 1
        where = f"n={n} {cause} call {k}"
        g = grads[k].clone()
        if skip and cause == "nan_gradient":
            g[n // 2] = float("nan")
        bucket = g.to(DEV)
        stats = _stats(nat, 1.0 if skip and cause == "stats_found_inf" else 0.0)
        extra = torch.full((1,), 1.0 if skip and cause == "found_inf_extra" else 0.0, device=DEV)
        host = _pinned(0xAB)
        before = (p.clone(), m.clone(), v.clone())
        nat.clip_optim_step_(_cfg(nat, rule, c.lr, max_norm), p, bucket, m, v, state, parity, norm_out=norm, stats=stats,
                             stats_host=host, found_inf_extra=extra)
        torch.cuda.synchronize()
        st, rec = state.tolist(), nat.decode_stats(stats.cpu())
        assert torch.equal(host, stats.cpu()), where                         # the pinned copy is the device record, all 48 bytes
        assert (rec["loss"], rec["correct"], rec["tp"], rec["tn"], rec["fp"], rec["fn"], rec["count"]) == (0.25, 3, 1, 2, 4, 5, 9)
        if skip:
            assert all(torch.equal(a, b) for a, b in zip((p, m, v), before)), where
            assert st[parity ^ 1] == st[parity] == c.t, (where, st)
            assert rec["found_inf"] == 1.0, where
            if cause == "nan_gradient":
                assert np.isnan(rec["grad_norm"]) and np.isnan(norm.item()), where
            else:
                _close("stats.grad_norm", np.float64(rec["grad_norm"]), c.norm, c.e32["norm"], 1e-5 * c.norm, where)
                _close("clipped gradients", bucket, c.g, c.e32["g"], 1e-6 * _top(c.g), where)
        else:
            assert st[parity ^ 1] == c.t and st[parity] == c.t - 1, (where, st)
            assert rec["found_inf"] == 0.0 and rec["grad_norm"] == norm.item(), where
            _check_call(c, where, p, m, v, bucket, norm.item())
    assert calls[-1].t == 2


# --------------------------------------------------------------------------- c. loss scale, per arm
def _scale_slots(nat, ls):
    return [(nat.loss_scale_read(ls, s)["scale"], nat.loss_scale_read(ls, s)["growth_tracker"]) for s in (0, 1)]


@pytest.mark.parametrize("n", _FULL)
def test_loss_scale_is_divided_out_and_follows_gradscaler(nat, n):
    """Gradients arrive times scale[parity]; parameters, moments and the bucket left behind are those of the unscaled run.
    Three applied steps double the scale, an inf gradient halves it and skips, a batch skipped for found_inf leaves it alone;
    then one applied step and a second overflow, so that the tracker reset shows."""
    from oracle.optim import grad_scaler_update
    rule, max_norm, interval = "adamw", 1.0, 3
    plan = "aaaofao"                                                         # o = overflow, f = skipped for found_inf
    p0, grads, calls = _reference(rule, n, max_norm, plan.replace("o", "s").replace("f", "s"))
    p, m, v = _buffers(rule, p0)
    state = torch.zeros(2, dtype=torch.int64, device=DEV)
    norm = torch.zeros(1, device=DEV)
    ls = nat.loss_scale_new(DEV, 2.0 ** 10, growth_interval=interval)
    slots = [(2.0 ** 10, 0), (2.0 ** 10, 0)]
    assert _scale_slots(nat, ls) == slots
    for k, (what, c) in enumerate(zip(plan, calls)):
        parity = k & 1
        where = f"n={n} call {k} ({what})"
        scale = slots[parity][0]
        g = grads[k].clone()
        if what == "o":
            g[n // 3] = float("inf")
        bucket = (g * scale).to(DEV)                                         # a power of two: exact
        stats = _stats(nat, 1.0 if what == "f" else 0.0)
        before = (p.clone(), m.clone(), v.clone())
        nat.clip_optim_step_(_cfg(nat, rule, c.lr, max_norm), p, bucket, m, v, state, parity, norm_out=norm, stats=stats,
                             loss_scale=ls)
        slots[parity ^ 1] = grad_scaler_update(*slots[parity], 2.0, 0.5, interval, grads_nonfinite=what == "o", skipped=what != "a")
        assert _scale_slots(nat, ls) == slots, where                         # slot parity^1 written, slot parity untouched
        st = state.tolist()
        assert st[parity ^ 1] == c.t and st[parity] == (c.t - 1 if what == "a" else c.t), (where, st)
        assert nat.decode_stats(stats.cpu())["found_inf"] == (0.0 if what == "a" else 1.0), where
        if what == "a":
            _check_call(c, where, p, m, v, bucket, norm.item())
        else:
            assert all(torch.equal(a, b) for a, b in zip((p, m, v), before)), where
            if what == "f":
                _check_call(c, where, p, m, v, bucket, norm.item())          # unscaled and clipped all the same
            else:
                assert np.isinf(norm.item()), where
    assert [s for s, _ in slots] == [2.0 ** 10, 2.0 ** 9] and calls[-1].t == 4


# --------------------------------------------------------------------------- d. bound control block
@pytest.mark.parametrize("n", [1025, 4097])
def test_bound_step_ctl_supplies_lr_and_parity(nat, n):
    """With a bound ww_step_ctl the learning rate and the slot come from device memory: cfg.lr = 0 is accepted, the parity
    argument is ignored, and the record goes to stats_host_alt at parity 1, to stats_host at parity 0."""
    rule, max_norm = "adamw", 1.0
    p0, grads, calls = _reference(rule, n, max_norm, "aa")
    p, m, v = _buffers(rule, p0)
    state = torch.tensor([10, 0], dtype=torch.int64, device=DEV)              # slot 1 holds the count; slot 0 is a decoy
    norm = torch.zeros(1, device=DEV)
    ctl = nat.step_ctl_new(DEV, step=0, lr=calls[0].lr, parity=1)
    host, alt = _pinned(0xAB), _pinned(0xCD)
    nat.bind_step_ctl(DEV, ctl)
    try:
        cfg = _cfg(nat, rule, 0.0, max_norm)
        stats, bucket = _stats(nat), grads[0].to(DEV)
        nat.clip_optim_step_(cfg, p, bucket, m, v, state, 0, norm_out=norm, stats=stats, stats_host=host, stats_host_alt=alt)
        torch.cuda.synchronize()
        assert state.tolist() == [1, 0]                                      # read slot 1 (the block's parity), wrote slot 0
        assert torch.equal(alt, stats.cpu()) and bool((host == 0xAB).all())
        _check_call(calls[0], f"n={n} ctl parity 1", p, m, v, bucket, norm.item())
        nat.step_ctl_advance(DEV)
        nat.step_ctl_write(ctl, lr=calls[1].lr)
        assert nat.step_ctl_read(ctl)["parity"] == 0 and nat.step_ctl_read(ctl)["step"] == 1
        first = alt.clone()
        stats, bucket = _stats(nat), grads[1].to(DEV)
        nat.clip_optim_step_(cfg, p, bucket, m, v, state, 1, norm_out=norm, stats=stats, stats_host=host, stats_host_alt=alt)
        torch.cuda.synchronize()
        assert state.tolist() == [1, 2]
        assert torch.equal(host, stats.cpu()) and torch.equal(alt, first)
        _check_call(calls[1], f"n={n} ctl parity 0", p, m, v, bucket, norm.item())
    finally:
        nat.bind_step_ctl(DEV, None)                                         # the context is shared by every test of the process


# --------------------------------------------------------------------------- e. loss kernel
MARGINS = (0.0,) + tuple(s * a for a in (1e-3, 1.0, 15.0, 17.5, 30.0, 90.0, 200.0) for s in (1.0, -1.0))
LOSSES = [("ce", dict(eps=0.0)), ("ce", dict(eps=_f32(0.1))), ("focal", dict(alpha=0.25, gamma=2.0)),
          ("focal", dict(alpha=0.75, gamma=0.5)), ("focal", dict(alpha=0.25, gamma=0.0))]
LOSS_B = (1, 1023, 1024, 1025, 2500)


@functools.lru_cache(maxsize=None)
def _loss_batch(B):
    """(logits (B,2) f32, targets (B,) i64): every margin z1 - z0 of MARGINS with both labels, in an order that has no
    period in common with the block.  A margin of 0 is an exact tie; none lies within 0.5 of 16.118, where focal's p_t
    clamp makes the reference's own gradient discontinuous."""
    combos = [(mg, y) for mg in MARGINS for y in (0, 1)]
    pick = (np.arange(B) * 7) % len(combos)
    z0 = np.random.default_rng(B).normal(0.0, 1.0, B).astype(np.float32)
    z1 = (z0 + np.array([combos[i][0] for i in pick], np.float32)).astype(np.float32)
    z = np.stack([z0, z1], axis=1)
    assert not ((np.abs(np.abs(z[:, 1].astype(np.float64) - z[:, 0]) - 16.118) < 0.5).any())
    return z, np.array([combos[i][1] for i in pick], np.int64)


@functools.lru_cache(maxsize=None)
def _loss_reference(B, li):
    """-> (loss, B * dlogits) of the float64 oracle and the fp32 CPU formulation's error against each."""
    from oracle import losses as OL
    from oracle.train_step import TorchLoss
    kind, kw = LOSSES[li]
    z, y = _loss_batch(B)
    zt = torch.from_numpy(z.copy()).requires_grad_()
    if kind == "ce":
        loss, d = OL.ce_label_smoothing(z, y, kw["eps"])
        # the reference smooths to (1 - eps, eps/(C-1)), torch to (1 - e + e/C, e/C): the same target at C = 2 with e = 2 eps
        l32 = torch.nn.functional.cross_entropy(zt, torch.from_numpy(y), label_smoothing=2.0 * kw["eps"])
    else:
        loss, d = OL.focal(z, y, kw["alpha"], kw["gamma"])
        l32 = TorchLoss("focal", alpha=kw["alpha"], gamma=kw["gamma"])(zt, torch.from_numpy(y))
    l32.backward()
    return float(loss), B * d, abs(l32.item() - float(loss)), _maxabs(B * zt.grad.numpy().astype(np.float64), B * d)


def _native_loss(nat, B, li, **extra):
    kind, kw = LOSSES[li]
    z, y = _loss_batch(B)
    zt, yt = torch.from_numpy(z).to(DEV), torch.from_numpy(y).to(DEV)
    if kind == "ce":
        return nat.ce2_loss_fwd_bwd(zt, yt, nat.LOSS_CE, kw["eps"], **extra)
    return nat.ce2_loss_fwd_bwd(zt, yt, nat.LOSS_FOCAL, 0.0, kw["alpha"], kw["gamma"], **extra)


@pytest.mark.parametrize("li", range(len(LOSSES)), ids=lambda i: LOSSES[i][0] + "-" + "-".join(f"{v:g}" for v in LOSSES[i][1].values()))
@pytest.mark.parametrize("B", LOSS_B)
def test_loss_kernel_matches_float64_oracle(nat, B, li):
    """B * dlogits against B * the oracle's gradient, so that a large batch does not loosen the bound; the loss to 1e-6
    relative (every sample's term is non-negative and good to a few fp32 ulp, the sum is taken in double and rounded once);
    the counters exactly."""
    from oracle.losses import batch_counters
    z, y = _loss_batch(B)
    ref_loss, ref_d, e_loss, e_d = _loss_reference(B, li)
    found = torch.full((1,), 7.0, device=DEV)
    loss, dl, stats = _native_loss(nat, B, li, found_inf_out=found)
    where = f"B={B} {LOSSES[li]}"
    _close("loss", np.float64(loss.item()), ref_loss, e_loss, 1e-6 * abs(ref_loss), where)
    _close("B * dlogits", B * dl.cpu().numpy().astype(np.float64), ref_d, e_d, 1e-6 * _top(ref_d), where)
    st = nat.decode_stats(stats.cpu())
    assert (st["correct"], st["tp"], st["tn"], st["fp"], st["fn"]) == batch_counters(z, y), where
    assert st["count"] == B and st["nonfinite"] == 0 and st["bad_target"] == 0 and st["reserved"] == 0, where
    assert st["loss"] == loss.item() and st["grad_norm"] == 0.0 and st["found_inf"] == 0.0 and found.item() == 0.0, where
    assert (z[:, 0] == z[:, 1]).any()                                        # ties are in: they count as class 0 above


@pytest.mark.parametrize("li", [1, 2], ids=["ce-0.1", "focal-0.25-2"])
@pytest.mark.parametrize("B", [1, 2500])
def test_loss_scale_multiplies_dlogits_by_the_chosen_slot(nat, B, li):
    """dlogits times scale[slot] for either slot, the reported loss unchanged.  The scales are powers of two, so the scaled
    gradient is the unscaled one bit for bit -- wherever the unscaled value is a normal float; an unscaled value below
    2^-126 (a margin of 90 leaves e^-90 / B) has already lost bits that the scaled one keeps, and may differ from it by
    one unit of the subnormal grid, 2^-149, times the scale."""
    ls = nat.loss_scale_new(DEV, 2.0 ** 10)
    ls[0:8].view(torch.float32)[1] = 2.0 ** 16
    assert [nat.loss_scale_read(ls, s)["scale"] for s in (0, 1)] == [2.0 ** 10, 2.0 ** 16]
    loss0, dl0, _ = _native_loss(nat, B, li)
    plain = dl0.cpu().numpy().astype(np.float64)
    for slot, scale in ((0, 2.0 ** 10), (1, 2.0 ** 16)):
        loss, dl, _ = _native_loss(nat, B, li, loss_scale=ls, loss_scale_slot=slot)
        assert loss.item() == loss0.item()
        diff = np.abs(dl.cpu().numpy().astype(np.float64) - plain * scale)
        allowed = np.where(np.abs(plain) >= 2.0 ** -126, 0.0, scale * 2.0 ** -149)
        assert (diff <= allowed).all(), f"B={B} slot {slot}: {int((diff > allowed).sum())} elements differ, max {diff.max():.3e}"
        assert (np.abs(plain) >= 2.0 ** -126).sum() > plain.size // 2
    assert [nat.loss_scale_read(ls, s)["scale"] for s in (0, 1)] == [2.0 ** 10, 2.0 ** 16]      # the loss kernel only reads it


@pytest.mark.parametrize("B", [1, 2500])
@pytest.mark.parametrize("bad", ["target_2", "target_-1", "inf_logit"])
def test_loss_found_inf_out_mirrors_the_flag(nat, B, bad):
    """The bad element sits at index 1500 of B = 2500, which the block reaches only on its second trip."""
    z, y = (a.copy() for a in _loss_batch(B))
    at = B * 3 // 5
    assert at == (1500 if B == 2500 else 0)
    if bad == "inf_logit":
        z[at, 0] = np.inf
    else:
        y[at] = 2 if bad == "target_2" else -1
    found = torch.full((1,), 7.0, device=DEV)
    _, _, stats = nat.ce2_loss_fwd_bwd(torch.from_numpy(z).to(DEV), torch.from_numpy(y).to(DEV), nat.LOSS_CE, _f32(0.1),
                                       found_inf_out=found)
    st = nat.decode_stats(stats.cpu())
    assert found.item() == 1.0 and st["found_inf"] == 1.0
    assert (st["nonfinite"], st["bad_target"]) == ((1, 0) if bad == "inf_logit" else (0, 1))
    assert st["count"] == B


# --------------------------------------------------------------------------- f. ww_grad_norm_clip
CLIP_N = (1, 1024, 1025, 65536, 65537)


@functools.lru_cache(maxsize=None)
def _clip_input(n):
    g = torch.randn(n, generator=torch.Generator().manual_seed(n)) * 3.0
    g[0] = -2.5                                                              # n = 1 is over the threshold too
    return g


def _torch_clip(g, max_norm):
    q = torch.nn.Parameter(torch.zeros_like(g))
    q.grad = g.clone()
    n32 = torch.nn.utils.clip_grad_norm_([q], max_norm)
    return n32, q.grad


@pytest.mark.parametrize("max_norm", [0.0, 1e6, 1.0])
@pytest.mark.parametrize("n", CLIP_N)
def test_grad_norm_clip_matches_float64_oracle(nat, n, max_norm):
    from oracle.optim import clip_grad_norm
    g = _clip_input(n)
    ref_norm, ref_g = clip_grad_norm(g.numpy(), max_norm)
    assert ref_norm > 1.0
    n32, g32 = _torch_clip(g, max_norm) if max_norm > 0 else (g.norm(), g)
    flat, norm, stats = g.to(DEV), torch.zeros(1, device=DEV), _stats(nat)
    nat.grad_norm_clip_(flat, max_norm, norm_out=norm, stats=stats)
    where = f"n={n} max_norm={max_norm:g}"
    _close("grad norm", np.float64(norm.item()), ref_norm, abs(n32.item() - ref_norm), 1e-5 * ref_norm, where)
    st = nat.decode_stats(stats.cpu())
    assert st["grad_norm"] == norm.item() and st["found_inf"] == 0.0 and (st["loss"], st["count"]) == (0.25, 9), where
    if max_norm == 1.0:
        _close("clipped gradients", flat, ref_g, _maxabs(g32.numpy(), ref_g), 1e-6 * _top(ref_g), where)
    else:
        assert torch.equal(flat.cpu(), g), where                             # no clipping: bit-identical to the input


@pytest.mark.parametrize("bad", [float("inf"), float("nan")])
@pytest.mark.parametrize("n", CLIP_N)
def test_grad_norm_clip_nonfinite_propagates_like_torch(nat, n, bad):
    g = _clip_input(n).clone()
    g[n // 2] = bad
    n32, g32 = _torch_clip(g, 1.0)
    flat, norm, stats = g.to(DEV), torch.zeros(1, device=DEV), _stats(nat)
    nat.grad_norm_clip_(flat, 1.0, norm_out=norm, stats=stats)
    st = nat.decode_stats(stats.cpu())
    assert st["found_inf"] == 1.0
    assert np.array_equal(np.float32(norm.item()), n32.numpy(), equal_nan=True)
    assert np.array_equal(np.float32(st["grad_norm"]), n32.numpy(), equal_nan=True)
    assert np.array_equal(flat.cpu().numpy(), g32.numpy(), equal_nan=True), f"n={n} {bad}"
