"""oracle/optim.py against what it restates, on the CPU: torch.optim.Adam / AdamW / SGD(nesterov=True) and
torch.nn.utils.clip_grad_norm_ on float64 parameters, and torch.amp.GradScaler's update rule.  Both sides of the optimizer
comparison are the same float64 formulas, so only the order of operations differs: 1e-12 relative.  The scaler's scale
(powers of two) and growth tracker must agree exactly."""
import numpy as np
import pytest
import torch

from oracle import optim as OO


def _rel(got, ref):
    ref = np.asarray(ref, dtype=np.float64)
    return float(np.abs(np.asarray(got, dtype=np.float64) - ref).max() / max(np.abs(ref).max(), 1e-300))


def _torch_opt(kind, q, lr, wd, momentum):
    if kind == "adam":
        return torch.optim.Adam([q], lr=lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=wd)
    if kind == "adamw":
        return torch.optim.AdamW([q], lr=lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=wd)
    return torch.optim.SGD([q], lr=lr, momentum=momentum, weight_decay=wd, nesterov=momentum > 0)


@pytest.mark.parametrize("kind,wd,momentum", [
    ("adam", 0.0, 0.0), ("adam", 1e-2, 0.0), ("adamw", 0.0, 0.0), ("adamw", 1e-2, 0.0),
    ("sgd", 0.0, 0.0), ("sgd", 1e-2, 0.0), ("sgd", 0.0, 0.9), ("sgd", 1e-2, 0.9)])
@pytest.mark.parametrize("max_norm", [1.0, 0.0])
def test_optim_step_and_clip_match_torch_float64(kind, wd, momentum, max_norm):
    n = 257
    gen = torch.Generator().manual_seed(11)
    p0 = torch.randn(n, generator=gen, dtype=torch.float64)
    q = torch.nn.Parameter(p0.clone())
    topt = _torch_opt(kind, q, 3e-3, wd, momentum)
    p, m, v = p0.numpy().copy(), np.zeros(n), np.zeros(n)
    lr = 3e-3
    for step in range(8):
        g = torch.randn(n, generator=gen, dtype=torch.float64) * (3.0 if step % 2 else 0.01)   # both sides of the clip threshold
        g[:3] = 0.0
        if step == 4:                                                   # a scheduler changes lr mid-run
            lr = 1e-3
            for gp in topt.param_groups:
                gp["lr"] = lr
        q.grad = g.clone()
        norm, gc = OO.clip_grad_norm(g.numpy(), max_norm)
        if max_norm > 0:
            tn = torch.nn.utils.clip_grad_norm_([q], max_norm)
            assert abs(norm - tn.item()) <= 1e-12 * tn.item()
        else:
            assert abs(norm - g.norm().item()) <= 1e-12 * norm and np.array_equal(gc, g.numpy())
        assert _rel(gc, q.grad.numpy()) <= 1e-12
        topt.step()
        p, m, v = OO.optim_step(kind, p, gc, m, v, step + 1, lr, (0.9, 0.999), 1e-8, wd, momentum)
        assert _rel(p, q.detach().numpy()) <= 1e-12, step
        st = topt.state[q]
        if kind == "sgd":
            buf = st.get("momentum_buffer")
            if momentum > 0:
                assert _rel(m, buf.numpy()) <= 1e-12, step
            else:
                assert buf is None and not m.any()                       # the buffer is passed through untouched
            assert not v.any()
        else:
            assert int(st["step"]) == step + 1
            assert _rel(m, st["exp_avg"].numpy()) <= 1e-12 and _rel(v, st["exp_avg_sq"].numpy()) <= 1e-12, step


def test_optim_step_rejects_unknown_kind_and_leaves_inputs_alone():
    p, g, m, v = np.ones(4), np.full(4, 0.5), np.zeros(4), np.zeros(4)
    OO.optim_step("adam", p, g, m, v, 1, 1e-2, wd=1e-2)
    OO.optim_step("sgd", p, g, m, v, 1, 1e-2, wd=1e-2, momentum=0.9)
    assert (p == 1).all() and (g == 0.5).all() and not m.any() and not v.any()
    with pytest.raises(ValueError):
        OO.optim_step("rmsprop", p, g, m, v, 1, 1e-2)


@pytest.mark.parametrize("bad", [float("inf"), float("nan")])
def test_clip_propagates_nonfinite_norm_like_torch(bad):
    g = torch.linspace(-1.0, 1.0, 9, dtype=torch.float64)
    g[4] = bad
    q = torch.nn.Parameter(torch.zeros(9, dtype=torch.float64))
    q.grad = g.clone()
    tn = torch.nn.utils.clip_grad_norm_([q], 1.0)
    norm, gc = OO.clip_grad_norm(g.numpy(), 1.0)
    assert np.array_equal(np.float64(norm), tn.numpy(), equal_nan=True)
    assert np.array_equal(gc, q.grad.numpy(), equal_nan=True)


def test_grad_scaler_update_matches_torch_gradscaler():
    """growth at the interval, backoff with a tracker reset, and again growth counted from the reset."""
    kw = dict(init_scale=2.0 ** 10, growth_factor=2.0, backoff_factor=0.5, growth_interval=3)
    scaler = torch.amp.GradScaler("cpu", **kw)
    q = torch.nn.Parameter(torch.ones(4))
    opt = torch.optim.SGD([q], lr=0.1)
    scale, tracker = kw["init_scale"], 0
    for overflow in (0, 0, 0, 0, 1, 0, 0, 1, 1, 0, 0, 0, 0, 0, 0):
        q.grad = scaler.scale(torch.full((4,), float("inf") if overflow else 1.0))
        before = q.detach().clone()
        scaler.step(opt)
        scaler.update()
        assert torch.equal(q.detach(), before) == bool(overflow)          # GradScaler skipped exactly the overflowing steps
        new = OO.grad_scaler_update(scale, tracker, kw["growth_factor"], kw["backoff_factor"], kw["growth_interval"],
                                    grads_nonfinite=bool(overflow), skipped=bool(overflow))
        scale, tracker = new
        assert scale == scaler.get_scale() and tracker == scaler._get_growth_tracker()
    assert (scale, tracker) == (2.0 ** 10, 0)               # up once, down three times (one from tracker 2), up twice
    # a batch dropped for its loss never reaches the scaler (trainer.py:177-179): nothing changes
    assert OO.grad_scaler_update(512.0, 2, 2.0, 0.5, 3, grads_nonfinite=False, skipped=True) == (512.0, 2)
