"""Host side of the persistent-loop tests of the conv stack (tests/conv_trip_cases.py, tests/test_conv_trips_gpu.py); no GPU.

  * every integer-exact case meets its two exactness conditions (the builders assert them; building a case is the test), the
    full-slab shapes included;
  * the hand-written backward restatement equals torch autograd through  bn -> relu -> conv -> bn  on a consistent random case to
    1e-12, with ``coef`` taken from tests/test_hip_kernels.py:_coef_from -- the GPU tests' reference is itself pinned;
  * the forward restatement equals nn.BatchNorm2d's training forward (scale/shift, running statistics);
  * the header declares the entry points these tests drive, under ABI version 16."""
import re
from pathlib import Path

import pytest
import torch
import torch.nn.functional as F

from tests import conv_trip_cases as K

REPO = Path(__file__).resolve().parents[1]
C = K.C


def rel(got, ref):
    return (got - ref).abs().max().item() / max(ref.abs().max().item(), 1e-300)


@pytest.mark.parametrize("case", K.FWD_CASES, ids=K.case_id)
def test_forward_cases_are_integer_exact(case):
    c, ref = K.fwd_case(*case)
    assert ref["y"].abs().max() > 0 and ref["mr"][C:].isfinite().all()
    # the three storage types share one reference: the restatement with the roundings in place returns the same values
    for t in K.T16:
        assert torch.equal(K.layer_fwd(case[0], c, t)["y"], ref["y"])


@pytest.mark.parametrize("case", K.BWD_CASES, ids=K.case_id)
def test_backward_cases_are_integer_exact(case):
    kind, shape, pooled = case
    c, ref = K.bwd_case(kind, shape, pooled)
    assert ref["dw"].abs().max() > 0
    for t in K.T16:
        r16 = K.layer_bwd(kind, c, t)
        assert torch.equal(r16["dw"], ref["dw"])
        if kind != "stem":
            assert torch.equal(r16["g_in"], ref["g_in"]) and torch.equal(r16["dgamma"], ref["dgamma"])
    if kind != "stem":
        # about half of the input ReLU mask set, and a gradient that reaches most channels
        frac = (K.act_in(c["y_in"], c["ss_in"])[0] > 0).double().mean().item()
        assert 0.2 < frac < 0.8, frac
        assert (ref["g_in"].reshape(-1, C).abs().sum(0) > 0).sum() >= C // 2


@pytest.mark.parametrize("kind", ["dw", "pw", "stem"])
def test_full_slab_cases_are_integer_exact(kind):
    """the shapes that fill the partial slabs: the 2^24 condition must still hold at their pixel counts"""
    shape = K.FULL_SHAPES[kind]
    K.build_fwd(kind, shape, small=True)
    K.build_bwd(kind, shape, small=True)
    if kind == "pw":
        K.build_bwd(kind, shape, pooled=True, small=True)


def _consistent(kind, pooled, seed):
    """a random layer pair through autograd, nn.BatchNorm2d in training mode on both sides of the convolution"""
    from tests.test_hip_kernels import _coef_from
    gen = torch.Generator().manual_seed(seed)
    B, H, W = (3, 9, 11) if kind == "stem" else (3, 5, 7)
    rn = lambda *s: torch.randn(*s, generator=gen, dtype=torch.float64)
    bn_in, bn_out = torch.nn.BatchNorm2d(C).double(), torch.nn.BatchNorm2d(C).double()
    with torch.no_grad():
        for bn in (bn_in, bn_out):
            bn.weight.copy_(torch.rand(C, generator=gen, dtype=torch.float64) + 0.5)
            bn.bias.copy_(rn(C) * 0.3)
    cl = lambda t: t.detach().permute(0, 2, 3, 1).contiguous()
    if kind == "stem":
        x = rn(B, 1, H, W)
        w = (rn(C, 1, 3, 3) * 0.3).requires_grad_(True)
        y = F.conv2d(x, w, stride=2, padding=1)
        c = dict(x=x[:, 0].contiguous())
        y_in = z_in = None
    else:
        y_in = rn(B, C, H, W) + rn(C)[None, :, None, None]
        z_in = bn_in(y_in)
        z_in.retain_grad()
        a = torch.relu(z_in)
        w = (rn(C, 1, 3, 3) * 0.3 if kind == "dw" else rn(C, C, 1, 1) * 0.2).requires_grad_(True)
        y = F.conv2d(a, w, padding=1, groups=C) if kind == "dw" else F.conv2d(a, w)
        mean_in = y_in.mean(dim=(0, 2, 3))
        rstd_in = 1.0 / torch.sqrt(y_in.var(dim=(0, 2, 3), unbiased=False) + 1e-5)
        scale_in = bn_in.weight.detach() * rstd_in
        c = dict(y_in=cl(y_in), ss_in=torch.cat([scale_in, bn_in.bias.detach() - mean_in * scale_in]),
                 mr_in=torch.cat([mean_in, rstd_in]), gamma_in=bn_in.weight.detach())
    z = bn_out(y)
    yd = y.detach()
    if pooled:
        dpool = rn(B, C)
        (torch.relu(z) * dpool[:, :, None, None]).sum().backward()
        g = dpool[:, :, None, None] * (z.detach() > 0)
        mean_out = yd.mean(dim=(0, 2, 3))
        scale_out = bn_out.weight.detach() / torch.sqrt(yd.var(dim=(0, 2, 3), unbiased=False) + 1e-5)
        c.update(g=None, dpool=dpool, ss_out=torch.cat([scale_out, bn_out.bias.detach() - mean_out * scale_out]))
    else:
        g = rn(*yd.shape) * (torch.rand(*yd.shape, generator=gen) > 0.4)
        (z * g).sum().backward()
        c["g"] = cl(g)
    c.update(y_out=cl(yd), w=w.detach(), coef=_coef_from(g, yd, bn_out.weight.detach())[0])
    want = dict(dw=w.grad)
    if kind != "stem":
        want.update(g_in=cl(z_in.grad), dgamma=bn_in.weight.grad, dbeta=bn_in.bias.grad,
                    coef_in=_coef_from(z_in.grad, y_in, bn_in.weight.detach())[0])
    return c, want


@pytest.mark.parametrize("kind,pooled", [("dw", False), ("pw", False), ("pw", True), ("stem", False)])
def test_backward_restatement_equals_autograd(kind, pooled):
    c, want = _consistent(kind, pooled, seed=17)
    got = K.layer_bwd(kind, c)
    for name, ref in want.items():
        assert rel(got[name], ref) < 1e-12, (name, rel(got[name], ref))
    # and the forward: the layer's output and nn.BatchNorm2d's training statistics of it
    if kind != "stem":
        assert rel(K.conv_fwd(kind, K.act_in(c["y_in"], c["ss_in"])[1], c["w"]), c["y_out"]) < 1e-12
    else:
        assert rel(K.conv_fwd(kind, c["x"], c["w"]), c["y_out"]) < 1e-12


def test_forward_restatement_equals_batchnorm():
    gen = torch.Generator().manual_seed(3)
    y = torch.randn(4, 6, 5, C, generator=gen, dtype=torch.float64) * 2 + 1
    bn = torch.nn.BatchNorm2d(C, momentum=K.MOMENTUM, eps=K.EPS).double()
    with torch.no_grad():
        bn.weight.uniform_(0.5, 1.5)
        bn.bias.normal_(0, 0.3)
        bn.running_mean.normal_(0, 0.2)
        bn.running_var.uniform_(0.5, 1.5)
    rm, rv = bn.running_mean.clone(), bn.running_var.clone()
    z = bn(y.permute(0, 3, 1, 2)).permute(0, 2, 3, 1)
    f = K.bn_finalize(y, bn.weight.detach(), bn.bias.detach(), rm, rv)
    assert rel(y * f["ss"][:C] + f["ss"][C:], z.detach()) < 1e-12
    assert rel(f["running_mean"], bn.running_mean) < 1e-12 and rel(f["running_var"], bn.running_var) < 1e-12
    assert rel(f["mr"][:C], y.reshape(-1, C).mean(0)) < 1e-12


def test_values_per_thread_follow_the_kernel_geometry():
    assert K.dw_geometry(20, 76) == (19, 1, 20) and K.dw_geometry(41, 10) == (3, 3, 14) and K.dw_geometry(21, 3) == (1, 2, 11)
    assert K.values_per_thread("dw", (3, 20, 76), 0) == 80 + 10          # 57 items in 8 workgroups: one item per slot
    assert K.values_per_thread("dw", (3, 20, 76), 1) == 8 * 80 + 10      # one workgroup: 57 items in 8 slots
    assert K.values_per_thread("pw", (2, 20, 76), 1) == 48 * 16 + 2 and K.values_per_thread("pw", (2, 20, 76), 0) == 18


def test_header_declares_the_grid_cap_and_the_abi_version():
    from wakeword_trainer_home_amd import _native as nat
    header = (REPO / "include" / "wwhip.h").read_text()
    assert nat.ABI_VERSION == 17 and re.search(r"#define WW_ABI_VERSION 17\b", header)
    assert re.search(r"\bint ww_ctx_set_grid_cap\(ww_ctx \*ctx, int n\);", header)
    assert re.search(r"\bint ww_conv_stem_bwd_recompute\(", header)
    for name in ("ww_ctx_set_grid_cap", "ww_conv_stem_bwd_recompute"):
        assert name in nat.EXPORTS
    assert callable(nat.set_grid_cap)
