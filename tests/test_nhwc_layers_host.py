"""Host side of the per-launch-path tests of the channels-last layer library (tests/nhwc_cases.py, tests/test_nhwc_layers_gpu.py);
no GPU.

  * every integer-exact case meets its exactness conditions (building a case asserts them);
  * every case reaches the launch path it is listed for, by the library's host-only plan queries (ww_nhwc_plan_*,
    ww_conv1x1_row_tile), which run the dispatch code of the entry points themselves;
  * the hand-written float64 restatements equal torch (nn.functional / autograd) on random data to 1e-12, so the GPU tests'
    references are themselves pinned;
  * the header declares the plan queries."""
import math
import re
from pathlib import Path

import pytest
import torch
import torch.nn.functional as Fn

from tests import nhwc_cases as K

REPO = Path(__file__).resolve().parents[1]
ident = lambda c: "-".join(map(str, c[0]))
TORCH_ACT = {0: lambda z: z, 1: Fn.hardswish, 2: torch.relu, 3: Fn.hardsigmoid}


def rel(got, ref):
    return (got - ref).abs().max().item() / max(ref.abs().max().item(), 1e-300)


# ------------------------------------------------------------------------------------------ exactness and launch paths
@pytest.mark.parametrize("case", K.DW_CASES, ids=ident)
def test_depthwise_cases_are_exact_and_reach_their_paths(case):
    shape, want = case
    K.assert_dw_plan(shape, want)
    c = K.dw_case(*shape)
    assert c["y"].abs().max() > 0 and c["dx"].abs().max() > 0 and c["dw"].abs().max() > 0


@pytest.mark.parametrize("case", K.STEM_CASES, ids=ident)
def test_stem_cases_are_exact_and_reach_their_paths(case):
    shape, want = case
    K.assert_stem_plan(shape, want)
    c = K.stem_case(*shape)
    assert (c["dw"] != 0).double().mean() > 0.5


@pytest.mark.parametrize("case", K.BN_CASES, ids=ident)
def test_batchnorm_cases_are_exact_and_reach_their_paths(case):
    (M, C), want = case
    K.assert_bn_plan((M, C), want)
    c = K.bn_exact_case(M, C)
    K.bn_exactness(c, M)
    ref = K.bn_fwd(c["x"], c["gamma"], c["beta"], c["rm"], c["rv"], 0, eps=c["eps"])
    # what fp32 must hold exactly: integer scale, shift and y; mean = m, rstd = 1/(2a)
    assert torch.equal(ref["mr"][:C], c["m"]) and torch.equal(ref["mr"][C:], torch.full((C,), 1 / (2 * c["a"]), dtype=torch.float64))
    assert torch.equal(ref["ss"][:C], c["g"]) and torch.equal(ref["ss"][C:], c["beta"] - c["m"] * c["g"])
    assert torch.equal(ref["y"], ref["y"].round()) and torch.equal(K.f32(ref["rm"]), K.f32(ref["rm"]))
    for kind in (0, 2):
        got, _, _ = K.bn_bwd(c["x"], c["da"], ref["ss"], ref["mr"], kind)
        assert torch.equal(got["dbeta"], got["dbeta"].round()) and torch.equal(2 * got["dgamma"], (2 * got["dgamma"]).round())
        assert got["dbeta"].abs().max() < K.LIMIT


@pytest.mark.parametrize("case", K.C1_CASES, ids=ident)
def test_conv1x1_cases_are_exact_and_reach_their_paths(case):
    (M, Kd, N), want = case
    K.assert_c1_plan((M, Kd, N), want)
    K.assert_c1_plan((M, Kd, N), want, aligned=False)
    x, w = K.conv1x1_exact_case(M, Kd, N)
    y, S = K.conv1x1(x, w)
    K.exactness(dict(x=x, w=w, y=y), dict(y=S, sum_y2=(y * y).sum(0)))
    for mode in ("bf16", "fp16"):                # the operands are exact in both 16-bit types: one reference for the three modes
        assert torch.equal(K.conv1x1(x, w, mode)[0], y)
    m = y.mean(0)
    assert torch.equal(m, m.round()) and torch.equal((y - m).abs(), torch.full_like(y, 2.0))
    xr, wr = K.pattern((M, Kd), -4, 4, 1), K.pattern((N, Kd), -3, 3, 2)       # and the plain integer product
    K.exactness(dict(x=xr, w=wr), dict(y=K.conv1x1(xr, wr)[1]))


def test_elementwise_cases_reach_the_second_trip():
    from wakeword_trainer_home_amd import _native as nat
    for n, C in ((K.EW_BIG, 4), (math.prod(K.EW_SCALE), K.EW_SCALE[2])):      # ww_add_f32 and the gating kernels, one-float form
        p = nat.plan_ew(n, C)
        assert p == dict(grid=8192, V=1) and n > 8192 * 256, (n, p)
    assert nat.plan_ew(1 << 20, 64) == dict(grid=1024, V=4) and nat.plan_ew(1 << 20, 64, aligned=False)["V"] == 1


def test_se_shapes_cover_one_two_and_four_images_per_workgroup():
    plans = [K.assert_se_plan(s) for s in K.SE_SHAPES]
    assert {p["img"] for p in plans} == {1, 2, 4}


def test_plan_queries_reject_what_the_entry_points_reject():
    from wakeword_trainer_home_amd import _native as nat
    with pytest.raises((ValueError, nat.NativeError)):
        nat.plan_dw("fwd", 2, 5, 5, 16, 4, 1)                      # k = 4
    with pytest.raises((ValueError, nat.NativeError)):
        nat.plan_stem(2, 8, 8, 6)                                  # C % 4 != 0
    with pytest.raises((ValueError, nat.NativeError)):
        nat.plan_bn("fwd", 8, 2048)                                # C > 1024


# ------------------------------------------------------------------------------------------ the restatements against torch
@pytest.mark.parametrize("kind", [0, 1, 2, 3])
@pytest.mark.parametrize("training", [True, False])
def test_batchnorm_restatement_equals_torch(kind, training):
    g = torch.Generator().manual_seed(kind + 4 * training)
    M, C = 37, 6
    x = (torch.randn(M, C, generator=g, dtype=torch.float64) * 2 + 1).requires_grad_(True)
    gamma = (torch.rand(C, generator=g, dtype=torch.float64) + 0.5).requires_grad_(True)
    beta = (torch.randn(C, generator=g, dtype=torch.float64) * 0.3).requires_grad_(True)
    rm, rv = torch.randn(C, generator=g, dtype=torch.float64) * 0.1, torch.rand(C, generator=g, dtype=torch.float64) + 0.5
    da = torch.randn(M, C, generator=g, dtype=torch.float64)
    rm_t, rv_t = rm.clone(), rv.clone()
    y = TORCH_ACT[kind](Fn.batch_norm(x, rm_t, rv_t, gamma, beta, training=training, momentum=K.r32(K.MOMENTUM), eps=K.r32(K.EPS)))
    (y * da).sum().backward()
    ref = K.bn_fwd(x.detach(), gamma.detach(), beta.detach(), rm, rv, kind, training)
    assert rel(ref["y"], y.detach()) < 1e-12 and rel(ref["rm"], rm_t) < 1e-12 and rel(ref["rv"], rv_t) < 1e-12
    got, bnd, _ = K.bn_bwd(x.detach(), da, ref["ss"], ref["mr"], kind, training)       # (z32 rounds z: no kink within 1e-7 here)
    tol = 1e-12 if kind in (0, 2) else 1e-7                # torch's float64 hardswish / hardsigmoid backward carries fp32 constants
    assert rel(got["dx"], x.grad) < tol and rel(got["dgamma"], gamma.grad) < tol and rel(got["dbeta"], beta.grad) < tol
    assert all((b >= 0).all() for b in bnd.values())


@pytest.mark.parametrize("k,s", [(3, 1), (3, 2), (5, 1), (5, 2)])
def test_depthwise_restatement_equals_torch(k, s):
    g = torch.Generator().manual_seed(k + s)
    x = torch.randn(3, 6, 7, 5, generator=g, dtype=torch.float64)              # (B, H, W, C)
    w = torch.randn(5, 1, k, k, generator=g, dtype=torch.float64, requires_grad=True)
    xt = x.permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    y = Fn.conv2d(xt, w, stride=s, padding=k // 2, groups=xt.shape[1])
    dy = torch.randn(y.shape, generator=g, dtype=torch.float64)
    (y * dy).sum().backward()
    cl = lambda t: t.detach().permute(0, 2, 3, 1).contiguous()
    assert rel(K.dw_fwd(x, w.detach()[:, 0], k, s), cl(y)) < 1e-12
    dx, dw = K.dw_bwd(x, w.detach()[:, 0], cl(dy), k, s)
    assert rel(dx, cl(xt.grad)) < 1e-12 and rel(dw, w.grad[:, 0]) < 1e-12


def test_stem_and_im2col_restatements_equal_torch():
    g = torch.Generator().manual_seed(9)
    x = torch.randn(3, 1, 9, 12, generator=g, dtype=torch.float64)
    w = torch.randn(8, 1, 3, 3, generator=g, dtype=torch.float64, requires_grad=True)
    y = Fn.conv2d(x, w, stride=2, padding=1)
    dy = torch.randn(y.shape, generator=g, dtype=torch.float64)
    (y * dy).sum().backward()
    cl = lambda t: t.detach().permute(0, 2, 3, 1).contiguous()
    assert rel(K.stem_fwd(x[:, 0], w.detach()[:, 0]), cl(y)) < 1e-12
    assert rel(K.stem_dw(x[:, 0], cl(dy)), w.grad[:, 0]) < 1e-12
    assert torch.equal(K.im2col3x3s2(x[:, 0]), Fn.unfold(x, 3, padding=1, stride=2).transpose(1, 2).reshape(-1, 9))


def test_se_restatement_equals_autograd():
    g = torch.Generator().manual_seed(4)
    B, HW, C, Cs = 5, 7, 12, 4
    rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    x, w1, b1, w2, b2 = (t.requires_grad_(True) for t in (rn(B, HW, C), rn(Cs, C) * 0.3, rn(Cs) * 0.2, rn(C, Cs) * 0.5, rn(C) * 0.5))
    dy = rn(B, HW, C)
    s = x.mean(1)
    pre1 = s @ w1.t() + b1
    pre2 = torch.relu(pre1) @ w2.t() + b2
    y = x * Fn.hardsigmoid(pre2)[:, None, :]
    (y * dy).sum().backward()
    d = lambda t: t.detach()
    f = K.se_fwd(d(x), d(w1), d(b1), d(w2), d(b2))
    assert rel(f["y"], d(y)) < 1e-12 and rel(f["pre2"], d(pre2)) < 1e-12
    got, bnd = K.se_bwd(d(x), dy, f["s"], f["pre1"], f["pre2"], d(w1), d(w2))
    for name, want in (("dx", x.grad), ("dw1", w1.grad), ("db1", b1.grad), ("dw2", w2.grad), ("db2", b2.grad)):
        assert rel(got[name], want) < 1e-7, name             # (1/6 as an fp32 constant in torch's float64 hardsigmoid backward)
        assert (bnd[name] >= 0).all() and bnd[name].shape == want.shape


def test_activation_restatements():
    z = torch.linspace(-5, 5, 201, dtype=torch.float64)
    for kind in (1, 2, 3):
        assert rel(K.act(kind, z), TORCH_ACT[kind](z)) < 1e-15
        assert (K.act32(kind, z) - K.act(kind, K.f32(z))).abs().max() < 4 * K.U * 6
        zz = z.clone().requires_grad_(True)
        TORCH_ACT[kind](zz).sum().backward()
        assert rel(K.act_grad(kind, z)[0], zz.grad) < (1e-15 if kind == 2 else 1e-7)      # torch: fp32 constants in float64 kernels


def test_header_declares_the_plan_queries():
    from wakeword_trainer_home_amd import _native as nat
    header = (REPO / "include" / "wwhip.h").read_text()
    for name in ("ww_nhwc_plan_dw", "ww_nhwc_plan_bn", "ww_nhwc_plan_stem", "ww_nhwc_plan_ew", "ww_conv1x1_row_tile", "ww_se_plan"):
        assert re.search(rf"\bint {name}\(", header) and name in nat.EXPORTS
