"""GPU: the 16-bit pointwise backward kernel (k_pw_bwd_bf16) tile by tile, through _native.pwconv1x1_bwd, against a float64
torch restatement of the layer pair  y_in -> bn_in -> relu -> 1x1 conv -> bn_out -> dL/dz.

Shapes (B, H, W) -> pixels M, 64-pixel tiles:
    (1, 3, 5)    15    one partial tile                          pooled: the narrow variant (an image < one tile)
    (2, 8, 8)    128   exact tiles                               pooled: WIDE_IMG with an image of exactly one tile
    (3, 5, 19)   285   ragged last tile, an image boundary inside a tile
    (2, 20, 76)  3040  the workload's image (1520 pixels)        pooled: WIDE_IMG, image boundary inside a tile
Each runs with an incoming gradient tensor in bf16 and fp16; the three marked shapes also run as the last layer, which takes
the pooled gradient (B x 64) and the ReLU mask of its own recomputed output instead of a gradient tensor.

Inputs: unit-normal y_in plus a per-channel offset of up to 3 standard deviations (a large mean is where forming sum d*yhat
as rstd * (sum d*y - mean * sum d) would cancel; the kernel sums d*yhat value by value), about half of both ReLU masks set.  The layer's own output is restated as the device recomputes it: relu(bn(y_in)) and W rounded to
the 16-bit type, the product rounded again.

Bounds are those of tests/test_bf16_mode.py::test_conv_bwd_layers_bf16 and tests/test_fp16_mode.py::test_conv_bwd_layers_fp16
for this layer: g_in within 3 roundings of its largest entry, dW 4e-3 (bf16) / 2 x 2^-10 (fp16), d-gamma / d-beta of the input
layer 1e-4 against sums of the stored g_in.  coef = (A, Bc, Cc) of the input layer is built from those sums, c1 = sum d / M and
c2 = sum d*yhat / M, each held to 1e-4 of its largest entry: A = gamma * rstd holds no sum (2e-5, the fp32 kernels' bound),
Bc = -A rstd c2 may be off by max(A rstd) * 1e-4 max|c2|, and Cc = A (mean rstd c2 - c1) by
max(A) * 1e-4 (max|mean rstd| max|c2| + max|c1|).

The tile walk direction (WW_PW_BWD_REV, read once per process) only permutes the tiles among the workgroups: g_in is
bit-equal between the two directions.  One child interpreter runs every case in the ascending order."""
import functools
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
REPO = Path(__file__).resolve().parents[1]
DEV = "cuda:0"
DTYPES = {"bf16": (torch.bfloat16, 2.0 ** -8, 4e-3), "fp16": (torch.float16, 2.0 ** -10, 2 * 2.0 ** -10)}   # eps per rounding, dW bound
SHAPES = [(1, 3, 5), (2, 8, 8), (3, 5, 19), (2, 20, 76)]
POOLED_SHAPES = [(1, 3, 5), (2, 8, 8), (2, 20, 76)]
CASES = [(s, d, False) for s in SHAPES for d in DTYPES] + [(s, d, True) for s in POOLED_SHAPES for d in DTYPES]


def _id(case):
    (B, H, W), d, pooled = case
    return f"{B}x{H}x{W}-{d}-{'pooled' if pooled else 'tensor'}"


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def _coef_from(g, y, gamma, eps=1e-5):
    """BatchNorm-backward constants A, Bc, Cc from dL/dz (g) and the pre-BN tensor y (NCHW, float64)."""
    mean = y.mean(dim=(0, 2, 3))
    rstd = 1.0 / torch.sqrt(y.var(dim=(0, 2, 3), unbiased=False) + eps)
    yhat = (y - mean[None, :, None, None]) * rstd[None, :, None, None]
    c1, c2 = g.mean(dim=(0, 2, 3)), (g * yhat).mean(dim=(0, 2, 3))
    A = gamma * rstd
    return torch.cat([A, -A * rstd * c2, A * (mean * rstd * c2 - c1)])


@functools.lru_cache(maxsize=None)
def reference(shape, dname, pooled):
    """float64 inputs and expected outputs of one case; computed once, shared by the tests, never modified."""
    B, H, W = shape
    dt = DTYPES[dname][0]
    r16 = lambda t: t.float().to(dt).double()
    gen = torch.Generator().manual_seed(1000 * B + 10 * H + W + (500 if pooled else 0))
    offs = (torch.rand(64, generator=gen, dtype=torch.float64) * 2 - 1) * 3
    y_in = r16(torch.randn(B, 64, H, W, generator=gen, dtype=torch.float64) + offs[None, :, None, None])
    bn_in, bn_out = torch.nn.BatchNorm2d(64).double(), torch.nn.BatchNorm2d(64).double()
    with torch.no_grad():
        for bn in (bn_in, bn_out):
            bn.weight.copy_(torch.rand(64, generator=gen, dtype=torch.float64) + 0.5)
            bn.bias.copy_(torch.randn(64, generator=gen, dtype=torch.float64) * 0.3)
    w = (torch.randn(64, 64, 1, 1, generator=gen, dtype=torch.float64) * 0.25).requires_grad_(True)
    z_in = bn_in(y_in)
    z_in.retain_grad()
    a = torch.relu(z_in)
    y_raw = F.conv2d(a, w)
    y_dev = r16(F.conv2d(r16(a.detach()), r16(w.detach())))      # the stored y_out, as the kernel recomputes it
    y = y_raw + (y_dev - y_raw.detach())                          # gradient passes through the rounding
    z = bn_out(y)
    mean_out = y_dev.mean(dim=(0, 2, 3))
    rstd_out = 1.0 / torch.sqrt(y_dev.var(dim=(0, 2, 3), unbiased=False) + 1e-5)
    scale_out = bn_out.weight.detach() * rstd_out
    ss_out = torch.cat([scale_out, bn_out.bias.detach() - mean_out * scale_out])
    if pooled:
        dpool = torch.randn(B, 64, generator=gen, dtype=torch.float64).float().double()
        (torch.relu(z) * dpool[:, :, None, None]).sum().backward()
        g = dpool[:, :, None, None] * (z.detach() > 0)
    else:
        dpool = None
        g = r16(torch.randn(B, 64, H, W, generator=gen, dtype=torch.float64) * (torch.rand(B, 64, H, W, generator=gen) > 0.5))
        (z * g).sum().backward()
    mean_in = y_in.mean(dim=(0, 2, 3))
    rstd_in = 1.0 / torch.sqrt(y_in.var(dim=(0, 2, 3), unbiased=False) + 1e-5)
    scale_in = bn_in.weight.detach() * rstd_in
    return dict(dt=dt, y_in=y_in, y_out=y_dev, g=None if pooled else g, dpool=dpool, ss_out=ss_out,
                coef=_coef_from(g, y_dev, bn_out.weight.detach()), w=w.detach(), gamma_in=bn_in.weight.detach(),
                ss_in=torch.cat([scale_in, bn_in.bias.detach() - mean_in * scale_in]), mean_in=mean_in, rstd_in=rstd_in,
                ref_g_in=nhwc(z_in.grad), ref_dw=w.grad.reshape(64, 64))


def run_device(nat, c):
    f32 = lambda t: t.float().to(DEV).contiguous()
    t16 = lambda t: nhwc(t).to(c["dt"]).to(DEV).contiguous()
    pooled = c["g"] is None
    return nat.pwconv1x1_bwd(None if pooled else t16(c["g"]), f32(c["dpool"]) if pooled else None, y_out=t16(c["y_out"]),
                             ss_out=f32(c["ss_out"]) if pooled else None, coef=f32(c["coef"]), y_in=t16(c["y_in"]),
                             ss_in=f32(c["ss_in"]), mr_in=f32(torch.cat([c["mean_in"], c["rstd_in"]])),
                             gamma_in=f32(c["gamma_in"]), w=f32(c["w"]), scratch=nat.layer_scratch(DEV))


def _bits(g_in):
    return g_in.view(torch.int16).cpu().numpy()


def dump_g_in(path):
    """child process entry: g_in of every case, as stored, to one .npz"""
    from wakeword_trainer_home_amd import _native as nat
    nat.load()
    np.savez(path, **{_id(case): _bits(run_device(nat, reference(*case))[0]) for case in CASES})


@pytest.fixture(scope="module")
def nat():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from wakeword_trainer_home_amd import _native
    _native.load()
    return _native


def rel_err(got, ref):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return float(np.abs(got - ref).max() / (np.abs(ref).max() + 1e-30))


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_pw_bwd_tile_shapes(nat, case):
    shape, dname, pooled = case
    _, eps, dw_tol = DTYPES[dname]
    c = reference(*case)
    g_in, dw, coef_in, dgamma, dbeta = run_device(nat, c)
    torch.cuda.synchronize()
    assert g_in.dtype == c["dt"] and torch.isfinite(g_in.float()).all()
    gi = g_in.float().cpu().double()
    e_g = ((gi - c["ref_g_in"]).abs().max() / c["ref_g_in"].abs().max()).item()
    e_w = rel_err(dw.cpu(), c["ref_dw"])
    # the input layer's sums are taken over the ROUNDED g_in: compare with sums of the device tensor itself
    yhat_in = (nhwc(c["y_in"]) - c["mean_in"]) * c["rstd_in"]
    e_b = rel_err(dbeta.cpu(), gi.sum(dim=(0, 1, 2)))
    e_ga = rel_err(dgamma.cpu(), (gi * yhat_in).sum(dim=(0, 1, 2)))
    coef_ref = _coef_from(gi.permute(0, 3, 1, 2), c["y_in"], c["gamma_in"]).numpy()
    e_c = np.abs(coef_in.cpu().numpy().astype(np.float64) - coef_ref).reshape(3, 64).max(axis=1)
    A, mr = coef_ref[:64], (c["mean_in"] * c["rstd_in"]).abs().max().item()
    c1, c2 = gi.mean(dim=(0, 1, 2)).abs().max().item(), (gi * yhat_in).mean(dim=(0, 1, 2)).abs().max().item()
    tol_c = [2e-5 * A.max(), (A * c["rstd_in"].numpy()).max() * 1e-4 * c2, A.max() * 1e-4 * (mr * c2 + c1)]
    print(f"pw bwd {_id(case)}: g_in={e_g:.2e} dw={e_w:.2e} dbeta={e_b:.2e} dgamma={e_ga:.2e} "
          f"coef A={e_c[0]:.2e}/{tol_c[0]:.2e} Bc={e_c[1]:.2e}/{tol_c[1]:.2e} Cc={e_c[2]:.2e}/{tol_c[2]:.2e}")
    assert e_g <= 3 * eps, "dL/dz_in"
    assert e_w < dw_tol, "dW"
    assert e_b < 1e-4, "dbeta_in"
    assert e_ga < 1e-4, "dgamma_in"
    assert e_c[0] <= tol_c[0] and e_c[1] <= tol_c[1] and e_c[2] <= tol_c[2], "coef_in"


def test_pw_bwd_g_in_is_the_same_in_both_tile_orders(nat, tmp_path):
    assert os.environ.get("WW_PW_BWD_REV", "1") != "0", "this process must run the default (descending) order"
    out = tmp_path / "g_in_ascending.npz"
    code = f"import sys; sys.path.insert(0, {str(REPO)!r}); from tests.test_pw_bwd_tiles import dump_g_in; dump_g_in({str(out)!r})"
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=dict(os.environ, WW_PW_BWD_REV="0"),
                       timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    ascending = np.load(out)
    for case in CASES:
        here = _bits(run_device(nat, reference(*case))[0])
        assert np.array_equal(here, ascending[_id(case)]), _id(case)
