"""16-bit activation storage of the native Conv2d path and ResNet18Wakeword (the ``*_st_*`` kernels, ``storage="bf16" | "fp16"``) on
the MI355X.

References: float64 (tests/resnet_cases.py, tests/resnet_storage_cases.py) applied to the tensors the device itself read, so every
stored tensor is held to the bound of the ONE op that made it: the fp32 round-off of that op's few operations plus half a unit in the
last place of the storage type S (the one rounding).  No bound comes from what the device gave.  Written out per op:
  conv y / dx     R sum|a b| + ulp_S/2        R = 5e-7, test_resnet_gpu.py's bound of the fp32 accumulation (blocked sums, K <= 4608)
  conv dw (fp32)  R sum|a b|
  BatchNorm y     k eps sum|terms| + ulp_S/2  k fp32 roundings: fma (1); + residual add (2); + the residual's own fma (3)
  BatchNorm dx    12 eps sum|terms| + ulp_S/2 (x - mean) rstd: 2, dz - s1/M - xhat s2/M: 7, times scale: 1, the two sums: 2 (the same
                  for the pass that finishes the sums itself, which layers of <= 4 Mi elements take)
  dgamma / dbeta  4 eps sum|dz xhat| / 2 eps sum|dz|   fp32 partial + fp32 result, and xhat's two roundings
  epilogue statistics: a tile's fp32 partial holds n = 64 terms (16 registers, 2 lane halves, 2 row wavefronts: 18 fp32 additions):
                  |S - sum y| <= 64 eps sum|y| over the tile, likewise for sum y^2 (fma: the square is not rounded on its own)
  ss / mr / running statistics: intervals from |d sum x| <= k eps sum|x|, |d sum x^2| <= k eps sum x^2, plus the fp32 rounding of the
                  result; k = 2 for the pass of its own (an fp32 partial per chunk of fp64 sums, finished in fp64), k = 64 + 1 for
                  the epilogue's partials (the tile's 64 terms, and the fold's one rounding where there are more than 1024 tiles)
  stem y          k k eps sum|a b| + ulp_S/2  an fp32 fma chain of k k terms;  stem dw: P eps sum|a b| (P pixels, fp32 sums)
  pool            exact;  its gradient: 3 eps sum|g| + ulp_S/2 (at most four window gradients)
  mean            eps |mean| (fp64 sum, one fp32 rounding);  its gradient: eps |g| + ulp_S/2;  ReLU mask: exact
eps = 2^-24."""
import copy
import ctypes as C

import numpy as np
import pytest
import torch

from tests.resnet_cases import (BN_EPS, BN_MOMENTUM, ResNetRestated, conv2d_bwd, conv2d_fwd, golden_case, layer_case, layer_inputs,
                                maxpool_bwd, maxpool_fwd)
from tests.resnet_storage_cases import EPS32, MANT, MIN_EXP, ST_SHAPES, ResNetStorageRestated, bn_apply, bn_bwd, bn_vectors, col_sums, half_ulp

gpu = pytest.mark.gpu
DEV = "cuda:0"
_ST = {"bf16": torch.bfloat16, "fp16": torch.float16}
_IDS = ["-".join(map(str, s)) for s in ST_SHAPES]
# fp16 gradients travel times the loss scale (GradScaler's initial 65536, what the Trainer's DeviceGradScaler starts from), as they do
# in training: without it the model's activation gradients reach fp16's subnormal range
_SCALE = {"bf16": 1.0, "fp16": 65536.0}
_ROUNDOFF = 5e-7          # test_resnet_gpu.py's per-element bound of the fp32 accumulation, x sum|a b|
_REF = {}


def _d(t):
    return t.detach().cpu().double()


def _nat():
    from wakeword_trainer_home_amd import _native as nat
    return nat


def _hold(what, got, ref, bound, worst=None):
    """|got - ref| <= bound everywhere; non-finite values must agree exactly.  Records the largest error / bound."""
    got, ref = _d(got), ref.double()
    assert tuple(got.shape) == tuple(ref.shape), (what, tuple(got.shape), tuple(ref.shape))
    fin = torch.isfinite(ref)
    assert torch.equal(torch.isfinite(got), fin), what
    err = (got - ref).abs()[fin]
    b = bound.expand_as(ref)[fin] if torch.is_tensor(bound) else torch.full_like(err, bound)
    ratio = (err / b.clamp_min(1e-300)).max().item() if err.numel() else 0.0
    if worst is not None:
        worst[what] = max(worst.get(what, 0.0), ratio)
    assert not (err > b).any(), (what, ratio, err.max().item())
    return ratio


def _rounded(err_scale, ref, st):
    """fp32 round-off `err_scale` followed by ONE rounding to st."""
    return err_scale + half_ulp(ref.abs() + err_scale, st)


# ------------------------------------------------------------------------------------------ per-op checks (float64 on the device's inputs)
def _check_conv_fwd(x, w, stride, y, st, worst):
    ref, mag = conv2d_fwd(_d(x), _d(w), stride, st), conv2d_fwd(_d(x).abs(), _d(w).abs(), stride, st)
    _hold("conv.y", y, ref, _rounded(_ROUNDOFF * mag, ref, st), worst)


def _subnormal(t, st):
    """Half the spacing of st's subnormals where t holds one, else 0: what RNE itself leaves uncertain in such a value."""
    lim = 2.0 ** MIN_EXP[st]
    return ((t != 0) & (t.abs() < lim)).double() * (0.5 * lim * 2.0 ** -(MANT[st] - 1))


def _check_partials(y, part, worst):
    """The epilogue's tile partials against float64 sums of the device's OWN stored output: n = 64 terms per fp32 partial."""
    y64 = _d(y).reshape(-1, y.shape[-1])
    M, Cn = y64.shape
    tiles = (M + 63) // 64
    assert tuple(part.shape) == (tiles, 2 * Cn)
    pad = torch.zeros(tiles * 64 - M, Cn, dtype=torch.float64)
    t = torch.cat([y64, pad]).reshape(tiles, 64, Cn)
    _hold("epilogue.sum", part[:, :Cn], t.sum(1), 64 * EPS32 * t.abs().sum(1), worst)
    _hold("epilogue.sumsq", part[:, Cn:], (t * t).sum(1), 64 * EPS32 * (t * t).sum(1), worst)


def _check_conv_bwd(x, w, dy, stride, dx, dw, st, worst, dx_prev=None, subnormal=False):
    rdx, rdw = conv2d_bwd(_d(x), _d(w), _d(dy), stride, st)
    mdx, mdw = conv2d_bwd(_d(x).abs(), _d(w).abs(), _d(dy).abs(), stride, st)
    if subnormal:       # an operand in the subnormal range is taken to within half its spacing, the accuracy its own rounding has
        mdw = mdw + (conv2d_bwd(_d(x).abs(), _d(w), _subnormal(_d(dy), st), stride)[1] +
                     conv2d_bwd(_subnormal(_d(x), st), _d(w), _d(dy).abs(), stride)[1]) / _ROUNDOFF
    if dx is not None:
        if dx_prev is not None:          # dx = S(acc + float(dx_prev)): one more fp32 addition
            rdx, mdx = rdx + _d(dx_prev), mdx + _d(dx_prev).abs()
            mdx = mdx * (1 + EPS32 / _ROUNDOFF)
        _hold("conv.dx", dx, rdx, _rounded(_ROUNDOFF * mdx, rdx, st), worst)
    _hold("conv.dw", dw, rdw, _ROUNDOFF * mdw, worst)


def _check_bn_stats(x, gamma, beta, rm0, rv0, training, ss, mr, rm1, rv1, worst, k=2):
    """ss, mr and the running statistics against float64 from the column sums of the device's own x; k: the fp32 roundings a column
    sum has seen (2: the pass of its own, 65: the conv epilogue's partials)."""
    x64, g, b = _d(x), _d(gamma), _d(beta)
    Cn = x64.shape[-1]
    M = x64.numel() // Cn
    if not training:
        mean, var = _d(rm0), _d(rv0)
        rstd = 1.0 / torch.sqrt(var + BN_EPS)
        ref_ss, ref_mr = torch.cat([g * rstd, b - mean * g * rstd]), torch.cat([mean, rstd])
        _hold("bn.ss", ss, ref_ss, 2 * EPS32 * (ref_ss.abs() + torch.cat([ref_ss[:Cn].abs(), (mean * g * rstd).abs()])), worst)
        _hold("bn.mr", mr, ref_mr, EPS32 * ref_mr.abs(), worst)
        assert torch.equal(rm1, rm0) and torch.equal(rv1, rv0)
        return
    s, q, sa = col_sums(x64)
    ref_ss, ref_mr, var = bn_vectors(s, q, M, g, b)
    mean, rstd, scale = ref_mr[:Cn], ref_mr[Cn:], ref_ss[:Cn]
    d_mean = k * EPS32 * sa / M
    d_var = k * EPS32 * q / M + 2 * mean.abs() * d_mean + d_mean ** 2
    d_rstd = torch.maximum(1.0 / torch.sqrt((var - d_var).clamp_min(0.0) + BN_EPS) - rstd, rstd - 1.0 / torch.sqrt(var + d_var + BN_EPS))
    d_scale = g.abs() * d_rstd
    d_shift = mean.abs() * d_scale + scale.abs() * d_mean + d_mean * d_scale
    _hold("bn.mr", mr, ref_mr, torch.cat([d_mean, d_rstd]) + EPS32 * ref_mr.abs(), worst)
    _hold("bn.ss", ss, ref_ss, torch.cat([d_scale, d_shift + EPS32 * (b.abs() + (mean * scale).abs())]) + EPS32 * ref_ss.abs(), worst)
    m = BN_MOMENTUM
    unb = var * M / (M - 1) if M > 1 else var
    ref_rm, ref_rv = (1 - m) * _d(rm0) + m * mean, (1 - m) * _d(rv0) + m * unb
    _hold("bn.running_mean", rm1, ref_rm, m * d_mean + EPS32 * ref_rm.abs(), worst)
    _hold("bn.running_var", rv1, ref_rv, m * d_var * (M / max(M - 1, 1)) + EPS32 * ref_rv.abs(), worst)


def _check_bn_apply(x, ss, relu, res, res_ss, y, st, worst):
    ref, mag, _ = bn_apply(_d(x), _d(ss), relu, None if res is None else _d(res), None if res_ss is None else _d(res_ss))
    k = 1 if res is None else (2 if res_ss is None else 3)
    _hold("bn.y" if res is None else "bn.tail", y, ref, _rounded(k * EPS32 * mag, ref, st), worst)


def _check_bn_bwd(x, da, ss, mr, relu, training, dx, dgamma, dbeta, st, worst):
    ref, rg, rb, mag, _, (a1, a2) = bn_bwd(_d(x), _d(da), _d(ss), _d(mr), relu, training)
    _hold("bn.dx", dx, ref, _rounded(12 * EPS32 * mag, ref, st), worst)
    _hold("bn.dgamma", dgamma, rg, 4 * EPS32 * a2, worst)
    _hold("bn.dbeta", dbeta, rb, 2 * EPS32 * a1, worst)


def _check_stem_fwd(x, w, stride, y, st, worst):
    k = w.shape[2]
    ref, mag = conv2d_fwd(_d(x)[..., None], _d(w), stride), conv2d_fwd(_d(x).abs()[..., None], _d(w).abs(), stride)
    _hold("stem.y", y, ref, _rounded(k * k * EPS32 * mag, ref, st), worst)


def _check_stem_dw(x, dy, w_shape, stride, dw, worst):
    w0 = torch.zeros(w_shape, dtype=torch.float64)
    _, ref = conv2d_bwd(_d(x)[..., None], w0, _d(dy), stride)
    _, mag = conv2d_bwd(_d(x).abs()[..., None], w0, _d(dy).abs(), stride)
    _hold("stem.dw", dw, ref, dy.numel() // dy.shape[-1] * EPS32 * mag, worst)


def _check_pool(x, y, dy, dx, st, worst):
    ry, idx = maxpool_fwd(x.detach().cpu().float())
    assert torch.equal(y.cpu().float(), ry), "pool.y"
    if dy is not None:
        H, W = x.shape[1], x.shape[2]
        ref, mag = maxpool_bwd(idx, _d(dy), H, W), maxpool_bwd(idx, _d(dy).abs(), H, W)
        _hold("pool.dx", dx, ref, _rounded(3 * EPS32 * mag, ref, st), worst)


def _check_mean(x, mean, worst):
    ref = _d(x).mean(1)
    _hold("mean", mean, ref, EPS32 * ref.abs() + 1e-15 * _d(x).abs().mean(1), worst)


def _check_mean_bwd(dmean, HW, dx, st, worst):
    ref = (_d(dmean) / HW)[:, None, :].expand(-1, HW, -1)
    _hold("mean.dx", dx, ref, _rounded(EPS32 * ref.abs(), ref, st), worst)


def _check_mask(dy, y, dx):
    assert torch.equal(dx, torch.where(y != 0, dy, torch.zeros_like(dy))), "relu mask"


# ------------------------------------------------------------------------------------------ 1. the layer on integer data
def _int_case(shape):
    if shape not in _REF:
        d_in = layer_inputs(*shape, seed=sum(shape) + 17, integer=True)
        _REF[shape] = (d_in, layer_case(d_in["x"], d_in["w"], d_in["dy"], shape[6]))
    return _REF[shape]


@gpu
@pytest.mark.parametrize("mode", list(_ST))
@pytest.mark.parametrize("shape", ST_SHAPES, ids=_IDS)
def test_conv2d_st_is_the_rounded_exact_result_on_integer_data(shape, mode):
    """Integer x, dy in [-4, 4], W in [-2, 2]: every fp32 sum is exact (test_resnet_storage_host.py asserts the conditions), so y and
    dx are S(exact) BIT FOR BIT, ties to even included, and dw is the exact integers.  Also dx accumulated onto a tensor of 3s
    (S(exact + 3)), no dx at all, and a dx buffer full of NaN that comes back fully written."""
    nat, st, stride = _nat(), _ST[mode], shape[6]
    d_in, ref = _int_case(shape)
    s_ = lambda t: t.float().to(st)
    x, dy, w = s_(d_in["x"]).to(DEV), s_(d_in["dy"]).to(DEV), d_in["w"].float().to(DEV)
    y = nat.conv2d_st_fwd(x, w, stride)
    dx, dw = nat.conv2d_st_bwd(x, w, dy, stride)
    assert y.dtype is st and dx.dtype is st and dw.dtype is torch.float32
    assert torch.equal(y.cpu(), s_(ref["y"])), (ref["y"] - _d(y)).abs().max().item()
    assert torch.equal(dx.cpu(), s_(ref["dx"])), (ref["dx"] - _d(dx)).abs().max().item()
    assert torch.equal(_d(dw), ref["dw"])
    base = torch.full_like(x, 3.0)
    dx2, dw2 = nat.conv2d_st_bwd(x, w, dy, stride, dx=base)
    assert dx2 is base and torch.equal(base.cpu(), s_(ref["dx"] + 3.0)) and torch.equal(dw2, dw)
    dx3, dw3 = nat.conv2d_st_bwd(x, w, dy, stride, need_dx=False)
    assert dx3 is None and torch.equal(dw3, dw)
    nan = torch.full_like(x, float("nan"))
    dx4, _ = nat.conv2d_st_bwd(x, w, dy, stride, dx=nan, accumulate=False)
    assert dx4 is nan and torch.equal(nan.cpu(), s_(ref["dx"]))


@gpu
@pytest.mark.parametrize("mode", list(_ST))
def test_deferred_weight_gradient_equals_immediate(mode):
    """M = 1360: ten row ranges whose sum is queued under ww_ctx_set_deferred_reduce and run by the flush."""
    nat, st, shape = _nat(), _ST[mode], ST_SHAPES[-1]
    d_in, ref = _int_case(shape)
    lib, cx = nat.load(), nat.ctx(DEV)
    assert lib.ww_deferred_reduce_pending(cx) == 0
    slot = torch.full(tuple(d_in["w"].shape), float("nan"), device=DEV)
    x, dy = d_in["x"].float().to(st).to(DEV), d_in["dy"].float().to(st).to(DEV)
    _, dw = nat.conv2d_st_bwd(x, d_in["w"].float().to(DEV), dy, shape[6], dw_out=slot, defer=True)
    assert lib.ww_deferred_reduce_pending(cx) == 1
    nat.deferred_flush(DEV)
    torch.cuda.synchronize()
    assert lib.ww_deferred_reduce_pending(cx) == 0 and dw is slot and torch.equal(_d(slot), ref["dw"])


# ------------------------------------------------------------------------------------------ 2. the layer on N(0,1) data
@gpu
@pytest.mark.parametrize("mode", list(_ST))
@pytest.mark.parametrize("shape", ST_SHAPES[-3:], ids=_IDS[-3:])
def test_conv2d_st_roundoff_against_restatement(shape, mode):
    """The reference rounds the operands to S and nothing else; the device adds fp32 accumulation and one RNE:
    |got - ref| <= R sum|a b| + ulp_S(|ref| + R sum|a b|) / 2; dw, an fp32 result, keeps the existing bound."""
    nat, st = _nat(), _ST[mode]
    d_in = layer_inputs(*shape, seed=sum(shape), integer=False)
    x, dy, w = d_in["x"].float().to(st).to(DEV), d_in["dy"].float().to(st).to(DEV), d_in["w"].float().to(DEV)
    worst = {}
    y = nat.conv2d_st_fwd(x, w, shape[6])
    dx, dw = nat.conv2d_st_bwd(x, w, dy, shape[6])
    _check_conv_fwd(x, w, shape[6], y, st, worst)
    _check_conv_bwd(x, w, dy, shape[6], dx, dw, st, worst)
    prev = torch.randn(x.shape, device=DEV).to(st)
    acc = prev.clone()
    nat.conv2d_st_bwd(x, w, dy, shape[6], dx=acc)
    _check_conv_bwd(x, w, dy, shape[6], acc, dw, st, worst, dx_prev=prev)
    print(f"resnet-storage layer {'-'.join(map(str, shape))} {mode}: error / bound " + " ".join(f"{k}={v:.2f}" for k, v in worst.items()))


# ------------------------------------------------------------------------------------------ 3. statistics from the conv epilogue
# (B, H, W, Cin, Cout, k, stride): M = 70 (one full tile and 6 rows), 16 columns of a 64-wide tile; M = 1360 over 64 columns;
# two column tiles, stride 2; M = 2 x 182 x 182 = 66 248 -> 1036 tiles, no multiple of 64 and more than the 1024 rows one finish
# launch takes (folded to 256 first)
_EPI = [(2, 5, 7, 8, 16, 3, 1), (4, 20, 17, 64, 64, 3, 1), (3, 6, 4, 64, 128, 3, 2), (2, 182, 182, 8, 8, 1, 1)]


@gpu
@pytest.mark.parametrize("mode", list(_ST))
@pytest.mark.parametrize("shape", _EPI, ids=lambda s: "-".join(map(str, s)))
def test_conv_epilogue_statistics(shape, mode):
    """The rows kernel's per-tile partials against float64 sums of the device's OWN stored output (n = 64 terms per fp32 partial),
    the output itself unchanged by asking for them, and ss / mr / running statistics finished from them against float64 from
    those sums; two runs give the same bits (no atomics)."""
    nat, st = _nat(), _ST[mode]
    B, H, W, Cin, Cout, k, stride = shape
    g = torch.Generator().manual_seed(sum(shape))
    x = torch.randn(B, H, W, Cin, generator=g).to(st).to(DEV)
    w = (torch.randn(Cout, Cin, k, k, generator=g) * (Cin * k * k) ** -0.5 + 0.05).to(DEV)
    y, part = nat.conv2d_st_fwd(x, w, stride, stats=True)
    y2, part2 = nat.conv2d_st_fwd(x, w, stride, stats=True)
    assert torch.equal(y, nat.conv2d_st_fwd(x, w, stride)) and torch.equal(y, y2) and torch.equal(part, part2)
    worst = {}
    _check_partials(y, part, worst)
    M = y.numel() // Cout
    assert part.shape[0] == (M + 63) // 64
    p = dict(gamma=(torch.rand(Cout, generator=g) + 0.5).to(DEV), beta=(torch.randn(Cout, generator=g) * 0.3).to(DEV),
             rm=torch.zeros(Cout, device=DEV), rv=torch.ones(Cout, device=DEV))
    bn = nat.make_bn(p["gamma"], p["beta"], p["rm"], p["rv"], momentum=BN_MOMENTUM, eps=BN_EPS, training=True)
    rm0, rv0 = p["rm"].clone(), p["rv"].clone()
    a, ss, mr = nat.bn_act_st_fwd(y, bn, nat.LIN_RELU, Cout, part=part)
    _check_bn_stats(y, p["gamma"], p["beta"], rm0, rv0, True, ss, mr, p["rm"], p["rv"], worst, k=65)
    _check_bn_apply(y, ss, True, None, None, a, st, worst)
    print(f"resnet-storage epilogue {'-'.join(map(str, shape))} {mode} ({part.shape[0]} tiles): error / bound " + " ".join(f"{k_}={v:.2f}" for k_, v in worst.items()))


# ------------------------------------------------------------------------------------------ 4. BatchNorm, tail, stem, pool, mean, mask
def _bn_case(nat, M, Cn, st, seed, training=True):
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g)
    x = (rn(M, Cn) * (1 + rn(Cn).abs()) + rn(Cn)).to(st).to(DEV)
    p = dict(gamma=(rn(Cn).abs() + 0.5).to(DEV), beta=(rn(Cn) * 0.3).to(DEV), rm=(rn(Cn) * 0.1).to(DEV), rv=(rn(Cn).abs() + 0.5).to(DEV))
    bn = nat.make_bn(p["gamma"], p["beta"], p["rm"], p["rv"], momentum=BN_MOMENTUM, eps=BN_EPS, training=training)
    return x, p, bn, g


# (M, C): C = 8 (one column octet, 256 row lanes) and a single row; an odd M below one chunk with C = 24 (85 row lanes, idle
# threads); the widest layer; M = 16448 x 512: 1 052 672 vectors of 8, more than the 4096 x 256 threads of one grid pass, 1024 chunks
_BN_SHAPES = [(1, 8), (37, 8), (301, 24), (1360, 64), (45, 512), (16448, 512)]


@gpu
@pytest.mark.parametrize("mode", list(_ST))
@pytest.mark.parametrize("shape", _BN_SHAPES, ids=[f"{m}x{c}" for m, c in _BN_SHAPES])
def test_bn_act_st_forward_and_backward(shape, mode):
    """Training statistics of the STORED tensor, ss / mr / running statistics, y = S(relu(bn(x))), the fused tail with a plain
    residual and with a residual that has a scale|shift of its own, the statistics-only call, and the backward (with and without
    ReLU) -- each against float64 on the device's own inputs."""
    nat, st = _nat(), _ST[mode]
    M, Cn = shape
    worst = {}
    x, p, bn, g = _bn_case(nat, M, Cn, st, seed=M + Cn)
    rm0, rv0 = p["rm"].clone(), p["rv"].clone()
    y, ss, mr = nat.bn_act_st_fwd(x, bn, nat.LIN_RELU, Cn)
    assert y.dtype is st and ss.dtype is torch.float32
    _check_bn_stats(x, p["gamma"], p["beta"], rm0, rv0, True, ss, mr, p["rm"], p["rv"], worst)
    _check_bn_apply(x, ss, True, None, None, y, st, worst)
    res = torch.randn(M, Cn, generator=g).to(st).to(DEV)
    res_ss = torch.cat([torch.randn(Cn, generator=g).abs() + 0.5, torch.randn(Cn, generator=g)]).to(DEV)
    for rs in (None, res_ss):
        t, ss2, _ = nat.bn_act_st_fwd(x, bn, nat.LIN_RELU, Cn, res=res, res_ss=rs)
        _check_bn_apply(x, ss2, True, res, rs, t, st, worst)
    none, ss3, mr3 = nat.bn_act_st_fwd(x, bn, nat.LIN_NONE, Cn, want_y=False)
    assert none is None and torch.equal(ss3, ss2) and torch.isfinite(mr3).all()
    da = torch.randn(M, Cn, generator=g).to(st).to(DEV)
    for relu in (True, False):
        dx, dg, db = nat.bn_act_st_bwd(x, da, ss, mr, nat.LIN_RELU if relu else nat.LIN_NONE, True, Cn)
        assert dx.dtype is st and dg.dtype is torch.float32
        _check_bn_bwd(x, da, ss, mr, relu, True, dx, dg, db, st, worst)
    print(f"resnet-storage bn {M}x{Cn} {mode}: error / bound " + " ".join(f"{k}={v:.2f}" for k, v in worst.items()))


@gpu
@pytest.mark.parametrize("mode", list(_ST))
def test_bn_act_st_eval_mode_uses_the_running_statistics(mode):
    nat, st = _nat(), _ST[mode]
    worst = {}
    x, p, bn, g = _bn_case(nat, 301, 24, st, seed=5, training=False)
    rm0, rv0 = p["rm"].clone(), p["rv"].clone()
    y, ss, mr = nat.bn_act_st_fwd(x, bn, nat.LIN_RELU, 24)
    _check_bn_stats(x, p["gamma"], p["beta"], rm0, rv0, False, ss, mr, p["rm"], p["rv"], worst)
    _check_bn_apply(x, ss, True, None, None, y, st, worst)
    da = torch.randn(301, 24, generator=g).to(st).to(DEV)
    dx, dg, db = nat.bn_act_st_bwd(x, da, ss, mr, nat.LIN_RELU, False, 24)
    _check_bn_bwd(x, da, ss, mr, True, False, dx, dg, db, st, worst)


@gpu
@pytest.mark.parametrize("mode", list(_ST))
@pytest.mark.parametrize("shape", [(1, 5, 3, 64, 7, 2), (3, 13, 8, 8, 3, 1), (2, 40, 33, 64, 7, 2), (2, 260, 259, 64, 3, 2)],
                         ids=lambda s: "-".join(map(str, s)))
def test_stem_st(shape, mode):
    """(B, H, W, C, k, stride): an image smaller than the kernel; C = 8, stride 1; the fixture's stem; P = 2 x 130 x 130 = 33 800
    pixels at C = 64 (16 pixel lanes per workgroup): more than the 2048 x 16 of one pass of the forward's persistent loop and than
    the 256 x 16 of the weight gradient's, so a workgroup makes a second trip in both (sum|dy x| <= 33 800 x 16 < 2^24).  Integer data: y = S(exact) and
    dw exact, bit for bit; N(0,1) data: the bounds of the fma chain."""
    nat, st = _nat(), _ST[mode]
    B, H, W, Cn, k, stride = shape
    d_in = layer_inputs(B, H, W, 8, Cn, k, stride, seed=sum(shape), integer=True)
    x, w, dy = d_in["x"][..., 0].contiguous(), d_in["w"][:, :1].contiguous(), d_in["dy"]
    y = nat.conv2d_stem_st_fwd(x.float().to(DEV), w.float().to(DEV), stride, st)
    assert y.dtype is st and torch.equal(y.cpu(), conv2d_fwd(x[..., None], w, stride).float().to(st))
    dw = nat.conv2d_stem_st_bwd_dw(x.float().to(DEV), dy.float().to(st).to(DEV), tuple(w.shape), stride)
    assert torch.equal(_d(dw), conv2d_bwd(x[..., None], w, dy, stride)[1])
    worst = {}
    g = torch.Generator().manual_seed(sum(shape))
    xr, wr = torch.randn(B, H, W, generator=g).to(DEV), (torch.randn(Cn, 1, k, k, generator=g) / k).to(DEV)
    yr = nat.conv2d_stem_st_fwd(xr, wr, stride, st)
    _check_stem_fwd(xr, wr, stride, yr, st, worst)
    dyr = torch.randn(yr.shape, generator=g).to(st).to(DEV)
    _check_stem_dw(xr, dyr, tuple(wr.shape), stride, nat.conv2d_stem_st_bwd_dw(xr, dyr, tuple(wr.shape), stride), worst)


# (B, H, W, C): one pixel; odd sizes with C = 8; the fixture's map; 4 x 130 x 130 x 64 outputs = 1 081 600 channel quads, more than the
# 4096 x 256 threads of one grid pass (forward and backward)
_POOLS = [(1, 1, 1, 8), (2, 5, 7, 8), (2, 20, 17, 64), (4, 260, 260, 64)]


@gpu
@pytest.mark.parametrize("mode", list(_ST))
@pytest.mark.parametrize("shape", _POOLS, ids=lambda s: "-".join(map(str, s)))
def test_maxpool_st_selects_exactly_and_rounds_the_gradient_once(shape, mode):
    """Integer data in [0, 2] (most windows tie, as after a ReLU) and in [-4, -1] (padding must never win): the pool and, with integer
    gradients, its backward are exact -- the first maximum takes the gradient; N(0,1) gradients: the fp32 sum of at most four of them,
    rounded once."""
    nat, st = _nat(), _ST[mode]
    g = torch.Generator().manual_seed(sum(shape))
    big = shape[1] > 100
    for lo, hi in ((0, 2),) if big else ((0, 2), (-4, -1)):
        x = torch.randint(lo, hi + 1, shape, generator=g).float()
        ry, idx = maxpool_fwd(x)
        dy = torch.randint(-4, 5, tuple(ry.shape), generator=g).float()
        y = nat.maxpool3x3s2_st_fwd(x.to(st).to(DEV))
        dx = nat.maxpool3x3s2_st_bwd(x.to(st).to(DEV), dy.to(st).to(DEV))
        assert y.dtype is st and torch.equal(y.cpu().float(), ry)
        assert torch.equal(dx.cpu().float(), maxpool_bwd(idx, dy, shape[1], shape[2]))      # |sum| <= 16: exact in S
    if not big:
        xs = torch.randn(shape, generator=g).to(st).to(DEV)
        dys = torch.randn(tuple(ry.shape), generator=g).to(st).to(DEV)
        _check_pool(xs, nat.maxpool3x3s2_st_fwd(xs), dys, nat.maxpool3x3s2_st_bwd(xs, dys), st, {})


@gpu
@pytest.mark.parametrize("mode", list(_ST))
def test_mean_and_relu_mask_st(mode):
    """(B, HW, C) = (3, 35, 8), (2, 4, 512) and (33, 500, 512): 1 056 000 vectors of 8 in the mean's gradient and in the mask, more
    than one grid pass.  The mask is exact: zeros (of either sign) stop the gradient, everything else -- NaN too -- passes it."""
    nat, st = _nat(), _ST[mode]
    worst = {}
    g = torch.Generator().manual_seed(8)
    for B, HW, Cn in ((3, 35, 8), (2, 4, 512), (33, 500, 512)):
        x = (torch.randn(B, HW, Cn, generator=g) + 0.5).to(st).to(DEV)
        mean = nat.mean_hw_st_fwd(x)
        assert mean.dtype is torch.float32
        _check_mean(x, mean, worst)
        dmean = torch.randn(B, Cn, generator=g).to(DEV)
        dx = nat.mean_hw_st_bwd(dmean, HW, st)
        assert dx.dtype is st
        _check_mean_bwd(dmean, HW, dx, st, worst)
        y = x.clamp_min(0)
        y.view(-1)[1], y.view(-1)[2], y.view(-1)[3] = -0.0, float("nan"), float("inf")
        dy = torch.randn(B, HW, Cn, generator=g).to(st).to(DEV)
        _check_mask(dy, y, nat.relu_mask_st_bwd(dy, y))
    print(f"resnet-storage mean {mode}: error / bound " + " ".join(f"{k}={v:.2f}" for k, v in worst.items()))


# ------------------------------------------------------------------------------------------ 5. block and model, teacher-forced
class _Spy:
    """Records every ``nat.*_st_*`` call of a forward + backward with its inputs as they were BEFORE the call (clones) and checks each
    stored tensor afterwards against float64 on those inputs."""
    NAMES = ("conv2d_st_fwd", "conv2d_st_bwd", "bn_act_st_fwd", "bn_act_st_bwd", "relu_mask_st_bwd", "conv2d_stem_st_fwd",
             "conv2d_stem_st_bwd_dw", "maxpool3x3s2_st_fwd", "maxpool3x3s2_st_bwd", "mean_hw_st_fwd", "mean_hw_st_bwd")

    def __init__(self, monkeypatch):
        nat = _nat()
        self.calls, self.bns = [], {}
        make_bn = nat.make_bn

        def spy_make_bn(gamma, beta, rm, rv, **kw):
            bn = make_bn(gamma, beta, rm, rv, **kw)
            self.bns[id(bn)] = (bn, gamma, beta, rm, rv, kw["training"])
            return bn
        monkeypatch.setattr(nat, "make_bn", spy_make_bn)
        for name in self.NAMES:
            monkeypatch.setattr(nat, name, self._wrap(name, getattr(nat, name)))

    def _wrap(self, name, fn):
        def spy(*a, **kw):
            pre = {}
            if name == "conv2d_st_bwd" and kw.get("dx") is not None:
                pre["dx_prev"] = kw["dx"].clone()
            if name == "bn_act_st_fwd":
                _, gamma, beta, rm, rv, training = self.bns[id(a[1])]
                pre.update(gamma=gamma, beta=beta, rm0=rm.clone(), rv0=rv.clone(), training=training, rm=rm, rv=rv)
            # (a later call may write into one of these tensors -- conv1's dx is accumulated onto dsum: keep them as they are NOW)
            keep = lambda t: t.clone() if torch.is_tensor(t) else t
            a_in, kw_in = tuple(keep(t) for t in a), {k: keep(v) for k, v in kw.items() if k in ("res", "res_ss", "part")}
            out = fn(*a, **kw)
            if name == "bn_act_st_fwd":
                pre.update(rm1=pre["rm"].clone(), rv1=pre["rv"].clone())
            # outputs likewise, except the weight gradients: their partial sums may be queued until the end of the backward pass
            if name in ("conv2d_st_bwd",):
                rec = (keep(out[0]), out[1])
            elif name == "conv2d_stem_st_bwd_dw":
                rec = out
            else:
                rec = tuple(keep(t) for t in out) if isinstance(out, tuple) else keep(out)
            self.calls.append((name, a_in, kw_in, pre, rec))
            return out
        return spy

    def stored(self):
        """Every activation or activation-gradient tensor the calls produced (not the fp32 weight gradients and vectors)."""
        out = []
        for name, a, kw, pre, res in self.calls:
            if name == "conv2d_stem_st_bwd_dw":
                continue
            res = res[:1] if name in ("conv2d_st_bwd", "conv2d_st_fwd") and isinstance(res, tuple) else (res if isinstance(res, tuple) else (res,))
            out += [t for t in res if torch.is_tensor(t) and t.dim() >= 3]
        return out

    def check(self, st, subnormal=False):
        nat, worst = _nat(), {}
        torch.cuda.synchronize()
        for name, a, kw, pre, out in self.calls:
            if name == "conv2d_st_fwd":
                y, part = out if isinstance(out, tuple) else (out, None)
                _check_conv_fwd(a[0], a[1], a[2] if len(a) > 2 else kw.get("stride", 1), y, st, worst)
                if part is not None:
                    _check_partials(y, part, worst)
            elif name == "conv2d_st_bwd":
                _check_conv_bwd(a[0], a[1], a[2], a[3], out[0], out[1], st, worst, dx_prev=pre.get("dx_prev"), subnormal=subnormal)
            elif name == "bn_act_st_fwd":
                y, ss, mr = out
                _check_bn_stats(a[0], pre["gamma"], pre["beta"], pre["rm0"], pre["rv0"], pre["training"], ss, mr, pre["rm1"], pre["rv1"], worst,
                                k=2 if kw.get("part") is None else 65)
                if y is not None:
                    _check_bn_apply(a[0], ss, a[2] == nat.LIN_RELU, kw.get("res"), kw.get("res_ss"), y, st, worst)
            elif name == "bn_act_st_bwd":
                _check_bn_bwd(a[0], a[1], a[2], a[3], a[4] == nat.LIN_RELU, a[5], *out, st, worst)
            elif name == "relu_mask_st_bwd":
                _check_mask(a[0], a[1], out)
            elif name == "conv2d_stem_st_fwd":
                _check_stem_fwd(a[0], a[1], a[2], out, st, worst)
            elif name == "conv2d_stem_st_bwd_dw":
                _check_stem_dw(a[0], a[1], a[2], a[3], out, worst)
            elif name == "maxpool3x3s2_st_fwd":
                self.pool_x, self.pool_y = a[0], out
            elif name == "maxpool3x3s2_st_bwd":
                _check_pool(a[0], self.pool_y, a[1], out, st, worst)
            elif name == "mean_hw_st_fwd":
                _check_mean(a[0], out, worst)
            elif name == "mean_hw_st_bwd":
                _check_mean_bwd(a[0], a[1], out, st, worst)
        return worst


def _block(inplanes, planes, stride, mode, seed):
    from wakeword_trainer_home_amd.models.resnet import BasicBlock
    torch.manual_seed(seed)
    blk = BasicBlock(inplanes, planes, stride, mode, mode).to(DEV)
    with torch.no_grad():
        for m in blk.modules():
            if hasattr(m, "running_mean"):
                m.weight.uniform_(0.5, 1.5)
                m.bias.uniform_(-0.3, 0.3)
    return blk.train()


@gpu
@pytest.mark.parametrize("mode", list(_ST))
@pytest.mark.parametrize("case", [(64, 128, 2, 3, 6, 4), (64, 64, 1, 4, 20, 17)], ids=["downsample-3x6x4", "identity-4x20x17"])
def test_basic_block_st_every_stored_tensor_meets_its_ops_bound(case, mode, monkeypatch):
    """BasicBlock(64,128,2) at B=3, 6x4 and BasicBlock(64,64,1) at B=4, 20x17: every tensor the forward and the backward store is
    within the bound of its op, applied to what the device produced upstream -- the wiring, without compounding rounding flips.
    Everything saved for the backward has the storage dtype, and the block is one autograd node."""
    inplanes, planes, stride, B, H, W = case
    st = _ST[mode]
    blk = _block(inplanes, planes, stride, mode, seed=sum(case))
    spy = _Spy(monkeypatch)
    x = torch.randn(B, H, W, inplanes, device=DEV).to(st).requires_grad_(True)
    out = blk(x)
    assert out.dtype is st and out.grad_fn.name() == "_BlockFnBackward" and out.grad_fn.next_functions[0][0].name() == "torch::autograd::AccumulateGrad"
    saved = [t for t in out.grad_fn.saved_tensors if t.dim() == 4 and t.shape[-1] in (inplanes, planes) and t.shape[0] == B]
    assert len(saved) == (6 if blk.downsample is not None else 5) and all(t.dtype is st for t in saved)
    out.backward(torch.randn(out.shape, device=DEV).to(st))
    assert x.grad.dtype is st and all(p.grad is not None and p.grad.dtype is torch.float32 for p in blk.parameters())
    names = [c[0] for c in spy.calls]
    assert names.count("conv2d_st_fwd") == names.count("conv2d_st_bwd") == (3 if blk.downsample is not None else 2)
    assert all(t.dtype is st for t in spy.stored())
    worst = spy.check(st)
    print(f"resnet-storage block {case} {mode}: error / bound " + " ".join(f"{k}={v:.2f}" for k, v in sorted(worst.items())))


def _model(sd, **kw):
    from wakeword_trainer_home_amd.models import ResNet18Wakeword
    model = ResNet18Wakeword(**kw)
    model.load_state_dict(sd)
    return model.to(DEV)


@gpu
@pytest.mark.parametrize("mode,scale", [("bf16", 1.0), ("fp16", _SCALE["fp16"]), ("fp16", 1.0)], ids=["bf16", "fp16-loss-scale", "fp16-unscaled"])
def test_resnet18_st_every_stored_tensor_meets_its_ops_bound(mode, scale, monkeypatch):
    """The whole model on the fixture input (2,1,40,33), train mode, dropout 0: 20 convolutions, 20 BatchNorms, the stem, the pool
    and the mean, forward and backward, each held to its op's bound on the device's own upstream tensors; every stored activation and
    activation gradient has the storage dtype, parameters' gradients, ss / mr and the pooled features are fp32.  fp16: the backward
    runs at the loss scale, as it does under the Trainer.  (Measured without it: 215 of the 4096 gradients that reach layer4.1.conv2
    are fp16 subnormals, and there the weight-gradient entries of |dw| = 2.9e-7 miss the fp32 bound by up to 18.8x, an absolute
    2.7e-12 -- layer4.1.conv1 4.2x, layer4.0.conv2 2.0x, layer4.0.conv1 1.4x; every other op and layer held.  It is the f16
    matrix instruction on subnormal operands, not these kernels: on the same x and dy the fp32-storage fp16 matrix mode
    (ww_conv2d_bwd) misses by the same 18.8x, the fp32 matrix mode reads 0.31x, and with dy times 1024 -- exact, out of the
    subnormal range -- this kernel reads 0.26x.  A single product with a subnormal operand is exact; sums of several are not.)
    The unscaled fp16 run stays pinned: every op at the same bound, except that conv.dw allows each term with a subnormal operand
    the half spacing of fp16's subnormals (2^-25) times its other factor -- the accuracy RNE itself gave that operand when it was
    stored, so a weight gradient cannot mean more than that."""
    sd, g = golden_case()
    st = _ST[mode]
    model = _model(sd, dropout=0.0, mode=mode, storage=mode).train()
    spy = _Spy(monkeypatch)
    out = model(torch.from_numpy(g["x"]).to(DEV))
    (torch.nn.functional.cross_entropy(out, torch.from_numpy(g["y"]).to(DEV)) * scale).backward()
    names = [c[0] for c in spy.calls]
    assert names.count("conv2d_st_fwd") == names.count("conv2d_st_bwd") == 19 and names.count("bn_act_st_fwd") == names.count("bn_act_st_bwd") == 20
    assert names.count("relu_mask_st_bwd") == 8 and names.count("mean_hw_st_fwd") == names.count("mean_hw_st_bwd") == 1
    assert all(t.dtype is st for t in spy.stored()) and out.dtype is torch.float32
    assert all(p.grad.dtype is torch.float32 for p in model.parameters())
    worst = spy.check(st, subnormal=(mode == "fp16" and scale == 1.0))
    print(f"resnet18 storage {mode} x{scale:g} teacher-forced: error / bound " + " ".join(f"{k}={v:.2f}" for k, v in sorted(worst.items())))


# ------------------------------------------------------------------------------------------ 6. end to end, a sanity bound
def _end_to_end_yardstick(mode):
    """Distances to the float64 exact model of the storage restatement and of four copies perturbed by 1e-6 ahead of every storage
    rounding (seeds 1-4): equally valid roundings of the same contract.  -> (exact results, the largest distance per figure)."""
    key = ("e2e", mode)
    if key not in _REF:
        sd, g = golden_case()
        x64, y64 = torch.from_numpy(g["x"]).double(), torch.from_numpy(g["y"])
        ref0, lo0, go0 = ResNetRestated(sd).loss_and_grads(x64, y64)
        l2 = lambda a, b: ((a - b).norm() / b.norm()).item()
        top = dict(logits=0.0, loss=0.0, grads={n: 0.0 for n in go0})
        for perturb in (None, (1e-6, 1), (1e-6, 2), (1e-6, 3), (1e-6, 4)):
            ref, lo, go = ResNetStorageRestated(sd, st=_ST[mode], perturb=perturb).loss_and_grads(x64, y64)
            top["logits"], top["loss"] = max(top["logits"], (ref - ref0).abs().max().item()), max(top["loss"], abs(lo - lo0))
            top["grads"] = {n: max(top["grads"][n], l2(go[n], go0[n])) for n in go0}
        _REF[key] = ((ref0, lo0, go0), top)
    return _REF[key]


@gpu
@pytest.mark.parametrize("mode", list(_ST))
def test_resnet18_st_end_to_end_sanity(mode):
    """Logits, loss and per-tensor gradient l2 distances to the float64 exact model are within 4x (the fixture's margin) the largest
    of the same distances over the storage restatement and four perturbed copies of it.  A sanity bound only: roundings that flip
    compound through 17 layers, so equally valid evaluations differ by about as much as any of them does from float64."""
    sd, g = golden_case()
    (ref0, lo0, go0), top = _end_to_end_yardstick(mode)
    model = _model(sd, dropout=0.0, mode=mode, storage=mode).train()
    out = model(torch.from_numpy(g["x"]).to(DEV))
    loss = torch.nn.functional.cross_entropy(out, torch.from_numpy(g["y"]).to(DEV))
    (loss * _SCALE[mode]).backward()                      # fp16: at the loss scale, divided out below
    l2 = lambda a, b: ((a - b).norm() / b.norm()).item()
    dev = dict(logits=(_d(out) - ref0).abs().max().item(), loss=abs(loss.item() - lo0),
               grads={n: l2(_d(p.grad) / _SCALE[mode], go0[n]) for n, p in model.named_parameters()})
    rmax = max(dev["grads"][n] / top["grads"][n] for n in go0)
    print(f"resnet18 storage {mode} end to end, device | restatements (largest of 5) vs float64: logits {dev['logits']:.2e} | {top['logits']:.2e} "
          f"loss {dev['loss']:.2e} | {top['loss']:.2e} grads l2 max {max(dev['grads'].values()):.2e} | {max(top['grads'].values()):.2e} "
          f"(largest ratio {rmax:.2f}x)")
    assert dev["logits"] <= 4 * top["logits"] and dev["loss"] <= 4 * top["loss"]
    for n in go0:
        assert dev["grads"][n] <= 4 * top["grads"][n], (n, dev["grads"][n], top["grads"][n])


# ------------------------------------------------------------------------------------------ 7. properties
@gpu
@pytest.mark.parametrize("mode", list(_ST))
def test_resnet18_st_properties(mode):
    """Eval logits of a row do not depend on the batch's other rows; two identical training steps give identical bits."""
    sd, g = golden_case()
    x, y = torch.from_numpy(g["x"]).to(DEV), torch.from_numpy(g["y"]).to(DEV)
    model = _model(sd, dropout=0.0, mode=mode, storage=mode).eval()
    with torch.no_grad():
        ev, alone, swapped = model(x), model(x[1:].contiguous()), model(torch.stack([x[1], x[0]]))
    assert torch.isfinite(ev).all() and torch.equal(alone[0], ev[1]) and torch.equal(swapped[0], ev[1]) and torch.equal(swapped[1], ev[0])
    runs = []
    for _ in range(2):
        m = _model(sd, dropout=0.3, dropout_seed=4, mode=mode, storage=mode).train()
        out = m(x)
        torch.nn.functional.cross_entropy(out, y).backward()
        runs.append((out.detach().clone(), [p.grad.clone() for p in m.parameters()], {k: v.clone() for k, v in m.state_dict().items()}))
    assert torch.equal(runs[0][0], runs[1][0]) and all(torch.equal(a, b) for a, b in zip(runs[0][1], runs[1][1]))
    assert all(torch.equal(runs[0][2][k], runs[1][2][k]) for k in runs[0][2])
    assert all(int(v) == 1 for k, v in runs[0][2].items() if k.endswith("num_batches_tracked"))


@gpu
@pytest.mark.parametrize("mode", ["fp32", "bf16", "fp16"])
def test_storage_fp32_is_the_model_built_without_the_argument(mode):
    sd, g = golden_case()
    x, y = torch.from_numpy(g["x"]).to(DEV), torch.from_numpy(g["y"]).to(DEV)
    runs = []
    for kw in ({}, {"storage": "fp32"}):
        m = _model(sd, dropout=0.0, mode=mode, **kw).train()
        out = m(x)
        torch.nn.functional.cross_entropy(out, y).backward()
        runs.append((out.detach(), [p.grad for p in m.parameters()]))
    assert torch.equal(runs[0][0], runs[1][0]) and all(torch.equal(a, b) for a, b in zip(runs[0][1], runs[1][1]))


# ------------------------------------------------------------------------------------------ 8. the Trainer
def _trainer_cfg(batch_size=8, epochs=1):
    from wakeword_trainer_home_amd.config import get_preset
    cfg = get_preset("cnn_small_logmel40")
    cfg.training.epochs, cfg.optimizer.warmup_epochs, cfg.training.batch_size = epochs, 0, batch_size
    cfg.loss.label_smoothing = 0.0
    cfg.optimizer.mixed_precision = False
    cfg.training.checkpoint_frequency = "best_only"
    return cfg


def _batches(n, seed):
    from wakeword_trainer_home_amd.data import make_synthetic_batch
    wave, y = make_synthetic_batch(n, 5440, seed=seed)                 # 5440 samples: 35 frames
    y[::3] = 1
    return [(wave[i:i + 8], y[i:i + 8]) for i in range(0, n, 8)]


@gpu
@pytest.mark.parametrize("mode", list(_ST))
def test_trainer_trains_and_graph_replays_equal_eager_steps_bit_for_bit(mode, tmp_path):
    """Two epochs of two full batches and a ragged one (8, 8, 5 rows), eager and hip_graph=True: finite losses that change, and the
    replays equal the eager steps bit for bit (loss trace, parameters, buffers, optimizer moments).  fp16 runs under the
    DeviceGradScaler.  Changing a block's storage re-keys the captured graph."""
    from wakeword_trainer_home_amd.models import ResNet18Wakeword
    from wakeword_trainer_home_amd.training import Trainer
    from wakeword_trainer_home_amd.training.optimizer_factory import DeviceGradScaler, FlatFusedOptimizer
    batches = _batches(21, seed=6)
    assert len(batches[-1][0]) == 5
    runs = []
    for graph in (False, True):
        cfg = _trainer_cfg(epochs=2)
        cfg.training.hip_graph, cfg.training.hip_graph_auto = graph, False
        torch.manual_seed(11)
        model = ResNet18Wakeword(dropout=0.3, dropout_seed=2, mode=mode, storage=mode)
        t = Trainer(model, batches, batches[:1], cfg, checkpoint_dir=tmp_path / f"g{int(graph)}", device=DEV)
        assert isinstance(t.optimizer, FlatFusedOptimizer) and t._async_autograd
        assert isinstance(getattr(t, "scaler", None), DeviceGradScaler) == (mode == "fp16")
        rec = []
        t.add_callback(type("R", (), {"on_batch_end": lambda self, i, l, a: rec.append((i, l))})())
        t.train()
        runs.append((t, rec, {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}, copy.deepcopy(t.optimizer.state_dict())))
    assert runs[1][0]._graph is not None and runs[0][0]._graph is None
    assert len(runs[1][1]) == 6 and all(np.isfinite(l) for _, l in runs[0][1]) and len({l for _, l in runs[0][1]}) > 1
    assert runs[0][1] == runs[1][1], "loss traces differ"
    for k in runs[0][2]:
        assert torch.equal(runs[0][2][k], runs[1][2][k]), k
    for (ka, va), (kb, vb) in zip(sorted(runs[0][3]["state"].items()), sorted(runs[1][3]["state"].items())):
        for f in va:
            assert torch.equal(torch.as_tensor(va[f]).cpu(), torch.as_tensor(vb[f]).cpu()), (ka, f)
    t = runs[1][0]
    shape = (8, 1, 40, 35)
    key = t._graph_key(shape)
    assert key in t._graphs
    blk = t.model.resnet.layer1[0]
    blk.storage = torch.float32
    assert t._graph_key(shape) != key and t._graph_key(shape) not in t._graphs
    blk.storage = _ST[mode]
    assert t._graph_key(shape) == key


@gpu
@pytest.mark.parametrize("mode", list(_ST))
def test_nonfinite_batch_is_skipped_on_device(mode, tmp_path):
    """A batch with a NaN sample changes no parameter (the fused optimizer gets the flag on the device) and is not reported."""
    from wakeword_trainer_home_amd.models import ResNet18Wakeword
    from wakeword_trainer_home_amd.training import Trainer
    cfg = _trainer_cfg()
    torch.manual_seed(2)
    model = ResNet18Wakeword(dropout=0.0, mode=mode, storage=mode)
    batches = _batches(24, seed=6)
    bad = batches[1][0].clone()
    bad[3, 100] = float("nan")
    batches[1] = (bad, batches[1][1])
    t = Trainer(model, batches, batches[:1], cfg, checkpoint_dir=tmp_path, device=DEV)
    assert t._async_autograd and t.deferred_metrics
    seen, snaps = [], []
    t.add_callback(type("R", (), {"on_batch_end": lambda self, i, l, a: seen.append((i, l))})())
    orig = t._step_autograd_async
    pnames = [n for n, _ in model.named_parameters()]

    def spy(inputs, targets, idx):
        snaps.append({k: v.clone() for k, v in model.state_dict().items() if k in pnames})
        return orig(inputs, targets, idx)
    t._step_autograd_async = spy
    t.train_epoch(0)
    after = {k: v.clone() for k, v in model.state_dict().items() if k in pnames}
    assert [i for i, _ in seen] == [0, 2] and all(np.isfinite(l) for _, l in seen)
    assert any(not torch.equal(snaps[0][k], snaps[1][k]) for k in snaps[0])
    assert all(torch.equal(snaps[1][k], snaps[2][k]) for k in snaps[1])
    assert any(not torch.equal(snaps[2][k], after[k]) for k in after)


# ------------------------------------------------------------------------------------------ 9. argument checks
@gpu
def test_argument_checks_return_error_codes_before_any_launch():
    """WW_ACT_F32 as the storage, channel counts that are no multiple of 8 and null pointers are WW_E_INVALID, a short scratch is
    WW_E_WORKSPACE -- before any launch: the output buffers keep their sentinel.  The bindings raise WW_E_INVALID as ValueError."""
    nat = _nat()
    lib, cx = nat.load(), nat.ctx(DEV)
    B, H, W, Cin, Cout, k = 2, 5, 7, 8, 16, 3
    h = lambda *s: torch.full(s, 7.0, device=DEV, dtype=torch.bfloat16)
    f = lambda *s: torch.full(s, 7.0, device=DEV)
    x, w, y, dx, dw = h(B, H, W, Cin), f(Cout, Cin, k, k), h(B, H, W, Cout), h(B, H, W, Cin), f(Cout, Cin, k, k)
    nbytes = lib.ww_conv2d_st_scratch_bytes(B, H, W, Cin, Cout, k, 1)
    scratch = f(nbytes // 4)
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    fwd = lambda st=1, cin=Cin, cout=Cout, sb=nbytes, xx=x: lib.ww_conv2d_st_fwd(cx, st, p(xx), p(w), B, H, W, cin, cout, k, 1, p(y), None, p(scratch), sb, None)
    assert fwd(st=0) == -1 and b"storage" in lib.ww_last_error()
    assert fwd(st=3) == -1 and fwd(cin=4) == -1 and b"multiples of 8" in lib.ww_last_error()
    assert fwd(cout=12) == -1 and fwd(xx=None) == -1 and fwd(sb=nbytes - 4) == -3 and b"scratch too small" in lib.ww_last_error()
    bwd = lambda st=1, cin=Cin, sb=nbytes, gg=y: lib.ww_conv2d_st_bwd(cx, st, p(x), p(w), p(gg), B, H, W, cin, Cout, k, 1, p(dx), 0, p(dw), p(scratch), sb, None)
    assert bwd(st=0) == -1 and bwd(cin=12) == -1 and bwd(gg=None) == -1 and bwd(sb=16) == -3
    ss, mr = f(2 * Cout), f(2 * Cout)
    bn_t = [f(Cout) for _ in range(4)]
    bn = nat.make_bn(*bn_t, training=True)
    bnf = lambda st=1, c=Cout, xx=y: lib.ww_bn_act_st_fwd(cx, st, p(xx), B * H * W, c, C.byref(bn), 0, None, None, None, 0, p(y), p(ss), p(mr), p(scratch), None)
    assert bnf(st=0) == -1 and bnf(c=12) == -1 and bnf(xx=None) == -1
    bnb = lambda st=1, c=Cout, xx=y: lib.ww_bn_act_st_bwd(cx, st, p(xx), p(y), B * H * W, c, p(ss), p(mr), 0, 1, p(y), p(ss), p(mr), p(scratch), None)
    assert bnb(st=0) == -1 and bnb(c=4) == -1 and bnb(xx=None) == -1
    img, sw = f(B, H, W), f(16, 1, 7, 7)
    sy = h(B, 3, 4, 16)
    stem = lambda st=1, c=16, xx=img: lib.ww_conv2d_stem_st_fwd(cx, st, p(xx), p(sw), B, H, W, c, 7, 2, p(sy), None)
    assert stem(st=0) == -1 and stem(c=12) == -1 and stem(xx=None) == -1
    assert lib.ww_conv2d_stem_st_bwd_dw(cx, 1, p(img), p(sy), B, H, W, 16, 7, 2, p(sw), p(scratch), 16, None) == -3
    assert lib.ww_conv2d_stem_st_bwd_dw(cx, 0, p(img), p(sy), B, H, W, 16, 7, 2, p(sw), p(scratch), nbytes, None) == -1
    assert lib.ww_maxpool3x3s2_st_fwd(cx, 0, p(x), B, H, W, Cin, p(y), None) == -1 and lib.ww_maxpool3x3s2_st_fwd(cx, 1, p(x), B, H, W, 12, p(y), None) == -1
    assert lib.ww_maxpool3x3s2_st_bwd(cx, 2, p(x), None, B, H, W, Cin, p(dx), None) == -1 and lib.ww_maxpool3x3s2_st_bwd(cx, 0, p(x), p(y), B, H, W, Cin, p(dx), None) == -1
    assert lib.ww_mean_hw_st_fwd(cx, 0, p(x), B, H * W, Cin, p(ss), None) == -1 and lib.ww_mean_hw_st_fwd(cx, 1, p(x), B, H * W, 4, p(ss), None) == -1
    assert lib.ww_mean_hw_st_bwd(cx, 0, p(ss), B, H * W, Cin, p(dx), None) == -1 and lib.ww_mean_hw_st_bwd(cx, 1, None, B, H * W, Cin, p(dx), None) == -1
    assert lib.ww_relu_mask_st_bwd(cx, 0, p(y), p(y), y.numel(), p(dx), None) == -1 and lib.ww_relu_mask_st_bwd(cx, 1, p(y), p(y), 12, p(dx), None) == -1
    torch.cuda.synchronize()
    for t in (y, dx, dw, sw, sy, ss, mr):
        assert t.eq(7.0).all()          # nothing was launched
    with pytest.raises(ValueError, match="multiples of 8"):
        nat.conv2d_st_fwd(h(B, H, W, 4), f(Cout, 4, k, k))
    with pytest.raises(ValueError, match="bfloat16 or float16"):
        nat.conv2d_st_fwd(f(B, H, W, Cin), w)
    with pytest.raises(ValueError, match="one dtype"):
        nat.conv2d_st_bwd(x, w, y.half(), 1)
