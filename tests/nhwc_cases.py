"""Float64 restatements, case builders and error bounds for the channels-last layer library (csrc/ww_nhwc.hip, ww_se.hip), shared
by test_nhwc_layers_host.py and test_nhwc_layers_gpu.py.  No device code; every contract is written out by hand, channels-last.

Two instruments:

INTEGER-EXACT cases.  Small integers with a pattern of their own per sample, image row, channel quad and channel (channel 0 is a
ramp whose phase depends on sample and row), so a read across an image, group, chunk or quad boundary changes a sum and cannot
cancel.  Every product and partial sum is an integer below 2^24, which fp32 holds exactly in any order: the device must return
the reference bit for bit.  BatchNorm gets columns  m_c + a t  with t = +-1 on exactly M/2 rows each (balanced pseudo-random
order per column), m_c an integer, a a power of two and eps = 3 a^2: then mean = m_c, var = a^2, rstd = 1/(2a), and with
gamma = 2a g_c (g_c, beta_c integers) scale = g_c, shift = beta_c - m_c g_c and y = beta_c +- a g_c are exact whatever the
order of the sums and whether or not the compiler contracts  q/M - mean^2  into an fma.  ``exactness`` asserts the conditions.

ROUND-OFF cases.  N(0,1)-like data, PER-ELEMENT bounds  K * u * S[i],  u = 2^-24 (fp32 unit round-off), S[i] the sum of the
absolute values of the terms that make element i.  The K are derived here from the kernels' order of operations, not fitted:

BatchNorm forward, partials accumulated to depth D in fp32 (D = 1: fp64 accumulation, one rounding when a chunk's sum is stored
as fp32 -- k_colstats, col_reduce_store; the GEMM epilogue, the LDS depthwise kernel and the stem accumulate D - 1 values in fp32
registers first).  With ma = mean|x|, m2 = mean(x^2), r = D m2 / (var + eps):
    |d mean| <= D u ma                                    (each partial: D u sum|x| of its rows)
    |d var|  <= D u m2 + 2 |mean| D u ma <= 3 D u m2      (q/M and mean^2; ma^2 <= m2) = 3 D u (1 + (mean/std)^2) var
    scale = fl32(gamma rstd):  relative 1.5 r u + u       (rstd = (var+eps)^-1/2: half the relative error of var + eps; one cast)
    shift = fl32(beta - mean scale):  u |shift| + |scale| D u ma + |mean| |scale| 1.5 r u
    z = fmaf(x, scale, shift):  |x||scale| (1 + 1.5 r) u + [shift] + u |z|
  every factor |x||scale|, |shift|, |scale| ma, |mean||scale|, |z| is <= S = |scale| (|x| + ma) + |beta|, so
    |dz| <= (3 + D + 3 r) u S                            eval mode (no statistics): r = 0, D = 1 -> 4 u S
  activations: identity / ReLU are 1-Lipschitz and add nothing;  hardswish z clamp(z+3,0,6) (1/6) is 1.5-Lipschitz and rounds
  z+3, the product, the constant and the second product: 1.5 |dz| + 4 u S (|h| <= |z| <= S);  hardsigmoid is 1/6-Lipschitz with
  values <= 1: |dz|/6 + 3 u.  A residual adds one rounding of the sum.
BatchNorm backward from given fp32 ss / mr (the reference takes the same): dz = da act'(z32) with z32 the fp32 fma (restated by
rounding the float64 value: the kink decisions are then the device's), A = |da| gmax on the active branch (gmax = 1, 1.5, 1,
1/6), Kg = 0 / 4 / 0 / 2 roundings in act' and the product (identity, hardswish, ReLU, hardsigmoid):
    dbeta  = s1:  Kg u SA + u SA (chunk partial) + u |s1| (cast of the total)          <= (2 + Kg) u SA,   SA = sum A
    dgamma = s2:  xhat = fl(fl(x - mu) rs) carries 2 u |xhat|                           <= (4 + Kg) u SAx,  SAx = sum A |xhat|
    dx = sc (dz - s1 invM - xhat s2 invM), invM = fl(1/M): T1 = A, T2 = SA/M, T3 = |xhat| SAx/M carry Kg, (2+Kg)+2 and
         (4+Kg)+2+3 roundings, the two subtractions and the last product 3 more on T1+T2+T3: <= (12 + Kg) u |sc| (T1+T2+T3)
    eval: dx = sc dz <= (1 + Kg) u |sc| A
A dot product of n terms summed to depth d in fp32 (fma chain + tree): d u sum|terms| -- the matrix-core GEMM of the 1x1 conv
(d = K + 1), the SE row dots (d = 4 SE_Q + log2(32) + 1 = 46)."""
import math

import numpy as np
import torch
import torch.nn.functional as Fn

from oracle.rounding import mround

U = 2.0 ** -24
EPS, MOMENTUM = 1e-3, 0.01
LIMIT = float(2 ** 24)
f32 = lambda t: t.float().double()                      # the fp32 value nearest to each float64 entry
r32 = lambda v: float(np.float32(v))
MODES = {"fp32": None, "bf16": torch.bfloat16, "fp16": torch.float16}


# ------------------------------------------------------------------------------------------ activations (WW_LIN_*: 0 1 2 3)
def act(kind, z):
    if kind == 1:
        return z * (z + 3).clamp(0, 6) / 6
    if kind == 2:
        return z.clamp_min(0)
    if kind == 3:
        return (z + 3).clamp(0, 6) / 6
    return z


def act32(kind, z):
    """lin_act on fp32 values, operation by operation in float32 (for exact-integer z the device's bits)."""
    z = z.float()
    c6 = torch.tensor(1.0 / 6.0, dtype=torch.float32)
    if kind == 1:
        return ((z * (z + 3).clamp(0, 6)) * c6).double()
    if kind == 2:
        return z.clamp_min(0).double()
    if kind == 3:
        return ((z + 3).clamp(0, 6) * c6).double()
    return z.double()


def act_grad(kind, z, zb=None):
    """(act'(z), active branch) with torch's conventions at the kinks: relu'(0) = 0, hardswish'(-3) = 0, (3) = 1, hardsigmoid'(+-3) = 0.
    zb: the value the branch is decided on (the device's fp32 z), z by default."""
    one = torch.ones_like(z)
    zb = z if zb is None else zb
    if kind == 1:
        return torch.where(zb <= -3, 0 * one, torch.where(zb < 3, z / 3 + 0.5, one)), zb > -3
    if kind == 2:
        return (zb > 0).double(), zb > 0
    if kind == 3:
        inside = (zb > -3) & (zb < 3)
        return inside.double() / 6, inside
    return one, one.bool()


GMAX = {0: 1.0, 1: 1.5, 2: 1.0, 3: 1.0 / 6.0}
KG = {0: 0, 1: 4, 2: 0, 3: 2}


# ------------------------------------------------------------------------------------------ BatchNorm (+activation)
def bn_fwd(x, gamma, beta, rm, rv, kind, training=True, eps=EPS, momentum=MOMENTUM, res=None):
    """x (M, C) float64 -> everything ww_bn_act_fwd leaves: y, ss = scale|shift, mr = mean|rstd, the running statistics as
    nn.BatchNorm2d moves them (biased variance normalises, unbiased variance is tracked).  eps, momentum: the fp32 values."""
    M = x.shape[0]
    eps, momentum = r32(eps), r32(momentum)
    if training:
        mean = x.mean(0)
        var = ((x - mean) ** 2).mean(0)
    else:
        mean, var = rm.clone(), rv.clone()
    rstd = 1.0 / torch.sqrt(var + eps)
    scale = gamma * rstd
    shift = beta - mean * scale
    z = x * scale + shift
    y = act(kind, z)
    if res is not None:
        y = y + res
    out = dict(y=y, z=z, mean=mean, var=var, ss=torch.cat([scale, shift]), mr=torch.cat([mean, rstd]), rm=rm, rv=rv)
    if training and rm is not None:
        out["rm"] = (1 - momentum) * rm + momentum * mean
        out["rv"] = (1 - momentum) * rv + momentum * (var * M / (M - 1) if M > 1 else var)
    return out


def bn_fwd_bounds(x, ref, gamma, beta, kind, training=True, eps=EPS, momentum=MOMENTUM, res=None, D=1):
    """per-element bounds (module docstring) on what bn_fwd returns, partials accumulated to depth D in fp32"""
    M, C = x.shape
    eps, momentum = r32(eps), r32(momentum)
    mean, var = ref["mean"], ref["var"]
    scale, shift, rstd = ref["ss"][:C], ref["ss"][C:], ref["mr"][C:]
    if training:
        ma, m2 = x.abs().mean(0), (x * x).mean(0)
        r = D * m2 / (var + eps)
        kz = 3 + D + 3 * r
    else:
        ma, m2, r, D, kz = mean.abs(), mean * mean, torch.zeros(C, dtype=torch.float64), 1, 4.0
    S = scale.abs() * (x.abs() + ma) + beta.abs()
    bz = U * kz * S
    by = {0: bz, 2: bz, 1: 1.5 * bz + 4 * U * S, 3: bz / 6 + 3 * U}[kind]
    if res is not None:
        by = by + U * ref["y"].abs()
    b = dict(y=by, S=S, mean=U * (D * ma + mean.abs()), rstd=U * rstd * (1 + 1.5 * r), var_rel=3 * U * r,
             scale=U * scale.abs() * (1 + 1.5 * r), shift=U * (shift.abs() + scale.abs() * D * ma + 1.5 * r * mean.abs() * scale.abs()))
    if training and ref["rm"] is not None:
        b["rm"] = momentum * U * D * ma + U * ref["rm"].abs()
        b["rv"] = momentum * 3 * U * D * m2 * (M / (M - 1) if M > 1 else 1) + U * ref["rv"].abs()
    return b


def bn_bwd(x, da, ss, mr, kind, training=True):
    """ww_bn_act_bwd from the fp32 ss / mr it is handed (float64 copies): (dx, dgamma, dbeta), their bounds, and the S of each
    (sum of the absolute values of its terms; bound = K u S)."""
    M, C = x.shape
    sc, sf, mu, rs = ss[:C], ss[C:], mr[:C], mr[C:]
    z = x * sc + sf
    g, active = act_grad(kind, z, f32(z))
    dz = da * g
    xh = (x - mu) * rs
    s1, s2 = dz.sum(0), (dz * xh).sum(0)
    A = da.abs() * GMAX[kind] * active
    SA, SAx = A.sum(0), (A * xh.abs()).sum(0)
    kg = KG[kind]
    if training:
        dx = sc * (dz - s1 / M - xh * s2 / M)
        bdx = U * (12 + kg) * sc.abs() * (A + SA / M + xh.abs() * SAx / M)
    else:
        dx = sc * dz
        bdx = U * (1 + kg) * sc.abs() * A
    sdx = sc.abs() * (A + SA / M + xh.abs() * SAx / M) if training else sc.abs() * A
    return (dict(dx=dx, dgamma=s2, dbeta=s1), dict(dx=bdx, dgamma=U * (4 + kg) * SAx, dbeta=U * (2 + kg) * SA),
            dict(dx=sdx, dgamma=SAx, dbeta=SA))


# ------------------------------------------------------------------------------------------ depthwise k x k, stem, 1x1
def out_hw(H, W, k, s):
    return (H + 2 * (k // 2) - k) // s + 1, (W + 2 * (k // 2) - k) // s + 1


def _taps(xp, kh, kw, Ho, Wo, s):
    return xp[:, kh:kh + s * (Ho - 1) + 1:s, kw:kw + s * (Wo - 1) + 1:s]


def dw_fwd(x, w, k, s):
    """x (B,H,W,C), w (C,k,k): depthwise Conv2d(C, C, k, s, padding=k//2, groups=C, bias=False) -> y (B,Ho,Wo,C)"""
    B, H, W, C = x.shape
    Ho, Wo = out_hw(H, W, k, s)
    p = k // 2
    xp = Fn.pad(x, (0, 0, p, p, p, p))
    y = torch.zeros(B, Ho, Wo, C, dtype=torch.float64)
    for kh in range(k):
        for kw in range(k):
            y += _taps(xp, kh, kw, Ho, Wo, s) * w[:, kh, kw]
    return y


def dw_bwd(x, w, dy, k, s):
    """-> (dx (B,H,W,C), dw (C,k,k)) of dw_fwd"""
    B, H, W, C = x.shape
    Ho, Wo = out_hw(H, W, k, s)
    p = k // 2
    xp = Fn.pad(x, (0, 0, p, p, p, p))
    dxp = torch.zeros_like(xp)
    dw = torch.zeros_like(w)
    for kh in range(k):
        for kw in range(k):
            _taps(dxp, kh, kw, Ho, Wo, s).add_(dy * w[:, kh, kw])
            dw[:, kh, kw] = (_taps(xp, kh, kw, Ho, Wo, s) * dy).sum((0, 1, 2))
    return dxp[:, p:p + H, p:p + W].contiguous(), dw


def stem_fwd(x, w):
    """x (B,H,W) one-channel images, w (C,3,3): Conv2d(1, C, 3, stride 2, padding 1, bias=False) -> y (B,Ho,Wo,C)"""
    B, H, W = x.shape
    Ho, Wo = (H + 1) // 2, (W + 1) // 2
    xp = Fn.pad(x, (1, 1, 1, 1))
    y = torch.zeros(B, Ho, Wo, w.shape[0], dtype=torch.float64)
    for kh in range(3):
        for kw in range(3):
            y += _taps(xp, kh, kw, Ho, Wo, 2)[..., None] * w[:, kh, kw]
    return y


def stem_dw(x, dy):
    B, H, W = x.shape
    Ho, Wo = (H + 1) // 2, (W + 1) // 2
    xp = Fn.pad(x, (1, 1, 1, 1))
    dw = torch.zeros(dy.shape[-1], 3, 3, dtype=torch.float64)
    for kh in range(3):
        for kw in range(3):
            dw[:, kh, kw] = (_taps(xp, kh, kw, Ho, Wo, 2)[..., None] * dy).sum((0, 1, 2))
    return dw


def im2col3x3s2(x):
    B, H, W = x.shape
    Ho, Wo = (H + 1) // 2, (W + 1) // 2
    xp = Fn.pad(x, (1, 1, 1, 1))
    return torch.stack([_taps(xp, t // 3, t % 3, Ho, Wo, 2) for t in range(9)], -1).reshape(-1, 9)


def conv1x1(x, w, mode="fp32"):
    """x (M,K) @ w (N,K)^T with both operands rounded to the matrix mode's type -> (y, S = sum of |products|)"""
    xr, wr = mround(x, MODES[mode]), mround(w, MODES[mode])
    return xr @ wr.t(), xr.abs() @ wr.abs().t()


# ------------------------------------------------------------------------------------------ squeeze-excitation
def se_fwd(x, w1, b1, w2, b2):
    """torchvision SqueezeExcitation: s = mean_hw x, pre1 = W1 s + b1, pre2 = W2 relu(pre1) + b2, y = x hardsigmoid(pre2)"""
    s = x.mean(1)
    pre1 = s @ w1.t() + b1
    pre2 = pre1.clamp_min(0) @ w2.t() + b2
    return dict(s=s, pre1=pre1, pre2=pre2, y=x * act(3, pre2)[:, None, :])


SE_DEPTH = 46


def se_fwd_stage_bounds(x, w1, b1, w2, b2, s, pre1, pre2):
    """each stage from the DEVICE's fp32 inputs of that stage (s, pre1, pre2 as float64): reference value and bound"""
    h = pre1.clamp_min(0)
    return dict(s=(x.mean(1), 2 * U * x.abs().mean(1)),
                pre1=(s @ w1.t() + b1, SE_DEPTH * U * (s.abs() @ w1.abs().t() + b1.abs())),
                pre2=(h @ w2.t() + b2, SE_DEPTH * U * (h @ w2.abs().t() + b2.abs())),
                y=(x * act(3, pre2)[:, None, :], 4 * U * x.abs()))


def se_bwd(x, dy, s, pre1, pre2, w1, w2):
    """backward of se_fwd from the kept s, pre1, pre2 -> dx, dw1, db1, dw2, db2 and per-element bounds.  Every product of the
    chain is an fp32 fma sum of depth <= its length, so a stage's bound is the incoming error through |W| plus depth * u *
    sum|terms| of its own sum; dgate is an fp64 sum cast once."""
    B, HW, C = x.shape
    Cs = w1.shape[0]
    g = act(3, pre2)
    gg, _ = act_grad(3, pre2)
    h, hm = pre1.clamp_min(0), (pre1 > 0).double()
    dgate = (dy * x).sum(1)
    e = 2 * U * (dy * x).abs().sum(1)
    dpre2 = dgate * gg
    e = e * gg + 2 * U * dpre2.abs()
    d2 = math.ceil(C / 16) + 64 + 1                     # se_wcolsum: rows / lanes fma chain + <= 64 lanes summed in order
    dh = dpre2 @ w2
    e_h = e @ w2.abs() + d2 * U * (dpre2.abs() @ w2.abs())
    dpre1 = dh * hm
    e1 = e_h * hm
    d1 = math.ceil(Cs / 4) + 64 + 1
    dpool = dpre1 @ w1
    e_p = e1 @ w1.abs() + d1 * U * (dpre1.abs() @ w1.abs())
    dx = dy * g[:, None, :] + dpool[:, None, :] / HW
    bdx = e_p[:, None, :] / HW + U * (3 * dpool.abs()[:, None, :] / HW + 6 * (dy * g[:, None, :]).abs())
    db = math.ceil(B / 32) + 32 + 1                     # k_se_wgrad: 32 batch lanes, each an fma chain, summed in order
    ref = dict(dx=dx, dw1=dpre1.t() @ s, db1=dpre1.sum(0), dw2=dpre2.t() @ h, db2=dpre2.sum(0))
    bnd = dict(dx=bdx, dw1=e1.t() @ s.abs() + db * U * (dpre1.abs().t() @ s.abs()), db1=e1.sum(0) + db * U * dpre1.abs().sum(0),
               dw2=e.t() @ h + db * U * (dpre2.abs().t() @ h), db2=e.sum(0) + db * U * dpre2.abs().sum(0))
    return ref, bnd


# ------------------------------------------------------------------------------------------ integer patterns
def pattern(shape, lo, hi, seed):
    """integers in [lo, hi] over `shape` (..., C): an index hash that changes with every leading index, the channel quad and the
    channel within the quad; channel 0 is a ramp along the last spatial axis whose phase depends on all the axes before it"""
    n = hi - lo + 1
    idx = torch.meshgrid(*[torch.arange(d, dtype=torch.int64) for d in shape], indexing="ij")
    c = idx[-1]
    v = 3 * (c // 4) + 5 * (c % 4) + seed
    for a, i in enumerate(idx[:-1]):
        v = v + (2 * a + 3) * i + (i * (c // 4 + a + 1)) % 7
    if len(shape) >= 2:
        ramp = idx[-2] + seed
        for a, i in enumerate(idx[:-2]):
            ramp = ramp + (2 * a + 3) * i
        v = torch.where(c == 0, ramp, v)
    return (v % n + lo).double()


def balanced_signs(M, C, seed):
    """(M, C) of +-1, exactly M/2 of each in every column, in a pseudo-random order of the column's own"""
    assert M % 2 == 0
    g = torch.Generator().manual_seed(seed)
    order = torch.rand(M, C, generator=g).argsort(0).argsort(0)
    return torch.where(order < M // 2, 1.0, -1.0).double()


def bn_exact_case(M, C, seed=0, a=2.0, res=False):
    """columns m_c +- a (module docstring): mean, var = a^2, rstd = 1/(2a), scale, shift and y are exact in fp32; the running
    statistics rm = m_c + {-1, 0, 1}, rv = a^2 make eval mode exact as well (rstd = 1/(2a) again, another integer shift)"""
    c = torch.arange(C, dtype=torch.float64)
    m = (c * 7 + seed) % 23 - 11
    gq = (c * 5 + seed) % 7 - 3
    gq = torch.where(gq == 0, 4.0, gq)
    case = dict(x=m + a * balanced_signs(M, C, seed + 1), gamma=2 * a * gq, beta=(c * 3 + seed) % 9 - 4, eps=3 * a * a,
                rm=m + c % 3 - 1, rv=torch.full((C,), a * a, dtype=torch.float64), da=pattern((M, C), -4, 4, seed + 2), a=a, m=m, g=gq)
    if res:
        case["res"] = pattern((M, C), -5, 5, seed + 3)
    return case


def conv1x1_exact_case(M, K, N, seed=0, a=2.0):
    """x (M,K), w (N,K) small integers (exact in bf16 and fp16 too) whose product has BatchNorm-exact columns m_n +- a:
    x[i] = (t_i, 1, z_i, -z_i, ...), w[n] = (a, m_n, q_n, q_n, ...): the pairs cancel only if every product is taken at its own
    (row, k); a wrong k, a wrong row's z or a dropped term leaves an integer behind."""
    assert K >= 4 and K % 2 == 0
    P = (K - 2) // 2
    z = pattern((M, P), -3, 3, seed)
    q = pattern((N, P), -2, 2, seed + 1)
    n = torch.arange(N, dtype=torch.float64)
    m = (n * 7 + seed) % 13 - 6
    x = torch.cat([balanced_signs(M, 1, seed + 2), torch.ones(M, 1, dtype=torch.float64),
                   torch.stack([z, -z], -1).reshape(M, 2 * P)], 1)
    w = torch.cat([torch.full((N, 1), a, dtype=torch.float64), m[:, None], torch.stack([q, q], -1).reshape(N, 2 * P)], 1)
    return x, w


def exactness(stored, sums):
    """stored: tensors the device holds (integers of magnitude < 2^24; halves allowed where stated by the caller through a
    scale); sums: sums of the absolute values of the terms of every fp32 sum, each < 2^24.  Conditions on the inputs: if one
    fails the builder is wrong."""
    for name, t in stored.items():
        assert torch.equal(t, t.round()) and t.abs().max().item() < LIMIT, f"{name}: not an integer below 2^24"
    for name, t in sums.items():
        assert t.abs().max().item() < LIMIT, f"{name}: an fp32 sum may round ({t.abs().max().item():.3g} >= 2^24)"


def bn_exactness(case, M):
    """the exact BatchNorm case's conditions: integer inputs; x^2 and dz sums below 2^24; the exact values are what fp32 holds"""
    x, a = case["x"], case["a"]
    exactness(dict(x=x, da=case["da"], gamma=case["gamma"], beta=case["beta"]),
              dict(sum_x=x.abs().sum(0), sum_x2=(x * x).sum(0), sum_da=case["da"].abs().sum(0)))
    assert torch.equal(x.mean(0), case["m"]) and torch.equal(((x - case["m"]) ** 2).mean(0), torch.full_like(case["m"], a * a))
    assert math.log2(a) == round(math.log2(a)) and 1.0 / math.sqrt(a * a + case["eps"]) == 1 / (2 * a)


# ------------------------------------------------------------------------------------------ the cases and the path each is for
# depthwise (B, H, W, C, k, s): what the plan query must report for (fwd, dx, dw)
DW_CASES = [
    ((65, 2, 3, 1024, 3, 1), dict(nimg=2, groups=33, G_c=16, ragged=True, lds=(1, 1, 1))),
    ((251, 2, 3, 1024, 5, 2), dict(nimg=8, groups=32, G_c=16, ragged=True, last=3, lds=(1, 1, 1))),
    ((131, 2, 5, 576, 5, 1), dict(nimg=2, groups=66, G_c=9, ragged=True, lds=(1, 1, 1))),
    ((67, 3, 3, 1000, 3, 2), dict(nimg=2, groups=34, G_c=16, ragged=True, tail=True, lds=(1, 1, 1))),
    ((13, 8, 16, 512, 3, 1), dict(nimg=1, groups=13, G_c=8, lds=(1, 1, 0))),
    ((2, 33, 32, 1022, 3, 1), dict(lds=(0, 0, 0), V=1, second_trip=True)),
]
DW_RAGGED = [c for c, p in DW_CASES if p.get("ragged")]
# stem (B, Hin, Win, C)
# the kernels take FOUR pixels per trip, at p0 + u * blocks * L: `slots` = how many of a trip's four are live somewhere, `trips` = 2
# where 4 blocks L < P < 8 blocks L, so that some workgroups go round the loop a second time (ragged) and most do not
STEM_CASES = [((36, 37, 101, 64), dict(blocks=512, L=16, trips=2)), ((9, 37, 101, 64), dict(blocks=512, L=16, trips=1, slots=2)),
              ((3, 40, 151, 32), dict(blocks=143, L=32, trips=1, slots=1))]
# BatchNorm (M, C)
BN_CASES = [
    ((1030, 1024), dict(chunks=256, rows_per_chunk=5, R=1, empty_chunks=50)),
    ((2, 8), dict(chunks=1)),
    ((6, 1024), dict(chunks=1, R=1)),
    ((2054, 1022), dict(V=1, second_trip=True)),
    ((8200, 1024), dict(V=4, second_trip=True, bwd_three_launch=True)),
]
# 1x1 conv + BatchNorm (M, K, N): the form of the finishing apply pass, whether the last channel group is short
C1_CASES = [
    ((3050, 24, 72), dict(tiles=48, cap=16, CG4=9, G_c=2, tail=False)),
    ((4130, 24, 64), dict(tiles=65, cap=8, CG4=8, G_c=2, tail=False)),
    ((16500, 24, 64), dict(tiles=129, cap=4, CG4=4, G_c=4, tail=False)),
    ((3050, 24, 136), dict(tiles=48, cap=16, CG4=12, G_c=3, tail=True)),
    ((21900, 24, 72), dict(tiles=172, cap=4, CG4=4, G_c=5, tail=True)),
]
# SE (B, HW, C, Cs): images per workgroup, and whether the last workgroup is short
SE_SHAPES = [(5, 190, 16, 8), (3, 30, 96, 24), (6, 30, 240, 64), (2, 10, 576, 144), (7, 9, 40, 12), (130, 6, 24, 8), (41, 4, 32, 8),
             (129, 10, 576, 144), (34, 3, 1024, 256)]
SE_PLANS = {(130, 6, 24, 8): (4, True), (129, 10, 576, 144): (4, True), (41, 4, 32, 8): (2, True), (34, 3, 1024, 256): (2, False)}


def assert_se_plan(shape):
    from wakeword_trainer_home_amd import _native as nat
    img, ragged = SE_PLANS.get(shape, (1, False))
    p = nat.plan_se(*shape)
    assert p["img"] == img and p["grid"] == -(-shape[0] // img) and (shape[0] % img != 0) == ragged, (shape, p)
    return p
EW_BIG = 2097152 + 1021                # single floats: just past egrid's 8192 workgroups x 256 threads
EW_SCALE = (2, 1024, 1025)             # (B, HW, C) of the same size for the gating kernels, C % 4 != 0, HW a power of two


def dw_case(B, H, W, C, k, s, seed=0):
    """integer inputs and the float64 reference of one depthwise case, its exactness asserted"""
    Ho, Wo = out_hw(H, W, k, s)
    x, dy = pattern((B, H, W, C), -4, 4, seed), pattern((B, Ho, Wo, C), -4, 4, seed + 1)
    w = pattern((k, k, C), -3, 3, seed + 2).permute(2, 0, 1).contiguous()
    y = dw_fwd(x, w, k, s)
    dx, dw = dw_bwd(x, w, dy, k, s)
    _, dw_abs = dw_bwd(x.abs(), w.abs(), dy.abs(), k, s)
    exactness(dict(x=x, w=w, dy=dy, y=y, dx=dx, dw=dw),
              dict(y=dw_fwd(x.abs(), w.abs(), k, s), dx=dw_bwd(x.abs(), w.abs(), dy.abs(), k, s)[0], dw=dw_abs,
                   sum_y=y.abs().sum((0, 1, 2)), sum_y2=(y * y).sum((0, 1, 2))))
    return dict(x=x, w=w, dy=dy, y=y, dx=dx, dw=dw)


def stem_case(B, H, W, C, seed=0):
    Ho, Wo = (H + 1) // 2, (W + 1) // 2
    # (x, w in [-2, 2]: the sum of y^2 over all the pixels of the largest case stays an exact fp32 integer)
    x = pattern((B, H, W, 1), -2, 2, seed)[..., 0].contiguous()
    w = pattern((3, 3, C), -2, 2, seed + 1).permute(2, 0, 1).contiguous()
    dy = pattern((B, Ho, Wo, C), -4, 4, seed + 2)
    y, dw = stem_fwd(x, w), stem_dw(x, dy)
    exactness(dict(x=x, w=w, dy=dy, y=y, dw=dw),
              dict(y=stem_fwd(x.abs(), w.abs()), dw=stem_dw(x.abs(), dy.abs()), sum_y=y.abs().sum((0, 1, 2)), sum_y2=(y * y).sum((0, 1, 2))))
    return dict(x=x, w=w, dy=dy, y=y, dw=dw)


def ulp32(ref):
    """the spacing of fp32 at each float64 value"""
    r = ref.float().abs()
    return (torch.nextafter(r, torch.full_like(r, math.inf)) - r).double()


def worst_ratio(got, ref, bound):
    """max over the elements of |got - ref| / bound (a zero bound demands equality: inf if it is missed)"""
    err = (got - ref).abs()
    ratio = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err > 0, math.inf, 0.0))
    return ratio.max().item()


# ------------------------------------------------------------------------------------------ the path each case is there for
# asserted through the library's host-only plan queries (include/wwhip.h ww_nhwc_plan_*), which run the entry points' own
# dispatch code: whoever retunes a heuristic is told which case stopped reaching its path
def assert_dw_plan(shape, want):
    from wakeword_trainer_home_amd import _native as nat
    B, H, W, C, k, s = shape
    Ho, Wo = out_hw(H, W, k, s)
    plans = {w: nat.plan_dw(w, *shape) for w in ("fwd", "dx", "dw")}
    assert tuple(p["lds"] for p in plans.values()) == want["lds"], (shape, plans)
    for which, p in plans.items():
        if p["lds"]:
            assert (p["nimg"], p["groups"], p["G_c"]) == (want["nimg"], want["groups"], want["G_c"]), (shape, which, p)
            assert p["grid"] == p["groups"] * p["G_c"] and p["V"] == 4
            if want.get("ragged"):
                assert B % p["nimg"] != 0 and B - (p["groups"] - 1) * p["nimg"] == want.get("last", B % p["nimg"]), (shape, which, p)
            if want.get("tail"):
                assert p["G_c"] * p["CC4"] > C // 4, (shape, which, p)
        elif "V" in want:
            assert p["V"] == want["V"], (shape, which, p)
    if want.get("second_trip"):
        V = want["V"]
        assert B * Ho * Wo * (C // V) > plans["fwd"]["grid"] * 256 and B * H * W * (C // V) > plans["dx"]["grid"] * 256, (shape, plans)
    return plans


def assert_stem_plan(shape, want):
    from wakeword_trainer_home_amd import _native as nat
    B, H, W, C = shape
    p = nat.plan_stem(*shape)
    P = B * ((H + 1) // 2) * ((W + 1) // 2)
    assert (p["blocks"], p["L"]) == (want["blocks"], want["L"]), (shape, p)
    stride = p["blocks"] * p["L"]
    if want["trips"] == 2:                  # the loop's back edge: a ragged second trip, in some workgroups only
        assert 4 * stride < P < 5 * stride, (shape, p, P)
    else:                                   # one trip; the last live slot of its four is live in some workgroups only
        assert (want["slots"] - 1) * stride < P <= want["slots"] * stride and (want["slots"] == 1 or P < want["slots"] * stride), (shape, p, P)
    return p


def assert_bn_plan(shape, want):
    from wakeword_trainer_home_amd import _native as nat
    M, C = shape
    f, b = nat.plan_bn("fwd", M, C), nat.plan_bn("bwd", M, C)
    for key in ("chunks", "rows_per_chunk", "R", "V"):
        if key in want:
            assert f[key] == want[key] and (key == "V" or b[key] == want[key]), (shape, key, f, b)
    assert f["fused"] == 0                   # ww_bn_act_fwd: statistics, finish, elementwise apply
    if "empty_chunks" in want:
        assert f["chunks"] - -(-M // f["rows_per_chunk"]) == want["empty_chunks"], (shape, f)
    if f["chunks"] == 1:
        assert M < 4 * f["R"] or M // (4 * f["R"]) == 1, (shape, f)
    if want.get("second_trip"):
        assert M * C // f["V"] > f["grid"] * 256 and f["grid"] == 8192, (shape, f)
    if want.get("bwd_three_launch"):
        assert b["fused"] == 0 and b["V"] == 4 and M * C // 4 > b["grid"] * 256, (shape, b)
    elif C % 4 == 0:
        assert b["fused"] == 1, (shape, b)
    else:
        assert b["fused"] == 0 and b["V"] == 1, (shape, b)
    assert nat.plan_bn("bwd", M, C, training=False)["fused"] == 0
    return f, b


def assert_c1_plan(shape, want, aligned=True):
    from wakeword_trainer_home_amd import _native as nat
    M, K, N = shape
    for mode in MODES.values():
        rt = nat.conv1x1_row_tile(M, K, N, mode or torch.float32)
        assert -(-M // rt) == want["tiles"], (shape, mode, rt)
    p = nat.plan_bn("partials", M, N, chunks=want["tiles"], aligned=aligned)
    if not aligned:                          # finish launch + elementwise apply (+ in-place add of the residual); the query
        assert p["fused"] == 0, (shape, p)   # describes ALL pointers off the grid, so its V is not that of a misaligned residual alone
        return p
    assert p["fused"] == 1 and (p["CG4"], p["G_c"]) == (want["CG4"], want["G_c"]), (shape, p)
    assert want["cap"] // 2 < p["CG4"] <= want["cap"] and (p["G_c"] * p["CG4"] > N // 4) == want["tail"], (shape, p)
    return p
