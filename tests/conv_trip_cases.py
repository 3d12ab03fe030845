"""The layer contracts of the cnn_small conv stack (stem, depthwise 3x3, pointwise 1x1; include/wwhip.h) written out by hand in
float64, forward and backward, and the cases that test_conv_trips_host.py / test_conv_trips_gpu.py run them on.  No device code.

Tensors are channels-last float64 (B,H,W,64), the stem's input (B,Hin,Win); weights have nn.Conv2d's shapes.  ``mtype`` places the
16-bit roundings where oracle/conv_stack.py documents them: every stored tensor (y, g_in), and the pointwise layers' matrix
operands (relu(z) and W forward; dy, W and relu(z) backward).  Depthwise and stem products take fp32 operands.

Integer-exact cases.  Every input is a small integer (scale, A, rstd_in powers of two; where one of them is 1/2 the values it
multiplies are even), so every value the device stores or feeds to the matrix cores is an integer of at most 256 -- exact in
fp32, bf16 and fp16 -- and every sum it forms in fp32 has terms whose absolute values add up to less than 2^24: no operation
rounds, in any order, and the device must return the float64 result bit for bit whatever the number of trips a workgroup makes.
``exactness`` asserts both conditions on the reference; they are conditions on the inputs, the builder is at fault if one fails.
Every sample and every image row carries a pattern of its own (independent draws, and channel 0 is a ramp whose phase depends
on sample and row), so a read across a tile, strip, row or sample boundary cannot cancel."""
import functools

import numpy as np
import torch
import torch.nn.functional as F

from oracle.rounding import mround

C = 64
MOMENTUM = float(np.float32(0.1))        # ww_bn_t holds momentum and eps as floats; the finalize kernel widens them
EPS = float(np.float32(1e-5))
T16 = (torch.bfloat16, torch.float16)

# (B, H, W): see the GPU test's docstring for the path each shape reaches
DW_SHAPES = [(3, 20, 76), (2, 41, 10), (1, 21, 3), (5, 1, 1)]
PW_SHAPES = [(1, 3, 5), (2, 8, 8), (3, 5, 19), (2, 20, 76)]
POOLED_SHAPES = [(7, 3, 5), (3, 8, 8), (2, 20, 76)]
STEM_SHAPES = [(3, 40, 151), (2, 13, 50), (1, 9, 251), (2, 7, 9)]           # (B, Hin, Win)
FULL_SHAPES = {"dw": (432, 2, 76), "pw": (87, 20, 76), "stem": (103, 40, 151)}
FWD_CASES = [("stem", s) for s in STEM_SHAPES] + [("dw", s) for s in DW_SHAPES] + [("pw", s) for s in PW_SHAPES]
BWD_CASES = ([("stem", s, False) for s in STEM_SHAPES] + [("dw", s, False) for s in DW_SHAPES]
             + [("pw", s, False) for s in PW_SHAPES] + [("pw", s, True) for s in POOLED_SHAPES])


def case_id(case):
    kind, (B, H, W) = case[0], case[1]
    return f"{kind}-{B}x{H}x{W}" + ("-pooled" if len(case) > 2 and case[2] else "")


# ------------------------------------------------------------------------------------------ the contracts, float64
def act_in(y_in, ss_in):
    """-> z = fma(y_in, scale, shift), a = relu(z)"""
    z = y_in * ss_in[:C] + ss_in[C:]
    return z, torch.relu(z)


def _pad_hw(t, p=1):
    return F.pad(t, (0, 0, p, p, p, p))


def conv_fwd(kind, a, w, mtype=None):
    """stem: a (B,Hin,Win), 3x3 stride 2 pad 1, one input channel; dw: 3x3 pad 1 per channel; pw: 64 -> 64 per pixel."""
    if kind == "stem":
        B, Hin, Win = a.shape
        Ho, Wo = (Hin + 1) // 2, (Win + 1) // 2
        ap = F.pad(a, (1, 1, 1, 1))
        y = torch.zeros(B, Ho, Wo, C, dtype=torch.float64)
        for kh in range(3):
            for kw in range(3):
                y += ap[:, kh:kh + 2 * Ho - 1:2, kw:kw + 2 * Wo - 1:2, None] * w[:, 0, kh, kw]
        return y
    if kind == "dw":
        B, H, W, _ = a.shape
        ap = _pad_hw(a)
        y = torch.zeros_like(a)
        for kh in range(3):
            for kw in range(3):
                y += ap[:, kh:kh + H, kw:kw + W] * w[:, 0, kh, kw]
        return y
    return mround(a, mtype) @ mround(w.reshape(C, C), mtype).t()


def bn_finalize(y, gamma, beta, rm, rv, momentum=MOMENTUM, eps=EPS):
    """k_bn_fwd_finalize on the STORED y: scale/shift, mean/rstd, the running statistics as nn.BatchNorm2d moves them; with
    each output, ``*_mag`` = the larger term of the difference or sum it is (the scale of its last rounding)."""
    yf = y.reshape(-1, C)
    n = yf.shape[0]
    s1, s2 = yf.sum(0), (yf * yf).sum(0)
    mean = s1 / n
    var = (s2 / n - mean * mean).clamp_min(0.0)
    rstd = 1.0 / torch.sqrt(var + eps)
    scale = gamma * rstd
    unb = var * n / (n - 1) if n > 1 else var
    big = lambda p, q: torch.maximum(p.abs(), q.abs())
    return dict(ss=torch.cat([scale, beta - mean * scale]), ss_mag=torch.cat([scale.abs(), big(beta, mean * scale)]),
                mr=torch.cat([mean, rstd]), mr_mag=torch.cat([mean.abs(), rstd]),
                running_mean=(1.0 - momentum) * rm + momentum * mean, running_mean_mag=big((1.0 - momentum) * rm, momentum * mean),
                running_var=(1.0 - momentum) * rv + momentum * unb, running_var_mag=big((1.0 - momentum) * rv, momentum * unb),
                sum_abs={"sum y": yf.abs().sum(0), "sum y^2": s2})


def layer_fwd(kind, c, mtype=None):
    """c: x | (y_in, ss_in), w, gamma, beta, running_mean, running_var -> a, y (as stored) and bn_finalize's outputs."""
    a = c["x"] if kind == "stem" else act_in(c["y_in"], c["ss_in"])[1]
    y = mround(conv_fwd(kind, a, c["w"], mtype), mtype)
    out = dict(a=a, y=y, **bn_finalize(y, c["gamma"], c["beta"], c["running_mean"], c["running_var"]))
    out["sum_abs"]["conv"] = conv_fwd(kind, a.abs(), c["w"].abs(), mtype)
    return out


def coef_from_sums(s1, s2, n, gamma, mean, rstd):
    """bn_bwd_finalize_group: (A, Bc, Cc) of dy = A dz + Bc y + Cc from s1 = sum dz, s2 = sum dz * yhat over n values per channel
    (tests/test_hip_kernels.py:_coef_from with the sums and the layer's mean / rstd given); and the larger term of each."""
    c1, c2 = s1 / n, s2 / n
    A = gamma * rstd
    coef = torch.cat([A, -A * rstd * c2, A * (mean * rstd * c2 - c1)])
    mag = torch.cat([A.abs(), (A * rstd * c2).abs(), torch.maximum((A * mean * rstd * c2).abs(), (A * c1).abs())])
    return coef, mag


def layer_bwd(kind, c, mtype=None):
    """c: g | (dpool, ss_out), y_out, coef, w and, but for the stem, y_in, ss_in, mr_in, gamma_in; the stem takes x.
    dy = A g + Bc y_out + Cc;  g_in = [z_in > 0] * (transposed product), stored;  dW = sum a * dy;  dbeta_in = sum g_in;
    dgamma_in = sum g_in * yhat_in;  coef_in = coef_from_sums of those.  ``sum_abs``: per output, the sum of the absolute values
    of the terms of every fp32 sum the device forms for it."""
    y_out, w = c["y_out"], c["w"]
    A, Bc, Cc = c["coef"][:C], c["coef"][C:2 * C], c["coef"][2 * C:]
    if c.get("g") is None:                      # the last layer: the pooled gradient through the layer's own ReLU
        dz = c["dpool"][:, None, None, :] * (y_out * c["ss_out"][:C] + c["ss_out"][C:] > 0)
    else:
        dz = c["g"]
    dy = A * dz + Bc * y_out + Cc
    sums = {"dy": (A * dz).abs() + (Bc * y_out).abs() + Cc.abs()}
    if kind == "stem":
        x = c["x"]
        Ho, Wo = dy.shape[1], dy.shape[2]
        xp = F.pad(x, (1, 1, 1, 1))
        dw, dwa = torch.zeros(C, 1, 3, 3, dtype=torch.float64), torch.zeros(C, 1, 3, 3, dtype=torch.float64)
        for kh in range(3):
            for kw in range(3):
                patch = xp[:, kh:kh + 2 * Ho - 1:2, kw:kw + 2 * Wo - 1:2]
                dw[:, 0, kh, kw] = torch.einsum("bhwc,bhw->c", dy, patch)
                dwa[:, 0, kh, kw] = torch.einsum("bhwc,bhw->c", dy.abs(), patch.abs())
        sums["dW"] = dwa
        return dict(dy=dy, dw=dw, sum_abs=sums)
    y_in, mean, rstd = c["y_in"], c["mr_in"][:C], c["mr_in"][C:]
    z_in, a = act_in(y_in, c["ss_in"])
    B, H, W, _ = y_in.shape
    if kind == "dw":
        ap, dyp = _pad_hw(a), _pad_hw(dy)
        da, daa = torch.zeros_like(dy), torch.zeros_like(dy)
        dw, dwa = torch.zeros(C, 1, 3, 3, dtype=torch.float64), torch.zeros(C, 1, 3, 3, dtype=torch.float64)
        for kh in range(3):
            for kw in range(3):
                # y[h][w] takes a[h + kh - 1][w + kw - 1] * w[kh][kw]:  da[h][w] += dy[h - kh + 1][w - kw + 1] * w[kh][kw]
                sh = dyp[:, 2 - kh:2 - kh + H, 2 - kw:2 - kw + W]
                da += sh * w[:, 0, kh, kw]
                daa += sh.abs() * w[:, 0, kh, kw].abs()
                ash = ap[:, kh:kh + H, kw:kw + W]
                dw[:, 0, kh, kw] = (ash * dy).sum(dim=(0, 1, 2))
                dwa[:, 0, kh, kw] = (ash * dy.abs()).sum(dim=(0, 1, 2))
    else:
        dyr, wr, ar = mround(dy, mtype), mround(w.reshape(C, C), mtype), mround(a, mtype)
        da, daa = dyr @ wr, dyr.abs() @ wr.abs()
        dw = (dyr.reshape(-1, C).t() @ ar.reshape(-1, C)).reshape(C, C, 1, 1)
        dwa = (dyr.abs().reshape(-1, C).t() @ ar.reshape(-1, C)).reshape(C, C, 1, 1)
        sums["y_out recomputed"] = ar.abs() @ wr.abs().t()          # k_pw_bwd_bf16 forms y_out again from a and W
    g_in = mround((z_in > 0) * da, mtype)
    yhat = (y_in - mean) * rstd
    gf = g_in.reshape(-1, C)
    s1, s2 = gf.sum(0), (g_in * yhat).reshape(-1, C).sum(0)
    coef_in, coef_mag = coef_from_sums(s1, s2, gf.shape[0], c["gamma_in"], mean, rstd)
    # k_dw_bwd sums g*y and forms rstd * (sum g*y - mean * sum g) once; the pointwise kernels sum g*yhat value by value
    sums.update({"da": daa, "dW": dwa, "sum g_in": gf.abs().sum(0), "sum g_in*yhat": (g_in * yhat).abs().reshape(-1, C).sum(0),
                 "sum g_in*y_in": (g_in * y_in).abs().reshape(-1, C).sum(0) + mean.abs() * gf.abs().sum(0)})
    return dict(dy=dy, a=a, g_in=g_in, dw=dw, dbeta=s1, dgamma=s2, coef_in=coef_in, coef_mag=coef_mag, sum_abs=sums)


def exactness(values, sum_abs):
    """The two conditions of an integer-exact case.  values: name -> every tensor the device stores in the storage type or hands
    to the matrix cores; sum_abs: name -> per output, the sum of |terms| of an fp32 sum.  Raises AssertionError naming the culprit."""
    for name, v in values.items():
        assert torch.equal(v, v.round()), f"{name}: not integers"
        assert v.abs().max().item() <= 256, f"{name}: |value| up to {v.abs().max().item()} > 256"
        for t in T16:
            assert torch.equal(mround(v, t), v), f"{name}: not exact in {t}"
    for name, s in sum_abs.items():
        assert s.max().item() < 2.0 ** 24, f"{name}: sum of |terms| up to {s.max().item():.3g} >= 2^24"


# ------------------------------------------------------------------------------------------ integer-exact inputs
class _Ints:
    def __init__(self, seed):
        self.g = torch.Generator().manual_seed(seed)

    def ints(self, lo, hi, *shape):
        return torch.randint(lo, hi + 1, shape, generator=self.g).double()

    def pow2(self):
        """per channel 1/2, 1 or 2"""
        return 2.0 ** self.ints(-1, 1, C)

    def f32(self, lo, hi):
        """per channel, any fp32 value in [lo, hi)"""
        return (torch.rand(C, generator=self.g, dtype=torch.float64) * (hi - lo) + lo).float().double()

    def image(self, amp, B, H, W, keep=1.0):
        """(B,H,W,64) integers in [-amp, amp], a fraction ``keep`` of them non-zero; channel 0 is the ramp"""
        t = self.ints(-amp, amp, B, H, W, C)
        if keep < 1.0:
            t = t * (torch.rand(B, H, W, C, generator=self.g) < keep)
        m = 2 * amp + 1
        t[..., 0] = ((torch.arange(B)[:, None, None] * 5 + torch.arange(H)[None, :, None] * 3 + torch.arange(W)[None, None, :]) % m - amp).double()
        return t


def _seed(kind, shape, extra=0):
    B, H, W = shape
    return {"stem": 1, "dw": 2, "pw": 3}[kind] * 1000003 + B * 10007 + H * 101 + W + extra


def pw_weight(r):
    """A dense 64 x 64 integer weight does not keep bf16 outputs within 8 significant bits: a four-tap circulant of +-1, four
    entries in every row and every column."""
    w = torch.zeros(C, C, dtype=torch.float64)
    sign = r.ints(0, 1, C, 4) * 2 - 1
    for t, o in enumerate((0, 7, 19, 42)):
        w[torch.arange(C), (torch.arange(C) + o) % C] = sign[:, t]
    return w.reshape(C, C, 1, 1)


def _input_layer(r, B, H, W, small, backward):
    """y_in, ss_in (and mr_in, gamma_in) of the layer in front: where scale or rstd is 1/2, y_in and mean are even.
    ``small``: the narrower ranges (the full-slab shapes; the depthwise layer, whose nine-tap sums grow fastest)"""
    amp = 2 if small else 3
    scale, rstd = r.pow2(), r.pow2()
    even = 1.0 + ((scale < 1) | (rstd < 1)).double()
    y_in = r.image(amp, B, H, W) * even
    c = dict(y_in=y_in, ss_in=torch.cat([scale, r.ints(-1 if small else -2, 1 if small else 2, C)]))
    if backward:
        c.update(mr_in=torch.cat([r.ints(-1, 1, C) * even, rstd]), gamma_in=r.f32(0.5, 1.5))
    return c


def _bn(r):
    return dict(gamma=r.f32(0.5, 1.5), beta=r.f32(-0.5, 0.5), running_mean=r.f32(-0.3, 0.3), running_var=r.f32(0.5, 1.5))


def _weight(kind, r, small):
    if kind == "pw":
        return pw_weight(r)
    lim = 1 if (kind == "dw" or small) else 2
    return r.ints(-lim, lim, C, 1, 3, 3)


def build_fwd(kind, shape, small=False):
    """-> (inputs, reference) of one forward case; ``small``: the narrower value ranges of the full-slab shapes."""
    r = _Ints(_seed(kind, shape))
    B, H, W = shape
    c = (dict(x=r.image(2 if small else 4, B, H, W)[..., 0].contiguous()) if kind == "stem"
         else _input_layer(r, B, H, W, small or kind == "dw", False))
    c.update(w=_weight(kind, r, small), **_bn(r))
    ref = layer_fwd(kind, c)
    vals = {"y": ref["y"], "w": c["w"]}
    if kind != "stem":
        vals.update(y_in=c["y_in"], a=ref["a"])
    exactness(vals, ref["sum_abs"])
    return c, ref


def build_bwd(kind, shape, pooled=False, small=False):
    """-> (inputs, reference) of one backward case.  y_out is the layer's own forward output (the 16-bit pointwise kernel
    recomputes it); coef, mean_in and rstd_in are free inputs of the contract and chosen, not derived."""
    r = _Ints(_seed(kind, shape, 500 if pooled else 77))
    B, H, W = shape
    if kind == "stem":
        c = dict(x=r.image(2 if small else 4, B, H, W)[..., 0].contiguous())
        a = c["x"]
    else:
        c = _input_layer(r, B, H, W, small or kind == "dw", True)
        a = act_in(c["y_in"], c["ss_in"])[1]
    c["w"] = _weight(kind, r, small)
    c["y_out"] = conv_fwd(kind, a, c["w"])
    A = r.pow2()
    even = 1.0 + (A < 1).double()
    c["coef"] = torch.cat([A, r.ints(-1, 1, C), r.ints(-2, 2, C)])
    Bo, Ho, Wo, _ = c["y_out"].shape
    amp = 2 if small else 3
    if pooled:
        so = r.pow2()
        c["ss_out"] = torch.cat([so, r.ints(-2, 2, C)])
        c["dpool"] = r.ints(-amp, amp, B, C) * even
        c["dpool"][:, 0] = (torch.arange(B) % (2 * amp + 1) - amp).double() * even[0]
        c["g"] = None
    else:
        c["g"] = r.image(amp, Bo, Ho, Wo, keep=0.6) * even
    ref = layer_bwd(kind, c)
    vals = {"y_out": c["y_out"], "w": c["w"], "dy": ref["dy"]}
    if kind != "stem":
        vals.update(y_in=c["y_in"], a=ref["a"], g_in=ref["g_in"])
    if not pooled:
        vals["g"] = c["g"]
    exactness(vals, ref["sum_abs"])
    return c, ref


fwd_case = functools.lru_cache(maxsize=None)(build_fwd)          # the small cases: built once, shared, never modified
bwd_case = functools.lru_cache(maxsize=None)(build_bwd)


# ------------------------------------------------------------------------------------------ round-off away from zero mean
ROUNDOFF_CASES = [("dw", (3, 20, 76)), ("dw", (2, 41, 10)), ("pw", (2, 20, 76))]


@functools.lru_cache(maxsize=None)
def roundoff_case(kind, shape, dname):
    """The inputs of tests/test_pw_bwd_tiles.py (unit-normal y_in plus a per-channel offset of up to 3 standard deviations, about
    half of both ReLU masks set) for the layer pair y_in -> bn_in -> relu -> conv -> bn_out -> dL/dz, channels-last float64, with the
    stored tensors rounded to the storage type ``dname``; the expected outputs come from autograd."""
    dt = {"fp32": None, "bf16": torch.bfloat16, "fp16": torch.float16}[dname]
    r16 = lambda t: t.float().double() if dt is None else mround(t, dt)
    B, H, W = shape
    gen = torch.Generator().manual_seed(_seed(kind, shape, 9000))
    offs = (torch.rand(C, generator=gen, dtype=torch.float64) * 2 - 1) * 3
    y_in = r16(torch.randn(B, C, H, W, generator=gen, dtype=torch.float64) + offs[None, :, None, None])
    bn_in, bn_out = torch.nn.BatchNorm2d(C).double(), torch.nn.BatchNorm2d(C).double()
    with torch.no_grad():
        for bn in (bn_in, bn_out):
            bn.weight.copy_((torch.rand(C, generator=gen, dtype=torch.float64) + 0.5).float().double())
            bn.bias.copy_((torch.randn(C, generator=gen, dtype=torch.float64) * 0.3).float().double())
    wshape = (C, 1, 3, 3) if kind == "dw" else (C, C, 1, 1)
    w = (torch.randn(*wshape, generator=gen, dtype=torch.float64) * 0.25).float().double().requires_grad_(True)
    z_in = bn_in(y_in)
    z_in.retain_grad()
    a = torch.relu(z_in)
    if kind == "dw":
        y_raw = F.conv2d(a, w, padding=1, groups=C)
        y_dev = r16(y_raw.detach())
    else:
        y_raw = F.conv2d(a, w)
        y_dev = r16(F.conv2d(mround(a.detach(), dt), mround(w.detach(), dt)))     # as the 16-bit kernel recomputes it
    y = y_raw + (y_dev - y_raw.detach())                   # the gradient passes through the rounding
    z = bn_out(y)
    g = r16(torch.randn(B, C, H, W, generator=gen, dtype=torch.float64) * (torch.rand(B, C, H, W, generator=gen) > 0.5))
    (z * g).sum().backward()
    n = B * H * W
    mean_out, var_out = y_dev.mean(dim=(0, 2, 3)), y_dev.var(dim=(0, 2, 3), unbiased=False)
    rstd_out = 1.0 / torch.sqrt(var_out + 1e-5)
    yhat_out = (y_dev - mean_out[None, :, None, None]) * rstd_out[None, :, None, None]
    coef, _ = coef_from_sums(g.sum(dim=(0, 2, 3)), (g * yhat_out).sum(dim=(0, 2, 3)), n, bn_out.weight.detach(), mean_out, rstd_out)
    mean_in = y_in.mean(dim=(0, 2, 3))
    rstd_in = 1.0 / torch.sqrt(y_in.var(dim=(0, 2, 3), unbiased=False) + 1e-5)
    scale_in = bn_in.weight.detach() * rstd_in
    cl = lambda t: t.detach().permute(0, 2, 3, 1).contiguous()
    f32 = lambda t: t.float().double()                     # the fp32 arguments as the device receives them
    return dict(dt=dt, y_in=cl(y_in), y_out=cl(y_dev), g=cl(g), coef=f32(coef), w=w.detach(), gamma_in=bn_in.weight.detach(),
                ss_in=f32(torch.cat([scale_in, bn_in.bias.detach() - mean_in * scale_in])), mr_in=f32(torch.cat([mean_in, rstd_in])),
                ref_g_in=cl(z_in.grad), ref_dw=w.grad.detach().clone())


def dw_geometry(H, W):
    """ww_dwconv3x3_*: an item is a strip of 4 columns and one of nseg row segments of hs_len <= 20 rows -> (ncs, nseg, hs_len)"""
    nseg = (H + 19) // 20
    return (W + 3) // 4, nseg, (H + nseg - 1) // nseg


def values_per_thread(kind, shape, cap):
    """How many values one thread of the backward kernel adds in sequence into its BatchNorm sums when the launch has ``cap``
    workgroups (0: as many as the work asks for -- for these shapes one residency round of the device is more than that).
    k_dw_bwd: 8 item slots per workgroup, an item is 4 columns x hs_len rows of one channel pair per lane, then the 8 slots are
    added and rstd * (s2 - mean * s1) is formed (+ 8 + 2).  k_pw_bwd / k_pw_bwd_bf16: 16 pixels of a 64-pixel tile per lane, then
    the other half-wave and the other wave (+ 2)."""
    B, H, W = shape
    if kind == "dw":
        ncs, nseg, hs_len = dw_geometry(H, W)
        items = B * nseg * ncs
        grid = min((items + 7) // 8, cap) if cap else (items + 7) // 8
        return -(-items // (8 * grid)) * 4 * hs_len + 10
    tiles = (B * H * W + 63) // 64
    grid = min(tiles, cap) if cap else tiles
    return -(-tiles // grid) * 16 + 2
