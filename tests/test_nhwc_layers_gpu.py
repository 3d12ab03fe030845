"""The channels-last layer library (csrc/ww_nhwc.hip, ww_se.hip) per launch path, on exact data: every case of
tests/nhwc_cases.py states the path it is there for and asserts it through the library's plan queries before it runs.

Integer-exact cases come back bit for bit; round-off cases are held to the per-element bounds derived in tests/nhwc_cases.py
(K * 2^-24 * sum|terms|), and each prints its worst observed  err / bound  and, where the bound is one K, the worst
err / (2^-24 S) beside that K  (profiles/r14_nhwc_layers_measured.txt keeps them; the assertions are the derived bounds, never the
measurements).  The C entry points are driven directly, so that every output sits
NaN-poisoned inside a larger NaN-filled buffer: every element must come back written and nothing around the tensor may be."""
import ctypes
import functools
import math

import pytest
import torch

from tests import nhwc_cases as K

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
# floats on either side of an output (a multiple of 4: the tensor keeps its 16-byte alignment).  Wide enough for the images a
# depthwise kernel would write past the batch if it took a short last group for a full one (5 images x 6 pixels x 1024 channels in
# the largest case): such a kernel is caught by the guard, inside memory the test owns
GUARD = 32768
ident = lambda c: "-".join(map(str, c[0]))


def dev(t):
    return t.float().to(DEV).contiguous()


def back(t):
    return t.detach().cpu().double()


class Out:
    """an fp32 output tensor poisoned with NaN inside a NaN-filled buffer"""

    def __init__(self, *shape):
        n = math.prod(shape)
        self.buf = torch.full((n + 2 * GUARD,), math.nan, dtype=torch.float32, device=DEV)
        self.t = self.buf[GUARD:GUARD + n].view(shape)
        assert self.t.data_ptr() % 16 == 0

    def read(self, what):
        n = self.t.numel()
        assert self.buf[:GUARD].isnan().all() and self.buf[GUARD + n:].isnan().all(), f"{what}: written outside the tensor"
        assert not self.t.isnan().any(), f"{what}: elements left unwritten"
        return back(self.t)


def call(name, *args):
    """a C entry point on the current stream; tensors go as pointers"""
    from wakeword_trainer_home_amd import _native as nat
    conv = lambda a: a.t.data_ptr() if isinstance(a, Out) else a.data_ptr() if isinstance(a, torch.Tensor) else a
    nat._check(getattr(nat.load(), name)(nat.ctx(DEV), *map(conv, args), torch.cuda.current_stream().cuda_stream), name)


def make_bn(gamma, beta, rm, rv, eps, training):
    """-> (ww_bn_t, the device tensors it points to: gamma, beta, running mean, running var)"""
    from wakeword_trainer_home_amd import _native as nat
    keep = [dev(gamma), dev(beta), dev(rm), dev(rv)]
    return nat.make_bn(*keep, momentum=K.MOMENTUM, eps=eps, training=training), keep


def scratch(C):
    from wakeword_trainer_home_amd import _native as nat
    return nat.nhwc_scratch(C, torch.device(DEV))


def misaligned(t):
    """a contiguous device copy of ``t`` that starts one float into a larger buffer: 4-byte aligned, never 16-byte aligned"""
    buf = torch.empty(t.numel() + 1, dtype=torch.float32, device=DEV)
    v = buf[1:].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4
    return v


def held(name, got, ref, bound, S=None):
    """assert |got - ref| <= bound element by element; print the worst error / bound and, where the bound is K u S with S the
    sum of the absolute values of the element's terms, the worst error / (u S) -- the measured K beside the derived one"""
    ratio = K.worst_ratio(got, ref, bound)
    k = "" if S is None else f" err/(uS) {K.worst_ratio(got, ref, K.U * S):.3f} of {(bound / (K.U * S).clamp_min(1e-300)).max().item():.1f}"
    print(f"nhwc-ratio {name} {ratio:.3f}{k}")
    assert ratio <= 1.0, f"{name}: {ratio:.3f} x its bound"
    return ratio


def one_ulp(name, got, ref, slack=0.0):
    """got is the fp32 cast of a float64 value that equals ref up to float64 round-off (slack): within ONE fp32 spacing of ref"""
    return held(name, got, ref, K.ulp32(ref) + slack)


def check_bn_outputs(name, y, ref, bnd, a, ss, mr, keep, C):
    """the BatchNorm outputs of a producer + BatchNorm call on an EXACT integer y.  Both sums are exact, so the mean is bit for
    bit (one division) and the variance is exact up to float64 round-off: rstd, scale and shift, each ONE cast of a float64
    value, come back within one fp32 spacing; the activation and the running statistics by their bounds."""
    M = y.shape[0]
    s, q = y.sum(0), (y * y).sum(0)
    assert q.max().item() < 2.0 ** 53
    mean = s / M
    assert torch.equal(mr[:C], K.f32(mean)), f"{name}: mean"
    rstd = 1.0 / torch.sqrt(q / M - mean * mean + K.r32(K.EPS))          # the kernel's own one-pass form, in float64
    assert (rstd - ref["mr"][C:]).abs().max().item() <= 1e-9 * rstd.max().item()
    scale = ref["ss"][:C]
    one_ulp(f"{name} rstd", mr[C:], rstd)
    one_ulp(f"{name} scale", ss[:C], scale)
    one_ulp(f"{name} shift", ss[C:], ref["ss"][C:], 1e-12 * (1 + (mean * scale).abs()))
    held(f"{name} a", a, ref["y"], bnd["y"], bnd["S"])
    held(f"{name} running_mean", back(keep[2]), ref["rm"], bnd["rm"])
    held(f"{name} running_var", back(keep[3]), ref["rv"], bnd["rv"])


# ------------------------------------------------------------------------------------------ depthwise
@pytest.mark.parametrize("case", K.DW_CASES, ids=ident)
def test_depthwise_integer_exact(case):
    shape, want = case
    B, H, W, C, k, s = shape
    K.assert_dw_plan(shape, want)
    c = K.dw_case(*shape)
    Ho, Wo = K.out_hw(H, W, k, s)
    x, w, dy = dev(c["x"]), dev(c["w"]), dev(c["dy"])
    y = Out(B, Ho, Wo, C)
    call("ww_dwconv_nhwc_fwd", x, w, B, H, W, C, k, s, y)
    assert torch.equal(y.read("y"), c["y"])
    dx, dw = Out(B, H, W, C), Out(C, k, k)
    call("ww_dwconv_nhwc_bwd", x, w, dy, B, H, W, C, k, s, dx, dw, scratch(C))
    assert torch.equal(dx.read("dx"), c["dx"])
    assert torch.equal(dw.read("dw"), c["dw"])


@pytest.mark.parametrize("shape", K.DW_RAGGED, ids=lambda c: "-".join(map(str, c)))
def test_depthwise_batchnorm_statistics_of_a_short_image_group(shape):
    """ww_dwconv_bn_act_fwd where the last image group is short: its statistics partial must give the exact mean and variance"""
    from wakeword_trainer_home_amd import _native as nat
    B, H, W, C, k, s = shape
    p = nat.plan_dw("fwd", *shape)
    assert p["lds"] == 1 and B % p["nimg"] != 0
    c = K.dw_case(*shape)
    Ho, Wo = K.out_hw(H, W, k, s)
    M, kind = B * Ho * Wo, 1 if k == 5 else 2
    assert nat.plan_bn("partials", M, C, chunks=p["groups"])["fused"] == 1
    g = torch.Generator().manual_seed(C)
    gamma, beta = torch.rand(C, generator=g, dtype=torch.float64) + 0.5, torch.randn(C, generator=g, dtype=torch.float64) * 0.3
    gamma, beta = K.f32(gamma), K.f32(beta)
    rm, rv = torch.zeros(C, dtype=torch.float64), torch.ones(C, dtype=torch.float64)
    bn, keep = make_bn(gamma, beta, rm, rv, K.EPS, True)
    y, a, ss, mr = Out(B, Ho, Wo, C), Out(B, Ho, Wo, C), Out(2 * C), Out(2 * C)
    call("ww_dwconv_bn_act_fwd", dev(c["x"]), dev(c["w"]), B, H, W, C, k, s, ctypes.byref(bn), kind, y, a, ss, mr, scratch(C))
    assert torch.equal(y.read("y"), c["y"])
    y2 = c["y"].reshape(M, C)
    ref = K.bn_fwd(y2, gamma, beta, rm, rv, kind)
    # the LDS kernel's threads add their own outputs in fp32 first: exact on integers, and a depth the bound must not rely on
    bnd = K.bn_fwd_bounds(y2, ref, gamma, beta, kind, D=1)
    check_bn_outputs(f"dwbn {shape}", y2, ref, bnd, a.read("a").reshape(M, C), ss.read("ss"), mr.read("mr"), keep, C)


# ------------------------------------------------------------------------------------------ stem
@pytest.mark.parametrize("case", K.STEM_CASES, ids=ident)
def test_stem_integer_exact(case):
    shape, want = case
    B, H, W, C = shape
    plan = K.assert_stem_plan(shape, want)
    c = K.stem_case(*shape)
    Ho, Wo = (H + 1) // 2, (W + 1) // 2
    M, kind = B * Ho * Wo, 1
    g = torch.Generator().manual_seed(C)
    gamma, beta = K.f32(torch.rand(C, generator=g, dtype=torch.float64) + 0.5), K.f32(torch.randn(C, generator=g, dtype=torch.float64) * 0.3)
    rm, rv = torch.zeros(C, dtype=torch.float64), torch.ones(C, dtype=torch.float64)
    bn, keep = make_bn(gamma, beta, rm, rv, K.EPS, True)
    x, w, dy = dev(c["x"]), dev(c["w"]), dev(c["dy"])
    y, a, ss, mr = Out(B, Ho, Wo, C), Out(B, Ho, Wo, C), Out(2 * C), Out(2 * C)
    call("ww_stem3x3s2_bn_act_fwd", x, w, B, H, W, C, ctypes.byref(bn), kind, y, a, ss, mr, scratch(C))
    assert torch.equal(y.read("y"), c["y"])
    y2 = c["y"].reshape(M, C)
    ref = K.bn_fwd(y2, gamma, beta, rm, rv, kind)
    bnd = K.bn_fwd_bounds(y2, ref, gamma, beta, kind, D=1)
    check_bn_outputs(f"stem {shape}", y2, ref, bnd, a.read("a").reshape(M, C), ss.read("ss"), mr.read("mr"), keep, C)
    dw = Out(C, 3, 3)
    call("ww_stem3x3s2_bwd_dw", x, dy, B, H, W, C, dw, scratch(C))
    assert torch.equal(dw.read("dw"), c["dw"])
    assert plan["blocks"] >= 1


# ------------------------------------------------------------------------------------------ BatchNorm (+activation)
@functools.lru_cache(maxsize=2)
def _bn_exact(M, C):
    c = K.bn_exact_case(M, C)
    K.bn_exactness(c, M)
    return c, dev(c["x"]), dev(c["da"])


@functools.lru_cache(maxsize=2)
def _bn_random(M, C):
    g = torch.Generator().manual_seed(M + C)
    f = lambda t: K.f32(t)
    c = dict(x=f(torch.randn(M, C, generator=g, dtype=torch.float64) * 2 + 1), gamma=f(torch.rand(C, generator=g, dtype=torch.float64) + 0.5),
             beta=f(torch.randn(C, generator=g, dtype=torch.float64) * 0.3), rm=f(torch.randn(C, generator=g, dtype=torch.float64) * 0.1),
             rv=f(torch.rand(C, generator=g, dtype=torch.float64) + 0.5), da=f(torch.randn(M, C, generator=g, dtype=torch.float64)))
    return c, dev(c["x"]), dev(c["da"])


def _bn_run(c, xd, dad, M, C, kind, training, eps, ss_mr=None):
    """ww_bn_act_fwd, then ww_bn_act_bwd from the forward's own ss / mr or from the given ones"""
    bn, keep = make_bn(c["gamma"], c["beta"], c["rm"], c["rv"], eps, training)
    y, ss, mr = Out(M, C), Out(2 * C), Out(2 * C)
    call("ww_bn_act_fwd", xd, M, C, ctypes.byref(bn), kind, y, ss, mr, scratch(C))
    fwd = dict(y=y.read("y"), ss=ss.read("ss"), mr=mr.read("mr"), rm=back(keep[2]), rv=back(keep[3]))
    ssd, mrd = (ss.t, mr.t) if ss_mr is None else (dev(ss_mr[0]), dev(ss_mr[1]))
    dx, dg, db = Out(M, C), Out(C), Out(C)
    call("ww_bn_act_bwd", xd, dad, M, C, ssd, mrd, kind, int(training), dx, dg, db, scratch(C))
    return fwd, dict(dx=dx.read("dx"), dgamma=dg.read("dgamma"), dbeta=db.read("dbeta"))


@pytest.mark.parametrize("training", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("kind", [0, 1, 2, 3])
@pytest.mark.parametrize("case", K.BN_CASES, ids=ident)
def test_batchnorm_integer_exact(case, kind, training):
    (M, C), want = case
    K.assert_bn_plan((M, C), want)
    c, xd, dad = _bn_exact(M, C)
    ref = K.bn_fwd(c["x"], c["gamma"], c["beta"], c["rm"], c["rv"], kind, training, eps=c["eps"])
    fwd, bwd = _bn_run(c, xd, dad, M, C, kind, training, c["eps"])
    assert torch.equal(fwd["mr"], ref["mr"]) and torch.equal(fwd["ss"], ref["ss"])
    assert torch.equal(fwd["y"], K.act32(kind, ref["z"]))                       # z is an integer: lin_act's own fp32 operations
    tag = f"bn-exact {M}x{C} act{kind} {'train' if training else 'eval'}"
    one_ulp(f"{tag} running_mean", fwd["rm"], ref["rm"])
    one_ulp(f"{tag} running_var", fwd["rv"], ref["rv"])
    want_b, bnd, Sb = K.bn_bwd(c["x"], c["da"], ref["ss"], ref["mr"], kind, training)
    if kind in (0, 2):                                                          # integer dz, xhat = +-1/2 (eval: quarters)
        assert torch.equal(bwd["dgamma"], want_b["dgamma"]) and torch.equal(bwd["dbeta"], want_b["dbeta"])
    else:
        held(f"{tag} dgamma", bwd["dgamma"], want_b["dgamma"], bnd["dgamma"], Sb["dgamma"])
        held(f"{tag} dbeta", bwd["dbeta"], want_b["dbeta"], bnd["dbeta"], Sb["dbeta"])
    held(f"{tag} dx", bwd["dx"], want_b["dx"], bnd["dx"], Sb["dx"])


@pytest.mark.parametrize("training", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("kind", [0, 1, 2, 3])
@pytest.mark.parametrize("case", K.BN_CASES, ids=ident)
def test_batchnorm_round_off(case, kind, training):
    (M, C), want = case
    K.assert_bn_plan((M, C), want)
    c, xd, dad = _bn_random(M, C)
    ref = K.bn_fwd(c["x"], c["gamma"], c["beta"], c["rm"], c["rv"], kind, training)
    bnd = K.bn_fwd_bounds(c["x"], ref, c["gamma"], c["beta"], kind, training)
    ss_mr = (K.f32(ref["ss"]), K.f32(ref["mr"]))        # the backward from the reference's statistics: a function of its inputs
    fwd, bwd = _bn_run(c, xd, dad, M, C, kind, training, K.EPS, ss_mr)
    tag = f"bn {M}x{C} act{kind} {'train' if training else 'eval'}"
    held(f"{tag} y", fwd["y"], ref["y"], bnd["y"], bnd["S"] if kind != 3 else None)
    held(f"{tag} mean", fwd["mr"][:C], ref["mr"][:C], bnd["mean"])
    held(f"{tag} rstd", fwd["mr"][C:], ref["mr"][C:], bnd["rstd"])
    held(f"{tag} scale", fwd["ss"][:C], ref["ss"][:C], bnd["scale"])
    held(f"{tag} shift", fwd["ss"][C:], ref["ss"][C:], bnd["shift"])
    if training:
        held(f"{tag} running_mean", fwd["rm"], ref["rm"], bnd["rm"])
        held(f"{tag} running_var", fwd["rv"], ref["rv"], bnd["rv"])
    else:
        assert torch.equal(fwd["rm"], c["rm"]) and torch.equal(fwd["rv"], c["rv"])
    want_b, bb, Sb = K.bn_bwd(c["x"], c["da"], *ss_mr, kind, training)
    for name in ("dx", "dgamma", "dbeta"):
        held(f"{tag} {name}", bwd[name], want_b[name], bb[name], Sb[name])


@pytest.mark.parametrize("ratio", [8, 32, 128])
@pytest.mark.parametrize("M", [4096, 1030])
def test_batchnorm_off_centre_statistics(ratio, M):
    """Columns with mean / std = 8, 32, 128.  A workgroup's sums are fp64 but leave as fp32 partials and the variance is
    q/M - mean^2: one rounding each of sum x and sum x^2 per chunk bounds the relative variance error by
    3 * 2^-24 * (1 + (mean/std)^2) (tests/nhwc_cases.py; read back through the fp32 rstd, which adds its own cast: 2u (var + eps)).
    y is held with that error propagated.  Over the bound = an accumulation narrower than the header says."""
    from wakeword_trainer_home_amd import _native as nat
    C = 64
    plan = nat.plan_bn("fwd", M, C)         # k_colstats over several chunks of 16 row lanes: 64 chunks of 64 rows / 16 of 65
    assert (plan["R"], plan["chunks"], plan["rows_per_chunk"], plan["V"]) == (16, M // 64, -(-M // (M // 64)), 4), plan
    g = torch.Generator().manual_seed(ratio + M)
    x = K.f32(torch.randn(M, C, generator=g, dtype=torch.float64) + ratio)
    gamma, beta = K.f32(torch.rand(C, generator=g, dtype=torch.float64) + 0.5), K.f32(torch.randn(C, generator=g, dtype=torch.float64) * 0.3)
    rm, rv = torch.zeros(C, dtype=torch.float64), torch.ones(C, dtype=torch.float64)
    bn, keep = make_bn(gamma, beta, rm, rv, K.EPS, True)
    y, ss, mr = Out(M, C), Out(2 * C), Out(2 * C)
    call("ww_bn_act_fwd", dev(x), M, C, ctypes.byref(bn), 0, y, ss, mr, scratch(C))
    ref = K.bn_fwd(x, gamma, beta, rm, rv, 0)
    bnd = K.bn_fwd_bounds(x, ref, gamma, beta, 0)
    eps = K.r32(K.EPS)
    var_dev = 1.0 / mr.read("mr")[C:] ** 2 - eps
    m2 = (x * x).mean(0)
    err = (var_dev - ref["var"]).abs()
    err32 = (x.float().var(0, unbiased=False).double() - ref["var"]).abs()
    print(f"nhwc-offcentre mean/std={ratio} M={M}: relative variance error device {(err / ref['var']).max().item():.2e} "
          f"float32 CPU torch {(err32 / ref['var']).max().item():.2e} bound {(3 * K.U * m2 / ref['var']).max().item():.2e}")
    assert (err <= 3 * K.U * m2 + 2 * K.U * (ref["var"] + eps)).all()
    held(f"offcentre {ratio} M={M} y", y.read("y"), ref["y"], bnd["y"], bnd["S"])
    held(f"offcentre {ratio} M={M} mean", mr.read("mr")[:C], ref["mr"][:C], bnd["mean"])


# ------------------------------------------------------------------------------------------ 1x1 conv + BatchNorm + activation
def _conv1x1(mode, x, w, bn, kind, res, M, Kd, N):
    from wakeword_trainer_home_amd import _native as nat
    y, a, ss, mr = Out(M, N), Out(M, N), Out(2 * N), Out(2 * N)
    sc = scratch(N)
    assert sc.numel() >= ((M + 63) // 64) * 2 * N
    call("ww_conv1x1_bn_act_fwd", nat.act_code(K.MODES[mode] or torch.float32), x, w, M, Kd, N, ctypes.byref(bn), kind, res, y, a, ss, mr,
         sc, sc.numel() * 4)
    return y.read("y"), a.read("a"), ss.read("ss"), mr.read("mr")


@pytest.mark.parametrize("mode", list(K.MODES))
@pytest.mark.parametrize("case", K.C1_CASES, ids=ident)
def test_conv1x1_batchnorm_integer_exact(case, mode):
    """the finishing apply pass at CG4 <= 16 / 8 / 4, with and without a short last channel group, with a residual on and off
    the 16-byte grid (off it: finish launch + apply + in-place add): everything bit for bit, in the three matrix modes"""
    (M, Kd, N), want = case
    K.assert_c1_plan((M, Kd, N), want)
    K.assert_c1_plan((M, Kd, N), want, aligned=False)
    a0 = 2.0
    x, w = K.conv1x1_exact_case(M, Kd, N, a=a0)
    n = torch.arange(N, dtype=torch.float64)
    gq = torch.where((n * 5) % 7 - 3 == 0, 4.0, (n * 5) % 7 - 3)
    gamma, beta = 2 * a0 * gq, (n * 3) % 9 - 4
    rm, rv = (n % 5 - 2).double(), (n % 3 + 1).double()
    res = K.pattern((M, N), -5, 5, 3)
    y_ref = K.conv1x1(x, w, mode)[0]
    xd, wd = dev(x), dev(w)
    residuals = (("", None), (" res", dev(res)), (" res-misaligned", misaligned(dev(res))))
    for kind in (0, 1, 2, 3):
        ref = K.bn_fwd(y_ref, gamma, beta, rm, rv, kind, eps=3 * a0 * a0)
        for rtag, resd in residuals:
            bn, keep = make_bn(gamma, beta, rm, rv, 3 * a0 * a0, True)
            y, a, ss, mr = _conv1x1(mode, xd, wd, bn, kind, resd, M, Kd, N)
            tag = f"c1-exact {M}x{N} {mode} act{kind}{rtag}"
            assert torch.equal(y, y_ref), tag
            assert torch.equal(mr, ref["mr"]) and torch.equal(ss, ref["ss"]), tag
            a_ref = K.act32(kind, ref["z"])                     # z is an integer: lin_act's own fp32 operations, then ONE fp32 add
            assert torch.equal(a, a_ref if resd is None else K.f32(a_ref + res)), tag
            one_ulp(f"{tag} running_mean", back(keep[2]), ref["rm"])
            one_ulp(f"{tag} running_var", back(keep[3]), ref["rv"])
    # and a plain integer product, every row and column with a pattern of its own
    xr, wr = K.pattern((M, Kd), -4, 4, 1), K.pattern((N, Kd), -3, 3, 2)
    bn, keep = make_bn(gamma, beta, rm, rv, K.EPS, True)
    y, *_ = _conv1x1(mode, dev(xr), dev(wr), bn, 0, None, M, Kd, N)
    assert torch.equal(y, K.conv1x1(xr, wr, mode)[0])


@pytest.mark.parametrize("mode", list(K.MODES))
@pytest.mark.parametrize("case", K.C1_CASES, ids=ident)
def test_conv1x1_batchnorm_round_off(case, mode):
    """N(0,1) operands: y against the product of the operands rounded to the mode's type (depth K + 1), then the BatchNorm
    outputs against float64 BatchNorm of the DEVICE's y, whose statistics partials the GEMM epilogue sums in fp32: a thread adds
    16 values per 64 rows of the tile, a shuffle and an LDS step follow -- depth D = rows / 4 + 3"""
    from wakeword_trainer_home_amd import _native as nat
    (M, Kd, N), want = case
    K.assert_c1_plan((M, Kd, N), want)
    g = torch.Generator().manual_seed(M + N)
    x = K.f32(torch.randn(M, Kd, generator=g, dtype=torch.float64))
    w = K.f32(torch.randn(N, Kd, generator=g, dtype=torch.float64) * 0.3)
    gamma, beta = K.f32(torch.rand(N, generator=g, dtype=torch.float64) + 0.5), K.f32(torch.randn(N, generator=g, dtype=torch.float64) * 0.3)
    rm, rv = K.f32(torch.randn(N, generator=g, dtype=torch.float64) * 0.1), K.f32(torch.rand(N, generator=g, dtype=torch.float64) + 0.5)
    bn, keep = make_bn(gamma, beta, rm, rv, K.EPS, True)
    y, a, ss, mr = _conv1x1(mode, dev(x), dev(w), bn, 1, None, M, Kd, N)
    y_ref, S = K.conv1x1(x, w, mode)
    tag = f"c1 {M}x{Kd}x{N} {mode}"
    held(f"{tag} y", y, y_ref, (Kd + 1) * K.U * S, S)
    D = nat.conv1x1_row_tile(M, Kd, N, K.MODES[mode] or torch.float32) // 4 + 3
    ref = K.bn_fwd(y, gamma, beta, rm, rv, 1)
    bnd = K.bn_fwd_bounds(y, ref, gamma, beta, 1, D=D)
    held(f"{tag} a", a, ref["y"], bnd["y"], bnd["S"])
    held(f"{tag} mean", mr[:N], ref["mr"][:N], bnd["mean"])
    held(f"{tag} rstd", mr[N:], ref["mr"][N:], bnd["rstd"])
    held(f"{tag} scale", ss[:N], ref["ss"][:N], bnd["scale"])
    held(f"{tag} shift", ss[N:], ref["ss"][N:], bnd["shift"])
    held(f"{tag} running_mean", back(keep[2]), ref["rm"], bnd["rm"])
    held(f"{tag} running_var", back(keep[3]), ref["rv"], bnd["rv"])


# ------------------------------------------------------------------------------------------ squeeze-excitation and its pieces
@pytest.mark.parametrize("B,HW,C,Cs", K.SE_SHAPES)
def test_se_block_per_element(B, HW, C, Cs):
    """ww_se_fwd / ww_se_bwd, every stage against float64 from the device's own inputs of that stage, element by element"""
    from wakeword_trainer_home_amd import _native as nat
    K.assert_se_plan((B, HW, C, Cs))
    g = torch.Generator().manual_seed(B + C)
    rn = lambda *s: K.f32(torch.randn(*s, generator=g, dtype=torch.float64))
    x, w1, b1, w2, b2, dy = rn(B, HW, C), K.f32(rn(Cs, C) * 0.3), K.f32(rn(Cs) * 0.2), K.f32(rn(C, Cs) * 0.5), K.f32(rn(C) * 0.5), rn(B, HW, C)
    xd, w1d, b1d, w2d, b2d = dev(x), dev(w1), dev(b1), dev(w2), dev(b2)
    y, s, pre1, pre2 = Out(B, HW, C), Out(B, C), Out(B, Cs), Out(B, C)
    call("ww_se_fwd", xd, B, HW, C, Cs, w1d, b1d, w2d, b2d, y, s, pre1, pre2)
    got = dict(y=y.read("y"), s=s.read("s"), pre1=pre1.read("pre1"), pre2=pre2.read("pre2"))
    tag = f"se {B}x{HW}x{C}x{Cs}"
    for name, (ref, bound) in K.se_fwd_stage_bounds(x, w1, b1, w2, b2, got["s"], got["pre1"], got["pre2"]).items():
        held(f"{tag} {name}", got[name], ref, bound)
    dx, dw1, db1, dw2, db2 = nat.se_bwd(xd, dev(dy), s.t, pre1.t, pre2.t, w1d, w2d)
    ref, bnd = K.se_bwd(x, dy, got["s"], got["pre1"], got["pre2"], w1, w2)
    for name, t in (("dx", dx), ("dw1", dw1), ("db1", db1), ("dw2", dw2), ("db2", db2)):
        held(f"{tag} {name}", back(t), ref[name], bnd[name])


def test_se_pieces_integer_exact():
    """pool (HW a power of two), scale_bc and its gate gradient, scale_pool_bwd and add on integers: bit for bit, in the float4
    and in the one-float form"""
    from wakeword_trainer_home_amd import _native as nat
    for B, HW, C in ((6, 64, 72), (3, 16, 10)):
        x, dy = K.pattern((B, HW, C), -4, 4, 1), K.pattern((B, HW, C), -4, 4, 2)
        gate, dpool = K.pattern((B, C), -3, 3, 3), K.pattern((B, C), -4, 4, 4) * HW
        xd, dyd, gd, dpd = dev(x), dev(dy), dev(gate), dev(dpool)
        assert torch.equal(back(nat.pool_hw_fwd(xd)), x.mean(1))
        y = Out(B, HW, C)
        call("ww_scale_bc_fwd", xd, gd, B, HW, C, y)
        assert torch.equal(y.read("scale_bc"), x * gate[:, None, :])
        assert torch.equal(back(nat.scale_bc_bwd_gate(xd, dyd)), (x * dy).sum(1))
        dx = Out(B, HW, C)
        call("ww_scale_pool_bwd", dyd, gd, dpd, B, HW, C, dx)
        assert torch.equal(dx.read("scale_pool_bwd"), dy * gate[:, None, :] + dpool[:, None, :] / HW)
        o = Out(B, HW, C)
        call("ww_add_f32", xd, dyd, B * HW * C, o)
        assert torch.equal(o.read("add"), x + dy)


def test_elementwise_second_trip_in_the_one_float_form():
    """k_add, k_scale_fwd, k_scale_pool_bwd and k_im2col3x3s2 at just over 8192 workgroups x 256 threads of single floats"""
    from wakeword_trainer_home_amd import _native as nat
    n = K.EW_BIG
    assert nat.plan_ew(n, 4) == dict(grid=8192, V=1) and n > 8192 * 256
    a, b = K.pattern((n // 7 + 1, 7), -9, 9, 1).reshape(-1)[:n], K.pattern((n // 5 + 1, 5), -9, 9, 2).reshape(-1)[:n]
    o = Out(n)
    call("ww_add_f32", dev(a), dev(b), n, o)
    assert torch.equal(o.read("add"), a + b)
    B, HW, C = K.EW_SCALE
    assert nat.plan_ew(B * HW * C, C) == dict(grid=8192, V=1) and B * HW * C > 8192 * 256
    x, gate, dpool = K.pattern((B, HW, C), -4, 4, 3), K.pattern((B, C), -3, 3, 4), K.pattern((B, C), -4, 4, 6) * HW
    xd, gd = dev(x), dev(gate)
    y = Out(B, HW, C)
    call("ww_scale_bc_fwd", xd, gd, B, HW, C, y)
    assert torch.equal(y.read("scale_bc"), x * gate[:, None, :])
    dx = Out(B, HW, C)                                             # (x stands in for dy; HW is a power of two: dpool / HW is exact)
    call("ww_scale_pool_bwd", xd, gd, dev(dpool), B, HW, C, dx)
    assert torch.equal(dx.read("scale_pool_bwd"), x * gate[:, None, :] + dpool[:, None, :] / HW)
    Bi, H, W = 64, 121, 121
    P = Bi * 61 * 61
    assert nat.plan_ew(P * 9, 1, aligned=False) == dict(grid=8192, V=1) and P * 9 > 8192 * 256
    img = K.pattern((Bi, H, W, 1), -4, 4, 5)[..., 0].contiguous()
    cols = Out(P, 9)
    call("ww_im2col3x3s2", dev(img), Bi, H, W, cols)
    assert torch.equal(cols.read("im2col"), K.im2col3x3s2(img))
