"""GPU: the persistent loops of the cnn_small conv stack beyond one trip per workgroup.

Every kernel of the stack walks ``item += gridDim.x`` and carries state from one trip to the next: k_pw_bwd_bf16 issues a tile
one trip ahead, alternates two y_in tiles, carries the pooled gradients of the next tile's images, walks with a signed stride and
has a body of its own for the ragged tile; k_stem_fwd / k_stem_bwd / k_pw_fwd / k_pw_fwd_bf16 fetch the next item under the
current one (the stem stages inputs wider than 202 / 168 columns in place); k_dw_fwd / k_dw_bwd keep BatchNorm sums and nine tap
gradients in registers, and every kernel's dW and statistics accumulate over all trips.  At the layer shapes of the other test
files every workgroup makes exactly one trip.  ``ww_ctx_set_grid_cap`` (a test and tuning parameter) caps every persistent launch,
so that small tensors take many trips: caps 1, 2, 3 and 0 (none) give odd, even and unequal numbers of trips per workgroup.

Shapes (B, H, W):
  depthwise   (3,20,76) the workload's image, 57 items; (2,41,10) three row segments of 14, 14, 13 rows and a last strip two columns
              wide; (1,21,3) two segments, an image narrower than a strip; (5,1,1)
  pointwise   (1,3,5) one partial tile; (2,8,8); (3,5,19) ragged; (2,20,76) the workload's image -- forward 128-pixel, backward 64-pixel
              tiles; from a pooled gradient (7,3,5) narrow, a tile spans several images; (3,8,8) an image is exactly one tile;
              (2,20,76) an image boundary inside a tile, 48 tiles with a ragged last one
  stem        (B,Hin,Win) = (3,40,151); (2,13,50) odd Ho: the last row pair has one row; (1,9,251) the stage-in-place path of both
              kernels; (2,7,9).  The backward runs through ww_conv_stem_bwd and through the recomputing form the model uses.
  full slabs  (432,2,76), (87,20,76), (103,40,151): more work items than the partial slabs have rows (1024 / 768 / 2048), so a
              residency round of workgroups is what limits the grid and the finalize kernels walk the partial rows in several
              passes (a thread of ww_colgroup_sum takes rows part, part + 256, ...; of colsum_body rows part, part + 64, ...).

Integer-exact data (tests/conv_trip_cases.py): y, g_in, dW, dbeta_in and dgamma_in must equal the float64 restatement bit for bit
at every cap.  What the finalize kernels derive from the sums -- ss, mr, the running statistics, coef_in -- is formed in double from
exact sums (k_bn_fwd_finalize, bn_bwd_finalize_group: the fp32 partials are widened before they are added, every product and
quotient is a double operation) and rounded to fp32 once: within 1 fp32 ulp of the float64 value, the ulp being that of the
larger term where the value is a difference or sum of two (shift = beta - mean * scale, Cc, the running statistics).  None of
them needs a wider allowance.  dW, dbeta_in and dgamma_in are double sums of integers below 2^24 and convert exactly."""
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

from tests import conv_trip_cases as K

pytestmark = pytest.mark.gpu
REPO = Path(__file__).resolve().parents[1]
DEV = "cuda:0"
ACTS = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}
CAPS = (1, 2, 3, 0)
C = K.C
REV_KNOBS = ("WW_STEM_FWD_REV", "WW_PW_FWD_REV", "WW_PW_BWD_REV", "WW_STEM_BWD_REV")


@pytest.fixture(scope="module")
def nat():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from wakeword_trainer_home_amd import _native
    _native.load()
    return _native


def f32(t):
    return None if t is None else t.float().to(DEV).contiguous()


def stored(t, dt):
    return None if t is None else t.float().to(dt).to(DEV).contiguous()


def bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16).cpu()


def ulps(got, ref, mag):
    """largest |got - ref| in fp32 ulps of max(|ref|, mag) per entry"""
    g = got.detach().cpu().double().numpy().reshape(-1)
    r = ref.numpy().reshape(-1)
    u = np.spacing(np.maximum(np.abs(r), mag.numpy().reshape(-1)).astype(np.float32)).astype(np.float64)
    return float((np.abs(g - r) / u).max())


# ------------------------------------------------------------------------------------------ device runs
def fwd_inputs(kind, c, dt):
    d = {k: f32(c[k]) for k in ("w", "gamma", "beta", "running_mean", "running_var")}
    if kind == "stem":
        d["x"] = f32(c["x"])
    else:
        d.update(y_in=stored(c["y_in"], dt), ss_in=f32(c["ss_in"]))
    return d


def run_fwd(nat, kind, d, dt):
    rm, rv = d["running_mean"].clone(), d["running_var"].clone()
    bn = nat.make_bn(d["gamma"], d["beta"], rm, rv, momentum=0.1, eps=1e-5)
    scratch = nat.layer_scratch(DEV)
    if kind == "stem":
        y, ss, mr = nat.conv_stem_fwd(d["x"], d["w"], bn, scratch, act=dt)
    else:
        y, ss, mr = (nat.dwconv3x3_fwd if kind == "dw" else nat.pwconv1x1_fwd)(d["y_in"], d["ss_in"], d["w"], bn, scratch)
    torch.cuda.synchronize()
    return dict(y=y, ss=ss, mr=mr, running_mean=rm, running_var=rv)


def check_fwd(out, ref, tag):
    assert torch.equal(out["y"].cpu().double(), ref["y"]), f"{tag}: y"
    for name in ("ss", "mr", "running_mean", "running_var"):
        e = ulps(out[name], ref[name], ref[name + "_mag"])
        assert e <= 1.0, f"{tag}: {name} off by {e:.2f} ulp"


def bwd_inputs(kind, c, dt):
    d = dict(w=f32(c["w"]), coef=f32(c["coef"]), y_out=stored(c["y_out"], dt), g=stored(c.get("g"), dt))
    if kind == "stem":
        d["x"] = f32(c["x"])
    else:
        d.update(y_in=stored(c["y_in"], dt), ss_in=f32(c["ss_in"]), mr_in=f32(c["mr_in"]), gamma_in=f32(c["gamma_in"]),
                 dpool=f32(c.get("dpool")), ss_out=f32(c.get("ss_out")))
    return d


def run_bwd(nat, kind, d, recompute=False):
    scratch = nat.layer_scratch(DEV)
    if kind == "stem":
        out = dict(dw=nat.conv_stem_bwd(d["g"], d["y_out"], d["coef"], d["x"], scratch, w=d["w"] if recompute else None))
    else:
        args = dict(y_out=d["y_out"], coef=d["coef"], y_in=d["y_in"], ss_in=d["ss_in"], mr_in=d["mr_in"], gamma_in=d["gamma_in"],
                    w=d["w"], scratch=scratch)
        if kind == "dw":
            r = nat.dwconv3x3_bwd(d["g"], **args)
        else:
            r = nat.pwconv1x1_bwd(d["g"], d["dpool"], ss_out=d["ss_out"], **args)
        out = dict(zip(("g_in", "dw", "coef_in", "dgamma", "dbeta"), r))
    torch.cuda.synchronize()
    return out


def check_bwd(out, ref, tag):
    assert torch.equal(out["dw"].cpu().double().reshape(ref["dw"].shape), ref["dw"]), f"{tag}: dW"
    if "g_in" not in ref:
        return
    assert torch.equal(out["g_in"].cpu().double(), ref["g_in"]), f"{tag}: g_in"
    assert torch.equal(out["dbeta"].cpu().double(), ref["dbeta"]), f"{tag}: dbeta_in"
    assert torch.equal(out["dgamma"].cpu().double(), ref["dgamma"]), f"{tag}: dgamma_in"
    e = ulps(out["coef_in"], ref["coef_in"], ref["coef_mag"])
    assert e <= 1.0, f"{tag}: coef_in off by {e:.2f} ulp"


def fwd_trips(nat, kind, c, ref, dname, caps, tag):
    """one forward case in one storage type at each cap; the stored tensor is also bit-equal between the caps"""
    d = fwd_inputs(kind, c, ACTS[dname])
    first = None
    for cap in caps:
        nat.set_grid_cap(DEV, cap)
        out = run_fwd(nat, kind, d, ACTS[dname])
        check_fwd(out, ref, f"{tag} {dname} cap {cap}")
        first = bits(out["y"]) if first is None else first
        assert torch.equal(bits(out["y"]), first), f"{tag} {dname} cap {cap}: y differs from cap {caps[0]}"


def bwd_trips(nat, kind, c, ref, dname, caps, tag):
    d = bwd_inputs(kind, c, ACTS[dname])
    first = None
    for cap in caps:
        nat.set_grid_cap(DEV, cap)
        for recompute in ((False, True) if kind == "stem" else (False,)):
            out = run_bwd(nat, kind, d, recompute)
            check_bwd(out, ref, f"{tag} {dname} cap {cap}{' recomputing' if recompute else ''}")
        if kind != "stem":
            first = bits(out["g_in"]) if first is None else first
            assert torch.equal(bits(out["g_in"]), first), f"{tag} {dname} cap {cap}: g_in differs from cap {caps[0]}"


# ------------------------------------------------------------------------------------------ integer-exact cases under the caps
@pytest.mark.parametrize("case", K.FWD_CASES, ids=K.case_id)
def test_forward_trips_are_exact(nat, case):
    c, ref = K.fwd_case(*case)
    try:
        for dname in ACTS:
            fwd_trips(nat, case[0], c, ref, dname, CAPS, K.case_id(case))
    finally:
        nat.set_grid_cap(DEV, 0)


@pytest.mark.parametrize("case", K.BWD_CASES, ids=K.case_id)
def test_backward_trips_are_exact(nat, case):
    c, ref = K.bwd_case(*case)
    try:
        for dname in ACTS:
            bwd_trips(nat, case[0], c, ref, dname, CAPS, K.case_id(case))
    finally:
        nat.set_grid_cap(DEV, 0)


@pytest.mark.parametrize("kind", ["dw", "pw", "stem"])
def test_full_slabs_are_exact(nat, kind):
    """No cap, as many workgroups as the partial slabs have rows: the finalize kernels walk the rows in several passes."""
    shape = K.FULL_SHAPES[kind]
    c, ref = K.build_fwd(kind, shape, small=True)
    for dname in ("fp32", "bf16"):
        fwd_trips(nat, kind, c, ref, dname, (0,), f"full {kind} fwd")
    del c, ref
    for pooled in ((False, True) if kind == "pw" else (False,)):
        c, ref = K.build_bwd(kind, shape, pooled=pooled, small=True)
        for dname in ("fp32", "bf16"):
            bwd_trips(nat, kind, c, ref, dname, (0,), f"full {kind} bwd{' pooled' if pooled else ''}")
        del c, ref


def run_ascending():
    """child process entry (every WW_*_REV knob 0: the tile / row walks ascend): the small integer cases at caps 1 and 3"""
    assert all(os.environ.get(k) == "0" for k in REV_KNOBS)
    from wakeword_trainer_home_amd import _native as nat
    nat.load()
    try:
        for dname in ACTS:
            for case in K.FWD_CASES:
                c, ref = K.fwd_case(*case)
                fwd_trips(nat, case[0], c, ref, dname, (1, 3), "ascending " + K.case_id(case))
            for case in K.BWD_CASES:
                c, ref = K.bwd_case(*case)
                bwd_trips(nat, case[0], c, ref, dname, (1, 3), "ascending " + K.case_id(case))
    finally:
        nat.set_grid_cap(DEV, 0)
    print(f"ascending: {len(K.FWD_CASES)} forward and {len(K.BWD_CASES)} backward cases exact")


def test_ascending_walks_are_exact(nat):
    """The WW_*_REV knobs are read once per process: one child interpreter with all four at 0."""
    assert all(os.environ.get(k, "1") != "0" for k in REV_KNOBS), "this process must run the default (descending) order"
    code = f"import sys; sys.path.insert(0, {str(REPO)!r}); from tests.test_conv_trips_gpu import run_ascending; run_ascending()"
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=dict(os.environ, **{k: "0" for k in REV_KNOBS}),
                       timeout=600)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-3000:])
    assert "cases exact" in r.stdout


# ------------------------------------------------------------------------------------------ round-off away from zero mean
U = 2.0 ** -24
# (stored g_in in roundings of its largest entry, dW, dbeta_in): tests/test_hip_kernels.py:test_conv_bwd_layers (fp32),
# tests/test_bf16_mode.py:test_conv_bwd_layers_bf16, tests/test_fp16_mode.py:test_conv_bwd_layers_fp16, tests/test_pw_bwd_tiles.py
LAYER_BOUNDS = {("dw", "fp32"): (2e-5, 2e-5, 2e-5), ("pw", "fp32"): (2e-5, 2e-5, 2e-5),
                ("dw", "bf16"): (2.0 ** -8, 1e-4, 1e-4), ("pw", "bf16"): (3 * 2.0 ** -8, 4e-3, 1e-4),
                ("dw", "fp16"): (2.0 ** -10, 2e-6, 1e-4), ("pw", "fp16"): (3 * 2.0 ** -10, 2 * 2.0 ** -10, 1e-4)}


@pytest.mark.parametrize("dname", list(ACTS))
@pytest.mark.parametrize("case", K.ROUNDOFF_CASES, ids=K.case_id)
def test_roundoff_away_from_zero_mean(nat, case, dname):
    """Unit-normal y_in plus a per-channel offset of up to 3 standard deviations, one workgroup (cap 1) and no cap.  k_dw_bwd forms
    rstd * (sum g*y - mean * sum g) once per workgroup: the difference cancels more the more a workgroup has summed and the further
    the mean lies from zero.  Stored tensors, dW and dbeta_in keep the bounds of the layer tests.  dgamma_in, Bc and Cc of coef_in
    are held to the a-priori bound of the summation the kernel performs, per channel
        n * 2^-24 * rstd * (sum |g y| + |mean| sum |g|)        (dbeta_in's share of Cc: n * 2^-24 * sum |g|)
    with n = the values one thread adds in sequence at that cap (conv_trip_cases.values_per_thread) and the sums taken over the
    float64 reference g_in.  They are compared with float64 sums of the device's own stored g_in, which is first held to its bound:
    the summation bound covers the summation, not the rounding of g_in.  A = gamma * rstd holds no sum: 1 ulp.  Measured on the
    MI355X: profiles/r13_conv_trips_measured.txt."""
    kind, shape = case
    c = K.roundoff_case(kind, shape, dname)
    dt = ACTS[dname]
    d = bwd_inputs(kind, c, dt)
    n_pix = shape[0] * shape[1] * shape[2]
    mean, rstd, gamma = c["mr_in"][:C], c["mr_in"][C:], c["gamma_in"]
    tol_g, tol_w, tol_b = LAYER_BOUNDS[(kind, dname)]
    rel = lambda got, ref: ((got - ref).abs().max() / ref.abs().max()).item()
    ref_g = c["ref_g_in"] if c["dt"] is None else K.mround(c["ref_g_in"], c["dt"])
    sum_g = ref_g.abs().reshape(-1, C).sum(0)
    sum_gy = (ref_g * c["y_in"]).abs().reshape(-1, C).sum(0)
    A = gamma * rstd
    try:
        for cap in (1, 0):
            nat.set_grid_cap(DEV, cap)
            out = run_bwd(nat, kind, d)
            gi = out["g_in"].cpu().double()
            e_g, e_w = rel(gi, c["ref_g_in"]), rel(out["dw"].cpu().double().reshape(-1), c["ref_dw"].reshape(-1))
            s1 = gi.reshape(-1, C).sum(0)
            s2 = (gi * ((c["y_in"] - mean) * rstd)).reshape(-1, C).sum(0)
            e_b = rel(out["dbeta"].cpu().double(), s1)
            n = K.values_per_thread(kind, shape, cap)
            b1, b2 = n * U * sum_g, n * U * rstd * (sum_gy + mean.abs() * sum_g)
            coef_ref, coef_mag = K.coef_from_sums(s1, s2, n_pix, gamma, mean, rstd)
            ulp = torch.from_numpy(np.spacing(torch.maximum(coef_ref.abs(), coef_mag).numpy().astype(np.float32)).astype(np.float64))
            coef_tol = torch.cat([torch.zeros(C), A * rstd * b2 / n_pix, A * (mean.abs() * rstd * b2 + b1) / n_pix]) + ulp
            r_ga = ((out["dgamma"].cpu().double() - s2).abs() / (b2 + np.spacing(np.float32(1)) * s2.abs())).max().item()
            r_c = ((out["coef_in"].cpu().double() - coef_ref).abs() / coef_tol).reshape(3, C).max(dim=1).values.tolist()
            print(f"\nROUNDOFF {K.case_id(case)} {dname} cap {cap} n={n}: g_in {e_g:.2e}/{tol_g:.2e} dW {e_w:.2e}/{tol_w:.2e} dbeta {e_b:.2e}/{tol_b:.2e} "
                  f"dgamma/bound {r_ga:.1e} A/ulp {r_c[0]:.2f} Bc/bound {r_c[1]:.1e} Cc/bound {r_c[2]:.1e}")
            assert e_g <= tol_g, "dL/dz_in"
            assert e_w < tol_w, "dW"
            assert e_b < tol_b, "dbeta_in"
            assert r_ga <= 1.0, "dgamma_in"
            assert max(r_c) <= 1.0, "coef_in"
    finally:
        nat.set_grid_cap(DEV, 0)


# ------------------------------------------------------------------------------------------ the whole stack under a cap
@pytest.mark.parametrize("act", ["fp32", "bf16"])
@pytest.mark.parametrize("B,F,T", [(3, 13, 49), (4, 40, 151)])
def test_whole_stack_under_a_cap(nat, act, B, F, T):
    """The per-tensor checkers of tests/test_cnn_front.py with their bounds, every conv kernel and the two frequency-pool kernels on
    1 and on 3 workgroups: cnn_small (the recomputing stem backward, the pooled-gradient pointwise backward) and the CRNN front end."""
    from tests import test_cnn_front as TF
    try:
        for cap in (1, 3):
            nat.set_grid_cap(DEV, cap)
            TF.check_cnn_small(nat, act, B, F, T, 0.0, seed=B + F)
            TF.check_front(nat, act, B, F, T, seed=B + F + T)
    finally:
        nat.set_grid_cap(DEV, 0)


def test_grid_cap_argument_checks(nat):
    """a negative cap is refused; a cap larger than the work changes nothing, bit for bit (finalized outputs included)"""
    with pytest.raises(ValueError):
        nat.set_grid_cap(DEV, -1)
    try:
        for case in (("stem", (2, 13, 50)), ("dw", (2, 41, 10)), ("pw", (3, 5, 19))):
            kind = case[0]
            for dname in ("fp32", "bf16"):
                df = fwd_inputs(kind, K.fwd_case(*case)[0], ACTS[dname])
                db = bwd_inputs(kind, K.bwd_case(*case)[0], ACTS[dname])
                res = []
                for cap in (0, 100000):
                    nat.set_grid_cap(DEV, cap)
                    res.append({**run_fwd(nat, kind, df, ACTS[dname]), **{"b_" + k: v for k, v in run_bwd(nat, kind, db).items()}})
                for k in res[0]:
                    assert torch.equal(bits(res[0][k]), bits(res[1][k])), (case, dname, k)
    finally:
        nat.set_grid_cap(DEV, 0)
