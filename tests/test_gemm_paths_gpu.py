"""The dense GEMM family per launch path on the device (tests/gemm_cases.py holds the cases, the float64 restatements and the
derivation of the bounds; tests/test_gemm_paths_host.py proves, without a device, that every case reaches the path it is listed for).

  * integer-exact data: forward (y and pre) and backward (dx, dw, db) equal the float64 products bit for bit, every case x mode,
    every epilogue; the immediate (k_splitk_sum) and the deferred (ww_deferred_reduce_flush) sum of the same partials equal each other
    and the reference;
  * N(0,1) data: every element within the derived  d u S[i]  of float64 on the restated operands; the largest err / bound per
    product is printed;
  * k_gemm_pair<*, 2, 0> (128-row dX tiles with a deep stage) exists only under WW_GEMM_PAIR_TALL=2, which the library reads once:
    a child process runs those cases."""
import os
import subprocess
import sys
from pathlib import Path

import pytest
import torch

from tests import gemm_cases as G

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
REPO = Path(__file__).resolve().parents[1]
CASE_MODES = lambda cases: [(c, m) for c in cases for m in G.MODES]
case_mode_id = lambda v: G.shape_id(v) if isinstance(v, tuple) else v


def dev32(t, offset=False):
    """float64 host tensor -> float32 on the device; offset: as a contiguous view 4 bytes past a 16-byte boundary"""
    t = t.float()
    if not offset:
        return t.to(DEV)
    buf = torch.empty(t.numel() + 1, dtype=torch.float32, device=DEV)
    v = buf[1:].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % 16 == 4
    return v


def run_fwd(nat, xd, wd, bd, epi, mode):
    """-> (pre or None, y) as float64 host tensors"""
    act, p = epi
    if act is None:
        return None, nat.linear_mfma_fwd(xd, wd, bd, mode=G.MODES[mode]).cpu().double()
    y, pre = nat.linear_mfma_fwd(xd, wd, bd, act=act, dropout_p=p, seed=G.SEED, step=G.STEP, sample_offset=G.OFFSET,
                                 mode=G.MODES[mode], want_pre=True)
    return pre.cpu().double(), y.cpu().double()


def run_bwd(nat, xd, wd, pred, dyd, epi, mode, need_dx=True, defer=False, want_nz=None):
    """-> (dx or None, dw, db) as float64 host tensors; defer: the partial sums queued and run by deferred_flush"""
    act, p = epi
    lib, cx = nat.load(), nat.ctx(DEV)
    assert lib.ww_deferred_reduce_pending(cx) == 0
    dx, dw, db = nat.linear_mfma_bwd(xd, wd, pred if act != G.ACT_NONE else None, dyd, act=act, dropout_p=p, seed=G.SEED, step=G.STEP,
                                     sample_offset=G.OFFSET, mode=G.MODES[mode], need_dx=need_dx, defer=defer)
    if defer:
        assert lib.ww_deferred_reduce_pending(cx) == (1 if want_nz > 1 else 0)      # one split: nothing to sum, nothing queued
        nat.deferred_flush(DEV)
        assert lib.ww_deferred_reduce_pending(cx) == 0
    torch.cuda.synchronize()
    return (None if dx is None else dx.cpu().double()), dw.cpu().double(), db.cpu().double()


def bad_elements(got, ref):
    return int((got != ref).sum().item())


def check_bwd_exact(nat, shape, mode, nz, epilogues=G.BWD_EPILOGUES, need_dx=True, offset=False):
    """the integer-exact backward of one shape and mode: immediate and (with several splits) deferred, both bit-equal to float64"""
    x, w, b, dy = G.exact_operands(*shape)
    xd, wd, dyd = dev32(x, offset), dev32(w, offset), dev32(dy, offset)
    pred = None
    for epi in epilogues:
        pre, dx_ref, dw_ref, db_ref = G.exact_bwd(shape, epi)
        if pred is None:
            pred = dev32(pre, offset)
        runs = {"immediate": run_bwd(nat, xd, wd, pred, dyd, epi, mode, need_dx)}
        if nz > 1:
            runs["deferred"] = run_bwd(nat, xd, wd, pred, dyd, epi, mode, need_dx, defer=True, want_nz=nz)
        for how, (dx, dw, db) in runs.items():
            bad = dict(dw=bad_elements(dw, dw_ref), db=bad_elements(db, db_ref))
            if need_dx:
                bad["dx"] = bad_elements(dx, dx_ref)
            assert not any(bad.values()), (shape, mode, epi, how, bad)
        if nz > 1:
            assert torch.equal(runs["immediate"][1], runs["deferred"][1])


# ------------------------------------------------------------------------------------------ integer-exact
@pytest.fixture(scope="module")
def nat():
    from wakeword_trainer_home_amd import _native
    return _native


@pytest.mark.parametrize("case,mode", CASE_MODES(G.FWD_CASES), ids=case_mode_id)
def test_forward_is_bit_exact_on_integer_data(nat, case, mode):
    shape, _ = case
    x, w, b, _ = G.exact_operands(*shape)
    xd, wd, bd = dev32(x), dev32(w), dev32(b)
    for epi in G.FWD_EPILOGUES:
        pre_ref, y_ref = G.exact_fwd(shape, epi)
        pre, y = run_fwd(nat, xd, wd, bd, epi, mode)
        bad = dict(y=bad_elements(y, y_ref), pre=0 if pre is None else bad_elements(pre, pre_ref))
        assert not any(bad.values()), (shape, mode, epi, bad)


@pytest.mark.parametrize("case,mode", CASE_MODES(G.BWD_CASES), ids=case_mode_id)
def test_backward_is_bit_exact_on_integer_data(nat, case, mode):
    shape, want = case
    check_bwd_exact(nat, shape, mode, want[G.mode_class(mode)]["nz"])


@pytest.mark.parametrize("mode", list(G.MODES))
def test_weight_gradient_alone_is_bit_exact(nat, mode):
    """need_dx = False: dW through launch_gemm (no pair), its partials summed at once and deferred"""
    nz = nat.plan_gemm("bwd", *G.NO_DX_CASE, mode=G.MODES[mode], need_dx=False)["nz"]
    assert nz == 2
    check_bwd_exact(nat, G.NO_DX_CASE, mode, nz, need_dx=False)


@pytest.mark.parametrize("mode", list(G.MODES))
def test_operands_off_the_16_byte_grid_are_bit_exact(nat, mode):
    """x, w, bias, dy as views 4 bytes past a 16-byte boundary: the scalar fetch branch although every leading dimension is a
    multiple of 4 (ww_gemm_plan with aligned = 0)"""
    shape = G.UNALIGNED_CASE
    x, w, b, _ = G.exact_operands(*shape)
    pre_ref, y_ref = G.exact_fwd(shape, (None, None))
    _, y = run_fwd(nat, dev32(x, True), dev32(w, True), dev32(b, True), (None, None), mode)
    assert bad_elements(y, y_ref) == 0
    check_bwd_exact(nat, shape, mode, G.UNALIGNED_PLAN[G.mode_class(mode)]["nz"], epilogues=[(G.ACT_NONE, 0.0)], offset=True)


# ------------------------------------------------------------------------------------------ round-off
@pytest.mark.parametrize("case,mode", CASE_MODES(G.FWD_CASES), ids=case_mode_id)
def test_forward_round_off_is_within_the_derived_bound(nat, case, mode):
    (M, K, N), _ = case
    x, w, b, _, _ = G.round_operands(M, K, N)
    rx, rw, b64 = G.restate(x, mode), G.restate(w, mode), b.double()
    bound = G.bound_y(rx, rw, b64, K)
    xd, wd, bd = x.to(DEV), w.to(DEV), b.to(DEV)
    worst = 0.0
    for epi in G.ROUND_FWD_EPILOGUES:
        pre_ref, y_ref = G.fwd_ref(rx, rw, b64, epi)
        pre, y = run_fwd(nat, xd, wd, bd, epi, mode)
        scale = 2.0 if epi[1] else 1.0
        ry = G.worst_ratio(y, y_ref, scale * bound)
        rp = 0.0 if pre is None else G.worst_ratio(pre, pre_ref, bound)
        print(f"ROUNDOFF {mode} y {M}x{K}x{N} epi={epi} err/bound={ry:.4f} pre={rp:.4f}")
        worst = max(worst, ry, rp)
    assert worst <= 1.0, worst


@pytest.mark.parametrize("case,mode", CASE_MODES(G.BWD_CASES), ids=case_mode_id)
def test_backward_round_off_is_within_the_derived_bound(nat, case, mode):
    (M, K, N), want = case
    plan = want[G.mode_class(mode)]
    x, w, _, dy, pre = G.round_operands(M, K, N)
    rx, rw = G.restate(x, mode), G.restate(w, mode)
    xd, wd, dyd, pred = x.to(DEV), w.to(DEV), dy.to(DEV), pre.to(DEV)
    worst = {}
    for epi in G.ROUND_BWD_EPILOGUES:
        dpre = G.dpre_ref(dy.double(), pre.double(), epi)
        assert torch.equal(dpre.float().double(), dpre)                     # fp32 holds it: k_linear_dpre adds no rounding
        dpre_mm = G.restate(dpre.float(), mode)
        refs = G.bwd_ref(rx, rw, dpre, dpre_mm)
        bounds = G.bounds_bwd(rx, rw, dpre, dpre_mm, M, N, plan["kps"], plan["nz"])
        for how in ("immediate", "deferred") if plan["nz"] > 1 else ("immediate",):
            got = run_bwd(nat, xd, wd, pred, dyd, epi, mode, defer=how == "deferred", want_nz=plan["nz"])
            for name, g, r, bnd in zip(("dx", "dw", "db"), got, refs, bounds):
                ratio = G.worst_ratio(g, r, bnd)
                print(f"ROUNDOFF {mode} {name} {M}x{K}x{N} epi={epi} {how} err/bound={ratio:.4f}")
                worst[name] = max(worst.get(name, 0.0), ratio)
    assert all(v <= 1.0 for v in worst.values()), worst


# ------------------------------------------------------------------------------------------ WW_GEMM_PAIR_TALL=2, in a child process
_CHILD = """
import torch
from wakeword_trainer_home_amd import _native as nat
from tests import gemm_cases as G
from tests.test_gemm_paths_gpu import check_bwd_exact
for shape in G.TALL2_CASES:
    for mode in ("bf16", "fp32"):
        p = nat.plan_gemm("bwd", *shape, mode=G.MODES[mode])
        assert p["env_pair_tall"] == 2 and p["paired"] == 1, p               # the library did read the switch
        assert p["dx_cfg"] == p["dx_cfg_plain"] == (1 if shape[0] >= 8192 else 0) and not p["dx_shallow"], p
        check_bwd_exact(nat, shape, mode, p["nz"])
print("tall pair ok")
"""


def test_tall_pair_with_128_row_tiles_is_bit_exact_in_a_child_process():
    env = dict(os.environ, WW_GEMM_PAIR_TALL="2")
    r = subprocess.run([sys.executable, "-c", _CHILD], cwd=REPO, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "tall pair ok" in r.stdout
