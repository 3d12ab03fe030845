"""Float64 restatements, case builders, error bounds and the case table of the dense GEMM family (csrc/ww_linear.hip: gemm_block
behind ww_linear_mfma_fwd / _bwd, k_gemm_pair, the split-K partials with k_splitk_sum and the deferred flush, k_linear_dpre,
k_colsum_any), shared by test_gemm_paths_host.py and test_gemm_paths_gpu.py.  No device code, nothing imported from the package.

Two instruments, as in nhwc_cases.py:

INTEGER-EXACT cases.  Operands are integers in [-3, 3] (biases |b| <= 64) from an index hash whose phase depends on the 64-row
tile, the 32-wide K stage, the row within the tile, the column quad and the column within the quad.  A read across a tile,
stage, split or quad boundary, a transposed fragment or a swapped bx / by therefore changes a sum and cannot cancel.  Every
operand is exact in bf16 and fp16, every product is an integer, and the sum of the ABSOLUTE values of the terms of every output is
below 2^24, so every full sum and every partial sum of any split, in any order, is an integer fp32 holds: the device must return
the float64 product bit for bit in all three modes.  ``exactness`` asserts the conditions.  Epilogues: none and ReLU are exact;
Hardswish and Hardsigmoid are nhwc_cases.act32 (lin_act operation by operation in fp32, on integer pre-activations the device's
bits); dropout at p = 0.5 scales by exactly 2, its mask is oracle.cnn_small.dropout_keep_mask.  Backward: dpre = dy * 2 * keep *
(pre > 0) is an integer of magnitude <= 6, exact in both 16-bit types.

ROUND-OFF cases.  N(0,1) data against float64 on the operands restated in the mode's matrix type (fp32: as they are; bf16 / fp16:
rounded once, as stage_tile rounds them when it fills LDS).  A product of two 16-bit values is exact in fp32; the fp32 MFMA fuses
each product into the accumulation.  PER-ELEMENT bounds  d * u * S[i],  u = 2^-24,  S[i] = the sum of |terms| of element i,
with d read off the kernel's order of operations:
    gemm_block keeps one fp32 accumulator per output and feeds it the K terms of its split through a chain of MFMAs (32x32x2 fp32:
    2 k per instruction; 32x32x16 bf16 / fp16: 16 k per instruction), LDS stage after LDS stage, in k order.  A chain of n fused
    accumulations into fp32 rounds at most n times, each on a partial sum of magnitude <= S (the sums inside one 16-bit MFMA are
    a short tree, which rounds no more often than the chain).  The project's rule for a matrix-core dot product of n terms
    (nhwc_cases.py: "fma chain + tree") is  d = n + 1.
  y   = acc + bias:                 (K + 1) for the dot, 1 for the bias add, 1 for the stored value      -> d = K + 3
        ReLU and p = 0.5 dropout (x 2) are exact on top of it and 1-Lipschitz up to the factor 2 that S carries too.
  dx  = sum over N:                 (N + 1) + 1                                                             -> d = N + 2
  dw  = nz partials of kps rows each, every one a chain of its own: (kps + 1) u S_z each, sum_z S_z = S; then their sum in
        fixed order (k_splitk_sum: fp32, nz - 1 additions; the deferred flush: double, one rounding), and the stored value
                                                                                                            -> d = min(kps, M) + 1 + nz + 1
  db  = k_colsum_any: double accumulation (its own round-off is 2^-53 M S, nothing beside u), one rounding to fp32, one for the
        stored value                                                                                        -> d = 2
  The 16-bit modes see dpre rounded to the matrix type at LDS-fill time; the reference rounds the same fp32 dpre the same way, so
  that rounding is not an error.  db is summed from the fp32 dpre in every mode.
The tests print the largest err / bound per product; nothing here is fitted to what the device returns.

THE CASE TABLE lists, per shape, the plan ww_gemm_plan must report (the launchers' own dispatch code), derived by hand from the
rules in ww_linear.hip:
    gemm_tile_cfg: cfg 2 (128 x 128) iff EPI != 1, 16-bit mode, both extents >= 128 and ceil(rA/128) ceil(rB/128) nz >= 256;
                   else cfg 1 (128 x 64) iff rowsA >= 8192; else cfg 0 (64 x 64)
    shallow:       16-bit mode, contraction <= 32, one split, cfg != 2: one 32-deep LDS stage
    stage depth:   fp32 32; 16-bit 128, cfg 2 64, shallow 32
    vec:           base on 16 bytes and the leading dimension a multiple of 4 (fwd: K for both; dX: N for dpre, K for w; dW: N, K)
    dw_splits:     min(ceil(1024 / (ceil(N/64) ceil(K/64))), M / 128, 256), at least 1;  kps = ceil(ceil(M / splits) / kt) kt with
                   kt = 128 (16-bit) / 32 (fp32);  nz = ceil(M / kps)
    pair:          refused when dX is cfg 2, when dW is not cfg 0, when dW is shallow (M <= 32, 16-bit); a tall (cfg 1) deep dX is
                   paired on 64-row tiles (WW_GEMM_PAIR_TALL=1, the default) or 128-row tiles (=2)
    k_linear_dpre: min(ceil(M N / 256), 4096) workgroups;  k_splitk_sum: min((N K / 4 + 255) / 256 + 1, 2048) workgroups x 1024 sums
"""
import functools
import math

import numpy as np
import torch

from oracle.cnn_small import dropout_keep_mask
from tests.nhwc_cases import act32

U = 2.0 ** -24
LIMIT = float(2 ** 24)
MODES = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}
SEED, STEP, OFFSET = 9, 5, 3                     # the Philox stream of every dropout epilogue here
ACT_NONE, ACT_HARDSWISH, ACT_RELU, ACT_HARDSIGMOID = 0, 1, 2, 3      # WW_LIN_*
# epilogues: (activation, dropout p).  Forward EPI 1 (always with the pre-activation copy); (None, None) = EPI 2, plain + bias
FWD_EPILOGUES = [(None, None)] + [(a, p) for a in (ACT_NONE, ACT_RELU, ACT_HARDSWISH, ACT_HARDSIGMOID) for p in (0.0, 0.5)]
BWD_EPILOGUES = [(ACT_NONE, 0.0), (ACT_NONE, 0.5), (ACT_RELU, 0.0), (ACT_RELU, 0.5)]
ROUND_FWD_EPILOGUES = [(None, None), (ACT_RELU, 0.5)]
ROUND_BWD_EPILOGUES = [(ACT_NONE, 0.0), (ACT_RELU, 0.5)]


# ------------------------------------------------------------------------------------------ integer patterns
def gpattern(rows, cols, seed, lo=-3, hi=3):
    """(rows, cols) integers in [lo, hi]: a hash of (row tile of 64, row in the tile, K stage of 32, column quad, column in the quad)"""
    i = torch.arange(rows, dtype=torch.int64)[:, None]
    k = torch.arange(cols, dtype=torch.int64)[None, :]
    it, ir, ks, kq, kr = i // 64, i % 64, k // 32, k // 4, k % 4
    v = 5 * kr + 3 * kq + 7 * ir + 11 * it + 13 * ks + (ir * (kq + 1)) % 7 + ((it + 1) * (ks + 2)) % 5 + ((ir + it) * (kr + 2)) % 3 + seed
    return (v % (hi - lo + 1) + lo).double()


@functools.lru_cache(maxsize=4)
def exact_operands(M, K, N):
    """x (M,K), w (N,K), dy (M,N) in [-3, 3], bias (N) in [-64, 64]; float64"""
    return gpattern(M, K, 1), gpattern(N, K, 2), gpattern(1, N, 3, -64, 64)[0].contiguous(), gpattern(M, N, 4)


@functools.lru_cache(maxsize=4)
def round_operands(M, K, N):
    g = torch.Generator().manual_seed(M * 7 + K * 3 + N)
    x = torch.randn(M, K, generator=g)
    w = torch.randn(N, K, generator=g) / K ** 0.5
    b = torch.randn(N, generator=g)
    dy = torch.randn(M, N, generator=g)
    pre = torch.randn(M, N, generator=g)
    return x, w, b, dy, pre


@functools.lru_cache(maxsize=4)
def keep_mask(M, N, p):
    """float64 (M, N): 1 where the dropout epilogue keeps the element"""
    return torch.from_numpy(dropout_keep_mask(M, N, p, SEED, STEP, OFFSET).astype(np.float64))


def restate(t, mode):
    """a float32 tensor as the mode's matrix cores see it, in float64"""
    return t.to(MODES[mode]).double() if mode != "fp32" else t.double()


# ------------------------------------------------------------------------------------------ references
def fwd_ref(x, w, b, epi):
    """float64 (pre, y) of ww_linear_mfma_fwd for float64 operands; epi = (act, p) or (None, None)"""
    pre = x @ w.t() + b
    act, p = epi
    if act is None:
        return pre, pre
    y = act32(act, pre) if act in (ACT_HARDSWISH, ACT_HARDSIGMOID) else (pre.clamp_min(0) if act == ACT_RELU else pre)
    if p:
        y = y * keep_mask(x.shape[0], w.shape[0], p) * (1.0 / (1.0 - p))
    return pre, y


def dpre_ref(dy, pre, epi):
    """k_linear_dpre in float64: dy * dropout * act'(pre), for activation none / ReLU (exact in fp32 at p = 0.5)"""
    act, p = epi
    assert act in (ACT_NONE, ACT_RELU)
    g = dy * keep_mask(dy.shape[0], dy.shape[1], p) * (1.0 / (1.0 - p)) if p else dy
    return g * (pre > 0) if act == ACT_RELU else g


def bwd_ref(x, w, dpre, dpre_mm=None):
    """float64 (dx, dw, db); dpre_mm: dpre as the matrix cores see it (db sums the fp32 dpre itself)"""
    dm = dpre if dpre_mm is None else dpre_mm
    return dm @ w, dm.t() @ x, dpre.sum(0)


@functools.lru_cache(maxsize=len(FWD_EPILOGUES))
def exact_fwd(shape, epi):
    """(pre, y) of an integer-exact case, computed once for the three modes"""
    x, w, b, _ = exact_operands(*shape)
    return fwd_ref(x, w, b, epi)


@functools.lru_cache(maxsize=len(BWD_EPILOGUES))
def exact_bwd(shape, epi):
    """(pre, dx, dw, db) of an integer-exact case, computed once for the three modes and both ways of summing the partials"""
    x, w, b, dy = exact_operands(*shape)
    pre = x @ w.t() + b
    return (pre,) + bwd_ref(x, w, dpre_ref(dy, pre, epi))


def exactness(M, K, N):
    """the two conditions of an integer-exact case (module docstring), over every epilogue it is run with"""
    x, w, b, dy = exact_operands(M, K, N)
    for name, t in dict(x=x, w=w, b=b, dy=dy, dpre=2 * dy).items():
        assert torch.equal(t, t.round()), name
        for dt in (torch.bfloat16, torch.float16, torch.float32):
            assert torch.equal(t.to(dt).double(), t), f"{name} does not round-trip through {dt}"
    sums = dict(y=x.abs() @ w.abs().t() + b.abs(), dx=(2 * dy.abs()) @ w.abs(), dw=(2 * dy.abs()).t() @ x.abs(), db=(2 * dy.abs()).sum(0))
    for name, s in sums.items():
        assert s.max().item() < LIMIT, f"{name}: a partial sum may round ({s.max().item():.3g} >= 2^24)"
    pre = x @ w.t() + b
    assert torch.equal(pre, pre.round()) and torch.equal(pre.float().double(), pre)
    # Hardswish multiplies z by clamp(z + 3, 0, 6) <= 6 before the one rounding product with fl(1/6): still an exact integer
    assert (6 * pre.abs()).max().item() < LIMIT
    return sums


# ------------------------------------------------------------------------------------------ round-off bounds
def bound_y(x, w, b, K):
    return (K + 3) * U * (x.abs() @ w.abs().t() + b.abs())


def bounds_bwd(x, w, dpre, dpre_mm, M, N, kps, nz):
    """per-element bounds of (dx, dw, db) (module docstring)"""
    return ((N + 2) * U * (dpre_mm.abs() @ w.abs()), (min(kps, M) + 1 + nz + 1) * U * (dpre_mm.abs().t() @ x.abs()),
            2 * U * dpre.abs().sum(0))


def worst_ratio(got, ref, bound):
    """max over the elements of |got - ref| / bound (a zero bound demands equality: inf if it is missed)"""
    err = (got - ref).abs()
    ratio = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err > 0, math.inf, 0.0))
    return ratio.max().item()


# ------------------------------------------------------------------------------------------ the cases and the plan each is for
# forward (M, K, N): cfg = (16-bit EPI 2, 16-bit EPI 1, fp32), shallow16 (fp32 is never shallow), vec (both operands: K % 4 == 0)
FWD_CASES = [
    ((130, 200, 70), dict(cfg=(0, 0, 0), shallow16=False, vec=1)),      # cfg 0 deep: one 128-deep stage + a 72-wide tail; M, N off the tile
    ((130, 197, 70), dict(cfg=(0, 0, 0), shallow16=False, vec=0)),      # the scalar fetch branch, ragged K tail
    ((66, 32, 66), dict(cfg=(0, 0, 0), shallow16=True, vec=1)),         # K = exactly one fp32 stage (and the one shallow stage)
    ((66, 33, 66), dict(cfg=(0, 0, 0), shallow16=False, vec=0)),        # one fp32 stage + 1; the first K past the shallow form
    ((66, 128, 66), dict(cfg=(0, 0, 0), shallow16=False, vec=1)),       # K = exactly one 16-bit stage
    ((66, 129, 66), dict(cfg=(0, 0, 0), shallow16=False, vec=0)),       # one 16-bit stage + 1
    ((130, 24, 70), dict(cfg=(0, 0, 0), shallow16=True, vec=1)),        # cfg 0 shallow
    ((130, 30, 70), dict(cfg=(0, 0, 0), shallow16=True, vec=0)),        # cfg 0 shallow, scalar fetch
    ((8229, 40, 70), dict(cfg=(1, 1, 1), shallow16=False, vec=1)),      # cfg 1 deep (M >= 8192), ragged last 128-row tile
    ((8229, 24, 20), dict(cfg=(1, 1, 1), shallow16=True, vec=1)),       # cfg 1 shallow
    ((1930, 72, 1930), dict(cfg=(2, 0, 0), shallow16=False, vec=1)),    # cfg 2: 16 x 16 tiles of 128, a 64-deep stage + 8, ragged both ways
]
# every (cfg, shallow) launch_gemm has a launch line for and gemm_tile_cfg can select, per (mode class, EPI)
FWD_REACHABLE = {("16", 2): {(0, False), (0, True), (1, False), (1, True), (2, False)},
                 ("16", 1): {(0, False), (0, True), (1, False), (1, True)},
                 ("32", 2): {(0, False), (1, False)}, ("32", 1): {(0, False), (1, False)}}

# backward (M, K, N): per mode class ("16", "32") what ww_gemm_plan(which = 1) must report; dx / dw = (cfg as launched, shallow)
_P = lambda refused, dx, dw, kps, nz, dx_plain=None: dict(refused=refused, dx=dx, dw=dw, kps=kps, nz=nz, dx_plain=dx[0] if dx_plain is None else dx_plain)
BWD_CASES = [
    # pair, one split
    ((77, 72, 70), {"16": _P("paired", (0, False), (0, False), 77, 1), "32": _P("paired", (0, False), (0, False), 77, 1)}),
    # pair, 2 splits (16-bit: the last one a single row); M N odd -> the partials start off the 16-byte grid; N K % 4 == 3 -> the
    # scalar tail of k_splitk_sum and every other partial off the grid as well; every leading dimension odd -> no float4 fetch
    ((257, 33, 71), {"16": _P("paired", (0, False), (0, False), 256, 2), "32": _P("paired", (0, False), (0, False), 160, 2)}),
    # pair, shallow dX (N = 2)
    ((130, 40, 2), {"16": _P("paired", (0, True), (0, False), 130, 1), "32": _P("paired", (0, False), (0, False), 130, 1)}),
    # pair, tall shallow dX on 128-row tiles (16-bit); fp32 has no shallow form: tall deep, remapped to 64 rows
    ((8229, 24, 20), {"16": _P("paired", (1, True), (0, False), 256, 33), "32": _P("paired", (0, False), (0, False), 160, 52, 1)}),
    # pair, tall deep dX remapped to 64 rows (128 rows under WW_GEMM_PAIR_TALL=2); M N = 1 069 770 > 4096 x 256: k_linear_dpre's
    # second grid-stride trip.  (The issue's (8229, 130, 64) has M N = 526 656 and stays within one trip.)
    ((8229, 130, 130), {"16": _P("paired", (0, False), (0, False), 256, 33, 1), "32": _P("paired", (0, False), (0, False), 160, 52, 1)}),
    # refused: the dW side is shallow (M <= 32, 16-bit); fp32 pairs
    ((30, 70, 70), {"16": _P("dw_shallow", (0, False), (0, True), 30, 1), "32": _P("paired", (0, False), (0, False), 30, 1)}),
    ((1, 7, 3), {"16": _P("dw_shallow", (0, True), (0, True), 1, 1), "32": _P("paired", (0, False), (0, False), 1, 1)}),
    # refused: dX is cfg 2 (16-bit; dW 8 splits through launch_gemm); fp32 pairs with 13 splits
    ((1930, 1930, 72), {"16": _P("dx_cfg2", (2, False), (0, False), 256, 8), "32": _P("paired", (0, False), (0, False), 160, 13)}),
    # refused: dW is cfg 2 with 2 splits (16-bit); fp32 pairs.  N K = 2 100 000 > 2048 x 1024: k_splitk_sum's second trip
    ((256, 1400, 1500), {"16": _P("dw_tile", (0, False), (2, False), 128, 2), "32": _P("paired", (0, False), (0, False), 128, 2)}),
    # refused: dW is cfg 1 (N >= 8192), in every mode; 16-bit: the shallow 128-row form of the transposed dW product
    ((20, 8, 8200), {"16": _P("dw_tile", (0, False), (1, True), 20, 1), "32": _P("dw_tile", (0, False), (1, False), 20, 1)}),
]
# dW alone (need_dx = False) through launch_gemm, immediate and deferred; and base pointers 4 bytes off the 16-byte grid: the
# Python wrapper passes a contiguous tensor's data pointer on as it is (it copies only what is not contiguous), so a view into a
# larger buffer reaches the kernels misaligned -> every vec flag 0 although the leading dimensions are multiples of 4
NO_DX_CASE = (257, 33, 71)
UNALIGNED_CASE = (257, 200, 72)
UNALIGNED_PLAN = {"16": _P("paired", (0, False), (0, False), 256, 2), "32": _P("paired", (0, False), (0, False), 160, 2)}
TALL2_CASES = [(257, 33, 71), (8229, 130, 130)]          # run in a child process under WW_GEMM_PAIR_TALL=2
# k_gemm_pair<MODE, TMX, KSX> reachable with the default environment, as (mode class, dX cfg, dX shallow)
PAIR_REACHABLE = {("16", 0, False), ("16", 0, True), ("16", 1, True), ("32", 0, False)}
REFUSALS_REACHABLE = {"dx_cfg2", "dw_tile", "dw_shallow", "no_dx"}      # "off" / "tall_off" need WW_GEMM_PAIR=0 / WW_GEMM_PAIR_TALL=0

# What the docstring of test_linear_mfma.py::test_linear_fwd_bwd_matches_torch used to claim its shapes reach in the 16-bit modes,
# as data: shape -> (forward fields, backward fields) of ww_gemm_plan.  All of it held when it was first asked of the query.
LEGACY_CLAIMS = {
    (4096, 64, 1024): (dict(cfg=2), dict(refused="paired", nz=32)),
    (2048, 576, 1024): ({}, dict(refused="dw_tile", dw_cfg=2, nz=8, splitk_sum=1, dx_cfg=0)),
    (8192, 200, 64): (dict(cfg=1, shallow=0), dict(refused="paired", dx_cfg_plain=1, dx_cfg=0, dx_shallow=0, nz=64)),
    (8192, 24, 20): (dict(cfg=1, shallow=1), dict(refused="paired", dx_cfg=1, dx_shallow=1, nz=64)),
    (1, 7, 3): (dict(cfg=0, shallow=1, vecA=0, vecB=0), dict(refused="dw_shallow", dx_cfg=0, dx_shallow=1, dw_cfg=0, dw_shallow=1)),
    (300, 30, 300): (dict(cfg=0, shallow=1, vecA=0, vecB=0), dict(refused="paired", nz=2, dw_vecB=0, dx_vecB=0)),
    (130, 40, 2): ({}, dict(refused="paired", dx_shallow=1, dx_vecA=0, dw_vecA=0)),
    (200, 1024, 2): ({}, dict(refused="paired", dx_shallow=1, dx_vecA=0, dw_vecA=0)),
    (77, 576, 1024): ({}, dict(refused="paired", dx_cfg=0, dw_cfg=0, nz=1)),
    (64, 64, 64): ({}, dict(refused="paired", dx_cfg=0, dw_cfg=0, nz=1)),
}

mode_class = lambda mode: "32" if mode == "fp32" else "16"
cdiv = lambda a, b: -(-a // b)
shape_id = lambda s: "x".join(map(str, s[0] if isinstance(s[0], tuple) else s))


def expect_fwd_plan(shape, want, mode, epi, aligned=True):
    """the GEMM_PLAN_FWD dict ww_gemm_plan(which = 0) must return for a FWD_CASES entry"""
    M, K, N = shape
    cfg = want["cfg"][2] if mode == "fp32" else want["cfg"][0 if epi == 2 else 1]
    shallow = int(want["shallow16"] and mode != "fp32")
    stage = 32 if mode == "fp32" or shallow else (64 if cfg == 2 else 128)
    vec = int(bool(want["vec"]) and aligned)
    return dict(epi=epi, cfg=cfg, shallow=shallow, stage_k=stage, vecA=vec, vecB=vec, gx=cdiv(N, 128 if cfg == 2 else 64),
                gy=cdiv(M, 128 if cfg else 64), gz=1)


def expect_bwd_plan(shape, want, mode, full_epilogue, need_dx=True, aligned=True):
    """the fields of GEMM_PLAN_BWD a BWD_CASES entry fixes (the environment read-backs aside)"""
    M, K, N = shape
    w = want[mode_class(mode)]
    refused = w["refused"] if need_dx else "no_dx"
    (dxc, dxs), (dwc, dws) = w["dx"], w["dw"]
    nbx = cdiv(K, 128 if dxc == 2 else 64) * cdiv(M, 128 if dxc else 64) if need_dx else 0
    nbw = cdiv(K, 128 if dwc == 2 else 64) * cdiv(N, 128 if dwc else 64) * w["nz"]
    v = lambda ld: int(aligned and ld % 4 == 0)
    return dict(dpre=int(full_epilogue), dpre_grid=min(cdiv(M * N, 256), 4096) if full_epilogue else 0, paired=int(refused == "paired"),
                refused=refused, dx_cfg=dxc, dx_shallow=int(dxs), dw_cfg=dwc, dw_shallow=int(dws), kps=w["kps"], nz=w["nz"], nbw=nbw, nbx=nbx,
                splitk_sum=int(w["nz"] > 1), splitk_grid=min((N * K // 4 + 255) // 256 + 1, 2048) if w["nz"] > 1 else 0,
                dx_cfg_plain=w["dx_plain"], dx_vecA=v(N), dx_vecB=v(K), dw_vecA=v(N), dw_vecB=v(K), db_grid=cdiv(N, 64))
