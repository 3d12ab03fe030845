"""Host side of the per-launch-path tests of the dense GEMM family (tests/gemm_cases.py, tests/test_gemm_paths_gpu.py); no GPU.

  * every integer-exact case meets its exactness conditions;
  * every case reaches, in every mode, exactly the plan the table lists for it, by ww_gemm_plan -- the launchers' own dispatch
    code -- and the table lists every outcome that code can produce with the default environment: a retuned gemm_tile_cfg,
    dw_splits or pair rule turns these red here, without a device, instead of leaving a path without a test;
  * what the docstring of test_linear_fwd_bwd_matches_torch claimed its shapes reach, asked of the same query;
  * the query's argument checks, its prototype in the header and its binding."""
import ctypes as C
import re
from pathlib import Path

import pytest
import torch

from tests import gemm_cases as G

REPO = Path(__file__).resolve().parents[1]


@pytest.fixture(scope="module")
def nat():
    from wakeword_trainer_home_amd import _native
    _native.load()
    return _native


def _sub(plan, want):
    return {k: plan[k] for k in want}


ALL_BWD_SHAPES = [s for s, _ in G.BWD_CASES] + [G.UNALIGNED_CASE]


@pytest.mark.parametrize("shape", sorted({s for s, _ in G.FWD_CASES} | set(ALL_BWD_SHAPES)), ids=G.shape_id)
def test_cases_are_integer_exact(shape):
    G.exactness(*shape)
    x, w, b, dy = G.exact_operands(*shape)
    if min(shape) >= 20:               # the patterns are not degenerate: the products use most of their range
        assert (x @ w.t()).unique().numel() > 8 and (dy.t() @ x).unique().numel() > 8


@pytest.mark.parametrize("case", G.FWD_CASES, ids=G.shape_id)
def test_forward_cases_reach_the_plan_they_list(nat, case):
    shape, want = case
    for mode, dt in G.MODES.items():
        for epi in (2, 1):
            for aligned in (True, False):
                got = nat.plan_gemm("fwd", *shape, mode=dt, full_epilogue=epi == 1, aligned=aligned)
                assert got == G.expect_fwd_plan(shape, want, mode, epi, aligned), (shape, mode, epi, aligned, got)


@pytest.mark.parametrize("case", G.BWD_CASES + [(G.UNALIGNED_CASE, G.UNALIGNED_PLAN)], ids=G.shape_id)
def test_backward_cases_reach_the_plan_they_list(nat, case):
    shape, want = case
    for mode, dt in G.MODES.items():
        for full in (False, True):
            for need_dx in (True, False):
                for aligned in (True, False):
                    got = nat.plan_gemm("bwd", *shape, mode=dt, full_epilogue=full, need_dx=need_dx, aligned=aligned)
                    exp = G.expect_bwd_plan(shape, want, mode, full, need_dx, aligned)
                    assert _sub(got, exp) == exp, (shape, mode, full, need_dx, aligned, got)
                    assert (got["env_pair"], got["env_pair_tall"], got["dw_min_rows"]) == (1, 1, 128)      # the defaults, as read


def test_the_table_lists_every_outcome_of_the_dispatch(nat):
    """conversely: every launch line of launch_gemm under EPI 1 / EPI 2, every k_gemm_pair instantiation and every refusal rule
    that the default environment can reach, one and several K splits, k_splitk_sum with one and with two grid-stride trips,
    k_linear_dpre with one and with two -- each is the listed plan of at least one case"""
    fwd = {}
    for shape, want in G.FWD_CASES:
        for mode, dt in G.MODES.items():
            for epi in (2, 1):
                p = nat.plan_gemm("fwd", *shape, mode=dt, full_epilogue=epi == 1)
                fwd.setdefault((G.mode_class(mode), epi), set()).add((p["cfg"], bool(p["shallow"])))
    assert fwd == G.FWD_REACHABLE, fwd
    pairs, refusals, nzs, sum_trips, dpre_trips = set(), set(), set(), set(), set()
    for shape, want in G.BWD_CASES:
        M, K, N = shape
        for mode, dt in G.MODES.items():
            p = nat.plan_gemm("bwd", *shape, mode=dt, full_epilogue=True)
            if p["paired"]:
                pairs.add((G.mode_class(mode), p["dx_cfg"], bool(p["dx_shallow"])))
            refusals.add(p["refused"])
            nzs.add(min(p["nz"], 2))
            if p["splitk_sum"]:
                sum_trips.add(min(G.cdiv(N * K, p["splitk_grid"] * 1024), 2))
            dpre_trips.add(min(G.cdiv(M * N, p["dpre_grid"] * 256), 2))
    refusals.add(nat.plan_gemm("bwd", *G.NO_DX_CASE, need_dx=False)["refused"])
    assert pairs == G.PAIR_REACHABLE, pairs
    assert refusals == G.REFUSALS_REACHABLE | {"paired"}, refusals
    assert nzs == {1, 2} and sum_trips == {1, 2} and dpre_trips == {1, 2}, (nzs, sum_trips, dpre_trips)
    # the scalar tail of k_splitk_sum (N K % 4 != 0) and partials off the 16-byte grid (M N % 4 != 0), on a case with splits
    M, K, N = G.NO_DX_CASE
    assert (N * K) % 4 == 3 and (M * N) % 2 == 1 and nat.plan_gemm("bwd", M, K, N)["nz"] == 2
    assert nat.plan_gemm("bwd", M, K, N, mode=torch.bfloat16)["kps"] == M - 1       # 16-bit: the last split is one row
    # db (k_colsum_any: 16 row parts, 64 columns per workgroup): rows no multiple of 16 and N no multiple of 64 are in the table
    assert any(M % 16 and N % 64 and N > 64 for (M, K, N), _ in G.BWD_CASES)
    # the tall cases that WW_GEMM_PAIR_TALL=2 turns into 128-row pairs: tall and deep in every mode for one of them
    assert any(all(nat.plan_gemm("bwd", *s, mode=dt)["dx_cfg_plain"] == 1 and not nat.plan_gemm("bwd", *s, mode=dt)["dx_shallow"]
                   for dt in G.MODES.values()) for s in G.TALL2_CASES)


@pytest.mark.parametrize("shape", list(G.LEGACY_CLAIMS), ids=G.shape_id)
def test_what_the_older_linear_test_reaches(nat, shape):
    """the shape list of test_linear_mfma.py::test_linear_fwd_bwd_matches_torch (its calls: bias only -> EPI 2; no activation)"""
    fwd, bwd = G.LEGACY_CLAIMS[shape]
    for dt in (torch.bfloat16, torch.float16):
        assert _sub(nat.plan_gemm("fwd", *shape, mode=dt), fwd) == fwd, (shape, dt)
        assert _sub(nat.plan_gemm("bwd", *shape, mode=dt), bwd) == bwd, (shape, dt, nat.plan_gemm("bwd", *shape, mode=dt))


def test_plan_rules_at_their_thresholds(nat):
    p = lambda *a, **k: nat.plan_gemm(*a, **k)
    bf = torch.bfloat16
    # 128 x 128 tiles from 256 of them on: 16 x 16 tiles of 128 rows is the first square count
    assert p("fwd", 1930, 72, 1930, mode=bf)["cfg"] == 2 and p("fwd", 1920, 72, 1920, mode=bf)["cfg"] == 0       # 15 x 15
    assert p("fwd", 8192, 40, 70, mode=bf)["cfg"] == 1 and p("fwd", 8191, 40, 70, mode=bf)["cfg"] == 0
    assert p("fwd", 130, 32, 70, mode=bf)["shallow"] == 1 and p("fwd", 130, 33, 70, mode=bf)["shallow"] == 0
    assert p("bwd", 32, 70, 70, mode=bf)["refused"] == "dw_shallow" and p("bwd", 33, 70, 70, mode=bf)["refused"] == "paired"
    assert p("bwd", 255, 33, 71)["nz"] == 1 and p("bwd", 256, 33, 71)["nz"] == 2              # dw_splits: M / 128 rows per split
    assert p("bwd", 1 << 20, 8, 8)["splits"] == 256                                            # and its cap


def test_plan_argument_checks(nat):
    lib, out = nat.load(), (C.c_long * 24)()
    ok = (0, 0, 4, 4, 4, 0, 1, 1)
    assert lib.ww_gemm_plan(*ok, out) == 0
    for i, bad in ((0, 2), (0, -1), (1, 3), (2, 0), (3, 0), (4, -5), (5, 2), (6, 2), (7, -1)):
        args = list(ok)
        args[i] = bad
        assert lib.ww_gemm_plan(*args, out) == -1 and b"ww_gemm_plan" in lib.ww_last_error(), (i, bad)
    assert lib.ww_gemm_plan(*ok, None) == -1
    with pytest.raises(ValueError):
        nat.plan_gemm("bwd", 0, 4, 4)


def test_header_and_bindings_declare_the_query(nat):
    header = (REPO / "include" / "wwhip.h").read_text()
    assert re.search(r"\bint ww_gemm_plan\(int which, int mode, int M, int K, int N, int full_epilogue, int aligned, int need_dx, "
                     r"long \*out\);", header)
    for i, name in enumerate(nat.PAIR_REFUSALS):
        macro = "WW_PAIR_OK" if name == "paired" else "WW_PAIR_" + name.upper()
        assert re.search(rf"#define {macro} {i}\b", header), macro
    assert "ww_gemm_plan" in nat.EXPORTS and hasattr(nat.load(), "ww_gemm_plan") and callable(nat.plan_gemm)
    assert len(nat.GEMM_PLAN_BWD) == 24 and len(nat.GEMM_PLAN_FWD) == 9
    assert nat.ABI_VERSION == 17 and re.search(r"#define WW_ABI_VERSION 17\b", header)
