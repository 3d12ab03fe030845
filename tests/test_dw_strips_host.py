"""CPU: the dispatch of the depthwise kernels, asked of the code that launches (ww_dw_plan runs the launchers' own functions), and the
integer-exactness of the cases test_dw_strips_gpu.py runs.  A changed dispatch rule -- what counts as interior, which tensors
take the scalar-base address form -- shows up here, without a device."""
import re
from pathlib import Path

import pytest
import torch

from tests import conv_trip_cases as K
from tests import dw_strip_cases as D

REPO = Path(__file__).resolve().parents[1]


@pytest.fixture(scope="module")
def nat():
    from wakeword_trainer_home_amd import _native
    _native.load()
    return _native


@pytest.mark.parametrize("shape", D.SHAPES, ids=D.shape_id)
def test_each_case_reaches_the_body_it_claims(nat, shape):
    for dname, dt in D.ACTS.items():
        p = nat.plan_dw_strips(*shape, dt)
        assert (p["ncs"], p["nseg"], p["hs_len"], p["items"]) == D.GEOMETRY[shape], (dname, p)
        assert (p["ncs"], p["nseg"], p["hs_len"]) == K.dw_geometry(shape[1], shape[2])
        assert (p["waves"], p["interior_waves"]) == D.EXPECT[shape], (dname, p)
        assert p["addr_bits"] == 32, (dname, p)


def test_interior_rule_by_hand(nat):
    """interior <=> cs >= 1 and 4 cs + 5 <= W, and a wave needs both of items 2k, 2k + 1: counted here from the rule alone"""
    for B, H, W in [(1, 3, 13), (1, 3, 12), (4, 2, 76), (3, 45, 33), (5, 20, 9), (2, 1, 100)]:
        ncs, nseg, _ = K.dw_geometry(H, W)
        items = B * nseg * ncs
        inner = lambda it: it % ncs >= 1 and 4 * (it % ncs) + 5 <= W
        want = sum(inner(e) and inner(e + 1) for e in range(0, items - 1, 2))
        p = nat.plan_dw_strips(B, H, W, torch.bfloat16)
        assert (p["items"], p["waves"], p["interior_waves"]) == (items, (items + 1) // 2, want), (B, H, W, p)
    # the boundary of the rule: strip 3 needs column 4 * 3 + 4 = 16 as its right halo, so W = 17 is the first width with pair (2, 3)
    assert nat.plan_dw_strips(1, 3, 17, torch.float32)["interior_waves"] == 1
    assert nat.plan_dw_strips(1, 3, 16, torch.float32)["interior_waves"] == 0


def test_address_form_follows_the_byte_size_and_the_switch(nat):
    for dt in D.ACTS.values():
        forced = nat.plan_dw_strips(*D.WIDE_SHAPE, dt, wide=True)
        assert forced["addr_bits"] == 64 and forced["interior_waves"] == 0 and forced["waves"] == D.EXPECT[D.WIDE_SHAPE][0]
    # B * 20 * 76 * 64 elements: fp32 crosses 2^32 bytes between B = 11037 and 11038, the 16-bit types between 22075 and 22076
    assert nat.plan_dw_strips(11037, 20, 76, torch.float32)["addr_bits"] == 32
    assert nat.plan_dw_strips(11038, 20, 76, torch.float32)["addr_bits"] == 64
    assert nat.plan_dw_strips(11038, 20, 76, torch.bfloat16)["addr_bits"] == 32
    assert nat.plan_dw_strips(22075, 20, 76, torch.float16)["addr_bits"] == 32
    assert nat.plan_dw_strips(22076, 20, 76, torch.float16)["addr_bits"] == 64
    assert nat.plan_dw_strips(22076, 20, 76, torch.float16)["interior_waves"] == 0
    big = nat.plan_dw_strips(512, 20, 76, torch.bfloat16)                     # the benchmark's layer: 16 of every 19 waves are interior
    assert (big["items"], big["waves"], big["interior_waves"], big["addr_bits"]) == (9728, 4864, 4096, 32)


def test_plan_argument_checks(nat):
    import ctypes as C
    lib, out = nat.load(), (C.c_long * 7)()
    assert lib.ww_dw_plan(0, 1, 1, 0, 0, out) == -1 and b"ww_dw_plan" in lib.ww_last_error()
    assert lib.ww_dw_plan(1, 1, 1, 3, 0, out) == -1 and b"act_dtype" in lib.ww_last_error()
    assert lib.ww_dw_plan(1, 1, 1, 0, 2, out) == -1 and lib.ww_dw_plan(1, 1, 1, 0, 0, None) == -1
    assert lib.ww_dw_plan(1, 1, 1, 0, 0, out) == 0 and list(out) == [1, 1, 1, 1, 1, 0, 32]


def test_header_and_bindings_declare_the_query_and_the_switch(nat):
    header = (REPO / "include" / "wwhip.h").read_text()
    assert re.search(r"\bint ww_dw_plan\(int B, int H, int W, int act_dtype, int wide, long \*out\);", header)
    assert re.search(r"\bint ww_ctx_set_dw_wide_addr\(ww_ctx \*ctx, int on\);", header)
    lib = nat.load()
    for name in ("ww_dw_plan", "ww_ctx_set_dw_wide_addr"):
        assert name in nat.EXPORTS and hasattr(lib, name)
    assert callable(nat.set_dw_wide_addr) and callable(nat.plan_dw_strips)


@pytest.mark.parametrize("shape", D.SHAPES, ids=D.shape_id)
def test_cases_are_integer_exact(shape):
    """the builders assert both exactness conditions (conv_trip_cases.exactness); the references are shared with the GPU test"""
    c, ref = K.fwd_case("dw", shape)
    assert ref["y"].shape == (*shape, K.C) and torch.equal(ref["y"], ref["y"].round())
    c, ref = K.bwd_case("dw", shape, False)
    assert ref["g_in"].shape == (*shape, K.C) and ref["dw"].shape == (K.C, 1, 3, 3)
