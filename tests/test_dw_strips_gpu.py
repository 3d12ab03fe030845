"""GPU: the two bodies and the two address forms of the depthwise kernels (k_dw_fwd_sb / k_dw_bwd_sb: interior and edge body on a
scalar base with 32-bit lane offsets; k_dw_fwd / k_dw_bwd: one body, 64-bit lane addresses), on the shapes of
tests/dw_strip_cases.py -- its docstring says which wave of which shape takes which body, and test_dw_strips_host.py asserts it.

Integer-exact data (tests/conv_trip_cases.py): no operation rounds, in any order, so y, g_in, dW, dbeta_in and dgamma_in must
equal the float64 restatement bit for bit in fp32, bf16 and fp16 at every grid cap.  What the finalize kernels derive in double
from the exact partial sums and round to fp32 once -- ss, mr, the running statistics, coef_in -- is within 1 fp32 ulp of the float64
value (test_conv_trips_gpu.py's docstring has the argument; that file's checks are used as they are).  On top of that every
output, the derived ones included, must be bit-identical between the scalar-base form and the forced 64-bit form at the same cap:
the 64-bit form is the kernel as it was before the scalar-base form existed, the partial rows are the same rows, and so a
difference in any bit is a changed operation or operation order."""
import pytest
import torch

from tests import conv_trip_cases as K
from tests import dw_strip_cases as D
from tests.test_conv_trips_gpu import DEV, bits, bwd_inputs, check_bwd, check_fwd, fwd_inputs, run_bwd, run_fwd

pytestmark = pytest.mark.gpu
FWD_OUT = ("y", "ss", "mr", "running_mean", "running_var")
BWD_OUT = ("g_in", "dw", "coef_in", "dgamma", "dbeta")


@pytest.fixture(scope="module")
def nat():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from wakeword_trainer_home_amd import _native
    _native.load()
    return _native


def both_forms(nat, run, check, names, caps, tag):
    """run() under each cap in the scalar-base form, checked against the reference; then in the 64-bit form, checked too and
    bit-equal to the first in every output"""
    try:
        for cap in caps:
            nat.set_grid_cap(DEV, cap)
            nat.set_dw_wide_addr(DEV, False)
            out = run()
            check(out, f"{tag} cap {cap}")
            nat.set_dw_wide_addr(DEV, True)
            wide = run()
            check(wide, f"{tag} cap {cap} 64-bit form")
            for name in names:
                assert torch.equal(bits(out[name]), bits(wide[name])), f"{tag} cap {cap}: {name} differs between the address forms"
    finally:
        nat.set_grid_cap(DEV, 0)
        nat.set_dw_wide_addr(DEV, False)


@pytest.mark.parametrize("shape", D.SHAPES, ids=D.shape_id)
def test_forward_bodies_are_exact(nat, shape):
    c, ref = K.fwd_case("dw", shape)
    for dname, dt in D.ACTS.items():
        assert nat.plan_dw_strips(*shape, dt)["interior_waves"] == D.EXPECT[shape][1]
        d = fwd_inputs("dw", c, dt)
        both_forms(nat, lambda: run_fwd(nat, "dw", d, dt), lambda out, tag: check_fwd(out, ref, tag), FWD_OUT, D.caps(shape),
                   f"dw fwd {D.shape_id(shape)} {dname}")


@pytest.mark.parametrize("shape", D.SHAPES, ids=D.shape_id)
def test_backward_bodies_are_exact(nat, shape):
    c, ref = K.bwd_case("dw", shape, False)
    for dname, dt in D.ACTS.items():
        d = bwd_inputs("dw", c, dt)
        both_forms(nat, lambda: run_bwd(nat, "dw", d), lambda out, tag: check_bwd(out, ref, tag), BWD_OUT, D.caps(shape),
                   f"dw bwd {D.shape_id(shape)} {dname}")


def test_the_switch_takes_0_or_1(nat):
    lib = nat.load()
    assert lib.ww_ctx_set_dw_wide_addr(nat.ctx(DEV), 2) == -1 and b"must be 0 or 1" in lib.ww_last_error()
    assert lib.ww_ctx_set_dw_wide_addr(None, 0) == -1
    nat.set_dw_wide_addr(DEV, False)
