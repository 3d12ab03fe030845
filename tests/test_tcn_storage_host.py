"""16-bit activation storage of the causal Conv1d path and TCNWakeword, without a GPU: the constructors' ``storage`` argument, the
C-ABI's new entry points, the float64 restatement (tests/tcn_storage_cases.py) pinned to TCNRestated, and the exactness conditions
of the integer layer cases that test_tcn_storage_gpu.py runs on the device."""
import re
from pathlib import Path

import pytest
import torch

from tests.tcn_cases import TCNRestated, conv_bwd, conv_fwd, golden_case, layer_inputs
from tests.tcn_storage_cases import ST_NAMES, ST_SHAPES, TCNStorageRestated, st_layer

REPO = Path(__file__).resolve().parents[1]
_ST = [torch.bfloat16, torch.float16]
_CASES = [("", {}), ("small.", dict(num_channels=[32, 48], kernel_size=2))]


def _is_s(t, st):
    return torch.equal(t.float().to(st).double(), t)


def test_constructors_take_and_validate_storage():
    from wakeword_trainer_home_amd import _native as nat
    from wakeword_trainer_home_amd.models import TCNWakeword
    from wakeword_trainer_home_amd.models.tcn import NativeCausalConv1d, TemporalBlock, TemporalConvNet
    base = TCNWakeword(dropout=0.0)
    hip = lambda m: [c for c in m.modules() if isinstance(c, (NativeCausalConv1d, TemporalBlock, TemporalConvNet))]
    assert base.storage is torch.float32 and hip(base) and all(c.storage is torch.float32 for c in hip(base))
    for mode, dt in (("bf16", torch.bfloat16), ("fp16", torch.float16)):
        m = TCNWakeword(dropout=0.0, mode=mode, storage=mode)
        assert list(m.state_dict()) == list(base.state_dict())
        assert all(p.dtype is torch.float32 for p in m.parameters())
        assert [tuple(p.shape) for p in m.parameters()] == [tuple(p.shape) for p in base.parameters()]
        assert m.storage is dt and m.mode is dt and all(c.storage is dt and c.mode is dt for c in hip(m))
        fp = TCNWakeword(mode=mode, storage="fp32")                   # the matrix modes of today
        assert fp.storage is torch.float32 and all(c.storage is torch.float32 and c.mode is dt for c in hip(fp))
        assert NativeCausalConv1d(8, 16, 3, 2, mode=mode, storage=mode).storage is dt
        assert TemporalBlock(40, 64, 3, 1, mode=dt, storage=dt).storage is dt
        assert TemporalConvNet(mode=mode, storage=mode).storage is dt
        # a 16-byte access is 8 elements: channel counts that are multiples of 4 only
        for ctor in (lambda: NativeCausalConv1d(12, 16, 3, mode=mode, storage=mode), lambda: NativeCausalConv1d(16, 20, 3, mode=mode, storage=mode),
                     lambda: TemporalBlock(40, 36, 3, 1, mode=mode, storage=mode), lambda: TCNWakeword(input_size=44, mode=mode, storage=mode)):
            with pytest.raises(nat.NativeError, match="multiples of 8"):
                ctor()
        NativeCausalConv1d(12, 20, 3, mode=mode)                        # ... which fp32 storage still takes
    for ctor in (lambda **kw: TCNWakeword(**kw), lambda **kw: TemporalConvNet(**kw), lambda **kw: TemporalBlock(40, 64, 3, 1, **kw),
                 lambda **kw: NativeCausalConv1d(8, 8, 3, **kw)):
        for kw in (dict(mode="fp32", storage="bf16"), dict(mode="fp32", storage="fp16"), dict(mode="bf16", storage="fp16"),
                   dict(mode="fp16", storage="bf16"), dict(mode="bf16", storage="int8")):
            with pytest.raises(ValueError, match="storage"):
                ctor(**kw)


def test_initialisation_does_not_depend_on_storage():
    from wakeword_trainer_home_amd.models import TCNWakeword
    torch.manual_seed(3)
    a = TCNWakeword(dropout=0.0).state_dict()
    torch.manual_seed(3)
    b = TCNWakeword(dropout=0.0, mode="fp16", storage="fp16").state_dict()
    assert list(a) == list(b) and all(torch.equal(a[k], b[k]) and a[k].dtype is b[k].dtype for k in a)


def test_storage_helper_is_shared_with_resnet():
    from wakeword_trainer_home_amd.models import resnet, storage, tcn
    assert resnet._storage is storage._storage is tcn._storage


def test_header_library_and_binding_carry_the_storage_entry_points():
    from wakeword_trainer_home_amd import _native as nat
    header = (REPO / "include" / "wwhip.h").read_text()
    declared = set(re.findall(r"\b(ww_[a-z0-9_]+)\s*\(", header))
    lib = nat.load()
    for name in ST_NAMES:
        assert name in declared and name in nat.EXPORTS and hasattr(lib, name), name
    for name in ("tconv1d_st_fwd", "tconv1d_st_bwd", "dropout_bt_st", "add_relu_st_fwd", "seq_round_st"):
        assert callable(getattr(nat, name)), name
    assert nat.ABI_VERSION == 17 and re.search(r"#define WW_ABI_VERSION 17\b", header) and lib.ww_abi_version() == 17
    # the scratch size is host arithmetic: packed 16-bit weights + 16-bit dpre + fp32 partials; 0 for what the kernels refuse
    B, T, Cin, Cout, k = 2, 130, 128, 256, 3
    for code in (1, 2):
        assert lib.ww_tconv1d_st_scratch_bytes(code, B, T, Cin, Cout, k) >= k * Cin * Cout * (2 + 2 * 4) + B * T * Cout * 2
    for bad in ((0, B, T, Cin, Cout, k), (3, B, T, Cin, Cout, k), (1, B, T, 12, Cout, k), (1, B, T, Cin, 20, k), (1, B, T, Cin, Cout, 0),
                (1, B, T, Cin, Cout, 9), (1, 0, T, Cin, Cout, k)):
        assert lib.ww_tconv1d_st_scratch_bytes(*bad) == 0, bad


def test_trainer_graph_key_names_the_storage():
    from wakeword_trainer_home_amd.models import TCNWakeword
    from wakeword_trainer_home_amd.training import Trainer
    key = lambda **kw: Trainer._graph_mode_key(type("T", (), {"model": TCNWakeword(**kw)})())
    assert key(mode="bf16") != key(mode="bf16", storage="bf16") != key(mode="fp16", storage="fp16")
    assert key() == key(storage="fp32")


def test_factory_still_refuses_tcn():
    from wakeword_trainer_home_amd.models import create_model
    with pytest.raises(ValueError):
        create_model("tcn")


@pytest.mark.parametrize("prefix,kw", _CASES)
@pytest.mark.parametrize("dropout", [0.0, 0.3])
def test_restatement_without_storage_is_tcnrestated_bit_for_bit(prefix, kw, dropout):
    sd, g = golden_case(prefix)
    x, y = torch.from_numpy(g["x"]).double().transpose(1, 2), torch.from_numpy(g["y"])
    a, b = TCNRestated(sd, dropout=dropout, seed=4), TCNStorageRestated(sd, dropout=dropout, seed=4, st=None)
    la, lossa, ga, dxa = a.loss_and_grads(x, y, step=3, sample_offset=2)
    lb, lossb, gb, dxb = b.loss_and_grads(x, y, step=3, sample_offset=2)
    assert torch.equal(la, lb) and lossa == lossb and torch.equal(dxa, dxb)
    assert set(ga) == set(gb) and all(torch.equal(ga[k], gb[k]) for k in ga)
    if dropout == 0.0:            # ... and through it to the reference's own class
        assert (la - torch.from_numpy(g["logits_train"]).double()).abs().max().item() < 1e-6


@pytest.mark.parametrize("prefix,kw", _CASES)
@pytest.mark.parametrize("st", _ST, ids=["bf16", "fp16"])
def test_restatement_stores_values_of_the_storage_type(prefix, kw, st):
    """Every tensor the restatement marks as stored is a value of S (and was not before the rounding, where it was computed); the
    cost of the contract itself -- the restated storage logits and loss against the fixture's float64 ones -- is printed."""
    sd, g = golden_case(prefix)
    x, y = torch.from_numpy(g["x"]).double().transpose(1, 2), torch.from_numpy(g["y"])
    for dropout in (0.0, 0.3):
        r = TCNStorageRestated(sd, dropout=dropout, seed=1, st=st)
        logits, loss, grads, _ = r.loss_and_grads(x, y)
        assert len(r.stored) == 2 + 10 * r.n_blocks
        for name, (raw, stored) in r.stored.items():
            assert _is_s(stored, st), name
            assert torch.equal(stored, raw.float().to(st).double()), name
        assert not _is_s(r.stored["0.y1"][0], st) and not _is_s(r.stored["0.dh1"][0], st)
        assert all(torch.isfinite(v).all() for v in grads.values())
        if dropout == 0.0:
            print(f"tcn-storage restated '{prefix}' {st}: logits vs fixture {(logits - torch.from_numpy(g['logits_train']).double()).abs().max().item():.2e} "
                  f"loss {abs(loss - float(g['loss'])):.2e} (loss {loss:.6f})")


@pytest.mark.parametrize("shape", ST_SHAPES, ids=["-".join(map(str, s)) for s in ST_SHAPES])
def test_integer_layer_cases_are_exact_in_fp32(shape):
    """The premise of the device's bit-for-bit test: on the integer inputs every fp32 quantity the device forms -- the forward and dX
    accumulations with bias, residual and the 3s of the accumulate case, the dW and db sums over the stored values, also with the
    mask scale 2 -- stays below 2^24 in magnitude, so fp32 sums are exact in any order and the one rounding to S is all that happens.
    The inputs are values of both storage types; fp16 holds every result; bf16 has to round some (K = 768: sums of some 100 in standard deviation, a few of them odd and above 256)."""
    B, T, Cin, Cout, k, d = shape
    d_in = layer_inputs(B, T, Cin, Cout, k, seed=sum(shape) + 17, integer=True)
    ab = {n: v.abs() for n, v in d_in.items()}
    y_abs = conv_fwd(ab["x"], ab["w"], ab["b"], d) + ab["res"]
    dx_abs, dw_abs, db_abs = conv_bwd(ab["x"], ab["w"], 2.0 * ab["dy"], d)
    for n, v in (("y", y_abs), ("dx", dx_abs + 3.0), ("dw", dw_abs), ("db", db_abs)):
        assert v.max().item() < 2 ** 24 and v.max().item() <= 65504, n
    for n in ("x", "dy", "res"):
        assert all(_is_s(d_in[n], st) for st in _ST), n
    for st in _ST:
        r = st_layer(d_in["x"], d_in["w"], d_in["b"], d_in["dy"], d, st, relu=True, residual=d_in["res"])
        e = st_layer(d_in["x"], d_in["w"], d_in["b"], d_in["dy"], d, None, relu=True, residual=d_in["res"])
        assert torch.equal(r["pre"], e["pre"]) and torch.equal(r["y"], e["y"].float().to(st).double())     # W, x are values of S
        assert torch.equal(r["dw"], e["dw"]) and torch.equal(r["db"], e["db"]) and torch.equal(r["dx_raw"], e["dx_raw"])
    if k * Cin >= 768:
        y = st_layer(d_in["x"], d_in["w"], d_in["b"], d_in["dy"], d, None)["y"]
        assert not _is_s(y, torch.bfloat16) and _is_s(y, torch.float16)
