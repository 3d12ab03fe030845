"""16-bit activation storage of the native Conv2d path and ResNet18Wakeword, without a GPU: the constructor's ``storage`` argument,
the C-ABI's new entry points, the float64 restatement (tests/resnet_storage_cases.py) and the exactness conditions of the integer
layer cases that test_resnet_storage_gpu.py runs on the device."""
import re
from pathlib import Path

import pytest
import torch

from tests.resnet_cases import ResNetRestated, golden_case, layer_case, layer_inputs
from tests.resnet_storage_cases import ST_NAMES, ST_SHAPES, ResNetStorageRestated

REPO = Path(__file__).resolve().parents[1]


def test_constructor_takes_and_validates_storage():
    from wakeword_trainer_home_amd.models import ResNet18Wakeword
    from wakeword_trainer_home_amd.models.resnet import BasicBlock, NativeConv2d
    base = ResNet18Wakeword(dropout=0.0)
    assert base.resnet.storage is torch.float32 and all(b.storage is torch.float32 for b in base.modules() if isinstance(b, BasicBlock))
    for mode, dt in (("bf16", torch.bfloat16), ("fp16", torch.float16)):
        m = ResNet18Wakeword(dropout=0.0, mode=mode, storage=mode)
        assert list(m.state_dict()) == list(base.state_dict())
        assert all(p.dtype is torch.float32 for p in m.parameters()) and all(b.dtype is not dt for b in m.buffers())
        assert [tuple(p.shape) for p in m.parameters()] == [tuple(p.shape) for p in base.parameters()]
        assert m.resnet.storage is dt and all(b.storage is dt and b.mode is dt for b in m.modules() if isinstance(b, BasicBlock))
        assert ResNet18Wakeword(mode=mode, storage="fp32").resnet.storage is torch.float32      # the matrix modes of today
        assert BasicBlock(64, 128, 2, mode, mode).storage is dt and NativeConv2d(8, 16, 3, 1, mode, mode).storage is dt
        assert BasicBlock(64, 128, 2, dt, dt).storage is dt
    # a 16-bit storage with fp32 matrices, a storage that is not the matrix mode, an unknown storage
    for ctor in (lambda **kw: ResNet18Wakeword(**kw), lambda **kw: BasicBlock(64, 64, 1, **kw), lambda **kw: NativeConv2d(8, 8, 3, 1, **kw)):
        for kw in (dict(mode="fp32", storage="bf16"), dict(mode="fp32", storage="fp16"), dict(mode="bf16", storage="fp16"),
                   dict(mode="fp16", storage="bf16"), dict(mode="bf16", storage="int8")):
            with pytest.raises(ValueError, match="storage"):
                ctor(**kw)


def test_initialisation_does_not_depend_on_storage():
    from wakeword_trainer_home_amd.models import ResNet18Wakeword
    torch.manual_seed(3)
    a = ResNet18Wakeword(dropout=0.0).state_dict()
    torch.manual_seed(3)
    b = ResNet18Wakeword(dropout=0.0, mode="bf16", storage="bf16").state_dict()
    assert all(torch.equal(a[k], b[k]) for k in a)


def test_factory_still_refuses_resnet18():
    from wakeword_trainer_home_amd.models import create_model
    with pytest.raises(ValueError, match="outside this build"):
        create_model("resnet18")


def test_header_library_and_binding_carry_the_storage_entry_points():
    from wakeword_trainer_home_amd import _native as nat
    header = (REPO / "include" / "wwhip.h").read_text()
    declared = set(re.findall(r"\b(ww_[a-z0-9_]+)\s*\(", header))
    lib = nat.load()
    for name in ST_NAMES:
        assert name in declared and name in nat.EXPORTS and hasattr(lib, name), name
    assert nat.ABI_VERSION == 17 and re.search(r"#define WW_ABI_VERSION 17\b", header) and lib.ww_abi_version() == 17
    # the scratch size is host arithmetic: packed 16-bit weights + fp32 partials; 0 for the shapes the kernels refuse
    assert lib.ww_conv2d_st_scratch_bytes(2, 5, 7, 8, 16, 3, 2) >= 9 * 8 * 16 * (2 + 4)
    for bad in ((2, 5, 7, 4, 16, 3, 1), (2, 5, 7, 8, 12, 3, 1), (2, 5, 7, 8, 16, 2, 1), (2, 5, 7, 8, 16, 3, 3), (0, 5, 7, 8, 16, 3, 1)):
        assert lib.ww_conv2d_st_scratch_bytes(*bad) == 0, bad


def test_trainer_graph_key_names_the_storage():
    from wakeword_trainer_home_amd.models import ResNet18Wakeword
    from wakeword_trainer_home_amd.training import Trainer
    key = lambda **kw: Trainer._graph_mode_key(type("T", (), {"model": ResNet18Wakeword(**kw)})())
    assert key(mode="bf16") != key(mode="bf16", storage="bf16") != key(mode="fp16", storage="fp16")
    assert key() == key(storage="fp32")


def test_restatement_without_storage_is_the_parent_bit_for_bit():
    sd, g = golden_case()
    x, y = torch.from_numpy(g["x"]).double(), torch.from_numpy(g["y"])
    a, b = ResNetRestated(sd), ResNetStorageRestated(sd, st=None)
    la, lossa, ga = a.loss_and_grads(x, y)
    lb, lossb, gb = b.loss_and_grads(x, y)
    assert torch.equal(la, lb) and lossa == lossb and all(torch.equal(ga[k], gb[k]) for k in ga)
    assert all(torch.equal(a.sd[k], b.sd[k]) for k in a.sd) and all(torch.equal(p, q) for p, q in zip(a.pres, b.pres))


@pytest.mark.parametrize("st", [torch.bfloat16, torch.float16])
def test_restatement_rounds_values_and_gradients_at_the_storage_points(st):
    """One downsample block: every stored activation is a value of S, and so are the gradients that reach the block's input and its
    stored intermediates (hooks on the graph)."""
    from tests.resnet_storage_cases import basic_block_st
    g = torch.Generator().manual_seed(4)
    rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    sd = {"b.conv1.weight": rn(16, 8, 3, 3) * 0.1, "b.conv2.weight": rn(16, 16, 3, 3) * 0.1, "b.downsample.0.weight": rn(16, 8, 1, 1) * 0.3}
    for bn in ("bn1.", "bn2.", "downsample.1."):
        sd.update({"b." + bn + "weight": rn(16).abs() + 0.5, "b." + bn + "bias": rn(16) * 0.1, "b." + bn + "running_mean": torch.zeros(16, dtype=torch.float64),
                   "b." + bn + "running_var": torch.ones(16, dtype=torch.float64)})
    is_s = lambda t: torch.equal(t.float().to(st).double(), t)
    x = rn(2, 6, 5, 8).float().to(st).double().requires_grad_(True)
    seen = {}
    out = basic_block_st(x, sd, "b.", 2, True, st)
    node = out.grad_fn                       # the _Store of the block's output: the gradient it hands on is a value of S
    node.register_hook(lambda gin, gout: seen.update(dout=gin[0].clone()))
    assert is_s(out.detach()) and not is_s(out.detach() * 1.001)
    (out * rn(*out.shape)).sum().backward()
    assert is_s(seen["dout"]) and x.grad.abs().max() > 0
    exact = basic_block_st(x.detach(), sd, "b.", 2, True, None)
    assert not torch.equal(exact, out.detach()) and not is_s(exact)


@pytest.mark.parametrize("shape", ST_SHAPES, ids=["-".join(map(str, s)) for s in ST_SHAPES])
def test_integer_layer_cases_are_exact_in_fp32(shape):
    """The conditions under which the device must return S(exact) bit for bit: on the integer inputs every sum of |a b| stays at or
    below 4608 * 8 < 2^24, so fp32 accumulation in any order is exact and the one rounding to S is all that happens -- for dx also
    after the +3 of the accumulate case.  fp16 holds the results (65504 > 4608 * 8), and some of them do need the rounding."""
    d_in = layer_inputs(*shape, seed=sum(shape) + 17, integer=True)
    ref = layer_case(d_in["x"], d_in["w"], d_in["dy"], shape[6])
    for n in ("y", "dx", "dw"):
        assert ref[n + "_abs"].max().item() + 3 <= 4608 * 8 < 2 ** 24, n
        assert torch.equal(ref[n], ref[n].round())
    for n in ("x", "dy"):          # the inputs themselves are values of both storage types
        assert torch.equal(d_in[n].float().to(torch.bfloat16).double(), d_in[n]) and torch.equal(d_in[n].half().double(), d_in[n])
    if shape[3] * shape[5] ** 2 >= 576:                # K >= 576: some outputs exceed bf16's 8 bits and are rounded
        assert not torch.equal(ref["y"].float().to(torch.bfloat16).double(), ref["y"])
