"""TCNWakeword without a GPU: constructor, state dict, input orientation, and the float64 restatement (tests/tcn_cases.py) pinned
to the reference's own TCNWakeword through tests/golden/g10_tcn.npz (make_golden_tcn.py)."""
import re
from pathlib import Path

import numpy as np
import pytest
import torch

from tests.tcn_cases import GOLDEN, TCNRestated, golden_case, sampled_rel

REPO = Path(__file__).resolve().parents[1]
_CASES = [("", {}), ("small.", dict(num_channels=[32, 48], kernel_size=2))]


def test_constructor_defaults_are_the_reference_ones():
    from wakeword_trainer_home_amd.models import TCNWakeword
    from wakeword_trainer_home_amd.models.architectures import TCNWakeword as FromArch
    from wakeword_trainer_home_amd.models.flat_buckets import FlatBuckets
    assert FromArch is TCNWakeword and issubclass(TCNWakeword, FlatBuckets)
    m = TCNWakeword()
    blocks = list(m.tcn.network)
    assert m.input_size == 40 and len(blocks) == 3
    assert [(b.conv1.in_channels, b.conv1.out_channels, b.conv1.kernel_size, b.dilation) for b in blocks] == \
        [(40, 64, 3, 1), (64, 128, 3, 2), (128, 256, 3, 4)]
    assert all(b.conv2.in_channels == b.conv2.out_channels == b.conv1.out_channels and b.conv2.dilation == b.dilation for b in blocks)
    assert all(b.downsample.kernel_size == 1 and b.downsample.dilation == 1 for b in blocks)
    assert all(b.dropout == pytest.approx(0.3) for b in blocks) and m.fc[2].p == pytest.approx(0.3)
    assert [b.stream_ids for b in blocks] == [(16, 17), (18, 19), (20, 21)]
    assert m.tcn.dropout_seed == 0 and blocks[0].mode == torch.float32 and m.fc[3].mode == torch.float32 and m.hip_backed
    assert m.fc[3].weight.shape == (2, 256)
    assert TCNWakeword(num_channels=[64, 64]).tcn.network[1].downsample is None           # equal channel counts: identity skip
    assert TCNWakeword(mode="bf16", dropout_seed=5).tcn.network[2].conv2.mode == torch.bfloat16
    bound = (40 * 3) ** -0.5                                         # nn.Conv1d.reset_parameters: U(-1/sqrt(Cin k), 1/sqrt(Cin k))
    assert m.tcn.network[0].conv1.weight.abs().max().item() <= bound and m.tcn.network[0].conv1.bias.abs().max().item() <= bound


@pytest.mark.parametrize("prefix,kw", _CASES)
def test_state_dict_matches_reference_fixture(prefix, kw):
    from wakeword_trainer_home_amd.models import TCNWakeword
    sd, g = golden_case(prefix)
    m = TCNWakeword(dropout=0.0, **kw)
    assert list(m.state_dict().keys()) == g["keys"]
    assert all(tuple(v.shape) == tuple(g["shapes"][k]) for k, v in m.state_dict().items())
    m.load_state_dict(sd)
    assert all(torch.equal(v, sd[k]) for k, v in m.state_dict().items())
    if not prefix:
        assert len(g["keys"]) == 20 and g["keys"][0] == "tcn.network.0.conv1.weight" and g["keys"][-2:] == ["fc.3.weight", "fc.3.bias"]
        assert tuple(g["shapes"]["tcn.network.0.conv1.weight"]) == (64, 40, 3)
        assert tuple(g["shapes"]["tcn.network.2.downsample.weight"]) == (256, 128, 1)


def test_fixture_keeps_the_margin_its_generator_searched_for():
    g = np.load(GOLDEN)
    for prefix in ("", "small."):
        assert float(g[prefix + "relu_margin"]) >= 1e-6 and float(g[prefix + "grad_agreement"]) <= 1e-5
        assert int(g[prefix + "param_seed"]) >= 0


@pytest.mark.parametrize("prefix,kw", _CASES)
def test_float64_restatement_matches_reference_fixture(prefix, kw):
    """The float64 model the GPU tests compare with (TCNRestated: causal convolutions on (B,T,C), masks from the saved signs) is
    the reference's TCNWakeword: logits <= 1e-5, loss <= 1e-6, sampled parameter gradients <= 1e-5 of their largest entry."""
    sd, g = golden_case(prefix)
    oracle = TCNRestated(sd)
    x, y = torch.from_numpy(g["x"]).double().transpose(1, 2), torch.from_numpy(g["y"])
    ev = oracle.forward(x, training=False)
    assert (ev - torch.from_numpy(g["logits_eval"]).double()).abs().max().item() <= 1e-5
    out, loss, grads, _ = oracle.loss_and_grads(x, y)
    assert (out - torch.from_numpy(g["logits_train"]).double()).abs().max().item() <= 1e-5
    assert abs(loss - float(g["loss"])) <= 1e-6
    assert sorted(grads) == sorted(g["gsamp"])
    for n, gr in grads.items():
        assert tuple(gr.shape) == tuple(g["shapes"][n]), n
        assert sampled_rel(gr, g, n) <= 1e-5, n
    # the restatement sees the margin the generator stored: no ReLU input of the float64 run is closer to zero
    assert len(oracle.relu_masks) == 3 * oracle.n_blocks


def test_restatement_reads_the_public_forward_orientations_as_the_reference_does():
    """(4,37,40) is (B,T,F) (the reference transposes it); the square (2,40,40) is (B,F,T) (the reference does not)."""
    from wakeword_trainer_home_amd.models import TCNWakeword
    sd, _ = golden_case("")
    g = np.load(GOLDEN)
    oracle, m = TCNRestated(sd), TCNWakeword()
    for name in ("btf", "sq"):
        x = torch.from_numpy(g[f"fwd.x_{name}"])
        seq = m._sequence(x)
        assert tuple(seq.shape) == ((4, 37, 40) if name == "btf" else (2, 40, 40))
        assert torch.equal(seq, x if name == "btf" else x.transpose(1, 2))
        ev = oracle.forward(seq.double(), training=False)
        assert (ev - torch.from_numpy(g[f"fwd.logits_{name}"]).double()).abs().max().item() <= 1e-5, name


def test_input_orientation_rule():
    from wakeword_trainer_home_amd.models import TCNWakeword
    m = TCNWakeword()
    z = torch.zeros
    assert tuple(m._sequence(z(3, 1, 40, 151)).shape) == (3, 151, 40)         # the Trainer's feature batches
    assert tuple(m._sequence(z(3, 151, 40)).shape) == (3, 151, 40)            # only size(2) == input_size: (B,T,F)
    assert tuple(m._sequence(z(3, 40, 151)).shape) == (3, 151, 40)            # size(1) == input_size: (B,F,T)
    x = torch.arange(2 * 40 * 40, dtype=torch.float32).reshape(2, 40, 40)
    assert torch.equal(m._sequence(x), x.transpose(1, 2))                     # square: (B,F,T), the reference's reading
    for bad in (z(3, 39, 41), z(3, 40), z(3, 2, 40, 151), z(3, 1, 41, 151), z(2, 1, 1, 40, 9)):
        with pytest.raises(ValueError):
            m._sequence(bad)
    m16 = TCNWakeword(input_size=16, num_channels=[8])
    assert tuple(m16._sequence(z(2, 16, 5)).shape) == (2, 5, 16) and tuple(m16._sequence(z(2, 5, 16)).shape) == (2, 5, 16)


def test_cpu_forward_has_no_fallback():
    from wakeword_trainer_home_amd import _native as nat
    from wakeword_trainer_home_amd.models import TCNWakeword
    from wakeword_trainer_home_amd.models.architectures import NativeCausalConv1d
    with pytest.raises(nat.NativeError, match="no CPU fallback"):
        TCNWakeword()(torch.zeros(2, 5, 40))
    with pytest.raises(nat.NativeError, match="no CPU fallback"):
        NativeCausalConv1d(8, 8, 3)(torch.zeros(2, 5, 8))
    with pytest.raises(ValueError):
        TCNWakeword()(torch.zeros(2, 5, 41))


def test_unsupported_sizes_raise_at_construction():
    from wakeword_trainer_home_amd import _native as nat
    from wakeword_trainer_home_amd.models import TCNWakeword
    with pytest.raises(nat.NativeError, match="multiples of 4"):
        TCNWakeword(num_channels=[30])
    with pytest.raises(nat.NativeError, match="kernel_size"):
        TCNWakeword(kernel_size=9)
    with pytest.raises(nat.NativeError, match="blocks"):
        TCNWakeword(num_channels=[8] * 9)


def test_factory_still_refuses_tcn():
    from wakeword_trainer_home_amd.models import create_model
    with pytest.raises(ValueError, match="outside this build"):
        create_model("tcn")


def test_header_declares_the_layer_and_keeps_the_abi_version():
    from wakeword_trainer_home_amd import _native as nat
    header = (REPO / "include" / "wwhip.h").read_text()
    declared = set(re.findall(r"\b(ww_[a-z0-9_]+)\s*\(", header))
    for name in ("ww_tconv1d_scratch_bytes", "ww_tconv1d_fwd", "ww_tconv1d_bwd"):
        assert name in declared and name in nat.EXPORTS, name
    assert nat.ABI_VERSION == 17 and re.search(r"#define WW_ABI_VERSION 17\b", header)
    lib = nat.load()
    assert lib.ww_abi_version() == 17
    # the scratch size is host arithmetic: 0 for shapes the kernels refuse
    assert lib.ww_tconv1d_scratch_bytes(2, 5, 40, 64, 3) > 0
    assert lib.ww_tconv1d_scratch_bytes(2, 5, 42, 64, 3) == 0 and lib.ww_tconv1d_scratch_bytes(2, 5, 40, 64, 9) == 0
    assert lib.ww_tconv1d_scratch_bytes(2, 5, 40, 64, 0) == 0 and lib.ww_tconv1d_scratch_bytes(0, 5, 40, 64, 3) == 0
