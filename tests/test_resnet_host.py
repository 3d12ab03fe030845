"""ResNet18Wakeword without a GPU: constructor, state dict, and the float64 restatement (tests/resnet_cases.py) pinned to the
reference's own ResNet18Wakeword through tests/golden/g11_resnet18.npz (make_golden_resnet18.py)."""
import re
from pathlib import Path

import numpy as np
import pytest
import torch

from tests.resnet_cases import GOLDEN, ResNetRestated, conv2d_bwd, conv2d_fwd, golden_case, maxpool_bwd, maxpool_fwd, sampled_rel

REPO = Path(__file__).resolve().parents[1]
NEW_NAMES = ("ww_conv2d_scratch_bytes", "ww_conv2d_fwd", "ww_conv2d_bwd", "ww_conv2d_stem_scratch_bytes", "ww_conv2d_stem_fwd",
             "ww_conv2d_stem_bwd_dw", "ww_maxpool3x3s2_fwd", "ww_maxpool3x3s2_bwd")


def test_fixture_holds_the_reference_key_list_and_margin():
    """torchvision's 122 keys under the reference's ``resnet.`` prefix, in torchvision's order, 11 171 266 parameters."""
    sd, g = golden_case()
    keys = g["keys"]
    assert len(keys) == 122 and keys[0] == "resnet.conv1.weight" and keys[-2:] == ["resnet.fc.1.weight", "resnet.fc.1.bias"]
    bn = lambda p: [p + s for s in ("weight", "bias", "running_mean", "running_var", "num_batches_tracked")]
    want = ["resnet.conv1.weight"] + bn("resnet.bn1.")
    for i in range(1, 5):
        for j in range(2):
            p = f"resnet.layer{i}.{j}."
            want += [p + "conv1.weight"] + bn(p + "bn1.") + [p + "conv2.weight"] + bn(p + "bn2.")
            if i > 1 and j == 0:
                want += [p + "downsample.0.weight"] + bn(p + "downsample.1.")
    want += ["resnet.fc.1.weight", "resnet.fc.1.bias"]
    assert keys == want
    assert g["shapes"]["resnet.conv1.weight"] == (64, 1, 7, 7) and g["shapes"]["resnet.layer4.0.downsample.0.weight"] == (512, 256, 1, 1)
    assert g["shapes"]["resnet.fc.1.weight"] == (2, 512) and g["shapes"]["resnet.bn1.num_batches_tracked"] == ()
    n = sum(int(np.prod(g["shapes"][k])) for k in keys if k.endswith(("weight", "bias")))
    assert n == 11171266 == int(np.load(GOLDEN)["n_params"])
    assert float(g["relu_margin"]) >= 4e-5 and int(g["relu_inputs"]) == 150016
    assert tuple(g["x"].shape) == (2, 1, 40, 33) and g["y"].tolist() == [0, 1]


def test_float64_restatement_matches_reference_fixture():
    """The float64 model the GPU tests compare with is the reference's ResNet18Wakeword (run in float64): logits and loss to 1e-12,
    the moved running statistics and the sampled gradients to 1e-10 of their largest entry."""
    sd, g = golden_case()
    x, y = torch.from_numpy(g["x"]).double(), torch.from_numpy(g["y"])
    oracle = ResNetRestated(sd)
    ev = oracle.forward(x, training=False)
    assert (ev - torch.from_numpy(g["logits_eval"])).abs().max().item() <= 1e-12
    out, loss, grads = oracle.loss_and_grads(x, y)
    assert (out - torch.from_numpy(g["logits_train"])).abs().max().item() <= 1e-12
    assert abs(loss - float(g["loss"])) <= 1e-12
    assert len(oracle.pres) == 17 and sum(p.numel() for p in oracle.pres) == 150016
    assert min(p.abs().min().item() for p in oracle.pres) == pytest.approx(float(g["relu_margin"]), rel=1e-6)
    assert sorted(grads) == sorted(g["gsamp"])
    for n, gr in grads.items():
        assert tuple(gr.shape) == g["shapes"][n], n
        assert sampled_rel(gr, g, n) <= 1e-10, n
    for k, v in g["rstat"].items():
        assert (oracle.sd[k] - torch.from_numpy(v)).abs().max().item() <= 1e-10 * np.abs(v).max(), k
    assert all(int(oracle.sd[k]) == 1 for k in oracle.sd if k.endswith("num_batches_tracked"))


def test_native_state_dict_matches_fixture_and_round_trips():
    from wakeword_trainer_home_amd.models import ResNet18Wakeword
    from wakeword_trainer_home_amd.models.architectures import ResNet18Wakeword as FromArch, NativeConv2d, BasicBlock  # noqa: F401
    from wakeword_trainer_home_amd.models.flat_buckets import FlatBuckets
    assert FromArch is ResNet18Wakeword and issubclass(ResNet18Wakeword, FlatBuckets) and ResNet18Wakeword.hip_backed
    sd, g = golden_case()
    m = ResNet18Wakeword(dropout=0.0)
    assert list(m.state_dict().keys()) == g["keys"]
    assert all(tuple(v.shape) == g["shapes"][k] for k, v in m.state_dict().items())
    assert sum(p.numel() for p in m.parameters()) == 11171266
    m.load_state_dict(sd)
    assert all(torch.equal(v, sd[k]) for k, v in m.state_dict().items())


def test_constructor_and_initialisation():
    from wakeword_trainer_home_amd.models import ResNet18Wakeword
    torch.manual_seed(0)
    m = ResNet18Wakeword()
    r = m.resnet
    assert r.fc[0].p == pytest.approx(0.3) and r.fc[1].weight.shape == (2, 512) and r.dropout_seed == 0
    assert r.layer1[0].downsample is None and r.layer2[0].downsample is not None and r.layer2[1].downsample is None
    assert [(b.stride, b.conv1.weight.shape[0]) for i in range(1, 5) for b in getattr(r, f"layer{i}")] == \
        [(1, 64), (1, 64), (2, 128), (1, 128), (2, 256), (1, 256), (2, 512), (1, 512)]
    assert r.bn1.eps == 1e-5 and r.bn1.momentum == 0.1 and r.layer3[0].downsample[1].eps == 1e-5
    assert all(torch.equal(b.weight, torch.ones_like(b.weight)) and not b.bias.any() for b in (r.bn1, r.layer4[1].bn2))
    # torchvision's kaiming_normal_(fan_out, relu) for the block convolutions: std = sqrt(2 / (Cout k k))
    w = r.layer2[0].conv1.weight
    assert w.std().item() == pytest.approx((2.0 / (128 * 9)) ** 0.5, rel=0.05)
    # nn.Conv2d's and nn.Linear's defaults for the replaced conv1 and fc: U(+-1/sqrt(fan_in))
    assert r.conv1.weight.abs().max().item() <= 49 ** -0.5 and r.fc[1].weight.abs().max().item() <= 512 ** -0.5
    assert ResNet18Wakeword(num_classes=5, mode="bf16", dropout_seed=3).resnet.fc[1].weight.shape == (5, 512)
    assert ResNet18Wakeword(mode="bf16").resnet.layer1[0].mode == torch.bfloat16
    with pytest.raises(ValueError, match="pretrained"):
        ResNet18Wakeword(pretrained=True)
    with pytest.raises(ValueError, match="input_channels"):
        ResNet18Wakeword(input_channels=3)
    with pytest.raises(ValueError):
        ResNet18Wakeword(mode="int8")
    with pytest.raises(ValueError):
        ResNet18Wakeword(dropout=1.0)


def test_cpu_forward_has_no_fallback():
    from wakeword_trainer_home_amd import _native as nat
    from wakeword_trainer_home_amd.models import ResNet18Wakeword
    from wakeword_trainer_home_amd.models.resnet import BasicBlock, NativeConv2d
    with pytest.raises(nat.NativeError, match="no CPU fallback"):
        ResNet18Wakeword()(torch.zeros(2, 1, 40, 33))
    with pytest.raises(nat.NativeError, match="no CPU fallback"):
        NativeConv2d(8, 8, 3)(torch.zeros(2, 5, 5, 8))
    with pytest.raises(nat.NativeError, match="no CPU fallback"):
        BasicBlock(8, 16, 2)(torch.zeros(2, 5, 5, 8))
    with pytest.raises(ValueError):
        ResNet18Wakeword()(torch.zeros(2, 3, 40, 33))
    with pytest.raises(nat.NativeError, match="multiples of 4"):
        NativeConv2d(6, 8, 3)
    with pytest.raises(nat.NativeError, match="kernel_size"):
        NativeConv2d(8, 8, 4)


def test_factory_still_refuses_resnet18():
    from wakeword_trainer_home_amd.models import create_model
    with pytest.raises(ValueError, match="outside this build"):
        create_model("resnet18")


def test_header_declares_the_layers_and_keeps_the_abi_version():
    from wakeword_trainer_home_amd import _native as nat
    header = (REPO / "include" / "wwhip.h").read_text()
    declared = set(re.findall(r"\b(ww_[a-z0-9_]+)\s*\(", header))
    for name in NEW_NAMES:
        assert name in declared and name in nat.EXPORTS, name
    assert nat.ABI_VERSION == 17 and re.search(r"#define WW_ABI_VERSION 17\b", header)
    lib = nat.load()
    assert lib.ww_abi_version() == 17
    # the scratch size is host arithmetic: 0 for shapes the kernels refuse
    assert lib.ww_conv2d_scratch_bytes(2, 5, 7, 8, 12, 3, 2) >= 9 * 8 * 12 * 4 * 2
    for bad in ((2, 5, 7, 6, 12, 3, 1), (2, 5, 7, 8, 10, 3, 1), (2, 5, 7, 8, 12, 2, 1), (2, 5, 7, 8, 12, 9, 1), (2, 5, 7, 8, 12, 3, 3),
                (0, 5, 7, 8, 12, 3, 1)):
        assert lib.ww_conv2d_scratch_bytes(*bad) == 0, bad
    assert lib.ww_conv2d_stem_scratch_bytes(64, 7) > 0 and lib.ww_conv2d_stem_scratch_bytes(64, 4) == 0


def test_restated_maxpool_is_torchs_on_data_full_of_ties():
    """Integer data in [0, 2] (most windows tie, as after a ReLU): the restated forward and its first-maximum backward equal
    torch.nn.functional.max_pool2d's, for odd and even sizes and an image smaller than the window."""
    g = torch.Generator().manual_seed(4)
    for shape in ((1, 1, 1, 4), (2, 5, 7, 8), (3, 6, 4, 4), (2, 20, 17, 8)):
        x = torch.randint(0, 3, shape, generator=g).double()
        y, idx = maxpool_fwd(x)
        xt = x.permute(0, 3, 1, 2).clone().requires_grad_(True)
        yt = torch.nn.functional.max_pool2d(xt, 3, 2, 1)
        assert torch.equal(y, yt.detach().permute(0, 2, 3, 1))
        dy = torch.randint(-4, 5, tuple(y.shape), generator=g).double()
        yt.backward(dy.permute(0, 3, 1, 2))
        assert torch.equal(maxpool_bwd(idx, dy, shape[1], shape[2]), xt.grad.permute(0, 2, 3, 1))


def test_restated_conv2d_is_torchs():
    """The NHWC restatement against torch's conv2d and its autograd, float64, the strides and sizes of the GPU cases."""
    g = torch.Generator().manual_seed(5)
    for B, H, W, Cin, Cout, k, st in ((2, 5, 7, 8, 12, 3, 1), (2, 5, 7, 8, 12, 3, 2), (3, 6, 4, 8, 4, 1, 2), (1, 5, 3, 1, 4, 7, 2), (1, 1, 1, 4, 4, 3, 1)):
        x = torch.randn(B, H, W, Cin, generator=g, dtype=torch.float64)
        w = torch.randn(Cout, Cin, k, k, generator=g, dtype=torch.float64)
        xt, wt = x.permute(0, 3, 1, 2).clone().requires_grad_(True), w.clone().requires_grad_(True)
        yt = torch.nn.functional.conv2d(xt, wt, None, st, k // 2)
        y = conv2d_fwd(x, w, st)
        assert tuple(y.shape) == tuple(yt.permute(0, 2, 3, 1).shape)
        assert (y - yt.detach().permute(0, 2, 3, 1)).abs().max().item() <= 1e-12
        dy = torch.randn(tuple(y.shape), generator=g, dtype=torch.float64)
        yt.backward(dy.permute(0, 3, 1, 2))
        dx, dw = conv2d_bwd(x, w, dy, st)
        assert (dx - xt.grad.permute(0, 2, 3, 1)).abs().max().item() <= 1e-12 and (dw - wt.grad).abs().max().item() <= 1e-12
