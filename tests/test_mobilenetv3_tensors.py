"""GPU: MobileNetV3Wakeword per tensor against the rounding-aware float64 restatement (oracle/mobilenetv3.py, ``restate=True``)
in fp32, bf16 and fp16 -- logits, loss, all 142 gradients, the 34 BatchNorm layers' running statistics and
num_batches_tracked after the step, and the eval logits -- with error = max |got - ref| / max |ref| per tensor.

The BatchNorm affine parameters, running statistics, SE and head biases are random (at gamma 1 / beta 0 / biases 0 a wrong
dgamma hides: tests/test_cnn_front.py), and no reference gradient may be negligible next to the rest -- except the eleven
projection BatchNorms' dbeta, which is structurally zero (a 1x1 convolution + BatchNorm consumes every block's output, so a
per-channel shift of it changes nothing); their error is taken against the median tensor's magnitude instead.  Dropout 0.3 as
the reference head; fp16 runs at GradScaler's 65536 loss scale (the Trainer's DeviceGradScaler) and compares grad / scale.

Bounds: fp32 one fixed 1e-4 (cnn_small's); 16-bit 9x the error measured on the MI355X for that tensor, the largest over the
shapes of its test (tests/golden/mobilenetv3_16bit_errors.json; every test prints a MEASURED line)."""
import json
from pathlib import Path

import numpy as np
import pytest
import torch
import torch.nn.functional as Fn

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MT = {"fp32": None, "bf16": torch.bfloat16, "fp16": torch.float16}
LOSS_SCALE = {"fp32": 1.0, "bf16": 1.0, "fp16": 65536.0}
FP32_BOUND = 1e-4
BOUND_FACTOR = 9.0
NEGLIGIBLE = 1e-3
BN_FUSED_MAX = 16384 * 1024          # ww_nhwc.hip: WW_BN_BWD_FUSED_MAX_KB, the apply pass finishes the statistics up to it
_MEASURED = {}


def bound(kind, act, name):
    if act == "fp32":
        return FP32_BOUND
    if not _MEASURED:
        _MEASURED.update(json.loads((Path(__file__).parent / "golden" / "mobilenetv3_16bit_errors.json").read_text()))
    return BOUND_FACTOR * _MEASURED[kind][act][name]


def _models(act, seed):
    from oracle.mobilenetv3 import MobileNetV3Oracle
    from wakeword_trainer_home_amd.models.mobilenet import MobileNetV3Wakeword
    torch.manual_seed(seed)
    model = MobileNetV3Wakeword(dropout=0.3, mode=act, dropout_seed=6).to(DEV)
    with torch.no_grad():
        for n, t in model.named_parameters():
            if n.endswith("bias"):
                t.normal_(0, 0.2)
        for m in model.modules():
            if hasattr(m, "running_var"):
                m.weight.uniform_(0.5, 1.5)
                m.running_mean.normal_(0, 0.1)
                m.running_var.uniform_(0.5, 1.5)
    oracle = MobileNetV3Oracle(2, dropout=0.3, seed=6)
    oracle.load_state_dict({k: v.cpu().double() if v.is_floating_point() else v.cpu() for k, v in model.state_dict().items()})
    return model, oracle


def _structural_zero(model):
    from wakeword_trainer_home_amd.models.mobilenet import InvertedResidual
    return {f"mobilenet.features.{i}.block.{len(f.block) - 1}.1.bias" for i, f in enumerate(model.mobilenet.features)
            if isinstance(f, InvertedResidual)}


def _errs(got, ref, floor=0.0):
    got, ref = torch.as_tensor(got).double().cpu(), torch.as_tensor(ref).double().cpu()
    return (got - ref).abs().max().item() / max(ref.abs().max().item(), floor, 1e-300)


def _report_and_check(kind, act, tag, errs, ref_mags=None, zero=()):
    print(f"\nMEASURED {json.dumps({'kind': kind, 'act': act, 'tag': tag, 'errs': errs})}")
    worst = max(errs, key=errs.get)
    print(f"{tag}: worst {worst} {errs[worst]:.2e}")
    if ref_mags:
        med = float(np.median(list(ref_mags.values())))
        small = {n: m / med for n, m in ref_mags.items() if m < NEGLIGIBLE * med and n not in zero}
        assert not small, f"{tag}: negligible reference tensors: {small}"
    bad = {n: (e, bound(kind, act, n)) for n, e in errs.items() if not e <= bound(kind, act, n)}
    assert not bad, f"{tag}: over the bound (error, bound): {bad}"


def check_model(act, B, F, T, seed=0, se_composed=False, monkeypatch=None):
    kind = "se_composed" if se_composed else "train"
    if se_composed:
        from wakeword_trainer_home_amd import _native as nat
        monkeypatch.setattr(nat, "se_supported", lambda *a, **k: False)
    model, oracle = _models(act, seed)
    g = torch.Generator().manual_seed(seed + 1)
    x = torch.randn(B, 1, F, T, generator=g) * 2 - 4
    y = torch.randint(0, 2, (B,), generator=g)
    S = LOSS_SCALE[act]
    model.train()
    oracle.train()
    out = model(x.to(DEV))
    loss = Fn.cross_entropy(out, y.to(DEV))
    (loss * S).backward()
    ref = oracle(x.double(), step=0, training=True, mtype=MT[act], se_rounded=se_composed, restate=True)
    lo = Fn.cross_entropy(ref, y)
    (lo * S).backward()
    torch.cuda.synchronize()
    mags = {n: q.grad.abs().max().item() / S for n, q in oracle.named_parameters()}
    med = float(np.median(list(mags.values())))
    zero = _structural_zero(model)
    errs = {"logits": _errs(out.detach(), ref.detach()), "loss": _errs(loss.detach(), lo.detach())}
    for (n, p), (n2, q) in zip(model.named_parameters(), oracle.named_parameters()):
        assert n == n2
        errs[n] = _errs(p.grad / S, q.grad / S, med if n in zero else 0.0)
    assert len(errs) == 2 + 142
    model.state_dict()                                  # folds the host-side num_batches_tracked counts into the buffers
    for (n, b), (n2, c) in zip(model.named_buffers(), oracle.named_buffers()):
        assert n == n2
        if n.endswith("num_batches_tracked"):
            assert int(b) == int(c) == 1, n
        else:
            errs[n] = _errs(b, c)
    assert len(errs) == 2 + 142 + 68
    model.eval()
    oracle.eval()
    with torch.no_grad():
        ev = model(x.to(DEV))
        ev_ref = oracle(x.double(), training=False, mtype=MT[act], se_rounded=se_composed, restate=True)
    errs["eval_logits"] = _errs(ev, ev_ref)
    _report_and_check(kind, act, f"mobilenetv3 {kind} {act} B={B} F={F} T={T}", errs, mags, zero)
    assert all(torch.isfinite(p.grad).all() for p in model.parameters())
    return model


def restated_grad_errors(model, state0, x, y, act, dropout_seed, S=1.0):
    """Per-tensor errors of ``model``'s gradients (already computed from cross_entropy(model(x), y) * S, dropout step 0) against
    the restatement of its mode, from the state ``state0`` the step started from -- for the whole-model tests that judge the
    16-bit modes by a cosine (tests/test_config_sizes.py, tests/test_mobilenetv3.py)."""
    from oracle.mobilenetv3 import MobileNetV3Oracle
    oracle = MobileNetV3Oracle(2, dropout=model.mobilenet.classifier[0].dropout, seed=dropout_seed)
    oracle.load_state_dict(state0)
    oracle.train()
    (Fn.cross_entropy(oracle(x.double(), step=0, training=True, mtype=MT[act], restate=True), y) * S).backward()
    mags = {n: q.grad.abs().max().item() / S for n, q in oracle.named_parameters()}
    med = float(np.median(list(mags.values())))
    zero = _structural_zero(model)
    return {n: _errs(p.grad / S, q.grad / S, med if n in zero else 0.0)
            for (n, p), (_, q) in zip(model.named_parameters(), oracle.named_parameters())}


# config 3's features; the reference's smoke shape; maps that reach 1 x k deep in the network; config 3's per-GPU batch (the
# stem / block-1 BatchNorm backward takes its three-launch form there: more than 16 MB of activation)
SHAPES = [(16, 40, 151), (3, 64, 50), (4, 13, 50)]


@pytest.mark.parametrize("act", ["fp32", "bf16", "fp16"])
@pytest.mark.parametrize("B,F,T", SHAPES)
def test_mobilenetv3_per_tensor(act, B, F, T):
    check_model(act, B, F, T, seed=B + F + T)


@pytest.mark.parametrize("act", ["bf16", "fp16"])
def test_mobilenetv3_per_tensor_config3_batch(act):
    """B = 256: both forms of the BatchNorm backward's statistics (finished in the apply pass up to 16 MB of activation, a
    finish launch beyond) are reached.  (fp32 at this batch: tests/test_config_sizes.py.)"""
    B, F, T = 256, 40, 151
    stem = B * ((F + 1) // 2) * ((T + 1) // 2) * 16 * 4       # the stem's BatchNorm input, M * C * 4 bytes
    deep = B * 3 * 10 * 96 * 4                                # the last block's projection
    assert stem > BN_FUSED_MAX > deep
    check_model(act, B, F, T, seed=7)


@pytest.mark.parametrize("act", ["bf16", "fp16"])
def test_mobilenetv3_composed_se_per_tensor(act, monkeypatch):
    """se_supported False: every squeeze-excitation block composed of pool -> matrix-core FC + ReLU -> FC + Hardsigmoid -> scale,
    whose FCs round like any GEMM (the restatement's se_rounded)."""
    check_model(act, 3, 64, 50, seed=5, se_composed=True, monkeypatch=monkeypatch)
