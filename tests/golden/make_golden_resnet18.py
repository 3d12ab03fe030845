"""Generate tests/golden/g11_resnet18.npz from the reference's own ResNet18Wakeword (``src/models/architectures.py:14-65``).

    python tests/golden/make_golden_resnet18.py --reference PATH/TO/wakeword_trainer_home

The reference class wraps ``torchvision.models.resnet18(weights=None)``, replaces its ``conv1`` by ``Conv2d(1, 64, 7, 2, 3, bias=False)``
and its ``fc`` by ``Sequential(Dropout, Linear)``.  torchvision is not installed where this runs, so a stand-in module is put into
``sys.modules`` whose ``models.resnet18`` is this file's restatement of torchvision's published resnet18 in ``torch.nn`` (module names,
registration order and layer arguments as published); the reference's OWN class is then built around it, so the fixture pins what
the reference decides: the ``resnet.`` prefix, the replaced ``conv1`` and ``fc``, the forward contract.

One case, dropout 0: x (2, 1, 40, 33), labels [0, 1] -- every stage at an odd size (20x17 -> 10x9 -> 5x5 -> 3x3 -> 2x2), 150 016 ReLU
inputs.  A ReLU network's gradient jumps where a pre-activation changes sign, so the generator searches parameter seeds until, in a
float64 copy of the reference, the smallest |ReLU input| is >= 4e-5 (float32 runs differ from float64 by up to ~4e-5 in a
pre-activation here); seed and margin are stored.

Stored: the float64 eval logits (from the loaded running statistics), training logits, loss, the running statistics after that one
training forward, per parameter ``gsamp.*`` (the float64 gradient at ``sample_index``) and ``gmax.*`` (its largest |entry|); and under
``err.*`` the error of FLOAT32 CPU torch against those float64 values for the same case -- logits and loss absolute, running
statistics and gradients per tensor relative to the tensor's largest entry.  The fixture stays small as g8 / g10 do: parameters are
``reference_params(seed, keys, shapes)`` with ``psamp.*`` to confirm the regeneration.  The tests read only the .npz."""
import argparse
import copy
import sys
import types
from pathlib import Path

import numpy as np
import torch
import torch.nn as nn

HERE = Path(__file__).resolve().parent
SAMPLES = 256
MARGIN = 4e-5
SHAPE, LABELS = (2, 1, 40, 33), [0, 1]


def reference_params(seed, keys, shapes):
    """{key: array} in state-dict order from numpy's PCG64 stream: convolutions N(0, 2 / fan_out) (torchvision's initialisation
    scale), BatchNorm weight U(0.5, 1.5), bias U(-0.2, 0.2), running_mean N(0, 0.1), running_var U(0.5, 1.5), num_batches_tracked
    0, Linear U(+-1/sqrt(fan_in)); float32 (the count: int64)."""
    rng = np.random.default_rng(seed)
    out = {}
    for k in keys:
        shape = tuple(int(s) for s in shapes[k])
        if k.endswith("num_batches_tracked"):
            out[k] = np.zeros((), dtype=np.int64)
        elif len(shape) == 4:
            out[k] = (rng.standard_normal(shape) * (2.0 / (shape[0] * shape[2] * shape[3])) ** 0.5).astype(np.float32)
        elif k.endswith("running_mean"):
            out[k] = (0.1 * rng.standard_normal(shape)).astype(np.float32)
        elif k.endswith("running_var"):
            out[k] = rng.uniform(0.5, 1.5, shape).astype(np.float32)
        elif ".fc." in k:
            wshape = shapes[k[:-len("bias")] + "weight"] if k.endswith("bias") else shapes[k]
            bound = float(int(wshape[1])) ** -0.5
            out[k] = rng.uniform(-bound, bound, shape).astype(np.float32)
        elif k.endswith("weight"):
            out[k] = rng.uniform(0.5, 1.5, shape).astype(np.float32)
        else:
            out[k] = rng.uniform(-0.2, 0.2, shape).astype(np.float32)
    return out


def sample_index(n):
    """Flat indices of the sampled entries of a tensor of n elements: all of them, or SAMPLES evenly spaced ones."""
    return np.arange(n) if n <= SAMPLES else np.linspace(0, n - 1, SAMPLES).astype(np.int64)


# ------------------------------------------------------------------------------------------ torchvision's resnet18, restated
class _BasicBlock(nn.Module):
    expansion = 1

    def __init__(self, inplanes, planes, stride=1, downsample=None):
        super().__init__()
        self.conv1 = nn.Conv2d(inplanes, planes, 3, stride, 1, bias=False)
        self.bn1 = nn.BatchNorm2d(planes)
        self.relu = nn.ReLU(inplace=True)
        self.conv2 = nn.Conv2d(planes, planes, 3, 1, 1, bias=False)
        self.bn2 = nn.BatchNorm2d(planes)
        self.downsample = downsample
        self.stride = stride

    def forward(self, x):
        identity = x
        out = self.relu(self.bn1(self.conv1(x)))
        out = self.bn2(self.conv2(out))
        if self.downsample is not None:
            identity = self.downsample(x)
        out += identity
        return self.relu(out)


class _ResNet18(nn.Module):
    def __init__(self, num_classes=1000):
        super().__init__()
        self.inplanes = 64
        self.conv1 = nn.Conv2d(3, 64, 7, 2, 3, bias=False)
        self.bn1 = nn.BatchNorm2d(64)
        self.relu = nn.ReLU(inplace=True)
        self.maxpool = nn.MaxPool2d(3, 2, 1)
        self.layer1 = self._make_layer(64, 1)
        self.layer2 = self._make_layer(128, 2)
        self.layer3 = self._make_layer(256, 2)
        self.layer4 = self._make_layer(512, 2)
        self.avgpool = nn.AdaptiveAvgPool2d((1, 1))
        self.fc = nn.Linear(512, num_classes)
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                nn.init.kaiming_normal_(m.weight, mode="fan_out", nonlinearity="relu")
            elif isinstance(m, nn.BatchNorm2d):
                nn.init.constant_(m.weight, 1)
                nn.init.constant_(m.bias, 0)

    def _make_layer(self, planes, stride):
        downsample = None
        if stride != 1 or self.inplanes != planes:
            downsample = nn.Sequential(nn.Conv2d(self.inplanes, planes, 1, stride, bias=False), nn.BatchNorm2d(planes))
        layers = [_BasicBlock(self.inplanes, planes, stride, downsample), _BasicBlock(planes, planes)]
        self.inplanes = planes
        return nn.Sequential(*layers)

    def forward(self, x):
        x = self.maxpool(self.relu(self.bn1(self.conv1(x))))
        x = self.layer4(self.layer3(self.layer2(self.layer1(x))))
        return self.fc(torch.flatten(self.avgpool(x), 1))


def install_torchvision_stand_in():
    if "torchvision" in sys.modules and hasattr(sys.modules["torchvision"], "__file__"):
        return                                        # a real torchvision: use it
    tv = types.ModuleType("torchvision")
    tv.models = types.ModuleType("torchvision.models")
    tv.models.resnet18 = lambda weights=None, **kw: _ResNet18(**kw)
    sys.modules["torchvision"] = tv
    sys.modules["torchvision.models"] = tv.models


# ------------------------------------------------------------------------------------------ the case
def _relus(model):
    return [m for m in model.modules() if isinstance(m, nn.ReLU)]


def _margin(model, x):
    """Smallest |ReLU input| of a training-mode forward (which moves the running statistics: reload the state afterwards)."""
    seen = []
    handles = [m.register_forward_pre_hook(lambda mod, inp: seen.append((inp[0].detach().abs().min().item(), inp[0].numel()))) for m in _relus(model)]
    with torch.no_grad():
        model(x)
    for h in handles:
        h.remove()
    return min(s[0] for s in seen), sum(s[1] for s in seen)


def _run(model, x, y):
    """-> (eval logits, train logits, loss, {name: grad}, {name: running statistic after the training forward})"""
    model.eval()
    with torch.no_grad():
        ev = model(x).clone()
    model.train()
    model.zero_grad()
    out = model(x)
    loss = torch.nn.functional.cross_entropy(out, y)
    loss.backward()
    stats = {k: v.detach().clone() for k, v in model.state_dict().items() if "running_" in k}
    return ev, out.detach().clone(), loss.item(), {n: p.grad.detach().clone() for n, p in model.named_parameters()}, stats


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="checkout of the reference project (its src/ package is imported)")
    ap.add_argument("--first-seed", type=int, default=0)
    ap.add_argument("--seeds", type=int, default=4000)
    args = ap.parse_args()
    sys.path.insert(0, str(Path(args.reference).resolve()))
    install_torchvision_stand_in()
    from src.models.architectures import ResNet18Wakeword as RefResNet       # noqa: E402  (reference)
    model = RefResNet(num_classes=2, pretrained=False, dropout=0.0, input_channels=1)
    keys = list(model.state_dict().keys())
    shapes = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    n_params = sum(p.numel() for p in model.parameters())
    print(f"{len(keys)} state-dict keys, {n_params} parameters")
    y = torch.tensor(LABELS)
    wide = copy.deepcopy(model).double().train()
    best = 0.0
    for seed in range(args.first_seed, args.first_seed + args.seeds):
        params = reference_params(seed, keys, shapes)
        sd = {k: torch.from_numpy(np.asarray(v)) for k, v in params.items()}
        x = torch.from_numpy(np.random.default_rng(seed + 100000).standard_normal(SHAPE).astype(np.float32))
        wide.load_state_dict(sd)
        margin, n_relu = _margin(wide, x.double())
        best = max(best, margin)
        if seed % 50 == 0:
            print(f"  seed {seed}: smallest |ReLU input| {margin:.3e} of {n_relu} (best so far {best:.3e})", flush=True)
        if margin >= MARGIN:
            break
    else:
        raise SystemExit("no seed met the margin: shrink the case, do not lower the margin")
    print(f"seed {seed}: margin {margin:.3e} over {n_relu} ReLU inputs")
    model.load_state_dict(sd)
    wide.load_state_dict(sd)
    ev64, out64, loss64, g64, st64 = _run(wide, x.double(), y)
    ev32, out32, loss32, g32, st32 = _run(model, x, y)
    relmax = lambda a, b: (a.double() - b).abs().max().item() / b.abs().max().item()
    d = dict(x=x.numpy(), y=y.numpy(), logits_eval=ev64.numpy(), logits_train=out64.numpy(), loss=np.float64(loss64),
             param_seed=np.int64(seed), relu_margin=np.float64(margin), relu_inputs=np.int64(n_relu), n_params=np.int64(n_params),
             keys=np.array(keys))
    d["err.logits_eval"] = np.float64((ev32.double() - ev64).abs().max().item())
    d["err.logits_train"] = np.float64((out32.double() - out64).abs().max().item())
    d["err.loss"] = np.float64(abs(loss32 - loss64))
    for k in keys:
        idx = sample_index(params[k].size)
        d["shape." + k] = np.array(shapes[k], dtype=np.int64)
        d["psamp." + k] = np.asarray(params[k]).reshape(-1)[idx]
    for k in g64:
        d["gsamp." + k] = g64[k].numpy().reshape(-1)[sample_index(g64[k].numel())]
        d["gmax." + k] = np.float64(g64[k].abs().max().item())
        d["err.grad." + k] = np.float64(relmax(g32[k], g64[k]))
    for k in st64:
        d["rstat." + k] = st64[k].numpy()
        d["err.rstat." + k] = np.float64(relmax(st32[k], st64[k]))
    print(f"float32 CPU torch against float64: eval logits {d['err.logits_eval']:.2e} train logits {d['err.logits_train']:.2e} "
          f"loss {d['err.loss']:.2e} gradients {min(d['err.grad.' + k] for k in g64):.2e} .. {max(d['err.grad.' + k] for k in g64):.2e} "
          f"running statistics {min(d['err.rstat.' + k] for k in st64):.2e} .. {max(d['err.rstat.' + k] for k in st64):.2e}")
    np.savez_compressed(HERE / "g11_resnet18.npz", **d)
    print(f"wrote {HERE / 'g11_resnet18.npz'}")


if __name__ == "__main__":
    main()
