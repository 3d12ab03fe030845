"""Generate tests/golden/g10_tcn.npz from the reference's own TCNWakeword (``src/models/architectures.py:270-434``).

    python tests/golden/make_golden_tcn.py --reference PATH/TO/wakeword_trainer_home

Two cases with dropout=0.0, both through ``model.fc(model.tcn(x))`` on (B, F, T) input (the reference's ``forward`` transposes
whenever size(1) < size(2), so it cannot take T > F itself): the reference default (channels 40 -> 64 -> 128 -> 256, k = 3) on
x (4, 40, 45) under the plain keys, and ``num_channels=[32, 48], kernel_size=2`` on x (5, 40, 70) under keys prefixed ``small.``.
Under ``fwd.`` the eval logits of the default model through the public ``forward`` for a (4, 37, 40) input (read as (B,T,F)) and a
square (2, 40, 40) one (read as (B,F,T)).

A ReLU network's gradient jumps where a pre-activation changes sign, so a fixture whose float64 and float32 runs disagree about
one sign cannot pin anything to round-off.  ``_case`` therefore searches parameter seeds until, in a float64 copy of the
reference, the smallest |ReLU input| that reaches the output is >= 1e-6 AND every parameter gradient of the float32 run agrees
with the float64 one to <= 1e-5 of its largest entry.  The seed found and that smallest magnitude are stored.

The fixture stays small as g8_lstm.npz does: parameters are ``reference_params(seed, keys, shapes)`` (numpy's PCG64 stream, each
tensor uniform in nn.Conv1d's / nn.Linear's own initialisation range) with ``psamp.*`` to confirm the regeneration; per parameter
``gsamp.*`` (the float32 reference gradient at ``sample_index``) and ``gmax.*`` (its largest |entry|); x, y, logits and the loss
in full.  The reference module imports torchvision at the top; TCNWakeword only uses torch.nn, so an empty stand-in module
satisfies that import.  The tests read only the .npz."""
import argparse
import copy
import sys
import types
from pathlib import Path

import numpy as np
import torch

HERE = Path(__file__).resolve().parent
SAMPLES = 1024
MARGIN = 1e-6
GRAD_AGREE = 1e-5


def reference_params(seed, keys, shapes):
    """{key: float32 array} in state-dict order, each uniform in +-1/sqrt(fan_in): nn.Conv1d's bound for weight and bias
    (fan_in = Cin * k, read off the layer's weight shape) and nn.Linear's."""
    rng = np.random.default_rng(seed)
    out = {}
    for k in keys:
        wshape = shapes[k if k.endswith("weight") else k[:-len("bias")] + "weight"]
        bound = float(np.prod([int(s) for s in wshape[1:]])) ** -0.5
        out[k] = rng.uniform(-bound, bound, tuple(int(s) for s in shapes[k])).astype(np.float32)
    return out


def sample_index(n):
    """Flat indices of the sampled entries of a tensor of n elements: all of them, or SAMPLES evenly spaced ones."""
    return np.arange(n) if n <= SAMPLES else np.linspace(0, n - 1, SAMPLES).astype(np.int64)


def _run(model, x, y, T):
    """-> (logits, loss, {name: grad}, smallest |ReLU input| among those that reach the output) of model.fc(model.tcn(x))."""
    seen = []

    def hook(trim):
        return lambda mod, inp: seen.append(inp[0].detach()[:, :, :T].abs().min().item() if trim else inp[0].detach().abs().min().item())
    handles = []
    for blk in model.tcn.network:
        handles += [blk.relu1.register_forward_pre_hook(hook(True)), blk.relu2.register_forward_pre_hook(hook(True)),
                    blk.relu.register_forward_pre_hook(hook(False))]
    model.zero_grad()
    out = model.fc(model.tcn(x))
    loss = torch.nn.functional.cross_entropy(out, y)
    loss.backward()
    for h in handles:
        h.remove()
    return out.detach(), loss.item(), {n: p.grad.detach().clone() for n, p in model.named_parameters()}, min(seen)


def _case(RefTCN, kw, shape, labels, first_seed):
    model = RefTCN(dropout=0.0, **kw)
    model.train()
    keys = list(model.state_dict().keys())
    shapes = {k: np.array(v.shape, dtype=np.int64) for k, v in model.state_dict().items()}
    y = torch.tensor(labels)
    T = shape[2]
    for seed in range(first_seed, first_seed + 200):
        params = reference_params(seed, keys, shapes)
        model.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()})
        x = torch.from_numpy(np.random.default_rng(seed + 100000).standard_normal(shape).astype(np.float32))
        wide = copy.deepcopy(model).double()
        _, _, g64, margin = _run(wide, x.double(), y, T)
        out, loss, g32, _ = _run(model, x, y, T)
        worst = max((g32[n].double() - g64[n]).abs().max().item() / g64[n].abs().max().item() for n in g32)
        print(f"  seed {seed}: smallest |ReLU input| {margin:.3e}, float32 vs float64 gradients {worst:.2e}")
        if margin >= MARGIN and worst <= GRAD_AGREE:
            break
    else:
        raise SystemExit("no seed met the margin and agreement conditions")
    model.eval()
    with torch.no_grad():
        logits_eval = model.fc(model.tcn(x))
    d = dict(x=x.numpy(), y=y.numpy(), logits_eval=logits_eval.numpy(), logits_train=out.numpy(), loss=np.float64(loss),
             param_seed=np.int64(seed), relu_margin=np.float64(margin), grad_agreement=np.float64(worst), keys=np.array(keys))
    for k in keys:
        idx = sample_index(params[k].size)
        d["shape." + k] = shapes[k]
        d["psamp." + k] = params[k].reshape(-1)[idx]
        d["gsamp." + k] = g32[k].numpy().reshape(-1)[idx]
        d["gmax." + k] = np.float64(g32[k].abs().max().item())
    print(f"{kw or 'default'}: {len(keys)} state-dict keys, seed {seed}, loss {loss:.6f}")
    return d, model


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="checkout of the reference project (its src/ package is imported)")
    args = ap.parse_args()
    sys.path.insert(0, str(Path(args.reference).resolve()))
    if "torchvision" not in sys.modules:
        tv = types.ModuleType("torchvision")
        tv.models = types.ModuleType("torchvision.models")
        sys.modules["torchvision"] = tv
        sys.modules["torchvision.models"] = tv.models
    from src.models.architectures import TCNWakeword as RefTCN       # noqa: E402  (reference)
    out, model = _case(RefTCN, {}, (4, 40, 45), [0, 1, 1, 0], 0)
    small, _ = _case(RefTCN, dict(num_channels=[32, 48], kernel_size=2), (5, 40, 70), [1, 0, 0, 1, 1], 0)
    out.update({"small." + k: v for k, v in small.items()})
    model.eval()
    rng = np.random.default_rng(7)
    with torch.no_grad():
        for name, shape in (("btf", (4, 37, 40)), ("sq", (2, 40, 40))):
            x = torch.from_numpy(rng.standard_normal(shape).astype(np.float32))
            out[f"fwd.x_{name}"] = x.numpy()
            out[f"fwd.logits_{name}"] = model(x).numpy()          # the reference's public forward
    np.savez_compressed(HERE / "g10_tcn.npz", **out)
    print(f"wrote {HERE / 'g10_tcn.npz'}")


if __name__ == "__main__":
    main()
