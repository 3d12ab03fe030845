"""Generate tests/golden/g8_lstm.npz from the reference's own LSTMWakeword (its ``create_model("lstm", ...)``).

    python tests/golden/make_golden_lstm.py --reference PATH/TO/wakeword_trainer_home

Two cases with dropout=0.0: the reference default (2 layers, bidirectional: the ``cat(h_n[-2], h_n[-1])`` branch) under the
plain keys, and a 1-layer unidirectional model (the ``h_n[-1]`` branch) under keys prefixed ``uni.``.

The fixture stays small by not storing whole parameter / gradient tensors (0.57 M floats each for the default model):
* the parameters are ``reference_params(seed, keys, shapes)`` below -- numpy's PCG64 stream, each tensor uniform in nn.LSTM's /
  nn.Linear's own initialisation range -- loaded into the reference model; the npz keeps the seed, the state-dict keys and
  shapes, and ``psamp.*`` (the parameters at ``sample_index``) so a reader can confirm it regenerated the same values;
* per parameter, ``gsamp.*`` holds the reference's gradient at ``sample_index`` and ``gmax.*`` the largest |entry| of the whole
  gradient (the scale of the relative error measure);
* x (6, 31, 40), y, eval logits, train logits and the cross-entropy loss in full.
The reference module imports torchvision at the top; LSTMWakeword only uses torch.nn, so an empty stand-in module satisfies
that import.  The tests read only the .npz."""
import argparse
import sys
import types
from pathlib import Path

import numpy as np
import torch

HERE = Path(__file__).resolve().parent
SAMPLES = 2048


def reference_params(seed, keys, shapes):
    """{key: float32 array} in state-dict order: lstm.* uniform in +-1/sqrt(hidden) (nn.LSTM.reset_parameters), fc.* in
    +-1/sqrt(in_features) (nn.Linear's bound for weight and bias)."""
    rng = np.random.default_rng(seed)
    fc_in = int(shapes["fc.1.weight"][1])
    out = {}
    for k in keys:
        bound = 128 ** -0.5 if k.startswith("lstm.") else fc_in ** -0.5
        out[k] = rng.uniform(-bound, bound, tuple(int(s) for s in shapes[k])).astype(np.float32)
    return out


def sample_index(n):
    """Flat indices of the sampled entries of a tensor of n elements: all of them, or SAMPLES evenly spaced ones."""
    return np.arange(n) if n <= SAMPLES else np.linspace(0, n - 1, SAMPLES).astype(np.int64)


def _case(ref_create_model, seed, layers, bidir):
    model = ref_create_model("lstm", num_classes=2, input_size=40, hidden_size=128, num_layers=layers, bidirectional=bidir,
                             dropout=0.0)
    keys = list(model.state_dict().keys())
    shapes = {k: np.array(v.shape, dtype=np.int64) for k, v in model.state_dict().items()}
    params = reference_params(seed, keys, shapes)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()})
    g = torch.Generator().manual_seed(seed + 1)
    x = torch.randn(6, 31, 40, generator=g)
    y = torch.tensor([0, 1, 1, 0, 1, 0])
    model.eval()
    with torch.no_grad():
        logits_eval = model(x)
    model.train()
    out = model(x)
    loss = torch.nn.functional.cross_entropy(out, y)
    loss.backward()
    d = dict(x=x.numpy(), y=y.numpy(), logits_eval=logits_eval.numpy(), logits_train=out.detach().numpy(),
             loss=np.float64(loss.item()), param_seed=np.int64(seed), keys=np.array(keys))
    for k, p in model.named_parameters():
        idx = sample_index(p.numel())
        d["shape." + k] = shapes[k]
        d["psamp." + k] = params[k].reshape(-1)[idx]
        d["gsamp." + k] = p.grad.numpy().reshape(-1)[idx]
        d["gmax." + k] = np.float64(p.grad.abs().max().item())
    print(f"layers={layers} bidirectional={bidir}: {len(keys)} state-dict keys, loss {loss.item():.6f}")
    return d


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
    from src.models.architectures import create_model as ref_create_model       # noqa: E402  (reference)
    out = _case(ref_create_model, 88, 2, True)
    out.update({"uni." + k: v for k, v in _case(ref_create_model, 89, 1, False).items()})
    np.savez_compressed(HERE / "g8_lstm.npz", **out)


if __name__ == "__main__":
    main()
