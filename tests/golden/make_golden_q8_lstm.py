"""Writes g16_q8_lstm.npz and q8_lstm_errors.json:

    python tests/golden/make_golden_q8_lstm.py --reference PATH/TO/wakeword_trainer_home

The fixture: the default LSTMWakeword (40 -> 2 layers, bidirectional, H = 128, 2 classes) at (F, T) = (40, 45).  Its parameters are
NOT stored: they are ``q8_lstm_cases.random_state(args, 2, seed=param_seed, head_gain=head_gain)`` (NumPy's PCG64 stream; lstm.*
in nn.LSTM's own initialisation range, fc.weight in nn.Linear's times ``head_gain``), with ``psamp.*`` -- a few evenly spaced
entries of every tensor -- to confirm the regeneration, the form make_golden_lstm.py uses.  Stored in full: 24 structured
log-mel-like feature maps (float16: every value is exactly a float16, the tests widen them), the input range over the first 12
(all the LSTM law calibrates) and the float64 logits of all 24, which come from the REFERENCE's own LSTMWakeword, loaded with
these parameters and run in float64 with dropout 0.  The reference module imports torchvision at the top; LSTMWakeword only uses
torch.nn, so an empty stand-in module satisfies that import.  The tests read only the .npz and the .json.

q8_lstm_errors.json records what the RESTATED law (tests/q8_lstm_cases.py, not the package's interpreter) loses against those
logits on all 24 maps (maximum and mean), and the span of the logit margin.  tests/test_export_lstm_host.py holds the interpreter
to twice that maximum and requires the margins to span more than 20 times it; this script asserts that the restated law itself
meets both.  Tried: param_seed 0, 1, 2, each with head_gain 1, 2 and 4.  The head gain scales margin and loss alike and decided
nothing: span / loss was 13.1 at seed 0 (which fails the check), 25.2 at seed 1 and 32.0 at seed 2, at every head gain.  Kept: seed 2,
the widest ratio of the three, with head_gain 1, nn.Linear's own range.
"""
import argparse
import json
import sys
import types
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent.parent))

from tests import q8_lstm_cases as LQ  # noqa: E402

N, N_CAL, F, T = 24, 12, 40, 45
LAYERS, BIDIR, PARAM_SEED, HEAD_GAIN = 2, True, 2, 1.0
PSAMP = 16


def sample_index(n):
    return np.arange(n) if n <= PSAMP else np.linspace(0, n - 1, PSAMP).astype(np.int64)


def reference_logits(reference, state, x):
    """float64 logits of the reference's LSTMWakeword with ``state`` on x (N,1,F,T)."""
    import torch
    sys.path.insert(0, str(Path(reference).resolve()))
    if "torchvision" not in sys.modules:
        tv = types.ModuleType("torchvision")
        tv.models = types.ModuleType("torchvision.models")
        sys.modules["torchvision"] = tv
        sys.modules["torchvision.models"] = tv.models
    from src.models.architectures import create_model as ref_create_model       # noqa: E402  (reference)
    model = ref_create_model("lstm", num_classes=2, input_size=F, hidden_size=128, num_layers=LAYERS, bidirectional=BIDIR,
                             dropout=0.0)
    assert list(model.state_dict()) == list(state), "the seeded law does not produce the reference's state-dict keys in order"
    model.load_state_dict({k: torch.from_numpy(v) for k, v in state.items()})
    model.double().eval()
    with torch.no_grad():
        return model(torch.from_numpy(x[:, 0].transpose(0, 2, 1).astype(np.float64))).numpy()


def main(seed=PARAM_SEED, head_gain=HEAD_GAIN, write=True):
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="checkout of the reference project (its src/ package is imported)")
    ref = ap.parse_args().reference
    args = LQ.lstm_args(F, LAYERS, BIDIR)
    state = LQ.random_state(args, 2, seed=seed, head_gain=head_gain)
    x = LQ.structured_features(N, F, T, seed=0).astype(np.float16)
    xf = x.astype(np.float32)
    logits = reference_logits(ref, state, xf)
    own = LQ.float_forward(state, args, xf)
    assert np.abs(own - logits).max() < 1e-9, "the restated float model and the reference disagree"
    x_min, x_max = float(xf[:N_CAL].min()), float(xf[:N_CAL].max())
    q = LQ.r_forward(args, LQ.r_quantize_model(state, args, x_min, x_max), xf)["logits"]
    d = np.abs(q.astype(np.float64) - logits)
    margin = logits[:, 1] - logits[:, 0]
    rec = {"LSTMWakeword": {"max_abs_dlogit": float(f"{d.max():.3g}"), "mean_abs_dlogit": float(f"{d.mean():.3g}"),
                            "margin_min": float(f"{margin.min():.4g}"), "margin_max": float(f"{margin.max():.4g}"),
                            "samples": N, "calibration_samples": N_CAL, "feature_shape": [F, T]}}
    print(json.dumps(rec), "span / loss", (margin.max() - margin.min()) / d.max())
    assert margin.max() - margin.min() > 20 * rec["LSTMWakeword"]["max_abs_dlogit"], rec
    assert d.max() <= 2 * rec["LSTMWakeword"]["max_abs_dlogit"]
    if not write:
        return
    arrays = {"x": x, "logits": logits, "x_min": np.float64(x_min), "x_max": np.float64(x_max), "param_seed": np.int64(seed),
              "head_gain": np.float64(head_gain), "num_layers": np.int64(LAYERS), "bidirectional": np.bool_(BIDIR)}
    for k, v in state.items():
        arrays["psamp." + k] = v.reshape(-1)[sample_index(v.size)]
    np.savez_compressed(HERE / "g16_q8_lstm.npz", **arrays)
    (HERE / "q8_lstm_errors.json").write_text(json.dumps(rec, indent=1) + "\n")


if __name__ == "__main__":
    main()
