"""Writes g14_q8_tcn.npz and q8_tcn_errors.json: `python tests/golden/make_golden_q8_tcn.py` from the repository root.

The fixture: the default TCNWakeword (40 -> 64 -> 128 -> 256, k = 3) at g10's size, (F, T) = (40, 45).  Its parameters are NOT
stored: they are ``q8_tcn_cases.random_state(args, 2, seed=param_seed, gain=gain)`` (NumPy's PCG64 stream), with ``psamp.*`` -- a
few evenly spaced entries of every tensor -- to confirm the regeneration, as g10_tcn.npz does.  Stored in full: 24 structured
log-mel-like feature maps (float16: every value is exactly a float16, the tests widen them), the calibration ranges of the
float64 model over the first 12, and the float64 logits of all 24.

q8_tcn_errors.json records what the RESTATED law (tests/q8_tcn_cases.py, not the package's interpreter) loses against the float64
model on all 24 maps, and the span of the logit margin.  tests/test_export_tcn_host.py holds the interpreter to twice that
maximum and requires the margins to span more than 20 times it; this script asserts that the restated law itself meets both, so
the inputs chosen here (levels, floors and bursts that differ from sample to sample) are ones on which the check can fail.
"""
import json
import sys
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent.parent))

from tests import q8_tcn_cases as TQ  # noqa: E402

N, N_CAL, F, T = 24, 12, 40, 45
CHANNELS, K, PARAM_SEED, GAIN = [64, 128, 256], 3, 0, 2.0
PSAMP = 16


def sample_index(n):
    return np.arange(n) if n <= PSAMP else np.linspace(0, n - 1, PSAMP).astype(np.int64)


def main():
    args = TQ.tcn_args(F, CHANNELS, K)
    state = TQ.random_state(args, 2, seed=PARAM_SEED, gain=GAIN)
    x = TQ.structured_features(N, F, T, seed=0).astype(np.float16)
    xf = x.astype(np.float32)
    _, ranges = TQ.float_forward(state, args, xf[:N_CAL])
    logits, _ = TQ.float_forward(state, args, xf)
    arrays = {"x": x, "logits": logits, "x_min": np.float64(ranges["x_min"]), "x_max": np.float64(ranges["x_max"]),
              "a_max": np.array(ranges["a_max"], np.float64), "p_max": np.float64(ranges["p_max"]),
              "param_seed": np.int64(PARAM_SEED), "gain": np.float64(GAIN), "num_channels": np.array(CHANNELS, np.int64),
              "kernel_size": np.int64(K)}
    for k, v in state.items():
        arrays["psamp." + k] = v.reshape(-1)[sample_index(v.size)]
    np.savez_compressed(HERE / "g14_q8_tcn.npz", **arrays)
    q = TQ.r_forward(args, TQ.r_quantize_model(state, args, (F, T), ranges), xf)["logits"]
    d = np.abs(q.astype(np.float64) - logits)
    margin = logits[:, 1] - logits[:, 0]
    rec = {"TCNWakeword": {"max_abs_dlogit": float(f"{d.max():.3g}"), "mean_abs_dlogit": float(f"{d.mean():.3g}"),
                           "margin_min": float(f"{margin.min():.4g}"), "margin_max": float(f"{margin.max():.4g}"),
                           "samples": N, "calibration_samples": N_CAL, "feature_shape": [F, T]}}
    assert margin.max() - margin.min() > 20 * rec["TCNWakeword"]["max_abs_dlogit"], rec
    (HERE / "q8_tcn_errors.json").write_text(json.dumps(rec, indent=1) + "\n")
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
