"""Writes g13_q8_cnn_small.npz and q8_errors.json: `python tests/golden/make_golden_q8.py` from the repository root.

The fixture: a seeded cnn_small state with non-trivial BatchNorm statistics, 32 structured feature maps (stored as float16:
every value is exactly a float16, the tests widen them), and the calibration ranges of the float64 model over the first 16.
q8_errors.json records what the RESTATED law (tests/q8_cases.py, not the package's interpreter) loses against the float64
model on all 32 maps; tests/test_export_host.py holds the interpreter to twice that.
"""
import json
import sys
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent.parent))

from tests import q8_cases as Q  # noqa: E402

N, N_CAL, F, T = 32, 16, 40, 151


def main():
    state = Q.random_state(seed=0)
    x = Q.structured_features(N, F, T, seed=0).astype(np.float16)
    xf = x.astype(np.float32)
    _, ranges = Q.float_forward(state, xf[:N_CAL])
    arrays = {"state/" + k: v for k, v in state.items()}
    arrays.update(x=x, x_min=np.float64(ranges["x_min"]), x_max=np.float64(ranges["x_max"]),
                  a_max=np.array(ranges["a_max"], np.float64), p_max=np.float64(ranges["p_max"]))
    np.savez_compressed(HERE / "g13_q8_cnn_small.npz", **arrays)
    logits, _ = Q.float_forward(state, xf)
    q = Q.r_forward(Q.r_quantize_model(state, (F, T), ranges), xf)["logits"]
    d = np.abs(q.astype(np.float64) - logits)
    margin = logits[:, 1] - logits[:, 0]
    rec = {"cnn_small": {"max_abs_dlogit": float(f"{d.max():.3g}"), "mean_abs_dlogit": float(f"{d.mean():.3g}"),
                         "margin_min": float(f"{margin.min():.4g}"), "margin_max": float(f"{margin.max():.4g}"),
                         "samples": N, "calibration_samples": N_CAL, "feature_shape": [F, T]}}
    (HERE / "q8_errors.json").write_text(json.dumps(rec, indent=1) + "\n")
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
