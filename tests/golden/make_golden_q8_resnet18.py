"""Writes g15_q8_resnet18.npz and q8_resnet18_errors.json: `python tests/golden/make_golden_q8_resnet18.py` from the repository root.

The fixture: ResNet18Wakeword with two classes at (F, T) = (40, 33), where every stage has an odd size.  Its 11 M parameters are NOT
stored: they are ``q8_resnet_cases.random_state(2, seed=param_seed, gain=gain)`` (NumPy's PCG64 stream), with ``psamp.*`` -- a few
evenly spaced entries of every tensor -- to confirm the regeneration.  Stored in full: 16 structured log-mel-like feature maps
(float16: every value is exactly a float16, the tests widen them), the calibration ranges of the float64 model over the first 8,
and the float64 logits of all 16.

q8_resnet18_errors.json records what the RESTATED law (tests/q8_resnet_cases.py, not the package's interpreter) loses against the
float64 model on all 16 maps, and the span of the logit margin.  tests/test_export_resnet_host.py holds the interpreter to twice
that maximum and requires the margins to span more than 20 times it; this script asserts that the restated law itself meets both,
so the inputs chosen here are ones on which the check can fail.  The parameter gain decides that: with max-calibrated per-tensor
scales a randomly initialised residual network loses about a tenth of its margin span at gain 1.0 (span / loss = 7.0; 11 at 0.7,
14 at 0.4); at gain 0.5 the span is 20.9 times the loss, and that is the fixture.  It also records ``calibration_fp32_rel``: the largest relative
difference between the calibration ranges CPU torch computes in float32 and in float64 -- the round-off any fp32 calibration of
this model carries, against which the device calibration's tolerance is set (tests/test_export_resnet_gpu.py).
"""
import json
import sys
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent.parent))

from tests import q8_resnet_cases as RQ  # noqa: E402

N, N_CAL, F, T = 16, 8, 40, 33
PARAM_SEED, GAIN = 0, 0.5
PSAMP = 16


def sample_index(n):
    return np.arange(n) if n <= PSAMP else np.linspace(0, n - 1, PSAMP).astype(np.int64)


def main():
    import torch
    state = RQ.random_state(2, seed=PARAM_SEED, gain=GAIN)
    x = RQ.structured_features(N, F, T, seed=0).astype(np.float16)
    xf = x.astype(np.float32)
    _, ranges = RQ.float_forward(state, xf[:N_CAL])
    logits, _ = RQ.float_forward(state, xf)
    arrays = {"x": x, "logits": logits, "x_min": np.float64(ranges["x_min"]), "x_max": np.float64(ranges["x_max"]),
              "a_max": np.array(RQ.flat_ranges(ranges), np.float64), "param_seed": np.int64(PARAM_SEED), "gain": np.float64(GAIN)}
    for k, v in state.items():
        arrays["psamp." + k] = v.reshape(-1)[sample_index(v.size)]
    np.savez_compressed(HERE / "g15_q8_resnet18.npz", **arrays)
    q = RQ.r_forward(RQ.r_quantize_model(state, (F, T), ranges), xf)["logits"]
    d = np.abs(q.astype(np.float64) - logits)
    margin = logits[:, 1] - logits[:, 0]
    r32, r64 = RQ.torch_ranges(state, xf[:N_CAL], torch.float32), RQ.torch_ranges(state, xf[:N_CAL], torch.float64)
    a32, a64, ours = (np.array(RQ.flat_ranges(r)) for r in (r32, r64, ranges))
    assert np.abs(a64 - ours).max() <= 1e-9 * np.abs(ours).max(), "torch in float64 and the NumPy restatement disagree"
    assert (a64 > 0).all()
    cal = float((np.abs(a32 - a64) / a64).max())
    rec = {"ResNet18Wakeword": {"max_abs_dlogit": float(f"{d.max():.3g}"), "mean_abs_dlogit": float(f"{d.mean():.3g}"),
                                "margin_min": float(f"{margin.min():.4g}"), "margin_max": float(f"{margin.max():.4g}"),
                                "calibration_fp32_rel": float(f"{cal:.3g}"), "samples": N, "calibration_samples": N_CAL,
                                "feature_shape": [F, T]}}
    assert margin.max() - margin.min() > 20 * rec["ResNet18Wakeword"]["max_abs_dlogit"], rec
    (HERE / "q8_resnet18_errors.json").write_text(json.dumps(rec, indent=1) + "\n")
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
