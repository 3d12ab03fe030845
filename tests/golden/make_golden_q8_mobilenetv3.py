"""Writes g18_q8_mobilenetv3.npz and q8_mobilenetv3_errors.json:

    python tests/golden/make_golden_q8_mobilenetv3.py [--survey]

The fixture: MobileNetV3Wakeword (mobilenet_v3_small, one-channel stem, the Linear(576,1024) -> Hardswish -> Linear(1024,2) head) at
(F, T) = (40, 45).  Its parameters are NOT stored: they are ``q8_mobilenet_cases.random_state(num_classes, seed, gain)`` (NumPy's
PCG64 stream; BatchNorm running statistics non-trivial), with ``psamp.*`` -- sixteen evenly strided entries of a few tensors -- to
confirm the regeneration.  Stored in full: 24 structured log-mel-like feature maps (float16: every value is exactly a float16, the
tests widen them), the ranges the restated float model (``q8_mobilenet_cases.float_walk``, float64) reaches over the first 12 --
the input's and, in ``range_names()`` order, every calibrated tensor's (min, max) -- and the float64 logits of all 24.

The reference's MobileNetV3Wakeword needs torchvision, which is not installed where this script runs, so the float64 logits come
from ``oracle/mobilenetv3.py`` (the reference's model restated in plain torch.nn with torchvision's module tree) in float64 eval mode,
loaded with the seeded state; the script asserts that the restated float walk agrees with it to 1e-9.  The tests read only the .npz
and the .json.

q8_mobilenetv3_errors.json records what the RESTATED law (tests/q8_mobilenet_cases.py, not the package's interpreter) loses against
those logits on all 24 maps (maximum and mean), the span of the logit margin, and ``factor`` = span / maximum loss.  The project's
other fixtures reach a factor above 20; tests/test_export_mobilenet_host.py holds the interpreter to twice the recorded maximum and
requires the margins to span ``factor`` times it.  Tried (factor as ``--survey`` printed it): see TRIED below; where none reaches 20
the widest is kept and the JSON carries ``shortfall``.
"""
import argparse
import json
import sys
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent.parent))

from tests import q8_mobilenet_cases as MQ  # noqa: E402

N, N_CAL, F, T, NUM_CLASSES = 24, 12, 40, 45, 2
SEED, GAIN = 0, 1.0
PSAMP_KEYS = ("mobilenet.features.0.0.weight", "mobilenet.features.0.1.running_mean", "mobilenet.features.0.1.running_var",
              "mobilenet.features.2.block.1.0.weight", "mobilenet.features.4.block.2.fc1.weight", "mobilenet.features.4.block.2.fc2.bias",
              "mobilenet.features.9.block.3.1.weight", "mobilenet.features.12.0.weight", "mobilenet.features.12.1.running_var",
              "mobilenet.classifier.0.weight", "mobilenet.classifier.0.bias", "mobilenet.classifier.3.weight")
# (seed, gain) -> span / loss of the restated law, as --survey printed them
TRIED = {(0, 0.7): 0.1, (0, 0.85): 1.5, (0, 0.9): 3.7, (0, 0.95): 5.7, (0, 1.0): 10.0, (0, 1.05): 4.5, (0, 1.1): 2.9, (0, 1.4): 1.2, (0, 2.0): 1.6,
         (1, 0.7): 0.0, (1, 0.9): 0.3, (1, 0.95): 2.3, (1, 1.0): 3.4, (1, 1.05): 2.2, (1, 1.1): 2.1, (1, 1.2): 2.2, (1, 1.4): 1.7, (1, 2.0): 1.6,
         (2, 0.7): 1.0, (2, 0.85): 3.4, (2, 0.9): 7.4, (2, 0.95): 4.8, (2, 1.0): 3.2, (2, 1.05): 1.9, (2, 1.1): 1.8, (2, 1.2): 1.2, (2, 1.4): 2.5,
         (2, 2.0): 1.0, (3, 0.85): 4.0, (3, 0.9): 7.5, (3, 0.95): 5.9, (3, 1.0): 1.8, (3, 1.05): 2.2, (3, 1.1): 1.4, (3, 1.2): 2.3,
         (4, 0.85): 6.1, (4, 0.9): 9.2, (4, 0.95): 5.5, (4, 1.0): 4.7, (4, 1.05): 2.5, (4, 1.1): 1.6, (4, 1.2): 1.4,
         (5, 0.85): 2.1, (5, 0.9): 8.3, (5, 0.95): 3.3, (5, 1.0): 7.6, (5, 1.05): 3.6, (5, 1.1): 2.0, (5, 1.2): 2.2}
# kept: (0, 1.0), the widest.  None reaches 20: the seeded network is chaotic -- its logit span moves by four orders of magnitude between
# gains 0.85 and 1.2 -- so it amplifies the rounding of each of its ~60 requantisations (two per Hardswish layer) about as much as it
# amplifies the differences between the inputs.


def oracle_logits(state, xf):
    import torch
    from oracle.mobilenetv3 import MobileNetV3Oracle
    model = MobileNetV3Oracle(num_classes=NUM_CLASSES, dropout=0.0)
    own = model.state_dict()
    assert list(own) == list(state), "the seeded law does not produce the oracle's state-dict keys in order"
    model.load_state_dict({k: torch.from_numpy(np.asarray(v)).to(own[k].dtype) for k, v in state.items()})
    model.eval()
    with torch.no_grad():
        return model(torch.from_numpy(np.ascontiguousarray(xf, np.float64)), training=False).numpy()


def evaluate(seed, gain, xf):
    state = MQ.random_state(NUM_CLASSES, seed, gain)
    cal, _ = MQ.float_walk(state, xf[:N_CAL])
    _, logits = MQ.float_walk(state, xf)
    q = MQ.r_forward(MQ.r_quantize_model(state, (F, T), cal), xf, F, T)["logits"]
    d = np.abs(q.astype(np.float64) - logits)
    return state, cal, logits, d, logits[:, 1] - logits[:, 0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--survey", action="store_true", help="print span / loss of the restated law for other seeds and gains")
    opt = ap.parse_args()
    x = MQ.structured_features(N, F, T, seed=0).astype(np.float16)
    xf = x.astype(np.float32)
    if opt.survey:
        for seed in (0, 1, 2, 3, 4, 5):
            for gain in (0.7, 0.85, 0.9, 0.95, 1.0, 1.05, 1.1, 1.2, 1.4, 2.0):
                _, _, _, d, margin = evaluate(seed, gain, xf)
                print(f"seed {seed} gain {gain}: loss {d.max():.4g}, margin {margin.min():.4g} .. {margin.max():.4g}, "
                      f"span / loss {(margin.max() - margin.min()) / d.max():.1f}", flush=True)
        return
    state, cal, logits, d, margin = evaluate(SEED, GAIN, xf)
    oracle = oracle_logits(state, xf)
    assert np.abs(oracle - logits).max() < 1e-9 * max(1.0, np.abs(oracle).max()), "the restated float walk and the oracle disagree"
    loss = float(f"{d.max():.3g}")
    span = float(margin.max() - margin.min())
    factor = float(f"{span / loss * 0.999:.3g}")
    rec = {"max_abs_dlogit": loss, "mean_abs_dlogit": float(f"{d.mean():.3g}"), "margin_min": float(f"{margin.min():.4g}"),
           "margin_max": float(f"{margin.max():.4g}"), "factor": factor, "samples": N, "calibration_samples": N_CAL,
           "feature_shape": [F, T], "seed": SEED, "gain": GAIN}
    if factor < 20:
        rec["shortfall"] = (f"no surveyed (seed, gain) reaches the project's factor of 20; {factor} is the widest: the table-based "
                            "Hardswish rule requantises twice per layer")
    print(json.dumps(rec))
    assert span >= factor * loss and d.max() <= 2 * loss
    assert factor >= 20 or factor >= max(TRIED.values(), default=0.0) * 0.99, "a surveyed setting is wider: keep that one"
    meta = {"seed": SEED, "gain": GAIN, "num_classes": NUM_CLASSES, "feature_shape": [F, T], "calibration_samples": N_CAL}
    arrays = {"x": x, "logits64": oracle, "x_range": np.array([cal["x_min"], cal["x_max"]], np.float64),
              "ranges": np.array([cal["ranges"][n] for n in MQ.range_names()], np.float64),
              "meta": np.frombuffer(json.dumps(meta).encode(), np.uint8)}
    for k in PSAMP_KEYS:
        flat = state[k].reshape(-1)
        arrays["psamp." + k] = flat[:: max(1, flat.size // 16)][:16]
    np.savez_compressed(HERE / "g18_q8_mobilenetv3.npz", **arrays)
    (HERE / "q8_mobilenetv3_errors.json").write_text(json.dumps(rec, indent=1) + "\n")


if __name__ == "__main__":
    main()
