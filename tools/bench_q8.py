#!/usr/bin/env python
"""Times the int8 cnn_small forward against the fp32 model's eval forward, in one process, on one GPU.

    python tools/bench_q8.py [--batch 512] [--rounds 7] [--iters 50] [--out profiles/q8_cnn_small_measured.txt]

Four arms on (B,1,40,151) features: QuantizedCNNSmall in its two forms (depthwise and pointwise as two launches / as one),
CNNSmallWakeword in eval mode with fp32 and with bf16 activation storage.  The arms alternate round by round; each figure is
the median over the rounds of (device-event time of `iters` forwards) / iters, with the rounds' spread beside it.  A second
pass with the library's per-class event timers on gives microseconds per launch class, and the bytes each class must move
(computed from the shapes, below) are set against the 6.29 TB/s the project measured for a device copy.  The int8 bundle is
exported here from a seeded model, calibrated on structured feature maps -- never on noise.
"""
import argparse
import statistics
import sys
import tempfile
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from tests import q8_cases as Q  # noqa: E402
from wakeword_trainer_home_amd import _native as nat  # noqa: E402
from wakeword_trainer_home_amd.export import ExportConfig, ModelExporter, load_exported_model, validate_exported_model  # noqa: E402
from wakeword_trainer_home_amd.models import create_model  # noqa: E402

COPY_RATE = 6.29e12     # bytes/s of a device-to-device copy on this GPU, as DESIGN.md quotes it
F, T = 40, 151


def int8_bytes(B):
    """Bytes each launch class of the int8 forward must move at least (activations only; the weights are 21 KB)."""
    H, W = (F + 1) // 2, (T + 1) // 2
    act, x = B * H * W * 64, B * F * T
    return {"quantize": 4 * x + x, "stem": x + act, "dw": 2 * act, "pw": 2 * act, "dwpw": 2 * act, "gap_fc": act}


def timed(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / iters          # us per forward


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--out", type=Path, default=None)
    args = ap.parse_args()
    dev, B = "cuda:0", args.batch
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    def model_of(act):
        m = create_model("cnn_small", dropout=0.3, act_dtype=act)
        m.load_state_dict({k: torch.from_numpy(v) for k, v in Q.random_state(0).items()}, strict=False)
        return m.to(dev).eval()
    fp32, bf16 = model_of("fp32"), model_of("bf16")
    cal = torch.from_numpy(Q.structured_features(32, F, T, seed=2)).to(dev)
    x = torch.from_numpy(Q.structured_features(64, F, T, seed=3)).to(dev).repeat((B + 63) // 64, 1, 1, 1)[:B].contiguous()
    with tempfile.TemporaryDirectory() as tmp:
        res = ModelExporter(fp32, (1, 1, F, T), dev, calibration=[cal[:16], cal[16:]]).export(
            ExportConfig(output_path=Path(tmp) / "m.npz", quantize_fp16=True, quantize_int8=True))
        assert res["success"] and "int8_error" not in res and "fp16_error" not in res, res
        say(f"bundle sizes: fp32 {res['file_size_mb'] * 1024:.1f} KiB, fp16 {res['fp16_size_mb'] * 1024:.1f} KiB "
            f"(-{res['fp16_reduction']:.1f} %), int8 {res['int8_size_mb'] * 1024:.1f} KiB (-{res['int8_reduction']:.1f} %)")
        for kind in ("path", "fp16_path", "int8_path"):
            v = validate_exported_model(res[kind], fp32, x[:64], dev)
            say(f"validate {kind.replace('_path', '').replace('path', 'fp32'):5s}: max_difference {v['max_difference']:.4g}, "
                f"mean_difference {v['mean_difference']:.4g}")
        with torch.no_grad():
            lg = fp32(x[:64])
        say(f"  (fp32 logits of those 64 maps span {float(lg.min()):.4g} .. {float(lg.max()):.4g})")
        q8 = {form: load_exported_model(res["int8_path"], dev).set_form(form) for form in ("pair", "fused")}
    with torch.no_grad():
        assert torch.equal(q8["pair"](x), q8["fused"](x)), "the two forms differ"
    arms = {"int8 pair": lambda: q8["pair"](x), "int8 fused": lambda: q8["fused"](x), "fp32 eval": lambda: fp32(x),
            "bf16 eval": lambda: bf16(x)}
    times = {k: [] for k in arms}
    with torch.no_grad():
        for fn in arms.values():
            timed(fn, 10)                                   # warm-up of every arm at the timed shape
        for _ in range(args.rounds):
            for k, fn in arms.items():                      # alternating: a drift of the machine hits every arm alike
                times[k].append(timed(fn, args.iters))
    say(f"\nforward at B = {B} on (1,{F},{T}), {args.rounds} alternating rounds of {args.iters} forwards, device events:")
    for k, ts in times.items():
        med = statistics.median(ts)
        say(f"  {k:10s}  {med:8.1f} us/forward  (min {min(ts):.1f}, max {max(ts):.1f})   {B / med * 1e6 / 1e6:7.3f} M samples/s")
    ab = statistics.median(times["int8 pair"]) / statistics.median(times["int8 fused"])
    say(f"  A/B of the two int8 forms: pair / fused = {ab:.3f}")
    # per launch class, the library's event timers on (a run of its own: the events add to the end-to-end time)
    nat.prof_enable(dev)
    by = int8_bytes(B)
    with torch.no_grad():
        for form, classes in (("pair", {"conv_stem_fwd": ["stem"], "dwconv3x3_fwd": ["dw"], "pwconv1x1_fwd": ["pw"], "gap_fwd": ["gap_fc"]}),
                              ("fused", {"conv_stem_fwd": ["stem"], "pwconv1x1_fwd": ["dwpw"], "gap_fwd": ["gap_fc"]})):
            nat.prof_collect(dev)
            for _ in range(args.iters):
                q8[form](x)
            got = nat.prof_collect(dev)
            say(f"\nint8 {form} (the quantize launch has no timer class): us per launch, bytes the launch must move, and that over the {COPY_RATE / 1e12:.2f} TB/s copy rate:")
            for cls, names in classes.items():
                if cls not in got:
                    continue
                ms, n = got[cls]
                us, nbytes = ms * 1e3 / n, by[names[0]]
                say(f"  {cls:13s} ({names[0]:6s}) {us:7.1f} us x {n // args.iters} per forward   {nbytes / 1e6:7.1f} MB   "
                    f"{nbytes / (us * 1e-6) / 1e12:5.2f} TB/s = {nbytes / (us * 1e-6) / COPY_RATE:4.2f} of the copy rate")
    nat.prof_enable(dev, [])
    if args.out:
        args.out.parent.mkdir(parents=True, exist_ok=True)
        args.out.write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
