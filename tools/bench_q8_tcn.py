#!/usr/bin/env python
"""Times the int8 TCNWakeword forward against the fp32 model's eval forward, in one process, on one GPU.

    python tools/bench_q8_tcn.py [--batch 512] [--rounds 7] [--iters 30] [--out profiles/q8_tcn_measured.txt]

Four arms on (B,1,40,151) features, the default model (40 -> 64 -> 128 -> 256, k = 3): QuantizedTCN with the conv kernel's weights
resident in LDS (the default) and streamed through L2 (WW_TQ8_WEIGHTS=stream, the library's A/B switch, set per forward here),
TCNWakeword in eval mode with fp32 storage, and TCNWakeword(mode="bf16", storage="bf16") in eval mode -- the yardstick.  The arms
alternate round by round; each figure is the median over the rounds of (device-event time of `iters` forwards) / iters, with the rounds' spread
beside it.  Every timed arm runs under its own time limit (a watchdog ends the process with status 124 if an arm overruns it,
so nothing more is started on the device).  A second pass with the library's per-class event timers on times every launch of the
int8 forward's conv kernel on its own, in both forms: the nine convs of the model, each fed the tensor the forward left in the
workspace.
The int8 bundle is exported here from a seeded model, calibrated on structured feature maps -- never on noise.
"""
import argparse
import os
import statistics
import sys
import tempfile
import threading
from contextlib import contextmanager
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from tests import q8_tcn_cases as TQ  # noqa: E402
from wakeword_trainer_home_amd import _native as nat  # noqa: E402
from wakeword_trainer_home_amd.export import ExportConfig, ModelExporter, load_exported_model, validate_exported_model  # noqa: E402
from wakeword_trainer_home_amd.models import TCNWakeword  # noqa: E402

F, T = 40, 151
CHANNELS, K = [64, 128, 256], 3


@contextmanager
def time_limit(seconds, what):
    def expire():
        print(f"TIME LIMIT: {what} ran past {seconds} s", flush=True)
        os._exit(124)
    timer = threading.Timer(seconds, expire)
    timer.daemon = True
    timer.start()
    try:
        yield
    finally:
        timer.cancel()


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
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--arm-limit", type=float, default=60.0, help="seconds one timed arm of one round may take")
    ap.add_argument("--out", type=Path, default=None)
    args = ap.parse_args()
    dev, B = "cuda:0", args.batch
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    targs = TQ.tcn_args(F, CHANNELS, K)
    state = {k: torch.from_numpy(v) for k, v in TQ.random_state(targs, 2, seed=0, gain=2.0).items()}

    def model_of(**kw):
        m = TCNWakeword(input_size=F, num_channels=CHANNELS, kernel_size=K, num_classes=2, dropout=0.3, **kw)
        m.load_state_dict(state)
        return m.to(dev).eval()
    fp32, bf16 = model_of(), model_of(mode="bf16", storage="bf16")
    cal = torch.from_numpy(TQ.structured_features(32, F, T, seed=2)).to(dev)
    x = torch.from_numpy(TQ.structured_features(64, F, T, seed=3)).to(dev).repeat((B + 63) // 64, 1, 1, 1)[:B].contiguous()
    with tempfile.TemporaryDirectory() as tmp, time_limit(300, "the export"):
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
        q8 = load_exported_model(res["int8_path"], dev)

    def int8_arm(weights):
        def run():
            os.environ["WW_TQ8_WEIGHTS"] = weights              # read by the library at every conv launch
            return q8(x)
        return run
    with torch.no_grad():
        assert torch.equal(int8_arm("lds")(), int8_arm("stream")()), "the two forms of the conv kernel differ"
    arms = {"int8 lds": int8_arm("lds"), "int8 stream": int8_arm("stream"), "fp32 eval": lambda: fp32(x),
            "bf16 eval": lambda: bf16(x)}
    times = {k: [] for k in arms}
    with torch.no_grad():
        for k, fn in arms.items():
            with time_limit(args.arm_limit, f"the warm-up of {k}"):
                timed(fn, 5)                                    # warm-up of every arm at the timed shape
        for _ in range(args.rounds):
            for k, fn in arms.items():                          # alternating: a drift of the machine hits every arm alike
                with time_limit(args.arm_limit, k):
                    times[k].append(timed(fn, args.iters))
    say(f"\nforward at B = {B} on (1,{F},{T}), {args.rounds} alternating rounds of {args.iters} forwards, device events:")
    med = {k: statistics.median(ts) for k, ts in times.items()}
    for k, ts in times.items():
        say(f"  {k:11s}  {med[k]:8.1f} us/forward  (min {min(ts):.1f}, max {max(ts):.1f})   {B / med[k]:7.3f} M samples/s")
    say(f"  A/B of the two int8 forms: stream / lds = {med['int8 stream'] / med['int8 lds']:.3f}")
    for k in ("int8 lds", "int8 stream"):
        say(f"  {k} / bf16 eval = {med[k] / med['bf16 eval']:.3f}, {k} / fp32 eval = {med[k] / med['fp32 eval']:.3f}")
    # per launch of the conv kernel: the library's event timers around each launch (a run of its own)
    views = nat.tq8_workspace_views(q8.workspace(B), B, F, T, CHANNELS)
    nat.prof_enable(dev, ["pwconv1x1_fwd"])
    say(f"\nint8 conv kernel, us per launch with the weights in LDS | streamed (event pairs around each of {args.iters} launches), MACs "
        f"of the padded product and the rate of the faster form:")
    total = {"lds": 0.0, "stream": 0.0}
    with torch.no_grad(), time_limit(args.arm_limit, "the per-launch pass"):
        src, zero, cin = views["xq"], q8.io.in_zero, F
        for i, c in enumerate(CHANNELS):
            h1, h2 = views[f"b{i}.h1"], views[f"b{i}.h2"]
            am, ash = q8.io.add_mult[i], q8.io.add_shift[i]
            launches = [("conv1", src, zero, 2 ** i, {}), ("conv2", h1, -128, 2 ** i, {})]
            if cin != c:
                launches.append(("down", src, zero, 1, dict(residual=h2, res_mult=am, res_shift=ash)))
            for name, a, z, d, kw in launches:
                w = q8.conv(i, name)[0]
                us = {}
                for weights in total:
                    os.environ["WW_TQ8_WEIGHTS"] = weights
                    nat.prof_collect(dev)
                    for _ in range(args.iters):
                        nat.tq8_conv1d_fwd(a, *q8.conv(i, name), d, z, **kw)
                    ms, n = nat.prof_collect(dev)["pwconv1x1_fwd"]
                    us[weights] = ms * 1e3 / n
                    total[weights] += us[weights]
                macs = B * T * w.numel()
                say(f"  b{i}.{name:5s} {a.shape[2]:3d} -> {w.shape[0]:3d}, k = {w.shape[1]}, d = {d}: "
                    f"{us['lds']:7.1f} | {us['stream']:7.1f} us   "
                    f"{macs / 1e9:6.2f} GMAC   {2 * macs / (min(us.values()) * 1e-6) / 1e12:6.1f} TOP/s")
            src, zero, cin = views[f"b{i}.out"], -128, c
    say(f"  the nine conv launches together: {total['lds']:.1f} | {total['stream']:.1f} us of the {med['int8 lds']:.1f} | "
        f"{med['int8 stream']:.1f} us forward")
    os.environ.pop("WW_TQ8_WEIGHTS", None)
    nat.prof_enable(dev, [])
    if args.out:
        args.out.parent.mkdir(parents=True, exist_ok=True)
        args.out.write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
