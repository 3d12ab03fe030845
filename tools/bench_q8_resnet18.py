#!/usr/bin/env python
"""Times the int8 ResNet18Wakeword forward against the float model's eval forward, in one process, on one GPU.

    python tools/bench_q8_resnet18.py [--batch 128] [--rounds 7] [--iters 20] [--out profiles/q8_resnet18_measured.txt]

Two feature shapes, (1,40,151) and the preset's own (1,128,251), at the preset's per-GPU batch.  Arms per shape: QuantizedResNet18
as dispatched by default, with every conv's weights streamed through L2 (WW_RQ8_WEIGHTS=stream) and with every channel tile
that fits held in LDS (WW_RQ8_WEIGHTS=lds) -- the library's A/B switch, set per forward here -- ResNet18Wakeword in eval mode with
fp32 storage, and ResNet18Wakeword(mode="bf16", storage="bf16") in eval mode, the yardstick.  The arms alternate round by round;
each figure is the median over the rounds of (device-event time of `iters` forwards) / iters, with the rounds' spread beside it.
Every timed arm runs under its own time limit (a watchdog ends the process with status 124 if an arm overruns it, so nothing more
is started on the device).  A second pass with the library's per-class event timers on times every distinct conv launch of the
int8 forward on its own, fed the tensor the forward left in the workspace, in four forms: weights streamed | in LDS, 64 | 16 rows
a wave; and the stem and max-pool launches.
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

from tests import q8_resnet_cases as RQ  # noqa: E402
from wakeword_trainer_home_amd import _native as nat  # noqa: E402
from wakeword_trainer_home_amd.export import ExportConfig, ModelExporter, load_exported_model, validate_exported_model  # noqa: E402
from wakeword_trainer_home_amd.models import ResNet18Wakeword  # noqa: E402

SHAPES = [(40, 151), (128, 251)]
LDS_FITS = 144 * 1024


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


def set_form(weights=None, rowtile=None):
    for k, v in (("WW_RQ8_WEIGHTS", weights), ("WW_RQ8_ROWTILE", rowtile)):     # read by the library at every conv launch
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = v


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--arm-limit", type=float, default=90.0, help="seconds one timed arm of one round may take")
    ap.add_argument("--out", type=Path, default=None)
    args = ap.parse_args()
    dev, B = "cuda:0", args.batch
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    state = {k: torch.from_numpy(v) for k, v in RQ.random_state(2, seed=0, gain=0.5).items()}

    def model_of(**kw):
        m = ResNet18Wakeword(num_classes=2, **kw)
        m.load_state_dict(state)
        return m.to(dev).eval()
    fp32, bf16 = model_of(), model_of(mode="bf16", storage="bf16")
    for F, T in SHAPES:
        say(f"==== features (1,{F},{T}), B = {B}")
        cal = torch.from_numpy(RQ.structured_features(16, F, T, seed=2)).to(dev)
        x = torch.from_numpy(RQ.structured_features(32, F, T, seed=3)).to(dev).repeat((B + 31) // 32, 1, 1, 1)[:B].contiguous()
        with tempfile.TemporaryDirectory() as tmp, time_limit(300, "the export"):
            res = ModelExporter(fp32, (1, 1, F, T), dev, calibration=[cal[:8], cal[8:]]).export(
                ExportConfig(output_path=Path(tmp) / "m.npz", quantize_fp16=True, quantize_int8=True))
            assert res["success"] and "int8_error" not in res and "fp16_error" not in res, res
            say(f"bundle sizes: fp32 {res['file_size_mb']:.2f} MiB, fp16 {res['fp16_size_mb']:.2f} MiB "
                f"(-{res['fp16_reduction']:.1f} %), int8 {res['int8_size_mb']:.2f} MiB (-{res['int8_reduction']:.1f} %)")
            for kind in ("path", "fp16_path", "int8_path"):
                v = validate_exported_model(res[kind], fp32, x[:32], dev)
                say(f"validate {kind.replace('_path', '').replace('path', 'fp32'):5s}: max_difference {v['max_difference']:.4g}, "
                    f"mean_difference {v['mean_difference']:.4g}")
            with torch.no_grad():
                lg = fp32(x[:32])
            say(f"  (fp32 logits of those 32 maps span {float(lg.min()):.4g} .. {float(lg.max()):.4g})")
            q8 = load_exported_model(res["int8_path"], dev)

        def int8_arm(weights):
            def run():
                set_form(weights)
                return q8(x)
            return run
        with torch.no_grad():
            ref = int8_arm(None)()
            assert torch.equal(ref, int8_arm("lds")()) and torch.equal(ref, int8_arm("stream")()), "the forms of the conv kernel differ"
        arms = {"int8": int8_arm(None), "int8 stream": int8_arm("stream"), "int8 lds": int8_arm("lds"), "fp32 eval": lambda: fp32(x),
                "bf16 eval": lambda: bf16(x)}
        times = {k: [] for k in arms}
        with torch.no_grad():
            for k, fn in arms.items():
                with time_limit(args.arm_limit, f"the warm-up of {k}"):
                    timed(fn, 3)                                    # warm-up of every arm at the timed shape
            for _ in range(args.rounds):
                for k, fn in arms.items():                          # alternating: a drift of the machine hits every arm alike
                    with time_limit(args.arm_limit, k):
                        times[k].append(timed(fn, args.iters))
        set_form()
        say(f"\nforward, {args.rounds} alternating rounds of {args.iters} forwards, device events:")
        med = {k: statistics.median(ts) for k, ts in times.items()}
        for k, ts in times.items():
            say(f"  {k:11s}  {med[k]:9.1f} us/forward  (min {min(ts):.1f}, max {max(ts):.1f})   {B / med[k] * 1e3:8.1f} k samples/s")
        for k in ("int8", "int8 stream", "int8 lds"):
            say(f"  {k} / bf16 eval = {med[k] / med['bf16 eval']:.3f}, {k} / fp32 eval = {med[k] / med['fp32 eval']:.3f}")
        # per launch: the library's event timers around each launch (a run of its own)
        views = nat.rq8_workspace_views(q8.workspace(B), B, F, T)
        classes = nat.prof_classes()
        conv_cls, stem_cls = classes[3], classes[1]
        nat.prof_enable(dev, [conv_cls, stem_cls])
        say(f"\nint8 conv launches, us per launch (event pairs around each of {args.iters} launches): weights streamed | in LDS at "
            f"64 rows a wave, streamed | in LDS at 16 rows a wave ('-': the channel tile does not fit LDS; '*': the default "
            f"dispatch), MACs and the rate of the fastest form:")
        seen, total = {}, {"default": 0.0, "best": 0.0}
        with torch.no_grad(), time_limit(3 * args.arm_limit, "the per-launch pass"):
            prev = "pool0"
            for name, cin, cout, stride, down in RQ.blocks():
                launches = [(name + ".conv1", views[prev], 3, stride, nat.RQ8_RELU, {})]
                res_t, z_res = views[prev], -128
                if down:
                    launches.append((name + ".down", views[prev], 1, 2, nat.RQ8_SIGNED, {}))
                    res_t, z_res = views[name + ".ds"], 0
                i = [n for n, *_ in RQ.blocks()].index(name)
                launches.append((name + ".conv2", views[name + ".h1"], 3, 1, nat.RQ8_ADD,
                                 dict(residual=res_t, res_zero=z_res, res_mult=q8.io.res_mult[i], res_shift=q8.io.res_shift[i])))
                for lname, a, k, s, ep, kw in launches:
                    w = q8.conv(lname)[0]
                    key = (tuple(a.shape), w.shape[0], k, s, ep)
                    if key not in seen:
                        rows = a.shape[0] * (RQ.half(a.shape[1]) if s == 2 else a.shape[1]) * (RQ.half(a.shape[2]) if s == 2 else a.shape[2])
                        slab = 64 * k * k * a.shape[3]
                        us = {}
                        for form in (("stream", "4"), ("lds", "4"), ("stream", "1"), ("lds", "1"), (None, None)):
                            if form[0] == "lds" and slab > LDS_FITS:
                                continue
                            set_form(*form)
                            nat.prof_collect(dev)
                            for _ in range(args.iters):
                                nat.rq8_conv2d_fwd(a, *q8.conv(lname), k, s, -128, ep, **kw)
                            ms, n = nat.prof_collect(dev)[conv_cls]
                            us[form] = ms * 1e3 / n
                        seen[key] = (us, rows * w.numel())
                    us, macs = seen[key]
                    best = min(v for f, v in us.items() if f != (None, None))
                    cells = " | ".join(f"{us[f]:7.1f}" if f in us else "      -" for f in (("stream", "4"), ("lds", "4"), ("stream", "1"), ("lds", "1")))
                    say(f"  {lname:11s} {a.shape[1]:3d}x{a.shape[2]:<3d} {a.shape[3]:3d} -> {w.shape[0]:3d} k{k} s{s}: {cells}   * {us[(None, None)]:7.1f} us   "
                        f"{macs / 1e9:6.2f} GMAC   {2 * macs / (best * 1e-6) / 1e12:6.1f} TOP/s")
                    total["default"] += us[(None, None)]
                    total["best"] += best
                prev = name + ".out"
            set_form()
            other = {}
            for what, cls, fn in (("stem", stem_cls, lambda: nat.rq8_stem_fwd(views["xq"], *q8.conv("stem"), q8.io.in_zero)),):
                nat.prof_collect(dev)
                for _ in range(args.iters):
                    fn()
                ms, n = nat.prof_collect(dev)[cls]
                other[what] = ms * 1e3 / n
            other["maxpool"] = timed(lambda: nat.rq8_maxpool_fwd(views["stem"]), args.iters)
            x0 = x[:, 0].contiguous()
            other["quantize"] = timed(lambda: nat.q8_quantize(x0, q8.io.in_scale, q8.io.in_zero), args.iters)
        say(f"  the nineteen conv launches together: {total['default']:.1f} us as dispatched ({total['best']:.1f} us with the fastest form "
            f"of each) of the {med['int8']:.1f} us forward; stem {other['stem']:.1f} us (7x7 as one K chunk on the matrix pipe), max pool "
            f"{other['maxpool']:.1f} us and quantize {other['quantize']:.1f} us (the last two with the wrapper's allocation)")
        nat.prof_enable(dev, [])
        say()
    if args.out:
        args.out.parent.mkdir(parents=True, exist_ok=True)
        args.out.write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
