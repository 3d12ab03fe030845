#!/usr/bin/env python
"""Times the int8 MobileNetV3Wakeword forward against the model's own eval forward, in one process, on one GPU.

    python tools/bench_q8_mobilenetv3.py [--batch 256] [--rounds 7] [--iters 20] [--out profiles/q8_mobilenetv3_measured.txt]

Four arms on (B,1,40,151) features, a seeded default model: QuantizedMobileNetV3 with the gate multiply as a pass (WW_MQ8_GATE=pass)
and fused into the projection conv (WW_MQ8_GATE=fused; the library reads the variable at every call), MobileNetV3Wakeword(mode="bf16")
in eval mode -- the yardstick -- and MobileNetV3Wakeword in fp32 eval mode.  The arms alternate round by round; each figure is the
median over the rounds of (device-event time of `iters` forwards) / iters, with the rounds' spread beside it.  Every timed arm runs
under its own time limit (a watchdog ends the process with status 124 if an arm overruns it, so nothing more is started on the
device).  A second pass gives the int8 forward per launch: the library's own event timers (ww_prof_enable) over `iters` forwards, by
kernel class, and device events around `iters` calls of each kernel's own entry point, each fed the tensor the forward left in the
workspace.
The bundles are exported here from the seeded model, calibrated on structured feature maps -- never on noise; their sizes and the
``max_difference`` of ``validate_exported_model`` against the fp32 model are reported.  Not measured here: a trained model's
accuracy, other batch sizes or feature shapes, hardware counters.
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

from tests import q8_mobilenet_cases as MQ  # noqa: E402
from wakeword_trainer_home_amd import _native as nat  # noqa: E402
from wakeword_trainer_home_amd.export import ExportConfig, ModelExporter, load_exported_model, validate_exported_model  # noqa: E402
from wakeword_trainer_home_amd.models import create_model  # noqa: E402

F, T = 40, 151


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
    return a.elapsed_time(b) * 1e3 / iters          # us per call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--arm-limit", type=float, default=60.0, help="seconds one timed arm of one round may take")
    ap.add_argument("--out", type=Path, default=None)
    args = ap.parse_args()
    dev, B = "cuda:0", args.batch
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    state = {k: torch.from_numpy(v) for k, v in MQ.random_state(2, seed=0).items()}

    def model_of(**kw):
        m = create_model("mobilenetv3", num_classes=2, pretrained=False, **kw)
        m.load_state_dict(state)
        return m.to(dev).eval()
    fp32, bf16 = model_of(), model_of(mode="bf16")
    cal = torch.from_numpy(MQ.structured_features(32, F, T, seed=2)).to(dev)
    x = torch.from_numpy(MQ.structured_features(64, F, T, seed=3)).to(dev).repeat((B + 63) // 64, 1, 1, 1)[:B].contiguous()
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
        margin = lg[:, 1] - lg[:, 0]
        say(f"  (seeded model, tests/q8_mobilenet_cases.random_state(2, 0); fp32 logits of those 64 maps span {float(lg.min()):.4g} .. "
            f"{float(lg.max()):.4g}, their margins {float(margin.min()):.4g} .. {float(margin.max()):.4g})")
        q8 = load_exported_model(res["int8_path"], dev)

    def int8(form):
        def run():
            os.environ["WW_MQ8_GATE"] = form
            return q8(x)
        return run
    with torch.no_grad():
        a, b = int8("pass")(), int8("fused")()
        say(f"the two gate forms give the same logits: {bool(torch.equal(a, b))}")
    arms = {"int8 pass": int8("pass"), "int8 fused": int8("fused"), "bf16 eval": lambda: bf16(x), "fp32 eval": lambda: fp32(x)}
    times = {k: [] for k in arms}
    with torch.no_grad():
        for k, fn in arms.items():
            with time_limit(args.arm_limit, f"the warm-up of {k}"):
                timed(fn, 3)                                    # warm-up of every arm at the timed shape
        for _ in range(args.rounds):
            for k, fn in arms.items():                          # alternating: a drift of the machine hits every arm alike
                with time_limit(args.arm_limit, k):
                    times[k].append(timed(fn, args.iters))
    say(f"\nforward at B = {B} on (1,{F},{T}), {args.rounds} alternating rounds of {args.iters} forwards, device events:")
    med = {k: statistics.median(ts) for k, ts in times.items()}
    for k, ts in times.items():
        say(f"  {k:11s}  {med[k]:8.1f} us/forward  (min {min(ts):.1f}, max {max(ts):.1f})   {B / med[k]:7.3f} M samples/s")
    say(f"  int8 fused / int8 pass = {med['int8 fused'] / med['int8 pass']:.3f}")
    for k in ("int8 pass", "int8 fused"):
        say(f"  {k} / bf16 eval = {med[k] / med['bf16 eval']:.3f}, {k} / fp32 eval = {med[k] / med['fp32 eval']:.3f}")
    # per class: the library's own event timers around every launch of `iters` int8 forwards
    for form in ("pass", "fused"):
        with torch.no_grad(), time_limit(args.arm_limit, "the profiled forwards"):
            nat.prof_enable(dev)
            nat.prof_collect(dev)
            for _ in range(args.iters):
                int8(form)()
            prof = nat.prof_collect(dev)
            nat.prof_enable(dev, [])
        say(f"\nint8 forward ({form} form) by kernel class, the library's event timers over {args.iters} forwards (quantize carries none):")
        names = {"conv_stem_fwd": "stem", "dwconv3x3_fwd": "depthwise", "pwconv1x1_fwd": "1x1 convs + classifier.0", "gap_fwd": "head pool",
                 "nhwc": "squeeze-excitation + gate pass", "head_loss": "classifier.3"}
        tot = 0.0
        for cls, (ms, cnt) in prof.items():
            say(f"  {names.get(cls, cls):32s} {cnt // args.iters:3d} launches  {ms * 1e3 / args.iters:8.1f} us per forward  "
                f"{ms * 1e3 / cnt:8.1f} us per launch")
            tot += ms * 1e3 / args.iters
        say(f"  together {tot:.1f} us of the {med['int8 ' + form]:.1f} us forward")
    # per launch: device events around `iters` calls of each kernel's own entry point, fed the workspace's tensors (pass form)
    os.environ["WW_MQ8_GATE"] = "pass"
    with torch.no_grad():
        q8(x)
    views = {k: v.clone() for k, v in nat.mq8_workspace_views(q8.workspace(B), B, F, T).items()}
    q8._ws.clear()
    io = q8.io
    say(f"\nint8 forward, us per launch (device events around {args.iters} calls of the kernel's own entry point):")
    total = {"pass": 0.0, "fused": 0.0}

    def launch(name, fn, note="", forms=("pass", "fused")):
        with time_limit(args.arm_limit, name):
            timed(fn, 2)
            us = timed(fn, args.iters)
        say(f"  {name:34s} {us:8.1f} us   {note}")
        for f in forms:
            total[f] += us
        return us
    with torch.no_grad():
        xs = x[:, 0].contiguous()
        launch("quantize", lambda: nat.q8_quantize(xs, io.in_scale, io.in_zero))
        launch("stem 3x3 s2, 1 -> 16", lambda: nat.mq8_stem_fwd(views["xq"], *q8.conv("stem")[:4], io.in_zero, io.stem_zu, q8.conv("stem")[4]))
        cur, z = views["stem"], io.stem_zo
        for i, b in enumerate(q8.blocks):
            p, block_in = f"b{i}.", cur
            hw = f"{b['hw_in'][0]}x{b['hw_in'][1]}"
            if b["expand"]:
                w, bias, m, sh, tab = q8.conv(p + "expand")
                ep, zu = (nat.MQ8_HSWISH, io.exp_zu[i]) if b["hs"] else (nat.MQ8_RELU, 0)
                launch(f"{p}expand 1x1 {b['cin']} -> {b['exp']}", lambda: nat.mq8_conv1x1_fwd(cur, w, bias, m, sh, z, ep, zu, tab), hw)
                cur, z = views[p + "expand"], (io.exp_zo[i] if b["hs"] else -128)
            w, bias, m, sh, tab = q8.conv(p + "dw")
            ep, zu = (nat.MQ8_HSWISH, io.dw_zu[i]) if b["hs"] else (nat.MQ8_RELU, 0)
            launch(f"{p}dw {b['k']}x{b['k']} s{b['stride']}, {b['exp']}",
                   lambda: nat.mq8_dwconv_fwd(cur, w, bias, m, sh, b["k"], b["stride"], z, ep, zu, tab), hw)
            cur, z = views[p + "dw"], (io.dw_zo[i] if b["hs"] else -128)
            gate = None
            if b["se"]:
                launch(f"{p}squeeze-excitation, {b['exp']} / {b['se']}",
                       lambda: nat.mq8_se_fwd(cur, b["exp"], z, io.sepool_mult[i], io.sepool_shift[i], q8.conv(p + "fc1")[:4],
                                              q8.conv(p + "fc2")[:4]))
                gate = views[p + "gate"]
                launch(f"{p}gate pass", lambda: nat.mq8_gate_fwd(cur, gate, z, io.gate_mult[i], io.gate_shift[i]), forms=("pass",))
            w, bias, m, sh, _ = q8.conv(p + "project")
            res = block_in if b["res"] else None
            a_in = views[p + "y"] if b["se"] else cur
            launch(f"{p}project 1x1 {b['exp']} -> {b['cout']}",
                   lambda: nat.mq8_conv1x1_fwd(a_in, w, bias, m, sh, z, nat.MQ8_SIGNED, residual=res, res_mult=io.res_mult[i],
                                               res_shift=io.res_shift[i]), forms=("pass",) if b["se"] else ("pass", "fused"))
            if b["se"]:
                launch(f"{p}project 1x1, gate fused",
                       lambda: nat.mq8_conv1x1_fwd(cur, w, bias, m, sh, z, nat.MQ8_SIGNED, residual=res, res_mult=io.res_mult[i],
                                                   res_shift=io.res_shift[i], gate=gate, gate_mult=io.gate_mult[i],
                                                   gate_shift=io.gate_shift[i]), forms=("fused",))
            cur, z = views[p + "out"], 0
        w, bias, m, sh, tab = q8.conv("last")
        launch("last 1x1 96 -> 576", lambda: nat.mq8_conv1x1_fwd(cur, w, bias, m, sh, 0, nat.MQ8_HSWISH, io.last_zu, tab))
        launch("head: pool, classifier.0, classifier.3",
               lambda: nat.mq8_head_fwd(views["last"], io.last_zo, io.pool_mult, io.pool_shift, q8.conv("cls0")[:4], io.cls_zu, q8.conv("cls0")[4],
                                        io.cls_zo, q8.fc_w, q8.fc_b, q8.fc_scale), "three launches")
    for f in ("pass", "fused"):
        say(f"  the launches of the {f} form together: {total[f]:.1f} us of the {med['int8 ' + f]:.1f} us forward")
    if args.out:
        args.out.parent.mkdir(parents=True, exist_ok=True)
        args.out.write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
