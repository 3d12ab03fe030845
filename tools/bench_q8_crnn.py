#!/usr/bin/env python
"""Times the int8 CRNNWakeword forward against the model's own eval forward, in one process, on one GPU.

    python tools/bench_q8_crnn.py [--batch 512] [--rounds 7] [--iters 20] [--out profiles/q8_crnn_measured.txt]

Three arms on (B,1,40,151) features, the default model (cnn_small's conv stack -> frequency mean -> 2-layer bidirectional GRU,
H = 128): QuantizedCRNN, CRNNWakeword(act_dtype="fp16") in eval mode -- the yardstick -- and CRNNWakeword in fp32 eval mode.  The
arms alternate round by round; each figure is the median over the rounds of (device-event time of `iters` forwards) / iters, with
the rounds' spread beside it.  Every timed arm runs under its own time limit (a watchdog ends the process with status 124 if an arm
overruns it, so nothing more is started on the device).  A second pass gives the int8 forward per launch: the library's own event
timers (ww_prof_enable) over `iters` forwards, by kernel class, and device events around `iters` calls of each kernel's own entry
point, each fed the tensor the forward left in the workspace; the recurrence also on a half, a quarter and 16 of the batch rows
(fewer workgroups, the same work each).
The bundles are exported here from a seeded model, calibrated on structured feature maps -- never on noise; their sizes and the
``max_difference`` of ``validate_exported_model`` against the fp32 model are reported.  Not measured here: a trained model's
accuracy, other batch sizes, counters of the recurrence.
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

from tests import q8_crnn_cases as CQ  # noqa: E402
from wakeword_trainer_home_amd import _native as nat  # noqa: E402
from wakeword_trainer_home_amd.export import ExportConfig, ModelExporter, load_exported_model, validate_exported_model  # noqa: E402
from wakeword_trainer_home_amd.models import create_model  # noqa: E402

F, T, LAYERS = 40, 151, 2


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
    ap.add_argument("--batch", type=int, default=512)
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

    cargs = CQ.crnn_args(LAYERS, True)
    state = {k: torch.from_numpy(v) for k, v in CQ.random_state(cargs, 2, seed=1, gain=4.0).items()}

    def model_of(**kw):
        m = create_model("crnn", num_classes=2, num_layers=LAYERS, bidirectional=True, **kw)
        missing = m.load_state_dict(state, strict=False).missing_keys
        assert all(k.endswith("num_batches_tracked") for k in missing), missing
        return m.to(dev).eval()
    fp32, fp16 = model_of(), model_of(act_dtype="fp16")
    cal = torch.from_numpy(CQ.structured_features(32, F, T, seed=2)).to(dev)
    x = torch.from_numpy(CQ.structured_features(64, F, T, seed=3)).to(dev).repeat((B + 63) // 64, 1, 1, 1)[:B].contiguous()
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
        say(f"  (seeded model, GRU weights at 4 x nn.GRU's range; fp32 logits of those 64 maps span {float(lg.min()):.4g} .. "
            f"{float(lg.max()):.4g}, their margins {float(margin.min()):.4g} .. {float(margin.max()):.4g})")
        q8 = load_exported_model(res["int8_path"], dev)

    arms = {"int8": lambda: q8(x), "fp16 eval": lambda: fp16(x), "fp32 eval": lambda: fp32(x)}
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
    say(f"  int8 / fp16 eval = {med['int8'] / med['fp16 eval']:.3f}, int8 / fp32 eval = {med['int8'] / med['fp32 eval']:.3f}")
    # per class: the library's own event timers around every launch of `iters` int8 forwards
    Tp = (T + 1) // 2
    with torch.no_grad(), time_limit(args.arm_limit, "the profiled forwards"):
        nat.prof_enable(dev)
        nat.prof_collect(dev)
        for _ in range(args.iters):
            q8(x)
        prof = nat.prof_collect(dev)
        nat.prof_enable(dev, [])
    say(f"\nint8 forward by kernel class, the library's event timers over {args.iters} forwards (quantize and head carry none):")
    names = {"conv_stem_fwd": "stem", "pwconv1x1_fwd": "depthwise + pointwise", "gap_fwd": "frequency mean",
             "linear_mfma": "projection", "gru": "recurrence"}
    tot = 0.0
    for cls, (ms, cnt) in prof.items():
        say(f"  {names.get(cls, cls):24s} {cnt // args.iters} launches  {ms * 1e3 / args.iters:8.1f} us per forward  "
            f"{ms * 1e3 / cnt:8.1f} us per launch")
        tot += ms * 1e3 / args.iters
    say(f"  together {tot:.1f} us of the {med['int8']:.1f} us forward")
    # per launch: device events around `iters` calls of each kernel's own entry point, fed the workspace's tensors
    views = {k: v.clone() for k, v in nat.cq8_workspace_views(q8.workspace(B, T), B, F, T, LAYERS, 2).items()}
    q8._ws.clear()
    say(f"\nint8 forward, us per launch (device events around {args.iters} calls of the kernel's own entry point):")
    total = 0.0

    def launch(name, fn, note=""):
        with time_limit(args.arm_limit, name):
            timed(fn, 2)
            us = timed(fn, args.iters)
        say(f"  {name:28s} {us:8.1f} us   {note}")
        return us
    with torch.no_grad():
        xs = x[:, 0].contiguous()
        total += launch("quantize", lambda: nat.q8_quantize(xs, q8.io.in_scale, q8.io.in_zero))
        total += launch("stem", lambda: nat.q8_stem_fwd(views["xq"], *q8.conv("stem"), q8.io.in_zero))
        a_in = views["front.stem"]
        for k in range(4):
            total += launch(f"block {k}: dw + pw", lambda: nat.q8_dwpw_fwd(a_in, q8.conv(f"dw{k}"), q8.conv(f"pw{k}")))
            a_in = views[f"front.pw{k}"]
        total += launch("frequency mean", lambda: nat.cq8_fmean_fwd(a_in, q8.io.fmean_mult, q8.io.fmean_shift),
                        f"{B * 20 * Tp * 64 / 1e6:.1f} MB read")
        a_in = views["seq"]
        for k in range(LAYERS):
            w_ih, b_ih, m_i, sh_i, w_hh, b_hh, m_h, sh_h = q8.layer(k)
            total += launch(f"l{k} projection, K = {w_ih.shape[1]}", lambda: nat.lq8_proj_fwd(a_in, w_ih, b_ih, m_i, sh_i),
                            f"{B * Tp * w_ih.numel() / 1e9:5.2f} GMAC, {B * Tp * 768 * 2 / 1e6:.0f} MB of int16 u written")
            u = views[f"l{k}.u"]
            us = launch(f"l{k} recurrence", lambda: nat.cq8_gru_layer_fwd(u, w_hh, b_hh, m_h, sh_h, q8.tab_sigmoid, q8.tab_tanh),
                        f"{Tp} dependent steps")
            say(f"  {'':28s} {us / Tp:8.3f} us per step")
            total += us
            a_in = views[f"l{k}.y"]
        total += launch("head", lambda: nat.lq8_head_fwd(a_in, q8.fc_w, q8.fc_b, q8.fc_scale))
    say(f"  the launches together: {total:.1f} us of the {med['int8']:.1f} us forward")
    # is the recurrence bound by its step latency or by the number of workgroups?  A workgroup owns 16 batch rows of one direction:
    # the same launch on fewer rows of the same u runs fewer workgroups, each doing what it did before
    say("\nlayer-0 recurrence on the first rows of the same u, 2 x B / 16 workgroups:")
    with torch.no_grad():
        w_hh, b_hh, m_h, sh_h = q8.layer(0)[4:]
        for b in sorted({B, B // 2, B // 4, 16}, reverse=True):
            ub = views["l0.u"][:b].contiguous()
            launch(f"B = {b}: {2 * ((b + 15) // 16)} workgroups", lambda: nat.cq8_gru_layer_fwd(ub, w_hh, b_hh, m_h, sh_h, q8.tab_sigmoid,
                                                                                            q8.tab_tanh), f"{Tp} dependent steps")
    if args.out:
        args.out.parent.mkdir(parents=True, exist_ok=True)
        args.out.write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
