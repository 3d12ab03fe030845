#!/usr/bin/env python
"""Times the int8 LSTMWakeword forward against the model's own eval forward, in one process, on one GPU.

    python tools/bench_q8_lstm.py [--batch 512] [--rounds 7] [--iters 20] [--out profiles/q8_lstm_measured.txt]

Four arms on (B,1,40,151) features, the default model (40 -> 2 layers, bidirectional, H = 128): QuantizedLSTM with the gate tables
in LDS (the default) and read through the caches (WW_LQ8_TABLES=global, the library's A/B switch, set per forward here),
LSTMWakeword(mode="fp16") in eval mode -- the yardstick -- and LSTMWakeword in fp32 eval mode.  The arms alternate round by round;
each figure is the median over the rounds of (device-event time of `iters` forwards) / iters, with the rounds' spread beside it.
Every timed arm runs under its own time limit (a watchdog ends the process with status 124 if an arm overruns it, so nothing more
is started on the device).  A second pass times every launch of the int8 forward on its own, device events around `iters` calls
of the per-kernel entry point, each fed the tensor the forward left in the workspace; the recurrence in both table forms, and
on a half, a quarter and 16 of the batch rows (fewer workgroups, the same work each).
The bundles are exported here from a seeded model, calibrated on structured feature maps -- never on noise; their sizes and the
``max_difference`` of ``validate_exported_model`` against the fp32 model are reported.  Not measured here: a trained model's
accuracy, other batch sizes.
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

from tests import q8_lstm_cases as LQ  # noqa: E402
from wakeword_trainer_home_amd import _native as nat  # noqa: E402
from wakeword_trainer_home_amd.export import ExportConfig, ModelExporter, load_exported_model, validate_exported_model  # noqa: E402
from wakeword_trainer_home_amd.models import LSTMWakeword  # noqa: E402

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

    largs = LQ.lstm_args(F, LAYERS, True)
    state = {k: torch.from_numpy(v) for k, v in LQ.random_state(largs, 2, seed=0).items()}

    def model_of(**kw):
        m = LSTMWakeword(input_size=F, hidden_size=128, num_layers=LAYERS, num_classes=2, bidirectional=True, dropout=0.3, **kw)
        m.load_state_dict(state)
        return m.to(dev).eval()
    fp32, fp16 = model_of(), model_of(mode="fp16")
    cal = torch.from_numpy(LQ.structured_features(32, F, T, seed=2)).to(dev)
    x = torch.from_numpy(LQ.structured_features(64, F, T, seed=3)).to(dev).repeat((B + 63) // 64, 1, 1, 1)[:B].contiguous()
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
        say(f"  (fp32 logits of those 64 maps span {float(lg.min()):.4g} .. {float(lg.max()):.4g}, their margins "
            f"{float(margin.min()):.4g} .. {float(margin.max()):.4g})")
        q8 = load_exported_model(res["int8_path"], dev)

    def int8_arm(tables):
        def run():
            os.environ["WW_LQ8_TABLES"] = tables                # read by the library at every recurrence launch
            return q8(x)
        return run
    with torch.no_grad():
        assert torch.equal(int8_arm("lds")(), int8_arm("global")()), "the two forms of the recurrence differ"
    arms = {"int8 lds": int8_arm("lds"), "int8 global": int8_arm("global"), "fp16 eval": lambda: fp16(x),
            "fp32 eval": lambda: fp32(x)}
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
    say(f"  A/B of the two int8 forms: global / lds = {med['int8 global'] / med['int8 lds']:.3f}")
    for k in ("int8 lds", "int8 global"):
        say(f"  {k} / fp16 eval = {med[k] / med['fp16 eval']:.3f}, {k} / fp32 eval = {med[k] / med['fp32 eval']:.3f}")
    # per launch: device events around `iters` calls of each kernel's own entry point, fed the workspace's tensors
    views = {k: v.clone() for k, v in nat.lq8_workspace_views(q8.workspace(B, T), B, T, F, LAYERS, 2).items()}
    q8._ws.clear()
    say(f"\nint8 forward, us per launch (device events around {args.iters} calls of the kernel's own entry point):")
    total = {"lds": 0.0, "global": 0.0}

    def launch(name, fn, note=""):
        with time_limit(args.arm_limit, name):
            timed(fn, 2)
            us = timed(fn, args.iters)
        say(f"  {name:28s} {us:8.1f} us   {note}")
        return us
    with torch.no_grad():
        xs = x[:, 0].contiguous()
        us = launch("quantize + transpose", lambda: nat.tq8_quantize_bt(xs, q8.io.in_scale, q8.io.in_zero))
        total = {k: v + us for k, v in total.items()}
        a_in = views["xq"]
        for k in range(LAYERS):
            w_ih, b_ih, m_i, sh_i, w_hh, b_hh, m_h, sh_h = q8.layer(k)
            macs = B * T * w_ih.numel()
            us = launch(f"l{k} projection, K = {w_ih.shape[1]}", lambda: nat.lq8_proj_fwd(a_in, w_ih, b_ih, m_i, sh_i),
                        f"{macs / 1e9:5.2f} GMAC of the padded product, {B * T * 1024 * 2 / 1e6:.0f} MB of int16 u written")
            total = {kk: v + us for kk, v in total.items()}
            u = views[f"l{k}.u"]
            for tables in total:
                os.environ["WW_LQ8_TABLES"] = tables
                us = launch(f"l{k} recurrence, tables {tables}",
                            lambda: nat.lq8_lstm_layer_fwd(u, w_hh, b_hh, m_h, sh_h, q8.tab_sigmoid, q8.tab_tanh),
                            f"{T} dependent steps")
                say(f"  {'':28s} {us / T:8.3f} us per step")
                total[tables] += us
            a_in = views[f"l{k}.y"]
        us = launch("head", lambda: nat.lq8_head_fwd(a_in, q8.fc_w, q8.fc_b, q8.fc_scale))
        total = {k: v + us for k, v in total.items()}
    say(f"  the launches together: {total['lds']:.1f} | {total['global']:.1f} us of the {med['int8 lds']:.1f} | "
        f"{med['int8 global']:.1f} us forward (tables in LDS | global)")
    os.environ.pop("WW_LQ8_TABLES", None)
    # is the recurrence bound by its step latency or by the number of workgroups?  A workgroup owns 16 batch rows of one direction:
    # the same launch on fewer rows of the same u runs fewer workgroups, each doing what it did before
    say("\nlayer-0 recurrence (tables in LDS) on the first rows of the same u, 2 x B / 16 workgroups:")
    with torch.no_grad():
        w_hh, b_hh, m_h, sh_h = q8.layer(0)[4:]
        for b in sorted({B, B // 2, B // 4, 16}, reverse=True):
            ub = views["l0.u"][:b].contiguous()
            launch(f"B = {b}: {2 * ((b + 15) // 16)} workgroups", lambda: nat.lq8_lstm_layer_fwd(ub, w_hh, b_hh, m_h, sh_h, q8.tab_sigmoid,
                                                                                              q8.tab_tanh), f"{T} dependent steps")
    if args.out:
        args.out.parent.mkdir(parents=True, exist_ok=True)
        args.out.write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
