"""Time of the C-class loss kernel (ww_cen_loss_fwd_bwd) beside the 2-class weighted one (ww_ce2_loss_weighted_fwd_bwd), in one
process: smoothed CE (eps 0.1), a class weight, MEAN over the batch, no confusion matrix and with one.

Each figure is the device time of one launch: --launches back-to-back launches on one stream, captured once into a HIP graph so
that the host's enqueue rate is not what gets measured, bracketed by two events; a warm-up replay, then three timed replays
per kernel, the kernels taking turns, and the median of the three.  The 2-class kernel is timed again beside every C so that
the ratio compares two figures of the same minute.  Prints one JSON line per (B, C) and a last line with the one condition set
in advance: at C = 3, B = 512 the C-class kernel takes at most 1.5x the 2-class weighted kernel's time.

    python tools/bench_loss.py [--launches 200] [--batches 512 4096] [--classes 2 3 12 64]
"""
import argparse
import json
import statistics
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import torch

DEV = "cuda:0"


def graph_of(fn, launches):
    fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(launches):
            fn()
    g.replay()                                                 # warm-up
    torch.cuda.synchronize()
    return g


def timed_us(g, launches):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    g.replay()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1000.0 / launches


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--batches", type=int, nargs="+", default=[512, 4096])
    ap.add_argument("--classes", type=int, nargs="+", default=[2, 3, 12, 64])
    args = ap.parse_args()
    if args.launches < 200:
        raise SystemExit("at least 200 launches per timed window")
    from wakeword_trainer_home_amd import _native as nat
    lib, dev = nat.load(), torch.device(DEV)
    ctx = nat.ctx(dev)
    verdict = None
    for B in args.batches:
        for C in args.classes:
            gen = torch.Generator(device=DEV).manual_seed(1000 * B + C)
            z2 = torch.randn(B, 2, device=DEV, generator=gen) * 2.5
            y2 = torch.randint(0, 2, (B,), device=DEV, generator=gen)
            zc = torch.randn(B, C, device=DEV, generator=gen) * 2.5
            yc = torch.randint(0, C, (B,), device=DEV, generator=gen)
            w2, wc = torch.tensor([0.55, 5.0], device=DEV), torch.linspace(0.5, 5.0, C, device=DEV)
            d2, dc = torch.empty_like(z2), torch.empty_like(zc)
            loss = torch.empty(1, device=DEV)
            stats = torch.zeros(nat.STEP_STATS_BYTES, dtype=torch.uint8, device=DEV)
            matrix = torch.zeros(C, C, dtype=torch.int64, device=DEV)
            stream = lambda: torch.cuda.current_stream(dev).cuda_stream

            def two():
                nat._check(lib.ww_ce2_loss_weighted_fwd_bwd(ctx, z2.data_ptr(), y2.data_ptr(), B, nat.LOSS_CE, 0.1, 0.25, 2.0,
                                                            w2.data_ptr(), nat.REDUCE_MEAN, nat.DIV_BATCH, loss.data_ptr(), None,
                                                            d2.data_ptr(), stats.data_ptr(), None, None, 0, stream()), "ce2")

            def many(conf):
                nat._check(lib.ww_cen_loss_fwd_bwd(ctx, zc.data_ptr(), yc.data_ptr(), B, C, nat.LOSS_CE, 0.1, 0.25, 2.0,
                                                   wc.data_ptr(), nat.REDUCE_MEAN, nat.DIV_BATCH, loss.data_ptr(), None,
                                                   dc.data_ptr(), stats.data_ptr(), None, conf, None, 0, stream()), "cen")
            graphs = {"ce2_weighted": graph_of(two, args.launches), "cen": graph_of(lambda: many(None), args.launches),
                      "cen_confusion": graph_of(lambda: many(matrix.data_ptr()), args.launches)}
            runs = {k: [] for k in graphs}
            for _ in range(3):
                for k, g in graphs.items():
                    runs[k].append(timed_us(g, args.launches))
            med = {k: statistics.median(v) for k, v in runs.items()}
            row = {"bench": "loss_kernel", "gpu": torch.cuda.get_device_name(0), "B": B, "C": C, "launches": args.launches,
                   "ce2_weighted_us": round(med["ce2_weighted"], 3), "cen_us": round(med["cen"], 3),
                   "cen_confusion_us": round(med["cen_confusion"], 3), "cen_over_ce2": round(med["cen"] / med["ce2_weighted"], 3),
                   "runs_us": {k: [round(t, 3) for t in v] for k, v in runs.items()}}
            print(json.dumps(row), flush=True)
            if (B, C) == (512, 3):
                verdict = {"condition": "cen_us <= 1.5 * ce2_weighted_us at C=3, B=512", "cen_us": row["cen_us"],
                           "ce2_weighted_us": row["ce2_weighted_us"], "ratio": row["cen_over_ce2"],
                           "holds": bool(med["cen"] <= 1.5 * med["ce2_weighted"])}
    if verdict is not None:
        print(json.dumps(verdict), flush=True)
        if not verdict["holds"]:
            raise SystemExit(1)


if __name__ == "__main__":
    main()
