"""sha256 of every output tensor of the depthwise layer calls (ww_dwconv3x3_fwd / _bwd), to compare two builds bit for bit: the cases
of tests/dw_strip_cases.py on their integer data at their grid caps, and the benchmark's layer (512, 20, 76) on random data, each in
fp32, bf16 and fp16.
    python tools/dw_output_hashes.py NEW.json
    WW_AB_LIB=other/libwwhip.so python tools/ab_lib.py tools/dw_output_hashes.py REF.json
    python tools/dw_output_hashes.py NEW.json REF.json        # compares, prints one line per case, exit 1 on any difference"""
import hashlib
import json
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))


def sha(t):
    import torch
    return hashlib.sha256(t.contiguous().view(torch.uint8).cpu().numpy().tobytes()).hexdigest()


def dump(path):
    import torch
    from tests import conv_trip_cases as K
    from tests import dw_strip_cases as D
    from tests.test_conv_trips_gpu import DEV, bwd_inputs, fwd_inputs, run_bwd, run_fwd
    from wakeword_trainer_home_amd import _native as nat
    nat.load()
    out = {}
    try:
        for shape in D.SHAPES:
            cf, cb = K.fwd_case("dw", shape)[0], K.bwd_case("dw", shape, False)[0]
            for dname, dt in D.ACTS.items():
                df, db = fwd_inputs("dw", cf, dt), bwd_inputs("dw", cb, dt)
                for cap in D.caps(shape):
                    nat.set_grid_cap(DEV, cap)
                    for dirn, res in (("fwd", run_fwd(nat, "dw", df, dt)), ("bwd", run_bwd(nat, "dw", db))):
                        out[f"{D.shape_id(shape)} {dname} cap {cap} {dirn}"] = {k: sha(v) for k, v in sorted(res.items())}
        nat.set_grid_cap(DEV, 0)
        B, H, W = 512, 20, 76
        gen = torch.Generator().manual_seed(20)
        rnd = lambda *s: torch.randn(*s, generator=gen)
        y32, g32 = rnd(B, H, W, 64), rnd(B, H, W, 64) * (torch.rand(B, H, W, 64, generator=gen) > 0.4)
        vec = dict(w=rnd(64, 1, 3, 3) * 0.3, coef=rnd(192) * 0.1, ss_in=torch.cat([torch.rand(64, generator=gen) + 0.5, rnd(64) * 0.3]),
                   mr_in=torch.cat([rnd(64) * 0.1, torch.rand(64, generator=gen) + 0.7]), gamma_in=torch.rand(64, generator=gen) + 0.5,
                   gamma=torch.rand(64, generator=gen) + 0.5, beta=rnd(64) * 0.2, running_mean=torch.zeros(64), running_var=torch.ones(64))
        vec = {k: v.to(DEV) for k, v in vec.items()}
        for dname, dt in D.ACTS.items():
            y_in, g = y32.to(dt).to(DEV), g32.to(dt).to(DEV)
            f = run_fwd(nat, "dw", dict(vec, y_in=y_in), dt)
            b = run_bwd(nat, "dw", dict(vec, y_in=y_in, y_out=f["y"], g=g))
            out[f"{B}x{H}x{W} {dname} fwd"] = {k: sha(v) for k, v in sorted(f.items())}
            out[f"{B}x{H}x{W} {dname} bwd"] = {k: sha(v) for k, v in sorted(b.items())}
    finally:
        nat.set_grid_cap(DEV, 0)
    Path(path).write_text(json.dumps(out, indent=1))
    print(f"{path}: {len(out)} runs, {sum(len(v) for v in out.values())} tensors")


if len(sys.argv) == 2:
    dump(sys.argv[1])
else:
    a, b = (json.loads(Path(p).read_text()) for p in sys.argv[1:3])
    bad = sorted(set(a) ^ set(b))
    for k in sorted(set(a) & set(b)):
        diff = [n for n in b[k] if a[k].get(n) != b[k][n]]
        bad += diff
        print(f"{k}: {len(b[k])} tensors, {'all equal' if not diff else 'DIFFER: ' + ', '.join(diff)}")
    sys.exit(1 if bad else 0)
