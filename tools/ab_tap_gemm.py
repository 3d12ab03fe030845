"""Bitwise A/B of the Conv1d / Conv2d layer entry points between two builds of the library:

    tools/build_ab.sh <parent revision> ww_tconv ww_conv2d        # -> csrc/libwwhip_ab.so
    python tools/ab_tap_gemm.py [--out profiles/r12_tap_gemm_ab_digests.txt]

For libwwhip_ab.so, then for the working tree's libwwhip.so, a fresh child process (own time limit; the second starts only if the
first exited 0) runs ww_tconv1d_fwd / _bwd and ww_conv2d_fwd / _bwd on NON-integer seeded data (tests/tcn_cases.layer_inputs,
tests/resnet_cases.layer_inputs, integer=False) at the _SHAPES of tests/test_tcn_gpu.py and tests/test_resnet_gpu.py in fp32, bf16
and fp16 and prints a sha256 per output tensor.  Conv1d: ReLU on / off x residual on / off, y and y2 masks with a scale != 1,
need_dx=False, dx= accumulate, deferred then flushed; Conv2d: plain, need_dx=False, dx= accumulate, deferred then flushed.  The parent
process compares the two lists line by line and exits non-zero on any difference."""
import argparse
import hashlib
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "wakeword_trainer_home_amd" / "csrc"
CHILD_TIMEOUT_S = 420


def child(lib_path):
    sys.path.insert(0, str(ROOT))
    import torch
    from wakeword_trainer_home_amd import _native as nat
    nat._LIB_PATH = Path(lib_path).resolve()
    from tests import resnet_cases, tcn_cases
    from tests.test_resnet_gpu import _SHAPES as conv2d_shapes
    from tests.test_tcn_gpu import _SHAPES as tconv_shapes
    dev = "cuda:0"
    modes = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}
    f = lambda t: t.float().to(dev)

    def emit(tag, **tensors):
        torch.cuda.synchronize()
        for name, t in tensors.items():
            if t is not None:
                print(f"{tag} {name} {hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()}")

    for shape in tconv_shapes:
        B, T, Cin, Cout, k, d = shape
        d_in = tcn_cases.layer_inputs(B, T, Cin, Cout, k, seed=sum(shape), integer=False)
        x, w, b, dy, res = (f(d_in[n]) for n in ("x", "w", "b", "dy", "res"))
        g = torch.Generator().manual_seed(sum(shape) + 1)
        y1 = f(torch.randint(-1, 2, (B, T, Cout), generator=g).double())
        y2 = f(torch.randint(0, 2, (B, T, Cout), generator=g).double())
        base = f(torch.randn(B, T, Cin, generator=g, dtype=torch.float64))
        for mname, md in modes.items():
            tag = "tconv1d " + "-".join(map(str, shape)) + " " + mname
            for relu in (False, True):
                for residual in (False, True):
                    y = nat.tconv1d_fwd(x, w, b, d, relu=relu, residual=res if residual else None, mode=md)
                    dx, dw, db = nat.tconv1d_bwd(x, w, dy, d, y=y if relu else None, mode=md)
                    emit(f"{tag} relu={int(relu)} residual={int(residual)}", y=y, dx=dx, dw=dw, db=db)
            dx, dw, db = nat.tconv1d_bwd(x, w, dy, d, y=y1, y2=y2, mask_scale=1.7, mode=md)
            emit(f"{tag} masks-y-y2-scale-1.7", dx=dx, dw=dw, db=db)
            dx, dw, db = nat.tconv1d_bwd(x, w, dy, d, mode=md, need_dx=False)
            assert dx is None
            emit(f"{tag} need_dx=False", dw=dw, db=db)
            acc = base.clone()
            dx, dw, db = nat.tconv1d_bwd(x, w, dy, d, mode=md, dx=acc)
            emit(f"{tag} dx-accumulate", dx=acc, dw=dw, db=db)
            slot_w, slot_b = torch.full_like(w, float("nan")), torch.full_like(b, float("nan"))
            dx, _, _ = nat.tconv1d_bwd(x, w, dy, d, mode=md, dw_out=slot_w, db_out=slot_b, defer=True)
            nat.deferred_flush(dev)
            emit(f"{tag} deferred-flushed", dx=dx, dw=slot_w, db=slot_b)

    for shape in conv2d_shapes:
        stride = shape[6]
        d_in = resnet_cases.layer_inputs(*shape, seed=sum(shape), integer=False)
        x, w, dy = (f(d_in[n]) for n in ("x", "w", "dy"))
        g = torch.Generator().manual_seed(sum(shape) + 1)
        base = f(torch.randn(*d_in["x"].shape, generator=g, dtype=torch.float64))
        for mname, md in modes.items():
            tag = "conv2d " + "-".join(map(str, shape)) + " " + mname
            y = nat.conv2d_fwd(x, w, stride, mode=md)
            dx, dw = nat.conv2d_bwd(x, w, dy, stride, mode=md)
            emit(f"{tag} plain", y=y, dx=dx, dw=dw)
            dx, dw = nat.conv2d_bwd(x, w, dy, stride, mode=md, need_dx=False)
            assert dx is None
            emit(f"{tag} need_dx=False", dw=dw)
            acc = base.clone()
            dx, dw = nat.conv2d_bwd(x, w, dy, stride, mode=md, dx=acc)
            emit(f"{tag} dx-accumulate", dx=acc, dw=dw)
            slot = torch.full_like(w, float("nan"))
            dx, _ = nat.conv2d_bwd(x, w, dy, stride, mode=md, dw_out=slot, defer=True)
            nat.deferred_flush(dev)
            emit(f"{tag} deferred-flushed", dx=dx, dw=slot)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", help="(internal) run the layers against this library and print the digests")
    ap.add_argument("--out", help="also write the comparison to this file")
    args = ap.parse_args()
    if args.child:
        child(args.child)
        return 0
    builds = [("parent", CSRC / "libwwhip_ab.so"), ("tree", CSRC / "libwwhip.so")]
    lists = []
    for name, lib in builds:
        if not lib.exists():
            print(f"{lib} not found (parent: tools/build_ab.sh <revision> ww_tconv ww_conv2d)", file=sys.stderr)
            return 2
        try:
            r = subprocess.run([sys.executable, __file__, "--child", str(lib)], capture_output=True, text=True, timeout=CHILD_TIMEOUT_S)
        except subprocess.TimeoutExpired:
            print(f"{name} ({lib.name}) ran into its {CHILD_TIMEOUT_S} s limit; nothing more is started", file=sys.stderr)
            return 3
        if r.returncode != 0:
            print(f"{name} ({lib.name}) exited {r.returncode}; nothing more is started\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}", file=sys.stderr)
            return 3
        lists.append([l for l in r.stdout.splitlines() if l.startswith(("tconv1d ", "conv2d "))])
    a, b = lists
    keys = lambda ls: [l.rsplit(" ", 1)[0] for l in ls]
    differing = [f"{x}  !=  {y.rsplit(' ', 1)[1]}" for x, y in zip(a, b) if x != y] if keys(a) == keys(b) else ["the two runs list different tensors"]
    head = (f"{len(a)} output tensors per build ({builds[0][1].name} = parent, {builds[1][1].name} = this tree), sha256 of the fp32 bytes: "
            + ("all equal" if not differing else f"{len(differing)} DIFFER"))
    text = "\n".join([head] + (["-- differing (parent != tree)"] + differing if differing else []) + ["-- digests"] + b) + "\n"
    print(head)
    for l in differing:
        print(l)
    if args.out:
        Path(args.out).write_text(text)
    return 1 if differing or not a else 0


if __name__ == "__main__":
    sys.exit(main())
