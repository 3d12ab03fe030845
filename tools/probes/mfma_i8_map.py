#!/usr/bin/env python
"""Recovers the A / B / C lane maps of v_mfma_i32_16x16x64_i8 from one-hot operands and records them in DESIGN.md.

    python tools/probes/mfma_i8_map.py [--binary PATH | --block SAVED_OUTPUT] [--design DESIGN.md]
    python tools/probes/mfma_i8_map.py --build-only PATH          # compile only: needs no GPU

Builds tools/probes/mfma_i8_map.hip for gfx950 (unless --binary names a build of it), runs it on the GPU and prints the
markdown block it reports; with --design the block replaces the text between the two `mfma_i8_map` markers of that file.
--block takes the block from a saved output of the probe instead of running it.
The probe fails (exit status 1) if a one-hot operand byte does not light exactly one whole row or column of the result.
"""
import argparse
import subprocess
import sys
import tempfile
from pathlib import Path

HERE = Path(__file__).resolve().parent
BEGIN, END = "<!-- mfma_i8_map:begin -->", "<!-- mfma_i8_map:end -->"


def build(binary: Path) -> None:
    subprocess.run(["hipcc", "-O2", "--offload-arch=gfx950", str(HERE / "mfma_i8_map.hip"), "-o", str(binary)], check=True)


def run(binary: Path) -> str:
    r = subprocess.run([str(binary)], capture_output=True, text=True, timeout=120)
    sys.stderr.write(r.stderr)
    if r.returncode != 0:
        sys.stdout.write(r.stdout)
        sys.exit(r.returncode)
    return r.stdout


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--binary", type=Path, default=None, help="a build of mfma_i8_map.hip to run")
    ap.add_argument("--block", type=Path, default=None, help="a saved output of the probe: record it without running")
    ap.add_argument("--design", type=Path, default=None, help="the document whose marked block is replaced")
    ap.add_argument("--build-only", type=Path, default=None, help="write the binary here and stop")
    args = ap.parse_args()
    if args.build_only:
        build(args.build_only)
        return 0
    if args.block:
        block = args.block.read_text()
    elif args.binary:
        block = run(args.binary)
    else:
        with tempfile.TemporaryDirectory() as tmp:
            build(Path(tmp) / "mfma_i8_map")
            block = run(Path(tmp) / "mfma_i8_map")
    sys.stdout.write(block)
    if args.design:
        text = args.design.read_text()
        if BEGIN not in text or END not in text:
            print(f"{args.design}: no {BEGIN} .. {END} block to fill", file=sys.stderr)
            return 1
        head, rest = text.split(BEGIN, 1)
        args.design.write_text(head + BEGIN + "\n" + block.strip() + "\n" + END + rest.split(END, 1)[1])
    return 0


if __name__ == "__main__":
    sys.exit(main())
