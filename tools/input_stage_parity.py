"""Per-path summary of the input stage's parity lines.

    python -m pytest tests/test_hip_kernels.py tests/test_audio_augment.py -m gpu -s > log
    python tools/input_stage_parity.py log profiles/<name>.txt

Reads the MEASURED lines (one per compared tensor: device error, the fp32 CPU yardstick's own error, the bound), the
HELD-TO-TIGHT lines (the clips of a tensor held to ln(32768/32767)) and the AT-CEILING lines (one per clip whose bound is
the old rule, with the reason) that tests/input_stage.py prints."""
import collections
import re
import sys

MEASURED = re.compile(r"MEASURED (.+?): max err (\S+) yardstick (\S+) ratio (\S+) worst err/bound (\S+) "
                      r"\(clip (\d+): err (\S+) yardstick (\S+) bound (\S+)\)")
TIGHT = re.compile(r"HELD-TO-TIGHT (.+?): (\d+) of (\d+) clips at (\S+): max err (\S+) yardstick (\S+)")
CEILING = re.compile(r"AT-CEILING (.+?) clip (\d+): err (\S+) yardstick (\S+) bound (\S+) \((.+?)\)$", re.M)
HEADER = """\
# Input stage parity on one MI355X: device against the float64 oracle.  Per path: the case closest to its bound and the largest
# error of any case.  yardstick = the fp32 CPU formulation's own error against the oracle (torch.stft log-mel / MFCC; the fp32
# restatement of the augmentation law, for the direct form the larger of the blocked and the running-sum one).
# From the MEASURED / HELD-TO-TIGHT / AT-CEILING lines of tests/test_hip_kernels.py and tests/test_audio_augment.py (pytest -m gpu -s)."""


def ratio(a, b):
    return f"{a / b:.2f}" if b > 0 else "n/a (yardstick exact)"


def summarise(log):
    groups = collections.defaultdict(list)
    for m in MEASURED.finditer(log):
        groups[re.sub(r" N=\d+ L=\d+", "", m.group(1))].append(tuple(float(v) for v in m.groups()[1:]))
    out = [HEADER]
    for tag in sorted(groups):
        rows = groups[tag]
        w, e = max(rows, key=lambda r: r[3]), max(rows, key=lambda r: r[0])
        out.append(f"{tag}: cases {len(rows)}; closest to its bound: err {w[5]:.3e} yardstick {w[6]:.3e} (ratio "
                   f"{ratio(w[5], w[6])}) bound {w[7]:.3e} err/bound {w[3]:.3f}; largest error: {e[0]:.3e} (yardstick of "
                   f"that case {e[1]:.3e}, ratio {ratio(e[0], e[1])})")
    tight = collections.defaultdict(list)
    for m in TIGHT.finditer(log):
        tight[m.group(1)].append((int(m.group(2)), int(m.group(3)), float(m.group(5)), float(m.group(6))))
    out.append("# Log-mel clips held to ln(32768/32767) = 3.052e-05 itself")
    for tag in sorted(tight):
        rows = tight[tag]
        e = max(rows, key=lambda r: r[2])
        out.append(f"{tag}: {sum(r[0] for r in rows)} of {sum(r[1] for r in rows)} clips; largest error {e[2]:.3e} (yardstick of that "
                   f"case {e[3]:.3e}, ratio {ratio(e[2], e[3])})")
    held = collections.defaultdict(list)
    for m in CEILING.finditer(log):
        held[(m.group(1), int(m.group(2)), m.group(6))].append(tuple(float(v) for v in m.group(3, 4, 5)))
    out.append("# Clips held at the old rule instead of max(ln(32768/32767), 4 x yardstick), and why")
    for (tag, clip, why), rows in sorted(held.items()):
        e = max(rows, key=lambda r: r[0] / r[2])
        out.append(f"{tag} clip {clip}: {len(rows)} cases; worst err {e[0]:.3e} yardstick {e[1]:.3e} bound {e[2]:.3e}: {why}")
    return "\n".join(out) + "\n"


def main(argv):
    if len(argv) != 3:
        sys.exit(__doc__)
    with open(argv[1]) as f:
        text = summarise(f.read())
    with open(argv[2], "w") as f:
        f.write(text)
    print(text, end="")


if __name__ == "__main__":
    main(sys.argv)
