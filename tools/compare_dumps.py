"""Compare two `bench.py --dump-outputs` directories array by array (two builds, same box, same command line):
the largest absolute difference against the reference's largest entry, and the largest element-wise relative difference
over the entries that are not tiny (|ref| > 1e-3 of the largest).  usage: python tools/compare_dumps.py NEW_DIR REF_DIR"""
import json
import sys
from pathlib import Path

import numpy as np

new_dir, ref_dir = Path(sys.argv[1]), Path(sys.argv[2])
out = {}
for f in sorted(ref_dir.glob("*.npy")):
    a, b = np.load(new_dir / f.name).astype(np.float64), np.load(f).astype(np.float64)
    scale = float(np.abs(b).max()) or 1.0
    big = np.abs(b) > 1e-3 * scale
    out[f.stem] = {"n": int(b.size), "max_abs_ref": scale, "max_abs_diff_over_max_ref": float(np.abs(a - b).max() / scale),
                   "max_elementwise_rel_diff": float((np.abs(a - b)[big] / np.abs(b)[big]).max()) if big.any() else 0.0}
print(json.dumps(out, indent=1))
