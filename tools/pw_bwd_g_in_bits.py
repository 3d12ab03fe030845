"""g_in of the pointwise backward kernel, as stored, for every case of tests/test_pw_bwd_tiles.py -- to compare two builds bit for bit:
    python tools/pw_bwd_g_in_bits.py NEW.npz
    WW_AB_LIB=other/libwwhip.so python tools/ab_lib.py tools/pw_bwd_g_in_bits.py REF.npz
    python tools/pw_bwd_g_in_bits.py NEW.npz REF.npz        # compares, prints one line per case, exit 1 on any difference"""
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

if len(sys.argv) == 2:
    from tests.test_pw_bwd_tiles import dump_g_in
    dump_g_in(sys.argv[1])
else:
    a, b = np.load(sys.argv[1]), np.load(sys.argv[2])
    bad = 0
    for k in b.files:
        n = int((a[k] != b[k]).sum())
        bad += n
        print(f"{k}: {b[k].size} values, {n} differ")
    sys.exit(1 if bad else 0)
