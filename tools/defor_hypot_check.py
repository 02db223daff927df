#!/usr/bin/env python3
"""Bit-for-bit check of the deformation kernel's float64 hypot (csrc/defor_hypot.h) against NumPy's np.hypot (libm).

    python tools/defor_hypot_check.py [--pairs 100000000] [--device -1]

--device -1 (default) evaluates the host instance of the same source, no GPU needed; --device N the kernel on HIP device N.
The pairs come from tests/golden/make_golden_defor.hypot_pairs (bit patterns with NaN / inf / subnormals, wide ratios,
near-equal magnitudes, both scaling thresholds) in chunks of 2^22 with seeds 0, 1, 2, ...  Prints one JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from sea_ice_drift_amd import _capi                      # noqa: E402
from tests.golden import make_golden_defor as mg         # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--pairs', type=int, default=100_000_000)
    ap.add_argument('--device', type=int, default=-1)
    args = ap.parse_args()
    chunk = 1 << 22
    done = mism = 0
    first = None
    t0 = time.time()
    seed = 0
    while done < args.pairs:
        n = min(chunk, args.pairs - done)
        x, y = mg.hypot_pairs(n, seed)
        got = _capi.defor_debug_hypot(x, y, device=args.device)
        with np.errstate(all='ignore'):
            exp = np.hypot(x, y)
        bad = ~((got.view(np.int64) == exp.view(np.int64)) | (np.isnan(got) & np.isnan(exp)))
        if bad.any() and first is None:
            i = int(np.flatnonzero(bad)[0])
            first = dict(x=float.hex(float(x[i])), y=float.hex(float(y[i])), got=float.hex(float(got[i])), exp=float.hex(float(exp[i])))
        mism += int(bad.sum())
        done += n
        seed += 1
    print(json.dumps(dict(pairs=done, mismatches=mism, device=args.device, seconds=round(time.time() - t0, 1), first_mismatch=first)))
    return 0 if mism == 0 else 1


if __name__ == '__main__':
    sys.exit(main())
