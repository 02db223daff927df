#!/usr/bin/env python3
"""Timings of the pattern-matching prelude with the reference's first guess (method='linear': Delaunay triangulation on the
host, point location on the device) and with the triangulation-free one (method='knn', include/sid_fg.h sid_fg_knn) on the
bench's workload: 10000 x 10000 images, 20 000 key points, the 200 x 200 grid of bench.py.

Median / p10 / p90 / min / max in microseconds, host clock around calls that end in a device synchronise (the entry points
copy their results back to host arrays), 20 warm-up calls, then --reps calls (a fifth of them for the Qhull route):
  prelude_linear   pmlib.pm_prelude(..., first_guess_on='device'): the triangulation is paid in the call
                   (SID_NO_TRI_PREFETCH=1 is set: nothing is prefetched anywhere)
  prelude_knn      pmlib.pm_prelude(..., method='knn', first_guess_on='device')
  fg_knn_k1/5/16   _capi.fg_knn alone (40 000 queries, 20 000 seeds)
  parity           the device result equals the library's host instance (device = -1) bit for bit, k = 5 and 16
Kernel times alone: run under `rocprofv3 --kernel-trace --stats` with --trace (kernels k_knn_grid, k_seed_bin, k_grid_scan).

    python tools/first_guess_bench.py [--reps 50] [--out profiles/first_guess_bench.json] [--trace]
"""
import argparse
import hashlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ['SID_NO_TRI_PREFETCH'] = '1'

from sea_ice_drift_amd import _capi, pmlib, synthetic as syn           # noqa: E402
from sea_ice_drift_amd.domain import ArrayNansat                       # noqa: E402

SIZE, GRID, N_KP = 10000, 200, 20000


def workload(seed=2002):
    """bench.py --mode ftpm's georeference and grid; key points as feature tracking delivers them there (uniform, true
    displacement + N(0, 1) px).  The prelude reads the images' shapes only."""
    rng = np.random.default_rng(seed)
    img = np.zeros((SIZE, SIZE), dtype=np.uint8)
    scale = 4e-4
    n1 = ArrayNansat(img, origin=(10.0, 80.0), matrix=((scale, 0.0), (0.0, -scale)))
    n2 = ArrayNansat(img, origin=(10.0, 80.0), matrix=((scale, 0.0), (0.0, -scale)))
    cg, rg = np.meshgrid(np.rint(np.linspace(100, SIZE - 101, GRID)), np.rint(np.linspace(100, SIZE - 101, GRID)))
    lon, lat = n1.transform_points(cg.ravel(), rg.ravel(), 0)
    c1, r1 = rng.uniform(0, SIZE, N_KP), rng.uniform(0, SIZE, N_KP)
    dc, dr = syn.true_displacement(c1, r1)
    c2 = np.clip(c1 + dc + rng.normal(0, 1, N_KP), 0, SIZE - 1)
    r2 = np.clip(r1 + dr + rng.normal(0, 1, N_KP), 0, SIZE - 1)
    return n1, n2, lon.reshape(cg.shape), lat.reshape(cg.shape), c1, r1, c2, r2


def stats_us(fn, reps):
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e6)
    ts = np.sort(ts)
    return dict(median=round(float(np.median(ts)), 1), p10=round(float(ts[int(0.1 * (len(ts) - 1))]), 1),
                p90=round(float(ts[int(round(0.9 * (len(ts) - 1)))]), 1), min=round(float(ts[0]), 1), max=round(float(ts[-1]), 1),
                reps=len(ts))


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype.kind != 'f':
        return bool(np.array_equal(a, b))
    return bool(np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(a[~np.isnan(a)].view(np.int64), b[~np.isnan(b)].view(np.int64)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=50)
    ap.add_argument('--out', default=None)
    ap.add_argument('--trace', action='store_true', help='a few _capi.fg_knn calls only (for a run under rocprofv3)')
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('no GPU: nothing is measured without one')
    n1, n2, lon, lat, c1, r1, c2, r2 = workload()
    seeds, vals = np.stack([r1, c1], axis=1), np.stack([c2 - c1, r2 - r1], axis=1)
    q = np.stack(n2.transform_points(lon.ravel(), lat.ravel(), 1)[::-1], axis=1)
    if args.trace:
        for k in (1, 5, 16):
            for _ in range(10):
                _capi.fg_knn(seeds, vals, q, k=k)
        return 0
    with open(_capi.LIB_PATH, 'rb') as f:
        md5 = hashlib.md5(f.read()).hexdigest()
    res = dict(device=torch.cuda.get_device_name(0), library_md5=md5, key_points=N_KP, grid_points=GRID * GRID, size=SIZE)

    def prelude(**kw):
        return pmlib.pm_prelude(lon, lat, n1, c1, r1, n2, c2, r2, img_size=34, first_guess_on='device', **kw)
    calls = dict(prelude_linear=(prelude, max(10, args.reps // 5)), prelude_knn=(lambda: prelude(method='knn'), args.reps))
    for k in (1, 5, 16):
        calls['fg_knn_k%d' % k] = (lambda k=k: _capi.fg_knn(seeds, vals, q, k=k), args.reps)
    for key, (fn, reps) in calls.items():
        for _ in range(20):
            fn()
        res[key + '_us'] = stats_us(fn, reps)
    res['parity'] = all(all(same(g, e) for g, e in zip(_capi.fg_knn(seeds, vals, q, k=k, details=True),
                                                       _capi.fg_knn(seeds, vals, q, k=k, details=True, device=-1))) for k in (5, 16))
    res['prelude_linear_over_knn'] = round(res['prelude_linear_us']['median'] / res['prelude_knn_us']['median'], 2)
    lin, knn = prelude(), prelude(method='knn')
    res['first_guess_differs_by_px'] = dict(median=float(np.median(np.hypot(lin['c2fg'] - knn['c2fg'], lin['r2fg'] - knn['r2fg']))),
                                            max=float(np.max(np.hypot(lin['c2fg'] - knn['c2fg'], lin['r2fg'] - knn['r2fg']))))
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(line + '\n')
    return 0 if res['parity'] and res['prelude_knn_us']['median'] < res['prelude_linear_us']['median'] else 1


if __name__ == '__main__':
    sys.exit(main())
