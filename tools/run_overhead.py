"""Host overhead of sid_pm_run: 1000 back-to-back run() calls of a 5-launch, 120-point handle (five border classes x 24 points on
a 640 x 640 pair, 34 px, 15 angles - the shape of tests/test_gpu_chained_launches.py test_five_classes), where the kernels are
short and the host work per run (the schedule, the stream waits, the launches) is what shows.

    [SID_PM_LIB=<other library>] python tools/run_overhead.py [--runs 1000] [--blocks 5]

Prints one JSON line per launch order (the short run's own - side by side - and chained, SID_PM_SIDE_BY_SIDE=0): per block of
`runs` calls the median host time of one run() call and the wall time per run including the sync at the end (microseconds).
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sea_ice_drift_amd import _capi, synthetic as syn  # noqa: E402
from sea_ice_drift_amd.pmlib import rotation_table  # noqa: E402


def points(borders=(20, 24, 30, 40, 50), per_class=24):
    n = len(borders) * per_class
    rng = np.random.default_rng(7)
    k = np.arange(n)
    c1 = 90.0 + 46.0 * (k % 11)
    r1 = 90.0 + 46.0 * (k // 11)
    dc, dr = syn.true_displacement(c1, r1)
    c2 = c1 + np.rint(dc) + rng.integers(-2, 3, n)
    r2 = r1 + np.rint(dr) + rng.integers(-2, 3, n)
    border = np.repeat(np.asarray(borders, dtype=np.float64), per_class)[rng.permutation(n)]
    return c1, r1, c2, r2, border


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--runs', type=int, default=1000)
    ap.add_argument('--blocks', type=int, default=5)
    a = ap.parse_args()
    img1, img2 = syn.make_pair(640, 640, seed=31)
    v = points()
    angles = [float(x) for x in range(-7, 8)]
    for order, env in (('side by side', None), ('chained', '0')):
        os.environ.pop('SID_PM_SIDE_BY_SIDE', None)
        if env is not None:
            os.environ['SID_PM_SIDE_BY_SIDE'] = env
        with _capi.PMContext(0) as ctx:
            ctx.upload_pair(img1, img2)
            ctx.set_points(*v, 34, 0.0, angles, rot=rotation_table(angles, 0.0, 34))
            launches = int(ctx.work_info()['launches'])
            for _ in range(50):
                ctx.run()
            ctx.sync()
            call_us, wall_us = [], []
            for _ in range(a.blocks):
                t = np.empty(a.runs)
                t0 = time.perf_counter()
                for i in range(a.runs):
                    t1 = time.perf_counter()
                    ctx.run()
                    t[i] = time.perf_counter() - t1
                ctx.sync()
                wall_us.append(round((time.perf_counter() - t0) / a.runs * 1e6, 2))
                call_us.append(round(float(np.median(t)) * 1e6, 2))
            ctx.check()
        print(json.dumps({'library': os.environ.get('SID_PM_LIB') or 'this tree', 'order': order, 'launches': launches, 'points': int(v[0].size),
                          'runs_per_block': a.runs, 'run_call_us_median': call_us, 'wall_us_per_run': wall_us}))


if __name__ == '__main__':
    main()
