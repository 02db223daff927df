#!/usr/bin/env python3
"""One pm_dispatch call on 1, 2, 4 and 8 device handles (``devices=`` of sea_ice_drift_amd.pmlib), pair resident.

The benchmark's grid (``synthetic.make_pair(10000, 10000)``, ``make_grid(..., 200)``: 40 000 points) in two
configurations: 34 px / 15 angles (bench.py) and the reference's defaults, 35 px / 3 angles.  For ``devices=None``,
``devices=[0]`` and 1, 2, 4, 8 handles spread round-robin over the visible GPUs:

* median, minimum, maximum and inter-quartile range of ``--calls`` (>= 20) timed calls after ``--warmup`` calls, the
  configurations taken in turn within every round so that a drift of the machine hits all of them alike; a call ends in
  the fetch of the last shard, i.e. after a device synchronise;
* the split of a call into shard plan, set_points, run (enqueue), wait for the kernels, fetch and merge, from a few
  calls with ``timings=`` (these carry one extra synchronise per handle and are not among the timed calls);
* the same split with one worker thread per handle doing set_points + run (``threaded_dispatch``: does it pay?);
* ``distinct_devices`` and ``shared_device`` (handles outnumber GPUs: the figure is then the OVERHEAD of several handles
  on one device and says nothing about scaling).

``devices=[0]`` is the code path of ``devices=None``; the tool checks that its median lies within the spread it measured
for ``devices=None`` (``one_handle_list_within_spread_of_none``) and exits with status 1 if it does not.

Writes ONE JSON line to profiles/multi_device_bench.json (``--out``) and prints it.  Needs a GPU; there is no fallback.
"""
import argparse
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from sea_ice_drift_amd import _capi, pmlib, synthetic as syn  # noqa: E402

NAMES = ('c1', 'r1', 'c2fg', 'r2fg', 'border')


def stats(ms):
    ms = np.asarray(ms, dtype=np.float64)
    q1, med, q3 = np.percentile(ms, [25, 50, 75])
    return dict(median_ms=round(float(med), 3), min_ms=round(float(ms.min()), 3), max_ms=round(float(ms.max()), 3),
                iqr_ms=round(float(q3 - q1), 3), calls=int(ms.size))


def threaded_dispatch(devs, v, img_size, angles):
    """The dispatch of pmlib._dispatch_sharded with set_points + run of every handle on a worker thread of its own
    (both are C calls that release the interpreter lock) -> milliseconds of one call.  Only measured here."""
    ang, flags = pmlib._sweep_options(dict(angles=angles))
    rot = pmlib.rotation_table(ang, 0.0, img_size)
    with pmlib._Handles(devs) as ctxs:
        t0 = time.perf_counter()
        shards = pmlib.plan_shards(v[4], len(ctxs), img_size, len(ang), flags)
        work = [(c, i) for c, i in zip(ctxs, shards) if i.size]

        def start(ci):
            ci[0].set_points(*[x[ci[1]] for x in v], img_size, 0.0, ang, rot=rot, flags=flags)
            ci[0].run()
        with ThreadPoolExecutor(max_workers=len(work)) as pool:
            list(pool.map(start, work))
        out = np.empty((v[0].size, 5))
        for c, i in work:
            out[i] = c.fetch(want_ij=False)
        return (time.perf_counter() - t0) * 1e3, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--size', type=int, default=10000)
    ap.add_argument('--grid', type=int, default=200)
    ap.add_argument('--calls', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--handles', type=int, nargs='+', default=[1, 2, 4, 8])
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'multi_device_bench.json'))
    a = ap.parse_args()
    if a.calls < 20:
        ap.error('--calls: at least 20 timed calls')
    n_gpus = _capi.device_count()
    if n_gpus < 1:
        raise SystemExit('no GPU visible: this tool measures on the device only')
    img1, img2 = syn.make_pair(a.size, a.size)
    g = syn.make_grid(a.size, a.size, a.grid)
    v = [g[k] for k in NAMES]
    configs = [('devices=None', None), ('devices=[0]', [0])]
    configs += [('%d handles' % h, [k % n_gpus for k in range(h)]) for h in a.handles if h > 1]
    res = dict(tool='tools/multi_device_bench.py', size=a.size, points=int(v[0].size), visible_gpus=n_gpus, warmup=a.warmup,
               workloads=[])
    ok = True
    for img_size, angles in ((34, list(range(-7, 8))), (35, [-3, 0, 3])):
        kw = dict(angles=angles)
        ref = pmlib.pm_dispatch(img1, img2, *v, img_size, 0.0, **kw)              # uploads to handle (0, 0)
        rows = []
        for name, devs in configs:                                                # upload to every handle, warm up, check
            got = pmlib.pm_dispatch(img1, img2, *v, img_size, 0.0, devices=devs, **kw)
            if not np.array_equal(got, ref, equal_nan=True):
                raise SystemExit('%s: results differ from devices=None' % name)
            for _ in range(a.warmup):
                pmlib.pm_dispatch(None, None, *v, img_size, 0.0, devices=devs, **kw)
            rows.append(dict(config=name, devices=devs, handles=1 if devs is None else len(devs),
                             distinct_devices=1 if devs is None else len(set(devs)),
                             shared_device=devs is not None and len(devs) > len(set(devs)), ms=[]))
        for _ in range(a.calls):                                                  # the configurations in turn, every round
            for row in rows:
                t0 = time.perf_counter()
                pmlib.pm_dispatch(None, None, *v, img_size, 0.0, devices=row['devices'], **kw)
                row['ms'].append((time.perf_counter() - t0) * 1e3)
        for row in rows:
            row.update(stats(row.pop('ms')))
            devs = row['devices']
            if devs is not None and len(devs) > 1:
                split = []
                for _ in range(5):
                    t = {}
                    pmlib.pm_dispatch(None, None, *v, img_size, 0.0, devices=devs, timings=t, **kw)
                    split.append(t)
                row['split_ms'] = {k: round(float(np.median([s[k] for s in split])) * 1e3, 3)
                                   for k in ('plan', 'set_points', 'run', 'kernel_wait', 'fetch', 'merge')}
                row['points_per_handle'] = split[0]['points_per_handle']
                th = []
                for k in range(3 + 7):
                    ms, got = threaded_dispatch(devs, v, img_size, angles)
                    if not np.array_equal(got, ref, equal_nan=True):
                        raise SystemExit('%s (threaded): results differ from devices=None' % row['config'])
                    th.append(ms)
                row['threaded_dispatch_median_ms'] = round(float(np.median(th[3:])), 3)
            else:                                                                 # the one handle: the same stages by hand
                ctx, lock = pmlib._shared_context(0)
                ang, flags = pmlib._sweep_options(dict(kw))
                rot = pmlib.rotation_table(ang, 0.0, img_size)
                split = []
                with lock:
                    for _ in range(5):
                        t0 = time.perf_counter()
                        ctx.set_points(*v, img_size, 0.0, ang, rot=rot, flags=flags)
                        t1 = time.perf_counter()
                        ctx.run()
                        t2 = time.perf_counter()
                        ctx.sync()
                        t3 = time.perf_counter()
                        ctx.fetch(want_ij=False)
                        split.append((t1 - t0, t2 - t1, t3 - t2, time.perf_counter() - t3))
                m = np.median(np.array(split), axis=0) * 1e3
                row['split_ms'] = dict(plan=0.0, set_points=round(float(m[0]), 3), run=round(float(m[1]), 3),
                                       kernel_wait=round(float(m[2]), 3), fetch=round(float(m[3]), 3), merge=0.0)
        none, one = rows[0], rows[1]
        lo, hi = none['min_ms'], none['max_ms']
        within = lo <= one['median_ms'] <= hi                                      # the spread: fastest .. slowest call
        ok = ok and within
        res['workloads'].append(dict(img_size=img_size, n_angles=len(angles), configs=rows,
                                     none_median_ms=none['median_ms'], none_spread_ms=[lo, hi], none_iqr_ms=none['iqr_ms'],
                                     one_handle_list_median_ms=one['median_ms'], one_handle_list_iqr_ms=one['iqr_ms'],
                                     one_handle_list_within_spread_of_none=bool(within)))
    distinct = max(r['distinct_devices'] for w in res['workloads'] for r in w['configs'])
    res['max_distinct_devices'] = distinct
    res['note'] = ('several GPUs were used: see distinct_devices per configuration' if distinct > 1 else
                   'ONE GPU was visible: every multi-handle figure is the overhead of several handles sharing one device; '
                   'no speed-up over one handle has been measured')
    line = json.dumps(res)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write(line + '\n')
    print(line)
    pmlib.release_contexts()
    return 0 if ok else 1


if __name__ == '__main__':
    sys.exit(main())
