#!/usr/bin/env python3
"""Timings of the guided matcher (include/sid_ftg.h) beside the brute-force matcher (include/sid_ft.h) on the same descriptors.

Workload: 100 000 x 100 000 random 256-bit descriptors on a 5000 x 5000 frame; half of the queries are planted pairs - a copy of
a train descriptor with up to 40 bits flipped, predicted within 30 px of it.  The guided call runs at radii 50, 135 and 540 px
(135 px: max_speed = 0.5 m/s over six hours at 80 m pixels; 540 px: over a day), ALTERNATING in the same loop with sid_ft_knn2,
all on device tensors through the _device entries (no copies in the timed window), each call between two device events.

Per entry: median / p10 / p90 / min / max in microseconds of --reps calls after warm-up; per radius the candidates per query
(mean, max), the planted pairs whose partner is the nearest candidate, the time over sid_ft_knn2's, and parity - idx, dist and
count of a seeded sample of queries against the specification (tests/ft_guided_spec.py), bit for bit.

    python tools/ft_guided_bench.py [--reps 20] [--n 100000] [--out profiles/ft_guided_bench.json]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from sea_ice_drift_amd import _capi                                  # noqa: E402
from tests import ft_guided_spec as gs                               # noqa: E402

FRAME, RADII, SAMPLE = 5000.0, (50.0, 135.0, 540.0), 200


def workload(n, seed=26):
    rng = np.random.default_rng(seed)
    d2 = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    t = rng.uniform(0.0, FRAME, (n, 2))
    d1 = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    q = rng.uniform(0.0, FRAME, (n, 2))
    pairs = n // 2
    partner = rng.permutation(n)[:pairs]
    flips = rng.random((pairs, 256)) < (rng.integers(0, 41, (pairs, 1)) / 256.0)
    d1[:pairs] = d2[partner] ^ np.packbits(flips, axis=1)
    q[:pairs] = t[partner] + rng.uniform(-21.0, 21.0, (pairs, 2))      # (within 30 px)
    return d1, q, d2, t, partner


def stats(ts):
    ts = np.sort(np.asarray(ts))
    return dict(median=round(float(np.median(ts)), 1), p10=round(float(ts[int(0.1 * (len(ts) - 1))]), 1),
                p90=round(float(ts[int(round(0.9 * (len(ts) - 1)))]), 1), min=round(float(ts[0]), 1), max=round(float(ts[-1]), 1), reps=len(ts))


def timed(torch, calls, reps, warm):
    """Every call of `calls` (name -> function) `reps` times, alternating, each between two device events -> name -> [us]."""
    for _ in range(warm):
        for f in calls.values():
            f()
    torch.cuda.synchronize()
    ts = {name: [] for name in calls}
    for _ in range(reps):
        for name, f in calls.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            f()
            e1.record()
            e1.synchronize()
            ts[name].append(e0.elapsed_time(e1) * 1e3)
    return ts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--n', type=int, default=100000)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('no GPU: nothing is measured without one')
    n = args.n
    d1, q, d2, t, partner = workload(n)
    dev = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (d1, q[:, 0], q[:, 1], d2, t[:, 0], t[:, 1])]
    stream = torch.cuda.current_stream().cuda_stream
    ws_ft = torch.empty(_capi.ft_workspace_bytes(n, n), dtype=torch.uint8, device='cuda')
    ws_ftg = torch.empty(_capi.ftg_workspace_bytes(n, n), dtype=torch.uint8, device='cuda')
    out = {name: (torch.empty((n, 2), dtype=torch.int32, device='cuda'), torch.empty((n, 2), dtype=torch.int32, device='cuda'),
                  torch.empty(n, dtype=torch.int32, device='cuda')) for name in ['ft_knn2'] + ['guided_%g' % r for r in RADII]}

    def brute():
        idx, dist, _ = out['ft_knn2']
        _capi.ft_knn2_device(dev[0].data_ptr(), n, dev[3].data_ptr(), n, idx.data_ptr(), dist.data_ptr(), ws_ft.data_ptr(), stream)

    def guided(radius):
        idx, dist, count = out['guided_%g' % radius]
        return lambda: _capi.ftg_knn2_device(dev[0].data_ptr(), dev[1].data_ptr(), dev[2].data_ptr(), n, dev[3].data_ptr(), dev[4].data_ptr(),
                                             dev[5].data_ptr(), n, radius, idx.data_ptr(), dist.data_ptr(), count.data_ptr(), ws_ftg.data_ptr(), stream)
    calls = dict(ft_knn2=brute)
    calls.update({'guided_%g' % r: guided(r) for r in RADII})
    ts = timed(torch, calls, max(args.reps, 20), 3)
    res = dict(device=torch.cuda.get_device_name(0), n1=n, n2=n, frame=FRAME, planted_pairs=len(partner), entries={},
               workspace_bytes=dict(ft_knn2=int(ws_ft.numel()), guided=int(ws_ftg.numel())))
    res['entries']['ft_knn2'] = stats(ts['ft_knn2'])
    sel = np.sort(np.random.default_rng(11).choice(n, min(SAMPLE, n), replace=False))
    fidx = out['ft_knn2'][0].cpu().numpy()
    res['entries']['ft_knn2']['planted_nearest'] = int((fidx[:len(partner), 0] == partner).sum())
    ok = True
    for r in RADII:
        name = 'guided_%g' % r
        idx, dist, count = (a.cpu().numpy() for a in out[name])
        entry = stats(ts[name])
        entry['over_ft_knn2'] = round(entry['median'] / res['entries']['ft_knn2']['median'], 3)
        entry['candidates_mean'], entry['candidates_max'] = round(float(count.mean()), 1), int(count.max())
        entry['planted_nearest'] = int((idx[:len(partner), 0] == partner).sum())
        eidx, edist, ecount = gs.knn2(d1[sel], q[sel, 0], q[sel, 1], d2, t[:, 0], t[:, 1], r, chunk=32)
        entry['parity'] = bool((idx[sel] == eidx).all() and (dist[sel] == edist).all() and (count[sel] == ecount).all())
        entry['parity_queries'] = len(sel)
        ok = ok and entry['parity']
        res['entries'][name] = entry
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(line + '\n')
    return 0 if ok else 1


if __name__ == '__main__':
    sys.exit(main())
