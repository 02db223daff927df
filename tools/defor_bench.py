#!/usr/bin/env python3
"""Timings of sea_ice_drift_amd.libdefor (include/sid_defor.h) on the bench's geometry: the 200 x 200 grid of pattern-matching
points (all nodes: 79 202 triangles) and the same grid with 30 % of the nodes masked.

Per case (median of --reps calls after warm-up):
  device_call_us      get_deformation_on_triangulation on float64 device tensors: host clock around the call (the call
                      returns after its stream is done: it reads the index flag)
  device_events_us    the same call bracketed by HIP events on its stream (kernel + the flag's 4-byte copy, plus the time
                      from the start event to the launch)
  numpy_call_us       NumPy arrays in, NumPy arrays out (copies to and from the device included)
  host_numpy_us       the reference's computation in NumPy on the host (libdefor.py restated operation for operation)
  parity              the NumPy-path outputs equal the host NumPy outputs bit for bit (NaN in the same places)
Kernel time alone: run under `rocprofv3 --kernel-trace --stats` (kernels k_defor_tri<int> / <long>).

    python tools/defor_bench.py [--reps 200] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from sea_ice_drift_amd import libdefor                   # noqa: E402
from tests.golden import make_golden_defor as mg         # noqa: E402


def host_numpy(x, y, u, v, t):
    xt, yt, ut, vt = [i[t].T for i in (x, y, u, v)]
    s = np.hypot(np.diff(np.vstack([xt, xt[0]]), axis=0), np.diff(np.vstack([yt, yt[0]]), axis=0))
    p = np.sum(s, axis=0)
    h = p / 2
    a = np.sqrt(h * (h - s[0]) * (h - s[1]) * (h - s[2]))
    ux = uy = vx = vy = 0
    for i0, i1 in zip([1, 2, 0], [0, 1, 2]):
        ux += (ut[i0] + ut[i1]) * (yt[i0] - yt[i1])
        uy -= (ut[i0] + ut[i1]) * (xt[i0] - xt[i1])
        vx += (vt[i0] + vt[i1]) * (yt[i0] - yt[i1])
        vy -= (vt[i0] + vt[i1]) * (xt[i0] - xt[i1])
    ux, uy, vx, vy = [i / (2 * a) for i in (ux, uy, vx, vy)]
    return ux + vy, ((ux - vy) ** 2 + (uy + vx) ** 2) ** 0.5, vx - uy, a, p


def bench_grid(masked, seed=2001):
    """The bench's 200 x 200 grid of pattern-matching points (50 px apart) in metres at 40 m / px, slightly rotated and
    sheared as a polar-stereographic grid is (x ~ 4e5 .. 8e5, y ~ -1.1e6 .. -0.7e6): every quad is split in two, 79 202
    triangles.  Drift ~0.1 m/s; a fraction `masked` of the nodes left out."""
    rng = np.random.default_rng(seed)
    r, c = np.meshgrid(np.arange(200.0), np.arange(200.0), indexing='ij')
    x, y = 4.0e5 + 2000.0 * c + 30.0 * r, -1.1e6 + 2000.0 * r - 20.0 * c
    u = 0.1 * np.cos(0.05 * r + 0.03 * c) + 0.01 * rng.standard_normal(r.shape)
    v = 0.08 * np.sin(0.04 * r - 0.02 * c) + 0.01 * rng.standard_normal(r.shape)
    keep = rng.random(r.shape) >= masked
    return [a[keep].copy() for a in (x, y, u, v)]


def triangles(x, y, masked):
    try:
        from matplotlib.tri import Triangulation
        return Triangulation(x, y).triangles, 'matplotlib'
    except ImportError:
        if masked:
            return None, 'matplotlib missing'
        i = np.arange(199 * 200).reshape(199, 200)[:, :199].ravel()          # two triangles per quad of the full grid
        return np.concatenate([np.stack([i, i + 1, i + 201], 1), np.stack([i, i + 201, i + 200], 1)]).astype(np.int32), 'structured'


def median_us(fn, reps):
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts) * 1e6)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=200)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    import torch
    res = dict(device=torch.cuda.get_device_name(0), cases=[])
    for name, masked in (('grid200_full', 0.0), ('grid200_masked30', 0.3)):
        x, y, u, v = bench_grid(masked)
        t, how = triangles(x, y, masked)
        if t is None:
            res['cases'].append(dict(case=name, skipped=how))
            continue
        with np.errstate(all='ignore'):
            exp = host_numpy(x, y, u, v, t)
        got = libdefor.get_deformation_on_triangulation(x, y, u, v, t)
        parity = all(mg.same_bits(g, e) for g, e in zip(got, exp))
        dev = [torch.tensor(q, device='cuda') for q in (x, y, u, v, t)]
        for _ in range(20):
            libdefor.get_deformation_on_triangulation(*dev)
        torch.cuda.synchronize()
        device_call = median_us(lambda: libdefor.get_deformation_on_triangulation(*dev), args.reps)
        ev = []
        for _ in range(args.reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            libdefor.get_deformation_on_triangulation(*dev)
            b.record()
            b.synchronize()
            ev.append(a.elapsed_time(b) * 1e3)
        numpy_call = median_us(lambda: libdefor.get_deformation_on_triangulation(x, y, u, v, t), args.reps)
        with np.errstate(all='ignore'):
            host = median_us(lambda: host_numpy(x, y, u, v, t), max(5, args.reps // 10))
        bytes_moved = 8 * 5 * len(t) + t.itemsize * t.size + 4 * 8 * 3 * len(t)        # outputs + t + corner gathers (upper bound)
        res['cases'].append(dict(case=name, nodes=len(x), triangles=len(t), triangulation=how, parity=parity,
                                 device_call_us=round(device_call, 1), device_events_us=round(float(np.median(ev)), 1),
                                 numpy_call_us=round(numpy_call, 1), host_numpy_us=round(host, 1),
                                 kernel_bytes_upper_bound=int(bytes_moved)))
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(line + '\n')
    return 0 if all(c.get('parity', True) for c in res['cases']) else 1


if __name__ == '__main__':
    sys.exit(main())
