#!/usr/bin/env python3
"""Timings of the point map of a drift grid (include/sid_track.h, libtrack.map_points) at Sentinel-1 size: a 200 x 200 node
grid over a 10000 x 10000 frame with synthetic.true_displacement (cells of about 50 x 50 pixels), on device tensors.

Workloads:
    round_trip   40 000 points: the nodes of a second 200 x 200 grid, shifted by half a cell - what a forward-backward check
                 sends through the field.  Also under SID_TRACK_NO_GRID=1 (every cell for every point), for contrast
    lattice8     the lattice at step 8 of the frame: 1250 x 1250 = 1.56 M points
    crop4000     the pixel centres of a 4000 x 4000 crop: 16 M points; in the same loop, alternating with it,
                 libwarp.warp_maps of that crop - the dense lattice is the image warp's own ground
    floor        per workload, a device copy of the same 32 bytes per point (16 read, 16 written)

Per entry: median / p10 / p90 / min / max in microseconds of --reps calls after warm-up, each between two device events on
the stream, and nanoseconds per point.  Parity: a seeded 1 % of each workload against the host instance, bit for bit.
Kernel times alone: run under `rocprofv3 --kernel-trace --stats` with --trace (kernels k_track_boxes, k_track_axes,
k_track_build, k_track_points).

    python tools/track_bench.py [--reps 20] [--out profiles/track_bench.json] [--trace]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from sea_ice_drift_amd import libtrack, libwarp, synthetic           # noqa: E402

SIZE, NODES, CROP = 10000, 200, 4000


def nodes(size, n, offset=0.0):
    """n x n nodes over a size x size frame (moved by `offset` pixels) and where the synthetic field carries them."""
    y, x = np.meshgrid(np.linspace(0.0, size - 1.0, n) + offset, np.linspace(0.0, size - 1.0, n) + offset, indexing='ij')
    dc, dr = synthetic.true_displacement(x, y)
    return [np.ascontiguousarray(q) for q in (x, y, x + dc, y + dr)]


def stats(ts, points):
    ts = np.sort(np.asarray(ts))
    med = float(np.median(ts))
    return dict(median=round(med, 1), p10=round(float(ts[int(0.1 * (len(ts) - 1))]), 1),
                p90=round(float(ts[int(round(0.9 * (len(ts) - 1)))]), 1), min=round(float(ts[0]), 1), max=round(float(ts[-1]), 1),
                reps=len(ts), ns_per_point=round(med * 1e3 / points, 3))


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
            keep = f()
            e1.record()
            e1.synchronize()
            ts[name].append(e0.elapsed_time(e1) * 1e3)
            del keep
    return ts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--out', default=None)
    ap.add_argument('--trace', action='store_true', help='a few device calls only (for a run under rocprofv3)')
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('no GPU: nothing is measured without one')
    reps, warm = (3, 1) if args.trace else (max(args.reps, 20), 3)
    host_grid = nodes(SIZE, NODES)
    grid = [torch.tensor(q, device='cuda') for q in host_grid]
    half = 0.5 * (SIZE - 1.0) / (NODES - 1)
    other = nodes(SIZE - 2 * half, NODES, offset=half)
    step8 = np.arange(0.0, SIZE, 8.0)
    crop = np.arange(0.0, CROP, 1.0)
    workloads = dict(round_trip=(other[2].ravel(), other[3].ravel()),
                     lattice8=[q.ravel() for q in np.meshgrid(step8, step8)],
                     crop4000=[q.ravel() for q in np.meshgrid(crop, crop)])
    res = dict(device=torch.cuda.get_device_name(0), frame=SIZE, nodes=NODES, bytes_per_point=32, workloads={})
    ok = True
    for name, (hx, hy) in workloads.items():
        n = len(hx)
        px, py = torch.tensor(hx, device='cuda'), torch.tensor(hy, device='cuda')
        src, dst = torch.stack([px, py]), torch.empty((2, n), dtype=torch.float64, device='cuda')
        calls = dict(map_points=lambda: libtrack.map_points(*grid, px, py), floor=lambda: dst.copy_(src))
        if name == 'crop4000':
            calls['warp_maps'] = lambda: libwarp.warp_maps(*grid, (CROP, CROP))
        entry = dict(points=n)
        for key, ts in timed(torch, calls, reps, warm).items():
            entry[key] = stats(ts, n)
        if name == 'round_trip':
            os.environ['SID_TRACK_NO_GRID'] = '1'
            try:
                entry['map_points_every_cell'] = stats(timed(torch, dict(m=calls['map_points']), reps, warm)['m'], n)
            finally:
                del os.environ['SID_TRACK_NO_GRID']
        if 'warp_maps' in entry:
            entry['map_points_over_warp_maps'] = round(entry['map_points']['median'] / entry['warp_maps']['median'], 2)
        entry['map_points_over_floor'] = round(entry['map_points']['median'] / entry['floor']['median'], 2)
        if not args.trace:
            sel = np.sort(np.random.default_rng(11).choice(n, max(n // 100, 1), replace=False))
            exp = libtrack.map_points(*host_grid, hx[sel], hy[sel], return_triangle=True, device=-1)
            dsel = torch.from_numpy(sel).cuda()
            got = libtrack.map_points(*grid, px[dsel], py[dsel], return_triangle=True)
            entry['parity'] = all(e.tobytes() == g.cpu().numpy().tobytes() for e, g in zip(exp, got))
            entry['parity_points'], entry['parity_inside'] = len(sel), int((exp[2] >= 0).sum())
            ok = ok and entry['parity']
        res['workloads'][name] = entry
        del px, py, src, dst
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(line + '\n')
    return 0 if ok else 1


if __name__ == '__main__':
    sys.exit(main())
