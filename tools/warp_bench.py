#!/usr/bin/env python3
"""Timings of the piecewise-affine warp (include/sid_warp.h, libwarp) at Sentinel-1 size: a 10000 x 10000 uint8 source on
device tensors, resampled with synthetic.true_displacement on a 200 x 200 node grid (cells of 50 x 50 pixels) and on a 5 x 5
node grid (cells of 2500 x 2500 pixels: the same pixels, 1600 times fewer cells), order 0 and 1, image alone and image + maps.

Per case: median / p10 / p90 / min / max in microseconds of --reps calls after warm-up, each between two device events on the
stream; the algorithmic bytes from the shapes (fill pass: every wanted output written once; walk: the source read once, every
wanted output written once more where a triangle owns the pixel) and their rate as a share of the HBM peak (8.0 TB/s
specified, 6.29 TB/s measured with a float4 copy).  The result is checked against the host instance on a 300 x 300 corner.
For contrast the same job at 2000 x 2000 on the host: matplotlib's LinearTriInterpolator for the maps, SciPy's
map_coordinates for the image.
Kernel times alone: run under `rocprofv3 --kernel-trace --stats` with --trace (kernels k_warp_fill, k_warp_count,
k_warp_scan, k_warp_walk).

    python tools/warp_bench.py [--reps 20] [--size 10000] [--out profiles/warp_bench.json] [--trace]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from sea_ice_drift_amd import libwarp, synthetic           # noqa: E402

HBM_SPEC, HBM_COPY = 8.0e12, 6.29e12


def nodes(size, n):
    """n x n nodes over a size x size image and where the synthetic field carries them."""
    y, x = np.meshgrid(np.linspace(0.0, size - 1.0, n), np.linspace(0.0, size - 1.0, n), indexing='ij')
    dc, dr = synthetic.true_displacement(x, y)
    return [np.ascontiguousarray(q) for q in (x, y, x + dc, y + dr)]


def stats(ts):
    ts = np.sort(np.asarray(ts))
    return dict(median=round(float(np.median(ts)), 1), p10=round(float(ts[int(0.1 * (len(ts) - 1))]), 1),
                p90=round(float(ts[int(round(0.9 * (len(ts) - 1)))]), 1), min=round(float(ts[0]), 1), max=round(float(ts[-1]), 1),
                reps=len(ts))


def algorithmic_bytes(size, maps):
    n = size * size
    fill = n + (8 * n if maps else 0)
    walk = n + n + (8 * n if maps else 0)
    return dict(fill_pass=fill, walk_read_source=n, walk_write=walk - n, total=fill + walk)


def host_contrast(size, n):
    from matplotlib.tri import LinearTriInterpolator, Triangulation
    from scipy import ndimage as nd
    x, y, xs, ys = nodes(size, n)
    img = np.random.default_rng(3).integers(1, 256, size=(size, size), dtype=np.uint8)
    t0 = time.perf_counter()
    tri = Triangulation(x.ravel(), y.ravel())
    rr, cc = np.meshgrid(np.arange(size, dtype=np.float64), np.arange(size, dtype=np.float64), indexing='ij')
    mx = LinearTriInterpolator(tri, xs.ravel())(cc, rr)
    my = LinearTriInterpolator(tri, ys.ravel())(cc, rr)
    t1 = time.perf_counter()
    nd.map_coordinates(img, [np.ma.filled(my, -1.0), np.ma.filled(mx, -1.0)], order=1, mode='constant')
    t2 = time.perf_counter()
    return dict(size=size, nodes=n, maps_seconds=round(t1 - t0, 3), resample_seconds=round(t2 - t1, 3), total_seconds=round(t2 - t0, 3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--size', type=int, default=10000)
    ap.add_argument('--out', default=None)
    ap.add_argument('--trace', action='store_true', help='a few device calls only (for a run under rocprofv3)')
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('no GPU: nothing is measured without one')
    size = args.size
    gen = torch.Generator(device='cuda').manual_seed(5)
    img = torch.randint(1, 256, (size, size), dtype=torch.uint8, device='cuda', generator=gen)
    res = dict(device=torch.cuda.get_device_name(0), size=size, hbm_peak_spec=HBM_SPEC, hbm_peak_copy=HBM_COPY, cases=[])
    ok = True
    for n in (200, 5):
        host_nodes = nodes(size, n)
        dev = [torch.tensor(q, device='cuda') for q in host_nodes]
        for order in (0, 1):
            for maps in (False, True):
                def call():
                    return libwarp._run(img, *dev, (size, size), None, order, 0, 'shorter', None, True, False, maps, 0)
                reps = 3 if args.trace else args.reps
                for _ in range(1 if args.trace else 3):
                    call()
                torch.cuda.synchronize()
                ts = []
                for _ in range(reps):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    out = call()
                    e1.record()
                    e1.synchronize()
                    ts.append(e0.elapsed_time(e1) * 1e3)
                nbytes = algorithmic_bytes(size, maps)
                case = dict(nodes=n, order=order, maps=maps, time_us=stats(ts), bytes=nbytes)
                rate = nbytes['total'] / (case['time_us']['median'] * 1e-6)
                case.update(bytes_per_second=round(rate, -6), share_of_hbm_spec=round(rate / HBM_SPEC, 4),
                            share_of_hbm_copy=round(rate / HBM_COPY, 4))
                if not args.trace:
                    k = min(300, size)                                # parity on a corner: the host loop is slow
                    exp = libwarp._run(img[:k + 40, :k + 40].cpu().numpy(), *host_nodes, (k, k), None, order, 0, 'shorter', None,
                                       True, False, maps, -1)
                    got = libwarp._run(img[:k + 40, :k + 40].contiguous(), *dev, (k, k), None, order, 0, 'shorter', None, True,
                                       False, maps, 0)
                    case['parity'] = all(e is None or e.tobytes() == g.cpu().numpy().tobytes() for e, g in zip(exp, got))
                    ok = ok and case['parity']
                del out
                res['cases'].append(case)
    if not args.trace:
        try:
            res['host_contrast'] = host_contrast(2000, 40)
        except ImportError as e:
            res['host_contrast'] = 'missing: %s' % e
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(line + '\n')
    return 0 if ok else 1


if __name__ == '__main__':
    sys.exit(main())
