#!/usr/bin/env python3
"""Timings of the drift-grid chain (include/sid_grid.h) on tools/defor_bench.py's geometry: the 200 x 200 grid of
pattern-matching points, once with all nodes and once with 30 % of them masked.

Per case, median / p10 / p90 / min / max in microseconds of --reps calls after warm-up (host clock around work that ends in a
device synchronise):
  route_a_triangulation   matplotlib.tri.Triangulation of the valid nodes (host, Qhull)            } the parent's route:
  route_a_deformation     libdefor.get_deformation_on_triangulation, NumPy in / out, on them       } get_deformation_nodes
  route_b_chain           normalized_median_test + get_deformation_grid(valid=keep), device tensors in and out
  filter_r1, filter_r2    normalized_median_test alone (radius 1, 2), device tensors
  deformation_grid        get_deformation_grid alone, device tensors
  chain_numpy             the chain with NumPy arrays in and out (copies included)
  parity                  the device results equal the host instance of the same source (device = -1) bit for bit
Kernel times alone: run under `rocprofv3 --kernel-trace --stats` with --trace (kernels k_grid_filter, k_grid_defor).

    python tools/grid_bench.py [--reps 200] [--out profiles/grid_bench.json] [--trace]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from sea_ice_drift_amd import _capi, libdefor, libfilter           # noqa: E402

EPS = 0.01           # m/s: the noise the bench's field carries


def grid2d(masked, seed=2001):
    """tools/defor_bench.bench_grid before its mask is applied: x, y, u, v (200, 200) and the mask."""
    rng = np.random.default_rng(seed)
    r, c = np.meshgrid(np.arange(200.0), np.arange(200.0), indexing='ij')
    x, y = 4.0e5 + 2000.0 * c + 30.0 * r, -1.1e6 + 2000.0 * r - 20.0 * c
    u = 0.1 * np.cos(0.05 * r + 0.03 * c) + 0.01 * rng.standard_normal(r.shape)
    v = 0.08 * np.sin(0.04 * r - 0.02 * c) + 0.01 * rng.standard_normal(r.shape)
    return x, y, u, v, rng.random(r.shape) >= masked


def stats_us(fn, reps, sync=None):
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        if sync:
            sync()
        ts.append((time.perf_counter() - t0) * 1e6)
    ts = np.sort(ts)
    return dict(median=round(float(np.median(ts)), 1), p10=round(float(ts[int(0.1 * (len(ts) - 1))]), 1),
                p90=round(float(ts[int(round(0.9 * (len(ts) - 1)))]), 1), min=round(float(ts[0]), 1), max=round(float(ts[-1]), 1),
                reps=len(ts))


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype.kind != 'f':
        return bool(np.array_equal(a.astype(np.int64), b.astype(np.int64)))
    return bool(np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(a[~np.isnan(a)].view(np.int64), b[~np.isnan(b)].view(np.int64)))


def host_instance(x, y, u, v, valid):
    vv = np.ascontiguousarray(valid).view(np.uint8)
    keep, res = _capi.grid_filter(u, v, vv, EPS, 2.0, 1, 3, device=-1)
    return (keep, res) + _capi.grid_deformation(x, y, u, v, keep, _capi.GRID_DIAGONALS['shorter'], device=-1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=200)
    ap.add_argument('--out', default=None)
    ap.add_argument('--trace', action='store_true', help='device-tensor calls only (for a run under rocprofv3)')
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('no GPU: nothing is measured without one')
    sync = torch.cuda.synchronize
    res = dict(device=torch.cuda.get_device_name(0), eps=EPS, cases=[])
    for name, masked in (('grid200_full', 0.0), ('grid200_masked30', 0.3)):
        x, y, u, v, valid = grid2d(masked)
        dev = [torch.tensor(q, device='cuda') for q in (x, y, u, v, valid)]

        def chain():
            keep, _ = libfilter.normalized_median_test(dev[2], dev[3], EPS, valid=dev[4])
            return libdefor.get_deformation_grid(*dev[:4], valid=keep)

        calls = dict(route_b_chain=chain,
                     filter_r1=lambda: libfilter.normalized_median_test(dev[2], dev[3], EPS, valid=dev[4]),
                     filter_r2=lambda: libfilter.normalized_median_test(dev[2], dev[3], EPS, valid=dev[4], radius=2),
                     deformation_grid=lambda: libdefor.get_deformation_grid(*dev[:4], valid=dev[4]))
        case = dict(case=name, nodes=int(valid.sum()), rows=200, cols=200)
        for key, fn in calls.items():
            for _ in range(20):
                fn()
            sync()
            case[key + '_us'] = stats_us(fn, args.reps, sync)
        if not args.trace:
            keep_d, res_d = libfilter.normalized_median_test(dev[2], dev[3], EPS, valid=dev[4])
            got = [keep_d.cpu().numpy(), res_d.cpu().numpy()] + [o.cpu().numpy() for o in libdefor.get_deformation_grid(*dev[:4], valid=keep_d)]
            case['parity'] = all(same(g, e) for g, e in zip(got, host_instance(x, y, u, v, valid)))
            case['kept'] = int(got[0].sum())
            case['triangles'] = int((got[7][..., 0] >= 0).sum())

            def chain_numpy():
                keep, _ = libfilter.normalized_median_test(u, v, EPS, valid=valid)
                return libdefor.get_deformation_grid(x, y, u, v, valid=keep)
            for _ in range(5):
                chain_numpy()
            case['chain_numpy_us'] = stats_us(chain_numpy, args.reps)
            try:
                from matplotlib.tri import Triangulation
                xs, ys, us, vs = [np.ascontiguousarray(q[valid]) for q in (x, y, u, v)]
                tri = Triangulation(xs, ys).triangles
                case['route_a_triangles'] = int(len(tri))
                case['route_a_triangulation_us'] = stats_us(lambda: Triangulation(xs, ys).triangles, max(5, args.reps // 20))
                for _ in range(5):
                    libdefor.get_deformation_on_triangulation(xs, ys, us, vs, tri)
                case['route_a_deformation_us'] = stats_us(lambda: libdefor.get_deformation_on_triangulation(xs, ys, us, vs, tri), args.reps)
            except ImportError:
                case['route_a'] = 'matplotlib missing'
        res['cases'].append(case)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(line + '\n')
    return 0 if all(c.get('parity', True) for c in res['cases']) else 1


if __name__ == '__main__':
    sys.exit(main())
