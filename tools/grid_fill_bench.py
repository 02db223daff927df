#!/usr/bin/env python3
"""Timings of detect / replace / smooth on a drift grid (include/sid_grid.h) on tools/grid_bench.py's
200 x 200 grid with 5 % of the nodes rejected at random and one 20 x 20 hole.

Median / p10 / p90 / min / max in microseconds of --reps calls after 20 warm-up calls (host clock around work that ends in a
device synchronise; device tensors in and out):
  fill_gaps        radius 1, min_neighbours 3, max_passes 16 (16 launches, however many passes fill something)
  smooth_r1 / _r2  the default Gaussian table, on the filled grid
  clean_drift      two detection passes, fill, smooth (sigma = 1)
  fill_gaps_numpy  the same fill with NumPy arrays in and out (copies included)
  passes_filling   passes that filled at least one node (gen.max())
  parity           the device results equal the host instance of the same source (device = -1) bit for bit
  host_route       for contrast, what a caller did before: per pass, scipy.ndimage.generic_filter with a NaN-aware median of
                   the 3 x 3 neighbours (at least 3 of them) over u and over v, until a pass fills nothing (--host-reps calls)
Kernel times alone: run under `rocprofv3 --kernel-trace --stats` with --trace (kernels k_grid_fill, k_grid_smooth).

    python tools/grid_fill_bench.py [--reps 200] [--out profiles/grid_fill_bench.json] [--trace]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))

from grid_bench import EPS, grid2d, same, stats_us                 # noqa: E402
from sea_ice_drift_amd import _capi, libfilter                     # noqa: E402


def workload():
    """u, v (200, 200) and the mask: 5 % rejected at random, and the hole."""
    _, _, u, v, valid = grid2d(0.05)
    valid[90:110, 90:110] = False
    return u, v, valid


def host_instance(u, v, valid):
    """fill, smooth and the chain from the host instances (device = -1), composed as libfilter.clean_drift composes them."""
    vv = np.ascontiguousarray(valid).view(np.uint8)
    fill = _capi.grid_fill(u, v, vv, None, 1, 3, 16, device=-1)
    w = libfilter.gaussian_weights(1.0, 1)
    smooth = _capi.grid_smooth(fill[0], fill[1], (fill[2] >= 0).view(np.uint8), w, 1, device=-1)
    s = valid & np.isfinite(u) & np.isfinite(v)
    for _ in range(2):
        res = _capi.grid_filter(u, v, s.view(np.uint8), EPS, 2.0, 1, 3, device=-1)[1]
        with np.errstate(invalid='ignore'):
            s = s & ~(res > 2.0)
    cf = _capi.grid_fill(u, v, s.view(np.uint8), None, 1, 3, 16, device=-1)
    cs = _capi.grid_smooth(cf[0], cf[1], (cf[2] >= 0).view(np.uint8), w, 1, device=-1)
    return fill, smooth, cs + (s, cf[2])


def host_route(u, v, valid):
    """Per pass one generic_filter per component; a node is filled when 3 of its 8 neighbours hold a value."""
    from scipy.ndimage import generic_filter
    footprint = np.ones((3, 3), dtype=bool)
    footprint[1, 1] = False

    def nanmedian3(w):
        w = w[~np.isnan(w)]
        return np.median(w) if len(w) >= 3 else np.nan
    uf, vf = np.where(valid, u, np.nan), np.where(valid, v, np.nan)
    passes = 0
    while True:
        mu = generic_filter(uf, nanmedian3, footprint=footprint, mode='constant', cval=np.nan)
        mv = generic_filter(vf, nanmedian3, footprint=footprint, mode='constant', cval=np.nan)
        new = np.isnan(uf) & ~np.isnan(mu)
        if not new.any():
            return uf, vf, passes
        uf[new], vf[new] = mu[new], mv[new]
        passes += 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=200)
    ap.add_argument('--host-reps', type=int, default=3)
    ap.add_argument('--out', default=None)
    ap.add_argument('--trace', action='store_true', help='device-tensor calls only (for a run under rocprofv3)')
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('no GPU: nothing is measured without one')
    sync = torch.cuda.synchronize
    u, v, valid = workload()
    du, dv, dvalid = [torch.tensor(q, device='cuda') for q in (u, v, valid)]
    uf, vf, gen = libfilter.fill_gaps(du, dv, valid=dvalid)
    filled = gen >= 0
    res = dict(device=torch.cuda.get_device_name(0), eps=EPS, rows=200, cols=200, usable=int(valid.sum()),
               gaps=int((~valid).sum()))
    calls = dict(fill_gaps=lambda: libfilter.fill_gaps(du, dv, valid=dvalid),
                 smooth_r1=lambda: libfilter.smooth(uf, vf, valid=filled),
                 smooth_r2=lambda: libfilter.smooth(uf, vf, radius=2, sigma=1.5, valid=filled),
                 clean_drift=lambda: libfilter.clean_drift(du, dv, EPS, valid=dvalid, sigma=1.0))
    for key, fn in calls.items():
        for _ in range(20):
            fn()
        sync()
        res[key + '_us'] = stats_us(fn, args.reps, sync)
    if not args.trace:
        gen_h = gen.cpu().numpy()
        res['passes_filling'] = int(gen_h.max())
        res['unfilled'] = int((gen_h < 0).sum())
        fill_h, smooth_h, clean_h = host_instance(u, v, valid)
        smooth_d = libfilter.smooth(uf, vf, valid=filled)
        clean_d = libfilter.clean_drift(du, dv, EPS, valid=dvalid, sigma=1.0)
        res['parity'] = dict(
            fill_gaps=all(same(g.cpu().numpy(), e) for g, e in zip((uf, vf, gen), fill_h)),
            smooth=all(same(g.cpu().numpy(), e) for g, e in zip(smooth_d, smooth_h)),
            clean_drift=all(same(g.cpu().numpy(), e) for g, e in zip(clean_d, clean_h)))
        res['clean_drift_rejected'] = int(valid.sum() - clean_d[2].sum().item())
        for _ in range(5):
            libfilter.fill_gaps(u, v, valid=valid)
        res['fill_gaps_numpy_us'] = stats_us(lambda: libfilter.fill_gaps(u, v, valid=valid), args.reps)
        try:
            hu, hv, passes = host_route(u, v, valid)
            res['host_route_passes'] = passes
            res['host_route_us'] = stats_us(lambda: host_route(u, v, valid), args.host_reps)
            # the same medians of the same neighbours: equal up to the zero's sign (np.median adds no 0.0)
            res['host_route_equal_values'] = bool(np.array_equal(hu, fill_h[0], equal_nan=True) and np.array_equal(hv, fill_h[1], equal_nan=True))
        except ImportError:
            res['host_route'] = 'scipy missing'
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(line + '\n')
    return 0 if all(res.get('parity', {}).values()) else 1


if __name__ == '__main__':
    sys.exit(main())
