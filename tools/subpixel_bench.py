#!/usr/bin/env python3
"""What the sub-pixel peak (include/sid_pm.h SID_PM_SUBPIXEL, ``subpixel=True``) costs: the headline workload of bench.py
(10000 x 10000 pair, 200 x 200 grid, mixed borders, template 34 px, angles -7..7) and the reference-defaults workload (template
35 px, angles [-3, 0, 3]) through one ``PMContext`` with the flag off and on.

A round = set_points with the flag off, ``--steps`` runs between two HIP events, the same with the flag on; ``--rounds`` rounds,
off and on alternating so that a drift of the clocks hits both.  Per workload and flag: the median, the smallest and the largest
kernel time of a run over the rounds, and on / off of the medians.  The results of the last round are compared: angle, r, h
and the peak indices must not change, c2 / r2 move by at most half a pixel.

    python tools/subpixel_bench.py [--size 10000] [--grid 200] [--steps 10] [--rounds 7] [--out profiles/subpixel_bench.json]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from sea_ice_drift_amd import _capi, synthetic as syn      # noqa: E402
from sea_ice_drift_amd.pmlib import rotation_table         # noqa: E402

WORKLOADS = (('headline', 34, list(range(-7, 8))), ('reference_defaults', 35, [-3, 0, 3]))


def run_ms(torch, ctx, steps):
    ctx.run()                                              # untimed: the first run after set_points
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        ctx.run()
    b.record()
    b.synchronize()
    ctx.check()
    return a.elapsed_time(b) / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--size', type=int, default=10000)
    ap.add_argument('--grid', type=int, default=200)
    ap.add_argument('--border', default='mixed')
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    import torch
    dev = torch.device('cuda', 0)
    img1, img2 = syn.make_pair(args.size, args.size)
    t1, t2 = torch.from_numpy(img1).to(dev), torch.from_numpy(img2).to(dev)
    border = args.border if args.border == 'mixed' else int(args.border)
    g = syn.make_grid(args.size, args.size, args.grid, border=border)
    vec = [g[k] for k in ('c1', 'r1', 'c2fg', 'r2fg', 'border')]
    res = dict(device=torch.cuda.get_device_name(0), size=args.size, grid=args.grid, border=str(args.border), steps=args.steps,
               rounds=args.rounds, points=int(g['c1'].size), unit='ms of kernel time per run (HIP events around `steps` runs)')
    with _capi.PMContext(0) as ctx:
        ctx.set_stream(torch.cuda.current_stream().cuda_stream)
        ctx.bind_pair_tensors(t1, t2)
        for name, s, angles in WORKLOADS:
            rot = rotation_table(angles, 0.0, s)
            ms = {0: [], _capi.SUBPIXEL: []}
            out = {}
            for _ in range(args.rounds):
                for bit in (0, _capi.SUBPIXEL):
                    ctx.set_points(*vec, s, 0.0, angles, rot=rot, flags=_capi.HES_NORM | bit)
                    ms[bit].append(run_ms(torch, ctx, args.steps))
                    out[bit] = ctx.fetch()
            (off, off_ij), (on, on_ij) = out[0], out[_capi.SUBPIXEL]
            ok = np.isfinite(off[:, 0])
            same = bool(np.array_equal(off_ij, on_ij) and np.array_equal(off[:, 2:], on[:, 2:], equal_nan=True)
                        and np.array_equal(np.isnan(off), np.isnan(on)))
            d = np.abs(on[ok, :2] - off[ok, :2])
            w = dict(template=s, angles=len(angles), launches=ctx.work_info()['launches'], valid_points=int(ok.sum()))
            for key, bit in (('off', 0), ('on', _capi.SUBPIXEL)):
                v = np.array(ms[bit])
                w[key] = dict(median_ms=round(float(np.median(v)), 4), min_ms=round(float(v.min()), 4), max_ms=round(float(v.max()), 4),
                              all_ms=[round(float(x), 4) for x in v])
            w['on_over_off'] = round(w['on']['median_ms'] / w['off']['median_ms'], 5)
            w['angle_r_h_ij_unchanged'] = same
            w['max_abs_offset_px'] = round(float(d.max()), 6)
            w['points_with_a_nonzero_offset'] = int((d > 0).any(axis=1).sum())
            res[name] = w
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(line + '\n')
    bad = [n for n, _, _ in WORKLOADS if not res[n]['angle_r_h_ij_unchanged'] or res[n]['max_abs_offset_px'] > 0.5]
    return 1 if bad else 0


if __name__ == '__main__':
    sys.exit(main())
