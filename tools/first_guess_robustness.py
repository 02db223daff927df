#!/usr/bin/env python3
"""How far wrong key points move the first guess, per interpolant, on the host with NumPy and SciPy alone (DESIGN.md
section 20): 20 000 random key points on a 10000 x 10000 scene carrying synthetic.true_displacement + N(0, 1) px, a share of
them (default 1 %) displaced by up to +-150 px per component, evaluated on the bench's 200 x 200 grid.

Per interpolant of the DISPLACEMENT field: grid points further than 17 px from the truth (outside a min_border = 20 window
once the rounding of the first guess is allowed for), the largest and the median error.
  linear    scipy LinearNDInterpolator in the Delaunay triangulation (the reference's first guess)
  median5   component-wise median of the 5 nearest key points (method='knn')
  idw5      inverse-distance weights over the same 5 neighbours

    python tools/first_guess_robustness.py [--share 0.01] [--seed 0]
"""
import argparse
import json
import os
import sys

import numpy as np
from scipy.interpolate import LinearNDInterpolator
from scipy.spatial import cKDTree

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sea_ice_drift_amd import synthetic as syn                          # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--share', type=float, default=0.01)
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--k', type=int, default=5)
    args = ap.parse_args()
    rng = np.random.default_rng(args.seed)
    n, size = 20000, 10000
    c, r = rng.uniform(0, size, n), rng.uniform(0, size, n)
    d = np.stack(syn.true_displacement(c, r), axis=1) + rng.normal(0, 1, (n, 2))
    bad = rng.choice(n, int(round(args.share * n)), replace=False)
    d[bad] += rng.uniform(-150, 150, (len(bad), 2))
    cg, rg = np.meshgrid(np.rint(np.linspace(100, size - 101, 200)), np.rint(np.linspace(100, size - 101, 200)))
    pts, grid = np.stack([r, c], axis=1), np.stack([rg.ravel(), cg.ravel()], axis=1)
    truth = np.stack(syn.true_displacement(cg.ravel(), rg.ravel()), axis=1)
    dist, idx = cKDTree(pts).query(grid, k=args.k)
    w = 1.0 / np.maximum(dist, 1e-9)
    est = {'linear': LinearNDInterpolator(pts, d)(grid),
           'median%d' % args.k: np.median(d[idx], axis=1),
           'idw%d' % args.k: (d[idx] * w[..., None]).sum(axis=1) / w.sum(axis=1)[:, None]}
    out = dict(key_points=n, wrong=len(bad), grid_points=len(grid))
    for name, e in est.items():
        err = np.hypot(*(e - truth).T)
        ok = np.isfinite(err)
        out[name] = dict(beyond_17px=int((err[ok] > 17).sum()), outside_hull=int((~ok).sum()), max_px=round(float(err[ok].max()), 2),
                         median_px=round(float(np.median(err[ok])), 2))
    print(json.dumps(out))


if __name__ == '__main__':
    main()
