#!/usr/bin/env python3
"""Generate tests/golden/g13_grid.npz: include/sid_grid.h's cases.

Runs only in the build container: the reference's libdefor is imported through the stubs of oracle/ref_harness.py.  The fixture
holds numbers only.  Per deformation case NAME: NAME_out (5, M) - what the REFERENCE's get_deformation_on_triangulation returned
for the present triangles of the specification (tests/grid_spec.py), in slot order - and NAME_t, the specification's triangles.
Per filter case NAME: NAME_keep and NAME_res of the specification (the reference has no filter).  `names` / `shas`: every
case and the sha256 of the arrays the seeded generators below rebuild (the GPU box has no reference; its tests import this
module for the inputs alone).

    python tests/golden/make_golden_grid.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import grid_spec as gs                                  # noqa: E402
from tests.golden.make_golden_defor import reference_libdefor, sha256      # noqa: E402

PATH = os.path.join(HERE, 'g13_grid.npz')


def pm_geometry(rows, cols):
    """make_golden_defor.pm_grid's curvilinear geometry on the full (rows, cols) grid: a ~10 km grid bent like a projected
    lon / lat grid, polar-stereographic metres."""
    r, c = np.meshgrid(np.arange(rows, dtype=np.float64), np.arange(cols, dtype=np.float64), indexing='ij')
    th = np.deg2rad(-45.0 + 0.35 * c)
    rad = 1.0e6 + 1.0e4 * r
    return r, c, rad * np.cos(th) + 3.0e5, rad * np.sin(th) - 2.5e5


def pm_case(rows, cols, seed, masked=0.3, holes=4):
    rng = np.random.default_rng(seed)
    r, c, x, y = pm_geometry(rows, cols)
    u = 0.1 * np.cos(0.05 * r + 0.03 * c) + 0.01 * rng.standard_normal(r.shape)
    v = 0.08 * np.sin(0.04 * r - 0.02 * c) + 0.01 * rng.standard_normal(r.shape)
    valid = rng.random(r.shape) >= masked
    for k, n in enumerate(rng.choice(rows * cols, holes, replace=False)):            # NaN in u or v at a few more
        (u if k % 2 else v).ravel()[n] = np.nan
    return x, y, u, v, valid


def sheared(rows, cols, shear, ydown, seed):
    """An affinely sheared 10 km grid: x = 1e4 (c + shear r), y = +-1e4 r.  Every cell is the same parallelogram."""
    rng = np.random.default_rng(seed)
    r, c = np.meshgrid(np.arange(rows, dtype=np.float64), np.arange(cols, dtype=np.float64), indexing='ij')
    x, y = 1.0e4 * (c + shear * r) + 2.0e5, (-1.0e4 if ydown else 1.0e4) * r - 5.0e5
    return x, y, 0.1 * rng.standard_normal(r.shape), 0.1 * rng.standard_normal(r.shape), None


SHEARED = {'shear_p': (0.3, False), 'shear_m': (-0.3, False), 'shear_p_ydown': (0.3, True), 'shear_m_ydown': (-0.3, True)}
DEFOR_CASES = (('pm_curvi', 'pm_main', 'pm_anti', 'regular') + tuple(SHEARED) + tuple('p2x2_%02d' % k for k in range(16)) +
               ('coincident', 'shape_2x2', 'shape_2x7', 'shape_7x2'))


def defor_inputs(name):
    """-> x, y, u, v, valid (bool or None), diagonal"""
    if name in ('pm_curvi', 'pm_main', 'pm_anti'):
        return pm_case(9, 11, seed=1301) + ({'pm_curvi': 'shorter', 'pm_main': 'main', 'pm_anti': 'anti'}[name],)
    if name == 'regular':                                             # every da == dm: the main split
        rng = np.random.default_rng(1302)
        r, c = np.meshgrid(np.arange(6, dtype=np.float64), np.arange(7, dtype=np.float64), indexing='ij')
        return 4.0e5 + 1.0e4 * c, -9.0e5 + 1.0e4 * r, 0.1 * rng.standard_normal(r.shape), 0.1 * rng.standard_normal(r.shape), None, 'shorter'
    if name in SHEARED:
        return sheared(7, 9, *SHEARED[name], seed=1303) + ('shorter',)
    if name.startswith('p2x2_'):                                      # all 16 usable patterns of one cell
        k = int(name[-2:])
        x, y, u, v, _ = sheared(2, 2, 0.3, False, seed=1304)
        valid = np.array([[k & 1, k & 2], [k & 8, k & 4]], dtype=bool)                # bits in ring order A, B, E, D
        return x, y, u, v, valid, 'shorter'
    if name == 'coincident':                                          # node (1, 1) lies on node (1, 2): cr = 0, area 0
        x, y, u, v, _ = sheared(3, 4, 0.0, False, seed=1305)
        x[1, 1], y[1, 1] = x[1, 2], y[1, 2]
        return x, y, u, v, None, 'shorter'
    if name.startswith('shape_'):
        rows, cols = [int(q) for q in name[6:].split('x')]
        return pm_case(rows, cols, seed=1306 + rows, masked=0.0, holes=0)[:4] + (None, 'shorter')
    raise KeyError(name)


# name: (field, eps, threshold, radius, min_neighbours)
FILTER_CASES = dict(
    [('quant_r%d_m%d' % (r, m), ('quant', 0.1, 2.0, r, m)) for r in (1, 2) for m in (1, 3, 8)] +
    [('smooth_r1', ('smooth', 0.002, 2.0, 1, 3)), ('smooth_r2', ('smooth', 0.002, 1.5, 2, 3)),
     ('row_1x9', ('row', 0.05, 2.0, 1, 1)), ('col_9x1', ('col', 0.05, 2.0, 2, 2)),
     ('all_invalid', ('none', 0.1, 2.0, 1, 1)), ('isolated', ('isolated', 0.1, 2.0, 2, 1)),
     ('huge_r1', ('huge', 0.1, 2.0, 1, 3)), ('huge_r2', ('huge', 0.1, 2.0, 2, 3))])


def filter_field(kind):
    """-> u, v, valid (bool or None)"""
    if kind == 'quant':                        # a few levels, signed zeros among them: medians and MADs tie, mu = 0
        rng = np.random.default_rng(1311)
        lv = np.array([-0.5, -0.0, 0.0, 0.5])
        return lv[rng.integers(0, 4, (9, 11))], lv[rng.integers(0, 4, (9, 11))], rng.random((9, 11)) >= 0.2
    if kind == 'smooth':                       # a smooth field with noise, outliers, NaN and inf; no mask
        rng = np.random.default_rng(1312)
        r, c = np.meshgrid(np.arange(10.0), np.arange(13.0), indexing='ij')
        u = 0.05 + 0.002 * r - 0.001 * c + 0.0005 * rng.standard_normal(r.shape)
        v = -0.02 + 0.001 * r + 0.003 * c + 0.0005 * rng.standard_normal(r.shape)
        u[2::4, 1::5] += 0.05
        v[1::3, 3::4] -= 0.04
        u[0, 0], v[9, 12], u[4, 4], v[5, 7] = np.nan, np.nan, np.inf, -np.inf
        return u, v, None
    if kind in ('row', 'col'):
        rng = np.random.default_rng(1313)
        u, v = rng.standard_normal(9), rng.standard_normal(9)
        valid = np.ones(9, dtype=bool)
        valid[6] = False
        shape = (1, 9) if kind == 'row' else (9, 1)
        return u.reshape(shape), v.reshape(shape), valid.reshape(shape)
    if kind == 'none':
        return np.ones((4, 5)), np.ones((4, 5)), np.zeros((4, 5), dtype=bool)
    if kind == 'isolated':                     # one usable node, nobody around it; and a pair in a corner
        valid = np.zeros((7, 7), dtype=bool)
        valid[3, 3] = valid[0, 0] = valid[0, 1] = True
        rng = np.random.default_rng(1314)
        return rng.standard_normal((7, 7)), rng.standard_normal((7, 7)), valid
    if kind == 'huge':                         # neighbours of +-1e308: their differences and even medians overflow
        rng = np.random.default_rng(1315)
        u = np.where(rng.random((5, 6)) < 0.5, 1e308, -1e308)
        v = np.where(rng.random((5, 6)) < 0.5, 1e308, -1e308)
        u[2, 2], v[2, 2], u[1, 4], v[3, 1] = 0.0, 1.0, 3.0, -2.0
        return u, v, None
    raise KeyError(kind)


def filter_inputs(name):
    """-> u, v, valid, eps, threshold, radius, min_neighbours"""
    kind, eps, threshold, radius, minn = FILTER_CASES[name]
    return filter_field(kind) + (eps, threshold, radius, minn)


def input_sha(arrays):
    return sha256(*[np.asarray(a) for a in arrays if a is not None and not isinstance(a, str)])


def chain_inputs():
    """The end-to-end check of section 19: a linear velocity field on the PM geometry at 12 x 15 (divergence 2.5e-7,
    shear 2.5e-7 ... see tests), 15 % of the nodes unusable, outliers planted at [2::4, 1::4] where usable.
    -> x, y, u, v, usable, planted (bool), eps"""
    _, _, x, y = pm_geometry(12, 15)
    u = 0.05 + 2e-7 * (x - 5e5) - 1e-7 * (y + 1e6)
    v = -0.02 + 3e-7 * (x - 5e5) + 0.5e-7 * (y + 1e6)
    usable = np.random.default_rng(1).random((12, 15)) > 0.15
    planted = np.zeros((12, 15), dtype=bool)
    planted[2::4, 1::4] = True
    planted &= usable
    u, v = u.copy(), v.copy()
    u[planted] += 0.05
    v[planted] -= 0.04
    return x, y, u, v, usable, planted, 0.002


def compute(ref):
    """Every fixture array; the deformation outputs from the reference module `ref`."""
    out, names, shas = {}, [], []
    with np.errstate(all='ignore'):
        for name in DEFOR_CASES:
            x, y, u, v, valid, diagonal = defor_inputs(name)
            names.append(name)
            shas.append(input_sha((x, y, u, v, valid)))
            t = gs.grid_triangles(x, y, gs.usable_xyuv(x, y, u, v, valid), diagonal)
            _, tri = gs.present(t)
            vals = ref.get_deformation_on_triangulation(x.ravel(), y.ravel(), u.ravel(), v.ravel(), tri) if len(tri) else [np.empty(0)] * 5
            out[name + '_out'] = np.asarray(vals, dtype=np.float64).reshape(5, -1)
            out[name + '_t'] = t
        for name in FILTER_CASES:
            args = filter_inputs(name)
            names.append(name)
            shas.append(input_sha(args[:3]))
            keep, res = gs.nmt(*args)
            out[name + '_keep'] = keep
            out[name + '_res'] = res
    out['names'] = np.array(names)
    out['shas'] = np.array(shas)
    return out


def main():
    out = compute(reference_libdefor())
    np.savez_compressed(PATH, **out)
    print('wrote %s (%d bytes, %d cases)' % (PATH, os.path.getsize(PATH), len(out['names'])))


if __name__ == '__main__':
    main()
