#!/usr/bin/env python3
"""Generate tests/golden/g10_deformation.npz from the REFERENCE's own libdefor (libdefor.py).

Runs only in the build container: the reference is imported through the stubs of oracle/ref_harness.py.  The fixture holds
numbers only: the outputs the reference's functions returned, and for every input the sha256 of the arrays that the seeded
generators below rebuild (the GPU box has no reference; its tests import this module for the inputs alone).

Cases (names are the fixture's key prefixes):
  nodes_pm       get_deformation_nodes on a PM-like curvilinear grid in polar-stereographic metres (x, y ~1e5 .. 1e6 m,
                 u, v ~0.1 m/s) with 30 % of the nodes masked at random
  nodes_regular  get_deformation_nodes on an exactly regular grid (every quad co-circular: Qhull picks the diagonal)
  nodes_scatter  get_deformation_nodes on scattered points with exact duplicates (a duplicate is in no triangle)
  tri_i32, tri_i64  get_deformation_on_triangulation with a given t (int32 / int64): random triangles with negative
                 indices, collinear and repeated-vertex triangles, NaN and +-inf in u and v
  tri_empty_i32, tri_empty_i64  the same nodes, M = 0
  elems          get_deformation_elems with a given a that holds zeros (and -0.0)
Errors (err_names / err_types): where the reference raises - an index out of range (IndexError), fewer than 3 nodes
(matplotlib's ValueError), all nodes collinear (Qhull's RuntimeError).

    python tests/golden/make_golden_defor.py
"""
import hashlib
import importlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

PATH = os.path.join(HERE, 'g10_deformation.npz')
NODE_CASES = ('nodes_pm', 'nodes_regular', 'nodes_scatter')
TRI_CASES = ('tri_i32', 'tri_i64', 'tri_empty_i32', 'tri_empty_i64')
ERROR_CASES = ('index_out_of_range', 'fewer_than_3_nodes', 'all_collinear')


def sha256(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        a = np.ascontiguousarray(a)
        h.update(str(a.dtype).encode() + str(a.shape).encode())
        h.update(a.tobytes())
    return h.hexdigest()


def pm_grid(rows, cols, seed, masked=0.3):
    """Nodes of a pattern-matching grid in polar-stereographic metres: a ~10 km grid bent like a projected lon / lat grid
    (x ~ 2e5 .. 6e5, y ~ -1.2e6 .. -0.8e6), smooth drift of ~0.1 m/s plus noise, a fraction `masked` of the nodes left out."""
    rng = np.random.default_rng(seed)
    r, c = np.meshgrid(np.arange(rows, dtype=np.float64), np.arange(cols, dtype=np.float64), indexing='ij')
    th = np.deg2rad(-45.0 + 0.35 * c)
    rad = 1.0e6 + 1.0e4 * r
    x, y = rad * np.cos(th) + 3.0e5, rad * np.sin(th) - 2.5e5
    u = 0.1 * np.cos(0.05 * r + 0.03 * c) + 0.01 * rng.standard_normal(r.shape)
    v = 0.08 * np.sin(0.04 * r - 0.02 * c) + 0.01 * rng.standard_normal(r.shape)
    keep = rng.random(r.shape) >= masked
    return [a[keep].ravel().copy() for a in (x, y, u, v)]


def node_inputs(name):
    if name == 'nodes_pm':
        return pm_grid(40, 40, seed=1001)
    if name == 'nodes_regular':
        rng = np.random.default_rng(1002)
        r, c = np.meshgrid(np.arange(15, dtype=np.float64), np.arange(17, dtype=np.float64), indexing='ij')
        x, y = (4.0e5 + 1.0e4 * c).ravel(), (-9.0e5 + 1.0e4 * r).ravel()
        return [x, y, 0.1 * rng.standard_normal(x.size), 0.1 * rng.standard_normal(x.size)]
    if name == 'nodes_scatter':
        rng = np.random.default_rng(1003)
        x, y = rng.uniform(1.0e5, 9.0e5, 300), rng.uniform(-1.0e6, -2.0e5, 300)
        dup = rng.choice(300, 20, replace=False)
        x, y = np.concatenate([x, x[dup]]), np.concatenate([y, y[dup]])
        return [x, y, 0.1 * rng.standard_normal(x.size), 0.1 * rng.standard_normal(x.size)]
    raise KeyError(name)


def tri_nodes():
    """60 nodes: 48 scattered, 12 on the line y = 2 x + 5e4 (collinear triangles); NaN and +-inf in some u and v."""
    rng = np.random.default_rng(1004)
    x = np.concatenate([rng.uniform(0.0, 5.0e5, 48), 1.0e4 * np.arange(12.0)])
    y = np.concatenate([rng.uniform(0.0, 5.0e5, 48), 2.0 * 1.0e4 * np.arange(12.0) + 5.0e4])
    u, v = 0.1 * rng.standard_normal(60), 0.1 * rng.standard_normal(60)
    u[[3, 17]] = np.nan
    v[[5]] = np.inf
    u[[22]] = -np.inf
    v[[30]] = np.nan
    return x, y, u, v


def tri_triangles(dtype):
    """Random triangles over the 60 nodes with indices in [-60, 60), plus collinear and repeated-vertex triangles."""
    rng = np.random.default_rng(1005)
    t = [rng.integers(-60, 60, (400, 3))]
    t.append(np.array([[48, 49, 50], [48, 55, 59], [-1, -5, 52], [50, 49, 48]]))        # collinear (49 / 50 / 52 ... on the line)
    t.append(np.array([[7, 7, 9], [7, 9, 7], [9, 7, 7], [11, 11, 11], [3, 3, 5], [-60, 0, 1], [5, 30, 30]]))   # repeated vertices
    return np.ascontiguousarray(np.concatenate(t), dtype=dtype)


def tri_inputs(name):
    x, y, u, v = tri_nodes()
    dtype = np.int32 if name.endswith('i32') else np.int64
    t = tri_triangles(dtype) if 'empty' not in name else np.zeros((0, 3), dtype=dtype)
    return x, y, u, v, t


def elems_inputs():
    """(3, M) corners of 500 elements and an area (M,) with zeros and -0.0; NaN in a few corners."""
    rng = np.random.default_rng(1006)
    m = 500
    x, y = rng.uniform(1.0e5, 1.0e6, (3, m)), rng.uniform(-1.0e6, -1.0e5, (3, m))
    u, v = 0.1 * rng.standard_normal((3, m)), 0.1 * rng.standard_normal((3, m))
    a = rng.uniform(1.0e6, 1.0e8, m)
    a[::25] = 0.0
    a[7::50] = -0.0
    u[1, 3] = np.nan
    v[2, 4] = np.inf
    return x, y, u, v, a


def error_call(lib_module, name):
    """The call of error case `name` on a libdefor-like module (the reference's or this package's)."""
    if name == 'index_out_of_range':
        x, y, u, v = tri_nodes()
        t = np.array([[0, 1, 2], [3, 60, 4]], dtype=np.int32)
        return lib_module.get_deformation_on_triangulation(x, y, u, v, t)
    if name == 'fewer_than_3_nodes':
        x, y, u, v = [a[:2] for a in tri_nodes()]
        return lib_module.get_deformation_nodes(x, y, u, v)
    if name == 'all_collinear':
        x, y, u, v = [a[48:] for a in tri_nodes()]
        return lib_module.get_deformation_nodes(x, y, u, v)
    raise KeyError(name)


def hypot_pairs(n, seed):
    """n float64 pairs for hypot checks: random bit patterns (NaN, inf, subnormals), wide exponent ratios, near-equal and
    opposite magnitudes, subnormal and huge pairs, pairs across the scaling thresholds 2^-459 / 2^511, zeros and infinities."""
    rng = np.random.default_rng(seed)
    k = n // 8
    parts = []
    b = rng.integers(0, 2 ** 63, (2, k), dtype=np.int64).view(np.float64)
    parts.append(np.where(rng.random((2, k)) < 0.5, -b, b))
    m = rng.random((2, k)) + 0.5
    parts.append(np.ldexp(m, rng.integers(-70, 70, (2, k))))                                       # ratios up to 2^140
    x = rng.uniform(-1e6, 1e6, k)
    parts.append(np.stack([x, x * (1.0 + rng.uniform(-1e-8, 1e-8, k))]))
    parts.append(np.ldexp(m, rng.integers(-1075, -1010, (2, k))))                                # subnormal / tiny
    parts.append(np.ldexp(m, rng.integers(960, 1024, (2, k))))                                   # huge (overflow near the top)
    e = rng.integers(-470, -440, k)
    parts.append(np.stack([np.ldexp(m[0], e), np.ldexp(m[1], e - rng.integers(0, 8, k))]))         # around 2^-459
    e = rng.integers(500, 520, k)
    parts.append(np.stack([np.ldexp(m[0], e), np.ldexp(m[1], e - rng.integers(0, 60, k))]))        # around 2^511
    rest = n - 7 * k
    sp = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 5e-324, 1.7976931348623157e308, 1.0, -3.0])
    parts.append(np.stack([rng.choice(sp, rest), np.where(rng.random(rest) < 0.5, rng.choice(sp, rest), rng.standard_normal(rest))]))
    xy = np.concatenate(parts, axis=1)
    return np.ascontiguousarray(xy[0]), np.ascontiguousarray(xy[1])


def same_bits(got, exp):
    """Equal shapes, NaN in the same places, identical float64 bit patterns everywhere else (signed zeros included)."""
    got, exp = np.asarray(got, dtype=np.float64), np.asarray(exp, dtype=np.float64)
    if got.shape != exp.shape:
        return False
    gn, en = np.isnan(got), np.isnan(exp)
    return bool(np.array_equal(gn, en) and np.array_equal(got[~gn].view(np.int64), exp[~en].view(np.int64)))


def reference_libdefor():
    from oracle import ref_harness
    ref_harness.load()
    return importlib.import_module('sea_ice_drift.libdefor')


def compute(ref):
    """Every fixture array, from the reference module `ref`."""
    out = {}
    with np.errstate(all='ignore'):
        for name in NODE_CASES:
            x, y, u, v = node_inputs(name)
            out[name + '_in_sha'] = np.array(sha256(x, y, u, v))
            for key, val in zip(('e1', 'e2', 'e3', 'a', 'p', 't'), ref.get_deformation_nodes(x, y, u, v)):
                out['%s_%s' % (name, key)] = np.asarray(val)
        for name in TRI_CASES:
            x, y, u, v, t = tri_inputs(name)
            out[name + '_in_sha'] = np.array(sha256(x, y, u, v, t))
            for key, val in zip(('e1', 'e2', 'e3', 'a', 'p'), ref.get_deformation_on_triangulation(x, y, u, v, t)):
                out['%s_%s' % (name, key)] = np.asarray(val)
        x, y, u, v, a = elems_inputs()
        out['elems_in_sha'] = np.array(sha256(x, y, u, v, a))
        for key, val in zip(('e1', 'e2', 'e3'), ref.get_deformation_elems(x, y, u, v, a)):
            out['elems_' + key] = np.asarray(val)
        types = []
        for name in ERROR_CASES:
            try:
                error_call(ref, name)
                types.append('')
            except Exception as e:                 # noqa: the type is what is recorded
                types.append(type(e).__name__)
        out['err_names'] = np.array(ERROR_CASES)
        out['err_types'] = np.array(types)
    return out


def main():
    out = compute(reference_libdefor())
    np.savez_compressed(PATH, **out)
    print('wrote %s (%d bytes): %s' % (PATH, os.path.getsize(PATH), ', '.join(
        '%s M=%d' % (n, len(out[n + '_e1'])) for n in NODE_CASES + TRI_CASES)))


if __name__ == '__main__':
    main()
