"""Constructed inputs of the first-guess evaluation (include/sid_fg.h), each with its claim; shared by
tests/test_fg_spec_host.py (the specification against SciPy, CPU) and tests/test_gpu_fg_small.py (the device against the
specification).  The specification's answer for a case is computed once per process (``expected`` / ``expected_dist``) and
never modified.  No tests in here.

An interpolation case is a dict: pts [n,2], simplices [m,3] int32, values [n,2], q [k,2];
    known     {query index: simplex index} - queries at the centroid of a simplex, located without SciPy
    half      the queries a case places at a value that is exactly a half-integer (they stay flagged)
    route     what sid_fg_debug_route must report on the default route (a subset of its fields), where the case claims one in
              numbers; tests/fg_spec.py bucket_entries counts the bucket entries of every case
    scipy     'same': the simplex list is SciPy's own Delaunay triangulation of pts, index for index; 'hull': another list with
              the same interpolant (SciPy's hull membership and rounded values still hold); False: neither
A nearest-distance case is (seeds, q, buckets): buckets = whether the default route walks the buckets."""
import functools

import numpy as np
from scipy.spatial import Delaunay

from tests import fg_spec as spec

INF, NAN = np.inf, np.nan
NON_FINITE = np.array([[NAN, 3.0], [3.0, NAN], [NAN, NAN], [INF, 3.0], [-INF, 3.0], [3.0, INF], [3.0, -INF], [INF, -INF], [INF, NAN]])


def _values(rng, pts, simplices):
    """Two value columns, drawn again until no centroid's value comes within 1e-3 of a half-integer."""
    while True:
        a, b = rng.uniform(0.9, 1.1, 2), rng.uniform(-5, 5, 2)
        v = np.stack([pts[:, 1] * a[0] + b[0] + rng.normal(0, 2, len(pts)), pts[:, 0] * a[1] + b[1] + rng.normal(0, 2, len(pts))], axis=1)
        o = v[simplices].mean(axis=1)
        if (np.abs(o - np.floor(o) - 0.5) > 1e-3).all():
            return v


def _triangulated(rng, pts, n_vertices=60, n_mid=40, n_out=100):
    """SciPy's triangulation of pts; queries: the centroid of every simplex, vertices, edge midpoints, points outside the hull
    and the non-finite ones."""
    tri = Delaunay(pts)
    pts, simp = tri.points.copy(), tri.simplices.astype(np.int32)
    cen = pts[simp].mean(axis=1)
    lo, hi = pts.min(axis=0), pts.max(axis=0)
    ext = hi - lo
    out = lo - ext + rng.uniform(0, 1, (n_out, 2)) * 3 * ext
    inside = ((out > lo) & (out < hi)).all(axis=1)
    out[inside, 0] = hi[0] + ext[0] * rng.uniform(0.001, 1, inside.sum())
    e = simp[rng.integers(0, len(simp), n_mid)]
    q = np.concatenate([cen, pts[rng.permutation(len(pts))[:n_vertices]], (pts[e[:, 0]] + pts[e[:, 1]]) / 2, out, NON_FINITE + lo])
    return dict(pts=pts, simplices=simp, values=_values(rng, pts, simp), q=q, known={k: k for k in range(len(simp))},
                half=[], route=None, scipy='same')


def _triangle(order):
    """One triangle with axis-parallel legs; the six vertex orders put the zeros of the 2 x 2 system in different places and take
    the pivot swap or not.  The value at vertex 1 is exactly 7.5."""
    pts = np.array([[1.0, 2.0], [5.0, 2.0], [1.0, 5.0]])
    values = np.array([[3.2, -1.3], [7.5, 2.25], [-4.1, 9.8]])
    A, B, C = pts
    mids = [(A + B) / 2, (B + C) / 2, (A + C) / 2]
    normals = [np.array([0.0, -1.0]), np.array([0.6, 0.8]), np.array([-1.0, 0.0])]      # outward, unit length
    q = [A, B, C] + mids + [(A + B + C) / 3]
    for d in (1e-12, 1e-8):
        q += [m + d * n for m, n in zip(mids, normals)]
    q += [np.array([-40.0, 2.5]), np.array([2.0, 1e9]), np.array([1e300, 1e300])]
    q = np.concatenate([np.array(q), NON_FINITE])
    return dict(pts=pts, simplices=np.array([order], dtype=np.int32), values=values, q=q, known={6: 0}, half=[1],
                route=dict(buckets=1, entries=16384, capacity=8 + 16384), scipy='hull')


@functools.lru_cache(maxsize=None)
def interp_cases():
    rng = np.random.default_rng(20261021)
    c = {}
    for order in ((0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0)):
        c['triangle_%d%d%d' % order] = _triangle(order)
    # a square of two triangles, queries along the shared diagonal: each covers every cell of the grid, so the lists do not fit
    sq = np.array([[0.0, 0.0], [10.0, 0.0], [10.0, 10.0], [0.0, 10.0]])
    t = np.concatenate([np.linspace(0.0, 1.0, 41), [1.0 / 3.0, 0.1 + 1e-13]])
    c['square_diagonal'] = dict(pts=sq, simplices=np.array([[0, 1, 2], [0, 2, 3]], dtype=np.int32),
                                values=np.array([[1.3, 2.2], [11.4, 2.9], [12.1, 13.3], [0.7, 12.6]]),
                                q=np.concatenate([np.outer(t, [10.0, 10.0]), [[20.0 / 3, 10.0 / 3], [10.0 / 3, 20.0 / 3]]]),
                                known={43: 0, 44: 1}, half=[], route=dict(buckets=0, entries=32768, capacity=16 + 16384, ychunks=1, chunk=256),
                                scipy=False)
    gy, gx = np.meshgrid(np.arange(12.0), np.arange(13.0), indexing='ij')
    c['lattice_jitter_12x13'] = _triangulated(rng, np.stack([gy.ravel(), gx.ravel()], axis=1) * 7.0 + rng.uniform(-1.5, 1.5, (156, 2)))
    gy, gx = np.meshgrid(np.arange(17.0), np.arange(17.0), indexing='ij')
    c['lattice_int_17x17'] = _triangulated(rng, np.stack([gy.ravel(), gx.ravel()], axis=1))
    sc = _triangulated(rng, rng.uniform(0, 1000, (300, 2)))
    c['scattered_300'] = sc
    for n in (1, 255, 256, 257):                                          # one block of queries, full, and one query more
        d = dict(sc, q=sc['q'][:n], known={k: v for k, v in sc['known'].items() if k < n})
        c['scattered_300_nq%d' % n] = d
    for n in (255, 256, 257, 513):                                        # simplex counts around the 256-entry tile of the brute-force pass
        c['scattered_300_ns%d' % n] = dict(sc, simplices=sc['simplices'][:n], known={k: v for k, v in sc['known'].items() if k < n}, scipy=False)
    # two key points far away that no simplex uses: the box is wide, the triangulation sits in a few cells and the bucket lists
    # fit - the bucket route with many simplices per cell (a few hundred simplices over the whole box never fit: 8 n + 128^2)
    # Twenty key points carry a value that is exactly a half-integer and are queries themselves: such a query lies in several
    # simplices and STAYS flagged, so what it reports is the location's own choice among them, not the second look's.
    for name, span in (('lattice_int_17x17', 1000.0), ('scattered_300', 20000.0)):
        d = c[name]
        hv = np.arange(20) * (len(d['pts']) // 20) + 7
        vals = d['values'].copy()
        vals[hv, 0] = np.floor(vals[hv, 0]) + 0.5
        c[name + '_wide_box'] = dict(d, pts=np.concatenate([d['pts'], [[-span, -span], [span, span]]]),
                                     values=np.concatenate([vals, [[0.25, 0.25], [0.25, 0.25]]]),
                                     q=np.concatenate([d['q'], d['pts'][hv]]), scipy=False)
    # forty points in the unit square and three a million away: slivers across the whole box, the bucket lists do not fit
    far = _triangulated(rng, np.concatenate([rng.uniform(0, 1, (40, 2)), [[1e6, 0.5], [-1e6, 0.4], [0.5, 1e6]]]), 20, 20, 40)
    far['route'] = dict(buckets=0, ychunks=1, chunk=256)
    c['sliver_fan'] = far
    # flat simplices in a hand-made list: a horizontal one at index 0, a vertical one in the middle; they are skipped
    lat = c['lattice_int_17x17']
    s, mid = lat['simplices'], len(lat['simplices']) // 2
    flat = np.concatenate([[[0, 1, 2]], s[:mid], [[0, 17, 34]], s[mid:]]).astype(np.int32)
    assert (lat['pts'][[0, 1, 2], 0] == 0).all() and (lat['pts'][[0, 17, 34], 1] == 0).all()
    c['flat_simplices_inserted'] = dict(lat, simplices=flat, known={k: k + 1 + (k >= mid) for k in lat['known']}, scipy='hull')
    c['flat_simplices_only'] = dict(lat, simplices=np.array([[0, 1, 2], [0, 17, 34], [5, 5, 9], [288, 271, 254]], dtype=np.int32), known={}, scipy=False)
    # key points and queries offset by 2^20 in both coordinates
    off = float(1 << 20)
    c['scattered_300_offset_2p20'] = _triangulated(rng, rng.uniform(0, 1000, (300, 2)) + off)
    for d in c.values():
        for k in ('pts', 'simplices', 'values', 'q'):
            d[k] = np.ascontiguousarray(d[k])
            d[k].setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def expected(name):
    """The specification's (out, simplex, doubt, details) for an interpolation case, computed once."""
    c = interp_cases()[name]
    res = spec.interp_linear(c['pts'], c['simplices'], c['values'], c['q'], details=True)
    for a in res[:3]:
        a.setflags(write=False)
    return res


@functools.lru_cache(maxsize=None)
def dist_cases():
    """name -> (seeds, q, buckets)."""
    rng = np.random.default_rng(20261022)
    c = {}
    around = lambda lo, hi, n: np.concatenate([rng.uniform(lo - 0.2 * (hi - lo), hi + 0.2 * (hi - lo), (n, 2)), NON_FINITE + lo])
    for n in (255, 256, 257):                                             # the switch to the buckets at 256 seeds
        c['seeds_%d' % n] = (rng.uniform(0, 100, (n, 2)), around(0.0, 100.0, 300), n >= 256)
    # 255 seeds within one cell at a corner, one at the opposite corner: queries next to the lone seed walk all 127 rings
    corner = np.concatenate([rng.uniform(0, 0.5, (255, 2)), [[128.0, 128.0]]])
    c['lone_seed_opposite'] = (corner, np.concatenate([rng.uniform(120, 128, (200, 2)), rng.uniform(0, 128, (100, 2)), [[128.0, 128.0], [127.5, 0.2]]]), True)
    # integer seeds on [0, 128]^2: every seed on a cell border; queries at integers and half-integers
    lat = np.unique(np.concatenate([np.floor(rng.uniform(0, 129, (400, 2))), [[0.0, 0.0], [128.0, 128.0]]]), axis=0)
    hx, hy = np.meshgrid(np.arange(-2.0, 131.0, 4.5), np.arange(-2.0, 131.0, 3.5))
    c['integer_seeds_on_borders'] = (lat, np.concatenate([np.stack([hy.ravel(), hx.ravel()], axis=1), lat[:100]]), True)
    # a box whose width is no dyadic number
    box = np.concatenate([rng.uniform(0.1, 0.7, (298, 2)), [[0.1, 0.1], [0.7, 0.7]]])
    c['box_0p1_0p7'] = (box, np.concatenate([around(0.1, 0.7, 300), 0.1 + 0.6 * np.arange(0, 129)[:, None] / 128.0 * np.ones((1, 2))]), True)
    # queries outside the box on all eight sides, 1 ulp and 1e6 away; a query on a seed; two equidistant seeds
    s = rng.uniform(10, 20, (330, 2))
    s = np.concatenate([s[np.hypot(s[:, 0] - 15.0, s[:, 1] - 15.0) > 1.5], [[10.0, 10.0], [20.0, 20.0], [14.0, 15.0], [16.0, 15.0]]])
    assert len(s) >= 256
    out = []
    for sx in (-1, 0, 1):
        for sy in (-1, 0, 1):
            if sx or sy:
                for far in (False, True):
                    p = [15.0, 15.0]
                    for ax, sg in ((0, sx), (1, sy)):
                        if sg:
                            edge = 10.0 if sg < 0 else 20.0
                            p[ax] = edge + sg * 1e6 if far else np.nextafter(edge, sg * INF)
                    out.append(p)
    c['outside_on_eight_sides'] = (s, np.concatenate([np.array(out), s[:40], [[15.0, 15.0], [15.0, 12.0]]]), True)
    # no area: seeds on a vertical and on a horizontal line take the brute-force route
    line = np.arange(300.0)
    c['vertical_line'] = (np.stack([line, np.full(300, 7.0)], axis=1), around(0.0, 300.0, 200), False)
    c['horizontal_line'] = (np.stack([np.full(300, -3.0), line], axis=1), around(0.0, 300.0, 200), False)
    c['one_seed_300_times'] = (np.tile([[4.0, 9.0]], (300, 1)), around(0.0, 10.0, 100), False)
    # The ring walk stops when nothing outside the block can be closer than the best seed inside - with a margin for the rounding
    # of the cell index.  Box [0, 128]^2, cells one wide.  Per direction: the query a quarter from a side of its cell, a seed
    # 1e-8 BEHIND that side (the next ring), a seed inside the cell 2e-8 further away than that one.  The walk must go on.
    d = 1e-8
    bg = np.concatenate([rng.uniform(0, 20, (300, 2)), [[0.0, 0.0], [128.0, 128.0]]])
    plant, qs = [], []
    for (cx, cy), (ax, sg) in zip(((40.0, 40.0), (40.0, 80.0), (80.0, 40.0), (80.0, 80.0)), ((0, 1), (0, -1), (1, 1), (1, -1))):
        q0, behind, inside = [cx + 0.5, cy + 0.5], [cx + 0.5, cy + 0.5], [cx + 0.5, cy + 0.5]
        base = (cx, cy)[ax]
        q0[ax] = base + (0.75 if sg > 0 else 0.25)
        behind[ax] = base + 1.0 + d if sg > 0 else base - d
        inside[ax] = q0[ax] - sg * (0.25 + 2 * d)
        plant += [behind, inside]
        qs.append(q0)
    c['seed_just_behind_a_side'] = (np.concatenate([bg, plant]), np.array(qs), True)
    for v in c.values():
        for a in v[:2]:
            a.setflags(write=False)
    return c


# sid_fg_distance_image: rows != columns, so a swapped axis shows; 300 seeds = (row, column) inside and around the image
IMAGE_SHAPES = ((1, 1), (1, 300), (300, 1), (5, 400))


@functools.lru_cache(maxsize=None)
def image_seeds():
    rng = np.random.default_rng(20261023)
    s = np.floor(np.stack([rng.uniform(-3, 12, 300), rng.uniform(-10, 420, 300)], axis=1))
    s.setflags(write=False)
    return s


@functools.lru_cache(maxsize=None)
def expected_dist(name):
    seeds, q, _ = dist_cases()[name]
    d = spec.nearest_dist(seeds, q)
    d.setflags(write=False)
    return d
