"""The cases that tests/test_track_host.py (host instance) and tests/test_gpu_track.py (device) run against tests/track_spec.py.
No tests in here.  Node grids are those of tests/warp_cases.py where a case of that file is named, at most 40 x 40 nodes and
20 000 points otherwise - the smallest at which each path can go wrong: see the reason beside each case.  What a case is made
for is asserted from the specification in test_track_host.py::test_cases_cover_what_they_claim."""
import numpy as np

from sea_ice_drift_amd import _capi
from tests import warp_cases as wc

DIAGONALS = ('shorter', 'main', 'anti')
BRUTE = _capi.TRACK_BRUTE_CELLS

# points no mesh has, and points that are no points; every case gets them, twice (duplicated points)
SPECIAL = np.array([[1e7, 3.0], [-1e7, -1e7], [3.0, 1e300], [np.nan, 5.0], [5.0, np.nan], [np.inf, 5.0], [5.0, -np.inf],
                    [-np.inf, np.inf], [np.nan, np.nan]])


def case(name, x, y, xs, ys, px, py, valid=None, diagonal='shorter'):
    px = np.concatenate([np.ravel(px), SPECIAL[:, 0], SPECIAL[:, 0]])
    py = np.concatenate([np.ravel(py), SPECIAL[:, 1], SPECIAL[:, 1]])
    return dict(name=name, x=np.ascontiguousarray(x), y=np.ascontiguousarray(y), xs=np.ascontiguousarray(xs),
                ys=np.ascontiguousarray(ys), valid=valid, diagonal=diagonal, px=px, py=py)


def around(x, y, n, seed, margin=15.0):
    """n seeded fractional points in the bounding box of the finite nodes and `margin` pixels around it; the first tenth twice."""
    rng = np.random.default_rng(seed)
    fx, fy = x[np.isfinite(x)], y[np.isfinite(y)]
    px = rng.uniform(fx.min() - margin, fx.max() + margin, n)
    py = rng.uniform(fy.min() - margin, fy.max() + margin, n)
    return np.concatenate([px, px[:n // 10]]), np.concatenate([py, py[:n // 10]])


def nodes_midpoints_rim(x, y):
    """Every node, the midpoint of every grid edge and of both diagonals of every cell, and points along the four rims."""
    px = [x.ravel(), (x[:, :-1] + x[:, 1:]).ravel() / 2, (x[:-1] + x[1:]).ravel() / 2, (x[:-1, :-1] + x[1:, 1:]).ravel() / 2,
          (x[:-1, 1:] + x[1:, :-1]).ravel() / 2]
    py = [y.ravel(), (y[:, :-1] + y[:, 1:]).ravel() / 2, (y[:-1] + y[1:]).ravel() / 2, (y[:-1, :-1] + y[1:, 1:]).ravel() / 2,
          (y[:-1, 1:] + y[1:, :-1]).ravel() / 2]
    t = np.linspace(0.0, 1.0, 41)
    x0, x1, y0, y1 = x.min(), x.max(), y.min(), y.max()
    for ax, ay in ((x0 + t * (x1 - x0), y0 + 0 * t), (x0 + t * (x1 - x0), y1 + 0 * t), (x0 + 0 * t, y0 + t * (y1 - y0)),
                   (x1 + 0 * t, y0 + t * (y1 - y0))):
        px.append(ax)
        py.append(ay)
    return np.concatenate(px), np.concatenate(py)


def jittered(rows, cols, seed, pitch=10.0):
    """A curvilinear grid of `pitch` pixels with nodes moved by up to a quarter of it, and a smooth field on it."""
    x, y = wc.node_grid(rows, cols, pitch, pitch, r0=7.3, c0=4.6, jitter=0.25, seed=seed)
    xs, ys = wc.smooth_source(x, y, seed)
    return x, y, xs, ys


def folded_grid():
    """A regular 5 x 6 grid of 10 pixels with node (2, 2) moved from x = 20 to x = 37, across its neighbour at x = 30: the four
    cells around it overlap."""
    x, y = wc.node_grid(5, 6, 10, 10)
    x[2, 2] = 37.0
    xs, ys = wc.smooth_source(x, y, 90)
    return x, y, xs, ys


def stretched_grid():
    """The 40 x 40 grid with the two ends of the main diagonal of cell (20, 20) moved beyond opposite corners of the grid: the
    box of that cell (and of its neighbours) spans every bucket."""
    x, y, xs, ys = jittered(40, 40, 95)
    x[20, 20], y[20, 20] = x.min() - 5.0, y.min() - 5.0
    x[21, 21], y[21, 21] = x.max() + 5.0, y.max() + 5.0
    return x, y, xs, ys


def three_fields():
    """Three consecutive fields for advect, each on a grid of its own, the second with holes."""
    fields = []
    for k in range(3):
        x, y, xs, ys = jittered(9, 11, 70 + k)
        fields.append((x, y, xs, ys, wc.holes(x.shape, 70 + k, share=0.05)) if k == 1 else (x, y, xs, ys))
    return fields


def _cases():
    out = []
    for diag in DIAGONALS:
        # ---- the fractional grids of the warp's cases, points in and around them: the general position
        for base in ('curvi_frac_', 'holed_'):
            w = wc.BY_NAME[base + diag]
            px, py = around(w['x'], w['y'], 1500, len(out))
            out.append(case(base + diag, w['x'], w['y'], w['xs'], w['ys'], px, py, valid=w['valid'], diagonal=diag))
        # ---- degenerate triangles, and a grid without a cell
        for base in ('coincident_nodes', 'one_row_of_nodes'):
            w = wc.BY_NAME[base]
            px, py = around(w['x'], w['y'], 600, len(out), margin=5.0)
            if base == 'coincident_nodes':
                qx, qy = nodes_midpoints_rim(w['x'], w['y'])
                px, py = np.concatenate([px, qx]), np.concatenate([py, qy])
            out.append(case('%s_%s' % (base, diag), w['x'], w['y'], w['xs'], w['ys'], px, py, diagonal=diag))
        # ---- an integer grid: points on nodes, on edge midpoints and on the rim (Ed == 0 everywhere it matters)
        x, y = wc.node_grid(5, 6, 10, 10)
        xs, ys = wc.smooth_source(x, y, 85)
        px, py = nodes_midpoints_rim(x, y)
        out.append(case('integer_grid_' + diag, x, y, xs, ys, px, py, diagonal=diag))
        # ---- the smallest grid with a cell
        x, y = np.array([[2.0, 9.5], [1.5, 11.0]]), np.array([[1.0, 2.5], [8.0, 7.5]])
        px, py = around(x, y, 300, len(out), margin=3.0)
        qx, qy = nodes_midpoints_rim(x, y)
        out.append(case('two_by_two_' + diag, x, y, x * 1.1 + 3.0, y * 0.9 - 2.0, np.concatenate([px, qx]), np.concatenate([py, qy]),
                        diagonal=diag))
        # ---- overlapping triangles: the lowest number wins
        x, y, xs, ys = folded_grid()
        rng = np.random.default_rng(91)
        out.append(case('folded_' + diag, x, y, xs, ys, rng.uniform(15, 45, 4000), rng.uniform(5, 35, 4000), diagonal=diag))
    # ---- the bucket route: above SID_TRACK_BRUTE_CELLS cells, the same points on a sub-grid below it, and index rectangles
    #      that span the grid
    x, y, xs, ys = jittered(40, 40, 95)
    px, py = around(x, y, 20000, 96)
    out.append(case('bucket_40x40', x, y, xs, ys, px, py))
    out.append(case('bucket_subgrid', x[:8, :8], y[:8, :8], xs[:8, :8], ys[:8, :8], px, py, diagonal='main'))
    valid = wc.holes(x.shape, 97, share=0.1)
    out.append(case('bucket_holed', x, y, xs, ys, px, py, valid=valid, diagonal='anti'))
    x, y, xs, ys = stretched_grid()
    out.append(case('bucket_stretched', x, y, xs, ys, px, py))
    return out


CASES = _cases()
NAMES = [c['name'] for c in CASES]
BY_NAME = dict(zip(NAMES, CASES))
assert len(BY_NAME) == len(CASES)

_expected = {}


def expected(name, closed):
    """The specification's result of a case, computed once and shared (read-only).  The specification runs with the closed rule;
    without it the points that rule gave a triangle (`shut`) have none - the rule adds points and changes no other."""
    if name not in _expected:
        from tests import track_spec as ts
        c = BY_NAME[name]
        res = ts.track(c['x'], c['y'], c['xs'], c['ys'], c['valid'], c['diagonal'], c['px'], c['py'], closed=True)
        opened = dict(res, sx=np.where(res['shut'], np.nan, res['sx']), sy=np.where(res['shut'], np.nan, res['sy']),
                      tri=np.where(res['shut'], -1, res['tri']).astype(np.int32), shut=np.zeros_like(res['shut']))
        for r in (res, opened):
            for v in r.values():
                v.setflags(write=False)
        _expected[name] = {True: res, False: opened}
    return _expected[name][bool(closed)]


def check(got, name, closed, what):
    """got = (sx, sy, tri): bit for bit the specification's."""
    from tests import track_spec as ts
    exp = expected(name, closed)
    for key, g in zip(('sx', 'sy', 'tri'), got):
        assert g is not None and g.dtype == exp[key].dtype and g.shape == exp[key].shape, '%s %s: %s' % (name, what, key)
        if not ts.same_bits(g, exp[key]):
            diff = np.nonzero(np.ascontiguousarray(g).view(np.uint8).reshape(len(g), -1)
                              != np.ascontiguousarray(exp[key]).view(np.uint8).reshape(len(g), -1))[0]
            k = int(diff[0])
            raise AssertionError('%s %s (closed=%s): %s differs from the specification at %d points, first %d = (%r, %r): got %r, expected %r'
                                 % (name, what, closed, key, len(set(diff.tolist())), k, BY_NAME[name]['px'][k], BY_NAME[name]['py'][k],
                                    g[k], exp[key][k]))
