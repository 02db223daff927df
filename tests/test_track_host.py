"""CPU tests of include/sid_track.h (libtrack.map_points, advect, round_trip): the host instance of the kernels' source
(device = -1) against the warp's specification at pixel centres and against tests/track_spec.py at arbitrary points, bit for
bit; the folded mesh; the bucket route against every-cell runs; the Python layer; every argument error; the exported symbols;
the stand-alone check of the bucket index."""
import ctypes
import hashlib
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from sea_ice_drift_amd import _capi, libtrack, synthetic
from tests import track_cases as tc
from tests import track_spec as ts
from tests import warp_cases as wc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VP = ctypes.c_void_p
ERR_ARG, ERR_UNSUPPORTED = -1, -4          # checked against include/sid_pm.h below
POISON_F, POISON_I, GUARD = -12345.678, 113, 3


def vp(a):
    return VP(a.ctypes.data) if a is not None else None


def raw_call(device, x, y, xs, ys, valid, grid, diagonal, flags, px, py, n, sx, sy, tri):
    """sid_track_points with every argument as given (arrays or None)."""
    return _capi.lib().sid_track_points(device, vp(x), vp(y), vp(xs), vp(ys), vp(valid), grid[0], grid[1], diagonal, flags,
                                        vp(px), vp(py), n, vp(sx), vp(sy), vp(tri))


def host_points(x, y, xs, ys, valid, diagonal, px, py, closed, want_tri=True):
    """sid_track_points(device = -1) into poisoned outputs with guard elements behind them -> sx, sy, tri."""
    x, y, xs, ys = [np.ascontiguousarray(q, dtype=np.float64) for q in (x, y, xs, ys)]
    px, py = np.ascontiguousarray(px, dtype=np.float64), np.ascontiguousarray(py, dtype=np.float64)
    n = px.size
    sx, sy = np.full(n + GUARD, POISON_F), np.full(n + GUARD, POISON_F)
    tri = np.full(n + GUARD, POISON_I, dtype=np.int32) if want_tri else None
    rc = raw_call(-1, x, y, xs, ys, valid, x.shape, _capi.GRID_DIAGONALS[diagonal], 1 if closed else 0, px, py, n, sx, sy, tri)
    assert rc == 0, _capi.lib().sid_track_last_error()
    assert (sx[n:] == POISON_F).all() and (sy[n:] == POISON_F).all() and (tri is None or (tri[n:] == POISON_I).all()), 'written beyond n'
    return sx[:n].copy(), sy[:n].copy(), (tri[:n].copy() if want_tri else None)


def host_case(c, closed):
    return host_points(c['x'], c['y'], c['xs'], c['ys'], c['valid'], c['diagonal'], c['px'], c['py'], closed)


# ---------------------------------------------------------------- 1. against the existing warp specification
LATTICES = [n for n in wc.NAMES if wc.BY_NAME[n]['out_shape'][0] * wc.BY_NAME[n]['out_shape'][1] > 0]


def test_every_non_empty_warp_case_is_used():
    assert len(LATTICES) == 48 and len(wc.NAMES) == 49


@pytest.mark.parametrize('name', LATTICES)
def test_pixel_centres_equal_the_warp_specification(name):
    """Without the closed flag the pixel-centre lattice of a warp case gets the image warp's sx, sy and owners; with it the
    same wherever the warp owns the pixel, and every point it adds lies on an edge (Ed == 0) of the triangle that has it."""
    c, e = wc.BY_NAME[name], wc.expected(name)
    assert e['owners'].max() <= 1                                         # (none of these cases is folded)
    ro, co = c['out_shape']
    rr, cc = np.meshgrid(np.arange(ro, dtype=np.float64), np.arange(co, dtype=np.float64), indexing='ij')
    sx, sy, tri = host_points(c['x'], c['y'], c['xs'], c['ys'], c['valid'], c['diagonal'], cc.ravel(), rr.ravel(), False)
    assert ts.same_bits(sx.reshape(ro, co), e['sx']) and ts.same_bits(sy.reshape(ro, co), e['sy'])
    assert np.array_equal(tri.reshape(ro, co) >= 0, e['owners'] > 0)
    cx, cy, ctri = host_points(c['x'], c['y'], c['xs'], c['ys'], c['valid'], c['diagonal'], cc.ravel(), rr.ravel(), True)
    own = (e['owners'] == 1).ravel()
    assert ts.same_bits(cx[own], sx[own]) and ts.same_bits(cy[own], sy[own]) and np.array_equal(ctri[own], tri[own])
    extra = np.nonzero(~own & (ctri >= 0))[0]
    assert not np.isnan(cx[extra]).any() and np.isnan(cx[~own & (ctri < 0)]).all()
    xf, yf, t = c['x'].ravel(), c['y'].ravel(), e['triangles'].reshape(-1, 3)
    for k in extra:
        d = ts.edge_sides(xf, yf, t[ctri[k]], cc.ravel()[k], rr.ravel()[k])
        assert min(d) == 0, (name, k, d)


# ---------------------------------------------------------------- 2. - 4. against track_spec
@pytest.mark.parametrize('closed', [True, False], ids=['closed', 'open'])
@pytest.mark.parametrize('name', tc.NAMES)
def test_host_instance_equals_spec(name, closed):
    tc.check(host_case(tc.BY_NAME[name], closed), name, closed, 'host instance')


def test_cases_cover_what_they_claim():
    e = tc.expected
    for diag in tc.DIAGONALS:
        for base in ('curvi_frac_', 'holed_'):
            r = e(base + diag, True)
            assert (r['tri'] >= 0).sum() > 500 and (r['tri'] < 0).sum() > 200 and r['owners'].max() == 1
            c = tc.BY_NAME[base + diag]
            assert (c['px'] != np.floor(c['px'])).sum() > 1000
        t = e('holed_' + diag, True)['triangles']
        assert ((t[..., 0, 0] >= 0) & (t[..., 1, 0] < 0)).any() and (t[..., 0, 0] < 0).any()           # one triangle, none
        c, r = tc.BY_NAME['coincident_nodes_' + diag], e('coincident_nodes_' + diag, True)
        xf, yf = c['x'].ravel(), c['y'].ravel()
        det = [(xf[b] - xf[a]) * (yf[q] - yf[a]) - (xf[q] - xf[a]) * (yf[b] - yf[a]) for a, b, q in r['triangles'].reshape(-1, 3)]
        assert sum(d == 0 for d in det) >= 2 and (r['tri'] >= 0).sum() > 100
        assert (e('one_row_of_nodes_' + diag, True)['tri'] == -1).all()
        # the integer grid: the open rule leaves the first column and the last row of nodes to nobody, the closed rule has all 30
        c, closed, opened = tc.BY_NAME['integer_grid_' + diag], e('integer_grid_' + diag, True), e('integer_grid_' + diag, False)
        assert np.array_equal(c['px'][:30], c['x'].ravel()) and np.array_equal(c['py'][:30], c['y'].ravel())
        assert (closed['tri'][:30] >= 0).all()
        assert np.array_equal(opened['tri'][:30].reshape(5, 6) < 0, (c['x'] == 0) | (c['y'] == 40))
        assert closed['shut'].sum() >= 10 + 41 + 41 and closed['owners'].max() == 1
        r = e('two_by_two_' + diag, True)
        assert (r['tri'] == 0).any() and (r['tri'] == 1).any() and (r['tri'] == -1).any() and r['tri'].max() == 1
        # the folded mesh: points with two owners and more, the lowest-numbered one's values returned
        r = e('folded_' + diag, True)
        assert (r['owners'] >= 2).sum() > 100, (r['owners'] >= 2).sum()
        for name in ('folded_' + diag, 'curvi_frac_' + diag, 'integer_grid_' + diag):                  # (how `expected` derives the open rule)
            c, opened = tc.BY_NAME[name], e(name, False)
            direct = ts.track(c['x'], c['y'], c['xs'], c['ys'], c['valid'], c['diagonal'], c['px'], c['py'], closed=False)
            assert all(ts.same_bits(direct[k], opened[k]) for k in ('sx', 'sy', 'tri', 'shut'))
    assert (e('folded_shorter', True)['owners'] == 3).sum() > 100         # (298 of these 4000 seeded points)
    for name in tc.NAMES:                                                 # every case: the special points and the duplicates
        c, r = tc.BY_NAME[name], e(name, True)
        k = 2 * len(tc.SPECIAL)
        assert (r['tri'][-k:] == -1).all() and np.isnan(r['sx'][-k:]).all() and np.isnan(r['sy'][-k:]).all()
    cells = {n: (tc.BY_NAME[n]['x'].shape[0] - 1) * (tc.BY_NAME[n]['x'].shape[1] - 1) for n in tc.NAMES}
    assert cells['bucket_subgrid'] < tc.BRUTE <= cells['curvi_frac_main'] < cells['bucket_40x40'] == cells['bucket_stretched']
    assert len(tc.BY_NAME['bucket_40x40']['px']) >= 20000 and (e('bucket_40x40', True)['tri'] >= 0).sum() > 10000
    assert (e('bucket_subgrid', True)['tri'] >= 0).sum() > 300
    c = tc.BY_NAME['bucket_stretched']                                    # one cell's box holds every node of the grid
    ring_x, ring_y = c['x'][20:22, 20:22], c['y'][20:22, 20:22]
    assert ring_x.min() == c['x'].min() and ring_x.max() == c['x'].max() and ring_y.min() == c['y'].min() and ring_y.max() == c['y'].max()
    assert e('bucket_stretched', True)['owners'].max() >= 2


def test_no_points_and_no_cells():
    c = tc.BY_NAME['curvi_frac_main']
    sx, sy, tri = host_points(c['x'], c['y'], c['xs'], c['ys'], None, 'main', np.zeros(0), np.zeros(0), True)
    assert sx.shape == sy.shape == tri.shape == (0,)
    for sl in ((slice(0, 1), slice(None)), (slice(None), slice(0, 1)), (slice(0, 0), slice(0, 0))):
        g = [np.ascontiguousarray(c[k][sl]) for k in ('x', 'y', 'xs', 'ys')]
        sx, sy, tri = host_points(*g, None, 'main', c['px'], c['py'], True)
        assert np.isnan(sx).all() and np.isnan(sy).all() and (tri == -1).all()
    sx, sy, tri = host_points(c['x'], c['y'], c['xs'], c['ys'], None, 'main', c['px'], c['py'], True, want_tri=False)
    assert tri is None and ts.same_bits(sx, tc.expected('curvi_frac_main', True)['sx'])


CHILD = """
import hashlib, sys
sys.path.insert(0, %r)
from tests import track_cases as tc
from tests.test_track_host import host_case
for name in sys.argv[1:]:
    for closed in (True, False):
        print(name, closed, hashlib.sha256(b''.join(a.tobytes() for a in host_case(tc.BY_NAME[name], closed))).hexdigest())
"""


def test_bucket_route_equals_every_cell_route():
    """The grids above SID_TRACK_BRUTE_CELLS again in a child process under SID_TRACK_NO_GRID=1: identical bytes."""
    names = ['bucket_40x40', 'bucket_holed', 'bucket_stretched']
    assert not os.environ.get('SID_TRACK_NO_GRID')
    env = dict(os.environ, SID_TRACK_NO_GRID='1')
    p = subprocess.run([sys.executable, '-c', CHILD % ROOT] + names, env=env, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       universal_newlines=True)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = p.stdout.split('\n')
    for name in names:
        for closed in (True, False):
            digest = hashlib.sha256(b''.join(a.tobytes() for a in host_case(tc.BY_NAME[name], closed))).hexdigest()
            assert '%s %s %s' % (name, closed, digest) in lines, (name, closed)


# ---------------------------------------------------------------- 5. the Python layer
def test_map_points_takes_any_shape():
    c, e = tc.BY_NAME['curvi_frac_anti'], tc.expected('curvi_frac_anti', True)
    grid = dict(valid=c['valid'], diagonal='anti', device=-1)
    for shape in ((1200,), (3, 4, 100), (2, 600), (0,), (2, 0, 3), ()):
        n = int(np.prod(shape))
        px, py = c['px'][:n].reshape(shape), c['py'][:n].reshape(shape)
        sx, sy, tri = libtrack.map_points(c['x'], c['y'], c['xs'], c['ys'], px, py, return_triangle=True, **grid)
        assert sx.shape == sy.shape == tri.shape == shape and sx.dtype == np.float64 and tri.dtype == np.int32
        assert ts.same_bits(sx.ravel(), e['sx'][:n]) and ts.same_bits(sy.ravel(), e['sy'][:n]) and ts.same_bits(tri.ravel(), e['tri'][:n])
        assert len(libtrack.map_points(c['x'], c['y'], c['xs'], c['ys'], px, py, **grid)) == 2
    view = np.stack([c['px'], c['py']], axis=1)                           # points as strided views, a grid as a transposed view
    sx, sy = libtrack.map_points(np.asfortranarray(c['x']), c['y'], c['xs'], c['ys'], view[:, 0], view[:, 1], **grid)
    assert ts.same_bits(sx, e['sx']) and ts.same_bits(sy, e['sy'])
    opened = tc.expected('curvi_frac_anti', False)
    sx, sy = libtrack.map_points(c['x'], c['y'], c['xs'], c['ys'], c['px'], c['py'], closed=False, **grid)
    assert ts.same_bits(sx, opened['sx']) and ts.same_bits(sy, opened['sy'])


def test_advect_equals_chained_specification_calls():
    fields = tc.three_fields()
    px, py = tc.around(fields[0][0], fields[0][1], 800, 75, margin=6.0)
    px, py = np.append(px, [np.nan, 20.0]).reshape(2, -1), np.append(py, [20.0, np.inf]).reshape(2, -1)
    ex, ey, steps, path = px, py, np.zeros(px.shape, dtype=np.int32), [(px, py)]
    for f in fields:
        r = ts.track(f[0], f[1], f[2], f[3], f[4] if len(f) == 5 else None, 'shorter', ex, ey, closed=True)
        ex, ey = r['sx'], r['sy']
        steps = steps + (np.isfinite(ex) & np.isfinite(ey))
        path.append((ex, ey))
    gx, gy, gsteps, path_x, path_y = libtrack.advect(px, py, fields, return_path=True, device=-1)
    assert ts.same_bits(gx, ex) and ts.same_bits(gy, ey) and gsteps.dtype == np.int32 and np.array_equal(gsteps, steps)
    assert path_x.shape == path_y.shape == (4,) + px.shape
    assert all(ts.same_bits(path_x[k], path[k][0]) and ts.same_bits(path_y[k], path[k][1]) for k in range(4))
    assert set(np.unique(steps)) == {0, 1, 2, 3}                          # points are lost at every stage
    lost = steps < 3
    assert np.isnan(gx[lost]).all() and np.isfinite(gx[~lost]).all()
    for k in range(1, 4):                                                 # NaN from then on
        assert np.isnan(path_x[k:, steps < k]).all()
    again = libtrack.advect(px, py, fields, device=-1)
    assert len(again) == 3 and ts.same_bits(again[0], gx) and ts.same_bits(again[2], gsteps)
    same, _, none = libtrack.advect(px, py, [], device=-1)
    assert ts.same_bits(same, px) and not none.any()
    with pytest.raises(ValueError, match='field 1 must be'):
        libtrack.advect(px, py, [fields[0], fields[1][:3]], device=-1)


def test_round_trip_equals_the_specification():
    x, y, xs, ys = tc.jittered(9, 11, 80)
    xb, yb, _, _ = tc.jittered(12, 13, 81, pitch=8.0)
    xbs, ybs = xb - 2.0 + 0.01 * yb, yb + 1.5 - 0.02 * xb
    valid, valid_b = wc.holes(x.shape, 80, share=0.1), wc.holes(xb.shape, 81, share=0.05)
    xs[3, 3], y[4, 4] = np.nan, np.inf
    for diag in tc.DIAGONALS:
        for closed in (True, False):
            dx, dy = libtrack.round_trip(x, y, xs, ys, xb, yb, xbs, ybs, valid=valid, valid_b=valid_b, diagonal=diag, closed=closed, device=-1)
            use = ts.ws.usable(x, y, xs, ys, valid)
            r = ts.track(xb, yb, xbs, ybs, valid_b, diag, np.where(use, xs, np.nan), np.where(use, ys, np.nan), closed=closed)
            assert ts.same_bits(dx, r['sx'] - x) and ts.same_bits(dy, r['sy'] - y)
            assert np.isnan(dx[~use]).all() and np.isfinite(dx).sum() > 30 and dx.shape == x.shape


def test_constant_shift_is_exact_at_nodes_and_the_rim_is_the_closed_rule():
    x, y = wc.node_grid(5, 6, 10, 10)
    xs, ys = x + 3.5, y - 2.25
    for diag in tc.DIAGONALS:
        sx, sy = libtrack.map_points(x, y, xs, ys, x, y, diagonal=diag, device=-1)
        assert np.array_equal(sx, xs) and np.array_equal(sy, ys)                    # closed: every node, the rim included
        sx, sy = libtrack.map_points(x, y, xs, ys, x, y, diagonal=diag, closed=False, device=-1)
        rim = (x == 0) | (y == 40)
        assert np.isnan(sx[rim]).all() and np.isnan(sy[rim]).all() and rim.sum() == 10
        assert np.array_equal(sx[~rim], xs[~rim]) and np.array_equal(sy[~rim], ys[~rim])


def test_affine_field_is_reproduced():
    """An affine field is its own piecewise-linear interpolant: on a jittered grid of about 20 pixels with coordinates up to
    400 the result is the field to 1e-9 pixels (the specification's own error was measured at 1.1e-13; the kernels equal it
    bit for bit, so the bound is on the definition)."""
    x, y = wc.node_grid(20, 20, 20, 20, r0=5.5, c0=8.25, jitter=0.25, seed=7)
    f = lambda a, b: (12.5 + 0.98 * a - 0.07 * b, -3.25 + 0.05 * a + 1.03 * b)            # noqa: E731
    xs, ys = f(x, y)
    rng = np.random.default_rng(8)
    px, py = rng.uniform(x.min(), x.max(), 5000), rng.uniform(y.min(), y.max(), 5000)
    sx, sy = libtrack.map_points(x, y, xs, ys, px, py, device=-1)
    ok = np.isfinite(sx)
    ex, ey = f(px, py)
    worst = max(np.abs(sx[ok] - ex[ok]).max(), np.abs(sy[ok] - ey[ok]).max())
    print('affine field: %d points inside, max error %.3e px' % (ok.sum(), worst))
    assert ok.sum() > 4000 and worst <= 1e-9


def test_round_trip_through_the_inverse_field_is_zero():
    """The synthetic pair's true field on nodes 40 pixels apart, and as the backward field the same nodes the other way round:
    every forward end point is a node of the backward grid, so the round trip is exactly 0 at every node."""
    y, x = np.meshgrid(np.arange(0.0, 400.0, 40.0), np.arange(0.0, 400.0, 40.0), indexing='ij')
    dc, dr = synthetic.true_displacement(x, y)
    xs, ys = x + dc, y + dr
    dx, dy = libtrack.round_trip(x, y, xs, ys, xs, ys, x, y, device=-1)
    assert dx.shape == x.shape and not dx.any() and not dy.any()
    dx, dy = libtrack.round_trip(x, y, xs, ys, xs, ys, x, y, closed=False, device=-1)
    own = np.isfinite(dx)
    assert 60 <= own.sum() < 100 and not dx[own].any() and not dy[own].any() and np.isnan(dy[~own]).all()


def test_sea_ice_drift_wrappers():
    """SeaIceDrift.track_points and get_round_trip on ArrayNansat objects whose georeferences differ: positions go through
    transform_points, the rest is libtrack on the pixel nodes."""
    from sea_ice_drift_amd.domain import ArrayNansat
    from sea_ice_drift_amd.seaicedrift import SeaIceDrift
    img1, img2 = synthetic.make_pair(400, 400, seed=17)
    n1 = ArrayNansat(img1, origin=(10.0, 70.0), matrix=((0.002, 0.0), (0.0, -0.001)))
    n2 = ArrayNansat(img2[:380], origin=(10.1, 70.05), matrix=((0.0025, 0.0001), (0.0, -0.0012)))
    y, x = np.meshgrid(np.arange(0.0, 400.0, 40.0), np.arange(0.0, 400.0, 40.0), indexing='ij')
    dc, dr = synthetic.true_displacement(x, y)
    lons, lats = n1.transform_points(x, y, 0)
    lon2, lat2 = n2.transform_points(x + dc, y + dr, 0)
    sid = SeaIceDrift(n1, n2)
    rng = np.random.default_rng(3)
    px, py = rng.uniform(-20, 400, (4, 50)), rng.uniform(-20, 400, (4, 50))
    lon, lat = n1.transform_points(px, py, 0)
    lon_pts, lat_pts = sid.track_points(lon, lat, lons, lats, lon2, lat2, device=-1)
    x1, y1 = n1.transform_points(lons, lats, 1)
    x2, y2 = n2.transform_points(lon2, lat2, 1)
    qx, qy = n1.transform_points(lon, lat, 1)
    sx, sy = libtrack.map_points(x1, y1, x2, y2, qx, qy, device=-1)
    elon, elat = n2.transform_points(sx, sy, 0)
    inside = np.isfinite(sx)
    assert lon_pts.shape == lat_pts.shape == (4, 50) and 100 < inside.sum() < 200
    assert np.array_equal(lon_pts[inside], elon[inside]) and np.array_equal(lat_pts[inside], elat[inside])
    assert np.isnan(lon_pts[~inside]).all() and np.isnan(lat_pts[~inside]).all()
    tx, ty = synthetic.true_displacement(qx, qy)                          # the field is smooth: the mesh follows it to a pixel
    assert np.abs(sx - (qx + tx))[inside].max() < 1.0 and np.abs(sy - (qy + ty))[inside].max() < 1.0
    # the backward field on a grid of its own (35 pixels, image 2's frame): the inverse displacement at its nodes, to first order
    yb, xb = np.meshgrid(np.arange(0.0, 380.0, 35.0), np.arange(0.0, 400.0, 35.0), indexing='ij')
    bc, br = synthetic.true_displacement(xb, yb)
    lons_b, lats_b = n2.transform_points(xb, yb, 0)
    lon1_b, lat1_b = n1.transform_points(xb - bc, yb - br, 0)
    dx, dy = sid.get_round_trip(lons, lats, lon2, lat2, lons_b, lats_b, lon1_b, lat1_b, device=-1)
    xb_, yb_ = n2.transform_points(lons_b, lats_b, 1)
    xbs_, ybs_ = n1.transform_points(lon1_b, lat1_b, 1)
    ex, ey = libtrack.round_trip(x1, y1, x2, y2, xb_, yb_, xbs_, ybs_, device=-1)
    assert dx.shape == lons.shape and ts.same_bits(dx, ex) and ts.same_bits(dy, ey)
    ok = np.isfinite(dx)
    assert ok.sum() > 50 and np.hypot(dx[ok], dy[ok]).max() < 1.0
    with pytest.raises(ValueError, match='2-D grids of one shape'):
        sid.track_points(lon, lat, lons, lats, lon2[:5], lat2)
    with pytest.raises(ValueError, match='lon and lat must have one shape'):
        sid.track_points(lon, lat[:2], lons, lats, lon2, lat2)
    with pytest.raises(ValueError, match='lons_b, lats_b, lon1_b, lat1_b must be 2-D grids'):
        sid.get_round_trip(lons, lats, lon2, lat2, lons_b, lats_b[:3], lon1_b, lat1_b)


# ---------------------------------------------------------------- 6. argument and error paths
def good_args():
    x, y = wc.node_grid(3, 4, 5, 5)
    return dict(device=-1, x=x, y=y, xs=x.copy(), ys=y.copy(), valid=np.ones(x.shape, np.uint8), grid=x.shape, diagonal=0, flags=1,
                px=np.array([1.0, 2.0, 3.0]), py=np.array([1.0, 2.0, 3.0]), n=3, sx=np.zeros(3), sy=np.zeros(3),
                tri=np.zeros(3, np.int32))


BUF = np.zeros(64)
HEADER_ERRORS = [
    ('null x', dict(x=None), ERR_ARG, 'null node grid'), ('null y', dict(y=None), ERR_ARG, 'null node grid'),
    ('null xs', dict(xs=None), ERR_ARG, 'null node grid'), ('null ys', dict(ys=None), ERR_ARG, 'null node grid'),
    ('null px', dict(px=None), ERR_ARG, 'null point array'), ('null py', dict(py=None), ERR_ARG, 'null point array'),
    ('null sx', dict(sx=None), ERR_ARG, 'null output'), ('null sy', dict(sy=None), ERR_ARG, 'null output'),
    ('negative grid rows', dict(grid=(-1, 4)), ERR_ARG, 'negative size'), ('negative grid cols', dict(grid=(3, -4)), ERR_ARG, 'negative size'),
    ('negative n', dict(n=-1), ERR_ARG, 'negative size'),
    ('diagonal', dict(diagonal=3), ERR_ARG, 'unknown diagonal code 3'), ('diagonal negative', dict(diagonal=-1), ERR_ARG, 'unknown diagonal'),
    ('flag', dict(flags=2), ERR_ARG, 'unknown flags 0x2'), ('flags', dict(flags=0x80000001), ERR_ARG, 'unknown flags'),
    ('sx is px', dict(px=BUF[:3], sx=BUF[:3]), ERR_ARG, 'an output overlaps an input'),
    ('sy inside py', dict(py=BUF[:3], sy=BUF[2:5]), ERR_ARG, 'an output overlaps an input'),
    ('sx inside x', dict(x=BUF[:12].reshape(3, 4), sx=BUF[11:14]), ERR_ARG, 'an output overlaps an input'),
    ('tri inside valid', dict(valid=BUF.view(np.uint8)[:12].reshape(3, 4), tri=BUF.view(np.int32)[2:5]), ERR_ARG, 'an output overlaps an input'),
    ('sy inside sx', dict(sx=BUF[:3], sy=BUF[2:5]), ERR_ARG, 'two outputs overlap'),
    ('tri inside sy', dict(sy=BUF[:3], tri=BUF.view(np.int32)[4:7]), ERR_ARG, 'two outputs overlap'),
    ('grid too large', dict(grid=(1 << 16, 1 << 15)), ERR_UNSUPPORTED, r'grid_rows \* grid_cols >= 2\^31'),
    ('triangle numbers too large', dict(grid=((1 << 15) + 1, (1 << 15) + 1)), ERR_UNSUPPORTED, r'tri wanted with 2\^30 cells or more'),
]


@pytest.mark.parametrize('what,change,code,message', HEADER_ERRORS, ids=[h[0] for h in HEADER_ERRORS])
def test_header_argument_errors(what, change, code, message):
    header = open(os.path.join(ROOT, 'include', 'sid_pm.h')).read()
    assert re.search(r'SID_PM_ERR_ARG\s+\(?-1\)?', header) and re.search(r'SID_PM_ERR_UNSUPPORTED\s+\(?-4\)?', header)
    assert raw_call(**good_args()) == 0
    for device in (-1, 0):                                 # found before any device call: the same without a GPU
        args = dict(good_args(), device=device)
        args.update(change)
        assert raw_call(**args) == code, what
        assert re.search(message, _capi.lib().sid_track_last_error().decode()), _capi.lib().sid_track_last_error()


def test_adjacent_buffers_and_no_points_are_fine():
    args = good_args()
    args.update(px=BUF[:3], py=BUF[3:6], sx=BUF[6:9], sy=BUF[9:12])
    assert raw_call(**args) == 0
    assert raw_call(**dict(good_args(), n=0, px=None, py=None, sx=None, sy=None, tri=None)) == 0
    assert raw_call(**dict(good_args(), n=0, device=0)) == 0


def test_python_argument_errors():
    x, y = wc.node_grid(3, 4, 5, 5)
    p = np.array([1.0, 2.0])
    ok = dict(x=x, y=y, xs=x.copy(), ys=y.copy(), px=p, py=p.copy(), device=-1)

    def call(**change):
        return libtrack.map_points(**dict(ok, **change))
    assert call()[0].shape == (2,)
    for name in ('x', 'y', 'xs', 'ys', 'px', 'py'):
        with pytest.raises(NotImplementedError, match=r'\b%s is float32' % name):
            call(**{name: ok[name].astype(np.float32)})
    with pytest.raises(ValueError, match='x, y, xs, ys must be 2-D arrays of one shape'):
        call(x=x[:, :3])
    with pytest.raises(ValueError, match='px and py must have one shape'):
        call(px=np.zeros(3))
    with pytest.raises(TypeError, match='valid is float64'):
        call(valid=np.ones(x.shape))
    with pytest.raises(ValueError, match='valid must have the shape'):
        call(valid=np.ones((3, 3), dtype=bool))
    with pytest.raises(ValueError, match='diagonal must be'):
        call(diagonal='both')
    with pytest.raises(ValueError, match='device must be a HIP device index'):
        call(device=-2)
    with pytest.raises(ValueError, match='diagonal must be'):
        libtrack.round_trip(x, y, x, y, x, y, x, y, diagonal='none', device=-1)
    with pytest.raises(ValueError, match='device must be a HIP device index'):
        libtrack.round_trip(x, y, x, y, x, y, x, y, device=-3)
    torch = pytest.importorskip('torch')
    with pytest.raises(TypeError, match='not a mix'):
        call(x=torch.from_numpy(x))
    with pytest.raises(TypeError, match='not a mix'):
        call(px=torch.from_numpy(p))
    with pytest.raises(TypeError, match='not a mix'):
        libtrack.advect(torch.from_numpy(p), p, [])
    with pytest.raises(TypeError, match='on one ROCm device'):
        libtrack.map_points(*[torch.from_numpy(q) for q in (x, y, x, y, p, p)])


def test_header_symbols_and_abi():
    header = open(os.path.join(ROOT, 'include', 'sid_track.h')).read()
    body = re.sub(r'/\*.*?\*/', '', header, flags=re.S)
    assert sorted(set(re.findall(r'\b(sid_track_\w+)\s*\(', body))) == sorted(_capi.TRACK_SYMBOLS)
    lib = _capi.lib()
    for name in _capi.TRACK_SYMBOLS:
        assert hasattr(lib, name), name
    assert lib.sid_pm_abi_version() == 6 and _capi.ABI_VERSION == 6
    assert int(re.search(r'SID_TRACK_CLOSED\s+(\d+)', header).group(1)) == _capi.TRACK_CLOSED
    assert int(re.search(r'SID_TRACK_BRUTE_CELLS\s+(\d+)', header).group(1)) == _capi.TRACK_BRUTE_CELLS
    assert lib.sid_track_release(-1) == 0                                 # nothing cached, no device: no HIP call


def test_bucket_index_check(tmp_path):
    """tests/cpp/track_bucket_check.cpp: csrc/track_bucket.h alone, under the address and undefined-behaviour sanitizers."""
    exe = str(tmp_path / 'track_bucket_check')
    subprocess.check_call(['g++', '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fsanitize=float-cast-overflow',
                           '-fno-sanitize-recover=all', '-o', exe, os.path.join(ROOT, 'tests', 'cpp', 'track_bucket_check.cpp')])
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    assert p.returncode == 0 and p.stdout.strip().endswith(' 0 violations'), p.stdout[-3000:]
