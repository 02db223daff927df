"""GPU: the first-guess evaluation (include/sid_fg.h) on the cases of tests/fg_cases.py against the specification
tests/fg_spec.py - every assertion an equality, bit for bit, on the bucket route and on the brute-force route
(SID_FG_NO_GRID=1), with the route a call took read from sid_fg_debug_route.  tests/test_fg_spec_host.py holds the specification
against SciPy on the CPU."""
import numpy as np
import pytest
from scipy.interpolate import LinearNDInterpolator
from scipy.spatial import Delaunay

from sea_ice_drift_amd import _capi, lib
from tests import fg_cases as fc
from tests import fg_knn_cases as kc
from tests import fg_spec as spec

pytestmark = pytest.mark.gpu


def same_bits(got, exp):
    """NaN at the same places, every other value the same 64 bits (a zero's sign included)."""
    got, exp = np.ascontiguousarray(got, dtype=np.float64), np.ascontiguousarray(exp, dtype=np.float64)
    assert got.shape == exp.shape
    np.testing.assert_array_equal(np.isnan(got), np.isnan(exp))
    fin = ~np.isnan(exp)
    np.testing.assert_array_equal(got[fin].view(np.int64), exp[fin].view(np.int64))


def route_env(monkeypatch, brute):
    if brute:
        monkeypatch.setenv('SID_FG_NO_GRID', '1')
    else:
        monkeypatch.delenv('SID_FG_NO_GRID', raising=False)


def brute_plan(n_simp, n_q):
    """ychunks, chunk of the brute-force point location, from first_guess.hip: >= 2048 blocks, whole tiles of 256 simplices."""
    qb, tiles = -(-n_q // 256), -(-n_simp // 256)
    ychunks = min(1 if qb >= 2048 else -(-2048 // qb), tiles)
    chunk = -(-tiles // ychunks) * 256
    return -(-n_simp // chunk), chunk


@pytest.mark.parametrize('brute', [False, True], ids=['default', 'no_grid'])
@pytest.mark.parametrize('name', sorted(fc.interp_cases()))
def test_interpolation_equals_the_specification(monkeypatch, name, brute):
    c = fc.interp_cases()[name]
    eout, esx, edoubt, det = fc.expected(name)
    route_env(monkeypatch, brute)
    out, sx, doubt = _capi.fg_interp_linear(c['pts'], c['simplices'], c['values'], c['q'], details=True)
    route = _capi.fg_debug_route()
    monkeypatch.delenv('SID_FG_NO_GRID', raising=False)
    np.testing.assert_array_equal(sx, esx)
    np.testing.assert_array_equal(doubt, edoubt)
    same_bits(out, eout)
    ns, nq = len(c['simplices']), len(c['q'])
    entries, capacity = spec.bucket_entries(c['pts'], c['simplices'], det['ok'])
    assert capacity == 8 * ns + 128 * 128
    if brute:
        assert (route['buckets'], route['entries'], route['capacity']) == (0, 0, capacity)
    else:                                                                  # the lists are counted, and walked where they fit
        assert (route['buckets'], route['entries'], route['capacity']) == (int(entries <= capacity), entries, capacity)
        if c['route'] is not None:
            assert {k: route[k] for k in c['route']} == c['route']
    if route['buckets']:
        assert (route['ychunks'], route['chunk']) == (0, 0)
    else:
        assert (route['ychunks'], route['chunk']) == brute_plan(ns, nq)


def test_brute_force_chunks_around_the_tile(monkeypatch):
    """About 600 simplices and at most 256 queries: 3 chunks of 256; 255 and 256 simplices: one chunk; 257: two; 513: three."""
    route_env(monkeypatch, True)
    seen = {}
    for name in ('scattered_300_nq1', 'scattered_300_nq255', 'scattered_300_nq256', 'scattered_300_ns255', 'scattered_300_ns256',
                 'scattered_300_ns257', 'scattered_300_ns513'):
        c = fc.interp_cases()[name]
        _capi.fg_interp_linear(c['pts'], c['simplices'], c['values'], c['q'])
        r = _capi.fg_debug_route()
        seen[name] = (r['ychunks'], r['chunk'])
    monkeypatch.delenv('SID_FG_NO_GRID')
    assert 512 < len(fc.interp_cases()['scattered_300']['simplices']) <= 768
    assert seen == {'scattered_300_nq1': (3, 256), 'scattered_300_nq255': (3, 256), 'scattered_300_nq256': (3, 256),
                    'scattered_300_ns255': (1, 256), 'scattered_300_ns256': (1, 256), 'scattered_300_ns257': (2, 256),
                    'scattered_300_ns513': (3, 256)}


@pytest.mark.parametrize('brute', [False, True], ids=['default', 'no_grid'])
@pytest.mark.parametrize('name', sorted(fc.dist_cases()))
def test_nearest_distance_equals_the_specification(monkeypatch, name, brute):
    seeds, q, buckets = fc.dist_cases()[name]
    route_env(monkeypatch, brute)
    got = _capi.fg_nearest_dist(seeds, q)
    route = _capi.fg_debug_route()
    monkeypatch.delenv('SID_FG_NO_GRID', raising=False)
    same_bits(got, fc.expected_dist(name))
    use = buckets and not brute
    assert route == dict(buckets=int(use), entries=len(seeds) if use else 0, capacity=len(seeds), ychunks=0, chunk=0)


@pytest.mark.parametrize('brute', [False, True], ids=['default', 'no_grid'])
def test_distance_image_rows_are_not_columns(monkeypatch, brute):
    seeds = fc.image_seeds()
    route_env(monkeypatch, brute)
    for rows, cols in fc.IMAGE_SHAPES:
        got = _capi.fg_distance_image(seeds, rows, cols)
        assert _capi.fg_debug_route()['buckets'] == int(not brute)
        same_bits(got, spec.distance_image(seeds, rows, cols))
    monkeypatch.delenv('SID_FG_NO_GRID', raising=False)


@pytest.mark.parametrize('name', ['lattice_jitter_12x13', 'lattice_int_17x17', 'scattered_300', 'scattered_300_offset_2p20'])
def test_interpolation_near_rounds_like_scipy_everywhere(name):
    """The product's entry (flagged queries go to SciPy): SciPy's hull membership and rounded value at EVERY query, the ones on
    vertices and edges and the non-finite ones included."""
    c = fc.interp_cases()[name]
    pts, vals, q = c['pts'], c['values'], c['q']
    exp = LinearNDInterpolator(Delaunay(pts), vals)(q)
    xg, yg = lib.interpolation_near(pts[:, 1], pts[:, 0], vals[:, 0], vals[:, 1], q[:, 1], q[:, 0], first_guess_device=0)
    both = np.stack([xg, yg], axis=1)
    np.testing.assert_array_equal(np.isnan(both), np.isnan(exp))
    fin = ~np.isnan(exp[:, 0])
    np.testing.assert_array_equal(np.round(both[fin]), np.round(exp[fin]))


def test_pool_is_shared_by_the_entry_points():
    """One grow-only block serves the interpolation, the distances and sid_fg_knn, carved anew per call: a large interpolation,
    the distances, the k nearest and a one-triangle interpolation give what each gives on a pool released just before."""
    L = _capi.lib()
    big, tri = fc.interp_cases()['scattered_300'], fc.interp_cases()['triangle_120']
    seeds, q, _ = fc.dist_cases()['seeds_257']
    ks, kv, kq, kk, kmax = kc.build()['uniform300_k5']
    calls = [lambda: _capi.fg_interp_linear(big['pts'], big['simplices'], big['values'], big['q'], details=True),
             lambda: (_capi.fg_nearest_dist(seeds, q),),
             lambda: _capi.fg_knn(ks, kv, kq, k=kk, max_dist=kmax, details=True),
             lambda: _capi.fg_interp_linear(tri['pts'], tri['simplices'], tri['values'], tri['q'], details=True)]
    warm = [f() for f in calls]
    cold = []
    for f in calls:
        assert L.sid_fg_release(0) == 0
        cold.append(f())
    for w, c in zip(warm, cold):
        for a, b in zip(w, c):
            if a.dtype == np.float64:
                same_bits(a, b)
            else:
                np.testing.assert_array_equal(a, b)
    same_bits(warm[0][0], fc.expected('scattered_300')[0])
    same_bits(warm[1][0], fc.expected_dist('seeds_257'))
    same_bits(warm[3][0], fc.expected('triangle_120')[0])
