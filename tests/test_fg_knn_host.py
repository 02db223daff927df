"""The triangulation-free first guess (include/sid_fg.h sid_fg_knn) without a GPU: the library's host
instance (device = -1, the kernels' own source in a loop) against the NumPy specification tests/fg_knn_spec.py bit for bit,
and ``method='knn'`` through lib.interpolation_near, the prelude and SeaIceDrift on the host route."""
import ctypes as C
import os

import numpy as np
import pytest
from scipy.spatial import cKDTree

from sea_ice_drift_amd import _capi, lib, pmlib as my
from sea_ice_drift_amd.seaicedrift import SeaIceDrift
from tests import fg_knn_cases as cases
from tests import fg_knn_spec as spec


@pytest.mark.parametrize('name', sorted(cases.CASES))
def test_host_instance_equals_the_specification(name):
    s, v, q, k, md = cases.CASES[name]
    got = _capi.fg_knn(s, v, q, k=k, max_dist=md, device=-1, details=True)
    cases.assert_equals_spec(got, cases.expected(name))
    plain = _capi.fg_knn(s, v, q, k=k, max_dist=md, device=-1)           # (count and index not asked for: the same values)
    assert spec.same_bits(plain, got[0])


def test_the_cases_hold_what_they_are_named_for():
    """Asserted from the specification's own answer: ties on the lattice, the counts the limits leave, a candidate exactly ON
    the limit, empty results where nothing is usable."""
    for name in ('lattice', 'limit_m0', 'limit_m1_on', 'limit_m2_tie_on', 'limit_m4_on', 'non_finite', 'seven_k16'):
        s, v, q, k, md = cases.CASES[name]                                 # (what is asserted below holds for the library's answer)
        cases.assert_equals_spec(_capi.fg_knn(s, v, q, k=k, max_dist=md, device=-1, details=True), cases.expected(name))
    _, cnt, idx, d2 = cases.expected('lattice')
    assert (cnt == 5).all()
    # a tie between the last neighbour and a seed that did not make it: the index decides who is in
    s, v, q, k, md = cases.CASES['lattice']
    all_d2 = ((q[:, None, :] - s[None, :, :]) ** 2).sum(axis=2)
    assert ((all_d2 == d2[:, 4:5]).sum(axis=1) > (d2 == d2[:, 4:5]).sum(axis=1)).mean() > 0.3
    assert (np.diff(d2, axis=1) == 0).any(axis=1).mean() > 0.9            # ties inside the list: nearly every query
    assert cases.expected('limit_m0')[1][0] == 0 and cases.expected('limit_m0')[1][2] == 0
    _, cnt, idx, d2 = cases.expected('limit_m1_on')
    assert cnt[0] == 1 and d2[0, 0] == 25.0 and idx[0, 0] == 0            # d2 == m2: admissible
    _, cnt, idx, d2 = cases.expected('limit_m2_tie_on')
    assert cnt[0] == 2 and list(d2[0, :2]) == [25.0, 25.0] and list(idx[0, :2]) == [0, 5]
    _, cnt, idx, d2 = cases.expected('limit_m4_on')
    assert cnt[0] == 4 and d2[0, 3] == 289.0 and idx[0, 4] == -1          # m = k - 1, the last one ON the limit
    out, cnt, idx, _ = cases.expected('non_finite')
    assert not np.isin(idx, [0, 3, 5, 7, 11, 39]).any()                    # the unusable seeds are nobody's neighbour
    assert np.isnan(out[[2, 9, 30]]).all() and (cnt[[2, 9, 30]] == 0).all() and (cnt[[0, 1]] == 5).all()
    for name in ('all_unusable', 'no_seeds'):
        out, cnt, idx, _ = cases.expected(name)
        assert np.isnan(out).all() and (cnt == 0).all() and (idx == -1).all()
    assert (cases.expected('seven_k16')[1][:5] == 7).all()                 # k > n_seeds: all seven
    dup = cases.expected('duplicates_adjacent')
    assert (np.diff(dup[3], axis=1) == 0).any(axis=1).all()


def test_k1_is_the_kd_trees_nearest_seed():
    """k = 1 against cKDTree on the queries whose nearest seed is unique (which of several tied seeds a KD-tree returns is
    not documented): nearly all of them."""
    rng = np.random.default_rng(21)
    s, q = rng.uniform(0, 2000, (1500, 2)), rng.uniform(-100, 2100, (2000, 2))
    v = np.stack([s[:, 0] * 2.0, s[:, 1] - 7.0], axis=1)
    out, cnt, idx = _capi.fg_knn(s, v, q, k=1, device=-1, details=True)
    d2 = spec.knn(s, v, q, 2)[3]
    unique = d2[:, 0] < d2[:, 1]
    assert unique.mean() > 0.99
    _, tree_idx = cKDTree(s).query(q, k=1)
    np.testing.assert_array_equal(idx[unique, 0], tree_idx[unique])
    np.testing.assert_array_equal(out[unique], v[tree_idx[unique]])        # the median of one value is that value
    assert (cnt == 1).all()


def test_argument_errors_without_a_device():
    """Every argument error, from the checks that precede any device call: device 0 is named and none is present here."""
    L = _capi.lib()
    f64, i32 = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    s = np.zeros((4, 2)); v = np.zeros((4, 2)); q = np.zeros((3, 2)); out = np.zeros((3, 2))   # noqa: E702
    P = lambda a: a.ctypes.data_as(f64)                                   # noqa: E731
    inf = float('inf')

    def call(seeds=P(s), ns=4, values=P(v), qq=P(q), nq=3, k=5, md=inf, o=P(out)):
        return L.sid_fg_knn(0, seeds, ns, values, qq, nq, k, md, o, None, None)
    assert call(nq=0) == 0                                                 # nothing to do: OK at once
    assert call(nq=0, seeds=None, values=None, qq=None, o=None, k=99) == 0
    for kw in (dict(seeds=None), dict(values=None), dict(qq=None), dict(o=None), dict(ns=-1), dict(nq=-1),
               dict(k=0), dict(k=17), dict(k=-3), dict(md=float('nan')), dict(md=0.0), dict(md=-1.0), dict(md=-inf),
               dict(values=None, ns=0, seeds=None)):
        assert call(**kw) == -1, kw
        assert L.sid_fg_last_error()
    assert call(ns=2 ** 31) == -4 and call(ns=2 ** 40) == -4              # 32-bit seed indices
    assert call(ns=2 ** 31, k=0) == -1                                     # (argument errors first)
    with pytest.raises(_capi.SidPmError) as e:
        _capi.fg_knn(s, v, q, k=17, device=0)
    assert e.value.code == -1 and '1..16' in str(e.value)
    with pytest.raises(_capi.SidPmError) as e:
        _capi.fg_knn(s, v, q, max_dist=0.0, device=0)
    assert e.value.code == -1
    with pytest.raises(ValueError):
        _capi.fg_knn(s, v[:3], q, device=-1)
    assert _capi.fg_knn(s, v, np.empty((0, 2)), device=0).shape == (0, 2)  # n_q = 0 needs no device either
    assert 'sid_fg_knn' in _capi.FG_SYMBOLS


def test_interpolation_near_knn_on_the_host():
    """method='knn' through lib.interpolation_near: the (row, col) point order of the reference's function, the grid's shape,
    knn_k / knn_max_dist, NaN where the limit leaves nobody, ValueError for values that are not finite; the other methods
    are SciPy's as before."""
    rng = np.random.default_rng(22)
    x1, y1 = rng.uniform(0, 400, 250), rng.uniform(0, 300, 250)
    x2, y2 = x1 + rng.normal(5, 1, 250), y1 + rng.normal(-3, 1, 250)
    xg, yg = np.meshgrid(np.linspace(-50, 450, 23), np.linspace(10, 290, 17))
    for k, md in ((5, None), (3, 30.0), (1, None)):
        gx, gy = lib.interpolation_near(x1, y1, x2, y2, xg, yg, method='knn', knn_k=k, knn_max_dist=md, knn_displacement=False)
        assert gx.shape == xg.shape and gy.shape == xg.shape
        exp = spec.knn(np.stack([y1, x1], axis=1), np.stack([x2, y2], axis=1), np.stack([yg.ravel(), xg.ravel()], axis=1), k, md)[0]
        assert spec.same_bits(gx.ravel(), exp[:, 0]) and spec.same_bits(gy.ravel(), exp[:, 1])
        assert np.isnan(gx).any() == (md is not None)
        # the default: x2, y2 are positions - grid point + the median of the neighbours' displacements
        gx, gy = lib.interpolation_near(x1, y1, x2, y2, xg, yg, method='knn', knn_k=k, knn_max_dist=md)
        exp = spec.knn(np.stack([y1, x1], axis=1), np.stack([x2 - x1, y2 - y1], axis=1), np.stack([yg.ravel(), xg.ravel()], axis=1), k, md)[0]
        assert spec.same_bits(gx.ravel(), xg.ravel() + exp[:, 0]) and spec.same_bits(gy.ravel(), yg.ravel() + exp[:, 1])
    fx, fy = lib.interpolation_near(x1, y1, x2, y2, xg.ravel(), yg.ravel(), method='knn')       # flat grids, the prelude's form
    gx, gy = lib.interpolation_near(x1, y1, x2, y2, xg, yg, method='knn')
    assert spec.same_bits(fx, gx.ravel()) and spec.same_bits(fy, gy.ravel())
    bad = x2.copy()
    bad[17] = np.nan
    with pytest.raises(ValueError):
        lib.interpolation_near(x1, y1, bad, y2, xg, yg, method='knn')
    with pytest.raises(_capi.SidPmError):
        lib.interpolation_near(x1, y1, x2, y2, xg, yg, method='knn', knn_k=17)
    from scipy.interpolate import griddata
    src, dst = np.array([y1, x1]).T, np.array([yg, xg]).T
    for method in ('linear', 'nearest'):
        gx, gy = lib.interpolation_near(x1, y1, x2, y2, xg, yg, method=method)
        assert spec.same_bits(gx, griddata(src, x2, dst, method=method).T)
        assert spec.same_bits(gy, griddata(src, y2, dst, method=method).T)


@pytest.mark.parametrize('seed', [1, 2, 3])
def test_prelude_with_planted_wrong_key_points(seed):
    """2 % of the key points are wrong matches, 60 to 150 px off.  With method='knn' the first guess of every grid point stays
    within 17 px of the true position (both components together: the Euclidean distance) - inside a min_border = 20 window -
    and with method='linear', on the same inputs, at least one grid point is more than 17 px off in one component alone.
    Measured (seeds 1, 2, 3): knn largest distance 5.5, 5.5, 6.0 px; linear 63, 56, 76 grid points out, the worst 105 - 125 px."""
    sc = cases.prelude_scenario(seed)
    knn = cases.run_prelude(sc, method='knn', first_guess_on='host')
    ec, er = cases.prelude_error(knn)
    print('seed %d knn: largest distance %.2f px' % (seed, np.hypot(ec, er).max()))
    lin = cases.run_prelude(sc, method='linear', first_guess_on='host')
    lc, lr = cases.prelude_error(lin)
    print('seed %d linear: %d grid points out, largest %.1f px' % (seed, (np.maximum(lc, lr) > cases.BOUND).sum(), np.maximum(lc, lr).max()))
    assert (np.hypot(ec, er) <= cases.BOUND).all()
    assert (np.maximum(lc, lr) > cases.BOUND).any()
    assert knn['gpi'].all() and (knn['brd2'] >= 20).all()


def test_knn_prelude_never_triangulates(monkeypatch):
    """With method='knn' neither lib._triangulation nor scipy.spatial.Delaunay is reached - old_border True and False, a
    limit that sends grid points to the polynomial fallback included."""
    import scipy.spatial

    def boom(*a, **k):
        raise AssertionError('a triangulation was asked for')
    sc = cases.prelude_scenario(4, n_kp=400)
    ref = {ob: cases.run_prelude(sc, method='knn', first_guess_on='host', old_border=ob) for ob in (True, False)}
    monkeypatch.setattr(lib, '_triangulation', boom)
    monkeypatch.setattr(scipy.spatial, 'Delaunay', boom)
    monkeypatch.setattr(lib, 'griddata', boom)
    for ob in (True, False):
        pre = cases.run_prelude(sc, method='knn', first_guess_on='host', old_border=ob)
        for key in ('c2fg', 'r2fg', 'brd2', 'gpi'):
            np.testing.assert_array_equal(pre[key], ref[ob][key])
        assert np.isfinite(pre['c2fg']).all() and (pre['brd2'] >= 20).all() and (pre['brd2'] <= 50).all()
        assert (pre['brd2'] < 50).any()
    # a limit of 40 px leaves grid points without a key point: polynomial first guess, max_border
    lim = cases.run_prelude(sc, method='knn', knn_max_dist=40.0, first_guess_on='host')
    poly = np.round(lib.interpolation_poly(sc['c1'], sc['r1'], sc['c2'], sc['r2'], lim['c2pm1i'], lim['r2pm1i']))
    raw = lib.interpolation_near(sc['c1'], sc['r1'], sc['c2'], sc['r2'], lim['c2pm1i'], lim['r2pm1i'], method='knn', knn_max_dist=40.0)
    gone = np.isnan(raw[0])
    assert gone.any() and not gone.all()
    np.testing.assert_array_equal(lim['c2fg'][gone], poly[0][gone])
    np.testing.assert_array_equal(lim['r2fg'][gone], poly[1][gone])
    assert (lim['brd2'][gone] == 50).all()
    np.testing.assert_array_equal(lim['c2fg'][~gone], np.round(raw[0][~gone]))
    with pytest.raises(AssertionError):                                    # (the guard itself: 'linear' does triangulate)
        cases.run_prelude(sc, method='linear', first_guess_on='host')


def test_seaicedrift_first_guess_method(monkeypatch):
    """SeaIceDrift(first_guess_method='knn'): get_drift_FT starts no triangulation ahead of get_drift_PM (without it, it
    does), and get_drift_PM's default method is the constructor's unless the call names one.  Tracking and matching are
    stubbed: they need a GPU."""
    from sea_ice_drift_amd import seaicedrift as sd
    sc = cases.prelude_scenario(5, n_kp=50)
    monkeypatch.setattr(sd, 'feature_tracking', lambda n1, n2, **kw: (sc['c1'], sc['r1'], sc['c2'], sc['r2']))
    monkeypatch.delenv('SID_NO_TRI_PREFETCH', raising=False)
    seen = []
    monkeypatch.setattr(sd, 'pattern_matching', lambda *a, **kw: seen.append(kw.get('method', 'absent')))
    lib._TRI_CACHE.clear()
    s = SeaIceDrift(sc['n1'], sc['n2'], first_guess_method='knn')
    out = s.get_drift_FT()
    assert len(out) == 6 and not lib._TRI_CACHE
    s.get_drift_PM(sc['lon'], sc['lat'], out[2], out[3], out[4], out[5])
    s.get_drift_PM(sc['lon'], sc['lat'], out[2], out[3], out[4], out[5], method='linear')
    plain = SeaIceDrift(sc['n1'], sc['n2'])
    out = plain.get_drift_FT()
    assert len(lib._TRI_CACHE) == 1                                        # (the guard: the default does prefetch)
    for t, _ in list(lib._TRI_CACHE.values()):
        t.join()
    lib._TRI_CACHE.clear()
    plain.get_drift_PM(sc['lon'], sc['lat'], out[2], out[3], out[4], out[5])
    assert seen == ['knn', 'linear', 'absent']


def test_default_prelude_still_reproduces_fixture_g4():
    """Nothing changes for a call that names no method: fixture G4's kernel inputs (the reference's own prelude) on the host
    route, with and without the new keywords' defaults spelled out."""
    from tests.golden import make_golden as mg
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'g4_pattern_matching.npz'))
    n1, n2, c1, r1, c2, r2, lon_g, lat_g = mg.g4_inputs()
    for extra in ({}, dict(method='linear', knn_k=5, knn_max_dist=None)):
        pre = my.pm_prelude(lon_g, lat_g, n1, c1, r1, n2, c2, r2, img_size=34, angles=list(range(-3, 4)), first_guess_on='host', **extra)
        np.testing.assert_array_equal(pre['c2fg'], g['fg_c2'])
        np.testing.assert_array_equal(pre['r2fg'], g['fg_r2'])
        np.testing.assert_array_equal(pre['brd2'], g['fg_border'])
    knn = my.pm_prelude(lon_g, lat_g, n1, c1, r1, n2, c2, r2, img_size=34, angles=list(range(-3, 4)), first_guess_on='host', method='knn')
    assert not np.array_equal(knn['c2fg'], g['fg_c2'])                    # (another method: other numbers)
