"""The guided matcher without a device: the specification (tests/ft_guided_spec.py) against the brute-force oracle and on the
boundary of the inclusion rule, the argument errors of the binding and of the C entry points (before any device call),
ftlib.drift_limit_pixels, the plan the library reports, and the distractor construction of the end-to-end GPU test evaluated
with the specification alone."""
import ctypes
import datetime

import numpy as np
import pytest

from oracle import ft_oracle as fo
from sea_ice_drift_amd import _capi, ftlib
from sea_ice_drift_amd.domain import ArrayNansat
from tests import ft_guided_cases as gc
from tests import ft_guided_spec as gs


def test_spec_with_an_all_covering_radius_is_the_brute_force_oracle():
    rng = np.random.default_rng(1)
    for n1, n2 in ((1, 1), (1, 2), (5, 0), (257, 255), (300, 400)):
        d2 = gc.descriptors(rng, n2)
        d1 = gc.descriptors(rng, n1, like=d2)
        if n2 > 20:
            d2[17] = d2[5]; d1[0] = d2[5]                                       # ties: the smaller index first
        q, t = gc.frame_points(rng, n1), gc.frame_points(rng, n2)
        idx, dist, count = gs.knn2(d1, q[:, 0], q[:, 1], d2, t[:, 0], t[:, 1], 1e9)
        eidx, edist = fo.knn2(d1, d2)
        np.testing.assert_array_equal(idx, eidx)
        np.testing.assert_array_equal(dist, edist)
        np.testing.assert_array_equal(count, np.full(n1, n2))


def test_spec_inclusion_rule_on_pythagorean_offsets_and_positions_that_are_not_finite():
    d = np.zeros((1, 32), dtype=np.uint8)
    for ox, oy in ((3.0, 4.0), (-3.0, 4.0), (4.0, -3.0), (5.0, 0.0), (0.0, -5.0)):
        for base in (0.0, 1000.0, -1e7):
            args = (d, [base], [base], d, [base + ox], [base + oy])
            assert gs.knn2(*args, 5.0)[2][0] == 1, (ox, oy, base)               # 9 + 16 <= 25: inside
            assert gs.knn2(*args, np.nextafter(5.0, 0.0))[2][0] == 0, (ox, oy, base)
    assert gs.knn2(d, [2.0], [2.0], d, [2.0], [2.0], 0.0)[2][0] == 1            # radius 0: the same position only
    assert gs.knn2(d, [2.0], [2.0], d, [np.nextafter(2.0, 3.0)], [2.0], 0.0)[2][0] == 0
    for bad in (np.nan, np.inf, -np.inf):
        assert gs.knn2(d, [bad], [0.0], d, [0.0], [0.0], 1e300)[2][0] == 0      # (1e300 squared is inf: every finite pair is inside)
        assert gs.knn2(d, [0.0], [0.0], d, [0.0], [bad], 1e300)[2][0] == 0
    assert gs.knn2(d, [0.0], [0.0], d, [1e200], [-1e200], 1e300)[2][0] == 1
    for bad in (np.nan, np.inf, -1.0, -np.inf):
        with pytest.raises(ValueError):
            gs.knn2(d, [0.0], [0.0], d, [0.0], [0.0], bad)


def test_binding_rejects_bad_arguments_before_any_device_call():
    """On a machine without a device every call that got past the checks would fail with SID_PM_ERR_NODEVICE, not these."""
    d1, d2 = np.zeros((3, 32), dtype=np.uint8), np.zeros((4, 32), dtype=np.uint8)
    q, t = np.zeros((3, 2)), np.zeros((4, 2))
    for bad in (np.nan, np.inf, -np.inf, -1.0, -1e-300):
        with pytest.raises(ValueError, match='radius'):
            _capi.ftg_knn2(d1, q, d2, t, bad)
        with pytest.raises(ValueError, match='radius'):
            _capi.ftg_knn2_device(256, 256, 256, 3, 256, 256, 256, 4, bad, 256, 256, 0, 256)
    with pytest.raises(ValueError, match='positions'):
        _capi.ftg_knn2(d1, t, d2, t, 5.0)                                       # four positions for three queries
    with pytest.raises(ValueError, match='positions'):
        _capi.ftg_knn2(d1, q, d2, t[:, 0], 5.0)
    with pytest.raises(ValueError, match='positions'):
        _capi.ftg_knn2(d1, q, d2, np.zeros((4, 3)), 5.0)
    with pytest.raises(TypeError, match='descriptors'):
        _capi.ftg_knn2(d1.astype(np.int32), q, d2, t, 5.0)
    with pytest.raises(TypeError, match='descriptors'):
        _capi.ftg_knn2(np.zeros((3, 16), dtype=np.uint8), q, d2, t, 5.0)
    with pytest.raises(TypeError, match='descriptors'):
        _capi.ftg_knn2(d1, q, d2.reshape(-1), t, 5.0)
    idx, dist, count = _capi.ftg_knn2(d1[:0], q[:0], d2, t, 5.0)                # no query: nothing to do, no device needed
    assert idx.shape == (0, 2) and dist.shape == (0, 2) and count.shape == (0,)
    assert _capi.ftg_knn2(d1[:0], q[:0], d2, t, 5.0, want_count=False)[2] is None


def test_ftlib_rejects_bad_guided_arguments_before_any_device_call():
    kp1, kp2 = np.zeros((3, 2)), np.zeros((4, 2))
    d1, d2 = np.zeros((3, 32), dtype=np.uint8), np.zeros((4, 32), dtype=np.uint8)
    with pytest.raises(ValueError, match='predicted'):
        ftlib.match(kp1, d1, kp2, d2, search_radius=10.0)                       # predicted missing
    with pytest.raises(ValueError, match='predicted'):
        ftlib.get_match_coords(kp1, d1, kp2, d2, search_radius=10.0)
    with pytest.raises(ValueError, match='predicted'):
        ftlib.match(kp1, d1, kp2, d2, search_radius=10.0, predicted=np.zeros((4, 2)))
    with pytest.raises(ValueError, match='radius'):
        ftlib.match(kp1, d1, kp2, d2, search_radius=np.nan, predicted=kp1)
    with pytest.raises(ValueError, match='radius'):
        ftlib.get_match_coords(kp1, d1, kp2, d2, search_radius=-2.0, predicted=kp1)
    for kw in (dict(predicted=kp1), dict(cross_check=True), dict(accept_lone=True)):
        with pytest.raises(ValueError, match='search_radius'):
            ftlib.match(kp1, d1, kp2, d2, **kw)
    with pytest.raises(NotImplementedError):
        ftlib.get_match_coords(kp1, d1, kp2, d2, matcher='flann', search_radius=10.0, predicted=kp1)


def test_c_entry_points_reject_bad_arguments_before_any_device_call():
    lib = _capi.lib()
    assert sorted(_capi.FTG_SYMBOLS) == sorted(n for n in _capi.FTG_SYMBOLS if hasattr(lib, n))
    d = np.zeros((4, 32), dtype=np.uint8)
    p = np.zeros(4)
    out = np.zeros((4, 2), dtype=np.int32)
    vp = _capi._vp
    host = lambda n1, n2, r, d1=d, qx=p, idx=out: lib.sid_ftg_knn2(0, vp(d1), vp(qx), vp(p), n1, vp(d), vp(p), vp(p), n2, r, vp(idx), vp(out), None)
    dev = lambda n1, n2, r, ws=256: lib.sid_ftg_knn2_device(vp(256), vp(256), vp(256), n1, vp(256), vp(256), vp(256), n2, r, vp(256), vp(256), None, vp(ws), None)
    for call in (host, dev):
        for bad in (float('nan'), float('inf'), -float('inf'), -1.0):
            assert call(4, 4, bad) == -1
            assert b'radius' in lib.sid_ftg_last_error()
        assert call(4, 1 << 22, 5.0) == -1 and b'train' in lib.sid_ftg_last_error()
        assert call(-1, 4, 5.0) == -1 and call(4, -1, 5.0) == -1
        assert call(0, 4, 5.0) == 0                                             # nothing to do
        assert call(0, 0, 0.0) == 0
    assert host(4, 4, 5.0, d1=None) == -1 and b'null pointer' in lib.sid_ftg_last_error()
    assert host(4, 4, 5.0, qx=None) == -1 and host(4, 4, 5.0, idx=None) == -1
    assert lib.sid_ftg_knn2(0, vp(d), vp(p), vp(p), 4, None, vp(p), vp(p), 4, 5.0, vp(out), vp(out), None) == -1
    assert dev(4, 4, 5.0, ws=0) == -1 and b'null pointer' in lib.sid_ftg_last_error()
    assert dev(4, 4, 5.0, ws=264) == -1 and b'aligned' in lib.sid_ftg_last_error()
    assert lib.sid_ftg_debug_plan(4, 4, 0.0, 1.0, 0.0, 1.0, 5.0, None) == -1
    assert lib.sid_ftg_release(-1) == 0                                         # nothing cached, no device: no HIP call
    assert lib.sid_ftg_workspace_bytes(1, 1 << 22) == 0 and lib.sid_ftg_workspace_bytes(-1, 4) == 0
    assert lib.sid_ftg_workspace_bytes(1000, 1300) >= 1300 * (32 + 8 + 8 + 4)


def test_debug_plan_reports_the_plan_header():
    p = _capi.ftg_debug_plan(1000, 1300, (0.0, 400.0, 0.0, 300.0), 60.0)
    assert p['axis_cap'] == 37 and p['x0'] == 0.0 and p['y0'] == 0.0
    assert p['cell_x'] == 60.0 * (1.0 + 2.0 ** -20) and p['cell_y'] == p['cell_x']
    assert (p['nx'], p['ny']) == (7, 5)                                         # floor(400 / 60.00006) + 1, floor(300 / 60.00006) + 1
    assert p['max_items'] == 1000 // 256 + 1000 + 1
    assert p['workspace_bytes'] == _capi.ftg_workspace_bytes(1000, 1300)
    p = _capi.ftg_debug_plan(10, 100000, (-5e5, 5e5, 7.0, 7.0), 0.5)            # radius 0.5 on an extent of 1e6: the cap; one row
    assert p['axis_cap'] == 317 and (p['nx'], p['ny']) == (317, 1) and p['cell_x'] == 1e6 / 317
    p = _capi.ftg_debug_plan(10, 3 << 20, (-5e5, 5e5, 0.0, 1e6), 0.5)
    assert p['axis_cap'] == 1024 and (p['nx'], p['ny']) == (1024, 1024)
    p = _capi.ftg_debug_plan(10, 10, (np.inf, -np.inf, np.inf, -np.inf), 2.0)    # no finite train position
    assert (p['nx'], p['ny']) == (1, 1)
    with pytest.raises(_capi.SidPmError):
        _capi.ftg_debug_plan(10, 10, (0.0, 1.0, 0.0, 1.0), -1.0)


class _Timed(ArrayNansat):
    def __init__(self, image, when, **kw):
        ArrayNansat.__init__(self, image, **kw)
        self.time_coverage_start = when


def test_drift_limit_pixels_on_a_known_scale():
    """0.001 degrees per pixel both ways, 100 rows from the equator southwards: a row step is R * radians(0.001) =
    111.19 m everywhere, a column step that times cos(latitude) - smallest at the lower corners, 0.1 degrees south."""
    image = np.ones((100, 100), dtype=np.uint8)
    geo = dict(origin=(20.0, 0.0), matrix=((0.001, 0.0), (0.0, -0.001)))
    n1, n2 = ArrayNansat(image, **geo), ArrayNansat(image, **geo)
    step = 6371000.0 * np.radians(0.001)
    smallest = step * np.cos(np.radians(0.1))
    assert step - smallest < 1e-3 and 111.19 < smallest < 111.20
    assert ftlib.drift_limit_pixels(n1, n2, max_drift=5000.0) == int(np.ceil(1.05 * 5000.0 / smallest)) == 48
    assert ftlib.drift_limit_pixels(n1, n2, max_speed=9.0, max_drift=1000.0) == 10          # (no time stamps: max_speed is not used)
    with pytest.raises(ValueError):
        ftlib.drift_limit_pixels(n1, n2)                                        # as mask_drift_limit: no time stamp, no max_drift
    t0 = datetime.datetime(2026, 3, 1)
    a, b = _Timed(image, t0, **geo), _Timed(image, t0 + datetime.timedelta(days=1), **geo)
    assert ftlib.drift_limit_pixels(a, b) == int(np.ceil(1.05 * 0.5 * 86400.0 / smallest)) == 408
    assert ftlib.drift_limit_pixels(b, a, max_speed=0.25, max_drift=1.0) == 204   # time stamps win; the order does not matter
    # twice the pixel size along the rows: the columns still set the scale
    n3 = ArrayNansat(image, origin=(20.0, 0.0), matrix=((0.001, 0.0), (0.0, -0.002)))
    assert ftlib.drift_limit_pixels(n1, n3, max_drift=5000.0) == 48


def _pairs(idx, keep):
    q = np.flatnonzero(keep)
    return set(zip(q.tolist(), idx[q, 0].tolist()))


def test_distractor_scene_global_route_keeps_no_planted_pair_and_the_guided_route_keeps_all():
    """The condition the end-to-end GPU test rests on, with the specification alone."""
    s = gc.scene()
    planted = set(zip(range(gc.PLANTED), s.true_of.tolist()))
    eidx, edist = fo.knn2(s.d1, s.d2)
    globally = _pairs(eidx, ftlib.mask_lowe_ratio(edist, 0.7))
    assert not globally & planted
    assert all(edist[i, 0] == 10 and edist[i, 1] == 12 and eidx[i, 0] == i and eidx[i, 1] == 2 * gc.PLANTED + i for i in range(gc.PLANTED))
    idx, dist, count = gs.knn2(s.d1, s.pred[:, 0], s.pred[:, 1], s.d2, s.xy2[:, 0], s.xy2[:, 1], gc.RADIUS)
    guided = _pairs(idx, gs.lowe_keep(dist, count, 0.7))
    assert planted <= guided
    assert (count[:gc.PLANTED] >= 2).all() and (dist[:gc.PLANTED, 0] == 10).all()
    # every distractor is outside the disc of every planted query, up to a radius of 25
    far = gs.candidates(s.pred[:gc.PLANTED, 0], s.pred[:gc.PLANTED, 1], s.xy2[2 * gc.PLANTED:3 * gc.PLANTED, 0], s.xy2[2 * gc.PLANTED:3 * gc.PLANTED, 1], 25.0)
    assert not far.any()
    # the lone query has one candidate, the other none
    assert count[s.lone] == 1 and idx[s.lone, 0] == s.lone_train and count[s.nobody] == 0
    assert (s.lone, s.lone_train) not in guided
    with_lone = _pairs(idx, gs.lowe_keep(dist, count, 0.7, accept_lone=True))
    ones = np.flatnonzero(count == 1)                                           # (background queries with one candidate too)
    assert with_lone - guided == set(zip(ones.tolist(), idx[ones, 0].tolist())) and (s.lone, s.lone_train) in with_lone
    assert not any(q == s.nobody for q, _ in with_lone)
    # the one-sided pair: forward both query 0 and its rival reach train 0; backwards train 0 prefers the rival
    assert (0, 0) in guided and (s.rival, 0) in guided
    bidx, bdist, bcount = gs.knn2(s.d2, s.xy2[:, 0], s.xy2[:, 1], s.d1, s.pred[:, 0], s.pred[:, 1], gc.RADIUS)
    back = _pairs(bidx, gs.lowe_keep(bdist, bcount, 0.7))
    mutual = {(i, j) for i, j in guided if (j, i) in back}
    assert guided - mutual == {(0, 0)}
    assert planted - mutual == {(0, 0)} and (s.rival, 0) in mutual
