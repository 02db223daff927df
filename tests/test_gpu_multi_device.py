"""``devices=``: one pattern_matching / pm_dispatch call sharded over several device handles in this process.

A one-GPU machine exercises the sharding with a repeated index (``[0, 0]`` is two handles on GPU 0).  Every comparison with
the one-handle call is bit for bit in all five columns: the kernels are the same, and the result of a point does not
depend on which other points share its call (tests/test_gpu_configs.py, test_full_size_properties_order_subset_and_translation)."""
import os
import threading

import numpy as np
import pytest

from sea_ice_drift_amd import _capi, ftlib, pmlib as my, synthetic as syn
from sea_ice_drift_amd.domain import ArrayNansat
from sea_ice_drift_amd.seaicedrift import SeaIceDrift
from tests.golden import make_golden as mg

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
NAMES = ('c1', 'r1', 'c2fg', 'r2fg', 'border')
CASES = [(34, [-3, 0, 3]), (35, [-3, 0, 3]), (34, list(range(-3, 4))), (35, list(range(-3, 4)))]


@pytest.fixture(scope='module')
def scene():
    """700x700 pair, the 144 points of a 12x12 grid with mixed borders 20..50 (grid lines every 45 px, the first at 100)
    and three more: the template of point 144 covers a zeroed block of image 1 that no grid point's template reaches (NaN
    row), point 145 has border 112 (large-window class), the window of point 146 is clipped by the bottom edge of image 2.
    ``ref`` holds the one-handle results of every (template side, angles) case, computed once."""
    img1, img2 = syn.make_pair(700, 700)
    img1 = img1.copy()
    img1[347:352, 347:352] = 0                                     # between the grid lines at 327 and 372
    g = syn.make_grid(700, 700, 12)
    assert g['border'].size == 144 and g['border'].min() >= 20 and g['border'].max() <= 50
    extra = dict(c1=[349.0, 350.0, 300.0], r1=[349.0, 300.0, 600.0], c2fg=[349.0, 350.0, 300.0], r2fg=[349.0, 300.0, 670.0],
                 border=[20.0, 112.0, 20.0])
    v = [np.concatenate([g[k], extra[k]]) for k in NAMES]
    ref = {}
    for k, (s, angles) in enumerate(CASES):
        ref[k] = my.pm_dispatch(img1, img2, *v, s, 0.0, angles=angles, devices=None)
        nan = np.isnan(ref[k][:, 0])
        assert nan[144] and not nan[145] and (~nan[:144]).sum() > 100
    return img1, img2, v, ref


@pytest.mark.parametrize('case', range(len(CASES)))
@pytest.mark.parametrize('devices', [[0, 0], [0, 0, 0], [0] * 8], ids=['2', '3', '8'])
def test_sharded_dispatch_equals_the_one_handle_call_bit_for_bit(scene, devices, case):
    img1, img2, v, ref = scene
    s, angles = CASES[case]
    got = my.pm_dispatch(img1, img2, *v, s, 0.0, angles=angles, devices=devices)
    assert got.shape == (147, 5) and got.dtype == np.float64
    np.testing.assert_array_equal(got, ref[case])                  # (NaNs compare equal)


def test_sharding_is_real(scene):
    img1, img2, v, ref = scene
    s, angles = CASES[0]
    my.pm_dispatch(img1, img2, *v, s, 0.0, angles=angles, devices=None)
    valid = my._shared_context(0)[0].work_info()['valid_points']
    assert 0 < valid <= 147
    timings = {}
    my.pm_dispatch(img1, img2, *v, s, 0.0, angles=angles, devices=[0, 0, 0], timings=timings)
    assert {(0, 0), (0, 1), (0, 2)} <= set(my.resident_handles())
    per_handle = [my._shared_context(0, k)[0].work_info()['valid_points'] for k in range(3)]
    assert sum(per_handle) == valid
    assert sum(p > 0 for p in per_handle) >= 2
    assert sum(timings['points_per_handle']) == 147 and len(timings['points_per_handle']) == 3
    # the same three handles, and the same object for replica 0 as the one-handle call uses
    assert my._shared_context(0)[0] is my._shared_context(0, 0)[0]
    assert len({id(my._shared_context(0, k)[0]) for k in range(3)}) == 3


def test_fewer_points_than_handles_and_no_points(scene):
    img1, img2, v, ref = scene
    s, angles = CASES[2]
    sel = np.array([7, 145, 144])
    got = my.pm_dispatch(img1, img2, *[x[sel] for x in v], s, 0.0, angles=angles, devices=[0] * 8)
    np.testing.assert_array_equal(got, ref[2][sel])
    none = np.zeros(0)
    got = my.pm_dispatch(img1, img2, none, none, none, none, none, s, 0.0, angles=angles, devices=[0, 0])
    assert got.shape == (0, 5) and got.dtype == np.float64


def test_a_refused_devices_argument_touches_nothing(scene):
    img1, img2, v, ref = scene
    s, angles = CASES[0]
    before = my.resident_handles()
    n = _capi.device_count()
    with pytest.raises(ValueError) as e:
        my.pm_dispatch(img1, img2, *v, s, 0.0, angles=angles, devices=[0, n])
    assert 'devices[1]=%d' % n in str(e.value)
    with pytest.raises(ValueError):
        my.pm_dispatch(img1, img2, *v, s, 0.0, angles=angles, devices=n + 1)
    with _capi.PMContext(0) as ctx, pytest.raises(ValueError):
        my.pm_dispatch(img1, img2, *v, s, 0.0, angles=angles, devices=[0, 0], context=ctx)
    with pytest.raises(NotImplementedError):                       # an unsupported option still comes first
        my.pm_dispatch(img1, img2, *v, s, 0.0, angles=angles, mtype=3, devices=[0, n])
    assert my.resident_handles() == before
    with pytest.raises(NotImplementedError):                       # what set_points refuses (code -4) keeps its type
        my.pm_dispatch(img1, img2, *v, 256, 0.0, angles=angles, devices=[0, 0])
    # devices=[0] and devices=1 are the one-handle call
    np.testing.assert_array_equal(my.pm_dispatch(img1, img2, *v, s, 0.0, angles=angles, devices=[0]), ref[0])
    np.testing.assert_array_equal(my.pm_dispatch(img1, img2, *v, s, 0.0, angles=angles, devices=1), ref[0])
    np.testing.assert_array_equal(my.pm_dispatch(img1, img2, *v, s, 0.0, angles=angles, devices=[0, 0]), ref[0])


def test_g4_pattern_matching_on_two_handles():
    """The public call with ``devices=[0, 0]`` against the reference's output grids (fixture G4), compared as
    tests/test_gpu_golden.py::test_g4_pattern_matching_end_to_end compares the one-handle call; then the class, whose
    ``get_drift_PM`` with a default or a per-call ``devices`` equals the one-handle grids bit for bit."""
    g = np.load(os.path.join(GOLD, 'g4_pattern_matching.npz'))
    n1, n2, c1, r1, c2, r2, lon_g, lat_g = mg.g4_inputs()
    kw = dict(img_size=34, angles=list(range(-3, 4)))
    out = my.pattern_matching(lon_g, lat_g, n1, c1, r1, n2, c2, r2, threads=5, devices=[0, 0], **kw)
    assert len(out) == 7
    for name, arr in zip(('u', 'v', 'a', 'r', 'lon2', 'lat2'), (out[0], out[1], out[2], out[3], out[5], out[6])):
        np.testing.assert_array_equal(arr, g[name], err_msg=name)
    np.testing.assert_allclose(out[4], g['h'], rtol=1e-5, atol=1e-5, equal_nan=True)
    one = my.pattern_matching(lon_g, lat_g, n1, c1, r1, n2, c2, r2, **kw)
    lon1, lat1 = n1.transform_points(c1, r1)
    lon2, lat2 = n2.transform_points(c2, r2)
    single = SeaIceDrift(n1, n2).get_drift_PM(lon_g, lat_g, lon1, lat1, lon2, lat2, **kw)
    by_default = SeaIceDrift(n1, n2, devices=[0, 0]).get_drift_PM(lon_g, lat_g, lon1, lat1, lon2, lat2, **kw)
    per_call = SeaIceDrift(n1, n2, devices=[0]).get_drift_PM(lon_g, lat_g, lon1, lat1, lon2, lat2, devices=[0, 0, 0], **kw)
    for k in range(7):
        np.testing.assert_array_equal(out[k], one[k])
        np.testing.assert_array_equal(by_default[k], single[k])
        np.testing.assert_array_equal(per_call[k], single[k])
    with pytest.raises(ValueError):
        my.pattern_matching(lon_g, lat_g, n1, c1, r1, n2, c2, r2, devices=[], **kw)
    with pytest.raises(NotImplementedError):
        my.pattern_matching(lon_g, lat_g, n1, c1, r1, n2, c2, r2, devices=[], mtype=1, **kw)


def test_class_with_devices_on_g7_inputs():
    """``SeaIceDrift(n1, n2, devices=[0, 0])`` on fixture G7's inputs: ``get_drift_FT`` (G7's key points through
    ``find_key_points=``, the matcher on the GPU) and ``get_drift_PM`` from its vectors equal the one-handle results bit for
    bit."""
    kw = dict(max_drift=25000.0, domainMargin=10, ratio_test=0.75, psi=150)

    def run(**cls_kw):
        n1, n2, xy1, d1, xy2, d2 = mg.g7_inputs(False)
        feeds = [(xy1, d1), (xy2, d2)]
        sid = SeaIceDrift(n1, n2, **cls_kw)
        ft = sid.get_drift_FT(find_key_points=lambda image, **k: feeds.pop(0), **kw)
        lon_g, lat_g = np.meshgrid(np.linspace(10.3, 10.9, 6), np.linspace(77.2, 77.8, 5))
        pm = sid.get_drift_PM(lon_g, lat_g, ft[2], ft[3], ft[4], ft[5], img_size=34)
        return ft, pm
    ft1, pm1 = run()
    ft2, pm2 = run(devices=[0, 0])
    assert len(ft1[0]) > 2000
    for a, b in zip(ft1, ft2):
        np.testing.assert_array_equal(a, b)
    assert pm1[0].shape == (5, 6)
    for a, b in zip(pm1, pm2):
        np.testing.assert_array_equal(a, b)


def test_feature_tracking_with_the_gpu_detector_on_two_devices():
    """The package's own detector: with ``devices=[0, 0]`` the two images are detected on two threads with their device
    named per image; the matched vectors are those of the call without ``devices``."""
    img1, img2 = syn.make_pair(1000, 1000, seed=55, speckle=0.03)
    m = ((1e-4, 0.0), (0.0, 1e-4))
    n1, n2 = ArrayNansat(img1, matrix=m), ArrayNansat(img2, matrix=m)
    kw = dict(nFeatures=8000, max_drift=1e9, ratio_test=0.75)
    ref = ftlib.feature_tracking(n1, n2, **kw)
    got = ftlib.feature_tracking(n1, n2, devices=[0, 0], **kw)
    print('matched vectors: %d' % len(ref[0]))
    assert len(ref[0]) > 0
    for a, b in zip(got, ref):
        np.testing.assert_array_equal(a, b)


def test_two_threads_each_on_two_handles(scene):
    """Two concurrent calls that want the same two handles, three times each: the locks are taken in sorted key order, so
    the calls queue up instead of holding one handle each, and each returns the rows of its own points."""
    img1, img2, v, ref = scene
    sets = [np.arange(0, 147, 2), np.arange(1, 147, 3)]
    cases = [0, 3]
    got, errors = [None, None], []
    start = threading.Barrier(2, timeout=60)

    def worker(k):
        try:
            s, angles = CASES[cases[k]]
            start.wait()
            for _ in range(3):
                got[k] = my.pm_dispatch(img1, img2, *[x[sets[k]] for x in v], s, 0.0, angles=angles, devices=[0, 0])
        except BaseException as e:                                 # noqa: reported by the main thread
            errors.append((k, e))
    threads = [threading.Thread(target=worker, args=(k,), daemon=True) for k in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout=120)
    assert not any(t.is_alive() for t in threads), 'deadlock: a pm_dispatch(devices=[0, 0]) did not return'
    assert not errors, errors
    for k in range(2):
        np.testing.assert_array_equal(got[k], ref[cases[k]][sets[k]])


def test_release_contexts_closes_every_replica(scene):
    img1, img2, v, ref = scene
    s, angles = CASES[1]
    my.pm_dispatch(img1, img2, *v, s, 0.0, angles=angles, devices=[0, 0, 0])
    assert len(my.resident_handles()) >= 3
    my.release_contexts()
    assert my.resident_handles() == []
    got = my.pm_dispatch(img1, img2, *v, s, 0.0, angles=angles, devices=[0, 0])
    np.testing.assert_array_equal(got, ref[1])
    assert my.resident_handles() == [(0, 0), (0, 1)]
