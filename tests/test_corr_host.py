"""CPU tests of include/sid_corr.h (libcorr.local_correlation, libcorr.local_correlation_at): the host instance of the
kernels' source (device = -1) against the specification (tests/corr_spec.py) bit for bit, the specification against
np.corrcoef and the TM_CCOEFF_NORMED oracle, every argument error, the exported symbols, and what the cases claim to cover."""
import ctypes
import os
import re

import numpy as np
import pytest

from oracle import pm_oracle
from sea_ice_drift_amd import _capi, libcorr, synthetic
from tests import corr_cases as cc
from tests import corr_spec as cs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VP = ctypes.c_void_p
ERR_ARG, ERR_UNSUPPORTED = -1, -4          # checked against include/sid_pm.h below


def vp(a):
    return VP(a.ctypes.data) if a is not None else None


def stride_of(img):
    return img.strides[0] if img.shape[0] > 1 and img.shape[1] > 0 else img.shape[1]


def poisoned(shape):
    return (np.full(shape, -12345.678, dtype=np.float64), np.full(shape, -77, dtype=np.int32),
            np.full(tuple(shape) + (5,), -99, dtype=np.int64))


def host_case(c):
    """A case through the C entry point with device = -1, into poisoned outputs -> r, count, sums."""
    a, b, w = c['a'], c['b'], c['window']
    L = _capi.lib()
    dummy = np.zeros(1, dtype=np.uint8)
    pa, pb = (vp(a), vp(b)) if a.size else (vp(dummy), vp(dummy))
    if c['kind'] == 'lattice':
        (sr, sc), (r0, c0), (nr, nc), min_count = cc.resolved(c)
        r, count, sums = poisoned((nr, nc))
        rc = L.sid_corr_lattice(-1, pa, stride_of(a), pb, stride_of(b), a.shape[0], a.shape[1], w, r0, c0, sr, sc, nr, nc, min_count,
                                vp(r), vp(count), vp(sums))
    else:
        shape = c['c'].shape
        cen_c, cen_r = [np.ascontiguousarray(q, dtype=np.int32).ravel() for q in (c['c'], c['r'])]
        valid = np.ascontiguousarray(c['valid'], dtype=np.uint8).ravel() if c['valid'] is not None else None
        r, count, sums = poisoned(shape)
        rc = L.sid_corr_points(-1, pa, stride_of(a), pb, stride_of(b), a.shape[0], a.shape[1], w, vp(cen_c), vp(cen_r), vp(valid),
                               cen_c.size, (w * w + 1) // 2 if c['min_count'] is None else c['min_count'], vp(r), vp(count), vp(sums))
    assert rc == 0, L.sid_corr_last_error()
    return r, count, sums


def through_libcorr(c, **kw):
    if c['kind'] == 'lattice':
        return libcorr.local_correlation(c['a'], c['b'], window=c['window'], step=c['step'], origin=c['origin'], shape=c['shape'],
                                         min_count=c['min_count'], return_count=True, return_sums=True, **kw)
    return libcorr.local_correlation_at(c['a'], c['b'], c['c'], c['r'], window=c['window'], valid=c['valid'], min_count=c['min_count'],
                                        return_count=True, return_sums=True, **kw)


# ---------------------------------------------------------------- host instance against the specification
@pytest.mark.parametrize('name', cc.NAMES)
def test_host_instance_equals_spec(name):
    cc.check(host_case(cc.BY_NAME[name]), name, 'host instance')


@pytest.mark.parametrize('name', cc.NAMES)
def test_python_route_on_the_host_instance(name):
    cc.check(through_libcorr(cc.BY_NAME[name], device=-1), name, 'libcorr, device=-1')


def test_cases_cover_what_they_claim():
    e = cc.expected
    full = 9 * 9
    n = e('origin_outside')['count']
    assert (n == 0).any() and ((n > 0) & (n < full // 2)).any() and (n > full // 2).any()              # empty, clipped, whole
    assert n[0].max() == 0 and n[-1].max() == 0 and n[:, 0].max() == 0 and n[:, -1].max() == 0       # empty on all four sides
    assert all(0 < n[i, j] < 30 for i in (3, 9) for j in (2, 11))                                    # windows clipped at the four corners
    assert np.isfinite(e('origin_outside')['r']).sum() > 50
    assert (e('origin_beyond_last')['count'] == 0).any() and (e('origin_beyond_last')['count'] > 0).any()
    n = e('origin_int64')['count']
    assert n[2, 0] > 0 and n.sum() == n[2, 0]                                                        # the one centre inside
    assert e('empty_image')['count'].shape == (2, 3) and not e('empty_image')['count'].any()
    for name in ('overflow_255', 'overflow_checkerboards'):
        assert e(name)['sums'][..., 2].min() > 2 ** 31 and e(name)['r'].shape == (4, 4)
    assert np.isnan(e('overflow_255')['r']).all() and np.isfinite(e('overflow_checkerboards')['r']).all()
    assert 0 < np.abs(e('overflow_checkerboards')['r']).max() < 1
    m = e('min_count_both_sides')
    assert m['count'][0, 0] == 20 and m['count'][0, 1] == 19 and np.isfinite(m['r'][0, 0]) and np.isnan(m['r'][0, 1])
    assert (m['va'][0, 1] > 0) and (m['vb'][0, 1] > 0)                                                # NaN by the count alone
    w1 = e('window_1')
    assert (w1['count'] == 1).any() and (w1['va'] == 0).all() and np.isnan(w1['r']).all()            # min_count = 1, va = 0
    assert np.array_equal(e('zeros_in_a')['count'], e('zeros_in_b')['count']) and (e('zeros_in_a')['count'] < 81).any()
    assert not e('a_all_zero')['count'].any() and np.isnan(e('a_all_zero')['r']).all()
    assert (e('zero_band')['count'] == 0).any() and np.isfinite(e('zero_band')['r']).any()
    assert e('window_255_small_image')['count'].max() > 1000 and np.isfinite(e('window_255_small_image')['r']).any()
    for name in ('wide_row_255', 'wide_row_gaps'):
        c = cc.BY_NAME[name]
        (sr, sc), _, (nr, nc), _ = cc.resolved(c)
        assert (min(nc, cc.TC) - 1) * min(sc, c['window']) + c['window'] > 2048 and np.isfinite(e(name)['r']).any()
        assert sr < c['window'] <= sc                                                                # (the tiled kernel, not the plain one)
    many = np.isfinite(e('step_larger_many')['r']).ravel()
    assert many.sum() > 900 and not many[:4 * (1 << 14)].any()                                       # all behind the first 65536 nodes
    for d in (-1, 0, 1):
        assert e('tile%+d' % d)['r'].shape == (cc.TR + d, cc.TC + d) and np.isfinite(e('tile%+d' % d)['r']).all()
    assert e('step_1')['r'].shape[0] > 2 * cc.TR and e('step_1')['r'].shape[1] > cc.TC
    ident = e('identical')['r']
    assert np.isfinite(ident).all() and ident.max() <= 1.0 and np.abs(ident - 1.0).max() <= 1e-15
    p = e('points_valid')
    valid = cc.BY_NAME['points_valid']['valid']
    assert (valid == 0).sum() > 5 and not p['count'][valid == 0].any() and not p['sums'][valid == 0].any() and np.isnan(p['r'][valid == 0]).all()
    assert np.isfinite(p['r'][valid != 0]).any()
    q = e('points_anywhere')
    assert cs.same_bits(q['r'][0], q['r'][1]) and not q['count'][2, :4].any() and np.isfinite(q['r']).sum() > 20
    assert e('points_none')['r'].shape == (0,) and np.isfinite(e('points_one')['r']).all()
    assert np.isfinite(e('points_70000')['r']).sum() > 60000
    for name in cc.NAMES:
        r = e(name)['r']
        assert r.dtype == np.float64 and (np.isnan(r) | ((r >= -1.0) & (r <= 1.0))).all()


# ---------------------------------------------------------------- the specification against NumPy and the oracle
SMALL = ['step_larger', 'origin_outside', 'zeros_in_a', 'min_count_both_sides', 'tile+1', 'overflow_checkerboards', 'identical']


@pytest.mark.parametrize('name', SMALL)
def test_spec_against_corrcoef(name):
    """r of every finite node against np.corrcoef on the usable pixels of its window, extracted by slicing: to 1e-12."""
    c, e = cc.BY_NAME[name], cc.expected(name)
    (sr, sc), (r0, c0), (nr, nc), _ = cc.resolved(c)
    worst, seen = 0.0, 0
    for i in range(0, nr):
        for j in range(0, nc):
            if (i * nc + j) % 3 and nr * nc > 200:
                continue
            pa, pb = cs.window_pixels(c['a'], c['b'], c['window'], r0 + i * sr, c0 + j * sc)
            assert len(pa) == e['count'][i, j]
            assert [int(q) for q in e['sums'][i, j]] == [int(pa.astype(np.int64).sum()), int(pb.astype(np.int64).sum()),
                                                          int((pa.astype(np.int64) ** 2).sum()), int((pb.astype(np.int64) ** 2).sum()),
                                                          int((pa.astype(np.int64) * pb).sum())]
            if np.isfinite(e['r'][i, j]):
                ref = np.corrcoef(pa.astype(np.float64), pb.astype(np.float64))[0, 1]
                worst, seen = max(worst, abs(ref - e['r'][i, j])), seen + 1
    print(name, 'max |spec - corrcoef| = %.3e over %d nodes' % (worst, seen))
    assert seen >= 1 and worst <= 1e-12


def test_spec_against_the_template_matching_oracle():
    """On windows without zeros r is the 1 x 1 TM_CCOEFF_NORMED value of window b against window a, which the oracle gives in
    float32: |difference| <= 2^-24, the spacing of float32 below 1 (its rounding is at most half of that)."""
    a, b = cc.pair((60, 80), 21)
    worst = 0.0
    for w in (2, 7, 35):
        e = cs.lattice(a, b, w, (w // 2 + 1, w // 2 + 2), (9, 11), (3, 4), 1)
        for i in range(3):
            for j in range(4):
                r_lo, c_lo = 1 + 9 * i, 2 + 11 * j
                wa, wb = a[r_lo:r_lo + w, c_lo:c_lo + w], b[r_lo:r_lo + w, c_lo:c_lo + w]
                assert wa.shape == (w, w) and e['count'][i, j] == w * w
                ref = pm_oracle.match_template(wb, wa)
                assert ref.shape == (1, 1)
                worst = max(worst, abs(float(ref[0, 0]) - e['r'][i, j]))
    print('max |spec - oracle| = %.3e' % worst)
    assert worst <= 2.0 ** -24


# ---------------------------------------------------------------- argument errors of the C entry points
def good_lattice():
    a, b = cc.pair((12, 17), 1)
    return dict(device=-1, a=a, a_stride=17, b=b, b_stride=17, rows=12, cols=17, w=5, r0=2, c0=2, sr=2, sc=3, nr=4, nc=5, min_count=3,
                corr=np.zeros((4, 5)), count=np.zeros((4, 5), np.int32), sums=np.zeros((4, 5, 5), np.int64))


def call_lattice(device, a, a_stride, b, b_stride, rows, cols, w, r0, c0, sr, sc, nr, nc, min_count, corr, count, sums):
    return _capi.lib().sid_corr_lattice(device, vp(a), a_stride, vp(b), b_stride, rows, cols, w, r0, c0, sr, sc, nr, nc, min_count,
                                        vp(corr), vp(count), vp(sums))


def good_points():
    g = good_lattice()
    for k in ('r0', 'c0', 'sr', 'sc', 'nr', 'nc'):
        del g[k]
    g.update(c=np.array([3, 4, 5], np.int32), r=np.array([3, 4, 5], np.int32), valid=None, npts=3, corr=np.zeros(3),
             count=np.zeros(3, np.int32), sums=np.zeros((3, 5), np.int64))
    return g


def call_points(device, a, a_stride, b, b_stride, rows, cols, w, c, r, valid, npts, min_count, corr, count, sums):
    return _capi.lib().sid_corr_points(device, vp(a), a_stride, vp(b), b_stride, rows, cols, w, vp(c), vp(r), vp(valid), npts, min_count,
                                       vp(corr), vp(count), vp(sums))


COMMON_ERRORS = [
    ('null a', dict(a=None), ERR_ARG), ('null b', dict(b=None), ERR_ARG),
    ('no output', dict(corr=None, count=None, sums=None), ERR_ARG),
    ('negative rows', dict(rows=-1), ERR_ARG), ('negative cols', dict(cols=-1), ERR_ARG),
    ('a stride', dict(a_stride=16), ERR_ARG), ('b stride', dict(b_stride=16), ERR_ARG),
    ('min_count 0', dict(min_count=0), ERR_ARG), ('min_count negative', dict(min_count=-3), ERR_ARG),
    ('window 0', dict(w=0), ERR_UNSUPPORTED), ('window 256', dict(w=256), ERR_UNSUPPORTED), ('window negative', dict(w=-5), ERR_UNSUPPORTED),
    ('rows too large', dict(rows=1 << 31), ERR_UNSUPPORTED),
    ('cols too large', dict(cols=1 << 31, a_stride=1 << 31, b_stride=1 << 31), ERR_UNSUPPORTED),
]
LATTICE_ERRORS = COMMON_ERRORS + [
    ('negative nr', dict(nr=-1), ERR_ARG), ('negative nc', dict(nc=-1), ERR_ARG),
    ('sr 0', dict(sr=0), ERR_ARG), ('sc 0', dict(sc=0), ERR_ARG), ('sr negative', dict(sr=-2), ERR_ARG),
    ('too many nodes', dict(nr=1 << 16, nc=1 << 15), ERR_UNSUPPORTED),
]
POINTS_ERRORS = COMMON_ERRORS + [
    ('negative npts', dict(npts=-1), ERR_ARG), ('null c', dict(c=None), ERR_ARG), ('null r', dict(r=None), ERR_ARG),
    ('too many points', dict(npts=1 << 31), ERR_UNSUPPORTED),
]


def _errors(good, call, what, change, code):
    header = open(os.path.join(ROOT, 'include', 'sid_pm.h')).read()
    assert re.search(r'SID_PM_ERR_ARG\s+\(?-1\)?', header) and re.search(r'SID_PM_ERR_UNSUPPORTED\s+\(?-4\)?', header)
    assert call(**good()) == 0
    args = good()
    args.update(change)
    assert call(**args) == code, what
    assert _capi.lib().sid_corr_last_error()
    args['device'] = 0                                     # found before any device call: the same without a GPU
    assert call(**args) == code, what


@pytest.mark.parametrize('what,change,code', LATTICE_ERRORS, ids=[h[0] for h in LATTICE_ERRORS])
def test_lattice_argument_errors(what, change, code):
    _errors(good_lattice, call_lattice, what, change, code)


@pytest.mark.parametrize('what,change,code', POINTS_ERRORS, ids=[h[0] for h in POINTS_ERRORS])
def test_points_argument_errors(what, change, code):
    _errors(good_points, call_points, what, change, code)


def test_device_entry_points_refuse_the_same_before_any_device_call():
    """The _device versions run the same checks first: an error comes back on a machine without a GPU too."""
    g = good_lattice()
    L = _capi.lib()
    tail = (g['rows'], g['cols'], 0, 2, 2, 2, 3, 4, 5, 3, vp(g['corr']), None, None, None)
    assert L.sid_corr_lattice_device(vp(g['a']), 17, vp(g['b']), 17, *tail) == ERR_UNSUPPORTED
    p = good_points()
    assert L.sid_corr_points_device(vp(p['a']), 17, vp(p['b']), 17, 12, 17, 5, None, vp(p['r']), None, 3, 3, vp(p['corr']), None, None,
                                    None) == ERR_ARG
    assert L.sid_corr_points_device(vp(p['a']), 17, vp(p['b']), 17, 12, 17, 5, vp(p['c']), vp(p['r']), None, 3, 3, None, None, None,
                                    None) == ERR_ARG


def test_outputs_may_not_overlap_the_images():
    buf = np.zeros(12 * 17 + 4004, dtype=np.uint8)
    buf[:12 * 17] = cc.pair((12, 17), 1)[0].ravel()
    for key, dtype in (('corr', np.float64), ('count', np.int32), ('sums', np.int64)):
        for image in ('a', 'b'):
            args = good_lattice()
            args[image] = buf[:12 * 17].reshape(12, 17)
            args[key] = buf[200:200 + 8].view(dtype)                         # begins inside the image
            assert call_lattice(**args) == ERR_ARG and b'overlap' in _capi.lib().sid_corr_last_error()
            aligned = buf[208:].view(dtype)                                      # begins behind it: fine
            args[key] = aligned
            assert call_lattice(**args) == 0


def test_empty_calls_are_not_errors():
    args = good_lattice()
    assert call_lattice(**dict(args, nr=0)) == 0 and call_lattice(**dict(args, nc=0)) == 0
    assert call_points(**dict(good_points(), npts=0, c=None, r=None)) == 0
    for device in (-1,):
        a = dict(args, rows=0, device=device)
        assert call_lattice(**a) == 0 and not a['count'].any() and np.isnan(a['corr']).all() and not a['sums'].any()
        a = dict(args, cols=0, device=device, corr=np.zeros((4, 5)), count=np.ones((4, 5), np.int32))
        assert call_lattice(**a) == 0 and not a['count'].any() and np.isnan(a['corr']).all()
    one = dict(args, corr=None, sums=None, count=np.full((4, 5), -1, np.int32))                      # one output alone
    assert call_lattice(**one) == 0 and (one['count'] == 25).all()


# ---------------------------------------------------------------- argument errors and defaults of the Python functions
def test_python_argument_errors():
    a, b = cc.pair((12, 17), 1)

    def call(**change):
        return libcorr.local_correlation(**dict(dict(a=a, b=b, window=5, device=-1), **change))

    def call_at(**change):
        return libcorr.local_correlation_at(**dict(dict(a=a, b=b, c=[3, 4], r=[5, 6], window=5, device=-1), **change))
    assert call().shape == (8, 13) and call_at().shape == (2,)
    for fn in (call, call_at):
        with pytest.raises(TypeError, match='a is float32'):
            fn(a=a.astype(np.float32))
        with pytest.raises(TypeError, match='b is int16'):
            fn(b=b.astype(np.int16))
        with pytest.raises(ValueError, match='a must be 2-D'):
            fn(a=a[0])
        with pytest.raises(ValueError, match='one shape'):
            fn(b=b[:, :5])
        for bad in (0, 256, 2.5, -1):
            with pytest.raises(ValueError, match='window must be an integer in 1..255'):
                fn(window=bad)
        for bad in (0, -2, 1.5):
            with pytest.raises(ValueError, match='min_count must be an integer >= 1'):
                fn(min_count=bad)
        with pytest.raises(ValueError, match='device must be a HIP device index'):
            fn(device=-2)
    for bad in (0, (1, 0), (1, 2, 3), 'ab', 1.5, (2, -1)):
        with pytest.raises(ValueError, match='step must be'):
            call(step=bad)
    for bad in ((1,), (1.5, 2), 'ab'):
        with pytest.raises(ValueError, match='origin must be'):
            call(origin=bad)
    for bad in ((-1, 2), (2,), (1.5, 2), 'ab'):
        with pytest.raises(ValueError, match='shape must be'):
            call(shape=bad)
    with pytest.raises(ValueError, match='c and r must have one shape'):
        call_at(c=[1, 2, 3])
    with pytest.raises(ValueError, match='not integers'):
        call_at(c=[1.5, 2.0])
    with pytest.raises(ValueError, match='not integers'):
        call_at(r=np.array([np.nan, 2.0]))
    with pytest.raises(ValueError, match='int32 cannot hold'):
        call_at(c=np.array([1 << 40, 2]))
    with pytest.raises(TypeError, match='c is bool'):
        call_at(c=np.array([True, False]))
    with pytest.raises(TypeError, match='valid is float64'):
        call_at(valid=np.ones(2))
    with pytest.raises(ValueError, match='valid must have the shape'):
        call_at(valid=np.ones(3, dtype=bool))
    torch = pytest.importorskip('torch')
    with pytest.raises(TypeError, match='not a mix'):
        call(a=torch.from_numpy(a))
    with pytest.raises(TypeError, match='not a mix'):
        call_at(c=torch.tensor([3, 4]))
    with pytest.raises(TypeError, match='on one ROCm device'):
        libcorr.local_correlation(torch.from_numpy(a), torch.from_numpy(b), window=5)


def test_python_defaults_and_conventions():
    a, b = cc.pair((40, 50), 2, zeros=0.05)
    r = libcorr.local_correlation(a, b, window=7, device=-1)                   # step 1, origin (3, 3), whole windows, half the window
    e = cs.lattice(a, b, 7, (3, 3), (1, 1), (34, 44), 25)
    assert cs.same_bits(r, e['r'])
    r, n = libcorr.local_correlation(a, b, window=8, step=(3, 5), return_count=True, device=-1)
    e = cs.lattice(a, b, 8, (4, 4), (3, 5), (11, 9), 32)
    assert cs.same_bits(r, e['r']) and cs.same_bits(n, e['count'])
    r, s = libcorr.local_correlation(a, b, window=7, step=4, return_sums=True, device=-1)
    assert cs.same_bits(s, cs.lattice(a, b, 7, (3, 3), (4, 4), (9, 11), 25)['sums'])
    assert libcorr.local_correlation(a[:5], b[:5], window=7, device=-1).shape == (0, 44)               # smaller than the window
    e = cs.lattice(a[::2, ::3], b[::2, ::3], 5, (2, 2), (1, 1), (16, 13), 13)                          # an inner stride is copied
    assert cs.same_bits(libcorr.local_correlation(a[::2, ::3], b[::2, ::3], window=5, device=-1), e['r'])
    e = cs.lattice(a[:, 3:40], b[:, 5:42], 5, (2, 2), (1, 1), (36, 33), 13)                            # views as they are
    assert cs.same_bits(libcorr.local_correlation(a[:, 3:40], b[:, 5:42], window=5, device=-1), e['r'])
    c, r = np.array([[3.0, 10.0], [np.nan, 49.0]]), np.array([[4.0, 11.0], [5.0, np.inf]])          # floats that hold integers
    valid = np.array([[1, 1], [0, 0]], dtype=bool)
    got = libcorr.local_correlation_at(a, b, c, r, window=9, valid=valid, min_count=1, return_count=True, return_sums=True, device=-1)
    e = cs.points(a, b, 9, np.array([[3, 10], [0, 0]]), np.array([[4, 11], [0, 0]]), valid, 1)
    assert all(cs.same_bits(g, e[k]) for g, k in zip(got, ('r', 'count', 'sums')))
    for dtype in (np.int8, np.uint16, np.int64):
        got = libcorr.local_correlation_at(a, b, np.array([3, 10], dtype=dtype), np.array([4, 11], dtype=dtype), window=9, device=-1)
        assert cs.same_bits(got, cs.points(a, b, 9, [3, 10], [4, 11], None, 41)['r'])


# ---------------------------------------------------------------- exported symbols
def test_header_symbols():
    header = open(os.path.join(ROOT, 'include', 'sid_corr.h')).read()
    body = re.sub(r'/\*.*?\*/', '', header, flags=re.S)
    assert sorted(set(re.findall(r'\b(sid_corr_\w+)\s*\(', body))) == sorted(_capi.CORR_SYMBOLS)
    lib = _capi.lib()
    for name in _capi.CORR_SYMBOLS:
        assert hasattr(lib, name), name
    assert (int(re.search(r'SID_CORR_TILE_ROWS\s+(\d+)', header).group(1)),
            int(re.search(r'SID_CORR_TILE_COLS\s+(\d+)', header).group(1))) == _capi.CORR_TILE
    _capi.release_workspaces()                                                  # (nothing cached without a GPU: no device call)


# ---------------------------------------------------------------- the warp's quality, on the host instance
def test_get_warp_correlation_on_the_synthetic_pair():
    """SeaIceDrift.get_warp_correlation with the true field: image 2 warped onto image 1 correlates with it, node by node, better
    than unwarped; it is get_warped_image followed by local_correlation_at at the rounded nodes."""
    from sea_ice_drift_amd.domain import ArrayNansat
    from sea_ice_drift_amd.seaicedrift import SeaIceDrift
    img1, img2 = synthetic.make_pair(400, 400, seed=17)
    geo = dict(origin=(10.0, 70.0), matrix=((0.002, 0.0), (0.0, -0.001)))
    n1, n2 = ArrayNansat(img1, **geo), ArrayNansat(img2, **geo)
    y, x = np.meshgrid(np.arange(40.0, 400.0, 40.0), np.arange(40.0, 400.0, 40.0), indexing='ij')
    dc, dr = synthetic.true_displacement(x, y)
    lons, lats = n1.transform_points(x, y, 0)
    lon2, lat2 = n2.transform_points(x + dc, y + dr, 0)
    lons, lats, lon2, lat2 = [np.asarray(q).reshape(x.shape) for q in (lons, lats, lon2, lat2)]
    lons[0, 0] = np.nan                                                        # a node without a position: NaN, count 0
    sid = SeaIceDrift(n1, n2)
    r, count = sid.get_warp_correlation(lons, lats, lon2, lat2, window=35, return_count=True, device=-1)
    assert r.shape == x.shape and count.dtype == np.int32 and np.isnan(r[0, 0]) and count[0, 0] == 0
    warped = sid.get_warped_image(lons, lats, lon2, lat2, device=-1)
    x1, y1 = [np.asarray(q).reshape(x.shape) for q in n1.transform_points(lons, lats, 1)]
    ok = np.isfinite(x1) & np.isfinite(y1)
    e = cs.points(img1, warped, 35, np.where(ok, np.rint(x1), 0).astype(np.int64), np.where(ok, np.rint(y1), 0).astype(np.int64), ok, 613)
    assert cs.same_bits(r, e['r']) and cs.same_bits(count, e['count'])
    unwarped = cs.points(img1, img2, 35, np.rint(x).astype(np.int64), np.rint(y).astype(np.int64), None, 613)['r']
    both = np.isfinite(r) & np.isfinite(unwarped)
    print('mean r over %d nodes: %.4f unwarped, %.4f warped with the true field' % (both.sum(), unwarped[both].mean(), r[both].mean()))
    assert both.sum() >= 20 and r[both].mean() > unwarped[both].mean()
    assert sid.get_warp_correlation(lons, lats, lon2, lat2, window=21, order=0, device=-1).shape == x.shape
