"""GPU: the sub-pixel peak (include/sid_pm.h SID_PM_SUBPIXEL, ``subpixel=True``) in every kernel family and every place the
winner's NCC matrix can live - LDS, the recycled global blocks, the kept accumulators, the large-window pipeline's global
matrix - and through every public call.

Every case asserts that c2, r2 under the flag equal, bit for bit, the C oracle's c2, r2 plus the specification's offsets
(tests/subpixel_spec.py) on the ORACLE's raw matrix - never the device's own - and that angle, r, h and the peak indices equal
those of the same call without the flag bit for bit.  What a case is made for (no NaN point, interior peaks with both offsets
non-zero, peaks on the frame, the launch class) is asserted from the oracle and the host arithmetic before the kernels run."""
import contextlib
import io

import numpy as np
import pytest

from sea_ice_drift_amd import _capi, pmlib, synthetic as syn
from sea_ice_drift_amd.domain import ArrayNansat
from tests import subpixel_spec as sp

pytestmark = pytest.mark.gpu

SIZE = 300
A3, A15 = [-3, 0, 3], list(range(-7, 8))
_CACHE = {}


def _pair():
    if 'pair' not in _CACHE:
        _CACHE['pair'] = syn.make_pair(SIZE, SIZE, seed=2)
    return _CACHE['pair']


def _grid(n, b, s):
    return syn.make_grid(SIZE, SIZE, n, border=b, seed=5, margin=b + s // 2 + 25)


def _vec(g):
    return [g[k] for k in ('c1', 'r1', 'c2fg', 'r2fg', 'border')]


def _oracle(c_oracle, name, pair, g, s, angles, flags):
    """(oracle's rows without the flag, its peak indices, per-point offsets from its matrices); computed once per case.  The
    matrix of the winning angle does not depend on the flags, so the offsets are shared by the flag sets of a case."""
    kp = (name, s, tuple(angles))
    if kp not in _CACHE:
        _CACHE[kp] = sp.oracle_offsets(c_oracle, pair[0], pair[1], g, s, angles, flags=1)
    kb = kp + (flags,)
    if kb not in _CACHE:
        exp, exp_ij = c_oracle.pm_batch(pair[0], pair[1], *_vec(g), s, 0.0, angles, rot=pmlib.rotation_table(angles, 0.0, s),
                                        flags=flags, nthreads=16)
        exp.setflags(write=False); exp_ij.setflags(write=False)
        _CACHE[kb] = (exp, exp_ij)
    pts = _CACHE[kp]
    exp, exp_ij = _CACHE[kb]
    for i, p in enumerate(pts):                                       # the two oracle calls agree on the peak
        assert tuple(p['ij']) == tuple(exp_ij[i])
        assert p['nan'] or (p['out'][0] == exp[i, 0] and p['out'][1] == exp[i, 1])
    return exp, exp_ij, pts


def _claim(pts, frame=False, nan_rows=()):
    """What the case is made for, from the oracle."""
    assert [i for i, p in enumerate(pts) if p['nan']] == list(nan_rows)
    live = [p for p in pts if not p['nan']]
    both = sum(1 for p in live if all(p['interior']) and p['dx'] != 0.0 and p['dy'] != 0.0)
    on_frame = sum(1 for p in live if not all(p['interior']))
    if frame:
        assert on_frame >= 1 and both >= 1
        assert any((p['interior'][0] != p['interior'][1]) and (p['dx'] != 0.0 or p['dy'] != 0.0) for p in live)   # zero next to non-zero
    else:
        assert 4 * both >= 3 * len(pts), '%d of %d points have an interior peak with both offsets non-zero' % (both, len(pts))
    for p in live:
        assert -0.5 <= p['dx'] <= 0.5 and -0.5 <= p['dy'] <= 0.5
        assert (p['interior'][0] or p['dx'] == 0.0) and (p['interior'][1] or p['dy'] == 0.0)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _check(got, ij, base, base_ij, exp, exp_ij, pts, mcc_norm=False, msg=''):
    """got / ij: the call with the flag; base / base_ij: the same call without; exp / exp_ij / pts: the oracle."""
    np.testing.assert_array_equal(base_ij, exp_ij, err_msg=msg)       # the call without the flag is today's (the parity rule's exact part)
    np.testing.assert_array_equal(base[:, :3], exp[:, :3], err_msg=msg)
    np.testing.assert_array_equal(ij, base_ij, err_msg=msg)
    np.testing.assert_array_equal(_bits(got[:, 2:]), _bits(base[:, 2:]), err_msg=msg + ': angle, r, h changed under the flag')
    want = sp.expected_c2r2(exp, pts)
    nan = np.array([p['nan'] for p in pts])
    assert np.isnan(got[nan]).all() and (ij[nan] == -1).all(), msg
    np.testing.assert_array_equal(_bits(got[~nan, :2]), _bits(want[~nan]), err_msg=msg + ': c2, r2 under the flag')


def _run(ctx, g, s, angles, flags):
    ctx.set_points(*_vec(g), s, 0.0, angles, rot=pmlib.rotation_table(angles, 0.0, s), flags=flags)
    ctx.run()
    return ctx.fetch()


def _case(pm_ctx, c_oracle, name, g, s, angles, flag_sets=(1,), frame=False, pair=None, nan_rows=()):
    pair = pair or _pair()
    pm_ctx.upload_pair(*pair)
    for flags in flag_sets:
        exp, exp_ij, pts = _oracle(c_oracle, name, pair, g, s, angles, flags)
        _claim(pts, frame=frame, nan_rows=nan_rows)
        base, base_ij = _run(pm_ctx, g, s, angles, flags)
        got, ij = _run(pm_ctx, g, s, angles, flags | _capi.SUBPIXEL)
        _check(got, ij, base, base_ij, exp, exp_ij, pts, msg='%s side %d, %d angles, flags %d' % (name, s, len(angles), flags))


def _classes(g, s, K, flags=1):
    return _capi.estimate_residency(g['border'], s, K, flags)


# ---- row-pair kernels, NCC matrix in LDS ----

@pytest.mark.parametrize('angles', [A3, A15], ids=['3', '15'])
@pytest.mark.parametrize('s', [34, 35])
def test_row_pair_defaults(pm_ctx, c_oracle, s, angles):
    """Border 20, the reference's flags: ph_hessian_fast."""
    g = _grid(4, 20, s)
    assert not (_classes(g, s, len(angles)) & (_capi.CLASS_BIG | _capi.CLASS_LARGE)).any()
    _case(pm_ctx, c_oracle, 'rp20', g, s, angles)


@pytest.mark.parametrize('angles', [A3, A15], ids=['3', '15'])
@pytest.mark.parametrize('s', [34, 35])
def test_row_pair_general_hessian_reads_the_raw_matrix(pm_ctx, c_oracle, s, angles):
    """hes_smth, mcc_norm and both: the general ph_hessian, which smooths the matrix in place - offsets read after that would be
    those of the smoothed matrix."""
    _case(pm_ctx, c_oracle, 'rp20', _grid(4, 20, s), s, angles, flag_sets=(3, 5, 7))


# ---- global-table classes ----

@pytest.mark.parametrize('s', [34, 35])
def test_kept_accumulators(pm_ctx, c_oracle, s):
    """Border 30 with 3 angles: sums and accumulators in recycled global blocks, the winner's matrix normalised from them."""
    g = _grid(4, 30, s)
    assert (_classes(g, s, 3) & _capi.CLASS_GS).all()
    _case(pm_ctx, c_oracle, 'gs30', g, s, A3)


def test_global_sums_border_50(pm_ctx, c_oracle):
    g = _grid(3, 50, 35)
    cls = _classes(g, 35, 15)
    assert (cls & _capi.CLASS_GS).all() and not (cls & (_capi.CLASS_BIG | _capi.CLASS_LARGE)).any()
    _case(pm_ctx, c_oracle, 'gs50', g, 35, A15)


@pytest.mark.parametrize('s', [34, 35])
def test_big_layout_matrix_in_global_memory(pm_ctx, c_oracle, s):
    """Border 70: every per-placement table, the NCC matrix among them, in the point's block of global memory."""
    g = _grid(2, 70, s)
    assert (_classes(g, s, 2) & _capi.CLASS_BIG).all()
    _case(pm_ctx, c_oracle, 'big70', g, s, [0, 3], flag_sets=(1, 3))


# ---- classic kernel ----

@pytest.mark.parametrize('s,b,frame', [(20, 5, False), (64, 7, False), (50, 4, True), (2, 3, True)])
def test_classic_kernel(pm_ctx, c_oracle, s, b, frame):
    """Sides with three and four k-groups, the largest and the smallest side; 50 / 4 and 2 / 3 have peaks on the frame of the
    matrix: a zero offset on that axis next to a non-zero one on the other."""
    g = _grid(4, b, s)
    assert not (_classes(g, s, 3) & (_capi.CLASS_GS | _capi.CLASS_LARGE)).any()
    _case(pm_ctx, c_oracle, 'classic', g, s, A3, flag_sets=(1, 7), frame=frame)


# ---- large-window pipeline ----

def test_large_window_point(pm_ctx, c_oracle):
    g = dict(c1=np.array([150.0]), r1=np.array([150.0]), c2fg=np.array([150.0]), r2fg=np.array([150.0]), border=np.array([112.0]))
    assert (_classes(g, 34, 3) & _capi.CLASS_LARGE).all()
    _case(pm_ctx, c_oracle, 'large112', g, 34, A3, flag_sets=(1, 7))


@pytest.mark.parametrize('s,window', [(20, (120, 105, 60, 90)), (100, (80, 85, 140, 130))], ids=['20', '100'])
def test_rotate_and_match(pm_ctx, c_oracle, s, window):
    img1, img2 = _pair()
    r0, c0, wh, ww = window
    rot = pmlib.rotation_table(A3, 0.0, s)
    pm_ctx.upload_pair(img1, img2)
    for flags in (1, 3, 7):
        exp = c_oracle.rotate_and_match(img1, 150.0, 150.0, s, np.ascontiguousarray(img2[r0:r0 + wh, c0:c0 + ww]), 0.0, A3, rot, flags=flags)
        assert exp['ij'][2] >= 0 and exp['ccm'].shape == (wh - s + 1, ww - s + 1)
        iy, ix = int(exp['ij'][0]), int(exp['ij'][1])
        dx, dy = sp.offsets(exp['ccm'], iy, ix)
        assert 0 < iy < wh - s and 0 < ix < ww - s and dx != 0.0 and dy != 0.0
        base = pm_ctx.rotate_and_match(150.0, 150.0, s, 0.0, A3, rot=rot, flags=flags, window=window)
        got = pm_ctx.rotate_and_match(150.0, 150.0, s, 0.0, A3, rot=rot, flags=flags | _capi.SUBPIXEL, window=window)
        msg = 'side %d, flags %d' % (s, flags)
        np.testing.assert_array_equal(base['out'][:3], exp['out'][:3], err_msg=msg)
        np.testing.assert_array_equal(got['ij'], exp['ij'], err_msg=msg)
        np.testing.assert_array_equal(got['ccm'], exp['ccm'], err_msg=msg)                    # best_result is still the oracle's
        np.testing.assert_array_equal(got['template'], exp['template'], err_msg=msg)
        np.testing.assert_array_equal(_bits(got['out'][2:]), _bits(base['out'][2:]), err_msg=msg)
        want = np.array([exp['out'][0] + dx, exp['out'][1] + dy])
        np.testing.assert_array_equal(_bits(got['out'][:2]), _bits(want), err_msg=msg)


def test_pmlib_rotate_and_match_keyword(c_oracle):
    img1, img2 = _pair()
    image2 = np.ascontiguousarray(img2[120:180, 105:195])
    exp = c_oracle.rotate_and_match(img1, 150.0, 150.0, 20, image2, 0.0, A3, pmlib.rotation_table(A3, 0.0, 20))
    dx, dy = sp.offsets(exp['ccm'], exp['ij'][0], exp['ij'][1])
    base = pmlib.rotate_and_match(img1, 150.0, 150.0, 20, image2, 0.0, angles=A3)
    got = pmlib.rotate_and_match(img1, 150.0, 150.0, 20, image2, 0.0, angles=A3, subpixel=True)
    assert (base[0], base[1]) == (exp['out'][0], exp['out'][1])
    assert (got[0], got[1]) == (exp['out'][0] + dx, exp['out'][1] + dy) and dx != 0.0 and dy != 0.0
    assert got[2:5] == base[2:5]
    np.testing.assert_array_equal(got[5], exp['ccm'])
    np.testing.assert_array_equal(got[6], base[6])


# ---- every launch class in one set of points ----

def _mixed_points():
    c1 = np.array([130.0, 150.0, 170.0, 150.0, 130.0, 150.0, 170.0, 150.0, 130.0, 170.0, 150.0, 140.0])
    r1 = np.array([130.0, 130.0, 130.0, 150.0, 150.0, 170.0, 170.0, 150.0, 170.0, 150.0, 160.0, 140.0])
    border = np.array([20.0, 30.0, 70.0, 112.0, 30.0, 20.0, 70.0, 112.0, 20.0, 30.0, 70.0, 20.0])
    dc, dr = syn.true_displacement(c1, r1)
    err = np.random.Generator(np.random.PCG64(9)).integers(-1, 2, size=(2, c1.size))
    c2fg, r2fg = c1 + np.rint(dc) + err[0], r1 + np.rint(dr) + err[1]
    big = border == 112.0
    c2fg[big], r2fg[big] = 150.0, 150.0                               # (a window of 259 px has a pixel of room on a 300 px image)
    return dict(c1=c1, r1=r1, c2fg=c2fg, r2fg=r2fg, border=border)


def test_mixed_launch_classes_write_their_rows_in_place(pm_ctx, c_oracle):
    g = _mixed_points()
    cls = _classes(g, 34, 3)
    b = g['border']
    assert (cls[b == 112] & _capi.CLASS_LARGE).all() and (cls[b == 70] & _capi.CLASS_BIG).all() and (cls[b == 30] & _capi.CLASS_GS).all()
    assert not (cls[b == 20] & (_capi.CLASS_BIG | _capi.CLASS_LARGE)).any()
    assert len(set(cls.tolist())) >= 4
    _case(pm_ctx, c_oracle, 'mixed', g, 34, A3, flag_sets=(1, 3))


# ---- NaN points ----

def test_zero_pixel_point_stays_nan(pm_ctx, c_oracle):
    img1, img2 = _pair()
    g = _grid(4, 20, 34)
    img1 = img1.copy()
    img1[int(g['r1'][5]), int(g['c1'][5])] = 0                        # the centre of point 5's template
    _case(pm_ctx, c_oracle, 'zero', g, 34, A3, pair=(img1, img2), nan_rows=(5,))


# ---- public calls ----

def test_pm_dispatch_on_two_handles(c_oracle):
    img1, img2 = _pair()
    g = _grid(4, 20, 34)
    exp, exp_ij, pts = _oracle(c_oracle, 'rp20', (img1, img2), g, 34, A3, 1)
    one = pmlib.pm_dispatch(img1, img2, *_vec(g), 34, 0.0, angles=A3, subpixel=True)
    two = pmlib.pm_dispatch(img1, img2, *_vec(g), 34, 0.0, angles=A3, subpixel=True, devices=[0, 0])
    off = pmlib.pm_dispatch(img1, img2, *_vec(g), 34, 0.0, angles=A3, devices=[0, 0])
    np.testing.assert_array_equal(_bits(two), _bits(one))
    np.testing.assert_array_equal(_bits(one[:, :2]), _bits(sp.expected_c2r2(exp, pts)))
    np.testing.assert_array_equal(off[:, :3], exp[:, :3])
    np.testing.assert_array_equal(_bits(one[:, 2:]), _bits(off[:, 2:]))
    c2, r2, a, r, h = pmlib.use_mcc(g['c1'][3], g['r1'][3], g['c2fg'][3], g['r2fg'][3], 20.0, img1, img2, 34, 0.0, angles=A3, subpixel=True)
    assert (c2, r2, a) == tuple(one[3, :3]) and r == np.float32(one[3, 3]) and h == np.float32(one[3, 4])


def test_pattern_matching_keyword(c_oracle):
    """Identity georeference: u, v are c2 - c1, r2 - r1 of the grid, so the keyword moves them by the offsets and nothing else."""
    img1, img2 = _pair()
    n1, n2 = ArrayNansat(img1), ArrayNansat(img2)
    rng = np.random.Generator(np.random.PCG64(40))
    kc1, kr1 = rng.uniform(30, 270, 40), rng.uniform(30, 270, 40)
    dc, dr = syn.true_displacement(kc1, kr1)
    kc2, kr2 = kc1 + dc, kr1 + dr
    cg, rg = np.meshgrid(np.rint(np.linspace(90, 210, 6)), np.rint(np.linspace(90, 210, 6)))
    lon, lat = n1.transform_points(cg, rg, 0)
    with contextlib.redirect_stdout(io.StringIO()):
        off = pmlib.pattern_matching(lon, lat, n1, kc1, kr1, n2, kc2, kr2, subpixel=False)
        on = pmlib.pattern_matching(lon, lat, n1, kc1, kr1, n2, kc2, kr2, subpixel=True)
        pre = pmlib.pm_prelude(lon, lat, n1, kc1, kr1, n2, kc2, kr2, img_size=35)
    gpi = pre['gpi']
    assert gpi.sum() >= 30 and pre['alpha0'] == 0.0
    g = dict(c1=pre['c1pm1i'][gpi], r1=pre['r1pm1i'][gpi], c2fg=pre['c2fg'][gpi], r2fg=pre['r2fg'][gpi], border=pre['brd2'][gpi])
    exp, exp_ij, pts = _oracle(c_oracle, 'pm', (img1, img2), g, 35, A3, 1)
    _claim(pts)
    for k in (2, 3, 4):                                               # a, r, h
        np.testing.assert_array_equal(_bits(on[k]), _bits(off[k]))
    for k in range(7):
        np.testing.assert_array_equal(np.isnan(on[k]), np.isnan(off[k]))
    assert np.isfinite(off[0].ravel()[gpi.ravel()]).all()
    with_off = np.array(exp, copy=True)
    with_off[:, :2] = sp.expected_c2r2(exp, pts)
    want_off, want_on = pmlib.pm_postlude(pre, exp, n2), pmlib.pm_postlude(pre, with_off, n2)
    for k in (0, 1, 5, 6):                                            # u, v, lon2, lat2
        np.testing.assert_array_equal(_bits(off[k]), _bits(want_off[k]))
        np.testing.assert_array_equal(_bits(on[k]), _bits(want_on[k]))
    dxy = np.array([[p['dx'], p['dy']] for p in pts])
    sel = gpi.reshape(on[0].shape)
    np.testing.assert_allclose((on[0] - off[0])[sel], dxy[:, 0], rtol=0, atol=2.0 ** -40)   # (the sums were rounded at ~2^8)
    np.testing.assert_allclose((on[1] - off[1])[sel], dxy[:, 1], rtol=0, atol=2.0 ** -40)


# ---- C ABI ----

def test_c_abi_accepts_the_flag(pm_ctx, c_oracle):
    img1, img2 = _pair()
    g = _grid(4, 20, 34)
    pm_ctx.upload_pair(img1, img2)
    pm_ctx.set_points(*_vec(g), 34, 0.0, A3, rot=pmlib.rotation_table(A3, 0.0, 34), flags=128 | 1)
    assert _capi.lib().sid_pm_abi_version() == 6
    with pytest.raises(_capi.SidPmError) as e:                        # get_hessian keeps refusing it
        _capi.get_hessian(np.zeros((8, 8), dtype=np.float32), flags=128 | 1)
    assert e.value.code == -1
    for f in (1, 129):                                                # the estimates take it, and estimate the same
        assert np.array_equal(_capi.estimate_cost(g['border'], 34, 3, f), _capi.estimate_cost(g['border'], 34, 3, 1))
        assert np.array_equal(_capi.estimate_residency(g['border'], 34, 3, f), _capi.estimate_residency(g['border'], 34, 3, 1))
        assert _capi.estimate_run_time(g['border'], 34, 3, f) == _capi.estimate_run_time(g['border'], 34, 3, 1)
    exp, exp_ij, pts = _oracle(c_oracle, 'rp20', (img1, img2), g, 34, A3, 1)
    got, ij = _capi.pm_batch(img1, img2, *_vec(g), 34, 0.0, A3, rot=pmlib.rotation_table(A3, 0.0, 34), flags=129)
    np.testing.assert_array_equal(ij, exp_ij)
    np.testing.assert_array_equal(_bits(got[:, :2]), _bits(sp.expected_c2r2(exp, pts)))
    i = 6
    d = pm_ctx.debug_point(g['c1'][i], g['r1'][i], g['c2fg'][i], g['r2fg'][i], 20.0, 34, 0.0, A3, rot=pmlib.rotation_table(A3, 0.0, 34), flags=129)
    np.testing.assert_array_equal(d['ccm'], pts[i]['R'])
    np.testing.assert_array_equal(_bits(d['out'][:2]), _bits(sp.expected_c2r2(exp, pts)[i]))
