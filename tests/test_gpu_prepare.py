"""GPU parity of the sigma0 preparation (include/sid_prep.h; sea_ice_drift_amd.lib.prepare_image, get_spatial_mean,
hh_angular_correction; replaces the array half of get_n, lib.py:318-331) against the reference's own outputs (g11 fixture)
and against a NumPy restatement of the chain run on the same host."""
import contextlib
import io
import os
import warnings

import numpy as np
import pytest

from oracle import stage_oracle as so
from sea_ice_drift_amd import lib
from tests.golden import make_golden_prepare as mg

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
FACTOR = mg.HH_FACTOR


@pytest.fixture(scope='module')
def g11():
    return np.load(os.path.join(HERE, 'golden', 'g11_prepare.npz'))


def quiet(fn, *a, **k):
    with contextlib.redirect_stdout(io.StringIO()), warnings.catch_warnings(), np.errstate(all='ignore'):
        warnings.simplefilter('ignore')
        return fn(*a, **k)


def device_float(img, ia=None, mask=None, dB=False, coeffs=None):
    """The float32 working image of the device pass (what prepare_image hands to the uint8 staging)."""
    work, _ = lib._prep_apply(img, ia, mask, dB, FACTOR, coeffs is not None, coeffs, 0)
    return work.cpu().numpy()


def device_mean(shape, coeffs):
    import torch
    from sea_ice_drift_amd import _capi
    out = torch.empty(shape, dtype=torch.float64, device='cuda')
    _capi.prep_spatial_mean(shape[0], shape[1], coeffs, out.data_ptr(), out.stride(0), torch.cuda.current_stream().cuda_stream)
    return out.cpu().numpy()


def log10_cr(x):
    return np.log10(x.astype(np.float64)).astype(np.float32)


def numpy_spatial_mean(shape, x):
    cols, rows = np.meshgrid(np.arange(0, shape[1]), np.arange(0, shape[0]))
    img2 = x[0] * cols
    img2 += x[1] * cols ** 2
    img2 += x[2] * rows
    img2 += x[3] * rows ** 2
    img2 += x[4] * cols * rows
    img2 += x[5]
    return img2


def numpy_chain(img, dB=True, ia=None, mask=None, detrend=False, coeffs=None, floats=False):
    """get_n's lines 318-331 in NumPy with the correctly rounded logarithm; the fit is the package's host function (the
    reference's NumPy calls) on the same host as the call under test."""
    with np.errstate(all='ignore'), warnings.catch_warnings():
        warnings.simplefilter('ignore')
        img = np.array(img, dtype=np.float32, copy=True)
        if dB:
            img[img <= 0] = np.nan
            img = 10 * log10_cr(img)
        if ia is not None:
            img = img - ia * FACTOR
        if mask is not None:
            img[np.asarray(mask, dtype=bool)] = np.nan
        if detrend:
            x = lib.fit_spatial_mean(img[::50, ::50]) if coeffs is None else coeffs
            img -= numpy_spatial_mean(img.shape, x)
        assert img.dtype == np.float32
        return img if floats else so.get_uint8_image(img, None, None, mg.PMIN, mg.PMAX)[0]


def has_step(name, step):
    return bool(mg.STEPS[name] & step)


def case_args(name, steps, dB):
    lin, db, ia, mask = mg.inputs(name)
    return (lin if dB else db), (ia if steps & mg.HH else None), (mask if steps & mg.MASK else None)


# ---------------------------------------------------------------- dB alone
def test_db_is_the_correctly_rounded_logarithm():
    """10 * float32(log10(float64(x))): a pixel may differ from the host's value only by double rounding inside the device's
    float64 log10 (an error of a few float64 ulp next to a float32 rounding boundary: about 1e-8 of the pixels).  Condition:
    no difference above 1 float32 ulp, at most 1e-6 of the pixels different at all.  Inputs: every float32 binade including
    subnormals, SAR-like sigma0, zeros, negatives, NaN, +-inf."""
    rng = np.random.default_rng(501)
    n = 2048
    bits = rng.integers(1, 0x7f800000, (n, n), dtype=np.int64).astype(np.int32)          # every positive finite float32
    x = bits.view(np.float32).copy()
    x[: n // 2] = (10.0 ** rng.normal(-2.2, 0.5, (n // 2, n))).astype(np.float32)
    u = rng.random((n, n))
    x[u < 0.01] = 0.0
    x[(u >= 0.01) & (u < 0.02)] *= -1.0
    x[(u >= 0.02) & (u < 0.03)] = np.nan
    x[(u >= 0.03) & (u < 0.031)] = np.inf
    x[(u >= 0.031) & (u < 0.032)] = -np.inf
    x[0, :4] = [1.0, 10.0, 1e-45, 3.4028235e38]
    keep = x.copy()
    got = device_float(x, dB=True)
    assert np.array_equal(x.view(np.int32), keep.view(np.int32))
    with np.errstate(all='ignore'):
        exp = np.float32(10) * log10_cr(np.where(x > 0, x, np.nan).astype(np.float32))
    assert np.array_equal(np.isnan(got), np.isnan(exp)) and np.isnan(exp).sum() > 0.03 * n * n
    ok = ~np.isnan(exp)
    differ = ok & (got != exp)
    with np.errstate(all='ignore'):
        ulps = np.abs(got[differ].astype(np.float64) - exp[differ].astype(np.float64)) / np.spacing(np.abs(exp[differ])).astype(np.float64)
    print('dB: %d of %d pixels differ (share %.3g), max %.3g ulp' % (differ.sum(), ok.sum(), differ.sum() / ok.sum(),
                                                                      ulps.max() if ulps.size else 0.0))
    assert got[0, 0] == 0.0 and got[0, 1] == 10.0 and np.isposinf(got[x == np.inf]).all()
    assert ulps.size == 0 or ulps.max() <= 1.0
    assert differ.sum() <= 1e-6 * ok.sum()


def test_short_logarithm_equals_the_float64_route_for_every_float32():
    """The dB step decides most pixels with a short float64 evaluation and hands the rest to the library's float64 log10
    (csrc/prep.hip log10_f32).  Swept on the device over every positive float32 bit pattern, +inf included: not one differs
    from float(log10(double(x)))."""
    from sea_ice_drift_amd import _capi
    n = 0x7f800000                                             # bit patterns 1 .. 0x7f800000 (+inf)
    bad, slow = _capi.prep_debug_log10(1, n)
    print('log10 sweep: %d of %d differ; %d (1 in %.0f) took the library route' % (bad, n, slow, n / max(slow, 1)))
    assert bad == 0
    assert 0 < slow < n / 1000
    assert _capi.prep_debug_log10(0x80000000, 1 << 20) == (0, 0)        # negative patterns are skipped


# ---------------------------------------------------------------- float stages against the fixture, bit for bit
def test_hh_correction_bit_exact(g11):
    import torch
    for name in mg.CASES:
        if not has_step(name, mg.HH):
            continue
        _, db, ia, _ = mg.inputs(name)
        keep = db.copy()
        got = lib.hh_angular_correction(mg.Scene(ia), db, 'sigma0_HH', FACTOR)
        assert isinstance(got, np.ndarray) and got.dtype == np.float32 and got is not db
        assert np.array_equal(db.view(np.int32), keep.view(np.int32)), 'input modified'
        assert mg.digest(got) == str(g11[name + '_hh_sha']), name
        if name == 'small':
            assert mg.same_bits(got, g11['small_hh'])
        if name == 'view':                                    # the same on strided device views of the parents
            tdb, tia = [torch.from_numpy(np.ascontiguousarray(a.base)).cuda()[mg.VIEW] for a in (db, ia)]
            assert not tdb.is_contiguous()
            out = lib.hh_angular_correction(mg.Scene(tia), tdb, 'sigma0_HH', FACTOR)
            assert out.is_cuda and mg.digest(out.cpu().numpy()) == str(g11['view_hh_sha'])


def test_mask_and_detrend_with_fixture_coefficients_bit_exact(g11):
    for name in ('small', 'big', 'odd'):
        img, ia, mask = case_args(name, mg.STEPS[name], False)
        got = device_float(img, ia, mask, coeffs=g11[name + '_db0_coeffs'])
        assert mg.digest(got) == str(g11[name + '_detr_sha']), name
        if name == 'small':
            assert mg.same_bits(got, g11['small_detr'])
            assert np.isnan(got[mask]).all()


def test_spatial_mean_with_fixture_coefficients_bit_exact(g11):
    for name in ('small', 'big', 'odd'):
        shape = mg.inputs(name)[0].shape
        got = device_mean(shape, g11[name + '_db0_coeffs'])
        assert mg.digest(got) == str(g11[name + '_mean_sha']), name
        if name == 'small':
            assert mg.same_bits(got, g11['small_mean'])
    # a buffer whose rows are not 16-byte aligned, and an odd width on aligned rows
    import torch
    from sea_ice_drift_amd import _capi
    x = g11['big_db0_coeffs']
    for rows, cols, pad in ((37, 41, 0), (37, 41, 1), (64, 51, 3)):
        buf = torch.zeros((rows, cols + pad), dtype=torch.float64, device='cuda')
        _capi.prep_spatial_mean(rows, cols, x, buf.data_ptr(), buf.stride(0), torch.cuda.current_stream().cuda_stream)
        assert mg.same_bits(buf.cpu().numpy()[:, :cols], numpy_spatial_mean((rows, cols), x))
        assert (buf.cpu().numpy()[:, cols:] == 0).all()


# ---------------------------------------------------------------- uint8 against the fixture
def test_prepare_image_db_false_bit_exact(g11):
    """The input already in dB (get_n's denoise=True route): the reference's own uint8 output, for every combination of
    HH / mask / detrend (small) and for every other case's chain."""
    for k in range(8):
        img, ia, mask = case_args('small', k, False)
        coeffs = g11['small_db0_coeffs_%d' % k] if k & mg.DETREND else None
        got = quiet(lib.prepare_image, img, dB=False, incidence_angle=ia, mask=mask, remove_spatial_mean=bool(k & mg.DETREND),
                    spatial_mean_coeffs=coeffs)
        np.testing.assert_array_equal(got, g11['small_db0_u8_%d' % k], err_msg='small, combination %d' % k)
    for name in ('big', 'odd', 'view', 'tiny'):
        steps = mg.STEPS[name]
        img, ia, mask = case_args(name, steps, False)
        coeffs = g11[name + '_db0_coeffs'] if steps & mg.DETREND else None
        got = quiet(lib.prepare_image, img, dB=False, incidence_angle=ia, mask=mask, remove_spatial_mean=bool(steps & mg.DETREND),
                    spatial_mean_coeffs=coeffs)
        assert got.dtype == np.uint8
        np.testing.assert_array_equal(got, g11[name + '_db0_u8'], err_msg=name)


def test_prepare_image_db_true_against_both_logarithms(g11):
    """Bit for bit the reference's chain with the correctly rounded logarithm; against the same chain with NumPy's own
    float32 log10 (as recorded where the fixture was generated) no pixel off by more than one count and exactly the
    fixture's flip_share apart - the number README and DESIGN quote."""
    differ = total = 0
    for name in mg.CASES:
        steps = mg.STEPS[name]
        img, ia, mask = case_args(name, steps, True)
        keep = img.copy()
        coeffs = g11[name + '_db1_coeffs'] if steps & mg.DETREND else None
        got = quiet(lib.prepare_image, img, incidence_angle=ia, mask=mask, remove_spatial_mean=bool(steps & mg.DETREND),
                    spatial_mean_coeffs=coeffs)
        assert np.array_equal(img.view(np.int32), keep.view(np.int32)), 'input modified'
        cr = g11[name + '_db1_u8_cr']
        np.testing.assert_array_equal(got, cr, err_msg=name)
        npy = cr.copy()
        npy.ravel()[g11[name + '_db1_u8_numpy_idx']] = g11[name + '_db1_u8_numpy_val']
        d = np.abs(got.astype(np.int64) - npy.astype(np.int64))
        print('%s: %d of %d pixels differ from the NumPy-log10 chain, max %d' % (name, (d > 0).sum(), d.size, d.max()))
        assert d.max() <= 1
        assert (d > 0).sum() / d.size == float(g11[name + '_flip_share'])
        differ += int((d > 0).sum())
        total += d.size
    assert differ / total == float(g11['flip_share_all'])


# ---------------------------------------------------------------- the host fit in the loop
@pytest.mark.parametrize('dB', [False, True])
def test_end_to_end_with_the_host_fit(dB):
    """No spatial_mean_coeffs: the device's subsample feeds the host's lstsq; the restatement feeds the same lstsq the same
    numbers, so the coefficients - and the images - are equal bit for bit."""
    for name in ('small', 'big', 'odd'):
        img, ia, mask = case_args(name, mg.STEPS[name], dB)
        got = quiet(lib.prepare_image, img, dB=dB, incidence_angle=ia, mask=mask, remove_spatial_mean=True)
        np.testing.assert_array_equal(got, numpy_chain(img, dB, ia, mask, True), err_msg=name)


def test_get_spatial_mean_against_numpy():
    import torch
    for name in ('small', 'big', 'odd', 'view', 'tiny'):
        _, db, _, _ = mg.inputs(name)
        img = np.where(np.isfinite(db), db, np.nan).astype(np.float32)
        if name == 'tiny':
            img[0, 0] = -20.0            # one sample, not above its own 5th percentile: lstsq on an empty system (all zeros)
        keep = img.copy()
        with np.errstate(all='ignore'), warnings.catch_warnings():
            warnings.simplefilter('ignore')
            exp = numpy_spatial_mean(img.shape, lib.fit_spatial_mean(img[::50, ::50]))
        got = quiet(lib.get_spatial_mean, img)
        assert isinstance(got, np.ndarray) and got.dtype == np.float64
        assert mg.same_bits(got, exp), name
        t = torch.from_numpy(np.ascontiguousarray(img)).cuda()
        got_t = quiet(lib.get_spatial_mean, t)
        assert got_t.is_cuda and got_t.dtype == torch.float64 and mg.same_bits(got_t.cpu().numpy(), exp), name
        assert np.array_equal(img.view(np.int32), keep.view(np.int32))


# ---------------------------------------------------------------- a large scene, views, degenerate inputs
def large_scene():
    rng = np.random.default_rng(77)
    rows, cols = 3000, 2500
    c = np.arange(cols, dtype=np.float64)[None, :]
    lin = (10.0 ** ((-20.0 - 8.0 * c / cols + 4.0 * rng.standard_normal((rows, cols))) / 10.0)).astype(np.float32)
    lin[rng.random((rows, cols)) < 0.05] = np.nan
    lin[rng.random((rows, cols)) < 0.001] = 0.0
    lin[:, :20] = 0.0
    ia = np.broadcast_to((20.0 + 25.0 * c / cols).astype(np.float32), (rows, cols)).copy()
    mask = np.zeros((rows, cols), dtype=bool)
    mask[1000:1100, 500:900] = True
    return lin, ia, mask


def test_large_scene_tensors_and_views():
    import torch
    lin, ia, mask = large_scene()
    keep = lin.copy()
    exp = numpy_chain(lin, True, ia, mask, True)
    got = quiet(lib.prepare_image, lin, incidence_angle=ia, mask=mask, remove_spatial_mean=True)
    assert isinstance(got, np.ndarray)
    np.testing.assert_array_equal(got, exp)
    assert np.array_equal(lin.view(np.int32), keep.view(np.int32)), 'input modified'
    assert (got[np.isnan(lin) | (lin <= 0) | mask] == 0).all() and got.max() == 255
    # uint8 mask, dB alone
    np.testing.assert_array_equal(quiet(lib.prepare_image, lin, mask=mask.view(np.uint8)), numpy_chain(lin, True, None, mask))
    np.testing.assert_array_equal(quiet(lib.prepare_image, lin), numpy_chain(lin))
    # device tensors stay on the device and are left as they were
    tl, ti, tm = torch.from_numpy(lin).cuda(), torch.from_numpy(ia).cuda(), torch.from_numpy(mask).cuda()
    out = quiet(lib.prepare_image, tl, incidence_angle=ti, mask=tm, remove_spatial_mean=True)
    assert out.is_cuda and out.dtype == torch.uint8
    np.testing.assert_array_equal(out.cpu().numpy(), exp)
    assert np.array_equal(tl.cpu().numpy().view(np.int32), keep.view(np.int32)), 'device input modified'
    # strided views: aligned rows (16-byte path with a row stride) and misaligned ones (one pixel per lane)
    for sl in ((slice(10, 2010), slice(100, 2100)), (slice(3, 1503), slice(1, 2002))):
        exp_v = numpy_chain(lin[sl], True, ia[sl], mask[sl], True)
        out_v = quiet(lib.prepare_image, tl[sl], incidence_angle=ti[sl], mask=tm[sl], remove_spatial_mean=True)
        assert out_v.is_cuda
        np.testing.assert_array_equal(out_v.cpu().numpy(), exp_v, err_msg=str(sl))
        np.testing.assert_array_equal(quiet(lib.prepare_image, lin[sl], incidence_angle=ia[sl], mask=mask[sl], remove_spatial_mean=True), exp_v)
    # given limits instead of percentiles
    exp_l = so.get_uint8_image(numpy_chain(lin, True, ia, mask, True, floats=True), -6.0, 9.0, 10, 99)[0]
    np.testing.assert_array_equal(quiet(lib.prepare_image, tl, incidence_angle=ti, mask=tm, remove_spatial_mean=True, vmin=-6.0, vmax=9.0).cpu().numpy(), exp_l)


def test_degenerate_inputs():
    allnan = np.full((40, 50), np.nan, dtype=np.float32)
    assert (quiet(lib.prepare_image, allnan) == 0).all()
    assert (quiet(lib.prepare_image, np.zeros((64, 64), dtype=np.float32), mask=np.zeros((64, 64), dtype=bool)) == 0).all()
    one = np.full((1, 1), 0.5, dtype=np.float32)
    assert quiet(lib.prepare_image, one, vmin=-10.0, vmax=0.0).shape == (1, 1)
    with pytest.raises(NotImplementedError, match='float64'):
        lib.prepare_image(np.ones((4, 4)))
    import torch
    with pytest.raises(NotImplementedError, match='float64'):
        lib.prepare_image(torch.ones((4, 4), dtype=torch.float64, device='cuda'))
    with pytest.raises(NotImplementedError, match='stride'):
        lib.prepare_image(torch.ones((8, 8), device='cuda').t())
