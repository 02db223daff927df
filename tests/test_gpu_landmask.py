"""GPU parity of the invalid-pixel mask (include/sid_mask.h; sea_ice_drift_amd.lib.zoom_landmask, invalid_mask, get_invalid_mask
and prepare_image_masked(mask_invalid=, watermask=); replaces get_invalid_mask, lib.py:342-373): every byte against SciPy called here,
every mask against the reference's own outputs (g12 fixture)."""
import contextlib
import io
import os
import warnings

import numpy as np
import pytest

from sea_ice_drift_amd import lib
from tests.golden import make_golden_landmask as ml
from tests.golden import make_golden_prepare as mg

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
# a downscale whose coefficient patch exceeds the kernel's LDS budget (coefficients read from global memory), and an upscale by
# 2.5 of a raster wide enough for the same on aligned rows
WIDE = {'wide_down': ((8, 2000), (20, 600)), 'wide_up': ((60, 900), (150, 2252))}


def scipy_zoom(wm, shape):
    from scipy.ndimage import maximum_filter, zoom
    wm = wm.copy()
    wm[wm > 2] = 2
    return zoom(maximum_filter(wm, 3), np.array(shape) / np.array(wm.shape))


def quiet(fn, *a, **k):
    with contextlib.redirect_stdout(io.StringIO()), warnings.catch_warnings(), np.errstate(all='ignore'):
        warnings.simplefilter('ignore')
        return fn(*a, **k)


@pytest.fixture(scope='module')
def g12():
    return np.load(os.path.join(HERE, 'golden', 'g12_invalid_mask.npz'))


@pytest.fixture(scope='module')
def cases():
    """name -> (image, water mask, SciPy's zoomed mask); computed once, never written to."""
    out = {}
    for name in ml.CASES:
        img, wm = ml.inputs(name)
        out[name] = (img, wm, scipy_zoom(wm, img.shape))
    for name, (ws, shape) in WIDE.items():
        wm = ml.watermask(ws, 99)
        out[name] = (ml.image(shape, 99), wm, scipy_zoom(wm, shape))
    for v in out.values():
        for a in v:
            a.setflags(write=False)
    return out


def test_inputs_meet_the_quirks(cases):
    """Conditions on the inputs, on the SciPy side: the cases hold 0, 1, 2 AND the overshoot 3, and the 'outside' cases have an
    all-zero last row / column beside one that is not."""
    seen = set()
    for name in ml.CASES:
        seen |= set(np.unique(cases[name][2]).tolist())
    assert seen >= {0, 1, 2, 3}
    z = cases['lastrow'][2]
    assert not z[-1].any() and z[-2].any()
    z = cases['lastcol'][2]
    assert not z[:, -1].any() and z[:, -2].any()


@pytest.mark.parametrize('name', ml.CASES + tuple(WIDE))
def test_zoom_landmask_equals_scipy_in_every_byte(cases, g12, name):
    import torch
    img, wm, exp = cases[name]
    keep = wm.copy()
    got = lib.zoom_landmask(wm, img.shape)
    assert isinstance(got, np.ndarray) and got.dtype == np.uint8
    np.testing.assert_array_equal(got, exp)
    assert np.array_equal(wm, keep), 'input modified'
    t = torch.from_numpy(wm.copy()).cuda()
    got_t = lib.zoom_landmask(t, img.shape)
    assert got_t.is_cuda and got_t.dtype == torch.uint8
    np.testing.assert_array_equal(got_t.cpu().numpy(), exp)
    assert np.array_equal(t.cpu().numpy(), keep), 'device input modified'
    if name == ml.WMZ_CASE:
        np.testing.assert_array_equal(got, g12[name + '_wmz'])


@pytest.mark.parametrize('name', ml.CASES + tuple(WIDE))
def test_invalid_mask_equals_the_reference(cases, g12, name):
    import torch
    img, wm, zoomed = cases[name]
    exp = ml.unpack(g12, name + '_mask', img.shape) if name in ml.CASES else (zoomed == 2) | np.isnan(img) | np.isinf(img)
    assert np.array_equal(exp, (zoomed == 2) | np.isnan(img) | np.isinf(img))
    keep_img, keep_wm = img.copy(), wm.copy()
    got = lib.invalid_mask(img, wm)
    assert isinstance(got, np.ndarray) and got.dtype == np.bool_
    np.testing.assert_array_equal(got, exp)
    ti, tw = torch.from_numpy(img.copy()).cuda(), torch.from_numpy(wm.copy()).cuda()
    got_t = lib.invalid_mask(ti, tw)
    assert got_t.is_cuda and got_t.dtype == torch.bool
    np.testing.assert_array_equal(got_t.cpu().numpy(), exp)
    assert np.array_equal(img.view(np.int32), keep_img.view(np.int32)) and np.array_equal(wm, keep_wm), 'input modified'
    assert np.array_equal(ti.cpu().numpy().view(np.int32), keep_img.view(np.int32)) and np.array_equal(tw.cpu().numpy(), keep_wm)
    # no water mask: the non-finite pixels alone
    nonfinite = np.isnan(img) | np.isinf(img)
    np.testing.assert_array_equal(lib.invalid_mask(img), nonfinite)
    np.testing.assert_array_equal(lib.invalid_mask(ti, None).cpu().numpy(), nonfinite)
    if img.size > 200:
        assert np.isnan(img).any() and np.isposinf(img).any() and np.isneginf(img).any()


@pytest.mark.parametrize('name', ['odd', 'even', 'lastcol', 'wide_down'])
def test_strided_views(cases, name):
    """Image, water mask and mask output as views of larger parents: row starts that are 16-byte aligned (offset 16 of a parent
    whose width is a multiple of 4) and row starts that are not (offset 3)."""
    import torch
    from sea_ice_drift_amd import _capi
    img, wm, zoomed = cases[name]
    H, W = img.shape
    exp = (zoomed == 2) | np.isnan(img) | np.isinf(img)
    for off, pad in ((16, 48), (3, 9)):
        parent = torch.full((H + 7, W + pad), float('nan'), dtype=torch.float32, device='cuda')
        view = parent[5:5 + H, off:off + W]
        view.copy_(torch.from_numpy(img.copy()))
        wparent = torch.full((wm.shape[0] + 2, wm.shape[1] + 5), 2, dtype=torch.uint8, device='cuda')
        wview = wparent[1:1 + wm.shape[0], 2:2 + wm.shape[1]]
        wview.copy_(torch.from_numpy(wm.copy()))
        assert not view.is_contiguous() and not wview.is_contiguous()
        np.testing.assert_array_equal(lib.invalid_mask(view, wview).cpu().numpy(), exp, err_msg='%s offset %d' % (name, off))
        # the C ABI writing into views of larger planes: nothing outside the views is touched
        mparent = torch.full((H + 7, W + pad), 7, dtype=torch.uint8, device='cuda')
        zparent = torch.full((H + 7, W + pad), 9, dtype=torch.uint8, device='cuda')
        mview, zview = mparent[5:5 + H, off:off + W], zparent[5:5 + H, off:off + W]
        work = torch.empty(_capi.mask_workspace_bytes(*wm.shape), dtype=torch.uint8, device='cuda')
        _capi.mask_invalid(lib._plane(wview), wm.shape[0], wm.shape[1], H, W, work.data_ptr(), lib._plane(view), False, None, 0.0,
                           lib._plane(mview), lib._plane(zview), torch.cuda.current_stream().cuda_stream)
        np.testing.assert_array_equal(mview.cpu().numpy(), exp.view(np.uint8))
        np.testing.assert_array_equal(zview.cpu().numpy(), zoomed)
        mparent[5:5 + H, off:off + W] = 7
        zparent[5:5 + H, off:off + W] = 9
        assert bool((mparent == 7).all()) and bool((zparent == 9).all())


def test_get_invalid_mask_protocol(cases, g12, capsys):
    import torch
    img, wm, _ = cases['odd']
    exp = ml.unpack(g12, 'odd_mask', img.shape)
    scene = ml.Scene(wm.copy())
    got = lib.get_invalid_mask(img, scene, ml.LANDMASK_BORDER)
    assert (scene.resized, scene.undone, scene.factor) == (1, 1, 1. / 20)
    assert [scene.resized, scene.undone, 1.0 / scene.factor] == g12['odd_calls'].tolist()
    assert got.dtype == np.bool_
    np.testing.assert_array_equal(got, exp)
    assert np.array_equal(scene.wm, wm), 'raster modified'
    assert 'Cannot add landmask' not in capsys.readouterr().out
    # a device image with the NumPy raster a scene returns
    scene = ml.Scene(wm.copy())
    got_t = lib.get_invalid_mask(torch.from_numpy(img.copy()).cuda(), scene, ml.LANDMASK_BORDER)
    assert got_t.is_cuda and (scene.resized, scene.undone) == (1, 1)
    np.testing.assert_array_equal(got_t.cpu().numpy(), exp)
    capsys.readouterr()
    # watermask() raises: the message, undo all the same, no land
    scene = ml.Scene(None)
    got = lib.get_invalid_mask(img, scene, ml.LANDMASK_BORDER)
    assert (scene.resized, scene.undone, scene.factor) == (1, 1, 1. / 20)
    assert capsys.readouterr().out == 'Cannot add landmask\n'
    np.testing.assert_array_equal(got, ml.unpack(g12, 'nowm_mask', img.shape))


@pytest.mark.parametrize('scene', list(ml.PREP_SCENES))
def test_prepare_image_mask_invalid_equals_the_reference_mask(g12, scene):
    """prepare_image_masked(mask_invalid=True, watermask=wm) is prepare_image(mask=<the reference's get_invalid_mask of the image after
    dB / HH>) in every uint8 pixel: with and without dB, HH and detrend, NumPy and (for the strided 'view' scene) device views;
    with watermask=None it is prepare_image(mask=isnan | isinf of that image); a caller's mask is ORed in."""
    import torch
    _, _, _, user_mask = mg.inputs(scene)
    for k in range(4):
        src, dB, ia, after, wm = ml.prep_inputs(scene, k)
        ref = ml.unpack(g12, 'prep_%s_%d' % (scene, k), after.shape)
        nonfinite = np.isnan(after) | np.isinf(after)
        assert (ref & ~nonfinite).any() and (nonfinite & ~ref).sum() == 0
        keep = src.copy()
        for detrend in (False, True):
            common = dict(dB=dB, incidence_angle=ia, remove_spatial_mean=detrend)
            exp = quiet(lib.prepare_image, src, mask=ref, **common)
            got = quiet(lib.prepare_image_masked, src, mask_invalid=True, watermask=wm, **common)
            assert isinstance(got, np.ndarray) and got.dtype == np.uint8
            np.testing.assert_array_equal(got, exp, err_msg='%s %d detrend %s' % (scene, k, detrend))
            assert (got[ref] == 0).all()
            exp_nf = quiet(lib.prepare_image, src, mask=nonfinite, **common)
            np.testing.assert_array_equal(quiet(lib.prepare_image_masked, src, mask_invalid=True, **common), exp_nf)
            if not detrend:
                exp_or = quiet(lib.prepare_image, src, mask=ref | user_mask, **common)
                np.testing.assert_array_equal(quiet(lib.prepare_image_masked, src, mask_invalid=True, watermask=wm, mask=user_mask, **common), exp_or)
            if scene == 'view':                   # strided device views of the parents
                ts = torch.from_numpy(np.ascontiguousarray(src.base)).cuda()[mg.VIEW]
                ti = None if ia is None else torch.from_numpy(np.ascontiguousarray(ia.base)).cuda()[mg.VIEW]
                assert not ts.is_contiguous()
                out = quiet(lib.prepare_image_masked, ts, dB=dB, incidence_angle=ti, remove_spatial_mean=detrend, mask_invalid=True,
                            watermask=torch.from_numpy(wm.copy()).cuda())
                assert out.is_cuda
                np.testing.assert_array_equal(out.cpu().numpy(), exp)
        assert np.array_equal(src.view(np.int32), keep.view(np.int32)), 'input modified'


def test_infinities_become_invalid_only_with_mask_invalid():
    """get_n masks +-inf before the percentiles (mask_invalid is its default); without the keyword prepare_image leaves them to the
    staging step as before - and so does prepare_image_masked with its defaults."""
    img = np.random.default_rng(3).normal(-20.0, 4.0, (64, 80)).astype(np.float32)
    img[5, 5] = np.inf
    img[6, 6] = -np.inf
    masked = img.copy()
    masked[5, 5] = masked[6, 6] = np.nan
    got = quiet(lib.prepare_image_masked, img, dB=False, mask_invalid=True)
    np.testing.assert_array_equal(got, quiet(lib.prepare_image, masked, dB=False))
    assert got[5, 5] == 0 and got[6, 6] == 0
    np.testing.assert_array_equal(quiet(lib.prepare_image_masked, img, dB=False), quiet(lib.prepare_image, img, dB=False))
