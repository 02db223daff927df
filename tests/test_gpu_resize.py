"""GPU tests of the area-average downsampling (include/sid_resize.h; sea_ice_drift_amd.lib.resize_image, prepare_image_resized(factor=),
ArrayNansat.resized): every shared case (tests/resize_cases.py) bit for bit against the specification (tests/resize_spec.py)
through the NumPy route and the tensor route, the fused front of prepare_image against the two-call composition, and the
resized ArrayNansat."""
import contextlib
import io
import warnings

import numpy as np
import pytest

from sea_ice_drift_amd import _capi, lib
from sea_ice_drift_amd.domain import ArrayNansat
from tests import resize_cases as rc
from tests import resize_spec as spec

pytestmark = pytest.mark.gpu
HH_FACTOR = -0.27


@pytest.fixture
def no_host_copies(monkeypatch):
    """Any move of a tensor to the host raises while the fixture is active."""
    torch = pytest.importorskip('torch')

    def refuse(*a, **k):
        raise AssertionError('a tensor was copied to the host')
    for name in ('cpu', 'numpy', 'tolist', 'item', '__array__'):
        monkeypatch.setattr(torch.Tensor, name, refuse)
    return torch


def _host(tensor):
    """A device tensor's values through a copy into a host tensor and DLPack (the fixture refuses .cpu() and .numpy())."""
    import torch
    out = torch.empty(tuple(tensor.shape), dtype=tensor.dtype)
    out.copy_(tensor)
    return np.from_dlpack(out).copy()


def on_device(torch, a, strided=False):
    """`a` on the device; `strided`: as a view with padded rows that starts 3 elements into its row - no row start is 16-byte
    aligned, so the one-pixel-per-lane kernels run."""
    a = np.ascontiguousarray(a)
    if not strided:
        return torch.from_numpy(a).cuda()
    wide = torch.zeros((a.shape[0], a.shape[1] + 7), dtype=torch.from_numpy(a[:0]).dtype, device='cuda')
    view = wide[:, 3:3 + a.shape[1]]
    view.copy_(torch.from_numpy(a))
    return view


def poison_pool(torch):
    """Fill blocks of the caching allocator with a pattern and free them, so that torch.empty on the same stream hands out
    poisoned memory for the outputs."""
    for dtype, val in ((torch.float32, -12345.678), (torch.uint8, 113)):
        blocks = [torch.full((1 << 16,), val, dtype=dtype, device='cuda') for _ in range(4)]
        del blocks


def quiet(fn, *a, **k):
    with contextlib.redirect_stdout(io.StringIO()), warnings.catch_warnings(), np.errstate(all='ignore'):
        warnings.simplefilter('ignore')
        return fn(*a, **k)


def check(got, name, how):
    exp = rc.expected(name)
    assert got.shape == exp.shape and got.dtype == exp.dtype, (name, how, got.shape, got.dtype)
    if not spec.same_bits(got, exp):
        g, e = got.astype(np.float64), exp.astype(np.float64)
        bad = np.argwhere(~(((g == e) & (np.signbit(g) == np.signbit(e))) | (np.isnan(g) & np.isnan(e))))
        r, c = bad[0]
        raise AssertionError('%s, %s: %d pixels differ, first at (%d, %d): got %r, expected %r'
                             % (name, how, len(bad), r, c, got[r, c], exp[r, c]))


# ---------------------------------------------------------------- the cases
@pytest.mark.parametrize('name', rc.NAMES)
def test_case_numpy_route(name):
    c = rc.BY_NAME[name]
    keep = c['image'].copy()
    first = lib.resize_image(c['image'], **rc.call_kwargs(c))
    assert isinstance(first, np.ndarray) and first is not c['image'] and not np.shares_memory(first, c['image'])
    check(first, name, 'numpy route')
    assert c['image'].tobytes() == keep.tobytes(), 'the input was modified'
    assert first.tobytes() == lib.resize_image(c['image'], **rc.call_kwargs(c)).tobytes(), 'two runs differ'


@pytest.mark.parametrize('name', rc.NAMES)
def test_case_tensor_route(no_host_copies, name):
    torch = no_host_copies
    c = rc.BY_NAME[name]
    runs = []
    for strided in (True, False, True, False):
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            t = on_device(torch, c['image'], strided)
            poison_pool(torch)
            got = lib.resize_image(t, **rc.call_kwargs(c))
        s.synchronize()
        assert got.is_cuda and got.data_ptr() != t.data_ptr() and got.is_contiguous()
        assert _host(t).tobytes() == c['image'].tobytes(), 'the input was modified'
        runs.append(_host(got))
        check(runs[-1], name, 'tensor route, strided view' if strided else 'tensor route')
    assert runs[0].tobytes() == runs[2].tobytes() and runs[1].tobytes() == runs[3].tobytes(), 'two runs differ'


def padded(torch, rows, cols, dtype, fill):
    """(wide, view): a rows x cols view whose rows start 16-byte aligned inside a wider buffer filled with `fill`."""
    pad = 16 if dtype == torch.uint8 else 4
    wide = torch.full((rows, -(-cols // 16) * 16 + 2 * pad), fill, dtype=dtype, device='cuda')
    return wide, wide[:, pad:pad + cols]


@pytest.mark.parametrize('name', ['half_w24', 'quarter_w48', 'half_w514', 'frac_11x11_to_9x9', 'u8_half_w32', 'u8_half_w44', 'u8_half_w1072',
                                  'u8_frac_7x7_to_3x3'])
def test_device_entry_point_with_padded_rows(no_host_copies, name):
    """sid_resize_* read from and write into rows longer than the image, every row start aligned (the 16-byte kernels where the
    ratio allows; for a uint8 width of 44 with single columns at the end), and leave the padding alone."""
    torch = no_host_copies
    c = rc.BY_NAME[name]
    ro, co = rc.shape_of(c)
    img = torch.from_numpy(c['image'])
    _, src = padded(torch, img.shape[0], img.shape[1], img.dtype, 0)
    src.copy_(img)
    wide, dst = padded(torch, ro, co, img.dtype, 113)
    dtype = str(img.dtype).replace('torch.', '')
    for _ in range(2):
        _capi.resize(src.data_ptr(), dtype, src.shape[0], src.shape[1], src.stride(0), dst.data_ptr(), ro, co, dst.stride(0),
                     dtype == 'uint8', torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    check(_host(dst), name, 'device entry point')
    w, pad = _host(wide), (wide.shape[1] - -(-co // 16) * 16) // 2
    assert (w[:, :pad] == 113).all() and (w[:, pad + co:] == 113).all()


# ---------------------------------------------------------------- the fused front of prepare_image
def scene(rows, cols, seed):
    """(linear sigma0, incidence angle) at full resolution: several decades, NaN, inf, zeros and negative values."""
    rng = np.random.default_rng(seed)
    r, c = np.meshgrid(np.arange(rows, dtype=np.float64), np.arange(cols, dtype=np.float64), indexing='ij')
    db = -18.0 - 9.0 * c / cols + 2.0 * (r / rows) ** 2 + 4.0 * rng.standard_normal((rows, cols))
    lin = (10.0 ** (db / 10.0) * 10.0 ** rng.uniform(-2.0, 1.0, (rows, cols))).astype(np.float32)
    u = rng.random((rows, cols))
    lin[u < 0.003] = np.nan
    lin[(u >= 0.003) & (u < 0.0032)] = np.inf
    lin[(u >= 0.004) & (u < 0.008)] = 0.0
    lin[(u >= 0.008) & (u < 0.012)] *= np.float32(-1.0)
    lin[:2, :] = 0.0
    lin[:, :2] = 0.0
    lin[rows // 2, cols // 2] = np.inf
    ia = (20.0 + 26.0 * c / cols + 0.3 * r / rows).astype(np.float32)
    return lin, ia


def reduced_mask(shape, seed):
    rng = np.random.default_rng(seed)
    mask = rng.random(shape) < 0.02
    mask[shape[0] // 2: shape[0] // 2 + max(1, shape[0] // 6), shape[1] // 5: shape[1] // 5 + max(1, shape[1] // 4)] = True
    return mask


COEFFS = np.array([-0.031, 1.7e-4, 0.012, -2.3e-5, 6.1e-5, -21.5])
FUSED = [((64, 96), 0.5), ((64, 96), 0.25), ((101, 77), 0.5), ((101, 77), 0.4), ((8200, 8), 0.5), ((8202, 3), 0.5)]


def fused_and_composed(conv, host, shape, factor, steps, seed):
    """(fused, composed): float32 working image and uint8 image of prepare_image_resized(factor=) and of the two-call composition."""
    lin, ia = scene(shape[0], shape[1], seed)
    out_shape = lib.resize_shape(shape[0], shape[1], factor)
    kw = dict(dB=True)
    if steps == 'full':
        kw.update(mask=conv(reduced_mask(out_shape, seed + 1)), remove_spatial_mean=True, spatial_mean_coeffs=COEFFS)
    elif steps == 'fit':
        kw.update(mask=conv(reduced_mask(out_shape, seed + 1)), remove_spatial_mean=True)
    hh = steps != 'db'
    t, a = conv(lin), conv(ia) if hh else None
    small_t, small_a = lib.resize_image(t, factor), lib.resize_image(a, factor) if hh else None
    work = lambda img, ang, f: quiet(lib._prep_apply, img, ang, kw.get('mask'), True, HH_FACTOR, 'mask' in kw,       # noqa: E731
                                     kw.get('spatial_mean_coeffs'), 0, f)[0]
    fused = (work(t, a, factor), quiet(lib.prepare_image_resized, t, incidence_angle=a, factor=factor, **kw))
    composed = (work(small_t, small_a, 1), quiet(lib.prepare_image, small_t, incidence_angle=small_a, **kw))
    staged = quiet(lib.get_uint8_image, fused[0], None, None, 10, 99)
    return [tuple(host(q) for q in pair) for pair in (fused, composed)] + [host(staged)], out_shape


@pytest.mark.parametrize('steps', ['db', 'full'])
@pytest.mark.parametrize('shape,factor', FUSED)
def test_fused_prepare_equals_the_two_calls(shape, factor, steps):
    (fused, composed, staged), out_shape = fused_and_composed(lambda a: a, lambda a: a if isinstance(a, np.ndarray) else a.cpu().numpy(),
                                                               shape, factor, steps, 700 + shape[0])
    assert fused[0].shape == fused[1].shape == out_shape and fused[0].dtype == np.float32 and fused[1].dtype == np.uint8
    assert spec.same_bits(fused[0], composed[0]), 'float32 working image: %d pixels differ' % (
        ~((fused[0] == composed[0]) | (np.isnan(fused[0]) & np.isnan(composed[0])))).sum()
    assert fused[1].tobytes() == composed[1].tobytes() == staged.tobytes()
    assert np.isfinite(fused[0]).sum() > 0.5 * fused[0].size and len(np.unique(fused[1])) > (20 if fused[1].size > 1000 else 3)
    if steps == 'full':
        assert (fused[1][reduced_mask(out_shape, 700 + shape[0] + 1)] == 0).all()


@pytest.mark.parametrize('shape,factor', [((120, 160), 0.5), ((203, 211), 0.5)])
def test_fused_prepare_on_tensors_and_with_the_host_fit(shape, factor):
    """The tensor route (strided views: the one-pixel-per-lane kernels; then aligned tensors) with the detrend fitted on the
    host to the [::50, ::50] subsample of the reduced image - 2 x 2 samples of a 60 x 80 image, 3 x 3 of a 101 x 105 one - which the fused subsample
    pass delivers from the full-resolution planes."""
    import torch
    host = lambda t: t.cpu().numpy()                                                  # noqa: E731
    out_shape = lib.resize_shape(shape[0], shape[1], factor)
    sub_shape = (-(-out_shape[0] // 50), -(-out_shape[1] // 50))
    assert sub_shape[0] > 1 and sub_shape[1] > 1
    lin, ia = scene(shape[0], shape[1], 900)
    for strided in (True, False):
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            poison_pool(torch)
            (fused, composed, staged), _ = fused_and_composed(lambda a: on_device(torch, a, strided), host, shape, factor, 'fit', 900)
            # the subsample itself, from the full-resolution planes and from the reduced ones
            t, a, mk = [on_device(torch, q, strided) for q in (lin, ia, reduced_mask(out_shape, 901).view(np.uint8))]
            subs = [lib._prep_subsample(t, a, mk, True, HH_FACTOR, s, out_shape),
                    lib._prep_subsample(lib.resize_image(t, factor), lib.resize_image(a, factor), mk, True, HH_FACTOR, s)]
        s.synchronize()
        assert spec.same_bits(fused[0], composed[0]) and fused[1].tobytes() == composed[1].tobytes() == staged.tobytes()
        assert subs[0].shape == sub_shape and spec.same_bits(subs[0], subs[1]) and np.isfinite(subs[0]).any()


def test_masked_preparation_with_a_factor():
    """prepare_image_resized(mask_invalid=True, factor=) is the masked preparation of the two resized planes: the mask and the
    water mask refer to the reduced image."""
    lin, ia = scene(64, 96, 1200)
    rng = np.random.default_rng(1201)
    wm = rng.integers(0, 3, (8, 12)).astype(np.uint8)
    mask = reduced_mask((32, 48), 1202)
    for kw in (dict(), dict(incidence_angle=True, mask=mask, watermask=wm, remove_spatial_mean=True, spatial_mean_coeffs=COEFFS)):
        hh = kw.pop('incidence_angle', False)
        got = quiet(lib.prepare_image_resized, lin, incidence_angle=ia if hh else None, mask_invalid=True, factor=0.5, **kw)
        exp = quiet(lib.prepare_image_masked, lib.resize_image(lin, 0.5), incidence_angle=lib.resize_image(ia, 0.5) if hh else None,
                    mask_invalid=True, **kw)
        assert got.shape == (32, 48) and got.dtype == np.uint8 and got.tobytes() == exp.tobytes()
        assert (got[0] == 0).all() and len(np.unique(got)) > 20
    assert quiet(lib.prepare_image_resized, lin).tobytes() == quiet(lib.prepare_image, lib.resize_image(lin, 0.5)).tobytes()   # factor=0.5
    assert quiet(lib.prepare_image_resized, lin, 1).tobytes() == quiet(lib.prepare_image, lin).tobytes()


# ---------------------------------------------------------------- ArrayNansat.resized
def test_resized_array_nansat():
    img = rc.bytes_(40, 60, 1300)
    img[10:14, 20:29] = 0                                       # a zero block: rows 10..13, columns 20..28
    n = ArrayNansat(img, origin=(10.0, 70.0), matrix=((0.01, 0.002), (-0.001, -0.004)))
    keep = img.copy()
    for factor in (0.5, 0.3):
        m = n.resized(factor)
        shape = lib.resize_shape(40, 60, factor)
        assert spec.same_bits(m[1], spec.resize_u8(img, *shape, zero_invalid=True))
        for a, b in zip(m.get_corners(), n.get_corners()):
            np.testing.assert_allclose(a, b, rtol=1e-14, atol=0)
        assert (m[1] == 0).sum() > 0 and ((m[1] == 0) == (spec.resize_u8((img == 0).astype(np.uint8) * 255, *shape, zero_invalid=False) > 0)).all()
    assert (n.resized(0.5)[1][5:7, 10:15] == 0).all() and (n.resized(0.5)[1] == 0).sum() == 10
    assert n.image is img and img.tobytes() == keep.tobytes()
