"""CPU tests of the area-average downsampling (sea_ice_drift_amd.lib.resize_image, prepare_image_resized(factor=), ArrayNansat.resized,
include/sid_resize.h): properties of the specification (tests/resize_spec.py), the georeference of a resized ArrayNansat, the
argument checks that happen before any device work, and the exported symbols."""
import ctypes
import os
import re
from fractions import Fraction

import numpy as np
import pytest

from sea_ice_drift_amd import _capi, lib
from sea_ice_drift_amd.domain import ArrayNansat
from tests import resize_cases as rc
from tests import resize_spec as spec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

RATIOS = [(2, 1), (4, 2), (6, 2), (7, 3), (10, 3), (11, 9), (9, 4), (5, 2), (8, 8), (13, 1), (12, 8), (1, 1)]


def integers_f32(rows, cols, seed, limit=1 << 20):
    rng = np.random.default_rng(seed)
    return rng.integers(-limit + 1, limit, (rows, cols)).astype(np.float32)


# ---------------------------------------------------------------- the specification
@pytest.mark.parametrize('n,m', RATIOS + [(10000, 4000), (1 << 24, 3)])
def test_weights_cover_the_axis(n, m):
    if n > 100000:                                              # (the largest length: the first and last windows only)
        g = np.gcd(n, m)
        a, b = n // g, m // g
        assert (m - 1) * a // b >= 0 and -(-(m * a) // b) - 1 == n - 1
        return
    a, b, first, weights = spec.axis_weights(n, m)
    assert a * m == b * n and len(first) == len(weights) == m
    seen = np.zeros(n, dtype=np.int64)
    for j in range(m):
        assert sum(weights[j]) == a and all(1 <= w <= b for w in weights[j])
        assert first[j] == (j * a) // b and first[j] + len(weights[j]) - 1 == -(-((j + 1) * a) // b) - 1
        seen[first[j]: first[j] + len(weights[j])] += weights[j]
    assert (seen == b).all()                                    # every source pixel is handed out exactly once
    if n % m == 0:
        assert b == 1 and weights == [[1] * (n // m)] * m and first == list(range(0, n, n // m))


@pytest.mark.parametrize('k', [2, 3, 4])
def test_whole_ratio_is_the_block_mean(k):
    x = integers_f32(6 * k, 5 * k, k)                            # (integers below 2^20: the float64 block sum is exact in any order)
    block = x.reshape(6, k, 5, k).astype(np.float64).sum(axis=(1, 3))
    assert spec.same_bits(spec.resize_f32(x, 6, 5), (block / (k * k)).astype(np.float32))
    assert spec.same_bits(spec.resize_f32(x, 6, 5), spec.resize_f32_scalar(x, 6, 5))


@pytest.mark.parametrize('shape,out', [((7, 9), (3, 4)), ((10, 10), (3, 3)), ((11, 11), (9, 9)), ((6, 8), (3, 4)), ((5, 8), (2, 4)),
                                       ((13, 17), (1, 1)), ((9, 1), (4, 1))])
def test_ones_stay_ones_and_integers_give_the_exact_mean(shape, out):
    assert spec.same_bits(spec.resize_f32(np.ones(shape, dtype=np.float32), *out), np.ones(out, dtype=np.float32))
    x = integers_f32(shape[0], shape[1], shape[0] * 31 + shape[1])
    got = spec.resize_f32(x, *out)
    ar, br, rfirst, rweights = spec.axis_weights(shape[0], out[0])
    ac, bc, cfirst, cweights = spec.axis_weights(shape[1], out[1])
    for r in range(out[0]):
        for c in range(out[1]):
            S = sum(wr * wc * int(x[rfirst[r] + i, cfirst[c] + k]) for i, wr in enumerate(rweights[r]) for k, wc in enumerate(cweights[c]))
            assert got[r, c] == np.float32(float(Fraction(S, ar * ac))), (r, c)
    assert spec.same_bits(got, spec.resize_f32_scalar(x, *out))


@pytest.mark.parametrize('shape,out', [((7, 9), (3, 4)), ((10, 10), (3, 3)), ((11, 11), (9, 9)), ((6, 8), (3, 4)), ((9, 14), (1, 1))])
def test_uint8_is_the_exact_mean_rounded_half_up(shape, out):
    x = rc.bytes_(shape[0], shape[1], shape[0] + shape[1], zeros=0.05)
    ar, br, rfirst, rweights = spec.axis_weights(shape[0], out[0])
    ac, bc, cfirst, cweights = spec.axis_weights(shape[1], out[1])
    for zero_invalid in (True, False):
        got = spec.resize_u8(x, *out, zero_invalid=zero_invalid)
        assert spec.same_bits(got, spec.resize_u8_scalar(x, *out, zero_invalid=zero_invalid))
        for r in range(out[0]):
            for c in range(out[1]):
                win = [(wr * wc, int(x[rfirst[r] + i, cfirst[c] + k])) for i, wr in enumerate(rweights[r]) for k, wc in enumerate(cweights[c])]
                mean = Fraction(sum(w * v for w, v in win), ar * ac)
                exp = (mean + Fraction(1, 2)).__floor__()
                if zero_invalid and any(v == 0 for _, v in win):
                    exp = 0
                assert got[r, c] == exp, (r, c, zero_invalid)
                if all(v >= 1 for _, v in win):
                    assert got[r, c] >= 1
    assert spec.resize_u8(np.array([[1, 2], [1, 2]], dtype=np.uint8), 1, 1)[0, 0] == 2          # 1.5 rounds up
    assert spec.resize_u8(np.array([[1, 2], [1, 1]], dtype=np.uint8), 1, 1)[0, 0] == 1          # 1.25 does not


def test_every_shared_case_agrees_with_the_scalar_text():
    """The row-at-a-time specification the GPU tests compare with is the pixel-at-a-time text, on every small case."""
    for name in rc.NAMES:
        c = rc.BY_NAME[name]
        if c['image'].size > 400:
            continue
        fn = spec.resize_f32_scalar if c['image'].dtype == np.float32 else spec.resize_u8_scalar
        assert spec.same_bits(fn(c['image'], *rc.shape_of(c), **c['options']), rc.expected(name)), name


def test_nan_inf_and_minus_zero_in_the_specification():
    e = rc.expected('nan_in_2x2_block')
    assert np.isnan(e[0, 1]) and np.isnan(e).sum() == 1
    e = rc.expected('nan_in_shared_pixel')
    assert np.isnan(e[:2, :2]).all() and np.isnan(e).sum() == 4
    e = rc.expected('inf_and_minus_inf')
    assert np.isnan(e[0, 0]) and np.isposinf(e[1, 1]) and np.isfinite(e[0, 1])
    e = rc.expected('omit_some_and_all')
    assert np.isnan(e[1, 1]) and np.isnan(e).sum() == 1 and np.isposinf(e[2, 0])
    x = rc.BY_NAME['omit_some_and_all']['image']
    assert e[0, 0] == np.float32((float(x[0, 1]) + float(x[1, 0])) / 2.0)
    e = rc.expected('minus_zero_window')
    assert e[0, 0] == 0 and not np.signbit(e[0, 0]) and not np.signbit(e[1, 2])
    e = rc.expected('identity_5x7')
    assert e.tobytes() == rc.BY_NAME['identity_5x7']['image'].tobytes() and np.signbit(e[0, 0])


def test_shape_from_a_factor():
    assert lib.resize_shape(10000, 10000, 0.5) == (5000, 5000) == spec.out_shape(10000, 10000, 0.5)
    assert lib.resize_shape(10, 10, 0.3) == (3, 3) and lib.resize_shape(5, 8, 0.5) == (2, 4)
    assert lib.resize_shape(7, 9, 1) == (7, 9) and lib.resize_shape(7, 9, 0.1, out_shape=(3, 2)) == (3, 2)
    for rows, cols, f in ((1030, 2050, 0.5), (101, 77, 0.4), (33, 57, 0.7)):
        assert lib.resize_shape(rows, cols, f) == spec.out_shape(rows, cols, f) == (int(rows * f), int(cols * f))


# ---------------------------------------------------------------- ArrayNansat.resized (the georeference; the resize call is replaced)
def test_resized_keeps_the_corners(monkeypatch):
    calls = []

    def fake_resize(image, factor=0.5, out_shape=None, nan_policy='propagate', zero_invalid=True, device=0):
        calls.append((factor, zero_invalid, device))
        r, c = lib.resize_shape(image.shape[0], image.shape[1], factor)
        return np.full((r, c), 9, dtype=np.uint8)
    monkeypatch.setattr(lib, 'resize_image', fake_resize)
    img = np.full((40, 60), 7, dtype=np.uint8)
    for n in (ArrayNansat(img, origin=(10.0, 70.0), matrix=((0.01, 0.002), (-0.001, -0.004)), dst_scale=3.0),
              ArrayNansat.rotated(img, angle_deg=25.0, scale=0.003, origin=(-5.0, 80.0))):
        keep = (n.image.copy(), n.origin.copy(), n.matrix.copy())
        for factor in (0.5, 0.25, 0.3):
            m = n.resized(factor, device=0)
            assert m is not n and m.shape() == lib.resize_shape(40, 60, factor) and (m.image == 9).all()
            assert np.array_equal(m.origin, n.origin) and m.dst_scale == n.dst_scale
            sc, sr = 60 / m.shape()[1], 40 / m.shape()[0]
            assert np.array_equal(m.matrix, n.matrix @ np.diag([sc, sr]))
            for a, b in zip(m.get_corners(), n.get_corners()):
                np.testing.assert_allclose(a, b, rtol=1e-14, atol=0)
            lon, lat = m.transform_points(np.array([0.0, 3.5, m.shape()[1]]), np.array([0.0, 7.25, m.shape()[0]]), 0)
            col, row = m.transform_points(lon, lat, 1)
            np.testing.assert_allclose(col, [0.0, 3.5, m.shape()[1]], atol=1e-9)
            np.testing.assert_allclose(row, [0.0, 7.25, m.shape()[0]], atol=1e-9)
            # a reduced pixel is the same place as the block of full-resolution pixels under it
            np.testing.assert_allclose(m.transform_points(2.0, 3.0, 0), n.transform_points(2.0 * sc, 3.0 * sr, 0), rtol=1e-14)
        assert np.array_equal(n.image, keep[0]) and np.array_equal(n.origin, keep[1]) and np.array_equal(n.matrix, keep[2])
    assert calls[0] == (0.5, True, 0) and len(calls) == 6


# ---------------------------------------------------------------- argument errors, raised before any device work
def image(rows=20, cols=30, seed=0):
    return np.random.default_rng(seed).normal(-20.0, 4.0, (rows, cols)).astype(np.float32)


@pytest.mark.parametrize('factor', [1.5, 2, 0, 0.0, -0.5, float('nan'), float('inf'), -float('inf')])
def test_bad_factor(factor):
    for call in (lambda: lib.resize_image(image(), factor), lambda: lib.resize_image(image().astype(np.uint8), factor),
                 lambda: lib.prepare_image_resized(image(), factor=factor), lambda: lib.prepare_image_resized(image(), factor=factor),
                 lambda: lib.prepare_image_resized(image(), mask_invalid=True, factor=factor)):
        with pytest.raises(ValueError, match='factor'):
            call()


def test_output_dimension_of_zero():
    with pytest.raises(ValueError, match='dimension of 0'):
        lib.resize_image(image(1, 30), 0.5)
    with pytest.raises(ValueError, match='dimension of 0'):
        lib.resize_image(image(20, 30), 0.01)
    with pytest.raises(ValueError, match='dimension of 0'):
        lib.resize_image(image(), out_shape=(0, 5))
    with pytest.raises(ValueError, match='dimension of 0'):
        lib.prepare_image_resized(image(1, 30), factor=0.5)
    with pytest.raises(ValueError, match='downsampling only'):
        lib.resize_image(image(), out_shape=(21, 30))
    with pytest.raises(ValueError, match='out_shape'):
        lib.resize_image(image(), out_shape=5)


@pytest.mark.parametrize('dtype', [np.float64, np.float16, np.int16, np.int8, np.uint16, np.complex64, bool])
def test_dtype_refused_by_name(dtype):
    with pytest.raises(NotImplementedError, match=np.dtype(dtype).name):
        lib.resize_image(image().astype(dtype))


def test_options_of_the_other_dtype_and_shapes():
    with pytest.raises(ValueError, match='nan_policy'):
        lib.resize_image(image().astype(np.uint8), nan_policy='omit')
    with pytest.raises(ValueError, match='zero_invalid'):
        lib.resize_image(image(), zero_invalid=False)
    with pytest.raises(ValueError, match='nan_policy'):
        lib.resize_image(image(), nan_policy='skip')
    with pytest.raises(ValueError, match='2-D'):
        lib.resize_image(image().ravel())
    with pytest.raises(ValueError, match='2-D'):
        lib.resize_image(image()[None])


def test_mixed_tensor_and_array_refused():
    torch = pytest.importorskip('torch')
    with pytest.raises(ValueError, match='GPU'):
        lib.resize_image(torch.zeros(20, 30))
    with pytest.raises(NotImplementedError, match='float64'):
        lib.resize_image(torch.zeros(20, 30, dtype=torch.float64))
    with pytest.raises(TypeError, match='mix'):
        lib.prepare_image_resized(image(), incidence_angle=torch.zeros(20, 30), factor=0.5)
    with pytest.raises(TypeError, match='mix'):
        lib.prepare_image_resized(image(), mask=torch.zeros(10, 15, dtype=torch.bool), factor=0.5)
    with pytest.raises(TypeError, match='mix'):
        lib.prepare_image_resized(image(), mask=torch.zeros(10, 15, dtype=torch.bool), mask_invalid=True, factor=0.5)


def test_mask_refers_to_the_reduced_image():
    a = image()
    for call in (lib.prepare_image_resized, lambda *p, **k: lib.prepare_image_resized(*p, mask_invalid=True, **k)):
        with pytest.raises(ValueError, match=r'mask.*\(20, 30\).*\(10, 15\)'):
            call(a, mask=np.zeros((20, 30), dtype=bool), factor=0.5)
    with pytest.raises(ValueError, match='incidence_angle'):                   # (the incidence angle is full resolution)
        lib.prepare_image_resized(a, incidence_angle=image(10, 15), factor=0.5)
    with pytest.raises(ValueError, match=r'\(20, 30\)'):                       # (without a resize the mask has the image's shape, as before)
        lib.prepare_image(a, mask=np.zeros((10, 15), dtype=bool))


def test_c_abi_argument_errors_without_a_device():
    L = _capi.lib()
    err = lambda: L.sid_resize_last_error().decode()                            # noqa: E731
    p = ctypes.c_void_p(4096)                                                   # (never dereferenced: the checks come first)
    for fn in (L.sid_resize_f32, L.sid_resize_u8):
        assert fn(None, 4, 4, 4, p, 2, 2, 2, 0, None) == -1 and 'null source' in err()
        assert fn(p, 4, 4, 4, None, 2, 2, 2, 0, None) == -1 and 'null destination' in err()
        assert fn(p, 4, 4, 4, p, 5, 2, 2, 0, None) == -1 and 'exceeds' in err()
        assert fn(p, 4, 4, 4, p, 2, 5, 5, 0, None) == -1 and 'exceeds' in err()
        assert fn(p, 4, 4, 4, p, 0, 2, 2, 0, None) == -1 and 'output shape' in err()
        assert fn(p, 0, 4, 4, p, 1, 1, 1, 0, None) == -1 and 'image shape' in err()
        assert fn(p, 4, 4, 3, p, 2, 2, 2, 0, None) == -1 and 'stride' in err()
        assert fn(p, 4, 4, 4, p, 2, 2, 1, 0, None) == -1 and 'stride' in err()
        assert fn(p, (1 << 24) + 1, 4, 4, p, 2, 2, 2, 0, None) == -4 and '2^24' in err()
    apply_, sub = L.sid_resize_prep_apply, L.sid_resize_prep_subsample
    assert apply_(None, 4, 4, 4, None, 0, None, 0, 1, 0.0, None, p, 2, 2, 2, None) == -1 and 'null image' in err()
    assert apply_(p, 4, 4, 4, None, 0, None, 0, 1, 0.0, None, None, 2, 2, 2, None) == -1 and 'null output' in err()
    assert apply_(p, 4, 4, 4, None, 0, None, 0, 1, 0.0, None, p, 5, 2, 2, None) == -1 and 'exceeds' in err()
    assert apply_(p, 4, 4, 4, p, 3, None, 0, 1, 0.0, None, p, 2, 2, 2, None) == -1 and 'incidence angle' in err()
    assert apply_(p, 4, 4, 4, None, 0, p, 1, 1, 0.0, None, p, 2, 2, 2, None) == -1 and 'mask' in err()
    assert sub(None, 4, 4, 4, None, 0, None, 0, 1, 0.0, 50, 2, 2, p, None) == -1 and 'null image' in err()
    assert sub(p, 4, 4, 4, None, 0, None, 0, 1, 0.0, 50, 2, 2, None, None) == -1 and 'null output' in err()
    assert sub(p, 4, 4, 4, None, 0, None, 0, 1, 0.0, 0, 2, 2, p, None) == -1 and 'step' in err()
    assert sub(p, 4, 4, 4, None, 0, None, 0, 1, 0.0, 50, 2, 5, p, None) == -1 and 'exceeds' in err()
    with pytest.raises(_capi.SidPmError) as e:
        _capi.resize(0, 'float32', 4, 4, 4, 4096, 2, 2, 2, False)
    assert e.value.code == -1 and 'null source' in str(e.value)


# ---------------------------------------------------------------- symbols
def resize_header_functions():
    src = open(os.path.join(ROOT, 'include', 'sid_resize.h')).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    return sorted(set(re.findall(r'\b(sid_resize_[a-z_0-9]+)\s*\(', src)))


def test_resize_symbols_exported():
    assert resize_header_functions() == sorted(_capi.RESIZE_SYMBOLS)
    assert os.path.exists(_capi.LIB_PATH), 'build with __graft_entry__.build() first'
    so = ctypes.CDLL(_capi.LIB_PATH)
    for name in _capi.RESIZE_SYMBOLS:
        assert hasattr(so, name), name
    src = open(os.path.join(ROOT, 'include', 'sid_resize.h')).read()
    assert int(re.search(r'#define SID_RESIZE_MAX_DIM (\d+)', src).group(1)) == _capi.RESIZE_MAX_DIM == lib.RESIZE_MAX_DIM == spec.MAX_DIM


def test_signatures():
    import inspect
    assert list(inspect.signature(lib.resize_image).parameters) == ['image', 'factor', 'out_shape', 'nan_policy', 'zero_invalid', 'device']
    d = {k: p.default for k, p in inspect.signature(lib.resize_image).parameters.items() if p.default is not inspect.Parameter.empty}
    assert d == dict(factor=0.5, out_shape=None, nan_policy='propagate', zero_invalid=True, device=0)
    assert list(inspect.signature(ArrayNansat.resized).parameters) == ['self', 'factor', 'device']
    base = inspect.signature(lib.prepare_image_masked)
    sig = inspect.signature(lib.prepare_image_resized)
    assert list(sig.parameters) == ['image', 'factor'] + list(base.parameters)[1:] and sig.parameters['factor'].default == 0.5
    assert all(sig.parameters[k].default == p.default for k, p in base.parameters.items())
    assert 'factor' not in base.parameters and 'factor' not in inspect.signature(lib.prepare_image).parameters
