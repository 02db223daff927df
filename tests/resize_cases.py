"""Named small cases of the area-average downsampling, shared by tests/test_resize_host.py and tests/test_gpu_resize.py.
Each case: the input array, how the output shape is asked for (``factor`` or ``out_shape``), the options, and - computed once
and left unchanged - the specification's result (tests/resize_spec.py)."""
import numpy as np

from tests import resize_spec as spec

NAN, INF = np.float32(np.nan), np.float32(np.inf)


def floats(rows, cols, seed):
    """SAR-like positive float32 with a wide spread, a few zeros and negative values."""
    rng = np.random.default_rng(seed)
    x = (10.0 ** rng.normal(-2.0, 0.8, (rows, cols))).astype(np.float32)
    u = rng.random((rows, cols))
    x[u < 0.03] = 0.0
    x[(u >= 0.03) & (u < 0.06)] *= np.float32(-1.0)
    return x


def finite_bit_patterns(rows, cols, seed):
    """Random float32 bit patterns with the NaN / inf patterns removed: every exponent, both signs, subnormals."""
    rng = np.random.default_rng(seed)
    bits = rng.integers(0, 1 << 32, (rows, cols), dtype=np.uint64).astype(np.uint32)
    bad = (bits & np.uint32(0x7f800000)) == np.uint32(0x7f800000)
    bits[bad] &= np.uint32(0xbfffffff)                           # (clears one exponent bit: finite)
    return bits.view(np.float32)


def bytes_(rows, cols, seed, zeros=0.0):
    rng = np.random.default_rng(seed)
    x = rng.integers(1, 256, (rows, cols), dtype=np.int64).astype(np.uint8)
    if zeros:
        x[rng.random((rows, cols)) < zeros] = 0
    return x


def _case(name, image, factor=None, out_shape=None, **options):
    assert (factor is None) != (out_shape is None)
    return dict(name=name, image=image, factor=factor, out_shape=out_shape, options=options)


def _f32_cases():
    c = []
    # whole ratios
    c.append(_case('whole_2x2_to_1x1', floats(2, 2, 1), out_shape=(1, 1)))
    c.append(_case('whole_4x6_to_2x3', floats(4, 6, 2), factor=0.5))
    c.append(_case('whole_9x6_to_3x2', floats(9, 6, 3), out_shape=(3, 2)))
    c.append(_case('whole_8x16_to_2x4', floats(8, 16, 4), factor=0.25))
    # the 16-byte route at factor 0.5 and its edges
    c.append(_case('half_w8', floats(6, 8, 5), factor=0.5))
    c.append(_case('half_w24', floats(6, 24, 6), factor=0.5))
    c.append(_case('half_w520', floats(4, 2 * 256 + 8, 7), factor=0.5))
    c.append(_case('half_w514', floats(4, 2 * 256 + 2, 8), factor=0.5))
    c.append(_case('half_w4112', floats(2, 2 * 2048 + 16, 14), factor=0.5))          # more than one step of a workgroup across a row
    c.append(_case('quarter_w48', floats(8, 48, 15), factor=0.25))
    c.append(_case('half_1030x2050_bits', finite_bit_patterns(1030, 2050, 9), factor=0.5))
    c.append(_case('half_64x2048_bits', finite_bit_patterns(64, 2048, 16), factor=0.5))
    # more output rows than the grid has workgroups (4096): the stride over rows, on both routes
    c.append(_case('tall_8200x8_to_4100x4', floats(8200, 8, 40), factor=0.5))
    c.append(_case('tall_8202x3_to_4101x1', floats(8202, 3, 41), out_shape=(4101, 1)))
    # mixed and fractional
    c.append(_case('mixed_5x8_to_2x4', floats(5, 8, 10), factor=0.5))
    c.append(_case('frac_7x7_to_3x3', floats(7, 7, 11), out_shape=(3, 3)))
    c.append(_case('frac_10x10_at_0.3', floats(10, 10, 12), factor=0.3))
    c.append(_case('frac_11x11_to_9x9', floats(11, 11, 13), out_shape=(9, 9)))
    c.append(_case('frac_1x9_to_1x4', floats(1, 9, 17), out_shape=(1, 4)))
    c.append(_case('frac_9x1_to_4x1', floats(9, 1, 18), out_shape=(4, 1)))
    c.append(_case('any_13x17_to_1x1', floats(13, 17, 19), out_shape=(1, 1)))
    c.append(_case('frac_300x7_to_290x5', floats(300, 7, 20), out_shape=(290, 5)))
    # identity
    x = floats(5, 7, 21)
    x[0, 0], x[1, 1], x[2, 2] = np.float32(-0.0), NAN, -INF
    c.append(_case('identity_5x7', x, factor=1))
    # NaN / inf
    x = floats(4, 4, 22)
    x[1, 2] = NAN
    c.append(_case('nan_in_2x2_block', x, factor=0.5))
    x = floats(11, 11, 23)
    x[1, 1] = NAN                                                                     # source 1 lies in outputs 0 and 1 (11 -> 9)
    c.append(_case('nan_in_shared_pixel', x, out_shape=(9, 9)))
    x = floats(4, 4, 24)
    x[0, 0], x[1, 1] = INF, -INF
    x[2, 2] = INF
    c.append(_case('inf_and_minus_inf', x, factor=0.5))
    x = floats(6, 6, 25)
    x[0, 0] = x[1, 1] = x[4, 5] = NAN
    x[2:4, 2:4] = NAN
    x[4, 0] = INF
    c.append(_case('omit_some_and_all', x, factor=0.5, nan_policy='omit'))
    x = floats(11, 11, 26)
    x[1, 1] = x[5, 6] = NAN
    c.append(_case('omit_fractional', x, out_shape=(9, 9), nan_policy='omit'))
    x = floats(4, 8, 27)
    x[:2, :2] = np.float32(-0.0)
    x[2:, 4:6] = np.float32(-0.0)
    c.append(_case('minus_zero_window', x, factor=0.5))
    x = floats(5, 5, 28)
    x[:3, :3] = np.float32(-0.0)
    c.append(_case('minus_zero_fractional', x, out_shape=(3, 3)))
    return c


def _u8_cases():
    c = []
    x = np.array([[1, 2, 1, 1, 255, 255, 7, 0],
                  [2, 1, 1, 2, 255, 254, 7, 7]], dtype=np.uint8)                      # means 1.5, 1.25, 254.75, (0)
    c.append(_case('u8_half_rounds_up', x, factor=0.5))
    c.append(_case('u8_half_rounds_up_keep_zero', x, factor=0.5, zero_invalid=False))
    x = bytes_(6, 8, 31)
    x[3, 5] = 0
    c.append(_case('u8_single_zero', x, factor=0.5))
    c.append(_case('u8_single_zero_in_mean', x, factor=0.5, zero_invalid=False))
    x = bytes_(11, 11, 32)
    x[1, 1] = 0
    c.append(_case('u8_shared_zero', x, out_shape=(9, 9)))
    c.append(_case('u8_shared_zero_in_mean', x, out_shape=(9, 9), zero_invalid=False))
    c.append(_case('u8_half_w16', bytes_(4, 16, 44, 0.05), factor=0.5))                # one 16-byte word per source row
    c.append(_case('u8_half_w32', bytes_(4, 32, 33, 0.05), factor=0.5))
    c.append(_case('u8_half_w48', bytes_(6, 48, 45, 0.05), factor=0.5))
    c.append(_case('u8_half_w1072', bytes_(4, 2 * 512 + 48, 46, 0.02), factor=0.5))     # more than one step across a row (out 536 = 67 words)
    c.append(_case('u8_half_w44', bytes_(4, 44, 47, 0.05), factor=0.5))                 # in aligned padded rows: 2 words and 6 single columns
    c.append(_case('u8_half_w8224', bytes_(2, 2 * 4096 + 32, 34, 0.02), factor=0.5))   # more than one step across a row
    c.append(_case('u8_half_w30', bytes_(4, 30, 35, 0.05), factor=0.5))
    c.append(_case('u8_quarter', bytes_(8, 64, 36, 0.02), factor=0.25))
    c.append(_case('u8_frac_7x7_to_3x3', bytes_(7, 7, 37, 0.05), out_shape=(3, 3)))
    c.append(_case('u8_any_to_1x1', bytes_(9, 14, 38), out_shape=(1, 1), zero_invalid=False))
    c.append(_case('u8_all_255', np.full((10, 10), 255, dtype=np.uint8), factor=0.3))
    c.append(_case('u8_tall_8200x32_to_4100x16', bytes_(8200, 32, 42, 0.02), factor=0.5))
    c.append(_case('u8_tall_8202x3_to_4101x1', bytes_(8202, 3, 43, 0.02), out_shape=(4101, 1)))
    c.append(_case('u8_identity', bytes_(3, 5, 39, 0.2), factor=1))
    return c


CASES = _f32_cases() + _u8_cases()
BY_NAME = {c['name']: c for c in CASES}
NAMES = [c['name'] for c in CASES]
assert len(BY_NAME) == len(CASES)
_EXPECTED = {}


def shape_of(c):
    if c['out_shape'] is not None:
        return tuple(c['out_shape'])
    return spec.out_shape(c['image'].shape[0], c['image'].shape[1], c['factor'])


def expected(name):
    """The specification's result of a case: computed on first use, shared, read-only."""
    if name not in _EXPECTED:
        c = BY_NAME[name]
        fn = spec.resize_f32 if c['image'].dtype == np.float32 else spec.resize_u8
        out = fn(c['image'], *shape_of(c), **c['options'])
        out.setflags(write=False)
        _EXPECTED[name] = out
    return _EXPECTED[name]


def call_kwargs(c):
    """The keyword arguments of lib.resize_image for a case."""
    kw = dict(c['options'])
    if c['out_shape'] is not None:
        kw['out_shape'] = c['out_shape']
    else:
        kw['factor'] = c['factor']
    return kw
