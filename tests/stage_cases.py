"""Small named inputs of the uint8 staging step, shared by tests/test_stage_spec_host.py (CPU: the premises),
tests/test_gpu_stage_paths.py (the kernels) and tests/golden/make_golden.py (fixture g6b).  Every image has at most about
25 000 pixels; every builder is cached, and the arrays it returns are read-only.  No tests in here.

  route_cases()     96 x 100 images whose key distribution is 2^T keys wide: (name, image, fractions, aim); the aim is the route
                    the case was written for - ('direct', 0), ('resolved', states per bin) or ('radix', 0) - for EVERY rank of
                    stage_spec.fraction_ranks; test_stage_spec_host.py checks it against the spec, so no GPU case is vacuous
  selector_cases()  (name, image, fractions, rank lists of consecutive order_stats calls, aim) for sid_stage_order_stats_ws
  sampler_cases()   name -> image: the sizes around the sample's 8192 and the m < 256 cut-off, NaN-heavy images
  keyspace_cases()  name -> 64 x 64 image: the edges of the key space
  layout_cases()    placements of one image content in a larger buffer (each path of hist / range / scale_kernel)
  scale_probes()    pixels whose scaled value lies within a few ulp of an integer, per (vmin, denom) pair
  golden_g6b()      fixture tests/golden/g6b_uint8_small.npz: the reference's own outputs on public_cases()
"""
import functools
import os

import numpy as np

from sea_ice_drift_amd import synthetic as syn
from tests import stage_spec as spec

HERE = os.path.dirname(os.path.abspath(__file__))

FLT_MAX = np.float32(3.4028234663852886e38)
SUB_MIN = np.uint32(0x00000001).view(np.float32)       # smallest subnormal, 2^-149
SUB_MAX = np.uint32(0x007fffff).view(np.float32)       # largest subnormal
FRACTION_SETS = ([0.10, 0.99], [0.5], [0.0, 1.0], [0.001, 0.25, 0.75, 0.999], [0.1, 0.5, 0.9], [-0.5, 1.5], [0.5, 0.5])
PERCENTILE_PAIRS = ((10, 99), (0, 100), (50, 50), (1, 99.9))


def _ro(a):
    a = np.ascontiguousarray(a, dtype=np.float32)
    a.setflags(write=False)
    return a


def _bits(rng, shape, base, width):
    return (np.uint32(base) + rng.integers(0, width, shape).astype(np.uint32)).view(np.float32)


def wide_image(log2_width, shape=(96, 100)):
    """Positive floats whose bit patterns are uniform over 2^log2_width keys from 1.0 upwards."""
    return _ro(_bits(np.random.default_rng(5), shape, 0x3f800000, 2 ** log2_width))


# ---------------------------------------------------------------------------------------------- route cases
@functools.lru_cache(maxsize=None)
def route_cases():
    out = []
    for t, fr, aim in ((14, [0.10, 0.99], ('direct', 0)), (14, [0.5], ('direct', 0)), (20, [0.10, 0.99], ('resolved', 1)),
                       (20, [0.5], ('resolved', 1)), (26, [0.5], ('resolved', 2)), (27, [0.5], ('resolved', 4)),
                       (28, [0.5], ('resolved', 8)), (29, [0.5], ('radix', 0)),
                       (14, [0.0, 1.0], ('radix', 0)), (20, [0.0, 1.0], ('radix', 0)), (28, [0.0, 1.0], ('radix', 0))):
        out.append(('w%d_%s' % (t, '_'.join('%g' % f for f in fr)), wide_image(t), fr, aim))
    sar = _ro(np.random.default_rng(5).normal(-20.0, 5.0, (96, 100)))       # negative floats: the key is ~bits
    out.append(('sar_0.5', sar, [0.5], ('resolved', 1)))
    out.append(('sar_0_1', sar, [0.0, 1.0], ('radix', 0)))
    return tuple(out)


# ---------------------------------------------------------------------------------------------- selector cases
@functools.lru_cache(maxsize=None)
def mixed_image():
    """Lower half of the values 2^12 keys wide (a hinted range there has one key per bin), upper half 2^24 keys wide."""
    rng = np.random.default_rng(8)
    a = np.concatenate([_bits(rng, 4800, 0x3f800000, 2 ** 12), _bits(rng, 4800, 0x40000000, 2 ** 24)])
    return _ro(rng.permutation(a).reshape(96, 100))


TWO_WIDTHS_FRACTIONS = (0.5, 0.55)


@functools.lru_cache(maxsize=None)
def two_widths_image():
    """(image, rank A, rank B) of 64 x 64 pixels laid out key by key (every pixel is sampled, so sample ranks are image ranks):
    the ranks the sampler brackets fraction 0.5 with are 16 keys apart, the ranks above them 65536 keys apart except the first,
    which follows 2 keys behind.  The range of 0.5 then has bins of a few keys, the range of 0.55 - which overlaps it and
    reaches further up - bins of 8192 keys.  Rank A (in the first range) and rank B (just above it: second range only) have
    bins that START AT THE SAME KEY, a multiple of 8192, with different widths."""
    m = 4096
    a_lo, a_hi, _ = spec.bracket_ranks(TWO_WIDTHS_FRACTIONS[0], m)
    x = 0xC0010000                                                   # key of float32 2.0001...; a multiple of 8192
    k0 = x - 16 * 380
    r = np.arange(m, dtype=np.int64)
    keys = np.where(r < a_lo, k0 - (a_lo - r) * 4096, k0 + (r - a_lo) * 16)
    top = k0 + (a_hi - a_lo) * 16 + 2
    keys = np.where(r > a_hi, top + (r - a_hi - 1) * 65536, keys)
    assert (np.diff(keys) > 0).all() and keys.min() > 0x80000000 and keys.max() < 0xff000000
    img = spec.key2f(keys.astype(np.uint32))
    return _ro(np.random.default_rng(2).permutation(img).reshape(64, 64)), a_lo + 380, a_hi + 1


def _spread(B, q, count):
    return [int(r) for r in np.linspace(B['below'][q], B['below'][q] + B['inside'][q] - 1, count).astype(np.int64)]


def _same_bin_pair(B, q):
    """Two neighbouring ranks of range q whose keys differ and lie in one bin."""
    for r in range(B['below'][q], B['below'][q] + B['inside'][q] - 1):
        a, b = spec.rank_route(B, r), spec.rank_route(B, r + 1)
        if a == b and B['keys'][r] != B['keys'][r + 1]:
            return [r, r + 1]
    raise AssertionError('no two keys share a bin')


@functools.lru_cache(maxsize=None)
def selector_cases():
    """(name, image, fractions, calls, aim): `calls` = the rank lists of consecutive order_stats calls after one begin;
    aim = per call (n_direct, n_resolved, n_radix, resolve_passes, resolve_states) as the case was written."""
    out = []
    for t in (27, 28):                                               # shift 13 / 14: 4 / 8 states per bin
        img = wide_image(t)
        B = spec.begin_hint(img, [0.5])
        twelve = _spread(B, 0, 12)
        per = 4 if t == 27 else 8
        out.append(('twelve_w%d' % t, img, [0.5], (twelve,), ((0, 12, 0, 12 * per // 8, 12 * per),)))
    img = wide_image(27)
    B = spec.begin_hint(img, [0.5])
    twelve, far = _spread(B, 0, 12), [0, B['n_valid'] // 3, B['n_valid'] - 1]
    # a second and a third call after the first: the resolving passes have overwritten the pinned states meanwhile
    out.append(('again_w27', img, [0.5], (twelve, twelve[::-1], far, twelve[:3] + far),
                ((0, 12, 0, 6, 48), (0, 12, 0, 6, 48), (0, 0, 3, 0, 0), (0, 3, 3, 2, 12))))
    img = wide_image(20)
    B = spec.begin_hint(img, [0.5])
    pair = _same_bin_pair(B, 0)
    out.append(('shared_bin_w20', img, [0.5], (pair, pair + [pair[0]]), ((0, 2, 0, 1, 1), (0, 3, 0, 1, 1))))
    img = mixed_image()
    B = spec.begin_hint(img, [0.25, 0.75])
    n = B['n_valid']
    split = [B['below'][0] + 5, B['below'][1] + 7, n - 1, B['below'][0] + B['inside'][0] - 1, 0, B['below'][1] + B['inside'][1] - 1]
    out.append(('split_mixed', img, [0.25, 0.75], (split,), ((2, 2, 2, 1, 2),)))
    n = 9600
    out.append(('clamped_w20', wide_image(20), [-0.5, 1.5], (spec.fraction_ranks(n, [0.0, 1.0]),), ((0, 0, 3, 0, 0),)))
    four = [0.001, 0.25, 0.75, 0.999]
    out.append(('four_w20', wide_image(20), four, (spec.fraction_ranks(n, four),), ((0, 4, 4, 1, 4),)))    # (0.001 and 0.999: open brackets)
    three = [0.1, 0.5, 0.9]
    out.append(('three_w20', wide_image(20), three, (spec.fraction_ranks(n, three),), ((0, 6, 0, 1, 5),)))   # (two of the ranks share a bin)
    # two overlapping ranges whose bins start at one key with different widths: two states, not one shared
    img, a, b = two_widths_image()
    out.append(('two_widths', img, list(TWO_WIDTHS_FRACTIONS), ([a, b], [b, a], [b], [a]), ((0, 2, 0, 1, 5), (0, 2, 0, 1, 5), (0, 1, 0, 1, 4), (0, 1, 0, 1, 1))))
    # nine ranks outside every range: two radix sweeps
    out.append(('nine_radix_w20', wide_image(20), [0.5], ([100 * k for k in range(9)],), ((0, 0, 9, 0, 0),)))
    return tuple(out)


# ---------------------------------------------------------------------------------------------- sampler cases
def _sar(rng, shape, nan=0.03):
    a = rng.normal(-20.0, 5.0, shape).astype(np.float32)
    a[rng.random(shape) < nan] = np.nan
    return a


@functools.lru_cache(maxsize=None)
def sampler_cases():
    rng = np.random.default_rng(31)
    c = {}
    c['n1'] = np.full((1, 1), -17.25, dtype=np.float32)
    c['n255'] = rng.normal(-20.0, 5.0, (15, 17))                     # m = 255: one below the cut-off
    c['n256'] = rng.normal(-20.0, 5.0, (16, 16))                     # m = 256 exactly, all valid
    c['n257_one_nan'] = rng.normal(-20.0, 5.0, (1, 257))             # 257 pixels, one NaN: m = 256 again
    c['n257_one_nan'][0, 100] = np.nan
    c['n8191'] = _sar(rng, (1, 8191))                                # step 0, the last sample position is skipped
    c['n8192'] = _sar(rng, (64, 128))                                # step 1: every pixel
    c['n8193'] = _sar(rng, (3, 2731))                                # step 1: the last pixel is never sampled
    c['step2'] = _sar(rng, (130, 130))
    c['step3'] = _sar(rng, (200, 123))
    sparse = np.full((128, 128), np.nan, dtype=np.float32)           # 99 % NaN: the sample has m < 256, the image ~1 % of 16384 valid
    put = rng.permutation(128 * 128)[:300]
    sparse.flat[put] = rng.normal(-20.0, 5.0, 300)
    c['nan99'] = sparse
    c['all_nan'] = np.full((40, 52), np.nan, dtype=np.float32)
    one = np.full((33, 47), np.nan, dtype=np.float32)
    one[20, 11] = 3.5
    c['one_valid'] = one
    return {k: _ro(v) for k, v in c.items()}


# ---------------------------------------------------------------------------------------------- key-space cases
def _sprinkle(rng, img, values, each=40):
    flat = img.reshape(-1)
    pos = rng.permutation(flat.size)[:each * len(values)]
    for k, v in enumerate(values):
        flat[pos[k * each:(k + 1) * each]] = v
    return img


def _f(bits):
    return np.uint32(bits).view(np.float32)


@functools.lru_cache(maxsize=None)
def keyspace_cases():
    rng = np.random.default_rng(47)
    base = lambda: rng.normal(0.0, 4.0, (64, 64)).astype(np.float32)
    c = {}
    c['inf'] = _sprinkle(rng, base(), [np.inf, -np.inf, np.nan], each=30)
    c['inf_heavy'] = _sprinkle(rng, base(), [np.inf, -np.inf], each=700)         # +-inf ARE the 10th and 99th percentiles
    c['zeros'] = _sprinkle(rng, base(), [np.float32(-0.0), np.float32(0.0)], each=600)
    c['subnormal'] = _sprinkle(rng, base(), [SUB_MIN, -SUB_MIN, SUB_MAX, -SUB_MAX, _f(0x00800000), _f(0x80800000)], each=60)
    c['flt_max'] = _sprinkle(rng, base(), [FLT_MAX, -FLT_MAX], each=50)
    c['nan_payload'] = _sprinkle(rng, base(), [_f(0xffc00000), _f(0xffc00001), _f(0x7f800001), _f(0xff800001), _f(0x7fffffff),
                                               _f(0xffffffff)], each=25)
    c['constant'] = np.full((64, 64), -17.5, dtype=np.float32)
    c['two_valued'] = np.where(rng.random((64, 64)) < 0.3, np.float32(-3.25), np.float32(12.5)).astype(np.float32)
    c['last10'] = _bits(rng, (64, 64), 0x41200000, 1024)                          # one bin in the first two radix digits
    k = rng.integers(-3000, 3001, (64, 64))                                        # k * 2^-149: keys contiguous across the sign change
    c['sign_straddle'] = np.where(k < 0, np.uint32(0x80000000) + np.abs(k).astype(np.uint32), k.astype(np.uint32)).astype(np.uint32).view(np.float32)
    c['sign_wide'] = rng.normal(0.0, 1.0, (64, 64)).astype(np.float32)            # the 0.5 bracket spans -x .. +x: almost all keys
    return {k_: _ro(v) for k_, v in c.items()}


def public_cases():
    """The inputs of the public-call test and of fixture g6b: every sampler and key-space case."""
    d = dict(sampler_cases())
    d.update(keyspace_cases())
    return d


def has_two_finite_values(img):
    v = img[np.isfinite(img)]
    return v.size > 0 and v.min() != v.max()


# ---------------------------------------------------------------------------------------------- layout cases
SENTINEL_IN = np.float32(np.inf)
SENTINEL_OUT = 0xAB


@functools.lru_cache(maxsize=None)
def layout_content(rows, cols):
    rng = np.random.default_rng(1000 * rows + cols)
    a = rng.normal(-20.0, 5.0, (rows, cols)).astype(np.float32)
    if a.size > 8:
        a[rng.random(a.shape) < 0.05] = np.nan
    return _ro(a)


# name -> (rows, cols, row stride, offset of pixel (0, 0) in a 256-byte aligned float32 buffer), all in elements
LAYOUTS = {
    'contiguous': (7, 1028, 1028, 0),                # flat 16-byte path, 1799 words: more than one workgroup, a tail
    'words_3x8': (3, 8, 8, 0),                       # 6 words: x >= n4 for most lanes
    'words_1x4': (1, 4, 4, 0),
    'one_pixel': (1, 1, 1, 0),
    'stride_vec': (7, 1028, 1036, 4),                # row-wise vector path, n4 = 257 > 256 lanes
    'base_plus1': (7, 1028, 1028, 1),                # 4-byte aligned only: scalar path with cols % 4 == 0
    'stride_plus2': (7, 1028, 1030, 0),              # stride % 4 != 0 at cols % 4 == 0
    'odd_cols': (5, 1027, 1027, 0),
    'odd_cols_strided': (5, 1027, 1031, 3),
    'tall': (4100, 4, 4, 0),                         # contiguous: flat path
    'tall_stride_vec': (4100, 4, 8, 4),              # the row loop's second trip (grid 4096; 1024 in the range pass)
    'tall_stride_scalar': (4100, 4, 5, 1),
}
# out: (row stride - cols, offset of out(0, 0) in a 256-byte aligned uint8 buffer)
OUT_LAYOUTS = {'contiguous': (0, 0), 'strided': (4, 8), 'byte_off': (0, 1), 'strided_odd': (3, 4)}


def layout_buffer(name):
    """(flat float32 buffer filled with +inf around the view, rows, cols, stride, offset, content)."""
    rows, cols, stride, off = LAYOUTS[name]
    content = layout_content(rows, cols)
    buf = np.full(off + rows * stride + 9, SENTINEL_IN, dtype=np.float32)
    view = np.lib.stride_tricks.as_strided(buf[off:], (rows, cols), (4 * stride, 4))
    view[...] = content
    return buf, rows, cols, stride, off, content


# ---------------------------------------------------------------------------------------------- scale probes
SCALE_PAIRS = ((-21.37, 11.93), (-0.0031, 0.0077), (1e-39, 1e-38), (5.0, -3.0))      # (vmin, denom), taken as float32
SCALE_PAIRS_BLIND = ((-30.0, 17.5), (0.0, 1.0))      # pairs at which t * (1 / denom) equals t / denom on every probe: not enough
SCALE_SPECIALS = np.array([np.inf, -np.inf, np.nan, 0.0, -0.0, FLT_MAX, -FLT_MAX], dtype=np.float32)
# (vmin, vmax) whose float32 difference is 0, NaN, +inf, -inf and a subnormal
SCALE_ODD_DENOMS = ((-17.5, -17.5), (-20.0, np.nan), (-20.0, np.inf), (-20.0, -np.inf), (0.0, 1e-40), (np.inf, np.inf))


@functools.lru_cache(maxsize=None)
def scale_probes(vmin, denom):
    """For n = 1 .. 255 the float32 nearest the pixel value that scales to n exactly, and its 8 float32 neighbours on either
    side: 4335 pixels; then the special values.  As one row (1 x 4342: cols % 4 != 0 - reshape for the vector path)."""
    vmin, denom = np.float32(vmin), np.float32(denom)
    n = np.arange(1, 256, dtype=np.float64)
    centre = (np.float64(vmin) + (n - 1) * np.float64(denom) / 254.0).astype(np.float32)
    cols = [centre]
    up, down = centre, centre
    for _ in range(8):
        up = np.nextafter(up, np.float32(np.inf))
        down = np.nextafter(down, np.float32(-np.inf))
        cols += [up, down]
    return _ro(np.concatenate([np.stack(cols, axis=1).ravel(), SCALE_SPECIALS])[None, :])


def scale_reference(x, vmin, denom, reciprocal=False):
    """lib.py:54-59 of the reference in NumPy float32 with the denominator given (oracle/stage_oracle.get_uint8_image's
    arithmetic); reciprocal=True: the same with `* (1 / denom)`, the subtly wrong form the probes must tell apart."""
    x, vmin, denom = np.asarray(x, dtype=np.float32), np.float32(vmin), np.float32(denom)
    with np.errstate(all='ignore'):
        t = np.float32(254) * (x - vmin)
        u = np.float32(1) + (t * (np.float32(1) / denom) if reciprocal else t / denom)
        assert u.dtype == np.float32
        u[u < 1] = 1
        u[u > 255] = 255
        u[~np.isfinite(x)] = 0
        u[np.isnan(u)] = 0
        return u.astype('uint8')


# ---------------------------------------------------------------------------------------------- fixture g6b
G6B_EVERY = 61                   # the fixture keeps the sha256 of an output and every 61st of its pixels


def golden_g6b():
    """Fixture g6b as {name: (sha256, subsample, vmin, vmax)} and the names it leaves to the oracle."""
    g = np.load(os.path.join(HERE, 'golden', 'g6b_uint8_small.npz'))
    start = g['sub_start']
    stored = {str(n): (str(g['sha'][k]), g['sub'][start[k]:start[k + 1]], g['vmin'][k], g['vmax'][k]) for k, n in enumerate(g['names'])}
    return stored, set(str(s) for s in g['left_to_the_oracle'])


def g6b_equal(stored, key, out):
    """`out` is the stored output `key` of fixture g6b: the subsample (for a readable failure), then the sha256 of all of it."""
    out = np.ascontiguousarray(out)
    assert out.dtype == np.uint8
    np.testing.assert_array_equal(out.ravel()[::G6B_EVERY], stored[key][1], err_msg=key)
    assert syn.sha256(out) == stored[key][0], key
