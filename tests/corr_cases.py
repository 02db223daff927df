"""The cases that tests/test_corr_host.py (host instance) and tests/test_gpu_corr.py (device) run against tests/corr_spec.py.
No tests in here.  Images are at most 300 x 300, the smallest at which each path can go wrong: see the reason beside each
case.  A lattice case holds what libcorr.local_correlation takes (window, step, origin, shape, min_count; None = the default),
a points case what libcorr.local_correlation_at takes (c, r, valid)."""
import numpy as np

from sea_ice_drift_amd import _capi

TR, TC = _capi.CORR_TILE


def pair(shape, seed, zeros=0.0, noise=40.0):
    """Two uint8 images in 1..255, the second the first plus noise (so that r is neither 0 nor 1), each with its own share
    `zeros` of 0 (invalid) pixels."""
    rng = np.random.default_rng(seed)
    a = rng.integers(1, 256, size=shape, dtype=np.uint8)
    b = np.clip(np.rint(a + noise * rng.normal(size=shape)), 1, 255).astype(np.uint8)
    if zeros:
        a[rng.random(shape) < zeros] = 0
        b[rng.random(shape) < zeros] = 0
    return a, b


def lattice(name, a, b, window, step=1, origin=None, shape=None, min_count=None):
    return dict(name=name, kind='lattice', a=a, b=b, window=window, step=step, origin=origin, shape=shape, min_count=min_count)


def at(name, a, b, window, c, r, valid=None, min_count=None):
    return dict(name=name, kind='points', a=a, b=b, window=window, c=np.asarray(c), r=np.asarray(r), valid=valid, min_count=min_count)


def resolved(c):
    """The defaults of libcorr.local_correlation, restated: -> step (sr, sc), origin, shape, min_count."""
    w = c['window']
    step = (c['step'], c['step']) if np.ndim(c['step']) == 0 else tuple(c['step'])
    origin = (w // 2, w // 2) if c.get('origin') is None else tuple(c['origin'])
    rows, cols = c['a'].shape
    shape = c.get('shape')
    if shape is None:
        shape = tuple((n - w) // s + 1 if n >= w else 0 for n, s in ((rows, step[0]), (cols, step[1])))
    return step, origin, tuple(shape), (w * w + 1) // 2 if c['min_count'] is None else c['min_count']


def _cases():
    out = []
    # ---- step against window: larger (nothing shared: a wavefront per node; sr != sc), equal, smaller, 1
    a, b = pair((120, 150), 1, zeros=0.05)
    out.append(lattice('step_larger', a, b, 7, step=(11, 9)))
    out.append(lattice('step_equal_even_window', a, b, 8, step=8))
    a, b = pair((100, 300), 2, zeros=0.05)
    out.append(lattice('step_smaller', a, b, 35, step=(4, 8)))                # 17 x 34 nodes: three tile rows
    a, b = pair((80, 140), 3, zeros=0.05)
    out.append(lattice('step_1', a, b, 35))                                   # 46 x 106 nodes: tiles along both axes
    out.append(lattice('step_mixed_rows', a, b, 9, step=(20, 2)))             # rows side by side, columns shared
    out.append(lattice('step_mixed_cols', a, b, 9, step=(2, 20)))             # and the reverse
    # 69 000 nodes, more than one launch of wavefronts per node holds; the windows inside the image belong to the last of them
    out.append(lattice('step_larger_many', a, b, 3, step=3, origin=(1 - 3 * 1474, 1), shape=(1500, 46), min_count=1))
    # ---- window: 1 (va = 0 everywhere: NaN with min_count = 1), 2, 255 on an image smaller than the window
    a, b = pair((20, 70), 4, zeros=0.05)
    out.append(lattice('window_1', a, b, 1))
    out.append(lattice('window_2', a, b, 2))
    a, b = pair((100, 90), 5, zeros=0.05)
    out.append(lattice('window_255_small_image', a, b, 255, step=(20, 30), origin=(50, 45), shape=(3, 3), min_count=1000))
    # ---- the wide LDS segment: a tile row of more than 2048 slots, windows side by side along the columns (equal step; a
    # larger one, the pixels between the windows never read), shared along the rows
    a, b = pair((40, 300), 6, zeros=0.05)
    out.append(lattice('wide_row_255', a, b, 255, step=(100, 255), origin=(20, -300), shape=(2, 10), min_count=1))
    out.append(lattice('wide_row_gaps', a, b, 101, step=(30, 150), origin=(25, -500), shape=(2, 30), min_count=1))
    # ---- tile: one node short of, on and one node past the workgroup's tile, per axis
    a, b = pair((24, 140), 7, zeros=0.05)
    for d in (-1, 0, 1):
        out.append(lattice('tile%+d' % d, a, b, 5, step=2, shape=(TR + d, TC + d)))
    # ---- origin: windows clipped at every edge and corner, empty windows on every side; centres that int64 barely holds
    a, b = pair((40, 50), 8, zeros=0.05)
    out.append(lattice('origin_outside', a, b, 9, step=(7, 6), origin=(-20, -15), shape=(12, 16), min_count=1))
    out.append(lattice('origin_beyond_last', a, b, 9, step=(3, 4), origin=(30, 40), shape=(8, 8), min_count=1))
    out.append(lattice('origin_int64', a, b, 9, step=(2 ** 61, 2 ** 40), origin=(-2 ** 62, 3), shape=(5, 3), min_count=1))
    # ---- alignment: 61 columns, rows 61 and 67 bytes apart, a view that starts at column 3
    a, b = pair((30, 61), 9, zeros=0.05)
    wide = np.zeros((30, 67), dtype=np.uint8)
    wide[:, 3:64] = b
    out.append(lattice('unaligned_b_view', a, wide[:, 3:64], 6, step=(3, 5)))
    wide_a = np.zeros((30, 67), dtype=np.uint8)
    wide_a[:, 3:64] = a
    out.append(lattice('unaligned_a_view', wide_a[:, 3:64], b, 7, step=1))
    a, b = pair((1, 1), 10)
    out.append(lattice('image_1x1', a, b, 3, origin=(0, 0), shape=(2, 2), min_count=1))
    a, b = pair((40, 1), 11, zeros=0.05)
    out.append(lattice('one_column', a, b, 5, step=(2, 1), origin=(0, 0), shape=(20, 2), min_count=2))
    out.append(lattice('empty_image', np.zeros((0, 7), np.uint8), np.zeros((0, 7), np.uint8), 3, origin=(0, 0), shape=(2, 3)))
    out.append(lattice('no_nodes', a, b, 5, shape=(0, 4)))
    # ---- zeros: in one image only (the mask is the same whichever image holds them), a band of rows, a whole image
    a, b = pair((50, 80), 12)
    z = np.random.default_rng(12).random(a.shape) < 0.1
    az, bz = a.copy(), b.copy()
    az[z], bz[z] = 0, 0
    out.append(lattice('zeros_in_a', az, b, 9, step=3, min_count=1))
    out.append(lattice('zeros_in_b', a, bz, 9, step=3, min_count=1))
    band = a.copy()
    band[10:31] = 0
    out.append(lattice('zero_band', band, b, 9, step=3))
    out.append(lattice('a_all_zero', np.zeros_like(a), b, 9, step=3, min_count=1))
    # ---- overflow: Saa of a window beyond 2^31 (w >= 182 with 255s); constant images give NaN, checkerboards a value
    full = np.full((200, 200), 255, dtype=np.uint8)
    out.append(lattice('overflow_255', full, full, 183, step=5))
    ii, jj = np.meshgrid(np.arange(200), np.arange(200), indexing='ij')
    out.append(lattice('overflow_checkerboards', (254 + (ii + jj) % 2).astype(np.uint8), (254 + (ii + jj // 2) % 2).astype(np.uint8),
                       183, step=5))
    # ---- min_count: windows of 25 pixels side by side, the first with 20 usable pixels, the second with 19
    a, b = pair((10, 30), 13)
    a[0, 0:5] = 0
    a[1, 5:8] = 0
    b[2, 5:8] = 0
    out.append(lattice('min_count_both_sides', a, b, 5, step=5, min_count=20))
    # ---- identical images: r is whatever the arithmetic gives, 1 to within rounding
    a, _ = pair((64, 100), 14, zeros=0.05)
    out.append(lattice('identical', a, a.copy(), 11, step=3))
    # ---- points
    a, b = pair((60, 70), 15, zeros=0.05)
    rng = np.random.default_rng(15)
    c, r = rng.integers(-10, 81, size=(5, 8)), rng.integers(-10, 71, size=(5, 8))
    c[1], r[1] = c[0], r[0]                                                   # duplicates
    c[2, :4], r[2, :4] = (-100, 500, 30, 30), (30, 30, -100, 500)             # far outside on each side: empty windows
    out.append(at('points_anywhere', a, b, 9, c, r, min_count=1))
    valid = (rng.random((5, 8)) < 0.6).astype(np.uint8)
    cg, rg = c.astype(np.int32), r.astype(np.int32)
    cg[valid == 0], rg[valid == 0] = np.iinfo(np.int32).min, np.iinfo(np.int32).max           # garbage behind valid == 0
    out.append(at('points_valid', a, b, 9, cg, rg, valid=valid, min_count=1))
    out.append(at('points_int32_extremes', a, b, 255, np.array([np.iinfo(np.int32).max, np.iinfo(np.int32).min, 35], dtype=np.int32),
                  np.array([30, 30, np.iinfo(np.int32).max], dtype=np.int32), min_count=1))
    out.append(at('points_none', a, b, 9, np.zeros((0,), dtype=np.int32), np.zeros((0,), dtype=np.int32)))
    out.append(at('points_one', a, b, 35, np.array([33]), np.array([28])))
    out.append(at('points_window_255', a, b, 255, np.array([0, 35, 69]), np.array([0, 30, 59]), min_count=1000))
    a, b = pair((40, 50), 16, zeros=0.05)
    out.append(at('points_70000', a, b, 3, rng.integers(-2, 52, size=70000).astype(np.int32),     # more than 65535 wavefronts
                  rng.integers(-2, 42, size=70000).astype(np.int32), min_count=2))
    return out


CASES = _cases()
NAMES = [c['name'] for c in CASES]
BY_NAME = dict(zip(NAMES, CASES))
assert len(BY_NAME) == len(CASES)

_expected = {}


def expected(name):
    """The specification's result of a case, computed once and shared (read-only)."""
    if name not in _expected:
        from tests import corr_spec as cs
        c = BY_NAME[name]
        if c['kind'] == 'lattice':
            step, origin, shape, min_count = resolved(c)
            res = cs.lattice(c['a'], c['b'], c['window'], origin, step, shape, min_count)
        else:
            w = c['window']
            res = cs.points(c['a'], c['b'], w, c['c'], c['r'], c['valid'], (w * w + 1) // 2 if c['min_count'] is None else c['min_count'])
        for v in res.values():
            v.setflags(write=False)
        _expected[name] = res
    return _expected[name]


def check(got, name, what):
    """got = (r, count, sums): bit for bit the specification's."""
    from tests import corr_spec as cs
    exp = expected(name)
    for key, g in zip(('r', 'count', 'sums'), got):
        e = exp[key]
        assert g is not None and g.dtype == e.dtype and g.shape == e.shape, '%s %s: %s is %s %s, expected %s %s' % (
            name, what, key, getattr(g, 'dtype', None), getattr(g, 'shape', None), e.dtype, e.shape)
        if not cs.same_bits(g, e):
            gb = np.ascontiguousarray(g).view(np.uint8).reshape(g.shape + (g.itemsize,))
            eb = np.ascontiguousarray(e).view(np.uint8).reshape(g.shape + (g.itemsize,))
            diff = np.argwhere((gb != eb).any(-1))
            raise AssertionError('%s %s: %s differs from the specification at %d elements, first %s (got %r, expected %r)'
                                 % (name, what, key, len(diff), diff[0].tolist(), g[tuple(diff[0])], e[tuple(diff[0])]))
