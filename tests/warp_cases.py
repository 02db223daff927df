"""The cases that tests/test_warp_host.py (host instance) and tests/test_gpu_warp.py (device) run against tests/warp_spec.py.
No tests in here.  Images are at most 300 x 300 and node grids at most 9 x 13, the smallest at which each path can go wrong:
see the reason beside each case."""
import numpy as np

from sea_ice_drift_amd import _capi

TR, TC = _capi.WARP_TILE


def image_u8(shape, seed, zeros=0.0):
    """Random uint8 image in 1..255, with a share `zeros` of 0 (invalid) pixels."""
    rng = np.random.default_rng(seed)
    img = rng.integers(1, 256, size=shape, dtype=np.uint8)
    if zeros:
        img[rng.random(shape) < zeros] = 0
    return img


def image_f32(shape, seed):
    return np.random.default_rng(seed).normal(size=shape).astype(np.float32)


def node_grid(rows, cols, dr, dc, r0=0.0, c0=0.0, jitter=0.0, integer=False, seed=0):
    """(rows, cols) nodes `dr`, `dc` pixels apart from (r0, c0), each moved by up to `jitter` of the spacing (at most a quarter:
    the cells stay convex), rounded to integers on request.  -> x, y"""
    assert jitter <= 0.25
    rng = np.random.default_rng(seed)
    y, x = np.meshgrid(r0 + dr * np.arange(rows, dtype=np.float64), c0 + dc * np.arange(cols, dtype=np.float64), indexing='ij')
    x = x + jitter * dc * rng.uniform(-1, 1, size=x.shape)
    y = y + jitter * dr * rng.uniform(-1, 1, size=y.shape)
    if integer:
        x, y = np.rint(x), np.rint(y)
    return np.ascontiguousarray(x), np.ascontiguousarray(y)


def smooth_source(x, y, seed, amp=3.0, shift=(0.0, 0.0)):
    """Source positions of the nodes: a shift plus a smooth field plus a little noise."""
    rng = np.random.default_rng(seed + 1000)
    xs = x + shift[0] + amp * np.sin(y / 23.0) + 0.3 * rng.normal(size=x.shape)
    ys = y + shift[1] + amp * np.cos(x / 31.0) + 0.3 * rng.normal(size=x.shape)
    return xs, ys


def holes(shape, seed, share=0.2):
    return (np.random.default_rng(seed + 2000).random(shape) >= share).astype(np.uint8)


def case(name, x, y, xs, ys, out_shape, image=None, src_shape=None, valid=None, diagonal='shorter', order=1, fill=0,
         keep_zero=None, want=('out', 'covered', 'maps')):
    if image is not None:
        src_shape = image.shape
        if keep_zero is None:
            keep_zero = image.dtype == np.uint8
    else:
        want = tuple(w for w in want if w != 'out')
    return dict(name=name, x=x, y=y, xs=xs, ys=ys, out_shape=tuple(out_shape), image=image, src_shape=tuple(src_shape), valid=valid,
                diagonal=diagonal, order=order, fill=fill, keep_zero=bool(keep_zero), want=want)


def _cases():
    out = []
    # ---- the four ownership grids (regular, curvilinear-integer, curvilinear-fractional, holed), through every option
    x, y = node_grid(7, 9, 5, 6)                                          # nodes on pixel centres: 31 x 49 pixels of hull
    xs, ys = smooth_source(x, y, 1, shift=(4.0, 3.0))
    out.append(case('regular_u8_o1', x, y, xs, ys, (35, 53), image_u8((40, 60), 1, zeros=0.05)))
    out.append(case('regular_u8_o0', x, y, xs, ys, (35, 53), image_u8((40, 60), 1), order=0, fill=9))
    out.append(case('regular_f32_o1', x, y, xs, ys, (35, 53), image_f32((40, 60), 2), fill=-1.5, diagonal='main'))
    out.append(case('regular_f32_o0', x, y, xs, ys, (35, 53), image_f32((40, 60), 2), order=0, diagonal='anti'))
    for k, diag in enumerate(('shorter', 'main', 'anti')):
        x, y = node_grid(9, 13, 11, 9, r0=3, c0=2, jitter=0.25, integer=True, seed=10 + k)
        xs, ys = smooth_source(x, y, 10 + k)
        out.append(case('curvi_int_' + diag, x, y, xs, ys, (100, 120), image_u8((100, 120), 3 + k, zeros=0.1), diagonal=diag,
                        keep_zero=bool(k % 2), order=1))
        x, y = node_grid(9, 13, 11.3, 9.7, r0=2.6, c0=1.4, jitter=0.25, seed=20 + k)
        xs, ys = smooth_source(x, y, 20 + k)
        out.append(case('curvi_frac_' + diag, x, y, xs, ys, (100, 125), image_u8((110, 130), 6 + k), diagonal=diag, order=k % 2))
        x, y = node_grid(9, 13, 10, 10, r0=4, c0=4, jitter=0.2, integer=bool(k % 2), seed=30 + k)
        xs, ys = smooth_source(x, y, 30 + k)
        valid = holes(x.shape, 30 + k)
        x[2, 3] = np.nan                                                  # a NaN node beside the mask's holes: one-triangle cells
        ys[5, 7] = np.inf
        out.append(case('holed_' + diag, x, y, xs, ys, (95, 130), image_f32((95, 130), 9 + k), valid=valid, diagonal=diag))
    # ---- work items
    x, y = np.array([[0.0, 299.0], [0.0, 299.0]]), np.array([[0.0, 0.0], [256.0, 256.0]])      # one cell of 257 x 300 pixels
    xs, ys = x * 0.9 + 0.02 * y + 3.0, y * 1.05 + 0.01 * x + 1.0
    img = image_u8((280, 300), 40)
    out.append(case('one_cell_2x2_nodes', x, y, xs, ys, (257, 300), img))
    for dr in (-1, 0, 1):                                                 # the clipped box ends one short of, on and one past a tile
        out.append(case('one_cell_tiles%+d' % dr, x, y, xs, ys, (4 * TR + dr, 2 * TC + dr), img, order=(dr + 1) % 2))
    x, y = node_grid(9, 13, 0.3, 0.3, r0=5.1, c0=7.2, jitter=0.2, seed=41)                      # cells smaller than a pixel
    xs, ys = smooth_source(x, y, 41, amp=0.5)
    out.append(case('subpixel_cells', x, y, xs, ys, (12, 16), image_u8((12, 16), 41)))
    for k, (r0, c0) in enumerate(((-20, 10), (10, -25), (45, 10), (10, 60), (-200, 10), (10, -300), (90, 10), (10, 130))):
        x, y = node_grid(5, 6, 9, 11, r0=r0, c0=c0, jitter=0.2, seed=50 + k)                    # partly (first four) and wholly
        xs, ys = smooth_source(x, y, 50 + k, shift=(-c0 + 5.0, -r0 + 4.0))                      # outside the output, each side
        out.append(case('outside_%d' % k, x, y, xs, ys, (60, 80), image_u8((60, 80), 50 + k), order=k % 2))
    # ---- triangles
    x, y = node_grid(4, 5, 8, 8, r0=1, c0=1)
    x[1, 1], y[1, 1] = x[1, 2], y[1, 2]                                   # coincident nodes: degenerate triangles around them
    xs, ys = smooth_source(x, y, 60)
    out.append(case('coincident_nodes', x, y, xs, ys, (30, 40), image_u8((30, 40), 60)))
    # ---- sampling: the source leaves the image on each side, and ends exactly on its last row / column
    x, y = node_grid(4, 5, 10, 10)                                        # nodes 0..30 x 0..40, identity: sx = c, sy = r; the mesh
    img = image_u8((30, 41), 70, zeros=0.1)                               # owns rows 0..29 and columns 1..40: the image's last ones
    for order in (0, 1):
        out.append(case('last_row_col_o%d' % order, x, y, x.copy(), y.copy(), (31, 41), img, order=order, fill=7))
        for k, (sx, sy) in enumerate(((-3.5, 0.0), (3.5, 0.0), (0.0, -2.5), (0.0, 2.5), (-0.5, -0.5), (0.5, 0.5))):
            out.append(case('leaves_o%d_%d' % (order, k), x, y, x + sx, y + sy, (31, 41), img, order=order, fill=7,
                            keep_zero=bool(k % 2)))
    out.append(case('f32_last_row_col', x, y, x.copy(), y.copy(), (31, 41), image_f32((30, 41), 71), fill=np.pi))
    # ---- buffers
    x, y = node_grid(6, 7, 9, 9, r0=2, c0=2, jitter=0.2, seed=80)
    xs, ys = smooth_source(x, y, 80)
    out.append(case('maps_only', x, y, xs, ys, (50, 60), None, src_shape=(0, 0), want=('maps',)))
    out.append(case('covered_only', x, y, xs, ys, (50, 60), None, src_shape=(40, 50), want=('covered',)))
    out.append(case('image_only', x, y, xs, ys, (50, 60), image_u8((55, 66), 80), want=('out',)))
    wide = image_u8((55, 80), 81)
    out.append(case('strided_source', x, y, xs, ys, (50, 60), wide[:, 3:69], want=('out', 'covered')))
    out.append(case('empty_output', x, y, xs, ys, (0, 60), image_u8((55, 66), 80)))
    out.append(case('empty_source', x, y, xs, ys, (20, 30), np.zeros((0, 10), dtype=np.uint8), fill=5))
    out.append(case('one_row_of_nodes', x[:1], y[:1], xs[:1], ys[:1], (20, 30), image_u8((20, 30), 82), fill=3))
    return out


CASES = _cases()
NAMES = [c['name'] for c in CASES]
BY_NAME = dict(zip(NAMES, CASES))
assert len(BY_NAME) == len(CASES)

_expected = {}


def expected(name):
    """The specification's result of a case, computed once and shared (read-only)."""
    if name not in _expected:
        from tests import warp_spec as ws
        c = BY_NAME[name]
        res = ws.warp(c['x'], c['y'], c['xs'], c['ys'], c['valid'], c['diagonal'], c['out_shape'], image=c['image'],
                      src_shape=c['src_shape'], order=c['order'], fill=c['fill'], keep_zero=c['keep_zero'] and c['order'] == 1)
        for v in res.values():
            if v is not None:
                v.setflags(write=False)
        _expected[name] = res
    return _expected[name]


def check(got, name, what):
    """got = (out, covered, map_x, map_y), None where not asked for: bit for bit the specification's."""
    from tests import warp_spec as ws
    exp, want = expected(name), BY_NAME[name]['want']
    for key, g, wanted in (('out', got[0], 'out' in want), ('covered', got[1], 'covered' in want),
                           ('map_x', got[2], 'maps' in want), ('map_y', got[3], 'maps' in want)):
        if not wanted:
            assert g is None, '%s %s: %s was not asked for' % (name, what, key)
            continue
        assert g is not None and g.dtype == exp[key].dtype and g.shape == exp[key].shape, '%s %s: %s' % (name, what, key)
        if not ws.same_bits(g, exp[key]):
            gb = np.ascontiguousarray(g).view(np.uint8).reshape(g.shape + (g.itemsize,))
            eb = np.ascontiguousarray(exp[key]).view(np.uint8).reshape(g.shape + (g.itemsize,))
            diff = np.argwhere((gb != eb).any(-1))
            raise AssertionError('%s %s: %s differs from the specification at %d pixels, first %s (got %r, expected %r)'
                                 % (name, what, key, len(diff), diff[0].tolist(), g[tuple(diff[0])], exp[key][tuple(diff[0])]))
