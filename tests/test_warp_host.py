"""CPU tests of include/sid_warp.h (libwarp.warp_image, libwarp.warp_maps): the host instance of the kernels' source
(device = -1) against the specification (tests/warp_spec.py) bit for bit, the specification against matplotlib and SciPy, the
ownership rule (single owner, watertight), exact cases, keep_zero at zero weights, every argument error, the exported symbols
and the synthetic pair."""
import ctypes
import os
import re

import numpy as np
import pytest

from sea_ice_drift_amd import _capi, libwarp, synthetic
from tests import warp_cases as wc
from tests import warp_spec as ws

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VP = ctypes.c_void_p
ERR_ARG, ERR_UNSUPPORTED = -1, -4          # checked against include/sid_pm.h below


def vp(a):
    return VP(a.ctypes.data) if a is not None else None


def raw_call(device, x, y, xs, ys, valid, grid, src, dtype, src_shape, src_stride, out_shape, order, fill, diagonal, flags,
             out, out_stride, covered, map_x, map_y):
    """sid_warp_image with every argument as given (arrays or None)."""
    f64p = ctypes.POINTER(ctypes.c_double)
    nodes = [a.ctypes.data_as(f64p) if a is not None else None for a in (x, y, xs, ys)]
    return _capi.lib().sid_warp_image(device, *nodes, valid.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)) if valid is not None else None,
                                      grid[0], grid[1], vp(src), dtype, src_shape[0], src_shape[1], src_stride,
                                      out_shape[0], out_shape[1], order, fill, diagonal, flags, vp(out), out_stride, vp(covered),
                                      vp(map_x), vp(map_y))


def host_case(c, pad=5):
    """A case through sid_warp_image(device = -1) into poisoned outputs, `out` with rows `pad` elements longer than the image's.
    -> out, covered, map_x, map_y (None where the case does not want them), and the padding of out."""
    x, y, xs, ys = [np.ascontiguousarray(c[k]) for k in ('x', 'y', 'xs', 'ys')]
    img, (ro, co) = c['image'], c['out_shape']
    dtype = img.dtype if img is not None else np.dtype(np.uint8)
    wide = np.full((ro, co + pad), 113, dtype=dtype) if 'out' in c['want'] else None
    covered = np.full((ro, co), 7, dtype=np.uint8) if 'covered' in c['want'] else None
    map_x = np.full((ro, co), -12345.678, dtype=np.float32) if 'maps' in c['want'] else None
    map_y = np.full((ro, co), -12345.678, dtype=np.float32) if 'maps' in c['want'] else None
    stride = 0 if img is None else img.strides[0] // img.itemsize if img.shape[0] > 1 else img.shape[1]
    rc = raw_call(-1, x, y, xs, ys, c['valid'], x.shape, img, _capi.WARP_DTYPES[str(dtype)], c['src_shape'], stride, (ro, co),
                  c['order'], float(c['fill']), _capi.GRID_DIAGONALS[c['diagonal']], 1 if c['keep_zero'] else 0,
                  wide, co + pad, covered, map_x, map_y)
    assert rc == 0, _capi.lib().sid_warp_last_error()
    return (wide[:, :co] if wide is not None else None, covered, map_x, map_y), (wide[:, co:] if wide is not None else None)


# ---------------------------------------------------------------- host instance against the specification
@pytest.mark.parametrize('name', wc.NAMES)
def test_host_instance_equals_spec(name):
    got, padding = host_case(wc.BY_NAME[name])
    wc.check(got, name, 'host instance')
    if padding is not None:
        assert (padding == 113).all(), 'the bytes between cols_o and out_stride were written'


def test_cases_cover_what_they_claim():
    e = wc.expected
    assert e('subpixel_cells')['owners'].sum() > 0 and (e('subpixel_cells')['triangles'][..., 0] >= 0).all()
    assert all(e('outside_%d' % k)['owners'].sum() > 0 for k in range(4)) and not any(e('outside_%d' % k)['owners'].sum() for k in range(4, 8))
    t = e('coincident_nodes')['triangles'].reshape(-1, 3)
    c = wc.BY_NAME['coincident_nodes']
    xf, yf = c['x'].ravel(), c['y'].ravel()
    det = [(xf[b] - xf[a]) * (yf[q] - yf[a]) - (xf[q] - xf[a]) * (yf[b] - yf[a]) for a, b, q in t]
    assert sum(d == 0 for d in det) >= 2
    for diag in ('shorter', 'main', 'anti'):
        t = e('holed_' + diag)['triangles']
        assert ((t[..., 0, 0] >= 0) & (t[..., 1, 0] < 0)).any() and (t[..., 0, 0] < 0).any()           # one triangle, none
    assert not np.array_equal(e('curvi_frac_main')['triangles'], ws.gs.grid_triangles(
        wc.BY_NAME['curvi_frac_main']['x'], wc.BY_NAME['curvi_frac_main']['y'], np.ones((9, 13), bool), 'shorter'))
    for order in (0, 1):
        cov = e('last_row_col_o%d' % order)['covered']
        assert cov[29, 1:].all() and cov[:30, 40].all() and not cov[30].any() and not cov[:, 0].any()
        for k in range(4):
            cov = e('leaves_o%d_%d' % (order, k))
            assert 0 < cov['covered'].sum() < (cov['owners'] > 0).sum()
    assert e('one_cell_2x2_nodes')['owners'].sum() > 4 * wc.TR * wc.TC


# ---------------------------------------------------------------- the specification against matplotlib and SciPy
GRIDS = [n for n in wc.NAMES if n.startswith(('regular', 'curvi', 'holed'))]
# Largest |difference| measured between the two on these cases: 4.263e-14 pixels (source positions of about 100) and
# 8.527e-14 grey levels (values of about 250); the bounds are ten times that.
TOL_POSITION = 10 * 4.263e-14
TOL_VALUE = 10 * 8.527e-14


@pytest.mark.parametrize('name', GRIDS)
def test_spec_positions_against_matplotlib(name):
    tri_mod = pytest.importorskip('matplotlib.tri')
    c, e = wc.BY_NAME[name], wc.expected(name)
    t = e['triangles'].reshape(-1, 3)
    t = t[t[:, 0] >= 0]
    flat = [np.where(np.isfinite(c[k].ravel()), c[k].ravel(), -1000.0) for k in ('x', 'y', 'xs', 'ys')]     # (unusable: in no triangle)
    tri = tri_mod.Triangulation(flat[0], flat[1], t)
    rr, cc = np.nonzero(e['owners'])
    assert len(rr) > 1000
    for key, z in (('sx', flat[2]), ('sy', flat[3])):
        ref = tri_mod.LinearTriInterpolator(tri, z)(cc.astype(np.float64), rr.astype(np.float64))
        assert not np.ma.getmaskarray(ref).any(), 'an owned pixel lies in no triangle of matplotlib'
        worst = np.abs(np.ma.filled(ref) - e[key][rr, cc]).max()
        print(name, key, 'max |spec - matplotlib| = %.3e' % worst)
        assert worst <= TOL_POSITION


@pytest.mark.parametrize('name', [n for n in GRIDS if wc.BY_NAME[n]['order'] == 1])
def test_spec_bilinear_against_scipy(name):
    nd = pytest.importorskip('scipy.ndimage')
    c, e = wc.BY_NAME[name], wc.expected(name)
    cov = e['covered'] > 0
    ref = nd.map_coordinates(c['image'].astype(np.float64), [e['sy'][cov], e['sx'][cov]], order=1, mode='nearest')
    worst = np.abs(ref - e['v'][cov]).max()
    print(name, 'max |spec - scipy| = %.3e' % worst)
    assert cov.sum() > 1000 and worst <= TOL_VALUE


# ---------------------------------------------------------------- ownership
def live_triangles(c, e):
    xf, yf = c['x'].ravel(), c['y'].ravel()
    out = []
    for a, b, q in e['triangles'].reshape(-1, 3):
        if a >= 0 and (xf[b] - xf[a]) * (yf[q] - yf[a]) - (xf[q] - xf[a]) * (yf[b] - yf[a]) > 0:
            out.append((int(a), int(b), int(q)))
    return xf, yf, out


@pytest.mark.parametrize('name', GRIDS)
def test_single_owner_and_watertight(name):
    """No pixel has two owners; an unowned pixel inside some closed triangle lies on an edge that one triangle alone uses, or
    on a node that touches such an edge."""
    c, e = wc.BY_NAME[name], wc.expected(name)
    assert e['owners'].max() == 1
    xf, yf, tris = live_triangles(c, e)
    uses = {}
    for a, b, q in tris:
        for p, r in ((a, b), (b, q), (q, a)):
            uses[(min(p, r), max(p, r))] = uses.get((min(p, r), max(p, r)), 0) + 1
    border_nodes = set(n for edge, k in uses.items() if k == 1 for n in edge)
    rows_o, cols_o = c['out_shape']
    rr, cc = np.meshgrid(np.arange(rows_o), np.arange(cols_o), indexing='ij')
    px, py = cc.astype(np.float64), rr.astype(np.float64)
    excused = np.zeros((rows_o, cols_o), dtype=bool)
    closed = np.zeros((rows_o, cols_o), dtype=bool)
    for a, b, q in tris:
        inside, on_border = np.ones((rows_o, cols_o), dtype=bool), np.zeros((rows_o, cols_o), dtype=bool)
        for p, r in ((a, b), (b, q), (q, a)):
            lo, hi = min(p, r), max(p, r)
            E = (xf[hi] - xf[lo]) * (py - yf[lo]) - (yf[hi] - yf[lo]) * (px - xf[lo])
            Ed = E if p == lo else -E
            inside &= Ed >= 0
            if uses[(lo, hi)] == 1:
                on_border |= Ed == 0
        for n in (a, b, q):
            if n in border_nodes:
                on_border |= (px == xf[n]) & (py == yf[n])
        closed |= inside
        excused |= inside & on_border
    leak = closed & (e['owners'] == 0) & ~excused
    assert closed.sum() > 1000 and not leak.any(), 'unowned pixels inside the mesh: %s' % np.argwhere(leak)[:5].tolist()


def test_regular_grid_owns_the_half_open_hull():
    """7 x 9 nodes 5 and 6 pixels apart span 31 x 49 pixel centres.  Counter-clockwise, the edge along row 0 runs towards +x and
    the one along column 48 towards +y: pixels on them are inside; those on row 30 and column 0 are not.  30 x 48 pixels."""
    owners = wc.expected('regular_u8_o1')['owners']
    exp = np.zeros(owners.shape, dtype=np.int32)
    exp[0:30, 1:49] = 1
    assert np.array_equal(owners, exp) and owners.sum() == 30 * 48


# ---------------------------------------------------------------- exact cases
def host_warp(image, x, y, xs, ys, out_shape, order=1, fill=0, keep_zero=False, diagonal='shorter'):
    c = wc.case('adhoc', x, y, xs, ys, out_shape, image, order=order, fill=fill, keep_zero=keep_zero, diagonal=diagonal)
    (out, covered, _, _), _ = host_case(c)
    return out, covered


@pytest.mark.parametrize('dtype', ['uint8', 'float32'])
@pytest.mark.parametrize('order', [0, 1])
def test_identity_and_integer_translation(dtype, order):
    img = wc.image_u8((40, 50), 5) if dtype == 'uint8' else wc.image_f32((40, 50), 5)
    x, y = wc.node_grid(5, 6, 8, 8, r0=2, c0=3, jitter=0.25, integer=True, seed=5)
    out, covered = host_warp(img, x, y, x.copy(), y.copy(), (40, 50), order=order)
    assert covered.sum() > 800 and np.array_equal(out[covered > 0], img[covered > 0]) and not out[covered == 0].any()
    out, covered = host_warp(img, x, y, x + 4.0, y - 2.0, (40, 50), order=order, fill=1)
    rr, cc = np.nonzero(covered)
    assert len(rr) > 800 and np.array_equal(out[rr, cc], img[rr - 2, cc + 4]) and (out[covered == 0] == 1).all()


def test_half_pixel_translation_gives_two_tap_means_with_ties_to_even():
    img = wc.image_u8((40, 50), 6)
    x, y = wc.node_grid(5, 6, 8, 8, r0=2, c0=3)
    out, covered = host_warp(img, x, y, x + 0.5, y.copy(), (40, 50))
    rr, cc = np.nonzero(covered)
    pair = img[rr, cc].astype(np.int64) + img[rr, cc + 1]
    exp = pair // 2 + ((pair % 2 == 1) & ((pair // 2) % 2 == 1))               # x.5 goes to the even neighbour
    assert len(rr) > 800 and (pair % 2 == 1).sum() > 100 and np.array_equal(out[rr, cc], exp)
    out, covered = host_warp(img, x, y, x.copy(), y + 0.5, (40, 50))
    rr, cc = np.nonzero(covered)
    pair = img[rr, cc].astype(np.int64) + img[rr + 1, cc]
    assert np.array_equal(out[rr, cc], pair // 2 + ((pair % 2 == 1) & ((pair // 2) % 2 == 1)))


def test_keep_zero_counts_only_taps_with_weight():
    img = np.full((20, 20), 100, dtype=np.uint8)
    img[:, 10] = 0                                                             # one invalid column
    x, y = wc.node_grid(2, 2, 19, 19)
    out, covered = host_warp(img, x, y, x.copy(), y.copy(), (20, 20), keep_zero=True)          # integer sx: fx = 0
    assert covered[:19, 1:].all() and (out[:19, 9] == 100).all() and (out[:19, 11] == 100).all() and (out[:19, 10] == 0).all()
    out, covered = host_warp(img, x, y, x + 0.25, y.copy(), (20, 20), keep_zero=True)          # between valid and invalid: 0
    assert (out[:19, 9] == 0).all() and (out[:19, 10] == 0).all() and (out[:19, 8] == 100).all() and (out[:19, 11] == 100).all()
    out, covered = host_warp(img, x, y, x + 0.25, y.copy(), (20, 20), keep_zero=False)
    assert (out[:19, 9] == 75).all() and (out[:19, 10] == 25).all()
    img[:, 10] = 100
    img[10, :] = 0                                                             # and the same along rows
    out, covered = host_warp(img, x, y, x.copy(), y.copy(), (20, 20), keep_zero=True)
    assert (out[9, 1:] == 100).all() and (out[11, 1:] == 100).all() and (out[10, 1:] == 0).all()
    out, covered = host_warp(img, x, y, x.copy(), y + 0.5, (20, 20), keep_zero=True)
    assert (out[9, 1:] == 0).all() and (out[10, 1:] == 0).all() and (out[8, 1:] == 100).all()


# ---------------------------------------------------------------- argument errors
def good_args():
    x, y = wc.node_grid(3, 4, 5, 5)
    img = wc.image_u8((12, 17), 1)
    return dict(device=-1, x=x, y=y, xs=x.copy(), ys=y.copy(), valid=None, grid=x.shape, src=img, dtype=0, src_shape=img.shape,
                src_stride=17, out_shape=(11, 16), order=1, fill=0.0, diagonal=0, flags=1, out=np.zeros((11, 16), np.uint8),
                out_stride=16, covered=np.zeros((11, 16), np.uint8), map_x=np.zeros((11, 16), np.float32),
                map_y=np.zeros((11, 16), np.float32))


BIG = np.zeros(4, dtype=np.uint8)
HEADER_ERRORS = [
    ('null x', dict(x=None), ERR_ARG), ('null y', dict(y=None), ERR_ARG), ('null xs', dict(xs=None), ERR_ARG),
    ('null ys', dict(ys=None), ERR_ARG),
    ('no output', dict(out=None, covered=None, map_x=None, map_y=None), ERR_ARG),
    ('out without source', dict(src=None), ERR_ARG),
    ('negative grid rows', dict(grid=(-1, 4)), ERR_ARG), ('negative grid cols', dict(grid=(3, -4)), ERR_ARG),
    ('negative source rows', dict(src_shape=(-1, 17)), ERR_ARG), ('negative source cols', dict(src_shape=(12, -1)), ERR_ARG),
    ('negative output rows', dict(out_shape=(-1, 16)), ERR_ARG), ('negative output cols', dict(out_shape=(11, -1)), ERR_ARG),
    ('source stride', dict(src_stride=16), ERR_ARG), ('output stride', dict(out_stride=15), ERR_ARG),
    ('order', dict(order=2), ERR_ARG), ('order negative', dict(order=-1), ERR_ARG), ('diagonal', dict(diagonal=3), ERR_ARG),
    ('flag', dict(flags=2), ERR_ARG), ('dtype', dict(dtype=2), ERR_ARG),
    ('keep_zero with float32', dict(dtype=1, src=np.zeros((12, 17), np.float32), out=np.zeros((11, 16), np.float32)), ERR_ARG),
    ('fill 256', dict(fill=256.0), ERR_ARG), ('fill -1', dict(fill=-1.0), ERR_ARG), ('fill 0.5', dict(fill=0.5), ERR_ARG),
    ('fill nan', dict(fill=float('nan')), ERR_ARG),
    ('grid too large', dict(grid=(1 << 16, 1 << 15)), ERR_UNSUPPORTED),
    ('source axis too large', dict(src_shape=(12, 1 << 31), src_stride=1 << 31), ERR_UNSUPPORTED),
    ('output axis too large', dict(out_shape=(1 << 31, 16)), ERR_UNSUPPORTED),
]


@pytest.mark.parametrize('what,change,code', HEADER_ERRORS, ids=[h[0] for h in HEADER_ERRORS])
def test_header_argument_errors(what, change, code):
    header = open(os.path.join(ROOT, 'include', 'sid_pm.h')).read()
    assert re.search(r'SID_PM_ERR_ARG\s+\(?-1\)?', header) and re.search(r'SID_PM_ERR_UNSUPPORTED\s+\(?-4\)?', header)
    assert raw_call(**good_args()) == 0
    args = good_args()
    args.update(change)
    assert raw_call(**args) == code, what
    assert _capi.lib().sid_warp_last_error()
    args['device'] = 0                                     # found before any device call: the same without a GPU
    assert raw_call(**args) == code, what


def test_header_refuses_overlap_and_takes_float_fill():
    args = good_args()
    buf = np.zeros((30, 17), dtype=np.uint8)
    args.update(src=buf, out=buf[5:], out_stride=17)
    assert raw_call(**args) == ERR_ARG and b'overlap' in _capi.lib().sid_warp_last_error()
    args.update(src=buf[:12], out=buf[12:])                                    # adjacent is fine
    assert raw_call(**args) == 0
    args = good_args()
    args.update(dtype=1, flags=0, fill=-0.5, src=np.zeros((12, 17), np.float32), out=np.zeros((11, 16), np.float32))
    assert raw_call(**args) == 0 and (args['out'][10] == np.float32(-0.5)).all()


def test_degenerate_sizes_fill_the_outputs():
    args = good_args()
    for change in (dict(grid=(1, 4)), dict(grid=(3, 1)), dict(grid=(0, 0))):
        a = dict(args, **change)
        a.update(fill=9.0, out=np.zeros((11, 16), np.uint8), covered=np.ones((11, 16), np.uint8))
        assert raw_call(**a) == 0
        assert (a['out'] == 9).all() and not a['covered'].any() and np.isnan(a['map_x']).all() and np.isnan(a['map_y']).all()
    assert raw_call(**dict(args, out_shape=(0, 16))) == 0 and raw_call(**dict(args, out_shape=(11, 0), out_stride=0)) == 0


def test_python_argument_errors():
    x, y = wc.node_grid(3, 4, 5, 5)
    img = wc.image_u8((12, 17), 1)
    ok = dict(image=img, x=x, y=y, xs=x.copy(), ys=y.copy(), device=-1)

    def call(**change):
        return libwarp.warp_image(**dict(ok, **change))
    assert call().shape == (12, 17)
    for name in ('x', 'y', 'xs', 'ys'):
        with pytest.raises(NotImplementedError, match=r'\b%s is float32' % name):
            call(**{name: ok[name].astype(np.float32)})
        with pytest.raises(ValueError, match='x, y, xs, ys must be 2-D arrays of one shape'):
            call(**{name: ok[name][:, :3]})
    with pytest.raises(ValueError, match='x, y, xs, ys must be 2-D'):
        call(x=x.ravel(), y=y.ravel(), xs=x.ravel(), ys=y.ravel())
    with pytest.raises(TypeError, match='valid is float64'):
        call(valid=np.ones(x.shape))
    with pytest.raises(ValueError, match='valid must have the shape'):
        call(valid=np.ones((3, 3), dtype=bool))
    with pytest.raises(TypeError, match='image is float64'):
        call(image=img.astype(np.float64))
    with pytest.raises(ValueError, match='image must be 2-D'):
        call(image=img[0])
    with pytest.raises(ValueError, match='image is None'):
        call(image=None)
    with pytest.raises(ValueError, match='order must be 0'):
        call(order=2)
    with pytest.raises(ValueError, match='diagonal must be'):
        call(diagonal='both')
    with pytest.raises(ValueError, match='fill must be a uint8 value'):
        call(fill=300)
    with pytest.raises(ValueError, match='fill must be a uint8 value'):
        call(fill=0.5)
    with pytest.raises(ValueError, match='keep_zero is for uint8'):
        call(image=img.astype(np.float32), keep_zero=True)
    for bad in ((3,), (3, 4, 5), (-1, 4), (2.5, 4), 'ab', 7):
        with pytest.raises(ValueError, match='out_shape'):
            call(out_shape=bad)
    with pytest.raises(ValueError, match='out_shape'):
        libwarp.warp_maps(x, y, x, y, None, device=-1)
    torch = pytest.importorskip('torch')
    with pytest.raises(TypeError, match='not a mix'):
        call(x=torch.from_numpy(x))
    with pytest.raises(TypeError, match='not a mix'):
        call(image=torch.from_numpy(img))
    with pytest.raises(TypeError, match='on one ROCm device'):
        libwarp.warp_maps(*[torch.from_numpy(q) for q in (x, y, x, y)], (5, 5))
    with pytest.raises(ValueError, match='device must be a HIP device index'):
        call(device=-2)


def test_python_defaults_on_the_host_instance():
    """out_shape defaults to the image's, keep_zero to the image's type, and the two functions agree with the specification."""
    c = wc.BY_NAME['curvi_int_main']
    e = ws.warp(c['x'], c['y'], c['xs'], c['ys'], None, 'shorter', c['image'].shape, image=c['image'], keep_zero=True)
    out, covered = libwarp.warp_image(c['image'], c['x'], c['y'], c['xs'], c['ys'], return_covered=True, device=-1)
    assert ws.same_bits(out, e['out']) and ws.same_bits(covered, e['covered'])
    assert ws.same_bits(libwarp.warp_image(c['image'], c['x'], c['y'], c['xs'], c['ys'], device=-1), e['out'])
    mx, my = libwarp.warp_maps(c['x'], c['y'], c['xs'], c['ys'], c['image'].shape, device=-1)
    assert ws.same_bits(mx, e['map_x']) and ws.same_bits(my, e['map_y'])
    f32 = c['image'].astype(np.float32)
    e = ws.warp(c['x'], c['y'], c['xs'], c['ys'], None, 'anti', (50, 70), image=f32, fill=2.5)
    out = libwarp.warp_image(f32, c['x'], c['y'], c['xs'], c['ys'], out_shape=(50, 70), fill=2.5, diagonal='anti', device=-1)
    assert ws.same_bits(out, e['out'])
    e = ws.warp(c['x'], c['y'], c['xs'], c['ys'], None, 'shorter', (50, 70), image=c['image'][::2, ::3], order=0, fill=4)
    out = libwarp.warp_image(c['image'][::2, ::3], c['x'], c['y'], c['xs'], c['ys'], out_shape=(50, 70), order=0, fill=4, device=-1)
    assert ws.same_bits(out, e['out'])                                          # (a view with an inner stride is copied)


# ---------------------------------------------------------------- exported symbols
def test_header_symbols_and_abi():
    header = open(os.path.join(ROOT, 'include', 'sid_warp.h')).read()
    body = re.sub(r'/\*.*?\*/', '', header, flags=re.S)
    assert sorted(set(re.findall(r'\b(sid_warp_\w+)\s*\(', body))) == sorted(_capi.WARP_SYMBOLS)
    lib = _capi.lib()
    for name in _capi.WARP_SYMBOLS:
        assert hasattr(lib, name), name
    assert lib.sid_pm_abi_version() == 6 and _capi.ABI_VERSION == 6
    assert (int(re.search(r'SID_WARP_TILE_ROWS\s+(\d+)', header).group(1)),
            int(re.search(r'SID_WARP_TILE_COLS\s+(\d+)', header).group(1))) == _capi.WARP_TILE
    assert int(re.search(r'SID_WARP_KEEP_ZERO\s+(\d+)', header).group(1)) == _capi.WARP_KEEP_ZERO
    assert {k: int(re.search(r'SID_WARP_%s\s+(\d+)' % n, header).group(1)) for k, n in (('uint8', 'U8'), ('float32', 'F32'))} == _capi.WARP_DTYPES


# ---------------------------------------------------------------- the synthetic pair
def corr(a, b, mask):
    return float(np.corrcoef(a[mask].astype(np.float64), b[mask].astype(np.float64))[0, 1])


def test_synthetic_pair_lines_up():
    """Image 2 of the synthetic pair, warped back with the true field on nodes 40 pixels apart, correlates with image 1 far
    better than it does unwarped - the specification and the host instance alike."""
    img1, img2 = synthetic.make_pair(400, 400, seed=17)
    y, x = np.meshgrid(np.arange(0.0, 400.0, 40.0), np.arange(0.0, 400.0, 40.0), indexing='ij')
    dc, dr = synthetic.true_displacement(x, y)
    for order in (0, 1):
        e = ws.warp(x, y, x + dc, y + dr, None, 'shorter', (400, 400), image=img2, order=order, keep_zero=order == 1)
        out, covered = libwarp.warp_image(img2, x, y, x + dc, y + dr, order=order, return_covered=True, device=-1)
        assert ws.same_bits(out, e['out']) and ws.same_bits(covered, e['covered'])
        mask = covered > 0
        before, after = corr(img1, img2, mask), corr(img1, out, mask)
        print('order %d: correlation %.3f unwarped, %.3f warped, %d pixels' % (order, before, after, mask.sum()))
        assert mask.sum() > 100000 and after > before


def test_get_warped_image_both_ways():
    """SeaIceDrift.get_warped_image on ArrayNansat objects with a georeference that is not the identity: `to=1` brings image 2
    into image 1's frame, `to=2` the reverse; both are libwarp.warp_image on the pixel nodes."""
    from sea_ice_drift_amd.domain import ArrayNansat
    from sea_ice_drift_amd.seaicedrift import SeaIceDrift
    img1, img2 = synthetic.make_pair(400, 400, seed=17)
    geo = dict(origin=(10.0, 70.0), matrix=((0.002, 0.0), (0.0, -0.001)))
    n1, n2 = ArrayNansat(img1, **geo), ArrayNansat(img2[:380], **geo)
    y, x = np.meshgrid(np.arange(0.0, 400.0, 40.0), np.arange(0.0, 400.0, 40.0), indexing='ij')
    dc, dr = synthetic.true_displacement(x, y)
    lons, lats = n1.transform_points(x, y, 0)
    lon2, lat2 = n2.transform_points(x + dc, y + dr, 0)
    sid = SeaIceDrift(n1, n2)
    x1, y1 = n1.transform_points(lons, lats, 1)
    x2, y2 = n2.transform_points(lon2, lat2, 1)
    out, covered = sid.get_warped_image(lons, lats, lon2, lat2, return_covered=True, device=-1)
    exp = libwarp.warp_image(img2[:380], x1, y1, x2, y2, out_shape=(400, 400), device=-1)
    assert out.shape == (400, 400) and ws.same_bits(out, exp)
    assert corr(img1, out, covered > 0) > corr(img1[:380], img2[:380], covered[:380] > 0)
    back = sid.get_warped_image(lons, lats, lon2, lat2, to=2, order=0, device=-1)
    assert back.shape == (380, 400)
    assert ws.same_bits(back, libwarp.warp_image(img1, x2, y2, x1, y1, out_shape=(380, 400), order=0, device=-1))
    with pytest.raises(ValueError, match='to must be 1 or 2'):
        sid.get_warped_image(lons, lats, lon2, lat2, to=3)
    with pytest.raises(ValueError, match='2-D grids of one shape'):
        sid.get_warped_image(lons, lats, lon2[:5], lat2)
