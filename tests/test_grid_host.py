"""CPU tests of include/sid_grid.h (libfilter.normalized_median_test, libdefor.get_deformation_grid): the specification
(tests/grid_spec.py) against the fixture and the reference, the host instance of the kernels' source (device = -1) against both
bit for bit, the triangle rule against matplotlib, every argument error, the exported symbols, and the end-to-end check."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

from oracle import ref_harness
from sea_ice_drift_amd import _capi, libdefor, libfilter
from tests import grid_spec as gs
from tests.grid_checks import assert_deformation, assert_filter, chain_check
from tests.golden import make_golden_grid as mgg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POISON = -12345.678


@pytest.fixture(scope='module')
def gold():
    return np.load(mgg.PATH)


def u8(valid):
    return None if valid is None else np.ascontiguousarray(valid).view(np.uint8)


def host_deformation(x, y, u, v, valid, diagonal):
    """sid_grid_deformation(device = -1) into poisoned outputs."""
    rows, cols = x.shape
    out = [np.full((rows - 1, cols - 1, 2), POISON) for _ in range(5)]
    t = np.full((rows - 1, cols - 1, 2, 3), 77, dtype=np.int32)
    f64p, i32p = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int32)
    ins = [np.ascontiguousarray(q) for q in (x, y, u, v)]
    vv = u8(valid)
    rc = _capi.lib().sid_grid_deformation(-1, *[q.ctypes.data_as(f64p) for q in ins],
                                          vv.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)) if vv is not None else None,
                                          rows, cols, _capi.GRID_DIAGONALS[diagonal], *[q.ctypes.data_as(f64p) for q in out],
                                          t.ctypes.data_as(i32p))
    assert rc == 0
    return tuple(out) + (t,)


def host_filter(u, v, valid, eps, threshold, radius, minn):
    keep, res = np.full(u.shape, 7, dtype=np.uint8), np.full(u.shape, POISON)
    f64p, u8p = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_uint8)
    u, v, vv = np.ascontiguousarray(u), np.ascontiguousarray(v), u8(valid)
    rc = _capi.lib().sid_grid_filter(-1, u.ctypes.data_as(f64p), v.ctypes.data_as(f64p),
                                     vv.ctypes.data_as(u8p) if vv is not None else None, u.shape[0], u.shape[1],
                                     eps, threshold, radius, minn, keep.ctypes.data_as(u8p), res.ctypes.data_as(f64p))
    assert rc == 0
    return keep, res


# ---------------------------------------------------------------- fixture
def test_fixture_inputs_regenerate_and_is_small(gold):
    shas = dict(zip(gold['names'], gold['shas']))
    assert list(gold['names']) == list(mgg.DEFOR_CASES) + list(mgg.FILTER_CASES)
    for name in mgg.DEFOR_CASES:
        assert mgg.input_sha(mgg.defor_inputs(name)[:5]) == shas[name], name
    for name in mgg.FILTER_CASES:
        assert mgg.input_sha(mgg.filter_inputs(name)[:3]) == shas[name], name
    assert os.path.getsize(mgg.PATH) < 200 * 1024


def test_fixture_covers_what_it_claims(gold):
    """The cases are there for a reason each: check that the reason holds."""
    assert (gold['regular_t'][:, :, 0, 2] == gold['regular_t'][:, :, 1, 1]).all()                  # main split: E in both slots
    for name in ('shear_p_ydown', 'shear_m_ydown'):                                                 # y falling: every triangle swapped
        xd, yd, ud, vd, valid, diag = mgg.defor_inputs(name)
        unswapped = gs.grid_triangles(xd, -yd, np.ones(xd.shape, bool), diag)
        assert np.array_equal(unswapped[..., [0, 2, 1]], gold[name + '_t'])
    assert sorted(int((gold['p2x2_%02d_t' % k][..., 0] >= 0).sum()) for k in range(16)) == [0] * 11 + [1] * 4 + [2]
    out = gold['coincident_out']
    assert np.isnan(out[0]).sum() == 2 and (out[3][np.isnan(out[0])] == 0).all()                  # area 0, NaN deformation
    assert not np.array_equal(gold['pm_main_t'], gold['pm_anti_t'])
    assert (gold['pm_curvi_t'][..., 1, 0] < 0).any() and (gold['pm_curvi_t'][..., 0, 0] < 0).any()  # one triangle, none
    for name in ('quant_r1_m3', 'quant_r2_m3'):                                                     # mu = 0: res = |u - um| / eps
        res = gold[name + '_res']
        assert (res == 0).any() and (res[np.isfinite(res)] >= 5.0 - 1e-9).any()
    assert np.isnan(gold['all_invalid_res']).all() and not gold['all_invalid_keep'].any()
    assert np.isnan(gold['isolated_res'][3, 3]) and np.isfinite(gold['isolated_res'][0, :2]).all()
    for name in ('huge_r1', 'huge_r2'):                                                             # overflowing differences
        res = gold[name + '_res']
        assert np.isinf(res).any() and np.isnan(res).any() and np.isfinite(res).any()


@pytest.mark.parametrize('name', mgg.DEFOR_CASES)
def test_deformation_spec_and_host_instance_equal_fixture(gold, name):
    x, y, u, v, valid, diagonal = mgg.defor_inputs(name)
    exp = gs.scatter(gold[name + '_t'], gold[name + '_out']) + (gold[name + '_t'],)
    assert_deformation(gs.deformation(x, y, u, v, valid, diagonal), exp, name + ' spec')
    assert_deformation(host_deformation(x, y, u, v, valid, diagonal), exp, name + ' host instance')


@pytest.mark.parametrize('name', list(mgg.FILTER_CASES))
def test_filter_spec_and_host_instance_equal_fixture(gold, name):
    args = mgg.filter_inputs(name)
    exp = (gold[name + '_keep'], gold[name + '_res'])
    assert_filter(gs.nmt(*args), exp, name + ' spec')
    assert_filter(host_filter(*args), exp, name + ' host instance')


@pytest.mark.skipif(not ref_harness.available(), reason='the reference tree is not on this machine')
def test_fixture_regenerates_from_reference(gold):
    pytest.importorskip('matplotlib.tri')
    modules, path = dict(sys.modules), list(sys.path)
    try:
        fresh = mgg.compute(mgg.reference_libdefor())
    finally:                                    # the harness's stub modules (nansat, cv2, osgeo) must not reach later tests
        for name in [k for k in sys.modules if k not in modules]:
            del sys.modules[name]
        sys.path[:] = path
    assert sorted(fresh) == sorted(gold.files)
    for key, val in fresh.items():
        if val.dtype.kind == 'f':
            assert gs.same_bits(val, gold[key]), key
        else:
            assert val.dtype == gold[key].dtype and np.array_equal(val, gold[key]), key


# ---------------------------------------------------------------- random fields: host instance against the spec
@pytest.mark.parametrize('rows,cols,radius,seed', [(1, 1, 1, 1), (1, 12, 2, 2), (12, 1, 1, 3), (2, 2, 2, 4), (9, 33, 1, 5), (10, 34, 2, 6)])
def test_host_instance_random_against_spec(rows, cols, radius, seed):
    rng = np.random.default_rng(seed)
    _, _, x, y = mgg.pm_geometry(rows, cols)
    u, v = np.round(rng.standard_normal((rows, cols)), 1), np.round(rng.standard_normal((rows, cols)), 1)
    valid = rng.random((rows, cols)) >= 0.3
    u[rng.random((rows, cols)) < 0.05] = np.nan
    x[rng.random((rows, cols)) < 0.03] = np.nan                  # unusable for the deformation alone
    y[rng.random((rows, cols)) < 0.03] = -np.inf
    for minn in (1, 4):
        assert_filter(host_filter(u, v, valid, 0.1, 2.0, radius, minn), gs.nmt(u, v, valid, 0.1, 2.0, radius, minn), 'filter')
    if rows >= 2 and cols >= 2:
        for diagonal in ('shorter', 'main', 'anti'):
            assert_deformation(host_deformation(x, y, u, v, valid, diagonal), gs.deformation(x, y, u, v, valid, diagonal), diagonal)


# ---------------------------------------------------------------- the triangle rule against matplotlib
def canonical(tris):
    """Triangles as a set, each rotated to start at its smallest node: the cyclic order - the orientation - still counts."""
    return {tuple(int(q) for q in np.roll(t, -int(np.argmin(t)))) for t in tris}


@pytest.mark.parametrize('name', list(mgg.SHEARED))
def test_triangles_on_sheared_grids_are_matplotlibs(gold, name):
    tri = pytest.importorskip('matplotlib.tri')
    x, y = mgg.defor_inputs(name)[:2]
    _, mine = gs.present(gold[name + '_t'])
    assert canonical(mine) == canonical(tri.Triangulation(x.ravel(), y.ravel()).triangles)


# ---------------------------------------------------------------- argument errors of the C ABI (before any device call)
def c_filter(u='ok', v='ok', rows=3, cols=4, eps=0.1, threshold=2.0, radius=1, minn=3, keep='ok', res='ok', device=0):
    a = np.zeros(12)
    k = np.zeros(12, dtype=np.uint8)
    f64p, u8p = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_uint8)
    p = lambda s, arr, ty: arr.ctypes.data_as(ty) if s == 'ok' else None          # noqa: E731
    return _capi.lib().sid_grid_filter(device, p(u, a, f64p), p(v, a, f64p), None, rows, cols, eps, threshold, radius, minn,
                                       p(keep, k, u8p), p(res, a, f64p))


def c_deformation(null=None, rows=3, cols=4, diagonal=0, device=0):
    a = np.zeros(12)
    o = np.zeros(12)
    t = np.zeros(36, dtype=np.int32)
    f64p = ctypes.POINTER(ctypes.c_double)
    ptrs = [a.ctypes.data_as(f64p)] * 4 + [None, rows, cols, diagonal] + [o.ctypes.data_as(f64p)] * 5 + [t.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))]
    if null is not None:
        ptrs[null] = None
    return _capi.lib().sid_grid_deformation(device, *ptrs)


ERR_ARG, ERR_UNSUPPORTED = -1, -4


def test_c_abi_argument_errors():
    lib = _capi.lib()
    assert lib.sid_pm_strerror(ERR_UNSUPPORTED) == b'unsupported option or size'
    for kw in (dict(u=None), dict(v=None), dict(keep=None), dict(res=None),
               dict(eps=0.0), dict(eps=-1.0), dict(eps=np.nan), dict(eps=np.inf),
               dict(threshold=0.0), dict(threshold=-2.0), dict(threshold=np.nan), dict(threshold=np.inf),
               dict(radius=0), dict(radius=3), dict(radius=-1), dict(minn=0), dict(minn=9), dict(radius=2, minn=25), dict(minn=-1),
               dict(rows=-1)):
        for device in (0, -1):
            assert c_filter(device=device, **kw) == ERR_ARG, kw
            assert lib.sid_grid_last_error()
    assert c_filter(radius=2, minn=24, device=-1) == 0 and c_filter(minn=8, device=-1) == 0
    for null in (0, 1, 2, 3, 8, 9, 10, 11, 12, 13):
        assert c_deformation(null=null) == ERR_ARG and c_deformation(null=null, device=-1) == ERR_ARG
    for diagonal in (-1, 3, 100):
        assert c_deformation(diagonal=diagonal) == ERR_ARG and c_deformation(diagonal=diagonal, device=-1) == ERR_ARG
    assert c_deformation(rows=-3) == ERR_ARG
    for rows, cols in ((1 << 16, 1 << 15), (1 << 31, 1), (3, 1 << 62), (1 << 40, 1 << 40)):
        assert c_filter(rows=rows, cols=cols) == ERR_UNSUPPORTED and c_deformation(rows=rows, cols=cols) == ERR_UNSUPPORTED
        assert b'2^31' in lib.sid_grid_last_error()
    vp = ctypes.c_void_p
    one = vp(16)                                 # never dereferenced: the checks come first
    assert lib.sid_grid_filter_device(one, one, None, 3, 4, 0.0, 2.0, 1, 3, one, one, None) == ERR_ARG
    assert lib.sid_grid_filter_device(one, None, None, 3, 4, 0.1, 2.0, 1, 3, one, one, None) == ERR_ARG
    assert lib.sid_grid_filter_device(one, one, None, 1 << 20, 1 << 20, 0.1, 2.0, 1, 3, one, one, None) == ERR_UNSUPPORTED
    assert lib.sid_grid_deformation_device(one, one, one, one, None, 3, 4, 5, one, one, one, one, one, one, None) == ERR_ARG
    assert lib.sid_grid_deformation_device(one, one, one, one, None, 3, 4, 0, one, one, one, one, one, None, None) == ERR_ARG
    assert lib.sid_grid_deformation_device(one, one, one, one, None, 1 << 31, 4, 0, one, one, one, one, one, one, None) == ERR_UNSUPPORTED


def test_c_abi_empty_and_thin_grids_are_valid_calls():
    """Nothing to write for the deformation; the filter judges nobody who has fewer than min_neighbours neighbours.  The
    device entry points return before any device call too."""
    assert c_filter(rows=0, cols=4) == 0 and c_filter(rows=3, cols=0) == 0 and c_filter(rows=0, cols=0, device=-1) == 0
    for rows, cols in ((0, 0), (1, 12), (12, 1), (0, 5), (1, 1)):
        assert c_deformation(rows=rows, cols=cols) == 0 and c_deformation(rows=rows, cols=cols, device=-1) == 0
    lib, one = _capi.lib(), ctypes.c_void_p(16)
    assert lib.sid_grid_filter_device(one, one, None, 0, 4, 0.1, 2.0, 1, 3, one, one, None) == 0
    assert lib.sid_grid_deformation_device(one, one, one, one, None, 1, 4, 0, one, one, one, one, one, one, None) == 0
    keep, res = host_filter(np.ones((1, 1)), np.ones((1, 1)), None, 0.1, 2.0, 1, 1)
    assert keep[0, 0] == 0 and np.isnan(res[0, 0])
    assert lib.sid_grid_release(-1) == 0 and lib.sid_grid_release(0) == 0           # nothing cached: no device call either


# ---------------------------------------------------------------- argument errors of the Python API
def grids(rows=4, cols=5, n=4):
    rng = np.random.default_rng(0)
    return [rng.standard_normal((rows, cols)) for _ in range(n)]


def test_python_value_errors():
    u, v = grids(n=2)
    for kw in (dict(eps=0.0), dict(eps=-0.1), dict(eps=np.nan), dict(eps=np.inf), dict(eps=0.1, threshold=0.0),
               dict(eps=0.1, threshold=np.nan), dict(eps=0.1, radius=0), dict(eps=0.1, radius=3), dict(eps=0.1, radius=1.5),
               dict(eps=0.1, min_neighbours=0), dict(eps=0.1, min_neighbours=9), dict(eps=0.1, radius=2, min_neighbours=25),
               dict(eps=0.1, min_neighbours=2.5), dict(eps=0.1, device=-1)):
        with pytest.raises(ValueError, match='libfilter'):
            libfilter.normalized_median_test(u, v, **kw)
    with pytest.raises(TypeError):
        libfilter.normalized_median_test(u, v)                                      # eps has no default
    x, y, u, v = grids()
    for diagonal in ('Shorter', 'delaunay', 0, None):
        with pytest.raises(ValueError, match='diagonal'):
            libdefor.get_deformation_grid(x, y, u, v, diagonal=diagonal)
    with pytest.raises(ValueError, match='device'):
        libdefor.get_deformation_grid(x, y, u, v, device=-1)


def test_python_shapes():
    x, y, u, v = grids()
    for bad in ((x.ravel(), y.ravel(), u.ravel(), v.ravel()), (x, y[:-1], u, v), (x, y, u, v[:, :3]), (x[None], y[None], u[None], v[None])):
        with pytest.raises(ValueError, match='2-D'):
            libdefor.get_deformation_grid(*bad)
    for bad in ((u.ravel(), v.ravel()), (u, v.T), (u[None], v[None])):
        with pytest.raises(ValueError, match='2-D'):
            libfilter.normalized_median_test(*bad, 0.1)
    for valid in (np.ones((4, 4), dtype=bool), np.ones(20, dtype=np.uint8)):
        with pytest.raises(ValueError, match='valid'):
            libfilter.normalized_median_test(u, v, 0.1, valid=valid)
        with pytest.raises(ValueError, match='valid'):
            libdefor.get_deformation_grid(x, y, u, v, valid=valid)


@pytest.mark.parametrize('dtype', [np.float32, np.int64, np.complex128])
def test_python_dtypes(dtype):
    for k in range(4):
        args = grids()
        args[k] = args[k].astype(dtype)
        with pytest.raises(NotImplementedError, match='only float64'):
            libdefor.get_deformation_grid(*args)
    for k in range(2):
        args = grids(n=2)
        args[k] = args[k].astype(dtype)
        with pytest.raises(NotImplementedError, match='only float64'):
            libfilter.normalized_median_test(*args, 0.1)
    x, y, u, v = grids()
    if dtype is not np.complex128:
        with pytest.raises(TypeError, match='bool or uint8'):
            libfilter.normalized_median_test(u, v, 0.1, valid=np.ones((4, 5), dtype=dtype))
        with pytest.raises(TypeError, match='bool or uint8'):
            libdefor.get_deformation_grid(x, y, u, v, valid=np.ones((4, 5), dtype=dtype))


def test_python_tensor_numpy_mix_refused():
    torch = pytest.importorskip('torch')
    x, y, u, v = grids()
    with pytest.raises(TypeError, match='mix'):
        libdefor.get_deformation_grid(torch.from_numpy(x), y, u, v)
    with pytest.raises(TypeError, match='mix'):
        libfilter.normalized_median_test(u, torch.from_numpy(v), 0.1)
    with pytest.raises(TypeError, match='mix'):
        libfilter.normalized_median_test(u, v, 0.1, valid=torch.ones((4, 5), dtype=torch.bool))
    with pytest.raises(TypeError, match='one ROCm device'):                         # host tensors: no CPU fallback
        libfilter.normalized_median_test(torch.from_numpy(u), torch.from_numpy(v), 0.1)


def test_python_empty_and_thin_grids_need_no_device():
    e = np.empty((0, 5))
    keep, res = libfilter.normalized_median_test(e, e, 0.1)
    assert keep.shape == (0, 5) and keep.dtype == bool and res.shape == (0, 5) and res.dtype == np.float64
    for shape, cells in (((1, 6), (0, 5)), ((6, 1), (5, 0)), ((0, 0), (0, 0)), ((1, 1), (0, 0))):
        z = np.zeros(shape)
        out = libdefor.get_deformation_grid(z, z, z, z)
        assert all(o.shape == cells + (2,) and o.dtype == np.float64 for o in out[:5])
        assert out[5].shape == cells + (2, 3) and out[5].dtype == np.int32


# ---------------------------------------------------------------- symbols
def grid_header_functions():
    src = open(os.path.join(ROOT, 'include', 'sid_grid.h')).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    return sorted(set(re.findall(r'\b(sid_grid_[a-z_0-9]+)\s*\(', src)))


def test_grid_symbols_exported():
    assert grid_header_functions() == sorted(_capi.GRID_SYMBOLS)
    assert os.path.exists(_capi.LIB_PATH), 'build with __graft_entry__.build() first'
    lib = ctypes.CDLL(_capi.LIB_PATH)
    for name in _capi.GRID_SYMBOLS:
        assert hasattr(lib, name), name
    assert _capi.ABI_VERSION == 6 and lib.sid_pm_abi_version() == 6
    src = open(os.path.join(ROOT, 'include', 'sid_grid.h')).read()
    assert (int(re.search(r'SID_GRID_TILE_ROWS\s+(\d+)', src).group(1)), int(re.search(r'SID_GRID_TILE_COLS\s+(\d+)', src).group(1))) == _capi.GRID_TILE
    for name, code in _capi.GRID_DIAGONALS.items():
        assert int(re.search(r'SID_GRID_DIAG_%s\s+(\d+)' % name.upper(), src).group(1)) == code


# ---------------------------------------------------------------- end to end: filter, then deformation of what it kept
def test_chain_on_spec_and_host_instance():
    spec = chain_check(lambda u, v, eps, valid: gs.nmt(u, v, valid, eps, 2.0, 1, 3),
                       lambda x, y, u, v, valid: gs.deformation(x, y, u, v, valid, 'shorter'))
    host = chain_check(lambda u, v, eps, valid: tuple(q.astype(bool) if q.dtype == np.uint8 else q for q in host_filter(u, v, valid, eps, 2.0, 1, 3)),
                       lambda x, y, u, v, valid: host_deformation(x, y, u, v, valid, 'shorter'))
    assert np.array_equal(spec[0], host[0]) and np.array_equal(spec[7], host[7])
    for a, b in zip(spec[1:7], host[1:7]):
        assert gs.same_bits(a, b)


@pytest.mark.skipif(not ref_harness.available(), reason='the reference tree is not on this machine')
def test_chain_deformation_is_the_references():
    pytest.importorskip('matplotlib.tri')
    x, y, u, v, usable, planted, eps = mgg.chain_inputs()
    keep, _ = gs.nmt(u, v, usable, eps, 2.0, 1, 3)
    modules, path = dict(sys.modules), list(sys.path)
    try:
        ref = mgg.reference_libdefor()
        exp = gs.deformation(x, y, u, v, keep, 'shorter', on_triangulation=ref.get_deformation_on_triangulation)
    finally:
        for name in [k for k in sys.modules if k not in modules]:
            del sys.modules[name]
        sys.path[:] = path
    assert_deformation(host_deformation(x, y, u, v, keep, 'shorter'), exp, 'chain')
