"""CPU tests of sea_ice_drift_amd.libdefor: the argument checks that happen before any device work, the fixture against the
reference (when its tree is present), the exported symbols and the host instance of the kernel's float64 hypot."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from oracle import ref_harness
from sea_ice_drift_amd import _capi, libdefor
from tests.golden import make_golden_defor as mg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def nodes(n=10, seed=0):
    rng = np.random.default_rng(seed)
    return [rng.uniform(0, 1e5, n), rng.uniform(0, 1e5, n), rng.standard_normal(n) * 0.1, rng.standard_normal(n) * 0.1]


def corners(m=4, seed=0):
    rng = np.random.default_rng(seed)
    return [rng.uniform(0, 1e5, (3, m)) for _ in range(4)] + [rng.uniform(1e6, 1e7, m)]


# ---------------------------------------------------------------- dtypes
@pytest.mark.parametrize('k', range(4))
@pytest.mark.parametrize('dtype', [np.float32, np.int64, np.complex128])
def test_non_float64_nodes_refused(k, dtype):
    args = nodes()
    args[k] = args[k].astype(dtype)
    t = np.array([[0, 1, 2]], dtype=np.int32)
    with pytest.raises(NotImplementedError, match='float64'):
        libdefor.get_deformation_on_triangulation(*args, t)
    with pytest.raises(NotImplementedError, match='float64'):
        libdefor.get_deformation_nodes(*args)


@pytest.mark.parametrize('k', range(5))
def test_non_float64_elems_refused(k):
    args = corners()
    args[k] = args[k].astype(np.float32)
    with pytest.raises(NotImplementedError, match='float64'):
        libdefor.get_deformation_elems(*args)


@pytest.mark.parametrize('dtype', [np.float64, np.uint32, np.int16, np.bool_])
def test_triangle_dtype_refused(dtype):
    with pytest.raises(NotImplementedError, match='int32 or int64'):
        libdefor.get_deformation_on_triangulation(*nodes(), np.zeros((2, 3), dtype=dtype))


# ---------------------------------------------------------------- shapes
def test_node_shapes():
    x, y, u, v = nodes()
    t = np.array([[0, 1, 2]], dtype=np.int32)
    for bad in ((x[:, None], y, u, v), (x, y[:-1], u, v), (x, y, u, v[:5]), (x.reshape(2, 5), y.reshape(2, 5), u.reshape(2, 5), v.reshape(2, 5))):
        with pytest.raises(ValueError, match='1-D'):
            libdefor.get_deformation_on_triangulation(*bad, t)


@pytest.mark.parametrize('shape', [(3,), (6,), (1, 3, 1), (2, 4), (3, 2), (0,)])
def test_triangle_shape(shape):
    with pytest.raises(ValueError, match=r'\(M, 3\)'):
        libdefor.get_deformation_on_triangulation(*nodes(), np.zeros(shape, dtype=np.int32))


def test_elems_shapes():
    x, y, u, v, a = corners(m=4)
    with pytest.raises(ValueError, match=r'\(M,\)'):
        libdefor.get_deformation_elems(x, y, u, v, a[:, None])            # NumPy would broadcast the result to (M, M)
    with pytest.raises(ValueError, match=r'\(M,\)'):
        libdefor.get_deformation_elems(x, y, u, v, a[:3])
    with pytest.raises(ValueError, match=r'\(3, M\)'):
        libdefor.get_deformation_elems(x.T, y.T, u.T, v.T, a)
    with pytest.raises(ValueError, match=r'\(3, M\)'):
        libdefor.get_deformation_elems(x, y[:, :3], u, v, a)


def test_mixed_tensor_and_array_refused():
    torch = pytest.importorskip('torch')
    x, y, u, v = nodes()
    with pytest.raises(TypeError, match='mix'):
        libdefor.get_deformation_on_triangulation(torch.from_numpy(x), y, u, v, np.array([[0, 1, 2]], dtype=np.int32))


# ---------------------------------------------------------------- indices
@pytest.mark.parametrize('dtype', [np.int32, np.int64])
@pytest.mark.parametrize('bad', [10, 11, -11, 2 ** 31 - 1, -2 ** 31])
def test_out_of_range_index_raises_index_error(dtype, bad):
    x, y, u, v = nodes(10)
    t = np.array([[0, 1, 2], [3, bad, 4]], dtype=dtype)
    with pytest.raises(IndexError, match='out of bounds for axis 0 with size 10'):
        libdefor.get_deformation_on_triangulation(x, y, u, v, t)
    with pytest.raises(IndexError):                                        # what NumPy, and so the reference, raises
        x[t]


def test_any_index_into_no_nodes_raises():
    e = np.empty(0)
    with pytest.raises(IndexError):
        libdefor.get_deformation_on_triangulation(e, e, e, e, np.zeros((1, 3), dtype=np.int32))


# ---------------------------------------------------------------- M = 0: no device work
@pytest.mark.parametrize('dtype', [np.int32, np.int64])
def test_no_triangles(dtype):
    out = libdefor.get_deformation_on_triangulation(*nodes(), np.zeros((0, 3), dtype=dtype))
    assert len(out) == 5
    for o in out:
        assert isinstance(o, np.ndarray) and o.shape == (0,) and o.dtype == np.float64
    e = np.empty(0)
    assert all(o.shape == (0,) for o in libdefor.get_deformation_on_triangulation(e, e, e, e, np.zeros((0, 3), dtype=dtype)))


def test_no_elements():
    z = np.zeros((3, 0))
    out = libdefor.get_deformation_elems(z, z, z, z, np.zeros(0))
    assert len(out) == 3 and all(o.shape == (0,) and o.dtype == np.float64 for o in out)


def test_fixture_m0_cases_match():
    g = np.load(os.path.join(ROOT, 'tests', 'golden', 'g10_deformation.npz'))
    for name in ('tri_empty_i32', 'tri_empty_i64'):
        got = libdefor.get_deformation_on_triangulation(*mg.tri_inputs(name))
        for key, o in zip(('e1', 'e2', 'e3', 'a', 'p'), got):
            assert mg.same_bits(o, g['%s_%s' % (name, key)])


def test_package_and_two_functions_do_not_need_matplotlib():
    code = ('import sys; sys.modules["matplotlib"] = None; sys.modules["matplotlib.tri"] = None\n'
            'import numpy as np\n'
            'from sea_ice_drift_amd import libdefor\n'
            'z = np.zeros((3, 0)); e = np.zeros(0)\n'
            'assert len(libdefor.get_deformation_elems(z, z, z, z, e)) == 3\n'
            'assert len(libdefor.get_deformation_on_triangulation(e, e, e, e, np.zeros((0, 3), dtype=np.int32))) == 5\n'
            'try:\n'
            '    libdefor.get_deformation_nodes(e, e, e, e)\n'
            '    raise SystemExit("get_deformation_nodes ran without matplotlib")\n'
            'except ImportError:\n'
            '    pass\n')
    subprocess.check_call([sys.executable, '-c', code], cwd=ROOT)


# ---------------------------------------------------------------- errors where the reference raises
def test_reference_errors_recorded():
    g = np.load(os.path.join(ROOT, 'tests', 'golden', 'g10_deformation.npz'))
    assert list(g['err_names']) == list(mg.ERROR_CASES)
    assert list(g['err_types']) == ['IndexError', 'ValueError', 'RuntimeError']


@pytest.mark.parametrize('name', mg.ERROR_CASES)
def test_same_error_as_reference(name):
    """Each raises before any device work: the index check on the host, matplotlib's own checks in Triangulation."""
    if name != 'index_out_of_range':
        pytest.importorskip('matplotlib.tri')
    g = np.load(os.path.join(ROOT, 'tests', 'golden', 'g10_deformation.npz'))
    exp = dict(zip(g['err_names'], g['err_types']))[name]
    with pytest.raises(Exception) as info:
        mg.error_call(libdefor, name)
    assert type(info.value).__name__ == exp


# ---------------------------------------------------------------- fixture
def test_fixture_inputs_regenerate():
    g = np.load(os.path.join(ROOT, 'tests', 'golden', 'g10_deformation.npz'))
    for name in mg.NODE_CASES:
        assert mg.sha256(*mg.node_inputs(name)) == str(g[name + '_in_sha'])
    for name in mg.TRI_CASES:
        assert mg.sha256(*mg.tri_inputs(name)) == str(g[name + '_in_sha'])
    assert mg.sha256(*mg.elems_inputs()) == str(g['elems_in_sha'])


def test_fixture_is_small():
    assert os.path.getsize(os.path.join(ROOT, 'tests', 'golden', 'g10_deformation.npz')) < 256 * 1024


@pytest.mark.skipif(not ref_harness.available(), reason='the reference tree is not on this machine')
def test_fixture_regenerates_from_reference():
    pytest.importorskip('matplotlib.tri')
    g = np.load(os.path.join(ROOT, 'tests', 'golden', 'g10_deformation.npz'))
    modules, path = dict(sys.modules), list(sys.path)
    try:
        fresh = mg.compute(mg.reference_libdefor())
    finally:                                    # the harness's stub modules (nansat, cv2, osgeo) must not reach later tests
        for name in [k for k in sys.modules if k not in modules]:
            del sys.modules[name]
        sys.path[:] = path
    assert sorted(fresh) == sorted(g.files)
    for key, val in fresh.items():
        if val.dtype.kind == 'f':
            assert mg.same_bits(val, g[key]), key
        else:
            assert val.dtype == g[key].dtype and np.array_equal(val, g[key]), key


# ---------------------------------------------------------------- symbols and the host hypot
def defor_header_functions():
    src = open(os.path.join(ROOT, 'include', 'sid_defor.h')).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    return sorted(set(re.findall(r'\b(sid_defor_[a-z_0-9]+)\s*\(', src)))


def test_defor_symbols_exported():
    assert defor_header_functions() == sorted(_capi.DEFOR_SYMBOLS)
    assert os.path.exists(_capi.LIB_PATH), 'build with __graft_entry__.build() first'
    lib = ctypes.CDLL(_capi.LIB_PATH)
    for name in _capi.DEFOR_SYMBOLS:
        assert hasattr(lib, name), name


def test_host_hypot_matches_libm_bit_for_bit():
    """The one source of the kernel's hypot, compiled for the host, against np.hypot (glibc) on 2^20 pairs that cover NaN,
    inf, subnormals, wide ratios and both scaling thresholds.  (tools/defor_hypot_check.py runs 10^8 of them.)"""
    x, y = mg.hypot_pairs(1 << 20, seed=12345)
    got = _capi.defor_debug_hypot(x, y, device=-1)
    with np.errstate(all='ignore'):
        exp = np.hypot(x, y)
    assert np.isnan(exp).sum() > 1000 and np.isinf(exp).sum() > 1000 and (exp < 2.2250738585072014e-308).sum() > 1000
    assert mg.same_bits(got, exp)
