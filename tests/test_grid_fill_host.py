"""CPU tests of the gap filling, the smoothing and the chain of include/sid_grid.h (libfilter.fill_gaps, smooth, clean_drift):
the host instance of the kernels' source (device = -1) into poisoned outputs against the specification
(tests/grid_fill_spec.py) bit for bit, the reason of every case on the specification's own result, every argument error before
any device call, empty grids, and the Python API's refusals."""
import ctypes

import numpy as np
import pytest

from sea_ice_drift_amd import _capi, libfilter
from tests import grid_fill_cases as gc
from tests import grid_fill_spec as fs
from tests import grid_spec as gs
from tests.golden import make_golden_grid as mgg

POISON = -12345.678
ERR_ARG, ERR_UNSUPPORTED = -1, -4
F64P, U8P, I32P = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_uint8), ctypes.POINTER(ctypes.c_int32)


def u8(mask):
    return None if mask is None else np.ascontiguousarray(mask).view(np.uint8)


def host_fill(u, v, valid, domain, radius, minn, passes):
    """sid_grid_fill(device = -1) into poisoned outputs."""
    u, v, vv, dd = np.ascontiguousarray(u), np.ascontiguousarray(v), u8(valid), u8(domain)
    uo, vo, gen = np.full(u.shape, POISON), np.full(u.shape, POISON), np.full(u.shape, 77, dtype=np.int32)
    rc = _capi.lib().sid_grid_fill(-1, u.ctypes.data_as(F64P), v.ctypes.data_as(F64P),
                                   vv.ctypes.data_as(U8P) if vv is not None else None,
                                   dd.ctypes.data_as(U8P) if dd is not None else None, u.shape[0], u.shape[1],
                                   radius, minn, passes, uo.ctypes.data_as(F64P), vo.ctypes.data_as(F64P), gen.ctypes.data_as(I32P))
    assert rc == 0, _capi.lib().sid_grid_last_error()
    return uo, vo, gen


def host_smooth(u, v, valid, radius=1, sigma=1.0, weights=None):
    u, v, vv = np.ascontiguousarray(u), np.ascontiguousarray(v), u8(valid)
    w = np.ascontiguousarray(fs.gaussian_weights(sigma, radius) if weights is None else weights)
    uo, vo = np.full(u.shape, POISON), np.full(u.shape, POISON)
    rc = _capi.lib().sid_grid_smooth(-1, u.ctypes.data_as(F64P), v.ctypes.data_as(F64P),
                                     vv.ctypes.data_as(U8P) if vv is not None else None, u.shape[0], u.shape[1],
                                     w.ctypes.data_as(F64P), radius, uo.ctypes.data_as(F64P), vo.ctypes.data_as(F64P))
    assert rc == 0, _capi.lib().sid_grid_last_error()
    return uo, vo


# ---------------------------------------------------------------- the host instance against the specification
@pytest.mark.parametrize('name', list(gc.FILL))
def test_fill_host_instance_equals_spec(name):
    exp = gc.fill_expected(name)
    gc.check_properties(name, exp)
    assert gc.same_fill(host_fill(*gc.FILL[name]), exp), name


def test_fill_later_passes_are_no_ops():
    """A pass that fills nothing ends the process: more passes than the holes need change nothing."""
    u, v, valid, domain, radius, minn, _ = gc.FILL['tiles_9x33_r1_m3']
    need = int(gc.fill_expected('tiles_9x33_r1_m3')[2].max())
    assert gc.same_fill(host_fill(u, v, valid, domain, radius, minn, need), gc.fill_expected('tiles_9x33_r1_m3'))
    assert gc.same_fill(host_fill(u, v, valid, domain, radius, minn, 256), gc.fill_expected('tiles_9x33_r1_m3'))
    short = host_fill(u, v, valid, domain, radius, minn, need - 1)
    assert gc.same_fill(short, fs.fill_gaps(u, v, valid, domain, radius, minn, need - 1)) and (short[2] == -1).any()


@pytest.mark.parametrize('name', list(gc.SMOOTH))
def test_smooth_host_instance_equals_spec(name):
    u, v, valid, kw = gc.SMOOTH[name]
    exp = gc.smooth_expected(name)
    got = host_smooth(u, v, valid, **kw)
    assert gs.same_bits(got[0], exp[0]) and gs.same_bits(got[1], exp[1]), name
    ok = gs.usable_uv(u, v, valid)
    assert np.array_equal(np.isnan(exp[0]), ~ok) and np.array_equal(np.isnan(exp[1]), ~ok)
    if name.startswith('isolated'):                                  # its own value: (w * u) / w in the specification's arithmetic
        w = kw['weights'][kw['radius'], kw['radius']]
        for node in ((3, 3), (0, 0)):
            assert got[0][node] == (w * u[node]) / w and got[1][node] == (w * v[node]) / w


def test_gaussian_weights_is_the_specifications():
    for sigma, radius in ((1.0, 1), (0.8, 1), (1.6, 2), (3.0, 2)):
        w = libfilter.gaussian_weights(sigma, radius)
        assert w.shape == (2 * radius + 1, 2 * radius + 1) and gs.same_bits(w, fs.gaussian_weights(sigma, radius))
        assert w[radius, radius] == 1.0
    for bad in (dict(sigma=0.0, radius=1), dict(sigma=np.nan, radius=1), dict(sigma=-1.0, radius=2), dict(sigma=1.0, radius=3)):
        with pytest.raises(ValueError, match='libfilter'):
            libfilter.gaussian_weights(**bad)


# ---------------------------------------------------------------- the chain on the specification and the host instance
def host_clean_drift(u, v, eps, valid, detect_passes, sigma=None):
    """clean_drift composed from the host instances, as libfilter composes the device calls."""
    s = gs.usable_uv(u, v, valid)
    for _ in range(detect_passes):
        res = _capi.grid_filter(np.ascontiguousarray(u), np.ascontiguousarray(v), u8(s), eps, 2.0, 1, 3, device=-1)[1]
        with np.errstate(invalid='ignore'):
            s = s & ~(res > 2.0)
    uc, vc, gen = host_fill(u, v, s, None, 1, 3, 16)
    if sigma is not None:
        uc, vc = host_smooth(uc, vc, gen >= 0, radius=1, sigma=sigma)
    return uc, vc, s, gen


def test_chain_detects_fills_and_stays_within_the_bound():
    x, y, u, v, usable, planted, eps = mgg.chain_inputs()
    uc, vc, keep, gen, sets = gc.chain_expected(detect_passes=3)
    assert np.array_equal(sets[0], usable) and np.array_equal(sets[1], usable & ~planted)       # pass 1: the 10 planted nodes
    assert int(planted.sum()) == 10 and np.array_equal(sets[2], sets[1]) and np.array_equal(sets[3], sets[1])
    assert int((gen == 1).sum()) == 31 and int((gen == 0).sum()) == 149 and gen.max() == 1      # all 31 gaps, in pass 1
    tu, tv = gc.chain_truth()
    for got, truth in ((uc, tu), (vc, tv)):
        step = gc.step_of(truth, 1)
        filled = gen > 0
        assert (np.abs(got - truth)[filled] <= gen[filled] * step).all()
        assert np.array_equal(got[gen == 0].view(np.int64), (u if truth is tu else v)[gen == 0].view(np.int64))
    assert 0.002 < gc.step_of(tu, 1) < 0.003                                                    # the planted error is 0.05
    # feeding the filter's own keep back instead would drop good nodes in the second pass
    k1, _ = gs.nmt(u, v, usable, eps, 2.0, 1, 3)
    k2, _ = gs.nmt(u, v, k1, eps, 2.0, 1, 3)
    assert int((k1 & ~k2).sum()) > 0 and not (k1 & ~k2 & planted).any()
    host = host_clean_drift(u, v, eps, usable, 3)
    assert gc.same_fill((host[0], host[1], host[3]), (uc, vc, gen)) and np.array_equal(host[2], keep)
    exp = gc.chain_expected(detect_passes=2, sigma=1.0)
    host = host_clean_drift(u, v, eps, usable, 2, sigma=1.0)
    assert gc.same_fill((host[0], host[1], host[3]), (exp[0], exp[1], exp[3])) and np.array_equal(host[2], exp[2])
    assert np.abs(exp[0] - tu).max() < 0.003 and np.abs(exp[1] - tv).max() < 0.004              # smoothed: still the field


# ---------------------------------------------------------------- argument errors of the C ABI (before any device call)
def c_fill(null=(), rows=3, cols=4, radius=1, minn=3, passes=16, device=0, alias=None):
    a, b, uo, vo = np.zeros(12), np.zeros(12), np.zeros(12), np.zeros(12)
    gen = np.zeros(12, dtype=np.int32)
    args = dict(u=a, v=b, uo=uo, vo=vo, gen=gen)
    if alias:
        args[alias[0]] = args[alias[1]]
    p = {k: (None if k in null else q.ctypes.data_as(I32P if k == 'gen' else F64P)) for k, q in args.items()}
    return _capi.lib().sid_grid_fill(device, p['u'], p['v'], None, None, rows, cols, radius, minn, passes, p['uo'], p['vo'], p['gen'])


def c_smooth(null=(), rows=3, cols=4, radius=1, weights='ok', device=0, alias=None):
    a, b, uo, vo = np.zeros(12), np.zeros(12), np.zeros(12), np.zeros(12)
    w = np.ones((2 * radius + 1) ** 2 if radius in (1, 2) else 9) if isinstance(weights, str) else np.ascontiguousarray(weights, dtype=np.float64)
    args = dict(u=a, v=b, uo=uo, vo=vo, w=w)
    if alias:
        args[alias[0]] = args[alias[1]]
    p = {k: (None if k in null else q.ctypes.data_as(F64P)) for k, q in args.items()}
    return _capi.lib().sid_grid_smooth(device, p['u'], p['v'], None, rows, cols, p['w'], radius, p['uo'], p['vo'])


def test_c_abi_argument_errors():
    lib = _capi.lib()
    for kw in (dict(null=('u',)), dict(null=('v',)), dict(null=('uo',)), dict(null=('vo',)), dict(null=('gen',)),
               dict(radius=0), dict(radius=3), dict(radius=-1), dict(minn=0), dict(minn=9), dict(radius=2, minn=25), dict(minn=-1),
               dict(passes=0), dict(passes=257), dict(passes=-1), dict(rows=-1), dict(cols=-2),
               dict(alias=('uo', 'u')), dict(alias=('vo', 'v')), dict(alias=('uo', 'v')), dict(alias=('vo', 'u')), dict(alias=('vo', 'uo'))):
        for device in (0, -1):
            assert c_fill(device=device, **kw) == ERR_ARG, kw
            assert lib.sid_grid_last_error()
    assert c_fill(device=-1) == 0 and c_fill(radius=2, minn=24, passes=256, device=-1) == 0 and c_fill(minn=8, passes=1, device=-1) == 0
    bad_centre, negative, nan, inf = np.ones((3, 3)), np.ones((3, 3)), np.ones((3, 3)), np.ones((3, 3))
    bad_centre[1, 1], negative[0, 2], nan[2, 0], inf[1, 0] = 0.0, -1e-300, np.nan, np.inf
    for kw in (dict(null=('u',)), dict(null=('v',)), dict(null=('uo',)), dict(null=('vo',)), dict(null=('w',)),
               dict(radius=0), dict(radius=3), dict(rows=-1), dict(weights=bad_centre), dict(weights=negative), dict(weights=nan),
               dict(weights=inf), dict(alias=('uo', 'u')), dict(alias=('vo', 'v')), dict(alias=('vo', 'uo'))):
        for device in (0, -1):
            assert c_smooth(device=device, **kw) == ERR_ARG, kw
            assert lib.sid_grid_last_error()
    zero_elsewhere = np.zeros((3, 3))
    zero_elsewhere[1, 1] = 1e-300
    assert c_smooth(device=-1) == 0 and c_smooth(weights=zero_elsewhere, device=-1) == 0 and c_smooth(radius=2, device=-1) == 0
    for rows, cols in ((1 << 16, 1 << 15), (1 << 31, 1), (3, 1 << 62), (1 << 40, 1 << 40)):
        assert c_fill(rows=rows, cols=cols) == ERR_UNSUPPORTED and c_smooth(rows=rows, cols=cols) == ERR_UNSUPPORTED
        assert b'2^31' in lib.sid_grid_last_error()
    # the device entry points: the checks come first, no pointer is dereferenced on the device
    vp = ctypes.c_void_p
    p = [vp(1 << 20), vp(2 << 20), vp(3 << 20), vp(4 << 20), vp(5 << 20)]
    w = np.ones(9).ctypes.data_as(F64P)
    assert lib.sid_grid_fill_device(p[0], p[1], None, None, 3, 4, 1, 3, 0, p[2], p[3], p[4], None) == ERR_ARG
    assert lib.sid_grid_fill_device(p[0], p[1], None, None, 3, 4, 3, 3, 16, p[2], p[3], p[4], None) == ERR_ARG
    assert lib.sid_grid_fill_device(p[0], None, None, None, 3, 4, 1, 3, 16, p[2], p[3], p[4], None) == ERR_ARG
    assert lib.sid_grid_fill_device(p[0], p[1], None, None, 3, 4, 1, 3, 16, p[0], p[3], p[4], None) == ERR_ARG      # u_out is u
    assert lib.sid_grid_fill_device(p[0], p[1], None, None, 3, 4, 1, 3, 16, p[2], vp((2 << 20) + 8), p[4], None) == ERR_ARG    # overlaps v
    assert lib.sid_grid_fill_device(p[0], p[1], None, None, 1 << 20, 1 << 20, 1, 3, 16, p[2], p[3], p[4], None) == ERR_UNSUPPORTED
    assert lib.sid_grid_smooth_device(p[0], p[1], None, 3, 4, w, 0, p[2], p[3], None) == ERR_ARG
    assert lib.sid_grid_smooth_device(p[0], p[1], None, 3, 4, None, 1, p[2], p[3], None) == ERR_ARG
    assert lib.sid_grid_smooth_device(p[0], p[1], None, 3, 4, bad_centre.ctypes.data_as(F64P), 1, p[2], p[3], None) == ERR_ARG
    assert lib.sid_grid_smooth_device(p[0], p[1], None, 3, 4, w, 1, p[1], p[3], None) == ERR_ARG                     # u_out is v
    assert lib.sid_grid_smooth_device(p[0], p[1], None, 1 << 31, 4, w, 1, p[2], p[3], None) == ERR_UNSUPPORTED


def test_c_abi_empty_grids_are_valid_calls():
    """Nothing to write; the device entry points return before any device call too."""
    for rows, cols in ((0, 4), (3, 0), (0, 0)):
        for device in (0, -1):
            assert c_fill(rows=rows, cols=cols, device=device) == 0 and c_smooth(rows=rows, cols=cols, device=device) == 0
    lib, one = _capi.lib(), ctypes.c_void_p(16)
    w = np.ones(9).ctypes.data_as(F64P)
    assert lib.sid_grid_fill_device(one, one, None, None, 0, 4, 1, 3, 16, one, one, one, None) == 0
    assert lib.sid_grid_smooth_device(one, one, None, 4, 0, w, 1, one, one, None) == 0
    uo, vo, gen = host_fill(np.ones((1, 1)), np.ones((1, 1)), None, None, 1, 1, 4)
    assert uo[0, 0] == 1.0 and vo[0, 0] == 1.0 and gen[0, 0] == 0


# ---------------------------------------------------------------- the Python API's refusals (before any device call)
def grids(rows=4, cols=5):
    rng = np.random.default_rng(0)
    return rng.standard_normal((rows, cols)), rng.standard_normal((rows, cols))


def test_python_value_errors():
    u, v = grids()
    for kw in (dict(radius=0), dict(radius=3), dict(radius=1.5), dict(min_neighbours=0), dict(min_neighbours=9),
               dict(radius=2, min_neighbours=25), dict(min_neighbours=2.5), dict(max_passes=0), dict(max_passes=257),
               dict(max_passes=1.5), dict(device=-1)):
        with pytest.raises(ValueError, match='libfilter'):
            libfilter.fill_gaps(u, v, **kw)
    for kw in (dict(radius=0), dict(radius=3), dict(sigma=0.0), dict(sigma=np.inf), dict(weights=np.ones((5, 5))),
               dict(radius=2, weights=np.ones((3, 3))), dict(weights=-np.ones((3, 3))), dict(weights=np.full((3, 3), np.nan)),
               dict(weights=np.zeros((3, 3))), dict(device=-1)):
        with pytest.raises(ValueError, match='libfilter'):
            libfilter.smooth(u, v, **kw)
    for kw in (dict(eps=0.0), dict(eps=np.nan), dict(eps=0.1, threshold=0.0), dict(eps=0.1, radius=3), dict(eps=0.1, min_neighbours=0),
               dict(eps=0.1, detect_passes=-1), dict(eps=0.1, detect_passes=1.5), dict(eps=0.1, max_passes=0),
               dict(eps=0.1, sigma=0.0), dict(eps=0.1, device=-1)):
        with pytest.raises(ValueError, match='libfilter'):
            libfilter.clean_drift(u, v, **kw)
    with pytest.raises(TypeError):
        libfilter.clean_drift(u, v)                                                 # eps has no default


def test_python_shapes_dtypes_and_mixes():
    u, v = grids()
    for fn in (libfilter.fill_gaps, libfilter.smooth, lambda *a, **k: libfilter.clean_drift(*a, eps=0.1, **k)):
        for bad in ((u.ravel(), v.ravel()), (u, v.T), (u[None], v[None])):
            with pytest.raises(ValueError, match='2-D'):
                fn(*bad)
        with pytest.raises(ValueError, match='valid'):
            fn(u, v, valid=np.ones((4, 4), dtype=bool))
        with pytest.raises(TypeError, match='bool or uint8'):
            fn(u, v, valid=np.ones((4, 5), dtype=np.int64))
        with pytest.raises(NotImplementedError, match='only float64'):
            fn(u.astype(np.float32), v)
    for fn in (libfilter.fill_gaps, lambda *a, **k: libfilter.clean_drift(*a, eps=0.1, **k)):
        with pytest.raises(ValueError, match='domain'):
            fn(u, v, domain=np.ones((5, 4), dtype=bool))
        with pytest.raises(TypeError, match='domain'):
            fn(u, v, domain=np.ones((4, 5)))
    torch = pytest.importorskip('torch')
    with pytest.raises(TypeError, match='mix'):
        libfilter.fill_gaps(u, torch.from_numpy(v))
    with pytest.raises(TypeError, match='mix'):
        libfilter.fill_gaps(u, v, domain=torch.ones((4, 5), dtype=torch.bool))
    with pytest.raises(TypeError, match='mix'):
        libfilter.smooth(u, v, valid=torch.ones((4, 5), dtype=torch.bool))
    with pytest.raises(TypeError, match='host table'):
        libfilter.smooth(u, v, weights=torch.ones((3, 3), dtype=torch.float64))
    with pytest.raises(TypeError, match='one ROCm device'):                         # host tensors: no CPU fallback
        libfilter.fill_gaps(torch.from_numpy(u), torch.from_numpy(v))
    with pytest.raises(TypeError, match='one ROCm device'):
        libfilter.clean_drift(torch.from_numpy(u), torch.from_numpy(v), 0.1)


def test_python_empty_grids_need_no_device():
    e = np.empty((0, 5))
    uf, vf, gen = libfilter.fill_gaps(e, e)
    assert uf.shape == vf.shape == gen.shape == (0, 5) and uf.dtype == np.float64 and gen.dtype == np.int32
    us, vs = libfilter.smooth(e, e)
    assert us.shape == vs.shape == (0, 5) and us.dtype == np.float64
    uc, vc, keep, gen = libfilter.clean_drift(e, e, 0.1, sigma=1.0)
    assert uc.shape == (0, 5) and keep.dtype == bool and keep.shape == (0, 5) and gen.dtype == np.int32
