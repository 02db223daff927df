"""GPU tests of sea_ice_drift_amd.libdefor (include/sid_defor.h): the reference's fixture bit for bit, the device-tensor path,
random triangulations against a NumPy restatement of the reference's formulas, and the kernel's float64 hypot against
np.hypot."""
import os
import warnings

import numpy as np
import pytest

from sea_ice_drift_amd import _capi, libdefor
from tests.golden import make_golden_defor as mg

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'g10_deformation.npz')
KEYS = ('e1', 'e2', 'e3', 'a', 'p')


def gold():
    return np.load(GOLD)


# NumPy restatement of libdefor.py (the reference itself is not on the GPU box): the same operations in the same order
def np_elems(xt, yt, ut, vt, a):
    ux = uy = vx = vy = 0
    for i0, i1 in zip([1, 2, 0], [0, 1, 2]):
        ux = ux + (ut[i0] + ut[i1]) * (yt[i0] - yt[i1])
        uy = uy - (ut[i0] + ut[i1]) * (xt[i0] - xt[i1])
        vx = vx + (vt[i0] + vt[i1]) * (yt[i0] - yt[i1])
        vy = vy - (vt[i0] + vt[i1]) * (xt[i0] - xt[i1])
    ux, uy, vx, vy = [i / (2 * a) for i in (ux, uy, vx, vy)]
    return ux + vy, ((ux - vy) ** 2 + (uy + vx) ** 2) ** 0.5, vx - uy


def np_triangulation(x, y, u, v, t):
    xt, yt, ut, vt = [i[t].T for i in (x, y, u, v)]
    sx = [xt[1] - xt[0], xt[2] - xt[1], xt[0] - xt[2]]
    sy = [yt[1] - yt[0], yt[2] - yt[1], yt[0] - yt[2]]
    s = [np.hypot(sx[k], sy[k]) for k in range(3)]
    p = (s[0] + s[1]) + s[2]
    h = p / 2
    a = np.sqrt(h * (h - s[0]) * (h - s[1]) * (h - s[2]))
    return np_elems(xt, yt, ut, vt, a) + (a, p)


def assert_same(got, exp, what):
    for key, g, e in zip(KEYS, got, exp):
        assert mg.same_bits(np.asarray(g), np.asarray(e)), '%s: %s differs' % (what, key)


# ---------------------------------------------------------------- fixture parity (the reference's own outputs)
@pytest.mark.parametrize('name', mg.TRI_CASES)
def test_fixture_on_triangulation(name):
    g = gold()
    args = mg.tri_inputs(name)
    assert mg.sha256(*args) == str(g[name + '_in_sha'])
    got = libdefor.get_deformation_on_triangulation(*args)
    assert_same(got, [g['%s_%s' % (name, k)] for k in KEYS], name)


def test_fixture_elems():
    g = gold()
    args = mg.elems_inputs()
    assert mg.sha256(*args) == str(g['elems_in_sha'])
    got = libdefor.get_deformation_elems(*args)
    assert_same(got, [g['elems_' + k] for k in ('e1', 'e2', 'e3')], 'elems')


@pytest.mark.parametrize('name', mg.NODE_CASES)
def test_fixture_nodes_on_reference_triangles(name):
    """The reference's triangles (stored) with the nodes: the element pass alone, whatever matplotlib the box has."""
    g = gold()
    x, y, u, v = mg.node_inputs(name)
    assert mg.sha256(x, y, u, v) == str(g[name + '_in_sha'])
    got = libdefor.get_deformation_on_triangulation(x, y, u, v, g[name + '_t'])
    assert_same(got, [g['%s_%s' % (name, k)] for k in KEYS], name)


@pytest.mark.parametrize('name', mg.NODE_CASES)
def test_fixture_get_deformation_nodes(name):
    pytest.importorskip('matplotlib.tri')
    g = gold()
    x, y, u, v = mg.node_inputs(name)
    out = libdefor.get_deformation_nodes(x, y, u, v)
    t = out[5]
    assert t.dtype == np.int32
    if t.shape == g[name + '_t'].shape and np.array_equal(t, g[name + '_t']):
        assert_same(out[:5], [g['%s_%s' % (name, k)] for k in KEYS], name)
    else:                                       # another matplotlib / Qhull: compare against this box's own triangulation
        warnings.warn('%s: this matplotlib triangulates the fixture differently from the one that wrote it; '
                      'compared against its own triangles' % name)
        with np.errstate(all='ignore'):
            assert_same(out[:5], np_triangulation(x, y, u, v, t), name)


# ---------------------------------------------------------------- errors
def test_out_of_range_index_flag_host_buffers():
    """The C ABI's own check (the device-side flag), below the Python one."""
    x, y, u, v = mg.tri_nodes()
    for dtype in (np.int32, np.int64):
        for bad in (60, -61, 1 << 30):
            t = np.array([[0, 1, 2]] * 300 + [[3, bad, 4]] + [[5, 6, 7]] * 10, dtype=dtype)
            with pytest.raises(IndexError, match='outside'):
                _capi.defor_triangulation(x, y, u, v, t)
        ok = _capi.defor_triangulation(x, y, u, v, np.array([[0, -1, -60]], dtype=dtype))     # the next call is clean
        assert np.isfinite(ok[3]).all()


def test_reference_error_types():
    g = gold()
    for name, exp in zip(g['err_names'], g['err_types']):
        if name != 'index_out_of_range':
            pytest.importorskip('matplotlib.tri')
        with pytest.raises(Exception) as info:
            mg.error_call(libdefor, str(name))
        assert type(info.value).__name__ == exp


# ---------------------------------------------------------------- random triangulations up to N = 40 000
@pytest.mark.parametrize('n,m,dtype,seed', [(3, 1, np.int32, 1), (17, 1000, np.int64, 2), (1000, 2000, np.int32, 3),
                                            (40000, 80000, np.int32, 4), (40000, 79202, np.int64, 5), (257, 100003, np.int32, 6)])
def test_random_against_numpy_restatement(n, m, dtype, seed):
    rng = np.random.default_rng(seed)
    x, y = rng.uniform(1e5, 1e6, n), rng.uniform(-1e6, -1e5, n)
    u, v = 0.1 * rng.standard_normal(n), 0.1 * rng.standard_normal(n)
    t = rng.integers(-n, n, (m, 3)).astype(dtype)
    t[::97, 1] = t[::97, 0]                                     # repeated vertices
    with np.errstate(all='ignore'):
        exp = np_triangulation(x, y, u, v, t)
    assert_same(libdefor.get_deformation_on_triangulation(x, y, u, v, t), exp, 'n=%d m=%d' % (n, m))
    xt, yt, ut, vt = [i[t].T for i in (x, y, u, v)]
    with np.errstate(all='ignore'):
        exp3 = np_elems(xt, yt, ut, vt, exp[3])
    assert_same(libdefor.get_deformation_elems(xt, yt, ut, vt, exp[3]), exp3, 'elems n=%d m=%d' % (n, m))


# ---------------------------------------------------------------- device tensors
@pytest.fixture
def no_host_copies(monkeypatch):
    """Any move of a tensor to the host raises while the fixture is active."""
    torch = pytest.importorskip('torch')

    def refuse(*a, **k):
        raise AssertionError('a tensor was copied to the host')
    for name in ('cpu', 'numpy', 'tolist', 'item', '__array__'):
        monkeypatch.setattr(torch.Tensor, name, refuse)
    return torch


def test_device_tensors_match_numpy_path(no_host_copies):
    torch = no_host_copies
    rng = np.random.default_rng(11)
    n, m = 40000, 79202
    x, y = rng.uniform(1e5, 1e6, n), rng.uniform(-1e6, -1e5, n)
    u, v = 0.1 * rng.standard_normal(n), 0.1 * rng.standard_normal(n)
    for dtype in (np.int32, np.int64):
        t = rng.integers(-n, n, (m, 3)).astype(dtype)
        exp = libdefor.get_deformation_on_triangulation(x, y, u, v, t)
        dev = [torch.tensor(q, device='cuda') for q in (x, y, u, v, t)]
        got = libdefor.get_deformation_on_triangulation(*dev)
        assert all(g.is_cuda and g.dtype == torch.float64 and tuple(g.shape) == (m,) for g in got)
        assert_same([_host(g) for g in got], exp, 'tensors %s' % np.dtype(dtype).name)


def _host(tensor):
    """A device tensor's values through a copy into a host tensor and DLPack (the fixture refuses .cpu() and .numpy())."""
    import torch
    out = torch.empty(tuple(tensor.shape), dtype=tensor.dtype)
    out.copy_(tensor)
    return np.from_dlpack(out).copy()


def test_device_tensors_on_a_side_stream_and_elems(no_host_copies):
    torch = no_host_copies
    rng = np.random.default_rng(12)
    n, m = 5000, 9000
    x, y = rng.uniform(1e5, 1e6, n), rng.uniform(-1e6, -1e5, n)
    u, v = 0.1 * rng.standard_normal(n), 0.1 * rng.standard_normal(n)
    t = rng.integers(0, n, (m, 3)).astype(np.int32)
    with np.errstate(all='ignore'):
        exp = np_triangulation(x, y, u, v, t)
    dev = [torch.tensor(q, device='cuda') for q in (x, y, u, v, t)]
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        got = libdefor.get_deformation_on_triangulation(*dev)
        xt, yt, ut, vt = [q[dev[4].long()].T for q in dev[:4]]
        e = libdefor.get_deformation_elems(xt, yt, ut, vt, got[3])
    s.synchronize()
    assert_same([_host(g) for g in got], exp, 'side stream')
    with np.errstate(all='ignore'):
        exp3 = np_elems(*[i[t].T for i in (x, y, u, v)], exp[3])
    assert_same([_host(g) for g in e], exp3, 'elems tensors')


def test_device_tensor_out_of_range_index(no_host_copies):
    torch = no_host_copies
    x, y, u, v = [torch.tensor(q, device='cuda') for q in mg.tri_nodes()]
    for bad in (60, -61):
        t = torch.tensor([[0, 1, 2], [3, bad, 4]], dtype=torch.int32, device='cuda')
        with pytest.raises(IndexError):
            libdefor.get_deformation_on_triangulation(x, y, u, v, t)
    ok = libdefor.get_deformation_on_triangulation(x, y, u, v, torch.tensor([[0, 1, -1]], dtype=torch.int64, device='cuda'))
    assert tuple(ok[0].shape) == (1,)


# ---------------------------------------------------------------- float64 hypot on the device
def test_device_hypot_matches_numpy_bit_for_bit():
    x, y = mg.hypot_pairs(1 << 24, seed=2024)
    got = _capi.defor_debug_hypot(x, y, device=0)
    with np.errstate(all='ignore'):
        exp = np.hypot(x, y)
    bad = ~((got.view(np.int64) == exp.view(np.int64)) | (np.isnan(got) & np.isnan(exp)))
    assert int(bad.sum()) == 0, 'first mismatch: hypot(%r, %r) = %r, numpy %r' % (
        x[bad][0], y[bad][0], got[bad][0], exp[bad][0])
