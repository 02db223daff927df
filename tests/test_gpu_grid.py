"""GPU tests of include/sid_grid.h: every fixture case on the device bit for bit - NumPy path and device tensors (side stream,
non-contiguous views, poisoned outputs) - random fields against the specification at shapes that straddle the filter's
workgroup tile, and the end-to-end chain on tensors."""
import numpy as np
import pytest

from sea_ice_drift_amd import _capi, libdefor, libfilter
from tests import grid_spec as gs
from tests.golden import make_golden_grid as mgg
from tests.grid_checks import assert_deformation, assert_filter, chain_check

pytestmark = pytest.mark.gpu
TR, TC = _capi.GRID_TILE


@pytest.fixture(scope='module')
def gold():
    return np.load(mgg.PATH)


@pytest.fixture
def no_host_copies(monkeypatch):
    """Any move of a tensor to the host raises while the fixture is active."""
    torch = pytest.importorskip('torch')

    def refuse(*a, **k):
        raise AssertionError('a tensor was copied to the host')
    for name in ('cpu', 'numpy', 'tolist', 'item', '__array__'):
        monkeypatch.setattr(torch.Tensor, name, refuse)
    return torch


def _host(tensor):
    """A device tensor's values through a copy into a host tensor and DLPack (the fixture refuses .cpu() and .numpy())."""
    import torch
    if tensor.dtype == torch.bool:
        tensor = tensor.view(torch.uint8)
    out = torch.empty(tuple(tensor.shape), dtype=tensor.dtype)
    out.copy_(tensor)
    return np.from_dlpack(out).copy()


def strided(torch, a):
    """`a` on the device as a non-contiguous view: every second column of a wider tensor."""
    if a is None:
        return None
    a = np.asarray(a)
    wide = torch.zeros((a.shape[0], 2 * a.shape[1]), dtype=torch.from_numpy(a[:0]).dtype, device='cuda')
    view = wide[:, ::2]
    view.copy_(torch.from_numpy(np.ascontiguousarray(a)))
    assert a.shape[1] < 2 or not view.is_contiguous()
    return view


def poison_pool(torch):
    """Fill blocks of the caching allocator with a pattern and free them, so that torch.empty on the same stream hands out
    poisoned memory for the outputs."""
    for dtype, val in ((torch.float64, -12345.678), (torch.int32, 77), (torch.uint8, 7)):
        blocks = [torch.full((1 << 14,), val, dtype=dtype, device='cuda') for _ in range(4)]
        del blocks


# ---------------------------------------------------------------- fixture parity
@pytest.mark.parametrize('name', mgg.DEFOR_CASES)
def test_fixture_deformation_numpy_and_tensors(gold, no_host_copies, name):
    torch = no_host_copies
    x, y, u, v, valid, diagonal = mgg.defor_inputs(name)
    exp = gs.scatter(gold[name + '_t'], gold[name + '_out']) + (gold[name + '_t'],)
    assert_deformation(libdefor.get_deformation_grid(x, y, u, v, valid=valid, diagonal=diagonal), exp, name + ' numpy')
    dev = [strided(torch, q) for q in (x, y, u, v, valid)]
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        poison_pool(torch)
        got = libdefor.get_deformation_grid(*dev[:4], valid=dev[4], diagonal=diagonal)
    s.synchronize()
    assert all(g.is_cuda for g in got) and got[5].dtype == torch.int32
    assert_deformation([_host(g) for g in got], exp, name + ' tensors')


@pytest.mark.parametrize('name', list(mgg.FILTER_CASES))
def test_fixture_filter_numpy_and_tensors(gold, no_host_copies, name):
    torch = no_host_copies
    u, v, valid, eps, threshold, radius, minn = mgg.filter_inputs(name)
    exp = (gold[name + '_keep'], gold[name + '_res'])
    got = libfilter.normalized_median_test(u, v, eps, valid=valid, threshold=threshold, radius=radius, min_neighbours=minn)
    assert got[0].dtype == bool
    assert_filter((got[0].view(np.uint8), got[1]), exp, name + ' numpy')
    dev = [strided(torch, q) for q in (u, v, valid)]
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        poison_pool(torch)
        keep, res = libfilter.normalized_median_test(dev[0], dev[1], eps, valid=dev[2], threshold=threshold, radius=radius,
                                                     min_neighbours=minn)
    s.synchronize()
    assert keep.is_cuda and keep.dtype == torch.bool and res.dtype == torch.float64
    assert_filter((_host(keep), _host(res)), exp, name + ' tensors')


def test_c_abi_writes_every_output_element():
    """The host-buffer entry points into poisoned NumPy outputs (the wrappers' np.empty is not poison)."""
    import ctypes
    x, y, u, v, valid, diagonal = mgg.defor_inputs('pm_curvi')
    rows, cols = x.shape
    f64p, u8p = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_uint8)
    vv = np.ascontiguousarray(valid).view(np.uint8)
    out = [np.full((rows - 1, cols - 1, 2), -12345.678) for _ in range(5)]
    t = np.full((rows - 1, cols - 1, 2, 3), 77, dtype=np.int32)
    assert _capi.lib().sid_grid_deformation(0, *[q.ctypes.data_as(f64p) for q in (x, y, u, v)], vv.ctypes.data_as(u8p), rows, cols,
                                            0, *[q.ctypes.data_as(f64p) for q in out], t.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))) == 0
    assert_deformation(tuple(out) + (t,), gs.deformation(x, y, u, v, valid, diagonal), 'poisoned')
    keep, res = np.full((rows, cols), 7, dtype=np.uint8), np.full((rows, cols), -12345.678)
    assert _capi.lib().sid_grid_filter(0, u.ctypes.data_as(f64p), v.ctypes.data_as(f64p), vv.ctypes.data_as(u8p), rows, cols,
                                       0.01, 2.0, 1, 3, keep.ctypes.data_as(u8p), res.ctypes.data_as(f64p)) == 0
    assert_filter((keep, res), gs.nmt(u, v, valid, 0.01, 2.0, 1, 3), 'poisoned')


# ---------------------------------------------------------------- random fields at shapes that straddle the tile
SHAPES = [(1, 1), (1, 40), (40, 1), (2, 2)] + [(r, c) for r in (TR - 1, TR, TR + 1) for c in (TC - 1, TC, TC + 1)] + [(35, 70)]
_spec = {}


def random_case(rows, cols):
    """Inputs and the specification's results, computed once per shape."""
    if (rows, cols) not in _spec:
        rng = np.random.default_rng(100 * rows + cols)
        _, _, x, y = mgg.pm_geometry(rows, cols)
        u, v = np.round(rng.standard_normal((rows, cols)), 1), np.round(rng.standard_normal((rows, cols)), 1)    # ties
        valid = rng.random((rows, cols)) >= 0.3
        u[rng.random((rows, cols)) < 0.03] = np.nan
        nmt = {r: gs.nmt(u, v, valid, 0.1, 2.0, r, 3) for r in (1, 2)}
        defor = {d: gs.deformation(x, y, u, v, valid, d) for d in ('shorter', 'main', 'anti')} if rows > 1 and cols > 1 else {}
        _spec[rows, cols] = (x, y, u, v, valid, nmt, defor)
    return _spec[rows, cols]


@pytest.mark.parametrize('rows,cols', SHAPES)
def test_random_fields_against_spec(rows, cols):
    x, y, u, v, valid, nmt, defor = random_case(rows, cols)
    for radius, exp in nmt.items():
        keep, res = libfilter.normalized_median_test(u, v, 0.1, valid=valid, radius=radius)
        assert_filter((keep.view(np.uint8), res), exp, 'radius %d' % radius)
    for diagonal, exp in defor.items():
        assert_deformation(libdefor.get_deformation_grid(x, y, u, v, valid=valid, diagonal=diagonal), exp, diagonal)
    if not defor:
        out = libdefor.get_deformation_grid(x, y, u, v, valid=valid)
        assert out[0].size == 0 and out[5].shape == (rows - 1, cols - 1, 2, 3)


# ---------------------------------------------------------------- end to end on tensors
def test_chain_on_tensors(no_host_copies):
    torch = no_host_copies

    def dev(a):
        return torch.from_numpy(np.ascontiguousarray(a)).cuda()

    state = {}

    def filter_fn(u, v, eps, valid):
        state['keep'], res = libfilter.normalized_median_test(dev(u), dev(v), eps, valid=dev(valid))
        return _host(state['keep']).astype(bool), _host(res)

    def deformation_fn(x, y, u, v, valid):
        # the first call gets the filter's own tensor: nothing returns to the host between the two steps
        mask = state.pop('keep') if 'keep' in state else dev(valid)
        return tuple(_host(o) for o in libdefor.get_deformation_grid(dev(x), dev(y), dev(u), dev(v), valid=mask))

    got = chain_check(filter_fn, deformation_fn)
    x, y, u, v, usable, planted, eps = mgg.chain_inputs()
    keep, res = gs.nmt(u, v, usable, eps, 2.0, 1, 3)
    assert_filter((got[0].view(np.uint8), got[1]), (keep, res), 'chain filter')
    assert_deformation(got[2:], gs.deformation(x, y, u, v, keep, 'shorter'), 'chain deformation')
