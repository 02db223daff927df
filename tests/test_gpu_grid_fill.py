"""GPU tests of the gap filling, the smoothing and the chain of include/sid_grid.h: every case of tests/grid_fill_cases.py on
the device bit for bit against the specification (tests/grid_fill_spec.py) - NumPy path and device tensors (non-contiguous
views, poisoned outputs, no copy to the host) - the C ABI into poisoned host buffers, and the chain detect, fill, smooth,
deformation on tensors."""
import ctypes

import numpy as np
import pytest

from sea_ice_drift_amd import _capi, libdefor, libfilter
from tests import grid_fill_cases as gc
from tests import grid_fill_spec as fs
from tests import grid_spec as gs
from tests.golden import make_golden_grid as mgg

pytestmark = pytest.mark.gpu
POISON = -12345.678


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
    return view


def poison_pool(torch):
    """Fill blocks of the caching allocator with a pattern and free them, so that torch.empty hands out poisoned memory."""
    for dtype, val in ((torch.float64, POISON), (torch.int32, 77), (torch.uint8, 7)):
        blocks = [torch.full((1 << 14,), val, dtype=dtype, device='cuda') for _ in range(4)]
        del blocks


# ---------------------------------------------------------------- fill_gaps
@pytest.mark.parametrize('name', list(gc.FILL))
def test_fill_numpy_and_tensors(no_host_copies, name):
    torch = no_host_copies
    u, v, valid, domain, radius, minn, passes = gc.FILL[name]
    exp = gc.fill_expected(name)
    gc.check_properties(name, exp)
    kw = dict(radius=radius, min_neighbours=minn, max_passes=passes)
    got = libfilter.fill_gaps(u, v, valid=valid, domain=domain, **kw)
    assert gc.same_fill(got, exp), name + ' numpy'
    dev = [strided(torch, q) for q in (u, v, valid, domain)]
    poison_pool(torch)
    got = libfilter.fill_gaps(dev[0], dev[1], valid=dev[2], domain=dev[3], **kw)
    assert all(g.is_cuda for g in got) and got[0].dtype == torch.float64 and got[2].dtype == torch.int32
    assert gc.same_fill([_host(g) for g in got], exp), name + ' tensors'


def test_fill_more_passes_than_needed_change_nothing():
    u, v, valid, domain, radius, minn, _ = gc.FILL['tiles_17x65_r1_m3']
    exp = gc.fill_expected('tiles_17x65_r1_m3')
    for passes in (int(exp[2].max()), 256):
        assert gc.same_fill(libfilter.fill_gaps(u, v, valid=valid, radius=radius, min_neighbours=minn, max_passes=passes), exp)


def test_c_abi_writes_every_output_element():
    """The host-buffer entry points into poisoned NumPy outputs (the wrappers' np.empty is not poison)."""
    f64p, u8p, i32p = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_uint8), ctypes.POINTER(ctypes.c_int32)
    u, v, valid, domain, radius, minn, passes = gc.FILL['walled_r1']
    u, v, vv, dd = np.ascontiguousarray(u), np.ascontiguousarray(v), np.ascontiguousarray(valid).view(np.uint8), np.ascontiguousarray(domain)
    uo, vo, gen = np.full(u.shape, POISON), np.full(u.shape, POISON), np.full(u.shape, 77, dtype=np.int32)
    assert _capi.lib().sid_grid_fill(0, u.ctypes.data_as(f64p), v.ctypes.data_as(f64p), vv.ctypes.data_as(u8p), dd.ctypes.data_as(u8p),
                                     u.shape[0], u.shape[1], radius, minn, passes, uo.ctypes.data_as(f64p), vo.ctypes.data_as(f64p),
                                     gen.ctypes.data_as(i32p)) == 0
    assert gc.same_fill((uo, vo, gen), gc.fill_expected('walled_r1'))
    name = 'table_9x33_r2'
    u, v, valid, kw = gc.SMOOTH[name]
    u, v, vv, w = np.ascontiguousarray(u), np.ascontiguousarray(v), np.ascontiguousarray(valid).view(np.uint8), np.ascontiguousarray(kw['weights'])
    uo, vo = np.full(u.shape, POISON), np.full(u.shape, POISON)
    assert _capi.lib().sid_grid_smooth(0, u.ctypes.data_as(f64p), v.ctypes.data_as(f64p), vv.ctypes.data_as(u8p), u.shape[0], u.shape[1],
                                       w.ctypes.data_as(f64p), 2, uo.ctypes.data_as(f64p), vo.ctypes.data_as(f64p)) == 0
    exp = gc.smooth_expected(name)
    assert gs.same_bits(uo, exp[0]) and gs.same_bits(vo, exp[1])


# ---------------------------------------------------------------- smooth
@pytest.mark.parametrize('name', list(gc.SMOOTH))
def test_smooth_numpy_and_tensors(no_host_copies, name):
    torch = no_host_copies
    u, v, valid, kw = gc.SMOOTH[name]
    exp = gc.smooth_expected(name)
    got = libfilter.smooth(u, v, valid=valid, **kw)
    assert gs.same_bits(got[0], exp[0]) and gs.same_bits(got[1], exp[1]), name + ' numpy'
    if name.startswith('isolated'):                                  # its own value: (w * u) / w
        w = kw['weights'][kw['radius'], kw['radius']]
        assert got[0][3, 3] == (w * u[3, 3]) / w and got[1][0, 0] == (w * v[0, 0]) / w
    dev = [strided(torch, q) for q in (u, v, valid)]
    poison_pool(torch)
    got = libfilter.smooth(dev[0], dev[1], valid=dev[2], **kw)
    assert all(g.is_cuda and g.dtype == torch.float64 for g in got)
    got = [_host(g) for g in got]
    assert gs.same_bits(got[0], exp[0]) and gs.same_bits(got[1], exp[1]), name + ' tensors'


# ---------------------------------------------------------------- the chain
def test_chain_numpy():
    x, y, u, v, usable, planted, eps = mgg.chain_inputs()
    keep1 = libfilter.clean_drift(u, v, eps, valid=usable, detect_passes=1)[2]
    assert keep1.dtype == bool and np.array_equal(keep1, usable & ~planted)         # pass 1: exactly the 10 planted nodes
    uc, vc, keep, gen = libfilter.clean_drift(u, v, eps, valid=usable, detect_passes=3)
    assert int(planted.sum()) == 10 and np.array_equal(keep, keep1)                 # passes 2 and 3 remove none
    exp = gc.chain_expected(detect_passes=3)
    assert gc.same_fill((uc, vc, gen), (exp[0], exp[1], exp[3])) and np.array_equal(keep, exp[2])
    assert int((gen == 1).sum()) == 31 and int((gen > 1).sum()) == 0 and int((gen < 0).sum()) == 0   # all 31 gaps in pass 1
    tu, tv = gc.chain_truth()
    filled = gen > 0
    for got, truth in ((uc, tu), (vc, tv)):
        step = gc.step_of(truth, 1)                                                 # from the truth, never from the code under test
        assert (np.abs(got - truth)[filled] <= gen[filled] * step).all()
    domain = np.ones(u.shape, dtype=bool)
    t = libdefor.get_deformation_grid(x, y, uc, vc, valid=gen >= 0)[5]
    inside = domain[:-1, :-1] & domain[:-1, 1:] & domain[1:, :-1] & domain[1:, 1:]  # cells whose nodes all lie in the domain
    assert inside.all() and (t[inside][..., 0] >= 0).all()                          # a triangle in both of their slots
    exp = gc.chain_expected(detect_passes=2, sigma=1.0)
    got = libfilter.clean_drift(u, v, eps, valid=usable, sigma=1.0)
    assert gc.same_fill((got[0], got[1], got[3]), (exp[0], exp[1], exp[3])) and np.array_equal(got[2], exp[2])


def test_chain_with_a_domain():
    """A domain without five columns: their gaps stay, and every slot whose three nodes lie in the domain has a triangle."""
    x, y, u, v, usable, planted, eps = mgg.chain_inputs()
    domain = np.ones(u.shape, dtype=bool)
    domain[:, 4:9] = False
    uc, vc, keep, gen = libfilter.clean_drift(u, v, eps, valid=usable, domain=domain, detect_passes=3)
    exp = fs.clean_drift(u, v, eps, valid=usable, domain=domain, detect_passes=3)
    assert gc.same_fill((uc, vc, gen), (exp[0], exp[1], exp[3])) and np.array_equal(keep, exp[2])
    assert (gen[~domain & ~keep] == -1).all() and (gen[~domain & ~keep] == -1).any() and (gen[domain] >= 0).all()
    t = libdefor.get_deformation_grid(x, y, uc, vc, valid=gen >= 0)[5]
    inside = domain[:-1, :-1] & domain[:-1, 1:] & domain[1:, :-1] & domain[1:, 1:]  # cells whose nodes all lie in the domain
    assert inside.any() and (t[inside][..., 0] >= 0).all() and (t[..., 0] < 0).any()


def test_chain_on_tensors_in_a_stream(no_host_copies):
    """Outputs are on the inputs' device, and a call inside a torch.cuda.stream context is correct after a stream
    synchronise: every step ran on that stream, nothing went to the host in between."""
    torch = no_host_copies
    x, y, u, v, usable, planted, eps = mgg.chain_inputs()
    exp = gc.chain_expected(detect_passes=3, sigma=1.0)
    dev = [strided(torch, q) for q in (u, v, usable)]
    xd, yd = [torch.from_numpy(np.ascontiguousarray(q)).cuda() for q in (x, y)]
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        poison_pool(torch)
        uc, vc, keep, gen = libfilter.clean_drift(dev[0], dev[1], eps, valid=dev[2], detect_passes=3, sigma=1.0)
        t = libdefor.get_deformation_grid(xd, yd, uc, vc, valid=gen >= 0)[5]
    s.synchronize()
    assert all(q.is_cuda and q.device == dev[0].device for q in (uc, vc, keep, gen, t))
    assert keep.dtype == torch.bool and gen.dtype == torch.int32 and uc.dtype == torch.float64
    assert gc.same_fill((_host(uc), _host(vc), _host(gen)), (exp[0], exp[1], exp[3]))
    assert np.array_equal(_host(keep).astype(bool), exp[2]) and (_host(t)[..., 0] >= 0).all()
