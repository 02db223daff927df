"""GPU tests of include/sid_track.h: every case of tests/track_cases.py on the device bit for bit against the specification
(tests/track_spec.py) - NumPy route and device tensors (side stream, strided point views, poisoned outputs, no copy to the
host) - each twice with identical bytes; the bucket route against the host instance with and without the every-cell switch;
the device entry point with guard words behind its outputs; advect and round_trip on tensors; the image warp's maps."""
import numpy as np
import pytest

from sea_ice_drift_amd import _capi, libtrack, libwarp
from tests import track_cases as tc
from tests import track_spec as ts
from tests import warp_cases as wc

pytestmark = pytest.mark.gpu


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
    out = torch.empty(tuple(tensor.shape), dtype=tensor.dtype)
    out.copy_(tensor)
    return np.from_dlpack(out).copy()


def on_device(torch, a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def strided_pair(torch, px, py):
    """px, py as the two columns of one (n, 2) device tensor: views with a stride of two elements."""
    both = torch.from_numpy(np.ascontiguousarray(np.stack([px, py], axis=1))).cuda()
    return both[:, 0], both[:, 1]


def poison_pool(torch):
    """Fill blocks of the caching allocator with a pattern and free them, so that torch.empty on the same stream hands out
    poisoned memory for the outputs."""
    for dtype, val in ((torch.float64, -12345.678), (torch.int32, 113)):
        blocks = [torch.full((1 << 15,), val, dtype=dtype, device='cuda') for _ in range(4)]
        del blocks


def same(a, b):
    return all(ts.same_bits(p, q) for p, q in zip(a, b))


def run_numpy(c, closed, device=0):
    return libtrack.map_points(c['x'], c['y'], c['xs'], c['ys'], c['px'], c['py'], valid=c['valid'], diagonal=c['diagonal'],
                               closed=closed, return_triangle=True, device=device)


# ---------------------------------------------------------------- the cases
@pytest.mark.parametrize('closed', [True, False], ids=['closed', 'open'])
@pytest.mark.parametrize('name', tc.NAMES)
def test_case_numpy_route(name, closed):
    c = tc.BY_NAME[name]
    first = run_numpy(c, closed)
    tc.check(first, name, closed, 'numpy route')
    assert same(first, run_numpy(c, closed)), 'two runs differ'


@pytest.mark.parametrize('closed', [True, False], ids=['closed', 'open'])
@pytest.mark.parametrize('name', tc.NAMES)
def test_case_tensor_route(no_host_copies, name, closed):
    torch = no_host_copies
    c = tc.BY_NAME[name]
    runs = []
    for strided in (True, False):
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            grid = [on_device(torch, c[k]) for k in ('x', 'y', 'xs', 'ys')]
            px, py = strided_pair(torch, c['px'], c['py']) if strided else (on_device(torch, c['px']), on_device(torch, c['py']))
            assert px.is_contiguous() != strided
            poison_pool(torch)
            got = libtrack.map_points(*grid, px, py, valid=on_device(torch, c['valid']), diagonal=c['diagonal'], closed=closed,
                                      return_triangle=True)
        s.synchronize()
        assert all(g.is_cuda for g in got)
        runs.append(tuple(_host(g) for g in got))
        tc.check(runs[-1], name, closed, 'tensor route, strided points' if strided else 'tensor route')
    assert same(*runs), 'two runs differ'


def test_bucket_route_equals_the_host_instance_with_and_without_the_switch(monkeypatch):
    for name in ('bucket_40x40', 'bucket_stretched'):
        c = tc.BY_NAME[name]
        monkeypatch.delenv('SID_TRACK_NO_GRID', raising=False)
        host = run_numpy(c, True, device=-1)
        assert same(host, run_numpy(c, True))
        monkeypatch.setenv('SID_TRACK_NO_GRID', '1')
        assert same(host, run_numpy(c, True))
        assert same(host, run_numpy(c, True, device=-1))
        monkeypatch.delenv('SID_TRACK_NO_GRID')


def test_device_entry_point_writes_n_elements_and_nothing_beyond(no_host_copies):
    """sid_track_points_device into the front of longer buffers: guard words behind the n results stay; with and without tri;
    a second call with a smaller grid and fewer points reuses the scratch."""
    torch = no_host_copies
    guard = 5
    for name, n_used, want_tri in (('bucket_40x40', None, True), ('curvi_frac_main', 777, False), ('two_by_two_anti', 1, True)):
        c, e = tc.BY_NAME[name], tc.expected(name, True)
        n = len(c['px']) if n_used is None else n_used
        grid = [on_device(torch, c[k]) for k in ('x', 'y', 'xs', 'ys')]
        px, py = on_device(torch, c['px']), on_device(torch, c['py'])
        sx = torch.full((n + guard,), -12345.678, dtype=torch.float64, device='cuda')
        sy = torch.full((n + guard,), -12345.678, dtype=torch.float64, device='cuda')
        tri = torch.full((n + guard,), 113, dtype=torch.int32, device='cuda')
        for _ in range(2):
            _capi.track_points_device(*[g.data_ptr() for g in grid], 0, c['x'].shape[0], c['x'].shape[1], _capi.GRID_DIAGONALS[c['diagonal']],
                                      _capi.TRACK_CLOSED, px.data_ptr(), py.data_ptr(), n, sx.data_ptr(), sy.data_ptr(),
                                      tri.data_ptr() if want_tri else 0, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        hx, hy, ht = _host(sx), _host(sy), _host(tri)
        assert ts.same_bits(hx[:n], e['sx'][:n]) and ts.same_bits(hy[:n], e['sy'][:n])
        assert (hx[n:] == -12345.678).all() and (hy[n:] == -12345.678).all() and (ht[n:] == 113).all()
        assert ts.same_bits(ht[:n], e['tri'][:n]) if want_tri else (ht == 113).all()


def test_release_and_run_again():
    c = tc.BY_NAME['curvi_frac_shorter']
    first = run_numpy(c, True)
    _capi.release_workspaces()
    assert same(first, run_numpy(c, True))


# ---------------------------------------------------------------- the Python layer on tensors
def test_advect_and_round_trip_on_tensors(no_host_copies):
    torch = no_host_copies
    fields = tc.three_fields()
    px, py = tc.around(fields[0][0], fields[0][1], 800, 75, margin=6.0)
    px, py = px.reshape(2, -1), py.reshape(2, -1)
    exp = libtrack.advect(px, py, fields, return_path=True, device=-1)
    got = libtrack.advect(on_device(torch, px), on_device(torch, py), [tuple(on_device(torch, a) for a in f) for f in fields],
                          return_path=True)
    assert all(g.is_cuda for g in got) and got[2].dtype == torch.int32
    assert same([_host(g) for g in got], exp)
    x, y, xs, ys = tc.jittered(9, 11, 80)
    xb, yb, _, _ = tc.jittered(12, 13, 81, pitch=8.0)
    xbs, ybs = xb - 2.0 + 0.01 * yb, yb + 1.5 - 0.02 * xb
    valid, valid_b = wc.holes(x.shape, 80, share=0.1), wc.holes(xb.shape, 81, share=0.05)
    xs[3, 3], y[4, 4] = np.nan, np.inf
    exp = libtrack.round_trip(x, y, xs, ys, xb, yb, xbs, ybs, valid=valid, valid_b=valid_b, device=-1)
    dev = [on_device(torch, a) for a in (x, y, xs, ys, xb, yb, xbs, ybs)]
    got = libtrack.round_trip(*dev, valid=on_device(torch, valid), valid_b=on_device(torch, valid_b))
    assert same([_host(g) for g in got], exp) and np.isfinite(exp[0]).sum() > 30
    assert same(libtrack.round_trip(x, y, xs, ys, xb, yb, xbs, ybs, valid=valid, valid_b=valid_b), exp)      # (NumPy route, device 0)


def test_warp_maps_are_the_float32_of_map_points_at_pixel_centres():
    for diag in tc.DIAGONALS:
        w = wc.BY_NAME['curvi_frac_' + diag]
        ro, co = w['out_shape']
        rr, cc = np.meshgrid(np.arange(ro, dtype=np.float64), np.arange(co, dtype=np.float64), indexing='ij')
        sx, sy = libtrack.map_points(w['x'], w['y'], w['xs'], w['ys'], cc, rr, diagonal=diag, closed=False)
        map_x, map_y = libwarp.warp_maps(w['x'], w['y'], w['xs'], w['ys'], (ro, co), diagonal=diag)
        assert np.isfinite(sx).sum() > 5000
        assert ts.same_bits(map_x, sx.astype(np.float32)) and ts.same_bits(map_y, sy.astype(np.float32))
