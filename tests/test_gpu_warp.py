"""GPU tests of include/sid_warp.h: every case of tests/warp_cases.py on the device bit for bit against the specification
(tests/warp_spec.py) - NumPy route and device tensors (side stream, strided views, poisoned outputs, no copy to the host) -
each twice with identical bytes, the device entry point with a padded output, and the end-to-end check on the smoke pair."""
import numpy as np
import pytest

from sea_ice_drift_amd import _capi, libwarp, pmlib, synthetic
from tests import warp_cases as wc
from tests import warp_spec as ws

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
    if tensor is None:
        return None
    out = torch.empty(tuple(tensor.shape), dtype=tensor.dtype)
    out.copy_(tensor)
    return np.from_dlpack(out).copy()


def on_device(torch, a, strided=False):
    """`a` on the device; `strided`: as a view with padded rows (2-D) that is not contiguous."""
    if a is None:
        return None
    a = np.ascontiguousarray(a)
    if not strided or a.ndim != 2 or a.shape[1] < 1:
        return torch.from_numpy(a).cuda()
    wide = torch.zeros((a.shape[0], a.shape[1] + 7), dtype=torch.from_numpy(a[:0]).dtype, device='cuda')
    view = wide[:, 3:3 + a.shape[1]]
    view.copy_(torch.from_numpy(a))
    return view


def poison_pool(torch):
    """Fill blocks of the caching allocator with a pattern and free them, so that torch.empty on the same stream hands out
    poisoned memory for the outputs."""
    for dtype, val in ((torch.float32, -12345.678), (torch.uint8, 113)):
        blocks = [torch.full((1 << 16,), val, dtype=dtype, device='cuda') for _ in range(4)]
        del blocks


def through_libwarp(c, conv, host, **kw):
    """A case through the public functions.  conv: array -> what is passed; host: result -> NumPy.  The one combination they
    do not offer (covered without an image) goes through the bindings."""
    x, y, xs, ys, valid, image = [conv(c[k]) for k in ('x', 'y', 'xs', 'ys', 'valid', 'image')]
    out = covered = map_x = map_y = None
    if 'out' in c['want']:
        out, covered = libwarp.warp_image(image, x, y, xs, ys, out_shape=c['out_shape'], valid=valid, order=c['order'],
                                          fill=c['fill'], diagonal=c['diagonal'], keep_zero=c['keep_zero'], return_covered=True, **kw)
        if 'covered' not in c['want']:
            covered = None
    elif 'covered' in c['want']:
        _, covered, _, _ = covered_alone(c, conv)
    if 'maps' in c['want']:
        map_x, map_y = libwarp.warp_maps(x, y, xs, ys, c['out_shape'], valid=valid, diagonal=c['diagonal'], **kw)
    return tuple(host(q) if q is not None else None for q in (out, covered, map_x, map_y))


def covered_alone(c, conv):
    """covered without an image: what is in range is the source shape's say alone."""
    x, y, xs, ys, valid = [conv(c[k]) for k in ('x', 'y', 'xs', 'ys', 'valid')]
    code = _capi.GRID_DIAGONALS[c['diagonal']]
    if isinstance(x, np.ndarray):
        return _capi.warp_image(x, y, xs, ys, valid, None, 'uint8', c['src_shape'], c['out_shape'], c['order'], c['fill'], code, 0,
                                False, True, False, device=0)
    import torch
    x, y, xs, ys = [q.contiguous() for q in (x, y, xs, ys)]
    covered = torch.empty(c['out_shape'], dtype=torch.uint8, device='cuda')
    _capi.warp_image_device(x.data_ptr(), y.data_ptr(), xs.data_ptr(), ys.data_ptr(), valid.contiguous().data_ptr() if valid is not None else 0,
                            x.shape[0], x.shape[1], 0, 'uint8', c['src_shape'], 0, c['out_shape'], c['order'], c['fill'], code, 0,
                            0, 0, covered.data_ptr(), 0, 0, torch.cuda.current_stream().cuda_stream)
    return None, covered, None, None


def same(a, b):
    return all((p is None and q is None) or ws.same_bits(p, q) for p, q in zip(a, b))


# ---------------------------------------------------------------- the cases
@pytest.mark.parametrize('name', wc.NAMES)
def test_case_numpy_route(name):
    c = wc.BY_NAME[name]
    first = through_libwarp(c, lambda a: a, lambda a: a)
    wc.check(first, name, 'numpy route')
    assert same(first, through_libwarp(c, lambda a: a, lambda a: a)), 'two runs differ'


@pytest.mark.parametrize('name', wc.NAMES)
def test_case_tensor_route(no_host_copies, name):
    torch = no_host_copies
    c = wc.BY_NAME[name]
    runs = []
    for strided in (True, False):
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            poison_pool(torch)
            got = through_libwarp(c, lambda a: on_device(torch, a, strided), lambda t: t)
        s.synchronize()
        assert all(g is None or g.is_cuda for g in got)
        runs.append(tuple(_host(g) for g in got))
        wc.check(runs[-1], name, 'tensor route, strided inputs' if strided else 'tensor route')
    assert same(*runs), 'two runs differ'


def test_device_entry_point_with_padded_output(no_host_copies):
    """sid_warp_image_device writes into rows longer than the image and leaves the padding alone; all four outputs at once."""
    torch = no_host_copies
    name = 'curvi_frac_main'
    c = wc.BY_NAME[name]
    ro, co = c['out_shape']
    x, y, xs, ys, img = [on_device(torch, c[k]) for k in ('x', 'y', 'xs', 'ys', 'image')]
    wide = torch.full((ro, co + 9), 113, dtype=torch.uint8, device='cuda')
    covered = torch.full((ro, co), 7, dtype=torch.uint8, device='cuda')
    map_x, map_y = [torch.full((ro, co), -1.0, dtype=torch.float32, device='cuda') for _ in range(2)]
    for _ in range(2):
        _capi.warp_image_device(x.data_ptr(), y.data_ptr(), xs.data_ptr(), ys.data_ptr(), 0, x.shape[0], x.shape[1], img.data_ptr(),
                                'uint8', c['src_shape'], img.stride(0), (ro, co), c['order'], c['fill'],
                                _capi.GRID_DIAGONALS[c['diagonal']], 1 if c['keep_zero'] else 0, wide[:, 2:].data_ptr(), co + 9,
                                covered.data_ptr(), map_x.data_ptr(), map_y.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    w = _host(wide)
    wc.check((w[:, 2:2 + co], _host(covered), _host(map_x), _host(map_y)), name, 'device entry point')
    assert (w[:, :2] == 113).all() and (w[:, 2 + co:] == 113).all()


def test_release_and_run_again():
    c = wc.BY_NAME['regular_u8_o1']
    first = through_libwarp(c, lambda a: a, lambda a: a)
    _capi.release_workspaces()
    assert same(first, through_libwarp(c, lambda a: a, lambda a: a))


# ---------------------------------------------------------------- end to end
def corr(a, b, mask):
    return float(np.corrcoef(a[mask].astype(np.float64), b[mask].astype(np.float64))[0, 1])


def test_pattern_matching_then_warp_lines_the_pair_up():
    """The smoke pair and grid: sub-pixel pattern matching, then image 2 warped onto image 1 with the matched positions.  On the
    covered pixels its correlation with image 1 reaches at least the midpoint between the unwarped correlation and the one the
    specification gets with the true field on the same nodes."""
    img1, img2 = synthetic.make_pair(400, 400, seed=17)
    g = synthetic.make_grid(400, 400, 6, margin=90)
    res = pmlib.pm_dispatch(img1, img2, g['c1'], g['r1'], g['c2fg'], g['r2fg'], g['border'], 34, 0.0, subpixel=True)
    x, y = g['c1'].reshape(6, 6), g['r1'].reshape(6, 6)
    xs, ys = np.ascontiguousarray(res[:, 0]).reshape(6, 6), np.ascontiguousarray(res[:, 1]).reshape(6, 6)
    assert np.isfinite(xs).all() and np.isfinite(ys).all()
    out, covered = libwarp.warp_image(img2, x, y, xs, ys, return_covered=True)
    mask = covered > 0
    dc, dr = synthetic.true_displacement(x, y)
    ideal = ws.warp(x, y, x + dc, y + dr, None, 'shorter', (400, 400), image=img2, keep_zero=True)
    both = mask & (ideal['covered'] > 0)
    before, after, best = corr(img1, img2, both), corr(img1, out, both), corr(img1, ideal['out'], both)
    print('correlation with image 1: %.4f unwarped, %.4f warped with the matched positions, %.4f with the true field, %d pixels'
          % (before, after, best, both.sum()))
    assert both.sum() > 40000 and best > before
    assert after >= (before + best) / 2
