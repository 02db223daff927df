"""GPU tests of include/sid_corr.h: every case of tests/corr_cases.py on the device bit for bit against the specification
(tests/corr_spec.py) - NumPy route and device tensors (side stream, strided views, poisoned outputs, no copy to the host) -
each twice with identical bytes, the device entry points with padded outputs, and the end-to-end check on the smoke pair."""
import numpy as np
import pytest

from sea_ice_drift_amd import _capi, libcorr, libwarp, pmlib, synthetic
from tests import corr_cases as cc
from tests import corr_spec as cs
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
    out = torch.empty(tuple(tensor.shape), dtype=tensor.dtype)
    out.copy_(tensor)
    return np.from_dlpack(out).copy()


def on_device(torch, a, strided=False):
    """`a` on the device; `strided`: a 2-D array as a view with padded rows that starts at column 3."""
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
    for dtype, val in ((torch.float64, -12345.678), (torch.int32, -77), (torch.int64, -99)):
        blocks = [torch.full((1 << 16,), val, dtype=dtype, device='cuda') for _ in range(4)]
        del blocks


def through_libcorr(c, conv, **kw):
    a, b = conv(c['a']), conv(c['b'])
    if c['kind'] == 'lattice':
        return libcorr.local_correlation(a, b, window=c['window'], step=c['step'], origin=c['origin'], shape=c['shape'],
                                         min_count=c['min_count'], return_count=True, return_sums=True, **kw)
    return libcorr.local_correlation_at(a, b, conv(c['c']), conv(c['r']), window=c['window'], valid=conv(c['valid']),
                                        min_count=c['min_count'], return_count=True, return_sums=True, **kw)


def same(p, q):
    return all(cs.same_bits(x, y) for x, y in zip(p, q))


# ---------------------------------------------------------------- the cases
@pytest.mark.parametrize('name', cc.NAMES)
def test_case_numpy_route(name):
    c = cc.BY_NAME[name]
    first = through_libcorr(c, lambda q: q)
    cc.check(first, name, 'numpy route')
    assert same(first, through_libcorr(c, lambda q: q)), 'two runs differ'


@pytest.mark.parametrize('name', cc.NAMES)
def test_case_tensor_route(no_host_copies, name):
    torch = no_host_copies
    c = cc.BY_NAME[name]
    runs = []
    for strided in (True, False):
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            poison_pool(torch)
            got = through_libcorr(c, lambda q: on_device(torch, q, strided))
        s.synchronize()
        assert all(g.is_cuda for g in got)
        runs.append(tuple(_host(g) for g in got))
        cc.check(runs[-1], name, 'tensor route, strided inputs' if strided else 'tensor route')
    assert same(*runs), 'two runs differ'


def test_device_entry_points_with_padded_outputs(no_host_copies):
    """sid_corr_lattice_device and sid_corr_points_device write their nodes and nothing around them; all three outputs, then
    each output alone."""
    torch = no_host_copies
    for name in ('step_smaller', 'points_valid'):
        c, e = cc.BY_NAME[name], cc.expected(name)
        a, b = on_device(torch, c['a'], True), on_device(torch, c['b'])
        n = e['count'].size
        stream = torch.cuda.current_stream().cuda_stream

        def run(r, count, sums):
            ptr = [q[16:].data_ptr() if q is not None else 0 for q in (r, count, sums)]
            if c['kind'] == 'lattice':
                (sr, sc), (r0, c0), (nr, nc), m = cc.resolved(c)
                _capi.corr_lattice_device(a.data_ptr(), a.stride(0), b.data_ptr(), b.stride(0), a.shape[0], a.shape[1], c['window'],
                                          r0, c0, sr, sc, nr, nc, m, *ptr, stream)
            else:
                cen = [on_device(torch, np.ascontiguousarray(c[k], dtype=np.int32).ravel()) for k in ('c', 'r')]
                valid = on_device(torch, np.ascontiguousarray(c['valid'], dtype=np.uint8).ravel())
                _capi.corr_points_device(a.data_ptr(), a.stride(0), b.data_ptr(), b.stride(0), a.shape[0], a.shape[1], c['window'],
                                         cen[0].data_ptr(), cen[1].data_ptr(), valid.data_ptr(), n, c['min_count'], *ptr, stream)
            torch.cuda.synchronize()

        def padded():
            return (torch.full((n + 32,), -12345.678, dtype=torch.float64, device='cuda'),
                    torch.full((n + 32,), -77, dtype=torch.int32, device='cuda'),
                    torch.full((5 * n + 32,), -99, dtype=torch.int64, device='cuda'))
        for wanted in ((0, 1, 2), (0,), (1,), (2,)):
            bufs = padded()
            for _ in range(2):
                run(*[q if k in wanted else None for k, q in enumerate(bufs)])
            for k, (key, poison) in enumerate((('r', -12345.678), ('count', -77), ('sums', -99))):
                h = _host(bufs[k])
                if k not in wanted:
                    assert (h == poison).all()
                    continue
                assert (h[:16] == poison).all() and (h[16 + e[key].size:] == poison).all(), 'written outside the output'
                assert cs.same_bits(h[16:16 + e[key].size].reshape(e[key].shape), e[key]), '%s: %s' % (name, key)


def test_release_and_run_again():
    c = cc.BY_NAME['step_smaller']
    first = through_libcorr(c, lambda q: q)
    _capi.release_workspaces()
    assert same(first, through_libcorr(c, lambda q: q))


# ---------------------------------------------------------------- end to end
def test_pattern_matching_then_warp_then_local_correlation():
    """The smoke pair and grid: sub-pixel pattern matching, image 2 warped onto image 1 with the matched positions, then the
    local correlation with image 1 at the grid nodes.  Its mean over the nodes that are finite in all three runs reaches at least
    the midpoint between the unwarped value and the one the specification gets with the true field on the same nodes.
    The grid's hull is what the warp covers, so a window of 35 around a node on the hull's edge holds 17 or 18 of its 35 rows or
    columns and one around a corner 17 x 17 pixels at the least: min_count = 200 (below 289) lets every node take part."""
    img1, img2 = synthetic.make_pair(400, 400, seed=17)
    g = synthetic.make_grid(400, 400, 6, margin=90)
    res = pmlib.pm_dispatch(img1, img2, g['c1'], g['r1'], g['c2fg'], g['r2fg'], g['border'], 34, 0.0, subpixel=True)
    x, y = g['c1'].reshape(6, 6), g['r1'].reshape(6, 6)
    xs, ys = np.ascontiguousarray(res[:, 0]).reshape(6, 6), np.ascontiguousarray(res[:, 1]).reshape(6, 6)
    assert np.isfinite(xs).all() and np.isfinite(ys).all()
    warped = libwarp.warp_image(img2, x, y, xs, ys)
    c, r = np.rint(x).astype(np.int32), np.rint(y).astype(np.int32)
    after = libcorr.local_correlation_at(img1, warped, c, r, window=35, min_count=200)
    assert cs.same_bits(after, cs.points(img1, warped, 35, c, r, None, 200)['r'])
    before = libcorr.local_correlation_at(img1, img2, c, r, window=35, min_count=200)
    dc, dr = synthetic.true_displacement(x, y)
    ideal = ws.warp(x, y, x + dc, y + dr, None, 'shorter', (400, 400), image=img2, keep_zero=True)['out']
    best = cs.points(img1, ideal, 35, c, r, None, 200)['r']
    ok = np.isfinite(before) & np.isfinite(after) & np.isfinite(best)
    print('mean local correlation with image 1 over %d of %d nodes: %.4f unwarped, %.4f warped with the matched positions, %.4f with '
          'the true field' % (ok.sum(), ok.size, before[ok].mean(), after[ok].mean(), best[ok].mean()))
    assert 2 * ok.sum() >= ok.size and best[ok].mean() > before[ok].mean()
    assert after[ok].mean() >= (before[ok].mean() + best[ok].mean()) / 2
