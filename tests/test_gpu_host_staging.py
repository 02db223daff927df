"""The host-buffer entry points on the GPU, call after call through one staging block (csrc/host_util.h DevicePool, Carver,
Staging): large after small after large, optional regions present and absent in turn, entry points that carve the same block
differently interleaved, and a release in between.  Every call is compared bit for bit with the same entry point at
device = -1, or with the unit's specification (sid_defor, sid_ft: NumPy restatements and the oracle)."""
import threading

import numpy as np
import pytest

from oracle import ft_oracle as fo
from sea_ice_drift_amd import _capi
from tests import fg_knn_spec as ks
from tests import grid_spec as gs
from tests import warp_cases as wc

pytestmark = pytest.mark.gpu


def same(got, exp):
    """Tuples of arrays (None: not asked for): integers equal, floats with identical bits and NaN in the same places."""
    assert len(got) == len(exp)
    for g, e in zip(got, exp):
        if g is None or e is None:
            assert g is None and e is None
        elif np.issubdtype(np.asarray(e).dtype, np.floating):
            assert gs.same_bits(g, e)
        else:
            np.testing.assert_array_equal(g, e)


# ---------------------------------------------------------------- sid_defor
def triangles(rng, n, m, dtype):
    """m triangles with three different corners each among n nodes, a third of the indices written as negative ones."""
    a = rng.integers(0, n, m)
    d1, d2 = rng.integers(1, n // 3 + 1, m), rng.integers(1, n // 3 + 1, m)
    t = np.stack([a, (a + d1) % n, (a + d1 + d2) % n], axis=1)
    t[rng.random(t.shape) < 1 / 3] -= n
    return np.ascontiguousarray(t, dtype=dtype)


def defor_case(seed, n, m, dtype):
    rng = np.random.default_rng(seed)
    x, y, u, v = rng.uniform(0, 1000, (4, n))
    t = triangles(rng, n, m, dtype)
    with np.errstate(all='ignore'):
        return (x, y, u, v, t), gs.np_triangulation(x, y, u, v, t)


def test_defor_triangulation_large_small_large():
    small32, big64, small64, big32 = (defor_case(1, 40, 3, np.int32), defor_case(2, 2000, 5000, np.int64),
                                      defor_case(3, 40, 3, np.int64), defor_case(4, 2000, 5000, np.int32))
    _capi.release_workspaces()
    for args, exp in (small32, big64, small64, big32, small32):            # (the block's t region changes width)
        same(_capi.defor_triangulation(*args), exp)
    _capi.release_workspaces()
    same(_capi.defor_triangulation(*small64[0]), small64[1])
    x, y, u, v, t = big32[0]
    bad = t.copy()
    bad[4321, 1] = 2000                                                    # outside [-n, n)
    with pytest.raises(IndexError):
        _capi.defor_triangulation(x, y, u, v, bad)
    same(_capi.defor_triangulation(*small32[0]), small32[1])
    same(_capi.defor_triangulation(*big32[0]), big32[1])


def test_defor_elems_large_small_large_between_triangulations():
    def elems_case(seed, m):
        rng = np.random.default_rng(seed)
        x, y, u, v = rng.uniform(0, 1000, (4, 3, m))
        a = rng.uniform(1, 100, m)
        return (x, y, u, v, a), gs.np_elems(x, y, u, v, a)
    small, big = elems_case(5, 3), elems_case(6, 5000)
    tri = defor_case(7, 40, 3, np.int32)
    _capi.release_workspaces()
    for args, exp in (small, big, small):
        same(_capi.defor_elems(*args), exp)
        same(_capi.defor_triangulation(*tri[0]), tri[1])                   # (the same block, carved differently)
    _capi.release_workspaces()
    same(_capi.defor_elems(*small[0]), small[1])


# ---------------------------------------------------------------- sid_grid
def grid_case(seed, rows, cols):
    rng = np.random.default_rng(seed)
    x, y = wc.node_grid(rows, cols, 10.0, 10.0, jitter=0.2, seed=seed)
    u, v = np.round(rng.standard_normal((2, rows, cols)), 1)
    u[rng.random((rows, cols)) < 0.05] = np.nan
    valid = (rng.random((rows, cols)) >= 0.2).astype(np.uint8)
    return x, y, u, v, valid


def test_grid_filter_and_deformation_share_one_block():
    cases = [grid_case(11, 2, 2), grid_case(12, 40, 50), grid_case(13, 2, 3)]
    _capi.release_workspaces()
    for with_valid in (True, False, True):
        for x, y, u, v, valid in cases:
            va = valid if with_valid else None
            for radius in (1, 2):
                args = (u, v, va, 0.1, 2.0, radius, 3)
                same(_capi.grid_filter(*args), _capi.grid_filter(*args, device=-1))
                for diagonal in (0, 1, 2):                                  # (interleaved: the other carving of the block)
                    same(_capi.grid_deformation(x, y, u, v, va, diagonal), _capi.grid_deformation(x, y, u, v, va, diagonal, device=-1))
        _capi.release_workspaces()


# ---------------------------------------------------------------- sid_warp
WANTS = [(True, False, False), (False, True, False), (False, False, True), (True, True, True), (False, True, True)]   # out, covered, maps


@pytest.mark.parametrize('dtype', ['uint8', 'float32'])
def test_warp_optional_regions_come_and_go(dtype):
    x, y = wc.node_grid(6, 6, 60.0, 60.0, r0=-20.0, c0=-15.0, jitter=0.2, seed=21)
    xs, ys = wc.smooth_source(x, y, 21, shift=(4.0, -3.0))
    valid = wc.holes(x.shape, 21, share=0.1)
    wide = wc.image_u8((230, 350), 22, zeros=0.05) if dtype == 'uint8' else wc.image_f32((230, 350), 22)
    strided = wide[:, :290]                                                # src_stride 350 > cols_s 290
    assert not strided.flags['C_CONTIGUOUS']
    flags = 1 if dtype == 'uint8' else 0                                   # SID_WARP_KEEP_ZERO
    _capi.release_workspaces()
    k = 0
    for out_shape in ((16, 64), (200, 300), (16, 64)):
        for va in (valid, None):
            for want in WANTS:
                k += 1
                src = None if want == WANTS[-1] else strided if k % 2 else np.ascontiguousarray(strided)
                args = (x, y, xs, ys, va, src, dtype, strided.shape, out_shape, k % 2, 7, k % 3, flags) + want
                same(_capi.warp_image(*args), _capi.warp_image(*args, device=-1))


# ---------------------------------------------------------------- sid_ft
def descriptors(rng, n2, n1):
    d2 = rng.integers(0, 256, (n2, 32), dtype=np.uint8)
    d1 = rng.integers(0, 256, (n1, 32), dtype=np.uint8)
    if n2:
        near = d2[rng.integers(0, n2, n1)].copy()
        near[:, rng.integers(0, 32)] ^= 0x5a                               # near matches
        d1[::2] = near[::2]
    return d1, d2


_ft = {}


def ft_cases():
    if not _ft:
        rng = np.random.default_rng(41)
        for n1, n2 in ((1, 0), (3000, 2900), (5, 7)):
            d1, d2 = descriptors(rng, n2, n1)
            _ft[n1, n2] = (d1, d2, fo.knn2(d1, d2))
    return _ft


def ft_series(device, errors=None):
    try:
        for key in ((1, 0), (3000, 2900), (5, 7), (3000, 2900)):
            d1, d2, exp = ft_cases()[key]
            same(_capi.ft_knn2(d1, d2, device=device), exp)
    except BaseException as e:                                             # (a thread: hand it to the test)
        if errors is None:
            raise
        errors.append(e)


def test_ft_knn2_large_small_large():
    _capi.release_workspaces()
    ft_series(0)
    _capi.release_workspaces()
    d1, d2, exp = ft_cases()[5, 7]
    same(_capi.ft_knn2(d1, d2), exp)


def test_ft_knn2_on_two_devices_side_by_side():
    """The pool has one mutex per device: two threads on two devices do not wait for each other, and each gets its own block."""
    import torch
    if torch.cuda.device_count() < 2:
        pytest.skip('needs two visible devices')
    ft_cases()
    errors = []
    threads = [threading.Thread(target=ft_series, args=(d, errors)) for d in (0, 1, 0, 1)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors


# ---------------------------------------------------------------- sid_fg
@pytest.mark.parametrize('n', [255, 256, 257])
def test_fg_both_entry_points_on_either_side_of_the_bucket_threshold(monkeypatch, n):
    """sid_fg_nearest_dist and sid_fg_knn build the buckets with one function (from 256 seeds on): each equals its
    SID_FG_NO_GRID=1 run, the host instance and the specification, and the two agree on the nearest seed's distance."""
    rng = np.random.default_rng(50 + n)
    s, v, q = rng.uniform(0, 1000, (n, 2)), rng.normal(0, 9, (n, 2)), rng.uniform(-100, 1100, (400, 2))
    exp = ks.knn(s, v, q, 3, None)
    for no_grid in (False, True, False):
        if no_grid:
            monkeypatch.setenv('SID_FG_NO_GRID', '1')
        else:
            monkeypatch.delenv('SID_FG_NO_GRID', raising=False)
        got = _capi.fg_knn(s, v, q, k=3, details=True)
        same(got, _capi.fg_knn(s, v, q, k=3, details=True, device=-1))
        same(got, exp[:3])
        np.testing.assert_array_equal(_capi.fg_nearest_dist(s, q), np.sqrt(exp[3][:, 0]))
