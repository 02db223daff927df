"""GPU parity at the edges of the images: search windows flush with / clipped by the edges of image 2 (NumPy slicing,
pmlib.py:200-202), templates whose bounding box reaches the edges of image 1, the points where the reference raises - through
the public calls against fixture G9, through every launch path against the C oracle, and through every way of binding a pair,
with the bytes around a borrowed image set to sentinels that must not change a result.

Where the points run: a window clipped by the bottom / right edge of image 2 always runs the large-window pipeline
(pm_capi.hip classify_points; the one-point kernels are not validated on such shapes, and their prologues reject them).  So
the one-point kernel paths below see the flush windows - which reach the last row and column of image 2 and exercise the
clamped loads there -, the fractional starts, the edge templates and the NaN cases; their clipped points check the
pipeline's answer under that path's switches."""
import os

import numpy as np
import pytest
import torch

from sea_ice_drift_amd import _capi, pmlib as my, synthetic as syn
from tests.golden import make_golden as mg
from tests.test_gpu_parity import assert_parity, rot_for

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
ANGLES3, ANGLES7, ANGLES15, ANGLES17 = [-3, 0, 3], list(range(-3, 4)), list(range(-7, 8)), list(range(-8, 9))
ENVS = ('SID_PM_NO_W3', 'SID_PM_ALWAYS_GS', 'SID_PM_NO_SAMP_TABLE', 'SID_PM_NO_RP', 'SID_PM_ALL_LARGE')


def edge_points(img1, img2, s, alpha0, angles, order, borders):
    names, c1, r1, c2fg, r2fg, border, raises = mg.g9_points(img1, img2, s, alpha0, angles, min(order, 1), borders)
    return names, (c1, r1, c2fg, r2fg, border), raises


def set_env(monkeypatch, env):
    for k in ENVS:
        monkeypatch.delenv(k, raising=False)
    if env:
        monkeypatch.setenv(env, '1')


def assert_fixture(got, exp, raises, got_ij=None, mcc_norm=False):
    """assert_parity's bar against a reference fixture: c2, r2, a exact; r exact (within 1e-5 with mcc_norm); h within 1e-5
    (NaN where the reference's is NaN); NaN rows exactly on the cases where the reference raises."""
    nan = np.isnan(got[:, 0])
    np.testing.assert_array_equal(nan, raises)
    assert np.isnan(got[nan]).all()
    g, e = got[~nan], exp[~nan]
    np.testing.assert_array_equal(g[:, :3], e[:, :3])
    if mcc_norm:
        np.testing.assert_allclose(g[:, 3], e[:, 3], rtol=1e-5, atol=1e-5)
    else:
        np.testing.assert_array_equal(g[:, 3], e[:, 3])
    np.testing.assert_allclose(g[:, 4], e[:, 4], rtol=1e-5, atol=1e-5)
    if got_ij is not None:
        assert (got_ij[nan] == -1).all() and (got_ij[~nan] >= 0).all()


# ---------------------------------------------------------------- 1. G9 through the public calls
@pytest.mark.parametrize('p', range(len(mg.G9_PAIRS)))
def test_g9_edges_through_use_mcc_pm_dispatch_and_sid_pm_batch(pm_ctx, c_oracle, p):
    g = np.load(os.path.join(GOLD, 'g9_edges.npz'))
    img1, img2 = mg.g9_pair(p)
    assert syn.sha256(img1, img2) == str(g['pair%d_sha' % p])
    for s, alpha0, order in mg.G9_VARIANTS:
        key = 'p%d_s%d_o%d' % (p, s, order)
        pts, exp = g['pts_' + key], g['out_' + key]
        raised = set(str(x).split(':')[0] for x in g['raised_' + key])
        raises = np.array([str(n) in raised for n in g['names_' + key]])
        v = [pts[:, k] for k in range(5)]
        kw = dict(angles=mg.G9_ANGLES, rot_order=order)
        got = my.pm_dispatch(img1, img2, *v, s, alpha0, context=pm_ctx, **kw)
        assert_fixture(got, exp, raises)
        rot, flags = rot_for(mg.G9_ANGLES, alpha0, s), _capi.flags_from_kwargs(rot_order=order)
        got, ij = _capi.pm_batch(img1, img2, *v, s, alpha0, mg.G9_ANGLES, rot=rot, flags=flags)
        assert_fixture(got, exp, raises, ij)
        # the peak indices exactly: the C oracle reproduces the fixture bit for bit (tests/test_oracle_golden.py) and gives them
        exp_c, exp_ij = c_oracle.pm_batch(img1, img2, *v, s, alpha0, mg.G9_ANGLES, rot=rot, flags=flags, nthreads=16)
        np.testing.assert_array_equal(exp_c, exp)
        np.testing.assert_array_equal(ij, exp_ij)
        got = np.array([my.use_mcc(*pts[i], img1, img2, s, alpha0, **kw) for i in range(len(pts))], dtype=np.float64)
        assert_fixture(got, exp, raises)


# ---------------------------------------------------------------- 2. the edge set through every launch path
# (s, angles, flags, borders, switch): the row-pair kernel (its three-wavefront, slot-group, full-table, global-sums and big
# layouts), the classic kernel, the large-window pipeline, both sampling routes, rot_order 1 and 3, hes_smth + mcc_norm
PATHS = {
    'rp34_b20_23_24_50': (34, ANGLES3, 1, (20, 23, 24, 50), None),
    'rp35_b20_23_24_50': (35, ANGLES7, 1, (20, 23, 24, 50), None),
    'rp34_big_b69_111': (34, ANGLES15, 1, (69, 111), None),
    'rp35_big_b69': (35, ANGLES17, 1, (69,), None),
    'rp34_no_w3': (34, ANGLES3, 1, (20, 23), 'SID_PM_NO_W3'),
    'rp35_always_gs': (35, ANGLES15, 1, (24, 50), 'SID_PM_ALWAYS_GS'),
    'rp34_no_samp_table': (34, ANGLES7, 1, (20, 50), 'SID_PM_NO_SAMP_TABLE'),
    'classic21': (21, ANGLES3, 1, (20, 50), 'SID_PM_NO_RP'),
    'classic64': (64, ANGLES17, 1, (20,), 'SID_PM_NO_RP'),
    'classic34_b23': (34, ANGLES15, 1, (23,), 'SID_PM_NO_RP'),
    'large80': (80, ANGLES3, 1, (20,), 'SID_PM_ALL_LARGE'),
    'large34': (34, ANGLES7, 1, (20, 50), 'SID_PM_ALL_LARGE'),
    'rot_order1': (35, ANGLES7, 1 | _capi.rot_order_flag(1), (20, 50), None),
    'rot_order3': (34, ANGLES3, 1 | _capi.rot_order_flag(3), (20, 24), None),
    'flags7': (34, ANGLES7, 7, (20, 50), None),
    'flags7_classic': (21, ANGLES15, 7, (20,), 'SID_PM_NO_RP'),
}


@pytest.mark.parametrize('path', sorted(PATHS))
def test_edge_points_every_launch_path_against_the_oracle(pm_ctx, c_oracle, monkeypatch, path):
    s, angles, flags, borders, env = PATHS[path]
    alpha0 = -3.85 if s % 2 else 0.0
    order = (flags >> 3) & 7
    set_env(monkeypatch, env)
    try:
        for p in range(len(mg.G9_PAIRS)):
            img1, img2 = mg.g9_pair(p)
            names, v, raises = edge_points(img1, img2, s, alpha0, angles, order, borders)
            rot = rot_for(angles, alpha0, s)
            exp, exp_ij = c_oracle.pm_batch(img1, img2, *v, s, alpha0, angles, rot=rot, flags=flags, nthreads=16)
            np.testing.assert_array_equal(np.isnan(exp[:, 0]) & raises, raises)
            assert np.isfinite(exp[:, 0]).sum() >= len(names) // 3            # (spline order 3: overshoots to 0 turn more templates NaN)
            pm_ctx.upload_pair(img1, img2)
            pm_ctx.set_points(*v, s, alpha0, angles, rot=rot, flags=flags)
            pm_ctx.run()
            got, got_ij = pm_ctx.fetch()
            assert_parity(got, got_ij, exp, exp_ij, mcc_norm=bool(flags & 4))
    finally:
        set_env(monkeypatch, None)


# ---------------------------------------------------------------- 3. the ways of binding a pair, with sentinels around it
BIND_PATHS = {
    'rp34': (34, ANGLES7, 1, None),
    'classic21': (21, ANGLES3, 1, 'SID_PM_NO_RP'),
    'large80': (80, ANGLES3, 1, None),
    'large34': (34, ANGLES3, 1, 'SID_PM_ALL_LARGE'),
    'spline3': (35, ANGLES3, 1 | _capi.rot_order_flag(3), None),
}


def padded_view(img, off, stride, fill, rng):
    """A device buffer of off + rows * stride + 64 bytes filled with `fill` (0, 255 or 'random'), and the image written into the
    view that starts `off` bytes in with row stride `stride`: returns (buffer, address of the view)."""
    rows, cols = img.shape
    n = off + rows * stride + 64
    if fill == 'random':
        host = rng.integers(0, 256, n, dtype=np.uint8)
    else:
        host = np.full(n, fill, dtype=np.uint8)
    host[off:off + rows * stride].reshape(rows, stride)[:, :cols] = img
    buf = torch.from_numpy(host).cuda()
    return buf, buf.data_ptr() + off


@pytest.mark.parametrize('path', sorted(BIND_PATHS))
def test_edge_points_every_pair_binding_with_sentinels(pm_ctx, c_oracle, monkeypatch, path):
    s, angles, flags, env = BIND_PATHS[path]
    alpha0 = 0.0
    order = (flags >> 3) & 7
    img1, img2 = mg.g9_pair(1)
    names, v, raises = edge_points(img1, img2, s, alpha0, angles, order, (20, 50))
    rot = rot_for(angles, alpha0, s)
    exp, exp_ij = c_oracle.pm_batch(img1, img2, *v, s, alpha0, angles, rot=rot, flags=flags, nthreads=16)
    assert np.isfinite(exp[:, 0]).sum() >= len(names) // 3
    set_env(monkeypatch, env)
    rng = np.random.default_rng(1234)
    runs = {}

    def run(tag):
        pm_ctx.set_points(*v, s, alpha0, angles, rot=rot, flags=flags)
        pm_ctx.run()
        runs[tag] = pm_ctx.fetch()                                   # (synchronous: the borrowed buffers are still alive)

    try:
        pm_ctx.upload_pair(img1, img2)                               # (a) contiguous host arrays
        run('upload')
        h1 = np.full((img1.shape[0], img1.shape[1] + 13), 7, dtype=np.uint8)
        h2 = np.full((img2.shape[0], img2.shape[1] + 29), 7, dtype=np.uint8)
        h1[:, 3:3 + img1.shape[1]] = img1
        h2[:, 5:5 + img2.shape[1]] = img2
        v1, v2 = h1[:, 3:3 + img1.shape[1]], h2[:, 5:5 + img2.shape[1]]
        assert v1.strides[0] > v1.shape[1] and v2.strides[0] > v2.shape[1]
        pm_ctx.upload_pair(v1, v2)                                   # (b) host views, stride > width
        run('upload_strided')
        t1, t2 = torch.from_numpy(img1).cuda(), torch.from_numpy(img2).cuda()
        pm_ctx.bind_pair_tensors(t1, t2)                             # (c) device tensors of exactly the image size
        run('tensors')
        for off in (1, 2, 3):                                        # (d) views into larger buffers: odd strides, odd bases
            st1, st2 = (img1.shape[1] + 2 * off + 5) | 1, (img2.shape[1] + 2 * off + 9) | 1
            assert st1 % 2 and st2 % 2
            for fill in (0, 255, 'random'):
                b1, p1 = padded_view(img1, off, st1, fill, rng)
                b2, p2 = padded_view(img2, off + 1, st2, fill, rng)
                pm_ctx.bind_pair_ptr(p1, img1.shape[0], img1.shape[1], st1, p2, img2.shape[0], img2.shape[1], st2)
                run('ptr_off%d_%s' % (off, fill))
    finally:
        set_env(monkeypatch, None)
    got, got_ij = runs['upload']
    assert_parity(got, got_ij, exp, exp_ij, mcc_norm=bool(flags & 4))
    for tag, (g, ij) in runs.items():
        np.testing.assert_array_equal(ij, got_ij, err_msg=tag)
        np.testing.assert_array_equal(g, got, err_msg=tag)          # bit-identical, h included


# ---------------------------------------------------------------- 4. debug_point: the one-point kernels never see a clipped window
def test_debug_point_refuses_a_clipped_window_and_takes_a_flush_one(pm_ctx, c_oracle):
    """sid_pm_debug_point launches a one-point kernel directly: a window clipped by the edge of image 2 is SID_PM_ERR_UNSUPPORTED
    there (the batch entry points run it through the large-window pipeline and return the reference's value); a window flush
    with the last row and column still runs and agrees with the batch."""
    g = np.load(os.path.join(GOLD, 'g9_edges.npz'))
    img1, img2 = mg.g9_pair(0)
    s, alpha0, angles = 34, 0.0, mg.G9_ANGLES
    key = 'p0_s34_o0'
    names, pts, exp = [str(n) for n in g['names_' + key]], g['pts_' + key], g['out_' + key]
    rot = rot_for(angles, alpha0, s)
    pm_ctx.upload_pair(img1, img2)
    for name in ('b20_clip1_bottom', 'b20_clip3_right', 'b50_clip47_both', 'b20_min_both'):
        i = names.index(name)
        assert np.isfinite(exp[i, :4]).all()
        with pytest.raises(_capi.SidPmError) as e:
            pm_ctx.debug_point(*pts[i], s, alpha0, angles, rot=rot)
        assert e.value.code == -4, name
        got, ij = _capi.pm_batch(img1, img2, *[pts[i:i + 1, k] for k in range(5)], s, alpha0, angles, rot=rot)
        assert_fixture(got, exp[i:i + 1], np.array([False]), ij)
    for name in ('b20_flush_br', 'b50_flush_br'):
        i = names.index(name)
        d = pm_ctx.debug_point(*pts[i], s, alpha0, angles, rot=rot)
        exp_c, exp_ij = c_oracle.pm_batch(img1, img2, *[pts[i:i + 1, k] for k in range(5)], s, alpha0, angles, rot=rot)
        np.testing.assert_array_equal(d['ij'], exp_ij[0])
        np.testing.assert_array_equal(d['out'][:4], exp[i, :4])
        assert d['ccm'].shape == (int(pts[i, 4]) * 2 + 2,) * 2
