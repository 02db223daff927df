"""GPU parity of the front end of the row-pair kernels - the window load (ph_window_t, csrc/pm_kernel_phases.h) and the box sums of
w'^2 (rp_sums, csrc/pm_kernel_rp.inc) - on a pair made for them: image 1 holds only the bytes 1 and 255, image 2 is image 1 rolled by
(3, -2) with every 1 turned into 0, so that the re-centred window bytes are the extremes -128 (square 16 384) and 127, plus one
constant block of 0 and one of 255 (flat windows: sum w'^2 = N * 16 384 and N * 16 129, variance exactly 0).  A packed or byte-wise
sum that drops a carry or a sign shows here.

_capi against the C oracle under the parity rule of test_gpu_ragged_tiles.py - peak row / column / angle index, c2, r2, a, r
bit-exact, h within rtol = atol = 1e-5 - with no point left out and NaN rows compared as NaN.

Borders: 1, 2, 3 (fewer placement columns than a segment of the sums), both ends of every launch class (20 .. 68, with 50, the
benchmark's largest), the last border with the per-placement tables in LDS (68) and two that keep them in global memory (69, 100)."""
import numpy as np
import pytest

from sea_ice_drift_amd import _capi, pmlib as my, synthetic as syn

pytestmark = pytest.mark.gpu

SIZE = 700
BORDERS = (1, 2, 3, 20, 23, 24, 27, 28, 36, 37, 47, 48, 50, 68, 69, 100)
ANGLES = {15: list(range(-7, 8)), 7: list(range(-3, 4)), 3: [-3, 0, 3]}
GS_ENVS = ('SID_PM_ALWAYS_GS', 'SID_PM_NO_GS')


def _pair():
    rng = np.random.default_rng(8100)
    img1 = np.where(rng.integers(0, 2, size=(SIZE, SIZE)) == 1, 255, 1).astype(np.uint8)
    assert img1.min() == 1                                           # (a template with a zero byte is refused by the reference)
    img2 = np.roll(img1, (3, -2), axis=(0, 1))
    img2[img2 == 1] = 0
    img2[0:200, 0:200] = 0
    img2[500:, 500:] = 255
    return img1, np.ascontiguousarray(img2)


def _grid():
    parts = [syn.make_grid(SIZE, SIZE, 4, border=b, margin=b + 30, seed=b) for b in BORDERS]
    return {k: np.concatenate([p[k] for p in parts]) for k in parts[0]}


def _corners():
    """Windows flush with the edges of image 2: all four corners - rows / columns from 0, rows / columns up to the last one - at
    one border of every launch class.  (hws = 17 for both template sides.)"""
    c2, r2, bb = [], [], []
    for b in (20, 24, 36, 50, 69):
        lo, hi = 17.0 + b, SIZE - 18.0 - b
        for (c, r) in ((lo, lo), (hi, lo), (lo, hi), (hi, hi)):
            c2.append(c); r2.append(r); bb.append(float(b))
    n = len(bb)
    rng = np.random.default_rng(8101)
    return dict(c1=np.rint(rng.uniform(150, SIZE - 150, n)), r1=np.rint(rng.uniform(150, SIZE - 150, n)),
                c2fg=np.array(c2), r2fg=np.array(r2), border=np.array(bb))


@pytest.fixture(scope='module')
def pair():
    return _pair()


_REF = {}


def _oracle(c_oracle, pair, name, g, s, k):
    """The C oracle's answer, computed once per (points, side, angle set) and shared by the tests."""
    key = (name, s, k)
    if key not in _REF:
        rot = my.rotation_table(ANGLES[k], 0.0, s)
        exp, exp_ij = c_oracle.pm_batch(pair[0], pair[1], g['c1'], g['r1'], g['c2fg'], g['r2fg'], g['border'], s, 0.0, ANGLES[k],
                                        rot=rot, nthreads=16)
        exp.setflags(write=False); exp_ij.setflags(write=False)
        _REF[key] = (exp, exp_ij)
    return _REF[key]


def _compare(got, ij, exp, exp_ij):
    """The parity rule over every row; a NaN row of the oracle must be a NaN row of the kernel."""
    np.testing.assert_array_equal(ij, exp_ij)
    nan = np.isnan(exp)
    np.testing.assert_array_equal(np.isnan(got), nan)
    np.testing.assert_array_equal(got[:, :4][~nan[:, :4]], exp[:, :4][~nan[:, :4]])
    np.testing.assert_allclose(got[:, 4], exp[:, 4], rtol=1e-5, atol=1e-5, equal_nan=True)


def _run_ctx(ctx, g, s, k):
    ctx.set_points(g['c1'], g['r1'], g['c2fg'], g['r2fg'], g['border'], s, 0.0, ANGLES[k], rot=my.rotation_table(ANGLES[k], 0.0, s))
    ctx.run()
    return ctx.fetch()


@pytest.mark.parametrize('s,k', [(34, 15), (34, 7), (34, 3), (35, 15), (35, 7), (35, 3), (20, 15)])
def test_every_border_class(pm_ctx, c_oracle, pair, s, k):
    """16 points per border; 15, 7 and 3 angles (workgroups of 192 / 256 / 768 threads, the slot-group kernels), template sides 34
    and 35, and the classic kernel (side 20), which shares the window phase."""
    g = _grid()
    assert g['c1'].size == 16 * len(BORDERS)
    exp, exp_ij = _oracle(c_oracle, pair, 'grid', g, s, k)
    finite = np.isfinite(exp).all(axis=1).reshape(len(BORDERS), 16).sum(axis=1)
    print('finite oracle rows per border:', dict(zip(BORDERS, finite.tolist())))
    assert (finite >= 12).all()
    pm_ctx.upload_pair(*pair)
    got, ij = _run_ctx(pm_ctx, g, s, k)
    _compare(got, ij, exp, exp_ij)


@pytest.mark.parametrize('s', [34, 35])
def test_both_homes_of_the_sums(pm_ctx, c_oracle, pair, monkeypatch, s):
    """Borders 20 and 24 with sum w'^2 in LDS and in global memory (SID_PM_NO_GS / SID_PM_ALWAYS_GS; read when the points are set)."""
    g = _grid()
    sel = np.isin(g['border'], (20.0, 24.0))
    g = {key: v[sel] for key, v in g.items()}
    exp, exp_ij = _oracle(c_oracle, pair, 'b20_24', g, s, 15)
    assert np.isfinite(exp).all(axis=1).sum() >= 24
    pm_ctx.upload_pair(*pair)
    try:
        for env in GS_ENVS:
            for e in GS_ENVS:
                monkeypatch.delenv(e, raising=False)
            monkeypatch.setenv(env, '1')
            got, ij = _run_ctx(pm_ctx, g, s, 15)
            _compare(got, ij, exp, exp_ij)
    finally:
        for e in GS_ENVS:
            monkeypatch.delenv(e, raising=False)


@pytest.mark.parametrize('k,borders', [(15, (20, 24, 28, 37, 48, 68)), (7, (20, 36)), (3, (20, 50))])
def test_whole_ncc_matrix(pm_ctx, c_oracle, pair, k, borders):
    """One point of a border of every launch class: every value of the winning angle's NCC matrix (debug_point) against the
    oracle's match_template of the same window and template, bit for bit - each of them is a function of its placement's sum
    w'^2.  (debug_point runs one workgroup of 256 threads with the run-time window pitch and the sums in global memory, an
    instantiation the batch launches use for few shapes; it takes windows up to border 68, the last with its tables in LDS.)"""
    img1, img2 = pair
    g = _grid()
    s = 34
    exp, _ = _oracle(c_oracle, pair, 'grid', g, s, k)
    rot = my.rotation_table(ANGLES[k], 0.0, s)
    pm_ctx.upload_pair(img1, img2)
    for b in borders:
        i = int(np.flatnonzero((g['border'] == b) & np.isfinite(exp).all(axis=1))[0])
        d = pm_ctx.debug_point(g['c1'][i], g['r1'][i], g['c2fg'][i], g['r2fg'][i], float(b), s, 0.0, ANGLES[k], rot=rot)
        r0, c0, w = int(g['r2fg'][i]) - 17 - b, int(g['c2fg'][i]) - 17 - b, 2 * 17 + 2 * b + 1
        want = c_oracle.match_template(img2[r0:r0 + w, c0:c0 + w], d['templates'][int(d['ij'][2])])
        assert d['ccm'].shape == want.shape == (2 * b + 2, 2 * b + 2)
        np.testing.assert_array_equal(d['ccm'], want, err_msg='border %d' % b)
        np.testing.assert_array_equal(d['out'][:4], exp[i, :4])


@pytest.mark.parametrize('s,k', [(34, 15), (35, 15), (34, 3)])
def test_windows_flush_with_the_image(c_oracle, pair, s, k):
    """Windows that start at row / column 0 and windows that end on the last row and column of image 2: the pair uploaded by the
    library, and bound as unpadded device tensors (stride == cols: the byte behind the last pixel is not the image's)."""
    import torch
    g = _corners()
    exp, exp_ij = _oracle(c_oracle, pair, 'corners', g, s, k)
    assert np.isfinite(exp).all(axis=1).sum() >= len(g['border']) // 2
    with _capi.PMContext(0) as ctx:
        ctx.upload_pair(*pair)
        got, ij = _run_ctx(ctx, g, s, k)
        _compare(got, ij, exp, exp_ij)
    t1, t2 = torch.from_numpy(pair[0]).cuda(), torch.from_numpy(pair[1]).cuda()
    assert t2.stride(0) == SIZE
    with _capi.PMContext(0) as ctx:
        ctx.bind_pair_tensors(t1, t2)
        got, ij = _run_ctx(ctx, g, s, k)
        _compare(got, ij, exp, exp_ij)
