"""CPU tests: the oracle (NumPy and C forms) against the fixtures generated from the
reference's own Python (tests/golden/make_golden.py), and against each other."""
import os

import numpy as np
import pytest

from oracle import pm_oracle as po
from sea_ice_drift_amd import synthetic as syn
from tests.golden import make_golden as mg

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')


def load(name):
    return np.load(os.path.join(GOLD, name))


def rot_for(angles, alpha0, s):
    return np.array([po.rotation_terms(a - alpha0, s) for a in angles])


# ---------------------------------------------------------------- G1 get_template
def test_g1_templates_numpy_and_c(c_oracle):
    g = load('g1_templates.npz')
    img = mg.g1_image()
    assert syn.sha256(img) == str(g['img_sha'])
    k = 0
    for s, key in ((34, 't34'), (35, 't35')):
        k = 0
        for a in mg.G1_ANGLES:
            for (c, r) in mg.G1_CENTRES:
                exp = g[key][k].reshape(s, s)
                np.testing.assert_array_equal(po.get_template(img, c, r, a, s), exp)
                np.testing.assert_array_equal(c_oracle.get_template(img, c, r, po.rotation_terms(a, s), s), exp)
                k += 1
    np.testing.assert_array_equal(po.get_template(img, 5, 5, 10, 34), g['edge'])
    np.testing.assert_array_equal(c_oracle.get_template(img, 5, 5, po.rotation_terms(10, 34), 34), g['edge'])
    assert g['edge'].min() == 0


# ---------------------------------------------------------------- G1b get_template(rot_order=1)
def test_g1b_templates_order1_numpy_and_c(c_oracle):
    """scipy's bilinear sampling (pmlib.py:89,112-113 with rot_order=1), restated in NumPy and C, against the reference's
    own get_template on G1's angle / centre set and on templates cut by the image border."""
    g = load('g1b_templates_order1.npz')
    img = mg.g1_image()
    assert syn.sha256(img) == str(g['img_sha'])
    differs_from_order0 = 0
    for s, key in ((34, 't34'), (35, 't35')):
        k = 0
        for a in mg.G1_ANGLES:
            for (c, r) in mg.G1_CENTRES:
                exp = g[key][k].reshape(s, s)
                np.testing.assert_array_equal(po.get_template_order1(img, c, r, a, s), exp)
                np.testing.assert_array_equal(c_oracle.get_template(img, c, r, po.rotation_terms(a, s), s, rot_order=1), exp)
                differs_from_order0 += int((po.get_template(img, c, r, a, s) != exp).any())
                k += 1
    assert differs_from_order0 > 60                                # (integral centres at 0 / 90 degrees sample the grid itself)
    for k, (c, r, a, s) in enumerate(g['edge_args']):
        s = int(s)
        np.testing.assert_array_equal(po.get_template_order1(img, c, r, a, s), g['edge%d' % k])
        np.testing.assert_array_equal(c_oracle.get_template(img, c, r, po.rotation_terms(a, s), s, rot_order=1), g['edge%d' % k])
        assert g['edge%d' % k].min() == 0


@pytest.mark.parametrize('s,alpha0', [(34, 0.0), (35, -3.85)])
def test_g3b_use_mcc_order1(c_oracle, s, alpha0):
    g = load('g3b_use_mcc_order1.npz')
    g3 = load('g3_use_mcc.npz')
    img1, img2 = mg.g3_pair()
    assert syn.sha256(img1, img2) == str(g['pair_sha'])
    v = [g3[k] for k in ('c1', 'r1', 'c2fg', 'r2fg', 'border')]
    for k, angles in enumerate(mg.G3_ANGLE_SETS):
        exp = g['out_s%d_k%d' % (s, k)]
        got_c, ij = c_oracle.pm_batch(img1, img2, *v, s, alpha0, angles, rot=rot_for(angles, alpha0, s), flags=1 | 8, nthreads=4)
        np.testing.assert_array_equal(got_c, exp)
        assert ((ij[:, 2] == -1) == np.isnan(exp[:, 0])).all()
        if k == 0:
            got_n, _ = po.pm_batch(img1, img2, *v, s, alpha0, angles, flags=1 | po.FLAG_ROT_ORDER1)
            np.testing.assert_array_equal(got_n, exp)
        assert not np.array_equal(exp, g3['out_s%d_k%d_m0' % (s, k)], equal_nan=True)   # (order 1 is not order 0)
    assert np.isnan(g['out_s%d_k0' % s][:, 0]).any()


# ---------------------------------------------------------------- G2 get_hessian
@pytest.mark.parametrize('n', [42, 72, 101, 102])
def test_g2_hessian(c_oracle, n):
    g = load('g2_hessian.npz')
    m = g['in%d' % n]
    np.testing.assert_array_equal(po.raw_hessian(m), g['raw%d' % n])
    np.testing.assert_array_equal(po.get_hessian(m), g['norm%d' % n])
    np.testing.assert_array_equal(c_oracle.hessian(m, 0), g['raw%d' % n])
    np.testing.assert_array_equal(c_oracle.hessian(m, 1), g['norm%d' % n])
    # hes_smth: the C form restates scipy's gaussian_filter (taps, 'reflect', accumulation order) bit for bit
    np.testing.assert_array_equal(c_oracle.hessian(m, 3), g['smth%d' % n])


# ---------------------------------------------------------------- matcher
def test_match_template_definition_and_c_form(c_oracle):
    rng = np.random.default_rng(9)
    for (wh, ww, s) in ((75, 75, 34), (60, 71, 35), (40, 37, 34)):
        img = rng.integers(1, 256, (wh, ww), dtype=np.uint8)
        t = rng.integers(1, 256, (s, s), dtype=np.uint8)
        r = po.match_template(img, t)
        assert r.dtype == np.float32 and r.shape == (wh - s + 1, ww - s + 1)
        np.testing.assert_allclose(r, po.ncc_bruteforce_f64(img, t), atol=2e-7)
        np.testing.assert_array_equal(c_oracle.match_template(img, t), r)


def test_match_template_special_cases(c_oracle):
    rng = np.random.default_rng(10)
    img = rng.integers(1, 256, (50, 50), dtype=np.uint8)
    flat_t = np.full((34, 34), 77, dtype=np.uint8)
    for f in (po.match_template, c_oracle.match_template):
        np.testing.assert_array_equal(f(img, flat_t), np.ones((17, 17), dtype=np.float32))   # constant template
        flat_img = np.full((50, 50), 9, dtype=np.uint8)
        t = rng.integers(1, 256, (34, 34), dtype=np.uint8)
        np.testing.assert_array_equal(f(flat_img, t), np.zeros((17, 17), dtype=np.float32))  # no window variance
        exact = img.copy()
        exact[5:39, 7:41] = t
        r = f(exact, t)
        assert r[5, 7] == np.float32(1.0) and np.argmax(r) == 5 * 17 + 7                     # perfect match


# ---------------------------------------------------------------- G3 use_mcc
@pytest.mark.parametrize('s,alpha0', [(34, 0.0), (35, -3.85)])
def test_g3_use_mcc(c_oracle, s, alpha0):
    g = load('g3_use_mcc.npz')
    img1, img2 = mg.g3_pair()
    assert syn.sha256(img1, img2) == str(g['pair_sha'])
    v = [g[k] for k in ('c1', 'r1', 'c2fg', 'r2fg', 'border')]
    n_nan = 0
    for k, angles in enumerate(mg.G3_ANGLE_SETS):
        for mcc in ((0, 1) if k == 1 else (0,)):
            exp = g['out_s%d_k%d_m%d' % (s, k, mcc)]
            flags = 1 | (4 if mcc else 0)
            got_c, ij = c_oracle.pm_batch(img1, img2, *v, s, alpha0, angles, rot=rot_for(angles, alpha0, s),
                                          flags=flags, nthreads=4)
            np.testing.assert_array_equal(got_c, exp)              # bit-exact incl. NaN rows and h
            assert ((ij[:, 2] == -1) == np.isnan(exp[:, 0])).all()
            n_nan += int(np.isnan(exp[:, 0]).sum())
            if k == 0:                                             # NumPy form on the cheapest set
                got_n, _ = po.pm_batch(img1, img2, *v, s, alpha0, angles, flags=flags)
                np.testing.assert_array_equal(got_n, exp)
    assert n_nan > 0                                               # the zero-pixel NaN path is exercised


def test_g3_full_intermediates(c_oracle):
    g = load('g3_use_mcc.npz')
    img1, img2 = mg.g3_pair()
    angles, s, alpha0 = mg.G3_ANGLE_SETS[1], 34, 0.0
    for i in g['full_points']:
        res, (bij, bk, bres, btmpl) = po.use_mcc(g['c1'][i], g['r1'][i], g['c2fg'][i], g['r2fg'][i], g['border'][i],
                                                 img1, img2, s, alpha0, full=True, angles=angles)
        np.testing.assert_array_equal(bres, g['full%d_result' % i])
        np.testing.assert_array_equal(btmpl, g['full%d_template' % i])
        dc, dr, ba, br, bh = g['full%d_scalars' % i]
        assert (res[0] - g['c2fg'][i], res[1] - g['r2fg'][i], res[2], res[3], res[4]) == (dc, dr, ba, br, bh)
        np.testing.assert_array_equal(c_oracle.match_template(
            img2[int(g['r2fg'][i] - 17 - g['border'][i]):int(g['r2fg'][i] + 17 + g['border'][i] + 1),
                 int(g['c2fg'][i] - 17 - g['border'][i]):int(g['c2fg'][i] + 17 + g['border'][i] + 1)], btmpl), bres)


def test_reference_quirks_are_kept():
    """tc = int(s/2.)+1 biases the displacement by -1.5 px (s=34) / -1 px (s=35)."""
    rng = np.random.default_rng(1)
    img1 = rng.integers(1, 256, (300, 300), dtype=np.uint8)
    img2 = np.roll(np.roll(img1, 4, axis=0), -6, axis=1)          # shift +4 rows, -6 cols
    for s, (edr, edc) in ((35, (3.0, -7.0)), (34, (2.5, -7.5))):
        c2, r2, a, r, h = po.use_mcc(150.0, 150.0, 150.0, 150.0, 20.0, img1, img2, s, 0.0, angles=[0])
        assert (r2 - 150.0, c2 - 150.0) == (edr, edc)
        assert r == np.float32(1.0)


def test_out_of_image_window_is_nan(c_oracle):
    img1, img2 = syn.make_pair(200, 200, seed=2)
    out, ij = c_oracle.pm_batch(img1, img2, [100.0, 100.0], [100.0, 100.0], [30.0, 100.0], [100.0, 100.0],
                                [20.0, 20.0], 34, 0.0, [0.0])
    assert np.isnan(out[0]).all() and (ij[0] == -1).all() and np.isfinite(out[1]).all()
    exp, _ = po.pm_batch(img1, img2, [100.0, 100.0], [100.0, 100.0], [30.0, 100.0], [100.0, 100.0], [20.0, 20.0],
                         34, 0.0, [0.0])
    np.testing.assert_array_equal(out, exp)


# ---------------------------------------------------------------- G9 edges
@pytest.mark.parametrize('p', range(len(mg.G9_PAIRS)))
def test_g9_edges_numpy_and_c(c_oracle, p):
    """Fixture G9: the reference's use_mcc with search windows flush with / clipped by the edges of image 2 (NumPy slicing,
    pmlib.py:200-202) and templates flush with the edges of image 1, on odd-sized pairs of unequal shapes.  Both oracle forms
    reproduce it bit for bit, h included; where the reference raises, they return NaN (ij -1)."""
    g = load('g9_edges.npz')
    img1, img2 = mg.g9_pair(p)
    assert syn.sha256(img1, img2) == str(g['pair%d_sha' % p])
    assert img1.shape != img2.shape and all(n % 4 for n in img1.shape + img2.shape)
    for s, alpha0, order in mg.G9_VARIANTS:
        key = 'p%d_s%d_o%d' % (p, s, order)
        names, c1, r1, c2fg, r2fg, border, raises = mg.g9_points(img1, img2, s, alpha0, mg.G9_ANGLES, order)
        np.testing.assert_array_equal(names, g['names_' + key])                     # the points regenerate from the code
        np.testing.assert_array_equal(np.stack([c1, r1, c2fg, r2fg, border], axis=1), g['pts_' + key])
        exp = g['out_' + key]
        raised = [str(x).split(':')[0] for x in g['raised_' + key]]
        assert raised == list(names[raises]) and len(raised) == 8
        assert np.isnan(exp[raises]).all() and np.isfinite(exp[~raises, :4]).all()
        flags = 1 | (po.FLAG_ROT_ORDER1 if order else 0)
        got_c, ij = c_oracle.pm_batch(img1, img2, c1, r1, c2fg, r2fg, border, s, alpha0, mg.G9_ANGLES,
                                      rot=rot_for(mg.G9_ANGLES, alpha0, s), flags=flags, nthreads=4)
        np.testing.assert_array_equal(got_c, exp, err_msg=key)                       # bit-exact incl. NaN rows and h
        assert ((ij[:, 2] == -1) == raises).all()
        got_n, ij_n = po.pm_batch(img1, img2, c1, r1, c2fg, r2fg, border, s, alpha0, mg.G9_ANGLES, flags=flags)
        np.testing.assert_array_equal(got_n, exp, err_msg=key)
        np.testing.assert_array_equal(ij_n, ij)
        # the windows the fixture covers: clipped at the bottom / right, down to s + 1 rows / columns, flush
        hws = s // 2
        r0 = (r2fg - hws - border).astype(np.int64)
        r1e = np.minimum((r2fg + hws + border + 1).astype(np.int64), img2.shape[0])
        c1e = np.minimum((c2fg + hws + border + 1).astype(np.int64), img2.shape[1])
        ok = ~raises
        assert ((r2fg + hws + border + 1).astype(np.int64) > img2.shape[0])[ok].sum() >= 10
        assert ((c2fg + hws + border + 1).astype(np.int64) > img2.shape[1])[ok].sum() >= 10
        assert (((r1e - r0) == s + 1) & ok).any() and (r0[ok] == 0).any() and (r1e[ok] == img2.shape[0]).any()
        assert (c1e[ok] == img2.shape[1]).any()


def test_g5_fullsize_subsample_present():
    g = load('g5_fullsize.npz')
    assert g['out'].shape == (400, 5) and g['ij'].shape == (400, 3)
    assert np.isfinite(g['out']).all()


# ---------------------------------------------------------------- G3c large effective rotations
@pytest.mark.parametrize('s', [34, 35])
def test_g3c_large_rotations(c_oracle, s):
    """Fixture G3c: the reference's use_mcc with alpha0 of 30 / 90 / -137.5 degrees (pmlib.py:79-87,151: the template is sampled
    at angle - alpha0), rot_order 0 and 1 - the C oracle on every case, the NumPy oracle on the cheapest."""
    g = load('g3c_large_rotations.npz')
    g3 = load('g3_use_mcc.npz')
    img1, img2 = mg.g3_pair()
    assert syn.sha256(img1, img2) == str(g['pair_sha'])
    v = [g3[k] for k in ('c1', 'r1', 'c2fg', 'r2fg', 'border')]
    for ai, alpha0 in enumerate(mg.G3C_ALPHA0):
        for k, angles in enumerate(mg.G3C_ANGLE_SETS):
            for order in (0, 1):
                exp = g['out_s%d_a%d_k%d_o%d' % (s, ai, k, order)]
                flags = 1 | (8 if order else 0)
                got, ij = c_oracle.pm_batch(img1, img2, *v, s, alpha0, angles, rot=rot_for(angles, alpha0, s), flags=flags, nthreads=4)
                np.testing.assert_array_equal(got, exp)
                assert ((ij[:, 2] == -1) == np.isnan(exp[:, 0])).all()
                if k == 0 and ai == 2:
                    got_n, _ = po.pm_batch(img1, img2, *v, s, alpha0, angles, flags=flags)
                    np.testing.assert_array_equal(got_n, exp)


# ---------------------------------------------------------------- G1c / G3d rot_order 2..5 (scipy's spline interpolation)
@pytest.mark.parametrize('order', [2, 3, 4, 5])
def test_spline_restatement_is_scipys_own_arithmetic(c_oracle, order):
    """The prefilter against scipy.ndimage.spline_filter and the interpolation weights against scipy's own, read out through
    map_coordinates(prefilter=False) on impulse images - bit for bit, NumPy and C forms."""
    import math
    from scipy import ndimage as nd
    rng = np.random.default_rng(50 + order)
    for shape in ((2, 3), (5, 17), (64, 31), (300, 280)):
        img = rng.integers(0, 256, shape, dtype=np.uint8)
        ref = nd.spline_filter(img, order, output=np.float64, mode='constant')
        np.testing.assert_array_equal(po.spline_coefficients(img, order), ref)
        np.testing.assert_array_equal(c_oracle.spline_coefficients(img, order), ref)
    xs = np.concatenate([rng.uniform(8, 30, 500), [10.0, 10.5, 11.25]])
    w = po.spline_weights(xs, order)
    for x, wx in zip(xs, np.array(w).T):
        base = math.floor(x) - order // 2 if order & 1 else math.floor(x + 0.5) - order // 2
        for t in range(order + 1):
            imp = np.zeros(41)
            imp[base + t] = 1.0
            assert nd.map_coordinates(imp, [[x]], order=order, prefilter=False, mode='constant')[0] == wx[t]


@pytest.mark.parametrize('order', [2, 3, 4, 5])
def test_g1c_templates_spline_numpy_and_c(c_oracle, order):
    g = load('g1c_templates_spline.npz')
    for name, img in (('smooth', mg.g1c_image()), ('noise', mg.g1_image())):
        assert syn.sha256(img) == str(g['img_sha' if name == 'smooth' else 'noise_sha'])
        cf = po.spline_coefficients(img, order)
        for k, (c, r, a, s) in enumerate(mg.G1C_CASES):
            exp = g['%s_o%d_%d' % (name, order, k)]
            np.testing.assert_array_equal(po.get_template_spline(img, c, r, a, int(s), order, coeffs=cf), exp)
            np.testing.assert_array_equal(c_oracle.get_template(img, c, r, po.rotation_terms(a, int(s)), int(s), rot_order=order, coeffs=cf), exp)


@pytest.mark.parametrize('case', mg.G3D_CASES)
def test_g3d_use_mcc_spline(c_oracle, case):
    s, alpha0, order, k = case
    g = load('g3d_use_mcc_spline.npz')
    g3 = load('g3_use_mcc.npz')
    img1, img2 = mg.g3_pair()
    v = [g3[x] for x in ('c1', 'r1', 'c2fg', 'r2fg', 'border')]
    angles = mg.G3_ANGLE_SETS[k]
    exp = g['out_s%d_o%d_k%d' % (s, order, k)]
    got, ij = c_oracle.pm_batch(img1, img2, *v, s, alpha0, angles, rot=rot_for(angles, alpha0, s), flags=1 | po.flag_rot_order(order), nthreads=4)
    np.testing.assert_array_equal(got, exp)
    if k == 0 and order == 3:
        got_n, _ = po.pm_batch(img1, img2, *v, s, alpha0, angles, flags=1 | po.flag_rot_order(order))
        np.testing.assert_array_equal(got_n, exp)
