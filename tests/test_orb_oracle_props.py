"""The detector's oracle (oracle/orb_oracle.py) against plain restatements of include/sid_orb.h that share neither code nor
formulation with it: the kernels are pinned to the oracle bit for bit (tests/test_orb.py, tests/test_gpu_orb_edges.py), and
the oracle was written beside them - FAST as a maximum over arcs of a minimum, the same shifts - so a shared misreading of the
header would pass there.  Here FAST is a run count over the ring, NMS a double loop, Harris and the blur SciPy correlations,
the resize a float64 bilinear evaluation, the orientation an arctangent, the descriptor a loop over its 256 bits.  CPU only."""
import math

import numpy as np
import pytest
from scipy import ndimage

from oracle import orb_oracle as oo
from sea_ice_drift_amd import orb, synthetic as syn

# the Bresenham circle of radius 3, clockwise from the top (image coordinates, y down), written out on its own
CIRCLE = ((0, -3), (1, -3), (2, -2), (3, -1), (3, 0), (3, 1), (2, 2), (1, 3),
          (0, 3), (-1, 3), (-2, 2), (-3, 1), (-3, 0), (-3, -1), (-2, -2), (-1, -3))


@pytest.fixture(scope='module')
def images():
    noise = np.random.default_rng(2024).integers(0, 256, (80, 90)).astype(np.uint8)
    synth = np.ascontiguousarray(syn.make_pair(300, 280, seed=5)[0][100:180, 60:150])
    for im in (noise, synth):
        im.setflags(write=False)
    return {'noise': noise, 'synth': synth}


def is_corner(img, y, x, t):
    """FAST-9 as the header words it: 9 contiguous ring pixels all brighter than centre + t or all darker than centre - t."""
    c = int(img[y, x])
    run_b = run_d = 0
    for k in range(16 + 8):                                            # once round and 8 more: every run that wraps
        v = int(img[y + CIRCLE[k % 16][1], x + CIRCLE[k % 16][0]])
        run_b = run_b + 1 if v > c + t else 0
        run_d = run_d + 1 if v < c - t else 0
        if run_b >= 9 or run_d >= 9:
            return True
    return False


@pytest.mark.parametrize('name,edge,t', [('noise', 16, 20), ('noise', 34, 40), ('synth', 16, 5), ('synth', 16, 1)])
def test_fast_score_is_the_threshold_at_which_the_corner_property_ends(images, name, edge, t):
    img = images[name]
    rows, cols = img.shape
    score = oo.fast_score(img, edge, t)
    assert score.shape == img.shape
    inner = np.zeros(img.shape, dtype=bool)
    inner[edge:rows - edge, edge:cols - edge] = True
    assert not score[~inner].any()                                     # nothing closer than `edge` to a border scores
    assert (score[inner] > 0).sum() >= 5 and (score[inner] == 0).sum() >= 5, 'both kinds of pixel are wanted'
    for y in range(edge, rows - edge):
        for x in range(edge, cols - edge):
            s = int(score[y, x])
            if s:
                assert s > t
                assert is_corner(img, y, x, s - 1) and not is_corner(img, y, x, s), (y, x, s)
            else:
                assert not is_corner(img, y, x, t), (y, x)


@pytest.mark.parametrize('name,edge,t', [('noise', 16, 20), ('synth', 16, 5), ('noise', 34, 20)])
def test_candidates_are_the_strict_3x3_maxima_with_their_harris_response(images, name, edge, t):
    img = images[name]
    rows, cols = img.shape
    score = oo.fast_score(img, edge, t)
    xs, ys, resp = oo.candidates(img, score, edge)
    exp = []
    for y in range(edge, rows - edge):
        for x in range(edge, cols - edge):
            v = score[y, x]
            if v > 0 and all(v > score[y + dy, x + dx] for dy in (-1, 0, 1) for dx in (-1, 0, 1) if dx or dy):
                exp.append((y, x))
    assert len(exp) >= 3
    assert sorted(zip(ys.tolist(), xs.tolist())) == exp                # every maximum is a candidate and nothing else is
    assert len(set(zip(ys.tolist(), xs.tolist()))) == len(xs)
    # Harris: central differences, 7x7 box sums, 25 (ab - c^2) - (a + b)^2 (k = 0.04 times 25), all int64
    I = img.astype(np.int64)
    ix = ndimage.correlate(I, np.array([[-1, 0, 1]], dtype=np.int64), mode='constant')
    iy = ndimage.correlate(I, np.array([[-1], [0], [1]], dtype=np.int64), mode='constant')
    box = np.ones((7, 7), dtype=np.int64)
    a = ndimage.correlate(ix * ix, box, mode='constant')
    b = ndimage.correlate(iy * iy, box, mode='constant')
    c = ndimage.correlate(ix * iy, box, mode='constant')
    harris = 25 * (a * b - c * c) - (a + b) * (a + b)
    assert harris.dtype == np.int64
    np.testing.assert_array_equal(resp, harris[ys, xs])


def binomial_blur(img):
    v = ndimage.correlate1d(img.astype(np.int64), [1, 4, 6, 4, 1], axis=0, mode='nearest')
    v = ndimage.correlate1d(v, [1, 4, 6, 4, 1], axis=1, mode='nearest')
    return (v + 128) >> 8


@pytest.mark.parametrize('name', ['noise', 'synth'])
def test_blur_is_the_separable_binomial_with_replicated_borders(images, name):
    got = oo.blur(images[name])
    assert got.dtype == np.uint8
    np.testing.assert_array_equal(got, binomial_blur(images[name]))


def test_blur_of_a_tiny_image():
    img = np.array([[0, 255, 3], [9, 1, 200]], dtype=np.uint8)         # every tap but the centre is a replicated border somewhere
    np.testing.assert_array_equal(oo.blur(img), binomial_blur(img))


def test_resize_identity_constant_and_ramp(images):
    for name in ('noise', 'synth'):
        np.testing.assert_array_equal(oo.resize(images[name], 80, 90), images[name])
    _, lr, lc, _ = oo.level_geometry(80, 90, 8, 1.2, 100)
    sizes = list(zip(lr, lc)) + [(40, 45), (37, 90), (80, 41), (1, 1)]
    const = np.full((80, 90), 173, dtype=np.uint8)
    slope, offset = 2, 10
    ramp = np.broadcast_to((slope * np.arange(90) + offset).astype(np.uint8), (80, 90))
    for r, c in sizes:
        assert (oo.resize(const, r, c) == 173).all() and oo.resize(const, r, c).shape == (r, c)
        got = oo.resize(ramp, r, c).astype(np.float64)
        # float64 bilinear at the pixel-centre mapping; on a ramp the interpolant between two columns IS the ramp, and rows
        # do not matter.  Source coordinates are clamped to the image like the header's "16.16 fixed-point source coordinates".
        fx = np.clip((np.arange(c) + 0.5) * 90 / c - 0.5, 0.0, 89.0)
        exp = np.broadcast_to(slope * fx + offset, (r, c))
        # Bound: 1 grey level.  The fixed-point column differs from fx by the truncated 16.16 step (< 2^-16 per column, < c 2^-16
        # in all), the half step's truncation (2^-16) and the 8-bit weight's truncation (< 2^-8): < 2^-8 + (c + 1) 2^-16 < 0.0053
        # pixels for c <= 90, i.e. < 0.011 grey levels at 2 grey levels per pixel; the one rounding to uint8 adds at most 0.5.
        # 0.511 < 1, and 1 is the smallest bound in whole grey levels that the 8-bit weights can promise on any image (a step
        # of 255 between two columns times 2^-8 is already 0.996).
        assert np.abs(got - exp).max() <= 1.0, (r, c)
        assert (np.diff(got, axis=1) >= 0).all()                       # and it stays monotone


def moments(lvl, x, y, R):
    m10 = m01 = 0
    for dy in range(-R, R + 1):
        for dx in range(-R, R + 1):
            if dx * dx + dy * dy <= R * R:
                v = int(lvl[y + dy, x + dx])
                m10 += dx * v
                m01 += dy * v
    return m10, m01


def direction_margin():
    """How far past half a bin the quantised direction may lie.  The direction is the b that maximises m . d_b with
    d_b = round(2^14 u_b) = 2^14 u_b + e_b, u_b the unit vector of bin b and |e_b| <= E (E measured from the table below;
    it cannot exceed sqrt(2) / 2).  With |m| = M and delta the angle between m and bin b, m . d_b lies within M E of
    2^14 M cos(delta).  If the winner b is not the nearest bin b*, then cos(delta*) - cos(delta) <= 2 E / 2^14.  m lies
    between the two bins, so delta + delta* >= pi / 16 (equality for neighbours), and cos(delta*) - cos(delta) =
    2 sin((delta + delta*) / 2) sin((delta - delta*) / 2) >= 2 sin(pi / 32) sin((delta - delta*) / 2), hence
    (delta - delta*) / 2 <= asin(E / (2^14 sin(pi / 32))).  The winner's excess over half a bin is delta - pi / 32 <=
    (delta - delta*) / 2, because delta* >= pi / 16 - delta."""
    d = orb.direction_table().astype(np.float64)
    th = 2.0 * np.pi * np.arange(32) / 32
    E = np.hypot(d[:, 0] - 16384.0 * np.cos(th), d[:, 1] - 16384.0 * np.sin(th)).max()
    assert E <= math.sqrt(0.5)
    return math.asin(E / (16384.0 * math.sin(math.pi / 32)))


@pytest.mark.parametrize('name,kw', [('noise', dict(edge_threshold=20, patch_size=31, n_levels=2, n_features=60)),
                                     ('synth', dict(edge_threshold=16, patch_size=24, n_levels=2, n_features=60, fast_threshold=5))])
def test_direction_is_the_nearest_of_32_and_descriptor_bits_sit_least_significant_first(images, name, kw):
    img = images[name]
    pattern, dirs = orb.rotated_pattern(), orb.direction_table()
    xy, meta, resp, desc = oo.detect_and_compute(img, pattern, dirs, **kw)
    assert len(xy) >= 10 and desc.shape == (len(xy), 32) and desc.dtype == np.uint8
    assert set(meta[:, 2].tolist()) == {0, 1}, 'both levels are wanted'
    sc, lr, lc, _ = oo.level_geometry(80, 90, kw['n_levels'], 1.2, kw['n_features'])
    margin = direction_margin()
    assert 0 < margin < 1e-3
    R = kw['patch_size'] // 2
    for (x, y, l, b), d, p in zip(meta.tolist(), desc, xy):
        lvl = img if l == 0 else oo.resize(img, lr[l], lc[l])
        assert p[0] == np.float32(x * sc[l]) and p[1] == np.float32(y * sc[l])
        m10, m01 = moments(lvl, x, y, R)
        assert m10 or m01
        assert 0 <= b < 32
        off = (math.atan2(m01, m10) - 2.0 * math.pi * b / 32 + math.pi) % (2.0 * math.pi) - math.pi
        assert abs(off) <= math.pi / 32 + margin, (x, y, l, b, m10, m01)
        bl = binomial_blur(lvl)
        for k in range(256):
            ax, ay, bx, by = (int(v) for v in pattern[b, k])
            bit = 1 if bl[y + ay, x + ax] < bl[y + by, x + bx] else 0
            assert (int(d[k // 8]) >> (k % 8)) & 1 == bit, (x, y, l, k)


def test_a_patch_without_a_centroid_gets_direction_0():
    """One bright pixel on a flat image: a corner whose disc is flat but for its own centre, m10 = m01 = 0, every dot product
    with the direction table is 0 and the first maximum is direction 0."""
    img = np.full((80, 90), 10, dtype=np.uint8)
    img[40, 45] = 250
    xy, meta, resp, desc = oo.detect_and_compute(img, orb.rotated_pattern(), orb.direction_table(), n_levels=1, n_features=10,
                                                 edge_threshold=20, patch_size=34)
    assert meta.tolist() == [[45, 40, 0, 0]]
    assert moments(img, 45, 40, 17) == (0, 0)


@pytest.mark.parametrize('scale', [1.05, 1.2, 2.0])
def test_level_shares_sum_to_n_features(scale):
    for n_levels in range(1, 17):
        for nf in (0, 1, 2, 3, 10, 100, 500, 1000, 2000, 3000, 5000, 100000):
            sc, lr, lc, want = oo.level_geometry(1000, 800, n_levels, scale, nf)
            assert len(sc) == len(lr) == len(lc) == len(want) == n_levels
            assert all(w >= 0 for w in want), (n_levels, nf, want)
            assert sum(want) == nf, (n_levels, nf, want)
            assert lr[0] == 1000 and lc[0] == 800 and sc[0] == 1.0
            s32 = float(np.float32(scale))
            for l in range(n_levels):
                assert sc[l] == pytest.approx(s32 ** l, rel=1e-14)
                assert abs(lr[l] - 1000 / s32 ** l) <= 0.5 + 1e-9 and abs(lc[l] - 800 / s32 ** l) <= 0.5 + 1e-9
