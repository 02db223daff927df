"""Case builders of tests/test_gpu_template_sides.py (the kernels) and tests/test_side_cases_cpu.py (the same inputs on the C
oracle alone): image pairs, points and angle sets for the classic one-workgroup-per-point kernel at run-time template sides
2 .. 64 and for NCC matrices of 2 .. 14 placements per axis.  Plain NumPy; nothing here touches a device.

What the inputs are made for is asserted from the oracle's answer (the `check_*` functions), so that a claim such as "this set
has winners in the second group of slots" is verified where there is no GPU, and again in front of every GPU comparison."""
import numpy as np
from scipy import ndimage as nd

from sea_ice_drift_amd import pmlib as my, synthetic as syn

SIZE = 400
SIDES = [s for s in range(2, 65) if s not in (34, 35)]                # 34 / 35 run the row-pair kernels
BOUNDARY_SIDES = (2, 3, 4, 5, 15, 16, 17, 18, 31, 32, 33, 47, 48, 49, 50, 63, 64)   # k-groups of 16 columns, every s & 3
ANGLES3 = [-3.0, 0.0, 3.0]                                            # paired slots
ANGLES7 = [float(a) for a in range(-3, 4)]
ANGLES9 = [float(a) for a in range(-4, 5)]                            # one group, unpaired
ANGLES15 = [float(a) for a in range(-7, 8)]
ANGLES17 = [float(a) for a in range(-8, 9)]                           # two groups (15 + 2)
ANGLES_ROLLED = [float(a) for a in range(30, 171, 10)] + [0.0, 5.0]   # group 1: rotations no template survives; 0 and 5 in group 2
SIDE_BORDERS = (0, 0, 1, 2, 3, 4, 7, 12, 20, 20)
ROLL = (2, -1)                                                        # rows, columns
ZERO_ROW = 5                                                          # the point of side_points whose template holds zero pixels
FRACTIONAL_ROW = 6                                                    # ... and the one with a fractional centre

HES_SHAPES = ((2, 2), (2, 9), (3, 3), (4, 5), (5, 4), (8, 8), (9, 2), (9, 9), (10, 3), (3, 40))
SMALL_BORDERS = (0, 1, 2, 3, 4, 6)
CONST_VALUE = 77

_CACHE = {}


def _cached(key, make):
    if key not in _CACHE:
        v = make()
        for a in (v if isinstance(v, tuple) else (v,)):
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _CACHE[key] = v
    return _CACHE[key]


def speckled_pair():
    """synthetic.make_pair(400, 400, seed=5); image 1 with a block of zero pixels in its top left corner (a template on it is
    a NaN row) and a block of one value in its bottom left corner (a constant template: the NCC matrix is all ones)."""
    def make():
        img1, img2 = syn.make_pair(SIZE, SIZE, seed=5)
        img1 = img1.copy()
        img1[0:80, 0:80] = 0
        img1[310:400, 0:90] = CONST_VALUE
        return img1, img2
    return _cached('speckled', make)


def rolled_pair():
    """Image 2 = image 1 rolled by ROLL, no speckle: at 0 degrees the match is perfect, so the large rotations of the first
    group of ANGLES_ROLLED lose and the winners sit in the later groups."""
    def make():
        img1, _ = syn.make_pair(SIZE, SIZE, seed=5)
        return img1, np.ascontiguousarray(np.roll(img1, ROLL, axis=(0, 1)))
    return _cached('rolled', make)


def _pts(c1, r1, c2, r2, b):
    return dict(c1=np.asarray(c1, dtype=np.float64), r1=np.asarray(r1, dtype=np.float64), c2fg=np.asarray(c2, dtype=np.float64),
                r2fg=np.asarray(r2, dtype=np.float64), border=np.asarray(b, dtype=np.float64))


def vectors(g):
    return [g[k] for k in ('c1', 'r1', 'c2fg', 'r2fg', 'border')]


def side_points(s):
    """Ten points on the speckled pair, borders SIDE_BORDERS, first guess = the rounded true displacement.  Row ZERO_ROW sits on
    the zero block of image 1; row FRACTIONAL_ROW has a fractional centre (the on-the-fly sampler instead of the table)."""
    rng = np.random.default_rng(5000 + s)
    n = len(SIDE_BORDERS)
    c1 = np.rint(rng.uniform(130, 270, n)); r1 = np.rint(rng.uniform(130, 270, n))
    dc, dr = syn.true_displacement(c1, r1)
    c2 = c1 + np.rint(dc); r2 = r1 + np.rint(dr)
    c1[ZERO_ROW], r1[ZERO_ROW] = 40.0, 40.0                           # (its window around (200, 200) is a valid one)
    c2[ZERO_ROW], r2[ZERO_ROW] = 200.0, 200.0
    c1[FRACTIONAL_ROW] += 0.3; r1[FRACTIONAL_ROW] -= 0.45
    return _pts(c1, r1, c2, r2, SIDE_BORDERS)


def rolled_points(s, borders=(1, 2, 3, 4, 7, 12, 20, 20), seed=0):
    """Points on the rolled pair with first guesses within one pixel of the roll."""
    rng = np.random.default_rng(6000 + s + seed)
    n = len(borders)
    c1 = np.rint(rng.uniform(130, 270, n)); r1 = np.rint(rng.uniform(130, 270, n))
    e = rng.integers(-1, 2, size=(2, n))
    return _pts(c1, r1, c1 + ROLL[1] + e[0], r1 + ROLL[0] + e[1], borders)


def count_angles(K):
    """K angles whose last entry is 0 degrees, the others large rotations (30 .. 170 degrees)."""
    return [float(a) for a in np.round(np.linspace(30.0, 170.0, K - 1), 3)] + [0.0]


def last_group_start(K, group=15):
    return group * ((K - 1) // group)


def small_matrix_points(s):
    """Four points per border of SMALL_BORDERS on the speckled pair, four more at border 1, and one point on the constant block
    of image 1 (border 2).
    A first guess that is e pixels off the true displacement puts the peak at placement border - 1 - e of an axis; the four
    guesses aim at (border, border) - inside the matrix where it has an interior -, at column 0, at the last row, and at that
    corner."""
    rng = np.random.default_rng(7000 + s)
    c1, r1, c2, r2, bb = [], [], [], [], []
    for b in SMALL_BORDERS + (1,):
        cc = np.rint(rng.uniform(130, 270, 4)); rr = np.rint(rng.uniform(130, 270, 4))
        dc, dr = syn.true_displacement(cc, rr)
        n = placements(s, b)
        ec = np.array([-1, b - 1, -1, b - 1]); er = np.array([-1, -1, b - n, b - n])
        if len(bb) >= 4 * len(SMALL_BORDERS):                          # border 1 once more, every guess aimed at the interior: the
            ec[:] = -1; er[:] = -1                                     # field moves a peak by a pixel, and one pixel is the whole interior
        c1 += list(cc); r1 += list(rr); c2 += list(cc + np.rint(dc) + ec); r2 += list(rr + np.rint(dr) + er); bb += [b] * 4
    c1.append(45.0); r1.append(355.0); c2.append(200.0); r2.append(200.0); bb.append(2)
    return _pts(c1, r1, c2, r2, bb)


TINY_SIDES = (2, 3, 4, 5)
MED_LIST = 256                                                        # kMedList of csrc/pm_kernel_base.h: keys the median ranks by brute force


def tiny_side_points(s):
    """Sides 2 .. 5 at borders 6 and 7: two points on the constant block of image 1 - an all-ones NCC matrix of 169 .. 256
    values, every one of them in the one bucket of the median's histogram, so the list of keys is as long as it gets without
    the radix select taking over - and four points on the speckle."""
    rng = np.random.default_rng(7500 + s)
    cc = np.rint(rng.uniform(130, 270, 4)); rr = np.rint(rng.uniform(130, 270, 4))
    dc, dr = syn.true_displacement(cc, rr)
    return _pts([45.0, 45.0] + list(cc), [355.0, 355.0] + list(rr), [200.0, 210.0] + list(cc + np.rint(dc)),
                [200.0, 190.0] + list(rr + np.rint(dr)), [6, 7, 6, 7, 6, 7])


def check_tiny_set(s, g, exp, exp_ij, flags):
    n = np.array([placements(s, b) for b in g['border']])
    assert (n[:2] ** 2 <= MED_LIST).all() and (n[:2] ** 2 > 160).all()     # one bucket, ranked from the list
    for k in (0, 1):                                                   # all ones: the first placement of the first angle
        assert tuple(exp_ij[k]) == (0, 0, 0)
        assert np.isnan(exp[k, 3]) if flags & 4 else exp[k, 3] == 1.0   # (1 - 1) / 0
        assert np.isnan(exp[k, 4]) if flags & 1 else exp[k, 4] == 0.0   # (0 - 0) / 0
    assert np.isfinite(exp[2:]).all()


EDGE_SIDES = (2, 3, 4, 5, 16, 20, 21, 34, 35, 48, 50, 64)
EDGE_BORDERS = (1, 2, 3)


def edge_points(s):
    """Windows at the top and left edge of image 2 that are one row or column short.  The start of a window is int(c2fg - hws -
    border), truncated toward zero (pmlib.py:201-202), so a first guess half a pixel inside that distance starts at 0 and loses
    a column: a matrix that is not square - 6 x 5 at an even side with border 2, whose interior is one column wide; a window of
    four columns, one dword, at sides 2 and 3 with border 1.  Per border: short in columns, in rows, in both, and flush with
    both edges at full size.  -> (points, expected (rows, columns) of every window)."""
    rng = np.random.default_rng(9500 + s)
    hws = s // 2
    c1, r1, c2, r2, bb, shape = [], [], [], [], [], []
    for b in EDGE_BORDERS:
        w = 2 * hws + 2 * b + 1
        near, flush = hws + b - 0.5, float(hws + b)
        for cc, rr, ww, wh in ((near, 150.0, w - 1, w), (160.0, near, w, w - 1), (near, near, w - 1, w - 1), (flush, flush, w, w)):
            c1.append(np.rint(rng.uniform(130, 270))); r1.append(np.rint(rng.uniform(130, 270)))
            c2.append(cc); r2.append(rr); bb.append(b); shape.append((wh, ww))
    return _pts(c1, r1, c2, r2, bb), np.array(shape)


def check_edge_set(s, g, shape, exp, exp_ij):
    """Every window is a valid one of the expected size: the oracle places the centre of the matrix at the first guess, so
    c2 = c2fg + ix - (ww - s) / 2 gives the width back, and r2 the height."""
    assert (exp_ij >= 0).all() and np.isfinite(exp[:, :4]).all()
    ww = s + 2 * (g['c2fg'] + exp_ij[:, 1] - exp[:, 0])
    wh = s + 2 * (g['r2fg'] + exp_ij[:, 0] - exp[:, 1])
    np.testing.assert_array_equal(np.stack([wh, ww], axis=1), shape)
    assert (shape.min(axis=1) >= s + 1).all()
    rh, rw = shape[:, 0] - s + 1, shape[:, 1] - s + 1
    assert ((rh - rw) == 1).any() and ((rw - rh) == 1).any()           # not square, either way
    if s % 2 == 0:
        assert ((rh == 6) & (rw == 5)).any()                           # an interior of one column and two rows
    if s in (2, 3):
        assert (shape[:, 1] == 4).any()                                # one dword per window row, more rows than that


def placements(s, b):
    """Placements per axis of a window of border b that lies inside image 2 (pmlib.py:200-202): 2 b + 2 for an even side,
    2 b + 1 for an odd one."""
    return 2 * (s // 2) + 2 * int(b) + 1 - s + 1


def handover_borders(classes, first=1):
    """From the launch classes of borders first, first + 1, ... (estimate_residency): the first and the last border of every
    run of equal class up to and including the first border of the large-window pipeline.  -> (borders, their classes)."""
    from sea_ice_drift_amd import _capi
    cls = [int(c) for c in classes]
    large = [k for k, c in enumerate(cls) if c & _capi.CLASS_LARGE]
    assert large and large[0] > 0, 'no hand-over in the range of borders'
    end = large[0]
    picked = []
    for k in range(end):
        if k == 0 or cls[k] != cls[k - 1] or k == end - 1 or cls[k + 1] != cls[k]:
            picked.append(k)
    picked.append(end)
    return [first + k for k in picked], [cls[k] for k in picked]


HANDOVER_SIDES = (20, 33, 48, 49, 64)
HANDOVER_SIZE = 700


def handover_pair():
    return _cached('handover', lambda: syn.make_pair(HANDOVER_SIZE, HANDOVER_SIZE, seed=9))


def handover_points(s, n_angles=15, flags=1):
    """Two points per hand-over border of side s (handover_borders of the library's own host arithmetic, nothing hard-coded).
    -> (points, class of every point)."""
    from sea_ice_drift_amd import _capi
    first = 1
    all_borders = np.arange(first, 301, dtype=np.float64)
    borders, cls = handover_borders(_capi.estimate_residency(all_borders, s, n_angles, flags), first)
    rng = np.random.default_rng(9000 + s)
    b = np.repeat(np.asarray(borders, dtype=np.float64), 2)
    assert s // 2 + b.max() + 1 + 12 <= HANDOVER_SIZE // 2 - 20       # every window lies inside image 2
    c1 = np.rint(rng.uniform(340, 360, b.size)); r1 = np.rint(rng.uniform(340, 360, b.size))
    dc, dr = syn.true_displacement(c1, r1)
    e = rng.integers(-2, 3, size=(2, b.size))
    return _pts(c1, r1, c1 + np.rint(dc) + e[0], r1 + np.rint(dr) + e[1], b), np.repeat(np.asarray(cls), 2)


def rot_of(angles, s, alpha0=0.0):
    return my.rotation_table(angles, alpha0, s)


def oracle_batch(c_oracle, pair, g, s, angles, flags=1, alpha0=0.0):
    exp, exp_ij = c_oracle.pm_batch(pair[0], pair[1], *vectors(g), s, alpha0, angles, rot=rot_of(angles, s, alpha0), flags=flags, nthreads=16)
    exp.setflags(write=False); exp_ij.setflags(write=False)
    return exp, exp_ij


# ---- what the inputs are made for, asserted from the oracle's answer ----

def check_side_set(s, exp, exp_ij):
    """side_points(s): odd sides - the border-0 windows have s columns, no placement pair: NaN rows; even sides - a 2 x 2
    matrix, whose Hessian is all zero: finite c2, r2, a, r and h = 0 / 0.  The zero-pixel row is NaN.  Everything else finite."""
    nan = np.isnan(exp)
    want = np.zeros_like(nan)
    b0 = np.flatnonzero(np.asarray(SIDE_BORDERS) == 0)
    assert ZERO_ROW not in b0 and FRACTIONAL_ROW not in b0
    if s & 1:
        want[b0, :] = True
    else:
        want[b0, 4] = True
    want[ZERO_ROW, :] = True
    np.testing.assert_array_equal(nan, want)
    np.testing.assert_array_equal((exp_ij < 0).all(axis=1), want.all(axis=1))
    assert np.isfinite(exp).all(axis=1).sum() >= 6
    assert np.isfinite(exp[FRACTIONAL_ROW]).all()


def check_rolled_set(exp, exp_ij, first=15, at_least=6):
    assert np.isfinite(exp).all()
    assert (exp_ij[:, 2] >= first).sum() >= at_least


def check_small_set(s, g, exp, exp_ij, flags):
    """small_matrix_points(s): the placement counts, a peak on the edge of a matrix and one off it, the constant template."""
    b = g['border'].astype(int)
    n = np.array([placements(s, x) for x in b])
    assert set(n % 2) == {s % 2}                                       # (the other parity is the other side of the family)
    valid = n >= 2
    np.testing.assert_array_equal(exp_ij[:, 2] >= 0, valid)           # no zero pixel: NaN rows are the windows without a placement pair
    iy, ix = exp_ij[:, 0], exp_ij[:, 1]
    edge = valid & ((iy == 0) | (ix == 0) | (iy == n - 1) | (ix == n - 1))
    inner = valid & ~edge
    assert edge[valid & (n > 2)].any() and inner.any()
    assert (n[inner] >= 3).all()
    for x in set(b[valid & (n >= 3)]):                                 # every matrix size with an interior has a peak in it and one on its edge
        assert inner[b == x].any() and edge[b == x].any(), 'border %d' % x
    k = len(b) - 1                                                     # the constant template: all ones, the first placement wins
    assert tuple(exp_ij[k]) == (0, 0, 0)
    if flags & 4:
        assert not np.isfinite(exp[k, 3])                              # (1 - 1) / 0
    else:
        assert exp[k, 3] == 1.0
    if flags & 1:
        assert not np.isfinite(exp[k, 4])                              # (0 - 0) / 0
    else:
        assert exp[k, 4] == 0.0
    two = valid & (n == 2)
    if two.any():                                                      # a 2 x 2 matrix: the Hessian is all zero
        assert (np.isnan(exp[two, 4]) if flags & 1 else exp[two, 4] == 0.0).all()
        assert np.isfinite(exp[two, :3]).all()


def assert_parity(got, got_ij, exp, exp_ij, mcc_norm=False):
    """The project's parity rule (test_gpu_parity.assert_parity, test_gpu_front_end._compare) over every row: peak row, column
    and angle index, c2, r2, a bit-exact; r bit-exact, within rtol = atol = 1e-5 when mcc_norm divides it by a float32 standard
    deviation; h within rtol = atol = 1e-5; NaN compared as NaN value by value (a finite row with a NaN h must be exactly that),
    an infinity as that infinity."""
    assert got.shape == exp.shape and got_ij.shape == exp_ij.shape
    np.testing.assert_array_equal(got_ij, exp_ij)
    np.testing.assert_array_equal(np.isnan(got), np.isnan(exp))
    np.testing.assert_array_equal(got[:, :3], exp[:, :3])
    if mcc_norm:
        np.testing.assert_allclose(got[:, 3], exp[:, 3], rtol=1e-5, atol=1e-5, equal_nan=True)
    else:
        np.testing.assert_array_equal(got[:, 3], exp[:, 3])
    np.testing.assert_allclose(got[:, 4], exp[:, 4], rtol=1e-5, atol=1e-5, equal_nan=True)


# ---- the Hessian in NumPy / SciPy ----

def hessian_matrix(shape, seed=0):
    """A seeded float32 matrix with the range of an NCC matrix."""
    rng = np.random.default_rng(8000 + 100 * shape[0] + shape[1] + seed)
    return rng.uniform(-0.3, 1.0, shape).astype(np.float32)


def numpy_hessian(m, flags):
    """get_hessian in NumPy / SciPy (flags bit 0 = hes_norm, bit 1 = hes_smth): a sigma-1 Gaussian, the second differences along
    each axis by np.gradient applied twice, their magnitude, then (h - median) / std."""
    m = np.asarray(m, dtype=np.float32)
    if flags & 2:
        m = nd.gaussian_filter(m, 1)
    d2y = np.gradient(np.gradient(m, axis=0), axis=0)
    d2x = np.gradient(np.gradient(m, axis=1), axis=1)
    h = np.hypot(d2x, d2y)
    assert h.dtype == np.float32
    if flags & 1:
        with np.errstate(invalid='ignore', divide='ignore'):
            h = (h - np.median(h)) / np.std(h)
    return h
