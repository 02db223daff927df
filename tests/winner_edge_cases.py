"""Inputs that drive the normalisation of the winner's NCC matrix (csrc/ncc_norm.h) to its edges, on 256 x 256 images, and the
shapes they are run at.

Cases (one point at the image centre; `check` asserts from the C oracle's answer what each is made for):
  shifted   image 2 = image 1 moved by (2, -1): the winner's matrix holds an exact 1.0f (q = 1 to within rounding: the
            neighbourhood of the clamp threshold, decided by the specification's route)
  inverted  image 2 = 255 - image 1, moved: an exact -1.0f.  Image 1 carries rows of period 4, so the inverted image matches
            two rows off and the unrotated template wins (the angles are 12 degrees apart); the matrix also holds values
            beyond neither threshold and the ordinary kind
  block     image 2 is constant over the top left corner of the search window: placements inside it have dI = 0 - the
            low-variance rule, 0.0f (the short route divides 0 by 0 there)
  const     image 1 is constant around the point: a constant template, the matrix is all ones
  textured  an ordinary synthetic pair

Two routes on the GPU (tests/test_gpu_winner_edges.py):
  debug_point  returns the whole matrix.  It does not ask the launch planner: whatever the border, it runs the run-time-pitch
               instantiation pm_kernel_rp<S, 4, paired, 0, false> (sums in global memory, no kept sum w': the winner multiplies
               the all-ones operand; rp_winner_kept at 3 / 7 angles), or the classic kernel at other sides.  Its shapes vary
               the matrix: single items only, pair + single, remainders.
  set_points / run / fetch  goes through the planner, so the border picks the launch class - compile-time pitches, sums in LDS
               or in global memory, the winner that reads the sweep's kept sum w', the 8-row band, the 128-register build -
               and SID_PM_ALWAYS_GS / SID_PM_NO_GS / SID_PM_NO_GSI (as in tests/test_gpu_parity.py) force the other forms.  It
               returns the peak, r and h: h is the Hessian of the whole matrix at the peak, normalised by the matrix's median and
               standard deviation, so a wrong or non-finite value anywhere in the matrix shows in it.
"""
import numpy as np

from sea_ice_drift_amd import pmlib as my
from sea_ice_drift_amd import synthetic as syn

SIZE = 256
C1 = R1 = 128.0
SHIFT = (2, -1)                                                       # rows, columns
CASES = ('shifted', 'inverted', 'block', 'const', 'textured')
ANGLES = {3: [-12.0, 0.0, 12.0], 7: [12.0 * k for k in range(-3, 4)], 15: [12.0 * k for k in range(-7, 8)]}

# debug_point: (side, border, number of angles) - borders 3 and 7: single items only; 9: a remainder of 20 columns; 20 and up:
# pair + single items; 7 and 3 angles: the slot-group kernels, whose winner is rp_winner_kept
ROW_PAIR_SHAPES = ([(s, b, 15) for s in (34, 35) for b in (3, 7, 9, 20, 24, 30, 40)] +
                   [(s, b, K) for s in (34, 35) for K in (7, 3) for b in (7, 20, 30)])
CLASSIC_SHAPES = [(s, b, 15) for s in (20, 33) for b in (3, 20)]
SHAPES = ROW_PAIR_SHAPES + CLASSIC_SHAPES

# set_points: the borders of one call (the planner sorts them into launch classes) - 3, 7: single items only; 9: rem 20; 20: the
# three-wavefront class (four workgroups per CU); 24: sums in LDS; 30: sums in global memory, pitch 136; 40: the 8-row band
PLAN_BORDERS = (3, 7, 9, 20, 24, 30, 40)
PLAN_SIDES = (34, 35)
PLAN_ANGLES = (15, 7, 3)
PLAN_SWITCHES = (None, 'SID_PM_ALWAYS_GS', 'SID_PM_NO_GS', 'SID_PM_NO_GSI')

_CACHE = {}


def _striped():
    """Image 1 of the shifted / inverted / block cases: rows of period 4 (128, 208, 128, 48) under a texture of +-24."""
    if 'striped' not in _CACHE:
        rng = np.random.default_rng(20261021)
        rows = np.array([128, 208, 128, 48])[np.arange(SIZE) % 4][:, None]
        img = (rows + rng.integers(-24, 25, (SIZE, SIZE))).astype(np.uint8)
        assert img.min() >= 1
        img.setflags(write=False)
        _CACHE['striped'] = img
    return _CACHE['striped']


def window_of(s, b):
    """(row0, col0, side) of the search window in image 2 (pmlib.py: hws = s // 2, first guess rounded down)."""
    hws = s // 2
    r2, c2 = int(R1) + SHIFT[0], int(C1) + SHIFT[1]
    return r2 - hws - b, c2 - hws - b, 2 * hws + 2 * b + 1


def images(case, s, b):
    """(image 1, image 2) of a case; only `block` depends on the shape (the block sits in the corner of its window)."""
    key = (case, s, b) if case == 'block' else case
    if key not in _CACHE:
        if case == 'textured':
            img1, img2 = syn.make_pair(SIZE, SIZE, seed=41, amplitude=0.0)
            img2 = np.roll(img2, SHIFT, axis=(0, 1))
        else:
            img1 = _striped()
            img2 = np.roll(img1, SHIFT, axis=(0, 1))
            if case == 'inverted':
                img2 = 255 - img2
            elif case == 'block':
                r0, c0, _ = window_of(s, b)
                img2 = img2.copy()
                img2[r0:r0 + s + 3, c0:c0 + s + 4] = 90                # 4 x 5 placements (rows x columns) lie inside
            elif case == 'const':
                img1 = img1.copy()
                img1[int(R1) - 60:int(R1) + 61, int(C1) - 60:int(C1) + 61] = 77
        img1, img2 = np.ascontiguousarray(img1), np.ascontiguousarray(img2)
        img1.setflags(write=False); img2.setflags(write=False)
        _CACHE[key] = (img1, img2)
    return _CACHE[key]


def point():
    """c1, r1, c2fg, r2fg of the one point."""
    return C1, R1, C1 + SHIFT[1], R1 + SHIFT[0]


def reference(c_oracle, case, s, b, K):
    """The C oracle's answer, computed once per (case, shape) and shared: dict(out [5], ij [3], ccm = the winning angle's NCC
    matrix, hes = its raw Hessian)."""
    key = ('ref', case, s, b, K)
    if key not in _CACHE:
        img1, img2 = images(case, s, b)
        angles = ANGLES[K]
        rot = my.rotation_table(angles, 0.0, s)
        c1, r1, c2, r2 = point()
        exp, exp_ij = c_oracle.pm_batch(img1, img2, [c1], [r1], [c2], [r2], [float(b)], s, 0.0, angles, rot=rot)
        assert exp_ij[0, 2] >= 0, 'the oracle refuses the point'
        r0, c0, w = window_of(s, b)
        tmpl = c_oracle.get_template(img1, c1, r1, rot[int(exp_ij[0, 2])], s)
        ccm = c_oracle.match_template(img2[r0:r0 + w, c0:c0 + w], tmpl)
        assert ccm[exp_ij[0, 0], exp_ij[0, 1]] == ccm.max() == np.float32(exp[0, 3])
        ref = dict(out=exp[0], ij=exp_ij[0], ccm=ccm, hes=c_oracle.hessian(ccm, flags=0))
        for v in ref.values():
            v.setflags(write=False)
        _CACHE[key] = ref
    return _CACHE[key]


def plan_sets(case, s):
    """[(image pair, borders)] of the set_points route: all borders in one call, but for `block`, whose image 2 belongs to one
    border - one call per border there."""
    if case == 'block':
        return [(images(case, s, b), (b,)) for b in PLAN_BORDERS]
    return [(images(case, s, 0), PLAN_BORDERS)]


def plan_vectors(borders):
    c1, r1, c2, r2 = point()
    n = len(borders)
    return [np.full(n, v) for v in (c1, r1, c2, r2)] + [np.asarray(borders, dtype=np.float64)]


def plan_reference(c_oracle, case, s, K, borders):
    """The oracle's (out [n, 5], ij [n, 3]) of one set_points call, computed once and shared."""
    key = ('plan', case, s, K, tuple(borders))
    if key not in _CACHE:
        img1, img2 = images(case, s, borders[0])
        angles = ANGLES[K]
        exp, exp_ij = c_oracle.pm_batch(img1, img2, *plan_vectors(borders), s, 0.0, angles, rot=my.rotation_table(angles, 0.0, s), nthreads=8)
        assert (exp_ij[:, 2] >= 0).all(), 'the oracle refuses a point'
        exp.setflags(write=False); exp_ij.setflags(write=False)
        _CACHE[key] = (exp, exp_ij)
    return _CACHE[key]


def check(case, s, b, K, ref):
    """What the case is made for, from the oracle's matrix alone."""
    ccm, ij = ref['ccm'], ref['ij']
    n = 2 * b + (2 if s % 2 == 0 else 1)
    assert ccm.shape == (n, n) and ccm.dtype == np.float32
    assert np.isfinite(ccm).all() and np.abs(ccm).max() <= 1.0
    mid = ANGLES[K].index(0.0)
    if case == 'shifted':
        assert ij[2] == mid and (ij[0], ij[1]) == (b - 1, b - 1)
        assert ccm[b - 1, b - 1] == np.float32(1.0) and (ccm == np.float32(1.0)).sum() == 1
    elif case == 'inverted':
        assert ij[2] == mid, 'the unrotated template must win for the matrix to hold the inverted match'
        assert ccm[b - 1, b - 1] == np.float32(-1.0) and (ccm == np.float32(-1.0)).sum() == 1
        assert 0.5 < ccm.max() < 1.0                                   # the rows realign two placements up or down
    elif case == 'block':
        assert (ccm[:4, :5] == 0.0).all() and not np.signbit(ccm[:4, :5]).any()
        assert (ccm == 0.0).sum() == 20                                # nowhere else
        assert ccm.max() > 0.2
    elif case == 'const':
        assert (ccm == np.float32(1.0)).all() and tuple(ij) == (0, 0, 0)
    else:
        assert 0.3 < ccm.max() < 1.0 and (np.abs(ccm) < 1.0).all() and (ccm != 0.0).all()
