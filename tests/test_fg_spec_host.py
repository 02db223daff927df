"""CPU: the specification of the first-guess evaluation (tests/fg_spec.py) against SciPy, on the cases of tests/fg_cases.py and
on 20 random triangulations.  Every query the specification leaves unflagged has SciPy's hull membership and SciPy's rounded
value (what the reference computes next, pmlib.py:285-288); a query at the centroid of a simplex is located in that simplex; of
those strictly interior queries the specification flags none but the ones a case places at a half-integer.  Where the simplex is
SciPy's the bit-equal values are counted and printed (no share is asserted: SciPy's BLAS may round the 2 x 2 solve differently).
The nearest-distance specification equals the exact integer computation on integer seeds and queries."""
import numpy as np
import pytest
from scipy.interpolate import LinearNDInterpolator
from scipy.spatial import Delaunay

from tests import fg_cases as fc
from tests import fg_spec as spec


def check_against_scipy(c, res, label):
    out, sx, doubt, det = res
    tri = Delaunay(c['pts'])
    if c['scipy'] == 'same':
        np.testing.assert_array_equal(tri.simplices, c['simplices'])
    exp = LinearNDInterpolator(tri, c['values'])(c['q'])
    clear = ~doubt
    np.testing.assert_array_equal(np.isnan(out[clear]), np.isnan(exp[clear]))
    fin = clear & ~np.isnan(exp[:, 0])
    np.testing.assert_array_equal(np.round(out[fin]), np.round(exp[fin]))
    if c['scipy'] == 'same':
        same = fin & (sx == tri.find_simplex(c['q']))
        bits = (out[same] == exp[same]).all(axis=1)
        print('%s: %d unflagged and finite, %d in SciPy\'s simplex, %d of those bit-equal' % (label, fin.sum(), same.sum(), bits.sum()))
        for k in c['known']:
            assert same[k], k                                              # strictly interior: SciPy's simplex too


def check_interior(c, res):
    out, sx, doubt, det = res
    for k, s in c['known'].items():
        assert sx[k] == s, k
        assert bool(det['flagged'][k]) == (k in c['half']) and bool(doubt[k]) == (k in c['half']), k
    for k in c['half']:
        assert doubt[k] and (np.abs(out[k] - np.floor(out[k]) - 0.5) < 1e-6).any()


@pytest.mark.parametrize('name', sorted(fc.interp_cases()))
def test_case_against_scipy_and_its_own_claims(name):
    c = fc.interp_cases()[name]
    res = fc.expected(name)
    check_interior(c, res)
    if c['scipy']:
        check_against_scipy(c, res, name)


def test_twenty_random_triangulations():
    rng = np.random.default_rng(77)
    for k in range(20):
        n = int(rng.integers(50, 401))
        c = fc._triangulated(rng, rng.uniform(0, float(rng.choice([1.0, 300.0, 5000.0])), (n, 2)))
        res = spec.interp_linear(c['pts'], c['simplices'], c['values'], c['q'], details=True)
        check_interior(c, res)
        check_against_scipy(c, res, 'random %d (%d points)' % (k, n))


def test_claims_of_the_hand_made_cases():
    """What a case says about itself in words: a query that is not a number is in no simplex and unflagged; flat simplices
    are skipped, alone they leave every query outside; the half-integer vertex keeps its flag; the diagonal of the square
    belongs to both triangles and resolves to the lower one."""
    for name, c in fc.interp_cases().items():
        out, sx, doubt, det = fc.expected(name)
        nan_q = np.isnan(c['q']).any(axis=1)
        assert np.isnan(out[nan_q]).all() and (sx[nan_q] == -1).all() and not doubt[nan_q].any(), name
        assert not det['ok'][~np.isfinite(det['T']).all(axis=1)].any()
    out, sx, doubt, det = fc.expected('flat_simplices_only')
    assert np.isnan(out).all() and (sx == -1).all() and not doubt.any() and not det['ok'].any()
    out, sx, doubt, det = fc.expected('flat_simplices_inserted')
    lat = fc.expected('lattice_int_17x17')
    assert not det['ok'][0] and not det['ok'][257] and det['ok'].sum() == 512
    np.testing.assert_array_equal(out, lat[0])                            # the neighbours still answer, bit for bit
    np.testing.assert_array_equal(doubt, lat[2])
    for name in sorted(fc.interp_cases()):
        if name.startswith('triangle_'):
            out, sx, doubt, det = fc.expected(name)
            assert out[1, 0] == 7.5 and doubt[1] and sx[1] == 0
            assert (sx[:7] == 0).all() and (sx[7:16] == -1).all()          # vertices, midpoints, centroid: inside; 1e-12 outside an edge is outside
    out, sx, doubt, det = fc.expected('square_diagonal')
    assert det['flagged'][:43].all() and (sx[:43] == 0).all()
    for name in ('lattice_int_17x17_wide_box', 'scattered_300_wide_box'):  # the half-integer key points: in several simplices, still flagged
        out, sx, doubt, det = fc.expected(name)
        mc = det['mc'][:, -20:]
        assert doubt[-20:].all() and (np.abs(out[-20:, 0] % 1.0 - 0.5) < 1e-6).all() and ((mc >= -spec.EPS).sum(axis=0) >= 3).all()
    # the bucket entries a case names in numbers are those of the count: one triangle over the whole box lies in every cell
    # (it fits, 16384 <= 8 + 16384), two do not fit; a few hundred simplices over the whole box never fit, in a wide box they do
    for name, c in fc.interp_cases().items():
        entries, capacity = spec.bucket_entries(c['pts'], c['simplices'], fc.expected(name)[3]['ok'])
        if c['route'] is not None:
            assert c['route'].get('entries', entries) == entries and c['route'].get('capacity', capacity) == capacity, name
            assert c['route']['buckets'] == int(entries <= capacity), name
        assert (entries <= capacity) == (name.startswith('triangle_') or name.endswith('_wide_box') or name == 'flat_simplices_only'), name
    assert spec.bucket_entries(np.array([[0.0, 1.0], [0.0, 2.0], [0.0, 5.0]]), [[0, 1, 2]], [True]) is None


def test_nearest_distance_spec_is_the_exact_integer_computation():
    def exact(seeds, q):
        s, p = seeds.astype(np.int64), q.astype(np.int64)
        d2 = ((p[:, None, :] - s[None, :, :]) ** 2).sum(axis=2).min(axis=1)
        return np.sqrt(d2.astype(np.float64))
    seeds, q, _ = fc.dist_cases()['integer_seeds_on_borders']
    whole = (q == np.floor(q)).all(axis=1)
    assert whole.sum() > 100 and (seeds == np.floor(seeds)).all()
    np.testing.assert_array_equal(fc.expected_dist('integer_seeds_on_borders')[whole], exact(seeds, q[whole]))
    s = fc.image_seeds()
    for rows, cols in fc.IMAGE_SHAPES:
        r, c = np.divmod(np.arange(rows * cols), cols)
        np.testing.assert_array_equal(spec.distance_image(s, rows, cols).ravel(), exact(s, np.stack([r, c], axis=1)))
    for name, (seeds, q, _) in fc.dist_cases().items():                   # not finite: +inf, whatever the seeds
        bad = ~np.isfinite(q).all(axis=1)
        assert bad.sum() in (0, 9) and (fc.expected_dist(name)[bad] == np.inf).all(), name
    seeds, q, _ = fc.dist_cases()['seed_just_behind_a_side']             # the nearest seed is the one behind the side, by 1e-8
    d = fc.expected_dist('seed_just_behind_a_side')
    assert (np.abs(d - (0.25 + 1e-8)) < 1e-12).all() and (np.floor(seeds[-8::2]) != np.floor(q)).any(axis=1).all()
    assert (np.floor(seeds[-7::2]) == np.floor(q)).all()
    seeds, q, _ = fc.dist_cases()['outside_on_eight_sides']
    d = fc.expected_dist('outside_on_eight_sides')
    assert (d[16:56] == 0.0).all() and d[56] == 1.0                   # queries on seeds; the two equidistant seeds
