"""Inputs shared by tests/test_fg_knn_host.py (device = -1) and tests/test_gpu_fg_knn.py (a GPU): the cases of sid_fg_knn and
the prelude scenario with planted wrong key points.  The specification's answer for a case is computed once per process
(``expected``) and never modified.  No tests in here."""
import numpy as np

from sea_ice_drift_amd import synthetic as syn
from sea_ice_drift_amd.domain import ArrayNansat
from tests import fg_knn_spec as spec

KS = (1, 2, 5, 16)

# integer offsets with an integer length (3-4-5 and its kin): d2 == m2 exactly for max_dist = that length
PYTHAGOREAN = np.array([[3.0, 4.0], [6.0, 8.0], [5.0, 12.0], [8.0, 15.0], [20.0, 21.0], [-3.0, 4.0], [9.0, 40.0]])   # 5, 10, 13, 17, 29, 5, 41


def _vals(rng, n):
    return np.stack([rng.normal(0, 30, n), rng.normal(0, 30, n)], axis=1)


def build():
    """name -> (seeds, values, q, k, max_dist)."""
    rng = np.random.default_rng(20)
    c = {}
    s7, q7 = rng.uniform(0, 100, (7, 2)), rng.uniform(-20, 120, (60, 2))
    v7 = _vals(rng, 7)
    s300, q300 = rng.uniform(0, 1000, (300, 2)), rng.uniform(0, 1000, (400, 2))
    v300 = _vals(rng, 300)
    for k in KS:
        c['seven_k%d' % k] = (s7, v7, q7, k, None)                        # k = 16 > n_seeds
        c['uniform300_k%d' % k] = (s300, v300, q300, k, None)
    # lattice seeds, lattice queries (on seeds and on cell centres): many exact ties
    gx, gy = np.meshgrid(np.arange(0.0, 18.0), np.arange(0.0, 17.0))
    lat = np.stack([gy.ravel(), gx.ravel()], axis=1)                      # 306 seeds
    qx, qy = np.meshgrid(np.arange(-1.0, 19.0, 0.5), np.arange(-1.0, 18.0, 0.5))
    c['lattice'] = (lat, _vals(rng, len(lat)), np.stack([qy.ravel(), qx.ravel()], axis=1), 5, None)
    c['lattice_k16_limit'] = (lat, _vals(rng, len(lat)), np.stack([qy.ravel(), qx.ravel()], axis=1), 16, 2.0)
    # every seed twice (other values), in two layouts: the copy right behind, and all copies at the end
    d = rng.uniform(0, 500, (150, 2))
    c['duplicates_adjacent'] = (np.repeat(d, 2, axis=0), _vals(rng, 300), rng.uniform(0, 500, (300, 2)), 5, None)
    c['duplicates_appended'] = (np.concatenate([d, d]), _vals(rng, 300), np.concatenate([d[:100], rng.uniform(0, 500, (200, 2))]), 2, None)
    # queries ON seeds, and far outside the seeds' box
    c['on_seeds'] = (s300, v300, s300[:120].copy(), 5, None)
    c['far_outside'] = (s300, v300, np.concatenate([rng.uniform(-1e5, 1e5, (200, 2)), [[-1e9, 3.0], [4.0, 1e12], [1e150, -1e150]]]), 5, None)
    # max_dist: queries at integer points, seeds at Pythagorean offsets from the first one (and far from the others)
    qs = np.array([[100.0, 100.0], [100.0, 101.0], [400.0, 400.0]])
    ps = qs[0] + PYTHAGOREAN
    vp = _vals(rng, len(ps))
    c['limit_m0'] = (ps, vp, qs, 5, 4.999)                                # nobody within reach
    c['limit_m1_on'] = (ps[:5], vp[:5], qs, 5, 5.0)                       # (3, 4) exactly on the limit: m = 1
    c['limit_m2_tie_on'] = (ps, vp, qs, 5, 5.0)                           # (3, 4) and (-3, 4): a tie ON the limit
    c['limit_m4_on'] = (ps[:5], vp[:5], qs, 5, 17.0)                      # m = k - 1 = 4, (8, 15) exactly on the limit
    c['limit_k1'] = (ps, vp, qs, 1, 5.0)
    # seeds, values and queries that are not finite
    sb, vb = rng.uniform(0, 200, (40, 2)), _vals(rng, 40)
    sb[3, 0] = np.nan; sb[7, 1] = np.inf; sb[11] = -np.inf; vb[0, 1] = np.nan; vb[5, 0] = np.inf; vb[39] = np.nan   # noqa: E702
    qb = rng.uniform(0, 200, (50, 2))
    qb[2, 0] = np.nan; qb[9, 1] = np.inf; qb[30] = (-np.inf, np.nan)     # noqa: E702
    c['non_finite'] = (sb, vb, qb, 5, None)
    c['non_finite_k16'] = (sb, vb, qb, 16, 60.0)
    c['all_unusable'] = (np.full((5, 2), np.nan), _vals(rng, 5), qb, 5, None)
    c['no_seeds'] = (np.empty((0, 2)), np.empty((0, 2)), q7, 5, None)
    return c


CASES = build()
_EXPECTED = {}


def expected(name):
    """(out, count, index, d2) of the specification for CASES[name]."""
    if name not in _EXPECTED:
        s, v, q, k, md = CASES[name]
        _EXPECTED[name] = spec.knn(s, v, q, k, md)
    return _EXPECTED[name]


def assert_equals_spec(got, exp):
    np.testing.assert_array_equal(got[1], exp[1])
    np.testing.assert_array_equal(got[2], exp[2])
    assert got[1].dtype == np.int32 and got[2].dtype == np.int32
    assert spec.same_bits(got[0], exp[0])


# ---- the prelude scenario: identity georeference, key points with planted outliers ----
SCENE = 3000
OUTLIER_SHARE = 0.02
BOUND = 17.0                       # px: min_border = 20 less the rounding of the first guess and of the grid point


def prelude_scenario(seed, n_kp=1800, outliers=OUTLIER_SHARE):
    """-> dict(n1, n2, c1, r1, c2, r2, lon, lat): 1 800 key points uniform on a 3000 x 3000 scene carrying the synthetic
    field's true displacement + N(0, 1) px, 2 % of them moved by +-(60 .. 150) px per component (wrong matches); a 40 x 40
    grid from 150 to 2850.  Key points of image 2 are kept inside the image (the prelude's nearest-key-point distance indexes
    the image with them, as the reference does)."""
    rng = np.random.default_rng(seed)
    img = np.zeros((SCENE, SCENE), dtype=np.uint8)
    n1, n2 = ArrayNansat(img), ArrayNansat(img)
    c1, r1 = rng.uniform(0, SCENE, n_kp), rng.uniform(0, SCENE, n_kp)
    dc, dr = syn.true_displacement(c1, r1)
    c2, r2 = c1 + dc + rng.normal(0, 1, n_kp), r1 + dr + rng.normal(0, 1, n_kp)
    bad = rng.choice(n_kp, int(round(outliers * n_kp)), replace=False)
    c2[bad] += rng.choice([-1.0, 1.0], len(bad)) * rng.uniform(60, 150, len(bad))
    r2[bad] += rng.choice([-1.0, 1.0], len(bad)) * rng.uniform(60, 150, len(bad))
    c2, r2 = np.clip(c2, 0, SCENE - 1), np.clip(r2, 0, SCENE - 1)
    lon, lat = np.meshgrid(np.linspace(150, 2850, 40), np.linspace(150, 2850, 40))
    return dict(n1=n1, n2=n2, c1=c1, r1=r1, c2=c2, r2=r2, lon=lon, lat=lat)


def prelude_error(pre):
    """Distance of every grid point's first guess from the true position, per component: (|dc|, |dr|)."""
    dc, dr = syn.true_displacement(pre['c2pm1i'], pre['r2pm1i'])
    return np.abs(pre['c2fg'] - (pre['c2pm1i'] + dc)), np.abs(pre['r2fg'] - (pre['r2pm1i'] + dr))


def run_prelude(sc, **kwargs):
    from sea_ice_drift_amd import pmlib
    return pmlib.pm_prelude(sc['lon'], sc['lat'], sc['n1'], sc['c1'], sc['r1'], sc['n2'], sc['c2'], sc['r2'], img_size=34, **kwargs)
