"""The triangulation-free first guess on the GPU (include/sid_fg.h sid_fg_knn): the kernels against the
NumPy specification tests/fg_knn_spec.py bit for bit - values, counts and neighbour indices - on both paths (every seed
through LDS; the ring walk over the buckets), and ``method='knn'`` through the prelude and pattern_matching."""
import numpy as np
import pytest

from sea_ice_drift_amd import _capi, pmlib as my, synthetic as syn
from sea_ice_drift_amd.domain import ArrayNansat
from tests import fg_knn_cases as cases
from tests import fg_knn_spec as spec

pytestmark = pytest.mark.gpu


def _check(s, v, q, k, md=None):
    got = _capi.fg_knn(s, v, q, k=k, max_dist=md, details=True)
    exp = spec.check(got, s, v, q, k, md)
    assert spec.same_bits(_capi.fg_knn(s, v, q, k=k, max_dist=md), exp[0])   # (count and index not asked for)
    return got, exp


@pytest.mark.parametrize('name', sorted(cases.CASES))
def test_device_equals_the_specification(name):
    """The cases of the host test (fewer than 256 usable seeds: every seed through LDS; the 300 uniform seeds, the lattice
    and the duplicates: the buckets)."""
    s, v, q, k, md = cases.CASES[name]
    got = _capi.fg_knn(s, v, q, k=k, max_dist=md, details=True)
    cases.assert_equals_spec(got, cases.expected(name))
    assert spec.same_bits(_capi.fg_knn(s, v, q, k=k, max_dist=md), got[0])


def test_clustered_seeds_long_ring_walks():
    """4 000 seeds clustered in a corner plus 40 scattered ones, queries over the whole box and beyond: most cells are empty,
    the walks are long, and with a limit most of them end on it.  k at every capacity of the register list and next to it."""
    rng = np.random.default_rng(31)
    s = np.concatenate([np.floor(rng.normal(400, 60, (4000, 2))), np.floor(rng.uniform(0, 10000, (40, 2)))])
    v = np.stack([rng.normal(0, 30, len(s)), rng.normal(0, 30, len(s))], axis=1)
    q = np.concatenate([np.floor(rng.uniform(-500, 10500, (1200, 2))), rng.uniform(200, 600, (300, 2)), s[:100]])
    for k, md in ((1, None), (4, None), (5, None), (8, None), (9, None), (16, None), (5, 700.0), (16, 25.0)):
        got, exp = _check(s, v, q, k, md)
        if md is None:
            assert (got[1] == k).all()
        else:
            assert (got[1] == 0).any() and (got[1] == k).any()
    assert (np.diff(exp[3], axis=1) == 0).any()                            # integer seeds: ties


def test_degenerate_box_and_the_path_switch():
    """Seeds on one line (a box without area: every seed through LDS - 1 024 of them fill one tile exactly, 1 500 leave a
    remainder), and 255 / 256 / 257 usable seeds - the switch between the two kernels - with and without unusable ones among
    them."""
    rng = np.random.default_rng(32)
    for n in (1024, 1500):
        s = np.stack([np.arange(float(n)), np.full(n, 77.0)], axis=1)
        _check(s, rng.normal(0, 9, (n, 2)), np.floor(rng.uniform(-50, n + 50, (700, 2))), 5)
    q = rng.uniform(-100, 1100, (600, 2))
    for n in (255, 256, 257):
        s, v = rng.uniform(0, 1000, (n, 2)), rng.normal(0, 9, (n, 2))
        _check(s, v, q, 5)
        s2, v2 = np.concatenate([s, rng.uniform(0, 1000, (30, 2))]), np.concatenate([v, rng.normal(0, 9, (30, 2))])
        s2[n:n + 10, 0] = np.nan
        v2[n + 10:, 1] = np.inf                                            # n usable of n + 30
        perm = rng.permutation(n + 30)
        got, _ = _check(s2[perm], v2[perm], q, 5, 400.0)
        assert not np.isin(got[2], np.flatnonzero(perm >= n)).any()


def test_unusable_seeds_never_take_part():
    """300 seeds of which 60 are unusable (240 left: every seed through LDS) and 400 of which 60 are (340: the buckets, whose
    box comes from the usable seeds alone - the unusable ones lie far outside it, or are NaN)."""
    rng = np.random.default_rng(33)
    q = np.concatenate([rng.uniform(-100, 1100, (500, 2)), [[5000.0, 5000.0]]])
    for n in (300, 400):
        s, v = rng.uniform(0, 1000, (n, 2)), rng.normal(0, 9, (n, 2))
        bad = rng.choice(n, 60, replace=False)
        s[bad[:15], 0] = np.nan
        s[bad[15:30], 1] = np.inf
        v[bad[30:45], 0] = -np.inf
        v[bad[45:], 1] = np.nan
        s[bad[45:]] = 5000.0                                               # finite coordinates, no value: ON a query
        for k in (1, 5, 16):
            got, _ = _check(s, v, q, k)
            assert not np.isin(got[2], bad).any() and (got[1] == k).all()


def test_buckets_equal_every_seed(monkeypatch):
    """The ring walk against the kernel that looks at every seed (SID_FG_NO_GRID=1), at a size where the specification in
    NumPy would take too long for a test: 20 000 integer seeds, 30 000 queries inside, outside and ON seeds."""
    rng = np.random.default_rng(34)
    s = np.floor(rng.uniform(2000, 2600, (20000, 2)))
    v = rng.normal(0, 30, (20000, 2))
    q = np.concatenate([s[:5000], np.floor(rng.uniform(0, 10000, (20000, 2))), rng.uniform(1900, 2700, (5000, 2))])
    for k, md in ((5, None), (16, 9.0), (1, None)):
        monkeypatch.delenv('SID_FG_NO_GRID', raising=False)
        got = _capi.fg_knn(s, v, q, k=k, max_dist=md, details=True)
        monkeypatch.setenv('SID_FG_NO_GRID', '1')
        exp = _capi.fg_knn(s, v, q, k=k, max_dist=md, details=True)
        monkeypatch.delenv('SID_FG_NO_GRID')
        np.testing.assert_array_equal(got[1], exp[1])
        np.testing.assert_array_equal(got[2], exp[2])
        assert spec.same_bits(got[0], exp[0])
    sub = rng.choice(len(q), 300, replace=False)                           # ... and a sample of it against the specification
    cases.assert_equals_spec(tuple(a[sub] for a in got), spec.knn(s, v, q[sub], 1, None))


def test_one_pool_large_small_large():
    """The grow-only scratch block serves calls of any size in any order, the other entry points of sid_fg.h in between."""
    rng = np.random.default_rng(35)
    big = (rng.uniform(0, 5000, (6000, 2)), rng.normal(0, 9, (6000, 2)), rng.uniform(0, 5000, (1500, 2)))
    small = (rng.uniform(0, 50, (9, 2)), rng.normal(0, 9, (9, 2)), rng.uniform(0, 50, (20, 2)))
    exp_big, exp_small = spec.knn(*big, 5), spec.knn(*small, 5)
    _capi.release_workspaces()
    for args, exp in ((big, exp_big), (small, exp_small), (big, exp_big)):
        cases.assert_equals_spec(_capi.fg_knn(*args, k=5, details=True), exp)
        d = _capi.fg_nearest_dist(args[0], args[2])
        np.testing.assert_array_equal(d, np.sqrt(exp[3][:, 0]))           # (the same squared distance, the same buckets)
    _capi.release_workspaces()
    cases.assert_equals_spec(_capi.fg_knn(*small, k=5, details=True), exp_small)


@pytest.mark.parametrize('old_border', [True, False])
def test_prelude_on_the_device_equals_the_host_instance(old_border):
    sc = cases.prelude_scenario(1)
    for extra in ({}, dict(knn_k=3, knn_max_dist=60.0)):
        dev = cases.run_prelude(sc, method='knn', first_guess_on='device', old_border=old_border, **extra)
        host = cases.run_prelude(sc, method='knn', first_guess_on='host', old_border=old_border, **extra)
        for key in ('c2fg', 'r2fg', 'brd2', 'gpi'):
            np.testing.assert_array_equal(dev[key], host[key])
    ec, er = cases.prelude_error(cases.run_prelude(sc, method='knn', first_guess_on='device', old_border=old_border))
    assert (np.hypot(ec, er) <= cases.BOUND).all()


def _hits(n1, n2, grid, c1, r1, c2, r2, **kwargs):
    """Grid points whose drift is within 1.5 px of the true displacement in both components."""
    out = my.pattern_matching(grid[0], grid[1], n1, c1, r1, n2, c2, r2, img_size=34, **kwargs)
    dc, dr = syn.true_displacement(grid[0], grid[1])
    with np.errstate(invalid='ignore'):
        return int(((np.abs(out[5] - grid[0] - dc) <= 1.5) & (np.abs(out[6] - grid[1] - dr) <= 1.5)).sum())


def test_pattern_matching_end_to_end():
    """pattern_matching with method='knn' against the default on the same inputs - a 900 x 900 synthetic pair, a 12 x 12 grid,
    400 key points carrying the true displacement + N(0, 1) px: the number of grid points whose drift is within 1.5 px of the
    truth is not below the linear route's, with clean key points and with 2 % of them wrong by 60 - 150 px.
    Measured on an MI355X (knn / linear of 144): clean 45 / 45, with the wrong key points 45 / 44."""
    img1, img2 = syn.make_pair(900, 900, seed=11)
    n1, n2 = ArrayNansat(img1), ArrayNansat(img2)
    g = np.rint(np.linspace(120, 780, 12))
    grid = np.meshgrid(g, g)
    rng = np.random.default_rng(36)
    c1, r1 = rng.uniform(0, 900, 400), rng.uniform(0, 900, 400)
    dc, dr = syn.true_displacement(c1, r1)
    c2, r2 = np.clip(c1 + dc + rng.normal(0, 1, 400), 0, 899), np.clip(r1 + dr + rng.normal(0, 1, 400), 0, 899)   # (inside image 2)
    clean = (_hits(n1, n2, grid, c1, r1, c2, r2, method='knn'), _hits(n1, n2, grid, c1, r1, c2, r2))
    # the sharded path runs the same prelude once and hands the keywords through: two handles, the same seven grids
    one = my.pattern_matching(grid[0], grid[1], n1, c1, r1, n2, c2, r2, img_size=34, method='knn', knn_k=3)
    two = my.pattern_matching(grid[0], grid[1], n1, c1, r1, n2, c2, r2, img_size=34, method='knn', knn_k=3, devices=[0, 0])
    for a, b in zip(one, two):
        assert spec.same_bits(a, b)
    bad = rng.choice(400, 8, replace=False)
    c2b, r2b = c2.copy(), r2.copy()
    c2b[bad] += rng.choice([-1.0, 1.0], 8) * rng.uniform(60, 150, 8)
    r2b[bad] += rng.choice([-1.0, 1.0], 8) * rng.uniform(60, 150, 8)
    c2b, r2b = np.clip(c2b, 0, 899), np.clip(r2b, 0, 899)
    planted = (_hits(n1, n2, grid, c1, r1, c2b, r2b, method='knn'), _hits(n1, n2, grid, c1, r1, c2b, r2b))
    print('hits of 144, knn / linear: clean %d / %d, 2 %% wrong key points %d / %d' % (clean + planted))
    assert clean[0] >= clean[1]
    assert planted[0] >= planted[1]
    assert clean[1] > 0                                                    # (the yardstick measures something)
