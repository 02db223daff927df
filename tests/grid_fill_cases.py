"""The cases the CPU and the GPU tests of fill_gaps, smooth and clean_drift share, with the specification's results computed
once per process (tests/grid_fill_spec.py).  No tests in here."""
import numpy as np

from sea_ice_drift_amd import _capi
from tests import grid_fill_spec as fs
from tests.golden import make_golden_grid as mgg

TR, TC = _capi.GRID_TILE
SINGLE = (4, 16)                    # the one known node of the 'single' cases, on a 9 x 33 grid


def field(rows, cols, seed, rejected=0.15, hole=None):
    """A smooth field with noise; `rejected` of the nodes masked, NaN at a few more, and a rectangular hole (r0, r1, c0, c1)."""
    rng = np.random.default_rng(seed)
    r, c = np.meshgrid(np.arange(rows, dtype=np.float64), np.arange(cols, dtype=np.float64), indexing='ij')
    u = 0.1 * np.cos(0.05 * r + 0.03 * c) + 0.01 * rng.standard_normal(r.shape)
    v = 0.08 * np.sin(0.04 * r - 0.02 * c) + 0.01 * rng.standard_normal(r.shape)
    valid = rng.random(r.shape) >= rejected
    u[rng.random(r.shape) < 0.03] = np.nan
    v[rng.random(r.shape) < 0.02] = np.inf
    if hole is not None:
        valid[hole[0]:hole[1], hole[2]:hole[3]] = False
    return u, v, valid


def single(v0=-0.0):
    u, v = np.full((9, 33), np.nan), np.full((9, 33), np.nan)
    u[SINGLE], v[SINGLE] = 0.25, v0
    return u, v


def walled(radius):
    """9 x 14: known nodes on the left, a wall of domain = 0 (as wide as the window reaches) and nothing known to its right.
    Some wall nodes hold values: generation 0 all the same, and the only source the right side could have."""
    u, v, valid = field(9, 14, 2305, rejected=0.3)
    domain = np.ones((9, 14), dtype=np.uint8)
    domain[:, 6:6 + radius] = 0
    valid[:, 6:] = False
    domain[0, 2] = domain[5, 3] = 0                 # two more nodes that may not be filled, among the known ones
    valid[0, 2] = valid[5, 3] = False
    return u, v, valid, domain


def huge():
    """Neighbours of +-1e308 around holes: an even median of two equal ones overflows to inf."""
    rng = np.random.default_rng(2306)
    u = np.where(rng.random((7, 9)) < 0.5, 1e308, -1e308)
    v = np.where(rng.random((7, 9)) < 0.5, 1e308, -1e308)
    valid = rng.random((7, 9)) >= 0.25
    valid[2:5, 3:6] = False
    return u, v, valid


def fill_cases():
    """name -> (u, v, valid, domain, radius, min_neighbours, max_passes)"""
    cases = {}
    for rows, cols in ((1, 1), (1, 9), (9, 1)):
        for radius in (1, 2):
            cases['thin_%dx%d_r%d' % (rows, cols, radius)] = field(rows, cols, 2300 + rows + cols, rejected=0.4) + (None, radius, 1, 16)
    # a hole across the corner where four tiles meet (rows TR-2..TR+1, cols TC-2..TC+1), clipped by the 9 x 33 grid
    for rows, cols in ((TR + 1, TC + 1), (2 * TR + 1, 2 * TC + 1)):
        for radius, minn in ((1, 3), (2, 3), (1, 5), (2, 12)):
            u, v, valid = field(rows, cols, 2310 + rows, hole=(TR - 2, TR + 2, TC - 2, TC + 2))
            cases['tiles_%dx%d_r%d_m%d' % (rows, cols, radius, minn)] = (u, v, valid, None, radius, minn, 16)
    for radius in (1, 2):
        cases['single_r%d' % radius] = single() + (None, None, radius, 1, 16)
        cases['walled_r%d' % radius] = walled(radius) + (radius, 2, 16)
    cases['single_r1_p5'] = single() + (None, None, 1, 1, 5)
    cases['single_r1_m2'] = single() + (None, None, 1, 2, 16)
    u, v, _ = field(6, 7, 2320)
    cases['all_unusable'] = (u, v, np.zeros((6, 7), dtype=bool), None, 1, 1, 16)
    cases['all_nan'] = (np.full((3, 40), np.nan), np.full((3, 40), np.nan), None, None, 2, 1, 3)
    qu, qv, qvalid = mgg.filter_field('quant')                       # four levels with both zeros: medians tie
    for radius, minn in ((1, 1), (1, 3), (2, 2), (2, 4)):
        cases['quant_r%d_m%d' % (radius, minn)] = (qu, qv, qvalid, None, radius, minn, 16)
    for radius, minn in ((1, 2), (1, 4), (2, 2)):
        cases['huge_r%d_m%d' % (radius, minn)] = huge() + (None, radius, minn, 16)
    return cases


def asymmetric_weights(radius):
    """No symmetry at all, some zeros, a centre > 0."""
    side = 2 * radius + 1
    w = np.random.default_rng(2330 + radius).random((side, side))
    w[0, side - 1] = w[side - 1, 1] = 0.0
    w[radius, radius] = 0.75
    return w


def smooth_cases():
    """name -> (u, v, valid, kwargs of smooth)"""
    cases = {}
    for rows, cols in ((TR + 1, TC + 1), (2 * TR + 1, 2 * TC + 1)):
        u, v, valid = field(rows, cols, 2340 + rows, rejected=0.25)
        for r, c in ((0, 0), (0, cols - 1), (rows - 1, 0), (rows - 1, cols - 1), (0, 7), (5, 0), (rows - 1, 20), (3, cols - 1)):
            valid[r, c] = False                                      # masked nodes in corners and on edges
        for radius in (1, 2):
            cases['gauss_%dx%d_r%d' % (rows, cols, radius)] = (u, v, valid, dict(radius=radius, sigma=0.8 * radius))
            cases['table_%dx%d_r%d' % (rows, cols, radius)] = (u, v, valid, dict(radius=radius, weights=asymmetric_weights(radius)))
    u, v, _ = field(9, 12, 2350, rejected=0.0)
    cases['default_no_mask'] = (u, v, None, {})
    for rows, cols in ((1, 1), (1, 9), (9, 1)):
        u, v, valid = field(rows, cols, 2360 + rows, rejected=0.3)
        cases['thin_%dx%d' % (rows, cols)] = (u, v, valid, dict(radius=2, sigma=1.5))
    valid = np.zeros((7, 7), dtype=bool)
    valid[3, 3] = valid[0, 0] = True                                 # isolated nodes: (w * u) / w
    u, v, _ = field(7, 7, 2370, rejected=0.0)
    u, v = np.nan_to_num(u, nan=0.3), np.nan_to_num(v, posinf=-0.7)
    for radius in (1, 2):
        cases['isolated_r%d' % radius] = (u, v, valid, dict(radius=radius, weights=asymmetric_weights(radius)))
    cases['all_unusable'] = (u, v, np.zeros((7, 7), dtype=bool), dict(radius=1))
    return cases


FILL, SMOOTH = fill_cases(), smooth_cases()
_expected = {}


def fill_expected(name):
    if ('fill', name) not in _expected:
        u, v, valid, domain, radius, minn, passes = FILL[name]
        _expected['fill', name] = fs.fill_gaps(u, v, valid, domain, radius, minn, passes)
    return _expected['fill', name]


def smooth_expected(name):
    if ('smooth', name) not in _expected:
        u, v, valid, kw = SMOOTH[name]
        _expected['smooth', name] = fs.smooth(u, v, valid=valid, **kw)
    return _expected['smooth', name]


def chain_truth():
    """The linear field of make_golden_grid.chain_inputs before the outliers were planted."""
    _, _, x, y = mgg.pm_geometry(12, 15)
    return 0.05 + 2e-7 * (x - 5e5) - 1e-7 * (y + 1e6), -0.02 + 3e-7 * (x - 5e5) + 0.5e-7 * (y + 1e6)


def chain_expected(**kw):
    key = ('chain',) + tuple(sorted(kw.items()))
    if key not in _expected:
        x, y, u, v, usable, planted, eps = mgg.chain_inputs()
        _expected[key] = fs.clean_drift(u, v, eps, valid=usable, **kw)
    return _expected[key]


def step_of(truth, radius):
    """The largest difference of `truth` between two nodes within Chebyshev distance `radius`."""
    rows, cols = truth.shape
    worst = 0.0
    for di in range(-radius, radius + 1):
        for dj in range(-radius, radius + 1):
            a = truth[max(di, 0):rows + min(di, 0), max(dj, 0):cols + min(dj, 0)]
            b = truth[max(-di, 0):rows + min(-di, 0), max(-dj, 0):cols + min(-dj, 0)]
            worst = max(worst, float(np.abs(a - b).max()))
    return worst


def same_fill(got, exp):
    from tests import grid_spec as gs
    return (gs.same_bits(got[0], exp[0]) and gs.same_bits(got[1], exp[1]) and
            np.asarray(got[2]).dtype == np.int32 and np.array_equal(got[2], exp[2]))


def check_properties(name, exp):
    """What each case is there for, asserted on the SPECIFICATION's result (so a case that stops covering its reason fails)."""
    uf, vf, gen = exp
    u, v, valid, domain, radius, minn, passes = FILL[name]
    if name in ('single_r1', 'single_r2'):
        i, j = np.indices(gen.shape)
        cheb = np.maximum(np.abs(i - SINGLE[0]), np.abs(j - SINGLE[1]))
        assert np.array_equal(gen, -(-cheb // radius))                                  # ceil(Chebyshev distance / radius)
        assert np.signbit(vf[SINGLE]) and vf[SINGLE] == 0.0                             # the known node keeps its sign bit
        filled = gen > 0
        assert (uf[filled] == 0.25).all() and (vf[filled] == 0.0).all() and not np.signbit(vf[filled]).any()
    elif name == 'single_r1_p5':
        assert int((gen == -1).sum()) == 198 and gen.max() == 5
        assert np.isnan(uf[gen == -1]).all() and np.isnan(vf[gen == -1]).all()
    elif name == 'single_r1_m2':
        assert int((gen == 0).sum()) == 1 and int((gen == -1).sum()) == gen.size - 1
    elif name in ('all_unusable', 'all_nan'):
        assert (gen == -1).all() and np.isnan(uf).all() and np.isnan(vf).all()
    elif name.startswith('walled'):
        assert (gen[:, 6 + radius:] == -1).all()                                        # the walled-off region: no source
        assert (gen[(domain == 0) & ~valid] == -1).all() and (gen[:, :6][domain[:, :6] != 0] >= 0).all()
        assert gen[0, 2] == -1 and gen[5, 3] == -1 and gen.max() >= 1
    elif name.startswith('quant'):
        filled = gen > 0
        assert filled.any() and (uf[filled] == 0.0).any() and not np.signbit(uf[filled & (uf == 0.0)]).any()
        assert set(np.unique(uf[filled])) - {-0.5, -0.25, 0.0, 0.25, 0.5} == set()
    elif name.startswith('huge'):
        bad = (gen > 0) & ~(np.isfinite(uf) & np.isfinite(vf))
        assert bad.any()                                                                # a generation, but an inf value
        if name == 'huge_r1_m2':
            assert gen.max() >= 2                                                       # and passes after it
    elif name.startswith('tiles'):
        ok = valid & np.isfinite(u) & np.isfinite(v)
        assert (gen[ok] == 0).all() and (gen[~ok] != 0).all() and (gen[TR - 2:TR + 2, TC - 2:TC + 2] > 0).any()
        if radius == 1 and minn == 3:
            assert gen.max() >= 2 and gen[TR - 1, TC - 1] > 0                           # the hole takes more than one pass
