"""Chained launches (csrc/pm_plan.h launch_schedule / chain_rule, executed by sid_pm_run): the launches of a long run
go alternately onto two side streams, and launch k + 1 is released - a stream wait on signal memory - by the workgroup of
launch k that arrives last (PMArgs::chain).  Nothing in the results may depend on that order, so every case compares a chained
run bit for bit, NaN rows included, with the same run under SID_PM_NO_CHAIN=1, and with the C oracle under the parity rule
(indices, c2, r2, a, r exact; h to 1e-5).

The runs here are a few dozen points per launch - short runs, which the launcher would put side by side - so every run of this
file sets SID_PM_SIDE_BY_SIDE=0, the A/B switch that takes the side-by-side order away: what is left is `chained`, or `sequence`
with SID_PM_NO_CHAIN=1.  The order a run took is read from the line SID_PM_VERBOSE=1 prints; a device without stream
wait-value support skips with the reason that line gives.

Points sit on a 46-pixel lattice of a 640 x 640 pair: the templates (34 px, up to +-7 degrees) of two points never overlap, so a
zeroed pixel of image 1 belongs to one point."""
import re

import numpy as np
import pytest

from sea_ice_drift_amd import _capi, synthetic as syn
from sea_ice_drift_amd.pmlib import rotation_table
from tests.test_gpu_parity import assert_parity

pytestmark = pytest.mark.gpu

ANGLES15 = [float(a) for a in range(-7, 8)]
ANGLES9 = [float(a) for a in range(-4, 5)]
BORDERS5 = (20, 24, 30, 40, 50)
PER_CLASS = 24

_CACHE = {}


def pair(seed=31):
    if ('pair', seed) not in _CACHE:
        p = syn.make_pair(640, 640, seed=seed)
        for x in p:
            x.setflags(write=False)
        _CACHE['pair', seed] = p
    return _CACHE['pair', seed]


def points(borders, counts=None):
    """len(borders) x PER_CLASS (or counts[k]) lattice points, the classes interleaved over the lattice; first guess = the true
    displacement rounded, off by up to 2 px."""
    counts = [PER_CLASS] * len(borders) if counts is None else list(counts)
    n = sum(counts)
    assert n <= 121
    rng = np.random.default_rng(7)
    k = np.arange(n)
    c1 = 90.0 + 46.0 * (k % 11)
    r1 = 90.0 + 46.0 * (k // 11)
    dc, dr = syn.true_displacement(c1, r1)
    c2 = c1 + np.rint(dc) + rng.integers(-2, 3, n)
    r2 = r1 + np.rint(dr) + rng.integers(-2, 3, n)
    border = np.concatenate([np.full(m, float(b)) for b, m in zip(borders, counts)])[rng.permutation(n)]
    v = (c1, r1, c2, r2, border)
    for x in v:
        x.setflags(write=False)
    return v


def oracle(c_oracle, key, img1, img2, v, s, angles):
    if key not in _CACHE:
        _CACHE[key] = c_oracle.pm_batch(img1, img2, *v, s, 0.0, angles, rot=rotation_table(angles, 0.0, s), nthreads=8)
        for x in _CACHE[key]:
            x.setflags(write=False)
    return _CACHE[key]


class Runner(object):
    def __init__(self, ctx, monkeypatch, capfd):
        self.ctx, self.mp, self.capfd = ctx, monkeypatch, capfd
        monkeypatch.setenv('SID_PM_VERBOSE', '1')
        monkeypatch.setenv('SID_PM_SIDE_BY_SIDE', '0')

    def set_points(self, v, s, angles):
        self.ctx.set_points(*v, s, 0.0, angles, rot=rotation_table(angles, 0.0, s))

    def order_of(self, err):
        """(order, launches) of the LAST run in this stderr text; skips when the device cannot chain."""
        lines = re.findall(r'sid_pm: launch order ([a-z ]+?), (\d+) launches(?: \(not chained: ([^)]*)\))?\n', err)
        assert lines, err[-2000:]
        order, n, why = lines[-1]
        if why and 'lacks stream wait-value support' in why:
            pytest.skip('this device ' + why.replace('the device ', ''))
        assert not why, why
        return order, int(n)

    def run(self, chain=True, runs=1):
        """`runs` run() calls back to back, then the results; returns (results, indices, order, launches)."""
        if chain:
            self.mp.delenv('SID_PM_NO_CHAIN', raising=False)
        else:
            self.mp.setenv('SID_PM_NO_CHAIN', '1')
        self.capfd.readouterr()
        for _ in range(runs):
            self.ctx.run()
        self.ctx.sync()
        self.ctx.check()
        got, ij = self.ctx.fetch()
        order, n = self.order_of(self.capfd.readouterr().err)
        return got, ij, order, n

    def both(self, launches, runs=1):
        """A chained run and its SID_PM_NO_CHAIN=1 twin: orders as expected, results equal (NaN = NaN); returns the chained ones."""
        got, ij, order, n = self.run(True, runs)
        assert (order, n) == ('chained' if launches > 1 else 'sequence', launches)
        ref, ref_ij, order, n = self.run(False)
        assert (order, n) == ('sequence', launches)
        assert np.array_equal(ij, ref_ij) and np.array_equal(got, ref, equal_nan=True)
        return got, ij


def test_five_classes(pm_ctx, c_oracle, monkeypatch, capfd):
    img1, img2 = pair()
    v = points(BORDERS5)
    R = Runner(pm_ctx, monkeypatch, capfd)
    pm_ctx.upload_pair(img1, img2)
    R.set_points(v, 34, ANGLES15)
    assert pm_ctx.work_info()['launches'] == 5
    got, ij = R.both(5)
    exp, exp_ij = oracle(c_oracle, 'five', img1, img2, v, 34, ANGLES15)
    assert not np.isnan(exp[:, 0]).any()
    assert_parity(got, ij, exp, exp_ij)


def test_early_leavers_count(pm_ctx, c_oracle, monkeypatch, capfd):
    """A zero pixel under a template makes the point's workgroup leave early with a NaN row (the reference's rule): a third of
    the points of every class leave that way, and every launch still releases its successor."""
    img1, img2 = pair()
    v = points(BORDERS5)
    zero = np.zeros(v[0].size, dtype=bool)
    for b in BORDERS5:
        zero[np.flatnonzero(v[4] == b)[:PER_CLASS // 3]] = True
    img1z = img1.copy()
    assert img1z.min() >= 1
    img1z[v[1][zero].astype(int), v[0][zero].astype(int)] = 0        # the template's centre: sampled at every angle
    exp, exp_ij = oracle(c_oracle, 'leavers', img1z, img2, v, 34, ANGLES15)
    assert np.array_equal(np.isnan(exp[:, 0]), zero)
    R = Runner(pm_ctx, monkeypatch, capfd)
    pm_ctx.upload_pair(img1z, img2)
    R.set_points(v, 34, ANGLES15)
    assert pm_ctx.work_info()['launches'] == 5
    got, ij = R.both(5)
    assert_parity(got, ij, exp, exp_ij)


def test_one_handle_many_runs(pm_ctx, monkeypatch, capfd):
    img1, img2 = pair()
    v5 = points(BORDERS5)
    R = Runner(pm_ctx, monkeypatch, capfd)
    pm_ctx.upload_pair(img1, img2)
    R.set_points(v5, 34, ANGLES15)
    first, first_ij = R.both(5)
    # 50 runs back to back, nothing synchronised in between: every run has an epoch of its own, the counters are zero again
    # when a run ends, and no stream is left waiting
    got, ij, order, n = R.run(True, runs=50)
    assert (order, n) == ('chained', 5)
    assert np.array_equal(ij, first_ij) and np.array_equal(got, first, equal_nan=True)
    # other point sets on the same handle: two classes (the launch that counts its arrivals has 5 workgroups: three of its
    # eight shards are empty), one class, five again
    R.set_points(points((50, 20), (5, PER_CLASS)), 34, ANGLES15)
    assert pm_ctx.work_info()['launches'] == 2
    R.both(2)
    R.set_points(points((30,)), 34, ANGLES15)
    assert pm_ctx.work_info()['launches'] == 1
    R.both(1)
    R.set_points(v5, 34, ANGLES15)
    again, again_ij = R.both(5)
    assert np.array_equal(again_ij, first_ij) and np.array_equal(again, first, equal_nan=True)


def test_classic_kernel(pm_ctx, c_oracle, monkeypatch, capfd):
    """Template side 20 runs the classic kernel; two borders of different launch classes (estimate_residency)."""
    borders = np.arange(20.0, 61.0)
    cls = _capi.estimate_residency(borders, 20, len(ANGLES9))
    assert not (cls & _capi.CLASS_LARGE).any()
    other = borders[cls != cls[0]]
    assert other.size, cls
    img1, img2 = pair()
    v = points((int(borders[0]), int(other[0])))
    R = Runner(pm_ctx, monkeypatch, capfd)
    pm_ctx.upload_pair(img1, img2)
    R.set_points(v, 20, ANGLES9)
    assert pm_ctx.work_info()['launches'] == 2
    got, ij = R.both(2)
    exp, exp_ij = oracle(c_oracle, 'classic', img1, img2, v, 20, ANGLES9)
    assert_parity(got, ij, exp, exp_ij)


def test_both_pair_slots(pm_ctx, monkeypatch, capfd):
    img1, img2 = pair()
    other1, other2 = pair(seed=32)
    v = points(BORDERS5)
    R = Runner(pm_ctx, monkeypatch, capfd)
    pm_ctx.upload_pair(img1, img2, slot=0)
    pm_ctx.upload_pair(other1, other2, slot=1, select=False)
    R.set_points(v, 34, ANGLES15)
    a, a_ij = R.both(5)
    pm_ctx.select_pair(1)
    b, b_ij = R.both(5)
    assert not np.array_equal(a, b, equal_nan=True)                   # (other pixels: other answers)
