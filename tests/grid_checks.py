"""Assertions the CPU and the GPU tests of include/sid_grid.h share.  No tests in here."""
import numpy as np

from tests import grid_spec as gs
from tests.golden import make_golden_grid as mgg


def assert_deformation(got, exp, what):
    for key, g, e in zip(gs.KEYS, got, exp):
        assert gs.same_bits(g, e), '%s: %s differs' % (what, key)
    assert got[5].dtype == np.int32 and np.array_equal(got[5], exp[5]), '%s: t differs' % what


def assert_filter(got, exp, what):
    assert set(np.unique(got[0]).tolist()) <= {0, 1}, '%s: keep is not 0 / 1' % what
    assert np.array_equal(np.asarray(got[0]).astype(bool), exp[0]), '%s: keep differs' % what
    assert gs.same_bits(got[1], exp[1]), '%s: res differs' % what


def chain_check(filter_fn, deformation_fn):
    """The chain on a linear velocity field (e1 = 2e-7 + 0.5e-7, e2 = hypot(1.5e-7, 2e-7), e3 = 3e-7 + 1e-7) with planted
    outliers.  The bound 1e-12 only separates the filtered result from the unfiltered one (7e-6 and more)."""
    x, y, u, v, usable, planted, eps = mgg.chain_inputs()
    assert int(planted.sum()) == 10
    keep, res = filter_fn(u, v, eps, usable)
    judged = np.isfinite(res)
    assert not keep[planted].any() and judged[planted].all()                        # every planted node rejected
    assert keep[judged & ~planted].all()                                            # and no other judged node
    assert res[judged & ~planted].max() < 1.5 and res[planted].min() > 10.0         # (1.04 and 16.5 when this was written)
    assert int((usable & ~judged).sum()) == 1 and not keep[usable & ~judged].any()  # one node has fewer than 3 neighbours
    assert not keep[~usable].any()
    want = (2.5e-7, 2.5e-7, 4e-7)
    out = deformation_fn(x, y, u, v, keep)
    has = out[5][..., 0] >= 0
    assert int(has.sum()) > 100
    for e, w in zip(out[:3], want):
        assert np.isnan(e[~has]).all() and np.abs(e[has] - w).max() < 1e-12
    raw = deformation_fn(x, y, u, v, usable)
    worst = [np.abs(e[raw[5][..., 0] >= 0] - w).max() for e, w in zip(raw[:3], want)]
    assert min(worst) > 1e-6                                                        # unfiltered: the outliers ruin it
    return (keep, res) + tuple(out)
