"""The winner's NCC matrix at the edges of its normalisation (csrc/ncc_norm.h), on the GPU - perfect and inverted matches
(|q| = 1: the clamp thresholds), flat windows (dI = 0: the short route yields NaN there and must be caught), a constant template,
and an ordinary pair - by two routes (tests/winner_edge_cases.py says what each runs):
  debug_point: the matrix of the winning angle bit for bit the C oracle's, h within 1e-5; one instantiation per side and
  angle count (the run-time pitch, the all-ones winner or rp_winner_kept) and the classic kernel, matrices of every item mix;
  set_points / run / fetch: peak, angle, c2, r2, r bit for bit and h within 1e-5 in every launch class the planner picks for
  borders 3 .. 40, with 15 / 7 / 3 angles, under SID_PM_ALWAYS_GS, SID_PM_NO_GS and SID_PM_NO_GSI as well."""
import numpy as np
import pytest

from sea_ice_drift_amd import _capi, pmlib as my
from tests import winner_edge_cases as wc

pytestmark = pytest.mark.gpu


def _run_shapes(pm_ctx, c_oracle, case, shapes):
    c1, r1, c2, r2 = wc.point()
    loaded = None
    for (s, b, K) in shapes:
        ref = wc.reference(c_oracle, case, s, b, K)
        wc.check(case, s, b, K, ref)
        pair = wc.images(case, s, b)
        if pair is not loaded:
            pm_ctx.upload_pair(*pair)
            loaded = pair
        angles = wc.ANGLES[K]
        d = pm_ctx.debug_point(c1, r1, c2, r2, float(b), s, 0.0, angles, rot=my.rotation_table(angles, 0.0, s))
        msg = '%s, side %d, border %d, %d angles' % (case, s, b, K)
        np.testing.assert_array_equal(d['ij'], ref['ij'], err_msg=msg)
        assert d['ccm'].shape == ref['ccm'].shape, msg
        np.testing.assert_array_equal(d['ccm'].view(np.uint32), ref['ccm'].view(np.uint32), err_msg=msg)   # (bits: -0.0 is not 0.0)
        np.testing.assert_array_equal(d['out'][:4], ref['out'][:4], err_msg=msg)
        np.testing.assert_allclose(d['out'][4], ref['out'][4], rtol=1e-5, atol=1e-5, equal_nan=True, err_msg=msg)


@pytest.mark.parametrize('case', wc.CASES)
def test_row_pair_kernels(pm_ctx, c_oracle, case):
    _run_shapes(pm_ctx, c_oracle, case, wc.ROW_PAIR_SHAPES)


@pytest.mark.parametrize('case', wc.CASES)
def test_classic_kernel(pm_ctx, c_oracle, case):
    _run_shapes(pm_ctx, c_oracle, case, wc.CLASSIC_SHAPES)


@pytest.mark.parametrize('case', wc.CASES)
def test_every_launch_class_through_the_planner(pm_ctx, c_oracle, monkeypatch, case):
    """set_points / run / fetch: the planner sorts borders 3 .. 40 into their launch classes; the switches force the sums into
    global memory everywhere, into LDS wherever an instantiation exists, and the all-ones winner (no kept sum w')."""
    switches = [k for k in wc.PLAN_SWITCHES if k]
    try:
        for s in wc.PLAN_SIDES:
            for pair, borders in wc.plan_sets(case, s):
                pm_ctx.upload_pair(*pair)
                for K in wc.PLAN_ANGLES:
                    exp, exp_ij = wc.plan_reference(c_oracle, case, s, K, borders)
                    if case != 'const':
                        assert np.isfinite(exp).all()
                    angles = wc.ANGLES[K]
                    rot = my.rotation_table(angles, 0.0, s)
                    for env in wc.PLAN_SWITCHES:
                        for k in switches:
                            monkeypatch.delenv(k, raising=False)
                        if env:
                            monkeypatch.setenv(env, '1')
                        pm_ctx.set_points(*wc.plan_vectors(borders), s, 0.0, angles, rot=rot)
                        pm_ctx.run()
                        got, got_ij = pm_ctx.fetch()
                        if env is None:                                # one launch per class the host arithmetic gives these borders
                            classes = _capi.estimate_residency(np.asarray(borders, dtype=np.float64), s, K)
                            assert pm_ctx.work_info()['launches'] == len(set(classes.tolist()))
                            assert len(borders) == 1 or len(set(classes.tolist())) >= 3
                        msg = '%s, side %d, borders %s, %d angles, %s' % (case, s, list(borders), K, env)
                        np.testing.assert_array_equal(got_ij, exp_ij, err_msg=msg)
                        np.testing.assert_array_equal(got[:, :4], exp[:, :4], err_msg=msg)
                        np.testing.assert_allclose(got[:, 4], exp[:, 4], rtol=1e-5, atol=1e-5, equal_nan=True, err_msg=msg)
    finally:
        for k in switches:
            monkeypatch.delenv(k, raising=False)
