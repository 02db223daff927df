"""The edge cases of the winner's NCC matrix (tests/winner_edge_cases.py) are what they are made for - asserted on the C oracle
alone, no GPU: an exact 1.0f, an exact -1.0f, zeros from the low-variance rule, an all-ones matrix, an ordinary matrix; at every
shape tests/test_gpu_winner_edges.py runs."""
import numpy as np
import pytest

from tests import winner_edge_cases as wc


@pytest.mark.parametrize('case', wc.CASES)
def test_cases_are_what_they_are_made_for(c_oracle, case):
    for (s, b, K) in wc.SHAPES:
        try:
            wc.check(case, s, b, K, wc.reference(c_oracle, case, s, b, K))
        except AssertionError as e:
            raise AssertionError('%s, side %d, border %d, %d angles: %s' % (case, s, b, K, e))
    # the set_points route: the oracle answers every point, with a finite h unless the template is constant
    for s in wc.PLAN_SIDES:
        for _pair, borders in wc.plan_sets(case, s):
            for K in wc.PLAN_ANGLES:
                exp, exp_ij = wc.plan_reference(c_oracle, case, s, K, borders)
                assert exp.shape == (len(borders), 5) and (exp_ij[:, 2] >= 0).all()
                assert np.isnan(exp[:, 4]).all() if case == 'const' else np.isfinite(exp).all(), (case, s, K, borders)
