"""The inputs of tests/test_gpu_template_sides.py on the C oracle alone: every claim that file makes about its cases (NaN
patterns, finite rows, winners in the later groups of slots, peaks on and off the edge of a small NCC matrix, the launch classes
of the hand-over borders) holds before a kernel is asked, and the oracle's Hessian equals NumPy / SciPy at the small shapes.
No GPU."""
import os
import subprocess

import numpy as np
import pytest

from tests import side_cases as sc


def test_every_side_has_its_nan_pattern_and_its_finite_rows(c_oracle):
    """Sides 2 .. 64 (without 34 / 35), three angle sets: odd sides answer border 0 with NaN rows, even sides with a finite row
    whose h is NaN; the zero-pixel row is NaN; at least six rows are finite."""
    pair = sc.speckled_pair()
    for s in sc.SIDES:
        g = sc.side_points(s)
        for angles in (sc.ANGLES3, sc.ANGLES9, sc.ANGLES17):
            exp, exp_ij = sc.oracle_batch(c_oracle, pair, g, s, angles)
            sc.check_side_set(s, exp, exp_ij)


def test_rolled_pair_puts_the_winners_into_the_second_group(c_oracle):
    pair = sc.rolled_pair()
    for s in sc.SIDES:
        exp, exp_ij = sc.oracle_batch(c_oracle, pair, sc.rolled_points(s), s, sc.ANGLES_ROLLED)
        sc.check_rolled_set(exp, exp_ij)


@pytest.mark.parametrize('s', [20, 50])
def test_angle_counts_put_the_winners_into_the_last_group(c_oracle, s):
    pair = sc.rolled_pair()
    g = sc.rolled_points(s, borders=(3, 20) * 4, seed=1)
    for K in (1, 7, 8, 15, 16, 31, 64):
        angles = sc.count_angles(K)
        assert len(angles) == K and angles[-1] == 0.0
        exp, exp_ij = sc.oracle_batch(c_oracle, pair, g, s, angles)
        sc.check_rolled_set(exp, exp_ij, first=sc.last_group_start(K), at_least=len(g['border']) // 2)
    assert sc.last_group_start(16) == 15 and sc.last_group_start(31) == 30 and sc.last_group_start(64) == 60


@pytest.mark.parametrize('sides,angle_sets', [((20, 21), (sc.ANGLES3, sc.ANGLES9, sc.ANGLES17)), ((34, 35), (sc.ANGLES3, sc.ANGLES7, sc.ANGLES15))])
def test_small_matrix_sets(c_oracle, sides, angle_sets):
    """Each family has both parities of the placement count; each set has a peak on the edge and one off it at every matrix size
    with an interior, windows without a placement pair (odd side, border 0), 2 x 2 matrices (even side, border 0) and the constant
    template, under every combination of hes_norm, hes_smth and mcc_norm."""
    pair = sc.speckled_pair()
    parities = set()
    for s in sides:
        g = sc.small_matrix_points(s)
        parities |= {sc.placements(s, b) % 2 for b in g['border']}
        assert {sc.placements(s, b) for b in sc.SMALL_BORDERS} == ({2, 4, 6, 8, 10, 14} if s % 2 == 0 else {1, 3, 5, 7, 9, 13})
        for angles in angle_sets:
            for flags in range(8):
                exp, exp_ij = sc.oracle_batch(c_oracle, pair, g, s, angles, flags=flags)
                sc.check_small_set(s, g, exp, exp_ij, flags)
    assert parities == {0, 1}


@pytest.mark.parametrize('shape', sc.HES_SHAPES)
def test_oracle_hessian_is_numpys_at_small_shapes(c_oracle, shape):
    """c_oracle.hessian against gaussian_filter / np.gradient / np.hypot / np.median / np.std: matrices with fewer rows or columns
    than the Gaussian's radius (the reflection folds several times) and without an interior; 2 x 2 with hes_norm is 0 / 0 in both."""
    m = sc.hessian_matrix(shape)
    for flags in range(4):
        want = sc.numpy_hessian(m, flags)
        got = c_oracle.hessian(m, flags=flags)
        np.testing.assert_array_equal(np.isnan(got), np.isnan(want))
        np.testing.assert_allclose(got, want, rtol=1e-5, atol=1e-5, equal_nan=True)
        if shape == (2, 2):
            assert np.isnan(got).all() if flags & 1 else (got == 0).all()
        else:
            assert np.isfinite(got).all() and got.any()


def test_handover_borders_from_a_class_table():
    """handover_borders on a made-up table: first and last border of every class, and the first large one."""
    borders, cls = sc.handover_borders([3, 3, 3, 2, 1, 1, 129, 129], first=1)
    assert borders == [1, 3, 4, 5, 6, 7] and cls == [3, 3, 2, 1, 1, 129]


@pytest.mark.parametrize('s', sc.HANDOVER_SIDES)
def test_handover_points_cover_every_class(c_oracle, s):
    """The library's host arithmetic gives the classic kernel up to three workgroups per CU, fewer as the border grows, and then
    hands over to the large-window pipeline; the points picked at those borders are finite in the oracle."""
    from sea_ice_drift_amd import _capi
    g, cls = sc.handover_points(s)
    assert (cls[-2:] & _capi.CLASS_LARGE).all()
    classic = cls[:-2]
    assert set(classic.tolist()) <= {1, 2, 3}
    assert (np.diff(classic) <= 0).all()                                # larger windows, fewer workgroups per CU
    assert g['border'][-1] == g['border'][-3] + 1
    assert (np.diff(g['border']) >= 0).all() and g['border'][0] == 1
    exp, _ = sc.oracle_batch(c_oracle, sc.handover_pair(), g, s, sc.ANGLES15)
    assert np.isfinite(exp).all()


def test_tiny_side_sets(c_oracle):
    """Sides 2 .. 5: the constant-template points have an all-ones matrix that fills the median's list, under every flag."""
    pair = sc.speckled_pair()
    for s in sc.TINY_SIDES:
        g = sc.tiny_side_points(s)
        for angles in (sc.ANGLES3, sc.ANGLES9):
            for flags in range(8):
                exp, exp_ij = sc.oracle_batch(c_oracle, pair, g, s, angles, flags=flags)
                sc.check_tiny_set(s, g, exp, exp_ij, flags)


def test_edge_sets(c_oracle):
    """Windows one row or column short at the top / left edge of image 2: the sizes the points are made for, under every flag."""
    pair = sc.speckled_pair()
    for s in sc.EDGE_SIDES:
        g, shape = sc.edge_points(s)
        for angles in (sc.ANGLES3, sc.ANGLES9):
            for flags in range(8):
                exp, exp_ij = sc.oracle_batch(c_oracle, pair, g, s, angles, flags=flags)
                sc.check_edge_set(s, g, shape, exp, exp_ij)


def test_classic_lds_layout_invariants(tmp_path):
    """mfma_lds_layout (csrc/pm_kernel.h is plain C++ on the host) at every side 2 .. 64, paired and not, borders 0 .. 70: the
    k-groups of a table row, the window pitch against the last fragment read, the regions in order, and the 5 KB of median
    scratch that ph_hessian lays over the dead winner operands in front of the NCC matrix."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / 'mfma_layout_check')
    subprocess.check_call(['g++', '-std=c++17', '-O1', '-o', exe, os.path.join(root, 'tests', 'cpp', 'mfma_layout_check.cpp')])
    p = subprocess.run([exe], stdout=subprocess.PIPE, universal_newlines=True)
    assert p.returncode == 0 and p.stdout.strip().endswith(' 0 violations'), p.stdout[-3000:]
