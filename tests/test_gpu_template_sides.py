"""GPU parity of the classic one-workgroup-per-point kernel (`pm_kernel_mfma<0, 4, paired>`, csrc/pm_kernel_classic.h) at its
run-time template sides - every side 2 .. 64 but 34 and 35, which the row-pair kernels take - and of the Hessian code of every
kernel family on NCC matrices of 2 .. 14 placements per axis.

The kernel branches on the side: three or four k-groups of 16 template columns (s <= 48 / above), the tail mask of the last quad
of a template row (s & 3), the pitch of the sampling table, the paired table's zero rows, the winner's step count.  The Hessian
branches on the matrix: no interior below 5 x 5, a Gaussian whose radius of 4 exceeds the axis and folds several times, medians
and standard deviations of 4 .. 196 values, an all-zero Hessian at 2 x 2.

Everything against the C oracle under the parity rule (tests/side_cases.py assert_parity).  The cases come from tests/side_cases.py;
what they are made for is asserted from the oracle's answer before the kernel's is looked at (tests/test_side_cases_cpu.py checks
the same where there is no GPU)."""
import numpy as np
import pytest

from sea_ice_drift_amd import _capi, pmlib as my
from tests import side_cases as sc

pytestmark = pytest.mark.gpu

_REF = {}


def _oracle(c_oracle, name, pair, g, s, angles, flags=1):
    """The C oracle's answer, computed once per case and shared."""
    key = (name, s, tuple(angles), flags)
    if key not in _REF:
        _REF[key] = sc.oracle_batch(c_oracle, pair, g, s, angles, flags=flags)
    return _REF[key]


def _run(ctx, g, s, angles, flags=1):
    ctx.set_points(*sc.vectors(g), s, 0.0, angles, rot=sc.rot_of(angles, s), flags=flags)
    ctx.run()
    return ctx.fetch()


# ---- a. every side ----

@pytest.mark.parametrize('s', sc.SIDES)
def test_every_side(pm_ctx, c_oracle, s):
    """Ten points, borders 0, 0, 1, 2, 3, 4, 7, 12, 20, 20, one fractional centre, one template on zero pixels; 3 angles (paired
    slots), 9 (one group, unpaired) and 17 (two groups); then the rolled pair, whose winners are the last two of 17 angles."""
    pair, g = sc.speckled_pair(), sc.side_points(s)
    refs = []
    for angles in (sc.ANGLES3, sc.ANGLES9, sc.ANGLES17):
        exp, exp_ij = _oracle(c_oracle, 'side', pair, g, s, angles)
        sc.check_side_set(s, exp, exp_ij)
        refs.append((angles, exp, exp_ij))
    rolled, gr = sc.rolled_pair(), sc.rolled_points(s)
    exp_r, exp_r_ij = _oracle(c_oracle, 'rolled', rolled, gr, s, sc.ANGLES_ROLLED)
    sc.check_rolled_set(exp_r, exp_r_ij)
    pm_ctx.upload_pair(*pair)
    for angles, exp, exp_ij in refs:
        got, ij = _run(pm_ctx, g, s, angles)
        sc.assert_parity(got, ij, exp, exp_ij)
    pm_ctx.upload_pair(*rolled)
    got, ij = _run(pm_ctx, gr, s, sc.ANGLES_ROLLED)
    sc.assert_parity(got, ij, exp_r, exp_r_ij)


# ---- b. whole templates and whole matrices at the k-group and tail-mask boundaries ----

@pytest.mark.parametrize('s', sc.BOUNDARY_SIDES)
def test_whole_templates_and_matrices_at_the_boundaries(pm_ctx, c_oracle, s):
    """debug_point: every one of the K templates against the oracle's get_template, the winning angle's NCC matrix against its
    match_template of the same window and template, the raw Hessian against its hessian - all bit for bit; 3 and 9 angles,
    borders 2 and 20, an integral and a fractional centre."""
    img1, img2 = sc.speckled_pair()
    hws = s // 2
    pm_ctx.upload_pair(img1, img2)
    for angles in (sc.ANGLES3, sc.ANGLES9):
        rot = sc.rot_of(angles, s)
        for b in (2, 20):
            for (c1, r1) in ((200.0, 180.0), (200.3, 179.55)):
                c2, r2 = 203.0, 178.0
                want_t = [c_oracle.get_template(img1, c1, r1, rot[k], s) for k in range(len(angles))]
                assert min(int(t.min()) for t in want_t) > 0                                  # no NaN point
                exp, exp_ij = c_oracle.pm_batch(img1, img2, [c1], [r1], [c2], [r2], [float(b)], s, 0.0, angles, rot=rot)
                assert np.isfinite(exp).all()
                msg = 'side %d, %d angles, border %d, centre %r' % (s, len(angles), b, (c1, r1))
                d = pm_ctx.debug_point(c1, r1, c2, r2, float(b), s, 0.0, angles, rot=rot)
                for k in range(len(angles)):
                    np.testing.assert_array_equal(d['templates'][k], want_t[k], err_msg=msg + ', template %d' % k)
                np.testing.assert_array_equal(d['ij'], exp_ij[0], err_msg=msg)
                r0, c0, w = int(r2) - hws - b, int(c2) - hws - b, 2 * hws + 2 * b + 1
                want = c_oracle.match_template(img2[r0:r0 + w, c0:c0 + w], want_t[int(exp_ij[0, 2])])
                assert d['ccm'].shape == want.shape == (sc.placements(s, b),) * 2
                np.testing.assert_array_equal(d['ccm'], want, err_msg=msg)
                np.testing.assert_array_equal(d['hes'], c_oracle.hessian(want, flags=0), err_msg=msg)
                np.testing.assert_array_equal(d['out'][:4], exp[0, :4], err_msg=msg)
                np.testing.assert_allclose(d['out'][4], exp[0, 4], rtol=1e-5, atol=1e-5, err_msg=msg)


# ---- c. angle counts ----

@pytest.mark.parametrize('K', [1, 7, 8, 15, 16, 31, 64])
@pytest.mark.parametrize('s', [20, 50])
def test_angle_counts(pm_ctx, c_oracle, s, K):
    """1 .. 64 angles (kMaxAngles: four full groups of 15 and one of four) at a side with three k-groups and one with four; eight
    points, borders 3 and 20; 0 degrees is the last angle of the list, so the last group holds the winners."""
    pair = sc.rolled_pair()
    g = sc.rolled_points(s, borders=(3, 20) * 4, seed=1)
    angles = sc.count_angles(K)
    exp, exp_ij = _oracle(c_oracle, 'count', pair, g, s, angles)
    sc.check_rolled_set(exp, exp_ij, first=sc.last_group_start(K), at_least=4)
    pm_ctx.upload_pair(*pair)
    got, ij = _run(pm_ctx, g, s, angles)
    sc.assert_parity(got, ij, exp, exp_ij)


# ---- d. Hessian options on small matrices, in every kernel family ----

@pytest.mark.parametrize('s,angles', [(20, sc.ANGLES3), (20, sc.ANGLES9), (20, sc.ANGLES17), (21, sc.ANGLES3), (21, sc.ANGLES9),
                                      (21, sc.ANGLES17), (34, sc.ANGLES3), (34, sc.ANGLES7), (34, sc.ANGLES15), (35, sc.ANGLES3),
                                      (35, sc.ANGLES7), (35, sc.ANGLES15)], ids=lambda v: str(len(v)) if isinstance(v, list) else str(v))
def test_hessian_options_on_small_matrices(pm_ctx, c_oracle, monkeypatch, s, angles):
    """Borders 0, 1, 2, 3, 4 and 6 - matrices of 2 .. 14 (even sides) and 1 .. 13 (odd sides: border 0 has no placement pair, a NaN
    row) - under every combination of hes_norm, hes_smth and mcc_norm: the classic kernel (sides 20 / 21: the general
    ph_hessian, one and several groups), the row-pair kernels (34 / 35: quad, paired, full table; ph_hessian_fast under
    hes_norm alone), and the same points through the large-window pipeline (SID_PM_ALL_LARGE: lw_reflect, its median).  A constant template rides along: the matrix is all ones,
    sd = 0 under mcc_norm and hes_norm, and what the oracle answers (NaN) is what the kernel must answer."""
    pair, g = sc.speckled_pair(), sc.small_matrix_points(s)
    pm_ctx.upload_pair(*pair)
    monkeypatch.delenv('SID_PM_ALL_LARGE', raising=False)
    # the family the host arithmetic gives these points: only the row-pair kernels keep sums in global memory (CLASS_GS)
    gs = (_capi.estimate_residency(g['border'], s, len(angles)) & _capi.CLASS_GS) != 0
    valid = np.array([sc.placements(s, b) >= 2 for b in g['border']])
    assert gs[valid].all() if s in (34, 35) else not gs.any()
    try:
        for flags in range(8):
            exp, exp_ij = _oracle(c_oracle, 'small', pair, g, s, angles, flags=flags)
            sc.check_small_set(s, g, exp, exp_ij, flags)
            n_refused = int((exp_ij[:, 2] < 0).sum())                  # (no zero pixel here: windows without a placement pair)
            info = {}
            for env in (None, 'SID_PM_ALL_LARGE'):
                monkeypatch.delenv('SID_PM_ALL_LARGE', raising=False)
                if env:
                    monkeypatch.setenv(env, '1')
                got, ij = _run(pm_ctx, g, s, angles, flags=flags)
                info[env] = pm_ctx.work_info()
                if env:
                    # every valid window went through the pipeline: no launch of a one-point kernel but the one that writes the
                    # NaN rows, and no window in LDS
                    assert info[env]['launches'] == (1 if n_refused else 0)
                    assert info[None]['launches'] >= 1 and info[None]['max_lds_bytes'] > info[env]['max_lds_bytes']
                    assert info[env]['valid_points'] == info[None]['valid_points'] == len(g['border']) - n_refused
                try:
                    sc.assert_parity(got, ij, exp, exp_ij, mcc_norm=bool(flags & 4))
                except AssertionError as e:
                    raise AssertionError('flags %d, %s, borders %s:\n%s' % (flags, env or 'one workgroup per point', g['border'].astype(int).tolist(), e))
    finally:
        monkeypatch.delenv('SID_PM_ALL_LARGE', raising=False)


@pytest.mark.parametrize('s', sc.TINY_SIDES)
def test_median_scratch_at_the_smallest_sides(pm_ctx, c_oracle, s):
    """Sides 2 .. 5 with all-ones NCC matrices of 169 .. 256 values under every flag: the median's list of keys is full.  At
    sides 2 and 3 the winner's operand blocks are shorter than the 5 KB of median scratch laid over them, and the end of the
    list once lay over the first values of the NCC matrix (mcc_norm ranks that matrix, the Hessian reads it afterwards)."""
    pair, g = sc.speckled_pair(), sc.tiny_side_points(s)
    pm_ctx.upload_pair(*pair)
    for angles in (sc.ANGLES3, sc.ANGLES9):
        for flags in range(8):
            exp, exp_ij = _oracle(c_oracle, 'tiny', pair, g, s, angles, flags=flags)
            sc.check_tiny_set(s, g, exp, exp_ij, flags)
            got, ij = _run(pm_ctx, g, s, angles, flags=flags)
            try:
                sc.assert_parity(got, ij, exp, exp_ij, mcc_norm=bool(flags & 4))
            except AssertionError as e:
                raise AssertionError('%d angles, flags %d:\n%s' % (len(angles), flags, e))


@pytest.mark.parametrize('s', sc.EDGE_SIDES)
def test_windows_one_short_at_the_top_and_left_edge(pm_ctx, c_oracle, s):
    """A first guess within a pixel of the top / left edge of image 2 starts its window at 0 and loses a row or column: the
    one-point kernels take such a window (it is not clipped at the far side), and its matrix is not square.  6 x 5 has an
    interior of one column - ph_hessian divides by its width -, sides 2 and 3 at border 1 a window of one dword per row and
    more rows than columns.  Borders 1, 2, 3, every flag, 3 and 9 angles."""
    pair = sc.speckled_pair()
    g, shape = sc.edge_points(s)
    pm_ctx.upload_pair(*pair)
    for angles in (sc.ANGLES3, sc.ANGLES9):
        for flags in range(8):
            exp, exp_ij = _oracle(c_oracle, 'edge', pair, g, s, angles, flags=flags)
            sc.check_edge_set(s, g, shape, exp, exp_ij)
            got, ij = _run(pm_ctx, g, s, angles, flags=flags)
            assert pm_ctx.work_info()['launches'] >= 1 and pm_ctx.work_info()['valid_points'] == len(shape)
            try:
                sc.assert_parity(got, ij, exp, exp_ij, mcc_norm=bool(flags & 4))
            except AssertionError as e:
                raise AssertionError('%d angles, flags %d, windows %s:\n%s' % (len(angles), flags, shape.tolist(), e))


# ---- e. get_hessian and rotate_and_match at the same sizes ----

@pytest.mark.parametrize('shape', sc.HES_SHAPES)
def test_get_hessian_of_small_matrices(c_oracle, shape):
    """pmlib.get_hessian under hes_norm / hes_smth against the oracle and against NumPy / SciPy written out (side_cases.numpy_hessian);
    2 x 2 under hes_norm is NaN in all three."""
    m = sc.hessian_matrix(shape)
    for flags in range(4):
        want, want_np = c_oracle.hessian(m, flags=flags), sc.numpy_hessian(m, flags)
        np.testing.assert_allclose(want, want_np, rtol=1e-5, atol=1e-5, equal_nan=True)
        assert np.isnan(want).all() if (shape == (2, 2) and flags & 1) else np.isfinite(want).all()
        got = my.get_hessian(m, hes_norm=bool(flags & 1), hes_smth=bool(flags & 2))
        assert got.shape == shape and got.dtype == np.float32
        for ref in (want, want_np):
            np.testing.assert_array_equal(np.isnan(got), np.isnan(ref), err_msg='flags %d' % flags)
            np.testing.assert_allclose(got, ref, rtol=1e-5, atol=1e-5, equal_nan=True, err_msg='flags %d' % flags)


@pytest.mark.parametrize('s', [20, 34, 100])
def test_rotate_and_match_on_windows_of_few_placements(pm_ctx, c_oracle, s):
    """Windows of s + 1 .. s + 9 rows by s + 1 .. s + 9 columns (2 .. 10 placements per axis, all 81 rectangles) through the
    large-window pipeline, hes_smth with and without mcc_norm: NCC matrix and template bit for bit, out5 under the parity rule."""
    img1, img2 = sc.speckled_pair()
    angles = sc.ANGLES3
    rot = sc.rot_of(angles, s)
    c1, r1, r0, c0 = 200.0, 200.0, 150, 140
    pm_ctx.upload_pair(img1, img2)
    for flags in (3, 7):
        for wh in range(s + 1, s + 10):
            for ww in range(s + 1, s + 10):
                image2 = np.ascontiguousarray(img2[r0:r0 + wh, c0:c0 + ww])
                exp = c_oracle.rotate_and_match(img1, c1, r1, s, image2, 0.0, angles, rot, flags=flags)
                assert exp['ij'][2] >= 0 and exp['ccm'].shape == (wh - s + 1, ww - s + 1)
                got = pm_ctx.rotate_and_match(c1, r1, s, 0.0, angles, rot=rot, flags=flags, window=(r0, c0, wh, ww))
                msg = 'side %d, window %d x %d, flags %d' % (s, wh, ww, flags)
                np.testing.assert_array_equal(got['ij'], exp['ij'], err_msg=msg)
                np.testing.assert_array_equal(got['ccm'], exp['ccm'], err_msg=msg)
                np.testing.assert_array_equal(got['template'], exp['template'], err_msg=msg)
                sc.assert_parity(got['out'][None, :], got['ij'][None, :], exp['out'][None, :], exp['ij'][None, :], mcc_norm=bool(flags & 4))


# ---- f. hand-over to the large-window pipeline ----

@pytest.mark.parametrize('s', sc.HANDOVER_SIDES)
def test_handover_to_the_large_window_pipeline(pm_ctx, c_oracle, s):
    """The last border estimate_residency gives to the classic kernel, the first it marks CLASS_LARGE, and the first and last
    border of every workgroups-per-CU class below: two points each, 15 angles.  The classes are separate launches, and the points
    of the pipeline are in none of them."""
    pair = sc.handover_pair()
    g, cls = sc.handover_points(s)
    classic = cls[(cls & _capi.CLASS_LARGE) == 0]
    print('side %d: borders %s, classes %s' % (s, g['border'][::2].astype(int).tolist(), cls[::2].tolist()))
    assert (cls[-2:] & _capi.CLASS_LARGE).all() and classic.size == cls.size - 2
    n_classes = len(set(classic.tolist()))
    assert n_classes >= 1 and set(classic.tolist()) <= {1, 2, 3}      # workgroups per CU
    assert g['border'][-1] == g['border'][-3] + 1                     # the hand-over: two neighbouring borders
    exp, exp_ij = _oracle(c_oracle, 'handover', pair, g, s, sc.ANGLES15)
    assert np.isfinite(exp).all()
    pm_ctx.upload_pair(*pair)
    got, ij = _run(pm_ctx, g, s, sc.ANGLES15)
    assert pm_ctx.work_info()['launches'] == n_classes
    sc.assert_parity(got, ij, exp, exp_ij)
    tail = {k: v[-4:] for k, v in g.items()}                          # the two borders of the hand-over alone: one launch and the pipeline
    got, ij = _run(pm_ctx, tail, s, sc.ANGLES15)
    assert pm_ctx.work_info()['launches'] == 1
    sc.assert_parity(got, ij, exp[-4:], exp_ij[-4:])
