"""GPU parity of the sweep's ragged single items (rp_sweep_items, csrc/pm_kernel.h): the leftover placement columns of all bands
packed into full 16-wide tiles, every lane in a band of its own.  _capi.pm_batch against the C oracle under the project's parity
rule - peak row / column / angle index, c2, r2, a, r bit-exact, h within rtol = atol = 1e-5 - with no point left out."""
import numpy as np
import pytest

from sea_ice_drift_amd import _capi, pmlib as my, synthetic as syn

pytestmark = pytest.mark.gpu

ANGLES15 = list(range(-7, 8))
SIZE = 2000


def _grids(borders, shift=False):
    """make_grid(2000, 2000, 10, border=b, margin=160, seed=b) for every border (100 points each); shift: the first guess moved
    up and left by border - 4, so that the peaks fall into the last columns and rows of the placement matrix."""
    parts = []
    for b in borders:
        g = syn.make_grid(SIZE, SIZE, 10, border=b, margin=160, seed=b)
        if shift:
            g['c2fg'] = g['c2fg'] - (b - 4)
            g['r2fg'] = g['r2fg'] - (b - 4)
        parts.append(g)
    return {k: np.concatenate([p[k] for p in parts]) for k in parts[0]}


def _compare(got, ij, exp, exp_ij):
    """The parity rule, over every row."""
    assert not np.isnan(exp).any(), 'the oracle returns NaN rows: %d' % int(np.isnan(exp).any(axis=1).sum())
    np.testing.assert_array_equal(ij, exp_ij)
    np.testing.assert_array_equal(got[:, :4], exp[:, :4])
    np.testing.assert_allclose(got[:, 4], exp[:, 4], rtol=1e-5, atol=1e-5)


def _compare_with_nan(got, ij, exp, exp_ij):
    """Ties and flat windows: the oracle may answer NaN; then so must the kernel - every row is compared."""
    np.testing.assert_array_equal(ij, exp_ij)
    nan = np.isnan(exp)
    np.testing.assert_array_equal(np.isnan(got), nan)
    np.testing.assert_array_equal(got[:, :4][~nan[:, :4]], exp[:, :4][~nan[:, :4]])
    np.testing.assert_allclose(got[:, 4], exp[:, 4], rtol=1e-5, atol=1e-5, equal_nan=True)


def _run(c_oracle, img1, img2, g, s, angles, flags=1):
    rot = my.rotation_table(angles, 0.0, s)
    exp, exp_ij = c_oracle.pm_batch(img1, img2, g['c1'], g['r1'], g['c2fg'], g['r2fg'], g['border'], s, 0.0, angles, rot=rot, nthreads=16, flags=flags)
    got, ij = _capi.pm_batch(img1, img2, g['c1'], g['r1'], g['c2fg'], g['r2fg'], g['border'], s, 0.0, angles, rot=rot, flags=flags)
    return got, ij, exp, exp_ij


@pytest.fixture(scope='module')
def pair():
    return syn.make_pair(SIZE, SIZE, seed=6100)


def test_every_rem(c_oracle, pair):
    """Borders 20 .. 68: every leftover width rem = (2 b + 2) % 32 of the 4-row, 8-row and twelve-wavefront classes."""
    g = _grids(range(20, 69))
    assert g['c1'].size == 4900
    got, ij, exp, exp_ij = _run(c_oracle, pair[0], pair[1], g, 34, ANGLES15)
    _compare(got, ij, exp, exp_ij)


def test_peaks_inside_the_ragged_items(c_oracle, pair):
    """First guess moved by border - 4: most peaks lie in the leftover columns and many in the last rows of the matrix."""
    g = _grids(range(20, 69), shift=True)
    got, ij, exp, exp_ij = _run(c_oracle, pair[0], pair[1], g, 34, ANGLES15)
    rw = 2 * g['border'].astype(int) + 2
    in_leftover = int((exp_ij[:, 1] >= 32 * (rw // 32)).sum())
    in_last_rows = int((exp_ij[:, 0] >= rw - 6).sum())
    print('oracle peaks in the leftover columns: %d, in the last six rows: %d' % (in_leftover, in_last_rows))
    assert in_leftover >= 3000 and in_last_rows >= 1500
    _compare(got, ij, exp, exp_ij)


@pytest.mark.parametrize('shift', [False, True])
def test_template_side_35(c_oracle, pair, shift):
    g = _grids([20, 24, 32, 40, 50], shift=shift)
    got, ij, exp, exp_ij = _run(c_oracle, pair[0], pair[1], g, 35, ANGLES15)
    assert np.isfinite(exp[:, 0]).sum() > 0.9 * exp.shape[0]
    _compare_with_nan(got, ij, exp, exp_ij)


@pytest.mark.parametrize('kind', ['constant', 'periodic', 'flat_leftover'])
def test_ties_and_cold_paths(c_oracle, pair, kind):
    """constant: image 2 is one value - every estimate is flat, every value ties, the candidate queue overflows.  periodic: both
    images repeat an 8 x 8 tile, so equal peaks fall 8 rows and columns apart - into different bands of one ragged item; the
    first angle, then the first row-major index must win.  flat_leftover: the windows are constant from placement column 32 on
    (the flat -> exact route inside the ragged items only)."""
    img1, img2 = pair
    borders = [20, 21, 26, 30, 33, 40]
    g = _grids(borders)
    g = {k: v[::4] for k, v in g.items()}                           # 25 points per border
    if kind == 'constant':
        img2 = np.full_like(img2, 77)
    elif kind == 'periodic':
        tile = np.random.default_rng(6101).integers(1, 256, size=(8, 8)).astype(np.uint8)
        img1 = np.tile(tile, (SIZE // 8, SIZE // 8))
        img2 = img1.copy()
    else:
        img2 = img2.copy()
        for c2, r2, b in zip(g['c2fg'].astype(int), g['r2fg'].astype(int), g['border'].astype(int)):
            r0, c0, w = r2 - 17 - b, c2 - 17 - b, 35 + 2 * b
            img2[r0:r0 + w, c0 + 32:c0 + w] = 90
    got, ij, exp, exp_ij = _run(c_oracle, img1, img2, g, 34, ANGLES15)
    if kind == 'periodic':
        assert not np.isnan(exp).any() and np.all(exp[:, 3] > 0.999)     # exact ties at the maximum
    _compare_with_nan(got, ij, exp, exp_ij)


@pytest.mark.parametrize('s,angles', [(34, [-3, 0, 3]), (34, list(range(-3, 4))), (20, ANGLES15)])
def test_the_rest_did_not_move(c_oracle, pair, s, angles):
    """Slot-group kernels (3 and 7 angles) and the classic kernel (img_size = 20) keep today's tiling: borders 20 and 26."""
    for shift in (False, True):
        g = _grids([20, 26], shift=shift)
        got, ij, exp, exp_ij = _run(c_oracle, pair[0], pair[1], g, s, angles)
        assert np.isfinite(exp[:, 0]).sum() > 0.9 * exp.shape[0]
        _compare_with_nan(got, ij, exp, exp_ij)
