"""What a reused PM handle remembers between calls (csrc/pm_capi.hip, struct sid_pm_ctx; DESIGN.md "What a handle remembers"):
the spline coefficients of image 1 (valid for a pair and an order), the pre-sampled templates of the resident points (valid for a
pair and a point set), the current pair (two owned slots and a borrowed binding), the results binding, the grow-only buffers and
the launch classes.  A stale item does not crash: it returns a plausible (c2, r2, a, r, h) for the wrong image or the wrong
spline order.  So every step below is checked twice - against the C oracle for the state the handle SHOULD be in
(assert_parity's bar), and bit for bit, h included, against a fresh handle that was given only that state - and every test first
asserts from the oracle alone that the states of its sequence have different answers (a stale answer would otherwise pass).

Every handle under test is created in its test, so the sequence of states it went through is the one written there.
The tests named ``same_shape`` keep every image shape, so a stale buffer is a wrong answer and never an out-of-range read; the
``other_shape`` tests change the shapes (growth and reuse of the coefficient buffers, re-classification, templates beyond a
smaller image 1)."""
import collections

import numpy as np
import pytest
import torch

from oracle import pm_oracle as po
from sea_ice_drift_amd import _capi, pmlib as my, synthetic as syn
from tests.test_gpu_parity import assert_parity

pytestmark = pytest.mark.gpu

ANGLES3 = (-3.0, 0.0, 3.0)
ANGLES7 = (-3.5, -2.5, -1.5, -0.5, 0.5, 1.5, 2.5)                    # (no angle in common with ANGLES3: every template differs)
ORDER_FLAGS = [1 | po.flag_rot_order(o) for o in (0, 1, 3, 5)]       # HES_NORM with rot_order 0, 1, 3, 5
ORDER_IDS = ['order%d' % o for o in (0, 1, 3, 5)]


def flags_of(order):
    return 1 | po.flag_rot_order(order)


# ---------------------------------------------------------------- inputs (built once, read-only)
def _bright(x):
    return (60 + x * 0.6).astype(np.uint8)                           # (brighter: a spline template that dips to 0 is a NaN point)


_PAIRS = {}


def pair(name):
    """A, B: 320 x 300, other pixels.  AZ: A with a zeroed block in image 1.  C: both images of another shape.  C1: image 2
    shaped like A's, image 1 smaller (sid_pm_run does not classify again for it, and some templates leave image 1).
    D: a third image (get_template)."""
    if name not in _PAIRS:
        if name in ('A', 'B'):
            p = [_bright(x) for x in syn.make_pair(320, 300, seed=3 if name == 'A' else 4)]
        elif name == 'AZ':
            p = [x.copy() for x in pair('A')]
            p[0][20:30, 20:30] = 0
        elif name == 'C':
            p = [_bright(x) for x in syn.make_pair(300, 340, seed=5)]
        elif name == 'C1':
            p = [np.ascontiguousarray(pair('B')[0][:200, :220]), pair('B')[1].copy()]
        elif name == 'D':
            p = [_bright(x) for x in syn.make_pair(120, 130, seed=6)]
        for x in p:
            x.setflags(write=False)
        _PAIRS[name] = tuple(p)
    return _PAIRS[name]


def _points(seed, n, large=0):
    """n integral points with borders 20..39 whose windows lie inside a 320 x 300 image 2 for template sides up to 35; point
    `large` sits at (150, 150) with a border of 120 px: beyond one workgroup's LDS, it runs the large-window pipeline, which
    reads the spline coefficients directly."""
    rng = np.random.default_rng(seed)
    c1 = rng.integers(70, 231, n).astype(np.float64)
    r1 = rng.integers(70, 251, n).astype(np.float64)
    dc, dr = syn.true_displacement(c1, r1)
    c2 = c1 + np.rint(dc) + rng.integers(-2, 3, n)
    r2 = r1 + np.rint(dr) + rng.integers(-2, 3, n)
    border = rng.integers(20, 40, n).astype(np.float64)
    if large is not None:
        c1[large] = r1[large] = c2[large] = r2[large] = 150.0
        border[large] = 120.0
    v = (c1, r1, c2, r2, border)
    for x in v:
        x.setflags(write=False)
    return v


def _nan_rows(s):
    """The rows that held finite results now hold: s = 34 - row 0 a window outside image 2, row 1 a template over the zeroed
    block of image 1 (pair AZ); s = 100 - row 0 a point without a valid window (no one-point kernel of that side exists: the
    NaN row is written by the large-window pipeline's lw_write_nan).  The other rows stay valid."""
    v = [x[:5].copy() for x in POINTS['v12']]
    if s == 34:
        v[2][0] = 290.0                                               # c2fg: the window ends beyond column 300 ... and starts inside
        v[3][0] = -30.0                                               # r2fg: ... but above row 0
        v[0][1], v[1][1] = 40.0, 40.0                                 # template rows / columns 23 .. 57: over the block 20 .. 29
    else:
        v = [x[:3].copy() for x in v]
        v[0][:], v[1][:] = [150.0, 120.0, 170.0], [150.0, 160.0, 130.0]
        v[2][:], v[3][:] = [40.0, 125.0, 172.0], [150.0, 158.0, 133.0]   # row 0: the window would start at column -30
        v[4][:] = 20.0
    for x in v:
        x.setflags(write=False)
    return tuple(v)


POINTS = {'v12': _points(101, 12), 'w12': _points(202, 12, large=7), 'v40': _points(303, 40, large=31)}
POINTS['v5'] = tuple(x[:5] for x in POINTS['v12'])                    # (the border-120 point, row 0, stays)
POINTS['nan34'] = _nan_rows(34)
POINTS['nan100'] = _nan_rows(100)

# one state of a handle: the current pair, the resident points, the sweep
State = collections.namedtuple('State', 'pair pts s alpha0 angles flags')


def state(pair_name, flags=1, pts='v12', s=34, alpha0=0.0, angles=ANGLES3):
    return State(pair_name, pts, s, alpha0, tuple(angles), flags)


def rot_of(st):
    return my.rotation_table(st.angles, st.alpha0, st.s)


def set_points(ctx, st):
    ctx.set_points(*POINTS[st.pts], st.s, st.alpha0, list(st.angles), rot=rot_of(st), flags=st.flags)


# ---------------------------------------------------------------- the two references, each computed once per state
_ORACLE, _FRESH = {}, {}


def oracle(st):
    if st not in _ORACLE:
        from oracle import c_oracle as co
        co.build()
        img1, img2 = pair(st.pair)
        exp = co.pm_batch(img1, img2, *POINTS[st.pts], st.s, st.alpha0, list(st.angles), rot=rot_of(st), flags=st.flags, nthreads=8)
        for x in exp:
            x.setflags(write=False)
        _ORACLE[st] = exp
    return _ORACLE[st]


def fresh(st):
    """The state on a handle that has seen nothing else: upload, set_points, run, fetch, close."""
    if st not in _FRESH:
        with _capi.PMContext(0) as ctx:
            ctx.upload_pair(*pair(st.pair))
            set_points(ctx, st)
            ctx.run()
            got = ctx.fetch()
        for x in got:
            x.setflags(write=False)
        _FRESH[st] = got
    return _FRESH[st]


def check_result(got, st, what=''):
    out, ij = got
    exp, exp_ij = oracle(st)
    print('%s %s: %d rows, %d valid' % (what, st, len(exp), int(np.isfinite(exp[:, 0]).sum())))
    assert_parity(out, ij, exp, exp_ij, mcc_norm=bool(st.flags & 4))
    f_out, f_ij = fresh(st)
    np.testing.assert_array_equal(ij, f_ij, err_msg='fresh handle, ' + what)
    np.testing.assert_array_equal(out, f_out, err_msg='fresh handle, ' + what)
    assert out.tobytes() == f_out.tobytes(), 'fresh handle, bit for bit: ' + what


def check(ctx, st, what=''):
    """run() + fetch() on the reused handle, which should be in state `st`."""
    ctx.run()
    got = ctx.fetch()
    check_result(got, st, what)
    return got


def differ(st_a, st_b, every, rows=None, least=6):
    """Precondition, from the oracle alone: r of the two states differs on every row valid in both (other pixels, other points),
    or on at least half of them (another order, other angles or flags)."""
    ea, eb = oracle(st_a)[0], oracle(st_b)[0]
    n = min(len(ea), len(eb)) if rows is None else rows
    ea, eb = ea[:n], eb[:n]
    ok = np.isfinite(ea[:, 3]) & np.isfinite(eb[:, 3])
    d = ea[ok, 3] != eb[ok, 3]
    print('precondition %s | %s: r differs on %d of %d' % (st_a, st_b, int(d.sum()), int(ok.sum())))
    assert ok.sum() >= least
    assert d.all() if every else 2 * d.sum() >= ok.sum()


def all_valid(st):
    assert np.isfinite(oracle(st)[0]).all()


def device_pair(name):
    return tuple(torch.from_numpy(x.copy()).cuda() for x in pair(name))


# ---------------------------------------------------------------- group A: transitions that keep every shape
@pytest.mark.parametrize('flags', ORDER_FLAGS, ids=ORDER_IDS)
def test_same_shape_refresh_in_the_selected_slot(flags):
    """upload_pair(A), then B into the same slot with the C call alone (select=False: no sid_pm_select_pair behind it) - the
    upload itself re-points the current pair and must invalidate the coefficients."""
    a, b = state('A', flags), state('B', flags)
    all_valid(a), all_valid(b)
    differ(a, b, every=True)
    with _capi.PMContext(0) as ctx:
        ctx.upload_pair(*pair('A'))
        set_points(ctx, a)
        check(ctx, a, 'A')
        ctx.upload_pair(*pair('B'), slot=0, select=False)
        check(ctx, b, 'B into the selected slot')
        ctx.upload_pair(*pair('A'), slot=0, select=False)
        check(ctx, a, 'A again')


@pytest.mark.parametrize('flags', ORDER_FLAGS, ids=ORDER_IDS)
def test_same_shape_prefetch_into_the_other_slot(flags):
    a, b = state('A', flags), state('B', flags)
    differ(a, b, every=True)
    with _capi.PMContext(0) as ctx:
        ctx.upload_pair(*pair('A'), slot=0)
        set_points(ctx, a)
        check(ctx, a, 'A in slot 0')
        ctx.upload_pair(*pair('B'), slot=1, select=False)
        check(ctx, a, 'still A: B went into the other slot')
        ctx.select_pair(1)
        check(ctx, b, 'select_pair(1)')
        ctx.select_pair(0)
        check(ctx, a, 'select_pair(0), no upload')
        ctx.select_pair(1)
        check(ctx, b, 'select_pair(1) again')


@pytest.mark.parametrize('flags', ORDER_FLAGS, ids=ORDER_IDS)
def test_same_shape_borrowed_bindings(flags):
    a, b = state('A', flags), state('B', flags)
    differ(a, b, every=True)
    ta, tb = device_pair('A'), device_pair('B')
    with _capi.PMContext(0) as ctx:
        ctx.bind_pair_tensors(*ta)
        set_points(ctx, a)
        check(ctx, a, 'tensors of A')
        ctx.bind_pair_tensors(*tb)
        check(ctx, b, 'other tensors, holding B')
        ctx.upload_pair(*pair('A'), slot=0, select=False)             # (an upload replaces a borrowed binding: sid_pm_upload_pair)
        check(ctx, a, 'upload_pair(A) while the binding was current')
        ctx.bind_pair_tensors(*tb)
        check(ctx, b, 'B bound again')


@pytest.mark.parametrize('flags', ORDER_FLAGS, ids=ORDER_IDS)
def test_same_shape_in_place_change_of_a_borrowed_pair(flags):
    """The contract of include/sid_pm.h sid_pm_bind_pair: orders 0 and 1 read the pixels at every run; orders 2..5 keep the
    coefficients and templates of the first run after the bind, and binding the same tensors again makes the next run compute
    them anew.  (What orders 2..5 return WITHOUT the second bind is not asserted: it is the documented stale case.)"""
    a, b = state('A', flags), state('B', flags)
    differ(a, b, every=True)
    t1, t2 = device_pair('A')
    u1, u2 = device_pair('B')
    with _capi.PMContext(0) as ctx:
        ctx.bind_pair_tensors(t1, t2)
        set_points(ctx, a)
        check(ctx, a, 'tensors holding A')
        t1.copy_(u1)
        t2.copy_(u2)
        torch.cuda.synchronize()
        if po.rot_order_of(flags) >= 2:
            ctx.bind_pair_tensors(t1, t2)
        check(ctx, b, 'the same tensors, overwritten with B')


@pytest.mark.parametrize('flags', ORDER_FLAGS, ids=ORDER_IDS)
def test_same_shape_an_owned_slot_is_a_snapshot(flags):
    a, b = state('A', flags), state('B', flags)
    differ(a, b, every=True)
    h1, h2 = [x.copy() for x in pair('A')]
    with _capi.PMContext(0) as ctx:
        ctx.upload_pair(h1, h2)
        set_points(ctx, a)
        check(ctx, a, 'uploaded from arrays of the test')
        h1[...] = pair('B')[0]
        h2[...] = pair('B')[1]
        check(ctx, a, 'the host arrays now hold B: the slot still holds A')
        set_points(ctx, a)
        check(ctx, a, 'and after set_points')


def test_same_shape_order_change_on_an_unchanged_pair():
    """set_points with the same vectors and another order: coefficients of the other order, templates sampled anew."""
    orders = (3, 2, 5, 0, 3)
    for o, p in zip(orders[1:], orders[:-1]):
        differ(state('A', flags_of(p)), state('A', flags_of(o)), every=False)
    with _capi.PMContext(0) as ctx:
        ctx.upload_pair(*pair('A'))
        for o in orders:
            st = state('A', flags_of(o))
            set_points(ctx, st)
            check(ctx, st, 'order %d' % o)
            check(ctx, st, 'order %d, second run' % o)


def test_same_shape_sweep_change_at_order_3():
    f3 = flags_of(3)
    seq = [state('A', f3), state('A', f3, angles=ANGLES7), state('A', f3),                      # angles 3 -> 7 -> 3
           state('A', f3, alpha0=-3.85), state('A', f3),                                        # alpha0 0 -> -3.85 (-> 0)
           state('A', f3, s=35, angles=ANGLES7), state('A', f3, s=21), state('A', f3),          # side 34 -> 35 -> 21 -> 34
           state('A', 7 | po.flag_rot_order(3))]                                                # flags 1 -> 7
    for p, q in zip(seq[:-1], seq[1:]):
        differ(p, q, every=False)
    with _capi.PMContext(0) as ctx:
        ctx.upload_pair(*pair('A'))
        for k, st in enumerate(seq):
            set_points(ctx, st)
            check(ctx, st, 'step %d' % k)


@pytest.mark.parametrize('order', [3, 0])
def test_same_shape_point_set_change(order):
    """Fewer points, other points, more points than ever before (arena, out and pre grow), then sets whose leading rows - which
    held finite results - are NaN points of every kind: NaN x 5 and ij = -1 there."""
    f = flags_of(order)
    st = {p: state('AZ', f, pts=p) for p in ('v12', 'v5', 'w12', 'v40', 'nan34')}
    st['nan100'] = state('AZ', f, pts='nan100', s=100)
    for p in ('v12', 'v5', 'w12', 'v40'):
        all_valid(st[p])
    differ(st['v5'], st['w12'], every=True, least=5)                 # other points in the rows the five held
    differ(st['w12'], st['v40'], every=True)
    nan_rows = {'nan34': 2, 'nan100': 1}
    for p, k in nan_rows.items():
        exp, exp_ij = oracle(st[p])
        assert np.isnan(exp[:k]).all() and (exp_ij[:k] == -1).all() and np.isfinite(exp[k:]).all()
    with _capi.PMContext(0) as ctx:
        ctx.upload_pair(*pair('AZ'))
        for p in ('v12', 'v5', 'w12', 'v40', 'nan34', 'v40', 'nan100', 'v12'):   # (forty finite rows before each NaN set)
            set_points(ctx, st[p])
            out, ij = check(ctx, st[p], p)
            k = nan_rows.get(p, 0)
            assert np.isnan(out[:k]).all() and (ij[:k] == -1).all() and np.isfinite(out[k:]).all()


def assert_single(d, exp, what):
    """rotate_and_match against the C oracle: peak and angle index, dc, dr, a, r and the whole matrix and template exact; h to 1e-5."""
    print(what, d['out'], exp['out'])
    np.testing.assert_array_equal(d['ij'], exp['ij'], err_msg=what)
    assert exp['ij'][2] >= 0
    np.testing.assert_array_equal(d['out'][:4], exp['out'][:4], err_msg=what)
    np.testing.assert_allclose(d['out'][4], exp['out'][4], rtol=1e-5, atol=1e-5, err_msg=what)
    np.testing.assert_array_equal(d['ccm'], exp['ccm'], err_msg=what)
    np.testing.assert_array_equal(d['template'], exp['template'], err_msg=what)


def single(ctx, co, name, c1, r1, s, angles, order, window):
    """ctx.rotate_and_match on the handle's current pair and the oracle's answer for pair `name`."""
    r0, c0, wh, ww = window
    img1, img2 = pair(name)
    rot = my.rotation_table(angles, 0.0, s)
    d = ctx.rotate_and_match(c1, r1, s, 0.0, list(angles), rot=rot, flags=flags_of(order), window=window)
    exp = co.rotate_and_match(img1, c1, r1, s, np.ascontiguousarray(img2[r0:r0 + wh, c0:c0 + ww]), 0.0, list(angles), rot, flags=flags_of(order))
    return d, exp


def test_same_shape_single_point_calls_between_runs(c_oracle):
    """sid_pm_rotate_and_match and sid_pm_debug_point compute coefficients of THEIR order on the handle the resident points
    share: each must get its own order's, and the resident order-3 points theirs again at the next run()."""
    a3, b3 = state('A', flags_of(3)), state('B', flags_of(3))
    differ(a3, b3, every=True)
    differ(a3, state('A', flags_of(2)), every=False)
    differ(a3, state('A', flags_of(5)), every=False)
    with _capi.PMContext(0) as ctx:
        ctx.upload_pair(*pair('B'), slot=1, select=False)
        ctx.upload_pair(*pair('A'), slot=0)
        set_points(ctx, a3)
        first = check(ctx, a3, 'order 3 resident')
        # 1. order 2 through rotate_and_match
        d, exp = single(ctx, c_oracle, 'A', 140.25, 160.5, 34, ANGLES3, 2, (100, 90, 110, 120))
        assert_single(d, exp, 'rotate_and_match, order 2')
        d3, exp3 = single(ctx, c_oracle, 'A', 140.25, 160.5, 34, ANGLES3, 3, (100, 90, 110, 120))
        assert exp3['out'][3] != exp['out'][3]                        # (the orders have different answers here)
        assert_single(d3, exp3, 'rotate_and_match, order 3')
        d, exp = single(ctx, c_oracle, 'A', 140.25, 160.5, 34, ANGLES3, 2, (100, 90, 110, 120))
        assert_single(d, exp, 'rotate_and_match, order 2 after order 3')
        # 2. the resident points, no set_points
        got = check(ctx, a3, 'run() after rotate_and_match at order 2')
        assert got[0].tobytes() == first[0].tobytes()
        # 3. order 5 through debug_point
        angles = [-9.0, 0.0, 1.234]
        dbg = ctx.debug_point(151.3, 139.7, 150.0, 140.0, 20.0, 34, 0.0, angles, flags=flags_of(5))
        coeffs = po.spline_coefficients(pair('A')[0], 5)
        t3 = po.get_template_spline(pair('A')[0], 151.3, 139.7, 0.0, 34, 3)
        for k, ang in enumerate(angles):
            t5 = po.get_template_spline(pair('A')[0], 151.3, 139.7, ang, 34, 5, coeffs=coeffs)
            np.testing.assert_array_equal(dbg['templates'][k], t5, err_msg='debug_point, order 5, angle %r' % ang)
        assert (po.get_template_spline(pair('A')[0], 151.3, 139.7, 0.0, 34, 5, coeffs=coeffs) != t3).any()
        got = check(ctx, a3, 'run() after debug_point at order 5')
        assert got[0].tobytes() == first[0].tobytes()
        # 4. forty angles on a 200 x 180 window: lw_small and the large-window scratch grow, the border-120 point shares them
        forty = [0.25 * k for k in range(-20, 20)]
        d, exp = single(ctx, c_oracle, 'A', 150.0, 155.0, 34, forty, 3, (60, 70, 200, 180))
        assert_single(d, exp, 'rotate_and_match, 40 angles, 200 x 180')
        got = check(ctx, a3, 'run() after the scratch grew')
        assert got[0].tobytes() == first[0].tobytes()
        # 5. the other slot: B's coefficients
        ctx.select_pair(1)
        d, exp = single(ctx, c_oracle, 'B', 140.25, 160.5, 34, ANGLES3, 3, (100, 90, 110, 120))
        assert exp['out'][3] != exp3['out'][3]
        assert_single(d, exp, 'rotate_and_match, order 3, after select_pair')
        check(ctx, b3, 'run() on B')


def test_same_shape_results_binding():
    """bind_results_host: the kernels write into the pinned tensors; the next set_points drops the binding, so the old tensors
    are never written again and fetch() reads the handle's own arrays."""
    a, w = state('A', flags_of(3)), state('A', flags_of(3), pts='w12')
    differ(a, w, every=True)
    sentinel = -12345.5
    with _capi.PMContext(0) as ctx:
        ctx.upload_pair(*pair('A'))
        set_points(ctx, a)
        unbound = check(ctx, a, 'unbound')
        out, ij = ctx.bind_results_host()
        out.fill_(sentinel)
        ij.fill_(-7)
        ctx.run()
        ctx.sync()
        check_result((out.numpy().copy(), ij.numpy().copy()), a, 'pinned tensors')
        assert out.numpy().tobytes() == unbound[0].tobytes() and (ij.numpy() == unbound[1]).all()
        set_points(ctx, w)                                            # (as many points: the old tensors could hold them)
        out.fill_(sentinel)
        ij.fill_(-7)
        ctx.run()
        ctx.sync()
        assert (out.numpy() == sentinel).all() and (ij.numpy() == -7).all(), 'a run after set_points wrote into the tensors of the dropped binding'
        check_result(ctx.fetch(), w, 'fetch() after the binding was dropped')
        assert (out.numpy() == sentinel).all() and (ij.numpy() == -7).all()


def assert_use_mcc(got, st, i):
    exp = oracle(st)[0][i]
    print('use_mcc', got, exp)
    assert got[:3] == tuple(exp[:3]) and isinstance(got[3], np.float32) and np.float64(got[3]) == exp[3]
    np.testing.assert_allclose(got[4], exp[4], rtol=1e-5, atol=1e-5)


def test_same_shape_public_calls_on_the_shared_handle(c_oracle):
    """use_mcc, rotate_and_match and get_template of pmlib on the per-device handle they share, one after the other with other
    images and other orders: each result is the oracle's for its own arguments."""
    a3, b3 = state('A', flags_of(3)), state('B', flags_of(3))
    differ(a3, b3, every=True)
    i = 3
    v = [x[i] for x in POINTS['v12']]
    h1, h2 = [x.copy() for x in pair('A')]
    assert_use_mcc(my.use_mcc(*v, h1, h2, 34, 0.0, angles=list(ANGLES3), rot_order=3), a3, i)
    b1, b2 = pair('B')
    win = np.ascontiguousarray(b2[100:210, 90:210])
    got = my.rotate_and_match(b1, 140.25, 160.5, 34, win, 0.0, angles=list(ANGLES3), rot_order=2)
    exp = c_oracle.rotate_and_match(b1, 140.25, 160.5, 34, win, 0.0, list(ANGLES3), my.rotation_table(ANGLES3, 0.0, 34), flags=flags_of(2))
    assert exp['ij'][2] >= 0
    assert (got[0], got[1], got[2]) == tuple(exp['out'][:3]) and np.float64(got[3]) == exp['out'][3]
    np.testing.assert_allclose(got[4], exp['out'][4], rtol=1e-5, atol=1e-5)
    np.testing.assert_array_equal(got[5], exp['ccm'])
    np.testing.assert_array_equal(got[6], exp['template'])
    d = pair('D')[0]
    np.testing.assert_array_equal(my.get_template(d, 60.3, 55.7, 1.234, 34, rot_order=5), po.get_template_spline(d, 60.3, 55.7, 1.234, 34, 5))
    h1[...] = b1                                                      # A's ndarrays, overwritten in place with B
    h2[...] = b2
    assert_use_mcc(my.use_mcc(*v, h1, h2, 34, 0.0, angles=list(ANGLES3), rot_order=3), b3, i)


# ---------------------------------------------------------------- rotate_and_match(window=None)
def test_rotate_and_match_window_none_is_the_whole_of_image_2_of_the_current_pair(c_oracle):
    """window=None = the whole of image 2 of the pair that is current: the wrapper follows uploads into either slot,
    select_pair and bindings.  Each against the explicit whole-image window (everything bit for bit) and the oracle."""
    rot = my.rotation_table(ANGLES3, 0.0, 34)
    exp = {}

    def both(ctx, name, what):
        img1, img2 = pair(name)
        if name not in exp:
            exp[name] = c_oracle.rotate_and_match(img1, 120.0, 110.0, 34, img2, 0.0, list(ANGLES3), rot)
        d = ctx.rotate_and_match(120.0, 110.0, 34, 0.0, list(ANGLES3), rot=rot)
        e = ctx.rotate_and_match(120.0, 110.0, 34, 0.0, list(ANGLES3), rot=rot, window=(0, 0) + img2.shape)
        assert d['ccm'].shape == (img2.shape[0] - 33, img2.shape[1] - 33), what
        for k in ('out', 'ij', 'ccm', 'template'):
            np.testing.assert_array_equal(d[k], e[k], err_msg=what)
        assert_single(d, exp[name], what)

    with _capi.PMContext(0) as ctx:
        with pytest.raises(ValueError):
            ctx.rotate_and_match(120.0, 110.0, 34, 0.0, list(ANGLES3), rot=rot)
        ctx.upload_pair(*pair('A'))
        both(ctx, 'A', 'A in slot 0')
        ctx.upload_pair(*pair('C'), slot=1, select=False)
        both(ctx, 'A', 'C went into the other slot')
        ctx.select_pair(1)
        both(ctx, 'C', 'select_pair(1)')
        ctx.select_pair(0)
        both(ctx, 'A', 'select_pair(0)')
        t = device_pair('C1')
        ctx.bind_pair_tensors(*t)
        both(ctx, 'C1', 'borrowed binding')
        ctx.upload_pair(*pair('C'), slot=1, select=False)
        both(ctx, 'C', 'an upload replaces the binding')


# ---------------------------------------------------------------- group B: transitions that change the shapes
@pytest.mark.parametrize('how', ['upload_pair', 'bind_pair_tensors'])
@pytest.mark.parametrize('order', [0, 3])
def test_other_shape_pairs_on_one_handle(order, how):
    """A -> C -> A -> C1: the coefficient buffers grow and are reused for a smaller image, the points are classified again for
    C's image 2 (and not for C1's, whose image 2 has A's shape), and C1's smaller image 1 cuts templates that were valid."""
    f = flags_of(order)
    seq = [state(n, f) for n in ('A', 'C', 'A', 'C1')]
    for p, q in zip(seq[:-1], seq[1:]):
        differ(p, q, every=True, least=4)
    ea, e1 = oracle(seq[0])[0], oracle(seq[3])[0]
    lost = np.isfinite(ea[:, 0]) & np.isnan(e1[:, 0])
    assert lost.sum() >= 1 and np.isfinite(e1[:, 0]).sum() >= 4
    tensors = {n: device_pair(n) for n in ('A', 'C', 'C1')} if how == 'bind_pair_tensors' else None
    with _capi.PMContext(0) as ctx:
        for k, st in enumerate(seq):
            if tensors:
                ctx.bind_pair_tensors(*tensors[st.pair])
            else:
                ctx.upload_pair(*pair(st.pair))
            if k == 0:
                set_points(ctx, st)
            check(ctx, st, '%s of %s' % (how, st.pair))
