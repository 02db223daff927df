"""The key-point detector (csrc/orb.hip) where tests/test_orb.py does not reach: pyramids that thin out or vanish, every
parameter at both ends of its range, images across the 256-wide blocks and the 16-row tiles, strided images, a binding
max_out, equal responses on either side of the selection buffer (the overflow fallback), one workspace reused across sizes,
and the argument checks.  Every case runs three ways - the NumPy oracle (pinned on its own by tests/test_orb_oracle_props.py),
the device route and the host route (SID_ORB_HOST_SELECT=1) - and all outputs are compared for bit equality: the arithmetic
is integer, there is no tolerance.  Each case also asserts from the oracle alone that it is the case it claims to be."""
import collections
import ctypes as C
import functools

import numpy as np
import pytest

from oracle import orb_oracle as oo
from sea_ice_drift_amd import orb, synthetic as syn

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_NODEVICE = -1, -5                                         # include/sid_pm.h
SENT, N_SENT = 0xA5, -77777
DEFAULTS = dict(edge_threshold=34, n_features=100000, n_levels=7, patch_size=34, fast_threshold=20, scale_factor=1.2)


# ---- images, by a hashable key (so that the oracle's results are computed once and shared) ----
def _synth(rows=300, cols=280):
    return syn.make_pair(300, 280, seed=5)[0][:rows, :cols]


def _noise(rows, cols, seed):
    return np.random.default_rng(seed).integers(0, 256, (rows, cols)).astype(np.uint8)


def _bw(rows, cols, seed):
    return (np.random.default_rng(seed).integers(0, 2, (rows, cols)) * 255).astype(np.uint8)


def _flat(rows, cols):
    return np.full((rows, cols), 7, dtype=np.uint8)


def _dots(n):
    img = np.full((n, n), 10, dtype=np.uint8)
    img[::4, ::4] = 250                                                # every dot: a strict FAST maximum, one Harris response for all
    return img


def _lattice():
    img = np.full((600, 600), 90, dtype=np.uint8)
    img[::40, :] = 200
    img[:, ::40] = 200                                                 # (the lattice of tests/test_orb.py: plateaus of equal responses)
    return img


_MAKERS = dict(synth=_synth, noise=_noise, bw=_bw, flat=_flat, dots=_dots, lattice=_lattice)
SYN = ('synth',)


@functools.lru_cache(maxsize=None)
def get_image(key):
    img = np.ascontiguousarray(_MAKERS[key[0]](*key[1:]))
    img.setflags(write=False)
    return img


@functools.lru_cache(maxsize=None)
def _oracle(key, kw_items):
    out = oo.detect_and_compute(get_image(key), orb.rotated_pattern(), orb.direction_table(), **dict(kw_items))
    for a in out:
        a.setflags(write=False)
    return out


def oracle(key, **kw):
    """-> xy float32 [N, 2], meta int32 [N, 4], response int64 [N], desc uint8 [N, 32]; computed once per case."""
    return _oracle(key, tuple(sorted(kw.items())))


@functools.lru_cache(maxsize=None)
def _candidates(key, e, t, n_levels, scale):
    img = get_image(key)
    _, lr, lc, _ = oo.level_geometry(img.shape[0], img.shape[1], n_levels, scale, 0)
    cands = []
    for l in range(n_levels):
        if lr[l] <= 2 * e or lc[l] <= 2 * e:
            cands.append(None)
            continue
        lvl = img if l == 0 else oo.resize(img, lr[l], lc[l])
        cands.append(oo.candidates(lvl, oo.fast_score(lvl, e, t), e))
    return cands


def levels(key, **kw):
    """The oracle's view of a case: (share of every level, (xs, ys, response) of every level's candidates - None for a level
    that is too small to run)."""
    kw = dict(DEFAULTS, **kw)
    img = get_image(key)
    want = oo.level_geometry(img.shape[0], img.shape[1], kw['n_levels'], kw['scale_factor'], kw['n_features'])[3]
    return want, _candidates(key, kw['edge_threshold'], kw['fast_threshold'], kw['n_levels'], kw['scale_factor'])


def counts(key, **kw):
    return [None if c is None else len(c[0]) for c in levels(key, **kw)[1]]


# ---- the two helpers ----
NAMES = ('xy', 'meta', 'response', 'desc')


def assert_same(got, exp, what):
    """got, exp: (xy, meta, response, desc)."""
    assert len(got[0]) == len(exp[0]), '%s: %d key points, the oracle has %d' % (what, len(got[0]), len(exp[0]))
    for name, g, e in zip(NAMES, got, exp):
        assert g.dtype == e.dtype and g.shape == e.shape, (what, name, g.dtype, g.shape, e.shape)
        if not np.array_equal(g, e):
            k = int(np.nonzero((g != e).reshape(len(g), -1).any(axis=1))[0][0])
            raise AssertionError('%s: %s differs first at row %d (level %d): got %s, the oracle %s'
                                 % (what, name, k, int(exp[1][k, 2]), g[k].tolist(), e[k].tolist()))


def run_three_ways(monkeypatch, key, **kw):
    """Oracle, device route, host route: xy, meta, response and desc equal among all three.  Returns the oracle's."""
    img = get_image(key)
    exp = oracle(key, **kw)
    for route in ('device', 'host'):
        if route == 'host':
            monkeypatch.setenv('SID_ORB_HOST_SELECT', '1')
        else:
            monkeypatch.delenv('SID_ORB_HOST_SELECT', raising=False)
        xy, desc, meta, resp = orb.detect_and_compute(img, full=True, **kw)
        monkeypatch.delenv('SID_ORB_HOST_SELECT', raising=False)
        assert xy.dtype == np.float64
        assert_same((xy.astype(np.float32), meta, resp, desc), exp, '%s route' % route)
    return exp


Direct = collections.namedtuple('Direct', 'rc n_out xy meta response desc err')
_WIDTH = dict(xy=8, meta=16, response=8, desc=32)                      # bytes per key point


def direct(img, rows=None, cols=None, stride=None, max_out=None, meta=True, response=True, xy=True, device=0, **kw):
    """sid_orb_detect itself: the caller's stride and max_out, NULL for meta / response / xy on request, output buffers of
    max_out + 4 rows pre-filled with a sentinel, a sentinel in n_out.  The buffers come back as raw bytes [rows, width]."""
    from sea_ice_drift_amd import _capi
    L = _capi.lib()
    p = dict(DEFAULTS, **kw)
    rows = img.shape[0] if rows is None else rows
    cols = img.shape[1] if cols is None else cols
    stride = img.strides[0] if stride is None else stride
    assert img.dtype == np.uint8 and img.strides[1] == 1
    max_out = p['n_features'] if max_out is None else max_out
    bufs = {name: np.full((max(max_out, 0) + 4, w), SENT, dtype=np.uint8) for name, w in _WIDTH.items()}
    n = C.c_int64(N_SENT)
    par = orb.OrbParams(p['edge_threshold'], p['n_features'], p['n_levels'], p['patch_size'], p['fast_threshold'], p['scale_factor'])
    pat, dirs = np.ascontiguousarray(orb.rotated_pattern()), np.ascontiguousarray(orb.direction_table())

    def ptr(name, ctype, wanted):
        return bufs[name].ctypes.data_as(C.POINTER(ctype)) if wanted else None

    rc = L.sid_orb_detect(device, img.ctypes.data_as(C.POINTER(C.c_uint8)), rows, cols, stride, C.byref(par),
                          pat.ctypes.data_as(C.POINTER(C.c_int8)), dirs.ctypes.data_as(C.POINTER(C.c_int32)),
                          ptr('xy', C.c_float, xy), ptr('meta', C.c_int32, meta), ptr('response', C.c_int64, response),
                          ptr('desc', C.c_uint8, True), max_out, C.byref(n))
    err = L.sid_orb_last_error().decode() if rc != 0 else ''
    return Direct(rc, int(n.value), bufs['xy'], bufs['meta'], bufs['response'], bufs['desc'], err)


def assert_direct_prefix(res, exp, n, what, meta=True, response=True):
    """The first n rows of the outputs are the first n of exp; the sentinel survives everywhere else."""
    assert res.rc == 0, (what, res.rc, res.err)
    assert res.n_out == n, '%s: n_out = %d, expected %d' % (what, res.n_out, n)
    got = (res.xy[:n].view(np.float32), res.meta[:n].view(np.int32), res.response[:n].view(np.int64).reshape(n), res.desc[:n])
    for name, g, e, given in zip(NAMES, got, exp, (True, meta, response, True)):
        raw = getattr(res, name)
        if given:
            assert np.array_equal(g, e[:n]), '%s: %s is not the first %d rows of the uncapped result' % (what, name, n)
            assert (raw[n:] == SENT).all(), '%s: %s was written past row %d' % (what, name, n)
        else:
            assert (raw == SENT).all()


def both_routes(monkeypatch):
    for route in ('device', 'host'):
        if route == 'host':
            monkeypatch.setenv('SID_ORB_HOST_SELECT', '1')
        else:
            monkeypatch.delenv('SID_ORB_HOST_SELECT', raising=False)
        yield route
    monkeypatch.delenv('SID_ORB_HOST_SELECT', raising=False)


# ---- small pyramids and parameters: (key, kw, what the oracle must say about the case) ----
def _seven_levels(exp, want, n):
    assert sorted(set(exp[1][:, 2].tolist())) == list(range(7))        # all 7 levels contribute
    assert n[0] > want[0] and 0 < n[6] < want[6]                       # level 0 is cut to its share, the last one falls short of it
    assert len(exp[0]) < 2000


def _thins_to_one(exp, want, n):
    assert (exp[1][:, 2] == 7).sum() == 1 and n[7] is not None and (exp[1][:, 2] == 0).sum() > 10


def _one_pixel(exp, want, n):
    assert n == [1] and exp[1].tolist()[0][:3] == [34, 34, 0]          # 69 - 2 * 34 = 1 admissible pixel, and it is a corner


def _no_level_runs(exp, want, n):
    assert all(c is None for c in n) and len(exp[0]) == 0


def _nothing_wanted(exp, want, n):
    assert n[0] > 0 and sum(want) == 0 and len(exp[0]) == 0


def _all_levels(n_levels):
    def check(exp, want, n):
        assert sorted(set(exp[1][:, 2].tolist())) == list(range(n_levels)) and len(set(exp[1][:, 3].tolist())) > 4
    return check


def _some(exp, want, n):
    assert len(exp[0]) > 20 and len(set(exp[1][:, 3].tolist())) > 4   # key points, in several directions


def _black_and_white(exp, want, n):
    # steps of 255 pass the highest thresholds at level 0; the resampled levels run and have nothing that steep
    assert n[0] > 50 and len(exp[0]) > 50 and (exp[1][:, 2] == 0).all()
    assert sum(c is not None for c in n) > 3 and all(c == 0 for c in n[1:] if c is not None)


def _levels_run_empty(exp, want, n):
    assert all(c == 0 for c in n) and len(exp[0]) == 0


def _fewer_than_wanted_everywhere(exp, want, n):
    assert all(0 < c < w for c, w in zip(n, want)) and len(exp[0]) == sum(n) > 1000


def _two_admissible(axis):
    def check(exp, want, n):
        assert n[0] > 0 and n[1] is None and len(exp[0]) == min(n[0], want[0])
        assert set(exp[1][:, axis].tolist()) <= {34, 35}               # 70 - 2 * 34 = 2 admissible columns (rows)
        assert exp[1][:, 1 - axis].max() > 3000                        # and key points in the last blocks / tiles
    return check


def _two_levels(exp, want, n):
    assert n[0] > 0 and n[1] is not None and n[1] > 0 and set(exp[1][:, 2].tolist()) == {0, 1}


CASES = {
    # small pyramids
    'seven-levels': (SYN, dict(n_levels=7, n_features=2000), _seven_levels),
    'thins-to-one': (('synth', 120, 131), dict(edge_threshold=16, patch_size=30, n_levels=8, n_features=2000), _thins_to_one),
    'one-pixel': (('synth', 69, 69), dict(n_levels=1, fast_threshold=1, n_features=2000), _one_pixel),
    'too-low': (('synth', 68, 200), dict(n_features=2000), _no_level_runs),
    '1x1': (('flat', 1, 1), dict(n_features=2000), _no_level_runs),
    '1x500': (('noise', 1, 500, 11), dict(n_features=2000), _no_level_runs),
    'n_features=0': (SYN, dict(n_features=0), _nothing_wanted),
    # parameters at the ends of their ranges
    'scale-2': (SYN, dict(scale_factor=2.0, edge_threshold=20, patch_size=31, n_levels=3, n_features=2000), _all_levels(3)),
    'scale-1.05': (SYN, dict(scale_factor=1.05, n_levels=16, fast_threshold=5, n_features=3000), _all_levels(16)),
    'patch-2': (SYN, dict(patch_size=2, edge_threshold=16, n_features=2000), _some),
    'patch-200': (('noise', 330, 340, 12), dict(patch_size=200, edge_threshold=101, n_levels=3, n_features=500), _some),
    'fast-254-bw': (('bw', 200, 333, 13), dict(fast_threshold=254, n_features=2000), _black_and_white),
    'fast-253-bw': (('bw', 200, 333, 13), dict(fast_threshold=253, n_features=2000), _black_and_white),
    'fast-254-synth': (SYN, dict(fast_threshold=254, n_features=2000), _levels_run_empty),
    # more features than candidates at every level
    'all-candidates': (('noise', 200, 333, 14), dict(n_features=100000, n_levels=4, fast_threshold=1), _fewer_than_wanted_everywhere),
    # across the 256-wide blocks and the 16-row tiles of non-maximum suppression
    '70x4001': (('noise', 70, 4001, 15), dict(n_levels=2, n_features=2000), _two_admissible(1)),
    '4001x70': (('noise', 4001, 70, 16), dict(n_levels=2, n_features=2000), _two_admissible(0)),
    'w255': (('noise', 100, 255, 17), dict(n_levels=2, n_features=1000), _two_levels),
    'w256': (('noise', 100, 256, 17), dict(n_levels=2, n_features=1000), _two_levels),
    'w257': (('noise', 100, 257, 17), dict(n_levels=2, n_features=1000), _two_levels),
    'h83': (('noise', 2 * 34 + 15, 300, 18), dict(n_levels=2, n_features=1000), _two_levels),
    'h84': (('noise', 2 * 34 + 16, 300, 18), dict(n_levels=2, n_features=1000), _two_levels),
    'h85': (('noise', 2 * 34 + 17, 300, 18), dict(n_levels=2, n_features=1000), _two_levels),
}


@pytest.mark.parametrize('name', list(CASES))
def test_case_equals_the_oracle_on_both_routes(monkeypatch, name):
    key, kw, claim = CASES[name]
    exp = oracle(key, **kw)
    claim(exp, levels(key, **kw)[0], counts(key, **kw))
    run_three_ways(monkeypatch, key, **kw)


def test_n_features_bounds_the_key_points_when_max_out_does_not(monkeypatch):
    """The rounded level shares of OpenCV's split can add up to more than n_features (1 + 1 + 1 + 1 for n_features = 3 on 5
    levels of scale 1.05).  n_features is an upper bound (include/sid_orb.h) and the device buffers are sized by it: a share
    is capped by what the levels before it left.  Before that cap, a caller with max_out > n_features got 4 key points here."""
    kw = dict(n_features=3, n_levels=5, scale_factor=1.05)
    s, rounded = float(np.float32(1.05)), []
    nd = 3 * (1.0 - 1.0 / s) / (1.0 - (1.0 / s) ** 5)
    for _ in range(4):
        rounded.append(int(np.floor(nd + 0.5)))
        nd /= s
    assert sum(rounded) > 3 and all(c > 1 for c in counts(SYN, **kw))  # the plain rounding oversubscribes, every level could deliver
    exp = oracle(SYN, **kw)
    assert len(exp[0]) == 3
    for route in both_routes(monkeypatch):
        assert_direct_prefix(direct(get_image(SYN), max_out=10, **kw), exp, 3, route)
    run_three_ways(monkeypatch, SYN, **kw)


# ---- strides ----
def test_strided_images_equal_their_contiguous_copy(monkeypatch):
    big = _noise(260, 350, 21)
    view = big[5:205, 7:307]
    flat = np.ascontiguousarray(view)
    kw = dict(n_levels=3, n_features=1500)
    exp = oo.detect_and_compute(flat, orb.rotated_pattern(), orb.direction_table(), **kw)
    assert len(exp[0]) > 200 and view.strides == (350, 1)
    padded = _noise(200, 300 + 37, 22)                                 # other noise between the rows: a wrong stride shows
    padded[:, :300] = flat
    wide = _noise(200, 600, 23)
    wide[:, ::2] = flat
    assert wide[:, ::2].strides == (600, 2)
    for route in both_routes(monkeypatch):
        for what, img in (('contiguous', flat), ('row stride 350', view), ('column stride 2', wide[:, ::2])):
            xy, desc, meta, resp = orb.detect_and_compute(img, full=True, **kw)
            assert_same((xy.astype(np.float32), meta, resp, desc), exp, '%s, %s route' % (what, route))
        res = direct(padded, cols=300, stride=337, **kw)
        assert_direct_prefix(res, exp, len(exp[0]), 'stride = cols + 37, %s route' % route)


# ---- max_out ----
def test_max_out_keeps_a_prefix(monkeypatch):
    """Key points are ordered by level and best first within a level, so a cap by max_out keeps a prefix of the uncapped list:
    inside level 0, at its end, inside later levels, one short of everything, exactly everything, and more."""
    kw = dict(n_levels=7, n_features=2000)
    img, exp = get_image(SYN), oracle(SYN, **kw)
    N, w0 = len(exp[0]), levels(SYN, **kw)[0][0]
    assert (exp[1][:, 2] == 0).sum() == w0 and 2 < w0 and w0 + 2 < N < 2000 - 5   # level 0 is full; every cap below is a strict prefix
    for route in both_routes(monkeypatch):
        for m in (0, 1, w0 - 1, w0, w0 + 1, N - 1, N, N + 5):
            assert_direct_prefix(direct(img, max_out=m, **kw), exp, min(m, N), 'max_out = %d, %s route' % (m, route))
        for m in (w0 + 1, N + 5):
            res = direct(img, max_out=m, meta=False, response=False, **kw)
            assert_direct_prefix(res, exp, min(m, N), 'max_out = %d without meta and response, %s route' % (m, route), meta=False, response=False)


# ---- ties and the overflow fallback ----
def _selection(key, level, **kw):
    """What the selection of a level meets: (keep, candidates tied at the response of rank keep, candidates that the radix pick
    of that rank keeps - those whose float32 response is not below it)."""
    want, cands = levels(key, **kw)
    resp = cands[level][2]
    keep = min(want[level], len(resp))
    r_keep = np.sort(resp)[::-1][keep - 1]
    return keep, int((resp == r_keep).sum()), int((resp.astype(np.float32) >= np.float32(r_keep)).sum())


@pytest.mark.parametrize('n_features,overflows', [(1, True), (5000, False)])
def test_equal_responses_on_either_side_of_the_selection_buffer(monkeypatch, n_features, overflows):
    """283^2 = 80089 dots with one response.  The selection buffer of orb.hip holds sel_cap = 4 n_features + 65536 candidates:
    with n_features = 1 the tie does not fit, the device route raises DState::flags and the call is repeated on the host
    route, which orders all candidates ("massive ties"); with n_features = 5000 it fits and the device orders it.  Either way
    the key points are the first in (y, x) order."""
    key, kw = ('dots', 1200), dict(n_levels=1, n_features=n_features)
    sel_cap = 65536 + 4 * n_features
    xs, ys, resp = levels(key, **kw)[1][0]
    assert len(set(resp.tolist())) == 1
    keep, tied, kept = _selection(key, 0, **kw)
    assert keep == n_features
    if overflows:
        assert tied > sel_cap, 'sel_cap has changed: this case no longer overflows the selection buffer'
    else:
        assert keep < tied <= kept <= sel_cap, 'sel_cap has changed: this case no longer fits the selection buffer'
    exp = run_three_ways(monkeypatch, key, **kw)
    first = np.lexsort((xs, ys))[:n_features]
    assert exp[1][:, 0].tolist() == xs[first].tolist() and exp[1][:, 1].tolist() == ys[first].tolist()
    assert exp[1][0, :2].tolist() == [36, 36] and len(exp[0]) == n_features


@pytest.mark.parametrize('n_features,cut', [(100, True), (100000, False)])
def test_lattice_selection_through_a_plateau_and_past_it(monkeypatch, n_features, cut):
    key, kw = ('lattice',), dict(n_levels=4, n_features=n_features)
    want, n = levels(key, **kw)[0], counts(key, **kw)
    assert n[0] == 0 and n[1] > 50                                     # (the ideal crossings of level 0 are plateaus of the FAST score)
    if cut:
        keep, tied, kept = _selection(key, 1, **kw)
        assert 1 < keep < kept < n[1] and tied > 1                     # rank keep lies inside a plateau of equal responses
    else:
        assert all(c < w for c, w in zip(n, want))
    exp = run_three_ways(monkeypatch, key, **kw)
    assert len(exp[0]) > 50


# ---- workspace reuse ----
def test_one_workspace_serves_large_and_small_images_in_turn(monkeypatch):
    """The device block of a workspace grows with the largest image and is reused for every smaller one: score maps, candidate
    lists, histograms and ranks of the previous call lie in it.  Largest and smallest cases in turn, the overflow fallback
    among them; the first case again at the end gives the same bytes."""
    monkeypatch.delenv('SID_ORB_HOST_SELECT', raising=False)
    order = [(('dots', 1200), dict(n_levels=1, n_features=5000))]
    order += [CASES[k][:2] for k in ('one-pixel', '4001x70', '1x1', 'patch-200', 'too-low')]
    order += [(('dots', 1200), dict(n_levels=1, n_features=1))]
    order += [CASES[k][:2] for k in ('n_features=0', '70x4001', 'thins-to-one', 'all-candidates', 'fast-254-synth', 'seven-levels')]
    order += [(('lattice',), dict(n_levels=4, n_features=100)), order[0]]
    got = []
    for key, kw in order:
        xy, desc, meta, resp = orb.detect_and_compute(get_image(key), full=True, **kw)
        got.append((xy.astype(np.float32), meta, resp, desc))
        assert_same(got[-1], oracle(key, **kw), '%s %s after %d calls' % (key, kw, len(got) - 1))
    assert len(got[0][0]) == 5000
    for a, b in zip(got[0], got[-1]):
        assert a.tobytes() == b.tobytes()


# ---- argument checks: host checks that return before any launch ----
def _args(name):
    img = get_image(('noise', 100, 255, 17))
    if name == 'rows = 65536':
        return _flat(65536, 70), dict()
    return img, {
        'stride < cols': dict(stride=254),
        'n_levels = 0': dict(n_levels=0),
        'n_levels = 17': dict(n_levels=17),
        'edge_threshold = 15': dict(edge_threshold=15, patch_size=20),
        'patch_size / 2 + 1 > edge_threshold': dict(edge_threshold=16, patch_size=32),
        'fast_threshold = 0': dict(fast_threshold=0),
        'fast_threshold = 255': dict(fast_threshold=255),
        'scale_factor = 1': dict(scale_factor=1.0),
        'max_out = -1': dict(max_out=-1),
        'xy = NULL': dict(xy=False),
        'device = 99': dict(device=99),
    }[name]


@pytest.mark.parametrize('name,code,word', [
    ('rows = 65536', ERR_ARG, 'shape'), ('stride < cols', ERR_ARG, 'stride'), ('n_levels = 0', ERR_ARG, 'parameters'),
    ('n_levels = 17', ERR_ARG, 'parameters'), ('edge_threshold = 15', ERR_ARG, 'parameters'),
    ('patch_size / 2 + 1 > edge_threshold', ERR_ARG, 'parameters'), ('fast_threshold = 0', ERR_ARG, 'parameters'),
    ('fast_threshold = 255', ERR_ARG, 'parameters'), ('scale_factor = 1', ERR_ARG, 'parameters'), ('max_out = -1', ERR_ARG, 'argument'),
    ('xy = NULL', ERR_ARG, 'argument'), ('device = 99', ERR_NODEVICE, 'device')])
def test_bad_arguments_are_refused_before_anything_runs(name, code, word):
    img, how = _args(name)
    res = direct(img, **dict(dict(n_features=50, n_levels=2), **how))
    assert res.rc == code
    assert res.err and word in res.err, res.err                        # a message, and this call's (the last error is kept per thread)
    assert res.n_out in (N_SENT, 0)
    for name_ in NAMES:
        assert (getattr(res, name_) == SENT).all()
    # the same call with the argument put right runs
    good = direct(get_image(('noise', 100, 255, 17)), n_features=50, n_levels=2)
    assert good.rc == 0 and 0 < good.n_out <= 50
