"""Host side of the multi-device call (``devices=`` of pattern_matching / pm_dispatch): how the argument is normalised
(``pmlib.resolve_devices``) and how the points of a call are cut into one shard per handle (``pmlib.plan_shards``).
Both are pure functions; the shard plan prices points with the library's host arithmetic, no GPU is touched."""
import numpy as np
import pytest

from sea_ice_drift_amd import dist, pmlib as my, synthetic as syn


# ------------------------------------------------------------------ resolve_devices
@pytest.mark.parametrize('n_visible', [1, 8])
def test_resolve_devices_none_is_the_one_handle_of_device(n_visible):
    assert my.resolve_devices(None, 0, n_visible) == [0]
    assert my.resolve_devices(None, np.int64(0), n_visible) == [0]
    assert my.resolve_devices(None, 5, n_visible) == [5]             # today's behaviour: ``device=`` is not second-guessed
    assert all(type(d) is int for d in my.resolve_devices(None, np.int64(0), n_visible))


def test_resolve_devices_all():
    assert my.resolve_devices('all', 0, 1) == [0]
    assert my.resolve_devices('all', 0, 8) == list(range(8))
    assert my.resolve_devices('all', 3, 8) == list(range(8))         # ``device=`` plays no part once devices is given


def test_resolve_devices_count():
    assert my.resolve_devices(1, 0, 1) == [0]
    assert my.resolve_devices(1, 0, 8) == [0]
    assert my.resolve_devices(3, 0, 8) == [0, 1, 2]
    assert my.resolve_devices(8, 0, 8) == list(range(8))
    assert my.resolve_devices(np.int32(2), 0, 8) == [0, 1]


def test_resolve_devices_sequences_keep_order_and_repeats():
    assert my.resolve_devices([0], 0, 1) == [0]
    assert my.resolve_devices([0, 0], 0, 1) == [0, 0]
    assert my.resolve_devices([0] * 8, 0, 1) == [0] * 8
    assert my.resolve_devices((3, 1, 3), 0, 8) == [3, 1, 3]
    assert my.resolve_devices(range(4), 0, 8) == [0, 1, 2, 3]
    got = my.resolve_devices(np.array([7, 0]), 0, 8)
    assert got == [7, 0] and all(type(d) is int for d in got)


@pytest.mark.parametrize('n_visible,devices,names', [
    (1, True, 'True'), (8, True, 'True'), (8, False, 'False'),                 # a bool is not a count
    (1, [True], 'devices[0]=True'), (8, [0, False], 'devices[1]=False'),       # ... nor an index
    (1, 0, 'devices=0'), (8, 0, 'devices=0'), (8, -1, 'devices=-1'),           # n < 1
    (1, 2, 'devices=2'), (8, 9, 'devices=9'),                                  # n > visible
    (1, [], '[]'), (8, (), '()'), (8, np.zeros(0, dtype=np.int64), 'empty'),   # names no GPU
    (1, [-1], 'devices[0]=-1'), (8, [0, -2], 'devices[1]=-2'),                 # negative index
    (1, [0, 1], 'devices[1]=1'), (8, [0, 8], 'devices[1]=8'), (8, [3, 1, 99], 'devices[2]=99'),   # index >= visible
    (8, 'ALL', "'ALL'"), (8, 'cuda:0', "'cuda:0'"), (8, '0', "'0'"),           # strings other than 'all'
    (8, [0, 1.0], 'devices[1]=1.0'), (8, ['0'], "devices[0]='0'"), (8, [None], 'devices[0]=None'),
    (8, [[0, 1]], 'devices[0]=[0, 1]'), (8, np.zeros((2, 2), dtype=np.int64), 'flat'),
    (8, 2.0, '2.0'), (8, {0, 1}, '{0, 1}'), (8, {0: 1}, '{0: 1}'),
    (0, 'all', 'no GPU'), (0, 1, 'devices=1'), (0, [0], 'devices[0]=0'),       # nothing visible
])
def test_resolve_devices_refuses_everything_else_and_names_the_entry(n_visible, devices, names):
    with pytest.raises(ValueError) as e:
        my.resolve_devices(devices, 0, n_visible)
    assert names in str(e.value), str(e.value)


# ------------------------------------------------------------------ plan_shards
@pytest.fixture(scope='module')
def borders():
    b = syn.make_grid(700, 700, 12)['border']
    assert b.size == 144 and b.min() >= 20 and b.max() <= 50 and np.unique(b).size > 3    # mixed borders
    return b


@pytest.mark.parametrize('n_angles', [3, 15])
@pytest.mark.parametrize('n_shards', [1, 2, 3, 8])
def test_plan_shards_partitions_the_points_and_is_the_cut_of_dist(borders, n_angles, n_shards):
    shards = my.plan_shards(borders, n_shards, 34, n_angles, 1)
    assert isinstance(shards, list) and len(shards) == n_shards
    for idx in shards:
        assert isinstance(idx, np.ndarray) and idx.dtype == np.int64 and idx.ndim == 1
        assert (np.diff(idx) > 0).all()                                       # ascending, no repeats
    np.testing.assert_array_equal(np.sort(np.concatenate(shards)), np.arange(144))
    # a pure function of its arguments
    again = my.plan_shards(borders.copy(), n_shards, 34, n_angles, 1)
    for a, b in zip(shards, again):
        np.testing.assert_array_equal(a, b)
    # the cost model is dist's, not a second one
    order, cuts, _ = dist.shard_cuts_by_cost(borders, n_shards, 34, n_angles, 1)
    for k, idx in enumerate(shards):
        np.testing.assert_array_equal(idx, dist.indices_of_cut(order, cuts, k))
    if n_shards == 1:
        np.testing.assert_array_equal(shards[0], np.arange(144))
    else:
        assert sum(idx.size > 0 for idx in shards) >= 2                       # 144 points are not left to one handle


def test_plan_shards_fewer_points_than_shards():
    shards = my.plan_shards(np.array([20.0, 50.0, 33.0]), 8, 35, 3, 1)
    assert len(shards) == 8
    assert sum(idx.size > 0 for idx in shards) <= 3
    assert all(idx.dtype == np.int64 for idx in shards)
    assert sorted(np.concatenate(shards).tolist()) == [0, 1, 2]


@pytest.mark.parametrize('n_shards', [1, 3])
def test_plan_shards_no_points(n_shards):
    shards = my.plan_shards(np.zeros(0), n_shards, 34, 3, 1)
    assert len(shards) == n_shards and all(idx.size == 0 and idx.dtype == np.int64 for idx in shards)


def test_plan_shards_needs_a_shard():
    with pytest.raises(ValueError):
        my.plan_shards(np.array([20.0]), 0, 34, 3, 1)


# ------------------------------------------------------------------ argument checks that come before any device work
def test_unsupported_sweep_options_still_raise_first():
    with pytest.raises(NotImplementedError):
        my.pm_dispatch(None, None, [], [], [], [], [], 34, 0.0, mtype=3, devices='bogus')
    with pytest.raises(NotImplementedError):
        my.pm_dispatch(None, None, [], [], [], [], [], 34, 0.0, template_matcher=lambda *a: None, devices=[0, 0], context=object())


def test_devices_with_a_context_is_refused():
    with pytest.raises(ValueError) as e:
        my.pm_dispatch(None, None, [], [], [], [], [], 34, 0.0, devices=[0, 0], context=object())
    assert 'context' in str(e.value)


# ------------------------------------------------------------------ feature tracking: which image goes where
def test_feature_tracking_detects_image_1_on_the_first_device_and_image_2_on_the_second(monkeypatch):
    """The detector and the matcher replaced by stand-ins that record their ``device``: with ``devices=[5, 2, 7]`` image 1 is
    detected on GPU 5, image 2 on GPU 2, both in flight at once on threads of their own, the matcher runs on GPU 5; with one entry both images
    go there.  The matched vectors are those of the call without ``devices`` (fixture G7's inputs)."""
    import threading

    from oracle import ft_oracle as fo
    from sea_ice_drift_amd import _capi, ftlib, orb
    from sea_ice_drift_amd.seaicedrift import SeaIceDrift
    from tests.golden import make_golden as mg
    n1, n2, xy1, d1, xy2, d2 = mg.g7_inputs(False)
    n2.image = np.full_like(n1.image, 2)                                  # (G7's two images are one array of ones)
    seen, matched = {}, []

    both_in = threading.Barrier(2, timeout=60)                            # (a detection that waited for the other one to end
                                                                          # would break it)
    def detect(image, device=0, **kw):
        both_in.wait()
        seen[int(image[0, 0])] = (device, threading.get_ident())
        return (xy1, d1) if image[0, 0] == 1 else (xy2, d2)

    def knn(da, db, device=0, verbose=False):
        matched.append(device)
        return fo.knn2(da, db)
    monkeypatch.setattr(orb, 'detect_and_compute', detect)
    monkeypatch.setattr(ftlib, '_get_matches', knn)
    monkeypatch.setattr(_capi, 'device_count', lambda: 8)
    kw = dict(domainMargin=10, ratio_test=0.75, psi=150, max_drift=25000.0)
    ref = ftlib.feature_tracking(n1, n2, **kw)
    assert len(ref[0]) > 2000 and seen[1][0] == 0 and seen[2][0] == 0 and matched == [0]
    for devices, want in (([5, 2, 7], (5, 2)), ([3], (3, 3)), (2, (0, 1)), ('all', (0, 1))):
        seen.clear()
        del matched[:]
        got = ftlib.feature_tracking(n1, n2, devices=devices, **kw)
        assert (seen[1][0], seen[2][0]) == want and matched == [want[0]], devices
        assert seen[1][1] != seen[2][1] and threading.get_ident() not in (seen[1][1], seen[2][1])
        for a, b in zip(got, ref):
            np.testing.assert_array_equal(a, b)
    # the class hands its default on, and a call's own devices= overrides it
    seen.clear()
    out = SeaIceDrift(n1, n2, devices=[4, 6]).get_drift_FT(**kw)
    assert (seen[1][0], seen[2][0]) == (4, 6) and len(out[0]) == len(ref[0])
    seen.clear()
    SeaIceDrift(n1, n2, devices=[4, 6]).get_drift_FT(devices=[1], **kw)
    assert (seen[1][0], seen[2][0]) == (1, 1)
    with pytest.raises(ValueError):
        ftlib.feature_tracking(n1, n2, devices=[0, 8], **kw)


# ------------------------------------------------------------------ the dispatch over stand-in handles
class FakeHandle(object):
    """Records what the dispatch asks of a handle; its 'results' are the c1 of its points in column 0."""

    def __init__(self, log, name, fail_in=None, error=RuntimeError('boom')):
        self.log, self.name, self.fail_in, self.error, self.c1 = log, name, fail_in, error, None

    def _call(self, what):
        self.log.append((self.name, what))
        if what == self.fail_in:
            raise self.error

    def set_points(self, c1, r1, c2fg, r2fg, border, img_size, alpha0, angles, rot=None, flags=1):
        self.c1 = np.array(c1)
        self._call('set_points')

    def run(self):
        self._call('run')

    def sync(self):
        self._call('sync')

    def fetch(self, want_ij=True):
        self._call('fetch')
        out = np.zeros((self.c1.size, 5))
        out[:, 0] = self.c1
        return out


def _fake_dispatch(handles, n=400, **kw):
    g = syn.make_grid(3000, 3000, 40)                                      # (400 of its points: three shards, none empty)
    v = [g[k][:n] for k in ('c1', 'r1', 'c2fg', 'r2fg', 'border')]
    v[0] = np.arange(n, dtype=np.float64)                                  # c1 = the point's index
    return my._dispatch_sharded(handles, *v, 34, 0.0, [-3, 0, 3], 1, None, **kw)


def test_dispatch_enqueues_every_shard_before_the_first_fetch_and_merges_in_point_order():
    log = []
    handles = [FakeHandle(log, k) for k in range(3)]
    timings = {}
    out = _fake_dispatch(handles, timings=timings)
    assert out.shape == (400, 5) and out.dtype == np.float64
    np.testing.assert_array_equal(out[:, 0], np.arange(400))
    kinds = [what for _, what in log if what != 'sync']                    # (timings= adds a sync before each fetch)
    assert sum(timings['points_per_handle']) == 400 and min(timings['points_per_handle']) > 0
    assert kinds == ['set_points', 'run'] * 3 + ['fetch'] * 3
    assert set(timings) >= {'plan', 'set_points', 'run', 'kernel_wait', 'fetch', 'merge'}
    del log[:]
    _fake_dispatch(handles)
    assert [what for _, what in log] == ['set_points', 'run'] * 3 + ['fetch'] * 3      # no extra sync without timings=
    # an empty shard's handle is left alone; no points: no handle is touched
    del log[:]
    out = _fake_dispatch([FakeHandle(log, k) for k in range(8)], n=3)
    np.testing.assert_array_equal(out[:, 0], np.arange(3))
    assert len({name for name, _ in log}) <= 3
    del log[:]
    assert _fake_dispatch(handles, n=0).shape == (0, 5) and log == []


@pytest.mark.parametrize('fail_in', ['set_points', 'run', 'fetch'])
def test_a_failing_shard_leaves_no_run_in_flight(fail_in):
    """Handle 1 of three raises: every handle that was given work and has not been fetched is synchronised before the
    exception leaves the dispatch - the caller releases the locks next."""
    log = []
    handles = [FakeHandle(log, 0), FakeHandle(log, 1, fail_in=fail_in), FakeHandle(log, 2)]
    with pytest.raises(RuntimeError, match='boom'):
        _fake_dispatch(handles)
    at = log.index((1, fail_in))
    after = log[at + 1:]
    if fail_in == 'fetch':                                                 # 0 was fetched (a fetch synchronises); 1 and 2 were running
        assert (0, 'fetch') in log[:at] and set(after) == {(1, 'sync'), (2, 'sync')}
    else:                                                                  # 2 was never started; 0 is running, 1 may be
        assert set(after) == {(0, 'sync'), (1, 'sync')} and not any(name == 2 for name, _ in log)


def test_a_failing_sync_does_not_hide_the_first_error_and_code_minus_4_keeps_its_type():
    from sea_ice_drift_amd import _capi
    log = []
    handles = [FakeHandle(log, 0, fail_in='sync', error=ValueError('late')), FakeHandle(log, 1, fail_in='run')]
    with pytest.raises(RuntimeError, match='boom'):
        _fake_dispatch(handles)
    assert (0, 'sync') in log
    handles = [FakeHandle(log, 0), FakeHandle(log, 1, fail_in='set_points', error=_capi.SidPmError(-4, 'not supported'))]
    with pytest.raises(NotImplementedError):
        _fake_dispatch(handles)
    handles = [FakeHandle(log, 0), FakeHandle(log, 1, fail_in='set_points', error=_capi.SidPmError(-2, 'other'))]
    with pytest.raises(_capi.SidPmError):
        _fake_dispatch(handles)


def test_handles_are_locked_in_sorted_key_order_and_released(monkeypatch):
    """``_Handles``: the k-th repeat of a GPU is replica k; the locks are taken in sorted key order whatever the order of the
    list, held inside the block and free after it - also when a handle cannot be created."""
    made = []

    class Ctx(object):
        def __init__(self, device):
            if device == 9:
                raise RuntimeError('no such device')
            made.append(device)

        def close(self):
            pass
    monkeypatch.setattr(my._capi, 'PMContext', Ctx)
    monkeypatch.setattr(my, '_CONTEXTS', {})
    monkeypatch.setattr(my, '_CONTEXT_LOCKS', {})
    order = []

    class Spy(object):
        def __init__(self, key):
            self.key, self.lock = key, __import__('threading').RLock()

        def acquire(self, *a, **k):
            order.append(self.key)
            return self.lock.acquire(*a, **k)

        def release(self):
            self.lock.release()
    for key in ((1, 0), (0, 0), (1, 1), (9, 0)):
        my._CONTEXT_LOCKS[key] = Spy(key)
    hs = my._Handles([1, 0, 1])
    assert hs.keys == [(1, 0), (0, 0), (1, 1)]
    with hs as ctxs:
        assert order == [(0, 0), (1, 0), (1, 1)] and len(ctxs) == 3 and made == [1, 0, 1]
        assert my.resident_handles() == [(0, 0), (1, 0), (1, 1)]
        assert ctxs[0] is my._shared_context(1)[0] and ctxs[2] is my._shared_context(1, 1)[0]
    import threading
    free = []
    def probe():                                                           # another thread can take every lock at once
        for s in list(my._CONTEXT_LOCKS.values()):
            free.append(s.lock.acquire(timeout=5))
        for s, ok in zip(list(my._CONTEXT_LOCKS.values()), free):
            if ok:
                s.lock.release()
    t = threading.Thread(target=probe, daemon=True)
    t.start()
    t.join(30)
    assert free == [True] * 4
    with pytest.raises(RuntimeError, match='no such device'):
        with my._Handles([0, 9]):
            pass
    assert my.resident_handles() == [(0, 0), (1, 0), (1, 1)]
    my.release_contexts()
    assert my.resident_handles() == []
