"""CPU: the premises of tests/test_gpu_stage_paths.py.  The GPU tests compare csrc/stage.hip with tests/stage_spec.py on the
inputs of tests/stage_cases.py; here the spec says that every case is what it claims to be (so no GPU case is vacuous), the
spec's key map and order statistics are held against NumPy and oracle/stage_oracle.py, the scale probes are shown to tell a
division from a multiplication by the reciprocal, and the oracle reproduces fixture g6b (the reference's own outputs)."""
import numpy as np

from oracle import stage_oracle as so
from sea_ice_drift_amd import lib
from tests import stage_cases as cases
from tests import stage_spec as spec


def test_route_cases_take_the_route_they_name():
    seen = set()
    for name, img, fractions, aim in cases.route_cases():
        B = spec.begin_hint(img, fractions)
        assert B['m_valid'] >= spec.M_MIN, name
        S = spec.select(B, spec.fraction_ranks(B['n_valid'], fractions))
        assert all(r == aim for r in S['routes']), (name, B['shift'], S['routes'])
        seen.add(aim)
    assert seen == {('direct', 0), ('resolved', 1), ('resolved', 2), ('resolved', 4), ('resolved', 8), ('radix', 0)}
    # the widths at which the radix route is taken for want of a narrow enough bracket, and for an open one
    by = {c[0]: spec.begin_hint(c[1], c[2]) for c in cases.route_cases()}
    assert by['w28_0.5']['shift'] == [14] and by['w29_0.5']['shift'] == [15]
    assert by['w20_0_1']['lo'][0] == 0 and by['w20_0_1']['lo'][1] + by['w20_0_1']['span'][1] == spec.OPEN_HI
    assert by['sar_0.5']['lo'][0] < 0x80000000                       # keys of negative floats


def test_selector_cases_do_what_they_name():
    for name, img, fractions, calls, aim in cases.selector_cases():
        B = spec.begin_hint(img, fractions)
        for ranks, want in zip(calls, aim):
            S = spec.select(B, ranks)
            got = (S['n_direct'], S['n_resolved'], S['n_radix'], S['resolve_passes'], S['resolve_states'])
            assert got == want, (name, ranks, got, want)
    by = {c[0]: c for c in cases.selector_cases()}
    for t in (27, 28):
        assert spec.begin_hint(by['twelve_w%d' % t][1], [0.5])['shift'] == [t - 14]
    B = spec.begin_hint(by['split_mixed'][1], by['split_mixed'][2])
    assert B['shift'][0] == 0 and 0 < B['shift'][1] <= spec.MAX_SHIFT
    assert len(spec.begin_hint(by['three_w20'][1], by['three_w20'][2])['lo']) == 3
    # two_widths: rank A in range 0, rank B in range 1 only; their bins start at one key, 4 and 8192 keys wide
    img, a, b = cases.two_widths_image()
    B = spec.begin_hint(img, list(cases.TWO_WIDTHS_FRACTIONS))
    ra, rb = spec.rank_route(B, a), spec.rank_route(B, b)
    assert ra[:2] == ('resolved', 0) and rb[:2] == ('resolved', 1) and ra[2] == rb[2] and (ra[3], rb[3]) == (1, 4), (ra, rb, B['shift'])
    assert B['shift'][0] < 11 and B['shift'][1] == 13 and not B['below'][0] <= b < B['below'][0] + B['inside'][0]


def test_sampler_cases_sit_where_they_say():
    c = cases.sampler_cases()
    m = {k: len(spec.sample_keys(v)) for k, v in c.items()}
    assert m['n1'] == 1 and m['n255'] == 255 and m['n256'] == 256 and m['n257_one_nan'] == 256
    for k in ('n1', 'n255', 'nan99', 'all_nan', 'one_valid'):          # below the cut-off: the state that matches nothing
        B = spec.begin_hint(c[k], [0.1, 0.99])
        assert B['lo'] == [spec.NO_KEY] * 2 and B['span'] == [0, 0] and B['below'] == [B['n_valid']] * 2 and B['inside'] == [0, 0], k
    for k in ('n256', 'n257_one_nan', 'n8191', 'n8192', 'n8193', 'step2', 'step3'):
        assert spec.begin_hint(c[k], [0.5])['inside'][0] > 0, k
    assert m['nan99'] < 256 < int((~np.isnan(c['nan99'])).sum())
    assert m['all_nan'] == 0 and int((~np.isnan(c['one_valid'])).sum()) == 1
    for k, step in (('n8191', 0), ('n8192', 1), ('n8193', 1), ('step2', 2), ('step3', 3)):
        assert c[k].size // spec.K_SAMPLE == step, k
    assert len(spec.sample_positions(8191)) == 8191 and spec.sample_positions(8193).max() == 8191
    for npix in (16900, 24600):                                         # one position per stride of `step`, all inside
        p = spec.sample_positions(npix)
        assert len(p) == 8192 and (p // (npix // 8192) == np.arange(8192)).all() and len(set(p % (npix // 8192))) > 1


def test_keyspace_cases_hold_what_they_name():
    c = cases.keyspace_cases()
    assert np.isposinf(c['inf']).any() and np.isneginf(c['inf']).any()
    n = int((~np.isnan(c['inf_heavy'])).sum())
    assert np.isneginf(spec.order_stats(c['inf_heavy'], [int(0.1 * (n - 1))])) and np.isposinf(spec.order_stats(c['inf_heavy'], [int(0.99 * (n - 1))]))
    z = c['zeros']
    assert (np.signbit(z) & (z == 0)).sum() >= 500 and (~np.signbit(z) & (z == 0)).sum() >= 500
    bits = c['nan_payload'].view(np.uint32)
    assert {0xffc00001, 0x7f800001, 0xffffffff} <= set(bits[np.isnan(c['nan_payload'])].tolist())
    assert spec.begin_hint(c['constant'], [0.5])['span'] == [0]
    k = spec.valid_keys(c['last10'])
    assert (k >> 10).min() == (k >> 10).max() and len(np.unique(k)) > 900
    B = spec.begin_hint(c['sign_straddle'], [0.5])
    assert B['lo'][0] < 0x80000000 <= B['lo'][0] + B['span'][0] and B['shift'] == [0]
    B = spec.begin_hint(c['sign_wide'], [0.5])
    assert B['lo'][0] < 0x80000000 <= B['lo'][0] + B['span'][0] and B['shift'][0] > spec.MAX_SHIFT
    sub = c['subnormal']
    for v in (cases.SUB_MIN, -cases.SUB_MIN, cases.SUB_MAX, -cases.SUB_MAX):
        assert (sub == v).sum() >= 60


def test_no_bracket_rank_hangs_on_the_last_bit_of_a_square_root():
    """idx -+ dev is floored / ceiled: a device square root that differed in the last bit could change a rank only where
    that value is within rounding of an integer.  No case is within 1e-6 of one (fractions 0 and 1 take sqrt(0), exactly 0)."""
    imgs = [c[1] for c in cases.route_cases()] + [c[1] for c in cases.selector_cases()] + list(cases.public_cases().values())
    for m in sorted({len(spec.sample_keys(i)) for i in imgs}):
        if m >= spec.M_MIN:
            for fr in cases.FRACTION_SETS + tuple([a / 100.0, b / 100.0] for a, b in cases.PERCENTILE_PAIRS):
                for f in fr:
                    assert spec.bracket_ranks(f, m)[2] > 1e-6, (m, f)


def test_key_map_is_monotone_and_invertible():
    edge = np.array([-np.inf, -cases.FLT_MAX, -1.0, -cases.SUB_MAX, -cases.SUB_MIN, -0.0, 0.0, cases.SUB_MIN, cases.SUB_MAX,
                     np.uint32(0x00800000).view(np.float32), 1.0, cases.FLT_MAX, np.inf], dtype=np.float32)
    k = spec.f2key(edge).astype(np.int64)
    assert (np.diff(k) > 0).all() and k.max() < spec.OPEN_HI
    np.testing.assert_array_equal(spec.key2f(spec.f2key(edge)).view(np.uint32), edge.view(np.uint32))
    x = np.random.default_rng(3).integers(0, 2 ** 32, 100000, dtype=np.uint64).astype(np.uint32).view(np.float32)
    x = x[~np.isnan(x)]
    np.testing.assert_array_equal(spec.key2f(spec.f2key(x)).view(np.uint32), x.view(np.uint32))
    o = np.argsort(spec.f2key(x), kind='stable')
    assert (np.diff(x[o]) >= 0).all()
    nan_keys = spec.f2key(np.array([0x7fffffff], dtype=np.uint32).view(np.float32))
    assert nan_keys[0] == spec.NO_KEY                                   # only a NaN has the key the kernels use for "none"


def test_spec_order_statistics_give_numpys_percentiles():
    for name, img in cases.public_cases().items():
        n = int((~np.isnan(img)).sum())
        if n == 0:
            continue
        for pair in cases.PERCENTILE_PAIRS:
            for p in pair:
                lo, hi, t = lib._percentile_ranks(n, p, np.float32)
                a, b = spec.order_stats(img, [lo, hi])
                got = lib._lerp(a, b, t)
                with np.errstate(all='ignore'):
                    ref, ora = np.nanpercentile(img, p), so.nanpercentile(img, p)
                for other in (ref, ora):
                    assert got == other or (np.isnan(got) and np.isnan(other)), (name, p, got, other)
                assert np.asarray(got).dtype == np.float32


def test_scale_probes_tell_a_division_from_a_reciprocal():
    counts = []
    for vmin, denom in cases.SCALE_PAIRS:
        x = cases.scale_probes(vmin, denom)
        assert x.shape == (1, 4335 + len(cases.SCALE_SPECIALS))
        a, b = cases.scale_reference(x, vmin, denom), cases.scale_reference(x, vmin, denom, reciprocal=True)
        counts.append(int((a[:, :4335] != b[:, :4335]).sum()))
        exp, _, _ = so.get_uint8_image(x.copy(), np.float32(vmin), np.float32(vmin) + np.float32(denom), 0, 0)
        if np.float32(np.float32(vmin) + np.float32(denom)) - np.float32(vmin) == np.float32(denom):
            np.testing.assert_array_equal(a, exp)                      # the same arithmetic as the oracle's
        assert set(np.unique(a[:, :4335]).tolist()) >= set(range(1, 256)), (vmin, denom)
    assert all(c > 0 for c in counts), counts
    for vmin, denom in cases.SCALE_PAIRS_BLIND:
        x = cases.scale_probes(vmin, denom)
        assert (cases.scale_reference(x, vmin, denom) == cases.scale_reference(x, vmin, denom, reciprocal=True)).all()
    # the subnormal pair's probes are subnormal: a kernel that flushed them would scale every one to the same value
    x = cases.scale_probes(*cases.SCALE_PAIRS[2])[:, :4335]
    assert (np.abs(x) < np.float32(1.1754944e-38)).sum() > 4000


def test_oracle_reproduces_fixture_g6b():
    """The reference's own get_uint8_image on the small cases (tests/golden/make_golden.py g6b): every stored output."""
    stored, left = cases.golden_g6b()
    imgs = cases.public_cases()
    assert all(k.endswith('_2') for k in left if not k.startswith(('out_inf', 'out_flt_max')))   # pmin == pmax: 0 / 0
    n = 0
    for name in sorted(imgs):
        for pi, (pmin, pmax) in enumerate(cases.PERCENTILE_PAIRS):
            key = 'out_%s_%d' % (name, pi)
            if key in stored:
                out, v0, v1 = so.get_uint8_image(imgs[name].copy(), None, None, pmin, pmax)
                cases.g6b_equal(stored, key, out)
                assert np.float64(v0) == stored[key][2] and np.float64(v1) == stored[key][3], key
                n += 1
            else:
                assert not cases.has_two_finite_values(imgs[name]) or key in left, key
    assert n == len(stored) >= 40


def test_debug_route_checks_its_arguments_without_a_device():
    import ctypes
    from sea_ice_drift_amd import _capi
    L = _capi.lib()
    assert L.sid_stage_debug_route(None, None) == -1 and b'null' in L.sid_stage_last_error()
    assert ctypes.sizeof(_capi._StageRoute) == 152                    # struct sid_stage_route: no padding to guess at
