"""GPU: every kernel path of the uint8 staging step (csrc/stage.hip) on tiny images, bit for bit.

The sampler and the selector are held against tests/stage_spec.py through sid_stage_debug_route (StageWorkspace.route()): a
mistake in the sampler or in the bracket arithmetic would otherwise only send a rank down the radix route, whose result is as
exact as the hinted one.  Layouts, the edges of the key space and the integer boundaries of the scale map are held against
NumPy and oracle/stage_oracle.py; the public call also against the reference's own outputs (fixture g6b).  The inputs are
those of tests/stage_cases.py; tests/test_stage_spec_host.py shows on the CPU that each is what it claims to be.  No
tolerance appears anywhere."""
import contextlib
import io

import numpy as np
import pytest

from oracle import stage_oracle as so
from sea_ice_drift_amd import _capi, lib
from tests import stage_cases as cases
from tests import stage_spec as spec

pytestmark = pytest.mark.gpu
BEGIN_FIELDS = ('n_hint', 'm_valid', 'n_valid', 'lo', 'span', 'shift', 'below', 'inside')
CALL_FIELDS = ('n_direct', 'n_resolved', 'n_radix', 'resolve_passes', 'resolve_states')


@pytest.fixture(scope='module')
def ws():
    w = _capi.StageWorkspace(0)
    yield w
    w.close()


def quiet(fn, *a):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*a)


def device(a):
    import torch
    return torch.from_numpy(np.array(a)).cuda()


def stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def begin(ws, t, fractions=None):
    """begin on a 2-D device tensor (any row stride)."""
    return ws.begin(t.data_ptr(), int(t.shape[0]), int(t.shape[1]), int(t.stride(0)), stream(), fractions=fractions)


def assert_begin(ws, t, img, fractions, what):
    """Hinted begin against the spec: the count and every field sid_stage_begin_hint keeps; one pass over the image so far."""
    B = spec.begin_hint(img, fractions)
    assert begin(ws, t, fractions) == B['n_valid'], what
    R = ws.route()
    assert {k: R[k] for k in BEGIN_FIELDS} == {k: B[k] for k in BEGIN_FIELDS}, what
    assert R['image_passes'] == 1 and all(R[k] == 0 for k in CALL_FIELDS), what
    return B


def assert_calls(ws, B, img, calls, what):
    """Consecutive order_stats calls after one begin: values against np.sort, the route counters and the passes against the spec."""
    passes, known = 1, B['n_hint'] == 0
    for ranks in calls:
        got = ws.order_stats(ranks)
        np.testing.assert_array_equal(got, spec.order_stats(img, ranks), err_msg='%s ranks %s' % (what, ranks))
        S = spec.select(B, ranks, first_digit_known=known)
        R = ws.route()
        assert {k: R[k] for k in CALL_FIELDS} == {k: S[k] for k in CALL_FIELDS}, (what, ranks)
        passes += S['image_passes_added']
        known = known or S['n_radix'] > 0
        assert R['image_passes'] == passes, (what, ranks)
    return passes


def all_images():
    """(name, image, fraction sets) of every route, selector, sampler and key-space case."""
    out = [(n, i, [f]) for n, i, f, _ in cases.route_cases()] + [(n, i, [f]) for n, i, f, _, _ in cases.selector_cases()]
    out += [(n, i, list(cases.FRACTION_SETS)) for n, i in cases.public_cases().items()]
    out += [('wide20', cases.wide_image(20), list(cases.FRACTION_SETS)), ('mixed', cases.mixed_image(), list(cases.FRACTION_SETS))]
    return out


def test_sampler_against_the_spec(ws):
    """m_valid, n_valid and per range lo, span, shift, below, inside of every case equal the NumPy sampler's."""
    for name, img, fraction_sets in all_images():
        t = device(img)
        for fr in fraction_sets:
            assert_begin(ws, t, img, fr, '%s %s' % (name, fr))


def test_routes_are_the_ones_the_cases_name(ws):
    """Every rank of a route case takes the route the case was written for, and the value is np.sort's."""
    for name, img, fr, aim in cases.route_cases():
        t = device(img)
        B = assert_begin(ws, t, img, fr, name)
        ranks = spec.fraction_ranks(B['n_valid'], fr)
        passes = assert_calls(ws, B, img, [ranks], name)
        R = ws.route()
        want = {'direct': 'n_direct', 'resolved': 'n_resolved', 'radix': 'n_radix'}[aim[0]]
        assert R[want] == len(ranks) and R['n_direct'] + R['n_resolved'] + R['n_radix'] == len(ranks), name
        # (sample aside) 1 pass + the resolving passes + 3 where a rank took the radix route
        assert passes == 1 + R['resolve_passes'] + (3 if aim[0] == 'radix' else 0), name
        if aim[0] == 'resolved':
            assert R['resolve_states'] >= aim[1] and R['resolve_states'] % aim[1] == 0, name


def test_selector_against_the_spec(ws, monkeypatch):
    """The selector cases call by call; then the same ranks without the hint (SID_STAGE_NO_HINT=1, and a plain begin)."""
    for name, img, fr, calls, aim in cases.selector_cases():
        t = device(img)
        B = assert_begin(ws, t, img, fr, name)
        assert_calls(ws, B, img, calls, name)
        P = spec.plain_begin(img)
        for env in (True, False):
            if env:
                monkeypatch.setenv('SID_STAGE_NO_HINT', '1')
            assert begin(ws, t, fr if env else None) == P['n_valid'], name
            if env:
                monkeypatch.delenv('SID_STAGE_NO_HINT')
            R = ws.route()
            assert R['n_hint'] == 0 and R['lo'] == [] and R['m_valid'] == 0 and R['image_passes'] == 1, name
            assert_calls(ws, P, img, calls, name + ' (no hint)')


def test_order_statistics_of_every_case(ws):
    """Sampler and key-space cases: the ranks next to each fraction, the ends and the middle, hinted and plain; +-inf are order
    statistics like any value, -0.0 and +0.0 compare as values, NaNs of either sign and any payload never count."""
    for name, img in cases.public_cases().items():
        t = device(img)
        n = int((~np.isnan(img)).sum())
        for fr in ([0.10, 0.99], [0.5], [0.0, 1.0], [0.001, 0.25, 0.75, 0.999]):
            B = assert_begin(ws, t, img, fr, name)
            if n == 0:
                with pytest.raises(_capi.SidPmError):
                    ws.order_stats([0])
                continue
            ranks = spec.fraction_ranks(n, fr)
            ends = sorted({0, min(1, n - 1), n // 3, n // 2, max(n - 2, 0), n - 1})
            assert_calls(ws, B, img, [ranks, ends], '%s %s' % (name, fr))
            with pytest.raises(_capi.SidPmError):
                ws.order_stats([n])
        if n:
            begin(ws, t)
            assert_calls(ws, spec.plain_begin(img), img, [ends], name + ' (plain)')
    inf = cases.keyspace_cases()['inf']
    n = int((~np.isnan(inf)).sum())
    begin(ws, device(inf), [0.0, 1.0])
    assert np.isneginf(ws.order_stats([0])[0]) and np.isposinf(ws.order_stats([n - 1])[0])


def scale(t, vmin, denom, out):
    _capi.stage_scale_u8(t.data_ptr(), int(t.shape[0]), int(t.shape[1]), int(t.stride(0)), np.float32(vmin), np.float32(denom),
                         out.data_ptr(), int(out.stride(0)), stream())


@pytest.mark.parametrize('name', sorted(cases.LAYOUTS))
def test_layouts(ws, name):
    """One content at every placement: counts, order statistics and the scaled image are those of the content alone; the +inf
    around the input view would show as a wrong count, a write outside the output view as a changed 0xAB."""
    import torch
    buf, rows, cols, stride, off, content = cases.layout_buffer(name)
    dbuf = device(buf)
    assert dbuf.data_ptr() % 256 == 0
    t = dbuf.as_strided((rows, cols), (stride, 1), off)
    assert (t.data_ptr() - dbuf.data_ptr()) == 4 * off
    n = int((~np.isnan(content)).sum())
    ends = sorted({0, min(1, n - 1), n // 3, n // 2, max(n - 2, 0), n - 1})
    assert begin(ws, t) == n
    assert_calls(ws, spec.plain_begin(content), content, [ends], name)
    for fr in ([0.5], [0.10, 0.99], [0.001, 0.25, 0.75, 0.999]):
        B = assert_begin(ws, t, content, fr, name)
        assert_calls(ws, B, content, [ends, spec.fraction_ranks(n, fr)], '%s %s' % (name, fr))
    vmin, vmax = np.float32(-30.0), np.float32(-12.0)
    exp, _, _ = so.get_uint8_image(content.copy(), vmin, vmax, 0, 0)
    for oname, (extra, ooff) in cases.OUT_LAYOUTS.items():
        ostride = cols + extra
        obuf = torch.full((ooff + rows * ostride + 16,), cases.SENTINEL_OUT, dtype=torch.uint8, device='cuda')
        assert obuf.data_ptr() % 256 == 0
        out = obuf.as_strided((rows, cols), (ostride, 1), ooff)
        scale(t, vmin, vmax - vmin, out)
        np.testing.assert_array_equal(out.cpu().numpy(), exp, err_msg='%s -> %s' % (name, oname))
        mask = torch.ones_like(obuf, dtype=torch.bool)
        mask.as_strided((rows, cols), (ostride, 1), ooff)[...] = False
        assert bool((obuf[mask] == cases.SENTINEL_OUT).all()), '%s -> %s: a write outside the view' % (name, oname)
    np.testing.assert_array_equal(dbuf.cpu().numpy().view(np.uint32), buf.view(np.uint32))     # the input is untouched


@pytest.mark.parametrize('vmin,denom', cases.SCALE_PAIRS)
def test_scale_at_the_integer_boundaries(vmin, denom):
    """Pixels whose scaled value is within a few ulp of an integer: a division that is not correctly rounded (or a multiplication
    by the reciprocal) and flushed subnormals show here and hardly anywhere else.  Scalar, flat vector and row-wise vector path."""
    import torch
    x = cases.scale_probes(vmin, denom)
    exp = cases.scale_reference(x, vmin, denom)
    t = device(x)
    out = torch.zeros(x.shape, dtype=torch.uint8, device='cuda')
    scale(t, vmin, denom, out)                                          # 1 x 4342: cols % 4 != 0, the scalar path
    got = out.cpu().numpy()
    bad = np.flatnonzero(got != exp)
    assert bad.size == 0, 'pixels %s: %s, expected %s' % (x[0, bad[:5]], got[0, bad[:5]], exp[0, bad[:5]])
    n = 4340
    flat = device(x[0, :n].reshape(5, 868))                             # contiguous, cols % 4 == 0: flat 16-byte path
    out = torch.zeros((5, 868), dtype=torch.uint8, device='cuda')
    scale(flat, vmin, denom, out)
    np.testing.assert_array_equal(out.cpu().numpy().ravel(), exp[0, :n])
    wide = torch.full((5, 872), float('inf'), dtype=torch.float32, device='cuda')
    wide[:, :868] = flat
    out = torch.zeros((5, 868), dtype=torch.uint8, device='cuda')
    scale(wide[:, :868], vmin, denom, out)                              # stride 872: row-wise 16-byte path
    np.testing.assert_array_equal(out.cpu().numpy().ravel(), exp[0, :n])


def test_scale_with_odd_denominators():
    """vmax - vmin of 0, NaN, +-inf and a subnormal, against the oracle."""
    import torch
    x = np.concatenate([cases.scale_probes(*cases.SCALE_PAIRS[0]), cases.scale_probes(*cases.SCALE_PAIRS[2])], axis=1)
    t = device(x)
    for vmin, vmax in cases.SCALE_ODD_DENOMS:
        vmin, vmax = np.float32(vmin), np.float32(vmax)
        exp, _, _ = so.get_uint8_image(x.copy(), vmin, vmax, 0, 0)
        with np.errstate(all='ignore'):
            denom = np.float32(vmax - vmin)
        out = torch.full(x.shape, 7, dtype=torch.uint8, device='cuda')
        scale(t, vmin, denom, out)
        np.testing.assert_array_equal(out.cpu().numpy(), exp, err_msg='vmin %r vmax %r' % (vmin, vmax))


def test_public_call_on_every_case():
    """lib.get_uint8_image on every sampler and key-space case, from a NumPy array and from a strided device view, against the
    oracle and - where the reference's own result is defined - against fixture g6b.  (50, 50): pmin == pmax, duplicate hints."""
    import torch
    stored, _ = cases.golden_g6b()
    hits = 0
    for name, img in sorted(cases.public_cases().items()):
        rows, cols = img.shape
        parent = torch.full((rows + 3, cols + 5), float('inf'), dtype=torch.float32, device='cuda')
        view = parent[1:1 + rows, 3:3 + cols]
        view[...] = device(img)
        for pi, (pmin, pmax) in enumerate(cases.PERCENTILE_PAIRS):
            exp, _, _ = so.get_uint8_image(img.copy(), None, None, pmin, pmax)
            with np.errstate(all='ignore'):
                got = quiet(lib.get_uint8_image, np.array(img), None, None, pmin, pmax)
                got_view = quiet(lib.get_uint8_image, view, None, None, pmin, pmax)
            what = '%s (%s, %s)' % (name, pmin, pmax)
            assert got.dtype == np.uint8 and got_view.is_cuda and got_view.dtype == torch.uint8
            np.testing.assert_array_equal(got, exp, err_msg=what)
            np.testing.assert_array_equal(got_view.cpu().numpy(), exp, err_msg=what + ' (device view)')
            key = 'out_%s_%d' % (name, pi)
            if key in stored:
                cases.g6b_equal(stored, key, got)
                hits += 1
        assert bool(torch.isinf(parent[0]).all()) and bool(torch.isinf(parent[:, :3]).all())
    assert hits == len(stored)
    zeros = quiet(lib.get_uint8_image, np.array(cases.sampler_cases()['all_nan']), None, None, 10, 99)
    assert zeros.shape == (40, 52) and not zeros.any()
