"""GPU: the Hamming matcher (include/sid_ft.h) on the constructed cases of tests/ft_cases.py - every assertion an equality.
Each case names the plan it must take (sid_ft_debug_plan), the results it knows by construction and the queries compared with the
oracle (tests/test_ft_cases_host.py shows on the CPU that the cases are what they claim).  The device entry runs between guard
regions on a stream of its own, with a workspace of exactly sid_ft_workspace_bytes; the staging pool is reused across sizes
and forms."""
import numpy as np
import pytest

from sea_ice_drift_amd import _capi
from tests import ft_cases as fc

pytestmark = pytest.mark.gpu

GUARD = 4096


def run(monkeypatch, c, no_mfma=False):
    monkeypatch.delenv('SID_FT_NO_MFMA', raising=False)
    for k, v in c['env'].items():
        monkeypatch.setenv(k, v)
    if no_mfma:
        monkeypatch.setenv('SID_FT_NO_MFMA', '1')
    plan = _capi.ft_debug_plan(len(c['d1']), len(c['d2']))
    idx, dist = _capi.ft_knn2(c['d1'], c['d2'])
    monkeypatch.delenv('SID_FT_NO_MFMA', raising=False)
    return plan, idx, dist


@pytest.mark.parametrize('name', fc.names())
def test_case_takes_its_plan_and_equals_the_oracle(monkeypatch, name):
    c = fc.case(name)
    plan, idx, dist = run(monkeypatch, c)
    assert plan == c['plan']
    for q, slot, j, d in c['claims']:
        assert (int(idx[q, slot]), int(dist[q, slot])) == (j, d), (q, slot)
    sel, eidx, edist = fc.oracle(name)
    np.testing.assert_array_equal(dist[sel], edist)
    np.testing.assert_array_equal(idx[sel], eidx)
    if c['plan']['mfma']:                                                  # the other form on the same input: every query
        vplan, vidx, vdist = run(monkeypatch, c, no_mfma=True)
        assert vplan == fc.plan_spec(len(c['d1']), len(c['d2']), True) and vplan['mfma'] == 0
        np.testing.assert_array_equal(dist, vdist)
        np.testing.assert_array_equal(idx, vidx)


def guarded(torch, nbytes, fill=None):
    """A device buffer of nbytes between two guards of 0xAB, inside one larger allocation: (whole, payload view)."""
    whole = torch.full((GUARD + nbytes + GUARD,), 0xAB, dtype=torch.uint8, device='cuda')
    body = whole[GUARD:GUARD + nbytes]
    if fill is not None:
        body.copy_(torch.from_numpy(np.array(fill).view(np.uint8).reshape(-1)))      # (np.array: a writable copy)
    return whole, body


@pytest.mark.parametrize('name', ['valu_257x513', 'mfma_32768x1025'])
def test_device_entry_between_guards_on_its_own_stream(monkeypatch, name):
    """sid_ft_knn2_device on torch tensors: descriptors, workspace (exactly sid_ft_workspace_bytes) and both outputs each lie
    inside a larger allocation between 4096-byte guards.  The results are the host entry's and no guard byte changed: neither
    form writes outside its workspace plan or its outputs.  Descriptors off by 8 bytes, and in the MFMA form a workspace off by
    8 bytes, are SID_PM_ERR_ARG before any launch."""
    import torch
    c = fc.case(name)
    n1, n2 = len(c['d1']), len(c['d2'])
    plan, hidx, hdist = run(monkeypatch, c)
    assert plan == c['plan']
    ws_bytes = _capi.ft_workspace_bytes(n1, n2)
    assert ws_bytes == fc.workspace_spec(n1, n2)
    w1, b1 = guarded(torch, 32 * n1, c['d1'])
    w2, b2 = guarded(torch, 32 * n2, c['d2'])
    wws, bws = guarded(torch, ws_bytes)
    wi, bi = guarded(torch, 8 * n1)
    wd, bd = guarded(torch, 8 * n1)
    for b in (b1, b2, bws, bi, bd):
        assert b.data_ptr() % 16 == 0
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    assert stream.cuda_stream != 0
    with torch.cuda.stream(stream):
        _capi.ft_knn2_device(b1.data_ptr(), n1, b2.data_ptr(), n2, bi.data_ptr(), bd.data_ptr(), bws.data_ptr(), stream.cuda_stream)
    stream.synchronize()
    np.testing.assert_array_equal(bi.cpu().numpy().view(np.int32).reshape(n1, 2), hidx)
    np.testing.assert_array_equal(bd.cpu().numpy().view(np.int32).reshape(n1, 2), hdist)
    for whole, body in ((w1, b1), (w2, b2), (wws, bws), (wi, bi), (wd, bd)):
        g = whole.cpu().numpy()
        assert (g[:GUARD] == 0xAB).all() and (g[GUARD + body.numel():] == 0xAB).all()
    np.testing.assert_array_equal(b1.cpu().numpy().reshape(n1, 32), c['d1'])  # (the inputs are read only)
    np.testing.assert_array_equal(b2.cpu().numpy().reshape(n2, 32), c['d2'])
    # refused before any launch: the outputs keep what they hold
    before = bi.clone()
    for p1, p2, pw in ((8, 0, 0), (0, 8, 0)) + (((0, 0, 8),) if c['plan']['mfma'] else ()):
        with pytest.raises(_capi.SidPmError) as e:
            _capi.ft_knn2_device(b1.data_ptr() + p1, n1, b2.data_ptr() + p2, n2, bi.data_ptr(), bd.data_ptr(), bws.data_ptr() + pw,
                                 stream.cuda_stream)
        assert e.value.code == -1 and 'aligned' in str(e.value)
    stream.synchronize()
    assert torch.equal(bi, before)


def test_pool_is_reused_across_sizes_and_forms(monkeypatch):
    """The staging block of the host entry grows and is carved anew per call: a large MFMA call, two small ones and the large
    one again give, call for call, what each gives on a pool that was released just before."""
    order = ['mfma_32768x1025', 'valu_1x2', 'valu_257x513', 'mfma_32768x1025']
    L = _capi.lib()
    warm = [run(monkeypatch, fc.case(n)) for n in order]
    cold = []
    for n in order:
        assert L.sid_ft_release(0) == 0
        cold.append(run(monkeypatch, fc.case(n)))
    for n, (wp, wi, wd), (cp, ci, cd) in zip(order, warm, cold):
        assert wp == cp == fc.case(n)['plan']
        np.testing.assert_array_equal(wi, ci)
        np.testing.assert_array_equal(wd, cd)
    np.testing.assert_array_equal(warm[0][1], warm[3][1])
    np.testing.assert_array_equal(warm[0][2], warm[3][2])
    sel, eidx, edist = fc.oracle('valu_257x513')
    np.testing.assert_array_equal(warm[2][1][sel], eidx)
    np.testing.assert_array_equal(warm[2][2][sel], edist)
