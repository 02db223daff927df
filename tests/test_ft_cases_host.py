"""CPU: every case of tests/ft_cases.py is what it claims.  The results a case knows by construction are those of the oracle
(oracle/ft_oracle.py: the pure-Python loops up to 300 x 600, the NumPy scan on the asserted queries of the large cases), and
the plans written into the cases as literal numbers are those of a Python restatement of csrc/ft_plan.h."""
import numpy as np
import pytest

from oracle import ft_oracle as fo
from tests import ft_cases as fc


oracle = fc.oracle


@pytest.mark.parametrize('name', fc.names())
def test_claims_are_the_oracles(name):
    c = fc.case(name)
    sel, idx, dist = oracle(name)
    assert len(sel) <= 1024 and len(c['claims']) > 0
    row = {int(q): k for k, q in enumerate(sel)}
    for q, slot, j, d in c['claims']:
        assert (int(idx[row[q], slot]), int(dist[row[q], slot])) == (j, d), (name, q, slot)


@pytest.mark.parametrize('name', fc.names())
def test_plans_in_the_tables_are_the_headers(name):
    c = fc.case(name)
    n1, n2 = len(c['d1']), len(c['d2'])
    assert fc.plan_spec(n1, n2, bool(c['env'])) == c['plan']
    if c['plan']['mfma']:
        assert n1 * n2 >= 1 << 24 and n2 >= 1024 and not c['env']
        assert fc.plan_spec(n1, n2, True)['mfma'] == 0


def test_the_tables_of_the_cases():
    """Shapes and plans as listed for the two forms: the sizes on either side of the switch, the chunk that is no multiple of
    the unroll with its short last chunk, the batches per chunk of the ragged MFMA case."""
    shape = {c['name']: (len(c['d1']), len(c['d2']), c['plan']['mfma'], c['plan']['chunk'], c['plan']['nchunks']) for c in fc.cases()}
    assert shape['valu_1x2'] == (1, 2, 0, 2, 1) and shape['valu_1x255'] == (1, 255, 0, 255, 1) and shape['valu_255x256'] == (255, 256, 0, 256, 1)
    assert shape['valu_256x257'] == (256, 257, 0, 256, 2) and shape['valu_257x513'] == (257, 513, 0, 256, 3)
    assert shape['valu_300x1025'] == (300, 1025, 0, 256, 5)
    assert shape['valu_16384x8200_chunk257'] == (16384, 8200, 0, 257, 32) and 8200 - 31 * 257 == 233
    assert shape['valu_16383x1024'] == (16383, 1024, 0, 256, 4) and 16383 * 1024 == (1 << 24) - 1024
    assert shape['valu_16401x1023'] == (16401, 1023, 0, 256, 4) and 16401 * 1023 > 1 << 24
    assert shape['mfma_16384x1024'] == (16384, 1024, 1, 256, 4) and 16384 * 1024 == 1 << 24
    assert shape['mfma_16385x1024'] == (16385, 1024, 1, 256, 4) and fc.case('mfma_16385x1024')['plan']['n1pad'] == 16640
    p = fc.case('mfma_32768x1025')['plan']
    assert (p['n2pad'], p['chunk'], p['nchunks']) == (1280, 512, 3)           # batches per chunk: 2, 2, 1
    assert shape['mfma_8193x2049'] == (8193, 2049, 1, 256, 9)
    assert fc.workspace_spec(1000, 1000) == 8 * 1000 * 4 + 256 * 1024 * 2 + 4 * 1024


def test_the_library_plans_and_sizes_as_the_restatement(monkeypatch):
    """sid_ft_debug_plan and sid_ft_workspace_bytes are host arithmetic: no device is needed to hold them against the
    restatement, for every case and with the switch set and unset."""
    from sea_ice_drift_amd import _capi
    for c in fc.cases():
        n1, n2 = len(c['d1']), len(c['d2'])
        for no_mfma in (False, True):
            if no_mfma:
                monkeypatch.setenv('SID_FT_NO_MFMA', '1')
            else:
                monkeypatch.delenv('SID_FT_NO_MFMA', raising=False)
            assert _capi.ft_debug_plan(n1, n2) == fc.plan_spec(n1, n2, no_mfma), (c['name'], no_mfma)
            assert _capi.ft_workspace_bytes(n1, n2) == fc.workspace_spec(n1, n2), c['name']
    monkeypatch.delenv('SID_FT_NO_MFMA', raising=False)
    for n1, n2, code in ((-1, 5, -1), (5, -1, -1), (5, 1 << 22, -4), ((1 << 29), 5, -4)):
        with pytest.raises(_capi.SidPmError) as e:
            _capi.ft_debug_plan(n1, n2)
        assert e.value.code == code, (n1, n2)
    assert _capi.ft_debug_plan(5, (1 << 22) - 1)['n2pad'] == 1 << 22 and _capi.lib().sid_ft_debug_plan(1, 1, None) == -1


def test_background_is_far_from_everything():
    """No random descriptor comes near a planted distance: the claims stand on the construction alone."""
    for name in ('valu_257x513', 'valu_300x1025'):
        c = fc.case(name)
        _, idx, dist = oracle(name)
        claimed = {q for q, _, _, _ in c['claims']}
        others = np.array([q for q in range(len(c['d1'])) if q not in claimed])
        assert dist[others].min() > 60
