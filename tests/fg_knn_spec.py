"""The specification of sid_fg_knn (include/sid_fg.h) in NumPy - the only restatement the tests use.  No tests in here.

    usable seed   both coordinates and both values finite; the others never take part.
    d2            dx = q0 - s0 ; dy = q1 - s1 ; d2 = dx*dx + dy*dy
    admissible    d2 <= m2, m2 = max_dist * max_dist (None / inf: no limit)
    neighbours    the first m = min(k, #admissible usable seeds) in ascending (d2, seed index) order: np.lexsort((idx, d2))
    result        per component the median of the neighbours' values (tests/grid_spec.py's: m odd s[m//2], m even
                  (s[m/2-1] + s[m/2]) / 2.0); m = 0 or a query that is not finite: NaN, NaN, count 0, index all -1.

Every operation is one IEEE double rounding (NumPy neither fuses nor reorders them)."""
import numpy as np


def median(values):
    s = np.sort(np.asarray(values, dtype=np.float64))
    n = len(s)
    assert n >= 1
    if n % 2:
        return s[n // 2]
    return (s[n // 2 - 1] + s[n // 2]) / np.float64(2.0)


def knn(seeds, values, q, k=5, max_dist=None):
    """-> out float64 [n_q, 2], count int32 [n_q], index int32 [n_q, k], d2 of the neighbours float64 [n_q, k] (NaN padded)."""
    seeds = np.asarray(seeds, dtype=np.float64).reshape(-1, 2)
    values = np.asarray(values, dtype=np.float64).reshape(-1, 2)
    q = np.asarray(q, dtype=np.float64).reshape(-1, 2)
    m2 = np.float64(np.inf if max_dist is None else max_dist) * np.float64(np.inf if max_dist is None else max_dist)
    usable = np.flatnonzero(np.isfinite(seeds).all(axis=1) & np.isfinite(values).all(axis=1))
    s, v = seeds[usable], values[usable]
    out = np.full((len(q), 2), np.nan)
    count = np.zeros(len(q), dtype=np.int32)
    index = np.full((len(q), k), -1, dtype=np.int32)
    dist2 = np.full((len(q), k), np.nan)
    with np.errstate(all='ignore'):
        for i in range(len(q)):
            if not np.isfinite(q[i]).all():
                continue
            dx = q[i, 0] - s[:, 0]
            dy = q[i, 1] - s[:, 1]
            d2 = dx * dx + dy * dy
            ok = np.flatnonzero(d2 <= m2)
            order = ok[np.lexsort((usable[ok], d2[ok]))][:k]
            m = len(order)
            count[i] = m
            index[i, :m] = usable[order]
            dist2[i, :m] = d2[order]
            if m:
                out[i, 0] = median(v[order, 0])
                out[i, 1] = median(v[order, 1])
    return out, count, index, dist2


def same_bits(got, exp):
    """Equal shapes, NaN in the same places, identical float64 bit patterns everywhere else (signed zeros included)."""
    got, exp = np.asarray(got, dtype=np.float64), np.asarray(exp, dtype=np.float64)
    if got.shape != exp.shape:
        return False
    gn, en = np.isnan(got), np.isnan(exp)
    return bool(np.array_equal(gn, en) and np.array_equal(got[~gn].view(np.int64), exp[~en].view(np.int64)))


def check(got, seeds, values, q, k=5, max_dist=None):
    """Assert that got = (out, count, index) of _capi.fg_knn(..., details=True) is the specification's, bit for bit; returns
    the specification's tuple (with d2) for further assertions."""
    exp = knn(seeds, values, q, k, max_dist)
    np.testing.assert_array_equal(got[1], exp[1])
    np.testing.assert_array_equal(got[2], exp[2])
    assert got[1].dtype == np.int32 and got[2].dtype == np.int32
    assert same_bits(got[0], exp[0])
    return exp
