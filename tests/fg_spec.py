"""Specification of the first-guess evaluation (include/sid_fg.h: sid_fg_interp_linear, sid_fg_nearest_dist,
sid_fg_distance_image) in NumPy: csrc/first_guess.hip restated, one IEEE double rounding per operation in the order written.
The library is built with -ffp-contract=off; its only fused operations are the two fma calls of k_transform, taken here as the
exact rational a * b + c rounded once.  fmin ignores a NaN operand (np.fmin does too).  The device must equal this bit for
bit; tests/test_fg_spec_host.py holds it against SciPy on the CPU.  No tests in here."""
from fractions import Fraction

import numpy as np

EPS = 100.0 * np.finfo(np.float64).eps      # SciPy's location tolerance: a simplex contains a query when min c >= -EPS
KTOL = 1e-9                                 # queries with a smallest coordinate in [-KTOL, KTOL) are flagged
NONE = -1
F = np.float64


def fma(a, b, c):
    """a * b + c with ONE rounding."""
    a, b, c = F(a), F(b), F(c)
    if not (np.isfinite(a) and np.isfinite(b) and np.isfinite(c)):
        return a * b + c                                                   # (NaN and infinities come out of the plain form alike)
    if a == 0.0 or b == 0.0:
        return a * b + c                                                   # (exact, and keeps the sign of a zero)
    r = Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c))
    return F(0.0) if r == 0 else F(float(r))                               # (x + (-x) = +0 in round-to-nearest; float(): correctly rounded)


def transform(pts, simplices):
    """k_transform: per simplex (t00, t01, t10, t11, rx, ry) and ok.  LU with partial pivoting of
    M = [[x_a - x_c, y_a - y_c], [x_b - x_c, y_b - y_c]]; Tinv = M^-T."""
    pts = np.asarray(pts, dtype=F)
    T = np.zeros((len(simplices), 6), dtype=F)
    ok = np.zeros(len(simplices), dtype=bool)
    one, zero = F(1.0), F(0.0)
    with np.errstate(all='ignore'):
        for k, (a, b, c) in enumerate(np.asarray(simplices).tolist()):
            rx, ry = pts[c]
            m00, m01, m10, m11 = pts[a, 0] - rx, pts[a, 1] - ry, pts[b, 0] - rx, pts[b, 1] - ry
            swap = abs(m10) > abs(m00)
            if swap:
                m00, m10, m01, m11 = m10, m00, m11, m01
            l = m10 * (one / m00)
            u11 = m11 - l * m01
            ok[k] = m00 != 0.0 and u11 != 0.0 and np.isfinite(l) and np.isfinite(one / u11)
            iu11, iu00 = one / u11, one / m00
            x = [[zero, zero], [zero, zero]]
            for col in range(2):
                b0, b1 = (one, zero) if col == 0 else (zero, one)
                if swap:
                    b0, b1 = b1, b0
                y1 = fma(-l, b0, b1)
                x1 = y1 * iu11
                x0 = fma(-m01, x1, b0) * iu00
                x[0][col], x[1][col] = x0, x1
            T[k] = (x[0][0], x[1][0], x[0][1], x[1][1], rx, ry)
    return T, ok


def coordinates(T, q):
    """c0, c1, c2 [n_simp, n_q] and their NaN-ignoring minimum, as every kernel computes them."""
    x, y = q[None, :, 0], q[None, :, 1]
    with np.errstate(all='ignore'):
        dx, dy = x - T[:, 4, None], y - T[:, 5, None]
        c0 = T[:, 0, None] * dx + T[:, 1, None] * dy
        c1 = T[:, 2, None] * dx + T[:, 3, None] * dy
        c2 = 1.0 - c0 - c1
        mc = np.fmin(c0, np.fmin(c1, c2))
    return c0, c1, c2, mc


def _values(c0, c1, c2, values, s):
    """The value sum in vertex order, both components: arrays over queries for the vertex triples s [n, 3]."""
    with np.errstate(all='ignore'):
        o = c0[:, None] * values[s[:, 0]]
        o = o + c1[:, None] * values[s[:, 1]]
        o = o + c2[:, None] * values[s[:, 2]]
    return o


def _near_half(o):
    with np.errstate(all='ignore'):
        return (np.abs(o - np.floor(o) - 0.5) < 1e-6) | ~(np.abs(o) < 1e15)


def interp_linear(pts, simplices, values, q, details=False):
    """sid_fg_interp_linear: out [n_q, 2], simplex [n_q], doubt [n_q] - k_transform, location (the lowest index of an ok
    simplex with min c >= -EPS), k_eval and k_resolve.  details=True: also a dict with 'flagged' (doubt before k_resolve)."""
    pts, values, q = np.asarray(pts, dtype=F), np.asarray(values, dtype=F), np.asarray(q, dtype=F).reshape(-1, 2)
    simplices = np.asarray(simplices, dtype=np.int64)
    nq = len(q)
    T, ok = transform(pts, simplices)
    c0, c1, c2, mc = coordinates(T, q)
    live = np.isfinite(q).all(axis=1)                                      # a query that is not finite is in no simplex and near none
    with np.errstate(all='ignore'):
        contains = ok[:, None] & live[None, :] & (mc >= -EPS)
        close = ok[:, None] & live[None, :] & (mc >= -KTOL)
    located = contains.any(axis=0)
    k = np.where(located, contains.argmax(axis=0), 0)
    ar = np.arange(nq)
    # k_eval
    o = _values(c0[k, ar], c1[k, ar], c2[k, ar], values, simplices[k])
    with np.errstate(all='ignore'):
        dbt = (mc[k, ar] < KTOL) | _near_half(o).any(axis=1)
    out = np.where(located[:, None], o, np.nan)
    simplex = np.where(located, k, NONE).astype(np.int32)
    doubt = np.where(located, dbt, close.any(axis=0))
    flagged = doubt.copy()
    # k_resolve: the flagged queries against every ok simplex
    for i in np.nonzero(flagged)[0]:
        cand = close[:, i]
        with np.errstate(all='ignore'):
            hull_unclear = (cand & (np.abs(mc[:, i] + EPS) < 4e-15)).any()
        ks = np.nonzero(contains[:, i])[0]
        oi = _values(c0[ks, i], c1[ks, i], c2[ks, i], values, simplices[ks])
        r = np.rint(oi)
        near_half = _near_half(oi).any()
        disagree = len(ks) > 0 and not (r == r[0]).all()
        if hull_unclear or disagree or near_half:
            continue
        out[i] = oi[0] if len(ks) else np.nan
        simplex[i] = ks[0] if len(ks) else NONE
        doubt[i] = False
    if details:
        return out, simplex, doubt, dict(flagged=flagged, T=T, ok=ok, mc=mc)
    return out, simplex, doubt


def nearest_dist(seeds, q):
    """sid_fg_nearest_dist: sqrt of the smallest dx dx + dy dy over the seeds; a sum that is not a number is never the smallest
    (+inf when none is a number)."""
    seeds, q = np.asarray(seeds, dtype=F).reshape(-1, 2), np.asarray(q, dtype=F).reshape(-1, 2)
    with np.errstate(all='ignore'):
        dx, dy = q[:, None, 0] - seeds[None, :, 0], q[:, None, 1] - seeds[None, :, 1]
        d2 = dx * dx + dy * dy
        return np.sqrt(np.fmin.reduce(d2, axis=1, initial=np.inf))


def distance_image(seeds, rows, cols):
    """sid_fg_distance_image: pixel i of the image is the query (row i / cols, column i % cols)."""
    r, c = np.divmod(np.arange(rows * cols), cols)
    return nearest_dist(seeds, np.stack([r, c], axis=1).astype(F)).reshape(rows, cols)


GRID = 128                                  # cells per axis of the bucket grid over the bounding box of the key points


def bucket_entries(pts, simplices, ok):
    """What the bucket lists of the point location hold (k_grid_build): every ok simplex is listed in the cells its bounding
    box, widened by m, touches.  Returns (entries, capacity) - the lists are used when entries <= capacity = 8 n_simp + GRID^2 -
    or None where no grid is laid (a bounding box of the key points without area)."""
    pts = np.asarray(pts, dtype=F)
    lo, hi = pts.min(axis=0), pts.max(axis=0)
    w, h = hi - lo
    if not (w > 0.0 and h > 0.0 and np.isfinite(w) and np.isfinite(h)):
        return None
    inv = (F(GRID) / w, F(GRID) / h)
    p = pts[np.asarray(simplices, dtype=np.int64)]
    x_lo, x_hi, y_lo, y_hi = p[:, :, 0].min(axis=1), p[:, :, 0].max(axis=1), p[:, :, 1].min(axis=1), p[:, :, 1].max(axis=1)
    m = 1e-6 * ((x_hi - x_lo) + (y_hi - y_lo)) + 1e-9 * (np.abs(x_hi) + np.abs(x_lo) + np.abs(y_hi) + np.abs(y_lo)) + 1e-12
    cell = lambda v, axis: np.clip(np.floor((v - lo[axis]) * inv[axis]), 0, GRID - 1).astype(np.int64)
    n = (cell(x_hi + m, 0) - cell(x_lo - m, 0) + 1) * (cell(y_hi + m, 1) - cell(y_lo - m, 1) + 1)
    return int(n[np.asarray(ok, dtype=bool)].sum()), 8 * len(p) + GRID * GRID
