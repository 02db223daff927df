"""The specification of include/sid_track.h in NumPy - the only restatement the tests use.  No tests in here.

It is tests/warp_spec.py asked at arbitrary points: the usable nodes, the triangles (grid_spec.grid_triangles), the ownership
rule (warp_spec.owned_by) and the interpolant (warp_spec.source_of) are that module's.  What is added:

    examined   a cell with at least three usable nodes, for the point (px, py), iff floor(min) - 1 <= p <= ceil(max) + 1 on
               both axes (min, max over its usable nodes; no clip)
    owner      of the triangles with det > 0 of examined cells that own the point, the one with the lowest 2 * cell + slot
    closed     when no triangle owns the point: the lowest-numbered one of an examined cell with Ed >= 0 on all three edges
    result     sx, sy of the triangle that has the point, tri = 2 * cell + slot; NaN, NaN, -1 when none has it or the point
               is not finite; a result that is not a number is the quiet NaN

Every cell is looked at for every point: no search."""
import numpy as np

from tests import grid_spec as gs
from tests import warp_spec as ws


def edge_sides(xf, yf, tri, px, py):
    """Ed of the three directed edges a -> b, b -> c, c -> a (the E of warp_spec.owned_by, signed towards the triangle)."""
    a, b, c = [int(q) for q in tri]
    out = []
    for p, q in ((a, b), (b, c), (c, a)):
        lo, hi = (p, q) if p < q else (q, p)
        E = (xf[hi] - xf[lo]) * (py - yf[lo]) - (yf[hi] - yf[lo]) * (px - xf[lo])
        out.append(E if p == lo else -E)
    return out


def track(x, y, xs, ys, valid, diagonal, px, py, closed=True):
    """-> dict: sx, sy (float64), tri (int32) of px's shape, and for the tests owners (int32: how many triangles own each
    point), shut (bool: the point has its result from the closed rule), triangles (the t of grid_spec.grid_triangles)."""
    x, y, xs, ys = [np.asarray(q, dtype=np.float64) for q in (x, y, xs, ys)]
    shape = np.shape(px)
    px, py = np.asarray(px, dtype=np.float64).ravel(), np.asarray(py, dtype=np.float64).ravel()
    n = px.size
    ok = ws.usable(x, y, xs, ys, valid)
    t = gs.grid_triangles(x, y, ok, diagonal)
    xf, yf, xsf, ysf, okf = x.ravel(), y.ravel(), xs.ravel(), ys.ravel(), ok.ravel()
    res = [dict(sx=np.full(n, np.nan), sy=np.full(n, np.nan), tri=np.full(n, -1, dtype=np.int32)) for _ in range(2)]   # owner, closed
    owners = np.zeros(n, dtype=np.int32)
    finite = np.isfinite(px) & np.isfinite(py)
    rows, cols = x.shape if x.ndim == 2 else (0, 0)
    with np.errstate(all='ignore'):
        for i in range(rows - 1):
            for j in range(cols - 1):
                A = i * cols + j
                ring = [m for m in (A, A + 1, A + cols + 1, A + cols) if okf[m]]
                if len(ring) < 3:
                    continue
                xl, xh = np.floor(xf[ring].min()) - 1.0, np.ceil(xf[ring].max()) + 1.0
                yl, yh = np.floor(yf[ring].min()) - 1.0, np.ceil(yf[ring].max()) + 1.0
                sel = np.nonzero(finite & (xl <= px) & (px <= xh) & (yl <= py) & (py <= yh))[0]
                if not sel.size:
                    continue
                qx, qy = px[sel], py[sel]
                for s in range(2):
                    tri = t[i, j, s]
                    if tri[0] < 0:
                        continue
                    a, b, c = [int(q) for q in tri]
                    det = (xf[b] - xf[a]) * (yf[c] - yf[a]) - (xf[c] - xf[a]) * (yf[b] - yf[a])
                    if not det > 0:
                        continue
                    own = ws.owned_by(xf, yf, tri, qx, qy)
                    owners[sel[own]] += 1
                    d0, d1, d2 = edge_sides(xf, yf, tri, qx, qy)
                    for r, has in ((res[0], own), (res[1], (d0 >= 0) & (d1 >= 0) & (d2 >= 0))):
                        first = has & (r['tri'][sel] < 0)                      # cells and slots come in ascending number
                        if first.any():
                            sx, sy = ws.source_of(xf, yf, xsf, ysf, tri, qx[first], qy[first])
                            r['sx'][sel[first]], r['sy'][sel[first]] = sx, sy
                            r['tri'][sel[first]] = 2 * (i * (cols - 1) + j) + s
    shut = (res[0]['tri'] < 0) & (res[1]['tri'] >= 0) if closed else np.zeros(n, dtype=bool)
    out = {k: np.where(shut, res[1][k], res[0][k]) for k in ('sx', 'sy', 'tri')}
    for k in ('sx', 'sy'):
        out[k] = np.where(np.isnan(out[k]), np.nan, out[k]).reshape(shape)
    out['tri'] = out['tri'].astype(np.int32).reshape(shape)
    out.update(owners=owners.reshape(shape), shut=shut.reshape(shape), triangles=t)
    return out


def same_bits(a, b):
    return ws.same_bits(a, b)
