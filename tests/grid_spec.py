"""The specification of include/sid_grid.h in NumPy - the only restatement the tests use.  No tests in here.

Usable node: (valid is None or valid[i, j] != 0) and u, v finite (the filter); x and y finite as well (the deformation).
median(n >= 1 values): sorted s; n odd: s[(n-1)/2]; n even: (s[n/2-1] + s[n/2]) / 2.0.

    nmt: for a usable node, N = the usable nodes of the (2 radius + 1)^2 window, centre excluded, clipped at the edges;
         |N| < min_neighbours: res = NaN, keep = False; else
             um = median(u_N) ; mu = median(|u_N - um|) ; ru = |u - um| / (mu + eps)       (rv: the same with v)
             res = sqrt(ru*ru + rv*rv) ; keep = res <= threshold
         unusable nodes: res = NaN, keep = False.
    grid_triangles: cell (i, j), A = i*C + j, B = A + 1, D = A + C, E = D + 1, ring A, B, E, D.  Four usable nodes:
         dm = (xE-xA)*(xE-xA) + (yE-yA)*(yE-yA), da = (xD-xB)*(xD-xB) + (yD-yB)*(yD-yB); anti split (A, B, D), (B, E, D) for
         'anti' or for 'shorter' with da < dm, else main split (A, B, E), (A, E, D).  Three usable: slot 0 = those three in ring
         order.  Each triangle (a, b, c) with cr = (xb-xa)*(yc-ya) - (xc-xa)*(yb-ya) < 0 has b and c swapped.
    deformation: the reference's get_deformation_on_triangulation (restated below, operation for operation) on the present
         triangles; absent slots hold NaN and -1.

Every operation is one IEEE double rounding (np.float64 scalars: NumPy neither fuses nor reorders them)."""
import numpy as np

KEYS = ('e1', 'e2', 'e3', 'a', 'p')


def usable_uv(u, v, valid):
    ok = np.isfinite(u) & np.isfinite(v)
    return ok if valid is None else ok & (np.asarray(valid) != 0)


def usable_xyuv(x, y, u, v, valid):
    return usable_uv(u, v, valid) & np.isfinite(x) & np.isfinite(y)


def median(values):
    s = np.sort(np.asarray(values, dtype=np.float64))
    n = len(s)
    assert n >= 1
    if n % 2:
        return s[n // 2]
    return (s[n // 2 - 1] + s[n // 2]) / np.float64(2.0)


def nmt(u, v, valid, eps, threshold, radius, min_neighbours):
    """-> keep (bool), res (float64), both of u's shape."""
    u, v = np.asarray(u, dtype=np.float64), np.asarray(v, dtype=np.float64)
    rows, cols = u.shape
    ok = usable_uv(u, v, valid)
    keep, res = np.zeros((rows, cols), dtype=bool), np.full((rows, cols), np.nan)
    eps, threshold = np.float64(eps), np.float64(threshold)
    with np.errstate(all='ignore'):
        for i in range(rows):
            for j in range(cols):
                if not ok[i, j]:
                    continue
                un, vn = [], []
                for ii in range(max(i - radius, 0), min(i + radius, rows - 1) + 1):
                    for jj in range(max(j - radius, 0), min(j + radius, cols - 1) + 1):
                        if (ii, jj) != (i, j) and ok[ii, jj]:
                            un.append(u[ii, jj])
                            vn.append(v[ii, jj])
                if len(un) < min_neighbours:
                    continue
                r = []
                for c, cn in ((u[i, j], np.array(un)), (v[i, j], np.array(vn))):
                    m = median(cn)
                    mad = median(np.abs(cn - m))
                    r.append(np.abs(c - m) / (mad + eps))
                res[i, j] = np.sqrt(r[0] * r[0] + r[1] * r[1])
                keep[i, j] = res[i, j] <= threshold
    return keep, res


def grid_triangles(x, y, usable, diagonal):
    """-> t (R-1, C-1, 2, 3) int32, -1 where a slot holds no triangle."""
    assert diagonal in ('shorter', 'main', 'anti')
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    rows, cols = x.shape
    t = np.full((max(rows - 1, 0), max(cols - 1, 0), 2, 3), -1, dtype=np.int32)
    xf, yf, uf = x.ravel(), y.ravel(), np.asarray(usable).ravel()
    with np.errstate(all='ignore'):
        for i in range(rows - 1):
            for j in range(cols - 1):
                A = i * cols + j
                B, D = A + 1, A + cols
                E = D + 1
                ring = [n for n in (A, B, E, D) if uf[n]]
                if len(ring) == 4:
                    dm = (xf[E] - xf[A]) * (xf[E] - xf[A]) + (yf[E] - yf[A]) * (yf[E] - yf[A])
                    da = (xf[D] - xf[B]) * (xf[D] - xf[B]) + (yf[D] - yf[B]) * (yf[D] - yf[B])
                    if diagonal == 'anti' or (diagonal == 'shorter' and da < dm):
                        tris = [(A, B, D), (B, E, D)]
                    else:
                        tris = [(A, B, E), (A, E, D)]
                elif len(ring) == 3:
                    tris = [tuple(ring)]
                else:
                    tris = []
                for s, (a, b, c) in enumerate(tris):
                    cr = (xf[b] - xf[a]) * (yf[c] - yf[a]) - (xf[c] - xf[a]) * (yf[b] - yf[a])
                    if cr < 0:
                        b, c = c, b
                    t[i, j, s] = (a, b, c)
    return t


# NumPy restatement of the reference's libdefor.py: the same operations in the same order
def np_elems(xt, yt, ut, vt, a):
    ux = uy = vx = vy = 0
    for i0, i1 in zip([1, 2, 0], [0, 1, 2]):
        ux = ux + (ut[i0] + ut[i1]) * (yt[i0] - yt[i1])
        uy = uy - (ut[i0] + ut[i1]) * (xt[i0] - xt[i1])
        vx = vx + (vt[i0] + vt[i1]) * (yt[i0] - yt[i1])
        vy = vy - (vt[i0] + vt[i1]) * (xt[i0] - xt[i1])
    ux, uy, vx, vy = [i / (2 * a) for i in (ux, uy, vx, vy)]
    return ux + vy, ((ux - vy) ** 2 + (uy + vx) ** 2) ** 0.5, vx - uy


def np_triangulation(x, y, u, v, t):
    xt, yt, ut, vt = [i[t].T for i in (x, y, u, v)]
    sx = [xt[1] - xt[0], xt[2] - xt[1], xt[0] - xt[2]]
    sy = [yt[1] - yt[0], yt[2] - yt[1], yt[0] - yt[2]]
    s = [np.hypot(sx[k], sy[k]) for k in range(3)]
    p = (s[0] + s[1]) + s[2]
    h = p / 2
    a = np.sqrt(h * (h - s[0]) * (h - s[1]) * (h - s[2]))
    return np_elems(xt, yt, ut, vt, a) + (a, p)


def present(t):
    """The slots of t that hold a triangle (bool (R-1, C-1, 2)) and those triangles (M, 3) in slot order (row-major)."""
    has = t[..., 0] >= 0
    return has, np.ascontiguousarray(t[has])


def scatter(t, flat):
    """The (5, M) values of the present triangles, in slot order, into five (R-1, C-1, 2) arrays with NaN elsewhere."""
    has, _ = present(t)
    out = []
    for row in flat:
        full = np.full(has.shape, np.nan)
        full[has] = row
        out.append(full)
    return tuple(out)


def deformation(x, y, u, v, valid, diagonal, on_triangulation=np_triangulation):
    """-> e1, e2, e3, a, p (R-1, C-1, 2) float64 and t (R-1, C-1, 2, 3) int32.  `on_triangulation` computes the present
    triangles: the restatement above, or the reference's own function."""
    x, y, u, v = [np.asarray(q, dtype=np.float64) for q in (x, y, u, v)]
    t = grid_triangles(x, y, usable_xyuv(x, y, u, v, valid), diagonal)
    _, tri = present(t)
    with np.errstate(all='ignore'):
        flat = on_triangulation(x.ravel(), y.ravel(), u.ravel(), v.ravel(), tri) if len(tri) else [np.empty(0)] * 5
    return scatter(t, np.asarray(flat).reshape(5, -1)) + (t,)


def same_bits(got, exp):
    """Equal shapes, NaN in the same places, identical float64 bit patterns everywhere else (signed zeros included)."""
    got, exp = np.asarray(got, dtype=np.float64), np.asarray(exp, dtype=np.float64)
    if got.shape != exp.shape:
        return False
    gn, en = np.isnan(got), np.isnan(exp)
    return bool(np.array_equal(gn, en) and np.array_equal(got[~gn].view(np.int64), exp[~en].view(np.int64)))
