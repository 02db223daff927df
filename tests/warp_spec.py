"""The specification of include/sid_warp.h in NumPy - the only restatement the tests use.  No tests in here.

Usable node: (valid is None or valid != 0) and x, y, xs, ys finite.  Triangles: grid_spec.grid_triangles on (x, y).
A cell is examined over the pixels floor(min) - 1 .. ceil(max) + 1 of its usable nodes (per axis, clipped to the output).
For a triangle (a, b, c) with det = (xb-xa)*(yc-ya) - (xc-xa)*(yb-ya) > 0 and a pixel (r, c), px = c, py = r:

    edge p -> q (a -> b, b -> c, c -> a), lo / hi its endpoints by flat node number:
        E = (x_hi - x_lo)*(py - y_lo) - (y_hi - y_lo)*(px - x_lo) ; Ed = E if p is lo else -E
        inside iff Ed > 0 or (Ed == 0 and (dy > 0 or (dy == 0 and dx > 0))),  dx = x_q - x_p, dy = y_q - y_p
    owned iff inside all three edges
    l1 = ((px-xa)*(yc-ya) - (xc-xa)*(py-ya)) / det ; l2 = ((xb-xa)*(py-ya) - (px-xa)*(yb-ya)) / det
    sx = xs_a + l1*(xs_b - xs_a) + l2*(xs_c - xs_a) ; sy likewise
    order 0: jc = rint(sx), jr = rint(sy); in range iff 0 <= jc <= cols_s - 1 and 0 <= jr <= rows_s - 1
    order 1: in range iff 0 <= sx <= cols_s - 1 and 0 <= sy <= rows_s - 1; c0 = floor(sx), fx = sx - c0, c1 = min(c0 + 1,
             cols_s - 1) (rows likewise); v = (1-fy)*((1-fx)*p00 + fx*p01) + fy*((1-fx)*p10 + fx*p11); uint8: rint(v),
             float32: the cast; keep_zero: 0 when a tap whose two weights are both non-zero holds 0

Every operation is one IEEE double rounding (NumPy neither fuses nor reorders array operations)."""
import numpy as np

from tests import grid_spec as gs

NAN32 = np.array([0x7fc00000], dtype=np.uint32).view(np.float32)[0]


def usable(x, y, xs, ys, valid):
    ok = np.isfinite(x) & np.isfinite(y) & np.isfinite(xs) & np.isfinite(ys)
    return ok if valid is None else ok & (np.asarray(valid) != 0)


def cell_box(xn, yn, rows_o, cols_o):
    """Pixel box of a cell with the usable nodes (xn, yn): r_lo, r_hi, c_lo, c_hi, or None when it is empty."""
    cl, ch = max(np.floor(xn.min()) - 1.0, 0.0), min(np.ceil(xn.max()) + 1.0, float(cols_o - 1))
    rl, rh = max(np.floor(yn.min()) - 1.0, 0.0), min(np.ceil(yn.max()) + 1.0, float(rows_o - 1))
    if not (cl <= ch and rl <= rh):
        return None
    return int(rl), int(rh), int(cl), int(ch)


def owned_by(xf, yf, tri, px, py):
    """Boolean array: the pixels (px, py) that the oriented triangle `tri` (flat node numbers) owns."""
    a, b, c = [int(q) for q in tri]
    inside = np.ones(px.shape, dtype=bool)
    for p, q in ((a, b), (b, c), (c, a)):
        lo, hi = (p, q) if p < q else (q, p)
        E = (xf[hi] - xf[lo]) * (py - yf[lo]) - (yf[hi] - yf[lo]) * (px - xf[lo])
        Ed = E if p == lo else -E
        dx, dy = xf[q] - xf[p], yf[q] - yf[p]
        tie = bool(dy > 0 or (dy == 0 and dx > 0))
        inside &= (Ed > 0) | ((Ed == 0) & tie)
    return inside


def source_of(xf, yf, xsf, ysf, tri, px, py):
    a, b, c = [int(q) for q in tri]
    det = (xf[b] - xf[a]) * (yf[c] - yf[a]) - (xf[c] - xf[a]) * (yf[b] - yf[a])
    l1 = ((px - xf[a]) * (yf[c] - yf[a]) - (xf[c] - xf[a]) * (py - yf[a])) / det
    l2 = ((xf[b] - xf[a]) * (py - yf[a]) - (px - xf[a]) * (yf[b] - yf[a])) / det
    sx = xsf[a] + l1 * (xsf[b] - xsf[a]) + l2 * (xsf[c] - xsf[a])
    sy = ysf[a] + l1 * (ysf[b] - ysf[a]) + l2 * (ysf[c] - ysf[a])
    return sx, sy


def sample(image, src_shape, order, keep_zero, sx, sy):
    """-> in_range (bool), v (float64 value before rounding; the pixel itself for order 0), zero (bool: keep_zero applies)."""
    rows_s, cols_s = src_shape
    v, zero = np.zeros(sx.shape), np.zeros(sx.shape, dtype=bool)
    if order == 0:
        jc, jr = np.rint(sx), np.rint(sy)
        ok = (jc >= 0) & (jc <= cols_s - 1) & (jr >= 0) & (jr <= rows_s - 1)
        if image is not None:
            v[ok] = image[jr[ok].astype(np.int64), jc[ok].astype(np.int64)]
        return ok, v, zero
    ok = (sx >= 0) & (sx <= cols_s - 1) & (sy >= 0) & (sy <= rows_s - 1)
    if image is None:
        return ok, v, zero
    x1, y1 = sx[ok], sy[ok]
    c0, r0 = np.floor(x1), np.floor(y1)
    fx, fy = x1 - c0, y1 - r0
    c0, r0 = c0.astype(np.int64), r0.astype(np.int64)
    c1, r1 = np.minimum(c0 + 1, cols_s - 1), np.minimum(r0 + 1, rows_s - 1)
    p00, p01 = image[r0, c0].astype(np.float64), image[r0, c1].astype(np.float64)
    p10, p11 = image[r1, c0].astype(np.float64), image[r1, c1].astype(np.float64)
    wx, wy = 1.0 - fx, 1.0 - fy
    v[ok] = wy * (wx * p00 + fx * p01) + fy * (wx * p10 + fx * p11)
    if keep_zero:
        zero[ok] = (((wx != 0) & (wy != 0) & (p00 == 0)) | ((fx != 0) & (wy != 0) & (p01 == 0))
                    | ((wx != 0) & (fy != 0) & (p10 == 0)) | ((fx != 0) & (fy != 0) & (p11 == 0)))
    return ok, v, zero


def warp(x, y, xs, ys, valid, diagonal, out_shape, image=None, src_shape=None, order=1, fill=0, keep_zero=False):
    """-> dict: out (image's dtype; None without an image), covered (uint8), map_x, map_y (float32), and for the tests
    owners (int32: how many triangles own each pixel), sx, sy (float64, NaN where unowned), v (float64: the sampled value before
    it is rounded or cast, NaN where not covered), triangles (the t of grid_spec.grid_triangles)."""
    x, y, xs, ys = [np.asarray(q, dtype=np.float64) for q in (x, y, xs, ys)]
    rows_o, cols_o = out_shape
    if image is not None:
        image = np.asarray(image)
        src_shape = image.shape
    ok = usable(x, y, xs, ys, valid)
    t = gs.grid_triangles(x, y, ok, diagonal)
    xf, yf, xsf, ysf, okf = x.ravel(), y.ravel(), xs.ravel(), ys.ravel(), ok.ravel()
    out = np.full(out_shape, fill, dtype=image.dtype) if image is not None else None
    covered = np.zeros(out_shape, dtype=np.uint8)
    map_x, map_y = np.full(out_shape, NAN32, dtype=np.float32), np.full(out_shape, NAN32, dtype=np.float32)
    owners = np.zeros(out_shape, dtype=np.int32)
    sxo, syo, vo = np.full(out_shape, np.nan), np.full(out_shape, np.nan), np.full(out_shape, np.nan)
    rows, cols = x.shape
    with np.errstate(all='ignore'):
        for i in range(rows - 1):
            for j in range(cols - 1):
                A = i * cols + j
                ring = [n for n in (A, A + 1, A + cols + 1, A + cols) if okf[n]]
                if len(ring) < 3:
                    continue
                box = cell_box(xf[ring], yf[ring], rows_o, cols_o)
                if box is None:
                    continue
                r_lo, r_hi, c_lo, c_hi = box
                rr, cc = np.meshgrid(np.arange(r_lo, r_hi + 1), np.arange(c_lo, c_hi + 1), indexing='ij')
                px, py = cc.astype(np.float64), rr.astype(np.float64)
                for s in range(2):
                    tri = t[i, j, s]
                    if tri[0] < 0:
                        continue
                    a, b, c = [int(q) for q in tri]
                    det = (xf[b] - xf[a]) * (yf[c] - yf[a]) - (xf[c] - xf[a]) * (yf[b] - yf[a])
                    if not det > 0:
                        continue
                    own = owned_by(xf, yf, tri, px, py)
                    if not own.any():
                        continue
                    r1, c1 = rr[own], cc[own]
                    sx, sy = source_of(xf, yf, xsf, ysf, tri, px[own], py[own])
                    owners[r1, c1] += 1
                    sxo[r1, c1], syo[r1, c1] = sx, sy
                    map_x[r1, c1] = np.where(np.isnan(sx), NAN32, sx.astype(np.float32))
                    map_y[r1, c1] = np.where(np.isnan(sy), NAN32, sy.astype(np.float32))
                    inr, v, zero = sample(image, src_shape, order, keep_zero, sx, sy)
                    covered[r1[inr], c1[inr]] = 1
                    if image is not None:
                        vo[r1[inr], c1[inr]] = v[inr]
                        if image.dtype == np.uint8:
                            val = np.where(zero, 0.0, np.rint(v)).astype(np.uint8)
                        else:
                            val = v.astype(np.float32)
                        out[r1[inr], c1[inr]] = val[inr]
    return dict(out=out, covered=covered, map_x=map_x, map_y=map_y, owners=owners, sx=sxo, sy=syo, v=vo, triangles=t)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()
