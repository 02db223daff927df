"""The specification of include/sid_corr.h in NumPy - the only restatement the tests use.  No tests in here.

A node centred at the integers (rc, cc) has the window rows rc - w//2 .. rc - w//2 + w - 1 and the columns likewise, clipped to
the image (it may be empty).  A pixel is usable iff a != 0 and b != 0.  Over the usable pixels, in integers:

    n, Sa, Sb, Saa, Sbb, Sab ;  va = n*Saa - Sa*Sa ; vb = n*Sbb - Sb*Sb ; cab = n*Sab - Sa*Sb
    r = NaN if n < min_count or va <= 0 or vb <= 0 else clamp(float64(cab) / sqrt(float64(va) * float64(vb)), -1, 1)

The sums are differences of int64 summed-area tables (exact: the table of a 10000 x 10000 image of 255s stays below 2^43), the
float64 operations NumPy array operations in the order written (NumPy neither fuses nor reorders them).  A lattice centre is
origin + i*step in Python integers, beyond +-2^40 taken as +-2^40 (the window is empty either way)."""
import numpy as np

FAR = 1 << 40


def same_bits(a, b):
    """Equal shape, dtype and bytes (a NaN equals a NaN of the same bits only)."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def centres(origin, step, count):
    return [min(max(int(origin) + i * int(step), -FAR), FAR) for i in range(int(count))]


def clipped(cs, w, size):
    """lo, hi (int64 arrays) of the windows of side w around the centres `cs`, clipped to [0, size) as slicing clips."""
    lo = np.array([min(max(c - w // 2, 0), size) for c in cs], dtype=np.int64).reshape(len(cs))
    hi = np.array([min(max(c - w // 2 + w, 0), size) for c in cs], dtype=np.int64).reshape(len(cs))
    return lo, np.maximum(hi, lo)


def tables(a, b):
    """Summed-area tables (int64, one row and column of zeros in front) of: usable, a, b, a*a, b*b, a*b over the usable pixels."""
    a, b = np.asarray(a), np.asarray(b)
    assert a.dtype == np.uint8 and b.dtype == np.uint8 and a.shape == b.shape and a.ndim == 2
    ok = (a != 0) & (b != 0)
    a64, b64 = np.where(ok, a, 0).astype(np.int64), np.where(ok, b, 0).astype(np.int64)
    out = []
    for x in (ok.astype(np.int64), a64, b64, a64 * a64, b64 * b64, a64 * b64):
        t = np.zeros((a.shape[0] + 1, a.shape[1] + 1), dtype=np.int64)
        t[1:, 1:] = x.cumsum(0).cumsum(1)
        out.append(t)
    return out


def finalise(n, sa, sb, saa, sbb, sab, min_count):
    """int64 arrays of one shape -> r float64."""
    va, vb, cab = n * saa - sa * sa, n * sbb - sb * sb, n * sab - sa * sb
    ok = (n >= min_count) & (va > 0) & (vb > 0)
    r = np.full(n.shape, np.nan, dtype=np.float64)
    prod = va[ok].astype(np.float64) * vb[ok].astype(np.float64)
    q = cab[ok].astype(np.float64) / np.sqrt(prod)
    r[ok] = np.where(q > 1.0, 1.0, np.where(q < -1.0, -1.0, q))
    return r


def _result(six, min_count):
    n, sa, sb, saa, sbb, sab = six
    return dict(r=finalise(n, sa, sb, saa, sbb, sab, int(min_count)), count=n.astype(np.int32),
                sums=np.ascontiguousarray(np.stack([sa, sb, saa, sbb, sab], axis=-1)), va=n * saa - sa * sa, vb=n * sbb - sb * sb)


def lattice(a, b, w, origin, step, shape, min_count):
    """-> dict(r [nr, nc] float64, count int32, sums [nr, nc, 5] int64; va, vb int64 for the tests' own checks)."""
    rows, cols = np.asarray(a).shape
    r_lo, r_hi = clipped(centres(origin[0], step[0], shape[0]), w, rows)
    c_lo, c_hi = clipped(centres(origin[1], step[1], shape[1]), w, cols)
    six = [t[np.ix_(r_hi, c_hi)] - t[np.ix_(r_lo, c_hi)] - t[np.ix_(r_hi, c_lo)] + t[np.ix_(r_lo, c_lo)] for t in tables(a, b)]
    return _result(six, min_count)


def points(a, b, w, c, r, valid, min_count):
    """c, r integer arrays of one shape, valid of that shape or None -> the same dict, with the shape of c."""
    rows, cols = np.asarray(a).shape
    c, r = np.asarray(c), np.asarray(r)
    ok = np.ones(c.shape, dtype=bool) if valid is None else np.asarray(valid) != 0
    cs = [int(q) if k else 0 for q, k in zip(c.ravel(), ok.ravel())]                # (a centre behind valid == 0 is not read)
    rs = [int(q) if k else 0 for q, k in zip(r.ravel(), ok.ravel())]
    r_lo, r_hi = clipped(rs, w, rows)
    c_lo, c_hi = clipped(cs, w, cols)
    six = [np.where(ok.ravel(), t[r_hi, c_hi] - t[r_lo, c_hi] - t[r_hi, c_lo] + t[r_lo, c_lo], 0).reshape(c.shape) for t in tables(a, b)]
    return _result(six, min_count)


def window_pixels(a, b, w, rc, cc):
    """The usable pixels of one window, by slicing: two 1-D uint8 arrays (what np.corrcoef is given in the tests)."""
    a, b = np.asarray(a), np.asarray(b)
    r_lo, r_hi = clipped([int(rc)], w, a.shape[0])
    c_lo, c_hi = clipped([int(cc)], w, a.shape[1])
    wa, wb = a[r_lo[0]:r_hi[0], c_lo[0]:c_hi[0]], b[r_lo[0]:r_hi[0], c_lo[0]:c_hi[0]]
    ok = (wa != 0) & (wb != 0)
    return wa[ok], wb[ok]
