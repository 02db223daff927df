"""The specification of the gap filling, the smoothing and the chain of include/sid_grid.h in NumPy -
the only restatement the tests use.  No tests in here.  Usable node and median: tests/grid_spec.py.

    fill_gaps: generation 0 = the usable nodes; their u_f, v_f are the inputs bit for bit.  Pass p = 1..max_passes: the
         candidates are the nodes without a generation that have (domain is None or domain != 0); N = the nodes of the
         candidate's (2 radius + 1)^2 window, centre excluded, clipped at the edges, with a generation in 0..p-1 and finite
         u_f, v_f.  |N| >= min_neighbours: u_f = median(u_N) + 0.0, v_f = median(v_N) + 0.0, gen = p.  A pass reads only
         generations below its own: what it fills is written after all of it was computed.  Never filled: NaN, NaN, -1.  A pass
         that fills nothing ends the process.
    smooth: for a usable node sw = su = sv = 0.0; for di = -r..r, for dj = -r..r, for a usable node (i + di, j + dj) inside the
         grid (the centre included): sw = sw + w ; su = su + w * u ; sv = sv + w * v.  u_s = su / sw, v_s = sv / sw.  Unusable
         nodes: NaN in both.  The default table is gaussian_weights.
    clean_drift: S_0 = the usable nodes; S_k = S_{k-1} & ~(res_k > threshold) with res_k of the normalised median test on
         valid = S_{k-1}; fill_gaps(valid = S); smooth(valid = gen >= 0) when sigma is not None.

Every operation is one IEEE double rounding (np.float64 scalars: NumPy neither fuses nor reorders them)."""
import numpy as np

from tests import grid_spec as gs


def fill_gaps(u, v, valid=None, domain=None, radius=1, min_neighbours=3, max_passes=16):
    """-> u_f, v_f (float64), gen (int32), all of u's shape."""
    u, v = np.asarray(u, dtype=np.float64), np.asarray(v, dtype=np.float64)
    rows, cols = u.shape
    ok = gs.usable_uv(u, v, valid)
    uf, vf = np.where(ok, u, np.nan), np.where(ok, v, np.nan)
    gen = np.where(ok, 0, -1).astype(np.int32)
    dom = np.ones((rows, cols), dtype=bool) if domain is None else np.asarray(domain) != 0
    zero = np.float64(0.0)
    with np.errstate(all='ignore'):
        for p in range(1, max_passes + 1):
            new = []
            for i in range(rows):
                for j in range(cols):
                    if gen[i, j] >= 0 or not dom[i, j]:
                        continue
                    un, vn = [], []
                    for ii in range(max(i - radius, 0), min(i + radius, rows - 1) + 1):
                        for jj in range(max(j - radius, 0), min(j + radius, cols - 1) + 1):
                            if (ii, jj) != (i, j) and 0 <= gen[ii, jj] < p and np.isfinite(uf[ii, jj]) and np.isfinite(vf[ii, jj]):
                                un.append(uf[ii, jj])
                                vn.append(vf[ii, jj])
                    if len(un) >= min_neighbours:
                        new.append((i, j, gs.median(un) + zero, gs.median(vn) + zero))
            if not new:
                break
            for i, j, a, b in new:                      # Jacobi order: written after the whole pass was computed
                uf[i, j], vf[i, j], gen[i, j] = a, b, p
    return uf, vf, gen


def gaussian_weights(sigma, radius):
    di, dj = np.meshgrid(np.arange(-radius, radius + 1, dtype=np.float64), np.arange(-radius, radius + 1, dtype=np.float64),
                         indexing='ij')
    return np.exp(-(di * di + dj * dj) / (2.0 * sigma * sigma))


def smooth(u, v, sigma=1.0, radius=1, valid=None, weights=None):
    """-> u_s, v_s (float64) of u's shape."""
    u, v = np.asarray(u, dtype=np.float64), np.asarray(v, dtype=np.float64)
    w = gaussian_weights(sigma, radius) if weights is None else np.asarray(weights, dtype=np.float64)
    assert w.shape == (2 * radius + 1, 2 * radius + 1)
    rows, cols = u.shape
    ok = gs.usable_uv(u, v, valid)
    us, vs = np.full((rows, cols), np.nan), np.full((rows, cols), np.nan)
    with np.errstate(all='ignore'):
        for i in range(rows):
            for j in range(cols):
                if not ok[i, j]:
                    continue
                sw = su = sv = np.float64(0.0)
                for di in range(-radius, radius + 1):
                    for dj in range(-radius, radius + 1):
                        ii, jj = i + di, j + dj
                        if 0 <= ii < rows and 0 <= jj < cols and ok[ii, jj]:
                            ww = w[di + radius, dj + radius]
                            sw = sw + ww
                            su = su + ww * u[ii, jj]
                            sv = sv + ww * v[ii, jj]
                us[i, j], vs[i, j] = su / sw, sv / sw
    return us, vs


def clean_drift(u, v, eps, valid=None, domain=None, threshold=2.0, radius=1, min_neighbours=3, detect_passes=2, max_passes=16,
                sigma=None):
    """-> u_c, v_c (float64), keep (bool), gen (int32), and the list of S_0 .. S_detect_passes."""
    u, v = np.asarray(u, dtype=np.float64), np.asarray(v, dtype=np.float64)
    s = gs.usable_uv(u, v, valid)
    sets = [s]
    for _ in range(detect_passes):
        _, res = gs.nmt(u, v, s, eps, threshold, radius, min_neighbours)
        with np.errstate(invalid='ignore'):
            s = s & ~(res > threshold)
        sets.append(s)
    uc, vc, gen = fill_gaps(u, v, s, domain, radius, min_neighbours, max_passes)
    if sigma is not None:
        uc, vc = smooth(uc, vc, sigma, radius, gen >= 0)
    return uc, vc, s, gen, sets
