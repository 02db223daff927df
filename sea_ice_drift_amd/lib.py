"""Host-side helpers the PM path needs from the reference's lib.py.

What ``pattern_matching`` touches: the two first-guess interpolators (reference lib.py:139-177 and
:179-201), the grid scatter (lib.py:408-412) and a stand-in for ``nansat.NSR``; plus the uint8 staging step
``get_uint8_image`` (lib.py:27-59), whose two full-image passes run on the GPU (include/sid_stage.h), and the array steps of ``get_n`` in
front of it (lib.py:318-331: dB, ``hh_angular_correction``, mask, ``get_spatial_mean``; include/sid_prep.h): ``prepare_image``,
and the resize at its head (lib.py:314-316, ``n.resize(factor, resample_alg=-1)``; include/sid_resize.h): ``resize_image``.
Reading files (lib.py:309-316, 333-340) and the geo/Haversine helpers are outside the hot path.
"""
import numpy as np
from scipy.interpolate import griddata

try:                                      # a real nansat passes through untouched
    from nansat import NSR                # pragma: no cover - not installed in this image
except Exception:                         # noqa: BLE001
    class NSR(object):
        """Placeholder for nansat.NSR: carries the srs string to duck-typed domains."""
        def __init__(self, srs=None):
            self.srs = srs
            self.wkt = srs

        def __repr__(self):
            return 'NSR(%r)' % (self.srs,)


EARTH_RADIUS_KM = 6371  # mean radius the reference's Haversine uses (lib.py:25)
AVG_EARTH_RADIUS = EARTH_RADIUS_KM  # the reference's name for it


def _haversine_km(lon_a, lat_a, lon_b, lat_b):
    """Great-circle distance in km between (lon, lat) pairs given in degrees."""
    phi_a, phi_b = np.radians(lat_a), np.radians(lat_b)
    half_dphi = (phi_b - phi_a) * 0.5
    half_dlam = (np.radians(lon_b) - np.radians(lon_a)) * 0.5
    hav = np.sin(half_dphi) ** 2 + np.cos(phi_a) * np.cos(phi_b) * np.sin(half_dlam) ** 2
    return 2 * EARTH_RADIUS_KM * np.arcsin(np.sqrt(hav))


def great_circle_km(n1, x1, y1, n2, x2, y2):
    """Distance in km between pixel (x1, y1) of image n1 and pixel (x2, y2) of image n2 (what the
    reference's get_displacement_km returns, lib.py:61-85)."""
    return _haversine_km(*(n1.transform_points(x1, y1) + n2.transform_points(x2, y2)))


def get_displacement_km(n1, x1, y1, n2, x2, y2):
    """Reference name (lib.py:61) of ``great_circle_km``."""
    return great_circle_km(n1, x1, y1, n2, x2, y2)


def get_displacement_pix(n1, x1, y1, n2, x2, y2):
    """Displacement in pixels of the first image (reference lib.py:103-121): the key points of image 2 are carried
    through lon/lat into the pixel space of image 1; returns (dx, dy) = their offsets from (x1, y1)."""
    on_n1 = n1.transform_points(*n2.transform_points(x2, y2), 1)
    return on_n1[0] - x1, on_n1[1] - y1


def get_speed_ms(n1, x1, y1, n2, x2, y2):
    """Drift speed in m/s between two time-stamped images (reference lib.py:87-102)."""
    elapsed = abs((n2.time_coverage_start - n1.time_coverage_start).total_seconds())
    return 1000. * great_circle_km(n1, x1, y1, n2, x2, y2) / elapsed


def _is_projected(nsr):
    """True when ``nsr`` names a projected spatial reference.  Understood: an ``osr.SpatialReference`` (what nansat's NSR
    is: ``IsGeographic()``), the local placeholder (``.srs``), anything else that carries its definition as ``.wkt`` -
    a definition that reads as geographic ('+proj=longlat', 'GEOGCS[', 'GEOGCRS[') is not projected."""
    if nsr is None:
        return False
    is_geographic = getattr(nsr, 'IsGeographic', None)
    if callable(is_geographic):
        try:
            return not bool(is_geographic())
        except Exception:                        # noqa: BLE001
            pass
    text = getattr(nsr, 'srs', None)
    if text in (None, ''):
        text = getattr(nsr, 'wkt', None)
    if text in (None, ''):
        return False
    text = str(text).lstrip()
    return not ('+proj=longlat' in text or '+proj=latlong' in text or text.upper().startswith(('GEOGCS', 'GEOGCRS')))


def _nansat_domain():
    """nansat's ``Domain`` class when nansat is installed, else None."""
    try:
        from nansat import Domain                # pragma: no cover - not installed in this image
    except Exception:                            # noqa: BLE001
        return None
    return Domain                                # pragma: no cover


def get_drift_vectors(n1, x1, y1, n2, x2, y2, nsr=None, **kwargs):
    """u, v, lon1, lat1, lon2, lat2 of matched points (reference lib.py:375-406).

    The reference projects lon/lat through ``nansat.Domain(nsr, '-te -10 -10 10 10 -tr 1 1')`` - a grid with origin
    (-10, 10) and unit pixels in the units of ``nsr`` - and returns pixel differences: with (X, Y) the coordinates of
    a point in ``nsr``, its pixel is (X + 10, 10 - Y), so u = (X2 + 10) - (X1 + 10) and v = (10 - Y1) - (10 - Y2).
    That arithmetic is restated here.  Where (X, Y) come from:

    * nansat installed: the reference's own Domain call, for every ``nsr``;
    * no nansat, default or geographic ``nsr`` (lon/lat WGS84): X = lon, Y = lat;
    * no nansat, projected ``nsr`` (``_is_projected``: an ``osr.SpatialReference`` that is not geographic, the local
      placeholder's ``.srs``, or a ``.wkt`` that does not read as geographic): the images' own ``transform_points(x, y, 0, nsr)`` (pixel -> coordinates
      in the destination SRS, the call pm_postlude makes for ``srs=``, pmlib.py:473-478; Appendix A of SURVEY.md) -
      any Nansat-like object that implements it serves; one that does not raises NotImplementedError."""
    lon1, lat1 = n1.transform_points(x1, y1)
    lon2, lat2 = n2.transform_points(x2, y2)
    Domain = _nansat_domain()
    if nsr is not None and Domain is not None:
        # nansat is installed: the reference's own call for every nsr, geographic or projected (lib.py:394-399)
        d = Domain(nsr, '-te -10 -10 10 10 -tr 1 1')
        px1, py1 = d.transform_points(lon1, lat1, 1)
        px2, py2 = d.transform_points(lon2, lat2, 1)
        return px2 - px1, py1 - py2, lon1, lat1, lon2, lat2
    if _is_projected(nsr):
        try:
            X1, Y1 = n1.transform_points(x1, y1, 0, nsr)
            X2, Y2 = n2.transform_points(x2, y2, 0, nsr)
        except TypeError:
            raise NotImplementedError('a projected nsr needs nansat, or image objects whose transform_points accepts a '
                                      'destination SRS (transform_points(x, y, 0, nsr))')
    else:
        X1, Y1, X2, Y2 = lon1, lat1, lon2, lat2
    px1, py1 = X1 - (-10.0), 10.0 - Y1                                        # Domain('-te -10 -10 10 10 -tr 1 1')
    px2, py2 = X2 - (-10.0), 10.0 - Y2
    return px2 - px1, py1 - py2, lon1, lat1, lon2, lat2


def _poly_terms(x, y, order):
    """Columns of the design matrix in the reference's term order (lib.py:160-168):
    1, x, y | x^2, y^2, xy | x^3, y^3, x^2 y, y^2 x."""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    terms = [np.ones(len(x)), x, y]
    if order > 1:
        terms.extend((x ** 2, y ** 2, x * y))
    if order > 2:
        terms.extend((x ** 3, y ** 3, x ** 2 * y, y ** 2 * x))
    return np.vstack(terms).T


def fit_polynomial_map(x1, y1, x2, y2, order=1):
    """Least-squares polynomial map (x1, y1) -> (x2, y2); returns ``f(x, y) -> (x', y')`` for flat arrays.
    The solve is NumPy's ``lstsq`` with ``rcond=-1`` on the design matrix above, one right-hand side at a
    time, and the evaluation is a matrix-vector product - the arithmetic of lib.py:139-177."""
    design = _poly_terms(x1, y1, order)
    coef_x = np.linalg.lstsq(design, x2, rcond=-1)[0]
    coef_y = np.linalg.lstsq(design, y2, rcond=-1)[0]

    def evaluate(x, y):
        g = _poly_terms(x, y, order)
        return np.dot(g, coef_x), np.dot(g, coef_y)
    evaluate.coefficients = (coef_x, coef_y)
    return evaluate


def interpolation_poly(x1, y1, x2, y2, x1grd, y1grd, order=1, **kwargs):
    """Reference name and signature (lib.py:139-177): the polynomial map evaluated on the grid points,
    shaped like ``x1grd``."""
    fx, fy = fit_polynomial_map(x1, y1, x2, y2, order)(np.ravel(x1grd), np.ravel(y1grd))
    return fx.reshape(np.shape(x1grd)), fy.reshape(np.shape(x1grd))


# Triangulations started ahead of their use (``prefetch_triangulation``): key = digest of the point array, value = a
# one-element future.  SeaIceDrift.get_drift_FT starts the triangulation of its matched key points on a worker thread the
# moment the filters return - the Delaunay triangulation (Qhull, 30-85 ms for 2-3 x 10^4 points) is the longest step of the
# pattern-matching prelude, and whatever the caller does between the two calls now runs beside it.
_TRI_CACHE = {}
_TRI_LOCK = None


def _tri_key(src):
    import hashlib
    a = np.ascontiguousarray(src, dtype=np.float64)
    return hashlib.blake2b(a.tobytes(), digest_size=16).digest() + str(a.shape).encode()


def prefetch_triangulation(src):
    """Start ``scipy.spatial.Delaunay(src)`` on a worker thread; ``_triangulation(src)`` with the SAME points (bit for bit)
    picks the result up.  At most two are kept."""
    import threading
    global _TRI_LOCK
    if _TRI_LOCK is None:
        _TRI_LOCK = threading.Lock()
    src = np.array(src, dtype=np.float64)
    if src.ndim != 2 or src.shape[0] < 4 or src.shape[1] != 2:
        return None
    key = _tri_key(src)
    box = {}

    def work():
        from scipy.spatial import Delaunay
        try:
            box['tri'] = Delaunay(src)
        except Exception as e:                   # noqa: BLE001 - the consumer triangulates itself and raises what it raises
            box['err'] = e
    t = threading.Thread(target=work, name='sid-delaunay', daemon=True)
    with _TRI_LOCK:
        while len(_TRI_CACHE) >= 2:
            _TRI_CACHE.pop(next(iter(_TRI_CACHE)))
        _TRI_CACHE[key] = (t, box)
    t.start()
    return key


def _triangulation(src):
    """``scipy.spatial.Delaunay(src)`` - the one started by ``prefetch_triangulation`` for these very points, if any."""
    from scipy.spatial import Delaunay
    if _TRI_CACHE:
        key = _tri_key(src)
        with _TRI_LOCK:
            hit = _TRI_CACHE.pop(key, None)
        if hit is not None:
            t, box = hit
            t.join()
            tri = box.get('tri')
            if tri is not None and tri.points.shape == np.shape(src) and np.array_equal(tri.points, src):
                return tri
    return Delaunay(src)


def interpolation_near(x1, y1, x2, y2, x1grd, y1grd, method='linear', first_guess_device=None, knn_k=5, knn_max_dist=None,
                       knn_displacement=True, **kwargs):
    """scipy griddata of x2/y2 from the keypoints onto the grid points; NaN outside the
    convex hull (reference lib.py:179-201; note the (row, col) point order).

    ``first_guess_device`` (not a reference argument): GPU index on which the grid points are located in the
    triangulation and interpolated (include/sid_fg.h) - the triangulation is SciPy's Delaunay either way.  ``None``
    evaluates with SciPy on the host.

    ``method='knn'`` with ``knn_k`` (1..16, default 5) and ``knn_max_dist`` (pixels; None: no limit) - none of them the
    reference's: the component-wise median of x2 / y2 over the ``knn_k`` nearest key points (include/sid_fg.h sid_fg_knn,
    DESIGN.md section 20).  No triangulation and no SciPy call: the search runs on ``first_guess_device``, or in the
    library's host instance when that is None - the same numbers bit for bit.  Defined everywhere (no convex hull); NaN
    only where ``knn_max_dist`` leaves a grid point without a key point.  A median ignores up to (knn_k - 1) / 2 wrong
    key points around a grid point, which a linear interpolant passes on into every triangle they touch.  Key-point
    values that are not finite raise ValueError.  ``knn_displacement=True`` (default): x2, y2 are positions, as in the
    first guess - the median is taken over the key points' displacements x2 - x1, y2 - y1 and added to the grid point
    (the median of the neighbours' positions would be the position of one neighbour, tens of pixels from the grid
    point: a linear interpolant reproduces a shift either way, a median only this way).  False: x2, y2 are the values
    of a field and their median is the result (the residuals of ``old_border=False``)."""
    if method == 'knn':
        from . import _capi
        vals = np.array([x2, y2], dtype=np.float64).T
        if not np.isfinite(vals).all():
            raise ValueError("method='knn': key-point values (x2, y2) must be finite")
        src = np.array([y1, x1], dtype=np.float64).T
        grd_shape = np.shape(x1grd)
        flat = np.array([np.ravel(y1grd), np.ravel(x1grd)], dtype=np.float64).T
        if knn_displacement:
            vals = vals - src[:, ::-1]
        both = _capi.fg_knn(src, vals, flat, k=knn_k, max_dist=knn_max_dist,
                            device=-1 if first_guess_device is None else first_guess_device)
        if knn_displacement:
            both = flat[:, ::-1] + both
        return both[:, 0].reshape(grd_shape), both[:, 1].reshape(grd_shape)
    src = np.array([y1, x1]).T
    dst = np.array([y1grd, x1grd]).T
    if method == 'linear' and src.shape[1] == 2:
        # The reference calls griddata twice, i.e. triangulates the same keypoints twice - the slowest
        # step of the whole prelude.  One Delaunay triangulation serves both components; every component
        # is the same barycentric sum, so the values are bit-identical to the two separate calls.
        tri = _triangulation(src)
        vals = np.array([x2, y2], dtype=np.float64).T
        if first_guess_device is not None and _has_degenerate_simplex(tri):
            # SciPy gives a (nearly) flat simplex a NaN barycentric transform and then accepts queries in its neighbours
            # with a much wider tolerance (sqrt(eps)) towards it; the device's flags do not model that,
            # so such a triangulation - collinear or duplicated key points - is evaluated by SciPy alone
            first_guess_device = None
        if first_guess_device is not None:
            # Point location and barycentric evaluation on the GPU.  Queries whose result could depend on SciPy's own choice
            # of simplex (on an edge, a vertex or the hull) or on the last bit of its arithmetic (value next to a
            # half-integer, which the caller rounds) come back flagged and are evaluated by SciPy itself, so that the
            # ROUNDED first guess is the reference's in every case (include/sid_fg.h).
            from . import _capi
            flat = dst.reshape(-1, 2)
            both, _, doubt = _capi.fg_interp_linear(tri.points, tri.simplices, vals, flat, device=first_guess_device, details=True)
            # (SciPy rejects a query outside the bounding box of the points before it looks at any simplex: queries on the
            # box, where that absolute test and the barycentric one could part, go to SciPy as well)
            lo, hi = tri.points.min(axis=0), tri.points.max(axis=0)
            doubt |= (np.abs(flat - lo) < 1e-9).any(axis=1) | (np.abs(flat - hi) < 1e-9).any(axis=1)
            if doubt.any():
                from scipy.interpolate import LinearNDInterpolator
                both[doubt] = LinearNDInterpolator(tri, vals)(flat[doubt])
            both = both.reshape(dst.shape[:-1] + (2,))
        else:
            from scipy.interpolate import LinearNDInterpolator
            both = LinearNDInterpolator(tri, vals)(dst)
        return both[..., 0].T, both[..., 1].T
    return griddata(src, x2, dst, method=method).T, griddata(src, y2, dst, method=method).T


def _has_degenerate_simplex(tri, rcond_limit=1e-10):
    """True when some simplex of the 2-D triangulation is so flat that SciPy may treat it as degenerate: SciPy's test is
    LAPACK's reciprocal condition estimate of the 2 x 2 edge matrix below 1000 eps (qhull.pyx, _get_barycentric_transforms);
    here the exact 1-norm condition number with a limit three orders of magnitude more careful."""
    p = tri.points[tri.simplices]                                     # [ns, 3, 2]
    a, b = p[:, 0] - p[:, 2], p[:, 1] - p[:, 2]                       # columns of the matrix SciPy factorises
    det = a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]
    n1 = np.maximum(np.abs(a).sum(axis=1), np.abs(b).sum(axis=1))     # ||M||_1; the adjugate has the same column sums, permuted
    nadj = np.maximum(np.abs(b[:, 1]) + np.abs(a[:, 1]), np.abs(b[:, 0]) + np.abs(a[:, 0]))
    with np.errstate(divide='ignore', invalid='ignore'):
        rcond = np.abs(det) / (n1 * nadj)
    return bool((~np.isfinite(rcond) | (rcond < rcond_limit)).any())


def _fill_gpi(shape, gpi, data):
    """Grid of ``shape`` holding ``data`` at the flat positions where ``gpi`` is set and NaN elsewhere
    (reference lib.py:408-412)."""
    grid = np.full(int(np.prod(shape)), np.nan)
    grid[np.asarray(gpi, dtype=bool).ravel()] = data
    return grid.reshape(shape)


def _percentile_ranks(n, p, ftype):
    """Neighbour ranks and weight of np.nanpercentile's 'linear' interpolation for a float32 image:
    q = p / float32(100), virtual index (n - 1) * q in float32 (numpy/lib/_function_base_impl.py)."""
    q = np.true_divide(p, ftype(100))
    vi = (n - 1) * q
    prev = np.floor(vi)
    lo = min(max(int(prev), 0), n - 1)
    return lo, min(lo + 1, n - 1), vi - prev


def _lerp(a, b, t):
    with np.errstate(all='ignore'):
        d = np.subtract(b, a)
        r = np.add(a, d * t)
        if t >= 0.5:
            r = np.subtract(b, d * (1 - t))
    return r


_STAGE_WS = {}                     # one staging workspace per device, created on first use


def get_uint8_image(image, vmin, vmax, pmin, pmax, device=0):
    """Scale a float32 image to uint8 on the GPU: signature and results of the reference's
    ``get_uint8_image`` (lib.py:27-59): ``1 + 254 * (image - vmin) / (vmax - vmin)`` clipped to [1, 255],
    0 for pixels that are not finite; ``vmin`` / ``vmax`` default to ``np.nanpercentile(image, pmin / pmax)``.

    ``image``: 2-D float32 NumPy array (uploaded) or a CUDA/HIP torch tensor (used in place); the result is of
    the same kind.  The device selects the order statistics and maps the pixels (include/sid_stage.h); the
    three-operation float32 interpolation between the two neighbouring order statistics is NumPy's own
    arithmetic, so the percentiles - and the image - equal the reference's bit for bit.  No CPU fallback."""
    import torch
    from . import _capi
    is_tensor = isinstance(image, torch.Tensor)
    if is_tensor:
        t = image
        if not t.is_cuda:
            raise ValueError('a torch input must live on the GPU (pass NumPy arrays for host data)')
    else:
        a = np.asarray(image)
        if a.dtype != np.float32:
            raise NotImplementedError('get_uint8_image on the device takes float32 images (got %s)' % a.dtype)
        t = torch.from_numpy(np.ascontiguousarray(a)).to(torch.device('cuda', device))
    if t.dtype != torch.float32 or t.dim() != 2 or t.stride(1) != 1:
        raise NotImplementedError('2-D float32 image with unit inner stride expected')
    rows, cols, stride = int(t.shape[0]), int(t.shape[1]), int(t.stride(0))
    stream = torch.cuda.current_stream(t.device).cuda_stream
    ftype = np.float32
    if vmin is None or vmax is None:
        dev_index = t.device.index or 0
        ws = _STAGE_WS.get(dev_index)
        if ws is None:
            ws = _STAGE_WS[dev_index] = _capi.StageWorkspace(dev_index)
        want = [p for p, v in ((pmin, vmin), (pmax, vmax)) if v is None]
        # (the percentiles as fractions: the first pass then already counts inside sampled key ranges around them)
        n = ws.begin(t.data_ptr(), rows, cols, stride, stream, fractions=[float(p) / 100.0 for p in want])
        if n == 0:
            vals = {p: ftype(np.nan) for p in want}
        else:
            rk = {p: _percentile_ranks(n, p, ftype) for p in want}
            ranks = sorted({r for p in want for r in rk[p][:2]})
            stat = dict(zip(ranks, ws.order_stats(ranks)))
            vals = {p: _lerp(stat[rk[p][0]], stat[rk[p][1]], rk[p][2]) for p in want}
        if vmin is None:
            vmin = vals[pmin]
            print('VMIN: ', vmin)
        if vmax is None:
            vmax = vals[pmax]
            print('VMAX: ', vmax)
    with np.errstate(all='ignore'):
        denom = ftype(vmax - vmin)                    # NumPy scalar rules: float32 when either is a percentile
        vmin32 = ftype(vmin)
    out = torch.empty((rows, cols), dtype=torch.uint8, device=t.device)
    _capi.stage_scale_u8(t.data_ptr(), rows, cols, stride, vmin32, denom, out.data_ptr(), int(out.stride(0)), stream)
    return out if is_tensor else out.cpu().numpy()


# ---------------------------------------------------------------------------------------------------------------------
# downsampling by area average: the first line of get_n, n.resize(factor, resample_alg=-1) (reference lib.py:314-316), on the
# GPU (include/sid_resize.h)
# ---------------------------------------------------------------------------------------------------------------------
RESIZE_MAX_DIM = 1 << 24           # SID_RESIZE_MAX_DIM


def resize_shape(rows, cols, factor=0.5, out_shape=None):
    """The shape ``resize_image`` gives a ``rows`` x ``cols`` image: ``out_shape`` when given, else ``(int(rows * factor),
    int(cols * factor))`` in Python float arithmetic (what nansat's ``resize(factor)`` is understood to do).  ValueError for a
    factor that is not finite, not positive or above 1, for a dimension of 0 and for an ``out_shape`` beyond the image."""
    import math
    if out_shape is not None:
        try:
            r, c = (int(v) for v in out_shape)
        except (TypeError, ValueError):
            raise ValueError('out_shape: (rows, cols) expected, got %r' % (out_shape,))
    else:
        factor = float(factor)
        if not math.isfinite(factor) or factor <= 0.0:
            raise ValueError('factor: a finite positive number expected (got %r)' % (factor,))
        if factor > 1.0:
            raise ValueError('factor %r is above 1: downsampling only' % (factor,))
        r, c = int(rows * factor), int(cols * factor)
    if r < 1 or c < 1:
        raise ValueError('a %d x %d image resized to %d x %d: an output dimension of 0' % (rows, cols, r, c))
    if r > rows or c > cols:
        raise ValueError('a %d x %d image resized to %d x %d: downsampling only' % (rows, cols, r, c))
    if rows > RESIZE_MAX_DIM or cols > RESIZE_MAX_DIM:
        raise ValueError('a %d x %d image: dimensions up to 2^24 are supported' % (rows, cols))
    return r, c


def _resize_kind(image):
    """(is_tensor, dtype name, rows, cols) of a 2-D float32 or uint8 image: NumPy array or ROCm tensor with unit inner stride."""
    import torch
    is_tensor = isinstance(image, torch.Tensor)
    if not is_tensor:
        image = np.asarray(image)
    name = str(image.dtype).replace('torch.', '')
    if name not in ('float32', 'uint8'):
        raise NotImplementedError('resize_image takes float32 and uint8 images (got %s)' % name)
    if len(image.shape) != 2:
        raise ValueError('image: 2-D array expected (got %d-D)' % len(image.shape))
    if is_tensor:
        if not image.is_cuda:
            raise ValueError('a torch input must live on the GPU (pass NumPy arrays for host data)')
        if image.stride(1) != 1 and image.shape[1] > 1:
            raise NotImplementedError('image: unit inner stride expected (row stride is free)')
    return is_tensor, name, int(image.shape[0]), int(image.shape[1])


def _resize_device(t, name, out_rows, out_cols, option):
    """``sid_resize_f32`` / ``sid_resize_u8`` of a device tensor on the current stream -> a new device tensor."""
    import torch
    from . import _capi
    out = torch.empty((out_rows, out_cols), dtype=t.dtype, device=t.device)
    _capi.resize(t.data_ptr(), name, int(t.shape[0]), int(t.shape[1]), int(t.stride(0)), out.data_ptr(), out_rows, out_cols,
                 int(out.stride(0)), option, torch.cuda.current_stream(t.device).cuda_stream)
    return out


def resize_image(image, factor=0.5, out_shape=None, nan_policy='propagate', zero_invalid=True, device=0):
    """Downsample a 2-D image by area average on the GPU: what ``n.resize(factor, resample_alg=-1)`` does to the band at the
    head of the reference's ``get_n`` (lib.py:314-316), for a caller who holds the band as an array.  The result has
    ``resize_shape(rows, cols, factor, out_shape)``; where rows and columns divide evenly (``factor=0.5`` on even sizes) every
    output pixel is the mean of its k x k block, otherwise the exact area-weighted mean (include/sid_resize.h has the
    weights and every rounding).  The same shape (``factor=1``) returns a copy with identical bits.

    float32: float64 accumulation in row-major order, rounded once to float32; NaN and +-inf propagate, or
    ``nan_policy='omit'`` leaves NaN pixels out of the sum and the divisor (a window of NaN alone gives NaN).  uint8: the mean
    rounded half up in integer arithmetic; with ``zero_invalid`` (default: 0 means invalid throughout this package) an output
    pixel is 0 exactly when one of its source pixels is.  An option of the other dtype given a non-default value raises
    ValueError; other dtypes raise NotImplementedError.

    A NumPy array is uploaded and a NumPy array comes back; a ROCm torch tensor (unit inner stride, any row stride) is read in
    place on the current stream and a device tensor comes back.  The input is never modified.  No CPU fallback."""
    import torch
    is_tensor, name, rows, cols = _resize_kind(image)
    if nan_policy not in ('propagate', 'omit'):
        raise ValueError("nan_policy: 'propagate' or 'omit' expected (got %r)" % (nan_policy,))
    if name == 'uint8' and nan_policy != 'propagate':
        raise ValueError('nan_policy applies to float32 images (the image is uint8)')
    if name == 'float32' and not zero_invalid:
        raise ValueError('zero_invalid applies to uint8 images (the image is float32)')
    out_rows, out_cols = resize_shape(rows, cols, factor, out_shape)
    if (out_rows, out_cols) == (rows, cols):
        return image.clone(memory_format=torch.contiguous_format) if is_tensor else np.array(image, copy=True, order='C')
    option = (nan_policy == 'omit') if name == 'float32' else bool(zero_invalid)
    t = image if is_tensor else _prep_upload(image, torch.device('cuda', device))
    out = _resize_device(t, name, out_rows, out_cols, option)
    return out if is_tensor else out.cpu().numpy()


# ---------------------------------------------------------------------------------------------------------------------
# sigma0 preparation: the array half of get_n (reference lib.py:318-331) on the GPU (include/sid_prep.h)
# ---------------------------------------------------------------------------------------------------------------------
SPATIAL_MEAN_STEP = 50             # the reference's subsampling step of get_spatial_mean (lib.py:239)
_PREP_WS = {}                      # per device: the subsample's device buffer and its pinned host copy


def _prep_kind(image, what='image'):
    """(is_tensor, rows, cols) of a 2-D float32 image: NumPy array or ROCm torch tensor with unit inner stride."""
    import torch
    if isinstance(image, torch.Tensor):
        if image.dtype != torch.float32:
            raise NotImplementedError('%s: float32 expected on the device (got %s)' % (what, image.dtype))
        if image.dim() != 2:
            raise ValueError('%s: 2-D array expected (got %d-D)' % (what, image.dim()))
        if not image.is_cuda:
            raise ValueError('a torch input must live on the GPU (pass NumPy arrays for host data)')
        if image.stride(1) != 1 and image.shape[1] > 1:
            raise NotImplementedError('%s: unit inner stride expected (row stride is free)' % what)
        return True, int(image.shape[0]), int(image.shape[1])
    a = np.asarray(image)
    if a.dtype != np.float32:
        raise NotImplementedError('%s: float32 expected on the device (got %s)' % (what, a.dtype))
    if a.ndim != 2:
        raise ValueError('%s: 2-D array expected (got %d-D)' % (what, a.ndim))
    return False, int(a.shape[0]), int(a.shape[1])


def _prep_side(arr, what, is_tensor, shape, mask=False):
    """Check an optional plane (incidence angle: float32; mask: bool / uint8) against the image: same kind, same shape."""
    import torch
    if isinstance(arr, torch.Tensor) != is_tensor:
        raise TypeError('%s: do not mix NumPy arrays and torch tensors in one call' % what)
    if not is_tensor:
        arr = np.asarray(arr)
    if mask:
        ok = arr.dtype in ((torch.bool, torch.uint8) if is_tensor else (np.dtype(bool), np.dtype(np.uint8)))
        if not ok:
            raise NotImplementedError('%s: bool or uint8 expected (got %s)' % (what, arr.dtype))
    elif arr.dtype != (torch.float32 if is_tensor else np.float32):
        raise NotImplementedError('%s: float32 expected on the device (got %s)' % (what, arr.dtype))
    if tuple(arr.shape) != tuple(shape):
        raise ValueError('%s: shape %s differs from the image\'s %s' % (what, tuple(arr.shape), tuple(shape)))
    if is_tensor:
        if not arr.is_cuda:
            raise ValueError('a torch input must live on the GPU (pass NumPy arrays for host data)')
        if arr.stride(1) != 1 and arr.shape[1] > 1:
            raise NotImplementedError('%s: unit inner stride expected (row stride is free)' % what)
    return arr


def _prep_coeffs(coeffs):
    c = np.ascontiguousarray(coeffs, dtype=np.float64)
    if c.shape != (6,):
        raise ValueError('spatial_mean_coeffs: six float64 coefficients expected (col, col^2, row, row^2, col*row, 1), '
                         'got shape %s' % (c.shape,))
    return c


def _prep_upload(arr, dev, mask=False):
    import torch
    a = np.ascontiguousarray(arr)
    if mask:
        a = a.view(np.uint8)
    return torch.from_numpy(a).to(dev)


def _plane(t):
    return (t.data_ptr(), int(t.stride(0)))


def fit_spatial_mean(imgsub, step=SPATIAL_MEAN_STEP):
    """The six coefficients of the reference's get_spatial_mean (lib.py:240-247) from ``imgsub`` = ``img[::step, ::step]``:
    samples that are finite and above the subsample's 5th percentile, the int64 predictors [col, col^2, row, row^2,
    col*row, 1] at the samples' pixel positions, ``np.linalg.lstsq(..., rcond=None)``.  NumPy's own calls on the host -
    whatever they warn or raise for a degenerate subsample is what the caller gets."""
    imgsub = np.asarray(imgsub)
    colsub, rowsub = np.meshgrid(np.arange(0, imgsub.shape[1]) * step, np.arange(0, imgsub.shape[0]) * step)
    gpi = np.isfinite(imgsub) * (imgsub > np.nanpercentile(imgsub, 5))
    z, y, x = imgsub[gpi], rowsub[gpi], colsub[gpi]
    predictors = np.array([x, x ** 2, y, y ** 2, x * y, np.ones_like(x)]).T
    return np.linalg.lstsq(predictors, z, rcond=None)[0]


def _prep_subsample(t, ia, mask, dB, factor, stream, out_shape=None):
    """``[::50, ::50]`` of the image after dB / HH correction / mask, as a NumPy array (a few ten thousand samples).
    ``out_shape``: of the image and incidence angle averaged down to that shape first (``mask`` has that shape)."""
    import torch
    from . import _capi
    full = (int(t.shape[0]), int(t.shape[1]))
    rows, cols = full if out_shape is None else out_shape
    nrs, ncs = -(-rows // SPATIAL_MEAN_STEP), -(-cols // SPATIAL_MEAN_STEP)
    n = nrs * ncs
    dev_index = t.device.index or 0
    ws = _PREP_WS.get(dev_index)
    if ws is None or ws[0].numel() < n:
        cap = max(n, 65536)
        ws = _PREP_WS[dev_index] = (torch.empty(cap, dtype=torch.float32, device=t.device),
                                    torch.empty(cap, dtype=torch.float32, pin_memory=True))
    d_sub, h_sub = ws
    if out_shape is None:
        _capi.prep_subsample(t.data_ptr(), rows, cols, int(t.stride(0)), None if ia is None else _plane(ia),
                             None if mask is None else _plane(mask), dB, factor, SPATIAL_MEAN_STEP, d_sub.data_ptr(), stream.cuda_stream)
    else:
        _capi.resize_prep_subsample(t.data_ptr(), full[0], full[1], int(t.stride(0)), None if ia is None else _plane(ia),
                                    None if mask is None else _plane(mask), dB, factor, SPATIAL_MEAN_STEP, rows, cols,
                                    d_sub.data_ptr(), stream.cuda_stream)
    with torch.cuda.stream(stream):
        h_sub[:n].copy_(d_sub[:n], non_blocking=True)
    stream.synchronize()
    return h_sub[:n].numpy().reshape(nrs, ncs).copy()


def _prep_apply(image, incidence_angle, mask, dB, factor, remove_spatial_mean, coeffs, device, resize=1):
    """Checks, uploads and the one streaming pass: -> (float32 working image on the device, is_tensor).  ``resize`` != 1: the
    pass averages ``image`` and ``incidence_angle`` down to ``resize_shape(rows, cols, resize)`` first (include/sid_resize.h);
    ``mask`` has that shape."""
    import torch
    from . import _capi
    is_tensor, rows, cols = _prep_kind(image)
    out_shape = None
    if resize != 1:
        out_shape = resize_shape(rows, cols, resize)
        if out_shape == (rows, cols):
            out_shape = None
    if incidence_angle is not None:
        incidence_angle = _prep_side(incidence_angle, 'incidence_angle', is_tensor, (rows, cols))
    if mask is not None:
        if out_shape is not None and tuple(np.shape(mask)) != out_shape:
            raise ValueError('mask: shape %s differs from %s, the shape of the %s image at factor=%r (the mask refers to the '
                             'reduced image)' % (tuple(np.shape(mask)), out_shape, (rows, cols), resize))
        mask = _prep_side(mask, 'mask', is_tensor, out_shape or (rows, cols), mask=True)
    if coeffs is not None:
        coeffs = _prep_coeffs(coeffs)
    if rows < 1 or cols < 1:
        raise ValueError('image: empty array')
    dev = image.device if is_tensor else torch.device('cuda', device)
    t = image if is_tensor else _prep_upload(image, dev)
    ia = None if incidence_angle is None else (incidence_angle if is_tensor else _prep_upload(incidence_angle, dev))
    mk = None if mask is None else (mask if is_tensor else _prep_upload(mask, dev, mask=True))
    stream = torch.cuda.current_stream(dev)
    if remove_spatial_mean and coeffs is None:
        coeffs = fit_spatial_mean(_prep_subsample(t, ia, mk, dB, factor, stream, out_shape))
    work = torch.empty(out_shape or (rows, cols), dtype=torch.float32, device=dev)
    if out_shape is not None:
        _capi.resize_prep_apply(t.data_ptr(), rows, cols, int(t.stride(0)), None if ia is None else _plane(ia),
                                None if mk is None else _plane(mk), dB, factor, coeffs if remove_spatial_mean else None,
                                work.data_ptr(), out_shape[0], out_shape[1], int(work.stride(0)), stream.cuda_stream)
        return work, is_tensor
    _capi.prep_apply(t.data_ptr(), rows, cols, int(t.stride(0)), None if ia is None else _plane(ia),
                     None if mk is None else _plane(mk), dB, factor, coeffs if remove_spatial_mean else None,
                     work.data_ptr(), int(work.stride(0)), stream.cuda_stream)
    return work, is_tensor


def hh_angular_correction(n, img, bandName, correct_hh_factor, device=0):
    """sigma0_HH corrected for its incidence-angle dependence on the GPU: signature and result of the reference's
    ``hh_angular_correction`` (lib.py:203-223): ``img - n['incidence_angle'] * correct_hh_factor`` in float32 when
    ``bandName == 'sigma0_HH' and n.has_band('incidence_angle')``, otherwise ``img`` itself.  ``img`` and the incidence
    angle: float32 NumPy arrays (uploaded; a NumPy array comes back) or ROCm torch tensors (a device tensor comes back);
    ``correct_hh_factor`` a Python float (a weak scalar beside the float32 arrays, as in the reference)."""
    if not (bandName == 'sigma0_HH' and n.has_band('incidence_angle')):
        return img
    out, is_tensor = _prep_apply(img, n['incidence_angle'], None, False, float(correct_hh_factor), False, None, device)
    return out if is_tensor else out.cpu().numpy()


def get_spatial_mean(img, device=0):
    """Second-order polynomial approximation of the image's spatial mean brightness: signature and result of the
    reference's ``get_spatial_mean`` (lib.py:225-254), a float64 image.  The fit to every 50th pixel in both directions
    runs on the host (``fit_spatial_mean``); the device evaluates the polynomial at every pixel in the reference's order
    of operations (include/sid_prep.h).  float32 NumPy array in, NumPy array out; ROCm torch tensor in, device tensor out."""
    import torch
    from . import _capi
    is_tensor, rows, cols = _prep_kind(img, 'img')
    if rows < 1 or cols < 1:
        raise ValueError('img: empty array')
    dev = img.device if is_tensor else torch.device('cuda', device)
    stream = torch.cuda.current_stream(dev)
    if is_tensor:
        sub = _prep_subsample(img, None, None, False, 0.0, stream)
    else:
        sub = np.asarray(img)[::SPATIAL_MEAN_STEP, ::SPATIAL_MEAN_STEP]
    coeffs = fit_spatial_mean(sub)
    out = torch.empty((rows, cols), dtype=torch.float64, device=dev)
    _capi.prep_spatial_mean(rows, cols, coeffs, out.data_ptr(), int(out.stride(0)), stream.cuda_stream)
    return out if is_tensor else out.cpu().numpy()


# ---------------------------------------------------------------------------------------------------------------------
# invalid-pixel mask: get_invalid_mask (reference lib.py:342-373) on the GPU (include/sid_mask.h)
# ---------------------------------------------------------------------------------------------------------------------
_MASK_WS = {}                      # per device: the scratch of the water-mask prefilter (grow-only)


def _mask_raster(wm, is_tensor):
    """Check a water-mask raster (2-D uint8, the image's kind, both axes longer than 1) -> (the raster, h, w)."""
    import torch
    if isinstance(wm, torch.Tensor) != is_tensor:
        raise TypeError('watermask: do not mix NumPy arrays and torch tensors in one call')
    if not is_tensor:
        wm = np.asarray(wm)
    if wm.dtype != (torch.uint8 if is_tensor else np.uint8):
        raise NotImplementedError('watermask: uint8 expected (got %s).  The MODIS water mask nansat serves is a byte raster; a raster of '
                                  'another dtype - float64 zeros, say, whose unrounded spline is compared with 2 - follows another '
                                  'specification and is out of scope' % (wm.dtype,))
    if len(wm.shape) != 2:
        raise ValueError('watermask: 2-D array expected (got %d-D)' % len(wm.shape))
    h, w = int(wm.shape[0]), int(wm.shape[1])
    if h < 1 or w < 1:
        raise ValueError('watermask: empty array')
    if h < 2 or w < 2:
        raise ValueError('watermask: shape %s has an axis of length 1 (SciPy does not prefilter such an axis; not supported)' % ((h, w),))
    if is_tensor:
        if not wm.is_cuda:
            raise ValueError('a torch input must live on the GPU (pass NumPy arrays for host data)')
        if wm.stride(1) != 1:
            raise NotImplementedError('watermask: unit inner stride expected (row stride is free)')
    return wm, h, w


def _zoom_shape_check(h, w, H, W):
    """The shape scipy.ndimage.zoom gives the reference's call - round(n_in * (n_out / n_in)) per axis - must be the image's:
    where it is not, the reference's ``mask[wmz == 2]`` raises IndexError, and so does this."""
    got = tuple(int(round(n_in * (n_out / n_in))) for n_in, n_out in ((h, H), (w, W)))
    if got != (H, W):
        raise IndexError('boolean index did not match: the water mask of %s zooms to %s, the image is %s' % ((h, w), got, (H, W)))


def _mask_workspace(dev, h, w):
    import torch
    from . import _capi
    need = _capi.mask_workspace_bytes(h, w)
    key = dev.index or 0
    ws = _MASK_WS.get(key)
    if ws is None or ws.numel() < need:
        ws = _MASK_WS[key] = torch.empty(max(need, 1 << 20), dtype=torch.uint8, device=dev)
    return ws


def _invalid_plane(t, ia, dB, factor, wm, wmz=None):
    """uint8 device plane, 1 = invalid: land (``wm``: device uint8 raster or None) OR the pixel of the device image ``t`` is not
    finite after dB / HH (``t`` None: land alone, of the shape of ``wmz``, which then receives the zoomed bytes)."""
    import torch
    from . import _capi
    ref = t if t is not None else wmz
    H, W, dev = int(ref.shape[0]), int(ref.shape[1]), ref.device
    stream = torch.cuda.current_stream(dev)
    h = w = 0
    work = None
    if wm is not None:
        h, w = int(wm.shape[0]), int(wm.shape[1])
        work = _mask_workspace(dev, h, w)
    with torch.cuda.device(dev):
        if t is None:
            _capi.mask_landmask(_plane(wm), h, w, H, W, work.data_ptr(), None, _plane(wmz), stream.cuda_stream)
            return wmz
        plane = torch.empty((H, W), dtype=torch.uint8, device=dev)
        _capi.mask_invalid(None if wm is None else _plane(wm), h, w, H, W, 0 if work is None else work.data_ptr(), _plane(t), dB,
                           None if ia is None else _plane(ia), factor, _plane(plane), None, stream.cuda_stream)
    return plane


def zoom_landmask(wm, shape, device=0):
    """The uint8 image ``scipy.ndimage.zoom(maximum_filter(np.minimum(wm, 2), 3), np.array(shape) / np.array(wm.shape))`` returns
    (lines 367-369 of the reference's ``get_invalid_mask``; SciPy's defaults: cubic spline, mode 'constant', prefilter), every byte
    of it, computed on the GPU (include/sid_mask.h).  ``wm``: 2-D uint8 NumPy array (a NumPy array comes
    back) or ROCm torch tensor (a device tensor comes back); never modified.  No CPU fallback."""
    import torch
    is_tensor = isinstance(wm, torch.Tensor)
    wm, h, w = _mask_raster(wm, is_tensor)
    H, W = (int(v) for v in shape)
    if H < 1 or W < 1:
        raise ValueError('shape: empty array')
    _zoom_shape_check(h, w, H, W)
    dev = wm.device if is_tensor else torch.device('cuda', device)
    t = wm if is_tensor else _prep_upload(wm, dev)
    out = _invalid_plane(None, None, False, 0.0, t, wmz=torch.empty((H, W), dtype=torch.uint8, device=dev))
    return out if is_tensor else out.cpu().numpy()


def invalid_mask(img, watermask=None, device=0):
    """bool mask of the pixels that are NaN, +-inf or land: what the reference's ``get_invalid_mask`` (lib.py:342-373) computes
    from the image and the water-mask raster ``n.watermask()[1]`` - land is where ``zoom_landmask(watermask, img.shape) == 2``.
    ``watermask=None``: ``isnan(img) | isinf(img)`` alone.  ``img``: 2-D float32, ``watermask``: 2-D uint8; both NumPy arrays (a
    NumPy array comes back) or both ROCm torch tensors (a device tensor comes back); neither is modified.  No CPU fallback."""
    import torch
    is_tensor, H, W = _prep_kind(img, 'img')
    if H < 1 or W < 1:
        raise ValueError('img: empty array')
    if watermask is not None:
        watermask, h, w = _mask_raster(watermask, is_tensor)
        _zoom_shape_check(h, w, H, W)
    dev = img.device if is_tensor else torch.device('cuda', device)
    t = img if is_tensor else _prep_upload(img, dev)
    wm = None if watermask is None else (watermask if is_tensor else _prep_upload(watermask, dev))
    out = _invalid_plane(t, None, False, 0.0, wm).view(torch.bool)
    return out if is_tensor else out.cpu().numpy()


def get_invalid_mask(img, n, landmask_border, device=0):
    """Mask of invalid pixels (land, coast, NaN, inf) on the GPU: signature, protocol and result of the reference's
    ``get_invalid_mask`` (lib.py:342-373): ``n.resize(1. / landmask_border)``, ``n.watermask()[1]`` - when that raises, 'Cannot add
    landmask' is printed and the mask has no land - ``n.undo()``, then ``invalid_mask(img, wm)``.  ``img``: float32 NumPy array
    or ROCm torch tensor (the raster nansat returns is then uploaded); the raster is not modified."""
    import torch
    is_tensor, _, _ = _prep_kind(img, 'img')
    n.resize(1. / landmask_border)
    try:
        wm = n.watermask()[1]
    except:                                      # noqa: E722 - the reference's bare except (lib.py:364)
        print('Cannot add landmask')
        wm = None
    n.undo()
    if is_tensor and wm is not None and not isinstance(wm, torch.Tensor):
        wm = np.asarray(wm)
        if wm.dtype == np.uint8 and wm.ndim == 2 and wm.size:
            wm = _prep_upload(wm, img.device)
    return invalid_mask(img, wm, device)


def prepare_image(image, dB=True, incidence_angle=None, correct_hh_factor=-0.27, mask=None, remove_spatial_mean=False,
                  vmin=None, vmax=None, pmin=10, pmax=99, device=0, spatial_mean_coeffs=None):
    """float32 sigma0 -> the uint8 image that feature tracking and pattern matching read: lines 318-331 of the reference's
    ``get_n`` on arrays, keyword names and defaults from ``get_n`` (lib.py:256-268).

    In ``get_n``'s order: ``dB`` (values <= 0 become NaN, then 10 * log10), the HH angular correction when
    ``incidence_angle`` (float32, same shape) is given, ``mask`` (bool or uint8, same shape, True = invalid: those pixels
    become NaN; stands in for ``get_invalid_mask``), ``remove_spatial_mean`` (minus the second-order polynomial fitted to
    every 50th pixel; ``spatial_mean_coeffs`` - six float64 - skips the fit) and ``get_uint8_image(vmin, vmax, pmin, pmax)``.
    The first four are one pass over the image on the device (include/sid_prep.h), the last is the staging step above.

    NumPy arrays are uploaded and a NumPy array comes back; ROCm torch tensors (unit inner stride, any row stride) are read
    in place on the current stream and a device tensor comes back.  The input is never modified.  Every step repeats
    NumPy's float32 / float64 arithmetic operation for operation, with one documented exception: the float32 logarithm is
    the float64 ``log10`` rounded once, which NumPy's own float32 ``log10`` misses by 1 ulp on about half of all inputs
    (DESIGN.md section 16 has what that means for the uint8 image).  No CPU fallback.

    ``prepare_image_masked`` below is this function with ``get_n``'s ``mask_invalid`` step computed on the device as well,
    ``prepare_image_resized`` is both with ``get_n``'s resize in front."""
    work, is_tensor = _prep_apply(image, incidence_angle, mask, bool(dB), float(correct_hh_factor), bool(remove_spatial_mean),
                                  spatial_mean_coeffs, device)
    out = get_uint8_image(work, vmin, vmax, pmin, pmax)
    return out if is_tensor else out.cpu().numpy()


def prepare_image_masked(image, dB=True, incidence_angle=None, correct_hh_factor=-0.27, mask=None, remove_spatial_mean=False,
                         vmin=None, vmax=None, pmin=10, pmax=99, device=0, spatial_mean_coeffs=None, mask_invalid=False,
                         watermask=None):
    """``prepare_image`` with two more keywords at the end, whose defaults make it ``prepare_image`` itself (that function keeps
    the signature its callers know): ``mask_invalid=True`` is ``get_n``'s own ``mask_invalid`` - the device computes
    ``get_invalid_mask`` of the image after dB / HH (NaN, +-inf and - with ``watermask``, the uint8 raster ``n.watermask()[1]``
    at 1 / landmask_border of the resolution, of the image's kind - land: ``invalid_mask``), ORs ``mask`` in when one is given,
    and that plane is the mask of ``prepare_image``'s steps; it never leaves the device.  So +-inf become NaN before the
    percentiles, as in ``get_n``.  ``watermask`` without ``mask_invalid=True`` raises ValueError."""
    return prepare_image_resized(image, 1, dB, incidence_angle, correct_hh_factor, mask, remove_spatial_mean, vmin, vmax, pmin, pmax,
                                 device, spatial_mean_coeffs, mask_invalid, watermask)


def prepare_image_resized(image, factor=0.5, dB=True, incidence_angle=None, correct_hh_factor=-0.27, mask=None,
                          remove_spatial_mean=False, vmin=None, vmax=None, pmin=10, pmax=99, device=0, spatial_mean_coeffs=None,
                          mask_invalid=False, watermask=None):
    """``prepare_image_masked`` with ``get_n``'s resize in front (``factor``, ``get_n``'s own first keyword with its default;
    the two functions above keep the signatures their callers know): ``image`` and ``incidence_angle`` are full resolution
    and are averaged down as ``resize_image(..., factor)`` does, in the same pass as dB, HH correction, mask and detrend - the
    reduced float images are never written; the result equals ``prepare_image(resize_image(image, factor),
    incidence_angle=resize_image(incidence_angle, factor), ...)`` bit for bit.  ``mask``, and the shape ``watermask`` is
    zoomed to, refer to the reduced image, as in ``get_n``, where the mask is computed after the resize: a mask of another
    shape raises ValueError naming both.  The detrend is fitted to every 50th pixel of the reduced image.  With
    ``mask_invalid=True`` the two planes are averaged down by ``resize_image`` first (the invalid-pixel mask reads the
    reduced image a second time, so it is written once) and the rest is ``prepare_image_masked``'s route.  ``factor=1``:
    no resize."""
    if watermask is not None and not mask_invalid:
        raise ValueError('watermask: needs mask_invalid=True')
    if not mask_invalid:
        work, is_tensor = _prep_apply(image, incidence_angle, mask, bool(dB), float(correct_hh_factor), bool(remove_spatial_mean),
                                      spatial_mean_coeffs, device, factor)
        out = get_uint8_image(work, vmin, vmax, pmin, pmax)
        return out if is_tensor else out.cpu().numpy()
    import torch
    is_tensor, rows, cols = _prep_kind(image)
    if incidence_angle is not None:
        incidence_angle = _prep_side(incidence_angle, 'incidence_angle', is_tensor, (rows, cols))
    if factor != 1:
        full = (rows, cols)
        rows, cols = resize_shape(rows, cols, factor)
        if mask is not None and tuple(np.shape(mask)) != (rows, cols):
            raise ValueError('mask: shape %s differs from %s, the shape of the %s image at factor=%r (the mask refers to the '
                             'reduced image)' % (tuple(np.shape(mask)), (rows, cols), full, factor))
    if mask is not None:
        mask = _prep_side(mask, 'mask', is_tensor, (rows, cols), mask=True)
    if spatial_mean_coeffs is not None:
        spatial_mean_coeffs = _prep_coeffs(spatial_mean_coeffs)
    if rows < 1 or cols < 1:
        raise ValueError('image: empty array')
    if watermask is not None:
        watermask, h, w = _mask_raster(watermask, is_tensor)
        _zoom_shape_check(h, w, rows, cols)
    dev = image.device if is_tensor else torch.device('cuda', device)
    up = (lambda a, **k: a) if is_tensor else (lambda a, **k: _prep_upload(a, dev, **k))
    image = up(image)
    incidence_angle = None if incidence_angle is None else up(incidence_angle)
    if (rows, cols) != (int(image.shape[0]), int(image.shape[1])):
        with torch.cuda.device(dev):
            image = _resize_device(image, 'float32', rows, cols, False)
            incidence_angle = None if incidence_angle is None else _resize_device(incidence_angle, 'float32', rows, cols, False)
    plane = _invalid_plane(image, incidence_angle, bool(dB), float(correct_hh_factor), None if watermask is None else up(watermask))
    if mask is not None:
        plane |= (up(mask, mask=True) != 0).view(torch.uint8)
    work, _ = _prep_apply(image, incidence_angle, plane, bool(dB), float(correct_hh_factor), bool(remove_spatial_mean),
                          spatial_mean_coeffs, device)
    out = get_uint8_image(work, vmin, vmax, pmin, pmax)
    return out if is_tensor else out.cpu().numpy()
