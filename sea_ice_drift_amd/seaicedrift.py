"""``SeaIceDrift`` with the reference's public methods (reference seaicedrift.py:23-88).

``get_drift_PM`` is the hot path; ``get_drift_FT`` runs the key-point detector (``sea_ice_drift_amd.orb``, an
ORB-family detector behind the reference's interface - OpenCV is not used) and the Hamming matcher on the GPU and
the reference's filters on the host; a ``find_key_points=`` callable replaces the detector.  The
constructor takes two Nansat-like objects (``sea_ice_drift_amd.domain.ArrayNansat`` or real
``nansat.Nansat``); opening Sentinel-1 files (reference lib.get_n, lib.py:256-340) needs nansat/GDAL and
is outside the scope of this package - passing file names raises with a pointer to what to pass instead.
"""
from sea_ice_drift_amd.ftlib import feature_tracking
from sea_ice_drift_amd.lib import get_drift_vectors, prefetch_triangulation
from sea_ice_drift_amd.libcorr import local_correlation_at
from sea_ice_drift_amd.libtrack import map_points, round_trip
from sea_ice_drift_amd.libwarp import warp_image
from sea_ice_drift_amd.pmlib import pattern_matching


class SeaIceDrift(object):
    """Retrieve sea ice drift with pattern matching on an MI355X."""

    def __init__(self, n1, n2, devices=None, first_guess_method=None, **kwargs):
        """``devices``: the GPUs that ``get_drift_FT`` and ``get_drift_PM`` use unless a call names its own - None (one
        handle, GPU ``device=`` of the call), 'all', a count or a sequence of GPU indices (``pmlib.resolve_devices``).
        ``first_guess_method`` (not the reference's): the ``method=`` of ``get_drift_PM`` unless a call names its own - None
        (the reference's 'linear') or e.g. 'knn', the triangulation-free first guess of ``lib.interpolation_near``; with
        'knn' ``get_drift_FT`` starts no triangulation ahead of ``get_drift_PM``."""
        for n in (n1, n2):
            if isinstance(n, str):
                raise NotImplementedError(
                    'file staging (reference lib.get_n) is out of scope here: open the files with '
                    'sea_ice_drift.lib.get_n / nansat yourself and pass the two Nansat objects, '
                    'or wrap uint8 arrays in sea_ice_drift_amd.domain.ArrayNansat')
        self.n1 = n1
        self.n2 = n2
        self.devices = devices
        self.first_guess_method = first_guess_method

    def get_drift_FT(self, **kwargs):
        """Same returns as the reference (seaicedrift.py:42-60): u, v, lon1, lat1, lon2, lat2 of the matched
        key points.  Detection and matching run on the GPU (``sea_ice_drift_amd.orb``, ``include/sid_ft.h``), the
        filters on the host; ``find_key_points=`` takes another detector (see ``ftlib.feature_tracking``).  ``nsr=``
        selects the units of u, v as in the reference (``lib.get_drift_vectors``).  ``devices=`` (or the constructor's): the
        key points of image 1 on its first GPU, those of image 2 on its second (``ftlib.feature_tracking``)."""
        if self.devices is not None:
            kwargs.setdefault('devices', self.devices)
        x1, y1, x2, y2 = feature_tracking(self.n1, self.n2, **kwargs)
        kwargs.pop('find_key_points', None)
        kwargs.pop('devices', None)
        out = get_drift_vectors(self.n1, x1, y1, self.n2, x2, y2, **kwargs)
        self._prefetch_first_guess(out[2], out[3])
        return out

    def _prefetch_first_guess(self, lon1, lat1):
        """The usual next call is ``get_drift_PM(lons, lats, lon1, lat1, lon2, lat2)`` with these very vectors; its prelude
        triangulates the key points of image 1 carried into the pixel space of image 2 (pmlib.py:280-288 through
        lib.interpolation_near) - the longest step of the call.  The same arithmetic on the same numbers, started now on a
        worker thread: whatever the caller does before ``get_drift_PM`` runs beside the triangulation, and the call picks
        the result up when its points are bit-identical (otherwise it triangulates as before).  Results are unchanged."""
        try:
            import os
            import numpy as np
            if len(lon1) < 4 or os.environ.get('SID_NO_TRI_PREFETCH'):   # (the switch: A/B runs)
                return
            if self.first_guess_method == 'knn':                         # (that first guess has no triangulation)
                return
            x1, y1 = self.n1.transform_points(lon1, lat1, 1)             # get_drift_PM (seaicedrift.py:85)
            lon, lat = self.n1.transform_points(x1, y1)                  # prepare_first_guess (pmlib.py:280-282)
            c1n2, r1n2 = self.n2.transform_points(lon, lat, 1)
            prefetch_triangulation(np.array([r1n2, c1n2]).T)             # interpolation_near's point order (lib.py:195)
        except Exception:                                                # noqa: BLE001 - a convenience, never an error
            pass

    def get_drift_PM(self, lons, lats, lon1, lat1, lon2, lat2, **kwargs):
        """Same arguments and returns as the reference (seaicedrift.py:62-88):
        u, v, a, r, h, lon2_dst, lat2_dst on the (lons, lats) grid.  ``devices=`` (or the constructor's) spreads the grid
        points over several GPUs (``pmlib.pattern_matching``).

        Keyword arguments that are NOT the reference's: those of ``pmlib.pattern_matching``, among them ``subpixel=True`` -
        drift with the parabolic sub-pixel offset of the correlation peak, what ``libdefor`` wants to be fed."""
        if self.devices is not None:
            kwargs.setdefault('devices', self.devices)
        if self.first_guess_method is not None:
            kwargs.setdefault('method', self.first_guess_method)
        x1, y1 = self.n1.transform_points(lon1, lat1, 1)
        x2, y2 = self.n2.transform_points(lon2, lat2, 1)
        return pattern_matching(lons, lats, self.n1, x1, y1, self.n2, x2, y2, **kwargs)

    def get_warped_image(self, lons, lats, lon2, lat2, to=1, **kwargs):
        """One image of the pair resampled into the other's frame along a drift grid (not the reference's; ``libwarp``).

        lons, lats : (R, C) grid of start positions on image 1, as given to ``get_drift_PM``
        lon2, lat2 : (R, C) the positions of the same ice on image 2, as ``get_drift_PM`` returns them (NaN: no result)
        to : 1 - image 2 in the frame of image 1 (motion compensated: to look at, or to difference with image 1);
             2 - image 1 in the frame of image 2
        Other keyword arguments are those of ``libwarp.warp_image`` (``valid=``, ``order=``, ``fill=``, ``return_covered=``...).

        Returns the warped uint8 image with the shape of the frame it is in (and the covered mask on request)."""
        import numpy as np
        shape = np.shape(lons)
        if len(shape) != 2 or any(np.shape(a) != shape for a in (lats, lon2, lat2)):
            raise ValueError('get_warped_image: lons, lats, lon2, lat2 must be 2-D grids of one shape (got %s)'
                             % ([np.shape(a) for a in (lons, lats, lon2, lat2)],))
        if to not in (1, 2):
            raise ValueError('get_warped_image: to must be 1 or 2 (got %r)' % (to,))
        x1, y1 = [np.asarray(a, dtype=np.float64).reshape(shape) for a in self.n1.transform_points(lons, lats, 1)]
        x2, y2 = [np.asarray(a, dtype=np.float64).reshape(shape) for a in self.n2.transform_points(lon2, lat2, 1)]
        if to == 1:
            return warp_image(self.n2[1], x1, y1, x2, y2, out_shape=tuple(self.n1.shape()), **kwargs)
        return warp_image(self.n1[1], x2, y2, x1, y1, out_shape=tuple(self.n2.shape()), **kwargs)

    def get_warp_correlation(self, lons, lats, lon2, lat2, window=35, min_count=None, return_count=False, device=0, **kwargs):
        """How well the drift field lines the pair up, node by node (not the reference's; ``libcorr``): image 2 is warped into
        the frame of image 1 (``get_warped_image(..., to=1)``) and correlated with image 1 in a ``window`` x ``window`` square
        around every node of the grid.

        lons, lats, lon2, lat2 : as in ``get_warped_image``
        window, min_count, return_count : as in ``libcorr.local_correlation_at``
        Other keyword arguments are the warp's (``valid=``, ``order=``, ``diagonal=``).

        Returns r with the shape of ``lons`` (NaN at nodes whose position on image 1 is not finite, and where too few
        pixels of the window hold both images), and the int32 count of usable pixels on request."""
        import numpy as np
        warped = self.get_warped_image(lons, lats, lon2, lat2, to=1, device=device, **kwargs)
        shape = np.shape(lons)
        x1, y1 = [np.asarray(a, dtype=np.float64).reshape(shape) for a in self.n1.transform_points(lons, lats, 1)]
        finite = np.isfinite(x1) & np.isfinite(y1)
        return local_correlation_at(self.n1[1], warped, np.rint(x1), np.rint(y1), window=window, valid=finite, min_count=min_count,
                                    return_count=return_count, device=device)

    def track_points(self, lon, lat, lons, lats, lon2, lat2, **kwargs):
        """Where arbitrary positions on image 1 - buoys, parcels, the nodes of another grid - lie on image 2 according to a
        drift grid (not the reference's; ``libtrack.map_points``).

        lon, lat : the positions, any one shape
        lons, lats, lon2, lat2 : as in ``get_warped_image``
        Other keyword arguments are those of ``libtrack.map_points`` (``valid=``, ``diagonal=``, ``closed=``, ``device=``).

        Returns lon2_pts, lat2_pts with the shape of ``lon``, NaN outside the field."""
        import numpy as np
        shape = np.shape(lons)
        if len(shape) != 2 or any(np.shape(a) != shape for a in (lats, lon2, lat2)):
            raise ValueError('track_points: lons, lats, lon2, lat2 must be 2-D grids of one shape (got %s)'
                             % ([np.shape(a) for a in (lons, lats, lon2, lat2)],))
        if np.shape(lon) != np.shape(lat):
            raise ValueError('track_points: lon and lat must have one shape (got %s and %s)' % (np.shape(lon), np.shape(lat)))
        x1, y1 = [np.asarray(a, dtype=np.float64).reshape(shape) for a in self.n1.transform_points(lons, lats, 1)]
        x2, y2 = [np.asarray(a, dtype=np.float64).reshape(shape) for a in self.n2.transform_points(lon2, lat2, 1)]
        px, py = [np.asarray(a, dtype=np.float64).reshape(np.shape(lon)) for a in self.n1.transform_points(lon, lat, 1)]
        sx, sy = map_points(x1, y1, x2, y2, px, py, **kwargs)
        lon_pts, lat_pts = [np.asarray(a, dtype=np.float64).reshape(np.shape(lon)) for a in self.n2.transform_points(sx, sy, 0)]
        gone = ~(np.isfinite(sx) & np.isfinite(sy))                       # (whatever the projection makes of a NaN pixel)
        return np.where(gone, np.nan, lon_pts), np.where(gone, np.nan, lat_pts)

    def get_round_trip(self, lons, lats, lon2, lat2, lons_b, lats_b, lon1_b, lat1_b, **kwargs):
        """The forward-backward check of a drift grid (not the reference's; ``libtrack.round_trip``): every end point of the
        forward field 1 -> 2 is sent through the backward field 2 -> 1; what comes back is how far it lands from its start.

        lons, lats, lon2, lat2 : the forward field, as in ``get_warped_image``
        lons_b, lats_b : (Rb, Cb) the grid of start positions on image 2 that ``SeaIceDrift(n2, n1).get_drift_PM`` was given
        lon1_b, lat1_b : (Rb, Cb) the positions on image 1 it returned (NaN: no result)
        Other keyword arguments are those of ``libtrack.round_trip`` (``valid=``, ``valid_b=``, ``diagonal=``, ``closed=``,
        ``device=``).

        Returns dx, dy in pixels of image 1, shaped like ``lons``; NaN where either field has nothing to say."""
        import numpy as np
        shape, shape_b = np.shape(lons), np.shape(lons_b)
        if len(shape) != 2 or any(np.shape(a) != shape for a in (lats, lon2, lat2)):
            raise ValueError('get_round_trip: lons, lats, lon2, lat2 must be 2-D grids of one shape (got %s)'
                             % ([np.shape(a) for a in (lons, lats, lon2, lat2)],))
        if len(shape_b) != 2 or any(np.shape(a) != shape_b for a in (lats_b, lon1_b, lat1_b)):
            raise ValueError('get_round_trip: lons_b, lats_b, lon1_b, lat1_b must be 2-D grids of one shape (got %s)'
                             % ([np.shape(a) for a in (lons_b, lats_b, lon1_b, lat1_b)],))
        x, y = [np.asarray(a, dtype=np.float64).reshape(shape) for a in self.n1.transform_points(lons, lats, 1)]
        xs, ys = [np.asarray(a, dtype=np.float64).reshape(shape) for a in self.n2.transform_points(lon2, lat2, 1)]
        xb, yb = [np.asarray(a, dtype=np.float64).reshape(shape_b) for a in self.n2.transform_points(lons_b, lats_b, 1)]
        xbs, ybs = [np.asarray(a, dtype=np.float64).reshape(shape_b) for a in self.n1.transform_points(lon1_b, lat1_b, 1)]
        return round_trip(x, y, xs, ys, xb, yb, xbs, ybs, **kwargs)
