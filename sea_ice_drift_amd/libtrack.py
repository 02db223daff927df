"""Map arbitrary points through a drift grid on the MI355X (not the reference's): where does this point lie in the other image?

A grid of nodes is known in two frames - (``x``, ``y``) and (``xs``, ``ys``), pixels, x = column, y = row - and cut into the
triangles of ``libdefor.get_deformation_grid``; a point of the first frame that a triangle has is carried to the second by the
triangle's linear interpolant.  It is the field ``libwarp`` resamples images with, evaluated at scattered points: a buoy, an
ice parcel, the nodes of another grid.  Specification: include/sid_track.h; kernels: csrc/track.hip.

NumPy arrays in give NumPy arrays out (the call copies to and from device ``device``).  Torch tensors on one ROCm device give
tensors on that device, computed on the caller's current stream with no copy to the host and no wait.  A mix raises
TypeError.  There is no CPU fallback.
"""
import numpy as np

from . import _capi
from .libdefor import _grid_inputs, _is_tensor, _need_f64

__all__ = ['map_points', 'advect', 'round_trip']

WHO = 'libtrack'


def _device_arg(device):
    if int(device) < -1:
        raise ValueError('%s: device must be a HIP device index >= 0, or -1 for the host instance (got %d)' % (WHO, int(device)))
    return int(device)


def _points(px, py, tensors):
    """px, py of one kind with the grids, float64, of one shape."""
    if _is_tensor(px) != tensors or _is_tensor(py) != tensors:
        raise TypeError('%s: pass either torch tensors on one ROCm device or NumPy arrays, not a mix' % WHO)
    if not tensors:
        px, py = np.asarray(px), np.asarray(py)
    _need_f64(('px', 'py'), (px, py), WHO)
    if tuple(px.shape) != tuple(py.shape):
        raise ValueError('%s: px and py must have one shape (got %s and %s)' % (WHO, tuple(px.shape), tuple(py.shape)))
    return px, py


def map_points(x, y, xs, ys, px, py, valid=None, diagonal='shorter', closed=True, return_triangle=False, device=0):
    """The positions (px, py) of the frame of (x, y) in the frame of (xs, ys).

    x, y  : (R, C) float64, the nodes in the points' frame, pixels;  xs, ys : (R, C) float64, the same nodes in the other frame
    px, py : float64 of one shape (any shape), the points
    valid : (R, C) bool or uint8, or None.  A node takes part when valid (or no mask) and x, y, xs, ys are finite - e.g. the
            ``keep`` of libfilter.normalized_median_test
    diagonal : 'shorter', 'main' or 'anti', as in libdefor.get_deformation_grid
    closed : True - a point on the rim of the mesh (the first column and last row of nodes of a regular grid, which the
             half-open ownership rule of the image warp leaves to no triangle) belongs to the triangle it touches.  False - the
             image warp's rule alone: at pixel centres the result is ``libwarp.warp_maps`` before its cast to float32
    return_triangle : also return int32 ``2 * cell + slot`` of the triangle each point lies in (cell = i * (C - 1) + j), -1: none
    device : HIP device of a NumPy call (tensors run on their own device); -1 runs the kernels' source in a host loop, without
             a GPU (slow: for tests)

    Returns sx, sy float64 of px's shape, NaN where no triangle has the point or the point is not finite (and the triangles).
    Where triangles overlap (a folded mesh) the one with the lowest number has the point."""
    if diagonal not in _capi.GRID_DIAGONALS:
        raise ValueError("%s: diagonal must be 'shorter', 'main' or 'anti' (got %r)" % (WHO, diagonal))
    device = _device_arg(device)
    kind, (x, y, xs, ys), valid, dev = _grid_inputs(WHO, ('x', 'y', 'xs', 'ys'), (x, y, xs, ys), valid, max(device, 0))
    px, py = _points(px, py, kind == 'tensor')
    shape = tuple(px.shape)
    code, flags = _capi.GRID_DIAGONALS[diagonal], _capi.TRACK_CLOSED if closed else 0
    if kind == 'numpy':
        px, py = np.ascontiguousarray(px).reshape(-1), np.ascontiguousarray(py).reshape(-1)
        sx, sy, tri = _capi.track_points(x, y, xs, ys, valid, code, flags, px, py, want_tri=bool(return_triangle), device=device)
        sx, sy = sx.reshape(shape), sy.reshape(shape)
        return (sx, sy, tri.reshape(shape)) if return_triangle else (sx, sy)
    import torch
    for name, t in (('px', px), ('py', py)):
        if t.device != dev:
            raise TypeError('%s: tensors must all be on one ROCm device (%s is on %s, the grids on %s)' % (WHO, name, t.device, dev))
    px, py = px.contiguous(), py.contiguous()
    sx = torch.empty(shape, dtype=torch.float64, device=dev)
    sy = torch.empty(shape, dtype=torch.float64, device=dev)
    tri = torch.empty(shape, dtype=torch.int32, device=dev) if return_triangle else None
    if px.numel():                                                      # (an empty tensor has no address to hand over)
        with torch.cuda.device(dev):
            _capi.track_points_device(x.data_ptr() or 1, y.data_ptr() or 1, xs.data_ptr() or 1, ys.data_ptr() or 1,
                                      valid.data_ptr() if valid is not None else 0, x.shape[0], x.shape[1], code, flags,
                                      px.data_ptr(), py.data_ptr(), px.numel(), sx.data_ptr(), sy.data_ptr(),
                                      tri.data_ptr() if tri is not None else 0, torch.cuda.current_stream(dev).cuda_stream)
    return (sx, sy, tri) if return_triangle else (sx, sy)


def advect(px, py, fields, closed=True, return_path=False, device=0):
    """Carry points through the drift fields of consecutive pairs (t0 -> t1 -> t2 ...), each on its own grid.

    px, py : float64 of one shape, the points in the first frame of the first field
    fields : a sequence of (x, y, xs, ys) or (x, y, xs, ys, valid), applied in order: ``map_points`` of each
    closed, device : as in ``map_points``; every field is cut along its cells' shorter diagonals
    return_path : also return the positions after every field

    A point that leaves a mesh is NaN from then on; NaN in gives NaN out.
    Returns px, py after the last field and ``steps``, the int32 count of fields each point came through with finite
    coordinates (and path_x, path_y of shape (K + 1, ...), the start included, on request)."""
    tensors = _is_tensor(px)
    px, py = _points(px, py, tensors)
    fields = list(fields)
    if tensors:
        import torch
        finite, stack = lambda a, b: (torch.isfinite(a) & torch.isfinite(b)).to(torch.int32), torch.stack           # noqa: E731
        steps = torch.zeros(tuple(px.shape), dtype=torch.int32, device=px.device)
    else:
        finite, stack = lambda a, b: (np.isfinite(a) & np.isfinite(b)).astype(np.int32), np.stack                   # noqa: E731
        steps = np.zeros(px.shape, dtype=np.int32)
    path_x, path_y = [px], [py]
    for k, field in enumerate(fields):
        if len(field) not in (4, 5):
            raise ValueError('%s: field %d must be (x, y, xs, ys) or (x, y, xs, ys, valid) (got %d items)' % (WHO, k, len(field)))
        valid = field[4] if len(field) == 5 else None
        px, py = map_points(field[0], field[1], field[2], field[3], px, py, valid=valid, closed=closed, device=device)
        steps = steps + finite(px, py)
        path_x.append(px)
        path_y.append(py)
    if return_path:
        return px, py, steps, stack(path_x), stack(path_y)
    return px, py, steps


def round_trip(x, y, xs, ys, xb, yb, xbs, ybs, valid=None, valid_b=None, diagonal='shorter', closed=True, device=0):
    """The forward-backward check of a drift field: every forward end point goes through the backward field, and what is
    returned is how far it lands from where it started.

    x, y, xs, ys, valid : the forward field, nodes (x, y) of image 1 found at (xs, ys) on image 2 - (R, C) float64
    xb, yb, xbs, ybs, valid_b : the backward field on its own grid, nodes (xb, yb) of image 2 found at (xbs, ybs) on image 1
    diagonal, closed, device : as in ``map_points`` (of the backward field)

    Returns dx, dy (R, C) float64, pixels of image 1: the backward field at (xs, ys), minus (x, y) - one subtraction each.  NaN
    where the forward node is not usable or the backward field has no triangle there.  Typical use:
    ``keep &= np.hypot(dx, dy) < tol`` before ``libfilter.clean_drift``."""
    device = _device_arg(device)
    kind, (x, y, xs, ys), valid, _ = _grid_inputs(WHO, ('x', 'y', 'xs', 'ys'), (x, y, xs, ys), valid, max(device, 0))
    if kind == 'tensor':
        import torch
        usable = torch.isfinite(x) & torch.isfinite(y) & torch.isfinite(xs) & torch.isfinite(ys)
        if valid is not None:
            usable = usable & (valid != 0)
        nan = torch.full_like(xs, float('nan'))
        qx, qy = torch.where(usable, xs, nan), torch.where(usable, ys, nan)
    else:
        usable = np.isfinite(x) & np.isfinite(y) & np.isfinite(xs) & np.isfinite(ys)
        if valid is not None:
            usable = usable & (valid != 0)
        qx, qy = np.where(usable, xs, np.nan), np.where(usable, ys, np.nan)
    bx, by = map_points(xb, yb, xbs, ybs, qx, qy, valid=valid_b, diagonal=diagonal, closed=closed, device=device)
    return bx - x, by - y
