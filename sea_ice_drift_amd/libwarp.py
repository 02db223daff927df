"""Warp an image along a drift grid on the MI355X: piecewise affine, one streaming pass (not the reference's: it has no
resampling step).

A grid of nodes is known in two frames - where each node lies in the output (``x``, ``y``) and where the same node lies in
the source image (``xs``, ``ys``), both in pixels (x = column, y = row; an integer is a pixel centre).  The grid is cut into
the triangles of ``libdefor.get_deformation_grid``; inside a triangle the source position of an output pixel is the linear
interpolant of the three nodes.  Specification: include/sid_warp.h; kernels: csrc/warp.hip.

NumPy arrays in give NumPy arrays out (the call copies to and from device ``device``).  Torch tensors on one ROCm device give
tensors on that device, computed on the caller's current stream with no copy to the host and no wait.  A mix raises
TypeError.  There is no CPU fallback.
"""
import numpy as np

from . import _capi
from .libdefor import _dtype_name, _grid_inputs, _is_tensor

__all__ = ['warp_image', 'warp_maps']

WHO = 'libwarp'


def _out_shape(out_shape, default):
    if out_shape is None:
        if default is None:
            raise ValueError('%s: out_shape is needed when there is no image' % WHO)
        return default
    try:
        ro, co = [int(q) for q in out_shape]
    except (TypeError, ValueError):
        raise ValueError('%s: out_shape must be (rows, cols) (got %r)' % (WHO, out_shape))
    if ro < 0 or co < 0 or (ro, co) != tuple(out_shape):
        raise ValueError('%s: out_shape must be two integers >= 0 (got %r)' % (WHO, out_shape))
    return ro, co


def _run(image, x, y, xs, ys, out_shape, valid, order, fill, diagonal, keep_zero, want_out, want_covered, want_maps, device):
    if diagonal not in _capi.GRID_DIAGONALS:
        raise ValueError("%s: diagonal must be 'shorter', 'main' or 'anti' (got %r)" % (WHO, diagonal))
    if order not in (0, 1):
        raise ValueError('%s: order must be 0 (nearest) or 1 (bilinear) (got %r)' % (WHO, order))
    if image is not None and _is_tensor(image) != _is_tensor(x):
        raise TypeError('%s: pass either torch tensors on one ROCm device or NumPy arrays, not a mix' % WHO)
    if int(device) < -1:
        raise ValueError('%s: device must be a HIP device index >= 0, or -1 for the host instance (got %d)' % (WHO, int(device)))
    kind, (x, y, xs, ys), valid, dev = _grid_inputs(WHO, ('x', 'y', 'xs', 'ys'), (x, y, xs, ys), valid, max(int(device), 0))
    dtype, src_shape = 'uint8', (0, 0)
    if image is not None:
        if kind == 'numpy':
            image = np.asarray(image)
        dtype = _dtype_name(image)
        if dtype not in _capi.WARP_DTYPES:
            raise TypeError('%s: image is %s; it must be uint8 or float32' % (WHO, dtype))
        if len(image.shape) != 2:
            raise ValueError('%s: image must be 2-D (rows, cols) (got shape %s)' % (WHO, tuple(image.shape)))
        src_shape = tuple(int(q) for q in image.shape)
    ro, co = _out_shape(out_shape, src_shape if image is not None else None)
    if keep_zero is None:
        keep_zero = dtype == 'uint8'
    if keep_zero and dtype != 'uint8':
        raise ValueError('%s: keep_zero is for uint8 images (0 = invalid); image is %s' % (WHO, dtype))
    fill = float(fill)
    if dtype == 'uint8' and not (0 <= fill <= 255 and fill == int(fill)):
        raise ValueError('%s: fill must be a uint8 value for a uint8 image (got %r)' % (WHO, fill))
    flags = _capi.WARP_KEEP_ZERO if keep_zero else 0
    code = _capi.GRID_DIAGONALS[diagonal]
    if kind == 'numpy':
        if image is not None and (image.strides[1] != image.itemsize or image.strides[0] < image.shape[1] * image.itemsize
                                  or image.strides[0] % image.itemsize):
            image = np.ascontiguousarray(image)                     # (rows a whole number of elements apart, unit inner stride)
        return _capi.warp_image(x, y, xs, ys, valid, image, dtype, src_shape, (ro, co), order, fill, code, flags,
                                want_out, want_covered, want_maps, device=device)
    import torch
    if image is not None:
        if image.device != dev:
            raise TypeError('%s: tensors must all be on one ROCm device (got %s and %s)' % (WHO, image.device, dev))
        if image.numel() == 0:
            image = image.new_zeros((1, max(src_shape[1], 1)))         # (an address to hand over; src_shape says nothing is in range)
        elif image.stride(1) != 1 or image.stride(0) < image.shape[1]:
            image = image.contiguous()
    out = torch.empty((ro, co), dtype=getattr(torch, dtype), device=dev) if want_out else None
    covered = torch.empty((ro, co), dtype=torch.uint8, device=dev) if want_covered else None
    map_x = torch.empty((ro, co), dtype=torch.float32, device=dev) if want_maps else None
    map_y = torch.empty((ro, co), dtype=torch.float32, device=dev) if want_maps else None
    ptr = lambda t: t.data_ptr() if t is not None else 0                                            # noqa: E731
    if ro * co == 0:                                                    # (an empty tensor has no address to hand over)
        return out, covered, map_x, map_y
    with torch.cuda.device(dev):
        _capi.warp_image_device(x.data_ptr(), y.data_ptr(), xs.data_ptr(), ys.data_ptr(), ptr(valid), x.shape[0], x.shape[1],
                                ptr(image), dtype, src_shape, image.stride(0) if image is not None else 0, (ro, co), order, fill,
                                code, flags, ptr(out), co, ptr(covered), ptr(map_x), ptr(map_y),
                                torch.cuda.current_stream(dev).cuda_stream)
    return out, covered, map_x, map_y


def warp_image(image, x, y, xs, ys, out_shape=None, valid=None, order=1, fill=0, diagonal='shorter', keep_zero=None,
               return_covered=False, device=0):
    """Resample ``image`` into the frame of the nodes (x, y).

    image : (rows_s, cols_s) uint8 or float32
    x, y  : (R, C) float64, the nodes in the output frame, pixels;  xs, ys : (R, C) float64, the same nodes in ``image``
    out_shape : (rows, cols) of the result; the image's shape when None
    valid : (R, C) bool or uint8, or None.  A node takes part when valid (or no mask) and x, y, xs, ys are finite - e.g. the
            ``keep`` of libfilter.normalized_median_test
    order : 0 (nearest, ties to even) or 1 (bilinear)
    fill  : the value of pixels that no triangle owns or whose source lies outside ``image``
    diagonal : 'shorter', 'main' or 'anti', as in libdefor.get_deformation_grid
    keep_zero : with order 1, a result that a 0 pixel (the project's invalid value) takes part in is 0.  Default: True for
                uint8, False for float32 (where it is refused)
    return_covered : also return the uint8 mask of the pixels that hold a resampled value
    device : HIP device of a NumPy call (tensors run on their own device); -1 runs the kernels' source in a host loop, without
             a GPU (slow: for tests)

    Returns the (rows, cols) image of ``image``'s dtype, or (image, covered)."""
    if image is None:
        raise ValueError('%s: image is None (warp_maps gives the maps alone)' % WHO)
    out, covered, _, _ = _run(image, x, y, xs, ys, out_shape, valid, order, fill, diagonal, keep_zero, True,
                              bool(return_covered), False, device)
    return (out, covered) if return_covered else out


def warp_maps(x, y, xs, ys, out_shape, valid=None, diagonal='shorter', device=0):
    """The dense maps of the warp: for every pixel of a (rows, cols) output the position in the source frame it comes from,
    float32 ``map_x`` (column) and ``map_y`` (row) as remap functions take them; NaN where no triangle owns the pixel.
    Arguments as in ``warp_image``."""
    _, _, map_x, map_y = _run(None, x, y, xs, ys, out_shape, valid, 1, 0, diagonal, False, False, False, True, device)
    return map_x, map_y
