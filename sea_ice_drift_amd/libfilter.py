"""Outlier filter for grids of drift vectors on the MI355X: the normalised median test of PIV practice (Westerweel and Scarano,
"Universal outlier detection for PIV data", 2005).  Not the reference's - it offers only a threshold on r * h.

A deformation is a difference of neighbouring vectors, so one wrong match ruins every triangle it touches; this marks the
vectors that disagree with the median of their neighbours, and ``libdefor.get_deformation_grid(valid=keep)`` leaves them out.
One HIP kernel (include/sid_grid.h, csrc/drift_grid.hip) with an exact float64 specification (NumPy
restatement: tests/grid_spec.py).  There is no CPU fallback.

PIV practice runs three steps - detect, replace, smooth - and the other two are here as well, not the reference's either:
``fill_gaps`` replaces rejected vectors by the median of their neighbours, pass by pass from the rim of a hole inwards,
``smooth`` is a normalised convolution over the usable nodes, and ``clean_drift`` chains an iterated detection with both
(NumPy restatement: tests/grid_fill_spec.py).  HIP kernels of the same file, tensors in and out on the
caller's stream.
"""
import math

import numpy as np

from . import _capi
from .libdefor import _device_of, _dtype_name, _grid_inputs, _is_tensor

__all__ = ['normalized_median_test', 'fill_gaps', 'smooth', 'gaussian_weights', 'clean_drift']


def normalized_median_test(u, v, eps, valid=None, threshold=2.0, radius=1, min_neighbours=3, device=0):
    """Normalised median test of every node of a (R, C) grid of drift vectors, one pass.

    u, v : (R, C) float64, the grids as get_drift_PM returns them (NaN where there is no result)
    eps  : the noise of a good vector, in the unit of u (> 0; no default).  0.1 - 0.2 pixel spacings is the usual choice: for
           drift in m/s, 0.1 - 0.2 x pixel size / time between the images
    valid : (R, C) bool or uint8, or None.  A node is usable when valid (or no mask) and u, v are finite
    threshold : a node is kept when its residual is <= threshold (2.0: the customary value)
    radius : 1 (3 x 3 window) or 2 (5 x 5)
    min_neighbours : a node with fewer usable neighbours in its window is not judged and not kept (1 .. (2 radius + 1)^2 - 1)
    device : HIP device of a NumPy call (tensors run on their own device).

    For a usable node with the usable neighbours N of its window (centre excluded, clipped at the grid's edges):
        um = median(u_N) ; mu = median(|u_N - um|) ; ru = |u - um| / (mu + eps)      (rv: the same with v)
        res = sqrt(ru^2 + rv^2) ; keep = res <= threshold
    Neighbours that are outliers themselves take part: the median is what makes that safe.

    Returns keep (R, C) bool and res (R, C) float64 (NaN where the node is unusable or was not judged; keep is False there).
    NumPy in gives NumPy out; tensors give tensors on their device, computed on the caller's current stream with no wait and
    no copy to the host."""
    eps, threshold = float(eps), float(threshold)
    if not (math.isfinite(eps) and eps > 0.0):
        raise ValueError('libfilter: eps must be finite and > 0 (got %r)' % (eps,))
    if not (math.isfinite(threshold) and threshold > 0.0):
        raise ValueError('libfilter: threshold must be finite and > 0 (got %r)' % (threshold,))
    if radius not in (1, 2):
        raise ValueError('libfilter: radius must be 1 or 2 (got %r)' % (radius,))
    most = (2 * radius + 1) ** 2 - 1
    if int(min_neighbours) != min_neighbours or not 1 <= min_neighbours <= most:
        raise ValueError('libfilter: min_neighbours must be in 1..%d for radius %d (got %r)' % (most, radius, min_neighbours))
    kind, (u, v), valid, dev = _grid_inputs('libfilter', ('u', 'v'), (u, v), valid, device)
    rows, cols = u.shape
    if kind == 'numpy':
        if rows * cols == 0:
            return np.zeros((rows, cols), dtype=bool), np.empty((rows, cols), dtype=np.float64)
        keep, res = _capi.grid_filter(u, v, valid, eps, threshold, radius, min_neighbours, device=device)
        return keep.view(bool), res
    import torch
    keep = torch.empty((rows, cols), dtype=torch.uint8, device=dev)
    res = torch.empty((rows, cols), dtype=torch.float64, device=dev)
    if rows * cols:
        with torch.cuda.device(dev):
            _capi.grid_filter_device(u.data_ptr(), v.data_ptr(), valid.data_ptr() if valid is not None else 0, rows, cols,
                                     eps, threshold, radius, min_neighbours, keep.data_ptr(), res.data_ptr(),
                                     torch.cuda.current_stream(dev).cuda_stream)
    return keep.view(torch.bool), res


def _check_window(radius, min_neighbours):
    if radius not in (1, 2):
        raise ValueError('libfilter: radius must be 1 or 2 (got %r)' % (radius,))
    most = (2 * radius + 1) ** 2 - 1
    if int(min_neighbours) != min_neighbours or not 1 <= min_neighbours <= most:
        raise ValueError('libfilter: min_neighbours must be in 1..%d for radius %d (got %r)' % (most, radius, min_neighbours))


def _second_mask(name, mask, kind, shape, dev):
    """A second node mask under the rules libdefor._grid_inputs applies to `valid` -> uint8, C-contiguous, or None."""
    if mask is None:
        return None
    if _is_tensor(mask) != (kind == 'tensor'):
        raise TypeError('libfilter: pass either torch tensors on one ROCm device or NumPy arrays, not a mix')
    if kind == 'numpy':
        mask = np.asarray(mask)
    if _dtype_name(mask) not in ('bool', 'uint8'):
        raise TypeError('libfilter: %s is %s; it must be bool or uint8' % (name, _dtype_name(mask)))
    if tuple(mask.shape) != tuple(shape):
        raise ValueError('libfilter: %s must have the shape of the grids, %s (got %s)' % (name, tuple(shape), tuple(mask.shape)))
    if kind == 'numpy':
        return np.ascontiguousarray(mask).view(np.uint8)
    import torch
    if _device_of((mask,), 'libfilter') != dev:
        raise TypeError('libfilter: tensors must all be on one ROCm device (got %s for %s)' % (mask.device, name))
    return mask.contiguous().view(torch.uint8)


def fill_gaps(u, v, valid=None, domain=None, radius=1, min_neighbours=3, max_passes=16, device=0):
    """Replace the unusable nodes of a (R, C) grid of drift vectors by the median of their neighbours, pass by pass from the
    rim of every hole inwards.  Not the reference's: it replaces nothing.

    u, v : (R, C) float64 (NaN where there is no result)
    valid : (R, C) bool or uint8, or None - e.g. the `keep` of normalized_median_test.  A node is usable when valid (or no
            mask) and u, v are finite; usable nodes are generation 0 and come back bit for bit
    domain : (R, C) bool or uint8, or None: where it is 0 a node is never filled (land, the outside of the ice cover)
    radius : 1 (3 x 3 window) or 2 (5 x 5)
    min_neighbours : a node is filled in a pass when that many nodes of its window hold a value (1 .. (2 radius + 1)^2 - 1)
    max_passes : 1 .. 256.  Pass p fills what has enough neighbours of the generations 0 .. p-1 with finite values:
            u_f = median(u_N) + 0.0, v_f likewise (the filter's median).  A pass reads only earlier generations, so the
            result does not depend on the order of the nodes; a pass that fills nothing ends the process.
    device : HIP device of a NumPy call (tensors run on their own device).

    Returns u_f, v_f (R, C) float64 and gen (R, C) int32: 0 for the usable nodes, the pass that filled a node, -1 (with NaN
    in u_f and v_f) for the nodes never filled.  A median of values near the largest float64 may overflow to inf: that node
    keeps its generation and is nobody's neighbour afterwards.  NumPy in gives NumPy out; tensors give tensors on their
    device, computed on the caller's current stream (max_passes launches) with no wait and no copy to the host."""
    _check_window(radius, min_neighbours)
    if int(max_passes) != max_passes or not 1 <= max_passes <= 256:
        raise ValueError('libfilter: max_passes must be in 1..256 (got %r)' % (max_passes,))
    kind, (u, v), valid, dev = _grid_inputs('libfilter', ('u', 'v'), (u, v), valid, device)
    domain = _second_mask('domain', domain, kind, u.shape, dev)
    rows, cols = u.shape
    if kind == 'numpy':
        if rows * cols == 0:
            return np.empty((rows, cols)), np.empty((rows, cols)), np.empty((rows, cols), dtype=np.int32)
        return _capi.grid_fill(u, v, valid, domain, radius, min_neighbours, max_passes, device=device)
    import torch
    uf, vf = torch.empty_like(u), torch.empty_like(v)
    gen = torch.empty((rows, cols), dtype=torch.int32, device=dev)
    if rows * cols:
        with torch.cuda.device(dev):
            _capi.grid_fill_device(u.data_ptr(), v.data_ptr(), valid.data_ptr() if valid is not None else 0,
                                   domain.data_ptr() if domain is not None else 0, rows, cols, radius, min_neighbours,
                                   max_passes, uf.data_ptr(), vf.data_ptr(), gen.data_ptr(),
                                   torch.cuda.current_stream(dev).cuda_stream)
    return uf, vf, gen


def gaussian_weights(sigma, radius):
    """The default weight table of smooth: exp(-(di^2 + dj^2) / (2 sigma^2)) for di, dj = -radius .. radius, computed by
    NumPy on the host -> (2 radius + 1, 2 radius + 1) float64."""
    sigma = float(sigma)
    if not (math.isfinite(sigma) and sigma > 0.0):
        raise ValueError('libfilter: sigma must be finite and > 0 (got %r)' % (sigma,))
    if radius not in (1, 2):
        raise ValueError('libfilter: radius must be 1 or 2 (got %r)' % (radius,))
    di, dj = np.meshgrid(np.arange(-radius, radius + 1, dtype=np.float64), np.arange(-radius, radius + 1, dtype=np.float64),
                         indexing='ij')
    return np.exp(-(di * di + dj * dj) / (2.0 * sigma * sigma))


def smooth(u, v, sigma=1.0, radius=1, valid=None, weights=None, device=0):
    """Normalised convolution of a (R, C) grid of drift vectors over its usable nodes: a weighted mean of the usable nodes of
    the window, the centre included, so holes and edges take no weight and bias nothing.  Not the reference's.

    u, v : (R, C) float64
    sigma : width of the default Gaussian table, in nodes (ignored when `weights` is given)
    radius : 1 (3 x 3 window) or 2 (5 x 5)
    valid : (R, C) bool or uint8, or None.  A node is usable when valid (or no mask) and u, v are finite
    weights : (2 radius + 1, 2 radius + 1) float64 NumPy array (or nested sequence) in place of gaussian_weights(sigma,
            radius): every entry finite and >= 0, the centre > 0.  It stays on the host and travels as a kernel argument: no
            exp runs on the device
    device : HIP device of a NumPy call (tensors run on their own device).

    For a usable node: sw = su = sv = 0; for di = -radius .. radius, for dj = -radius .. radius, for a usable node
    (i + di, j + dj): sw += w ; su += w * u ; sv += w * v, in that order; u_s = su / sw, v_s = sv / sw.

    Returns u_s, v_s (R, C) float64, NaN in both where the node is unusable.  NumPy in gives NumPy out; tensors give tensors
    on their device, computed on the caller's current stream with no wait and no copy to the host."""
    if radius not in (1, 2):
        raise ValueError('libfilter: radius must be 1 or 2 (got %r)' % (radius,))
    side = 2 * radius + 1
    if weights is None:
        weights = gaussian_weights(sigma, radius)
    else:
        if _is_tensor(weights):
            raise TypeError('libfilter: weights is a host table: pass a NumPy array, not a tensor')
        weights = np.ascontiguousarray(weights, dtype=np.float64)
        if weights.shape != (side, side):
            raise ValueError('libfilter: weights must be (%d, %d) for radius %d (got %s)' % (side, side, radius, weights.shape))
        if not (np.isfinite(weights).all() and (weights >= 0.0).all() and weights[radius, radius] > 0.0):
            raise ValueError('libfilter: weights must be finite and >= 0, the centre > 0')
    kind, (u, v), valid, dev = _grid_inputs('libfilter', ('u', 'v'), (u, v), valid, device)
    rows, cols = u.shape
    if kind == 'numpy':
        if rows * cols == 0:
            return np.empty((rows, cols)), np.empty((rows, cols))
        return _capi.grid_smooth(u, v, valid, weights, radius, device=device)
    import torch
    us, vs = torch.empty_like(u), torch.empty_like(v)
    if rows * cols:
        with torch.cuda.device(dev):
            _capi.grid_smooth_device(u.data_ptr(), v.data_ptr(), valid.data_ptr() if valid is not None else 0, rows, cols,
                                     weights, radius, us.data_ptr(), vs.data_ptr(), torch.cuda.current_stream(dev).cuda_stream)
    return us, vs


def clean_drift(u, v, eps, valid=None, domain=None, threshold=2.0, radius=1, min_neighbours=3, detect_passes=2, max_passes=16,
                sigma=None, device=0):
    """Detect, replace, smooth: the three steps of PIV practice on a (R, C) grid of drift vectors.  Not the reference's.

    Detect : S_0 = the usable nodes (valid, or no mask, and u, v finite).  For k = 1 .. detect_passes:
             res = normalized_median_test(u, v, eps, valid=S_{k-1}, threshold, radius, min_neighbours)[1] and
             S_k = S_{k-1} & ~(res > threshold): rejected vectors are left out of the next pass's medians.  Only a node that
             was JUDGED and failed is removed; a node with too few neighbours to be judged (res = NaN) stays in S, unlike in
             the filter's own `keep`, which would drop good nodes at the rim of the holes pass after pass.
    Fill   : fill_gaps(u, v, valid=S, domain, radius, min_neighbours, max_passes)
    Smooth : when sigma is not None, smooth(u_f, v_f, sigma, radius, valid=(gen >= 0)); else nothing.

    eps, threshold, radius, min_neighbours : as in normalized_median_test, for every step that takes them
    domain, max_passes : as in fill_gaps;  detect_passes : >= 0;  sigma : None, or the Gaussian width of smooth.

    Returns u_c, v_c (R, C) float64, keep = S (R, C) bool and gen (R, C) int32 as fill_gaps gives it.  NumPy in gives NumPy
    out; tensors give tensors on their device, every step on the caller's current stream with nothing going to the host in
    between."""
    if int(detect_passes) != detect_passes or detect_passes < 0:
        raise ValueError('libfilter: detect_passes must be an integer >= 0 (got %r)' % (detect_passes,))
    eps, threshold = float(eps), float(threshold)                  # every refusal before the first step runs
    if not (math.isfinite(eps) and eps > 0.0):
        raise ValueError('libfilter: eps must be finite and > 0 (got %r)' % (eps,))
    if not (math.isfinite(threshold) and threshold > 0.0):
        raise ValueError('libfilter: threshold must be finite and > 0 (got %r)' % (threshold,))
    _check_window(radius, min_neighbours)
    if int(max_passes) != max_passes or not 1 <= max_passes <= 256:
        raise ValueError('libfilter: max_passes must be in 1..256 (got %r)' % (max_passes,))
    if sigma is not None:
        gaussian_weights(sigma, radius)
    kind, (u, v), valid, dev = _grid_inputs('libfilter', ('u', 'v'), (u, v), valid, device)
    domain = _second_mask('domain', domain, kind, u.shape, dev)
    if kind == 'numpy':
        keep = np.isfinite(u) & np.isfinite(v)
    else:
        import torch
        keep = torch.isfinite(u) & torch.isfinite(v)
    if valid is not None:
        keep = keep & (valid != 0)
    for _ in range(int(detect_passes)):
        _, res = normalized_median_test(u, v, eps, valid=keep, threshold=threshold, radius=radius,
                                        min_neighbours=min_neighbours, device=device)
        keep = keep & ~(res > threshold)
    uc, vc, gen = fill_gaps(u, v, valid=keep, domain=domain, radius=radius, min_neighbours=min_neighbours,
                            max_passes=max_passes, device=device)
    if sigma is not None:
        uc, vc = smooth(uc, vc, sigma=sigma, radius=radius, valid=gen >= 0, device=device)
    return uc, vc, keep, gen
