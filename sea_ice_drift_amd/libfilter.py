"""Outlier filter for grids of drift vectors on the MI355X: the normalised median test of PIV practice (Westerweel and Scarano,
"Universal outlier detection for PIV data", 2005).  Not the reference's - it offers only a threshold on r * h.

A deformation is a difference of neighbouring vectors, so one wrong match ruins every triangle it touches; this marks the
vectors that disagree with the median of their neighbours, and ``libdefor.get_deformation_grid(valid=keep)`` leaves them out.
One HIP kernel (include/sid_grid.h, csrc/drift_grid.hip) with an exact float64 specification (NumPy
restatement: tests/grid_spec.py).  There is no CPU fallback.
"""
import math

import numpy as np

from . import _capi
from .libdefor import _grid_inputs

__all__ = ['normalized_median_test']


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
