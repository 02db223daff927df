"""Sea-ice deformation from drift vectors: the reference's ``sea_ice_drift.libdefor`` (libdefor.py) on the MI355X.

The per-element pass - corners, sides, perimeter, area, contour integrals, divergence / shear / vorticity - is one HIP kernel
(include/sid_defor.h, csrc/defor.hip) that repeats NumPy's float64 arithmetic operation for operation, so the outputs are the
reference's bit for bit.  The triangulation of ``get_deformation_nodes`` stays the reference's own
call, ``matplotlib.tri.Triangulation`` on the host: its triangles and their order are Qhull's.  ``get_deformation_grid`` (not
the reference's) needs no triangulation: it takes the 2-D grids ``get_drift_PM`` returns and splits every cell in two
(include/sid_grid.h, csrc/drift_grid.hip).

NumPy arrays in give NumPy arrays out (the call copies to and from device ``device``).  float64 torch tensors on a ROCm
device give tensors on that device out, computed on the caller's current stream with no copy to the host (the call waits for
the stream once, to read the out-of-range flag of the indices).  Only float64 is implemented: NumPy would compute float32 or
mixed inputs with other roundings, so they raise NotImplementedError.  There is no CPU fallback.

Array shapes follow the reference's code, not its docstrings: the triangle array ``t`` is (M, 3), one row of node indices per
triangle (``Triangulation.triangles``), and ``a`` of ``get_deformation_elems`` is (M,).  Indices follow NumPy's indexing:
negative ones wrap, one outside [-N, N) raises IndexError.
"""
import numpy as np

from . import _capi

__all__ = ['get_deformation_elems', 'get_deformation_on_triangulation', 'get_deformation_nodes', 'get_deformation_grid']


def _is_tensor(a):
    return type(a).__module__.split('.')[0] == 'torch'


def _kind(arrays):
    """'tensor' when every argument is a torch tensor, 'numpy' when none is; a mix raises TypeError."""
    flags = [_is_tensor(a) for a in arrays]
    if all(flags):
        return 'tensor'
    if any(flags):
        raise TypeError('libdefor: pass either torch tensors on one ROCm device or NumPy arrays, not a mix')
    return 'numpy'


def _dtype_name(a):
    return str(a.dtype).replace('torch.', '')


def _need_f64(names, arrays, who='libdefor'):
    for name, a in zip(names, arrays):
        if _dtype_name(a) != 'float64':
            raise NotImplementedError('%s: %s is %s; only float64 inputs are implemented (NumPy rounds float32 or mixed '
                                      'inputs differently)' % (who, name, _dtype_name(a)))


def _node_arrays(x, y, u, v):
    if _kind((x, y, u, v)) == 'numpy':
        x, y, u, v = [np.asarray(a) for a in (x, y, u, v)]
    _need_f64('xyuv', (x, y, u, v))
    shapes = [tuple(a.shape) for a in (x, y, u, v)]
    if len(shapes[0]) != 1 or any(s != shapes[0] for s in shapes):
        raise ValueError('libdefor: x, y, u, v must be 1-D arrays of one length N (got shapes %s)' % (shapes,))
    return x, y, u, v


def _index_error(t, n):
    """NumPy's message for the first index of t outside [-n, n)."""
    flat = t.ravel()
    bad = flat[(flat < -n) | (flat >= n)]
    return IndexError('index %d is out of bounds for axis 0 with size %d' % (int(bad[0]), n))


def _triangles(t, n):
    if _dtype_name(t) not in ('int32', 'int64'):
        raise NotImplementedError('libdefor: t is %s; triangle indices must be int32 or int64' % _dtype_name(t))
    if len(t.shape) != 2 or t.shape[1] != 3:
        raise ValueError('libdefor: t must be (M, 3), one row of node indices per triangle (got shape %s)' % (tuple(t.shape),))


def _device_of(arrays, who='libdefor'):
    dev = arrays[0].device
    for a in arrays:
        if a.device != dev or a.device.type != 'cuda':
            raise TypeError('%s: tensors must all be on one ROCm device (got %s)' % (who, [str(b.device) for b in arrays]))
    return dev


def _grid_inputs(who, names, arrays, valid, device):
    """The checks the two grid functions share (this one and libfilter.normalized_median_test): float64 2-D arrays of one
    shape, `valid` bool or uint8 of that shape or None, all NumPy or all tensors on one ROCm device.
    -> kind, arrays, valid (uint8 or None; C-contiguous all), the tensors' device (None for NumPy)."""
    given = tuple(arrays) + ((valid,) if valid is not None else ())
    flags = [_is_tensor(a) for a in given]
    if any(flags) and not all(flags):
        raise TypeError('%s: pass either torch tensors on one ROCm device or NumPy arrays, not a mix' % who)
    kind = 'tensor' if flags[0] else 'numpy'
    if kind == 'numpy':
        arrays = [np.asarray(a) for a in arrays]
        valid = np.asarray(valid) if valid is not None else None
    _need_f64(names, arrays, who)
    shapes = [tuple(a.shape) for a in arrays]
    if len(shapes[0]) != 2 or any(s != shapes[0] for s in shapes):
        raise ValueError('%s: %s must be 2-D arrays of one shape (rows, cols) (got shapes %s)' % (who, ', '.join(names), shapes))
    if valid is not None:
        if _dtype_name(valid) not in ('bool', 'uint8'):
            raise TypeError('%s: valid is %s; it must be bool or uint8' % (who, _dtype_name(valid)))
        if tuple(valid.shape) != shapes[0]:
            raise ValueError('%s: valid must have the shape of the grids, %s (got %s)' % (who, shapes[0], tuple(valid.shape)))
    if kind == 'numpy':
        if int(device) < 0:
            raise ValueError('%s: device must be a HIP device index >= 0 (got %d)' % (who, int(device)))
        arrays = [np.ascontiguousarray(a) for a in arrays]
        if valid is not None:
            valid = np.ascontiguousarray(valid).view(np.uint8)
        return kind, arrays, valid, None
    import torch
    dev = _device_of(given, who)
    arrays = [a.contiguous() for a in arrays]
    if valid is not None:
        valid = valid.contiguous().view(torch.uint8)
    return kind, arrays, valid, dev


def get_deformation_elems(x, y, u, v, a, device=0):
    """Deformation of M elements from the values at their corners (reference: libdefor.get_deformation_elems).

    x, y : (3, M) float64, corner coordinates, m (row k: corner k of every element)
    u, v : (3, M) float64, corner velocities, m/s
    a    : (M,) float64, element areas, m2.  An (M, 1) array is refused (ValueError): NumPy would broadcast the reference's
           result to (M, M).
    device : HIP device of a NumPy call (tensors run on their own device).

    Returns e1, e2, e3 (M,) float64: divergence, shear, vorticity, 1/s (times 8640000 for %/day)."""
    kind = _kind((x, y, u, v, a))
    if kind == 'numpy':
        x, y, u, v, a = [np.asarray(b) for b in (x, y, u, v, a)]
    _need_f64(('x', 'y', 'u', 'v', 'a'), (x, y, u, v, a))
    shapes = [tuple(b.shape) for b in (x, y, u, v)]
    if len(shapes[0]) != 2 or shapes[0][0] != 3 or any(s != shapes[0] for s in shapes):
        raise ValueError('libdefor: x, y, u, v must be (3, M) arrays of one shape (got shapes %s)' % (shapes,))
    m = shapes[0][1]
    if tuple(a.shape) != (m,):
        raise ValueError('libdefor: a must be (M,) = (%d,) (got shape %s)' % (m, tuple(a.shape)))
    if kind == 'numpy':
        x, y, u, v, a = [np.ascontiguousarray(b) for b in (x, y, u, v, a)]
        if m == 0:
            return tuple(np.empty(0, dtype=np.float64) for _ in range(3))
        return _capi.defor_elems(x, y, u, v, a, device=device)
    import torch
    dev = _device_of((x, y, u, v, a))
    x, y, u, v, a = [b.contiguous() for b in (x, y, u, v, a)]
    outs = tuple(torch.empty(m, dtype=torch.float64, device=dev) for _ in range(3))
    if m:
        with torch.cuda.device(dev):
            _capi.defor_elems_device(x.data_ptr(), y.data_ptr(), u.data_ptr(), v.data_ptr(), a.data_ptr(), m,
                                     [o.data_ptr() for o in outs], torch.cuda.current_stream(dev).cuda_stream)
    return outs


def get_deformation_on_triangulation(x, y, u, v, t, device=0):
    """Deformation on a given triangulation (reference: libdefor.get_deformation_on_triangulation).

    x, y : (N,) float64 node coordinates, m;  u, v : (N,) float64 node velocities, m/s
    t    : (M, 3) int32 or int64, node indices of each triangle (negative indices wrap; outside [-N, N): IndexError)
    device : HIP device of a NumPy call (tensors run on their own device).

    Returns e1, e2, e3, a, p (M,) float64: divergence, shear, vorticity (1/s), area (m2), perimeter (m)."""
    kind = _kind((x, y, u, v, t))
    if kind == 'numpy':
        t = np.asarray(t)
    x, y, u, v = _node_arrays(x, y, u, v)
    n = x.shape[0]
    _triangles(t, n)
    m = t.shape[0]
    if kind == 'numpy':
        if m and (t.min() < -n or t.max() >= n):
            raise _index_error(t, n)
        x, y, u, v, t = [np.ascontiguousarray(b) for b in (x, y, u, v, t)]
        if m == 0:
            return tuple(np.empty(0, dtype=np.float64) for _ in range(5))
        return _capi.defor_triangulation(x, y, u, v, t, device=device)
    import torch
    dev = _device_of((x, y, u, v, t))
    x, y, u, v, t = [b.contiguous() for b in (x, y, u, v, t)]
    outs = tuple(torch.empty(m, dtype=torch.float64, device=dev) for _ in range(5))
    if m:
        with torch.cuda.device(dev):
            _capi.defor_triangulation_device(x.data_ptr(), y.data_ptr(), u.data_ptr(), v.data_ptr(), n, t.data_ptr(),
                                             t.dtype == torch.int64, m, [o.data_ptr() for o in outs],
                                             torch.cuda.current_stream(dev).cuda_stream)
    return outs


def get_deformation_nodes(x, y, u, v, device=0):
    """Triangulate the nodes and compute the deformation of every triangle (reference: libdefor.get_deformation_nodes).

    x, y : (N,) float64 node coordinates, m;  u, v : (N,) float64 node velocities, m/s
    device : HIP device of a NumPy call (tensors run on their own device).

    The triangulation is ``matplotlib.tri.Triangulation(x, y)`` on the host, the reference's own call (so its errors too:
    ValueError for fewer than 3 nodes, Qhull's RuntimeError when all nodes are collinear).  Tensor inputs: x and y are
    copied to the host for it, and t is returned as an int32 tensor on their device.

    Returns e1, e2, e3, a, p (M,) float64 and t (M, 3) int32."""
    x, y, u, v = _node_arrays(x, y, u, v)
    from matplotlib.tri import Triangulation
    if _is_tensor(x):
        import torch
        tri = Triangulation(x.detach().cpu().numpy(), y.detach().cpu().numpy())
        t = torch.from_numpy(tri.triangles).to(x.device)
    else:
        tri = Triangulation(x, y)
        t = tri.triangles
    e1, e2, e3, a, p = get_deformation_on_triangulation(x, y, u, v, t, device=device)
    return e1, e2, e3, a, p, t


def get_deformation_grid(x, y, u, v, valid=None, diagonal='shorter', device=0):
    """Deformation on the grid's own triangles: every cell of a (R, C) grid of drift vectors is split in two, no triangulation
    (not the reference's; specification: include/sid_grid.h).

    x, y : (R, C) float64 node coordinates, m;  u, v : (R, C) float64 node velocities, m/s - the grids as get_drift_PM returns
           them, NaN where there is no result
    valid : (R, C) bool or uint8, or None.  A node takes part when valid (or no mask) and x, y, u, v are finite - e.g. the
            ``keep`` of libfilter.normalized_median_test
    diagonal : 'shorter' (the shorter diagonal of each cell - the Delaunay one of a parallelogram; ties take the main one),
               'main' ((i, j) - (i+1, j+1)) or 'anti' ((i, j+1) - (i+1, j))
    device : HIP device of a NumPy call (tensors run on their own device).

    A cell with four usable nodes holds two triangles, one with three holds one (slot 0), fewer none; triangles are
    counter-clockwise.  Each triangle's values are get_deformation_on_triangulation's on its three nodes.

    Returns e1, e2, e3, a, p (R-1, C-1, 2) float64 - NaN where a slot holds no triangle - and t (R-1, C-1, 2, 3) int32, flat
    node numbers (row * C + column), -1 there.  NumPy in gives NumPy out; tensors give tensors on their device, computed on the
    caller's current stream with no wait and no copy to the host."""
    if diagonal not in _capi.GRID_DIAGONALS:
        raise ValueError("libdefor: diagonal must be 'shorter', 'main' or 'anti' (got %r)" % (diagonal,))
    kind, (x, y, u, v), valid, dev = _grid_inputs('libdefor', ('x', 'y', 'u', 'v'), (x, y, u, v), valid, device)
    rows, cols = x.shape
    shape = (max(rows - 1, 0), max(cols - 1, 0), 2)
    code = _capi.GRID_DIAGONALS[diagonal]
    if kind == 'numpy':
        if shape[0] * shape[1] == 0:
            return tuple(np.empty(shape, dtype=np.float64) for _ in range(5)) + (np.empty(shape + (3,), dtype=np.int32),)
        return _capi.grid_deformation(x, y, u, v, valid, code, device=device)
    import torch
    outs = tuple(torch.empty(shape, dtype=torch.float64, device=dev) for _ in range(5)) + (
        torch.empty(shape + (3,), dtype=torch.int32, device=dev),)
    if shape[0] * shape[1]:
        with torch.cuda.device(dev):
            _capi.grid_deformation_device(x.data_ptr(), y.data_ptr(), u.data_ptr(), v.data_ptr(),
                                          valid.data_ptr() if valid is not None else 0, rows, cols, code,
                                          [o.data_ptr() for o in outs], torch.cuda.current_stream(dev).cuda_stream)
    return outs
