"""Sea-ice deformation from drift vectors: the reference's ``sea_ice_drift.libdefor`` (libdefor.py) on the MI355X.

The per-element pass - corners, sides, perimeter, area, contour integrals, divergence / shear / vorticity - is one HIP kernel
(include/sid_defor.h, csrc/defor.hip) that repeats NumPy's float64 arithmetic operation for operation, so the outputs are the
reference's bit for bit.  The triangulation of ``get_deformation_nodes`` stays the reference's own
call, ``matplotlib.tri.Triangulation`` on the host: its triangles and their order are Qhull's.

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

__all__ = ['get_deformation_elems', 'get_deformation_on_triangulation', 'get_deformation_nodes']


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


def _need_f64(names, arrays):
    for name, a in zip(names, arrays):
        if _dtype_name(a) != 'float64':
            raise NotImplementedError('libdefor: %s is %s; only float64 inputs are implemented (NumPy rounds float32 or mixed '
                                      'inputs differently)' % (name, _dtype_name(a)))


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


def _device_of(arrays):
    dev = arrays[0].device
    for a in arrays:
        if a.device != dev or a.device.type != 'cuda':
            raise TypeError('libdefor: tensors must all be on one ROCm device (got %s)' % [str(b.device) for b in arrays])
    return dev


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
