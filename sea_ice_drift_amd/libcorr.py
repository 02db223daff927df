"""Local correlation of two uint8 images on the MI355X: the zero-mean normalised correlation over a square window around each
node, on a regular lattice (a map) or at given points (not the reference's: it has no such step).

The use: image 1 against image 2 warped onto it (``libwarp.warp_image``) - how well the drift field lines the pair up, and
where; and the detection of change between the scenes.  0 is the project's invalid value: a pixel takes part when it is not 0
in either image.  Specification: include/sid_corr.h; kernels: csrc/local_corr.hip.

NumPy arrays in give NumPy arrays out (the call copies to and from device ``device``).  Torch tensors on one ROCm device give
tensors on that device, computed on the caller's current stream with no copy to the host and no wait.  A mix raises
TypeError.  There is no CPU fallback.
"""
import numpy as np

from . import _capi
from .libdefor import _dtype_name, _is_tensor

__all__ = ['local_correlation', 'local_correlation_at']

WHO = 'libcorr'


def _images(a, b, device, others=()):
    """-> kind ('numpy' or 'tensor'), a, b (uint8, 2-D, one shape, unit inner stride), the tensors' device (None for NumPy)."""
    given = [a, b] + [q for q in others if q is not None]
    flags = [_is_tensor(q) for q in given]
    if any(flags) and not all(flags):
        raise TypeError('%s: pass either torch tensors on one ROCm device or NumPy arrays, not a mix' % WHO)
    if int(device) < -1:
        raise ValueError('%s: device must be a HIP device index >= 0, or -1 for the host instance (got %d)' % (WHO, int(device)))
    kind = 'tensor' if flags[0] else 'numpy'
    if kind == 'numpy':
        a, b = np.asarray(a), np.asarray(b)
    for name, img in (('a', a), ('b', b)):
        if _dtype_name(img) != 'uint8':
            raise TypeError('%s: %s is %s; it must be uint8 (0 = invalid)' % (WHO, name, _dtype_name(img)))
        if len(img.shape) != 2:
            raise ValueError('%s: %s must be 2-D (rows, cols) (got shape %s)' % (WHO, name, tuple(img.shape)))
    if tuple(a.shape) != tuple(b.shape):
        raise ValueError('%s: a and b must have one shape (got %s and %s)' % (WHO, tuple(a.shape), tuple(b.shape)))
    if kind == 'numpy':
        a, b = [q if q.strides[1] == 1 and q.strides[0] >= q.shape[1] else np.ascontiguousarray(q) for q in (a, b)]
        return kind, a, b, None
    dev = a.device
    if dev.type != 'cuda' or any(q.device != dev for q in given):
        raise TypeError('%s: tensors must all be on one ROCm device (got %s)' % (WHO, [str(q.device) for q in given]))
    a, b = [q if q.numel() == 0 or (q.stride(1) == 1 and q.stride(0) >= q.shape[1]) else q.contiguous() for q in (a, b)]
    return kind, a, b, dev


def _window(window):
    w = int(window)
    if w != window or not 1 <= w <= 255:
        raise ValueError('%s: window must be an integer in 1..255 (got %r)' % (WHO, window))
    return w


def _min_count(min_count, w):
    if min_count is None:
        return (w * w + 1) // 2
    m = int(min_count)
    if m != min_count or m < 1:
        raise ValueError('%s: min_count must be an integer >= 1 (got %r)' % (WHO, min_count))
    return m


def _pair(value, name, least=None):
    try:
        p = (value, value) if np.ndim(value) == 0 else tuple(value)
        q = tuple(int(v) for v in p)
    except (TypeError, ValueError):
        raise ValueError('%s: %s must be an integer or two integers (got %r)' % (WHO, name, value))
    if len(q) != 2 or q != tuple(p) or (least is not None and min(q) < least):
        raise ValueError('%s: %s must be an integer or two integers%s (got %r)'
                         % (WHO, name, '' if least is None else ' >= %d' % least, value))
    return q


def _results(r, count, sums, return_count, return_sums):
    out = (r,) + ((count,) if return_count else ()) + ((sums,) if return_sums else ())
    return out if len(out) > 1 else r


def _address(t):
    """A tensor's address for the C call; an empty image has none, and nothing is read from it: any non-null value does."""
    return t.data_ptr() or 1


def _stride(t):
    return t.stride(0) if t.shape[0] > 1 and t.shape[1] > 0 else max(int(t.shape[1]), 0)


def local_correlation(a, b, window=35, step=1, origin=None, shape=None, min_count=None, return_count=False, return_sums=False,
                      device=0):
    """The map of local correlation of ``a`` against ``b`` on a regular lattice of nodes.

    a, b : (rows, cols) uint8, 0 = invalid
    window : side w of the square window, 1..255; a node at (rc, cc) takes the rows rc - w//2 .. rc - w//2 + w - 1 and the
             columns likewise, clipped to the image
    step : distance of the nodes in pixels, an int or (sr, sc)
    origin : (r0, c0), the centre of node (0, 0); any integers.  Default (w//2, w//2): the first window starts at pixel 0
    shape : (nr, nc) nodes.  Default: the nodes whose windows lie wholly inside the image
    min_count : fewest usable pixels of a window that give a value.  Default: half the window, (w*w + 1)//2
    return_count : also return the int32 number of usable pixels per node
    return_sums : also return the int64 (nr, nc, 5) sums Sa, Sb, Saa, Sbb, Sab over the usable pixels
    device : HIP device of a NumPy call (tensors run on their own device); -1 runs the kernels' source in a host loop, without
             a GPU (slow: for tests)

    Returns r (nr, nc) float64 in [-1, 1], NaN where fewer than min_count pixels are usable or either image is constant
    there; then count and sums as asked."""
    kind, a, b, dev = _images(a, b, device)
    w = _window(window)
    sr, sc = _pair(step, 'step', least=1)
    r0, c0 = (w // 2, w // 2) if origin is None else _pair(origin, 'origin')
    rows, cols = int(a.shape[0]), int(a.shape[1])
    if shape is None:
        nr, nc = [(n - w) // s + 1 if n >= w else 0 for n, s in ((rows, sr), (cols, sc))]
    else:
        nr, nc = _pair(shape, 'shape', least=0)
    m = _min_count(min_count, w)
    if kind == 'numpy':
        return _results(*_capi.corr_lattice(a, b, w, r0, c0, sr, sc, nr, nc, m, True, bool(return_count), bool(return_sums),
                                            device=device), return_count, return_sums)
    import torch
    r = torch.empty((nr, nc), dtype=torch.float64, device=dev)
    count = torch.empty((nr, nc), dtype=torch.int32, device=dev) if return_count else None
    sums = torch.empty((nr, nc, 5), dtype=torch.int64, device=dev) if return_sums else None
    if nr * nc:
        with torch.cuda.device(dev):
            _capi.corr_lattice_device(_address(a), _stride(a), _address(b), _stride(b), rows, cols, w, r0, c0, sr, sc, nr, nc, m,
                                      r.data_ptr(), count.data_ptr() if return_count else 0, sums.data_ptr() if return_sums else 0,
                                      torch.cuda.current_stream(dev).cuda_stream)
    return _results(r, count, sums, return_count, return_sums)


def _centres(kind, c, r, valid):
    """c, r as int32 of one shape (float input must hold integers), valid as uint8 of that shape or None; C-contiguous all."""
    if kind == 'numpy':
        c, r = np.asarray(c), np.asarray(r)
        valid = np.asarray(valid) if valid is not None else None
    if tuple(c.shape) != tuple(r.shape):
        raise ValueError('%s: c and r must have one shape (got %s and %s)' % (WHO, tuple(c.shape), tuple(r.shape)))
    if valid is not None:
        if _dtype_name(valid) not in ('bool', 'uint8'):
            raise TypeError('%s: valid is %s; it must be bool or uint8' % (WHO, _dtype_name(valid)))
        if tuple(valid.shape) != tuple(c.shape):
            raise ValueError('%s: valid must have the shape of c, %s (got %s)' % (WHO, tuple(c.shape), tuple(valid.shape)))
    out = []
    for name, q in (('c', c), ('r', r)):
        dt = _dtype_name(q)
        if dt.startswith('float'):
            if kind == 'numpy':
                ok = valid.astype(bool) if valid is not None else np.ones(q.shape, dtype=bool)
                whole = bool(np.all((q[ok] == np.rint(q[ok])) & (np.abs(q[ok]) < 2.0 ** 31)))
                q = np.where(ok, q, 0)
            else:
                import torch
                ok = valid.bool() if valid is not None else torch.ones_like(q, dtype=torch.bool)
                q = torch.where(ok, q, torch.zeros_like(q))
                whole = None                                            # (asking would be a wait and a copy to the host)
            if whole is False:
                raise ValueError('%s: %s holds values that are not integers (of int32); round them first' % (WHO, name))
        elif not (dt.startswith('int') or dt.startswith('uint')):
            raise TypeError('%s: %s is %s; it must be an integer array (or a float array that holds integers)' % (WHO, name, dt))
        if kind == 'numpy':
            if q.size and not dt.startswith('float') and (int(q.min()) < -2 ** 31 or int(q.max()) >= 2 ** 31):
                raise ValueError('%s: %s holds values that int32 cannot hold' % (WHO, name))
            q = np.ascontiguousarray(q, dtype=np.int32 if dt != 'int32' else None)
        else:
            import torch
            q = q.to(torch.int32).contiguous()
        out.append(q)
    if valid is not None:
        if kind == 'numpy':
            valid = np.ascontiguousarray(valid, dtype=np.uint8)
        else:
            import torch
            valid = valid.to(torch.uint8).contiguous()
    return out[0], out[1], valid


def local_correlation_at(a, b, c, r, window=35, valid=None, min_count=None, return_count=False, return_sums=False, device=0):
    """The local correlation of ``a`` against ``b`` in windows centred at the given pixels.

    c, r : columns and rows of the centres, integer arrays (or tensors) of any one shape; float arrays must hold integers
           (ValueError otherwise; tensors are not asked - that would be a wait - and are truncated).  Centres may lie outside
           the image: the window is clipped, and an empty one gives NaN
    valid : bool or uint8 of that shape, or None.  A node with valid == 0 gets NaN, count 0 and zero sums; its centre is not
            looked at
    Other arguments and the results as in ``local_correlation``, with the shape of ``c``."""
    kind, a, b, dev = _images(a, b, device, others=(c, r, valid))
    w = _window(window)
    m = _min_count(min_count, w)
    c, r, valid = _centres(kind, c, r, valid)
    shape = tuple(c.shape)
    rows, cols = int(a.shape[0]), int(a.shape[1])
    if kind == 'numpy':
        out, count, sums = _capi.corr_points(a, b, w, c.reshape(-1), r.reshape(-1), valid.reshape(-1) if valid is not None else None,
                                             m, True, bool(return_count), bool(return_sums), device=device)
        return _results(out.reshape(shape), count.reshape(shape) if return_count else None,
                        sums.reshape(shape + (5,)) if return_sums else None, return_count, return_sums)
    import torch
    out = torch.empty(shape, dtype=torch.float64, device=dev)
    count = torch.empty(shape, dtype=torch.int32, device=dev) if return_count else None
    sums = torch.empty(shape + (5,), dtype=torch.int64, device=dev) if return_sums else None
    if c.numel():
        with torch.cuda.device(dev):
            _capi.corr_points_device(_address(a), _stride(a), _address(b), _stride(b), rows, cols, w, c.data_ptr(), r.data_ptr(),
                                     valid.data_ptr() if valid is not None else 0, c.numel(), m, out.data_ptr(),
                                     count.data_ptr() if return_count else 0, sums.data_ptr() if return_sums else 0,
                                     torch.cuda.current_stream(dev).cuda_stream)
    return _results(out, count, sums, return_count, return_sums)
