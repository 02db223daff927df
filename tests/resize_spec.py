"""Specification of the area-average downsampling (include/sid_resize.h) in NumPy / Python, written from the
text of the header and shared by the host and the GPU tests.

Per axis (n input length, m output length): g = gcd(n, m), a = n / g, b = m / g; output index j covers [j a, (j + 1) a) and source
index i covers [i b, (i + 1) b) of a common fine axis; the weight of i in j is the integer length of the overlap.

``resize_f32`` / ``resize_u8`` walk every window in row-major order, one output ROW at a time (NumPy operations across the
columns of that row: the same scalar operations in the same order for every pixel).  ``resize_f32_scalar`` / ``resize_u8_scalar``
are the same text pixel by pixel in plain Python, for the small cases of the host tests.
"""
import math

import numpy as np

MAX_DIM = 1 << 24


def out_shape(rows, cols, factor):
    """(int(rows * factor), int(cols * factor)) in Python float arithmetic; ValueError for a factor that is not in (0, 1] or a
    dimension that comes out as 0."""
    factor = float(factor)
    if not math.isfinite(factor) or factor <= 0.0 or factor > 1.0:
        raise ValueError('factor %r is not in (0, 1]' % (factor,))
    shape = (int(rows * factor), int(cols * factor))
    if shape[0] < 1 or shape[1] < 1:
        raise ValueError('factor %r leaves an empty image' % (factor,))
    return shape


def axis_weights(n, m):
    """(a, b, first, weights): for every output index j, first[j] = its first source index and weights[j] = the list of integer
    weights of the sources first[j], first[j] + 1, ..."""
    if not (1 <= m <= n <= MAX_DIM):
        raise ValueError('need 1 <= m <= n <= 2^24 (got n = %r, m = %r)' % (n, m))
    g = math.gcd(n, m)
    a, b = n // g, m // g
    first, weights = [], []
    for j in range(m):
        s, e = j * a, (j + 1) * a
        i0, i1 = s // b, -(-e // b) - 1
        first.append(i0)
        weights.append([min((i + 1) * b, e) - max(i * b, s) for i in range(i0, i1 + 1)])
    return a, b, first, weights


def _padded(first, weights):
    """The weight lists as arrays [m, longest]: source index, weight (0 past the end of a window)."""
    width = max(len(w) for w in weights)
    idx = np.zeros((len(weights), width), dtype=np.int64)
    wgt = np.zeros((len(weights), width), dtype=np.int64)
    for j, (i0, w) in enumerate(zip(first, weights)):
        idx[j, :len(w)] = np.arange(i0, i0 + len(w))
        idx[j, len(w):] = i0
        wgt[j, :len(w)] = w
    return idx, wgt


def resize_f32(x, out_rows, out_cols, nan_policy='propagate'):
    x = np.asarray(x)
    assert x.dtype == np.float32 and x.ndim == 2 and nan_policy in ('propagate', 'omit')
    rows, cols = x.shape
    if (out_rows, out_cols) == (rows, cols):
        return x.copy()
    ar, _, rfirst, rweights = axis_weights(rows, out_rows)
    ac, _, cfirst, cweights = axis_weights(cols, out_cols)
    cidx, cwgt = _padded(cfirst, cweights)
    total = float(ar * ac)
    out = np.empty((out_rows, out_cols), dtype=np.float32)
    with np.errstate(all='ignore'):
        for r in range(out_rows):
            acc = np.zeros(out_cols, dtype=np.float64)
            used = np.zeros(out_cols, dtype=np.int64)
            for i, wr in zip(range(rfirst[r], rfirst[r] + len(rweights[r])), rweights[r]):
                row = x[i].astype(np.float64)
                for t in range(cidx.shape[1]):
                    w = wr * cwgt[:, t]                                # the integer product ...
                    v = row[cidx[:, t]]
                    take = w > 0
                    if nan_policy == 'omit':
                        take = take & ~np.isnan(v)
                    term = w.astype(np.float64) * v                    # ... converted once; one rounding for the product
                    acc = np.where(take, acc + term, acc)              # and one for the sum
                    used = np.where(take, used + w, used)
            if nan_policy == 'omit':
                out[r] = np.where(used > 0, acc / used.astype(np.float64), np.nan).astype(np.float32)
            else:
                out[r] = (acc / total).astype(np.float32)
    return out


def resize_u8(x, out_rows, out_cols, zero_invalid=True):
    x = np.asarray(x)
    assert x.dtype == np.uint8 and x.ndim == 2
    rows, cols = x.shape
    if (out_rows, out_cols) == (rows, cols):
        return x.copy()
    ar, _, rfirst, rweights = axis_weights(rows, out_rows)
    ac, _, cfirst, cweights = axis_weights(cols, out_cols)
    cidx, cwgt = _padded(cfirst, cweights)
    total = ar * ac
    out = np.empty((out_rows, out_cols), dtype=np.uint8)
    for r in range(out_rows):
        S = np.zeros(out_cols, dtype=np.int64)
        zero = np.zeros(out_cols, dtype=bool)
        for i, wr in zip(range(rfirst[r], rfirst[r] + len(rweights[r])), rweights[r]):
            row = x[i].astype(np.int64)
            for t in range(cidx.shape[1]):
                w = wr * cwgt[:, t]
                v = row[cidx[:, t]]
                S += w * v
                zero |= (w > 0) & (v == 0)
        res = (2 * S + total) // (2 * total)
        if zero_invalid:
            res[zero] = 0
        out[r] = res.astype(np.uint8)
    return out


def resize_f32_scalar(x, out_rows, out_cols, nan_policy='propagate'):
    """The header's text one pixel at a time (Python floats are IEEE float64)."""
    x = np.asarray(x)
    rows, cols = x.shape
    if (out_rows, out_cols) == (rows, cols):
        return x.copy()
    ar, _, rfirst, rweights = axis_weights(rows, out_rows)
    ac, _, cfirst, cweights = axis_weights(cols, out_cols)
    out = np.empty((out_rows, out_cols), dtype=np.float32)
    with np.errstate(all='ignore'):
        for r in range(out_rows):
            for c in range(out_cols):
                acc, used = 0.0, 0
                for di, wr in enumerate(rweights[r]):
                    for dk, wc in enumerate(cweights[c]):
                        v = float(x[rfirst[r] + di, cfirst[c] + dk])
                        if nan_policy == 'omit' and v != v:
                            continue
                        acc = acc + float(wr * wc) * v
                        used += wr * wc
                if nan_policy == 'omit':
                    out[r, c] = np.float32(np.float64(acc) / np.float64(used)) if used else np.float32(np.nan)
                else:
                    out[r, c] = np.float32(np.float64(acc) / np.float64(ar * ac))
    return out


def resize_u8_scalar(x, out_rows, out_cols, zero_invalid=True):
    x = np.asarray(x)
    rows, cols = x.shape
    if (out_rows, out_cols) == (rows, cols):
        return x.copy()
    ar, _, rfirst, rweights = axis_weights(rows, out_rows)
    ac, _, cfirst, cweights = axis_weights(cols, out_cols)
    total = ar * ac
    out = np.empty((out_rows, out_cols), dtype=np.uint8)
    for r in range(out_rows):
        for c in range(out_cols):
            S, zero = 0, False
            for di, wr in enumerate(rweights[r]):
                for dk, wc in enumerate(cweights[c]):
                    v = int(x[rfirst[r] + di, cfirst[c] + dk])
                    S += wr * wc * v
                    zero = zero or v == 0
            out[r, c] = 0 if (zero_invalid and zero) else (2 * S + total) // (2 * total)
    return out


def same_bits(a, b):
    """Equal shape, dtype and bytes; every NaN counts as the same value (the payload and sign of a NaN that arithmetic
    produced is the processor's choice, not the specification's)."""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype.kind != 'f':
        return a.tobytes() == b.tobytes()
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb)) and np.where(na, 0, a).tobytes() == np.where(nb, 0, b).tobytes()
