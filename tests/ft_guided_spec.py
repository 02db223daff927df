"""Specification of the guided matcher (include/sid_ftg.h) in NumPy: no device, no product code.

Train descriptor j is a candidate of query i iff ``dx * dx + dy * dy <= radius * radius`` with ``dx = tx[j] - qx[i]`` and
``dy = ty[j] - qy[i]``, every operation one IEEE float64 rounding (NumPy's element-wise arithmetic: no fused multiply-add).
A query whose position is not finite has no candidates; a train point whose position is not finite is nobody's candidate.
``idx``, ``dist`` [n1, 2] int32: the two candidates of smallest Hamming distance, nearest first, equal distances by the smaller
train index, -1 where there is none; ``count`` [n1] int32: the number of candidates."""
import numpy as np

MAX_TRAIN = 1 << 22                     # index bits of the ordering key


def check_radius(radius):
    r = float(radius)
    if not (np.isfinite(r) and r >= 0.0):
        raise ValueError('radius must be finite and >= 0')
    return np.float64(r)


def candidates(qx, qy, tx, ty, radius):
    """[n1, n2] bool: the inclusion rule."""
    r = check_radius(radius)
    qx, qy, tx, ty = (np.asarray(a, dtype=np.float64).reshape(-1) for a in (qx, qy, tx, ty))
    with np.errstate(all='ignore'):
        dx = tx[None, :] - qx[:, None]
        dy = ty[None, :] - qy[:, None]
        inside = dx * dx + dy * dy <= r * r
    inside &= (np.isfinite(qx) & np.isfinite(qy))[:, None]
    inside &= (np.isfinite(tx) & np.isfinite(ty))[None, :]
    return inside


def knn2(desc1, qx, qy, desc2, tx, ty, radius, chunk=256):
    d1 = np.ascontiguousarray(desc1, dtype=np.uint8).reshape(-1, 32)
    d2 = np.ascontiguousarray(desc2, dtype=np.uint8).reshape(-1, 32)
    n1, n2 = len(d1), len(d2)
    if n2 >= MAX_TRAIN:
        raise ValueError('at most 2^22 - 1 train descriptors')
    qx, qy, tx, ty = (np.asarray(a, dtype=np.float64).reshape(-1) for a in (qx, qy, tx, ty))
    if len(qx) != n1 or len(qy) != n1 or len(tx) != n2 or len(ty) != n2:
        raise ValueError('one position per descriptor')
    check_radius(radius)
    idx = np.full((n1, 2), -1, dtype=np.int32)
    dist = np.full((n1, 2), -1, dtype=np.int32)
    count = np.zeros(n1, dtype=np.int32)
    if n2 == 0 or n1 == 0:
        return idx, dist, count
    w2 = d2.view(np.uint64).reshape(n2, 4)
    none = np.int64(1) << 62
    for a in range(0, n1, chunk):
        w1 = d1[a:a + chunk].view(np.uint64).reshape(-1, 4)
        inside = candidates(qx[a:a + chunk], qy[a:a + chunk], tx, ty, radius)
        dm = np.bitwise_count(w1[:, None, :] ^ w2[None, :, :]).sum(axis=2).astype(np.int64)
        key = np.where(inside, dm * (1 << 32) + np.arange(n2, dtype=np.int64)[None, :], none)      # distance, then index
        kk = min(2, n2)
        part = np.sort(np.partition(key, kk - 1, axis=1)[:, :kk], axis=1)
        have = part != none
        idx[a:a + chunk, :kk] = np.where(have, part & 0xffffffff, -1).astype(np.int32)
        dist[a:a + chunk, :kk] = np.where(have, part >> 32, -1).astype(np.int32)
        count[a:a + chunk] = inside.sum(axis=1)
    return idx, dist, count


def lowe_keep(dist, count, ratio, accept_lone=False):
    """Which queries ftlib.match keeps under ``search_radius``: Lowe's test where there is a runner-up; a query with one
    candidate only with ``accept_lone``; a query with none never."""
    d = np.asarray(dist, dtype=np.float64)
    keep = (count >= 2) & (d[:, 0] < float(ratio) * d[:, 1])
    if accept_lone:
        keep |= count == 1
    return keep
