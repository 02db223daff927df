#!/usr/bin/env python3
"""Generate tests/golden/g12_invalid_mask.npz from the REFERENCE's own lib.get_invalid_mask (lib.py:342-373), called with a
stand-in scene object on seeded inputs, and hold the written specification of what it computes: `landmask_numpy`.

Runs only where the reference tree is present (it is imported through the stubs of oracle/ref_harness.py).  The fixture holds
numbers only: the masks the reference returned (np.packbits), the zoomed water mask of the smallest case, and for every case
the sha256 of the inputs that the seeded generators below rebuild (the GPU box has no reference; its tests import this
module for the inputs and for the restatement).

Cases (water mask -> image; names are the fixture's key prefixes):
  odd      (25,31)->(487,613)   odd width, non-integer ratio
  even     (24,30)->(480,600)   every row 16-byte aligned
  narrow3  (3,3)->(61,67)       a grid narrower than the four taps: mirrored on both sides
  narrow2  (2,5)->(40,100)      likewise
  lastrow  (4,9)->(188,181)     187 * (3 / 187) rounds one ulp above 3: the last ROW lies outside and is 0
  lastcol  (9,4)->(181,188)     the last COLUMN
  down     (40,50)->(23,31)     a downscale
  same     (12,12)->(12,12)
  nowm     the image of `odd` with a scene whose watermask() raises: no land
Water masks: about 20 % twos, 10 % ones, a few values above 2 (clipped); images: float32 with NaN, +inf and -inf.
The scenes 'small' and 'view' of g11 (make_golden_prepare) get a water mask each, and the reference's mask of their image after
dB / HH for the four combinations of the two (keys prep_<scene>_<k>, k = bit 0 dB, bit 1 HH).

Keys per case C: C_in_sha, C_mask (packbits of the reference's bool mask), C_calls (resize count, undo count, 1 / the factor
resize was given); the smallest case alone stores its zoomed water mask (narrow3_wmz).

    python tests/golden/make_golden_landmask.py
"""
import contextlib
import io
import math
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests.golden import make_golden_prepare as mgp   # noqa: E402

PATH = os.path.join(HERE, 'g12_invalid_mask.npz')
LANDMASK_BORDER = 20                                 # get_n's default
SHAPES = {'odd': ((25, 31), (487, 613)), 'even': ((24, 30), (480, 600)), 'narrow3': ((3, 3), (61, 67)),
          'narrow2': ((2, 5), (40, 100)), 'lastrow': ((4, 9), (188, 181)), 'lastcol': ((9, 4), (181, 188)),
          'down': ((40, 50), (23, 31)), 'same': ((12, 12), (12, 12))}
CASES = tuple(SHAPES)
SEEDS = {'odd': 42, 'even': 25, 'narrow3': 1203, 'narrow2': 1204, 'lastrow': 1205, 'lastcol': 1206, 'down': 1207, 'same': 1208}
WMZ_CASE = 'narrow3'
PREP_SCENES = {'small': ((6, 8), 1221), 'view': ((10, 16), 1222)}       # g11 scene -> (water-mask shape, seed)

sha256 = mgp.sha256
write_npz = mgp.write_npz


# ---------------------------------------------------------------- seeded inputs
def watermask(shape, seed):
    """uint8 raster: about 20 % twos, 10 % ones, 2 % values above 2."""
    rng = np.random.default_rng(seed)
    u = rng.random(shape)
    wm = np.zeros(shape, dtype=np.uint8)
    wm[u < 0.20] = 2
    wm[(u >= 0.20) & (u < 0.30)] = 1
    big = u >= 0.98
    wm[big] = rng.integers(3, 256, shape, dtype=np.int64).astype(np.uint8)[big]
    return wm


def image(shape, seed):
    """float32 scene in dB with NaN, +inf and -inf pixels."""
    rng = np.random.default_rng(seed + 7000)
    img = rng.normal(-20.0, 4.0, shape).astype(np.float32)
    u = rng.random(shape)
    img[u < 0.01] = np.nan
    img[(u >= 0.01) & (u < 0.015)] = np.inf
    img[(u >= 0.015) & (u < 0.02)] = -np.inf
    return img


def inputs(name):
    """(image float32, water mask uint8) of case `name`."""
    wshape, ishape = SHAPES[name]
    return image(ishape, SEEDS[name]), watermask(wshape, SEEDS[name])


def prep_inputs(scene, k):
    """(the g11 scene's input image, dB flag, incidence angle or None, its image after dB / HH, water mask) for combination k."""
    lin, db, ia, _ = mgp.inputs(scene)
    dB, hh = bool(k & 1), bool(k & 2)
    src = lin if dB else db
    with np.errstate(all='ignore'):
        img = np.array(src, dtype=np.float32, copy=True)
        if dB:
            img[img <= 0] = np.nan
            img = 10 * mgp.log10_cr(img)
        if hh:
            img = img - ia * mgp.HH_FACTOR
    wshape, seed = PREP_SCENES[scene]
    return src, dB, (ia if hh else None), img, watermask(wshape, seed)


# ---------------------------------------------------------------- the specification
def spline_mirror(idx, n):
    """SciPy's mirror mapping of tap indices (ni_interpolation.c, NI_EXTEND_MIRROR) for an int64 array."""
    idx = np.array(idx, dtype=np.int64, copy=True)
    if n <= 1:
        return np.zeros_like(idx)
    s2 = 2 * n - 2
    neg = idx < 0
    v = s2 * ((-idx[neg]) // s2) + idx[neg]
    idx[neg] = np.where(v <= 1 - n, v + s2, -v)
    big = idx >= n
    v = idx[big] - s2 * (idx[big] // s2)
    idx[big] = np.where(v >= n, s2 - v, v)
    return idx


def spline_prefilter(a):
    """Cubic B-spline coefficients of a 2-D array: scipy.ndimage.spline_filter(a, 3, output=float64, mode='mirror'), axis 0 then
    axis 1, SciPy's operations in SciPy's order (ni_splines.c apply_filter); an axis of length 1 is left alone."""
    z = -0.267949192431122706472553658494             # sqrt(3) - 2
    gain = (1.0 - z) * (1.0 - 1.0 / z)
    c = np.array(a, dtype=np.float64, copy=True)
    for axis in (0, 1):
        n = c.shape[axis]
        if n <= 1:
            continue
        c = np.moveaxis(c, axis, 0)                   # (a view: lines run along axis 0, all lines at once)
        c *= gain
        z_n_1 = math.pow(z, n - 1)
        z_i = z
        c[0] = c[0] + z_n_1 * c[n - 1]
        for i in range(1, n - 1):
            c[0] += z_i * (c[i] + z_n_1 * c[n - 1 - i])
            z_i *= z
        c[0] /= 1 - z_n_1 * z_n_1
        for i in range(1, n):
            c[i] += z * c[i - 1]
        c[n - 1] = (z * c[n - 2] + c[n - 1]) * z / (z * z - 1)
        for i in range(n - 2, -1, -1):
            c[i] = z * (c[i + 1] - c[i])
        c = np.moveaxis(c, 0, axis)
    return c


def zoom_axis(n_in, n_out):
    """Per output index of an axis: (outside flag, four mirrored tap indices, four weights)."""
    z = np.float64(n_in - 1) / np.float64(n_out - 1) if n_out > 1 else np.float64(1.0)
    cc = np.arange(n_out, dtype=np.float64) * z       # one multiplication per index, no running sum
    outside = (cc < 0) | (cc > n_in - 1)              # no tolerance
    fl = np.floor(cc)
    taps = spline_mirror((fl.astype(np.int64) - 1)[:, None] + np.arange(4), n_in)
    x = cc - fl
    y, zz = x, 1.0 - x
    w = np.empty((n_out, 4))
    w[:, 1] = (y * y * (y - 2.0) * 3.0 + 4.0) / 6.0
    w[:, 2] = (zz * zz * (zz - 2.0) * 3.0 + 4.0) / 6.0
    w[:, 0] = zz * zz * zz / 6.0
    w[:, 3] = ((1.0 - w[:, 0]) - w[:, 1]) - w[:, 2]
    return outside, taps, w


def landmask_numpy(wm, shape):
    """The uint8 image scipy.ndimage.zoom(maximum_filter(np.minimum(wm, 2), 3), np.array(shape) / wm.shape) returns - steps 1-6
    of DESIGN.md section 17 - in NumPy.  Raises IndexError when SciPy's zoom would give another shape than `shape` (step 8)."""
    wm = np.asarray(wm)
    assert wm.dtype == np.uint8 and wm.ndim == 2
    h, w = wm.shape
    H, W = (int(v) for v in shape)
    if (int(round(h * (H / h))), int(round(w * (W / w)))) != (H, W):
        raise IndexError('zoomed shape differs from the image')
    p = np.pad(np.minimum(wm, 2), 1, mode='edge')     # 1: clip, 3 x 3 maximum with clamped indices
    wmf = np.max([p[i:i + h, j:j + w] for i in range(3) for j in range(3)], axis=0)
    coef = spline_prefilter(wmf)                      # 2
    out0, ia, w0 = zoom_axis(h, H)                    # 3
    out1, ib, w1 = zoom_axis(w, W)
    t = np.zeros((H, W))                              # 4: axis 0 outer, axis 1 inner; every product and sum rounded
    for a in range(4):
        for b in range(4):
            t = t + (coef[ia[:, a]][:, ib[:, b]] * w0[:, a, None]) * w1[None, :, b]
    t = np.where(t > 0, t + 0.5, 0.0)                 # 5
    t = np.minimum(t, 255.0)
    t[out0, :] = 0.0
    t[:, out1] = 0.0
    return t.astype(np.int64).astype(np.uint8)


def invalid_numpy(img, wm):
    """Steps 1-7: the reference's get_invalid_mask for an image and the raster its scene returns (None: no land)."""
    mask = np.isnan(img) | np.isinf(img)
    if wm is not None:
        mask = mask | (landmask_numpy(wm, img.shape) == 2)
    return mask


# ---------------------------------------------------------------- the reference
class Scene(object):
    """What get_invalid_mask asks of a Nansat object: resize, watermask, undo; counts the calls."""
    def __init__(self, wm):
        self.wm = wm
        self.resized, self.undone, self.factor = 0, 0, None

    def resize(self, factor):
        self.resized += 1
        self.factor = factor

    def watermask(self):
        if self.wm is None:
            raise RuntimeError('no MOD44W here')
        return None, self.wm.copy()

    def undo(self):
        self.undone += 1


def reference_lib():
    from oracle import ref_harness
    return ref_harness.load()[1]


def reference_mask(ref, img, wm):
    scene = Scene(wm)
    with contextlib.redirect_stdout(io.StringIO()) as said:
        mask = ref.get_invalid_mask(img.copy(), scene, LANDMASK_BORDER)
    assert (wm is None) == ('Cannot add landmask' in said.getvalue())
    return np.asarray(mask, dtype=bool), np.array([scene.resized, scene.undone, 1.0 / scene.factor])


def compute(ref):
    """Every fixture array, from the reference module `ref`."""
    from scipy.ndimage import maximum_filter, zoom
    out = {}
    for name in CASES:
        img, wm = inputs(name)
        out[name + '_in_sha'] = np.array(sha256(img, wm))
        mask, calls = reference_mask(ref, img, wm)
        out[name + '_mask'] = np.packbits(mask)
        out[name + '_calls'] = calls
    img, _ = inputs('odd')
    mask, calls = reference_mask(ref, img, None)
    out['nowm_mask'], out['nowm_calls'] = np.packbits(mask), calls
    wm = inputs(WMZ_CASE)[1]
    out[WMZ_CASE + '_wmz'] = zoom(maximum_filter(np.minimum(wm, 2), 3), np.array(SHAPES[WMZ_CASE][1]) / np.array(wm.shape))
    for scene in PREP_SCENES:
        for k in range(4):
            _, _, _, img, wm = prep_inputs(scene, k)
            out['prep_%s_%d' % (scene, k)] = np.packbits(reference_mask(ref, img, wm)[0])
            out['prep_%s_%d_in_sha' % (scene, k)] = np.array(sha256(img, wm))
    return {k: np.asarray(v) for k, v in out.items()}


def unpack(g, key, shape):
    """The bool mask stored under `key`."""
    return np.unpackbits(g[key])[:shape[0] * shape[1]].reshape(shape).astype(bool)


def main():
    out = compute(reference_lib())
    write_npz(PATH, out)
    print('wrote %s (%d bytes, %d arrays)' % (PATH, os.path.getsize(PATH), len(out)))


if __name__ == '__main__':
    main()
