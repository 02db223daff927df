#!/usr/bin/env python3
"""Generate tests/golden/g11_prepare.npz from the REFERENCE's own lib.py: hh_angular_correction, get_spatial_mean and
get_uint8_image called in get_n's order (lib.py:318-331) on seeded synthetic sigma0 scenes.

Runs only where the reference tree is present (it is imported through the stubs of oracle/ref_harness.py).  The fixture holds
numbers only: the outputs the reference's functions returned, the six lstsq coefficients of every detrended chain, and for
every case the sha256 of the inputs that the seeded generators below rebuild (the GPU box has no reference; its tests
import this module for the inputs alone).

Cases (names are the fixture's key prefixes; STEPS says which of HH correction / mask / detrend a case's chain runs):
  small  101 x 151   odd width (no 16-byte rows), 3 x 4 samples for the six unknowns.  Float outputs in full: the HH-corrected
                     image, the float64 spatial mean and the detrended image of the dB=False chain; the uint8 output of the
                     dB=False chain for all eight combinations of HH / mask / detrend; the full dB=True chain
  big    240 x 320   every row 16-byte aligned: HH + mask + detrend
  odd    203 x 301   odd width: detrend alone
  view   200 x 320   a strided view (rows 5:205, columns 16:336) of a 260 x 352 parent: HH + mask
  tiny    37 x 41    smaller than one 50-pixel step: dB alone
Every scene: sigma0 over several decades with a brightness trend across range, zeros, negatives, NaN, +inf and a zeroed
border; the incidence angle is a ramp across range; the mask a few rectangles plus scattered pixels.  The dB=False chains
read the scene in dB (get_n's denoise=True route), the dB=True chains the linear scene.

Keys per case C: C_in_sha; C_db0_u8 (full) or C_db0_u8_<k> (small: k = bit 0 HH, bit 1 mask, bit 2 detrend);
C_db0_coeffs / C_db1_coeffs (detrended chains); C_hh, C_mean, C_detr in full (small) and C_hh_sha, C_mean_sha, C_detr_sha
(every case that has the step; NaNs are canonicalised before hashing: `digest`); and for dB=True
  C_db1_u8_cr     the chain with the correctly rounded float32 logarithm - float64 log10 rounded once - in place of np.log10
                  in the three glue lines below (what the device computes: DESIGN.md section 16)
  C_db1_u8_numpy_idx / _val   where, and to what, NumPy's own float32 log10 on the generating machine changes that image
  C_flip_share, C_max_diff    the share of pixels that differ between the two, and their largest difference in counts
flip_share_all: the same share over all dB=True cases together.

    python tests/golden/make_golden_prepare.py
"""
import contextlib
import hashlib
import io
import os
import sys
import warnings
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

PATH = os.path.join(HERE, 'g11_prepare.npz')
HH_FACTOR = -0.27                                   # get_n's default correct_hh_factor
PMIN, PMAX = 10, 99                                 # get_n's defaults
HH, MASK, DETREND = 1, 2, 4
CASES = ('small', 'big', 'odd', 'view', 'tiny')
SHAPES = {'small': (101, 151), 'big': (240, 320), 'odd': (203, 301), 'view': (260, 352), 'tiny': (37, 41)}
SEEDS = {'small': 1101, 'big': 1102, 'odd': 1103, 'view': 1104, 'tiny': 1105}
STEPS = {'small': HH | MASK | DETREND, 'big': HH | MASK | DETREND, 'odd': DETREND, 'view': HH | MASK, 'tiny': 0}
VIEW = (slice(5, 205), slice(16, 336))


def sha256(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        a = np.ascontiguousarray(a)
        h.update(str(a.dtype).encode() + str(a.shape).encode())
        h.update(a.tobytes())
    return h.hexdigest()


def digest(a):
    """sha256 of a float array with every NaN replaced by the one canonical NaN (sign and payload of a NaN are not part of
    the specification: NumPy's own differ between an assigned np.nan and one an operation produced)."""
    a = np.array(a, copy=True)
    a[np.isnan(a)] = np.nan
    return sha256(a)


def same_bits(got, exp):
    """Equal dtype and shape, NaN in the same places, identical bit patterns everywhere else."""
    got, exp = np.asarray(got), np.asarray(exp)
    if got.dtype != exp.dtype or got.shape != exp.shape:
        return False
    gn, en = np.isnan(got), np.isnan(exp)
    bits = {4: np.int32, 8: np.int64}[got.dtype.itemsize]
    return bool(np.array_equal(gn, en) and np.array_equal(got[~gn].view(bits), exp[~en].view(bits)))


def inputs(name):
    """(linear sigma0 float32, the same scene in dB float32, incidence angle float32, mask bool) of case `name`;
    'view' returns strided views of its parent arrays."""
    rows, cols = SHAPES[name]
    rng = np.random.default_rng(SEEDS[name])
    r, c = np.meshgrid(np.arange(rows, dtype=np.float64), np.arange(cols, dtype=np.float64), indexing='ij')
    # dB: ice texture around -22 dB, 9 dB darker at far range, a gentle bend along azimuth, a bright lead
    db = -18.0 - 9.0 * c / cols + 2.0 * (r / rows) ** 2 + 4.0 * rng.standard_normal((rows, cols))
    db[rows // 3: rows // 3 + 4, :] += 12.0
    lin = (10.0 ** (db / 10.0) * 10.0 ** rng.uniform(-2.0, 1.0, (rows, cols))).astype(np.float32)   # several decades
    db = db.astype(np.float32)
    for a in (lin, db):
        u = rng.random((rows, cols))
        a[u < 0.005] = np.nan
        a[(u >= 0.005) & (u < 0.0055)] = np.inf
    u = rng.random((rows, cols))
    lin[u < 0.005] = 0.0
    lin[(u >= 0.005) & (u < 0.01)] = -lin[(u >= 0.005) & (u < 0.01)]
    db[(u >= 0.005) & (u < 0.0055)] = -np.inf
    b = 3
    for a, fill in ((lin, 0.0), (db, np.nan)):                                   # the zeroed border of a SAR product
        a[:b, :] = fill; a[-b:, :] = fill; a[:, :b] = fill; a[:, -b:] = fill
    ia = (20.0 + 26.0 * c / cols + 0.3 * r / rows).astype(np.float32)
    mask = rng.random((rows, cols)) < 0.01
    mask[rows // 2: rows // 2 + rows // 6, cols // 5: cols // 5 + cols // 4] = True
    mask[: rows // 8, -cols // 6:] = True
    if name == 'view':
        return tuple(a[VIEW] for a in (lin, db, ia, mask))
    return lin, db, ia, mask


class Scene(object):
    """What hh_angular_correction asks of a Nansat object: has_band and the incidence-angle band."""
    def __init__(self, ia):
        self.ia = ia

    def has_band(self, name):
        return name == 'incidence_angle' and self.ia is not None

    def __getitem__(self, name):
        if name != 'incidence_angle':
            raise KeyError(name)
        return self.ia


def log10_cr(a):
    """The correctly rounded float32 logarithm: float64 log10 rounded once."""
    return np.log10(a.astype(np.float64)).astype(np.float32)


@contextlib.contextmanager
def recorded_lstsq(box):
    """np.linalg.lstsq with its solutions appended to `box` (get_spatial_mean does not return its coefficients)."""
    real = np.linalg.lstsq

    def spy(*a, **k):
        res = real(*a, **k)
        box.append(np.array(res[0], dtype=np.float64))
        return res
    np.linalg.lstsq = spy
    try:
        yield
    finally:
        np.linalg.lstsq = real


def chain(ref, img, dB, log10, ia, mask, detrend):
    """Lines 318-331 of get_n on arrays: the reference's functions, glued by get_n's own three array statements (dB,
    mask, the in-place subtraction).  -> dict(u8, and where the step ran: hh, mean, coeffs, detr)."""
    out = {}
    img = np.array(img, dtype=np.float32, copy=True)
    with np.errstate(all='ignore'), warnings.catch_warnings(), contextlib.redirect_stdout(io.StringIO()):
        warnings.simplefilter('ignore')
        if dB:
            img[img <= 0] = np.nan
            img = 10 * log10(img)
        if ia is not None:
            img = ref.hh_angular_correction(Scene(ia), img, 'sigma0_HH', HH_FACTOR)
            out['hh'] = img.copy()
        if mask is not None:
            img[mask] = np.nan
        if detrend:
            box = []
            with recorded_lstsq(box):
                mean = ref.get_spatial_mean(img)
            out['mean'], out['coeffs'] = mean, box[-1]
            img -= mean
            out['detr'] = img.copy()
        out['u8'] = ref.get_uint8_image(img, None, None, PMIN, PMAX)
    return out


def run(ref, name, dB, log10, steps):
    lin, db, ia, mask = inputs(name)
    return chain(ref, lin if dB else db, dB, log10, ia if steps & HH else None, mask if steps & MASK else None,
                 bool(steps & DETREND))


def reference_lib():
    from oracle import ref_harness
    return ref_harness.load()[1]


def compute(ref):
    """Every fixture array, from the reference module `ref`."""
    out = {}
    differ = total = 0
    for name in CASES:
        out[name + '_in_sha'] = np.array(sha256(*inputs(name)))
        steps = STEPS[name]
        res = run(ref, name, False, None, steps)
        for key in ('hh', 'mean', 'detr'):
            if key in res:
                out['%s_%s_sha' % (name, key)] = np.array(digest(res[key]))
                if name == 'small':
                    out['%s_%s' % (name, key)] = res[key]
        if 'coeffs' in res:
            out[name + '_db0_coeffs'] = res['coeffs']
        if name == 'small':
            for k in range(8):
                one = run(ref, name, False, None, k)
                out['%s_db0_u8_%d' % (name, k)] = one['u8']
                if k & DETREND:
                    out['%s_db0_coeffs_%d' % (name, k)] = one['coeffs']
        else:
            out[name + '_db0_u8'] = res['u8']
        cr = run(ref, name, True, log10_cr, steps)
        npy = run(ref, name, True, np.log10, steps)
        if 'coeffs' in cr:
            out[name + '_db1_coeffs'] = cr['coeffs']
        idx = np.flatnonzero(cr['u8'] != npy['u8'])
        out[name + '_db1_u8_cr'] = cr['u8']
        out[name + '_db1_u8_numpy_idx'] = idx.astype(np.int32)
        out[name + '_db1_u8_numpy_val'] = npy['u8'].ravel()[idx]
        out[name + '_flip_share'] = np.float64(len(idx) / cr['u8'].size)
        out[name + '_max_diff'] = np.int64(np.abs(cr['u8'].astype(np.int64) - npy['u8'].astype(np.int64)).max())
        differ += len(idx)
        total += cr['u8'].size
    out['flip_share_all'] = np.float64(differ / total)
    return {k: np.asarray(v) for k, v in out.items()}


def write_npz(path, arrays):
    """A compressed .npz whose bytes depend on the arrays alone (np.savez stamps every member with the time of day)."""
    with zipfile.ZipFile(path, 'w', zipfile.ZIP_DEFLATED) as zf:
        for key in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asarray(arrays[key]), allow_pickle=False)
            info = zipfile.ZipInfo(key + '.npy', date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            zf.writestr(info, buf.getvalue())


def main():
    out = compute(reference_lib())
    write_npz(PATH, out)
    print('wrote %s (%d bytes, %d arrays); flip_share_all = %.3g; per case: %s' % (
        PATH, os.path.getsize(PATH), len(out), float(out['flip_share_all']),
        ', '.join('%s %.3g (max %d)' % (n, float(out[n + '_flip_share']), int(out[n + '_max_diff'])) for n in CASES)))


if __name__ == '__main__':
    main()
