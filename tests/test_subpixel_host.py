"""Sub-pixel peak (include/sid_pm.h SID_PM_SUBPIXEL, ``subpixel=True``) where no GPU is needed: the specification on hand-made
triples (tests/subpixel_spec.py is its only restatement), the same triples through the C++ function the kernels call
(csrc/pm_kernel.h is plain C++ on the host), the flag's way through ``flags_from_kwargs`` / ``_sweep_options``, and what the
offsets are worth on the C oracle's matrices of a pair shifted by a known fraction of a pixel."""
import itertools
import os
import struct
import subprocess

import numpy as np
import pytest
from scipy import ndimage

from sea_ice_drift_amd import _capi, pmlib, synthetic
from tests import subpixel_spec as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the specification on hand-made triples ----

def _parabola(b, k, x0):
    return [np.float32(b - k * (x - x0) ** 2) for x in (-1.0, 0.0, 1.0)]


DYADIC = [(b, k, x0) for b in (0.75, 0.5, 1.0) for k in (0.125, 0.25, 0.0625, 0.5) for x0 in (0.0, 0.25, -0.25, 0.375, -0.4375, 0.5, -0.5)]


def test_dyadic_parabolas_give_their_vertex_exactly():
    """b - k (x - x0)^2 at x = -1, 0, 1 with dyadic b, k, x0: the three samples are exact in float32, every step of the fit is
    exact in double, and the fit returns x0 itself."""
    for b, k, x0 in DYADIC:
        a_, b_, c_ = _parabola(b, k, x0)
        assert float(a_) == b - k * (-1 - x0) ** 2 and float(c_) == b - k * (1 - x0) ** 2      # the samples are exact
        got = sp.fit(a_, b_, c_)
        assert got == x0 and isinstance(got, np.float64), (b, k, x0, got)


def test_ties_and_symmetry():
    assert sp.fit(np.float32(0.25), np.float32(0.5), np.float32(0.5)) == 0.5                  # a < b == c: exactly +0.5
    assert sp.fit(np.float32(0.1), np.float32(0.7), np.float32(0.7)) == 0.5
    assert sp.fit(np.float32(0.3), np.float32(0.9), np.float32(0.3)) == 0.0                   # a == c
    assert sp.fit(np.float32(0.5), np.float32(0.5), np.float32(0.5)) == 0.0                   # den == 0: the guard
    rng = np.random.Generator(np.random.PCG64(3))
    for _ in range(2000):                                                                     # first-maximum triples: a < b, c <= b
        b = np.float32(rng.uniform(-1, 1))
        a = np.nextafter(b, np.float32(-2)) if rng.random() < 0.2 else np.float32(b - rng.uniform(1e-7, 1))
        c = b if rng.random() < 0.2 else np.float32(b - rng.uniform(0, 1))
        if not (a < b and c <= b):
            continue
        d = sp.fit(a, b, c)
        assert -0.5 <= d <= 0.5
        if c == b:
            assert d == 0.5                                          # exactly


def test_frame_peaks_give_zero_on_that_axis():
    R = np.float32(0.5) - np.float32(0.125) * ((np.arange(5, dtype=np.float32)[:, None] - np.float32(2.25)) ** 2 +
                                                   (np.arange(6, dtype=np.float32)[None, :] - np.float32(2.5)) ** 2)
    R = R.astype(np.float32)
    for iy, ix in itertools.product(range(5), range(6)):
        dx, dy = sp.offsets(R, iy, ix)
        assert (dx == 0.0) if ix in (0, 5) else (dx == sp.fit(R[iy, ix - 1], R[iy, ix], R[iy, ix + 1]))
        assert (dy == 0.0) if iy in (0, 4) else (dy == sp.fit(R[iy - 1, ix], R[iy, ix], R[iy + 1, ix]))
    dx, dy = sp.offsets(R, 2, 2)                                     # the peak of this matrix: vertex at (2.25, 2.5)
    assert (dx, dy) == (0.5, 0.25)
    for shape, (iy, ix) in (((2, 2), (0, 1)), ((2, 7), (1, 3)), ((7, 2), (3, 0))):
        M = np.zeros(shape, dtype=np.float32)
        M[iy, ix] = 1.0
        dx, dy = sp.offsets(M, iy, ix)
        assert dx == 0.0 and dy == 0.0                               # on the frame, or between equal neighbours


def test_the_kernels_function_is_the_specification(tmp_path):
    """subpixel_fit / subpixel_offsets of csrc/pm_kernel.h - what all three kernel families call - compiled for the host with
    the library's -ffp-contract=off, against the specification bit for bit on the dyadic triples, ties and 4000 random ones."""
    rng = np.random.Generator(np.random.PCG64(11))
    triples = [tuple(np.float32(v) for v in _parabola(*t)) for t in DYADIC]
    triples += [(np.float32(0.25), np.float32(0.5), np.float32(0.5)), (np.float32(0.5),) * 3, (np.float32(0.3), np.float32(0.9), np.float32(0.3))]
    for _ in range(4000):
        b = np.float32(rng.uniform(-1, 1))
        triples.append((np.float32(b - np.float32(rng.uniform(0, 0.3)) ** 2), b, np.float32(b - np.float32(rng.uniform(0, 0.3)) ** 2)))
    src = tmp_path / 'fit.cpp'
    src.write_text('#include <cstdio>\n#include <cstring>\n#include <cstdint>\n#define __host__\n#define __device__\n'
                   '#include "%s"\n'
                   'int main() { float t[3]; while (fread(t, 4, 3, stdin) == 3) { float R[9] = {0, t[0], 0, t[0], t[1], t[2], 0, t[2], 0};\n'
                   '  double v[3]; v[0] = sid::subpixel_fit(t[0], t[1], t[2]); sid::subpixel_offsets(R, 3, 3, 1, 1, v[1], v[2]);\n'
                   '  fwrite(v, 8, 3, stdout); } return 0; }\n' % os.path.join(ROOT, 'sea_ice_drift_amd', 'csrc', 'pm_kernel.h'))
    exe = tmp_path / 'fit'
    subprocess.check_call(['g++', '-std=c++17', '-O2', '-ffp-contract=off', '-o', str(exe), str(src)])
    blob = b''.join(struct.pack('<3f', *t) for t in triples)
    out = subprocess.run([str(exe)], input=blob, stdout=subprocess.PIPE, check=True).stdout
    got = np.frombuffer(out, dtype=np.float64).reshape(-1, 3)
    assert got.shape[0] == len(triples)
    want = np.array([[sp.fit(*t)] * 3 for t in triples], dtype=np.float64)
    assert sp.same_bits(got, want)


# ---- the flag ----

def test_flag_value():
    assert _capi.SUBPIXEL == 128 and _capi.ABI_VERSION == 6
    hdr = open(os.path.join(ROOT, 'include', 'sid_pm.h')).read()
    assert '#define SID_PM_SUBPIXEL 128u' in hdr and '#define SID_PM_ABI_VERSION 6' in hdr


def test_flags_from_kwargs_sets_bit_7_and_nothing_else():
    for hn, hs, mn, ro in itertools.product((True, False), (True, False), (True, False), range(6)):
        today = (1 if hn else 0) | (2 if hs else 0) | (4 if mn else 0) | (ro << 3)
        assert _capi.flags_from_kwargs(hes_norm=hn, hes_smth=hs, mcc_norm=mn, rot_order=ro) == today
        assert _capi.flags_from_kwargs(hn, hs, mn, ro) == today                              # the positional order stays
        assert _capi.flags_from_kwargs(hes_norm=hn, hes_smth=hs, mcc_norm=mn, rot_order=ro, subpixel=False) == today
        assert _capi.flags_from_kwargs(hes_norm=hn, hes_smth=hs, mcc_norm=mn, rot_order=ro, subpixel=True) == today | 128
        assert today & (64 | 128) == 0
    assert _capi.flags_from_kwargs() == 1 and _capi.flags_from_kwargs(subpixel=True) == 129


def test_sweep_options_reads_the_keyword():
    assert pmlib._sweep_options({}) == ([-3, 0, 3], 1)
    assert pmlib._sweep_options({'subpixel': False}) == ([-3, 0, 3], 1)
    assert pmlib._sweep_options({'subpixel': True}) == ([-3, 0, 3], 129)
    for kw in ({'hes_smth': True}, {'mcc_norm': True, 'hes_norm': False}, {'rot_order': 3, 'angles': [0]}, {'angles': range(-7, 8)}):
        a0, f0 = pmlib._sweep_options(dict(kw))
        a1, f1 = pmlib._sweep_options(dict(kw, subpixel=True))
        assert a0 == a1 and f1 == f0 | 128 and f0 & 128 == 0
    with pytest.raises(NotImplementedError):                         # what is refused stays refused
        pmlib._sweep_options({'mtype': 3, 'subpixel': True})


# ---- accuracy, on the oracle alone ----

SHIFTS = [(2.3, -1.4), (0.5, 0.25), (-0.2, 3.45)]                    # (rows, columns), as scipy.ndimage.shift takes them
CENTRES = [(c, r) for r in (60, 100, 140) for c in (60, 100, 140)] + [(80, 80), (120, 120), (80, 120)]


def _quantise(tex, m, s):
    return np.clip(np.rint(128.0 + 45.0 * (tex - m) / s), 1, 255).astype(np.uint8)


@pytest.fixture(scope='module')
def shifted_pairs():
    tex = synthetic._texture(200, 200, np.random.Generator(np.random.PCG64(7)))
    m, s = float(tex.mean(dtype=np.float64)), float(tex.std(dtype=np.float64))
    img1 = _quantise(tex, m, s)
    return img1, {sh: _quantise(ndimage.shift(tex, sh, order=3, mode='nearest'), m, s) for sh in SHIFTS}


@pytest.mark.parametrize('side,border', [(20, 6), (35, 5)])
def test_offsets_halve_the_error_on_a_shifted_pair(c_oracle, shifted_pairs, side, border):
    """Twelve points per shift, angle 0, first guess = the point itself.  Position of a point = oracle's c2, r2 (+ the
    specification's offsets on the oracle's matrix); error = position on the shifted pair - position on the unshifted pair
    (image 2 = image 1) - the shift.  RMS over points and axes, per shift: with the offsets at most half of without."""
    img1, shifted = shifted_pairs

    def positions(img2):
        pts = [sp.oracle_point(c_oracle, img1, img2, float(c), float(r), float(c), float(r), float(border), side, [0]) for c, r in CENTRES]
        assert not any(p['nan'] for p in pts)
        whole = np.array([[p['out'][0], p['out'][1]] for p in pts])
        return whole, whole + np.array([[p['dx'], p['dy']] for p in pts])

    zero_i, zero_s = positions(img1)
    assert len({tuple(v) for v in (zero_i - np.array(CENTRES, dtype=np.float64)).tolist()}) == 1    # the template convention's constant offset
    for sh in SHIFTS:
        got_i, got_s = positions(shifted[sh])
        truth = np.array([sh[1], sh[0]])                                                      # (columns, rows)
        rms_i = float(np.sqrt(np.mean((got_i - zero_i - truth) ** 2)))
        rms_s = float(np.sqrt(np.mean((got_s - zero_s - truth) ** 2)))
        print('side %d shift %r: RMS error %.4f px whole-pixel, %.4f px sub-pixel (%.2f x)' % (side, sh, rms_i, rms_s, rms_s / rms_i))
        assert rms_s <= 0.5 * rms_i, (side, sh, rms_i, rms_s)
