"""Host check of the shortened normalisation of the winner's NCC matrix (csrc/ncc_norm.h - the arithmetic the kernels compile),
g++ only: tests/cpp/ncc_norm_check.cpp compares it with the specification written out (1 / sqrt, two roundings, no fused
operation) under reciprocal-square-root seeds of three qualities - correctly rounded, rounded to float32, off by +-2^-20.
(a) 10^7 physical inputs per seed at sides 2, 34, 35, 64, 255: every unflagged value is the specification's bit for bit and at
most 20 are flagged (the guard band is 129 of 2^29 double mantissas: 2.4 expected); (b) constructed inputs - float32 rounding
midpoints +-100 ulps, q = +-1, both clamp thresholds and their 1e-13 neighbourhoods, beyond them, dI = 0, dI <= N / 2 with the
low-variance rule true and false, a constant template, 1 / sqrt(dT) = inf: the final value is the specification's and every
inf / NaN of the short route is flagged; (c) the fma forms of dI and the numerator equal the mul / sub forms on the largest
integers of side 255."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_ncc_norm_is_the_specification(tmp_path):
    exe = str(tmp_path / 'ncc_norm_check')
    subprocess.check_call(['g++', '-std=c++17', '-O2', '-ffp-contract=off', '-o', exe, os.path.join(ROOT, 'tests', 'cpp', 'ncc_norm_check.cpp')])
    p = subprocess.run([exe], stdout=subprocess.PIPE, universal_newlines=True)
    print(p.stdout[-3000:])
    assert p.returncode == 0 and p.stdout.strip().endswith('\n0 violations'), p.stdout[-3000:]
