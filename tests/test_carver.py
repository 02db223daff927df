"""Host-side invariants of the staging layouts (csrc/carve.h): the header is plain C++, so that measuring and carving agree,
that regions are aligned, disjoint and in order, and that absent regions take no room is checked without a GPU (g++ only)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_carver_invariants(tmp_path):
    exe = str(tmp_path / 'carver_check')
    subprocess.check_call(['g++', '-std=c++17', '-O1', '-o', exe, os.path.join(ROOT, 'tests', 'cpp', 'carver_check.cpp')])
    p = subprocess.run([exe], stdout=subprocess.PIPE, universal_newlines=True)
    assert p.returncode == 0 and p.stdout.strip().endswith(' 0 violations'), p.stdout[-3000:]
