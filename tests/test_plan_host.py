"""Host-side invariants of the PM launch planner (csrc/pm_plan.h plan_points), g++ only: tests/cpp/plan_check.cpp plans a
matrix of template sides (34, 35: row-pair kernel; 20: classic kernel; 70: large-window pipeline only) x angle counts (3, 7, 15,
16) x flags x switch sets (filled into Switches directly) over every border 2..112 and 120 on a 400 x 400 image 2, with NaN and
negative borders, clipped windows, windows starting outside the image, runs of 31..34 points of equal border, and 0 / 1 points.
It checks coverage, the tiling of the buckets, footprints and kernel instantiations, block offsets, the XCD interleave, and the
agreement with the cost model (estimate_points) for every point in a launch - no case excluded: points clipped by the edge of
image 2 or without a window are in no launch class the estimate describes and are checked for their list only."""
import os
import re
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build(tmp_path):
    exe = str(tmp_path / 'plan_check')
    subprocess.check_call(['g++', '-std=c++17', '-O1', '-o', exe, os.path.join(ROOT, 'tests', 'cpp', 'plan_check.cpp')])
    return exe


def test_plan_invariants(tmp_path):
    p = subprocess.run([_build(tmp_path)], stdout=subprocess.PIPE, universal_newlines=True)
    print(p.stdout[-3000:])
    assert p.returncode == 0 and p.stdout.strip().endswith(' 0 violations'), p.stdout[-3000:]


def test_instance_table_against_the_written_predicate(tmp_path):
    """What the planner is told about the kernels' instantiations comes from the table the library ships (csrc/pm_instances.h).
    The predicate that plan_check.cpp used to answer with is asserted against that table over the whole domain: band 4 / 8 x
    paired 0 / 1 / 2 x occ 3 / 4 x the six pitches the kernels carry and four they do not (120 checks); both template sides carry
    the same rows (240); the default register budget (1); mfma_img_size_supported, mfma_band8_supported and the classic kernel's
    side argument for sides -1 .. 70 (216); max_lds_bytes (1)."""
    p = subprocess.run([_build(tmp_path), 'instances'], stdout=subprocess.PIPE, universal_newlines=True)
    print(p.stdout[-3000:])
    m = re.search(r'(\d+) instance checks, (\d+) violations\s*$', p.stdout)
    assert p.returncode == 0 and m, p.stdout[-3000:]
    assert int(m.group(1)) == 120 + 240 + 2 + 216 and int(m.group(2)) == 0


def test_plan_of_the_benchmark_grid(tmp_path):
    """The launches of the benchmark grid (count, LDS bytes, band, window pitch, wavefronts per SIMD) are those the library
    printed under SID_PM_VERBOSE=1 on an MI355X before the planner was split off (tests/golden/plan_bench_launches.txt)."""
    from sea_ice_drift_amd import synthetic as syn
    g = syn.make_grid(10000, 10000, 200, 'mixed')
    pts = str(tmp_path / 'grid.txt')
    with open(pts, 'w') as f:
        f.write('%d\n' % g['border'].size)
        np.savetxt(f, np.stack([g[k] for k in ('c1', 'r1', 'c2fg', 'r2fg', 'border')], axis=1), fmt='%.1f')
    want, key = {}, None
    for line in open(os.path.join(ROOT, 'tests', 'golden', 'plan_bench_launches.txt')):
        m = re.match(r'== grid s=(\d+) K=(\d+)', line)
        if m:
            key = (int(m.group(1)), int(m.group(2)))
            want[key] = []
            continue
        m = re.match(r'sid_pm: launch of (\d+) points, (\d+) B of LDS \(\d+ per CU\), band (\d+), window pitch (\d+), (\d+) wavefronts per SIMD', line)
        assert m, line
        want[key].append(tuple(int(v) for v in m.groups()))
    assert sorted(want) == [(34, 15), (35, 3)]
    exe = _build(tmp_path)
    for (s, K), rows in want.items():
        out = subprocess.run([exe, 'grid', pts, str(s), str(K)], stdout=subprocess.PIPE, universal_newlines=True, check=True).stdout
        got = [tuple(int(v) for v in line.split()) for line in out.strip().split('\n')]
        print(s, K, got)
        assert got == rows, (s, K)
