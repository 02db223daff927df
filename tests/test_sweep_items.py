"""Host-side invariants of the sweep's work items (csrc/pm_kernel.h rp_sweep_items / rp_sweep_single_lane): the ragged single
items that pack the leftover columns of all bands cover every placement exactly as often as today's tiling does, with the
key of the placement they read, inside the LDS regions of rp_lds_layout, in no more units (g++ only)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build(tmp_path):
    exe = str(tmp_path / 'sweep_items_check')
    subprocess.check_call(['g++', '-std=c++17', '-O1', '-o', exe, os.path.join(ROOT, 'tests', 'cpp', 'sweep_items_check.cpp')])
    return exe


def test_sweep_items_invariants(tmp_path):
    p = subprocess.run([_build(tmp_path)], stdout=subprocess.PIPE, universal_newlines=True)
    assert p.returncode == 0 and p.stdout.strip().endswith('0 violations'), p.stdout[-3000:]


def test_sweep_items_units_of_the_benchmark_grid(tmp_path):
    """The chosen tiling never has more units than today's, per border and for the busiest wavefront of the benchmark's
    launch classes; in the benchmark's largest class (borders 20 .. 23) it removes a tenth of the sweep's units."""
    import numpy as np
    from sea_ice_drift_amd import synthetic as syn
    p = subprocess.run([_build(tmp_path), 'units'], stdout=subprocess.PIPE, universal_newlines=True, check=True)
    tab = {}
    for line in p.stdout.split('\n'):
        if line.strip():
            v = [int(x) for x in line.split()]
            tab[(v[0], v[1])] = v[2:]
    for (band, b), v in tab.items():
        assert v[2] <= v[1], (band, b, v)
    border = syn.make_grid(10000, 10000, 200, 'mixed')['border'].astype(int)
    assert border.size == 40000

    def units(sel, col):
        # 8-row items count double; borders 37 .. 47 run 8-row bands
        return sum((2 if 37 <= b <= 47 else 1) * tab[(8 if 37 <= b <= 47 else 4, b)][col] for b in border[sel])
    everything = np.ones(border.size, dtype=bool)
    today, new = units(everything, 1), units(everything, 2)
    print('units of the benchmark grid: today %d, chosen %d (x %.3f)' % (today, new, new / today))
    assert new < today
    # the class of borders 20 .. 23 (68 % of the points; rem = 10 .. 16): x 0.893 by the arithmetic of the item lists
    low = border <= 23
    assert abs(units(low, 2) / units(low, 1) - 0.893) < 0.001
