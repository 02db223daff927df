"""Host-side check of the guided matcher's plan, g++ only: tests/cpp/ft_guided_plan_check.cpp sweeps csrc/ft_guided_plan.h -
radii from 0 to the largest double, extents from 0 to overflowing, negative and huge offsets, degenerate boxes: the cell count
stays within the cap, every point gets a cell inside the grid, pairs within the radius (a few ulps either side of cell
boundaries and exactly one radius apart included) lie in adjacent cells, and the regions of the workspace are aligned,
disjoint and within sid_ftg_workspace_bytes."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_ft_guided_plan_cells_adjacency_and_regions(tmp_path):
    exe = str(tmp_path / 'ft_guided_plan_check')
    subprocess.check_call(['g++', '-std=c++17', '-O1', '-ffp-contract=off', '-o', exe,
                           os.path.join(ROOT, 'tests', 'cpp', 'ft_guided_plan_check.cpp')])
    p = subprocess.run([exe], stdout=subprocess.PIPE, universal_newlines=True)
    print(p.stdout[-3000:])
    assert p.returncode == 0 and p.stdout.strip().split('\n')[-1] == '0 violations', p.stdout[-3000:]
