"""Host-side check of the matcher's launch plan, g++ only: tests/cpp/ft_plan_check.cpp sweeps csrc/ft_plan.h - the chunks of
both forms tile the train set, the four regions of the MFMA form's workspace are aligned, disjoint and within
sid_ft_workspace_bytes, the switch between the forms at 2^24 pairs / 1024 train descriptors with and without SID_FT_NO_MFMA,
and the size limits of sid_ft_knn2_device."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_ft_plan_tiling_regions_switch_and_limits(tmp_path):
    exe = str(tmp_path / 'ft_plan_check')
    subprocess.check_call(['g++', '-std=c++17', '-O1', '-o', exe, os.path.join(ROOT, 'tests', 'cpp', 'ft_plan_check.cpp')])
    p = subprocess.run([exe], stdout=subprocess.PIPE, universal_newlines=True)
    print(p.stdout[-3000:])
    assert p.returncode == 0 and p.stdout.strip().split('\n')[-1] == '0 violations', p.stdout[-3000:]
