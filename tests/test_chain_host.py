"""Host-side checks of the chained launches, g++ only: tests/cpp/chain_check.cpp checks that the shards of the kernels' arrival
count (csrc/pm_kernel.h chain_shard_count) sum to the launch for 1..4100 workgroups and are empty exactly where they must be,
and the truth table of the launcher's rule (csrc/pm_plan.h chain_rule) over 1 / 2 / 5 launches, short and long runs, devices
with and without stream wait-value support, handles with and without signal memory, and SID_PM_NO_CHAIN."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_chain_shards_and_rule(tmp_path):
    exe = str(tmp_path / 'chain_check')
    subprocess.check_call(['g++', '-std=c++17', '-O1', '-o', exe, os.path.join(ROOT, 'tests', 'cpp', 'chain_check.cpp')])
    p = subprocess.run([exe], stdout=subprocess.PIPE, universal_newlines=True)
    print(p.stdout[-3000:])
    assert p.returncode == 0 and p.stdout.strip().split('\n')[-1] == '0 violations', p.stdout[-3000:]
