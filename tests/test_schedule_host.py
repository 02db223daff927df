"""Host-side checks of what sid_pm_run executes and what the shards are priced with, g++ only (csrc/pm_plan.h, csrc/pm_host.h):

tests/cpp/schedule_check.cpp - the launch order of a run (launch_schedule) over every vector of 1..6 bucket counts from
{0, 1, 24, 5000}, both kernel families, the three per-run switches, devices with and without stream wait-value support and handles
with and without signal memory: one step per launch, order and reason as side_by_side_rule / chain_reason say, every wait of a
chained run on the release word of the latest earlier launch that counts its arrivals, the last launch counting nothing, the
streams draining with at most two chained launches in flight, and - cut after any step, as a failed launch would - the words the
host stores covering every wait already enqueued; the side-by-side stream assignment, its one join and the fork waits.

tests/cpp/run_time_check.cpp - estimate_run_time against tests/golden/run_time_cases.txt, recorded from the library before the
model moved into pm_plan.h (tools/record_run_time_cases.py): 5952 cases, the doubles equal.

tests/cpp/lifetime_check.cpp - a program of its own under AddressSanitizer and UBSan: the scoped device buffer against a stub
allocator (move, grow, refuse, early return, members of a deleted handle) and the arena layout of sid_pm_set_points."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(tmp_path, name, flags=('-O1',), args=()):
    exe = str(tmp_path / name)
    subprocess.check_call(['g++', '-std=c++17', *flags, '-o', exe, os.path.join(ROOT, 'tests', 'cpp', name + '.cpp')])
    p = subprocess.run([exe, *args], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    print(p.stdout[-3000:])
    assert p.returncode == 0 and p.stdout.strip().split('\n')[-1] == '0 violations', p.stdout[-3000:]
    return p.stdout


def test_launch_schedule(tmp_path):
    _run(tmp_path, 'schedule_check')


def test_run_time_model_is_the_recorded_one(tmp_path):
    import numpy as np
    from sea_ice_drift_amd import synthetic
    border = np.asarray(synthetic.make_grid(10000, 10000, 200, 'mixed')['border'], dtype=np.float64).ravel()
    grid = tmp_path / 'grid_borders.txt'
    grid.write_text('%d\n%s\n' % (border.size, ' '.join('%.17g' % v for v in border)))
    out = _run(tmp_path, 'run_time_check', args=(os.path.join(ROOT, 'tests', 'golden', 'run_time_cases.txt'), str(grid)))
    assert '5952 cases' in out


def test_lifetimes_under_sanitizers(tmp_path):
    _run(tmp_path, 'lifetime_check', flags=('-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=undefined'))
