"""Records sid_pm_estimate_run_time for the fixed list of cases of tests/golden/run_time_cases.txt.

    SID_PM_LIB=<library to record> python tools/record_run_time_cases.py > tests/golden/run_time_cases.txt

The function is host arithmetic (no HIP call), so any machine that can load the library will do.  tests/cpp/run_time_check.cpp
recomputes every case from csrc/pm_plan.h alone and compares the doubles for equality: record from the library BEFORE a change
that must leave the model as it is.

One line per (borders, img_size): `<grid | border:n> <img_size>`, then the 48 times (ns, %.17g) of n_angles 3, 7, 15, 16 x flags
1, 7 x SID_PM_SIDE_BY_SIDE unset, 0, 1 x SID_DIST_TAIL_BLEND unset, 0.3, the last varying fastest; `=` repeats the value before it.
`grid` is the border vector of synthetic.make_grid(10000, 10000, 200, 'mixed') (grid_borders; the test hands it to the checker).
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sea_ice_drift_amd import synthetic  # noqa: E402


def grid_borders():
    return np.ascontiguousarray(synthetic.make_grid(10000, 10000, 200, 'mixed')['border'], dtype=np.float64).ravel()


def main():
    from sea_ice_drift_amd import _capi
    sets = [('grid', grid_borders())]
    for b in (20, 24, 30, 50, 70, 112):
        for n in (1, 255, 256, 257, 40000):
            sets.append(('%d:%d' % (b, n), np.full(n, float(b))))
    print('# sid_pm_estimate_run_time, recorded by tools/record_run_time_cases.py (the format is told there)')
    for name, border in sets:
        for s in (34, 35, 20, 70):
            vals = []
            for K in (3, 7, 15, 16):
                for flags in (1, 7):
                    for side in (None, '0', '1'):
                        for blend in (None, '0.3'):
                            for key, val in (('SID_PM_SIDE_BY_SIDE', side), ('SID_DIST_TAIL_BLEND', blend)):
                                os.environ.pop(key, None)
                                if val is not None:
                                    os.environ[key] = val
                            t = '%.17g' % _capi.estimate_run_time(border, s, K, flags)
                            vals.append('=' if vals and t == last else t)
                            last = t
            print('%s %d %s' % (name, s, ' '.join(vals)))


if __name__ == '__main__':
    main()
