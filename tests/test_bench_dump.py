"""CPU tests of bench.py's --dump-outputs writer and of its command line (no GPU: nothing here starts a run)."""
import os

import numpy as np

import bench


def test_dump_outputs_writes_float64_arrays(tmp_path):
    bench.dump_outputs(str(tmp_path), {'results': np.arange(10.0).reshape(5, 2), 'peak_index': np.arange(6, dtype=np.int32).reshape(3, 2)})
    r, ij = np.load(str(tmp_path / 'results.npy')), np.load(str(tmp_path / 'peak_index.npy'))
    assert r.dtype == ij.dtype == np.float64
    np.testing.assert_array_equal(r, np.arange(10.0).reshape(5, 2))
    np.testing.assert_array_equal(ij, np.arange(6).reshape(3, 2))


def test_dump_outputs_samples_large_outputs_within_64_mb(tmp_path):
    """Beyond 64 MB every array keeps the same seeded share of its rows: the same rows on every call, in order."""
    big = {'a': np.arange(6 << 20, dtype=np.float64).reshape(-1, 2), 'b': np.arange(5 << 20, dtype=np.int32)}
    for sub in ('one', 'two'):
        bench.dump_outputs(str(tmp_path / sub), big)
    total = sum(os.path.getsize(str(tmp_path / 'one' / f)) for f in os.listdir(str(tmp_path / 'one')))
    assert total <= bench.DUMP_LIMIT_BYTES + 4096
    for name in ('a', 'b'):
        x, y = np.load(str(tmp_path / 'one' / (name + '.npy'))), np.load(str(tmp_path / 'two' / (name + '.npy')))
        np.testing.assert_array_equal(x, y)
        rows = x[:, 0] if x.ndim == 2 else x
        assert 0 < len(rows) < len(big[name]) and np.all(np.diff(rows) > 0)
    a = np.load(str(tmp_path / 'one' / 'a.npy'))
    np.testing.assert_array_equal(a[:, 1], a[:, 0] + 1)          # whole rows are kept


def test_plain_run_is_the_default_and_full_is_an_option():
    args = bench.parse_args(['--gpus', '1', '--steps', '7', '--warmup', '2'])
    assert args.steps == 7 and args.warmup == 2 and not args.full and args.dump_outputs is None
    args = bench.parse_args(['--steps', '3', '--full', '--dump-outputs', 'out'])
    assert args.full and args.dump_outputs == 'out'
