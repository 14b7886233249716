"""CPU: bench.py's --dump-outputs writer (float32 .npy files, a fixed seeded sample above DUMP_MAX elements) and its option rules."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def test_dump_outputs_writes_float32_and_samples_large_arrays_the_same_way_every_time(tmp_path):
    import bench
    big = np.arange(bench.DUMP_MAX + 1000, dtype=np.float64)
    small = np.array([[1, 2], [3, 4]], dtype=np.int64)
    for d in ('a', 'b'):
        bench.dump_outputs(str(tmp_path / d), dict(big=big, small=small))
    a_big, a_small = np.load(tmp_path / 'a' / 'big.npy'), np.load(tmp_path / 'a' / 'small.npy')
    assert a_small.dtype == np.float32 and a_small.shape == (2, 2) and a_small.tolist() == [[1, 2], [3, 4]]
    assert a_big.dtype == np.float32 and a_big.shape == (bench.DUMP_MAX,)
    assert np.all(np.diff(a_big) >= 0) and a_big.min() >= 0 and a_big.max() < big.size      # sorted indices into the array
    assert np.array_equal(a_big, np.load(tmp_path / 'b' / 'big.npy'))                        # same sample on every call


def test_shapes_needs_full(monkeypatch):
    import bench
    monkeypatch.setattr(sys, 'argv', ['bench.py', '--shapes', 'x.txt'])
    with pytest.raises(SystemExit):
        bench.parse()
    monkeypatch.setattr(sys, 'argv', ['bench.py', '--full', '--shapes', 'x.txt', '--dump-outputs', 'out'])
    args = bench.parse()
    assert args.full and args.shapes == 'x.txt' and args.dump_outputs == 'out'
    monkeypatch.setattr(sys, 'argv', ['bench.py', '--steps', '7'])
    args = bench.parse()
    assert not args.full and args.dump_outputs is None and args.steps == 7
