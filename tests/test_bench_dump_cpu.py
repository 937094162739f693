"""bench.py --dump-outputs helpers on the host: the seeded sample repeats, dtypes are written as documented
(float64 stays float64, everything else becomes float32), and the 64 MB budget is enforced before anything is written."""
import os

import numpy as np
import pytest
import torch

import bench


def test_sample_is_whole_below_the_limit_and_repeatable_above_it():
    small = torch.arange(10, dtype=torch.float32)
    assert torch.equal(bench.dump_sample(small, 10), small)
    big = torch.arange(100_000, dtype=torch.float32).reshape(100, 1000)
    a, b = bench.dump_sample(big, 4096), bench.dump_sample(big, 4096)
    assert a.shape == (4096,) and torch.equal(a, b)
    # distinct positions, in increasing order, taken from the flattened array
    assert bool((a[1:] > a[:-1]).all()) and float(a.min()) >= 0 and float(a.max()) < 100_000


def test_dump_writes_float32_and_keeps_float64(tmp_path):
    out = str(tmp_path / 'dump')
    bench.dump_outputs(out, {'h': torch.ones(2, 3, dtype=torch.bfloat16), 'i': torch.arange(4),
                             'l': torch.tensor([1.5], dtype=torch.float64)})
    got = {f: np.load(os.path.join(out, f)) for f in sorted(os.listdir(out))}
    assert sorted(got) == ['h.npy', 'i.npy', 'l.npy']
    assert got['h.npy'].dtype == np.float32 and got['h.npy'].shape == (2, 3) and np.all(got['h.npy'] == 1.0)
    assert got['i.npy'].dtype == np.float32 and np.array_equal(got['i.npy'], np.arange(4, dtype=np.float32))
    assert got['l.npy'].dtype == np.float64 and got['l.npy'][0] == 1.5


def test_dump_over_budget_raises_and_writes_nothing(tmp_path):
    out = str(tmp_path / 'dump')
    with pytest.raises(RuntimeError, match='budget'):
        bench.dump_outputs(out, {'big': torch.zeros(bench.DUMP_MAX_BYTES // 4 + 1)})
    assert not os.path.exists(out)
