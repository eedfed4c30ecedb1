"""bench.py --dump-outputs (dump_outputs) on host tensors: the files, their dtypes, the block
sums against numpy, the sample against the grid, and the same bytes from call to call."""
import os

import numpy as np
import torch


def _dump(tmp_path, name, grid, seed=7):
    import bench
    g = torch.Generator().manual_seed(seed)
    lo = torch.randint(-32768, 32767, (grid ** 3 + 40,), dtype=torch.int16, generator=g)  # padded like the bench's
    out = tmp_path / name
    bench.dump_outputs(str(out), lo, grid, (30.0, 20.0, 10.0), 10)
    return lo.numpy()[:grid ** 3], {f[:-4]: np.load(out / f) for f in sorted(os.listdir(out))}


def test_dump_outputs_small_grid(tmp_path):
    grid = 24  # three blocks of 8 per axis; fewer cells than the sample: every cell is written
    lo, d = _dump(tmp_path, "a", grid)
    assert sorted(d) == ["fuse_counts", "logodds_block_sums", "logodds_sample", "logodds_sample_cells"]
    assert d["logodds_sample"].dtype == np.float32
    assert all(d[k].dtype == np.float64 for k in d if k != "logodds_sample")
    ref = lo.astype(np.float64).reshape(3, 8, 3, 8, 3, 8).sum(axis=(1, 3, 5))
    assert np.array_equal(d["logodds_block_sums"], ref)
    assert np.array_equal(d["logodds_sample_cells"], np.arange(grid ** 3))
    assert np.array_equal(d["logodds_sample"], lo.astype(np.float32))
    assert np.array_equal(d["fuse_counts"], [3.0, 2.0, 1.0])
    _, again = _dump(tmp_path, "b", grid)
    assert all(np.array_equal(d[k], again[k]) for k in d)


def test_dump_outputs_sampled_grid(tmp_path, monkeypatch):
    import bench
    monkeypatch.setattr(bench, "DUMP_SAMPLE_CELLS", 1000)
    grid = 20  # no multiple of the block: no block sums; more cells than the sample
    lo, d = _dump(tmp_path, "a", grid)
    assert sorted(d) == ["fuse_counts", "logodds_sample", "logodds_sample_cells"]
    cells = d["logodds_sample_cells"].astype(np.int64)
    assert cells.shape == (1000,) and np.all(np.diff(cells) >= 0) and cells[0] >= 0 and cells[-1] < grid ** 3
    assert np.array_equal(d["logodds_sample"], lo[cells].astype(np.float32))
    _, again = _dump(tmp_path, "b", grid, seed=8)  # other values, the same cells
    assert np.array_equal(d["logodds_sample_cells"], again["logodds_sample_cells"])
