"""bench.py --dump-outputs (CPU): the writer keeps small arrays whole, samples a large one by a fixed seeded
set of rows inside the byte budget, and writes float32 files that are identical from call to call."""
import os

import numpy as np
import torch

import bench


def _outputs():
    g = torch.Generator().manual_seed(5)
    return {"imp": torch.rand(3, 40, 6, generator=g), "h1": torch.rand(3, 40, 2, generator=g, dtype=torch.float64),
            "h2": torch.rand(3, 40, 50, generator=g)}


def test_dump_whole_arrays(tmp_path):
    out = _outputs()
    bench.dump_outputs(out, str(tmp_path / "d"), 0, 1)
    assert sorted(os.listdir(tmp_path / "d")) == ["h1.npy", "h2.npy", "imp.npy"]
    for name, t in out.items():
        a = np.load(tmp_path / "d" / f"{name}.npy")
        assert a.dtype == np.float32 and a.shape == tuple(t.shape)
        assert np.array_equal(a, t.to(torch.float32).numpy())


def test_dump_samples_rows_within_budget(tmp_path, monkeypatch):
    out = _outputs()
    budget = 3 * 40 * (6 + 2) * 4 + 30 * 50 * 4          # imp and h1 whole, 30 of h2's 120 rows
    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", budget)
    bench.dump_outputs(out, str(tmp_path / "a"), 0, 1)
    bench.dump_outputs(out, str(tmp_path / "b"), 0, 1)
    imp, h1, h2 = (np.load(tmp_path / "a" / f"{n}.npy") for n in ("imp", "h1", "h2"))
    assert imp.shape == (3, 40, 6) and h1.shape == (3, 40, 2) and h2.shape == (30, 50)
    assert imp.nbytes + h1.nbytes + h2.nbytes <= budget
    # the sample is rows of the flattened array in ascending order, the same rows in every call
    flat = out["h2"].reshape(-1, 50).numpy()
    rows = [int(np.flatnonzero((flat == r).all(axis=1))[0]) for r in h2]
    assert rows == sorted(set(rows))
    assert np.array_equal(h2, np.load(tmp_path / "b" / "h2.npy"))


def test_dump_ranks_split_the_budget(tmp_path, monkeypatch):
    out = _outputs()
    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", 2 * 3 * 40 * (6 + 2 + 50) * 4 - 2 * 20 * 50 * 4)
    for rank in range(2):
        bench.dump_outputs(out, str(tmp_path), rank, 2)
    files = sorted(os.listdir(tmp_path))
    assert files == [f"{n}_rank{r}.npy" for n in ("h1", "h2", "imp") for r in range(2)]
    assert sum(np.load(tmp_path / f).nbytes for f in files) <= bench.DUMP_BUDGET_BYTES
    assert np.load(tmp_path / "h2_rank1.npy").shape == (100, 50)      # each rank: everything but 20 rows of h2
