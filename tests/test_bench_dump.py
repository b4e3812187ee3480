"""bench.py --dump-outputs: what bench.dump_outputs writes for a step's shards.  CPU only: the shards are host tensors of
the shapes and dtypes the timed path returns (Q float32, idx uint8, row_err float32, info int32)."""

import importlib.util
import os

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def load_bench():
    spec = importlib.util.spec_from_file_location("bench_module", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    return bench


def fake_step(shapes, seed):
    g = torch.Generator().manual_seed(seed)
    shards = []
    for R, n in shapes:
        idx = torch.randint(0, 8, (R, n), generator=g, dtype=torch.uint8)
        shards.append({"Q": idx.float() / 7 - 0.5, "idx": idx, "row_err": torch.rand(R, generator=g), "rows": (0, R),
                       "info": torch.zeros(1, dtype=torch.int32)})
    return shards


def test_dump_is_a_fixed_sample_under_the_limit(tmp_path):
    bench = load_bench()
    shapes = [(512, 384), (256, 1024), (512, 384)]
    shards = fake_step(shapes, 7)
    errs = [float(sh["row_err"].double().mean()) for sh in shards]
    limit = 400_000  # far below the 2.2 MB of Q and idx: a sample of rows
    written = bench.dump_outputs(str(tmp_path / "a"), shapes, shards, errs, limit=limit)
    files = sorted(os.listdir(tmp_path / "a"))
    assert 0 < written <= limit and written == sum(os.path.getsize(tmp_path / "a" / f) for f in files)
    assert files == sorted(["layer_errors.npy", "info.npy"] + [f"layer{i:03d}_{k}.npy" for i in range(3) for k in ("rows", "row_err", "Q", "idx")])
    for f in files:
        assert np.load(tmp_path / "a" / f).dtype in (np.float32, np.float64), f
    np.testing.assert_array_equal(np.load(tmp_path / "a" / "layer_errors.npy"), errs)
    for i, (R, n) in enumerate(shapes):
        rows = np.load(tmp_path / "a" / f"layer{i:03d}_rows.npy").astype(np.int64)
        assert 0 < len(rows) < R and np.all(np.diff(rows) > 0)
        np.testing.assert_array_equal(np.load(tmp_path / "a" / f"layer{i:03d}_Q.npy"), shards[i]["Q"].numpy()[rows])
        np.testing.assert_array_equal(np.load(tmp_path / "a" / f"layer{i:03d}_idx.npy"), shards[i]["idx"].numpy()[rows].astype(np.float32))
        np.testing.assert_array_equal(np.load(tmp_path / "a" / f"layer{i:03d}_row_err.npy"), shards[i]["row_err"].numpy())
    # another step with other values: the same rows are sampled
    bench.dump_outputs(str(tmp_path / "b"), shapes, fake_step(shapes, 8), errs, limit=limit)
    for i in range(3):
        np.testing.assert_array_equal(np.load(tmp_path / "a" / f"layer{i:03d}_rows.npy"), np.load(tmp_path / "b" / f"layer{i:03d}_rows.npy"))


def test_small_outputs_are_dumped_whole(tmp_path):
    bench = load_bench()
    shapes = [(64, 96)]
    shards = fake_step(shapes, 3)
    bench.dump_outputs(str(tmp_path), shapes, shards, [0.5])
    np.testing.assert_array_equal(np.load(tmp_path / "layer000_Q.npy"), shards[0]["Q"].numpy())
    np.testing.assert_array_equal(np.load(tmp_path / "layer000_rows.npy"), np.arange(64))
