"""bench.py --dump-outputs (bench.dump_outputs): the CSR result of a step as .npy files, every query when it fits in
64 MB, else a fixed seeded sample of the queries -- the same sample from run to run."""
import os

import numpy as np

import bench


def _csr(n, mean, seed):
    rng = np.random.default_rng(seed)
    lens = rng.integers(0, 2 * mean + 1, n)
    off = np.zeros(n + 1, dtype=np.int64)
    off[1:] = np.cumsum(lens)
    cells = rng.integers(0, 4096, (int(off[-1]), 2)).astype(np.int32)
    status = lens.astype(np.int32)
    status[::97] = -3  # (a per-query error code)
    return off, cells, rng.random(n), status


def _load(d):
    return {k: np.load(os.path.join(d, k + ".npy")) for k in ("offsets", "cells", "cost", "status", "query_ids")}


def _check(got, res):
    off, cells, cost, status = res
    ids = got["query_ids"].astype(np.int64)
    assert got["cells"].dtype == np.float32 and all(got[k].dtype == np.float64 for k in ("offsets", "cost", "status", "query_ids"))
    assert np.array_equal(got["cost"], cost[ids]) and np.array_equal(got["status"], status[ids].astype(np.float64))
    o = got["offsets"].astype(np.int64)
    assert len(o) == len(ids) + 1 and o[0] == 0
    for j, q in enumerate(ids):
        assert np.array_equal(got["cells"][o[j]:o[j + 1]].astype(np.int32), cells[off[q]:off[q + 1]])


def test_small_output_is_written_whole(tmp_path):
    res = _csr(3000, 40, 1)
    rec = bench.dump_outputs(str(tmp_path), res)
    got = _load(str(tmp_path))
    assert not rec["sampled"] and np.array_equal(got["query_ids"], np.arange(3000, dtype=np.float64))
    _check(got, res)


def test_large_output_is_a_fixed_sample_within_64_mb(tmp_path):
    res = _csr(200000, 60, 2)  # (~ 190 MB of cells as float32)
    a, b = tmp_path / "a", tmp_path / "b"
    ra, rb = bench.dump_outputs(str(a), res), bench.dump_outputs(str(b), res)
    assert ra["sampled"] and 0 < ra["queries_written"] < 200000
    assert sum(os.path.getsize(os.path.join(str(a), f)) for f in os.listdir(str(a))) <= 64 << 20
    ga, gb = _load(str(a)), _load(str(b))
    for k in ga:
        assert ga[k].tobytes() == gb[k].tobytes()
    ids = ga["query_ids"].astype(np.int64)
    assert np.all(np.diff(ids) > 0)
    _check(ga, res)
