"""GPU suite (-m gpu): a plain batch that streams its results (FXJPS_STREAM_RESULTS=1, set for every test of this module)
-- the search kernel leaves every finished path in a pinned arena on the host as the query ends, and the host assembles
offsets and cells from there.  Every result is compared bit for bit (offsets, cells, status, float64
cost bytes) with the CPU oracle or with the same call under FXJPS_STREAM_RESULTS=0, which packs on the device and copies
back as every batch does by default.

That a batch did stream is read off the pinned memory the library holds (Planner.live_bytes): the arena is pinned, and
FXJPS_ARENA_CELLS makes it a size nothing else of a small batch comes near."""
import ctypes as C

import numpy as np
import pytest

from test_gpu_fullsize import assert_same, oracle_csr, with_env

pytestmark = pytest.mark.gpu
NTHREADS = 16  # (the oracle's threads: what a test command may use)
OFF = {"FXJPS_STREAM_RESULTS": 0}


@pytest.fixture(scope="module", autouse=True)
def streaming_on():
    with with_env(FXJPS_STREAM_RESULTS=1):
        yield


@pytest.fixture(scope="module")
def planner():
    import fuxi_planner_amd as fx
    p = fx.Planner([0])
    yield p
    p.close()


def pinned():
    import fuxi_planner_amd as fx
    return fx.Planner.live_bytes()[1]


@pytest.fixture(scope="module")
def mixed():
    """300 queries on 64 x 64 at 20 %: random ones, start == goal (free and occupied), goals in a walled-in cell, a start
    off the grid, a goal on an obstacle."""
    from fuxi_planner_amd import synth
    occ = synth.synth_grid(64, 64, 21, 0.20)
    occ[29:34, 29:34] = 0
    occ[30:33, 30:33] = 1
    occ[31, 31] = 0  # a free cell nothing leads to
    s, g = synth.synth_queries(occ, 21, 300)
    s, g = s.copy(), g.copy()
    free = np.argwhere(occ == 0)
    wall = np.argwhere(occ == 1)
    s[10:20] = g[10:20]                 # start == goal on free cells
    s[20], g[20] = wall[0], wall[0]     # ... on an obstacle
    g[30:40] = [31, 31]                 # walled-in goals
    s[40], g[41] = [31, 31], [31, 31]   # out of the pocket; into it
    s[41] = [31, 31]                    # ... and inside it: start == goal
    s[50] = [-1, 3]
    g[51] = wall[1]
    g[52] = [64, 0]
    s[53], g[53] = free[0], free[-1]
    return occ, s.astype(np.int32), g.astype(np.int32)


@pytest.fixture(scope="module")
def head():
    """4 096 queries on 128 x 128: the head launch runs beside the batch's."""
    from fuxi_planner_amd import synth
    occ = synth.synth_grid(128, 128, 22, 0.20)
    s, g = synth.synth_queries(occ, 22, 4096)
    return occ, s, g


@pytest.fixture(scope="module")
def head_off(planner, head):
    """... and its results with streaming switched off (read-only: shared by the tests below)."""
    occ, s, g = head
    planner.set_grid_occ(occ)
    with with_env(**OFF):
        return planner.plan_batch(s, g, 2, 512)


def test_mixed_batch_matches_the_oracle(planner, oracle, mixed):
    occ, s, g = mixed
    planner.set_grid_occ(occ)
    for h in (2, 1):
        res = planner.plan_batch(s, g, h, 256)
        assert planner.timing()["table_direct"] == 1, planner.timing()  # (the instantiations that stream)
        assert_same(res, oracle_csr(oracle, occ, s, g, h, 256, NTHREADS))
        st = res[3]
        assert (st[10:20] == 1).all() and st[20] == 1 and st[41] == 1 and (st[30:40] == 0).all() and st[40] == 0 and st[50] == -2
    # a path slot of ten cells: -1 (FXJPS_Q_PATH_TOO_LONG) where the path has more jump points, per query (both kinds occur)
    short = planner.plan_batch(s, g, 2, 10)
    assert (short[3] == -1).any() and (short[3] > 1).any(), np.bincount(short[3] + 5)
    assert_same(short, oracle_csr(oracle, occ, s, g, 2, 10, NTHREADS))
    with with_env(**OFF):
        assert_same(planner.plan_batch(s, g, 2, 10), short)


def test_a_plain_batch_streams_and_the_knob_switches_it_off(mixed):
    """The arena is there after a batch under FXJPS_STREAM_RESULTS=1 and is not under =0; the results are the same."""
    import fuxi_planner_amd as fx
    occ, s, g = mixed
    cells, res = 3000000, []
    for env, streams in (({"FXJPS_ARENA_CELLS": cells}, True), (dict(OFF, FXJPS_ARENA_CELLS=cells), False)):
        with fx.Planner([0]) as p:
            p.set_grid_occ(occ)
            before = pinned()
            with with_env(**env):
                res.append(p.plan_batch(s, g, 2, 256))
            grown = pinned() - before
            assert (grown >= 4 * cells) == streams, (env, grown)
    assert_same(res[0], res[1])


def test_without_the_knob(planner, oracle, mixed, monkeypatch):
    """No FXJPS_STREAM_RESULTS in the environment: the library's default, through the same exit code of the kernel, against
    the oracle -- resident grid and grid slots."""
    occ, s, g = mixed
    monkeypatch.delenv("FXJPS_STREAM_RESULTS")
    planner.set_grid_occ(occ)
    want = oracle_csr(oracle, occ, s, g, 2, 256, NTHREADS)
    assert_same(planner.plan_batch(s, g, 2, 256), want)
    planner.set_grid_slot(5, occ)
    assert_same(planner.plan_batch_slots(np.full(len(s), 5, np.int32), s, g, 2, 256), want)
    planner.clear_grid_slot(5)


def test_head_launch(planner, head, head_off):
    occ, s, g = head
    planner.set_grid_occ(occ)
    t0 = planner.timing()["solo_timeouts"]
    res = planner.plan_batch(s, g, 2, 512)
    t = planner.timing()
    assert t["search_launches"] == 2 or t["solo_timeouts"] > t0, t
    assert t["table_direct"] == 1, t
    assert_same(res, head_off)


def test_arena_overflow(head, head_off):
    """An arena of 64 cells overflows: the batch is packed on the device as before, the results are the same, and the next
    call -- without the knob -- streams again, into an arena of its own size."""
    import fuxi_planner_amd as fx
    occ, s, g = head
    assert head_off[0][-1] > 64 * 100
    with fx.Planner([0]) as p:
        p.set_grid_occ(occ)
        with with_env(FXJPS_ARENA_CELLS=64):
            assert_same(p.plan_batch(s, g, 2, 512), head_off)
        before = pinned()
        assert_same(p.plan_batch(s, g, 2, 512), head_off)
        assert pinned() - before >= 4 * len(s) * 512, (before, pinned())  # (the first-use size: nq * min(max_len, 512) cells)
        assert_same(p.plan_batch(s, g, 2, 512), head_off)


def test_retry_on_the_large_pool(planner):
    from fuxi_planner_amd import synth
    occ = synth.synth_grid(300, 200, 11, 0.02)  # (the sparse map of the retry scenarios in test_search_work_gpu.py)
    s, g = synth.synth_queries(occ, 11, 400)
    planner.set_grid_occ(occ)
    with with_env(**OFF):
        want = {h: planner.plan_batch(s, g, h, 1024) for h in (2, 1)}
    # (a far tier of 64 alone: cell-indexed tables, the first pass streams and the large pool's hashed kernel does not)
    for env in ({"FXJPS_FAR_CAP": 64, "FXJPS_TABLE_LOG2": 8}, {"FXJPS_FAR_CAP": 64}):
        with with_env(**env):
            for h in (2, 1):
                res = planner.plan_batch(s, g, h, 1024)
                assert planner.timing()["retried"] > 0, (env, planner.timing())
                assert_same(res, want[h])
    assert_same(planner.plan_batch(s, g, 2, 1024), want[2])


def test_grid_slot_batch(planner, oracle, mixed):
    from fuxi_planner_amd import synth
    grids = {3: mixed[0], 7: synth.synth_grid(50, 70, 23, 0.20)}
    ids, S, G = [], [mixed[1]], [mixed[2]]
    ids += [3] * len(mixed[1])
    s7, g7 = synth.synth_queries(grids[7], 23, 200)
    ids += [7] * len(s7)
    ids = np.array(ids, np.int32)
    s, g = np.concatenate(S + [s7]).astype(np.int32), np.concatenate(G + [g7]).astype(np.int32)
    perm = np.random.default_rng(23).permutation(len(ids))
    ids, s, g = ids[perm], s[perm], g[perm]
    for k, occ in grids.items():
        planner.set_grid_slot(k, occ)
    res = planner.plan_batch_slots(ids, s, g, 2, 256)
    assert planner.timing()["table_direct"] == 1, planner.timing()
    with with_env(**OFF):
        assert_same(planner.plan_batch_slots(ids, s, g, 2, 256), res)
    off, cells, cost, st = res
    for k, occ in grids.items():
        idx = np.flatnonzero(ids == k)
        want = oracle_csr(oracle, occ, s[idx], g[idx], 2, 256, NTHREADS)
        assert np.array_equal(st[idx], want[3]) and cost[idx].tobytes() == want[2].tobytes()
        assert np.array_equal(np.concatenate([cells[off[q]:off[q + 1]] for q in idx]), want[1])
    for k in grids:
        planner.clear_grid_slot(k)


def test_dense_call_and_resident_waypoints_after_a_streamed_batch(planner, mixed):
    """The dense fxjps_plan_batch reads h_cells, the resident form of the waypoint call the CSR on the device: both are
    built on demand out of what a streamed batch left."""
    from fuxi_planner_amd import _lib, waypoints
    occ, s, g = mixed
    n, mpl = len(s), 256
    planner.set_grid_occ(occ)
    with with_env(**OFF):
        off, cells, cost, st = planner.plan_batch(s, g, 2, mpl)
    dense = np.full((n, mpl, 2), -7, np.int32)
    dlen, dcost, secs = np.zeros(n, np.int32), np.zeros(n), C.c_double(0.0)
    planner._chk(planner._L.fxjps_plan_batch(planner._h, _lib.ptr(s, C.c_int32), _lib.ptr(g, C.c_int32), n, 2, mpl, _lib.ptr(dense, C.c_int32),
                                             _lib.ptr(dlen, C.c_int32), _lib.ptr(dcost, C.c_double), C.byref(secs)))
    assert np.array_equal(dlen, st) and dcost.tobytes() == cost.tobytes()
    for q in range(n):
        k = max(int(st[q]), 0)
        assert np.array_equal(dense[q, :k], cells[off[q]:off[q + 1]]) and (dense[q, k:] == -7).all(), q
    # the resident paths of a streamed batch == the same paths handed over
    assert_same(planner.plan_batch(s, g, 2, mpl), (off, cells, cost, st))
    pos, goal = np.c_[s + 0.5, np.zeros(n)], np.c_[g + 0.0, np.ones(n)]
    a = waypoints.select_ccst_batch(planner, n, 1.0, (0.0, 0.0), pos, goal)
    b = waypoints.select_ccst_batch(planner, n, 1.0, (0.0, 0.0), pos, goal, paths=(off, cells))
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
    assert (a[2] > 0).sum() > 100
    # ... and the cells are still there for the caller afterwards
    again = np.empty((int(off[n]), 2), np.int32)
    planner._chk(planner._L.fxjps_last_cells(planner._h, _lib.ptr(again, C.c_int32), int(off[n])))
    assert np.array_equal(again, cells)


def test_two_contexts(head, head_off):
    import fuxi_planner_amd as fx
    occ, s, g = head
    with fx.Planner([0, 0]) as p2:
        p2.set_grid_occ(occ)
        assert_same(p2.plan_batch(s, g, 2, 512), head_off)
        assert min(t["queries"] for t in p2.timing_per_context()) > 0
        with with_env(FXJPS_ARENA_CELLS=64):  # (both arenas overflow)
            assert_same(p2.plan_batch(s, g, 2, 512), head_off)
        assert_same(p2.plan_batch(s, g, 2, 512), head_off)
