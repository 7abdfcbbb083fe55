"""GPU suite (-m gpu): grid slots -- several resident grids per handle, one batch in which every query names its grid
(fxjps_set_grid_slot / fxjps_plan_batch_slots_csr).  Every result is compared bit for bit (cells, lengths, float64 cost)
with the CPU oracle on that query's own grid, and with the resident-grid path of a separate handle."""
import os

import numpy as np
import pytest

from test_gpu_fullsize import assert_same, oracle_csr, with_env
from test_gpu_parity import path_invariants

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MPL = 1024
NTHREADS = 16  # (the oracle's threads: what a test command may use)


def subset(res, idx):
    """The results of queries `idx` (in that order) of a CSR batch, as a CSR batch of their own."""
    off, cells, cost, st = res
    parts = [cells[off[q]:off[q + 1]] for q in idx]
    sub_off = np.zeros(len(idx) + 1, dtype=np.int64)
    sub_off[1:] = np.cumsum([len(p) for p in parts])
    sub_cells = np.concatenate(parts) if parts else np.zeros((0, 2), np.int32)
    return sub_off, sub_cells.reshape(-1, 2), cost[idx], st[idx]


def check_oracle(oracle, grids, ids, s, g, res, h, mpl=MPL):
    for k in np.unique(ids):
        idx = np.flatnonzero(ids == k)
        assert_same(subset(res, idx), oracle_csr(oracle, grids[int(k)], s[idx], g[idx], h, mpl, NTHREADS))


def check_resident(other, grids, ids, s, g, res, h, mpl=MPL):
    """Each slot's queries against set_grid + plan_batch on a separate handle."""
    for k in np.unique(ids):
        idx = np.flatnonzero(ids == k)
        other.set_grid_occ(grids[int(k)])
        assert_same(subset(res, idx), other.plan_batch(s[idx], g[idx], h, mpl))


def reference_map():
    """The largest map of the reference's PNG fixtures (uint8 [W][H])."""
    import json
    z = np.load(os.path.join(ROOT, "tests", "golden", "maps_png.npz"))
    with open(os.path.join(ROOT, "tests", "golden", "maps_png.json")) as f:
        recs = [r for r in json.load(f) if "canvas" not in r]
    rec = max(recs, key=lambda r: r["shape"][0] * r["shape"][1])
    W, H = rec["shape"]
    return np.unpackbits(z[rec["map"]])[:W * H].reshape(W, H).astype(np.uint8)


@pytest.fixture(scope="module")
def planner():
    import fuxi_planner_amd as fx
    p = fx.Planner([0])
    yield p
    p.close()


@pytest.fixture(scope="module")
def other():
    import fuxi_planner_amd as fx
    p = fx.Planner([0])
    yield p
    p.close()


@pytest.fixture(scope="module")
def mixed(planner):
    """Six slots of every kind of shape and a batch interleaved at random over them, with the edge cases."""
    from fuxi_planner_amd import synth
    grids = {0: synth.synth_grid(1024, 1024, 1, 0.20), 1: synth.synth_grid(700, 333, 2, 0.20), 2: synth.synth_grid(130, 2100, 3, 0.20),
             3: synth.synth_grid(3, 40, 4, 0.10), 4: reference_map(), 5: np.zeros((300, 200), np.uint8)}
    nper = {0: 300, 1: 200, 2: 200, 3: 40, 4: 200, 5: 100}
    ids, S, G = [], [], []
    for k, occ in grids.items():
        planner.set_grid_slot(k, occ)
        s, g = synth.synth_queries(occ, 10 + k, nper[k])
        ids += [k] * len(s)
        S.append(s)
        G.append(g)
    occ0 = grids[0]
    ox, oy = np.argwhere(occ0 == 1)[0]
    fx_, fy = np.argwhere(occ0 == 0)[0]
    extra = [(3, (500, 500), (1, 1)),        # inside the 1024^2 slot, outside its own 3 x 40 slot: BAD_START
             (3, (2, 39), (600, 600)),       # goal off its grid (on the large ones it would be a cell)
             (2, (0, 0), (129, 2100)), (0, (fx_, fy), (-1, 5)), (0, (fx_, fy), (1024, 3)),
             (0, (fx_, fy), (ox, oy)),       # goal on an obstacle
             (1, (5, 5), (5, 5)), (0, (ox, oy), (ox, oy)),  # start == goal (free / occupied)
             (5, (0, 0), (299, 199)), (4, (-1, 0), (3, 3))]
    for k, a, b in extra:
        ids.append(k)
        S.append(np.array([a], np.int32))
        G.append(np.array([b], np.int32))
    ids = np.array(ids, np.int32)
    S, G = np.concatenate(S).astype(np.int32), np.concatenate(G).astype(np.int32)
    perm = np.random.default_rng(7).permutation(len(ids))
    return grids, ids[perm], S[perm], G[perm]


def test_mixed_batch_matches_the_oracle(planner, oracle, mixed):
    grids, ids, s, g = mixed
    for h in (2, 1):
        res = planner.plan_batch_slots(ids, s, g, h, MPL)
        t = planner.timing()
        # (the largest W and the largest H of the batch's slots, 1024 and 2100: 10 + 12 bits of cell index do not fit the
        # budget -> hashed tables for the whole batch; test_hashed_tables_for_a_large_slot has a cell-indexed batch)
        assert t["table_direct"] == 0, t
        assert (res[3] == -2).sum() >= 2
        check_oracle(oracle, grids, ids, s, g, res, h)
    # a slot of path length too small: -1 where the path has more jump points, per query
    short = planner.plan_batch_slots(ids, s, g, 2, 3)
    assert (short[3] == -1).any()
    check_oracle(oracle, grids, ids, s, g, short, 2, 3)


def test_slot_batch_equals_the_resident_path(planner, other, mixed):
    grids, ids, s, g = mixed
    for h in (2, 1):
        check_resident(other, grids, ids, s, g, planner.plan_batch_slots(ids, s, g, h, MPL), h)
    for k, occ in grids.items():
        assert np.array_equal(planner.get_grid_slot(k), occ)
        other.set_grid_occ(occ)
        want, got = other.debug_maps(), planner.debug_slot_maps(k)
        assert set(want) == set(got)
        for name in want:
            assert want[name].tobytes() == got[name].tobytes(), (k, name)


def test_hashed_tables_for_a_large_slot(planner, oracle, mixed):
    """1100 x 1000: 11 + 10 bits of cell index do not fit the 40 % budget of a full chip -> the whole batch hashes."""
    from fuxi_planner_amd import synth
    grids = dict(mixed[0])
    grids[10] = synth.synth_grid(1100, 1000, 4, 0.20)
    planner.set_grid_slot(10, grids[10])
    parts = [(10, 600), (1, 200), (5, 200)]
    ids = np.concatenate([np.full(n, k, np.int32) for k, n in parts])
    qs = [synth.synth_queries(grids[k], 30 + k, n) for k, n in parts]
    s, g = np.concatenate([q[0] for q in qs]), np.concatenate([q[1] for q in qs])
    perm = np.random.default_rng(3).permutation(len(ids))
    ids, s, g = ids[perm], s[perm], g[perm]
    res = planner.plan_batch_slots(ids, s, g, 2, MPL)
    assert planner.timing()["table_direct"] == 0, planner.timing()
    check_oracle(oracle, grids, ids, s, g, res, 2)
    small = ids != 10
    res = planner.plan_batch_slots(ids[small], s[small], g[small], 2, MPL)
    assert planner.timing()["table_direct"] == 1, planner.timing()
    check_oracle(oracle, grids, ids[small], s[small], g[small], res, 2)
    planner.clear_grid_slot(10)


def _sixteen(planner, n_each, qseed):
    from fuxi_planner_amd import synth
    grids = {20 + i: synth.synth_grid(256, 256, 100 + i, 0.20) for i in range(16)}
    ids, S, G = [], [], []
    for k, occ in grids.items():
        planner.set_grid_slot(k, occ)
        s, g = synth.synth_queries(occ, qseed + k, n_each)
        ids.append(np.full(n_each, k, np.int32))
        S.append(s)
        G.append(g)
    ids, s, g = np.concatenate(ids), np.concatenate(S), np.concatenate(G)
    perm = np.random.default_rng(qseed).permutation(len(ids))
    return grids, ids[perm], s[perm], g[perm]


def _sample_check(oracle, other, grids, ids, s, g, res, h, per_slot):
    off, cells, cost, st = res
    rng = np.random.default_rng(5)
    pick = np.concatenate([rng.choice(np.flatnonzero(ids == k), per_slot, replace=False) for k in np.unique(ids)])
    check_oracle(oracle, grids, ids[pick], s[pick], g[pick], subset(res, pick), h, 512)
    check_resident(other, grids, ids, s, g, res, h, 512)  # (every query: against the resident path)
    for k in np.unique(ids)[:4]:
        idx = np.flatnonzero(ids == k)[:200]
        path_invariants(grids[int(k)], s[idx], g[idx], *subset(res, idx), hchoice=h)


def test_launch_shapes(planner, oracle, other):
    grids, ids, s, g = _sixteen(planner, 375, 40)  # 6 000 queries over 16 slots: the head launch beside the batch's
    t0 = planner.timing()["solo_timeouts"]
    res = planner.plan_batch_slots(ids, s, g, 2, 512)
    t = planner.timing()
    assert t["search_launches"] == 2 or t["solo_timeouts"] > t0, t
    _sample_check(oracle, other, grids, ids, s, g, res, 2, 30)
    grids, ids, s, g = _sixteen(planner, 2100, 41)  # 33 600 queries: one launch
    res = planner.plan_batch_slots(ids, s, g, 2, 512)
    assert planner.timing()["search_launches"] == 1, planner.timing()
    _sample_check(oracle, other, grids, ids, s, g, res, 2, 15)


def test_large_pool_retry(planner, mixed):
    grids, ids, s, g = mixed
    keep = np.isin(ids, [1, 3, 4, 5])
    ids, s, g = ids[keep], s[keep], g[keep]
    want = {h: planner.plan_batch_slots(ids, s, g, h, MPL) for h in (2, 1)}  # (oracle-checked above: same grids, same queries)
    for env in ({"FXJPS_TABLE_LOG2": 8}, {"FXJPS_FAR_CAP": 64}):
        with with_env(**env):
            for h in (2, 1):
                res = planner.plan_batch_slots(ids, s, g, h, MPL)
                assert planner.timing()["retried"] > 0, (env, planner.timing())
                assert_same(res, want[h])
    assert_same(planner.plan_batch_slots(ids, s, g, 2, MPL), want[2])


def test_lifecycle(planner, oracle, mixed):
    import fuxi_planner_amd as fx
    from fuxi_planner_amd import FxjpsError, _lib, synth, waypoints
    grids, ids, s, g = mixed
    occ_r = synth.synth_grid(400, 300, 9, 0.20)
    rs, rg = synth.synth_queries(occ_r, 9, 300)
    planner.set_grid_occ(occ_r)
    before = planner.plan_batch(rs, rg, 2, MPL)
    # a slot overwritten with another grid (another shape): results follow the new grid
    a, b = synth.synth_grid(200, 150, 50, 0.2), synth.synth_grid(180, 260, 51, 0.25)
    for occ in (a, b):
        planner.set_grid_slot(7, occ)
        assert np.array_equal(planner.get_grid_slot(7), occ)
        qs, qg = synth.synth_queries(occ, 52, 200)
        res = planner.plan_batch_slots(np.full(200, 7), qs, qg, 2, MPL)
        assert_same(res, oracle_csr(oracle, occ, qs, qg, 2, MPL, NTHREADS))
    # one query: the batch path, the same bytes
    one = planner.plan_batch_slots([1], s[ids == 1][:1], g[ids == 1][:1], 2, MPL)
    assert_same(one, oracle_csr(oracle, grids[1], s[ids == 1][:1], g[ids == 1][:1], 2, MPL, NTHREADS))
    # the ccst waypoint batch reads the resident grid: not on a slots batch's own paths, but on explicit ones as before
    with pytest.raises(FxjpsError) as e:
        waypoints.select_ccst_batch(planner, 1, 0.1, (0.0, 0.0), (0.0, 0.0, 0.0), (1.0, 1.0, 0.0))
    assert e.value.code == _lib.E_ARG
    q0 = int(np.flatnonzero(before[3] > 0)[0])  # (a path on the resident grid)
    path = (np.array([0, before[3][q0]], np.int64), before[1][before[0][q0]:before[0][q0 + 1]])
    waypoints.select_ccst_batch(planner, 1, 0.1, (0.0, 0.0), (0.0, 0.0, 0.0), (1.0, 1.0, 0.0), paths=path)
    # a released slot, ids out of range: FXJPS_E_ARG, and the handle goes on
    planner.clear_grid_slot(7)
    for bad in (7, -1, _lib.MAX_GRID_SLOTS, 100):
        with pytest.raises(FxjpsError) as e:
            planner.plan_batch_slots([1, bad], s[:2], g[:2], 2, MPL)
        assert e.value.code == _lib.E_ARG
    with pytest.raises(FxjpsError) as e:
        planner.get_grid_slot(7)
    assert e.value.code == _lib.E_ARG
    with pytest.raises(FxjpsError) as e:
        planner.set_grid_slot(_lib.MAX_GRID_SLOTS, a)
    assert e.value.code == _lib.E_ARG
    res = planner.plan_batch_slots(ids, s, g, 2, MPL)
    # the resident grid's results are untouched by all of it
    assert_same(planner.plan_batch(rs, rg, 2, MPL), before)
    # two contexts on one device: every slot on both, a shard each -- the same bytes
    with fx.Planner([0, 0]) as p2:
        for k, occ in grids.items():
            p2.set_grid_slot(k, occ)
        assert_same(p2.plan_batch_slots(ids, s, g, 2, MPL), res)
        assert np.array_equal(p2.get_grid_slot(2), grids[2])


def test_st_waypoints_on_a_slots_batch_without_explicit_paths(mixed):
    """fxjps_waypoint_st_batch with paths=None after a slots batch reads that batch's paths; its atan2 table must span the
    slots' extents, not the resident grid's -- on a handle without a resident grid, and on one whose resident grid is
    smaller than the slots.  Same bytes as the call given the paths explicitly.  And an empty slots batch needs no ids."""
    import ctypes as C
    import fuxi_planner_amd as fx
    from fuxi_planner_amd import synth, waypoints
    grids, ids, s, g = mixed
    keep = np.isin(ids, [0, 1, 2]) & (s[:, 0] >= 0)
    ids, s, g = ids[keep], s[keep], g[keep]
    n = len(ids)
    pos = np.concatenate([s * 0.1, np.zeros((n, 1))], axis=1)
    goal = np.concatenate([g * 0.1, np.zeros((n, 1))], axis=1)
    for resident in (None, synth.synth_grid(40, 30, 3, 0.1)):
        with fx.Planner([0]) as p:
            for k in (0, 1, 2):
                p.set_grid_slot(k, grids[k])
            if resident is not None:
                p.set_grid_occ(resident)
            else:
                out = np.zeros(1, np.int64)
                assert p._L.fxjps_plan_batch_slots_csr(p._h, None, None, None, 0, 2, 16, out.ctypes.data_as(C.POINTER(C.c_int64)),
                                                       None, 0, None, None, None) == 0, p._L.fxjps_last_error(p._h)
            off, cells, cost, st = p.plan_batch_slots(ids, s, g, 2, MPL)
            assert (st > 0).sum() > n // 2
            a = waypoints.select_st_batch(p, n, (0, 0), 0.1, (0.0, 0.0), pos, goal, nthreads=NTHREADS)
            b = waypoints.select_st_batch(p, n, (0, 0), 0.1, (0.0, 0.0), pos, goal, paths=(off, cells), nthreads=NTHREADS)
            for x, y in zip(a, b):
                assert x.tobytes() == y.tobytes()
