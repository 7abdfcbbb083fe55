"""GPU suite (-m gpu): fxjps_refresh_slots -- fxjps_prepare_slots that keeps the maps of every slot whose prepared grid is
byte for byte what the slot already holds.  The yardstick is a twin handle that runs prepare_slots (which always builds) on
the same jobs: the outputs, the slot's bytes and all six derived arrays are compared for equality after every tick, and the
first tick also with oracle.gridprep.prepare_full and the host reference of the derived maps.  What only this call has --
which jobs report `kept` -- is stated tick by tick.

The fleet is small and mixed: raws of 5 x 7, 33 x 64, 64 x 65 and 100 x 37, one of 513 x 513 (its prepared grid has more
than 2^18 cells: always built), ifa 0, 1 and 2, both variants, both layouts.  The 100 x 37 job has ifa 0 and the ccst
variant, so its prepared grid is the raw itself: 3700 cells, 15 blocks of the gather, the last of them partly filled, and
the raw's last cell is the last cell of that block."""
import ctypes as C

import numpy as np
import pytest

from test_derived_maps_gpu import check_maps
from test_prepare_slots_gpu import _raw_jobs

pytestmark = pytest.mark.gpu
LARGE = 4   # the index of the 513 x 513 job
FLIP = 3    # ... and of the 100 x 37 job


@pytest.fixture(scope="module")
def planner():
    import fuxi_planner_amd as fx
    p = fx.Planner([0])
    yield p
    p.close()


@pytest.fixture(scope="module")
def twin():
    import fuxi_planner_amd as fx
    p = fx.Planner([0])
    yield p
    p.close()


def raw_map(rng, W, H, density=0.15):
    """A random raw whose corners have no obstacle within three cells: a flipped corner cell always changes the prepared grid."""
    m = (rng.random((W, H)) < density).astype(np.uint8)
    m[:3, :3] = 0
    m[-3:, -3:] = 0
    return m


def as_msg(m):
    """raw[x][y] -> (data, width, height) of a nav_msgs/OccupancyGrid: 100 occupied, 0 free, some free cells unknown (-1)."""
    d = np.where(m.T > 0, 100, 0).astype(np.int8)
    d[(m.T == 0) & (np.add.outer(np.arange(m.shape[1]), np.arange(m.shape[0])) % 7 == 3)] = -1
    return (d.reshape(-1), m.shape[0], m.shape[1])


def as_map(job):
    """What map_callback stores for a job's raw: [x][y], 1 = occupied."""
    raw = job[1]
    if isinstance(raw, tuple):
        return (np.asarray(raw[0]).reshape(raw[2], raw[1]).T > 0).astype(np.uint8)
    return (np.asarray(raw) > 0).astype(np.uint8)


def mixed_fleet(first_slot=0):
    rng = np.random.default_rng(760)
    # (sparse where the dilation is wide: 25 offsets at ifa 2 in the ccst variant)
    maps = [raw_map(rng, 5, 7, 0.1), raw_map(rng, 33, 64, 0.02), raw_map(rng, 64, 65, 0.04), raw_map(rng, 100, 37), raw_map(rng, 513, 513, 0.05),
            raw_map(rng, 33, 64, 0.02)]
    s = first_slot
    return [(s + 0, maps[0], (1, 1), (4, 6), 1, 0),
            (s + 1, maps[1], (-3, 2), (30, 60), 2, 1),
            (s + 2, as_msg(maps[2]), (2, 2), (60, 70), 1, 0),
            (s + 3, maps[3], (1, 1), (98, 35), 0, 1),
            (s + 4, maps[4], (2, 2), (510, 509), 0, 1),
            (s + 5, as_msg(maps[5]), (1, -2), (31, 62), 2, 1)]


def with_raw(job, raw):
    return (job[0], raw) + tuple(job[2:])


def with_goal(job, goal):
    return tuple(job[:3]) + (goal,) + tuple(job[4:])


def same_slots(p, other, slots, tag):
    for s in slots:
        assert p.get_grid_slot(s).tobytes() == other.get_grid_slot(s).tobytes(), (tag, s)
        got, want = p.debug_slot_maps(s), other.debug_slot_maps(s)
        assert set(got) == set(want)
        for name in want:
            assert got[name].tobytes() == want[name].tobytes(), (tag, s, name)


def tick(p, other, jobs, kept, tag):
    """One refresh_slots on p, one prepare_slots on the twin: the same outputs, the same slots, and `kept` as stated."""
    outs = p.refresh_slots(jobs)
    want = other.prepare_slots(jobs)
    assert [o[:6] for o in outs] == want, (tag, outs, want)
    assert [o[6] for o in outs] == list(kept), (tag, [o[6] for o in outs])
    same_slots(p, other, [j[0] for j, o in zip(jobs, want) if o[5]], tag)
    return outs


def check_prepared(p, job, out, tag):
    from oracle import gridprep
    eg, es, ego, ed, eeo = gridprep.prepare_full(as_map(job), job[2], job[3], job[4], job[5])
    assert out[:5] == (es, ego, ed, eg.shape, eeo) and out[5], (tag, out, (es, ego, ed, eg.shape, eeo))
    assert np.array_equal(p.get_grid_slot(job[0]), eg), tag
    check_maps(p.debug_slot_maps(job[0]), eg, tag)
    return eg


def test_ticks(planner, twin):
    jobs = mixed_fleet()
    n = len(jobs)
    but_large = [v != LARGE for v in range(n)]
    # 1. empty slots: everything is built
    outs = tick(planner, twin, jobs, [False] * n, "tick 1")
    shapes = [o[3][0] * o[3][1] for o in outs]
    assert shapes[LARGE] > 1 << 18 and max(s for v, s in enumerate(shapes) if v != LARGE) <= 1 << 18 and outs[FLIP][3] == (100, 37)
    for job, o in zip(jobs, outs):
        check_prepared(planner, job, o, ("tick 1", job[0]))
    # 2. the same jobs again: every slot keeps its maps, the large one is built
    assert [o[:6] for o in tick(planner, twin, jobs, but_large, "tick 2")] == [o[:6] for o in outs]
    for flip in ((0, 0), (99, 36)):
        # 3. one raw cell flipped in one job: that job alone is built
        raw = jobs[FLIP][1].copy()
        raw[flip] ^= 1
        before = planner.get_grid_slot(jobs[FLIP][0])
        jobs[FLIP] = with_raw(jobs[FLIP], raw)
        o3 = tick(planner, twin, jobs, [v not in (LARGE, FLIP) for v in range(n)], ("tick 3", flip))
        eg = check_prepared(planner, jobs[FLIP], o3[FLIP], ("tick 3", flip))
        diff = np.flatnonzero(eg.reshape(-1) != before.reshape(-1))
        assert diff.tolist() == [0 if flip == (0, 0) else eg.size - 1]  # (the first thread of the first block / the last of the last)
        # 4. tick 3's jobs again: the flag of the call before is not seen
        tick(planner, twin, jobs, but_large, ("tick 4", flip))
    # end to end after a mixed tick: the batch over all slots is the twin's
    ids = np.array([j[0] for j in jobs], np.int32)
    starts, goals = [o[0] for o in o3], [o[1] for o in o3]
    got, want = planner.plan_batch_slots(ids, starts, goals, 2), twin.plan_batch_slots(ids, starts, goals, 2)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(got, want)) and (got[3] > 0).sum() >= 3, got[3]
    # 5. the goal moved onto an obstacle of an unchanged map: kept, and goal_xy / end_occu follow the new goal
    m = as_map(jobs[1])
    x, y = [int(c) for c in np.argwhere(m[5:-5, 5:-5] == 1)[0] + 5]
    jobs[1] = with_goal(jobs[1], (x, y))
    o5 = tick(planner, twin, jobs, but_large, "tick 5")
    check_prepared(planner, jobs[1], o5[1], "tick 5")
    dx, dy = o5[1][2]
    assert o5[1][1] != (x + dx, y + dy) and o5[1][1] != o3[1][1] and o5[1][4] == 1, (o5[1], o3[1])


def test_extents_swapped_and_padding_shifted(planner, twin):
    free = lambda W, H: np.zeros((W, H), np.uint8)
    # the bytes are equal (all free), the extents are not
    tick(planner, twin, [(20, free(40, 60), (1, 1), (5, 5), 0, 1)], [False], "40 x 60")
    tick(planner, twin, [(20, free(40, 60), (1, 1), (5, 5), 0, 1)], [True], "40 x 60 again")
    o = tick(planner, twin, [(20, free(60, 40), (1, 1), (5, 5), 0, 1)], [False], "60 x 40")
    assert o[0][3] == (60, 40)
    # the padding moves by one cell, the extents stay
    rng = np.random.default_rng(761)
    W0 = 30
    for slot, raw, kept in ((21, raw_map(rng, W0, 20, 0.05), False), (22, free(W0, 20), True)):
        a = (slot, raw, (-1, 3), (W0, 10), 1, 1)
        b = (slot, raw, (0, 3), (W0 + 1, 10), 1, 1)
        oa = tick(planner, twin, [a], [False], ("padding a", slot))
        ob = tick(planner, twin, [b], [kept], ("padding b", slot))
        assert oa[0][3] == ob[0][3] == (W0 + 7, 26) and oa[0][2] == (3, 2) and ob[0][2] == (2, 2), (oa, ob)
        check_prepared(planner, b, ob[0], ("padding b", slot))


def test_slots_filled_by_other_calls(planner, twin):
    from oracle import gridprep
    from fuxi_planner_amd import _lib
    rng = np.random.default_rng(762)
    job = (24, raw_map(rng, 50, 45, 0.04), (2, 2), (40, 40), 1, 1)
    eg = gridprep.prepare_full(as_map(job), job[2], job[3], job[4], job[5])[0].astype(np.uint8)
    assert eg.max() == 1
    # set_grid_slot of exactly the prepared bytes: kept, and the slot plans
    planner.set_grid_slot(24, eg)
    o = tick(planner, twin, [job], [True], "set_grid_slot")
    got, want = (p.plan_batch_slots([24], [o[0][0]], [o[0][1]], 2) for p in (planner, twin))
    assert all(x.tobytes() == y.tobytes() for x, y in zip(got, want)) and got[3][0] > 0
    # byte 7 where the prepared byte is 1 (through the C call: set_grid_slot of the binding writes 0 / 1): built, reads back 1
    seven = np.ascontiguousarray(eg * 7)
    planner._chk(planner._L.fxjps_set_grid_slot(planner._h, 24, _lib.ptr(seven, C.c_uint8), eg.shape[0], eg.shape[1]))
    assert planner.get_grid_slot(24).max() == 7
    tick(planner, twin, [job], [False], "byte 7")
    assert np.array_equal(planner.get_grid_slot(24), eg)
    tick(planner, twin, [job], [True], "byte 7 again")
    # cleared: built
    planner.clear_grid_slot(24)
    tick(planner, twin, [job], [False], "cleared")
    check_prepared(planner, job, planner.refresh_slots([job])[0][:6], "cleared, again")


def test_failing_job_on_two_ticks_running(planner, twin):
    from fuxi_planner_amd import FxjpsError, _lib
    rng = np.random.default_rng(763)
    cross = np.zeros((5, 4), np.uint8)
    cross[2, :] = 1
    cross[:, 1] = 1
    jobs = [(30, raw_map(rng, 20, 31, 0.05), (1, 1), (15, 25), 1, 0), (31, cross, (0, 0), (2, 1), 0, 1), (32, raw_map(rng, 44, 9, 0.02), (1, 1), (40, 7), 2, 1)]
    planner.set_grid_slot(31, np.zeros((5, 4), np.uint8))  # (a grid of the failing job's extents: compared, and empty afterwards)
    for kept in ([False] * 3, [True, False, True]):
        outs = tick(planner, twin, jobs, kept, ("failing", kept))
        assert [o[5] for o in outs] == [True, False, True]
        with pytest.raises(FxjpsError) as e:
            planner.get_grid_slot(31)
        assert e.value.code == _lib.E_ARG
    # the status as the C call reports it
    arr, keep = planner._slot_jobs(jobs)
    flags = np.full(3, -5, np.int32)
    assert planner._L.fxjps_refresh_slots(planner._h, arr, 3, _lib.ptr(flags, C.c_int32)) == 0
    assert [j.status for j in arr] == [0, _lib.E_ARG, 0] and flags.tolist() == [1, 0, 1]


def test_refusals_change_nothing(planner):
    from fuxi_planner_amd import _lib
    rng = np.random.default_rng(764)
    held = {200: (rng.random((40, 30)) < 0.15).astype(np.uint8), 201: (rng.random((25, 60)) < 0.15).astype(np.uint8)}
    jobs = [(k, raw, (1, 1), (20, 20), 1, k & 1) for k, raw in held.items()]
    outs = planner.refresh_slots(jobs)
    ids = np.array(list(held), np.int32)
    starts, goals = [o[0] for o in outs], [o[1] for o in outs]
    grids = {k: planner.get_grid_slot(k) for k in held}
    maps = {k: planner.debug_slot_maps(k) for k in held}
    plan = planner.plan_batch_slots(ids, starts, goals, 2)
    L, h = planner._L, planner._h
    flags = np.full(_lib.MAX_GRID_SLOTS + 1, -5, np.int32)
    out_kept = _lib.ptr(flags, C.c_int32)
    good = {"slot": 200, "raw": np.ones((6, 5), np.uint8)}  # (job 0 of every refused call would overwrite slot 200)
    # every refusal of fxjps_prepare_slots (tests/test_prepare_slots_gpu.py)
    bad = [{"slot": -1}, {"slot": _lib.MAX_GRID_SLOTS}, {"slot": 200}, {"slot": 201, "null_raw": True}, {"slot": 201, "W0": 0},
           {"slot": 201, "H0": -3}, {"slot": 201, "ifa": -1}, {"slot": 201, "ifa": 65}, {"slot": 201, "variant": 2},
           {"slot": 201, "layout": 2}, {"slot": 201, "raw": np.zeros((8000, 2), np.uint8), "ifa": 64},
           {"slot": 201, "start": (-8100, 0), "goal": (100, 0)}, {"slot": 201, "ifa": 0, "variant": 0, "goal": (0, 2)},
           {"slot": 201, "ifa": 0, "variant": 1, "goal": (6, 2)}]
    for sp in bad:
        arr, keep = _raw_jobs([good, sp])
        assert L.fxjps_refresh_slots(h, arr, 2, out_kept) == _lib.E_ARG, sp
        assert b"job 1" in L.fxjps_last_error(h), (sp, L.fxjps_last_error(h))
    arr, keep = _raw_jobs([{"slot": s} for s in range(_lib.MAX_GRID_SLOTS)] + [{"slot": 0}])
    for n in (-1, _lib.MAX_GRID_SLOTS + 1):
        assert L.fxjps_refresh_slots(h, arr, n, out_kept) == _lib.E_ARG, n
    assert L.fxjps_refresh_slots(h, None, 1, out_kept) == _lib.E_ARG
    assert L.fxjps_refresh_slots(h, None, 0, out_kept) == 0  # (an empty call is no error, and does nothing)
    assert (flags == -5).all()
    for k in held:
        assert np.array_equal(planner.get_grid_slot(k), grids[k]), k
        now = planner.debug_slot_maps(k)
        assert all(now[name].tobytes() == maps[k][name].tobytes() for name in now), k
    again = planner.plan_batch_slots(ids, starts, goals, 2)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(again, plan))
    # out_kept = NULL: the call runs, and the slots are kept all the same (the next call says so)
    arr, keep = planner._slot_jobs(jobs)
    assert L.fxjps_refresh_slots(h, arr, 2, None) == 0
    assert [o[:6] for o in planner._slot_outs(arr, 2)] == [o[:6] for o in outs]
    assert [o[6] for o in planner.refresh_slots(jobs)] == [True, True]
    for k in held:
        assert np.array_equal(planner.get_grid_slot(k), grids[k]), k


def same_value(a, b):
    if isinstance(a, np.ndarray) or isinstance(b, np.ndarray):
        return isinstance(a, np.ndarray) and isinstance(b, np.ndarray) and a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()
    if isinstance(a, (list, tuple)):
        return isinstance(b, (list, tuple)) and len(a) == len(b) and all(same_value(x, y) for x, y in zip(a, b))
    if isinstance(a, float) and isinstance(b, float):
        return np.float64(a).tobytes() == np.float64(b).tobytes()
    return type(a) is type(b) and a == b


def test_fleet_tick_with_refresh(planner, twin):
    """Planner.fleet_tick_refresh over three ticks against Planner.fleet_tick on the twin, record by record.  (A sibling
    method, not a flag of fleet_tick: tests/test_tick_outputs_host.py pins fleet_tick's parameter list.)"""
    jobs = [(40 + v,) + tuple(j[1:]) for v, j in enumerate(mixed_fleet()) if v != LARGE]
    cross = np.zeros((5, 4), np.uint8)
    cross[2, :] = 1
    cross[:, 1] = 1
    jobs.insert(2, (49, cross, (0, 0), (2, 1), 0, 1))
    n = len(jobs)
    reso, map_o = 0.25, (-2.0, 1.0)
    pos = np.array([[reso * j[2][0] - 2.0, reso * j[2][1] + 1.0, 1.0] for j in jobs])
    goals = np.array([[reso * j[3][0] - 2.0, reso * j[3][1] + 1.0, 1.5 + 0.25 * (v % 3)] for v, j in enumerate(jobs)])
    home = np.array([[-2.0 + 0.5 * v, 1.0] for v in range(n)])
    live = [v for v in range(n) if v != 2]
    for t in range(3):
        if t == 2:  # a new map for one vehicle
            raw = jobs[4][1].copy()
            raw[50, 20] ^= 1
            jobs[4] = with_raw(jobs[4], raw)
        recs = planner.fleet_tick_refresh(jobs, pos, goals, home, reso, map_o, publish=True, image_channels=1)
        want = twin.fleet_tick(jobs, pos, goals, home, reso, map_o, publish=True, image_channels=1)
        assert len(recs) == len(want) == n
        for v in range(n):
            assert ("kept" in recs[v]) == (v in live) and "kept" not in want[v], (t, v)
            assert set(recs[v]) - {"kept"} == set(want[v])
            for k in want[v]:
                assert same_value(recs[v][k], want[v][k]), (t, v, k, recs[v][k], want[v][k])
        assert recs[2]["ok"] is False and sum(r["status"] > 0 for r in recs if r["ok"]) >= 3
        assert [recs[v]["kept"] for v in live] == [t == 1 or (t == 2 and v != 4) for v in live], t


def test_two_contexts(twin):
    import fuxi_planner_amd as fx
    jobs = mixed_fleet(60)
    n = len(jobs)

    def both_contexts(p2, tag):
        for j in jobs:
            s = j[0]
            want_occ, want = twin.get_grid_slot(s), twin.debug_slot_maps(s)
            for c in (0, 1):
                occ, got = p2.debug_slot_context(c, s)
                assert occ.tobytes() == want_occ.tobytes(), (tag, c, s)
                for name in want:
                    assert got[name].tobytes() == want[name].tobytes(), (tag, c, s, name)

    with fx.Planner([0, 0]) as p2:
        tick(p2, twin, jobs, [False] * n, "two contexts, tick 1")
        both_contexts(p2, "tick 1")
        tick(p2, twin, jobs, [v != LARGE for v in range(n)], "two contexts, tick 2")
        both_contexts(p2, "tick 2")
        raw = jobs[FLIP][1].copy()
        raw[99, 36] ^= 1
        jobs[FLIP] = with_raw(jobs[FLIP], raw)
        outs = tick(p2, twin, jobs, [v not in (LARGE, FLIP) for v in range(n)], "two contexts, tick 3")
        both_contexts(p2, "tick 3")
        ids = np.array([j[0] for j in jobs], np.int32)
        starts, goals = [o[0] for o in outs], [o[1] for o in outs]
        got, want = p2.plan_batch_slots(ids, starts, goals, 2), twin.plan_batch_slots(ids, starts, goals, 2)
        assert all(x.tobytes() == y.tobytes() for x, y in zip(got, want))
        per = [t["queries"] for t in p2.timing_per_context()]
        assert sum(per) == n and min(per) > 0, per  # (both contexts' slots served a shard)
