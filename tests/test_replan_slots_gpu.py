"""GPU suite (-m gpu): fxjps_replan_slots -- fxjps_plan_batch_slots_csr that hands back the stored path of every query whose
slot, start and goal did not change since the previous such call.  The yardstick is a twin handle that gets the same slot
calls and runs fxjps_plan_batch_slots_csr with the same arguments: after every tick the offsets, lengths, costs, cells,
fxjps_last_cells and every output of fxjps_tick_outputs_slots on the resident paths are compared byte for byte, and the
first tick's paths also with the CPU oracle.  What only this call has -- which queries report `reused`, and
fxjps_timing_t.reused -- is stated tick by tick.

The fleet: 7 slots, raws of 5 x 7 up to 40 x 37 and one of 130 x 70 whose walls force a path of many jump points, ifa 0 to 2,
both variants.  11 queries: one per vehicle, a second one on slot 3, one whose start is its goal, one whose goal is walled in
(NOPATH), one whose start is off its grid (BAD_START); the batch's max_path_len is the longest of the other paths, so the
130 x 70 vehicle's is PATH_TOO_LONG."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NV = 7            # vehicles = slots
SHARED = 3        # the slot with two queries (q3 and q7); tick 5 flips a cell of its raw
SAME, WALLED, OFF, LONG = 8, 9, 10, 6  # queries: start == goal (slot 1), NOPATH (slot 5), BAD_START (slot 2), PATH_TOO_LONG (slot 6)
QSLOT = [0, 1, 2, 3, 4, 5, 6, SHARED, 1, 5, 2]
NQ = len(QSLOT)
RESO, MAP_O = 0.25, (-2.0, 1.0)


def raw_map(rng, W, H, density):
    m = (rng.random((W, H)) < density).astype(np.uint8)
    m[:3, :3] = 0
    m[-3:, -3:] = 0
    return m


def fleet():
    """-> jobs as Planner.prepare_slots takes them: (slot, raw [x][y], start, goal, ifa, variant)."""
    rng = np.random.default_rng(770)
    maps = [raw_map(rng, 5, 7, 0.1), raw_map(rng, 12, 9, 0.1), raw_map(rng, 21, 17, 0.03), raw_map(rng, 33, 20, 0.06), raw_map(rng, 40, 37, 0.02),
            raw_map(rng, 17, 30, 0.08), np.zeros((130, 70), np.uint8)]
    maps[5][7:12, 12:17] = 0
    maps[5][8:11, 13:16] = 1
    maps[5][9, 14] = 0  # (a free cell inside a closed ring: WALLED's goal)
    for k, x in enumerate(range(10, 130, 10)):  # walls with a gap at alternating ends: a path of two jump points per wall
        maps[6][x, :] = 1
        if k % 2:
            maps[6][x, :4] = 0
        else:
            maps[6][x, -4:] = 0
    return [(0, maps[0], (1, 1), (4, 6), 1, 0), (1, maps[1], (1, 1), (10, 7), 0, 1), (2, maps[2], (-2, 1), (19, 15), 2, 1),
            (3, maps[3], (1, 1), (31, 18), 1, 1), (4, maps[4], (1, 1), (38, 35), 2, 0), (5, maps[5], (1, 1), (15, 28), 0, 1),
            (6, maps[6], (1, 1), (128, 68), 0, 1)]


def prepared(jobs):
    """The CPU's prepared grid, start, goal, map_d and end_occu of every job."""
    from oracle import gridprep
    return [gridprep.prepare_full(np.asarray(j[1]), j[2], j[3], j[4], j[5]) for j in jobs]


def queries(prep):
    """-> (ids, starts, goals) of the 11 queries, in prepared-grid cells."""
    starts = [tuple(p[1]) for p in prep]
    goals = [tuple(p[2]) for p in prep]
    g3 = prep[SHARED][0]
    free = [tuple(int(v) for v in c) for c in np.argwhere(g3 == 0)]
    starts.append(next(c for c in free if c != starts[SHARED] and c[0] > 8 and c[1] > 8))  # q7: the shared slot, another start
    goals.append(goals[SHARED])
    starts.append(starts[1])  # SAME
    goals.append(starts[1])
    d5 = prep[5][3]
    starts.append(starts[5])  # WALLED
    goals.append((9 + d5[0], 14 + d5[1]))
    starts.append((prep[2][0].shape[0] + 1, 0))  # OFF
    goals.append(goals[2])
    return np.array(QSLOT, np.int32), np.array(starts, np.int32), np.array(goals, np.int32)


def oracle_batch(grids, ids, starts, goals, hchoice, max_len):
    """The CPU oracle, query by query on the grid of its slot -> (list of cells [len, 2], len int32[nq], cost float64[nq])."""
    from oracle import oracle
    cells, ln, cost = [], np.zeros(len(ids), np.int32), np.zeros(len(ids))
    for q, s in enumerate(ids):
        c, l, k, _ = oracle.plan_batch(grids[int(s)], starts[q:q + 1], goals[q:q + 1], hchoice, literal=False, max_len=max_len)
        ln[q], cost[q] = l[0], k[0]
        cells.append(c[0, :max(int(l[0]), 0)].copy())
    return cells, ln, cost


def path_len_bound(grids, ids, starts, goals):
    """The batch's max_path_len: the longest path of every query but LONG, whose own path is longer."""
    _, ln, _ = oracle_batch(grids, ids, starts, goals, 2, 512)
    others = [int(ln[q]) for q in range(len(ids)) if q != LONG]
    assert ln[LONG] > max(others) >= 3, ln
    return max(others)


def moved_start(grid, start, goal, max_len):
    """A free cell next to `start` from which the oracle still finds a path."""
    from oracle import oracle
    for dx, dy in ((1, 0), (0, 1), (1, 1), (-1, 0), (0, -1), (-1, -1), (1, -1), (-1, 1)):
        c = np.array([[int(start[0]) + dx, int(start[1]) + dy]], np.int32)
        if grid[c[0, 0], c[0, 1]] == 0 and oracle.plan_batch(grid, c, np.array([goal], np.int32), 2, literal=False, max_len=max_len)[1][0] > 0:
            return c[0]
    raise AssertionError("no neighbour of the start has a path")


def flip_on_path(job, prep, path):
    """A raw cell of `job` that is free, lies under an inner jump point of `path` (prepared-grid cells), and whose flip to
    occupied leaves the job's prepared start and goal as they are -> (raw with the cell flipped, the jump point)."""
    from oracle import gridprep
    grid, s, g, d, eo = prep
    for jx, jy in path[1:-1]:
        rx, ry = int(jx) - d[0], int(jy) - d[1]
        raw = np.asarray(job[1])
        if not (0 <= rx < raw.shape[0] and 0 <= ry < raw.shape[1]) or raw[rx, ry]:
            continue
        new = raw.copy()
        new[rx, ry] = 1
        g2, s2, go2, d2, eo2 = gridprep.prepare_full(new, job[2], job[3], job[4], job[5])
        if (tuple(s2), tuple(go2), tuple(d2), eo2) == (tuple(s), tuple(g), tuple(d), eo) and g2[int(jx), int(jy)] == 1 and g2[tuple(s)] == 0:
            return new, (int(jx), int(jy))
    raise AssertionError("no inner jump point of the path can be flipped")


class Handle(object):
    """One planner and the raw C calls of a tick on it."""

    def __init__(self, devices=(0,)):
        import fuxi_planner_amd as fx
        self.p = fx.Planner(list(devices))

    def close(self):
        self.p.close()

    def batch(self, replan, ids, starts, goals, hchoice, mpl):
        """-> (rc, {offsets, len, cost, cells, last_cells} as bytes-comparable arrays, reused int32[nq] | None)"""
        from fuxi_planner_amd import _lib
        p = self.p
        n = len(ids)
        ids, starts, goals = (np.ascontiguousarray(a, np.int32) for a in (ids, starts, goals))
        off, ln, cost = np.full(n + 1, -7, np.int64), np.full(n, -7, np.int32), np.full(n, -7.0)
        cap = n * mpl
        cells = np.full((cap, 2), -7, np.int32)
        reused = np.full(n, -7, np.int32)
        secs = C.c_double(0.0)
        head = (p._h, _lib.ptr(ids, C.c_int32), _lib.ptr(starts, C.c_int32), _lib.ptr(goals, C.c_int32), n, hchoice, mpl, _lib.ptr(off, C.c_int64),
                _lib.ptr(cells, C.c_int32), cap, _lib.ptr(ln, C.c_int32), _lib.ptr(cost, C.c_double))
        if replan:
            rc = p._L.fxjps_replan_slots(*(head + (_lib.ptr(reused, C.c_int32), C.byref(secs))))
        else:
            rc = p._L.fxjps_plan_batch_slots_csr(*(head + (C.byref(secs),)))
        if rc != 0:
            return rc, None, reused
        total = int(off[n])
        last = np.full((max(total, 1), 2), -7, np.int32)
        if total > 0:
            p._chk(p._L.fxjps_last_cells(p._h, _lib.ptr(last, C.c_int32), total))
        return rc, {"offsets": off, "len": ln, "cost": cost, "cells": cells[:total].copy(), "last_cells": last[:total]}, reused

    def tick_outputs(self, offsets, tick_args):
        from fuxi_planner_amd import waypoints
        return waypoints.tick_outputs_slots(self.p, *tick_args, offsets=offsets, return_kept=True)


def flat(x):
    if isinstance(x, (list, tuple)):
        return b"|".join(flat(v) for v in x)
    return np.ascontiguousarray(x).tobytes()


class Fleet(object):
    """Both handles, the jobs and the queries of the ticks."""

    def __init__(self):
        self.a, self.b = Handle(), Handle()
        self.jobs = fleet()
        self.prep = prepared(self.jobs)
        self.grids = {j[0]: np.ascontiguousarray(p[0] == 1, dtype=np.uint8) for j, p in zip(self.jobs, self.prep)}
        self.ids, self.starts, self.goals = queries(self.prep)
        self.mpl = path_len_bound(self.grids, self.ids, self.starts, self.goals)
        # what fxjps_tick_outputs_slots needs per query: its vehicle's rule, map_start, shifted origin, pose, goal, home, end_occu
        from fuxi_planner_amd import Planner
        v = [int(s) for s in self.ids]
        origin = [Planner.shifted_origin(MAP_O, self.prep[s][3], RESO) for s in v]
        pos = np.array([[RESO * self.jobs[s][2][0] - 2.0, RESO * self.jobs[s][2][1] + 1.0, 1.0] for s in v])
        goal = np.array([[RESO * self.jobs[s][3][0] - 2.0, RESO * self.jobs[s][3][1] + 1.0, 1.5 + 0.25 * (q % 3)] for q, s in enumerate(v)])
        home = np.array([[-2.0 + 0.5 * q, 1.0] for q in range(len(v))])
        self.tick_args = lambda n: ([self.jobs[s][5] for s in v[:n]], [self.prep[s][1] for s in v[:n]], RESO, origin[:n], pos[:n], goal[:n], home[:n],
                                    [self.prep[s][4] for s in v[:n]])

    def close(self):
        self.a.close()
        self.b.close()

    def slots_call(self, name, *args):
        """The same slot call on both handles -> the first handle's result."""
        out = getattr(self.a.p, name)(*args)
        getattr(self.b.p, name)(*args)
        return out

    def tick(self, tag, want_reused, ids=None, starts=None, goals=None, hchoice=2, mpl=None):
        """fxjps_replan_slots on the first handle, fxjps_plan_batch_slots_csr on the twin: equal bytes, and `reused` as stated."""
        ids = self.ids if ids is None else ids
        starts = self.starts if starts is None else starts
        goals = self.goals if goals is None else goals
        mpl = self.mpl if mpl is None else mpl
        n = len(ids)
        rc, got, reused = self.a.batch(True, ids, starts, goals, hchoice, mpl)
        rcb, want, _ = self.b.batch(False, ids, starts, goals, hchoice, mpl)
        assert rc == rcb == 0, (tag, rc, rcb, self.a.p._L.fxjps_last_error(self.a.p._h))
        for k in want:
            assert got[k].tobytes() == want[k].tobytes(), (tag, k, got[k], want[k])
        assert got["cells"].tobytes() == got["last_cells"].tobytes(), tag
        want_reused = [bool(r) for r in (want_reused if not isinstance(want_reused, bool) else [want_reused] * n)]
        T = self.a.p.timing()
        assert reused.tolist() == [int(r) for r in want_reused], (tag, reused.tolist())
        assert T["reused"] == sum(want_reused), (tag, T)
        if all(want_reused):
            assert T["search_launches"] == 0 and T["pops"] == 0 and T["pushes"] == 0, (tag, T)
        else:
            assert T["search_launches"] >= 1, (tag, T)
        oa, ob = self.a.tick_outputs(got["offsets"], self.tick_args(n)), self.b.tick_outputs(want["offsets"], self.tick_args(n))
        assert len(oa) == len(ob) == 10
        for i, (x, y) in enumerate(zip(oa, ob)):
            assert flat(x) == flat(y), (tag, "tick output", i)
        return got


def on_slots(slots):
    return [s not in slots for s in QSLOT]


@pytest.fixture(scope="module")
def fl():
    f = Fleet()
    yield f
    f.close()


def test_ticks(fl):
    from fuxi_planner_amd import _lib
    outs = fl.slots_call("prepare_slots", fl.jobs)
    for o, p, j in zip(outs, fl.prep, fl.jobs):
        assert o[:5] == (tuple(p[1]), tuple(p[2]), tuple(p[3]), p[0].shape, p[4]) and o[5], (j[0], o)
    for h in (fl.a, fl.b):  # (a resident grid of its own: tick 10 plans on it)
        h.p.set_grid_occ(fl.grids[1])
    # 1. the first call: nothing is reused; the paths are the oracle's
    t1 = fl.tick("tick 1", False)
    cells, ln, cost = oracle_batch(fl.grids, fl.ids, fl.starts, fl.goals, 2, fl.mpl)
    assert t1["len"].tolist() == ln.tolist() and t1["cost"].tobytes() == cost.tobytes(), (t1["len"], ln)
    for q in range(NQ):
        assert np.array_equal(t1["cells"][t1["offsets"][q]:t1["offsets"][q + 1]], cells[q]), q
    assert ln[LONG] == _lib.Q_PATH_TOO_LONG and ln[WALLED] == _lib.Q_NOPATH and ln[OFF] == _lib.Q_BAD_START, ln
    assert (ln[:LONG] > 0).all() and ln[7] > 0 and ln[SAME] >= 0 and max(ln) == fl.mpl, ln
    assert len({int(o) & 1 for o in t1["offsets"][:-1]}) == 2  # (paths at even and at odd offsets)
    # 2. the same call again: everything is reused (no query is CAPACITY), nothing is launched
    assert (t1["len"] != _lib.Q_CAPACITY).all()
    fl.tick("tick 2", True)
    # 3. one vehicle's start moved by one cell: that query alone is searched
    fl.starts = fl.starts.copy()
    fl.starts[4] = moved_start(fl.grids[4], fl.starts[4], fl.goals[4], fl.mpl)
    t3 = fl.tick("tick 3", [q != 4 for q in range(NQ)])
    assert t3["len"][4] > 0
    # 4. refresh_slots with identical raws: every slot is kept, everything is reused
    assert [o[6] for o in fl.slots_call("refresh_slots", fl.jobs)] == [True] * NV
    t4 = fl.tick("tick 4", True)
    # 5. a raw cell under an inner jump point of q3's stored path becomes occupied: the slot is rebuilt, its queries are searched
    lo, hi = int(t4["offsets"][SHARED]), int(t4["offsets"][SHARED + 1])
    old = t4["cells"][lo:hi].copy()
    assert np.array_equal(old, oracle_batch(fl.grids, fl.ids[SHARED:SHARED + 1], fl.starts[SHARED:SHARED + 1], fl.goals[SHARED:SHARED + 1], 2, fl.mpl)[0][0])
    new_raw, jp = flip_on_path(fl.jobs[SHARED], fl.prep[SHARED], old)
    fl.jobs[SHARED] = (fl.jobs[SHARED][0], new_raw) + tuple(fl.jobs[SHARED][2:])
    fl.prep[SHARED] = prepared([fl.jobs[SHARED]])[0]
    fl.grids[SHARED] = np.ascontiguousarray(fl.prep[SHARED][0] == 1, dtype=np.uint8)
    assert fl.grids[SHARED][tuple(int(v) for v in fl.starts[7])] == 0  # (q7's start stays free)
    want = oracle_batch(fl.grids, fl.ids[SHARED:SHARED + 1], fl.starts[SHARED:SHARED + 1], fl.goals[SHARED:SHARED + 1], 2, fl.mpl)
    assert not any((c == jp).all() for c in want[0][0])  # (the path must change: its jump point is occupied)
    assert [o[6] for o in fl.slots_call("refresh_slots", fl.jobs)] == [v != SHARED for v in range(NV)]
    t5 = fl.tick("tick 5", on_slots({SHARED}))
    new = t5["cells"][int(t5["offsets"][SHARED]):int(t5["offsets"][SHARED + 1])]
    assert new.tobytes() != old.tobytes() and t5["len"][SHARED] == want[1][0] and (want[1][0] <= 0 or np.array_equal(new, want[0][0])), (old, new)
    # 6. the same again: everything is reused (the generation was recorded after the rebuild)
    assert [o[6] for o in fl.slots_call("refresh_slots", fl.jobs)] == [True] * NV
    fl.tick("tick 6", True)
    # 7. prepare_slots with identical raws always builds: the queries of every slot it names are searched
    fl.slots_call("prepare_slots", [fl.jobs[0], fl.jobs[2]])
    fl.tick("tick 7", on_slots({0, 2}))
    # 8. set_grid_slot on one slot between two calls: its queries are searched
    fl.slots_call("set_grid_slot", 1, fl.grids[1])
    fl.tick("tick 8", on_slots({1}))
    # 9. a changed hchoice, then a changed max_path_len, then a changed nq: nothing is reused
    fl.tick("tick 9 hchoice", False, hchoice=1)
    t9 = fl.tick("tick 9 max_path_len", False, hchoice=1, mpl=256)
    assert t9["len"][LONG] > fl.mpl
    fl.tick("tick 9 nq", False, fl.ids[:-1], fl.starts[:-1], fl.goals[:-1], hchoice=1, mpl=256)
    fl.tick("tick 9 again", True, fl.ids[:-1], fl.starts[:-1], fl.goals[:-1], hchoice=1, mpl=256)
    # 10. another batch call in between drops the stored results
    fl.tick("tick 10 before", False)
    rc, plain, _ = fl.a.batch(False, fl.ids, fl.starts, fl.goals, 2, fl.mpl)
    assert rc == 0
    t10 = fl.tick("tick 10 after plan_batch_slots_csr", False)
    assert all(plain[k].tobytes() == t10[k].tobytes() for k in plain)
    fl.tick("tick 10 again", True)
    s, g = np.array([[1, 1]], np.int32), np.array([[10, 7]], np.int32)
    fl.a.p.plan_batch(s, g, 2, 64)
    fl.tick("tick 10 after plan_batch", False)
    # 11. a released slot named by a query: refused, nothing queued, and the stored results survive
    fl.slots_call("clear_grid_slot", 0)
    rc, _, reused = fl.a.batch(True, fl.ids, fl.starts, fl.goals, 2, fl.mpl)
    assert rc == _lib.E_ARG and b"slot 0" in fl.a.p._L.fxjps_last_error(fl.a.p._h) and (reused == -7).all()
    assert fl.b.batch(False, fl.ids, fl.starts, fl.goals, 2, fl.mpl)[0] == _lib.E_ARG
    ids, starts, goals = fl.ids.copy(), fl.starts.copy(), fl.goals.copy()
    ids[0], starts[0], goals[0] = ids[1], starts[1], goals[1]
    fl.tick("tick 11", [q != 0 for q in range(NQ)], ids, starts, goals)
    # ... and refusals of the arguments leave them too
    assert fl.a.batch(True, ids, starts, goals, 3, fl.mpl)[0] == _lib.E_ARG
    assert fl.a.batch(True, ids, starts, goals, 2, 0)[0] == _lib.E_ARG
    fl.tick("tick 11 again", True, ids, starts, goals)


def reuse_off_main():
    """Tick 12, run in a process of its own (the library reads FXJPS_REPLAN_REUSE once): nothing is reused, the bytes are equal."""
    f = Fleet()
    f.slots_call("prepare_slots", f.jobs)
    f.tick("reuse off 1", False)
    f.tick("reuse off 2", False)
    f.close()
    print("reuse-off ok")


def test_reuse_turned_off_by_the_environment():
    env = dict(os.environ, FXJPS_REPLAN_REUSE="0", PYTHONPATH=os.pathsep.join([ROOT, os.path.join(ROOT, "tests")]))
    r = subprocess.run([sys.executable, "-c", "import test_replan_slots_gpu as t; t.reuse_off_main()"], env=env, cwd=ROOT, capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 0 and "reuse-off ok" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])


def test_two_contexts(fl):
    """A handle with two contexts on device 0 runs the call as a plain slots batch: reused is 0, the bytes are the twin's."""
    jobs = fleet()
    prep = prepared(jobs)
    ids, starts, goals = queries(prep)
    grids = {j[0]: np.ascontiguousarray(p[0] == 1, dtype=np.uint8) for j, p in zip(jobs, prep)}
    mpl = path_len_bound(grids, ids, starts, goals)
    h2 = Handle((0, 0))
    try:
        h2.p.prepare_slots(jobs)
        fl.b.p.prepare_slots(jobs)
        rcb, want, _ = fl.b.batch(False, ids, starts, goals, 2, mpl)
        assert rcb == 0
        for t in range(2):
            rc, got, reused = h2.batch(True, ids, starts, goals, 2, mpl)
            assert rc == 0 and (reused == 0).all() and h2.p.timing()["reused"] == 0, (t, reused)
            for k in want:
                assert got[k].tobytes() == want[k].tobytes(), (t, k)
    finally:
        h2.close()


def test_fleet_tick_refresh_with_reuse(fl):
    """Planner.fleet_tick_refresh(reuse=True) on two ticks running: the records of reuse=False on the twin, plus `reused`."""
    from test_refresh_slots_gpu import same_value
    jobs = [(40 + j[0],) + tuple(j[1:]) for j in fleet()]
    n = len(jobs)
    pos = np.array([[RESO * j[2][0] - 2.0, RESO * j[2][1] + 1.0, 1.0] for j in jobs])
    goals = np.array([[RESO * j[3][0] - 2.0, RESO * j[3][1] + 1.0, 1.5 + 0.25 * (v % 3)] for v, j in enumerate(jobs)])
    home = np.array([[-2.0 + 0.5 * v, 1.0] for v in range(n)])
    for t in range(2):
        recs = fl.a.p.fleet_tick_refresh(jobs, pos, goals, home, RESO, MAP_O, publish=True, image_channels=1, reuse=True)
        want = fl.b.p.fleet_tick_refresh(jobs, pos, goals, home, RESO, MAP_O, publish=True, image_channels=1)
        assert len(recs) == len(want) == n
        for v in range(n):
            assert set(recs[v]) - {"reused"} == set(want[v]) and "reused" not in want[v] and recs[v]["ok"], (t, v)
            for k in want[v]:
                assert same_value(recs[v][k], want[v][k]), (t, v, k, recs[v][k], want[v][k])
        assert [r["reused"] for r in recs] == [t == 1] * n and [r["kept"] for r in recs] == [t == 1] * n, (t, recs)
        assert sum(r["status"] > 0 for r in recs) >= 5
