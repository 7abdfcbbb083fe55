"""GPU suite (-m gpu): the fleet ticks under the ccst node's replan throttle --
Planner.fleet_tick_throttled, fleet_tick_refresh(throttle=) with and without reuse.

Six vehicles on 48 x 40 raw maps, three ccst and three st, five ticks with a fake clock and scripted positions.  The model
is the all-planned tick (Planner.fleet_tick) run beside it on a second handle, and replan.ReplanThrottle per vehicle:

    tick 0  t = 100.00  everybody is searched (nothing searched yet)
    tick 1  t = 100.05  vehicle 0 has moved 0.5 m: due; the others keep their paths
    tick 2  t = 100.10  an obstacle lands on vehicle 1's kept path: forced.  Vehicle 3 has moved: due.  Vehicle 2's map origin
                        moves by two whole cells (the map's content with it): its path is checked two cells over, and kept
    tick 3  t = 100.15  vehicle 4's origin moves by half a cell: forced.  Vehicle 0 has moved again: due.  Vehicle 2's path,
                        still the one of tick 0, is still checked two cells over
    tick 4  t = 100.42  more than 0.3 s since the searches of ticks 0 - 2: vehicles 1, 2, 3 and 5 are due, 0 and 4 are not
"""
import numpy as np
import pytest

from test_refresh_slots_gpu import same_value

pytestmark = pytest.mark.gpu
N, W0, H0, RESO, IFA = 6, 48, 40, 0.25, 1
VARIANT = (1, 0, 1, 0, 0, 1)  # vehicles 0, 2 and 5 are ccst
KEPT_KEYS = ("status", "cost", "wp", "dim", "goal_out", "ang_wp", "n_kept", "path", "dir_path", "dir_back", "cells")
MAP_KEYS = ("start", "goal", "map_d", "shape", "end_occu", "origin", "msg", "image")
TIMES = (100.0, 100.05, 100.10, 100.15, 100.42)
FORCED = {(2, 1), (3, 4)}  # (tick, vehicle)


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


class Clock(object):
    t = 0.0

    def __call__(self):
        return self.t


class Script(object):
    """The fleet's state tick by tick: raws, origins, positions (and the cells they fall in)."""

    def __init__(self):
        rng = np.random.default_rng(8404)
        self.raw = []
        for v in range(N):
            m = np.zeros((W0, H0), dtype=np.uint8)
            m[8:40, 8:32] = rng.random((32, 24)) < 0.07  # (nothing near the border: a map that moves by two cells loses nothing)
            self.raw.append(m)
        self.map_o = np.array([[-2.0 + v, 1.0 - 0.5 * v] for v in range(N)])
        self.goal_xy = self.map_o + RESO * np.array([[43.0, 35.0 - 3 * (v % 3)] for v in range(N)])
        self.goal_z = np.array([1.5 + 0.25 * (v % 3) for v in range(N)])
        self.pos = np.c_[self.map_o + RESO * np.array([[4.5, 3.5 + 4 * (v % 2)] for v in range(N)]), np.ones(N)]
        self.home = self.pos[:, :2] - np.array([0.3, 0.2])

    def advance(self, t, kept_cells):
        """The scripted change in front of tick t; kept_cells: vehicle 1's path of tick 0 (prepared-grid cells)."""
        if t in (1, 3):
            self.pos[0, :2] += (0.4, 0.3)
        if t == 2:
            self.pos[3, :2] += (0.0, 0.4)
            c = kept_cells[len(kept_cells) // 2] - 2 * IFA  # a jump point in the middle of the path, in raw cells
            assert 0 <= c[0] < W0 and 0 <= c[1] < H0
            self.raw[1] = self.raw[1].copy()
            self.raw[1][c[0], c[1]] = 1
            self.map_o[2, 0] += 2 * RESO
            self.raw[2] = np.roll(self.raw[2], -2, axis=0)
        if t == 3:
            self.map_o[4, 0] += 0.5 * RESO
        self.pos[5, :2] += (0.01, 0.02)  # less than 0.3 m in all

    def cell(self, xy, v):
        return tuple(int(c) for c in np.floor((np.asarray(xy) - self.map_o[v]) / RESO + 1e-9))

    def jobs(self, first_slot):
        return [(first_slot + v, self.raw[v], self.cell(self.pos[v, :2], v), self.cell(self.goal_xy[v], v), IFA, VARIANT[v]) for v in range(N)]

    def goals(self):
        return np.c_[self.goal_xy, self.goal_z]


def node_z(variant, rec, pos, home):
    """pointw.z as the nodes write it: st:335 / ccst:559-562."""
    wp, goal = np.asarray(rec["wp"], dtype=np.float64), rec["goal_out"]
    with np.errstate(all="ignore"):
        if variant == 1 and (np.linalg.norm(goal[0:2] - pos[0:2]) < 0.5 or rec["end_occu"]):
            return 0.0
        return 1 + min(np.linalg.norm(wp[0:2] - home) / np.linalg.norm(goal[0:2] - home), 1) * (goal[2] - 1)


def run(planner, twin, form, check_kept=True):
    from fuxi_planner_amd.replan import FleetThrottle, ReplanThrottle
    clock = Clock()
    throttle = FleetThrottle(N, clock=clock)
    model = [ReplanThrottle(clock=clock) for _ in range(N)]
    sc = Script()
    searched = [None] * N  # each vehicle's record of its last search
    seen = []
    for t, now in enumerate(TIMES):
        clock.t = now
        if t:
            sc.advance(t, kept_cells)
        jobs, goals = sc.jobs(70), sc.goals()
        if form == "plain":
            recs = planner.fleet_tick_throttled(jobs, sc.pos, goals, sc.home, RESO, sc.map_o, throttle, publish=True, image_channels=1,
                                                check_kept=check_kept)
        else:
            recs = planner.fleet_tick_refresh(jobs, sc.pos, goals, sc.home, RESO, sc.map_o, publish=True, image_channels=1, reuse=form == "reuse",
                                              throttle=throttle, check_kept=check_kept)
        want = twin.fleet_tick(sc.jobs(10), sc.pos, goals, sc.home, RESO, sc.map_o, publish=True, image_channels=1)
        assert len(recs) == N and all(r["ok"] for r in recs) and all(w["ok"] and w["status"] > 0 for w in want), t
        extra = {"cells", "due", "forced", "path_check"} | ({"kept"} if form != "plain" else set()) | ({"reused"} if form == "reuse" else set())
        for v in range(N):
            r, w = recs[v], want[v]
            assert set(r) == set(w) | extra, (t, v)
            forced = check_kept and (t, v) in FORCED
            due = model[v].due(sc.pos[v]) or forced
            assert (r["due"], r["forced"]) == (due, forced), (form, t, v, r["due"], r["forced"], r["path_check"])
            for k in MAP_KEYS:
                assert same_value(r[k], w[k]), (t, v, k)
            if due:
                model[v].mark(sc.pos[v])
                for k in w:  # the all-planned tick's record, key by key
                    assert same_value(r[k], w[k]), (form, t, v, k, r[k], w[k])
                assert r["cells"].dtype == np.int32 and r["cells"].shape == (r["status"], 2)
                world = (r["cells"] + (1, 0 if VARIANT[v] else 1)) * RESO + np.asarray(r["origin"])  # path3 of st:292-298 / ccst:487-494
                assert np.array_equal(world, r["path"][:, :2])
                assert r["path_check"] == (2 if forced and v == 1 else None), (t, v)
                searched[v] = r
            else:
                for k in KEPT_KEYS:
                    assert same_value(r[k], searched[v][k]), (form, t, v, k)
                assert r["point"].dtype == np.float64 and r["point"][:2].tobytes() == np.asarray(r["wp"][:2]).tobytes()
                assert np.float64(r["point"][2]).tobytes() == np.float64(node_z(VARIANT[v], r, sc.pos[v], sc.home[v])).tobytes(), (t, v)
                assert r["path_check"] == (None if not check_kept else 1), (t, v)
                if form == "reuse":
                    assert r["reused"] is False
                if v == 2 and t >= 2:  # checked two cells over: the kept cells are those of tick 0's grid
                    assert r["origin"][0] == searched[v]["origin"][0] + 2 * RESO
        if t == 0:
            kept_cells = recs[1]["cells"]
        seen.append([r["due"] for r in recs])
        assert throttle.records[0] is recs[0]
    return seen


@pytest.mark.parametrize("form", ["plain", "refresh", "reuse"])
def test_throttled_tick(planner, twin, form):
    seen = run(planner, twin, form)
    assert seen == [[True] * 6,
                    [True, False, False, False, False, False],
                    [False, True, False, True, False, False],
                    [True, False, False, False, True, False],
                    [False, True, True, True, False, True]]


def test_without_the_check_nobody_is_forced(planner, twin):
    seen = run(planner, twin, "refresh", check_kept=False)
    assert seen == [[True] * 6,
                    [True, False, False, False, False, False],
                    [False, False, False, True, False, False],
                    [True, False, False, False, False, False],
                    [False, True, True, True, True, True]]


def test_without_a_throttle_the_records_are_what_they_were(planner, twin):
    """The assertion of test_refresh_slots_gpu.test_fleet_tick_with_refresh, once more with the new arguments spelt out."""
    sc = Script()
    for t in range(2):
        recs = planner.fleet_tick_refresh(sc.jobs(70), sc.pos, sc.goals(), sc.home, RESO, sc.map_o, publish=True, image_channels=1, throttle=None,
                                          check_kept=True)
        want = twin.fleet_tick(sc.jobs(10), sc.pos, sc.goals(), sc.home, RESO, sc.map_o, publish=True, image_channels=1)
        for v in range(N):
            assert set(recs[v]) - {"kept"} == set(want[v]), v
            for k in want[v]:
                assert same_value(recs[v][k], want[v][k]), (t, v, k)


def test_world_form(planner, twin):
    """fleet_tick_world under the throttle: tick 0 searches everybody and equals the call without a throttle; on tick 1,
    0.05 s later with nobody moved, every path is checked, found valid and kept, and the maps are this tick's."""
    from fuxi_planner_amd.replan import FleetThrottle
    sc = Script()
    clock = Clock()
    throttle = FleetThrottle(N, clock=clock)
    wjobs = lambda s: [(s + v, sc.raw[v], sc.map_o[v], RESO, sc.pos[v, :2], sc.goal_xy[v], IFA, VARIANT[v]) for v in range(N)]
    first = None
    for t, now in enumerate((50.0, 50.05)):
        clock.t = now
        if t == 1:  # a new map for vehicle 3, away from its path
            sc.raw[3] = sc.raw[3].copy()
            sc.raw[3][44:46, 2:4] = 1
        recs = planner.fleet_tick_world(wjobs(70), sc.pos, sc.goals(), sc.home, publish=True, image_channels=1, refresh=True, throttle=throttle)
        want = twin.fleet_tick_world(wjobs(10), sc.pos, sc.goals(), sc.home, publish=True, image_channels=1, refresh=True)
        for v in range(N):
            r, w = recs[v], want[v]
            assert r["ok"] and w["status"] > 0 and set(r) == set(w) | {"cells", "due", "forced", "path_check"}, (t, v)
            assert (r["due"], r["forced"], r["path_check"]) == ((True, False, None) if t == 0 else (False, False, 1)), (t, v)
            for k in set(w) - {"kept"} if t == 0 else MAP_KEYS + ("kept",):  # (tick 0's kept hangs on what the slots held before)
                assert same_value(r[k], w[k]), (t, v, k)
            if t == 1:
                for k in KEPT_KEYS:
                    assert same_value(r[k], first[v][k]), (t, v, k)
                assert np.float64(r["point"][2]).tobytes() == np.float64(node_z(VARIANT[v], r, sc.pos[v], sc.home[v])).tobytes(), (t, v)
        assert t == 0 or not want[3]["kept"]
        first = first or recs
