"""CPU suite: the path check's host form (fxjps_check_path through waypoints.check_path) against the
golden records made with the reference's own blocked() (tests/golden/make_golden_path_check.py) and against a restatement of
the definition on 2 000 further random cases; replan.FleetThrottle against replan.ReplanThrottle vehicle by vehicle."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT, grid_from_bits, load_golden, pairs

VALID, EMPTY, BLOCKED, OUTSIDE, MALFORMED = 1, 0, 2, 3, -1


@pytest.fixture(scope="module")
def built():
    import __graft_entry__
    __graft_entry__.build()


def restated(path, occ, shift=(0, 0)):
    """The definition of the issue, step by step."""
    W, H = occ.shape
    if len(path) == 0:
        return EMPTY, -1, (-1, -1)
    cx, cy = path[0][0] + shift[0], path[0][1] + shift[1]
    if not (0 <= cx < W and 0 <= cy < H):
        return OUTSIDE, 0, (cx, cy)
    for i in range(len(path) - 1):
        dx, dy = path[i + 1][0] - path[i][0], path[i + 1][1] - path[i][1]
        if (dx, dy) == (0, 0) or (dx != 0 and dy != 0 and abs(dx) != abs(dy)):
            return MALFORMED, i, (cx, cy)
        ux, uy = (dx > 0) - (dx < 0), (dy > 0) - (dy < 0)
        for _ in range(max(abs(dx), abs(dy))):
            tx, ty = cx + ux, cy + uy
            if not (0 <= tx < W and 0 <= ty < H):
                return OUTSIDE, i, (tx, ty)
            if occ[tx, ty] != 0 or (ux != 0 and uy != 0 and occ[tx, cy] != 0 and occ[cx, ty] != 0):
                return BLOCKED, i, (tx, ty)
            cx, cy = tx, ty
    return VALID, -1, (-1, -1)


def test_declared_exported_and_bound(built):
    from fuxi_planner_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "fxjps.h")).read()
    version = int(re.search(r"#define FXJPS_VERSION (\d+)", hdr).group(1))
    assert version >= 840 and _lib.VERSION == version
    assert re.search(r"^ \*\s+840\s+fxjps_check_path, fxjps_check_paths_slots", hdr, re.M), "no changelog line for version 840"
    for name, value in (("VALID", 1), ("EMPTY", 0), ("BLOCKED", 2), ("OUTSIDE", 3), ("MALFORMED", -1)):
        assert int(re.search(r"#define FXJPS_PATH_%s \(?(-?\d+)\)?" % name, hdr).group(1)) == value == getattr(_lib, "PATH_" + name)
    assert {"fxjps_check_path", "fxjps_check_paths_slots"} <= set(_lib.SYMBOLS)
    L = _lib.load()
    assert len(L.fxjps_check_path.argtypes) == 9 and len(L.fxjps_check_paths_slots.argtypes) == 9
    for doc in ("DESIGN.md", "INTEGRATION.md", "README.md"):
        assert "fxjps_check_paths_slots" in open(os.path.join(ROOT, doc)).read(), doc


def test_golden_records(built):
    from fuxi_planner_amd import waypoints
    recs = load_golden("path_check.json")
    assert len(recs) >= 300
    seen = {}
    for k, rec in enumerate(recs):
        occ = grid_from_bits(rec["grid_bits"], rec["shape"])
        got = waypoints.check_path(pairs(rec["path"]), occ, rec["shift"])
        assert got == (rec["verdict"], rec["seg"], tuple(rec["cell"])), (k, rec["kind"], got)
        assert got == restated(pairs(rec["path"]), occ, rec["shift"]), k
        seen[rec["verdict"]] = seen.get(rec["verdict"], 0) + 1
    assert all(seen.get(v, 0) >= 20 for v in (VALID, EMPTY, BLOCKED, OUTSIDE)), seen


def random_case(rng, k):
    """A grid and a path that mostly follows the rules: random straight and diagonal segments from a random cell; every so
    often a knight's move or a repeated cell, a shift, obstacle bytes of 7 and 255."""
    W, H = int(rng.integers(1, 30)), int(rng.integers(1, 30))
    occ = (rng.random((W, H)) < rng.uniform(0.0, 0.2)).astype(np.uint8)
    occ[occ != 0] = rng.choice(np.array([1, 7, 255], dtype=np.uint8), int((occ != 0).sum()))
    n = int(rng.choice([0, 1, 1, 2, 3, 5, 9, 20]))
    path = []
    if n:
        path.append((int(rng.integers(W)), int(rng.integers(H))))
    while len(path) < n:
        x, y = path[-1]
        r = rng.random()
        if r < 0.04:
            d = [(1, 2), (-2, 1), (2, -1), (-1, -2), (3, 1)][int(rng.integers(5))]  # a knight's move
        elif r < 0.08:
            d = (0, 0)  # a repeated cell
        else:
            u = [(1, 0), (-1, 0), (0, 1), (0, -1), (1, 1), (1, -1), (-1, 1), (-1, -1)][int(rng.integers(8))]
            m = int(rng.integers(1, 6))
            d = (u[0] * m, u[1] * m)
        path.append((x + d[0], y + d[1]))
    shift = None if k % 3 == 0 else (int(rng.integers(-2, 3)), int(rng.integers(-2, 3)))
    return path, occ, shift


def test_restatement_on_random_cases(built):
    from fuxi_planner_amd import waypoints
    rng = np.random.default_rng(841)
    seen = {}
    for k in range(2000):
        path, occ, shift = random_case(rng, k)
        got = waypoints.check_path(path, occ, shift)
        assert got == restated(path, occ, shift or (0, 0)), (k, path, shift, got)
        key = (got[0], min(len(path), 2))
        seen[key] = seen.get(key, 0) + 1
    for key in ((EMPTY, 0), (VALID, 1), (OUTSIDE, 1), (VALID, 2), (BLOCKED, 2), (OUTSIDE, 2), (MALFORMED, 2)):
        assert seen.get(key, 0) >= 10, (key, seen)


def test_edges_and_refusals(built):
    from fuxi_planner_amd import _lib, waypoints
    occ = np.zeros((4, 5), dtype=np.uint8)
    occ[2, 2] = 255
    assert waypoints.check_path([(2, 2)], occ) == (VALID, -1, (-1, -1))  # the first cell's own occupancy is not read
    assert waypoints.check_path([(2, 2), (2, 4)], occ) == (VALID, -1, (-1, -1))
    assert waypoints.check_path([(0, 2), (3, 2)], occ) == (BLOCKED, 0, (2, 2))
    assert waypoints.check_path([(1, 1), (3, 3)], occ) == (BLOCKED, 0, (2, 2))
    occ[2, 2] = 0
    occ[1, 2] = occ[2, 1] = 7
    assert waypoints.check_path([(1, 1), (3, 3)], occ) == (BLOCKED, 0, (2, 2))  # squeezed between two obstacles
    assert waypoints.check_path([(2, 2), (1, 1)], occ) == (BLOCKED, 0, (1, 1))
    assert waypoints.check_path([(0, 0), (0, 4), (3, 4)], occ, (0, 1)) == (OUTSIDE, 0, (0, 5))
    assert waypoints.check_path([(0, 0), (0, 4)], occ, (-1, 0)) == (OUTSIDE, 0, (-1, 0))
    assert waypoints.check_path([(0, 0), (0, 4), (1, 2)], occ) == (MALFORMED, 1, (0, 4))
    assert waypoints.check_path([(0, 0), (0, 9), (1, 2)], occ) == (OUTSIDE, 0, (0, 5))  # the earlier failure wins
    assert waypoints.check_path([(0, 0), (2, 1), (2, 9)], occ) == (MALFORMED, 0, (0, 0))  # ... and so does the malformed segment
    # cells at the ends of the int32 range: the differences do not wrap
    big = 2 ** 31 - 1
    assert waypoints.check_path([(0, 0), (big, 0)], occ) == (OUTSIDE, 0, (4, 0))
    assert waypoints.check_path([(-big - 1, 0), (big, 0)], occ) == (OUTSIDE, 0, (-big - 1, 0))
    # refusals of the C ABI
    L = _lib.load()
    c = np.zeros(4, dtype=np.int32)
    v, s = C.c_int32(), C.c_int32()
    cell = np.zeros(2, dtype=np.int32)
    ok = (_lib.ptr(c, C.c_int32), 2, _lib.ptr(occ, C.c_uint8), 4, 5, None, C.byref(v), C.byref(s), _lib.ptr(cell, C.c_int32))
    assert L.fxjps_check_path(*ok) == 0
    for at, bad in ((1, -1), (2, None), (3, 0), (4, 0), (6, None), (7, None), (8, None), (0, None)):
        args = list(ok)
        args[at] = bad
        assert L.fxjps_check_path(*args) == _lib.E_ARG, at
    args = list(ok)
    args[0], args[1] = None, 0
    assert L.fxjps_check_path(*args) == 0 and v.value == EMPTY


class FakeClock(object):
    def __init__(self):
        self.t = 100.0

    def __call__(self):
        return self.t


def test_fleet_throttle_is_replan_throttle_per_vehicle():
    from fuxi_planner_amd.replan import FleetThrottle, ReplanThrottle
    rng = np.random.default_rng(842)
    n = 7
    clock = FakeClock()
    fleet = FleetThrottle(n, clock=clock)
    single = [ReplanThrottle(clock=clock) for _ in range(n)]
    pos = rng.uniform(-2.0, 2.0, (n, 3))
    n_due = n_not = 0
    for t in range(200):
        clock.t += float(rng.choice([0.0, 0.05, 0.1, 0.31]))
        pos = pos + rng.choice([0.0, 0.02, 0.2, 0.4], (n, 1)) * rng.uniform(-1.0, 1.0, (n, 3))
        if t % 9 == 4:
            pos[t % n, 0] = 0.0  # the quirk: a search at x == 0.0 exactly leaves "nothing searched yet"
        due = fleet.due(pos)
        want = [single[v].due(pos[v]) for v in range(n)]
        assert due.dtype == bool and due.shape == (n,) and due.tolist() == want, t
        n_due += sum(want)
        n_not += n - sum(want)
        go = [v for v in range(n) if want[v] and rng.random() < 0.8]  # (a host may mark fewer than are due)
        clock.t += 0.01
        fleet.mark(go, pos[go])
        for v in go:
            single[v].mark(pos[v])
        assert np.array_equal(fleet.last_pos, np.array([np.asarray(s.last_pos, dtype=np.float64) for s in single]))
        assert fleet.last_time.tolist() == [float(s.last_time) for s in single]
    assert n_due > 100 and n_not > 100
    # a vehicle marked at x == 0.0 is due again at once, whatever the clock says
    fleet.mark([3], [[0.0, 1.0, 1.0]])
    assert fleet.due(np.tile([0.0, 1.0, 1.0], (n, 1)))[3]
