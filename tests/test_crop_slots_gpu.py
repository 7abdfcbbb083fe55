"""GPU suite (-m gpu): fxjps_prepare_slots_cropped / fxjps_refresh_slots_cropped -- the world-frame calls with the ccst
node's crop of every map message in front, the box found on the device.

Two yardsticks.  tests/golden/cropprep.json holds what the reference's own lines make of every case: status, the crop
record, the prepared grid and its cells are compared with it.  And a twin handle that never sees a cropped job:
worldprep.crop_host (pinned against the same fixture by tests/test_crop_slots_host.py) crops every message on the host,
the twin takes the window through prepare_slots_world / refresh_slots_world, and the per-job outputs, the slot's bytes and
all six derived arrays are compared byte for byte."""
import ctypes as C

import numpy as np
import pytest

from cropprep_cases import bits, cases, check_record, message
from test_refresh_slots_gpu import same_slots, same_value

pytestmark = pytest.mark.gpu
R = 0.25
I32_MAX = 2147483647
NONE_BOX = [I32_MAX, I32_MAX, -1, -1]


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


def job(slot, raw, map_o, cell_s, cell_g, ifa=1, prior=None, ori_pre=(-15.0, -15.0), reso=R):
    """A cropped job (as Planner.prepare_slots_cropped takes it) whose vehicle and goal lie in the middle of a cell of the
    message's grid.  (ifa = 0 only with a goal inside the window: the reference's padded map ends at the goal's cell
    otherwise, and the call is refused as prepare_slots refuses it.)"""
    pos = (map_o[0] + (cell_s[0] + 0.5) * reso, map_o[1] + (cell_s[1] + 0.5) * reso)
    goal = (map_o[0] + (cell_g[0] + 0.5) * reso, map_o[1] + (cell_g[1] + 0.5) * reso)
    return (slot, raw, map_o, reso, pos, goal, ifa, 1, prior, ori_pre)


def host_crop(cj):
    """-> (crop record, outcome, the world job the twin takes or None)."""
    from fuxi_planner_amd import worldprep
    slot, raw, map_o, reso, pos, goal, ifa, variant, prior, ori_pre = cj
    m = raw if isinstance(raw, tuple) else (np.asarray(raw) > 0).astype(np.uint8)  # (the binding hands a matrix in as 0 / 1)
    rec, outcome, window = worldprep.crop_host(m, map_o, reso, pos, ifa)
    wj = None
    if outcome == 0:
        wj = (slot, window, rec["map_o"], reso, pos, goal, ifa, variant, prior, ori_pre, rec["map_t"])
    return rec, outcome, wj


def same_record(got, want, where):
    for k in ("bbox", "start0", "lo", "win"):
        assert list(got[k]) == list(want[k]), (where, k, got, want)
    assert bits(got["map_o"]) == bits(want["map_o"]) and bits(got["map_t"]) == bits(want["map_t"]), (where, got, want)


def is_empty(p, slot):
    from fuxi_planner_amd import FxjpsError
    try:
        p.get_grid_slot(slot)
    except FxjpsError:
        return True
    return False


def tick(p, other, cjobs, refresh, tag):
    """One cropped call on p; crop_host and the world-frame call on the twin for the jobs that go on: the same status, crop
    record, outputs and slots, and empty slots for the others.  -> (outs, status per job, kept per job or None)."""
    host = [host_crop(cj) for cj in cjobs]
    go = [v for v, h in enumerate(host) if h[1] == 0]
    outs = p.refresh_slots_cropped(cjobs) if refresh else p.prepare_slots_cropped(cjobs)
    want = (other.refresh_slots_world if refresh else other.prepare_slots_world)([host[v][2] for v in go])
    for v, (o, h) in enumerate(zip(outs, host)):
        same_record(o[-1], h[0], (tag, v))
    for i, v in enumerate(go):  # (a job that went on: 0, or E_ARG from the preparation -- a goal with no free cell -- as the twin reports it)
        assert outs[v][:-2] == want[i] and (outs[v][-2] == 0) == want[i][5], (tag, v, outs[v], want[i])
    for v, (o, h) in enumerate(zip(outs, host)):
        if h[1] != 0:
            k = 7 if refresh else 6
            zero = ((0, 0), (0, 0), (0, 0), (0, 0), 0, False) + ((False,) if refresh else ()) + ([0.0, 0.0], (0, 0), [0.0, 0.0])
            assert o[-2] == h[1] and o[:k + 3] == zero, (tag, v, o)
            assert is_empty(p, cjobs[v][0]), (tag, v)
    same_slots(p, other, [cjobs[v][0] for i, v in enumerate(go) if want[i][5]], tag)
    return outs, [o[-2] for o in outs], ([o[6] for o in outs] if refresh else None)


def test_goldens(planner, twin):
    """Every case of the fixture, 16 jobs a call, the layouts alternating, planned and unplanned jobs side by side."""
    G = cases()
    seen = set()
    for base in range(0, len(G), 16):
        chunk = G[base:base + 16]
        cjobs = []
        for k, c in enumerate(chunk):
            if c["prior"] is not None:
                planner.set_prior_map(k, c["prior"])
                twin.set_prior_map(k, c["prior"])
            # (layout 0 takes the matrix as 0 / 1: every value of the fixture is >= 0, non-zero and > 0 are the same cells)
            raw = message(c) if (base + k) % 2 else c["raw"]
            cjobs.append((k, raw, c["map_o"], c["reso"], c["pos"], c["goal_xy"], c["ifa"], 1, None if c["prior"] is None else k, c["ori_pre"]))
        outs, status, _ = tick(planner, twin, cjobs, False, ("goldens", base))
        assert len(set(status)) > 1 or base + 16 > len(G), (base, status)
        for k, (c, o) in enumerate(zip(chunk, outs)):
            where = (base + k, c["cls"])
            assert o[-2] == c["status"], (where, o)
            check_record(o[-1], c, where)
            seen.add((c["cls"], (base + k) % 2))
            if c["status"] != 0:
                continue
            pr = c["prep"]
            assert o[:6] == (tuple(pr["start_out"]), tuple(pr["goal_out"]), tuple(pr["map_d"]), tuple(pr["grid_shape"]), pr["end_occu"], True), where
            assert bits(o[6]) == bits(pr["origin"]) and list(o[7]) == c["canvas_shape"] and bits(o[8]) == bits(c["canvas_o"]), where
            assert np.array_equal(planner.get_grid_slot(k), pr["grid"]), where
    assert len(seen) == 14  # (every class in both layouts)


SINGLE = (125, 66)  # in the third block of a 130 x 70 message in either layout


def bounds_messages():
    """(name, W0, H0, cells or None: random) -- the shapes at which k_crop_bounds can go wrong, in the order of the call:
    64 x 64 fills its block exactly, and a job follows it."""
    return [("1x1", 1, 1, [(0, 0)]), ("1x17", 1, 17, None), ("17x1", 17, 1, None), ("5x7", 5, 7, None), ("16x16", 16, 16, None),
            ("64x64", 64, 64, None), ("64x65", 64, 65, None), ("130x70", 130, 70, None), ("first byte", 130, 70, [(0, 0)]),
            ("last byte", 130, 70, [(129, 69)]), ("last block", 130, 70, [SINGLE]), ("none", 130, 70, [])]


def test_bounds_kernel_shapes(planner, twin):
    rng = np.random.default_rng(790)
    assert SINGLE[0] * 70 + SINGLE[1] >= 8192 and SINGLE[1] * 130 + SINGLE[0] >= 8192
    cjobs, names = [], []
    for layout in (0, 1):
        for name, W0, H0, cells in bounds_messages():
            if layout == 0:
                m = np.zeros((W0, H0), np.uint8)
                if cells is None:
                    m[:] = rng.random((W0, H0)) < (0.5 if W0 * H0 < 300 else 0.01)
                    m[rng.integers(0, W0), rng.integers(0, H0)] = 1
                for x, y in cells or []:
                    m[x, y] = 1
                raw, nz = m, m.nonzero()
            else:  # -1 (unknown) and 0 do not count; 50, 100 and -5 do, though -5 is not occupied
                d = np.zeros((H0, W0), np.int8)
                if cells is None:
                    few = W0 * H0 < 300
                    d[:] = rng.choice(np.array([0, -1, 50, 100, -5], np.int8), size=(H0, W0), p=[0.3, 0.2, 0.2, 0.2, 0.1] if few else [0.7, 0.29, 0.004, 0.004, 0.002])
                    d[rng.integers(0, H0), rng.integers(0, W0)] = 100
                else:
                    d[:] = rng.choice(np.array([0, -1], np.int8), size=(H0, W0))
                for i, (x, y) in enumerate(cells or []):
                    d[y, x] = (100, 50, -5)[(i + len(name)) % 3]
                raw, nz = (d.reshape(-1), W0, H0), ((d.T != 0) & (d.T != -1)).nonzero()
            # the vehicle on the first non-zero cell (so that lo is the box's corner and the window is the box less its last row / column)
            cs = (int(nz[0].min()), int(nz[1].min())) if len(nz[0]) else (0, 0)
            cjobs.append(job(len(cjobs), raw, (-3.0 + 0.25 * len(cjobs), 1.5), cs, (W0 - 1, H0 - 1)))
            names.append((layout, name))
    outs, status, _ = tick(planner, twin, cjobs, False, "bounds")
    for (layout, name), cj, o, (_, W0, H0, cells) in zip(names, cjobs, outs, bounds_messages() * 2):
        rec = o[-1]
        if cells is not None and len(cells) == 1:
            assert rec["bbox"] == [cells[0][0], cells[0][1]] * 2 and o[-2] == 1, (layout, name, rec)  # (a window of 0 x 0: not planned)
        if cells == []:
            assert rec["bbox"] == NONE_BOX and o[-2] == 1, (layout, name, rec)
    by = {nm: st for nm, st in zip(names, status)}
    for layout in (0, 1):
        assert by[(layout, "64x65")] == 0 and by[(layout, "130x70")] == 0 and by[(layout, "64x64")] == 0 and by[(layout, "16x16")] == 0, by
    # a layout-1 value that counts for the box and is not occupied: it lies in the window, the prepared grid is free there
    d = np.zeros((6, 8), np.int8)
    d[1, 1], d[4, 6], d[2, 4], d[2, 3] = 100, 50, -5, -1
    o, st, _ = tick(planner, twin, [job(40, (d.reshape(-1), 8, 6), (0.0, 0.0), (1, 1), (3, 2), 0)], False, "minus five")
    assert st == [0] and o[0][-1]["bbox"] == [1, 1, 6, 4] and o[0][-1]["win"] == [5, 3] and planner.get_grid_slot(40).sum() == 1


def test_stale_padding_does_not_count(planner):
    """A 7 x 7 message of ones leaves 49 non-zero bytes where the next call stages its only message; that one has 35 cells in
    a room of 48 bytes, and the 13 bytes behind them are the earlier call's."""
    for layout in (0, 1):
        full = np.ones((7, 7), np.uint8)
        one = np.zeros((5, 7), np.uint8)
        one[1, 2] = 1
        as_raw = (lambda m: (np.where(m.T > 0, 100, 0).astype(np.int8).reshape(-1), m.shape[0], m.shape[1])) if layout else (lambda m: m)
        o = planner.prepare_slots_cropped([job(50, as_raw(full), (0.0, 0.0), (3, 3), (5, 5))])
        assert o[0][-1]["bbox"] == [0, 0, 6, 6] and o[0][-1]["win"] == [6, 6], (layout, o)
        o = planner.prepare_slots_cropped([job(50, as_raw(one), (0.0, 0.0), (3, 3), (4, 5))])
        assert o[0][-1]["bbox"] == [1, 2, 1, 2] and o[0][-1]["win"] == [0, 0] and o[0][-2] == 1, (layout, o)
        assert is_empty(planner, 50)


def refresh_fleet(rng):
    a = np.zeros((40, 30), np.uint8)
    a[5:31, 4:25] = rng.random((26, 21)) < 0.08
    a[5, 4] = a[30, 24] = 1
    b = np.zeros((33, 64), np.uint8)
    b[2:20, 10:50] = rng.random((18, 40)) < 0.05
    b[2, 10] = b[19, 49] = 1
    db = np.where(b.T > 0, 100, -1).astype(np.int8)
    c = np.zeros((12, 9), np.uint8)
    c[3, 2] = c[8, 7] = c[5, 4] = 1
    blank = np.zeros((10, 10), np.uint8)
    prior = (rng.random((50, 45)) < 0.04).astype(np.uint8)
    jobs = [job(60, a, (1.0, -2.0), (8, 8), (28, 20), 1),
            job(61, (db.reshape(-1), 33, 64), (-14.0, -13.0), (4, 20), (15, 40), 2, 0, (-15.0, -15.0)),
            job(62, c, (3.0, 3.0), (5, 5), (6, 3), 0),
            job(63, blank, (0.0, 0.0), (2, 2), (5, 5), 0),          # no non-zero cell: not planned
            job(64, c, (3.0, 3.0), (-4, 5), (6, 3), 0)]             # the vehicle left of the message: refused
    return jobs, prior


def test_refresh(planner, twin):
    from fuxi_planner_amd import FxjpsError, _lib
    rng = np.random.default_rng(791)
    jobs, prior = refresh_fleet(rng)
    planner.set_prior_map(0, prior)
    twin.set_prior_map(0, prior)
    ids = np.array([60, 61, 62], np.int32)
    outs, status, _ = tick(planner, twin, jobs, False, "tick 1")
    assert status == [0, 0, 0, _lib.JOB_NOT_PLANNED, _lib.E_ARG]
    starts, goals = [o[0] for o in outs[:3]], [o[1] for o in outs[:3]]
    planner.replan_slots(ids, starts, goals, 2)
    assert planner.replan_slots(ids, starts, goals, 2)[4].all()
    # 2. the same jobs: all kept, no generation moves, the outputs are the same
    o2, status2, kept = tick(planner, twin, jobs, True, "tick 2")
    assert kept == [True, True, True, False, False] and status2 == status
    assert all(same_value(list(x), list(y)) for x, y in zip([o[:6] + o[7:] for o in o2], outs))
    assert planner.replan_slots(ids, starts, goals, 2)[4].all()
    # 3. one cell of one message changed inside the window: that job is rebuilt, the extents stay
    a = jobs[0][1].copy()
    g = planner.get_grid_slot(60)
    lo, md = o2[0][-1]["lo"], o2[0][2]
    x, y = next((x, y) for x in range(10, 25) for y in range(8, 20) if g[x - lo[0] + md[0], y - lo[1] + md[1]] == 0)
    assert a[x, y] == 0
    a[x, y] = 1
    jobs[0] = (60, a) + tuple(jobs[0][2:])
    o3, _, kept = tick(planner, twin, jobs, True, "tick 3")
    assert kept == [False, True, True, False, False] and o3[0][3] == o2[0][3] and o3[0][-1] == o2[0][-1]
    assert planner.get_grid_slot(60)[x - lo[0] + md[0], y - lo[1] + md[1]] == 1
    assert list(planner.replan_slots(ids, starts, goals, 2)[4]) == [0, 1, 1]
    # 4. one cell changed so that the box grows: other extents, the job is rebuilt
    d = jobs[1][1][0].copy().reshape(64, 33)
    assert o3[1][-1]["bbox"] == [2, 10, 19, 49]
    d[55, 25] = 100
    jobs[1] = (61, (d.reshape(-1), 33, 64)) + tuple(jobs[1][2:])
    o4, _, kept = tick(planner, twin, jobs, True, "tick 4")
    assert kept == [True, False, True, False, False] and o4[1][-1]["bbox"] == [2, 10, 25, 55] and o4[1][-1]["win"] != o3[1][-1]["win"]
    # 5. a planned vehicle's message goes blank: its slot is emptied and its generation moves; the others are kept
    plan = planner.replan_slots(ids, [o[0] for o in o4[:3]], [o[1] for o in o4[:3]], 2)
    was = jobs[2]
    jobs[2] = (62, np.zeros((12, 9), np.uint8)) + tuple(was[2:])
    _, status5, kept = tick(planner, twin, jobs, True, "tick 5")
    assert kept == [True, True, False, False, False] and status5[2] == _lib.JOB_NOT_PLANNED and is_empty(planner, 62)
    with pytest.raises(FxjpsError):  # (refused: the slot is empty; the stored results stay)
        planner.replan_slots(ids, [o[0] for o in o4[:3]], [o[1] for o in o4[:3]], 2)
    jobs[2] = was
    twin.clear_grid_slot(62)  # (the twin never saw the blank message)
    o6, _, kept = tick(planner, twin, jobs, True, "tick 6")
    assert kept == [True, True, False, False, False] and o6[2][:6] == o4[2][:6]
    again = planner.replan_slots(ids, [o[0] for o in o6[:3]], [o[1] for o in o6[:3]], 2)
    assert list(again[4]) == [1, 1, 0] and all(x.tobytes() == y.tobytes() for x, y in zip(again[:4], plan[:4]))


def test_refusals_change_nothing(planner):
    from fuxi_planner_amd import _lib
    rng = np.random.default_rng(792)
    jobs, prior = refresh_fleet(rng)
    planner.set_prior_map(0, prior)
    planner.clear_prior_map(14)  # (the fixture's cases set it)
    held = [(200,) + tuple(jobs[0][1:]), (201,) + tuple(jobs[1][1:])]
    outs = planner.prepare_slots_cropped(held)
    assert [o[-2] for o in outs] == [0, 0]
    ids = np.array([200, 201], np.int32)
    starts, goals = [o[0] for o in outs], [o[1] for o in outs]
    plan = planner.replan_slots(ids, starts, goals, 2)
    assert planner.replan_slots(ids, starts, goals, 2)[4].all()
    grids = {k: planner.get_grid_slot(k) for k in (200, 201)}
    maps = {k: planner.debug_slot_maps(k) for k in (200, 201)}
    L, h = planner._L, planner._h
    flags = np.full(_lib.MAX_GRID_SLOTS + 1, -5, np.int32)
    out_kept = _lib.ptr(flags, C.c_int32)
    crop = (_lib.Crop * 2)()
    good = job(200, np.ones((6, 5), np.uint8), (0.0, 0.0), (0, 0), (2, 2))     # (job 0 of a refused call would overwrite slot 200)
    blank = job(200, np.zeros((6, 5), np.uint8), (0.0, 0.0), (0, 0), (2, 2))   # (... and this one would empty it)
    base = job(201, np.ones((6, 5), np.uint8), (-14.0, -14.0), (1, 1), (3, 3), 1, 0, (-15.0, -15.0))
    nan, inf = float("nan"), float("inf")
    bad = [{"pos_xy": (0, nan)}, {"pos_xy": (1, inf)}, {"prior": 14}, {"prior": _lib.MAX_PRIOR_MAPS},   # (14: in range, not set)
           {"pos_xy": (0, 1e12)},                        # start0 outside int32
           {"goal_xy": (0, -14.0 + 9000 * R)},           # a prepared grid over 8190 cells: judged after the box
           {"goal_xy": (1, -14.0 - 9000 * R)},
           {"map_o": (0, nan)}, {"goal_xy": (1, nan)}, {"ori_pre": (0, inf)}, {"map_reso": 0.0}, {"map_reso": nan},
           {"slot": -1}, {"slot": 200}, {"raw": None}, {"W0": 0}, {"H0": 8191}, {"ifa": 65}, {"variant": 2}, {"layout": 2}]
    from test_world_slots_gpu import raw_world_jobs
    for fn, extra in ((L.fxjps_prepare_slots_cropped, ()), (L.fxjps_refresh_slots_cropped, (out_kept,))):
        for sp in bad:
            for other in (good, blank):
                arr, keep = raw_world_jobs(planner, [(other, {}), (base, sp)])
                assert fn(h, arr, 2, *extra, crop) == _lib.E_ARG, sp
                assert b"job" in L.fxjps_last_error(h), (sp, L.fxjps_last_error(h))
        arr, keep = raw_world_jobs(planner, [(good, {})])
        for n in (-1, _lib.MAX_GRID_SLOTS + 1):
            assert fn(h, arr, n, *extra, crop) == _lib.E_ARG, n
        assert fn(h, None, 1, *extra, crop) == _lib.E_ARG
        assert fn(h, None, 0, *extra, crop) == 0
    assert (flags == -5).all()
    for k in (200, 201):
        assert np.array_equal(planner.get_grid_slot(k), grids[k]), k
        now = planner.debug_slot_maps(k)
        assert all(now[name].tobytes() == maps[k][name].tobytes() for name in now), k
    again = planner.replan_slots(ids, starts, goals, 2)
    assert again[4].all() and all(a.tobytes() == b.tobytes() for a, b in zip(again[:4], plan[:4]))
    # map_t is not read (the crop computes it), out_crop and out_kept may be NULL
    arr, keep = raw_world_jobs(planner, [(held[0], {"map_t": (0, nan)}), (held[1], {"map_t": (1, inf)})])
    assert L.fxjps_refresh_slots_cropped(h, arr, 2, None, None) == 0 and [j.status for j in arr[:2]] == [0, 0]
    assert [o[6] for o in planner.refresh_slots_cropped(held)] == [True, True]


def test_two_contexts(twin):
    import fuxi_planner_amd as fx
    rng = np.random.default_rng(793)
    jobs, prior = refresh_fleet(rng)
    twin.set_prior_map(0, prior)
    with fx.Planner([0, 0]) as p2:
        p2.set_prior_map(0, prior)
        for refresh in (False, True):
            _, status, kept = tick(p2, twin, jobs, refresh, ("two contexts", refresh))
            assert status == [0, 0, 0, 1, -1] and (kept is None or kept == [True, True, True, False, False])
            for s in (60, 61, 62):
                want_occ, want = twin.get_grid_slot(s), twin.debug_slot_maps(s)
                for c in (0, 1):
                    occ, got = p2.debug_slot_context(c, s)
                    assert occ.tobytes() == want_occ.tobytes(), (refresh, c, s)
                    for name in want:
                        assert got[name].tobytes() == want[name].tobytes(), (refresh, c, s, name)
            assert is_empty(p2, 63) and is_empty(p2, 64)


def test_fleet_tick_world_with_crop(planner, twin):
    """Planner.fleet_tick_world(crop=True) against fleet_tick_world on the host-cropped jobs of the vehicles that are
    planned, record by record; the vehicle that is not planned and the one refused have ok False."""
    rng = np.random.default_rng(794)
    jobs, prior = refresh_fleet(rng)
    jobs = [(100 + v,) + tuple(j[1:]) for v, j in enumerate(jobs)]
    planner.set_prior_map(0, prior)
    twin.set_prior_map(0, prior)
    n = len(jobs)
    pos = np.array([[j[4][0], j[4][1], 1.0] for j in jobs])
    goals = np.array([[j[5][0], j[5][1], 1.5 + 0.25 * (v % 3)] for v, j in enumerate(jobs)])
    home = np.array([[-2.0 + 0.5 * v, 1.0] for v in range(n)])
    host = [host_crop(j) for j in jobs]
    go = [v for v in range(n) if host[v][1] == 0]
    assert go == [0, 1, 2]
    for refresh in (False, True):
        recs = planner.fleet_tick_world(jobs, pos, goals, home, publish=True, image_channels=1, refresh=refresh, reuse=refresh, crop=True)
        want = twin.fleet_tick_world([host[v][2] for v in go], pos[go], goals[go], home[go], publish=True, image_channels=1, refresh=refresh, reuse=refresh)
        assert [r["not_planned"] for r in recs] == [False, False, False, True, False] and [r["ok"] for r in recs] == [True, True, True, False, False]
        for i, v in enumerate(go):
            assert set(recs[v]) == set(want[i]) | {"not_planned"}, (refresh, v)
            for k in want[i]:
                assert same_value(recs[v][k], want[i][k]), (refresh, v, k, recs[v][k], want[i][k])
        for v in (3, 4):
            assert all(val is None for k, val in recs[v].items() if k not in ("ok", "not_planned")), recs[v]
        assert sum(r["ok"] and r["status"] > 0 for r in recs) >= 2
