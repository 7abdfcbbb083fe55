"""GPU suite (-m gpu): fxjps_prepare_slots -- n vehicles' raw maps padded, dilated, their goals relocated and their derived
maps built into n grid slots by ONE call.  Everything is compared for equality: with the goldens captured from the
reference's own lines (gridprep.json, occupancy_msg.json, tick.json), with oracle/gridprep.py (which test_gridprep.py pins
to those goldens), with the host reference of the derived maps, and with the one-grid calls on a second handle."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from conftest import load_golden
from test_derived_maps_gpu import check_maps

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def unpack(bits_hex, shape):
    W, H = shape
    return np.unpackbits(np.frombuffer(bytes.fromhex(bits_hex), dtype=np.uint8))[:W * H].reshape(W, H)


def golden_job(slot, r):
    return (slot, unpack(r["raw_bits"], r["raw_shape"]), r["start"], r["goal"], r["ifa"], r["variant"])


def check_against_gridprep_golden(p, slot, out, r, tag):
    """One job's outputs and its slot against a record of gridprep.json."""
    s, g, d, shape, eo, ok = out
    assert ok, tag
    assert list(s) == r["start_out"] and list(g) == r["goal_out"] and list(d) == r["map_d"], (tag, out)
    assert list(shape) == r["grid_shape"] and eo == r["end_occu"], (tag, out)
    grid = unpack(r["grid_bits"], r["grid_shape"])
    assert np.array_equal(p.get_grid_slot(slot), grid), tag
    check_maps(p.debug_slot_maps(slot), grid, tag)


def check_against_prepare_full(p, slot, out, job, tag, maps=True):
    """One job's outputs and its slot against oracle.gridprep.prepare_full of the same inputs.  -> the prepared grid"""
    from oracle import gridprep
    _, raw, start, goal, ifa, variant = job
    eg, es, ego, ed, eeo = gridprep.prepare_full(raw, start, goal, ifa, {"st": 0, "ccst": 1}.get(variant, variant))
    s, g, d, shape, eo, ok = out
    assert ok, tag
    assert (s, g, d, eo) == (es, ego, ed, eeo) and shape == eg.shape, (tag, out, (es, ego, ed, eeo, eg.shape))
    assert np.array_equal(p.get_grid_slot(slot), eg), tag
    if maps:
        check_maps(p.debug_slot_maps(slot), eg, tag)
    return eg


def largest_reference_map():
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


def test_all_golden_preparations_in_one_call(planner):
    recs = load_golden("gridprep.json")
    assert len(recs) == 240
    outs = planner.prepare_slots([golden_job(i, r) for i, r in enumerate(recs)])
    assert len(outs) == 240
    for i, (o, r) in enumerate(zip(outs, recs)):
        check_against_gridprep_golden(planner, i, o, r, ("golden", i))
    # what the fixture must exercise, so that a thinner one cannot pass silently
    moved = sum(r["goal_out"] != [r["goal"][k] + r["map_d"][k] - (1 if r["variant"] == 0 else 0) for k in (0, 1)] for r in recs)
    negative = sum(min(r["start"] + r["goal"]) < 0 for r in recs)
    assert sum(r["end_occu"] for r in recs) >= 80 and moved >= 80 and negative >= 30, (moved, negative)
    assert {r["variant"] for r in recs} == {0, 1}


def test_occupancy_messages(planner, other):
    from oracle import gridprep
    recs = load_golden("occupancy_msg.json")
    assert len(recs) == 40
    jobs, maps = [], []
    for k, r in enumerate(recs):
        w, h = r["width"], r["height"]
        data = np.array(r["data"], dtype=np.int8)
        jobs.append((k, (data, w, h), (0, 0), (w - 1, h - 1), 1 + (k & 1), k & 1))  # the pattern of test_gridprep.py
        maps.append(np.array(r["map"], dtype=np.int64).reshape(w, h))               # what map_callback stores
    outs = planner.prepare_slots(jobs)
    for k, (o, job, m) in enumerate(zip(outs, jobs, maps)):
        eg, es, ego, ed, eeo = gridprep.prepare_full(m, job[2], job[3], job[4], job[5])
        s, g, d, shape, eo, ok = o
        assert ok and (s, g, d, eo) == (es, ego, ed, eeo) and shape == eg.shape, (k, o)
        got = planner.get_grid_slot(k)
        assert np.array_equal(got, eg), k
        check_maps(planner.debug_slot_maps(k), eg, ("msg", k))
        # ... and the one-grid call on a second handle
        assert other.prepare_occupancy_msg(job[1][0], job[1][1], job[1][2], job[2], job[3], job[4], job[5]) == o[:5], k
        assert np.array_equal(other.get_grid(), got), k


def test_constructed_edge_cases(planner):
    from fuxi_planner_amd import FxjpsError, _lib
    rng = np.random.default_rng(11)
    wall = np.zeros((5, 4), np.uint8)
    wall[2, :] = 1           # the goal's row is full: the column decides, (1, 1) and (3, 1) tie, the lower index wins
    cross = wall.copy()
    cross[:, 1] = 1          # ... and its column too: the reference raises
    dot = np.zeros((10, 10), np.uint8)
    dot[4, 6] = 1
    jobs = [(30, (rng.random((20, 15)) < 0.2).astype(np.uint8), (1, 1), (10, 10), 0, 1),
            (31, wall, (0, 0), (2, 1), 0, 1),
            (32, cross, (0, 0), (2, 1), 0, 1),
            (33, np.zeros((1, 1), np.uint8), (0, 0), (0, 0), 1, 1),
            (34, np.ones((1, 1), np.uint8), (0, 0), (0, 0), 1, 0),
            (35, dot, (1, 1), (4, 6), 64, 0),
            (36, dot, (1, 1), (4, 6), 64, 1),
            (37, (rng.random((30, 40)) < 0.1).astype(np.uint8), (-300, 5), (3, 3), 1, 0),
            (38, (rng.random((30, 40)) < 0.1).astype(np.uint8), (7, -211), (29, 39), 2, 1)]
    planner.set_grid_slot(32, np.zeros((3, 3), np.uint8))  # (the failing job's slot held a grid: it is empty afterwards)
    outs = planner.prepare_slots(jobs)
    for o, job in zip(outs, jobs):
        if job[0] == 32:
            from oracle import gridprep
            with pytest.raises(ValueError):
                gridprep.prepare_full(*job[1:])
            assert o[5] is False
            continue
        check_against_prepare_full(planner, job[0], o, job, ("edge", job[0]))
    assert outs[1][1] == (1, 1)
    # the failed job's slot is empty: reading it and planning on it refuse, the other slots of the call plan
    with pytest.raises(FxjpsError) as e:
        planner.get_grid_slot(32)
    assert e.value.code == _lib.E_ARG
    with pytest.raises(FxjpsError) as e:
        planner.plan_batch_slots([31, 32], [(0, 0), (0, 0)], [(1, 1), (1, 1)], 2)
    assert e.value.code == _lib.E_ARG and "32" in str(e.value)
    off, cells, cost, st = planner.plan_batch_slots([31, 33], [outs[1][0], outs[3][0]], [outs[1][1], outs[3][1]], 2)
    assert st[0] > 0 and cells[off[1] - 1].tolist() == [1, 1]
    # ... and takes a grid again
    again = planner.prepare_slots([(32, wall, (0, 0), (2, 1), 0, 1)])
    check_against_prepare_full(planner, 32, again[0], (32, wall, (0, 0), (2, 1), 0, 1), "edge 32 again")


def test_mixed_sizes_in_one_call(planner, other):
    """Among them a prepared grid of more than 2^18 cells (its maps are built behind the shared launches) and the largest
    map of the reference's PNG fixtures: occupancy and every derived array byte-identical with set_grid_slot of the
    host-prepared grid on a second handle, and equal to the host reference."""
    from fuxi_planner_amd import synth
    rng = np.random.default_rng(13)
    ref = largest_reference_map()
    big = (rng.random((600, 600)) < 0.05).astype(np.uint8)
    jobs = [(40, (rng.random((9, 200)) < 0.1).astype(np.uint8), (0, 0), (8, 199), 1, 0),
            (41, big, (3, 3), (590, 580), 1, 1),
            (42, ref, (1, 1), (ref.shape[0] - 2, ref.shape[1] - 2), 2, 0),
            (43, synth.synth_grid(256, 256, 5, 0.20), (0, 0), (255, 255), 1, 1),
            (44, (rng.random((3, 2)) < 0.3).astype(np.uint8), (0, 0), (2, 1), 1, 0),
            (45, (rng.random((520, 505)) < 0.1).astype(np.uint8), (-2, 7), (500, 400), 1, 0),
            (46, (rng.random((130, 127)) < 0.3).astype(np.uint8), (5, 5), (100, 100), 3, 1)]
    outs = planner.prepare_slots(jobs)
    shapes = [o[3][0] * o[3][1] for o in outs]
    assert max(shapes) > 1 << 18 and sum(s > 1 << 18 for s in shapes) == 2 and min(shapes) < 100
    for o, job in zip(outs, jobs):
        eg = check_against_prepare_full(planner, job[0], o, job, ("mixed", job[0]))
        other.set_grid_slot(job[0], eg)
        want, got = other.debug_slot_maps(job[0]), planner.debug_slot_maps(job[0])
        assert set(want) == set(got)
        for name in want:
            assert want[name].tobytes() == got[name].tobytes(), (job[0], name)
        other.clear_grid_slot(job[0])


def run_fleet_tick(p):
    """The 120 ticks of tick.json as one fleet tick: one prepare_slots, one plan_batch_slots, waypoints per path."""
    import fuxi_planner_amd as fx
    from fuxi_planner_amd import waypoints
    recs = load_golden("tick.json")
    assert len(recs) == 120 and {r["variant"] for r in recs} == {0, 1}
    outs = p.prepare_slots([golden_job(i, r) for i, r in enumerate(recs)])                      # N1, every vehicle
    for i, (o, r) in enumerate(zip(outs, recs)):
        s, g, d, shape, end_occu, ok = o
        assert ok and list(s) == r["map_start"] and list(g) == r["map_goal"] and list(shape) == r["grid_shape"], (i, o)
        assert end_occu == r["end_occu"], i
    off, cells, cost, st = p.plan_batch_slots(np.arange(120), [o[0] for o in outs], [o[1] for o in outs], 2)  # hot path
    planned = inter = held = 0
    for i, (o, r) in enumerate(zip(outs, recs)):
        s, g, d, shape, end_occu, ok = o
        if r["path"] is None:
            assert st[i] == 0, (i, st[i])
            continue
        assert st[i] > 0, (i, st[i])
        path = cells[off[i]:off[i + 1]].tolist()
        assert path == r["path"], i
        planned += 1
        origin = fx.Planner.shifted_origin(r["origin"], d, r["reso"])
        if r["variant"] == 0:                                                                    # N2
            wp, goal_out, _ = waypoints.select_st(path, s, r["reso"], origin, r["pos"], r["goal3"], end_occu, r["prev_wp"])
        else:
            wp, _, goal_out = waypoints.select_ccst(path, p.get_grid_slot(i), r["reso"], origin, r["pos"], r["goal3"], end_occu,
                                                    return_goal=True)
        assert goal_out.tolist() == r["goal_out"], i
        assert wp.tolist() == r["wp"], (i, r["variant"], wp, r["wp"])
        inter += r["wp"][:2] != r["goal3"][:2]
        held += end_occu
    assert planned > 50 and inter > 20 and held > 15


def test_fleet_tick_matches_reference_sequence(planner):
    run_fleet_tick(planner)


def test_steady_state_and_isolation(planner):
    """The same slots prepared three times with different raws (smaller, larger, the first again); slots not named and
    the resident grid with its stored replan results are what they were."""
    from fuxi_planner_amd import synth
    recs = sorted(load_golden("gridprep.json"), key=lambda r: r["grid_shape"][0] * r["grid_shape"][1])
    small, large = recs[:12], recs[-12:]
    slots = list(range(100, 112))
    keep = {120: synth.synth_grid(90, 70, 21, 0.2), 121: synth.synth_grid(40, 130, 22, 0.25)}
    for k, occ in keep.items():
        planner.set_grid_slot(k, occ)
    kid = np.repeat(list(keep), 50).astype(np.int32)
    kq = [synth.synth_queries(keep[k], 5 + k, 50) for k in keep]
    ks, kg = np.concatenate([q[0] for q in kq]), np.concatenate([q[1] for q in kq])
    resident = synth.synth_grid(150, 110, 23, 0.2)
    rs, rg = synth.synth_queries(resident, 23, 100)
    planner.set_grid_occ(resident)
    planner.set_queries(rs, rg, 2)
    first = planner.replan_frame()
    planner.replan_frame()
    reused = planner.timing()["reused"]
    assert reused > 0

    def same(a, b):
        return all(x.tobytes() == y.tobytes() for x, y in zip(a, b))

    def round_(rs_):
        outs = planner.prepare_slots([golden_job(s, r) for s, r in zip(slots, rs_)])
        for s, o, r in zip(slots, outs, rs_):
            check_against_gridprep_golden(planner, s, o, r, ("steady", s, r["grid_shape"]))

    round_(small)
    # the stored results of the resident grid were not dropped, nor its grid touched
    assert same(planner.replan_frame(), first) and planner.timing()["reused"] == reused
    assert np.array_equal(planner.get_grid(), resident)
    before = planner.plan_batch_slots(kid, ks, kg, 2)
    round_(large)
    round_(small)
    assert same(planner.plan_batch_slots(kid, ks, kg, 2), before)
    for k, occ in keep.items():
        assert np.array_equal(planner.get_grid_slot(k), occ)
    assert np.array_equal(planner.get_grid(), resident)
    assert same(planner.replan_frame(), first)


def _raw_jobs(specs):
    """A fxjps_slot_job_t array from dicts (the refusals need what Planner.prepare_slots cannot express)."""
    from fuxi_planner_amd import _lib
    arr = (_lib.SlotJob * max(len(specs), 1))()
    keep = []
    for j, sp in zip(arr, specs):
        raw = np.ascontiguousarray(sp.get("raw", np.zeros((6, 5), np.uint8)), dtype=np.uint8)
        keep.append(raw)
        j.raw = None if sp.get("null_raw") else raw.ctypes.data
        j.slot, j.layout = sp.get("slot", 0), sp.get("layout", 0)
        j.W0, j.H0 = sp.get("W0", raw.shape[0]), sp.get("H0", raw.shape[1])
        j.ifa, j.variant = sp.get("ifa", 1), sp.get("variant", 0)
        j.start_xy[0], j.start_xy[1] = sp.get("start", (1, 1))
        j.goal_xy[0], j.goal_xy[1] = sp.get("goal", (3, 3))
    return arr, keep


def test_refusals_change_nothing(planner):
    from fuxi_planner_amd import _lib
    rng = np.random.default_rng(17)
    held = {200: (rng.random((40, 30)) < 0.15).astype(np.uint8), 201: (rng.random((25, 60)) < 0.15).astype(np.uint8)}
    jobs = [(k, raw, (1, 1), (20, 20), 1, k & 1) for k, raw in held.items()]
    outs = planner.prepare_slots(jobs)
    ids = np.array(list(held), np.int32)
    starts, goals = [o[0] for o in outs], [o[1] for o in outs]
    grids = {k: planner.get_grid_slot(k) for k in held}
    plan = planner.plan_batch_slots(ids, starts, goals, 2)
    L, h = planner._L, planner._h
    good = {"slot": 200, "raw": np.ones((6, 5), np.uint8)}  # (job 0 of every refused call would overwrite slot 200)
    bad = [{"slot": -1}, {"slot": _lib.MAX_GRID_SLOTS}, {"slot": 200}, {"slot": 201, "null_raw": True}, {"slot": 201, "W0": 0},
           {"slot": 201, "H0": -3}, {"slot": 201, "ifa": -1}, {"slot": 201, "ifa": 65}, {"slot": 201, "variant": 2},
           {"slot": 201, "layout": 2}, {"slot": 201, "raw": np.zeros((8000, 2), np.uint8), "ifa": 64},
           {"slot": 201, "start": (-8100, 0), "goal": (100, 0)}, {"slot": 201, "ifa": 0, "variant": 0, "goal": (0, 2)},
           {"slot": 201, "ifa": 0, "variant": 1, "goal": (6, 2)}]
    for sp in bad:
        arr, keep = _raw_jobs([good, sp])
        assert L.fxjps_prepare_slots(h, arr, 2) == _lib.E_ARG, sp
        assert b"job 1" in L.fxjps_last_error(h), (sp, L.fxjps_last_error(h))
    arr, keep = _raw_jobs([{"slot": s} for s in range(_lib.MAX_GRID_SLOTS)] + [{"slot": 0}])
    for n in (-1, _lib.MAX_GRID_SLOTS + 1):
        assert L.fxjps_prepare_slots(h, arr, n) == _lib.E_ARG, n
    assert L.fxjps_prepare_slots(h, None, 1) == _lib.E_ARG
    assert L.fxjps_prepare_slots(h, None, 0) == 0  # (an empty call is no error, and does nothing)
    for k in held:
        assert np.array_equal(planner.get_grid_slot(k), grids[k]), k
    again = planner.plan_batch_slots(ids, starts, goals, 2)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(again, plan))
    # the struct the binding fills is the one the library reads
    assert L.fxjps_slot_job_size() == C.sizeof(_lib.SlotJob)


def test_two_contexts():
    import fuxi_planner_amd as fx
    with fx.Planner([0, 0]) as p2:
        run_fleet_tick(p2)
        per = [t["queries"] for t in p2.timing_per_context()]
        assert sum(per) == 120 and min(per) > 0, per  # (both contexts' slots served a shard)
