"""GPU suite (-m gpu): jps1.method_many -- the reference's call, jps1.method(matrix, start, goal, hchoice), for a fleet: one
refresh_grid_slots and one replan_slots for up to 256 vehicles, vehicle v on grid slot v of the process-wide planner.  The
goldens captured from the real jps1.py go through it grouped by hchoice: the return tuples, `is 0` and the printed costs in
vehicle order.  What the fleet form adds -- a tick whose matrices, starts and goals are those of the tick before builds
nothing and searches nothing, by the library's own bytes and generations -- is read off Planner.timing()."""
import contextlib
import io

import numpy as np
import pytest

from conftest import grid_from_bits, load_golden, pairs

pytestmark = pytest.mark.gpu


def many(calls, hchoice):
    """-> (what method_many returns, the printed lines)"""
    from fuxi_planner_amd import jps1
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        out = jps1.method_many(calls, hchoice)
    return out, buf.getvalue().splitlines()


def check_call(recs, grids, hchoice, tag):
    """One method_many over the records (all of `hchoice`) against what the real jps1.method returned and printed."""
    out, lines = many([(g, tuple(r["start"]), tuple(r["goal"])) for r, g in zip(recs, grids)], hchoice)
    assert isinstance(out, list) and len(out) == len(recs), tag
    assert len({r[1] for r in out}) == 1 and isinstance(out[0][1], float), (tag, "one time for the whole call")
    for v, (r, rec) in enumerate(zip(out, recs)):
        assert isinstance(r, tuple) and len(r) == 2, (tag, v)
        if rec["path"] is None:
            assert r[0] is 0, (tag, v, r[0])  # noqa: F632  (the callers' own idiom, global_planner_st.py:287)
        else:
            assert r[0] == pairs(rec["path"]) and all(type(c) is int for cell in r[0] for c in cell), (tag, v, r[0], rec["path"])
    want = [rec["printed"] for rec in recs if rec["path"] is not None]
    assert len(lines) == len(want), (tag, lines, want)
    for got, w in zip(lines, want):
        assert got == w or float(got) == float(w), (tag, got, w)
    return out


def by_hchoice(recs, grids):
    for hc in (1, 2):
        pick = [k for k, r in enumerate(recs) if r["hchoice"] == hc]
        if pick:
            yield hc, [recs[k] for k in pick], [grids[k] for k in pick]


def test_known_answers_in_one_call_each():
    recs = load_golden("known_answers.json")
    grids = [np.array(r["grid"], dtype=np.float64).reshape(r["shape"]) for r in recs]
    seen = 0
    for hc, rs, gs in by_hchoice(recs, grids):
        out = check_call(rs, gs, hc, ("known_answers", hc))
        seen += len(out)
        names = [r["name"] for r in rs]
        if hc == 2:  # (the printed `0` of start == goal, on a free cell and on an obstacle; 100 is free)
            assert {"start == goal", "start == goal on an obstacle", "value 100 is free", "goal out of bounds"} <= set(names)
    assert seen == 16


def test_random_small_goldens_in_calls_of_at_most_256():
    recs = load_golden("random_small.json")
    grids = [grid_from_bits(r["grid_bits"], r["shape"]) for r in recs]
    assert len(recs) == 400
    calls = 0
    for hc, rs, gs in by_hchoice(recs, grids):
        for at in range(0, len(rs), 256):
            check_call(rs[at:at + 256], gs[at:at + 256], hc, ("random_small", hc, at))
            calls += 1
    assert calls >= 2


def test_the_reference_maps_one_call_per_query_round(map_grids):
    recs = load_golden("maps_png.json")
    per_map = {}
    for r in recs:
        per_map.setdefault(r["map"], []).append(r)
    assert len(per_map) == 35 and len(recs) == 180

    def grid_of(r):
        bits = np.unpackbits(map_grids[r["map"]])
        if "canvas" in r:  # (the 147 x 112 map in the corner of the 256 x 256 canvas, as tests/test_search_work_gpu.py places it)
            g = np.zeros((256, 256), np.uint8)
            g[:147, :112] = bits[:147 * 112].reshape(147, 112)
            return g
        W, H = r["shape"]
        return bits[:W * H].reshape(W, H).astype(np.uint8)

    seen = 0
    for k in range(max(len(v) for v in per_map.values())):
        rs = [v[k] for v in per_map.values() if k < len(v)]
        for hc, rr, gs in by_hchoice(rs, [grid_of(r) for r in rs]):
            seen += len(check_call(rr, gs, hc, ("maps_png", k, hc)))
    assert seen == 180


def fleet(seed=826):
    rng = np.random.default_rng(seed)
    calls = []
    for W, H in ((30, 41), (64, 64), (17, 90), (55, 23), (100, 37)):
        m = (rng.random((W, H)) < 0.12).astype(np.float64)
        m[:3, :3] = 0
        m[-3:, -3:] = 0
        calls.append((m, (0, 0), (W - 1, H - 1)))
    return calls


def oracle_answers(oracle, calls):
    out = []
    for m, s, g in calls:
        path, cost, _ = oracle.plan((np.asarray(m) == 1).astype(np.uint8), s, g, 2, literal=False)
        out.append((path, cost))
    return out


def check_tick(oracle, calls, searched, tag):
    """One method_many against the oracle on THIS tick's matrices; `searched`: whether anything was searched, as the
    planner's timing record of the call's replan_slots says."""
    from fuxi_planner_amd import default_planner
    out, lines = many(calls, 2)
    want = oracle_answers(oracle, calls)
    assert [r[0] for r in out] == [p for p, _ in want], tag
    assert [float(x) for x in lines] == [c for p, c in want if p], (tag, lines)
    T = default_planner().timing()
    if searched is None:
        assert T["reused"] == len(calls) and T["search_launches"] == 0 and T["pops"] == 0, (tag, T)
    else:
        assert T["reused"] == len(calls) - len(searched) and T["search_launches"] >= 1, (tag, T)
    return out


def test_ticks_of_a_fleet(oracle):
    from fuxi_planner_amd import default_planner
    p = default_planner()
    calls = fleet()
    n = len(calls)
    first = check_tick(oracle, calls, range(n), "tick 1")
    assert sum(isinstance(r[0], list) for r in first) >= 3
    gens = [p.get_grid_slot(v).tobytes() for v in range(n)]
    # the same call again: identical returns, nothing built (every slot kept), nothing searched
    again = check_tick(oracle, calls, None, "tick 2")
    assert [r[0] for r in again] == [r[0] for r in first]
    assert p.refresh_grid_slots([(v, c[0]) for v, c in enumerate(calls)]) == [True] * n
    # a free cell's 0 turned into 100: still free by the matrix rule, the prepared bytes are equal -- kept, nothing searched
    m = calls[1][0].copy()
    fx, fy = [int(c) for c in np.argwhere(m == 0)[40]]
    m[fx, fy] = 100
    calls[1] = (m,) + calls[1][1:]
    check_tick(oracle, calls, None, "tick 3")
    assert [p.get_grid_slot(v).tobytes() for v in range(n)] == gens
    # a cell under vehicle 3's path turned into 1: only that vehicle is searched, and its answer is the oracle's on this map
    path = first[3][0]
    (ax, ay), (bx, by) = path[0], path[1]
    cell = (ax + int(np.sign(bx - ax)), ay + int(np.sign(by - ay)))
    m = calls[3][0].copy()
    assert m[cell] == 0 and cell != calls[3][2]
    m[cell] = 1
    calls[3] = (m,) + calls[3][1:]
    out = check_tick(oracle, calls, [3], "tick 4")
    assert out[3][0] != path and [out[v][0] for v in range(n) if v != 3] == [first[v][0] for v in range(n) if v != 3]
    # a slot overwritten by somebody else's set_grid_slot in between: the right answer on this tick
    p.set_grid_slot(2, np.zeros((9, 9), np.uint8))
    check_tick(oracle, calls, [2], "tick 5")
    # a start and a goal that move are searched on a kept map
    calls[0] = (calls[0][0], (1, 1), calls[0][2])
    check_tick(oracle, calls, [0], "tick 6")
    # fewer vehicles: the maps are kept, the queries searched (replan_slots reuses within a batch of the same size); then kept
    check_tick(oracle, calls[:2], [0, 1], "tick 7")
    check_tick(oracle, calls[:2], None, "tick 8")


def test_errors_plan_nothing(oracle):
    from fuxi_planner_amd import default_planner, jps1
    p = default_planner()
    calls = fleet(827)
    check_tick(oracle, calls, range(len(calls)), "before")
    held = [p.get_grid_slot(v).tobytes() for v in range(len(calls))]
    other = [(np.ones((4, 4)), (0, 0), (3, 3)) for _ in calls]  # (what a call that went through would leave in the slots)
    with pytest.raises(IndexError, match="vehicle 2"):
        jps1.method_many(other[:2] + [(np.zeros((5, 5)), (5, 5), (1, 1))] + other[3:], 2)
    with pytest.raises(IndexError, match="vehicle 0"):
        jps1.method_many([(np.zeros((5, 5)), (0, -1), (1, 1))], 2)
    with pytest.raises(TypeError):
        jps1.method_many(other, 3)
    with pytest.raises(ValueError):
        jps1.method_many([other[0]] * 257, 2)
    assert jps1.method_many([], 2) == []
    assert [p.get_grid_slot(v).tobytes() for v in range(len(calls))] == held
    check_tick(oracle, calls, None, "after")  # (neither a slot's generation nor a stored result moved)
    # numpy integers as the nodes hand them in; a goal off the grid is no path
    out, lines = many([(np.zeros((5, 5)), (np.int64(0), np.int64(0)), (np.int64(9), np.int64(9)))], 2)
    assert out[0][0] is 0 and lines == []  # noqa: F632
