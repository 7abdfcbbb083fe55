"""GPU suite (-m gpu): the goal rule of the single-grid prepare calls runs on the device (fx::goal_rule through
k_prepare_goal), the one copy that the slot calls run as well.

Every case goes through four routes on one fresh handle -- refresh_grid into the empty handle (mode 2) and again on the
same arguments (mode 0), prepare_grid, prepare_occupancy_msg (the same map as a message), prepare_slots with one job --
and every output of every route is the same and is oracle.gridprep.prepare_full's wherever that has an answer (the
reference raises at ifa 0 in the st variant and on a goal whose row and column are full; those expectations are stated by
hand).  Each case asserts, from the oracle's grid, that its input reaches the branch it is named for.  The C functions are
called directly: the outputs start at a sentinel, so a failing call can be seen to leave them alone."""
import ctypes as C

import numpy as np
import pytest

import refresh_grid_cases as rc
from oracle import gridprep

pytestmark = pytest.mark.gpu
SENT = -7777
ROUTES = ("refresh, mode 2", "refresh, mode 0", "prepare_grid", "prepare_occupancy_msg")


def single(p, route, raw, start, goal, ifa, variant):
    """One single-grid route through the C ABI -> (rc, (start', goal', map_d, (W, H), end_occu), (changed, mode))."""
    from fuxi_planner_amd import _lib
    L, h = p._L, p._h
    W0, H0 = raw.shape
    s, g, md = (C.c_int32 * 2)(*start), (C.c_int32 * 2)(*goal), (C.c_int32 * 2)(SENT, SENT)
    W, H, eo, mode, ch = C.c_int32(SENT), C.c_int32(SENT), C.c_int32(SENT), C.c_int32(SENT), C.c_int64(SENT)
    outs = [s, g, C.byref(W), C.byref(H), md, C.byref(eo)]
    u8 = np.ascontiguousarray(raw, dtype=np.uint8)
    if route.startswith("refresh"):
        rcode = L.fxjps_refresh_grid(h, _lib.ptr(u8, C.c_uint8), W0, H0, ifa, variant, *outs, C.byref(ch), C.byref(mode))
    elif route == "prepare_grid":
        rcode = L.fxjps_prepare_grid(h, _lib.ptr(u8, C.c_uint8), W0, H0, ifa, variant, *outs)
    else:
        msg = rc.to_msg(raw > 0, 3)
        rcode = L.fxjps_prepare_occupancy_msg(h, _lib.ptr(msg, C.c_int8), W0, H0, ifa, variant, *outs)
    return rcode, (tuple(s), tuple(g), tuple(md), (W.value, H.value), eo.value), (ch.value, mode.value)


def slot_route(p, raw, start, goal, ifa, variant):
    """prepare_slots with one job (slot 0) -> (rc of the call, the job's status, the outputs as `single` gives them)."""
    arr, keep = p._slot_jobs([(0, raw, start, goal, ifa, variant)])
    rcode = p._L.fxjps_prepare_slots(p._h, arr, 1)
    j = arr[0]
    del keep
    return rcode, j.status, (tuple(j.start_xy), tuple(j.goal_xy), tuple(j.map_d), (j.W, j.H), j.end_occu)


def four_routes(p, raw, start, goal, ifa, variant, want, grid, tag, contexts=1):
    """`want`: (start', goal', map_d, (W, H), end_occu); `grid`: the prepared grid.  `p` holds no grid of these extents."""
    for route in ROUTES:
        rcode, out, (ch, mode) = single(p, route, raw, start, goal, ifa, variant)
        assert rcode == 0, (tag, route, p._L.fxjps_last_error(p._h))
        assert out == want, (tag, route, out, want)
        if route.startswith("refresh"):
            assert (ch, mode) == ((-1, 2) if route.endswith("2") else (0, 0)), (tag, route, ch, mode)
        for c in range(contexts):
            assert np.array_equal(p.get_grid(c), grid), (tag, route, c)
    rcode, status, out = slot_route(p, raw, start, goal, ifa, variant)
    assert (rcode, status) == (0, 0) and out == want, (tag, "slot", rcode, status, out, want)
    assert np.array_equal(p.get_grid_slot(0), grid), (tag, "slot")


def row_raw(free, shape=(3, 200)):
    """Row 1 occupied except the cells `free`."""
    raw = np.zeros(shape, np.uint8)
    raw[1, :] = 1
    raw[1, list(free)] = 0
    return raw


def column_raw():
    raw = np.zeros((200, 3), np.uint8)
    raw[:, 1] = 1
    raw[100, :] = 1
    raw[3, 1] = 0
    return raw


def bar_raw():
    raw = np.zeros((9, 9), np.uint8)
    raw[4, 3:6] = 1
    return raw


def dot_raw():
    raw = np.zeros((12, 12), np.uint8)
    raw[9, 9] = 1
    return raw


def free_dists(line, c):
    """Distances from index c to the free cells of a grid line, ascending."""
    return sorted(abs(int(y) - c) for y in np.flatnonzero(line == 0))


# what a case's name claims, judged on the oracle's grid G, the shifted goal (x, y) and ifa
def row_second_step(G, x, y, ifa):
    return G[x, y] == 1 and free_dists(G[x], y)[0] == 97  # (>= 64: the first ballot step of 64 lanes finds nothing)


def row_tie(G, x, y, ifa):
    return G[x, y] == 1 and free_dists(G[x], y)[:2] == [97, 97]


def row_boundary_a(G, x, y, ifa):
    return G[x, y] == 1 and free_dists(G[x], y) == [64, 65]  # (the first cell of the second step against the second)


def row_boundary_b(G, x, y, ifa):
    return G[x, y] == 1 and free_dists(G[x], y) == [63, 64]  # (the last cell of the first step against the second step)


def row_full_column_free(G, x, y, ifa):
    return G[x].all() and not G[:, y].all()


def goal_occupied_in_padded_grid(G, x, y, ifa):
    return ifa > 0 and G[x, y] == 1 and not G[x].all()


def box_misses_above(G, x, y, ifa):  # the occupied cell nearest to the goal lies at x + ifa: the slice's open end
    return G[x, y] == 0 and G[x + ifa, y] == 1 and not G[x - ifa:x + ifa, y - ifa:y + ifa].any()


def box_hits_its_first_row(G, x, y, ifa):  # ... at x - ifa: the slice's closed end, and nowhere else in the box
    return G[x, y] == 0 and G[x - ifa, y] == 1 and not G[x - ifa + 1:x + ifa, y - ifa:y + ifa].any()


def box_misses_below(G, x, y, ifa):  # ... at x - ifa - 1
    return G[x, y] == 0 and G[x - ifa - 1, y] == 1 and not G[x - ifa:x + ifa, y - ifa:y + ifa].any()


# (name, raw, goal, ifa, variant, branch, expected goal' or None, expected end_occu)
CASES = [
    ("row, second ballot step", row_raw([3]), (1, 100), 0, 1, row_second_step, (1, 3), 0),
    ("row, tie", row_raw([3, 197]), (1, 100), 0, 1, row_tie, (1, 3), 0),
    ("row, step boundary (a)", row_raw([36, 165]), (1, 100), 0, 1, row_boundary_a, (1, 36), 0),
    ("row, step boundary (b)", row_raw([37, 164]), (1, 100), 0, 1, row_boundary_b, (1, 37), 0),
    ("row full -> column", column_raw(), (100, 1), 0, 1, row_full_column_free, (3, 1), 0),
    ("padding, st", bar_raw(), (5, 5), 1, 0, goal_occupied_in_padded_grid, (6, 3), 1),
    ("padding, ccst", bar_raw(), (4, 4), 1, 1, goal_occupied_in_padded_grid, (6, 3), 0),
    ("ccst box, ifa 1, below", dot_raw(), (7, 9), 1, 1, box_misses_above, None, 0),
    ("ccst box, ifa 1, first row", dot_raw(), (11, 9), 1, 1, box_hits_its_first_row, None, 1),
    ("ccst box, ifa 1, above", dot_raw(), (12, 9), 1, 1, box_misses_below, None, 0),
    ("ccst box, ifa 2, below", dot_raw(), (5, 9), 2, 1, box_misses_above, None, 0),
    ("ccst box, ifa 2, first row", dot_raw(), (13, 9), 2, 1, box_hits_its_first_row, None, 1),
    ("ccst box, ifa 2, above", dot_raw(), (14, 9), 2, 1, box_misses_below, None, 0),
]
START = (0, 0)


@pytest.fixture(scope="module")
def oracle_answers():
    """prepare_full of every case, computed once."""
    return {c[0]: gridprep.prepare_full(c[1], START, c[2], c[3], c[4]) for c in CASES}


@pytest.mark.parametrize("case", CASES, ids=lambda c: c[0])
def test_four_routes_equal_the_oracle(case, oracle_answers):
    import fuxi_planner_amd as fx
    name, raw, goal, ifa, variant, branch, moved, end_occu = case
    grid, s, g, md, eo = oracle_answers[name]
    g0 = (goal[0] + md[0] - (variant == 0), goal[1] + md[1] - (variant == 0))
    assert branch(grid, g0[0], g0[1], ifa), (name, "the input misses its branch")
    assert g == (g0 if moved is None else moved) and eo == end_occu, (name, g, eo)  # (the issue's table against the oracle)
    assert max(grid.shape) <= 200 and (min(grid.shape) <= 3 or max(grid.shape) < 30)
    with fx.Planner([0]) as p:
        four_routes(p, raw, START, goal, ifa, variant, (s, g, md, grid.shape, eo), grid, name)


def test_st_without_dilation():
    """ifa 0 in the st variant: the reference raises (a range with step 0), the library defines it -- no dilation, the st
    shift.  The expectation is stated by hand: the grid is the raw map, the goal (2, 101) is cell (1, 100), which moves to
    (1, 3) as in the first case, and st reports end_occu 1 for a goal that was occupied."""
    import fuxi_planner_amd as fx
    raw = row_raw([3])
    with pytest.raises(ValueError):
        gridprep.prepare_full(raw, START, (2, 101), 0, 0)
    assert row_second_step(raw, 1, 100, 0)
    with fx.Planner([0]) as p:
        four_routes(p, raw, START, (2, 101), 0, 0, ((-1, -1), (1, 3), (0, 0), (3, 200), 1), raw, "st, ifa 0")


def test_row_and_column_full():
    """The reference raises (np.argmin of nothing).  Every single-grid route returns E_ARG with its message, leaves the
    caller's arrays alone and the grid resident all the same; the slot route reports the job's status, the call is fine.
    (out_changed / out_mode of a refresh are the diff's outcome, reported before the goal is judged: not checked here.)"""
    import fuxi_planner_amd as fx
    from fuxi_planner_amd import _lib
    raw, goal = np.ones((5, 7), np.uint8), (2, 3)
    with pytest.raises(ValueError):
        gridprep.prepare_full(raw, START, goal, 0, 1)
    assert raw[2].all() and raw[:, 3].all()
    untouched = (START, goal, (SENT, SENT), (SENT, SENT), SENT)
    with fx.Planner([0]) as p:
        for route in ROUTES:
            if route.startswith("prepare"):  # (another grid: the route has to build this one itself)
                p.set_grid_occ(np.zeros((2, 2), np.uint8))
            rcode, out, _ = single(p, route, raw, START, goal, 0, 1)
            assert rcode == _lib.E_ARG, (route, rcode)
            assert b"fully occupied" in p._L.fxjps_last_error(p._h), route
            assert out == untouched, (route, out)
            assert np.array_equal(p.get_grid(), raw), route
        rcode, status, _ = slot_route(p, raw, START, goal, 0, 1)
        assert (rcode, status) == (0, _lib.E_ARG)


def test_two_contexts(oracle_answers):
    import fuxi_planner_amd as fx
    name, raw, goal, ifa, variant = CASES[6][:5]
    grid, s, g, md, eo = oracle_answers[name]
    assert g != (goal[0] + md[0], goal[1] + md[1])  # (a moved goal)
    with fx.Planner([0, 0]) as p2:
        four_routes(p2, raw, START, goal, ifa, variant, (s, g, md, grid.shape, eo), grid, "two contexts", contexts=2)


def test_a_deferred_update_in_front_of_the_goal():
    """The goal's row has two free cells; a deferred cell update, still queued on the context's stream when refresh_grid is
    called, occupies the nearer one, and the raw handed in says the same (mode 0: nothing to apply).  The goal rule runs
    behind the update on that stream, so the goal moves to the farther cell."""
    import fuxi_planner_amd as fx
    raw, goal = row_raw([90, 120]), (1, 100)
    with fx.Planner([0]) as p:
        assert p.prepare_grid(raw, START, goal, 0, "ccst") == (START, (1, 90), (0, 0), (3, 200), 0)
        p.update_cells(np.array([[1, 90]], np.int32), np.array([1], np.uint8), rebuild=False)
        raw[1, 90] = 1
        want = gridprep.prepare_full(raw, START, goal, 0, 1)
        assert want[2] == (1, 120) and free_dists(want[0][1], 100) == [20]
        rcode, out, (ch, mode) = single(p, "refresh", raw, START, goal, 0, 1)
        assert rcode == 0 and (ch, mode) == (0, 0), (rcode, ch, mode)
        assert out == (want[1], want[2], want[3], want[0].shape, want[4]), out
        assert np.array_equal(p.get_grid(), want[0])


def test_replan_frame_raw_moves_the_goal_as_prepare_grid():
    """A frame that changes one raw cell and whose goal lies on a dilated obstacle: the preparation outputs and the two
    stored queries' results equal those of prepare_grid + plan_batch on a twin handle, and the oracle's preparation."""
    import fuxi_planner_amd as fx
    raw = np.zeros((32, 32), np.uint8)
    raw[10, 5:20] = 1
    raw[20, 12:30] = 1
    start, ifa = (2, 2), 1
    s = np.array([[5, 5], [5, 33]], np.int32)
    g = np.array([[33, 33], [33, 5]], np.int32)
    with fx.Planner([0]) as p, fx.Planner([0]) as q:
        p.prepare_grid(raw, start, (29, 29), ifa, "ccst")
        p.set_queries(s, g, 2, 4096)
        raw[15, 15] = 1           # (the frame's change: a mode-1 update is queued in front of the goal rule)
        goal = (20, 20)           # (on the second bar)
        grid, s1, g1, md, eo = gridprep.prepare_full(raw, start, goal, ifa, 1)
        assert grid[goal[0] + md[0], goal[1] + md[1]] == 1 and g1 != (goal[0] + md[0], goal[1] + md[1])
        assert not grid[s[:, 0], s[:, 1]].any() and not grid[g[:, 0], g[:, 1]].any()
        out = p.replan_frame_raw(raw, start, goal, ifa, "ccst")
        want = q.prepare_grid(raw, start, goal, ifa, "ccst")
        assert want == (s1, g1, md, grid.shape, eo)
        assert out[4:9] == want and out[10] == 1 and out[9] > 0, out[4:]
        assert np.array_equal(p.get_grid(), grid) and np.array_equal(q.get_grid(), grid)
        paths = q.plan_batch(s, g, 2, 4096)
        for a, b in zip(out[:4], paths):
            assert np.array_equal(a, b)
        assert (out[3] > 0).all()
