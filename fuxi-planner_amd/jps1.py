"""Drop-in for the reference's scripts/jps1.py: same module name, same entry point.

The ROS nodes do `import jps1` and call, once per tick,
    path1 = jps1.method(mapu, tuple(map_start), tuple(map_goal), 2)
(global_planner_st.py:285, global_planner_ccst.py:477) and then test
`path1[0] is 0` and take `np.array(path1[0]) + np.array([1, 1])`.  Put this
package's directory on sys.path ahead of scripts/  and the nodes
run unchanged; the search itself executes on the MI355X through libfxjps.so.
"""
import time

import numpy as np

from . import planner as _planner
from . import _lib


def method(matrix, start, goal, hchoice):
    """-> (list[(x, y)], seconds) or (0, seconds), as jps1.py:183-230.

    Side effect kept from the reference: on success the path cost is printed
    (jps1.py:207; `0` for start == goal)."""
    t0 = time.time()
    p = _planner.default_planner()
    p.set_grid(matrix)  # (not uploaded again when it equals the resident grid)
    start = (int(start[0]), int(start[1]))
    goal = (int(goal[0]), int(goal[1]))
    st, cost0, cells = p.plan_one(start, goal, hchoice)
    if st == _lib.Q_BAD_START:
        # jps1.py indexes matrix[start] unchecked: IndexError (or silent numpy wrap-around for
        # negative indices, which no caller relies on)
        raise IndexError("index %r is out of bounds for grid of shape %r" % (start, p.shape))
    if st < 0:
        raise _lib.FxjpsError(st, "query failed")
    elapsed = round(time.time() - t0, 6)
    if st == 0:
        return (0, elapsed)
    path = [(int(x), int(y)) for x, y in cells]
    print(0 if start == goal else cost0)
    return (path, elapsed)


def method_many(calls, hchoice):
    """jps1.method for a fleet: calls is a sequence of up to 256 (matrix, start, goal), vehicle v's call in calls[v].
    -> per vehicle what method returns, (list[(x, y)], seconds) or (0, seconds); seconds is the whole call's time.

    Vehicle v's matrix lives in grid slot v of the default planner.  One refresh_grid_slots and one replan_slots serve
    the whole fleet: a matrix whose prepared bytes are what its slot holds is not built again, and a vehicle whose
    slot, start and goal are those of the call before is not searched again -- by the library's own bytes and
    generations, nothing is cached here.  The costs of the found paths are printed in vehicle order (`0` for
    start == goal), as method prints its one.  Raises before anything is planned: ValueError for more than 256 calls,
    the reference's TypeError for an hchoice other than 1 or 2, IndexError for a start outside its own matrix."""
    t0 = time.time()
    calls = list(calls)
    if len(calls) > _lib.MAX_GRID_SLOTS:
        raise ValueError("%d calls: a fleet call takes at most %d" % (len(calls), _lib.MAX_GRID_SLOTS))
    if hchoice not in (1, 2):
        raise TypeError("unsupported operand type(s) for +: 'float' and 'NoneType' (hchoice must be 1 or 2)")
    grids, starts, goals = [], [], []
    for v, (matrix, start, goal) in enumerate(calls):
        occ = _planner.as_occ(matrix)
        if occ.ndim != 2:
            raise ValueError("vehicle %d: grid must be 2-D" % v)
        start = (int(start[0]), int(start[1]))
        if not (0 <= start[0] < occ.shape[0] and 0 <= start[1] < occ.shape[1]):
            raise IndexError("vehicle %d: index %r is out of bounds for grid of shape %r" % (v, start, occ.shape))
        grids.append(occ)
        starts.append(start)
        goals.append((int(goal[0]), int(goal[1])))
    if not calls:
        return []
    p = _planner.default_planner()
    p.refresh_grid_slots(list(enumerate(grids)))
    offsets, cells, cost, status, _ = p.replan_slots(range(len(calls)), starts, goals, hchoice)
    elapsed = round(time.time() - t0, 6)
    for v in np.flatnonzero(status < 0):
        raise _lib.FxjpsError(int(status[v]), "vehicle %d: query failed" % v)
    out = []
    for v, st in enumerate(status):
        if st == 0:
            out.append((0, elapsed))
            continue
        out.append(([(int(x), int(y)) for x, y in cells[offsets[v]:offsets[v + 1]]], elapsed))
        print(0 if starts[v] == goals[v] else float(cost[v]))
    return out
