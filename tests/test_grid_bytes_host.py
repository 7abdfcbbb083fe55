"""CPU suite: the C ABI's obstacle rule -- "a cell is an obstacle iff its byte is non-zero" (include/fxjps.h) -- at the one
host function that reads a caller's grid, fxjps_waypoint_ccst.  The same grid with its occupied cells written as 1, 100,
255, 2, 128 or a random non-zero byte each must give the same waypoint, goal and kept cells, byte for byte: the line tests of
map_line_col (ccst:258-283) see a wall whatever non-zero byte stands for it.  The paths are the C oracle's.  Called
through the library itself (waypoints.select_ccst converts its matrix with == 1 first and would hide the bytes)."""
import numpy as np

from test_grid_bytes_gpu import RECODINGS, host_ccst, recode, waypoint_case


def test_host_ccst_rule_reads_non_zero_bytes(oracle):
    from fuxi_planner_amd import _lib
    L = _lib.load()
    g, paths, pos, goal = waypoint_case(oracle)
    ones = [host_ccst(L, p, recode(g, "ones"), pos[q], goal[q]) for q, p in enumerate(paths)]
    # non-vacuity: the paths turn corners the line tests have to keep (290 of 295 as the case stands); were every line free,
    # as an `== 1` reader finds them on a grid without a byte 1, each path would be cut to its two ends
    turning = sum(len(k) > 2 for _, _, k in ones)
    assert turning >= 200, (turning, len(paths))
    assert sum(len(k) < len(p) for (_, _, k), p in zip(ones, paths)) > 0  # (and some lines ARE free: the pruning does something)
    for name in RECODINGS[1:]:
        rec = recode(g, name)
        assert np.array_equal(rec != 0, g != 0) and (name == "mixed" or not (rec == 1).any())
        bad = [q for q, p in enumerate(paths) if not all(a.tobytes() == b.tobytes() for a, b in zip(host_ccst(L, p, rec, pos[q], goal[q]), ones[q]))]
        assert not bad, "%s: %d of %d paths differ from the grid of ones, first %r" % (name, len(bad), len(paths), bad[:5])
