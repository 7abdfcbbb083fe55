#!/usr/bin/env python3
"""Golden vectors for what both nodes send out after their waypoint block, produced by EXECUTING the
reference's own lines at generation time (the method of make_golden_waypoints.py: the lines are read from /root/reference,
dedented and exec'ed on prepared inputs; only inputs and outputs are stored):

    st    scripts/global_planner_st.py:287-327 (no path / the waypoint block with path3), :335 (pointw.z), :356-361 (the
          Point's x, y and the two publish calls)
    ccst  scripts/global_planner_ccst.py:481-544 (with map_line_col, :258-283), :559-562, :590-598

The publish calls land in a stub that records their arguments.  Every float64 is stored as the 16 hex digits of its bit
pattern (a NaN keeps its sign).  A handful of maps of at most 48 x 48 cells are shared by all cases, so that a GPU test can
hold them in as many grid slots.

    python tests/golden/make_golden_tick_outputs.py
"""
import contextlib
import io
import json
import math
import os
import sys
import textwrap
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
REF = "/root/reference/scripts"


def ref_lines(name, lo, hi):
    with open(os.path.join(REF, name), encoding="utf-8", errors="replace") as f:
        return "".join(f.readlines()[lo - 1:hi])


def bits(a):
    return ["%016x" % int(v) for v in np.ascontiguousarray(a, dtype=np.float64).reshape(-1).view(np.uint64)]


class Sink(object):
    def __init__(self):
        self.calls = []

    def publish(self, msg):
        self.calls.append(("goal_global", (msg.x, msg.y, msg.z)))


class Point(object):
    x = y = z = 0.0


def planner_stub():
    """map_line_col is the reference's method (ccst:258-283); the publishers record what they are given."""
    src = "class P(object):\n" + ref_lines("global_planner_ccst.py", 258, 283)
    ns = {"np": np}
    exec(compile(src, "map_line_col", "exec"), ns)

    class Stub(ns["P"]):
        def __init__(self):
            self.goalpub = Sink()
            self.calls = self.goalpub.calls

        def publish_goal(self, g):
            self.calls.append(("goal", list(g)))

        def publish_path(self, p):
            self.calls.append(("path", np.array(p, dtype=np.float64)))

        def publish_dir_path(self, p, back):
            self.calls.append(("dir", np.array(p, dtype=np.float64), back))
    return Stub()


def run_blocks(name, ranges, ns):
    with contextlib.redirect_stdout(io.StringIO()), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for lo, hi in ranges:
            exec(compile(textwrap.dedent(ref_lines(name, lo, hi)), "%s:%d-%d" % (name, lo, hi), "exec"), ns)


def run_case(c, maps):
    P = planner_stub()
    path1 = (list(map(tuple, c["path"])), 0.0) if c["path"] else (0, 0.0)
    ns = {"np": np, "math": math, "path1": path1, "map_reso": c["reso"], "map_o": list(c["origin"]), "global_goal": np.array(c["goal"]),
          "px": c["pos"][0], "py": c["pos"][1], "pz": c["pos"][2], "xo": c["home"][0], "yo": c["home"][1], "end_occu": c["end_occu"],
          "planner": P, "pointw": Point(), "path3": None, "path4": None, "wp": None, "ang_wp": 0}
    if c["variant"] == 0:
        ns.update({"map_start": np.array(c["map_start"]), "dis_wp_tre": 2, "ang_wp_tre": math.pi / 4,
                   "wp": None if c["prev_wp"] is None else np.array(c["prev_wp"])})
        run_blocks("global_planner_st.py", [(287, 327), (335, 335), (356, 361)], ns)
    else:
        ns["mapu"] = maps[c["map"]].astype(np.float64)
        run_blocks("global_planner_ccst.py", [(481, 544), (559, 562), (590, 598)], ns)
    point = [c2 for c2 in P.calls if c2[0] == "goal_global"]
    assert len(point) == 1
    paths = [c2[1] for c2 in P.calls if c2[0] == "path"]
    dirs = [c2 for c2 in P.calls if c2[0] == "dir"]
    assert len(paths) == (1 if c["path"] else 0) and len(dirs) == (1 if c["variant"] == 1 else 0)
    out = {"wp": bits(ns["wp"]), "goal_out": bits(ns["global_goal"]), "point": bits(point[0][1]),
           "path3": bits(paths[0]) if paths else [], "dir": bits(dirs[0][1]) if dirs else [], "dir_back": int(dirs[0][2]) if dirs else 0}
    if c["variant"] == 0:
        out["ang_wp"] = bits([ns["ang_wp"]])[0]
    else:
        out["kept"] = [[int(k[0]), int(k[1])] for k in ns["path2_c"]] if c["path"] else []
    return out, np.asarray(ns["wp"], dtype=np.float64)


def main():
    from oracle import oracle
    rng = np.random.default_rng(20261018)
    maps = []
    for W, H, dens in ((48, 48, 0.12), (41, 47, 0.2), (33, 29, 0.08), (48, 17, 0.15), (23, 48, 0.25), (9, 11, 0.0)):
        maps.append((rng.random((W, H)) < dens).astype(np.uint8))
    cases = []
    tries = 0
    while len(cases) < 72 and tries < 5000:
        tries += 1
        k = len(cases)
        variant = k % 2
        mi = int(rng.integers(0, len(maps)))
        occ = maps[mi]
        free = np.argwhere(occ == 0)
        s, g = free[rng.integers(0, len(free))], free[rng.integers(0, len(free))]
        cells, _, _ = oracle.plan(occ, (int(s[0]), int(s[1])), (int(g[0]), int(g[1])), 2)
        if cells == 0:
            continue
        path = [[int(c[0]), int(c[1])] for c in cells]
        kind = (k // 2) % 12  # what this case is about
        if kind == 0:
            path = []               # no path
        elif kind in (1, 2, 3):
            path = path[:kind]      # 1, 2 and 3 points
        reso = float(rng.choice([0.1, 0.2, 0.25, 0.5]))
        origin = [float(rng.uniform(-5, 5)), float(rng.uniform(-5, 5))]
        first = path[0] if path else [int(s[0]), int(s[1])]
        base = (np.array(first) + 1) * reso + np.array(origin)
        pos = [float(base[0] + rng.normal(0, 0.3)), float(base[1] + rng.normal(0, 0.3)), float(rng.choice([0.0, 0.5, 1.0, 1.5]))]
        goal = [float((g[0] + 1) * reso + origin[0]), float((g[1] + 1) * reso + origin[1]), float(rng.choice([1.0, 1.5, 2.0]))]
        home = [float(pos[0] + rng.normal(0, 2.0)), float(pos[1] + rng.normal(0, 2.0))]
        c = {"map": mi, "variant": variant, "path": path, "reso": reso, "origin": origin, "pos": pos, "goal": goal, "home": home,
             "end_occu": int(kind in (4, 5) or (kind == 0 and (k // 24) % 2 == 1)), "kind": kind}  # (no path: 0, 1, 0 per node)
        if variant == 0:
            c["map_start"] = [first[0] + 1 + int(rng.integers(-1, 2)), first[1] + 1 + int(rng.integers(-1, 2))]
            c["prev_wp"] = None if rng.random() < 0.5 else [float(rng.uniform(-5, 20)), float(rng.uniform(-5, 20))] + ([1.0] if rng.random() < 0.5 else [])
        if kind == 5:
            c["home"] = pos[:2]     # end_occu holds the position: wp == goal == home, 0 / 0
        elif kind == 6:
            c["home"] = goal[:2]    # goal == home: x / 0, or 0 / 0 when the waypoint is the goal
        elif kind == 7:
            c["home"] = [float(v) for v in run_case(c, maps)[1][:2]]  # wp == home: 0 / x
        elif kind == 8:
            c["pos"] = [goal[0] + 0.2, goal[1] - 0.3, pos[2]]        # ccst: within 0.5 of the goal
        elif kind == 9 and not path:
            continue
        c["out"] = run_case(c, maps)[0]
        cases.append(c)
    doc = {"maps": [{"W": int(m.shape[0]), "H": int(m.shape[1]), "occ_bits": np.packbits(m).tobytes().hex()} for m in maps], "cases": cases}
    p = os.path.join(HERE, "tick_outputs.json")
    with open(p, "w") as f:
        json.dump(doc, f, separators=(",", ":"))
    nan = sum(1 for c in cases if math.isnan(np.array([int(c["out"]["point"][2], 16)], dtype=np.uint64).view(np.float64)[0]))
    print("wrote", p, len(cases), "cases,", os.path.getsize(p), "bytes;", nan, "with a NaN z;",
          sum(1 for c in cases if not c["path"]), "without a path;", sum(c["end_occu"] for c in cases), "with end_occu")


if __name__ == "__main__":
    main()
