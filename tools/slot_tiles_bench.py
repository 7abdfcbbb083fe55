#!/usr/bin/env python3
"""A fleet tick whose maps changed a little -> one JSON line, also written to --out.

n = 64 vehicles on 256 x 256 raws at 20 % density (ccst, ifa 0: the prepared grid is the raw map, tsh 2), one query each,
start and goal free cells of [16, 96)^2 with a path.  Three kinds of tick, each alternating between two sets of raws so that
every tick hands in what the kind says:
    a   nothing changed
    b   eight cells changed per vehicle in the far corner (x, y >= 160: no tile row or column of a read set)
    c   eight cells changed per vehicle under its path (inner jump points and cells between them)
Two handles, the same ticks on each: mode 0 (the generation rule; its launches are the parent commit's, kernel for kernel)
and mode 1 (fxjps_set_slot_reuse(1), the tile rule).  Per kind and mode: Planner.fleet_tick_refresh(reuse=True), and the
plain refresh_slots call alone (the tile form's cost).  Method of tools/fleet_tick_bench.py: the sides alternate in one
process, a repetition is a window of as many ticks as make a side run >= 0.2 s, medians of --reps windows, per tick.  Before
anything is timed every kind runs four ticks on both handles: the records are equal value for value and the flags are what
the kind says (a: all 1; b: mode 0 none, mode 1 all 2; c: none).  Nothing here is a threshold.
Usage: python tools/slot_tiles_bench.py [--reps 5]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
N, SIDE, NCHG = 64, 256, 8
RESO, MAP_O = 0.25, (-2.0, 1.0)


def same(a, b):
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
    if isinstance(a, np.ndarray):
        return a.shape == np.shape(b) and a.tobytes() == np.asarray(b).tobytes()
    if isinstance(a, float):
        return isinstance(b, float) and np.float64(a).tobytes() == np.float64(b).tobytes()  # (NaN included)
    return a == b


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "slot_tiles_bench.json"))
    a = ap.parse_args()
    import fuxi_planner_amd as fx
    from fuxi_planner_amd import synth
    import fleet_tick_bench as ftb

    p = {0: fx.Planner([0]), 1: fx.Planner([0])}
    p[1].set_slot_reuse("tiles")
    rng = np.random.default_rng(830)
    raws = [synth.synth_grid(SIDE, SIDE, 2000 + v, 0.20) for v in range(N)]
    # one query per vehicle with a path, in the low corner
    for m in p:
        p[m].set_grid_slots([(v, raws[v]) for v in range(N)])
    starts, goals = np.zeros((N, 2), np.int32), np.zeros((N, 2), np.int32)
    todo = list(range(N))
    while todo:
        for v in todo:
            free = np.argwhere(raws[v][16:96, 16:96] == 0) + 16
            starts[v], goals[v] = free[rng.choice(len(free), 2, replace=False)]
        off, cells, _, st = p[0].plan_batch_slots(np.arange(N), starts, goals, 2)
        todo = [v for v in todo if st[v] < 3]  # (at least one inner jump point)
    jobs = lambda maps: [(v, maps[v], tuple(starts[v]), tuple(goals[v]), 0, "ccst") for v in range(N)]
    far, under = [m.copy() for m in raws], [m.copy() for m in raws]
    for v in range(N):
        fx_, fy = rng.integers(160, SIDE, NCHG), rng.integers(160, SIDE, NCHG)
        far[v][fx_, fy] ^= 1
        path = cells[off[v]:off[v + 1]]
        n = 0
        for (ax, ay), (bx, by) in zip(path[1:-1], path[2:]):  # inner jump points, then cells of the segments behind them
            for i in range(max(abs(bx - ax), abs(by - ay))):
                c = (ax + i * np.sign(bx - ax), ay + i * np.sign(by - ay))
                if n < NCHG and c != tuple(goals[v]):
                    under[v][c] = 1
                    n += 1
    kinds = {"a": (jobs(raws), jobs(raws), 1, 1), "b": (jobs(raws), jobs(far), 0, 2), "c": (jobs(raws), jobs(under), 0, 0)}
    pos = np.array([[RESO * x + MAP_O[0], RESO * y + MAP_O[1], 1.0] for x, y in starts])
    goal = np.array([[RESO * x + MAP_O[0], RESO * y + MAP_O[1], 1.5] for x, y in goals])
    home = pos[:, :2] + 1.0
    tick = lambda m, jb: p[m].fleet_tick_refresh(jb, pos, goal, home, RESO, MAP_O, publish=False, reuse=True)
    out = {"tool": "slot_tiles_bench", "n": N, "raw": [SIDE, SIDE], "changed_cells_per_vehicle": NCHG, "reps": a.reps, "window_s": ftb.WINDOW_S,
           "timed": "Planner.fleet_tick_refresh(reuse=True, publish=False) / Planner.refresh_slots", "cases": []}
    ms = lambda ts: round(float(np.median(ts)) * 1e3, 4)
    spread = lambda ts: [round(min(ts) * 1e3, 4), round(max(ts) * 1e3, 4)]
    for kind, (even, odd, flag0, flag1) in kinds.items():
        # both handles on the same ticks, value for value, and the flags of the kind, before anything is timed
        seen = {0: [], 1: []}
        for t in range(5):
            recs = {m: tick(m, odd if t & 1 else even) for m in p}
            for r0, r1 in zip(recs[0], recs[1]):
                bad = [k for k in r0 if k != "reused" and not same(r0[k], r1[k])]  # (what was searched is the modes' difference)
                assert not bad, (kind, t, bad)
            for m in p:
                seen[m].append([int(r["reused"]) + int(r.get("reused_tiles", False)) for r in recs[m]])
        assert all(f == [flag0] * N for f in seen[0][1:]) and all(f == [flag1] * N for f in seen[1][1:]), (kind, seen)
        state = {m: 1 for m in p}  # (tick 4 handed in `even`)

        def run(m, call):
            call(m, odd if state[m] & 1 else even)
            state[m] += 1

        sides = {"tick_mode0": lambda: run(0, tick), "tick_mode1": lambda: run(1, tick),
                 "refresh_mode0": lambda: run(0, lambda m, jb: p[m].refresh_slots(jb)), "refresh_mode1": lambda: run(1, lambda m, jb: p[m].refresh_slots(jb))}
        t, per = ftb.windows(sides, a.reps)
        case = {"kind": kind, "flags_mode0": flag0, "flags_mode1": flag1, "calls_per_window": per}
        for name in sides:
            case[name + "_ms"] = ms(t[name])
            case["spread_" + name + "_ms"] = spread(t[name])
        case["tick_mode1_over_mode0"] = round(float(np.median(t["tick_mode1"]) / np.median(t["tick_mode0"])), 4)
        case["refresh_mode1_over_mode0"] = round(float(np.median(t["refresh_mode1"]) / np.median(t["refresh_mode0"])), 4)
        out["cases"].append(case)
        for m in p:  # (the refresh windows moved the maps without a replan: start the next kind from stored results of its own)
            tick(m, even)
    for h in p.values():
        h.close()
    line = json.dumps(out)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
