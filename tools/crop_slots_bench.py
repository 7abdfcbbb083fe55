#!/usr/bin/env python3
"""The map half of a ccst fleet tick from map MESSAGES -> one JSON line, also written to --out.

n = 64 vehicles, no prior, ifa = 1, the ccst variant, resolution 0.25, every origin on its grid.  `synth`: 256 x 256
messages at 20 % obstacles (the box is nearly the message); `png`: the reference's own maps embedded in 256 x 256 messages
of zeros (the box is a fraction of the message).  The vehicle stands on a free cell of the map.  Sides, alternated in one
process (method of tools/refresh_slots_bench.py / tools/fleet_tick_bench.py: a repetition is a window of as many calls as
make a side run >= 0.2 s, medians of --reps windows, per call):
    cropped          Planner._world_jobs + fxjps_prepare_slots_cropped: what a ccst fleet host runs per tick with this library
    host_parent_a, host_parent_b   worldprep.crop_host per vehicle + Planner._world_jobs + fxjps_prepare_slots_world of the PARENT
                     commit's library (--parent-lib): what it ran before.  The same side twice: what the two differ by, window
                     by window, is the spread a difference has to exceed to mean anything.  Build the parent from a checkout
                     into a scratch directory:
                         git worktree add /tmp/parent HEAD~1 && make -C /tmp/parent/fuxi-planner_amd libfxjps.so
    cropped_call     the C call alone on an array filled beforehand
    world_call, parent_world_call   fxjps_prepare_slots_world of this and of the parent's library on the same host-cropped jobs
Before anything is timed the per-job outputs and every slot's bytes are compared across the three handles, and the crop
records with worldprep.crop_host's.  Bars: cropped <= host_parent_a x (1 + the A/A spread: the largest over the smallest
window of both host_parent sides, less 1); world_call <= 1.05 x parent_world_call.
Usage: python tools/crop_slots_bench.py --parent-lib /tmp/parent/fuxi-planner_amd/libfxjps.so [--reps 5] [--shapes synth png]"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
N = 64
R = 0.25
SIDE = 256


def message_fleet(shape, n):
    """-> cropped jobs as Planner.prepare_slots_cropped takes them."""
    import fleet_tick_bench as ftb
    from fuxi_planner_amd import worldprep
    out = []
    for _, raw, start, goal, ifa, _ in ftb.fleet(shape, 4 * n):
        v = slot = len(out)
        if v == n:
            break
        ax, ay = ((5 * v) % (SIDE - raw.shape[0] + 1), (3 * v) % (SIDE - raw.shape[1] + 1)) if shape != "synth" else (0, 0)
        msg = np.zeros((SIDE, SIDE), np.uint8)
        msg[ax:ax + raw.shape[0], ay:ay + raw.shape[1]] = raw
        map_o = (-15.0 + 2 * v * R, -15.0 + v * R)
        pos = (map_o[0] + (ax + start[0] + 0.5) * R, map_o[1] + (ay + start[1] + 0.5) * R)
        goal_xy = (map_o[0] + (ax + goal[0] + 0.5) * R, map_o[1] + (ay + goal[1] + 0.5) * R)
        if worldprep.crop_host(msg, map_o, R, pos, ifa)[1] == 0:  # (some of the reference's maps are blank, or a single line: the node does not plan on them)
            out.append((slot, msg, map_o, R, pos, goal_xy, ifa, 1))
    assert len(out) == n
    return out


def host_cropped(cjobs):
    """The parent's way: worldprep.crop_host per vehicle -> (world jobs, crop records)."""
    from fuxi_planner_amd import worldprep
    jobs, recs = [], []
    for slot, msg, map_o, reso, pos, goal, ifa, variant in cjobs:
        rec, outcome, window = worldprep.crop_host(msg, map_o, reso, pos, ifa)
        assert outcome == 0, (slot, rec)
        jobs.append((slot, window, rec["map_o"], reso, pos, goal, ifa, variant, None, (-15.0, -15.0), rec["map_t"]))
        recs.append(rec)
    return jobs, recs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", required=True, help="libfxjps.so built from the parent commit")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--shapes", nargs="+", default=["synth", "png"])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "crop_slots_bench.json"))
    a = ap.parse_args()
    import fuxi_planner_amd as fx
    from fuxi_planner_amd import _lib
    import fleet_tick_bench as ftb
    from world_slots_bench import Parent

    _lib.load()
    cropped, world, parent = fx.Planner([0]), fx.Planner([0]), Parent(a.parent_lib)
    assert parent.has_world and parent.version <= _lib.VERSION, (parent.version, _lib.VERSION)
    out = {"tool": "crop_slots_bench", "n": N, "reps": a.reps, "window_s": ftb.WINDOW_S, "ifa": 1, "map_reso": R, "message": [SIDE, SIDE],
           "parent_version": parent.version, "version": _lib.VERSION, "cases": []}
    ms = lambda ts: round(float(np.median(ts)) * 1e3, 4)
    spread = lambda ts: [round(min(ts) * 1e3, 4), round(max(ts) * 1e3, 4)]
    for shape in a.shapes:
        cjobs = message_fleet(shape, N)
        hjobs, recs = host_cropped(cjobs)
        # the same slots three ways, byte for byte, before anything is timed
        o_crop = cropped.prepare_slots_cropped(cjobs)
        o_world = world.prepare_slots_world(hjobs)
        parr, pkeep = fx.Planner._world_jobs(hjobs)
        assert parent.L.fxjps_prepare_slots_world(parent.h, parr, N) == 0
        assert [o[:-2] for o in o_crop] == o_world and all(o[5] for o in o_world), shape
        assert [tuple(j.goal_xy_cell) + (j.W, j.H, j.end_occu, j.status) for j in parr] == [tuple(o[1]) + tuple(o[3]) + (o[4], 0) for o in o_world], shape
        for v in range(N):
            rec = o_crop[v][-1]
            assert o_crop[v][-2] == 0 and all(list(rec[k]) == list(recs[v][k]) for k in ("bbox", "start0", "lo", "win")), (shape, v)
            assert np.array(rec["map_o"] + rec["map_t"]).tobytes() == np.array(recs[v]["map_o"] + recs[v]["map_t"]).tobytes(), (shape, v)
            g = cropped.get_grid_slot(v)
            assert g.tobytes() == world.get_grid_slot(v).tobytes() == parent.slot(v).tobytes(), (shape, v)
        carr, ckeep = fx.Planner._world_jobs(cjobs)
        warr, wkeep = fx.Planner._world_jobs(hjobs)
        crop_out = (_lib.Crop * N)()

        def side_cropped():
            arr, keep = fx.Planner._world_jobs(cjobs)
            assert cropped._L.fxjps_prepare_slots_cropped(cropped._h, arr, N, crop_out) == 0

        def side_host_parent():
            arr, keep = fx.Planner._world_jobs(host_cropped(cjobs)[0])
            assert parent.L.fxjps_prepare_slots_world(parent.h, arr, N) == 0

        def c_call(fn, h, arr, *more):
            assert fn(h, arr, N, *more) == 0

        sides = {"cropped": side_cropped, "host_parent_a": side_host_parent, "host_parent_b": side_host_parent,
                 "cropped_call": lambda: c_call(cropped._L.fxjps_prepare_slots_cropped, cropped._h, carr, crop_out),
                 "world_call": lambda: c_call(world._L.fxjps_prepare_slots_world, world._h, warr),
                 "parent_world_call": lambda: c_call(parent.L.fxjps_prepare_slots_world, parent.h, parr)}
        t, per = ftb.windows(sides, a.reps)
        med = {k: float(np.median(t[k])) for k in sides}
        aa = t["host_parent_a"] + t["host_parent_b"]
        aa_spread = max(aa) / min(aa) - 1.0
        cells = [o[3][0] * o[3][1] for o in o_world]
        case = {"shape": shape, "prepared_cells_min_max": [min(cells), max(cells)], "staged_bytes_cropped": int(sum(j[1].size for j in cjobs)),
                "staged_bytes_host": int(sum(j[1].size for j in hjobs)), "calls_per_window": per}
        for k in sides:
            case[k + "_ms"] = ms(t[k])
            case["spread_" + k + "_ms"] = spread(t[k])
        case["aa_spread"] = round(aa_spread, 4)
        case["cropped_over_host_parent"] = round(med["cropped"] / med["host_parent_a"], 4)
        case["world_call_over_parent_world_call"] = round(med["world_call"] / med["parent_world_call"], 4)
        case["bar_cropped_within_aa_spread_met"] = bool(med["cropped"] <= med["host_parent_a"] * (1.0 + aa_spread))
        case["bar_world_call_1_05_met"] = bool(med["world_call"] <= 1.05 * med["parent_world_call"])
        out["cases"].append(case)
    for p in (cropped, world, parent):
        p.close()
    line = json.dumps(out)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
