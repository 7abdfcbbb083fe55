#!/usr/bin/env python3
"""A fleet's detected maps folded into a shared prior map that SLIDES along with the fleet -> one
JSON line, also written to --out.

tools/grow_prior_bench.py's shapes: n = 64 vehicles, each with a `synth` 256 x 256 detected map at 20 % obstacles, on one
prior map that all share and that starts at 400 x 400 and at 2048 x 2048 cells; resolution 0.25, every origin on its grid,
mode overwrite.  A ROUND is the start prior uploaded (not timed) and then --ticks calls, each a blocking call timed by
itself: on tick t the fleet has drifted STEP = 32 cells up both axes, its box reaching from MARGIN cells inside the frame
[STEP * (t + 1), STEP * (t + 1) + side) to that frame's top, vehicle 0 in the box's low corner and vehicle 1 in its high
corner.  The keep window is the fleet's box plus MARGIN on every side, i.e. that frame (the margin above the box holds no
cell yet), so EVERY call grows the prior by STEP cells at the top, cuts STEP cells at the bottom (use "always") and moves
its origin, and the prior's size stays what it was.  Sides, alternated round by round in one process, medians and ranges
over the --reps x --ticks calls:
    slide        Planner.absorb_prior_slide: the job array filled from the world jobs, then fxjps_absorb_prior_slide
    slide_call   the C call alone on arrays filled beforehand
    grow_call    fxjps_absorb_prior_grow alone on the same arrays: the prior grows by STEP cells a tick and is never cut
    host_route   what a host does without the call: Planner.get_prior_map (a blocking copy out), worldprep.slide_host
                 (numpy), Planner.set_prior_map (a blocking copy in)
    host_copies  the two blocking copies of that route alone, nothing folded
Before anything is timed one round of every route is compared tick by tick: extents, origin and bytes (the grown prior's
through its slice).  --grow-only: the grow_call side alone, through nothing newer than header version 860, so that with
--tree it runs on a checkout of the commit before fxjps_absorb_prior_slide; its JSON goes into a full run as --parent-grow.
--trace-call: ONE round of `slide` and nothing else (for rocprofv3 --kernel-trace --stats).
Usage: python tools/slide_prior_bench.py [--reps 3] [--ticks 6] [--priors 400 2048] [--parent-grow FILE]"""
import argparse
import json
import os
import sys
import time

import numpy as np

N = 64
R = 0.25
ORI_PRE = (-15.0, -15.0)
PRIOR = 0
STEP = 32
MARGIN = 16
INF = float("inf")


def origin_at(t):
    """The slid prior's origin before tick t: it has moved STEP cells up both axes on every tick before."""
    return (ORI_PRE[0] + STEP * t * R, ORI_PRE[1] + STEP * t * R)


def rounds(side, n, ticks, slid=True):
    """-> (the start prior, per tick the list of world jobs -- ori_pre as the prior lies before that tick: slid along, or
    never moved (a prior that only grows at its top keeps its origin) --, per tick the keep window)."""
    import fleet_tick_bench as ftb
    from fuxi_planner_amd import synth
    prior = synth.synth_grid(side, side, 4000, 0.20)
    base = ftb.fleet("synth", n)
    out, keeps = [], []
    for t in range(ticks):
        lo, span = STEP * (t + 1) + MARGIN, side - MARGIN  # the fleet's box, in cells of the start prior
        jobs = []
        for v, (slot, raw, start, goal, ifa, variant) in enumerate(base):
            room = span - raw.shape[0] + 1
            cx, cy = ((0, 0), (room - 1, room - 1))[v] if v < 2 else ((7 * v * span // 400) % room, (11 * v * span // 400) % room)
            map_o = (ORI_PRE[0] + (lo + cx) * R, ORI_PRE[1] + (lo + cy) * R)
            m = raw if t % 2 == 0 else np.ascontiguousarray(raw[::-1, ::-1])
            jobs.append((slot, m, map_o, R, map_o, map_o, ifa, variant, PRIOR, origin_at(t) if slid else ORI_PRE))
        out.append(jobs)
        box_lo = [ORI_PRE[k] + lo * R for k in range(2)]
        box_hi = [ORI_PRE[k] + (lo + span) * R for k in range(2)]
        keeps.append({PRIOR: (tuple(x - MARGIN * R for x in box_lo), tuple(x + MARGIN * R for x in box_hi))})
    return prior, out, keeps


def host_tick(p, jobs, keep):
    from fuxi_planner_amd import worldprep
    after, recs, _ = worldprep.slide_host({PRIOR: p.get_prior_map(PRIOR)}, jobs, "overwrite", keep=keep, use="always")
    p.set_prior_map(PRIOR, after[PRIOR])
    return after[PRIOR], recs[PRIOR]


def job_array(jobs):
    """-> (the fxjps_grow_job_t array Planner.absorb_prior_slide would fill, what it points into)."""
    from fuxi_planner_amd import _lib
    arr = (_lib.GrowJob * len(jobs))()
    alive = []
    for a, j in zip(arr, jobs):
        raw = np.ascontiguousarray(np.asarray(j[1]) > 0, dtype=np.uint8)
        alive.append(raw)
        a.raw, a.layout, a.W0, a.H0, a.prior, a.map_reso = raw.ctypes.data, 0, raw.shape[0], raw.shape[1], j[8], j[3]
        for k in range(2):
            a.lo[k], a.win[k], a.map_o[k], a.ori_pre[k] = 0, raw.shape[k], j[2][k], j[9][k]
            a.map_t[k] = j[2][k] + raw.shape[k] * j[3]
    return arr, alive


def keep_array(keep):
    from fuxi_planner_amd import _lib
    arr = (_lib.PriorKeep * _lib.MAX_PRIOR_MAPS)()
    for p, (lo, hi) in keep.items():
        arr[p].use = _lib.KEEP_ALWAYS
        for k in range(2):
            arr[p].lo[k], arr[p].hi[k] = lo[k], hi[k]
    return arr


def timed(fn):
    t0 = time.perf_counter()
    fn()
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--ticks", type=int, default=6)
    ap.add_argument("--priors", type=int, nargs="+", default=[400, 2048])
    ap.add_argument("--trace-call", action="store_true")
    ap.add_argument("--grow-only", action="store_true")
    ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--parent-grow", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    sys.path.insert(0, a.tree)
    sys.path.insert(0, os.path.join(a.tree, "tools"))
    import fuxi_planner_amd as fx
    from fuxi_planner_amd import _lib

    out = {"tool": "slide_prior_bench", "n": N, "reps": a.reps, "ticks": a.ticks, "step_cells": STEP, "margin_cells": MARGIN, "map_reso": R,
           "mode": "overwrite", "version": _lib.VERSION, "cases": []}
    ms = lambda ts: round(float(np.median(ts)) * 1e3, 4)
    spread = lambda ts: [round(min(ts) * 1e3, 4), round(max(ts) * 1e3, 4)]
    parent = {c["start_prior_shape"][0]: c for c in json.load(open(a.parent_grow))["cases"]} if a.parent_grow else {}
    dev, host, grow = fx.Planner([0]), fx.Planner([0]), fx.Planner([0])
    for side in a.priors:
        prior, ticks, keeps = rounds(side, N, a.ticks)
        _, still, _ = rounds(side, N, a.ticks, slid=False)
        grow_arrs = [job_array(jobs) for jobs in still]
        grown_out = (_lib.PriorGrown * _lib.MAX_PRIOR_MAPS)()

        def grow_call(t):
            assert grow._L.fxjps_absorb_prior_grow(grow._h, grow_arrs[t][0], N, _lib.ABSORB_OVERWRITE, None, grown_out) == 0
            assert grown_out[PRIOR].W == side + STEP * (t + 1)

        if a.grow_only:
            times = []
            for rep in range(a.reps + 1):  # (the first round warms up and is not counted)
                grow.set_prior_map(PRIOR, prior)
                ts = [timed(lambda: grow_call(t)) for t in range(a.ticks)]
                if rep:
                    times += ts
            out["cases"].append({"start_prior_shape": [side, side], "grow_call_ms": ms(times), "spread_grow_call_ms": spread(times)})
            continue
        if a.trace_call:
            dev.set_prior_map(PRIOR, prior)
            res = [dev.absorb_prior_slide(jobs, keep=keep, use="always")[1][PRIOR] for jobs, keep in zip(ticks, keeps)]
            print(json.dumps({"tool": "slide_prior_bench", "trace_call": True, "prior": side, "slid": [[g["W"], g["H"]] for g in res]}))
            continue
        # the same extents, origins and bytes every way, tick by tick, before anything is timed
        for p in (dev, host, grow):
            p.set_prior_map(PRIOR, prior)
        flips, inside = [], []
        for t, (jobs, keep) in enumerate(zip(ticks, keeps)):
            per_job, slid = dev.absorb_prior_slide(jobs, keep=keep, use="always")
            want, want_rec = host_tick(host, jobs, keep)
            g = slid[PRIOR]
            got = dev.get_prior_map(PRIOR)
            assert got.shape == want.shape == (g["W"], g["H"]) == (side, side), (side, t, got.shape, want.shape)
            assert g == want_rec and tuple(g["origin"]) == origin_at(t + 1) and g["shift"] == (-STEP, -STEP) and g["cut_lo"] == (STEP, STEP), (side, t, g)
            assert got.tobytes() == want.tobytes() == host.get_prior_map(PRIOR).tobytes(), (side, t)
            grow_call(t)   # ... and the prior that only grows holds the same bytes in the cells the slid one kept
            whole = grow.get_prior_map(PRIOR)
            assert whole[STEP * (t + 1):, STEP * (t + 1):].tobytes() == got.tobytes(), (side, t, whole.shape)
            flips.append(g["changed"])
            inside.append(int(sum(j[1] for j in per_job)))
        arrs = [job_array(jobs) for jobs in ticks]
        wins = [keep_array(keep) for keep in keeps]
        slid_out = (_lib.PriorSlid * _lib.MAX_PRIOR_MAPS)()
        blank = np.zeros((side, side), dtype=np.uint8)

        def call(t):
            assert dev._L.fxjps_absorb_prior_slide(dev._h, arrs[t][0], N, _lib.ABSORB_OVERWRITE, None, wins[t], slid_out) == 0 and slid_out[PRIOR].W == side

        def copies(t):
            host.get_prior_map(PRIOR)
            host.set_prior_map(PRIOR, blank)

        sides = {"slide": (dev, lambda t: dev.absorb_prior_slide(ticks[t], keep=keeps[t], use="always")), "slide_call": (dev, call), "grow_call": (grow, grow_call),
                 "host_route": (host, lambda t: host_tick(host, ticks[t], keeps[t])), "host_copies": (host, copies)}
        times = {k: [] for k in sides}
        for rep in range(a.reps + 1):  # (the first round warms every side up and is not counted)
            for k, (p, fn) in sides.items():
                p.set_prior_map(PRIOR, prior)
                ts = [timed(lambda: fn(t)) for t in range(a.ticks)]
                if rep:
                    times[k] += ts
        med = {k: float(np.median(times[k])) for k in sides}
        case = {"start_prior_shape": [side, side], "slid_shape": [side, side], "grown_shapes": [[side + STEP * (t + 1)] * 2 for t in range(a.ticks)],
                "detected_shape": [256, 256], "staged_raw_bytes": int(sum(j[1].size for j in ticks[0])), "cells_inside_per_call": inside,
                "cells_changed_per_call": flips}
        for k in sides:
            case[k + "_ms"] = ms(times[k])
            case["spread_" + k + "_ms"] = spread(times[k])
        if side in parent:
            case["grow_call_parent_ms"] = parent[side]["grow_call_ms"]
            case["spread_grow_call_parent_ms"] = parent[side]["spread_grow_call_ms"]
        case["host_route_over_slide"] = round(med["host_route"] / med["slide"], 2)
        case["host_copies_over_slide_call"] = round(med["host_copies"] / med["slide_call"], 2)
        case["grow_call_over_slide_call"] = round(med["grow_call"] / med["slide_call"], 2)
        out["cases"].append(case)
    for p in (dev, host, grow):
        p.close()
    if a.trace_call:
        return
    line = json.dumps(out)
    if a.out is None and not a.grow_only:
        a.out = os.path.join(a.tree, "profiles", "slide_prior_bench.json")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
