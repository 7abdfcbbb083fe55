#!/usr/bin/env python3
"""A fleet's detected maps folded into a shared prior map that GROWS -> one JSON line, also written
to --out.

n = 64 vehicles, each with a `synth` 256 x 256 detected map at 20 % obstacles (tools/fleet_tick_bench.py's fleet), on one prior
map that all share and that starts at 400 x 400 and at 2048 x 2048 cells; resolution 0.25, every origin on its grid, mode
overwrite.  A ROUND is the start prior uploaded (not timed) and then --ticks calls, each a blocking call timed by itself: on
tick t the fleet is spread over the frame that reaches STEP * (t + 1) cells beyond the start prior on every side, vehicle 0 in
its low corner and vehicle 1 in its high corner, so that EVERY call grows the prior by STEP cells on all four sides and
moves its origin.  Sides, alternated round by round in one process, medians and ranges over the --reps x --ticks calls:
    grow         Planner.absorb_prior_grow: the job array filled from the world jobs, then fxjps_absorb_prior_grow
    grow_call    the C call alone on arrays filled beforehand
    host_route   what a host does without the call: Planner.get_prior_map (a blocking copy out), worldprep.grow_host per job
                 (numpy), Planner.set_prior_map with the larger array (a blocking copy in)
    host_copies  the two blocking copies of that route alone, at the extents the tick ends with, nothing folded
Before anything is timed one round of both routes is compared tick by tick: extents, origin and bytes.  --trace-call: ONE
round of `grow` and nothing else (for rocprofv3 --kernel-trace --stats).
Usage: python tools/grow_prior_bench.py [--reps 3] [--ticks 6] [--priors 400 2048]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
N = 64
R = 0.25
ORI_PRE = (-15.0, -15.0)
PRIOR = 0
STEP = 32


def origin_at(t):
    """The prior's origin before tick t: it has moved STEP cells down both axes on every tick before."""
    return (ORI_PRE[0] - STEP * t * R, ORI_PRE[1] - STEP * t * R)


def rounds(side, n, ticks):
    """-> (the start prior, per tick the list of world jobs, ori_pre as the prior lies before that tick)."""
    import fleet_tick_bench as ftb
    from fuxi_planner_amd import synth
    prior = synth.synth_grid(side, side, 4000, 0.20)
    base = ftb.fleet("synth", n)
    out = []
    for t in range(ticks):
        lo, span = -STEP * (t + 1), side + 2 * STEP * (t + 1)
        jobs = []
        for v, (slot, raw, start, goal, ifa, variant) in enumerate(base):
            room = span - raw.shape[0] + 1
            cx, cy = ((0, 0), (room - 1, room - 1))[v] if v < 2 else ((7 * v * span // 400) % room, (11 * v * span // 400) % room)
            map_o = (ORI_PRE[0] + (lo + cx) * R, ORI_PRE[1] + (lo + cy) * R)
            m = raw if t % 2 == 0 else np.ascontiguousarray(raw[::-1, ::-1])
            jobs.append((slot, m, map_o, R, map_o, map_o, ifa, variant, PRIOR, origin_at(t)))
        out.append(jobs)
    return prior, out


def host_tick(p, jobs):
    from fuxi_planner_amd import worldprep
    cur, at = p.get_prior_map(PRIOR), jobs[0][9]
    for j in jobs:
        cur, at, _, _, _ = worldprep.grow_host(cur, at, j[1], j[2], j[3], "overwrite")
    p.set_prior_map(PRIOR, cur)
    return cur, at


def job_array(jobs):
    """-> (the fxjps_grow_job_t array Planner.absorb_prior_grow would fill, what it points into)."""
    from fuxi_planner_amd import _lib
    arr = (_lib.GrowJob * len(jobs))()
    keep = []
    for a, j in zip(arr, jobs):
        raw = np.ascontiguousarray(np.asarray(j[1]) > 0, dtype=np.uint8)
        keep.append(raw)
        a.raw, a.layout, a.W0, a.H0, a.prior, a.map_reso = raw.ctypes.data, 0, raw.shape[0], raw.shape[1], j[8], j[3]
        for k in range(2):
            a.lo[k], a.win[k], a.map_o[k], a.ori_pre[k] = 0, raw.shape[k], j[2][k], j[9][k]
            a.map_t[k] = j[2][k] + raw.shape[k] * j[3]
    return arr, keep


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--ticks", type=int, default=6)
    ap.add_argument("--priors", type=int, nargs="+", default=[400, 2048])
    ap.add_argument("--trace-call", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "grow_prior_bench.json"))
    a = ap.parse_args()
    import fuxi_planner_amd as fx
    from fuxi_planner_amd import _lib

    out = {"tool": "grow_prior_bench", "n": N, "reps": a.reps, "ticks": a.ticks, "step_cells": STEP, "map_reso": R, "mode": "overwrite",
           "version": _lib.VERSION, "cases": []}
    ms = lambda ts: round(float(np.median(ts)) * 1e3, 4)
    spread = lambda ts: [round(min(ts) * 1e3, 4), round(max(ts) * 1e3, 4)]
    dev, host = fx.Planner([0]), fx.Planner([0])
    for side in a.priors:
        prior, ticks = rounds(side, N, a.ticks)
        if a.trace_call:
            dev.set_prior_map(PRIOR, prior)
            res = [dev.absorb_prior_grow(jobs)[1][PRIOR] for jobs in ticks]
            print(json.dumps({"tool": "grow_prior_bench", "trace_call": True, "prior": side, "grown": [[g["W"], g["H"]] for g in res]}))
            continue
        # the same extents, origins and bytes both ways, tick by tick, before anything is timed
        dev.set_prior_map(PRIOR, prior)
        host.set_prior_map(PRIOR, prior)
        extents, flips = [], []
        for t, jobs in enumerate(ticks):
            _, grown = dev.absorb_prior_grow(jobs)
            want, want_origin = host_tick(host, jobs)
            g = grown[PRIOR]
            got = dev.get_prior_map(PRIOR)
            assert got.shape == want.shape == (g["W"], g["H"]) == (side + 2 * STEP * (t + 1),) * 2, (side, t, got.shape, want.shape)
            assert tuple(g["origin"]) == tuple(want_origin) == origin_at(t + 1) and g["shift"] == (STEP, STEP), (side, t, g)
            assert got.tobytes() == want.tobytes() == host.get_prior_map(PRIOR).tobytes(), (side, t)
            extents.append([g["W"], g["H"]])
            flips.append(g["changed"])
        arrs = [job_array(jobs) for jobs in ticks]
        grown_out = (_lib.PriorGrown * _lib.MAX_PRIOR_MAPS)()
        blank = [np.zeros(e, dtype=np.uint8) for e in extents]

        def timed(fn):
            t0 = time.perf_counter()
            fn()
            return time.perf_counter() - t0

        def call(t):
            assert dev._L.fxjps_absorb_prior_grow(dev._h, arrs[t][0], N, _lib.ABSORB_OVERWRITE, None, grown_out) == 0 and grown_out[PRIOR].W == extents[t][0]

        def copies(t):
            host.get_prior_map(PRIOR)
            host.set_prior_map(PRIOR, blank[t])

        sides = {"grow": (dev, lambda t: dev.absorb_prior_grow(ticks[t])), "grow_call": (dev, call),
                 "host_route": (host, lambda t: host_tick(host, ticks[t])), "host_copies": (host, copies)}
        times = {k: [] for k in sides}
        for rep in range(a.reps + 1):  # (the first round warms every side up and is not counted)
            for k, (p, fn) in sides.items():
                p.set_prior_map(PRIOR, prior)
                ts = [timed(lambda: fn(t)) for t in range(a.ticks)]
                if rep:
                    times[k] += ts
        med = {k: float(np.median(times[k])) for k in sides}
        case = {"start_prior_shape": [side, side], "grown_shapes": extents, "detected_shape": [256, 256],
                "staged_raw_bytes": int(sum(j[1].size for j in ticks[0])), "cells_changed_per_call": flips}
        for k in sides:
            case[k + "_ms"] = ms(times[k])
            case["spread_" + k + "_ms"] = spread(times[k])
        case["host_route_over_grow"] = round(med["host_route"] / med["grow"], 2)
        case["host_copies_over_grow_call"] = round(med["host_copies"] / med["grow_call"], 2)
        out["cases"].append(case)
    dev.close()
    host.close()
    if a.trace_call:
        return
    line = json.dumps(out)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
