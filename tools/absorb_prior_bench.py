#!/usr/bin/env python3
"""A fleet's detected maps folded into the shared prior map -> one JSON line, also written to --out.

n = 64 vehicles, each with a `synth` 256 x 256 detected map at 20 % obstacles (tools/fleet_tick_bench.py's fleet) somewhere on
one prior map that all share, of 400 x 400 and of 2048 x 2048 cells; resolution 0.25, every origin on its grid, mode
overwrite.  Two fleets with different maps at the same places take turns call by call, so that every call flips cells and
stores bytes (the same fleet twice would find the prior as it leaves it).  Sides, alternated in one process (method of
tools/fleet_tick_bench.py: a repetition is a window of as many blocking calls as make a side run >= 0.2 s after a warm-up
call, medians of --reps windows, per call):
    absorb       Planner.absorb_prior: the job array filled from the world jobs, then fxjps_absorb_prior
    absorb_call  the C call alone on arrays filled beforehand
    host_route   what a host does without the call: Planner.get_prior_map (a blocking copy out), worldprep.absorb_host per
                 job (numpy), Planner.set_prior_map (a blocking copy in)
    host_copies  the two blocking copies of that route alone, nothing pasted
Before anything is timed the prior after one call of each fleet is compared byte for byte with the host route's, and so are
inside, outside and changed.  --trace-call: ONE call per fleet and nothing else (for rocprofv3 --kernel-trace --stats).
Usage: python tools/absorb_prior_bench.py [--reps 5] [--priors 400 2048]"""
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
ORI_PRE = (-15.0, -15.0)
PRIOR = 0


def fleets(side, n):
    """-> (the prior map, two lists of world jobs at the same places with different detected maps)."""
    import fleet_tick_bench as ftb
    from fuxi_planner_amd import synth
    prior = synth.synth_grid(side, side, 4000, 0.20)
    base = ftb.fleet("synth", n)
    out = ([], [])
    for v, (slot, raw, start, goal, ifa, variant) in enumerate(base):
        cx, cy = (7 * v * side // 400) % (side - raw.shape[0] + 1), (11 * v * side // 400) % (side - raw.shape[1] + 1)
        map_o = (ORI_PRE[0] + cx * R, ORI_PRE[1] + cy * R)
        for k, m in enumerate((raw, np.ascontiguousarray(raw[::-1, ::-1]))):
            out[k].append((slot, m, map_o, R, map_o, map_o, ifa, variant, PRIOR, ORI_PRE))
    return prior, out


def host_route(p, jobs):
    from fuxi_planner_amd import worldprep
    cur = p.get_prior_map(PRIOR)
    counts = []
    for j in jobs:
        cur, ins, outs, _ = worldprep.absorb_host(cur, j[9], j[1], j[2], j[3], "overwrite")
        counts.append((ins, outs))
    p.set_prior_map(PRIOR, cur)
    return cur, counts


def job_array(p, jobs):
    """-> (the fxjps_absorb_job_t array Planner.absorb_prior would fill, what it points into)."""
    from fuxi_planner_amd import _lib
    arr = (_lib.AbsorbJob * len(jobs))()
    keep = []
    for a, j in zip(arr, jobs):
        raw = np.ascontiguousarray(np.asarray(j[1]) > 0, dtype=np.uint8)
        keep.append(raw)
        a.raw, a.layout, a.W0, a.H0, a.prior, a.map_reso = raw.ctypes.data, 0, raw.shape[0], raw.shape[1], j[8], j[3]
        for k in range(2):
            a.lo[k], a.win[k], a.map_o[k], a.ori_pre[k] = 0, raw.shape[k], j[2][k], j[9][k]
    return arr, keep


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--priors", type=int, nargs="+", default=[400, 2048])
    ap.add_argument("--trace-call", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "absorb_prior_bench.json"))
    a = ap.parse_args()
    import fuxi_planner_amd as fx
    from fuxi_planner_amd import _lib
    import fleet_tick_bench as ftb

    out = {"tool": "absorb_prior_bench", "n": N, "reps": a.reps, "window_s": ftb.WINDOW_S, "map_reso": R, "mode": "overwrite",
           "version": _lib.VERSION, "cases": []}
    ms = lambda ts: round(float(np.median(ts)) * 1e3, 4)
    spread = lambda ts: [round(min(ts) * 1e3, 4), round(max(ts) * 1e3, 4)]
    dev, host = fx.Planner([0]), fx.Planner([0])
    for side in a.priors:
        prior, two = fleets(side, N)
        dev.set_prior_map(PRIOR, prior)
        if a.trace_call:
            res = [dev.absorb_prior(jobs) for jobs in two]
            print(json.dumps({"tool": "absorb_prior_bench", "trace_call": True, "prior": side, "changed": [r[1][PRIOR] for r in res]}))
            continue
        host.set_prior_map(PRIOR, prior)
        # the same bytes and counts both ways, before anything is timed
        flips = []
        for jobs in two:
            before = dev.get_prior_map(PRIOR)
            counts, changed = dev.absorb_prior(jobs)
            want, want_counts = host_route(host, jobs)
            assert dev.get_prior_map(PRIOR).tobytes() == want.tobytes() == host.get_prior_map(PRIOR).tobytes(), side
            assert counts == want_counts and changed[PRIOR] == int(np.count_nonzero((want != 0) != (before != 0))), side
            flips.append(changed[PRIOR])
        arrs = [job_array(dev, jobs) for jobs in two]
        changed = np.zeros(_lib.MAX_PRIOR_MAPS, dtype=np.int64)
        p_changed = changed.ctypes.data_as(C.POINTER(C.c_int64))
        turn = {"dev": 1, "host": 1}  # (per handle: every call pastes the fleet the call before it on that handle did not)

        def take(k):
            turn[k] ^= 1
            return turn[k]

        def side_call():
            arr = arrs[take("dev")][0]
            assert dev._L.fxjps_absorb_prior(dev._h, arr, N, _lib.ABSORB_OVERWRITE, p_changed) == 0 and changed[PRIOR] > 0

        def side_copies():
            host.set_prior_map(PRIOR, host.get_prior_map(PRIOR))

        sides = {"absorb": lambda: dev.absorb_prior(two[take("dev")]), "absorb_call": side_call,
                 "host_route": lambda: host_route(host, two[take("host")]), "host_copies": side_copies}
        t, per = ftb.windows(sides, a.reps)
        med = {k: float(np.median(t[k])) for k in sides}
        case = {"prior_shape": [side, side], "detected_shape": [256, 256], "staged_raw_bytes": int(sum(j[1].size for j in two[0])),
                "cells_flipped_per_call": flips, "calls_per_window": per}
        for k in sides:
            case[k + "_ms"] = ms(t[k])
            case["spread_" + k + "_ms"] = spread(t[k])
        case["host_route_over_absorb"] = round(med["host_route"] / med["absorb"], 2)
        case["host_copies_over_absorb_call"] = round(med["host_copies"] / med["absorb_call"], 2)
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
