#!/usr/bin/env python3
"""The map half of a fleet tick -> one JSON line.

n vehicles each deliver a RAW map; it has to end up padded, dilated and with its derived maps built in the vehicle's grid
slot.  new: ONE prepare_slots call.  today: what the library offered before that call existed, per vehicle prepare_grid
(resident) -> get_grid -> set_grid_slot.  For information: per vehicle set_grid_slot of prepared bytes the host already
holds, and the whole tick (maps + one plan_batch_slots with one query per vehicle) both ways.
n = 16, 64, 256; shapes: `synth` 256 x 256 raws at 20 % obstacles, `png` the reference's own maps; ifa = 1, the two
variants alternate over the vehicles.  Both sides' slots are compared byte for byte before anything is timed.  Sides are
alternated in one process; a repetition is a window of as many ticks as make a side run >= 0.2 s; medians of --reps
windows, per tick.  The bar: new / today <= 1/2 at n = 64 on `synth`.
--trace-call N [--shape S]: ONE prepare_slots call of N jobs and nothing else (for rocprofv3 --kernel-trace --stats).
Usage: python tools/fleet_tick_bench.py [--reps 5] [--ns 16 64 256]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
WINDOW_S = 0.2


def fleet(shape, n):
    """-> jobs [(slot, raw, start, goal, ifa, variant)] of n vehicles."""
    from fuxi_planner_amd import synth
    if shape == "synth":
        raws = [synth.synth_grid(256, 256, 2000 + v, 0.20) for v in range(n)]
    else:
        z = np.load(os.path.join(ROOT, "tests", "golden", "maps_png.npz"))
        with open(os.path.join(ROOT, "tests", "golden", "maps_png.json")) as f:
            shapes = {r["map"]: r["shape"] for r in json.load(f) if "canvas" not in r}
        maps = [np.unpackbits(z[nm])[:shapes[nm][0] * shapes[nm][1]].reshape(shapes[nm]).astype(np.uint8) for nm in sorted(z.files)]
        raws = [maps[v % len(maps)] for v in range(n)]
    jobs = []
    for v, raw in enumerate(raws):
        s, g = synth.synth_queries(raw, 3000 + v, 1)
        jobs.append((v, raw, tuple(int(c) for c in s[0]), tuple(int(c) for c in g[0]), 1, v & 1))
    return jobs


def side_new(p, jobs):
    return p.prepare_slots(jobs)


def side_today(p, jobs):
    outs = []
    for slot, raw, start, goal, ifa, variant in jobs:
        o = p.prepare_grid(raw, start, goal, ifa, variant)
        p.set_grid_slot(slot, p.get_grid())
        outs.append(o)
    return outs


def slots_bytes(p, n, maps):
    out = []
    for v in range(n):
        out.append(p.get_grid_slot(v).tobytes())
        if maps:
            m = p.debug_slot_maps(v)
            out += [m[k].tobytes() for k in sorted(m)]
    return out


def windows(sides, reps):
    """sides: {name: fn}.  -> {name: [seconds per call, one per window]}; the sides alternate window by window."""
    per = {}
    for name, fn in sides.items():  # warm-up, and how many calls fill a window
        fn()
        t0 = time.perf_counter()
        fn()
        per[name] = max(1, int(np.ceil(WINDOW_S / max(time.perf_counter() - t0, 1e-6))))
    out = {name: [] for name in sides}
    for _ in range(reps):
        for name, fn in sides.items():
            t0 = time.perf_counter()
            for _ in range(per[name]):
                fn()
            out[name].append((time.perf_counter() - t0) / per[name])
    return out, per


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--ns", type=int, nargs="+", default=[16, 64, 256])
    ap.add_argument("--shapes", nargs="+", default=["synth", "png"])
    ap.add_argument("--trace-call", type=int, default=0)
    ap.add_argument("--shape", default="synth")
    a = ap.parse_args()
    import fuxi_planner_amd as fx

    p = fx.Planner([0])
    if a.trace_call:
        outs = p.prepare_slots(fleet(a.shape, a.trace_call))
        print(json.dumps({"tool": "fleet_tick_bench", "trace_call": a.trace_call, "shape": a.shape, "ok": sum(o[5] for o in outs)}))
        p.close()
        return
    out = {"tool": "fleet_tick_bench", "reps": a.reps, "window_s": WINDOW_S, "ifa": 1, "cases": []}
    ms = lambda ts: round(float(np.median(ts)) * 1e3, 4)
    spread = lambda ts: [round(min(ts) * 1e3, 4), round(max(ts) * 1e3, 4)]
    for shape in a.shapes:
        for n in a.ns:
            jobs = fleet(shape, n)
            # the same slots both ways, byte for byte (occupancy and all six derived arrays), before anything is timed
            o_today = side_today(p, jobs)
            b_today = slots_bytes(p, n, True)
            for v in range(n):
                p.clear_grid_slot(v)
            o_new = side_new(p, jobs)
            assert all(o[5] for o in o_new) and [o[:5] for o in o_new] == o_today, (shape, n)
            assert slots_bytes(p, n, True) == b_today, (shape, n)
            prepared = [p.get_grid_slot(v) for v in range(n)]
            ids = np.arange(n, dtype=np.int32)
            starts, goals = [o[0] for o in o_new], [o[1] for o in o_new]
            plan = lambda: p.plan_batch_slots(ids, starts, goals, 2)
            sides = {"new": lambda: side_new(p, jobs), "today": lambda: side_today(p, jobs),
                     "set_only": lambda: [p.set_grid_slot(v, occ) for v, occ in enumerate(prepared)],
                     "tick_new": lambda: (side_new(p, jobs), plan()), "tick_today": lambda: (side_today(p, jobs), plan())}
            t, per = windows(sides, a.reps)
            cells = [o[3][0] * o[3][1] for o in o_new]
            case = {"shape": shape, "n": n, "prepared_cells_min_max": [min(cells), max(cells)], "calls_per_window": per,
                    "new_ms": ms(t["new"]), "today_ms": ms(t["today"]), "ratio": round(float(np.median(t["new"]) / np.median(t["today"])), 4),
                    "spread_new_ms": spread(t["new"]), "spread_today_ms": spread(t["today"]),
                    "set_only_ms": ms(t["set_only"]), "tick_new_ms": ms(t["tick_new"]), "tick_today_ms": ms(t["tick_today"]),
                    "new_us_per_vehicle": round(float(np.median(t["new"])) * 1e6 / n, 2),
                    "today_us_per_vehicle": round(float(np.median(t["today"])) * 1e6 / n, 2)}
            if shape == "synth" and n == 64:
                case["bar_half_met"] = bool(np.median(t["new"]) <= 0.5 * np.median(t["today"]))
            out["cases"].append(case)
    p.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
