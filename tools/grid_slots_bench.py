#!/usr/bin/env python3
"""Grid slots on one handle -> one JSON line.

fleet: 16 different 1024^2 grids (20 % obstacles) x 625 queries -- ONE plan_batch_slots call against what a caller does
without slots: for each grid in turn set_grid, then plan_batch (only the 16 plan_batch calls are timed).  Beside it, the
same 10 000 queries' worth of plans/s on ONE grid (config 2's).
mg_overhead: the config-2 grid and its 10 000 queries in a slot (k_search<.., .., .., true>) against plan_batch on the
resident grid, the two alternated within this process; medians of the wall time of the calls.
Usage: python tools/grid_slots_bench.py [--reps 5]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn):
    t0 = time.perf_counter()
    r = fn()
    return time.perf_counter() - t0, r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    import fuxi_planner_amd as fx
    from fuxi_planner_amd import synth

    p = fx.Planner([0])
    out = {"tool": "grid_slots_bench", "reps": a.reps}
    # ---- fleet shape
    grids = [synth.synth_grid(1024, 1024, 1000 + i, 0.20) for i in range(16)]
    qs = [synth.synth_queries(occ, 1000 + i, 625) for i, occ in enumerate(grids)]
    for i, occ in enumerate(grids):
        p.set_grid_slot(i, occ)
    ids = np.concatenate([np.full(625, i, np.int32) for i in range(16)])
    s = np.concatenate([q[0] for q in qs])
    g = np.concatenate([q[1] for q in qs])

    def per_grid():
        t = 0.0
        res = []
        for occ, (qs_, qg_) in zip(grids, qs):
            p.set_grid_occ(occ)
            dt, r = timed(lambda: p.plan_batch(qs_, qg_, 2, 1024))
            t += dt
            res.append(r)
        return t, res

    p.plan_batch_slots(ids, s, g, 2, 1024)  # warm-up of both forms (code objects, scratch pools)
    per_grid()
    t_slots, t_seq = [], []
    for _ in range(a.reps):
        dt, rs = timed(lambda: p.plan_batch_slots(ids, s, g, 2, 1024))
        t_slots.append(dt)
        ts, rq = per_grid()
        t_seq.append(ts)
    # (the same answers both ways)
    for i in range(16):
        idx = np.flatnonzero(ids == i)
        assert np.array_equal(rs[3][idx], rq[i][3]) and rs[2][idx].tobytes() == rq[i][2].tobytes()
    ms_slots, ms_seq = float(np.median(t_slots)) * 1e3, float(np.median(t_seq)) * 1e3
    # the same number of queries on ONE grid (config 2's grid in a slot): what 16 distinct grids cost in cache
    occ2 = synth.synth_grid(1024, 1024, 1, 0.20)
    s2, g2 = synth.synth_queries(occ2, 1, 10000)
    p.set_grid_slot(16, occ2)
    one = np.full(10000, 16, np.int32)
    p.plan_batch_slots(one, s2, g2, 2, 1024)
    t_one = [timed(lambda: p.plan_batch_slots(one, s2, g2, 2, 1024))[0] for _ in range(a.reps)]
    ms_one = float(np.median(t_one)) * 1e3
    out["fleet"] = {"grids": 16, "queries": 10000, "slots_call_ms": round(ms_slots, 2), "per_grid_calls_ms": round(ms_seq, 2),
                    "ratio": round(ms_slots / ms_seq, 3), "bar_half_met": ms_slots <= 0.5 * ms_seq,
                    "plans_per_s_16_grids": round(10000 / (ms_slots / 1e3)), "plans_per_s_1_grid": round(10000 / (ms_one / 1e3))}
    # ---- the MG instantiation against the resident path: config 2, alternated
    p.set_grid_occ(occ2)
    p.plan_batch(s2, g2, 2, 1024)
    t_res, t_mg, k_res, k_mg = [], [], [], []
    for _ in range(a.reps):
        dt, r_res = timed(lambda: p.plan_batch(s2, g2, 2, 1024))
        t_res.append(dt)
        k_res.append(p.timing()["search_kernel_ms"])
        dt, r_mg = timed(lambda: p.plan_batch_slots(one, s2, g2, 2, 1024))
        t_mg.append(dt)
        k_mg.append(p.timing()["search_kernel_ms"])
    assert r_res[3].tobytes() == r_mg[3].tobytes() and r_res[2].tobytes() == r_mg[2].tobytes()
    assert np.array_equal(r_res[1], r_mg[1])
    ms_res, ms_mg = float(np.median(t_res)) * 1e3, float(np.median(t_mg)) * 1e3
    out["mg_overhead"] = {"queries": 10000, "resident_ms": round(ms_res, 2), "slot_ms": round(ms_mg, 2),
                          "resident_kernel_ms": round(float(np.median(k_res)), 2), "slot_kernel_ms": round(float(np.median(k_mg)), 2),
                          "overhead": round(ms_mg / ms_res - 1.0, 4), "bar_3pct_met": ms_mg <= 1.03 * ms_res,
                          "spread_resident_ms": [round(min(t_res) * 1e3, 2), round(max(t_res) * 1e3, 2)],
                          "spread_slot_ms": [round(min(t_mg) * 1e3, 2), round(max(t_mg) * 1e3, 2)]}
    p.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
