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

--stage waypoints: the waypoint third of the tick, one query per vehicle, the rules alternating
over the vehicles as the variants do.  loop: what a node ran before fxjps_waypoint_slots_batch existed, per vehicle
select_st, or get_grid_slot + select_ccst.  batch: ONE select_slots_batch on the resident paths.  Both sides' results are
compared byte for byte before anything is timed; the first batch call (it fills the table of angles) is reported apart.
For information the whole tick of three calls, and the same with the loop as its last third.  The bar: batch / loop <= 1/2
at n = 64 on `synth`.  With --trace-call N: prepare, plan, one warm batch call, a pause of 50 ms, then ONE batch call.

--stage publish: the publishing quarter of the tick, every vehicle's prepared map out of its slot
as the nav_msgs/OccupancyGrid data[] the nodes publish.  new: ONE publish_slots call, messages only.  loop: what a fleet host
writes without it, per vehicle get_grid_slot + the numpy lines of the reference's publish_map.  Both sides' outputs are
compared byte for byte before anything is timed.  At n = 64 also messages plus RGB snapshots both ways, and the whole tick
of four calls against the same tick with the loop as its last quarter and against the per-vehicle tick (all four stages
per vehicle).  The bar: new / loop <= 1/2 at n = 64 on `synth`.  The JSON line is also written to --out.

--stage outputs: what every node sends out per tick besides its map: the Point of /goal_global,
/jps_path and the ccst node's /direct_jps_path.  new: ONE tick_outputs_slots call on the resident paths.  loop: what a fleet
host writes without it, select_slots_batch on the same resident paths (with the kept cells) and then per vehicle the numpy lines of the nodes
(st:292-298, 335, 356-359; ccst:485, 487-495, 559-562, 590-593).  Both sides are compared byte for byte before anything is timed.
Also the whole tick of four calls both ways.  No bar is fixed; the JSON line is also written to --out.  With --trace-call N:
prepare, plan, one warm call, a pause of 50 ms, then ONE call.
Usage: python tools/fleet_tick_bench.py [--stage maps|waypoints|publish|outputs] [--reps 5] [--ns 16 64 256]"""
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


def waypoint_inputs(jobs, outs):
    """One query per vehicle: the keyword arguments of select_slots_batch on the paths of the tick's plan_batch_slots."""
    import fuxi_planner_amd as fx
    n = len(jobs)
    rng = np.random.default_rng(n)
    reso = np.array([(0.2, 0.5, 1.0)[v % 3] for v in range(n)])
    rule = np.array([j[5] for j in jobs], np.int32)
    s, g = np.array([o[0] for o in outs]), np.array([o[1] for o in outs])
    origin = np.array([fx.Planner.shifted_origin(rng.uniform(-20, 20, 2), o[2], r) for o, r in zip(outs, reso)])
    pos = np.c_[(s[:, 0] + 1) * reso + origin[:, 0] + rng.normal(0, 0.4, n), (s[:, 1] + 1 - rule) * reso + origin[:, 1] + rng.normal(0, 0.4, n),
                np.zeros(n)]
    goal = np.c_[(g[:, 0] + 1) * reso + origin[:, 0], (g[:, 1] + 1 - rule) * reso + origin[:, 1], np.full(n, 1.5)]
    return dict(rule=rule, map_start=s, map_reso=reso, map_o=origin, pos=pos, global_goal=goal, end_occu=np.array([o[4] for o in outs], np.int32))


def waypoints_loop(p, plan, a):
    """The per-vehicle loop: -> (wp [n, 3], valid components, goal [n, 3])"""
    from fuxi_planner_amd import waypoints
    off, cells, cost, st = plan
    n = len(st)
    wp, dim, gout = np.zeros((n, 3)), np.full(n, 3, np.int32), np.array(a["global_goal"])
    for v in range(n):
        if st[v] <= 0:
            wp[v] = a["global_goal"][v]
            continue
        path = cells[off[v]:off[v + 1]]
        if a["rule"][v] == 0:
            w, gout[v], _ = waypoints.select_st(path, a["map_start"][v], a["map_reso"][v], a["map_o"][v], a["pos"][v], a["global_goal"][v], a["end_occu"][v])
        else:
            w, _, gout[v] = waypoints.select_ccst(path, p.get_grid_slot(v), a["map_reso"][v], a["map_o"][v], a["pos"][v], a["global_goal"][v],
                                                  a["end_occu"][v], return_goal=True)
        wp[v, :len(w)] = w
        dim[v] = len(w)
    return wp, dim, gout


def waypoint_stage(p, a):
    from fuxi_planner_amd import waypoints
    ms = lambda ts: round(float(np.median(ts)) * 1e3, 4)
    spread = lambda ts: [round(min(ts) * 1e3, 4), round(max(ts) * 1e3, 4)]
    out = {"tool": "fleet_tick_bench", "stage": "waypoints", "reps": a.reps, "window_s": WINDOW_S, "ifa": 1, "cases": []}
    first_ms = None
    for shape in a.shapes:
        for n in a.ns:
            jobs = fleet(shape, n)
            outs = side_new(p, jobs)
            assert all(o[5] for o in outs), (shape, n)
            ids = np.arange(n, dtype=np.int32)
            starts, goals = [o[0] for o in outs], [o[1] for o in outs]
            plan = p.plan_batch_slots(ids, starts, goals, 2)
            inp = waypoint_inputs(jobs, outs)
            t0 = time.perf_counter()
            got = waypoints.select_slots_batch(p, **inp)
            first = (time.perf_counter() - t0) * 1e3
            if first_ms is None:
                first_ms = round(first, 4)  # (the process's first call: it fills the table of angles and loads the kernel)
            want = waypoints_loop(p, plan, inp)
            assert got[0].tobytes() == want[0].tobytes() and np.array_equal(got[1], want[1]) and got[2].tobytes() == want[2].tobytes(), (shape, n)
            tick = lambda: (side_new(p, jobs), p.plan_batch_slots(ids, starts, goals, 2))
            sides = {"batch": lambda: waypoints.select_slots_batch(p, **inp), "loop": lambda: waypoints_loop(p, plan, inp),
                     "tick_batch": lambda: (tick(), waypoints.select_slots_batch(p, **inp)),
                     "tick_loop": lambda: waypoints_loop(p, tick()[1], inp)}
            t, per = windows(sides, a.reps)
            case = {"shape": shape, "n": n, "planned": int((plan[3] > 0).sum()), "ccst": int((inp["rule"] == 1).sum()),
                    "path_points_max": int(plan[3].max()), "intermediate_wp": int((got[0][:, :2] != inp["global_goal"][:, :2]).any(1).sum()),
                    "calls_per_window": per, "batch_ms": ms(t["batch"]), "loop_ms": ms(t["loop"]),
                    "ratio": round(float(np.median(t["batch"]) / np.median(t["loop"])), 4), "spread_batch_ms": spread(t["batch"]),
                    "spread_loop_ms": spread(t["loop"]), "first_call_of_case_ms": round(first, 4), "tick_batch_ms": ms(t["tick_batch"]),
                    "tick_loop_ms": ms(t["tick_loop"]), "spread_tick_batch_ms": spread(t["tick_batch"]), "spread_tick_loop_ms": spread(t["tick_loop"]),
                    "batch_us_per_vehicle": round(float(np.median(t["batch"])) * 1e6 / n, 2),
                    "loop_us_per_vehicle": round(float(np.median(t["loop"])) * 1e6 / n, 2)}
            if shape == "synth" and n == 64:
                case["bar_half_met"] = bool(np.median(t["batch"]) <= 0.5 * np.median(t["loop"]))
            out["cases"].append(case)
    out["first_call_ms"] = first_ms
    print(json.dumps(out))


def publish_loop(p, n, rgb=False):
    """The per-vehicle loop: get_grid_slot, then publish_map (global_planner_st.py:103,109-115) and, with rgb, the snapshot
    (st:368-372) in numpy.  -> [(data int8[W*H], (W, H), image or None)]"""
    out = []
    for v in range(n):
        g = p.get_grid_slot(v)
        d = np.where(g == 1, 100, 0).astype(np.int8)
        img = None
        if rgb:
            img = np.where(g == 0, 255, 0).astype(np.uint8).T[::-1]
            img = np.repeat(img[:, :, None], 3, axis=2)
        out.append((d.T.reshape(-1), (g.shape[0], g.shape[1]), img))
    return out


def same_published(a, b):
    return len(a) == len(b) and all(x[0].tobytes() == y[0].tobytes() and tuple(x[1]) == tuple(y[1]) and (x[2] is None) == (y[2] is None)
                                    and (x[2] is None or (x[2].shape == y[2].shape and x[2].tobytes() == y[2].tobytes())) for x, y in zip(a, b))


def publish_stage(p, a):
    from fuxi_planner_amd import waypoints
    ms = lambda ts: round(float(np.median(ts)) * 1e3, 4)
    spread = lambda ts: [round(min(ts) * 1e3, 4), round(max(ts) * 1e3, 4)]
    out = {"tool": "fleet_tick_bench", "stage": "publish", "reps": a.reps, "window_s": WINDOW_S, "ifa": 1, "cases": []}
    for shape in a.shapes:
        for n in a.ns:
            jobs = fleet(shape, n)
            outs = side_new(p, jobs)
            assert all(o[5] for o in outs), (shape, n)
            slots = list(range(n))
            assert same_published(p.publish_slots(slots), publish_loop(p, n)), (shape, n)
            sides = {"new": lambda: p.publish_slots(slots), "loop": lambda: publish_loop(p, n)}
            if n == 64:
                assert same_published(p.publish_slots(slots, True, 3), publish_loop(p, n, True)), (shape, n)
                ids = np.arange(n, dtype=np.int32)
                starts, goals = [o[0] for o in outs], [o[1] for o in outs]
                inp = waypoint_inputs(jobs, outs)
                three = lambda: (side_new(p, jobs), p.plan_batch_slots(ids, starts, goals, 2), waypoints.select_slots_batch(p, **inp))
                sides.update({"new_rgb": lambda: p.publish_slots(slots, True, 3), "loop_rgb": lambda: publish_loop(p, n, True),
                              "tick_new": lambda: (three(), p.publish_slots(slots)), "tick_publish_loop": lambda: (three(), publish_loop(p, n)),
                              "tick_per_vehicle": lambda: (side_today(p, jobs), waypoints_loop(p, p.plan_batch_slots(ids, starts, goals, 2), inp),
                                                           publish_loop(p, n))})
            t, per = windows(sides, a.reps)
            cells = [o[3][0] * o[3][1] for o in outs]
            case = {"shape": shape, "n": n, "prepared_cells_min_max": [min(cells), max(cells)], "message_bytes": int(sum(cells)),
                    "calls_per_window": per, "new_ms": ms(t["new"]), "loop_ms": ms(t["loop"]),
                    "ratio": round(float(np.median(t["new"]) / np.median(t["loop"])), 4), "spread_new_ms": spread(t["new"]),
                    "spread_loop_ms": spread(t["loop"]), "new_us_per_vehicle": round(float(np.median(t["new"])) * 1e6 / n, 2),
                    "loop_us_per_vehicle": round(float(np.median(t["loop"])) * 1e6 / n, 2)}
            if n == 64:
                case.update({"new_rgb_ms": ms(t["new_rgb"]), "loop_rgb_ms": ms(t["loop_rgb"]),
                             "ratio_rgb": round(float(np.median(t["new_rgb"]) / np.median(t["loop_rgb"])), 4),
                             "spread_new_rgb_ms": spread(t["new_rgb"]), "spread_loop_rgb_ms": spread(t["loop_rgb"])})
                for k in ("tick_new", "tick_publish_loop", "tick_per_vehicle"):
                    case[k + "_ms"] = ms(t[k])
                    case["spread_" + k + "_ms"] = spread(t[k])
                case["publish_share_of_tick_new"] = round(float(np.median(t["new"]) / np.median(t["tick_new"])), 4)
                case["publish_loop_share_of_its_tick"] = round(float(np.median(t["loop"]) / np.median(t["tick_publish_loop"])), 4)
                if shape == "synth":
                    case["bar_half_met"] = bool(np.median(t["new"]) <= 0.5 * np.median(t["loop"]))
            out["cases"].append(case)
    line = json.dumps(out)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line)


def outputs_loop(p, plan, inp, home):
    """select_slots_batch, then the nodes' own numpy lines per vehicle.  -> (wp, dim, goal_out, point [n, 3], paths, dir_paths, dir_back)"""
    from fuxi_planner_amd import waypoints
    off, cells, cost, st = plan
    n = len(st)
    wps, dim, gout, ang, nk, kept = waypoints.select_slots_batch(p, paths=(off, None), return_kept=True, **inp)  # (the resident paths, as the tick runs it)
    point, paths, dirs, back = np.zeros((n, 3)), [], [], np.zeros(n, np.int32)
    with np.errstate(all="ignore"):
        for v in range(n):
            map_reso, map_o, ccst = inp["map_reso"][v], list(inp["map_o"][v]), inp["rule"][v] == 1
            px, py, pz = inp["pos"][v]
            xo, yo = home[v]
            wp, global_goal = wps[v, :dim[v]], gout[v]
            path3 = np.zeros((0, 3))
            path4 = None
            if st[v] > 0:
                path2 = cells[off[v]:off[v + 1]] + (np.array([1, 0]) if ccst else np.array([1, 1]))
                path3 = path2 * map_reso + map_o
                path3 = np.c_[path3, np.zeros([len(path3), 1])]
                if ccst:
                    path4 = (kept[off[v]:off[v] + nk[v]] + np.array([1, 0])) * map_reso + map_o
                    path4 = np.c_[path4, np.zeros([len(path4), 1])]
            elif ccst:
                path4 = np.array([[px, py, pz], wp])
                back[v] = 100
            if ccst and (np.linalg.norm(global_goal[0:2] - np.array([px, py])) < 0.5 or inp["end_occu"][v]):
                z = 0
            else:
                z = 1 + min(np.linalg.norm(wp[0:2] - np.array([xo, yo])) / np.linalg.norm(global_goal[0:2] - np.array([xo, yo])), 1) * (global_goal[2] - 1)
            point[v] = (wp[0], wp[1], z)
            paths.append(path3)
            dirs.append(np.zeros((0, 3)) if path4 is None else path4)
    return wps, dim, gout, point, paths, dirs, back


def outputs_stage(p, a):
    from fuxi_planner_amd import waypoints
    ms = lambda ts: round(float(np.median(ts)) * 1e3, 4)
    spread = lambda ts: [round(min(ts) * 1e3, 4), round(max(ts) * 1e3, 4)]
    out = {"tool": "fleet_tick_bench", "stage": "outputs", "reps": a.reps, "window_s": WINDOW_S, "ifa": 1, "cases": []}
    for shape in a.shapes:
        for n in a.ns:
            jobs = fleet(shape, n)
            outs = side_new(p, jobs)
            assert all(o[5] for o in outs), (shape, n)
            ids = np.arange(n, dtype=np.int32)
            slots = list(range(n))
            starts, goals = [o[0] for o in outs], [o[1] for o in outs]
            plan = p.plan_batch_slots(ids, starts, goals, 2)
            inp = waypoint_inputs(jobs, outs)
            home = inp["pos"][:, :2] + np.random.default_rng(n + 1).normal(0, 3.0, (n, 2))
            new = lambda off=plan[0]: waypoints.tick_outputs_slots(p, home=home, offsets=off, **inp)
            got, want = new(), outputs_loop(p, plan, inp, home)
            flat = lambda wp, dim, gout, point, paths, dirs, back: [wp, dim, gout, point, back] + list(paths) + list(dirs)
            a_, b_ = flat(got[0], got[1], got[2], got[5], got[6], got[7], got[8]), flat(*want)
            assert len(a_) == len(b_) and all(x.shape == y.shape and x.tobytes() == y.tobytes() for x, y in zip(a_, b_)), (shape, n)
            two = lambda: (side_new(p, jobs), p.plan_batch_slots(ids, starts, goals, 2))
            sides = {"new": new, "loop": lambda: outputs_loop(p, plan, inp, home),
                     "tick_new": lambda: (new(two()[1][0]), p.publish_slots(slots)),
                     "tick_loop": lambda: (outputs_loop(p, two()[1], inp, home), p.publish_slots(slots)),
                     "tick_without_outputs": lambda: (two(), waypoints.select_slots_batch(p, **inp), p.publish_slots(slots))}
            t, per = windows(sides, a.reps)
            case = {"shape": shape, "n": n, "planned": int((plan[3] > 0).sum()), "ccst": int((inp["rule"] == 1).sum()),
                    "path_points": int(plan[0][-1]), "calls_per_window": per, "new_ms": ms(t["new"]), "loop_ms": ms(t["loop"]),
                    "ratio": round(float(np.median(t["new"]) / np.median(t["loop"])), 4), "spread_new_ms": spread(t["new"]),
                    "spread_loop_ms": spread(t["loop"]), "new_us_per_vehicle": round(float(np.median(t["new"])) * 1e6 / n, 2),
                    "loop_us_per_vehicle": round(float(np.median(t["loop"])) * 1e6 / n, 2)}
            for k in ("tick_new", "tick_loop", "tick_without_outputs"):
                case[k + "_ms"] = ms(t[k])
                case["spread_" + k + "_ms"] = spread(t[k])
            case["new_faster_than_loop"] = bool(np.median(t["new"]) < np.median(t["loop"]))
            out["cases"].append(case)
    line = json.dumps(out)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line)


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
    ap.add_argument("--stage", choices=["maps", "waypoints", "publish", "outputs"], default="maps")
    ap.add_argument("--out", default=None, help="--stage publish / outputs: where the JSON line is written too (profiles/fleet_<stage>_bench.json)")
    a = ap.parse_args()
    if a.out is None:
        a.out = os.path.join(ROOT, "profiles", "fleet_%s_bench.json" % a.stage)
    import fuxi_planner_amd as fx

    p = fx.Planner([0])
    if a.stage == "publish":
        publish_stage(p, a)
        p.close()
        return
    if a.stage == "outputs":
        if a.trace_call:
            from fuxi_planner_amd import waypoints
            jobs = fleet(a.shape, a.trace_call)
            outs = side_new(p, jobs)
            plan = p.plan_batch_slots(np.arange(a.trace_call, dtype=np.int32), [o[0] for o in outs], [o[1] for o in outs], 2)
            inp = waypoint_inputs(jobs, outs)
            home = inp["pos"][:, :2] + 1.0
            waypoints.tick_outputs_slots(p, home=home, offsets=plan[0], **inp)
            time.sleep(0.05)
            got = waypoints.tick_outputs_slots(p, home=home, offsets=plan[0], **inp)
            print(json.dumps({"tool": "fleet_tick_bench", "stage": "outputs", "trace_call": a.trace_call, "shape": a.shape,
                              "planned": int((plan[3] > 0).sum()), "dir_points": int(sum(len(d) for d in got[7]))}))
        else:
            outputs_stage(p, a)
        p.close()
        return
    if a.stage == "waypoints":
        if a.trace_call:
            from fuxi_planner_amd import waypoints
            jobs = fleet(a.shape, a.trace_call)
            outs = side_new(p, jobs)
            plan = p.plan_batch_slots(np.arange(a.trace_call, dtype=np.int32), [o[0] for o in outs], [o[1] for o in outs], 2)
            inp = waypoint_inputs(jobs, outs)
            waypoints.select_slots_batch(p, **inp)
            time.sleep(0.05)
            got = waypoints.select_slots_batch(p, **inp)
            print(json.dumps({"tool": "fleet_tick_bench", "stage": "waypoints", "trace_call": a.trace_call, "shape": a.shape,
                              "planned": int((plan[3] > 0).sum()), "ccst_kept": int(got[4].sum())}))
        else:
            waypoint_stage(p, a)
        p.close()
        return
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
