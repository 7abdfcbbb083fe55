#!/usr/bin/env python3
"""The map half of a fleet tick from world-frame jobs -> one JSON line, also written to --out.

n = 64 vehicles, each with a detected map inside one prior map that all share: `synth` 256 x 256 raws at 20 % obstacles in a
400 x 400 prior, `png` the reference's own maps with a prior 144 cells larger around them; ifa = 1, the variants alternate,
resolution 0.25, every origin on its grid.  Sides, alternated in one process (method of tools/fleet_tick_bench.py: a
repetition is a window of as many calls as make a side run >= 0.2 s, medians of --reps windows, per call):
    world        Planner._world_jobs + fxjps_prepare_slots_world: what a fleet host runs per tick with this library
    host_parent  worldprep.merge_host per vehicle + Planner._slot_jobs + fxjps_prepare_slots of the PARENT commit's library
                 (--parent-lib) on the canvases: what it ran before.  Build the parent from a checkout into a scratch directory:
                     git worktree add /tmp/parent HEAD~1 && make -C /tmp/parent/fuxi-planner_amd libfxjps.so
    world_call, parent, this   the C call alone on arrays filled beforehand: fxjps_prepare_slots_world, and fxjps_prepare_slots
                 of the parent's and of this library on the same canvases
    world_refresh_call   fxjps_refresh_slots_world on the same jobs call after call: every slot is compared and kept
    parent_world_call, parent_world_refresh_call   the two world calls of the parent's library, where it has them (a change
                 that leaves the calls as they are -- a refactor -- is measured against these sides)
Before anything is timed every slot's bytes and the per-job outputs are compared across the three handles, and the six
derived arrays between the two handles of this library.  Bars: world <= 1.0 x host_parent; this <= 1.05 x parent.
--trace-call N --side world|canvas: ONE call of N jobs and nothing else (for rocprofv3 --kernel-trace --stats).
--fold-trace NAME=DIR (repeatable): put the kernels of such a run's *kernel_stats.csv under DIR into the JSON.
Usage: python tools/world_slots_bench.py --parent-lib /tmp/parent/fuxi-planner_amd/libfxjps.so [--reps 5] [--shapes synth png]"""
import argparse
import csv
import ctypes as C
import glob
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


class Parent(object):
    """A handle of the parent's library through prototypes of its own (it is older than the binding)."""

    def __init__(self, lib_path):
        from fuxi_planner_amd import _lib
        self.L = L = C.CDLL(lib_path)
        vp, i32 = C.c_void_p, C.c_int32
        L.fxjps_create.argtypes = [C.c_int, C.POINTER(C.c_int), C.c_int, C.POINTER(vp)]
        L.fxjps_destroy.restype = None
        L.fxjps_destroy.argtypes = [vp]
        L.fxjps_last_error.restype = C.c_char_p
        L.fxjps_last_error.argtypes = [vp]
        L.fxjps_prepare_slots.argtypes = [vp, C.POINTER(_lib.SlotJob), i32]
        L.fxjps_get_grid_slot.argtypes = [vp, i32, vp, vp, vp]
        self.has_world = hasattr(L, "fxjps_prepare_slots_world") and L.fxjps_world_job_size() == C.sizeof(_lib.WorldJob)
        if self.has_world:
            L.fxjps_set_prior_map.argtypes = [vp, i32, vp, i32, i32]
            L.fxjps_prepare_slots_world.argtypes = [vp, C.POINTER(_lib.WorldJob), i32]
            L.fxjps_refresh_slots_world.argtypes = [vp, C.POINTER(_lib.WorldJob), i32, C.POINTER(i32)]
        assert L.fxjps_slot_job_size() == C.sizeof(_lib.SlotJob), lib_path
        self.version = L.fxjps_version()
        self.h = vp()
        ids = (C.c_int * 1)(0)
        rc = L.fxjps_create(_lib.BACKEND_HIP, ids, 1, C.byref(self.h))
        assert rc == 0, (lib_path, rc, L.fxjps_last_error(None))

    def prepare(self, arr, n):
        assert self.L.fxjps_prepare_slots(self.h, arr, n) == 0, self.L.fxjps_last_error(self.h)

    def set_prior(self, prior, occ):
        assert self.L.fxjps_set_prior_map(self.h, prior, occ.ctypes.data_as(C.c_void_p), occ.shape[0], occ.shape[1]) == 0, self.L.fxjps_last_error(self.h)

    def slot(self, s):
        W, H = C.c_int32(), C.c_int32()
        assert self.L.fxjps_get_grid_slot(self.h, s, None, C.byref(W), C.byref(H)) == 0
        out = np.empty((W.value, H.value), np.uint8)
        assert self.L.fxjps_get_grid_slot(self.h, s, out.ctypes.data_as(C.c_void_p), None, None) == 0
        return out

    def close(self):
        self.L.fxjps_destroy(self.h)


def world_fleet(shape, n):
    """-> (the prior map, world jobs as Planner.prepare_slots_world takes them)."""
    import fleet_tick_bench as ftb
    from fuxi_planner_amd import synth
    jobs = ftb.fleet(shape, n)
    mw, mh = max(j[1].shape[0] for j in jobs), max(j[1].shape[1] for j in jobs)
    prior = synth.synth_grid(mw + 144, mh + 144, 4000, 0.20)
    out = []
    for v, (slot, raw, start, goal, ifa, variant) in enumerate(jobs):
        cx, cy = (7 * v) % (prior.shape[0] - raw.shape[0] + 1), (11 * v) % (prior.shape[1] - raw.shape[1] + 1)
        map_o = (ORI_PRE[0] + cx * R, ORI_PRE[1] + cy * R)
        pos = (map_o[0] + (start[0] + 0.5) * R, map_o[1] + (start[1] + 0.5) * R)
        goal_xy = (map_o[0] + (goal[0] + 0.5) * R, map_o[1] + (goal[1] + 0.5) * R)
        out.append((slot, raw, map_o, R, pos, goal_xy, ifa, variant, PRIOR, ORI_PRE))
    return prior, out


def host_jobs(wjobs, prior):
    from fuxi_planner_amd import worldprep
    out = []
    for slot, raw, map_o, reso, pos, goal, ifa, variant, _, ori_pre in wjobs:
        canvas, _, _, s, g = worldprep.merge_host(raw, map_o, reso, pos, goal, prior=prior, ori_pre=ori_pre)
        out.append((slot, canvas, s, g, ifa, variant))
    return out


def fold_trace(d):
    """{kernel: [calls, average us]} of the fx:: kernels in the *kernel_stats.csv files under d."""
    out = {}
    for path in sorted(glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)):
        with open(path) as f:
            for row in csv.DictReader(f):
                if "fx::" in row["Name"]:
                    name = row["Name"].split("fx::")[1].split("(")[0]
                    out[name] = [int(row["Calls"]), round(float(row["AverageNs"]) / 1e3, 2)]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", help="libfxjps.so built from the parent commit")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--shapes", nargs="+", default=["synth", "png"])
    ap.add_argument("--trace-call", type=int, default=0)
    ap.add_argument("--side", choices=["world", "canvas"], default="world")
    ap.add_argument("--shape", default="synth")
    ap.add_argument("--fold-trace", action="append", default=[], metavar="NAME=DIR")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "world_slots_bench.json"))
    a = ap.parse_args()
    import fuxi_planner_amd as fx
    from fuxi_planner_amd import _lib
    import fleet_tick_bench as ftb

    if a.trace_call:
        prior, wjobs = world_fleet(a.shape, a.trace_call)
        with fx.Planner([0]) as p:
            if a.side == "world":
                p.set_prior_map(PRIOR, prior)
                outs = p.prepare_slots_world(wjobs)
            else:
                outs = p.prepare_slots(host_jobs(wjobs, prior))
        print(json.dumps({"tool": "world_slots_bench", "trace_call": a.trace_call, "side": a.side, "shape": a.shape, "ok": sum(o[5] for o in outs)}))
        return
    if not a.parent_lib:
        ap.error("--parent-lib is required")
    _lib.load()
    world, this, parent = fx.Planner([0]), fx.Planner([0]), Parent(a.parent_lib)
    assert parent.version <= _lib.VERSION, (parent.version, _lib.VERSION)
    # (the world calls of the parent and the two refreshing sides: handles of their own, so that every side's slots hold what its own calls left)
    parent_world = Parent(a.parent_lib) if parent.has_world else None
    parent_world_refresh = Parent(a.parent_lib) if parent.has_world else None
    world_refresh = fx.Planner([0])
    out = {"tool": "world_slots_bench", "n": N, "reps": a.reps, "window_s": ftb.WINDOW_S, "ifa": 1, "map_reso": R,
           "parent_version": parent.version, "version": _lib.VERSION, "cases": []}
    ms = lambda ts: round(float(np.median(ts)) * 1e3, 4)
    spread = lambda ts: [round(min(ts) * 1e3, 4), round(max(ts) * 1e3, 4)]
    for shape in a.shapes:
        prior, wjobs = world_fleet(shape, N)
        world.set_prior_map(PRIOR, prior)
        world_refresh.set_prior_map(PRIOR, prior)
        for p in (parent_world, parent_world_refresh):
            if p is not None:
                p.set_prior(PRIOR, np.ascontiguousarray(prior > 0, dtype=np.uint8))
        hjobs = host_jobs(wjobs, prior)
        # the same slots three ways, byte for byte, before anything is timed
        o_world = world.prepare_slots_world(wjobs)
        o_this = this.prepare_slots(hjobs)
        harr, hkeep = fx.Planner._slot_jobs(hjobs)
        first = (_lib.SlotJob * N)()
        C.memmove(first, harr, C.sizeof(first))
        parent.prepare(first, N)
        assert [o[:6] for o in o_world] == o_this == fx.Planner._slot_outs(first, N) and all(o[5] for o in o_this), shape
        for v in range(N):
            g = world.get_grid_slot(v)
            assert g.tobytes() == this.get_grid_slot(v).tobytes() == parent.slot(v).tobytes(), (shape, v)
            m, m2 = world.debug_slot_maps(v), this.debug_slot_maps(v)
            assert all(m[k].tobytes() == m2[k].tobytes() for k in m2), (shape, v)
        warr, wkeep = fx.Planner._world_jobs(wjobs)

        def side_world():
            arr, keep = fx.Planner._world_jobs(wjobs)
            assert world._L.fxjps_prepare_slots_world(world._h, arr, N) == 0

        def side_host_parent():
            arr, keep = fx.Planner._slot_jobs(host_jobs(wjobs, prior))
            parent.prepare(arr, N)

        def c_call(fn, h, arr):
            assert fn(h, arr, N) == 0

        # (fxjps_slot_job_t's start and goal are in / out: every call gets the job table as it was; the world job's
        # inputs are not written)
        work = {k: (_lib.SlotJob * N)() for k in ("parent", "this")}

        def canvas_call(k, fn, h):
            C.memmove(work[k], harr, C.sizeof(work[k]))
            assert fn(h, work[k], N) == 0

        sides = {"world": side_world, "host_parent": side_host_parent,
                 "world_call": lambda: c_call(world._L.fxjps_prepare_slots_world, world._h, warr),
                 "parent": lambda: canvas_call("parent", parent.L.fxjps_prepare_slots, parent.h),
                 "this": lambda: canvas_call("this", this._L.fxjps_prepare_slots, this._h)}
        kept = np.zeros(N, np.int32)
        p_kept = kept.ctypes.data_as(C.POINTER(C.c_int32))

        def refresh_call(fn, h, arr):
            assert fn(h, arr, N, p_kept) == 0 and int(kept.sum()) == N

        # the refreshing sides and the parent's world calls, each on a job array of its own
        extra = {"world_refresh_call": (world_refresh._L, world_refresh._h)}
        if parent.has_world:
            extra["parent_world_refresh_call"] = (parent_world_refresh.L, parent_world_refresh.h)
            extra["parent_world_call"] = (parent_world.L, parent_world.h)
        rarr = {}
        for k, (L, h) in extra.items():
            rarr[k], keep_k = fx.Planner._world_jobs(wjobs)
            wkeep = wkeep + keep_k
            if k == "parent_world_call":
                sides[k] = lambda k=k, L=L, h=h: c_call(L.fxjps_prepare_slots_world, h, rarr[k])
                continue
            assert L.fxjps_refresh_slots_world(h, rarr[k], N, p_kept) == 0, (shape, k)  # (the first call builds what differs)
            assert [tuple(j.goal_xy_cell) + (j.W, j.H, j.end_occu, j.status) for j in rarr[k]] == \
                [tuple(j.goal_xy) + (j.W, j.H, j.end_occu, j.status) for j in first], (shape, k)
            sides[k] = lambda k=k, L=L, h=h: refresh_call(L.fxjps_refresh_slots_world, h, rarr[k])
        t, per = ftb.windows(sides, a.reps)
        if parent.has_world:
            for v in range(N):  # what the parent's world calls left in their slots is what this library's left
                g = world.get_grid_slot(v).tobytes()
                assert g == world_refresh.get_grid_slot(v).tobytes() == parent_world.slot(v).tobytes() == parent_world_refresh.slot(v).tobytes(), (shape, v)
        med = {k: float(np.median(t[k])) for k in sides}
        cells = [o[3][0] * o[3][1] for o in o_this]
        case = {"shape": shape, "prior_shape": list(prior.shape), "prepared_cells_min_max": [min(cells), max(cells)],
                "staged_raw_bytes_world": int(sum(j[1].size for j in wjobs)), "staged_raw_bytes_canvas": int(sum(j[1].size for j in hjobs)),
                "calls_per_window": per}
        for k in sides:
            case[k + "_ms"] = ms(t[k])
            case["spread_" + k + "_ms"] = spread(t[k])
        case["world_over_host_parent"] = round(med["world"] / med["host_parent"], 4)
        case["this_over_parent"] = round(med["this"] / med["parent"], 4)
        case["world_call_over_parent"] = round(med["world_call"] / med["parent"], 4)
        if parent.has_world:
            case["world_call_over_parent_world_call"] = round(med["world_call"] / med["parent_world_call"], 4)
            case["world_refresh_call_over_parent"] = round(med["world_refresh_call"] / med["parent_world_refresh_call"], 4)
        case["bar_world_1_00_met"] = bool(med["world"] <= 1.0 * med["host_parent"])
        case["bar_this_1_05_met"] = bool(med["this"] <= 1.05 * med["parent"])
        out["cases"].append(case)
    for spec in a.fold_trace:
        name, d = spec.split("=", 1)
        out.setdefault("trace_us", {})[name] = fold_trace(d)
    for p in (world, this, parent, world_refresh, parent_world, parent_world_refresh):
        if p is not None:
            p.close()
    line = json.dumps(out)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
