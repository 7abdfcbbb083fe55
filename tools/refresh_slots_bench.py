#!/usr/bin/env python3
"""The map half of a fleet tick when most maps did not change -> one JSON line, also written to --out.

n = 64 vehicles; per tick k of them hand in a NEW raw map (the two raws of such a vehicle alternate tick by tick, same shape,
another seed / the same map with a lattice of cells flipped), the others the raw of the tick before; k in {0, 8, 64}.  Three sides, each
on a handle of its own, the same sequence of ticks on each:
    refresh   fxjps_refresh_slots of this tree's library
    prepare   fxjps_prepare_slots of this tree's library
    parent    fxjps_prepare_slots of the PARENT commit's library (--parent-lib), loaded beside this tree's as a second
              library.  Build it from a checkout of the parent commit into a scratch directory:
                  git worktree add /tmp/parent HEAD~1 && make -C /tmp/parent/fuxi-planner_amd libfxjps.so
    parent_refresh   fxjps_refresh_slots of the parent's library, where it has the call (a change that leaves the call as
              it is -- a refactor -- is measured against this side)
What is timed is the C call on a job array filled beforehand (the inputs are restored by one memmove per call: the call
writes its outputs into the same fields), so the three sides differ in nothing but the library's work.  Method of
tools/fleet_tick_bench.py: the sides alternate in one process, a repetition is a window of as many ticks as make a side run
>= 0.2 s, medians of --reps windows, per tick.  Before anything is timed the three handles run four ticks of the k = 64
sequence (the last one repeats its raws) and every slot -- its bytes and all six derived arrays -- is compared byte for byte across them, and refresh's
kept flags are checked against k.
Bars at k = 0: refresh <= 0.5 x parent; at k = 64: refresh <= 1.10 x parent; prepare <= 1.05 x parent (every k).
Usage: python tools/refresh_slots_bench.py --parent-lib /tmp/parent/fuxi-planner_amd/libfxjps.so [--reps 5] [--shapes synth png]"""
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
KS = (0, 8, 64)


class Side(object):
    """A handle of one library and the calls the tool needs, through prototypes of its own (the parent's library is older
    than the binding and does not load through it)."""

    def __init__(self, lib_path, refresh):
        from fuxi_planner_amd import _lib
        self.L = L = C.CDLL(lib_path)
        vp, i32, i64 = C.c_void_p, C.c_int32, C.c_int64
        L.fxjps_create.argtypes = [C.c_int, C.POINTER(C.c_int), C.c_int, C.POINTER(vp)]
        L.fxjps_destroy.restype = None
        L.fxjps_destroy.argtypes = [vp]
        L.fxjps_last_error.restype = C.c_char_p
        L.fxjps_last_error.argtypes = [vp]
        L.fxjps_prepare_slots.argtypes = [vp, C.POINTER(_lib.SlotJob), i32]
        L.fxjps_get_grid_slot.argtypes = [vp, i32, vp, C.POINTER(i32), C.POINTER(i32)]
        L.fxjps_debug_read_slot_maps.argtypes = [vp, i32, i32, vp, i64, C.POINTER(i64)]
        assert L.fxjps_slot_job_size() == C.sizeof(_lib.SlotJob), lib_path
        self.version = L.fxjps_version()
        self.h = vp()
        ids = (C.c_int * 1)(0)
        rc = L.fxjps_create(_lib.BACKEND_HIP, ids, 1, C.byref(self.h))
        assert rc == 0, (lib_path, rc, L.fxjps_last_error(None))
        self.refresh = refresh
        if refresh:
            L.fxjps_refresh_slots.argtypes = [vp, C.POINTER(_lib.SlotJob), i32, C.POINTER(i32)]
        self.kept = np.zeros(N, np.int32)
        self.arr = (_lib.SlotJob * N)()

    def call(self, pristine):
        C.memmove(self.arr, pristine, C.sizeof(self.arr))
        if self.refresh:
            rc = self.L.fxjps_refresh_slots(self.h, self.arr, N, self.kept.ctypes.data_as(C.POINTER(C.c_int32)))
        else:
            rc = self.L.fxjps_prepare_slots(self.h, self.arr, N)
        assert rc == 0, (rc, self.L.fxjps_last_error(self.h))

    def outputs(self):
        return [(tuple(j.start_xy), tuple(j.goal_xy), j.W, j.H, tuple(j.map_d), j.end_occu, j.status) for j in self.arr]

    def slot_bytes(self, slot):
        W, H = C.c_int32(), C.c_int32()
        assert self.L.fxjps_get_grid_slot(self.h, slot, None, C.byref(W), C.byref(H)) == 0
        occ = np.empty(W.value * H.value, np.uint8)
        assert self.L.fxjps_get_grid_slot(self.h, slot, occ.ctypes.data_as(C.c_void_p), None, None) == 0
        return [(W.value, H.value), occ.tobytes()]

    def close(self):
        self.L.fxjps_destroy(self.h)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", required=True, help="libfxjps.so built from the parent commit")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--shapes", nargs="+", default=["synth", "png"])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "refresh_slots_bench.json"))
    a = ap.parse_args()
    import fuxi_planner_amd as fx
    from fuxi_planner_amd import _lib
    import fleet_tick_bench as ftb

    _lib.load()
    sides = {"refresh": Side(_lib.LIB_PATH, True), "prepare": Side(_lib.LIB_PATH, False), "parent": Side(a.parent_lib, False)}
    assert sides["parent"].version <= sides["prepare"].version, (sides["parent"].version, sides["prepare"].version)
    if hasattr(sides["parent"].L, "fxjps_refresh_slots"):
        sides["parent_refresh"] = Side(a.parent_lib, True)
    refreshing = [name for name, s in sides.items() if s.refresh]
    # the binding's readers on each side's handle: the derived maps as arrays with the unwritten parts cut off
    views = {}
    for name, s in sides.items():
        p = fx.Planner.__new__(fx.Planner)
        p._L, p._h, p.devices, p.shape = s.L, None, [0], None
        views[name] = p
    out = {"tool": "refresh_slots_bench", "n": N, "reps": a.reps, "window_s": ftb.WINDOW_S, "ifa": 1, "timed": "the C call",
           "parent_version": sides["parent"].version, "version": sides["prepare"].version, "cases": []}
    ms = lambda ts: round(float(np.median(ts)) * 1e3, 4)
    spread = lambda ts: [round(min(ts) * 1e3, 4), round(max(ts) * 1e3, 4)]
    for shape in a.shapes:
        jobs_a = ftb.fleet(shape, N)
        # the other raw of every vehicle: same shape, same start and goal
        if shape == "synth":
            from fuxi_planner_amd import synth
            other = [synth.synth_grid(256, 256, 5000 + v, 0.20) for v in range(N)]
        else:
            other = []
            for v, j in enumerate(jobs_a):
                m = j[1].copy()
                m[::7, ::5] ^= 1  # (a changed map of the same extents)
                other.append(m)
        for v, j in enumerate(jobs_a):  # start and goal stay free in both raws
            for c in (j[2], j[3]):
                other[v][c] = 0
        jobs_b = [(j[0], other[v]) + tuple(j[2:]) for v, j in enumerate(jobs_a)]
        arr_a, keep_a = fx.Planner._slot_jobs(jobs_a)
        arr_b, keep_b = fx.Planner._slot_jobs(jobs_b)

        def sequence(k):
            """-> the two job arrays a tick alternates between: k vehicles, spread evenly over the fleet, change their raw every tick."""
            even, odd = (_lib.SlotJob * N)(), (_lib.SlotJob * N)()
            C.memmove(even, arr_a, C.sizeof(even))
            C.memmove(odd, arr_a, C.sizeof(odd))
            step = N // k if k else 0
            for i in range(k):
                odd[i * step] = arr_b[i * step]
            return even, odd

        # the three sides on the same ticks, every slot byte for byte, before anything is timed
        even, odd = sequence(N)
        for t, pristine in enumerate((even, odd, even, even)):
            for s in sides.values():
                s.call(pristine)
            want = sides["parent"].outputs()
            assert all(w[6] == 0 for w in want), (shape, t)
            for name in sides:
                assert sides[name].outputs() == want, (shape, t, name)
            for name in refreshing:
                assert sides[name].kept.tolist() == [1 if t == 3 else 0] * N, (shape, t, name, sides[name].kept.tolist())
            for v in range(N if t in (1, 3) else 0):  # (after a tick that built every slot, and after one that kept every slot)
                ref = None
                for name, s in sides.items():
                    views[name]._h = s.h
                    got = [s.slot_bytes(v)] + [m for _, m in sorted(views[name].debug_slot_maps(v).items())]
                    views[name]._h = None
                    got = [got[0][0], got[0][1]] + [m.tobytes() for m in got[1:]]
                    if ref is None:
                        ref = got
                    assert got == ref, (shape, t, v, name)
        cells = [j.W * j.H for j in sides["parent"].arr]
        for k in KS:
            even, odd = sequence(k)
            state = {name: 0 for name in sides}
            kept_seen = []

            def tick(name):
                s = sides[name]
                s.call(odd if state[name] & 1 else even)
                state[name] += 1
                if s.refresh:
                    kept_seen.append(int(s.kept.sum()))

            for name in sides:  # every side's slots hold the `even` maps when its windows begin
                sides[name].call(even)
                state[name] = 1
            t, per = ftb.windows({name: (lambda name=name: tick(name)) for name in sides}, a.reps)
            assert set(kept_seen) == {N - k}, (shape, k, sorted(set(kept_seen)))
            med = {name: float(np.median(t[name])) for name in sides}
            case = {"shape": shape, "k": k, "kept_per_tick": N - k, "prepared_cells_min_max": [min(cells), max(cells)], "calls_per_window": per}
            for name in sides:
                case[name + "_ms"] = ms(t[name])
                case["spread_" + name + "_ms"] = spread(t[name])
            case["refresh_over_parent"] = round(med["refresh"] / med["parent"], 4)
            case["prepare_over_parent"] = round(med["prepare"] / med["parent"], 4)
            if "parent_refresh" in med:
                case["refresh_over_parent_refresh"] = round(med["refresh"] / med["parent_refresh"], 4)
            case["bar_prepare_1_05_met"] = bool(med["prepare"] <= 1.05 * med["parent"])
            if k == 0:
                case["bar_refresh_half_met"] = bool(med["refresh"] <= 0.5 * med["parent"])
            if k == N:
                case["bar_refresh_1_10_met"] = bool(med["refresh"] <= 1.10 * med["parent"])
            out["cases"].append(case)
    for s in sides.values():
        s.close()
    line = json.dumps(out)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
