#!/usr/bin/env python3
"""Many PREPARED grids into grid slots -> one JSON line, also written to --out.

n in {16, 64, 256} vehicles, each with a grid that is ready for its slot (the 256 x 256 / 20 % `synth` shape, or the
reference's 35 maps, cycled).  Sides, each on a handle of its own:
    parent_loop   n fxjps_set_grid_slot calls of the PARENT commit's library (--parent-lib), loaded beside this tree's as a
                  second library.  Build it from a checkout of the parent commit into a scratch directory:
                      git worktree add /tmp/parent HEAD~1 && make -C /tmp/parent/fuxi-planner_amd libfxjps.so
    loop          n fxjps_set_grid_slot calls of this tree's library
    set           one fxjps_set_grid_slots
    refresh_k     one fxjps_refresh_grid_slots per tick, k of the n grids changed since the tick before (the two grids of
                  such a vehicle alternate tick by tick), k in {0, n / 8, n}
What is timed is the C call (the loop: its n C calls) on job arrays filled beforehand.  Method of tools/fleet_tick_bench.py:
the sides alternate in one process, a repetition is a window of as many ticks as make a side run >= 0.2 s, medians of --reps
windows, per tick.  Before anything is timed all sides run the ticks a, b, a, a and every slot -- its bytes and all six
derived arrays -- is compared byte for byte across them, and the refresh sides' kept flags are checked.
Bars (n = 64, synth): set <= 0.5 x parent_loop; loop <= 1.05 x parent_loop (every case).  The refresh ratios against `set`
are reported without a bar.
Last, one jps1.method_many of 64 reference maps against 64 jps1.method calls on the same matrices in turn (the process-wide
planner; the printed costs go to a buffer): with the matrices of the tick before, and with every matrix changed.
Usage: python tools/set_grid_slots_bench.py --parent-lib /tmp/parent/fuxi-planner_amd/libfxjps.so [--reps 5] [--ns 16 64 256]"""
import argparse
import contextlib
import ctypes as C
import io
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
NMAX = 256


class Side(object):
    """A handle of one library and the calls the tool needs, through prototypes of its own (the parent's library is older
    than the binding and does not load through it)."""

    def __init__(self, lib_path, kind):
        from fuxi_planner_amd import _lib
        self.L = L = C.CDLL(lib_path)
        vp, i32, i64 = C.c_void_p, C.c_int32, C.c_int64
        L.fxjps_create.argtypes = [C.c_int, C.POINTER(C.c_int), C.c_int, C.POINTER(vp)]
        L.fxjps_destroy.restype = None
        L.fxjps_destroy.argtypes = [vp]
        L.fxjps_last_error.restype = C.c_char_p
        L.fxjps_last_error.argtypes = [vp]
        L.fxjps_set_grid_slot.argtypes = [vp, i32, C.POINTER(C.c_uint8), i32, i32]
        L.fxjps_get_grid_slot.argtypes = [vp, i32, vp, C.POINTER(i32), C.POINTER(i32)]
        L.fxjps_debug_read_slot_maps.argtypes = [vp, i32, i32, vp, i64, C.POINTER(i64)]
        self.version = L.fxjps_version()
        self.kind = kind  # "loop" / "set" / "refresh"
        if kind != "loop":
            assert L.fxjps_grid_job_size() == C.sizeof(_lib.GridJob), lib_path
            L.fxjps_set_grid_slots.argtypes = [vp, C.POINTER(_lib.GridJob), i32]
            L.fxjps_refresh_grid_slots.argtypes = [vp, C.POINTER(_lib.GridJob), i32, C.POINTER(i32)]
        self.h = vp()
        ids = (C.c_int * 1)(0)
        rc = L.fxjps_create(_lib.BACKEND_HIP, ids, 1, C.byref(self.h))
        assert rc == 0, (lib_path, rc, L.fxjps_last_error(None))
        self.kept = np.zeros(NMAX, np.int32)
        self.p_kept = self.kept.ctypes.data_as(C.POINTER(C.c_int32))
        self.args = {}

    def call(self, arr, n):
        L, h = self.L, self.h
        if self.kind == "loop":
            set_one = L.fxjps_set_grid_slot
            if id(arr) not in self.args:  # (a job array's arguments, read out of it once: the timed loop is the n C calls)
                self.args[id(arr)] = (arr, [(j.slot, j.occ, j.W, j.H) for j in arr])  # (arr: held, so that its id stays its own)
            rc = 0
            for slot, occ, W, H in self.args[id(arr)][1][:n]:
                rc |= set_one(h, slot, occ, W, H)
        elif self.kind == "set":
            rc = L.fxjps_set_grid_slots(h, arr, n)
        else:
            rc = L.fxjps_refresh_grid_slots(h, arr, n, self.p_kept)
        assert rc == 0, (self.kind, rc, L.fxjps_last_error(h))

    def slot_bytes(self, slot):
        W, H = C.c_int32(), C.c_int32()
        assert self.L.fxjps_get_grid_slot(self.h, slot, None, C.byref(W), C.byref(H)) == 0
        occ = np.empty(W.value * H.value, np.uint8)
        assert self.L.fxjps_get_grid_slot(self.h, slot, occ.ctypes.data_as(C.c_void_p), None, None) == 0
        return [(W.value, H.value), occ.tobytes()]

    def close(self):
        self.L.fxjps_destroy(self.h)


def grids(shape, n, other):
    """-> n grids [x][y] uint8; other: a changed grid of the same extents for every vehicle."""
    import fleet_tick_bench as ftb
    raws = [j[1] for j in ftb.fleet(shape, n)]
    if not other:
        return raws
    if shape == "synth":
        from fuxi_planner_amd import synth
        return [synth.synth_grid(256, 256, 5000 + v, 0.20) for v in range(n)]
    out = []
    for m in raws:
        m = m.copy()
        m[::7, ::5] ^= 1
        out.append(m)
    return out


def job_array(gs):
    from fuxi_planner_amd import _lib
    arr = (_lib.GridJob * NMAX)()
    keep = [np.ascontiguousarray(g, dtype=np.uint8) for g in gs]
    for v, (j, g) in enumerate(zip(arr, keep)):
        j.occ, j.slot, j.W, j.H = g.ctypes.data_as(C.POINTER(C.c_uint8)), v, g.shape[0], g.shape[1]
    return arr, keep


def method_many_case(reps):
    """One jps1.method_many of 64 reference maps against 64 jps1.method calls on the same matrices in turn."""
    import fleet_tick_bench as ftb
    from fuxi_planner_amd import jps1
    jobs = ftb.fleet("png", 64)
    calls_a = [(j[1].astype(np.float64), j[2], j[3]) for j in jobs]
    calls_b = []
    for m, s, g in calls_a:
        m = m.copy()
        m[::7, ::5] = 1 - m[::7, ::5]
        m[s] = m[g] = 0
        calls_b.append((m, s, g))
    state = {"t": 0}
    sink = io.StringIO()

    def many_same():
        jps1.method_many(calls_a, 2)

    def many_changed():
        state["t"] += 1
        jps1.method_many(calls_b if state["t"] & 1 else calls_a, 2)

    def loop():
        for m, s, g in calls_a:
            jps1.method(m, s, g, 2)

    with contextlib.redirect_stdout(sink):
        want = [jps1.method(m, s, g, 2)[0] for m, s, g in calls_a]
        assert [r[0] for r in jps1.method_many(calls_a, 2)] == want
        t, per = ftb.windows({"method_loop": loop, "many_same": many_same, "many_changed": many_changed}, reps)
    med = {k: float(np.median(v)) for k, v in t.items()}
    case = {"n": 64, "shape": "png", "paths_found": sum(1 for w in want if w), "calls_per_window": per}
    for k, v in t.items():
        case[k + "_ms"] = round(med[k] * 1e3, 4)
        case["spread_" + k + "_ms"] = [round(min(v) * 1e3, 4), round(max(v) * 1e3, 4)]
    case["many_same_over_method_loop"] = round(med["many_same"] / med["method_loop"], 4)
    case["many_changed_over_method_loop"] = round(med["many_changed"] / med["method_loop"], 4)
    return case


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", required=True, help="libfxjps.so built from the parent commit")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--ns", type=int, nargs="+", default=[16, 64, 256])
    ap.add_argument("--shapes", nargs="+", default=["synth", "png"])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "set_grid_slots_bench.json"))
    a = ap.parse_args()
    import fuxi_planner_amd as fx
    from fuxi_planner_amd import _lib
    import fleet_tick_bench as ftb

    _lib.load()
    sides = {"parent_loop": Side(a.parent_lib, "loop"), "loop": Side(_lib.LIB_PATH, "loop"), "set": Side(_lib.LIB_PATH, "set"),
             "refresh_0": Side(_lib.LIB_PATH, "refresh"), "refresh_eighth": Side(_lib.LIB_PATH, "refresh"),
             "refresh_all": Side(_lib.LIB_PATH, "refresh")}
    assert sides["parent_loop"].version <= sides["loop"].version, (sides["parent_loop"].version, sides["loop"].version)
    refreshing = [name for name, s in sides.items() if s.kind == "refresh"]
    views = {}
    for name, s in sides.items():  # the binding's readers on each side's handle
        p = fx.Planner.__new__(fx.Planner)
        p._L, p._h, p.devices, p.shape = s.L, None, [0], None
        views[name] = p
    out = {"tool": "set_grid_slots_bench", "reps": a.reps, "window_s": ftb.WINDOW_S, "timed": "the C call(s)",
           "parent_version": sides["parent_loop"].version, "version": sides["loop"].version, "cases": []}
    ms = lambda ts: round(float(np.median(ts)) * 1e3, 4)
    spread = lambda ts: [round(min(ts) * 1e3, 4), round(max(ts) * 1e3, 4)]
    for shape in a.shapes:
        ga, gb = grids(shape, max(a.ns), False), grids(shape, max(a.ns), True)
        arr_a, keep_a = job_array(ga)
        arr_b, keep_b = job_array(gb)
        for n in a.ns:
            # all sides on the same ticks, every slot byte for byte, before anything is timed
            for t, arr in enumerate((arr_a, arr_b, arr_a, arr_a)):
                for s in sides.values():
                    s.call(arr, n)
                for name in refreshing if t > 0 else ():  # (t = 0: the slots hold what the case before left)
                    large = [v for v in range(n) if arr[v].W * arr[v].H > 1 << 18]
                    want = [1 if t == 3 and v not in large else 0 for v in range(n)]
                    assert sides[name].kept[:n].tolist() == want, (shape, n, t, name)
                for v in range(n if t in (1, 3) else 0):
                    ref = None
                    for name, s in sides.items():
                        views[name]._h = s.h
                        got = s.slot_bytes(v) + [m.tobytes() for _, m in sorted(views[name].debug_slot_maps(v).items())]
                        views[name]._h = None
                        if ref is None:
                            ref = got
                            assert got[1] == (keep_b if t == 1 else keep_a)[v].tobytes(), (shape, n, t, v)
                        assert got == ref, (shape, n, t, v, name)
            ks = {"refresh_0": 0, "refresh_eighth": n // 8, "refresh_all": n}
            seq, state, kept_seen = {}, {}, {name: set() for name in refreshing}
            for name, k in ks.items():  # k vehicles, spread evenly over the fleet, change their grid every tick
                odd = (_lib.GridJob * NMAX)()
                C.memmove(odd, arr_a, C.sizeof(odd))
                for i in range(k):
                    odd[i * (n // k)] = arr_b[i * (n // k)]
                seq[name] = (arr_a, odd)
                sides[name].call(arr_a, n)
                state[name] = 1

            def tick(name):
                s = sides[name]
                if s.kind != "refresh":
                    s.call(arr_a, n)
                    return
                s.call(seq[name][state[name] & 1], n)
                state[name] += 1
                kept_seen[name].add(int(s.kept[:n].sum()))

            t, per = ftb.windows({name: (lambda name=name: tick(name)) for name in sides}, a.reps)
            cells = [arr_a[v].W * arr_a[v].H for v in range(n)]
            n_large = sum(c > 1 << 18 for c in cells)
            for name, k in ks.items():
                assert kept_seen[name] <= {n - k, n - max(k, n_large)} and kept_seen[name], (shape, n, name, kept_seen[name])
            med = {name: float(np.median(t[name])) for name in sides}
            case = {"shape": shape, "n": n, "cells_min_max": [min(cells), max(cells)], "k": ks, "calls_per_window": per}
            for name in sides:
                case[name + "_ms"] = ms(t[name])
                case["spread_" + name + "_ms"] = spread(t[name])
            case["set_over_parent_loop"] = round(med["set"] / med["parent_loop"], 4)
            case["loop_over_parent_loop"] = round(med["loop"] / med["parent_loop"], 4)
            for name in refreshing:
                case[name + "_over_set"] = round(med[name] / med["set"], 4)
            case["bar_loop_1_05_met"] = bool(med["loop"] <= 1.05 * med["parent_loop"])
            if shape == "synth" and n == 64:
                case["bar_set_half_met"] = bool(med["set"] <= 0.5 * med["parent_loop"])
            out["cases"].append(case)
    for s in sides.values():
        s.close()
    out["method_many"] = method_many_case(a.reps)
    line = json.dumps(out)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
