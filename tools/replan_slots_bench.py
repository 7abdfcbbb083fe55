#!/usr/bin/env python3
"""The planning half of a fleet tick when most vehicles did not move -> one JSON line, also written to --out.

n = 64 vehicles, one query each on the slot of its own map; the maps are prepared once and stay.  Per tick k of the vehicles
have moved their start by one cell (the two starts of such a vehicle alternate tick by tick), the others ask what they asked
the tick before; k in {0, 8, 64}.  Three sides, each on a handle of its own, the same sequence of ticks on each:
    replan    fxjps_replan_slots of this tree's library
    plan      fxjps_plan_batch_slots_csr of this tree's library
    parent    fxjps_plan_batch_slots_csr of the PARENT commit's library (--parent-lib), loaded beside this tree's as a second
              library.  Build it from a checkout of the parent commit into a scratch directory:
                  git worktree add /tmp/parent HEAD~1 && make -C /tmp/parent/fuxi-planner_amd libfxjps.so
What is timed is the C call with the cells brought out (out_cells_xy given), on arrays filled beforehand.  Method of
tools/refresh_slots_bench.py: the sides alternate in one process, a repetition is a window of as many ticks as make a side run
>= 0.2 s, medians of --reps windows, per tick.  Before anything is timed the three handles run four ticks of the k = 64
sequence (the last one repeats its queries) and offsets, lengths, costs and cells are compared byte for byte across them, and
replan's reused flags are checked against the sequence.
Bars at k = 64: replan <= 1.10 x parent; plan <= 1.05 x parent (every k).  k = 0: the ratio is reported, with the share of the
parent's call that its search launches took (fxjps_timing_t.search_kernel_ms of the parent's last call of the run); no bar.
Usage: python tools/replan_slots_bench.py --parent-lib /tmp/parent/fuxi-planner_amd/libfxjps.so [--reps 5] [--shapes synth png]"""
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

    def __init__(self, lib_path, replan):
        from fuxi_planner_amd import _lib
        self.L = L = C.CDLL(lib_path)
        vp, i32, i64 = C.c_void_p, C.c_int32, C.c_int64
        L.fxjps_create.argtypes = [C.c_int, C.POINTER(C.c_int), C.c_int, C.POINTER(vp)]
        L.fxjps_destroy.restype = None
        L.fxjps_destroy.argtypes = [vp]
        L.fxjps_last_error.restype = C.c_char_p
        L.fxjps_last_error.argtypes = [vp]
        L.fxjps_prepare_slots.argtypes = [vp, C.POINTER(_lib.SlotJob), i32]
        L.fxjps_last_timing.argtypes = [vp, C.POINTER(_lib.Timing)]
        batch = [vp, vp, vp, vp, i64, i32, i32, vp, vp, i64, vp, vp]
        L.fxjps_plan_batch_slots_csr.argtypes = batch + [vp]
        assert L.fxjps_slot_job_size() == C.sizeof(_lib.SlotJob) and L.fxjps_timing_size() == C.sizeof(_lib.Timing), lib_path
        self.version = L.fxjps_version()
        self.h = vp()
        ids = (C.c_int * 1)(0)
        rc = L.fxjps_create(_lib.BACKEND_HIP, ids, 1, C.byref(self.h))
        assert rc == 0, (lib_path, rc, L.fxjps_last_error(None))
        self.replan = replan
        if replan:
            L.fxjps_replan_slots.argtypes = batch + [vp, vp]
        self.reused = np.zeros(N, np.int32)
        self.off, self.len, self.cost = np.zeros(N + 1, np.int64), np.zeros(N, np.int32), np.zeros(N)
        self.cells = None

    def prepare(self, arr):
        assert self.L.fxjps_prepare_slots(self.h, arr, N) == 0, self.L.fxjps_last_error(self.h)
        return [(tuple(j.start_xy), tuple(j.goal_xy), j.W, j.H, j.status) for j in arr]

    def call(self, ids, starts, goals, mpl):
        if self.cells is None or len(self.cells) < N * mpl:
            self.cells = np.zeros((N * mpl, 2), np.int32)
        p = lambda a: a.ctypes.data_as(C.c_void_p)
        head = (self.h, p(ids), p(starts), p(goals), N, 2, mpl, p(self.off), p(self.cells), N * mpl, p(self.len), p(self.cost))
        if self.replan:
            rc = self.L.fxjps_replan_slots(*(head + (p(self.reused), None)))
        else:
            rc = self.L.fxjps_plan_batch_slots_csr(*(head + (None,)))
        assert rc == 0, (rc, self.L.fxjps_last_error(self.h))

    def outputs(self):
        return [self.off.tobytes(), self.len.tobytes(), self.cost.tobytes(), self.cells[:int(self.off[N])].tobytes()]

    def timing(self):
        from fuxi_planner_amd import _lib
        t = _lib.Timing()
        assert self.L.fxjps_last_timing(self.h, C.byref(t)) == 0
        return t

    def close(self):
        self.L.fxjps_destroy(self.h)


def moved(grid, start):
    """A free cell next to `start` (prepared-grid cells)."""
    for dx, dy in ((1, 0), (0, 1), (-1, 0), (0, -1), (1, 1), (-1, -1), (1, -1), (-1, 1)):
        x, y = start[0] + dx, start[1] + dy
        if 0 <= x < grid.shape[0] and 0 <= y < grid.shape[1] and grid[x, y] == 0:
            return (x, y)
    return start


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", required=True, help="libfxjps.so built from the parent commit")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--shapes", nargs="+", default=["synth", "png"])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "replan_slots_bench.json"))
    a = ap.parse_args()
    import fuxi_planner_amd as fx
    from fuxi_planner_amd import _lib
    from oracle import gridprep
    import fleet_tick_bench as ftb

    _lib.load()
    sides = {"replan": Side(_lib.LIB_PATH, True), "plan": Side(_lib.LIB_PATH, False), "parent": Side(a.parent_lib, False)}
    assert sides["parent"].version < sides["plan"].version, (sides["parent"].version, sides["plan"].version)
    out = {"tool": "replan_slots_bench", "n": N, "reps": a.reps, "window_s": ftb.WINDOW_S, "ifa": 1, "timed": "the C call, cells brought out",
           "parent_version": sides["parent"].version, "version": sides["plan"].version, "cases": []}
    ms = lambda ts: round(float(np.median(ts)) * 1e3, 4)
    spread = lambda ts: [round(min(ts) * 1e3, 4), round(max(ts) * 1e3, 4)]
    for shape in a.shapes:
        jobs = ftb.fleet(shape, N)
        arr, keep = fx.Planner._slot_jobs(jobs)
        outs = None
        for s in sides.values():
            fresh = (_lib.SlotJob * N)()
            C.memmove(fresh, arr, C.sizeof(fresh))
            got = s.prepare(fresh)
            assert outs is None or got == outs, shape
            outs = got
        assert all(o[4] == 0 for o in outs), shape
        ids = np.arange(N, dtype=np.int32)
        starts_a = np.array([o[0] for o in outs], np.int32)
        goals = np.array([o[1] for o in outs], np.int32)
        grids = [gridprep.prepare_full(j[1], j[2], j[3], j[4], j[5])[0] for j in jobs]
        starts_b = np.array([moved(grids[v], tuple(int(c) for c in starts_a[v])) for v in range(N)], np.int32)
        assert (starts_b != starts_a).any(axis=1).all(), shape
        mpl = max(int(min(o[2] * o[3] + 1, max(256, 4 * max(o[2], o[3])))) for o in outs)

        def sequence(k):
            """-> the two start arrays a tick alternates between: k vehicles, spread evenly over the fleet, move every tick."""
            odd = starts_a.copy()
            step = N // k if k else 0
            for i in range(k):
                odd[i * step] = starts_b[i * step]
            return starts_a, odd

        # the three sides on the same ticks, byte for byte, before anything is timed
        even, odd = sequence(N)
        while True:
            for t, st in enumerate((even, odd, even, even)):
                for s in sides.values():
                    s.call(ids, st, goals, mpl)
                want = sides["parent"].outputs()
                for name in ("replan", "plan"):
                    assert sides[name].outputs() == want, (shape, t, name)
                assert sides["replan"].reused.tolist() == [1 if t == 3 else 0] * N, (shape, t, sides["replan"].reused.tolist())
            if (sides["parent"].len == _lib.Q_PATH_TOO_LONG).any():  # (rare: grow the slot as Planner.plan_batch_slots does)
                mpl *= 8
                continue
            break
        reachable = int((sides["parent"].len > 0).sum())
        for k in KS:
            even, odd = sequence(k)
            state = {name: 0 for name in sides}
            reused_seen = []

            def tick(name):
                s = sides[name]
                s.call(ids, odd if state[name] & 1 else even, goals, mpl)
                state[name] += 1
                if name == "replan":
                    reused_seen.append(int(s.reused.sum()))

            for name in sides:  # every side has planned the `even` queries when its windows begin
                sides[name].call(ids, even, goals, mpl)
                state[name] = 1
            t, per = ftb.windows({name: (lambda name=name: tick(name)) for name in sides}, a.reps)
            assert set(reused_seen) == {N - k}, (shape, k, sorted(set(reused_seen)))
            med = {name: float(np.median(t[name])) for name in sides}
            case = {"shape": shape, "k": k, "reused_per_tick": N - k, "max_path_len": mpl, "reachable": reachable, "calls_per_window": per}
            for name in sides:
                case[name + "_ms"] = ms(t[name])
                case["spread_" + name + "_ms"] = spread(t[name])
            case["replan_over_parent"] = round(med["replan"] / med["parent"], 4)
            case["plan_over_parent"] = round(med["plan"] / med["parent"], 4)
            case["bar_plan_1_05_met"] = bool(med["plan"] <= 1.05 * med["parent"])
            if k == 0:
                case["parent_search_share"] = round(sides["parent"].timing().search_kernel_ms / (med["parent"] * 1e3), 4)
                case["replan_search_launches"] = int(sides["replan"].timing().search_launches)
            if k == N:
                case["bar_replan_1_10_met"] = bool(med["replan"] <= 1.10 * med["parent"])
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
