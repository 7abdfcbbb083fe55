#!/usr/bin/env python3
"""A one-vehicle node's map call when the mapper changed little or nothing -> one JSON line, also
written to --out, and the table of that section (--design rewrites it between its two marker lines).

Shapes: the reference's 147 x 112 map (st, ifa 1) and a 1024 x 1024 / 20 % synthetic raw (ccst, ifa 1).  Tick kinds: the
same raw again; 16 raw cells changed inside one 64 x 64 window; 10 % of the raw cells changed (the two raws of a kind
alternate tick by tick).  Six sides, each on a handle of its own, the same sequence of ticks on each:
    refresh   fxjps_refresh_grid of this tree's library
    parent_refresh   fxjps_refresh_grid of the PARENT commit's library
    prepare   fxjps_prepare_grid of this tree's library, on two handles (prepare, prepare_b)
    parent    fxjps_prepare_grid of the PARENT commit's library (--parent-lib), loaded beside this tree's as a second
              library, on two handles as well (parent, parent_b): two handles that make the same call of the same library
              show what a handle's place in the process is worth; --order changes the places.  Build it from a checkout of the parent commit into a scratch directory:
                  git worktree add /tmp/parent HEAD~1 && make -C /tmp/parent/fuxi-planner_amd libfxjps.so
What is timed is the C call (it returns with the device idle).  Method of tools/refresh_slots_bench.py: the sides alternate
in one process, a repetition is a window of as many ticks as make a side run >= 0.2 s, medians of --reps windows, per tick.
Before anything is timed the five handles run four ticks of every kind and the resident grid and the derived arrays are
compared byte for byte across them after each (the component forest of `refresh` only where its whole build ran: a cell
update unites labels, tests/test_map_updates_gpu.py), and refresh's mode is checked against the kind.
The bars fixed in advance: prepare <= 1.05 x parent, and refresh <= 1.05 x parent_refresh per tick kind.  refresh / parent
is reported per kind.
--goal-on-obstacle: the goal of every tick is a raw cell that is occupied in every raw, so the prepared goal lies on a
dilated obstacle (its row has free cells: the sides' moved goal is checked) and every call runs the whole goal rule.
Usage: python tools/refresh_grid_bench.py --parent-lib /tmp/parent/fuxi-planner_amd/libfxjps.so [--reps 5]
       python tools/refresh_grid_bench.py --design profiles/refresh_grid_bench.json [more.json]   (no GPU: the tables only)"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
KINDS = ("same", "16_cells", "10_percent")
MARK = ("<!-- refresh_grid_bench: begin -->", "<!-- refresh_grid_bench: end -->")


class Side(object):
    """A handle of one library and the calls the tool needs, through prototypes of its own (the parent's library is older
    than the binding and does not load through it)."""

    def __init__(self, lib_path, refresh):
        from fuxi_planner_amd import _lib
        self.L = L = C.CDLL(lib_path)
        vp, i32, p32 = C.c_void_p, C.c_int32, C.POINTER(C.c_int32)
        L.fxjps_create.argtypes = [C.c_int, C.POINTER(C.c_int), C.c_int, C.POINTER(vp)]
        L.fxjps_destroy.restype = None
        L.fxjps_destroy.argtypes = [vp]
        L.fxjps_last_error.restype = C.c_char_p
        L.fxjps_last_error.argtypes = [vp]
        L.fxjps_prepare_grid.argtypes = [vp, vp, i32, i32, i32, i32, p32, p32, p32, p32, p32, p32]
        L.fxjps_get_grid.argtypes = [vp, vp, p32, p32]
        L.fxjps_debug_read_maps.argtypes = [vp, i32, vp, C.c_int64, C.POINTER(C.c_int64)]
        L.fxjps_debug_read_nbmask.argtypes = [vp, vp]
        self.version = L.fxjps_version()
        self.h = vp()
        rc = L.fxjps_create(_lib.BACKEND_HIP, (C.c_int * 1)(0), 1, C.byref(self.h))
        assert rc == 0, (lib_path, rc, L.fxjps_last_error(None))
        self.refresh = refresh
        if refresh:
            L.fxjps_refresh_grid.argtypes = L.fxjps_prepare_grid.argtypes + [C.POINTER(C.c_int64), p32]
        self.s, self.g, self.md = (i32 * 2)(), (i32 * 2)(), (i32 * 2)()
        self.W, self.H, self.eo, self.mode, self.changed = i32(), i32(), i32(), i32(), C.c_int64()

    def call(self, raw, start, goal, ifa, variant):
        self.s[:], self.g[:] = start, goal
        a = [self.h, raw.ctypes.data_as(C.c_void_p), raw.shape[0], raw.shape[1], ifa, variant, self.s, self.g, C.byref(self.W), C.byref(self.H),
             self.md, C.byref(self.eo)]
        if self.refresh:
            rc = self.L.fxjps_refresh_grid(*(a + [C.byref(self.changed), C.byref(self.mode)]))
        else:
            rc = self.L.fxjps_prepare_grid(*a)
        assert rc == 0, (rc, self.L.fxjps_last_error(self.h))

    def outputs(self):
        return tuple(self.s), tuple(self.g), tuple(self.md), self.W.value, self.H.value, self.eo.value

    def state(self):
        """-> {name: bytes}: the resident grid, the neighbour mask and the six derived arrays, the parts no kernel writes cut off."""
        W, H = self.W.value, self.H.value
        PW, PH = W + 2, H + 2
        NS, LINES = (PH + 63) & ~63, max(PW, PH)
        WORDS = (LINES + 63) // 64
        grid, nbm = np.empty((W, H), np.uint8), np.empty((PW, PH), np.uint8)
        assert self.L.fxjps_get_grid(self.h, grid.ctypes.data_as(C.c_void_p), None, None) == 0
        assert self.L.fxjps_debug_read_nbmask(self.h, nbm.ctypes.data_as(C.c_void_p)) == 0
        out = {"grid": grid.tobytes(), "nbmask": nbm.tobytes()}
        for which, name, dt, shape in ((0, "bm", np.uint64, (4, LINES, WORDS, 2)), (1, "ci", np.uint16, (PW, NS)), (2, "comp", np.int32, (W, H)),
                                       (3, "nb8", np.uint8, (PW, NS)), (4, "dbm", np.uint64, (4, PW + PH - 1, WORDS, 2)), (5, "jd", np.uint16, (PW, NS, 8))):
            m, nb = np.zeros(shape, dt), C.c_int64(0)
            assert self.L.fxjps_debug_read_maps(self.h, which, m.ctypes.data_as(C.c_void_p), m.nbytes, C.byref(nb)) == 0 and nb.value == m.nbytes, name
            if name in ("ci", "nb8", "jd"):
                m = m[:, :PH]  # (columns beyond the padded height are unused)
            if name == "bm":   # (a line per padded y for the +-x scans, per padded x for the +-y scans: the rest is never written)
                m[0:2, PH:] = 0
                m[2:4, PW:] = 0
            out[name] = m.tobytes()
        return out

    def close(self):
        self.L.fxjps_destroy(self.h)


def raws_of(shape, rng, goal_on_obstacle=False):
    """-> (raw A uint8 [W0][H0], start, goal, ifa, variant, {kind: raw B})"""
    from fuxi_planner_amd import synth
    if shape == "png_147x112":
        z = np.load(os.path.join(ROOT, "tests", "golden", "maps_png.npz"))
        raw = np.unpackbits(z["-16.20-11.40_out.png"])[:147 * 112].reshape(147, 112).astype(np.uint8)
        variant = 0
    else:
        raw = synth.synth_grid(1024, 1024, 2, 0.20)
        variant = 1
    s, g = synth.synth_queries(raw, 7, 1)
    start, goal = tuple(int(c) for c in s[0]), tuple(int(c) for c in g[0])
    W0, H0 = raw.shape
    if goal_on_obstacle:  # the occupied raw cell nearest to the drawn goal
        occ = np.argwhere(raw != 0)
        goal = tuple(int(c) for c in occ[np.argmin(np.abs(occ - np.array(goal)).sum(1))])
    other = {"same": raw}
    b = raw.copy()
    x0, y0 = W0 // 2 - min(32, W0 // 2), H0 // 2 - min(32, H0 // 2)
    idx = rng.choice(min(64, W0) * min(64, H0), 16, replace=False)
    b[x0 + idx // min(64, H0), y0 + idx % min(64, H0)] ^= 1
    other["16_cells"] = b
    b = raw.copy()
    idx = rng.choice(W0 * H0, W0 * H0 // 10, replace=False)
    b.flat[idx] ^= 1
    other["10_percent"] = b
    for m in other.values():  # the start stays free in every raw, the goal free (or occupied)
        m[start] = 0
        m[goal] = 1 if goal_on_obstacle else 0
    return np.ascontiguousarray(raw), start, goal, 1, variant, {k: np.ascontiguousarray(v) for k, v in other.items()}


def table(out):
    rows = ["| raw | tick | refresh mode | changed cells | refresh ms | prepare ms (A, B) | parent ms (A, B) | refresh / parent | prepare / parent | prepare B / parent | parent B / parent | refresh / parent refresh |",
            "|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for c in out["cases"]:
        rows.append("| %s | %s | %d | %d | %.4f | %.4f, %.4f | %.4f, %.4f | %.3f | %.3f | %.3f | %.3f | %s |" % (
            c["shape"], c["kind"].replace("_", " "), c["refresh_mode"], c["changed_cells"], c["refresh_ms"], c["prepare_ms"], c["prepare_b_ms"],
            c["parent_ms"], c["parent_b_ms"], c["refresh_over_parent"], c["prepare_over_parent"], c["prepare_b_over_parent"], c["parent_b_over_parent"],
            "%.3f" % c["refresh_over_parent_refresh"] if "refresh_over_parent_refresh" in c else "-"))
    return "\n".join(rows)


def write_design(outs):
    path = os.path.join(ROOT, "DESIGN.md")
    text = open(path).read()
    a, b = text.index(MARK[0]) + len(MARK[0]), text.index(MARK[1])
    body = "\n\n".join("Handles created, and windows run, in the order %s:\n\n%s" % (", ".join("`%s`" % n for n in o["order"]), table(o)) for o in outs)
    with open(path, "w") as f:
        f.write(text[:a] + "\n" + body + "\n" + text[b:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", help="libfxjps.so built from the parent commit")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--shapes", nargs="+", default=["png_147x112", "synth_1024"])
    ap.add_argument("--order", nargs="+", default=["refresh", "prepare", "parent", "prepare_b", "parent_b", "parent_refresh"],
                    help="the six sides in the order their handles are created and their windows run")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "refresh_grid_bench.json"))
    ap.add_argument("--goal-on-obstacle", action="store_true", help="every tick's goal lies on a dilated obstacle whose row has a free cell")
    ap.add_argument("--design", metavar="JSON", nargs="+", help="rewrite the tables of DESIGN.md section 3.16 from these result files and exit")
    a = ap.parse_args()
    if a.design:
        write_design([json.loads(open(f).read()) for f in a.design])
        return
    assert a.parent_lib, "--parent-lib is required"
    from fuxi_planner_amd import _lib
    import fleet_tick_bench as ftb

    _lib.load()
    # handles are created, and the windows of a repetition run, in the order of --order
    make = {"refresh": (_lib.LIB_PATH, True), "prepare": (_lib.LIB_PATH, False), "prepare_b": (_lib.LIB_PATH, False),
            "parent": (a.parent_lib, False), "parent_b": (a.parent_lib, False), "parent_refresh": (a.parent_lib, True)}
    assert sorted(a.order) == sorted(make), a.order
    sides = {name: Side(*make[name]) for name in a.order}
    assert sides["parent"].version <= sides["prepare"].version, (sides["parent"].version, sides["prepare"].version)
    state = lambda name: sides[name].state()

    out = {"tool": "refresh_grid_bench", "reps": a.reps, "window_s": ftb.WINDOW_S, "ifa": 1, "timed": "the C call", "order": a.order,
           "goal_on_obstacle": a.goal_on_obstacle, "parent_version": sides["parent"].version, "version": sides["prepare"].version, "cases": []}
    ms = lambda ts: round(float(np.median(ts)) * 1e3, 4)
    spread = lambda ts: [round(min(ts) * 1e3, 4), round(max(ts) * 1e3, 4)]
    rng = np.random.default_rng(16)
    for shape in a.shapes:
        raw_a, start, goal, ifa, variant, other = raws_of(shape, rng, a.goal_on_obstacle)
        for kind in KINDS:
            raw_b = other[kind]
            # the sides on the same ticks, byte for byte, before anything is timed
            modes = []
            for t, raw in enumerate((raw_a, raw_b, raw_a, raw_a)):
                for s in sides.values():
                    s.call(raw, start, goal, ifa, variant)
                want, ref = sides["parent"].outputs(), state("parent")
                modes.append((sides["refresh"].mode.value, sides["refresh"].changed.value))
                sh = 1 if variant == 0 else 0
                if a.goal_on_obstacle:  # (moved: it was occupied, and its row had a free cell)
                    assert want[1] != (goal[0] + want[2][0] - sh, goal[1] + want[2][1] - sh), (shape, kind, t, want)
                for name in ("prepare", "prepare_b", "parent_b", "refresh", "parent_refresh"):
                    assert sides[name].outputs() == want, (shape, kind, t, name)
                    got = state(name)
                    for k in ref:
                        if k == "comp" and sides[name].refresh and modes[-1][0] != 2:
                            continue
                        assert got[k] == ref[k], (shape, kind, t, name, k)
            assert modes[0][0] == 2 or kind != "same" or modes[0][0] == 0, (shape, kind, modes)
            assert modes[3] == (0, 0) and (kind == "same") == (modes[1] == (0, 0)), (shape, kind, modes)
            tick_no = {name: 0 for name in sides}

            def tick(name):
                sides[name].call(raw_b if tick_no[name] & 1 else raw_a, start, goal, ifa, variant)
                tick_no[name] += 1

            for name in sides:  # every side holds raw A's grid when its windows begin
                sides[name].call(raw_a, start, goal, ifa, variant)
                tick_no[name] = 1
            t, per = ftb.windows({name: (lambda name=name: tick(name)) for name in sides}, a.reps)
            med = {name: float(np.median(t[name])) for name in sides}
            case = {"shape": shape, "kind": kind, "prepared": [sides["parent"].W.value, sides["parent"].H.value], "variant": variant,
                    "refresh_mode": modes[1][0], "changed_cells": modes[1][1], "calls_per_window": per}
            for name in sides:
                case[name + "_ms"] = ms(t[name])
                case["spread_" + name + "_ms"] = spread(t[name])
            case["refresh_over_parent"] = round(med["refresh"] / med["parent"], 4)
            case["prepare_over_parent"] = round(med["prepare"] / med["parent"], 4)
            case["prepare_b_over_parent"] = round(med["prepare_b"] / med["parent"], 4)
            case["parent_b_over_parent"] = round(med["parent_b"] / med["parent"], 4)
            case["refresh_over_parent_refresh"] = round(med["refresh"] / med["parent_refresh"], 4)
            case["bar_prepare_1_05_met"] = bool(med["prepare"] <= 1.05 * med["parent"])
            case["bar_refresh_1_05_met"] = bool(med["refresh"] <= 1.05 * med["parent_refresh"])
            out["cases"].append(case)
    for s in sides.values():
        s.close()
    line = json.dumps(out)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    print(line)
    print(table(out))


if __name__ == "__main__":
    main()
