#!/usr/bin/env python3
"""Plans a few queries of a benchmark workload with the HOST search (csrc/fxjps_host_search.cpp) on one core, on the maps
the device built: what one host thread of the host tail needs for a query, to set beside the lone
wavefront's time from tools/one_query.py.  The search and the test suite's thin C entry are compiled with g++ into a
temporary library; results are checked against the device's.

    python tools/host_query.py [workload=c2] [query ids, comma separated = 9206,5866,1020,606] [repeats = 3]"""
import ctypes as C, json, os, subprocess, sys, tempfile, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import fuxi_planner_amd as fx
from fuxi_planner_amd import synth
wname = sys.argv[1] if len(sys.argv) > 1 else "c2"
ids = [int(x) for x in (sys.argv[2] if len(sys.argv) > 2 else "9206,5866,1020,606").split(",")]
rep = int(sys.argv[3]) if len(sys.argv) > 3 else 3
wl = json.load(open(os.path.join(ROOT, "fuxi-planner_amd", "workloads.json")))[wname]
so = os.path.join(tempfile.mkdtemp(), "libhost_search.so")
subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-pthread", "-fPIC", "-shared", "-o", so,
                       os.path.join(ROOT, "fuxi-planner_amd", "csrc", "fxjps_host_search.cpp"), os.path.join(ROOT, "tests", "host_search_entry.cpp")])
L = C.CDLL(so)
L.fxh_plan_batch.restype = C.c_int
L.fxh_plan_batch.argtypes = [C.c_void_p] * 3 + [C.c_int32] * 5 + [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_uint64, C.c_int32] + [C.c_void_p] * 5
p = fx.Planner([0])
occ = synth.synth_grid(wl["W"], wl["H"], wl["grid_seed"], wl["p"])
p.set_grid_occ(occ)
s, g = synth.synth_queries(occ, wl["qseed"], wl["nq"])
s, g = np.ascontiguousarray(s, np.int32), np.ascontiguousarray(g, np.int32)
m = p.debug_maps()
W, H = occ.shape
NS = (H + 2 + 63) & ~63
jd = np.zeros((W + 2, NS, 8), np.uint16)
jd[:, :H + 2] = m["jd"]
bm, comp = np.ascontiguousarray(m["bm"]), np.ascontiguousarray(m["comp"], np.int32)
ml = wl["max_path_len"]
for q in ids:
    off, cells, cost, st = p.plan_batch(s[q:q + 1], g[q:q + 1], wl["hchoice"], ml)
    tm = p.timing()
    oc, ol, ocost = np.zeros((1, ml, 2), np.int32), np.zeros(1, np.int32), np.zeros(1, np.float64)
    pops, pushes = np.zeros(1, np.int64), np.zeros(1, np.int64)
    best = 1e9
    for r in range(rep):
        t0 = time.perf_counter()
        rc = L.fxh_plan_batch(jd.ctypes.data, bm.ctypes.data, comp.ctypes.data, W, H, NS, bm.shape[1], bm.shape[2], s[q:q + 1].ctypes.data,
                              g[q:q + 1].ctypes.data, 1, wl["hchoice"], ml, 64 * W * H + 4096, 1, oc.ctypes.data, ol.ctypes.data, ocost.ctypes.data,
                              pops.ctypes.data, pushes.ctypes.data)
        best = min(best, time.perf_counter() - t0)
        assert rc == 0
    same = ol[0] == st[0] and ocost.tobytes() == cost.tobytes() and np.array_equal(oc[0, :max(ol[0], 0)], cells) and \
        (pops[0], pushes[0]) == (tm["pops"], tm["pushes"])
    print("%s query %d: host %.2f ms (%.3f us per pop), lone wavefront %.2f ms (%.3f us per pop), pops %d, pushes %d, path %d cells, results %s" % (
        wname, q, best * 1e3, best * 1e6 / max(pops[0], 1), tm["search_kernel_ms"], 1e3 * tm["search_kernel_ms"] / max(tm["pops"], 1), pops[0],
        pushes[0], ol[0], "equal" if same else "DIFFER"))
    assert same
