"""CPU suite: fxjps_tick_outputs_slots (what both nodes send out per tick, for every query of a grid-slots batch in one call)
is declared, exported and bound; its kernel exists for gfx950 without a private segment, with the figures recorded in
profiles/tick_outputs_resource_usage.json, and the kernels recorded before it keep theirs; and a numpy restatement of
the lines the call follows -- global_planner_st.py:292-298, 335, 356-361 and global_planner_ccst.py:485, 487-495, 507-521 (the
points that remain), 559-562, 590-598 -- reproduces tests/golden/tick_outputs.json, which was produced by executing those
lines.  The GPU suite compares the device against both.  No GPU needed."""
import ctypes as C
import fnmatch
import inspect
import json
import os
import re
import subprocess

import numpy as np
import pytest

from test_grid_slots_host import HIPCC, _resource_usage

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "fxjps_tick_outputs_slots"
GOLDEN = os.path.join(ROOT, "tests", "golden", "tick_outputs.json")


# ---------------------------------------------------------------- the restatement (shared with the GPU suite)
def f64(hexes):
    """the float64 values behind a list of 16-digit bit patterns"""
    return np.array([int(h, 16) for h in hexes], dtype=np.uint64).view(np.float64)


def u64(a):
    return np.ascontiguousarray(a, dtype=np.float64).reshape(-1).view(np.uint64)


def load_golden():
    with open(GOLDEN) as f:
        doc = json.load(f)
    maps = [np.unpackbits(np.frombuffer(bytes.fromhex(m["occ_bits"]), dtype=np.uint8))[:m["W"] * m["H"]].reshape(m["W"], m["H"]).copy()
            for m in doc["maps"]]
    return maps, doc["cases"]


def restate(variant, path, reso, origin, pos, home, end_occu, wp, goal_after, kept):
    """What the node sends after its waypoint block, from what the block left: wp (2 or 3 components), the goal after the
    block and, for ccst, the cells that remain.  -> (point[3], path3 [n, 3], dir [m, 3], dir_back)"""
    px, py, pz = pos
    xo, yo = home
    wp = np.asarray(wp, dtype=np.float64)
    global_goal = np.asarray(goal_after, dtype=np.float64)
    path = np.asarray(path, dtype=np.int64).reshape(-1, 2)
    shift = np.array([1, 1]) if variant == 0 else np.array([1, 0])

    def world(cells):  # path2 = path + shift; path3 = path2 * map_reso + map_o; a zero z column
        p2 = np.asarray(cells, dtype=np.int64).reshape(-1, 2) + shift
        p3 = p2 * reso + list(origin)
        return np.c_[p3, np.zeros([len(p3), 1])]

    path3 = world(path) if len(path) else np.zeros((0, 3))
    if variant == 0:
        dirp, back = np.zeros((0, 3)), 0
    elif len(path):
        dirp, back = world(kept), 0
    else:
        dirp, back = np.array([[px, py, pz], [wp[0], wp[1], wp[2]]]), 100
    with np.errstate(all="ignore"):
        if variant == 1 and (np.linalg.norm(global_goal[0:2] - np.array([px, py])) < 0.5 or end_occu):
            z = 0
        else:
            z = 1 + min(np.linalg.norm(wp[0:2] - np.array([xo, yo])) / np.linalg.norm(global_goal[0:2] - np.array([xo, yo])), 1) * (global_goal[2] - 1)
    return np.array([wp[0], wp[1], z], dtype=np.float64), path3, dirp, back


def test_declared_exported_and_bound():
    from fuxi_planner_amd import _lib, waypoints
    from fuxi_planner_amd.planner import Planner
    hdr = open(os.path.join(ROOT, "include", "fxjps.h")).read()
    version = int(re.search(r"#define FXJPS_VERSION (\d+)", hdr).group(1))
    assert version >= 750 and _lib.VERSION == version
    assert re.search(r"^ \*\s+750\s+%s" % NAME, hdr, re.M), "no changelog line for version 750"
    exports = open(os.path.join(ROOT, "fuxi-planner_amd", "csrc", "exports.map")).read()
    patterns = re.findall(r"global:\s*([^;]+);", exports)
    decl = re.search(r"\bint %s\s*\(([^)]*)\)" % NAME, hdr)
    assert decl and len(decl.group(1).split(",")) == 32
    assert any(fnmatch.fnmatchcase(NAME, p.strip()) for pat in patterns for p in pat.split())
    assert NAME in _lib.SYMBOLS
    # the older call's declaration is what it was: the new one is a superset of its arguments, in its order
    old = re.search(r"\bint fxjps_waypoint_slots_batch\s*\(([^)]*)\)", hdr).group(1)
    names = lambda s: [re.sub(r".*[ *]", "", a.strip()) for a in s.split(",")]
    assert len(names(old)) == 24 and [a for a in names(decl.group(1)) if a in names(old)] == names(old)
    assert [a for a in names(decl.group(1)) if a not in names(old)] == ["home_xy", "out_point", "out_path_xyz", "path_capacity", "out_dir_xyz",
                                                                         "out_dir_n", "out_dir_back", "dir_capacity"]
    sig = inspect.signature(waypoints.tick_outputs_slots)
    assert list(sig.parameters)[:8] == ["planner", "rule", "map_start", "map_reso", "map_o", "pos", "global_goal", "home"]
    sig = inspect.signature(Planner.fleet_tick)
    assert list(sig.parameters) == ["self", "jobs", "pos", "global_goals", "home", "map_reso", "map_o", "prev_wp", "prev_dim", "publish",
                                    "image_channels"]


def test_library_has_the_symbol_and_the_binding_its_prototype():
    import __graft_entry__
    from fuxi_planner_amd import _lib
    __graft_entry__.build()
    L = C.CDLL(_lib.LIB_PATH)
    assert L.fxjps_version() >= 750
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert re.search(r" T %s$" % NAME, nm, re.M) and re.search(r" T fxjps_waypoint_slots_batch$", nm, re.M)
    assert len(getattr(_lib.load(), NAME).argtypes) == 32


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc")
def test_kernel_is_recorded_and_the_recorded_ones_are_unchanged():
    rows = _resource_usage()
    with open(os.path.join(ROOT, "profiles", "tick_outputs_resource_usage.json")) as f:
        rec = json.load(f)
    hit = {name: v for name, v in rows.items() if re.search(r"\d+k_tick_outputs_slotsE", name)}
    assert len(hit) == 1, sorted(rows)
    v = list(hit.values())[0]
    assert int(v["ScratchSize [bytes/lane]"]) == 0 and int(v["VGPRs Spill"]) == 0 and int(v["SGPRs Spill"]) == 0 and int(v["LDS Size [bytes/block]"]) == 0, v
    assert hit == rec["new"]
    # the waypoint and publish kernels as the parent commit compiled them, with the new kernel in the translation unit
    wp = {name: v for name, v in rows.items() if re.search(r"\d+k_(waypoint_slots|waypoint_st|waypoint_ccst|publish_slots)E", name)}
    assert len(wp) == 4 and wp == rec["parent"], sorted(n for n in wp if wp[n] != rec["parent"].get(n))
    with open(os.path.join(ROOT, "profiles", "prepare_slots_resource_usage.json")) as f:
        older = json.load(f)
    shared = {name: v for name, v in rows.items() if re.search(r"k_build_[123]|k_search", name)}
    assert len(shared) == 15 and shared == older["parent"], sorted(n for n in shared if shared[n] != older["parent"].get(n))


def test_golden_file_covers_what_it_should():
    maps, cases = load_golden()
    assert 4 <= len(maps) <= 8 and all(m.shape[0] <= 48 and m.shape[1] <= 48 for m in maps)
    for variant in (0, 1):
        cs = [c for c in cases if c["variant"] == variant]
        assert 24 <= len(cs) <= 60
        assert {0, 1, 2, 3} <= {len(c["path"]) for c in cs}
        assert {0, 1} == {c["end_occu"] for c in cs} and {0, 1} <= {c["end_occu"] for c in cs if c["path"]}
        assert {0, 1} == {c["end_occu"] for c in cs if not c["path"]}
        assert any(c["home"] == c["goal"][:2] for c in cs)
        assert any(list(f64(c["out"]["wp"])[:2]) == c["home"] for c in cs)
        z = np.array([f64(c["out"]["point"])[2] for c in cs])
        assert np.isnan(z).any() and (z == 1.0).any()
    near = [c for c in cases if c["variant"] == 1 and not c["end_occu"] and np.hypot(c["goal"][0] - c["pos"][0], c["goal"][1] - c["pos"][1]) < 0.5]
    assert near and all(f64(c["out"]["point"])[2] == 0.0 for c in near)
    assert any(c["out"]["dir_back"] == 100 for c in cases)


def test_restatement_reproduces_the_golden_file():
    maps, cases = load_golden()
    for i, c in enumerate(cases):
        o = c["out"]
        point, path3, dirp, back = restate(c["variant"], c["path"], c["reso"], c["origin"], c["pos"], c["home"], c["end_occu"], f64(o["wp"]),
                                           f64(o["goal_out"]), o.get("kept"))
        assert ["%016x" % v for v in u64(point)] == o["point"], (i, point, f64(o["point"]))
        assert ["%016x" % v for v in u64(path3)] == o["path3"], i
        assert ["%016x" % v for v in u64(dirp)] == o["dir"], i
        assert back == o["dir_back"], i


def test_host_rules_select_the_golden_waypoints():
    """fxjps_waypoint_st / fxjps_waypoint_ccst (host code) on the golden inputs: the selection the restatement starts from in
    the GPU suite is the golden one."""
    from fuxi_planner_amd import waypoints
    maps, cases = load_golden()
    for i, c in enumerate(cases):
        if not c["path"]:
            continue
        o = c["out"]
        if c["variant"] == 0:
            wp, gout, ang = waypoints.select_st(c["path"], c["map_start"], c["reso"], c["origin"], c["pos"], c["goal"], c["end_occu"], c["prev_wp"])
            assert ["%016x" % v for v in u64([ang])] == [o["ang_wp"]], i
        else:
            wp, kept, gout = waypoints.select_ccst(c["path"], maps[c["map"]], c["reso"], c["origin"], c["pos"], c["goal"], c["end_occu"], return_goal=True)
            assert kept.tolist() == o["kept"], i
        assert ["%016x" % v for v in u64(wp)] == o["wp"] and ["%016x" % v for v in u64(gout)] == o["goal_out"], i
