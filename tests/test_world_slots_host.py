"""CPU suite of the world-frame fleet calls: fxjps_prepare_slots_world / fxjps_refresh_slots_world
and the prior maps are declared, exported, bound and in the changelog; the ctypes mirror of fxjps_world_job_t is the
header's struct field by field; worldprep.merge_host -- the host form, and what the GPU suite compares the device with --
reproduces every case of tests/golden/worldprep.json, whose expected values come from executing the reference's own lines;
the two new gather kernels compile for gfx950 without scratch.  No GPU needed."""
import ctypes as C
import fnmatch
import os
import re

import numpy as np
import pytest

from conftest import load_golden
from test_grid_slots_host import HIPCC, _resource_usage
from worldprep_cases import cases, merge_args, placements, unpack

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("fxjps_set_prior_map", "fxjps_get_prior_map", "fxjps_prepare_slots_world", "fxjps_refresh_slots_world", "fxjps_world_job_size")
KERNELS = ("k_slots_gatherILb1ELb0EE", "k_slots_gatherILb1ELb1EE")  # k_slots_gather<WORLD = true, REFRESH> inside a mangled name
CTYPES = {"const void*": C.c_void_p, "int32_t": C.c_int32, "double": C.c_double}


def test_declared_exported_bound_and_in_the_changelog():
    from fuxi_planner_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "fxjps.h")).read()
    version = int(re.search(r"#define FXJPS_VERSION (\d+)", hdr).group(1))
    assert version >= 780 and _lib.VERSION == version
    assert re.search(r"^ \*\s+780\s+fxjps_prepare_slots_world", hdr, re.M), "no changelog line for version 780"
    assert int(re.search(r"#define FXJPS_MAX_PRIOR_MAPS (\d+)", hdr).group(1)) == 16 == _lib.MAX_PRIOR_MAPS
    exports = open(os.path.join(ROOT, "fuxi-planner_amd", "csrc", "exports.map")).read()
    patterns = re.findall(r"global:\s*([^;]+);", exports)
    for name in NEW:
        assert re.search(r"\bint %s\s*\(" % name, hdr), name
        assert any(fnmatch.fnmatchcase(name, p.strip()) for pat in patterns for p in pat.split()), name
        assert name in _lib.SYMBOLS
    src = open(os.path.join(ROOT, "fuxi-planner_amd", "csrc", "fxjps_maps.hip.inc")).read()
    for k in KERNELS:
        assert "k_search" not in k and re.search(r"__global__[^\n]*\bvoid %s\(" % k.split("I")[0], src), k


def test_ctypes_mirror_matches_the_header_field_by_field():
    from fuxi_planner_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "fxjps.h")).read()
    body = re.search(r"typedef struct fxjps_world_job \{(.*?)\} fxjps_world_job_t;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    decl = r"(const void\*|int32_t|double)\s+([^;]+);"
    for ty, names in re.findall(decl, body):
        for nm in names.split(","):
            m = re.match(r"\s*(\w+)(?:\[(\d+)\])?\s*$", nm)
            assert m, nm
            fields.append((m.group(1), CTYPES[ty] * int(m.group(2)) if m.group(2) else CTYPES[ty]))
    assert len(re.findall(r";", body)) == len(re.findall(decl, body)), "a field of another type"
    mirror = list(_lib.WorldJob._fields_)
    assert [f[0] for f in fields] == [f[0] for f in mirror]
    for (name, want), (_, got) in zip(fields, mirror):
        assert C.sizeof(want) == C.sizeof(got) and getattr(want, "_type_", want) == getattr(got, "_type_", got), name
        assert getattr(want, "_length_", 0) == getattr(got, "_length_", 0), name
    for name in ("raw", "slot", "layout", "W0", "H0", "ifa", "variant", "map_o", "map_t", "map_reso", "pos_xy", "goal_xy", "prior", "ori_pre",
                 "start_xy", "goal_xy_cell", "W", "H", "map_d", "end_occu", "status", "canvas_W", "canvas_H", "canvas_o", "origin"):
        assert name in [f[0] for f in mirror], name
    # the existing job struct is what it was
    assert C.sizeof(_lib.SlotJob) == C.sizeof(C.c_void_p) + 16 * 4


def test_library_reports_the_world_job_size_the_binding_has():
    import __graft_entry__
    from fuxi_planner_amd import _lib
    __graft_entry__.build()
    L = C.CDLL(_lib.LIB_PATH)
    assert L.fxjps_version() >= 780
    assert L.fxjps_world_job_size() == C.sizeof(_lib.WorldJob)
    for name in NEW:
        assert hasattr(L, name), name


def test_fixture_holds_the_cases_it_was_made_for():
    G = cases()
    assert len(G) <= 140 and os.path.getsize(os.path.join(ROOT, "tests", "golden", "worldprep.json")) <= 200 * 1024
    for v in (0, 1):
        sub = [c for c in G if c["variant"] == v]
        assert 50 <= len(sub) <= 70
        assert {c["ifa"] for c in sub} == {0, 1, 2}
        assert {c["arrange"] for c in sub} == {"inside", "left", "below", "right", "above", "disjoint", "none"}
        assert {c["reso"] for c in sub} == {0.05, 0.1, 0.2, 0.25}
        assert any(c["aligned"] for c in sub) and any(not c["aligned"] for c in sub)
    assert sum(c["raises"] for c in G) >= 10
    assert sum(1 for c in G if c["prior"] is not None and c["aligned"] and any(int(q) != int(round(q)) for q in placements(c))) >= 10
    assert any(not set(np.unique(c["raw"])) <= {0, 1} for c in G)
    assert sum(1 for c in G if not c["raises"] and (min(c["start"]) < 0 or min(c["goal"]) < 0)) >= 10
    over = 0
    for c in G:
        if c["raises"] or c["prior"] is None:
            continue
        at = [int(q) for q in placements(c)]
        (rw, rh), (pw, ph), (cw, ch) = c["raw"].shape, c["prior"].shape, c["canvas"].shape
        # no case in which the reference went on with a rectangle sticking out: the library deviates there
        assert at[0] + rw <= cw and at[1] + rh <= ch and at[2] + pw <= cw and at[3] + ph <= ch, c
        only_prior = np.zeros((cw, ch), dtype=np.uint8)
        only_prior[at[2]:at[2] + pw, at[3]:at[3] + ph] = c["prior"]
        under = only_prior[at[0]:at[0] + rw, at[1]:at[1] + rh]
        hit = (under > 0) & (c["raw"] <= 0)
        if hit.any():
            over += 1
            assert not c["canvas"][at[0]:at[0] + rw, at[1]:at[1] + rh][hit].any()  # it overwrites: not a union
    assert over >= 10


def test_merge_host_agrees_with_every_case():
    from fuxi_planner_amd import worldprep
    for i, c in enumerate(cases()):
        if c["raises"]:
            with pytest.raises(ValueError):
                worldprep.merge_host(**merge_args(c))
            continue
        canvas, shape, o, s, g = worldprep.merge_host(**merge_args(c))
        assert canvas.dtype == np.uint8 and list(shape) == c["canvas_shape"] == list(canvas.shape), i
        assert np.array_equal(canvas, c["canvas"]), i
        assert np.array(o, dtype=np.float64).tobytes() == np.array(c["canvas_o"], dtype=np.float64).tobytes(), i
        assert list(s) == c["start"] and list(g) == c["goal"], i
        # map_t left out is map_callback's own expression: the same canvas
        if c["prior"] is not None:
            a = dict(merge_args(c), map_t=None)
            again = worldprep.merge_host(**a)
            assert np.array_equal(again[0], canvas) and again[1:] == (shape, o, s, g), i
        # the message form of the same detected map
        m = c["raw"]
        msg = np.where(m == 1, 100, m).astype(np.int8).T.reshape(-1)
        viamsg = worldprep.merge_host(**dict(merge_args(c), raw=(msg, m.shape[0], m.shape[1])))
        assert np.array_equal(viamsg[0], canvas) and viamsg[1:] == (shape, o, s, g), i


def test_merge_host_then_the_preparation_reproduces_the_fixture():
    from fuxi_planner_amd import worldprep
    from fuxi_planner_amd.planner import Planner
    from oracle import gridprep
    done = 0
    for i, c in enumerate(cases()):
        if c["raises"] or c.get("prep") is None or not isinstance(c["prep"], dict):
            continue
        canvas, _, o, s, g = worldprep.merge_host(**merge_args(c))
        grid, s1, g1, md, eo = gridprep.prepare_full(canvas, s, g, c["ifa"], c["variant"])
        p = c["prep"]
        assert list(grid.shape) == p["grid_shape"] and np.array_equal(grid, p["grid"]), i
        assert list(s1) == p["start_out"] and list(g1) == p["goal_out"] and list(md) == p["map_d"] and eo == p["end_occu"], i
        origin = Planner.shifted_origin(o, md, c["reso"])
        assert np.array(origin, dtype=np.float64).tobytes() == np.array(p["origin"], dtype=np.float64).tobytes(), i
        done += 1
    assert done >= 60


def test_merge_host_refuses_what_the_library_refuses():
    from fuxi_planner_amd import worldprep
    raw, pre = np.zeros((4, 5), dtype=np.uint8), np.ones((6, 6), dtype=np.uint8)
    ok = dict(raw=raw, map_o=[-1.0, -1.0], map_reso=0.5, pos_xy=[0.0, 0.0], goal_xy=[1.0, 1.0], prior=pre, ori_pre=[-2.0, -2.0])
    worldprep.merge_host(**ok)
    for bad in (dict(map_reso=0.0), dict(map_reso=-0.5), dict(map_reso=float("nan")), dict(map_reso=float("inf")), dict(map_o=[float("nan"), 0.0]),
                dict(pos_xy=[0.0, float("inf")]), dict(goal_xy=[float("-inf"), 0.0]), dict(ori_pre=[float("nan"), 0.0]),
                dict(map_t=[float("inf"), 1.0]), dict(goal_xy=[3e9, 0.0]), dict(pos_xy=[0.0, -3e9]), dict(map_o=[4e9, 0.0]),
                dict(map_t=[0.0, 0.0], ori_pre=[-1.0, -1.0], prior=np.ones((1, 1), dtype=np.uint8))):  # a clipped detected map
        with pytest.raises(ValueError):
            worldprep.merge_host(**dict(ok, **bad))
    # the stated deviation: two rectangles one cell wide on a canvas of 0 cells (0.99999999999999645 truncated).  numpy
    # broadcasts a side of 1 into a side of 0 and the reference would go on; the library and merge_host refuse
    one = np.ones((1, 3), dtype=np.uint8)
    still = np.zeros((0, 3))
    still[0:1, 0:3] = one
    with pytest.raises(ValueError):
        worldprep.merge_host(one, (-32.0, 0.0), 0.2, (-31.9, 0.1), (-31.9, 0.3), prior=one, ori_pre=(-32.0, 0.0))


def test_prior_image_numpy_agrees_with_the_loader_cases():
    from fuxi_planner_amd import worldprep
    G = load_golden("adapters.json")["loader"]
    assert len(G) >= 15
    for r in G:
        gray = np.frombuffer(bytes.fromhex(r["gray_hex"]), dtype=np.uint8).reshape(r["rows"], r["cols"])
        m = worldprep.prior_from_image(gray)
        assert m.dtype == np.uint8 and m.flags["C_CONTIGUOUS"] and list(m.shape) == r["map_shape"]
        assert np.array_equal(m, unpack(r["map_bits"], r["map_shape"]))


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc")
def test_new_kernels_compile_without_scratch_or_spills():
    rows = _resource_usage()
    for k in KERNELS:
        hit = [v for name, v in rows.items() if re.search(r"\d+%sEv" % k, name)]
        assert len(hit) == 1, (k, sorted(rows))
        assert int(hit[0]["ScratchSize [bytes/lane]"]) == 0 and int(hit[0]["VGPRs Spill"]) == 0, (k, hit[0])
    assert len([n for n in rows if "k_search" in n]) == 12
