"""CPU suite of the cropped world-frame calls: fxjps_prepare_slots_cropped /
fxjps_refresh_slots_cropped / fxjps_crop_size are declared, exported, bound and in the changelog; the ctypes mirror of
fxjps_crop_t is the header's struct field by field; worldprep.crop_host followed by worldprep.merge_host -- the host form,
and what the GPU suite compares the device with -- reproduces every case of tests/golden/cropprep.json, whose expected
values come from executing the reference's own lines; the two crop kernels compile for gfx950 to the figures recorded in
profiles/crop_kernels_resource_usage.json, without scratch or spills.  No GPU needed."""
import ctypes as C
import fnmatch
import json
import os
import re

import numpy as np
import pytest

from cropprep_cases import bits, cases, check_record, message
from test_grid_slots_host import HIPCC, _resource_usage

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("fxjps_prepare_slots_cropped", "fxjps_refresh_slots_cropped", "fxjps_crop_size")
KERNELS = ("k_crop_bounds", "k_crop_window")
CTYPES = {"int32_t": C.c_int32, "double": C.c_double}
CLASSES = ("planned", "planned_prior", "none", "win_zero", "narrow", "lo_negative", "vehicle_decides")


def test_declared_exported_bound_and_in_the_changelog():
    from fuxi_planner_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "fxjps.h")).read()
    version = int(re.search(r"#define FXJPS_VERSION (\d+)", hdr).group(1))
    assert version >= 790 and _lib.VERSION == version
    assert re.search(r"^ \*\s+790\s+fxjps_prepare_slots_cropped, fxjps_refresh_slots_cropped", hdr, re.M), "no changelog line for version 790"
    assert int(re.search(r"#define FXJPS_JOB_NOT_PLANNED (\d+)", hdr).group(1)) == 1 == _lib.JOB_NOT_PLANNED
    exports = open(os.path.join(ROOT, "fuxi-planner_amd", "csrc", "exports.map")).read()
    patterns = re.findall(r"global:\s*([^;]+);", exports)
    for name in NEW:
        assert re.search(r"\bint %s\s*\(" % name, hdr), name
        assert any(fnmatch.fnmatchcase(name, p.strip()) for pat in patterns for p in pat.split()), name
        assert name in _lib.SYMBOLS
    src = open(os.path.join(ROOT, "fuxi-planner_amd", "csrc", "fxjps_maps.hip.inc")).read()
    for k in KERNELS:
        assert re.search(r"__global__[^\n]*\bvoid %s\(" % k, src), k


def test_ctypes_mirror_matches_the_header_field_by_field():
    from fuxi_planner_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "fxjps.h")).read()
    body = re.search(r"typedef struct fxjps_crop \{(.*?)\} fxjps_crop_t;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    decl = r"(int32_t|double)\s+(\w+)\[(\d+)\];"
    fields = [(nm, CTYPES[ty] * int(k)) for ty, nm, k in re.findall(decl, body)]
    assert len(re.findall(r";", body)) == len(fields) == 6, "a field of another form"
    mirror = list(_lib.Crop._fields_)
    assert [f[0] for f in fields] == [f[0] for f in mirror] == ["bbox", "start0", "lo", "win", "map_o", "map_t"]
    for (name, want), (_, got) in zip(fields, mirror):
        assert want._type_ == got._type_ and want._length_ == got._length_, name
    assert C.sizeof(_lib.Crop) == 10 * 4 + 4 * 8
    # the job struct of the world-frame calls is what it was
    assert C.sizeof(_lib.WorldJob) == C.sizeof(C.c_void_p) + 8 * 4 + 15 * 8 + 12 * 4


def test_library_reports_the_crop_size_the_binding_has():
    import __graft_entry__
    from fuxi_planner_amd import _lib
    __graft_entry__.build()
    L = C.CDLL(_lib.LIB_PATH)
    assert L.fxjps_version() >= 790
    assert L.fxjps_crop_size() == C.sizeof(_lib.Crop)
    assert L.fxjps_world_job_size() == C.sizeof(_lib.WorldJob)
    for name in NEW:
        assert hasattr(L, name), name


def test_fixture_holds_the_cases_it_was_made_for():
    G = cases()
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "cropprep.json")) <= 200 * 1024
    for cls in CLASSES:
        assert sum(1 for c in G if c["cls"] == cls) >= 15, cls
    assert all(1 <= min(c["raw"].shape) and max(c["raw"].shape) <= 20 for c in G)
    assert set(np.unique(np.concatenate([c["raw"].reshape(-1) for c in G]))) == {0, 1, 3, 50}
    assert {c["reso"] for c in G} == {0.05, 0.1, 0.2, 0.25}
    assert any(c["aligned"] for c in G) and any(not c["aligned"] for c in G)
    assert 0.3 <= sum(c["prior"] is not None for c in G) / len(G) <= 0.7
    for c in G:
        if c["cls"] == "lo_negative":
            assert c["status"] == -1 and "bbox" not in c
            continue
        nz = c["raw"].nonzero()
        if c["cls"] == "none":
            assert len(nz[0]) == 0 and c["status"] == 1 and c["lo"] is None
            continue
        # the box, and the two quirks: the low corner is min(first non-zero, vehicle's cell), the last row / column is excluded
        assert c["bbox"] == [nz[0].min(), nz[1].min(), nz[0].max(), nz[1].max()]
        assert c["lo"] == [min(c["bbox"][k], c["start0"][k]) for k in range(2)]
        assert c["win"] == [c["bbox"][2 + k] - c["lo"][k] for k in range(2)]
        if c["cls"] == "win_zero":
            assert c["status"] == 1 and c["win"][0] * c["win"][1] == 0
        elif c["cls"] == "narrow":
            assert c["status"] == 1 and c["raw"].shape[0] <= 2 * c["ifa"] and c["win"][0] * c["win"][1] > 0
        else:
            assert c["status"] == 0 and min(c["lo"]) >= 0 and list(c["window"].shape) == c["win"]
            assert (c["cls"] == "vehicle_decides") == any(c["start0"][k] < c["bbox"][k] for k in range(2))
            assert c["cls"] == "vehicle_decides" or (c["prior"] is not None) == (c["cls"] == "planned_prior")


def test_crop_host_then_merge_host_agrees_with_every_case():
    from fuxi_planner_amd import worldprep
    from fuxi_planner_amd.planner import Planner
    from oracle import gridprep
    done = 0
    for i, c in enumerate(cases()):
        rec, outcome, window = worldprep.crop_host(c["raw"], c["map_o"], c["reso"], c["pos"], c["ifa"])
        assert outcome == c["status"], i
        check_record(rec, c, i)
        # the message form of the same map
        rec1, outcome1, window1 = worldprep.crop_host(message(c), c["map_o"], c["reso"], c["pos"], c["ifa"])
        assert outcome1 == outcome and rec1["bbox"] == rec["bbox"] and rec1["win"] == rec["win"] and bits(rec1["map_t"]) == bits(rec["map_t"]), i
        if outcome != 0:
            assert window is None and window1 is None, i
            continue
        lo, hi = rec["lo"], rec["bbox"][2:]
        assert np.array_equal(window, c["raw"][lo[0]:hi[0], lo[1]:hi[1]]) and np.array_equal(window != 0, c["window"]), i
        assert np.array_equal(window1 > 0, window > 0), i
        canvas, shape, o, s, g = worldprep.merge_host(window, rec["map_o"], c["reso"], c["pos"], c["goal_xy"], prior=c["prior"], ori_pre=c["ori_pre"],
                                                      map_t=rec["map_t"])
        assert list(shape) == c["canvas_shape"] and np.array_equal(canvas, c["canvas"]), i
        assert bits(o) == bits(c["canvas_o"]) and list(s) == c["start"] and list(g) == c["goal"], i
        grid, s1, g1, md, eo = gridprep.prepare_full(canvas, s, g, c["ifa"], 1)
        p = c["prep"]
        assert list(grid.shape) == p["grid_shape"] and np.array_equal(grid, p["grid"]), i
        assert list(s1) == p["start_out"] and list(g1) == p["goal_out"] and list(md) == p["map_d"] and eo == p["end_occu"], i
        assert bits(Planner.shifted_origin(o, md, c["reso"])) == bits(p["origin"]), i
        done += 1
    assert done >= 45


def test_crop_host_counts_what_nonzero_counts_and_refuses_what_the_library_refuses():
    from fuxi_planner_amd import worldprep
    # a message with -1 (unknown), 100, 50 and -5: -1 became 0 and does not count, 50 and -5 do
    data = np.zeros((6, 8), dtype=np.int8)  # [y][x]
    data[0, 0] = -1
    data[2, 3] = 50
    data[4, 6] = -5
    data[3, 4] = 100
    rec, outcome, window = worldprep.crop_host((data.reshape(-1), 8, 6), [0.0, 0.0], 0.5, [2.1, 1.6], 1)
    assert rec["bbox"] == [3, 2, 6, 4] and rec["start0"] == [4, 3] and rec["lo"] == [3, 2] and rec["win"] == [3, 2] and outcome == 0
    assert window.shape == (3, 2) and window[0, 0] == 50 and window[1, 1] == 1
    for bad in (dict(map_reso=0.0), dict(map_reso=float("nan")), dict(map_o=[float("inf"), 0.0]), dict(pos_xy=[0.0, float("nan")]),
                dict(pos_xy=[3e9, 0.0])):
        with pytest.raises(ValueError):
            worldprep.crop_host(**dict(dict(raw=np.ones((3, 3)), map_o=[0.0, 0.0], map_reso=0.5, pos_xy=[0.0, 0.0], ifa=0), **bad))


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc")
def test_crop_kernels_compile_to_their_record_without_scratch_or_spills():
    with open(os.path.join(ROOT, "profiles", "crop_kernels_resource_usage.json")) as f:
        record = json.load(f)
    rows = _resource_usage()
    mine = {name: v for name, v in rows.items() if re.match(r"_ZN2fx\d+k_crop_", name)}
    assert sorted(re.match(r"_ZN2fx\d+(k_crop_[a-z]+)E", n).group(1) for n in mine) == sorted(KERNELS), sorted(mine)
    assert mine == record, (mine, record)
    for name, v in mine.items():
        assert int(v["ScratchSize [bytes/lane]"]) == 0 and int(v["VGPRs Spill"]) == 0 and int(v["SGPRs Spill"]) == 0, (name, v)
        assert v["Dynamic Stack"] == "False", (name, v)
