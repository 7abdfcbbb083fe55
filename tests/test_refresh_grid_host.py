"""CPU suite: fxjps_refresh_grid / fxjps_refresh_occupancy_msg / fxjps_last_refresh_cells / fxjps_replan_frame_raw
 are declared, exported and bound at version 800; the three diff kernels exist for gfx950 without
a private segment; and the ticks of tests/refresh_grid_cases.py, which the GPU suite replays, are what they claim to be
when oracle/gridprep.py prepares them on the host.  No GPU needed."""
import ctypes as C
import fnmatch
import os
import re

import numpy as np
import pytest

import refresh_grid_cases as rc
from oracle import gridprep
from test_grid_slots_host import HIPCC, _resource_usage

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("fxjps_refresh_grid", "fxjps_refresh_occupancy_msg", "fxjps_last_refresh_cells", "fxjps_replan_frame_raw")
DIFF_KERNELS = ("k_grid_diff_count", "k_grid_diff_scan", "k_grid_diff_write")


def test_declared_exported_and_bound():
    from fuxi_planner_amd import _lib
    from fuxi_planner_amd.planner import Planner
    hdr = open(os.path.join(ROOT, "include", "fxjps.h")).read()
    version = int(re.search(r"#define FXJPS_VERSION (\d+)", hdr).group(1))
    assert version >= 800 and _lib.VERSION == version
    assert re.search(r"^ \*\s+800\s+fxjps_refresh_grid", hdr, re.M), "no changelog line for version 800"
    exports = open(os.path.join(ROOT, "fuxi-planner_amd", "csrc", "exports.map")).read()
    patterns = re.findall(r"global:\s*([^;]+);", exports)
    for name in NEW:
        assert re.search(r"\bint %s\s*\(" % name, hdr), name
        assert any(fnmatch.fnmatchcase(name, p.strip()) for pat in patterns for p in pat.split()), name
        assert name in _lib.SYMBOLS
    for name in ("refresh_grid", "refresh_occupancy_msg", "last_refresh_cells", "replan_frame_raw"):
        assert callable(getattr(Planner, name)), name


def test_library_exports_the_calls():
    import __graft_entry__
    from fuxi_planner_amd import _lib
    __graft_entry__.build()
    L = C.CDLL(_lib.LIB_PATH)
    assert L.fxjps_version() >= 800
    for name in NEW:
        assert hasattr(L, name), name
    # a NULL handle is refused before anything is read (no device is touched)
    n = C.c_int64(-5)
    L.fxjps_last_refresh_cells.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]
    assert L.fxjps_last_refresh_cells(None, None, None, 0, C.byref(n)) == _lib.E_ARG
    L.fxjps_refresh_grid.argtypes = [C.c_void_p] * 2 + [C.c_int32] * 4 + [C.c_void_p] * 8
    assert L.fxjps_refresh_grid(None, None, 1, 1, 0, 0, None, None, None, None, None, None, None, None) == _lib.E_ARG


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc")
def test_diff_kernels_exist_without_scratch():
    rows = _resource_usage()
    for k in DIFF_KERNELS:
        hit = [v for name, v in rows.items() if re.search(r"\d+%sE" % k, name)]
        assert len(hit) == 1, (k, sorted(rows))
        assert int(hit[0]["ScratchSize [bytes/lane]"]) == 0 and int(hit[0]["VGPRs Spill"]) == 0, (k, hit[0])
        assert int(hit[0].get("SGPRs Spill", 0)) == 0, (k, hit[0])
    # (the names must not count as search or build kernels where other host tests count those)
    assert not [k for k in DIFF_KERNELS if "k_search" in k or "k_build_" in k]


@pytest.mark.parametrize("case", rc.CASES, ids=lambda c: "%dx%d-ifa%d-%s" % (c[0], c[1], c[2], ("st", "ccst")[c[3]]))
def test_the_cases_are_what_they_say(case):
    """Every step prepares on the host; a step that names its mode gets it by the rule (no byte differs: 0; at most
    max(4096, W * H / 8) cells differ: 1; else, or other extents: 2); the shapes reach what they were chosen for."""
    W0, H0, ifa, variant = case
    resident, seen, names = None, set(), []
    for st in rc.steps(*case):
        resident = rc.apply_pre(resident, st["pre"])
        grid, s, g, md, eo, cells, vals, n, mode = rc.simulate(resident, st["raw"], st["start"], st["goal"], ifa, variant)
        assert st["mode"] in (None, mode), (st["name"], mode, n)
        flat = cells[:, 0] * grid.shape[1] + cells[:, 1]
        assert (np.diff(flat) > 0).all()  # (np.argwhere: ascending order of the flat index)
        if st["pre"] is not None and st["pre"][0] == "poke":  # a poke on an unchanged raw comes back as exactly its cells
            assert flat.tolist() == sorted(st["pre"][1]), st["name"]
        if st["name"].startswith("the goal moved onto"):
            assert g != tuple(np.add(st["goal"], md) - (1 if variant == 0 else 0)) and (eo == 1 or variant == 1), st["name"]
        if st["name"].startswith("a change that occupies the goal"):
            assert grid[st["goal"][0] + md[0] - (variant == 0), st["goal"][1] + md[1] - (variant == 0)] == 1
        if st["name"].startswith("the padding moved"):
            assert grid.shape == resident.shape and md[0] == 2 * ifa + 1
        seen.add(mode)
        names.append(st["name"])
        resident = grid
    W1, H1 = W0 + 6 * ifa, H0 + 6 * ifa
    assert resident.shape == (W1, H1)
    assert (W1 * H1) % rc.BLOCK != 0  # (a partly filled last block)
    if (W0, H0) == (70, 37) and ifa == 0:
        assert (W1 * H1 + rc.BLOCK - 1) // rc.BLOCK == 11
    if (W0, H0) == (300, 300):
        assert (W1 * H1 + rc.BLOCK - 1) // rc.BLOCK > 300 and "prepared cells 255 and 256" in names
    assert seen == {0, 1, 2}


def test_a_long_list_and_an_overflow_are_among_the_cases():
    """At 300 x 300: a mode-1 list longer than the 4096 entries that come back with the header, and an inverted raw whose
    change count exceeds the capacity (mode 2 behind a diff: changed > 0)."""
    case = (300, 300, 0, 1)
    resident, got = None, {}
    for st in rc.steps(*case):
        resident = rc.apply_pre(resident, st["pre"])
        grid, *_, n, mode = rc.simulate(resident, st["raw"], st["start"], st["goal"], case[2], case[3])
        got[st["name"]] = (n, mode)
        resident = grid
    assert got["every other cell of the first 10000"] == (5000, 1) and 4096 < 5000 <= rc.capacity(300, 300)
    assert got["the raw inverted"][1] == 2 and got["the raw inverted"][0] > rc.capacity(300, 300)


def test_a_freed_cell_beside_an_occupied_one_changes_less_than_its_square():
    """ccst, ifa 1: two occupied raw neighbours dilate to overlapping 3 x 3 squares; freeing one changes only the cells the
    other does not cover -- the list of a refresh is the diff of the PREPARED grids, not the dilation of the raw diff."""
    raw = np.zeros((8, 8), np.uint8)
    raw[3, 3] = raw[4, 3] = 1
    a = gridprep.prepare_full(raw, (1, 1), (6, 6), 1, 1)[0]
    raw[3, 3] = 0
    _, _, _, md, _, cells, vals, n, mode = rc.simulate(a, raw.astype(bool), (1, 1), (6, 6), 1, 1)
    assert md == (2, 2) and mode == 1
    assert cells.tolist() == [[4, 4], [4, 5], [4, 6]] and vals.tolist() == [0, 0, 0] and n < 9


def test_an_st_dilation_of_two_changes_nine_spaced_cells():
    """st, ifa 2: the offsets are {-2, 0, 2}^2 -- one raw cell set changes nine prepared cells two apart."""
    raw = np.zeros((9, 9), np.uint8)
    a = gridprep.prepare_full(raw, (1, 1), (7, 7), 2, 0)[0]
    raw[4, 4] = 1
    _, _, _, md, _, cells, vals, n, mode = rc.simulate(a, raw.astype(bool), (1, 1), (7, 7), 2, 0)
    assert md == (4, 4) and mode == 1 and n == 9
    assert cells.tolist() == [[x, y] for x in (6, 8, 10) for y in (6, 8, 10)] and vals.tolist() == [1] * 9


def test_message_bytes_keep_the_occupancy():
    raw = np.random.default_rng(3).random((6, 4)) < 0.4
    data = rc.to_msg(raw, 1)
    assert set(np.unique(data).tolist()) <= {-1, 0, 50, 100} and len(np.unique(data)) == 4
    assert np.array_equal(data.reshape(4, 6).T > 0, raw)
