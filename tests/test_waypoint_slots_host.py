"""CPU suite: fxjps_waypoint_slots_batch (both waypoint rules over a grid-slots batch in one call) is declared, exported and
bound, its kernel exists for gfx950 without a private segment, and the kernels whose resource usage is recorded -- k_build_1
.. 3 and every k_search instantiation -- still compile to those figures (the slot descriptor they embed did not grow).
Device pass only, no GPU needed."""
import ctypes as C
import fnmatch
import inspect
import json
import os
import re

import pytest

from test_grid_slots_host import HIPCC, _resource_usage

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "fxjps_waypoint_slots_batch"
KERNELS = ("k_waypoint_slots", "k_waypoint_ccst", "k_waypoint_st")  # the new one, and the two it shares its rule bodies with


def test_declared_exported_and_bound():
    from fuxi_planner_amd import _lib, waypoints
    hdr = open(os.path.join(ROOT, "include", "fxjps.h")).read()
    version = int(re.search(r"#define FXJPS_VERSION (\d+)", hdr).group(1))
    assert version >= 730 and _lib.VERSION == version
    assert re.search(r"^ \*\s+730\s+%s" % NAME, hdr, re.M), "no changelog line for version 730"
    exports = open(os.path.join(ROOT, "fuxi-planner_amd", "csrc", "exports.map")).read()
    patterns = re.findall(r"global:\s*([^;]+);", exports)
    decl = re.search(r"\bint %s\s*\(([^)]*)\)" % NAME, hdr)
    assert decl, NAME
    assert any(fnmatch.fnmatchcase(NAME, p.strip()) for pat in patterns for p in pat.split())
    assert NAME in _lib.SYMBOLS
    # the header says when the slot's occupancy is read
    assert re.search(r"AS IT IS WHEN THIS CALL RUNS", hdr)
    # the wrapper has the arguments the C call has
    sig = inspect.signature(waypoints.select_slots_batch)
    assert list(sig.parameters) == ["planner", "rule", "map_start", "map_reso", "map_o", "pos", "global_goal", "end_occu", "prev_wp", "prev_dim",
                                    "grid_ids", "paths", "return_kept", "dis_wp_tre", "ang_wp_tre", "nthreads"]
    assert len(decl.group(1).split(",")) == 24


def test_library_has_the_symbol_and_the_binding_its_prototype():
    import __graft_entry__
    from fuxi_planner_amd import _lib
    __graft_entry__.build()
    L = C.CDLL(_lib.LIB_PATH)
    assert L.fxjps_version() >= 730
    assert hasattr(L, NAME)
    assert len(getattr(_lib.load(), NAME).argtypes) == 24


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc")
def test_kernel_exists_without_scratch_and_the_recorded_ones_are_unchanged():
    rows = _resource_usage()
    for k in KERNELS:
        hit = [v for name, v in rows.items() if re.search(r"\d+%sE" % k, name)]
        assert len(hit) == 1, (k, sorted(rows))
        assert int(hit[0]["ScratchSize [bytes/lane]"]) == 0 and int(hit[0]["VGPRs Spill"]) == 0 and int(hit[0]["SGPRs Spill"]) == 0, (k, hit[0])
    with open(os.path.join(ROOT, "profiles", "prepare_slots_resource_usage.json")) as f:
        rec = json.load(f)
    shared = {name: v for name, v in rows.items() if re.search(r"k_build_[123]|k_search", name)}
    assert len([n for n in shared if "k_search" in n]) == 12 and len(shared) == 15, sorted(shared)
    assert shared == rec["parent"], sorted(n for n in shared if shared[n] != rec["parent"].get(n))
