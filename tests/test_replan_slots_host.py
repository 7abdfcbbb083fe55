"""CPU suite: fxjps_replan_slots (fxjps_plan_batch_slots_csr that hands back the stored paths of queries whose slot, start and
goal did not change) is declared, exported and bound at version 770, Planner has replan_slots and fleet_tick_refresh its
`reuse` keyword, and the two kernels that assemble the full batch -- the scan through the source table and the gather, one
wavefront per path -- exist for gfx950 without a private segment.  Device pass only, no GPU needed."""
import ctypes as C
import fnmatch
import inspect
import os
import re

import pytest

from test_grid_slots_host import HIPCC, _resource_usage

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "fxjps_replan_slots"
KERNELS = ("k_replan_scan", "k_replan_gather")


def test_declared_exported_and_bound():
    from fuxi_planner_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "fxjps.h")).read()
    version = int(re.search(r"#define FXJPS_VERSION (\d+)", hdr).group(1))
    assert version >= 770 and _lib.VERSION == version
    assert re.search(r"^ \*\s+770\s+fxjps_replan_slots", hdr, re.M), "no changelog line for version 770"
    exports = open(os.path.join(ROOT, "fuxi-planner_amd", "csrc", "exports.map")).read()
    patterns = re.findall(r"global:\s*([^;]+);", exports)
    assert any(fnmatch.fnmatchcase(NAME, p.strip()) for pat in patterns for p in pat.split())
    assert NAME in _lib.SYMBOLS
    proto = re.search(r"\bint fxjps_replan_slots\s*\(([^;]*)\);", hdr).group(1)
    args = [re.sub(r"\s+", " ", a).strip() for a in proto.split(",")]
    assert args == ["fxjps_t* h", "const int32_t* grid_ids", "const int32_t* starts_xy", "const int32_t* goals_xy", "int64_t nq", "int32_t hchoice",
                    "int32_t max_path_len", "int64_t* out_offsets", "int32_t* out_cells_xy", "int64_t cells_capacity", "int32_t* out_len",
                    "double* out_cost", "int32_t* out_reused", "double* out_seconds_total"], args


def test_python_surface():
    from fuxi_planner_amd import Planner
    assert list(inspect.signature(Planner.replan_slots).parameters) == ["self", "grid_ids", "starts", "goals", "hchoice", "max_path_len"]
    assert inspect.signature(Planner.replan_slots).parameters["hchoice"].default == 2
    reuse = inspect.signature(Planner.fleet_tick_refresh).parameters["reuse"]
    assert reuse.default is False
    assert "reuse" not in inspect.signature(Planner.fleet_tick).parameters


def test_library_exports_the_call():
    import __graft_entry__
    from fuxi_planner_amd import _lib
    __graft_entry__.build()
    L = C.CDLL(_lib.LIB_PATH)
    assert L.fxjps_version() >= 770
    assert hasattr(L, NAME)
    # a NULL handle is refused before anything is read (no device is touched)
    L.fxjps_replan_slots.argtypes = [C.c_void_p] * 4 + [C.c_int64, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_int64] + [C.c_void_p] * 4
    assert L.fxjps_replan_slots(None, None, None, None, 0, 2, 16, None, None, 0, None, None, None, None) == _lib.E_ARG


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc")
def test_assembly_kernels_exist_without_scratch():
    rows = _resource_usage()
    for k in KERNELS:
        hit = [v for name, v in rows.items() if re.search(r"\d+%sE" % k, name)]
        assert len(hit) == 1, (k, sorted(rows))
        assert int(hit[0]["ScratchSize [bytes/lane]"]) == 0 and int(hit[0]["VGPRs Spill"]) == 0, (k, hit[0])
        assert int(hit[0].get("SGPRs Spill", 0)) == 0, (k, hit[0])
