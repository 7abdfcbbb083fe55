"""CPU suite: fxjps_refresh_slots (fxjps_prepare_slots that keeps the maps of a slot whose prepared grid did not change) is
declared, exported and bound at version 760, takes the job struct of fxjps_prepare_slots as it was, and its kernels -- the
gather with a compare, the goal launch that hands the answers back, the four gated build launches and the gated
jump-distance launch -- exist for gfx950 without a private segment.  So do the six kernels of fxjps_prepare_slots, whose
bodies they share.  Device pass only, no GPU needed."""
import ctypes as C
import fnmatch
import os
import re

import pytest

from test_grid_slots_host import HIPCC, _resource_usage

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("fxjps_refresh_slots", "fxjps_debug_read_slot_context")
# (template instantiations, as they are spelled inside a mangled name: gather <WORLD, REFRESH>, goal <REFRESH>, stage <L, REFRESH>)
REFRESH_KERNELS = ("k_slots_gatherILb0ELb1EE", "k_slots_goalILb1EE", "k_slots_stageILi1ELb1EE", "k_slots_stageILi2ELb1EE", "k_slots_stageILi3ELb1EE",
                   "k_slots_stageILi4ELb1EE")
# (changed: their bodies moved into functions the refresh kernels call too)
PREPARE_KERNELS = ("k_slots_gatherILb0ELb0EE", "k_slots_goalILb0EE", "k_slots_stageILi1ELb0EE", "k_slots_stageILi2ELb0EE", "k_slots_stageILi3ELb0EE",
                   "k_slots_stageILi4ELb0EE")


def test_declared_exported_and_bound():
    from fuxi_planner_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "fxjps.h")).read()
    version = int(re.search(r"#define FXJPS_VERSION (\d+)", hdr).group(1))
    assert version >= 760 and _lib.VERSION == version
    assert re.search(r"^ \*\s+760\s+fxjps_refresh_slots", hdr, re.M), "no changelog line for version 760"
    exports = open(os.path.join(ROOT, "fuxi-planner_amd", "csrc", "exports.map")).read()
    patterns = re.findall(r"global:\s*([^;]+);", exports)
    for name in NEW:
        assert re.search(r"\bint %s\s*\(" % name, hdr), name
        assert any(fnmatch.fnmatchcase(name, p.strip()) for pat in patterns for p in pat.split()), name
        assert name in _lib.SYMBOLS
    assert re.search(r"int fxjps_refresh_slots\(fxjps_t\* h, fxjps_slot_job_t\* jobs, int32_t n, int32_t\* out_kept\);", hdr)


def test_the_job_struct_is_unchanged():
    from fuxi_planner_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "fxjps.h")).read()
    body = re.search(r"typedef struct fxjps_slot_job \{(.*?)\} fxjps_slot_job_t;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for ty, names in re.findall(r"(const void\*|int32_t)\s+([^;]+);", body):
        fields += [(re.sub(r"\[\d+\]", "", nm).strip(), ty, int((re.search(r"\[(\d+)\]", nm) or [0, 1])[1])) for nm in names.split(",")]
    assert len(re.findall(r";", body)) == len(re.findall(r"(const void\*|int32_t)\s+[^;]+;", body)), "a field of another type"
    assert fields == [("raw", "const void*", 1), ("slot", "int32_t", 1), ("layout", "int32_t", 1), ("W0", "int32_t", 1), ("H0", "int32_t", 1),
                      ("ifa", "int32_t", 1), ("variant", "int32_t", 1), ("start_xy", "int32_t", 2), ("goal_xy", "int32_t", 2), ("W", "int32_t", 1),
                      ("H", "int32_t", 1), ("map_d", "int32_t", 2), ("end_occu", "int32_t", 1), ("status", "int32_t", 1)], fields
    assert [f[0] for f in fields] == [f[0] for f in _lib.SlotJob._fields_]
    assert C.sizeof(_lib.SlotJob) == C.sizeof(C.c_void_p) + 16 * 4


def test_library_exports_the_call():
    import __graft_entry__
    from fuxi_planner_amd import _lib
    __graft_entry__.build()
    L = C.CDLL(_lib.LIB_PATH)
    assert L.fxjps_version() >= 760
    assert L.fxjps_slot_job_size() == C.sizeof(_lib.SlotJob)
    for name in NEW:
        assert hasattr(L, name), name
    # a NULL handle is refused before anything is read (no device is touched)
    L.fxjps_refresh_slots.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]
    assert L.fxjps_refresh_slots(None, None, 0, None) == _lib.E_ARG


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc")
def test_new_and_changed_kernels_exist_without_scratch():
    rows = _resource_usage()
    for k in REFRESH_KERNELS + PREPARE_KERNELS:
        hit = [v for name, v in rows.items() if re.search(r"\d+%sEv" % k, name)]
        assert len(hit) == 1, (k, sorted(rows))
        assert int(hit[0]["ScratchSize [bytes/lane]"]) == 0 and int(hit[0]["VGPRs Spill"]) == 0, (k, hit[0])
        assert int(hit[0].get("SGPRs Spill", 0)) == 0, (k, hit[0])
