"""CPU suite: fxjps_prepare_slots (many raw maps into grid slots in one call) is declared, exported and bound, its six
kernels exist for gfx950 without a private segment, and the kernels it shares item functions with -- k_build_1 .. 3 -- and
every k_search instantiation compile to the figures recorded from the commit before it
(profiles/prepare_slots_resource_usage.json).  Device pass only, no GPU needed."""
import ctypes as C
import fnmatch
import json
import os
import re

import pytest

from test_grid_slots_host import HIPCC, _resource_usage

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("fxjps_prepare_slots", "fxjps_slot_job_size")
# (template instantiations, as they are spelled inside a mangled name: gather <WORLD, REFRESH>, goal <REFRESH>, stage <L, REFRESH>)
KERNELS = ("k_slots_gatherILb0ELb0EE", "k_slots_goalILb0EE", "k_slots_stageILi1ELb0EE", "k_slots_stageILi2ELb0EE", "k_slots_stageILi3ELb0EE",
           "k_slots_stageILi4ELb0EE")


def test_declared_exported_and_bound():
    from fuxi_planner_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "fxjps.h")).read()
    version = int(re.search(r"#define FXJPS_VERSION (\d+)", hdr).group(1))
    assert version >= 720 and _lib.VERSION == version
    assert re.search(r"^ \*\s+720\s+fxjps_prepare_slots", hdr, re.M), "no changelog line for version 720"
    exports = open(os.path.join(ROOT, "fuxi-planner_amd", "csrc", "exports.map")).read()
    patterns = re.findall(r"global:\s*([^;]+);", exports)
    for name in NEW:
        assert re.search(r"\bint %s\s*\(" % name, hdr), name
        assert any(fnmatch.fnmatchcase(name, p.strip()) for pat in patterns for p in pat.split()), name
        assert name in _lib.SYMBOLS
    # the ctypes mirror of fxjps_slot_job_t: one pointer and plain 32-bit fields, in the header's order
    body = re.search(r"typedef struct fxjps_slot_job \{(.*?)\} fxjps_slot_job_t;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for ty, names in re.findall(r"(const void\*|int32_t)\s+([^;]+);", body):
        fields += [re.sub(r"\[\d+\]", "", nm).strip() for nm in names.split(",")]
    assert len(re.findall(r";", body)) == len(re.findall(r"(const void\*|int32_t)\s+[^;]+;", body)), "a field of another type"
    assert fields == [f[0] for f in _lib.SlotJob._fields_], (fields, _lib.SlotJob._fields_)
    assert C.sizeof(_lib.SlotJob) == C.sizeof(C.c_void_p) + 16 * 4


def test_library_reports_the_job_size_the_binding_has():
    import __graft_entry__
    from fuxi_planner_amd import _lib
    __graft_entry__.build()
    L = C.CDLL(_lib.LIB_PATH)
    assert L.fxjps_version() >= 720
    assert L.fxjps_slot_job_size() == C.sizeof(_lib.SlotJob)
    assert hasattr(L, "fxjps_prepare_slots")


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc")
def test_kernels_exist_without_scratch_and_the_shared_ones_are_unchanged():
    rows = _resource_usage()
    for k in KERNELS:
        hit = [v for name, v in rows.items() if re.search(r"\d+%sEv" % k, name)]
        assert len(hit) == 1, (k, sorted(rows))
        assert int(hit[0]["ScratchSize [bytes/lane]"]) == 0 and int(hit[0]["VGPRs Spill"]) == 0, (k, hit[0])
    with open(os.path.join(ROOT, "profiles", "prepare_slots_resource_usage.json")) as f:
        rec = json.load(f)
    shared = {name: v for name, v in rows.items() if re.search(r"k_build_[123]|k_search", name)}
    assert len([n for n in shared if "k_search" in n]) == 12 and len(shared) == 15, sorted(shared)
    assert shared == rec["parent"], sorted(n for n in shared if shared[n] != rec["parent"].get(n))
    assert rec["this"] == rec["parent"]
