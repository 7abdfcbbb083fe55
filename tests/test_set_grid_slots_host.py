"""CPU suite: fxjps_set_grid_slots / fxjps_refresh_grid_slots (fxjps_set_grid_slot for many slots in one call) are declared,
exported and bound at version 820, the binding's GridJob mirrors the header's struct field by field, and both
instantiations of the copy kernel, k_slots_copy<REFRESH>, exist for gfx950 without a private segment or a spill and
compile to the figures recorded in profiles/set_grid_slots_resource_usage.json.  Device pass only, no GPU needed."""
import ctypes as C
import fnmatch
import json
import os
import re

import pytest

from test_grid_slots_host import HIPCC, _resource_usage

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("fxjps_set_grid_slots", "fxjps_refresh_grid_slots", "fxjps_grid_job_size")
COPY_KERNELS = ("k_slots_copyILb0EE", "k_slots_copyILb1EE")  # (as they are spelled inside a mangled name: <REFRESH>)
CTYPES = {"const uint8_t*": C.POINTER(C.c_uint8), "int32_t": C.c_int32}


def test_declared_exported_and_bound():
    from fuxi_planner_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "fxjps.h")).read()
    version = int(re.search(r"#define FXJPS_VERSION (\d+)", hdr).group(1))
    assert version >= 820 and _lib.VERSION == version
    assert re.search(r"^ \*\s+820\s+fxjps_set_grid_slots, fxjps_refresh_grid_slots", hdr, re.M), "no changelog line for version 820"
    exports = open(os.path.join(ROOT, "fuxi-planner_amd", "csrc", "exports.map")).read()
    patterns = re.findall(r"global:\s*([^;]+);", exports)
    for name in NEW:
        assert re.search(r"\bint %s\s*\(" % name, hdr), name
        assert any(fnmatch.fnmatchcase(name, p.strip()) for pat in patterns for p in pat.split()), name
        assert name in _lib.SYMBOLS
    assert re.search(r"int fxjps_set_grid_slots\(fxjps_t\* h, const fxjps_grid_job_t\* jobs, int32_t n\);", hdr)
    assert re.search(r"int fxjps_refresh_grid_slots\(fxjps_t\* h, const fxjps_grid_job_t\* jobs, int32_t n, int32_t\* out_kept\);", hdr)


def test_the_binding_mirrors_the_job_struct():
    from fuxi_planner_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "fxjps.h")).read()
    body = re.search(r"typedef struct fxjps_grid_job \{(.*?)\} fxjps_grid_job_t;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for ty, names in re.findall(r"(const uint8_t\*|int32_t)\s+([^;]+);", body):
        fields += [(nm.strip(), ty) for nm in names.split(",")]
    assert len(re.findall(r";", body)) == len(re.findall(r"(const uint8_t\*|int32_t)\s+[^;]+;", body)), "a field of another type"
    assert fields == [("occ", "const uint8_t*"), ("slot", "int32_t"), ("W", "int32_t"), ("H", "int32_t"), ("reserved", "int32_t")], fields
    assert [(n, t) for n, t in _lib.GridJob._fields_] == [(n, CTYPES[t]) for n, t in fields]
    assert C.sizeof(_lib.GridJob) == C.sizeof(C.c_void_p) + 4 * 4


def test_library_exports_the_calls():
    import __graft_entry__
    from fuxi_planner_amd import _lib
    __graft_entry__.build()
    L = C.CDLL(_lib.LIB_PATH)
    assert L.fxjps_version() >= 820
    assert L.fxjps_grid_job_size() == C.sizeof(_lib.GridJob)
    for name in NEW:
        assert hasattr(L, name), name
    # a NULL handle is refused before anything is read (no device is touched)
    L.fxjps_set_grid_slots.argtypes = [C.c_void_p, C.c_void_p, C.c_int32]
    L.fxjps_refresh_grid_slots.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]
    assert L.fxjps_set_grid_slots(None, None, 0) == _lib.E_ARG
    assert L.fxjps_refresh_grid_slots(None, None, 0, None) == _lib.E_ARG


@pytest.fixture(scope="module")
def rows():
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    return _resource_usage()


def test_both_copy_kernels_exist_without_scratch_or_spills(rows):
    for k in COPY_KERNELS:
        hit = [v for name, v in rows.items() if re.search(r"\d+%sEv" % k, name)]
        assert len(hit) == 1, (k, sorted(rows))
        assert int(hit[0]["ScratchSize [bytes/lane]"]) == 0 and int(hit[0]["VGPRs Spill"]) == 0 and int(hit[0]["SGPRs Spill"]) == 0, (k, hit[0])
        assert hit[0]["Dynamic Stack"] == "False", (k, hit[0])
    # no other form of the kernel, and it is no instantiation of the gather
    assert len([n for n in rows if "k_slots_copy" in n]) == 2
    assert len([n for n in rows if "k_slots_gather" in n]) == 4


def test_their_figures_are_the_recorded_ones(rows):
    with open(os.path.join(ROOT, "profiles", "set_grid_slots_resource_usage.json")) as f:
        record = json.load(f)["this"]
    assert len(record) == 2 and all(any(k in name for k in COPY_KERNELS) for name in record)
    for name, want in record.items():
        assert rows[name] == want, (name, rows[name], want)
