"""CPU suite: fxjps_publish_slots (the message and / or snapshot image of every named grid slot in one call) and
fxjps_slot_publish_size are declared, exported and bound, the binding's job struct is the library's, the kernel exists for
gfx950 without a private segment, and the kernels whose resource usage is recorded -- k_build_1 .. 3 and every k_search
instantiation -- still compile to those figures with the new kernel in the translation unit.  Device pass only, no GPU
needed."""
import ctypes as C
import fnmatch
import inspect
import json
import os
import re

import pytest

from test_grid_slots_host import HIPCC, _resource_usage

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("fxjps_publish_slots", "fxjps_slot_publish_size")


def test_declared_exported_and_bound():
    from fuxi_planner_amd import _lib
    from fuxi_planner_amd.planner import Planner
    hdr = open(os.path.join(ROOT, "include", "fxjps.h")).read()
    version = int(re.search(r"#define FXJPS_VERSION (\d+)", hdr).group(1))
    assert version >= 740 and _lib.VERSION == version
    assert re.search(r"^ \*\s+740\s+%s" % NAMES[0], hdr, re.M), "no changelog line for version 740"
    exports = open(os.path.join(ROOT, "fuxi-planner_amd", "csrc", "exports.map")).read()
    patterns = re.findall(r"global:\s*([^;]+);", exports)
    for name in NAMES:
        assert re.search(r"\bint %s\s*\(" % name, hdr), name
        assert any(fnmatch.fnmatchcase(name, p.strip()) for pat in patterns for p in pat.split()), name
        assert name in _lib.SYMBOLS
    assert re.search(r"int fxjps_publish_slots\(fxjps_t\* h, fxjps_slot_publish_t\* jobs, int32_t n\);", hdr)
    sig = inspect.signature(Planner.publish_slots)
    assert list(sig.parameters) == ["self", "slots", "msg", "image_channels"]
    assert sig.parameters["msg"].default is True and sig.parameters["image_channels"].default is None


def test_library_has_the_symbols_and_the_binding_its_struct():
    import __graft_entry__
    from fuxi_planner_amd import _lib
    __graft_entry__.build()
    L = C.CDLL(_lib.LIB_PATH)
    assert L.fxjps_version() >= 740
    for name in NAMES:
        assert hasattr(L, name), name
    L.fxjps_slot_publish_size.restype = C.c_int
    assert L.fxjps_slot_publish_size() == C.sizeof(_lib.SlotPublish)
    assert [f[0] for f in _lib.SlotPublish._fields_] == ["msg_data", "image", "slot", "channels", "W", "H"]
    assert len(_lib.load().fxjps_publish_slots.argtypes) == 3


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc")
def test_kernel_exists_without_scratch_and_the_recorded_ones_are_unchanged():
    rows = _resource_usage()
    hit = [v for name, v in rows.items() if re.search(r"\d+k_publish_slotsE", name)]
    assert len(hit) == 1, sorted(rows)
    assert int(hit[0]["ScratchSize [bytes/lane]"]) == 0 and int(hit[0]["VGPRs Spill"]) == 0 and int(hit[0]["SGPRs Spill"]) == 0, hit[0]
    with open(os.path.join(ROOT, "profiles", "prepare_slots_resource_usage.json")) as f:
        rec = json.load(f)
    shared = {name: v for name, v in rows.items() if re.search(r"k_build_[123]|k_search", name)}
    assert len([n for n in shared if "k_search" in n]) == 12 and len(shared) == 15, sorted(shared)
    assert shared == rec["parent"], sorted(n for n in shared if shared[n] != rec["parent"].get(n))
