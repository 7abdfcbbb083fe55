"""CPU suite: what the slotless open list and the 1024-cell collision detector cost the search kernels in registers and LDS,
from a device-only compile (-Rpass-analysis=kernel-resource-usage), against the figures of the commit before them
(profiles/slotless_open_list_resource_usage.json: `parent` beside `this`).  No GPU needed.

The untracked searches on cell-indexed tables, k_search<HC, false, true, MG>, carry no slot payload and hold a detector of
twice the size: fewer registers, more LDS -- and the LDS arithmetic of the launches must still hold: two blocks per CU for
the batch launch, and for the head launch one block beside the 36 KB pad with no room for a second.  Every other search
kernel (hashed tables, read-set recording) is the code it was: the parent's figures, all of them.
"""
import json
import os
import re

import pytest

from test_grid_slots_host import HIPCC, _resource_usage

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LDS_PER_CU = 163840   # 160 KB
HEAD_PAD = 36 << 10   # launch_search's dynamic LDS of the head launch (fxjps.hip)


@pytest.fixture(scope="module")
def rows():
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    return {k: v for k, v in _resource_usage().items() if re.search(r"\d+(k_search|k_slot_reads_search)I", k)}


@pytest.fixture(scope="module")
def rec():
    with open(os.path.join(ROOT, "profiles", "slotless_open_list_resource_usage.json")) as f:
        return json.load(f)


def inst(name):
    """(HC, TRK, DIRECT, MG) of a k_search instantiation, or None."""
    m = re.search(r"8k_searchILi(\d)ELb(\d)ELb(\d)ELb(\d)E", name)
    return (int(m.group(1)), m.group(2) == "1", m.group(3) == "1", m.group(4) == "1") if m else None


def slotless(name):
    i = inst(name)
    return i is not None and not i[1] and i[2]


def test_the_pad_is_the_one_the_host_launches_with():
    src = open(os.path.join(ROOT, "fuxi-planner_amd", "csrc", "fxjps.hip")).read()
    assert re.search(r"static const size_t pad = 36u << 10;", src)


def test_the_record_is_what_the_compiler_says(rows, rec):
    assert len(rows) == 16 and rows == rec["this"], sorted(n for n in rows if rows[n] != rec["this"].get(n))
    assert sorted(n for n in rows if slotless(n)) == rec["slotless"] and len(rec["slotless"]) == 4
    assert set(rec["parent"]) == set(rec["this"])


def test_headline_kernel_registers_and_lds(rows, rec):
    """k_search<2, false, true, false>, the kernel of the headline workload."""
    name = "_ZN2fx8k_searchILi2ELb0ELb1ELb0EEEvNS_10SearchArgsE"
    v, p = rows[name], rec["parent"][name]
    print(name, "parent", p, "this", v)
    assert int(v["VGPRs"]) <= int(p["VGPRs"]), (v["VGPRs"], p["VGPRs"])
    assert int(v["ScratchSize [bytes/lane]"]) == 0 and int(v["VGPRs Spill"]) == 0
    assert int(v["Occupancy [waves/SIMD]"]) == 4
    lds = int(v["LDS Size [bytes/block]"])
    assert 2 * lds <= LDS_PER_CU, lds                   # the batch launch: two blocks per CU
    assert lds + HEAD_PAD <= LDS_PER_CU, lds            # the head launch: the block and its pad fit ...
    assert lds + HEAD_PAD + lds > LDS_PER_CU, lds       # ... and no second block beside them


def test_every_slotless_kernel_fits_the_same_way(rows, rec):
    for name in rec["slotless"]:
        v, p = rows[name], rec["parent"][name]
        lds = int(v["LDS Size [bytes/block]"])
        assert int(v["VGPRs"]) <= int(p["VGPRs"]) and int(v["ScratchSize [bytes/lane]"]) == 0 and int(v["VGPRs Spill"]) == 0, (name, v, p)
        assert int(v["Occupancy [waves/SIMD]"]) == 4, (name, v)
        assert 2 * lds <= LDS_PER_CU and lds + HEAD_PAD <= LDS_PER_CU < 2 * lds + HEAD_PAD, (name, lds)


def test_hashed_and_tracking_kernels_are_the_parents(rows, rec):
    others = [n for n in rows if not slotless(n)]
    assert len(others) == 12
    for name in others:
        assert rows[name] == rec["parent"][name], (name, rows[name], rec["parent"][name])
        assert rows[name]["LDS Size [bytes/block]"] == rec["parent"][name]["LDS Size [bytes/block]"]
