"""CPU suite: the map half of a fleet tick is three kernel templates -- k_slots_gather<WORLD, REFRESH>, k_slots_goal<REFRESH>,
k_slots_stage<L, REFRESH> -- whose 14 instantiations took the places of 14 separate kernels.  The translation unit holds
exactly those 14 and none of the kernels they replaced; each compiles to the figures recorded in
profiles/slot_kernel_family_resource_usage.json (`this`), and against the kernel it replaced (`parent`: compiled from the
commit before, same flags) it has no more VGPRs and the same LDS, occupancy, scratch and spills.  Device pass only, one
compile, no GPU needed."""
import json
import os
import re

import pytest

from test_grid_slots_host import HIPCC, _resource_usage

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EQUAL = ("LDS Size [bytes/block]", "Occupancy [waves/SIMD]", "ScratchSize [bytes/lane]", "VGPRs Spill", "SGPRs Spill", "AGPRs", "Dynamic Stack")


def short(mangled):
    """_ZN2fx15k_whateverEPK... / _ZN2fx14k_whateverILb0EEEvPK... -> k_whatever"""
    m = re.match(r"_ZN2fx(\d+)", mangled)
    return mangled[m.end():m.end() + int(m.group(1))] if m else ""


def is_template(mangled):
    """(the identifier of a template instantiation is followed by its arguments, I .. E; of a plain function by the E that ends the name)"""
    return mangled[len("_ZN2fx%d%s" % (len(short(mangled)), short(mangled)))] == "I"


@pytest.fixture(scope="module")
def record():
    with open(os.path.join(ROOT, "profiles", "slot_kernel_family_resource_usage.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def rows():
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    return _resource_usage()


def test_record_pairs_fourteen_kernels_with_fourteen_instantiations(record):
    parent, this, replaces = record["parent"], record["this"], record["replaces"]
    assert len(parent) == 14 and len(this) == 14
    assert sorted(replaces) == sorted(parent) and sorted(replaces.values()) == sorted(this)
    assert {short(n) for n in this} == {"k_slots_gather", "k_slots_goal", "k_slots_stage"}
    count = lambda name: len([n for n in this if short(n) == name])
    assert (count("k_slots_gather"), count("k_slots_goal"), count("k_slots_stage")) == (4, 2, 8)
    assert not any(is_template(n) for n in parent) and all(is_template(n) for n in this)


def test_the_family_is_exactly_the_recorded_instantiations(rows, record):
    old = {short(n) for n in record["parent"]}
    new = {short(n) for n in record["this"]}
    family = {n for n in rows if short(n) in old | new}
    assert family == set(record["this"]), sorted(family ^ set(record["this"]))
    # (k_slots_goal is the one name a template kept: what is gone is the kernel that was no template)
    assert not set(rows) & set(record["parent"])
    src = open(os.path.join(ROOT, "fuxi-planner_amd", "csrc", "fxjps_maps.hip.inc")).read() + \
        open(os.path.join(ROOT, "fuxi-planner_amd", "csrc", "fxjps.hip")).read()
    for name in old - new:
        assert not re.search(r"\b%s\b" % name, src), name


def test_each_instantiation_compiles_to_its_record(rows, record):
    for name, want in record["this"].items():
        assert rows[name] == want, (name, rows[name], want)


def test_no_instantiation_costs_more_than_the_kernel_it_replaced(rows, record):
    for was, now in record["replaces"].items():
        p, t = record["parent"][was], rows[now]
        assert int(t["VGPRs"]) <= int(p["VGPRs"]), (was, now, p, t)
        for key in EQUAL:
            assert t[key] == p[key], (was, now, key, p, t)
        assert int(t["ScratchSize [bytes/lane]"]) == 0 and int(t["VGPRs Spill"]) == 0 and int(t["SGPRs Spill"]) == 0, (now, t)
