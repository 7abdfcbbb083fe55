"""CPU suite: fxjps_set_slot_reuse and its two debug calls are declared, exported and bound at version
830, the mode defaults to 0, and the kernels the tile rule adds exist for gfx950 within the budget of the kernels beside
them: the tracking slots search (k_slot_reads_search<HC, DIRECT>) without a private segment or a VGPR spill, as the
tracking search of the resident grid (k_search<HC, true, DIRECT, false>), and the tile forms of the refresh gather and copy
with 1 KB of LDS beyond the refresh form's and nothing else.  Device pass only, one compile, no GPU needed."""
import ctypes as C
import os
import re

import pytest

from test_grid_slots_host import HIPCC, _resource_usage

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("fxjps_set_slot_reuse", "fxjps_debug_slot_tiles", "fxjps_debug_slot_read_sets")


def test_declared_exported_and_bound_at_830():
    from fuxi_planner_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "fxjps.h")).read()
    version = int(re.search(r"#define FXJPS_VERSION (\d+)", hdr).group(1))
    assert version >= 830 and _lib.VERSION == version
    assert re.search(r"^ \*\s+830\s+fxjps_set_slot_reuse", hdr, re.M), "no changelog line for version 830"
    for name in NEW:
        assert re.search(r"^int %s\(fxjps_t\* h, " % name, hdr, re.M), name
        assert name in _lib.SYMBOLS
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libfxjps.so is not built")
    L = C.CDLL(_lib.LIB_PATH)
    assert L.fxjps_version() >= 830
    for name in NEW:
        assert hasattr(L, name), name
    # a NULL handle is refused before anything is read (no device is touched)
    L.fxjps_set_slot_reuse.argtypes = [C.c_void_p, C.c_int32]
    L.fxjps_debug_slot_tiles.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
    L.fxjps_debug_slot_read_sets.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
    assert L.fxjps_set_slot_reuse(None, 1) == _lib.E_ARG
    assert L.fxjps_debug_slot_tiles(None, 0, None, None, None) == _lib.E_ARG
    assert L.fxjps_debug_slot_read_sets(None, None, 0, None, None) == _lib.E_ARG


def test_the_mode_defaults_to_0():
    from fuxi_planner_amd import planner
    assert planner.Planner._slot_reuse == 0 and planner.Planner.SLOT_REUSE_MODES == {"generation": 0, "tiles": 1}
    src = open(os.path.join(ROOT, "fuxi-planner_amd", "csrc", "fxjps.hip")).read()
    assert re.search(r"^\s*int slot_reuse = 0;", src, re.M)  # (the handle's member and its initialiser)
    hdr = open(os.path.join(ROOT, "include", "fxjps.h")).read()
    assert "mode 0 (the default) is the generation rule" in hdr


@pytest.fixture(scope="module")
def rows():
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    return _resource_usage()


def test_tracking_slots_search_keeps_to_the_budget_of_the_tracking_search(rows):
    new = {m.groups(): v for n, v in rows.items() for m in [re.search(r"k_slot_reads_searchILi(\d)ELb(\d)EE", n)] if m}
    old = {(m.group(1), m.group(2)): v for n, v in rows.items() for m in [re.search(r"k_searchILi(\d)ELb1ELb(\d)ELb0EE", n)] if m}
    assert set(new) == set(old) == {("1", "0"), ("1", "1"), ("2", "0"), ("2", "1")}, (sorted(new), sorted(old))
    for k, v in new.items():
        print(k, "VGPRs", v["VGPRs"], "scratch", v["ScratchSize [bytes/lane]"], "| resident-grid form: VGPRs", old[k]["VGPRs"], "scratch",
              old[k]["ScratchSize [bytes/lane]"])
        assert int(old[k]["ScratchSize [bytes/lane]"]) == 0 and int(old[k]["VGPRs Spill"]) == 0, (k, old[k])
        assert int(v["ScratchSize [bytes/lane]"]) == 0 and int(v["VGPRs Spill"]) == 0, (k, v)
        assert int(v["VGPRs"]) <= 128 and int(v["Occupancy [waves/SIMD]"]) >= 4, (k, v)
        assert v["LDS Size [bytes/block]"] == old[k]["LDS Size [bytes/block]"], (k, v, old[k])


def test_tile_forms_of_the_refresh_kernels(rows):
    tile = {n: v for n, v in rows.items() if "k_slot_tiles_" in n}
    assert len([n for n in tile if "k_slot_tiles_gatherILb" in n]) == 2 and len([n for n in tile if "k_slot_tiles_copyE" in n]) == 1, sorted(tile)
    assert len(tile) == 3
    plain = [v for n, v in rows.items() if "k_slots_gatherILb0ELb1EE" in n]  # (the REFRESH form: the LDS of its block-wide OR)
    assert len(plain) == 1
    for n, v in tile.items():
        assert int(v["LDS Size [bytes/block]"]) == int(plain[0]["LDS Size [bytes/block]"]) + 1024, (n, v, plain[0])
        assert int(v["ScratchSize [bytes/lane]"]) == 0 and int(v["VGPRs Spill"]) == 0 and int(v["SGPRs Spill"]) == 0, (n, v)
        assert v["Dynamic Stack"] == "False", (n, v)
