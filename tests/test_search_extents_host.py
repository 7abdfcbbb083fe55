"""CPU suite: the host side of tests/test_search_extents_gpu.py -- the table-choice formula on every shape it plans, and the
conditions its shapes and queries were chosen by, from the reference alone: most queries searched, no path of 4096 points,
paths through the 13th bit of a coordinate, open lists beyond the two fast tiers at the table edge, and the classes of the
single lines."""
import re

import numpy as np
import pytest

import test_search_extents_gpu as ext
from test_search_extents_gpu import CHOICE, EDGE, GRIDS, LONG, SLOT_INPUTS, UNION_SLOTS, WIDE, check_conditions, fits, slots_fit
from test_search_work_gpu import inputs


def test_table_choice_formula_on_every_shape():
    """(W - 1).bit_length() + (H - 1).bit_length() <= 20, spelled out: which side of the choice each shape is on."""
    want = {"long x": True, "long y": True, "table edge x": True, "table edge y": True, "one wide x, empty": True, "one wide y, empty": True,
            "one wide x": True, "one wide y": True, "choice 2048x512": True, "choice 2049x512": False, "choice 1024x1025": False}
    assert set(want) == set(GRIDS)
    for name, (W, H, _, _) in GRIDS.items():
        assert fits(W, H) == want[name], (name, W, H)
    bits = {n: (GRIDS[n][0] - 1).bit_length() + (GRIDS[n][1] - 1).bit_length() for n in GRIDS}
    assert bits["table edge x"] == bits["table edge y"] == bits["choice 2048x512"] == 20
    assert bits["choice 2049x512"] == bits["choice 1024x1025"] == 21
    # the slot unions: the largest W and the largest H of the slots named
    assert slots_fit(list(UNION_SLOTS.values())) and max(w for w, _ in UNION_SLOTS.values()) == 2048 and max(h for _, h in UNION_SLOTS.values()) == 512
    assert not any(fits(W, H) is False for W, H in UNION_SLOTS.values())
    assert fits(8190, 16) and fits(16, 8190) and not slots_fit([(8190, 16), (16, 8190)])  # each alone is direct, together 26 bits
    ext.register_inputs()
    want_slots = {"extents union slots": True, "extents long slots": False, "extents tracked slots": False, "extents tracked union slots": True,
                  "extents tracked long-x slots": True}
    assert set(want_slots) == set(SLOT_INPUTS)
    for inp, w in want_slots.items():
        assert slots_fit(ext.slot_shapes(inp)) == w, inp
    assert (8190, 16) in ext.slot_shapes("extents tracked long-x slots")


def test_the_formula_is_the_hosts():
    """ensure_pool takes the cell-indexed layout from the rounded-up extents (each at least one bit) when a full set of
    wavefronts fits 40 % of the device: on an MI355X (256 CUs, 288 GB) that is 20 bits, as fits() says."""
    import os
    src = open(os.path.join(ext.ROOT, "fuxi-planner_amd", "csrc", "fxjps.hip")).read()
    assert re.search(r"lx = std::max\(ceil_log2\(\(uint64_t\)req\.W\), 1u\), ly = std::max\(ceil_log2\(\(uint64_t\)req\.H\), 1u\);", src)
    assert re.search(r"if \(allow && ld <= 23u && full \* \(\(uint64_t\)19 << ld\) <= cap\)", src)
    full, cap = 256 * 4 * 4, int(288e9 * 0.4)
    assert full * (19 << 20) <= cap < full * (19 << 21)
    for W, H, _, _ in GRIDS.values():  # (a one-cell extent counts one bit on the host, none in fits(): neither shape here is near the edge)
        ld = max((W - 1).bit_length(), 1) + max((H - 1).bit_length(), 1)
        assert (ld <= 20) == fits(W, H), (W, H)


def test_queries_are_what_the_issue_says():
    ext.register_inputs()
    for name, (W, H, p, n) in GRIDS.items():
        occ, s, g = inputs("extents " + name)
        assert occ.shape == (W, H) and len(s) == len(g) == n
        bw, bh = max(W // 16, 1), max(H // 16, 1)
        k = n // 2
        near = lambda c: (c[:, 0] < bw) & (c[:, 1] < bh)  # noqa: E731
        far = lambda c: (c[:, 0] >= W - bw) & (c[:, 1] >= H - bh)  # noqa: E731
        assert (near(s[:k:2]) & far(g[:k:2])).all() and (far(s[1:k:2]) & near(g[1:k:2])).all(), name
        assert (occ[g[:, 0], g[:, 1]] == 0).all(), name
    for name in LONG:
        occ, s, g = inputs("extents %s limits" % name)
        W, H = occ.shape
        assert s.tolist()[:2] == [[W, 0], [0, H]] and g.tolist()[2:5] == [[W, 0], [0, H], [W - 1, H]]
        assert s.tolist()[5] == g.tolist()[5] == [W - 1, H - 1] and (s.tolist()[6], g.tolist()[6]) == ([0, 0], [W - 1, H - 1])
    grids, ids, s, g = inputs("extents union slots")
    assert {k: v.shape for k, v in grids.items()} == UNION_SLOTS and np.bincount(ids).tolist() == [64, 64, 64]
    assert len(np.unique(np.diff(ids))) > 2  # (shuffled)


@pytest.mark.parametrize("group", ["long", "edge", "choice", "wide", "slots"])
def test_conditions_from_the_reference_alone(oracle, group):
    """The conditions test_search_extents_gpu asserts in front of its GPU runs, on the CPU alone, both heuristics."""
    names = {"long": LONG, "edge": EDGE, "choice": CHOICE, "wide": WIDE, "slots": SLOT_INPUTS}[group]
    fig = check_conditions(oracle, names)
    for k in sorted(fig):
        print(k, fig[k])
    assert len(fig) == 2 * len(names)
