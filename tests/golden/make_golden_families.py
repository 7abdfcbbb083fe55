#!/usr/bin/env python3
"""Generate tests/golden/families.json by IMPORTING the real reference (as make_golden.py does: build container only).

The GPU suite leans on map families that no other golden file covers: wide-open and 1 % maps (hundreds of equal-f ties
under hchoice 1), rooms with doors and a sealed pocket, the notched serpentine, one- and two-cell-wide grids,
checkerboards (every diagonal step is a squeeze), diagonal walls.  This script runs the reference's jps1.method on one
small grid of each, through make_golden.run_ref -- its record and its counting proxy: path, cost_hex, printed cost,
cells / pushes / pops -- so that the C oracle's tie order and corner rule are pinned to the reference THERE as well.

    python tests/golden/make_golden_families.py

Per grid: the first free cell to the last and back, ten random pairs of free cells (the rooms map: two more, into and out
of its sealed pocket), every query under both heuristics.  The file holds inputs and outputs only:
    {"families": [{"family": name, "shape": [W, H], "grid_bits": packed bits as hex, "records": [run_ref records]}]}
"""
import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import numpy as np  # noqa: E402

from make_golden import dump, run_ref  # noqa: E402  (puts the reference and the repository root on sys.path)

FAMILIES = ("empty 60x45", "empty 150x110", "sparse 120x90", "rooms 65x65", "serpentine 34x34", "line 1x200", "line 200x1", "strip 2x90",
            "checkerboard 30x30", "diagonal wall 50x50", "thick diagonal wall 50x50")
POCKET = (40, 40)  # a free cell inside the sealed pocket of the rooms map


def rooms(rng):
    """65 x 65: walls every 16 cells, one random door per wall segment, a sealed pocket of 3 x 3 free cells."""
    occ = np.zeros((65, 65), dtype=np.uint8)
    occ[::16, :] = 1
    occ[:, ::16] = 1
    for k in range(1, 4):
        for j in range(4):
            occ[16 * k, 16 * j + int(rng.integers(1, 16))] = 0
            occ[16 * j + int(rng.integers(1, 16)), 16 * k] = 0
    occ[36:45, 36:45] = 1
    occ[39:42, 39:42] = 0
    return occ


def serpentine(W, H):
    """The map of test_gpu_parity.test_a_path_longer_than_the_default_slot: corridors joined at alternating ends, a notch
    above every other cell of a corridor (a forced neighbour there)."""
    occ = np.ones((W, H), np.uint8)
    rows = list(range(1, H - 2, 3))
    for i, y in enumerate(rows):
        occ[1:W - 1, y] = 0
        occ[2:W - 2:2, y + 1] = 0
        if i + 1 < len(rows):
            occ[W - 2 if i % 2 == 0 else 1, y:rows[i + 1] + 1] = 0
    return occ


def diagonal_wall(n, thick):
    """An anti-diagonal wall that leaves three cells free at either end: no diagonal step may cross it, the way is round."""
    occ = np.zeros((n, n), dtype=np.uint8)
    for i in range(3, n - 3):
        occ[i, n - 1 - i] = 1
        if thick:
            occ[i, n - 2 - i] = 1
    return occ


def grids():
    rng = np.random.default_rng(20261020)
    out = {"empty 60x45": np.zeros((60, 45), np.uint8), "empty 150x110": np.zeros((150, 110), np.uint8),
           "sparse 120x90": (rng.random((120, 90)) < 0.01).astype(np.uint8), "rooms 65x65": rooms(rng), "serpentine 34x34": serpentine(34, 34),
           "line 1x200": (rng.random((1, 200)) < 0.02).astype(np.uint8), "line 200x1": np.zeros((200, 1), np.uint8),
           "strip 2x90": (rng.random((2, 90)) < 0.10).astype(np.uint8),
           "checkerboard 30x30": (np.add.outer(np.arange(30), np.arange(30)) % 2).astype(np.uint8),
           "diagonal wall 50x50": diagonal_wall(50, False), "thick diagonal wall 50x50": diagonal_wall(50, True)}
    assert tuple(out) == FAMILIES
    return out, rng


def queries(name, occ, rng):
    free = [tuple(int(v) for v in c) for c in np.argwhere(occ == 0)]
    qs = [(free[0], free[-1]), (free[-1], free[0])]
    for _ in range(10):
        a, b = rng.integers(0, len(free), 2)
        qs.append((free[a], free[b]))
    if name.startswith("rooms"):
        assert occ[POCKET] == 0
        qs += [(free[0], POCKET), ((POCKET[0], POCKET[1] + 1), free[-1])]
    return qs


def main():
    out = []
    gs, rng = grids()
    n = nopath = 0
    for name, occ in gs.items():
        recs = []
        for s, g in queries(name, occ, rng):
            for h in (2, 1):
                recs.append(run_ref(occ.astype(np.float64), s, g, h))
                nopath += recs[-1]["path"] is None
        n += len(recs)
        out.append({"family": name, "shape": list(occ.shape), "grid_bits": np.packbits(occ).tobytes().hex(), "records": recs})
    print("%d records, %d without a path" % (n, nopath))
    dump("families.json", {"families": out})


if __name__ == "__main__":
    main()
