"""The ticks that tests/test_refresh_grid_gpu.py feeds fxjps_refresh_grid, and what the host says about each of them
(tests/test_refresh_grid_host.py checks this file with oracle/gridprep.py alone, no GPU).

A case is (W0, H0, ifa, variant); `steps` makes its ticks.  A step is a dict:
  name         what the step is about
  pre          None, or what is done to the resident grid in front of the call:
               ("poke", cells, deferred)  fxjps_update_cells(_deferred) flips these cells (flat indices x * H + y)
               ("bytes", cells, byte)     fxjps_set_grid puts `byte` into these cells of the resident grid
  raw          bool [W0][H0], start, goal: the call's arguments
  mode         the mode the step is there for, or None: whatever the rule below gives
`simulate` is the host's account of a call: the prepared grid (oracle.gridprep), the cells in which it differs from the
resident bytes in ascending order of the flat index, and the mode by the rule of include/fxjps.h."""
import numpy as np

from oracle import gridprep

SHAPES = ((5, 7), (70, 37), (300, 300))
# (ifa 0 with the st variant is not among these cases: the reference's `range(-ifa, ifa + 1, ifa)` raises there, so
# oracle.gridprep has no answer.  The GPU suite runs it against the twin handle alone.)
CASES = [(W0, H0, ifa, variant) for (W0, H0) in SHAPES for ifa in (0, 1, 2) for variant in (0, 1) if (ifa, variant) != (0, 0)]
BLOCK = 256  # cells per block of the diff launches


def capacity(W, H):
    return max(4096, W * H // 8)


def to_msg(raw, seed):
    """bool [W0][H0] -> a message's int8 data [H0 * W0]: occupied cells 50 or 100, free cells -1 or 0."""
    rng = np.random.default_rng(seed)
    occ = rng.choice(np.array([50, 100], np.int8), raw.shape)
    free = rng.choice(np.array([-1, 0], np.int8), raw.shape)
    return np.ascontiguousarray(np.where(raw, occ, free).T).reshape(-1)


def simulate(resident, raw, start, goal, ifa, variant):
    """-> (prepared grid, start', goal', map_d, end_occu, cells int[n, 2], vals uint8[n], changed, mode)"""
    grid, s, g, md, eo = gridprep.prepare_full(raw.astype(np.uint8), start, goal, ifa, variant)
    if resident is None or resident.shape != grid.shape:
        return grid, s, g, md, eo, np.zeros((0, 2), np.int64), np.zeros(0, np.uint8), -1, 2
    cells = np.argwhere(resident != grid)
    vals = grid[cells[:, 0], cells[:, 1]]
    n = len(cells)
    mode = 0 if n == 0 else 1 if n <= capacity(*grid.shape) else 2
    return grid, s, g, md, eo, cells, vals, n, mode


def apply_pre(resident, pre):
    """The resident bytes after a step's `pre`."""
    if pre is None:
        return resident
    out = resident.copy()
    if pre[0] == "poke":
        out.flat[pre[1]] = 1 - (out.flat[pre[1]] != 0)
    else:
        out.flat[pre[1]] = pre[2]
    return out


def steps(W0, H0, ifa, variant, seed=5):
    rng = np.random.default_rng(seed + 1000 * W0 + 10 * ifa + variant)
    sh = 1 if variant == 0 else 0
    R = rng.random((W0, H0)) < 0.2
    R[0, 0] = R[-1, -1] = False
    R[W0 - 4:, H0 - 4:] = False   # (free around the goal: the step that occupies it changes something)
    R[1, 2] = True                # (an occupied cell for the goal to be moved onto)
    start, goal = (1, 1), (W0 - 2, H0 - 2)
    W1, H1 = W0 + 6 * ifa, H0 + 6 * ifa  # (start and goal inside the raw map)
    n = W1 * H1
    out = []

    def add(name, raw, s=start, g=goal, mode=None, pre=None):
        out.append(dict(name=name, raw=raw.copy(), start=s, goal=g, mode=mode, pre=pre))

    add("no grid resident", R, mode=2)
    add("the same raw", R, mode=0)
    add("the same raw, a second time", R, mode=0)
    R[0, 0] = True
    add("the raw's first cell", R, mode=1)
    R[-1, -1] = True
    add("the raw's last cell", R, mode=1)
    a = BLOCK - 1 if n > BLOCK + 1 else n // 2  # (the last cell of a block and the first of the next; a one-block grid: two neighbours)
    add("prepared cells %d and %d" % (a, a + 1), R, mode=1, pre=("poke", [a, a + 1], False))
    add("the first and the last cell of the last block", R, mode=1, pre=("poke", [(n - 1) // BLOCK * BLOCK, n - 1], False))
    add("the goal moved onto an obstacle", R, g=(1 + sh, 2 + sh), mode=0)
    R[-1, -1] = False
    R[W0 - 2 - sh, H0 - 2 - sh] = True
    add("a change that occupies the goal", R, mode=1)
    if ifa > 0:
        add("other extents: the goal beyond the raw map", R, g=(W0 + 1, H0 - 2), mode=2)
        add("the padding moved by one cell, equal extents", R, s=(-1, 1), g=(W0, H0 - 2))
    else:  # (without a margin a goal beyond the raw map lies outside the prepared grid: no way to equal extents there)
        add("other extents: the start left of the raw map", R, s=(-1, 1), mode=2)
    add("other extents: back", R, mode=2)
    Ri = ~R
    Ri[W0 - 2 - sh, 0] = False  # (a free cell in the goal's row)
    add("the raw inverted", Ri)
    add("the raw inverted back", R)
    k = min(5000, n // 2)  # (at 300 x 300: more entries than the 4096 that travel with the header, fewer than the capacity)
    add("every other cell of the first %d" % (2 * k), R, mode=1, pre=("poke", list(range(0, 2 * k, 2)), False))
    grid = gridprep.prepare_full(R.astype(np.uint8), start, goal, ifa, variant)[0]
    occ, free = np.flatnonzero(grid), np.flatnonzero(grid == 0)
    add("bytes 7 in the resident grid", R, mode=1, pre=("bytes", [int(occ[0]), int(occ[-1]), int(free[len(free) // 2])], 7))
    add("behind a deferred update", R, mode=1, pre=("poke", [int(free[0]), int(occ[len(occ) // 2]), n - 1], True))
    return out
