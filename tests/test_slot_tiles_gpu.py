"""GPU suite (-m gpu): fxjps_replan_slots under the tile rule (fxjps_set_slot_reuse(1)) -- a stored
path is handed back although its slot's bytes changed, when no changed cell touches a read-set tile of its search.

The yardstick everywhere is a twin handle in mode 0 that gets the same slot calls and plans with plan_batch_slots: offsets,
lengths, costs, cells, fxjps_last_cells and the tick_outputs_slots outputs are compared byte for byte after every tick,
the first tick also with the CPU oracle per slot.  What only mode 1 has -- the flags 0 / 1 / 2, the changed-tile records
and the stored read sets -- is checked against oracle/read_sets.py and the cells the reference reads (oracle.read_sets).

The fleet (prepared extents): slot 0 40 x 33 (tsh 0, ccst, ifa 0), slot 1 130 x 70 (tsh 2, ccst, ifa 0), slot 2 300 x 257
(tsh 3, st, ifa 2: a raw flip changes nine prepared cells that span a 5 x 5 box; the st preparation needs ifa > 0), all
through refresh_slots, and slot 3 37 x 27 (999 cells: no multiple of 16) through refresh_grid_slots.  The prepared grids are
random at 20 % density; for slot 2 that is a raw density of 1 - 0.8^(1/9) = 2.4 %, the 9 being the cells of the st dilation
(a raw map at 20 % would prepare to 87 % occupied and hold hardly a path).  Around the raw cells of slot 2 that the ticks
flip, the raw map is cleared 5 x 5, so that each of those flips changes its prepared cell whatever the draw was.  Starts and goals are free cells of [W/16, 3W/8) x [H/16, 3H/8), 24 queries per raw-map slot and
6 on slot 3, numpy.random.default_rng(830); on slot 0 also a goal walled in (NOPATH) and a start off the grid (BAD_START).
max_path_len is the longest path but the longest one's, so that one is PATH_TOO_LONG.

Cells with x >= 5W/8 and y >= 5H/8 share no tile row or column with a cell a search read (max read < W/2, H/2; whole-row
marks of reach class 3 stay in the rows and columns read); the test asserts that bound on the oracle's reads first."""
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import gridprep
from oracle import read_sets as rs

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RESO, MAP_O = 0.25, (-2.0, 1.0)
# slot -> (prepared W, H, ifa, variant)
RAW_SLOTS = {0: (40, 33, 0, 1), 1: (130, 70, 0, 1), 2: (300, 257, 2, 0)}
GRID_SLOT, GRID_WH = 3, (37, 27)
RAW_DENSITY = {0: 0.2, 2: 1.0 - 0.8 ** (1.0 / 9.0)}  # (prepared: 20 % either way)
NQ_RAW, NQ_GRID = 24, 6
Q_CAPACITY = -3


def words_of(T):
    """bool[64, 64] indexed [tx, ty] -> the 128 words that mark exactly those tiles in both halves."""
    out = np.zeros(128, dtype=np.uint64)
    for tx, ty in np.argwhere(T):
        out[ty] |= np.uint64(1) << np.uint64(tx)
        out[64 + tx] |= np.uint64(1) << np.uint64(ty)
    return out


def flat(x):
    if isinstance(x, (list, tuple)):
        return b"|".join(flat(v) for v in x)
    return np.ascontiguousarray(x).tobytes()


def far_cell(W, H, d, k=0):
    """A prepared cell of the far corner (x >= 5W/8, y >= 5H/8) that a raw cell lies under; d = 2 ifa."""
    x, y = W - 3 - 2 * d - k, H - 3 - 2 * d - 2 * k
    assert 8 * (x - 1 - d) >= 5 * W and 8 * (y - 1 - d) >= 5 * H  # (with the st dilation's reach of d cells, and the box's one)
    return x, y


def flip_cases(W, H, d):
    """The single-cell flips of test 1 on a W x H prepared grid (raw cell (x - d, y - d) lies under (x, y)): the first and the
    last cell a raw cell reaches, and for tsh >= 2 both sides of a tile edge in x and in y and the first cell of the last tile
    reached (the grid's last, partial tile when d == 0)."""
    tsh = rs.tile_shift(W, H)
    cases = [(d, d), (W - 1 - 2 * d, H - 1 - 2 * d)]
    if tsh >= 2:
        cases += [((5 << tsh) - 1, 3 << tsh), (5 << tsh, (3 << tsh) - 1), ((W - 1 - 2 * d) >> tsh << tsh, 8 << tsh)]
    return cases


def inputs():
    """The fleet's maps, jobs and queries (no GPU) -> dict: raw {slot: raw map}, geo {slot: (d, sh)}, job {slot: raw -> job},
    grid3, ids, starts, goals, NOPATH, BAD."""
    rng = np.random.default_rng(830)
    raws, jobs, geo = {}, {}, {}
    ids, starts, goals = [], [], []
    for s, (W, H, ifa, variant) in RAW_SLOTS.items():
        W0, H0 = W - 6 * ifa, H - 6 * ifa
        raw = (rng.random((W0, H0)) < RAW_DENSITY[ifa]).astype(np.uint8)
        if s == 0:  # a closed ring around (19, 16): NOPATH's goal
            raw[17:22, 14:19] = 1
            raw[19, 16] = 0
        d, sh = 2 * ifa, 1 if variant == 0 else 0  # raw (x, y) lies at prepared (x + d, y + d); sh moves only start and goal
        if ifa > 0:
            for x, y in flip_cases(W, H, d) + [far_cell(W, H, d, k) for k in (0, 1)]:
                raw[max(x - d - ifa, 0):x - d + ifa + 1, max(y - d - ifa, 0):y - d + ifa + 1] = 0
        grid = gridprep.prepare_full(raw, (5, 5), (6, 6), ifa, variant)[0]
        assert grid.shape == (W, H)
        free = [(x, y) for x in range(W // 16, 3 * W // 8) for y in range(H // 16, 3 * H // 8) if grid[x, y] == 0]
        pick = rng.choice(len(free), 2 * NQ_RAW, replace=False)
        st, go = [free[i] for i in pick[:NQ_RAW]], [free[i] for i in pick[NQ_RAW:]]
        raws[s], geo[s] = raw, (d, sh)
        jobs[s] = lambda raw, s=s, a=st[0], g=go[0], d=d, sh=sh, ifa=ifa, v=variant: (
            s, raw, (a[0] - d + sh, a[1] - d + sh), (g[0] - d + sh, g[1] - d + sh), ifa, v)
        ids += [s] * NQ_RAW
        starts += st
        goals += go
    W, H = GRID_WH
    g3 = (rng.random((W, H)) < 0.2).astype(np.uint8)
    free = [(x, y) for x in range(W // 16, 3 * W // 8) for y in range(H // 16, 3 * H // 8) if g3[x, y] == 0]
    pick = rng.choice(len(free), 2 * NQ_GRID, replace=False)
    ids += [GRID_SLOT] * NQ_GRID
    starts += [free[i] for i in pick[:NQ_GRID]]
    goals += [free[i] for i in pick[NQ_GRID:]]
    n = len(ids)
    ids += [0, 0]
    starts += [starts[0], (RAW_SLOTS[0][0] + 1, 0)]
    goals += [(19, 16), goals[0]]
    return dict(raw=raws, geo=geo, job=jobs, grid3=g3, ids=np.array(ids, np.int32), starts=np.array(starts, np.int32),
                goals=np.array(goals, np.int32), NOPATH=n, BAD=n + 1)


class Fleet(object):
    """Both handles (a: the tile rule, b: the twin in mode 0), the jobs and the queries of the ticks."""

    def __init__(self, oracle, hchoice=2):
        import fuxi_planner_amd as fx
        self.oracle, self.h = oracle, hchoice
        self.a, self.b = fx.Planner([0]), fx.Planner([0])
        self.a.set_slot_reuse("tiles")
        I = inputs()
        self.raw, self.geo, self.job, self.grid3 = I["raw"], I["geo"], I["job"], I["grid3"]
        self.ids, self.starts, self.goals, self.NOPATH, self.BAD = I["ids"], I["starts"], I["goals"], I["NOPATH"], I["BAD"]
        self.nq = len(self.ids)
        self.slots = sorted(RAW_SLOTS) + [GRID_SLOT]
        # the first fill, through the refresh calls (empty slots: every job builds, nothing is compared)
        self.grids = {}
        self.written = set()
        self.refresh()
        lens = self.oracle_lens(512)
        self.has_path = lens > 0
        top = int(lens.max())
        self.mpl = int(lens[lens < top].max())
        self.LONG = np.nonzero(lens == top)[0]
        assert lens[self.NOPATH] == 0 and lens[self.BAD] == -2 and self.mpl >= 3 and self.has_path.sum() >= 3 * NQ_RAW, lens
        assert all(self.has_path[self.of_slot(s)].sum() >= 4 for s in self.slots)
        self.stored = None  # the previous replan's (ids, starts, goals, len, read sets, have)
        self.changed = {s: np.zeros(self.grids[s].shape, bool) for s in self.slots}  # cells that differ since the last replan

    def close(self):
        self.a.close()
        self.b.close()

    # ---- slot calls, the same on both handles
    def both(self, name, *args):
        out = getattr(self.a, name)(*args)
        getattr(self.b, name)(*args)
        return out

    def refresh(self, raw_slots=None, grid=True):
        """refresh_slots for the raw-map slots named (default: all) and refresh_grid_slots for slot 3; -> kept per slot.
        After each, the slot's changed-tile record is checked against the bytes that differ."""
        before = {s: g.copy() for s, g in self.grids.items()}
        raw_slots = sorted(RAW_SLOTS) if raw_slots is None else raw_slots
        kept = {}
        if raw_slots:
            outs = self.both("refresh_slots", [self.job[s](self.raw[s]) for s in raw_slots])
            for s, o in zip(raw_slots, outs):
                assert o[5], (s, o)
                kept[s] = o[6]
        if grid:
            kept[GRID_SLOT] = self.both("refresh_grid_slots", [(GRID_SLOT, self.grid3)])[0]
        for s in kept:
            self.grids[s] = self.a.get_grid_slot(s)
            assert self.grids[s].tobytes() == self.b.get_grid_slot(s).tobytes(), s
            if s in before and before[s].shape == self.grids[s].shape:
                diff = before[s] != self.grids[s]
                assert kept[s] == (not diff.any()), (s, kept[s], int(diff.sum()))
                self.changed[s] |= diff
            if not kept[s]:
                self.written.add(s)
        return kept

    def check_record(self, s, valid=True):
        """The slot's record is exactly the tiles touched by the cells that differ since the last replan."""
        D, tsh, v = self.a.debug_slot_tiles(s)
        W, H = self.grids[s].shape
        assert tsh == rs.tile_shift(W, H) and v == valid, (s, tsh, v)
        want = words_of(rs.touched_tiles(np.argwhere(self.changed[s]), W, H))
        assert D.tobytes() == want.tobytes(), (s, [(t, hex(int(D[t])), hex(int(want[t]))) for t in range(128) if D[t] != want[t]][:6])
        return D

    # ---- the oracle
    def of_slot(self, s):
        return np.nonzero(self.ids == s)[0]

    def oracle_lens(self, max_len, with_cells=False):
        lens, cost, cells = np.zeros(self.nq, np.int32), np.zeros(self.nq), [None] * self.nq
        for s in self.slots:
            qs = self.of_slot(s)
            c, l, k, _ = self.oracle.plan_batch(self.grids[s], self.starts[qs], self.goals[qs], self.h, literal=False, max_len=max_len)
            lens[qs], cost[qs] = l, k
            for i, q in enumerate(qs):
                cells[q] = c[i, :max(int(l[i]), 0)].copy()
        return (lens, cost, cells) if with_cells else lens

    def oracle_reads(self, qs=None):
        """{q: bool[W, H]} the cells the reference reads, for the queries with a path (default: all of them)."""
        out = {}
        for s in self.slots:
            sel = [q for q in self.of_slot(s) if self.has_path[q] and (qs is None or q in qs)]
            if not sel:
                continue
            W, H = self.grids[s].shape
            bits, _ = self.oracle.read_sets(self.grids[s], self.starts[sel], self.goals[sel], self.h, nthreads=16)
            for i, q in enumerate(sel):
                out[q] = self.oracle.unpack_read_set(bits[i], W, H)
        return out

    # ---- a planning tick
    def expected_flags(self):
        """The rule of DESIGN.md section 3.18, restated from the debug calls and the writes this test made."""
        want = np.zeros(self.nq, np.int32)
        if self.stored is None:
            return want
        ids, starts, goals, lens, read, have = self.stored
        for q in range(self.nq):
            s = int(self.ids[q])
            if ids[q] != s or (starts[q] != self.starts[q]).any() or (goals[q] != self.goals[q]).any() or lens[q] == Q_CAPACITY:
                continue
            if s not in self.written:
                want[q] = 1
                continue
            D, _, valid = self.a.debug_slot_tiles(s)
            if valid and lens[q] > 0 and have[q] and not (read[q] & D).any():
                want[q] = 2
        return want

    def tick(self, tag):
        """replan_slots on a, plan_batch_slots on the twin: equal bytes; the flags are the restated rule's -> (flags, result)."""
        import ctypes as C
        from fuxi_planner_amd import _lib, waypoints
        want_flags = self.expected_flags()
        before = self.oracle_reads() if self.stored is not None else {}
        got = self.a.replan_slots(self.ids, self.starts, self.goals, self.h, self.mpl)
        T = self.a.timing()
        want = self.b.plan_batch_slots(self.ids, self.starts, self.goals, self.h, self.mpl)
        for k, name in enumerate(("offsets", "cells", "cost", "status")):
            assert got[k].tobytes() == want[k].tobytes(), (tag, name)
        last = [np.zeros((max(len(got[1]), 1), 2), np.int32) for _ in range(2)]
        for p, buf in zip((self.a, self.b), last):
            if len(got[1]):
                p._chk(p._L.fxjps_last_cells(p._h, _lib.ptr(buf, C.c_int32), len(got[1])))
        assert last[0].tobytes() == last[1].tobytes() and (len(got[1]) == 0 or last[0].tobytes() == got[1].tobytes()), tag
        # every query as a vehicle of its slot's rule (slot 3: ccst), with a pose at its start and a goal at its goal
        v = [int(s) for s in self.ids]
        dd = [self.geo[s][0] if s in self.geo else 0 for s in v]
        origin = [self.a.shifted_origin(MAP_O, (d, d), RESO) for d in dd]
        pos = np.array([[RESO * x - 2.0, RESO * y + 1.0, 1.0] for x, y in self.starts])
        goal = np.array([[RESO * x - 2.0, RESO * y + 1.0, 1.5 + 0.25 * (q % 3)] for q, (x, y) in enumerate(self.goals)])
        home = np.array([[-2.0 + 0.5 * q, 1.0] for q in range(self.nq)])
        args = ([RAW_SLOTS[s][3] if s in RAW_SLOTS else 1 for s in v], self.starts, RESO, origin, pos, goal, home, [q % 2 for q in range(self.nq)])
        oa = waypoints.tick_outputs_slots(self.a, *args, offsets=got[0], return_kept=True)
        ob = waypoints.tick_outputs_slots(self.b, *args, offsets=want[0], return_kept=True)
        assert len(oa) == len(ob) == 10
        for i, (x, y) in enumerate(zip(oa, ob)):
            assert flat(x) == flat(y), (tag, "tick output", i)
        flags = got[4]
        assert flags.dtype == np.int32 and flags.tolist() == want_flags.tolist(), (tag, flags.tolist(), want_flags.tolist())
        assert T["reused"] == int((flags > 0).sum()), (tag, T)
        assert (T["search_launches"] == 0) == bool((flags > 0).all()), (tag, T)
        # for every flag 2, no cell that differs lies in what the reference read for that query
        for q in np.nonzero(flags == 2)[0]:
            assert not (before[q] & self.changed[int(self.ids[q])]).any(), (tag, q)
        # the stored read sets: a reused query keeps its own, and every query with a path covers the reference's reads on
        # the grids as they are now
        read, tsh, have = self.a.debug_slot_read_sets()
        if self.stored is not None:
            for q in np.nonzero(flags > 0)[0]:
                assert read[q].tobytes() == self.stored[4][q].tobytes() and have[q] == self.stored[5][q], (tag, q)
        self.has_path = got[3] > 0
        reads = self.oracle_reads()
        for q, mask in reads.items():
            W, H = self.grids[int(self.ids[q])].shape
            assert have[q] and tsh[q] == rs.tile_shift(W, H), (tag, q, tsh[q])
            u = rs.uncovered(mask, read[q], W, H)
            assert len(u) == 0, (tag, q, "cells read outside the read set", u[:4].tolist(), "flag", int(flags[q]))
        assert not have[self.NOPATH] and not have[self.BAD], tag
        self.stored = (self.ids.copy(), self.starts.copy(), self.goals.copy(), got[3].copy(), read, have)
        self.written = set()
        for s in self.slots:
            self.changed[s][:] = False
            self.check_record(s)
        return flags, got

    # ---- changes of the maps
    def flip_prepared(self, s, x, y):
        """Flip the raw cell under prepared cell (x, y) of a raw-map slot, or the cell itself of slot 3."""
        if s == GRID_SLOT:
            self.grid3 = self.grid3.copy()
            self.grid3[x, y] ^= 1
        else:
            d, sh = self.geo[s]  # (gridprep places raw (rx, ry) at prepared (rx + d, ry + d); sh moves only start and goal)
            self.raw[s] = self.raw[s].copy()
            self.raw[s][x - d, y - d] ^= 1

    def far_cell(self, s, k=0):
        W, H = self.grids[s].shape
        return far_cell(W, H, self.geo[s][0] if s in self.geo else 0, k)


@pytest.fixture()
def fl(oracle):
    f = Fleet(oracle)
    yield f
    f.close()


def test_reads_stay_in_the_low_half(fl):
    """The bound the far-corner ticks rely on, asserted on the oracle's reads of this test's own inputs."""
    for q, mask in fl.oracle_reads().items():
        W, H = mask.shape
        xs, ys = np.nonzero(mask)
        assert xs.max() <= W // 2 and ys.max() <= H // 2, (q, int(xs.max()), int(ys.max()), W, H)


# ------------------------------------------------------------------ 1. changed tiles are exact
def test_changed_tiles_are_exact(fl):
    fl.tick("first")
    cases = []
    for s in fl.slots:
        W, H = fl.grids[s].shape
        cases += [(s, x, y) for x, y in flip_cases(W, H, fl.geo[s][0] if s in fl.geo else 0)]
    # slot 3, 27 cells a column: the copy's 7-byte tail is cells (36, 20 .. 26); the piece of bytes 16 .. 31 holds (0, 16 .. 26)
    # and (1, 0 .. 4), the piece of bytes 976 .. 991 holds (36, 4 .. 19)
    cases += [(GRID_SLOT, 36, 22), (GRID_SLOT, 1, 1), (GRID_SLOT, 0, 16), (GRID_SLOT, 36, 19)]
    for s, x, y in cases:
        fl.flip_prepared(s, x, y)
        kept = fl.refresh()
        assert kept == {t: t != s for t in fl.slots}, (s, x, y, kept)
        assert fl.changed[s][x, y] and 1 <= fl.changed[s].sum() <= (9 if s == 2 else 1), (s, x, y, int(fl.changed[s].sum()))
        for t in fl.slots:
            fl.check_record(t)
        fl.tick("after flip %d (%d, %d)" % (s, x, y))
    # two refreshes in a row accumulate
    for s in fl.slots:
        fl.flip_prepared(s, *fl.far_cell(s))
    fl.refresh()
    for s in fl.slots:
        fl.flip_prepared(s, *fl.far_cell(s, 1))
    fl.refresh()
    for s in fl.slots:
        assert fl.changed[s].sum() >= 2
        fl.check_record(s)
    fl.tick("after two refreshes")
    # every byte of a slot changes (the gather on slot 0, the copy on slot 3)
    fl.raw[0] = 1 - fl.raw[0]
    fl.grid3 = 1 - fl.grid3
    fl.refresh()
    for s in (0, GRID_SLOT):
        assert fl.changed[s].all()
        D = fl.check_record(s)
        W, H = fl.grids[s].shape
        assert int(D[0]) == (1 << W) - 1 and int(D[64]) == (1 << H) - 1
    fl.raw[0] = 1 - fl.raw[0]
    fl.grid3 = 1 - fl.grid3
    fl.refresh()
    fl.tick("after the inversions")


def test_world_refresh_marks_tiles_and_void_writes_void(fl):
    fl.tick("first")
    rng = np.random.default_rng(831)
    raw = (rng.random((130, 70)) < 0.2).astype(np.uint8)
    job = lambda r: (5, r, (0.0, 0.0), 1.0, (10.5, 9.5), (40.5, 20.5), 0, "ccst")
    assert not fl.both("refresh_slots_world", [job(raw)])[0][6]
    assert not fl.a.debug_slot_tiles(5)[2]  # (an empty slot: built, not compared)
    fl.tick("world slot filled")
    before = fl.a.get_grid_slot(5)
    new = raw.copy()
    new[127, 69] ^= 1
    new[64, 33] ^= 1
    new[0, 0] ^= 1
    assert not fl.both("refresh_slots_world", [job(new)])[0][6]
    diff = before != fl.a.get_grid_slot(5)
    assert diff.sum() == 3
    D, tsh, valid = fl.a.debug_slot_tiles(5)
    assert valid and tsh == 2 and D.tobytes() == words_of(rs.touched_tiles(np.argwhere(diff), 130, 70)).tobytes()
    # a kept refresh leaves the record as it is
    assert fl.both("refresh_slots_world", [job(new)])[0][6]
    assert fl.a.debug_slot_tiles(5)[0].tobytes() == D.tobytes() and fl.a.debug_slot_tiles(5)[2]
    # writes that void a record: prepare_slots, other extents, set_grid_slot
    fl.both("prepare_slots", [fl.job[0](fl.raw[0])])
    assert not fl.a.debug_slot_tiles(0)[2]
    fl.grid3 = np.zeros((29, 37), np.uint8)
    fl.both("refresh_grid_slots", [(GRID_SLOT, fl.grid3)])
    assert not fl.a.debug_slot_tiles(GRID_SLOT)[2]
    fl.both("set_grid_slot", 2, fl.grids[2])
    assert not fl.a.debug_slot_tiles(2)[2]
    assert fl.a.debug_slot_tiles(1)[2]
    # ... and a change of mode voids all of them and drops the stored results
    fl.a.set_slot_reuse("generation")
    assert not fl.a.debug_slot_tiles(1)[2]
    with pytest.raises(Exception):
        fl.a.debug_slot_read_sets()
    with pytest.raises(ValueError):
        fl.a.set_slot_reuse("both")
    from fuxi_planner_amd import _lib
    assert fl.a._L.fxjps_set_slot_reuse(fl.a._h, 2) == _lib.E_ARG


# ------------------------------------------------------------------ 2. the tracked search on slots
def tracked_search_main(oracle=None):
    """Mode 1's first replan_slots: the twin's bytes, the oracle's paths, read sets that cover the reference's reads with
    each query's own slot's extents (Fleet.tick), for both heuristics."""
    if oracle is None:
        from oracle import oracle
        oracle.build()
    direct = set()
    for h in (1, 2):
        f = Fleet(oracle, h)
        try:
            flags, got = f.tick("first h=%d" % h)
            assert not flags.any()
            lens, cost, cells = f.oracle_lens(f.mpl, with_cells=True)
            assert got[3].tolist() == lens.tolist() and got[2].tobytes() == cost.tobytes(), (h, got[3], lens)
            for q in range(f.nq):
                assert np.array_equal(got[1][got[0][q]:got[0][q + 1]], cells[q]), (h, q)
            assert (lens[f.LONG] == -1).all() and lens[f.NOPATH] == 0 and lens[f.BAD] == -2
            direct.add(f.a.timing()["table_direct"])
        finally:
            f.close()
    print("tracked ok direct=%s" % sorted(direct))
    return direct


def test_tracked_search_on_slots(oracle):
    assert tracked_search_main(oracle) == {1}


def test_tracked_search_on_slots_with_hashed_tables():
    env = dict(os.environ, FXJPS_DIRECT="0", PYTHONPATH=os.pathsep.join([ROOT, os.path.join(ROOT, "tests")]))
    r = subprocess.run([sys.executable, "-c", "import test_slot_tiles_gpu as t; t.tracked_search_main()"], env=env, cwd=ROOT, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0 and "tracked ok direct=[0]" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])


# ------------------------------------------------------------------ 3. the rule, tick by tick
def run_ticks(fl, tiles):
    """The ticks of test 3 on a fleet whose handle a is in mode 1 (tiles) or 0; -> the flags per tick."""
    seen = []
    flags, t1 = fl.tick("first")
    seen.append(flags)
    special = [fl.NOPATH, fl.BAD] + fl.LONG.tolist()
    paths = fl.has_path.copy()
    # an unchanged tick: every query reports 1
    assert set(fl.refresh().values()) == {True}
    flags, _ = fl.tick("unchanged")
    assert (flags == 1).all()
    seen.append(flags)
    # a flip in the far corner of every slot: every query with a path reports 2, the others 0
    for s in fl.slots:
        fl.flip_prepared(s, *fl.far_cell(s))
    assert set(fl.refresh().values()) == {False}
    flags, _ = fl.tick("far flips")
    seen.append(flags)
    if tiles:
        assert (flags[paths] == 2).all() and paths.sum() >= 3 * NQ_RAW and (flags[special] == 0).all(), flags.tolist()
        assert (flags[~paths] == 0).all()
    # a flip under an inner jump point of one vehicle's path (slot 0, tsh 0): that query is searched, its path changes
    off, cells = t1[0], t1[1]
    q = next(q for q in fl.of_slot(0) if paths[q] and off[q + 1] - off[q] >= 3)
    jx, jy = (int(v) for v in cells[off[q] + 1])
    old = cells[off[q]:off[q + 1]].copy()
    fl.flip_prepared(0, jx, jy)
    for s in fl.slots[1:]:  # (the other vehicles' maps change in their far corners once more)
        fl.flip_prepared(s, *fl.far_cell(s, 1))
    assert set(fl.refresh().values()) == {False}
    flags, t = fl.tick("flip on a path")
    seen.append(flags)
    assert flags[q] == 0 and t[1][t[0][q]:t[0][q + 1]].tobytes() != old.tobytes()
    if tiles:
        # the other vehicles report 2; on slot 0 itself a query reports 2 unless the jump point's box touches what its own
        # search read (the restated rule in Fleet.tick decided which)
        assert (flags[paths & (fl.ids != 0)] == 2).all(), flags.tolist()
    # a far flip, then a flip on a path: the reused queries' kept read sets still cover the reads on the new grid (Fleet.tick)
    fl.flip_prepared(0, *fl.far_cell(0, 1))
    fl.refresh()
    flags, t = fl.tick("far flip again")
    seen.append(flags)
    paths = fl.has_path.copy()
    q2 = next(k for k in fl.of_slot(0) if paths[k] and t[0][k + 1] - t[0][k] >= 3 and k != q)
    jx, jy = (int(v) for v in t[1][t[0][q2] + 1])
    fl.flip_prepared(0, jx, jy)
    fl.refresh()
    flags, _ = fl.tick("then a flip on another path")
    seen.append(flags)
    assert flags[q2] == 0
    # a flip of a free cell next to a cell the reference read, not read itself, whose neighbour's tile the search marked
    reads = Fleet.oracle_reads(fl)
    read, _, have = fl.a.debug_slot_read_sets() if tiles else (None, None, None)
    grid = fl.grids[0]
    W, H = grid.shape
    found = None
    for k in fl.of_slot(0):
        if not fl.has_path[k] or found:
            continue
        M = rs.marked_tiles(read[k]) if tiles else reads[k]
        for x, y in np.argwhere((grid == 0) & ~reads[k]):
            x0, x1, y0, y1 = max(x - 1, 0), min(x + 1, W - 1), max(y - 1, 0), min(y + 1, H - 1)
            near = reads[k][x0:x1 + 1, y0:y1 + 1] & M[x0:x1 + 1, y0:y1 + 1]
            if near.any() and not M[x, y] and (x, y) not in [tuple(c) for c in fl.starts] + [tuple(c) for c in fl.goals]:
                found = (k, int(x), int(y))
                break
    assert found, "no free unread cell beside a read one"
    k, x, y = found
    fl.flip_prepared(0, x, y)
    fl.refresh()
    flags, _ = fl.tick("flip beside a read cell")
    seen.append(flags)
    assert flags[k] == 0
    # a moved start: that query reports 0
    k = int(fl.of_slot(1)[1])
    fl.starts = fl.starts.copy()
    fl.starts[k] = fl.starts[int(fl.of_slot(1)[2])]
    flags, _ = fl.tick("a moved start")
    seen.append(flags)
    assert flags[k] == 0 and (np.delete(flags, k) == 1).all()
    return seen


def test_the_rule_tick_by_tick(fl):
    seen = run_ticks(fl, True)
    assert any((f == 2).any() for f in seen)


# ------------------------------------------------------------------ 4. mode 0 on the same ticks
def test_mode_0_gives_todays_flags(fl):
    fl.a.set_slot_reuse("generation")
    fl.check_record = lambda s, valid=True: None  # (no record is kept in mode 0 ...)
    fl.a.debug_slot_read_sets = lambda: (np.zeros((fl.nq, 128), np.uint64), np.array([rs.tile_shift(*fl.grids[int(s)].shape) for s in fl.ids]),
                                         np.zeros(fl.nq, bool))
    # (... and no read set: the cover checks of Fleet.tick are mode 1's)
    real_reads = fl.oracle_reads
    fl.oracle_reads = lambda qs=None: {}
    seen = run_ticks(fl, False)
    assert all(set(f.tolist()) <= {0, 1} for f in seen)
    for s in fl.slots:
        assert not fl.a.debug_slot_tiles(s)[2]
    # a switch of mode drops the stored results: nothing is reused on the next call, everything on the one after
    fl.oracle_reads = real_reads
    del fl.check_record, fl.a.debug_slot_read_sets
    fl.a.set_slot_reuse("tiles")
    fl.stored = None
    flags, _ = fl.tick("after the switch")
    assert (flags == 0).all()
    flags, _ = fl.tick("again")
    assert (flags == 1).all()


def test_fleet_tick_refresh_reports_reused_tiles(fl):
    jobs = [fl.job[s](fl.raw[s]) for s in sorted(RAW_SLOTS)]
    n = len(jobs)
    pos = np.array([[RESO * j[2][0] - 2.0, RESO * j[2][1] + 1.0, 1.0] for j in jobs])
    goals = np.array([[RESO * j[3][0] - 2.0, RESO * j[3][1] + 1.0, 1.5] for j in jobs])
    home = np.array([[-2.0 + 0.5 * v, 1.0] for v in range(n)])
    from test_refresh_slots_gpu import same_value
    for t in range(3):
        if t == 2:
            for s in sorted(RAW_SLOTS):
                fl.flip_prepared(s, *fl.far_cell(s))
            jobs = [fl.job[s](fl.raw[s]) for s in sorted(RAW_SLOTS)]
        recs = fl.a.fleet_tick_refresh(jobs, pos, goals, home, RESO, MAP_O, reuse=True)
        want = fl.b.fleet_tick_refresh(jobs, pos, goals, home, RESO, MAP_O)
        for v in range(n):
            assert set(recs[v]) - {"reused", "reused_tiles"} == set(want[v]) and recs[v]["ok"] and recs[v]["status"] > 0, (t, v)
            for k in want[v]:
                assert same_value(recs[v][k], want[v][k]), (t, v, k)
        assert [r["reused"] for r in recs] == [t > 0] * n and [r["reused_tiles"] for r in recs] == [t == 2] * n, (t, recs)
        assert [r["kept"] for r in recs] == [t < 2] * n  # (the fixture filled the slots from these raws)


def test_two_contexts_accept_the_mode_and_plan_plainly(fl):
    """A handle with two contexts on device 0: mode 1 is accepted, its refresh calls run the tile forms on both contexts, and
    replan_slots stays the plain batch it is there (nothing is reused)."""
    import fuxi_planner_amd as fx
    p2 = fx.Planner([0, 0])
    try:
        p2.set_slot_reuse("tiles")
        jobs = [fl.job[s](fl.raw[s]) for s in sorted(RAW_SLOTS)]
        for t in range(3):  # the first fill, the same maps again, then a far flip on slot 1 and on slot 3
            if t == 2:
                fl.flip_prepared(1, *fl.far_cell(1))
                fl.flip_prepared(GRID_SLOT, *fl.far_cell(GRID_SLOT))
                jobs = [fl.job[s](fl.raw[s]) for s in sorted(RAW_SLOTS)]
                fl.refresh()
            assert [o[6] for o in p2.refresh_slots(jobs)] == [t > 0, t == 1, t > 0]
            assert p2.refresh_grid_slots([(GRID_SLOT, fl.grid3)]) == [t == 1]
            for c in (0, 1):
                for s in fl.slots:
                    occ, maps = p2.debug_slot_context(c, s)
                    assert occ.tobytes() == fl.grids[s].tobytes(), (t, c, s)
                    for k, m in fl.b.debug_slot_maps(s).items():
                        assert maps[k].tobytes() == m.tobytes(), (t, c, s, k)
            got = p2.replan_slots(fl.ids, fl.starts, fl.goals, 2, fl.mpl)
            want = fl.b.plan_batch_slots(fl.ids, fl.starts, fl.goals, 2, fl.mpl)
            assert not got[4].any() and p2.timing()["reused"] == 0, t
            for k in range(4):
                assert got[k].tobytes() == want[k].tobytes(), (t, k)
    finally:
        p2.close()


def test_cropped_refresh_marks_tiles_and_an_emptied_slot_voids(fl):
    """refresh_slots_cropped is refresh_slots_world behind the crop: a compared job's record is exact there too, and a job that
    leaves its slot empty (a message of zeros: the node does not plan on this tick) voids the record."""
    from fuxi_planner_amd import _lib
    rng = np.random.default_rng(832)
    msg = np.zeros((80, 60), np.uint8)
    msg[10:50, 8:40] = rng.random((40, 32)) < 0.2
    msg[10, 8] = msg[49, 39] = 1  # (the box of the non-zero cells stays what it is under the flips below)
    msg[12, 10] = msg[40, 30] = 0
    job = lambda m: (6, m, (0.0, 0.0), 1.0, (12.5, 10.5), (40.5, 30.5), 0, "ccst")
    o = fl.a.refresh_slots_cropped([job(msg)])[0]
    assert o[5] and not o[6] and o[-2] == 0, o
    got = fl.a.replan_slots([6], [o[0]], [o[1]], 2, 128)
    assert got[3][0] > 0 and got[4][0] == 0
    before = fl.a.get_grid_slot(6)
    new = msg.copy()
    new[45, 35] ^= 1
    new[20, 9] ^= 1
    o = fl.a.refresh_slots_cropped([job(new)])[0]
    assert o[5] and not o[6], o
    diff = before != fl.a.get_grid_slot(6)
    W, H = before.shape
    D, tsh, valid = fl.a.debug_slot_tiles(6)
    assert diff.sum() == 2 and valid and tsh == rs.tile_shift(W, H)
    assert D.tobytes() == words_of(rs.touched_tiles(np.argwhere(diff), W, H)).tobytes()
    o = fl.a.refresh_slots_cropped([job(np.zeros((80, 60), np.uint8))])[0]
    assert not o[5] and o[-2] == _lib.JOB_NOT_PLANNED, o
    assert not fl.a.debug_slot_tiles(6)[2]
