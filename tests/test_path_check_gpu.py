"""GPU suite (-m gpu): fxjps_check_paths_slots / k_check_paths_slots -- a fleet's kept paths against
their slots' grids in one launch.  The yardstick is the host form, waypoints.check_path, on the bytes get_grid_slot returns
(itself pinned to the reference's blocked() by tests/test_path_check_host.py), and the golden records made with the
reference's blocked().

Four slots in one call: 3 x 40, 96 x 80, 130 x 600 (walls across the whole width with a one-cell gap at alternating ends:
its long paths have hundreds of segments and thousands of unit steps, and pass x = 0 and x = W - 1) and the 193 x 193 rooms
map; about 300 paths from plan_batch_slots.  (The refusal of a rank handle with world > 1 needs two devices and is not
exercised here; it is the same first line as in the other slot calls.)"""
import ctypes as C

import numpy as np
import pytest

from conftest import grid_from_bits, load_golden, pairs
from test_search_work_gpu import rooms_map

pytestmark = pytest.mark.gpu
VALID, EMPTY, BLOCKED, OUTSIDE, MALFORMED = 1, 0, 2, 3, -1
SLOTS = (3, 17, 100, 255)  # the slots of the four grids


def serpentine(W=130, H=600):
    occ = np.zeros((W, H), dtype=np.uint8)
    for k, y in enumerate(range(5, H - 3, 6)):
        occ[:, y] = 1
        occ[0 if k % 2 == 0 else W - 1, y] = 0
    return occ


def make_grids():
    rng = np.random.default_rng(8401)
    thin = (rng.random((3, 40)) < 0.08).astype(np.uint8)
    mid = (rng.random((96, 80)) < 0.2).astype(np.uint8)
    return [thin, mid, serpentine(), rooms_map()]


def make_queries(grids):
    """-> (grid index, start, goal) per query: random free cells, and on the 130 x 600 grid also the whole way up."""
    rng = np.random.default_rng(8402)
    gi, s, g = [], [], []
    for k, (occ, n) in enumerate(zip(grids, (24, 120, 36, 120))):
        free = np.argwhere(occ == 0)
        for _ in range(n):
            a, b = free[rng.choice(len(free), 2, replace=False)]
            gi.append(k)
            s.append(a)
            g.append(b)
    for a, b in (((50, 50), (104, 104)), ((104, 105), (1, 1))):  # into and out of the rooms map's sealed pocket: no path
        gi.append(3)
        s.append(a)
        g.append(b)
    for a, b in (((60, 2), (60, 597)), ((0, 0), (129, 599)), ((129, 300), (3, 0))):
        gi.append(2)
        s.append(a)
        g.append(b)
    return np.array(gi), np.array(s, dtype=np.int32), np.array(g, dtype=np.int32)


def unit_steps(p):
    """The unit steps of a well-formed jump-point path: int64 [m, 5] rows (segment, cx, cy, ux, uy)."""
    out = []
    for i in range(len(p) - 1):
        d = p[i + 1].astype(np.int64) - p[i]
        m = int(np.abs(d).max())
        u = np.sign(d)
        k = np.arange(m)[:, None]
        out.append(np.c_[np.full(m, i), p[i] + u * k, np.tile(u, (m, 1))])
    return np.concatenate(out) if out else np.zeros((0, 5), dtype=np.int64)


def path_of(off, cells, q):
    return cells[int(off[q]):int(off[q + 1])]


def assert_features(grids, gi, off, cells):
    """What the planner's paths must contain for the checks below to mean something."""
    nseg = np.diff(off) - 1
    steps = [unit_steps(path_of(off, cells, q)) for q in range(len(gi))]
    assert len(gi) >= 300 and (np.diff(off) > 0).sum() >= 250
    assert sum(len(s) > 64 for s in steps) >= 20, "paths with more than 64 unit steps"
    assert (nseg > 64).any(), "a path with more than 64 segments"
    seg_len = np.concatenate([np.bincount(s[:, 0]) for s in steps if len(s)])
    assert (seg_len == 1).sum() >= 20, "segments of length 1"
    at0 = [q for q in range(len(gi)) if len(steps[q]) and (path_of(off, cells, q)[:, 0] == 0).any()]
    atW = [q for q in range(len(gi)) if len(steps[q]) and (path_of(off, cells, q)[:, 0] == grids[gi[q]].shape[0] - 1).any()]
    assert at0 and atW, "cells at x = 0 and x = W - 1"
    return steps


def mutate(grids, gi, off, cells, steps):
    """-> (new grids, new cells, shifts): obstacles put on and beside steps of some paths, shifts (small ones, and ones
    that push a path over an edge), malformed segments spliced in."""
    rng = np.random.default_rng(8403)
    new = [g.copy() for g in grids]
    cells = cells.copy()
    nq = len(gi)
    shift = np.zeros((nq, 2), dtype=np.int32)
    have = [q for q in range(nq) if len(steps[q])]
    kind = rng.choice(["block", "squeeze", "small", "edge", "edge0", "knight", "repeat", "mid", "none"], nq,
                      p=[0.1, 0.05, 0.1, 0.15, 0.15, 0.05, 0.03, 0.06, 0.31])
    kind[nq - 3:] = "none"
    for q in have:
        p = path_of(off, cells, q)  # (a view: the splices below write the copy)
        st, g = steps[q], new[gi[q]]
        W, H = g.shape
        if kind[q] == "block":
            _, cx, cy, ux, uy = st[int(rng.integers(len(st)))]
            g[cx + ux, cy + uy] = 1
        elif kind[q] == "squeeze":
            diag = st[(st[:, 3] != 0) & (st[:, 4] != 0)]
            if len(diag):
                _, cx, cy, ux, uy = diag[int(rng.integers(len(diag)))]
                g[cx + ux, cy] = g[cx, cy + uy] = 1
        elif kind[q] == "small":
            shift[q] = rng.integers(-2, 3, 2)
        elif kind[q] == "edge":
            over = int(rng.integers(1, 3))
            shift[q] = [(-(p[:, 0].min() + over), 0), (W - 1 - p[:, 0].max() + over, 0), (0, -(p[:, 1].min() + over)),
                        (0, H - 1 - p[:, 1].max() + over)][int(rng.integers(4))]
        elif kind[q] == "edge0":  # the first cell itself
            shift[q] = [(-(p[0, 0] + 1), 0), (W - p[0, 0], 1), (-1, -(p[0, 1] + 2)), (0, H - p[0, 1])][int(rng.integers(4))]
        elif kind[q] == "knight":
            p[1] = p[0] + (2, 1)  # the first segment: nothing can fail in front of it
        elif kind[q] == "repeat":
            p[1] = p[0]
        elif kind[q] == "mid" and len(p) >= 4:
            k = int(rng.integers(1, len(p) - 1))
            p[k] = p[k] + (1, 2) if k % 2 else p[k - 1]
    # the long way up the 130 x 600 grid (the third query from the end): its very last step
    _, cx, cy, ux, uy = steps[nq - 3][-1]
    new[gi[nq - 3]][cx + ux, cy + uy] = 1
    return new, cells, shift


def host_form(grids_now, gi, off, cells, shift):
    from fuxi_planner_amd import waypoints
    v, s, c = [], [], []
    for q in range(len(gi)):
        a, b, xy = waypoints.check_path(path_of(off, cells, q), grids_now[gi[q]], None if shift is None else shift[q])
        v.append(a)
        s.append(b)
        c.append(xy)
    return np.array(v, dtype=np.int32), np.array(s, dtype=np.int32), np.array(c, dtype=np.int32).reshape(-1, 2)


def same(got, want):
    return all(a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes() for a, b in zip(got, want))


class Fleet(object):
    pass


@pytest.fixture(scope="module")
def planner():
    import fuxi_planner_amd as fx
    p = fx.Planner([0])
    yield p
    p.close()


@pytest.fixture(scope="module")
def fleet(planner):
    """The four slots and the planner's paths on them, planned once for the module."""
    f = Fleet()
    f.grids = make_grids()
    f.gi, f.starts, f.goals = make_queries(f.grids)
    f.ids = np.array([SLOTS[k] for k in f.gi], dtype=np.int32)
    planner.set_grid_slots(list(zip(SLOTS, f.grids)))
    f.off, f.cells, f.cost, f.status = planner.replan_slots(f.ids, f.starts, f.goals, 2)[:4]
    f.steps = assert_features(f.grids, f.gi, f.off, f.cells)
    return f


def test_planner_paths_are_valid_on_their_own_slots(planner, fleet):
    f = fleet
    got = planner.check_paths_slots(f.ids, f.off, f.cells)
    have = np.diff(f.off) > 0
    assert got[0].tolist() == np.where(have, VALID, EMPTY).tolist() and (~have).sum() >= 1
    assert (got[1] == -1).all() and (got[2] == -1).all()
    assert same(got, host_form(f.grids, f.gi, f.off, f.cells, None))
    assert same(got, planner.check_paths_slots(f.ids, f.off, f.cells, np.zeros((len(f.ids), 2), np.int32)))


def test_changed_slots_shifts_and_malformed_paths(planner, fleet):
    """The device against the host form, byte for byte, after the slots changed; nothing of the handle changes."""
    f = fleet
    new, cells, shift = mutate(f.grids, f.gi, f.off, f.cells, f.steps)
    kept = planner.refresh_grid_slots(list(zip(SLOTS, new)))
    assert kept == [np.array_equal(a, b) for a, b in zip(new, f.grids)] and not all(kept)
    want = host_form(new, f.gi, f.off, cells, shift)
    n = {v: int((want[0] == v).sum()) for v in (VALID, EMPTY, BLOCKED, OUTSIDE, MALFORMED)}
    print("verdicts", n)
    assert n[BLOCKED] >= 30 and n[OUTSIDE] >= 30 and n[MALFORMED] >= 10 and n[VALID] >= 30, n
    late = want[1][(want[0] == BLOCKED) | (want[0] == OUTSIDE)]
    assert (late >= 64).any() and (late == 0).any(), "failures in the first and in a later chunk of segments"
    before = planner.replan_slots(f.ids, f.starts, f.goals, 2)
    got = planner.check_paths_slots(f.ids, f.off, cells, shift)
    for name, a, b in zip(("verdict", "seg", "cell"), got, want):
        bad = np.flatnonzero((a != b).reshape(len(f.ids), -1).any(axis=1))
        assert len(bad) == 0, (name, bad[:5], a[bad[:5]], b[bad[:5]])
    assert same(got, want)
    # a second identical call: the same bytes; the slots' bytes and generations are what they were
    assert same(planner.check_paths_slots(f.ids, f.off, cells, shift), got)
    for s, g in zip(SLOTS, new):
        assert planner.get_grid_slot(s).tobytes() == g.tobytes()
    again = planner.replan_slots(f.ids, f.starts, f.goals, 2)
    assert again[4].all() and all(a.tobytes() == b.tobytes() for a, b in zip(again[:4], before[:4]))


def long_cases():
    """200 unit steps in one segment and in 100 segments of two; the failure at the last step, at step 64 exactly (the
    first lane of the second group of steps), at step 63, and nowhere."""
    straight = np.array([(3, 0), (3, 200)], dtype=np.int32)
    zigzag = np.array([(2 + 2 * (i % 2), 2 * i) for i in range(101)], dtype=np.int32)
    cases = []
    for path in (straight, zigzag):
        st = unit_steps(path)
        assert len(st) == 200
        for at in (199, 64, 63, None):
            g = np.zeros((8, 210), dtype=np.uint8)
            want = (VALID, -1, (-1, -1))
            if at is not None:
                seg, cx, cy, ux, uy = (int(v) for v in st[at])
                g[cx + ux, cy + uy] = 1
                want = (BLOCKED, seg, (cx + ux, cy + uy))
            cases.append((path, g, want))
    # ... and the squeeze at the last step of the zigzag, an edge one step behind its end
    st = unit_steps(zigzag)
    seg, cx, cy, ux, uy = (int(v) for v in st[199])
    g = np.zeros((8, 210), dtype=np.uint8)
    g[cx + ux, cy] = g[cx, cy + uy] = 1
    cases.append((zigzag, g, (BLOCKED, seg, (cx + ux, cy + uy))))
    cases.append((zigzag, np.zeros((8, 200), dtype=np.uint8), (OUTSIDE, 99, (2, 200))))
    return cases


def test_failure_at_the_last_step_and_at_step_64(planner):
    from fuxi_planner_amd import waypoints
    cases = long_cases()
    slots = [30 + k for k in range(len(cases))]
    planner.set_grid_slots([(s, g) for s, (_, g, _) in zip(slots, cases)])
    off = np.concatenate([[0], np.cumsum([len(p) for p, _, _ in cases])])
    got = planner.check_paths_slots(slots, off, np.concatenate([p for p, _, _ in cases]))
    for k, (p, g, want) in enumerate(cases):
        assert waypoints.check_path(p, g) == want, k
        assert (int(got[0][k]), int(got[1][k]), tuple(int(v) for v in got[2][k])) == want, k
    for s in slots:
        planner.clear_grid_slot(s)


def test_golden_records(planner):
    """One slot per golden grid, in batches of at most 256 slots, on a handle of its own."""
    import fuxi_planner_amd as fx
    from fuxi_planner_amd import _lib
    recs = load_golden("path_check.json")
    with fx.Planner([0]) as p:
        for b0 in range(0, len(recs), _lib.MAX_GRID_SLOTS):
            batch = recs[b0:b0 + _lib.MAX_GRID_SLOTS]
            p.set_grid_slots([(k, grid_from_bits(r["grid_bits"], r["shape"])) for k, r in enumerate(batch)])
            paths = [np.array(pairs(r["path"]), dtype=np.int32).reshape(-1, 2) for r in batch]
            off = np.concatenate([[0], np.cumsum([len(c) for c in paths])])
            v, s, c = p.check_paths_slots(np.arange(len(batch)), off, np.concatenate(paths), np.array([r["shift"] for r in batch], dtype=np.int32))
            for k, r in enumerate(batch):
                assert (int(v[k]), int(s[k]), c[k].tolist()) == (r["verdict"], r["seg"], r["cell"]), (b0 + k, r["kind"])


def test_refusals_queue_nothing(planner, fleet):
    from fuxi_planner_amd import _lib
    f = fleet
    L, h = planner._L, planner._h
    nq = 6
    ids = np.ascontiguousarray(f.ids[:nq])
    off = np.ascontiguousarray(f.off[:nq + 1], dtype=np.int64)
    cells = np.ascontiguousarray(f.cells[:int(off[-1])])
    shift = np.zeros((nq, 2), dtype=np.int32)
    out = [np.full(nq, 77, dtype=np.int32), np.full(nq, 77, dtype=np.int32), np.full((nq, 2), 77, dtype=np.int32)]

    def call(n=nq, o=off, c=cells, i=ids, s=shift, outs=(0, 1, 2)):
        ptr = lambda a, t: None if a is None else _lib.ptr(a, t)
        o3 = [out[k] if k in outs else None for k in range(3)]
        rc = L.fxjps_check_paths_slots(h, n, ptr(o, C.c_int64), ptr(c, C.c_int32), ptr(i, C.c_int32), ptr(s, C.c_int32),
                                       ptr(o3[0], C.c_int32), ptr(o3[1], C.c_int32), ptr(o3[2], C.c_int32))
        return rc, L.fxjps_last_error(h).decode()

    def ids_with(q, v):
        a = ids.copy()
        a[q] = v
        return a

    descend = off.copy()
    descend[4] = descend[3] - 1
    first = off.copy()
    first[0] = 1
    refused = [(dict(i=ids_with(2, 256)), "query 2"), (dict(i=ids_with(5, -1)), "query 5"), (dict(i=ids_with(1, 200)), "query 1"),
               (dict(i=ids_with(4, 200), o=descend), "query 3"), (dict(o=descend), "query 3"), (dict(o=first), "query 0"),
               (dict(o=None, c=None), "resident"), (dict(o=None), "query 0"), (dict(c=None), "query 0"), (dict(i=None), "query 0"),
               (dict(outs=(1, 2)), "query 0"), (dict(outs=(0, 2)), "query 0"), (dict(outs=(0, 1)), "query 0"), (dict(n=-1), "query 0")]
    for kw, text in refused:
        rc, msg = call(**kw)
        assert rc == _lib.E_ARG and text in msg, (kw.keys(), rc, msg)
        assert all((a == 77).all() for a in out), kw.keys()
    assert L.fxjps_check_paths_slots(None, nq, None, None, None, None, None, None, None) == _lib.E_ARG
    # nq == 0 is no error, whatever else is passed; shift_xy may be NULL
    assert call(n=0)[0] == 0 and call(n=0, o=None, c=None, i=None, outs=())[0] == 0 and all((a == 77).all() for a in out)
    rc, msg = call(s=None)
    assert rc == 0 and (out[0] != 77).all(), msg
    want = planner.check_paths_slots(ids, off, cells)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(out, want))
    with pytest.raises(ValueError):
        planner.check_paths_slots(ids, off[:-1], cells)
    with pytest.raises(ValueError):
        planner.check_paths_slots(ids, off, cells[:-1])
