"""GPU suite (-m gpu): fxjps_set_grid_slots / fxjps_refresh_grid_slots -- fxjps_set_grid_slot for many slots in one call, and
its form for the tick after that keeps the maps and the generation of every slot whose bytes did not change.  The yardstick
is a twin handle that gets the same grids through fxjps_set_grid_slot one by one: after every step every slot's bytes and
all six derived arrays are compared for equality between the two handles, on the first step also with the host reference
of oracle/derived_maps.py.  What only the refresh call has -- which jobs report `kept` -- is stated tick by tick, and what
the generations are worth is shown by fxjps_replan_slots behind both calls against the twin's fxjps_plan_batch_slots_csr.

The copy kernel moves 16 bytes per lane and 256 lanes per block, so the fleet has cell counts one short of, at and one past
16 (3 x 5, 4 x 4, 1 x 17) and 4096 (63 x 65, 64 x 64, 1 x 4097), a single cell, 5 x 7, 33 x 64, 64 x 65 (a second block of
four whole lanes), 100 x 37 (3700 cells: the last lane moves 4 bytes one by one) and one 513 x 513 (more than 2^18 cells:
always built).  Obstacle bytes are 1, 7, 100 and 255."""
import ctypes as C

import numpy as np
import pytest

from test_derived_maps_gpu import check_maps

pytestmark = pytest.mark.gpu
SHAPES = [(1, 1), (3, 5), (4, 4), (1, 17), (63, 65), (64, 64), (1, 4097), (5, 7), (33, 64), (64, 65), (100, 37), (513, 513)]
FIRST, BLOCK2, TAIL, LARGE = 8, 9, 10, 11  # jobs: 33 x 64 (first byte flipped), 64 x 65 and 100 x 37 (last byte flipped), 513 x 513
VALUES = np.array([1, 7, 100, 255], np.uint8)


@pytest.fixture(scope="module")
def planner():
    import fuxi_planner_amd as fx
    p = fx.Planner([0])
    yield p
    p.close()


@pytest.fixture(scope="module")
def twin():
    import fuxi_planner_amd as fx
    p = fx.Planner([0])
    yield p
    p.close()


def grid(rng, W, H, density=0.15):
    """Random obstacles of the four byte values; the first and the last three cells of the byte stream are free, so a flip
    there changes exactly that byte."""
    g = np.where(rng.random((W, H)) < density, VALUES[rng.integers(0, 4, (W, H))], 0).astype(np.uint8)
    flat = g.reshape(-1)
    flat[:3] = 0
    flat[-3:] = 0
    return g


def fleet(first_slot=0, seed=820):
    rng = np.random.default_rng(seed)
    return [(first_slot + v, grid(rng, W, H, 0.05 if W * H > 1 << 16 else 0.15)) for v, (W, H) in enumerate(SHAPES)]


def c_jobs(jobs):
    """-> the fxjps_grid_job_t array of [(slot, uint8 [W][H])], and the arrays it points into."""
    from fuxi_planner_amd import _lib
    arr = (_lib.GridJob * max(len(jobs), 1))()
    keep = []
    for j, (slot, g) in zip(arr, jobs):
        g = np.ascontiguousarray(g, dtype=np.uint8)
        keep.append(g)
        j.occ, j.slot, j.W, j.H = _lib.ptr(g, C.c_uint8), int(slot), g.shape[0], g.shape[1]
    return arr, keep


def set_many(p, jobs):
    arr, keep = c_jobs(jobs)
    p._chk(p._L.fxjps_set_grid_slots(p._h, arr, len(jobs)))


def refresh_many(p, jobs):
    from fuxi_planner_amd import _lib
    arr, keep = c_jobs(jobs)
    kept = np.full(max(len(jobs), 1), -5, np.int32)
    p._chk(p._L.fxjps_refresh_grid_slots(p._h, arr, len(jobs), _lib.ptr(kept, C.c_int32)))
    assert set(kept[:len(jobs)].tolist()) <= {0, 1}, kept
    return [bool(k) for k in kept[:len(jobs)]]


def set_one(p, slot, g):
    """fxjps_set_grid_slot through the C call: the bytes as they are (Planner.set_grid_slot writes 0 / 1)."""
    from fuxi_planner_amd import _lib
    g = np.ascontiguousarray(g, dtype=np.uint8)
    p._chk(p._L.fxjps_set_grid_slot(p._h, int(slot), _lib.ptr(g, C.c_uint8), g.shape[0], g.shape[1]))


def same_slots(p, other, jobs, tag):
    for s, g in jobs:
        got = p.get_grid_slot(s)
        assert got.shape == g.shape and got.tobytes() == g.tobytes(), (tag, s, "the bytes handed in")
        assert got.tobytes() == other.get_grid_slot(s).tobytes(), (tag, s)
        a, b = p.debug_slot_maps(s), other.debug_slot_maps(s)
        assert set(a) == set(b) and len(b) == 6, sorted(b)
        for name in b:
            assert a[name].tobytes() == b[name].tobytes(), (tag, s, name)


def tick(p, other, jobs, kept, tag, changed=()):
    """One refresh_grid_slots on p; the twin gets the grids of `changed` (indices into jobs) one by one."""
    got = refresh_many(p, jobs)
    for v in changed:
        set_one(other, *jobs[v])
    assert got == list(kept), (tag, got)
    same_slots(p, other, jobs, tag)


def with_byte(job, index, value):
    g = job[1].copy()
    g.reshape(-1)[index] = value
    return (job[0], g)


def test_ticks(planner, twin):
    jobs = fleet()
    n = len(jobs)
    everything = range(n)
    assert sorted({int(v) for _, g in jobs for v in np.unique(g)}) == [0, 1, 7, 100, 255]
    # 1. one call into empty slots against n calls on the twin; also against the host's own derived maps
    set_many(planner, jobs)
    for job in jobs:
        set_one(twin, *job)
    same_slots(planner, twin, jobs, "set")
    for s, g in jobs:
        check_maps(planner.debug_slot_maps(s), (g != 0).astype(np.uint8), ("set", s))
    but_large = [v != LARGE for v in everything]
    # 2. the same grids again: all kept but the large one
    tick(planner, twin, jobs, but_large, "tick 2")
    # 3. the first byte of one grid, the last byte of two others: the last lane of a partly filled second block (four
    # lanes of 256) decides for 64 x 65, the lane that moves its bytes one by one for 100 x 37
    assert jobs[BLOCK2][1].size == 4096 + 64 and jobs[TAIL][1].size % 16 == 4
    jobs[FIRST] = with_byte(jobs[FIRST], 0, 255)
    jobs[BLOCK2] = with_byte(jobs[BLOCK2], -1, 1)
    jobs[TAIL] = with_byte(jobs[TAIL], -1, 7)
    flipped = (FIRST, BLOCK2, TAIL)
    tick(planner, twin, jobs, [v not in flipped + (LARGE,) for v in everything], "tick 3", changed=flipped)
    for v in flipped:
        check_maps(planner.debug_slot_maps(jobs[v][0]), (jobs[v][1] != 0).astype(np.uint8), ("tick 3", v))
    # 4. tick 3's grids again: the word of the call before is not seen
    tick(planner, twin, jobs, but_large, "tick 4")
    # 5. a 1 turned into a 7: the same obstacles, another byte -- built
    v, at = next((v, int(np.flatnonzero(g.reshape(-1) == 1)[0])) for v, (_, g) in enumerate(jobs) if v != LARGE and (g == 1).any())
    jobs[v] = with_byte(jobs[v], at, 7)
    tick(planner, twin, jobs, [u not in (v, LARGE) for u in everything], "tick 5", changed=(v,))
    # 6. equal bytes under swapped extents: built
    jobs[FIRST] = (jobs[FIRST][0], np.ascontiguousarray(jobs[FIRST][1].reshape(64, 33)))
    tick(planner, twin, jobs, [u not in (FIRST, LARGE) for u in everything], "tick 6", changed=(FIRST,))
    tick(planner, twin, jobs, but_large, "tick 6 again")
    # 7. a cleared slot: built
    planner.clear_grid_slot(jobs[2][0])
    tick(planner, twin, jobs, [u not in (2, LARGE) for u in everything], "tick 7")
    # 8. set_grid_slots over everything builds everything, whatever the slots hold: the next refresh keeps all
    set_many(planner, jobs)
    same_slots(planner, twin, jobs, "set again")
    tick(planner, twin, jobs, but_large, "tick 8")
    # n = 1
    one = [(jobs[TAIL][0], with_byte(jobs[TAIL], 5, 100)[1])]
    set_many(planner, one)
    set_one(twin, *one[0])
    same_slots(planner, twin, one, "n = 1")
    assert refresh_many(planner, one) == [True]
    same_slots(planner, twin, one, "n = 1, kept")


def test_a_slot_last_written_by_prepare_slots(planner, twin):
    rng = np.random.default_rng(821)
    raw = (rng.random((50, 45)) < 0.04).astype(np.uint8)
    job = (30, raw, (2, 2), (40, 40), 1, 1)
    assert planner.prepare_slots([job]) == twin.prepare_slots([job])
    held = planner.get_grid_slot(30)
    assert held.max() == 1 and held.shape != raw.shape
    tick(planner, twin, [(30, held)], [True], "prepared bytes")
    other = held.copy()
    other[7, 9] ^= 1
    tick(planner, twin, [(30, other)], [False], "one byte off", changed=(0,))
    check_maps(planner.debug_slot_maps(30), other, "one byte off")
    # ... and the other way round: refresh_slots compares with what refresh_grid_slots left
    tick(planner, twin, [(30, held)], [False], "back", changed=(0,))
    assert planner.refresh_slots([job])[0][6] is True


def test_256_jobs_in_one_call():
    import fuxi_planner_amd as fx
    rng = np.random.default_rng(822)
    jobs = [(s, grid(rng, int(rng.integers(1, 7)), int(rng.integers(1, 7)), 0.3)) for s in rng.permutation(256)]
    with fx.Planner([0]) as p, fx.Planner([0]) as other:
        set_many(p, jobs)
        for job in jobs:
            set_one(other, *job)
        same_slots(p, other, jobs, "256 jobs")
        jobs[100] = with_byte(jobs[100], 0, 100)
        tick(p, other, jobs, [v != 100 for v in range(256)], "256 jobs, one changed", changed=(100,))
        tick(p, other, jobs, [True] * 256, "256 jobs, kept")


# ------------------------------------------------------------------ planning behind the calls
def planning_fleet(seed=823):
    """Five grids with the obstacle bytes 1 and 7 and free corners, and one query each, corner to corner."""
    rng = np.random.default_rng(seed)
    jobs = []
    for v, (W, H) in enumerate([(12, 9), (21, 17), (33, 20), (40, 37), (64, 65)]):
        g = np.where(rng.random((W, H)) < 0.08, VALUES[rng.integers(0, 2, (W, H))], 0).astype(np.uint8)
        g[:3, :3] = 0
        g[-3:, -3:] = 0
        jobs.append((40 + v, g))
    ids = np.array([s for s, _ in jobs], np.int32)
    starts = np.array([(0, 0)] * len(jobs), np.int32)
    goals = np.array([(g.shape[0] - 1, g.shape[1] - 1) for _, g in jobs], np.int32)
    return jobs, ids, starts, goals


def replan(p, other, ids, starts, goals, reused, tag):
    """One replan_slots on p against the twin's plan_batch_slots, byte for byte; `reused` per query and what was launched."""
    got = p.replan_slots(ids, starts, goals, 2)
    T = p.timing()
    want = other.plan_batch_slots(ids, starts, goals, 2)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(got[:4], want)), (tag, got, want)
    assert got[4].tolist() == list(reused) and T["reused"] == sum(reused), (tag, got[4], T)
    if all(reused):
        assert T["search_launches"] == 0 and T["pops"] == 0, (tag, T)
    else:
        assert T["search_launches"] >= 1, (tag, T)
    return got


def path_of(out, q):
    return [tuple(int(v) for v in c) for c in out[1][out[0][q]:out[0][q + 1]]]


def test_replan_slots_behind_both_calls(planner, twin, oracle):
    jobs, ids, starts, goals = planning_fleet()
    n = len(jobs)
    # after set_grid_slots: all searched
    set_many(planner, jobs)
    for job in jobs:
        set_one(twin, *job)
    first = replan(planner, twin, ids, starts, goals, [False] * n, "set")
    assert (first[3] > 0).sum() >= 3, first[3]
    for q in range(n):
        want, _, _ = oracle.plan((jobs[q][1] != 0).astype(np.uint8), tuple(starts[q]), tuple(goals[q]), 2, literal=False)
        assert (path_of(first, q) or 0) == want, q
    # all kept and the same queries: nothing searched
    tick(planner, twin, jobs, [True] * n, "kept")
    replan(planner, twin, ids, starts, goals, [True] * n, "kept")
    # one grid changed under its stored path: the cell behind the path's first jump point, found with the CPU oracle
    q = int(np.argmax(first[3]))
    path = path_of(first, q)
    (ax, ay), (bx, by) = path[0], path[1]
    cell = (ax + int(np.sign(bx - ax)), ay + int(np.sign(by - ay)))
    assert cell != tuple(goals[q]) and jobs[q][1][cell] == 0
    changed = jobs[q][1].copy()
    changed[cell] = 7
    want, _, _ = oracle.plan((changed != 0).astype(np.uint8), tuple(starts[q]), tuple(goals[q]), 2, literal=False)
    assert want != path
    jobs[q] = (jobs[q][0], changed)
    tick(planner, twin, jobs, [v != q for v in range(n)], "changed", changed=(q,))
    out = replan(planner, twin, ids, starts, goals, [v != q for v in range(n)], "changed")
    assert (path_of(out, q) or 0) == want
    # the same grids through set_grid_slots: every generation moves, all searched, the same answers
    set_many(planner, jobs)
    again = replan(planner, twin, ids, starts, goals, [False] * n, "set again")
    assert all(x.tobytes() == y.tobytes() for x, y in zip(again[:4], out[:4]))


# ------------------------------------------------------------------ refusals and contexts
def test_refusals_change_nothing(planner):
    from fuxi_planner_amd import _lib
    rng = np.random.default_rng(824)
    held = {200: grid(rng, 40, 30), 201: grid(rng, 25, 60)}
    for g in held.values():
        g[-3:, -3:] = 0
    set_many(planner, list(held.items()))
    ids = np.array(list(held), np.int32)
    starts, goals = np.array([(0, 0), (0, 0)], np.int32), np.array([(39, 29), (24, 59)], np.int32)
    maps = {k: planner.debug_slot_maps(k) for k in held}
    plan = planner.replan_slots(ids, starts, goals, 2)
    assert not plan[4].any()
    L, h = planner._L, planner._h
    flags = np.full(_lib.MAX_GRID_SLOTS + 1, -5, np.int32)
    out_kept = _lib.ptr(flags, C.c_int32)
    good = (200, np.ones((6, 5), np.uint8))  # (job 0 of every refused call would overwrite slot 200)
    calls = (("set", lambda arr, n: L.fxjps_set_grid_slots(h, arr, n)), ("refresh", lambda arr, n: L.fxjps_refresh_grid_slots(h, arr, n, out_kept)))

    def refused(arr, n, job=None):
        for name, call in calls:
            assert call(arr, n) == _lib.E_ARG, (name, n, job)
            if job is not None:
                assert b"job %d" % job in L.fxjps_last_error(h), (name, L.fxjps_last_error(h))

    free = np.zeros((4, 4), np.uint8)
    for field, value in (("slot", -1), ("slot", _lib.MAX_GRID_SLOTS), ("slot", 200), ("occ", None), ("W", 0), ("W", 8191), ("H", -3), ("H", 8191),
                         ("reserved", 1), ("reserved", -1)):
        arr, keep = c_jobs([good, (201, free)])
        if field == "occ":
            arr[1].occ = C.POINTER(C.c_uint8)()
        else:
            setattr(arr[1], field, value)
        refused(arr, 2, job=1)
    arr, keep = c_jobs([(s, free) for s in range(_lib.MAX_GRID_SLOTS)] + [(0, free)])
    for n in (-1, _lib.MAX_GRID_SLOTS + 1):
        refused(arr, n)
    refused(None, 1)
    arr, keep = c_jobs([good])
    assert L.fxjps_refresh_grid_slots(h, arr, 1, None) == _lib.E_ARG  # (NULL out_kept with n > 0)
    # an empty call is no error, and does nothing
    assert L.fxjps_set_grid_slots(h, None, 0) == 0 and L.fxjps_refresh_grid_slots(h, None, 0, None) == 0
    assert (flags == -5).all()
    # the slots, their generations and the stored results: untouched
    for k, g in held.items():
        assert planner.get_grid_slot(k).tobytes() == g.tobytes(), k
        now = planner.debug_slot_maps(k)
        assert all(now[name].tobytes() == maps[k][name].tobytes() for name in now), k
    again = planner.replan_slots(ids, starts, goals, 2)
    assert again[4].all() and planner.timing()["search_launches"] == 0
    assert all(x.tobytes() == y.tobytes() for x, y in zip(again[:4], plan[:4]))


def test_the_binding(planner, twin):
    """Planner.set_grid_slots / refresh_grid_slots: matrix[x][y] with an obstacle iff == 1, as Planner.set_grid_slot."""
    rng = np.random.default_rng(825)
    m = rng.choice([0.0, 1.0, 100.0, 0.5], (23, 31), p=[0.6, 0.2, 0.1, 0.1])
    ints = (rng.random((9, 40)) < 0.2).astype(np.int64)
    planner.set_grid_slots([(50, m), (51, ints)])
    twin.set_grid_slot(50, m)
    twin.set_grid_slot(51, ints)
    same_slots(planner, twin, [(50, (m == 1).astype(np.uint8)), (51, ints.astype(np.uint8))], "binding")
    m2 = np.where(m == 0.0, 100.0, m)  # (still free by the matrix rule: the prepared bytes are equal)
    assert planner.refresh_grid_slots([(50, m2), (51, ints)]) == [True, True]
    ints[4, 4] ^= 1
    assert planner.refresh_grid_slots([(51, ints), (50, m2)]) == [False, True]
    assert np.array_equal(planner.get_grid_slot(51), ints.astype(np.uint8))
    assert planner.refresh_grid_slots([]) == []
    planner.set_grid_slots([])
    with pytest.raises(ValueError):
        planner.set_grid_slots([(52, np.zeros(5))])


def test_two_contexts(twin):
    import fuxi_planner_amd as fx
    jobs = fleet(60)
    n = len(jobs)
    for job in jobs:
        set_one(twin, *job)

    def both_contexts(p2, tag):
        for s, g in jobs:
            want = twin.debug_slot_maps(s)
            for c in (0, 1):
                occ, got = p2.debug_slot_context(c, s)
                assert occ.tobytes() == g.tobytes(), (tag, c, s)
                for name in want:
                    assert got[name].tobytes() == want[name].tobytes(), (tag, c, s, name)

    with fx.Planner([0, 0]) as p2:
        set_many(p2, jobs)
        both_contexts(p2, "set")
        tick(p2, twin, jobs, [v != LARGE for v in range(n)], "two contexts, tick 2")
        both_contexts(p2, "tick 2")
        jobs[TAIL] = with_byte(jobs[TAIL], -1, 255)
        tick(p2, twin, jobs, [v not in (LARGE, TAIL) for v in range(n)], "two contexts, tick 3", changed=(TAIL,))
        both_contexts(p2, "tick 3")
