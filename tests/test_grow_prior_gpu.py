"""GPU suite (-m gpu): fxjps_absorb_prior_grow -- the vehicles' detected rectangles folded into prior maps that grow to hold
them.

The yardstick is worldprep.grow_host (pinned to the reference-made canvases by tests/test_grow_prior_host.py) folded job by
job over get_prior_map() from before the call (test_grow_prior_host.host_fold): the bytes and extents of EVERY set prior
after the call, named or not, and origin, shift, at and changed are compared for equality.  What the slots make of a grown
prior is compared with a twin handle whose prior is the host result, uploaded at the new origin.

Priors of 1 x 1, 9 x 4, 40 x 33 and 130 x 70; rectangles left of, right of, above, below, apart from, inside and covering
the prior, matrices and messages with -1 cells, all three modes; grown sides of 65 and 257 cells along y (one cell past a
wavefront's 64 lanes and a block's 256 threads).  The constructed jobs use the resolution 0.25 and origins on its grid, so
that the cell offsets below are exact; the placements that truncate one cell off the rounded quotient are the host suite's."""
import ctypes as C

import numpy as np
import pytest

from test_absorb_prior_gpu import set_prior_bytes
from test_grow_prior_host import host_fold
from test_refresh_slots_gpu import as_msg, same_slots, same_value

pytestmark = pytest.mark.gpu
R = 0.25
MODES = ("overwrite", "occupied", "known")
SHAPES = {0: (1, 1), 1: (9, 4), 2: (40, 33), 3: (130, 70)}
ORI = {0: (2.0, -1.0), 1: (-3.0, 2.0), 2: (-15.0, -15.0), 3: (4.0, -7.5), 5: (0.0, 0.0), 6: (0.0, 0.0), 7: (1.0, 1.0)}  # at the upload


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


def make_priors(seed=860):
    rng = np.random.default_rng(seed)
    return {k: (rng.random(s) < 0.3).astype(np.uint8) for k, s in SHAPES.items()}


def upload(p, priors):
    """-> the origins the priors lie at now: those of the upload."""
    for k, m in priors.items():
        p.set_prior_map(k, m)
        assert p.prior_origin(k) is None
    return {k: ORI[k] for k in priors}


def job(raw, prior, cx, cy, slot=0, ifa=0, variant=1, start=(0, 0), goal=(0, 0)):
    """A world job whose detected map's cell (0, 0) lies cx, cy cells from cell (0, 0) of the prior AS UPLOADED; start and goal
    in cells of the map.  Its ori_pre is the upload's: at_origin() moves it to where the prior lies now."""
    map_o = (ORI[prior][0] + cx * R, ORI[prior][1] + cy * R)
    pos = (map_o[0] + (start[0] + 0.5) * R, map_o[1] + (start[1] + 0.5) * R)
    to = (map_o[0] + (goal[0] + 0.5) * R, map_o[1] + (goal[1] + 0.5) * R)
    return (slot, raw, map_o, R, pos, to, ifa, variant, prior, ORI[prior])


def at_origin(jobs, origins):
    return [j[:9] + (tuple(origins[j[8]]),) + j[10:] for j in jobs]


def detected(rng, w, h, msg):
    m = (rng.random((w, h)) < 0.4).astype(np.uint8)
    return as_msg(m) if msg else m


def rectangles(rng, prior, first_msg):
    """Jobs on one prior: left of it, right of it, below, above, apart from it, inside and covering it."""
    pw, ph = SHAPES[prior]
    spec = [((5, min(ph, 7)), (-7, ph // 3)), ((6, min(ph, 5)), (pw + 1, 0)), ((min(pw, 7), 6), (pw // 3, -9)), ((min(pw, 9), 5), (0, ph + 2)),
            ((4, 3), (pw + 5, ph + 5)), ((max(pw // 2, 1), max(ph // 2, 1)), (pw // 4, ph // 4)), ((pw + 4, ph + 6), (-2, -3)),
            ((3, ph + 2), (-2, -1)), ((pw + 2, 2), (-1, ph - 1))]   # ... and two that straddle an edge
    return [job(detected(rng, w, h, (i + first_msg) % 2 == 1), prior, cx, cy) for i, ((w, h), (cx, cy)) in enumerate(spec)]


def grow_and_check(p, set_priors, origins, jobs, mode, tag, crops=None, limit=None):
    """One absorb_prior_grow on p against host_fold on the priors as they were; `origins` ({prior: origin now}) is moved
    on.  -> (before, after, grown)."""
    before = {k: p.get_prior_map(k) for k in set_priors}
    jobs = at_origin(jobs, origins)
    want, want_origin, want_shift, want_at, want_changed = host_fold(before, jobs, mode, crops)
    at, grown = p.absorb_prior_grow(jobs, mode, crops, limit)
    assert at == want_at, (tag, at, want_at)
    assert sorted(grown) == sorted(want_origin), (tag, sorted(grown))
    for k, g in grown.items():
        assert (g["W"], g["H"]) == want[k].shape and g["shift"] == want_shift[k] and g["origin"] == want_origin[k], (tag, k, g, want[k].shape)
        assert g["changed"] == want_changed[k], (tag, k, g["changed"], want_changed[k])
        assert p.prior_origin(k) == tuple(want_origin[k]), (tag, k)
        origins[k] = tuple(want_origin[k])
    after = {k: p.get_prior_map(k) for k in set_priors}
    for k in set_priors:  # (the priors no job names among them: untouched)
        assert after[k].shape == want[k].shape, (tag, k, after[k].shape, want[k].shape)
        assert after[k].tobytes() == want[k].tobytes(), (tag, k, np.argwhere(after[k] != want[k])[:5])
    return before, after, grown


@pytest.mark.parametrize("mode", MODES)
def test_every_shape_and_arrangement(planner, mode):
    priors = make_priors()
    finals = []
    for named in ((0, 1, 3), (1, 2, 3)):  # three priors in one call of interleaved jobs, the fourth left untouched
        origins = upload(planner, priors)
        rng = np.random.default_rng(861)
        jobs = [j for k in named for j in rectangles(rng, k, k % 2)]
        jobs = [jobs[i] for i in np.random.default_rng(862).permutation(len(jobs))]
        before, after, grown = grow_and_check(planner, list(SHAPES), origins, jobs, mode, (mode, named))
        assert sorted(grown) == list(named)
        for k in named:
            pw, ph = SHAPES[k]
            assert grown[k]["shift"] == (7, 9) and (grown[k]["W"], grown[k]["H"]) == (pw + 16, ph + 17), (k, grown[k])
            assert origins[k] == (ORI[k][0] - 7 * R, ORI[k][1] - 9 * R) and grown[k]["changed"] > 0
        # ... and job by job from the upload: the same bytes again (a call per job is the sequential fold by construction)
        origins = upload(planner, priors)
        for i, j in enumerate(jobs):
            grow_and_check(planner, [j[8]], origins, [j], mode, (mode, named, "alone", i))
        for k in SHAPES:
            got = planner.get_prior_map(k)
            assert got.shape == after[k].shape and got.tobytes() == after[k].tobytes(), (mode, named, k)
        finals.append(after)
    assert finals[0][2].tobytes() == priors[2].tobytes() and finals[1][0].tobytes() == priors[0].tobytes()


@pytest.mark.parametrize("mode", MODES)
def test_a_full_job_table_on_one_prior(planner, mode):
    rng = np.random.default_rng(863)
    origins = upload(planner, {3: make_priors()[3]})
    jobs = [job(detected(rng, 5, 7, v % 2 == 1), 3, int(rng.integers(-12, 140)), int(rng.integers(-10, 78))) for v in range(256)]
    _, after, grown = grow_and_check(planner, [3], origins, jobs, mode, mode)
    assert grown[3]["changed"] > 100 and grown[3]["shift"][0] > 0 and grown[3]["shift"][1] > 0 and after[3].shape[0] > 130 and after[3].shape[1] > 70


@pytest.mark.parametrize("side, low", [(63, False), (63, True), (255, False), (255, True)])
def test_a_side_grows_past_a_wavefront_and_a_block(planner, side, low):
    """Along y, the contiguous axis that adjacent lanes walk: 63 -> 65 and 255 -> 257 cells, at the high end and at the low
    end (where every old byte moves by two lanes)."""
    rng = np.random.default_rng(864 + side)
    occ = rng.choice(np.array([0, 1, 100, 255], dtype=np.uint8), size=(3, side))
    set_prior_bytes(planner, 5, occ)
    origins = {5: ORI[5]}
    jobs = [job(detected(rng, 2, 4, low), 5, 1, -2 if low else side - 2)]
    _, after, grown = grow_and_check(planner, [5], origins, jobs, "known", (side, low))
    assert after[5].shape == (3, side + 2) and grown[5]["shift"] == (0, 2 if low else 0)
    keep = after[5][:, 2:] if low else after[5][:, :side]
    untouched = np.ones(occ.shape, dtype=bool)
    untouched[1:3, :2] = untouched[1:3, side - 2:] = False
    assert (keep[untouched] == occ[untouched]).all() and (after[5] == 255).any()
    # a second grow on the grown prior, back across the boundary on the other axis' side: x 3 -> 5
    jobs = [job(as_msg(np.ones((2, side + 2), dtype=np.uint8)), 5, 3, -2 if low else 0)]
    _, after, grown = grow_and_check(planner, [5], origins, jobs, "overwrite", (side, low, "second"))
    assert after[5].shape == (5, side + 2) and after[5][3:].all() and grown[5]["changed"] == 2 * (side + 2)
    planner.clear_prior_map(5)


@pytest.mark.parametrize("mode", MODES)
def test_bytes_other_than_0_and_1_and_a_message(planner, mode):
    rng = np.random.default_rng(865)
    occ = rng.choice(np.array([0, 0, 1, 100, 255], dtype=np.uint8), size=(40, 33))
    set_prior_bytes(planner, 2, occ)
    assert planner.get_prior_map(2).tobytes() == occ.tobytes()
    origins = {2: ORI[2]}
    # a layout-1 message with -1 cells over the prior's low corner, a matrix over its right edge
    jobs = [job(as_msg((rng.random((20, 18)) < 0.5).astype(np.uint8)), 2, -5, -4), job((rng.random((9, 30)) < 0.5).astype(np.uint8), 2, 36, 10)]
    before, after, grown = grow_and_check(planner, [2], origins, jobs, mode, mode)
    a = after[2]
    assert a.shape == (50, 44) and grown[2]["shift"] == (5, 4)
    moved = a[5:45, 4:37]
    decided = np.zeros(moved.shape, dtype=bool)
    decided[0:15, 0:14] = decided[36:40, 10:33] = True
    assert (moved[~decided] == occ[~decided]).all() and (moved[~decided] == 255).any() and (moved[~decided] == 100).any()  # carried byte for byte
    beyond = np.ones(a.shape, dtype=bool)
    beyond[5:45, 4:37] = False
    assert set(np.unique(a[beyond])) <= {0, 1}
    if mode == "overwrite":
        assert set(np.unique(moved[decided])) == {0, 1}
    else:
        assert (moved[decided] == 255).any() or (moved[decided] == 100).any()  # occupied leaves them where it sets nothing, known under a -1


def test_a_cropped_job_grows_the_prior_through_its_window(planner):
    rng = np.random.default_rng(866)
    m = np.zeros((40, 30), dtype=np.uint8)
    m[10:25, 8:20] = rng.random((15, 12)) < 0.3
    m[10, 8] = m[24, 19] = 1
    for mode in MODES:
        origins = upload(planner, {2: make_priors()[2]})
        jobs = [job(as_msg(m), 2, 25, 20, slot=120, ifa=1, variant=1, start=(12, 10), goal=(20, 15))]
        out = planner.prepare_slots_cropped(jobs)[0]
        status, rec = out[-2], out[-1]
        assert status == 0 and rec["lo"] == [10, 8] and rec["win"] == [14, 11], (status, rec)
        _, after, grown = grow_and_check(planner, [2], origins, jobs, mode, ("cropped", mode), crops=[rec])
        # the window alone, at the crop's origin: message cell (10, 8) is prior cell (35, 28); the whole message would reach 65 x 50
        assert after[2].shape == (49, 39) and grown[2]["shift"] == (0, 0)
    with pytest.raises(ValueError):
        planner.absorb_prior_grow(jobs, "overwrite", crops=[])


def test_a_call_that_needs_no_growth_is_absorb_prior(planner, twin):
    priors = make_priors(867)
    rng = np.random.default_rng(868)
    # every rectangle inside its prior: one in a corner of the 9 x 4 prior, one covering it exactly, eight in the larger two
    jobs = [job(detected(rng, 4, 2, True), 1, 3, 1), job(detected(rng, 9, 4, False), 1, 0, 0)]
    jobs += [job(detected(rng, 12, 9, v % 2 == 0), (2, 3)[v % 2], 3 * v, 2 * v + 1) for v in range(8)]
    for mode in MODES:
        origins = upload(planner, priors)
        upload(twin, priors)
        _, after, grown = grow_and_check(planner, list(SHAPES), origins, jobs, mode, ("inside", mode))
        counts, changed = twin.absorb_prior(jobs, mode)
        assert all(c[1] == 0 for c in counts)
        for k in SHAPES:
            got = twin.get_prior_map(k)
            assert after[k].shape == got.shape == SHAPES[k] and after[k].tobytes() == got.tobytes(), (mode, k)
        assert {k: g["changed"] for k, g in grown.items()} == changed
        assert all(g["shift"] == (0, 0) and tuple(g["origin"]) == ORI[k] for k, g in grown.items())


def test_refusals_and_the_limit_change_nothing(planner):
    from fuxi_planner_amd import FxjpsError, _lib
    base = make_priors()[2]
    origins = upload(planner, {2: base})
    planner.clear_prior_map(14)
    good = job(np.ones((6, 5), dtype=np.uint8), 2, 38, 30)  # grows the 40 x 33 prior to 44 x 35
    for bad in (good[:8] + (14, (0.0, 0.0)), good[:3] + (0.0,) + good[4:], good[:2] + ((float("nan"), 0.0),) + good[3:],
                good[:2] + ((1e12, 0.0),) + good[3:], good + ((float("inf"), 0.0),), good[:9] + ((-15.0, -14.75),), good[:3] + (0.5,) + good[4:]):
        with pytest.raises(FxjpsError) as e:
            planner.absorb_prior_grow([good, bad])
        assert e.value.code == _lib.E_ARG and "job 1" in str(e.value), str(e.value)
    for limit in ((43, 35), (44, 34), 43):
        with pytest.raises(FxjpsError) as e:
            planner.absorb_prior_grow([good], limit=limit)
        assert e.value.code == _lib.E_ARG and "above the limit" in str(e.value), str(e.value)
    with pytest.raises(ValueError):
        planner.absorb_prior_grow([good[:8]])          # no prior named
    with pytest.raises(ValueError):
        planner.absorb_prior_grow([good], mode="union")
    arr = (_lib.GrowJob * 1)()
    out = (_lib.PriorGrown * _lib.MAX_PRIOR_MAPS)()
    assert planner._L.fxjps_absorb_prior_grow(planner._h, arr, 1, 0, None, None) == _lib.E_ARG
    assert planner._L.fxjps_absorb_prior_grow(planner._h, arr, 257, 0, None, out) == _lib.E_ARG
    assert planner.absorb_prior_grow([]) == ([], {})
    got = planner.get_prior_map(2)
    assert got.shape == base.shape and got.tobytes() == base.tobytes() and planner.prior_origin(2) is None
    # exactly at the limit it passes
    _, after, grown = grow_and_check(planner, [2], origins, [good], "overwrite", "at the limit", limit=(44, 35))
    assert after[2].shape == (44, 35)
    # set_prior_map and clear_prior_map forget the origin
    moved = job(np.ones((2, 2), dtype=np.uint8), 2, -3, -3)
    grow_and_check(planner, [2], origins, [moved], "overwrite", "moved")
    assert planner.prior_origin(2) == (ORI[2][0] - 3 * R, ORI[2][1] - 3 * R)
    planner.set_prior_map(2, base)
    assert planner.prior_origin(2) is None
    grow_and_check(planner, [2], {2: ORI[2]}, [moved], "overwrite", "moved again")
    planner.clear_prior_map(2)
    assert planner.prior_origin(2) is None


def slot_fleet(first_slot):
    """Three vehicles: A and B on prior 3 with their detected maps apart, C on prior 2.  A's map sticks out of prior 3 on
    the low side of both axes, so the prior's origin moves."""
    rng = np.random.default_rng(869)
    a = (rng.random((33, 40)) < 0.1).astype(np.uint8)
    a[:3, :3] = a[-3:, -3:] = 0
    b = (rng.random((30, 25)) < 0.05).astype(np.uint8)
    b[:3, :3] = b[-3:, -3:] = 0
    c = (rng.random((20, 20)) < 0.05).astype(np.uint8)
    c[:3, :3] = c[-3:, -3:] = 0
    s = first_slot
    return [job(as_msg(a), 3, -10, -5, slot=s, ifa=1, variant=0, start=(1, 1), goal=(31, 38)),
            job(b, 3, 90, 40, slot=s + 1, ifa=1, variant=1, start=(1, 1), goal=(28, 23)),
            job(c, 2, 4, 4, slot=s + 2, ifa=0, variant=1, start=(1, 1), goal=(18, 18))]


def test_the_slots_see_the_grown_prior(planner, twin):
    priors = {k: make_priors(870)[k] for k in (2, 3)}
    origins = upload(planner, priors)
    upload(twin, priors)
    jobs = slot_fleet(130)
    assert planner.prepare_slots_world(jobs) == twin.prepare_slots_world(jobs)
    ids = [j[0] for j in jobs]
    same_slots(planner, twin, ids, "before")
    # A's detected map into prior 3, which grows by 10 x 5 cells on its low side: the twin gets the host result as an upload
    _, after, grown = grow_and_check(planner, [2, 3], origins, jobs[:1], "overwrite", "A absorbed")
    assert grown[3]["shift"] == (10, 5) and after[3].shape == (140, 75) and grown[3]["changed"] > 20
    twin.set_prior_map(3, after[3])
    moved = at_origin(jobs, origins)
    assert moved[1][9] == (ORI[3][0] - 10 * R, ORI[3][1] - 5 * R) and moved[2][9] == ORI[2]
    got, want = planner.refresh_slots_world(moved), twin.refresh_slots_world(moved)
    assert got == want
    same_slots(planner, twin, ids, "after")
    # A's canvas holds its own detected map where the prior changed, and B's canvas shows A's cells only as the grown margin:
    # both canvases changed in extent or bytes for B, not for A or C
    assert [o[6] for o in got] == [True, False, True], [o[6] for o in got]
    # the grow itself moved no slot and no generation: nothing is built by a further refresh
    planner.absorb_prior_grow(moved[:1], "overwrite")
    assert [o[6] for o in planner.refresh_slots_world(moved)] == [True, True, True]
    assert planner.get_prior_map(3).tobytes() == after[3].tobytes()   # (absorbing the same map twice changes nothing)


def wall_fleet(first_slot):
    """Two vehicles on the empty 32 x 64 prior 6.  A flies LEFT of it: its detected map (20 x 40 at cell (-40, 12)) holds a
    wall at its x = 8, the prior frame's x = -32, over all its rows.  B (8 x 8 at (-44, 28), empty) flies along y = 32 from
    x = -40 to x = 24, into the prior: straight through where A sees the wall."""
    a = np.zeros((20, 40), dtype=np.uint8)
    a[8, :] = 1
    b = np.zeros((8, 8), dtype=np.uint8)
    s = first_slot
    return [job(a, 6, -40, 12, slot=s, ifa=0, variant=1, start=(2, 2), goal=(17, 37)),
            job(b, 6, -44, 28, slot=s + 1, ifa=0, variant=1, start=(4, 4), goal=(68, 4))]


def test_fleet_tick_world_grows_the_prior_to_what_one_vehicle_saw(planner, twin):
    empty = np.zeros((32, 64), dtype=np.uint8)
    for p in (planner, twin):
        p.set_prior_map(6, empty)
    jobs = wall_fleet(140)
    pos = np.array([[j[4][0], j[4][1], 1.0] for j in jobs])
    goals = np.array([[j[5][0], j[5][1], 1.5] for j in jobs])
    home = np.array([[0.0, 0.0], [1.0, 1.0]])
    ticks, flat = [], []
    for t in range(2):
        recs = planner.fleet_tick_world(jobs, pos, goals, home, publish=True, absorb="overwrite", grow=True)
        same = twin.fleet_tick_world(jobs, pos, goals, home, publish=True, absorb="overwrite")   # grow=False: what it is today
        assert all(r["ok"] and r["status"] > 0 for r in recs) and all(r["ok"] and r["status"] > 0 for r in same)
        for v in range(2):
            assert set(recs[v]) == set(same[v]) | {"ori_pre", "grown"} and not {"ori_pre", "grown"} & set(same[v]), (t, v)
        ticks.append(recs)
        flat.append(same)
    # ---- without growth: both rectangles lie outside the uploaded prior, every cell is dropped, B never learns of the wall
    assert [[r["absorbed"] for r in tick] for tick in flat] == [[(0, 800), (0, 64)]] * 2
    assert twin.get_prior_map(6).shape == (32, 64) and not twin.get_prior_map(6).any() and twin.prior_origin(6) is None
    assert flat[0][1]["cost"] == flat[1][1]["cost"] == 64.0
    # ---- with growth: tick 1 is that same tick; the prior then reaches 44 cells further left and holds A's wall
    for v in range(2):
        for k in flat[0][v]:
            if k != "absorbed":
                assert same_value(ticks[0][v][k], flat[0][v][k]), (v, k)
    assert [r["absorbed"] for r in ticks[0]] == [(800, 0), (64, 0)]
    assert [r["ori_pre"] for r in ticks[0]] == [(0.0, 0.0)] * 2 and [r["ori_pre"] for r in ticks[1]] == [(-11.0, 0.0)] * 2
    g = ticks[0][0]["grown"]
    assert g is ticks[0][1]["grown"] and (g["W"], g["H"], g["shift"], g["origin"], g["changed"]) == (76, 64, (44, 0), [-11.0, 0.0], 40)
    assert planner.prior_origin(6) == (-11.0, 0.0)
    grown = planner.get_prior_map(6)
    assert grown.shape == (76, 64) and grown[12, 12:52].all() and grown.sum() == 40
    assert ticks[1][0]["grown"]["changed"] == 0 and ticks[1][0]["grown"]["shift"] == (0, 0)
    # tick 1: B flies straight (64 cells); tick 2: around the wall A has seen, on the same canvas
    assert ticks[0][1]["cost"] == 64.0 and ticks[1][1]["cost"] > 64.0 + 10
    assert ticks[1][1]["shape"] == ticks[0][1]["shape"] and ticks[1][1]["start"] == ticks[0][1]["start"]
    for p in (planner, twin):
        p.clear_prior_map(6)


def test_two_contexts_grow_alike(twin):
    import fuxi_planner_amd as fx
    priors = {k: make_priors(871)[k] for k in (2, 3)}
    jobs = slot_fleet(150)
    with fx.Planner([0, 0]) as p2:
        origins = upload(p2, priors)
        _, after, grown = grow_and_check(p2, [2, 3], origins, jobs[:2], "known", "two contexts")
        assert grown[3]["shift"] == (10, 5) and grown[3]["changed"] > 20
        for k in (2, 3):
            twin.set_prior_map(k, after[k])
        moved = at_origin(jobs, origins)
        assert p2.prepare_slots_world(moved) == twin.prepare_slots_world(moved)
        for j in jobs:
            want_occ, want = twin.get_grid_slot(j[0]), twin.debug_slot_maps(j[0])
            for c in (0, 1):
                occ, got = p2.debug_slot_context(c, j[0])
                assert occ.tobytes() == want_occ.tobytes(), (c, j[0])
                for name in want:
                    assert got[name].tobytes() == want[name].tobytes(), (c, j[0], name)
