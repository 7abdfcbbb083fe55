"""GPU suite (-m gpu): fxjps_absorb_prior -- the vehicles' detected rectangles pasted into the prior maps on the device
(DESIGN.md section 3.20).

The yardstick is worldprep.absorb_host (pinned to the reference-made canvases by tests/test_absorb_prior_host.py) applied job
by job to get_prior_map() from before the call: the bytes of EVERY set prior after the call, named or not, and inside,
outside and changed are compared for equality.  What the slots make of an absorbed prior is compared with a twin handle
whose prior is the host result, uploaded.

Priors of 1 x 1, 9 x 4, 40 x 33, 130 x 70 (H no multiple of 16) and 520 x 510 (1037 blocks); rectangles inside the prior,
covering it, sticking out on each side, disjoint, one cell wide and one cell high; matrices and messages with -1 cells; all
three modes.  The constructed jobs use the resolution 0.25 and origins on its grid; the placements that truncate one cell off
the rounded quotient come from the fixture."""
import ctypes as C

import numpy as np
import pytest

from test_refresh_slots_gpu import as_msg, same_slots, same_value
from test_world_slots_gpu import fixture_pair
from worldprep_cases import placements

pytestmark = pytest.mark.gpu
R = 0.25
MODES = ("overwrite", "occupied", "known")
SHAPES = {0: (1, 1), 1: (9, 4), 2: (40, 33), 3: (130, 70), 4: (520, 510)}
ORI = {0: (2.0, -1.0), 1: (-3.0, 2.0), 2: (-15.0, -15.0), 3: (4.0, -7.5), 4: (-40.0, 10.0), 6: (0.0, 0.0), 7: (1.0, 1.0)}


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


def make_priors(seed=850):
    rng = np.random.default_rng(seed)
    return {k: (rng.random(s) < 0.3).astype(np.uint8) for k, s in SHAPES.items()}


def set_prior_bytes(p, prior, occ):
    """The bytes as they are (Planner.set_prior_map hands in 0 / 1)."""
    occ = np.ascontiguousarray(occ, dtype=np.uint8)
    p._chk(p._L.fxjps_set_prior_map(p._h, prior, occ.ctypes.data_as(C.POINTER(C.c_uint8)), occ.shape[0], occ.shape[1]))


def job(raw, prior, cx, cy, slot=0, ifa=0, variant=1, start=(0, 0), goal=(0, 0)):
    """A world job whose detected map's cell (0, 0) lies cx, cy cells from the prior's; start and goal in cells of the map."""
    W = raw[1] if isinstance(raw, tuple) else raw.shape[0]
    assert W > 0
    map_o = (ORI[prior][0] + cx * R, ORI[prior][1] + cy * R)
    pos = (map_o[0] + (start[0] + 0.5) * R, map_o[1] + (start[1] + 0.5) * R)
    to = (map_o[0] + (goal[0] + 0.5) * R, map_o[1] + (goal[1] + 0.5) * R)
    return (slot, raw, map_o, R, pos, to, ifa, variant, prior, ORI[prior])


def detected(rng, w, h, msg):
    m = (rng.random((w, h)) < 0.4).astype(np.uint8)
    return as_msg(m) if msg else m


def rectangles(rng, prior, first_msg):
    """Jobs on one prior: inside, covering it wholly, out on each of the four sides, disjoint, 1 x N and N x 1."""
    pw, ph = SHAPES[prior]
    spec = [((max(pw // 2, 1), max(ph // 2, 1)), (pw // 4, ph // 4)), ((pw + 4, ph + 6), (-2, -3)),
            ((5, min(ph, 7)), (-3, ph // 3)), ((6, min(ph, 5)), (pw - 2, 0)), ((min(pw, 7), 6), (pw // 3, -4)), ((min(pw, 9), 5), (0, ph - 3)),
            ((4, 3), (pw + 5, ph + 5)), ((1, ph + 2), (pw // 2, -1)), ((pw + 2, 1), (-1, ph // 2))]
    return [job(detected(rng, w, h, (i + first_msg) % 2 == 1), prior, cx, cy) for i, ((w, h), (cx, cy)) in enumerate(spec)]


def host_apply(before, jobs, mode, crops=None):
    """absorb_host job by job on copies of `before` -> (after, [(inside, outside)], {named prior: cells that flipped})."""
    from fuxi_planner_amd import worldprep
    cur = {k: v.copy() for k, v in before.items()}
    counts = []
    for v, wj in enumerate(jobs):
        raw, map_o, reso, prior, ori_pre = wj[1], wj[2], wj[3], wj[8], wj[9]
        rec = crops[v] if crops is not None else None
        lo, win = (None, None) if rec is None else (rec["lo"], rec["win"])
        new, ins, out, _ = worldprep.absorb_host(cur[prior], ori_pre, raw, map_o if rec is None else rec["map_o"], reso, mode, lo=lo, win=win)
        cur[prior] = new
        counts.append((ins, out))
    named = sorted({wj[8] for wj in jobs})
    return cur, counts, {k: int(np.count_nonzero((cur[k] != 0) != (before[k] != 0))) for k in named}


def absorb_and_check(p, set_priors, jobs, mode, tag, crops=None):
    """One absorb_prior on p against host_apply on the priors as they were.  -> (before, after, changed)."""
    before = {k: p.get_prior_map(k) for k in set_priors}
    want, want_counts, want_changed = host_apply(before, jobs, mode, crops)
    counts, changed = p.absorb_prior(jobs, mode, crops)
    assert counts == want_counts, (tag, counts, want_counts)
    assert changed == want_changed, (tag, changed, want_changed)
    after = {k: p.get_prior_map(k) for k in set_priors}
    for k in set_priors:  # (the priors no job names among them: untouched)
        assert after[k].shape == want[k].shape and after[k].tobytes() == want[k].tobytes(), (tag, k, np.argwhere(after[k] != want[k])[:5])
    return before, after, changed


@pytest.mark.parametrize("mode", MODES)
def test_every_shape_and_arrangement(planner, mode):
    priors = make_priors()
    for k, m in priors.items():
        planner.set_prior_map(k, m)
    rng = np.random.default_rng(851)
    jobs = [j for k in SHAPES for j in rectangles(rng, k, k % 2)]
    order = np.random.default_rng(852).permutation(len(jobs))  # (the priors' jobs interleaved: the call groups them)
    jobs = [jobs[i] for i in order]
    before, after, changed = absorb_and_check(planner, list(SHAPES), jobs, mode, mode)
    assert all(changed[k] > 0 for k in (2, 3, 4)), changed
    if mode == "occupied":
        assert all(np.all(after[k] >= before[k]) for k in SHAPES)
    # each prior by itself, job by job: the same bytes again (a call per job is n sequential pastes by construction)
    for k, m in priors.items():
        planner.set_prior_map(k, m)
    for i, j in enumerate(jobs):
        absorb_and_check(planner, [j[8]], [j], mode, (mode, "alone", i))
    for k in SHAPES:
        assert planner.get_prior_map(k).tobytes() == after[k].tobytes(), (mode, k)


@pytest.mark.parametrize("mode", MODES)
def test_two_overlapping_jobs_in_both_orders(planner, mode):
    rng = np.random.default_rng(853)
    base = make_priors()[2]
    a, b = job(as_msg((rng.random((20, 18)) < 0.5).astype(np.uint8)), 2, 5, 4), job(as_msg((rng.random((22, 16)) < 0.5).astype(np.uint8)), 2, 12, 9)
    got = []
    for pair in ([a, b], [b, a]):
        planner.set_prior_map(2, base)
        got.append(absorb_and_check(planner, [2], pair, mode, (mode, len(got)))[1][2])
    # overwrite and known depend on the order where the two differ; occupied does not
    assert (got[0].tobytes() == got[1].tobytes()) == (mode == "occupied")


@pytest.mark.parametrize("mode", MODES)
def test_a_full_job_table_on_one_prior(planner, mode):
    rng = np.random.default_rng(854)
    planner.set_prior_map(3, make_priors()[3])
    jobs = [job(detected(rng, 5, 7, v % 2 == 1), 3, int(rng.integers(-4, 130)), int(rng.integers(-6, 70))) for v in range(256)]
    _, _, changed = absorb_and_check(planner, [3], jobs, mode, mode)
    assert changed[3] > 100


def test_several_priors_in_one_call_and_one_left_alone(planner):
    priors = make_priors(855)
    for k, m in priors.items():
        planner.set_prior_map(k, m)
    rng = np.random.default_rng(856)
    jobs = [job(detected(rng, 30, 20, v % 2 == 0), (1, 3, 4)[v % 3], 3 * v - 5, 2 * v - 3) for v in range(9)]
    before, after, changed = absorb_and_check(planner, list(SHAPES), jobs, "overwrite", "three priors")
    assert sorted(changed) == [1, 3, 4] and after[2].tobytes() == before[2].tobytes() and after[0].tobytes() == before[0].tobytes()


def test_a_cropped_job_is_absorbed_through_its_window(planner):
    from fuxi_planner_amd import _lib
    rng = np.random.default_rng(857)
    planner.set_prior_map(2, make_priors()[2])
    m = np.zeros((40, 30), dtype=np.uint8)
    m[10:25, 8:20] = rng.random((15, 12)) < 0.3
    m[10, 8] = m[24, 19] = 1
    for mode in MODES:
        jobs = [job(as_msg(m), 2, 3, 2, slot=120, ifa=1, variant=1, start=(12, 10), goal=(20, 15))]
        out = planner.prepare_slots_cropped(jobs)[0]
        status, rec = out[-2], out[-1]
        assert status == 0 and rec["lo"] == [10, 8] and rec["win"] == [14, 11], (status, rec)
        _, _, changed = absorb_and_check(planner, [2], jobs, mode, ("cropped", mode), crops=[rec])
        # the window alone: the whole message would have cleared or kept other cells
        whole = host_apply({2: make_priors()[2]}, jobs, "overwrite")[0][2]
        assert mode != "overwrite" or planner.get_prior_map(2).tobytes() != whole.tobytes()
        planner.set_prior_map(2, make_priors()[2])
    with pytest.raises(ValueError):
        planner.absorb_prior(jobs, "overwrite", crops=[])
    assert _lib.ABSORB_MODES == {"overwrite": 0, "occupied": 1, "known": 2}


def test_the_fixture_cases_with_truncated_placements(planner):
    for prior, c in zip((8, 9), fixture_pair()):
        assert any(int(q) != int(round(q)) for q in placements(c))
        planner.set_prior_map(prior, c["prior"])
        wj = (0, c["raw"], c["map_o"], c["reso"], c["pos"], c["goal_xy"], c["ifa"], c["variant"], prior, c["ori_pre"], c["map_t"])
        absorb_and_check(planner, [prior], [wj], "overwrite", ("fixture", prior))
        at = [int(q) for q in placements(c)]
        pw, ph = c["prior"].shape
        assert np.array_equal(planner.get_prior_map(prior), c["canvas"][at[2]:at[2] + pw, at[3]:at[3] + ph])  # the reference's own canvas
        planner.clear_prior_map(prior)


@pytest.mark.parametrize("mode", MODES)
def test_bytes_other_than_0_and_1(planner, mode):
    rng = np.random.default_rng(858)
    occ = rng.choice(np.array([0, 0, 1, 100, 255], dtype=np.uint8), size=(40, 33))
    set_prior_bytes(planner, 2, occ)
    assert planner.get_prior_map(2).tobytes() == occ.tobytes()
    jobs = [job(as_msg((rng.random((20, 18)) < 0.5).astype(np.uint8)), 2, 5, 4), job((rng.random((9, 30)) < 0.5).astype(np.uint8), 2, 28, -2)]
    before, after, _ = absorb_and_check(planner, [2], jobs, mode, mode)
    a, b = after[2], before[2]
    assert set(np.unique(a[a != b])) <= {0, 1} and (a[:5] == b[:5]).all() and (a[:5] == 255).any() and (a[:5] == 100).any()
    decided = np.zeros(a.shape, dtype=bool)
    decided[5:25, 4:22] = decided[28:37, 0:28] = True
    assert (a[~decided] == b[~decided]).all()
    if mode == "overwrite":
        assert set(np.unique(a[decided])) == {0, 1}
    else:
        assert (a[decided] == 255).any() or (a[decided] == 100).any()  # occupied leaves them where it sets nothing, known under a -1


def test_refusals_change_nothing(planner):
    from fuxi_planner_amd import FxjpsError, _lib
    base = make_priors()[2]
    planner.set_prior_map(2, base)
    planner.clear_prior_map(14)
    good = job(np.ones((6, 5), dtype=np.uint8), 2, 1, 1)
    for bad in (good[:8] + (14, (0.0, 0.0)), good[:3] + (0.0,) + good[4:], good[:2] + ((float("nan"), 0.0),) + good[3:],
                good[:2] + ((1e12, 0.0),) + good[3:]):
        with pytest.raises(FxjpsError) as e:
            planner.absorb_prior([good, bad])
        assert e.value.code == _lib.E_ARG and "job 1" in str(e.value), str(e.value)
    with pytest.raises(ValueError):
        planner.absorb_prior([good[:8]])          # no prior named
    with pytest.raises(ValueError):
        planner.absorb_prior([good], mode="union")
    arr = (_lib.AbsorbJob * 1)()
    assert planner._L.fxjps_absorb_prior(planner._h, arr, 1, 0, None) == _lib.E_ARG
    changed = np.zeros(_lib.MAX_PRIOR_MAPS, dtype=np.int64)
    assert planner._L.fxjps_absorb_prior(planner._h, arr, 257, 0, _lib.ptr(changed, C.c_int64)) == _lib.E_ARG
    assert planner.absorb_prior([]) == ([], {})
    assert planner.get_prior_map(2).tobytes() == base.tobytes()


def slot_fleet(first_slot):
    """Three vehicles: A and B on prior 3 with their detected maps apart, C on prior 2."""
    rng = np.random.default_rng(859)
    a = (rng.random((33, 40)) < 0.1).astype(np.uint8)
    a[:3, :3] = a[-3:, -3:] = 0
    b = (rng.random((30, 25)) < 0.05).astype(np.uint8)
    b[:3, :3] = b[-3:, -3:] = 0
    c = (rng.random((20, 20)) < 0.05).astype(np.uint8)
    c[:3, :3] = c[-3:, -3:] = 0
    s = first_slot
    return [job(as_msg(a), 3, 10, 5, slot=s, ifa=1, variant=0, start=(1, 1), goal=(31, 38)),
            job(b, 3, 90, 40, slot=s + 1, ifa=1, variant=1, start=(1, 1), goal=(28, 23)),
            job(c, 2, 4, 4, slot=s + 2, ifa=0, variant=1, start=(1, 1), goal=(18, 18))]


def test_the_slots_see_the_absorbed_prior(planner, twin):
    priors = make_priors(860)
    for p in (planner, twin):
        for k in (2, 3):
            p.set_prior_map(k, priors[k])
    jobs = slot_fleet(130)
    assert planner.prepare_slots_world(jobs) == twin.prepare_slots_world(jobs)
    ids = [j[0] for j in jobs]
    same_slots(planner, twin, ids, "before")
    # A's detected map into prior 3: the twin gets the host result as an upload
    before, after, changed = absorb_and_check(planner, [2, 3], jobs[:1], "overwrite", "A absorbed")
    assert changed[3] > 20
    twin.set_prior_map(3, after[3])
    assert twin.get_prior_map(3).tobytes() == planner.get_prior_map(3).tobytes()
    got, want = planner.refresh_slots_world(jobs), twin.refresh_slots_world(jobs)
    assert got == want
    same_slots(planner, twin, ids, "after")
    # A's canvas holds its own detected map where the prior flipped: kept.  B's canvas shows the flipped prior cells: built.
    # C's prior was not named: kept.
    assert [o[6] for o in got] == [True, False, True]
    # the absorb itself moved no slot and no generation: nothing is built by a further refresh
    planner.absorb_prior(jobs[:1], "overwrite")
    assert [o[6] for o in planner.refresh_slots_world(jobs)] == [True, True, True]


def wall_fleet(first_slot):
    """Two vehicles on the empty 64 x 64 prior 6.  A's detected map (20 x 40 at cell (22, 12)) holds a wall at its x = 8, the
    prior's x = 30, over all its rows; B (8 x 8 at (0, 28), empty) flies along y = 32 from x = 4 to x = 60: straight through
    where A sees the wall."""
    a = np.zeros((20, 40), dtype=np.uint8)
    a[8, :] = 1
    b = np.zeros((8, 8), dtype=np.uint8)
    s = first_slot
    return [job(a, 6, 22, 12, slot=s, ifa=0, variant=1, start=(2, 2), goal=(17, 37)),
            job(b, 6, 0, 28, slot=s + 1, ifa=0, variant=1, start=(4, 4), goal=(60, 4))]


def test_fleet_tick_world_shares_what_one_vehicle_saw(planner, twin):
    empty = np.zeros((64, 64), dtype=np.uint8)
    for p in (planner, twin):
        p.set_prior_map(6, empty)
    jobs = wall_fleet(140)
    pos = np.array([[j[4][0], j[4][1], 1.0] for j in jobs])
    goals = np.array([[j[5][0], j[5][1], 1.5] for j in jobs])
    home = np.array([[0.0, 0.0], [1.0, 1.0]])
    ticks = []
    for t in range(2):
        recs = planner.fleet_tick_world(jobs, pos, goals, home, publish=True, absorb="overwrite")
        want = twin.fleet_tick_world(jobs, pos, goals, home, publish=True)
        for v in range(2):
            assert set(recs[v]) == set(want[v]) | {"absorbed"} and "absorbed" not in want[v], (t, v)
            for k in want[v]:  # this tick's records are those of absorb=None on the prior as it was before the tick
                assert same_value(recs[v][k], want[v][k]), (t, v, k, recs[v][k], want[v][k])
        assert [r["absorbed"] for r in recs] == [(800, 0), (64, 0)]
        assert all(r["ok"] and r["status"] > 0 for r in recs)
        cells = [p.plan_batch_slots([jobs[1][0]], [recs[1]["start"]], [recs[1]["goal"]], 2) for p in (planner, twin)]
        assert all(x.tobytes() == y.tobytes() for x, y in zip(*cells))
        ticks.append(recs)
        # the twin learns on the host what the device has learnt
        twin.set_prior_map(6, host_apply({6: twin.get_prior_map(6)}, jobs, "overwrite")[0][6])
        assert planner.get_prior_map(6).tobytes() == twin.get_prior_map(6).tobytes()
    assert planner.get_prior_map(6)[30, 12:52].all() and planner.get_prior_map(6).sum() == 40
    # tick 1: B flies straight (56 cells); tick 2: around the wall A has seen
    assert ticks[0][1]["cost"] == 56.0 and ticks[1][1]["cost"] > ticks[0][1]["cost"] + 10
    assert ticks[1][0]["cost"] == ticks[0][0]["cost"]  # A's own canvas did not change


def test_two_contexts_absorb_alike(twin):
    import fuxi_planner_amd as fx
    priors = make_priors(861)
    jobs = slot_fleet(150)
    with fx.Planner([0, 0]) as p2:
        for k in (2, 3):
            p2.set_prior_map(k, priors[k])
        _, after, changed = absorb_and_check(p2, [2, 3], jobs[:2], "known", "two contexts")
        assert changed[3] > 20
        for k in (2, 3):
            twin.set_prior_map(k, after[k])
        assert p2.prepare_slots_world(jobs) == twin.prepare_slots_world(jobs)
        for j in jobs:
            want_occ, want = twin.get_grid_slot(j[0]), twin.debug_slot_maps(j[0])
            for c in (0, 1):
                occ, got = p2.debug_slot_context(c, j[0])
                assert occ.tobytes() == want_occ.tobytes(), (c, j[0])
                for name in want:
                    assert got[name].tobytes() == want[name].tobytes(), (c, j[0], name)


def test_fleet_tick_world_absorbs_a_cropped_job_through_its_window(planner):
    from fuxi_planner_amd import worldprep
    rng = np.random.default_rng(862)
    base = make_priors()[2]
    planner.set_prior_map(2, base)
    m = np.zeros((40, 30), dtype=np.uint8)
    m[10:25, 8:20] = rng.random((15, 12)) < 0.3
    m[10, 8] = m[24, 19] = 1
    jobs = [job(as_msg(m), 2, 3, 2, slot=160, ifa=1, variant=1, start=(12, 10), goal=(20, 15)),
            job(as_msg(np.zeros((12, 9), dtype=np.uint8)), 2, 1, 1, slot=161, ifa=1, variant=1, start=(2, 2), goal=(5, 5))]  # no occupied cell
    pos = np.array([[j[4][0], j[4][1], 1.0] for j in jobs])
    goals = np.array([[j[5][0], j[5][1], 1.5] for j in jobs])
    recs = planner.fleet_tick_world(jobs, pos, goals, np.zeros((2, 2)), publish=False, crop=True, absorb="known")
    assert [r["not_planned"] for r in recs] == [False, True]
    assert recs[0]["absorbed"] == (14 * 11, 0) and recs[1]["absorbed"] is None  # (a job that is not planned has no window)
    rec, outcome, _ = worldprep.crop_host(jobs[0][1], jobs[0][2], R, jobs[0][4], 1)
    assert outcome == 0 and rec["lo"] == [10, 8] and rec["win"] == [14, 11]
    want = host_apply({2: base}, jobs[:1], "known", crops=[rec])[0][2]
    assert planner.get_prior_map(2).tobytes() == want.tobytes() and want.tobytes() != base.tobytes()
