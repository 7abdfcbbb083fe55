"""GPU suite (-m gpu): fxjps_absorb_prior_slide -- the vehicles' detected rectangles folded into prior maps that grow to hold
them and are cut, in the same launch, to a keep window.

The yardstick is worldprep.slide_host -- the grow_host fold of the grow suite, then a numpy slice of it
(tests/test_slide_prior_host.py pins it) -- over get_prior_map() from before the call: after every call the bytes and
extents of EVERY set prior, named or not, and origin, shift, cut_lo / cut_hi, grown_wh, trimmed, every job's at / inside /
outside and changed are compared for equality.  What the slots make of a slid prior is compared with a twin handle whose
prior is the host result, uploaded at the new origin.

The constructed jobs use the resolution 0.25 and origins on its grid, and the windows are given in cells of the prior AS
UPLOADED with their bounds half a cell inside, so that every cell index below is exact; the placements and bounds that
truncate one cell off the rounded quotient are the host suite's."""
import numpy as np
import pytest

from test_absorb_prior_gpu import set_prior_bytes
from test_grow_prior_gpu import MODES, ORI, R, SHAPES, as_msg, at_origin, detected, job, make_priors, rectangles, same_slots, slot_fleet, upload
from test_grow_prior_host import host_fold

pytestmark = pytest.mark.gpu
INF = float("inf")


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


def window(prior, x0, y0, x1, y1):
    """The keep window that holds the cells [x0, x1) x [y0, y1) of the prior AS UPLOADED (None: no bound on that side)."""
    def at(k, c, none):
        return none if c is None else ORI[prior][k] + (c + 0.5) * R
    return ((at(0, x0, -INF), at(1, y0, -INF)), (at(0, x1, INF), at(1, y1, INF)))


def slide_and_check(p, set_priors, origins, jobs, mode, tag, keep, use, crops=None, limit=None):
    """One absorb_prior_slide on p against slide_host on the priors as they were; `origins` ({prior: origin now}) is moved
    on.  -> (before, after, records, per_job)."""
    from fuxi_planner_amd.worldprep import slide_host
    before = {k: p.get_prior_map(k) for k in set_priors}
    jobs = at_origin(jobs, origins)
    want, want_recs, want_jobs = slide_host(before, jobs, mode, crops, limit, keep, use)
    per_job, recs = p.absorb_prior_slide(jobs, mode, crops, limit, keep, use)
    assert per_job == want_jobs, (tag, per_job, want_jobs)
    assert recs == want_recs, (tag, recs, want_recs)      # W, H, shift, origin, changed, trimmed, grown_wh, cut_lo, cut_hi of every named prior
    for k, r in recs.items():
        assert p.prior_origin(k) == tuple(want_recs[k]["origin"]), (tag, k)
        origins[k] = tuple(r["origin"])
    after = {k: p.get_prior_map(k) for k in set_priors}
    for k in set_priors:  # (the priors no job names among them: untouched)
        assert after[k].shape == want[k].shape, (tag, k, after[k].shape, want[k].shape)
        assert after[k].tobytes() == want[k].tobytes(), (tag, k, np.argwhere(after[k] != want[k])[:5])
    return before, after, recs, per_job


# per prior, a window in cells of the prior as uploaded: it cuts the low side of x and the high side of y of what
# rectangles() grows (7 cells below and 9 above x, 9 below and 8 above y), through several of the rectangles
WINDOWS = {0: window(0, -3, -9, 6, 4), 1: window(1, -4, -2, 14, 8), 2: window(2, -3, None, 30, 35), 3: window(3, -5, -4, 120, 72)}


@pytest.mark.parametrize("mode", MODES)
def test_every_shape_and_arrangement(planner, mode):
    """Three priors per call with use none / always / over_limit and a fourth untouched, nine arrangements of rectangles on
    each; then the same jobs one call each."""
    priors = make_priors()
    limit = (140, 90)   # the 130 x 70 prior grows to 146 x 87: over the limit on x alone, and the whole window applies
    for named, uses in (((0, 1, 3), {0: "none", 1: "always", 3: "over_limit"}), ((1, 2, 3), {1: "over_limit", 2: "always", 3: "none"})):
        if uses[3] == "none":
            limit = (150, 90)
        origins = upload(planner, priors)
        rng = np.random.default_rng(871)
        jobs = [j for k in named for j in rectangles(rng, k, k % 2)]
        jobs = [jobs[i] for i in np.random.default_rng(872).permutation(len(jobs))]
        keep = {k: WINDOWS[k] for k in named}
        before, after, recs, per_job = slide_and_check(planner, list(SHAPES), origins, jobs, mode, (mode, named), keep, uses, limit=limit)
        assert sorted(recs) == list(named)
        for k in named:
            pw, ph = SHAPES[k]
            assert recs[k]["grown_wh"] == (pw + 16, ph + 17), (k, recs[k])
            cut = uses[k] == "always" or (uses[k] == "over_limit" and k == 3)
            assert recs[k]["trimmed"] is cut and (recs[k]["cut_lo"] != (0, 0)) is cut, (k, recs[k])
            if not cut:
                assert recs[k]["shift"] == (7, 9) and (recs[k]["W"], recs[k]["H"]) == (pw + 16, ph + 17)
        assert recs[named[1]]["shift"] == {1: (4, 2), 2: (3, 9)}[named[1]]     # 7 - 3 cut on x, nothing cut below on y (no bound)
        assert any(j[2] > 0 for j in per_job) and any(j[1] == 0 for j in per_job) and recs[named[1]]["changed"] > 0
        # ... and one call per job from the upload, every call against the host
        origins = upload(planner, priors)
        for i, j in enumerate(jobs):
            slide_and_check(planner, [j[8]], origins, [j], mode, (mode, named, "alone", i), {j[8]: WINDOWS[j[8]]}, uses[j[8]], limit=limit)


@pytest.mark.parametrize("cut", ["low", "high", "both", "both axes", "nothing"])
def test_windows_on_either_side_through_a_rectangle_and_through_the_old_prior(planner, twin, cut):
    rng = np.random.default_rng(873)
    priors = {2: make_priors(874)[2]}
    # a rectangle sticking out on the low side of both axes, one on the high side, one apart: the 40 x 33 prior grows to 59 x 50
    jobs = [job(detected(rng, 14, 12, True), 2, -6, -5), job(detected(rng, 10, 16, False), 2, 35, 25), job(detected(rng, 4, 4, False), 2, 49, 41)]
    win = {"low": window(2, 3, None, None, None), "high": window(2, None, None, 37, None), "both": window(2, -2, None, 37, None),
           "both axes": window(2, 3, 4, 37, 30), "nothing": window(2, -6, -5, 53, 45)}[cut]
    for mode in MODES:
        origins = upload(planner, priors)
        _, after, recs, per_job = slide_and_check(planner, [2], origins, jobs, mode, (cut, mode), {2: win}, "always")
        r = recs[2]
        assert r["grown_wh"] == (59, 50) and r["trimmed"]
        if cut == "nothing":      # ... against fxjps_absorb_prior_grow on the twin: bytes and every field the two calls share
            upload(twin, priors)
            at, grown = twin.absorb_prior_grow(at_origin(jobs, {2: ORI[2]}), mode)
            got = twin.get_prior_map(2)
            assert got.shape == after[2].shape and got.tobytes() == after[2].tobytes()
            assert {k: r[k] for k in grown[2]} == grown[2] and [j[0] for j in per_job] == at and all(j[2] == 0 for j in per_job)
            assert r["cut_lo"] == r["cut_hi"] == (0, 0) and twin.prior_origin(2) == planner.prior_origin(2)
        else:
            want = {"low": ((9, 0), (0, 0)), "high": ((0, 0), (16, 0)), "both": ((4, 0), (16, 0)), "both axes": ((9, 9), (16, 15))}[cut]
            assert (r["cut_lo"], r["cut_hi"]) == want, (cut, r)
            # the old prior occupies grown cells 6 .. 46, 5 .. 38: "low" and "both axes" cut through it (shift goes negative), and
            # through the middle of the first rectangle (grown cells 0 .. 14); the high cuts go through the second (41 .. 51)
            assert r["shift"] == (6 - want[0][0], 5 - want[0][1])
            assert per_job[2][1:] == ((16, 0) if want[1][0] == 0 else (0, 16))          # the one apart: kept whole or excluded whole
            if cut != "high":
                assert 0 < per_job[0][1] < 14 * 12 and per_job[0][0][0] < 0
            if cut != "low":
                assert 0 < per_job[1][1] < 10 * 16


@pytest.mark.parametrize("extent", [63, 64, 65, 255, 256, 257])
def test_a_window_ends_at_a_wavefront_and_a_block(planner, extent):
    """Along y, the contiguous axis that adjacent lanes walk: windows of 63 .. 65 and 255 .. 257 cells that begin at the odd
    grown cell 7, so that a thread's window cell and its grown cell differ in every lane."""
    rng = np.random.default_rng(875 + extent)
    occ = rng.choice(np.array([0, 1, 100, 255], dtype=np.uint8), size=(3, 300))
    planner.clear_prior_map(5)
    set_prior_bytes(planner, 5, occ)
    origins = {5: ORI[5]}
    # a rectangle across the window's low edge, one across its high edge, and one below the prior (it grows by 4: k0[1] = 7)
    jobs = [job(detected(rng, 2, 6, True), 5, 1, 1), job(detected(rng, 3, 5, False), 5, 0, 3 + extent - 3), job(detected(rng, 1, 2, False), 5, 0, -4)]
    _, after, recs, per_job = slide_and_check(planner, [5], origins, jobs, "known", extent, {5: window(5, None, 3, None, 3 + extent)}, "always")
    r = recs[5]
    assert after[5].shape == (3, extent) and r["cut_lo"] == (0, 7) and r["shift"] == (0, -3) and r["cut_hi"] == (0, 304 - 7 - extent)
    assert [j[1:] for j in per_job] == [(8, 4), (9, 6), (0, 2)]
    untouched = np.ones((3, extent), dtype=bool)
    untouched[1:3, 0:4] = untouched[0:3, extent - 3:] = False
    assert (after[5][untouched] == occ[:, 3:3 + extent][untouched]).all() and (after[5] == 255).any() and (after[5] == 100).any()
    planner.clear_prior_map(5)


@pytest.mark.parametrize("mode", MODES)
def test_a_full_job_table_on_one_prior(planner, mode):
    rng = np.random.default_rng(876)
    origins = upload(planner, {3: make_priors()[3]})
    jobs = [job(detected(rng, 5, 7, v % 2 == 1), 3, int(rng.integers(-12, 140)), int(rng.integers(-10, 78))) for v in range(256)]
    _, after, recs, per_job = slide_and_check(planner, [3], origins, jobs, mode, mode, {3: window(3, 10, 6, 125, 66)}, "always")
    assert after[3].shape == (115, 60) and recs[3]["changed"] > 100 and recs[3]["shift"] == (-10, -6)
    assert sum(1 for j in per_job if j[1] == 0) > 10 and sum(1 for j in per_job if 0 < j[1] < 35) > 10


@pytest.mark.parametrize("mode", MODES)
def test_bytes_other_than_0_and_1_and_a_message(planner, mode):
    rng = np.random.default_rng(877)
    occ = rng.choice(np.array([0, 0, 1, 100, 255], dtype=np.uint8), size=(40, 33))
    planner.clear_prior_map(2)
    set_prior_bytes(planner, 2, occ)
    origins = {2: ORI[2]}
    # a layout-1 message with -1 cells over the prior's low corner, a matrix over its right edge; the window cuts both
    jobs = [job(as_msg((rng.random((20, 18)) < 0.5).astype(np.uint8)), 2, -5, -4), job((rng.random((9, 30)) < 0.5).astype(np.uint8), 2, 36, 10)]
    _, after, recs, _ = slide_and_check(planner, [2], origins, jobs, mode, mode, {2: window(2, -2, 2, 42, 31)}, "always")
    a = after[2]
    assert a.shape == (44, 29) and recs[2]["shift"] == (2, -2) and recs[2]["cut_lo"] == (3, 6)
    moved = a[2:42, :]                      # old cells [0:40, 2:31]
    decided = np.zeros(moved.shape, dtype=bool)
    decided[0:15, 0:12] = decided[36:40, 8:29] = True
    kept = occ[:, 2:31]
    assert (moved[~decided] == kept[~decided]).all() and (moved[~decided] == 255).any() and (moved[~decided] == 100).any()  # carried byte for byte
    assert set(np.unique(a[:2])) <= {0, 1} and set(np.unique(a[42:])) <= {0, 1}


def test_a_cropped_job_slides_the_prior_through_its_window(planner):
    rng = np.random.default_rng(878)
    m = np.zeros((40, 30), dtype=np.uint8)
    m[10:25, 8:20] = rng.random((15, 12)) < 0.3
    m[10, 8] = m[24, 19] = 1
    for mode in MODES:
        origins = upload(planner, {2: make_priors()[2]})
        jobs = [job(as_msg(m), 2, 25, 20, slot=120, ifa=1, variant=1, start=(12, 10), goal=(20, 15))]
        out = planner.prepare_slots_cropped(jobs)[0]
        status, rec = out[-2], out[-1]
        assert status == 0 and rec["lo"] == [10, 8] and rec["win"] == [14, 11], (status, rec)
        # message cell (10, 8) is prior cell (35, 28): the crop window alone grows the prior to 49 x 39; kept: x 20 .. 42, y 10 .. 39
        _, after, recs, per_job = slide_and_check(planner, [2], origins, jobs, mode, ("cropped", mode), {2: window(2, 20, 10, 42, None)}, "always", crops=[rec])
        assert after[2].shape == (22, 29) and recs[2]["grown_wh"] == (49, 39) and per_job == [((15, 18), 7 * 11, 7 * 11)]
    with pytest.raises(ValueError):
        planner.absorb_prior_slide(jobs, "overwrite", crops=[])


def test_refusals_and_a_window_over_the_limit_change_nothing(planner):
    from fuxi_planner_amd import FxjpsError, _lib
    base = make_priors()[2]
    upload(planner, {2: base})
    planner.clear_prior_map(14)
    good = job(np.ones((6, 5), dtype=np.uint8), 2, 38, 30)  # grows the 40 x 33 prior to 44 x 35
    win = window(2, 4, 3, 44, 35)                           # 40 x 32 of it
    for bad in (good[:8] + (14, (0.0, 0.0)), good[:3] + (0.0,) + good[4:], good[:2] + ((float("nan"), 0.0),) + good[3:], good[:9] + ((-15.0, -14.75),)):
        with pytest.raises(FxjpsError) as e:
            planner.absorb_prior_slide([good, bad], keep={2: win}, use="always")
        assert e.value.code == _lib.E_ARG and "job 1" in str(e.value), str(e.value)
    nan = float("nan")
    for keep, use, limit, word in (({2: ((nan, 0.0), (1.0, 1.0))}, "always", None, "NaN"), ({2: ((0.0, 0.0), (-1.0, 1.0))}, "always", None, "above its hi"),
                                   ({2: window(2, 50, 0, 60, 9)}, "always", None, "holds no cell"), ({2: win, 5: win}, "always", None, "no job names"),
                                   ({2: win}, "always", (39, 35), "above the limit"), ({2: win}, "over_limit", (43, 31), "above the limit"),
                                   ({2: win}, "none", (43, 35), "above the limit")):
        with pytest.raises(FxjpsError) as e:
            planner.absorb_prior_slide([good], limit=limit, keep=keep, use=use)
        assert e.value.code == _lib.E_ARG and word in str(e.value) and ("prior" in str(e.value)) , str(e.value)
    with pytest.raises(ValueError):
        planner.absorb_prior_slide([good], keep={2: win}, use="sometimes")
    with pytest.raises(ValueError):
        planner.absorb_prior_slide([good], mode="union")
    arr = (_lib.GrowJob * 1)()
    out = (_lib.PriorSlid * _lib.MAX_PRIOR_MAPS)()
    assert planner._L.fxjps_absorb_prior_slide(planner._h, arr, 1, 0, None, None, None) == _lib.E_ARG
    assert planner._L.fxjps_absorb_prior_slide(planner._h, arr, 257, 0, None, None, out) == _lib.E_ARG
    assert planner.absorb_prior_slide([]) == ([], {})
    got = planner.get_prior_map(2)
    assert got.shape == base.shape and got.tobytes() == base.tobytes() and planner.prior_origin(2) is None
    # exactly at the limit the window passes
    origins = {2: ORI[2]}
    _, after, recs, _ = slide_and_check(planner, [2], origins, [good], "overwrite", "at the limit", {2: win}, "over_limit", limit=(40, 32))
    assert after[2].shape == (40, 32) and recs[2]["trimmed"] and planner.prior_origin(2) == (ORI[2][0] + 4 * R, ORI[2][1] + 3 * R)
    planner.set_prior_map(2, base)
    assert planner.prior_origin(2) is None


def test_the_slots_see_the_slid_prior(planner, twin):
    priors = {k: make_priors(879)[k] for k in (2, 3)}
    origins = upload(planner, priors)
    upload(twin, priors)
    jobs = slot_fleet(160)
    assert planner.prepare_slots_world(jobs) == twin.prepare_slots_world(jobs)
    ids = [j[0] for j in jobs]
    same_slots(planner, twin, ids, "before")
    # A's detected map into prior 3, which grows by 10 x 5 cells on its low side and loses its columns from 125 and its rows from 68
    # on: the twin gets the host result as an upload
    _, after, recs, _ = slide_and_check(planner, [2, 3], origins, jobs[:1], "overwrite", "A absorbed", {3: window(3, None, None, 125, 68)}, "always")
    assert recs[3]["shift"] == (10, 5) and after[3].shape == (135, 73) and recs[3]["changed"] > 20 and recs[3]["cut_hi"] == (5, 2)
    twin.set_prior_map(3, after[3])
    moved = at_origin(jobs, origins)
    got, want = planner.refresh_slots_world(moved), twin.refresh_slots_world(moved)
    assert got == want
    same_slots(planner, twin, ids, "after")
    # ... and once more with the low side cut as well, so that the origin is og + reso * k0 and B's map sticks out of the prior
    _, after, recs, _ = slide_and_check(planner, [2, 3], origins, jobs[:1], "overwrite", "cut low", {3: window(3, -4, 1, 100, 60)}, "always")
    assert after[3].shape == (104, 59) and recs[3]["shift"] == (-6, -6) and origins[3] == (ORI[3][0] - 4 * R, ORI[3][1] + 1 * R)
    twin.set_prior_map(3, after[3])
    moved = at_origin(jobs, origins)
    got, want = planner.refresh_slots_world(moved), twin.refresh_slots_world(moved)
    assert got == want
    same_slots(planner, twin, ids, "after the low cut")
    # the slide itself moved no slot and no generation: nothing is built by a further refresh
    assert [o[6] for o in planner.refresh_slots_world(moved)] == [True, True, True]


def test_two_contexts_slide_alike(twin):
    import fuxi_planner_amd as fx
    priors = {k: make_priors(880)[k] for k in (2, 3)}
    jobs = slot_fleet(170)
    with fx.Planner([0, 0]) as p2:
        origins = upload(p2, priors)
        _, after, recs, _ = slide_and_check(p2, [2, 3], origins, jobs[:2], "known", "two contexts", {3: window(3, -4, 1, 125, 68)}, "always")
        assert recs[3]["shift"] == (4, -1) and recs[3]["cut_lo"] == (6, 6) and recs[3]["changed"] > 20     # grown by (10, 5), cut by (6, 6)
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


def fleet_at(t, first_slot):
    """Two vehicles on prior 7 (40 x 33), both drifting 8 cells to the LEFT per tick.  A's detected map (12 x 20 at cell
    (2 - 8 t, 6)) holds a wall at its column 4 over all its rows.  B (8 x 8 at (22 - 8 t, 12), empty) flies along y = 16 to
    the cell A's map began at the tick before: straight through the wall A saw then."""
    a = np.zeros((12, 20), dtype=np.uint8)
    a[4, :] = 1
    b = np.zeros((8, 8), dtype=np.uint8)
    ax, bx = 2 - 8 * t, 22 - 8 * t
    return [job(a, 7, ax, 6, slot=first_slot, ifa=0, variant=1, start=(1, 1), goal=(2, 18)),
            job(b, 7, bx, 12, slot=first_slot + 1, ifa=0, variant=1, start=(4, 4), goal=(ax + 8 + 1 - bx, 4))]


def test_fleet_tick_world_slides_the_prior_along_with_the_fleet(planner, twin):
    """The test that fails without fxjps_absorb_prior_slide: the fleet leaves the area of the uploaded prior; without slide=
    the tick that crosses grow_limit raises, with it every tick succeeds and the prior stays within the limit."""
    from fuxi_planner_amd import FxjpsError
    from fuxi_planner_amd.worldprep import slide_host
    start = np.zeros((40, 33), dtype=np.uint8)
    start[38, :] = 1                                    # a wall at the far right: behind the fleet from the first tick on
    for p in (planner, twin):
        p.set_prior_map(7, start)
    home = np.array([[0.0, 0.0], [1.0, 1.0]])
    margin, limit = 1.0, 48
    costs, shapes = [], []
    for t in range(6):
        jobs = fleet_at(t, 180)
        pos = np.array([[j[4][0], j[4][1], 1.0] for j in jobs])
        goals = np.array([[j[5][0], j[5][1], 1.5] for j in jobs])
        # ---- the host's tick: the fold over both jobs, then the keep box over rectangles, positions and goals plus the margin
        before = planner.get_prior_map(7)
        origin = planner.prior_origin(7) or ORI[7]
        moved = at_origin(jobs, {7: origin})
        lo = [min(min(j[2][k], j[4][k], j[5][k]) for j in jobs) - margin for k in range(2)]
        hi = [max(max(j[2][k] + np.asarray(j[1]).shape[k] * R, j[4][k], j[5][k]) for j in jobs) + margin for k in range(2)]
        want, want_recs, want_jobs = slide_host({7: before}, moved, "overwrite", None, limit, {7: (lo, hi)}, "over_limit")
        # ---- without slide the tick that crosses the limit raises (and leaves the twin's prior alone)
        if t < 2:
            twin.fleet_tick_world(jobs, pos, goals, home, publish=False, absorb="overwrite", grow=True, grow_limit=limit)
        elif t == 2:
            held = twin.get_prior_map(7)
            with pytest.raises(FxjpsError) as e:
                twin.fleet_tick_world(jobs, pos, goals, home, publish=False, absorb="overwrite", grow=True, grow_limit=limit)
            assert "above the limit" in str(e.value) and twin.get_prior_map(7).tobytes() == held.tobytes() and held.shape == (46, 33)
        recs = planner.fleet_tick_world(jobs, pos, goals, home, publish=False, absorb="overwrite", grow=True, grow_limit=limit, slide=margin)
        assert all(r["ok"] and r["status"] > 0 for r in recs), (t, [(r["ok"], r["status"]) for r in recs])
        got = planner.get_prior_map(7)
        assert got.shape == want[7].shape and got.tobytes() == want[7].tobytes(), (t, got.shape, want[7].shape)
        assert max(got.shape) <= limit and planner.prior_origin(7) == tuple(want_recs[7]["origin"]), (t, got.shape)
        assert recs[0]["slid"] is recs[1]["slid"] and recs[0]["slid"] == want_recs[7] and recs[0]["grown"] == want_recs[7], (t, recs[0]["slid"], want_recs[7])
        assert [r["absorbed"] for r in recs] == [(j[1], j[2]) for j in want_jobs] and [r["ori_pre"] for r in recs] == [tuple(origin)] * 2, t
        costs.append(recs[1]["cost"])
        shapes.append((got.shape, want_recs[7]["trimmed"]))
    # the prior grew for two ticks, was cut on the third, grew to exactly the limit (which is not cut) and was cut again
    assert shapes == [((40, 33), False), ((46, 33), False), ((32, 28), True), ((40, 28), False), ((48, 28), False), ((32, 28), True)], shapes
    # B flies 15 cells straight on the first tick; from then on around the wall A saw the tick before, which spans rows 6 .. 26
    assert costs[0] == 15.0 and all(c > 15.0 + 10 for c in costs[1:]), costs
    # the wall at the far right lay outside the keep box of the first cut and is gone; A's last walls are there
    final = planner.get_prior_map(7)
    # (B's empty map has since passed over the two older ones and cleared its 8 rows of them)
    assert start.sum() == 33 and sorted(set(np.argwhere(final)[:, 0])) == [4, 12, 20, 28] and final.sum() == 2 * 20 + 2 * 12
    with pytest.raises(ValueError):
        planner.fleet_tick_world(jobs, pos, goals, home, publish=False, absorb="overwrite", slide=1.0)     # needs grow=True
    with pytest.raises(ValueError):
        planner.fleet_tick_world(jobs, pos, goals, home, publish=False, absorb="overwrite", grow=True, slide=-0.5)
    for p in (planner, twin):
        p.clear_prior_map(7)
