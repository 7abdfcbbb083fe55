"""GPU suite (-m gpu): a closed handle gives back every byte it allocated ("who frees what").

Planner.live_bytes() (fxjps_debug_live_bytes) counts the device and the pinned host bytes that the library's buffers hold,
where they are allocated and freed.  Each case reads it, opens a handle, works, closes the handle and reads it again: the
two readings are equal, exactly, for both counters.  A difference and not an absolute figure, because the module-scoped
planners of other test files are alive in the same process; a counter of the library's own and not the device's free
memory, because that moves under other processes' work and never shows a pinned host buffer at all."""
import numpy as np
import pytest

import cropprep_cases
import refresh_grid_cases as rc
import worldprep_cases

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(120)]  # (each case under a time limit of its own)


def slot_jobs(first_slot):
    """Two prepare_slots jobs of 48 x 40 raw cells, one per variant, from the refresh-grid cases' first tick."""
    jobs = []
    for v in (0, 1):
        st = rc.steps(48, 40, 1, v)[0]
        jobs.append((first_slot + v, st["raw"], st["start"], st["goal"], 1, v))
    return jobs


def test_one_context_every_buffer_family():
    import fuxi_planner_amd as fx
    from fuxi_planner_amd import synth, waypoints
    before = fx.Planner.live_bytes()
    p = fx.Planner([0])
    try:
        # the resident grid: a single call (the path arrives in the pinned h_path1), a batch, both waypoint rules over it
        occ = synth.synth_grid(96, 80, 3, 0.2)
        s, g = synth.synth_queries(occ, 3, 8)
        p.set_grid_occ(occ)
        p.plan_batch(s[:1], g[:1], 2)
        off, cells, cost, status = p.plan_batch(s, g, 2)
        pos, goal = (1.0, 2.0, 1.0), (9.0, 7.0, 1.0)
        waypoints.select_ccst_batch(p, 8, 0.2, (0.0, 0.0), pos, goal)
        waypoints.select_st_batch(p, 8, s, 0.2, (0.0, 0.0), pos, goal)
        # cell updates, then the streaming replan
        free = np.argwhere(occ == 0)[:4].astype(np.int32)
        p.update_cells(free, np.ones(4, np.uint8))
        p.plan_batch(s, g, 2)
        p.set_queries(s, g, 2)
        p.replan_frame()
        p.replan_frame(free, np.zeros(4, np.uint8))
        # a raw map prepared, then the same map with 16 cells flipped: the diff against the resident grid
        st = rc.steps(40, 32, 1, 1)[0]
        raw = st["raw"].copy()
        p.prepare_grid(raw, st["start"], st["goal"], 1, 1)
        raw[10:14, 10:14] ^= True
        dev0 = fx.Planner.live_bytes()[0]
        out = p.refresh_grid(raw, st["start"], st["goal"], 1, 1)
        dev1 = fx.Planner.live_bytes()[0]
        print("refresh_grid: prepared %s, changed %d, mode %d, device bytes %d -> %d" % (out[3], out[5], out[6], dev0, dev1))
        assert out[6] == 1, out
        assert dev1 > dev0, (dev0, dev1)  # (the diff buffer: what a handle used to keep when it was destroyed)
        p.publish_map()
        p.snapshot_image(1)
        # grid slots: set, prepared from raw maps, from world-frame jobs over a prior, from cropped messages; published
        p.set_grid_slot(3, occ)
        jobs = slot_jobs(0)
        outs = p.prepare_slots(jobs)
        assert all(o[5] for o in outs), outs
        c = next(c for c in worldprep_cases.cases() if not c["raises"] and c["prior"] is not None and c.get("prep"))
        p.set_prior_map(0, c["prior"])
        p.prepare_slots_world([(4, c["raw"], c["map_o"], c["reso"], c["pos"], c["goal_xy"], c["ifa"], c["variant"], 0, c["ori_pre"], c["map_t"])])
        c = next(c for c in cropprep_cases.cases() if c["status"] == 0)
        if c["prior"] is not None:
            p.set_prior_map(1, c["prior"])
        w = p.prepare_slots_cropped([(5, cropprep_cases.message(c), c["map_o"], c["reso"], c["pos"], c["goal_xy"], c["ifa"], 1,
                                      None if c["prior"] is None else 1, c["ori_pre"])])
        assert w[0][-2] == 0, w
        p.publish_slots([0, 1, 5], msg=True, image_channels=1)
        # a slots batch, the tick after it twice, and what the nodes send out, on the resident paths
        ids = [0, 1]
        starts, goals = [o[0] for o in outs], [o[1] for o in outs]
        soff = p.plan_batch_slots(ids, starts, goals, 2)[0]
        waypoints.select_slots_batch(p, [0, 1], starts, 0.2, (0.0, 0.0), pos, goal)
        waypoints.tick_outputs_slots(p, [0, 1], starts, 0.2, (0.0, 0.0), pos, goal, (0.0, 0.0), offsets=soff)
        p.replan_slots(ids, starts, goals, 2)
        assert p.replan_slots(ids, starts, goals, 2)[4].all()
        held = fx.Planner.live_bytes()
        print("live bytes: before", before, "open", held)
        assert held[0] > before[0] and held[1] > before[1], (before, held)
    finally:
        p.close()
    after = fx.Planner.live_bytes()
    print("live bytes: after", after)
    assert after == before, (before, after, (after[0] - before[0], after[1] - before[1]))


def test_two_contexts_on_one_device():
    import fuxi_planner_amd as fx
    from fuxi_planner_amd import synth
    before = fx.Planner.live_bytes()
    p = fx.Planner([0, 0])
    try:
        occ = synth.synth_grid(96, 80, 3, 0.2)
        s, g = synth.synth_queries(occ, 3, 8)
        p.set_grid_occ(occ)
        p.plan_batch(s, g, 2)
        assert all(o[5] for o in p.prepare_slots(slot_jobs(0)))
        held = fx.Planner.live_bytes()
        assert held[0] > before[0] and held[1] > before[1], (before, held)
    finally:
        p.close()
    assert fx.Planner.live_bytes() == before, (before, fx.Planner.live_bytes())


def test_created_and_closed_at_once():
    import fuxi_planner_amd as fx
    before = fx.Planner.live_bytes()
    fx.Planner([0]).close()
    assert fx.Planner.live_bytes() == before
    p = fx.Planner([0])
    p.close()
    p.close()
    p.__del__()
    del p
    assert fx.Planner.live_bytes() == before
