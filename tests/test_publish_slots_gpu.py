"""GPU suite (-m gpu): fxjps_publish_slots -- the nav_msgs/OccupancyGrid data[] and / or the snapshot image of every named
grid slot by ONE call.  Everything is compared for equality with oracle/adapters.py (publish_map, snapshot_image), with the
goldens captured from the reference's own lines (adapters.json), and with the single-grid calls on a second handle."""
import ctypes as C

import numpy as np
import pytest

from conftest import load_golden
from test_adapters import unpack

pytestmark = pytest.mark.gpu
GUARD, TAIL = 0xA5, 32


@pytest.fixture(scope="module")
def planner():
    import fuxi_planner_amd as fx
    p = fx.Planner([0])
    yield p
    p.close()


@pytest.fixture(scope="module")
def other():
    import fuxi_planner_amd as fx
    p = fx.Planner([0])
    yield p
    p.close()


def check_against_oracle(res, grid, msg, channels, tag):
    from oracle import adapters
    data, (W, H), img = res
    assert (W, H) == grid.shape, tag
    if msg:
        ed, ew, eh = adapters.publish_map(grid)
        assert (ew, eh) == (W, H) and data.dtype == np.int8 and data.tobytes() == ed.tobytes(), tag
    else:
        assert data is None, tag
    if channels is not None:
        ei = adapters.snapshot_image(grid, channels)
        assert img.dtype == np.uint8 and img.shape == ei.shape and img.tobytes() == ei.tobytes(), tag
    else:
        assert img is None, tag


def raw_call(p, specs, n=None, extents=None):
    """The C call itself on guarded buffers.  specs: [(slot, msg, channels or None)]; extents: {slot: (W, H)} sizes the
    buffers (default 4096 bytes each).  -> (rc, error text, job array, [(msg buffer, image buffer)])"""
    from fuxi_planner_amd import _lib
    arr = (_lib.SlotPublish * max(len(specs), 1))()
    bufs = []
    for j, (slot, msg, ch) in zip(arr, specs):
        W, H = (extents or {}).get(slot, (64, 64))
        mb = np.full(W * H + TAIL, GUARD, np.uint8) if msg else None
        ib = np.full(W * H * max(ch, 1) + TAIL, GUARD, np.uint8) if ch is not None else None
        j.slot, j.channels, j.W, j.H = slot, ch if ch is not None else 0, -7, -7
        j.msg_data = mb.ctypes.data if msg else None
        j.image = ib.ctypes.data if ch is not None else None
        bufs.append((mb, ib))
    rc = p._L.fxjps_publish_slots(p._h, arr, len(specs) if n is None else n)
    return rc, p._L.fxjps_last_error(p._h).decode(), arr, bufs


def untouched(arr, bufs):
    return all(j.W == -7 and j.H == -7 for j in arr) and all((b == GUARD).all() for pair in bufs for b in pair if b is not None)


def test_goldens_through_slots(planner):
    G = load_golden("adapters.json")
    recs = [("publish", r) for r in G["publish"]] + [("snapshot", r) for r in G["snapshot"]]
    assert len(G["publish"]) >= 20 and len(G["snapshot"]) >= 15 and len(recs) <= 256
    for k, (_, r) in enumerate(recs):
        planner.set_grid_slot(k, unpack(r["grid_bits"], r["shape"]))
    res = planner.publish_slots(range(len(recs)), True, 3)
    assert len(res) == len(recs)
    for k, ((kind, r), (data, (W, H), img)) in enumerate(zip(recs, res)):
        assert [W, H] == list(r["shape"]), k
        if kind == "publish":
            assert (W, H) == (r["width"], r["height"]) and data.tolist() == r["data"], k
        else:
            assert list(img.shape) == r["rgb_shape"] and img.tobytes().hex() == r["rgb_hex"], k
        check_against_oracle((data, (W, H), img), unpack(r["grid_bits"], r["shape"]), True, 3, ("golden", k))
    for k in range(len(recs)):
        planner.clear_grid_slot(k)


EXTENTS = [(1, 1), (1, 33), (33, 1), (32, 32), (31, 65), (64, 64), (97, 5), (1, 1), (200, 130), (2, 2)]
SLOTS = [7, 3, 255, 0, 100, 41, 200, 3, 12, 9]  # not ascending; slot 3 is named by jobs 1 and 7


@pytest.fixture(scope="module")
def boundary_grids(planner):
    rng = np.random.default_rng(740)
    grids = {}
    for s, (W, H) in zip(SLOTS, EXTENTS):
        if s not in grids:  # (the job that names slot 3 again sees the 1 x 33 grid, whatever its line above says)
            grids[s] = (rng.random((W, H)) < 0.2).astype(np.uint8)
            planner.set_grid_slot(s, grids[s])
    return grids


@pytest.mark.parametrize("msg,channels", [(True, None), (False, 1), (True, 3)], ids=["msg", "gray", "msg_rgb"])
def test_tile_and_job_boundaries(planner, boundary_grids, msg, channels):
    from oracle import adapters
    grids = boundary_grids
    assert [grids[s].shape for s in SLOTS if s != 3] == [e for s, e in zip(SLOTS, EXTENTS) if s != 3] and grids[3].shape == (1, 33)
    res = planner.publish_slots(SLOTS, msg, channels)
    for j, (s, r) in enumerate(zip(SLOTS, res)):
        check_against_oracle(r, grids[s], msg, channels, ("boundary", j, s))
    # the caller's arrays end where their job ends: a guard behind every buffer survives
    ext = {s: g.shape for s, g in grids.items()}
    rc, err, arr, bufs = raw_call(planner, [(s, msg, channels) for s in SLOTS], extents=ext)
    assert rc == 0, err
    for j, (s, (mb, ib)) in enumerate(zip(SLOTS, bufs)):
        W, H = grids[s].shape
        assert (arr[j].W, arr[j].H) == (W, H), j
        if msg:
            assert mb[:W * H].tobytes() == adapters.publish_map(grids[s])[0].tobytes() and (mb[W * H:] == GUARD).all(), j
        if channels is not None:
            n = W * H * channels
            assert ib[:n].tobytes() == adapters.snapshot_image(grids[s], channels).tobytes() and (ib[n:] == GUARD).all(), j


def test_mixed_modes_in_one_call(planner, boundary_grids):
    """msg and image_channels per slot: every combination side by side, among them a job that only asks for its extents."""
    modes = [(True, None), (False, 1), (True, 3), (False, None), (True, 1), (False, 3), (True, None), (False, 1), (True, 3), (False, None)]
    res = planner.publish_slots(SLOTS, [m for m, _ in modes], [c for _, c in modes])
    for j, (s, r, (m, c)) in enumerate(zip(SLOTS, res, modes)):
        check_against_oracle(r, boundary_grids[s], m, c, ("mixed", j, s))


def test_256_jobs_in_one_call(planner):
    rng = np.random.default_rng(256)
    grids = [(rng.random((9 + (k * 7) % 32, 7 + (k * 5) % 17)) < 0.2).astype(np.uint8) for k in range(256)]
    shapes = {g.shape for g in grids}
    assert min(shapes) == (9, 7) and max(s[0] for s in shapes) == 40 and max(s[1] for s in shapes) == 23 and len(shapes) > 100
    for k, g in enumerate(grids):
        planner.set_grid_slot(k, g)
    res = planner.publish_slots(range(256), True, 3)
    for k, (r, g) in enumerate(zip(res, grids)):
        check_against_oracle(r, g, True, 3, ("256", k))
    for k in range(256):
        planner.clear_grid_slot(k)


def test_agrees_with_single_grid_calls_behind_prepare_slots(planner, other):
    from fuxi_planner_amd import synth
    raws = [synth.synth_grid(40 + 11 * v, 90 - 7 * v, 300 + v, 0.2) for v in range(8)]
    jobs = [(v, raw, (1, 1), (raw.shape[0] - 2, raw.shape[1] - 2), 1, v & 1) for v, raw in enumerate(raws)]
    outs = planner.prepare_slots(jobs)
    res = planner.publish_slots(range(8), True, 3)  # (immediately behind: nothing in between waits for the slots)
    assert all(o[5] for o in outs)
    for v, (data, (W, H), img) in enumerate(res):
        grid = planner.get_grid_slot(v)
        assert (W, H) == outs[v][3] == grid.shape and grid.any(), v
        other.set_grid_occ(grid)
        d1, w1, h1 = other.publish_map()
        assert (w1, h1) == (W, H) and data.tobytes() == d1.tobytes(), v
        assert img.tobytes() == other.snapshot_image(3).tobytes() and img.shape == (H, W, 3), v
    # a slot replaced by a smaller grid: the new extents and bytes come back
    small = synth.synth_grid(13, 37, 77, 0.3)
    planner.set_grid_slot(5, small)
    data, (W, H), img = planner.publish_slots([5], True, 1)[0]
    check_against_oracle((data, (W, H), img), small, True, 1, "replaced")
    assert (W, H) == (13, 37)
    for v in range(8):
        planner.clear_grid_slot(v)


def test_refusals_and_what_they_leave_alone(planner):
    from fuxi_planner_amd import _lib, waypoints
    from test_waypoint_slots_gpu import same, small_fleet
    grids, ids, s, g, inp = small_fleet(planner)  # slots 20 .. 25
    ext = {20 + k: occ.shape for k, occ in enumerate(grids)}
    planner.clear_grid_slot(60)
    good = (20, True, 3)
    for bad, what in [((60, True, None), "60"), ((_lib.MAX_GRID_SLOTS, True, None), "256"), ((-1, False, 1), "-1"), ((21, True, 2), "channels")]:
        rc, err, arr, bufs = raw_call(planner, [good, bad], extents=ext)
        assert rc == _lib.E_ARG and "job 1" in err and what in err, (bad, err)
        assert untouched(arr, bufs), bad
    # channels is not read without an image
    rc, err, arr, bufs = raw_call(planner, [(21, True, None)], extents=ext)
    arr[0].channels = 2
    assert planner._L.fxjps_publish_slots(planner._h, arr, 1) == 0
    specs = [(20 + (k % 6), True, None) for k in range(_lib.MAX_GRID_SLOTS + 1)]
    rc, err, arr, bufs = raw_call(planner, specs, extents=ext)
    assert rc == _lib.E_ARG and "257" in err and untouched(arr, bufs), err
    rc, err, arr, bufs = raw_call(planner, specs, n=-1, extents=ext)
    assert rc == _lib.E_ARG and untouched(arr, bufs), err
    assert planner._L.fxjps_publish_slots(planner._h, None, 1) == _lib.E_ARG
    assert planner._L.fxjps_publish_slots(planner._h, None, 0) == 0
    # a sizes-only call returns extents and writes nothing
    rc, err, arr, bufs = raw_call(planner, [(20 + k, False, None) for k in range(6)], extents=ext)
    assert rc == 0 and [(j.W, j.H) for j in arr] == [ext[20 + k] for k in range(6)], err
    # plan, publish, select on the resident paths: the waypoints of the same sequence without the publish call
    planner.set_grid_occ(grids[0])
    plan = planner.plan_batch_slots(ids, s, g, 2)
    want = waypoints.select_slots_batch(planner, **inp)
    again = planner.plan_batch_slots(ids, s, g, 2)
    res = planner.publish_slots(range(20, 26), True, 3)
    got = waypoints.select_slots_batch(planner, **inp)
    assert same(again, plan) and same(got, want)
    for k, r in enumerate(res):
        check_against_oracle(r, grids[k], True, 3, ("after plan", k))
        assert np.array_equal(planner.get_grid_slot(20 + k), grids[k]), k
    assert np.array_equal(planner.get_grid(), grids[0])
    assert C.sizeof(_lib.SlotPublish) == planner._L.fxjps_slot_publish_size()
