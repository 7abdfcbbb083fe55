"""GPU suite (-m gpu): the same six jobs through all four instantiations of the slot gather (k_slots_gather<WORLD, REFRESH>)
and, behind each, the goal and stage templates of its call -- prepare_slots, refresh_slots, prepare_slots_world,
refresh_slots_world -- each on slots of its own.  The slots are compared WITH EACH OTHER: job outputs, occupancy bytes and
all six derived maps, and with the single-grid path (prepare_grid / prepare_occupancy_msg on a second planner), which
shares prepared_byte and the build stage bodies with them.  `kept` is stated call by call.

The jobs, none larger than 24 cells a side:
  0  16 x 16, ifa 0, ccst: the prepared grid is the raw, exactly 256 cells -- its only gather block is full and job 1's
     first block follows it directly
  1  5 x 7, ifa 1, ccst: 11 x 13 = 143 cells, less than a block
  2  20 x 23, ifa 0, st (the step = 1 branch of the dilation): 460 cells, no multiple of 256; the job whose raw is flipped
  3  24 x 17, ifa 2, st (step = ifa): 36 x 29 = 1044 cells, five blocks
  4  a 13 x 21 message (layout 1) holding -1, 0 and 100, ifa 1, st, the start at x = -3 (low-side padding)
  5  18 x 11, ifa 0, ccst, the goal on an obstacle whose row has a free cell two cells on
The world form of a job has no prior, map_o = (0, 0) and map_reso = 1: a position of c + 0.5 (c - 0.5 below zero)
truncates toward zero to cell c, the cell of the plain job."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
N = 6
FLIP = 2


@pytest.fixture(scope="module")
def planner():
    import fuxi_planner_amd as fx
    p = fx.Planner([0])
    yield p
    p.close()


@pytest.fixture(scope="module")
def single():
    import fuxi_planner_amd as fx
    p = fx.Planner([0])
    yield p
    p.close()


def fleet():
    """-> [(raw, start, goal, ifa, variant)]"""
    rng = np.random.default_rng(14)
    maps = [(rng.random(s) < 0.08).astype(np.uint8) for s in ((16, 16), (5, 7), (20, 23), (24, 17), (13, 21), (18, 11))]
    for m in maps:
        m[:2, :2] = 0
    m4 = maps[4]
    data = np.where(m4.T > 0, 100, 0).astype(np.int8)
    data[(m4.T == 0) & (np.add.outer(np.arange(m4.shape[1]), np.arange(m4.shape[0])) % 5 == 2)] = -1
    assert set(np.unique(data)) == {-1, 0, 100} and m4.shape[0] != m4.shape[1]
    maps[5][9, 4:7] = (1, 1, 0)  # the goal (9, 4) on an obstacle; the nearest free cell of its row is (9, 6), unless (9, 3) or (9, 2) is free
    return [(maps[0], (1, 1), (14, 14), 0, 1),
            (maps[1], (0, 1), (4, 6), 1, 1),
            (maps[2], (2, 2), (18, 20), 0, 0),
            (maps[3], (1, 1), (22, 15), 2, 0),
            ((data.reshape(-1), m4.shape[0], m4.shape[1]), (-3, 2), (11, 19), 1, 0),
            (maps[5], (1, 1), (9, 4), 0, 1)]


def plain_jobs(F, first_slot):
    return [(first_slot + k,) + tuple(f) for k, f in enumerate(F)]


def world_jobs(F, first_slot):
    pos = lambda c: (c[0] + (0.5 if c[0] >= 0 else -0.5), c[1] + (0.5 if c[1] >= 0 else -0.5))
    return [(first_slot + k, raw, (0.0, 0.0), 1.0, pos(s), pos(g), ifa, v) for k, (raw, s, g, ifa, v) in enumerate(F)]


def slot_state(p, slot):
    return p.get_grid_slot(slot).tobytes(), {k: v.tobytes() for k, v in p.debug_slot_maps(slot).items()}


def single_state(single, f):
    raw, s, g, ifa, v = f
    out = single.prepare_occupancy_msg(raw[0], raw[1], raw[2], s, g, ifa, v) if isinstance(raw, tuple) else single.prepare_grid(raw, s, g, ifa, v)
    return out, (single.get_grid().tobytes(), {k: m.tobytes() for k, m in single.debug_maps().items()})


def same_as(p, first_slot, want, tag):
    for k in range(N):
        occ, maps = slot_state(p, first_slot + k)
        assert occ == want[k][0], (tag, k, "occ")
        assert set(maps) == set(want[k][1]) and len(maps) == 6, (tag, k)
        for name in maps:
            assert maps[name] == want[k][1][name], (tag, k, name)


def test_four_entry_points_one_result(planner, single):
    F = fleet()
    # 1. prepare_slots: the yardstick of every later call
    outs = planner.prepare_slots(plain_jobs(F, 0))
    assert all(o[5] for o in outs), outs
    shapes = [o[3] for o in outs]
    assert shapes[0] == (16, 16) and shapes[1] == (11, 13) and shapes[2] == (20, 23) and shapes[3] == (36, 29), shapes
    assert outs[4][2][0] == 5 and outs[5][1][0] == 9 and outs[5][1][1] != 4, outs  # the padding of x = -3 at ifa 1; the goal moved along its row
    want = [slot_state(planner, k) for k in range(N)]
    # ... which is the single-grid path's result, output for output and byte for byte
    for k, f in enumerate(F):
        o1, st1 = single_state(single, f)
        assert o1 == outs[k][:5], (k, o1, outs[k])
        assert st1[0] == want[k][0], (k, "occ")
        for name in st1[1]:
            assert st1[1][name] == want[k][1][name], (k, name)
    # 2. refresh_slots on empty slots: everything is built
    r = planner.refresh_slots(plain_jobs(F, 6))
    assert [o[:6] for o in r] == outs and [o[6] for o in r] == [False] * N, r
    same_as(planner, 6, want, "refresh, empty slots")
    # 3. ... again: everything is kept
    r = planner.refresh_slots(plain_jobs(F, 6))
    assert [o[:6] for o in r] == outs and [o[6] for o in r] == [True] * N, r
    same_as(planner, 6, want, "refresh, unchanged")
    # 4. one byte of one raw flipped: that job alone is built; the yardstick is prepare_slots with the same jobs
    raw = F[FLIP][0].copy()
    raw[3, 4] ^= 1
    F2 = list(F)
    F2[FLIP] = (raw,) + tuple(F[FLIP][1:])
    outs2 = planner.prepare_slots(plain_jobs(F2, 24))
    want2 = [slot_state(planner, 24 + k) for k in range(N)]
    assert all(o[5] for o in outs2) and want2[FLIP][0] != want[FLIP][0]
    assert [w for k, w in enumerate(want2) if k != FLIP] == [w for k, w in enumerate(want) if k != FLIP]
    o1, st1 = single_state(single, F2[FLIP])
    assert o1 == outs2[FLIP][:5] and st1 == want2[FLIP]
    r = planner.refresh_slots(plain_jobs(F2, 6))
    assert [o[:6] for o in r] == outs2 and [o[6] for o in r] == [k != FLIP for k in range(N)], r
    same_as(planner, 6, want2, "refresh, one raw flipped")
    # 5. prepare_slots_world
    w = planner.prepare_slots_world(world_jobs(F, 12))
    assert [o[:6] for o in w] == outs, (w, outs)
    same_as(planner, 12, want, "world prepare")
    # 6. refresh_slots_world, twice
    for kept in (False, True):
        w = planner.refresh_slots_world(world_jobs(F, 18))
        assert [o[:6] for o in w] == outs and [o[6] for o in w] == [kept] * N, (kept, w)
        same_as(planner, 18, want, ("world refresh", kept))
