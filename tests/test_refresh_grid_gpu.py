"""GPU suite (-m gpu): fxjps_refresh_grid / fxjps_refresh_occupancy_msg / fxjps_replan_frame_raw.

The yardstick is a twin handle that runs prepare_grid (which always builds) on the same arguments after every step: the
resident grid, the derived maps and every output of the refreshing handle equal the twin's byte for byte -- the component
forest as tests/test_map_updates_gpu.py compares it after any cell update (it must keep together what the fresh labels
keep together; byte for byte where the whole build ran).  The list of fxjps_last_refresh_cells equals np.argwhere of
(resident bytes read before the call != the prepared grid of oracle/gridprep.py), in order, with the values.  The steps
and their modes are those of tests/refresh_grid_cases.py (checked on the host by tests/test_refresh_grid_host.py).

The frame call: offsets, lengths, costs and cells of every tick equal a fresh handle's prepare_grid + plan_batch and the
CPU oracle's; the number of stored results handed back is what oracle.read_sets.replan_reuse says when it is fed the
device's own bitmaps, the host diff list and the stored status, all read before the frame.  WHICH queries were searched
has no accessor: the library reports the count (fxjps_timing_t.reused), and the per-query diagnostics of FXJPS_QSTAT are
not written by every launch (the head launch of the longest queries leaves them out), so they cannot serve as one.  The
tests therefore pin the count to the rule's, the rule's answer for the near and the far queries, and every byte of the
result to a fresh handle's: a wrong selection with the right count would hand back a stale path and show there."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import refresh_grid_cases as rc
from oracle import gridprep
from oracle import read_sets as rs
from test_gpu_fullsize import assert_same, oracle_csr
from test_map_updates_gpu import roots

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MPL = 8192
MAPS = ("nb8", "bm", "ci", "dbm", "jd")


@pytest.fixture(scope="module")
def pair():
    import fuxi_planner_amd as fx
    p, q = fx.Planner([0]), fx.Planner([0])
    yield p, q
    p.close()
    q.close()


def same_state(p, q, tag, whole_build, contexts=1):
    gq = q.get_grid()
    for c in range(contexts):
        assert np.array_equal(p.get_grid(c), gq), (tag, "grid of context %d" % c)
    a, b = p.debug_maps(), q.debug_maps()
    for k in MAPS:
        assert np.array_equal(a[k], b[k]), (tag, k, int((a[k] != b[k]).sum()))
    assert np.array_equal(p.debug_nbmask(), q.debug_nbmask()), tag
    if whole_build:
        assert np.array_equal(a["comp"], b["comp"]), (tag, "comp")
    free = np.flatnonzero(gq.ravel() == 0)
    ra, rb = roots(a["comp"])[free], roots(b["comp"])[free]
    assert (ra >= 0).all() and (rb >= 0).all(), tag
    pairs = np.unique(np.stack([rb, ra]), axis=1)
    assert pairs.shape[1] == len(np.unique(rb)), (tag, "a fresh component is split over several roots")


def do_pre(p, pre, resident):
    """A step's `pre` on the device; -> the bytes the host expects to be resident afterwards."""
    want = rc.apply_pre(resident, pre)
    if pre[0] == "poke":
        idx = np.asarray(pre[1], np.int64)
        H = resident.shape[1]
        p.update_cells(np.stack([idx // H, idx % H], 1).astype(np.int32), want.flat[idx].astype(np.uint8), rebuild=not pre[2])
    else:
        p.set_grid_occ(want)
    return want


def call(planner, refresh, layout, st, ifa, variant, seed):
    raw = st["raw"]
    if layout == 0:
        fn = planner.refresh_grid if refresh else planner.prepare_grid
        return fn(raw.astype(np.uint8), st["start"], st["goal"], ifa, variant)
    fn = planner.refresh_occupancy_msg if refresh else planner.prepare_occupancy_msg
    return fn(rc.to_msg(raw, seed), raw.shape[0], raw.shape[1], st["start"], st["goal"], ifa, variant)


def run_steps(p, q, case, layout, contexts=1):
    W0, H0, ifa, variant = case
    resident = None
    for k, st in enumerate(rc.steps(*case)):
        tag = (case, layout, st["name"])
        if st["pre"] is not None:
            resident = do_pre(p, st["pre"], resident)
        if resident is not None:
            assert np.array_equal(p.get_grid(), resident), tag  # (behind a deferred update as well: the read is ordered behind it)
        grid, s, g, md, eo, cells, vals, n, mode = rc.simulate(resident, st["raw"], st["start"], st["goal"], ifa, variant)
        out = call(p, True, layout, st, ifa, variant, k)
        want = call(q, False, layout, st, ifa, variant, k)
        assert want == (s, g, md, grid.shape, eo), tag
        assert out[:5] == want, (tag, out, want)
        assert out[5:] == (n, mode), (tag, out[5:], (n, mode))
        assert st["mode"] in (None, mode), tag
        xy, val = p.last_refresh_cells()
        if mode == 1:
            assert np.array_equal(xy, cells) and np.array_equal(val, vals), tag
        else:
            assert len(xy) == 0 and len(val) == 0, tag
        assert np.array_equal(q.get_grid(), grid), tag
        same_state(p, q, tag, mode == 2, contexts)
        resident = grid


@pytest.mark.parametrize("layout", (0, 1), ids=("matrix", "message"))
@pytest.mark.parametrize("case", rc.CASES, ids=lambda c: "%dx%d-ifa%d-%s" % (c[0], c[1], c[2], ("st", "ccst")[c[3]]))
def test_refresh_equals_prepare_step_by_step(pair, case, layout):
    p, q = pair
    p.set_grid_occ(np.zeros((3, 3), np.uint8))  # (another case's grid: the first step finds other extents or none to compare)
    run_steps(p, q, case, layout)


@pytest.mark.parametrize("shape", rc.SHAPES, ids=lambda c: "%dx%d" % c)
def test_ifa_0_with_the_st_variant_against_the_twin(pair, shape):
    """The reference raises at ifa 0 in the st variant (a range with step 0), so oracle.gridprep has no answer; the library
    defines it (no dilation, the st shift).  Here the twin's prepare_grid alone is the yardstick: grid, maps, outputs, and
    the list against np.argwhere of (resident bytes before != the twin's grid)."""
    p, q = pair
    W0, H0 = shape
    rng = np.random.default_rng(W0)
    R = (rng.random((W0, H0)) < 0.2).astype(np.uint8)
    R[0, 0] = R[-1, -1] = R[W0 - 3, H0 - 3] = 0
    R[1, 2] = 1
    start, goal = (1, 1), (W0 - 2, H0 - 2)
    n = W0 * H0
    a = rc.BLOCK - 1 if n > rc.BLOCK + 1 else n // 2
    p.set_grid_occ(np.zeros((3, 3), np.uint8))
    steps = [("other extents", None, goal, 2), ("the same raw", None, goal, 0), ("the raw's first cell", (0, 0), goal, 1),
             ("the raw's last cell", (W0 - 1, H0 - 1), goal, 1), ("two resident cells", "poke", goal, 1),
             ("the goal moved onto an obstacle", None, (2, 3), 0), ("the raw inverted", "invert", goal, None)]
    for name, what, g, mode in steps:
        if what == "poke":
            xy = np.array([[a // H0, a % H0], [(a + 1) // H0, (a + 1) % H0]], np.int32)
            p.update_cells(xy, 1 - p.get_grid()[xy[:, 0], xy[:, 1]])
        elif what == "invert":
            R = 1 - R
            R[W0 - 3, 0] = 0  # (a free cell in the goal's row)
        elif what is not None:
            R[what] ^= 1
        before = p.get_grid()
        out = p.refresh_grid(R, start, g, 0, 0)
        want = q.prepare_grid(R, start, g, 0, 0)
        assert out[:5] == want, (shape, name, out, want)
        new = q.get_grid()
        if before.shape != new.shape:
            cells, cnt, m = np.zeros((0, 2), np.int64), -1, 2
        else:
            cells = np.argwhere(before != new)
            cnt = len(cells)
            m = 0 if cnt == 0 else 1 if cnt <= rc.capacity(*new.shape) else 2
        assert out[5:] == (cnt, m) and mode in (None, m), (shape, name, out[5:], (cnt, m))
        if name == "the goal moved onto an obstacle":
            assert out[4] == 1 and out[1] != (1, 2), out
        xy, val = p.last_refresh_cells()
        if m == 1:
            assert np.array_equal(xy, cells) and np.array_equal(val, new[cells[:, 0], cells[:, 1]]), (shape, name)
        else:
            assert len(val) == 0, (shape, name)
        same_state(p, q, (shape, name), m == 2)


def test_two_contexts(pair):
    import fuxi_planner_amd as fx
    _, q = pair
    with fx.Planner([0, 0]) as p2:
        run_steps(p2, q, (70, 37, 1, 1), 0, contexts=2)
        run_steps(p2, q, (300, 300, 2, 0), 1, contexts=2)


def test_refusals_touch_nothing(pair, oracle):
    """Every refusal of prepare_grid that comes before its build, and the frame call's own: the grid, the maps, the list of
    the last refresh and the stored results of replan_frame are what they were."""
    from fuxi_planner_amd import _lib
    p, q = pair
    case = (70, 37, 1, 1)
    st = rc.steps(*case)[3]
    q.prepare_grid(st["raw"].astype(np.uint8), st["start"], st["goal"], 1, 1)
    grid = q.get_grid()
    c = np.argwhere(grid == 0)[40]
    p.prepare_grid(st["raw"].astype(np.uint8), st["start"], st["goal"], 1, 1)
    p.update_cells(c[None].astype(np.int32), np.array([1], np.uint8))
    out = p.refresh_grid(st["raw"].astype(np.uint8), st["start"], st["goal"], 1, 1)
    assert out[5:] == (1, 1)
    free = np.argwhere(grid == 0)
    s, g = free[::97][:8].astype(np.int32), free[::-89][:8].astype(np.int32)
    p.set_queries(s, g, 2, MPL)
    res = p.replan_frame()
    assert_same(res, oracle_csr(oracle, grid, s, g, 2, MPL))
    L, h = p._L, p._h
    raw = np.ascontiguousarray(st["raw"].astype(np.uint8))
    W, H, eo, mode, ch = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int32(), C.c_int64()
    md = (C.c_int32 * 2)()
    bad = [dict(variant=2), dict(ifa=-1), dict(ifa=65), dict(W0=0), dict(H0=0), dict(raw=None), dict(start=None), dict(goal=None),
           dict(goal=(9000, 5)), dict(start=(5, -9000))]
    for kw in bad:
        a = dict(raw=_lib.ptr(raw, C.c_uint8), W0=70, H0=37, ifa=1, variant=1, start=(1, 1), goal=(68, 35))
        a.update(kw)
        sv = None if a["start"] is None else (C.c_int32 * 2)(*a["start"])
        gv = None if a["goal"] is None else (C.c_int32 * 2)(*a["goal"])
        outs = (sv, gv, C.byref(W), C.byref(H), md, C.byref(eo), C.byref(ch), C.byref(mode))
        for fn in (L.fxjps_refresh_grid, L.fxjps_refresh_occupancy_msg):
            rcode = fn(h, C.cast(a["raw"], fn.argtypes[1]), a["W0"], a["H0"], a["ifa"], a["variant"], *outs)
            assert rcode == _lib.E_ARG, (kw, rcode)
        rcode = L.fxjps_replan_frame_raw(h, C.cast(a["raw"], C.c_void_p), 0, a["W0"], a["H0"], a["ifa"], a["variant"], *outs,
                                         None, None, 0, None, None, None)
        assert rcode == _lib.E_ARG, (kw, rcode)
        if sv is not None and gv is not None:
            assert tuple(sv) == tuple(a["start"]) and tuple(gv) == tuple(a["goal"]), kw
    xy, val = p.last_refresh_cells()
    assert xy.tolist() == [c.tolist()] and val.tolist() == [0]
    same_state(p, q, "after the refusals", False)
    again = p.replan_frame()  # (the stored results are still there: every query with a path is handed back)
    assert_same(again, res)
    assert p.timing()["reused"] == int((res[3] > 0).sum()) > 0
    # the frame call without stored queries
    import fuxi_planner_amd as fx
    with fx.Planner([0]) as fresh:
        fresh.prepare_grid(st["raw"].astype(np.uint8), st["start"], st["goal"], 1, 1)
        with pytest.raises(fx.FxjpsError, match="fxjps_prepare_grid and fxjps_set_queries again") as e:
            fresh.replan_frame_raw(st["raw"].astype(np.uint8), st["start"], st["goal"], 1, 1)
        assert e.value.code == _lib.E_ARG


# ------------------------------------------------------------------ the frame call
def frame_scene(oracle):
    """A 128 x 128 / 20 % raw, ifa 1 (the prepared grid is 78 % occupied: paths are local), three raw cells changed inside
    one small window, and 8 queries of the prepared grid: for some of them every cell the reference reads is at least 24
    cells (six read-set tiles of 4 cells; the dilation reaches 1) from every changed prepared cell, for some the reference
    reads a changed cell.  The window is put where the reference reads: three free cells of one query's read set."""
    from fuxi_planner_amd import synth
    raw0 = synth.synth_grid(128, 128, 11, 0.20) > 0
    start, goal, ifa, variant = (2, 2), (125, 125), 1, 1
    g0 = gridprep.prepare_full(raw0.astype(np.uint8), start, goal, ifa, variant)[0]
    W, H = g0.shape
    rng = np.random.default_rng(12)
    free = np.argwhere(g0 == 0)
    s = free[rng.integers(0, len(free), 400)].astype(np.int32)
    near_s = [free[np.abs(free - c).max(1) <= 6] for c in s]
    g = np.array([c[rng.integers(0, len(c))] for c in near_s], np.int32)
    bits, ost = oracle.read_sets(g0, s, g, 2, nthreads=16)
    masks = {i: oracle.unpack_read_set(bits[i], W, H) for i in range(len(s)) if ost[i] >= 3}
    # the anchor: the first query with a path of three jump points or more whose reads hold three free cells over raw cells
    raw1 = None
    for i, m in masks.items():
        c = np.argwhere(m & (g0 == 0))
        c = c[(c >= 2).all(1) & (c < 130).all(1) & (np.abs(c - s[i]).max(1) >= 2) & (np.abs(c - g[i]).max(1) >= 2)]  # (the dilation must not reach its start or goal)
        if len(c) >= 3:
            raw1 = raw0.copy()
            for x, y in c[[0, len(c) // 2, -1]]:
                raw1[x - 2, y - 2] = True  # (map_d is (2, 2))
            break
    assert raw1 is not None and (raw1 != raw0).sum() == 3
    g1 = gridprep.prepare_full(raw1.astype(np.uint8), start, goal, ifa, variant)[0]
    D = np.argwhere(g0 != g1)
    assert 3 <= len(D) <= 27 and np.ptp(D, 0).max() < 16
    dmask = np.zeros((W, H), bool)
    dmask[D[:, 0], D[:, 1]] = True
    near, far = [], []
    for i, m in masks.items():
        if g1[s[i, 0], s[i, 1]] or g1[g[i, 0], g[i, 1]]:
            continue
        xs, ys = np.nonzero(m)
        if (m & dmask).any():
            near.append(i)
        elif np.maximum(np.abs(xs[:, None] - D[None, :, 0]), np.abs(ys[:, None] - D[None, :, 1])).min() >= 24:
            far.append(i)
    assert len(near) >= 1 and len(far) >= 5, (near, far)
    near = near[:3]
    pick = near + far[:8 - len(near)]
    return dict(raw0=raw0, raw1=raw1, g0=g0, g1=g1, D=D, s=s[pick], g=g[pick], near=list(range(len(near))),
                far=list(range(len(near), len(pick))), args=(start, goal, ifa, variant))


def fresh_result(q, raw, args, s, g):
    q.prepare_grid(raw.astype(np.uint8), *args)
    return q.plan_batch(s, g, 2, MPL)


def test_frames_from_raw_maps(pair, oracle):
    import fuxi_planner_amd as fx
    p, q = pair
    sc = frame_scene(oracle)
    s, g, args = sc["s"], sc["g"], sc["args"]
    W, H = sc["g0"].shape
    # tick 1
    prep = p.prepare_grid(sc["raw0"].astype(np.uint8), *args)
    p.set_queries(s, g, 2, MPL)
    res = p.replan_frame()
    assert_same(res, oracle_csr(oracle, sc["g0"], s, g, 2, MPL))
    assert_same(res, fresh_result(q, sc["raw0"], args, s, g))
    assert (res[3][sc["near"] + sc["far"]] > 0).all()
    # tick 2: three raw cells changed
    b, tsh = p.debug_read_sets()
    assert tsh == rs.tile_shift(W, H) == 2
    track, want = rs.replan_reuse(b, res[3], sc["D"], W, H)
    assert track and not want[sc["near"]].any(), want  # (a query that reads a changed cell is searched)
    assert want[sc["far"]].all(), want                  # (a query that reads nothing near the window is not)
    out = p.replan_frame_raw(sc["raw1"].astype(np.uint8), *args)
    res = out[:4]
    assert out[4:9] == prep and out[9:] == (len(sc["D"]), 1), out[4:]
    assert p.timing()["reused"] == int(want.sum())
    xy, val = p.last_refresh_cells()
    assert np.array_equal(xy, sc["D"]) and np.array_equal(val, sc["g1"][sc["D"][:, 0], sc["D"][:, 1]])
    assert_same(res, oracle_csr(oracle, sc["g1"], s, g, 2, MPL))
    assert_same(res, fresh_result(q, sc["raw1"], args, s, g))
    same_state(p, q, "frame with three raw cells changed", False)
    # tick 3: the same raw again, as a message
    b, _ = p.debug_read_sets()
    track, want = rs.replan_reuse(b, res[3], np.zeros((0, 2), np.int64), W, H)
    assert track and np.array_equal(want, res[3] > 0)
    out = p.replan_frame_raw(rc.to_msg(sc["raw1"], 3).reshape(128, 128), *args)
    assert out[4:9] == prep and out[9:] == (0, 0)
    assert p.timing()["reused"] == int(want.sum()) == int((res[3] > 0).sum())
    assert_same(out[:4], res)
    assert len(p.last_refresh_cells()[1]) == 0
    # tick 4: other extents are refused, the stored results survive
    with pytest.raises(fx.FxjpsError, match="fxjps_prepare_grid and fxjps_set_queries again"):
        p.replan_frame_raw(sc["raw1"].astype(np.uint8), args[0], (130, 125), args[2], args[3])
    again = p.replan_frame()
    assert_same(again, res)
    assert p.timing()["reused"] == int((res[3] > 0).sum())
    # tick 5: more changed cells than the list holds -- the whole build, every query searched
    from fuxi_planner_amd import synth
    raw2 = synth.synth_grid(128, 128, 12, 0.20) > 0
    raw2[1:4, 1:4] = False
    g2, _, _, _, _, _, _, n, mode = rc.simulate(sc["g1"], raw2, args[0], args[1], args[2], args[3])
    assert mode == 2 and n > rc.capacity(W, H)
    out = p.replan_frame_raw(raw2.astype(np.uint8), *args)
    assert out[9:] == (n, 2) and p.timing()["reused"] == 0
    assert_same(out[:4], oracle_csr(oracle, g2, s, g, 2, MPL))
    assert_same(out[:4], fresh_result(q, raw2, args, s, g))
    same_state(p, q, "frame behind a whole build", True)
    # ... it was tracked iff the box of its changed cells touches at most half of the tiles: then the next frame reuses
    d = np.argwhere(sc["g1"] != g2)
    tx = (min(d[:, 0].max() + 1, W - 1) >> 2) - (max(d[:, 0].min() - 1, 0) >> 2) + 1
    ty = (min(d[:, 1].max() + 1, H - 1) >> 2) - (max(d[:, 1].min() - 1, 0) >> 2) + 1
    tracked = 2 * tx * ty <= (((W - 1) >> 2) + 1) * (((H - 1) >> 2) + 1)
    paths = int((out[3] > 0).sum())
    for want in (paths if tracked else 0, paths):
        out2 = p.replan_frame_raw(raw2.astype(np.uint8), *args)
        assert out2[9:] == (0, 0) and p.timing()["reused"] == want
        assert_same(out2[:4], out[:4])


CHILD = r"""
import os, sys
import numpy as np
sys.path.insert(0, os.path.join(%(root)r, "tests"))
sys.path.insert(0, %(root)r)
import fuxi_planner_amd as fx
from oracle import oracle as orc
from oracle import gridprep
from test_gpu_fullsize import assert_same, oracle_csr
from test_refresh_grid_gpu import frame_scene, MPL
orc.build()
sc = frame_scene(orc)
s, g, args = sc["s"], sc["g"], sc["args"]
xy = sc["D"].astype(np.int32)
val = sc["g1"][xy[:, 0], xy[:, 1]]
with fx.Planner([0]) as p:
    def two_frames():
        p.prepare_grid(sc["raw0"].astype(np.uint8), *args)
        p.set_queries(s, g, 2, MPL)
        a = p.replan_frame()
        ra = p.timing()["reused"]
        b = p.replan_frame(xy, val)
        return a, ra, b, p.timing()["reused"]
    a, ra, b, rb = two_frames()
    assert_same(a, oracle_csr(orc, sc["g0"], s, g, 2, MPL))
    assert_same(b, oracle_csr(orc, sc["g1"], s, g, 2, MPL))
    out = p.replan_frame_raw(sc["raw1"].astype(np.uint8), *args)
    assert out[9:] == (0, 0), out[9:]
    assert_same(out[:4], b)
    r_same = p.timing()["reused"]
    out = p.replan_frame_raw(sc["raw0"].astype(np.uint8), *args)
    assert out[9:] == (len(xy), 1), out[9:]
    assert_same(out[:4], a)
    r_back = p.timing()["reused"]
    a2, ra2, b2, rb2 = two_frames()
    assert_same(a2, a)
    assert_same(b2, b)
    assert (ra2, rb2) == (ra, rb)
    print("REUSED", ra, rb, r_same, r_back, int((b[3] > 0).sum()))
"""


def run_child(env):
    e = dict(os.environ)
    e.update(env)
    r = subprocess.run([sys.executable, "-c", CHILD % dict(root=ROOT)], env=e, capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-3000:]
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("REUSED")][-1]
    return [int(v) for v in line.split()[1:]]


def test_reuse_switched_off_in_a_process_of_its_own():
    """FXJPS_REPLAN_REUSE=0 (read once per process): the same bytes, nothing handed back by either frame call."""
    assert run_child({"FXJPS_REPLAN_REUSE": "0"})[:4] == [0, 0, 0, 0]


def test_replan_frame_is_unchanged_around_the_new_calls():
    """A process of its own: replan_frame returns the same bytes and the same reuse counts before and after the new frame
    calls ran on the handle; a frame call on an unchanged raw hands back every stored path."""
    ra, rb, r_same, r_back, paths = run_child({})
    assert ra == 0 and rb > 0 and r_same == paths and r_back > 0
