"""GPU suite (-m gpu): the C ABI's obstacle rule -- "a cell is an obstacle iff its byte is non-zero" (include/fxjps.h) -- at
every reader of an uploaded grid.  fxjps_set_grid, fxjps_set_grid_device, fxjps_set_grid_slot and fxjps_set_prior_map copy
the caller's bytes to the device as they are, and the rest of the suite uploads 0 and 1 only: a reader that tests `== 1`
passes it and sees straight through a wall written as 100 or 255.

Here every call runs on a handle whose occupied cells hold 100, 255, 2, 128 or a random non-zero byte each (`recode`), and
is compared, byte for byte, with (a) the same call on a twin handle that holds ones and (b) a yardstick that never sees
the recoded bytes: oracle.plan_batch / oracle.read_sets, oracle.derived_maps.reference_maps, oracle.adapters and the
one-path host function fxjps_waypoint_ccst, all given the 0 / 1 grid.  No tolerance anywhere.

Shapes: 96 x 80 at 25 %, the 130 x 70 one-door wall of test_door_between_components_and_plans, and 600 x 500 at 20 % (more
than 2^18 cells: fxjps_set_grid waits instead of staging).  The helpers at the top are shared with the CPU suite
(tests/test_grid_bytes_host.py) and need no device."""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import derived_maps as dm
from oracle import read_sets as rs

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MPL = 1024
NTHREADS = 8  # the oracle's threads
MAPS = ("nb8", "bm", "ci", "dbm", "jd")

# ------------------------------------------------------------------ the recodings (host only)
RECODINGS = ("ones", "x100", "xff", "x2", "x128", "mixed")  # "ones" is the control: what the twin handle holds
OTHERS = RECODINGS[1:]
_BYTE = {"ones": 1, "x100": 100, "xff": 255, "x2": 2, "x128": 128}


def recode(g, name, seed=5):
    """The 0 / 1 grid `g` with its occupied cells written as `name` says; the zero cells stay zero.  -> a new uint8 array."""
    g = np.asarray(g)
    assert g.dtype == np.uint8 and ((g == 0) | (g == 1)).all()
    occ = g != 0
    out = np.zeros(g.shape, np.uint8)
    if name != "mixed":
        out[occ] = _BYTE[name]
        return out
    n = int(occ.sum())
    for k in range(4096):  # (a draw without a single 1 -- likely on a grid of a few dozen obstacles -- is drawn again)
        v = np.random.default_rng(seed + 1000 * k).integers(1, 256, n).astype(np.uint8)
        if (v == 1).any() or n == 0:
            break
    out[occ] = v
    if n:
        assert (out[occ] == 1).any() and 2 * int((out[occ] != 1).sum()) > n, "mixed: a 1 among mostly other bytes"
    assert np.array_equal(out != 0, occ)
    return out


def door_grid(opened=False):
    """The 130 x 70 wall with one door of test_door_between_components_and_plans."""
    g = np.zeros((130, 70), np.uint8)
    g[65, :] = 1
    if opened:
        g[65, 33] = 0
    return g


@functools.lru_cache(maxsize=None)
def grid(name):
    from fuxi_planner_amd import synth
    g = {"small": lambda: synth.synth_grid(96, 80, 7, 0.25), "door": door_grid, "door_open": lambda: door_grid(True),
         "large": lambda: synth.synth_grid(600, 500, 9, 0.20), "second": lambda: synth.synth_grid(128, 96, 4, 0.22),
         "third": lambda: synth.synth_grid(61, 127, 3, 0.30)}[name]()
    g.setflags(write=False)
    return g


def reference_maps(g):
    from oracle import oracle
    return dm.reference_maps(g, table=oracle.jump_table(np.ascontiguousarray(g), flags=True, nthreads=NTHREADS))


@functools.lru_cache(maxsize=None)
def grid_reference(name):
    """reference_maps of grid(name), computed once for the module."""
    return reference_maps(grid(name))


@functools.lru_cache(maxsize=None)
def queries(name, n=300):
    from fuxi_planner_amd import synth
    if name.startswith("door"):  # across the wall, both ways
        rng = np.random.default_rng(79)
        left = np.stack([rng.integers(0, 65, n // 2), rng.integers(0, 70, n // 2)], 1).astype(np.int32)
        right = np.stack([rng.integers(66, 130, n // 2), rng.integers(0, 70, n // 2)], 1).astype(np.int32)
        return np.concatenate([left, right]), np.concatenate([right, left])
    return synth.synth_queries(grid(name), {"small": 7, "second": 4, "third": 3, "large": 9}[name], n)


@functools.lru_cache(maxsize=None)
def oracle_result(name, h=2, n=300):
    """The oracle's plans of queries(name, n) on grid(name), in the planner's CSR layout."""
    from oracle import oracle
    from test_gpu_fullsize import oracle_csr
    s, q = queries(name, n)
    return oracle_csr(oracle, grid(name), s, q, h, MPL, NTHREADS)


# ------------------------------------------------------------------ the waypoint case (host only)
def host_ccst(L, cells, occ, pos, goal, end_occu=0, reso=1.0, origin=(0.0, 0.0)):
    """fxjps_waypoint_ccst of library L on the BYTES of occ (no conversion in between).  -> (wp, goal_out, kept cells)"""
    from fuxi_planner_amd import _lib
    c = np.ascontiguousarray(cells, dtype=np.int32).reshape(-1, 2)
    occ = np.ascontiguousarray(occ, dtype=np.uint8)
    o, p, g = (np.ascontiguousarray(v, dtype=np.float64) for v in (origin, pos, goal))
    wp, gout, kept, nk = np.zeros(3), np.zeros(3), np.zeros((len(c), 2), np.int32), C.c_int32(0)
    rc = L.fxjps_waypoint_ccst(_lib.ptr(c, C.c_int32), len(c), _lib.ptr(occ, C.c_uint8), occ.shape[0], occ.shape[1], float(reso),
                               _lib.ptr(o, C.c_double), _lib.ptr(p, C.c_double), _lib.ptr(g, C.c_double), int(end_occu),
                               _lib.ptr(wp, C.c_double), _lib.ptr(gout, C.c_double), _lib.ptr(kept, C.c_int32), C.byref(nk))
    assert rc == 0, rc
    return wp, gout, kept[:nk.value].copy()


def waypoint_inputs(name, n):
    """Per query of queries(name, n), in the frame reso 1, origin (0, 0): the vehicle 40 cells above its start's point of
    path3 (ccst:487-495: (x + 1, y, 0)), so that the 1.5 distance rule (:507-513) drops nothing; the goal at the goal cell's
    point."""
    s, q = queries(name, n)
    pos = np.c_[s[:, 0] + 1.0, s[:, 1] + 0.0, np.full(len(s), 40.0)]
    goal = np.c_[q[:, 0] + 1.0, q[:, 1] + 0.0, np.full(len(s), 1.5)]
    return pos, goal


def waypoint_case(oracle):
    """synth_grid(96, 80, 7, 0.25) with synth_queries(occ, 7, 300): -> (g, the oracle's paths, pos and goal per path)."""
    off, cells, _, st = oracle_result("small")
    pos, goal = waypoint_inputs("small", 300)
    has = np.flatnonzero(st > 0)
    return grid("small"), [cells[off[q]:off[q + 1]] for q in has], pos[has], goal[has]


@functools.lru_cache(maxsize=None)
def host_waypoints(name, n):
    """The one-path host function on grid(name) (0 / 1) for every query of oracle_result(name, n): the third yardstick.
    -> per query (wp, goal_out, kept cells); a query without a path: (goal, goal, no cells) (ccst:481-485)."""
    from fuxi_planner_amd import _lib
    L = _lib.load()
    off, cells, _, st = oracle_result(name, 2, n)
    pos, goal = waypoint_inputs(name, n)
    none = np.zeros((0, 2), np.int32)
    return [host_ccst(L, cells[off[q]:off[q + 1]], grid(name), pos[q], goal[q]) if st[q] > 0 else (goal[q], goal[q], none) for q in range(len(st))]


# ------------------------------------------------------------------ device helpers
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


def raw_set_slot(p, slot, occ):
    """fxjps_set_grid_slot itself: Planner.set_grid_slot converts its matrix with == 1 first."""
    from fuxi_planner_amd import _lib
    occ = np.ascontiguousarray(occ, dtype=np.uint8)
    p._chk(p._L.fxjps_set_grid_slot(p._h, int(slot), _lib.ptr(occ, C.c_uint8), occ.shape[0], occ.shape[1]))


def raw_set_prior(p, prior, occ):
    """fxjps_set_prior_map itself: Planner.set_prior_map converts its matrix with > 0 first."""
    from fuxi_planner_amd import _lib
    occ = np.ascontiguousarray(occ, dtype=np.uint8)
    p._chk(p._L.fxjps_set_prior_map(p._h, int(prior), _lib.ptr(occ, C.c_uint8), occ.shape[0], occ.shape[1]))


def same_truth(got, g):
    return got.shape == g.shape and np.array_equal(got != 0, np.asarray(g) != 0)


def check_maps(dev, ref, g, tag, exact=True, ever_free=None):
    msg = dm.first_difference(dev, ref)
    assert msg is None, (tag, msg)
    msg = dm.component_problem(dev["comp"], g, exact=exact, ever_free=ever_free)
    assert msg is None, (tag, "comp", msg)


def same_maps(a, b, tag, comp=True):
    for k in MAPS + (("comp",) if comp else ()):
        assert a[k].tobytes() == b[k].tobytes(), (tag, k)


def check_resident(p, twin, g, ref, tag):
    """The resident grid of p (recoded bytes) against the reference of the 0 / 1 grid g and against the twin, which holds g."""
    check_maps(p.debug_maps(), ref, g, tag)
    assert np.array_equal(p.debug_nbmask(), twin.debug_nbmask()), (tag, "nbmask")
    assert same_truth(p.get_grid(), g), (tag, "get_grid")


def assert_csr(a, b, tag):
    for what, x, y in zip(("offsets", "cells", "cost", "status"), a, b):
        assert np.asarray(x).tobytes() == np.asarray(y).tobytes(), (tag, what)


# ------------------------------------------------------------------ 1. upload routes
@pytest.mark.parametrize("name", OTHERS)
def test_upload_routes(planner, twin, oracle, name, monkeypatch):
    """set_grid_occ staged, waiting by request (FXJPS_SETGRID_WAIT=1, read per call) and waiting by size; the raw
    fxjps_set_grid_slot; a handle of two contexts, every context read."""
    import fuxi_planner_amd as fx
    for gname, wait in (("small", False), ("small", True), ("door", False), ("large", False)):
        g, rec = grid(gname), recode(grid(gname), name)
        assert (g.size > 1 << 18) == (gname == "large")
        twin.set_grid_occ(g)
        if wait:
            monkeypatch.setenv("FXJPS_SETGRID_WAIT", "1")
        planner.set_grid_occ(rec)
        monkeypatch.delenv("FXJPS_SETGRID_WAIT", raising=False)
        check_resident(planner, twin, g, grid_reference(gname), (name, gname, wait))
    for slot, gname in ((3, "small"), (200, "door"), (4, "third")):
        raw_set_slot(planner, slot, recode(grid(gname), name))
    for slot, gname in ((3, "small"), (200, "door"), (4, "third")):
        check_maps(planner.debug_slot_maps(slot), grid_reference(gname), grid(gname), (name, "slot", gname))
        assert same_truth(planner.get_grid_slot(slot), grid(gname)), (name, "slot", gname)
    check_resident(planner, twin, grid("large"), grid_reference("large"), (name, "resident beside the slots"))
    for slot in (3, 200, 4):
        planner.clear_grid_slot(slot)
    s, q = queries("small")
    with fx.Planner([0, 0]) as p2:
        p2.set_grid_occ(recode(grid("small"), name))
        raw_set_slot(p2, 1, recode(grid("door"), name))
        for c in range(2):
            assert same_truth(p2.get_grid(c), grid("small")), (name, "context", c)
            occ, maps = p2.debug_slot_context(c, 1)
            assert same_truth(occ, grid("door")), (name, "slot on context", c)
            check_maps(maps, grid_reference("door"), grid("door"), (name, "slot on context", c))
        check_maps(p2.debug_maps(), grid_reference("small"), grid("small"), (name, "two contexts"))
        assert_csr(p2.plan_batch(s, q, 2, MPL), oracle_result("small"), (name, "two contexts"))
        per = [t["queries"] for t in p2.timing_per_context()]
        assert sum(per) == len(s) and min(per) > 0, per  # (both contexts searched their copy)


_DEVICE = r'''
import sys
sys.path.insert(0, %(root)r)
sys.path.insert(0, %(tests)r)
import numpy as np
import torch
import fuxi_planner_amd as fx
from test_grid_bytes_gpu import OTHERS, check_resident, grid, grid_reference, recode
with fx.Planner([0]) as p, fx.Planner([0]) as twin:
    for gname, names in (("small", OTHERS), ("large", ("x100",))):
        g = grid(gname)
        twin.set_grid_occ(g)
        for name in names:
            rec = recode(g, name)
            buf = torch.from_numpy(rec.reshape(-1).copy()).to("cuda:0")
            torch.cuda.synchronize()
            p.set_grid_device(buf.data_ptr(), g.shape[0], g.shape[1])
            check_resident(p, twin, g, grid_reference(gname), ("device", gname, name))
            del buf
print("DEVICE-BYTES-OK")
'''


def test_upload_from_a_device_buffer(tmp_path):
    """fxjps_set_grid_device from a torch uint8 buffer (a process of its own: torch's HIP runtime initialises first)."""
    pytest.importorskip("torch")
    script = tmp_path / "device_bytes.py"
    script.write_text(_DEVICE % {"root": ROOT, "tests": os.path.join(ROOT, "tests")})
    r = subprocess.run([sys.executable, str(script)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "DEVICE-BYTES-OK" in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])


# ------------------------------------------------------------------ 2. search
def slots_case():
    """Three slots of different shapes and a batch interleaved over them at random, every slot's queries in their own
    order.  -> ({slot: grid name}, ids, starts, goals)"""
    names = {0: "small", 7: "door_open", 255: "third"}
    ids = np.repeat(np.array(list(names), np.int32), 120)[np.random.default_rng(17).permutation(360)]
    S, Q = np.zeros((360, 2), np.int32), np.zeros((360, 2), np.int32)
    for k, gname in names.items():
        S[ids == k], Q[ids == k] = queries(gname, 120)
    return names, ids, S, Q


def check_slots_batch(res, names, ids, tag):
    from test_grid_slots_gpu import subset
    for k, gname in names.items():
        assert_csr(subset(res, np.flatnonzero(ids == k)), oracle_result(gname, 2, 120), (tag, "slot", k))


@pytest.mark.parametrize("table", ("direct", "hashed"))
@pytest.mark.parametrize("name", OTHERS)
def test_plan_batch(oracle, name, table, monkeypatch):
    """plan_batch under both heuristics, on the cell-indexed visited table and (FXJPS_DIRECT=0, handles of their own: the
    table is chosen when a handle first plans) on the hashed one."""
    import fuxi_planner_amd as fx
    if table == "hashed":
        monkeypatch.setenv("FXJPS_DIRECT", "0")
    s, q = queries("small")
    with fx.Planner([0]) as p, fx.Planner([0]) as t:
        p.set_grid_occ(recode(grid("small"), name))
        t.set_grid_occ(grid("small"))
        for h in (2, 1):
            res = p.plan_batch(s, q, h, MPL)
            assert p.timing()["table_direct"] == (1 if table == "direct" else 0), (name, table, h)
            assert_csr(res, t.plan_batch(s, q, h, MPL), (name, table, h, "twin"))
            assert_csr(res, oracle_result("small", h), (name, table, h, "oracle"))
        assert (res[3] > 0).sum() > 200


@pytest.mark.parametrize("name", OTHERS)
def test_single_slots_and_streaming_search(planner, twin, oracle, name):
    """plan_one, a slots batch over three recoded slots of different shapes, set_queries + replan_frame and its read sets."""
    g, rec = grid("small"), recode(grid("small"), name)
    s, q = queries("small")
    off, cells, cost, st = oracle_result("small")
    planner.set_grid_occ(rec)
    twin.set_grid_occ(g)
    for k in range(40):
        n, c, path = planner.plan_one(s[k], q[k])
        assert n == st[k] and np.float64(c).tobytes() == cost[k].tobytes() and np.array_equal(path, cells[off[k]:off[k + 1]]), (name, "plan_one", k)
    names, ids, S, Q = slots_case()
    for k, gname in names.items():
        raw_set_slot(planner, k, recode(grid(gname), name))
        twin.set_grid_slot(k, grid(gname))
    res = planner.plan_batch_slots(ids, S, Q, 2, MPL)
    assert_csr(res, twin.plan_batch_slots(ids, S, Q, 2, MPL), (name, "slots batch"))
    check_slots_batch(res, names, ids, name)
    assert all((res[3][ids == k] > 0).sum() > 60 for k in names)
    for k in names:
        planner.clear_grid_slot(k)
        twin.clear_grid_slot(k)
    for p in (planner, twin):
        p.set_queries(s, q, 2, MPL)
    res = planner.replan_frame()
    assert_csr(res, twin.replan_frame(), (name, "replan_frame"))
    assert_csr(res, (off, cells, cost, st), (name, "replan_frame", "oracle"))
    b, tsh = planner.debug_read_sets()
    tb, ttsh = twin.debug_read_sets()
    assert tsh == ttsh == rs.tile_shift(*g.shape) and b.tobytes() == tb.tobytes(), (name, "read sets")
    has = np.flatnonzero(st > 0)[:100]  # ... and they cover what the reference reads on g
    bits, ost = oracle.read_sets(g, s[has], q[has], 2, nthreads=NTHREADS)
    assert np.array_equal(ost, st[has])
    for i, k in enumerate(has):
        assert len(rs.uncovered(oracle.unpack_read_set(bits[i], *g.shape), b[k], *g.shape)) == 0, (name, "read set of query", int(k))


# ------------------------------------------------------------------ 3. cell updates over recoded bytes
def update_script(name):
    """The updates of test_cell_updates over recode(door_grid(), name), host only: -> (the queries across the wall, the list of
    (xy, val, rebuild, tag, door open), the cells of the pool)."""
    W, H, door = 130, 70, (65, 33)
    b = recode(door_grid(), name)
    s, q = queries("door", 80)
    ends = {(int(x), int(y)) for x, y in np.concatenate([s, q])}
    rng = np.random.default_rng(83)
    pool = [c for c in zip(rng.integers(1, W - 1, 200).tolist(), rng.integers(1, H - 1, 200).tolist()) if c[0] not in (64, 65, 66) and c not in ends][:15]
    assert len(pool) == 15
    wall = np.array([(65, y) for y in range(H) if y != door[1]], np.int32)
    script = []

    def add(xy, val, rebuild, tag, is_open):
        xy, val = np.asarray(xy, np.int32).reshape(-1, 2), np.asarray(val).astype(np.uint8)
        assert set(val.tolist()) <= {0, 1, 2, 100, 255}
        for (x, y), v in zip(xy.tolist(), val.tolist()):  # (a cell named several times: the last entry wins)
            b[x, y] = v
        script.append((xy, val, rebuild, tag, is_open))

    # the wall's bytes change, its truth does not (1 -> 255, anything else -> 1); free cells are written 0 again
    old = b[wall[:, 0], wall[:, 1]]
    add(np.concatenate([wall, np.array(pool[:5], np.int32)]), np.concatenate([np.where(old == 1, 255, 1), np.zeros(5)]), True,
        "bytes change, truth does not", False)
    # the door opens; the fifteen cells of the pool are named 40 times with bytes of every kind
    add(np.array([door] + [pool[k] for k in rng.integers(0, 15, 40)], np.int32), np.concatenate([[0], rng.choice([0, 1, 2, 100, 255], 40)]), True,
        "door opened, repeated cells", True)
    # deferred: the door closes with 100, every cell of the pool changes its truth; then a rebuilding entry turns the
    # door's 100 into 1
    now = np.array([b[c] for c in pool])
    assert (now == 0).any() and (now != 0).any() and len(set(now.tolist())) >= 4
    add([door], [100], False, "door closed, deferred", False)
    add(pool, np.where(now != 0, 0, 255), False, "truth flipped, deferred", False)
    add([door], [1], True, "door 100 -> 1 behind two deferred updates", False)
    # the door named twice in one update: occupied, then free
    add([door, door, pool[0]], [2, 0, 100], True, "door 2 then 0 in one update", True)
    assert b[door] == 0
    return (s, q), script, pool


@pytest.mark.parametrize("name", OTHERS)
def test_cell_updates(planner, twin, oracle, name):
    """update_cells, rebuilding and deferred, with bytes of {0, 1, 2, 100, 255}: entries that change a byte but not its
    truth (1 <-> 255 and the like on the wall), entries that change it either way, cells named several times (the last
    entry wins), the door opened and closed."""
    from test_gpu_parity import gpu_vs_oracle
    W, H = 130, 70
    (s, q), script, _ = update_script(name)
    bytes_ = recode(door_grid(), name)
    planner.set_grid_occ(bytes_)
    twin.set_grid_occ(door_grid())
    ever_free = bytes_ == 0
    checked = 0
    for xy, val, rebuild, tag, is_open in script:
        for (x, y), v in zip(xy.tolist(), val.tolist()):
            bytes_[x, y] = v
        ever_free |= bytes_ == 0
        planner.update_cells(xy, val, rebuild=rebuild)
        twin.update_cells(xy, (val != 0).astype(np.uint8), rebuild=rebuild)
        if not rebuild:
            continue
        cur = (bytes_ != 0).astype(np.uint8)
        dev = planner.debug_maps()
        check_maps(dev, reference_maps(cur), cur, (name, tag), exact=False, ever_free=ever_free)
        same_maps(dev, twin.debug_maps(), (name, tag, "twin"), comp=False)
        assert np.array_equal(planner.debug_nbmask(), twin.debug_nbmask()), (name, tag, "nbmask")
        assert same_truth(planner.get_grid(), cur), (name, tag, "get_grid")
        _, _, _, st = gpu_vs_oracle(planner, oracle, cur, s, q, 2)
        if is_open:
            r = dm.roots(dev["comp"]).reshape(W, H)
            assert r[0, 0] == r[W - 1, H - 1] >= 0, (name, tag)
        assert ((st > 0) if is_open else (st <= 0)).all(), (name, tag, st)
        checked += 1
    assert checked == 4


# ------------------------------------------------------------------ 4. refresh over recoded bytes
@functools.lru_cache(maxsize=None)
def raw_scene():
    """A raw map whose prepared grid (ifa 1, the ccst variant) leaves room to plan; queries on the prepared grid."""
    from fuxi_planner_amd import synth
    from oracle import gridprep
    raw = synth.synth_grid(90, 74, 21, 0.04)
    args = ((2, 3), (86, 70), 1, 1)
    G = gridprep.prepare_full(raw, *args)[0].astype(np.uint8)
    s, q = synth.synth_queries(G, 21, 120)
    return raw, args, G, s, q


@pytest.mark.parametrize("name", OTHERS)
def test_refresh_over_recoded_bytes(planner, twin, oracle, name):
    """The prepared grid of a raw map is uploaded recoded; refresh_grid with that raw map then leaves what prepare_grid
    leaves on the twin -- whether it compared bytes (every occupied cell differs) or truth (nothing does): the first
    call's (changed, mode) is not pinned.  The second call finds nothing to do, and the frame call hands back the stored
    paths.  The same for a slot: fxjps_set_grid_slot, then refresh_slots twice."""
    from test_gpu_fullsize import oracle_csr
    raw, args, G, s, q = raw_scene()
    want = twin.prepare_grid(raw, *args)
    assert np.array_equal(twin.get_grid(), G) and want[3] == G.shape
    planner.set_grid_occ(recode(G, name))
    planner.set_queries(s, q, 2, MPL)
    res = planner.replan_frame()
    ref = oracle_csr(oracle, G, s, q, 2, MPL, NTHREADS)
    assert_csr(res, ref, (name, "before the refresh"))
    paths = int((ref[3] > 0).sum())
    assert paths > 80
    out = planner.refresh_grid(raw, *args)
    assert out[:5] == want, (name, out, want)
    same_maps(planner.debug_maps(), twin.debug_maps(), (name, "refresh"), comp=False)
    check_maps(planner.debug_maps(), reference_maps(G), G, (name, "refresh"), exact=False, ever_free=G == 0)
    assert np.array_equal(planner.debug_nbmask(), twin.debug_nbmask()) and same_truth(planner.get_grid(), G), name
    out = planner.refresh_grid(raw, *args)
    assert out[:5] == want and out[5:] == (0, 0), (name, out)
    for k in range(3):  # (the first may search: the refresh may have rebuilt the maps; the last searches nothing)
        out = planner.replan_frame_raw(raw, *args)
        assert out[4:9] == want and out[9:] == (0, 0), (name, k, out[4:])
        assert_csr(out[:4], ref, (name, "frame", k))
    assert planner.timing()["reused"] == paths, name  # (a frame that changed nothing searches nothing)
    # the slot form
    job = (5, raw) + args
    twant = twin.prepare_slots([job])
    assert np.array_equal(twin.get_grid_slot(5), G)
    raw_set_slot(planner, 5, recode(G, name))
    for k in range(2):
        out = planner.refresh_slots([job])
        assert [o[:6] for o in out] == twant, (name, k, out)
        assert same_truth(planner.get_grid_slot(5), G), (name, k)
        same_maps(planner.debug_slot_maps(5), twin.debug_slot_maps(5), (name, "slot refresh", k), comp=False)
        check_maps(planner.debug_slot_maps(5), reference_maps(G), G, (name, "slot refresh", k), exact=False, ever_free=G == 0)
    assert out[0][6] is True, (name, "the second refresh_slots keeps the slot")
    planner.clear_grid_slot(5)
    twin.clear_grid_slot(5)


# ------------------------------------------------------------------ 5. prior map
@pytest.mark.parametrize("name", OTHERS)
def test_recoded_prior_map(planner, twin, name):
    """prepare_slots_world over priors uploaded recoded through fxjps_set_prior_map itself: outputs and slots are those of the
    host merge with the 0 / 1 priors (worldprep.merge_host + prepare_slots) and of the same call over the 0 / 1 priors."""
    import fuxi_planner_amd as fx
    from test_refresh_slots_gpu import same_slots
    from test_world_slots_gpu import make_priors, tick, world_fleet
    priors = make_priors()
    wjobs = world_fleet(large=False)
    for k, m in priors.items():
        assert ((m == 0) | (m == 1)).all()
        raw_set_prior(planner, k, recode(m.astype(np.uint8), name, seed=k))
        assert same_truth(planner.get_prior_map(k), m), (name, k)
    outs, _ = tick(planner, twin, wjobs, priors, False, (name, "host merge"))
    assert all(o[5] for o in outs) and sum(len(wj) > 8 for wj in wjobs) >= 7  # (every job succeeds, most have a prior)
    with fx.Planner([0]) as third:
        for k, m in priors.items():
            third.set_prior_map(k, m)
        assert third.prepare_slots_world(wjobs) == outs, name
        same_slots(planner, third, [wj[0] for wj, o in zip(wjobs, outs) if o[5]], (name, "0 / 1 priors"))
    for wj in wjobs:
        planner.clear_grid_slot(wj[0])
        twin.clear_grid_slot(wj[0])
    for k in priors:
        planner.clear_prior_map(k)


# ------------------------------------------------------------------ 6. writers out
@pytest.mark.parametrize("name", OTHERS)
def test_writers_out(planner, twin, name):
    """publish_map, snapshot_image and publish_slots write 100 / 0 and 0 / 255 whatever non-zero byte stands for a wall."""
    from oracle import adapters
    for gname in ("small", "door"):
        g = grid(gname)
        planner.set_grid_occ(recode(g, name))
        twin.set_grid_occ(g)
        d, w, h = planner.publish_map()
        td, tw, th = twin.publish_map()
        ad, aw, ah = adapters.publish_map(g)
        assert (w, h) == (tw, th) == (aw, ah) and d.tobytes() == td.tobytes() == np.ascontiguousarray(ad).tobytes(), (name, gname, "publish_map")
        for ch in (1, 3):
            img = planner.snapshot_image(ch)
            want = np.ascontiguousarray(adapters.snapshot_image(g, ch))
            assert img.shape == want.shape and img.tobytes() == twin.snapshot_image(ch).tobytes() == want.tobytes(), (name, gname, "snapshot", ch)
    slots = {2: "small", 9: "door", 30: "third"}
    for k, gname in slots.items():
        raw_set_slot(planner, k, recode(grid(gname), name))
        twin.set_grid_slot(k, grid(gname))
    order = [9, 2, 30, 2]
    for ch in (1, 3):
        got = planner.publish_slots(order, msg=True, image_channels=ch)
        ref = twin.publish_slots(order, msg=True, image_channels=ch)
        for k, (d, wh, img), (td, twh, timg) in zip(order, got, ref):
            g = grid(slots[k])
            assert wh == twh == g.shape and d.tobytes() == td.tobytes() == np.ascontiguousarray(adapters.publish_map(g)[0]).tobytes(), (name, k, ch)
            assert img.tobytes() == timg.tobytes() == np.ascontiguousarray(adapters.snapshot_image(g, ch)).tobytes(), (name, k, ch)
    for k in slots:
        planner.clear_grid_slot(k)
        twin.clear_grid_slot(k)


# ------------------------------------------------------------------ 7. waypoints
def check_against_host(host, off, wp, gout, nk, kept, tag):
    for k, (w1, g1, k1) in enumerate(host):
        assert nk[k] == len(k1) and np.array_equal(kept[off[k]:off[k] + nk[k]], k1), (tag, "kept cells of path", k)
        assert wp[k].tobytes() == w1.tobytes() and gout[k].tobytes() == g1.tobytes(), (tag, "waypoint of path", k)


@pytest.mark.parametrize("name", OTHERS)
def test_ccst_rule_on_the_resident_grid(planner, twin, oracle, name):
    """select_ccst_batch on the paths the search left on the device and on explicit paths: the line tests see the walls the
    search went around."""
    from fuxi_planner_amd import waypoints
    g, rec = grid("small"), recode(grid("small"), name)
    if name in ("x100", "xff"):
        assert not (rec == 1).any()  # (to an `== 1` reader this map is empty)
    s, q = queries("small")
    ref = oracle_result("small")
    off, cells = ref[0], ref[1]
    pos, goal = waypoint_inputs("small", 300)
    host = host_waypoints("small", 300)
    assert sum(len(k1) > 2 for _, _, k1 in host) >= 200  # (the yardstick alone: 290 paths turn a corner that has to stay)
    outs = []
    for p, occ in ((planner, rec), (twin, g)):
        p.set_grid_occ(occ)
        assert_csr(p.plan_batch(s, q, 2, MPL), ref, (name, "plans"))
        resident = waypoints.select_ccst_batch(p, len(s), 1.0, (0.0, 0.0), pos, goal)
        explicit = waypoints.select_ccst_batch(p, len(s), 1.0, (0.0, 0.0), pos, goal, paths=(off, cells), return_kept=True)
        outs.append(resident + explicit)
    assert (outs[1][2] > 2).sum() >= 200, "control: at least 200 paths keep more than two points"
    for k, (a, b) in enumerate(zip(*outs)):
        assert a.tobytes() == b.tobytes(), (name, "twin", k)
    wp, gout, nk, wp2, gout2, nk2, kept = outs[0]
    assert wp.tobytes() == wp2.tobytes() and gout.tobytes() == gout2.tobytes() and nk.tobytes() == nk2.tobytes(), (name, "resident paths")
    check_against_host(host, off, wp2, gout2, nk2, kept, name)


def merged(names, n):
    """The queries of several grids as one slots batch, slot k holding grid names[k].  -> (ids, starts, goals, (offsets,
    cells) of the oracle's paths, status, pos, goal, the host function's answers)"""
    ids, S, Q, lens, cells, st, pos, goal, host = [], [], [], [], [], [], [], [], []
    for k, gname in enumerate(names):
        s, q = queries(gname, n[k])
        off, c, _, t = oracle_result(gname, 2, n[k])
        a, b = waypoint_inputs(gname, n[k])
        ids += [k] * len(s)
        S.append(s), Q.append(q), lens.append(np.diff(off)), cells.append(c), st.append(t), pos.append(a), goal.append(b)
        host += host_waypoints(gname, n[k])
    off = np.zeros(len(ids) + 1, np.int64)
    off[1:] = np.cumsum(np.concatenate(lens))
    return (np.array(ids, np.int32), np.concatenate(S), np.concatenate(Q), (off, np.concatenate(cells).astype(np.int32).reshape(-1, 2)),
            np.concatenate(st), np.concatenate(pos), np.concatenate(goal), host)


@pytest.mark.parametrize("name", OTHERS)
def test_ccst_rule_over_recoded_slots(planner, twin, oracle, name):
    """select_slots_batch and tick_outputs_slots with the ccst rule, every query against its own recoded slot: waypoint,
    goal, kept cells and the direct path with its count."""
    from fuxi_planner_amd import waypoints
    names, n = ("small", "second", "door_open"), (300, 333, 80)
    ids, S, Q, (off, cells), st, pos, goal, host = merged(names, n)
    nq = len(ids)
    assert sum(len(k1) > 2 for _, _, k1 in host) >= 200
    rule = np.ones(nq, np.int32)
    outs = []
    for p, raw in ((planner, True), (twin, False)):
        p.set_grid_occ(np.zeros((8, 8), np.uint8))  # (no rule may read it)
        for k, gname in enumerate(names):
            if raw:
                raw_set_slot(p, k, recode(grid(gname), name))
            else:
                p.set_grid_slot(k, grid(gname))
        res = p.plan_batch_slots(ids, S, Q, 2, MPL)
        assert res[0].tobytes() == off.tobytes() and res[1].tobytes() == cells.tobytes() and np.array_equal(res[3], st), (name, "plans")
        a = waypoints.select_slots_batch(p, rule, None, 1.0, (0.0, 0.0), pos, goal, paths=(res[0], None), return_kept=True)  # the resident paths
        b = waypoints.select_slots_batch(p, rule, None, 1.0, (0.0, 0.0), pos, goal, grid_ids=ids, paths=(off, cells), return_kept=True)
        c = waypoints.tick_outputs_slots(p, rule, None, 1.0, (0.0, 0.0), pos, goal, (0.0, 0.0), grid_ids=ids, paths=(off, cells), return_kept=True)
        outs.append((a, b, c))
        for k in range(len(names)):
            p.clear_grid_slot(k)
    (a, b, c), (ta, tb, tc) = outs
    assert (tb[4] > 2).sum() >= 200, "control: at least 200 paths keep more than two points"
    for x, y in ((a, ta), (b, tb)):
        assert all(u.tobytes() == v.tobytes() for u, v in zip(x, y)), (name, "select_slots_batch against the twin")
    assert all(u.tobytes() == v.tobytes() for u, v in zip(a, b)), (name, "resident paths")
    for u, v in zip(c, tc):  # (wp, dim, goal, ang, n_kept, point, paths, dir_paths, dir_back, kept)
        if isinstance(u, list):
            assert len(u) == len(v) and all(i.tobytes() == j.tobytes() for i, j in zip(u, v)), (name, "tick outputs against the twin")
        else:
            assert u.tobytes() == v.tobytes(), (name, "tick outputs against the twin")
    for res, kept in ((b, b[5]), (c, c[9])):
        wp, dim, gout, ang, nk = res[:5]
        assert (dim == 3).all() and not ang.any()
        check_against_host(host, off, wp, gout, nk, kept, name)
    dirs = c[7]
    for k, (w1, g1, k1) in enumerate(host):  # the direct path: path4 of the kept cells (ccst:495-521); without a path [pos, wp]
        want = np.c_[k1[:, 0] + 1.0, k1[:, 1] + 0.0, np.zeros(len(k1))] if st[k] > 0 else np.stack([pos[k], w1])
        assert dirs[k].shape == want.shape and dirs[k].tobytes() == np.ascontiguousarray(want).tobytes(), (name, "direct path", k)
