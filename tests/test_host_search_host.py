"""CPU suite: the host search (fuxi-planner_amd/csrc/fxjps_host_search.cpp) against the C oracle, one query at a time.

The host search reads the derived maps in the device layout; here they come from oracle/derived_maps.reference_maps (an
answer the product code had no part in), and every query's length, cells, cost bytes and -- where a search ran -- pops and
pushes must equal oracle.plan_batch(literal=False).  The search kernel does not count the start's push, so neither does
the host search: pushes == reference - 1.  Queries the library answers without a search (start == goal, an occupied or
outside goal, a goal in another component of a free start) report 0 pops and 0 pushes, as the kernel does.

host_search_check.cpp runs the same search with two threads as a stand-alone program under ASan + UBSan.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import exhaustive_cases as ex
from conftest import ROOT, grid_from_bits, load_golden

CSRC = os.path.join(ROOT, "fuxi-planner_amd", "csrc")
HERE = os.path.dirname(os.path.abspath(__file__))
FLAGS = ["-O2", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-Wall", "-pthread"]


@pytest.fixture(scope="module")
def hs(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("host_search") / "libfxjps_host_search_test.so")
    subprocess.check_call(["g++"] + FLAGS + ["-fPIC", "-shared", "-o", so, os.path.join(CSRC, "fxjps_host_search.cpp"),
                                             os.path.join(HERE, "host_search_entry.cpp")])
    L = C.CDLL(so)
    L.fxh_plan_batch.restype = C.c_int
    L.fxh_plan_batch.argtypes = [C.c_void_p] * 3 + [C.c_int32] * 5 + [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_uint64,
                                                                     C.c_int32] + [C.c_void_p] * 5
    return L


def device_maps(occ, dm, nthreads=16):
    """reference_maps of `occ` as the host search reads them: jd rows padded to the device's stride NS."""
    occ = np.ascontiguousarray(np.asarray(occ) != 0, dtype=np.uint8)
    W, H = occ.shape
    L = dm.layout(W, H)
    from oracle import oracle
    m = dm.reference_maps(occ, table=oracle.jump_table(occ, flags=True, nthreads=nthreads))
    jd = np.zeros((L["PW"], L["NS"], 8), np.uint16)
    jd[:, :L["PH"]] = m["jd"]
    return {"W": W, "H": H, "NS": L["NS"], "LINES": L["LINES"], "WORDS": L["WORDS"], "jd": jd, "bm": np.ascontiguousarray(m["bm"]),
            "comp": np.ascontiguousarray(m["comp"], dtype=np.int32)}


def host_plan(hs, M, starts, goals, h, max_len, nthreads=1, max_pops=None):
    starts = np.ascontiguousarray(starts, dtype=np.int32).reshape(-1, 2)
    goals = np.ascontiguousarray(goals, dtype=np.int32).reshape(-1, 2)
    nq = len(starts)
    cells = np.zeros((nq, max_len, 2), np.int32)
    ln, cost = np.zeros(nq, np.int32), np.zeros(nq, np.float64)
    pops, pushes = np.zeros(nq, np.int64), np.zeros(nq, np.int64)
    rc = hs.fxh_plan_batch(M["jd"].ctypes.data, M["bm"].ctypes.data, M["comp"].ctypes.data, M["W"], M["H"], M["NS"], M["LINES"], M["WORDS"],
                           starts.ctypes.data, goals.ctypes.data, nq, h, max_len, 64 * M["W"] * M["H"] + 4096 if max_pops is None else max_pops,
                           nthreads, cells.ctypes.data, ln.ctypes.data, cost.ctypes.data, pops.ctypes.data, pushes.ctypes.data)
    assert rc == 0
    return cells, ln, cost, pops, pushes


def searched_mask(occ, comp, starts, goals):
    """The queries the library searches (run_query): start != goal, goal on the grid and free, and not in another
    component than a free start."""
    W, H = occ.shape
    s, g = np.asarray(starts).reshape(-1, 2), np.asarray(goals).reshape(-1, 2)
    inb = (g[:, 0] >= 0) & (g[:, 1] >= 0) & (g[:, 0] < W) & (g[:, 1] < H)
    gx, gy = np.clip(g[:, 0], 0, W - 1), np.clip(g[:, 1], 0, H - 1)
    m = inb & (occ[gx, gy] == 0) & ~((s[:, 0] == g[:, 0]) & (s[:, 1] == g[:, 1]))
    sfree = occ[s[:, 0], s[:, 1]] == 0
    return m & ~(sfree & (comp[s[:, 0], s[:, 1]] != comp[gx, gy]))


def compare(hs, oracle, dm, occ, starts, goals, h, max_len, where, nthreads=1, M=None):
    """Every query of the batch against the oracle; -> (cells, length, cost, searched mask) of the host search."""
    occ = np.ascontiguousarray(np.asarray(occ) != 0, dtype=np.uint8)
    M = M or device_maps(occ, dm)
    oc, ol, ocost, st = oracle.plan_batch(occ, starts, goals, h, literal=False, max_len=max_len, nthreads=nthreads, want_stats=True)
    cells, ln, cost, pops, pushes = host_plan(hs, M, starts, goals, h, max_len, nthreads)
    srch = searched_mask(occ, M["comp"].reshape(occ.shape), starts, goals)
    bad = np.flatnonzero((ln != ol) | (cost.view(np.uint64) != ocost.view(np.uint64)))
    assert len(bad) == 0, (where, h, int(bad[0]), np.asarray(starts).reshape(-1, 2)[bad[0]].tolist(), np.asarray(goals).reshape(-1, 2)[bad[0]].tolist(),
                           int(ln[bad[0]]), int(ol[bad[0]]), float(cost[bad[0]]), float(ocost[bad[0]]))
    keep = np.arange(max_len)[None, :] < np.maximum(ol, 0)[:, None]
    assert np.array_equal(cells[keep], oc[keep]), (where, h)
    want_pops, want_pushes = np.where(srch, st["pops"], 0), np.where(srch, st["pushes"] - 1, 0)
    assert np.array_equal(pops, want_pops) and np.array_equal(pushes, want_pushes), (
        where, h, np.flatnonzero((pops != want_pops) | (pushes != want_pushes))[:4].tolist())
    return cells, ln, cost, srch


@pytest.fixture(scope="module")
def dm():
    from oracle import derived_maps
    return derived_maps


@pytest.mark.parametrize("W,H,chunk", [c[1:] for c in ex.case_ids()], ids=[c[0] for c in ex.case_ids()])
def test_exhaustive_small_grids(hs, oracle, dm, W, H, chunk):
    """Every grid of the shape, every start, every goal (the ring outside the grid included), both heuristics: the oracle's
    result, and the digest of the reference's own results in tests/golden/exhaustive.npz."""
    arrays, _ = ex.load_fixture()
    s, g = ex.queries(W, H)
    for b in ex.chunk_blocks(W, H, chunk):
        maps = [device_maps(ex.grid(W, H, c), dm, nthreads=1) for c in ex.block_codes(W, H, b)]
        for h in ex.HCHOICES:
            got = []
            for c, M in zip(ex.block_codes(W, H, b), maps):
                occ = ex.grid(W, H, c)
                cells, ln, cost, _ = compare(hs, oracle, dm, occ, s, g, h, ex.MAX_LEN, "%dx%d grid %d" % (W, H, c), M=M)
                got.append((ln, ex.padded_to_csr(cells, ln), cost))
            assert ex.result_digest(got) == int(arrays[ex.array_name("r", W, H, h)][b]), (W, H, b, h)


def test_structured_goldens(hs, oracle, dm):
    """The map families captured from jps1.py (families.json), random_small.json and known_answers.json: the records' own
    paths and cost bits, and the oracle on the same queries."""
    n = 0
    groups = [(f["family"], grid_from_bits(f["grid_bits"], f["shape"]), f["records"]) for f in load_golden("families.json")["families"]]
    groups += [("random_small %d" % i, grid_from_bits(r["grid_bits"], r["shape"]), [r]) for i, r in enumerate(load_golden("random_small.json"))]
    groups += [("known %d" % i, (np.array(r["grid"], dtype=np.float64).reshape(r["shape"]) == 1).astype(np.uint8), [r])
               for i, r in enumerate(load_golden("known_answers.json")) if not r.get("raises")]
    for name, grid, recs in groups:
        W, H = grid.shape
        M = device_maps(grid, dm)
        mpl = W * H + 1
        for h in (1, 2):
            rs = [r for r in recs if r["hchoice"] == h]
            if not rs:
                continue
            s, g = [r["start"] for r in rs], [r["goal"] for r in rs]
            cells, ln, cost, _ = compare(hs, oracle, dm, grid, s, g, h, mpl, name, M=M)
            for q, r in enumerate(rs):
                if r["path"] is None:
                    assert ln[q] == 0, (name, r["start"], r["goal"])
                else:
                    assert cells[q, :ln[q]].reshape(-1).tolist() == r["path"], (name, r["start"], r["goal"])
                    if r["start"] != r["goal"]:
                        assert float(cost[q]).hex() == r["cost_hex"], (name, r["start"], r["goal"])
                n += 1
    assert n >= 268 + 400


def test_reference_maps_png(hs, oracle, dm, map_grids):
    """The 35 maps of maps_png.npz: the recorded queries, and 64 random ones per map and heuristic."""
    recs = load_golden("maps_png.json")
    assert len({r["map"] for r in recs}) == 35
    rng = np.random.default_rng(35)
    done = {}
    for rec in recs:
        bits = np.unpackbits(map_grids[rec["map"]])
        if "canvas" in rec:
            occ = np.zeros((256, 256), dtype=np.uint8)
            occ[:147, :112] = bits[:147 * 112].reshape(147, 112)
        else:
            W, H = rec["shape"]
            occ = bits[:W * H].reshape(W, H)
        key = (rec["map"], "canvas" in rec)
        if key not in done:
            done[key] = device_maps(occ, dm)
            W, H = occ.shape
            s = np.stack([rng.integers(0, W, 64), rng.integers(0, H, 64)], -1)
            g = np.stack([rng.integers(0, W, 64), rng.integers(0, H, 64)], -1)
            for h in (1, 2):
                compare(hs, oracle, dm, occ, s, g, h, 1024, rec["map"], nthreads=4, M=done[key])
        M = done[key]
        cells, ln, cost, _, _ = host_plan(hs, M, [rec["start"]], [rec["goal"]], rec["hchoice"], 4096)
        if rec["path"] is None:
            assert ln[0] == 0, rec["map"]
        else:
            assert cells[0, :ln[0]].reshape(-1).tolist() == rec["path"], rec["map"]
            if rec["start"] != rec["goal"]:
                assert float(cost[0]).hex() == rec["cost_hex"], rec["map"]


def special_queries(occ, rng):
    """start == goal on an obstacle, an occupied goal, an unreachable goal (a sealed cell), goals outside the grid."""
    W, H = occ.shape
    ox, oy = np.argwhere(occ != 0)[0] if occ.any() else (0, 0)
    fx, fy = np.argwhere(occ == 0)[0]
    s = [[ox, oy], [fx, fy], [fx, fy], [fx, fy], [fx, fy], [ox, oy]]
    g = [[ox, oy], [ox, oy], [W, 0], [-1, H - 1], [fx, fy], [fx, fy]]
    return np.array(s, np.int32), np.array(g, np.int32)


@pytest.mark.parametrize("p", [0.0, 0.2, 0.4])
@pytest.mark.parametrize("h", [1, 2])
def test_random_grids(hs, oracle, dm, p, h):
    rng = np.random.default_rng(int(p * 100) * 7 + h)
    total = found = 0
    for W, H in ((96, 80), (33, 57), (64, 7), (5, 90), (17, 17)):
        occ = (rng.random((W, H)) < p).astype(np.uint8)
        if p > 0:  # a sealed free cell: unreachable from everywhere else
            occ[W // 2 - 1:W // 2 + 2, H // 2 - 1:H // 2 + 2] = 1
            occ[W // 2, H // 2] = 0
        n = 600
        s = np.stack([rng.integers(0, W, n), rng.integers(0, H, n)], -1).astype(np.int32)
        g = np.stack([rng.integers(0, W, n), rng.integers(0, H, n)], -1).astype(np.int32)
        ss, sg = special_queries(occ, rng)
        if p > 0:
            ss = np.concatenate([ss, [[0, 0], [W // 2, H // 2]]]).astype(np.int32)
            sg = np.concatenate([sg, [[W // 2, H // 2], [0, 0]]]).astype(np.int32)
        s, g = np.concatenate([ss, s]), np.concatenate([sg, g])
        _, ln, _, srch = compare(hs, oracle, dm, occ, s, g, h, W * H + 1, "random %dx%d p=%.1f" % (W, H, p), nthreads=4)
        total += len(ln)
        found += int((ln > 0).sum())
    assert found > total // 8


@pytest.mark.parametrize("h", [1, 2])
def test_max_len_exceeded(hs, oracle, dm, h):
    """A path longer than its slot is -1 with the goal's cost, on both sides; a slot of exactly the length holds it."""
    rng = np.random.default_rng(5)
    occ = (rng.random((96, 80)) < 0.3).astype(np.uint8)
    s = np.stack([rng.integers(0, 96, 400), rng.integers(0, 80, 400)], -1).astype(np.int32)
    g = np.stack([rng.integers(0, 96, 400), rng.integers(0, 80, 400)], -1).astype(np.int32)
    M = device_maps(occ, dm)
    _, full, _, _, _ = host_plan(hs, M, s, g, h, 96 * 80 + 1)
    assert full.max() >= 8
    for max_len in (1, 3, int(full.max()) - 1, int(full.max())):
        cells, ln, cost, pops, pushes = host_plan(hs, M, s, g, h, max_len)
        _, ol, ocost, _ = oracle.plan_batch(occ, s, g, h, literal=False, max_len=max_len)
        assert np.array_equal(ln, ol) and np.array_equal(ln == -1, full > max_len)
        assert (ln == -1).any() or max_len == full.max()
        assert np.array_equal(cost.view(np.uint64), ocost.view(np.uint64))  # (the -1 entries too: the goal's cost)
        assert (cost[ln == -1] > 0).all()
        _, _, _, fpops, fpushes = host_plan(hs, M, s, g, h, 96 * 80 + 1)
        assert np.array_equal(pops, fpops) and np.array_equal(pushes, fpushes)  # (the slot's size changes no search)


@pytest.mark.parametrize("h", [1, 2])
def test_empty_64(hs, oracle, dm, h):
    """Long jumps and goal-line scans: every start of a coarse lattice to every goal of another on an empty 64 x 64."""
    occ = np.zeros((64, 64), np.uint8)
    a = np.array([0, 1, 7, 31, 32, 62, 63])
    cells = np.stack(np.meshgrid(a, a, indexing="ij"), -1).reshape(-1, 2)
    s, g = np.repeat(cells, len(cells), axis=0), np.tile(cells, (len(cells), 1))
    _, ln, _, _ = compare(hs, oracle, dm, occ, s, g, h, 64, "empty 64x64", nthreads=4)
    assert (ln >= 1).all()


@pytest.mark.parametrize("shape", [(8, 8191), (8191, 8)])
@pytest.mark.parametrize("h", [1, 2])
def test_13_bit_strip(hs, oracle, dm, shape, h):
    W, H = shape
    rng = np.random.default_rng(13)
    occ = (rng.random((W, H)) < 0.15).astype(np.uint8)
    n = 48
    s = np.stack([rng.integers(0, W, n), rng.integers(0, H, n)], -1).astype(np.int32)
    g = np.stack([rng.integers(0, W, n), rng.integers(0, H, n)], -1).astype(np.int32)
    s[:4] = [[0, 0], [W - 1, H - 1], [0, H - 1], [W - 1, 0]]
    g[:4] = [[W - 1, H - 1], [0, 0], [W - 1, 0], [0, H - 1]]
    occ[s[:4, 0], s[:4, 1]] = 0
    compare(hs, oracle, dm, occ, s, g, h, 8192, "strip %dx%d" % shape, nthreads=4)


def test_watchdog_and_table_reuse(hs, oracle, dm):
    """A pop bound below what a query needs ends it with the internal code; the next queries on the same table are
    unaffected (generation tags), on another grid shape too."""
    rng = np.random.default_rng(9)
    occ = (rng.random((40, 40)) < 0.25).astype(np.uint8)
    occ[0, 0] = occ[39, 39] = 0
    M = device_maps(occ, dm)
    _, ln, _, pops, _ = host_plan(hs, M, [[0, 0]], [[39, 39]], 2, 1601)
    assert pops[0] > 4
    _, ln2, _, pops2, _ = host_plan(hs, M, [[0, 0]] * 3, [[39, 39]] * 3, 2, 1601, max_pops=int(pops[0]) - 1)
    assert (ln2 == -102).all() and (pops2 == pops[0]).all()
    _, ln3, _, pops3, _ = host_plan(hs, M, [[0, 0]] * 3, [[39, 39]] * 3, 2, 1601, max_pops=int(pops[0]))
    assert (ln3 == ln[0]).all() and (pops3 == pops[0]).all()


def test_two_threads_under_asan_ubsan(hs, oracle, dm, tmp_path):
    """host_search_check.cpp: the host search with two threads as a stand-alone program built with
    -fsanitize=address,undefined, on a map file written here.  The expected lengths, cost bytes and cells in the file are
    the oracle's; pops and pushes are the oracle's where a search ran (compare())."""
    exe = str(tmp_path / "host_search_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-pthread", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-o", exe, os.path.join(HERE, "host_search_check.cpp"),
                           os.path.join(CSRC, "fxjps_host_search.cpp")])
    rng = np.random.default_rng(21)
    blobs = []
    for (W, H), p, h in (((96, 80), 0.2, 2), ((33, 57), 0.4, 1), ((64, 64), 0.0, 2), ((8, 8191), 0.15, 1)):
        occ = (rng.random((W, H)) < p).astype(np.uint8)
        n = 300
        s = np.stack([rng.integers(0, W, n), rng.integers(-1, H + 1, n)], -1).astype(np.int32)
        g = np.stack([rng.integers(-1, W + 1, n), rng.integers(0, H, n)], -1).astype(np.int32)
        s[:, 1] = np.clip(s[:, 1], 0, H - 1)
        M = device_maps(occ, dm)
        max_len = 24  # (some paths do not fit)
        _, _, _, srch = compare(hs, oracle, dm, occ, s, g, h, max_len, "asan file %dx%d" % (W, H), M=M)
        cells, ln, cost, st = oracle.plan_batch(occ, s, g, h, literal=False, max_len=max_len, want_stats=True)
        pops, pushes = np.where(srch, st["pops"], 0).astype(np.int64), np.where(srch, st["pushes"] - 1, 0).astype(np.int64)
        head = np.array([W, H, M["NS"], M["LINES"], M["WORDS"], n, h, max_len], np.int32)
        packed = ((cells[:, :, 0].astype(np.uint32) << 16) | cells[:, :, 1].astype(np.uint32)).astype(np.uint32)
        packed[np.arange(max_len)[None, :] >= np.maximum(ln, 0)[:, None]] = 0
        blobs += [head.tobytes(), M["jd"].tobytes(), M["bm"].tobytes(), M["comp"].tobytes(), s.tobytes(), g.tobytes(), ln.tobytes(),
                  cost.tobytes(), pops.tobytes(), pushes.tobytes(), packed.tobytes()]
    path = tmp_path / "maps.bin"
    path.write_bytes(b"".join(blobs))
    r = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1"))
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert "HOST-SEARCH-CHECK-OK 4 grids 1200 queries" in r.stdout
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr
