"""GPU suite (-m gpu): the read sets behind fxjps_replan_frame's exact reuse, checked against the cells the reference
reads (oracle.read_sets, pinned on the CPU by tests/test_read_sets_host.py).

A stored result is returned without a search when the frame's updates touch none of the tiles its tracking search
marked (oracle/read_sets.py restates the rule).  The reference's answer is a function of the cells it reads, so the
reuse is exact iff every cell the reference read has a marked tile within one cell of it: then no update of such a cell
can slip past the host rule.  Single-cell tiles (grids up to 64 a side) make the check exact at cell level."""
import numpy as np
import pytest

from oracle import read_sets as rs
from test_gpu_fullsize import assert_same, oracle_csr, with_env

pytestmark = pytest.mark.gpu
MPL = 8192


@pytest.fixture(scope="module")
def planner():
    import fuxi_planner_amd as fx
    p = fx.Planner([0])
    yield p
    p.close()


# ------------------------------------------------------------------ maps and queries
def random_map(W, H, dens, rng):
    return (rng.random((W, H)) < dens).astype(np.uint8)


def rooms_map(W, H, rng):
    """Rooms and corridors (test_structured_maps_vs_oracle): walls every 16 cells with doors, a sealed pocket."""
    occ = np.zeros((W, H), dtype=np.uint8)
    occ[::16, :] = 1
    occ[:, ::16] = 1
    for k in range(1, (W - 1) // 16 + 1):
        for j in range((H + 15) // 16):
            occ[16 * k, min(16 * j + int(rng.integers(1, 16)), H - 1)] = 0
    for k in range(1, (H - 1) // 16 + 1):
        for j in range((W + 15) // 16):
            occ[min(16 * j + int(rng.integers(1, 16)), W - 1), 16 * k] = 0
    occ[W // 2:W // 2 + 10, H // 2:H // 2 + 10] = 1
    occ[W // 2 + 3:W // 2 + 6, H // 2 + 3:H // 2 + 6] = 0
    return occ


def open_map(W, H, rng, dens=0.0015):
    """Mostly free: long straight sub-jumps, many ties; a few long walls make corridors."""
    occ = random_map(W, H, dens, rng)
    for _ in range(max(2, (W + H) // 400)):
        if rng.random() < 0.5:
            x = int(rng.integers(0, W))
            y0 = int(rng.integers(0, H))
            occ[x, y0:y0 + int(rng.integers(H // 4, H))] = 1
        else:
            y = int(rng.integers(0, H))
            x0 = int(rng.integers(0, W))
            occ[x0:x0 + int(rng.integers(W // 4, W)), y] = 1
    return occ


def squeeze_map(W, H, rng):
    """Checkerboard patches (diagonal squeezes, jps1.py dblock) in a random map."""
    occ = random_map(W, H, 0.12, rng)
    cb = (np.add.outer(np.arange(W), np.arange(H)) % 2).astype(np.uint8)
    for _ in range(max(3, W * H // 600)):
        x, y = int(rng.integers(0, W)), int(rng.integers(0, H))
        a, b = int(rng.integers(3, 12)), int(rng.integers(3, 12))
        occ[x:x + a, y:y + b] = cb[x:x + a, y:y + b]
    return occ


def make_queries(occ, rng, n):
    """Free starts; a third of the goals on a row, column or diagonal through the start (rays end at the goal), a
    third within 12 cells, the rest anywhere free."""
    W, H = occ.shape
    free = np.argwhere(occ == 0)
    s = free[rng.integers(0, len(free), n)].astype(np.int64)
    g = free[rng.integers(0, len(free), n)].astype(np.int64)
    dirs = np.array([(1, 0), (0, 1), (1, 1), (1, -1), (-1, 0), (0, -1), (-1, -1), (-1, 1)])
    # dead ends (at most one free 4-neighbour): the start's own reads are all that lies behind it
    pad = np.pad(occ, 1, constant_values=1)
    walls = pad[:-2, 1:-1].astype(int) + pad[2:, 1:-1] + pad[1:-1, :-2] + pad[1:-1, 2:]
    ends = np.argwhere((occ == 0) & (walls >= 3))
    if len(ends):
        k = np.arange(2, n, 6)
        s[k] = ends[rng.integers(0, len(ends), len(k))]
    for i in range(n):
        if i % 3 == 0:
            d = dirs[i // 3 % 8]
            for _ in range(8):
                k = int(rng.integers(1, max(W, H)))
                x, y = s[i] + k * d
                if 0 <= x < W and 0 <= y < H and occ[x, y] == 0:
                    g[i] = (x, y)
                    break
        elif i % 3 == 1:
            g[i] = np.clip(s[i] + rng.integers(-12, 13, 2), 0, [W - 1, H - 1])
    return s.astype(np.int32), g.astype(np.int32)


# ------------------------------------------------------------------ the check
def check_cover(planner, oracle, occ, s, g, h, res, what, qs=None):
    """Every cell the reference read, for every query with a path, has a marked tile in its update box.  -> the read
    sets."""
    W, H = occ.shape
    b, tsh = planner.debug_read_sets()
    assert tsh == rs.tile_shift(W, H), (what, tsh)
    off, cells, _, st = res
    qs = np.nonzero(st > 0)[0] if qs is None else np.asarray([q for q in qs if st[q] > 0], dtype=np.int64)
    if len(qs) == 0:
        return b
    bits, ost = oracle.read_sets(occ, s[qs], g[qs], h, nthreads=16)
    assert np.array_equal(ost, st[qs]), what
    bad = []
    for i, q in enumerate(qs):
        u = rs.uncovered(oracle.unpack_read_set(bits[i], W, H), b[q], W, H)
        if len(u):
            x, y = (int(v) for v in u[0])
            on = (x, y) in rs.path_cells(cells[off[q]:off[q + 1]])
            bad.append("%s %dx%d h=%d: query %d %s -> %s: %d cells read outside the read set, first (%d, %d) [%s the path], "
                       "nearest marked tile %s (tsh %d)" % (what, W, H, h, q, s[q].tolist(), g[q].tolist(), len(u), x, y,
                                                            "on" if on else "off", rs.nearest_marked(b[q], x, y, W, H), tsh))
    assert not bad, "\n".join(bad[:8])
    return b


def first_frame(planner, oracle, occ, s, g, h):
    planner.set_grid_occ(occ)
    planner.set_queries(s, g, h, MPL)
    res = planner.replan_frame()
    assert_same(res, oracle_csr(oracle, occ, s, g, h, MPL))
    return res


def grids(rng):
    return [("random", random_map(40, 40, 0.25, rng), 160),     # tsh 0
            ("squeeze", squeeze_map(64, 64, rng), 160),        # tsh 0
            ("open", open_map(64, 50, rng, 0.01), 160),        # tsh 0
            ("random", random_map(100, 120, 0.2, rng), 160),   # tsh 1
            ("rooms", rooms_map(200, 193, rng), 160),          # tsh 2
            ("random", random_map(1024, 1024, 0.2, rng), 120),  # tsh 4
            ("open", open_map(5000, 130, rng), 60)]            # tsh 7, reach classes of 3


# ------------------------------------------------------------------ a. every tracking instantiation
def test_read_sets_cover_the_reference_reads(planner, oracle):
    """Both heuristics, on cell-indexed and on hashed visited tables: the four k_search<HC, true, DIRECT, false>."""
    rng = np.random.default_rng(41)
    seen_tsh, reach3 = set(), False
    for what, occ, n in grids(rng):
        s, g = make_queries(occ, rng, n)
        for direct in (None, 0):
            env = {} if direct is None else {"FXJPS_DIRECT": direct}
            with with_env(**env):
                for h in (2, 1):
                    res = first_frame(planner, oracle, occ, s, g, h)
                    fits = (occ.shape[0] - 1).bit_length() + (occ.shape[1] - 1).bit_length() <= 20
                    assert planner.timing()["table_direct"] == (1 if fits and direct is None else 0), what
                    check_cover(planner, oracle, occ, s, g, h, res, "%s direct=%s" % (what, direct))
        seen_tsh.add(rs.tile_shift(*occ.shape))
        if occ.shape == (5000, 130):
            ci = planner.debug_maps()["ci"][1:-1, 1:-1]
            reach3 = bool(((((ci >> 12) & 3) == 3) & (occ == 0)).any())
    assert seen_tsh == {0, 1, 2, 4, 7}
    assert reach3  # (rays that reach three tiles and more: the whole row is marked)
    planner.set_grid_occ(occ)  # (back to the default scratch configuration)


# ------------------------------------------------------------------ b. after reuse
def window(occ, rng, side, dens):
    W, H = occ.shape
    x0, y0 = int(rng.integers(0, max(W - side, 1))), int(rng.integers(0, max(H - side, 1)))
    xs, ys = np.meshgrid(np.arange(x0, min(x0 + side, W)), np.arange(y0, min(y0 + side, H)), indexing="ij")
    xy = np.stack([xs.ravel(), ys.ravel()], 1).astype(np.int32)
    return xy, (rng.random(len(xy)) < dens).astype(np.uint8)


def test_read_sets_after_reuse(planner, oracle):
    """Tracked frames of local updates: after each, every query with a path -- reused or searched again -- covers what
    the reference reads on the updated grid, and the number reused is what the host rule says."""
    rng = np.random.default_rng(42)
    total = 0
    for what, occ, n, side in (("random", random_map(64, 64, 0.22, rng), 200, 6), ("rooms", rooms_map(200, 193, rng), 200, 14),
                               ("random", random_map(1024, 1024, 0.2, rng), 150, 40)):
        W, H = occ.shape
        s, g = make_queries(occ, rng, n)
        for h in (2, 1):
            o = occ.copy()
            res = first_frame(planner, oracle, o, s, g, h)
            b = check_cover(planner, oracle, o, s, g, h, res, what)
            for f in range(4):
                if f % 2 == 0:
                    xy, val = window(o, rng, side, 0.2)
                else:  # single cells next to paths and anywhere
                    q = int(rng.integers(0, n))
                    c = res[1][res[0][q]:res[0][q + 1]]
                    pick = c[rng.integers(0, len(c))] + rng.integers(-1, 2, 2) if len(c) else rng.integers(0, [W, H])
                    xy = np.array([np.clip(pick, 0, [W - 1, H - 1]), rng.integers(0, [W, H])], np.int32)
                    val = (1 - o[xy[:, 0], xy[:, 1]]).astype(np.uint8)
                track, want = rs.replan_reuse(b, res[3], xy, W, H)
                assert track
                res = planner.replan_frame(xy, val)
                o[xy[:, 0], xy[:, 1]] = val
                assert_same(res, oracle_csr(oracle, o, s, g, h, MPL))
                assert planner.timing()["reused"] == int(want.sum()), (what, h, f)
                total += int(want.sum())
                b = check_cover(planner, oracle, o, s, g, h, res, "%s frame %d" % (what, f))
    assert total > 0


# ------------------------------------------------------------------ c. single cells the reference read
def candidates(mask, path, s, W, H, tsh, rng):
    """Read cells most likely to be missed, in rounds: next to a jump point (the end of a ray, the blocked cell past
    it), next to the start, on a tile border, at the far ends of what was read (the ends of sub-jumps)."""
    xs, ys = np.nonzero(mask)
    cells = np.stack([xs, ys], 1)
    groups = []
    jp = np.asarray(path, dtype=np.int64).reshape(-1, 2)
    if len(jp):
        d = np.abs(cells[:, None, :] - jp[None, :, :]).max(2).min(1)
        groups.append(cells[d <= 1])
    groups.append(cells[np.abs(cells - np.asarray(s, np.int64)).max(1) <= 1])
    if tsh > 0:
        t = (1 << tsh) - 1
        groups.append(cells[((xs & t) == 0) | ((xs & t) == t) | ((ys & t) == 0) | ((ys & t) == t)])
    groups.append(cells[(xs == xs.min()) | (xs == xs.max()) | (ys == ys.min()) | (ys == ys.max())])
    out = []
    for gr in groups:
        out += [tuple(int(v) for v in c) for c in gr[rng.permutation(len(gr))[:6]]]
    return out


def test_single_cell_flips_of_read_cells(planner, oracle):
    """Flip one cell the reference read for a sampled query -- one whose flip changes that query's answer: the frame
    equals the oracle from scratch, and that query is searched again (the count reused is the host rule's)."""
    rng = np.random.default_rng(43)
    changed = 0
    for what, occ, n, frames in (("random", random_map(64, 64, 0.25, rng), 120, 24), ("squeeze", squeeze_map(60, 64, rng), 120, 16),
                                 ("rooms", rooms_map(200, 193, rng), 150, 16), ("random", random_map(1024, 1024, 0.2, rng), 100, 8)):
        W, H = occ.shape
        tsh = rs.tile_shift(W, H)
        s, g = make_queries(occ, rng, n)
        h = 2 if what != "squeeze" else 1
        o = occ.copy()
        res = first_frame(planner, oracle, o, s, g, h)
        b, _ = planner.debug_read_sets()
        for f in range(frames):
            flip = None
            for q in rng.permutation(np.nonzero(res[3] > 0)[0])[:6]:
                bits, _ = oracle.read_sets(o, s[q:q + 1], g[q:q + 1], h)
                path = res[1][res[0][q]:res[0][q + 1]]
                before = oracle.plan_batch(o, s[q:q + 1], g[q:q + 1], h, max_len=MPL)
                for c in candidates(oracle.unpack_read_set(bits[0], W, H), path, s[q], W, H, tsh, rng):
                    o2 = o.copy()
                    o2[c] ^= 1
                    after = oracle.plan_batch(o2, s[q:q + 1], g[q:q + 1], h, max_len=MPL)
                    if after[1][0] != before[1][0] or after[2].tobytes() != before[2].tobytes() or \
                            not np.array_equal(after[0][0, :max(after[1][0], 0)], before[0][0, :max(before[1][0], 0)]):
                        flip = (int(q), c)
                        break
                if flip:
                    break
            if flip is None:
                continue
            q, (x, y) = flip
            xy = np.array([[x, y]], np.int32)
            val = np.array([1 - o[x, y]], np.uint8)
            track, want = rs.replan_reuse(b, res[3], xy, W, H)
            assert track and not want[q], (what, q, (x, y))
            res = planner.replan_frame(xy, val)
            o[x, y] = val[0]
            assert_same(res, oracle_csr(oracle, o, s, g, h, MPL))
            assert planner.timing()["reused"] == int(want.sum()), (what, f)
            b = check_cover(planner, oracle, o, s, g, h, res, "%s flip %d" % (what, f), qs=[q]) if W <= 200 else planner.debug_read_sets()[0]
            changed += 1
    assert changed >= 40


# ------------------------------------------------------------------ d. large-pool retry
def test_read_sets_of_retried_queries(planner, oracle):
    """Queries that outgrow the first scratch pool run again on the large one: their read sets cover their reads."""
    from fuxi_planner_amd import synth
    rng = np.random.default_rng(44)
    occ = synth.synth_grid(320, 288, 21, 0.22)
    s, g = synth.synth_queries(occ, 21, 300)
    for env in ({"FXJPS_TABLE_LOG2": 8}, {"FXJPS_FAR_CAP": 64}):
        with with_env(**env):
            for h in (2, 1):
                o = occ.copy()
                res = first_frame(planner, oracle, o, s, g, h)
                assert planner.timing()["retried"] > 0, env
                b = check_cover(planner, oracle, o, s, g, h, res, "retry %s" % env)
                xy, val = window(o, rng, 16, 0.25)
                track, want = rs.replan_reuse(b, res[3], xy, 320, 288)
                res = planner.replan_frame(xy, val)
                o[xy[:, 0], xy[:, 1]] = val
                assert_same(res, oracle_csr(oracle, o, s, g, h, MPL))
                assert planner.timing()["reused"] == int(want.sum())
                check_cover(planner, oracle, o, s, g, h, res, "retry %s, after a frame" % env)
    planner.set_grid_occ(occ)


# ------------------------------------------------------------------ e. three contexts
def test_three_contexts_return_the_same_read_sets(planner, oracle):
    import fuxi_planner_amd as fx
    rng = np.random.default_rng(45)
    occ = rooms_map(200, 193, rng)
    s, g = make_queries(occ, rng, 301)
    p3 = fx.Planner([0, 0, 0])
    try:
        o = occ.copy()
        for p in (planner, p3):
            p.set_grid_occ(o)
            p.set_queries(s, g, 2, MPL)
        for f in range(3):
            xy, val = window(o, rng, 10, 0.3) if f else (np.zeros((0, 2), np.int32), np.zeros(0, np.uint8))
            r1, r3 = planner.replan_frame(xy, val), p3.replan_frame(xy, val)
            o[xy[:, 0], xy[:, 1]] = val
            assert_same(r1, r3)
            assert planner.timing()["reused"] == p3.timing()["reused"]
            b1, t1 = planner.debug_read_sets()
            b3, t3 = p3.debug_read_sets()
            # (queries that end without a search -- no path, start == goal -- keep what their slot held before)
            searched = (r1[3] > 0) & (s != g).any(1)
            assert searched.sum() > 200
            diff = np.nonzero((b1 != b3).any(1) & searched)[0]
            assert t1 == t3 and len(diff) == 0, (f, diff[:10].tolist())
        assert [c["queries"] for c in p3.timing_per_context()] == [100, 100, 101]
    finally:
        p3.close()


# ------------------------------------------------------------------ f. the reuse happens
def test_reuse_is_not_vacuous(planner, oracle):
    """1024^2, one 64 x 64 window per frame: most frames return stored results without a search."""
    rng = np.random.default_rng(46)
    occ = random_map(1024, 1024, 0.2, rng)
    s, g = make_queries(occ, rng, 300)
    o = occ.copy()
    res = first_frame(planner, oracle, o, s, g, 2)
    b, tsh = planner.debug_read_sets()
    bits, _ = oracle.read_sets(o, s[:60], g[:60], 2)
    marked = sum(int(rs.marked_tiles(b[q]).sum()) for q in range(60) if res[3][q] > 0)
    cover = sum(int(rs.marked_tiles(rs.cover_bitmaps(oracle.unpack_read_set(bits[q], 1024, 1024), 1024, 1024)).sum())
                for q in range(60) if res[3][q] > 0)
    print("read sets: %d marked tiles for a minimum cover of %d (ratio %.2f)" % (marked, cover, marked / max(cover, 1)))
    hits = 0
    for f in range(6):
        xy, val = window(o, rng, 64, 0.2)
        res = planner.replan_frame(xy, val)
        o[xy[:, 0], xy[:, 1]] = val
        hits += planner.timing()["reused"] > 0
    assert_same(res, oracle_csr(oracle, o, s, g, 2, MPL))
    assert hits >= 4, hits
