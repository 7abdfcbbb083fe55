"""CPU suite: the host reference of the library's derived grid maps (oracle/derived_maps.py).  Its jump table is pinned to
the pure-Python restatement of jump() (oracle/jps_python.py, itself pinned to the real jps1.py by the goldens), its
memoised form to the literal recursion, its components to a plain BFS, and its packers to each other: decoding the
packed maps gives back the table they were packed from.  tests/test_derived_maps_gpu.py compares the device's maps with
it byte for byte."""
from collections import deque

import numpy as np

from oracle import derived_maps as dm
from oracle import jps_python as jp

OFF = (-1000, -1000)  # a goal no cell can match


def small_grids():
    """About 200 grids of up to 24 x 24: the degenerate shapes, all-free, all-occupied, checkerboards, random."""
    rng = np.random.default_rng(2026)
    out = [np.zeros((1, 1), np.uint8), np.ones((1, 1), np.uint8)]
    for n in (2, 5, 9):
        for W, H in ((1, n), (n, 1)):
            out += [np.zeros((W, H), np.uint8), np.ones((W, H), np.uint8), (rng.random((W, H)) < 0.4).astype(np.uint8)]
    for W, H in ((4, 4), (7, 5), (6, 11)):
        cb = (np.add.outer(np.arange(W), np.arange(H)) % 2).astype(np.uint8)
        out += [np.zeros((W, H), np.uint8), np.ones((W, H), np.uint8), cb, 1 - cb]
    while len(out) < 200:
        W, H = (int(v) for v in rng.integers(1, 25, 2))
        out.append((rng.random((W, H)) < rng.choice([0.05, 0.2, 0.35, 0.5])).astype(np.uint8))
    return out


GRIDS = small_grids()


def check_table_against_python(occ, found, k):
    W, H = occ.shape
    for x in range(W):
        for y in range(H):
            for s, (dx, dy) in enumerate(dm.SLOTS):
                r = jp._leap(occ, x, y, dx, dy, OFF)
                assert bool(found[x, y, s]) == (r is not None), (occ.shape, x, y, (dx, dy))
                kk = int(k[x, y, s])
                ex, ey = x + kk * dx, y + kk * dy
                if r is not None:
                    assert (ex, ey) == r, (occ.shape, x, y, (dx, dy), r, kk)
                    continue
                # None: the cell it returned on ends the ray (off the grid, occupied, or squeezed after the first
                # step), and every cell before it is free
                assert kk >= 1
                on = 0 <= ex < W and 0 <= ey < H
                assert not on or occ[ex, ey] == 1 or (dx and dy and kk > 1 and jp._squeezed(occ, ex, ey, dx, dy)), \
                    (occ.shape, x, y, (dx, dy), kk)
                for i in range(1, kk):
                    assert occ[x + i * dx, y + i * dy] == 0, (occ.shape, x, y, (dx, dy), i)


def test_jump_table_equals_the_python_jump(oracle):
    for occ in GRIDS:
        found, k = oracle.jump_table(occ)
        check_table_against_python(occ, found, k)


def test_memoised_table_equals_the_literal_recursion(oracle):
    for occ in GRIDS + [oracle.synth_grid(40, 37, 5, 0.1), np.zeros((30, 33), np.uint8)]:
        f1, k1, fl1 = oracle.jump_table(occ, flags=True)
        f2, k2, fl2 = oracle.jump_table(occ, literal=True, nthreads=3, flags=True)
        assert np.array_equal(f1, f2) and np.array_equal(k1, k2) and np.array_equal(fl1, fl2), occ.shape


def test_jump_table_flags_are_the_python_tests(oracle):
    """bit 0: the forced-neighbour test of jump()'s loop; bit 1: dblock (off the grid counted occupied)."""
    for occ in GRIDS[::4]:
        _, _, fl = oracle.jump_table(occ, flags=True)
        W, H = occ.shape
        pad = dm.padded(occ, 1)
        for x in range(W):
            for y in range(H):
                for s, (dx, dy) in enumerate(dm.SLOTS):
                    if dx and dy:
                        f = (not jp._wall(occ, x, y, -dx, dy) and jp._wall(occ, x, y, -dx, 0) or
                             not jp._wall(occ, x, y, dx, -dy) and jp._wall(occ, x, y, 0, -dy))
                        sq = pad[x + 1 - dx, y + 1] == 1 and pad[x + 1, y + 1 - dy] == 1
                    elif dx:
                        f = (not jp._wall(occ, x, y, dx, 1) and jp._wall(occ, x, y, 0, 1) or
                             not jp._wall(occ, x, y, dx, -1) and jp._wall(occ, x, y, 0, -1))
                        sq = False
                    else:
                        f = (not jp._wall(occ, x, y, 1, dy) and jp._wall(occ, x, y, 1, 0) or
                             not jp._wall(occ, x, y, -1, dy) and jp._wall(occ, x, y, -1, 0))
                        sq = False
                    assert fl[x, y, s] == int(bool(f)) | (int(bool(sq)) << 1), (occ.shape, x, y, (dx, dy))


def bfs_labels(occ):
    W, H = occ.shape
    lab = -np.ones((W, H), np.int64)
    for x0 in range(W):
        for y0 in range(H):
            if occ[x0, y0] or lab[x0, y0] >= 0:
                continue
            lab[x0, y0] = x0 * H + y0
            q = deque([(x0, y0)])
            while q:
                x, y = q.popleft()
                for ax, ay in ((x - 1, y), (x + 1, y), (x, y - 1), (x, y + 1)):
                    if 0 <= ax < W and 0 <= ay < H and not occ[ax, ay] and lab[ax, ay] < 0:
                        lab[ax, ay] = x0 * H + y0
                        q.append((ax, ay))
    return lab


def test_components_equal_a_python_bfs(oracle):
    for occ in GRIDS + [oracle.synth_grid(70, 130, 4, 0.45)]:
        assert np.array_equal(oracle.components(occ), bfs_labels(occ)), occ.shape


def test_component_checks_catch_wrong_forests(oracle):
    occ = np.zeros((6, 9), np.uint8)
    occ[3, :] = 1  # two components: x < 3 and x > 3
    lab = oracle.components(occ)
    assert dm.component_problem(lab, occ, exact=True) is None
    merged = lab.copy()
    merged[4:] = 0  # one root over both: sound, not exact
    assert dm.component_problem(merged, occ, exact=False) is None
    assert "share a root" in dm.component_problem(merged, occ, exact=True)
    split = lab.copy()
    split[5, 8] = 5 * 9 + 8  # a cell of the right component under a root of its own
    assert "split" in dm.component_problem(split, occ, exact=False)
    lost = lab.copy()
    lost[0, 0] = -1
    assert "no root" in dm.component_problem(lost, occ, exact=False)
    stale = lab.copy()
    stale[3, 4] = 0  # an occupied cell in the forest: fine after an update made it occupied, not after a full build
    assert dm.component_problem(stale, occ, exact=False) is None
    assert "was not free" in dm.component_problem(stale, occ, exact=True)
    assert "was not free" in dm.component_problem(stale, occ, exact=False, ever_free=occ == 0)


def test_nb8_packer_is_the_neighbour_mask_formula():
    """The formula of test_gpu_parity.test_neighbour_mask_map, on shapes of every kind."""
    for occ in GRIDS[::5] + [(np.random.default_rng(2).random((37, 70)) < 0.3).astype(np.uint8)]:
        W, H = occ.shape
        pad = np.ones((W + 4, H + 4), dtype=np.uint8)
        pad[2:-2, 2:-2] = occ
        exp = np.zeros((W + 2, H + 2), dtype=np.uint8)
        k = 0
        for dx in (-1, 0, 1):
            for dy in (-1, 0, 1):
                if dx or dy:
                    exp |= pad[1 + dx:W + 3 + dx, 1 + dy:H + 3 + dy] << k
                    k += 1
        assert np.array_equal(dm.nb8_map(occ), exp)


def unpack(words):
    """uint64[..., WORDS] -> bool[..., WORDS * 64], position 64 w + i = bit i of word w."""
    b = np.ascontiguousarray(words).view(np.uint8)
    return np.unpackbits(b, axis=-1, bitorder="little").astype(bool)


def scan(hit, die, pos, step, first_die=None):
    """First position at or after pos (moving by step) with either bit: -> (position, jump point?)."""
    while True:
        d = die[pos] if first_die is None else first_die
        if hit[pos] or d:
            return pos, not d
        pos += step
        first_die = None


def test_packed_maps_give_back_the_jump_table(oracle):
    """Decode what the packers wrote and walk it as the device does: a straight jump is the first stop bit of its scan
    line, a diagonal one the first hit / die bit of its diagonal (the first step dies on occupancy alone); the jd
    records, the ci bits 8 - 15 and the nb8 bits of the records say the same as the table."""
    for occ in GRIDS[::3] + [oracle.synth_grid(80, 70, 6, 0.2), np.zeros((1, 200), np.uint8)]:
        W, H = occ.shape
        found, k, fl = oracle.jump_table(occ, flags=True)
        ref = dm.reference_maps(occ, (found, k, fl))
        L = dm.layout(W, H)
        PW, PH = L["PW"], L["PH"]
        f2, k2, nb = dm.decode_jd(ref["jd"])
        assert np.array_equal(f2, found) and np.array_equal(k2, k & dm.JD_K), occ.shape
        assert not ref["jd"][0].any() and not ref["jd"][-1].any() and not ref["jd"][:, 0].any() and not ref["jd"][:, -1].any()
        nb8 = ref["nb8"][1:-1, 1:-1]
        for s in range(8):
            assert np.array_equal(nb[:, :, s], (nb8 >> (2 * s)) & 3 if s < 4 else 0 * nb8)
        ci = ref["ci"][1:-1, 1:-1]
        free = occ == 0
        assert np.array_equal(ci & 0xFF, nb8)
        assert not (ci[~free] >> 8).any()
        for i, d in enumerate(dm.STRAIGHT):
            assert np.array_equal((ci[free] >> (8 + i)) & 1, found[:, :, dm.SLOT[d]][free])
        bm = unpack(ref["bm"])      # [4, LINES, 2, WORDS * 64] after the view: (stop, occ) interleaved per word
        bm = bm.reshape(4, L["LINES"], L["WORDS"], 2, 64)
        stop, bocc = bm[:, :, :, 0, :].reshape(4, L["LINES"], -1), bm[:, :, :, 1, :].reshape(4, L["LINES"], -1)
        dbm = unpack(ref["dbm"]).reshape(4, L["DLINES"], L["WORDS"], 2, 64)
        dhit, ddie = dbm[:, :, :, 0, :].reshape(4, L["DLINES"], -1), dbm[:, :, :, 1, :].reshape(4, L["DLINES"], -1)
        for x in range(W):
            for y in range(H):
                px, py = x + 1, y + 1
                for di, (dx, dy) in enumerate(dm.STRAIGHT):
                    line, pos = (py, px) if dx else (px, py)
                    r, jpt = scan(stop[di, line], bocc[di, line], pos + dx + dy, dx + dy)
                    s = dm.SLOT[(dx, dy)]
                    assert (r - pos) * (dx + dy) == k[x, y, s] and jpt == bool(found[x, y, s]), (occ.shape, x, y, (dx, dy))
                for dd, (dx, dy) in enumerate(dm.DIAGONAL):
                    line = (px - py + PH - 1) if dx == dy else (px + py)
                    first = dm.padded(occ, 1)[px + dx, py + dy] == 1
                    r, jpt = scan(dhit[dd, line], ddie[dd, line], px + dx, dx, first_die=first)
                    s = dm.SLOT[(dx, dy)]
                    assert (r - px) * dx == k[x, y, s] and jpt == bool(found[x, y, s]), (occ.shape, x, y, (dx, dy))
        # positions no cell of the grid's padding occupies: die, never hit
        assert not dhit[:, :, PW:].any() and ddie[:, :, PW:].all()


def test_read_set_tile_extents():
    """ci bits 12 - 15 from their definition: tile(p) = min(max((p - 1) >> tsh, 0), 63), the farthest tile a +-x (+-y)
    ray's end reaches beyond the cell's own, at most 3; tsh is 0 at 64 cells a side, 1 at 65, 7 at 8190."""
    assert [dm.layout(n, 1)["tsh"] for n in (1, 64, 65, 128, 129, 2048, 2100, 4096, 8190)] == [0, 0, 1, 1, 2, 5, 6, 6, 7]
    occ = np.zeros((1, 200), np.uint8)  # tsh = 2: tiles of 4 cells; from y the +y ray ends at the border, y = 200
    ref = dm.reference_maps(occ)
    ci = ref["ci"][1, 1:-1]
    for y in range(200):
        ty = lambda p: min(max((p - 1) >> 2, 0), 63)  # noqa: E731
        py = y + 1
        ey = min(max(ty(201) - ty(py), ty(py) - ty(0), 0), 3)
        assert (ci[y] >> 14) == ey and (ci[y] >> 12) & 3 == 0, y


def test_longest_ray_fits_the_distance_field(oracle):
    """1 x 8190, empty: from the first cell the +y ray returns at the border, 8190 cells on -- JD_K is 8191."""
    occ = np.zeros((1, 8190), np.uint8)
    found, k = oracle.jump_table(occ)
    assert k[0, 0, dm.SLOT[(0, 1)]] == 8190 and k[0, 8189, dm.SLOT[(0, -1)]] == 8190 and not found.any()
    ref = dm.reference_maps(occ, oracle.jump_table(occ, flags=True))
    assert ref["jd"][1, 1, dm.SLOT[(0, 1)]] == 8190
