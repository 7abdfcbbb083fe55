"""CPU suite: the read-set recorder of the oracle (oracle.read_sets) and the coverage check the GPU read-set tests run
(oracle/read_sets.py).  The recorder is pinned to the pure-Python restatement (itself pinned to the real jps1.py by the
goldens) read for read, and shown sufficient: a cell outside a query's mask never changes that query's answer.  The
checker is shown to pass on a cover built from the mask and to fail on a cover with a tile missing or shifted."""
import numpy as np

from oracle import jps_python as jp
from oracle import read_sets as rs


class RecordingGrid(jp.CountingGrid):
    """A CountingGrid that also records every (x, y) it hands out."""

    class _Row(object):
        __slots__ = ("r", "o", "x")

        def __init__(self, r, o, x):
            self.r = r
            self.o = o
            self.x = x

        def __getitem__(self, y):
            self.o.reads += 1
            self.o.cells.add((self.x, int(y)))
            return self.r[y]

    def __init__(self, a):
        jp.CountingGrid.__init__(self, a)
        self.cells = set()

    def __getitem__(self, x):
        return RecordingGrid._Row(self.a[x], self, int(x))


def small_grids(n, side, seed):
    rng = np.random.default_rng(seed)
    out = [np.zeros((1, 1), np.uint8), np.zeros((1, 7), np.uint8), np.zeros((9, 1), np.uint8), np.zeros((6, 6), np.uint8)]
    cb = (np.add.outer(np.arange(8), np.arange(9)) % 2).astype(np.uint8)
    out += [cb, 1 - cb]
    while len(out) < n:
        W, H = (int(v) for v in rng.integers(1, side + 1, 2))
        out.append((rng.random((W, H)) < rng.choice([0.0, 0.05, 0.2, 0.35, 0.5])).astype(np.uint8))
    return out


def queries(occ, rng, n):
    """Random free starts; goals free, on an obstacle, off the grid, on the start, and on a row / column / diagonal
    through the start."""
    W, H = occ.shape
    free = np.argwhere(occ == 0)
    if len(free) == 0:
        return np.zeros((0, 2), np.int32), np.zeros((0, 2), np.int32)
    s = free[rng.integers(0, len(free), n)]
    g = free[rng.integers(0, len(free), n)]
    occd = np.argwhere(occ == 1)
    for i in range(n):
        k = i % 8
        if k == 1 and len(occd):
            g[i] = occd[rng.integers(0, len(occd))]
        elif k == 2:
            g[i] = [W + 1, int(rng.integers(0, H))] if i % 16 == 2 else [-1, -3]
        elif k == 3:
            g[i] = s[i]
        elif k in (4, 5, 6):
            d = int(rng.integers(1, max(W, H) + 1))
            dx, dy = ((1, 0), (0, 1), (1, 1))[k - 4]
            sg = 1 if rng.random() < 0.5 else -1
            g[i] = [min(max(s[i][0] + sg * d * dx, 0), W - 1), min(max(s[i][1] + sg * d * dy, 0), H - 1)]
    return s.astype(np.int32), g.astype(np.int32)


def test_recorded_cells_equal_the_python_restatement(oracle):
    rng = np.random.default_rng(7)
    grids = small_grids(200, 40, 11)
    checked = 0
    for gi, occ in enumerate(grids):
        W, H = occ.shape
        s, g = queries(occ, rng, 3)
        for h in (1, 2):
            bits, st = oracle.read_sets(occ, s, g, h, nthreads=4)
            for q in range(len(s)):
                m = RecordingGrid(occ)
                path, _, _ = jp.search(m, tuple(int(v) for v in s[q]), tuple(int(v) for v in g[q]), h)
                assert st[q] == (0 if path == 0 else len(path)), (gi, q, h)
                got = set(map(tuple, np.argwhere(oracle.unpack_read_set(bits[q], W, H)).tolist()))
                assert got == m.cells, (gi, occ.shape, s[q].tolist(), g[q].tolist(), h, sorted(got ^ m.cells)[:8])
                checked += 1
    assert checked > 900


def test_the_mask_is_sufficient(oracle):
    """Flip every cell outside a query's mask, one at a time: its status, path and cost bytes stay put."""
    rng = np.random.default_rng(8)
    grids = small_grids(40, 14, 12)
    for gi, occ in enumerate(grids):
        W, H = occ.shape
        s, g = queries(occ, rng, 10)
        if len(s) == 0:
            continue
        for h in (1, 2):
            bits, st = oracle.read_sets(occ, s, g, h, nthreads=4)
            masks = np.stack([oracle.unpack_read_set(b, W, H) for b in bits])
            ml = W * H + 1
            cells0, len0, cost0, _ = oracle.plan_batch(occ, s, g, h, literal=True, max_len=ml)
            assert np.array_equal(len0, st)
            for x in range(W):
                for y in range(H):
                    keep = ~masks[:, x, y]
                    if not keep.any():
                        continue
                    o2 = occ.copy()
                    o2[x, y] ^= 1
                    cells, ln, cost, _ = oracle.plan_batch(o2, s[keep], g[keep], h, literal=True, max_len=ml)
                    assert np.array_equal(ln, len0[keep]), (gi, x, y, h)
                    assert cost.tobytes() == cost0[keep].tobytes(), (gi, x, y, h)
                    assert np.array_equal(cells, cells0[keep]), (gi, x, y, h)


def read_masks(oracle, occ, s, g, h):
    W, H = occ.shape
    bits, st = oracle.read_sets(occ, s, g, h)
    masks = [oracle.unpack_read_set(b, W, H) for b, t in zip(bits, st) if t > 0]
    return [m for m in masks if m.sum() >= 8]  # (start == goal reads nothing)


def test_tile_shift():
    assert [rs.tile_shift(W, H) for W, H in ((1, 1), (64, 3), (65, 3), (3, 128), (3, 129), (200, 200), (1024, 1024), (5000, 130))] == \
        [0, 0, 1, 1, 2, 2, 4, 7]


def test_checker_passes_on_the_cover_of_the_mask(oracle):
    rng = np.random.default_rng(9)
    for W, H, dens in ((40, 40, 0.2), (64, 30, 0.3), (100, 120, 0.2), (200, 200, 0.15)):
        occ = (rng.random((W, H)) < dens).astype(np.uint8)
        s, g = queries(occ, rng, 24)
        for m in read_masks(oracle, occ, s, g, 2):
            assert len(rs.uncovered(m, rs.cover_bitmaps(m, W, H), W, H)) == 0
            # ... and the same tiles in the other half of the bitmaps
            b = rs.cover_bitmaps(m, W, H)
            M = rs.marked_tiles(b)
            b2 = np.zeros(128, np.uint64)
            for tx, ty in np.argwhere(M):
                b2[64 + tx] |= np.uint64(1) << np.uint64(ty)
            assert len(rs.uncovered(m, b2, W, H)) == 0


def test_checker_names_the_cell_of_a_dropped_tile(oracle):
    """Drop a tile that is the only marked tile in some read cell's box: the check fails and names that cell."""
    rng = np.random.default_rng(10)
    dropped = 0
    for W, H, dens in ((40, 40, 0.2), (50, 64, 0.3), (100, 120, 0.2), (200, 200, 0.15)):
        occ = (rng.random((W, H)) < dens).astype(np.uint8)
        s, g = queries(occ, rng, 24)
        tsh = rs.tile_shift(W, H)
        for m in read_masks(oracle, occ, s, g, 2):
            b = rs.cover_bitmaps(m, W, H)
            M = rs.marked_tiles(b)
            xs, ys = np.nonzero(m)
            for i in rng.permutation(len(xs))[:40]:
                x, y = int(xs[i]), int(ys[i])
                box = [(tx, ty) for tx in range(max(x - 1, 0) >> tsh, (min(x + 1, W - 1) >> tsh) + 1)
                       for ty in range(max(y - 1, 0) >> tsh, (min(y + 1, H - 1) >> tsh) + 1) if M[tx, ty]]
                if len(box) != 1:
                    continue
                tx, ty = box[0]
                b2 = b.copy()
                b2[ty] &= ~(np.uint64(1) << np.uint64(tx))
                bad = rs.uncovered(m, b2, W, H)
                assert [x, y] in bad.tolist(), (W, H, x, y)
                dropped += 1
                break
    assert dropped >= 10


def test_checker_fails_on_shifted_marks(oracle):
    """Every mark one tile over (two on single-cell tiles, where the one-cell dilation of the box absorbs one)."""
    rng = np.random.default_rng(11)
    for W, H, dens in ((40, 40, 0.2), (100, 120, 0.2), (200, 200, 0.15), (1024, 60, 0.2)):
        occ = (rng.random((W, H)) < dens).astype(np.uint8)
        s, g = queries(occ, rng, 16)
        k = np.uint64(1 if rs.tile_shift(W, H) > 0 else 2)
        for m in read_masks(oracle, occ, s, g, 1):
            b = rs.cover_bitmaps(m, W, H)
            right = b.copy()
            right[:64] = b[:64] << k
            left = b.copy()
            left[:64] = b[:64] >> k
            for b2 in (right, left):  # every x tile over
                assert len(rs.uncovered(m, b2, W, H)) > 0, (W, H)
            up = np.zeros(128, np.uint64)  # every y tile over, in the other half of the bitmaps
            for tx, ty in np.argwhere(rs.marked_tiles(b)):
                if ty + int(k) < 64:
                    up[64 + tx] |= np.uint64(1) << np.uint64(ty + int(k))
            assert len(rs.uncovered(m, up, W, H)) > 0, (W, H)


def test_replan_rule_restated():
    """replan_reuse: the dilation by one cell, the clamping at the grid's edge and the half-of-the-tiles cut-off."""
    W = H = 64  # tsh 0: a tile is a cell
    b = np.zeros((2, 128), np.uint64)
    b[0, 10] = np.uint64(1) << np.uint64(20)  # query 0 marked (20, 10)
    b[1, 64 + 0] = np.uint64(1)               # query 1 marked (0, 0)
    st = np.array([3, 2])
    assert replan(b, st, [[21, 11]]) == [False, True]  # next to (20, 10): query 0 searches again
    assert replan(b, st, [[22, 10]]) == [True, True]   # two cells away: both reused
    assert replan(b, st, [[1, 1]]) == [True, False]
    assert replan(b, np.array([0, 2]), [[40, 40]]) == [False, True]  # no path: always searched again
    assert replan(b, st, [[-1, 0], [64, 64]]) == [True, True]        # off the grid: ignored
    big = np.argwhere(np.ones((46, 46), bool))  # 48 x 48 touched tiles > half of 4096
    track, reused = rs.replan_reuse(b, st, big, W, H)
    assert not track and not reused.any()
    W, H = 1024, 1024  # tsh 4: (31, 31) touches tiles (1, 1) and (2, 2)
    b = np.zeros((1, 128), np.uint64)
    b[0, 2] = np.uint64(1) << np.uint64(2)
    assert rs.replan_reuse(b, np.array([1]), [[31, 31]], W, H)[1].tolist() == [False]
    assert rs.replan_reuse(b, np.array([1]), [[30, 30]], W, H)[1].tolist() == [True]


def replan(b, st, xy):
    track, reused = rs.replan_reuse(b, st, np.array(xy, np.int64), 64, 64)
    assert track
    return reused.tolist()
