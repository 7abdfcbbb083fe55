"""Read-set coverage, restated on the host -- TEST INFRASTRUCTURE, NOT THE PRODUCT.

The library's streaming replan (fxjps_replan_frame) returns a stored result without a search when the frame's cell
updates miss the result's read set: the grid tiles ((1 << tsh) cells a side, at most 64 x 64 of them) that the tracking
search marked.  A tile (tx, ty) is marked for a query when bit tx of bitmaps[ty] or bit ty of bitmaps[64 + tx] is set
(fxjps_debug_read_sets).  An update of cell (x, y) touches every tile of the box [max(x-1, 0) .. min(x+1, W-1)] x
[max(y-1, 0) .. min(y+1, H-1)] (cells), shifted right by tsh.

The ground truth is the set of cells the reference's search reads (oracle.read_sets): if none of them changes, the
answer cannot change.  So a read set is sufficient iff every cell the reference read has a marked tile in its box --
then any update of such a cell makes the host search the query again.
"""
import numpy as np


def tile_shift(W, H):
    """The least tsh with (max(W, H) - 1) >> tsh <= 63."""
    t = 0
    while ((max(W, H) - 1) >> t) > 63:
        t += 1
    return t


def marked_tiles(bitmaps):
    """bitmaps u64[128] -> bool[64, 64] indexed [tx, ty]."""
    b = np.asarray(bitmaps, dtype=np.uint64).reshape(128)
    bits = ((b[:, None] >> np.arange(64, dtype=np.uint64)[None, :]) & np.uint64(1)).astype(bool)
    return bits[:64].T | bits[64:]


def cover_bitmaps(mask, W, H):
    """The bitmaps that mark exactly the tile of every cell of mask (bool[W, H]), in the bx half."""
    tsh = tile_shift(W, H)
    out = np.zeros(128, dtype=np.uint64)
    xs, ys = np.nonzero(mask)
    for tx, ty in set(zip((xs >> tsh).tolist(), (ys >> tsh).tolist())):
        out[ty] |= np.uint64(1) << np.uint64(tx)
    return out


def _box(xs, ys, W, H, tsh):
    tx0, tx1 = np.maximum(xs - 1, 0) >> tsh, np.minimum(xs + 1, W - 1) >> tsh
    ty0, ty1 = np.maximum(ys - 1, 0) >> tsh, np.minimum(ys + 1, H - 1) >> tsh
    return tx0, tx1, ty0, ty1


def covered(xs, ys, M, W, H):
    """Per cell (xs, ys): does its update box hold a tile marked in M (bool[64, 64])?"""
    tsh = tile_shift(W, H)
    tx0, tx1, ty0, ty1 = _box(np.asarray(xs, np.int64), np.asarray(ys, np.int64), W, H, tsh)
    cov = np.zeros(len(tx0), dtype=bool)
    for tx in (tx0, np.minimum(tx0 + 1, tx1), tx1):  # (a box spans at most 3 tiles a side: tsh = 0)
        for ty in (ty0, np.minimum(ty0 + 1, ty1), ty1):
            cov |= M[tx, ty]
    return cov


def uncovered(mask, bitmaps, W, H):
    """The cells of mask (bool[W, H], what the reference read) whose update box holds no marked tile: int[n, 2].  Empty
    iff the read set is sufficient."""
    xs, ys = np.nonzero(mask)
    cov = covered(xs, ys, marked_tiles(bitmaps), W, H)
    return np.stack([xs[~cov], ys[~cov]], 1)


def nearest_marked(bitmaps, x, y, W, H):
    """The marked tile nearest (Chebyshev, in tiles) to the tile of (x, y): (tx, ty, distance), or None."""
    tsh = tile_shift(W, H)
    t = np.argwhere(marked_tiles(bitmaps))
    if len(t) == 0:
        return None
    d = np.maximum(np.abs(t[:, 0] - (x >> tsh)), np.abs(t[:, 1] - (y >> tsh)))
    i = int(np.argmin(d))
    return int(t[i, 0]), int(t[i, 1]), int(d[i])


def path_cells(jump_points):
    """Every cell of the straight / diagonal segments between consecutive jump points."""
    pts = [tuple(int(v) for v in p) for p in jump_points]
    out = set(pts[:1])
    for (ax, ay), (bx, by) in zip(pts, pts[1:]):
        n = max(abs(bx - ax), abs(by - ay))
        for i in range(1, n + 1):
            out.add((ax + i * np.sign(bx - ax), ay + i * np.sign(by - ay)))
    return out


def touched_tiles(xy, W, H):
    """bool[64, 64]: the tiles a frame's cell updates xy (int[n, 2]) touch, as fxjps_replan_frame computes them."""
    tsh = tile_shift(W, H)
    T = np.zeros((64, 64), dtype=bool)
    for x, y in np.asarray(xy, dtype=np.int64).reshape(-1, 2):
        if x < 0 or y < 0 or x >= W or y >= H:
            continue
        tx0, tx1, ty0, ty1 = _box(x, y, W, H, tsh)
        T[tx0:tx1 + 1, ty0:ty1 + 1] = True
    return T


def replan_reuse(bitmaps, status, xy, W, H):
    """The host rule of fxjps_replan_frame, restated: -> (track, reused bool[nq]).  track: the frame records read sets
    (it touches at most half of the tiles); reused: the stored results (of a tracked previous frame) it returns without
    a search -- a path, and no touched tile marked."""
    tsh = tile_shift(W, H)
    T = touched_tiles(xy, W, H)
    tiles = (((W - 1) >> tsh) + 1) * (((H - 1) >> tsh) + 1)
    track = 2 * int(T.sum()) <= tiles
    reused = np.zeros(len(status), dtype=bool)
    if track:
        for q in range(len(status)):
            reused[q] = status[q] > 0 and not (marked_tiles(bitmaps[q]) & T).any()
    return track, reused
