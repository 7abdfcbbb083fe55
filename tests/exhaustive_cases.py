"""The exhaustive small-grid families of tests/golden/exhaustive.npz: shapes, grids, blocks, queries and the two digests.

One module for the generator (tests/golden/make_golden_exhaustive.py, the real jps1.py), the host suite (the C oracle and
its Python restatement) and the GPU suite (the planner), so that the three cannot drift apart.  No reference code here.

Shapes   every (W, H) with W * H <= 12 (35 of them), then 4 x 4.
Grids    all 2^(W*H) of a shape; grid code b is occ = ((b >> arange(W*H)) & 1).reshape(W, H): bit x*H + y is cell (x, y),
         1 = obstacle.
Queries  of one grid, in this order: starts over the W*H cells in flat order (outer loop); goals (inner loop) over the
         (W+2) x (H+2) cells x = -1 .. W, y = -1 .. H, row-major -- the grid and the ring one cell outside it -- where
         W * H <= 12, over the 16 cells of the grid for 4 x 4.
Blocks   BLOCK = 16 consecutive grid codes (one block where a shape has fewer grids).
Digests  two per block and heuristic, each the first 8 bytes, little-endian, of a SHA-256 (RECIPE below).
"""
import hashlib

import numpy as np

BLOCK = 16
HCHOICES = (1, 2)
SHAPES = tuple((W, H) for W in range(1, 13) for H in range(1, 13) if W * H <= 12) + ((4, 4),)
CHUNKS_4X4 = 16  # the parametrisation of 4 x 4 in both suites: 16 chunks of 4 096 grids = 256 blocks

RECIPE = ("Per block of 16 consecutive grid codes (one block where a shape has fewer grids) and per hchoice, two uint64: the "
          "first 8 bytes, little-endian, of a SHA-256.  Result digest, over, for each grid of the block in code order: len of "
          "every query as <i4 (number of jump points, 0 = no path), then every query's cells as <i4 x, y pairs in query "
          "order, then cost of every query as <f8 (0.0 for no path and for start == goal).  Work digest, over, for each grid "
          "in code order: cells, pushes, pops of every query as <i8, three arrays in that order.  Queries of a grid: starts "
          "over all cells in flat order x*H + y (outer), goals (inner) over x = -1 .. W, y = -1 .. H row-major where "
          "W*H <= 12, over the grid's cells for 4x4.  Grid code b: bit x*H + y is cell (x, y), 1 = obstacle.")


def has_ring(W, H):
    return W * H <= 12


def shape_name(W, H):
    return "%dx%d" % (W, H)


def n_grids(W, H):
    return 1 << (W * H)


def n_blocks(W, H):
    return max(1, n_grids(W, H) // BLOCK)


def block_codes(W, H, block):
    """The grid codes of block `block`."""
    n = min(BLOCK, n_grids(W, H))
    return range(block * n, (block + 1) * n)


def grid(W, H, code):
    """Grid `code` of the shape: uint8[W, H], 1 = obstacle."""
    return ((int(code) >> np.arange(W * H, dtype=np.int64)) & 1).astype(np.uint8).reshape(W, H)


_queries = {}


def queries(W, H):
    """-> (starts int32[nq, 2], goals int32[nq, 2]) of one grid of the shape, in the fixture's order (read-only)."""
    if (W, H) not in _queries:
        cells = np.stack(np.meshgrid(np.arange(W), np.arange(H), indexing="ij"), -1).reshape(-1, 2)
        if has_ring(W, H):
            goals = np.stack(np.meshgrid(np.arange(-1, W + 1), np.arange(-1, H + 1), indexing="ij"), -1).reshape(-1, 2)
        else:
            goals = cells
        s = np.repeat(cells, len(goals), axis=0).astype(np.int32)
        g = np.tile(goals, (len(cells), 1)).astype(np.int32)
        s.setflags(write=False)
        g.setflags(write=False)
        _queries[(W, H)] = (s, g)
    return _queries[(W, H)]


def n_queries(W, H):
    """Queries of one grid of the shape, per heuristic."""
    return W * H * ((W + 2) * (H + 2) if has_ring(W, H) else W * H)


def shape_queries(W, H):
    """Queries of all grids of the shape, per heuristic."""
    return n_grids(W, H) * n_queries(W, H)


def array_name(kind, W, H, h):
    """kind "r" (result digests) or "w" (work digests): e.g. r_3x4_h2."""
    return "%s_%s_h%d" % (kind, shape_name(W, H), h)


def _u64(sha):
    return int.from_bytes(sha.digest()[:8], "little")


def result_digest(grids):
    """`grids`: per grid of the block, in code order, (length int[nq], cells int[sum(length), 2], cost float64[nq])."""
    sha = hashlib.sha256()
    for length, cells, cost in grids:
        length = np.asarray(length)
        cells = np.asarray(cells).reshape(-1, 2)
        assert len(cells) == int(np.maximum(length, 0).sum()), (len(cells), length)
        sha.update(np.ascontiguousarray(length, dtype="<i4").tobytes())
        sha.update(np.ascontiguousarray(cells, dtype="<i4").tobytes())
        sha.update(np.ascontiguousarray(cost, dtype="<f8").tobytes())
    return _u64(sha)


def work_digest(grids):
    """`grids`: per grid of the block, in code order, (cells int[nq], pushes int[nq], pops int[nq])."""
    sha = hashlib.sha256()
    for counts in grids:
        assert len(counts) == 3
        for a in counts:
            sha.update(np.ascontiguousarray(a, dtype="<i8").tobytes())
    return _u64(sha)


def padded_to_csr(cells, length):
    """The oracle's (cells int32[nq, max_len, 2], length int32[nq]) -> the cells of all queries in query order, [n, 2]."""
    keep = np.arange(cells.shape[1])[None, :] < np.maximum(length, 0)[:, None]
    return cells[keep].reshape(-1, 2)


# ------------------------------------------------------------------ the fixture
MAX_LEN = 32  # path slot of every run: a path visits a cell once, so it has at most W * H <= 16 jump points
THREADS = 16


def load_fixture():
    """tests/golden/exhaustive.npz -> ({array name: uint64[blocks]}, meta dict)."""
    import json
    import os
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "exhaustive.npz"))
    arrays = {k: z[k] for k in z.files if k != "meta"}
    return arrays, json.loads(str(z["meta"]))


def chunk_blocks(W, H, chunk=None):
    """The blocks of one test id: all of the shape, or chunk `chunk` of CHUNKS_4X4 of them."""
    n = n_blocks(W, H)
    if chunk is None:
        return range(n)
    per = n // CHUNKS_4X4
    return range(chunk * per, (chunk + 1) * per)


def case_ids():
    """(id, W, H, chunk): one per shape with W * H <= 12, CHUNKS_4X4 for 4 x 4 -- the same in the host and the GPU suite."""
    out = []
    for W, H in SHAPES:
        if has_ring(W, H):
            out.append((shape_name(W, H), W, H, None))
        else:
            out += [("%s-chunk%02d" % (shape_name(W, H), c), W, H, c) for c in range(CHUNKS_4X4)]
    return out


# ------------------------------------------------------------------ the C oracle on the fixture's queries
def oracle_grid(oracle, W, H, code, h, literal=False):
    """oracle.plan_batch of every query of one grid, one thread -> (length, cells [n, 2], cost, stats)."""
    s, g = queries(W, H)
    oc, ol, ocost, st = oracle.plan_batch(grid(W, H, code), s, g, h, literal=literal, max_len=MAX_LEN, nthreads=1, want_stats=True)
    return ol, padded_to_csr(oc, ol), ocost, st


def oracle_blocks(oracle, W, H, blocks, h, literal=False):
    """oracle_grid of every grid of `blocks`, THREADS blocks at a time (the ctypes call releases the GIL)
    -> {block: [oracle_grid of its grids, in code order]}."""
    from concurrent.futures import ThreadPoolExecutor
    blocks = list(blocks)
    with ThreadPoolExecutor(THREADS) as pool:
        out = pool.map(lambda b: [oracle_grid(oracle, W, H, c, h, literal) for c in block_codes(W, H, b)], blocks)
        return dict(zip(blocks, out))


def first_difference(W, H, code, h, got, want):
    """The first query of grid `code` on which two (length, cells, cost) triples differ, named; None when they agree."""
    s, g = queries(W, H)
    (gl, gc, gcost), (wl, wc, wcost) = got, want
    go, wo = np.concatenate([[0], np.cumsum(np.maximum(gl, 0))]), np.concatenate([[0], np.cumsum(np.maximum(wl, 0))])
    for q in range(len(s)):
        a, b = np.asarray(gc)[go[q]:go[q + 1]].tolist(), np.asarray(wc)[wo[q]:wo[q + 1]].tolist()
        if gl[q] != wl[q] or a != b or np.float64(gcost[q]).tobytes() != np.float64(wcost[q]).tobytes():
            return ("shape %dx%d grid code %d (occ %s) start %s goal %s hchoice %d: got len %d cells %s cost %r, want len %d cells %s cost %r"
                    % (W, H, code, grid(W, H, code).tolist(), s[q].tolist(), g[q].tolist(), h, gl[q], a, float(gcost[q]), wl[q], b, float(wcost[q])))
    return None
