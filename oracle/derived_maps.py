"""The library's derived grid maps recomputed on the host -- TEST INFRASTRUCTURE, NOT THE PRODUCT.

What a map holds comes from the C oracle alone: the goal-free jump() of every cell and direction, its forced-neighbour
and dblock tests (oracle.jump_table, jps1.py:14-38, 95-164) and the 4-connected components (oracle.components).  This
module only PACKS those answers into the device layouts that fxjps_debug_read_maps documents (include/fxjps.h) and
Planner.debug_maps returns, so that tests compare every byte of every map with an answer the device code had no part in:

    nb8   uint8[PW, PH]             bit nbit(dx, dy) = the neighbour (x+dx, y+dy) is occupied, off the grid = occupied
    bm    uint64[4, LINES, WORDS, 2] straight scan words {stop, occ}: +x, -x (line = padded y, bit = padded x), +y, -y
                                    (line = padded x, bit = padded y)
    ci    uint16[PW, PH]            cell infos
    dbm   uint64[4, DLINES, WORDS, 2] diagonal scan words {hit, die}: (+,+), (-,-), (+,-), (-,+), bit = padded x
    jd    uint16[PW, PH, 8]         jump-distance records
    comp  int32[W, H]               compared as a partition (roots), not byte for byte

PW = W + 2, PH = H + 2 (a one-cell occupied border), LINES = max(PW, PH), WORDS = ceil(LINES / 64), DLINES = PW + PH - 1.
Direction slots (nb8 bits, jd entries, jump tables): (-1,-1) 0, (-1,0) 1, (-1,1) 2, (0,-1) 3, (0,1) 4, (1,-1) 5, (1,0) 6,
(1,1) 7.
"""
import numpy as np

from . import oracle

SLOTS = ((-1, -1), (-1, 0), (-1, 1), (0, -1), (0, 1), (1, -1), (1, 0), (1, 1))
SLOT = {d: s for s, d in enumerate(SLOTS)}
STRAIGHT = ((1, 0), (-1, 0), (0, 1), (0, -1))  # bm directions 0 .. 3 and ci bits 8 .. 11
DIAGONAL = ((1, 1), (-1, -1), (1, -1), (-1, 1))  # dbm directions 0 .. 3
JD_K, JD_NB, JD_J = 0x1FFF, 0x6000, 0x8000


def layout(W, H):
    PW, PH = W + 2, H + 2
    LINES = max(PW, PH)
    tsh = 0  # read-set tiles: at most 64 x 64 of them cover the grid (fxjps.hip, alloc_grid_bufs)
    while ((max(W, H) - 1) >> tsh) > 63:
        tsh += 1
    return {"PW": PW, "PH": PH, "NS": (PH + 63) & ~63, "LINES": LINES, "WORDS": (LINES + 63) // 64, "DLINES": PW + PH - 1,
            "tsh": tsh}


def padded(a, fill, width=1):
    W, H = a.shape[:2]
    out = np.full((W + 2 * width, H + 2 * width) + a.shape[2:], fill, dtype=a.dtype)
    out[width:width + W, width:width + H] = a
    return out


def nb8_map(occ):
    """Neighbour bytes of every padded cell, the border and everything beyond it occupied."""
    W, H = occ.shape
    p2 = padded(np.asarray(occ != 0, np.uint8), 1, 2)
    out = np.zeros((W + 2, H + 2), np.uint8)
    for s, (dx, dy) in enumerate(SLOTS):
        out |= p2[1 + dx:W + 3 + dx, 1 + dy:H + 3 + dy] << s
    return out


def pack_lines(bits, words):
    """bool[lines, n] (n <= 64 * words) -> uint64[lines, words], bit i of word w = position 64 w + i; positions past n
    are 1."""
    lines, n = bits.shape
    full = np.ones((lines, words * 64), np.uint8)
    full[:, :n] = bits
    return np.packbits(full, axis=1, bitorder="little").view("<u8").reshape(lines, words)


def tile(p, tsh):
    return np.minimum(np.maximum((p - 1) >> tsh, 0), 63)


def reference_maps(occ, table=None):
    """The derived maps of grid `occ` (uint8[W, H], non-zero = obstacle) as Planner.debug_maps() returns them, from the
    oracle's jump table (oracle.jump_table(occ, flags=True), computed here unless given) and components."""
    occ = np.ascontiguousarray(occ != 0, dtype=np.uint8)
    W, H = occ.shape
    L = layout(W, H)
    PW, PH, WORDS, tsh = L["PW"], L["PH"], L["WORDS"], L["tsh"]
    found, k, flags = oracle.jump_table(occ, flags=True) if table is None else table
    occP = padded(occ, 1).astype(bool)
    foundP, kP, flagsP = padded(found, 0).astype(bool), padded(k, 0).astype(np.int64), padded(flags, 0)
    forcedP, dblockP = (flagsP & 1).astype(bool), (flagsP & 2).astype(bool)
    nb8 = nb8_map(occ)
    out = {"nb8": nb8}

    # straight scan words: stop = occupied or the forced-neighbour test of that travel direction
    bm = np.zeros((4, L["LINES"], WORDS, 2), np.uint64)
    for di, d in enumerate(STRAIGHT):
        s = SLOT[d]
        stop = occP | forcedP[:, :, s]
        if di < 2:  # line = padded y, bit = padded x
            bm[di, :PH, :, 0], bm[di, :PH, :, 1] = pack_lines(stop.T, WORDS), pack_lines(occP.T, WORDS)
        else:
            bm[di, :PW, :, 0], bm[di, :PW, :, 1] = pack_lines(stop, WORDS), pack_lines(occP, WORDS)
    out["bm"] = bm

    # cell infos: nb8 | straight goal-free found << 8 + i | read-set tile extents << 12 (x), << 14 (y); free cells only
    ci = nb8.astype(np.uint16)
    px, py = np.meshgrid(np.arange(PW), np.arange(PH), indexing="ij")
    info = np.zeros((PW, PH), np.uint16)
    for i, d in enumerate(STRAIGHT):
        info |= foundP[:, :, SLOT[d]].astype(np.uint16) << (8 + i)
    ex = np.maximum(np.maximum(tile(px + kP[:, :, SLOT[(1, 0)]], tsh) - tile(px, tsh),
                               tile(px, tsh) - tile(px - kP[:, :, SLOT[(-1, 0)]], tsh)), 0)
    ey = np.maximum(np.maximum(tile(py + kP[:, :, SLOT[(0, 1)]], tsh) - tile(py, tsh),
                               tile(py, tsh) - tile(py - kP[:, :, SLOT[(0, -1)]], tsh)), 0)
    info |= (np.minimum(ex, 3).astype(np.uint16) << 12) | (np.minimum(ey, 3).astype(np.uint16) << 14)
    ci[~occP] |= info[~occP]
    out["ci"] = ci

    # diagonal scan words: die = occupied or squeezed (dblock); hit = free and (forced or a straight sub-jump found)
    dbm = np.zeros((4, L["DLINES"], WORDS, 2), np.uint64)
    for dd, (dx, dy) in enumerate(DIAGONAL):
        s = SLOT[(dx, dy)]
        hit = ~occP & (forcedP[:, :, s] | foundP[:, :, SLOT[(dx, 0)]] | foundP[:, :, SLOT[(0, dy)]])
        die = occP | dblockP[:, :, s]
        line = (px - py + PH - 1) if dx == dy else (px + py)
        H2, D2 = np.zeros((L["DLINES"], WORDS * 64), bool), np.ones((L["DLINES"], WORDS * 64), bool)
        H2[line, px], D2[line, px] = hit, die
        dbm[dd, :, :, 0], dbm[dd, :, :, 1] = pack_lines(H2, WORDS), pack_lines(D2, WORDS)
    out["dbm"] = dbm

    # jump distances: steps to the cell the goal-free jump returned on | the cell's two neighbour bits (slots 0 .. 3) |
    # found << 15; the border's records are 0
    jd = (k.astype(np.uint32) & JD_K) | (found.astype(np.uint32) << 15)
    for s in range(4):
        jd[:, :, s] |= ((nb8[1:-1, 1:-1].astype(np.uint32) >> (2 * s)) & 3) << 13
    out["jd"] = padded(jd.astype(np.uint16), 0)
    out["comp"] = oracle.components(occ)
    return out


def decode_jd(jd):
    """jd uint16[PW, PH, 8] -> (found, k, neighbour bits) of the cells of the grid, [W, H, 8] each."""
    j = jd[1:-1, 1:-1].astype(np.uint32)
    return (j >> 15).astype(np.uint8), (j & JD_K).astype(np.uint16), ((j & JD_NB) >> 13).astype(np.uint8)


def roots(par):
    """Union-find parent links int32[W, H] -> the root of every cell (-1 where the link is -1), flat int64."""
    r = np.asarray(par).astype(np.int64).ravel().copy()
    idx = np.flatnonzero(r >= 0)
    while True:
        nxt = r[r[idx]]
        if np.array_equal(nxt, r[idx]):
            return r
        r[idx] = nxt


def _where(name, idx):
    if name in ("nb8", "ci"):
        return "cell (%d, %d)" % (idx[0] - 1, idx[1] - 1)
    if name == "jd":
        return "cell (%d, %d) direction %s" % (idx[0] - 1, idx[1] - 1, SLOTS[idx[2]])
    if name == "bm":
        di, line, w, f = idx
        return "%s word %d (%s): line %d" % (("+x", "-x", "+y", "-y")[di], w, ("stop", "occ")[f], line)
    di, line, w, f = idx
    return "%s diagonal %d word %d (%s)" % (DIAGONAL[di], line, w, ("hit", "die")[f])


def first_difference(dev, ref, names=("nb8", "bm", "ci", "dbm", "jd")):
    """None if the device maps equal the host reference, else a message naming the first differing field and cell."""
    for name in names:
        a, b = np.asarray(dev[name]), np.asarray(ref[name])
        if a.shape != b.shape:
            return "%s: shape %s, expected %s" % (name, a.shape, b.shape)
        bad = np.argwhere(a != b)
        if len(bad):
            idx = tuple(int(v) for v in bad[0])
            what = _where(name, idx)
            if name in ("bm", "dbm"):
                x = int(a[idx]) ^ int(b[idx])
                bit = (x & -x).bit_length() - 1
                pos = idx[2] * 64 + bit
                what += ", bit %d (padded position %d)" % (bit, pos)
            return "%s: %d entries differ, first at %s: device 0x%x, host 0x%x" % (name, len(bad), what, int(a[idx]), int(b[idx]))
    return None


def component_problem(comp, occ, exact, ever_free=None):
    """None if the device's union-find forest `comp` fits the host components of `occ`, else a message.
    exact: roots equal exactly where the host components are equal, and only cells that are free have one.  Otherwise
    sound: every host component lies under one root, every free cell has a root >= 0, and the cells never free since
    the forest was last built (~ever_free) have none."""
    occ = np.asarray(occ) != 0
    host = oracle.components(occ.astype(np.uint8)).ravel()
    r = roots(comp)
    free = np.flatnonzero(~occ.ravel())
    if (r[free] < 0).any():
        c = int(free[np.flatnonzero(r[free] < 0)[0]])
        return "free cell (%d, %d) has no root" % divmod(c, occ.shape[1])
    never_free = occ.ravel() if exact else (None if ever_free is None else ~np.asarray(ever_free).ravel())
    if never_free is not None and (never_free & (r >= 0)).any():
        c = int(np.flatnonzero(never_free & (r >= 0))[0])
        return "cell (%d, %d) has a root but was not free" % divmod(c, occ.shape[1])
    pairs = np.unique(np.stack([host[free], r[free]]), axis=1)
    if pairs.shape[1] != len(np.unique(host[free])):  # a host component under two roots
        h = pairs[0][np.flatnonzero(np.diff(pairs[0]) == 0)[0]]
        return "host component of cell (%d, %d) is split over several roots" % divmod(int(h), occ.shape[1])
    if exact and pairs.shape[1] != len(np.unique(r[free])):
        rr = np.unique(pairs[1], return_counts=True)
        bad = rr[0][rr[1] > 1][0]
        cs = pairs[0][pairs[1] == bad][:2]
        return "cells (%d, %d) and (%d, %d) share a root across host components" % (divmod(int(cs[0]), occ.shape[1]) + divmod(int(cs[1]), occ.shape[1]))
    return None
