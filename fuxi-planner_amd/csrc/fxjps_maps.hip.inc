// fxjps_maps.hip.inc -- device code of libfxjps.so around the search (included at the end of fxjps_kernels.hip.inc, inside
// namespace fx): the derived maps of a grid (scan words along rows, columns and diagonals, cell infos, jump-distance records),
// their partial rebuild after cell updates, the 4-connected component labels, the merged launches of a small grid's build,
// the callers' grid preparation, the wire / image adapters, and the ccst node's waypoint selection (DESIGN.md sections 3.2 - 3.5).
// Split off the search kernel's file in round 6; nothing in it is used by the search.

// ---------------------------------------------------------------- derived maps
// A rectangle of the derived maps: the lines l0 .. l1 and, of each, the words w0 .. w1 (k_derive_rows / _cols), or the
// padded cells x0 .. x1 by y0 .. y1 (k_derive_cellinfo).  The whole map after fxjps_set_grid; after a cell update only
// what the changed cells can reach (SURVEY K3): neighbour bytes and stop bits depend on the occupancy within Chebyshev
// distance 1, the straight-jump bits of a cell's info on its whole row and column.
struct MapRange {
    int32_t l0, l1, w0, w1;
};

// One wavefront per 64-bit word of a padded row (line = padded x, lane = padded y): neighbour bytes
// and the +y / -y scan words.
__device__ __forceinline__ void derive_rows_item(const uint8_t* __restrict__ occ, const GridDev& G, uint8_t* __restrict__ nb8,
                                                 BmWord* __restrict__ bm, const MapRange& R, long long wid, int lane) {
    const int nw = R.w1 - R.w0 + 1;
    if (wid >= (long long)(R.l1 - R.l0 + 1) * nw) return;
    const int px = R.l0 + (int)(wid / nw), w = R.w0 + (int)(wid % nw);
    const int py = w * 64 + lane;
    const int W = G.W, H = G.H;
    auto O = [&](int ax, int ay) -> uint32_t {  // padded coords; outside the real grid == occupied
        const int x = ax - 1, y = ay - 1;
        if (x < 0 || y < 0 || x >= W || y >= H) return 1u;
        return occ[(size_t)x * H + y] != 0;
    };
    uint32_t m = 0;
    const bool inside = py < G.PH;
#pragma unroll
    for (int dx = -1; dx <= 1; dx++)
#pragma unroll
        for (int dy = -1; dy <= 1; dy++)
            if (dx != 0 || dy != 0) m |= (inside ? O(px + dx, py + dy) : 1u) << nbit(dx, dy);
    const uint32_t self = inside ? O(px, py) : 1u;
    if (inside) nb8[(size_t)px * G.NS + py] = (uint8_t)m;
    // forced when travelling (0,dy): jps1.py:150-153 with blocked() expanded on the mask
    auto forcedY = [&](int dy) -> bool {
        const bool ahead = occN(m, 0, dy);
        return (occN(m, 1, 0) && !occN(m, 1, dy) && !ahead) || (occN(m, -1, 0) && !occN(m, -1, dy) && !ahead);
    };
    const uint64_t bo = __ballot(self != 0);
    const uint64_t bp = __ballot(self != 0 || forcedY(1));
    const uint64_t bn = __ballot(self != 0 || forcedY(-1));
    if (lane == 0) {
        BmWord u;
        u.occ = bo;
        u.stop = bp;
        bm[(size_t)(2 * G.LINES + px) * G.WORDS + w] = u;
        u.stop = bn;
        bm[(size_t)(3 * G.LINES + px) * G.WORDS + w] = u;
    }
}
__global__ __launch_bounds__(256) void k_derive_rows(const uint8_t* __restrict__ occ, GridDev G, uint8_t* __restrict__ nb8,
                                                    BmWord* __restrict__ bm, MapRange R) {
    derive_rows_item(occ, G, nb8, bm, R, (long long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6), (int)(threadIdx.x & 63));
}

// One wavefront per 64-bit word of a padded column (line = padded y, lane = padded x): +x / -x scan words.
template <bool FROM_OCC>  // the neighbour byte: read (k_derive_rows wrote it) or computed here (the fused build: beside the rows)
__device__ __forceinline__ void derive_cols_item(const uint8_t* __restrict__ occ, const GridDev& G, BmWord* __restrict__ bm, const MapRange& R,
                                                 long long wid, int lane) {
    const int nw = R.w1 - R.w0 + 1;
    if (wid >= (long long)(R.l1 - R.l0 + 1) * nw) return;
    const int py = R.l0 + (int)(wid / nw), w = R.w0 + (int)(wid % nw);
    const int px = w * 64 + lane;
    const bool inside = px < G.PW;
    uint32_t m = 0xFF, self = 1;
    if (inside) {
        const int x = px - 1, y = py - 1;
        self = (x < 0 || y < 0 || x >= G.W || y >= G.H) ? 1u : (occ[(size_t)x * G.H + y] != 0);
        if (FROM_OCC) {
            m = 0;
#pragma unroll
            for (int dx = -1; dx <= 1; dx++)
#pragma unroll
                for (int dy = -1; dy <= 1; dy++)
                    if (dx != 0 || dy != 0) {
                        const int ax = x + dx, ay = y + dy;
                        const uint32_t o = (ax < 0 || ay < 0 || ax >= G.W || ay >= G.H) ? 1u : (occ[(size_t)ax * G.H + ay] != 0);
                        m |= o << nbit(dx, dy);
                    }
        } else {
            m = G.nb8[(size_t)px * G.NS + py];
        }
    }
    // forced when travelling (dx,0): jps1.py:134-137
    auto forcedX = [&](int dx) -> bool {
        const bool ahead = occN(m, dx, 0);
        return (occN(m, 0, 1) && !occN(m, dx, 1) && !ahead) || (occN(m, 0, -1) && !occN(m, dx, -1) && !ahead);
    };
    const uint64_t bo = __ballot(self != 0);
    const uint64_t bp = __ballot(self != 0 || forcedX(1));
    const uint64_t bn = __ballot(self != 0 || forcedX(-1));
    if (lane == 0) {
        BmWord u;
        u.occ = bo;
        u.stop = bp;
        bm[(size_t)(0 * G.LINES + py) * G.WORDS + w] = u;
        u.stop = bn;
        bm[(size_t)(1 * G.LINES + py) * G.WORDS + w] = u;
    }
}
__global__ __launch_bounds__(256) void k_derive_cols(const uint8_t* __restrict__ occ, GridDev G, BmWord* __restrict__ bm, MapRange R) {
    derive_cols_item<false>(occ, G, bm, R, (long long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6), (int)(threadIdx.x & 63));
}

// Cell info map.  One thread per padded cell: low byte = neighbour mask, bits 8..11 = result of the
// goal-free straight jump (jps1.py:95-162 with dX*dY == 0) from this cell along +x, -x, +y, -y.
// After a cell update (C.map != nullptr) the kernel also says WHICH cells changed: every cell of the update's box B (its
// occupancy, neighbour byte and scan bits may differ) and every cell of the rows / columns through it whose info came out
// different (a straight jump from it ends elsewhere now) -- the cells whose diagonal scan bits can differ, which is what
// the jump distances are re-scanned from (k_jd_walk).  A changed cell is marked in C.map (one byte per padded cell, zero
// at rest) and appended to C.list.
struct ChangeOut {
    uint8_t* map;        // [PW][NS], nullptr: nothing is recorded
    uint32_t* list;      // px * NS + py of the changed cells
    unsigned int* cnt;   // [0] entries of the list, [1] "re-scan by streaming the table", [2] blocks of k_jd_finish that are through, [3] entries of ovf
    uint32_t cap;
    MapRange B;          // the cells this launch marks whether their info changed or not (l0 > l1: none)
    uint32_t* ovf;       // walks that outgrew their bound: (changed cell, direction | next step << 3), carried on by k_jd_finish
    uint32_t ovf_cap;    // (more of them than this: cnt[1], the table is streamed)
};
// Two rectangles in one launch (after a cell update: the rows through the box, then the columns through it; the cells
// of the columns that lie in those rows belong to the first).  R2.l0 > R2.l1: one rectangle.
__device__ __forceinline__ void derive_cellinfo_item(const GridDev& G, uint16_t* __restrict__ ci, const MapRange& R, const MapRange& R2, const ChangeOut& C,
                                                     long long i, int lane_) {  // x l0 .. l1, y w0 .. w1
    const long long n1 = (long long)(R.l1 - R.l0 + 1) * (R.w1 - R.w0 + 1);
    const bool second = i >= n1;
    if (second) {
        i -= n1;
        if (R2.l0 > R2.l1 || i >= (long long)(R2.l1 - R2.l0 + 1) * (R2.w1 - R2.w0 + 1)) return;
    }
    const MapRange Q = second ? R2 : R;
    const int ny = Q.w1 - Q.w0 + 1;
    const int px = Q.l0 + (int)(i / ny), py = Q.w0 + (int)(i % ny);
    if (second && px >= R.l0 && px <= R.l1 && py >= R.w0 && py <= R.w1) return;  // (done by the first rectangle's thread)
    const size_t at = (size_t)px * G.NS + py;
    uint32_t v = G.nb8[at];
    const bool self_occ = (G.bm[(size_t)(2 * G.LINES + px) * G.WORDS + (py >> 6)].occ >> (py & 63)) & 1ull;
    const bool inB = px >= C.B.l0 && px <= C.B.l1 && py >= C.B.w0 && py <= C.B.w1;
    // After an update a cell outside the box keeps the half of its info whose rays cannot have met a changed cell: a cell of
    // the rows through the box (same x as the box, another y) sends its +-x rays along a line of cells with that other y --
    // none of them in the box, whose cells are the only ones whose scan bits changed; likewise the +-y rays of a cell of the
    // columns through it.  Half the scans.
    const bool keep_x = C.map != nullptr && !inB && !second, keep_y = C.map != nullptr && !inB && second;
    if (!self_occ) {
        int rp;
        const auto tile = [&](int p) { return min(max((p - 1) >> G.tsh, 0), 63); };
        int ex = 0, ey = 0;  // read-set tiles beyond the cell's own that its rays reach (they end at rp, inclusive)
        if (keep_x) {
            v |= (uint32_t)ci[at] & 0x3300u;
        } else {
            if (scan_ray(G, px, py, 1, 0, -1000, -1000, &rp)) v |= 1u << 8;
            ex = max(ex, tile(rp) - tile(px));
            if (scan_ray(G, px, py, -1, 0, -1000, -1000, &rp)) v |= 1u << 9;
            ex = max(ex, tile(px) - tile(rp));
            v |= (uint32_t)min(ex, 3) << 12;
        }
        if (keep_y) {
            v |= (uint32_t)ci[at] & 0xCC00u;
        } else {
            if (scan_ray(G, px, py, 0, 1, -1000, -1000, &rp)) v |= 1u << 10;
            ey = max(ey, tile(rp) - tile(py));
            if (scan_ray(G, px, py, 0, -1, -1000, -1000, &rp)) v |= 1u << 11;
            ey = max(ey, tile(py) - tile(rp));
            v |= (uint32_t)min(ey, 3) << 14;
        }
    }
    if (C.map != nullptr) {
        const bool flag = px >= 1 && py >= 1 && px <= G.W && py <= G.H  // (the border never changes)
                          && (inB || (uint32_t)ci[at] != v) && C.map[at] == 0;
        const uint64_t fm = __ballot(flag);  // (the lanes that are here: one addition to the counter per wavefront)
        if (fm != 0ull) {
            const int leader = (int)__builtin_ctzll(fm), lane = lane_;
            uint32_t base = 0;
            if (lane == leader) base = atomicAdd(&C.cnt[0], (unsigned int)__popcll(fm));
            base = (uint32_t)__shfl((int)base, leader, 64);
            const uint32_t j = base + (uint32_t)__popcll(fm & ((1ull << lane) - 1ull));
            if (flag && j < C.cap) {  // (a mark without a list entry would never be taken back)
                C.list[j] = (uint32_t)at;
                C.map[at] = 1;
            }
        }
    }
    ci[at] = (uint16_t)v;
}
__global__ __launch_bounds__(256) void k_derive_cellinfo(GridDev G, uint16_t* __restrict__ ci, MapRange R, MapRange R2, ChangeOut C) {
    derive_cellinfo_item(G, ci, R, R2, C, (long long)blockIdx.x * blockDim.x + threadIdx.x, (int)(threadIdx.x & 63));
}

// Per-direction constants of a diagonal ray, as neighbour-mask bit patterns (see nbit()):
//   forced (jps1.py:110-113)  <=>  (m & K1) == A1  ||  (m & K2) == A2
//   dblock (jps1.py:35)       <=>  (m & (A1|A2)) == (A1|A2)
struct DiagConst {
    uint32_t K1, A1, K2, A2, NX, SUB;
};
template <int DX, int DY>
__host__ __device__ constexpr DiagConst diag_const() {
    return DiagConst{(1u << nbit(-DX, 0)) | (1u << nbit(0, DY)) | (1u << nbit(-DX, DY)), 1u << nbit(-DX, 0),
                     (1u << nbit(0, -DY)) | (1u << nbit(DX, 0)) | (1u << nbit(DX, -DY)), 1u << nbit(0, -DY),
                     1u << nbit(DX, DY), (DX > 0 ? 0x100u : 0x200u) | (DY > 0 ? 0x400u : 0x800u)};
}
// index of a diagonal travel direction among the diagonal scan lines: (+,+) 0, (-,-) 1, (+,-) 2, (-,+) 3
__device__ __forceinline__ int ddir_index(int dx, int dy) { return (dx == dy ? 0 : 2) + (dx > 0 ? 0 : 1); }
// the diagonal through padded cell (px, py) for that direction
__device__ __forceinline__ int dline_of(int px, int py, int dx, int dy, int PH) { return dx == dy ? px - py + PH - 1 : px + py; }

// Diagonal scan words (round 4).  What the loop of a diagonal jump (jps1.py:108-130) decides at a cell o it steps on
// depends on o alone -- its occupancy, its eight neighbours and whether a goal-free straight jump from o along either
// axis of the direction finds anything (bits 8-11 of the cell info): exactly the bit patterns the stepping form of the
// search evaluated cell by cell.  So, per direction and cell:
//     occ  ("die")  = o is occupied, or the step onto o squeezed between two obstacles (dblock, :126)
//     stop ("hit")  = o is free and (a forced neighbour, :110-113, or a straight sub-jump that is not None, :116-117)
// packed along the diagonals, and a diagonal jump without the goal is a find-first-set like a straight one: the first
// cell with either bit, a jump point unless its die bit is set.  The goal (its own cell, and the cells of the ray on its
// row and column, whose sub-jumps may reach it) and the first step (no dblock there, :97-103) are the caller's business.
// One wavefront per word: lane = padded x.  R: the words of the lines to redo -- everything, or after a cell update the
// words that hold cells of the rows x0 .. x1 or of the columns y0 .. y1 (whose cell infos were rebuilt).
struct DiagRange {
    int32_t whole, x0, x1, y0, y1;
};
__device__ __forceinline__ void derive_diag_item(const uint8_t* __restrict__ occ, const GridDev& G, BmWord* __restrict__ dbm, const DiagRange& R, long long wid,
                                                 int lane) {
    const int nwx = R.whole ? G.WORDS : (R.x1 >> 6) - (R.x0 >> 6) + 1;
    const int nwy = R.whole ? 0 : ((R.y1 - R.y0 + 63) >> 6) + 1;  // words that the columns y0 .. y1 can touch on one diagonal, at most
    const int per = nwx + nwy;
    if (wid >= (long long)4 * G.DLINES * per) return;
    // Consecutive wavefronts (the sixteen of a block) take the SAME word of consecutive diagonals: lane x of all of them reads
    // row x of the cell infos and of the grid at neighbouring y -- one cache line for the block instead of one per wavefront
    // (round 6: word-major order, where a block's wavefronts shared nothing, made this the slowest kernel of a map build --
    // 30 of 112 us at 256 x 256).
    const int L = (int)(wid % G.DLINES);
    const int slot = (int)((wid / G.DLINES) % per), dd = (int)(wid / ((long long)per * G.DLINES));
    const int dx = (dd == 0 || dd == 2) ? 1 : -1, dy = (dd == 0 || dd == 3) ? 1 : -1;
    int w;
    if (R.whole) {
        w = slot;
    } else if (slot < nwx) {
        w = (R.x0 >> 6) + slot;
    } else {  // the x positions of the cells of this diagonal in the columns y0 .. y1
        const int xa = dx == dy ? L - (G.PH - 1) + R.y0 : L - R.y1, xb = dx == dy ? L - (G.PH - 1) + R.y1 : L - R.y0;
        if (xb < 0 || xa >= G.PW) return;
        w = (max(xa, 0) >> 6) + (slot - nwx);
        if (w > (min(xb, G.PW - 1) >> 6)) return;
    }
    if (w < 0 || w >= G.WORDS) return;
    const int px = w * 64 + lane;
    const int py = dx == dy ? px - L + (G.PH - 1) : L - px;
    const bool inside = px < G.PW && py >= 0 && py < G.PH;
    bool hit = false, die = true;
    if (inside) {
        const int x = px - 1, y = py - 1;
        const bool self = (x < 0 || y < 0 || x >= G.W || y >= G.H) ? true : (occ[(size_t)x * G.H + y] != 0);
        const uint32_t m = G.ci[(size_t)px * G.NS + py];
        constexpr DiagConst cpp = diag_const<1, 1>(), cmm = diag_const<-1, -1>(), cpm = diag_const<1, -1>(), cmp = diag_const<-1, 1>();
        const DiagConst c = dd == 0 ? cpp : dd == 1 ? cmm : dd == 2 ? cpm : cmp;
        const bool dbl = (m & (c.A1 | c.A2)) == (c.A1 | c.A2);
        const bool forced = ((m & c.K1) == c.A1) || ((m & c.K2) == c.A2);
        hit = !self && (forced || (m & c.SUB) != 0u);
        die = self || dbl;
    }
    const uint64_t bh = __ballot(hit), bd = __ballot(die);
    if (lane == 0) {
        BmWord u;
        u.stop = bh;
        u.occ = bd;
        dbm[(size_t)(dd * G.DLINES + L) * G.WORDS + w] = u;
    }
}
__global__ __launch_bounds__(1024) void k_derive_diag(const uint8_t* __restrict__ occ, GridDev G, BmWord* __restrict__ dbm, DiagRange R) {
    derive_diag_item(occ, G, dbm, R, (long long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6), (int)(threadIdx.x & 63));
}

// The same bits for the cells a cell update changed (k_derive_cellinfo's list: the update's box and the cells of the rows /
// columns through it whose info came out different), one thread per (cell, direction): the cell's two bits are set or
// cleared in place.  (k_derive_diag over every word that holds a cell of those rows and columns -- 164 k words for a
// 64 x 64 window on a 4096 x 4096 map, read along the diagonals -- took 81 us of such an update's 214.)
__global__ __launch_bounds__(256) void k_diag_update(const uint8_t* __restrict__ occ, GridDev G, BmWord* __restrict__ dbm, ChangeOut C) {
    const uint32_t n = min(C.cnt[0], C.cap);
    if (blockIdx.x == 0 && threadIdx.x == 0) {  // (k_jd_walk, next, raises them; k_jd_finish, behind that, reads them)
        C.cnt[1] = 0u;
        C.cnt[3] = 0u;
    }
    for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x; t < (long long)n * 4; t += (long long)gridDim.x * blockDim.x) {
        const uint32_t at = C.list[t >> 2];
        const int dd = (int)(t & 3);
        const int px = (int)(at / (uint32_t)G.NS), py = (int)(at % (uint32_t)G.NS);  // (in the grid: the list holds no border cells)
        const int dx = (dd == 0 || dd == 2) ? 1 : -1, dy = (dd == 0 || dd == 3) ? 1 : -1;
        const bool self = occ[(size_t)(px - 1) * G.H + (py - 1)] != 0;
        const uint32_t m = G.ci[at];
        constexpr DiagConst cpp = diag_const<1, 1>(), cmm = diag_const<-1, -1>(), cpm = diag_const<1, -1>(), cmp = diag_const<-1, 1>();
        const DiagConst c = dd == 0 ? cpp : dd == 1 ? cmm : dd == 2 ? cpm : cmp;
        const bool dbl = (m & (c.A1 | c.A2)) == (c.A1 | c.A2);
        const bool forced = ((m & c.K1) == c.A1) || ((m & c.K2) == c.A2);
        const bool hit = !self && (forced || (m & c.SUB) != 0u);
        const bool die = self || dbl;
        BmWord* w = dbm + (size_t)(dd * G.DLINES + dline_of(px, py, dx, dy, G.PH)) * G.WORDS + (px >> 6);
        const unsigned long long bit = 1ull << (px & 63);
        unsigned long long* ws = reinterpret_cast<unsigned long long*>(&w->stop);
        unsigned long long* wo = reinterpret_cast<unsigned long long*>(&w->occ);
        if (hit) atomicOr(ws, bit); else atomicAnd(ws, ~bit);
        if (die) atomicOr(wo, bit); else atomicAnd(wo, ~bit);
    }
}

// A diagonal jump (jps1.py:108-130) without the goal's row / column business, on the diagonal scan words (k_derive_diag):
// the first cell at or after `pos` (padded x) on diagonal L of travel direction dd that ends the jump; true iff the jump
// returns that cell.  first_occ: occupancy of the first cell -- the first step knows no dblock (:97-103), so there the
// die bit is the occupancy alone.  gpos: the goal's padded x if it lies on this diagonal, else -1.
__device__ __forceinline__ bool scan_diag(const GridDev& G, int dd, int L, int pos, int sgn, uint32_t first_occ, int gpos, int* rp) {
    const BmWord* Lp = G.bm + (size_t)(4 * G.LINES + dd * G.DLINES + L) * G.WORDS;
    int w = pos >> 6;
    const int b = pos & 63;
    uint64_t m = sgn > 0 ? (~0ull << b) : (~0ull >> (63 - b));
    const int gw = gpos >> 6;
    const uint64_t gbit = gpos >= 0 ? (1ull << (gpos & 63)) : 0ull;
    bool first = true;
    while (w >= 0 && w < G.WORDS) {
        const BmWord u = Lp[w];
        uint64_t hit = u.stop, die = u.occ;
        if (first) die = (die & ~(1ull << b)) | ((uint64_t)first_occ << b);
        if (w == gw) hit |= gbit;
        const uint64_t s = (hit | die) & m;
        if (s) {
            const int bit = sgn > 0 ? __builtin_ctzll(s) : 63 - __builtin_clzll(s);
            *rp = w * 64 + bit;
            return !((die >> bit) & 1ull);
        }
        w += sgn;
        m = ~0ull;
        first = false;
    }
    *rp = -1;
    return false;  // unreachable: the border always stops the ray
}

// ---- jump distances (round 4): the goal-free result of jump(c, d) for every cell and direction, one u16 each, the eight of a
// cell in one 16-byte record -- so the rays of a node are ONE memory request (and on grids whose scan words miss the caches,
// config 3, requests are what the chip runs out of), and a lane's expansion is a load and an addition instead of masks and a
// find-first-set.  The goal is the caller's business (expand_jd): on the ray before the stop it is the jump point; the cells
// of a diagonal ray on its row and column are looked at with the scan words as before.
__device__ __forceinline__ uint32_t jd_entry(const GridDev& G, int px, int py, int slot) {
    const int code = jd_code(slot), dx = (code >> 2) - 1, dy = (code & 3) - 1;
    int rp = -1;
    bool jp;
    if (dx != 0 && dy != 0) {
        const uint32_t nbm = G.nb8[(size_t)px * G.NS + py];
        jp = scan_diag(G, ddir_index(dx, dy), dline_of(px, py, dx, dy, G.PH), px + dx, dx, occN(nbm, dx, dy) ? 1u : 0u, -1, &rp);
    } else {
        jp = scan_ray(G, px, py, dx, dy, -1000, -1000, &rp);
    }
    const int k = rp >= 0 ? abs(rp - (dx != 0 ? px : py)) : 0;  // (0: the ray found nothing at all -- cannot happen inside the border)
    // bits 13-14 of the first four entries: the cell's neighbour byte, two bits each -- whoever reads the record to expand
    // the cell has what nodeNeighbours (jps1.py:49-93) needs, without a read of the cell info
    const uint32_t nbits = slot < 4 ? ((((uint32_t)G.nb8[(size_t)px * G.NS + py]) >> (2 * slot)) & 3u) << 13 : 0u;
    return (uint32_t)k | nbits | (jp ? JD_J : 0u);
}
// One thread per (cell, direction).  whole == 0: only the entries whose OLD ray passes a cell whose scan bits a cell update
// can have changed (the update's box for the straight rays; for the diagonal rays the rows and the columns through it,
// whose cell infos -- and with them the diagonal scan words -- were rebuilt): a scan reads nothing beyond the cell that
// ended it, so an entry whose old ray misses all of them stands.
__device__ __forceinline__ void derive_jd_item(const GridDev& G, uint16_t* __restrict__ jd, const DiagRange& R, long long i) {
    if (i >= (long long)G.PW * G.PH * 8) return;
    const int slot = (int)(i & 7);
    const long long cell = i >> 3;
    const int px = (int)(cell / G.PH), py = (int)(cell % G.PH);
    const size_t at = ((size_t)px * G.NS + py) * 8 + slot;
    if (px < 1 || py < 1 || px > G.W || py > G.H) {  // the border: never a node
        if (R.whole) jd[at] = 0;
        return;
    }
    if (!R.whole) {
        const uint32_t v = jd[at];
        const int k = (int)(v & JD_K);
        const int code = jd_code(slot), dx = (code >> 2) - 1, dy = (code & 3) - 1;
        const int xa = min(px + dx, px + k * dx), xb = max(px + dx, px + k * dx), ya = min(py + dy, py + k * dy), yb = max(py + dy, py + k * dy);
        const bool xin = xa <= R.x1 && xb >= R.x0, yin = ya <= R.y1 && yb >= R.y0;
        const bool self = px >= R.x0 && px <= R.x1 && py >= R.y0 && py <= R.y1;
        const bool hit = k == 0 || self || ((dx != 0 && dy != 0) ? (xin || yin) : (xin && yin));
        if (!hit) return;
    }
    jd[at] = (uint16_t)jd_entry(G, px, py, slot);
}
__global__ __launch_bounds__(256) void k_derive_jd(GridDev G, uint16_t* __restrict__ jd, DiagRange R) {
    derive_jd_item(G, jd, R, (long long)blockIdx.x * blockDim.x + threadIdx.x);
}
// The same for what a cell update can have changed (DiagRange::whole == 0), one thread per CELL: it reads the cell's
// 16-byte record once, tests the eight old rays against the update's box / cross with a few comparisons each, and
// re-scans the few that pass it (a 64 x 64 window on a 4096 x 4096 map: 268 MB streamed, a few thousand scans).
__global__ __launch_bounds__(256) void k_update_jd(GridDev G, uint16_t* __restrict__ jd, DiagRange R) {
    const long long cell = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (cell >= (long long)G.W * G.H) return;
    const int px = (int)(cell / G.H) + 1, py = (int)(cell % G.H) + 1;
    uint16_t* rec = jd + ((size_t)px * G.NS + py) * 8;
    const uint4 v4 = *reinterpret_cast<const uint4*>(rec);
    const uint32_t w[4] = {v4.x, v4.y, v4.z, v4.w};
    const bool self = px >= R.x0 && px <= R.x1 && py >= R.y0 && py <= R.y1;
#pragma unroll
    for (int slot = 0; slot < 8; slot++) {
        const int k = (int)((w[slot >> 1] >> ((slot & 1) * 16)) & JD_K);
        const int code = jd_code(slot), dx = (code >> 2) - 1, dy = (code & 3) - 1;
        const int xa = min(px + dx, px + k * dx), xb = max(px + dx, px + k * dx), ya = min(py + dy, py + k * dy), yb = max(py + dy, py + k * dy);
        const bool xin = xa <= R.x1 && xb >= R.x0, yin = ya <= R.y1 && yb >= R.y0;
        const bool hit = k == 0 || self || ((dx != 0 && dy != 0) ? (xin || yin) : (xin && yin));
        if (hit) rec[slot] = (uint16_t)jd_entry(G, px, py, slot);
    }
}

// ---- the jump distances after a cell update, without streaming the table (round 5).  An entry (c, d) stands unless its
// OLD ray -- the cells c + d .. c + k d -- holds a cell whose scan bits for that kind of line changed: a cell of the
// update's box B for a straight d, a changed cell (k_derive_cellinfo's list: B, and the cells of the rows / columns through
// it whose info differs) for a diagonal d.  So the work starts at the changed cells and walks BACK along -d: c_i = e - i d
// is affected iff its old distance reaches e (k >= i), and once a cell's ray does not reach e no cell behind it does -- a
// ray from further back runs through the same cells with the same bits (a diagonal ray sees the squeeze test, dblock
// jps1.py:126, on every cell but its first: it stops sooner, never later).  A walk also ends at the next changed cell:
// what lies behind that one is reached from it.  Every (c, d) is therefore visited by ONE walker, which re-scans it in
// place; nobody else reads it (different d: different u16 of the record).  One thread per (changed cell, direction).
// Walks are short where maps are cluttered (a 64 x 64 window on the 4096^2 map of config 3: 5 k changed cells, 40 k
// walkers, a handful of steps each, instead of 268 MB of records).  On open maps a ray -- and a walk -- can be as long as
// the map: a walker that is not done after JD_WALK_MAX steps hands the rest of its line to k_jd_finish (ChangeOut::ovf),
// where a wavefront takes it 64 cells at a time -- the cells behind one another are independent tests of OLD entries, and
// the walk ends at the first of them that fails, so a chunk is one ballot.  Only when that list is full too (ovf_cap
// walks) cnt[1] is raised and k_jd_finish re-scans the old way (every record, k_update_jd's test): all three re-scan
// entries from the final scan words, so they mix freely.
#ifndef FXJPS_JD_WALK_MAX
#define FXJPS_JD_WALK_MAX 96
#endif
__global__ __launch_bounds__(256) void k_jd_walk(GridDev G, uint16_t* __restrict__ jd, ChangeOut C, DiagRange R, int walk_max, uint32_t stream_over) {
    const uint32_t n = min(C.cnt[0], C.cap);
    // More changed cells than `stream_over` (an open map: whole rows and columns through the box end their jumps elsewhere
    // now): eight walks from each of them cost more than reading every record once -- streamed up front, no walk at all.
    // (cnt[0] > cap cannot happen: the list is sized for every cell the launches visit.)
    if (C.cnt[0] > C.cap || n > stream_over) {
        if (blockIdx.x == 0 && threadIdx.x == 0) C.cnt[1] = 1u;
        return;
    }
    for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x; t < (long long)n * 8; t += (long long)gridDim.x * blockDim.x) {
        const uint32_t at = C.list[t >> 3];
        const int slot = (int)(t & 7);
        const int ex = (int)(at / (uint32_t)G.NS), ey = (int)(at % (uint32_t)G.NS);
        const int code = jd_code(slot), dx = (code >> 2) - 1, dy = (code & 3) - 1;
        const bool inB = ex >= R.x0 && ex <= R.x1 && ey >= R.y0 && ey <= R.y1;
        if (inB) jd[(size_t)at * 8 + slot] = (uint16_t)jd_entry(G, ex, ey, slot);  // its own rays: the first step, the neighbour byte in the spare bits
        if (dx * dy == 0 && !inB) continue;  // (straight scan bits change inside the box only)
        int cx = ex - dx, cy = ey - dy;
        for (int i = 1; cx >= 1 && cy >= 1 && cx <= G.W && cy <= G.H; i++, cx -= dx, cy -= dy) {
            if (cx >= R.x0 && cx <= R.x1 && cy >= R.y0 && cy <= R.y1) break;  // a cell of the box: re-scanned as such
            const size_t ca = (size_t)cx * G.NS + cy;
            const int k = (int)(jd[ca * 8 + slot] & JD_K);
            if (k != 0 && k < i) break;
            jd[ca * 8 + slot] = (uint16_t)jd_entry(G, cx, cy, slot);
            if (dx * dy != 0 && C.map[ca] != 0) break;  // the next changed cell of this diagonal: its walker goes on from here
            if (i >= walk_max) {  // a long ray of an open map: a wavefront of k_jd_finish carries on, 64 cells at a time
                const uint32_t o = atomicAdd(&C.cnt[3], 1u);
                if (o < C.ovf_cap) {
                    C.ovf[2 * o] = at;
                    C.ovf[2 * o + 1] = (uint32_t)slot | ((uint32_t)(i + 1) << 3);
                } else {
                    C.cnt[1] = 1u;
                }
                break;
            }
        }
    }
}
// Behind the walk: the old way if a walker gave up (else the blocks leave at once), then the marks are taken back.
__global__ __launch_bounds__(256) void k_jd_finish(GridDev G, uint16_t* __restrict__ jd, ChangeOut C, DiagRange R) {
    if (C.cnt[1] != 0u) {  // (cleared by the next update's k_diag_update: every block of this launch may still look at it)
        for (long long cell = (long long)blockIdx.x * blockDim.x + threadIdx.x; cell < (long long)G.W * G.H; cell += (long long)gridDim.x * blockDim.x) {
            const int px = (int)(cell / G.H) + 1, py = (int)(cell % G.H) + 1;
            uint16_t* rec = jd + ((size_t)px * G.NS + py) * 8;
            const uint4 v4 = *reinterpret_cast<const uint4*>(rec);
            const uint32_t w[4] = {v4.x, v4.y, v4.z, v4.w};
            const bool self = px >= R.x0 && px <= R.x1 && py >= R.y0 && py <= R.y1;
#pragma unroll
            for (int slot = 0; slot < 8; slot++) {
                const int k = (int)((w[slot >> 1] >> ((slot & 1) * 16)) & JD_K);
                const int code = jd_code(slot), dx = (code >> 2) - 1, dy = (code & 3) - 1;
                const int xa = min(px + dx, px + k * dx), xb = max(px + dx, px + k * dx), ya = min(py + dy, py + k * dy), yb = max(py + dy, py + k * dy);
                const bool xin = xa <= R.x1 && xb >= R.x0, yin = ya <= R.y1 && yb >= R.y0;
                const bool hit = k == 0 || self || ((dx != 0 && dy != 0) ? (xin || yin) : (xin && yin));
                if (hit) rec[slot] = (uint16_t)jd_entry(G, px, py, slot);
            }
        }
    } else {
        // the walks that outgrew k_jd_walk's bound, one wavefront each: step i of the walk on lane i - base
        const uint32_t no = min(C.cnt[3], C.ovf_cap);
        const uint32_t lane = threadIdx.x & 63u, nwv = (gridDim.x * blockDim.x) >> 6;
        for (uint32_t o = (blockIdx.x * blockDim.x + threadIdx.x) >> 6; o < no; o += nwv) {
            const uint32_t at = C.ovf[2 * o], pk = C.ovf[2 * o + 1];
            const int slot = (int)(pk & 7u);
            const int ex = (int)(at / (uint32_t)G.NS), ey = (int)(at % (uint32_t)G.NS);
            const int code = jd_code(slot), dx = (code >> 2) - 1, dy = (code & 3) - 1;
            for (int base = (int)(pk >> 3);; base += 64) {
                const int i = base + (int)lane, cx = ex - i * dx, cy = ey - i * dy;
                // what ends the walk in FRONT of this cell: the map's edge, the update's box, an old ray that does not reach e
                bool before = !(cx >= 1 && cy >= 1 && cx <= G.W && cy <= G.H) || (cx >= R.x0 && cx <= R.x1 && cy >= R.y0 && cy <= R.y1);
                size_t ca = 0;
                if (!before) {
                    ca = (size_t)cx * G.NS + cy;
                    const int k = (int)(jd[ca * 8 + slot] & JD_K);
                    before = k != 0 && k < i;
                }
                // ... and BEHIND it: the next changed cell of a diagonal (its walker goes on from there)
                const bool after = !before && dx * dy != 0 && C.map[ca] != 0;
                const unsigned long long mb = __ballot(before), ma = __ballot(after);
                const int fb = mb != 0ull ? __ffsll((long long)mb) - 1 : 64, fa = ma != 0ull ? __ffsll((long long)ma) - 1 : 64;
                if ((int)lane < fb && (int)lane <= fa) jd[ca * 8 + slot] = (uint16_t)jd_entry(G, cx, cy, slot);
                if (fb < 64 || fa < 64) break;
            }
        }
    }
    // the first few blocks take the marks back; the last of them to get through returns the list to empty (a ticket per
    // block of the whole launch: a thousand blocks spent 60 us queueing at that counter)
    constexpr uint32_t NCLR = 8;
    if (blockIdx.x >= NCLR) return;
    const uint32_t nclr = min((uint32_t)gridDim.x, NCLR);
    const uint32_t n = min(C.cnt[0], C.cap);
    for (uint32_t j = blockIdx.x * blockDim.x + threadIdx.x; j < n; j += nclr * blockDim.x) C.map[C.list[j]] = 0;
    __threadfence();
    __syncthreads();
    if (threadIdx.x == 0) {
        const unsigned int done = atomicAdd(&C.cnt[2], 1u) + 1u;
        if (done == nclr) {
            C.cnt[0] = 0u;
            C.cnt[2] = 0u;
        }
    }
}

// ---------------------------------------------------------------- connected components
// 4-connected components of the free cells (lock-free union-find, CAS hooking of roots).  Every move the
// reference makes joins two free cells of one such component: straight steps trivially, diagonal
// steps because blocked()/dblock() (jps1.py:20,35) reject a diagonal whose two orthogonal
// neighbours are both occupied, so one of them is a free stepping stone.  A goal in another
// component than a free start therefore always ends in the exhaustive (0, t) of jps1.py:230,
// and the search kernel returns that without expanding the whole component.
__device__ __forceinline__ int ccl_find(int* __restrict__ lab, int i) {
    int p = lab[i];
    while (p != i) {
        const int gp = lab[p];
        if (gp != p) lab[i] = gp;  // path halving (benign race: labels only ever decrease along a chain)
        i = p;
        p = gp;
    }
    return i;
}
__device__ __forceinline__ void ccl_union(int* __restrict__ lab, int a, int b) {
    for (;;) {
        a = ccl_find(lab, a);
        b = ccl_find(lab, b);
        if (a == b) return;
        if (a < b) {
            const int t = a;
            a = b;
            b = t;
        }
        // hook the larger root under the smaller; the CAS only succeeds while `a` is still a root,
        // so a link is never overwritten (path halving above only ever writes non-roots)
        if (atomicCAS(&lab[a], a, b) == a) return;
    }
}
// Round 6: on open maps every cell used to be united with both its neighbours -- 131 000 unions on the empty part of the
// 256 x 256 canvas of config 1, all fighting over one root: 45 of the 112 us of a map build.  Now (a) a cell starts out
// pointing at the first cell of its run of free cells along y inside its 64-cell word (one ballot: no union at all inside a
// word), (b) the first cell of a word is united with the cell before it, (c) a cell is united with its neighbour in the
// row before ONLY where that is not already implied: its y-neighbour and that one's neighbour in the row before are not both
// free (if they are, the pair to the left says the same thing, and by induction the leftmost pair of the overlap says it).
// One thread per cell, a wavefront = 64 consecutive cells (blockDim is a multiple of 64).
// (cell i sits in lane i % 64 of its wavefront: here, and in the fused build's loop)
__device__ __forceinline__ void ccl_init_item(const uint8_t* __restrict__ occ, long long n, int H, int* __restrict__ lab, long long i) {
    const int lane = (int)(i & 63);
    const bool fr = i < n && occ[i] == 0;
    const bool first = fr && (lane == 0 || (int)(i % H) == 0 || occ[i - 1] != 0);  // a run (re)starts here
    const uint64_t bm = __ballot(first);
    if (fr) {  // (a free lane always has a start at or below it: lane 0, or the lane behind the last occupied one)
        const uint64_t m = bm & (~0ull >> (63 - lane));
        lab[i] = (int)(i - (long long)(lane - (63 - (int)__builtin_clzll(m))));
    } else if (i < n) {
        lab[i] = -1;
    }
}
__global__ void k_ccl_init(const uint8_t* __restrict__ occ, long long n, int H, int* __restrict__ lab) {
    ccl_init_item(occ, n, H, lab, (long long)blockIdx.x * blockDim.x + threadIdx.x);
}
__device__ __forceinline__ void ccl_merge_item(const uint8_t* __restrict__ occ, int W, int H, int* __restrict__ lab, long long i) {
    if (i >= (long long)W * H || occ[i]) return;
    const int y = (int)(i % H);
    const bool left = y > 0 && !occ[i - 1];
    if ((i & 63) == 0 && left) ccl_union(lab, (int)i, (int)i - 1);  // (b)
    if (i >= H && !occ[i - H] && !(left && !occ[i - H - 1])) ccl_union(lab, (int)i, (int)i - H);  // (c)
}
__global__ void k_ccl_merge(const uint8_t* __restrict__ occ, int W, int H, int* __restrict__ lab) {
    ccl_merge_item(occ, W, H, lab, (long long)blockIdx.x * blockDim.x + threadIdx.x);
}
__device__ __forceinline__ void ccl_flatten_item(long long n, int* __restrict__ lab, long long i) {
    if (i < n && lab[i] >= 0) {
        int r = (int)i;
        while (lab[r] != r) r = lab[r];
        lab[i] = r;
    }
}
__global__ void k_ccl_flatten(long long n, int* __restrict__ lab) { ccl_flatten_item(n, lab, (long long)blockIdx.x * blockDim.x + threadIdx.x); }

// ---- the map build of a small grid in FOUR launches instead of eight (round 6).  A build of a 256 x 256 grid is eight
// kernels of 4 - 18 us; queued one by one each waits 5 - 9 us for the runtime to launch it, and the search of the same tick
// waits behind all of them.  What needs nothing of each other shares a launch -- its blocks are the blocks of the separate
// kernels, one kind after the other:
//     1  rows (neighbour bytes, +-y words)  |  columns (+-x words; the neighbour byte computed, not read)  |  label init
//     2  cell infos                         |  label merge
//     3  diagonal words                     |  label flatten
//     4  jump distances                                                          (k_derive_jd itself)
// Every array is the one the separate kernels write, byte for byte (tests/test_map_updates_gpu.py compares the two builds).
// (Measured and dropped on the way, profiles/r06_map_build.txt: the whole build as ONE launch with barriers across a
// co-resident grid -- an agent-scope release / acquire between blocks on different XCDs writes back and invalidates their
// L2s: 170 - 240 us per build whatever the barrier's form; and the eight launches as a HIP graph -- the runtime ran the
// graph's two branches one after the other, with the same gaps.)
// One function per launch: block b of the launch's grid, for one grid.  k_build_1 .. 3 below call them for the handle's
// grid, k_slots_stage (further down) for every job of a fleet call.  (No __restrict__ on their own parameters: the kernels'
// and the item functions' qualifiers are the ones the compiler had before the bodies were shared, and with a third layer
// of them k_build_2 came out with two more SGPRs than profiles/prepare_slots_resource_usage.json records.)
__device__ __forceinline__ void build_1_block(const uint8_t* occ, const GridDev& G, uint8_t* nb8, BmWord* bm,
                                              int* lab, unsigned nb_rows, unsigned nb_cols, unsigned b) {
    const int lane = (int)(threadIdx.x & 63);
    const MapRange rr{0, G.PW - 1, 0, G.WORDS - 1}, rc{0, G.PH - 1, 0, G.WORDS - 1};
    if (b < nb_rows) {
        derive_rows_item(occ, G, nb8, bm, rr, (long long)b * 4 + (threadIdx.x >> 6), lane);
        return;
    }
    b -= nb_rows;
    if (b < nb_cols) {
        derive_cols_item<true>(occ, G, bm, rc, (long long)b * 4 + (threadIdx.x >> 6), lane);
        return;
    }
    b -= nb_cols;
    ccl_init_item(occ, (long long)G.W * G.H, G.H, lab, (long long)b * 256 + threadIdx.x);
}
__device__ __forceinline__ void build_2_block(const uint8_t* occ, const GridDev& G, uint16_t* ci, int* lab,
                                              unsigned nb_ci, unsigned b) {
    if (b < nb_ci) {
        const ChangeOut none{nullptr, nullptr, nullptr, 0u, MapRange{1, 0, 1, 0}};
        derive_cellinfo_item(G, ci, MapRange{0, G.PW - 1, 0, G.PH - 1}, MapRange{1, 0, 1, 0}, none, (long long)b * 256 + threadIdx.x, (int)(threadIdx.x & 63));
        return;
    }
    b -= nb_ci;
    ccl_merge_item(occ, G.W, G.H, lab, (long long)b * 256 + threadIdx.x);
}
__device__ __forceinline__ void build_3_block(const uint8_t* occ, const GridDev& G, BmWord* dbm, int* lab,
                                              unsigned nb_diag, unsigned b) {
    if (b < nb_diag) {
        const DiagRange whole{1, 0, 0, 0, 0};
        derive_diag_item(occ, G, dbm, whole, (long long)b * 16 + (threadIdx.x >> 6), (int)(threadIdx.x & 63));
        return;
    }
    b -= nb_diag;
    ccl_flatten_item((long long)G.W * G.H, lab, (long long)b * 1024 + threadIdx.x);
}
__global__ __launch_bounds__(256) void k_build_1(const uint8_t* __restrict__ occ, GridDev G, uint8_t* __restrict__ nb8, BmWord* __restrict__ bm,
                                                int* __restrict__ lab, unsigned nb_rows, unsigned nb_cols) {
    build_1_block(occ, G, nb8, bm, lab, nb_rows, nb_cols, blockIdx.x);
}
__global__ __launch_bounds__(256) void k_build_2(const uint8_t* __restrict__ occ, GridDev G, uint16_t* __restrict__ ci, int* __restrict__ lab, unsigned nb_ci) {
    build_2_block(occ, G, ci, lab, nb_ci, blockIdx.x);
}
__global__ __launch_bounds__(1024) void k_build_3(const uint8_t* __restrict__ occ, GridDev G, BmWord* __restrict__ dbm, int* __restrict__ lab, unsigned nb_diag) {
    build_3_block(occ, G, dbm, lab, nb_diag, blockIdx.x);
}

// Callers' grid preparation (SURVEY.md 8f, N1): zero-pad by map_d on the low side, dilate every occupied cell
// by the variant's offset set -- global_planner_st.py:246-262 ({-ifa, 0, ifa}^2) / global_planner_ccst.py:431-448
// (every offset in [-ifa, ifa]^2).  Gather form of the reference's scatter; the padding guarantees that no
// scattered index leaves the array, so the two are the same function.  One thread per output cell.
// msg_layout != 0: `raw` is the int8 data[] of a nav_msgs/OccupancyGrid (row-major [y][x], 100 = occupied,
// -1 = unknown), i.e. the transpose/threshold of map_callback (global_planner_st.py:16-20) is fused in:
// after 100 -> 1 and -1 -> 0 a cell counts as occupied for the dilation iff its value is > 0.
// WORLD (fxjps_prepare_slots_world, DESIGN.md section 3.14): the W0 x H0 source is a CANVAS that nobody assembles, the
// detected map `raw` pasted over a prior map that lives on the device (global_planner_st.py:210-225 /
// global_planner_ccst.py:395-409).  A canvas cell is read from the detected map inside its rectangle (it overwrites: a
// free detected cell clears an occupied prior cell), else from the prior inside the prior's rectangle, else it is 0.
struct WorldSrcDev {
    const uint8_t* prior;  // [pW][pH] non-zero = occupied, resident on this context; nullptr: the job has no prior
    int32_t pW, pH, px, py;  // the prior's extents and where its cell (0, 0) lies in the canvas
    int32_t rW, rH, rx, ry;  // the detected map's (SlotJobDev::raw, SlotJobDev::layout)
};
// The geometry of one preparation: the source's extents (a raw map's, a canvas's), the padding, the dilation, the variant
// (0 st, 1 ccst), the source's layout and the prepared extents.  The host fills it in one place (PrepReq::geom); the slot
// gather builds it from its job, whose layout the recorded register figures of the k_slots_* family hang on.
struct PrepGeom {
    int32_t W0, H0, dx, dy, ifa, variant, layout, W1, H1;
};
template <bool WORLD>  // (S is read only when WORLD)
__device__ __forceinline__ uint8_t prepared_byte(const uint8_t* __restrict__ raw, const WorldSrcDev* __restrict__ S, const PrepGeom& g, long long i) {
    const int ifa = g.ifa;
    const int x = (int)(i / g.H1), y = (int)(i % g.H1);
    const int step = g.variant == 0 ? (ifa > 0 ? ifa : 1) : 1;
    // (block-uniform: loaded once, into scalar registers.  With the fields read inside the loop the gather had two VGPRs less
    // and the world calls took 1 - 5 % longer: profiles/slot_kernel_family_bench.json)
    const WorldSrcDev W = WORLD ? *S : WorldSrcDev{};
    uint8_t v = 0;
    for (int a = -ifa; a <= ifa; a += step)
        for (int b = -ifa; b <= ifa; b += step) {
            const int sx = x - g.dx - a, sy = y - g.dy - b;
            if (sx >= 0 && sy >= 0 && sx < g.W0 && sy < g.H0) {
                bool o = false;  // canvas cell (sx, sy)
                if constexpr (WORLD) {
                    const int ux = sx - W.rx, uy = sy - W.ry, qx = sx - W.px, qy = sy - W.py;
                    if (ux >= 0 && uy >= 0 && ux < W.rW && uy < W.rH)
                        o = g.layout ? (reinterpret_cast<const int8_t*>(raw)[(size_t)uy * W.rW + ux] > 0) : (raw[(size_t)ux * W.rH + uy] != 0);
                    else if (qx >= 0 && qy >= 0 && qx < W.pW && qy < W.pH)  // (pW == 0 without a prior)
                        o = W.prior[(size_t)qx * W.pH + qy] != 0;
                } else {
                    o = g.layout ? (reinterpret_cast<const int8_t*>(raw)[(size_t)sy * g.W0 + sx] > 0) : (raw[(size_t)sx * g.H0 + sy] != 0);
                }
                if (o) v = 1;
            }
        }
    return v;
}
__global__ __launch_bounds__(256) void k_prepare_grid(const uint8_t* __restrict__ raw, const PrepGeom g, uint8_t* __restrict__ out) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long long)g.W1 * g.H1) return;
    out[i] = prepared_byte<false>(raw, nullptr, g, i);
}

// ---- The prepared grid diffed against the resident one (fxjps_refresh_grid, DESIGN.md section 3.16): which cells of
// `occ` are not the byte k_prepare_grid would write there, as a list in ascending order of the cell index i = x * H1 + y.
// Three launches: every block of 256 threads counts the changed cells among its 256 cells (and folds their box into the
// header); one block turns the counts into exclusive offsets, in place (k_scan_len's form: linear in the number of
// blocks); every block with a count writes its cells at its offset, in cell order (ballot ranks inside a wavefront, the
// wavefronts' counts through LDS).  They write nothing but `diff`:
//   diff[0 .. 8)               header: [0] number of changed cells, [1] max(8191 - x) + ... the box, DIFF_* below; zero: none
//   diff[8 .. 8 + cap)         the list, one word per cell: x << 16 | y << 1 | v  (v, the prepared byte, is 0 or 1)
//   diff[8 + cap .. + nblk]    the blocks' counts, after k_grid_diff_scan their offsets, then the total
// More changed cells than `cap`: the list is not written (the caller rebuilds the grid).
constexpr int DIFF_HDR = 8, DIFF_N = 0, DIFF_X0 = 1, DIFF_X1 = 2, DIFF_Y0 = 3, DIFF_Y1 = 4;  // X0 / Y0 hold 8191 - min, X1 / Y1 hold max + 1
__global__ __launch_bounds__(256) void k_grid_diff_count(const uint8_t* __restrict__ raw, const PrepGeom g, const uint8_t* __restrict__ occ,
                                                        uint32_t* __restrict__ hdr, uint32_t* __restrict__ scan) {
    __shared__ int s_box[4];
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    bool chg = false;
    if (i < (long long)g.W1 * g.H1) chg = occ[i] != prepared_byte<false>(raw, nullptr, g, i);
    if (threadIdx.x < 4) s_box[threadIdx.x] = 0;
    const int cnt = __syncthreads_count(chg);
    if (threadIdx.x == 0) scan[blockIdx.x] = (uint32_t)cnt;
    if (cnt == 0) return;  // (block-uniform)
    if (chg) {
        const int x = (int)(i / g.H1), y = (int)(i % g.H1);
        atomicMax(&s_box[0], 8191 - x);
        atomicMax(&s_box[1], x + 1);
        atomicMax(&s_box[2], 8191 - y);
        atomicMax(&s_box[3], y + 1);
    }
    __syncthreads();
    if (threadIdx.x < 4) atomicMax(&hdr[DIFF_X0 + threadIdx.x], (uint32_t)s_box[threadIdx.x]);
}
__global__ __launch_bounds__(1024) void k_grid_diff_scan(uint32_t* __restrict__ scan, uint32_t nblk, uint32_t* __restrict__ hdr) {
    __shared__ uint32_t s_part[1024];
    const uint32_t tid = threadIdx.x;
    const uint32_t per = (nblk + 1023u) / 1024u;
    const uint32_t lo = min(tid * per, nblk), hi = min(lo + per, nblk);
    uint32_t sum = 0;
    for (uint32_t i = lo; i < hi; i++) sum += scan[i];
    s_part[tid] = sum;
    __syncthreads();
    for (uint32_t o = 1; o < 1024u; o <<= 1) {
        const uint32_t v = tid >= o ? s_part[tid - o] : 0u;
        __syncthreads();
        s_part[tid] += v;
        __syncthreads();
    }
    uint32_t run = tid ? s_part[tid - 1] : 0u;
    for (uint32_t i = lo; i < hi; i++) {
        const uint32_t c = scan[i];
        scan[i] = run;
        run += c;
    }
    if (tid == 1023u) {
        scan[nblk] = s_part[1023];
        hdr[DIFF_N] = s_part[1023];
    }
}
__global__ __launch_bounds__(256) void k_grid_diff_write(const uint8_t* __restrict__ raw, const PrepGeom g, const uint8_t* __restrict__ occ,
                                                        const uint32_t* __restrict__ scan, uint32_t nblk, uint32_t cap, uint32_t* __restrict__ list) {
    __shared__ uint32_t s_wave[4];
    const uint32_t off = scan[blockIdx.x];
    if (scan[nblk] > cap || scan[blockIdx.x + 1] == off) return;  // (block-uniform)
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    uint8_t v = 0;
    bool chg = false;
    if (i < (long long)g.W1 * g.H1) {
        v = prepared_byte<false>(raw, nullptr, g, i);
        chg = occ[i] != v;
    }
    const uint64_t m = __ballot(chg);
    const uint32_t wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) s_wave[wave] = (uint32_t)__popcll(m);
    __syncthreads();
    uint32_t pos = off + rank_below(m);
    for (uint32_t w = 0; w < wave; w++) pos += s_wave[w];
    if (chg && pos < cap) list[pos] = (uint32_t)(i / g.H1) << 16 | (uint32_t)(i % g.H1) << 1 | (uint32_t)v;
}

// ---- Many raw maps into grid slots in one call (fxjps_prepare_slots, DESIGN.md section 3.8): the preparation above, the
// goal relocation and the four-launch build, each ONE launch over all jobs of the call.  A launch's blocks are the blocks
// the single-grid kernel would run for job 0, then those for job 1, ...: SlotTable::first[launch][j] is the first block
// of job j (first[launch][n] the grid size), and a block finds its job by a block-uniform binary search of that row (jobs
// differ in size: a 2-D grid padded to the largest job would waste most of its blocks).  Everything per item is the
// single-grid code: prepared_byte, build_1 .. 3_block and derive_jd_item are called as they stand.
//
// Three kernel templates make the launches of the four calls of this family; what differs between the calls is a template
// parameter, never a run-time flag (the compare form has a barrier and its LDS, which the plain form must not acquire):
//   REFRESH (fxjps_refresh_slots, DESIGN.md section 3.12): a tick whose maps mostly did not change.  A vehicle hands in the
//     raw map of the tick before far more often than a new one, and then the prepared grid is byte for byte what its slot
//     holds.  `changed` has one word per job, set by the host for every call: 1 for a job that must build (an empty slot,
//     other extents, a grid beyond the fused build), 0 for a job whose slot holds a grid of the prepared extents
//     (SlotJobDev::compare).  The gather of such a job reads the slot's byte at the index it would write, stores only where
//     the two differ and raises the job's word when any byte of the block did; a thread touches its own cell alone.  The
//     stage launches then return at once in every block of a job whose word is still 0 -- the six derived arrays of that
//     slot are already those of these bytes.  The goal launch runs for every job (the goal may have moved on an unchanged
//     map) and hands the words to the host beside its results: res[n * SLOT_RES + j].
//   WORLD (fxjps_prepare_slots_world / fxjps_refresh_slots_world, DESIGN.md section 3.14): SlotJobDev stays as it is, W0 / H0
//     being the canvas extents; a WorldSrcDev per job, staged behind the raws, says where the two sources lie in the canvas.
//     Only the gather knows: every later launch is the plain one.
// The forms that do not read `S` or `changed` are handed nullptr.
constexpr int SLOT_JOBS_MAX = 256;  // FXJPS_MAX_GRID_SLOTS
enum { SL_PREPARE = 0, SL_BUILD_1, SL_BUILD_2, SL_BUILD_3, SL_JD, SL_LAUNCHES };
struct SlotJobDev {
    GridDev G;           // the slot's extents and maps (what its descriptor in d_slot_desc will say)
    uint8_t* occ;        // [W][H] the prepared grid
    const uint8_t* raw;  // this job's raw map inside the staged input
    int32_t W0, H0, dx, dy, ifa, variant, layout;
    int32_t gx, gy;      // the shifted goal (inside the prepared grid: the host checked)
    uint32_t nb_rows, nb_cols, nb_ci, nb_diag;  // build_1 .. 3_block: where the kinds of blocks change within the job's part
    int32_t compare;     // fxjps_refresh_slots: the slot holds a grid of these extents, store only the bytes that differ
};
struct SlotTable {
    uint32_t first[SL_LAUNCHES][SLOT_JOBS_MAX + 1];
    SlotJobDev job[SLOT_JOBS_MAX];
};
// per job, k_slots_goal -> host: the (moved) goal, end_occu, status (0, or -1: row and column fully occupied)
constexpr int SLOT_RES = 4;

__device__ __forceinline__ int slot_job_of(const uint32_t* __restrict__ first, int n, unsigned b) {
    int lo = 0, hi = n;  // first[lo] <= b < first[hi]
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (first[mid] <= b) lo = mid; else hi = mid;
    }
    return lo;
}

// TILES, a further parameter of the bodies below (fxjps_set_slot_reuse(1), DESIGN.md section 3.18; the kernels of that form
// are k_slot_tiles_gather<WORLD> and k_slot_tiles_copy, the REFRESH forms' bodies under kernel names of their own): a
// compared job also says WHERE its bytes differ, in read-set tiles.  Every cell whose byte differs marks the tiles of its box
// [max(x-1,0) .. min(x+1,W-1)] x [max(y-1,0) .. min(y+1,H-1)] shifted by G.tsh -- FrameTiles::mark_box for one cell -- in the
// job's record of 128 words: tiles[j * 128 + ty] has a bit per x tile, tiles[j * 128 + 64 + tx] a bit per y tile.  A block in
// which no byte differs does nothing more than the REFRESH form; a block in which one does gathers its marks in 1 KB of LDS
// and flushes the non-zero words with one atomic each (a 256-cell block lies in one or two columns of the grid: a handful of
// words), so a tick that changed every byte does not queue up on 128 words per job.
struct SlotTileMarks {
    unsigned long long w[128];
};
// (every thread of the block calls both, `any` being block-uniform and true)
__device__ __forceinline__ void slot_tiles_clear(SlotTileMarks& M) {
    if (threadIdx.x < 128) M.w[threadIdx.x] = 0ull;
    __syncthreads();
}
__device__ __forceinline__ void slot_tiles_mark(SlotTileMarks& M, const GridDev& G, long long cell) {
    const int x = (int)(cell / G.H), y = (int)(cell - (long long)x * G.H);  // occ is [W][H]
    const int tx0 = max(x - 1, 0) >> G.tsh, tx1 = min(x + 1, G.W - 1) >> G.tsh;
    const int ty0 = max(y - 1, 0) >> G.tsh, ty1 = min(y + 1, G.H - 1) >> G.tsh;  // (at most 63: the host chose tsh so)
    const unsigned long long mx = (~0ull >> (63 - tx1)) & (~0ull << tx0), my = (~0ull >> (63 - ty1)) & (~0ull << ty0);
    for (int ty = ty0; ty <= ty1; ty++) atomicOr(&M.w[ty], mx);  // (at most three words each)
    for (int tx = tx0; tx <= tx1; tx++) atomicOr(&M.w[64 + tx], my);
}
__device__ __forceinline__ void slot_tiles_flush(SlotTileMarks& M, unsigned long long* __restrict__ rec) {
    __syncthreads();
    if (threadIdx.x < 128) {
        const unsigned long long v = M.w[threadIdx.x];
        if (v != 0ull) atomicOr(rec + threadIdx.x, v);
    }
}

// k_prepare_grid's gather, for every output cell of every job.
template <bool WORLD, bool REFRESH, bool TILES>
__device__ __forceinline__ void slots_gather_body(const SlotTable* __restrict__ T, const WorldSrcDev* __restrict__ S, int n,
                                                  uint32_t* __restrict__ changed, unsigned long long* __restrict__ tiles) {
    static_assert(REFRESH || !TILES, "only a refresh compares");
    const int j = slot_job_of(T->first[SL_PREPARE], n, blockIdx.x);
    const SlotJobDev& J = T->job[j];
    const PrepGeom g{J.W0, J.H0, J.dx, J.dy, J.ifa, J.variant, J.layout, J.G.W, J.G.H};
    const uint8_t* __restrict__ raw = J.raw;
    uint8_t* __restrict__ occ = J.occ;
    const long long i = (long long)(blockIdx.x - T->first[SL_PREPARE][j]) * blockDim.x + threadIdx.x;
    const bool inside = i < (long long)g.W1 * g.H1;
    const WorldSrcDev* __restrict__ Sj = WORLD ? S + j : nullptr;
    if constexpr (!REFRESH) {
        if (!inside) return;
        occ[i] = prepared_byte<WORLD>(raw, Sj, g, i);
    } else {
        const uint8_t v = inside ? prepared_byte<WORLD>(raw, Sj, g, i) : (uint8_t)0;
        if (!J.compare) {  // (block-uniform) a job that builds whatever the bytes are: its word is 1 already
            if (inside) occ[i] = v;
            return;
        }
        const bool differs = inside && occ[i] != v;  // bytes, not truthiness: a slot set to 7 where this is 1 is rewritten
        if (differs) occ[i] = v;
        // (every thread of the block reaches the barrier: none has returned above)
        const bool any = __syncthreads_or(differs) != 0;
        if (any && threadIdx.x == 0) changed[j] = 1u;
        if constexpr (TILES) {
            if (!any) return;  // (block-uniform)
            __shared__ SlotTileMarks s_marks;
            slot_tiles_clear(s_marks);
            if (differs) slot_tiles_mark(s_marks, J.G, i);
            slot_tiles_flush(s_marks, tiles + (size_t)j * 128);
        }
    }
}
template <bool WORLD, bool REFRESH>
__global__ __launch_bounds__(256) void k_slots_gather(const SlotTable* __restrict__ T, const WorldSrcDev* __restrict__ S, int n,
                                                     uint32_t* __restrict__ changed) {
    slots_gather_body<WORLD, REFRESH, false>(T, S, n, changed, nullptr);
}
template <bool WORLD>
__global__ __launch_bounds__(256) void k_slot_tiles_gather(const SlotTable* __restrict__ T, const WorldSrcDev* __restrict__ S, int n,
                                                          uint32_t* __restrict__ changed, unsigned long long* __restrict__ tiles) {
    slots_gather_body<WORLD, true, true>(T, S, n, changed, tiles);
}

// The free cell of line[0], line[stride], .. (n cells) nearest to index c, the lower index of two equally near ones
// (np.argmin over the ascending indices of np.where: global_planner_st.py:269-272), or -1.  One wavefront: lane l of
// step k looks at distance 64 k + l on either side, a ballot finds the least distance with a free cell.
__device__ __forceinline__ int slot_nearest_free(const uint8_t* __restrict__ line, long long stride, int n, int c, int lane) {
    const int dmax = max(c, n - 1 - c);
    for (int d0 = 0; d0 <= dmax; d0 += 64) {
        const int d = d0 + lane, lo = c - d, hi = c + d;
        const bool flo = lo >= 0 && line[(long long)lo * stride] == 0;
        const bool fhi = hi < n && line[(long long)hi * stride] == 0;
        const uint64_t blo = __ballot(flo), bhi = __ballot(fhi);
        if (blo | bhi) {
            const int t = __builtin_ctzll(blo | bhi);
            return ((blo >> t) & 1ull) ? c - (d0 + t) : c + (d0 + t);
        }
    }
    return -1;
}
// The goal rule, one wavefront, the library's one copy of it: the goal moved off an obstacle (st:268-272 / ccst:454-458),
// end_occu (st:273 / ccst:461-464 with numpy's slice rules: a negative bound counts from the end, everything is clipped to
// the array).  (gx, gy) is the shifted goal, inside the W1 x H1 grid `occ`: the host checked.  Lane 0 writes the record
// res[0 .. SLOT_RES): the (moved) goal, end_occu, status (0, or -1: row and column fully occupied).
__device__ __forceinline__ void goal_rule(const uint8_t* __restrict__ occ, int W1, int H1, int gx, int gy, int ifa, int variant, int lane,
                                          int32_t* __restrict__ res) {
    int end_occu = 0, status = 0;
    if (occ[(size_t)gx * H1 + gy]) {
        if (variant == 0) end_occu = 1;
        int best = slot_nearest_free(occ + (size_t)gx * H1, 1, H1, gy, lane);
        if (best >= 0) {
            gy = best;
        } else {
            best = slot_nearest_free(occ + gy, H1, W1, gx, lane);
            if (best >= 0) gx = best; else status = -1;  // FXJPS_E_ARG: the reference raises here
        }
    }
    if (variant == 1 && ifa > 0 && status == 0) {
        auto bound = [](int v, int n) { return v < 0 ? max(v + n, 0) : min(v, n); };
        const int x0 = bound(gx - ifa, W1), x1 = bound(gx + ifa, W1), y0 = bound(gy - ifa, H1), y1 = bound(gy + ifa, H1);
        bool any = false;
        if (x1 > x0 && y1 > y0) {
            const int ny = y1 - y0, nc = (x1 - x0) * ny;  // (at most 128 x 128)
            for (int i = lane; i < nc; i += 64) any = any || occ[(size_t)(x0 + i / ny) * H1 + (y0 + i % ny)] != 0;
        }
        end_occu = __ballot(any) != 0ull ? 1 : 0;
    }
    if (lane == 0) {
        res[0] = gx;
        res[1] = gy;
        res[2] = end_occu;
        res[3] = status;
    }
}
// ... for the resident grid of a single-grid call (prepare_finish): one block of one wavefront
__global__ __launch_bounds__(64) void k_prepare_goal(const uint8_t* __restrict__ occ, int W1, int H1, int gx, int gy, int ifa, int variant,
                                                    int32_t* __restrict__ res) {
    goal_rule(occ, W1, H1, gx, gy, ifa, variant, (int)threadIdx.x, res);
}
// ... and for every job of a slot call, one wavefront per job
__device__ __forceinline__ void slots_goal_job(const SlotTable* __restrict__ T, int32_t* __restrict__ res, int j, int lane) {
    const SlotJobDev& J = T->job[j];
    goal_rule(J.occ, J.G.W, J.G.H, J.gx, J.gy, J.ifa, J.variant, lane, res + j * SLOT_RES);
}
template <bool REFRESH>
__global__ __launch_bounds__(64) void k_slots_goal(const SlotTable* __restrict__ T, int32_t* __restrict__ res, int n, const uint32_t* __restrict__ changed) {
    const int j = (int)blockIdx.x;
    slots_goal_job(T, res, j, (int)threadIdx.x);
    if constexpr (REFRESH)
        if (threadIdx.x == 0) res[n * SLOT_RES + j] = (int32_t)changed[j];
}

// k_build_1 .. 3 and k_derive_jd (L = SL_BUILD_1 .. SL_JD) over all jobs whose grid takes the fused build (at most 2^18
// cells; the others have no blocks here and are built by derive_maps behind these launches).
template <int L, bool REFRESH>
__global__ __launch_bounds__(L == SL_BUILD_3 ? 1024 : 256) void k_slots_stage(const SlotTable* __restrict__ T, int n, const uint32_t* __restrict__ changed) {
    static_assert(L >= SL_BUILD_1 && L <= SL_JD, "a build stage");
    const int j = slot_job_of(T->first[L], n, blockIdx.x);
    if constexpr (REFRESH)
        if (changed[j] == 0u) return;  // (block-uniform: one scalar load)
    const SlotJobDev& J = T->job[j];
    const GridDev G = J.G;
    const uint8_t* __restrict__ occ = J.occ;
    const unsigned b = blockIdx.x - T->first[L][j];
    if constexpr (L == SL_BUILD_1)
        build_1_block(occ, G, const_cast<uint8_t*>(G.nb8), const_cast<BmWord*>(G.bm), const_cast<int*>(G.comp), J.nb_rows, J.nb_cols, b);
    else if constexpr (L == SL_BUILD_2)
        build_2_block(occ, G, const_cast<uint16_t*>(G.ci), const_cast<int*>(G.comp), J.nb_ci, b);
    else if constexpr (L == SL_BUILD_3)
        build_3_block(occ, G, const_cast<BmWord*>(G.bm) + (size_t)4 * G.LINES * G.WORDS, const_cast<int*>(G.comp), J.nb_diag, b);
    else
        derive_jd_item(G, const_cast<uint16_t*>(G.jd), DiagRange{1, 0, 0, 0, 0}, (long long)b * 256 + threadIdx.x);
}

// ---- Many PREPARED grids into grid slots in one call (fxjps_set_grid_slots / fxjps_refresh_grid_slots, DESIGN.md section
// 3.17): the job's bytes are the slot's bytes, so in place of the gather there is a copy, and there is no goal launch.  The
// table is the family's: SlotJobDev::raw is the job's grid inside the staged input, G.W x G.H its extents, and the row
// SlotTable::first[SL_PREPARE] deals SLOT_COPY_BLOCK cells to a block (not the gather's 256).  Both sides are plain streams
// of bytes -- the staged grids begin at multiples of 16 bytes of one allocation, occ is the start of an allocation of its
// own -- so a lane moves 16 bytes with one load and one store; the last lane of a job whose cell count is no multiple of 16
// moves its 1 .. 15 bytes one by one and touches nothing behind the grid.
//   REFRESH: as in the gather.  A job marked `compare` reads the slot's 16 bytes beside the staged ones and stores only a
// piece in which a byte differs (bytes, not truthiness); every thread of the block reaches the barrier, one raises the
// job's word.  A job not marked is stored whole and its word stays at the host's 1.
constexpr int SLOT_COPY_LANE = 16, SLOT_COPY_BLOCK = 256 * SLOT_COPY_LANE;
//   TILES: as in the gather, exact per byte: a piece that is stored marks only the bytes of it that differ.
template <bool REFRESH, bool TILES>
__device__ __forceinline__ void slots_copy_body(const SlotTable* __restrict__ T, int n, uint32_t* __restrict__ changed,
                                                unsigned long long* __restrict__ tiles) {
    static_assert(REFRESH || !TILES, "only a refresh compares");
    const int j = slot_job_of(T->first[SL_PREPARE], n, blockIdx.x);
    const SlotJobDev& J = T->job[j];
    const uint8_t* __restrict__ src = J.raw;
    uint8_t* __restrict__ occ = J.occ;
    const long long ncell = (long long)J.G.W * J.G.H;
    const long long i = ((long long)(blockIdx.x - T->first[SL_PREPARE][j]) * blockDim.x + threadIdx.x) * SLOT_COPY_LANE;
    const bool whole = i + SLOT_COPY_LANE <= ncell;                    // a full piece
    const int tail = !whole && i < ncell ? (int)(ncell - i) : 0;       // ... or the grid's last 1 .. 15 bytes
    const bool compare = REFRESH && J.compare != 0;                    // (block-uniform)
    bool differs = false;
    uint32_t dbytes = 0u;  // TILES: bit k set, byte i + k of a compared job differs
    if (whole) {
        const uint4 v = *reinterpret_cast<const uint4*>(src + i);
        differs = true;
        if (compare) {
            const uint4 o = *reinterpret_cast<const uint4*>(occ + i);
            differs = ((v.x ^ o.x) | (v.y ^ o.y) | (v.z ^ o.z) | (v.w ^ o.w)) != 0u;
            if constexpr (TILES) {
                const uint32_t xw[4] = {v.x ^ o.x, v.y ^ o.y, v.z ^ o.z, v.w ^ o.w};
#pragma unroll
                for (int k = 0; k < 16; k++) dbytes |= ((xw[k >> 2] >> (8 * (k & 3))) & 0xFFu) != 0u ? 1u << k : 0u;
            }
        }
        if (differs) *reinterpret_cast<uint4*>(occ + i) = v;
    } else {
        for (int k = 0; k < tail; k++) {
            const uint8_t v = src[i + k];
            const bool d = !compare || occ[i + k] != v;
            if (d) occ[i + k] = v;
            differs = differs || d;
            if constexpr (TILES) dbytes |= compare && d ? 1u << k : 0u;
        }
    }
    if constexpr (REFRESH) {
        if (!compare) return;  // (the whole block: its job builds whatever the bytes are)
        const bool any = __syncthreads_or(differs) != 0;
        if (any && threadIdx.x == 0) changed[j] = 1u;
        if constexpr (TILES) {
            if (!any) return;  // (block-uniform)
            __shared__ SlotTileMarks s_marks;
            slot_tiles_clear(s_marks);
            for (uint32_t m = dbytes; m != 0u; m &= m - 1u) slot_tiles_mark(s_marks, J.G, i + __builtin_ctz(m));
            slot_tiles_flush(s_marks, tiles + (size_t)j * 128);
        }
    }
}
template <bool REFRESH>
__global__ __launch_bounds__(256) void k_slots_copy(const SlotTable* __restrict__ T, int n, uint32_t* __restrict__ changed) {
    slots_copy_body<REFRESH, false>(T, n, changed, nullptr);
}
__global__ __launch_bounds__(256) void k_slot_tiles_copy(const SlotTable* __restrict__ T, int n, uint32_t* __restrict__ changed,
                                                        unsigned long long* __restrict__ tiles) {
    slots_copy_body<true, true>(T, n, changed, tiles);
}

// ---- The ccst node's crop in front of the world-frame calls (fxjps_prepare_slots_cropped, DESIGN.md section 3.15):
// remove_zero_rowscols (global_planner_ccst.py:36-63) cuts every map message down to the box spanned by its non-zero
// cells and the vehicle's cell.  Two launches over all jobs of the call, queued back to back: k_crop_bounds reduces every
// message to its box of non-zero cells (a record of min x, min y, max x, max y per job, staged as INT32_MAX, INT32_MAX,
// -1, -1), k_crop_window copies the window that box and the vehicle's cell span densely into the window buffer, which
// the gather of the world-frame call then reads as its detected map.  A launch's blocks are dealt to the jobs by a prefix
// table, as SlotTable::first deals them: a block covers CROP_BLOCK_BYTES cells of its job's message.
//   Which cells count is the reference's X.nonzero() on the matrix map_callback made (ccst:21-23): a byte != 0 in layout
// 0; in layout 1 an int8 that is neither 0 nor -1 (100 became 1, -1 became 0; a 50 or a -5 counts for the box, though
// only values > 0 are occupied for the preparation).
constexpr int CROP_BLOCK_BYTES = 4096;  // 256 threads, one 16-byte load each
struct CropJobDev {
    const uint8_t* raw;  // the message inside the staged input; its room is a multiple of 16 bytes
    uint8_t* win;        // the job's room in the window buffer (as large as the message's)
    int32_t W0, H0, layout, ifa;
    int32_t s0x, s0y;    // the vehicle's cell in the message (ccst:47)
};
struct CropTable {
    uint32_t first[SLOT_JOBS_MAX + 1];
    CropJobDev job[SLOT_JOBS_MAX];
};

// A thread loads 16 cells at once and walks their (outer, inner) coordinates from ONE division; cells at and beyond
// W0 * H0 -- the tail of the room holds whatever an earlier call staged there -- are masked by their index.  The four
// extremes are reduced across the wavefront's 64 lanes, then across the block's four wavefronts in LDS, and a block that
// saw a non-zero cell issues four atomics on its job's record; a block that saw none issues none.
__global__ __launch_bounds__(256) void k_crop_bounds(const CropTable* __restrict__ T, int32_t* __restrict__ box, int n) {
    const int j = slot_job_of(T->first, n, blockIdx.x);
    const CropJobDev& J = T->job[j];
    const int layout = J.layout, ncell = J.W0 * J.H0;  // (at most 8190 x 8190)
    const int inner = layout ? J.W0 : J.H0;             // extent of the index that runs fastest: y in layout 0, x in layout 1
    const int i0 = ((int)(blockIdx.x - T->first[j]) * 256 + (int)threadIdx.x) * 16;
    int mn_o = INT32_MAX, mn_i = INT32_MAX, mx_o = -1, mx_i = -1;
    if (i0 < ncell) {
        const uint4 v = *reinterpret_cast<const uint4*>(J.raw + i0);
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
        int o = i0 / inner, i = i0 - o * inner;
#pragma unroll
        for (int k = 0; k < 16; k++) {
            const uint32_t b = (w[k >> 2] >> (8 * (k & 3))) & 0xffu;
            if (i0 + k < ncell && b != 0u && !(layout && b == 0xffu)) {
                mn_o = min(mn_o, o);
                mx_o = max(mx_o, o);
                mn_i = min(mn_i, i);
                mx_i = max(mx_i, i);
            }
            if (++i == inner) {
                i = 0;
                o++;
            }
        }
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        mn_o = min(mn_o, __shfl_xor(mn_o, m, 64));
        mn_i = min(mn_i, __shfl_xor(mn_i, m, 64));
        mx_o = max(mx_o, __shfl_xor(mx_o, m, 64));
        mx_i = max(mx_i, __shfl_xor(mx_i, m, 64));
    }
    __shared__ int red[4][4];
    const int wave = (int)threadIdx.x >> 6;
    if ((threadIdx.x & 63u) == 0u) {
        red[wave][0] = mn_o;
        red[wave][1] = mn_i;
        red[wave][2] = mx_o;
        red[wave][3] = mx_i;
    }
    __syncthreads();  // (every thread of the block reaches it: none has returned above)
    if (threadIdx.x == 0) {
        for (int k = 1; k < 4; k++) {
            mn_o = min(mn_o, red[k][0]);
            mn_i = min(mn_i, red[k][1]);
            mx_o = max(mx_o, red[k][2]);
            mx_i = max(mx_i, red[k][3]);
        }
        if (mx_o >= 0) {
            int32_t* B = box + 4 * j;
            atomicMin(B + 0, layout ? mn_i : mn_o);
            atomicMin(B + 1, layout ? mn_o : mn_i);
            atomicMax(B + 2, layout ? mx_i : mx_o);
            atomicMax(B + 3, layout ? mx_o : mx_i);
        }
    }
}

// The window of every job that goes on: lo = min(box min, vehicle's cell) per axis, win = box max - lo (the last
// non-zero row and column are EXCLUDED, as the reference's slice excludes them), copied as [win_x][win_y] (layout 0) /
// [win_y][win_x] (layout 1).  The grid is sized for the whole message; blocks past the window leave, and so do the blocks
// of a job that will not be planned or is refused -- the host's rule (crop_call), from the same integers.
__global__ __launch_bounds__(256) void k_crop_window(const CropTable* __restrict__ T, const int32_t* __restrict__ box, int n) {
    const int j = slot_job_of(T->first, n, blockIdx.x);
    const CropJobDev& J = T->job[j];
    const int W0 = J.W0, H0 = J.H0, layout = J.layout;
    const int32_t* B = box + 4 * j;
    const int mx_x = B[2], mx_y = B[3];
    if (mx_x < 0 || W0 <= 2 * J.ifa) return;  // no non-zero cell / ccst:351
    const int lo_x = min(B[0], J.s0x), lo_y = min(B[1], J.s0y);
    if (lo_x < 0 || lo_y < 0) return;          // the vehicle lies left of or below the message: refused
    const int win_x = mx_x - lo_x, win_y = mx_y - lo_y;  // (0 <= lo <= box min <= box max < 8190)
    if (win_x == 0 || win_y == 0) return;
    const int ncell = win_x * win_y, base = (int)(blockIdx.x - T->first[j]) * CROP_BLOCK_BYTES;
    if (base >= ncell) return;
    const uint8_t* __restrict__ raw = J.raw;
    uint8_t* __restrict__ win = J.win;
    const int fast = layout ? win_x : win_y;
    for (int i = base + (int)threadIdx.x; i < min(base + CROP_BLOCK_BYTES, ncell); i += 256) {
        const int a = i / fast, b = i - a * fast;  // layout 0: (x, y) of the window; layout 1: (y, x)
        win[i] = layout ? raw[(size_t)(lo_y + a) * W0 + (lo_x + b)] : raw[(size_t)(lo_x + a) * H0 + (lo_y + b)];
    }
}

// Wire / on-disk adapters (SURVEY.md 8f, N3): one tiled byte transpose with a value map.
//   dst[(fb ? B-1-b : b)][(fa ? A-1-a : a)][0..ch) = map(src[a][b])      src [A][B], dst [B][A][ch]
// TM_OCC_TO_MSG   grid -> nav_msgs/OccupancyGrid data[] (global_planner_st.py:103,115: 1 -> 100, data.T)
// TM_GRAY_TO_OCC  8-bit grey image -> grid (global_planner_st.py:179-182: > 200 free, else occupied; img[::-1].T)
// TM_OCC_TO_GRAY  grid -> 8-bit image (global_planner_st.py:368-370: 0 -> 255, else 0; mapsave.T[::-1])
constexpr int TM_OCC_TO_MSG = 0, TM_GRAY_TO_OCC = 1, TM_OCC_TO_GRAY = 2;
__global__ __launch_bounds__(256) void k_transpose_map(const uint8_t* __restrict__ src, int A, int B, int fa, int fb, int mode, int ch,
                                                      uint8_t* __restrict__ dst) {
    __shared__ uint8_t tile[32][33];
    const int b0 = blockIdx.x * 32, a0 = blockIdx.y * 32;
    for (int r = threadIdx.y; r < 32; r += 8) {  // rows of src: a; contiguous: b
        const int a = a0 + r, b = b0 + (int)threadIdx.x;
        uint8_t v = 0;
        if (a < A && b < B) {
            const uint8_t u = src[(size_t)a * B + b];
            v = mode == TM_OCC_TO_MSG ? (u ? 100 : 0) : mode == TM_GRAY_TO_OCC ? (u > 200 ? 0 : 1) : (u == 0 ? 255 : 0);
        }
        tile[r][threadIdx.x] = v;
    }
    __syncthreads();
    for (int r = threadIdx.y; r < 32; r += 8) {  // rows of dst: b; contiguous: a
        const int b = b0 + r, a = a0 + (int)threadIdx.x;
        if (a < A && b < B) {
            const size_t o = ((size_t)(fb ? B - 1 - b : b) * A + (size_t)(fa ? A - 1 - a : a)) * (size_t)ch;
            const uint8_t v = tile[threadIdx.x][r];
            for (int c = 0; c < ch; c++) dst[o + c] = v;
        }
    }
}

// ---- Many slots' maps on their way out in one call (fxjps_publish_slots, DESIGN.md section 3.10): the two grid -> wire
// adapters above (TM_OCC_TO_MSG, and TM_OCC_TO_GRAY with the rows flipped) for every job of the call in ONE launch.  Its
// blocks are the 32 x 32 tiles of job 0, then those of job 1, ...: PubTable::first[j] is the first block of job j
// (first[n] the grid size), found by the block-uniform search of section 3.8 (slot_job_of).  A block reads its tile of
// occ[x][y] once and writes from it whichever outputs its job asked for; both land in one output buffer, each at the
// 16-byte aligned offset the host chose.  Everything per job is block-uniform: it is loaded once, into scalar registers.
struct PubJobDev {
    const uint8_t* occ;  // [W][H] the slot's grid
    int32_t W, H;
    int32_t nty;         // tiles along y: (H + 31) / 32
    int32_t ch;          // channels of the image
    long long msg_off;   // of data[] [H][W] in the output buffer; < 0: not asked for
    long long img_off;   // of the image [H][W][ch]; < 0: not asked for
};
struct PubTable {
    uint32_t first[SLOT_JOBS_MAX + 1];
    uint32_t pad_[3];    // (the jobs start at a 16-byte boundary)
    PubJobDev job[SLOT_JOBS_MAX];
};
__global__ __launch_bounds__(256) void k_publish_slots(const PubTable* __restrict__ T, int n, uint8_t* __restrict__ out) {
    __shared__ uint8_t tile[32][33];
    const int j = slot_job_of(T->first, n, blockIdx.x);
    const PubJobDev& J = T->job[j];
    const uint8_t* __restrict__ occ = J.occ;
    const int W = J.W, H = J.H, nty = J.nty, ch = J.ch;
    const long long msg_off = J.msg_off, img_off = J.img_off;
    const int t = (int)(blockIdx.x - T->first[j]);
    const int x0 = (t / nty) * 32, y0 = (t % nty) * 32;
    const int tx = (int)(threadIdx.x & 31u), ty = (int)(threadIdx.x >> 5);
    for (int r = ty; r < 32; r += 8) {  // rows of occ: x; contiguous: y
        const int x = x0 + r, y = y0 + tx;
        tile[r][tx] = (x < W && y < H) ? occ[(size_t)x * H + y] : (uint8_t)0;
    }
    __syncthreads();
    for (int r = ty; r < 32; r += 8) {  // rows of both outputs: y; contiguous: x
        const int y = y0 + r, x = x0 + tx;
        if (x < W && y < H) {
            const uint8_t u = tile[tx][r];
            if (msg_off >= 0) out[(size_t)msg_off + (size_t)y * W + x] = u ? 100 : 0;  // data.T, 1 -> 100   st:103,114
            if (img_off >= 0) {                                                        // 0 -> 255, else 0; mapsave.T[::-1]   st:368-371
                const size_t o = (size_t)img_off + ((size_t)(H - 1 - y) * W + x) * (size_t)ch;
                const uint8_t v = u == 0 ? 255 : 0;
                out[o] = v;
                if (ch == 3) {  // (the host let nothing but 1 and 3 through)
                    out[o + 1] = v;
                    out[o + 2] = v;
                }
            }
        }
    }
}

// A cell that a list names more than once takes the value of its LAST entry (what `grid[xs, ys] = vals` does on the
// host): every entry leaves its index, by atomic maximum, in owner[cell] (all -1 at rest), and only the entry that
// finds its own index there applies its value -- and puts the -1 back.
__global__ void k_update_claim(int* __restrict__ owner, int W, int H, const int32_t* __restrict__ xy, long long n) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int x = xy[2 * i], y = xy[2 * i + 1];
    if (x >= 0 && y >= 0 && x < W && y < H) atomicMax(&owner[(size_t)x * H + y], (int)i);
}
// chg[i] (may be nullptr): 0 the cell keeps its value (or a later entry decides), 1 it became free, 2 it became occupied.
__global__ void k_update_cells(uint8_t* occ, int W, int H, const int32_t* xy, const uint8_t* val, long long n, uint8_t* chg, int* owner) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int x = xy[2 * i], y = xy[2 * i + 1];
    uint8_t c = 0;
    if (x >= 0 && y >= 0 && x < W && y < H) {
        const size_t cell = (size_t)x * H + y;
        if (owner[cell] == (int)i) {
            owner[cell] = -1;
            const uint8_t v = val[i] ? 1 : 0, old = occ[cell];
            if (old != v) {
                occ[cell] = v;
                c = v ? 2 : 1;
            }
        }
    }
    if (chg) chg[i] = c;
}

// The component labels after a small update, without relabelling the map (SURVEY K3).  `lab` is the union-find forest
// k_ccl_init / _merge / _flatten left (a free cell points at its root; roots at themselves; -1: never free since).
// A cell that became free gets a set of its own unless it still has one, and is united with its free 4-neighbours:
// whatever is connected on the updated grid has one root -- the direction the search's early-out needs (a goal under
// another root than the start is unreachable).  A cell that became occupied keeps its node (other cells' paths to
// their root may run through it), so a component that the update splits keeps one root: such queries are searched
// instead of answered at once, same result.  The host falls back to the full relabelling for large updates and every
// 64 small ones, so the labels never drift far from the exact components.
__global__ void k_ccl_update(const uint8_t* __restrict__ occ, int W, int H, const int32_t* __restrict__ xy, const uint8_t* __restrict__ chg,
                             long long n, int* __restrict__ lab, int phase) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n || chg[i] != 1) return;
    const int x = xy[2 * i], y = xy[2 * i + 1];
    const int c = x * H + y;
    if (phase == 0) {  // sets first: a union may run into a neighbour that became free in the same update
        if (lab[c] < 0) lab[c] = c;
        return;
    }
    if (y > 0 && !occ[c - 1]) ccl_union(lab, c, c - 1);
    if (y + 1 < H && !occ[c + 1]) ccl_union(lab, c, c + 1);
    if (x > 0 && !occ[c - H]) ccl_union(lab, c, c - H);
    if (x + 1 < W && !occ[c + H]) ccl_union(lab, c, c + H);
}

// ---------------------------------------------------------------- waypoint selection, ccst node (SURVEY 8f, N2)
// scripts/global_planner_ccst.py:487-544 with map_line_col (:258-283) for every path of a batch: one wavefront per
// path.  The points closer than 1.5 to the vehicle go (:507-513, a ballot compaction), then the line-of-sight pruning
// (:515-521) -- sequential by definition (`ii` advances or a point is deleted), but a single forward pass: with the kept
// prefix ending in a, candidate b and its successor c, "the line a-c is free" deletes b (c becomes the candidate), else b
// is kept and becomes a.  The lanes rasterise the segment together: lane k looks at x = p1.x + 1 + k, cell
// (x, rint(slope * x) + int(p1.y)) of the sub-map between the two end points, exactly the reference's np.arange /
// np.rint / astype(int) in float64 (IEEE division, multiplication and round-half-even on the device; -ffp-contract=off).
// map_line_col's first question -- is there any obstacle in the sub-map at all -- needs no scan of its own: the answer
// only matters when a rasterised cell is occupied.  The next 64 points of the path sit in the lanes (one each), so that
// stepping to the next point is a lane read, not a memory round trip.
// What the rules below need to know about the grid and the frame of ONE query (wave-uniform): the two batch kernels fill
// it from their arguments (one grid, one frame for the batch), k_waypoint_slots from its query's record.
struct WpView {
    const uint8_t* occ;  // ccst: the grid [W][H] the line tests read, obstacle iff non-zero
    int32_t W, H;
    double reso, ox, oy;
    int32_t msx, msy;    // st: map_start
};
// ... and what a rule returns (the same in every lane).
struct WpSel {
    double wx, wy, wz, ogx, ogy, ogz, ang;
    int dim;  // st: valid components of the waypoint
    int m;    // ccst: points that remain
};

struct WaypointArgs {
    const uint8_t* occ;      // resident grid [W][H], obstacle iff non-zero
    int32_t W, H;
    const int32_t* cells;    // CSR paths: (x, y) pairs
    const long long* offsets;
    const int32_t* len;      // > 0: jump points of the path; else no path
    long long nq;
    double reso, ox, oy;
    const double* pos;       // [nq][3] vehicle position
    const double* goal;      // [nq][3] global goal
    const int32_t* end_occu; // [nq] or nullptr
    double* out_wp;          // [nq][3]
    double* out_goal;        // [nq][3]
    int32_t* out_nkept;      // [nq]
    int32_t* kept;           // CSR with the offsets of the paths: the remaining cells of path q at offsets[q] .. + out_nkept[q]
};

__device__ __forceinline__ bool wp_line_is_free(const WpView& V, int ax, int ay, int bx, int by, int lane) {
    const int x0 = min(ax, bx), x1 = max(ax, bx), y0 = min(ay, by), y1 = max(ay, by);
    // relative to p0 = (x0, y0); p1 is the end with the smaller x (ties keep a)        ccst:261-268
    double p1x = (double)(ax - x0), p1y = (double)(ay - y0), p2x = (double)(bx - x0), p2y = (double)(by - y0);
    if (p2x < p1x) {
        const double tx = p1x, ty = p1y;
        p1x = p2x;
        p1y = p2y;
        p2x = tx;
        p2y = ty;
    }
    const int steps = (int)(p2x - p1x) - 1;  // np.arange(p1[0] + 1, p2[0], 1): the integers strictly between
    if (steps <= 0) return true;
    const double slope = (p2y - p1y) / (p2x - p1x);  // :270
    const int ip1y = (int)p1y;
    bool hit = false;
    for (int k0 = 0; k0 < steps; k0 += WAVE) {
        const int k = k0 + lane;
        if (k < steps) {
            const double x = p1x + 1.0 + (double)k;
            const int cx = (int)x, cy = (int)__builtin_rint(slope * x) + ip1y;
            // `lb in obstacles of the sub-map` (:279): the sub-map is mapu[x0:x1, y0:y1], clipped to the array
            if (cx >= 0 && cx < x1 - x0 && cy >= 0 && cy < y1 - y0) {
                const int gx = x0 + cx, gy = y0 + cy;
                if (gx < V.W && gy < V.H && V.occ[(size_t)gx * V.H + gy] != 0) hit = true;
            }
        }
        RECONV();
        if (__ballot(hit) != 0ull) return false;  // collide
    }
    return true;
}

// The ccst rule for one path (n jump points at src, n <= 0: no path) by one wavefront; the remaining cells go to dst.
__device__ __forceinline__ WpSel wp_rule_ccst(const WpView& V, const int2* __restrict__ src, int2* __restrict__ dst, int n, double px, double py,
                                              double pz, double gx, double gy, double gz, int eo, int lane) {
    double wx = gx, wy = gy, wz = gz;  // no path: wp = global_goal   ccst:481-485
    int m = 0;
    if (n > 0) {
        // ---- :507-513: drop the points (but the first) closer than 1.5 to the vehicle; path3 = (path + (1, 0)) * reso + origin, z = 0
        m = n;
        if (n > 2) {
            int w = 0;
            for (int b0 = 0; b0 < n; b0 += WAVE) {
                const int i = b0 + lane;
                int2 c = make_int2(0, 0);
                bool keep = false;
                if (i < n) {
                    c = src[i];
                    const double dx = ((double)(c.x + 1) * V.reso + V.ox) - px, dy = ((double)c.y * V.reso + V.oy) - py, dz = 0.0 - pz;
                    keep = i == 0 || !(sqrt(dx * dx + dy * dy + dz * dz) < 1.5);
                }
                RECONV();
                const uint64_t km = __ballot(keep);
                if (keep) dst[w + (int)rank_below(km)] = c;  // (moves down only; src and dst are different arrays anyway)
                RECONV();
                w += __popcll(km);
            }
            m = w;
        } else {
            if (lane < n) dst[lane] = src[lane];
            RECONV();
        }
        __threadfence_block();
        // ---- :515-521: drop a point when the straight line between its neighbours is free.  Forward pass over dst[0 .. m):
        // kept prefix dst[0 .. w), a = its last point, b = the candidate, c = the point behind it.
        int2 k1 = make_int2(0, 0), k2 = make_int2(0, 0);  // the second and third point that remain
        if (m > 2) {
            int w = 1;               // dst[0] stays
            int base = 0;            // the lanes hold dst[base .. base + 64)
            int2 buf = make_int2(0, 0);
            if (lane < m) buf = dst[lane];
            RECONV();
            const auto point = [&](int i) -> int2 {  // dst[i] as it was before this pass (i ascends)
                while (i >= base + WAVE) {
                    base += WAVE;
                    buf = make_int2(0, 0);
                    if (base + lane < m) buf = dst[base + lane];
                    RECONV();
                }
                const int l = rfli(i - base);
                return make_int2(__builtin_amdgcn_readlane(buf.x, l), __builtin_amdgcn_readlane(buf.y, l));
            };
            int2 a = point(0), b = point(1);
            for (int i = 2; i < m; i++) {
                const int2 c = point(i);
                if (!wp_line_is_free(V, a.x, a.y, c.x, c.y, lane)) {  // b stays: it becomes the end of the kept prefix
                    if (lane == 0) dst[w] = b;  // (w <= i - 1: never a point this pass has not read yet -- they sit in the lanes)
                    RECONV();
                    k1 = w == 1 ? b : k1;
                    k2 = w == 2 ? b : k2;
                    w++;
                    a = b;
                }
                b = c;
            }
            if (lane == 0) dst[w] = b;  // the last point always stays
            RECONV();
            k1 = w == 1 ? b : k1;
            k2 = w == 2 ? b : k2;
            w++;
            m = w;
        }
        // ---- :523-526
        if (m > 2) {
            const int2 c1 = k1, c2 = k2;
            const double x1 = (double)(c1.x + 1) * V.reso + V.ox, y1 = (double)c1.y * V.reso + V.oy;
            const double x2 = (double)(c2.x + 1) * V.reso + V.ox, y2 = (double)c2.y * V.reso + V.oy;
            wx = (x1 * 1.4 + x2 * 0.6) / 2;
            wy = (y1 * 1.4 + y2 * 0.6) / 2;
            wz = (0.0 * 1.4 + 0.0 * 0.6) / 2;
        }
    }
    double ogx = gx, ogy = gy, ogz = gz;
    if (n > 0 && eo == 1) {  // :541-544: the goal region is occupied: hold position, the vehicle position becomes the goal
        wx = ogx = px;
        wy = ogy = py;
        wz = ogz = pz;
    }
    return WpSel{wx, wy, wz, ogx, ogy, ogz, 0.0, 3, m};
}

__global__ __launch_bounds__(256) void k_waypoint_ccst(WaypointArgs A) {
    const int lane = threadIdx.x & 63;
    const long long q = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (q >= A.nq) return;
    const int n = rfli(A.len[q]);
    const double px = A.pos[3 * q], py = A.pos[3 * q + 1], pz = A.pos[3 * q + 2];
    const double gx = A.goal[3 * q], gy = A.goal[3 * q + 1], gz = A.goal[3 * q + 2];
    const int eo = A.end_occu ? rfli(A.end_occu[q]) : 0;
    const long long off = n > 0 ? A.offsets[q] : 0;
    const WpView V{A.occ, A.W, A.H, A.reso, A.ox, A.oy, 0, 0};
    const WpSel S = wp_rule_ccst(V, reinterpret_cast<const int2*>(A.cells) + off, reinterpret_cast<int2*>(A.kept) + off, n, px, py, pz, gx, gy, gz,
                                 eo, lane);
    if (lane == 0) {
        A.out_wp[3 * q] = S.wx;
        A.out_wp[3 * q + 1] = S.wy;
        A.out_wp[3 * q + 2] = S.wz;
        A.out_goal[3 * q] = S.ogx;
        A.out_goal[3 * q + 1] = S.ogy;
        A.out_goal[3 * q + 2] = S.ogz;
        A.out_nkept[q] = S.m;
    }
}

// ---------------------------------------------------------------- the st node's waypoint rule over a batch
// global_planner_st.py:292-327 (fxjps_waypoint_st in fxjps_waypoints.cpp is the same rule for one path on the host), one
// wavefront per path.  The rule's decisions, and the angle it returns, hang on math.atan2 -- the host's libm -- of INTEGER
// pairs (cell - map_start): the device does not compute them, it looks them up in a table the host filled with its own
// atan2 once per grid shape (WpAtab: a in [0, amax] x b in [-bmax, bmax], 8 bytes each: 17 MB for a
// 1024 x 1024 grid), atan2(-a, b) = -atan2(a, b) being exact in libm (tests/test_host_cpu.py checks that it is).
// The loop over the path -- "stop at the first point whose angle to the goal's bearing does not grow any more" -- is a
// comparison of neighbouring lanes and one ballot per 64 points.
struct WpAtab {
    const double* atab;  // atan2((double)a, (double)b) by the host's libm, [amax + 1][2 bmax + 1]
    int32_t amax, bmax;
};
struct WaypointStArgs {
    const int32_t* cells;     // CSR paths: (x, y) pairs
    const long long* offsets;
    const int32_t* len;       // > 0: jump points of the path; else no path
    long long nq;
    const int32_t* map_start; // [nq][2]
    double reso, ox, oy;
    const double* pos;        // [nq][3] vehicle position
    const double* goal;       // [nq][3] global goal
    const int32_t* end_occu;  // [nq] or nullptr
    double dis_wp_tre, ang_wp_tre;
    const double* prev_wp;    // [nq][3] or nullptr: the waypoint of the last tick (kept when the loop does not find one)
    const int32_t* prev_dim;  // [nq]: 2 / 3 components of it, anything else: none
    WpAtab T;
    double* out_wp;           // [nq][3]
    int32_t* out_dim;         // [nq]
    double* out_goal;         // [nq][3]
    double* out_ang;          // [nq]
};
__device__ __forceinline__ double wp_atan2(const WpAtab& T, int a, int b) {
    const int aa = min(abs(a), T.amax), bb = min(max(b, -T.bmax), T.bmax);  // (in range by construction: the host sized the table from the batch)
    const double v = T.atab[(size_t)aa * (size_t)(2 * T.bmax + 1) + (size_t)(bb + T.bmax)];
    return a < 0 ? -v : v;
}
// The st rule for one path (n jump points at c, n <= 0: no path) by one wavefront.  pd / prev: the components of the last
// tick's waypoint (2 or 3; anything else: none) and where they are.
__device__ __forceinline__ WpSel wp_rule_st(const WpView& V, const WpAtab& T, const int2* __restrict__ c, int n, double px, double py, double pz,
                                            double gx, double gy, double gz, int eo, int pd, const double* __restrict__ prev, double dis_wp_tre,
                                            double ang_wp_tre, int lane) {
    double wx = gx, wy = gy, wz = gz, ogx = gx, ogy = gy, ogz = gz, ang_wp = 0.0;
    int dim = 3;
    if (n > 0) {  // (no path: wp = global_goal, st:287-290)
        const int msx = V.msx, msy = V.msy;
        dim = 0;  // None
        if (pd == 2 || pd == 3) {
            dim = pd;
            wx = prev[0];
            wy = prev[1];
            wz = pd == 3 ? prev[2] : 0.0;
        }
        const int2 ce = c[n - 1];
        const double a_goal = wp_atan2(T, ce.x + 1 - msx, ce.y + 1 - msy);  // path2 = path + (1, 1), st:292
        double carry = 0.0;  // ang_wp as the loop enters the lanes' first point
        bool found = false;
        for (int k0 = 1; k0 < n && !found; k0 += WAVE) {  // :305-312
            const int k = k0 + lane;
            const bool on = k < n;
            const int2 p = c[on ? k : 0];
            const int dx = p.x + 1 - msx, dy = p.y + 1 - msy;
            const double d = fabs(a_goal - wp_atan2(T, dx, dy));
            double prv = __shfl_up(d, 1);
            prv = lane == 0 ? carry : prv;
            const bool far2 = (long long)dx * dx + (long long)dy * dy > 4ll;  // np.linalg.norm(map_wp - map_start) > 2, of integers
            const uint64_t hit = __ballot(on && d <= prv && far2);
            if (hit != 0ull) {
                const int l = (int)__builtin_ctzll(hit);
                const int kk = k0 + l;  // the first point that turns back: the waypoint is the one in front of it
                const int2 w = c[kk - 1];
                wx = (double)(w.x + 1) * V.reso + V.ox;
                wy = (double)(w.y + 1) * V.reso + V.oy;
                wz = 0.0;
                dim = 2;
                ang_wp = __longlong_as_double((long long)lane_get64((uint64_t)__double_as_longlong(prv), l));
                found = true;
            } else {
                const int last = min(n - k0, WAVE) - 1;  // the chunk's last point
                carry = __longlong_as_double((long long)lane_get64((uint64_t)__double_as_longlong(d), last));
            }
        }
        if (!found) ang_wp = carry;
        if (dim == 0) {  // :313-314
            wx = gx;
            wy = gy;
            wz = gz;
            dim = 3;
        }
        const double ex = wx - px, ey = wy - py;
        const double uav2next_wp = sqrt(ex * ex + ey * ey);  // :315
        if (eo == 1) {  // :317-320
            wx = ogx = px;
            wy = ogy = py;
            wz = ogz = pz;
            dim = 3;
        } else if (!(n > 2 && (uav2next_wp > dis_wp_tre || (ang_wp > ang_wp_tre && ang_wp < 3.14159265358979323846 * 0.5)))) {  // :321-322
            wx = gx;
            wy = gy;
            wz = gz;
            dim = 3;
        }
    }
    return WpSel{wx, wy, dim == 3 ? wz : 0.0, ogx, ogy, ogz, ang_wp, dim, 0};
}
__global__ __launch_bounds__(256) void k_waypoint_st(WaypointStArgs A) {
    const int lane = threadIdx.x & 63;
    const long long q = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (q >= A.nq) return;
    const int n = rfli(A.len[q]);
    const double px = A.pos[3 * q], py = A.pos[3 * q + 1], pz = A.pos[3 * q + 2];
    const double gx = A.goal[3 * q], gy = A.goal[3 * q + 1], gz = A.goal[3 * q + 2];
    WpView V{nullptr, 0, 0, A.reso, A.ox, A.oy, 0, 0};
    int pd = 0, eo = 0;
    const int2* c = nullptr;
    if (n > 0) {
        c = reinterpret_cast<const int2*>(A.cells) + A.offsets[q];
        V.msx = rfli(A.map_start[2 * q]);
        V.msy = rfli(A.map_start[2 * q + 1]);
        pd = A.prev_wp ? rfli(A.prev_dim[q]) : 0;
        eo = A.end_occu ? rfli(A.end_occu[q]) : 0;
    }
    const WpSel S = wp_rule_st(V, A.T, c, n, px, py, pz, gx, gy, gz, eo, pd, A.prev_wp ? A.prev_wp + 3 * q : nullptr, A.dis_wp_tre, A.ang_wp_tre, lane);
    if (lane == 0) {
        A.out_wp[3 * q] = S.wx;
        A.out_wp[3 * q + 1] = S.wy;
        A.out_wp[3 * q + 2] = S.wz;
        A.out_dim[q] = S.dim;
        A.out_goal[3 * q] = S.ogx;
        A.out_goal[3 * q + 1] = S.ogy;
        A.out_goal[3 * q + 2] = S.ogz;
        A.out_ang[q] = S.ang;
    }
}

// ---------------------------------------------------------------- both rules over a grid-slots batch (DESIGN.md section 3.9)
// fxjps_waypoint_slots_batch: every query brings its own rule, grid (the occupancy of the slot it names, resolved by the
// host from its slot records when the call is staged), resolution, origin and map_start.  One launch, one wavefront per
// path, which branches on its query's rule into the very functions the two kernels above call.  The record of a query is
// wave-uniform: it is read through readfirstlane and stays in scalar registers.
struct WpSlotQuery {
    const uint8_t* occ;  // ccst: the slot's grid [W][H]; st: unused (nullptr)
    int32_t W, H;
    double reso, ox, oy;
    int32_t msx, msy;
    int32_t rule;        // 0 st, 1 ccst, anything else: not this kernel's (the st rule on host threads)
    int32_t eo, pdim, pad_;
    double pos[3], goal[3], prev[3];
};
struct WpSlotResult {
    double wp[3], goal[3], ang;
    int32_t dim, nkept;
};
struct WaypointSlotsArgs {
    const WpSlotQuery* in;    // [nq]
    WpSlotResult* out;        // [nq]
    const int32_t* cells;     // CSR paths: (x, y) pairs
    const long long* offsets;
    const int32_t* len;       // > 0: jump points of the path, else no path; nullptr: offsets[q + 1] - offsets[q]
    int32_t* kept;            // CSR with the offsets of the paths (ccst queries only)
    long long nq;
    double dis_wp_tre, ang_wp_tre;
    WpAtab T;
};
__global__ __launch_bounds__(256) void k_waypoint_slots(WaypointSlotsArgs A) {
    const int lane = threadIdx.x & 63;
    const long long q = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (q >= A.nq) return;
    const WpSlotQuery& Q = A.in[q];
    const int rule = rfli(Q.rule);
    if (rule != 0 && rule != 1) return;
    const long long off = (long long)rfl64((uint64_t)A.offsets[q]);
    const int n = A.len ? rfli(A.len[q]) : rfli((int)min(A.offsets[q + 1] - off, 0x7FFFFFFFll));
    const WpView V{reinterpret_cast<const uint8_t*>(rfl64((uint64_t)Q.occ)), rfli(Q.W), rfli(Q.H), rfld(Q.reso), rfld(Q.ox), rfld(Q.oy),
                   rfli(Q.msx), rfli(Q.msy)};
    const int eo = rfli(Q.eo);
    const double px = rfld(Q.pos[0]), py = rfld(Q.pos[1]), pz = rfld(Q.pos[2]);
    const double gx = rfld(Q.goal[0]), gy = rfld(Q.goal[1]), gz = rfld(Q.goal[2]);
    const int2* c = reinterpret_cast<const int2*>(A.cells) + (n > 0 ? off : 0);
    WpSel S;
    if (rule == 1) {
        S = wp_rule_ccst(V, c, reinterpret_cast<int2*>(A.kept) + (n > 0 ? off : 0), n, px, py, pz, gx, gy, gz, eo, lane);
    } else {
        S = wp_rule_st(V, A.T, c, n, px, py, pz, gx, gy, gz, eo, rfli(Q.pdim), Q.prev, A.dis_wp_tre, A.ang_wp_tre, lane);
    }
    if (lane == 0) {
        WpSlotResult& R = A.out[q];
        R.wp[0] = S.wx;
        R.wp[1] = S.wy;
        R.wp[2] = S.wz;
        R.goal[0] = S.ogx;
        R.goal[1] = S.ogy;
        R.goal[2] = S.ogz;
        R.ang = S.ang;
        R.dim = S.dim;
        R.nkept = S.m;
    }
}

// ---------------------------------------------------------------- a fleet tick's outgoing messages (DESIGN.md section 3.11)
// fxjps_tick_outputs_slots: k_waypoint_slots' selection, and from the registers it leaves what each node publishes after
// its waypoint block -- /jps_path (path3: every jump point in the world frame, st:292-298 / ccst:487-494),
// /direct_jps_path (ccst: path4, the world-frame points of the cells the rule just kept, ccst:495-521; without a path the
// two poses [pos, wp], ccst:485) and the Point of /goal_global (st:335, 356-359 / ccst:559-562, 590-593).  The record of a
// query is k_waypoint_slots' with the vehicle's home position behind it; the rules are the very functions above.
// The world-frame expression and the 2-norm are the ones the rules use for path3 and uav2next_wp, written once here for
// the stores (IEEE multiply, add, divide and sqrt; -ffp-contract=off).
struct TickQuery {
    WpSlotQuery s;
    double hx, hy;  // (xo, yo): the vehicle's position on its first tick
};
struct TickResult {
    WpSlotResult r;
    double point[3];
    int32_t dir_n, dir_back;
};
struct TickOutputsArgs {
    const TickQuery* in;      // [nq]
    TickResult* out;          // [nq]
    const int32_t* cells;     // CSR paths: (x, y) pairs
    const long long* offsets; // [nq + 1]
    const int32_t* len;       // > 0: jump points of the path, else no path; nullptr: offsets[q + 1] - offsets[q]
    int32_t* kept;            // CSR with the offsets of the paths (ccst queries only)
    double* path_xyz;         // [cells][3]: path3 of query q at triple offsets[q]
    double* dir_xyz;          // [cells + 2 nq][3]: the direct path of query q at triple offsets[q] + 2 q
    long long nq;
    double dis_wp_tre, ang_wp_tre;
    WpAtab T;
};
// (host and device: the st rule's host form in fxjps.hip calls the same three functions)
__host__ __device__ __forceinline__ double wp_world(int c, double reso, double o) { return (double)c * reso + o; }
__host__ __device__ __forceinline__ double wp_norm2(double x, double y) { return sqrt(x * x + y * y); }
// st:335 / ccst:562 with Python's min(r, 1): 1 iff 1 < r, so a NaN (0 / 0) stays and x / 0 gives 1
__host__ __device__ __forceinline__ double tick_point_z(double wx, double wy, double gx, double gy, double gz, double hx, double hy) {
    const double r = wp_norm2(wx - hx, wy - hy) / wp_norm2(gx - hx, gy - hy);
    const double r1 = 1.0 < r ? 1.0 : r;
    return 1.0 + r1 * (gz - 1.0);
}
__global__ __launch_bounds__(256) void k_tick_outputs_slots(TickOutputsArgs A) {
    const int lane = threadIdx.x & 63;
    const long long q = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (q >= A.nq) return;
    const WpSlotQuery& Q = A.in[q].s;
    const int rule = rfli(Q.rule);
    if (rule != 0 && rule != 1) return;
    const long long off = (long long)rfl64((uint64_t)A.offsets[q]);
    const long long room = (long long)rfl64((uint64_t)A.offsets[q + 1]) - off;  // the query's own range: no store goes past it
    const int n = A.len ? rfli(A.len[q]) : rfli((int)min(room, 0x7FFFFFFFll));
    const WpView V{reinterpret_cast<const uint8_t*>(rfl64((uint64_t)Q.occ)), rfli(Q.W), rfli(Q.H), rfld(Q.reso), rfld(Q.ox), rfld(Q.oy),
                   rfli(Q.msx), rfli(Q.msy)};
    const int eo = rfli(Q.eo);
    const double px = rfld(Q.pos[0]), py = rfld(Q.pos[1]), pz = rfld(Q.pos[2]);
    const double gx = rfld(Q.goal[0]), gy = rfld(Q.goal[1]), gz = rfld(Q.goal[2]);
    const int2* c = reinterpret_cast<const int2*>(A.cells) + (n > 0 ? off : 0);
    int2* kept = reinterpret_cast<int2*>(A.kept) + (n > 0 ? off : 0);
    WpSel S;
    if (rule == 1) {
        S = wp_rule_ccst(V, c, kept, n, px, py, pz, gx, gy, gz, eo, lane);
    } else {
        S = wp_rule_st(V, A.T, c, n, px, py, pz, gx, gy, gz, eo, rfli(Q.pdim), Q.prev, A.dis_wp_tre, A.ang_wp_tre, lane);
    }
    // ---- /jps_path: path2 = path + (1, 1) (st) or + (1, 0) (ccst), path3 = path2 * map_reso + map_o, z = 0
    const int np = (int)min((long long)max(n, 0), room);
    const int yplus = rule == 1 ? 0 : 1;
    double* p3 = A.path_xyz + 3 * off;
    for (int i = lane; i < np; i += WAVE) {
        const int2 p = c[i];
        p3[3 * i] = wp_world(p.x + 1, V.reso, V.ox);
        p3[3 * i + 1] = wp_world(p.y + yplus, V.reso, V.oy);
        p3[3 * i + 2] = 0.0;
    }
    RECONV();
    // ---- /direct_jps_path (ccst): the kept cells in the world frame, or the two poses
    int dir_n = 0, dir_back = 0;
    if (rule == 1) {
        double* d4 = A.dir_xyz + 3 * (off + 2 * q);  // (room + 2 triples are this query's)
        if (n > 0) {
            dir_n = S.m;
            __threadfence_block();  // lane 0 wrote the cells the pruning kept
            const int nd = min(S.m, np);
            for (int i = lane; i < nd; i += WAVE) {
                const int2 p = kept[i];
                d4[3 * i] = wp_world(p.x + 1, V.reso, V.ox);
                d4[3 * i + 1] = wp_world(p.y, V.reso, V.oy);
                d4[3 * i + 2] = 0.0;
            }
            RECONV();
        } else {
            dir_n = 2;
            dir_back = 100;
            if (lane == 0) {
                d4[0] = px;
                d4[1] = py;
                d4[2] = pz;
                d4[3] = S.wx;
                d4[4] = S.wy;
                d4[5] = S.wz;
            }
            RECONV();
        }
    }
    // ---- /goal_global
    const double hx = rfld(A.in[q].hx), hy = rfld(A.in[q].hy);
    double z = tick_point_z(S.wx, S.wy, S.ogx, S.ogy, S.ogz, hx, hy);
    if (rule == 1 && (wp_norm2(S.ogx - px, S.ogy - py) < 0.5 || eo != 0)) z = 0.0;
    if (lane == 0) {
        TickResult& R = A.out[q];
        R.r.wp[0] = S.wx;
        R.r.wp[1] = S.wy;
        R.r.wp[2] = S.wz;
        R.r.goal[0] = S.ogx;
        R.r.goal[1] = S.ogy;
        R.r.goal[2] = S.ogz;
        R.r.ang = S.ang;
        R.r.dim = S.dim;
        R.r.nkept = S.m;
        R.point[0] = S.wx;
        R.point[1] = S.wy;
        R.point[2] = z;
        R.dir_n = dir_n;
        R.dir_back = dir_back;
    }
}

// ---------------------------------------------------------------- kept paths against their slots (DESIGN.md section 3.19)
// fxjps_check_paths_slots: does the grid of its slot, as it is now, still allow path q?  One wavefront per path.  The
// segments are taken 64 at a time, one per lane: its direction, its length (0 from the first malformed segment of the chunk
// on) and, by a shuffle scan over the lanes, the number of unit steps up to its end.  The chunk's unit steps are then taken
// in path order, 64 at a time, one per lane: the lane finds its segment in the scanned lengths (a binary search through
// lane reads), reads the one to three occupancy bytes blocked() of scripts/jps1.py:14-31 reads for that step, and the
// lowest failing lane of the first group of steps that has one is the answer.  A malformed segment is reported when the
// steps before it have passed.  The slot's grid comes with the query's record, resolved by the host from the context's slot
// records when the call is staged, as for k_waypoint_slots.  The verdicts are FXJPS_PATH_* of include/fxjps.h.
struct CheckQuery {
    const uint8_t* occ;  // the slot's grid [W][H], obstacle iff non-zero
    int32_t W, H;
    int32_t sx, sy;      // every cell of the path is moved by this first
};
struct CheckResult {
    int32_t verdict, seg, cx, cy;
};
struct CheckPathsArgs {
    const CheckQuery* in;      // [nq]
    CheckResult* out;          // [nq]
    const int32_t* cells;      // CSR paths: (x, y) pairs
    const long long* offsets;  // [nq + 1]
    long long nq;
};
constexpr int CHECK_VALID = 1, CHECK_EMPTY = 0, CHECK_BLOCKED = 2, CHECK_OUTSIDE = 3, CHECK_MALFORMED = -1;

__global__ __launch_bounds__(256) void k_check_paths_slots(CheckPathsArgs A) {
    const int lane = threadIdx.x & 63;
    const long long q = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (q >= A.nq) return;
    const CheckQuery& Q = A.in[q];
    const uint8_t* occ = reinterpret_cast<const uint8_t*>(rfl64((uint64_t)Q.occ));
    const long long W = rfli(Q.W), H = rfli(Q.H), sx = rfli(Q.sx), sy = rfli(Q.sy);
    const long long off = (long long)rfl64((uint64_t)A.offsets[q]);
    const long long n = (long long)rfl64((uint64_t)A.offsets[q + 1]) - off;
    const int2* c = reinterpret_cast<const int2*>(A.cells) + off;
    const auto outside = [&](long long x, long long y) { return x < 0 || x >= W || y < 0 || y >= H; };
    // the first cell: lane 0 judges it like a step's target and the answer comes back through the same ballot and lane
    // reads as a step's
    int verdict = n > 0 ? CHECK_VALID : CHECK_EMPTY;
    long long seg = -1, fx = -1, fy = -1;
    {
        long long x0 = 0, y0 = 0;
        bool out0 = false;
        if (n > 0 && lane == 0) {
            const int2 p0 = c[0];
            x0 = (long long)p0.x + sx;
            y0 = (long long)p0.y + sy;
            out0 = outside(x0, y0);
        }
        RECONV();
        if (__ballot(out0) != 0ull) {
            verdict = CHECK_OUTSIDE;
            seg = 0;
            fx = (long long)rfl64((uint64_t)__shfl(x0, 0, WAVE));
            fy = (long long)rfl64((uint64_t)__shfl(y0, 0, WAVE));
        }
    }
    const long long nseg = n - 1;
    for (long long s0 = 0; verdict == CHECK_VALID && s0 < nseg; s0 += WAVE) {
        // ---- this lane's segment
        const long long s = s0 + lane;
        long long ax = 0, ay = 0, len = 0;
        int ux = 0, uy = 0;
        bool bad = false;
        if (s < nseg) {
            const int2 a = c[s], b = c[s + 1];
            const long long dx = (long long)b.x - a.x, dy = (long long)b.y - a.y;
            const long long mx = dx < 0 ? -dx : dx, my = dy < 0 ? -dy : dy;
            bad = (dx == 0 && dy == 0) || (dx != 0 && dy != 0 && mx != my);
            len = mx > my ? mx : my;
            ux = (dx > 0) - (dx < 0);
            uy = (dy > 0) - (dy < 0);
            ax = (long long)a.x + sx;
            ay = (long long)a.y + sy;
        }
        RECONV();
        const uint64_t bm = __ballot(bad);
        const int mlane = bm != 0ull ? (int)__builtin_ctzll(bm) : WAVE;  // the walk ends in front of the first malformed segment
        if (lane >= mlane) len = 0;
        long long incl = len;  // unit steps up to the end of this lane's segment
        for (int o = 1; o < WAVE; o <<= 1) {
            const long long t = __shfl_up(incl, o, WAVE);
            if (lane >= o) incl += t;
        }
        const long long T = (long long)rfl64((uint64_t)__shfl(incl, WAVE - 1, WAVE));
        // ---- the chunk's unit steps, 64 at a time
        for (long long t0 = 0; t0 < T; t0 += WAVE) {
            const long long t = t0 + lane;
            int j = 0;  // the step's segment: the first whose scanned length exceeds t
            for (int w = WAVE / 2; w > 0; w >>= 1) {
                const long long v = __shfl(incl, j + w - 1, WAVE);
                if (v <= t) j += w;
            }
            const long long k = t - (__shfl(incl, j, WAVE) - __shfl(len, j, WAVE));  // steps of that segment already taken
            const long long bx = __shfl(ax, j, WAVE), by = __shfl(ay, j, WAVE);
            const int vx = __shfl(ux, j, WAVE), vy = __shfl(uy, j, WAVE);
            const long long cx = bx + vx * k, cy = by + vy * k, tx = cx + vx, ty = cy + vy;
            int f = 0;
            if (t < T) {
                if (outside(cx, cy) || outside(tx, ty)) {  // (a step from outside: the step that left the grid is an earlier one)
                    f = CHECK_OUTSIDE;
                } else {
                    bool o = occ[(size_t)tx * (size_t)H + (size_t)ty] != 0;
                    if (!o && vx != 0 && vy != 0) o = occ[(size_t)tx * (size_t)H + (size_t)cy] != 0 && occ[(size_t)cx * (size_t)H + (size_t)ty] != 0;
                    if (o) f = CHECK_BLOCKED;
                }
            }
            RECONV();
            const uint64_t fm = __ballot(f != 0);
            if (fm != 0ull) {
                const int fl = (int)__builtin_ctzll(fm);
                verdict = rfli(__shfl(f, fl, WAVE));
                seg = s0 + rfli(__shfl(j, fl, WAVE));
                fx = (long long)rfl64((uint64_t)__shfl(tx, fl, WAVE));
                fy = (long long)rfl64((uint64_t)__shfl(ty, fl, WAVE));
                break;
            }
        }
        if (verdict == CHECK_VALID && bm != 0ull) {
            verdict = CHECK_MALFORMED;
            seg = s0 + mlane;
            fx = (long long)rfl64((uint64_t)__shfl(ax, mlane, WAVE));
            fy = (long long)rfl64((uint64_t)__shfl(ay, mlane, WAVE));
        }
    }
    if (lane == 0) {
        CheckResult& R = A.out[q];
        R.verdict = verdict;
        R.seg = (int32_t)seg;
        R.cx = (int32_t)fx;
        R.cy = (int32_t)fy;
    }
}

// ---------------------------------------------------------------- detected maps into the prior maps (DESIGN.md section 3.20)
// fxjps_absorb_prior: the rectangles of up to 256 jobs pasted into the prior maps they name, as n sequential slice
// assignments on the host would paste them (global_planner_st.py:219-220).  ONE launch over the prior cells of the union
// boxes, one box per named prior: the host clips every rectangle to its prior, drops the jobs that miss it and deals the
// launch's blocks to the boxes by a prefix table (AbsorbTable::first, as SlotTable::first deals them).  A thread owns one
// prior cell, adjacent lanes adjacent y -- the contiguous axis of the prior and of a layout-0 raw.  It walks the jobs of
// ITS prior from the last to the first, out of the block's copy of them in LDS (every lane reads the same record: a
// broadcast), and stops at the first job that decides the cell under the mode's rule; it then stores the byte if it
// differs.  No thread reads a byte that another writes (the raws are the staged input, the prior byte is the thread's
// own), no atomic touches a map byte, and the result does not depend on the order in which threads run.  A layout-1 raw
// is [y][x]: its reads are strided across the lanes, taken as they come like those of prepared_byte and k_crop_window
// (a raw is read once per covering cell and stays in L2 for the lanes that share its lines).  The flips -- cells whose
// non-zero test changed -- are counted by one ballot per wavefront and one atomic add per wavefront that saw any, into
// the box's counter at the head of the table, which the staged copy zeroed and the one copy back returns.
constexpr int ABSORB_JOBS_MAX = 256, ABSORB_PRIORS_MAX = 16;  // FXJPS_MAX_GRID_SLOTS jobs, FXJPS_MAX_PRIOR_MAPS boxes
constexpr int ABSORB_OVERWRITE = 0, ABSORB_OCCUPIED = 1, ABSORB_KNOWN = 2;  // FXJPS_ABSORB_*
struct AbsorbJobDev {
    const uint8_t* at;  // the byte of rectangle cell (0, 0) inside the staged input
    int32_t stride;     // layout 0: cell (i, j) is at[i * stride + j] (stride = H0); layout 1: at[j * stride + i] (W0)
    int32_t layout;
    int32_t x0, y0;     // the prior cell that rectangle cell (0, 0) lands on (may lie outside the prior)
    int32_t w, h;       // the rectangle's extents
};
struct AbsorbBoxDev {
    uint8_t* occ;           // the prior [pW][pH] on this context
    int32_t pH;
    int32_t x0, y0, w, h;   // the union of the prior's clipped rectangles: every cell of it lies inside the prior
    int32_t job0, njobs;    // its jobs, AbsorbTable::job[job0 .. job0 + njobs), in job order
    int32_t prior;          // ... and its counter
};
struct AbsorbTable {
    unsigned long long changed[ABSORB_PRIORS_MAX];  // staged as 0; what comes back
    uint32_t first[ABSORB_PRIORS_MAX + 1];          // first[b]: the first block of box b; first[nbox]: the grid size
    int32_t nbox, mode;
    AbsorbBoxDev box[ABSORB_PRIORS_MAX];
    AbsorbJobDev job[ABSORB_JOBS_MAX];
};
static_assert(sizeof(AbsorbJobDev) % 4 == 0, "the job records are copied to LDS word by word");

// The flips of a wavefront into its prior's counter, for k_prior_absorb and k_prior_grow: one ballot, and one atomic add if
// it saw any.  Every lane of the block calls it.  (The box lookup, the copy of the job records to LDS and the job walk stay
// written out in both kernels: as inlined helpers each of them changed the instructions the compiler emits.)
__device__ __forceinline__ void prior_count_flips(unsigned long long* counter, bool flip) {
    RECONV();
    const uint64_t m = __ballot(flip);
    if ((threadIdx.x & 63u) == 0u && m != 0ull) atomicAdd(counter, (unsigned long long)__popcll(m));
}

__global__ __launch_bounds__(256) void k_prior_absorb(AbsorbTable* __restrict__ T) {
    __shared__ AbsorbJobDev s_job[ABSORB_JOBS_MAX];
    const int nbox = T->nbox, mode = T->mode;
    int b = 0;  // (block-uniform)
    while (b + 1 < nbox && T->first[b + 1] <= blockIdx.x) b++;
    const AbsorbBoxDev B = T->box[b];
    {
        const uint32_t* __restrict__ src = reinterpret_cast<const uint32_t*>(T->job + B.job0);
        uint32_t* dst = reinterpret_cast<uint32_t*>(s_job);
        const int nw = B.njobs * (int)(sizeof(AbsorbJobDev) / 4);
        for (int i = (int)threadIdx.x; i < nw; i += 256) dst[i] = src[i];
    }
    __syncthreads();  // (every thread of the block reaches it: none has returned above)
    const long long c = (long long)(blockIdx.x - T->first[b]) * 256 + threadIdx.x;
    bool flip = false;
    if (c < (long long)B.w * B.h) {
        const int cx = (int)(c / B.h), x = B.x0 + cx, y = B.y0 + (int)(c - (long long)cx * B.h);
        int val = -1;  // undecided
        for (int k = B.njobs - 1; k >= 0; k--) {
            const AbsorbJobDev& J = s_job[k];
            const int i = x - J.x0, j = y - J.y0;
            if ((unsigned)i >= (unsigned)J.w || (unsigned)j >= (unsigned)J.h) continue;
            const uint8_t v = J.layout ? J.at[(size_t)j * (size_t)J.stride + (size_t)i] : J.at[(size_t)i * (size_t)J.stride + (size_t)j];
            const bool occupied = J.layout ? (int8_t)v > 0 : v != 0;  // prepared_byte's predicate
            const bool unknown = J.layout && v == 0xffu;              // -1 of an OccupancyGrid
            if (mode == ABSORB_OVERWRITE || (mode == ABSORB_OCCUPIED && occupied) || (mode == ABSORB_KNOWN && !unknown)) {
                val = occupied ? 1 : 0;
                break;
            }
        }
        if (val >= 0) {
            uint8_t* p = B.occ + (size_t)x * (size_t)B.pH + (size_t)y;
            const uint8_t old = *p;
            if (old != (uint8_t)val) *p = (uint8_t)val;
            flip = (old != 0) != (val != 0);
        }
    }
    prior_count_flips(&T->changed[B.prior], flip);
}

// ---------------------------------------------------------------- ... into prior maps that grow (DESIGN.md section 3.21)
// fxjps_absorb_prior_grow: every named prior is written anew, into a NEW buffer of the grown extents, as the n sequential
// canvases of st:212-220 kept job after job would leave it.  The host has folded the geometry: per prior the grown
// extents, where the old prior's cell (0, 0) lies in them (the sum of every job's at_pre) and the union box of its
// rectangles; per job where its cell (0, 0) lies in the FINAL frame (its at_raw plus the at_pre of every later job on the
// prior).  ONE launch over the cells of the new priors, the blocks dealt to the priors by GrowTable::first.  A thread owns
// one cell of a new prior, adjacent lanes adjacent y.  Outside the union box it does not walk the jobs (a block that
// misses the box does not even copy them); inside it walks the block's LDS copy of the prior's job records from the last
// to the first and stops at the first job that decides the cell under the mode's rule, exactly as k_prior_absorb does.
// An undecided cell takes the old prior's byte if it lies in the old prior's placement, else 0.  Every cell of the new
// buffer is stored exactly once, by its owner, with a plain byte store; the old prior and the staged raws are only read,
// so no thread reads a byte another writes, no atomic touches a map byte and the order of the threads does not matter.
// Flips against the old byte (0 where the old prior has no cell) are counted as k_prior_absorb counts them.
struct GrowBoxDev {
    const uint8_t* old;     // the prior [oW][oH] as it is
    uint8_t* out;           // the grown prior [nW][nH]: a buffer of its own
    int32_t oW, oH, sx, sy; // the old extents, and the new cell that old cell (0, 0) lies on
    int32_t nW, nH;
    int32_t x0, y0, w, h;   // the union of the prior's rectangles in the new frame: every cell of it lies inside [nW][nH]
    int32_t job0, njobs;    // its jobs, GrowTable::job[job0 .. job0 + njobs), in job order
    int32_t prior, pad_;    // ... and its counter
};
struct GrowTable {
    unsigned long long changed[ABSORB_PRIORS_MAX];  // staged as 0; what comes back
    uint32_t first[ABSORB_PRIORS_MAX + 1];          // first[b]: the first block of prior b; first[nbox]: the grid size
    int32_t nbox, mode;
    GrowBoxDev box[ABSORB_PRIORS_MAX];
    AbsorbJobDev job[ABSORB_JOBS_MAX];              // (x0, y0: in the grown prior's frame; the rectangle lies inside it)
    int32_t k0[ABSORB_PRIORS_MAX][2];               // WINDOW only (behind everything k_prior_grow<false> reads): see below
};

// WINDOW (fxjps_absorb_prior_slide, DESIGN.md section 3.22): the new buffer [nW][nH] holds only the cells [k0, k0 + (nW, nH))
// of the grown frame, the prior's keep window; the grown frame itself exists nowhere.  A thread owns one cell of the WINDOW,
// adjacent lanes adjacent y; its coordinates in the grown frame are the window's plus k0, and everything else -- sx, sy, the
// union box (which the host has clipped to the window) and the jobs' x0, y0 -- stays in the grown frame, so the job walk,
// the predicates, the old-byte fallback and the ballot count are the same lines.  Of a rectangle only the rows inside the
// window are staged: a thread reads a raw only at a cell of its own, which lies in the window.  k0 = 0 with the grown
// extents is a prior that is not cut.  <false> is fxjps_absorb_prior_grow's kernel: it reads no k0 and adds none.
template <bool WINDOW> __global__ __launch_bounds__(256) void k_prior_grow(GrowTable* __restrict__ T) {
    __shared__ AbsorbJobDev s_job[ABSORB_JOBS_MAX];
    const int nbox = T->nbox, mode = T->mode;
    int b = 0;  // (block-uniform)
    while (b + 1 < nbox && T->first[b + 1] <= blockIdx.x) b++;
    const GrowBoxDev B = T->box[b];
    const int kx = WINDOW ? T->k0[b][0] : 0, ky = WINDOW ? T->k0[b][1] : 0;
    const long long cells = (long long)B.nW * B.nH;
    const long long c0 = (long long)(blockIdx.x - T->first[b]) * 256;
    // does any of the block's cells [c0, c1] lie in a column of the union box?  (block-uniform; columns only: a block that
    // spans more than one column covers every y of some of them)
    const long long c1 = c0 + 255 < cells - 1 ? c0 + 255 : cells - 1;
    const int bx0 = (int)(c0 / B.nH) + kx, bx1 = (int)(c1 / B.nH) + kx;
    const bool near_box = bx0 < B.x0 + B.w && bx1 >= B.x0;
    if (near_box) {
        const uint32_t* __restrict__ src = reinterpret_cast<const uint32_t*>(T->job + B.job0);
        uint32_t* dst = reinterpret_cast<uint32_t*>(s_job);
        const int nw = B.njobs * (int)(sizeof(AbsorbJobDev) / 4);
        for (int i = (int)threadIdx.x; i < nw; i += 256) dst[i] = src[i];
        __syncthreads();  // (near_box is block-uniform and no thread has returned above: all of them reach it or none)
    }
    const long long c = c0 + threadIdx.x;
    bool flip = false;
    if (c < cells) {
        const int wx = (int)(c / B.nH), wy = (int)(c - (long long)wx * B.nH);  // the cell in the new buffer ...
        const int x = wx + kx, y = wy + ky;                                    // ... and in the grown frame
        int val = -1;  // undecided
        if (near_box && (unsigned)(x - B.x0) < (unsigned)B.w && (unsigned)(y - B.y0) < (unsigned)B.h) {
            for (int k = B.njobs - 1; k >= 0; k--) {
                const AbsorbJobDev& J = s_job[k];
                const int i = x - J.x0, j = y - J.y0;
                if ((unsigned)i >= (unsigned)J.w || (unsigned)j >= (unsigned)J.h) continue;
                const uint8_t v = J.layout ? J.at[(size_t)j * (size_t)J.stride + (size_t)i] : J.at[(size_t)i * (size_t)J.stride + (size_t)j];
                const bool occupied = J.layout ? (int8_t)v > 0 : v != 0;  // prepared_byte's predicate
                const bool unknown = J.layout && v == 0xffu;              // -1 of an OccupancyGrid
                if (mode == ABSORB_OVERWRITE || (mode == ABSORB_OCCUPIED && occupied) || (mode == ABSORB_KNOWN && !unknown)) {
                    val = occupied ? 1 : 0;
                    break;
                }
            }
        }
        const int ox = x - B.sx, oy = y - B.sy;
        uint8_t old = 0;
        if ((unsigned)ox < (unsigned)B.oW && (unsigned)oy < (unsigned)B.oH) old = B.old[(size_t)ox * (size_t)B.oH + (size_t)oy];
        const uint8_t byte = val >= 0 ? (uint8_t)val : old;
        B.out[(size_t)wx * (size_t)B.nH + (size_t)wy] = byte;
        flip = (old != 0) != (byte != 0);
    }
    prior_count_flips(&T->changed[B.prior], flip);
}
