// fxjps_host_search.cpp -- see fxjps_host_search.h.  Plain C++17, built with -ffp-contract=off -fno-fast-math: f = g + h
// is one rounded add, std::sqrt the correctly rounded root the device's sqrt_u28 is pinned to.
#include "fxjps_host_search.h"

#include <cmath>
#include <cstdlib>
#include <cstring>

namespace fxh {

namespace {

constexpr uint32_t JD_K = 0x1FFFu, JD_J = 0x8000u;
constexpr uint32_t NO_PARENT = 0xFFFFFFFFu;

constexpr int nbit(int dx, int dy) { return ((dx + 1) * 3 + (dy + 1)) - ((((dx + 1) * 3 + (dy + 1)) > 4) ? 1 : 0); }
constexpr uint32_t jd_slot(uint32_t code) { return code - (code >= 3u ? 1u : 0u) - (code >= 5u ? 1u : 0u) - (code >= 7u ? 1u : 0u); }

inline uint64_t bits_of(double v) {
    uint64_t b;
    std::memcpy(&b, &v, sizeof b);
    return b;
}

template <int HC>
inline double heuristic(int ax, int ay, int bx, int by) {  // jps1.py:3-12
    if (HC == 1) {
        const int xd = std::abs(bx - ax), yd = std::abs(by - ay);
        return (double)(xd > yd ? 14 * yd + 10 * (xd - yd) : 14 * xd + 10 * (yd - xd));
    }
    const int dx = bx - ax, dy = by - ay;
    return std::sqrt((double)(uint32_t)(dx * dx + dy * dy));
}
template <int HC>
inline double seg_len(int cx, int cy, int jx, int jy) {  // jps1.py:232-246
    const int lx = std::abs(cx - jx), ly = std::abs(cy - jy);
    if (HC == 1) return (lx != 0 && ly != 0) ? (double)(lx * 14) : (double)((lx + ly) * 10);
    return std::sqrt((double)(uint32_t)(lx * lx + ly * ly));
}

// Straight ray: first cell at or after `pos` on `line` of travel direction `di` that is occupied, forced, or the goal
// (gpos: its position on this line, or -1).  True iff that cell is free (a jump point).
inline bool scan_line(const Maps& M, int di, int line, int pos, int gpos) {
    const int sgn = (di & 1) ? -1 : 1;
    const BmWord* L = M.bm + (size_t)(di * M.LINES + line) * M.WORDS;
    int w = pos >> 6;
    const int b = pos & 63;
    uint64_t m = sgn > 0 ? (~0ull << b) : (~0ull >> (63 - b));
    const int gw = gpos >> 6;
    const uint64_t gbit = gpos >= 0 ? (1ull << (gpos & 63)) : 0ull;
    while (w >= 0 && w < M.WORDS) {
        const BmWord u = L[w];
        uint64_t s = u.stop;
        if (w == gw) s |= gbit;
        s &= m;
        if (s) {
            const int bit = sgn > 0 ? __builtin_ctzll(s) : 63 - __builtin_clzll(s);
            return !((u.occ >> bit) & 1ull);
        }
        w += sgn;
        m = ~0ull;
    }
    return false;  // unreachable: the border always stops the ray
}
// jump(c, d) != None for a straight d from padded cell (px, py)   jps1.py:97-103, 132-162
inline bool scan_ray(const Maps& M, int px, int py, int dx, int dy, int gpx, int gpy) {
    if (dx != 0) return scan_line(M, dx > 0 ? 0 : 1, py, px + dx, py == gpy ? gpx : -1);
    return scan_line(M, dy > 0 ? 2 : 3, px, py + dy, px == gpx ? gpy : -1);
}
// the two straight sub-jumps of a diagonal step (jps1.py:116-117)
inline bool scan_two(const Maps& M, int ox, int oy, int dx, int dy, int gpx, int gpy) {
    return scan_ray(M, ox, oy, dx, 0, gpx, gpy) || scan_ray(M, ox, oy, 0, dy, gpx, gpy);
}

// jump(c, d) for one ray of a node (expand_jd): the record says how far the goal-free jump gets and whether it ends on a
// jump point; the goal on the ray at or before that cell is the jump point, and the cells of a diagonal ray on the goal's
// row and column are looked at with the scan words.  True: the jump point's padded cell in (*jxp, *jyp).
inline bool expand_ray(const Maps& M, const uint16_t* rec, int cpx, int cpy, uint32_t code, int gpx, int gpy, int* jxp, int* jyp) {
    const int dx = (int)(code >> 2) - 1, dy = (int)(code & 3u) - 1;
    const bool diag = dx != 0 && dy != 0, alongY = dx == 0;
    const uint32_t v = rec[jd_slot(code) & 7u];
    const int ax = dx > 0 ? gpx - cpx : cpx - gpx, ay = dy > 0 ? gpy - cpy : cpy - gpy;
    const bool gline = diag ? (ax == ay) : (alongY ? gpx == cpx : gpy == cpy);
    const int kg = alongY ? ay : ax;
    const int k = (int)(v & JD_K);
    const bool jp = (v & JD_J) != 0u;
    const bool goal_on = gline && kg >= 1 && kg <= k;
    bool has = goal_on ? (kg < k ? true : jp) : jp;
    int kres = goal_on ? kg : k;
    if (diag && ((ax >= 1 && ax < kres) || (ay >= 1 && ay < kres))) {
        const int k1 = ax < ay ? ax : ay, k2 = ax < ay ? ay : ax;
        if (k1 >= 1 && k1 < kres && scan_two(M, cpx + k1 * dx, cpy + k1 * dy, dx, dy, gpx, gpy)) {
            has = true;
            kres = k1;
        } else if (k2 != k1 && k2 >= 1 && k2 < kres && scan_two(M, cpx + k2 * dx, cpy + k2 * dy, dx, dy, gpx, gpy)) {
            has = true;
            kres = k2;
        }
    }
    *jxp = cpx + kres * dx;
    *jyp = cpy + kres * dy;
    return has;
}

inline bool occupied(const Maps& M, int x, int y) {  // the +y scan words: line = padded x, bit = padded y
    return (M.bm[(size_t)(2 * M.LINES + x + 1) * M.WORDS + ((y + 1) >> 6)].occ >> ((y + 1) & 63)) & 1ull;
}

}  // namespace

uint32_t dirlut_entry(uint32_t pd, uint32_t nbm) {
    auto occ = [&](int dx, int dy) -> bool { return (nbm >> nbit(dx, dy)) & 1u; };
    auto blocked = [&](int dx, int dy) -> bool {  // blocked(c, dx, dy), jps1.py:14-31, border == occupied
        if (dx != 0 && dy != 0) return (occ(dx, 0) && occ(0, dy)) || occ(dx, dy);
        return occ(dx, dy);
    };
    uint32_t codes[8];
    int n = 0;
    auto add = [&](int dx, int dy) { codes[n++] = (uint32_t)((dx + 1) * 4 + (dy + 1)); };
    const int pdx = (int)(pd >> 2) - 1, pdy = (int)(pd & 3u) - 1;
    if (pd == PD_NONE) {  // :51-56
        static const int all8[8][2] = {{-1, 0}, {0, -1}, {1, 0}, {0, 1}, {-1, -1}, {-1, 1}, {1, -1}, {1, 1}};
        for (auto& d : all8)
            if (!blocked(d[0], d[1])) add(d[0], d[1]);
    } else if (pdx < -1 || pdx > 1 || pdy < -1 || pdy > 1) {
        // not a direction code
    } else if (pdx != 0 && pdy != 0) {  // :59-73
        if (!blocked(0, pdy)) add(0, pdy);
        if (!blocked(pdx, 0)) add(pdx, 0);
        if ((!blocked(0, pdy) || !blocked(pdx, 0)) && !blocked(pdx, pdy)) add(pdx, pdy);
        if (blocked(-pdx, 0) && !blocked(0, pdy)) add(-pdx, pdy);
        if (blocked(0, -pdy) && !blocked(pdx, 0)) add(pdx, -pdy);
    } else if (pdx == 0) {  // :76-83; the guard at :77 tests the node itself, which is free
        if (!blocked(0, pdy)) add(0, pdy);
        if (blocked(1, 0)) add(1, pdy);
        if (blocked(-1, 0)) add(-1, pdy);
    } else {  // :85-92
        if (!blocked(pdx, 0)) {
            add(pdx, 0);
            if (blocked(0, 1)) add(pdx, 1);
            if (blocked(0, -1)) add(pdx, -1);
        }
    }
    uint32_t v = 0;
    for (int g = 0; g < 8; g++) v |= (g < n ? codes[g] : DIR_NONE) << (4 * g);
    return v;
}

void dirlut_fill(uint32_t* lut) {
    for (uint32_t pd = 0; pd < 11; pd++)
        for (uint32_t m = 0; m < 256; m++) lut[pd * 256 + m] = dirlut_entry(pd, m);
}

// ---- binary heap on the full key (f bits, then x, then y: jps1.py:192, 198)
static inline bool key_less(uint64_t af, uint32_t ac, uint64_t bf, uint32_t bc) { return af < bf || (af == bf && ac < bc); }

void Searcher::heap_push(HeapEnt e) {
    size_t i = heap_.size();
    heap_.push_back(e);
    HeapEnt* a = heap_.data();
    while (i > 0) {
        const size_t p = (i - 1) >> 1;
        if (!key_less(e.f, e.cell, a[p].f, a[p].cell)) break;
        a[i] = a[p];
        i = p;
    }
    a[i] = e;
}

Searcher::HeapEnt Searcher::heap_pop() {
    HeapEnt* a = heap_.data();
    const HeapEnt top = a[0];
    const HeapEnt last = heap_.back();
    heap_.pop_back();
    const size_t n = heap_.size();
    if (n > 0) {
        size_t i = 0;
        for (;;) {
            size_t c = 2 * i + 1;
            if (c >= n) break;
            if (c + 1 < n && key_less(a[c + 1].f, a[c + 1].cell, a[c].f, a[c].cell)) c++;
            if (!key_less(a[c].f, a[c].cell, last.f, last.cell)) break;
            a[i] = a[c];
            i = c;
        }
        a[i] = last;
    }
    return top;
}

template <int HC>
Result Searcher::search(const Maps& M, const uint32_t* dirlut, int sx, int sy, int gx, int gy, int max_len, uint32_t* out_path, uint64_t max_pops) {
    Result R;
    const int H = M.H;
    const size_t ncell = (size_t)M.W * (size_t)H;
    if (tab_.size() != ncell || gen_ >= 0x7FFFFFFEu) {  // another grid shape, or the tags ran out: every entry reads as never written
        tab_.assign(ncell, Ent{0.0, NO_PARENT, 0u});
        gen_ = 0;
    }
    gen_++;
    const uint32_t live = gen_ << 1;
    Ent* tab = tab_.data();
    heap_.clear();
    const int gpx = gx + 1, gpy = gy + 1;
    const uint32_t sidx = (uint32_t)(sx * H + sy), goal_cell = ((uint32_t)gx << 13) | (uint32_t)gy;
    // gscore = {start: 0}; heappush(f(start), start)   jps1.py:185-192
    tab[sidx] = Ent{0.0, NO_PARENT, live};
    heap_push(HeapEnt{bits_of(heuristic<HC>(sx, sy, gx, gy)), ((uint32_t)sx << 13) | (uint32_t)sy, sidx});
    while (!heap_.empty()) {
        const HeapEnt cur = heap_pop();  // :198
        R.pops++;
        if (R.pops > max_pops) {
            R.len = QI_WATCHDOG;
            return R;
        }
        const Ent ec = tab[cur.idx];
        if (cur.cell == goal_cell) {  // :199-208: walk came_from back to the start
            R.cost = ec.g;
            walk_.clear();
            uint32_t i = cur.idx;
            for (;;) {
                walk_.push_back(i);
                if (i == sidx) break;
                i = tab[i].par;
            }
            const size_t n = walk_.size();
            if (n > (size_t)max_len) {
                R.len = Q_PATH_TOO_LONG;
                return R;
            }
            for (size_t k = 0; k < n; k++) {
                const uint32_t c = walk_[n - 1 - k];
                out_path[k] = ((c / (uint32_t)H) << 16) | (c % (uint32_t)H);
            }
            R.len = (int32_t)n;
            return R;
        }
        if (ec.tag & 1u) continue;  // stale duplicate of a closed node: a provable no-op
        tab[cur.idx].tag = live | 1u;  // close_set.add   :210
        const int cx = (int)(cur.cell >> 13), cy = (int)(cur.cell & 0x1FFFu);
        // direction(c, came_from[c]) of the parent the table holds NOW (:168, :40-47)
        uint32_t pd = PD_NONE;
        if (ec.par != NO_PARENT) {
            const int px = (int)(ec.par / (uint32_t)H), py = (int)(ec.par % (uint32_t)H);
            const int ddx = cx > px ? 1 : (cx < px ? -1 : 0), ddy = cy > py ? 1 : (cy < py ? -1 : 0);
            pd = (uint32_t)((ddx + 1) * 4 + (ddy + 1));
        }
        const uint16_t* rec = M.jd + ((size_t)(cx + 1) * (size_t)M.NS + (size_t)(cy + 1)) * 8u;
        const uint32_t nb8 = ((rec[0] >> 13) & 3u) | (((rec[1] >> 13) & 3u) << 2) | (((rec[2] >> 13) & 3u) << 4) | (((rec[3] >> 13) & 3u) << 6);
        uint32_t codes = dirlut[pd * 256u + nb8];
        for (int ray = 0; ray < 8; ray++, codes >>= 4) {  // identifySuccessors :166-179 and the relaxation :215-228
            const uint32_t code = codes & 0xFu;
            if (code == DIR_NONE) break;  // (the directions come first)
            int jxp, jyp;
            if (!expand_ray(M, rec, cx + 1, cy + 1, code, gpx, gpy, &jxp, &jyp)) continue;
            const int jx = jxp - 1, jy = jyp - 1;
            const uint32_t jidx = (uint32_t)(jx * H + jy);
            Ent& ej = tab[jidx];
            const bool seen = (ej.tag >> 1) == gen_;
            if (seen && (ej.tag & 1u)) continue;  // :218
            const double tg = ec.g + seg_len<HC>(cx, cy, jx, jy);  // :221
            if (!seen || tg < ej.g) {  // :223-224 (strict <, Q17; "not in pqueue" == never pushed, Q2)
                ej = Ent{tg, cur.idx, live};
                const double f = tg + heuristic<HC>(jx, jy, gx, gy);  // :227
                heap_push(HeapEnt{bits_of(f), ((uint32_t)jx << 13) | (uint32_t)jy, jidx});
                R.pushes++;
            }
        }
    }
    return R;  // (0, t)   :230
}

Result Searcher::plan(const Maps& M, const uint32_t* dirlut, int hchoice, int sx, int sy, int gx, int gy, int max_len, uint32_t* out_path,
                      uint64_t max_pops) {
    Result R;
    // ---- outcomes that need no search (run_query: results-equivalent to the exhaustive run)
    if (sx < 0 || sy < 0 || sx >= M.W || sy >= M.H) {
        R.len = Q_BAD_START;
        return R;
    }
    if (sx == gx && sy == gy) {  // the first pop is the goal: jps1.py:199-208
        if (max_len < 1) {
            R.len = Q_PATH_TOO_LONG;
            return R;
        }
        out_path[0] = ((uint32_t)sx << 16) | (uint32_t)sy;
        R.len = 1;
        return R;
    }
    if (gx < 0 || gy < 0 || gx >= M.W || gy >= M.H) return R;
    if (occupied(M, gx, gy)) return R;  // an occupied goal is never returned by a jump (jps1.py:99-103)
    if (M.comp != nullptr && !occupied(M, sx, sy)) {  // a goal in another component of a free start: (0, t)
        const auto root = [&](int i) -> int {
            int p = M.comp[i];
            if (p < 0) return -1;
            for (int step = 0; step < 256 && p != i; step++) {
                i = p;
                p = M.comp[i];
            }
            return p == i ? i : -2;
        };
        const int cs = root(sx * M.H + sy), cg = root(gx * M.H + gy);
        if (cs >= 0 && cg >= 0 && cg != cs) return R;
    }
    R = hchoice == 1 ? search<1>(M, dirlut, sx, sy, gx, gy, max_len, out_path, max_pops)
                     : search<2>(M, dirlut, sx, sy, gx, gy, max_len, out_path, max_pops);
    if (R.len == 0 || R.len <= QI_WATCHDOG) R.cost = 0.0;
    return R;
}

}  // namespace fxh
