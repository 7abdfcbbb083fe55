// fxjps_kernels.hip.inc -- device code of libfxjps.so (gfx950 / CDNA4, wave64).
//
// Kernels (DESIGN.md section 3):
//   k_derive_rows / k_derive_cols / k_derive_cellinfo   occupancy bytes -> scan bitmaps + cell-info map (whole map, or the
//                                                       rectangle / rows / columns a cell update can reach)
//   k_ccl_init / k_ccl_merge / k_ccl_flatten            4-connected components of the free cells (union-find forest)
//   k_update_cells / k_ccl_update                       cell updates; small ones united into the forest
//   k_prepare_grid / k_transpose_map                    the callers' grid preparation, wire / image adapters
//   k_search<HC, TRK, DIRECT, MG>                       one (start, goal) query per wavefront, whole A*+JPS on device
//                                                       (heuristic; read-set recording; visited table indexed by the cell;
//                                                       each query on the grid of its own slot)
//   k_scan_len / k_gather_paths                         dense per-query path slots -> CSR
//   k_replan_scan / k_replan_gather                     a batch's CSR out of the previous batch's and a sub-batch's results
//   k_waypoint_ccst                                     the ccst node's waypoint selection, one wavefront per path
//   k_sqrt_selftest / k_selftest_wavemin / k_selftest_openlist   arithmetic and open-list proofs used by the tests
//
// The search follows the reference's semantics (scripts/jps1.py:49-230) but is organised for a 64-lane
// wavefront: every loop iteration takes up to KN = 16 of the smallest open-list entries, deals the lanes out to their
// rays (lane = (node, direction the node really has)) and expands all of them at once (straight rays are
// find-first-set scans over bit-packed "stop" maps, diagonal rays read one cell-info word per step), the visited table
// is probed for all successors in one round trip, and the nodes are committed in the reference's pop order if they
// really are the next pops.  The open list has three tiers: one entry per lane in registers, sorted across the lanes,
// 256 entries in LDS, the rest in global memory.

namespace fx {

constexpr int WAVE = 64;
#define FX_RARE(c) __builtin_expect(!!(c), 0)
#define FX_USUAL(c) __builtin_expect(!!(c), 1)
#ifndef FXJPS_WPB
#define FXJPS_WPB 8
#endif
#ifndef FXJPS_OCC
#define FXJPS_OCC 4
#endif
constexpr int WPB = FXJPS_WPB;  // independent wavefronts per block (they share only the 11 KB nodeNeighbours table in LDS)
constexpr int OCC = FXJPS_OCC;  // wavefronts per SIMD the register and LDS budgets are sized for (<= 128 VGPRs, 2 blocks per CU)
constexpr uint32_t KEY_CLOSED = 0x80000000u;
constexpr uint32_t CELL_MASK = 0x03FFFFFFu;  // x:13 | y:13
constexpr uint32_t PD_NONE = 5;              // (dx+1)*4 + (dy+1) with dx = dy = 0
constexpr uint32_t SLOT_NONE = 0xFFFFFFFFu;
// Visited-table entries carry a 6-bit generation tag (key bit 30 = low bit, par bits 27..31 = high bits): an entry
// is live only if its tag equals the running query's, so the table is never cleared between queries -- only when
// a wavefront's generation counter wraps (every 63 searches).  memset(0xFF) leaves tag 63 = "never written".
constexpr uint32_t PAR_MASK = 0x07FFFFFFu;  // parent slot
constexpr uint32_t PAR_NONE = PAR_MASK;     // came_from has no entry (the start node)
constexpr uint32_t GEN_WRAP = 63u;
__host__ __device__ constexpr uint32_t ent_gen(uint32_t key, uint32_t par) { return ((key >> 30) & 1u) | ((par >> 27) << 1); }
__host__ __device__ constexpr uint32_t gen_key_bits(uint32_t gen) { return (gen & 1u) << 30; }
__host__ __device__ constexpr uint32_t gen_par_bits(uint32_t gen) { return (gen >> 1) << 27; }
constexpr uint32_t DIR_NONE = 0xFu;

// internal per-query codes (never leave the library)
constexpr int32_t QI_TABLE_FULL = -100;
constexpr int32_t QI_FAR_FULL = -101;
constexpr int32_t QI_WATCHDOG = -102;  // a loop bound that no valid search reaches was hit

struct __attribute__((aligned(16))) TEnt {  // visited-table entry: gscore / came_from / close_set
    double g;      // gscore[node]                      jps1.py:187,226
    uint32_t key;  // x:13 | y:13 | pd:4 << 26 | generation low bit << 30 | closed << 31
    uint32_t par;  // table slot of came_from[node] (27 bits, jps1.py:225) | generation high bits << 27
};

struct __attribute__((aligned(16))) FarEnt {  // open-list entry spilled to global memory
    uint64_t fbits;  // f as raw bits (f >= +0, so unsigned order == numeric order)
    uint32_t xyd;    // x:13 | y:13 | pd:4   (compare as u32 == (x, y) tuple order)
    uint32_t slot;   // table slot of the node; in the slotless layout (see WaveLdsT) the node's cell info instead
};

struct __attribute__((aligned(16))) BmWord {  // 64 cells of one scan line
    uint64_t stop;  // occupied | forced-neighbour cell for this travel direction  jps1.py:134-137,150-153
    uint64_t occ;   // occupied (1-cell border and everything outside the grid included)
};

// Device-resident grid.  Padded coordinates: cell (x, y) lives at (x+1, y+1); the 1-cell border is
// occupied, which reproduces every out-of-bounds answer of blocked() (jps1.py:15-18).
struct GridDev {
    const BmWord* bm;     // [4][LINES][WORDS]: travel +x, -x (line = padded y, bit = padded x), +y, -y (line = padded x);
                          // behind them [4][DLINES][WORDS]: the diagonal travel directions (+,+), (-,-), (+,-), (-,+), one
                          // line per diagonal (id = x - y + PH - 1 for the first two, x + y for the others, padded
                          // coordinates), bit = padded x, and the word holds {stop = "a diagonal jump returns this cell when
                          // it gets here", occ = "... returns None here"} (see k_derive_diag)
    const uint16_t* ci;   // [PW][NS] cell info: bits 0-7 = occupancy of the 8 neighbours, bits 8-11 = "a straight
                          //          jump from here along +x / -x / +y / -y is not None" for rays without the goal,
                          //          bits 12-13 / 14-15 = how many read-set tiles beyond its own the cell's +-x / +-y
                          //          rays reach (3 = more: the whole row / column)
    const uint8_t* nb8;   // [PW][NS] the neighbour byte alone (input of k_derive_cols / k_derive_cellinfo, tests)
    const uint16_t* jd;   // [PW][NS][8] jump distances: what jump(c, d) returns from every cell c along each of the eight
                          //             directions when the goal is nowhere near (k_derive_jd) -- steps to the cell that ends
                          //             the ray (13 bits) | "that cell is a jump point" << 15
    const int32_t* comp;  // [W*H] 4-connected component label of free cells
    int32_t W, H, PW, PH, NS, LINES, WORDS;
    int32_t DLINES;       // PW + PH - 1 diagonals of either orientation
    int32_t tsh;          // read-set tiles are (1 << tsh) cells a side: at most 64 x 64 of them cover the grid
};

struct SearchArgs {
    GridDev G;
    const int32_t* starts;
    const int32_t* goals;
    const uint32_t* order;  // query ids to run (nullptr: 0..nrun-1)
    uint32_t nrun;
    int32_t max_len;
    uint32_t* out_path;  // [nq][max_len] x<<16|y
    int32_t* out_len;
    double* out_cost;
    unsigned long long* out_counters;  // [0] pops, [1] pushes, [2] far refills, [3] slow pops, [7] table wipes, [8..] FXJPS_PROF cycles
    TEnt* tables;
    FarEnt* far;
    uint32_t nbuckets;      // per-wavefront table = BUCKET * nbuckets entries (hashed tables: any number of buckets)
    uint32_t tab_usable;    // hashed tables: entries a search may insert before it gives the query to the large pool
    uint32_t direct_ly;     // k_search<.., .., true>: the table is indexed by the cell, slot = x << direct_ly | y (no hashing)
    uint32_t banded;        // k_search<2, ..>: the far band of the open list is a set of f bands (large grids, see NBANDS)
    uint32_t far_cap;
    uint32_t near_max;            // the near band of the far tier is split when it holds more entries than this at a refill
    unsigned int* next;           // work counter
    unsigned long long max_pops;  // watchdog: every wavefront leaves its query after this many pops
    uint32_t* wave_gen;           // [nwaves] generation counter of each wavefront's visited table
    unsigned long long* qstat;    // diagnostics (FXJPS_QSTAT=1, else nullptr): per query {start, end (100 MHz ticks), pops, wavefront}
    unsigned long long* qread;    // k_search<HC, true>: [nq][128] read-set bitmaps of each searched query (see ReadSet)
    uint32_t solo = 0;            // spread launch: this many live wavefronts per block (and, by its LDS size, per CU); 0: all of them
    uint32_t wave_base = 0;       // ... whose scratch slots start here
    uint32_t q0 = 0;              // position in `order` of this launch's first query
    uint32_t* started = nullptr;  // solo launch: counts its blocks as they start (the batch's launch waits for all of them)
    uint32_t single = 0;          // one query, one wavefront, no work counter: (start, goal) = imm, results straight into the
    int32_t imm[4] = {0, 0, 0, 0};  // host's pinned buffers (the node's real call: jps1.method, one query per tick)
    unsigned long long* host_counters = nullptr;  // ... out_counters too: zeroed by the kernel, copied there when it is done (no memset, no copy back)
    // k_search<.., .., .., true> (grid slots): query q runs on grids[grid_ids[q]] instead of G (the host checked every id)
    const GridDev* grids = nullptr;     // [FXJPS_MAX_GRID_SLOTS] descriptors of the context's slots
    const int32_t* grid_ids = nullptr;  // [nq]
    // a plain batch's results straight to the host as each query ends (DESIGN.md section 7; all null / zero: off).  Device
    // pointers of pinned host memory: the arena of packed cells and how many it holds, per query where its cells begin in
    // it (-1: they did not fit), its length and its cost; and the arena's cursor, in device memory.
    uint32_t* host_cells = nullptr;
    unsigned long long host_cap = 0ull;
    unsigned long long* host_cursor = nullptr;
    long long* host_base = nullptr;
    int32_t* host_len = nullptr;
    double* host_cost = nullptr;
};

// nodeNeighbours (jps1.py:49-93) as a table: entry [pd*256 + nbm] holds, for each of a node's 8 rays,
// the direction code (dx+1)*4+(dy+1) it follows or DIR_NONE.  Filled by the host at fxjps_create
// (dirlut_entry in fxjps.hip restates the reference branch by branch).  Uniform index -> scalar load.
__constant__ uint32_t c_dirlut[11 * 256];

// ---------------------------------------------------------------- small helpers
__host__ __device__ constexpr int nbit(int dx, int dy) {
    return ((dx + 1) * 3 + (dy + 1)) - ((((dx + 1) * 3 + (dy + 1)) > 4) ? 1 : 0);
}
__device__ __forceinline__ bool occN(uint32_t m, int dx, int dy) { return (m >> nbit(dx, dy)) & 1u; }

__device__ __forceinline__ uint64_t wave_min_u64(uint64_t v) {  // shuffle form (reference for the DPP form)
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        uint64_t t = __shfl_xor(v, o, WAVE);
        v = t < v ? t : v;
    }
    return v;
}
__device__ __forceinline__ uint32_t wave_min_u32(uint32_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        uint32_t t = __shfl_xor(v, o, WAVE);
        v = t < v ? t : v;
    }
    return v;
}

// sqrt((double)n) for the integers the planner takes roots of (n = dx^2 + dy^2 <= 2 * 8189^2 < 2^28): one v_rsq_f64, one
// coupled Newton step and one correction in fused multiply-adds -- the generic sqrt() without its scaling of tiny / huge
// arguments and without its second correction (nine instructions that never change the result in this range).  The result must be the correctly rounded root, bit for bit
// what math.sqrt returns (jps1.py:12,246): fxjps_selftest_sqrt runs THIS function over every possible argument and
// the GPU suite compares all of them with the host's sqrt.
__device__ __forceinline__ double sqrt_u28(uint32_t n) {
    const double x = (double)n;
    const double y = __builtin_amdgcn_rsq(x);
    double g = x * y, h = 0.5 * y;
    const double r = __builtin_fma(-h, g, 0.5);
    g = __builtin_fma(g, r, g);
    h = __builtin_fma(h, r, h);
    const double d = __builtin_fma(-g, g, x);
    g = __builtin_fma(d, h, g);
    return n == 0u ? 0.0 : g;
}

template <int HC>
__device__ __forceinline__ double heuristic(int ax, int ay, int bx, int by) {  // jps1.py:3-12
    if (HC == 1) {
        int xd = abs(bx - ax), yd = abs(by - ay);
        int v = xd > yd ? 14 * yd + 10 * (xd - yd) : 14 * xd + 10 * (yd - xd);
        return (double)v;
    }
    int dx = bx - ax, dy = by - ay;
    return sqrt_u28((uint32_t)(__mul24(dx, dx) + __mul24(dy, dy)));  // |dx|, |dy| < 2^13
}
template <int HC>
__device__ __forceinline__ double seg_len(int cx, int cy, int jx, int jy) {  // jps1.py:232-246
    int lx = abs(cx - jx), ly = abs(cy - jy);
    if (HC == 1) {
        if (lx != 0 && ly != 0) return (double)(lx * 14);
        return (double)((lx + ly) * 10);
    }
    return sqrt_u28((uint32_t)(__mul24(lx, lx) + __mul24(ly, ly)));
}

__device__ __forceinline__ int dir_index(int dx, int dy) { return dx != 0 ? (dx > 0 ? 0 : 1) : (dy > 0 ? 2 : 3); }

// Straight ray: first cell at or after `pos` on `line` of travel direction `di` that is occupied,
// forced, or the goal (gpos = the goal's position on this line, or -1) -- the closed form of the
// loops at jps1.py:132-162 (and of the checks at :99-103 for the first cell).  Returns true iff
// that cell is free (a jump point); its position in *rp.
__device__ __forceinline__ bool scan_line(const GridDev& G, int di, int line, int pos, int gpos, int* rp) {
    const int sgn = (di & 1) ? -1 : 1;
    const BmWord* L = G.bm + (size_t)(di * G.LINES + line) * G.WORDS;
    int w = pos >> 6;
    const int b = pos & 63;
    uint64_t m = sgn > 0 ? (~0ull << b) : (~0ull >> (63 - b));
    const int gw = gpos >> 6;
    const uint64_t gbit = gpos >= 0 ? (1ull << (gpos & 63)) : 0ull;
    while (w >= 0 && w < G.WORDS) {
        const BmWord u = L[w];
        uint64_t s = u.stop;
        if (w == gw) s |= gbit;
        s &= m;
        if (s) {
            const int bit = sgn > 0 ? __builtin_ctzll(s) : 63 - __builtin_clzll(s);
            *rp = w * 64 + bit;
            return !((u.occ >> bit) & 1ull);
        }
        w += sgn;
        m = ~0ull;
    }
    *rp = -1;
    return false;  // unreachable: the border always stops the ray
}

// jump(c, d) for a straight d from padded cell (px,py): scan from the neighbour cell (jps1.py:97-103).
__device__ __forceinline__ bool scan_ray(const GridDev& G, int px, int py, int dx, int dy, int gpx, int gpy, int* rp) {
    if (dx != 0) return scan_line(G, dx > 0 ? 0 : 1, py, px + dx, py == gpy ? gpx : -1, rp);
    return scan_line(G, dy > 0 ? 2 : 3, px, py + dy, px == gpx ? gpy : -1, rp);
}

// The two straight sub-jumps of a diagonal step (jps1.py:116-117) from cell (ox,oy): is either one not None?
__device__ __forceinline__ bool scan_two(const GridDev& G, int ox, int oy, int dx, int dy, int gpx, int gpy) {
    int rp;
    return scan_ray(G, ox, oy, dx, 0, gpx, gpy, &rp) || scan_ray(G, ox, oy, 0, dy, gpx, gpy, &rp);
}

// ---- jump-distance records: constants and accessors shared by the map build (fxjps_maps.hip.inc) and the search
constexpr uint32_t JD_K = 0x1FFFu, JD_J = 0x8000u;
__host__ __device__ constexpr int jd_slot(int code) { return code - (code >= 3 ? 1 : 0) - (code >= 5 ? 1 : 0) - (code >= 7 ? 1 : 0); }  // direction code (dx+1)*4+(dy+1) -> 0 .. 7
__host__ __device__ constexpr int jd_code(int slot) { return slot + (slot >= 3 ? 1 : 0) + (slot >= 4 ? 1 : 0) + (slot >= 5 ? 1 : 0); }
// the neighbour byte out of a record (x, y: its first two dwords)
__device__ __forceinline__ uint32_t jd_nb8(uint32_t x, uint32_t y) {
    return ((x >> 13) & 3u) | (((x >> 29) & 3u) << 2) | (((y >> 13) & 3u) << 4) | (((y >> 29) & 3u) << 6);
}
// entry `slot` of a record
__device__ __forceinline__ uint32_t jd_pick(uint32_t r0, uint32_t r1, uint32_t r2, uint32_t r3, uint32_t slot) {
    const uint32_t w = slot < 4u ? (slot < 2u ? r0 : r1) : (slot < 6u ? r2 : r3);
    return (w >> ((slot & 1u) * 16u)) & 0xFFFFu;
}

// ---------------------------------------------------------------- the search
// Wave-uniform values are forced into SGPRs with readfirstlane: control flow
// that depends on them is then a scalar branch, the whole wavefront takes it
// together, and every cross-lane operation runs with all 64 lanes enabled.
// A wave-uniform value that is deliberately kept in a vector register: loop-carried counters that are only added to
// (and compared once per iteration) cost one VALU instruction there; in scalar registers -- the kernel runs at the
// SGPR limit -- each of them was spilled and went through v_readlane / s_add / v_writelane every iteration.
__device__ __forceinline__ uint32_t vheld(uint32_t v) {
    asm volatile("" : "+v"(v));
    return v;
}
__device__ __forceinline__ uint32_t rfl(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }
__device__ __forceinline__ int rfli(int v) { return __builtin_amdgcn_readfirstlane(v); }
__device__ __forceinline__ uint64_t rfl64(uint64_t v) {
    return ((uint64_t)rfl((uint32_t)(v >> 32)) << 32) | (uint64_t)rfl((uint32_t)v);
}
__device__ __forceinline__ double rfld(double v) {
    return __longlong_as_double((long long)rfl64((uint64_t)__double_as_longlong(v)));
}
__device__ __forceinline__ TEnt uniform_ent(const TEnt& e) {  // every lane holds the same entry
    TEnt r;
    r.g = rfld(e.g);
    r.key = rfl(e.key);
    r.par = rfl(e.par);
    return r;
}

// ---- wavefront-wide minimum with DPP row operations (no LDS crossbar traffic): after the six
// steps lane 63 holds the minimum of all 64 lanes.  Out-of-row / masked lanes fall back to their
// own value (old == src), which is the identity for min.
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ uint32_t min_step32(uint32_t v) {
    // old = ~0 is the identity of umin, which lets the compiler fold the move into v_min_u32_dpp
    const uint32_t o = (uint32_t)__builtin_amdgcn_update_dpp(-1, (int)v, CTRL, ROW_MASK, 0xF, false);
    return min(o, v);
}
__device__ __forceinline__ uint32_t wave_umin32(uint32_t v) {
    v = min_step32<0x111, 0xF>(v);  // row_shr:1
    v = min_step32<0x112, 0xF>(v);  // row_shr:2
    v = min_step32<0x114, 0xF>(v);  // row_shr:4
    v = min_step32<0x118, 0xF>(v);  // row_shr:8
    v = min_step32<0x142, 0xA>(v);  // row_bcast:15 into rows 1 and 3
    v = min_step32<0x143, 0xC>(v);  // row_bcast:31 into rows 2 and 3
    return (uint32_t)__builtin_amdgcn_readlane((int)v, 63);
}
__device__ __forceinline__ uint64_t wave_umin64(uint64_t v) {
    // lexicographic (hi, lo): two 32-bit passes, each six v_min_u32_dpp
    const uint32_t hi = (uint32_t)(v >> 32), lo = (uint32_t)v;
    const uint32_t mh = wave_umin32(hi);
    const uint32_t ml = wave_umin32(hi == mh ? lo : ~0u);
    return ((uint64_t)mh << 32) | (uint64_t)ml;
}

constexpr uint64_t F_INF = 0x7FF0000000000000ull;

// Rank of this lane's key among the 64 keys of the wavefront: the number of lanes holding a smaller key (equal keys
// share a rank).  All 63 comparisons are independent -- rotations inside the 16-lane rows (DPP) of the key and of
// the three other rows brought to this lane's position (v_permlane16/32_swap).  Each comparison is a subtract whose
// borrow feeds an add-with-carry.
#define FX_RANK_STEP(acc, val, ror)                                                                         \
    asm("v_sub_co_u32_dpp %1, vcc, %2, %3 row_ror:" #ror " row_mask:0xf bank_mask:0xf\n\tv_addc_co_u32 %0, vcc, 0, %0, vcc" \
        : "+v"(acc), "=&v"(scratch)                                                                          \
        : "v"(val), "v"(key)                                                                                  \
        : "vcc")
#define FX_RANK_ROW(acc, val)                                                                                   \
    FX_RANK_STEP(acc, val, 1); FX_RANK_STEP(acc, val, 2); FX_RANK_STEP(acc, val, 3); FX_RANK_STEP(acc, val, 4);   \
    FX_RANK_STEP(acc, val, 5); FX_RANK_STEP(acc, val, 6); FX_RANK_STEP(acc, val, 7); FX_RANK_STEP(acc, val, 8);   \
    FX_RANK_STEP(acc, val, 9); FX_RANK_STEP(acc, val, 10); FX_RANK_STEP(acc, val, 11); FX_RANK_STEP(acc, val, 12); \
    FX_RANK_STEP(acc, val, 13); FX_RANK_STEP(acc, val, 14); FX_RANK_STEP(acc, val, 15)
__device__ __forceinline__ uint32_t wave_rank64(uint32_t key, int lane) {
    // the key of lane ^ 16, lane ^ 32, lane ^ 48
    const auto s16 = __builtin_amdgcn_permlane16_swap(key, key, false, false);
    const uint32_t o16 = (lane & 16) ? s16[0] : s16[1];
    const auto s32 = __builtin_amdgcn_permlane32_swap(key, key, false, false);
    const uint32_t o32 = (lane & 32) ? s32[0] : s32[1];
    const auto s48 = __builtin_amdgcn_permlane32_swap(o16, o16, false, false);
    const uint32_t o48 = (lane & 32) ? s48[0] : s48[1];
    uint32_t c0 = 0, c1 = (o16 < key) ? 1u : 0u, c2 = (o32 < key) ? 1u : 0u, c3 = (o48 < key) ? 1u : 0u, scratch;
    FX_RANK_ROW(c0, key);
    FX_RANK_ROW(c1, o16);
    FX_RANK_ROW(c2, o32);
    FX_RANK_ROW(c3, o48);
    return (c0 + c1) + (c2 + c3);
}

// The same for the full 96-bit open-list key (f as raw bits : packed x, y, direction): the three-dword subtraction
// other - mine through the borrow chain (v_sub_co / v_subb_co / v_subb_co, the other lane's dwords arriving by DPP),
// whose final borrow -- "the other key is smaller" -- feeds an add-with-carry.  Exact for every pair of keys, so a
// refill needs no quantised pre-sort and no fallback unless two entries carry the very same key.
#define FX_RANK3_STEP(acc, ox, olo, ohi, ror)                                                                          \
    asm("v_sub_co_u32_dpp %1, vcc, %2, %5 row_ror:" #ror " row_mask:0xf bank_mask:0xf\n\t"                               \
        "v_subb_co_u32_dpp %1, vcc, %3, %6, vcc row_ror:" #ror " row_mask:0xf bank_mask:0xf\n\t"                         \
        "v_subb_co_u32_dpp %1, vcc, %4, %7, vcc row_ror:" #ror " row_mask:0xf bank_mask:0xf\n\t"                         \
        "v_addc_co_u32 %0, vcc, 0, %0, vcc"                                                                             \
        : "+v"(acc), "=&v"(scratch)                                                                                     \
        : "v"(ox), "v"(olo), "v"(ohi), "v"(kx), "v"(klo), "v"(khi)                                                      \
        : "vcc")
#define FX_RANK3_ROW(acc, ox, olo, ohi)                                                                                  \
    FX_RANK3_STEP(acc, ox, olo, ohi, 1); FX_RANK3_STEP(acc, ox, olo, ohi, 2); FX_RANK3_STEP(acc, ox, olo, ohi, 3);       \
    FX_RANK3_STEP(acc, ox, olo, ohi, 4); FX_RANK3_STEP(acc, ox, olo, ohi, 5); FX_RANK3_STEP(acc, ox, olo, ohi, 6);       \
    FX_RANK3_STEP(acc, ox, olo, ohi, 7); FX_RANK3_STEP(acc, ox, olo, ohi, 8); FX_RANK3_STEP(acc, ox, olo, ohi, 9);       \
    FX_RANK3_STEP(acc, ox, olo, ohi, 10); FX_RANK3_STEP(acc, ox, olo, ohi, 11); FX_RANK3_STEP(acc, ox, olo, ohi, 12);    \
    FX_RANK3_STEP(acc, ox, olo, ohi, 13); FX_RANK3_STEP(acc, ox, olo, ohi, 14); FX_RANK3_STEP(acc, ox, olo, ohi, 15)
__device__ __forceinline__ uint32_t lane_xor16(uint32_t v, int lane) {
    const auto s = __builtin_amdgcn_permlane16_swap(v, v, false, false);
    return (lane & 16) ? s[0] : s[1];
}
__device__ __forceinline__ uint32_t lane_xor32(uint32_t v, int lane) {
    const auto s = __builtin_amdgcn_permlane32_swap(v, v, false, false);
    return (lane & 32) ? s[0] : s[1];
}
__device__ __forceinline__ uint32_t wave_rank96(uint32_t khi, uint32_t klo, uint32_t kx, int lane) {
    // the key of lane ^ 16, lane ^ 32, lane ^ 48
    const uint32_t x16 = lane_xor16(kx, lane), l16 = lane_xor16(klo, lane), h16 = lane_xor16(khi, lane);
    const uint32_t x32 = lane_xor32(kx, lane), l32 = lane_xor32(klo, lane), h32 = lane_xor32(khi, lane);
    const uint32_t x48 = lane_xor32(x16, lane), l48 = lane_xor32(l16, lane), h48 = lane_xor32(h16, lane);
    const auto lt = [&](uint32_t oh, uint32_t ol, uint32_t ox) -> uint32_t {
        const uint64_t of = ((uint64_t)oh << 32) | ol, kf = ((uint64_t)khi << 32) | klo;
        return (of < kf || (of == kf && ox < kx)) ? 1u : 0u;
    };
    uint32_t c0 = 0, c1 = lt(h16, l16, x16), c2 = lt(h32, l32, x32), c3 = lt(h48, l48, x48), scratch;
    FX_RANK3_ROW(c0, kx, klo, khi);
    FX_RANK3_ROW(c1, x16, l16, h16);
    FX_RANK3_ROW(c2, x32, l32, h32);
    FX_RANK3_ROW(c3, x48, l48, h48);
    return (c0 + c1) + (c2 + c3);
}

#ifdef FXJPS_PROF
// diagnostic build: shader-clock cycles per phase of the expansion loop, summed over wavefronts into
// out_counters[8 + phase] (never quote this build's run time)
#define PF_DECL unsigned long long pf_t = __builtin_readcyclecounter(), pf_acc[16] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0}
#define PF_PARAMS , unsigned long long &pf_t, unsigned long long *pf_acc
#define PF_ARGS , pf_t, pf_acc
#define PF(k)                                                         \
    do {                                                              \
        const unsigned long long pf_n = __builtin_readcyclecounter(); \
        pf_acc[k] += pf_n - pf_t;                                     \
        pf_t = pf_n;                                                  \
    } while (0)
#define PF_FLUSH                                                                  \
    do {                                                                          \
        if (cnt4 && (threadIdx.x & 63) == 0)                                       \
            for (int k_ = 0; k_ < 16; k_++) atomicAdd(&cnt4[k_ < 12 ? 8 + k_ : 48 + k_], pf_acc[k_]); \
    } while (0)
#elif defined(FXJPS_PHASE_S)
// one-interval build (-DFXJPS_PHASE_S=a -DFXJPS_PHASE_E=b): the cycles between mark a and the next mark b, summed into
// out_counters[8]; two clock reads per loop iteration instead of sixteen (each costs the wavefront ~ 200 cycles: the
// sixteen of the FXJPS_PROF build distort what they measure by 40 %).  tools/phase_times.sh builds and runs one per interval.
#define PF_DECL unsigned long long pf_t = 0, pf_sum = 0; uint32_t pf_on = 0u
#define PF_PARAMS , unsigned long long &pf_t, unsigned long long &pf_sum, uint32_t &pf_on
#define PF_ARGS , pf_t, pf_sum, pf_on
#define PF(k)                                                              \
    do {                                                                   \
        if ((k) == FXJPS_PHASE_S) {                                        \
            pf_t = __builtin_readcyclecounter();                           \
            pf_on = 1u;                                                    \
        } else if ((k) == FXJPS_PHASE_E && pf_on != 0u) {                  \
            pf_sum += __builtin_readcyclecounter() - pf_t;                 \
            pf_on = 0u;                                                    \
        }                                                                  \
    } while (0)
#define PF_FLUSH                                                           \
    do {                                                                   \
        if (cnt4 && (threadIdx.x & 63) == 0) atomicAdd(&cnt4[8], pf_sum);  \
    } while (0)
#else
#define PF_DECL
#define PF_PARAMS
#define PF_ARGS
#ifdef FXJPS_MARK  // analysis build: phase boundaries as comments in the assembly (tools/hot_loop.py)
#define PF(k) asm volatile("; FXMARK " #k)
#else
#define PF(k) \
    do {      \
    } while (0)
#endif
#define PF_FLUSH \
    do {         \
    } while (0)
#endif

// ---------------------------------------------------------------- open list
// Three tiers, ordered by the full key (f bits, x:13|y:13|dir:4):
//   R    registers, one entry per lane (64 per wavefront): popped with one DPP minimum, no bookkeeping
//   M    LDS, unsorted, MCAP entries: absorbs what does not fit R, feeds R when it runs dry
//   far  global memory, unsorted: everything else, touched only by refills, splits and far pushes; in two bands
//        (near: keys below (T2hi << 32, 0), what the next handful of refills will take; far: the rest), so that a refill
//        scans and rewrites the near band only -- the far band is gone through once per re-banding
// Invariant:   every R key  <  (Rbits, Rx)  <=  every M key  <  (Tbits, Tx)  <=  every far key,
//              every near-band key  <  (T2hi << 32, 0)  <=  every far-band key
// so the (f, x, y) minimum of jps1.py:198 is always in R while R is non-empty, and the pop order is exact.
struct OpenList {  // per-wavefront open-list state, all wave-uniform
    int r_n;         // entries in R
    uint32_t m_n;    // entries in M
    uint32_t far_n;  // entries in the near band of the far tier: far[0 .. far_n)
    uint32_t farb_n; // entries in its far band: far[far_cap / 2 .. far_cap / 2 + farb_n)
    uint32_t T2hi;   // band threshold: the high word of an f (low word and (x, y) part 0): near band < (T2hi << 32, 0) <= far band
    uint64_t Rbits;  // R / M threshold key, f part
    uint32_t Rx;     //                      packed (x, y, direction) part
    uint64_t Tbits;  // M / far threshold key
    uint32_t Tx;
    uint32_t dxs;    // > 0: the last far refill had to split one f level on (x, y); width of the slice it took
    double delta;    // width of the f band a far refill aims at
    uint32_t hshift; // bands of the far band: region k < NBANDS - 1 holds the high words [b0 + (k << hshift), b0 + (k + 1 << hshift)),
                     //                the last region everything above; b0 = T2hi - (cur0 << hshift)
    uint32_t cur0;   //                first band that has not been used up (T2hi is its lower bound)
    uint32_t fail;   // a region of the ring overflowed: the query is re-run on the large pool
    uint32_t banded; // the far band is kept in bands (SearchArgs::banded)
};

// Fence after a lane-dependent `if` / loop: the lanes provably reconverge here.  Without it the compiler threads
// the jump past the join into whatever follows (a loop back-edge, a return), and its divergence analysis then
// treats every wave-uniform value merged there as lane-dependent (VGPRs and exec-mask loops instead of SGPRs).
#define RECONV() __builtin_amdgcn_wave_barrier()

// Which lane touches which cell of a query's path slot: cell k belongs to lane k % WAVE.  search_one stores the slot by this
// rule and store_result reads it back by it with no fence between the two -- a lane only ever reads what it stored itself.
template <typename F>
__device__ __forceinline__ void for_path_cells(int lane, uint32_t n, F&& f) {
    for (uint32_t k = (uint32_t)lane; k < n; k += WAVE) f(k);
}

// The open-list state is wave-uniform by construction.  Saying so (readfirstlane folds away for values already
// in SGPRs) stops the compiler's divergence analysis from dragging it through joins of lane-dependent branches.
__device__ __forceinline__ void open_uniform(OpenList& Q) {
    Q.r_n = rfli(Q.r_n);
    Q.m_n = rfl(Q.m_n);
    Q.far_n = rfl(Q.far_n);
    Q.farb_n = rfl(Q.farb_n);
    Q.T2hi = rfl(Q.T2hi);
    Q.Rbits = rfl64(Q.Rbits);
    Q.Rx = rfl(Q.Rx);
    Q.Tbits = rfl64(Q.Tbits);
    Q.Tx = rfl(Q.Tx);
    Q.dxs = rfl(Q.dxs);
    Q.delta = rfld(Q.delta);
    Q.hshift = rfl(Q.hshift);
    Q.cur0 = rfl(Q.cur0);
    Q.fail = rfl(Q.fail);
    Q.banded = rfl(Q.banded);
}

struct RTier {   // this lane's entry of R; empty: f == ~0, x == ~0
    uint64_t f;  // f as raw bits
    uint32_t x;  // x:13 | y:13 | pd:4
    uint32_t s;  // table slot of the node
    uint32_t c;  // cell info of the node (GridDev::ci)
};

#ifndef FXJPS_FPD
#define FXJPS_FPD 1
#endif
constexpr int FPD = FXJPS_FPD;     // 64-entry chunks of the far tier kept in flight by a refill scan
#ifndef FXJPS_FBANDS
#define FXJPS_FBANDS 10
#endif
constexpr int FBANDS = FXJPS_FBANDS;  // refill widths of f the near band of the far tier spans after a re-banding
#ifndef FXJPS_RFILL
#define FXJPS_RFILL 0.75
#endif
#ifndef FXJPS_RLOW
#define FXJPS_RLOW 1
#endif
constexpr int RLOW = FXJPS_RLOW;   // R is refilled from M when it holds fewer entries than this
#ifndef FXJPS_MCAP
#define FXJPS_MCAP 256
#endif
constexpr int MCAP = FXJPS_MCAP;   // M entries per wavefront
#ifndef FXJPS_BANDED
#define FXJPS_BANDED 1
#endif
// Far band as a ring of f bands (Euclidean keys, k_search<2, ..>): the upper half of a wavefront's far array is NBANDS
// regions of equal size, one per band of (1 << hshift) high words of f -- half a refill width -- counted in LDS.  A
// push beyond the near band goes straight to the region of its band (slot from an LDS atomic), and a refill that finds
// the near band empty takes the next bands WHOLE into M: nothing is scanned for a threshold, nothing is compacted or
// rewritten.  The last region holds everything above the bands and is dealt out over a new set of bands once they are
// used up.
constexpr int NBANDS = 64;              // NBANDS - 1 bands + the region of everything above them
constexpr uint32_t BAND_MIN_CAP = 128;  // the bands are used only when a region holds at least this many entries
#ifndef FXJPS_BAND_FRAC
#define FXJPS_BAND_FRAC 0.25  // width of a band as a fraction of the width of f a refill aims at
#endif
// The upper half of the far array: NBANDS - 1 band regions in its first three quarters, the last region in the fourth.
__device__ __forceinline__ uint32_t band_cap(uint32_t half, uint32_t k) {
    return k == (uint32_t)NBANDS - 1u ? (half >> 2) : (half - (half >> 2)) / ((uint32_t)NBANDS - 1u);
}
__device__ __forceinline__ size_t band_base(uint32_t half, uint32_t k) {
    return k == (uint32_t)NBANDS - 1u ? (size_t)half + (size_t)(half - (half >> 2))
                                      : (size_t)half + (size_t)k * (size_t)((half - (half >> 2)) / ((uint32_t)NBANDS - 1u));
}
constexpr int MSLOT = MCAP / WAVE; // M entries a lane looks at when the whole tier is scanned
#ifndef FXJPS_HZ_LOG2
#define FXJPS_HZ_LOG2 9
#endif
#ifndef FXJPS_HZ_LOG2_DIRECT
#define FXJPS_HZ_LOG2_DIRECT 10
#endif
// Cells of the slot-collision detector (WaveLds::hz), a property of the instantiation: the untracked searches on
// cell-indexed tables carry no slot payload in LDS (see SLOTLESS below) and spend what that frees on a detector of twice
// the size; everywhere else -- the tracking instantiations hold 8 KB of read-set rows per block, the hashed ones keep s[] --
// it is FXJPS_HZ_LOG2.
constexpr int HZ_LOG2 = FXJPS_HZ_LOG2, HZ_LOG2_DIRECT = FXJPS_HZ_LOG2_DIRECT;
static_assert(HZ_LOG2 >= 7 && HZ_LOG2 <= 12 && HZ_LOG2_DIRECT >= 7 && HZ_LOG2_DIRECT <= 12, "detector sizes the hashes and the LDS budget were written for");

// Pointers into LDS carry their address space: through a generic pointer every access becomes a flat_load /
// flat_store (texture-path latency, and a wait on every outstanding global store) instead of ds_read / ds_write.
#define LDS_PTR(T) __attribute__((address_space(3))) T*

// The layout of the open list is a property of the instantiation.  On a table indexed by the cell a node's slot is a
// function of its cell (slot = x << direct_ly | y), so an open-list entry need not carry it: the SLOTLESS layout has no
// slot in R (RTier::s is never touched and takes no register), none in M, and the fourth dword of a far entry holds the
// entry's cell info instead (nothing is kept in the u16 array behind the entries).  The slot is derived where it is first
// needed, at the lane deal.  The carrying layout is the one of the hashed tables, of the tracking searches and of
// k_selftest_openlist (whose payloads are arbitrary numbers).
template <bool NOSLOT, int HZL>
struct WaveLdsT;
template <int HZL>
struct WaveLdsT<false, HZL> {  // LDS of one wavefront.  One base pointer: every array below is an immediate offset of the ds_* instruction
    static constexpr bool SLOTLESS = false;
    static constexpr int HZ_LOG2 = HZL, HZ_SIZE = 1 << HZL;
    unsigned long long f[MCAP];  // M tier: keys (f as raw bits)
    uint32_t x[MCAP];            //         packed (x, y, direction)
    uint32_t s[MCAP];            //         table slot
    uint16_t c[MCAP];            //         cell info
    uint16_t idx[WAVE];          // M indices on their way into R
    uint32_t hz[HZ_SIZE];        // HZ_SIZE cells (all ones at rest): slot-collision detector of the vectorised commit
    uint32_t bcnt[NBANDS];       // entries in each region of the far band's ring (k_search<2, ..>)
};
template <int HZL>
struct WaveLdsT<true, HZL> {  // the same without the slots
    static constexpr bool SLOTLESS = true;
    static constexpr int HZ_LOG2 = HZL, HZ_SIZE = 1 << HZL;
    unsigned long long f[MCAP];
    uint32_t x[MCAP];
    uint16_t c[MCAP];
    uint16_t idx[WAVE];
    uint32_t hz[HZ_SIZE];
    uint32_t bcnt[NBANDS];
};
using WaveLds = WaveLdsT<false, HZ_LOG2>;  // the carrying layout
// what k_search<HC, TRK, DIRECT, MG> runs on
template <bool TRK, bool DIRECT>
using SearchLds = WaveLdsT<DIRECT && !TRK, (DIRECT && !TRK) ? HZ_LOG2_DIRECT : HZ_LOG2>;
template <class WL>
struct MidT {
    static constexpr bool SLOTLESS = WL::SLOTLESS;
    static constexpr int HZ_LOG2 = WL::HZ_LOG2, HZ_SIZE = WL::HZ_SIZE;
    LDS_PTR(WL) w;
    LDS_PTR(const uint32_t) dirlut;  // block-wide LDS copy of c_dirlut
    LDS_PTR(unsigned long long) bx;  // read set (k_search<HC, true> only), see ReadSet: [64] rows = y tiles, bits = x tiles;
                                     // followed by by[64]: rows = x tiles, bits = y tiles
#ifdef FXJPS_PROF
    unsigned long long* dbg;      // diagnostic build: out_counters
#endif
};
using Mid = MidT<WaveLds>;
#if defined(FXJPS_PROF) && !defined(FXJPS_PROF_LIGHT)  // (FXJPS_PROF_LIGHT: the cycle counters per phase alone, without the event counters' atomics inside the phases)
// (v is evaluated by the whole wavefront, in front of the branch that leaves lane 0 alone: a __ballot in it would see lane 0 only)
#define DBG_COUNT(M, k, v)                                                     \
    do {                                                                       \
        const unsigned long long dbg_v_ = (unsigned long long)(v);             \
        if ((M).dbg && (threadIdx.x & 63) == 0) atomicAdd(&(M).dbg[k], dbg_v_); \
    } while (0)
#else
#define DBG_COUNT(M, k, v) \
    do {                   \
    } while (0)
#endif

// ---- read set of a search (streaming replan, fxjps_replan_frame).  The grid is covered by at most 64 x 64 tiles of
// (1 << tsh)^2 cells.  A search marks every tile holding a cell whose derived data (scan bits, cell info) it read:
// the cells of a straight scan from its first cell to the cell that ended it, the cells a diagonal ray stepped on
// plus -- through the reach classes in bits 12-15 of their cell info -- the tiles their precomputed sub-jumps scanned,
// the start and the goal.  Derived data of a cell depends on the occupancy within Chebyshev distance 1 of it, so a
// later change of the grid can alter the search only if a changed cell, or one of its 8 neighbours, lies in a marked
// tile; otherwise a from-scratch search would read the same bits, take the same decisions and return the same path.
// Two bitmaps, so that a span along either axis is one 64-bit mask: bx[y tile] has a bit per x tile, by[x tile] a
// bit per y tile.
__device__ __forceinline__ int rs_tile(int padded, int tsh) { return min(max((padded - 1) >> tsh, 0), 63); }
__device__ __forceinline__ unsigned long long rs_span(int ta, int tb) {  // bits ta .. tb (ta <= tb)
    return (~0ull >> (63 - tb)) & (~0ull << ta);
}
__device__ __forceinline__ void rs_or(LDS_PTR(unsigned long long) row, unsigned long long m) {
    __hip_atomic_fetch_or(row, m, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
}
// cells a .. b (padded positions, either order) of scan line `line`; alongY: the line is a padded x, positions are y
template <class MID>
__device__ __forceinline__ void rs_mark_scan(const MID& S, int tsh, bool alongY, int line, int a, int b) {
    const int tl = rs_tile(line, tsh), ta = rs_tile(min(a, b), tsh), tb = rs_tile(max(a, b), tsh);
    rs_or(alongY ? S.bx + 64 + tl : S.bx + tl, rs_span(ta, tb));
}
// a cell whose cell info `m` was read: its own tile, and the tiles its straight sub-jumps reach
template <class MID>
__device__ __forceinline__ void rs_mark_cell(const MID& S, int tsh, int px, int py, uint32_t m) {
    const int tx = rs_tile(px, tsh), ty = rs_tile(py, tsh);
    const int cx = (int)((m >> 12) & 3u), cy = (int)((m >> 14) & 3u);
    rs_or(S.bx + ty, cx == 3 ? ~0ull : rs_span(max(tx - cx, 0), min(tx + cx, 63)));
    rs_or(S.bx + 64 + tx, cy == 3 ? ~0ull : rs_span(max(ty - cy, 0), min(ty + cy, 63)));
}

// number of set bits of `m` below this lane
__device__ __forceinline__ uint32_t rank_below(uint64_t m) {
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
}

__device__ __forceinline__ bool key_lt(uint64_t f, uint32_t x, uint64_t Tf, uint32_t Tx) {
    return f < Tf || (f == Tf && x < Tx);
}

// The cell info of far entry i lives in a u16 array right behind the far_cap entries of the wavefront.
__device__ __forceinline__ uint16_t* far_ci(FarEnt* far, uint32_t far_cap) { return reinterpret_cast<uint16_t*>(far + far_cap); }

__device__ __forceinline__ uint32_t lane_get(uint32_t v, int i) { return (uint32_t)__builtin_amdgcn_readlane((int)v, i); }
__device__ __forceinline__ uint64_t lane_get64(uint64_t v, int i) {
    return ((uint64_t)lane_get((uint32_t)(v >> 32), i) << 32) | (uint64_t)lane_get((uint32_t)v, i);
}
__device__ __forceinline__ uint32_t lane_pull(uint32_t v, uint32_t src_lane) {  // v of lane src_lane (per lane)
    return (uint32_t)__builtin_amdgcn_ds_bpermute((int)(src_lane << 2), (int)v);
}

// The midpoint of a key range [(lo), (hi)] as a threshold that keeps the minimum and releases the maximum:
// in f when the f values differ, else in (x, y) (one f level: the normal case with the octile heuristic).
__device__ __forceinline__ void key_midpoint(uint64_t lo, uint64_t hi, uint32_t xmn, uint32_t xmx, uint64_t* Pf, uint32_t* Px) {
    const double dlo = __longlong_as_double((long long)lo), dhi = __longlong_as_double((long long)hi);
    const double mid = dlo + (dhi - dlo) * 0.5;
    *Pf = hi;
    *Px = 0;
    if (mid > dlo) {
        *Pf = (uint64_t)__double_as_longlong(mid);
    } else if (hi == lo) {
        *Px = xmn + (xmx - xmn + 1u) / 2u;  // > xmn unless all keys are equal, <= xmx
    }
}

// Append the entries held by the lanes of `out` (key (kf, kx), payload ks, kc) to the far tier: to the near band when
// below the band threshold, else to the far band.  The bands are the two halves of the wavefront's far array.
// NOSLOT (the slotless layout): the entry is {f, xyd, cell info}, one 16-byte store; ks and fci are not used.
template <bool NOSLOT>
__device__ __forceinline__ bool far_append(OpenList& Q, FarEnt* __restrict__ far, uint16_t* __restrict__ fci, uint32_t half, bool check,
                                           bool out, uint64_t kf, uint32_t kx, uint32_t ks, uint32_t kc) {
    const uint64_t om = __ballot(out);
    const uint64_t bm = __ballot(out && (uint32_t)(kf >> 32) >= Q.T2hi);
    const uint64_t am = om & ~bm;
    const uint32_t na = (uint32_t)__popcll(am), nb = (uint32_t)__popcll(bm);
    if (check && (Q.far_n + na > half || Q.farb_n + nb > half)) return false;
    if (out) {
        FarEnt e;
        e.fbits = kf;
        e.xyd = kx;
        e.slot = NOSLOT ? kc : ks;
        const bool toB = (uint32_t)(kf >> 32) >= Q.T2hi;
        const uint32_t j = (toB ? half + Q.farb_n : Q.far_n) + rank_below(toB ? bm : am);
        far[j] = e;
        if (!NOSLOT) fci[j] = (uint16_t)kc;
    }
    RECONV();
    Q.far_n += na;
    Q.farb_n += nb;
    return true;
}

// ---- the ring of bands (see NBANDS)
constexpr uint32_t INF_HI = (uint32_t)(0x7FF0000000000000ull >> 32);  // T2hi of a wavefront without a ring
// Width of a band, in high words of the double as a power of two (rounded down: narrower rather than wider): a quarter
// of the width of f a refill aims at (delta follows what the refills get), and no more than a sixteenth of the span
// lo .. hi of the entries that are about to be dealt out.
__device__ __forceinline__ uint32_t band_shift(uint32_t lo, uint32_t hi, double delta) {
    const double tf = __longlong_as_double((long long)((uint64_t)lo << 32));
    const uint32_t wd = (uint32_t)((uint64_t)__double_as_longlong(tf + FXJPS_BAND_FRAC * delta) >> 32) - lo;
    const uint32_t w = max(min(wd, (hi - lo) / 16u + 1u), 1u);
    const uint32_t s = 31u - (uint32_t)__builtin_clz(w);
    return s > 20u ? 20u : s;
}
// The entry held by the lanes of `on` goes to the region of its band (its key is at or above the start of the ring).
// Returns the lanes whose region is full.
template <class MID>
__device__ __forceinline__ uint64_t ring_put(const OpenList& Q, const MID& M, FarEnt* __restrict__ far, uint32_t far_cap, bool on,
                                             uint64_t kf, uint32_t kx, uint32_t ks) {
    const uint32_t half = far_cap >> 1;
    const uint32_t phys = min(Q.cur0 + (((uint32_t)(kf >> 32) - Q.T2hi) >> Q.hshift), (uint32_t)NBANDS - 1u);
    const uint32_t bcap = band_cap(half, phys);
    uint32_t pos = 0;
    if (on) pos = __hip_atomic_fetch_add(&M.w->bcnt[phys], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
    RECONV();
    const bool ok = on && pos < bcap;
    if (ok) {  // (the cell info is read from the map again when the entry comes back)
        FarEnt e;
        e.fbits = kf;
        e.xyd = kx;
        e.slot = ks;
        far[band_base(half, phys) + pos] = e;
    }
    RECONV();
    return __ballot(on && !ok);
}
// Pushes that go to the far tier: below the start of the ring to the near band (appended at their rank, as ever), the
// others to the ring.
template <bool BANDED, class MID>  // (the ring carries slots: it serves the hashed tables only)
__device__ __forceinline__ bool far_push(OpenList& Q, const MID& M, FarEnt* __restrict__ far, uint16_t* __restrict__ fci, uint32_t far_cap,
                                         bool out, uint64_t kf, uint32_t kx, uint32_t ks, uint32_t kc) {
    static_assert(!(BANDED && MID::SLOTLESS), "the ring of bands keeps the carrying layout");
    if (!BANDED || !Q.banded) return far_append<MID::SLOTLESS>(Q, far, fci, far_cap >> 1, true, out, kf, kx, ks, kc);
    const bool toB = out && (uint32_t)(kf >> 32) >= Q.T2hi;
    const uint64_t bm = __ballot(toB);
    if (__ballot(out && !toB) != 0ull && !far_append<MID::SLOTLESS>(Q, far, fci, far_cap >> 1, true, out && !toB, kf, kx, ks, kc)) return false;
    if (bm != 0ull) {
        if (ring_put(Q, M, far, far_cap, toB, kf, kx, ks) != 0ull) return false;
        Q.farb_n += (uint32_t)__popcll(bm);
    }
    return true;
}

// Move the M entries with key >= P to the far tier, close the gaps, and make P the M / far threshold.
template <class MID>
__device__ __forceinline__ bool m_evict(OpenList& Q, const MID& M, FarEnt* __restrict__ far, uint16_t* __restrict__ fci, int lane,
                                        uint64_t Pf, uint32_t Px, uint32_t far_cap, bool check = true) {
    open_uniform(Q);
    Pf = rfl64(Pf);
    Px = rfl(Px);
    const uint32_t n = Q.m_n;
    const uint32_t bhalf = far_cap >> 1;
    uint64_t f[MSLOT];
    uint32_t x[MSLOT];
    uint32_t na = 0, nb = 0;
#pragma unroll
    for (int k = 0; k < MSLOT; k++) {
        const uint32_t i = (uint32_t)lane + (uint32_t)(k * WAVE);
        f[k] = ~0ull;
        x[k] = ~0u;
        if (i < n) {
            f[k] = M.w->f[i];
            x[k] = M.w->x[i];
        }
        RECONV();
        const bool out = i < n && !key_lt(f[k], x[k], Pf, Px);
        const uint64_t om = __ballot(out), bm = __ballot(out && (uint32_t)(f[k] >> 32) >= Q.T2hi);
        na += (uint32_t)__popcll(om & ~bm);
        nb += (uint32_t)__popcll(bm);
    }
    if (check && (Q.far_n + na > bhalf || Q.farb_n + nb > bhalf)) return false;  // (!check: the entries came out of the far tier)
    uint32_t mw = 0;
#pragma unroll
    for (int k = 0; k < MSLOT; k++) {
        const uint32_t i = (uint32_t)lane + (uint32_t)(k * WAVE);
        const bool valid = i < n;
        const bool out = valid && !key_lt(f[k], x[k], Pf, Px);
        const bool keep = valid && !out;
        const uint64_t km = __ballot(keep);
        uint32_t es = 0, ec = 0;
        if (valid) {
            if constexpr (!MID::SLOTLESS) es = M.w->s[i];
            ec = M.w->c[i];
        }
        RECONV();
        (void)far_append<MID::SLOTLESS>(Q, far, fci, bhalf, false, out, f[k], x[k], es, ec);
        if (keep) {  // compaction moves entries down only, onto slots every lane has already read
            const uint32_t j = mw + rank_below(km);
            M.w->f[j] = f[k];
            M.w->x[j] = x[k];
            if constexpr (!MID::SLOTLESS) M.w->s[j] = es;
            M.w->c[j] = (uint16_t)ec;
        }
        RECONV();
        mw += (uint32_t)__popcll(km);
    }
    Q.m_n = mw;
    Q.Tbits = Pf;
    Q.Tx = Px;
    return true;
}

// M is full: release its upper half (by key range) to the far tier.
template <class MID>
__device__ __forceinline__ bool m_split(OpenList& Q, const MID& M, FarEnt* __restrict__ far, uint16_t* __restrict__ fci, int lane,
                                        uint32_t far_cap) {
    open_uniform(Q);
    const uint32_t n = Q.m_n;
    uint64_t lo = ~0ull, hi = 0ull;
    uint32_t xlo = ~0u, xhi = 0u;
#pragma unroll
    for (int k = 0; k < MSLOT; k++) {
        const uint32_t i = (uint32_t)lane + (uint32_t)(k * WAVE);
        if (i < n) {
            const uint64_t f = M.w->f[i];
            const uint32_t x = M.w->x[i];
            lo = f < lo ? f : lo;
            hi = f > hi ? f : hi;
            xlo = x < xlo ? x : xlo;
            xhi = x > xhi ? x : xhi;
        }
        RECONV();
    }
    lo = wave_umin64(lo);
    hi = ~wave_umin64(~hi);
    uint32_t xmn = 0, xmx = 0;
    if (hi == lo) {  // one f level: split on (x, y)
        xmn = wave_umin32(xlo);
        xmx = ~wave_umin32(~xhi);
    }
    uint64_t Pf;
    uint32_t Px;
    key_midpoint(lo, hi, xmn, xmx, &Pf, &Px);
    return m_evict(Q, M, far, fci, lane, Pf, Px, far_cap);
}

// R is full: its upper half (it is sorted: the lanes from r_n / 2 on) moves to M; the first key that leaves becomes
// the R / M threshold.
template <class MID>
__device__ __forceinline__ bool r_split(OpenList& Q, RTier& R, const MID& M, FarEnt* __restrict__ far, uint16_t* __restrict__ fci,
                                        int lane, uint32_t far_cap) {
    open_uniform(Q);
    const int keep = Q.r_n / 2;
    const uint32_t no = (uint32_t)(Q.r_n - keep);
    const uint64_t Pf = lane_get64(R.f, keep);
    const uint32_t Px = lane_get(R.x, keep);
    while (Q.m_n + no > (uint32_t)MCAP) {
        if (!m_split(Q, M, far, fci, lane, far_cap)) return false;
    }
    if (lane >= keep && lane < Q.r_n) {
        const uint32_t j = Q.m_n + (uint32_t)(lane - keep);
        M.w->f[j] = R.f;
        M.w->x[j] = R.x;
        if constexpr (!MID::SLOTLESS) M.w->s[j] = R.s;
        M.w->c[j] = (uint16_t)R.c;
        R.f = ~0ull;
        R.x = ~0u;
    }
    RECONV();
    Q.m_n += no;
    Q.r_n = keep;
    Q.Rbits = Pf;
    Q.Rx = Px;
    return true;
}

// ---- Sort the n entries in lanes 0 .. n-1 of R ascending by (f, x) (R is empty beyond them): a bitonic network (round 6).
// The rank sort it replaced (every lane ranked its 96-bit key among the others, wave_rank96) cost 63 three-dword comparisons
// per lane -- 252 vector instructions, 298 with the tie handling and the moves, once per ~ 5 iterations: 9 % of the vector
// instructions of a full chip's iteration (profiles/r06_phase_insts.txt).  A bitonic network in its "mirror" form (every
// block ascending: level k first pairs lane i with i ^ (2^k - 1), then i ^ 2^(j-1) for j = k-1 .. 1) needs 21
// compare-exchange stages of 8 vector instructions: the 96-bit subtraction partner - mine through the borrow chain
// (partner's dwords arriving by DPP), then five selects under its outcome (the entry travels with its key: nothing is
// permuted afterwards, equal keys cannot collide).  The lane with the lower number of a pair keeps the smaller key: it takes
// the partner's entry iff partner < mine, the upper lane iff partner > mine = not (partner <= mine) -- one borrow chain for
// both, the upper lanes enter it with a borrow of 1 (vcc preset to the mask of upper lanes), and
//     keep mine  =  borrow-out XNOR upper-mask.
// Partners beyond a DPP row operation's reach (i ^ 4, i ^ 16, i ^ 31, i ^ 63) come over the LDS crossbar (ds_swizzle /
// ds_bpermute: no vector-ALU issue).  Empty lanes hold the all-ones key and sort to the end; with n <= 32 (16) entries the
// last level (two levels) has nothing to do and is skipped.
// (s_xnor writes scc: it is in the clobber list -- without it the compiler kept the outcome of `n > 16` there, across the
// stages.)  (The masks are literals of the scalar instructions: as register operands the compiler hoists the six 64-bit constants out
// of the search loop and keeps them -- 12 scalar registers the kernel does not have -- in spill slots)
#define FX_BITONIC_DPP_(DPPSTR, ULO, UHI)                                                               \
    asm volatile("s_mov_b32 vcc_lo, " ULO "\n\ts_mov_b32 vcc_hi, " UHI "\n\t"                             \
                 "v_subb_co_u32_dpp %5, vcc, %2, %2, vcc " DPPSTR " row_mask:0xf bank_mask:0xf\n\t"      \
                 "v_subb_co_u32_dpp %5, vcc, %0, %0, vcc " DPPSTR " row_mask:0xf bank_mask:0xf\n\t"      \
                 "v_subb_co_u32_dpp %5, vcc, %1, %1, vcc " DPPSTR " row_mask:0xf bank_mask:0xf\n\t"      \
                 "s_xnor_b32 vcc_lo, vcc_lo, " ULO "\n\ts_xnor_b32 vcc_hi, vcc_hi, " UHI "\n\t"           \
                 "v_cndmask_b32_dpp %2, %2, %2, vcc " DPPSTR " row_mask:0xf bank_mask:0xf\n\t"           \
                 "v_cndmask_b32_dpp %0, %0, %0, vcc " DPPSTR " row_mask:0xf bank_mask:0xf\n\t"           \
                 "v_cndmask_b32_dpp %1, %1, %1, vcc " DPPSTR " row_mask:0xf bank_mask:0xf\n\t"           \
                 "v_cndmask_b32_dpp %3, %3, %3, vcc " DPPSTR " row_mask:0xf bank_mask:0xf\n\t"           \
                 "v_cndmask_b32_dpp %4, %4, %4, vcc " DPPSTR " row_mask:0xf bank_mask:0xf"                \
                 : "+v"(flo), "+v"(fhi), "+v"(kx), "+v"(ks), "+v"(kc), "=&v"(scr)                         \
                 :                                                                                        \
                 : "vcc", "scc")
// the same with the partner's entry already fetched (p*): plain VOP2
#define FX_BITONIC_XCH_(ULO, UHI)                                                                       \
    asm volatile("s_mov_b32 vcc_lo, " ULO "\n\ts_mov_b32 vcc_hi, " UHI "\n\t"                             \
                 "v_subb_co_u32 %5, vcc, %8, %2, vcc\n\t"                                                \
                 "v_subb_co_u32 %5, vcc, %6, %0, vcc\n\t"                                                \
                 "v_subb_co_u32 %5, vcc, %7, %1, vcc\n\t"                                                \
                 "s_xnor_b32 vcc_lo, vcc_lo, " ULO "\n\ts_xnor_b32 vcc_hi, vcc_hi, " UHI "\n\t"           \
                 "v_cndmask_b32 %2, %8, %2, vcc\n\t"                                                    \
                 "v_cndmask_b32 %0, %6, %0, vcc\n\t"                                                    \
                 "v_cndmask_b32 %1, %7, %1, vcc\n\t"                                                    \
                 "v_cndmask_b32 %3, %9, %3, vcc\n\t"                                                    \
                 "v_cndmask_b32 %4, %10, %4, vcc"                                                        \
                 : "+v"(flo), "+v"(fhi), "+v"(kx), "+v"(ks), "+v"(kc), "=&v"(scr)                         \
                 : "v"(pflo), "v"(pfhi), "v"(px), "v"(ps), "v"(pc)                                        \
                 : "vcc", "scc")
// partner = lane ^ xor-mask within each half of the wavefront (ds_swizzle, bit-mask mode: and 0x1f, or 0, xor m)
#define FX_BITONIC_SWZ_(M, ULO, UHI)                                                                    \
    do {                                                                                                \
        const uint32_t pflo = (uint32_t)__builtin_amdgcn_ds_swizzle((int)flo, 0x1F | ((M) << 10));      \
        const uint32_t pfhi = (uint32_t)__builtin_amdgcn_ds_swizzle((int)fhi, 0x1F | ((M) << 10));      \
        const uint32_t px = (uint32_t)__builtin_amdgcn_ds_swizzle((int)kx, 0x1F | ((M) << 10));         \
        const uint32_t ps = (uint32_t)__builtin_amdgcn_ds_swizzle((int)ks, 0x1F | ((M) << 10));         \
        const uint32_t pc = (uint32_t)__builtin_amdgcn_ds_swizzle((int)kc, 0x1F | ((M) << 10));         \
        FX_BITONIC_XCH_(ULO, UHI);                                                                      \
    } while (0)
// the lanes that hold the upper end of a pair: bit b of the lane number set (both halves of the 64-bit mask)
// (one more level of expansion: FX_Uk stands for two arguments)
#define FX_BITONIC_DPP(D, U) FX_BITONIC_DPP_(D, U)
#define FX_BITONIC_XCH(U) FX_BITONIC_XCH_(U)
#define FX_BITONIC_SWZ(M, U) FX_BITONIC_SWZ_(M, U)
#define FX_U0 "0xaaaaaaaa", "0xaaaaaaaa"
#define FX_U1 "0xcccccccc", "0xcccccccc"
#define FX_U2 "0xf0f0f0f0", "0xf0f0f0f0"
#define FX_U3 "0xff00ff00", "0xff00ff00"
#define FX_U4 "0xffff0000", "0xffff0000"
#define FX_U5 "0", "-1"
// The same three without the slot (the slotless layout): a stage is 7 vector instructions, and one crossbar transfer less
// where the partner comes over LDS.
#define FX_BITONIC3_DPP_(DPPSTR, ULO, UHI)                                                              \
    asm volatile("s_mov_b32 vcc_lo, " ULO "\n\ts_mov_b32 vcc_hi, " UHI "\n\t"                             \
                 "v_subb_co_u32_dpp %4, vcc, %2, %2, vcc " DPPSTR " row_mask:0xf bank_mask:0xf\n\t"      \
                 "v_subb_co_u32_dpp %4, vcc, %0, %0, vcc " DPPSTR " row_mask:0xf bank_mask:0xf\n\t"      \
                 "v_subb_co_u32_dpp %4, vcc, %1, %1, vcc " DPPSTR " row_mask:0xf bank_mask:0xf\n\t"      \
                 "s_xnor_b32 vcc_lo, vcc_lo, " ULO "\n\ts_xnor_b32 vcc_hi, vcc_hi, " UHI "\n\t"           \
                 "v_cndmask_b32_dpp %2, %2, %2, vcc " DPPSTR " row_mask:0xf bank_mask:0xf\n\t"           \
                 "v_cndmask_b32_dpp %0, %0, %0, vcc " DPPSTR " row_mask:0xf bank_mask:0xf\n\t"           \
                 "v_cndmask_b32_dpp %1, %1, %1, vcc " DPPSTR " row_mask:0xf bank_mask:0xf\n\t"           \
                 "v_cndmask_b32_dpp %3, %3, %3, vcc " DPPSTR " row_mask:0xf bank_mask:0xf"                \
                 : "+v"(flo), "+v"(fhi), "+v"(kx), "+v"(kc), "=&v"(scr)                                   \
                 :                                                                                        \
                 : "vcc", "scc")
#define FX_BITONIC3_XCH_(ULO, UHI)                                                                      \
    asm volatile("s_mov_b32 vcc_lo, " ULO "\n\ts_mov_b32 vcc_hi, " UHI "\n\t"                             \
                 "v_subb_co_u32 %4, vcc, %7, %2, vcc\n\t"                                                \
                 "v_subb_co_u32 %4, vcc, %5, %0, vcc\n\t"                                                \
                 "v_subb_co_u32 %4, vcc, %6, %1, vcc\n\t"                                                \
                 "s_xnor_b32 vcc_lo, vcc_lo, " ULO "\n\ts_xnor_b32 vcc_hi, vcc_hi, " UHI "\n\t"           \
                 "v_cndmask_b32 %2, %7, %2, vcc\n\t"                                                    \
                 "v_cndmask_b32 %0, %5, %0, vcc\n\t"                                                    \
                 "v_cndmask_b32 %1, %6, %1, vcc\n\t"                                                    \
                 "v_cndmask_b32 %3, %8, %3, vcc"                                                         \
                 : "+v"(flo), "+v"(fhi), "+v"(kx), "+v"(kc), "=&v"(scr)                                   \
                 : "v"(pflo), "v"(pfhi), "v"(px), "v"(pc)                                                 \
                 : "vcc", "scc")
#define FX_BITONIC3_SWZ_(M, ULO, UHI)                                                                   \
    do {                                                                                                \
        const uint32_t pflo = (uint32_t)__builtin_amdgcn_ds_swizzle((int)flo, 0x1F | ((M) << 10));      \
        const uint32_t pfhi = (uint32_t)__builtin_amdgcn_ds_swizzle((int)fhi, 0x1F | ((M) << 10));      \
        const uint32_t px = (uint32_t)__builtin_amdgcn_ds_swizzle((int)kx, 0x1F | ((M) << 10));         \
        const uint32_t pc = (uint32_t)__builtin_amdgcn_ds_swizzle((int)kc, 0x1F | ((M) << 10));         \
        FX_BITONIC3_XCH_(ULO, UHI);                                                                     \
    } while (0)
#define FX_BITONIC3_DPP(D, U) FX_BITONIC3_DPP_(D, U)
#define FX_BITONIC3_XCH(U) FX_BITONIC3_XCH_(U)
#define FX_BITONIC3_SWZ(M, U) FX_BITONIC3_SWZ_(M, U)
// The network, written once for both layouts: DPP / SWZ / M63 name the stage macros.
#define FX_BITONIC_NETWORK(DPP, SWZ, M63)                                          \
    /* blocks of 2 */                                                             \
    DPP("quad_perm:[1,0,3,2]", FX_U0);                                            \
    /* blocks of 4: mirror, then 1 */                                             \
    DPP("quad_perm:[3,2,1,0]", FX_U1);                                            \
    DPP("quad_perm:[1,0,3,2]", FX_U0);                                            \
    /* blocks of 8: mirror, 2, 1 */                                               \
    DPP("row_half_mirror", FX_U2);                                                \
    DPP("quad_perm:[2,3,0,1]", FX_U1);                                            \
    DPP("quad_perm:[1,0,3,2]", FX_U0);                                            \
    /* blocks of 16: mirror, 4, 2, 1 */                                           \
    DPP("row_mirror", FX_U3);                                                     \
    SWZ(4, FX_U2);                                                                \
    DPP("quad_perm:[2,3,0,1]", FX_U1);                                            \
    DPP("quad_perm:[1,0,3,2]", FX_U0);                                            \
    if (n > 16) {                                                                 \
        /* blocks of 32: mirror (lane ^ 31), 8, 4, 2, 1 */                        \
        SWZ(31, FX_U4);                                                           \
        DPP("row_ror:8", FX_U3);                                                  \
        SWZ(4, FX_U2);                                                            \
        DPP("quad_perm:[2,3,0,1]", FX_U1);                                        \
        DPP("quad_perm:[1,0,3,2]", FX_U0);                                        \
    }                                                                             \
    if (n > 32) {                                                                 \
        /* the wavefront: mirror (lane ^ 63), 16, 8, 4, 2, 1 */                   \
        M63();                                                                    \
        SWZ(16, FX_U4);                                                           \
        DPP("row_ror:8", FX_U3);                                                  \
        SWZ(4, FX_U2);                                                            \
        DPP("quad_perm:[2,3,0,1]", FX_U1);                                        \
        DPP("quad_perm:[1,0,3,2]", FX_U0);                                        \
    }
// the stage whose partner is lane ^ 63 (ds_bpermute)
#define FX_BITONIC_M63()                                                                                                     \
    do {                                                                                                                     \
        const int a = (lane ^ 63) << 2;                                                                                      \
        const uint32_t pflo = (uint32_t)__builtin_amdgcn_ds_bpermute(a, (int)flo), pfhi = (uint32_t)__builtin_amdgcn_ds_bpermute(a, (int)fhi), \
                       px = (uint32_t)__builtin_amdgcn_ds_bpermute(a, (int)kx), ps = (uint32_t)__builtin_amdgcn_ds_bpermute(a, (int)ks),       \
                       pc = (uint32_t)__builtin_amdgcn_ds_bpermute(a, (int)kc);                                              \
        FX_BITONIC_XCH(FX_U5);                                                                                               \
    } while (0)
#define FX_BITONIC3_M63()                                                                                                    \
    do {                                                                                                                     \
        const int a = (lane ^ 63) << 2;                                                                                      \
        const uint32_t pflo = (uint32_t)__builtin_amdgcn_ds_bpermute(a, (int)flo), pfhi = (uint32_t)__builtin_amdgcn_ds_bpermute(a, (int)fhi), \
                       px = (uint32_t)__builtin_amdgcn_ds_bpermute(a, (int)kx), pc = (uint32_t)__builtin_amdgcn_ds_bpermute(a, (int)kc);       \
        FX_BITONIC3_XCH(FX_U5);                                                                                              \
    } while (0)
template <bool NOSLOT>
__device__ __forceinline__ void r_sort(RTier& R, int lane, int n) {
    uint32_t flo = (uint32_t)R.f, fhi = (uint32_t)(R.f >> 32), kx = R.x, kc = R.c, scr;
    if constexpr (NOSLOT) {
        asm volatile("s_nop 1" : "+v"(flo), "+v"(fhi), "+v"(kx), "+v"(kc));  // (DPP reads want two wait states behind the VALU writes)
        FX_BITONIC_NETWORK(FX_BITONIC3_DPP, FX_BITONIC3_SWZ, FX_BITONIC3_M63)
    } else {
        uint32_t ks = R.s;
        asm volatile("s_nop 1" : "+v"(flo), "+v"(fhi), "+v"(kx), "+v"(ks), "+v"(kc));  // (DPP reads want two wait states behind the VALU writes)
        FX_BITONIC_NETWORK(FX_BITONIC_DPP, FX_BITONIC_SWZ, FX_BITONIC_M63)
        R.s = ks;
    }
    R.f = ((uint64_t)fhi << 32) | (uint64_t)flo;
    R.x = kx;
    R.c = kc;
}

// R runs low: hand it the smallest M entries, as many as it has room for, sorted behind the entries it still holds
// (every M key is at or above the R / M threshold, every R key below it), and close the gaps in M.
template <class MID>
__device__ __forceinline__ void r_refill(OpenList& Q, RTier& R, const MID& M, int lane) {
    open_uniform(Q);
#ifdef FXJPS_PROF
    unsigned long long rt_ = __builtin_readcyclecounter();
#define RT_MARK(k)                                                    \
    do {                                                              \
        const unsigned long long n_ = __builtin_readcyclecounter();   \
        DBG_COUNT(M, k, n_ - rt_);                                    \
        rt_ = n_;                                                     \
    } while (0)
#elif defined(FXJPS_MARK)
#define RT_MARK(k) asm volatile("; FXRT " #k)
#else
#define RT_MARK(k) \
    do {           \
    } while (0)
#endif
    // (the entry of r_refill: a mark of the FXJPS_MARK build.  The diagnostic build starts its clock above and counts
    // nothing here -- counter 39 is the detector's, the iterations with a hold)
#if !defined(FXJPS_PROF)
    RT_MARK(39);
#endif
    const uint32_t n = Q.m_n;
    const uint32_t room = min((uint32_t)(WAVE - Q.r_n), (uint32_t)WAVE);  // (r_n >= 0: the clamp is a no-op, kept for the instruction schedule it was measured with)
    uint64_t f[MSLOT];
    uint32_t x[MSLOT];
    uint64_t lo = ~0ull, hi = 0ull;
#pragma unroll
    for (int k = 0; k < MSLOT; k++) {
        const uint32_t i = (uint32_t)lane + (uint32_t)(k * WAVE);
        f[k] = ~0ull;
        x[k] = ~0u;
        if (i < n) {
            f[k] = M.w->f[i];
            x[k] = M.w->x[i];
            lo = f[k] < lo ? f[k] : lo;
            hi = f[k] > hi ? f[k] : hi;
        }
        RECONV();
    }
    uint64_t Pf = Q.Tbits;
    uint32_t Px = Q.Tx;
    uint32_t cnt = n;
    const uint64_t fmin_all = wave_umin64(lo);  // the smallest f of M: always among the entries taken
    if (n > room) {
        // aim at 3/4 of the room by interpolating in the key range of the candidates; narrow down while too many
        // qualify (a handful of rounds: the keys of an A* frontier are spread evenly)
        uint64_t fmn = fmin_all, fmx = ~wave_umin64(~hi);
        uint32_t cand = n;
        bool done = false, xm = false;
        for (int attempt = 0; attempt < 12 && !done; attempt++) {
            DBG_COUNT(M, 21, 1);
            const double frac = FXJPS_RFILL * (double)room / (double)cand;
            if (!xm) {
                const double dmn = __longlong_as_double((long long)fmn), dmx = __longlong_as_double((long long)fmx);
                const double mid = dmn + (dmx - dmn) * frac;
                if (mid > dmn) {
                    Pf = (uint64_t)__double_as_longlong(mid);
                    Px = 0;
                } else {
                    xm = true;
                }
            }
            if (xm) {
                // the candidates cannot be separated in f: slice the (x, y) range of the smallest f level
                uint32_t xl = ~0u, xh = 0u;
#pragma unroll
                for (int k = 0; k < MSLOT; k++) {
                    const bool at = f[k] == fmn && x[k] != ~0u && key_lt(f[k], x[k], Pf, Px);
                    xl = at && x[k] < xl ? x[k] : xl;
                    xh = at && x[k] > xh ? x[k] : xh;
                }
                const uint32_t xmn = wave_umin32(xl), xmx = ~wave_umin32(~xh);
                Pf = fmn;
                Px = xmn + 1u + (uint32_t)((double)(xmx - xmn) * frac);
            }
            uint32_t c = 0, cm = 0;  // entries below the threshold; those of them on the smallest f level
#pragma unroll
            for (int k = 0; k < MSLOT; k++) {
                const bool below = x[k] != ~0u && key_lt(f[k], x[k], Pf, Px);
                c += (uint32_t)__popcll(__ballot(below));
                cm += (uint32_t)__popcll(__ballot(below && f[k] == fmn));
            }
            cnt = c;
            if (c <= room) {
                done = true;  // c >= 1: the minimum is always below the threshold
            } else if (!xm && cm > room) {
                xm = true;  // the smallest f level alone is too much: slice it
                cand = cm;
            } else {
                if (!xm) fmx = Pf;  // still too many: they are the new candidates
                cand = c;
            }
        }
        if (!done) {
            // give up aiming: take the minimum alone (with its exact duplicates, if any)
            const uint64_t m0 = fmin_all;
            uint32_t xl = ~0u;
#pragma unroll
            for (int k = 0; k < MSLOT; k++) xl = (f[k] == m0 && x[k] < xl) ? x[k] : xl;
            Pf = m0;
            Px = wave_umin32(xl) + 1u;
            uint32_t c = 0;
#pragma unroll
            for (int k = 0; k < MSLOT; k++) c += (uint32_t)__popcll(__ballot(x[k] != ~0u && key_lt(f[k], x[k], Pf, Px)));
            cnt = c;
        }
    }
    RT_MARK(40);  // read M + threshold search
    // ---- the selected entries leave their M index for the free lanes of R, in rank order
    const uint32_t take_n = cnt < room ? cnt : room;  // (cnt > room only for > 64 identical keys: the rest stays behind)
    uint32_t base = 0;
    bool sel[MSLOT];
#pragma unroll
    for (int k = 0; k < MSLOT; k++) {
        const uint32_t i = (uint32_t)lane + (uint32_t)(k * WAVE);
        const bool s0 = x[k] != ~0u && key_lt(f[k], x[k], Pf, Px);
        const uint64_t sm = __ballot(s0);
        const uint32_t r = base + rank_below(sm);
        sel[k] = s0 && r < take_n;
        if (sel[k]) M.w->idx[r] = (uint16_t)i;
        RECONV();
        base += (uint32_t)__popcll(sm);
    }
    const uint32_t r0 = (uint32_t)Q.r_n;  // the entries R still holds stay in its first lanes
    if ((uint32_t)lane >= r0 && (uint32_t)lane < r0 + take_n) {
        const uint32_t j = M.w->idx[(uint32_t)lane - r0];
        R.f = M.w->f[j];
        R.x = M.w->x[j];
        if constexpr (!MID::SLOTLESS) R.s = M.w->s[j];
        R.c = M.w->c[j];
    }
    RECONV();
    DBG_COUNT(M, 20, 1);
    DBG_COUNT(M, 23, take_n);
    RT_MARK(41);  // select + gather
    r_sort<MID::SLOTLESS>(R, lane, (int)(r0 + take_n));
    RT_MARK(42);  // sort
    // ---- close the gaps (entries move down only, onto slots already read)
    uint32_t mw = 0;
#pragma unroll
    for (int k = 0; k < MSLOT; k++) {
        const uint32_t i = (uint32_t)lane + (uint32_t)(k * WAVE);
        const bool keep = x[k] != ~0u && !sel[k];
        const uint64_t km = __ballot(keep);
        uint32_t es = 0, ec = 0;
        if (keep) {
            if constexpr (!MID::SLOTLESS) es = M.w->s[i];
            ec = M.w->c[i];
        }
        RECONV();
        if (keep) {
            const uint32_t j = mw + rank_below(km);
            M.w->f[j] = f[k];
            M.w->x[j] = x[k];
            if constexpr (!MID::SLOTLESS) M.w->s[j] = es;
            M.w->c[j] = (uint16_t)ec;
        }
        RECONV();
        mw += (uint32_t)__popcll(km);
    }
    Q.m_n = mw;
    Q.r_n += (int)take_n;
    if (mw == 0) {  // M is empty: R may take everything below the far threshold
        Q.Rbits = Q.Tbits;
        Q.Rx = Q.Tx;
    } else if (cnt <= room) {
        Q.Rbits = Pf;
        Q.Rx = Px;
    }  // else (> 64 identical keys): the threshold stays; equal keys on both sides are interchangeable
}

// R after a batch: its first `drop` lanes (the committed nodes) leave and the entries held by the lanes of `rm`
// (key (kf, kx), payload ks, kc) merge in, keeping R sorted.  Each lane of the new R pulls its entry: a new one from
// the lane that pushed it, an old one from the lane it sat in.  NOSLOT (the slotless layout): no slot is pulled, ks is not used.
template <bool NOSLOT>
__device__ __forceinline__ void r_merge(OpenList& Q, RTier& R, int lane, int drop, bool toR, uint64_t rm, uint64_t kf, uint32_t kx,
                                        uint32_t ks, uint32_t kc) {
    const int old_n = Q.r_n;
    const bool old_valid = lane >= drop && lane < old_n;
    uint64_t newmask = 0ull;  // lanes of the merged R that receive a new entry
    uint32_t nsrc = 0;        // ... and the lane it comes from
    uint64_t m = rm;
    while (m != 0ull) {  // (wave-uniform loop over the new entries)
        const int src = (int)__builtin_ctzll(m);
        m &= m - 1ull;
        const uint64_t jf = lane_get64(kf, src);
        const uint32_t jx = lane_get(kx, src);
        // position = old entries at or before the new key + new entries before it (equal keys: lower lane first)
        const uint32_t cnt_old = (uint32_t)__popcll(__ballot(old_valid && !key_lt(jf, jx, R.f, R.x)));
        const uint32_t cnt_new = (uint32_t)__popcll(__ballot(toR && (key_lt(kf, kx, jf, jx) || (kf == jf && kx == jx && lane < src))));
        const uint32_t p = cnt_old + cnt_new;
        nsrc = (uint32_t)lane == p ? (uint32_t)src : nsrc;
        newmask |= 1ull << p;
    }
    const int new_n = old_n - drop + __popcll(rm);
    const bool isnew = ((newmask >> lane) & 1ull) != 0ull;
    const uint32_t srcl = (isnew ? nsrc : (uint32_t)(lane + drop) - rank_below(newmask)) & 63u;
    const bool live = lane < new_n;
    const uint32_t oflo = lane_pull((uint32_t)R.f, srcl), ofhi = lane_pull((uint32_t)(R.f >> 32), srcl);
    const uint32_t ox = lane_pull(R.x, srcl), os = NOSLOT ? 0u : lane_pull(R.s, srcl), oc = lane_pull(R.c, srcl);
    if (rm != 0ull) {
        const uint32_t nflo = lane_pull((uint32_t)kf, srcl), nfhi = lane_pull((uint32_t)(kf >> 32), srcl);
        const uint32_t nx = lane_pull(kx, srcl), ns = NOSLOT ? 0u : lane_pull(ks, srcl), nc = lane_pull(kc, srcl);
        R.f = !live ? ~0ull : (isnew ? (((uint64_t)nfhi << 32) | (uint64_t)nflo) : (((uint64_t)ofhi << 32) | (uint64_t)oflo));
        R.x = !live ? ~0u : (isnew ? nx : ox);
        if (!NOSLOT) R.s = isnew ? ns : os;
        R.c = isnew ? nc : oc;
    } else {
        R.f = !live ? ~0ull : (((uint64_t)ofhi << 32) | (uint64_t)oflo);
        R.x = !live ? ~0u : ox;
        if (!NOSLOT) R.s = os;
        R.c = oc;
    }
    Q.r_n = new_n;
}

// The open list after a batch: the first `drop` entries of R (the committed nodes) leave, and the entries held by the
// lanes with `w` (key (kf, kx), payload ks, kc) go into R when below the R / M threshold, into M when below the
// M / far threshold, else into the far tier.  jps1.py:227-228 for a whole batch.
template <bool BANDED, class MID>
__device__ __forceinline__ bool open_insert(const SearchArgs& A, OpenList& Q, RTier& R, const MID& M, FarEnt* __restrict__ far,
                                            int lane, int lane_c, int drop, bool w, uint64_t kf, uint32_t kx, uint32_t ks,
                                            uint32_t kc PF_PARAMS) {  // lane_c: the lane number again, for the rarely taken paths
    PF(2);
    uint16_t* fci = far_ci(far, A.far_cap);
    bool toR;
    uint64_t rm;
    for (;;) {  // make room in R by splitting it
        open_uniform(Q);
        drop = rfli(drop);
        toR = w && key_lt(kf, kx, Q.Rbits, Q.Rx);
        rm = __ballot(toR);
        if (FX_USUAL(Q.r_n - drop + __popcll(rm) <= WAVE)) break;
        if (drop > 0) {  // (rare: take the committed nodes out first, then halve what is left)
            r_merge<MID::SLOTLESS>(Q, R, lane_c, drop, false, 0ull, 0ull, 0u, 0u, 0u);
            drop = 0;
        }
        if (!r_split(Q, R, M, far, fci, lane_c, A.far_cap)) return false;
    }
    bool toM;
    uint64_t mm;
    for (;;) {  // make room in M by splitting it
        open_uniform(Q);
        toM = w && !toR && key_lt(kf, kx, Q.Tbits, Q.Tx);
        mm = __ballot(toM);
        if (FX_USUAL(Q.m_n + (uint32_t)__popcll(mm) <= (uint32_t)MCAP)) break;
        if (!m_split(Q, M, far, fci, lane_c, A.far_cap)) return false;
    }
    PF(12);
    const bool toFar = w && !toR && !toM;
    const uint64_t fmk = __ballot(toFar);
    if (fmk != 0ull && !far_push<BANDED>(Q, M, far, fci, A.far_cap, toFar, kf, kx, ks, kc)) return false;  // (nothing else has moved yet)
    DBG_COUNT(M, 32, __popcll(rm));   // pushes merged into R
    DBG_COUNT(M, 58, __popcll(mm));   // ... appended to M (the rest of the pushes goes to the far tier)
    DBG_COUNT(M, 50, (rm != 0ull || drop > 0) ? 1 : 0);
    if (rm != 0ull || drop > 0) r_merge<MID::SLOTLESS>(Q, R, lane, drop, toR, rm, kf, kx, ks, kc);
    PF(13);
    if (mm != 0ull) {
        if (toM) {
            const uint32_t j = Q.m_n + rank_below(mm);
            M.w->f[j] = kf;
            M.w->x[j] = kx;
            if constexpr (!MID::SLOTLESS) M.w->s[j] = ks;
            M.w->c[j] = (uint16_t)kc;
        }
        RECONV();
        Q.m_n += (uint32_t)__popcll(mm);
    }
    PF(14);
    return true;
}

// An explicit wait for everything in flight, on rarely taken paths.  The compiler's wait-count pass tracks "a load into
// register v may be outstanding" per register and merges that over every join of the control flow; a load that some
// rarely taken path issues and never looks at (a look-ahead, a value used under a condition) travels with the register
// around the search loop, and wherever the register is written next the pass drains the whole memory queue -- the
// previous batch's table stores included.  Seen in round 3 at the loop head and at the entry of every R refill
// (R refills twice as long, - 1.6 % plans/s); tools/isa_census.py lists the drain-everything waits of the hot path.
#define COLD_SYNC() __builtin_amdgcn_s_waitcnt(0x0F70)
// Make sure the minimum of the open list is in R (the heappop of jps1.py:198 then reads lane 0).  Returns false when
// the open list is empty.
template <bool BANDED, bool NOCI = false, class MID>  // NOCI: nobody reads the entries' cell info (rays on the jump-distance records)
__device__ __forceinline__ bool open_fill(const SearchArgs& A, const GridDev& G, OpenList& Q, RTier& R, const MID& M, FarEnt* __restrict__ far,
                                          int lane) {
    constexpr bool NOSLOT = MID::SLOTLESS;  // far entries are {f, xyd, cell info}: the u16 array behind them is not used
    uint16_t* fci = far_ci(far, A.far_cap);
    bool topped = false;
    for (;;) {
        open_uniform(Q);
        // (R is topped up from M -- once per call -- before it holds less than a full batch; the far tier waits until
        // both are empty)
        if (FX_USUAL(Q.r_n >= RLOW || (Q.r_n > 0 && (Q.m_n == 0 || topped)))) return true;
        if (FX_USUAL(Q.m_n > 0)) {
            topped = true;
#ifdef FXJPS_PROF
            const unsigned long long t0_ = __builtin_readcyclecounter();
#endif
            r_refill(Q, R, M, lane);
#ifdef FXJPS_PROF
            DBG_COUNT(M, 28, __builtin_readcyclecounter() - t0_);
            DBG_COUNT(M, 29, 1);
#endif
            continue;
        }
        if (Q.far_n == 0 && Q.farb_n == 0) return false;  // jps1.py:230
        // ---- far refill (R and M are empty): the far entries with key < (T.f + delta, 0) become the new M
        if (A.out_counters && lane == 0) atomicAdd(&A.out_counters[2], 1ull);  // (once per ~170 pops)
        RECONV();
        if (BANDED && Q.banded) {
            // (the lane number, opaque: what the ring's loops derive from it -- addresses into the regions -- is otherwise
            // hoisted to the top of the kernel and kept, or spilled, across the whole search)
            int lane_b = lane;
            asm volatile("" : "+v"(lane_b));
            // ---- the ring.  Once the near band is used up the refill takes the next bands of the ring whole (as many
            // as fit M): no threshold search, no compaction.  A band that alone is too much for M becomes the near
            // band and is handed out by the scan below; the last band of the ring (everything above it) is dealt out
            // over a new ring when its turn comes.  The ring is set up the first time the near band outgrows near_max.
            const uint32_t half = A.far_cap >> 1, bcap = band_cap(half, 0u);
            const uint32_t rmask = (uint32_t)NBANDS - 1u;
            const auto cell_info = [&](uint32_t xyd) -> uint32_t {
                if (NOCI) return 0u;
                return G.ci[(size_t)((xyd >> 17) + 1u) * (size_t)G.NS + (size_t)(((xyd >> 4) & 0x1FFFu) + 1u)];
            };
            bool took = false;
            if (Q.far_n == 0) {  // (then the ring is not empty: the far tier is not)
                for (;;) {
                    open_uniform(Q);
                    const uint32_t cnt_l = M.w->bcnt[lane_b];  // lane_b = band (the bands below cur0 are used up: empty)
                    const uint64_t nz = __ballot(cnt_l != 0u);
                    if (nz == 0ull) {  // (cannot happen: farb_n counts the entries of the ring)
                        Q.farb_n = 0;
                        break;
                    }
                    const int j0 = (int)__builtin_ctzll(nz);
                    if (j0 == NBANDS - 1) {
                        // ---- only the last region is left: new bands from its smallest key on
                        DBG_COUNT(M, 44, 1);
                        const uint32_t p = rmask;
                        const uint32_t n = lane_get(cnt_l, NBANDS - 1);
                        DBG_COUNT(M, 47, n);
                        FarEnt* reg = far + band_base(half, p);
                        uint32_t lo = ~0u, hi = 0u;
                        for (uint32_t i = (uint32_t)lane_b; i < n; i += WAVE) {
                            const uint32_t fh = (uint32_t)(reg[i].fbits >> 32);
                            lo = min(lo, fh);
                            hi = max(hi, fh);
                        }
                        RECONV();
                        // The bands start at the smallest key of the region -- but not below the M / far threshold:
                        // every M key must stay below the first band (M is evicted to the near band), so entries
                        // that share their high word with a threshold in the middle of it go to the near band.
                        const uint32_t tmin = (uint32_t)(Q.Tbits >> 32) + (((uint32_t)Q.Tbits != 0u || Q.Tx != 0u) ? 1u : 0u);
                        Q.T2hi = max(wave_umin32(lo), tmin);  // (at or above the start of the old last region)
                        Q.hshift = band_shift(Q.T2hi, max(~wave_umin32(~hi), Q.T2hi), Q.delta);
                        Q.cur0 = 0;
                        uint32_t wr = 0, nn = 0;
                        uint64_t ovf = 0ull;
                        for (uint32_t base = 0; base < n; base += WAVE) {
                            const uint32_t i = base + (uint32_t)lane_b;
                            const bool valid = i < n;
                            FarEnt e;
                            e.fbits = (uint64_t)Q.T2hi << 32;
                            e.xyd = 0;
                            e.slot = 0;
                            if (valid) e = reg[i];
                            RECONV();
                            const bool low = valid && (uint32_t)(e.fbits >> 32) < Q.T2hi;
                            const uint32_t rel = min(((uint32_t)(e.fbits >> 32) - Q.T2hi) >> Q.hshift, rmask);
                            const bool stay = valid && !low && rel == rmask;
                            const uint64_t sm = __ballot(stay), lm = __ballot(low);
                            ovf |= ring_put(Q, M, far, A.far_cap, valid && !low && !stay, e.fbits, e.xyd, e.slot);
                            if (stay) reg[wr + rank_below(sm)] = e;  // (moves down only, onto slots already read)
                            RECONV();
                            if (low) {  // (the near band is empty, and in the other half of the array)
                                const uint32_t j = nn + rank_below(lm);
                                far[j] = e;
                                fci[j] = (uint16_t)cell_info(e.xyd);
                            }
                            RECONV();
                            wr += (uint32_t)__popcll(sm);
                            nn += (uint32_t)__popcll(lm);
                        }
                        if (lane_b == 0) M.w->bcnt[p] = wr;
                        RECONV();
                        Q.far_n = nn;
                        Q.farb_n -= nn;
                        if (ovf != 0ull) {
                            Q.fail = 1u;
                            break;
                        }
                        if (nn != 0u) break;  // the scan below hands the near band out
                        if (Q.farb_n == 0) break;
                        continue;
                    }
                    uint32_t take = 0;
                    int j1 = j0 - 1;
                    for (int j = j0; j < NBANDS - 1; j++) {
                        const uint32_t c = lane_get(cnt_l, j);
                        if (take + c > (uint32_t)MCAP) break;
                        take += c;
                        j1 = j;
                        if (take >= (uint32_t)MCAP * 5u / 8u) break;
                    }
                    if (j1 < j0) {
                        // ---- one band is more than M holds: it becomes the near band
                        DBG_COUNT(M, 43, 1);
                        const uint32_t c = lane_get(cnt_l, j0);
                        const uint32_t p = (uint32_t)j0;
                        const FarEnt* reg = far + band_base(half, p);
                        for (uint32_t i = (uint32_t)lane_b; i < c; i += WAVE) {
                            const FarEnt e = reg[i];
                            far[i] = e;
                            fci[i] = (uint16_t)cell_info(e.xyd);
                        }
                        RECONV();
                        if (lane_b == 0) M.w->bcnt[p] = 0u;
                        RECONV();
                        Q.far_n = c;
                        Q.farb_n -= c;
                        Q.T2hi += (uint32_t)(j0 + 1 - (int)Q.cur0) << Q.hshift;
                        Q.cur0 = (uint32_t)j0 + 1u;
                        Q.delta = fmax(Q.delta * 0.75, 1e-9);
                        break;
                    }
                    // ---- the bands j0 .. j1 become M
                    uint32_t mn = 0;
                    for (int j = j0; j <= j1; j++) {
                        const uint32_t c = lane_get(cnt_l, j);
                        if (c == 0u) continue;
                        const uint32_t p = (uint32_t)j;
                        const FarEnt* reg = far + band_base(half, p);
                        for (uint32_t i = (uint32_t)lane_b; i < c; i += WAVE) {
                            const FarEnt e = reg[i];
                            const uint32_t ec = cell_info(e.xyd);
                            M.w->f[mn + i] = e.fbits;
                            M.w->x[mn + i] = e.xyd;
                            if constexpr (!MID::SLOTLESS) M.w->s[mn + i] = e.slot;  // (the ring serves the carrying layout only)
                            M.w->c[mn + i] = (uint16_t)ec;
                        }
                        RECONV();
                        if (lane_b == 0) M.w->bcnt[p] = 0u;
                        RECONV();
                        mn += c;
                    }
                    DBG_COUNT(M, 26, 1);
                    DBG_COUNT(M, 27, mn);
                    // (the width of the next set of bands follows what these held: 32 .. 96 entries per band)
                    if (mn > 96u * (uint32_t)(j1 - j0 + 1))
                        Q.delta = fmax(Q.delta * 0.75, 1e-9);
                    else if (mn < 32u * (uint32_t)(j1 - j0 + 1))
                        Q.delta *= 1.25;
                    Q.m_n = mn;
                    Q.farb_n -= mn;
                    Q.Rbits = Q.Tbits;  // R is empty and every entry of the new M came from the far tier: the old far
                    Q.Rx = Q.Tx;        // threshold separates them
                    Q.T2hi += (uint32_t)(j1 + 1 - (int)Q.cur0) << Q.hshift;
                    Q.cur0 = (uint32_t)j1 + 1u;
                    if (Q.farb_n == 0) {  // the far tier is empty
                        Q.T2hi = INF_HI;
                        Q.Tbits = F_INF;
                    } else {
                        Q.Tbits = (uint64_t)Q.T2hi << 32;
                    }
                    Q.Tx = 0;
                    took = true;
                    break;
                }
            } else if (Q.T2hi >= INF_HI && Q.far_n > A.near_max && bcap >= BAND_MIN_CAP) {
                // ---- the near band has grown: what lies more than a refill width above the threshold starts the ring
                const double tf = __longlong_as_double((long long)Q.Tbits);
                uint32_t t2 = (uint32_t)((uint64_t)__double_as_longlong(tf + Q.delta) >> 32) + 1u;
                if (t2 <= (uint32_t)(Q.Tbits >> 32)) t2 = (uint32_t)(Q.Tbits >> 32) + 1u;
                if (t2 < INF_HI) {
                    DBG_COUNT(M, 44, 1);
                    uint32_t hi = t2;
                    for (uint32_t i = (uint32_t)lane_b; i < Q.far_n; i += WAVE) hi = max(hi, (uint32_t)(far[i].fbits >> 32));
                    RECONV();
                    Q.T2hi = t2;
                    Q.hshift = band_shift(t2, ~wave_umin32(~hi), Q.delta);
                    Q.cur0 = 0;
                    const uint32_t an = Q.far_n;
                    DBG_COUNT(M, 47, an);
                    uint32_t wa = 0, up_n = 0;
                    uint64_t ovf = 0ull;
                    for (uint32_t base = 0; base < an; base += WAVE) {
                        const uint32_t i = base + (uint32_t)lane_b;
                        const bool valid = i < an;
                        FarEnt e;
                        e.fbits = (uint64_t)t2 << 32;
                        e.xyd = 0;
                        e.slot = 0;
                        uint32_t ec = 0;
                        if (valid) {
                            e = far[i];
                            ec = fci[i];
                        }
                        RECONV();
                        const bool up = valid && (uint32_t)(e.fbits >> 32) >= t2;
                        const bool stay = valid && !up;
                        const uint64_t sm = __ballot(stay);
                        ovf |= ring_put(Q, M, far, A.far_cap, up, e.fbits, e.xyd, e.slot);
                        if (stay) {
                            const uint32_t j = wa + rank_below(sm);
                            far[j] = e;
                            fci[j] = (uint16_t)ec;
                        }
                        RECONV();
                        wa += (uint32_t)__popcll(sm);
                        up_n += (uint32_t)__popcll(__ballot(up));
                    }
                    Q.far_n = wa;
                    Q.farb_n += up_n;
                    if (ovf != 0ull) Q.fail = 1u;
                }
            }
            open_uniform(Q);
            if (Q.fail != 0u) return true;  // (the caller gives the query up)
            if (took) continue;             // M is filled: R takes from it
            if (Q.far_n == 0) continue;     // (a new ring, or nothing at all: look again)
        } else {
        // ---- re-banding.  A refill scans and rewrites the near band only.  When that band is used up, the lowest
        // FBANDS refill widths of the far band become the new near band (one pass over the far band); when it has
        // grown beyond near_max entries, what lies above that width moves to the far band (one pass over the near
        // band).  Either way:  near < (T2hi << 32, 0) <= far.
        {
            const uint32_t half = A.far_cap >> 1;
            const double tf = __longlong_as_double((long long)Q.Tbits);  // every far key is >= (Tbits, Tx); finite: the tier is not empty
            // (the threshold is a high word: the band ends at the next multiple of 2^32 in f bits, > T)
            uint32_t t2 = (uint32_t)((uint64_t)__double_as_longlong(tf + (double)FBANDS * Q.delta) >> 32) + 1u;
            if (t2 <= (uint32_t)(Q.Tbits >> 32)) t2 = (uint32_t)(Q.Tbits >> 32) + 1u;
            if (Q.far_n == 0) {
                DBG_COUNT(M, 43, 1);
                for (int round = 0; round < 3 && Q.far_n == 0; round++) {
                    const uint32_t bn = Q.farb_n;
                    DBG_COUNT(M, 47, bn);
                    uint32_t wa = 0, wb = 0;
                    uint64_t fmin = ~0ull;  // smallest f that stays in the far band
                    for (uint32_t base = 0; base < bn; base += WAVE) {
                        const uint32_t i = base + (uint32_t)lane;
                        const bool valid = i < bn;
                        FarEnt e;
                        e.fbits = ~0ull;
                        e.xyd = 0;
                        e.slot = 0;
                        uint32_t ec = 0;
                        if (valid) {
                            e = far[half + i];
                            ec = NOSLOT ? e.slot : (uint32_t)fci[half + i];
                        }
                        RECONV();
                        const bool down = valid && (uint32_t)(e.fbits >> 32) < t2;
                        const bool stay = valid && !down;
                        const uint64_t dm = __ballot(down), sm = __ballot(stay);
                        if (down) {  // (the near band is empty and at most as long as what has been read: no overlap)
                            const uint32_t j = wa + rank_below(dm);
                            far[j] = e;
                            if (!NOSLOT) fci[j] = (uint16_t)ec;
                        }
                        RECONV();
                        if (stay) {  // compaction moves entries down only, onto slots already read
                            const uint32_t j = half + wb + rank_below(sm);
                            far[j] = e;
                            if (!NOSLOT) fci[j] = (uint16_t)ec;
                            fmin = e.fbits < fmin ? e.fbits : fmin;
                        }
                        RECONV();
                        wa += (uint32_t)__popcll(dm);
                        wb += (uint32_t)__popcll(sm);
                    }
                    Q.far_n = wa;
                    Q.farb_n = wb;
                    if (wa == 0) {  // a gap in the keys: the band starts at the smallest far key
                        fmin = wave_umin64(fmin);
                        t2 = (uint32_t)((uint64_t)__double_as_longlong(__longlong_as_double((long long)fmin) + (double)FBANDS * Q.delta) >> 32) + 1u;
                        if (t2 <= (uint32_t)(fmin >> 32)) t2 = (uint32_t)(fmin >> 32) + 1u;
                    }
                }
                Q.T2hi = Q.farb_n == 0 ? (uint32_t)(F_INF >> 32) : t2;
            } else if (Q.far_n > A.near_max && t2 < Q.T2hi && Q.far_n + Q.farb_n <= half) {
                DBG_COUNT(M, 44, 1);
                const uint32_t an = Q.far_n;
                DBG_COUNT(M, 47, an);
                uint32_t wa = 0, wb = Q.farb_n;
                for (uint32_t base = 0; base < an; base += WAVE) {
                    const uint32_t i = base + (uint32_t)lane;
                    const bool valid = i < an;
                    FarEnt e;
                    e.fbits = ~0ull;
                    e.xyd = 0;
                    e.slot = 0;
                    uint32_t ec = 0;
                    if (valid) {
                        e = far[i];
                        ec = NOSLOT ? e.slot : (uint32_t)fci[i];
                    }
                    RECONV();
                    const bool up = valid && (uint32_t)(e.fbits >> 32) >= t2;
                    const bool stay = valid && !up;
                    const uint64_t um = __ballot(up), sm = __ballot(stay);
                    if (up) {
                        const uint32_t j = half + wb + rank_below(um);
                        far[j] = e;
                        if (!NOSLOT) fci[j] = (uint16_t)ec;
                    }
                    RECONV();
                    if (stay) {
                        const uint32_t j = wa + rank_below(sm);
                        far[j] = e;
                        if (!NOSLOT) fci[j] = (uint16_t)ec;
                    }
                    RECONV();
                    wa += (uint32_t)__popcll(sm);
                    wb += (uint32_t)__popcll(um);
                }
                Q.far_n = wa;
                Q.farb_n = wb;
                Q.T2hi = t2;
            }
            open_uniform(Q);
            if (Q.far_n == 0) continue;  // (cannot happen: a pass over a non-empty far band moves at least its minimum)
        }
        }
        const uint64_t Tf_old = Q.Tbits;
        const uint32_t Tx_old = Q.Tx;
        uint64_t Tnb = (uint64_t)__double_as_longlong(__longlong_as_double((long long)Q.Tbits) + Q.delta);
        uint32_t Tnx = 0;
        if (Q.dxs > 0 && Q.Tbits != F_INF) {  // keep slicing the same f level (hchoice 1: hundreds of equal f)
            Tnb = Q.Tbits;
            Tnx = (Q.Tx > ~0u - Q.dxs) ? ~0u : Q.Tx + Q.dxs;
        }
        bool xmode = Q.dxs > 0;
        for (int attempt = 0; attempt < 12; attempt++) {
            // The first pass almost always succeeds (measured: 1.00 passes per refill), so it does not keep the
            // statistics a failed pass needs for re-aiming: when it does fail they are gathered by a read-only scan
            // (far_stats below), and the later passes keep them as they go.
            const bool trk = attempt > 0;
            // (a refill never reaches into the far band: its threshold stops at the band threshold)
            const uint64_t T2bits = (uint64_t)Q.T2hi << 32;
            const bool clamped = Tnb > T2bits || (Tnb == T2bits && Tnx != 0u);
            if (clamped) {
                Tnb = T2bits;
                Tnx = 0;
            }
            uint64_t wfmin = ~0ull, wfmax = 0ull;  // key range of the candidates
            uint32_t wxmin = ~0u, wxmax = 0u;
            uint64_t lfmin = ~0ull;                // smallest candidate key that did not fit
            uint32_t lxmin = ~0u;
            uint64_t fmin = ~0ull;                 // smallest f that stays behind
            uint32_t W = 0, wr = 0;
            const uint32_t fn = Q.far_n;
            // FPD chunks of 64 entries are kept in flight, each slot of the ring reloaded FPD chunks ahead as soon as
            // it has been consumed (compaction writes land at or below the entry being processed: never on an entry
            // that has not been loaded yet).  Measured on config 2: 4 in flight are no faster than 1 -- a refill scans
            // ~25 chunks once per ~170 pops and its cost is on the LDS side -- so FPD = 1 (3 VGPRs fewer).
            DBG_COUNT(M, 26, 1);
            DBG_COUNT(M, 27, fn);
#ifdef FXJPS_PROF
            const unsigned long long tf0_ = __builtin_readcyclecounter();
#endif
            FarEnt eq[FPD];
            uint32_t cq[FPD];
#pragma unroll
            for (int k = 0; k < FPD; k++) {
                eq[k].fbits = ~0ull;
                eq[k].xyd = 0;
                eq[k].slot = 0;
                cq[k] = 0;
                const uint32_t i0 = (uint32_t)(k * WAVE) + (uint32_t)lane;
                if (i0 < fn) {
                    eq[k] = far[i0];
                    if (!NOSLOT) cq[k] = fci[i0];
                }
                RECONV();
            }
            uint32_t mn = 0;  // entries placed in M so far
            for (uint32_t base0 = 0; base0 < fn; base0 += FPD * WAVE) {
#pragma unroll
              for (int k = 0; k < FPD; k++) {
                const uint32_t base = base0 + (uint32_t)(k * WAVE);
                if (base >= fn) break;
                const uint32_t i = base + lane;
                const FarEnt e = eq[k];
                const uint32_t ec = NOSLOT ? e.slot : cq[k];  // (the slotless layout: the cell info is the entry's fourth dword)
                const bool valid = i < fn;
                eq[k].fbits = ~0ull;
                if (i + FPD * WAVE < fn) {
                    eq[k] = far[i + FPD * WAVE];
                    if (!NOSLOT) cq[k] = fci[i + FPD * WAVE];
                }
                RECONV();
                const bool want = valid && key_lt(e.fbits, e.xyd, Tnb, Tnx);
                const uint64_t wm = __ballot(want);
                W += (uint32_t)__popcll(wm);
                const uint32_t rank = rank_below(wm);
                const bool fits = want && (mn + rank < (uint32_t)MCAP);
                if (trk && want) {  // f range of the candidates, and the (x, y) range of those with the smallest f
                    wfmax = e.fbits > wfmax ? e.fbits : wfmax;
                    if (e.fbits < wfmin) {
                        wfmin = e.fbits;
                        wxmin = e.xyd;
                        wxmax = e.xyd;
                    } else if (e.fbits == wfmin) {
                        wxmin = e.xyd < wxmin ? e.xyd : wxmin;
                        wxmax = e.xyd > wxmax ? e.xyd : wxmax;
                    }
                }
                RECONV();
                if (fits) {
                    const uint32_t j = mn + rank;
                    M.w->f[j] = e.fbits;
                    M.w->x[j] = e.xyd;
                    if constexpr (!NOSLOT) M.w->s[j] = e.slot;
                    M.w->c[j] = (uint16_t)ec;
                }
                RECONV();
                if (trk && want && !fits && key_lt(e.fbits, e.xyd, lfmin, lxmin)) {
                    lfmin = e.fbits;
                    lxmin = e.xyd;
                }
                RECONV();
                mn += (uint32_t)__popcll(__ballot(fits));
                const bool keep = valid && !fits;
                if (trk && keep) fmin = e.fbits < fmin ? e.fbits : fmin;
                RECONV();
                const uint64_t km = __ballot(keep);
                if (keep) {
                    const uint32_t j = wr + rank_below(km);
                    far[j] = e;
                    if (!NOSLOT) fci[j] = (uint16_t)ec;
                }
                RECONV();
                wr += (uint32_t)__popcll(km);
              }
            }
#ifdef FXJPS_PROF
            DBG_COUNT(M, 30, __builtin_readcyclecounter() - tf0_);
#endif
            Q.far_n = wr;
            Q.m_n = mn;
            const bool overflow = W > mn;  // M was empty: it holds what fitted
            // what the untracked first pass did not gather, for the far tier as it is now
            auto far_stats = [&]() {
                for (uint32_t i = lane; i < Q.far_n; i += WAVE) {
                    const FarEnt e = far[i];
                    fmin = e.fbits < fmin ? e.fbits : fmin;
                    if (key_lt(e.fbits, e.xyd, Tnb, Tnx)) {
                        wfmax = e.fbits > wfmax ? e.fbits : wfmax;
                        if (e.fbits < wfmin) {
                            wfmin = e.fbits;
                            wxmin = e.xyd;
                            wxmax = e.xyd;
                        } else if (e.fbits == wfmin) {
                            wxmin = e.xyd < wxmin ? e.xyd : wxmin;
                            wxmax = e.xyd > wxmax ? e.xyd : wxmax;
                        }
                    }
                }
                RECONV();
            };
            if (!overflow) {
                Q.Tbits = Tnb;
                Q.Tx = Tnx;
                if (mn > 0 || Q.far_n == 0) {
                    if (attempt == 0 && !clamped) {
                        if (xmode) {
                            if (mn < (uint32_t)MCAP / 4) Q.dxs = Q.dxs > 0x3FFFFFFFu ? ~0u : Q.dxs * 2u;
                        } else if (mn < (uint32_t)MCAP / 4) {
                            Q.delta *= 1.5;
                        } else if (mn > (uint32_t)MCAP * 3 / 4) {
                            Q.delta *= 0.75;
                        }
                    }
                    if (!xmode) Q.dxs = 0;
                    break;
                }
                // nothing was below the threshold (a gap in the keys): restart the band at the smallest far key
                if (!trk) far_stats();
                fmin = wave_umin64(fmin);
                Tnb = (uint64_t)__double_as_longlong(__longlong_as_double((long long)fmin) + Q.delta);
                if (Tnb <= fmin) Tnb = fmin + 1ull;  // delta below half an ulp of f: step to the next double
                Tnx = 0;
                xmode = false;
                continue;
            }
            if (attempt == 11) {
                // give up aiming: keep what sorts before the smallest candidate that stayed behind
                const uint64_t lf = wave_umin64(lfmin);
                const uint32_t lx = wave_umin32(lfmin == lf ? lxmin : ~0u);
                (void)m_evict(Q, M, far, fci, lane, lf, lx, A.far_cap, false);
                break;
            }
            // more candidates than slots.  Everything in M came from this refill: put it back and aim at a
            // fraction of the candidates' key range (f range, or (x, y) range when they all share one f -- the
            // normal case with the octile heuristic).
            (void)m_evict(Q, M, far, fci, lane, 0ull, 0u, A.far_cap, false);
            Q.Tbits = Tf_old;
            Q.Tx = Tx_old;
            if (!trk) far_stats();  // (everything is back in the far tier: the candidates are its entries below the threshold)
            const uint64_t fmn = wave_umin64(wfmin), fmx = ~wave_umin64(~wfmax);
            const double frac = 0.6 * (double)MCAP / (double)W;
            const double dmn = __longlong_as_double((long long)fmn), dmx = __longlong_as_double((long long)fmx);
            const double cand = dmn + (dmx - dmn) * frac;
            if (cand > dmn) {
                Tnb = (uint64_t)__double_as_longlong(cand);
                Tnx = 0;
                xmode = false;
                Q.delta = fmax(Q.delta * 0.5, 1e-9);
            } else {
                // cannot be separated in f: candidates with f == fmn, split on (x, y)
                const uint32_t xmn = wave_umin32(wfmin == fmn ? wxmin : ~0u);
                const uint32_t xmx = ~wave_umin32(wfmin == fmn ? ~wxmax : ~0u);
                Tnb = fmn;
                Tnx = xmn + 1u + (uint32_t)((double)(xmx - xmn) * frac);
                xmode = true;
                Q.dxs = Tnx - xmn;
            }
        }
        open_uniform(Q);
        if (Q.far_n == 0 && Q.farb_n == 0) {
            Q.Tbits = F_INF;
            Q.Tx = 0;
            Q.T2hi = (uint32_t)(F_INF >> 32);
        }
        // R is empty and every entry of the new M came from the far tier: the old far threshold separates them
        Q.Rbits = Tf_old;
        Q.Rx = Tx_old;
        if (Q.m_n > 0) continue;
        if (Q.far_n == 0 && Q.farb_n == 0) return false;
        if (Q.far_n == 0) continue;  // the near band is used up and nothing came of it: re-band and try again
        // ---- degenerate: more than MCAP entries tie at the minimum key.  Move the (f, x, y) minimum straight
        // from the far tier into R; the thresholds are untouched (R and M are empty).
        if (A.out_counters && lane == 0) atomicAdd(&A.out_counters[3], 1ull);
        RECONV();
        uint64_t cf = ~0ull;
        uint32_t cx = ~0u;
        int ci = -1;
        for (uint32_t i = lane; i < Q.far_n; i += WAVE) {
            const FarEnt e = far[i];
            if (e.fbits < cf || (e.fbits == cf && e.xyd < cx)) {
                cf = e.fbits;
                cx = e.xyd;
                ci = (int)i;
            }
        }
        RECONV();
        const uint64_t gf = wave_umin64(cf);
        const uint32_t gx = wave_umin32(cf == gf ? cx : ~0u);
        const uint64_t own = __ballot(ci >= 0 && cf == gf && cx == gx);
        const uint32_t fi = rfl((uint32_t)__shfl(ci, (int)__builtin_ctzll(own), WAVE));
        {  // it becomes the only entry of R
            const uint32_t gs = rfl(far[fi].slot), gc = NOSLOT ? gs : rfl((uint32_t)fci[fi]);
            const bool l0 = lane == 0;
            R.f = l0 ? gf : ~0ull;
            R.x = l0 ? gx : ~0u;
            if (!NOSLOT) R.s = gs;
            R.c = gc;
            Q.r_n = 1;
        }
        const uint32_t last = Q.far_n - 1;
        if (fi != last) {
            const FarEnt le = far[last];
            const uint16_t lc = NOSLOT ? (uint16_t)0 : fci[last];
            if (lane == 0) {
                far[fi] = le;
                if (!NOSLOT) fci[fi] = lc;
            }
            RECONV();
        }
        Q.far_n = last;
        return true;
    }
}

// ---- batch geometry.  One iteration of the search loop takes the first nodes of R -- up to KN of them, as many as
// their rays fit the 64 lanes -- and expands them together (all rays of all nodes in flight at once), then commits
// them in pop order.  Node i of a batch is only committed if the reference would really pop it next: no earlier node
// of the batch pushed a key <= its key.  A node that fails the test stays in the open list untouched, so the pop
// sequence, every relaxation and every tie-break are exactly those of jps1.py:196-228.
// Lanes are dealt out by need: a node gets one lane per direction nodeNeighbours (jps1.py:49-93) leaves it (1 - 3
// as a rule, 5 at most behind a diagonal parent, 8 for the start), at least one.  (Until round 2 every node had a
// fixed group of 8 lanes, 8 nodes per batch: the long queries of config 2 commit 7.7 of 8 nodes -- and 14 of 16.
// Measured with up to 24 / 32 nodes: a long query alone on the chip ends 13 % sooner, a chip full of queries gets
// through 5 - 7 % fewer -- the additional speculative loads are thrown away more often than not.)
// Batches of up to 32 nodes (build with -DFXJPS_KN=32; two DPP rows, duplicates across the rows by one swap and 16
// rotations) were measured in rounds 3 and 5: a lone 137 k-pop query 44 -> 39 ms, but the queries that end the launches of
// config 2 and config 5 are the ones whose successors keep landing inside the batch (5.8 nodes committed per iteration
// whatever its width), and the second row's bookkeeping costs every iteration: c2 - 1 %, c4shard - 3 %, c3 - 2 %.  So 16 is
// the width; the macro stays as a measurement aid (tests/test_host_cpu.py cross-compiles it).
#ifndef FXJPS_KN
#define FXJPS_KN 16
#endif
constexpr int KN = FXJPS_KN;        // nodes per batch, at most: the lanes of the first one or two DPP rows of R
static_assert(KN >= 1 && KN <= 32, "the lane allotment scans two 16-lane rows");
constexpr int SL = 1;               // lanes per ray (round 1 spread a ray over up to four)
constexpr int BUCKET = 4;           // table slots per bucket (one probe reads a whole bucket)
constexpr int EPL = BUCKET / SL;    // bucket slots the lane of a ray looks at
__host__ __device__ constexpr uint32_t ceil_log2_c(int v) { return v <= 1 ? 0u : 1u + ceil_log2_c((v + 1) / 2); }

// value of lane - K within the 16-lane row; lanes without such a lane get `old`
template <int K>
__device__ __forceinline__ uint32_t row_shr(uint32_t old, uint32_t v) {
    return (uint32_t)__builtin_amdgcn_update_dpp((int)old, (int)v, 0x110 + K, 0xF, 0xF, false);
}
// Inclusive prefix sum / prefix OR over the lanes of each 16-lane row.
__device__ __forceinline__ uint32_t row_scan_add(uint32_t v) {
    v += row_shr<1>(0u, v);
    v += row_shr<2>(0u, v);
    v += row_shr<4>(0u, v);
    v += row_shr<8>(0u, v);
    return v;
}
__device__ __forceinline__ uint32_t row_scan_or(uint32_t v) {
    v |= row_shr<1>(0u, v);
    v |= row_shr<2>(0u, v);
    v |= row_shr<4>(0u, v);
    v |= row_shr<8>(0u, v);
    return v;
}
// Does an earlier lane of my 16-lane row hold the same value?  All 15 comparisons: the value of lane - k arrives by
// DPP (row_shr; lanes without a source are skipped and keep the difference of the step before, which is harmless under
// a minimum).  `v` must not be all ones.
#define FX_DUP_STEP(k) \
    asm("v_xor_b32_dpp %1, %2, %2 row_shr:" #k " row_mask:0xf bank_mask:0xf\n\tv_min_u32 %0, %0, %1" : "+v"(acc), "+v"(tmp) : "v"(v))
__device__ __forceinline__ bool row_dup_before(uint32_t v) {
    uint32_t acc = ~0u, tmp = ~0u;
    asm volatile("s_nop 1" : "+v"(v));  // (a DPP read of a VGPR needs two wait states behind the VALU write; inline asm is not seen by the hazard pass)
    FX_DUP_STEP(1); FX_DUP_STEP(2); FX_DUP_STEP(3); FX_DUP_STEP(4); FX_DUP_STEP(5);
    FX_DUP_STEP(6); FX_DUP_STEP(7); FX_DUP_STEP(8); FX_DUP_STEP(9); FX_DUP_STEP(10);
    FX_DUP_STEP(11); FX_DUP_STEP(12); FX_DUP_STEP(13); FX_DUP_STEP(14); FX_DUP_STEP(15);
    return acc == 0u;
}

// Two rows (a batch of more than 16 nodes): does a lane of the OTHER row of my row pair (0 / 1) hold the same value?
// The other row's values come over with one swap, then 16 rotations inside the row.  Only row 1 asks (its nodes come
// after all of row 0).
#define FX_XDUP_STEP(k) \
    asm("v_xor_b32_dpp %1, %3, %2 row_ror:" #k " row_mask:0xf bank_mask:0xf\n\tv_min_u32 %0, %0, %1" : "+v"(acc), "+v"(tmp) : "v"(v), "v"(o))
__device__ __forceinline__ bool row_dup_cross(uint32_t v, int lane) {
    uint32_t o = lane_xor16(v, lane);
    uint32_t acc = o ^ v, tmp = ~0u;
    asm volatile("s_nop 1" : "+v"(o), "+v"(v));  // (DPP reads need two wait states behind the VALU writes; inline asm is not seen by the hazard pass)
    FX_XDUP_STEP(1); FX_XDUP_STEP(2); FX_XDUP_STEP(3); FX_XDUP_STEP(4); FX_XDUP_STEP(5);
    FX_XDUP_STEP(6); FX_XDUP_STEP(7); FX_XDUP_STEP(8); FX_XDUP_STEP(9); FX_XDUP_STEP(10);
    FX_XDUP_STEP(11); FX_XDUP_STEP(12); FX_XDUP_STEP(13); FX_XDUP_STEP(14); FX_XDUP_STEP(15);
    return acc == 0u;
}

// One probe of a ray's bucket: lane t holds slots t*EPL .. t*EPL+EPL-1.  Ray-uniform results.
struct Probe {
    TEnt e[EPL];
};
template <bool DIRECT>
__device__ __forceinline__ void probe_load(Probe& P, const TEnt* __restrict__ tab, uint32_t b, int t, bool act) {
    // every lane loads (no exec-mask block, no zero-filling): lanes without a ray read bucket 0, one line for all of
    // them, and probe_eval ignores what they got
    const uint32_t bb = act ? b : 0u;
    if (DIRECT) {  // b is the slot of the cell itself
        P.e[0] = tab[bb];
        return;
    }
#pragma unroll
    for (int k = 0; k < EPL; k++) P.e[k] = tab[(size_t)bb * BUCKET + (size_t)(t * EPL + k)];
}
template <bool DIRECT>
__device__ __forceinline__ void probe_eval(const Probe& P, bool act, uint32_t cellj, uint32_t b, uint32_t gen,
                                           bool* found, bool* has_empty, uint32_t* slot, double* jg, uint32_t* jkey) {
    if (DIRECT) {  // one entry per cell: it is the cell's if it is live, free otherwise
        const bool live = ent_gen(P.e[0].key, P.e[0].par) == gen;
        *found = act && live;
        *has_empty = act && !live;
        *slot = b;
        *jg = P.e[0].g;
        *jkey = P.e[0].key;
        return;
    }
    uint32_t lm = 0, le = 0;  // which of my slots match the cell / are empty
    double mg = 0.0;
    uint32_t mk = 0;
#pragma unroll
    for (int k = 0; k < EPL; k++) {
        const bool live = ent_gen(P.e[k].key, P.e[k].par) == gen;
        const bool m = act && live && ((P.e[k].key & CELL_MASK) == cellj);
        const bool v = act && !live;  // never written, or left over from an earlier query: free
        lm |= (m ? 1u : 0u) << k;
        le |= (v ? 1u : 0u) << k;
        mg = m ? P.e[k].g : mg;
        mk = m ? P.e[k].key : mk;
    }
    // (one lane per ray: everything is already in this lane)
    const bool f1 = lm != 0;
    const uint32_t sel = f1 ? lm : le;
    uint32_t in1 = (uint32_t)__builtin_ctz(sel | (1u << EPL));
    in1 = in1 >= (uint32_t)EPL ? 0u : in1;
    *found = f1;
    *has_empty = le != 0;
    *slot = b * (uint32_t)BUCKET + in1;
    *jg = mg;
    *jkey = mk;
}


// identifySuccessors (jps1.py:166-179) for the nodes of a batch: one lane per ray, a ray ONE u16 of its node's jump-distance
// record (k_derive_jd): how far the goal-free jump gets and whether it ends on a jump point -- the rays of a node one 16-byte
// record, one memory request.  (History: until round 3 a diagonal ray read the cell info of two cells per memory round trip
// and evaluated them step by step, `expand_steps`; round 4 first made every ray one 16-byte scan word and a find-first-set,
// `expand_words`, then precomputed the jumps themselves.  Both older forms were deleted in round 6; git has them.)
// The goal: on the ray at or before
// the cell that ends it, it is the jump point (a squeezed step onto it, dblock, still returns None: the record says so);
// the cells of a diagonal ray on the goal's row and column are looked at with the scan words (scan_two).
template <bool HAVE_REC>  // HAVE_REC: the node's record arrived with the lane deal (r0 .. r3); else the lane reads its own u16
__device__ __forceinline__ void expand_jd(const GridDev& G, uint32_t r0, uint32_t r1, uint32_t r2, uint32_t r3, int cpx, int cpy, const uint32_t code, bool node_on, int gpx, int gpy,
                                          bool* ohas, uint32_t* ocellj, uint32_t* ojci, const TEnt* __restrict__ tab, uint32_t n_slot,
                                          TEnt* ecv, int* okres PF_PARAMS) {
    const bool act = code != DIR_NONE;
    const int dx = (int)(code >> 2) - 1, dy = (int)(code & 3u) - 1;
    const bool diag = act && dx != 0 && dy != 0;
    const bool alongY = (dx == 0);
    const uint32_t slot = code - (code >= 3u ? 1u : 0u) - (code >= 5u ? 1u : 0u) - (code >= 7u ? 1u : 0u);
    const uint32_t v = HAVE_REC ? jd_pick(r0, r1, r2, r3, slot & 7u)
                                : (uint32_t)G.jd[act ? (size_t)((__umul24((uint32_t)cpx, (uint32_t)G.NS) + (uint32_t)cpy) * 8u + slot) : (size_t)0];
    if (ecv != nullptr) *ecv = tab[node_on ? n_slot : 0u];
    // (pure ALU while the loads are in flight: where the goal sits relative to this ray)
    const int ax = dx > 0 ? gpx - cpx : cpx - gpx, ay = dy > 0 ? gpy - cpy : cpy - gpy;  // steps to the goal's column / row along the ray (dx, dy != 0)
    const bool gline = diag ? (ax == ay) : (alongY ? gpx == cpx : gpy == cpy);
    const int kg = alongY ? ay : ax;  // steps to the goal if it lies on the ray's line
    PF(3);
    const int k = act ? (int)(v & JD_K) : 0;
    const bool jp = (v & JD_J) != 0u;
    const bool goal_on = act && gline && kg >= 1 && kg <= k;
    bool has = act && (goal_on ? (kg < k ? true : jp) : jp);
    int kres = goal_on ? kg : k;
    PF(4);
    {
        const bool need = diag && ((ax >= 1 && ax < kres) || (ay >= 1 && ay < kres));
        if (FX_RARE(__ballot(need) != 0ull)) {
            if (need) {
                const int k1 = min(ax, ay), k2 = max(ax, ay);
                const auto along = [](int c, int kk, int d) { return d > 0 ? c + kk : c - kk; };
                if (k1 >= 1 && k1 < kres && scan_two(G, along(cpx, k1, dx), along(cpy, k1, dy), dx, dy, gpx, gpy)) {
                    has = true;
                    kres = k1;
                } else if (k2 != k1 && k2 >= 1 && k2 < kres && scan_two(G, along(cpx, k2, dx), along(cpy, k2, dy), dx, dy, gpx, gpy)) {
                    has = true;
                    kres = k2;
                }
            }
            RECONV();
        }
    }
    const int jxp = dx == 0 ? cpx : (dx > 0 ? cpx + kres : cpx - kres);
    const int jyp = dy == 0 ? cpy : (dy > 0 ? cpy + kres : cpy - kres);
    *ocellj = has ? (((uint32_t)(jxp - 1) << 13) | (uint32_t)(jyp - 1)) : 0u;
    *ojci = 0xFFFFu;
    *ohas = has;
    if (okres != nullptr) *okres = act ? kres : 0;  // steps to the cell that ended the ray (the jump point, or what stopped it)
    PF(5);
}

// The read set of a ray that was answered by its jump-distance record: the cells the stepping form (expand_steps, the
// reference's loop) reads on the way to the same answer -- kres steps, up to and including the cell that ended the ray.
// A straight ray: that span of its scan line.  A diagonal ray: every cell it steps on, with the reach classes of the
// cell's info (the tiles its two straight sub-jumps scanned).  The record itself depends on nothing else up to there;
// what lies behind the ending cell (a goal or a sub-jump onto the goal ended the ray early) does not change the answer.
// The cell infos are independent loads, four per round: no chain of round trips as in the stepping form.
template <class MID>
__device__ __forceinline__ void rs_mark_ray(const GridDev& G, const MID& S, int cpx, int cpy, const uint32_t code, int kres) {
    const bool act = code != DIR_NONE && kres >= 1;
    const int dx = (int)(code >> 2) - 1, dy = (int)(code & 3u) - 1;
    const bool diag = act && dx != 0 && dy != 0;
    if (act && !diag) {
        const bool alongY = (dx == 0);
        const int p0 = alongY ? cpy + dy : cpx + dx, sgn = alongY ? dy : dx;
        rs_mark_scan(S, G.tsh, alongY, alongY ? cpx : cpy, p0, p0 + sgn * (kres - 1));
    }
    RECONV();
    int i = 1;
    while (__ballot(diag && i <= kres) != 0ull) {
        uint32_t m[4];
        int xs[4], ys[4];
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const int ii = min(i + u, kres);
            xs[u] = cpx + ii * dx;
            ys[u] = cpy + ii * dy;
            m[u] = G.ci[diag ? (size_t)(__umul24((uint32_t)xs[u], (uint32_t)G.NS) + (uint32_t)ys[u]) : (size_t)0];
        }
#pragma unroll
        for (int u = 0; u < 4; u++) {
            if (diag && i + u <= kres) rs_mark_cell(S, G.tsh, xs[u], ys[u], m[u]);
            RECONV();
        }
        i += 4;
    }
}

template <bool HAVE_REC>
__device__ __forceinline__ void expand_batch(const GridDev& G, uint32_t r0, uint32_t r1, uint32_t r2, uint32_t r3, int cpx, int cpy, const uint32_t code,
                                             bool node_on, int gpx, int gpy, bool* ohas, uint32_t* ocellj, uint32_t* ojci, const TEnt* __restrict__ tab,
                                             uint32_t n_slot, TEnt* ecv, int* okres PF_PARAMS) {
    if (okres != nullptr) *okres = 0;
    // (read sets: the caller marks the cells of the ray with rs_mark_ray, behind its next loads)
    expand_jd<HAVE_REC>(G, r0, r1, r2, r3, cpx, cpy, code, node_on, gpx, gpy, ohas, ocellj, ojci, tab, n_slot, ecv, okres PF_ARGS);
}

// The whole of jps1.method (jps1.py:183-230) for one query on one wavefront.
// Returns the result code; *res_cost is gscore[goal].
template <int HC, bool TRK, bool DIRECT, bool MG, class MID>
__device__ __forceinline__ int32_t search_one(const SearchArgs& A, const GridDev& Gq, const uint32_t q, const int sx, const int sy, const int gx,
                              const int gy, const MID& S, TEnt* __restrict__ tab, FarEnt* __restrict__ far,
                              const uint32_t gen, double* res_cost, unsigned long long* cnt4) {
    // The map pointers, the table pointer and the scan-line stride are used in per-lane address arithmetic only, a
    // dozen times per iteration.  Held in SGPRs they were spilled (the kernel runs at the scalar-register limit) and
    // re-read with v_readlane before every use; kept in vector registers on purpose they are plain operands.
    GridDev G = Gq;  // (A.G, or the query's slot: k_search<.., .., .., true>)
    {
        uint64_t vbm = (uint64_t)G.bm, vci = (uint64_t)G.ci, vtab = (uint64_t)tab, vjd = (uint64_t)G.jd;
        int vwords = G.WORDS;
        asm volatile("" : "+v"(vbm), "+v"(vci), "+v"(vtab), "+v"(vwords), "+v"(vjd));
        G.jd = (const uint16_t*)reinterpret_cast<__attribute__((address_space(1))) const uint16_t*>(vjd);
        // (through address-space-1 pointers: a pointer made from an integer is generic, and every access through it
        // a flat_load / flat_store)
        G.bm = (const BmWord*)reinterpret_cast<__attribute__((address_space(1))) const BmWord*>(vbm);
        G.ci = (const uint16_t*)reinterpret_cast<__attribute__((address_space(1))) const uint16_t*>(vci);
        G.WORDS = vwords;
        tab = (TEnt*)reinterpret_cast<__attribute__((address_space(1))) TEnt*>(vtab);
    }
    const int lane0 = threadIdx.x & 63;
    // On hashed tables (grids of more than 2^20 cells: every read is an HBM request, and requests are what the chip runs out
    // of) the node's lane reads the whole jump-distance record at the lane deal -- the neighbour byte comes with it, no cell
    // info is read for any successor.  Measured on both kinds: config 3 12.4 k -> 13.4 k plans/s; on the cell-indexed
    // tables of config 2 the read in front of the table lookup is a dependent wait the lone queries feel (62.1 -> 63.6 ms,
    // c2 145 k -> 141 k), so there the successor's cell info keeps riding along with its probe.
    constexpr bool JD2 = !DIRECT && !TRK;
    constexpr bool NOSLOT = MID::SLOTLESS;
    static_assert(!NOSLOT || DIRECT, "a node's slot follows from its cell on cell-indexed tables only");
    constexpr int HZ_LOG2 = MID::HZ_LOG2, HZ_SIZE = MID::HZ_SIZE;  // (this instantiation's detector)
    const uint32_t nbk = A.nbuckets;
    constexpr bool R2_ON = DIRECT;  // the second round (section 3.1b): on the cell-indexed tables, tracked searches included
    constexpr int KCAP_MIN2 = R2_ON ? 16 : 8;  // smallest batch of the Euclidean-key rule below
    // (a table indexed by the cell cannot fill up)
    const uint32_t tab_limit = DIRECT ? ~0u : A.tab_usable;
    const uint32_t dly = A.direct_ly;
    // where the probe of a cell starts: its own slot (DIRECT), else its bucket
    const auto probe_at = [&](uint32_t cell) -> uint32_t {
        // (hashed: Fibonacci hash, the product's high bits scaled to the bucket count -- a shift when that is a power of two)
        return DIRECT ? (((cell >> 13) << dly) | (cell & 0x1FFFu)) : __umulhi(cell * 0x9E3779B1u, nbk);
    };
    const int gpx = gx + 1, gpy = gy + 1;
    const uint32_t kg = gen_key_bits(gen), pg = gen_par_bits(gen);
    // loop-carried bookkeeping, vector-held (see vheld): result code, pops, pushes, "leave the loop"
    uint32_t res_len = vheld(0u), pops = vheld(0u), pushes = vheld(0u);  // (res_len != 0: the search is over)
    const uint32_t max_pops = (uint32_t)(A.max_pops < 0xFFFFFF00ull ? A.max_pops : 0xFFFFFF00ull);

    // ---- init: gscore = {start: 0}; heappush(f(start), start)   jps1.py:185-192
    OpenList Q;
    Q.r_n = 1;
    Q.m_n = 0;
    Q.far_n = 0;
    Q.farb_n = 0;
    Q.T2hi = (uint32_t)(F_INF >> 32);  // no far band yet: everything that goes to the far tier goes to its near band
    Q.Rbits = F_INF;
    Q.Rx = 0;
    Q.Tbits = F_INF;
    Q.Tx = 0;
    Q.dxs = 0;
    Q.delta = (HC == 1) ? 20.0 : 2.0;
    Q.hshift = 0;
    Q.cur0 = 0;
    Q.fail = 0;
    Q.banded = A.banded;
    if (lane0 < NBANDS) S.w->bcnt[lane0] = 0u;
    RECONV();
    uint32_t tcount = vheld(1u);
    RTier R;
    {
        const uint32_t cell = ((uint32_t)sx << 13) | (uint32_t)sy;
        const uint32_t slot = probe_at(cell) * (DIRECT ? 1u : (uint32_t)BUCKET);
        const uint32_t sci = G.ci[(size_t)(sx + 1) * G.NS + (sy + 1)];
        if (TRK) {  // the start's cell info and the goal's occupancy (read by run_query) are part of the read set
            if (lane0 == 0) {
                rs_mark_cell(S, G.tsh, sx + 1, sy + 1, sci);
                rs_mark_cell(S, G.tsh, gx + 1, gy + 1, 0u);
            }
            RECONV();
        }
        if (lane0 == 0) {
            TEnt e;
            e.g = 0.0;
            e.key = cell | (PD_NONE << 26) | kg;
            e.par = PAR_NONE | pg;
            tab[slot] = e;
        }
        RECONV();
        const bool me = lane0 == 0;
        R.f = me ? (uint64_t)__double_as_longlong(heuristic<HC>(sx, sy, gx, gy)) : ~0ull;
        R.x = me ? ((cell << 4) | PD_NONE) : ~0u;
        R.s = me ? slot : 0u;
        R.c = me ? sci : 0u;
    }

    PF_DECL;
    int kcap = KN;  // batch size the next iteration may try
#ifdef FXJPS_PROF
    unsigned long long pf_batches = 0, pf_popped = 0, pf_general = 0;
#endif
    while (rfl(res_len) == 0u) {
        // The open-list state and the counters are wave-uniform by construction; saying so at the loop head keeps
        // the compiler's divergence analysis from dragging them (and every branch on them) into VGPRs / exec masks.
        open_uniform(Q);
        // The lane number is made opaque once per iteration: otherwise every lane-class predicate (t == 0,
        // mynode == i, lane == 0 ...) is hoisted out of the loop as a 64-bit mask in two SGPRs, a dozen of them
        // live across the whole loop, and the scalar registers spill into VGPR lanes.
        int lane = lane0;
        asm volatile("" : "+v"(lane));
        const int t = lane & (SL - 1);
        const int gsh = lane;  // (this lane's ray: one lane per ray)
        kcap = rfli(kcap);
        constexpr int kmax = KN;
        // ================= pop the smallest (f, x, y)           jps1.py:198
        int nb = 0;
        PF(9);
        // (the refill code gets the plain lane number: what it derives from it is loop-invariant and stays in VGPRs
        // instead of being recomputed at every loop head)
        // (the read-set instantiations on hashed tables have no registers to spare for those: there the values are
        // derived again where they are used -- held, two of them went to scratch)
        if (!open_fill<HC == 2 && !DIRECT && !TRK && FXJPS_BANDED != 0, JD2>(A, Gq, Q, R, S, far, (TRK && !DIRECT) ? lane : lane0)) break;  // (0, t): jps1.py:230
        if (FX_RARE(Q.fail != 0u)) {  // a region of the far band's ring is full: the large pool takes the query
            res_len = (uint32_t)QI_FAR_FULL;
            break;
        }
        PF(8);
        // R is sorted: the batch is its first nb lanes -- the next pop and nb-1 speculative ones (all below
        // everything in M and the far tier).  With the octile heuristic (hchoice 1) equal f values are the rule and
        // make most runner-ups invalid: there the batch is no larger than what recent batches managed to commit,
        // plus one.  Nothing leaves R before the commit knows how many of the nodes really were the next pops; until
        // then the wave-uniform key of node j is a read of lane j.
        nb = min(min(kcap, kmax), Q.r_n);
        nb = rfli(nb);
        // ---- the lanes of the batch.  Lane j < nb holds node j.  It looks up the directions nodeNeighbours leaves
        // its node (jps1.py:49-93: the table entry of (parent direction, neighbour byte); the directions come first,
        // DIR_NONE fills the rest), asks for one lane per direction, and a prefix sum over the row deals the lanes out;
        // the batch ends before the first node whose rays do not fit.
        const bool inb0 = lane < nb;
        // On the jump-distance records the node's lane reads its node's 16-byte record here: the eight distances its rays
        // will pick from, and -- in the spare bits -- the neighbour byte nodeNeighbours wants.  One memory round trip in
        // front of the table lookup instead of one behind it; no cell info travels with the open-list entries and none is
        // read for the successors (one request per FOUND successor less).
        uint32_t rj0 = 0u, rj1 = 0u, rj2 = 0u, rj3 = 0u;
        uint32_t nb8_j = R.c & 0xFFu;
        if (JD2) {
            const uint32_t rx = (R.x >> 17) + 1u, ry = ((R.x >> 4) & 0x1FFFu) + 1u;
            const uint4 t4 = *reinterpret_cast<const uint4*>(G.jd + (inb0 ? (size_t)(__umul24(rx, (uint32_t)G.NS) + ry) * 8u : (size_t)0));
            rj0 = t4.x;
            rj1 = t4.y;
            rj2 = t4.z;
            rj3 = t4.w;
            nb8_j = jd_nb8(rj0, rj1);
        }
        const uint32_t my_codes = S.dirlut[inb0 ? (R.x & 0xFu) * 256u + nb8_j : 0u];
        uint32_t fnib = my_codes & (my_codes >> 1);  // bit 4k of fnib: nibble k is DIR_NONE
        fnib &= fnib >> 2;
        fnib &= 0x11111111u;
        const uint32_t nrays = fnib != 0u ? ((uint32_t)__builtin_ctz(fnib) >> 2) : 8u;
        const uint32_t need = inb0 ? max(nrays, 1u) : 0u;  // (a node without a ray still has to be closed by a lane)
        uint32_t incl = row_scan_add(need);
        if (KN > 16) incl += lane >= 16 ? lane_get(incl, 15) : 0u;  // (the second row continues the first)
        const bool fits = inb0 && incl <= (uint32_t)WAVE;  // (a prefix of the row: incl grows along it; node 0 always fits)
        DBG_COUNT(S, 34, nb - __popcll(__ballot(fits)));  // nodes that found no lanes
        nb = __popcll(__ballot(fits));
        nb = rfli(nb);
        const uint32_t lstart = incl - need;  // first lane of my node's rays
        // which lanes start a node: bit lstart of a 64-bit mask, ORed over the row
        const uint64_t hb = fits ? (1ull << lstart) : 0ull;
        const uint32_t hlo = row_scan_or((uint32_t)hb), hhi = row_scan_or((uint32_t)(hb >> 32));
        const uint64_t heads = (((uint64_t)lane_get(hhi, 15) << 32) | (uint64_t)lane_get(hlo, 15)) |
                               (KN > 16 ? (((uint64_t)lane_get(hhi, 31) << 32) | (uint64_t)lane_get(hlo, 31)) : 0ull);
        const int nlanes = (int)lane_get(incl, nb - 1);  // lanes in use
        DBG_COUNT(S, 33, nlanes);
        // A node whose cell also sits earlier in the batch is the stale duplicate of a better entry (pushed later, it
        // sorts before the old one): by the time it is popped the earlier node has closed the cell (SURVEY Q3).  One
        // row: 15 comparisons by DPP.  Two rows: same cell, same table slot -- every node leaves its lane number, by
        // atomic minimum, in two LDS cells picked by independent hashes of its slot (the detector of the commit, at
        // rest here); a node beaten in both asks the winner for its slot, and the rare one whose winner holds another
        // slot asks all.  (Measured with 16 nodes: the LDS form costs config 2 3 %, two more round trips in front of
        // the map loads.)
        bool dup_j = row_dup_before(R.x >> 4);
        if (KN > 16 && nb > 16) {  // (wide batches only: the second row against the first)
            const bool x = row_dup_cross(R.x >> 4, lane);
            dup_j = dup_j || (x && lane >= 16 && lane < 32);
        }
#ifdef FXJPS_PROF
        { const uint64_t dm_ = __ballot(dup_j && fits); DBG_COUNT(S, 45, __popcll(dm_)); DBG_COUNT(S, 46, dm_ != 0ull ? 1 : 0); }
#endif
        // my node = the number of nodes that start at or before this lane, minus one (lane 0 starts node 0)
        const int mynode = (int)rank_below(heads >> 1);
        const uint32_t pk_j = (JD2 ? nb8_j : (R.c & 0xFFFFu)) | (lstart << 16) | (dup_j ? 1u << 22 : 0u);
#ifdef FXJPS_PROF
        pf_batches++;
        pf_popped += (unsigned long long)nb;
#endif
        // the lanes of node i take its packed cell, table slot, cell info and directions from lane i ("my node")
        // (the slotless layout hands over three values: the slot is the cell's, derived here)
        const uint32_t n_xyd = lane_pull(R.x, (uint32_t)mynode), n_slot = NOSLOT ? probe_at(n_xyd >> 4) : lane_pull(R.s, (uint32_t)mynode),
                       n_pk = lane_pull(pk_j, (uint32_t)mynode), n_codes = lane_pull(my_codes, (uint32_t)mynode);
        uint32_t nr0 = 0u, nr1 = 0u, nr2 = 0u, nr3 = 0u;  // my node's jump-distance record
        if (JD2) {
            nr0 = lane_pull(rj0, (uint32_t)mynode);
            nr1 = lane_pull(rj1, (uint32_t)mynode);
            nr2 = lane_pull(rj2, (uint32_t)mynode);
            nr3 = lane_pull(rj3, (uint32_t)mynode);
        }
        PF(0);
        const bool node_on = lane < nlanes;
        const uint32_t n_ci = n_pk & 0xFFFFu;
        const uint32_t ray = ((uint32_t)lane - ((n_pk >> 16) & 63u)) & 7u;   // which of its node's directions this lane follows
        const bool dupnode = ((n_pk >> 22) & 1u) != 0u;
        const int lstart_m = (int)((n_pk >> 16) & 63u);  // first lane of my node
        const uint32_t code = node_on ? ((n_codes >> (4u * ray)) & 0xFu) : DIR_NONE;
        const int cx = (int)(n_xyd >> 17), cy = (int)((n_xyd >> 4) & 0x1FFFu);
        // The stores of the previous batch have had the whole pop phase to land.  Saying that they have lets the
        // waits below count loads (vmcnt(n)) instead of draining everything (loads and stores share one counter).
        __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0)
#ifdef FXJPS_PHASE_S
        PF(10);
#endif

        // ================= identifySuccessors                 jps1.py:166-179
        // The pruning direction comes from came_from[c] (jps1.py:57,168).  The open-list entry carries the
        // direction it was pushed with; the table is the truth (a later, better push may have replaced
        // the parent): a node whose table direction differs is expanded again on its own.
        const uint32_t pd_e = n_xyd & 0xFu;
        uint32_t cellj, jci;
        bool has;
        PF(0);
        TEnt ecv;  // gscore / came_from / closed flag of my node: needed only after the jumps
        ecv.g = 0.0;
        ecv.key = 0;
        ecv.par = 0;
        int kres = 0;
        expand_batch<JD2>(G, nr0, nr1, nr2, nr3, cx + 1, cy + 1, code, node_on, gpx, gpy, &has, &cellj, &jci, tab, n_slot, &ecv, TRK ? &kres : nullptr PF_ARGS);
        PF(5);

        // ---- probe the visited table for every successor of every node (one round trip for all)
        const int jx = (int)(cellj >> 13), jy = (int)(cellj & 0x1FFFu);
        const uint32_t newkey = cellj | (code << 26) | kg;
        uint32_t b = probe_at(cellj);
        const bool need_ci = !JD2 && has && t == 0 && jci == 0xFFFFu;  // (on the records nobody needs a successor's cell info)
        // (rides along with the first probe; every lane loads -- under `if (need_ci)` the compiler waits for the value
        // inside the block, an L2 round trip before the probe is even requested)
        const size_t lci_at = (size_t)(__umul24((uint32_t)(jx + 1), (uint32_t)G.NS) + (uint32_t)(jy + 1));
        const uint32_t lci = JD2 ? 0u : (uint32_t)G.ci[need_ci ? lci_at : (size_t)0];
        Probe pe;  // my slots of my ray's bucket
        probe_load<DIRECT>(pe, tab, b, t, has);
        if (TRK) rs_mark_ray(G, S, cx + 1, cy + 1, code, kres);  // (its cell-info loads ride behind the probes)

        // ================= commit, fast form: every node of the batch at once     jps1.py:210-228
        // Valid when the relaxations of the batch do not interact: no goal, no changed parent, no full
        // bucket, no two rays on the same cell or the same empty slot.  Anything else (a few % of the
        // batches) takes the node-by-node form below, which starts from the same untouched state.
        bool done_fast = false;
        // ONE call site of open_insert for the vectorised commit and the two exits of the general form that insert (its code
        // -- R and M splits inlined -- is 1 250 instructions; three copies of it were 15 KB of the kernel's 61).  On the
        // cell-indexed tables only (round 6: c2 + 1.8 %): the same on hashed tables costs config 3 1.6 - 2.4 %.
        constexpr bool ONE_INS = DIRECT;
        bool xi_do = false, xi_w = false;
        int xi_drop = 0;
        uint64_t xi_f = 0ull;
        uint32_t xi_x = 0u, xi_s = 0u, xi_c = 0u;
        {
            // A node whose cell is already closed is a stale duplicate: popping it is a no-op (SURVEY Q3).  So is a
            // node whose cell also sits earlier in this batch (dupnode, found when the lanes were dealt out).
            const bool closed_m = node_on && ((ecv.key & KEY_CLOSED) != 0 || dupnode);
            const bool isgoal_m = node_on && cx == gx && cy == gy;
            const bool pdmis_m = node_on && !closed_m && (((ecv.key >> 26) & 0xFu) != pd_e);
            // ---- everything that does not need the table lines is done while they are in flight (a random HBM
            // access each): segment length and heuristic, the relaxing rays, where a push of each ray would end the
            // valid prefix, and which rays share a bucket.
            const double seg = seg_len<HC>(cx, cy, jx, jy);          // :221
            const double hj = heuristic<HC>(jx, jy, gx, gy);         // :227
            const bool rel = has && !closed_m;
            const double tg = ecv.g + seg;                                       // :221
            const uint64_t fb = (uint64_t)__double_as_longlong(tg + hj);         // :227
            // (node j stops being the next pop when an earlier node pushes a key <= its key.  The keys of the batch
            // are sorted, so the nodes below my push key are a prefix of the batch: the first node at or above it,
            // and behind my own, is where the valid prefix ends if this ray pushes.)
            // Usually every push key lies above the whole batch (the successors of the 8 smallest open nodes are
            // seldom smaller than the 8th): then all nb nodes are below it and the count is not needed.
            uint32_t below = (uint32_t)nb;
            const uint64_t fmax = ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(R.f >> 32), nb - 1) << 32) |
                                  (uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)R.f, nb - 1);
            {
                // (the few rays with a key inside the batch, one after the other: the lanes of R compare their key with
                // the ray's, a ballot counts the nodes below it)
                uint64_t im = __ballot(rel & (fb <= fmax));
                DBG_COUNT(S, 59, __popcll(im));  // rays whose key lies inside the batch (trips of the loop below)
                const bool nodelane = lane < nb;
                const uint32_t rcell = R.x >> 4;
                while (im != 0ull) {
                    const int src = (int)__builtin_ctzll(im);
                    im &= im - 1ull;
                    const uint64_t pf = lane_get64(fb, src);
                    const uint32_t pc = lane_get(cellj, src);
                    const uint32_t cntb = (uint32_t)__popcll(__ballot(nodelane & ((R.f < pf) | ((R.f == pf) & (rcell < pc)))));
                    below = lane == src ? cntb : below;
                }
            }
            const uint32_t first_bad = max(below, (uint32_t)mynode + 1u);
            // Two rays that touch the same table slot (the same cell reached from two nodes, or the same empty slot)
            // cannot be relaxed in one pass: the prefix ends before the node of the later one.  Same slot implies
            // same bucket, so the test is on the bucket (known before the lines arrive; two different cells of one
            // batch in one bucket are a one-in-ten-thousand event).  Every relaxing ray leaves its lane number, by
            // atomic minimum, in two LDS cells picked by independent hashes of its bucket, each in its own half of
            // the array; it is held back only when a smaller lane beat it in both.
            int nvalid_hz = KN;
            // A ray held back by the detector is looked at again, exactly.  (1) Does a smaller lane really share its
            // bucket (the two cells may have been beaten by rays of other buckets)?  If not, it is not held back.
            // (2) If exactly one does, and both rays head for the same cell -- two nodes that see the same jump point,
            // two thirds of the real cases -- the pair is relaxed in this pass all the same, the later ray (pair2)
            // deciding on what the earlier one (its g: tgA) leaves behind; see below, behind the probe.
            bool pair2 = false;
            double tgA = 0.0;
            {
                const bool rl = rel && t == 0;
                if (__popcll(__ballot(rl)) > 1) {
                    const uint32_t h1 = (b * 0x9E3779B1u) >> (33 - HZ_LOG2);
                    const uint32_t h2 = (HZ_SIZE / 2) + ((b * 0x85EBCA6Bu + 0x27D4EB2Fu) >> (33 - HZ_LOG2));
                    if (rl) {
                        __hip_atomic_fetch_min(&S.w->hz[h1], (uint32_t)lane, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
                        __hip_atomic_fetch_min(&S.w->hz[h2], (uint32_t)lane, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
                    }
                    uint32_t first = (uint32_t)lane;
                    if (rl) {
                        const uint32_t f1 = S.w->hz[h1], f2 = S.w->hz[h2];
                        first = (f1 != (uint32_t)lane && f2 != (uint32_t)lane) ? f1 : (uint32_t)lane;
                        S.w->hz[h1] = ~0u;
                        S.w->hz[h2] = ~0u;
                    }
                    RECONV();
                    const bool held = rl && first != (uint32_t)lane;
                    const uint64_t lm = __ballot(held);
                    if (FX_RARE(lm != 0ull)) {
                        DBG_COUNT(S, 39, 1);
                        // the smallest lane that shares my bucket, exactly: the ray that beat me if it does (every
                        // ray of my bucket uses my two cells, so no smaller one can share it), else by asking
                        const uint32_t ob = lane_pull(b, first & 63u);
                        bool real = held && ob == b;
                        uint32_t alane = first & 63u;
                        uint64_t um = __ballot(held && !real);
                        while (um != 0ull) {
                            const int src = (int)__builtin_ctzll(um);
                            um &= um - 1ull;
                            const uint32_t bs = lane_get(b, src);
                            const uint64_t gm = __ballot(rl && b == bs) & ((1ull << src) - 1ull);
                            const bool me = lane == src;
                            real = (me && gm != 0ull) ? true : real;
                            alane = (me && gm != 0ull) ? (uint32_t)__builtin_ctzll(gm | (1ull << 63)) : alane;
                        }
                        // pairs: the ray at alane is the only other ray of my bucket, and it heads for my cell
                        const uint32_t oc = lane_pull(cellj, alane);
                        const uint32_t tglo = lane_pull((uint32_t)(uint64_t)__double_as_longlong(tg), alane),
                                       tghi = lane_pull((uint32_t)((uint64_t)__double_as_longlong(tg) >> 32), alane);
                        bool unres = real;
                        uint64_t rm_ = __ballot(real);
                        while (rm_ != 0ull) {
                            const int src = (int)__builtin_ctzll(rm_);
                            rm_ &= rm_ - 1ull;
                            const uint32_t bs = lane_get(b, src);
                            const bool alone = __popcll(__ballot(rl && b == bs)) == 2;
                            const bool me = lane == src;
                            if (me && alone && oc == cellj) {
                                unres = false;
                                pair2 = true;
                            }
                            RECONV();
                        }
                        tgA = __longlong_as_double((long long)(((uint64_t)tghi << 32) | (uint64_t)tglo));
                        DBG_COUNT(S, 35, __popcll(lm));
                        DBG_COUNT(S, 36, __popcll(__ballot(real)));
                        DBG_COUNT(S, 37, __popcll(__ballot(pair2)));
                        const uint64_t xm = __ballot(unres);
                        if (xm != 0ull) {
                            DBG_COUNT(S, 38, 1);
                            nvalid_hz = (int)lane_get((uint32_t)mynode, (int)__builtin_ctzll(xm));  // lanes are ordered by node
                        }
                    }
                }
            }
            DBG_COUNT(S, 31, nb - min(nb, nvalid_hz));  // nodes behind a shared bucket
#ifdef FXJPS_PROF
            // (diagnostics: would the intruder of the second round be known before the table lines arrive?  The cut if
            // every relaxing ray pushes, and the one ray that makes it, if it is one and its cell info is known)
            int pf_pred = -1;
            {
                const int np = min(min(nb, nvalid_hz), (int)wave_umin32((rel && t == 0) ? first_bad : (uint32_t)KN));
                const uint64_t pm_ = __ballot(rel && t == 0 && first_bad == (uint32_t)np);
                if (np < nb && __popcll(pm_) == 1) {
                    const int l_ = (int)__builtin_ctzll(pm_);
                    DBG_COUNT(S, 54, 1);
                    if (lane_get(jci, l_) != 0xFFFFu) {
                        DBG_COUNT(S, 55, 1);
                        pf_pred = l_;
                    }
                }
            }
#endif
            __builtin_amdgcn_sched_barrier(0);
#ifdef FXJPS_PHASE_S
            PF(11);
#endif
            // ---- the table lines
            bool found, has_empty;
            uint32_t jslot, jkey;
            double jg;
            probe_eval<DIRECT>(pe, has, cellj, b, gen, &found, &has_empty, &jslot, &jg, &jkey);
            PF(1);
            const bool full = rel && !found && !has_empty;
            bool push = rel && (found ? (!(jkey & KEY_CLOSED) && tg < jg) : true);    // :218, :223-224
            if (FX_RARE(__ballot(pair2) != 0ull)) {
                // The later ray of a pair: its partner (an earlier node, same cell, same table lines) relaxes first.
                // If the partner pushes, the cell then holds the partner's g (:226) and I push only below that (:223);
                // if not, nothing has changed.  (A cell nobody has seen is always pushed by the partner.)
                const bool pushA = found ? (!(jkey & KEY_CLOSED) && tgA < jg) : true;
                if (pair2) push = rel && (pushA ? tg < tgA : push);
                RECONV();
            }
            // The successor may be an earlier node of this batch: closed by the time my node relaxes (:218), though the
            // table does not say so yet.  Its newest open-list entry has the key jg + hj, and the entries of the batch
            // are the smallest of the open list: only a successor whose key lies within the batch can be one of its
            // nodes (with a consistent heuristic a better path to such a node is a matter of rounding).  My node then
            // waits for the next iteration, where the table knows.
            const bool selfq = push && found && mynode > 0 && (uint64_t)__double_as_longlong(jg + hj) <= fmax;
            const bool pl = push && t == 0;
            // how many nodes of the batch are really the next pops
            int nvalid = min(min(nb, nvalid_hz), (int)wave_umin32(pl ? first_bad : (uint32_t)KN));
            DBG_COUNT(S, 24, nb - nvalid);  // nodes lost to the key rule or a shared bucket
            PF(6);
            // Anything else the vectorised form cannot order ends the committed prefix at that node: the goal, a
            // changed parent direction, a full bucket, a successor that may be a node of the batch.
            int pn_all = KN;  // first node that ends the prefix for one of these reasons
            {
                const uint64_t pm = __ballot(isgoal_m || pdmis_m || full || selfq);
                if (pm != 0ull) {
                    const int pn = (int)lane_get((uint32_t)mynode, (int)__builtin_ctzll(pm));  // lanes are ordered by node
                    DBG_COUNT(S, 25, pn < nvalid ? nvalid - pn : 0);  // ... to the goal / a changed parent / a full bucket
                    nvalid = pn < nvalid ? pn : nvalid;
                    pn_all = pn;
                }
            }
            nvalid = rfli(nvalid);
            const bool cm = mynode < nvalid;  // my node is committed in this iteration
            PF(7);
            if (FX_USUAL(nvalid > 0)) {
                done_fast = true;
                // The next batch is no larger than what this one makes likely: the probes of the nodes that turn out not
                // to be the next pops are loads the iteration waits for all the same.  Octile keys (equal f is the rule):
                // what was committed, plus one; Euclidean keys on hashed tables: twice what was committed, at least 8
                // (config 3: always 16 costs 7 %, at least 12 3 %); on cell-indexed tables, with the second round behind the
                // first, always 16 (config 2 + 0.5 %, config-5 frames + 1.3 %, a 125 000-query batch the same).
                const int kcap0 = kcap;
                if (HC == 1)
                    kcap = nvalid == nb ? min(kcap + 2, kmax) : (2 * nvalid < nb ? nvalid + 1 : kcap);
                else
                    kcap = nvalid == nb ? min(kcap + 4, kmax) : max(min(kcap, 2 * nvalid), min(KCAP_MIN2, kmax));
                pops += (uint32_t)nvalid;
                if (FX_RARE(rfl(pops) > max_pops)) {
                    res_len = (uint32_t)QI_WATCHDOG;
                }
                const bool w = pl && cm;
                // ================= second round: through ONE intruding successor                  (round 3)
                // The prefix usually ends because a committed node pushed a key that sorts in front of the next node of
                // the batch: the reference pops that successor s next, THEN the rest of the batch.  When s is the only
                // such push (it is then the smallest key of the whole open list) the iteration goes on: s is expanded
                // and relaxed on lanes the batch left idle (it never enters the open list: pushed and popped within the
                // iteration), and the nodes behind the cut are committed from the expansions and table lines this
                // iteration already has -- up to the next push that sorts inside the batch, and not past a node that
                // s could have touched: a node or successor cell that is s or one of s's successors ends the prefix
                // (conservative: equal cells, whatever the relaxation decided).  The launches of config 2 and of the
                // config-5 frames end with queries whose successors keep landing inside the batch (5.8 nodes per
                // iteration): replaying the reference's pop sequence of such a query says 22.6 k -> 13.9 k iterations.
                // All of s's loads are issued BEFORE any table store of the iteration (loads and stores retire through
                // one in-order counter: a load behind a store waits for the store).  What the first round is about to
                // write into a cell s relaxes is taken from the registers instead: a node it closes, a g it pushes.
                int ndrop = nvalid;          // nodes of the batch that leave R
                bool w_ins = w;              // lanes whose entry goes into the open list
                uint64_t ins_f = fb;
                uint32_t ins_x = (cellj << 4) | code, ins_s = jslot, ins_c = JD2 ? 0u : (need_ci ? lci : jci);
                bool r2 = false, on2 = false, push2 = false;
                int Ls = 0;
                uint32_t s_slot = 0, s_key = 0, code2 = DIR_NONE, cellj2 = 0, slot2 = 0, below2 = (uint32_t)nb, cut = (uint32_t)nb;
                double tg2 = 0.0;
#ifdef FXJPS_HWID  // diagnostics (tools/r2_stats.py): what ends the first round's prefix
                const int nint = __popcll(__ballot(w && first_bad == (uint32_t)nvalid));
                if (DIRECT && !TRK && A.out_counters && lane == 0) {
                    atomicAdd(&A.out_counters[55], 1ull);
                    atomicAdd(&A.out_counters[nvalid >= nb ? 56 : (nvalid < nvalid_hz && nvalid < pn_all) ? (nint == 1 ? 57 : 58) : 59], 1ull);
                    atomicAdd(&A.out_counters[60], (unsigned long long)nb);
                    atomicAdd(&A.out_counters[61], (unsigned long long)nvalid);
                }
                RECONV();
#endif
                if (R2_ON && rfl(res_len) == 0u && nvalid < nb && nvalid < nvalid_hz && nvalid < pn_all &&
                    nlanes + 8 < WAVE) {  // (lane 63 stays free: its bit stands for s itself below)
                    const uint64_t im2 = __ballot(w && first_bad == (uint32_t)nvalid);  // the pushes that end the prefix here
                    if (__popcll(im2) == 1) {
                        Ls = (int)__builtin_ctzll(im2);
                        const uint32_t s_cell = lane_get(cellj, Ls), s_code = lane_get(code, Ls);
                        const uint32_t s_ci = JD2 ? 0u : (lane_get(need_ci ? lci : jci, Ls) & 0xFFFFu);
                        s_slot = lane_get(jslot, Ls);
                        s_key = lane_get(newkey, Ls);
                        const double s_g = __longlong_as_double((long long)lane_get64((uint64_t)__double_as_longlong(tg), Ls));
                        const int sx2 = (int)(s_cell >> 13), sy2 = (int)(s_cell & 0x1FFFu);
                        if (!(sx2 == gx && sy2 == gy)) {  // (the goal is popped by the general form)
                            r2 = true;
                            DBG_COUNT(S, 51, 1);
#ifdef FXJPS_PROF
                            if (lane_get(jci, Ls) != 0xFFFFu) DBG_COUNT(S, 53, 1);  // s hangs on a diagonal ray: its cell info was known early
                            if (pf_pred == Ls) DBG_COUNT(S, 56, 1);                  // ... and it was the predicted one
#endif
                            // ---- expand s on the idle lanes nlanes .. nlanes + 7 (jps1.py:166-179)
                            on2 = lane >= nlanes && lane < nlanes + 8;
                            // s's jump-distance record (every lane reads the same one): the whole of it -- one address for all
                            // lanes -- is requested here, beside the LDS lookup of its directions, instead of one u16 per lane
                            // behind it (round 6: query 9206 alone 59.4 -> 59.1 ms, c4shard + 1.5 %)
                            const uint4 t4 = *reinterpret_cast<const uint4*>(G.jd + (size_t)(__umul24((uint32_t)(sx2 + 1), (uint32_t)G.NS) + (uint32_t)(sy2 + 1)) * 8u);
                            const uint32_t rs0 = t4.x, rs1 = t4.y, rs2 = t4.z, rs3 = t4.w;
                            const uint32_t s_nb = JD2 ? jd_nb8(rs0, rs1) : s_ci & 0xFFu;
                            const uint32_t codes2 = S.dirlut[s_code * 256u + s_nb];
                            code2 = on2 ? ((codes2 >> (4u * (uint32_t)(lane - nlanes))) & 0xFu) : DIR_NONE;
                            bool has2;
                            uint32_t jci2;
                            int kres2 = 0;
                            expand_batch<true>(G, rs0, rs1, rs2, rs3, sx2 + 1, sy2 + 1, code2, on2, gpx, gpy, &has2, &cellj2, &jci2, tab, 0u, nullptr, TRK ? &kres2 : nullptr PF_ARGS);
                            has2 = has2 && on2;
                            const int jx2 = (int)(cellj2 >> 13), jy2 = (int)(cellj2 & 0x1FFFu);
                            const uint32_t b2 = probe_at(cellj2);
                            const bool need_ci2 = !JD2 && has2 && jci2 == 0xFFFFu;
                            const uint32_t lci2 = JD2 ? 0u : (uint32_t)G.ci[need_ci2 ? (size_t)(__umul24((uint32_t)(jx2 + 1), (uint32_t)G.NS) + (uint32_t)(jy2 + 1)) : (size_t)0];
                            Probe pe2;
                            probe_load<DIRECT>(pe2, tab, b2, 0, has2);
                            if (TRK) rs_mark_ray(G, S, sx2 + 1, sy2 + 1, code2, kres2);  // (s's rays belong to the read set like any node's)
                            tg2 = s_g + seg_len<HC>(sx2, sy2, jx2, jy2);                                                   // :221
                            const uint64_t fb2 = (uint64_t)__double_as_longlong(tg2 + heuristic<HC>(jx2, jy2, gx, gy));    // :227
                            // ---- which nodes behind the cut could s have touched, and what does the first round leave in
                            // the cells s relaxes?  (cells, before the lines arrive)
                            bool fw_closed = false, fw_hit = false;
                            double fw_g = 0.0;
                            {
                                const bool oldnode = lane >= nvalid && lane < nb;            // R lanes: the nodes not committed yet
                                const bool donenode = lane < nvalid;                          //          the nodes the first round closes
                                const bool oldray = node_on && has && mynode >= nvalid;       // the rays of the former
                                const uint32_t rcell2 = R.x >> 4;
                                uint64_t cm2 = __ballot(has2) | (1ull << 63);                 // s's successors, and (bit 63) s itself
                                // Mostly none of these cells is a node or a successor of this batch, and the loop below -- a
                                // trip of ~ 55 instructions per cell -- finds nothing.  So first a sieve through the (idle)
                                // collision detector: s and its successors leave a mark at the hash of their cell, every lane
                                // looks up the hash of its node's cell and of its ray's jump point.  No marks found: the loop
                                // is skipped.  (A mark found may be another cell with the same hash: the loop decides, exactly.
                                // s's own mark is written first, its successors' marks over it: a lane whose only business with
                                // s itself is none -- the nodes and pushes of the committed prefix, Ls's push of s among them --
                                // ignores a mark that still says "s".)
                                {
                                    const uint32_t hm = ((((lane == 63) ? s_cell : cellj2) * 0x9E3779B1u) >> (32 - HZ_LOG2));
                                    if (lane == 63) S.w->hz[hm] = 63u;
                                    RECONV();
                                    if (has2) S.w->hz[hm] = (uint32_t)lane;
                                    RECONV();
                                    const bool chk_n = lane < nb, chk_r = node_on && has;
                                    const uint32_t m_n = S.w->hz[chk_n ? ((rcell2 * 0x9E3779B1u) >> (32 - HZ_LOG2)) : 0u];
                                    const uint32_t m_r = S.w->hz[chk_r ? ((cellj * 0x9E3779B1u) >> (32 - HZ_LOG2)) : 0u];
                                    if (lane == 63 || has2) S.w->hz[hm] = ~0u;  // (at rest again before anybody else uses the detector)
                                    RECONV();
                                    const bool hit_n = chk_n && m_n != ~0u && (oldnode || m_n != 63u);
                                    const bool hit_r = chk_r && m_r != ~0u && (oldray || (w && m_r != 63u));
                                    if (__ballot(hit_n || hit_r) == 0ull) cm2 = 0ull;
                                    DBG_COUNT(S, 57, cm2 != 0ull ? 1 : 0);
                                }
                                DBG_COUNT(S, 48, __popcll(cm2));
                                while (cm2 != 0ull) {
                                    const int src = (int)__builtin_ctzll(cm2);
                                    cm2 &= cm2 - 1ull;
                                    const uint32_t c = src == 63 ? s_cell : lane_get(cellj2, src);
                                    const uint64_t hn = __ballot(oldnode && rcell2 == c);
                                    const uint64_t hr = __ballot(oldray && cellj == c);
                                    if (hn != 0ull) cut = min(cut, (uint32_t)__builtin_ctzll(hn));
                                    if (hr != 0ull) cut = min(cut, lane_get((uint32_t)mynode, (int)__builtin_ctzll(hr)));
                                    const uint64_t hc = __ballot(donenode && rcell2 == c);
                                    const uint64_t hw = __ballot(w && cellj == c);
                                    if (hw != 0ull) {  // (the later of two writers wrote last: pairs)
                                        const int hi = 63 - (int)__builtin_clzll(hw);
                                        const double g1 = __longlong_as_double((long long)lane_get64((uint64_t)__double_as_longlong(tg), hi));
                                        fw_g = lane == src ? g1 : fw_g;
                                        fw_hit = lane == src ? true : fw_hit;
                                    }
                                    fw_closed = (lane == src && hc != 0ull) ? true : fw_closed;
                                }
                                const uint64_t pp = __ballot(node_on && pair2 && mynode >= nvalid);
                                if (pp != 0ull) cut = min(cut, lane_get((uint32_t)mynode, (int)__builtin_ctzll(pp)));
                            }
                            // ---- where s's own pushes sort among the nodes of the batch
                            {
                                uint64_t im3 = __ballot(has2 & (fb2 <= fmax));
                                DBG_COUNT(S, 49, __popcll(im3));
                                const bool nodelane = lane < nb;
                                const uint32_t rcell2 = R.x >> 4;
                                while (im3 != 0ull) {
                                    const int src = (int)__builtin_ctzll(im3);
                                    im3 &= im3 - 1ull;
                                    const uint64_t pf = lane_get64(fb2, src);
                                    const uint32_t pc = lane_get(cellj2, src);
                                    const uint32_t cntb = (uint32_t)__popcll(__ballot(nodelane & ((R.f < pf) | ((R.f == pf) & (rcell2 < pc)))));
                                    below2 = lane == src ? cntb : below2;
                                }
                            }
                            // ---- s's table lines: relax its successors                               :215-228
                            bool found2, he2;
                            uint32_t jkey2;
                            double jg2;
                            probe_eval<DIRECT>(pe2, has2, cellj2, b2, gen, &found2, &he2, &slot2, &jg2, &jkey2);
                            const bool closed2 = fw_closed || (found2 && (jkey2 & KEY_CLOSED) != 0u);
                            found2 = found2 || fw_hit;
                            jg2 = fw_hit ? fw_g : jg2;
                            push2 = has2 && !closed2 && (found2 ? tg2 < jg2 : true);
                            ins_f = on2 ? fb2 : ins_f;
                            ins_x = on2 ? ((cellj2 << 4) | code2) : ins_x;
                            ins_s = on2 ? slot2 : ins_s;
                            ins_c = JD2 ? 0u : (on2 ? (need_ci2 ? lci2 : jci2) : ins_c);
                        }
                    }
                }
                // ---- the table stores of the first round
                if (node_on && cm && !closed_m && lane == lstart_m) tab[n_slot].key = ecv.key | KEY_CLOSED;  // :210
                RECONV();
                if (w && !pair2) {
                    TEnt e;
                    e.g = tg;
                    e.key = newkey;
                    e.par = n_slot | pg;
                    tab[jslot] = e;  // came_from / gscore, :225-226
                }
                RECONV();
                if (FX_RARE(__ballot(w && pair2) != 0ull)) {  // (a second store instruction: it lands behind the partner's)
                    if (w && pair2) {
                        TEnt e;
                        e.g = tg;
                        e.key = newkey;
                        e.par = n_slot | pg;
                        tab[jslot] = e;
                    }
                    RECONV();
                }
                tcount += (uint32_t)__popcll(__ballot(w && !found && !pair2));
                if (FX_RARE(rfl(tcount) > tab_limit)) {
                    res_len = (uint32_t)QI_TABLE_FULL;
                }
                const uint64_t pushm = __ballot(w);
                pushes += (uint32_t)__popcll(pushm);
                if (r2) {
                    // ---- ... of s, and of the nodes the second round commits behind it
                    if (lane == nlanes) tab[s_slot].key = s_key | KEY_CLOSED;                                              // :210
                    RECONV();
                    if (push2) {
                        TEnt e;
                        e.g = tg2;
                        e.key = cellj2 | (code2 << 26) | kg;
                        e.par = s_slot | pg;
                        tab[slot2] = e;                                                                                 // :225-226
                    }
                    RECONV();
                    // the prefix goes on behind s: up to the next push that sorts inside the batch
                    const uint32_t f1 = wave_umin32((pl && lane != Ls) ? first_bad : (uint32_t)KN);
                    const uint32_t f2 = wave_umin32(push2 ? max(below2, (uint32_t)nvalid) : (uint32_t)KN);
                    int nv2 = (int)min(min(min((uint32_t)nb, (uint32_t)nvalid_hz), min((uint32_t)pn_all, cut)), min(f1, f2));
                    nv2 = rfli(max(nv2, nvalid));
                    DBG_COUNT(S, 52, nv2 - nvalid);
#ifdef FXJPS_HWID  // diagnostics: what ends a second round -- [48] second rounds, [49] the end of the batch, [50] a push of the first
                   // round (another intruder), [51] a push of s (the chain goes on), [52] a touched node / hazard / goal, [53] nodes gained
                    if (A.out_counters && lane == 0) {
                        const uint32_t oth = min(min((uint32_t)nvalid_hz, (uint32_t)pn_all), cut);
                        const uint32_t why = (uint32_t)nv2 >= (uint32_t)nb ? 49u : (f1 <= f2 && f1 <= oth) ? 50u : (f2 <= oth ? 51u : 52u);
                        atomicAdd(&A.out_counters[48], 1ull);
                        atomicAdd(&A.out_counters[why], 1ull);
                        atomicAdd(&A.out_counters[53], (unsigned long long)(nv2 - nvalid));
                        atomicAdd(&A.out_counters[54], (unsigned long long)(nb - nv2));
                    }
                    RECONV();
#endif
                    const bool cm_b = node_on && mynode >= nvalid && mynode < nv2;  // my node is committed in the second round
                    if (cm_b && !closed_m && lane == lstart_m) tab[n_slot].key = ecv.key | KEY_CLOSED;                     // :210
                    RECONV();
                    const bool w_b = pl && cm_b;
                    if (w_b) {
                        TEnt e;
                        e.g = tg;
                        e.key = newkey;
                        e.par = n_slot | pg;
                        tab[jslot] = e;                                                                                 // :225-226
                    }
                    RECONV();
                    pops += 1u + (uint32_t)(nv2 - nvalid);
                    pushes += (uint32_t)__popcll(__ballot(push2)) + (uint32_t)__popcll(__ballot(w_b));
                    if (FX_RARE(rfl(pops) > max_pops)) res_len = (uint32_t)QI_WATCHDOG;
                    // what goes into the open list: the first round's pushes but s, s's pushes, the second round's
                    ndrop = nv2;
                    w_ins = on2 ? push2 : ((w && lane != Ls) || w_b);
                    if (HC != 1)
                        kcap = nv2 == nb ? min(kcap + 4, kmax) : max(min(kcap, 2 * nv2), min(KCAP_MIN2, kmax));
                    else  // (the batch may grow to what both rounds commit)
                        kcap = nv2 == nb ? min(kcap0 + 2, kmax) : (2 * nv2 < nb ? nv2 + 1 : kcap0);
                }
                if (FX_USUAL(rfl(res_len) == 0u)) {
                    // the committed nodes leave R; heappush (:227-228) of every relaxed successor.  The nodes that
                    // were not the next pops simply stay where they are.
                    if (ONE_INS) {
                        xi_do = true;
                        xi_drop = ndrop;
                        xi_w = w_ins;
                        xi_f = ins_f;
                        xi_x = ins_x;
                        xi_s = ins_s;
                        xi_c = ins_c;
                    } else if (!open_insert<HC == 2 && !DIRECT && !TRK && FXJPS_BANDED != 0>(A, Q, R, S, far, lane, lane0, ndrop, w_ins, ins_f, ins_x, ins_s, ins_c PF_ARGS)) {
                        res_len = (uint32_t)QI_FAR_FULL;
                    }
                }
            }
        }
        if (!ONE_INS) PF(2);
        if (!FX_USUAL(done_fast)) do {
        // (every path from here to the next iteration is rare.  Some of them never look at the probe lines and the cell
        // infos that are still on their way; the compiler's wait-count pass would carry "a load into these registers may
        // be outstanding" around the loop and drain the memory queue -- the previous batch's table stores included --
        // wherever the registers are written next, e.g. at the entry of every R refill: measured, - 1.6 % plans/s.)
        __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0)

        // (GEN_NEXT: on to the next iteration from the rarely taken general form -- with nothing outstanding that the
        // compiler's wait-count pass could carry around the loop, see COLD_SYNC)
        // (the general form is a do { } while (0) block in front of the one insertion and of the COLD_SYNC behind it: leave it)
#define GEN_NEXT \
    {            \
        break;   \
    }
        // ================= commit, general form: the first node alone     jps1.py:199-228
        // The other nodes of the batch stay in R untouched; node 0 is certainly the reference's next pop.
        if (HC == 1) kcap = 2;
#ifdef FXJPS_PROF
        pf_general++;
#endif
        if (rfl(res_len) != 0u) break;
        {
            const bool mine = mynode == 0;
            TEnt ec;
            ec.g = __longlong_as_double((long long)(((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)((uint64_t)__double_as_longlong(ecv.g) >> 32), 0) << 32) |
                                                    (uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(uint64_t)__double_as_longlong(ecv.g), 0)));
            ec.key = (uint32_t)__builtin_amdgcn_readlane((int)ecv.key, 0);
            ec.par = (uint32_t)__builtin_amdgcn_readlane((int)ecv.par, 0);
            const uint32_t b0slot = (uint32_t)__builtin_amdgcn_readlane((int)n_slot, 0);  // lane 0 belongs to node 0
            const uint32_t b0ci = (uint32_t)__builtin_amdgcn_readlane((int)n_ci, 0);
            const uint32_t b0xyd = lane_get(R.x, 0);
            const int ncx = (int)(b0xyd >> 17), ncy = (int)((b0xyd >> 4) & 0x1FFFu);
            pops += 1u;
            if (rfl(pops) > max_pops) {
                res_len = (uint32_t)QI_WATCHDOG;
                GEN_NEXT;
            }
            if (ncx == gx && ncy == gy) {
                // ============== goal popped: walk came_from back to the start   jps1.py:199-208
                *res_cost = ec.g;
                uint32_t n = 0;
                uint32_t sl = b0slot;
                uint32_t* scratch = reinterpret_cast<uint32_t*>(far);  // the far tier is dead now
                const uint32_t scratch_cap = A.far_cap * 4u;
                // (the walk ends at the start CELL, not at a parent sentinel: with 2^27 slots per table every 27-bit
                // value is a valid slot index)
                const uint32_t start_cell = ((uint32_t)sx << 13) | (uint32_t)sy;
                bool at_start = false;
                while (!at_start && n < scratch_cap) {
                    const TEnt e = uniform_ent(tab[sl]);
                    const uint32_t cell = e.key & CELL_MASK;
                    if (lane == 0) scratch[n] = ((cell >> 13) << 16) | (cell & 0x1FFFu);
                    RECONV();
                    n++;
                    at_start = cell == start_cell;
                    sl = e.par & PAR_MASK;
                }
                if (!at_start) {
                    res_len = (uint32_t)QI_FAR_FULL;  // the scratch ran out before the start: the large pool cannot
                } else if (n > (uint32_t)A.max_len) {
                    res_len = (uint32_t)-1;  // FXJPS_Q_PATH_TOO_LONG
                } else {
                    res_len = n;
                    uint32_t* dst = A.out_path + (size_t)q * A.max_len;
                    for_path_cells(lane, n, [&](uint32_t k) { dst[k] = scratch[n - 1 - k]; });  // (store_result reads the slot back by the same rule)
                    RECONV();
                }
                GEN_NEXT;
            }
            if (ec.key & KEY_CLOSED) {  // stale duplicate of a closed node: a provable no-op (SURVEY Q3); it leaves R
                if (ONE_INS) {
                    xi_do = true;
                    xi_drop = 1;
                    xi_w = false;
                } else {
                    (void)open_insert<HC == 2 && !DIRECT && !TRK && FXJPS_BANDED != 0>(A, Q, R, S, far, lane, lane0, 1, false, 0ull, 0u, 0u, 0u PF_ARGS);
                }
                GEN_NEXT;
            }
            bool nhas = has && mine;
            uint32_t ncode = code, ncellj = cellj, njci = jci, nlci = lci;
            bool nneed_ci = need_ci && mine;
            Probe npe = pe;
            uint32_t nb_ = b;
            bool reprobe = false;
            bool remine = mine;  // the lanes that work for node 0
            if (((ec.key >> 26) & 0xFu) != (b0xyd & 0xFu)) {
                // the parent changed after this entry was pushed: expand again with the table's direction
                // (node 0 alone: its rays on the lanes 0 .. 7, whatever lanes the batch had dealt out)
                const bool re_on = lane < 8;
                ncode = re_on ? ((S.dirlut[((ec.key >> 26) & 0xFu) * 256u + (b0ci & 0xFFu)] >> (4u * ((uint32_t)lane & 7u))) & 0xFu) : DIR_NONE;
                // (lane 0 belongs to node 0: its record)
                int nkres = 0;
                expand_batch<JD2>(G, lane_get(nr0, 0), lane_get(nr1, 0), lane_get(nr2, 0), lane_get(nr3, 0), ncx + 1, ncy + 1, ncode, re_on, gpx, gpy, &nhas, &ncellj, &njci, tab, 0u, nullptr,
                                  TRK ? &nkres : nullptr PF_ARGS);
                if (TRK) rs_mark_ray(G, S, ncx + 1, ncy + 1, ncode, nkres);
                remine = re_on;
                nhas = nhas && remine;
                nb_ = probe_at(ncellj);
                nneed_ci = !JD2 && nhas && t == 0 && njci == 0xFFFFu;
                nlci = 0;
                if (nneed_ci) nlci = G.ci[(size_t)((int)(ncellj >> 13) + 1) * G.NS + ((int)(ncellj & 0x1FFFu) + 1)];
                reprobe = true;
            }
            if (lane == 0) tab[b0slot].key = ec.key | KEY_CLOSED;  // close_set.add   jps1.py:210
            RECONV();
            const double gc = ec.g;
            // ---- relax the successors                      jps1.py:215-228
            bool pend = nhas;
            bool found = false, inserted = false;
            uint32_t jslot = 0, jkey = 0;
            double jg = 0.0;
            bool overflow = false;
            uint32_t probes = 0;
            bool first = true;
            while (__ballot(pend) != 0ull) {
                if (++probes > nbk + 16u) {  // watchdog: the table is never full
                    overflow = true;
                    break;
                }
                if (!first || reprobe) probe_load<DIRECT>(npe, tab, nb_, t, pend);
                first = false;
                bool pf, phe;
                uint32_t pslot, ek;
                double eg;
                probe_eval<DIRECT>(npe, pend, ncellj, nb_, gen, &pf, &phe, &pslot, &eg, &ek);
                bool cand = false;
                uint32_t cslot = SLOT_NONE;
                if (pend) {
                    if (pf) {
                        found = true;
                        jslot = pslot;
                        jg = eg;
                        jkey = ek;
                        pend = false;
                    } else if (phe) {
                        cand = true;
                        cslot = pslot;
                    } else {
                        nb_ = nb_ + 1u == nbk ? 0u : nb_ + 1u;
                        reprobe = true;
                    }
                }
                // two rays may want the same empty slot in the same round: the lowest ray wins, the other probes again
                bool conflict = false;
                if (__popcll(__ballot(cand && t == 0)) > 1) {
#pragma unroll
                    for (int r = 0; r < 7; r++) {
                        const int sl = r * SL;
                        const uint32_t os = (uint32_t)__builtin_amdgcn_readlane((int)cslot, sl);
                        if (sl < gsh && cand && os == cslot) conflict = true;
                    }
                }
                if (cand && !conflict) {
                    inserted = true;
                    jslot = cslot;
                    pend = false;
                    if (t == 0) {  // taken (live for this query): visible to a ray that probes again
                        tab[jslot].key = ncellj | (ncode << 26) | kg;
                        tab[jslot].par = PAR_NONE | pg;
                    }
                    RECONV();
                }
                if (cand && conflict) reprobe = true;
                if (__ballot(cand && conflict) != 0ull) __threadfence_block();
            }
            PF(6);
            const int njx = (int)(ncellj >> 13), njy = (int)(ncellj & 0x1FFFu);
            bool push = false;
            double tg = 0.0;
            if (nhas && !overflow) {
                tg = gc + seg_len<HC>(ncx, ncy, njx, njy);  // :221
                if (found) {
                    if (!(jkey & KEY_CLOSED) && tg < jg) push = true;  // :218, :223
                } else {
                    push = true;  // never seen: the `not in pqueue` clause, :224
                }
            }
            if (push && t == 0) {
                TEnt e;
                e.g = tg;
                e.key = ncellj | (ncode << 26) | kg;
                e.par = b0slot | pg;
                tab[jslot] = e;  // came_from / gscore, :225-226
            }
            RECONV();
            tcount += (uint32_t)__popcll(__ballot(inserted && t == 0));
            if (rfl(tcount) > tab_limit || __ballot(overflow) != 0ull) {
                res_len = (uint32_t)QI_TABLE_FULL;
                GEN_NEXT;
            }
            // ---- heappush (f, jp)                                jps1.py:227-228
            const uint64_t fb = (uint64_t)__double_as_longlong(tg + heuristic<HC>(njx, njy, gx, gy));
            const bool pl = push && t == 0;
            pushes += (uint32_t)__popcll(__ballot(pl));
            // node 0 leaves R, its successors enter the open list
            if (ONE_INS) {
                xi_do = true;
                xi_drop = 1;
                xi_w = pl;
                xi_f = fb;
                xi_x = (ncellj << 4) | ncode;
                xi_s = jslot;
                xi_c = nneed_ci ? nlci : njci;
            } else if (!open_insert<HC == 2 && !DIRECT && !TRK && FXJPS_BANDED != 0>(A, Q, R, S, far, lane, lane0, 1, pl, fb, (ncellj << 4) | ncode, jslot, nneed_ci ? nlci : njci PF_ARGS)) {
                res_len = (uint32_t)QI_FAR_FULL;
                GEN_NEXT;
            }
            PF(7);
        }
        } while (0);
        if (ONE_INS && xi_do) {
            if (!open_insert<HC == 2 && !DIRECT && !TRK && FXJPS_BANDED != 0>(A, Q, R, S, far, lane, lane0, xi_drop, xi_w, xi_f, xi_x, xi_s, xi_c PF_ARGS)) {
                res_len = (uint32_t)QI_FAR_FULL;
            }
        }
        if (ONE_INS) PF(2);
        if (!FX_USUAL(done_fast)) COLD_SYNC();  // (see GEN_NEXT)
    }
    PF_FLUSH;

    if (A.qstat && lane0 == 0) A.qstat[4 * (size_t)q + 2] = (unsigned long long)pops;
    if (cnt4 && lane0 == 0) {
        atomicAdd(&cnt4[0], (unsigned long long)pops);
        atomicAdd(&cnt4[1], (unsigned long long)pushes);
#ifdef FXJPS_PROF
        atomicAdd(&cnt4[4], pf_batches);
        atomicAdd(&cnt4[5], pf_popped);
        atomicAdd(&cnt4[6], pf_general);
#endif
    }
    return (int32_t)rfl(res_len);
}

// A plain batch: a finished path goes to the host now, not when the slowest query of the batch has ended (DESIGN.md
// section 7).  The wavefront takes res_len cells of the arena (every lane takes part in the add, as in the work counter's
// fetch: lane 0 adds, the others add 0) and copies its path slot there.  search_one's lanes stored the slot by the same
// rule (for_path_cells), so each lane reads back what it stored itself and program order is all the copy needs -- a
// release fence in front of it writes the L2 back once per query (profiles/result_streaming.txt section 1: + 6 % kernel
// time on 125 000 queries).  (The large retry pool's kernels are hashed ones and do not come here: a batch that retried is
// packed on the device, finish_search.)
// A function of its own, handed the kernel-argument segment (the kernel's one argument is SearchArgs, at offset 0):
// inlined into run_query, its six pointers are loaded in front of the loop over the queries and stay live across every
// search -- more scalar spills in every instantiation, a vector spill in the hashed ones.
__device__ __noinline__ __attribute__((cold)) void store_result(const __attribute__((address_space(4))) SearchArgs* A, uint32_t q, int32_t res_len, double res_cost,
                                                                uint32_t start_cell) {
    const int lane = threadIdx.x & 63;
    if (lane == 0) {
        if (start_cell != ~0u) A->out_path[(size_t)q * A->max_len] = start_cell;  // (start == goal: the path is the start)
        A->out_len[q] = res_len;
        A->out_cost[q] = (res_len == 0 || res_len <= QI_TABLE_FULL) ? 0.0 : res_cost;
    }
    if (A->host_len == nullptr) return;
    if (res_len > 0) {
        const unsigned long long base = rfl64(atomicAdd(A->host_cursor, lane == 0 ? (unsigned long long)res_len : 0ull));
        const bool fits = base + (unsigned long long)res_len <= A->host_cap;
        if (fits) {
            const uint32_t* src = A->out_path + (size_t)q * A->max_len;
            uint32_t* dst = A->host_cells + base;
            for_path_cells(lane, (uint32_t)res_len, [&](uint32_t k) { dst[k] = src[k]; });
        }
        if (lane == 0) A->host_base[q] = fits ? (long long)base : -1ll;
    }
    if (lane == 0) {
        A->host_len[q] = res_len;
        A->host_cost[q] = (res_len == 0 || res_len <= QI_TABLE_FULL) ? 0.0 : res_cost;
    }
}

template <int HC, bool TRK, bool DIRECT, bool MG, class MID>
__device__ __forceinline__ void run_query(const SearchArgs& A, const uint32_t q, const MID& S, TEnt* __restrict__ tab,
                          FarEnt* __restrict__ far, uint32_t& gen) {
    // The grid: the handle's resident one, or (MG) the slot this query names -- its descriptor read once, with scalar loads
    // (the id is wave-uniform; read through the constant address space, the descriptor's 80 bytes are scalar loads).
    // Nothing else of the search depends on which grid a wavefront's previous queries ran on: every search writes its
    // visited-table entries under a generation tag of its own and reads only entries with that tag (a cell-indexed slot
    // x << direct_ly | y that another grid's search left behind carries an older tag and reads as empty), and the wipe at
    // GEN_WRAP clears the whole per-wavefront table whatever its entries were.  direct_ly is sized by the host from the
    // largest H of the slots in the batch, so every slot's cells fit the same table.
    GridDev Gs;
    if (MG) {
        const int32_t gid = rfli(A.grid_ids[q]);
        const auto* src = reinterpret_cast<__attribute__((address_space(4))) const uint32_t*>((uint64_t)(A.grids + gid));
        uint32_t w[sizeof(GridDev) / 4];
#pragma unroll
        for (int i = 0; i < (int)(sizeof(GridDev) / 4); i++) w[i] = src[i];
        __builtin_memcpy(&Gs, w, sizeof(GridDev));
    }
    const GridDev& G = MG ? Gs : A.G;
    const int lane = threadIdx.x & 63;
    const bool imm = A.single != 0u;
    const int sx = imm ? A.imm[0] : rfli(A.starts[2 * q]), sy = imm ? A.imm[1] : rfli(A.starts[2 * q + 1]);
    const int gx = imm ? A.imm[2] : rfli(A.goals[2 * q]), gy = imm ? A.imm[3] : rfli(A.goals[2 * q + 1]);
    int32_t res_len = 0;
    double res_cost = 0.0;
    // ---- outcomes that need no search (results-equivalent to the exhaustive run, SURVEY Q11/Q14/Q15)
    // (every decision here is wave-uniform; lane-dependent work is kept in if-blocks without an else so that the
    // compiler's divergence analysis does not spread to the search state)
    bool search = false, start_only = false;
    if (sx < 0 || sy < 0 || sx >= G.W || sy >= G.H) {
        res_len = -2;  // FXJPS_Q_BAD_START
    } else if (sx == gx && sy == gy) {  // the first pop is the goal: jps1.py:199-208
        res_len = A.max_len >= 1 ? 1 : -1;
        start_only = A.max_len >= 1;
    } else if (gx >= 0 && gy >= 0 && gx < G.W && gy < G.H) {
        // an occupied goal is never returned by a jump (blocked() precedes the goal test, jps1.py:99-103)
        const uint64_t gw = G.bm[(size_t)(2 * G.LINES + gx + 1) * G.WORDS + ((gy + 1) >> 6)].occ;
        search = rfl((uint32_t)((gw >> ((gy + 1) & 63)) & 1ull)) == 0u;
        if (search && G.comp) {
            // every move of the reference joins two free cells that are 4-connected, so a goal in another
            // component (of a free start) can only end in the exhaustive (0, t) of jps1.py:230.  The labels are a
            // union-find forest (flat after a full relabelling, a few links deep after small cell updates, see
            // k_ccl_update); an occupied start may still carry the label of an earlier grid: the map decides.
            const uint64_t sw = G.bm[(size_t)(2 * G.LINES + sx + 1) * G.WORDS + ((sy + 1) >> 6)].occ;
            if (rfl((uint32_t)((sw >> ((sy + 1) & 63)) & 1ull)) == 0u) {
                const auto root = [&](int i) -> int {  // -1: no label, -2: not found within the step limit (no early-out then)
                    int p = rfli(G.comp[i]);
                    if (p < 0) return -1;
                    for (int step = 0; step < 256 && p != i; step++) {
                        i = p;
                        p = rfli(G.comp[i]);
                    }
                    return p == i ? i : -2;
                };
                const int cs = root(sx * G.H + sy), cg = root(gx * G.H + gy);
                if (cs >= 0 && cg >= 0 && cg != cs) search = false;
            }
        }
    }
    if (search) {
        if (A.qstat && lane == 0) {
            A.qstat[4 * (size_t)q] = __builtin_amdgcn_s_memrealtime();
            // (diagnostics: the shader-clock cycles of the search beside its wall time -- the clock the chip ran at.  The
            // start value waits in the slot of the end time: no register is held across the search for it)
            A.qstat[4 * (size_t)q + 1] = __builtin_readcyclecounter();
            A.qstat[4 * (size_t)q + 3] = (unsigned long long)(tab - A.tables) / ((size_t)BUCKET * A.nbuckets);
        }
        RECONV();
        res_len = search_one<HC, TRK, DIRECT, MG>(A, G, q, sx, sy, gx, gy, S, tab, far, gen, &res_cost, A.out_counters);
        if (TRK) {  // hand the read set over (one row of each bitmap per lane) and clear it for the next query
            unsigned long long* dst = A.qread + (size_t)q * 128;
            dst[lane] = S.bx[lane];
            dst[64 + lane] = S.bx[64 + lane];
            S.bx[lane] = 0ull;
            S.bx[64 + lane] = 0ull;
        }
        if (A.qstat && lane == 0) {
            const unsigned long long qc0 = A.qstat[4 * (size_t)q + 1];
            A.qstat[4 * (size_t)q + 3] |= (__builtin_readcyclecounter() - qc0) << 24;  // (wavefront index below, cycles above)
            A.qstat[4 * (size_t)q + 1] = __builtin_amdgcn_s_memrealtime();
        }
        RECONV();
        // the next search of this wavefront uses the next tag; when the tags run out the table is wiped once
        gen = rfl(gen + 1u);
        if (gen == GEN_WRAP) {
            gen = 0;
            if (A.out_counters && lane == 0) atomicAdd(&A.out_counters[7], 1ull);
            const uint32_t nent = (uint32_t)BUCKET * A.nbuckets;
            uint4* p = reinterpret_cast<uint4*>(tab);
            const uint4 ff = make_uint4(0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu);
            for (uint32_t i = lane; i < nent; i += WAVE) p[i] = ff;
            RECONV();
        }
    }
    if (TRK || !DIRECT) {
        if (lane == 0) {
            if (start_only) A.out_path[(size_t)q * A.max_len] = ((uint32_t)sx << 16) | (uint32_t)sy;
            A.out_len[q] = res_len;
            A.out_cost[q] = (res_len == 0 || res_len <= QI_TABLE_FULL) ? 0.0 : res_cost;
        }
        RECONV();
    } else {  // (cell-indexed tables, no read sets: the same three stores, and a plain batch's results to the host)
        store_result((const __attribute__((address_space(4))) SearchArgs*)__builtin_amdgcn_kernarg_segment_ptr(), q, res_len, res_cost,
                     start_only ? ((uint32_t)sx << 16) | (uint32_t)sy : ~0u);
        RECONV();
    }
}

// (SearchArgs is the kernel's ONE argument, so it lies at offset 0 of the kernel-argument segment: store_result reads it there)
template <int HC, bool TRK, bool DIRECT, bool MG>
__global__ __launch_bounds__(WAVE* WPB, OCC) void k_search(SearchArgs A) {
#include "fxjps_search_block.hip.inc"
}
// The tracking search of a slots batch (fxjps_replan_slots under fxjps_set_slot_reuse(1), DESIGN.md section 3.18): a grid per
// query AND read-set recording.  Every mark uses the tile shift of the query's own slot (run_query hands search_one that
// slot's descriptor), the bitmaps in LDS are cleared when a query hands its read set over, so they are clear between
// queries of different slots, and a read set lands at A.qread + q * 128, q being the index in the (sub-)batch.
// (A kernel name of its own, not k_search<HC, true, DIRECT, true>: the slots batch's k_search instantiations stay the four
// untracked ones, and so does every kernel the tile rule does not use.)
// (one argument, as k_search: run_query's exit may read SearchArgs at offset 0 of the kernel-argument segment)
template <int HC, bool DIRECT>
__global__ __launch_bounds__(WAVE* WPB, OCC) void k_slot_reads_search(SearchArgs A) {
    constexpr bool TRK = true, MG = true;
#include "fxjps_search_block.hip.inc"
}

// Device self-test of the DPP minimum against the shuffle form (tests/test_gpu_parity.py).
__global__ void k_selftest_wavemin(const uint64_t* __restrict__ in, uint64_t* __restrict__ out, int rounds) {
    const int lane = threadIdx.x & 63;
    for (int r = 0; r < rounds; r++) {
        const uint64_t v = in[(size_t)r * 64 + lane];
        const uint64_t a = wave_umin64(v), b = rfl64(wave_min_u64(v));
        const uint32_t c = wave_umin32((uint32_t)(v >> 7)), d = rfl(wave_min_u32((uint32_t)(v >> 7)));
        if (lane == 0) {
            out[(size_t)r * 4 + 0] = a;
            out[(size_t)r * 4 + 1] = b;
            out[(size_t)r * 4 + 2] = c;
            out[(size_t)r * 4 + 3] = d;
        }
        // ranks of the 64 values (v >> 7), behind the minima
        reinterpret_cast<uint32_t*>(out + (size_t)rounds * 4)[(size_t)r * 64 + lane] = wave_rank64((uint32_t)(v >> 7), lane);
        // ... and the ranks of the 96-bit keys (v >> 40 : low word of v : v >> 9 masked), behind those
        reinterpret_cast<uint32_t*>(out + (size_t)rounds * 4 + (size_t)rounds * 32)[(size_t)r * 64 + lane] =
            wave_rank96((uint32_t)(v >> 40) & 0x3u, (uint32_t)v & 0x7u, (uint32_t)(v >> 9) & 0x3u, lane);
    }
}

// Device self-test of the open list on its own (tests/test_gpu_parity.py): one wavefront runs a host-written script of
// steps -- "pop up to k entries, then push these m keys" -- through the very open_fill / open_insert the search uses,
// with far tiers as small as the test likes, and writes out what it popped.  The host replays the script on a binary
// heap: every pop must be the minimum of the (f, x, y, direction) keys in the list, every pushed entry must come out
// exactly once.  Reaches what no map does: thousands of entries with one and the same full key (the direct pop from
// the far tier), refills that discard what they took, rule sets of the lazily deleted near band that overflow.
template <bool BANDED>
__global__ __launch_bounds__(WAVE) void k_selftest_openlist(SearchArgs A, const unsigned long long* __restrict__ in_f,
                                                           const uint32_t* __restrict__ in_x, const uint32_t* __restrict__ step_pops,
                                                           const uint32_t* __restrict__ step_off, uint32_t nsteps, double delta0,
                                                           unsigned long long* __restrict__ out_f, uint32_t* __restrict__ out_x,
                                                           uint32_t* __restrict__ out_s, uint32_t* __restrict__ out_k,
                                                           uint32_t* __restrict__ out_info, uint32_t out_cap) {
    __shared__ WaveLds s_w[1];
    const int lane = threadIdx.x & 63;
    for (int i = lane; i < WaveLds::HZ_SIZE; i += WAVE) s_w[0].hz[i] = ~0u;
    if (lane < NBANDS) s_w[0].bcnt[lane] = 0u;
    __syncthreads();
    Mid S;
    S.w = (LDS_PTR(WaveLds))&s_w[0];
    S.dirlut = nullptr;
    S.bx = nullptr;
#ifdef FXJPS_PROF
    S.dbg = A.out_counters;
#endif
    FarEnt* far = A.far;
    OpenList Q;
    Q.r_n = 0;
    Q.m_n = 0;
    Q.far_n = 0;
    Q.farb_n = 0;
    Q.T2hi = (uint32_t)(F_INF >> 32);
    Q.Rbits = F_INF;
    Q.Rx = 0;
    Q.Tbits = F_INF;
    Q.Tx = 0;
    Q.dxs = 0;
    Q.delta = delta0;
    Q.hshift = 0;
    Q.cur0 = 0;
    Q.fail = 0;
    Q.banded = A.banded;
    RTier R;
    R.f = ~0ull;
    R.x = ~0u;
    R.s = 0u;
    R.c = 0u;
    PF_DECL;
    uint32_t total = 0, fail = 0;
    // the script, then pops of whatever R holds until the list is empty
    for (uint32_t st = 0; fail == 0u; st++) {
        open_uniform(Q);
        const bool scripted = st < nsteps;
        const bool any = open_fill<BANDED>(A, A.G, Q, R, S, far, lane);
        if (Q.fail != 0u) {
            fail = 2u;
            break;
        }
        if (!scripted && !any) break;
        uint32_t k = any ? (uint32_t)Q.r_n : 0u;
        if (scripted) k = min(k, step_pops[st]);
        k = rfl(k);
        if (total + k > out_cap) {
            fail = 3u;
            break;
        }
        if ((uint32_t)lane < k) {
            out_f[total + lane] = R.f;
            out_x[total + lane] = R.x;
            out_s[total + lane] = R.s;
        }
        RECONV();
        if (scripted && lane == 0) out_k[st] = k;
        RECONV();
        total += k;
        const uint32_t o0 = scripted ? step_off[st] : 0u, o1 = scripted ? step_off[st + 1] : 0u;
        const bool w = (uint32_t)lane < o1 - o0;
        unsigned long long kf = 0ull;
        uint32_t kx = 0u;
        if (w) {
            kf = in_f[o0 + lane];
            kx = in_x[o0 + lane];
        }
        RECONV();
        if (!open_insert<BANDED>(A, Q, R, S, far, lane, lane, (int)k, w, kf, kx, o0 + (uint32_t)lane, 0u PF_ARGS)) fail = 1u;
    }
    if (lane == 0) {
        out_info[0] = total;
        out_info[1] = fail;
        out_info[4] = (uint32_t)Q.r_n;  // what the tiers held when the script ended
        out_info[5] = Q.m_n;
        out_info[6] = Q.far_n;
        out_info[7] = Q.farb_n;
    }
}

// A streamed batch's 64 counters into the handle's pinned buffer, queued behind each of its searches: a kernel and not a
// copy, because a copy that waits in the copy engine's queue for a search holds up every copy queued after it (finish_search).
__global__ __launch_bounds__(64) void k_counters_out(const unsigned long long* __restrict__ counters, unsigned long long* __restrict__ host) {
    host[threadIdx.x] = counters[threadIdx.x];
}

// The results of the queries the host searched beside the device (fxjps.hip, HostTail) into their slots of the batch's
// device buffers, where packing, the retry path and the resident forms look for them: block i puts query ids[i].  The
// sources are pinned host memory.  Queued when the search is over, so the sums of the host's pops and pushes are plain adds.
__global__ __launch_bounds__(256) void k_host_tail_put(const uint32_t* __restrict__ ids, const uint32_t* __restrict__ path, const int32_t* __restrict__ len,
                                                       const double* __restrict__ cost, int max_len, long long nq, uint32_t* __restrict__ out_path,
                                                       int32_t* __restrict__ out_len, double* __restrict__ out_cost,
                                                       unsigned long long* __restrict__ counters, unsigned long long pops, unsigned long long pushes) {
    const uint32_t i = blockIdx.x, q = ids[i];
    if (i == 0u && threadIdx.x == 0u) {
        counters[0] += pops;
        counters[1] += pushes;
    }
    if ((long long)q >= nq) return;
    const int32_t n = len[i];
    const int cells = n < 0 ? 0 : (n > max_len ? max_len : n);
    for (int k = (int)threadIdx.x; k < cells; k += 256) out_path[(size_t)q * (size_t)max_len + (size_t)k] = path[(size_t)i * (size_t)max_len + (size_t)k];
    if (threadIdx.x == 0u) {
        out_len[q] = n;
        out_cost[q] = cost[i];
    }
}

// ---------------------------------------------------------------- CSR packing
// Exclusive scan of max(len, 0) over nq entries, one block.
__global__ __launch_bounds__(1024) void k_scan_len(const int32_t* __restrict__ len, long long nq,
                                                   long long* __restrict__ offsets) {
    __shared__ long long s_part[1024];
    const int tid = threadIdx.x;
    const long long per = (nq + 1023) / 1024;
    const long long lo = (long long)tid * per, hi = min(lo + per, nq);
    long long sum = 0;
    for (long long i = lo; i < hi; i++) sum += len[i] > 0 ? len[i] : 0;
    s_part[tid] = sum;
    __syncthreads();
    for (int o = 1; o < 1024; o <<= 1) {
        long long v = tid >= o ? s_part[tid - o] : 0;
        __syncthreads();
        s_part[tid] += v;
        __syncthreads();
    }
    long long run = tid ? s_part[tid - 1] : 0;
    for (long long i = lo; i < hi; i++) {
        offsets[i] = run;
        run += len[i] > 0 ? len[i] : 0;
    }
    if (tid == 1023) offsets[nq] = s_part[1023];
}

// One wavefront per query: dense slot -> int32 (x, y) pairs at its CSR offset.
__global__ __launch_bounds__(256) void k_gather_paths(const uint32_t* __restrict__ path, const int32_t* __restrict__ len,
                                                      const long long* __restrict__ offsets, long long nq, int max_len,
                                                      int32_t* __restrict__ cells, long long cells_cap) {
    const int lane = threadIdx.x & 63;
    const long long q = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (q >= nq) return;
    const int n = len[q];
    if (n <= 0) return;
    const long long off = offsets[q];
    if (off + n > cells_cap) return;
    const uint32_t* src = path + (size_t)q * max_len;
    int2* dst = reinterpret_cast<int2*>(cells) + off;
    for (int i = lane; i < n; i += WAVE) {
        const uint32_t v = src[i];
        dst[i] = make_int2((int)(v >> 16), (int)(v & 0xFFFFu));
    }
}

// ---- fxjps_replan_slots: the full batch's resident CSR out of two sources (DESIGN.md section 3.13).  src[q] < 0: query q
// was not searched, its length, cost and cells are the previous batch's at index q; else they are the sub-batch's at index
// src[q] (lengths and costs as k_search left them, cells still in the dense slots of max_len packed words).
struct ReplanSrc {
    const int32_t* src;
    const int32_t* p_len;  // the previous batch
    const double* p_cost;
    const long long* p_off;
    const int32_t* p_cells;
    const int32_t* s_len;  // the sub-batch
    const double* s_cost;
    const uint32_t* s_path;
    int max_len;
};

// Lengths and costs of the full batch, and the exclusive scan of max(len, 0) into offsets[0 .. nq]; one block (k_scan_len's
// scan, reading each length through the source table).
__global__ __launch_bounds__(1024) void k_replan_scan(ReplanSrc R, long long nq, int32_t* __restrict__ len, double* __restrict__ cost,
                                                      long long* __restrict__ offsets) {
    __shared__ long long s_part[1024];
    const int tid = threadIdx.x;
    const long long per = (nq + 1023) / 1024;
    const long long lo = (long long)tid * per, hi = min(lo + per, nq);
    long long sum = 0;
    for (long long i = lo; i < hi; i++) {
        const int32_t s = R.src[i];
        const int32_t n = s < 0 ? R.p_len[i] : R.s_len[s];
        len[i] = n;
        cost[i] = s < 0 ? R.p_cost[i] : R.s_cost[s];
        sum += n > 0 ? n : 0;
    }
    s_part[tid] = sum;
    __syncthreads();
    for (int o = 1; o < 1024; o <<= 1) {
        long long v = tid >= o ? s_part[tid - o] : 0;
        __syncthreads();
        s_part[tid] += v;
        __syncthreads();
    }
    long long run = tid ? s_part[tid - 1] : 0;
    for (long long i = lo; i < hi; i++) {  // (each thread reads back what it wrote itself)
        offsets[i] = run;
        const int32_t n = len[i];
        run += n > 0 ? n : 0;
    }
    if (tid == 1023) offsets[nq] = s_part[1023];
}

// One wavefront per query: its cells to their CSR offset, from the previous batch's cells or from the sub-batch's dense slot.
// A cell is 8 bytes, so an odd offset leaves the destination 8 bytes off a 16-byte boundary: that one cell goes out alone,
// the rest in pairs (16-byte stores; 16-byte loads too when the previous batch's offset has the same parity), an odd one
// at the end alone again.
__global__ __launch_bounds__(256) void k_replan_gather(ReplanSrc R, const int32_t* __restrict__ len, const long long* __restrict__ offsets,
                                                       long long nq, int32_t* __restrict__ cells, long long cells_cap) {
    const int lane = threadIdx.x & 63;
    const long long q = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (q >= nq) return;
    const int n = len[q];
    if (n <= 0) return;
    const long long off = offsets[q];
    if (off + n > cells_cap) return;
    int2* dst = reinterpret_cast<int2*>(cells) + off;
    const int head = (int)(off & 1), pairs = (n - head) >> 1, tail = head + 2 * pairs;  // tail == n or n - 1
    const int32_t s = R.src[q];
    if (s >= 0) {
        const uint32_t* sp = R.s_path + (size_t)s * (size_t)R.max_len;
        const auto cell = [](uint32_t v) { return make_int2((int)(v >> 16), (int)(v & 0xFFFFu)); };
        if (lane == 0 && head) dst[0] = cell(sp[0]);
        if (lane == 1 && tail < n) dst[tail] = cell(sp[tail]);
        const bool al = ((((size_t)s * (size_t)R.max_len) + (size_t)head) & 1u) == 0;  // the words of a pair in one 8-byte load
        for (int k = lane; k < pairs; k += WAVE) {
            const int i = head + 2 * k;
            uint32_t a, b;
            if (al) {
                const uint2 v = *reinterpret_cast<const uint2*>(sp + i);
                a = v.x;
                b = v.y;
            } else {
                a = sp[i];
                b = sp[i + 1];
            }
            *reinterpret_cast<int4*>(dst + i) = make_int4((int)(a >> 16), (int)(a & 0xFFFFu), (int)(b >> 16), (int)(b & 0xFFFFu));
        }
    } else {
        const long long poff = R.p_off[q];
        const int2* pp = reinterpret_cast<const int2*>(R.p_cells) + poff;
        if (((poff ^ off) & 1) == 0) {
            if (lane == 0 && head) dst[0] = pp[0];
            if (lane == 1 && tail < n) dst[tail] = pp[tail];
            for (int k = lane; k < pairs; k += WAVE) {
                const int i = head + 2 * k;
                *reinterpret_cast<int4*>(dst + i) = *reinterpret_cast<const int4*>(pp + i);
            }
        } else {
            for (int i = lane; i < n; i += WAVE) dst[i] = pp[i];
        }
    }
}

__global__ void k_sqrt_selftest(uint32_t n0, uint32_t n1, double* out) {
    const uint32_t i = n0 + blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n1) out[i - n0] = sqrt_u28(i);  // the very function the search uses
}

// ---- the kernels around the search: derived maps, component labels, grid preparation, adapters, cell updates, waypoints
#include "fxjps_maps.hip.inc"

}  // namespace fx
