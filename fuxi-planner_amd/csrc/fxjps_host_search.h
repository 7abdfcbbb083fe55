// fxjps_host_search.h -- one query's whole search (jps1.py:183-230) on a host core, over the derived maps the device built.
// Plain C++ (no HIP): the restatement of expand_jd and of the sequential commit of search_one (fxjps_kernels.hip.inc) that
// the library runs beside the device search on a batch's longest queries.  Results are the device's bit for bit: path
// cells, length, float64 cost, pops and pushes.
#pragma once
#include <cstdint>
#include <vector>

namespace fxh {

struct BmWord {  // 64 cells of one scan line (the device's layout)
    uint64_t stop, occ;
};

// A grid's derived maps in the device layout, read-only and shared by every thread.  Padded coordinates: cell (x, y)
// lives at (x + 1, y + 1).
struct Maps {
    const uint16_t* jd = nullptr;  // [PW][NS][8] jump-distance records (the neighbour byte rides in bits 13-14 of entries 0 .. 3)
    const BmWord* bm = nullptr;    // [4][LINES][WORDS] straight scan words: travel +x, -x, +y, -y
    const int32_t* comp = nullptr; // [W * H] component forest of the free cells, or nullptr: no early-out
    int32_t W = 0, H = 0, NS = 0, LINES = 0, WORDS = 0;
};

constexpr uint32_t PD_NONE = 5, DIR_NONE = 0xFu;
constexpr int32_t Q_PATH_TOO_LONG = -1, Q_BAD_START = -2, QI_WATCHDOG = -102;

// nodeNeighbours (jps1.py:49-93) on a neighbour mask: the direction codes (dx+1)*4 + (dy+1) of a node's rays, one per
// nibble, DIR_NONE behind the last.  pd = the code of direction(c, came_from[c]), PD_NONE for the start node.
uint32_t dirlut_entry(uint32_t pd, uint32_t nbm);
void dirlut_fill(uint32_t* lut);  // [11 * 256]: entry [pd * 256 + nbm]

struct Result {
    int32_t len = 0;     // cells of the path, 0: none, Q_PATH_TOO_LONG, Q_BAD_START, QI_WATCHDOG
    double cost = 0.0;   // gscore[goal] (0 when len is 0 or an internal code)
    uint64_t pops = 0, pushes = 0;  // as the search kernel counts them: the start's push is not counted
};

// One thread's search state: a dense visited table under generation tags (never cleared between queries) and the heap's
// storage, both kept from call to call.
class Searcher {
public:
    // out_path: [max_len] packed x << 16 | y, written for len >= 1.  hchoice 1 or 2; grids of at most 2^20 cells.
    Result plan(const Maps& M, const uint32_t* dirlut, int hchoice, int sx, int sy, int gx, int gy, int max_len, uint32_t* out_path,
                uint64_t max_pops);

private:
    struct Ent {
        double g;      // gscore[node]
        uint32_t par;  // flat index x * H + y of came_from[node], NO_PARENT for the start
        uint32_t tag;  // generation << 1 | closed
    };
    struct HeapEnt {
        uint64_t f;     // f as raw bits (f >= +0: unsigned order == numeric order)
        uint32_t cell;  // x << 13 | y (unsigned order == (x, y) tuple order)
        uint32_t idx;   // x * H + y
    };
    template <int HC>
    Result search(const Maps& M, const uint32_t* dirlut, int sx, int sy, int gx, int gy, int max_len, uint32_t* out_path, uint64_t max_pops);
    void heap_push(HeapEnt e);
    HeapEnt heap_pop();

    std::vector<Ent> tab_;
    std::vector<HeapEnt> heap_;
    std::vector<uint32_t> walk_;
    uint32_t gen_ = 0;
};

}  // namespace fxh
