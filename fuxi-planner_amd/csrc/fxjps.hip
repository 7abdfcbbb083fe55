// fxjps.hip -- host side of libfxjps.so: the C ABI of include/fxjps.h on top of
// the HIP kernels in fxjps_kernels.hip.inc.  gfx950 only; no CPU fallback: if
// there is no HIP device every entry point fails with FXJPS_E_NODEV.
//
// Build: hipcc --offload-arch=gfx950 -O3 -ffp-contract=off -fPIC -shared (see Makefile).
#include <hip/hip_runtime.h>

#include <dlfcn.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <condition_variable>
#include <cstdarg>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "../../include/fxjps.h"
#include "fxjps_host_search.h"
#include "fxjps_kernels.hip.inc"
#include "fxjps_owned.h"
#include "fxjps_results.h"

namespace {

using fx::FarEnt;
using fx::GridDev;
using fx::SearchArgs;
using fx::TEnt;

// (handles are created from threads: the text of a failed fxjps_create* belongs to the calling thread, which is the one that
// asks for it with fxjps_last_error(NULL))
thread_local std::string g_create_error;

// FXJPS_DEBUG=1 in the environment: progress lines on stderr (bring-up aid)
bool dbg_on() {
    static int on = -1;
    if (on < 0) on = getenv("FXJPS_DEBUG") ? 1 : 0;
    return on == 1;
}
#define DBG(...)                          \
    do {                                  \
        if (dbg_on()) {                   \
            fprintf(stderr, "[fxjps] ");  \
            fprintf(stderr, __VA_ARGS__); \
            fprintf(stderr, "\n");        \
            fflush(stderr);               \
        }                                 \
    } while (0)

// Independent jobs side by side on host threads (one per context of a multi-device handle; slices of one large copy).
// Nothing may leave the library as a C++ exception: a thread that cannot be created makes its job run on the calling
// thread instead, and a job that throws (std::bad_alloc in a worker's vectors) is reported as FXJPS_E_NOMEM.  -> the first
// non-zero result in job order.
template <typename F>
int run_side_by_side(size_t n, F&& job) {  // job(i) -> int
    std::vector<int> rcs(n, FXJPS_OK);
    const auto guarded = [&](size_t i) {
        try {
            rcs[i] = job(i);
        } catch (const std::bad_alloc&) {
            rcs[i] = FXJPS_E_NOMEM;
        } catch (...) {
            rcs[i] = FXJPS_E_HIP;
        }
    };
    std::vector<std::thread> th;
    try {
        th.reserve(n);
    } catch (...) {
    }
    for (size_t i = 1; i < n; i++) {
        bool started = false;
        try {
            th.emplace_back(guarded, i);
            started = true;
        } catch (...) {  // std::system_error: no more threads
        }
        if (!started) guarded(i);
    }
    if (n > 0) guarded(0);
    for (auto& t : th) t.join();
    for (size_t i = 0; i < n; i++)
        if (rcs[i]) return rcs[i];
    return FXJPS_OK;
}

double now_s() {
    return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

// Bytes the library holds right now, over every handle of the process (fxjps_debug_live_bytes): device memory, and pinned
// host memory.  Counted where memory is allocated or freed, nowhere else.
std::atomic<int64_t> g_live_device{0}, g_live_pinned{0};

struct DeviceMem {
    using error = hipError_t;
    static constexpr hipError_t ok = hipSuccess;
    static hipError_t alloc(void** p, size_t bytes) { return hipMalloc(p, bytes); }
    static void free(void* p) { (void)hipFree(p); }
    static std::atomic<int64_t>& live() { return g_live_device; }
};
struct PinnedMem {
    using error = hipError_t;
    static constexpr hipError_t ok = hipSuccess;
    static hipError_t alloc(void** p, size_t bytes) { return hipHostMalloc(p, bytes, hipHostMallocDefault); }
    static void free(void* p) { (void)hipHostFree(p); }
    static std::atomic<int64_t>& live() { return g_live_pinned; }
};
template <typename T>
using DBuf = fx::OwnedBuf<T, DeviceMem>;  // grow-only device buffer
template <typename T>
using HBuf = fx::OwnedBuf<T, PinnedMem>;  // grow-only pinned host buffer

struct StreamRes {
    using type = hipStream_t;
    static hipError_t create(hipStream_t* s, unsigned flags) { return hipStreamCreateWithFlags(s, flags); }
    static void destroy(hipStream_t s) { (void)hipStreamDestroy(s); }
};
struct EventRes {
    using type = hipEvent_t;
    static hipError_t create(hipEvent_t* ev, unsigned flags) { return hipEventCreateWithFlags(ev, flags); }
    static void destroy(hipEvent_t ev) { (void)hipEventDestroy(ev); }
};
struct MappedWordRes {  // one zeroed uint32_t in a 64-byte pinned allocation
    using type = uint32_t*;
    static constexpr int64_t BYTES = 64;
    static hipError_t create(uint32_t** w, unsigned flags) {
        hipError_t e = hipHostMalloc((void**)w, BYTES, flags);
        if (e == hipSuccess) {
            **w = 0u;
            g_live_pinned += BYTES;
        } else {
            *w = nullptr;
        }
        return e;
    }
    static void destroy(uint32_t* w) {
        (void)hipHostFree(w);
        g_live_pinned -= BYTES;
    }
};
using Stream = fx::Owned<StreamRes>;
using Event = fx::Owned<EventRes>;
using MappedWord = fx::Owned<MappedWordRes>;

// The host tail: the first `kh` queries of a batch's longest-first order are searched by host
// threads (fxjps_host_search.cpp) beside the device search, on host copies of the resident grid's maps.  One per context,
// behind a pointer (a context moves; threads, a mutex and atomics do not).  The threads of a batch are created before
// anything is launched -- a thread that cannot be created leaves the whole batch to the device -- wait for `go`, pull
// queries from `next` and are joined by whoever ends the batch: finish_search, an error path (drain_all) or the destructor.
// A query a thread did not finish keeps the watchdog's code in `len` and goes to the large pool like any other such code:
// a loaded or failing host costs speed, never a result.
constexpr uint32_t HOST_TAIL_MAX = 64, HOST_TAIL_THREADS_MAX = 12;
struct HostTail {
    // across batches
    uint32_t kh_cap = HOST_TAIL_MAX;  // halved by every batch whose host part outlasted the device's, doubled again (up to
                                      // HOST_TAIL_MAX) by 16 batches in a row whose host part was on time
    int late_run = 0;                 // late batches in a row (3: off for this handle, as solo_timeouts_run)
    int ontime_run = 0;               // batches on time in a row since the share last changed
    uint64_t maps_gen = ~0ull;        // DevCtx::map_gen the host copies were taken at
    fxh::Maps maps;
    HBuf<uint16_t> jd;
    HBuf<fx::BmWord> bm;
    HBuf<int32_t> comp;
    Stream stream;  // the map copies' own
    Event ev_grid, ev_maps;
    std::vector<uint32_t> lut;
    std::vector<std::unique_ptr<fxh::Searcher>> searchers;
    HBuf<uint32_t> path, ids;  // [kh][max_len] packed cells, [kh] query ids
    HBuf<int32_t> len;
    HBuf<double> cost;
    // the batch in progress
    std::vector<std::thread> threads;
    std::mutex mu;
    std::condition_variable cv;
    int go = 0;  // 0: wait, 1: search, -1: leave
    std::atomic<uint32_t> next{0}, ended{0};
    std::atomic<bool> cancel{false};
    std::atomic<unsigned long long> pops{0}, pushes{0};
    double t_first = 0, t_last = 0;  // first thread's start, last thread's end (under mu)
    uint32_t kh = 0;
    const int32_t *starts = nullptr, *goals = nullptr;
    const uint32_t* order = nullptr;
    int hchoice = 0, max_len = 0;
    uint64_t max_pops = 0;
    // ... and what it left for the timing record
    uint32_t done_kh = 0;
    double done_ms = 0;
    bool done_late = false;

    void work(size_t t) {
        {
            std::unique_lock<std::mutex> lk(mu);
            cv.wait(lk, [&] { return go != 0; });
            if (go < 0) return;
        }
        const double t0 = now_s();
        try {
            for (uint32_t i = next.fetch_add(1); i < kh && !cancel.load(std::memory_order_relaxed); i = next.fetch_add(1)) {
                const uint32_t q = order[i];
                const fxh::Result R = searchers[t]->plan(maps, lut.data(), hchoice, starts[2 * q], starts[2 * q + 1], goals[2 * q], goals[2 * q + 1],
                                                         max_len, path.p + (size_t)i * (size_t)max_len, max_pops);
                cost.p[i] = R.cost;
                len.p[i] = R.len;
                pops += R.pops;
                pushes += R.pushes;
            }
        } catch (...) {  // (std::bad_alloc in a table or a heap: the query keeps the watchdog's code)
        }
        const double t1 = now_s();
        std::lock_guard<std::mutex> lk(mu);
        t_first = ended.load() == 0 ? t0 : std::min(t_first, t0);
        t_last = ended.load() == 0 ? t1 : std::max(t_last, t1);
        ended++;
    }
    // T threads for the next batch, waiting; false (and none left) when one of them cannot be created
    bool spawn(size_t T) {
        go = 0;
        next = 0;
        ended = 0;
        cancel = false;
        pops = 0;
        pushes = 0;
        try {
            if (lut.empty()) {
                lut.resize(11 * 256);
                fxh::dirlut_fill(lut.data());
            }
            while (searchers.size() < T) searchers.emplace_back(new fxh::Searcher());
            threads.reserve(T);
            for (size_t t = 0; t < T; t++) threads.emplace_back([this, t] { work(t); });
        } catch (...) {  // std::system_error: no more threads; std::bad_alloc
            release(-1);
            return false;
        }
        return true;
    }
    void release(int how) {
        {
            std::lock_guard<std::mutex> lk(mu);
            go = how;
        }
        cv.notify_all();
        if (how < 0) join();
    }
    void join() {
        for (auto& t : threads)
            if (t.joinable()) t.join();
        threads.clear();
    }
    // an error path, or the end of the handle: whatever runs stops after its current query
    void abandon() {
        if (threads.empty()) return;
        cancel = true;
        release(go == 0 ? -1 : go);
        join();
        kh = 0;
        maps_gen = ~0ull;  // (a copy may not have landed: the next batch takes the maps again)
    }
    ~HostTail() { abandon(); }
};

struct ScratchCfg {
    uint32_t nwaves = 0;
    uint32_t nbuckets = 0;    // buckets per wavefront table (hashed: any number; cell-indexed: slots / BUCKET)
    uint32_t usable = 0;      // hashed: entries a search may insert (3/4 of a full-size table, 7/8 of a shrunk one)
    uint32_t direct_ly = 0;  // > 0: the table is indexed by the cell (slot = x << direct_ly | y), see ensure_pool
    uint32_t far_cap = 0;
};

// A grid on one device and its derived maps: the handle's resident grid (DevCtx derives from it) or a grid slot.
struct GridBufs {
    int W = 0, H = 0, PW = 0, PH = 0, NS = 0, LINES = 0, WORDS = 0, tsh = 0;
    DBuf<uint8_t> occ, nb8;
    DBuf<fx::BmWord> bm;
    DBuf<int> comp;
    DBuf<uint16_t> ci;
    DBuf<uint16_t> jd;  // jump distances [PW][NS][8] (k_derive_jd)
    void release() { *this = GridBufs(); }  // an empty slot: extents zero, memory returned at once
};

struct DevCtx : GridBufs {
    int dev = -1;
    int n_cu = 256;
    int share = 1;  // contexts of this handle on the same physical device (they split its memory and wavefront slots)
    size_t mem_total = 0;
    // (the streams stand in front of every buffer: members go in reverse order, so the buffers are freed while they exist)
    Stream stream;
    Stream stream_solo;                 // the launch of the longest queries, one wavefront per CU, beside the batch's launch
    MappedWord solo_started;            // pinned host word: blocks of such launches that have started (only ever counts up)
    uint32_t solo_target = 0;           // ... and how many have been launched
    int solo_timeouts = 0;              // waits for that counter that ran into their 5 ms bound, since the handle was created
    int solo_timeouts_run = 0;          // ... in a row (3: no more head launches on this device; a cold first launch of a
                                        // kernel -- its code object is loaded then -- is a lone timeout and means nothing)
    size_t cells_bound = 0;             // bytes the batch in progress may still allocate for its packed paths
    bool lds_attr_done[16] = {};        // k_search instantiations whose dynamic-LDS limit has been raised on this device
    Event ev0, ev1, ev_solo0, ev_solo1;
    Event ev_hd0, ev_hd1, ev_bt0, ev_bt1;  // around the head launch / the batch's launch alone
    // grid slots (fxjps_set_grid_slot): their maps, and their descriptors on the device (what k_search<.., .., .., true> reads)
    std::vector<GridBufs> slots;  // [FXJPS_MAX_GRID_SLOTS] once the first slot is set; W == 0: empty
    std::vector<GridDev> h_slot_desc;
    DBuf<GridDev> d_slot_desc;
    DBuf<int32_t> d_grid_ids;
    // fxjps_prepare_slots / fxjps_refresh_slots: the call's staged input (fx::SlotTable | the 256 slot descriptors | the raw
    // maps | a world-frame call's fx::WorldSrcDev records | a refresh's `changed` words), pinned and on the device, and the per-job results of k_slots_goal
    // (fxjps_set_grid_slots / fxjps_refresh_grid_slots: the same, prepared grids where the raws are, and only the words come back)
    HBuf<uint8_t> h_slots_in;
    DBuf<uint8_t> d_slots_in;
    HBuf<int32_t> h_slots_res;
    size_t slot_tiles_at = 0;  // the last slots call's tile records begin at this word of h_slots_res (fxjps_set_slot_reuse(1))
    DBuf<int32_t> d_slots_res;
    // fxjps_prepare_slots_cropped / fxjps_refresh_slots_cropped, first phase: the staged input (fx::CropTable | n box records
    // | the messages), the windows k_crop_window cuts out of them (what the second phase's gather reads as its raws), and
    // the box records on their way back
    HBuf<uint8_t> h_crop_in;
    DBuf<uint8_t> d_crop_in, d_crop_win;
    HBuf<int32_t> h_crop_box;
    // prior maps (fxjps_set_prior_map): [W][H] bytes the world-frame calls gather from; W == 0: not set
    struct PriorBuf {
        DBuf<uint8_t> occ;
        int W = 0, H = 0;
        DBuf<uint8_t> next;  // fxjps_absorb_prior_grow: the grown prior on its way in; swapped with occ once every context has
                             // succeeded, and afterwards the spare the next grow writes into
    };
    std::vector<PriorBuf> priors;  // [FXJPS_MAX_PRIOR_MAPS] once the first prior is set
    // fxjps_publish_slots: the call's job table (fx::PubTable) and all its outputs, pinned and on the device
    HBuf<uint8_t> h_pub_in, h_pub_out;
    DBuf<uint8_t> d_pub_in, d_pub_out;
    // search scratch (two pools: the regular one and the large retry one)
    DBuf<TEnt> tables[2];
    DBuf<FarEnt> far[2];
    DBuf<uint32_t> wave_gen[2];
    ScratchCfg cfg[2];
    int cfg_W = 0, cfg_H = 0;  // the batch extents (BatchReq::W / H) pool 0 was last configured for
    bool pool_clean[2] = {false, false};
    // batch buffers
    DBuf<int32_t> d_starts, d_goals, d_len, d_cells;
    DBuf<double> d_cost;
    DBuf<uint32_t> d_path, d_order, d_redo;
    DBuf<long long> d_offsets;
    DBuf<unsigned int> d_next;
    DBuf<unsigned long long> d_counters, d_qstat, d_qread;
    // fxjps_replan_slots: the previous full batch's results (the set that d_len / d_cost / d_offsets / d_cells flip with), the
    // sub-batch's lengths and costs, and which of the two each query of the full batch takes (fx::ReplanSrc::src)
    DBuf<int32_t> p_len, p_cells, s_len, d_rs_src;
    DBuf<double> p_cost, s_cost;
    DBuf<long long> p_offsets;
    HBuf<int32_t> h_rs_src;
    std::vector<unsigned long long> h_qread;  // read sets of the resident results (streaming replan)
    std::vector<uint8_t> h_sel;   // BatchReq::mode 2: which queries of the shard are searched again this frame
    DBuf<uint8_t> d_raw, d_img;
    // fxjps_refresh_grid (context 0 only): the diff kernels' buffer (fx::DIFF_HDR header words | the list | the blocks' counts)
    // and where its header and the head of the list arrive on the host
    DBuf<uint32_t> d_diff;
    HBuf<uint32_t> h_diff;
    struct Waypoints {
        // waypoint selection over a batch (fxjps_waypoint_ccst_batch)
        DBuf<double> d_in, d_out;
        DBuf<int32_t> d_eo, d_nkept, d_kept, d_cells, d_len;
        DBuf<long long> d_off;
        // ... the st rule (fxjps_waypoint_st_batch): per-query inputs / outputs, and the host libm's atan2 of integer pairs
        DBuf<int32_t> d_ms, d_pdim, d_dim;
        DBuf<double> d_prev, d_ang, d_atab;
        int atab_a = -1, atab_b = -1;  // d_atab holds atan2(a, b) for a in [0, atab_a], b in [-atab_b, atab_b]
        // ... both rules over a slots batch (fxjps_waypoint_slots_batch): the call's staged input (fx::WpSlotQuery per query |
        // the caller's offsets | cells) and output (fx::WpSlotResult per query | the kept cells), pinned and on the device
        HBuf<uint8_t> h_recs_in, h_recs_out;
        DBuf<uint8_t> d_recs_in, d_recs_out;
    } wp;
    DBuf<int32_t> d_upd_xy;
    DBuf<uint8_t> d_upd_chg;
    DBuf<int> d_owner;        // [W][H], -1 at rest: which entry of an update list decides a cell it names several times
    bool owner_ready = false;
    // a partial rebuild's changed cells (k_derive_cellinfo -> k_jd_walk): marks [PW][NS], zero at rest; their list; counters
    DBuf<uint8_t> d_chgmap;
    DBuf<uint32_t> d_chglist;
    DBuf<unsigned int> d_chgcnt;
    DBuf<uint32_t> d_chgovf;  // walks handed on to k_jd_finish: 2 words each
    bool chg_ready = false;
    // what the cell updates since the last rebuild of the derived maps can have changed: the box, in padded
    // coordinates, of the updated cells and their neighbours; whether the component labels need the full relabelling (a
    // large update, or 64 small ones, which are united into the existing labels as they come: k_ccl_update)
    bool dirty = false;
    int bx0 = 0, bx1 = 0, by0 = 0, by1 = 0;
    bool ccl_full = false;
    int ccl_small = 0;
    // pinned staging of a cell-update list: the caller's arrays are copied here before the asynchronous H2D copy, so
    // that they need not outlive the call (ev_upd: the last copy out of the staging buffers has completed)
    HBuf<int32_t> h_upd_xy;
    Event ev_upd;
    HBuf<uint8_t> h_occ_stage;      // a small grid on its way to the device (fxjps_set_grid returns while it travels)
    Event ev_stage;                 // ... the copy out of it has completed
    bool stage_pending = false;
    Event ev_ccl0, ev_ccl1;  // a whole map build: the component labels on the second stream, beside the maps
    bool upd_pending = false;
    HBuf<int32_t> h_len, h_cells;
    HBuf<uint32_t> h_path1;       // single calls: the search kernel writes the packed path of its one query here
    HBuf<double> h_cost;
    HBuf<long long> h_offsets;
    HBuf<unsigned long long> h_counters;
    // A plain batch streams its results: the search kernel leaves every finished path in h_arena
    // (packed cells, x << 16 | y, wherever d_cursor stood) and its place in h_base, its length in h_len, its cost in h_cost.
    // h_cells and the device CSR (d_offsets / d_cells) are then built by whoever asks first: host_cells / device_csr.
    HBuf<uint32_t> h_arena;
    HBuf<long long> h_base;
    DBuf<unsigned long long> d_cursor;
    long long arena_peak = 0;  // the largest total of cells a batch of this context has produced
    struct Streaming {         // the batch in progress streams: what fill_search_args hands the kernel (device pointers)
        bool on = false;
        uint32_t* cells = nullptr;
        unsigned long long cap = 0;
        long long* base = nullptr;
        int32_t* len = nullptr;
        double* cost = nullptr;
        unsigned long long* counters = nullptr;
    } st;
    bool cells_on_host = true, csr_on_device = true;  // h_cells / d_offsets and d_cells hold the last batch (false: only the arena does)
    int last_max_len = 0;                             // ... whose path slots in d_path are this long
    std::vector<uint32_t> h_order;
    // shard of the current batch
    int64_t q0 = 0, nq = 0;
    int wall_khz = 100000;  // hipDeviceAttributeWallClockRate (wall_clock64 ticks per ms)
    // ... and what its run left for the handle's timing record (collect_timing)
    struct RunStats {
        double kernel_ms = 0;
        int64_t launches = 0, retried = 0;
        int64_t nrun = 0;          // queries handed to the search kernel
        uint32_t waves_used = 0;   // resident wavefronts of the last regular-pool launch
        bool waves_short = false;  // a scratch pool was granted fewer wavefronts than the batch asked for (memory budget / out of memory)
        bool had_solo = false;     // the last regular-pool launch was two launches
        double head_ms = 0, batch_ms = 0;  // ... and how long each of them ran
    } run;
    // fxjps_absorb_prior: the call's staged input (fx::AbsorbTable | the rows of each raw that hold its rectangle), pinned
    // and on the device, and the table's counters on their way back (fxjps_absorb_prior_grow: the same with a fx::GrowTable)
    HBuf<uint8_t> h_absorb_in;
    DBuf<uint8_t> d_absorb_in;
    HBuf<unsigned long long> h_absorb_out;
    // the host tail: the generation of the resident grid's maps (moved by every call that writes the grid or its maps:
    // alloc_grid, derive_maps, update_cells_async -- every set_grid*, update_cells*, prepare_*, refresh_* and replan_frame*
    // goes through one of them), and the tail's state once a batch has used it (last: destroyed first, while the streams exist)
    uint64_t map_gen = 0;
    std::unique_ptr<HostTail> tail;

    DevCtx() = default;
    DevCtx(DevCtx&&) = default;  // (std::vector<DevCtx>::resize; nothing moves a context that is in use)
    DevCtx& operator=(DevCtx&&) = default;
    // Whatever is queued may still use the buffers: both streams are drained, then every member gives back what it holds,
    // with the context's device current.
    ~DevCtx() {
        if (tail) tail->abandon();
        if (dev < 0) return;
        (void)hipSetDevice(dev);
        if (tail && tail->stream) (void)hipStreamSynchronize(tail->stream);  // (a map copy reads the grid's buffers)
        if (stream_solo) (void)hipStreamSynchronize(stream_solo);
        if (stream) (void)hipStreamSynchronize(stream);
    }
};

}  // namespace

struct fxjps {
    std::vector<DevCtx> devs;
    std::string err;
    std::mutex err_mu;  // the shards of a multi-device batch run on one host thread each: whichever fails last leaves its text
    bool have_grid = false;
    bool maps_stale = false;  // cell updates were applied without rebuilding the derived maps (fxjps_update_cells_deferred)
    int mem_div = 1;          // handles sharing each device (fxjps_set_memory_share): the scratch budgets are divided by it
    fxjps_timing_t timing{};
    struct LastBatch {  // what the resident forms of the waypoint calls read (nq == 0 while a batch is under way: begin_batch)
        int64_t nq = 0;
        bool on_host = false;  // the last batch was a single call: its CSR is in the pinned host buffers only
        int W = 0, H = 0;      // the extents of the resident grid when a batch on it began: its paths lie on THAT grid, whatever is resident now
        bool slots = false;    // the last batch ran on grid slots: its paths are not the resident grid's ...
        int slots_W = 0, slots_H = 0;   // ... they lie within these extents (the largest of the slots it named)
        std::vector<int32_t> slot_ids;  // ... and these are the slots its queries named (fxjps_waypoint_slots_batch)
    } last;
    // persistent query set of the streaming-replan entry points (fxjps_set_queries / fxjps_replan_frame)
    std::vector<int32_t> q_starts, q_goals;
    int q_hchoice = 0, q_max_len = 0;
    bool q_set = false;
    // true while the device result buffers and the host read sets of every device describe the stored queries on the
    // resident grid: then a frame only searches the queries whose read set its cell updates touch
    bool q_results_valid = false;
    // fxjps_refresh_grid / fxjps_replan_frame_raw: the changed cells the last such call found and applied as a cell update
    // (mode 1; empty after any other mode), for fxjps_last_refresh_cells
    std::vector<int32_t> refresh_xy;
    std::vector<uint8_t> refresh_val;
    // fxjps_replan_slots: the previous such call's arguments, the generation of each query's slot then, and its per-query
    // codes; rs_valid while the device buffers of context 0 still hold that batch (whatever drops q_results_valid drops it)
    std::vector<int32_t> rs_ids, rs_starts, rs_goals, rs_len;
    std::vector<uint64_t> rs_gen;
    int64_t rs_nq = 0;
    int rs_hchoice = 0, rs_max_len = 0;
    bool rs_valid = false;
    // per-slot generation: bumped by every call that writes a slot's bytes or maps on any context (a release included)
    uint64_t slot_gen[FXJPS_MAX_GRID_SLOTS] = {};
    // fxjps_set_slot_reuse.  Mode 1: per slot, the read-set tiles that the compared refresh jobs
    // since generation `base` found changed (FrameTiles' layout); valid while every write of the slot since then was such a
    // job.  Per query of the stored fxjps_replan_slots results, the read set of the search that produced it (rs_have: it has
    // one -- a query that ended without a search has none).
    struct SlotTiles {
        bool valid = false;
        uint64_t base = 0;
        unsigned long long D[128] = {};  // DX[64] (a bit per x tile), then DY[64]
    };
    int slot_reuse = 0;
    std::vector<SlotTiles> slot_tiles = std::vector<SlotTiles>(FXJPS_MAX_GRID_SLOTS);
    std::vector<unsigned long long> rs_read;
    std::vector<uint8_t> rs_have;
    // a slot is written by anything but a compared refresh job: its generation moves and its tile record is void
    void bump_slot(int32_t slot) {
        slot_gen[(size_t)slot]++;
        slot_tiles[(size_t)slot].valid = false;
    }
    // ... by a compared refresh job whose changed bytes touch the tiles of `rec`
    void mark_slot(int32_t slot, const unsigned long long* rec) {
        slot_gen[(size_t)slot]++;
        for (int t = 0; t < 128; t++) slot_tiles[(size_t)slot].D[t] |= rec[t];
    }
    // RCCL (only for n_dev > 1), resolved with dlopen so that a single-GPU
    // deployment does not need librccl at load time
    void* rccl = nullptr;
    std::vector<void*> comms;
    // one process per GPU without torch (fxjps_create_rank): this handle is rank `rank` of `world`, its one communicator
    // (comms[0]) was made with ncclCommInitRank from the id rank 0 handed out
    int rank = -1, world = 0;

    ~fxjps() {  // the communicators first, then the contexts (their streams may be the ones a broadcast ran on)
        if (!rccl) return;
        auto destroy = (int (*)(void*))dlsym(rccl, "ncclCommDestroy");
        if (destroy)
            for (void* c : comms)
                if (c) destroy(c);
    }
};

namespace {

int fail(fxjps* h, int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    if (h) {
        std::lock_guard<std::mutex> lk(h->err_mu);
        h->err = buf;
    } else {
        g_create_error = buf;
    }
    return code;
}

#define HIPCHK(h, call)                                                                          \
    do {                                                                                         \
        hipError_t e__ = (call);                                                                 \
        if (e__ != hipSuccess)                                                                   \
            return fail(h, e__ == hipErrorOutOfMemory ? FXJPS_E_NOMEM : FXJPS_E_HIP, "%s: %s (%s:%d)", \
                        #call, hipGetErrorString(e__), __FILE__, __LINE__);                      \
    } while (0)

// nodeNeighbours (jps1.py:49-93) as a table: one definition for the device's table and the host search (fxjps_host_search.cpp)
using fxh::dirlut_entry;
static_assert(fxh::PD_NONE == fx::PD_NONE && fxh::DIR_NONE == fx::DIR_NONE && fxh::QI_WATCHDOG == fx::QI_WATCHDOG &&
                  sizeof(fxh::BmWord) == sizeof(fx::BmWord),
              "the host search reads the device's maps and codes");

GridDev grid_of(const GridBufs& d) {
    GridDev G;
    G.bm = d.bm.p;
    G.ci = d.ci.p;
    G.nb8 = d.nb8.p;
    G.jd = d.jd.p;
    G.comp = d.comp.p;
    G.W = d.W;
    G.H = d.H;
    G.PW = d.PW;
    G.PH = d.PH;
    G.NS = d.NS;
    G.LINES = d.LINES;
    G.WORDS = d.WORDS;
    G.DLINES = d.PW + d.PH - 1;
    G.tsh = d.tsh;
    return G;
}

// (re)build nb8, the scan bitmaps, the cell infos and the component labels from d.occ.  whole == false: only what the
// cell updates since the last rebuild can have changed (DevCtx::dirty and its box) -- the neighbour bytes and scan
// words of the box, the cell infos of the rows and columns through it; the labels were kept up to date by
// k_ccl_update unless a full relabelling is due.
// slot != nullptr: the whole build of a grid slot's maps on d's streams (the same kernels; d's update state untouched).
int derive_maps(fxjps* h, DevCtx& d, bool whole = true, GridBufs* slot = nullptr) {
    HIPCHK(h, hipSetDevice(d.dev));
    GridBufs& g = slot ? *slot : d;
    if (slot) whole = true;
    if (!slot) d.map_gen++;
    if (!whole && !d.dirty && !d.ccl_full) return FXJPS_OK;
    const bool box = !whole && d.dirty && (d.bx1 - d.bx0 + 1) * 2 <= g.PW && (d.by1 - d.by0 + 1) * 2 <= g.PH;
    const GridDev G = grid_of(g);
    // A whole build (a new grid): the component labels need nothing but the occupancy bytes, the five map kernels nothing of
    // the labels -- the three label kernels run on the handle's second stream beside them and join in front of whatever is
    // queued next (round 6: 27 of the 76 us of a 256 x 256 build; 221 of 382 us at 1024 x 1024).
    // A small grid: four launches instead of eight (k_build_1 .. 3, then k_derive_jd): what a build of tiny kernels waits for
    // is the runtime launching them one by one.  FXJPS_FUSED_BUILD=0: the separate kernels (test / measurement aid).
    const char* fused_env = getenv("FXJPS_FUSED_BUILD");  // (read per build: the tests compare the two forms in one process)
    if (whole && !(fused_env && atoi(fused_env) == 0) && (long long)g.W * g.H <= (1ll << 18)) {
        const long long ncell = (long long)g.W * g.H, npad = (long long)g.PW * g.PH;
        const unsigned nb_rows = (unsigned)(((long long)g.PW * g.WORDS + 3) / 4), nb_cols = (unsigned)(((long long)g.PH * g.WORDS + 3) / 4);
        const unsigned nb_cell = (unsigned)((ncell + 255) / 256), nb_ci = (unsigned)((npad + 255) / 256);
        const unsigned nb_diag = (unsigned)((4ll * G.DLINES * g.WORDS + 15) / 16), nb_flat = (unsigned)((ncell + 1023) / 1024);
        hipLaunchKernelGGL(fx::k_build_1, dim3(nb_rows + nb_cols + nb_cell), dim3(256), 0, d.stream, g.occ.p, G, g.nb8.p, g.bm.p, g.comp.p, nb_rows, nb_cols);
        hipLaunchKernelGGL(fx::k_build_2, dim3(nb_ci + nb_cell), dim3(256), 0, d.stream, g.occ.p, G, g.ci.p, g.comp.p, nb_ci);
        hipLaunchKernelGGL(fx::k_build_3, dim3(nb_diag + nb_flat), dim3(1024), 0, d.stream, g.occ.p, G, g.bm.p + (size_t)4 * g.LINES * g.WORDS, g.comp.p, nb_diag);
        hipLaunchKernelGGL(fx::k_derive_jd, dim3((unsigned)((npad * 8 + 255) / 256)), dim3(256), 0, d.stream, G, g.jd.p, fx::DiagRange{1, d.bx0, d.bx1, d.by0, d.by1});
        HIPCHK(h, hipGetLastError());
        if (!slot) {
            d.ccl_small = 0;
            d.dirty = false;
            d.ccl_full = false;
        }
        return FXJPS_OK;
    }
    const bool ccl_beside = whole && d.stream_solo != nullptr && d.ev_ccl0 != nullptr;
    const auto launch_ccl = [&](hipStream_t st) {
        const long long n = (long long)g.W * g.H;
        const unsigned nb = (unsigned)((n + 255) / 256);
        hipLaunchKernelGGL(fx::k_ccl_init, dim3(nb), dim3(256), 0, st, g.occ.p, n, g.H, g.comp.p);
        hipLaunchKernelGGL(fx::k_ccl_merge, dim3(nb), dim3(256), 0, st, g.occ.p, g.W, g.H, g.comp.p);
        hipLaunchKernelGGL(fx::k_ccl_flatten, dim3(nb), dim3(256), 0, st, n, g.comp.p);
    };
    if (ccl_beside) {
        HIPCHK(h, hipEventRecord(d.ev_ccl0, d.stream));  // (behind the copy / broadcast that brought the grid)
        HIPCHK(h, hipStreamWaitEvent(d.stream_solo, d.ev_ccl0, 0));
        launch_ccl(d.stream_solo);
        HIPCHK(h, hipEventRecord(d.ev_ccl1, d.stream_solo));
    }
    if (whole || d.dirty) {
        fx::MapRange rr{0, g.PW - 1, 0, g.WORDS - 1}, rc{0, g.PH - 1, 0, g.WORDS - 1};
        if (box) {
            rr = fx::MapRange{d.bx0, d.bx1, d.by0 >> 6, d.by1 >> 6};
            rc = fx::MapRange{d.by0, d.by1, d.bx0 >> 6, d.bx1 >> 6};
        }
        const long long nrw = (long long)(rr.l1 - rr.l0 + 1) * (rr.w1 - rr.w0 + 1), ncw = (long long)(rc.l1 - rc.l0 + 1) * (rc.w1 - rc.w0 + 1);
        hipLaunchKernelGGL(fx::k_derive_rows, dim3((unsigned)((nrw + 3) / 4)), dim3(256), 0, d.stream, g.occ.p, G, g.nb8.p, g.bm.p, rr);
        hipLaunchKernelGGL(fx::k_derive_cols, dim3((unsigned)((ncw + 3) / 4)), dim3(256), 0, d.stream, g.occ.p, G, g.bm.p, rc);
        fx::ChangeOut chg{nullptr, nullptr, nullptr, 0u, fx::MapRange{1, 0, 1, 0}};
        if (box) {  // the rows and the columns through the box (a straight jump ends where the line's next stop bit is)
            const fx::MapRange sa{d.bx0, d.bx1, 0, g.PH - 1}, sb{0, g.PW - 1, d.by0, d.by1};
            const long long na = (long long)(sa.l1 - sa.l0 + 1) * g.PH, nb = (long long)g.PW * (sb.w1 - sb.w0 + 1);
            // ... and which of those cells changed: where the re-scan of the jump distances starts (k_jd_walk)
            const bool walk = !(getenv("FXJPS_JD_WALK") && atoi(getenv("FXJPS_JD_WALK")) == 0);  // (0: measurement / test aid -- every record is read)
            if (walk) {
                // The change list is an optimisation with buffers of its own (up to 4 bytes per cell of the cross: 67 MB for
                // a half-map box at 4096^2): when the device has no room for them -- pool 0 of a lone handle may hold 80 % of
                // it -- the update does not fail, it takes round 4's way (every word of the diagonals through the cross
                // rebuilt, every record read: chg.map stays nullptr).
                bool room = true;
                if (!d.chg_ready) {  // (streaming callers only: with the first partial rebuild on a grid)
                    room = d.d_chgmap.ensure((size_t)g.PW * g.NS) == hipSuccess && d.d_chgcnt.ensure(4) == hipSuccess;
                    if (room) {
                        HIPCHK(h, hipMemsetAsync(d.d_chgmap.p, 0, (size_t)g.PW * g.NS, d.stream));
                        HIPCHK(h, hipMemsetAsync(d.d_chgcnt.p, 0, 4 * sizeof(unsigned int), d.stream));
                        d.chg_ready = true;
                    }
                }
                room = room && d.d_chglist.ensure((size_t)(na + nb)) == hipSuccess;
                constexpr uint32_t OVF_CAP = 16384;  // long walks handed on per update (2 words each); beyond it the records are streamed
                room = room && d.d_chgovf.ensure((size_t)2 * OVF_CAP) == hipSuccess;
                if (room) {
                    chg = fx::ChangeOut{d.d_chgmap.p, d.d_chglist.p, d.d_chgcnt.p, (uint32_t)(na + nb), fx::MapRange{d.bx0, d.bx1, d.by0, d.by1}, d.d_chgovf.p, OVF_CAP};
                    if (const char* e = getenv("FXJPS_JD_OVF_CAP")) chg.ovf_cap = (uint32_t)std::min(std::max(atoi(e), 0), (int)OVF_CAP);  // (test aid)
                } else
                    (void)hipGetLastError();  // (the failed allocation's sticky error: not this update's business)
            }
            hipLaunchKernelGGL(fx::k_derive_cellinfo, dim3((unsigned)((na + nb + 255) / 256)), dim3(256), 0, d.stream, G, g.ci.p, sa, sb, chg);
        } else {
            const long long ncell = (long long)g.PW * g.PH;
            hipLaunchKernelGGL(fx::k_derive_cellinfo, dim3((unsigned)((ncell + 255) / 256)), dim3(256), 0, d.stream, G, g.ci.p,
                               fx::MapRange{0, g.PW - 1, 0, g.PH - 1}, fx::MapRange{1, 0, 1, 0}, chg);
        }
        {  // the diagonal scan words: a function of the cell infos (and the occupancy) cell by cell -- of the cells above
            const fx::DiagRange dr{box ? 0 : 1, d.bx0, d.bx1, d.by0, d.by1};
            const long long per = box ? (long long)((d.bx1 >> 6) - (d.bx0 >> 6) + 1) + (((d.by1 - d.by0 + 63) >> 6) + 1) : (long long)g.WORDS;
            const long long nw = 4ll * G.DLINES * per;
            if (box && chg.map != nullptr)  // (the changed cells alone, bit by bit)
                hipLaunchKernelGGL(fx::k_diag_update, dim3((unsigned)std::min<long long>(((long long)chg.cap * 4 + 255) / 256, 256)), dim3(256), 0, d.stream,
                                   g.occ.p, G, g.bm.p + (size_t)4 * g.LINES * g.WORDS, chg);
            else
                hipLaunchKernelGGL(fx::k_derive_diag, dim3((unsigned)((nw + 15) / 16)), dim3(1024), 0, d.stream, g.occ.p, G,
                                   g.bm.p + (size_t)4 * g.LINES * g.WORDS, dr);
            // ... and the jump distances: the goal-free jumps themselves, from every cell along every direction, read off
            // the scan words above (after an update: the entries whose old ray passes what the update can have changed)
            if (box && chg.map != nullptr) {
                // what the update can have changed, found from the changed cells backwards (a walker per changed cell and
                // direction) instead of by reading every record
                const int walk_max = getenv("FXJPS_JD_WALK_MAX") ? std::max(1, atoi(getenv("FXJPS_JD_WALK_MAX"))) : FXJPS_JD_WALK_MAX;  // (test aid)
                const long long nt = (long long)chg.cap * 8, nc = (long long)g.W * g.H;
                // (walks pay while the changed cells are few against the table: past W * H / 128 of them the records are streamed
                // -- measured at 4096^2 over obstacle densities 0 ... 0.2, profiles/r06_map_build.txt)
                const int div = getenv("FXJPS_JD_STREAM_DIV") ? std::max(1, atoi(getenv("FXJPS_JD_STREAM_DIV"))) : 128;  // (measurement / test aid)
                const uint32_t stream_over = (uint32_t)std::max<long long>(nc / div, 1024);
                hipLaunchKernelGGL(fx::k_jd_walk, dim3((unsigned)std::min<long long>((nt + 255) / 256, 2048)), dim3(256), 0, d.stream, G, g.jd.p, chg, dr, walk_max, stream_over);
                hipLaunchKernelGGL(fx::k_jd_finish, dim3((unsigned)std::min<long long>((nc + 255) / 256, 1024)), dim3(256), 0, d.stream, G, g.jd.p, chg, dr);
            } else if (box) {
                const long long nc = (long long)g.W * g.H;
                hipLaunchKernelGGL(fx::k_update_jd, dim3((unsigned)((nc + 255) / 256)), dim3(256), 0, d.stream, G, g.jd.p, dr);
            } else {
                const long long nj = (long long)g.PW * g.PH * 8;
                hipLaunchKernelGGL(fx::k_derive_jd, dim3((unsigned)((nj + 255) / 256)), dim3(256), 0, d.stream, G, g.jd.p, dr);
            }
        }
        HIPCHK(h, hipGetLastError());
    }
    if (ccl_beside) {
        HIPCHK(h, hipStreamWaitEvent(d.stream, d.ev_ccl1, 0));  // the join: whatever is queued on the main stream next sees the labels
        HIPCHK(h, hipGetLastError());
        if (!slot) d.ccl_small = 0;
    } else if (whole || d.ccl_full) {
        // component labels for the unreachable-goal early-out
        launch_ccl(d.stream);
        HIPCHK(h, hipGetLastError());
        if (!slot) d.ccl_small = 0;
    }
    if (slot) return FXJPS_OK;  // (the resident grid's update state is not the slot's business)
    d.dirty = false;
    d.ccl_full = false;
    return FXJPS_OK;
}

// the extents and the buffers of a W x H grid (the resident grid's or a slot's; the current device)
int alloc_grid_bufs(fxjps* h, GridBufs& d, int W, int H) {
    d.W = W;
    d.H = H;
    d.PW = W + 2;
    d.PH = H + 2;
    d.NS = (d.PH + 63) & ~63;
    d.LINES = std::max(d.PW, d.PH);
    d.WORDS = (std::max(d.PW, d.PH) + 63) / 64;
    d.tsh = 0;  // read-set tiles (streaming replan): at most 64 x 64 of them cover the grid
    while (((std::max(W, H) - 1) >> d.tsh) > 63) d.tsh++;
    HIPCHK(h, d.occ.ensure((size_t)W * H));
    HIPCHK(h, d.comp.ensure((size_t)W * H));
    HIPCHK(h, d.nb8.ensure((size_t)d.PW * d.NS));
    HIPCHK(h, d.ci.ensure((size_t)d.PW * d.NS));
    HIPCHK(h, d.jd.ensure((size_t)d.PW * d.NS * 8));
    HIPCHK(h, d.bm.ensure((size_t)4 * d.LINES * d.WORDS + (size_t)4 * (d.PW + d.PH - 1) * d.WORDS));  // straight + diagonal scan lines
    return FXJPS_OK;
}

int alloc_grid(fxjps* h, DevCtx& d, int W, int H) {
    HIPCHK(h, hipSetDevice(d.dev));
    d.map_gen++;
    // The search scratch is sized by the grid's shape.  A new grid of the SAME shape keeps the pools as they are -- what
    // earlier searches left in the visited tables carries their generation tags and reads as empty, exactly as between two
    // batches on one grid -- so a caller that uploads a changed map every tick (jps1.method) does not pay for sizing and
    // wiping them again (~ 100 us of such a call); another shape makes the next batch size them anew.
    // (While one of the tests' sizing knobs is set every new grid makes the next batch size the pools anew, as before.)
    bool knob = false;
    for (const char* k : {"FXJPS_TABLE_LOG2", "FXJPS_TABLE_SHIFT", "FXJPS_FAR_CAP", "FXJPS_POOL_BUDGET_MB", "FXJPS_POOL_FRAC", "FXJPS_DIRECT",
                          "FXJPS_TABLE_SHRINK"})
        knob = knob || getenv(k) != nullptr;
    if (W != d.W || H != d.H || knob) {
        d.pool_clean[0] = d.pool_clean[1] = false;
        d.cfg[0] = ScratchCfg();
        d.cfg[1] = ScratchCfg();
        d.owner_ready = false;  // (the update lists' owner cells follow the grid's shape -- and are all -1 between two updates,
        d.chg_ready = false;    // as the marks of the changed cells are all zero: a grid of the same shape finds them in order)
    }
    return alloc_grid_bufs(h, d, W, H);
}

// wavefront counts are whole blocks of fx::WPB wavefronts (any block size: a measurement build runs ten per block)
constexpr uint64_t wpb_down(uint64_t v) { return v / (uint64_t)fx::WPB * (uint64_t)fx::WPB; }
constexpr uint64_t wpb_up(uint64_t v) { return wpb_down(v + (uint64_t)fx::WPB - 1u); }

uint32_t ceil_log2(uint64_t v) {
    uint32_t l = 0;
    while ((1ull << l) < v) l++;
    return l;
}

// What a planning call asks for, complete and checked before anything is queued (batch_request); every function of the
// planning path reads it, none changes it -- the shards of a several-context batch share it across their host threads.
struct BatchReq {
    const int32_t *starts = nullptr, *goals = nullptr;  // the caller's arrays, borrowed for the call
    int64_t nq = 0;
    int hchoice = 0, max_len = 0;
    int mode = 0;        // 0 plain batch, 1 search everything and record read sets, 2 the same for DevCtx::h_sel only
    bool slots = false;  // every query runs on the grid slot it names, not on the resident grid
    const int32_t* grid_ids = nullptr;  // ... these (the caller's array; may be NULL when nq == 0)
    // the extents the scratch, the watchdog and the far band's form are sized for: the resident grid's, or the largest
    // among the slots the batch names
    int W = 0, H = 0;
    uint64_t cells = 0;
    bool track() const { return mode != 0; }
    bool stream = false;  // plan_core: a plain batch, its results go to the host as the queries end (DevCtx::st)
};

// Gives the memory of pool 0 back (a batch buffer did not fit beside it); the next batch sizes it again from what is free.
void release_pool0(DevCtx& d) {
    if (d.stream_solo) (void)hipStreamSynchronize(d.stream_solo);
    (void)hipStreamSynchronize(d.stream);
    d.tables[0].release();
    d.far[0].release();
    d.wave_gen[0].release();
    d.cfg[0] = ScratchCfg();
    d.pool_clean[0] = false;
}

// Room for a batch buffer that pool 0 may be in the way of (the scratch of an earlier, smaller batch, or of a search that
// is over): when it does not fit, the pool's memory is given back and the buffer tried again.
template <typename T>
int ensure_beside_pool0(fxjps* h, DevCtx& d, DBuf<T>& buf, size_t n) {
    if (buf.ensure(n) != hipSuccess) {
        (void)hipGetLastError();
        release_pool0(d);
        HIPCHK(h, buf.ensure(n));
    }
    return FXJPS_OK;
}

// Size the per-wavefront scratch.  pool 0: many wavefronts, tables sized for the
// typical query; pool 1: few wavefronts, tables that cannot overflow.
// (A slots batch sizes them from the largest extents among the slots it names: BatchReq::W / H / cells.)
int ensure_pool(fxjps* h, DevCtx& d, const BatchReq& req, int pool, uint32_t want_waves) {
    const uint64_t cells = req.cells;
    ScratchCfg c;
    // Memory budget.  A handle that has the device to itself gives pool 0 up to 80 % of it, less what the batch still
    // has to allocate behind the search (the packed paths: at most nq * max_len cells), the smallest retry pool and a
    // margin -- on grids with hashed tables the number of resident wavefronts is what this budget buys, and the plans/s
    // of config 3 follow it almost linearly (1 536 / 2 270 / 2 840 wavefronts: 5.2 k / 7.5 k / 8.7 k plans/s).  Handles
    // that share a device keep to 60 % of their share.  Pool 1 (allocated while pool 0 stays resident) is sized from
    // what is free right now plus what it already holds, so that the two pools share one budget.  A batch buffer that
    // does not fit later takes the memory back (release_pool0 in run_shard).
    const size_t div = (size_t)(d.share * h->mem_div);
    double frac = div == 1 ? 0.8 : 0.6;
    if (const char* e = getenv("FXJPS_POOL_FRAC")) frac = std::min(0.95, std::max(0.05, atof(e)));  // measurement aid
    size_t budget = (d.mem_total ? (size_t)(d.mem_total * frac) : ((size_t)64 << 30)) / div;
    size_t free_b = 0, total_b = 0;
    const bool have_info = hipMemGetInfo(&free_b, &total_b) == hipSuccess;
    if (pool == 0 && div == 1 && have_info) {
        const size_t held = d.tables[0].cap * sizeof(TEnt) + d.far[0].cap * sizeof(FarEnt);
        const uint32_t l2r = std::max(ceil_log2(cells * 2 + 64), 12u);
        const size_t retry_wave = ((size_t)1 << l2r) * sizeof(TEnt) + (size_t)((cells * 2 + 1024) * 9 / 8) * sizeof(FarEnt);
        const size_t reserve = (size_t)fx::WPB * retry_wave + d.cells_bound + ((size_t)6 << 30);
        const size_t avail = free_b + held;
        budget = std::min(budget, avail > reserve ? avail - reserve : (size_t)0);
        budget = std::max(budget, std::min((size_t)(d.mem_total * 0.25), avail / 2));  // (never below what a shared device would get)
    }
    if (pool == 1 && have_info) {
        const size_t held = d.tables[1].cap * sizeof(TEnt) + d.far[1].cap * sizeof(FarEnt);
        budget = std::min(budget, (size_t)((free_b + held) * 0.9));
    }
    if (const char* e = getenv("FXJPS_POOL_BUDGET_MB")) budget = std::min<size_t>(budget, (size_t)std::max(1, atoi(e)) << 20);  // test aid
    if (pool == 0) {
        // measured on the config-2 workload (1024^2, 20 %): a reachable query inserts 34 k nodes
        // on average, 117 k at p99, 139 k at most, and keeps at most 2.4 k entries open; a table
        // of cells/4 entries (3/4 usable) covers all of them, the retry pool covers the rest
        uint32_t l2e = ceil_log2(std::max<uint64_t>(cells / 4, 1));  // entries
        // ... and up to four times that when a full set of wavefronts still fits in 40 % of the device: the hardest
        // queries fill half of a cells/4 table, where one 4-slot bucket in seven is full and the node that meets it
        // is committed by the slow general form (config 2: 152.9 -> 146.9 ms per 10 000 queries).
        {
            const uint64_t full = (uint64_t)d.n_cu * 4u * (uint64_t)fx::OCC / (uint64_t)(d.share * h->mem_div);
            const uint64_t cap = (d.mem_total ? (uint64_t)(d.mem_total * 0.4) : ((uint64_t)32 << 30)) / (uint64_t)(d.share * h->mem_div);
            uint32_t shift = 2;
            if (const char* e = getenv("FXJPS_TABLE_SHIFT")) shift = (uint32_t)std::max(0, atoi(e));  // measurement aid
            while (shift > 0 && full * (((uint64_t)19 << (l2e + shift))) > cap) shift--;  // 16-byte entries + the far tier (an eighth as many 18-byte entries)
            l2e += shift;
        }
        l2e = std::min(std::max(l2e, 12u), 23u);
        // A table with one slot per cell (slot = x << ly | y, both extents rounded up to powers of two) needs no
        // hashing, no buckets and cannot fill up: a probe is one 16-byte entry instead of a 64-byte bucket searched for
        // the cell.  Taken whenever a full set of wavefronts fits the same 40 % of the device with it (up to 2^20
        // slots: 1024^2, where it is exactly as large as the hashed table was); larger grids keep the hashed table.
        // FXJPS_DIRECT=0: measurement / test aid.
        {
            const uint32_t lx = std::max(ceil_log2((uint64_t)req.W), 1u), ly = std::max(ceil_log2((uint64_t)req.H), 1u);
            const uint32_t ld = std::max(lx + ly, 12u);
            const uint64_t full = (uint64_t)d.n_cu * 4u * (uint64_t)fx::OCC / (uint64_t)(d.share * h->mem_div);
            const uint64_t cap = (d.mem_total ? (uint64_t)(d.mem_total * 0.4) : ((uint64_t)32 << 30)) / (uint64_t)(d.share * h->mem_div);
            const bool allow = !(getenv("FXJPS_DIRECT") && atoi(getenv("FXJPS_DIRECT")) == 0) && !getenv("FXJPS_TABLE_LOG2");
            if (allow && ld <= 23u && full * ((uint64_t)19 << ld) <= cap) {
                l2e = ld;
                c.direct_ly = ly;
            }
        }
        // test aids: force a small table / far tier so that the overflow -> large-pool retry paths run
        if (const char* e = getenv("FXJPS_TABLE_LOG2")) l2e = (uint32_t)std::min(std::max(atoi(e), 4), 23);
        uint64_t entries = (uint64_t)1 << l2e;
        c.usable = (uint32_t)(entries / 4 * 3);
        // Hashed tables, and the wavefronts asked for do not fit the budget with them: the table shrinks, down to 3/4 of
        // its size (then filled up to 7/8 instead of 3/4: 88 % of the entries it could hold before), as far as it takes
        // to fit them.  The bucket count need not be a power of two (the hash is scaled to it).  Resident wavefronts are
        // what the plans/s of such grids follow (config 3, 4096^2: 2 270 wavefronts of 76 MB 7.5 k plans/s, 3 000 9.0 k;
        // the largest of its 100 000 queries inserts 2.42 M nodes, a shrunk table takes 2.75 M).  FXJPS_TABLE_SHRINK=0:
        // measurement aid.
        if (c.direct_ly == 0 && !getenv("FXJPS_TABLE_LOG2") && !(getenv("FXJPS_TABLE_SHRINK") && atoi(getenv("FXJPS_TABLE_SHRINK")) == 0)) {
            const uint64_t want = std::max<uint64_t>(wpb_up(want_waves), (uint64_t)fx::WPB);
            const double per_entry = (double)sizeof(TEnt) + (1.0 + 1.0 / 8) * sizeof(FarEnt) / 8.0;
            const ScratchCfg& have = d.cfg[0];
            if (have.nbuckets != 0u && have.direct_ly == 0u && have.nwaves >= want && d.cfg_W == req.W && d.cfg_H == req.H) {
                // (the pool in place serves this batch: its size stays -- sizes that follow the free memory of the
                // moment would have the pool allocated and wiped again and again)
                entries = (uint64_t)have.nbuckets * (uint64_t)fx::BUCKET;
                c.usable = have.usable;
            } else if ((double)want * (double)entries * per_entry > (double)budget) {
                uint64_t fit = (uint64_t)((double)budget / ((double)want * per_entry));
                fit = std::max<uint64_t>(fit, entries / 4 * 3) & ~(uint64_t)(8 * fx::BUCKET - 1);
                if (fit < entries) {
                    entries = fit;
                    c.usable = (uint32_t)(entries / 8 * 7);
                }
            }
        }
        c.nbuckets = (uint32_t)(entries / (uint64_t)fx::BUCKET);
        c.far_cap = std::max<uint32_t>(2048u, (uint32_t)(entries / 8));
        if (const char* e = getenv("FXJPS_FAR_CAP")) c.far_cap = (uint32_t)std::min(std::max(atoi(e), 64), 1 << 24);
        c.nwaves = want_waves;
    } else {
        const uint32_t l2e = std::max(ceil_log2(cells * 2 + 64), 12u);
        c.nbuckets = (uint32_t)(((uint64_t)1 << l2e) / (uint64_t)fx::BUCKET);
        c.usable = (uint32_t)(((uint64_t)1 << l2e) / 4 * 3);
        c.far_cap = (uint32_t)std::min<uint64_t>(cells * 2 + 1024, 0x7FFFFFFFull);
        c.nwaves = want_waves;
    }
    c.far_cap = (c.far_cap + 7u) & ~7u;  // the u16 cell-info array behind the entries stays 16-byte granular
    // (one size for both open-list layouts: the slotless instantiations keep the cell info inside the entry and leave that array alone)
    const size_t per_wave = ((size_t)fx::BUCKET * c.nbuckets) * sizeof(TEnt) + (size_t)(c.far_cap + c.far_cap / 8) * sizeof(FarEnt);
    uint32_t maxw = (uint32_t)std::min<size_t>(budget / per_wave, 1u << 20);
    maxw = (uint32_t)wpb_down(maxw);
    if (maxw < (uint32_t)fx::WPB) return fail(h, FXJPS_E_NOMEM, "grid %dx%d needs %zu bytes of scratch per wavefront", req.W, req.H, per_wave);
    if ((uint32_t)wpb_up(c.nwaves) > maxw) d.run.waves_short = true;
    c.nwaves = std::max((uint32_t)fx::WPB, std::min((uint32_t)wpb_up(c.nwaves), maxw));
    ScratchCfg& cur = d.cfg[pool];
    const bool same = cur.nbuckets == c.nbuckets && cur.usable == c.usable && cur.direct_ly == c.direct_ly && cur.far_cap == c.far_cap && cur.nwaves >= c.nwaves;
    if (pool == 0) {  // (the pool in place, or the one configured below, now serves these extents)
        d.cfg_W = req.W;
        d.cfg_H = req.H;
    }
    if (same && d.pool_clean[pool]) return FXJPS_OK;
    if (!same) {
        // the old buffers die inside ensure(): forget the old configuration first, so that a failed allocation can
        // never leave a stale cfg pointing at freed (or never wiped) memory
        cur = ScratchCfg();
        d.pool_clean[pool] = false;
        for (;;) {  // on out-of-memory run with fewer resident wavefronts instead of failing the batch
            hipError_t e = d.tables[pool].ensure((size_t)c.nwaves * ((size_t)fx::BUCKET * c.nbuckets));
            if (e == hipSuccess) e = d.far[pool].ensure((size_t)c.nwaves * (c.far_cap + c.far_cap / 8));
            if (e == hipSuccess) e = d.wave_gen[pool].ensure((size_t)c.nwaves);
            if (e == hipSuccess) break;
            (void)hipGetLastError();
            d.tables[pool].release();
            d.far[pool].release();
            if (e != hipErrorOutOfMemory || c.nwaves <= (uint32_t)fx::WPB)
                return fail(h, e == hipErrorOutOfMemory ? FXJPS_E_NOMEM : FXJPS_E_HIP, "scratch pool %d: %s", pool, hipGetErrorString(e));
            c.nwaves = std::max((uint32_t)fx::WPB, (uint32_t)wpb_down(c.nwaves / 2u));
            d.run.waves_short = true;
            DBG("pool %d: out of memory, retrying with %u wavefronts", pool, c.nwaves);
        }
        cur = c;
    }
    // tables must start all-empty (key 0xFFFFFFFF); wavefronts leave them clean after each query
    HIPCHK(h, hipMemsetAsync(d.tables[pool].p, 0xFF, (size_t)cur.nwaves * ((size_t)fx::BUCKET * cur.nbuckets) * sizeof(TEnt),
                             d.stream));
    HIPCHK(h, hipMemsetAsync(d.wave_gen[pool].p, 0, (size_t)cur.nwaves * sizeof(uint32_t), d.stream));
    d.pool_clean[pool] = true;
    return FXJPS_OK;
}

// The one table of k_search instantiations: heuristic x read-set recording (fxjps_replan_frame) x table indexed by the
// cell, heuristic x table indexed by the cell with a grid per query (a slots batch), and the same with read-set recording
// (fxjps_replan_slots under fxjps_set_slot_reuse(1)).  index: the instantiation's place in DevCtx::lds_attr_done.
using SearchFn = void (*)(SearchArgs);
struct SearchKernel {
    SearchFn fn;
    int index;
};
SearchKernel search_kernel(int hchoice, bool track, bool direct, bool grid_per_query) {
    static const SearchFn table[16] = {fx::k_search<1, false, false, false>, fx::k_search<1, false, true, false>,
                                       fx::k_search<1, true, false, false>,  fx::k_search<1, true, true, false>,
                                       fx::k_search<2, false, false, false>, fx::k_search<2, false, true, false>,
                                       fx::k_search<2, true, false, false>,  fx::k_search<2, true, true, false>,
                                       fx::k_search<1, false, false, true>,  fx::k_search<1, false, true, true>,
                                       fx::k_search<2, false, false, true>,  fx::k_search<2, false, true, true>,
                                       fx::k_slot_reads_search<1, false>,    fx::k_slot_reads_search<1, true>,
                                       fx::k_slot_reads_search<2, false>,    fx::k_slot_reads_search<2, true>};
    const int h2 = hchoice == 1 ? 0 : 1,
              index = (grid_per_query ? (track ? 12 : 8) + 2 * h2 : 4 * h2 + (track ? 2 : 0)) + (direct ? 1 : 0);
    return SearchKernel{table[index], index};
}

void fill_search_args(const DevCtx& d, const BatchReq& req, int pool, SearchArgs& A, const uint32_t* d_order, uint32_t nrun) {
    const ScratchCfg& c = d.cfg[pool];
    A.G = grid_of(d);
    A.starts = d.d_starts.p;
    A.goals = d.d_goals.p;
    A.order = d_order;
    A.nrun = nrun;
    A.max_len = req.max_len;
    A.out_path = d.d_path.p;
    A.out_len = d.d_len.p;
    A.out_cost = d.d_cost.p;
    A.out_counters = d.d_counters.p;
    A.qstat = d.d_qstat.p;  // nullptr unless FXJPS_QSTAT is set
    A.qread = req.track() ? d.d_qread.p : nullptr;
    A.tables = d.tables[pool].p;
    A.far = d.far[pool].p;
    A.nbuckets = c.nbuckets;
    A.tab_usable = c.usable;
    A.direct_ly = c.direct_ly;
    // The far band of the open list in f bands that a refill takes whole (no scan, no compaction): pays where open lists
    // hold thousands of entries (4096^2: + 10 %), costs where they hold hundreds (1024^2: - 10 %, an LDS atomic and a
    // scattered store per push instead of an append at a rank).  FXJPS_BANDED=0/1: measurement / test aid.
    A.banded = req.cells >= (1ull << 22) ? 1u : 0u;
    if (const char* e = getenv("FXJPS_BANDED")) A.banded = atoi(e) != 0 ? 1u : 0u;
    if (pool != 0) A.banded = 0u;  // the large pool is the last resort: its far tier has no regions that could fill up
    A.far_cap = c.far_cap;
    A.near_max = 512;  // near band of the far tier: re-banded beyond this many entries (FXJPS_NEAR_MAX: test / measurement aid;
                       // measured on c2 / c4 shard / c3: 256 .. 512 with 10 .. 16 refill widths per band is the plateau)
    if (const char* e = getenv("FXJPS_NEAR_MAX")) A.near_max = (uint32_t)std::max(1, atoi(e));
    A.next = d.d_next.p;
    A.wave_gen = d.wave_gen[pool].p;
    A.max_pops = 64ull * (unsigned long long)req.cells + 4096ull;
    if (req.slots) {  // a slots batch: every query reads the descriptor of its slot
        A.grids = d.d_slot_desc.p;
        A.grid_ids = d.d_grid_ids.p;
    }
    if (d.st.on) {  // a plain batch that streams: each query's results go to the host as it ends
        A.host_cells = d.st.cells;
        A.host_cap = d.st.cap;
        A.host_cursor = d.d_cursor.p;
        A.host_base = d.st.base;
        A.host_len = d.st.len;
        A.host_cost = d.st.cost;
    }
}

// ---- the host tail of a batch that has a head launch (launch_search): how many queries of the head of the longest-first
// order the host takes, its threads created and waiting.  0: the device keeps everything -- a shape the host search does
// not take, the knob, a handle whose host was late three batches in a row, or anything that could not be had (memory, a
// thread): decided here, before anything is launched.
// FXJPS_HOST_TAIL=<queries> (0: off) and FXJPS_HOST_THREADS=<threads> are read per call.  A share named that way is taken
// as it stands (a measurement and test aid, as FXJPS_SOLO: a sweep must run the setting it names); the load control --
// half the share after a late batch, off after three in a row -- governs the default share.
// (profiles/host_tail.txt section 2: on config 2 the settings from 8 to 24 queries lie within 1 % of each other; 16 on 8
// threads has the best median among those whose host part was never late -- 24 on 8 threads was, in 10 of 48 steps)
constexpr uint32_t HOST_TAIL_DEFAULT = 16, HOST_TAIL_THREADS_DEFAULT = 8;
uint32_t host_tail_begin(fxjps* h, DevCtx& d, const BatchReq& req, const ScratchCfg& c) {
    uint32_t kh = HOST_TAIL_DEFAULT, T = HOST_TAIL_THREADS_DEFAULT;
    if (d.tail) d.tail->done_kh = 0;
    const char* named = getenv("FXJPS_HOST_TAIL");
    if (named) kh = (uint32_t)std::min(std::max(0, atoi(named)), (int)HOST_TAIL_MAX);
    if (const char* e = getenv("FXJPS_HOST_THREADS")) T = (uint32_t)std::min(std::max(1, atoi(e)), (int)HOST_TAIL_THREADS_MAX);
    if (kh == 0u || h->devs.size() != 1 || c.direct_ly == 0u || req.slots || req.track() || d.st.on || getenv("FXJPS_QSTAT") ||
        req.max_len > (1 << 16) || req.cells > (1ull << 20))
        return 0u;
    if (!d.tail) {
        try {
            d.tail.reset(new HostTail());
        } catch (...) {
            return 0u;
        }
    }
    HostTail& t = *d.tail;
    t.abandon();  // (nothing runs here between two batches; an error path joined already)
    if (!named) {
        kh = std::min(kh, t.kh_cap);
        if (t.late_run >= 3 || kh == 0u) return 0u;
    }
    T = std::min(T, kh);
    const bool copy = t.maps_gen != d.map_gen;
    bool ok = t.path.ensure((size_t)kh * (size_t)req.max_len) == hipSuccess && t.ids.ensure(kh) == hipSuccess && t.len.ensure(kh) == hipSuccess &&
              t.cost.ensure(kh) == hipSuccess;
    if (ok && copy) {
        t.maps_gen = ~0ull;
        ok = t.jd.ensure((size_t)d.PW * d.NS * 8) == hipSuccess && t.bm.ensure((size_t)4 * d.LINES * d.WORDS) == hipSuccess &&
             t.comp.ensure((size_t)d.W * d.H) == hipSuccess && (t.stream || t.stream.create(hipStreamNonBlocking) == hipSuccess) &&
             (t.ev_grid || t.ev_grid.create(hipEventDisableTiming) == hipSuccess) && (t.ev_maps || t.ev_maps.create(hipEventDisableTiming) == hipSuccess) &&
             hipEventRecord(t.ev_grid, d.stream) == hipSuccess;  // (the maps are complete here: the copies wait for this, not for the search)
    }
    if (!ok) {
        (void)hipGetLastError();
        return 0u;
    }
    for (uint32_t i = 0; i < kh; i++) {
        t.ids.p[i] = d.h_order[i];
        t.len.p[i] = fx::QI_WATCHDOG;  // (until a thread has the query's result)
        t.cost.p[i] = 0.0;
    }
    t.starts = req.starts + 2 * d.q0;
    t.goals = req.goals + 2 * d.q0;
    t.order = d.h_order.data();
    t.hchoice = req.hchoice;
    t.max_len = req.max_len;
    t.max_pops = 64ull * (unsigned long long)req.cells + 4096ull;  // (the kernel's bound, fill_search_args)
    t.kh = kh;  // (what the threads pull up to; they wait for host_tail_go)
    if (!t.spawn(T)) {
        t.kh = 0;  // no thread could be had: the device keeps the whole order, and finish_search has nothing to put
        return 0u;
    }
    return kh;
}

// The device launches are queued: on the first batch of a map generation the maps travel to the host on a stream of their
// own beside the search, and the threads start when they have landed.
int host_tail_go(fxjps* h, DevCtx& d) {
    HostTail& t = *d.tail;
    if (t.maps_gen != d.map_gen) {
        HIPCHK(h, hipStreamWaitEvent(t.stream, t.ev_grid, 0));
        HIPCHK(h, hipMemcpyAsync(t.jd.p, d.jd.p, (size_t)d.PW * d.NS * 8 * sizeof(uint16_t), hipMemcpyDeviceToHost, t.stream));
        HIPCHK(h, hipMemcpyAsync(t.bm.p, d.bm.p, (size_t)4 * d.LINES * d.WORDS * sizeof(fx::BmWord), hipMemcpyDeviceToHost, t.stream));
        HIPCHK(h, hipMemcpyAsync(t.comp.p, d.comp.p, (size_t)d.W * d.H * sizeof(int32_t), hipMemcpyDeviceToHost, t.stream));
        HIPCHK(h, hipEventRecord(t.ev_maps, t.stream));
        HIPCHK(h, hipEventSynchronize(t.ev_maps));
        t.maps.jd = t.jd.p;
        t.maps.bm = reinterpret_cast<const fxh::BmWord*>(t.bm.p);
        t.maps.comp = t.comp.p;
        t.maps.W = d.W;
        t.maps.H = d.H;
        t.maps.NS = d.NS;
        t.maps.LINES = d.LINES;
        t.maps.WORDS = d.WORDS;
        t.maps_gen = d.map_gen;
    }
    t.release(1);
    return FXJPS_OK;
}

// The host has seen the device search finish: whether the host part is the later one (the load control: the share halves,
// three such batches in a row switch the tail off for the handle), then its results into the batch's device buffers.
int host_tail_end(fxjps* h, DevCtx& d, const BatchReq& req) {
    HostTail& t = *d.tail;
    const uint32_t kh = t.kh;
    const bool late = t.ended.load() < (uint32_t)t.threads.size();
    t.join();
    t.kh = 0;
    // the load control: a late batch halves the share of the next one (never to nothing: three late batches IN A ROW are
    // what switches the tail off), and a host that is on time again for 16 batches in a row gets the share back step by step
    if (late) {
        t.kh_cap = std::max(1u, std::min(t.kh_cap, kh) / 2u);
        t.late_run++;
        t.ontime_run = 0;
    } else {
        t.late_run = 0;
        if (++t.ontime_run >= 16) {
            t.kh_cap = std::min(HOST_TAIL_MAX, t.kh_cap * 2u);
            t.ontime_run = 0;
        }
    }
    t.done_kh = kh;
    t.done_ms = (t.t_last - t.t_first) * 1e3;
    t.done_late = late;
    void *dp_ids = nullptr, *dp_path = nullptr, *dp_len = nullptr, *dp_cost = nullptr;
    HIPCHK(h, hipHostGetDevicePointer(&dp_ids, t.ids.p, 0));
    HIPCHK(h, hipHostGetDevicePointer(&dp_path, t.path.p, 0));
    HIPCHK(h, hipHostGetDevicePointer(&dp_len, t.len.p, 0));
    HIPCHK(h, hipHostGetDevicePointer(&dp_cost, t.cost.p, 0));
    hipLaunchKernelGGL(fx::k_host_tail_put, dim3(kh), dim3(256), 0, d.stream, (const uint32_t*)dp_ids, (const uint32_t*)dp_path, (const int32_t*)dp_len,
                       (const double*)dp_cost, req.max_len, (long long)d.nq, d.d_path.p, d.d_len.p, d.d_cost.p, d.d_counters.p,
                       (unsigned long long)t.pops.load(), (unsigned long long)t.pushes.load());
    HIPCHK(h, hipGetLastError());
    DBG("host tail: %u queries, %.3f ms%s", kh, t.done_ms, late ? " (late)" : "");
    return FXJPS_OK;
}

int launch_search(fxjps* h, DevCtx& d, const BatchReq& req, int pool, const uint32_t* d_order, uint32_t nrun) {
    const ScratchCfg& c = d.cfg[pool];
    const bool track = req.track();
    SearchArgs A;
    fill_search_args(d, req, pool, A, d_order, nrun);
    uint32_t waves = std::min<uint32_t>(c.nwaves, (nrun + 0u));
    waves = std::max<uint32_t>((uint32_t)fx::WPB, (uint32_t)wpb_up(waves));
    waves = std::min<uint32_t>(waves, c.nwaves);
    // Wavefronts per CU.  A query is a chain of dependent pops, and a wavefront that shares its CU with fifteen others runs
    // that chain more slowly than one that has the CU to itself (config 2, the long diagonal queries: 0.69 us per pop among
    // the batch, 0.62 alone on a CU, 0.59 alone on the chip).  A batch lasts as long as its slowest query; when the batch is
    // small enough for that to show (up to 32 768 queries: beyond, the rest of the batch outlasts every single query), the
    // head of the longest-first order (`nsolo` queries) goes first, in a launch of its own on a second stream: ONE live
    // wavefront per block and an LDS size that lets no second block onto the CU.  The batch's launch is queued when every
    // block of that one has reported from its CU (a counter in pinned memory the host waits on) and fills the rest of the chip.
    // Measured on config 2: 102 k -> 114 k plans/s with 8 .. 48 such queries, two live wavefronts per CU 110 k, four 107 k;
    // on a 125 000-query batch 24 of them cost 1 - 2 %.  FXJPS_SOLO / FXJPS_SOLO_LIVE: measurement and test aids.
    // FXJPS_SPREAD=n (off by default: measured on config 5, 1000 queries, no gain) spreads a batch of at most n queries
    // per CU the same way.
    uint32_t nsolo = (nrun <= 32768u && d.share * h->mem_div == 1) ? 16u : 0u, live_solo = 1, live_main = 0;
    if (const char* e = getenv("FXJPS_SOLO")) nsolo = (uint32_t)std::max(0, atoi(e));
    if (const char* e = getenv("FXJPS_SOLO_LIVE")) live_solo = (uint32_t)std::max(1, atoi(e));
    if (const char* e = getenv("FXJPS_SPREAD")) live_main = (uint32_t)std::max(0, atoi(e));
    if (live_solo != 1u && live_solo != 2u && live_solo != 4u) live_solo = 4u;
    if (live_main != 0u && live_main != 1u && live_main != 2u && live_main != 4u) live_main = 4u;
    if (pool != 0 || track || d_order == nullptr || d.solo_started == nullptr || d.solo_timeouts_run >= 3 || nrun < 4096u || nrun < 64u * nsolo ||
        waves <= 2u * nsolo + (uint32_t)fx::WPB)
        nsolo = 0;
    nsolo = std::min<uint32_t>(nsolo, 512u) & ~(live_solo - 1u);
    if (nsolo != 0u) waves = std::min<uint32_t>(waves, (uint32_t)wpb_down(c.nwaves - nsolo));
    // The host tail: where there is a head launch, the very first queries of the order go to host threads instead (a host
    // core runs such a chain of dependent pops about twice as fast as a lone wavefront: profiles/host_tail.txt), and both
    // launches take theirs from behind them.
    const uint32_t kh = nsolo != 0u ? host_tail_begin(h, d, req, c) : 0u;
    if (kh != 0u) {
        d_order += kh;
        nrun -= kh;
        A.order = d_order;
        A.nrun = nrun;
    }

    if (pool != 0 || nsolo != 0u || (uint64_t)nrun > (uint64_t)d.n_cu * live_main || d.share * h->mem_div > 1) live_main = 0u;
    if (pool == 0) d.run.waves_used = waves;
    HIPCHK(h, hipMemsetAsync(d.d_next.p, 0, 4 * sizeof(unsigned int), d.stream));
    const dim3 block(fx::WAVE * fx::WPB);
    DBG("launch k_search pool=%d waves=%u nrun=%u buckets=%u far_cap=%u solo=%u x %u spread=%u", pool, waves, nrun, c.nbuckets, c.far_cap, nsolo,
        live_solo, live_main);
    HIPCHK(h, hipEventRecord(d.ev0, d.stream));
    {
        const SearchKernel k = search_kernel(req.hchoice, track, c.direct_ly > 0, req.slots);
        const SearchFn fn = k.fn;
        static const size_t pad = 36u << 10;  // 66 .. 74 KB of the block's own + this: no second block fits the CU's 160 KB
                                              // (74 KB + 36 KB = 110 KB fit, 184 KB with a second block do not: tests/test_slotless_open_list_host.py)
        if (nsolo != 0u || live_main != 0u) {
            if (!d.lds_attr_done[k.index]) {
                if (hipFuncSetAttribute(reinterpret_cast<const void*>(fn), hipFuncAttributeMaxDynamicSharedMemorySize, (int)pad) == hipSuccess) {
                    d.lds_attr_done[k.index] = true;
                } else {  // no such launches on this device then: the batch runs as one launch (speed, not correctness)
                    (void)hipGetLastError();
                    nsolo = 0u;
                    live_main = 0u;
                }
            }
        }
        if (nsolo != 0u) {
            SearchArgs B = A;
            B.nrun = nsolo;
            B.solo = live_solo;
            B.wave_base = waves;
            B.next = d.d_next.p + 1;
            A.q0 = nsolo;
            A.nrun = nrun - nsolo;
            B.started = d.solo_started;
            HIPCHK(h, hipEventRecord(d.ev_solo0, d.stream));
            HIPCHK(h, hipStreamWaitEvent(d.stream_solo, d.ev_solo0, 0));
            HIPCHK(h, hipEventRecord(d.ev_hd0, d.stream_solo));
            hipLaunchKernelGGL(fn, dim3(nsolo / live_solo), block, pad, d.stream_solo, B);
            HIPCHK(h, hipGetLastError());
            HIPCHK(h, hipEventRecord(d.ev_hd1, d.stream_solo));
            HIPCHK(h, hipEventRecord(d.ev_solo1, d.stream_solo));
            // The batch's launch must not take the CUs first: it is queued when every block of this one has reported from
            // its CU (a counter in pinned host memory; tens of microseconds).  The host waits, not the stream: a stream
            // wait on a value only another queue's kernel can write deadlocks under tools that run one kernel at a time
            // (rocprofv3 --pmc).  After 5 ms the batch goes ahead regardless -- placement is speed, never correctness.
            d.solo_target += nsolo / live_solo;
            const auto t0 = std::chrono::steady_clock::now();
            bool late = false;
            while ((int32_t)(__atomic_load_n(d.solo_started.h, __ATOMIC_ACQUIRE) - d.solo_target) < 0) {
                if (std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(5)) {
                    // (the counter did not arrive in time -- no PCIe atomics, a tool that serialises kernels: after three
                    // such waits in a row this device runs its batches as one launch; fxjps_timing_t::solo_timeouts counts them)
                    late = true;
                    break;
                }
            }
            d.solo_timeouts += late ? 1 : 0;
            d.solo_timeouts_run = late ? d.solo_timeouts_run + 1 : 0;
        }
        if (nsolo != 0u) HIPCHK(h, hipEventRecord(d.ev_bt0, d.stream));
        if (live_main != 0u) {
            A.solo = live_main;
            hipLaunchKernelGGL(fn, dim3(waves / live_main), block, pad, d.stream, A);
        } else {
            hipLaunchKernelGGL(fn, dim3(waves / fx::WPB), block, 0, d.stream, A);
        }
        HIPCHK(h, hipGetLastError());
        if (nsolo != 0u) {
            HIPCHK(h, hipEventRecord(d.ev_bt1, d.stream));
            HIPCHK(h, hipStreamWaitEvent(d.stream, d.ev_solo1, 0));
        }
        if (pool == 0) d.run.had_solo = nsolo != 0u;
    }
    HIPCHK(h, hipEventRecord(d.ev1, d.stream));
    if (d.st.on) {  // (behind both launches: the stream waits for the head launch above)
        hipLaunchKernelGGL(fx::k_counters_out, dim3(1), dim3(64), 0, d.stream, d.d_counters.p, d.st.counters);
        HIPCHK(h, hipGetLastError());
    }
    d.run.launches += nsolo != 0u ? 2 : 1;  // (the two launches overlap: the events span both)
    if (kh != 0u) return host_tail_go(h, d);
    return FXJPS_OK;
}

// A plain batch is about to be queued: the room its results stream into.  The arena starts at nq * min(max_len, 512)
// cells and follows 1.25 x the largest total this context has produced; ARENA_BYTES per handle, divided among its
// contexts, bound it, and a batch that is expected to need more does not stream (d.st.on stays false: today's tail).
// FXJPS_ARENA_CELLS=n: the arena holds n cells for this call (test aid: n below a batch's total makes it overflow).
constexpr size_t ARENA_BYTES = (size_t)1 << 30;
int begin_streaming(fxjps* h, DevCtx& d, const BatchReq& req) {
    const int64_t nq = d.nq;
    const unsigned long long limit = ARENA_BYTES / sizeof(uint32_t) / h->devs.size();
    unsigned long long want = (unsigned long long)nq * (unsigned long long)std::min(req.max_len, 512);
    want = std::max(want, (unsigned long long)d.arena_peak + (unsigned long long)d.arena_peak / 4);
    if (const char* e = getenv("FXJPS_ARENA_CELLS")) want = (unsigned long long)std::max(0ll, atoll(e));
    if (want > limit) return FXJPS_OK;
    HIPCHK(h, d.h_arena.ensure((size_t)std::max(want, 1ull)));
    HIPCHK(h, d.h_base.ensure((size_t)nq));
    HIPCHK(h, d.d_cursor.ensure(1));
    void *dp_cells = nullptr, *dp_base = nullptr, *dp_len = nullptr, *dp_cost = nullptr, *dp_cnt = nullptr;
    HIPCHK(h, hipHostGetDevicePointer(&dp_cells, d.h_arena.p, 0));
    HIPCHK(h, hipHostGetDevicePointer(&dp_base, d.h_base.p, 0));
    HIPCHK(h, hipHostGetDevicePointer(&dp_len, d.h_len.p, 0));
    HIPCHK(h, hipHostGetDevicePointer(&dp_cost, d.h_cost.p, 0));
    HIPCHK(h, hipHostGetDevicePointer(&dp_cnt, d.h_counters.p, 0));
    HIPCHK(h, hipMemsetAsync(d.d_cursor.p, 0, sizeof(unsigned long long), d.stream));
    d.st.on = true;
    d.st.cells = (uint32_t*)dp_cells;
    d.st.cap = want;
    d.st.base = (long long*)dp_base;
    d.st.len = (int32_t*)dp_len;
    d.st.cost = (double*)dp_cost;
    d.st.counters = (unsigned long long*)dp_cnt;
    return FXJPS_OK;
}

// Runs the shard [q0, q0+nq) of the batch on device d up to the point where the search is queued.
int run_shard(fxjps* h, DevCtx& d, const BatchReq& req) {
    HIPCHK(h, hipSetDevice(d.dev));
    const int64_t nq = d.nq;
    const int max_len = req.max_len;
    d.run = DevCtx::RunStats();
    if (nq == 0) return FXJPS_OK;
    HIPCHK(h, d.d_starts.ensure((size_t)nq * 2));
    HIPCHK(h, d.d_goals.ensure((size_t)nq * 2));
    HIPCHK(h, d.d_len.ensure((size_t)nq));
    HIPCHK(h, d.d_cost.ensure((size_t)nq));
    d.cells_bound = (size_t)nq * (size_t)max_len * 2 * sizeof(int32_t);
    if (int rc = ensure_beside_pool0(h, d, d.d_path, (size_t)nq * max_len)) return rc;
    HIPCHK(h, d.d_offsets.ensure((size_t)nq + 1));
    HIPCHK(h, d.d_next.ensure(4));
    HIPCHK(h, d.d_counters.ensure(64));
    HIPCHK(h, d.h_len.ensure((size_t)nq));
    HIPCHK(h, d.h_cost.ensure((size_t)nq));
    HIPCHK(h, d.h_offsets.ensure((size_t)nq + 1));
    HIPCHK(h, d.h_counters.ensure(64));
    HIPCHK(h, hipMemcpyAsync(d.d_starts.p, req.starts + 2 * d.q0, (size_t)nq * 2 * sizeof(int32_t), hipMemcpyHostToDevice, d.stream));
    HIPCHK(h, hipMemcpyAsync(d.d_goals.p, req.goals + 2 * d.q0, (size_t)nq * 2 * sizeof(int32_t), hipMemcpyHostToDevice, d.stream));
    if (req.slots) {
        HIPCHK(h, d.d_grid_ids.ensure((size_t)nq));
        HIPCHK(h, hipMemcpyAsync(d.d_grid_ids.p, req.grid_ids + d.q0, (size_t)nq * sizeof(int32_t), hipMemcpyHostToDevice, d.stream));
    }
    HIPCHK(h, hipMemsetAsync(d.d_counters.p, 0, 64 * sizeof(unsigned long long), d.stream));
    d.st = DevCtx::Streaming();
    if (getenv("FXJPS_QSTAT")) {  // diagnostics: per-query start / end time, pops, wavefront (tools/qstat.py)
        HIPCHK(h, d.d_qstat.ensure((size_t)nq * 4));
        HIPCHK(h, hipMemsetAsync(d.d_qstat.p, 0, (size_t)nq * 4 * sizeof(unsigned long long), d.stream));
    }
    uint32_t full = (uint32_t)d.n_cu * 4u * (uint32_t)fx::OCC / (uint32_t)(d.share * h->mem_div);  // every wavefront the chip can hold at once (this handle's share of them)
    full = std::max<uint32_t>((uint32_t)wpb_down(full), (uint32_t)fx::WPB);
    if (const char* e = getenv("FXJPS_WAVES")) full = (uint32_t)wpb_down((uint64_t)std::max(fx::WPB, atoi(e)));  // measurement aid
    // Longest-processing-time-first: the time a query takes grows with the start-goal distance, so far-apart queries are
    // handed out first and the short ones fill the tail.  The key is max(dx, dy) + min(dx, dy) / 2: on the config-2
    // workload it correlates 0.95 with the time a query takes and 0.95 with its expansions (Chebyshev distance: 0.91 /
    // 0.94; Manhattan: 0.94 / 0.92) -- the queries that end last are the long DIAGONAL ones, whose open lists are full of
    // equal keys (fewer nodes committed per iteration).  Counting sort, descending.
    {
        const int32_t* S = req.starts + 2 * d.q0;
        const int32_t* G = req.goals + 2 * d.q0;
        constexpr uint32_t KMAX = 3u * 8192u - 1u;
        std::vector<uint32_t> head(KMAX + 3u, 0);
        d.h_order.resize((size_t)nq);
        auto key = [&](int64_t i) -> uint32_t {
            const int64_t dx = std::llabs((int64_t)S[2 * i] - G[2 * i]), dy = std::llabs((int64_t)S[2 * i + 1] - G[2 * i + 1]);
            return (uint32_t)std::min<int64_t>(2 * std::max(dx, dy) + std::min(dx, dy), (int64_t)KMAX);
        };
        const bool subset = req.mode == 2;  // streaming replan: only the queries whose read set was touched
        auto in = [&](int64_t i) -> bool { return !subset || d.h_sel[(size_t)i] != 0; };
        for (int64_t i = 0; i < nq; i++)
            if (in(i)) head[KMAX - key(i) + 1]++;
        for (uint32_t k = 1; k < KMAX + 3u; k++) head[k] += head[k - 1];
        d.run.nrun = head[KMAX + 2u];
        for (int64_t i = 0; i < nq; i++)
            if (in(i)) d.h_order[head[KMAX - key(i)]++] = (uint32_t)i;
        HIPCHK(h, d.d_order.ensure((size_t)nq));
        if (d.run.nrun > 0)
            HIPCHK(h, hipMemcpyAsync(d.d_order.p, d.h_order.data(), (size_t)d.run.nrun * sizeof(uint32_t), hipMemcpyHostToDevice, d.stream));
    }
    if (req.track()) {  // read-set bitmaps: 128 x u64 per query, zero for queries that never searched
        const size_t had = d.d_qread.cap;
        HIPCHK(h, d.d_qread.ensure((size_t)nq * 128));
        if (d.d_qread.cap != had)
            HIPCHK(h, hipMemsetAsync(d.d_qread.p, 0, d.d_qread.cap * sizeof(unsigned long long), d.stream));
        else if (req.slots)  // (a sub-batch of fxjps_replan_slots: row k was another query's the call before)
            HIPCHK(h, hipMemsetAsync(d.d_qread.p, 0, (size_t)nq * 128 * sizeof(unsigned long long), d.stream));
    }
    if (d.run.nrun == 0) return FXJPS_OK;  // every result of the previous frame is still valid
    DBG("run_shard nq=%lld: inputs queued", (long long)nq);
    int rc = ensure_pool(h, d, req, 0, (uint32_t)std::min<int64_t>(full, (d.run.nrun + 3) & ~3ll));
    if (rc) return rc;
    DBG("pool ready");
    // (the search kernels with cell-indexed tables are the ones that stream: profiles/result_streaming_resource_usage.json)
    if (req.stream && d.cfg[0].direct_ly > 0)
        if ((rc = begin_streaming(h, d, req)) != FXJPS_OK) return rc;
    return launch_search(h, d, req, 0, d.d_order.p, (uint32_t)d.run.nrun);
}

// Second half, first part: wait for the search and retry overflowed queries with the large pool.  Leaves the lengths (internal
// codes included) in d.h_len.
int finish_search(fxjps* h, DevCtx& d, const BatchReq& req) {
    HIPCHK(h, hipSetDevice(d.dev));
    const int64_t nq = d.nq;
    if (nq == 0) return FXJPS_OK;
    // The result lengths are copied AFTER the host has seen the search finish, not queued behind it: a copy that waits
    // in the copy engine's queue for a kernel holds up every copy queued after it -- the input copies of another handle's
    // next batch on this device among them, and with them that batch's launch (two handles planning config-2 batches in
    // turn ran strictly one after the other: tools/copy_timeline.py).
    DBG("waiting for the search kernel");
    HIPCHK(h, hipStreamSynchronize(d.stream));
    DBG("search kernel done");
    if (d.tail && d.tail->kh != 0u)
        if (int rc = host_tail_end(h, d, req)) return rc;
    if (!d.st.on) {  // (a streamed batch: the kernel left the lengths in h_len)
        HIPCHK(h, hipMemcpyAsync(d.h_len.p, d.d_len.p, (size_t)nq * sizeof(int32_t), hipMemcpyDeviceToHost, d.stream));
        HIPCHK(h, hipStreamSynchronize(d.stream));
    }
    float ms = 0;
    if (d.run.launches > 0) {
        HIPCHK(h, hipEventElapsedTime(&ms, d.ev0, d.ev1));
        d.run.kernel_ms += ms;
        if (d.run.had_solo) {
            float a = 0, b = 0;
            HIPCHK(h, hipEventElapsedTime(&a, d.ev_hd0, d.ev_hd1));
            HIPCHK(h, hipEventElapsedTime(&b, d.ev_bt0, d.ev_bt1));
            d.run.head_ms = a;
            d.run.batch_ms = b;
        }
    }
    std::vector<uint32_t> redo;
    for (int64_t i = 0; i < nq; i++)
        if (d.h_len.p[i] <= fx::QI_TABLE_FULL) redo.push_back((uint32_t)i);
    if (!redo.empty()) {
        d.run.retried = (int64_t)redo.size();
        int rc = ensure_pool(h, d, req, 1, (uint32_t)std::min<size_t>(256, (redo.size() + 3) & ~(size_t)3));
        if (rc) return rc;
        HIPCHK(h, d.d_redo.ensure(redo.size()));
        HIPCHK(h, hipMemcpyAsync(d.d_redo.p, redo.data(), redo.size() * sizeof(uint32_t), hipMemcpyHostToDevice, d.stream));
        HIPCHK(h, hipStreamSynchronize(d.stream));  // `redo` is pageable host memory
        if (d.cfg[1].direct_ly == 0) d.st = DevCtx::Streaming();  // (the large pool's tables are hashed: its kernel leaves the retried
                                                                  // queries' results on the device only, and the batch is packed there)
        rc = launch_search(h, d, req, 1, d.d_redo.p, (uint32_t)redo.size());
        if (rc) return rc;
        HIPCHK(h, hipStreamSynchronize(d.stream));  // (as above: no copy waits in the engine's queue for a search)
        if (!d.st.on) {
            HIPCHK(h, hipMemcpyAsync(d.h_len.p, d.d_len.p, (size_t)nq * sizeof(int32_t), hipMemcpyDeviceToHost, d.stream));
            HIPCHK(h, hipStreamSynchronize(d.stream));
        }
        HIPCHK(h, hipEventElapsedTime(&ms, d.ev0, d.ev1));
        d.run.kernel_ms += ms;
    }
    DBG("kernel %.3f ms, %zu to redo", d.run.kernel_ms, redo.size());
    return FXJPS_OK;
}

// Internal codes must not leak: whatever the large pool could not finish either is FXJPS_Q_CAPACITY to the caller.
void hide_internal_codes(DevCtx& d) {
    for (int64_t i = 0; i < d.nq; i++)
        if (d.h_len.p[i] <= fx::QI_TABLE_FULL) d.h_len.p[i] = FXJPS_Q_CAPACITY;
}

// The search is over and its lengths are on the host: pack to CSR on the device, copy offsets / costs / counters / cells back.
int pack_shard(fxjps* h, DevCtx& d, const BatchReq& req) {
    const int64_t nq = d.nq;
    hipLaunchKernelGGL(fx::k_scan_len, dim3(1), dim3(1024), 0, d.stream, d.d_len.p, (long long)nq, d.d_offsets.p);
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipMemcpyAsync(d.h_offsets.p, d.d_offsets.p, ((size_t)nq + 1) * sizeof(long long), hipMemcpyDeviceToHost, d.stream));
    HIPCHK(h, hipMemcpyAsync(d.h_cost.p, d.d_cost.p, (size_t)nq * sizeof(double), hipMemcpyDeviceToHost, d.stream));
    HIPCHK(h, hipMemcpyAsync(d.h_counters.p, d.d_counters.p, 64 * sizeof(unsigned long long), hipMemcpyDeviceToHost, d.stream));
    if (req.track() && d.run.launches > 0) {  // the read sets of what ran (the rest of the buffer is unchanged)
        d.h_qread.resize((size_t)nq * 128);
        HIPCHK(h, hipMemcpyAsync(d.h_qread.data(), d.d_qread.p, (size_t)nq * 128 * sizeof(unsigned long long), hipMemcpyDeviceToHost, d.stream));
    }
    HIPCHK(h, hipStreamSynchronize(d.stream));
    const long long total = d.h_offsets.p[nq];
    DBG("scan done, %lld cells", total);
    if (total > 0) {
        if (int rc = ensure_beside_pool0(h, d, d.d_cells, (size_t)total * 2)) return rc;  // (the search is over: its scratch can go)
        HIPCHK(h, d.h_cells.ensure((size_t)total * 2));
        hipLaunchKernelGGL(fx::k_gather_paths, dim3((unsigned)((nq + 3) / 4)), dim3(256), 0, d.stream, d.d_path.p,
                           d.d_len.p, d.d_offsets.p, (long long)nq, req.max_len, d.d_cells.p, total);
        HIPCHK(h, hipGetLastError());
        HIPCHK(h, hipMemcpyAsync(d.h_cells.p, d.d_cells.p, (size_t)total * 2 * sizeof(int32_t), hipMemcpyDeviceToHost, d.stream));
        HIPCHK(h, hipStreamSynchronize(d.stream));
    }
    DBG("gather done");
    d.cells_on_host = d.csr_on_device = true;
    return FXJPS_OK;
}

// Second half: wait for the search, retry overflowed queries with the large pool, and leave lengths, costs, offsets and
// counters in pinned host memory.  A batch that streamed has them there already, with its cells in the arena: the offsets
// are a host prefix sum, and h_cells and the device CSR wait for a reader (host_cells / device_csr).  Any other batch, and
// a streamed one whose arena overflowed, packs on the device and copies back (pack_shard).
int finish_shard(fxjps* h, DevCtx& d, const BatchReq& req) {
    const int64_t nq = d.nq;
    if (nq == 0) return FXJPS_OK;
    if (int rc = finish_search(h, d, req)) return rc;
    d.last_max_len = req.max_len;
    bool packed = !d.st.on;
    if (d.st.on) {
        const fx::StreamedResults R{d.h_len.p, d.h_base.p, d.h_arena.p, nq};
        const long long total = fx::result_offsets(d.h_len.p, nq, d.h_offsets.p);
        d.arena_peak = std::max(d.arena_peak, total);
        packed = fx::result_overflows(R, 0, nq) != 0;  // (the next batch's arena is sized from the total just recorded)
        d.cells_on_host = d.csr_on_device = false;
        DBG("streamed %lld cells into an arena of %llu%s", total, d.st.cap, packed ? ": overflow" : "");
    }
    if (packed)
        if (int rc = pack_shard(h, d, req)) return rc;
    hide_internal_codes(d);
    return FXJPS_OK;
}

// A streamed batch's cells out of the arena into dst (int32 pairs, query order), by query ranges over host threads.
void expand_arena(const DevCtx& d, int32_t* dst) {
    const fx::StreamedResults R{d.h_len.p, d.h_base.p, d.h_arena.p, d.nq};
    fx::result_expand_split(R, d.h_offsets.p, dst, fx::result_threads(d.h_offsets.p[d.nq]), [](size_t n, auto&& job) {
        (void)run_side_by_side(n, [&](size_t i) {
            job(i);
            return 0;
        });
    });
}

// The last batch's cells in h_cells (int32 pairs, query order): a streamed batch's are expanded out of the arena the first
// time a reader asks.
int host_cells(fxjps* h, DevCtx& d) {
    if (d.cells_on_host || d.nq == 0) return FXJPS_OK;
    const long long total = d.h_offsets.p[d.nq];
    HIPCHK(h, hipSetDevice(d.dev));
    HIPCHK(h, d.h_cells.ensure((size_t)std::max(total, 1ll) * 2));
    expand_arena(d, d.h_cells.p);
    d.cells_on_host = true;
    return FXJPS_OK;
}

// ... and on the device (d_offsets / d_cells, for the resident forms of the waypoint calls): packed out of the path slots,
// which hold the batch until the next one begins, the first time a reader asks.  (Lazy, not queued behind the search: a
// batch whose paths nobody reads on the device pays nothing for them.)
int device_csr(fxjps* h, DevCtx& d) {
    if (d.csr_on_device || d.nq == 0) return FXJPS_OK;
    const int64_t nq = d.nq;
    const long long total = d.h_offsets.p[nq];
    HIPCHK(h, hipSetDevice(d.dev));
    hipLaunchKernelGGL(fx::k_scan_len, dim3(1), dim3(1024), 0, d.stream, d.d_len.p, (long long)nq, d.d_offsets.p);
    HIPCHK(h, hipGetLastError());
    if (total > 0) {
        if (int rc = ensure_beside_pool0(h, d, d.d_cells, (size_t)total * 2)) return rc;
        hipLaunchKernelGGL(fx::k_gather_paths, dim3((unsigned)((nq + 3) / 4)), dim3(256), 0, d.stream, d.d_path.p,
                           d.d_len.p, d.d_offsets.p, (long long)nq, d.last_max_len, d.d_cells.p, total);
        HIPCHK(h, hipGetLastError());
    }
    HIPCHK(h, hipStreamSynchronize(d.stream));
    d.csr_on_device = true;
    return FXJPS_OK;
}

// One query per call -- the node's real use of the drop-in (global_planner_st.py:285: jps1.method once per tick, on maps
// of ~150 x 110 cells).  The batch machinery around the search (uploads of the query arrays and of the longest-first
// order, the work counter, the length scan and the CSR gather with their three host waits) costs more than such a search:
// here the start and the goal travel in the kernel arguments, ONE wavefront runs the query, and the kernel writes the
// path, its length and its cost straight into the handle's pinned host buffers -- one launch, one host wait.  Results
// land where plan_core's other path leaves them (h_len / h_cost / h_offsets / h_cells), so the callers above see no
// difference.  Returns 1 when the query has to go through the batch path after all (it outgrew the regular scratch).
int plan_single(fxjps* h, DevCtx& d, const BatchReq& req) {
    HIPCHK(h, hipSetDevice(d.dev));
    const int max_len = req.max_len;
    d.q0 = 0;
    d.nq = 1;
    d.run = DevCtx::RunStats();
    d.run.nrun = d.run.waves_used = 1;
    d.st = DevCtx::Streaming();
    d.cells_on_host = d.csr_on_device = true;  // (a single call's CSR is on the host only: LastBatch::on_host)
    HIPCHK(h, d.h_len.ensure(1));
    HIPCHK(h, d.h_cost.ensure(1));
    HIPCHK(h, d.h_offsets.ensure(2));
    HIPCHK(h, d.h_counters.ensure(64));
    HIPCHK(h, d.d_counters.ensure(64));
    HIPCHK(h, d.h_path1.ensure((size_t)max_len));
    HIPCHK(h, d.h_cells.ensure((size_t)max_len * 2));
    d.cells_bound = 0;
    int rc = ensure_pool(h, d, req, 0, (uint32_t)fx::WPB);
    if (rc) return rc;
    const ScratchCfg& c = d.cfg[0];
    SearchArgs A;
    fill_search_args(d, req, 0, A, nullptr, 1u);
    A.starts = nullptr;
    A.goals = nullptr;
    A.next = nullptr;
    A.qstat = nullptr;
    A.single = 1u;
    A.solo = 1u;
    A.imm[0] = req.starts[0];
    A.imm[1] = req.starts[1];
    A.imm[2] = req.goals[0];
    A.imm[3] = req.goals[1];
    void *dp_path = nullptr, *dp_len = nullptr, *dp_cost = nullptr;
    HIPCHK(h, hipHostGetDevicePointer(&dp_path, d.h_path1.p, 0));
    HIPCHK(h, hipHostGetDevicePointer(&dp_len, d.h_len.p, 0));
    HIPCHK(h, hipHostGetDevicePointer(&dp_cost, d.h_cost.p, 0));
    A.out_path = (uint32_t*)dp_path;
    A.out_len = (int32_t*)dp_len;
    A.out_cost = (double*)dp_cost;
    d.h_len.p[0] = fx::QI_WATCHDOG;  // (overwritten by the kernel)
    // (round 6: the kernel zeroes its 64 counters itself and leaves them in the pinned host buffer when it is done -- a memset
    // and a copy back were two more operations for the runtime to queue, ~ 12 us of a call)
    void* dp_cnt = nullptr;
    HIPCHK(h, hipHostGetDevicePointer(&dp_cnt, d.h_counters.p, 0));
    A.host_counters = (unsigned long long*)dp_cnt;
    hipLaunchKernelGGL(search_kernel(req.hchoice, false, c.direct_ly > 0, false).fn, dim3(1), dim3(fx::WAVE * fx::WPB), 0, d.stream, A);
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipStreamSynchronize(d.stream));
    // (the kernel's time by the device's constant-rate clock, read by the one wavefront at its first and last instruction: two
    // event records and hipEventElapsedTime were three more runtime calls on a 250 us call)
    d.run.kernel_ms = (double)(d.h_counters.p[63] - d.h_counters.p[62]) / (double)d.wall_khz;
    DBG("single call: kernel %.1f us, %llu pops, shader clock %.0f MHz", d.run.kernel_ms * 1e3, (unsigned long long)d.h_counters.p[0],
        d.run.kernel_ms > 0 ? (double)(d.h_counters.p[61] - d.h_counters.p[60]) / (d.run.kernel_ms * 1e3) : 0.0);
    d.h_counters.p[60] = d.h_counters.p[61] = d.h_counters.p[62] = d.h_counters.p[63] = 0ull;
    d.run.launches = 1;
    const int32_t n = d.h_len.p[0];
    if (n <= fx::QI_TABLE_FULL) return 1;  // outgrew the regular scratch (or the watchdog): the batch path has the large pool
    d.h_offsets.p[0] = 0;
    d.h_offsets.p[1] = n > 0 ? n : 0;
    for (int32_t i = 0; i < n; i++) {
        const uint32_t v = d.h_path1.p[i];
        d.h_cells.p[2 * i] = (int32_t)(v >> 16);
        d.h_cells.p[2 * i + 1] = (int32_t)(v & 0xFFFFu);
    }
    return FXJPS_OK;
}

int update_cells_async(fxjps* h, const int32_t* xy, const uint8_t* val, int64_t n, bool derive);  // (below, with the streaming entry points)
void drain_all(fxjps* h);
void collect_timing(fxjps* h);

bool slot_in_use(fxjps* h, int32_t slot) {
    const DevCtx& d0 = h->devs[0];
    return slot >= 0 && slot < FXJPS_MAX_GRID_SLOTS && (size_t)slot < d0.slots.size() && d0.slots[(size_t)slot].W > 0;
}

// What every call that takes queries refuses about them (fxjps_set_queries stores them for later frames).
int check_queries(fxjps* h, const int32_t* starts, const int32_t* goals, int64_t nq, int hchoice, int max_len) {
    if (nq < 0 || (nq > 0 && (!starts || !goals))) return fail(h, FXJPS_E_ARG, "bad query arrays");
    if (hchoice != 1 && hchoice != 2)
        return fail(h, FXJPS_E_ARG, "hchoice must be 1 or 2 (the reference raises TypeError, jps1.py:188)");
    if (max_len < 1 || max_len > (1 << 20)) return fail(h, FXJPS_E_ARG, "max_path_len out of range");
    return FXJPS_OK;
}

// A planning call's request, built and checked: every refusal of a batch is made here, and nothing of the handle is
// touched.  grid_ids == nullptr: a batch on the resident grid (no grid is judged before the arrays); otherwise a slots
// batch (slots == true; its ids are judged before the arrays, every one of them: the batch is sized by the largest
// extents among the slots it names).  *req is complete when FXJPS_OK comes back.
int batch_request(fxjps* h, bool slots, const int32_t* grid_ids, const int32_t* starts, const int32_t* goals, int64_t nq, int hchoice,
                  int max_len, int mode, BatchReq* req) {
    BatchReq r;
    r.W = r.H = 1;
    r.cells = 1;
    if (slots) {
        if (nq > 0 && !grid_ids) return fail(h, FXJPS_E_ARG, "NULL grid_ids");
        std::vector<uint8_t> seen(FXJPS_MAX_GRID_SLOTS, 0);
        for (int64_t q = 0; q < nq; q++) {
            const int32_t id = grid_ids[q];
            if (!slot_in_use(h, id))
                return fail(h, FXJPS_E_ARG, "query %lld names grid slot %d, which is %s", (long long)q, (int)id,
                            id < 0 || id >= FXJPS_MAX_GRID_SLOTS ? "out of range" : "empty");
            if (seen[(size_t)id]) continue;
            seen[(size_t)id] = 1;
            const GridBufs& g = h->devs[0].slots[(size_t)id];
            r.W = std::max(r.W, g.W);
            r.H = std::max(r.H, g.H);
            r.cells = std::max(r.cells, (uint64_t)g.W * (uint64_t)g.H);
        }
    } else {
        if (!h->have_grid) return fail(h, FXJPS_E_NOGRID, "fxjps_plan_batch before fxjps_set_grid");
        r.W = h->devs[0].W;  // (every context holds the same grid)
        r.H = h->devs[0].H;
        r.cells = (uint64_t)r.W * r.H;
    }
    if (int rc = check_queries(h, starts, goals, nq, hchoice, max_len)) return rc;
    if (nq > 0x7FFFFFF0ll) return fail(h, FXJPS_E_ARG, "too many queries in one batch");
    r.starts = starts;
    r.goals = goals;
    r.nq = nq;
    r.hchoice = hchoice;
    r.max_len = max_len;
    r.mode = mode;
    r.slots = slots;
    r.grid_ids = grid_ids;
    *req = r;
    return FXJPS_OK;
}

// A batch begins.  Until it is complete (emit_csr) no earlier batch is "the last batch": the resident-path forms of the
// waypoint entry points refuse with FXJPS_E_ARG instead of reading lengths and offsets of different batches; and the
// results stored for reuse no longer describe the device buffers (fxjps_replan_frame / fxjps_replan_slots say so again
// once theirs are complete).
int begin_batch(fxjps* h, const BatchReq& req) {
    h->last.nq = 0;
    h->last.slots = req.slots;
    if (!req.slots) {
        h->last.W = req.W;
        h->last.H = req.H;
    }
    if (h->maps_stale && !req.slots) {  // deferred cell updates: the maps are rebuilt once, in front of the search
        int rc = update_cells_async(h, nullptr, nullptr, 0, true);
        if (rc) return rc;
    }
    h->q_results_valid = h->rs_valid = false;
    h->last.on_host = false;
    return FXJPS_OK;
}

// A call's tail: how long it took, into the timing record and to the caller.
int end_call(fxjps* h, double t0, double* out_seconds_total, int rc) {
    h->timing.total_ms = (now_s() - t0) * 1e3;
    if (out_seconds_total) *out_seconds_total = now_s() - t0;
    return rc;
}

int plan_core(fxjps* h, const BatchReq& request) {
    BatchReq req = request;
    // FXJPS_STREAM_RESULTS=1, read per call: a plain batch streams its results to the host (begin_streaming).  Off by
    // default (and with =0): the results are packed on the device and copied back when the search is over.  Measured
    // (profiles/result_streaming.txt): the stores to host memory slow the search down by what the
    // shorter tail saves on config 2 (+ 0.8 ms of kernel time for - 0.85 ms behind it) and by more on 125 000 queries.
    req.stream = req.mode == 0 && getenv("FXJPS_STREAM_RESULTS") && atoi(getenv("FXJPS_STREAM_RESULTS")) != 0;
    if (int rc = begin_batch(h, req)) return rc;
    const int64_t nq = req.nq;
    const int nd = (int)h->devs.size();
    for (int r = 0; r < nd; r++) {  // contiguous shards: SURVEY 8(e)
        h->devs[r].q0 = nq * r / nd;
        h->devs[r].nq = nq * (r + 1) / nd - h->devs[r].q0;
    }
    int rc = FXJPS_OK;
    static const bool single_ok = !(getenv("FXJPS_SINGLE") && atoi(getenv("FXJPS_SINGLE")) == 0) && !getenv("FXJPS_QSTAT");  // (0: test / measurement aid)
    bool done = false;
    if (nq == 1 && nd == 1 && req.mode == 0 && single_ok && !req.slots) {  // (a lone query on a slot takes the batch path)
        rc = plan_single(h, h->devs[0], req);
        if (rc == 1) {
            rc = FXJPS_OK;  // (rare: on to the batch path)
        } else {
            done = true;
            h->last.on_host = rc == FXJPS_OK;
        }
    }
    if (nd > 1 && !rc && !done) {
        // One host thread per context: each queues its shard's copies and launches, waits for its own search (the head
        // launch's start counter, then the kernel), packs its paths and brings them back.  The devices never wait for each
        // other's host-side tail -- run one after the other, eight tails of ~ 23 ms each behind ~ 570 ms of parallel search
        // capped config 4 at 75 % strong-scaling efficiency by construction.  (The shards share nothing, jps1.py:183-192.)
        rc = run_side_by_side((size_t)nd, [&](size_t r) {
            int e = run_shard(h, h->devs[r], req);
            if (!e) e = finish_shard(h, h->devs[r], req);
            return e;
        });
        done = true;
    }
    for (int r = 0; r < nd && !rc && !done; r++) rc = run_shard(h, h->devs[r], req);
    for (int r = 0; r < nd && !rc && !done; r++) rc = finish_shard(h, h->devs[r], req);
    if (rc) {
        drain_all(h);  // before the error leaves the library
        for (auto& d : h->devs) d.nq = 0;  // (no shard holds a result)
        return rc;
    }
    collect_timing(h);
    return FXJPS_OK;
}

// a batch on the resident grid: its request, then the batch
int plan_resident(fxjps* h, const int32_t* starts, const int32_t* goals, int64_t nq, int hchoice, int max_len, int mode = 0) {
    BatchReq req;
    if (int rc = batch_request(h, false, nullptr, starts, goals, nq, hchoice, max_len, mode, &req)) return rc;
    return plan_core(h, req);
}

// the handle's timing record out of what every context's last batch left
void collect_timing(fxjps* h) {
    fxjps_timing_t& T = h->timing;
    T.search_kernel_ms = 0;
    T.search_launches = 0;
    T.retried = 0;
    T.pops = 0;
    T.pushes = 0;
    T.far_refills = 0;
    T.slow_pops = 0;
    T.table_wipes = 0;
    T.reused = 0;
    T.table_direct = 0;
    T.waves = 0;
    T.waves_short = 0;
    T.head_launch_ms = 0;
    T.batch_launch_ms = 0;
    T.solo_timeouts = 0;
    T.host_tail_queries = 0;
    T.host_tail_ms = 0;
    T.host_tail_late = 0;
    for (auto& d : h->devs) {
        if (d.tail && d.tail->done_kh != 0u && d.nq > 0 && d.run.had_solo) {
            T.host_tail_queries += d.tail->done_kh;
            T.host_tail_ms = std::max(T.host_tail_ms, d.tail->done_ms);
            if (d.tail->done_late) T.host_tail_late = 1;
        }
        T.head_launch_ms = std::max(T.head_launch_ms, d.run.head_ms);
        T.batch_launch_ms = std::max(T.batch_launch_ms, d.run.batch_ms);
        T.solo_timeouts += d.solo_timeouts;
        T.waves += d.run.waves_used;
        if (d.run.waves_short) T.waves_short = 1;
        T.search_kernel_ms = std::max(T.search_kernel_ms, d.run.kernel_ms);
        T.search_launches += d.run.launches;
        T.retried += d.run.retried;
        if (d.nq > 0) {
            T.pops += (int64_t)d.h_counters.p[0];
            T.pushes += (int64_t)d.h_counters.p[1];
            T.far_refills += (int64_t)d.h_counters.p[2];
            T.slow_pops += (int64_t)d.h_counters.p[3];
            T.table_wipes += (int64_t)d.h_counters.p[7];
            if (d.cfg[0].direct_ly > 0) T.table_direct = 1;
        }
    }
}

typedef int (*nccl_init_all_t)(void**, int, const int*);
typedef int (*nccl_bcast_t)(const void*, void*, size_t, int, int, void*, hipStream_t);
typedef int (*nccl_group_t)(void);
typedef int (*nccl_destroy_t)(void*);

typedef struct {
    char b[128];
} nccl_uid_t;  // ncclUniqueId: NCCL_UNIQUE_ID_BYTES = 128
typedef int (*nccl_get_uid_t)(nccl_uid_t*);
typedef int (*nccl_init_rank_t)(void**, int, nccl_uid_t, int);

void* load_rccl(fxjps* h) {
    void* lib = dlopen("librccl.so", RTLD_NOW | RTLD_GLOBAL);
    if (!lib) lib = dlopen("librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
    if (!lib) fail(h, FXJPS_E_COMM, "cannot load librccl.so: %s", dlerror());
    return lib;
}

int broadcast_grid(fxjps* h, int W, int H) {
    const int nd = (int)h->devs.size();
    if (h->world > 0) {
        // one process per GPU: this rank's part of the one collective of the path -- ncclBroadcast of the W*H occupancy
        // bytes from rank 0 over xGMI, on this rank's stream (every rank calls fxjps_set_grid_rank with the same W, H)
        if (h->world == 1 && !h->rccl) return FXJPS_OK;
        auto bcast = (nccl_bcast_t)dlsym(h->rccl, "ncclBroadcast");
        if (!bcast) return fail(h, FXJPS_E_COMM, "ncclBroadcast not found");
        DevCtx& d = h->devs[0];
        HIPCHK(h, hipSetDevice(d.dev));
        if (bcast(d.occ.p, d.occ.p, (size_t)W * H, /*ncclUint8*/ 1, 0, h->comms[0], d.stream) != 0)
            return fail(h, FXJPS_E_COMM, "ncclBroadcast failed on rank %d", h->rank);
        return FXJPS_OK;
    }
    // (FXJPS_FORCE_RCCL=1: test aid -- a one-device handle goes through the collective too: a communicator of one rank,
    // an in-place broadcast from itself.  Exercises the loading of librccl, the symbols, their signatures and the
    // communicator's life cycle on a one-GPU box.)
    if (nd == 1 && !(getenv("FXJPS_FORCE_RCCL") && atoi(getenv("FXJPS_FORCE_RCCL")) != 0)) return FXJPS_OK;
    bool distinct = true;
    for (int a = 0; a < nd; a++)
        for (int b = a + 1; b < nd; b++)
            if (h->devs[a].dev == h->devs[b].dev) distinct = false;
    if (!distinct) {
        // several contexts share a device (more shards than GPUs): RCCL wants one rank per device, so the grid is
        // handed over by plain copies -- on-device for a context of the root's device, peer-to-peer otherwise
        DevCtx& d0 = h->devs[0];
        for (int r = 1; r < nd; r++) {
            DevCtx& d = h->devs[r];
            if (d.dev == d0.dev) {
                HIPCHK(h, hipSetDevice(d.dev));
                HIPCHK(h, hipMemcpyAsync(d.occ.p, d0.occ.p, (size_t)W * H, hipMemcpyDeviceToDevice, d.stream));
            } else {
                HIPCHK(h, hipMemcpyPeerAsync(d.occ.p, d.dev, d0.occ.p, d0.dev, (size_t)W * H, d.stream));
            }
        }
        return FXJPS_OK;
    }
    if (!h->rccl) {
        h->rccl = dlopen("librccl.so", RTLD_NOW | RTLD_GLOBAL);
        if (!h->rccl) h->rccl = dlopen("librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
        if (!h->rccl) return fail(h, FXJPS_E_COMM, "cannot load librccl.so: %s", dlerror());
        auto init_all = (nccl_init_all_t)dlsym(h->rccl, "ncclCommInitAll");
        if (!init_all) return fail(h, FXJPS_E_COMM, "ncclCommInitAll not found");
        std::vector<int> ids;
        for (auto& d : h->devs) ids.push_back(d.dev);
        h->comms.assign(nd, nullptr);
        if (init_all(h->comms.data(), nd, ids.data()) != 0) return fail(h, FXJPS_E_COMM, "ncclCommInitAll failed");
    }
    auto bcast = (nccl_bcast_t)dlsym(h->rccl, "ncclBroadcast");
    auto gstart = (nccl_group_t)dlsym(h->rccl, "ncclGroupStart");
    auto gend = (nccl_group_t)dlsym(h->rccl, "ncclGroupEnd");
    if (!bcast || !gstart || !gend) return fail(h, FXJPS_E_COMM, "RCCL symbols missing");
    // one broadcast of W*H bytes, root = first device, over xGMI; no other collective exists on this path
    gstart();
    for (int r = 0; r < nd; r++) {
        DevCtx& d = h->devs[r];
        (void)hipSetDevice(d.dev);
        if (bcast(d.occ.p, d.occ.p, (size_t)W * H, /*ncclUint8*/ 1, 0, h->comms[r], d.stream) != 0) {
            gend();
            return fail(h, FXJPS_E_COMM, "ncclBroadcast failed on device %d", d.dev);
        }
    }
    if (gend() != 0) return fail(h, FXJPS_E_COMM, "ncclGroupEnd failed");
    return FXJPS_OK;
}

// A handle that fxjps_create_rank made with world > 1 sets its grid with fxjps_set_grid_rank and nothing else: that call
// is a collective (every rank enters ncclBroadcast), so any other whole-grid setter on such a handle would have this rank
// wait in a broadcast its peers never join.
int refuse_on_rank_handle(fxjps* h, const char* what) {
    if (h->world > 1) return fail(h, FXJPS_E_ARG, "%s on rank %d of %d: a rank handle sets its grid with fxjps_set_grid_rank (collective)", what, h->rank, h->world);
    return FXJPS_OK;
}

int finish_set_grid(fxjps* h, int W, int H, bool wait = true) {
    int rc = broadcast_grid(h, W, H);
    if (rc) return rc;
    for (auto& d : h->devs) {
        rc = derive_maps(h, d);
        if (rc) return rc;
    }
    for (auto& d : h->devs) {
        if (!wait) break;  // (one context, a small grid out of a staging buffer: whatever is queued next runs behind the build)
        HIPCHK(h, hipSetDevice(d.dev));
        HIPCHK(h, hipStreamSynchronize(d.stream));
    }
    h->have_grid = true;
    h->maps_stale = false;  // (derived from the grid that was just set: a deferred update of the old grid is moot)
    return FXJPS_OK;
}

// every stream of the handle idle (error paths: copies and kernels of the other devices may still be in flight on the
// caller's buffers and on device buffers the next call may reallocate)
void drain_all(fxjps* h) {
    const std::string keep = h->err;
    for (auto& d : h->devs) {
        if (d.tail) d.tail->abandon();  // (host threads of a batch that failed half-way)
        if (hipSetDevice(d.dev) == hipSuccess) {
            if (d.tail && d.tail->stream) (void)hipStreamSynchronize(d.tail->stream);
            if (d.stream_solo) (void)hipStreamSynchronize(d.stream_solo);  // (a head launch may still be running)
            (void)hipStreamSynchronize(d.stream);
        }
        d.pool_clean[0] = d.pool_clean[1] = false;  // a search may have died half-way through a table
        d.owner_ready = d.chg_ready = false;        // ... or an update half-way through its marks
    }
    (void)hipGetLastError();
    h->err = keep;
}

// ---- waypoint selection over a batch: where the paths are.  The caller's CSR (context 0 takes all of them), the last
// batch's, resident shard by shard on the contexts that planned them, or a single call's, which is in the pinned host
// buffers only and is handed over like a caller's CSR.
struct WpPaths {
    struct Part {
        DevCtx* d;
        int64_t q0, n, total, kept_at;    // kept_at: where the part's cells begin among the call's (the caller's kept cells and triples)
        const long long* h_off;           // the part's offsets on the host (local: h_off[0] == 0) ...
        const int32_t* h_cells;           // ... and the cells they index
        const long long* d_off;           // the same on the device: a resident shard's, or what upload() left there (nullptr:
        const int32_t *d_cells, *d_len;   // an explicit CSR not uploaded -- the slots call stages it behind its records)
    };
    std::vector<Part> parts;
    int64_t total = 0;      // cells of all parts
    bool resident = false;  // the parts are the last batch's shards

    // nonneg(q): path q's cells are read as grid cells (the ccst rule) and may not be negative.  name_query: the slots calls'
    // refusals name the query.
    template <typename F>
    int resolve(fxjps* h, int64_t nq, const int64_t* offsets, const int32_t* cells_xy, bool name_query, F&& nonneg) {
        static_assert(sizeof(long long) == sizeof(int64_t), "offsets are handed over as they are");
        if (!cells_xy && h->last.on_host) {
            offsets = reinterpret_cast<const int64_t*>(h->devs[0].h_offsets.p);
            cells_xy = h->devs[0].h_cells.p;
        }
        resident = !cells_xy;
        if (resident) {
            for (auto& d : h->devs) {
                if (d.nq == 0) continue;
                if (int rc = host_cells(h, d)) return rc;  // (a streamed batch builds both forms here, the first time)
                if (int rc = device_csr(h, d)) return rc;
                const long long t = d.h_offsets.p[d.nq];
                parts.push_back(Part{&d, d.q0, d.nq, t, total, d.h_offsets.p, d.h_cells.p, d.d_offsets.p, d.d_cells.p, d.d_len.p});
                total += t;
            }
            return FXJPS_OK;
        }
        char pre[32] = "";
        const auto at = [&](int64_t q) -> const char* {
            if (name_query) snprintf(pre, sizeof(pre), "query %lld: ", (long long)q);
            return pre;
        };
        if (offsets[0] != 0) return fail(h, FXJPS_E_ARG, "%soffsets[0] must be 0", at(0));
        for (int64_t q = 0; q < nq; q++) {
            if (offsets[q + 1] < offsets[q]) return fail(h, FXJPS_E_ARG, "%soffsets must ascend", at(q));
            if (nonneg(q))
                for (int64_t i = 2 * offsets[q]; i < 2 * offsets[q + 1]; i++)
                    if (cells_xy[i] < 0) return fail(h, FXJPS_E_ARG, "%snegative cell", at(q));
        }
        total = offsets[nq];
        parts.push_back(Part{&h->devs[0], 0, nq, total, 0, reinterpret_cast<const long long*>(offsets), cells_xy, nullptr, nullptr, nullptr});
        return FXJPS_OK;
    }
    const Part* part_of(int64_t q) const {
        for (auto& P : parts)
            if (q >= P.q0 && q < P.q0 + P.n) return &P;
        return nullptr;
    }
    // path q on the host: its cells and their number ...
    int64_t path_of(int64_t q, const int32_t** c) const {
        const Part* P = part_of(q);
        *c = P ? P->h_cells + 2 * P->h_off[q - P->q0] : nullptr;
        return P ? P->h_off[q - P->q0 + 1] - P->h_off[q - P->q0] : 0;
    }
    // ... and where they begin among the call's
    int64_t path_at(int64_t q) const {
        const Part* P = part_of(q);
        return P ? P->kept_at + P->h_off[q - P->q0] : 0;
    }
    // an explicit CSR onto context 0 as it is (offsets | lengths | cells), for the single-grid kernels
    int upload(fxjps* h) {
        if (resident) return FXJPS_OK;
        Part& P = parts[0];
        DevCtx& d = *P.d;
        HIPCHK(h, hipSetDevice(d.dev));
        HIPCHK(h, d.wp.d_off.ensure((size_t)P.n + 1));
        HIPCHK(h, d.wp.d_len.ensure((size_t)P.n));
        HIPCHK(h, d.wp.d_cells.ensure((size_t)std::max<long long>(P.total, 1) * 2));
        std::vector<int32_t> len((size_t)P.n);
        for (int64_t q = 0; q < P.n; q++) len[(size_t)q] = (int32_t)std::min<int64_t>(P.h_off[q + 1] - P.h_off[q], 0x7FFFFFFF);
        HIPCHK(h, hipMemcpyAsync(d.wp.d_off.p, P.h_off, ((size_t)P.n + 1) * sizeof(long long), hipMemcpyHostToDevice, d.stream));
        HIPCHK(h, hipMemcpyAsync(d.wp.d_len.p, len.data(), (size_t)P.n * sizeof(int32_t), hipMemcpyHostToDevice, d.stream));
        if (P.total > 0) HIPCHK(h, hipMemcpyAsync(d.wp.d_cells.p, P.h_cells, (size_t)P.total * 2 * sizeof(int32_t), hipMemcpyHostToDevice, d.stream));
        HIPCHK(h, hipStreamSynchronize(d.stream));  // (`len` is pageable host memory)
        P.d_off = d.wp.d_off.p;
        P.d_cells = d.wp.d_cells.p;
        P.d_len = d.wp.d_len.p;
        return FXJPS_OK;
    }
};

// Queue every part's copies and launch (queue(P) -> int), run `beside` on the host while the devices work, then collect.
template <typename F, typename G>
int wp_queue_then_collect(fxjps* h, WpPaths& S, F&& queue, G&& beside) {
    int rc = FXJPS_OK;
    for (auto& P : S.parts)
        if ((rc = queue(P)) != FXJPS_OK) {  // copies of the contexts in front of the failing one are still queued on the caller's buffers
            drain_all(h);
            return rc;
        }
    beside();
    for (auto& P : S.parts)
        if (hipSetDevice(P.d->dev) != hipSuccess || hipStreamSynchronize(P.d->stream) != hipSuccess) rc = fail(h, FXJPS_E_HIP, "waypoint kernel failed");
    return rc;
}

// The st rule's table of angles (fx::WpAtab): atan2(a, b) by the HOST's libm for a in [0, am], b in [-bm, bm], on every
// context of the call -- grown to the largest range seen on each, filled once per range by `nthreads` host threads.
constexpr long long ATAB_MAX = 1ll << 27;  // entries (1 GiB): a map_start far off the grid takes the host form of the rule
bool wp_atab_fits(long long am, long long bm) { return (am + 1) * (2 * bm + 1) <= ATAB_MAX && am < (1ll << 30) && bm < (1ll << 30); }

// The range of (cell + 1 - map_start) over the st queries of a call (rule == nullptr: every query), which decides whether
// the table fits: exactly, cell by cell, for paths the host sees; resident paths lie on the grid their batch was planned
// on, a slots batch's within the largest slot it named.
void wp_st_range(const fxjps* h, const WpPaths& S, int64_t nq, const int32_t* rule, const int32_t* map_start, long long& am, long long& bm) {
    am = bm = 0;
    const long long W = h->last.slots ? h->last.slots_W : h->last.W, H = h->last.slots ? h->last.slots_H : h->last.H;
    for (int64_t q = 0; q < nq; q++) {
        if (rule && rule[q] != 0) continue;
        const long long mx = map_start[2 * q], my = map_start[2 * q + 1];
        if (S.resident) {
            am = std::max(am, std::max(std::llabs(1 - mx), std::llabs(W - mx)));
            bm = std::max(bm, std::max(std::llabs(1 - my), std::llabs(H - my)));
            continue;
        }
        const int32_t* c = nullptr;
        const int64_t n = S.path_of(q, &c);
        for (int64_t i = 0; i < n; i++) {
            am = std::max(am, std::llabs((long long)c[2 * i] + 1 - mx));
            bm = std::max(bm, std::llabs((long long)c[2 * i + 1] + 1 - my));
        }
    }
}

// -> FXJPS_OK: every context of the call holds a table that covers [0, am] x [-bm, bm]; 1: no table (a context has no memory
// for it: the caller takes the host form); else the error.  A context's atab_a / atab_b describe its table only while the
// table is there and whole.
int wp_ensure_atab(fxjps* h, WpPaths& S, long long am, long long bm, int nthreads) {
    std::vector<double> tab;
    int ta = -1, tb = -1;
    for (auto& P : S.parts) {
        DevCtx& d = *P.d;
        if (d.wp.atab_a >= (int)am && d.wp.atab_b >= (int)bm) continue;
        int wa = std::max<int>((int)am, d.wp.atab_a), wb = std::max<int>((int)bm, d.wp.atab_b);
        if ((long long)(wa + 1) * (2ll * wb + 1) > ATAB_MAX) {  // (the union of two ranges may not fit: start over with this one)
            wa = (int)am;
            wb = (int)bm;
        }
        if (ta != wa || tb != wb) {
            ta = wa;
            tb = wb;
            const size_t row = (size_t)(2 * tb + 1);
            tab.resize((size_t)(ta + 1) * row);
            int nt = std::max(1, std::min<int>(nthreads > 0 ? nthreads : (int)std::thread::hardware_concurrency(), 64));
            nt = (int)std::min<long long>(nt, std::max<long long>((long long)tab.size() >> 16, 1));
            double* T = tab.data();
            (void)run_side_by_side((size_t)nt, [&](size_t t) {
                for (long long a = (long long)(ta + 1) * (long long)t / nt; a < (long long)(ta + 1) * (long long)(t + 1) / nt; a++)
                    for (long long b = -tb; b <= tb; b++) T[(size_t)a * row + (size_t)(b + tb)] = std::atan2((double)a, (double)b);
                return 0;
            });
        }
        HIPCHK(h, hipSetDevice(d.dev));
        d.wp.atab_a = d.wp.atab_b = -1;  // (ensure frees the old table before it allocates, and the copy may fail)
        if (d.wp.d_atab.ensure(tab.size()) != hipSuccess) {
            (void)hipGetLastError();
            return 1;
        }
        HIPCHK(h, hipMemcpyAsync(d.wp.d_atab.p, tab.data(), tab.size() * sizeof(double), hipMemcpyHostToDevice, d.stream));
        HIPCHK(h, hipStreamSynchronize(d.stream));  // (`tab` is pageable and dies with this call)
        d.wp.atab_a = ta;
        d.wp.atab_b = tb;
    }
    return FXJPS_OK;
}

// Where the st queries of a call run (rule == nullptr: every query is one).  -> FXJPS_OK: on the device -- every context of
// the call holds a table of angles for them and, with `upload`, the explicit CSR; 1: on host threads (wp_st_on_host) -- the
// table would not fit or could not be had, or FXJPS_WAYPOINT_ST_HOST=1 (test / measurement aid, read per call); else the error
int wp_st_place(fxjps* h, WpPaths& S, int64_t nq, const int32_t* rule, const int32_t* map_start, int nthreads, bool upload) {
    if (getenv("FXJPS_WAYPOINT_ST_HOST") && atoi(getenv("FXJPS_WAYPOINT_ST_HOST")) != 0) return 1;
    long long am = 0, bm = 0;
    wp_st_range(h, S, nq, rule, map_start, am, bm);
    if (!wp_atab_fits(am, bm)) return 1;  // (a map_start far off the grid)
    if (upload)
        if (int rc = S.upload(h)) return rc;
    return wp_ensure_atab(h, S, am, bm, nthreads);
}

// What only fxjps_tick_outputs_slots takes and writes
struct TickIO {
    const double* home_xy;
    double* out_point;
    double* out_path_xyz;
    int64_t path_capacity;
    double* out_dir_xyz;
    int32_t* out_dir_n;
    int32_t* out_dir_back;
    int64_t dir_capacity;
};

// The st rule on host threads, by fxjps_waypoint_st: a table of angles that would not fit or could not be had, or
// FXJPS_WAYPOINT_ST_HOST=1.  For the st queries of the call (rule == nullptr: every query); per_query: reso and origin are
// arrays with one entry per query, not one value for all.  out_wp apart, an output that is nullptr is not written.
// -> the first query fxjps_waypoint_st refused, -1: none
struct WpStHost {
    const int32_t *rule, *map_start;
    const double *reso, *origin;
    bool per_query;
    const double *pos, *goal;
    const int32_t* end_occu;
    double dis_wp_tre, ang_wp_tre;
    const double* prev_wp;
    const int32_t* prev_dim;
    double* out_wp;
    int32_t* out_dim;
    double *out_goal, *out_ang_wp;
    int32_t* out_n_kept;
    const TickIO* K;
};
int64_t wp_st_on_host(const WpPaths& S, int64_t nq, int nthreads, const WpStHost& A) {
    int nt = std::max(1, std::min<int>(nthreads > 0 ? nthreads : (int)std::thread::hardware_concurrency(), 256));
    nt = (int)std::min<int64_t>(nt, std::max<int64_t>(nq / 256, 1));
    std::vector<int64_t> bad((size_t)nt, -1);
    const TickIO* K = A.K;
    (void)run_side_by_side((size_t)nt, [&](size_t t) {
        for (int64_t q = nq * (int64_t)t / nt; q < nq * (int64_t)(t + 1) / nt; q++) {
            if (A.rule && A.rule[q] != 0) continue;
            const double reso = A.reso[A.per_query ? q : 0], *origin = A.origin + (A.per_query ? 2 * q : 0);
            double* wp = A.out_wp + 3 * q;
            const int32_t* c = nullptr;
            const int64_t n = S.path_of(q, &c);
            double gl[3] = {A.goal[3 * q], A.goal[3 * q + 1], A.goal[3 * q + 2]}, ang = 0.0;
            int32_t dim = 3;
            if (n <= 0) {  // no path: wp = global_goal    global_planner_st.py:287-290
                for (int k = 0; k < 3; k++) wp[k] = gl[k];
            } else {
                const bool hp = A.prev_wp && (A.prev_dim[q] == 2 || A.prev_dim[q] == 3);
                if (fxjps_waypoint_st(c, (int32_t)std::min<int64_t>(n, 0x7FFFFFFF), A.map_start + 2 * q, reso, origin, A.pos + 3 * q, A.goal + 3 * q,
                                      A.end_occu ? A.end_occu[q] : 0, A.dis_wp_tre, A.ang_wp_tre, hp ? A.prev_wp + 3 * q : nullptr,
                                      hp ? A.prev_dim[q] : 0, wp, &dim, gl, &ang) != FXJPS_OK && bad[t] < 0)
                    bad[t] = q;
            }
            if (A.out_dim) A.out_dim[q] = dim;
            if (A.out_ang_wp) A.out_ang_wp[q] = ang;
            if (A.out_n_kept) A.out_n_kept[q] = 0;
            if (A.out_goal)
                for (int k = 0; k < 3; k++) A.out_goal[3 * q + k] = gl[k];
            if (!K) continue;
            // st:292-298, 335, 356-359 for the paths the host walked, by the functions the kernel calls
            if (K->out_point) {
                K->out_point[3 * q] = wp[0];
                K->out_point[3 * q + 1] = wp[1];
                K->out_point[3 * q + 2] = fx::tick_point_z(wp[0], wp[1], gl[0], gl[1], gl[2], K->home_xy[2 * q], K->home_xy[2 * q + 1]);
            }
            if (K->out_dir_n) K->out_dir_n[q] = 0;
            if (K->out_dir_back) K->out_dir_back[q] = 0;
            if (K->out_path_xyz && n > 0) {
                double* p3 = K->out_path_xyz + 3 * S.path_at(q);
                for (int64_t i = 0; i < n; i++) {
                    p3[3 * i] = fx::wp_world(c[2 * i] + 1, reso, origin[0]);
                    p3[3 * i + 1] = fx::wp_world(c[2 * i + 1] + 1, reso, origin[1]);
                    p3[3 * i + 2] = 0.0;
                }
            }
        }
        return 0;
    });
    for (int64_t b : bad)
        if (b >= 0) return b;
    return -1;
}

}  // namespace

extern "C" {

int fxjps_version(void) { return FXJPS_VERSION; }

int fxjps_timing_size(void) { return (int)sizeof(fxjps_timing_t); }

int fxjps_device_count(void) {
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) return FXJPS_E_NODEV;
    return n;
}

int fxjps_create(int backend, const int* device_ids, int n_dev, fxjps_t** out) {
    if (!out) return fail(nullptr, FXJPS_E_ARG, "out == NULL");
    *out = nullptr;
    if (backend != FXJPS_BACKEND_HIP)
        return fail(nullptr, FXJPS_E_ARG, "backend %d: only FXJPS_BACKEND_HIP exists (no CPU fallback)", backend);
    int navail = 0;
    if (hipGetDeviceCount(&navail) != hipSuccess || navail <= 0)
        return fail(nullptr, FXJPS_E_NODEV, "no HIP device visible: the planner needs an MI355X (no CPU fallback)");
    // (a device id may appear more than once: the handle then keeps several independent contexts -- streams, maps,
    // scratch, shards -- on that device; the grid reaches them by a device-to-device copy instead of the collective)
    if (n_dev < 1 || n_dev > 64 || (!device_ids && n_dev > navail))
        return fail(nullptr, FXJPS_E_ARG, "n_dev=%d but %d device(s) visible", n_dev, navail);
    if (device_ids)
        for (int r = 0; r < n_dev; r++)
            if (device_ids[r] < 0 || device_ids[r] >= navail)
                return fail(nullptr, FXJPS_E_ARG, "device id %d but %d device(s) visible", device_ids[r], navail);
    fxjps* h = new (std::nothrow) fxjps();
    if (!h) return fail(nullptr, FXJPS_E_NOMEM, "out of host memory");
    h->devs.resize(n_dev);
    for (int r = 0; r < n_dev; r++) {
        DevCtx& d = h->devs[r];
        d.dev = device_ids ? device_ids[r] : r;
        hipDeviceProp_t prop;
        hipError_t e = hipSetDevice(d.dev);
        if (e == hipSuccess) e = hipGetDeviceProperties(&prop, d.dev);
        if (e == hipSuccess) e = d.stream.create(hipStreamNonBlocking);
        // (FXJPS_ONE_STREAM=1: measurement aid -- no second stream, hence no head launches, on this handle: how the runtime
        // deals its hardware queues out over the streams of many handles)
        const bool one_stream = getenv("FXJPS_ONE_STREAM") && atoi(getenv("FXJPS_ONE_STREAM")) != 0;
        if (e == hipSuccess && !one_stream) e = d.stream_solo.create(hipStreamNonBlocking);
        // (fine-grained, mapped: the kernel counts with a system-scope atomic, the host polls; without it no solo launches
        // on this device)
        if (e == hipSuccess && !one_stream && d.solo_started.create(hipHostMallocCoherent | hipHostMallocMapped) != hipSuccess)
            (void)hipGetLastError();
        for (Event* ev : {&d.ev_solo0, &d.ev_solo1, &d.ev_upd, &d.ev_stage, &d.ev_ccl0, &d.ev_ccl1})
            if (e == hipSuccess) e = ev->create(hipEventDisableTiming);
        for (Event* ev : {&d.ev0, &d.ev1, &d.ev_hd0, &d.ev_hd1, &d.ev_bt0, &d.ev_bt1})
            if (e == hipSuccess) e = ev->create(hipEventDefault);
        if (e != hipSuccess) {
            int rc = fail(nullptr, FXJPS_E_HIP, "device %d: %s", d.dev, hipGetErrorString(e));
            fxjps_destroy(h);
            return rc;
        }
        {
            std::vector<uint32_t> lut(11 * 256);
            for (uint32_t pd = 0; pd < 11; pd++)
                for (uint32_t m = 0; m < 256; m++) lut[pd * 256 + m] = dirlut_entry(pd, m);
            e = hipMemcpyToSymbol(HIP_SYMBOL(fx::c_dirlut), lut.data(), lut.size() * sizeof(uint32_t));
            if (e != hipSuccess) {
                int rc = fail(nullptr, FXJPS_E_HIP, "device %d: %s", d.dev, hipGetErrorString(e));
                fxjps_destroy(h);
                return rc;
            }
        }
        d.n_cu = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
        d.mem_total = prop.totalGlobalMem;
        {
            int khz = 0;
            if (hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, d.dev) == hipSuccess && khz > 0) d.wall_khz = khz;
            (void)hipGetLastError();
        }
    }
    for (auto& a : h->devs) {
        a.share = 0;
        for (auto& b : h->devs) a.share += (a.dev == b.dev) ? 1 : 0;
    }
    *out = h;
    return FXJPS_OK;
}

int fxjps_rank_unique_id(void* out_id128) {
    if (!out_id128) return fail(nullptr, FXJPS_E_ARG, "out_id128 == NULL");
    void* lib = dlopen("librccl.so", RTLD_NOW | RTLD_GLOBAL);
    if (!lib) lib = dlopen("librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
    if (!lib) return fail(nullptr, FXJPS_E_COMM, "cannot load librccl.so: %s", dlerror());
    auto get = (nccl_get_uid_t)dlsym(lib, "ncclGetUniqueId");
    if (!get) return fail(nullptr, FXJPS_E_COMM, "ncclGetUniqueId not found");
    nccl_uid_t id;
    memset(&id, 0, sizeof(id));
    if (get(&id) != 0) return fail(nullptr, FXJPS_E_COMM, "ncclGetUniqueId failed");
    memcpy(out_id128, &id, sizeof(id));
    return FXJPS_OK;  // (the library stays loaded: the handle made next uses it)
}

int fxjps_rank_preflight(int device) {
    int navail = 0;
    if (hipGetDeviceCount(&navail) != hipSuccess || navail <= 0) return fail(nullptr, FXJPS_E_NODEV, "no HIP device visible");
    if (device < 0 || device >= navail) return fail(nullptr, FXJPS_E_ARG, "device id %d but %d device(s) visible", device, navail);
    void* probe = nullptr;
    hipError_t e = hipSetDevice(device);
    if (e == hipSuccess) e = hipMalloc(&probe, 256);
    if (e == hipSuccess) e = hipFree(probe);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        return fail(nullptr, FXJPS_E_HIP, "device %d: %s", device, hipGetErrorString(e));
    }
    void* lib = dlopen("librccl.so", RTLD_NOW | RTLD_GLOBAL);
    if (!lib) lib = dlopen("librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
    if (!lib) return fail(nullptr, FXJPS_E_COMM, "cannot load librccl.so: %s", dlerror());
    for (const char* sym : {"ncclGetUniqueId", "ncclCommInitRank", "ncclBroadcast", "ncclCommDestroy"})
        if (!dlsym(lib, sym)) return fail(nullptr, FXJPS_E_COMM, "%s not found in librccl.so", sym);
    return FXJPS_OK;  // (the library stays loaded: the handle made next uses it)
}

int fxjps_reserve_grid(fxjps_t* h, int32_t W, int32_t H) {
    if (!h) return FXJPS_E_ARG;
    if (W < 1 || H < 1 || W > 8190 || H > 8190) return fail(h, FXJPS_E_ARG, "grid must be 1..8190 cells a side");
    h->have_grid = false;  // (the buffers of the resident grid may have been replaced)
    h->q_results_valid = h->rs_valid = false;
    for (auto& d : h->devs) {
        int rc = alloc_grid(h, d, W, H);
        if (rc) return rc;
    }
    return FXJPS_OK;
}

int fxjps_create_rank(int device, int rank, int world, const void* id128, fxjps_t** out) {
    if (!out) return fail(nullptr, FXJPS_E_ARG, "out == NULL");
    *out = nullptr;
    if (world < 1 || rank < 0 || rank >= world || (world > 1 && !id128)) return fail(nullptr, FXJPS_E_ARG, "rank %d of %d", rank, world);
    const int ids[1] = {device};
    fxjps_t* h = nullptr;
    int rc = fxjps_create(FXJPS_BACKEND_HIP, ids, 1, &h);
    if (rc) return rc;
    h->rank = rank;
    h->world = world;
    if (world > 1 || (getenv("FXJPS_FORCE_RCCL") && atoi(getenv("FXJPS_FORCE_RCCL")) != 0 && id128)) {
        h->rccl = load_rccl(h);
        auto init = h->rccl ? (nccl_init_rank_t)dlsym(h->rccl, "ncclCommInitRank") : nullptr;
        if (!init) {
            g_create_error = h->rccl ? "ncclCommInitRank not found" : h->err;
            fxjps_destroy(h);
            return FXJPS_E_COMM;
        }
        nccl_uid_t id;
        memcpy(&id, id128, sizeof(id));
        h->comms.assign(1, nullptr);
        (void)hipSetDevice(device);
        if (init(&h->comms[0], world, id, rank) != 0) {
            g_create_error = "ncclCommInitRank failed";
            fxjps_destroy(h);
            return FXJPS_E_COMM;
        }
    }
    *out = h;
    return FXJPS_OK;
}

int fxjps_set_grid_rank(fxjps_t* h, const uint8_t* occ, int32_t W, int32_t H) {
    if (!h) return FXJPS_E_ARG;
    if (h->world < 1) return fail(h, FXJPS_E_ARG, "fxjps_set_grid_rank on a handle that fxjps_create_rank did not make");
    if (W < 1 || H < 1 || W > 8190 || H > 8190 || (h->rank == 0 && !occ)) return fail(h, FXJPS_E_ARG, "grid must be 1..8190 cells a side (rank 0 passes it)");
    h->have_grid = false;
    h->q_results_valid = h->rs_valid = false;
    DevCtx& d0 = h->devs[0];
    int rc = alloc_grid(h, d0, W, H);
    if (rc) return rc;
    HIPCHK(h, hipSetDevice(d0.dev));
    if (h->rank == 0) HIPCHK(h, hipMemcpyAsync(d0.occ.p, occ, (size_t)W * H, hipMemcpyHostToDevice, d0.stream));
    HIPCHK(h, hipStreamSynchronize(d0.stream));
    return finish_set_grid(h, W, H);  // the broadcast (root = rank 0), then every rank derives its maps itself
}

// (~fxjps, ~DevCtx and the owners of fxjps_owned.h do the work: there is no list of members to keep here)
void fxjps_destroy(fxjps_t* h) {
    if (!h) return;
    delete h;
}

const char* fxjps_last_error(fxjps_t* h) { return h ? h->err.c_str() : g_create_error.c_str(); }

int fxjps_set_grid(fxjps_t* h, const uint8_t* occ, int32_t W, int32_t H) {
    if (!h) return FXJPS_E_ARG;
    if (!occ || W < 1 || H < 1 || W > 8190 || H > 8190) return fail(h, FXJPS_E_ARG, "grid must be 1..8190 cells a side");
    if (int rr = refuse_on_rank_handle(h, "fxjps_set_grid")) return rr;
    h->have_grid = false;
    h->q_results_valid = h->rs_valid = false;
    for (auto& d : h->devs) {
        int rc = alloc_grid(h, d, W, H);
        if (rc) return rc;
    }
    DevCtx& d0 = h->devs[0];
    HIPCHK(h, hipSetDevice(d0.dev));
    // The node's call (jps1.method once per tick on a map of ~ 150 x 110 cells): a small grid on a one-context handle goes
    // through a pinned staging buffer of the handle, and the call returns as soon as the copy and the map build are QUEUED --
    // the search of the same tick is queued right behind them, no host wait in between (round 6: 437 -> ~ 300 us for a tick
    // whose map changed; the caller's buffer is its own again when the call returns, as the ABI promises).  An error of the
    // build itself would surface at the next call that waits.  FXJPS_SETGRID_WAIT=1: wait as before (test / measurement aid).
    const char* wait_env = getenv("FXJPS_SETGRID_WAIT");  // (read per call, as FXJPS_FUSED_BUILD: the tests take both paths in one process)
    const bool always_wait = wait_env && atoi(wait_env) != 0;
    const size_t bytes = (size_t)W * H;
    if (h->devs.size() == 1 && bytes <= ((size_t)1 << 18) && !always_wait && d0.ev_stage != nullptr) {
        if (d0.stage_pending) HIPCHK(h, hipEventSynchronize(d0.ev_stage));  // (the previous grid has left the buffer)
        d0.stage_pending = false;
        HIPCHK(h, d0.h_occ_stage.ensure(bytes));
        memcpy(d0.h_occ_stage.p, occ, bytes);
        HIPCHK(h, hipMemcpyAsync(d0.occ.p, d0.h_occ_stage.p, bytes, hipMemcpyHostToDevice, d0.stream));
        HIPCHK(h, hipEventRecord(d0.ev_stage, d0.stream));
        d0.stage_pending = true;
        return finish_set_grid(h, W, H, false);
    }
    HIPCHK(h, hipMemcpyAsync(d0.occ.p, occ, bytes, hipMemcpyHostToDevice, d0.stream));
    // (several contexts: the others copy from the first one's buffer on streams of their own.  One context: the map build
    // is queued behind the copy on the same stream, and finish_set_grid waits for both -- one host wait per call)
    if (h->devs.size() > 1) HIPCHK(h, hipStreamSynchronize(d0.stream));
    return finish_set_grid(h, W, H);
}

int fxjps_set_grid_device(fxjps_t* h, const void* d_occ, int32_t W, int32_t H) {
    if (!h) return FXJPS_E_ARG;
    if (!d_occ || W < 1 || H < 1 || W > 8190 || H > 8190) return fail(h, FXJPS_E_ARG, "grid must be 1..8190 cells a side");
    if (int rr = refuse_on_rank_handle(h, "fxjps_set_grid_device")) return rr;
    h->have_grid = false;
    h->q_results_valid = h->rs_valid = false;
    for (auto& d : h->devs) {
        int rc = alloc_grid(h, d, W, H);
        if (rc) return rc;
    }
    DevCtx& d0 = h->devs[0];
    HIPCHK(h, hipSetDevice(d0.dev));
    HIPCHK(h, hipMemcpyAsync(d0.occ.p, d_occ, (size_t)W * H, hipMemcpyDeviceToDevice, d0.stream));
    HIPCHK(h, hipStreamSynchronize(d0.stream));
    return finish_set_grid(h, W, H);
}

namespace {
// How every call over a job array opens: the handle, the number of jobs, the array, and no rank handle.
int jobs_call_check(fxjps_t* h, const void* jobs, int32_t n, const char* what) {
    if (!h) return FXJPS_E_ARG;
    if (n < 0 || n > FXJPS_MAX_GRID_SLOTS) return fail(h, FXJPS_E_ARG, "n = %d jobs: must be 0 .. %d", (int)n, FXJPS_MAX_GRID_SLOTS);
    if (n > 0 && !jobs) return fail(h, FXJPS_E_ARG, "NULL jobs");
    return refuse_on_rank_handle(h, what);
}

// What the host derives from a raw map's extents, the start and the goal before anything is queued: the padding, the
// prepared extents and the shifted start and goal.  The callers judge the result (extents over 8190, a goal outside).
struct SlotPlan {
    long long dx, dy, W1, H1, nsx, nsy, ngx, ngy;
    size_t raw_off;  // (fxjps_prepare_slots) of the job's raw map inside the staged input
};
SlotPlan prepared_geometry(long long W0, long long H0, long long ifa, int variant, const int32_t* start_xy, const int32_t* goal_xy) {
    const long long sx = start_xy[0], sy = start_xy[1], gx = goal_xy[0], gy = goal_xy[1];
    SlotPlan p{};
    // global_planner_st.py:230-235 / global_planner_ccst.py:415-420
    long long o2x = -2 * ifa, o2y = -2 * ifa;
    if (gx < 0 || sx < 0) o2x += std::min(gx, sx);
    if (gy < 0 || sy < 0) o2y += std::min(gy, sy);
    p.dx = std::llabs(o2x);
    p.dy = std::llabs(o2y);
    // :246-247 / :431-432
    p.W1 = std::max(std::max(W0, gx), sx) + p.dx + 4 * ifa;
    p.H1 = std::max(std::max(H0, gy), sy) + p.dy + 4 * ifa;
    // :266-267 (st: + map_d - 1) / :452-453 (ccst: + map_d)
    const long long sh = variant == 0 ? 1 : 0;
    p.nsx = sx + p.dx - sh;
    p.nsy = sy + p.dy - sh;
    p.ngx = gx + p.dx - sh;
    p.ngy = gy + p.dy - sh;
    return p;
}

// What a single-grid prepare call was asked for, filled once by its entry point, and the geometry prepare_check derives.
struct PrepReq {
    const uint8_t* raw;
    int32_t W0, H0, ifa, variant, layout;  // layout 1: `raw` is the int8 data[] of an OccupancyGrid message
    int32_t *start_xy, *goal_xy;           // in: the raw map's cells; out: the prepared grid's
    int32_t *out_W, *out_H, *out_map_d, *out_end_occu;  // (each may be NULL)
    SlotPlan p;
    fx::PrepGeom geom() const { return fx::PrepGeom{W0, H0, (int32_t)p.dx, (int32_t)p.dy, ifa, variant, layout, (int32_t)p.W1, (int32_t)p.H1}; }
    bool goal_inside() const { return p.ngx >= 0 && p.ngy >= 0 && p.ngx < p.W1 && p.ngy < p.H1; }
};

// prepare_grid's refusals (nothing is touched yet) and the geometry of the prepared grid
int prepare_check(fxjps_t* h, const char* what, PrepReq* q) {
    if (!q->raw || !q->start_xy || !q->goal_xy || q->W0 < 1 || q->H0 < 1 || q->ifa < 0 || q->ifa > 64 || (q->variant != 0 && q->variant != 1))
        return fail(h, FXJPS_E_ARG, "bad prepare_grid arguments");
    if (int rr = refuse_on_rank_handle(h, what)) return rr;
    q->p = prepared_geometry(q->W0, q->H0, q->ifa, q->variant, q->start_xy, q->goal_xy);
    if (q->p.W1 > 8190 || q->p.H1 > 8190) return fail(h, FXJPS_E_ARG, "prepared grid %lldx%lld exceeds 8190 cells a side", q->p.W1, q->p.H1);
    return FXJPS_OK;
}

// The goal rule (fx::goal_rule) queued on context 0's stream, behind whatever that stream holds, and its record on the way
// into h_slots_res (these calls are synchronous, as the slot calls are: the buffers are free).  A goal outside the prepared
// grid queues nothing: prepare_finish refuses it.
int goal_queue(fxjps_t* h, const PrepReq& q) {
    if (!q.goal_inside()) return FXJPS_OK;
    DevCtx& d0 = h->devs[0];
    HIPCHK(h, hipSetDevice(d0.dev));
    HIPCHK(h, d0.h_slots_res.ensure(fx::SLOT_RES));
    HIPCHK(h, d0.d_slots_res.ensure(fx::SLOT_RES));
    hipLaunchKernelGGL(fx::k_prepare_goal, dim3(1), dim3(64), 0, d0.stream, d0.occ.p, (int)q.p.W1, (int)q.p.H1, (int)q.p.ngx, (int)q.p.ngy, q.ifa,
                       q.variant, d0.d_slots_res.p);
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipMemcpyAsync(d0.h_slots_res.p, d0.d_slots_res.p, fx::SLOT_RES * sizeof(int32_t), hipMemcpyDeviceToHost, d0.stream));
    return FXJPS_OK;
}
// every context's stream idle
int wait_all(fxjps_t* h) {
    for (auto& d : h->devs) {
        HIPCHK(h, hipSetDevice(d.dev));
        HIPCHK(h, hipStreamSynchronize(d.stream));
    }
    return FXJPS_OK;
}

// The whole prepared grid written and every derived map built, on every context, and the goal rule behind context 0's
// build; ONE wait, and all streams are idle.  d0_staged: the raw map already lies in context 0's d_raw (fxjps_refresh_grid
// diffed against it).
int prepare_build(fxjps_t* h, const PrepReq& q, bool d0_staged = false) {
    const fx::PrepGeom g = q.geom();
    const size_t raw_bytes = (size_t)q.W0 * q.H0;
    h->have_grid = false;
    h->q_results_valid = h->rs_valid = false;
    for (auto& d : h->devs) {
        HIPCHK(h, hipSetDevice(d.dev));
        HIPCHK(h, d.d_raw.ensure(raw_bytes));
        int rc = alloc_grid(h, d, g.W1, g.H1);
        if (rc) return rc;
        // every device pads and dilates the raw grid itself: cheaper than broadcasting the larger result
        if (!(d0_staged && &d == &h->devs[0])) HIPCHK(h, hipMemcpyAsync(d.d_raw.p, q.raw, raw_bytes, hipMemcpyHostToDevice, d.stream));
        const long long n = (long long)g.W1 * g.H1;
        hipLaunchKernelGGL(fx::k_prepare_grid, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, d.stream, d.d_raw.p, g, d.occ.p);
        HIPCHK(h, hipGetLastError());
        rc = derive_maps(h, d);
        if (rc) return rc;
    }
    if (int rc = goal_queue(h, q)) return rc;
    if (int rc = wait_all(h)) return rc;
    h->have_grid = true;
    h->maps_stale = false;
    return FXJPS_OK;
}

// What the callers get back: the shifted start, the goal moved off an obstacle, end_occu, the extents and the padding.
// done: the goal's record is in and every stream is idle (prepare_build ran and waited; a diff that found no change
// behind no deferred update); else the goal rule is queued here, behind what the caller queued, and every context is waited
// for once.  Either way the call returns with all streams idle, and a call that fails writes nothing.
int prepare_finish(fxjps_t* h, const PrepReq& q, bool done) {
    if (!done) {
        if (int rc = goal_queue(h, q)) return rc;
        if (int rc = wait_all(h)) return rc;
    }
    if (!q.goal_inside()) return fail(h, FXJPS_E_ARG, "goal outside the prepared grid");
    const int32_t* res = h->devs[0].h_slots_res.p;
    if (res[3] != 0) return fail(h, FXJPS_E_ARG, "goal row and column are fully occupied (the reference raises here)");
    const SlotPlan& p = q.p;
    if (q.out_end_occu) *q.out_end_occu = res[2];
    q.start_xy[0] = (int32_t)p.nsx;
    q.start_xy[1] = (int32_t)p.nsy;
    q.goal_xy[0] = res[0];
    q.goal_xy[1] = res[1];
    if (q.out_W) *q.out_W = (int32_t)p.W1;
    if (q.out_H) *q.out_H = (int32_t)p.H1;
    if (q.out_map_d) {
        q.out_map_d[0] = (int32_t)p.dx;
        q.out_map_d[1] = (int32_t)p.dy;
    }
    return FXJPS_OK;
}

int prepare_grid_impl(fxjps_t* h, PrepReq q) {
    if (!h) return FXJPS_E_ARG;
    if (int rc = prepare_check(h, "fxjps_prepare_grid", &q)) return rc;
    if (int rc = prepare_build(h, q)) return rc;
    return prepare_finish(h, q, true);
}
}  // namespace

int fxjps_prepare_grid(fxjps_t* h, const uint8_t* raw, int32_t W0, int32_t H0, int32_t ifa, int32_t variant,
                       int32_t* start_xy, int32_t* goal_xy, int32_t* out_W, int32_t* out_H, int32_t* out_map_d,
                       int32_t* out_end_occu) {
    return prepare_grid_impl(h, PrepReq{raw, W0, H0, ifa, variant, 0, start_xy, goal_xy, out_W, out_H, out_map_d, out_end_occu, {}});
}

int fxjps_prepare_occupancy_msg(fxjps_t* h, const int8_t* data, int32_t width, int32_t height, int32_t ifa, int32_t variant,
                                int32_t* start_xy, int32_t* goal_xy, int32_t* out_W, int32_t* out_H, int32_t* out_map_d,
                                int32_t* out_end_occu) {
    return prepare_grid_impl(h, PrepReq{reinterpret_cast<const uint8_t*>(data), width, height, ifa, variant, 1, start_xy, goal_xy, out_W, out_H,
                                        out_map_d, out_end_occu, {}});
}

int fxjps_get_grid(fxjps_t* h, uint8_t* out, int32_t* out_W, int32_t* out_H) { return fxjps_get_grid_context(h, 0, out, out_W, out_H); }

int fxjps_get_grid_context(fxjps_t* h, int32_t ctx, uint8_t* out, int32_t* out_W, int32_t* out_H) {
    if (!h) return FXJPS_E_ARG;
    if (!h->have_grid) return fail(h, FXJPS_E_NOGRID, "no grid");
    if (ctx < 0 || ctx >= (int32_t)h->devs.size()) return fail(h, FXJPS_E_ARG, "context %d of %d", (int)ctx, (int)h->devs.size());
    DevCtx& d = h->devs[(size_t)ctx];
    if (out_W) *out_W = d.W;
    if (out_H) *out_H = d.H;
    if (out) {
        // on the context's stream: it is created non-blocking, so a null-stream copy would not order behind cell
        // updates that are still queued there (fxjps_update_cells_deferred)
        HIPCHK(h, hipSetDevice(d.dev));
        HIPCHK(h, hipMemcpyAsync(out, d.occ.p, (size_t)d.W * d.H, hipMemcpyDeviceToHost, d.stream));
        HIPCHK(h, hipStreamSynchronize(d.stream));
    }
    return FXJPS_OK;
}

// ------------------------------------------------------------------ wire / on-disk adapters
namespace {
// dst[(fb ? B-1-b : b)][(fa ? A-1-a : a)][0..ch) = map(src[a][b]) for src [A][B], dst [B][A][ch]
static int transpose_map(fxjps_t* h, DevCtx& d, const uint8_t* d_src, int A, int B, int fa, int fb, int mode, int ch, uint8_t* d_dst) {
    const dim3 grid((unsigned)((B + 31) / 32), (unsigned)((A + 31) / 32)), block(32, 8);
    hipLaunchKernelGGL(fx::k_transpose_map, grid, block, 0, d.stream, d_src, A, B, fa, fb, mode, ch, d_dst);
    HIPCHK(h, hipGetLastError());
    return FXJPS_OK;
}
}  // namespace

int fxjps_publish_map(fxjps_t* h, int8_t* out_data, int32_t* out_width, int32_t* out_height) {
    if (!h) return FXJPS_E_ARG;
    if (!h->have_grid) return fail(h, FXJPS_E_NOGRID, "no grid");
    DevCtx& d = h->devs[0];
    if (out_width) *out_width = d.W;    // info.width  = len(data)      global_planner_st.py:109
    if (out_height) *out_height = d.H;  // info.height = len(data[0])   :110
    if (!out_data) return FXJPS_OK;
    HIPCHK(h, hipSetDevice(d.dev));
    const size_t n = (size_t)d.W * d.H;
    HIPCHK(h, d.d_img.ensure(n));
    int rc = transpose_map(h, d, d.occ.p, d.W, d.H, 0, 0, fx::TM_OCC_TO_MSG, 1, d.d_img.p);  // data.T, 1 -> 100   :103,115
    if (rc) return rc;
    HIPCHK(h, hipMemcpyAsync(out_data, d.d_img.p, n, hipMemcpyDeviceToHost, d.stream));
    HIPCHK(h, hipStreamSynchronize(d.stream));
    return FXJPS_OK;
}

int fxjps_set_grid_image(fxjps_t* h, const uint8_t* gray, int32_t rows, int32_t cols) {
    if (!h) return FXJPS_E_ARG;
    if (!gray || rows < 1 || cols < 1 || rows > 8190 || cols > 8190) return fail(h, FXJPS_E_ARG, "image must be 1..8190 pixels a side");
    if (int rr = refuse_on_rank_handle(h, "fxjps_set_grid_image")) return rr;
    h->have_grid = false;
    h->q_results_valid = h->rs_valid = false;
    const size_t n = (size_t)rows * cols;
    for (auto& d : h->devs) {
        int rc = alloc_grid(h, d, cols, rows);  // map_pre = img[::-1].T: W = image columns, H = image rows   :182
        if (rc) return rc;
    }
    DevCtx& d0 = h->devs[0];
    HIPCHK(h, hipSetDevice(d0.dev));
    HIPCHK(h, d0.d_img.ensure(n));
    HIPCHK(h, hipMemcpyAsync(d0.d_img.p, gray, n, hipMemcpyHostToDevice, d0.stream));
    int rc = transpose_map(h, d0, d0.d_img.p, rows, cols, 1, 0, fx::TM_GRAY_TO_OCC, 1, d0.occ.p);  // > 200 white/free, else black/occupied   :179-180
    if (rc) return rc;
    HIPCHK(h, hipStreamSynchronize(d0.stream));
    return finish_set_grid(h, cols, rows);
}

int fxjps_snapshot_image(fxjps_t* h, uint8_t* out, int32_t channels, int32_t* out_rows, int32_t* out_cols) {
    if (!h) return FXJPS_E_ARG;
    if (!h->have_grid) return fail(h, FXJPS_E_NOGRID, "no grid");
    if (channels != 1 && channels != 3) return fail(h, FXJPS_E_ARG, "channels must be 1 (L) or 3 (RGB)");
    DevCtx& d = h->devs[0];
    if (out_rows) *out_rows = d.H;  // mapsave.T[::-1]: rows = y extent, top row = largest y   :370
    if (out_cols) *out_cols = d.W;
    if (!out) return FXJPS_OK;
    HIPCHK(h, hipSetDevice(d.dev));
    const size_t n = (size_t)d.W * d.H * channels;
    HIPCHK(h, d.d_img.ensure(n));
    int rc = transpose_map(h, d, d.occ.p, d.W, d.H, 0, 1, fx::TM_OCC_TO_GRAY, channels, d.d_img.p);  // 0 -> 255, else 0   :368-369
    if (rc) return rc;
    HIPCHK(h, hipMemcpyAsync(out, d.d_img.p, n, hipMemcpyDeviceToHost, d.stream));
    HIPCHK(h, hipStreamSynchronize(d.stream));
    return FXJPS_OK;
}

namespace {
// Queue the cell updates and the rebuild of the derived maps on every device's stream (no host wait).
int update_cells_async(fxjps_t* h, const int32_t* xy, const uint8_t* val, int64_t n, bool derive) {
    if (!h->have_grid) return fail(h, FXJPS_E_NOGRID, "cell update before fxjps_set_grid");
    if (n < 0 || n > 0x7FFFFFF0ll || (n > 0 && (!xy || !val))) return fail(h, FXJPS_E_ARG, "bad update arrays");
    if (n == 0 && !(derive && h->maps_stale)) return FXJPS_OK;
    for (auto& d : h->devs) d.map_gen++;  // (the cells and the component labels change here, the other maps in derive_maps)
    // the box of the cells of the list that lie on the grid
    int bx0 = 0, bx1 = -1, by0 = 0, by1 = -1;
    bool have_box = false;
    {
        const DevCtx& d0 = h->devs[0];
        for (int64_t i = 0; i < n; i++) {
            const int x = xy[2 * i], y = xy[2 * i + 1];
            if (x < 0 || y < 0 || x >= d0.W || y >= d0.H) continue;
            bx0 = have_box ? std::min(bx0, x) : x;
            bx1 = have_box ? std::max(bx1, x) : x;
            by0 = have_box ? std::min(by0, y) : y;
            by1 = have_box ? std::max(by1, y) : y;
            have_box = true;
        }
    }
    static const bool partial = !(getenv("FXJPS_PARTIAL_DERIVE") && atoi(getenv("FXJPS_PARTIAL_DERIVE")) == 0);  // (0: measurement / test aid)
    // every device applies the same (small) update list; cheaper than re-broadcasting the grid
    for (auto& d : h->devs) {
        HIPCHK(h, hipSetDevice(d.dev));
        if (n > 0) {
            // The caller's arrays go through pinned staging buffers of the context: the call may return while the H2D
            // copies are still queued (fxjps_update_cells_deferred), and the caller owns its buffers again at once.
            // Before the staging buffers (and the device list the queued kernel reads) are reused, the previous
            // update's copies and kernel must be through: ev_upd.
            if (d.upd_pending) HIPCHK(h, hipEventSynchronize(d.ev_upd));
            d.upd_pending = false;
            // (coordinates and values travel as ONE copy: the values sit behind the coordinates in both buffers)
            const size_t nwords = (size_t)n * 2 + ((size_t)n + 3) / 4;
            HIPCHK(h, d.d_upd_xy.ensure(nwords));
            HIPCHK(h, d.h_upd_xy.ensure(nwords));
            memcpy(d.h_upd_xy.p, xy, (size_t)n * 2 * sizeof(int32_t));
            memcpy(d.h_upd_xy.p + (size_t)n * 2, val, (size_t)n);
            HIPCHK(h, hipMemcpyAsync(d.d_upd_xy.p, d.h_upd_xy.p, (size_t)n * 2 * sizeof(int32_t) + (size_t)n, hipMemcpyHostToDevice, d.stream));
        }
        const uint8_t* d_val = reinterpret_cast<const uint8_t*>(d.d_upd_xy.p + (size_t)n * 2);
        if (n > 0) {
            HIPCHK(h, d.d_upd_chg.ensure((size_t)n));
            if (!d.owner_ready) {  // (streaming callers only: allocated with the first update of a grid)
                HIPCHK(h, d.d_owner.ensure((size_t)d.W * d.H));
                HIPCHK(h, hipMemsetAsync(d.d_owner.p, 0xFF, (size_t)d.W * d.H * sizeof(int), d.stream));
                d.owner_ready = true;
            }
            const unsigned nbk = (unsigned)((n + 255) / 256);
            // the labels: a small update is united into them right away (the list is on the device now, not when the
            // maps are rebuilt); a large one, and every 64th small one, asks for the full relabelling
            static const long long small_max = getenv("FXJPS_CCL_SMALL") ? atoll(getenv("FXJPS_CCL_SMALL")) : 8192;  // (0: always relabel)
            const bool ccl_now = !d.ccl_full && n <= small_max && d.ccl_small < 64;
            // (measured and dropped in round 5: these four list kernels as ONE launch with barriers over its blocks -- 19 -> 15 us,
            // a 64 x 64 window update 0.091 -> 0.089 ms: a barrier across CUs costs what a launch costs)
            hipLaunchKernelGGL(fx::k_update_claim, dim3(nbk), dim3(256), 0, d.stream, d.d_owner.p, d.W, d.H, d.d_upd_xy.p, (long long)n);
            hipLaunchKernelGGL(fx::k_update_cells, dim3(nbk), dim3(256), 0, d.stream, d.occ.p, d.W, d.H, d.d_upd_xy.p, d_val,
                               (long long)n, d.d_upd_chg.p, d.d_owner.p);
            if (ccl_now) {
                // (measured and dropped in round 5: the two label kernels on the handle's second stream, beside the partial
                // rebuild that follows -- the fork / join events cost what the overlap gains: 0.091 ms either way)
                hipLaunchKernelGGL(fx::k_ccl_update, dim3(nbk), dim3(256), 0, d.stream, d.occ.p, d.W, d.H, d.d_upd_xy.p, d.d_upd_chg.p, (long long)n,
                                   d.comp.p, 0);
                hipLaunchKernelGGL(fx::k_ccl_update, dim3(nbk), dim3(256), 0, d.stream, d.occ.p, d.W, d.H, d.d_upd_xy.p, d.d_upd_chg.p, (long long)n,
                                   d.comp.p, 1);
                d.ccl_small++;
            } else {
                d.ccl_full = true;
            }
            HIPCHK(h, hipGetLastError());
            if (have_box) {  // padded coordinates: cell x sits at x + 1, its neighbours at x .. x + 2
                const int x0 = std::max(bx0, 0), x1 = std::min(bx1 + 2, d.PW - 1), y0 = std::max(by0, 0), y1 = std::min(by1 + 2, d.PH - 1);
                d.bx0 = d.dirty ? std::min(d.bx0, x0) : x0;
                d.bx1 = d.dirty ? std::max(d.bx1, x1) : x1;
                d.by0 = d.dirty ? std::min(d.by0, y0) : y0;
                d.by1 = d.dirty ? std::max(d.by1, y1) : y1;
                d.dirty = true;
            }
        }
        if (derive) {
            int rc = derive_maps(h, d, !partial);
            if (rc) {
                // The cells and the labels are already changed on the device (k_update_cells, k_ccl_update are queued), the
                // maps are not: whoever plans next must rebuild them (maps_stale), and the staging buffers stay taken until
                // what was queued has passed (ev_upd) -- the next update would otherwise overwrite a copy still in flight.
                h->maps_stale = true;
                d.dirty = true;
                if (n > 0 && hipEventRecord(d.ev_upd, d.stream) == hipSuccess) d.upd_pending = true;
                return rc;
            }
        }
        if (n > 0) {  // the list's last readers are queued: the staging buffers are free again once this event has passed
            HIPCHK(h, hipEventRecord(d.ev_upd, d.stream));
            d.upd_pending = true;
        }
    }
    h->maps_stale = !derive;
    return FXJPS_OK;
}

// Pinned staging buffer -> the caller's array.  The caller's array is as a rule freshly allocated (every page of it
// faults on the first store): beyond a few MB the copy is split over host threads (config 2: 23 MB of cells, 2.5 -> 1 ms).
static void host_copy(void* dst, const void* src, size_t bytes) {
    const size_t chunk = (size_t)2 << 20;
    const size_t nt = std::min<size_t>(8, bytes / chunk);
    if (nt < 2) {
        memcpy(dst, src, bytes);
        return;
    }
    const size_t per = ((bytes / nt) + 4095) & ~(size_t)4095;
    (void)run_side_by_side(nt, [=](size_t i) {
        const size_t o = i * per;
        if (o < bytes) memcpy((char*)dst + o, (const char*)src + o, std::min(per, bytes - o));
        return 0;
    });
}

// The last batch's cells of one context -> the caller's array: a copy of h_cells where they are there, otherwise (a
// streamed batch nobody has read on the host yet) expanded straight out of the arena, by query ranges over host threads --
// the caller's pages are touched once.
static void put_cells(const DevCtx& d, int32_t* dst) {
    const long long total = d.h_offsets.p[d.nq];
    if (d.cells_on_host) {
        host_copy(dst, d.h_cells.p, (size_t)total * 2 * sizeof(int32_t));
        return;
    }
    expand_arena(d, dst);
}

// plan_core's results -> the caller's CSR arrays
static int emit_csr(fxjps_t* h, int64_t nq, int64_t* out_offsets, int32_t* out_cells_xy, int64_t cells_capacity, int32_t* out_len,
             double* out_cost) {
    int64_t base = 0;
    bool fits = true;
    // every context's slice of the caller's arrays: where it starts is a prefix sum over the shards' totals, the copies
    // themselves are independent -- one host thread per context when there are several
    struct Put {
        DevCtx* d;
        int64_t base, total;
        bool cells;
    };
    std::vector<Put> puts;
    for (auto& d : h->devs) {
        if (d.nq == 0) continue;
        const int64_t total = d.h_offsets.p[d.nq];
        const bool cells = out_cells_xy && base + total <= cells_capacity && total > 0;
        if (out_cells_xy && base + total > cells_capacity) fits = false;  // (out_cells_xy == NULL: sizing call, the cells stay in the handle for fxjps_last_cells())
        puts.push_back(Put{&d, base, total, cells});
        base += total;
    }
    (void)run_side_by_side(puts.size(), [&](size_t i) {
        const Put& u = puts[i];
        const DevCtx* dp = u.d;
        memcpy(out_len + dp->q0, dp->h_len.p, (size_t)dp->nq * sizeof(int32_t));
        memcpy(out_cost + dp->q0, dp->h_cost.p, (size_t)dp->nq * sizeof(double));
        for (int64_t k = 0; k < dp->nq; k++) out_offsets[dp->q0 + k] = u.base + dp->h_offsets.p[k];
        if (u.cells) put_cells(*dp, out_cells_xy + 2 * u.base);
        return 0;
    });
    if (out_offsets) out_offsets[nq] = base;
    h->last.nq = nq;
    if (!fits) return fail(h, FXJPS_E_ARG, "out_cells_xy holds %lld pairs, batch needs %lld", (long long)cells_capacity, (long long)base);
    return FXJPS_OK;
}
}  // namespace

int fxjps_update_cells(fxjps_t* h, const int32_t* xy, const uint8_t* val, int64_t n) {
    if (!h) return FXJPS_E_ARG;
    h->q_results_valid = h->rs_valid = false;  // the grid changes behind the stored results
    if (int rc = update_cells_async(h, xy, val, n, true)) return rc;
    return wait_all(h);
}

int fxjps_update_cells_deferred(fxjps_t* h, const int32_t* xy, const uint8_t* val, int64_t n) {
    if (!h) return FXJPS_E_ARG;
    h->q_results_valid = h->rs_valid = false;  // the grid changes behind the stored results
    return update_cells_async(h, xy, val, n, false);  // queued; the next planning call (or fxjps_update_cells) rebuilds the maps
}

int fxjps_set_queries(fxjps_t* h, const int32_t* starts_xy, const int32_t* goals_xy, int64_t nq, int32_t hchoice,
                      int32_t max_path_len) {
    if (!h) return FXJPS_E_ARG;
    if (int rc = check_queries(h, starts_xy, goals_xy, nq, hchoice, max_path_len)) return rc;
    h->q_starts.assign(starts_xy, starts_xy + 2 * nq);  // copied: the caller's arrays are not kept
    h->q_goals.assign(goals_xy, goals_xy + 2 * nq);
    h->q_hchoice = hchoice;
    h->q_max_len = max_path_len;
    h->q_set = true;
    h->q_results_valid = h->rs_valid = false;
    return FXJPS_OK;
}

namespace {
// ---- exact reuse (fxjps_replan_frame, fxjps_replan_frame_raw).  Which read-set tiles does this frame's update touch?
// Derived data of a cell depends on the occupancy within Chebyshev distance 1, so every changed cell marks the tiles of
// its 3 x 3 neighbourhood; a stored result whose read set (see ReadSet in the kernels) misses all of them is what a
// from-scratch search on the new grid would return, bit for bit, and is not searched again.
struct FrameTiles {
    unsigned long long DX[64], DY[64];  // DX[y tile]: bit per x tile, DY[x tile]: bit per y tile
    FrameTiles() {
        memset(DX, 0, sizeof(DX));
        memset(DY, 0, sizeof(DY));
    }
    // the cells x0 .. x1, y0 .. y1 (on the grid) and their neighbours
    void mark_box(const DevCtx& d0, int x0, int x1, int y0, int y1) {
        const int tx0 = std::max(x0 - 1, 0) >> d0.tsh, tx1 = std::min(x1 + 1, d0.W - 1) >> d0.tsh;
        const int ty0 = std::max(y0 - 1, 0) >> d0.tsh, ty1 = std::min(y1 + 1, d0.H - 1) >> d0.tsh;
        for (int ty = ty0; ty <= ty1; ty++)
            for (int tx = tx0; tx <= tx1; tx++) {
                DX[ty] |= 1ull << tx;
                DY[tx] |= 1ull << ty;
            }
    }
    void mark_cells(const DevCtx& d0, const int32_t* xy, int64_t n) {
        for (int64_t i = 0; i < n; i++) {
            const int x = xy[2 * i], y = xy[2 * i + 1];
            if (x < 0 || y < 0 || x >= d0.W || y >= d0.H) continue;  // (k_update_cells ignores it as well)
            mark_box(d0, x, x, y, y);
        }
    }
};
// -> plan_core's mode for the frame (0 untracked, 1 everything searched and tracked, 2 the queries of DevCtx::h_sel
// searched); *track: the frame's results carry read sets; *reused: stored results handed back.  search_all: the stored
// results are void whatever their read sets say (the grid was rebuilt from scratch).
int frame_reuse_rule(fxjps_t* h, const FrameTiles& T, bool search_all, int64_t* out_reused, bool* out_track) {
    static const bool allow_reuse = !(getenv("FXJPS_REPLAN_REUSE") && atoi(getenv("FXJPS_REPLAN_REUSE")) == 0);
    const DevCtx& d0 = h->devs[0];
    int64_t touched = 0, tiles = (int64_t)(((d0.W - 1) >> d0.tsh) + 1) * (((d0.H - 1) >> d0.tsh) + 1);
    for (int t = 0; t < 64; t++) touched += __builtin_popcountll(T.DX[t]);
    // Recording read sets costs a few instructions per ray; it pays only when the next frame can reuse something.
    // A frame that touches most tiles (config 5: 10 % of all cells) leaves nothing to reuse: it runs untracked.
    const bool track = allow_reuse && 2 * touched <= tiles;
    int mode = track ? 1 : 0;
    int64_t reused = 0;
    if (track && h->q_results_valid && !search_all) {
        mode = 2;
        for (auto& d : h->devs) {
            d.h_sel.assign((size_t)d.nq, 1);  // (the shards are those of the previous frame: same query set)
            const int64_t dn = d.nq;
            for (int64_t q = 0; q < dn; q++) {
                if (d.h_len.p[q] <= 0) continue;  // no path / an error code: depends on more than a read set, search again
                const unsigned long long* bx = d.h_qread.data() + (size_t)q * 128;
                const unsigned long long* by = bx + 64;
                unsigned long long hit = 0;
                for (int t = 0; t < 64; t++) hit |= (bx[t] & T.DX[t]) | (by[t] & T.DY[t]);
                if (!hit) {
                    d.h_sel[(size_t)q] = 0;
                    reused++;
                }
            }
        }
    }
    *out_reused = reused;
    *out_track = track;
    return mode;
}
}  // namespace

int fxjps_replan_frame(fxjps_t* h, const int32_t* xy, const uint8_t* val, int64_t n, int64_t* out_offsets, int32_t* out_cells_xy,
                       int64_t cells_capacity, int32_t* out_len, double* out_cost, double* out_seconds_total) {
    const double t0 = now_s();
    if (!h) return FXJPS_E_ARG;
    if (!h->q_set) return fail(h, FXJPS_E_ARG, "fxjps_replan_frame before fxjps_set_queries");
    const int64_t nq = (int64_t)h->q_starts.size() / 2;
    if (nq > 0 && (!out_offsets || !out_len || !out_cost)) return fail(h, FXJPS_E_ARG, "NULL output array");
    if (!h->have_grid) return fail(h, FXJPS_E_NOGRID, "fxjps_replan_frame before fxjps_set_grid");
    if (n < 0 || (n > 0 && (!xy || !val))) return fail(h, FXJPS_E_ARG, "bad update arrays");
    FrameTiles T;
    T.mark_cells(h->devs[0], xy, n);
    int64_t reused = 0;
    bool track = false;
    const int mode = frame_reuse_rule(h, T, false, &reused, &track);
    // the frame's map update is queued in front of the search on the same streams: the first host wait of the frame
    // is the one for the search results
    h->q_results_valid = h->rs_valid = false;  // (set again below, once the frame is complete)
    int rc = update_cells_async(h, xy, val, n, true);
    if (rc) {
        drain_all(h);  // the devices in front of the failing one have the update queued
        return rc;
    }
    rc = plan_resident(h, h->q_starts.data(), h->q_goals.data(), nq, h->q_hchoice, h->q_max_len, mode);
    if (rc) return rc;
    h->q_results_valid = track;
    h->timing.reused = reused;
    return end_call(h, t0, out_seconds_total, emit_csr(h, nq, out_offsets, out_cells_xy, cells_capacity, out_len, out_cost));
}

namespace {
// ---- fxjps_refresh_grid / fxjps_replan_frame_raw: the prepared grid of a raw map against the
// resident one.  mode 0: no byte differs; 1: `changed` cells differ, their list is in the handle (refresh_xy / refresh_val);
// 2: the grid is to be rebuilt (no resident grid or other extents: changed == -1, nothing ran; more changed cells than the
// list holds).  box: the changed cells' bounding box (modes 1 and 2 behind a diff).
struct RefreshDiff {
    int mode = 2;
    int64_t changed = -1;
    bool staged = false;  // the raw map lies in context 0's d_raw
    int x0 = 0, x1 = -1, y0 = 0, y1 = -1;
};
int refresh_diff(fxjps_t* h, const PrepReq& q, RefreshDiff* r) {
    const fx::PrepGeom g = q.geom();
    DevCtx& d = h->devs[0];
    h->refresh_xy.clear();
    h->refresh_val.clear();
    if (!h->have_grid || g.W1 != d.W || g.H1 != d.H) return FXJPS_OK;
    const long long ncell = (long long)g.W1 * g.H1;
    const size_t raw_bytes = (size_t)q.W0 * q.H0;
    const uint32_t nblk = (uint32_t)((ncell + 255) / 256), cap = (uint32_t)std::max<long long>(4096, ncell / 8);
    constexpr uint32_t HEAD = 4096;  // entries of the list that travel with the header: a longer list takes a second copy
    HIPCHK(h, hipSetDevice(d.dev));
    HIPCHK(h, d.d_raw.ensure(raw_bytes));
    HIPCHK(h, d.d_diff.ensure((size_t)fx::DIFF_HDR + cap + nblk + 1));
    HIPCHK(h, d.h_diff.ensure((size_t)fx::DIFF_HDR + HEAD));
    uint32_t *hdr = d.d_diff.p, *list = hdr + fx::DIFF_HDR, *scan = list + cap;
    // (on the context's stream: behind cell updates that are still queued there, fxjps_update_cells_deferred)
    HIPCHK(h, hipMemcpyAsync(d.d_raw.p, q.raw, raw_bytes, hipMemcpyHostToDevice, d.stream));
    r->staged = true;
    HIPCHK(h, hipMemsetAsync(hdr, 0, fx::DIFF_HDR * sizeof(uint32_t), d.stream));
    hipLaunchKernelGGL(fx::k_grid_diff_count, dim3(nblk), dim3(256), 0, d.stream, d.d_raw.p, g, d.occ.p, hdr, scan);
    hipLaunchKernelGGL(fx::k_grid_diff_scan, dim3(1), dim3(1024), 0, d.stream, scan, nblk, hdr);
    hipLaunchKernelGGL(fx::k_grid_diff_write, dim3(nblk), dim3(256), 0, d.stream, d.d_raw.p, g, d.occ.p, scan, nblk, cap, list);
    HIPCHK(h, hipGetLastError());
    // (the goal rule on the resident grid in front of the same wait: a mode 0 has its record when it learns that it is one;
    // the other modes change the grid and queue the rule again behind that.  Launch behind launch, copy behind copy)
    if (int rc = goal_queue(h, q)) return rc;
    HIPCHK(h, hipMemcpyAsync(d.h_diff.p, hdr, ((size_t)fx::DIFF_HDR + HEAD) * sizeof(uint32_t), hipMemcpyDeviceToHost, d.stream));
    HIPCHK(h, hipStreamSynchronize(d.stream));
    const uint32_t n = d.h_diff.p[fx::DIFF_N];
    r->changed = n;
    if (n == 0) {
        r->mode = 0;
        return FXJPS_OK;
    }
    r->x0 = 8191 - (int)d.h_diff.p[fx::DIFF_X0];
    r->x1 = (int)d.h_diff.p[fx::DIFF_X1] - 1;
    r->y0 = 8191 - (int)d.h_diff.p[fx::DIFF_Y0];
    r->y1 = (int)d.h_diff.p[fx::DIFF_Y1] - 1;
    if (n > cap) return FXJPS_OK;  // (mode 2: the list was not written)
    h->refresh_xy.resize((size_t)n * 2);
    h->refresh_val.resize(n);
    const auto decode = [&](uint32_t k0, uint32_t k1) {  // entries k0 .. k1 - 1 out of the pinned buffer
        const uint32_t* e = d.h_diff.p + fx::DIFF_HDR;
        for (uint32_t k = k0; k < k1; k++) {
            h->refresh_xy[2 * (size_t)k] = (int32_t)(e[k] >> 16);
            h->refresh_xy[2 * (size_t)k + 1] = (int32_t)((e[k] >> 1) & 0x7FFFu);
            h->refresh_val[k] = (uint8_t)(e[k] & 1u);
        }
    };
    decode(0, std::min(n, HEAD));
    if (n > HEAD) {  // the rest of a long list: one more copy, into a buffer sized for the capacity once
        HIPCHK(h, d.h_diff.ensure((size_t)fx::DIFF_HDR + cap));
        HIPCHK(h, hipMemcpyAsync(d.h_diff.p + fx::DIFF_HDR + HEAD, list + HEAD, (size_t)(n - HEAD) * sizeof(uint32_t), hipMemcpyDeviceToHost, d.stream));
        HIPCHK(h, hipStreamSynchronize(d.stream));
        decode(HEAD, n);
    }
    r->mode = 1;
    return FXJPS_OK;
}

// The diff's outcome applied, queued on every context: the list through the cell-update path (which also rebuilds what
// deferred updates left stale, mode 0 included), or the whole build.
int refresh_apply(fxjps_t* h, const PrepReq& q, const RefreshDiff& r) {
    if (r.mode == 2) return prepare_build(h, q, r.staged);
    int rc = update_cells_async(h, h->refresh_xy.data(), h->refresh_val.data(), r.changed, true);
    if (rc) drain_all(h);  // the devices in front of the failing one have the update queued
    return rc;
}

// prepare_finish's `done` behind a diff, judged before the diff's outcome is applied: mode 2 waits in prepare_build; a
// mode 0 that owes no rebuild to deferred updates queues nothing more, and its goal record came back with the diff's header.
bool refresh_done(const fxjps_t* h, const RefreshDiff& r) { return r.mode == 2 || (r.mode == 0 && !h->maps_stale); }

int refresh_grid_impl(fxjps_t* h, PrepReq q, int64_t* out_changed, int32_t* out_mode) {
    if (!h) return FXJPS_E_ARG;
    RefreshDiff r;
    if (int rc = prepare_check(h, "fxjps_refresh_grid", &q)) return rc;
    h->q_results_valid = h->rs_valid = false;  // (as fxjps_update_cells: the grid may change behind the stored results)
    if (int rc = refresh_diff(h, q, &r)) return rc;
    if (out_changed) *out_changed = r.changed;
    if (out_mode) *out_mode = r.mode;
    const bool done = refresh_done(h, r);
    if (int rc = refresh_apply(h, q, r)) return rc;
    return prepare_finish(h, q, done);
}

int replan_frame_raw_impl(fxjps_t* h, PrepReq q, int64_t* out_changed, int32_t* out_mode, int64_t* out_offsets, int32_t* out_cells_xy,
                          int64_t cells_capacity, int32_t* out_len, double* out_cost, double* out_seconds_total) {
    const double t0 = now_s();
    if (!h) return FXJPS_E_ARG;
    RefreshDiff r;
    if (int rc = prepare_check(h, "fxjps_replan_frame_raw", &q)) return rc;
    const int64_t nq = (int64_t)h->q_starts.size() / 2;
    if (h->q_set && nq > 0 && (!out_offsets || !out_len || !out_cost)) return fail(h, FXJPS_E_ARG, "NULL output array");
    if (!h->q_set || !h->have_grid || q.p.W1 != h->devs[0].W || q.p.H1 != h->devs[0].H)
        return fail(h, FXJPS_E_ARG, "fxjps_replan_frame_raw needs stored queries and a resident grid of the prepared extents (%lldx%lld): call "
                    "fxjps_prepare_grid and fxjps_set_queries again", q.p.W1, q.p.H1);
    if (int rc = refresh_diff(h, q, &r)) return rc;
    if (out_changed) *out_changed = r.changed;
    if (out_mode) *out_mode = r.mode;
    // fxjps_replan_frame's rule on the diff's list; a diff too long for its list marks the tiles of its box, and every query is searched
    FrameTiles T;
    if (r.mode == 1) T.mark_cells(h->devs[0], h->refresh_xy.data(), r.changed);
    if (r.mode == 2) T.mark_box(h->devs[0], r.x0, r.x1, r.y0, r.y1);
    int64_t reused = 0;
    bool track = false;
    const int mode = frame_reuse_rule(h, T, r.mode == 2, &reused, &track);
    h->q_results_valid = h->rs_valid = false;  // (set again below, once the frame is complete)
    const bool done = refresh_done(h, r);
    if (int rc = refresh_apply(h, q, r)) return rc;
    int rc = plan_resident(h, h->q_starts.data(), h->q_goals.data(), nq, h->q_hchoice, h->q_max_len, mode);
    if (rc) return rc;
    h->q_results_valid = track;
    h->timing.reused = reused;
    rc = emit_csr(h, nq, out_offsets, out_cells_xy, cells_capacity, out_len, out_cost);
    if (rc) return rc;
    return end_call(h, t0, out_seconds_total, prepare_finish(h, q, done));  // (its wait: a context without queries of the batch has not waited for its update)
}
}  // namespace

int fxjps_refresh_grid(fxjps_t* h, const uint8_t* raw, int32_t W0, int32_t H0, int32_t ifa, int32_t variant, int32_t* start_xy,
                       int32_t* goal_xy, int32_t* out_W, int32_t* out_H, int32_t* out_map_d, int32_t* out_end_occu, int64_t* out_changed,
                       int32_t* out_mode) {
    return refresh_grid_impl(h, PrepReq{raw, W0, H0, ifa, variant, 0, start_xy, goal_xy, out_W, out_H, out_map_d, out_end_occu, {}}, out_changed, out_mode);
}

int fxjps_refresh_occupancy_msg(fxjps_t* h, const int8_t* data, int32_t width, int32_t height, int32_t ifa, int32_t variant, int32_t* start_xy,
                                int32_t* goal_xy, int32_t* out_W, int32_t* out_H, int32_t* out_map_d, int32_t* out_end_occu,
                                int64_t* out_changed, int32_t* out_mode) {
    return refresh_grid_impl(h, PrepReq{reinterpret_cast<const uint8_t*>(data), width, height, ifa, variant, 1, start_xy, goal_xy, out_W, out_H,
                                        out_map_d, out_end_occu, {}}, out_changed, out_mode);
}

int fxjps_last_refresh_cells(fxjps_t* h, int32_t* out_xy, uint8_t* out_val, int64_t capacity, int64_t* out_n) {
    if (!h || !out_n) return FXJPS_E_ARG;
    const int64_t n = (int64_t)h->refresh_val.size();
    *out_n = n;
    if (!out_xy && !out_val) return FXJPS_OK;  // (sizing call)
    if (!out_xy || !out_val || capacity < n) return fail(h, FXJPS_E_ARG, "the last refresh changed %lld cells, the arrays hold %lld", (long long)n, (long long)capacity);
    if (n > 0) {
        memcpy(out_xy, h->refresh_xy.data(), (size_t)n * 2 * sizeof(int32_t));
        memcpy(out_val, h->refresh_val.data(), (size_t)n);
    }
    return FXJPS_OK;
}

int fxjps_replan_frame_raw(fxjps_t* h, const void* raw, int32_t layout, int32_t W0, int32_t H0, int32_t ifa, int32_t variant, int32_t* start_xy,
                           int32_t* goal_xy, int32_t* out_W, int32_t* out_H, int32_t* out_map_d, int32_t* out_end_occu, int64_t* out_changed,
                           int32_t* out_mode, int64_t* out_offsets, int32_t* out_cells_xy, int64_t cells_capacity, int32_t* out_len,
                           double* out_cost, double* out_seconds_total) {
    if (h && layout != 0 && layout != 1) return fail(h, FXJPS_E_ARG, "layout must be 0 (matrix [x][y]) or 1 (message data[])");
    return replan_frame_raw_impl(h, PrepReq{static_cast<const uint8_t*>(raw), W0, H0, ifa, variant, layout, start_xy, goal_xy, out_W, out_H, out_map_d,
                                            out_end_occu, {}},
                                 out_changed, out_mode, out_offsets, out_cells_xy, cells_capacity, out_len, out_cost, out_seconds_total);
}

int fxjps_plan_batch_csr(fxjps_t* h, const int32_t* starts_xy, const int32_t* goals_xy, int64_t nq,
                         int32_t hchoice, int32_t max_path_len, int64_t* out_offsets, int32_t* out_cells_xy,
                         int64_t cells_capacity, int32_t* out_len, double* out_cost, double* out_seconds_total) {
    const double t0 = now_s();
    if (!h) return FXJPS_E_ARG;
    if (nq > 0 && (!out_offsets || !out_len || !out_cost)) return fail(h, FXJPS_E_ARG, "NULL output array");
    int rc = plan_resident(h, starts_xy, goals_xy, nq, hchoice, max_path_len);
    if (rc) return rc;
    return end_call(h, t0, out_seconds_total, emit_csr(h, nq, out_offsets, out_cells_xy, cells_capacity, out_len, out_cost));
}

namespace {
// A context's slot tables, created by the first call that sets a slot (the context is current).
int ensure_slot_tables(fxjps_t* h, DevCtx& d) {
    if (d.slots.empty()) {
        d.slots.resize(FXJPS_MAX_GRID_SLOTS);
        d.h_slot_desc.assign(FXJPS_MAX_GRID_SLOTS, GridDev{});
        HIPCHK(h, d.d_slot_desc.ensure(FXJPS_MAX_GRID_SLOTS));
    }
    return FXJPS_OK;
}
// A slot whose call failed on one context is released on all of them, and every context's descriptor says so.
void release_slot_everywhere(fxjps_t* h, int32_t slot) {
    const size_t s = (size_t)slot;
    for (auto& d : h->devs) {
        if (d.slots.empty()) continue;
        const bool current = hipSetDevice(d.dev) == hipSuccess;
        if (current) d.slots[s].release();
        d.slots[s].W = 0;
        d.h_slot_desc[s] = GridDev{};
        if (current) (void)hipMemcpy(d.d_slot_desc.p + s, &d.h_slot_desc[s], sizeof(GridDev), hipMemcpyHostToDevice);
    }
}
}  // namespace

int fxjps_set_grid_slot(fxjps_t* h, int32_t slot, const uint8_t* occ, int32_t W, int32_t H) {
    if (!h) return FXJPS_E_ARG;
    if (slot < 0 || slot >= FXJPS_MAX_GRID_SLOTS) return fail(h, FXJPS_E_ARG, "slot %d is not in 0 .. %d", (int)slot, FXJPS_MAX_GRID_SLOTS - 1);
    if (occ && (W < 1 || H < 1 || W > 8190 || H > 8190)) return fail(h, FXJPS_E_ARG, "grid must be 1..8190 cells a side");
    if (int rr = refuse_on_rank_handle(h, "fxjps_set_grid_slot")) return rr;
    h->bump_slot(slot);  // (whatever becomes of the call: the slot's bytes are about to be written or released)
    // Every context gets its own copy from the host (no collective), builds the maps on its own streams, and refreshes its
    // table of slot descriptors.  The resident grid and its update state are not touched.
    int rc = run_side_by_side(h->devs.size(), [&](size_t r) -> int {
        DevCtx& d = h->devs[r];
        HIPCHK(h, hipSetDevice(d.dev));
        if (int e = ensure_slot_tables(h, d)) return e;
        GridBufs& g = d.slots[(size_t)slot];
        HIPCHK(h, hipStreamSynchronize(d.stream));  // (whatever is queued may still read the slot's buffers)
        if (!occ) {
            g.release();
            d.h_slot_desc[(size_t)slot] = GridDev{};
        } else {
            g.W = 0;  // (empty until its maps are built: a failure below leaves the slot released, not half-set)
            d.h_slot_desc[(size_t)slot] = GridDev{};
            int e = alloc_grid_bufs(h, g, W, H);
            if (e) {
                g.release();
                return e;
            }
            HIPCHK(h, hipMemcpyAsync(g.occ.p, occ, (size_t)W * H, hipMemcpyHostToDevice, d.stream));
            e = derive_maps(h, d, true, &g);
            if (e) {
                g.release();
                return e;
            }
            d.h_slot_desc[(size_t)slot] = grid_of(g);
        }
        HIPCHK(h, hipMemcpyAsync(d.d_slot_desc.p + slot, &d.h_slot_desc[(size_t)slot], sizeof(GridDev), hipMemcpyHostToDevice, d.stream));
        HIPCHK(h, hipStreamSynchronize(d.stream));
        return FXJPS_OK;
    });
    if (rc) {
        drain_all(h);
        release_slot_everywhere(h, slot);
        (void)hipGetLastError();
    }
    return rc;
}

int fxjps_get_grid_slot(fxjps_t* h, int32_t slot, uint8_t* out, int32_t* out_W, int32_t* out_H) {
    if (!h) return FXJPS_E_ARG;
    if (!slot_in_use(h, slot)) return fail(h, FXJPS_E_ARG, "grid slot %d is empty or out of range", (int)slot);
    DevCtx& d = h->devs[0];
    const GridBufs& g = d.slots[(size_t)slot];
    if (out_W) *out_W = g.W;
    if (out_H) *out_H = g.H;
    if (out) {
        HIPCHK(h, hipSetDevice(d.dev));
        HIPCHK(h, hipMemcpyAsync(out, g.occ.p, (size_t)g.W * g.H, hipMemcpyDeviceToHost, d.stream));
        HIPCHK(h, hipStreamSynchronize(d.stream));
    }
    return FXJPS_OK;
}

// ------------------------------------------------------------------ many raw maps into grid slots, one call
int fxjps_slot_job_size(void) { return (int)sizeof(fxjps_slot_job_t); }

namespace {
static_assert(fx::SLOT_JOBS_MAX == FXJPS_MAX_GRID_SLOTS, "the job table of fxjps_prepare_slots holds one job per slot");
// A world-frame job's two sources, in canvas cells (fxjps_prepare_slots_world): the job handed to slots_call has the canvas
// extents as W0 / H0 and the detected map as raw.
struct WorldSrc {
    int prior;           // -1: none
    int rW, rH, rx, ry;  // the detected map: its extents, where it lies
    int px, py;          // where the prior lies
};
struct WorldCall {
    const WorldSrc* src;
    size_t off;  // of the fx::WorldSrcDev records inside the staged input
};
// The staged input of a call: the job table, the context's 256 slot descriptors as they will be, then the raw maps.
constexpr size_t SLOTS_IN_DESC = (sizeof(fx::SlotTable) + 15) & ~(size_t)15;
constexpr size_t SLOTS_IN_RAWS = (SLOTS_IN_DESC + sizeof(GridDev) * FXJPS_MAX_GRID_SLOTS + 15) & ~(size_t)15;

// Job j's rows of the table: the blocks derive_maps would launch for this grid alone (the fused build: at most 2^18 cells;
// a larger grid has no blocks in the build launches), behind the blocks of the first launch, each of which covers
// `first_cells` cells of the grid.  T.job[j].G is set.  -> whether the grid takes the fused build.
bool slot_job_blocks(fx::SlotTable& T, int j, const GridBufs& g, long long first_cells, uint32_t at[fx::SL_LAUNCHES]) {
    fx::SlotJobDev& J = T.job[j];
    const long long ncell = (long long)g.W * g.H, npad = (long long)g.PW * g.PH;
    const bool fused = ncell <= (1ll << 18);
    J.nb_rows = (uint32_t)(((long long)g.PW * g.WORDS + 3) / 4);
    J.nb_cols = (uint32_t)(((long long)g.PH * g.WORDS + 3) / 4);
    J.nb_ci = (uint32_t)((npad + 255) / 256);
    J.nb_diag = (uint32_t)((4ll * J.G.DLINES * g.WORDS + 15) / 16);
    const uint32_t nb_cell = (uint32_t)((ncell + 255) / 256), nb_flat = (uint32_t)((ncell + 1023) / 1024);
    const uint32_t cnt[fx::SL_LAUNCHES] = {(uint32_t)((ncell + first_cells - 1) / first_cells), fused ? J.nb_rows + J.nb_cols + nb_cell : 0u,
                                           fused ? J.nb_ci + nb_cell : 0u, fused ? J.nb_diag + nb_flat : 0u,
                                           fused ? (uint32_t)((npad * 8 + 255) / 256) : 0u};
    for (int l = 0; l < fx::SL_LAUNCHES; l++) {
        T.first[l][j] = at[l];
        at[l] += cnt[l];
    }
    return fused;
}

// One context's part of fxjps_prepare_slots / fxjps_refresh_slots: everything is queued on d.stream behind ONE copy in, and
// waited for ONCE, whatever n is.  The results are left in d.h_slots_res.  refresh: a job whose slot holds a grid of the
// prepared extents is compared with it byte by byte while it is gathered, and built only if a byte differed (DESIGN.md
// section 3.12); the n `changed` words travel in behind the raws and come back behind the results, in the same two copies.
// staged_raw (a cropped call's second phase, fxjps_prepare_slots_cropped): the raws are on the device already, job j's at
// that offset of the context's window buffer, and none is copied or staged again.
// tiles (a refresh under fxjps_set_slot_reuse(1)): the gather is the form that marks the changed
// tiles.  The n records of 128 words travel in zeroed behind the `changed` words, and the results are written beside them
// in the staged input's device copy, so that results and records come back in the one copy out: d.h_slots_res holds the
// results as ever and the records from word d.slot_tiles_at on.
int prepare_slots_on(fxjps* h, DevCtx& d, const fxjps_slot_job_t* jobs, int n, const std::vector<SlotPlan>& plan, size_t in_bytes, bool refresh,
                     const WorldCall* world, const size_t* staged_raw, bool tiles) {
    HIPCHK(h, hipSetDevice(d.dev));
    if (int e = ensure_slot_tables(h, d)) return e;
    // (no host wait in front: every call of the library that reads a slot has returned; a buffer that grows is freed by
    // hipFree, which waits for the device itself)
    const size_t flags_off = in_bytes, n_res = (size_t)n * (fx::SLOT_RES + (refresh ? 1 : 0));
    if (refresh) in_bytes += (size_t)n * sizeof(uint32_t);  // (every raw's room is a multiple of 16 bytes: the words are aligned)
    const size_t res_bytes = (n_res * sizeof(int32_t) + 7) & ~(size_t)7, rec_bytes = (size_t)n * 128 * sizeof(unsigned long long);
    size_t res_off = 0;
    if (tiles) {  // [changed words | results | records], the last two as they come back
        res_off = in_bytes = (in_bytes + 15) & ~(size_t)15;
        in_bytes += res_bytes + rec_bytes;
    }
    HIPCHK(h, d.h_slots_in.ensure(in_bytes));
    HIPCHK(h, d.d_slots_in.ensure(in_bytes));
    HIPCHK(h, d.h_slots_res.ensure(tiles ? (res_bytes + rec_bytes) / sizeof(int32_t) : n_res));
    if (!tiles) HIPCHK(h, d.d_slots_res.ensure(n_res));
    d.slot_tiles_at = res_bytes / sizeof(int32_t);
    if (tiles) memset(d.h_slots_in.p + res_off, 0, res_bytes + rec_bytes);
    int32_t* d_res = tiles ? reinterpret_cast<int32_t*>(d.d_slots_in.p + res_off) : d.d_slots_res.p;
    unsigned long long* d_rec = tiles ? reinterpret_cast<unsigned long long*>(d.d_slots_in.p + res_off + res_bytes) : nullptr;
    fx::SlotTable& T = *reinterpret_cast<fx::SlotTable*>(d.h_slots_in.p);
    uint32_t* h_changed = reinterpret_cast<uint32_t*>(d.h_slots_in.p + flags_off);
    uint32_t* d_changed = reinterpret_cast<uint32_t*>(d.d_slots_in.p + flags_off);
    fx::WorldSrcDev* h_world = world ? reinterpret_cast<fx::WorldSrcDev*>(d.h_slots_in.p + world->off) : nullptr;
    uint32_t at[fx::SL_LAUNCHES] = {};
    bool any_large = false;
    for (int j = 0; j < n; j++) {
        const fxjps_slot_job_t& jb = jobs[j];
        const SlotPlan& p = plan[(size_t)j];
        GridBufs& g = d.slots[(size_t)jb.slot];
        // (what this context's copy of the slot holds now; a grid beyond the fused build is built by the host below, which
        // cannot know the device's word without a wait: it always builds)
        const bool compare = refresh && g.W > 0 && g.W == p.W1 && g.H == p.H1 && p.W1 * p.H1 <= (1ll << 18);
        d.h_slot_desc[(size_t)jb.slot] = GridDev{};
        int e = alloc_grid_bufs(h, g, (int)p.W1, (int)p.H1);  // (a slot that has room allocates nothing)
        if (e) return e;
        const GridDev G = grid_of(g);
        d.h_slot_desc[(size_t)jb.slot] = G;
        fx::SlotJobDev& J = T.job[j];
        J.G = G;
        J.occ = g.occ.p;
        J.raw = staged_raw ? d.d_crop_win.p + staged_raw[j] : d.d_slots_in.p + p.raw_off;
        J.W0 = jb.W0;
        J.H0 = jb.H0;
        J.dx = (int32_t)p.dx;
        J.dy = (int32_t)p.dy;
        J.ifa = jb.ifa;
        J.variant = jb.variant;
        J.layout = jb.layout;
        J.gx = (int32_t)p.ngx;
        J.gy = (int32_t)p.ngy;
        J.compare = compare ? 1 : 0;
        if (refresh) h_changed[j] = compare ? 0u : 1u;  // (written anew by every call: nothing of the call before is read)
        if (world) {  // (only the detected map is staged: the prior's bytes are on the device already)
            const WorldSrc& w = world->src[j];
            fx::WorldSrcDev& S = h_world[j];
            S = fx::WorldSrcDev{nullptr, 0, 0, 0, 0, w.rW, w.rH, w.rx, w.ry};
            if (w.prior >= 0) {
                const DevCtx::PriorBuf& pr = d.priors[(size_t)w.prior];
                S.prior = pr.occ.p;
                S.pW = pr.W;
                S.pH = pr.H;
                S.px = w.px;
                S.py = w.py;
            }
            if (!staged_raw) memcpy(d.h_slots_in.p + p.raw_off, jb.raw, (size_t)w.rW * (size_t)w.rH);
        } else {
            memcpy(d.h_slots_in.p + p.raw_off, jb.raw, (size_t)jb.W0 * (size_t)jb.H0);
        }
        any_large = !slot_job_blocks(T, j, g, 256, at) || any_large;
    }
    for (int l = 0; l < fx::SL_LAUNCHES; l++) T.first[l][n] = at[l];
    memcpy(d.h_slots_in.p + SLOTS_IN_DESC, d.h_slot_desc.data(), sizeof(GridDev) * FXJPS_MAX_GRID_SLOTS);
    HIPCHK(h, hipMemcpyAsync(d.d_slots_in.p, d.h_slots_in.p, in_bytes, hipMemcpyHostToDevice, d.stream));
    const fx::SlotTable* dT = reinterpret_cast<const fx::SlotTable*>(d.d_slots_in.p);
    // the instantiation of each launch by (world, refresh); the forms that do not read the sources or the words get nullptr
    using GatherFn = void (*)(const fx::SlotTable*, const fx::WorldSrcDev*, int, uint32_t*);
    using GoalFn = void (*)(const fx::SlotTable*, int32_t*, int, const uint32_t*);
    using StageFn = void (*)(const fx::SlotTable*, int, const uint32_t*);
    static const GatherFn gather[2][2] = {{fx::k_slots_gather<false, false>, fx::k_slots_gather<false, true>},
                                          {fx::k_slots_gather<true, false>, fx::k_slots_gather<true, true>}};
    static const GoalFn goal[2] = {fx::k_slots_goal<false>, fx::k_slots_goal<true>};
    static const StageFn stage[2][4] = {
        {fx::k_slots_stage<fx::SL_BUILD_1, false>, fx::k_slots_stage<fx::SL_BUILD_2, false>, fx::k_slots_stage<fx::SL_BUILD_3, false>, fx::k_slots_stage<fx::SL_JD, false>},
        {fx::k_slots_stage<fx::SL_BUILD_1, true>, fx::k_slots_stage<fx::SL_BUILD_2, true>, fx::k_slots_stage<fx::SL_BUILD_3, true>, fx::k_slots_stage<fx::SL_JD, true>}};
    const fx::WorldSrcDev* dS = world ? reinterpret_cast<const fx::WorldSrcDev*>(d.d_slots_in.p + world->off) : nullptr;
    uint32_t* dC = refresh ? d_changed : nullptr;
    if (tiles)
        hipLaunchKernelGGL(world ? fx::k_slot_tiles_gather<true> : fx::k_slot_tiles_gather<false>, dim3(at[fx::SL_PREPARE]), dim3(256), 0, d.stream, dT, dS,
                           n, dC, d_rec);
    else
        hipLaunchKernelGGL(gather[world ? 1 : 0][refresh ? 1 : 0], dim3(at[fx::SL_PREPARE]), dim3(256), 0, d.stream, dT, dS, n, dC);
    hipLaunchKernelGGL(goal[refresh ? 1 : 0], dim3((unsigned)n), dim3(64), 0, d.stream, dT, d_res, n, (const uint32_t*)dC);
    if (at[fx::SL_BUILD_1] > 0)
        for (int l = fx::SL_BUILD_1; l <= fx::SL_JD; l++)
            hipLaunchKernelGGL(stage[refresh ? 1 : 0][l - fx::SL_BUILD_1], dim3(at[l]), dim3(l == fx::SL_BUILD_3 ? 1024 : 256), 0, d.stream, dT, n,
                               (const uint32_t*)dC);
    HIPCHK(h, hipGetLastError());
    if (any_large)  // (grids beyond the fused build: their maps one by one, as fxjps_set_grid_slot builds them)
        for (int j = 0; j < n; j++)
            if (plan[(size_t)j].W1 * plan[(size_t)j].H1 > (1ll << 18)) {
                int e = derive_maps(h, d, true, &d.slots[(size_t)jobs[j].slot]);
                if (e) return e;
            }
    HIPCHK(h, hipMemcpyAsync(d.d_slot_desc.p, d.h_slots_in.p + SLOTS_IN_DESC, sizeof(GridDev) * FXJPS_MAX_GRID_SLOTS, hipMemcpyHostToDevice, d.stream));
    HIPCHK(h, hipMemcpyAsync(d.h_slots_res.p, d_res, tiles ? res_bytes + rec_bytes : n_res * sizeof(int32_t), hipMemcpyDeviceToHost, d.stream));
    HIPCHK(h, hipStreamSynchronize(d.stream));
    // a goal with no free cell in its row or column: that slot stays empty (its buffers keep their room)
    for (int j = 0; j < n; j++)
        if (d.h_slots_res.p[(size_t)j * fx::SLOT_RES + 3] != 0) {
            const size_t s = (size_t)jobs[j].slot;
            d.slots[s].W = d.slots[s].H = 0;
            d.h_slot_desc[s] = GridDev{};
            HIPCHK(h, hipMemcpy(d.d_slot_desc.p + s, &d.h_slot_desc[s], sizeof(GridDev), hipMemcpyHostToDevice));
        }
    return FXJPS_OK;
}
}  // namespace

namespace {
// what a context's last slots call staged and brought back: was job j compared; the tile records behind the results
bool job_compared(const DevCtx& d, int j) { return reinterpret_cast<const fx::SlotTable*>(d.h_slots_in.p)->job[j].compare != 0; }
const unsigned long long* slot_tile_records(const DevCtx& d) { return reinterpret_cast<const unsigned long long*>(d.h_slots_res.p + d.slot_tiles_at); }

// fxjps_prepare_slots (out_kept == nullptr, refresh false) and fxjps_refresh_slots: the checks, the call on every context
// and the outputs are the same code.
int slots_call(fxjps_t* h, fxjps_slot_job_t* jobs, int32_t n, bool refresh, int32_t* out_kept, const char* what, const WorldSrc* world_src = nullptr,
               const size_t* staged_raw = nullptr) {
    if (int rc = jobs_call_check(h, jobs, n, what)) return rc;
    // everything the host can judge, for every job, before anything is queued or any slot is touched
    std::vector<SlotPlan> plan((size_t)n);
    std::vector<int> named(FXJPS_MAX_GRID_SLOTS, -1);
    size_t in_bytes = SLOTS_IN_RAWS;
    for (int j = 0; j < n; j++) {
        const fxjps_slot_job_t& jb = jobs[j];
        if (jb.slot < 0 || jb.slot >= FXJPS_MAX_GRID_SLOTS) return fail(h, FXJPS_E_ARG, "job %d: slot %d is not in 0 .. %d", j, (int)jb.slot, FXJPS_MAX_GRID_SLOTS - 1);
        if (named[(size_t)jb.slot] >= 0) return fail(h, FXJPS_E_ARG, "job %d: slot %d is already named by job %d", j, (int)jb.slot, named[(size_t)jb.slot]);
        named[(size_t)jb.slot] = j;
        if (!jb.raw) return fail(h, FXJPS_E_ARG, "job %d: NULL raw", j);
        if (jb.W0 < 1 || jb.H0 < 1 || jb.ifa < 0 || jb.ifa > 64 || (jb.variant != 0 && jb.variant != 1) || (jb.layout != 0 && jb.layout != 1))
            return fail(h, FXJPS_E_ARG, "job %d: bad arguments (W0 %d, H0 %d, ifa %d, variant %d, layout %d)", j, (int)jb.W0, (int)jb.H0, (int)jb.ifa,
                        (int)jb.variant, (int)jb.layout);
        SlotPlan& p = plan[(size_t)j];
        p = prepared_geometry(jb.W0, jb.H0, jb.ifa, jb.variant, jb.start_xy, jb.goal_xy);
        if (p.W1 > 8190 || p.H1 > 8190) return fail(h, FXJPS_E_ARG, "job %d: prepared grid %lldx%lld exceeds 8190 cells a side", j, p.W1, p.H1);
        if (p.ngx < 0 || p.ngy < 0 || p.ngx >= p.W1 || p.ngy >= p.H1)
            return fail(h, FXJPS_E_ARG, "job %d: goal (%lld, %lld) outside the prepared grid %lldx%lld", j, p.ngx, p.ngy, p.W1, p.H1);
        p.raw_off = in_bytes;
        const size_t raw_bytes = staged_raw ? 0 : world_src ? (size_t)world_src[j].rW * (size_t)world_src[j].rH : (size_t)jb.W0 * (size_t)jb.H0;
        in_bytes += (raw_bytes + 15) & ~(size_t)15;
    }
    if (n == 0) return FXJPS_OK;
    WorldCall wc{world_src, in_bytes};
    const WorldCall* world = world_src ? &wc : nullptr;
    if (world) in_bytes += ((size_t)n * sizeof(fx::WorldSrcDev) + 15) & ~(size_t)15;
    // every context prepares every job from the caller's raws (host copies, no collective, as fxjps_set_grid_slot)
    const bool tiles = refresh && h->slot_reuse == 1;
    int rc = run_side_by_side(h->devs.size(),
                              [&](size_t r) -> int { return prepare_slots_on(h, h->devs[r], jobs, n, plan, in_bytes, refresh, world, staged_raw, tiles); });
    if (rc) {
        drain_all(h);
        for (int j = 0; j < n; j++) {  // (slots of a call that failed on one context are released on all of them)
            release_slot_everywhere(h, jobs[j].slot);
            h->bump_slot(jobs[j].slot);
        }
        (void)hipGetLastError();
        return rc;
    }
    const int32_t* res = h->devs[0].h_slots_res.p;  // (every context computed the same)
    for (int j = 0; j < n; j++) {
        fxjps_slot_job_t& jb = jobs[j];
        const SlotPlan& p = plan[(size_t)j];
        jb.start_xy[0] = (int32_t)p.nsx;
        jb.start_xy[1] = (int32_t)p.nsy;
        jb.goal_xy[0] = res[(size_t)j * fx::SLOT_RES + 0];
        jb.goal_xy[1] = res[(size_t)j * fx::SLOT_RES + 1];
        jb.W = (int32_t)p.W1;
        jb.H = (int32_t)p.H1;
        jb.map_d[0] = (int32_t)p.dx;
        jb.map_d[1] = (int32_t)p.dy;
        jb.end_occu = res[(size_t)j * fx::SLOT_RES + 2];
        jb.status = res[(size_t)j * fx::SLOT_RES + 3] != 0 ? FXJPS_E_ARG : FXJPS_OK;
        // kept: no byte of context 0's copy differed, so nothing was built (a job that failed has an empty slot: not kept)
        const bool kept = refresh && jb.status == FXJPS_OK && res[(size_t)n * fx::SLOT_RES + (size_t)j] == 0;
        if (out_kept) out_kept[j] = kept ? 1 : 0;
        if (kept) continue;
        // built, or left empty; a prepare always builds.  A compared job under the tile rule says where: its marks join the
        // slot's record (context 0's, as `kept`), whose validity stays what it was; every other write voids the record.
        if (tiles && jb.status == FXJPS_OK && job_compared(h->devs[0], j))
            h->mark_slot(jb.slot, slot_tile_records(h->devs[0]) + (size_t)j * 128);
        else
            h->bump_slot(jb.slot);
    }
    return FXJPS_OK;
}
}  // namespace

int fxjps_prepare_slots(fxjps_t* h, fxjps_slot_job_t* jobs, int32_t n) { return slots_call(h, jobs, n, false, nullptr, "fxjps_prepare_slots"); }

int fxjps_refresh_slots(fxjps_t* h, fxjps_slot_job_t* jobs, int32_t n, int32_t* out_kept) {
    return slots_call(h, jobs, n, true, out_kept, "fxjps_refresh_slots");
}

// ------------------------------------------------------------------ many prepared grids into grid slots, one call
int fxjps_grid_job_size(void) { return (int)sizeof(fxjps_grid_job_t); }

namespace {
// One context's part of fxjps_set_grid_slots / fxjps_refresh_grid_slots: prepare_slots_on with the
// copy launch in place of the gather, no goal launch, and the grids where the raws were (off[j], multiples of 16 bytes).
// refresh: the `changed` words travel in behind the grids and come back into d.h_slots_res, one word per job.
// tiles: the copy is the form that marks the changed tiles; the records travel in zeroed behind the
// words and come back behind them in the one copy out, from word d.slot_tiles_at of d.h_slots_res on.
int grid_slots_on(fxjps* h, DevCtx& d, const fxjps_grid_job_t* jobs, int n, const std::vector<size_t>& off, size_t in_bytes, bool refresh, bool tiles) {
    HIPCHK(h, hipSetDevice(d.dev));
    if (int e = ensure_slot_tables(h, d)) return e;
    const size_t flags_off = in_bytes;
    if (refresh) in_bytes += (size_t)n * sizeof(uint32_t);
    const size_t words_bytes = ((size_t)n * sizeof(uint32_t) + 7) & ~(size_t)7, rec_bytes = (size_t)n * 128 * sizeof(unsigned long long);
    if (tiles) in_bytes = flags_off + words_bytes + rec_bytes;
    HIPCHK(h, d.h_slots_in.ensure(in_bytes));
    HIPCHK(h, d.d_slots_in.ensure(in_bytes));
    if (refresh) HIPCHK(h, d.h_slots_res.ensure(tiles ? (words_bytes + rec_bytes) / sizeof(int32_t) : (size_t)n));
    d.slot_tiles_at = words_bytes / sizeof(int32_t);
    if (tiles) memset(d.h_slots_in.p + flags_off, 0, words_bytes + rec_bytes);
    fx::SlotTable& T = *reinterpret_cast<fx::SlotTable*>(d.h_slots_in.p);
    uint32_t* h_changed = reinterpret_cast<uint32_t*>(d.h_slots_in.p + flags_off);
    uint32_t* d_changed = reinterpret_cast<uint32_t*>(d.d_slots_in.p + flags_off);
    uint32_t at[fx::SL_LAUNCHES] = {};
    bool any_large = false;
    for (int j = 0; j < n; j++) {
        const fxjps_grid_job_t& jb = jobs[j];
        GridBufs& g = d.slots[(size_t)jb.slot];
        const size_t ncell = (size_t)jb.W * (size_t)jb.H;
        // (this context's copy of the slot, as fxjps_refresh_slots judges it: a grid beyond the fused build always builds)
        const bool compare = refresh && g.W == jb.W && g.H == jb.H && ncell <= ((size_t)1 << 18);
        d.h_slot_desc[(size_t)jb.slot] = GridDev{};
        int e = alloc_grid_bufs(h, g, jb.W, jb.H);  // (a slot that has room allocates nothing)
        if (e) return e;
        fx::SlotJobDev& J = T.job[j];
        J = fx::SlotJobDev{};
        J.G = d.h_slot_desc[(size_t)jb.slot] = grid_of(g);
        J.occ = g.occ.p;
        J.raw = d.d_slots_in.p + off[(size_t)j];
        J.W0 = jb.W;
        J.H0 = jb.H;
        J.compare = compare ? 1 : 0;
        if (refresh) h_changed[j] = compare ? 0u : 1u;
        memcpy(d.h_slots_in.p + off[(size_t)j], jb.occ, ncell);
        any_large = !slot_job_blocks(T, j, g, fx::SLOT_COPY_BLOCK, at) || any_large;
    }
    for (int l = 0; l < fx::SL_LAUNCHES; l++) T.first[l][n] = at[l];
    memcpy(d.h_slots_in.p + SLOTS_IN_DESC, d.h_slot_desc.data(), sizeof(GridDev) * FXJPS_MAX_GRID_SLOTS);
    HIPCHK(h, hipMemcpyAsync(d.d_slots_in.p, d.h_slots_in.p, in_bytes, hipMemcpyHostToDevice, d.stream));
    const fx::SlotTable* dT = reinterpret_cast<const fx::SlotTable*>(d.d_slots_in.p);
    using StageFn = void (*)(const fx::SlotTable*, int, const uint32_t*);
    static const StageFn stage[2][4] = {
        {fx::k_slots_stage<fx::SL_BUILD_1, false>, fx::k_slots_stage<fx::SL_BUILD_2, false>, fx::k_slots_stage<fx::SL_BUILD_3, false>, fx::k_slots_stage<fx::SL_JD, false>},
        {fx::k_slots_stage<fx::SL_BUILD_1, true>, fx::k_slots_stage<fx::SL_BUILD_2, true>, fx::k_slots_stage<fx::SL_BUILD_3, true>, fx::k_slots_stage<fx::SL_JD, true>}};
    uint32_t* dC = refresh ? d_changed : nullptr;
    if (tiles)
        hipLaunchKernelGGL(fx::k_slot_tiles_copy, dim3(at[fx::SL_PREPARE]), dim3(256), 0, d.stream, dT, n, dC,
                           reinterpret_cast<unsigned long long*>(d.d_slots_in.p + flags_off + words_bytes));
    else
        hipLaunchKernelGGL(refresh ? fx::k_slots_copy<true> : fx::k_slots_copy<false>, dim3(at[fx::SL_PREPARE]), dim3(256), 0, d.stream, dT, n, dC);
    if (at[fx::SL_BUILD_1] > 0)
        for (int l = fx::SL_BUILD_1; l <= fx::SL_JD; l++)
            hipLaunchKernelGGL(stage[refresh ? 1 : 0][l - fx::SL_BUILD_1], dim3(at[l]), dim3(l == fx::SL_BUILD_3 ? 1024 : 256), 0, d.stream, dT, n,
                               (const uint32_t*)dC);
    HIPCHK(h, hipGetLastError());
    if (any_large)  // (grids beyond the fused build: their maps one by one, as fxjps_set_grid_slot builds them)
        for (int j = 0; j < n; j++)
            if ((long long)jobs[j].W * jobs[j].H > (1ll << 18)) {
                int e = derive_maps(h, d, true, &d.slots[(size_t)jobs[j].slot]);
                if (e) return e;
            }
    HIPCHK(h, hipMemcpyAsync(d.d_slot_desc.p, d.h_slots_in.p + SLOTS_IN_DESC, sizeof(GridDev) * FXJPS_MAX_GRID_SLOTS, hipMemcpyHostToDevice, d.stream));
    if (refresh)
        HIPCHK(h, hipMemcpyAsync(d.h_slots_res.p, d_changed, tiles ? words_bytes + rec_bytes : (size_t)n * sizeof(uint32_t), hipMemcpyDeviceToHost, d.stream));
    HIPCHK(h, hipStreamSynchronize(d.stream));
    return FXJPS_OK;
}

// fxjps_set_grid_slots (refresh false) and fxjps_refresh_grid_slots: the checks, the call on every context and the
// generations are the same code.
int grid_slots_call(fxjps_t* h, const fxjps_grid_job_t* jobs, int32_t n, bool refresh, int32_t* out_kept, const char* what) {
    if (int rc = jobs_call_check(h, jobs, n, what)) return rc;
    if (refresh && n > 0 && !out_kept) return fail(h, FXJPS_E_ARG, "job 0: NULL out_kept");
    // everything the host can judge, for every job, before anything is queued or any slot is touched
    std::vector<size_t> off((size_t)n);
    std::vector<int> named(FXJPS_MAX_GRID_SLOTS, -1);
    size_t in_bytes = SLOTS_IN_RAWS;
    for (int j = 0; j < n; j++) {
        const fxjps_grid_job_t& jb = jobs[j];
        if (jb.slot < 0 || jb.slot >= FXJPS_MAX_GRID_SLOTS) return fail(h, FXJPS_E_ARG, "job %d: slot %d is not in 0 .. %d", j, (int)jb.slot, FXJPS_MAX_GRID_SLOTS - 1);
        if (named[(size_t)jb.slot] >= 0) return fail(h, FXJPS_E_ARG, "job %d: slot %d is already named by job %d", j, (int)jb.slot, named[(size_t)jb.slot]);
        named[(size_t)jb.slot] = j;
        if (!jb.occ) return fail(h, FXJPS_E_ARG, "job %d: NULL occ (fxjps_set_grid_slot releases a slot)", j);
        if (jb.W < 1 || jb.H < 1 || jb.W > 8190 || jb.H > 8190) return fail(h, FXJPS_E_ARG, "job %d: grid %dx%d must be 1..8190 cells a side", j, (int)jb.W, (int)jb.H);
        if (jb.reserved != 0) return fail(h, FXJPS_E_ARG, "job %d: reserved is %d, not 0", j, (int)jb.reserved);
        off[(size_t)j] = in_bytes;
        in_bytes += ((size_t)jb.W * (size_t)jb.H + 15) & ~(size_t)15;
    }
    if (n == 0) return FXJPS_OK;
    const bool tiles = refresh && h->slot_reuse == 1;
    int rc = run_side_by_side(h->devs.size(), [&](size_t r) -> int { return grid_slots_on(h, h->devs[r], jobs, n, off, in_bytes, refresh, tiles); });
    if (rc) {
        drain_all(h);
        for (int j = 0; j < n; j++) {  // (slots of a call that failed on one context are released on all of them)
            release_slot_everywhere(h, jobs[j].slot);
            h->bump_slot(jobs[j].slot);
        }
        (void)hipGetLastError();
        return rc;
    }
    const int32_t* words = h->devs[0].h_slots_res.p;
    for (int j = 0; j < n; j++) {
        const bool kept = refresh && words[j] == 0;  // (no byte of context 0's copy differed: nothing was built)
        if (out_kept) out_kept[j] = kept ? 1 : 0;
        if (kept) continue;
        if (tiles && job_compared(h->devs[0], j))  // (as fxjps_refresh_slots: a compared job's marks join the slot's record)
            h->mark_slot(jobs[j].slot, slot_tile_records(h->devs[0]) + (size_t)j * 128);
        else
            h->bump_slot(jobs[j].slot);
    }
    return FXJPS_OK;
}
}  // namespace

int fxjps_set_grid_slots(fxjps_t* h, const fxjps_grid_job_t* jobs, int32_t n) { return grid_slots_call(h, jobs, n, false, nullptr, "fxjps_set_grid_slots"); }

int fxjps_refresh_grid_slots(fxjps_t* h, const fxjps_grid_job_t* jobs, int32_t n, int32_t* out_kept) {
    return grid_slots_call(h, jobs, n, true, out_kept, "fxjps_refresh_grid_slots");
}

// ------------------------------------------------------------------ the same two calls from world-frame jobs
int fxjps_world_job_size(void) { return (int)sizeof(fxjps_world_job_t); }

int fxjps_set_prior_map(fxjps_t* h, int32_t prior, const uint8_t* occ, int32_t W, int32_t H) {
    if (!h) return FXJPS_E_ARG;
    if (prior < 0 || prior >= FXJPS_MAX_PRIOR_MAPS) return fail(h, FXJPS_E_ARG, "prior %d is not in 0 .. %d", (int)prior, FXJPS_MAX_PRIOR_MAPS - 1);
    if (occ && (W < 1 || H < 1 || W > 8190 || H > 8190)) return fail(h, FXJPS_E_ARG, "a prior map must be 1..8190 cells a side");
    if (int rr = refuse_on_rank_handle(h, "fxjps_set_prior_map")) return rr;
    // every context gets its own copy from the host, as a slot does; no slot, generation or stored result is touched
    int rc = run_side_by_side(h->devs.size(), [&](size_t r) -> int {
        DevCtx& d = h->devs[r];
        HIPCHK(h, hipSetDevice(d.dev));
        if (d.priors.empty()) d.priors.resize(FXJPS_MAX_PRIOR_MAPS);
        DevCtx::PriorBuf& pr = d.priors[(size_t)prior];
        HIPCHK(h, hipStreamSynchronize(d.stream));  // (whatever is queued may still read the prior's bytes)
        pr.W = pr.H = 0;
        pr.next.release();  // (a grown prior's spare buffer goes with it)
        if (!occ) {
            pr.occ.release();
            return FXJPS_OK;
        }
        HIPCHK(h, pr.occ.ensure((size_t)W * H));
        HIPCHK(h, hipMemcpyAsync(pr.occ.p, occ, (size_t)W * H, hipMemcpyHostToDevice, d.stream));
        HIPCHK(h, hipStreamSynchronize(d.stream));
        pr.W = W;
        pr.H = H;
        return FXJPS_OK;
    });
    if (rc) {
        drain_all(h);
        for (auto& d : h->devs)  // (a prior that failed on one context is released on all of them)
            if ((size_t)prior < d.priors.size()) {
                if (hipSetDevice(d.dev) == hipSuccess) d.priors[(size_t)prior].occ.release();
                d.priors[(size_t)prior].W = d.priors[(size_t)prior].H = 0;
            }
        (void)hipGetLastError();
    }
    return rc;
}

int fxjps_get_prior_map(fxjps_t* h, int32_t prior, uint8_t* out, int32_t* W, int32_t* H) {
    if (!h) return FXJPS_E_ARG;
    DevCtx& d = h->devs[0];
    if (prior < 0 || prior >= FXJPS_MAX_PRIOR_MAPS || (size_t)prior >= d.priors.size() || d.priors[(size_t)prior].W <= 0)
        return fail(h, FXJPS_E_ARG, "prior %d is not set or out of range", (int)prior);
    const DevCtx::PriorBuf& pr = d.priors[(size_t)prior];
    if (W) *W = pr.W;
    if (H) *H = pr.H;
    if (out) {
        HIPCHK(h, hipSetDevice(d.dev));
        HIPCHK(h, hipMemcpyAsync(out, pr.occ.p, (size_t)pr.W * pr.H, hipMemcpyDeviceToHost, d.stream));
        HIPCHK(h, hipStreamSynchronize(d.stream));
    }
    return FXJPS_OK;
}

namespace {
// numpy's .astype(int) / Python's int() of a float64 quotient, for quotients whose truncation is an int32
bool trunc_i32(double q, long long& out) {
    if (!(q > -2147483649.0 && q < 2147483648.0)) return false;  // (NaN fails both)
    out = (long long)q;
    return true;
}

// The eleven output fields of a world job: from another job (the slot job's results, a cropped call's second phase) ...
void copy_world_outputs(fxjps_world_job_t& to, const fxjps_world_job_t& from) {
    for (int k = 0; k < 2; k++) {
        to.canvas_o[k] = from.canvas_o[k];
        to.origin[k] = from.origin[k];
        to.start_xy[k] = from.start_xy[k];
        to.goal_xy_cell[k] = from.goal_xy_cell[k];
        to.map_d[k] = from.map_d[k];
    }
    to.W = from.W;
    to.H = from.H;
    to.end_occu = from.end_occu;
    to.status = from.status;
    to.canvas_W = from.canvas_W;
    to.canvas_H = from.canvas_H;
}
// ... and of a job that took no part: all zero but its status
void clear_world_outputs(fxjps_world_job_t& wj, int status) {
    fxjps_world_job_t none{};
    none.status = status;
    copy_world_outputs(wj, none);
}

// The conversion in front of slots_call: the reference's lines between the map callback and the preparation
// (global_planner_st.py:210-227 / global_planner_ccst.py:395-412), in float64 with the reference's operations in the
// reference's order (the library is built with -ffp-contract=off).  Each world job becomes the fxjps_slot_job_t whose raw is
// the canvas -- which only the gather ever sees, through WorldSrc -- and slots_call does the rest.
int world_call(fxjps_t* h, fxjps_world_job_t* jobs, int32_t n, bool refresh, int32_t* out_kept, const char* what, const size_t* staged_raw = nullptr) {
    if (int rc = jobs_call_check(h, jobs, n, what)) return rc;
    std::vector<fxjps_slot_job_t> sj((size_t)n);
    std::vector<WorldSrc> src((size_t)n);
    std::vector<double> co((size_t)n * 2);
    const DevCtx& d0 = h->devs[0];
    for (int j = 0; j < n; j++) {
        const fxjps_world_job_t& wj = jobs[j];
        if (!wj.raw) return fail(h, FXJPS_E_ARG, "job %d: NULL raw", j);
        if (wj.W0 < 1 || wj.H0 < 1 || wj.W0 > 8190 || wj.H0 > 8190)
            return fail(h, FXJPS_E_ARG, "job %d: bad arguments (W0 %d, H0 %d): the detected map must be 1..8190 cells a side", j, (int)wj.W0, (int)wj.H0);
        if (wj.prior < -1 || wj.prior >= FXJPS_MAX_PRIOR_MAPS)
            return fail(h, FXJPS_E_ARG, "job %d: prior %d is not in -1 .. %d", j, (int)wj.prior, FXJPS_MAX_PRIOR_MAPS - 1);
        const bool with_prior = wj.prior >= 0;
        if (with_prior && ((size_t)wj.prior >= d0.priors.size() || d0.priors[(size_t)wj.prior].W <= 0))
            return fail(h, FXJPS_E_ARG, "job %d: prior %d is not set", j, (int)wj.prior);
        const double reso = wj.map_reso;
        if (!std::isfinite(reso) || !(reso > 0.0)) return fail(h, FXJPS_E_ARG, "job %d: map_reso %g must be finite and > 0", j, reso);
        for (int k = 0; k < 2; k++)
            if (!std::isfinite(wj.map_o[k]) || !std::isfinite(wj.pos_xy[k]) || !std::isfinite(wj.goal_xy[k]) ||
                (with_prior && (!std::isfinite(wj.map_t[k]) || !std::isfinite(wj.ori_pre[k]))))
                return fail(h, FXJPS_E_ARG, "job %d: a non-finite map_o / map_t / pos_xy / goal_xy / ori_pre", j);
        WorldSrc& w = src[(size_t)j];
        w = WorldSrc{wj.prior, wj.W0, wj.H0, 0, 0, 0, 0};
        long long canvas[2] = {wj.W0, wj.H0};
        double* o = &co[(size_t)j * 2];
        o[0] = wj.map_o[0];
        o[1] = wj.map_o[1];
        if (with_prior) {
            const DevCtx::PriorBuf& pr = d0.priors[(size_t)wj.prior];
            const long long l[2] = {pr.W, pr.H}, rl[2] = {wj.W0, wj.H0};
            long long rpos[2], ppos[2];
            for (int k = 0; k < 2; k++) {
                const double t_pre = wj.ori_pre[k] + reso * (double)l[k];          // st:187
                o[k] = std::min(wj.map_o[k], wj.ori_pre[k]);                       // st:212 (the first of two equal ones, as min())
                const double top = std::max(t_pre, wj.map_t[k]);                   // st:215-216 (likewise)
                if (!trunc_i32((wj.map_o[k] - o[k]) / reso, rpos[k]) || !trunc_i32((wj.ori_pre[k] - o[k]) / reso, ppos[k]) ||
                    !trunc_i32((top - o[k]) / reso, canvas[k]))
                    return fail(h, FXJPS_E_ARG, "job %d: a placement index or a canvas extent is outside int32", j);
                // the reference's slice assignment raises here (st:219-220); where a side of 1 clipped to 0 would broadcast,
                // the library refuses all the same
                if (canvas[k] < 1 || rpos[k] < 0 || ppos[k] < 0 || rpos[k] + rl[k] > canvas[k] || ppos[k] + l[k] > canvas[k])
                    return fail(h, FXJPS_E_ARG, "job %d: axis %d: the detected map (%lld + %lld) or the prior (%lld + %lld) sticks out of the canvas of %lld cells",
                                j, k, rpos[k], rl[k], ppos[k], l[k], canvas[k]);
            }
            w.rx = (int)rpos[0];
            w.ry = (int)rpos[1];
            w.px = (int)ppos[0];
            w.py = (int)ppos[1];
        }
        long long sc[2], gc[2];
        for (int k = 0; k < 2; k++)  // st:226-227
            if (!trunc_i32((wj.goal_xy[k] - o[k]) / reso, gc[k]) || !trunc_i32((wj.pos_xy[k] - o[k]) / reso, sc[k]))
                return fail(h, FXJPS_E_ARG, "job %d: a start or goal cell is outside int32", j);
        fxjps_slot_job_t& s = sj[(size_t)j];
        s = fxjps_slot_job_t{};
        s.raw = wj.raw;
        s.slot = wj.slot;
        s.layout = wj.layout;
        s.W0 = (int32_t)canvas[0];
        s.H0 = (int32_t)canvas[1];
        s.ifa = wj.ifa;
        s.variant = wj.variant;
        s.start_xy[0] = (int32_t)sc[0];
        s.start_xy[1] = (int32_t)sc[1];
        s.goal_xy[0] = (int32_t)gc[0];
        s.goal_xy[1] = (int32_t)gc[1];
    }
    int rc = slots_call(h, sj.data(), n, refresh, out_kept, what, src.data(), staged_raw);
    if (rc) return rc;
    for (int j = 0; j < n; j++) {
        fxjps_world_job_t& wj = jobs[j];
        const fxjps_slot_job_t& s = sj[(size_t)j];
        fxjps_world_job_t o{};
        for (int k = 0; k < 2; k++) {
            o.start_xy[k] = s.start_xy[k];
            o.goal_xy_cell[k] = s.goal_xy[k];
            o.map_d[k] = s.map_d[k];
            o.canvas_o[k] = co[(size_t)j * 2 + k];
            o.origin[k] = (double)(-(long long)s.map_d[k]) * wj.map_reso + o.canvas_o[k];  // st:236: map_o2 * map_reso + map_o
        }
        o.W = s.W;
        o.H = s.H;
        o.end_occu = s.end_occu;
        o.status = s.status;
        o.canvas_W = s.W0;
        o.canvas_H = s.H0;
        copy_world_outputs(wj, o);
    }
    return FXJPS_OK;
}
}  // namespace

int fxjps_prepare_slots_world(fxjps_t* h, fxjps_world_job_t* jobs, int32_t n) { return world_call(h, jobs, n, false, nullptr, "fxjps_prepare_slots_world"); }

int fxjps_refresh_slots_world(fxjps_t* h, fxjps_world_job_t* jobs, int32_t n, int32_t* out_kept) {
    return world_call(h, jobs, n, true, out_kept, "fxjps_refresh_slots_world");
}

// ------------------------------------------------------------------ ... with the ccst node's crop in front
int fxjps_crop_size(void) { return (int)sizeof(fxjps_crop_t); }

namespace {
// The staged input of a cropped call's first phase: the job table, n box records, then the messages.
constexpr size_t CROP_IN_BOX = (sizeof(fx::CropTable) + 15) & ~(size_t)15;
constexpr size_t CROP_IN_RAWS = CROP_IN_BOX + sizeof(int32_t) * 4 * FXJPS_MAX_GRID_SLOTS;
static_assert(CROP_IN_RAWS % 16 == 0, "the messages are read with 16-byte loads");

// One context's first phase: ONE copy in, the two crop launches, ONE copy out, ONE wait.  The boxes are left in
// d.h_crop_box, the windows in d.d_crop_win at the offsets of the messages (a window is never larger than its message).
int crop_phase_on(fxjps* h, DevCtx& d, const fxjps_world_job_t* jobs, int n, const std::vector<size_t>& off, size_t raw_bytes,
                  const std::vector<long long>& start0) {
    HIPCHK(h, hipSetDevice(d.dev));
    // (no host wait in front: every call that reads the window buffer has returned)
    HIPCHK(h, d.h_crop_in.ensure(CROP_IN_RAWS + raw_bytes));
    HIPCHK(h, d.d_crop_in.ensure(CROP_IN_RAWS + raw_bytes));
    HIPCHK(h, d.d_crop_win.ensure(raw_bytes));
    HIPCHK(h, d.h_crop_box.ensure((size_t)n * 4));
    fx::CropTable& T = *reinterpret_cast<fx::CropTable*>(d.h_crop_in.p);
    int32_t* h_box = reinterpret_cast<int32_t*>(d.h_crop_in.p + CROP_IN_BOX);
    int32_t* d_box = reinterpret_cast<int32_t*>(d.d_crop_in.p + CROP_IN_BOX);
    uint32_t at = 0;
    for (int j = 0; j < n; j++) {
        const fxjps_world_job_t& wj = jobs[j];
        const size_t cells = (size_t)wj.W0 * (size_t)wj.H0;
        fx::CropJobDev& J = T.job[j];
        J.raw = d.d_crop_in.p + CROP_IN_RAWS + off[(size_t)j];
        J.win = d.d_crop_win.p + off[(size_t)j];
        J.W0 = wj.W0;
        J.H0 = wj.H0;
        J.layout = wj.layout;
        J.ifa = wj.ifa;
        J.s0x = (int32_t)start0[(size_t)j * 2];
        J.s0y = (int32_t)start0[(size_t)j * 2 + 1];
        h_box[4 * j + 0] = h_box[4 * j + 1] = INT32_MAX;
        h_box[4 * j + 2] = h_box[4 * j + 3] = -1;
        memcpy(d.h_crop_in.p + CROP_IN_RAWS + off[(size_t)j], wj.raw, cells);
        T.first[j] = at;
        at += (uint32_t)((cells + fx::CROP_BLOCK_BYTES - 1) / fx::CROP_BLOCK_BYTES);
    }
    T.first[n] = at;
    HIPCHK(h, hipMemcpyAsync(d.d_crop_in.p, d.h_crop_in.p, CROP_IN_RAWS + raw_bytes, hipMemcpyHostToDevice, d.stream));
    const fx::CropTable* dT = reinterpret_cast<const fx::CropTable*>(d.d_crop_in.p);
    hipLaunchKernelGGL(fx::k_crop_bounds, dim3(at), dim3(256), 0, d.stream, dT, d_box, n);
    hipLaunchKernelGGL(fx::k_crop_window, dim3(at), dim3(256), 0, d.stream, dT, (const int32_t*)d_box, n);
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipMemcpyAsync(d.h_crop_box.p, d_box, (size_t)n * 4 * sizeof(int32_t), hipMemcpyDeviceToHost, d.stream));
    HIPCHK(h, hipStreamSynchronize(d.stream));
    return FXJPS_OK;
}

// The slots of the jobs that took no part are left empty on every context (their buffers keep their room): one copy of the
// descriptor table per context, whatever their number.
int empty_slots_everywhere(fxjps* h, const std::vector<int32_t>& slots) {
    return run_side_by_side(h->devs.size(), [&](size_t r) -> int {
        DevCtx& d = h->devs[r];
        HIPCHK(h, hipSetDevice(d.dev));
        if (int e = ensure_slot_tables(h, d)) return e;
        for (int32_t s : slots) {
            d.slots[(size_t)s].W = d.slots[(size_t)s].H = 0;
            d.h_slot_desc[(size_t)s] = GridDev{};
        }
        HIPCHK(h, hipMemcpy(d.d_slot_desc.p, d.h_slot_desc.data(), sizeof(GridDev) * FXJPS_MAX_GRID_SLOTS, hipMemcpyHostToDevice));
        return FXJPS_OK;
    });
}

// fxjps_prepare_slots_cropped / fxjps_refresh_slots_cropped: remove_zero_rowscols (global_planner_ccst.py:36-63) in front of
// world_call.  The box of every message is found on the device (first phase); the float64 arithmetic of ccst:47-54 and the
// per-job outcome are the host's; the jobs that go on are handed to world_call with their windows where the first phase
// left them.
int crop_call(fxjps_t* h, fxjps_world_job_t* jobs, int32_t n, bool refresh, int32_t* out_kept, fxjps_crop_t* out_crop, const char* what) {
    if (int rc = jobs_call_check(h, jobs, n, what)) return rc;
    if (n == 0) return FXJPS_OK;
    // what can be judged without the box, for every job, before anything is queued
    std::vector<int> named(FXJPS_MAX_GRID_SLOTS, -1);
    std::vector<size_t> off((size_t)n);
    std::vector<long long> start0((size_t)n * 2);
    size_t raw_bytes = 0;
    const DevCtx& d0 = h->devs[0];
    for (int j = 0; j < n; j++) {
        const fxjps_world_job_t& wj = jobs[j];
        if (wj.slot < 0 || wj.slot >= FXJPS_MAX_GRID_SLOTS) return fail(h, FXJPS_E_ARG, "job %d: slot %d is not in 0 .. %d", j, (int)wj.slot, FXJPS_MAX_GRID_SLOTS - 1);
        if (named[(size_t)wj.slot] >= 0) return fail(h, FXJPS_E_ARG, "job %d: slot %d is already named by job %d", j, (int)wj.slot, named[(size_t)wj.slot]);
        named[(size_t)wj.slot] = j;
        if (!wj.raw) return fail(h, FXJPS_E_ARG, "job %d: NULL raw", j);
        if (wj.W0 < 1 || wj.H0 < 1 || wj.W0 > 8190 || wj.H0 > 8190 || wj.ifa < 0 || wj.ifa > 64 || (wj.variant != 0 && wj.variant != 1) ||
            (wj.layout != 0 && wj.layout != 1))
            return fail(h, FXJPS_E_ARG, "job %d: bad arguments (W0 %d, H0 %d, ifa %d, variant %d, layout %d): the message must be 1..8190 cells a side", j,
                        (int)wj.W0, (int)wj.H0, (int)wj.ifa, (int)wj.variant, (int)wj.layout);
        if (wj.prior < -1 || wj.prior >= FXJPS_MAX_PRIOR_MAPS)
            return fail(h, FXJPS_E_ARG, "job %d: prior %d is not in -1 .. %d", j, (int)wj.prior, FXJPS_MAX_PRIOR_MAPS - 1);
        if (wj.prior >= 0 && ((size_t)wj.prior >= d0.priors.size() || d0.priors[(size_t)wj.prior].W <= 0))
            return fail(h, FXJPS_E_ARG, "job %d: prior %d is not set", j, (int)wj.prior);
        const double reso = wj.map_reso;
        if (!std::isfinite(reso) || !(reso > 0.0)) return fail(h, FXJPS_E_ARG, "job %d: map_reso %g must be finite and > 0", j, reso);
        for (int k = 0; k < 2; k++) {
            if (!std::isfinite(wj.map_o[k]) || !std::isfinite(wj.pos_xy[k]) || !std::isfinite(wj.goal_xy[k]) || (wj.prior >= 0 && !std::isfinite(wj.ori_pre[k])))
                return fail(h, FXJPS_E_ARG, "job %d: a non-finite map_o / pos_xy / goal_xy / ori_pre", j);
            if (!trunc_i32((wj.pos_xy[k] - wj.map_o[k]) / reso, start0[(size_t)j * 2 + k]))  // ccst:47
                return fail(h, FXJPS_E_ARG, "job %d: the vehicle's cell in the message is outside int32", j);
        }
        off[(size_t)j] = raw_bytes;
        raw_bytes += ((size_t)wj.W0 * (size_t)wj.H0 + 15) & ~(size_t)15;
    }
    // first phase, on every context from the caller's messages (host copies, no collective); no slot is touched
    int rc = run_side_by_side(h->devs.size(), [&](size_t r) -> int { return crop_phase_on(h, h->devs[r], jobs, n, off, raw_bytes, start0); });
    if (rc) {
        drain_all(h);
        (void)hipGetLastError();
        return rc;
    }
    // ccst:47-54 and the outcome of every job, from context 0's boxes (every context computed the same)
    const int32_t* box = d0.h_crop_box.p;
    std::vector<fxjps_crop_t> crop((size_t)n);
    std::vector<int> outcome((size_t)n);
    std::vector<fxjps_world_job_t> go;
    std::vector<size_t> go_off;
    std::vector<int> go_job;
    std::vector<int32_t> empty;
    const auto sat32 = [](long long v) { return (int32_t)std::min<long long>(std::max<long long>(v, INT32_MIN), INT32_MAX); };
    for (int j = 0; j < n; j++) {
        const fxjps_world_job_t& wj = jobs[j];
        fxjps_crop_t& c = crop[(size_t)j];
        c = fxjps_crop_t{};
        const bool none = box[4 * j + 2] < 0;
        long long lo[2] = {0, 0}, win[2] = {0, 0};
        for (int k = 0; k < 4; k++) c.bbox[k] = box[4 * j + k];
        for (int k = 0; k < 2; k++) {
            const long long s0 = start0[(size_t)j * 2 + k];
            c.start0[k] = (int32_t)s0;
            if (!none) {
                lo[k] = std::min<long long>(c.bbox[k], s0);
                win[k] = (long long)c.bbox[2 + k] - lo[k];
            }
            c.lo[k] = (int32_t)lo[k];
            c.win[k] = sat32(win[k]);
            c.map_o[k] = (double)lo[k] * wj.map_reso + wj.map_o[k];       // ccst:52
            c.map_t[k] = c.map_o[k] + (double)win[k] * wj.map_reso;       // ccst:54
        }
        int& oc = outcome[(size_t)j];
        if (none || wj.W0 <= 2 * wj.ifa || win[0] == 0 || win[1] == 0)  // (win >= 0: the product is <= 0 iff one of them is 0)
            oc = FXJPS_JOB_NOT_PLANNED;
        else if (lo[0] < 0 || lo[1] < 0)
            oc = FXJPS_E_ARG;
        else
            oc = FXJPS_OK;
        if (oc != FXJPS_OK) {
            empty.push_back(wj.slot);
            continue;
        }
        fxjps_world_job_t g = wj;
        g.W0 = c.win[0];
        g.H0 = c.win[1];
        for (int k = 0; k < 2; k++) {
            g.map_o[k] = c.map_o[k];
            g.map_t[k] = c.map_t[k];
        }
        go.push_back(g);
        go_off.push_back(off[(size_t)j]);
        go_job.push_back(j);
    }
    // second phase: what needs the box is judged in there, before anything more is queued or any slot is touched
    std::vector<int32_t> go_kept(go.size() + 1, 0);
    rc = world_call(h, go.data(), (int32_t)go.size(), refresh, refresh ? go_kept.data() : nullptr, what, go_off.data());
    if (rc) return rc;
    if (!empty.empty()) {
        rc = empty_slots_everywhere(h, empty);
        for (int32_t s : empty) h->bump_slot(s);
        if (rc) {
            for (int32_t s : empty) release_slot_everywhere(h, s);
            (void)hipGetLastError();
            return rc;
        }
    }
    for (int j = 0; j < n; j++) {
        if (outcome[(size_t)j] == FXJPS_OK) continue;
        clear_world_outputs(jobs[j], outcome[(size_t)j]);
        if (out_kept) out_kept[j] = 0;
    }
    for (size_t i = 0; i < go.size(); i++) {
        copy_world_outputs(jobs[go_job[i]], go[i]);
        if (out_kept) out_kept[go_job[i]] = go_kept[i];
    }
    if (out_crop) memcpy(out_crop, crop.data(), sizeof(fxjps_crop_t) * (size_t)n);
    return FXJPS_OK;
}
}  // namespace

int fxjps_prepare_slots_cropped(fxjps_t* h, fxjps_world_job_t* jobs, int32_t n, fxjps_crop_t* out_crop) {
    return crop_call(h, jobs, n, false, nullptr, out_crop, "fxjps_prepare_slots_cropped");
}

int fxjps_refresh_slots_cropped(fxjps_t* h, fxjps_world_job_t* jobs, int32_t n, int32_t* out_kept, fxjps_crop_t* out_crop) {
    return crop_call(h, jobs, n, true, out_kept, out_crop, "fxjps_refresh_slots_cropped");
}

// ------------------------------------------------------------------ many slots' maps published, one call
int fxjps_slot_publish_size(void) { return (int)sizeof(fxjps_slot_publish_t); }

int fxjps_publish_slots(fxjps_t* h, fxjps_slot_publish_t* jobs, int32_t n) {
    if (int rc = jobs_call_check(h, jobs, n, "fxjps_publish_slots")) return rc;
    // everything the host can judge, for every job, before anything is queued or written
    constexpr size_t OUT_MAX = (size_t)1 << 30;
    const auto up16 = [](size_t v) { return (v + 15) & ~(size_t)15; };
    size_t out_bytes = 0;
    for (int j = 0; j < n; j++) {
        const fxjps_slot_publish_t& jb = jobs[j];
        if (!slot_in_use(h, jb.slot)) return fail(h, FXJPS_E_ARG, "job %d: grid slot %d is empty or out of range", j, (int)jb.slot);
        if (jb.image && jb.channels != 1 && jb.channels != 3) return fail(h, FXJPS_E_ARG, "job %d: channels = %d, must be 1 (L) or 3 (RGB)", j, (int)jb.channels);
        const GridBufs& g = h->devs[0].slots[(size_t)jb.slot];
        const size_t cells = (size_t)g.W * (size_t)g.H;  // (at most 8190^2: no overflow below)
        if (jb.msg_data) out_bytes += up16(cells);
        if (jb.image) out_bytes += up16(cells * (size_t)jb.channels);
        if (out_bytes > OUT_MAX) return fail(h, FXJPS_E_ARG, "job %d: the call's outputs exceed 2^30 bytes", j);
    }
    DevCtx& d = h->devs[0];
    for (int j = 0; j < n; j++) {
        const GridBufs& g = d.slots[(size_t)jobs[j].slot];
        jobs[j].W = g.W;
        jobs[j].H = g.H;
    }
    if (out_bytes == 0) return FXJPS_OK;  // (extents only)
    HIPCHK(h, hipSetDevice(d.dev));
    // (no host wait in front: every earlier call of this one has waited for its copy out of these buffers)
    const size_t in_bytes = offsetof(fx::PubTable, job) + (size_t)n * sizeof(fx::PubJobDev);
    HIPCHK(h, d.h_pub_in.ensure(sizeof(fx::PubTable)));
    HIPCHK(h, d.d_pub_in.ensure(sizeof(fx::PubTable)));
    HIPCHK(h, d.h_pub_out.ensure(out_bytes));
    HIPCHK(h, d.d_pub_out.ensure(out_bytes));
    fx::PubTable& T = *reinterpret_cast<fx::PubTable*>(d.h_pub_in.p);
    uint32_t at = 0;
    size_t off = 0;
    for (int j = 0; j < n; j++) {
        const fxjps_slot_publish_t& jb = jobs[j];
        const GridBufs& g = d.slots[(size_t)jb.slot];
        const size_t cells = (size_t)g.W * (size_t)g.H;
        fx::PubJobDev& J = T.job[j];
        J.occ = g.occ.p;
        J.W = g.W;
        J.H = g.H;
        J.nty = (g.H + 31) / 32;
        J.ch = jb.image ? jb.channels : 1;
        J.msg_off = J.img_off = -1;
        if (jb.msg_data) {
            J.msg_off = (long long)off;
            off += up16(cells);
        }
        if (jb.image) {
            J.img_off = (long long)off;
            off += up16(cells * (size_t)jb.channels);
        }
        T.first[j] = at;
        if (jb.msg_data || jb.image) at += (uint32_t)(((g.W + 31) / 32) * J.nty);  // (at most 2^30 / 2^10 tiles in all)
    }
    T.first[n] = at;
    HIPCHK(h, hipMemcpyAsync(d.d_pub_in.p, d.h_pub_in.p, in_bytes, hipMemcpyHostToDevice, d.stream));
    hipLaunchKernelGGL(fx::k_publish_slots, dim3(at), dim3(256), 0, d.stream, reinterpret_cast<const fx::PubTable*>(d.d_pub_in.p), (int)n, d.d_pub_out.p);
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipMemcpyAsync(d.h_pub_out.p, d.d_pub_out.p, out_bytes, hipMemcpyDeviceToHost, d.stream));
    HIPCHK(h, hipStreamSynchronize(d.stream));
    for (int j = 0; j < n; j++) {
        const fxjps_slot_publish_t& jb = jobs[j];
        const fx::PubJobDev& J = T.job[j];
        const size_t cells = (size_t)J.W * (size_t)J.H;
        if (jb.msg_data) memcpy(jb.msg_data, d.h_pub_out.p + J.msg_off, cells);
        if (jb.image) memcpy(jb.image, d.h_pub_out.p + J.img_off, cells * (size_t)jb.channels);
    }
    return FXJPS_OK;
}

int fxjps_plan_batch_slots_csr(fxjps_t* h, const int32_t* grid_ids, const int32_t* starts_xy, const int32_t* goals_xy, int64_t nq,
                               int32_t hchoice, int32_t max_path_len, int64_t* out_offsets, int32_t* out_cells_xy,
                               int64_t cells_capacity, int32_t* out_len, double* out_cost, double* out_seconds_total) {
    const double t0 = now_s();
    if (!h) return FXJPS_E_ARG;
    if (nq > 0 && (!out_offsets || !out_len || !out_cost)) return fail(h, FXJPS_E_ARG, "NULL output array");
    BatchReq req;
    if (int rc = batch_request(h, true, grid_ids, starts_xy, goals_xy, nq, hchoice, max_path_len, 0, &req)) return rc;
    if (int rc = plan_core(h, req)) return rc;
    h->last.slots_W = req.W;
    h->last.slots_H = req.H;
    h->last.slot_ids.assign(grid_ids, grid_ids + nq);
    return end_call(h, t0, out_seconds_total, emit_csr(h, nq, out_offsets, out_cells_xy, cells_capacity, out_len, out_cost));
}

namespace {
// fxjps_replan_slots on a handle with one context.  The arguments are checked; `searched` lists the
// queries to search, in query order.  Runs them as a sub-batch through run_shard / finish_search, then assembles the full
// batch on the device: one copy in (the source table), one scan launch, one gather launch, the copies out, one wait.
// req.track() (fxjps_set_slot_reuse(1)): the sub-batch runs the tracking instantiation, and its read sets come back among
// the copies out -- one copy, row k the k-th searched query's -- into d.h_qread.
int replan_slots_assemble(fxjps* h, DevCtx& d, const BatchReq& req, const std::vector<int64_t>& searched) {
    HIPCHK(h, hipSetDevice(d.dev));
    const int64_t nq = req.nq, nsub = (int64_t)searched.size();
    // the previous batch's results become the other set: what was `previous` before is written anew
    std::swap(d.d_len, d.p_len);
    std::swap(d.d_cost, d.p_cost);
    std::swap(d.d_offsets, d.p_offsets);
    std::swap(d.d_cells, d.p_cells);
    std::vector<int32_t> sub_len((size_t)nsub);
    d.q0 = 0;
    d.nq = nsub;
    if (nsub > 0) {
        std::vector<int32_t> ids((size_t)nsub), st((size_t)nsub * 2), go((size_t)nsub * 2);
        for (int64_t k = 0; k < nsub; k++) {
            const int64_t q = searched[(size_t)k];
            ids[(size_t)k] = req.grid_ids[q];
            st[(size_t)2 * k] = req.starts[2 * q];
            st[(size_t)2 * k + 1] = req.starts[2 * q + 1];
            go[(size_t)2 * k] = req.goals[2 * q];
            go[(size_t)2 * k + 1] = req.goals[2 * q + 1];
        }
        BatchReq sub = req;  // (the full batch's extents: the scratch is configured as the whole batch would configure it)
        sub.grid_ids = ids.data();
        sub.starts = st.data();
        sub.goals = go.data();
        sub.nq = nsub;
        int rc = run_shard(h, d, sub);
        if (!rc) rc = finish_search(h, d, sub);  // (waits: the pageable arrays above have been read)
        if (rc) return rc;
        memcpy(sub_len.data(), d.h_len.p, (size_t)nsub * sizeof(int32_t));
        std::swap(d.d_len, d.s_len);  // the sub-batch's lengths and costs step aside for the full batch's
        std::swap(d.d_cost, d.s_cost);
    } else {
        d.run = DevCtx::RunStats();
    }
    if (nq == 0) return FXJPS_OK;
    // every length is known to the host (the stored codes; the sub-batch's, which finish_search brought back): the cells'
    // room is sized before anything is queued, and nothing below waits but the last line
    HIPCHK(h, d.h_rs_src.ensure((size_t)nq));
    HIPCHK(h, d.d_rs_src.ensure((size_t)nq));
    long long total = 0;
    {
        int64_t k = 0;
        for (int64_t q = 0; q < nq; q++) {
            const bool s = k < nsub && searched[(size_t)k] == q;
            const int32_t n = s ? sub_len[(size_t)k] : h->rs_len[(size_t)q];
            d.h_rs_src.p[q] = s ? (int32_t)k : -1;
            if (s) k++;
            total += n > 0 ? n : 0;
        }
    }
    HIPCHK(h, d.d_len.ensure((size_t)nq));
    HIPCHK(h, d.d_cost.ensure((size_t)nq));
    HIPCHK(h, d.d_offsets.ensure((size_t)nq + 1));
    HIPCHK(h, d.h_len.ensure((size_t)nq));
    HIPCHK(h, d.h_cost.ensure((size_t)nq));
    HIPCHK(h, d.h_offsets.ensure((size_t)nq + 1));
    HIPCHK(h, d.h_counters.ensure(64));
    if (total > 0) {
        if (int rc = ensure_beside_pool0(h, d, d.d_cells, (size_t)total * 2)) return rc;  // (the search is over: its scratch can go)
        HIPCHK(h, d.h_cells.ensure((size_t)total * 2));
    }
    HIPCHK(h, hipMemcpyAsync(d.d_rs_src.p, d.h_rs_src.p, (size_t)nq * sizeof(int32_t), hipMemcpyHostToDevice, d.stream));
    const fx::ReplanSrc R{d.d_rs_src.p, d.p_len.p, d.p_cost.p, d.p_offsets.p, d.p_cells.p, d.s_len.p, d.s_cost.p, d.d_path.p, req.max_len};
    hipLaunchKernelGGL(fx::k_replan_scan, dim3(1), dim3(1024), 0, d.stream, R, (long long)nq, d.d_len.p, d.d_cost.p, d.d_offsets.p);
    if (total > 0)
        hipLaunchKernelGGL(fx::k_replan_gather, dim3((unsigned)((nq + 3) / 4)), dim3(256), 0, d.stream, R, d.d_len.p, d.d_offsets.p, (long long)nq,
                           d.d_cells.p, total);
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipMemcpyAsync(d.h_len.p, d.d_len.p, (size_t)nq * sizeof(int32_t), hipMemcpyDeviceToHost, d.stream));
    HIPCHK(h, hipMemcpyAsync(d.h_offsets.p, d.d_offsets.p, ((size_t)nq + 1) * sizeof(long long), hipMemcpyDeviceToHost, d.stream));
    HIPCHK(h, hipMemcpyAsync(d.h_cost.p, d.d_cost.p, (size_t)nq * sizeof(double), hipMemcpyDeviceToHost, d.stream));
    if (nsub > 0) HIPCHK(h, hipMemcpyAsync(d.h_counters.p, d.d_counters.p, 64 * sizeof(unsigned long long), hipMemcpyDeviceToHost, d.stream));
    if (total > 0) HIPCHK(h, hipMemcpyAsync(d.h_cells.p, d.d_cells.p, (size_t)total * 2 * sizeof(int32_t), hipMemcpyDeviceToHost, d.stream));
    if (req.track() && nsub > 0) {
        d.h_qread.resize((size_t)nsub * 128);
        HIPCHK(h, hipMemcpyAsync(d.h_qread.data(), d.d_qread.p, (size_t)nsub * 128 * sizeof(unsigned long long), hipMemcpyDeviceToHost, d.stream));
    }
    HIPCHK(h, hipStreamSynchronize(d.stream));
    if (nsub == 0) memset(d.h_counters.p, 0, 64 * sizeof(unsigned long long));  // (nothing was searched)
    d.nq = nq;
    d.cells_on_host = d.csr_on_device = true;
    if (d.h_offsets.p[nq] != total) return fail(h, FXJPS_E_HIP, "the assembled batch has %lld cells, the host counted %lld", (long long)d.h_offsets.p[nq], total);
    hide_internal_codes(d);
    return FXJPS_OK;
}
}  // namespace

int fxjps_replan_slots(fxjps_t* h, const int32_t* grid_ids, const int32_t* starts_xy, const int32_t* goals_xy, int64_t nq, int32_t hchoice,
                       int32_t max_path_len, int64_t* out_offsets, int32_t* out_cells_xy, int64_t cells_capacity, int32_t* out_len,
                       double* out_cost, int32_t* out_reused, double* out_seconds_total) {
    const double t0 = now_s();
    if (!h) return FXJPS_E_ARG;
    if (int rr = refuse_on_rank_handle(h, "fxjps_replan_slots")) return rr;
    if (h->devs.size() > 1) {  // several contexts: a plain slots batch (reuse across shards is not built)
        if (out_reused && nq > 0) memset(out_reused, 0, (size_t)nq * sizeof(int32_t));
        return fxjps_plan_batch_slots_csr(h, grid_ids, starts_xy, goals_xy, nq, hchoice, max_path_len, out_offsets, out_cells_xy, cells_capacity,
                                          out_len, out_cost, out_seconds_total);
    }
    // every refusal of fxjps_plan_batch_slots_csr, before the stored results are touched
    if (nq > 0 && (!out_offsets || !out_len || !out_cost)) return fail(h, FXJPS_E_ARG, "NULL output array");
    // (the tile rule, DESIGN.md section 3.18: every search of the call records its read set)
    const bool tiles = h->slot_reuse == 1;
    BatchReq req;
    if (int rc = batch_request(h, true, grid_ids, starts_xy, goals_xy, nq, hchoice, max_path_len, tiles ? 1 : 0, &req)) return rc;
    // ---- which queries are searched: plain compares of the arguments against the stored ones, before anything is queued
    static const bool allow_reuse = !(getenv("FXJPS_REPLAN_REUSE") && atoi(getenv("FXJPS_REPLAN_REUSE")) == 0);
    const bool stored = allow_reuse && h->rs_valid && h->rs_nq == nq && h->rs_hchoice == hchoice && h->rs_max_len == max_path_len;
    std::vector<int64_t> searched;
    std::vector<uint64_t> gen((size_t)nq);
    std::vector<int32_t> flag((size_t)nq, 0);  // out_reused: 0 searched, 1 the slot did not change, 2 it changed elsewhere
    for (int64_t q = 0; q < nq; q++) {
        const size_t i = (size_t)q;
        gen[i] = h->slot_gen[(size_t)grid_ids[q]];
        const bool same = stored && h->rs_ids[i] == grid_ids[q] && h->rs_len[i] != FXJPS_Q_CAPACITY &&
                          h->rs_starts[2 * i] == starts_xy[2 * q] && h->rs_starts[2 * i + 1] == starts_xy[2 * q + 1] &&
                          h->rs_goals[2 * i] == goals_xy[2 * q] && h->rs_goals[2 * i + 1] == goals_xy[2 * q + 1];
        if (same && h->rs_gen[i] == gen[i]) {
            flag[i] = 1;
        } else if (same && tiles) {
            // the slot's bytes changed, and every change since the stored search went through a compared refresh job: the
            // stored path stands iff no changed cell's box meets a tile the search read (a length <= 0 depends on more
            // than a read set, as in frame_reuse_rule)
            const fxjps::SlotTiles& R = h->slot_tiles[(size_t)grid_ids[q]];
            if (R.valid && R.base == h->rs_gen[i] && h->rs_len[i] > 0 && h->rs_have[i]) {
                const unsigned long long* b = h->rs_read.data() + i * 128;
                unsigned long long hit = 0;
                for (int t = 0; t < 128; t++) hit |= b[t] & R.D[t];
                if (!hit) flag[i] = 2;
            }
        }
        if (flag[i] == 0) searched.push_back(q);
    }
    DevCtx& d = h->devs[0];
    int rc = begin_batch(h, req);  // (a slots batch: nothing is queued, nothing can fail)
    if (!rc) rc = replan_slots_assemble(h, d, req, searched);
    if (rc) {
        drain_all(h);  // before the error leaves the library
        d.nq = 0;      // (the context holds no result)
        return rc;
    }
    collect_timing(h);
    h->timing.reused = nq - (int64_t)searched.size();
    h->last.slots_W = req.W;
    h->last.slots_H = req.H;
    h->last.slot_ids.assign(grid_ids, grid_ids + nq);
    h->rs_ids = h->last.slot_ids;
    h->rs_starts.assign(starts_xy, starts_xy + 2 * nq);
    h->rs_goals.assign(goals_xy, goals_xy + 2 * nq);
    h->rs_len.assign(d.h_len.p, d.h_len.p + nq);
    h->rs_gen.swap(gen);
    h->rs_nq = nq;
    h->rs_hchoice = hchoice;
    h->rs_max_len = max_path_len;
    h->rs_valid = true;
    if (tiles) {
        // the read set of the search that produced each stored result: a searched query's is new (none, all zero, when it
        // ended without a search: a search marks its start and its goal at the least); a reused query keeps its own -- a
        // fresh search would read the same bits.  Every slot's record begins again at the generation just recorded.
        h->rs_read.resize((size_t)nq * 128);
        h->rs_have.resize((size_t)nq);
        for (size_t k = 0; k < searched.size(); k++) {
            const unsigned long long* src = d.h_qread.data() + k * 128;
            unsigned long long any = 0;
            for (int t = 0; t < 128; t++) any |= src[t];
            memcpy(h->rs_read.data() + (size_t)searched[k] * 128, src, 128 * sizeof(unsigned long long));
            h->rs_have[(size_t)searched[k]] = any != 0;
        }
        for (int s2 = 0; s2 < FXJPS_MAX_GRID_SLOTS; s2++) {
            fxjps::SlotTiles& R = h->slot_tiles[(size_t)s2];
            R.valid = true;
            R.base = h->slot_gen[(size_t)s2];
            memset(R.D, 0, sizeof(R.D));
        }
    }
    if (out_reused) memcpy(out_reused, flag.data(), (size_t)nq * sizeof(int32_t));
    return end_call(h, t0, out_seconds_total, emit_csr(h, nq, out_offsets, out_cells_xy, cells_capacity, out_len, out_cost));
}

// ------------------------------------------------------------------ fxjps_replan_slots under the tile rule
int fxjps_set_slot_reuse(fxjps_t* h, int32_t mode) {
    if (!h) return FXJPS_E_ARG;
    if (int rr = refuse_on_rank_handle(h, "fxjps_set_slot_reuse")) return rr;
    if (mode != 0 && mode != 1) return fail(h, FXJPS_E_ARG, "slot reuse mode %d: 0 (the generation rule) or 1 (the tile rule)", (int)mode);
    if (mode == h->slot_reuse) return FXJPS_OK;
    h->slot_reuse = mode;
    h->rs_valid = false;  // (the stored results carry the other mode's bookkeeping)
    h->rs_read.clear();
    h->rs_have.clear();
    for (auto& R : h->slot_tiles) R = fxjps::SlotTiles();
    return FXJPS_OK;
}

int fxjps_debug_slot_tiles(fxjps_t* h, int32_t slot, uint64_t out[128], int32_t* tsh, int32_t* valid) {
    if (!h || !out || !tsh || !valid) return FXJPS_E_ARG;
    if (slot < 0 || slot >= FXJPS_MAX_GRID_SLOTS) return fail(h, FXJPS_E_ARG, "slot %d is not in 0 .. %d", (int)slot, FXJPS_MAX_GRID_SLOTS - 1);
    const fxjps::SlotTiles& R = h->slot_tiles[(size_t)slot];
    static_assert(sizeof(R.D) == 128 * sizeof(uint64_t), "the record is the caller's 128 words");
    memcpy(out, R.D, sizeof(R.D));
    *tsh = slot_in_use(h, slot) ? h->devs[0].slots[(size_t)slot].tsh : 0;
    *valid = R.valid ? 1 : 0;
    return FXJPS_OK;
}

int fxjps_debug_slot_read_sets(fxjps_t* h, uint64_t* out, int64_t nq, int32_t* out_tsh, int32_t* out_have) {
    if (!h || (nq > 0 && (!out || !out_tsh || !out_have))) return FXJPS_E_ARG;
    if (h->slot_reuse != 1 || !h->rs_valid) return fail(h, FXJPS_E_ARG, "no stored read sets: the last batch call was not a fxjps_replan_slots under the tile rule");
    if (nq != h->rs_nq) return fail(h, FXJPS_E_ARG, "the stored results hold %lld queries, not %lld", (long long)h->rs_nq, (long long)nq);
    if (nq > 0) memcpy(out, h->rs_read.data(), (size_t)nq * 128 * sizeof(uint64_t));
    for (int64_t q = 0; q < nq; q++) {
        const int32_t id = h->rs_ids[(size_t)q];
        out_tsh[q] = slot_in_use(h, id) ? h->devs[0].slots[(size_t)id].tsh : 0;
        out_have[q] = h->rs_have[(size_t)q] ? 1 : 0;
    }
    return FXJPS_OK;
}

int fxjps_last_cells(fxjps_t* h, int32_t* out_cells_xy, int64_t cells_capacity) {
    if (!h || !out_cells_xy) return FXJPS_E_ARG;
    int64_t base = 0;
    for (auto& d : h->devs) {
        if (d.nq == 0 || !d.h_offsets.p) continue;
        base += d.h_offsets.p[d.nq];
    }
    if (base > cells_capacity)
        return fail(h, FXJPS_E_ARG, "out_cells_xy holds %lld pairs, the last batch has more", (long long)cells_capacity);
    base = 0;
    struct Put {
        int32_t* dst;
        const DevCtx* d;
    };
    std::vector<Put> puts;  // (several contexts: their slices are copied side by side, as in emit_csr)
    for (auto& d : h->devs) {
        if (d.nq == 0 || !d.h_offsets.p) continue;
        const int64_t total = d.h_offsets.p[d.nq];
        if (total > 0) puts.push_back(Put{out_cells_xy + 2 * base, &d});
        base += total;
    }
    (void)run_side_by_side(puts.size(), [&](size_t i) {
        put_cells(*puts[i].d, puts[i].dst);
        return 0;
    });
    return FXJPS_OK;
}

int fxjps_plan_batch(fxjps_t* h, const int32_t* starts_xy, const int32_t* goals_xy, int64_t nq, int32_t hchoice,
                     int32_t max_path_len, int32_t* out_cells_xy, int32_t* out_len, double* out_cost,
                     double* out_seconds_total) {
    const double t0 = now_s();
    if (!h) return FXJPS_E_ARG;
    if (nq > 0 && (!out_len || !out_cost)) return fail(h, FXJPS_E_ARG, "NULL output array");
    int rc = plan_resident(h, starts_xy, goals_xy, nq, hchoice, max_path_len);
    if (rc) return rc;
    for (auto& d : h->devs) {
        if (d.nq == 0) continue;
        memcpy(out_len + d.q0, d.h_len.p, (size_t)d.nq * sizeof(int32_t));
        memcpy(out_cost + d.q0, d.h_cost.p, (size_t)d.nq * sizeof(double));
        if (!out_cells_xy) continue;
        if ((rc = host_cells(h, d)) != FXJPS_OK) return rc;
        for (int64_t i = 0; i < d.nq; i++) {
            const int32_t n = d.h_len.p[i];
            if (n > 0)
                memcpy(out_cells_xy + (size_t)(d.q0 + i) * max_path_len * 2, d.h_cells.p + 2 * d.h_offsets.p[i], (size_t)n * 2 * sizeof(int32_t));
        }
    }
    return end_call(h, t0, out_seconds_total, FXJPS_OK);
}

int fxjps_set_memory_share(fxjps_t* h, int32_t handles_per_device) {
    if (!h) return FXJPS_E_ARG;
    if (handles_per_device < 1 || handles_per_device > 64) return fail(h, FXJPS_E_ARG, "handles_per_device must be 1..64");
    if (h->mem_div != handles_per_device) {
        h->mem_div = handles_per_device;
        for (auto& d : h->devs) {  // the next batch sizes its pools again -- from nothing: the buffers are grow-only, and
                                   // a pool sized for the whole device would stay, and be credited to this handle's budget
            if (hipSetDevice(d.dev) == hipSuccess) {
                if (d.stream_solo) (void)hipStreamSynchronize(d.stream_solo);
                (void)hipStreamSynchronize(d.stream);
            }
            for (int p = 0; p < 2; p++) {
                d.tables[p].release();
                d.far[p].release();
                d.wave_gen[p].release();
                d.cfg[p] = ScratchCfg();
                d.pool_clean[p] = false;
            }
        }
    }
    return FXJPS_OK;
}

int fxjps_comm_info(fxjps_t* h, int32_t* out_contexts, int32_t* out_devices, int32_t* out_rccl_ranks) {
    if (!h) return FXJPS_E_ARG;
    if (out_contexts) *out_contexts = (int32_t)h->devs.size();
    if (out_devices) {
        int n = 0;
        for (size_t a = 0; a < h->devs.size(); a++) {
            bool first = true;
            for (size_t b = 0; b < a; b++)
                if (h->devs[b].dev == h->devs[a].dev) first = false;
            n += first ? 1 : 0;
        }
        *out_devices = n;
    }
    if (out_rccl_ranks) {
        *out_rccl_ranks = 0;
        if (h->rccl && !h->comms.empty() && h->comms[0]) {
            typedef int (*nccl_count_t)(void*, int*);
            auto count = (nccl_count_t)dlsym(h->rccl, "ncclCommCount");
            int n = 0;
            if (count && count(h->comms[0], &n) == 0) *out_rccl_ranks = n;
        }
    }
    return FXJPS_OK;
}

int fxjps_last_timing_device(fxjps_t* h, int32_t ctx, int32_t* out_device, int64_t* out_nq, double* out_kernel_ms, int64_t* out_waves) {
    if (!h || ctx < 0 || ctx >= (int32_t)h->devs.size()) return FXJPS_E_ARG;
    const DevCtx& d = h->devs[(size_t)ctx];
    if (out_device) *out_device = d.dev;
    if (out_nq) *out_nq = d.nq;
    if (out_kernel_ms) *out_kernel_ms = d.run.kernel_ms;
    if (out_waves) *out_waves = d.run.waves_used;
    return FXJPS_OK;
}

// ------------------------------------------------------------------ waypoint selection over a batch
int fxjps_waypoint_ccst_batch(fxjps_t* h, int64_t nq, const int64_t* offsets, const int32_t* cells_xy, double reso, const double* origin,
                              const double* pos, const double* goal, const int32_t* end_occu, double* out_wp, double* out_goal,
                              int32_t* out_n_kept, int32_t* out_kept_cells, int64_t kept_capacity) {
    if (!h) return FXJPS_E_ARG;
    if (!h->have_grid) return fail(h, FXJPS_E_NOGRID, "fxjps_waypoint_ccst_batch before fxjps_set_grid");
    if (nq < 0 || !origin || (nq > 0 && (!pos || !goal || !out_wp))) return fail(h, FXJPS_E_ARG, "bad waypoint arguments");
    if ((cells_xy != nullptr) != (offsets != nullptr)) return fail(h, FXJPS_E_ARG, "offsets and cells_xy go together");
    if (!cells_xy && nq != h->last.nq) return fail(h, FXJPS_E_ARG, "the last batch had %lld queries, not %lld", (long long)h->last.nq, (long long)nq);
    if (!cells_xy && h->last.slots)  // (the line tests read the resident grid: those paths were planned on other grids)
        return fail(h, FXJPS_E_ARG, "the last batch ran on grid slots: pass its paths explicitly");
    if (h->maps_stale) {  // (the grid is what the line test reads; deferred updates are queued on the same streams anyway)
        int rc = update_cells_async(h, nullptr, nullptr, 0, true);
        if (rc) return rc;
    }
    if (nq == 0) return FXJPS_OK;
    WpPaths S;
    if (int rc = S.resolve(h, nq, offsets, cells_xy, false, [](int64_t) { return true; })) return rc;
    if (out_kept_cells && kept_capacity < S.total)
        return fail(h, FXJPS_E_ARG, "out_kept_cells holds %lld pairs, the paths have %lld", (long long)kept_capacity, (long long)S.total);
    if (int rc = S.upload(h)) return rc;
    const auto queue = [&](WpPaths::Part& P) -> int {
        DevCtx& d = *P.d;
        HIPCHK(h, hipSetDevice(d.dev));
        const size_t n = (size_t)P.n;
        HIPCHK(h, d.wp.d_in.ensure(n * 6));
        HIPCHK(h, d.wp.d_out.ensure(n * 6));
        HIPCHK(h, d.wp.d_eo.ensure(n));
        HIPCHK(h, d.wp.d_nkept.ensure(n));
        HIPCHK(h, d.wp.d_kept.ensure((size_t)std::max<long long>(P.total, 1) * 2));
        HIPCHK(h, hipMemcpyAsync(d.wp.d_in.p, pos + 3 * P.q0, n * 3 * sizeof(double), hipMemcpyHostToDevice, d.stream));
        HIPCHK(h, hipMemcpyAsync(d.wp.d_in.p + n * 3, goal + 3 * P.q0, n * 3 * sizeof(double), hipMemcpyHostToDevice, d.stream));
        if (end_occu) HIPCHK(h, hipMemcpyAsync(d.wp.d_eo.p, end_occu + P.q0, n * sizeof(int32_t), hipMemcpyHostToDevice, d.stream));
        fx::WaypointArgs A;
        A.occ = d.occ.p;
        A.W = d.W;
        A.H = d.H;
        A.cells = P.d_cells;
        A.offsets = P.d_off;
        A.len = P.d_len;
        A.nq = (long long)P.n;
        A.reso = reso;
        A.ox = origin[0];
        A.oy = origin[1];
        A.pos = d.wp.d_in.p;
        A.goal = d.wp.d_in.p + n * 3;
        A.end_occu = end_occu ? d.wp.d_eo.p : nullptr;
        A.out_wp = d.wp.d_out.p;
        A.out_goal = d.wp.d_out.p + n * 3;
        A.out_nkept = d.wp.d_nkept.p;
        A.kept = d.wp.d_kept.p;
        hipLaunchKernelGGL(fx::k_waypoint_ccst, dim3((unsigned)((P.n + 3) / 4)), dim3(256), 0, d.stream, A);
        HIPCHK(h, hipGetLastError());
        HIPCHK(h, hipMemcpyAsync(out_wp + 3 * P.q0, d.wp.d_out.p, n * 3 * sizeof(double), hipMemcpyDeviceToHost, d.stream));
        if (out_goal) HIPCHK(h, hipMemcpyAsync(out_goal + 3 * P.q0, d.wp.d_out.p + n * 3, n * 3 * sizeof(double), hipMemcpyDeviceToHost, d.stream));
        if (out_n_kept) HIPCHK(h, hipMemcpyAsync(out_n_kept + P.q0, d.wp.d_nkept.p, n * sizeof(int32_t), hipMemcpyDeviceToHost, d.stream));
        if (out_kept_cells && P.total > 0)
            HIPCHK(h, hipMemcpyAsync(out_kept_cells + 2 * P.kept_at, d.wp.d_kept.p, (size_t)P.total * 2 * sizeof(int32_t), hipMemcpyDeviceToHost, d.stream));
        return FXJPS_OK;
    };
    return wp_queue_then_collect(h, S, queue, [] {});
}

int fxjps_waypoint_st_batch(fxjps_t* h, int64_t nq, const int64_t* offsets, const int32_t* cells_xy, const int32_t* map_start, double reso,
                            const double* origin, const double* pos, const double* goal, const int32_t* end_occu, double dis_wp_tre,
                            double ang_wp_tre, const double* prev_wp, const int32_t* prev_dim, double* out_wp, int32_t* out_dim,
                            double* out_goal, double* out_ang_wp, int32_t nthreads) {
    if (!h) return FXJPS_E_ARG;
    if (nq < 0 || !origin || (nq > 0 && (!map_start || !pos || !goal || !out_wp || !out_dim || !out_goal || !out_ang_wp)))
        return fail(h, FXJPS_E_ARG, "bad waypoint arguments");
    if ((cells_xy != nullptr) != (offsets != nullptr)) return fail(h, FXJPS_E_ARG, "offsets and cells_xy go together");
    if ((prev_wp != nullptr) != (prev_dim != nullptr)) return fail(h, FXJPS_E_ARG, "prev_wp and prev_dim go together");
    if (!cells_xy && nq != h->last.nq) return fail(h, FXJPS_E_ARG, "the last batch had %lld queries, not %lld", (long long)h->last.nq, (long long)nq);
    if (nq == 0) return FXJPS_OK;
    WpPaths S;
    if (int rc = S.resolve(h, nq, offsets, cells_xy, false, [](int64_t) { return false; })) return rc;
    // ---- on the device (round 6): one wavefront per path, the angles out of a table of the HOST's atan2 over the integer
    // pairs this batch can ask for.  The table is filled once per range (threads of this call) and stays on the device.
    const int place = wp_st_place(h, S, nq, nullptr, map_start, nthreads, true);
    if (place < 0) return place;
    if (place == FXJPS_OK) {
        const auto queue = [&](WpPaths::Part& P) -> int {
            DevCtx& d = *P.d;
            HIPCHK(h, hipSetDevice(d.dev));
            const size_t n = (size_t)P.n;
            HIPCHK(h, d.wp.d_in.ensure(n * 6));
            HIPCHK(h, d.wp.d_out.ensure(n * 6));
            HIPCHK(h, d.wp.d_eo.ensure(n));
            HIPCHK(h, d.wp.d_ms.ensure(n * 2));
            HIPCHK(h, d.wp.d_prev.ensure(n * 3));
            HIPCHK(h, d.wp.d_pdim.ensure(n));
            HIPCHK(h, d.wp.d_dim.ensure(n));
            HIPCHK(h, d.wp.d_ang.ensure(n));
            HIPCHK(h, hipMemcpyAsync(d.wp.d_in.p, pos + 3 * P.q0, n * 3 * sizeof(double), hipMemcpyHostToDevice, d.stream));
            HIPCHK(h, hipMemcpyAsync(d.wp.d_in.p + n * 3, goal + 3 * P.q0, n * 3 * sizeof(double), hipMemcpyHostToDevice, d.stream));
            HIPCHK(h, hipMemcpyAsync(d.wp.d_ms.p, map_start + 2 * P.q0, n * 2 * sizeof(int32_t), hipMemcpyHostToDevice, d.stream));
            if (end_occu) HIPCHK(h, hipMemcpyAsync(d.wp.d_eo.p, end_occu + P.q0, n * sizeof(int32_t), hipMemcpyHostToDevice, d.stream));
            if (prev_wp) {
                HIPCHK(h, hipMemcpyAsync(d.wp.d_prev.p, prev_wp + 3 * P.q0, n * 3 * sizeof(double), hipMemcpyHostToDevice, d.stream));
                HIPCHK(h, hipMemcpyAsync(d.wp.d_pdim.p, prev_dim + P.q0, n * sizeof(int32_t), hipMemcpyHostToDevice, d.stream));
            }
            fx::WaypointStArgs A;
            A.cells = P.d_cells;
            A.offsets = P.d_off;
            A.len = P.d_len;
            A.nq = (long long)P.n;
            A.map_start = d.wp.d_ms.p;
            A.reso = reso;
            A.ox = origin[0];
            A.oy = origin[1];
            A.pos = d.wp.d_in.p;
            A.goal = d.wp.d_in.p + n * 3;
            A.end_occu = end_occu ? d.wp.d_eo.p : nullptr;
            A.dis_wp_tre = dis_wp_tre;
            A.ang_wp_tre = ang_wp_tre;
            A.prev_wp = prev_wp ? d.wp.d_prev.p : nullptr;
            A.prev_dim = prev_wp ? d.wp.d_pdim.p : nullptr;
            A.T = fx::WpAtab{d.wp.d_atab.p, d.wp.atab_a, d.wp.atab_b};
            A.out_wp = d.wp.d_out.p;
            A.out_dim = d.wp.d_dim.p;
            A.out_goal = d.wp.d_out.p + n * 3;
            A.out_ang = d.wp.d_ang.p;
            hipLaunchKernelGGL(fx::k_waypoint_st, dim3((unsigned)((P.n + 3) / 4)), dim3(256), 0, d.stream, A);
            HIPCHK(h, hipGetLastError());
            HIPCHK(h, hipMemcpyAsync(out_wp + 3 * P.q0, d.wp.d_out.p, n * 3 * sizeof(double), hipMemcpyDeviceToHost, d.stream));
            HIPCHK(h, hipMemcpyAsync(out_goal + 3 * P.q0, d.wp.d_out.p + n * 3, n * 3 * sizeof(double), hipMemcpyDeviceToHost, d.stream));
            HIPCHK(h, hipMemcpyAsync(out_dim + P.q0, d.wp.d_dim.p, n * sizeof(int32_t), hipMemcpyDeviceToHost, d.stream));
            HIPCHK(h, hipMemcpyAsync(out_ang_wp + P.q0, d.wp.d_ang.p, n * sizeof(double), hipMemcpyDeviceToHost, d.stream));
            return FXJPS_OK;
        };
        return wp_queue_then_collect(h, S, queue, [] {});
    }
    // ---- on host threads
    const WpStHost A{nullptr, map_start, &reso, origin, false, pos, goal, end_occu, dis_wp_tre, ang_wp_tre, prev_wp, prev_dim,
                     out_wp, out_dim, out_goal, out_ang_wp, nullptr, nullptr};
    if (wp_st_on_host(S, nq, nthreads, A) >= 0) return fail(h, FXJPS_E_ARG, "fxjps_waypoint_st failed on a path");
    return FXJPS_OK;
}

// ------------------------------------------------------------------ both waypoint rules over a grid-slots batch
// Per context ONE copy in (the queries' records, and the caller's paths behind them), ONE launch, ONE copy back and one
// wait, whatever nq is and however many slots the queries name.  The slot of a ccst query is resolved HERE, from the
// context's own slot records (d.slots, the records every other slot call keeps): its record carries the occupancy pointer
// and the extents, so there is no second table on the device that could fall behind fxjps_set_grid_slot /
// fxjps_prepare_slots, and fx::GridDev stays as it is.
//
// fxjps_tick_outputs_slots is the same call with `K` set: the record of a query grows by its home position,
// the result by the Point and the direct path's length, the output buffer by the two world-frame sections, and the launch
// is k_tick_outputs_slots.  With K == nullptr every byte staged, launched and copied is what it was before that call existed.
static int wp_slots_call(fxjps_t* h, const char* fn, const TickIO* K, int64_t nq, const int64_t* offsets, const int32_t* cells_xy,
                         const int32_t* grid_ids, const int32_t* rule, const int32_t* map_start, const double* reso, const double* origin,
                         const double* pos, const double* goal, const int32_t* end_occu, double dis_wp_tre, double ang_wp_tre,
                         const double* prev_wp, const int32_t* prev_dim, double* out_wp, int32_t* out_dim, double* out_goal, double* out_ang_wp,
                         int32_t* out_n_kept, int32_t* out_kept_cells, int64_t kept_capacity, int32_t nthreads) {
    if (!h) return FXJPS_E_ARG;
    if (int rr = refuse_on_rank_handle(h, fn)) return rr;
    if (nq < 0 || (nq > 0 && (!rule || !reso || !origin || !pos || !goal || !out_wp))) return fail(h, FXJPS_E_ARG, "bad waypoint arguments");
    if ((cells_xy != nullptr) != (offsets != nullptr)) return fail(h, FXJPS_E_ARG, "offsets and cells_xy go together");
    if ((prev_wp != nullptr) != (prev_dim != nullptr)) return fail(h, FXJPS_E_ARG, "prev_wp and prev_dim go together");
    const bool resident = !cells_xy;
    if (resident && !h->last.slots) return fail(h, FXJPS_E_ARG, "the last batch did not run on grid slots: pass the paths explicitly");
    if (resident && (nq != h->last.nq || (int64_t)h->last.slot_ids.size() != nq))
        return fail(h, FXJPS_E_ARG, "the last batch had %lld queries, not %lld", (long long)h->last.nq, (long long)nq);
    if (nq == 0) return FXJPS_OK;
    if (K && K->out_point && !K->home_xy) return fail(h, FXJPS_E_ARG, "query 0: out_point needs home_xy");
    // ---- everything the host can judge, for every query, before anything is queued
    const int32_t* ids = grid_ids ? grid_ids : (resident ? h->last.slot_ids.data() : nullptr);
    int64_t n_st = 0;
    for (int64_t q = 0; q < nq; q++) {
        if (rule[q] != 0 && rule[q] != 1) return fail(h, FXJPS_E_ARG, "query %lld: rule %d is neither 0 (st) nor 1 (ccst)", (long long)q, (int)rule[q]);
        if (rule[q] == 0) {
            n_st++;
            continue;
        }
        if (!ids) return fail(h, FXJPS_E_ARG, "query %lld: the ccst rule needs grid_ids with explicit paths", (long long)q);
        if (!slot_in_use(h, ids[q]))
            return fail(h, FXJPS_E_ARG, "query %lld names grid slot %d, which is %s", (long long)q, (int)ids[q],
                        ids[q] < 0 || ids[q] >= FXJPS_MAX_GRID_SLOTS ? "out of range" : "empty");
    }
    if (n_st > 0 && !map_start) return fail(h, FXJPS_E_ARG, "the st rule needs map_start");
    // the paths: the caller's CSR (context 0 takes all of them, inside its staged input), or the last batch's, shard by shard
    WpPaths S;
    if (int rc = S.resolve(h, nq, offsets, cells_xy, true, [&](int64_t q) { return rule[q] == 1; })) return rc;
    // the first query whose range would not fit (query q ends at end(q) [+ 2 (q + 1)])
    const auto first_over = [&](int64_t cap, int64_t per_q) -> int64_t {
        for (auto& P : S.parts)
            for (int64_t i = 0; i < P.n; i++)
                if (P.kept_at + P.h_off[i + 1] + per_q * (P.q0 + i + 1) > cap) return P.q0 + i;
        return -1;
    };
    if (out_kept_cells && kept_capacity < S.total) {
        if (K)
            return fail(h, FXJPS_E_ARG, "query %lld: out_kept_cells holds %lld pairs, the paths have %lld", (long long)first_over(kept_capacity, 0),
                        (long long)kept_capacity, (long long)S.total);
        return fail(h, FXJPS_E_ARG, "out_kept_cells holds %lld pairs, the paths have %lld", (long long)kept_capacity, (long long)S.total);
    }
    if (K) {
        if (K->out_path_xyz && K->path_capacity < S.total)
            return fail(h, FXJPS_E_ARG, "query %lld: out_path_xyz holds %lld triples, the paths have %lld", (long long)first_over(K->path_capacity, 0),
                        (long long)K->path_capacity, (long long)S.total);
        if (K->out_dir_xyz && K->dir_capacity < S.total + 2 * nq)
            return fail(h, FXJPS_E_ARG, "query %lld: out_dir_xyz holds %lld triples, the direct paths need %lld", (long long)first_over(K->dir_capacity, 2),
                        (long long)K->dir_capacity, (long long)(S.total + 2 * nq));
    }
    // ---- the st rule's table of angles, or the rule's host form
    bool st_on_host = false;
    if (n_st > 0) {
        const int place = wp_st_place(h, S, nq, rule, map_start, nthreads, false);
        if (place < 0) return place;
        st_on_host = place != FXJPS_OK;
    }
    // ---- queue every context, then collect
    static_assert(sizeof(fx::WpSlotQuery) % 8 == 0 && sizeof(fx::WpSlotResult) % 8 == 0, "the offsets and cells behind the records stay aligned");
    static_assert(sizeof(fx::TickQuery) % 8 == 0 && sizeof(fx::TickResult) % 8 == 0 && offsetof(fx::TickQuery, s) == 0 && offsetof(fx::TickResult, r) == 0,
                  "a tick record begins with the waypoint record, and the doubles behind the records stay aligned");
    const auto queue = [&](WpPaths::Part& P) -> int {
        DevCtx& d = *P.d;
        HIPCHK(h, hipSetDevice(d.dev));
        const size_t n = (size_t)P.n, tot = (size_t)P.total;
        const size_t rec = K ? sizeof(fx::TickQuery) : sizeof(fx::WpSlotQuery);
        const size_t in_off = n * rec, in_cells = in_off + (n + 1) * sizeof(long long);
        const size_t in_bytes = S.resident ? in_off : in_cells + tot * 2 * sizeof(int32_t);
        // out: the records | (K: path3 triples | direct-path triples |) the kept cells
        const size_t out_path = n * (K ? sizeof(fx::TickResult) : sizeof(fx::WpSlotResult));
        const size_t out_dir = out_path + (K ? tot * 3 * sizeof(double) : 0);
        const size_t out_kept = out_dir + (K ? (tot + 2 * n) * 3 * sizeof(double) : 0);
        const size_t out_bytes = out_kept + std::max<size_t>(tot, 1) * 2 * sizeof(int32_t);
        HIPCHK(h, d.wp.h_recs_in.ensure(in_bytes));
        HIPCHK(h, d.wp.d_recs_in.ensure(in_bytes));
        HIPCHK(h, d.wp.h_recs_out.ensure(out_bytes));
        HIPCHK(h, d.wp.d_recs_out.ensure(out_bytes));
        for (size_t i = 0; i < n; i++) {
            const int64_t q = P.q0 + (int64_t)i;
            fx::WpSlotQuery& r = *reinterpret_cast<fx::WpSlotQuery*>(d.wp.h_recs_in.p + i * rec);  // (a TickQuery begins with one)
            r = fx::WpSlotQuery{};
            if (K) {
                fx::TickQuery& t = *reinterpret_cast<fx::TickQuery*>(d.wp.h_recs_in.p + i * rec);
                t.hx = K->home_xy ? K->home_xy[2 * q] : 0.0;
                t.hy = K->home_xy ? K->home_xy[2 * q + 1] : 0.0;
            }
            r.rule = rule[q];
            if (r.rule == 1) {
                const GridBufs& g = d.slots[(size_t)ids[q]];
                r.occ = g.occ.p;
                r.W = g.W;
                r.H = g.H;
            } else {
                r.msx = map_start[2 * q];
                r.msy = map_start[2 * q + 1];
                if (prev_wp && (prev_dim[q] == 2 || prev_dim[q] == 3)) {
                    r.pdim = prev_dim[q];
                    for (int k = 0; k < 3; k++) r.prev[k] = prev_wp[3 * q + k];
                }
                if (st_on_host) r.rule = 2;  // (not the kernel's: fxjps_waypoint_st below, on host threads)
            }
            r.reso = reso[q];
            r.ox = origin[2 * q];
            r.oy = origin[2 * q + 1];
            r.eo = end_occu ? end_occu[q] : 0;
            for (int k = 0; k < 3; k++) {
                r.pos[k] = pos[3 * q + k];
                r.goal[k] = goal[3 * q + k];
            }
        }
        if (!S.resident) {
            memcpy(d.wp.h_recs_in.p + in_off, P.h_off, (n + 1) * sizeof(long long));
            if (tot > 0) memcpy(d.wp.h_recs_in.p + in_cells, P.h_cells, tot * 2 * sizeof(int32_t));
        }
        HIPCHK(h, hipMemcpyAsync(d.wp.d_recs_in.p, d.wp.h_recs_in.p, in_bytes, hipMemcpyHostToDevice, d.stream));
        size_t back = out_path;  // the copy back ends after the last section the caller asked for
        if (!K) {
            fx::WaypointSlotsArgs A;
            A.in = reinterpret_cast<const fx::WpSlotQuery*>(d.wp.d_recs_in.p);
            A.out = reinterpret_cast<fx::WpSlotResult*>(d.wp.d_recs_out.p);
            A.cells = S.resident ? P.d_cells : reinterpret_cast<const int32_t*>(d.wp.d_recs_in.p + in_cells);
            A.offsets = S.resident ? P.d_off : reinterpret_cast<const long long*>(d.wp.d_recs_in.p + in_off);
            A.len = S.resident ? P.d_len : nullptr;
            A.kept = reinterpret_cast<int32_t*>(d.wp.d_recs_out.p + out_kept);
            A.nq = (long long)P.n;
            A.dis_wp_tre = dis_wp_tre;
            A.ang_wp_tre = ang_wp_tre;
            A.T = fx::WpAtab{d.wp.d_atab.p, d.wp.atab_a, d.wp.atab_b};
            hipLaunchKernelGGL(fx::k_waypoint_slots, dim3((unsigned)((P.n + 3) / 4)), dim3(256), 0, d.stream, A);
        } else {
            fx::TickOutputsArgs A;
            A.in = reinterpret_cast<const fx::TickQuery*>(d.wp.d_recs_in.p);
            A.out = reinterpret_cast<fx::TickResult*>(d.wp.d_recs_out.p);
            A.cells = S.resident ? P.d_cells : reinterpret_cast<const int32_t*>(d.wp.d_recs_in.p + in_cells);
            A.offsets = S.resident ? P.d_off : reinterpret_cast<const long long*>(d.wp.d_recs_in.p + in_off);
            A.len = S.resident ? P.d_len : nullptr;
            A.kept = reinterpret_cast<int32_t*>(d.wp.d_recs_out.p + out_kept);
            A.path_xyz = reinterpret_cast<double*>(d.wp.d_recs_out.p + out_path);
            A.dir_xyz = reinterpret_cast<double*>(d.wp.d_recs_out.p + out_dir);
            A.nq = (long long)P.n;
            A.dis_wp_tre = dis_wp_tre;
            A.ang_wp_tre = ang_wp_tre;
            A.T = fx::WpAtab{d.wp.d_atab.p, d.wp.atab_a, d.wp.atab_b};
            hipLaunchKernelGGL(fx::k_tick_outputs_slots, dim3((unsigned)((P.n + 3) / 4)), dim3(256), 0, d.stream, A);
            if (K->out_path_xyz) back = out_dir;
            if (K->out_dir_xyz) back = out_kept;
        }
        HIPCHK(h, hipGetLastError());
        if (out_kept_cells) back = out_kept + tot * 2 * sizeof(int32_t);
        HIPCHK(h, hipMemcpyAsync(d.wp.h_recs_out.p, d.wp.d_recs_out.p, back, hipMemcpyDeviceToHost, d.stream));
        return FXJPS_OK;
    };
    // (the st rule on host threads runs beside the device's work)
    int64_t bad_q = -1;
    const WpStHost A{rule, map_start, reso, origin, true, pos, goal, end_occu, dis_wp_tre, ang_wp_tre, prev_wp, prev_dim,
                     out_wp, out_dim, out_goal, out_ang_wp, out_n_kept, K};
    if (int rc = wp_queue_then_collect(h, S, queue, [&] { bad_q = st_on_host ? wp_st_on_host(S, nq, nthreads, A) : -1; })) return rc;
    if (bad_q >= 0) return fail(h, FXJPS_E_ARG, "query %d: fxjps_waypoint_st failed on its path", (int)bad_q);
    for (auto& P : S.parts) {
        const size_t n = (size_t)P.n, tot = (size_t)P.total;
        const size_t rec = K ? sizeof(fx::TickResult) : sizeof(fx::WpSlotResult);
        const uint8_t* base = P.d->wp.h_recs_out.p;
        const double* path3 = reinterpret_cast<const double*>(base + n * rec);
        const double* dir = path3 + (K ? tot * 3 : 0);
        const int32_t* kept = reinterpret_cast<const int32_t*>(dir + (K ? (tot + 2 * n) * 3 : 0));
        for (int64_t i = 0; i < P.n; i++) {
            const int64_t q = P.q0 + i;
            if (rule[q] == 0 && st_on_host) continue;
            const fx::WpSlotResult& r = *reinterpret_cast<const fx::WpSlotResult*>(base + (size_t)i * rec);  // (a TickResult begins with one)
            if (K) {
                const fx::TickResult& t = *reinterpret_cast<const fx::TickResult*>(base + (size_t)i * rec);
                const int64_t len = P.h_off[i + 1] - P.h_off[i];
                if (K->out_point)
                    for (int k = 0; k < 3; k++) K->out_point[3 * q + k] = t.point[k];
                if (K->out_dir_n) K->out_dir_n[q] = t.dir_n;
                if (K->out_dir_back) K->out_dir_back[q] = t.dir_back;
                if (K->out_path_xyz && len > 0)
                    memcpy(K->out_path_xyz + 3 * (P.kept_at + P.h_off[i]), path3 + 3 * P.h_off[i], (size_t)len * 3 * sizeof(double));
                if (K->out_dir_xyz && t.dir_n > 0)
                    memcpy(K->out_dir_xyz + 3 * (P.kept_at + P.h_off[i] + 2 * q), dir + 3 * (P.h_off[i] + 2 * i),
                           (size_t)std::min<int64_t>(t.dir_n, len + 2) * 3 * sizeof(double));
            }
            for (int k = 0; k < 3; k++) out_wp[3 * q + k] = r.wp[k];
            if (out_goal)
                for (int k = 0; k < 3; k++) out_goal[3 * q + k] = r.goal[k];
            if (out_dim) out_dim[q] = r.dim;
            if (out_ang_wp) out_ang_wp[q] = r.ang;
            if (out_n_kept) out_n_kept[q] = r.nkept;
            if (out_kept_cells && rule[q] == 1 && r.nkept > 0)
                memcpy(out_kept_cells + 2 * (P.kept_at + P.h_off[i]), kept + 2 * P.h_off[i], (size_t)r.nkept * 2 * sizeof(int32_t));
        }
    }
    return FXJPS_OK;
}

int fxjps_waypoint_slots_batch(fxjps_t* h, int64_t nq, const int64_t* offsets, const int32_t* cells_xy, const int32_t* grid_ids,
                               const int32_t* rule, const int32_t* map_start, const double* reso, const double* origin, const double* pos,
                               const double* goal, const int32_t* end_occu, double dis_wp_tre, double ang_wp_tre, const double* prev_wp,
                               const int32_t* prev_dim, double* out_wp, int32_t* out_dim, double* out_goal, double* out_ang_wp,
                               int32_t* out_n_kept, int32_t* out_kept_cells, int64_t kept_capacity, int32_t nthreads) {
    return wp_slots_call(h, "fxjps_waypoint_slots_batch", nullptr, nq, offsets, cells_xy, grid_ids, rule, map_start, reso, origin, pos, goal, end_occu,
                         dis_wp_tre, ang_wp_tre, prev_wp, prev_dim, out_wp, out_dim, out_goal, out_ang_wp, out_n_kept, out_kept_cells, kept_capacity,
                         nthreads);
}

int fxjps_tick_outputs_slots(fxjps_t* h, int64_t nq, const int64_t* offsets, const int32_t* cells_xy, const int32_t* grid_ids,
                             const int32_t* rule, const int32_t* map_start, const double* reso, const double* origin, const double* pos,
                             const double* goal, const int32_t* end_occu, double dis_wp_tre, double ang_wp_tre, const double* prev_wp,
                             const int32_t* prev_dim, const double* home_xy, double* out_wp, int32_t* out_dim, double* out_goal,
                             double* out_ang_wp, int32_t* out_n_kept, int32_t* out_kept_cells, int64_t kept_capacity, double* out_point,
                             double* out_path_xyz, int64_t path_capacity, double* out_dir_xyz, int32_t* out_dir_n, int32_t* out_dir_back,
                             int64_t dir_capacity, int32_t nthreads) {
    const TickIO K{home_xy, out_point, out_path_xyz, path_capacity, out_dir_xyz, out_dir_n, out_dir_back, dir_capacity};
    return wp_slots_call(h, "fxjps_tick_outputs_slots", &K, nq, offsets, cells_xy, grid_ids, rule, map_start, reso, origin, pos, goal, end_occu,
                         dis_wp_tre, ang_wp_tre, prev_wp, prev_dim, out_wp, out_dim, out_goal, out_ang_wp, out_n_kept, out_kept_cells, kept_capacity,
                         nthreads);
}

// ------------------------------------------------------------------ kept paths against their slots
// wp_slots_call's pattern on context 0: everything the host can judge first, then ONE copy in (the queries' records with
// their slots' occupancy pointers and extents, the offsets and the cells behind them), ONE launch, ONE copy back and one
// wait, whatever nq is and however many slots are named.  The staging buffers are the waypoint calls' own; nothing a slot,
// a stored result or a resident path lives in is written.
int fxjps_check_paths_slots(fxjps_t* h, int64_t nq, const int64_t* offsets, const int32_t* cells_xy, const int32_t* grid_ids,
                            const int32_t* shift_xy, int32_t* out_verdict, int32_t* out_seg, int32_t* out_cell_xy) {
    static_assert(fx::CHECK_VALID == FXJPS_PATH_VALID && fx::CHECK_EMPTY == FXJPS_PATH_EMPTY && fx::CHECK_BLOCKED == FXJPS_PATH_BLOCKED &&
                      fx::CHECK_OUTSIDE == FXJPS_PATH_OUTSIDE && fx::CHECK_MALFORMED == FXJPS_PATH_MALFORMED,
                  "the kernel's verdicts are the header's");
    static_assert(sizeof(fx::CheckQuery) % 8 == 0, "the offsets and cells behind the records stay aligned");
    if (!h) return FXJPS_E_ARG;
    if (int rr = refuse_on_rank_handle(h, "fxjps_check_paths_slots")) return rr;
    if (nq < 0) return fail(h, FXJPS_E_ARG, "query 0: nq = %lld", (long long)nq);
    if (nq == 0) return FXJPS_OK;
    if (!offsets && !cells_xy) return fail(h, FXJPS_E_ARG, "query 0: resident paths are not checked: pass the paths explicitly");
    if (!offsets || !cells_xy || !grid_ids || !out_verdict || !out_seg || !out_cell_xy)
        return fail(h, FXJPS_E_ARG, "query 0: offsets, cells_xy, grid_ids and the three outputs are required");
    if (offsets[0] != 0) return fail(h, FXJPS_E_ARG, "query 0: offsets[0] must be 0");
    for (int64_t q = 0; q < nq; q++) {
        if (!slot_in_use(h, grid_ids[q]))
            return fail(h, FXJPS_E_ARG, "query %lld names grid slot %d, which is %s", (long long)q, (int)grid_ids[q],
                        grid_ids[q] < 0 || grid_ids[q] >= FXJPS_MAX_GRID_SLOTS ? "out of range" : "empty");
        if (offsets[q + 1] < offsets[q]) return fail(h, FXJPS_E_ARG, "query %lld: offsets must ascend", (long long)q);
    }
    DevCtx& d = h->devs[0];
    const size_t n = (size_t)nq, tot = (size_t)offsets[nq];
    const size_t in_off = n * sizeof(fx::CheckQuery), in_cells = in_off + (n + 1) * sizeof(long long);
    const size_t in_bytes = in_cells + tot * 2 * sizeof(int32_t), out_bytes = n * sizeof(fx::CheckResult);
    const auto run = [&]() -> int {
        HIPCHK(h, hipSetDevice(d.dev));
        HIPCHK(h, d.wp.h_recs_in.ensure(in_bytes));
        HIPCHK(h, d.wp.d_recs_in.ensure(in_bytes));
        HIPCHK(h, d.wp.h_recs_out.ensure(out_bytes));
        HIPCHK(h, d.wp.d_recs_out.ensure(out_bytes));
        fx::CheckQuery* rec = reinterpret_cast<fx::CheckQuery*>(d.wp.h_recs_in.p);
        for (size_t q = 0; q < n; q++) {
            const GridBufs& g = d.slots[(size_t)grid_ids[q]];
            rec[q] = fx::CheckQuery{g.occ.p, g.W, g.H, shift_xy ? shift_xy[2 * q] : 0, shift_xy ? shift_xy[2 * q + 1] : 0};
        }
        memcpy(d.wp.h_recs_in.p + in_off, offsets, (n + 1) * sizeof(long long));
        if (tot > 0) memcpy(d.wp.h_recs_in.p + in_cells, cells_xy, tot * 2 * sizeof(int32_t));
        HIPCHK(h, hipMemcpyAsync(d.wp.d_recs_in.p, d.wp.h_recs_in.p, in_bytes, hipMemcpyHostToDevice, d.stream));
        fx::CheckPathsArgs A;
        A.in = reinterpret_cast<const fx::CheckQuery*>(d.wp.d_recs_in.p);
        A.out = reinterpret_cast<fx::CheckResult*>(d.wp.d_recs_out.p);
        A.cells = reinterpret_cast<const int32_t*>(d.wp.d_recs_in.p + in_cells);
        A.offsets = reinterpret_cast<const long long*>(d.wp.d_recs_in.p + in_off);
        A.nq = (long long)nq;
        hipLaunchKernelGGL(fx::k_check_paths_slots, dim3((unsigned)((nq + 3) / 4)), dim3(256), 0, d.stream, A);
        HIPCHK(h, hipGetLastError());
        HIPCHK(h, hipMemcpyAsync(d.wp.h_recs_out.p, d.wp.d_recs_out.p, out_bytes, hipMemcpyDeviceToHost, d.stream));
        HIPCHK(h, hipStreamSynchronize(d.stream));
        return FXJPS_OK;
    };
    if (int rc = run()) {
        drain_all(h);
        return rc;
    }
    const fx::CheckResult* res = reinterpret_cast<const fx::CheckResult*>(d.wp.h_recs_out.p);
    for (size_t q = 0; q < n; q++) {
        out_verdict[q] = res[q].verdict;
        out_seg[q] = res[q].seg;
        out_cell_xy[2 * q] = res[q].cx;
        out_cell_xy[2 * q + 1] = res[q].cy;
    }
    return FXJPS_OK;
}

// ------------------------------------------------------------------ detected maps into the prior maps
// fxjps_absorb_prior pastes into the priors as they are, fxjps_absorb_prior_grow into priors that grow to what the jobs
// cover, fxjps_absorb_prior_slide cuts every grown prior to a keep window.  One per-job argument check, one staging rule
// and one plan record serve all three; grow and slide share one fold, of which grow is the window that keeps everything.
int fxjps_absorb_job_size(void) { return (int)sizeof(fxjps_absorb_job_t); }
int fxjps_grow_job_size(void) { return (int)sizeof(fxjps_grow_job_t); }
int fxjps_prior_grown_size(void) { return (int)sizeof(fxjps_prior_grown_t); }
int fxjps_prior_keep_size(void) { return (int)sizeof(fxjps_prior_keep_t); }
int fxjps_prior_slid_size(void) { return (int)sizeof(fxjps_prior_slid_t); }

extern "C++" {  // (the helpers are templates over the job, table and out record types)
namespace {
static_assert(fx::ABSORB_JOBS_MAX == FXJPS_MAX_GRID_SLOTS && fx::ABSORB_PRIORS_MAX == FXJPS_MAX_PRIOR_MAPS, "the kernel's table holds every job and a box per prior");
static_assert(fx::ABSORB_OVERWRITE == FXJPS_ABSORB_OVERWRITE && fx::ABSORB_OCCUPIED == FXJPS_ABSORB_OCCUPIED && fx::ABSORB_KNOWN == FXJPS_ABSORB_KNOWN,
              "the kernel's modes are the header's");
static_assert(offsetof(fx::AbsorbTable, changed) == 0 && offsetof(fx::GrowTable, changed) == 0, "the counters come back from the head of the staged input");
constexpr size_t ABSORB_IN_RAWS = (sizeof(fx::AbsorbTable) + 15) & ~(size_t)15;
constexpr size_t GROW_IN_RAWS = (sizeof(fx::GrowTable) + 15) & ~(size_t)15;
template <class Job> constexpr bool IS_GROW_JOB = std::is_same<Job, fxjps_grow_job_t>::value;  // (fxjps_absorb_job_t is its prefix, field by field)

// What the host derives from the jobs before anything is queued.  Per job: where the rectangle lies in its frame -- the
// prior as it is (absorb), the grown prior (grow, slide) -- what of it lies inside the cells the call keeps, and which rows
// of raw are staged: rows (layout 0: x, layout 1: y) that hold those cells, one contiguous piece of raw.  Per prior: the
// union box of its jobs' kept cells and, from the fold, the grown extents, where the old prior's cell (0, 0) lies in them,
// the origin, and the window [k0, k1) of the grown frame that the new prior holds.
struct PriorPlan {
    struct Job {
        long long at[2];         // the frame's cell that rectangle cell (0, 0) lands on
        long long c0[2], c1[2];  // the rectangle clipped to the kept cells of its frame: [c0, c1)
        long long inside;        // how many those are; a job with none stages nothing and is left out of the kernel's table
        size_t raw_off, raw_bytes, in_off;  // the piece of raw, and where it lies in the staged input
        long long row0;          // the first staged row, counted in rows of the rectangle
    };
    struct Prior {
        long long lo[2] = {INT32_MAX, INT32_MAX}, hi[2] = {0, 0};  // the union box, in the jobs' frame
        // the fold's:
        bool named = false;
        int first = -1;                  // the first job that names it: every later one has its ori_pre and map_reso
        long long ext[2] = {0, 0};       // the grown extents, job after job
        long long shift[2] = {0, 0};     // the sum of every job's at_pre
        double op[2] = {0.0, 0.0};       // the grown frame's origin, job after job
        long long k0[2] = {0, 0}, k1[2] = {0, 0};  // the window; 0 and ext unless a keep window was applied (trimmed)
        bool trimmed = false;
        double origin[2] = {0.0, 0.0};   // the window's origin
    };
    std::vector<Job> job;
    Prior prior[FXJPS_MAX_PRIOR_MAPS];
    size_t in_bytes = 0;
};

int absorb_refuse(char* msg, size_t len, const char* fmt, ...) {
    if (msg && len > 0) {
        va_list ap;
        va_start(ap, fmt);
        vsnprintf(msg, len, fmt, ap);
        va_end(ap);
    }
    return FXJPS_E_ARG;
}

int head_check(bool no_jobs, int32_t n, const int32_t* prior_wh, int32_t mode, char* msg, size_t len) {
    if (n < 0 || n > FXJPS_MAX_GRID_SLOTS) return absorb_refuse(msg, len, "job 0: n = %d jobs: must be 0 .. %d", (int)n, FXJPS_MAX_GRID_SLOTS);
    if (n > 0 && no_jobs) return absorb_refuse(msg, len, "job 0: NULL jobs");
    if (!prior_wh) return absorb_refuse(msg, len, "job 0: NULL prior extents");
    if (mode < 0 || mode > 2) return absorb_refuse(msg, len, "job 0: mode %d is not FXJPS_ABSORB_OVERWRITE, _OCCUPIED or _KNOWN", (int)mode);
    return FXJPS_OK;
}

// The argument checks of one job, for all three calls.
template <class Job> int job_check(const Job& a, int j, const int32_t* prior_wh, char* msg, size_t len) {
    if (!a.raw) return absorb_refuse(msg, len, "job %d: NULL raw", j);
    if (a.layout != 0 && a.layout != 1) return absorb_refuse(msg, len, "job %d: layout %d is not 0 or 1", j, (int)a.layout);
    if (a.W0 < 1 || a.H0 < 1 || a.W0 > 8190 || a.H0 > 8190)
        return absorb_refuse(msg, len, "job %d: bad extents (W0 %d, H0 %d): raw must be 1..8190 cells a side", j, (int)a.W0, (int)a.H0);
    const long long ext[2] = {a.W0, a.H0};
    for (int k = 0; k < 2; k++)
        if (a.win[k] < 1 || a.lo[k] < 0 || (long long)a.lo[k] + a.win[k] > ext[k])
            return absorb_refuse(msg, len, "job %d: axis %d: the rectangle (%d + %d) is empty or does not lie inside raw's %lld cells", j, k, (int)a.lo[k],
                                 (int)a.win[k], ext[k]);
    if (a.prior < 0 || a.prior >= FXJPS_MAX_PRIOR_MAPS) return absorb_refuse(msg, len, "job %d: prior %d is not in 0 .. %d", j, (int)a.prior, FXJPS_MAX_PRIOR_MAPS - 1);
    if (prior_wh[2 * a.prior] < 1 || prior_wh[2 * a.prior + 1] < 1) return absorb_refuse(msg, len, "job %d: prior %d is not set", j, (int)a.prior);
    if (!std::isfinite(a.map_reso) || !(a.map_reso > 0.0)) return absorb_refuse(msg, len, "job %d: map_reso %g must be finite and > 0", j, a.map_reso);
    for (int k = 0; k < 2; k++) {
        if (!std::isfinite(a.map_o[k]) || !std::isfinite(a.ori_pre[k])) return absorb_refuse(msg, len, "job %d: a non-finite map_o / ori_pre", j);
        if constexpr (IS_GROW_JOB<Job>)
            if (!std::isfinite(a.map_t[k])) return absorb_refuse(msg, len, "job %d: a non-finite map_t", j);
    }
    return FXJPS_OK;
}

// The rectangle of job a, with cell (0, 0) on q.at, clipped to the cells [w0, w1) of its frame; P's union box takes what
// is left.  -> whether any cell is.
template <class Job> bool clip(const Job& a, PriorPlan::Job& q, PriorPlan::Prior& P, const long long w0[2], const long long w1[2]) {
    for (int k = 0; k < 2; k++) {
        q.c0[k] = std::max(q.at[k], w0[k]);
        q.c1[k] = std::min(q.at[k] + (long long)a.win[k], w1[k]);
    }
    q.inside = std::max(q.c1[0] - q.c0[0], 0ll) * std::max(q.c1[1] - q.c0[1], 0ll);
    if (q.inside > 0)
        for (int k = 0; k < 2; k++) {
            P.lo[k] = std::min(P.lo[k], q.c0[k]);
            P.hi[k] = std::max(P.hi[k], q.c1[k]);
        }
    return q.inside > 0;
}

// `rows` rows of job j's rectangle from row0 on go into the staged input, behind the `total` bytes that are there.
template <class Job> int stage(const Job& a, int j, PriorPlan::Job& q, long long row0, long long rows, size_t& total, char* msg, size_t len) {
    const size_t row = (size_t)(a.layout ? a.W0 : a.H0);
    q.row0 = row0;
    q.raw_off = (size_t)(a.lo[a.layout ? 1 : 0] + row0) * row;
    q.raw_bytes = (size_t)rows * row;
    q.in_off = total;
    total += (q.raw_bytes + 15) & ~(size_t)15;
    if (total > ((size_t)1 << 30)) return absorb_refuse(msg, len, "job %d: more than 2^30 bytes to stage", j);
    return FXJPS_OK;
}

// What a passed check tells the caller of every job: its cells kept and dropped and, for grow and slide, the cell of the
// prior AS THE CALL LEAVES IT that rectangle cell (0, 0) lies on.
template <class Job> void write_jobs(Job* jobs, int n, const PriorPlan& plan) {
    for (int j = 0; j < n; j++) {
        const PriorPlan::Job& q = plan.job[(size_t)j];
        jobs[j].inside = q.inside;
        jobs[j].outside = (long long)jobs[j].win[0] * jobs[j].win[1] - q.inside;
        if constexpr (IS_GROW_JOB<Job>)
            for (int k = 0; k < 2; k++) jobs[j].at[k] = (int32_t)(q.at[k] - plan.prior[jobs[j].prior].k0[k]);
    }
}

// Everything fxjps_absorb_prior refuses except a rank handle, from the arguments and the priors' extents alone.  Every job
// is placed against the prior as it is with ITS ori_pre and clipped to it; the placement is world_call's: float64, the
// reference's operations in the reference's order (st:212-214).  (Not the fold below, which moves the origin job after
// job: that is not bit-equal in float64.)  Writes nothing unless every job passes; then plan and every job's inside /
// outside.
int absorb_check(fxjps_absorb_job_t* jobs, int32_t n, int32_t mode, const int32_t* prior_wh, PriorPlan& plan, char* msg, size_t len) {
    if (int rc = head_check(!jobs, n, prior_wh, mode, msg, len)) return rc;
    plan = PriorPlan{};
    plan.job.resize((size_t)n);
    plan.in_bytes = ABSORB_IN_RAWS;
    const long long none[2] = {0, 0};
    for (int j = 0; j < n; j++) {
        const fxjps_absorb_job_t& a = jobs[j];
        if (int rc = job_check(a, j, prior_wh, msg, len)) return rc;
        PriorPlan::Job& q = plan.job[(size_t)j];
        for (int k = 0; k < 2; k++) {
            const double o1 = std::min(a.map_o[k], a.ori_pre[k]);  // st:212
            long long at_raw, at_pre;
            if (!trunc_i32((a.map_o[k] - o1) / a.map_reso, at_raw) || !trunc_i32((a.ori_pre[k] - o1) / a.map_reso, at_pre))  // st:213-214
                return absorb_refuse(msg, len, "job %d: a placement index is outside int32", j);
            q.at[k] = at_raw - at_pre;
        }
        const long long l[2] = {prior_wh[2 * a.prior], prior_wh[2 * a.prior + 1]};
        if (clip(a, q, plan.prior[a.prior], none, l))  // (the rectangle's rows whole: the kernel clips)
            if (int rc = stage(a, j, q, 0, a.win[a.layout ? 1 : 0], plan.in_bytes, msg, len)) return rc;
    }
    write_jobs(jobs, n, plan);
    return FXJPS_OK;
}

// The geometry of fxjps_absorb_prior_grow and fxjps_absorb_prior_slide and everything they refuse but a rank handle and a
// NULL out, from the arguments and the priors' extents alone; reads the jobs and writes only plan.  The fold is float64,
// the reference's operations in the reference's order (st:187, :212-216), job after job on the extents and origin the job
// before left.  Then per prior the window: the whole grown frame, or -- keep[p].use says when -- the keep window, by one
// division, one truncation and a clamp on the double per bound.  A prior that a keep window may cut is not held to the
// limit job after job, only to int32; its window is.  Then per job what of its rectangle lies inside the window: the rows
// to stage and the union box.  keep == NULL: no prior has a window, which is fxjps_absorb_prior_grow.
int prior_fold(const fxjps_grow_job_t* jobs, int32_t n, int32_t mode, const int32_t* prior_wh, const int32_t* limit_wh, const fxjps_prior_keep_t* keep,
               PriorPlan& plan, char* msg, size_t len) {
    const auto use = [keep](int p) -> int { return keep ? keep[p].use : FXJPS_KEEP_NONE; };
    for (int p = 0; p < FXJPS_MAX_PRIOR_MAPS; p++) {
        if (use(p) < FXJPS_KEEP_NONE || use(p) > FXJPS_KEEP_OVER_LIMIT)
            return absorb_refuse(msg, len, "prior %d: keep.use %d is not FXJPS_KEEP_NONE, _ALWAYS or _OVER_LIMIT", p, use(p));
        if (use(p) == FXJPS_KEEP_NONE) continue;
        for (int k = 0; k < 2; k++) {
            if (std::isnan(keep[p].lo[k]) || std::isnan(keep[p].hi[k])) return absorb_refuse(msg, len, "prior %d: axis %d: NaN in the keep window", p, k);
            if (keep[p].lo[k] > keep[p].hi[k])
                return absorb_refuse(msg, len, "prior %d: axis %d: the keep window's lo %g is above its hi %g", p, k, keep[p].lo[k], keep[p].hi[k]);
        }
    }
    if (int rc = head_check(!jobs, n, prior_wh, mode, msg, len)) return rc;
    long long limit[2] = {8190, 8190};
    if (limit_wh)
        for (int k = 0; k < 2; k++) {
            limit[k] = limit_wh[k];
            if (limit[k] < 1 || limit[k] > 8190) return absorb_refuse(msg, len, "job 0: axis %d: the limit %lld is not in 1 .. 8190", k, limit[k]);
        }
    plan = PriorPlan{};
    plan.job.resize((size_t)n);
    plan.in_bytes = GROW_IN_RAWS;
    for (int j = 0; j < n; j++) {
        const fxjps_grow_job_t& a = jobs[j];
        if (int rc = job_check(a, j, prior_wh, msg, len)) return rc;
        PriorPlan::Prior& P = plan.prior[a.prior];
        if (!P.named) {
            P.named = true;
            P.first = j;
            for (int k = 0; k < 2; k++) {
                P.ext[k] = prior_wh[2 * a.prior + k];
                P.op[k] = a.ori_pre[k];
            }
        } else {
            const fxjps_grow_job_t& f = jobs[P.first];
            if (memcmp(f.ori_pre, a.ori_pre, sizeof(a.ori_pre)) != 0 || memcmp(&f.map_reso, &a.map_reso, sizeof(double)) != 0)
                return absorb_refuse(msg, len, "job %d: ori_pre / map_reso are not bit-equal to those of job %d, which names prior %d as well", j, P.first,
                                     (int)a.prior);
        }
        const double reso = a.map_reso;
        PriorPlan::Job& q = plan.job[(size_t)j];
        long long at_pre[2];
        for (int k = 0; k < 2; k++) {
            const double o = a.map_o[k], op = P.op[k];
            const double o1 = std::min(o, op);                       // st:212
            const double t_pre = op + reso * (double)P.ext[k];       // st:187, with the current extents
            long long at_raw, ref;
            if (!trunc_i32((o - o1) / reso, at_raw) || !trunc_i32((op - o1) / reso, at_pre[k]) ||  // st:213-214
                !trunc_i32((std::max(t_pre, a.map_t[k]) - o1) / reso, ref))                        // st:215-216
                return absorb_refuse(msg, len, "job %d: a placement index or the canvas extent is outside int32", j);
            const long long size = std::max(ref, std::max(at_pre[k] + P.ext[k], at_raw + (long long)a.win[k]));
            if (use(a.prior) != FXJPS_KEEP_NONE) {
                if (size > INT32_MAX) return absorb_refuse(msg, len, "job %d: a placement index or the canvas extent is outside int32", j);
            } else if (size > limit[k])
                return absorb_refuse(msg, len, "job %d: axis %d: prior %d would grow to %lld cells, above the limit of %lld", j, k, (int)a.prior, size, limit[k]);
            q.at[k] = at_raw;
            P.ext[k] = size;
            P.op[k] = o1;
            P.shift[k] += at_pre[k];
        }
        for (int i = 0; i < j; i++)  // (the earlier rectangles on this prior move with the old prior)
            if (jobs[i].prior == a.prior)
                for (int k = 0; k < 2; k++) plan.job[(size_t)i].at[k] += at_pre[k];
    }
    for (int p = 0; p < FXJPS_MAX_PRIOR_MAPS; p++) {
        PriorPlan::Prior& P = plan.prior[p];
        if (!P.named) {
            if (use(p) != FXJPS_KEEP_NONE) return absorb_refuse(msg, len, "prior %d: a keep window for a prior that no job names", p);
            continue;
        }
        for (int k = 0; k < 2; k++) {
            P.k1[k] = P.ext[k];
            P.origin[k] = P.op[k];
        }
        if (use(p) == FXJPS_KEEP_NONE || (use(p) == FXJPS_KEEP_OVER_LIMIT && P.ext[0] <= limit[0] && P.ext[1] <= limit[1])) continue;
        P.trimmed = true;
        const double reso = jobs[P.first].map_reso;
        for (int k = 0; k < 2; k++) {
            const double G = (double)P.ext[k];
            const double a = std::trunc((keep[p].lo[k] - P.op[k]) / reso), b = std::trunc((keep[p].hi[k] - P.op[k]) / reso);
            P.k0[k] = (long long)(a < 0.0 ? 0.0 : a > G ? G : a);  // (clamped as a double: a bound may be infinite)
            P.k1[k] = (long long)(b < 0.0 ? 0.0 : b > G ? G : b);
            if (P.k1[k] <= P.k0[k])
                return absorb_refuse(msg, len, "prior %d: axis %d: the keep window holds no cell of the grown prior (cells %lld .. %lld of %lld)", p, k, P.k0[k],
                                     P.k1[k], P.ext[k]);
            if (P.k1[k] - P.k0[k] > limit[k])
                return absorb_refuse(msg, len, "prior %d: axis %d: the keep window of %lld cells is above the limit of %lld", p, k, P.k1[k] - P.k0[k], limit[k]);
            if (P.k0[k] != 0) P.origin[k] = P.op[k] + reso * (double)P.k0[k];
        }
    }
    for (int j = 0; j < n; j++) {  // (of a rectangle only the rows inside the window are staged; all of them where nothing is cut)
        const fxjps_grow_job_t& a = jobs[j];
        PriorPlan::Prior& P = plan.prior[a.prior];
        PriorPlan::Job& q = plan.job[(size_t)j];
        const int r = a.layout ? 1 : 0;
        if (clip(a, q, P, P.k0, P.k1))
            if (int rc = stage(a, j, q, q.c0[r] - q.at[r], q.c1[r] - q.c0[r], plan.in_bytes, msg, len)) return rc;
    }
    for (PriorPlan::Prior& P : plan.prior)
        if (P.lo[0] > P.hi[0]) P.lo[0] = P.lo[1] = P.hi[0] = P.hi[1] = 0;  // (no rectangle reaches the window: an empty box)
    return FXJPS_OK;
}

// fxjps_grow_check (Out = fxjps_prior_grown_t, keep NULL) and fxjps_slide_check (fxjps_prior_slid_t): the fold, and once it
// has passed -- nothing is written before -- every job's inside / outside / at and every field of out but `changed`.  The
// slid record begins as the grown record does.
template <class Out> int fold_check(fxjps_grow_job_t* jobs, int32_t n, int32_t mode, const int32_t* prior_wh, const int32_t* limit_wh,
                                    const fxjps_prior_keep_t* keep, Out* out, PriorPlan& plan, char* msg, size_t len) {
    constexpr bool SLID = std::is_same<Out, fxjps_prior_slid_t>::value;
    // (a NULL out: fxjps_slide_check refuses it before anything else, fxjps_grow_check behind the extents and before the mode)
    if (!out && (SLID || !head_check(!jobs, n, prior_wh, 0, nullptr, 0))) return absorb_refuse(msg, len, "job 0: NULL out");
    if (int rc = prior_fold(jobs, n, mode, prior_wh, limit_wh, keep, plan, msg, len)) return rc;
    write_jobs(jobs, n, plan);
    for (int p = 0; p < FXJPS_MAX_PRIOR_MAPS; p++) {
        const PriorPlan::Prior& P = plan.prior[p];
        Out& g = out[p];
        g.named = P.named ? 1 : 0;
        for (int k = 0; k < 2; k++) {
            const int32_t as_is = prior_wh[2 * p + k];
            (k ? g.H : g.W) = P.named ? (int32_t)(P.k1[k] - P.k0[k]) : as_is;
            g.shift[k] = (int32_t)(P.shift[k] - P.k0[k]);
            g.origin[k] = P.origin[k];
            if constexpr (SLID) {
                g.grown_wh[k] = P.named ? (int32_t)P.ext[k] : as_is;
                g.cut_lo[k] = (int32_t)P.k0[k];
                g.cut_hi[k] = (int32_t)(P.ext[k] - P.k1[k]);
            }
        }
        if constexpr (SLID)
            g.trimmed = P.trimmed ? 1 : 0;
        else
            g.reserved_ = 0;
    }
    return FXJPS_OK;
}

// ---- one context's part of a call: ONE copy in, ONE launch, one copy back and one wait, whatever n is.  The staged input
// begins with the kernel's table; the counters at its head are left in d.h_absorb_out.
template <class Table> int table_begin(fxjps* h, DevCtx& d, size_t in_bytes, int mode, Table*& T) {
    HIPCHK(h, hipSetDevice(d.dev));
    HIPCHK(h, d.h_absorb_in.ensure(in_bytes));
    HIPCHK(h, d.d_absorb_in.ensure(in_bytes));
    HIPCHK(h, d.h_absorb_out.ensure(FXJPS_MAX_PRIOR_MAPS));
    T = reinterpret_cast<Table*>(d.h_absorb_in.p);
    memset(T, 0, sizeof(Table));
    T->mode = mode;
    return FXJPS_OK;
}

// The jobs of prior p that stage anything, in job order, as job[nj ...], and their rows into the staged input.  -> nj
template <class Job> int table_jobs(DevCtx& d, fx::AbsorbJobDev* job, int nj, const Job* jobs, int n, int p, const PriorPlan& plan) {
    for (int j = 0; j < n; j++) {
        const Job& a = jobs[j];
        const PriorPlan::Job& q = plan.job[(size_t)j];
        if (a.prior != p || q.inside <= 0) continue;
        fx::AbsorbJobDev& J = job[nj++];
        J.stride = a.layout ? a.W0 : a.H0;
        // (cell (i, j) of the rectangle is read at row * stride + column from here; rows below row0 are not staged and not
        // read, so the address of row 0 is only ever an operand)
        J.at = reinterpret_cast<const uint8_t*>(reinterpret_cast<uintptr_t>(d.d_absorb_in.p) + q.in_off + (size_t)(a.layout ? a.lo[0] : a.lo[1]) -
                                                (size_t)q.row0 * (size_t)J.stride);
        J.layout = a.layout;
        J.x0 = (int32_t)q.at[0];
        J.y0 = (int32_t)q.at[1];
        J.w = a.win[0];
        J.h = a.win[1];
        memcpy(d.h_absorb_in.p + q.in_off, static_cast<const uint8_t*>(a.raw) + q.raw_off, q.raw_bytes);
    }
    return nj;
}

template <class Table> int table_run(fxjps* h, DevCtx& d, size_t in_bytes, uint32_t blocks, void (*kernel)(Table*)) {
    memset(d.h_absorb_out.p, 0, FXJPS_MAX_PRIOR_MAPS * sizeof(unsigned long long));
    if (blocks == 0) return FXJPS_OK;  // (no box: nothing to queue)
    HIPCHK(h, hipMemcpyAsync(d.d_absorb_in.p, d.h_absorb_in.p, in_bytes, hipMemcpyHostToDevice, d.stream));
    hipLaunchKernelGGL(kernel, dim3(blocks), dim3(256), 0, d.stream, reinterpret_cast<Table*>(d.d_absorb_in.p));
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipMemcpyAsync(d.h_absorb_out.p, d.d_absorb_in.p, FXJPS_MAX_PRIOR_MAPS * sizeof(unsigned long long), hipMemcpyDeviceToHost, d.stream));
    HIPCHK(h, hipStreamSynchronize(d.stream));
    return FXJPS_OK;
}

// fxjps_absorb_prior on one context: a box per prior that a rectangle meets, over the union of its clipped rectangles.
int absorb_on(fxjps* h, DevCtx& d, const fxjps_absorb_job_t* jobs, int n, int mode, const PriorPlan& plan) {
    fx::AbsorbTable* T;
    if (int rc = table_begin(h, d, plan.in_bytes, mode, T)) return rc;
    int nb = 0, nj = 0;
    uint32_t at = 0;
    for (int p = 0; p < FXJPS_MAX_PRIOR_MAPS; p++) {  // (jobs grouped by prior, in job order within a prior)
        const PriorPlan::Prior& P = plan.prior[p];
        fx::AbsorbBoxDev B{};
        B.job0 = nj;
        nj = table_jobs(d, T->job, nj, jobs, n, p, plan);
        B.njobs = nj - B.job0;
        if (B.njobs == 0) continue;
        const DevCtx::PriorBuf& pr = d.priors[(size_t)p];
        B.occ = pr.occ.p;
        B.pH = pr.H;
        B.x0 = (int32_t)P.lo[0];
        B.y0 = (int32_t)P.lo[1];
        B.w = (int32_t)(P.hi[0] - P.lo[0]);
        B.h = (int32_t)(P.hi[1] - P.lo[1]);
        B.prior = p;
        T->first[nb] = at;
        T->box[nb++] = B;
        at += (uint32_t)(((long long)B.w * B.h + 255) / 256);  // (at most 16 x 8190 x 8190 / 256 blocks)
    }
    T->first[nb] = at;
    T->nbox = nb;
    return table_run(h, d, plan.in_bytes, at, fx::k_prior_absorb);
}

// fxjps_absorb_prior_grow and (window) fxjps_absorb_prior_slide on one context: a box per named prior, over the cells
// [k0, k1) of its grown frame, written into the spare buffer (PriorBuf::next).  Nothing the world-frame calls read is
// touched.  The job records and the union box stay in the grown frame; the launch is k_prior_grow<window>.
int grow_on(fxjps* h, DevCtx& d, const fxjps_grow_job_t* jobs, int n, int mode, const PriorPlan& plan, bool window) {
    fx::GrowTable* T;
    if (int rc = table_begin(h, d, plan.in_bytes, mode, T)) return rc;
    int nb = 0, nj = 0;
    uint32_t at = 0;
    for (int p = 0; p < FXJPS_MAX_PRIOR_MAPS; p++) {  // (jobs grouped by prior, in job order within a prior)
        const PriorPlan::Prior& P = plan.prior[p];
        if (!P.named) continue;
        DevCtx::PriorBuf& pr = d.priors[(size_t)p];
        const long long nW = P.k1[0] - P.k0[0], nH = P.k1[1] - P.k0[1];
        HIPCHK(h, pr.next.ensure((size_t)(nW * nH)));
        fx::GrowBoxDev B{};
        B.job0 = nj;
        nj = table_jobs(d, T->job, nj, jobs, n, p, plan);
        B.njobs = nj - B.job0;
        B.old = pr.occ.p;
        B.out = pr.next.p;
        B.oW = pr.W;
        B.oH = pr.H;
        B.sx = (int32_t)P.shift[0];
        B.sy = (int32_t)P.shift[1];
        B.nW = (int32_t)nW;
        B.nH = (int32_t)nH;
        B.x0 = (int32_t)P.lo[0];
        B.y0 = (int32_t)P.lo[1];
        B.w = (int32_t)(P.hi[0] - P.lo[0]);
        B.h = (int32_t)(P.hi[1] - P.lo[1]);
        B.prior = p;
        T->k0[nb][0] = (int32_t)P.k0[0];  // (0 unless a window was applied; k_prior_grow<false> does not read it)
        T->k0[nb][1] = (int32_t)P.k0[1];
        T->first[nb] = at;
        T->box[nb++] = B;
        at += (uint32_t)((nW * nH + 255) / 256);  // (at most 16 x 8190 x 8190 / 256 blocks)
    }
    T->first[nb] = at;
    T->nbox = nb;
    return window ? table_run(h, d, plan.in_bytes, at, fx::k_prior_grow<true>) : table_run(h, d, plan.in_bytes, at, fx::k_prior_grow<false>);
}

// The priors' extents as the checks take them: context 0's (every context holds the same).
void prior_extents(const fxjps* h, int32_t prior_wh[2 * FXJPS_MAX_PRIOR_MAPS]) {
    const DevCtx& d0 = h->devs[0];
    for (size_t p = 0; p < FXJPS_MAX_PRIOR_MAPS; p++) {
        prior_wh[2 * p] = p < d0.priors.size() ? d0.priors[p].W : 0;
        prior_wh[2 * p + 1] = p < d0.priors.size() ? d0.priors[p].H : 0;
    }
}

// fxjps_absorb_prior_grow and fxjps_absorb_prior_slide (Out = fxjps_prior_slid_t: the window kernel).  Every context writes
// its own new copies from the caller's raws (host copies, no collective); the priors that the world-frame calls read are
// swapped only when all of them have succeeded, so a failure leaves every context as it was.
template <class Out> int grow_call(fxjps* h, const char* what, fxjps_grow_job_t* jobs, int32_t n, int32_t mode, const int32_t* limit_wh,
                                   const fxjps_prior_keep_t* keep, Out* out) {
    constexpr bool WINDOW = std::is_same<Out, fxjps_prior_slid_t>::value;
    if (!h) return FXJPS_E_ARG;
    if (int rr = refuse_on_rank_handle(h, what)) return rr;
    int32_t prior_wh[2 * FXJPS_MAX_PRIOR_MAPS];
    prior_extents(h, prior_wh);
    PriorPlan plan;
    char why[400] = "";
    if (fold_check(jobs, n, mode, prior_wh, limit_wh, keep, out, plan, why, sizeof(why))) return fail(h, FXJPS_E_ARG, "%s", why);
    for (int p = 0; p < FXJPS_MAX_PRIOR_MAPS; p++) out[p].changed = 0;
    if (n == 0) return FXJPS_OK;
    int rc = run_side_by_side(h->devs.size(), [&](size_t r) -> int { return grow_on(h, h->devs[r], jobs, n, mode, plan, WINDOW); });
    if (rc) {
        drain_all(h);
        (void)hipGetLastError();
        return rc;
    }
    for (auto& d : h->devs)
        for (int p = 0; p < FXJPS_MAX_PRIOR_MAPS; p++)
            if (plan.prior[p].named) {
                DevCtx::PriorBuf& pr = d.priors[(size_t)p];
                std::swap(pr.occ, pr.next);  // (the old buffer is the next call's spare)
                pr.W = (int)(plan.prior[p].k1[0] - plan.prior[p].k0[0]);
                pr.H = (int)(plan.prior[p].k1[1] - plan.prior[p].k0[1]);
            }
    for (int p = 0; p < FXJPS_MAX_PRIOR_MAPS; p++) out[p].changed = (int64_t)h->devs[0].h_absorb_out.p[p];
    return FXJPS_OK;
}
}  // namespace
}  // extern "C++"

int fxjps_absorb_check(fxjps_absorb_job_t* jobs, int32_t n, int32_t mode, const int32_t* prior_wh, char* msg, int32_t msg_len) {
    if (msg && msg_len > 0) msg[0] = 0;
    PriorPlan plan;
    return absorb_check(jobs, n, mode, prior_wh, plan, msg, msg_len > 0 ? (size_t)msg_len : 0);
}

int fxjps_absorb_prior(fxjps_t* h, fxjps_absorb_job_t* jobs, int32_t n, int32_t mode, int64_t out_changed[FXJPS_MAX_PRIOR_MAPS]) {
    if (!h) return FXJPS_E_ARG;
    if (!out_changed) return fail(h, FXJPS_E_ARG, "job 0: NULL out_changed");
    if (int rr = refuse_on_rank_handle(h, "fxjps_absorb_prior")) return rr;
    int32_t prior_wh[2 * FXJPS_MAX_PRIOR_MAPS];
    prior_extents(h, prior_wh);
    PriorPlan plan;
    char why[400] = "";
    if (absorb_check(jobs, n, mode, prior_wh, plan, why, sizeof(why))) return fail(h, FXJPS_E_ARG, "%s", why);
    // every context pastes into its own copy of the priors, in place, from the caller's raws (host copies, no collective)
    int rc = run_side_by_side(h->devs.size(), [&](size_t r) -> int { return absorb_on(h, h->devs[r], jobs, n, mode, plan); });
    if (rc) {
        drain_all(h);
        for (int j = 0; j < n; j++)  // (a prior whose paste failed on one context is released on all of them, as fxjps_set_prior_map does)
            for (auto& d : h->devs)
                if ((size_t)jobs[j].prior < d.priors.size()) {
                    DevCtx::PriorBuf& pr = d.priors[(size_t)jobs[j].prior];
                    if (hipSetDevice(d.dev) == hipSuccess) pr.occ.release();
                    pr.W = pr.H = 0;
                }
        (void)hipGetLastError();
        return rc;
    }
    for (int p = 0; p < FXJPS_MAX_PRIOR_MAPS; p++) out_changed[p] = (int64_t)h->devs[0].h_absorb_out.p[p];
    return FXJPS_OK;
}

int fxjps_grow_check(fxjps_grow_job_t* jobs, int32_t n, int32_t mode, const int32_t* prior_wh, const int32_t* limit_wh,
                     fxjps_prior_grown_t out[FXJPS_MAX_PRIOR_MAPS], char* msg, int32_t msg_len) {
    if (msg && msg_len > 0) msg[0] = 0;
    PriorPlan plan;
    return fold_check(jobs, n, mode, prior_wh, limit_wh, nullptr, out, plan, msg, msg_len > 0 ? (size_t)msg_len : 0);
}

int fxjps_absorb_prior_grow(fxjps_t* h, fxjps_grow_job_t* jobs, int32_t n, int32_t mode, const int32_t* limit_wh,
                            fxjps_prior_grown_t out[FXJPS_MAX_PRIOR_MAPS]) {
    return grow_call(h, "fxjps_absorb_prior_grow", jobs, n, mode, limit_wh, nullptr, out);
}

int fxjps_slide_check(fxjps_grow_job_t* jobs, int32_t n, int32_t mode, const int32_t* prior_wh, const int32_t* limit_wh,
                      const fxjps_prior_keep_t keep[FXJPS_MAX_PRIOR_MAPS], fxjps_prior_slid_t out[FXJPS_MAX_PRIOR_MAPS], char* msg, int32_t msg_len) {
    if (msg && msg_len > 0) msg[0] = 0;
    PriorPlan plan;
    return fold_check(jobs, n, mode, prior_wh, limit_wh, keep, out, plan, msg, msg_len > 0 ? (size_t)msg_len : 0);
}

int fxjps_absorb_prior_slide(fxjps_t* h, fxjps_grow_job_t* jobs, int32_t n, int32_t mode, const int32_t* limit_wh,
                             const fxjps_prior_keep_t keep[FXJPS_MAX_PRIOR_MAPS], fxjps_prior_slid_t out[FXJPS_MAX_PRIOR_MAPS]) {
    return grow_call(h, "fxjps_absorb_prior_slide", jobs, n, mode, limit_wh, keep, out);
}

int fxjps_last_timing(fxjps_t* h, fxjps_timing_t* out) {
    if (!h || !out) return FXJPS_E_ARG;
    *out = h->timing;
    return FXJPS_OK;
}

int fxjps_last_timing_sized(fxjps_t* h, void* out, int64_t out_size) {
    if (!h || !out || out_size < 0) return FXJPS_E_ARG;
    memcpy(out, &h->timing, (size_t)std::min<int64_t>(out_size, (int64_t)sizeof(fxjps_timing_t)));
    return FXJPS_OK;
}

int fxjps_selftest_sqrt(fxjps_t* h, uint32_t n0, uint32_t n1, double* out) {
    if (!h || !out || n1 < n0) return FXJPS_E_ARG;
    if (n1 == n0) return FXJPS_OK;
    DevCtx& d = h->devs[0];
    HIPCHK(h, hipSetDevice(d.dev));
    const size_t n = (size_t)(n1 - n0);
    double* buf = nullptr;
    HIPCHK(h, hipMalloc((void**)&buf, n * sizeof(double)));
    hipLaunchKernelGGL(fx::k_sqrt_selftest, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, d.stream, n0, n1, buf);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(out, buf, n * sizeof(double), hipMemcpyDeviceToHost, d.stream);
    if (e == hipSuccess) e = hipStreamSynchronize(d.stream);
    (void)hipFree(buf);
    if (e != hipSuccess) return fail(h, FXJPS_E_HIP, "selftest: %s", hipGetErrorString(e));
    return FXJPS_OK;
}


// raw device counters of the last batch on device 0: [0] pops [1] pushes [2] refills [3] slow pops,
// [8..17] per-phase cycles in FXJPS_PROF builds (tools only)
int fxjps_debug_counters(fxjps_t* h, unsigned long long* out32) {
    if (!h || !out32) return FXJPS_E_ARG;
    DevCtx& d = h->devs[0];
    if (!d.h_counters.p) return FXJPS_E_ARG;
    memcpy(out32, d.h_counters.p, 64 * sizeof(unsigned long long));
    return FXJPS_OK;
}

// per-query diagnostics of the last batch on device 0 (FXJPS_QSTAT=1): 4 u64 per query (tools only)
int fxjps_debug_qstat(fxjps_t* h, unsigned long long* out, int64_t nq) {
    if (!h || !out) return FXJPS_E_ARG;
    DevCtx& d = h->devs[0];
    if (!d.d_qstat.p || nq > d.nq) return FXJPS_E_ARG;
    HIPCHK(h, hipSetDevice(d.dev));
    HIPCHK(h, hipMemcpy(out, d.d_qstat.p, (size_t)nq * 4 * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    return FXJPS_OK;
}

// what every handle of the process holds right now (tests: a closed handle gives everything back)
int fxjps_debug_live_bytes(int64_t* out_device, int64_t* out_pinned) {
    if (out_device) *out_device = g_live_device.load();
    if (out_pinned) *out_pinned = g_live_pinned.load();
    return FXJPS_OK;
}

// the read sets of the stored results (tests): what fxjps_replan_frame tests the next frame's updates against
int fxjps_debug_read_sets(fxjps_t* h, uint64_t* out, int64_t nq, int32_t* out_tile_shift) {
    if (!h || !out || !out_tile_shift) return FXJPS_E_ARG;
    if (!h->q_results_valid) return fail(h, FXJPS_E_ARG, "no tracked results: the last call was not a tracked fxjps_replan_frame");
    int64_t total = 0;
    for (auto& d : h->devs) total += d.nq;
    if (nq != total) return fail(h, FXJPS_E_ARG, "the stored results hold %lld queries, not %lld", (long long)total, (long long)nq);
    for (auto& d : h->devs) {  // (shard order: the contexts' q0 ascend)
        uint64_t* dst = out + (size_t)d.q0 * 128;
        const size_t n = (size_t)d.nq * 128;
        if (d.h_qread.size() >= n)
            memcpy(dst, d.h_qread.data(), n * sizeof(uint64_t));
        else  // (no tracked search ever ran on this context: every query it holds ended without one)
            memset(dst, 0, n * sizeof(uint64_t));
    }
    *out_tile_shift = h->devs[0].tsh;
    return FXJPS_OK;
}

int fxjps_selftest_wavemin(fxjps_t* h, int32_t rounds, uint64_t seed, int64_t* mismatches) {
    if (!h || !mismatches || rounds < 1 || rounds > (1 << 16)) return FXJPS_E_ARG;
    DevCtx& d = h->devs[0];
    HIPCHK(h, hipSetDevice(d.dev));
    std::vector<uint64_t> in((size_t)rounds * 64), out((size_t)rounds * 4 + (size_t)rounds * 64);  // minima, then u32 ranks (32-bit keys, 96-bit keys)
    uint64_t x = seed * 0x9E3779B97F4A7C15ull + 1;
    for (size_t i = 0; i < in.size(); i++) {
        x ^= x << 13;
        x ^= x >> 7;
        x ^= x << 17;
        // mix of wide-range values and many ties
        in[i] = (i % 7 == 0) ? (x & 0xFF) : ((i % 5 == 0) ? (x | 0xFFFFFFFF00000000ull) : x);
    }
    uint64_t *din = nullptr, *dout = nullptr;
    HIPCHK(h, hipMalloc((void**)&din, in.size() * 8));
    HIPCHK(h, hipMalloc((void**)&dout, out.size() * 8));
    hipError_t e = hipMemcpy(din, in.data(), in.size() * 8, hipMemcpyHostToDevice);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(fx::k_selftest_wavemin, dim3(1), dim3(64), 0, d.stream, din, dout, rounds);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipStreamSynchronize(d.stream);
    if (e == hipSuccess) e = hipMemcpy(out.data(), dout, out.size() * 8, hipMemcpyDeviceToHost);
    (void)hipFree(din);
    (void)hipFree(dout);
    if (e != hipSuccess) return fail(h, FXJPS_E_HIP, "selftest: %s", hipGetErrorString(e));
    int64_t bad = 0;
    for (int r = 0; r < rounds; r++) {
        uint64_t m64 = ~0ull;
        uint32_t m32 = ~0u;
        for (int l = 0; l < 64; l++) {
            m64 = std::min(m64, in[(size_t)r * 64 + l]);
            m32 = std::min(m32, (uint32_t)(in[(size_t)r * 64 + l] >> 7));
        }
        if (out[(size_t)r * 4] != m64 || out[(size_t)r * 4 + 1] != m64 || out[(size_t)r * 4 + 2] != m32 || out[(size_t)r * 4 + 3] != m32) bad++;
        // wave_rank64: number of lanes with a smaller key
        const uint32_t* rk = reinterpret_cast<const uint32_t*>(out.data() + (size_t)rounds * 4) + (size_t)r * 64;
        for (int l = 0; l < 64; l++) {
            const uint32_t k = (uint32_t)(in[(size_t)r * 64 + l] >> 7);
            uint32_t c = 0;
            for (int m = 0; m < 64; m++) c += ((uint32_t)(in[(size_t)r * 64 + m] >> 7) < k) ? 1u : 0u;
            if (rk[l] != c) {
                bad++;
                break;
            }
        }
        // wave_rank96: the same for three-dword keys compared as (hi : lo : x); few distinct values per dword, so that
        // every dword decides some of the comparisons and many keys tie
        const uint32_t* rk3 = reinterpret_cast<const uint32_t*>(out.data() + (size_t)rounds * 4 + (size_t)rounds * 32) + (size_t)r * 64;
        auto k96 = [&](int l, uint32_t& hi, uint32_t& lo, uint32_t& x) {
            const uint64_t v = in[(size_t)r * 64 + l];
            hi = (uint32_t)(v >> 40) & 0x3u;
            lo = (uint32_t)v & 0x7u;
            x = (uint32_t)(v >> 9) & 0x3u;
        };
        for (int l = 0; l < 64; l++) {
            uint32_t h, lo, x, oh, ol, ox, c = 0;
            k96(l, h, lo, x);
            for (int m = 0; m < 64; m++) {
                k96(m, oh, ol, ox);
                c += (oh < h || (oh == h && (ol < lo || (ol == lo && ox < x)))) ? 1u : 0u;
            }
            if (rk3[l] != c) {
                bad++;
                break;
            }
        }
    }
    *mismatches = bad;
    return FXJPS_OK;
}

int fxjps_selftest_openlist(fxjps_t* h, int32_t banded, int32_t far_cap, int32_t near_max, double delta0, const uint64_t* keys_f,
                            const uint32_t* keys_x, int64_t nkeys, const uint32_t* step_pops, const uint32_t* step_off, int32_t nsteps,
                            uint64_t* out_f, uint32_t* out_x, uint32_t* out_slot, uint32_t* out_k, uint32_t* out_info) {
    if (!h || !keys_f || !keys_x || !step_pops || !step_off || !out_f || !out_x || !out_slot || !out_k || !out_info || nkeys < 0 ||
        nkeys > (1 << 24) || nsteps < 0 || far_cap < 64 || far_cap > (1 << 24) || (far_cap & 7) || near_max < 1 || !(delta0 > 0.0))
        return fail(h, FXJPS_E_ARG, "bad selftest arguments");
    if (step_off[0] != 0u || (int64_t)step_off[nsteps] != nkeys) return fail(h, FXJPS_E_ARG, "step offsets do not cover the keys");
    for (int32_t i = 0; i < nsteps; i++)
        if (step_off[i + 1] < step_off[i] || step_off[i + 1] - step_off[i] > 64u) return fail(h, FXJPS_E_ARG, "a step pushes at most 64 keys");
    if (banded)  // (the ring reads the cell info of an entry from the map again: the test map is 64 x 64)
        for (int64_t i = 0; i < nkeys; i++)
            if ((keys_x[i] >> 17) >= 64u || ((keys_x[i] >> 4) & 0x1FFFu) >= 64u) return fail(h, FXJPS_E_ARG, "banded selftest: cells below 64 x 64");
    DevCtx& d = h->devs[0];
    HIPCHK(h, hipSetDevice(d.dev));
    const size_t nk = (size_t)std::max<int64_t>(nkeys, 1), ns = (size_t)std::max(nsteps, 1);
    const size_t far_n = (size_t)far_cap + (size_t)far_cap / 8;
    const size_t ci_n = (size_t)66 * 128;
    // one allocation: far tier | cell info | keys f | out f | keys x | out x | out slot | step pops | step offsets | out k | info
    size_t off = 0;
    auto take = [&](size_t bytes) { const size_t o = off; off += (bytes + 255) & ~(size_t)255; return o; };
    const size_t o_far = take(far_n * sizeof(FarEnt)), o_ci = take(ci_n * 2), o_kf = take(nk * 8), o_of = take(nk * 8), o_kx = take(nk * 4),
                 o_ox = take(nk * 4), o_os = take(nk * 4), o_sp = take(ns * 4), o_so = take((ns + 1) * 4), o_ok = take(ns * 4), o_in = take(32), o_cn = take(64 * 8);
    char* buf = nullptr;
    HIPCHK(h, hipMalloc((void**)&buf, off));
    hipError_t e = hipMemsetAsync(buf, 0, off, d.stream);
    if (e == hipSuccess && nkeys > 0) e = hipMemcpyAsync(buf + o_kf, keys_f, (size_t)nkeys * 8, hipMemcpyHostToDevice, d.stream);
    if (e == hipSuccess && nkeys > 0) e = hipMemcpyAsync(buf + o_kx, keys_x, (size_t)nkeys * 4, hipMemcpyHostToDevice, d.stream);
    if (e == hipSuccess && nsteps > 0) e = hipMemcpyAsync(buf + o_sp, step_pops, (size_t)nsteps * 4, hipMemcpyHostToDevice, d.stream);
    if (e == hipSuccess) e = hipMemcpyAsync(buf + o_so, step_off, ((size_t)nsteps + 1) * 4, hipMemcpyHostToDevice, d.stream);
    if (e == hipSuccess) {
        SearchArgs A{};
        A.G.ci = reinterpret_cast<const uint16_t*>(buf + o_ci);
        A.G.NS = 128;
        A.far = reinterpret_cast<FarEnt*>(buf + o_far);
        A.far_cap = (uint32_t)far_cap;
        A.near_max = (uint32_t)near_max;
        A.banded = banded ? 1u : 0u;
        A.out_counters = reinterpret_cast<unsigned long long*>(buf + o_cn);  // [2] far refills, [3] direct pops from the far tier
        auto kf = reinterpret_cast<const unsigned long long*>(buf + o_kf);
        auto of = reinterpret_cast<unsigned long long*>(buf + o_of);
        auto kx = reinterpret_cast<const uint32_t*>(buf + o_kx);
        auto ox = reinterpret_cast<uint32_t*>(buf + o_ox), os = reinterpret_cast<uint32_t*>(buf + o_os), ok = reinterpret_cast<uint32_t*>(buf + o_ok),
             in = reinterpret_cast<uint32_t*>(buf + o_in);
        auto sp = reinterpret_cast<const uint32_t*>(buf + o_sp), so = reinterpret_cast<const uint32_t*>(buf + o_so);
        if (banded)
            hipLaunchKernelGGL(fx::k_selftest_openlist<true>, dim3(1), dim3(64), 0, d.stream, A, kf, kx, sp, so, (uint32_t)nsteps, delta0, of, ox, os, ok, in, (uint32_t)nkeys);
        else
            hipLaunchKernelGGL(fx::k_selftest_openlist<false>, dim3(1), dim3(64), 0, d.stream, A, kf, kx, sp, so, (uint32_t)nsteps, delta0, of, ox, os, ok, in, (uint32_t)nkeys);
        e = hipGetLastError();
    }
    if (e == hipSuccess && nkeys > 0) e = hipMemcpyAsync(out_f, buf + o_of, (size_t)nkeys * 8, hipMemcpyDeviceToHost, d.stream);
    if (e == hipSuccess && nkeys > 0) e = hipMemcpyAsync(out_x, buf + o_ox, (size_t)nkeys * 4, hipMemcpyDeviceToHost, d.stream);
    if (e == hipSuccess && nkeys > 0) e = hipMemcpyAsync(out_slot, buf + o_os, (size_t)nkeys * 4, hipMemcpyDeviceToHost, d.stream);
    if (e == hipSuccess && nsteps > 0) e = hipMemcpyAsync(out_k, buf + o_ok, (size_t)nsteps * 4, hipMemcpyDeviceToHost, d.stream);
    unsigned long long cn[4] = {0, 0, 0, 0};
    uint32_t inf[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (e == hipSuccess) e = hipMemcpyAsync(inf, buf + o_in, sizeof(inf), hipMemcpyDeviceToHost, d.stream);
    if (e == hipSuccess) e = hipMemcpyAsync(cn, buf + o_cn, sizeof(cn), hipMemcpyDeviceToHost, d.stream);
    if (e == hipSuccess) e = hipStreamSynchronize(d.stream);
    (void)hipFree(buf);
    for (int i = 0; i < 8; i++) out_info[i] = inf[i];
    out_info[2] = (uint32_t)std::min<unsigned long long>(cn[2], 0xFFFFFFFFull);
    out_info[3] = (uint32_t)std::min<unsigned long long>(cn[3], 0xFFFFFFFFull);
    if (e != hipSuccess) return fail(h, FXJPS_E_HIP, "selftest: %s", hipGetErrorString(e));
    return FXJPS_OK;
}

namespace {
// which = 0 .. 5 of a grid's derived maps (fxjps_debug_read_maps, fxjps_debug_read_slot_maps)
int read_maps(fxjps_t* h, DevCtx& d, const GridBufs& g, int32_t which, void* buf, int64_t capacity_bytes, int64_t* out_bytes) {
    const void* src = nullptr;
    size_t bytes = 0;
    switch (which) {
        case 0: src = g.bm.p; bytes = (size_t)4 * g.LINES * g.WORDS * sizeof(fx::BmWord); break;  // scan words [4][LINES][WORDS] x {stop, occ}
        case 1: src = g.ci.p; bytes = (size_t)g.PW * g.NS * sizeof(uint16_t); break;               // cell infos [PW][NS] (columns >= PH unused)
        case 2: src = g.comp.p; bytes = (size_t)g.W * g.H * sizeof(int); break;                    // component forest [W][H]
        case 3: src = g.nb8.p; bytes = (size_t)g.PW * g.NS; break;                                 // neighbour bytes [PW][NS]
        case 4: src = g.bm.p + (size_t)4 * g.LINES * g.WORDS; bytes = (size_t)4 * (g.PW + g.PH - 1) * g.WORDS * sizeof(fx::BmWord); break;  // diagonal scan words
        case 5: src = g.jd.p; bytes = (size_t)g.PW * g.NS * 8 * sizeof(uint16_t); break;              // jump distances [PW][NS][8]
        default: return fail(h, FXJPS_E_ARG, "which must be 0 .. 5");
    }
    if (out_bytes) *out_bytes = (int64_t)bytes;
    if (!buf) return FXJPS_OK;
    if (capacity_bytes < (int64_t)bytes) return fail(h, FXJPS_E_ARG, "buffer holds %lld bytes, the map has %zu", (long long)capacity_bytes, bytes);
    HIPCHK(h, hipMemcpyAsync(buf, src, bytes, hipMemcpyDeviceToHost, d.stream));
    HIPCHK(h, hipStreamSynchronize(d.stream));
    return FXJPS_OK;
}
}  // namespace

int fxjps_debug_read_maps(fxjps_t* h, int32_t which, void* buf, int64_t capacity_bytes, int64_t* out_bytes) {
    if (!h) return FXJPS_E_ARG;
    if (!h->have_grid) return fail(h, FXJPS_E_NOGRID, "no grid");
    DevCtx& d = h->devs[0];
    HIPCHK(h, hipSetDevice(d.dev));
    if (h->maps_stale) {  // deferred cell updates: the maps follow the grid first
        int rc = update_cells_async(h, nullptr, nullptr, 0, true);
        if (rc) return rc;
    }
    return read_maps(h, d, d, which, buf, capacity_bytes, out_bytes);
}

int fxjps_debug_read_slot_maps(fxjps_t* h, int32_t slot, int32_t which, void* buf, int64_t capacity_bytes, int64_t* out_bytes) {
    if (!h) return FXJPS_E_ARG;
    if (!slot_in_use(h, slot)) return fail(h, FXJPS_E_ARG, "grid slot %d is empty or out of range", (int)slot);
    DevCtx& d = h->devs[0];
    HIPCHK(h, hipSetDevice(d.dev));
    return read_maps(h, d, d.slots[(size_t)slot], which, buf, capacity_bytes, out_bytes);
}

int fxjps_debug_read_slot_context(fxjps_t* h, int32_t context, int32_t slot, int32_t which, void* buf, int64_t capacity_bytes, int64_t* out_bytes) {
    if (!h) return FXJPS_E_ARG;
    if (context < 0 || (size_t)context >= h->devs.size()) return fail(h, FXJPS_E_ARG, "context %d is not in 0 .. %zu", (int)context, h->devs.size() - 1);
    if (!slot_in_use(h, slot)) return fail(h, FXJPS_E_ARG, "grid slot %d is empty or out of range", (int)slot);
    DevCtx& d = h->devs[(size_t)context];
    const GridBufs& g = d.slots[(size_t)slot];
    HIPCHK(h, hipSetDevice(d.dev));
    if (which != -1) return read_maps(h, d, g, which, buf, capacity_bytes, out_bytes);
    const size_t bytes = (size_t)g.W * g.H;  // the occupancy bytes [W][H]
    if (out_bytes) *out_bytes = (int64_t)bytes;
    if (!buf) return FXJPS_OK;
    if (capacity_bytes < (int64_t)bytes) return fail(h, FXJPS_E_ARG, "buffer holds %lld bytes, the grid has %zu", (long long)capacity_bytes, bytes);
    HIPCHK(h, hipMemcpyAsync(buf, g.occ.p, bytes, hipMemcpyDeviceToHost, d.stream));
    HIPCHK(h, hipStreamSynchronize(d.stream));
    return FXJPS_OK;
}


int fxjps_debug_read_nbmask(fxjps_t* h, uint8_t* buf) {
    if (!h || !buf) return FXJPS_E_ARG;
    if (!h->have_grid) return fail(h, FXJPS_E_NOGRID, "no grid");
    DevCtx& d = h->devs[0];
    HIPCHK(h, hipSetDevice(d.dev));
    if (h->maps_stale) {  // deferred cell updates: the maps follow the grid first
        int rc = update_cells_async(h, nullptr, nullptr, 0, true);
        if (rc) return rc;
    }
    HIPCHK(h, hipMemcpy2DAsync(buf, (size_t)d.PH, d.nb8.p, (size_t)d.NS, (size_t)d.PH, (size_t)d.PW, hipMemcpyDeviceToHost, d.stream));
    HIPCHK(h, hipStreamSynchronize(d.stream));
    return FXJPS_OK;
}

}  // extern "C"
