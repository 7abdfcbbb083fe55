// A thin C entry over fxjps_host_search.cpp for tests/test_host_search_host.py: every query of a batch on ONE Searcher
// per thread (so the generation tags of its visited table are exercised), threads pulling queries from an atomic counter.
#include <atomic>
#include <cstdint>
#include <thread>
#include <vector>

#include "../fuxi-planner_amd/csrc/fxjps_host_search.h"

extern "C" __attribute__((visibility("default"))) int fxh_plan_batch(
    const uint16_t* jd, const uint64_t* bm, const int32_t* comp, int32_t W, int32_t H, int32_t NS, int32_t LINES, int32_t WORDS,
    const int32_t* starts, const int32_t* goals, int64_t nq, int32_t hchoice, int32_t max_len, uint64_t max_pops, int32_t nthreads,
    int32_t* out_cells_xy, int32_t* out_len, double* out_cost, int64_t* out_pops, int64_t* out_pushes) {
    if ((int64_t)W * H > (1ll << 20) || (hchoice != 1 && hchoice != 2) || max_len < 0) return -1;
    fxh::Maps M;
    M.jd = jd;
    M.bm = reinterpret_cast<const fxh::BmWord*>(bm);
    M.comp = comp;
    M.W = W;
    M.H = H;
    M.NS = NS;
    M.LINES = LINES;
    M.WORDS = WORDS;
    std::vector<uint32_t> lut(11 * 256);
    fxh::dirlut_fill(lut.data());
    std::atomic<int64_t> next{0};
    auto work = [&]() {
        fxh::Searcher S;
        std::vector<uint32_t> path((size_t)max_len + 1);
        for (int64_t q = next.fetch_add(1); q < nq; q = next.fetch_add(1)) {
            const fxh::Result R = S.plan(M, lut.data(), hchoice, starts[2 * q], starts[2 * q + 1], goals[2 * q], goals[2 * q + 1], max_len,
                                         path.data(), max_pops);
            out_len[q] = R.len;
            out_cost[q] = R.cost;
            out_pops[q] = (int64_t)R.pops;
            out_pushes[q] = (int64_t)R.pushes;
            for (int32_t k = 0; k < R.len; k++) {
                out_cells_xy[((size_t)q * max_len + k) * 2] = (int32_t)(path[k] >> 16);
                out_cells_xy[((size_t)q * max_len + k) * 2 + 1] = (int32_t)(path[k] & 0xFFFFu);
            }
        }
    };
    std::vector<std::thread> th;
    for (int t = 1; t < nthreads; t++) th.emplace_back(work);
    work();
    for (auto& t : th) t.join();
    return 0;
}
