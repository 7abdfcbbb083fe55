// Stand-alone check of fuxi-planner_amd/csrc/fxjps_results.h (tests/test_result_assembly_host.py builds it with
// AddressSanitizer + UBSan): a streamed batch's lengths, bases and arena become CSR offsets and int32 pairs in query order.
// Every buffer is a std::vector of exactly the size the routine may touch, so a read or a write past an end is reported.
#include <cstdio>
#include <cstdlib>
#include <numeric>
#include <random>
#include <thread>
#include <vector>

#include "../fuxi-planner_amd/csrc/fxjps_results.h"

namespace {

int g_fail = 0;
#define CHECK(c)                                                      \
    do {                                                              \
        if (!(c)) {                                                   \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); \
            g_fail++;                                                 \
        }                                                             \
    } while (0)

const auto threads = [](size_t n, auto&& job) {
    std::vector<std::thread> th;
    for (size_t i = 0; i < n; i++) th.emplace_back([&job, i] { job(i); });
    for (auto& t : th) t.join();
};

// One batch: the lengths (codes among them), the pieces laid into the arena in the order `place`, and what the CSR must be.
struct Batch {
    std::vector<int32_t> len;
    std::vector<long long> base;
    std::vector<uint32_t> arena;
    std::vector<long long> want_off;
    std::vector<int32_t> want_xy;
    fx::StreamedResults R() const { return fx::StreamedResults{len.data(), base.data(), arena.data(), (int64_t)len.size()}; }
};

uint32_t cell_of(int64_t q, int32_t i) { return (uint32_t)(((q * 131 + i * 7) & 0x1FFF) << 16) | (uint32_t)((q * 17 + i * 3 + 1) & 0x1FFF); }

Batch make(const std::vector<int32_t>& len, const std::vector<size_t>& place, const std::vector<size_t>& overflowed = {}) {
    Batch b;
    b.len = len;
    b.base.assign(len.size(), -7);  // (a query without cells has no base: whatever stands there is never read as one)
    std::vector<char> ovf(len.size(), 0);
    for (size_t q : overflowed) ovf[q] = 1;
    for (size_t q : place) {
        if (len[q] <= 0) continue;
        if (ovf[q]) {
            b.base[q] = -1;
            continue;
        }
        b.base[q] = (long long)b.arena.size();
        for (int32_t i = 0; i < len[q]; i++) b.arena.push_back(cell_of((int64_t)q, i));
    }
    long long at = 0;
    for (size_t q = 0; q < len.size(); q++) {
        b.want_off.push_back(at);
        for (int32_t i = 0; i < len[q]; i++) {
            const uint32_t v = cell_of((int64_t)q, i);
            b.want_xy.push_back(ovf[q] ? -99 : (int32_t)(v >> 16));
            b.want_xy.push_back(ovf[q] ? -99 : (int32_t)(v & 0xFFFFu));
        }
        at += len[q] > 0 ? len[q] : 0;
    }
    b.want_off.push_back(at);
    return b;
}

// offsets and cells of the batch with 1, 3 and 8 threads: all equal to what is expected, and to each other
void check(const Batch& b, int64_t want_overflows) {
    const int64_t nq = (int64_t)b.len.size();
    std::vector<long long> off((size_t)nq + 1, -1);
    const long long total = fx::result_offsets(b.len.data(), nq, off.data());
    CHECK(off == b.want_off);
    CHECK(total == b.want_off.back());
    CHECK(fx::result_overflows(b.R(), 0, nq) == want_overflows);
    std::vector<int32_t> first;
    for (size_t nt : {(size_t)1, (size_t)3, (size_t)8}) {
        std::vector<int32_t> xy((size_t)total * 2, -99);
        fx::result_expand_split(b.R(), off.data(), xy.data(), nt, threads);
        CHECK(xy == b.want_xy);
        if (nt == 1) first = xy;
        CHECK(xy == first);
        CHECK(fx::result_bound(off.data(), nq, 0, nt) == 0);
        CHECK(fx::result_bound(off.data(), nq, nt, nt) == nq);
        for (size_t i = 0; i < nt; i++) CHECK(fx::result_bound(off.data(), nq, i, nt) <= fx::result_bound(off.data(), nq, i + 1, nt));
    }
}

}  // namespace

int main() {
    // zero lengths and negative status codes between paths, arena pieces in query order
    {
        const std::vector<int32_t> len = {3, 0, -1, 5, -2, -5, 0, 2, -1000000, 4};
        std::vector<size_t> place(len.size());
        std::iota(place.begin(), place.end(), (size_t)0);
        check(make(len, place), 0);
    }
    // ... and in an order unrelated to query order
    {
        const std::vector<int32_t> len = {3, 0, -1, 5, -2, 1, 0, 2, 64, 4, 65, 63};
        check(make(len, {11, 3, 0, 9, 7, 10, 5, 8, 1, 2, 4, 6}), 0);
    }
    // a length-1 path alone, first, and last; an empty batch; a batch without a single cell
    check(make({1}, {0}), 0);
    check(make({1, 7, 0}, {1, 0, 2}), 0);
    check(make({0, 7, 1}, {2, 1, 0}), 0);
    check(make({}, {}), 0);
    check(make({0, -1, -2, 0}, {0, 1, 2, 3}), 0);
    // max_len-long paths (every slot full), in reverse order of the queries
    {
        const int32_t max_len = 4096;
        check(make({max_len, max_len, 1, max_len}, {3, 2, 1, 0}), 0);
    }
    // many queries in a random order: the split by cells falls inside the batch at every thread count
    {
        std::mt19937 rng(20240611u);
        std::vector<int32_t> len(5000);
        for (auto& n : len) {
            const uint32_t r = rng() % 10u;
            n = r == 0 ? 0 : r == 1 ? -1 - (int32_t)(rng() % 5u) : 1 + (int32_t)(rng() % 300u);
        }
        std::vector<size_t> place(len.size());
        std::iota(place.begin(), place.end(), (size_t)0);
        std::shuffle(place.begin(), place.end(), rng);
        check(make(len, place), 0);
        // overflow marks are reported and not read: those queries have no cells in the arena at all (a read of the arena
        // under a base of -1 lies in front of it), and their pairs stay as they were
        std::vector<size_t> ovf;
        int64_t n_ovf = 0;
        for (size_t q = 0; q < len.size(); q += 7) {
            ovf.push_back(q);
            n_ovf += len[q] > 0 ? 1 : 0;
        }
        check(make(len, place, ovf), n_ovf);
    }
    // an arena that holds nothing: every path overflowed
    check(make({2, 3, 0, 1}, {0, 1, 2, 3}, {0, 1, 3}), 3);
    CHECK(fx::result_threads(0) == 1 && fx::result_threads(1000) == 1 && fx::result_threads(2900000) == 8 && fx::result_threads(1ll << 40) == 8);
    if (g_fail) return 1;
    std::printf("result assembly ok\n");
    return 0;
}
