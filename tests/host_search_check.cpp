// Stand-alone check of the host search (fuxi-planner_amd/csrc/fxjps_host_search.cpp) under AddressSanitizer + UBSan:
// built and run as a program by tests/test_host_search_host.py, on a map file that test writes.  Two threads pull the
// queries of each grid from an atomic counter, each on its own Searcher (one visited table across grids of different
// shapes), and every result must equal the one recorded in the file (the test writes the C oracle's answers there).
//
// File: per grid, int32 {W, H, NS, LINES, WORDS, nq, hchoice, max_len}, then jd u16[(W+2) * NS * 8], bm u64[4 * LINES *
// WORDS * 2], comp i32[W * H], starts i32[nq * 2], goals i32[nq * 2], len i32[nq], cost f64[nq], pops i64[nq], pushes
// i64[nq], cells u32[nq * max_len] (x << 16 | y, 0 behind the path).
#include <atomic>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <thread>
#include <vector>

#include "../fuxi-planner_amd/csrc/fxjps_host_search.h"

namespace {

template <typename T>
bool take(const std::vector<uint8_t>& buf, size_t& at, size_t n, std::vector<T>& out) {
    if (n > (buf.size() - at) / sizeof(T)) return false;
    out.resize(n);
    if (n) std::memcpy(out.data(), buf.data() + at, n * sizeof(T));
    at += n * sizeof(T);
    return true;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    std::vector<uint8_t> buf;
    uint8_t chunk[1 << 16];
    for (size_t n; (n = std::fread(chunk, 1, sizeof chunk, f)) > 0;) buf.insert(buf.end(), chunk, chunk + n);
    std::fclose(f);

    std::vector<uint32_t> lut(11 * 256);
    fxh::dirlut_fill(lut.data());
    fxh::Searcher searchers[2];
    size_t at = 0;
    long grids = 0, queries = 0;
    while (at < buf.size()) {
        std::vector<int32_t> head, comp, starts, goals, len;
        std::vector<uint16_t> jd;
        std::vector<uint64_t> bm;
        std::vector<double> cost;
        std::vector<int64_t> pops, pushes;
        std::vector<uint32_t> cells;
        if (!take(buf, at, 8, head)) return 3;
        const int W = head[0], H = head[1], NS = head[2], LINES = head[3], WORDS = head[4], nq = head[5], hchoice = head[6], max_len = head[7];
        if (W < 1 || H < 1 || (long long)W * H > (1ll << 20) || NS < H + 2 || nq < 0 || max_len < 1) return 3;
        if (!take(buf, at, (size_t)(W + 2) * NS * 8, jd) || !take(buf, at, (size_t)4 * LINES * WORDS * 2, bm) || !take(buf, at, (size_t)W * H, comp) ||
            !take(buf, at, (size_t)nq * 2, starts) || !take(buf, at, (size_t)nq * 2, goals) || !take(buf, at, (size_t)nq, len) ||
            !take(buf, at, (size_t)nq, cost) || !take(buf, at, (size_t)nq, pops) || !take(buf, at, (size_t)nq, pushes) ||
            !take(buf, at, (size_t)nq * max_len, cells))
            return 3;
        fxh::Maps M;
        M.jd = jd.data();
        M.bm = reinterpret_cast<const fxh::BmWord*>(bm.data());
        M.comp = comp.data();
        M.W = W;
        M.H = H;
        M.NS = NS;
        M.LINES = LINES;
        M.WORDS = WORDS;
        std::atomic<int> next{0}, bad{0};
        auto work = [&](int t) {
            std::vector<uint32_t> path((size_t)max_len);  // exactly the slot: a store past it is an ASan report
            for (int q = next.fetch_add(1); q < nq; q = next.fetch_add(1)) {
                const fxh::Result R = searchers[t].plan(M, lut.data(), hchoice, starts[2 * q], starts[2 * q + 1], goals[2 * q], goals[2 * q + 1],
                                                        max_len, path.data(), 64ull * (uint64_t)W * (uint64_t)H + 4096ull);
                bool ok = R.len == len[q] && std::memcmp(&R.cost, &cost[q], 8) == 0 && (int64_t)R.pops == pops[q] && (int64_t)R.pushes == pushes[q];
                for (int k = 0; ok && k < R.len; k++) ok = path[k] == cells[(size_t)q * max_len + k];
                if (!ok) {
                    if (bad.fetch_add(1) == 0)
                        std::fprintf(stderr, "grid %ld query %d (%d,%d)->(%d,%d): len %d, expected %d\n", grids, q, starts[2 * q], starts[2 * q + 1],
                                     goals[2 * q], goals[2 * q + 1], R.len, len[q]);
                }
            }
        };
        std::thread other(work, 1);
        work(0);
        other.join();
        if (bad.load() != 0) return 1;
        grids++;
        queries += nq;
    }
    std::printf("HOST-SEARCH-CHECK-OK %ld grids %ld queries\n", grids, queries);
    return 0;
}
