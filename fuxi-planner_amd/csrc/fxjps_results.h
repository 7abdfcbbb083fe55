// fxjps_results.h -- a streamed batch's results on the host (fxjps.hip).  The search kernel leaves each
// query's path in a pinned arena as packed cells (x << 16 | y, the format of its path slots), wherever the arena's cursor
// stood when the query finished, and the place in `base`; here the lengths become CSR offsets and the pieces become int32
// pairs in query order.  Plain C++ without a runtime call: fxjps.hip passes the handle's pinned buffers and its thread
// runner, tests/result_assembly_check.cpp vectors and std::thread.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>

namespace fx {

// What the kernel left: per query its length (> 0: cells; otherwise a status code) and, for a positive length, where its
// cells begin in the arena (< 0: they did not fit -- the arena holds nothing of that query).
struct StreamedResults {
    const int32_t* len = nullptr;
    const long long* base = nullptr;
    const uint32_t* arena = nullptr;
    int64_t nq = 0;
};

// offsets[0 .. nq]: the exclusive prefix sum of max(len, 0).  Returns the total.
inline long long result_offsets(const int32_t* len, int64_t nq, long long* offsets) {
    long long at = 0;
    for (int64_t q = 0; q < nq; q++) {
        offsets[q] = at;
        at += len[q] > 0 ? len[q] : 0;
    }
    offsets[nq] = at;
    return at;
}

// Queries of [q_lo, q_hi) whose cells the arena does not hold (a positive length under an overflow mark).  Only lengths
// and bases are read.
inline int64_t result_overflows(const StreamedResults& R, int64_t q_lo, int64_t q_hi) {
    int64_t n = 0;
    for (int64_t q = q_lo; q < q_hi; q++) n += (R.len[q] > 0 && R.base[q] < 0) ? 1 : 0;
    return n;
}

// The cells of queries [q_lo, q_hi) as int32 pairs: query q's begin at out_xy + 2 * offsets[q].  A query under
// an overflow mark is skipped (its pairs stay as they were); the caller has asked result_overflows first.
inline void result_expand(const StreamedResults& R, const long long* offsets, int64_t q_lo, int64_t q_hi, int32_t* out_xy) {
    for (int64_t q = q_lo; q < q_hi; q++) {
        const int32_t n = R.len[q];
        if (n <= 0 || R.base[q] < 0) continue;
        const uint32_t* src = R.arena + R.base[q];
        int32_t* dst = out_xy + 2 * offsets[q];
        for (int32_t i = 0; i < n; i++) {
            const uint32_t v = src[i];
            dst[2 * i] = (int32_t)(v >> 16);
            dst[2 * i + 1] = (int32_t)(v & 0xFFFFu);
        }
    }
}

// How many threads an expansion of `total` cells is worth (host_copy's rule: 2 MB of output a thread, eight at the most).
inline size_t result_threads(long long total) { return (size_t)std::min<long long>(8, std::max<long long>(1, total * 8 / (2 << 20))); }

// Where thread i of nt begins: the first query whose offset reaches its share of the cells (bound[0] = 0, bound[nt] = nq).
inline int64_t result_bound(const long long* offsets, int64_t nq, size_t i, size_t nt) {
    if (i == 0) return 0;
    if (i >= nt) return nq;
    const long long want = offsets[nq] / (long long)nt * (long long)i;
    return (int64_t)(std::lower_bound(offsets, offsets + nq, want) - offsets);
}

// result_expand of all queries over nt threads by query ranges.  par(n, job) runs job(0) .. job(n - 1), in any order or
// at once, and returns when all are done; the ranges are disjoint in queries and so in the pairs they write.
template <typename Par>
void result_expand_split(const StreamedResults& R, const long long* offsets, int32_t* out_xy, size_t nt, Par&& par) {
    if (nt < 2) {
        result_expand(R, offsets, 0, R.nq, out_xy);
        return;
    }
    par(nt, [&R, offsets, out_xy, nt](size_t i) {
        result_expand(R, offsets, result_bound(offsets, R.nq, i, nt), result_bound(offsets, R.nq, i + 1, nt), out_xy);
    });
}

}  // namespace fx
