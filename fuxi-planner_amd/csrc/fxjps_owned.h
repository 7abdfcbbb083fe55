// fxjps_owned.h -- the move-only owners of everything a handle allocates (fxjps.hip): what one of them holds is given
// back when it is destroyed, so a member of DevCtx needs no line in any teardown list.  Plain C++ over a policy type that
// names the runtime's calls: fxjps.hip passes HIP's, tests/owned_check.cpp malloc / free and counting stand-ins.
#pragma once
#include <atomic>
#include <cstddef>
#include <cstdint>

namespace fx {

// Grow-only buffer of T.  M: `error` and its `ok` value, alloc(void**, bytes) -> error, free(void*), and live(), the
// counter of bytes that buffers of this kind hold (fxjps_debug_live_bytes) -- touched only where memory changes hands.
template <typename T, typename M>
struct OwnedBuf {
    T* p = nullptr;
    size_t cap = 0;
    OwnedBuf() = default;
    OwnedBuf(const OwnedBuf&) = delete;
    OwnedBuf& operator=(const OwnedBuf&) = delete;
    OwnedBuf(OwnedBuf&& o) noexcept : p(o.p), cap(o.cap) {
        o.p = nullptr;
        o.cap = 0;
    }
    OwnedBuf& operator=(OwnedBuf&& o) noexcept {
        if (this != &o) {
            release();
            p = o.p;
            cap = o.cap;
            o.p = nullptr;
            o.cap = 0;
        }
        return *this;
    }
    ~OwnedBuf() { release(); }
    typename M::error ensure(size_t n) {
        if (n <= cap) return M::ok;
        release();
        size_t want = n + n / 8 + 64;
        typename M::error e = M::alloc((void**)&p, want * sizeof(T));
        if (e == M::ok) {
            cap = want;
            M::live() += (int64_t)(want * sizeof(T));
        }
        return e;
    }
    void release() {
        if (p) {
            M::free(p);
            M::live() -= (int64_t)(cap * sizeof(T));
        }
        p = nullptr;
        cap = 0;
    }
};

// One runtime object (a stream, an event, the mapped counter word).  R: `type` (a pointer), create(type*, flags) -> error
// (which leaves a null handle when it fails), destroy(type).  Reads as the plain handle wherever one is expected.
template <typename R>
struct Owned {
    typename R::type h = nullptr;
    Owned() = default;
    Owned(const Owned&) = delete;
    Owned& operator=(const Owned&) = delete;
    Owned(Owned&& o) noexcept : h(o.h) { o.h = nullptr; }
    Owned& operator=(Owned&& o) noexcept {
        if (this != &o) {
            reset();
            h = o.h;
            o.h = nullptr;
        }
        return *this;
    }
    ~Owned() { reset(); }
    auto create(unsigned flags) {
        reset();
        return R::create(&h, flags);
    }
    void reset() {
        if (h) R::destroy(h);
        h = nullptr;
    }
    operator typename R::type() const { return h; }
};

}  // namespace fx
