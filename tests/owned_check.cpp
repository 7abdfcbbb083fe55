// owned_check.cpp -- the owners of fuxi-planner_amd/csrc/fxjps_owned.h alone, as plain host code: malloc / free and a counting
// destroy function stand in for the runtime's calls.  tests/test_owned_host.py builds it with -fsanitize=address,undefined
// and runs it; a double free, a leak or a use after a move ends it there, a broken count here.
#include <cstdio>
#include <cstdlib>
#include <set>
#include <utility>
#include <vector>

#include "../fuxi-planner_amd/csrc/fxjps_owned.h"

namespace {

int g_fail = 0;
#define CHECK(c)                                                        \
    do {                                                                \
        if (!(c)) {                                                     \
            fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c);     \
            g_fail++;                                                   \
        }                                                               \
    } while (0)

std::set<void*> g_open;          // allocations handed out and not yet freed
int g_allocs = 0, g_frees = 0, g_bad_frees = 0;
int g_refuse = 0;                // the next g_refuse allocations fail
std::atomic<int64_t> g_live{0};

struct FakeMem {
    using error = int;
    static constexpr int ok = 0;
    static int alloc(void** p, size_t bytes) {
        if (g_refuse > 0) {
            g_refuse--;
            return 2;
        }
        *p = malloc(bytes);
        g_open.insert(*p);
        g_allocs++;
        return 0;
    }
    static void free(void* p) {
        if (g_open.erase(p) != 1) g_bad_frees++;  // freed twice, or never allocated
        else ::free(p);
        g_frees++;
    }
    static std::atomic<int64_t>& live() { return g_live; }
};
using Buf = fx::OwnedBuf<double, FakeMem>;

std::multiset<int*> g_res_open;
int g_created = 0, g_destroyed = 0, g_bad_destroys = 0;
struct FakeRes {
    using type = int*;
    static int create(int** h, unsigned flags) {
        if (flags == 99u) {
            *h = nullptr;
            return 2;
        }
        *h = new int((int)flags);
        g_res_open.insert(*h);
        g_created++;
        return 0;
    }
    static void destroy(int* h) {
        auto it = g_res_open.find(h);
        if (it == g_res_open.end()) {
            g_bad_destroys++;
        } else {
            g_res_open.erase(it);
            delete h;
        }
        g_destroyed++;
    }
};
using Res = fx::Owned<FakeRes>;

struct Ctx {  // a context in small: holders side by side, in a vector that is resized
    Res stream;
    Buf a, b;
    Res ev;
};

void check_bufs() {
    {
        Buf x;
        CHECK(x.p == nullptr && x.cap == 0);
        CHECK(x.ensure(100) == 0);
        CHECK(x.p != nullptr && x.cap == 100 + 100 / 8 + 64);
        CHECK(g_live.load() == (int64_t)(x.cap * sizeof(double)));
        double* const p0 = x.p;
        CHECK(x.ensure(x.cap) == 0 && x.p == p0);  // the fast path: nothing moves
        for (size_t i = 0; i < x.cap; i++) x.p[i] = (double)i;
        CHECK(x.ensure(1000) == 0);  // growing: the old block is freed first
        CHECK(x.cap == 1000 + 125 + 64 && g_allocs == 2 && g_frees == 1);
        CHECK(g_live.load() == (int64_t)(x.cap * sizeof(double)));

        g_refuse = 1;  // a refused allocation leaves the buffer empty, and the next one works again
        CHECK(x.ensure(5000) != 0);
        CHECK(x.p == nullptr && x.cap == 0 && g_live.load() == 0);
        CHECK(x.ensure(10) == 0 && x.cap == 10 + 1 + 64);

        Buf y(std::move(x));  // move construction nulls the source
        CHECK(x.p == nullptr && x.cap == 0 && y.cap == 75);
        Buf z;
        CHECK(z.ensure(7) == 0);
        z = std::move(y);  // move assignment frees what the target held
        CHECK(y.p == nullptr && y.cap == 0 && z.cap == 75);
        Buf& zr = z;
        z = std::move(zr);  // self-assignment keeps it
        CHECK(z.p != nullptr && z.cap == 75);
        z.p[74] = 1.0;

        Buf w;
        CHECK(w.ensure(300) == 0);
        double *pz = z.p, *pw = w.p;
        std::swap(z, w);
        CHECK(z.p == pw && w.p == pz && w.cap == 75 && z.cap == 300 + 37 + 64);
        std::swap(w, x);  // with an empty one
        CHECK(w.p == nullptr && x.p == pz);
        w.release();  // releasing an empty buffer is nothing
        x.release();
        CHECK(x.p == nullptr && x.cap == 0);
        CHECK(g_live.load() == (int64_t)(z.cap * sizeof(double)));
    }
    CHECK(g_open.empty() && g_live.load() == 0 && g_allocs == g_frees && g_bad_frees == 0);
}

void check_handles() {
    {
        Res r;
        CHECK((int*)r == nullptr && !r);
        CHECK(r.create(99u) != 0 && (int*)r == nullptr);  // a failed create leaves it empty
        CHECK(r.create(3u) == 0 && *r.h == 3);
        int* const h0 = r;
        Res s(std::move(r));
        CHECK(r.h == nullptr && s.h == h0);
        Res t;
        CHECK(t.create(4u) == 0);
        t = std::move(s);
        CHECK(s.h == nullptr && t.h == h0 && g_destroyed == 1);
        Res& tr = t;
        t = std::move(tr);
        CHECK(t.h == h0);
        std::swap(t, r);
        CHECK(r.h == h0 && t.h == nullptr);
    }
    CHECK(g_res_open.empty() && g_created == g_destroyed && g_bad_destroys == 0);
}

void check_vector() {
    {
        std::vector<Ctx> v;
        v.resize(3);
        for (size_t i = 0; i < v.size(); i++) {
            CHECK(v[i].stream.create(1u) == 0 && v[i].ev.create(2u) == 0);
            CHECK(v[i].a.ensure(10 * (i + 1)) == 0);
        }
        double* const p1 = v[1].a.p;
        v.resize(40);  // reallocates: the live contexts are moved, their sources destroyed empty
        CHECK(v[1].a.p == p1 && v[39].a.p == nullptr);
        CHECK(v[39].b.ensure(5) == 0);
        v.resize(2);  // destroys contexts 2 .. 39
        CHECK(g_open.size() == 2 && g_res_open.size() == 4);
        v[0] = Ctx();  // how a grid slot is emptied
        CHECK(g_open.size() == 1 && g_res_open.size() == 2);
    }
    CHECK(g_open.empty() && g_res_open.empty() && g_live.load() == 0);
    CHECK(g_allocs == g_frees && g_created == g_destroyed && g_bad_frees == 0 && g_bad_destroys == 0);
}

}  // namespace

int main() {
    check_bufs();
    check_handles();
    check_vector();
    if (g_fail) return 1;
    printf("owned ok: %d allocations, %d handles\n", g_allocs, g_created);
    return 0;
}
