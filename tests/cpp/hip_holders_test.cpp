// Unit test of the resource owners of csrc/hip_host.hpp (HostBuf, Event, Stream, and DevBuf's ensure) on the host,
// built with the address and undefined-behaviour sanitizers.  It is meant to run with no device visible: every create
// then fails, and a failed create must leave the owner empty.  Where a device answers after all, the same sequence runs
// on real resources.  Either way: moves leave the source empty, release twice is harmless, "make if absent" twice
// makes once, a never-created owner destroys clean.  Prints "ok" and exits 0, or says what failed.
#include <cstdio>
#include <utility>
#include <vector>

#include "../../myldpccppapi_amd/csrc/hip_host.hpp"

#define CHECK(c) do { if (!(c)) { printf("FAILED: %s (line %d)\n", #c, __LINE__); return 1; } } while (0)

// hip_host.hpp only declares these (the library defines them); nothing here reports through them
int ldpc::set_error(int code, const char *, ...) { return code; }

namespace {

// what the four owners have in common, behind one set of names
struct PinnedOps {
    using T = ldpc::HostBuf<int32_t>;
    static hipError_t make(T &h) { return h.alloc(16); }
    static hipError_t ensure(T &h) { return h.ensure(16); }
    static const void *get(const T &h) { return h.p; }
    static bool sized(const T &h) { return h.n == (h.p ? 16u : 0u); }
};
struct DeviceOps {
    using T = ldpc::DevBuf<int32_t>;
    static hipError_t make(T &h) { return h.alloc(16); }
    static hipError_t ensure(T &h) { return h.ensure(16); }
    static const void *get(const T &h) { return h.p; }
    static bool sized(const T &) { return true; }       // DevBuf keeps the requested count: not this test's subject
};
template <bool TIMED> struct EventOps {
    using T = ldpc::Event;
    static hipError_t make(T &h) { return h.create(TIMED); }
    static hipError_t ensure(T &h) { return h.ensure(TIMED); }
    static const void *get(const T &h) { return h.e; }
    static bool sized(const T &) { return true; }
};
struct StreamOps {
    using T = ldpc::Stream;
    static hipError_t make(T &h) { return h.create(); }
    static hipError_t ensure(T &h) { return h.ensure(); }
    static const void *get(const T &h) { return h.s; }
    static bool sized(const T &) { return true; }
};

int g_made = 0, g_failed = 0;

template <typename Ops> int exercise(const char *what)
{
    using T = typename Ops::T;
    {   // never created
        T a;
        CHECK(Ops::get(a) == nullptr);
        a.release();
        a.release();
    }
    T a;
    const hipError_t e = Ops::make(a);
    (void)hipGetLastError();
    const bool have = e == hipSuccess;
    ++(have ? g_made : g_failed);
    // a failed create leaves the owner empty; a good one fills it
    CHECK(have == (Ops::get(a) != nullptr));
    CHECK(Ops::sized(a));
    // make if absent, twice: the second call keeps what the first made
    T b;
    const hipError_t e1 = Ops::ensure(b);
    (void)hipGetLastError();
    const void *first = Ops::get(b);
    CHECK((e1 == hipSuccess) == (first != nullptr));
    const hipError_t e2 = Ops::ensure(b);
    (void)hipGetLastError();
    if (first) CHECK(e2 == hipSuccess && Ops::get(b) == first);
    else CHECK((e2 == hipSuccess) == (Ops::get(b) != nullptr));
    // move construction and move assignment: the source is empty afterwards, the target holds what it held
    const void *pa = Ops::get(a);
    T c(std::move(a));
    CHECK(Ops::get(a) == nullptr && Ops::get(c) == pa);
    T d;
    d = std::move(c);
    CHECK(Ops::get(c) == nullptr && Ops::get(d) == pa);
    d = std::move(b);                      // releases what d held, takes b's
    CHECK(Ops::get(b) == nullptr);
    const void *pd = Ops::get(d);
    T &self = d;
    d = std::move(self);                   // self-assignment keeps it
    CHECK(Ops::get(d) == pd);
    // owners in a growing vector: what TimedSpan and RingChunk do
    std::vector<T> v;
    for (int i = 0; i < 9; ++i) {
        T t;
        (void)Ops::make(t);
        (void)hipGetLastError();
        v.push_back(std::move(t));
    }
    // release twice, then let the destructors run on released, moved-from and live owners alike
    d.release();
    CHECK(Ops::get(d) == nullptr && Ops::sized(d));
    d.release();
    a.release();
    printf("%s: %s\n", what, have ? "created" : "create refused, owner left empty");
    return 0;
}

}  // namespace

int main()
{
    if (exercise<PinnedOps>("HostBuf")) return 1;
    if (exercise<DeviceOps>("DevBuf")) return 1;
    if (exercise<EventOps<true>>("Event")) return 1;
    if (exercise<EventOps<false>>("Event (no timing)")) return 1;
    if (exercise<StreamOps>("Stream")) return 1;
    printf("%d created, %d refused\nok\n", g_made, g_failed);
    return 0;
}
