// Stand-alone host test of rs::DevBuf / rs::PinnedBuf, rs::Stream / rs::Event and rs::grown
// (rs_common.h) and of the idioms the handles write with them: group growth, lazily created
// stream groups, the event pool, a create's failure exit.  It links its own definitions of the
// four allocation functions and of the four stream and event functions -- malloc-backed,
// counting live blocks, able to refuse the k-th call -- in place of rs_common.cpp, so it needs
// no GPU; tests/test_host_buffers.py builds it with -fsanitize=address,undefined and runs it.
// Exit status 0: every check held.
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "rs_common.h"

namespace {

int g_live = 0;       // blocks, streams and events created and not yet released
int g_allocs = 0;     // allocation and creation calls so far
int g_frees = 0;      // release calls so far
int g_fail_at = -1;   // the allocation or creation call (0-based, counted from arm()) to refuse
int g_checks = 0, g_failed = 0;
char g_error[256] = {0};

void arm(int k) { g_allocs = 0; g_fail_at = k; }

hipError_t test_alloc(void** ptr, size_t bytes) {
    *ptr = nullptr;
    if (g_allocs++ == g_fail_at) return hipErrorOutOfMemory;
    *ptr = std::malloc(bytes ? bytes : 1);
    std::memset(*ptr, 0xA5, bytes);   // the whole block is writable
    ++g_live;
    return hipSuccess;
}

hipError_t test_free(void* ptr) {
    std::free(ptr);   // (a second release of one block is the sanitizer's to report)
    --g_live;
    ++g_frees;
    return hipSuccess;
}

// A stream or an event: a one-byte block behind the opaque pointer, through the same counters.
template <class T>
hipError_t test_create(T* obj) {
    void* p = nullptr;
    const hipError_t e = test_alloc(&p, 1);
    *obj = static_cast<T>(p);
    return e == hipSuccess ? hipSuccess : hipErrorInvalidValue;
}

#define CHECK(cond)                                                        \
    do {                                                                   \
        ++g_checks;                                                        \
        if (!(cond)) {                                                     \
            ++g_failed;                                                    \
            std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); \
        }                                                                  \
    } while (0)

}  // namespace

namespace rs {

void set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_error, sizeof(g_error), fmt, ap);
    va_end(ap);
}
void clear_error() { g_error[0] = 0; }

hipError_t dev_alloc(void** ptr, size_t bytes) { return test_alloc(ptr, bytes); }
hipError_t dev_free(void* ptr) { return test_free(ptr); }
hipError_t pinned_alloc(void** ptr, void** dev, size_t bytes, unsigned) {
    const hipError_t e = test_alloc(ptr, bytes);
    *dev = *ptr;
    return e;
}
hipError_t pinned_free(void* ptr) { return test_free(ptr); }

hipError_t stream_create(hipStream_t* s) { return test_create(s); }
hipError_t stream_destroy(hipStream_t s) { return test_free(s); }
hipError_t event_create(hipEvent_t* e, unsigned) { return test_create(e); }
hipError_t event_destroy(hipEvent_t e) { return test_free(e); }

}  // namespace rs

// HIP's error text: the one HIP symbol the header's failure path refers to.
extern "C" const char* hipGetErrorString(hipError_t e) {
    return e == hipErrorOutOfMemory ? "out of memory" : "error";
}

namespace {

// A group of buffers under one capacity, grown the way the handles grow theirs: the
// capacity is zero from before the first buffer is touched until the last has succeeded.
struct Group {
    int cap = 0;
    rs::DevBuf<uint32_t> a;
    rs::PinnedBuf<unsigned long long> b;
    rs::DevBuf<void> c;
    rs::DevBuf<uint8_t> d;
};
constexpr int GROUP_BUFS = 4;

int grow(Group* g, int n) {
    if (n <= g->cap) return RS_OK;
    const int cap = rs::grown(g->cap, n, 16);
    g->cap = 0;
    RS_TRY(g->a.reserve((size_t)cap));
    RS_TRY(g->b.reserve((size_t)cap, hipHostMallocDefault));
    RS_TRY(g->c.reserve(3 * (size_t)cap));
    RS_TRY(g->d.reserve(64 * (size_t)cap));
    g->cap = cap;
    return RS_OK;
}

void check_group(const Group& g) {   // a non-zero capacity: every buffer holds that much
    if (g.cap == 0) return;
    CHECK(g.a.get() && g.a.capacity() >= (size_t)g.cap);
    CHECK(g.b.get() && g.b.dev() && g.b.capacity() >= (size_t)g.cap);
    CHECK(g.c.get() && g.c.capacity() >= 3 * (size_t)g.cap);
    CHECK(g.d.get() && g.d.capacity() >= 64 * (size_t)g.cap);
    g.a.get()[g.cap - 1] = 1u;       // the last element is the block's (the sanitizer checks)
    g.b.get()[g.cap - 1] = 1ull;
    g.d.get()[64 * (size_t)g.cap - 1] = 1;
}

void test_reserve() {
    arm(-1);
    rs::DevBuf<uint32_t> b;
    CHECK(b.get() == nullptr && b.capacity() == 0);
    CHECK(b.reserve(100) == RS_OK && b.get() && b.capacity() == 100 && g_live == 1);
    uint32_t* const p = b.get();
    const int allocs = g_allocs;
    CHECK(b.reserve(100) == RS_OK && b.reserve(1) == RS_OK && b.reserve(0) == RS_OK);
    CHECK(g_allocs == allocs && b.get() == p && b.capacity() == 100);   // within capacity: nothing
    CHECK(b.reserve(101) == RS_OK && b.capacity() == 101 && g_live == 1);  // exactly n, old block gone
    b.reset();
    CHECK(b.get() == nullptr && b.capacity() == 0 && g_live == 0);
    b.reset();
    CHECK(g_live == 0);

    rs::DevBuf<void> v;   // untyped: bytes
    CHECK(v.reserve(7) == RS_OK && v.capacity() == 7);
    static_cast<char*>(v.get())[6] = 0;

    rs::PinnedBuf<double> h;
    CHECK(h.reserve(8, hipHostMallocMapped | hipHostMallocCoherent) == RS_OK);
    CHECK(h.get() && h.dev() == h.get() && h.capacity() == 8 && g_live == 2);
    h.get()[7] = 1.0;
    h.reset();
    CHECK(h.get() == nullptr && h.dev() == nullptr && h.capacity() == 0 && g_live == 1);
}

void test_failed_reserve() {
    rs::DevBuf<uint64_t> b;
    rs::PinnedBuf<uint8_t> h;
    arm(-1);
    CHECK(b.reserve(10) == RS_OK && h.reserve(10, hipHostMallocDefault) == RS_OK && g_live == 2);
    arm(0);
    rs::clear_error();
    CHECK(b.reserve(20, "test buffer") == RS_ERR_NOMEM);
    CHECK(b.get() == nullptr && b.capacity() == 0 && g_live == 1);   // the old block went first
    CHECK(std::strstr(g_error, "test buffer") && std::strstr(g_error, "out of memory"));
    arm(0);
    CHECK(h.reserve(20, hipHostMallocDefault) == RS_ERR_NOMEM);
    CHECK(h.get() == nullptr && h.dev() == nullptr && h.capacity() == 0 && g_live == 0);
    arm(-1);
    CHECK(b.reserve(20) == RS_OK && b.capacity() == 20 && g_live == 1);   // and grows again
}

void test_group_growth() {
    for (int first = 0; first < 2; ++first)          // from empty, and from a grown group
        for (int k = 0; k < GROUP_BUFS; ++k) {
            Group g;
            arm(-1);
            if (first) {
                CHECK(grow(&g, 20) == RS_OK && g.cap == 32);
                check_group(g);
            }
            const int want = first ? 70 : 20;
            arm(k);
            CHECK(grow(&g, want) == RS_ERR_NOMEM);
            CHECK(g.cap == 0);
            // no member points at a released block: each is empty or holds what it says
            CHECK((g.a.get() == nullptr) == (g.a.capacity() == 0));
            CHECK((g.b.get() == nullptr) == (g.b.capacity() == 0));
            CHECK((g.c.get() == nullptr) == (g.c.capacity() == 0));
            CHECK((g.d.get() == nullptr) == (g.d.capacity() == 0));
            int held = 0;
            for (const bool has : {g.a.get() != nullptr, g.b.get() != nullptr, g.c.get() != nullptr,
                                   g.d.get() != nullptr})
                held += has;
            CHECK(g_live == held);
            arm(-1);
            CHECK(grow(&g, 5) == RS_OK && g.cap == 16);   // a small call after the failure
            check_group(g);
            CHECK(grow(&g, want) == RS_OK && g.cap >= want && g_live == GROUP_BUFS);
            check_group(g);
        }
    CHECK(g_live == 0);
}

void test_move() {
    arm(-1);
    rs::DevBuf<int> a, b;
    CHECK(a.reserve(4) == RS_OK && b.reserve(9) == RS_OK && g_live == 2);
    int* const pb = b.get();
    const int frees = g_frees;
    a = std::move(b);   // copy-on-grow: a fresh buffer replaces the old one
    CHECK(g_frees == frees + 1 && g_live == 1);   // the target's old block, exactly once
    CHECK(a.get() == pb && a.capacity() == 9 && b.get() == nullptr && b.capacity() == 0);
    rs::DevBuf<int>& self = a;
    a = std::move(self);
    CHECK(a.get() == pb && g_live == 1);
    rs::DevBuf<int> c(std::move(a));
    CHECK(c.get() == pb && a.get() == nullptr && g_frees == frees + 1);

    rs::PinnedBuf<int> x, y;
    CHECK(x.reserve(4, hipHostMallocDefault) == RS_OK && y.reserve(9, hipHostMallocDefault) == RS_OK);
    int* const py = y.get();
    const int frees2 = g_frees;
    x = std::move(y);
    CHECK(g_frees == frees2 + 1 && x.get() == py && x.dev() == py && x.capacity() == 9);
    CHECK(y.get() == nullptr && y.dev() == nullptr && y.capacity() == 0);
}

// rs::grown against the loop every growth site wrote out before it, for the first
// capacities the handles start from (1, 16, 64, 4096) and the three integer types they use.
template <class T>
T doubling_loop(T old_cap, T need, T first) {
    if (need <= old_cap) return old_cap;
    T cap = old_cap > 0 ? old_cap : first;
    while (cap < need) cap *= 2;
    return cap;
}
template <class T>
void test_grown_as() {
    for (const T first : {(T)1, (T)16, (T)64, (T)4096})
        for (T old_cap = 0; old_cap <= 64 * first; old_cap = old_cap ? 2 * old_cap : first)
            for (const T need : {(T)0, (T)1, first - 1, first, first + 1, old_cap, old_cap + 1, 2 * old_cap,
                                 2 * old_cap + 1, (T)1000, (T)4097, (T)100000, (T)((1 << 30) - 1), (T)(1 << 30)}) {
                const T cap = rs::grown<T>(old_cap, need, first);
                CHECK(cap == doubling_loop<T>(old_cap, need, first));
                CHECK(cap >= need && cap >= old_cap);
                CHECK(need > old_cap || cap == old_cap);          // within capacity: unchanged
                CHECK(need <= old_cap || cap / 2 < need || cap == first);   // no further than needed
                T p = cap;   // first times a power of two, from such a capacity
                while (p > first && p % 2 == 0) p /= 2;
                CHECK(cap == 0 || p == first);
            }
    static_assert(rs::grown(0, 5, 16) == 16 && rs::grown(16, 17, 16) == 32 && rs::grown(64, 64, 16) == 64, "");
}
void test_grown() {
    test_grown_as<int>();
    test_grown_as<int64_t>();
    test_grown_as<size_t>();
}

// ---- rs::Stream / rs::Event ----

void test_owner_create() {
    arm(-1);
    {
        rs::Stream s;
        rs::Event e;
        CHECK(s.get() == nullptr && e.get() == nullptr);
        CHECK(s.create() == RS_OK && s.get() && g_live == 1);
        CHECK(e.create(hipEventDisableTiming) == RS_OK && e.get() && g_live == 2);
        const hipStream_t ps = s.get();
        const hipEvent_t pe = e.get();
        const int allocs = g_allocs;
        CHECK(s.create() == RS_OK && e.create() == RS_OK);   // on a full owner: nothing
        CHECK(g_allocs == allocs && s.get() == ps && e.get() == pe && g_live == 2);
        e.reset();
        CHECK(e.get() == nullptr && g_live == 1);
        e.reset();
        CHECK(g_live == 1);
    }
    CHECK(g_live == 0);   // the destructors
}

void test_owner_refused() {
    rs::Stream s;
    rs::Event e;
    arm(0);
    rs::clear_error();
    CHECK(s.create("test stream") == RS_ERR_HIP && s.get() == nullptr && g_live == 0);
    CHECK(std::strstr(g_error, "test stream") != nullptr);
    arm(0);
    CHECK(e.create(hipEventDefault, "test event") == RS_ERR_HIP && e.get() == nullptr && g_live == 0);
    CHECK(std::strstr(g_error, "test event") != nullptr);
    arm(-1);
    CHECK(s.create() == RS_OK && e.create() == RS_OK && g_live == 2);   // and creates again
}

void test_owner_move() {
    arm(-1);
    rs::Event a, b;
    CHECK(a.create() == RS_OK && b.create() == RS_OK && g_live == 2);
    const hipEvent_t pb = b.get();
    const int frees = g_frees;
    a = std::move(b);
    CHECK(g_frees == frees + 1 && g_live == 1);   // the target's old event, exactly once
    CHECK(a.get() == pb && b.get() == nullptr);
    rs::Event& self = a;
    a = std::move(self);
    CHECK(a.get() == pb && g_live == 1);
    {
        rs::Event c(std::move(a));
        CHECK(c.get() == pb && a.get() == nullptr && g_frees == frees + 1);
    }   // c destroys it; a, moved from, does not (a second release is the sanitizer's to report)
    CHECK(g_live == 0 && g_frees == frees + 2);
    rs::Stream s, t;
    CHECK(s.create() == RS_OK);
    const hipStream_t ps = s.get();
    t = std::move(s);
    CHECK(t.get() == ps && s.get() == nullptr && g_live == 1);
}

// A stream and its four events, created on first use the way rs_vt_match_stream creates its
// upload group: into locals, moved into the handle once every one exists.
struct Lazy {
    rs::Stream stream;
    rs::Event up[2], used[2];
};
constexpr int LAZY_OBJECTS = 5;

int ensure(Lazy* g) {
    if (g->stream.get()) return RS_OK;
    rs::Stream st;
    rs::Event up[2], used[2];
    RS_TRY(st.create());
    for (int i = 0; i < 2; ++i) {
        RS_TRY(up[i].create(hipEventDisableTiming));
        RS_TRY(used[i].create(hipEventDisableTiming));
    }
    for (int i = 0; i < 2; ++i) {
        g->up[i] = std::move(up[i]);
        g->used[i] = std::move(used[i]);
    }
    g->stream = std::move(st);
    return RS_OK;
}

bool lazy_absent(const Lazy& g) {
    return !g.stream.get() && !g.up[0].get() && !g.up[1].get() && !g.used[0].get() && !g.used[1].get();
}
bool lazy_whole(const Lazy& g) {
    return g.stream.get() && g.up[0].get() && g.up[1].get() && g.used[0].get() && g.used[1].get();
}

void test_lazy_group() {
    for (int k = 0; k < LAZY_OBJECTS; ++k) {
        Lazy g;
        arm(k);
        CHECK(ensure(&g) == RS_ERR_HIP);
        CHECK(lazy_absent(g) && g_live == 0);   // whole or not at all
        arm(-1);
        CHECK(ensure(&g) == RS_OK && lazy_whole(g) && g_live == LAZY_OBJECTS);   // the retry builds it
        const hipStream_t ps = g.stream.get();
        const int allocs = g_allocs;
        CHECK(ensure(&g) == RS_OK && g.stream.get() == ps && g_allocs == allocs);
    }
    CHECK(g_live == 0);
}

// The profiling-event pool of the pose cells (pc_ensure_events): the missing events whole or
// not at all.
int ensure_events(std::vector<rs::Event>* pool, size_t need) {
    std::vector<rs::Event> fresh(need > pool->size() ? need - pool->size() : 0);
    for (rs::Event& e : fresh) RS_TRY(e.create());
    for (rs::Event& e : fresh) pool->push_back(std::move(e));
    return RS_OK;
}

bool pool_valid(const std::vector<rs::Event>& pool) {
    for (const rs::Event& e : pool) {
        if (!e.get()) return false;
        *reinterpret_cast<volatile char*>(e.get());   // still the test's block (the sanitizer checks)
    }
    return true;
}

void test_event_pool() {
    for (int old = 0; old <= 4; old += 4)        // from empty, and from a pool of four
        for (int k = 0; k < 8 - old; ++k) {
            std::vector<rs::Event> pool;
            arm(-1);
            CHECK(ensure_events(&pool, (size_t)old) == RS_OK && (int)pool.size() == old && g_live == old);
            arm(k);
            CHECK(ensure_events(&pool, 8) == RS_ERR_HIP);
            CHECK((int)pool.size() == old && g_live == old && pool_valid(pool));   // the old size, all valid
            arm(-1);
            CHECK(ensure_events(&pool, 8) == RS_OK && pool.size() == 8 && g_live == 8 && pool_valid(pool));
            CHECK(ensure_events(&pool, 3) == RS_OK && pool.size() == 8 && g_live == 8);
        }
    CHECK(g_live == 0);
}

// A handle the way the library declares one -- buffers, then owners -- and its create: one
// exit through a unique_ptr whose deleter is the destroy function.
struct Handle {
    rs::DevBuf<float> state;
    rs::PinnedBuf<int> staging;
    rs::Stream stream;
    rs::Event ev[2];
};
constexpr int HANDLE_STAGES = 5;

int handle_destroy(Handle* h) {
    delete h;
    return RS_OK;
}

int handle_create(Handle** out) {
    *out = nullptr;
    std::unique_ptr<Handle, int (*)(Handle*)> owner(new Handle(), handle_destroy);
    Handle* const h = owner.get();
    RS_TRY(h->stream.create());
    for (rs::Event& e : h->ev) RS_TRY(e.create());
    RS_TRY(h->state.reserve(100));
    RS_TRY(h->staging.reserve(3, hipHostMallocDefault));
    *out = owner.release();
    return RS_OK;
}

void test_handle_create() {
    for (int k = 0; k < HANDLE_STAGES; ++k) {
        Handle* h = nullptr;
        arm(k);
        CHECK(handle_create(&h) != RS_OK && h == nullptr && g_live == 0);
    }
    Handle* h = nullptr;
    arm(-1);
    CHECK(handle_create(&h) == RS_OK && h && g_live == HANDLE_STAGES);
    CHECK(handle_destroy(h) == RS_OK && g_live == 0);
}

}  // namespace

int main() {
    test_grown();
    test_reserve();
    CHECK(g_live == 0);
    test_failed_reserve();
    CHECK(g_live == 0);
    test_group_growth();
    test_move();
    CHECK(g_live == 0);
    test_owner_create();
    test_owner_refused();
    CHECK(g_live == 0);
    test_owner_move();
    CHECK(g_live == 0);
    test_lazy_group();
    test_event_pool();
    test_handle_create();
    CHECK(g_live == 0);   // at exit nothing is live
    std::printf("%d checks, %d failed, %d live\n", g_checks, g_failed, g_live);
    return g_failed == 0 && g_live == 0 ? 0 : 1;
}
