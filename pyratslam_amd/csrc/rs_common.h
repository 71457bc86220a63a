// Shared helpers of libratslam_hip: error state, HIP call checking, the two owning buffer
// types (rs::DevBuf, rs::PinnedBuf) that hold every handle's device and pinned memory, and
// the two owners (rs::Stream, rs::Event) of its streams and events.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <memory>
#include <string>
#include <type_traits>
#include <utility>

#include "ratslam_abi.h"

namespace rs {

void set_error(const char* fmt, ...);
void clear_error();

// Return-on-failure wrappers for the extern "C" entry points.
#define RS_HIP(call)                                                              \
    do {                                                                          \
        hipError_t e_ = (call);                                                   \
        if (e_ != hipSuccess) {                                                   \
            ::rs::set_error("%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), \
                            __FILE__, __LINE__);                                  \
            return RS_ERR_HIP;                                                    \
        }                                                                         \
    } while (0)

#define RS_CHECK(cond, code, ...)            \
    do {                                     \
        if (!(cond)) {                       \
            ::rs::set_error(__VA_ARGS__);    \
            return (code);                   \
        }                                    \
    } while (0)

#define RS_TRY(expr)                 \
    do {                             \
        int s_ = (expr);             \
        if (s_ != RS_OK) return s_;  \
    } while (0)

// Positive modulo for (possibly negative) halo coordinates.
__host__ __device__ inline int wrapi(int v, int n) {
    int r = v % n;
    return r < 0 ? r + n : r;
}

inline size_t round_up(size_t v, size_t m) { return (v + m - 1) / m * m; }

// The capacity a buffer group of capacity old_cap grows to for `need` elements: old_cap while
// it suffices, otherwise old_cap (`first` for an empty group) doubled until it does.  How to
// grow (zeroing the group capacity first, fills, flags, synchronises) stays with the caller.
template <class T>
constexpr T grown(T old_cap, T need, T first) {
    if (need <= old_cap) return old_cap;
    T cap = old_cap > 0 ? old_cap : first;
    while (cap < need) cap *= 2;
    return cap;
}

// A kernel instance's integer parameter chosen at run time, passed on as a type.
template <int N>
using Int = std::integral_constant<int, N>;

// Whether p is device memory (hipMemoryTypeDevice exactly); a host pointer is not an error.
inline bool on_device(const void* p) {
    hipPointerAttribute_t attr{};
    const bool dev = hipPointerGetAttributes(&attr, p) == hipSuccess && attr.type == hipMemoryTypeDevice;
    (void)hipGetLastError();
    return dev;
}

// A switch read from the environment: on unless the variable is set to "0".
inline bool env_on(const char* name) { const char* e = std::getenv(name); return !(e && std::strcmp(e, "0") == 0); }

// The host's bounded wait for n items a kernel stores into pinned memory one by one:
// arrived(i) reads item i (through the caller's volatile pointer).  True once all n have
// arrived, false when the spin runs out (a slow or faulted kernel): the caller then
// synchronises the stream, which returns any error.
constexpr long SPIN_LIMIT = 4'000'000;
template <class Arrived>
__attribute__((always_inline)) inline bool spin_until(int n, Arrived arrived) {
    int i = 0;
    for (long spin = 0; spin < SPIN_LIMIT && i < n; ++spin)
        while (i < n && arrived(i)) ++i;
    return i == n;
}

// The library's only allocation and release calls (rs_common.cpp): hipMalloc, hipFree,
// hipHostMalloc (with the block's device address, hipHostGetDevicePointer) and hipHostFree.
// A refused call leaves no error behind for a later hipGetLastError.
hipError_t dev_alloc(void** ptr, size_t bytes);
hipError_t dev_free(void* ptr);
hipError_t pinned_alloc(void** ptr, void** dev, size_t bytes, unsigned flags);
hipError_t pinned_free(void* ptr);

inline int alloc_failed(hipError_t e, const char* what, size_t bytes) {
    set_error("%s: allocating %zu bytes failed: %s", what, bytes, hipGetErrorString(e));
    return e == hipErrorOutOfMemory ? RS_ERR_NOMEM : RS_ERR_HIP;
}

template <class T> constexpr size_t elem_bytes = sizeof(T);
template <> inline constexpr size_t elem_bytes<void> = 1;  // untyped buffers count bytes

// Owning, move-only device buffer of capacity() elements.  reserve() within the capacity
// does nothing; beyond it, it releases the old block first (a growth never holds both, and
// never copies) and allocates exactly n.  If that fails the buffer is empty: get() ==
// nullptr, capacity() == 0.  So after a failed growth no member of a handle points at freed
// memory; and a handle that guards several buffers by one capacity zeroes it before the
// first reserve of the group and sets it after the last, so that a non-zero group capacity
// means every buffer of the group holds at least that much.  How far to grow, the fill of a
// fresh block and the synchronise its old readers need stay with the caller; a buffer that
// keeps its contents reserves a fresh DevBuf, copies, and move-assigns it.
template <class T>
class DevBuf {
public:
    DevBuf() = default;
    DevBuf(DevBuf&& o) noexcept { *this = std::move(o); }
    DevBuf& operator=(DevBuf&& o) noexcept {
        if (this != &o) {
            reset();
            p_ = std::exchange(o.p_, nullptr);
            n_ = std::exchange(o.n_, 0);
        }
        return *this;
    }
    ~DevBuf() { reset(); }

    T* get() const { return p_; }
    size_t capacity() const { return n_; }
    void reset() { (void)release(); }
    int reserve(size_t n, const char* what = "device buffer") {
        if (n <= n_) return RS_OK;
        void* p = nullptr;
        hipError_t e = release();
        if (e == hipSuccess) e = dev_alloc(&p, elem_bytes<T> * n);
        if (e != hipSuccess) return alloc_failed(e, what, elem_bytes<T> * n);
        p_ = static_cast<T*>(p);
        n_ = n;
        return RS_OK;
    }

private:
    hipError_t release() {
        const hipError_t e = p_ ? dev_free(p_) : hipSuccess;
        p_ = nullptr;
        n_ = 0;
        return e;
    }
    T* p_ = nullptr;
    size_t n_ = 0;
};

// The same for page-locked host memory; dev() is the block in the device's address space.
// The hipHostMalloc flags are the caller's, buffer by buffer: Mapped | Coherent for words
// the host polls while a kernel stores them, Default for staging a copy engine reads.
template <class T>
class PinnedBuf {
public:
    PinnedBuf() = default;
    PinnedBuf(PinnedBuf&& o) noexcept { *this = std::move(o); }
    PinnedBuf& operator=(PinnedBuf&& o) noexcept {
        if (this != &o) {
            reset();
            p_ = std::exchange(o.p_, nullptr);
            d_ = std::exchange(o.d_, nullptr);
            n_ = std::exchange(o.n_, 0);
        }
        return *this;
    }
    ~PinnedBuf() { reset(); }

    T* get() const { return p_; }
    T* dev() const { return d_; }
    size_t capacity() const { return n_; }
    void reset() { (void)release(); }
    int reserve(size_t n, unsigned flags, const char* what = "pinned buffer") {
        if (n <= n_) return RS_OK;
        void *p = nullptr, *d = nullptr;
        hipError_t e = release();
        if (e == hipSuccess) e = pinned_alloc(&p, &d, elem_bytes<T> * n, flags);
        if (e != hipSuccess) return alloc_failed(e, what, elem_bytes<T> * n);
        p_ = static_cast<T*>(p);
        d_ = static_cast<T*>(d);
        n_ = n;
        return RS_OK;
    }

private:
    hipError_t release() {
        const hipError_t e = p_ ? pinned_free(p_) : hipSuccess;
        p_ = d_ = nullptr;
        n_ = 0;
        return e;
    }
    T *p_ = nullptr, *d_ = nullptr;
    size_t n_ = 0;
};

// The library's only calls that create or destroy a stream (always hipStreamNonBlocking) or
// an event (with the caller's flags), in rs_common.cpp.  A refused call leaves no error
// behind either.
hipError_t stream_create(hipStream_t* s);
hipError_t stream_destroy(hipStream_t s);
hipError_t event_create(hipEvent_t* e, unsigned flags);
hipError_t event_destroy(hipEvent_t e);

// Owning, move-only stream (rs::Stream) or event (rs::Event); get() is the raw object a
// launch, record or wait takes.  create() on an owner that holds an object does nothing, as
// reserve() within the capacity; a refused create() leaves it empty, get() == nullptr.  A
// handle declares its owners after its buffers, so that they are destroyed first.  Objects
// a call creates lazily as a group (a stream and the events recorded on it) are created
// into locals and move-assigned into the handle once every one exists: the group is whole or
// absent, and a call after a refused creation creates it again.
template <class T, hipError_t (*Destroy)(T)>
class Owned {
public:
    Owned() = default;
    Owned(Owned&& o) noexcept : p_(std::exchange(o.p_, nullptr)) {}
    Owned& operator=(Owned&& o) noexcept {
        if (this != &o) {
            reset();
            p_ = std::exchange(o.p_, nullptr);
        }
        return *this;
    }
    ~Owned() { reset(); }

    T get() const { return p_; }
    void reset() {
        if (p_) (void)Destroy(p_);
        p_ = nullptr;
    }

protected:
    int created(hipError_t e, const char* what) {
        if (e == hipSuccess) return RS_OK;
        p_ = nullptr;
        set_error("creating %s failed: %s", what, hipGetErrorString(e));
        return RS_ERR_HIP;
    }
    T p_ = nullptr;
};

class Stream : public Owned<hipStream_t, stream_destroy> {
public:
    int create(const char* what = "a stream") { return p_ ? RS_OK : created(stream_create(&p_), what); }
};

class Event : public Owned<hipEvent_t, event_destroy> {
public:
    int create(unsigned flags = hipEventDefault, const char* what = "an event") {
        return p_ ? RS_OK : created(event_create(&p_, flags), what);
    }
};

// What every rs_*_create does after its argument checks: `device` within the device count,
// and current.
int use_device(int device);

// What every rs_*_destroy does first: synchronise each stream the handle owns (null: not yet
// created) and return the first error, so that queued work that failed is reported, not dropped.
hipError_t sync_streams(std::initializer_list<hipStream_t> streams);

}  // namespace rs
