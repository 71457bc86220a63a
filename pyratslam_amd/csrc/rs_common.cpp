// Error state and library-level entry points of libratslam_hip.
#include "rs_common.h"

#include <cstring>

namespace rs {

static thread_local char g_err[1024] = {0};

void set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

void clear_error() { g_err[0] = 0; }

// (a refused allocation is the caller's error code, not a pending error for the next launch check)
static hipError_t forget(hipError_t e) {
    if (e != hipSuccess) (void)hipGetLastError();
    return e;
}

hipError_t dev_alloc(void** ptr, size_t bytes) { return forget(hipMalloc(ptr, bytes)); }

hipError_t dev_free(void* ptr) { return forget(hipFree(ptr)); }

hipError_t pinned_alloc(void** ptr, void** dev, size_t bytes, unsigned flags) {
    hipError_t e = hipHostMalloc(ptr, bytes, flags);
    if (e == hipSuccess && (e = hipHostGetDevicePointer(dev, *ptr, 0)) != hipSuccess) {
        (void)hipHostFree(*ptr);
        *ptr = nullptr;
    }
    return forget(e);
}

hipError_t pinned_free(void* ptr) { return forget(hipHostFree(ptr)); }

hipError_t stream_create(hipStream_t* s) { return forget(hipStreamCreateWithFlags(s, hipStreamNonBlocking)); }

hipError_t stream_destroy(hipStream_t s) { return forget(hipStreamDestroy(s)); }

hipError_t event_create(hipEvent_t* e, unsigned flags) { return forget(hipEventCreateWithFlags(e, flags)); }

hipError_t event_destroy(hipEvent_t e) { return forget(hipEventDestroy(e)); }

int use_device(int device) {
    int ndev = 0;
    RS_HIP(hipGetDeviceCount(&ndev));
    RS_CHECK(device >= 0 && device < ndev, RS_ERR_ARG, "device %d not in [0, %d)", device, ndev);
    RS_HIP(hipSetDevice(device));
    return RS_OK;
}

hipError_t sync_streams(std::initializer_list<hipStream_t> streams) {
    hipError_t first = hipSuccess;
    for (hipStream_t s : streams) {
        const hipError_t e = s ? hipStreamSynchronize(s) : hipSuccess;
        if (first == hipSuccess) first = e;
    }
    return first;
}

}  // namespace rs

extern "C" {

int rs_version(void) { return 100; }

const char* rs_last_error(void) { return rs::g_err; }

int rs_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

int rs_dev_malloc(int device, size_t bytes, void** ptr) {
    rs::clear_error();
    RS_CHECK(ptr, RS_ERR_ARG, "null output pointer");
    *ptr = nullptr;
    RS_HIP(hipSetDevice(device));
    RS_HIP(rs::dev_alloc(ptr, bytes));
    return RS_OK;
}

int rs_dev_free(void* ptr) {
    rs::clear_error();
    if (ptr) RS_HIP(rs::dev_free(ptr));
    return RS_OK;
}

int rs_dev_copy(void* dst, const void* src, size_t bytes) {
    rs::clear_error();
    RS_CHECK(dst && src, RS_ERR_ARG, "null pointer");
    RS_HIP(hipMemcpy(dst, src, bytes, hipMemcpyDefault));
    return RS_OK;
}

int rs_host_alloc(size_t bytes, void** ptr) {
    rs::clear_error();
    RS_CHECK(ptr, RS_ERR_ARG, "null output pointer");
    *ptr = nullptr;
    void* dev = nullptr;
    RS_HIP(rs::pinned_alloc(ptr, &dev, bytes, hipHostMallocMapped | hipHostMallocCoherent));
    return RS_OK;
}

int rs_host_free(void* ptr) {
    rs::clear_error();
    if (ptr) RS_HIP(rs::pinned_free(ptr));
    return RS_OK;
}

}  // extern "C"
