// Linked experience map on MI355X (gfx950): poses of the experiences on the device, the
// damped-Jacobi relaxation over their links as kernels.
//
// The reference's ExperienceMap is dead reckoning ("TODO: linking will go here",
// experience_map.py:58); pyratslam_amd/linked_experience_map.py defines the linked map and is
// the NumPy restatement.  The arithmetic is in em_rule.h, one function per experience that
// both kernel forms and rs_em_relax_host call, so all three give the same operations in the
// same order (this file is built with contraction off).
//
//   lds    one workgroup of 1,024 threads, both iterates in LDS (48 B per experience, 3,072
//          experiences = 144 KiB), all sweeps in one launch, one barrier per sweep
//   sweep  one launch per sweep, a thread per experience, two global buffers in turn; the
//          handle's `canon` index follows the result, so no copy is needed for odd counts
// A sweep of the lds form costs one compute unit's time for the whole map, a sweep of the
// sweep form costs a launch (about 6.5 us) while the map fits the chip: measured
// (tools/em_ab.py, profiles/linked_em) the lds form is the faster one up to 768 experiences
// and the slower one from 1,000 on, so the default follows the map's size.
//
// Link records and incidence lists stay in global memory (L2).  The host keeps the link
// list, rebuilds the incidence lists into pinned memory when the topology has changed since
// the last relax, and uploads them on the handle's stream.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "em_rule.h"
#include "rs_common.h"

namespace {

using rs::EmLink;

constexpr int EM_LDS_THREADS = 1024;
constexpr int EM_LDS_CAP = 3072;      // experiences whose two iterates fit 144 KiB of LDS
constexpr int EM_LDS_DEFAULT = 768;   // the largest measured size at which the lds form wins
constexpr int EM_SWEEP_THREADS = 256;
enum EmForm { EM_AUTO = -1, EM_LDS = 0, EM_SWEEP = 1 };

__global__ __launch_bounds__(EM_LDS_THREADS) void em_relax_lds_kernel(
    double* __restrict__ pose, int n, const int32_t* __restrict__ off, const int32_t* __restrict__ adj,
    const EmLink* __restrict__ lk, int loops, double c) {
    __shared__ double s[2][3 * EM_LDS_CAP];
    const int tid = threadIdx.x;
    for (int j = tid; j < 3 * n; j += EM_LDS_THREADS) s[0][j] = pose[j];
    __syncthreads();
    int p = 0;
    for (int it = 0; it < loops; ++it) {
        // reads s[p] only, writes s[p ^ 1] only: one barrier separates the sweeps
        for (int i = tid; i < n; i += EM_LDS_THREADS) rs::em_relax_one(i, s[p], s[p ^ 1], off, adj, lk, c);
        __syncthreads();
        p ^= 1;
    }
    for (int j = tid; j < 3 * n; j += EM_LDS_THREADS) pose[j] = s[p][j];
}

__global__ __launch_bounds__(EM_SWEEP_THREADS) void em_relax_sweep_kernel(
    const double* __restrict__ src, double* __restrict__ dst, int n, const int32_t* __restrict__ off,
    const int32_t* __restrict__ adj, const EmLink* __restrict__ lk, double c) {
    const int i = blockIdx.x * EM_SWEEP_THREADS + threadIdx.x;
    if (i < n) rs::em_relax_one(i, src, dst, off, adj, lk, c);
}

// pose[id] from pose[from] and the measurement (from < 0: the origin, heading `f`)
__global__ void em_place_kernel(double* pose, int from, int id, double d, double hd, double f) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    double out[3] = {0.0, 0.0, f};
    if (from >= 0) rs::em_place(pose + 3 * (size_t)from, d, hd, f, out);
    pose[3 * (size_t)id] = out[0];
    pose[3 * (size_t)id + 1] = out[1];
    pose[3 * (size_t)id + 2] = out[2];
}

int em_check_link(int n, int from, int to) {
    RS_CHECK(from >= 0 && from < n && to >= 0 && to < n, RS_ERR_ARG,
             "link %d -> %d outside the %d experiences", from, to, n);
    RS_CHECK(from != to, RS_ERR_ARG, "link %d -> %d joins an experience to itself", from, to);
    return RS_OK;
}

}  // namespace

// The buffers are rs::DevBuf / rs::PinnedBuf members (rs_common.h).  Group capacities: cap
// experiences (dPose[2], dOff, hOff), lcap links (dLinks, dAdj, hLinks, hAdj).  The stream
// and the events are rs::Stream / rs::Event owners.
struct rs_em {
    int device = 0;
    double c = 0.5;
    int forced = EM_AUTO;
    int n = 0, cap = 0, lcap = 0, canon = 0;
    std::vector<EmLink> links;               // the list itself (host)
    size_t uploaded = 0;                     // link records already in dLinks
    bool topoDirty = false;                  // n or the links changed since the last upload
    rs::DevBuf<double> dPose[2];
    rs::DevBuf<EmLink> dLinks;
    rs::DevBuf<int32_t> dOff, dAdj;
    rs::PinnedBuf<EmLink> hLinks;
    rs::PinnedBuf<int32_t> hOff, hAdj;
    rs::PinnedBuf<double> hPose;             // staging of rs_em_read / rs_em_write
    bool timing = false, timed = false;
    // the owners come after the buffers: members go in reverse order, streams and events first
    rs::Stream stream;
    rs::Event ev[2];   // around the relax launches (timing)
    rs::Event evUp;    // after the last read of the pinned staging
};

namespace {

int em_form_for(const rs_em* h, int n) {
    if (h->forced != EM_AUTO) return h->forced;
    return n <= EM_LDS_DEFAULT ? EM_LDS : EM_SWEEP;
}

// Room for n experiences; the poses move with a fresh pair of buffers.
int em_grow_pose(rs_em* h, int n) {
    if (n <= h->cap) return RS_OK;
    const int cap = rs::grown(h->cap, n, 1);
    RS_HIP(hipStreamSynchronize(h->stream.get()));
    rs::DevBuf<double> a, b;
    RS_TRY(a.reserve(3 * (size_t)cap, "experience poses"));
    RS_TRY(b.reserve(3 * (size_t)cap, "experience poses"));
    if (h->n > 0) {
        RS_HIP(hipMemcpyAsync(a.get(), h->dPose[h->canon].get(), sizeof(double) * 3 * h->n,
                              hipMemcpyDeviceToDevice, h->stream.get()));
        RS_HIP(hipStreamSynchronize(h->stream.get()));
    }
    h->dPose[0] = std::move(a);
    h->dPose[1] = std::move(b);
    h->canon = 0;
    h->cap = cap;
    return RS_OK;
}

// Rebuild and upload the incidence lists and the new link records (queued, not waited for).
int em_upload_topology(rs_em* h) {
    const size_t L = h->links.size();
    const size_t noff = 2 * (size_t)h->cap + 1;
    RS_HIP(hipEventSynchronize(h->evUp.get()));   // the last upload has read the pinned staging
    if (noff > h->dOff.capacity() || (int64_t)L > h->lcap)
        RS_HIP(hipStreamSynchronize(h->stream.get()));   // queued kernels read the blocks about to go
    RS_TRY(h->dOff.reserve(noff, "incidence offsets"));
    RS_TRY(h->hOff.reserve(noff, hipHostMallocDefault, "incidence offsets"));
    if ((int64_t)L > h->lcap) {
        const int lcap = rs::grown(h->lcap, (int)L, 16);
        h->lcap = 0;
        h->uploaded = 0;                            // the records are sent again, not copied
        RS_TRY(h->dLinks.reserve(lcap, "link records"));
        RS_TRY(h->dAdj.reserve(2 * (size_t)lcap, "incidence lists"));
        RS_TRY(h->hLinks.reserve(lcap, hipHostMallocDefault, "link records"));
        RS_TRY(h->hAdj.reserve(2 * (size_t)lcap, hipHostMallocDefault, "incidence lists"));
        h->lcap = lcap;
    }
    rs::em_build_incidence(h->n, (int)L, h->links.data(), h->hOff.get(), h->hAdj.get());
    RS_HIP(hipMemcpyAsync(h->dOff.get(), h->hOff.get(), sizeof(int32_t) * (2 * (size_t)h->n + 1),
                          hipMemcpyHostToDevice, h->stream.get()));
    if (L > 0) {
        RS_HIP(hipMemcpyAsync(h->dAdj.get(), h->hAdj.get(), sizeof(int32_t) * 2 * L, hipMemcpyHostToDevice,
                              h->stream.get()));
        const size_t u = h->uploaded;
        if (L > u) {
            std::memcpy(h->hLinks.get() + u, h->links.data() + u, sizeof(EmLink) * (L - u));
            RS_HIP(hipMemcpyAsync(h->dLinks.get() + u, h->hLinks.get() + u, sizeof(EmLink) * (L - u),
                                  hipMemcpyHostToDevice, h->stream.get()));
            h->uploaded = L;
        }
    }
    RS_HIP(hipEventRecord(h->evUp.get(), h->stream.get()));
    h->topoDirty = false;
    return RS_OK;
}

}  // namespace

extern "C" {

int rs_em_relax_host(int nexp, int nlinks, const int32_t* from, const int32_t* to, const double* d,
                     const double* heading, const double* facing, double* xyth, int loops,
                     double correction) {
    rs::clear_error();
    RS_CHECK(nexp >= 0 && nlinks >= 0 && loops >= 0, RS_ERR_ARG, "negative count");
    RS_CHECK(nexp == 0 || xyth, RS_ERR_ARG, "null poses");
    RS_CHECK(nlinks == 0 || (from && to && d && heading && facing), RS_ERR_ARG, "null link arrays");
    std::vector<EmLink> lk((size_t)nlinks);
    for (int l = 0; l < nlinks; ++l) {
        RS_TRY(em_check_link(nexp, from[l], to[l]));
        lk[l] = {from[l], to[l], d[l], heading[l], facing[l]};
    }
    if (nexp == 0 || loops == 0) return RS_OK;
    std::vector<int32_t> off(2 * (size_t)nexp + 1), adj(2 * (size_t)nlinks);
    rs::em_build_incidence(nexp, nlinks, lk.data(), off.data(), adj.data());
    std::vector<double> other(3 * (size_t)nexp);
    double *src = xyth, *dst = other.data();
    for (int it = 0; it < loops; ++it) {
        for (int i = 0; i < nexp; ++i) rs::em_relax_one(i, src, dst, off.data(), adj.data(), lk.data(), correction);
        std::swap(src, dst);
    }
    if (src != xyth) std::memcpy(xyth, src, sizeof(double) * 3 * (size_t)nexp);
    return RS_OK;
}

int rs_em_create(int capacity, double correction, int device, rs_em** out) {
    rs::clear_error();
    RS_CHECK(out, RS_ERR_ARG, "null output handle pointer");
    *out = nullptr;
    RS_CHECK(capacity >= 1, RS_ERR_ARG, "capacity %d < 1", capacity);
    RS_CHECK(correction > 0.0 && correction <= 1.0, RS_ERR_ARG, "correction %g outside (0, 1]", correction);
    int forced = EM_AUTO;
    if (const char* e = std::getenv("RS_EM_FORM")) {
        if (!std::strcmp(e, "lds")) forced = EM_LDS;
        else if (!std::strcmp(e, "sweep")) forced = EM_SWEEP;
        else RS_CHECK(!*e, RS_ERR_ARG, "RS_EM_FORM=%s: expected lds or sweep", e);
    }
    RS_TRY(rs::use_device(device));
    // one failure exit: rs_em_destroy takes a handle at any stage
    std::unique_ptr<rs_em, int (*)(rs_em*)> owner(new rs_em(), rs_em_destroy);
    rs_em* const h = owner.get();
    h->device = device;
    h->c = correction;
    h->forced = forced;
    RS_TRY(h->stream.create());
    for (rs::Event& e : h->ev) RS_TRY(e.create());
    RS_TRY(h->evUp.create(hipEventDisableTiming));
    RS_HIP(hipEventRecord(h->evUp.get(), h->stream.get()));
    RS_TRY(em_grow_pose(h, capacity));
    RS_TRY(h->hPose.reserve(3, hipHostMallocDefault, "pose staging"));
    *out = owner.release();
    return RS_OK;
}

int rs_em_destroy(rs_em* h) {
    if (!h) return RS_OK;
    (void)hipSetDevice(h->device);
    // queued work that failed after a call returned is reported here, not dropped
    const hipError_t se = rs::sync_streams({h->stream.get()});
    delete h;  // (the streams and events, then the buffers, go with their members)
    RS_CHECK(se == hipSuccess, RS_ERR_HIP, "work queued before rs_em_destroy failed: %s", hipGetErrorString(se));
    return RS_OK;
}

int rs_em_count(rs_em* h, int* nexp, int* nlinks) {
    rs::clear_error();
    RS_CHECK(h, RS_ERR_STATE, "null experience-map handle");
    if (nexp) *nexp = h->n;
    if (nlinks) *nlinks = (int)h->links.size();
    return RS_OK;
}

int rs_em_add_experience(rs_em* h, int from, double d, double heading, double facing, int* id) {
    rs::clear_error();
    RS_CHECK(h, RS_ERR_STATE, "null experience-map handle");
    RS_CHECK(from >= -1 && from < h->n, RS_ERR_ARG, "experience %d outside [-1, %d)", from, h->n);
    RS_CHECK(h->n < INT32_MAX / 8, RS_ERR_ARG, "too many experiences");
    RS_HIP(hipSetDevice(h->device));
    RS_TRY(em_grow_pose(h, h->n + 1));
    hipLaunchKernelGGL(em_place_kernel, dim3(1), dim3(64), 0, h->stream.get(), h->dPose[h->canon].get(), from,
                       h->n, d, heading, facing);
    RS_HIP(hipGetLastError());
    if (id) *id = h->n;
    ++h->n;
    h->topoDirty = true;
    return RS_OK;
}

int rs_em_add_link(rs_em* h, int from, int to, double d, double heading, double facing, int* id) {
    rs::clear_error();
    RS_CHECK(h, RS_ERR_STATE, "null experience-map handle");
    RS_TRY(em_check_link(h->n, from, to));
    RS_CHECK(h->links.size() < (size_t)INT32_MAX / 8, RS_ERR_ARG, "too many links");
    if (id) *id = (int)h->links.size();
    h->links.push_back({from, to, d, heading, facing});
    h->topoDirty = true;
    return RS_OK;
}

int rs_em_relax(rs_em* h, int loops) {
    rs::clear_error();
    RS_CHECK(h, RS_ERR_STATE, "null experience-map handle");
    RS_CHECK(loops >= 0, RS_ERR_ARG, "negative sweep count");
    const int form = em_form_for(h, h->n);
    RS_CHECK(form != EM_LDS || h->n <= EM_LDS_CAP, RS_ERR_ARG,
             "RS_EM_FORM=lds holds %d experiences at most, the map has %d", EM_LDS_CAP, h->n);
    h->timed = false;
    if (h->n == 0 || loops == 0) return RS_OK;
    RS_HIP(hipSetDevice(h->device));
    if (h->topoDirty) RS_TRY(em_upload_topology(h));
    const bool timed = h->timing;
    if (timed) RS_HIP(hipEventRecord(h->ev[0].get(), h->stream.get()));
    if (form == EM_LDS) {
        hipLaunchKernelGGL(em_relax_lds_kernel, dim3(1), dim3(EM_LDS_THREADS), 0, h->stream.get(),
                           h->dPose[h->canon].get(), h->n, h->dOff.get(), h->dAdj.get(), h->dLinks.get(),
                           loops, h->c);
        RS_HIP(hipGetLastError());
    } else {
        const int blocks = (h->n + EM_SWEEP_THREADS - 1) / EM_SWEEP_THREADS;
        for (int it = 0; it < loops; ++it) {
            hipLaunchKernelGGL(em_relax_sweep_kernel, dim3(blocks), dim3(EM_SWEEP_THREADS), 0, h->stream.get(),
                               h->dPose[h->canon].get(), h->dPose[h->canon ^ 1].get(), h->n, h->dOff.get(),
                               h->dAdj.get(), h->dLinks.get(), h->c);
            RS_HIP(hipGetLastError());
            h->canon ^= 1;   // the result is the canonical buffer from here on
        }
    }
    if (timed) {
        RS_HIP(hipEventRecord(h->ev[1].get(), h->stream.get()));
        h->timed = true;
    }
    return RS_OK;
}

int rs_em_read(rs_em* h, int first, int n, double* xyth) {
    rs::clear_error();
    RS_CHECK(h, RS_ERR_STATE, "null experience-map handle");
    RS_CHECK(first >= 0 && n >= 0 && first <= h->n && n <= h->n - first, RS_ERR_ARG,
             "experiences [%d, %d + %d) outside the %d of the map", first, first, n, h->n);
    if (n == 0) return RS_OK;
    RS_CHECK(xyth, RS_ERR_ARG, "null argument");
    RS_HIP(hipSetDevice(h->device));
    RS_TRY(h->hPose.reserve(3 * (size_t)n, hipHostMallocDefault, "pose staging"));
    RS_HIP(hipMemcpyAsync(h->hPose.get(), h->dPose[h->canon].get() + 3 * (size_t)first, sizeof(double) * 3 * n,
                          hipMemcpyDeviceToHost, h->stream.get()));
    RS_HIP(hipStreamSynchronize(h->stream.get()));
    std::memcpy(xyth, h->hPose.get(), sizeof(double) * 3 * n);
    return RS_OK;
}

int rs_em_write(rs_em* h, int first, int n, const double* xyth) {
    rs::clear_error();
    RS_CHECK(h, RS_ERR_STATE, "null experience-map handle");
    RS_CHECK(first >= 0 && n >= 0 && first <= h->n && n <= h->n - first, RS_ERR_ARG,
             "experiences [%d, %d + %d) outside the %d of the map", first, first, n, h->n);
    if (n == 0) return RS_OK;
    RS_CHECK(xyth, RS_ERR_ARG, "null argument");
    RS_HIP(hipSetDevice(h->device));
    RS_TRY(h->hPose.reserve(3 * (size_t)n, hipHostMallocDefault, "pose staging"));
    std::memcpy(h->hPose.get(), xyth, sizeof(double) * 3 * n);
    RS_HIP(hipMemcpyAsync(h->dPose[h->canon].get() + 3 * (size_t)first, h->hPose.get(), sizeof(double) * 3 * n,
                          hipMemcpyHostToDevice, h->stream.get()));
    RS_HIP(hipStreamSynchronize(h->stream.get()));   // the staging is free again
    return RS_OK;
}

int rs_em_set_timing(rs_em* h, int enable) {
    rs::clear_error();
    RS_CHECK(h, RS_ERR_STATE, "null experience-map handle");
    h->timing = enable != 0;
    return RS_OK;
}

int rs_em_last_ms(rs_em* h, double* ms) {
    rs::clear_error();
    RS_CHECK(h && ms, RS_ERR_ARG, "null argument");
    *ms = -1.0;
    if (!h->timed) return RS_OK;
    float t = 0.f;
    RS_HIP(hipEventSynchronize(h->ev[1].get()));
    RS_HIP(hipEventElapsedTime(&t, h->ev[0].get(), h->ev[1].get()));
    *ms = t;
    return RS_OK;
}

const char* rs_em_form(rs_em* h) {
    if (!h) return "";
    return em_form_for(h, h->n) == EM_LDS ? "lds" : "sweep";
}

}  // extern "C"
