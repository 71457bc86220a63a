// View-template matcher on MI355X (gfx950).
//
// Replaces ViewTemplate.match / ViewTemplates.match
// (/root/reference/ratslam/view_templates.py:16-28, 63-75).
//
// Score of template T against query Q (both H x W uint8):
//   min_{o=-(M-1)..M-1} sum_{r=M..H-M-1, c} (T[r+o][c] - Q[r][c]) mod 256
// (numpy uint8 subtraction wraps and abs() is the identity on uint8).
// Per 4-byte dword this is a carry-free SWAR add of the query's byte negation
// c = -Q (mod 256):  d = ((a & 0x7f7f7f7f) + cL) ^ (a & 0x80808080) ^ cH, then
// v_sad_u8(d, 0, acc) adds the four wrapped bytes: 3 VALU instructions
// (v_add_u32, v_bitop3_b32 XOR3, v_sad_u8) per template-dword x offset pair.
//
// Library layout in HBM (SoA, 16-byte chunks): chunk (tb, c, q, t) at byte
//   (((tb * WD + c) * HQ + q) * 64 + t) * 16
// holds rows 4q..4q+3 (one dword each) of dword column c of template slot
// tb*64 + t.  One global_load_dwordx4 by a wave = 1 KiB contiguous = the same
// 16 bytes of 64 templates.
//
// Result of a scan: per query, the first argmin as a packed key
// (score << 32) | global_index, min-reduced over lanes, waves and (RCCL
// allreduce(min, uint64)) ranks -- exactly numpy's argmin tie-break
// (view_templates.py:73).
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <algorithm>
#include <climits>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <type_traits>
#include <vector>

#include "rs_common.h"
#include "vt_norm_rule.h"
#include "vt_offset_rule.h"
#include "vt_plan.h"

// The device code, one header per scan family, in order of definition.
// They are parts of this translation unit, not free-standing: the file-wide compile flags
// (pyratslam_amd/_build.py, EXTRA) reach every kernel only this way.  A family header
// includes no other family's; what several use is vt_device.h.
namespace {

#include "vt_device.h"
#include "vt_store.h"
#include "vt_carry.h"

static_assert(vt_plan::METRIC_WRAPPED == RS_VT_METRIC_WRAPPED && vt_plan::METRIC_SAD == RS_VT_METRIC_SAD,
              "vt_plan.h restates the ABI's metric codes");
#include "vt_sad.h"
static_assert(rs::VTO_METRIC_WRAPPED == RS_VT_METRIC_WRAPPED && rs::VTO_METRIC_SAD == RS_VT_METRIC_SAD,
              "vt_offset_rule.h restates the ABI's metric codes");
#include "vt_offset.h"
#include "vt_norm.h"

#include "vt_planes.h"
#include "vt_plane_scan.h"
#include "vt_prune.h"

}  // namespace

// ===========================================================================
// Host side
// ===========================================================================
// The query forms a scan reads (planes, raw sums, QS_J, compact planes): a non-owning view
// of the handle's per-batch buffers (vt_batch_view) or, for rs_vt_match_stream, into its
// stream buffers (vt_stream_view), passed to the build and to the scan that reads it.
struct QueryForms {
    uint32_t *qp = nullptr, *qsum = nullptr, *qsj = nullptr, *qc = nullptr;
};

// The buffers are rs::DevBuf / rs::PinnedBuf members (rs_common.h, with the invariant the
// group capacities qCap, idxCap, matCap, candCap, frameCap, pruneCap, listCntCap,
// qpStreamCap, streamCap and upCap keep).  The library (localCap: dLib, dLibP, dLibTs) is
// copied when it grows, each buffer into a new block before its old one goes, so localCap
// simply stays until all three have grown.  The streams and events are rs::Stream /
// rs::Event owners; rs_vt_match_stream creates its two groups (the collective stream's, the
// upload stream's) on first use, each whole or not at all.
struct rs_vt {
    int H = 0, W = 0, M = 0, WD = 0, HQ = 0;
    // ViewTemplates.match's threshold (view_templates.py:67): a score (< 2^32, exact in
    // a double) makes a new template when score > thr, compared in float64 exactly as
    // numpy compares a uint64 with a Python float (NaN: never; negative: always)
    double thr = 0.0;
    int device = 0;
    int rank = 0, nranks = 1;
    ncclComm_t comm = nullptr;
    int64_t count = 0;     // global number of templates
    int64_t localCap = 0;  // local slots allocated (multiple of 64): dLib, dLibP, dLibTs
    rs::DevBuf<uint4> dLib;
    // query staging
    int qCap = 0;
    rs::DevBuf<uint8_t> dQraw;
    rs::PinnedBuf<uint8_t> hQraw;  // fine-grained (a small batch's plane kernel reads it in place)
    bool qrawBusy = false;     // hQraw read by queued work not yet known to have run
    rs::DevBuf<uint2> dQf;
    rs::DevBuf<uint32_t> dQsum;
    rs::DevBuf<unsigned long long> dBest;
    rs::PinnedBuf<unsigned long long> hBest;  // fine-grained: vt_fetch_keys polls the words the export kernel stores
    bool stagingBusy = false;  // copies from hSrc / hDst queued and not yet known to have run
    rs::DevBuf<uint8_t> dUp[2];              // rs_vt_match_stream: the upload stream's two raw-query group buffers
    size_t upCap = 0;                        // bytes per group buffer
    rs::DevBuf<uint32_t> dQpStream;          // rs_vt_match_stream: every batch's query planes
    rs::DevBuf<uint32_t> dQsumStream;
    size_t qpStreamCap = 0;                  // queries (dQpStream, dQsumStream, dQsjStream, dQcStream)
    rs::DevBuf<unsigned long long> dStream;  // keys of rs_vt_match_stream, one row per batch
    rs::PinnedBuf<unsigned long long> hStream;  // pinned copy (nb * nq)
    size_t streamCap = 0;
    bool streamClean = false;                // dStream holds UINT64_MAX (vt_keys_export resets it)
    int bestClean = 0;     // leading dBest entries known to hold UINT64_MAX
    int bestPending = 0;   // bestClean once the keys of the running scan are exported
    // index lists for stores
    int idxCap = 0;
    rs::DevBuf<int32_t> dSrc;
    rs::DevBuf<int64_t> dDst;
    rs::PinnedBuf<int32_t> hSrc;   // (staging a copy engine reads: not fine-grained)
    rs::PinnedBuf<int64_t> hDst;
    // candidate library and score matrix for in-batch resolution
    int64_t candCap = 0;   // slots: dCand, dCandP, dCandTs
    rs::DevBuf<uint4> dCand;
    size_t matCap = 0;
    rs::DevBuf<uint32_t> dMat;
    rs::PinnedBuf<uint32_t> hMat;
    bool timing = false;  // HIP events around every scan (rs_vt_set_timing; off: the keys are polled)
    bool timedScan = false;  // the last scan recorded ev0/ev1
    float lastMs = 0.f;
    int stagedQ = 0;  // queries staged by the last scan
    // bit-plane scan (default when W == 32, H in {32, 64}, max_offset 8; RS_VT_SCAN=plane):
    // planes + TS of the library and candidate slots, query planes + raw sums
    bool planar = false;
    // the metric, fixed at create (rs_vt_create_metric): RS_VT_METRIC_SAD handles are never
    // planar and never prune; their query form (vt_qform_sad_kernel) lives in dQf
    int metric = RS_VT_METRIC_WRAPPED;
    rs::DevBuf<uint32_t> dLibP, dLibTs, dCandP, dCandTs;
    rs::DevBuf<uint32_t> dQp, dQsumRaw;   // (with qCap, like dQsj and dQc)
    int planeSlots = 0;  // resident plane-scan blocks on the device (occupancy x CUs)
    rs::DevBuf<unsigned> dCtr;   // per template block x query group: next batch (plane scan)
    rs::DevBuf<unsigned> dDone;  // plane scan blocks finished (the folded key export; reset by the last)
    bool keysFolded = false;   // the running scan exports its own keys (vt_fetch_keys: no export launch)
    // pruned plane scan (H = 64 frozen key scans; RS_VT_PRUNE): 0 dense everywhere, 1 above
    // VT_PRUNE_MIN_Q queries and one template block, 2 ("force") at any size
    int prune = 0;
    // its front in one launch (vt_front_kernel; RS_VT_FRONT): 0 never, 1 where
    // vt_plan::front_fused says so, 2 ("force") for any shape
    int front = 1;
    // entries per batch of its list passes (RS_VT_LIST_NB): 0 by vt_plan::list_width, or 1, 2, 4
    int listNb = VT_LIST_NB;
    rs::DevBuf<uint32_t> dQsj;        // QS_J of the queries in dQp
    rs::DevBuf<uint32_t> dQsjStream;  // ... of dQpStream
    // compact query planes (the aligned start rows).  A build ahead of a pruned scan fills
    // the view's qc only and the verification expands into its qp the queries a scan pass
    // reads; every other reader of qp expands the rest first.
    rs::DevBuf<uint32_t> dQc;
    rs::DevBuf<uint32_t> dQcStream;
    // the queries last built, in the view (QueryForms) they were built into:
    bool qpFull = true;              // qp holds every start row of all of them
    bool qcValid = false;            // qc holds their compact planes
    rs::DevBuf<uint32_t> dMinLB;     // [ntb][nq]
    rs::DevBuf<uint32_t> dSecond;    // [ntb][nq] (min2 << 6) | lane of the minimum
    rs::DevBuf<int> dList;           // list1 [ntb][nq], then list2 [ntb][nq]
    size_t pruneCap = 0;             // ntb * nq the three are sized for
    rs::DevBuf<int> dTbStar;         // [nq] candidate block (~block: settled by verification)
    // [2][listCntCap] entries per list, then the verified count.  List 1's and the verified
    // count are zero between calls (vt_prune_rest_kernel); list 2's stay for
    // rs_vt_prune_stats until the next pruned launch's vt_prune_first_kernel zeroes them
    rs::DevBuf<unsigned> dListCnt;
    int listCntCap = 0;              // (dListCnt holds 2 * listCntCap + 1 words)
    rs::DevBuf<unsigned long long> dPruneStat;  // list 1's total ([0]) and the verified count ([2]) of the last pruned launch
    int64_t prunePairs = 0;          // its ntb * nq
    int prunePasses = 0;             // its scan passes (0: no pruned launch yet)
    int pruneNtb = 0;                // its template blocks (the entries of list2's counters)
    // the single list pass (RS_VT_PASSES): 1 (default) the front writes the
    // lists on U0 and one pass scans them, 2 the chain first, B1, rest, B2
    int passes = 1;
    int pruneMode = 0;               // the passes the last pruned launch ran with (the statistics' source)
    int pruneNq = 0;                 // its queries
    rs::DevBuf<uint32_t> dUblk;      // [nq] U(q): U0 of a settled query, else its candidate block's minimum
    rs::DevBuf<unsigned> dCntPar;    // [2][cntPar.cap] the single pass's list counters, by call parity
    vt_plan::ParityCounters cntPar;
    rs::DevBuf<unsigned long long> dCountAcc;  // rs_vt_prune_stats: the counting kernel's two sums
    // on-device subsampling of camera frames (rs_vt_set_subsample / rs_vt_match_frames)
    rs::DevBuf<int32_t> dPix;  // H*W byte offsets of the kept pixels in a frame
    int64_t frameBytes = 0;
    rs::DevBuf<uint8_t> dFrames;
    rs::PinnedBuf<uint8_t> hFrames;  // staging for host frames
    int frameCap = 0;
    // rs_vt_offset_profile (vt_offset.h), allocated by its first call: explicit host queries
    // (the staged batch in dQraw stays), and fine-grained arrays the kernel reads the indices
    // from and stores profile[nq][2M-1] and offset[nq] into in place
    rs::DevBuf<uint8_t> dOffQ;
    rs::PinnedBuf<int64_t> hOffIdx;
    rs::PinnedBuf<uint32_t> hOffProfile;
    rs::PinnedBuf<int32_t> hOffOffset;
    // patch normalisation (rs_vt_set_normalise, vt_norm.h): radius 0 is off.  On a normalising
    // handle every raw image is normalised on its way in, so dQraw, the library and dOffQ
    // hold normalised bytes only; these buffers take the raw bytes first and are reserved
    // on such a handle alone
    int radius = 0, gain = 0;
    rs::DevBuf<uint8_t> dNormRaw;     // (with qCap) raw uploads and gathers, normalised into dQraw
    rs::DevBuf<uint8_t> dNormStream;  // rs_vt_match_stream: a call's normalised queries (fused, host groups)
    rs::DevBuf<uint8_t> dOffRaw;      // rs_vt_offset_profile: raw host queries, normalised into dOffQ
    // the owners come after the buffers: members go in reverse order, streams and events first
    rs::Stream stream;
    rs::Event ev0, ev1;                      // around a timed scan
    rs::Stream cstream;                      // rs_vt_match_stream's collective stream (vt_ensure_comm_stream)
    rs::Event evScan, evComm;
    rs::Stream ustream;                      // rs_vt_match_stream: host batches' upload stream (vt_ensure_upload_stream)
    rs::Event evUp[2], evUsed[2];
};

namespace {

size_t tblock_bytes(const rs_vt* h) { return (size_t)h->WD * h->HQ * 64 * 16; }
size_t pblock_bytes(const rs_vt* h) { return (size_t)PL_CG * (h->H / 4) * 128 * 16; }
constexpr size_t TS_BLOCK_BYTES = 16 * 64 * sizeof(uint32_t);
int plane_ns(const rs_vt* h) { return h->H - 2 * h->M + 3; }

// Grow a slot buffer to `blocks` zeroed 64-slot blocks of `bb` bytes, keeping the first
// `keep` blocks: the new block is allocated and filled before the old one goes (the one
// growth that copies), so a failure leaves the old block and its capacity in place.
template <class T>
int vt_realloc_blocks(rs_vt* h, rs::DevBuf<T>& buf, int64_t keep, int64_t blocks, size_t bb,
                      const char* what = "template buffer growth") {
    rs::DevBuf<T> nb;
    const size_t bytes = (size_t)blocks * bb;
    RS_TRY(nb.reserve(bytes / sizeof(T), what));
    RS_HIP(hipMemsetAsync(nb.get(), 0, bytes, h->stream.get()));
    if (buf.get()) {
        if (keep > 0)
            RS_HIP(hipMemcpyAsync(nb.get(), buf.get(), (size_t)keep * bb, hipMemcpyDeviceToDevice, h->stream.get()));
        RS_HIP(hipStreamSynchronize(h->stream.get()));
    }
    buf = std::move(nb);
    return RS_OK;
}

int64_t local_count_of(const rs_vt* h, int64_t global_count) {
    return vt_plan::local_count_of(h->rank, h->nranks, global_count);
}

int vt_grow_lib(rs_vt* h, int64_t need_slots) {
    if (need_slots <= h->localCap) return RS_OK;
    const int64_t cap = (int64_t)rs::round_up((size_t)rs::grown<int64_t>(h->localCap, need_slots, 64), 64);
    RS_TRY(vt_realloc_blocks(h, h->dLib, h->localCap / 64, cap / 64, tblock_bytes(h), "template library growth"));
    if (h->planar) {
        RS_TRY(vt_realloc_blocks(h, h->dLibP, h->localCap / 64, cap / 64, pblock_bytes(h)));
        RS_TRY(vt_realloc_blocks(h, h->dLibTs, h->localCap / 64, cap / 64, TS_BLOCK_BYTES));
    }
    h->localCap = cap;
    return RS_OK;
}

// hQraw (pinned) is read by a queued copy (frames, float batches) or, for small batches,
// in place by the plane kernel: before the host writes or frees it again that work must
// have run.  Every call that stages into it waits for its keys before returning
// (vt_fetch_keys clears the flag); after an error between the staging and that wait the
// stream is synchronised here.  (rs_vt_add uploads the caller's array directly.)
int vt_qraw_idle(rs_vt* h) {
    if (h->qrawBusy) {
        RS_HIP(hipStreamSynchronize(h->stream.get()));
        h->qrawBusy = false;
    }
    return RS_OK;
}

constexpr unsigned VT_FINE = hipHostMallocMapped | hipHostMallocCoherent;

int vt_grow_queries(rs_vt* h, int nq) {
    if (nq <= h->qCap) return RS_OK;
    const int cap = rs::grown(h->qCap, nq, 64);
    RS_TRY(vt_qraw_idle(h));
    h->qCap = 0;
    h->bestClean = h->bestPending = 0;
    const size_t qb = (size_t)h->H * h->W, n = (size_t)cap;
    if (h->planar) {
        RS_TRY(h->dQp.reserve((size_t)PL_CG * plane_ns(h) * 8 * n));
        RS_TRY(h->dQsumRaw.reserve(n));
        if (h->prune) RS_TRY(h->dQsj.reserve((size_t)PF_NU * 16 * n));
        if (h->prune) RS_TRY(h->dQc.reserve((size_t)QC_Q4 * 4 * n));
    }
    RS_TRY(h->dQraw.reserve(qb * n));
    if (h->radius > 0) RS_TRY(h->dNormRaw.reserve(qb * n));
    RS_TRY(h->hQraw.reserve(qb * n, VT_FINE));
    RS_TRY(h->dQf.reserve((size_t)h->WD * h->H * n));
    RS_TRY(h->dQsum.reserve(n));
    RS_TRY(h->dBest.reserve(n));
    RS_TRY(h->hBest.reserve(n, VT_FINE));
    h->qCap = cap;
    return RS_OK;
}

int vt_grow_index(rs_vt* h, int n) {
    if (n <= h->idxCap) return RS_OK;
    const int cap = rs::grown(h->idxCap, n, 64);
    h->idxCap = 0;
    RS_TRY(h->dSrc.reserve((size_t)cap));
    RS_TRY(h->dDst.reserve((size_t)cap));
    RS_TRY(h->hSrc.reserve((size_t)cap, hipHostMallocDefault));
    RS_TRY(h->hDst.reserve((size_t)cap, hipHostMallocDefault));
    h->idxCap = cap;
    return RS_OK;
}

int vt_grow_matrix(rs_vt* h, size_t elems) {
    if (elems <= h->matCap) return RS_OK;
    const size_t cap = rs::grown<size_t>(h->matCap, elems, 4096);
    h->matCap = 0;
    RS_TRY(h->dMat.reserve(cap));
    RS_TRY(h->hMat.reserve(cap, hipHostMallocDefault));
    h->matCap = cap;
    return RS_OK;
}

int vt_grow_cand(rs_vt* h, int64_t slots) {
    if (slots <= h->candCap) return RS_OK;
    const int64_t cap = rs::grown<int64_t>(h->candCap, slots, 64);
    h->candCap = 0;
    RS_TRY(h->dCand.reserve((size_t)(cap / 64) * tblock_bytes(h) / sizeof(uint4)));
    if (h->planar) {
        RS_TRY(vt_realloc_blocks(h, h->dCandP, 0, cap / 64, pblock_bytes(h)));
        RS_TRY(vt_realloc_blocks(h, h->dCandTs, 0, cap / 64, TS_BLOCK_BYTES));
    }
    h->candCap = cap;
    return RS_OK;
}

QueryForms vt_batch_view(const rs_vt* h) {
    return {h->dQp.get(), h->dQsumRaw.get(), h->dQsj.get(), h->dQc.get()};
}

// The forms of rs_vt_match_stream's queries from query q0 on.
QueryForms vt_stream_view(const rs_vt* h, size_t q0) {
    const size_t qpq = (size_t)PL_CG * plane_ns(h) * 8;  // plane dwords per query
    QueryForms v{h->dQpStream.get() + qpq * q0, h->dQsumStream.get() + q0, nullptr, nullptr};
    if (h->dQsjStream.get()) v.qsj = h->dQsjStream.get() + (size_t)PF_NU * 16 * q0;
    if (h->dQcStream.get()) v.qc = h->dQcStream.get() + (size_t)QC_Q4 * 4 * q0;
    return v;
}

int vt_build_forms(rs_vt* h, const QueryForms& q, int nq);

// Whether a scan of nq queries (forms in q) against `count` slots from block tb0 takes the
// pruned path (vt_plan::prunes).
bool vt_prunes(const rs_vt* h, const QueryForms& q, bool cand, int64_t tb0, int64_t count, int nq) {
    return vt_plan::prunes(h->H, cand, tb0, q.qsj && q.qc, (count + 63) / 64, h->prune, nq);
}
// The plane build ahead of a key scan of the library: compact where that scan will prune.
// A wrong guess costs a conversion launch (vt_launch_plane), never a result.
// Threads of a compact build's block: phase 2 has 52 units to assemble, and two waves per
// query measured faster than four and level with one (15.8, 12.9 and 13.7 us at the
// headline shape).
constexpr int VT_QC_THREADS = 128;
uint32_t* vt_compact_for(rs_vt* h, const QueryForms& q, int nq) {
    const int64_t lc = local_count_of(h, h->count);
    const bool compact = h->planar && lc > 0 && vt_prunes(h, q, false, 0, lc, nq);
    h->qpFull = !compact;
    h->qcValid = compact;
    return compact ? q.qc : nullptr;
}

// Normalise n raw images at src (device memory, or pinned memory by its device address) into
// dst on the handle's stream: the only launch of vt_normalise_kernel, for handles with
// radius > 0.
int vt_normalise(rs_vt* h, const uint8_t* src, uint8_t* dst, size_t n) {
    const int tx = (h->W + VTN_T - 1) / VTN_T, ty = (h->H + VTN_T - 1) / VTN_T;
    hipLaunchKernelGGL(vt_normalise_kernel, dim3((unsigned)(tx * ty), (unsigned)std::min<size_t>(n, 65535)),
                       dim3(VTN_THREADS), 0, h->stream.get(), src, dst, (int)n, h->H, h->W, h->radius, h->gain, tx);
    RS_HIP(hipGetLastError());
    return RS_OK;
}

// RS_VT_ZC=0: no batch is read in place from the pinned staging array (vt_plan::stages_in_place).
bool vt_zc_env() { static const bool on = rs::env_on("RS_VT_ZC"); return on; }

// Upload nq raw queries and build their forms (the batch view) on the device.
int vt_stage_queries(rs_vt* h, int nq, const uint8_t* queries) {
    RS_TRY(vt_grow_queries(h, nq));
    RS_TRY(vt_qraw_idle(h));
    const QueryForms q = vt_batch_view(h);
    const size_t qb = (size_t)h->H * h->W * nq;
    if (h->radius > 0) {   // raw bytes into the handle's own buffer, normalised into dQraw
        RS_HIP(hipMemcpyAsync(h->dNormRaw.get(), queries, qb, hipMemcpyHostToDevice, h->stream.get()));
        RS_TRY(vt_normalise(h, h->dNormRaw.get(), h->dQraw.get(), (size_t)nq));
        return vt_build_forms(h, q, nq);
    }
    // larger batches: HIP's own upload of the caller's (pageable) array, which returns
    // once the bytes are staged (per-batch PCIe-inclusive rate 4.04-4.12 against 3.44-3.54
    // G compares/s through our memcpy into pinned staging, round 5).  The call waits for
    // its keys, which the scan stores after the copy has run, so a pinned caller array is
    // no longer read when it returns.
    if (vt_plan::stages_in_place(h->planar, nq, vt_zc_env())) {
        std::memcpy(h->hQraw.get(), queries, qb);
        h->qrawBusy = true;
        uint32_t* const qc = vt_compact_for(h, q, nq);
        hipLaunchKernelGGL(vt_qplane_kernel, dim3(nq), dim3(qc ? VT_QC_THREADS : 256), 0, h->stream.get(), h->hQraw.dev(), h->H,
                           h->M, q.qp, q.qsum, h->dQraw.get(), q.qsj, qc);
        RS_HIP(hipGetLastError());
        return RS_OK;
    }
    RS_HIP(hipMemcpyAsync(h->dQraw.get(), queries, qb, hipMemcpyHostToDevice, h->stream.get()));
    return vt_build_forms(h, q, nq);
}

// Build the query forms of nq raw queries in device memory (default: dQraw) into the view q.
// The plane scan reads only the planes; the byte-SWAR forms serve the other scans.
int vt_build_forms(rs_vt* h, const QueryForms& q, int nq, const uint8_t* src) {
    if (h->metric == RS_VT_METRIC_SAD)
        hipLaunchKernelGGL(vt_qform_sad_kernel, dim3(nq), dim3(256), 0, h->stream.get(), src, h->H, h->W, h->WD,
                           reinterpret_cast<uint32_t*>(h->dQf.get()));
    else if (!h->planar)
        hipLaunchKernelGGL(vt_qform_kernel, dim3(nq), dim3(256), 0, h->stream.get(), src, h->H, h->W,
                           h->WD, h->M, h->dQf.get(), h->dQsum.get());
    else {
        uint32_t* const qc = vt_compact_for(h, q, nq);
        hipLaunchKernelGGL(vt_qplane_kernel, dim3(nq), dim3(qc ? VT_QC_THREADS : 256), 0, h->stream.get(), src, h->H,
                           h->M, q.qp, q.qsum, nullptr, q.qsj, qc);
    }
    RS_HIP(hipGetLastError());
    return RS_OK;
}

int vt_build_forms(rs_vt* h, const QueryForms& q, int nq) { return vt_build_forms(h, q, nq, h->dQraw.get()); }

// Subsample nf frames on the device into the raw query buffer, then build the
// forms.  Host frames go through a pinned staging buffer; device-resident frames
// (a camera / decoder pipeline on the GPU) are gathered in place.
int vt_stage_frames(rs_vt* h, int nf, const uint8_t* frames) {
    RS_CHECK(h->dPix.get(), RS_ERR_STATE, "no subsampling mask: call rs_vt_set_subsample first");
    RS_TRY(vt_grow_queries(h, nf));
    const bool on_device = rs::on_device(frames);
    const uint8_t* src = frames;
    if (!on_device) {
        if (nf > h->frameCap) {
            const int cap = rs::grown(h->frameCap, nf, 16);
            h->frameCap = 0;
            RS_TRY(h->dFrames.reserve((size_t)h->frameBytes * cap));
            RS_TRY(h->hFrames.reserve((size_t)h->frameBytes * cap, hipHostMallocDefault));
            h->frameCap = cap;
        }
        const size_t fb = (size_t)h->frameBytes * nf;
        std::memcpy(h->hFrames.get(), frames, fb);
        RS_HIP(hipMemcpyAsync(h->dFrames.get(), h->hFrames.get(), fb, hipMemcpyHostToDevice, h->stream.get()));
        src = h->dFrames.get();
    }
    hipLaunchKernelGGL(vt_gather_kernel, dim3(nf), dim3(256), 0, h->stream.get(), src,
                       (size_t)h->frameBytes, h->dPix.get(), h->H * h->W,
                       h->radius > 0 ? h->dNormRaw.get() : h->dQraw.get());
    RS_HIP(hipGetLastError());
    if (h->radius > 0) RS_TRY(vt_normalise(h, h->dNormRaw.get(), h->dQraw.get(), (size_t)nf));
    return vt_build_forms(h, vt_batch_view(h), nf);
}

// Store raw staged queries src[i] into slots dst[i] of the library (or, with
// `cand`, of the candidate buffer).
int vt_store(rs_vt* h, bool cand, const uint8_t* d_raw, int n) {
    if (n == 0) return RS_OK;
    uint4* lib = cand ? h->dCand.get() : h->dLib.get();
    RS_HIP(hipMemcpyAsync(h->dSrc.get(), h->hSrc.get(), sizeof(int32_t) * n, hipMemcpyHostToDevice, h->stream.get()));
    RS_HIP(hipMemcpyAsync(h->dDst.get(), h->hDst.get(), sizeof(int64_t) * n, hipMemcpyHostToDevice, h->stream.get()));
    h->stagingBusy = true;
    const int64_t total = (int64_t)n * h->WD * h->HQ;
    const int grid = (int)std::min<int64_t>((total + 255) / 256, 4096);
    hipLaunchKernelGGL(vt_store_kernel, dim3(grid), dim3(256), 0, h->stream.get(), d_raw, h->dSrc.get(),
                       h->dDst.get(), n, lib, h->H, h->W, h->WD, h->HQ);
    if (h->planar)
        hipLaunchKernelGGL(vt_plane_store_kernel, dim3(n), dim3(256), 0, h->stream.get(), d_raw, h->dSrc.get(),
                           h->dDst.get(), h->H, h->M, cand ? h->dCandP.get() : h->dLibP.get(),
                           cand ? h->dCandTs.get() : h->dLibTs.get());
    RS_HIP(hipGetLastError());
    return RS_OK;
}

// f(Int<64>{}) or f(Int<32>{}): the kernel instance for the handle's template height
// (the scans with an H parameter exist for these two; every other shape is generic).
template <class F>
__attribute__((always_inline)) inline auto vt_by_h(const rs_vt* h, F&& f) {
    return h->H == 64 ? f(rs::Int<64>{}) : f(rs::Int<32>{});
}

// RS_VT_NQC (A/B, read at every launch): blocks per template block in place of
// vt_plan::plane_split's model; 0: unset.
int vt_nqc_env() {
    const char* e = std::getenv("RS_VT_NQC");
    return e ? std::max(1, std::atoi(e)) : 0;
}

// An A/B switch of the environment (read once, at create) with the grammar 0 | 1 | force:
// *out = 0, 1 (also unset or empty) or 2.
int vt_env_switch(const char* name, int* out) {
    const char* e = std::getenv(name);
    if (!e || e[0] == 0 || std::strcmp(e, "1") == 0) *out = 1;
    else if (std::strcmp(e, "force") == 0) *out = 2;
    else {
        RS_CHECK(std::strcmp(e, "0") == 0, RS_ERR_ARG, "%s='%s': expected 0, 1 or force", name, e);
        *out = 0;
    }
    return RS_OK;
}

// The only launch of vt_keys_export: n keys -> host (pinned, device address), reset behind it.
void vt_launch_keys_export(rs_vt* h, unsigned long long* keys, int n, unsigned long long* host, int max_blocks) {
    hipLaunchKernelGGL(vt_keys_export, dim3((unsigned)vt_plan::export_grid(n, max_blocks)), dim3(256), 0, h->stream.get(),
                       keys, n, host);
}

// One plane scan launch: its grid, the template planes and sums from block tb0 on, the queries.
struct PlaneScan {
    dim3 grid;
    const uint4* planes;
    const uint32_t* ts;
    int ntb;
    int64_t count;
    const QueryForms& q;
    int nq, nqc, rank, nranks;
};
template <int H, bool MATRIX, bool LIST>
void vt_launch_plane_scan(rs_vt* h, const PlaneScan& s, const ScanOut& out, const PlaneListArg<LIST>& list) {
    hipLaunchKernelGGL((vt_scan_plane_kernel<H, MATRIX, LIST>), s.grid, dim3(64 * PL_CG * PL_SPLIT), 0, h->stream.get(),
                       s.planes, s.ts, s.ntb, s.count, s.q.qp, s.q.qsum, s.nq, s.nqc, h->dCtr.get(), out, s.rank,
                       s.nranks, list);
}

// The pruned scan's buffers for ntb template blocks x nq queries.
int vt_ensure_prune_buffers(rs_vt* h, int ntb, int nq) {
    const size_t pairs = (size_t)ntb * nq;
    if (pairs > h->pruneCap) {
        const size_t cap = std::max(pairs, 2 * h->pruneCap);
        h->pruneCap = 0;
        RS_TRY(h->dMinLB.reserve(cap));
        RS_TRY(h->dSecond.reserve(cap));
        RS_TRY(h->dList.reserve(2 * cap));
        h->pruneCap = cap;
    }
    RS_TRY(h->dTbStar.reserve((size_t)nq));  // (exact)
    RS_TRY(h->dUblk.reserve((size_t)nq));
    if (vt_plan::parity_grows(h->cntPar, ntb)) {   // zero at first; every call zeroes the other parity's
        vt_plan::ParityCounters grown = h->cntPar;
        vt_plan::parity_grown(grown, ntb);
        h->cntPar = vt_plan::ParityCounters{};
        RS_TRY(h->dCntPar.reserve(2 * (size_t)grown.cap));
        RS_HIP(hipMemsetAsync(h->dCntPar.get(), 0, sizeof(unsigned) * 2 * (size_t)grown.cap, h->stream.get()));
        grown.par = 0;
        h->cntPar = grown;
    }
    if (ntb > h->listCntCap) {  // zero at first; the list kernels zero what they are about to fill
        const int cap = std::max(ntb, 2 * h->listCntCap);
        h->listCntCap = 0;
        RS_TRY(h->dListCnt.reserve(2 * (size_t)cap + 1));
        RS_HIP(hipMemsetAsync(h->dListCnt.get(), 0, sizeof(unsigned) * (2 * (size_t)cap + 1), h->stream.get()));
        h->listCntCap = cap;
    }
    if (!h->dPruneStat.get()) {
        RS_TRY(h->dPruneStat.reserve(3));
        RS_HIP(hipMemsetAsync(h->dPruneStat.get(), 0, 3 * sizeof(unsigned long long), h->stream.get()));
    }
    return RS_OK;
}

// Pruned scan of the frozen library (vt_prunes): prefilter and verification (one launch where
// vt_plan::front_fused), then one list pass over the lists the verification wrote on U0, or,
// with two passes (RS_VT_PASSES=2), the scan of each query's candidate block (list 1, pass B1)
// and of the blocks its bound leaves (list 2, pass B2).
int vt_launch_pruned(rs_vt* h, const PlaneScan& s, const ScanOut& out) {
    const QueryForms& q = s.q;
    const int ntb = s.ntb, nq = s.nq;
    if (!h->qcValid) {   // the build before did not expect this scan to prune
        hipLaunchKernelGGL(vt_qcompact_kernel, dim3((unsigned)nq), dim3(128), 0, h->stream.get(),
                           reinterpret_cast<const uint4*>(q.qp), reinterpret_cast<uint4*>(q.qc));
        h->qcValid = true;
    }
    RS_TRY(vt_ensure_prune_buffers(h, ntb, nq));
    const size_t pairs = (size_t)ntb * nq;
    unsigned* cnt1 = h->dListCnt.get();
    unsigned* cnt2 = h->dListCnt.get() + h->listCntCap;
    unsigned* verified = h->dListCnt.get() + 2 * (size_t)h->listCntCap;
    int* list1 = h->dList.get();
    int* list2 = h->dList.get() + pairs;
    const bool single = vt_plan::prune_passes(h->passes, ntb, nq) == 1;
    FrontLists fl{};
    if (single) {
        const vt_plan::ParityCall pc = vt_plan::parity_begin(h->cntPar, ntb);
        fl = FrontLists{h->dCntPar.get() + pc.mine, list1, h->dUblk.get(), h->dCntPar.get() + pc.other, pc.nzero};
    }
    if (h->front == 2 || (h->front == 1 && vt_plan::front_fused(ntb, PF_WAVES * PF_TPW))) {
        const vt_plan::Grid2 fg = vt_plan::front_grid(nq, PF_NB, VT_PF_GRID_CAP);
        hipLaunchKernelGGL(vt_front_kernel, dim3((unsigned)fg.x, (unsigned)fg.y), dim3(64 * PF_WAVES), 0, h->stream.get(),
                           s.planes, ntb, s.count, reinterpret_cast<const uint4*>(q.qc), q.qsj, nq, h->dMinLB.get(),
                           s.ts, reinterpret_cast<uint4*>(q.qp), q.qsum, out.best, s.rank, s.nranks,
                           h->dTbStar.get(), fl);
    } else {
        const vt_plan::Grid2 pf = vt_plan::prefilter_grid(ntb, nq, PF_WAVES * PF_TPW, PF_NB, VT_PF_GRID_CAP);
        hipLaunchKernelGGL(vt_prefilter_kernel, dim3((unsigned)pf.x, (unsigned)pf.y), dim3(64 * PF_WAVES), 0,
                           h->stream.get(), s.planes, ntb, s.count, reinterpret_cast<const uint4*>(q.qc), q.qsj, nq,
                           h->dMinLB.get(), h->dSecond.get(), fl);
        hipLaunchKernelGGL(vt_prune_verify_kernel, dim3((unsigned)nq), dim3(64), 0, h->stream.get(), h->dMinLB.get(),
                           h->dSecond.get(), ntb, nq, s.planes, s.ts, reinterpret_cast<const uint4*>(q.qc),
                           reinterpret_cast<uint4*>(q.qp), q.qsum, out.best, s.rank, s.nranks, h->dTbStar.get(), fl);
    }
    // the passes min into the same keys; the folded export (out.host) needs one
    // launch to be the last, so a pruned call exports with vt_keys_export
    ScanOut po = out;
    po.host = nullptr;
    po.done = nullptr;
    // working blocks per template block that make one resident round (vt_plan::list_width)
    const uint32_t fill = (uint32_t)std::min(65535, std::max(1, h->planeSlots / ntb));
    const uint32_t lnb = (uint32_t)h->listNb;
#ifdef VT_LIST_PER
    const int per2 = VT_LIST_PER;
#else
    const int per2 = vt_plan::list_per(ntb, h->planeSlots);
#endif
    h->prunePairs = (int64_t)pairs;
    h->prunePasses = 2;   // (the statistics are the two-pass rule's in either mode)
    h->pruneNtb = ntb;
    h->pruneNq = nq;
    h->pruneMode = single ? 1 : 2;
    if (single) {   // pass B2's settings over the one list, but its width chosen for four resident
        // rounds of blocks (vt_plan::single_pass_fill); the candidate block's wave stores U(q)
        const uint32_t fill1 = (uint32_t)vt_plan::single_pass_fill((int)fill);
        vt_launch_plane_scan<64, false, true>(
            h, s, po, PlaneListU{{list1, fl.cnt, nq, (uint32_t)per2, lnb, 0u, fill1}, h->dTbStar.get(), h->dUblk.get()});
        if (out.host) vt_launch_keys_export(h, out.best, nq, out.host, vt_plan::VT_EXPORT_BLOCKS);
        RS_HIP(hipGetLastError());
        return RS_OK;
    }
    const dim3 lgrid((unsigned)((nq + VT_LIST_T - 1) / VT_LIST_T), (unsigned)ntb);
    hipLaunchKernelGGL(vt_prune_first_kernel, lgrid, dim3(VT_LIST_T), 0, h->stream.get(), nq, h->dTbStar.get(), cnt1,
                       list1, verified, cnt2, ntb);
    vt_launch_plane_scan<64, false, true>(h, s, po,
                                          PlaneListU{{list1, cnt1, nq, (uint32_t)VT_LIST_PER_B1, lnb, 1u, fill}});
    hipLaunchKernelGGL(vt_prune_rest_kernel, lgrid, dim3(VT_LIST_T), 0, h->stream.get(), h->dMinLB.get(), nq,
                       h->dTbStar.get(), out.best, cnt2, list2, cnt1, verified, ntb, h->dPruneStat.get());
    vt_launch_plane_scan<64, false, true>(h, s, po, PlaneListU{{list2, cnt2, nq, (uint32_t)per2, lnb, 0u, fill}});
    if (out.host) vt_launch_keys_export(h, out.best, nq, out.host, vt_plan::VT_EXPORT_BLOCKS);
    RS_HIP(hipGetLastError());
    return RS_OK;
}

// Launch a scan of queries [0, nq) (forms in the view q) against `count` slots of lib.
template <bool MATRIX>
int vt_launch_plane(rs_vt* h, const QueryForms& q, bool cand, int64_t count, int nq, ScanOut out, int rank,
                    int nranks, int64_t tb0) {
    const int ntb = (int)((count + 63) / 64);
    const int nqc = vt_plan::plane_split(ntb, (nq + PL_NB - 1) / PL_NB, h->planeSlots, vt_nqc_env());
    if (8 * (size_t)ntb > h->dCtr.capacity()) {  // counters start at zero and every scan leaves them at zero
        const size_t cap = std::max(8 * (size_t)ntb, 2 * h->dCtr.capacity());
        RS_TRY(h->dCtr.reserve(cap));
        RS_HIP(hipMemsetAsync(h->dCtr.get(), 0, sizeof(unsigned) * cap, h->stream.get()));
    }
    RS_CHECK((int64_t)ntb * nqc < (1ll << 31), RS_ERR_ARG, "scan grid too large");
    const uint4* planes = reinterpret_cast<const uint4*>(
        reinterpret_cast<const uint8_t*>(cand ? h->dCandP.get() : h->dLibP.get()) + (size_t)tb0 * pblock_bytes(h));
    const uint32_t* ts = (cand ? h->dCandTs.get() : h->dLibTs.get()) + (size_t)tb0 * (TS_BLOCK_BYTES / 4);
    const PlaneScan s{dim3((unsigned)(ntb * nqc)), planes, ts, ntb, count, q, nq, nqc, rank, nranks};
    if constexpr (!MATRIX)
        if (vt_prunes(h, q, cand, tb0, count, nq)) return vt_launch_pruned(h, s, out);
    if (!h->qpFull) {   // a compact build, and a scan that reads every query's planes
        hipLaunchKernelGGL(vt_qexpand_kernel, dim3((unsigned)nq), dim3(256), 0, h->stream.get(),
                           reinterpret_cast<const uint4*>(q.qc), reinterpret_cast<uint4*>(q.qp));
        h->qpFull = true;
    }
    vt_by_h(h, [&](auto H) { vt_launch_plane_scan<decltype(H)::value, MATRIX, false>(h, s, out, PlaneList{}); });
    RS_HIP(hipGetLastError());
    return RS_OK;
}

// A scan under the true-SAD metric: the fast form or the generic one (vt_plan::sad_fast).
template <bool MATRIX>
int vt_launch_sad(rs_vt* h, const uint4* lib, int ntb, int64_t count, int nq, ScanOut out, int rank, int nranks) {
    const uint32_t* qd = reinterpret_cast<const uint32_t*>(h->dQf.get());
    if (vt_plan::sad_fast(h->H, h->M)) {
        const int nqc = vt_plan::sad_split(ntb, (nq + SAD_NQ - 1) / SAD_NQ);
        RS_CHECK((int64_t)ntb * nqc < (1ll << 31), RS_ERR_ARG, "scan grid too large (%d x %d)", ntb, nqc);
        vt_by_h(h, [&](auto H) {
            hipLaunchKernelGGL((vt_scan_sad_kernel<decltype(H)::value, MATRIX>), dim3((unsigned)(ntb * nqc)),
                               dim3(64 * vt_plan::sad_waves(h->WD)), 0, h->stream.get(), lib, ntb, count, h->WD, qd, nq,
                               nqc, out, rank, nranks);
        });
    } else {
        hipLaunchKernelGGL((vt_scan_sad_generic_kernel<MATRIX>), dim3((unsigned)(ntb * nq)), dim3(64), 0, h->stream.get(),
                           lib, ntb, count, h->H, h->M, h->WD, qd, nq, out, rank, nranks);
    }
    RS_HIP(hipGetLastError());
    return RS_OK;
}

// Launch a scan of queries [0, nq) against `count` slots of the library (or of
// the candidate buffer), starting at 64-slot block tb0 of it (q: the plane scan's forms).
template <bool MATRIX>
int vt_launch_scan(rs_vt* h, const QueryForms& q, bool cand, int64_t count, int nq, ScanOut out, int rank,
                   int nranks, int64_t tb0 = 0) {
    if (count <= 0 || nq <= 0) return RS_OK;
    if (h->planar) return vt_launch_plane<MATRIX>(h, q, cand, count, nq, out, rank, nranks, tb0);
    const uint4* lib = (cand ? h->dCand.get() : h->dLib.get()) + (size_t)tb0 * h->WD * h->HQ * 64;
    const int ntb = (int)((count + 63) / 64);
    const bool fast = h->M == FAST_M && (h->H == 64 || h->H == 32);
    RS_CHECK((int64_t)ntb * nq < (1ll << 31), RS_ERR_ARG, "scan grid too large (%d x %d)", ntb, nq);
    if (h->metric == RS_VT_METRIC_SAD) return vt_launch_sad<MATRIX>(h, lib, ntb, count, nq, out, rank, nranks);
    if (fast && !MATRIX && (int64_t)ntb * nq < 2048 && h->WD <= 8) {
        // few waves of work: spread each template over 8 column lanes
        const dim3 grid((unsigned)((count + 7) / 8), nq);
        vt_by_h(h, [&](auto H) {
            hipLaunchKernelGGL((vt_scan_carry_col_kernel<decltype(H)::value, 1>), grid, dim3(64), 0, h->stream.get(), lib,
                               count, h->WD, h->dQf.get(), h->dQsum.get(), nq, out, rank, nranks);
        });
    } else if (fast) {
        constexpr int NQ = 2;
        const int nqg = (nq + NQ - 1) / NQ;
        const dim3 grid((unsigned)(ntb * ((nqg + 7) / 8) * 8));
        vt_by_h(h, [&](auto H) {
            hipLaunchKernelGGL((vt_scan_carry_kernel<decltype(H)::value, NQ, MATRIX>), grid, dim3(64), 0, h->stream.get(),
                               lib, ntb, count, h->WD, h->dQf.get(), h->dQsum.get(), nq, out, rank, nranks);
        });
    } else {
        hipLaunchKernelGGL((vt_scan_generic_kernel<MATRIX>), dim3((unsigned)(ntb * nq)), dim3(64),
                           0, h->stream.get(), lib, ntb, count, h->H, h->M, h->WD, h->dQf.get(), nq, out, rank,
                           nranks);
    }
    RS_HIP(hipGetLastError());
    return RS_OK;
}

// The host waits for a call's keys by polling them (pinned, fine-grained; each key one
// 8-byte system-scope store by vt_keys_export, the call's last kernel) instead of the
// stream's completion signal and its own wake-up: the host reads nothing else the call
// wrote, and every later device access is ordered on the stream (the pinned staging
// arrays a call's copies read are guarded by vt_staging_idle).  A spin that runs out
// falls back to the stream synchronisation.  RS_VT_POLL=0: always synchronise.
constexpr unsigned long long KEY_PENDING = 0xFFFFFFFF00000000ull;  // score 2^32-1: never a key
bool vt_poll_env() { static const bool on = rs::env_on("RS_VT_POLL"); return on; }
bool vt_poll_keys(const unsigned long long* w_, int n) {
    const volatile unsigned long long* w = w_;
    return rs::spin_until(n, [w](int i) { return w[i] != KEY_PENDING; });
}

// The pinned staging arrays hSrc / hDst are read by asynchronous copies (vt_store):
// before the host writes or reallocates them again, those copies must have run.
int vt_staging_idle(rs_vt* h) {
    if (h->stagingBusy) {
        RS_HIP(hipStreamSynchronize(h->stream.get()));
        h->stagingBusy = false;
    }
    return RS_OK;
}

// Min-reduce n keys in place over the handle's communicator, queued on `stream`.
int vt_allreduce_min(rs_vt* h, unsigned long long* buf, size_t n, hipStream_t stream) {
    ncclResult_t r = ncclAllReduce(buf, buf, n, ncclUint64, ncclMin, h->comm, stream);
    RS_CHECK(r == ncclSuccess, RS_ERR_RCCL, "ncclAllReduce(min) failed: %s", ncclGetErrorString(r));
    return RS_OK;
}

// run() between the events ev0 and ev1 when `timed` (rs_vt_last_ms reads them once the
// stream has run); timedScan says whether the last scan was.
template <class Run>
int vt_timed_scan(rs_vt* h, bool timed, Run run) {
    if (timed) RS_HIP(hipEventRecord(h->ev0.get(), h->stream.get()));
    RS_TRY(run());
    if (timed) RS_HIP(hipEventRecord(h->ev1.get(), h->stream.get()));
    h->timedScan = timed;
    return RS_OK;
}

// Packed keys -> (index, score) of a frozen match; NO_KEY (an empty library): (-1, UINT64_MAX).
void vt_decode_keys(const unsigned long long* key, size_t n, uint64_t* best_score, int64_t* best_index) {
    for (size_t i = 0; i < n; ++i) {
        const unsigned long long k = key[i];   // (read once: the outputs may alias it for all the compiler knows)
        if (best_index) best_index[i] = k == NO_KEY ? -1 : (int64_t)(k & 0xFFFFFFFFull);
        if (best_score) best_score[i] = k == NO_KEY ? UINT64_MAX : (k >> 32);
    }
}

int vt_append_staged(rs_vt* h, const std::vector<std::pair<int, int64_t>>& news) {
    // news: (staged query index, global index) in order
    int mine = 0;
    RS_TRY(vt_staging_idle(h));
    RS_TRY(vt_grow_index(h, (int)news.size() + 1));
    const int64_t new_count = h->count + (int64_t)news.size();
    RS_TRY(vt_grow_lib(h, local_count_of(h, new_count)));
    for (const auto& p : news) {
        if (p.second % h->nranks != h->rank) continue;
        h->hSrc.get()[mine] = p.first;
        h->hDst.get()[mine] = p.second / h->nranks;
        ++mine;
    }
    RS_TRY(vt_store(h, false, h->dQraw.get(), mine));
    h->count = new_count;
    return RS_OK;
}

// Stage nq queries (raw H x W, or whole frames subsampled on the device) and
// min-reduce their local first-argmin keys into dBest.
int vt_scan_local_impl(rs_vt* h, int nq, const uint8_t* queries, bool frames = false, bool fold_ok = true) {
    RS_CHECK(h, RS_ERR_STATE, "null view-template handle");
    RS_CHECK(nq >= 0, RS_ERR_ARG, "negative query count");
    if (nq == 0) return RS_OK;
    RS_HIP(hipSetDevice(h->device));
    if (frames) {
        RS_CHECK(queries, RS_ERR_ARG, "null frames");
        RS_TRY(vt_stage_frames(h, nq, queries));
    } else if (queries) {
        RS_TRY(vt_stage_queries(h, nq, queries));
    } else {
        // re-match the queries already resident on the device (last staged batch)
        RS_CHECK(nq == h->stagedQ, RS_ERR_STATE, "no staged batch of %d queries (have %d)", nq,
                 h->stagedQ);
    }
    if (h->bestClean < nq) {  // vt_keys_export resets the keys it hands over
        RS_HIP(hipMemsetAsync(h->dBest.get(), 0xFF, sizeof(unsigned long long) * nq, h->stream.get()));
        h->bestClean = nq;
    }
    h->bestPending = h->bestClean;  // [0, nq) is dirty until exported; the rest stays clean
    h->bestClean = 0;
    const int64_t lc = local_count_of(h, h->count);
    ScanOut out{h->dBest.get(), nullptr, 0};
    // a plane scan whose keys the host polls exports them itself (vt_plan::folds_keys)
    h->keysFolded = vt_plan::folds_keys(fold_ok, h->planar, lc, vt_poll_env(), h->timing, nq);
    if (h->keysFolded) {
        if (!h->dDone.get()) {
            RS_TRY(h->dDone.reserve(1));
            RS_HIP(hipMemsetAsync(h->dDone.get(), 0, sizeof(unsigned), h->stream.get()));
        }
        for (int i = 0; i < nq; ++i) h->hBest.get()[i] = KEY_PENDING;
        out.host = h->hBest.dev();
        out.done = h->dDone.get();
    }
    RS_TRY(vt_timed_scan(h, h->timing, [&] {
        return vt_launch_scan<false>(h, vt_batch_view(h), false, lc, nq, out, h->rank, h->nranks);
    }));
    h->stagedQ = nq;
    return RS_OK;
}

// Given the global keys of the staged queries, decide hits / new templates in
// ViewTemplates.match order and append the new templates this rank owns.
int vt_resolve_impl(rs_vt* h, int nq, const unsigned long long* keys, int mode,
                    uint64_t* best_score, int64_t* best_index, uint8_t* is_new) {
    RS_CHECK(h, RS_ERR_STATE, "null view-template handle");
    RS_CHECK(mode == RS_VT_FROZEN || mode == RS_VT_SEQUENTIAL, RS_ERR_ARG, "unknown mode %d", mode);
    RS_CHECK(nq == h->stagedQ, RS_ERR_STATE, "resolve of %d queries, %d staged", nq, h->stagedQ);
    if (nq == 0) return RS_OK;
    RS_CHECK(keys, RS_ERR_ARG, "null keys");
    RS_HIP(hipSetDevice(h->device));
    std::vector<unsigned long long> key(keys, keys + nq);
    if (mode == RS_VT_FROZEN) {
        if (is_new) std::memset(is_new, 0, (size_t)nq);
        vt_decode_keys(key.data(), (size_t)nq, best_score, best_index);
        return RS_OK;
    }
    // Candidates: queries that miss the stored library.  Only they can become
    // templates; a later query may still prefer one of them (first argmin over
    // the grown list, view_templates.py:65-73), so every candidate is scored as
    // a template against every query once (replicated on all ranks).
    std::vector<int> cand;
    for (int i = 0; i < nq; ++i)
        if (key[i] == NO_KEY || (double)(key[i] >> 32) > h->thr) cand.push_back(i);
    std::vector<int> cpos(nq, -1);
    int64_t ldm = 0;
    if (!cand.empty() && cand.front() < nq - 1) {
        RS_TRY(vt_staging_idle(h));
        const int64_t C = (int64_t)cand.size();
        RS_TRY(vt_grow_cand(h, (int64_t)rs::round_up((size_t)C, 64)));
        RS_TRY(vt_grow_index(h, (int)C));
        for (int64_t j = 0; j < C; ++j) {
            h->hSrc.get()[j] = cand[j];
            h->hDst.get()[j] = j;
            cpos[cand[j]] = (int)j;
        }
        RS_TRY(vt_store(h, true, h->dQraw.get(), (int)C));
        ldm = (int64_t)rs::round_up((size_t)C, 64);
        RS_TRY(vt_grow_matrix(h, (size_t)ldm * nq));
        ScanOut mo{nullptr, h->dMat.get(), ldm};
        RS_TRY(vt_launch_scan<true>(h, vt_batch_view(h), true, C, nq, mo, 0, 1));
        RS_HIP(hipMemcpyAsync(h->hMat.get(), h->dMat.get(), sizeof(uint32_t) * ldm * nq, hipMemcpyDeviceToHost,
                              h->stream.get()));
        RS_HIP(hipStreamSynchronize(h->stream.get()));
        h->stagingBusy = false;
    }
    std::vector<std::pair<int, int64_t>> news;
    for (int i = 0; i < nq; ++i) {
        unsigned long long k = key[i];
        for (size_t a = 0; a < news.size(); ++a) {
            const int j = news[a].first;
            const unsigned long long kj =
                ((unsigned long long)h->hMat.get()[(size_t)i * ldm + cpos[j]] << 32) |
                (unsigned long long)news[a].second;
            k = kj < k ? kj : k;
        }
        if (k == NO_KEY || (double)(k >> 32) > h->thr) {
            const int64_t g = h->count + (int64_t)news.size();
            news.emplace_back(i, g);
            if (is_new) is_new[i] = 1;
            if (best_index) best_index[i] = g;
        } else {
            if (is_new) is_new[i] = 0;
            if (best_index) best_index[i] = (int64_t)(k & 0xFFFFFFFFull);
        }
        if (best_score) best_score[i] = k == NO_KEY ? UINT64_MAX : (k >> 32);
    }
    RS_TRY(vt_append_staged(h, news));   // (its copies guarded by vt_staging_idle, not a sync)
    return RS_OK;
}

int vt_fetch_keys(rs_vt* h, int nq, bool allreduce) {
    if (allreduce && h->nranks > 1) {
        RS_CHECK(h->comm, RS_ERR_STATE, "sharded handle without a communicator: use "
                 "rs_vt_scan_local + an external min-reduction + rs_vt_resolve");
        RS_TRY(vt_allreduce_min(h, h->dBest.get(), (size_t)nq, h->stream.get()));
    }
    const bool poll = vt_plan::polls_keys(vt_poll_env(), h->timedScan, nq);
    if (h->keysFolded) {   // the scan's last block exports them (vt_scan_local_impl)
        h->keysFolded = false;
    } else {
        if (poll)
            for (int i = 0; i < nq; ++i) h->hBest.get()[i] = KEY_PENDING;
        vt_launch_keys_export(h, h->dBest.get(), nq, h->hBest.dev(), vt_plan::VT_EXPORT_BLOCKS);
        RS_HIP(hipGetLastError());
    }
    if (!(poll && vt_poll_keys(h->hBest.get(), nq))) {
        RS_HIP(hipStreamSynchronize(h->stream.get()));
        h->stagingBusy = false;
    }
    // the keys are the call's last work: everything queued before them has run,
    // the readers of hQraw included (not the staging copies vt_store queues after them)
    h->qrawBusy = false;
    h->bestClean = h->bestPending;
    if (h->timedScan) RS_HIP(hipEventElapsedTime(&h->lastMs, h->ev0.get(), h->ev1.get()));
    return RS_OK;
}

// nb frozen-library batches queued back to back with one host synchronisation, their keys
// the rows of dStream; one export launch brings all rows back.  Three paths
// (vt_plan::StreamPath); each queues its scans and the min-reduction over the ranks of a
// handle with a communicator.

// Room for the forms of all `total` queries of a call (the fused and host-group paths).
int vt_grow_stream_forms(rs_vt* h, size_t total) {
    if (total <= h->qpStreamCap) return RS_OK;
    h->qpStreamCap = 0;
    RS_TRY(h->dQpStream.reserve((size_t)PL_CG * plane_ns(h) * 8 * total));
    RS_TRY(h->dQsumStream.reserve(total));
    if (h->prune) RS_TRY(h->dQsjStream.reserve((size_t)PF_NU * 16 * total));
    if (h->prune) RS_TRY(h->dQcStream.reserve((size_t)QC_Q4 * 4 * total));
    h->qpStreamCap = total;
    return RS_OK;
}

// Device-resident batches: one build, one scan (timed when timing is on), one collective.
int vt_stream_fused(rs_vt* h, size_t total, const uint8_t* queries, int64_t lc) {
    RS_TRY(vt_grow_stream_forms(h, total));
    const QueryForms q = vt_stream_view(h, 0);
    if (h->radius > 0) {   // the caller's batches stay as they are
        RS_TRY(h->dNormStream.reserve((size_t)h->H * h->W * total));
        RS_TRY(vt_normalise(h, queries, h->dNormStream.get(), total));
        queries = h->dNormStream.get();
    }
    RS_TRY(vt_build_forms(h, q, (int)total, queries));
    const ScanOut out{h->dStream.get(), nullptr, 0};
    RS_TRY(vt_timed_scan(h, h->timing, [&] {
        return vt_launch_scan<false>(h, q, false, lc, (int)total, out, h->rank, h->nranks);
    }));
    if (h->comm) RS_TRY(vt_allreduce_min(h, h->dStream.get(), total, h->stream.get()));
    return RS_OK;
}

// The two groups rs_vt_match_stream creates on first use: a stream and the events recorded
// for it, built into locals and moved into the handle once every one exists.  After a refused
// creation the group is absent and the next call creates it again.
int vt_ensure_upload_stream(rs_vt* h) {
    if (h->ustream.get()) return RS_OK;
    rs::Stream st;
    rs::Event up[2], used[2];
    RS_TRY(st.create());
    for (int i = 0; i < 2; ++i) {
        RS_TRY(up[i].create(hipEventDisableTiming));
        RS_TRY(used[i].create(hipEventDisableTiming));
    }
    for (int i = 0; i < 2; ++i) {
        h->evUp[i] = std::move(up[i]);
        h->evUsed[i] = std::move(used[i]);
    }
    h->ustream = std::move(st);
    return RS_OK;
}

int vt_ensure_comm_stream(rs_vt* h) {
    if (h->cstream.get()) return RS_OK;
    rs::Stream st;
    rs::Event scan, comm;
    RS_TRY(st.create());
    RS_TRY(scan.create(hipEventDisableTiming));
    RS_TRY(comm.create(hipEventDisableTiming));
    h->evScan = std::move(scan);
    h->evComm = std::move(comm);
    h->cstream = std::move(st);
    return RS_OK;
}

// Host batches in upload groups (vt_plan::host_groups), double-buffered on the upload
// stream; one collective.  Scans interleaved with upload waits have no single duration:
// timedScan stays false.
int vt_stream_host_groups(rs_vt* h, int nb, int nq, const uint8_t* queries, int64_t lc) {
    const size_t total = (size_t)nb * nq, qb = (size_t)h->H * h->W * nq;
    RS_TRY(vt_grow_stream_forms(h, total));
    const vt_plan::HostGroups plan = vt_plan::host_groups(nb);
    if (h->radius > 0) RS_TRY(h->dNormStream.reserve(qb * nb));
    RS_TRY(vt_ensure_upload_stream(h));
    if (qb * plan.gb > h->upCap) {
        RS_HIP(hipStreamSynchronize(h->ustream.get()));
        h->upCap = 0;
        for (int i = 0; i < 2; ++i) RS_TRY(h->dUp[i].reserve(qb * plan.gb));
        h->upCap = qb * plan.gb;
    }
    for (int g = 0;; ++g) {
        const vt_plan::HostGroup grp = plan.group(g);
        if (grp.n == 0) break;
        const int bi = grp.buf;
        if (grp.waits) RS_HIP(hipStreamWaitEvent(h->ustream.get(), h->evUsed[bi].get(), 0));
        RS_HIP(hipMemcpyAsync(h->dUp[bi].get(), queries + qb * grp.b0, qb * grp.n, hipMemcpyHostToDevice, h->ustream.get()));
        RS_HIP(hipEventRecord(h->evUp[bi].get(), h->ustream.get()));
        RS_HIP(hipStreamWaitEvent(h->stream.get(), h->evUp[bi].get(), 0));
        const QueryForms q = vt_stream_view(h, (size_t)grp.b0 * nq);
        const uint8_t* src = h->dUp[bi].get();
        if (h->radius > 0) {   // each group into its own part of dNormStream
            uint8_t* const dn = h->dNormStream.get() + qb * grp.b0;
            RS_TRY(vt_normalise(h, src, dn, (size_t)grp.n * nq));
            src = dn;
        }
        RS_TRY(vt_build_forms(h, q, grp.n * nq, src));
        RS_HIP(hipEventRecord(h->evUsed[bi].get(), h->stream.get()));
        const ScanOut out{h->dStream.get() + (size_t)grp.b0 * nq, nullptr, 0};
        RS_TRY(vt_launch_scan<false>(h, q, false, lc, grp.n * nq, out, h->rank, h->nranks));
    }
    if (h->comm) RS_TRY(vt_allreduce_min(h, h->dStream.get(), total, h->stream.get()));
    return RS_OK;
}

// A build and a scan per batch through the batch view (host batches through dQraw).  With a
// communicator each batch's row is reduced on the collective stream while the next batch's
// forms and scan run on the main stream (rows are distinct), and the main stream waits for
// the last.  Several scans: no single duration, timedScan stays false.
int vt_stream_per_batch(rs_vt* h, int nb, int nq, const uint8_t* queries, bool on_device, int64_t lc) {
    const size_t qb = (size_t)h->H * h->W * nq;
    for (int b = 0; b < nb; ++b) {
        unsigned long long* keys = h->dStream.get() + (size_t)b * nq;
        const ScanOut out{keys, nullptr, 0};
        const uint8_t* src = queries + qb * b;
        if (!on_device) {
            uint8_t* const up = h->radius > 0 ? h->dNormRaw.get() : h->dQraw.get();
            RS_HIP(hipMemcpyAsync(up, src, qb, hipMemcpyHostToDevice, h->stream.get()));
            src = up;
        }
        if (h->radius > 0) {   // (a device batch is read where it is and left as it is)
            RS_TRY(vt_normalise(h, src, h->dQraw.get(), (size_t)nq));
            src = h->dQraw.get();
        }
        RS_TRY(vt_build_forms(h, vt_batch_view(h), nq, src));
        RS_TRY(vt_launch_scan<false>(h, vt_batch_view(h), false, lc, nq, out, h->rank, h->nranks));
        if (h->comm) {
            RS_HIP(hipEventRecord(h->evScan.get(), h->stream.get()));
            RS_HIP(hipStreamWaitEvent(h->cstream.get(), h->evScan.get(), 0));
            RS_TRY(vt_allreduce_min(h, keys, (size_t)nq, h->cstream.get()));
        }
    }
    if (h->comm) {
        RS_HIP(hipEventRecord(h->evComm.get(), h->cstream.get()));
        RS_HIP(hipStreamWaitEvent(h->stream.get(), h->evComm.get(), 0));
    }
    return RS_OK;
}

int vt_match_stream_impl(rs_vt* h, int nb, int nq, const uint8_t* queries, uint64_t* best_score,
                         int64_t* best_index) {
    // arguments, streams and room for the keys
    RS_CHECK(h, RS_ERR_STATE, "null view-template handle");
    RS_CHECK(nb >= 0 && nq >= 0, RS_ERR_ARG, "negative batch or query count");
    if (nb == 0 || nq == 0) return RS_OK;
    RS_CHECK(queries, RS_ERR_ARG, "null queries");
    RS_CHECK(h->nranks == 1 || h->comm, RS_ERR_STATE, "sharded handle without a communicator: "
             "rs_vt_match_stream needs the RCCL reduction (rs_vt_attach_comm)");
    RS_HIP(hipSetDevice(h->device));
    if (h->comm) RS_TRY(vt_ensure_comm_stream(h));
    RS_TRY(vt_grow_queries(h, nq));
    const size_t total = (size_t)nb * nq;
    RS_CHECK(total <= INT32_MAX, RS_ERR_ARG, "too many queries in one stream");
    if (total > h->streamCap) {
        h->streamCap = 0;
        RS_TRY(h->hStream.reserve(total, hipHostMallocDefault));
        RS_TRY(h->dStream.reserve(total));
        h->streamCap = total;
        h->streamClean = false;
    }
    const bool on_device = rs::on_device(queries);
    RS_CHECK(!on_device || reinterpret_cast<uintptr_t>(queries) % 8 == 0, RS_ERR_ARG,
             "device-resident queries must be 8-byte aligned");
    // the keys start at UINT64_MAX: the export of the previous call reset them
    // (one memset after allocation, or after a call that did not reach its export)
    if (!h->streamClean)
        RS_HIP(hipMemsetAsync(h->dStream.get(), 0xFF, sizeof(unsigned long long) * h->streamCap, h->stream.get()));
    h->streamClean = false;
    h->stagedQ = 0;  // the forms no longer match dQraw
    h->timedScan = false;  // (only the fused path's one scan is timed)
    const int64_t lc = local_count_of(h, h->count);
    // the path's scans and its min-reduction
    switch (vt_plan::stream_path(on_device, h->planar, nb)) {
    case vt_plan::StreamPath::Fused: RS_TRY(vt_stream_fused(h, total, queries, lc)); break;
    case vt_plan::StreamPath::HostGroups: RS_TRY(vt_stream_host_groups(h, nb, nq, queries, lc)); break;
    case vt_plan::StreamPath::PerBatch: RS_TRY(vt_stream_per_batch(h, nb, nq, queries, on_device, lc)); break;
    }
    // keys -> pinned host memory and reset for the next call, in one queued launch
    // (in place of a device-to-host blit and a memset)
    vt_launch_keys_export(h, h->dStream.get(), (int)total, h->hStream.dev(), vt_plan::VT_EXPORT_BLOCKS_STREAM);
    RS_HIP(hipGetLastError());
    RS_HIP(hipStreamSynchronize(h->stream.get()));
    h->streamClean = true;
    if (h->timedScan) RS_HIP(hipEventElapsedTime(&h->lastMs, h->ev0.get(), h->ev1.get()));
    vt_decode_keys(h->hStream.get(), total, best_score, best_index);
    return RS_OK;
}

int vt_match_impl(rs_vt* h, int nq, const uint8_t* queries, int mode, uint64_t* best_score,
                  int64_t* best_index, uint8_t* is_new, bool frames = false) {
    RS_CHECK(mode == RS_VT_FROZEN || mode == RS_VT_SEQUENTIAL, RS_ERR_ARG, "unknown mode %d", mode);
    RS_TRY(vt_scan_local_impl(h, nq, queries, frames, h->nranks == 1));
    if (nq == 0) return RS_OK;
    RS_TRY(vt_fetch_keys(h, nq, true));
    return vt_resolve_impl(h, nq, h->hBest.get(), mode, best_score, best_index, is_new);
}

}  // namespace

extern "C" {

int rs_vt_create(int H, int W, int max_offset, uint64_t thr, int64_t capacity, int device,
                 rs_vt** out) {
    return rs_vt_create_metric(H, W, max_offset, thr, capacity, device, RS_VT_METRIC_WRAPPED, out);
}

int rs_vt_create_metric(int H, int W, int max_offset, uint64_t thr, int64_t capacity, int device,
                        int metric, rs_vt** out) {
    rs::clear_error();
    RS_CHECK(out, RS_ERR_ARG, "null output handle pointer");
    *out = nullptr;
    RS_CHECK(vt_plan::metric_known(metric), RS_ERR_ARG, "unknown metric %d: expected RS_VT_METRIC_WRAPPED or "
             "RS_VT_METRIC_SAD", metric);
    RS_CHECK(H > 0 && W > 0 && H <= 4096 && W <= 4096, RS_ERR_ARG, "bad template shape (%d, %d)", H, W);
    RS_CHECK(max_offset >= 1 && max_offset <= 64, RS_ERR_ARG, "max_offset %d outside [1, 64]", max_offset);
    RS_CHECK(capacity >= 0, RS_ERR_ARG, "negative capacity");
    // max score H*W*255 must fit the 32-bit half of the packed key
    RS_CHECK((uint64_t)H * W * 255u < 0xFFFFFFFFull, RS_ERR_ARG, "template too large");
    RS_TRY(rs::use_device(device));
    // one failure exit: rs_vt_destroy takes a handle at any stage
    std::unique_ptr<rs_vt, int (*)(rs_vt*)> owner(new rs_vt(), rs_vt_destroy);
    rs_vt* const h = owner.get();
    h->H = H; h->W = W; h->M = max_offset; h->thr = (double)thr; h->device = device;
    h->WD = (W + 3) / 4;
    h->HQ = (H + 3) / 4;
    h->metric = metric;
    // (a term is at most 255 under either metric: the bound above holds for both)
    const bool wrapped = metric == RS_VT_METRIC_WRAPPED;   // RS_VT_SCAN / _PRUNE / _FRONT are its switches
    h->planar = wrapped && W == 8 * PL_CG && (H == 64 || H == 32) && max_offset == FAST_M;
    if (const char* e = wrapped ? std::getenv("RS_VT_SCAN") : nullptr) {
        // A/B switch: "carry" forces the byte-SWAR carry-count scan; "plane" (or
        // unset) keeps the default
        if (std::strcmp(e, "carry") == 0) h->planar = false;
        else RS_CHECK(std::strcmp(e, "plane") == 0 || e[0] == 0, RS_ERR_ARG, "RS_VT_SCAN='%s': expected plane or carry", e);
    }
    if (h->planar && h->H == 64) {
        // A/B switch: "0" keeps the dense launch everywhere, "force" prunes at any size
        // (tests), "1" (or unset) prunes the large frozen scans
        RS_TRY(vt_env_switch("RS_VT_PRUNE", &h->prune));
        // A/B switch: "0" keeps the prefilter and the verification two launches, "force"
        // fuses them for any shape (tests), "1" (or unset) follows vt_plan::front_fused
        RS_TRY(vt_env_switch("RS_VT_FRONT", &h->front));
        // A/B switch: "1" (or unset) one list pass on the verified score, "2" the two-pass chain
        if (const char* ps = std::getenv("RS_VT_PASSES"); ps && ps[0]) {
            RS_CHECK((ps[0] == '1' || ps[0] == '2') && ps[1] == 0, RS_ERR_ARG, "RS_VT_PASSES='%s': expected 1 or 2", ps);
            h->passes = ps[0] - '0';
        }
        // A/B switch and tests: "1", "2" or "4" entries per batch in both list passes; unset:
        // each list's own width (vt_plan::list_width)
        if (const char* nb = std::getenv("RS_VT_LIST_NB"); nb && nb[0]) {
            RS_CHECK((nb[0] == '1' || nb[0] == '2' || nb[0] == '4') && nb[1] == 0, RS_ERR_ARG,
                     "RS_VT_LIST_NB='%s': expected 1, 2 or 4", nb);
            h->listNb = nb[0] - '0';
        }
    }
    if (h->planar) {
        // resident blocks per CU: the occupancy API, capped by the kernel's own VGPR and
        // LDS arithmetic (the API has read one block high on gfx950 for some SGPR counts)
        int per_cu = 0, cus = 0;
        hipFuncAttributes fa{};
        const void* fn = vt_by_h(h, [](auto H) {
            return reinterpret_cast<const void*>(vt_scan_plane_kernel<decltype(H)::value, false>);
        });
        hipError_t oe = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, fn, 64 * PL_CG * PL_SPLIT, 0);
        if (oe == hipSuccess) oe = hipFuncGetAttributes(&fa, fn);
        if (oe == hipSuccess) oe = hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device);
        RS_CHECK(oe == hipSuccess, RS_ERR_HIP, "occupancy query failed: %s", hipGetErrorString(oe));
        const int vg = std::max(8, (fa.numRegs + 7) / 8 * 8);
        const int by_vgpr = (512 / vg) * 4 / (PL_CG * PL_SPLIT);  // waves/SIMD x 4 SIMDs / waves/block
        const int by_lds = fa.sharedSizeBytes > 0 ? (int)(160 * 1024 / fa.sharedSizeBytes) : per_cu;
        const int api = per_cu;
        per_cu = std::max(1, std::min({api, by_vgpr, by_lds}));
        h->planeSlots = std::max(1, per_cu * cus);
    }
    RS_TRY(h->stream.create());
    RS_TRY(h->ev0.create());
    RS_TRY(h->ev1.create());
    RS_TRY(vt_grow_lib(h, capacity > 0 ? capacity : 64));
    RS_TRY(vt_grow_queries(h, 64));
    RS_TRY(vt_grow_index(h, 64));
    *out = owner.release();
    return RS_OK;
}

int rs_vt_destroy(rs_vt* h) {
    if (!h) return RS_OK;
    (void)hipSetDevice(h->device);
    // the handle's last queued work: a fault or launch error the early-returning calls
    // left on a stream is reported here instead of being dropped
    const hipError_t se = rs::sync_streams({h->stream.get(), h->cstream.get(), h->ustream.get()});
    if (h->comm) (void)ncclCommDestroy(h->comm);
    delete h;  // (the streams and events, then the buffers, go with their members)
    RS_CHECK(se == hipSuccess, RS_ERR_HIP, "work queued before rs_vt_destroy failed: %s", hipGetErrorString(se));
    return RS_OK;
}

int rs_vt_count(const rs_vt* h, int64_t* count) {
    RS_CHECK(h && count, RS_ERR_ARG, "null argument");
    *count = h->count;
    return RS_OK;
}

int rs_vt_add(rs_vt* h, int n, const uint8_t* templates, int64_t* first_index) {
    rs::clear_error();
    RS_CHECK(h, RS_ERR_STATE, "null view-template handle");
    RS_CHECK(n >= 0 && (n == 0 || templates), RS_ERR_ARG, "bad template batch");
    RS_HIP(hipSetDevice(h->device));
    if (first_index) *first_index = h->count;
    if (n == 0) return RS_OK;
    RS_TRY(vt_grow_queries(h, n));
    const size_t qb = (size_t)h->H * h->W * n;
    // A pageable array is uploaded by HIP, which returns once the bytes are staged in its
    // own buffers.  Pinned or registered host memory, or device memory, is read by the
    // DMA engine while the copy runs, after this call would return: those sources are
    // waited for below, so in every case the caller may reuse or free its array at once.
    hipPointerAttribute_t attr{};
    const bool direct_dma = hipPointerGetAttributes(&attr, templates) == hipSuccess &&
                            (attr.type == hipMemoryTypeHost || attr.type == hipMemoryTypeDevice ||
                             attr.type == hipMemoryTypeManaged);
    (void)hipGetLastError();  // a pageable pointer is not an error
    RS_HIP(hipMemcpyAsync(h->radius > 0 ? h->dNormRaw.get() : h->dQraw.get(), templates, qb,
                          attr.type == hipMemoryTypeDevice && direct_dma ? hipMemcpyDeviceToDevice
                                                                         : hipMemcpyHostToDevice,
                          h->stream.get()));
    int s = h->radius > 0 ? vt_normalise(h, h->dNormRaw.get(), h->dQraw.get(), (size_t)n) : RS_OK;
    h->stagedQ = 0;  // the staging buffer now holds templates, not a query batch
    std::vector<std::pair<int, int64_t>> news;
    news.reserve(n);
    for (int i = 0; i < n; ++i) news.emplace_back(i, h->count + i);
    if (s == RS_OK) s = vt_append_staged(h, news);   // (its copies guarded by vt_staging_idle, not a sync)
    // (on the error path as well: the upload above is queued either way)
    if (direct_dma) {
        const hipError_t e = hipStreamSynchronize(h->stream.get());
        RS_CHECK(s != RS_OK || e == hipSuccess, RS_ERR_HIP, "hipStreamSynchronize failed: %s", hipGetErrorString(e));
    }
    return s;
}

int rs_vt_read(rs_vt* h, int64_t index, uint8_t* out) {
    rs::clear_error();
    RS_CHECK(h && out, RS_ERR_ARG, "null argument");
    RS_CHECK(index >= 0 && index < h->count, RS_ERR_ARG, "template index %lld outside [0, %lld)",
             (long long)index, (long long)h->count);
    RS_CHECK(index % h->nranks == h->rank, RS_ERR_ARG, "template %lld lives on rank %lld",
             (long long)index, (long long)(index % h->nranks));
    RS_HIP(hipSetDevice(h->device));
    const int64_t slot = index / h->nranks;
    const int64_t tb = slot >> 6, tl = slot & 63;
    std::vector<uint4> chunks((size_t)h->WD * h->HQ);
    for (int c = 0; c < h->WD; ++c)
        for (int q = 0; q < h->HQ; ++q)
            RS_HIP(hipMemcpyAsync(&chunks[(size_t)c * h->HQ + q],
                                  h->dLib.get() + ((tb * h->WD + c) * h->HQ + q) * 64 + tl, sizeof(uint4),
                                  hipMemcpyDeviceToHost, h->stream.get()));
    RS_HIP(hipStreamSynchronize(h->stream.get()));
    for (int r = 0; r < h->H; ++r)
        for (int col = 0; col < h->W; ++col) {
            const uint4& ch = chunks[(size_t)(col / 4) * h->HQ + r / 4];
            const uint32_t w[4] = {ch.x, ch.y, ch.z, ch.w};
            out[(size_t)r * h->W + col] = (uint8_t)(w[r & 3] >> (8 * (col & 3)));
        }
    return RS_OK;
}

int rs_vt_match_batch(rs_vt* h, int nq, const uint8_t* queries, int mode, uint64_t* best_score,
                      int64_t* best_index, uint8_t* is_new) {
    rs::clear_error();
    return vt_match_impl(h, nq, queries, mode, best_score, best_index, is_new);
}

int rs_vt_match_stream(rs_vt* h, int nb, int nq, const uint8_t* queries, uint64_t* best_score,
                       int64_t* best_index) {
    rs::clear_error();
    return vt_match_stream_impl(h, nb, nq, queries, best_score, best_index);
}

int rs_vt_match(rs_vt* h, const uint8_t* query, uint64_t* best_score, int64_t* best_index,
                int* is_new) {
    rs::clear_error();
    uint8_t nw = 0;
    const int s = vt_match_impl(h, 1, query, RS_VT_SEQUENTIAL, best_score, best_index, &nw);
    if (is_new) *is_new = nw;
    return s;
}

int rs_vt_set_subsample(rs_vt* h, int64_t frame_bytes, const int32_t* pixels) {
    rs::clear_error();
    RS_CHECK(h && pixels, RS_ERR_ARG, "null argument");
    RS_CHECK(frame_bytes > 0 && frame_bytes <= INT32_MAX, RS_ERR_ARG, "bad frame size %lld",
             (long long)frame_bytes);
    const int npix = h->H * h->W;
    for (int i = 0; i < npix; ++i)
        RS_CHECK(pixels[i] >= 0 && pixels[i] < frame_bytes, RS_ERR_ARG,
                 "pixel offset %d of entry %d outside the %lld-byte frame", pixels[i], i,
                 (long long)frame_bytes);
    RS_HIP(hipSetDevice(h->device));
    RS_TRY(h->dPix.reserve((size_t)npix));
    RS_HIP(hipMemcpyAsync(h->dPix.get(), pixels, sizeof(int32_t) * npix, hipMemcpyHostToDevice, h->stream.get()));
    RS_HIP(hipStreamSynchronize(h->stream.get()));
    if (frame_bytes != h->frameBytes) {  // staging buffers are sized per frame
        h->frameCap = 0;
        h->dFrames.reset();
        h->hFrames.reset();
    }
    h->frameBytes = frame_bytes;
    return RS_OK;
}

int rs_vt_match_frames(rs_vt* h, int nf, const uint8_t* frames, int mode, uint64_t* best_score,
                       int64_t* best_index, uint8_t* is_new) {
    rs::clear_error();
    RS_CHECK(h, RS_ERR_STATE, "null view-template handle");
    return vt_match_impl(h, nf, frames, mode, best_score, best_index, is_new, true);
}

int rs_vt_scan_local(rs_vt* h, int nq, const uint8_t* queries, uint64_t* local_keys) {
    rs::clear_error();
    RS_TRY(vt_scan_local_impl(h, nq, queries));
    if (nq == 0) return RS_OK;
    RS_TRY(vt_fetch_keys(h, nq, false));
    if (local_keys) std::memcpy(local_keys, h->hBest.get(), sizeof(uint64_t) * nq);
    return RS_OK;
}

int rs_vt_resolve(rs_vt* h, int nq, const uint64_t* global_keys, int mode, uint64_t* best_score,
                  int64_t* best_index, uint8_t* is_new) {
    rs::clear_error();
    static_assert(sizeof(uint64_t) == sizeof(unsigned long long), "key width");
    return vt_resolve_impl(h, nq, reinterpret_cast<const unsigned long long*>(global_keys), mode,
                           best_score, best_index, is_new);
}

int rs_vt_set_shard(rs_vt* h, int rank, int nranks) {
    rs::clear_error();
    RS_CHECK(h, RS_ERR_STATE, "null view-template handle");
    RS_CHECK(nranks >= 1 && rank >= 0 && rank < nranks, RS_ERR_ARG, "bad rank %d of %d", rank, nranks);
    RS_CHECK(h->count == 0 && h->comm == nullptr, RS_ERR_STATE,
             "set the shard before adding templates, once");
    h->rank = rank;
    h->nranks = nranks;
    return RS_OK;
}

int rs_vt_set_normalise(rs_vt* h, int radius, int gain) {
    rs::clear_error();
    RS_CHECK(h, RS_ERR_STATE, "null view-template handle");
    RS_CHECK(radius >= 0 && radius <= rs::VTN_MAX_RADIUS, RS_ERR_ARG, "radius %d outside [0, %d]", radius,
             rs::VTN_MAX_RADIUS);
    RS_CHECK(radius == 0 || (gain >= 1 && gain <= rs::VTN_MAX_GAIN), RS_ERR_ARG, "gain %d outside [1, %d]", gain,
             rs::VTN_MAX_GAIN);
    // a library or a staged batch of the other kind of bytes must not meet the new setting
    RS_CHECK(h->count == 0 && h->stagedQ == 0, RS_ERR_STATE,
             "set the normalisation before adding templates or staging a batch");
    RS_HIP(hipSetDevice(h->device));
    if (radius > 0) {
        RS_TRY(h->dNormRaw.reserve((size_t)h->H * h->W * h->qCap));
    } else {
        RS_HIP(hipStreamSynchronize(h->stream.get()));   // (queued work may still read them)
        h->dNormRaw.reset();
        h->dNormStream.reset();
        h->dOffRaw.reset();
    }
    h->radius = radius;
    h->gain = radius > 0 ? gain : 0;
    return RS_OK;
}

int rs_vt_normalise(const rs_vt* h, int* radius, int* gain) {
    RS_CHECK(h, RS_ERR_STATE, "null view-template handle");
    if (radius) *radius = h->radius;
    if (gain) *gain = h->gain;
    return RS_OK;
}

int rs_vt_normalise_host(int H, int W, int radius, int gain, const uint8_t* src, uint8_t* dst) {
    rs::clear_error();
    RS_CHECK(H > 0 && W > 0 && H <= 4096 && W <= 4096, RS_ERR_ARG, "bad image shape (%d, %d)", H, W);
    RS_CHECK(radius >= 1 && radius <= rs::VTN_MAX_RADIUS, RS_ERR_ARG, "radius %d outside [1, %d]", radius,
             rs::VTN_MAX_RADIUS);
    RS_CHECK(gain >= 1 && gain <= rs::VTN_MAX_GAIN, RS_ERR_ARG, "gain %d outside [1, %d]", gain, rs::VTN_MAX_GAIN);
    RS_CHECK(src && dst && src != dst, RS_ERR_ARG, "null or aliased image");
    rs::vtn_normalise_host(H, W, radius, gain, src, dst);
    return RS_OK;
}

int rs_vt_rank(const rs_vt* h, int* rank, int* nranks) {
    RS_CHECK(h, RS_ERR_STATE, "null view-template handle");
    if (rank) *rank = h->rank;
    if (nranks) *nranks = h->nranks;
    return RS_OK;
}

int rs_vt_scores(rs_vt* h, int nq, const uint8_t* queries, int64_t t0, int64_t nt,
                 uint64_t* scores) {
    rs::clear_error();
    RS_CHECK(h, RS_ERR_STATE, "null view-template handle");
    RS_CHECK(h->nranks == 1, RS_ERR_STATE, "rs_vt_scores needs an unsharded library");
    RS_CHECK(nq >= 0 && t0 >= 0 && nt >= 0 && t0 + nt <= h->count, RS_ERR_ARG,
             "template range [%lld, %lld) outside [0, %lld)", (long long)t0,
             (long long)(t0 + nt), (long long)h->count);
    if (nq == 0 || nt == 0) return RS_OK;
    RS_CHECK(queries && scores, RS_ERR_ARG, "null argument");
    RS_HIP(hipSetDevice(h->device));
    RS_TRY(vt_stage_queries(h, nq, queries));
    h->stagedQ = 0;  // the staging buffer no longer holds the last match batch
    // only the 64-slot blocks that hold [t0, t0 + nt) are scanned
    const int64_t tb0 = t0 / 64, lo = t0 - tb0 * 64, span = lo + nt;
    const int64_t ld = (int64_t)rs::round_up((size_t)span, 64);
    RS_TRY(vt_grow_matrix(h, (size_t)ld * nq));
    ScanOut mo{nullptr, h->dMat.get(), ld};
    RS_TRY(vt_timed_scan(h, true, [&] {   // (always timed: rs_vt_last_ms after rs_vt_scores)
        return vt_launch_scan<true>(h, vt_batch_view(h), false, span, nq, mo, 0, 1, tb0);
    }));
    RS_HIP(hipMemcpy2DAsync(h->hMat.get(), sizeof(uint32_t) * nt, h->dMat.get() + lo, sizeof(uint32_t) * ld,
                            sizeof(uint32_t) * nt, nq, hipMemcpyDeviceToHost, h->stream.get()));
    RS_HIP(hipStreamSynchronize(h->stream.get()));
    RS_HIP(hipEventElapsedTime(&h->lastMs, h->ev0.get(), h->ev1.get()));
    for (size_t i = 0; i < (size_t)nq * nt; ++i) scores[i] = h->hMat.get()[i];
    return RS_OK;
}

int rs_vt_offset_profile(rs_vt* h, int nq, const uint8_t* queries, const int64_t* index, uint32_t* profile,
                         int32_t* offset) {
    rs::clear_error();
    RS_CHECK(h, RS_ERR_STATE, "null view-template handle");
    RS_CHECK(h->nranks == 1, RS_ERR_STATE, "rs_vt_offset_profile needs an unsharded library");
    RS_CHECK(nq >= 0, RS_ERR_ARG, "negative query count");
    if (nq == 0) return RS_OK;
    RS_CHECK(index && offset, RS_ERR_ARG, "null argument");
    for (int i = 0; i < nq; ++i)
        RS_CHECK(index[i] >= -1 && index[i] < h->count, RS_ERR_ARG,
                 "template index %lld of query %d outside [-1, %lld)", (long long)index[i], i,
                 (long long)h->count);
    RS_CHECK(queries || nq == h->stagedQ, RS_ERR_STATE, "no staged batch of %d queries (have %d)", nq,
             h->stagedQ);
    RS_HIP(hipSetDevice(h->device));
    const size_t n = (size_t)nq, no = (size_t)(2 * h->M - 1), qb = (size_t)h->H * h->W * n;
    RS_TRY(h->hOffIdx.reserve(rs::grown<size_t>(h->hOffIdx.capacity(), n, 64), VT_FINE));
    RS_TRY(h->hOffProfile.reserve(rs::grown<size_t>(h->hOffProfile.capacity(), n * no, 64 * no), VT_FINE));
    RS_TRY(h->hOffOffset.reserve(rs::grown<size_t>(h->hOffOffset.capacity(), n, 64), VT_FINE));
    const uint8_t* src = h->dQraw.get();
    const size_t offq = rs::grown<size_t>(h->dOffQ.capacity(), qb, 64 * (size_t)h->H * h->W);
    if (queries && h->radius > 0) {   // raw queries, host or device, normalised into dOffQ
        RS_TRY(h->dOffQ.reserve(offq));
        const uint8_t* raw = queries;
        if (!rs::on_device(queries)) {
            RS_TRY(h->dOffRaw.reserve(h->dOffQ.capacity()));
            RS_HIP(hipMemcpyAsync(h->dOffRaw.get(), queries, qb, hipMemcpyHostToDevice, h->stream.get()));
            raw = h->dOffRaw.get();
        }
        RS_TRY(vt_normalise(h, raw, h->dOffQ.get(), n));
        src = h->dOffQ.get();
    } else if (queries && rs::on_device(queries)) {
        src = queries;   // read in place
    } else if (queries) {
        RS_TRY(h->dOffQ.reserve(offq));
        RS_HIP(hipMemcpyAsync(h->dOffQ.get(), queries, qb, hipMemcpyHostToDevice, h->stream.get()));
        src = h->dOffQ.get();
    }
    std::memcpy(h->hOffIdx.get(), index, sizeof(int64_t) * n);
    const bool sad = h->metric == RS_VT_METRIC_SAD, fast = h->M == FAST_M;
    auto launch = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, dim3(nq), dim3(64), 0, h->stream.get(), h->dLib.get(), h->count, h->H, h->W,
                           h->WD, h->HQ, h->M, src, h->hOffIdx.dev(), h->hOffProfile.dev(),
                           h->hOffOffset.dev());
    };
    if (sad && fast) launch(vt_offset_profile_kernel<rs::VTO_METRIC_SAD, true>);
    else if (sad) launch(vt_offset_profile_kernel<rs::VTO_METRIC_SAD, false>);
    else if (fast) launch(vt_offset_profile_kernel<rs::VTO_METRIC_WRAPPED, true>);
    else launch(vt_offset_profile_kernel<rs::VTO_METRIC_WRAPPED, false>);
    RS_HIP(hipGetLastError());
    // the results are the kernel's own stores: the call waits for the stream, and with it
    // for everything queued before (an append's staging copies, a reader of hQraw)
    RS_HIP(hipStreamSynchronize(h->stream.get()));
    h->stagingBusy = false;
    h->qrawBusy = false;
    if (profile) std::memcpy(profile, h->hOffProfile.get(), sizeof(uint32_t) * n * no);
    std::memcpy(offset, h->hOffOffset.get(), sizeof(int32_t) * n);
    return RS_OK;
}

int rs_vt_offset_profile_host(int metric, int H, int W, int max_offset, const uint8_t* tpl, const uint8_t* query,
                              uint32_t* profile, int32_t* offset) {
    rs::clear_error();
    RS_CHECK(vt_plan::metric_known(metric), RS_ERR_ARG, "unknown metric %d", metric);
    RS_CHECK(H > 0 && W > 0 && max_offset >= 1 && H >= 2 * max_offset, RS_ERR_ARG,
             "bad shape (%d, %d) for max_offset %d", H, W, max_offset);
    RS_CHECK((uint64_t)H * W * 255u < 0xFFFFFFFFull, RS_ERR_ARG, "template too large");
    RS_CHECK(tpl && query && profile && offset, RS_ERR_ARG, "null argument");
    *offset = rs::vto_profile_host(metric, H, W, max_offset, tpl, query, profile);
    return RS_OK;
}

int rs_vt_set_threshold(rs_vt* h, double threshold) {
    rs::clear_error();
    RS_CHECK(h, RS_ERR_STATE, "null view-template handle");
    h->thr = threshold;
    return RS_OK;
}

int rs_vt_metric(const rs_vt* h, int* metric) {
    RS_CHECK(h && metric, RS_ERR_ARG, "null argument");
    *metric = h->metric;
    return RS_OK;
}

const char* rs_vt_scan_form(const rs_vt* h) {
    if (!h) return nullptr;
    if (h->metric == RS_VT_METRIC_SAD) return vt_plan::sad_form(h->H, h->M);
    if (h->planar) return h->prune ? "plane-pruned" : "plane";
    if (h->M != FAST_M || (h->H != 64 && h->H != 32)) return "generic";
    return "carry";
}

namespace {
// The two-pass rule's counts of the last (single-pass) pruned call, from the buffers it left:
// acc[0] the pairs of the rule's second list, acc[1] the settled queries (vt_prune_count_kernel).
int vt_prune_count(rs_vt* h, unsigned long long acc[2]) {
    if (!h->dCountAcc.get()) RS_TRY(h->dCountAcc.reserve(2));
    RS_HIP(hipMemsetAsync(h->dCountAcc.get(), 0, 2 * sizeof(unsigned long long), h->stream.get()));
    hipLaunchKernelGGL(vt_prune_count_kernel, dim3((unsigned)((h->pruneNq + 255) / 256)), dim3(256), 0, h->stream.get(),
                       h->dMinLB.get(), h->pruneNq, h->pruneNtb, h->dTbStar.get(), h->dUblk.get(),
                       h->dCountAcc.get());
    RS_HIP(hipGetLastError());
    RS_HIP(hipMemcpyAsync(acc, h->dCountAcc.get(), 2 * sizeof(unsigned long long), hipMemcpyDeviceToHost, h->stream.get()));
    RS_HIP(hipStreamSynchronize(h->stream.get()));
    return RS_OK;
}
}  // namespace

int rs_vt_prune_stats(rs_vt* h, int64_t out[4]) {
    rs::clear_error();
    RS_CHECK(h && out, RS_ERR_ARG, "null argument");
    out[0] = out[1] = out[2] = out[3] = 0;
    if (h->prunePasses == 0) return RS_OK;
    RS_HIP(hipSetDevice(h->device));
    out[2] = h->prunePairs;
    out[3] = h->prunePasses;
    if (h->pruneMode == 1) {   // a single list pass: the rule's counts, counted on demand
        unsigned long long acc[2] = {0ull, 0ull};
        RS_TRY(vt_prune_count(h, acc));
        out[0] = h->pruneNq;
        out[1] = (int64_t)acc[0];
        return RS_OK;
    }
    // the pairs of B2: list2's counters, which stay until the next pruned launch's lists
    unsigned long long s0 = 0ull;
    std::vector<unsigned> c2((size_t)h->pruneNtb);
    RS_HIP(hipMemcpyAsync(&s0, h->dPruneStat.get(), sizeof(s0), hipMemcpyDeviceToHost, h->stream.get()));
    RS_HIP(hipMemcpyAsync(c2.data(), h->dListCnt.get() + h->listCntCap, sizeof(unsigned) * c2.size(), hipMemcpyDeviceToHost,
                          h->stream.get()));
    RS_HIP(hipStreamSynchronize(h->stream.get()));
    out[0] = (int64_t)s0;
    for (const unsigned c : c2) out[1] += (int64_t)c;
    return RS_OK;
}

int rs_vt_prune_scanned(rs_vt* h, int64_t* out) {
    rs::clear_error();
    RS_CHECK(h && out, RS_ERR_ARG, "null argument");
    *out = 0;
    if (h->prunePasses == 0) return RS_OK;
    RS_HIP(hipSetDevice(h->device));
    if (h->pruneMode == 1) {   // the one list's entries: the last call's parity of the counters
        std::vector<unsigned> c((size_t)h->pruneNtb);
        RS_HIP(hipMemcpyAsync(c.data(), h->dCntPar.get() + vt_plan::parity_last_offset(h->cntPar),
                              sizeof(unsigned) * c.size(), hipMemcpyDeviceToHost, h->stream.get()));
        RS_HIP(hipStreamSynchronize(h->stream.get()));
        for (const unsigned n : c) *out += (int64_t)n;
        return RS_OK;
    }
    // two passes: list 1 holds the unsettled queries, list 2 the rule's pairs
    int64_t st[4];
    unsigned long long v = 0ull;
    RS_TRY(rs_vt_prune_stats(h, st));
    RS_HIP(hipMemcpyAsync(&v, h->dPruneStat.get() + 2, sizeof(v), hipMemcpyDeviceToHost, h->stream.get()));
    RS_HIP(hipStreamSynchronize(h->stream.get()));
    *out = st[0] - (int64_t)v + st[1];
    return RS_OK;
}

int rs_vt_prune_verified(rs_vt* h, int64_t* out) {
    rs::clear_error();
    RS_CHECK(h && out, RS_ERR_ARG, "null argument");
    *out = 0;
    if (h->prunePasses == 0) return RS_OK;
    RS_HIP(hipSetDevice(h->device));
    if (h->pruneMode == 1) {
        unsigned long long acc[2] = {0ull, 0ull};
        RS_TRY(vt_prune_count(h, acc));
        *out = (int64_t)acc[1];
        return RS_OK;
    }
    unsigned long long v = 0ull;
    RS_HIP(hipMemcpyAsync(&v, h->dPruneStat.get() + 2, sizeof(v), hipMemcpyDeviceToHost, h->stream.get()));
    RS_HIP(hipStreamSynchronize(h->stream.get()));
    *out = (int64_t)v;
    return RS_OK;
}

int rs_vt_last_ms(rs_vt* h, double* ms) {
    RS_CHECK(h && ms, RS_ERR_ARG, "null argument");
    *ms = h->timedScan ? h->lastMs : -1.0;
    return RS_OK;
}

int rs_vt_set_timing(rs_vt* h, int enable) {
    rs::clear_error();
    RS_CHECK(h, RS_ERR_STATE, "null view-template handle");
    h->timing = enable != 0;
    return RS_OK;
}

int rs_comm_unique_id(uint8_t id[RS_UNIQUE_ID_BYTES]) {
    rs::clear_error();
    RS_CHECK(id, RS_ERR_ARG, "null id buffer");
    static_assert(sizeof(ncclUniqueId) == RS_UNIQUE_ID_BYTES, "ncclUniqueId size");
    ncclUniqueId u;
    ncclResult_t r = ncclGetUniqueId(&u);
    RS_CHECK(r == ncclSuccess, RS_ERR_RCCL, "ncclGetUniqueId failed: %s", ncclGetErrorString(r));
    std::memcpy(id, &u, sizeof(u));
    return RS_OK;
}

int rs_vt_attach_comm(rs_vt* h, int rank, int nranks, const uint8_t id[RS_UNIQUE_ID_BYTES]) {
    rs::clear_error();
    RS_CHECK(h && id, RS_ERR_ARG, "null argument");
    RS_CHECK(nranks >= 1 && rank >= 0 && rank < nranks, RS_ERR_ARG, "bad rank %d of %d", rank, nranks);
    RS_CHECK(h->count == 0 && h->comm == nullptr, RS_ERR_STATE,
             "attach the communicator before adding templates, once");
    RS_HIP(hipSetDevice(h->device));
    {  // also for nranks == 1: rs_vt_match_stream then runs its collective path
        ncclUniqueId u;
        std::memcpy(&u, id, sizeof(u));
        ncclComm_t comm = nullptr;  // kept only on success: destroy never sees a failed init
        ncclResult_t r = ncclCommInitRank(&comm, nranks, u, rank);
        RS_CHECK(r == ncclSuccess, RS_ERR_RCCL, "ncclCommInitRank failed: %s", ncclGetErrorString(r));
        h->comm = comm;
    }
    h->rank = rank;
    h->nranks = nranks;
    return RS_OK;
}

}  // extern "C"
