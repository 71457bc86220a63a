// Pose-cell network step on MI355X (gfx950).
//
// Replaces PoseCellNetwork.update (the reference's ratslam/posecell_network.py:326-353)
// and the three OpenCL kernels it drives through Convolution.conv_im
// (convolution.py:228-246 `conv`, :320-340 `conv_xy_origin_filters`,
// :344-359 `conv_z`) plus the host-side numpy passes between them.
//
// A step: the 3-D DoG excitation as the exact rank-2 separable form (ge^3 - gi^3)*scale,
// three 7-tap passes per Gaussian, the global inhibition relu(v - 0.2) and per-block
// float64 partial sums of the total; then the per-layer shifted 7x7 filter (path
// integration), clamp, 7-tap theta filter, clamp, the division by the total and the
// argmax (first max in the reference's C order).  max(conv(Q/t), 0) == max(conv(Q), 0)/t
// for t > 0, so the normalisation is applied once, at the end of the step.
//
// Four kernel families ("forms"), one per handle (rs_pc::form, chosen by pc_choose_form):
//   rows   : pc_rows.h,   pc_excite_rows + pc_path_rows; small grids, any filter table
//   stream : pc_stream.h, pc_excite_stream + pc_path_stream; large grids outside cols' limits
//   cols   : pc_cols.h,   pc_excite_cols + pc_path_cols; large grids
//   halo   : pc_halo.h,   pc_step_halo, one launch per step (float32, small grids)
// rows and stream keep the volume layer-major, P[th][x][y] (y fastest): each theta layer,
// the unit the path-integration shift acts on, is one contiguous periodic 2-D image.
// cols and halo keep it theta-fastest, P[x][y][th], the reference's C order (pc_thfast):
// their blocks hold whole theta columns.  Q has P's layout.  Elsewhere the reference's
// order appears only in rs_pc_read/write and in the argmax tie-break index.
#include <type_traits>
#include <utility>
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cmath>
#include <limits>
#include <cstdio>
#include <cstdlib>
#include <cstdint>
#include <cstring>
#include <thread>
#include <vector>

#include "rs_common.h"
#include "pc_ctl.h"  // FL, HALF, the control structs and their constants, the result-word sentinels
#include "pc_peak_rule.h"  // the packet's circular centroid: the six sums of a wrapped box

// The device code, in the order of definition (pc_device.h: what every form uses;
// pc_state.h: the kernels on the stored state and the result words).  The headers are
// parts of this translation unit, not free-standing: one object, so the file-wide
// kernel-argument preload applies to every kernel.
#include "pc_device.h"
#include "pc_rows.h"
#include "pc_stream.h"
#include "pc_cols.h"
#include "pc_halo.h"
#include "pc_state.h"

// ===========================================================================
// Host side
// ===========================================================================
// Tables of path_integration's control (rs_pc_set_odometry_tables): NumPy-evaluated
// cos/sin per layer, the LUT key -> filter row map and the theta filters per origin.
struct OdoTables {
    int TH = 0;
    double vtScale = 0.0, vrScale = 0.0;
    const double* cosA = nullptr;
    const double* sinA = nullptr;
    int keyMin = 0, nKeys = 0;
    const int32_t* keyRows = nullptr;
    int zMin = 0, nZ = 0;
    const double* zfTab = nullptr;
    std::vector<double> own;        // owned copies when held by a handle
    std::vector<int32_t> ownRows;
};
static void fill_odo(OdoTables& o, int TH, double vt_scale, double vr_scale, const double* cos_a, const double* sin_a,
                     int key_min, int nkeys, const int32_t* key_rows, int z_min, int nz, const double* zf_table) {
    o.TH = TH; o.vtScale = vt_scale; o.vrScale = vr_scale;
    o.cosA = cos_a; o.sinA = sin_a;
    o.keyMin = key_min; o.nKeys = nkeys; o.keyRows = key_rows;
    o.zMin = z_min; o.nZ = nz; o.zfTab = zf_table;
}

// The step-kernel family of a handle (the file's header comment; rs_pc_step_form names it).
enum class PcForm { Rows, Stream, Cols, Halo };

// The buffers are rs::DevBuf / rs::PinnedBuf members (rs_common.h; untyped ones count bytes,
// the element being esz wide).  Group capacities: resCap (dRes, hRes, dArgV, dArgI), ctlCap.
// The stream and the events are rs::Stream / rs::Event owners.
struct rs_pc {
    int X = 0, Y = 0, TH = 0, prec = RS_PREC_F32, device = 0;
    size_t n = 0, esz = 4;
    rs::DevBuf<void> dP;
    rs::DevBuf<void> dQ;
    rs::DevBuf<void> dFilt;
    int nf = 0;
    rs::DevBuf<double> dPart;
    int nPart = 0;               // blocks of a step kernel (excitation and path alike; set by the form)
    rs::DevBuf<void> dBmax;      // f64 argmax partials (max(nPart, argmax grid))
    rs::DevBuf<unsigned> dBidx;
    int nBmaxCap = 0;
    rs::DevBuf<unsigned long long> dRes;
    int resCap = 0;
    rs::DevBuf<void> dArgV;       // per-step per-block argmax partials [resCap][nPart]
    rs::DevBuf<unsigned> dArgI;
    rs::PinnedBuf<unsigned long long> hRes;  // fine-grained; dev(): where pc_res_export stores
    rs::DevBuf<unsigned char> dCtl;
    rs::PinnedBuf<unsigned char> hCtl;
    size_t ctlStride = 0;
    int ctlCap = 0;
    rs::DevBuf<double> dTmp;             // export/import staging (n doubles)
    rs::DevBuf<double> dScalar;
    SepKernel<float> kf{};
    SepKernel<double> kd{};
    float lastMs = 0.f;
    bool profiling = false;  // HIP events around the whole call (device_ms)
    bool profKernels = false;  // ... and around every launch (kernel_ms; the events add gaps)
    double kernelMs[2] = {0.0, 0.0};
    PcForm form = PcForm::Rows;  // the step-kernel family (pc_choose_form); its geometry below
    int rowsYP = 0;         // rows: the kernels' YP instance, 64 (Y <= 64) or 128 (Y <= 128)
    rs::DevBuf<unsigned long long> dRec;     // halo: the last launch's per-block (key of max U, near count)
    rs::PinnedBuf<unsigned long long> hRec;  // ... for a one-step call: pinned host records
    rs::PinnedBuf<unsigned> hFlag;           // halo: pc_halo_finish's per-block flags (pinned; eager readback polls)
    rs::PinnedBuf<unsigned long long> hKey;  // halo: pc_halo_finish's per-block keys of a call's last step (pinned)
    unsigned flagSeq = 0u;
    bool haloPend = false;  // halo: the state is U, unnormalised, in buffer haloCur (0 dP, 1 dQ) with
    int haloCur = 0, haloPart = 0;  // its partial sums in half haloPart of dPart (pc_halo_settle)
    long haloAmbig = 0;     // calls whose last step was keyed by the finishing pass (RES_AMBIG)
    bool haloSettleAlways = false;  // rs_pc_debug(RS_PC_DBG_HALO_SETTLE)
    int cgx = 0, cgy = 0;   // cols, halo: tiles along x and y (CO_TX x CO_TY, HF_T x HF_T)
    int coKC = 0, coNch = 1;  // cols: layers per theta chunk (KC == TH: whole extent, no halo), chunks
    int sbx = 1, swr = 8, swc = 1;  // stream: BX rows per wave, WR row groups, WC column tiles
    StreamGrid sg{};
    // odometry -> control tables (rs_pc_set_odometry_tables) and per-call scratch
    bool odoReady = false;
    OdoTables odo{};
    std::vector<int32_t> cOx, cOy, cRows;
    std::vector<double> cZf;
    bool dbgSkipExport = false;  // rs_pc_debug(RS_PC_DBG_SKIP_EXPORT): the next run leaves hRes unwritten
    rs::PinnedBuf<double> hRead; // rs_pc_read: pinned float64 volume the export kernel writes in place
    // sub-cell peak (rs_pc_set_peak_tables): the box radius (0: no tables yet), the axes' sin | cos
    // weights, and six sums per step where pc_peak_kernel stores them (pinned; dev(): its address)
    int peakR = 0;
    rs::DevBuf<double> dPeakTab;
    rs::PinnedBuf<double> hPeak;
    // injections inside a run (rs_pc_run_odom_inject): each one's resolved C-order cell, on the
    // device for the call's same-as injections and in pinned memory for the host
    rs::DevBuf<unsigned> dInj;
    rs::PinnedBuf<unsigned> hInj;
    // the owners come after the buffers: members go in reverse order, streams and events first
    rs::Stream stream;
    rs::Event ev0, ev1;             // around the whole call (profiling)
    std::vector<rs::Event> evPool;  // around every launch (profKernels; pc_ensure_events)
};

namespace {

// P (and Q) theta-fastest, the reference's C order (x, y, th): the column and halo
// forms; the others keep P layer-major
inline bool pc_thfast(const rs_pc* h) { return h->form == PcForm::Cols || h->form == PcForm::Halo; }

// The handle's precision as a type: f(T{}) with T float or double (f a generic lambda
// that takes `auto t` and names the type decltype(t); both results of one type).
template <typename F>
__attribute__((always_inline)) inline auto pc_by_prec(const rs_pc* h, F&& f) {
    return h->prec == RS_PREC_F32 ? f(float{}) : f(double{});
}
using rs::Int;

// Per-step buffers of a call of n steps, grown in powers of two: the result slots and
// words always; the control ring (pinned staging + device copy, ctlStride bytes a step)
// only for the forms that read it (ctl): the halo and column forms take each step's
// control as kernel arguments, and a 10,000-step batch's 16 MiB of pinned ring was a
// few milliseconds of page-locking inside its first call.
constexpr unsigned PC_FINE = hipHostMallocMapped | hipHostMallocCoherent;

int pc_grow_steps(rs_pc* h, int n, bool ctl = true) {
    if (n > h->resCap) {
        const int cap = rs::grown(h->resCap, n, 16);
        h->resCap = 0;
        RS_TRY(h->dRes.reserve((size_t)RES_SLOTS * cap));
        // every slot starts zeroed (the excitation's block 0 zeroes a step's slots again
        // before its path kernel max-reduces into them; no step ever reads freed data)
        RS_HIP(hipMemsetAsync(h->dRes.get(), 0, sizeof(unsigned long long) * RES_SLOTS * cap, h->stream.get()));
        // the export kernel stores each step's key here with a system-scope store:
        // fine-grained (coherent) host memory, so the store is visible once the stream
        // has synchronised; pc_run_impl also checks a sentinel per step (RES_NONE)
        RS_TRY(h->hRes.reserve((size_t)cap, PC_FINE));
        for (int s = 0; s < cap; ++s) h->hRes.get()[s] = RES_NONE;
        if (h->prec == RS_PREC_F64) {  // float64 argmax: per-block partials + pc_argmax_steps
            RS_TRY(h->dArgV.reserve(h->esz * (size_t)cap * h->nPart));
            RS_TRY(h->dArgI.reserve((size_t)cap * h->nPart));
        }
        h->resCap = cap;
    }
    if (ctl && n > h->ctlCap) {
        const int cap = rs::grown(h->ctlCap, n, 16);
        h->ctlCap = 0;
        RS_TRY(h->dCtl.reserve(h->ctlStride * cap));
        RS_TRY(h->hCtl.reserve(h->ctlStride * cap, hipHostMallocDefault));
        h->ctlCap = cap;
    }
    return RS_OK;
}

// A pool of `need` events at least.  The missing ones are created whole or not at all: a
// refused creation leaves the pool at its old size.
int pc_ensure_events(rs_pc* h, size_t need) {
    std::vector<rs::Event> fresh(need > h->evPool.size() ? need - h->evPool.size() : 0);
    for (rs::Event& e : fresh) RS_TRY(e.create());
    for (rs::Event& e : fresh) h->evPool.push_back(std::move(e));
    return RS_OK;
}

// control record: int32 ox[TH] | int32 oy[TH] | int32 fidx[TH] | pad | double zf[8]
inline size_t ctl_off_oy(const rs_pc* h) { return sizeof(int32_t) * h->TH; }
inline size_t ctl_off_f(const rs_pc* h) { return 2 * sizeof(int32_t) * h->TH; }
inline size_t ctl_off_zf(const rs_pc* h) { return rs::round_up(3 * sizeof(int32_t) * h->TH, 16); }

int pc_check_ctl(const rs_pc* h, int n, const int32_t* ox, const int32_t* oy,
                 const int32_t* fidx, const double* zf) {
    RS_CHECK(ox && oy && fidx && zf, RS_ERR_ARG, "null control array");
    for (size_t e = 0; e < (size_t)n * h->TH; ++e) {
        const int32_t f = fidx[e];
        RS_CHECK(f >= 0 && f < h->nf, RS_ERR_ARG,
                 "step %d layer %d: filter index %d outside the table [0, %d)", (int)(e / h->TH),
                 (int)(e % h->TH), f, h->nf);
        if (h->TH <= CTL_INLINE_MAX)
            RS_CHECK(ox[e] >= -32768 && ox[e] <= 32767 && oy[e] >= -32768 && oy[e] <= 32767,
                     RS_ERR_ARG, "shift (%d, %d) outside the int16 inline control", ox[e], oy[e]);
    }
    return RS_OK;
}

int pc_pack_ctl(rs_pc* h, int n, const int32_t* ox, const int32_t* oy, const int32_t* fidx,
                const double* zf, unsigned char* dst = nullptr) {
    const int TH = h->TH;
    for (int s = 0; s < n; ++s) {
        unsigned char* rec = (dst ? dst : h->hCtl.get()) + (size_t)s * h->ctlStride;
        std::memcpy(rec, ox + (size_t)s * TH, sizeof(int32_t) * TH);
        std::memcpy(rec + ctl_off_oy(h), oy + (size_t)s * TH, sizeof(int32_t) * TH);
        std::memcpy(rec + ctl_off_f(h), fidx + (size_t)s * TH, sizeof(int32_t) * TH);
        std::memcpy(rec + ctl_off_zf(h), zf + (size_t)s * FL, sizeof(double) * FL);
    }
    return RS_OK;
}

template <typename T>
const SepKernel<T>& sep_of(const rs_pc* h);
template <>
const SepKernel<float>& sep_of<float>(const rs_pc* h) { return h->kf; }
template <>
const SepKernel<double>& sep_of<double>(const rs_pc* h) { return h->kd; }

// Control of step s as pointers into its device ring record (as a kernel argument,
// TH <= CTL_INLINE_MAX: make_ctl_inline, pc_ctl.h).
PcCtlRing make_ctl_ring(const rs_pc* h, int s) {
    const unsigned char* rec = h->dCtl.get() + (size_t)s * h->ctlStride;
    return PcCtlRing{reinterpret_cast<const int*>(rec),
                     reinterpret_cast<const int*>(rec + ctl_off_oy(h)),
                     reinterpret_cast<const int*>(rec + ctl_off_f(h)),
                     reinterpret_cast<const double*>(rec + ctl_off_zf(h))};
}

void decode_xyz(const rs_pc* h, unsigned long long key, int32_t* out) {
    const unsigned lin = 0xFFFFFFFFu - (unsigned)(key & 0xFFFFFFFFull);
    out[2] = (int32_t)(lin % (unsigned)h->TH);
    const unsigned xy = lin / (unsigned)h->TH;
    out[1] = (int32_t)(xy % (unsigned)h->Y);
    out[0] = (int32_t)(xy / (unsigned)h->Y);
}

// Where step s of a launch sequence leaves its results: its RES_SLOTS argmax
// slots, and (float64) its per-block argmax partials.
struct StepOut {
    unsigned long long* slot;
    void* bmax;
    unsigned* bidx;
};
inline StepOut step_out(const rs_pc* h, int s) {
    return StepOut{h->dRes.get() + (size_t)s * RES_SLOTS,
                   h->dArgV.get() ? static_cast<char*>(h->dArgV.get()) + h->esz * (size_t)s * h->nPart : nullptr,
                   h->dArgI.get() ? h->dArgI.get() + (size_t)s * h->nPart : nullptr};
}

// Wait for a call's result words (pinned host memory, each one 8-byte system-scope store
// by the call's last kernel) instead of the stream's completion signal: a bounded spin
// (rs::spin_until) that returns true once every word of steps [s0, s1) holds a key, false
// when it runs out (the caller then synchronises the stream, which returns any error).
// Safe for the same reason as the halo form's record polling (pc_run_halo): the host reads
// nothing else the call wrote, and every later device access is ordered on the stream.
bool pc_poll_words(const rs_pc* h, int s0, int s1) {
    const volatile unsigned long long* w = h->hRes.get() + s0;
    return rs::spin_until(s1 - s0, [w](int s) { return w[s] != RES_NONE; });
}

// An eager halo call (the volume written into the caller's pinned array) polls the
// finishing blocks' flags instead of the stream's completion when it is short and not
// profiled; RS_PC_HALO_FLAGS=0 keeps the stream synchronisation for it.
bool halo_poll_env() { static const bool on = rs::env_on("RS_PC_HALO_POLL"); return on; }
bool halo_flags_env() { static const bool on = rs::env_on("RS_PC_HALO_FLAGS"); return on; }
// pc_halo_finish's grid: 256 threads, a float4 each per pass
inline int hf_finish_blocks(const rs_pc* h) { return (int)std::min<size_t>(1024, (h->n / 4 + 255) / 256); }

// Spin until a volume-writing launch's nb blocks have each stored flag value seq (bounded;
// false when the spin runs out and the caller must synchronise the stream instead).
bool pc_poll_flags(const rs_pc* h, int nb, unsigned seq) {
    const volatile unsigned* f = h->hFlag.get();
    return rs::spin_until(nb, [f, seq](int b) { return f[b] == seq; });
}

// The next flag value of a volume-writing launch the host will poll (0 is the flags'
// initial value, never a live one), and whether a launch of nb blocks may be polled.
unsigned pc_next_seq(rs_pc* h) {
    unsigned seq = ++h->flagSeq;
    if (seq == 0u) seq = ++h->flagSeq;
    return seq;
}
bool pc_flags_ok(const rs_pc* h, int nb) {
    return halo_poll_env() && halo_flags_env() && h->hFlag.get() && !h->profiling && nb <= HF_FLAGS;
}
// ... and whether an n-step halo call with an eager readback (xp) may poll its finishing pass
bool xp_poll_ok(const rs_pc* h, int n, const double* xp) {
    return xp && pc_flags_ok(h, hf_finish_blocks(h)) && !h->dbgSkipExport && n <= HF_POLL_MAX;
}

// The only launch of pc_halo_finish: U in buffer src_buf (0 dP, 1 dQ), its partial sums in
// half part_half of dPart, normalised into dP; the handle's state is settled after it.
// What else the pass leaves is the caller's choice:
struct HaloFinishOut {
    unsigned long long* slot = nullptr;  // the last step's slots: every block max-reduces its key into them
    int nexp = 0;           // > 0, the call's own key export: block 0 stores the words of steps 0 .. nexp-2
                            // into hRes, every block its key of step nexp-1 into hKey (zeroed here)
    double* xp = nullptr;   // the float64 C-order volume (a pinned array's device address)
    unsigned* flag = nullptr;  // per-block flags set to seq behind the block's volume stores
    unsigned seq = 0u;
};
int pc_launch_halo_finish(rs_pc* h, int src_buf, int part_half, const HaloFinishOut& o = {}) {
    float* buf[2] = {static_cast<float*>(h->dP.get()), static_cast<float*>(h->dQ.get())};
    const int n4 = (int)(h->n / 4), nb = hf_finish_blocks(h);
    if (o.nexp > 0) std::memset(h->hKey.get(), 0, sizeof(unsigned long long) * nb);
    hipLaunchKernelGGL(pc_halo_finish, dim3(nb), dim3(256), 0, h->stream.get(), buf[src_buf], buf[0], n4,
                       h->dPart.get() + (size_t)part_half * h->nPart, h->nPart, o.slot, h->dRes.get(), o.nexp,
                       h->hRes.dev(), o.nexp > 0 ? h->hKey.dev() : nullptr, o.xp, (int)(h->n * sizeof(float)),
                       o.flag, o.seq);
    RS_HIP(hipGetLastError());
    h->haloPend = false;
    h->haloCur = 0;
    return RS_OK;
}

// The only launch of pc_step_halo (EXC: its excitation-only instance), forming the
// arguments the kernel has preloaded: the grid, the tile counts and the union's origin and
// extent as 16-bit pairs, and the two high-multiply divisors.
template <bool EXC>
int pc_launch_halo_step(rs_pc* h, const float* src, float* dst, const double* part_in, int npart_in,
                        double* part_out, unsigned long long* prev_slot, unsigned long long* slot,
                        const PcCtlHalo& c, unsigned long long* rec) {
    const int nblk = h->cgx * h->cgy;
    hf_launch<EXC>(h->TH, dim3(nblk), h->stream.get(), src, hf_pack(h->X, h->Y), hf_pack(h->cgx, nblk),
                   hf_pack(c.ux, c.uy), hf_pack(c.uw, c.uh), hf_magic(h->cgx), hf_magic(c.uh), part_in, npart_in, dst,
                   part_out, prev_slot, slot, static_cast<const float*>(h->dFilt.get()), h->nf, c, h->kf, rec);
    RS_HIP(hipGetLastError());
    return RS_OK;
}

// The only launch of pc_export2_kernel: the float64 C-order volume into pinned host
// memory (dst: its device address).  *seq != 0: the launch's *nb blocks each set their
// flag to it and the host may poll them (pc_poll_flags); the grid is then at most 128
// blocks, each thread storing a few 16-byte pieces (fewer blocks, fewer flags; 64x64x36
// rows-form read 32-36 us at 32-128 blocks against 36-37 at 289, within the boxes'
// spread, tools/node_step.py, round 5).
int pc_launch_export(rs_pc* h, double* dst, bool may_poll, int* nb, unsigned* seq) {
    int xnb = (int)std::min<size_t>(1024, (h->n / 2 + NT - 1) / NT + 1);
    const bool fl = may_poll && pc_flags_ok(h, xnb);
    if (fl) xnb = std::min(xnb, 128);
    *nb = xnb;
    *seq = fl ? pc_next_seq(h) : 0u;
    pc_by_prec(h, [&](auto t) {
        using T = decltype(t);
        hipLaunchKernelGGL((pc_export2_kernel<T>), dim3(xnb), dim3(NT), 0, h->stream.get(),
                           static_cast<const T*>(h->dP.get()), dst, h->X, h->Y, h->TH, (int)pc_thfast(h),
                           fl ? h->hFlag.dev() : nullptr, *seq);
    });
    RS_HIP(hipGetLastError());
    return RS_OK;
}

// Room for the six sums of each of a peaks call's n steps (grown in powers of two; every
// earlier peaks call has synchronised the stream, so no launch still stores into the old block).
int pc_grow_peaks(rs_pc* h, int n) {
    return h->hPeak.reserve(6 * rs::grown<size_t>(0, (size_t)n, 16), PC_FINE);
}

// The only launch of pc_peak_kernel: the sums of step s of a peaks call (hPeak[6s ..]) from the
// state in P, keyed by the step's slot words (slot) or by nb block partials (bmax, bidx).
int pc_launch_peak(rs_pc* h, const void* P, const unsigned long long* slot, const void* bmax,
                   const unsigned* bidx, int nb, int s) {
    pc_by_prec(h, [&](auto t) {
        using T = decltype(t);
        hipLaunchKernelGGL((pc_peak_kernel<T>), dim3(1), dim3(64), 0, h->stream.get(), static_cast<const T*>(P), h->X,
                           h->Y, h->TH, (int)pc_thfast(h), h->peakR, slot, static_cast<const T*>(bmax), bidx, nb,
                           h->dPeakTab.get(), h->hPeak.dev() + 6 * (size_t)s);
    });
    RS_HIP(hipGetLastError());
    return RS_OK;
}

// The stored state's per-block argmax partials into dBmax / dBidx (*nb_out of them).
int pc_launch_argmax_blocks(rs_pc* h, int* nb_out) {
    const int nb = h->nBmaxCap < 1024 ? h->nBmaxCap : 1024;
    *nb_out = nb;
    pc_by_prec(h, [&](auto t) {
        using T = decltype(t);
        hipLaunchKernelGGL((pc_argmax_blocks<T>), dim3(nb), dim3(NT), 0, h->stream.get(), static_cast<const T*>(h->dP.get()),
                           h->X, h->Y, h->TH, static_cast<T*>(h->dBmax.get()), h->dBidx.get(), (int)pc_thfast(h));
    });
    RS_HIP(hipGetLastError());
    return RS_OK;
}

// A run's injections (rs_pc_run_odom_inject; checked by pc_check_inj): ni of them, in the
// order of their steps.
struct PcInj {
    int ni = 0;
    const int32_t* step = nullptr;
    const double* energy = nullptr;
    const int32_t* loc = nullptr;   // [3 ni]: (x, y, th) | (RS_PC_INJ_AT_PEAK, ., .) | (RS_PC_INJ_SAME_AS, k, .)
};

// Where the first maximum of the state in dP is keyed on the device, when it is: a float32
// step's slot words, or nb block partials (pc_inject_run_kernel reads either).
struct PcKeySrc {
    const unsigned long long* slot = nullptr;
    const void* bmax = nullptr;
    const unsigned* bidx = nullptr;
    int nb = 0;
    bool valid() const { return slot || bmax; }
};
inline PcKeySrc step_key(const rs_pc* h, const StepOut& so) {
    return h->prec == RS_PREC_F32 ? PcKeySrc{so.slot, nullptr, nullptr, 0} : PcKeySrc{nullptr, so.bmax, so.bidx, h->nPart};
}

int pc_grow_inj(rs_pc* h, int ni) {
    if ((size_t)ni <= h->dInj.capacity()) return RS_OK;
    // (every call with injections has synchronised the stream: nothing still uses the old blocks)
    const size_t cap = rs::grown<size_t>(0, (size_t)ni, 64);
    RS_TRY(h->hInj.reserve(cap, PC_FINE));
    RS_TRY(h->dInj.reserve(cap));
    RS_HIP(hipMemsetAsync(h->dInj.get(), 0xFF, sizeof(unsigned) * cap, h->stream.get()));
    return RS_OK;
}

// The injection point in front of step s (s == n: behind the last step): every injection
// of the call with that step, in order, one pc_inject_run_kernel launch each, on the settled
// state in dP.  key: where that state's first maximum is keyed, if a step of this call left
// it; an at-peak injection without one -- before step 0, or behind another injection of this
// point, which changed the state -- takes pc_argmax_blocks' partials of dP as it stands.
int pc_inject_point(rs_pc* h, const PcInj& inj, int* cur, int s, PcKeySrc key) {
    for (; *cur < inj.ni && inj.step[*cur] == s; ++*cur) {
        const int i = *cur;
        const int32_t* loc = inj.loc + 3 * (size_t)i;
        int src = PC_INJ_EXPLICIT;
        unsigned arg = 0u;
        if (loc[0] == RS_PC_INJ_AT_PEAK) {
            src = PC_INJ_KEY;
            if (!key.valid()) {
                int nb = 0;
                RS_TRY(pc_launch_argmax_blocks(h, &nb));
                key = PcKeySrc{nullptr, h->dBmax.get(), h->dBidx.get(), nb};
            }
        } else if (loc[0] == RS_PC_INJ_SAME_AS) {
            src = PC_INJ_SAME;
            arg = (unsigned)loc[1];
        } else {
            arg = ((unsigned)loc[0] * h->Y + loc[1]) * h->TH + loc[2];
        }
        pc_by_prec(h, [&](auto t) {
            using T = decltype(t);
            hipLaunchKernelGGL((pc_inject_run_kernel<T>), dim3(1), dim3(64), 0, h->stream.get(), static_cast<T*>(h->dP.get()),
                               h->X, h->Y, h->TH, (int)pc_thfast(h), src, arg, key.slot, static_cast<const T*>(key.bmax),
                               key.bidx, key.nb, h->dInj.get(), h->hInj.dev(), i, inj.energy[i]);
        });
        RS_HIP(hipGetLastError());
        key = PcKeySrc{};   // the state has changed
    }
    return RS_OK;
}

// The end of a call of n steps, either run path: no result word may still hold the
// sentinel once the call has been waited for; the call's device time; the keys decoded.
int pc_end_call(rs_pc* h, int n, int32_t* out_xyz) {
    for (int s = 0; s < n; ++s)
        RS_CHECK(h->hRes.get()[s] != RES_NONE, RS_ERR_HIP,
                 "step %d of %d: its argmax key did not reach the host result buffer after the "
                 "stream synchronised", s, n);
    if (h->profiling) RS_HIP(hipEventElapsedTime(&h->lastMs, h->ev0.get(), h->ev1.get()));
    else h->lastMs = 0.f;  // the call-bracketing events are recorded only while profiling
    if (out_xyz)
        for (int s = 0; s < n; ++s) decode_xyz(h, h->hRes.get()[s], out_xyz + 3 * (size_t)s);
    return RS_OK;
}

// The halo form's state left unnormalised by a call (U in buffer haloCur, its partial
// sums in half haloPart of dPart), normalised into dP: the entry points that read or
// change the state directly (read, write, inject, get_max, total, excite, debug) settle
// it first.  (The next call's first launch consumes it as it is: it scales on load.)
int pc_halo_settle(rs_pc* h) {
    return h->haloPend ? pc_launch_halo_finish(h, h->haloCur, h->haloPart) : RS_OK;
}

// A volume read of a state a halo call left unnormalised (the ROS node's `.posecells`
// after update()): the finishing kernel normalises the state and writes the float64
// C-order volume into the pinned destination in the same pass (the eager readback's
// kernel: one launch in place of the settle and the export kernel), and the host waits
// for its blocks' flags -- each released at system scope after the block's volume
// stores -- instead of the stream's completion (RS_PC_HALO_POLL=0 or RS_PC_HALO_FLAGS=0:
// the stream synchronisation).  The host reads only what this kernel wrote, so the
// early return is safe as the eager call's is (pc_run_halo).  *done is false when no
// state is pending (the caller exports as usual).
int pc_halo_settle_read(rs_pc* h, double* xp_dev, bool* done) {
    *done = false;
    if (!h->haloPend) return RS_OK;
    const int nb = hf_finish_blocks(h);
    const bool fl = pc_flags_ok(h, nb);
    const unsigned seq = fl ? pc_next_seq(h) : 0u;
    RS_TRY(pc_launch_halo_finish(h, h->haloCur, h->haloPart, {nullptr, 0, xp_dev, fl ? h->hFlag.dev() : nullptr, seq}));
    if (!(fl && pc_poll_flags(h, nb, seq))) RS_HIP(hipStreamSynchronize(h->stream.get()));
    *done = true;
    return RS_OK;
}

// How a halo-form call ends (pc_run_halo): the last launch's per-block records of U in pinned
// host memory, reduced by the host after its wait (a one-step call: no export launch); the
// records on the device and pc_halo_export; or the finishing pass, pc_halo_finish.
enum class HaloEnd { HostRecords, DevRecords, Finish };

// n steps of the halo form: one launch each (step s reads the state in one buffer,
// scaled by the partials of the step before, and writes U into the other; the partial
// sums ping-pong between the two halves of dPart).  Then, by default, the call ends with
// the state left unnormalised (haloPend) and one small export launch (pc_halo_export):
// steps 0 .. n-2 keyed by the launch after each, step n-1 from the last launch's
// per-block records of U -- the finishing pass over the volume (pc_halo_finish) is off
// the per-call path (update() at 64x64x36: about 4 us of device time per call).  With an
// eager readback (xp: the float64 volume into the caller's pinned array), or when the
// records cannot settle the last step's first maximum (RES_AMBIG: a cell within
// HF_NEAR of the peak), pc_halo_finish normalises the state into dP, keys it and
// exports.  One host sync (two for RES_AMBIG).  rs_pc_debug(RS_PC_DBG_HALO_SETTLE) makes
// every later call finish.
// With injections (inj): an injection point settles a pending state with one pc_halo_finish --
// in front of step s > 0 it keys step s-1 in its slots from the normalised state, where an
// at-peak injection and the step's peak launch find it -- and the step behind it starts from
// the settled state in dP, as a call's first step does; the call always finishes.
int pc_run_halo(rs_pc* h, int n, const int32_t* ox, const int32_t* oy, const int32_t* fidx,
                const double* zf, int32_t* out_xyz, double* xp, double* sums, const PcInj* inj) {
    RS_TRY(pc_grow_steps(h, n, false));   // (the control travels as kernel arguments)
    if (sums) RS_TRY(pc_grow_peaks(h, n));
    const bool pk = h->profiling && h->profKernels;
    if (pk) RS_TRY(pc_ensure_events(h, (size_t)2 * n + 2));
    for (int s = 0; s < n; ++s) h->hRes.get()[s] = RES_NONE;
    // RS_PC_HALO_POLL=0: a one-step call waits for the kernel's completion signal instead
    // of returning once every block's record has reached host memory (below)
    const bool poll_env = halo_poll_env();
    // A peaks call (sums) finishes too: its last step is then keyed in last_slot from the
    // normalised state in dP, where the step's peak launch finds both (never RES_AMBIG)
    const HaloEnd end = xp || sums || inj || h->haloSettleAlways ? HaloEnd::Finish
                        : n == 1 && h->hRec.get()     ? HaloEnd::HostRecords
                                                      : HaloEnd::DevRecords;
    const bool lazy = end != HaloEnd::Finish;
    if (end == HaloEnd::HostRecords) std::memset(h->hRec.get(), 0, sizeof(unsigned long long) * 2 * h->nPart);
    if (h->profiling) RS_HIP(hipEventRecord(h->ev0.get(), h->stream.get()));

    // 1. the steps
    float* buf[2] = {static_cast<float*>(h->dP.get()), static_cast<float*>(h->dQ.get())};
    double* part[2] = {h->dPart.get(), h->dPart.get() + h->nPart};
    bool pend = h->haloPend;            // the state is U in buf[cb], its partials in part[ph]
    int cb = pend ? h->haloCur : 0;     // the buffer the next step reads
    int ph = pend ? h->haloPart : 1;    // the next step writes the other half (a settled state: half 0)
    int icur = 0;                       // the next injection
    unsigned long long* const last_slot = h->dRes.get() + (size_t)(n - 1) * RES_SLOTS;
    for (int s = 0; s < n; ++s) {
        unsigned long long* const prev = s > 0 ? h->dRes.get() + (size_t)(s - 1) * RES_SLOTS : nullptr;
        // an injection point: step s-1 is keyed and its peak taken from the settled state here
        const bool point = inj && icur < inj->ni && inj->step[icur] == s;
        if (point) {
            if (pend) RS_TRY(pc_launch_halo_finish(h, cb, ph, {prev}));
            pend = false, cb = 0, ph = 1;
            if (sums && s > 0) RS_TRY(pc_launch_peak(h, buf[0], prev, nullptr, nullptr, 0, s - 1));
            RS_TRY(pc_inject_point(h, *inj, &icur, s, PcKeySrc{prev, nullptr, nullptr, 0}));
        }
        PcCtlHalo c;
        make_ctl_halo(h->X, h->Y, h->TH, ox + (size_t)s * h->TH, oy + (size_t)s * h->TH, fidx + (size_t)s * h->TH,
                      zf + (size_t)s * FL, &c);
        unsigned long long* const slot = h->dRes.get() + (size_t)s * RES_SLOTS;
        unsigned long long* rec = nullptr;   // the last launch's records, where the ending reads them
        if (lazy && s == n - 1) rec = end == HaloEnd::HostRecords ? h->hRec.dev() : h->dRec.get();
        if (pk) RS_HIP(hipEventRecord(h->evPool[2 * s].get(), h->stream.get()));
        RS_TRY(pc_launch_halo_step<false>(h, buf[cb], buf[cb ^ 1], part[pend ? ph : 0], pend ? h->nPart : 0,
                                          part[ph ^ 1], point ? nullptr : prev, slot, c, rec));
        if (pk) RS_HIP(hipEventRecord(h->evPool[2 * s + 1].get(), h->stream.get()));
        // step s-1's key is complete now (this launch reduced it into slot - RES_SLOTS from the
        // state it loaded), and its U stays in the buffer this launch read until launch s+1
        // overwrites it: the peak launch of step s-1 goes between the two
        if (sums && s > 0 && !point) RS_TRY(pc_launch_peak(h, buf[cb], prev, nullptr, nullptr, 0, s - 1));
        pend = true, cb ^= 1, ph ^= 1;
    }
    const int cl = cb, pl = ph;   // where the last U and its partials are

    // 2. the ending
    const int nb = hf_finish_blocks(h);
    // an eager readback the host may poll for (per-block flags behind a system-scope release)
    const bool flag_poll = !sums && xp_poll_ok(h, n, xp);
    const unsigned seq = flag_poll ? pc_next_seq(h) : 0u;
    const bool skipped = h->dbgSkipExport;
    // own export: pc_halo_finish stores the words of steps 0 .. n-2 itself, and every block
    // its key of step n-1 into hKey, reduced below once the launch has been waited for
    const bool own_export = end == HaloEnd::Finish && !skipped && n <= HF_EXP_MAX;
    if (pk) RS_HIP(hipEventRecord(h->evPool[2 * n].get(), h->stream.get()));
    if (end == HaloEnd::DevRecords && !skipped) {
        hipLaunchKernelGGL(pc_halo_export, dim3(n < 1024 ? n : 1024), dim3(64), 0, h->stream.get(), h->dRes.get(), n,
                           h->dRec.get(), h->nPart, h->hRes.dev());
        RS_HIP(hipGetLastError());
    }
    if (end == HaloEnd::Finish) {
        RS_TRY(pc_launch_halo_finish(h, cl, pl, {last_slot, own_export ? n : 0, xp, flag_poll ? h->hFlag.dev() : nullptr, seq}));
        // the last step's peak: the normalised state in dP, its keys in last_slot
        if (sums) RS_TRY(pc_launch_peak(h, buf[0], last_slot, nullptr, nullptr, 0, n - 1));
        // the injections behind the last step, on the state the pass has just settled and keyed
        if (inj) RS_TRY(pc_inject_point(h, *inj, &icur, n, PcKeySrc{last_slot, nullptr, nullptr, 0}));
        if (!skipped && !own_export) {
            hipLaunchKernelGGL(pc_res_export, dim3(n < 1024 ? n : 1024), dim3(64), 0, h->stream.get(), h->dRes.get(), n,
                               h->hRes.dev());
            RS_HIP(hipGetLastError());
        }
    }
    if (lazy) {
        h->haloPend = true;
        h->haloCur = cl;
        h->haloPart = pl;
    }
    h->dbgSkipExport = false;
    if (pk) RS_HIP(hipEventRecord(h->evPool[2 * n + 1].get(), h->stream.get()));
    if (h->profiling) RS_HIP(hipEventRecord(h->ev1.get(), h->stream.get()));

    // 3. the wait
    // A one-step call returns as soon as every block's record has reached the pinned host
    // array, without waiting for the kernel's completion signal and the host's wake-up
    // (update() at 64x64x36: 22.5-24.3 -> 16.8-18.9 us, tools/pc_ab.py --mode update,
    // round 5).  What makes the early return safe: the host reads nothing but the
    // records, each block's last store (one 16-byte store, both words non-zero, checked
    // after the host zeroed them); the state and every other result stay on the device,
    // and every later access to them -- the next step, a read, inject, get_max,
    // settle -- is a launch or copy ordered on this stream behind the kernel (the
    // library's volume reads into pinned memory synchronise the stream themselves).
    // A spin that runs out (a slow or faulted kernel) falls back to the stream
    // synchronisation, which returns any error.
    bool polled = false;
    if (flag_poll) {
        // the eager readback: every finishing block's flag (its volume slice released at
        // system scope before it), then every step's key word
        polled = pc_poll_flags(h, nb, seq) && pc_poll_words(h, 0, n - 1);
    } else if (lazy && !skipped && poll_env && !h->profiling && n <= HF_POLL_MAX) {
        const volatile unsigned long long* r = h->hRec.get();
        polled = end == HaloEnd::HostRecords
                     ? rs::spin_until(h->nPart, [r](int b) { return r[2 * b] != 0ull && r[2 * b + 1] != 0ull; })
                     : pc_poll_words(h, 0, n);   // the export kernel's words
    }
    // (A peaks call never polls: the early returns above are safe only because the host reads
    // nothing but the key words or flagged volume slices, and the sums are plain stores of the
    // peak launches, visible to the host once the stream has synchronised.  Nor does a call
    // with injections: it finishes without xp, and its resolved cells are plain stores too.)
    if (!polled) RS_HIP(hipStreamSynchronize(h->stream.get()));
    if (sums) std::memcpy(sums, h->hPeak.get(), sizeof(double) * 6 * (size_t)n);

    // 4. the last step's key
    unsigned long long& last = h->hRes.get()[n - 1];
    if (end == HaloEnd::HostRecords && !skipped) last = halo_key_from_records(h->hRec.get(), h->nPart);
    if (own_export) {   // the finishing blocks' keys of the last step (a key is never 0)
        unsigned long long m = 0ull;
        bool all = true;
        for (int b = 0; b < nb; ++b) {
            all &= h->hKey.get()[b] != 0ull;
            m = std::max(m, h->hKey.get()[b]);
        }
        last = all ? m : RES_NONE;
    }
    if (lazy && !skipped && last == RES_AMBIG) {
        // a cell within HF_NEAR of the last step's peak: key the normalised state itself
        // (its slots were zeroed by the last launch and nothing has reduced into them)
        last = RES_NONE;
        RS_TRY(pc_launch_halo_finish(h, cl, pl, {last_slot}));
        hipLaunchKernelGGL(pc_res_export, dim3(1), dim3(64), 0, h->stream.get(), last_slot, 1, h->hRes.dev() + (n - 1));
        RS_HIP(hipGetLastError());
        if (!(poll_env && pc_poll_words(h, n - 1, n))) RS_HIP(hipStreamSynchronize(h->stream.get()));
        ++h->haloAmbig;
    }
    RS_TRY(pc_end_call(h, n, out_xyz));
    if (pk) {
        h->kernelMs[0] = h->kernelMs[1] = 0.0;
        for (int s = 0; s < n; ++s) {
            float a = 0.f;
            RS_HIP(hipEventElapsedTime(&a, h->evPool[2 * s].get(), h->evPool[2 * s + 1].get()));
            h->kernelMs[0] += a;
        }
        float b = 0.f;
        RS_HIP(hipEventElapsedTime(&b, h->evPool[2 * n].get(), h->evPool[2 * n + 1].get()));
        h->kernelMs[1] = b;
    }
    return RS_OK;
}

// Streaming variants instantiated: (BX rows per wave, WR row groups, WC column tiles of 64).
#define PC_STREAM_VARIANTS(X_) X_(1, 8, 1) X_(2, 8, 1)

// f(Int<BX>, Int<WR>, Int<WC>) for the instantiated variant (bx, wr, wc), the tile as
// types; RS_ERR_ARG where no such variant is instantiated.
template <typename F>
int with_stream_variant(int bx, int wr, int wc, F&& f) {
#define PC_VARIANT(bx_, wr_, wc_) \
    if (bx == bx_ && wr == wr_ && wc == wc_) return f(Int<bx_>{}, Int<wr_>{}, Int<wc_>{});
    PC_STREAM_VARIANTS(PC_VARIANT)
#undef PC_VARIANT
    RS_CHECK(false, RS_ERR_ARG, "no streaming variant BX=%d WR=%d WC=%d", bx, wr, wc);
}

// A step of the rows, stream and cols forms: the form's kernel instance is chosen once,
// and its excitation and path launches go out from that choice (two, below).
template <typename T, typename CTL>
int pc_launch_step(rs_pc* h, const StepOut& so, const CTL* ctl, int prof_base) {
    const T* P = static_cast<const T*>(h->dP.get());
    T* Q = static_cast<T*>(h->dQ.get());
    T* Pn = static_cast<T*>(h->dP.get());
    double* part = h->dPart.get();
    const SepKernel<T>& k = sep_of<T>(h);
    unsigned long long* slot = so.slot;
    T* bmax = static_cast<T*>(so.bmax);
    unsigned* bidx = so.bidx;
    const T* filt = static_cast<const T*>(h->dFilt.get());
    // excitation, then path integration, each between its profiling events; without a
    // control the excitation alone (rs_pc_excite() normalises with pc_scale_kernel)
    auto two = [&](auto&& excite, auto&& path) -> int {
        if (prof_base >= 0) RS_HIP(hipEventRecord(h->evPool[prof_base].get(), h->stream.get()));
        excite();
        RS_HIP(hipGetLastError());
        if (prof_base >= 0) RS_HIP(hipEventRecord(h->evPool[prof_base + 1].get(), h->stream.get()));
        if (!ctl) return RS_OK;
        if (prof_base >= 0) RS_HIP(hipEventRecord(h->evPool[prof_base + 2].get(), h->stream.get()));
        path();
        RS_HIP(hipGetLastError());
        if (prof_base >= 0) RS_HIP(hipEventRecord(h->evPool[prof_base + 3].get(), h->stream.get()));
        return RS_OK;
    };
    switch (h->form) {
    case PcForm::Cols: {
        const dim3 g(h->cgx * h->cgy * h->coNch);
        // an instance: NW waves, a window of THM layers, theta-chunked or whole, and FIX, the
        // fixed theta extent of the LDS-DMA kernels (0: any).  The path kernel has its LDS-DMA
        // window instance only with the control as kernel arguments; with the ring it is
        // the whole-extent one
        auto cols = [&](auto nw, auto thm, auto chunk, auto fix) -> int {
            constexpr int NW = decltype(nw)::value, THM = decltype(thm)::value, FIX = decltype(fix)::value;
            constexpr bool CHUNK = decltype(chunk)::value;
            constexpr bool DMA = FIX != 0 && std::is_same<CTL, PcCtlInline>::value;
            constexpr int PTHM = FIX != 0 && !DMA ? co_thmax<T>() : THM;
            return two([&] { hipLaunchKernelGGL((pc_excite_cols<T, CO_TX, CO_TY, NW, THM, CHUNK, FIX>), g, dim3(64 * NW), 0,
                                                h->stream.get(), P, h->X, h->Y, h->TH, h->cgx, h->cgy, (int)g.x, Q, part, slot,
                                                h->coKC, k); },
                       [&] { hipLaunchKernelGGL((pc_path_cols<T, CO_TX, CO_TY, NW, PTHM, CHUNK, CTL, DMA ? FIX : 0>), g,
                                                dim3(64 * NW), 0, h->stream.get(), Q, h->X, h->Y, h->TH, h->cgx, h->cgy, (int)g.x,
                                                Pn, part, h->nPart, filt, h->nf, *ctl, slot, bmax, bidx, h->coKC); });
        };
        const bool whole = h->coKC >= h->TH;
        if constexpr (std::is_same<T, float>::value)
            if (whole && h->TH == CO_DMA_TH)  // configs[3]'s theta extent
                return cols(Int<CO_NW>{}, Int<CO_DMA_TH>{}, std::false_type{}, Int<CO_DMA_TH>{});
        if (whole) return cols(Int<co_nw<T>()>{}, Int<co_thmax<T>()>{}, std::false_type{}, Int<0>{});
        return cols(Int<CO_NW_CHUNK>{}, Int<co_thmax_chunk<T>()>{}, std::true_type{}, Int<0>{});
    }
    case PcForm::Stream: {
        const StreamGrid G = h->sg;
        const dim3 grid(G.gx * G.gy * G.gz), block(64 * h->swr * h->swc);
        return with_stream_variant(h->sbx, h->swr, h->swc, [&](auto bx, auto wr, auto wc) -> int {
            constexpr int BX = decltype(bx)::value, WR = decltype(wr)::value, WC = decltype(wc)::value;
            return two([&] { hipLaunchKernelGGL((pc_excite_stream<T, BX, WR, WC>), grid, block, 0, h->stream.get(), P, Q, part,
                                                slot, h->X, h->Y, h->TH, G, k); },
                       [&] { hipLaunchKernelGGL((pc_path_stream<T, BX, WR, WC, CTL>), grid, block, 0, h->stream.get(), Q, Pn, part,
                                                h->nPart, filt, h->nf, *ctl, slot, bmax, bidx, h->X, h->Y, h->TH, G); });
        });
    }
    case PcForm::Rows: {
        const dim3 g((h->X + RT_BX - 1) / RT_BX, (h->TH + RT_BK - 1) / RT_BK);
        auto rows = [&](auto yp) -> int {
            constexpr int YP = decltype(yp)::value;
            return two([&] { hipLaunchKernelGGL((pc_excite_rows<T, YP>), g, dim3(RT_NT), 0, h->stream.get(), P, Q, part, slot,
                                                h->X, h->Y, h->TH, k); },
                       [&] { hipLaunchKernelGGL((pc_path_rows<T, YP, CTL>), g, dim3(RT_NT), 0, h->stream.get(), Q, Pn, part,
                                                h->nPart, filt, h->nf, *ctl, slot, bmax, bidx, h->X, h->Y, h->TH); });
        };
        return h->rowsYP == 64 ? rows(Int<64>{}) : rows(Int<128>{});
    }
    case PcForm::Halo: break;  // one launch per step: pc_run_halo, rs_pc_excite
    }
    RS_CHECK(false, RS_ERR_STATE, "the halo form has no two-launch step");
}

// n steps launched one by one on the handle's stream, then one export and a sync.
// With injections (inj): each injection point is queued in front of its step, where the state
// is in dP and the step before's key on the device (float32: its slot words; float64: its
// block partials, which an at-peak injection's wave reduces itself).
int pc_run_direct(rs_pc* h, int n, const int32_t* ox, const int32_t* oy, const int32_t* fidx,
                  const double* zf, int32_t* out_xyz, double* xp, double* sums, const PcInj* inj = nullptr) {
    if (n == 0) return RS_OK;
    // (the halo form's finishing pass exports in front of the injections behind the last step)
    RS_CHECK(!(xp && inj), RS_ERR_STATE, "an eager readback takes no injections");
    if (h->form == PcForm::Halo) return pc_run_halo(h, n, ox, oy, fidx, zf, out_xyz, xp, sums, inj);
    if (sums) RS_TRY(pc_grow_peaks(h, n));
    // Batches: the column form takes each step's control as kernel arguments too (its
    // path kernel then starts its window loads without a global round trip for the
    // shifts: 128x128x72 27.5 -> 27.1 us per step with the filter table staged behind
    // the window); the other forms read the device ring
    const bool inline_ctl = (n == 1 || h->form == PcForm::Cols) && h->TH <= CTL_INLINE_MAX;
    RS_TRY(pc_grow_steps(h, n, !inline_ctl));
    if (!inline_ctl) {
        RS_TRY(pc_pack_ctl(h, n, ox, oy, fidx, zf));
        RS_HIP(hipMemcpyAsync(h->dCtl.get(), h->hCtl.get(), h->ctlStride * n, hipMemcpyHostToDevice,
                              h->stream.get()));
    }
    const bool pk = h->profiling && h->profKernels;
    if (pk) RS_TRY(pc_ensure_events(h, (size_t)4 * n));
    if (h->profiling) RS_HIP(hipEventRecord(h->ev0.get(), h->stream.get()));
    int icur = 0;   // the next injection
    for (int s = 0; s < n; ++s) {
        const int pb = pk ? 4 * s : -1;
        const size_t b = (size_t)s * h->TH;
        if (inj) RS_TRY(pc_inject_point(h, *inj, &icur, s, s > 0 ? step_key(h, step_out(h, s - 1)) : PcKeySrc{}));
        if (inline_ctl) {
            PcCtlInline c;
            make_ctl_inline(h->X, h->Y, h->TH, ox + b, oy + b, fidx + b, zf + (size_t)s * FL, &c);
            RS_TRY(pc_by_prec(h, [&](auto t) { return pc_launch_step<decltype(t), PcCtlInline>(h, step_out(h, s), &c, pb); }));
        } else {
            const PcCtlRing c = make_ctl_ring(h, s);
            RS_TRY(pc_by_prec(h, [&](auto t) { return pc_launch_step<decltype(t), PcCtlRing>(h, step_out(h, s), &c, pb); }));
        }
        // the step's state is in dP and its key on the device (float32: its slot words;
        // float64: its block partials, pc_argmax_steps runs only after the last step) until
        // the next step's launches: the step's peak launch goes here
        if (sums) {
            const StepOut so = step_out(h, s);
            const bool f32 = h->prec == RS_PREC_F32;
            RS_TRY(pc_launch_peak(h, h->dP.get(), f32 ? so.slot : nullptr, so.bmax, so.bidx, h->nPart, s));
        }
    }
    if (inj) RS_TRY(pc_inject_point(h, *inj, &icur, n, step_key(h, step_out(h, n - 1))));
    if (h->prec == RS_PREC_F64) {
        hipLaunchKernelGGL((pc_argmax_steps<double>), dim3(n), dim3(NT), 0, h->stream.get(),
                           static_cast<const double*>(h->dArgV.get()), h->dArgI.get(), h->nPart, h->dRes.get());
        RS_HIP(hipGetLastError());
    }
    for (int s = 0; s < n; ++s) h->hRes.get()[s] = RES_NONE;
    const bool skipped = h->dbgSkipExport;
    if (!h->dbgSkipExport) {
        hipLaunchKernelGGL(pc_res_export, dim3(n < 1024 ? n : 1024), dim3(64), 0,
                           h->stream.get(), h->dRes.get(), n, h->hRes.dev());
        RS_HIP(hipGetLastError());
    }
    h->dbgSkipExport = false;
    // the volume after the last step, into the caller's pinned array (the eager
    // readback), its blocks' flags polled when the call may return early
    // (a peaks call synchronises the stream: the polled words' early return is safe only
    // because the host reads nothing else, and the sums are plain stores of other launches)
    // (nor does a call with injections: their resolved cells are plain stores as well)
    const bool may_poll = halo_poll_env() && !h->profiling && !skipped && n <= HF_POLL_MAX && !sums && !inj;
    int xnb = 0;
    unsigned seq = 0u;
    if (xp) RS_TRY(pc_launch_export(h, xp, may_poll, &xnb, &seq));
    if (h->profiling) RS_HIP(hipEventRecord(h->ev1.get(), h->stream.get()));
    // the result words polled (pc_poll_words), and with an eager readback the volume's
    // flags first (each block's stores released at system scope before its flag), unless
    // the call is profiled, long or its export was withheld (RS_PC_HALO_POLL=0: always the
    // stream synchronisation; RS_PC_HALO_FLAGS=0: for an eager readback)
    const bool polled = may_poll && (xp ? seq != 0u && pc_poll_flags(h, xnb, seq) : true) &&
                        pc_poll_words(h, 0, n);
    if (!polled) RS_HIP(hipStreamSynchronize(h->stream.get()));
    if (sums) std::memcpy(sums, h->hPeak.get(), sizeof(double) * 6 * (size_t)n);
    RS_TRY(pc_end_call(h, n, out_xyz));
    if (pk) {
        h->kernelMs[0] = h->kernelMs[1] = 0.0;
        for (int s = 0; s < n; ++s) {
            float a = 0.f, b = 0.f;
            RS_HIP(hipEventElapsedTime(&a, h->evPool[4 * s].get(), h->evPool[4 * s + 1].get()));
            RS_HIP(hipEventElapsedTime(&b, h->evPool[4 * s + 2].get(), h->evPool[4 * s + 3].get()));
            h->kernelMs[0] += a;
            h->kernelMs[1] += b;
        }
    }
    return RS_OK;
}

// xp: an eager readback, the float64 volume after the last step into the caller's
// pinned array (its device address), queued behind the steps; else null.  sums: a peaks
// call, six sums per step (pc_peak_kernel, queued behind each step) into this host array.
int pc_run_impl(rs_pc* h, int n, const int32_t* ox, const int32_t* oy, const int32_t* fidx,
                const double* zf, int32_t* out_xyz, double* xp = nullptr, double* sums = nullptr) {
    RS_CHECK(h, RS_ERR_STATE, "null pose-cell handle");
    RS_CHECK(n >= 0, RS_ERR_ARG, "negative step count");
    RS_CHECK(!sums || h->peakR > 0, RS_ERR_STATE, "rs_pc_set_peak_tables has not been called");
    if (n == 0) return RS_OK;
    RS_HIP(hipSetDevice(h->device));
    RS_TRY(pc_check_ctl(h, n, ox, oy, fidx, zf));
    return pc_run_direct(h, n, ox, oy, fidx, zf, out_xyz, xp, sums);
}

// A run's injections against the rule of rs_pc_run_odom_inject (pc_inj_first_bad, pc_ctl.h),
// before any device work.
int pc_check_inj(const rs_pc* h, int n, const PcInj& inj, const int32_t* out_inj_xyz) {
    RS_CHECK(inj.ni >= 0, RS_ERR_ARG, "negative injection count");
    if (inj.ni == 0) return RS_OK;
    RS_CHECK(inj.step && inj.energy && inj.loc && out_inj_xyz, RS_ERR_ARG, "null injection array");
    PcInjBad why = PC_INJ_OK;
    const int i = pc_inj_first_bad(h->X, h->Y, h->TH, n, inj.ni, inj.step, inj.loc, &why);
    if (i < 0) return RS_OK;
    const int32_t* loc = inj.loc + 3 * (size_t)i;
    RS_CHECK(why != PC_INJ_BAD_STEP, RS_ERR_ARG, "injection %d: step %d outside [0, %d]", i, inj.step[i], n);
    RS_CHECK(why != PC_INJ_BAD_ORDER, RS_ERR_ARG, "injection %d: step %d after step %d", i, inj.step[i], inj.step[i - 1]);
    RS_CHECK(why != PC_INJ_BAD_SAME, RS_ERR_ARG, "injection %d: same-as %d is no earlier injection", i, loc[1]);
    RS_CHECK(false, RS_ERR_ARG, "injection %d: location (%d, %d, %d) outside grid (%d, %d, %d)", i, loc[0], loc[1], loc[2],
             h->X, h->Y, h->TH);
}

// n steps with the injections of inj (checked) whose step is at most n: a caller that stops
// at a LUT miss passes the steps before it, and the later injections never run.  Every
// injection's resolved cell into out_inj_xyz, (-1, -1, -1) for one that did not run.
int pc_run_inj(rs_pc* h, int n, const int32_t* ox, const int32_t* oy, const int32_t* fidx, const double* zf,
               int32_t* out_xyz, double* sums, const PcInj& inj, int32_t* out_inj_xyz) {
    RS_HIP(hipSetDevice(h->device));
    if (n > 0) RS_TRY(pc_check_ctl(h, n, ox, oy, fidx, zf));
    PcInj run = inj;
    run.ni = 0;
    while (run.ni < inj.ni && inj.step[run.ni] <= n) ++run.ni;
    RS_TRY(pc_grow_inj(h, inj.ni));
    for (int i = 0; i < inj.ni; ++i) h->hInj.get()[i] = PC_INJ_NONE;
    if (n > 0) {
        RS_TRY(pc_run_direct(h, n, ox, oy, fidx, zf, out_xyz, nullptr, sums, run.ni > 0 ? &run : nullptr));
    } else if (run.ni > 0) {   // the injections alone, on the stored state
        int cur = 0;
        RS_TRY(pc_halo_settle(h));
        RS_TRY(pc_inject_point(h, run, &cur, 0, PcKeySrc{}));
        RS_HIP(hipStreamSynchronize(h->stream.get()));
    }
    for (int i = 0; i < inj.ni; ++i) {
        const unsigned lin = h->hInj.get()[i];
        int32_t* o = out_inj_xyz + 3 * (size_t)i;
        if (i < run.ni) {
            RS_CHECK(lin < h->n, RS_ERR_HIP, "injection %d of %d: its cell did not reach the host", i, inj.ni);
            decode_xyz(h, 0xFFFFFFFFull - lin, o);
        } else {
            o[0] = o[1] = o[2] = -1;
        }
    }
    return RS_OK;
}

// path_integration's control for one step (posecell_network.py:252-308) in the
// operation order of filters.step_control: vt = vtrans/0.2, vr = vrot/(2pi/TH),
// e = vt*cos|sin (:257-261), o = around(e) (:262-265, half-even = rint), key =
// int((e_x - o_x)*10) (:246-249), theta origin floor(vr + .5) (:304).  Each is one
// correctly rounded IEEE operation on the same operands as NumPy's, and
// contraction is off, so the result is bit-identical.  Returns RS_ERR_LUT_KEY on
// a key outside the LUT (the reference's KeyError, :249; checked before the theta
// filter, as the reference builds the xy filters first) and RS_ERR_CTL_RANGE when
// the theta origin or a shift lies outside what the tables cover.
constexpr double PC_LUT_PRECISION = 10.0;  // filter_dict_2d_precision, posecell_network.py:48

static inline __attribute__((always_inline)) int pc_odom_control_body(const OdoTables* h, double vtrans, double vrot,
                                                                      int32_t* ox, int32_t* oy, int32_t* rows, double* zf) {
#pragma clang fp contract(off)
    const double vt = vtrans / h->vtScale;
    const double vr = vrot / h->vrScale;
    for (int k = 0; k < h->TH; ++k) {
        const double ex = vt * h->cosA[k];
        const double ey = vt * h->sinA[k];
        const double rx = std::nearbyint(ex);
        const double ry = std::nearbyint(ey);
        const double key = std::trunc((ex - rx) * PC_LUT_PRECISION);
        if (!(key >= h->keyMin && key < h->keyMin + h->nKeys)) return RS_ERR_LUT_KEY;  // NaN too
        if (!(std::fabs(rx) < 1073741824.0 && std::fabs(ry) < 1073741824.0)) return RS_ERR_CTL_RANGE;
        ox[k] = (int32_t)rx;
        oy[k] = (int32_t)ry;
        rows[k] = h->keyRows[(int)key - h->keyMin];
    }
    const double zo = std::floor(vr + 0.5);
    if (!std::isfinite(zo)) {
        // Python 2's math.floor returns a NaN or infinite argument as it is, and the
        // theta filter built on it is all NaN (filters.theta_filter): the reference runs
        // on with a NaN volume (posecell_network.py:304-310)
        for (int t = 0; t < FL; ++t) zf[t] = std::numeric_limits<double>::quiet_NaN();
        return RS_OK;
    }
    if (!(zo >= h->zMin && zo < h->zMin + h->nZ)) return RS_ERR_CTL_RANGE;
    const double* f = h->zfTab + (size_t)((int)zo - h->zMin) * FL;
    for (int t = 0; t < FL; ++t) zf[t] = f[t];
    return RS_OK;
}
// The same operations compiled for SSE4.1 (nearbyint, trunc and floor become roundsd
// with the same IEEE results: 0.80 -> 0.42 us per 72-layer step on the build host), used
// when the CPU has it
__attribute__((target("sse4.1"))) int pc_odom_control_sse41(const OdoTables* h, double vtrans, double vrot,
                                                           int32_t* ox, int32_t* oy, int32_t* rows, double* zf) {
    return pc_odom_control_body(h, vtrans, vrot, ox, oy, rows, zf);
}
int pc_odom_control_base(const OdoTables* h, double vtrans, double vrot, int32_t* ox, int32_t* oy, int32_t* rows,
                         double* zf) {
    return pc_odom_control_body(h, vtrans, vrot, ox, oy, rows, zf);
}
int pc_odom_control(const OdoTables* h, double vtrans, double vrot, int32_t* ox, int32_t* oy, int32_t* rows,
                    double* zf) {
    static const bool sse41 = __builtin_cpu_supports("sse4.1");
    return sse41 ? pc_odom_control_sse41(h, vtrans, vrot, ox, oy, rows, zf)
                 : pc_odom_control_base(h, vtrans, vrot, ox, oy, rows, zf);
}

// The stored state's argmax, queued: its block partials in dBmax / dBidx (*nb of them), the
// key into dRes[0] and from there into hRes[0] once the stream has synchronised.
template <typename T>
int pc_argmax_queue(rs_pc* h, int* nb_out) {
    RS_TRY(pc_launch_argmax_blocks(h, nb_out));
    const int nb = *nb_out;
    hipLaunchKernelGGL((pc_argmax_steps<T>), dim3(1), dim3(NT), 0, h->stream.get(),
                       static_cast<const T*>(h->dBmax.get()), h->dBidx.get(), nb, h->dRes.get());
    RS_HIP(hipGetLastError());
    RS_HIP(hipMemcpyAsync(h->hRes.get(), h->dRes.get(), sizeof(unsigned long long), hipMemcpyDeviceToHost,
                          h->stream.get()));
    return RS_OK;
}

template <typename T>
int pc_argmax_impl(rs_pc* h, int32_t* out) {
    int nb = 0;
    RS_TRY(pc_argmax_queue<T>(h, &nb));
    RS_HIP(hipStreamSynchronize(h->stream.get()));
    decode_xyz(h, h->hRes.get()[0], out);
    return RS_OK;
}

template <typename T>
void fill_sep(SepKernel<T>& k, const rs_pc_params* p) {
    for (int t = 0; t < FL; ++t) {
        k.ge[t] = (T)p->ge[t];
        k.gi[t] = (T)p->gi[t];
    }
    k.scale = (T)p->k_scale;
    k.inhib = (T)p->global_inhibition;
}


// Step-kernel form.  Each form has a fit predicate (its kernels' limits on this grid,
// precision and filter table) and a set function (the form, its geometry and nPart);
// pc_choose_form, below them, takes RS_PC_FORM's request or walks the default order.
// rows: a grid row within the YP = 128 instance; a filter table of any size (read in place).
bool pc_rows_fit(const rs_pc* h) { return h->Y <= 128; }

int pc_rows_set(rs_pc* h) {
    h->form = PcForm::Rows;
    h->rowsYP = h->Y <= 64 ? 64 : 128;
    h->nPart = ((h->X + RT_BX - 1) / RT_BX) * ((h->TH + RT_BK - 1) / RT_BK);
    return RS_OK;
}

// Scratch traffic in the layer loop defeats the streaming kernels' prefetch
// pipeline: pc_stream_set refuses a variant that spills.
template <typename T>
int pc_stream_scratch(int bx, int wr, int wc, size_t* bytes) {
    *bytes = 0;
    return with_stream_variant(bx, wr, wc, [&](auto b, auto r, auto c) -> int {
        constexpr int BX = decltype(b)::value, WR = decltype(r)::value, WC = decltype(c)::value;
        const void* fns[3] = {reinterpret_cast<const void*>(&pc_excite_stream<T, BX, WR, WC>),
                              reinterpret_cast<const void*>(&pc_path_stream<T, BX, WR, WC, PcCtlRing>),
                              reinterpret_cast<const void*>(&pc_path_stream<T, BX, WR, WC, PcCtlInline>)};
        hipFuncAttributes a{};
        for (const void* f : fns) {
            RS_HIP(hipFuncGetAttributes(&a, f));
            *bytes += a.localSizeBytes;
        }
        return RS_OK;
    });
}

// The column kernels' limits: single-conditional wraps, the window in LDS, the
// filter table in LDS.
int pc_cols_vec(const rs_pc* h) {
    return pc_by_prec(h, [](auto t) { return co_vec<decltype(t)>(); });
}
bool pc_cols_fit(const rs_pc* h) {
    const int vec = pc_cols_vec(h);
    return h->X >= CO_TX + 2 * HALF && h->Y >= CO_TY + 2 * HALF + 4 && h->Y % vec == 0 &&
           h->TH >= CO_CH + 2 && h->nf <= RT_NFMAX;
}

// Theta chunking of the column form: kc = 0 picks it.  The whole extent in one
// block per CU when it fits the LDS window (no halo layers); KC < TH puts KC + 6
// layers in each of two blocks per CU.
int pc_cols_set(rs_pc* h, int kc) {
    const int thf = pc_by_prec(h, [](auto t) { return co_thmax<decltype(t)>(); });
    const int thc = pc_by_prec(h, [](auto t) { return co_thmax_chunk<decltype(t)>(); });
    if (kc <= 0) {
        kc = h->TH;
        if (h->TH > thf) {  // more layers than one block holds: the fewest chunks that fit
            const int nch = (h->TH + thc - 2 * HALF - 1) / (thc - 2 * HALF);
            kc = (h->TH + nch - 1) / nch;
        }
    }
    RS_CHECK(kc >= 1 && kc <= h->TH, RS_ERR_ARG, "cols KC=%d outside [1, %d]", kc, h->TH);
    RS_CHECK(kc < h->TH ? kc + 2 * HALF <= thc : h->TH <= thf, RS_ERR_ARG,
             "cols KC=%d: %d window layers exceed the LDS window (%d whole, %d per chunk)", kc,
             kc < h->TH ? kc + 2 * HALF : kc, thf, thc);
    h->form = PcForm::Cols;
    h->cgx = (h->X + CO_TX - 1) / CO_TX;
    h->cgy = (h->Y + CO_TY - 1) / CO_TY;
    h->coKC = kc;
    h->coNch = (h->TH + kc - 1) / kc;
    h->nPart = h->cgx * h->cgy * h->coNch;
    return RS_OK;
}

// The halo form's limits: float32, the instantiated theta extent, the 16 x 16 layer
// windows without self-overlap, the filter table in LDS, 32-bit buffer offsets.
bool pc_halo_fit(const rs_pc* h) {
    // (the union's origin and extent travel as 16-bit fields: make_ctl_halo, hf_pack)
    // (so do the grid, the tile count and the block count of pc_step_halo; tile / gx is a
    // high multiply valid below 2^16, hf_magic)
    return h->esz == 4 && hf_th_ok(h->TH) && h->X >= HF_W && h->Y >= HF_W && h->X <= 32767 && h->Y <= 32767 &&
           (size_t)((h->X + HF_T - 1) / HF_T) * ((h->Y + HF_T - 1) / HF_T) <= 65535 &&
           h->nf <= RT_NFMAX && h->n * sizeof(float) <= (size_t)INT_MAX && h->n % 4 == 0;   // (pc_halo_finish: float4s)
}

int pc_halo_set(rs_pc* h) {
    h->form = PcForm::Halo;
    h->cgx = (h->X + HF_T - 1) / HF_T;
    h->cgy = (h->Y + HF_T - 1) / HF_T;
    h->nPart = h->cgx * h->cgy;
    return RS_OK;
}

// The halo form by default where it fits and its tiles fill at most one block per CU
// (every block holds ~155 KiB of LDS): 64x64x36 9.49 vs 11.23 us per batched step
// against rows, 21x21x36 10.00 vs 11.12 (tools/pc_ab.py, 3 rounds, one box)
constexpr int HF_DEFAULT_MAX_TILES = 256;
bool pc_halo_default(const rs_pc* h) {
    return pc_halo_fit(h) && (size_t)((h->X + HF_T - 1) / HF_T) * ((h->Y + HF_T - 1) / HF_T) <=
                                 (size_t)HF_DEFAULT_MAX_TILES;
}

// The streaming kernels' limit: the filter table staged in LDS.
bool pc_stream_fit(const rs_pc* h) { return h->nf <= RT_NFMAX; }

// The streaming form with tile (bx, wr, wc): one wave per 64 columns, wr row groups of
// bx rows.  kc (layers per block) = 0 picks the smallest chunk that keeps the grid
// within one block per CU.
int pc_stream_set(rs_pc* h, int bx, int wr, int wc, int kc) {
    size_t scratch = 0;   // (a variant that is not instantiated is refused here: with_stream_variant)
    RS_TRY(pc_by_prec(h, [&](auto t) { return pc_stream_scratch<decltype(t)>(bx, wr, wc, &scratch); }));
    RS_CHECK(scratch == 0, RS_ERR_ARG,
             "streaming variant BX=%d WR=%d WC=%d spills %zu B to scratch at this precision", bx, wr,
             wc, scratch);
    const int bxb = bx * wr, yt = 64 * wc;
    StreamGrid g;
    g.gx = (h->X + bxb - 1) / bxb;
    g.gy = (h->Y + yt - 1) / yt;
    const int maxkc = st_maxkc((int)h->esz, bxb, yt);
    if (kc <= 0) {
        // a second block on some CUs doubles their share (fewer, longer blocks also
        // re-evaluate fewer halo layers)
        const int target = 256;
        kc = 2;
        while (kc < maxkc && kc < h->TH && (long)g.gx * g.gy * ((h->TH + kc - 1) / kc) > target) ++kc;
    }
    RS_CHECK(kc >= 1 && kc <= maxkc, RS_ERR_ARG, "stream KC=%d outside [1, %d]", kc, maxkc);
    if (kc > h->TH) kc = h->TH;
    g.KC = kc;
    g.gz = (h->TH + g.KC - 1) / g.KC;
    RS_CHECK((long)g.gx * g.gy * g.gz <= NPP_MAX_BLOCKS, RS_ERR_ARG,
             "streaming grid of %ld blocks exceeds %d", (long)g.gx * g.gy * g.gz, NPP_MAX_BLOCKS);
    h->form = PcForm::Stream;
    h->sbx = bx;
    h->swr = wr;
    h->swc = wc;
    h->sg = g;
    h->nPart = g.gx * g.gy * g.gz;
    return RS_OK;
}

int pc_choose_form(rs_pc* h) {
    const int def_bx = h->esz == 4 ? ST_DEF_BX : 1;
    // 1. RS_PC_FORM=rows|cols[:KC]|halo|stream[:BX,WR,WC[,KC]] (A/B runs, tests): that form,
    // or RS_ERR_ARG where it does not fit
    const char* env = std::getenv("RS_PC_FORM");
    if (env && std::strcmp(env, "halo") == 0) {
        RS_CHECK(pc_halo_fit(h), RS_ERR_ARG,
                 "RS_PC_FORM=halo needs float32, TH 10, 18 or %d, %d <= X, Y <= 32767 and at most %d path filters", HF_TH,
                 HF_W, RT_NFMAX);
        return pc_halo_set(h);
    }
    if (env && std::strcmp(env, "rows") == 0) {
        RS_CHECK(pc_rows_fit(h), RS_ERR_ARG, "RS_PC_FORM=rows needs Y <= 128");
        return pc_rows_set(h);
    }
    if (env && (std::strcmp(env, "cols") == 0 || std::strncmp(env, "cols:", 5) == 0)) {
        RS_CHECK(pc_cols_fit(h), RS_ERR_ARG,
                 "RS_PC_FORM=cols needs X >= %d, Y >= %d and a multiple of %d, TH >= %d and at most %d "
                 "path filters",
                 CO_TX + 2 * HALF, CO_TY + 2 * HALF + 4, pc_cols_vec(h),
                 CO_CH + 2, RT_NFMAX);
        return pc_cols_set(h, env[4] == ':' ? std::atoi(env + 5) : 0);
    }
    if (env && env[0]) {
        int bx = def_bx, wr = ST_DEF_WR, wc = ST_DEF_WC, kc = 0;
        if (std::strncmp(env, "stream:", 7) == 0) {
            const int n = std::sscanf(env + 7, "%d,%d,%d,%d", &bx, &wr, &wc, &kc);
            RS_CHECK(n >= 3, RS_ERR_ARG, "RS_PC_FORM=stream:BX,WR,WC[,KC], got '%s'", env);
        } else {
            RS_CHECK(std::strcmp(env, "stream") == 0, RS_ERR_ARG,
                     "unknown RS_PC_FORM '%s' (rows | cols | halo | stream[:BX,WR,WC[,KC]])", env);
        }
        RS_CHECK(pc_stream_fit(h), RS_ERR_ARG, "stream form stages at most %d path filters, table has %d", RT_NFMAX,
                 h->nf);
        return pc_stream_set(h, bx, wr, wc, kc);
    }
    // 2. the default order
    if (pc_halo_default(h)) return pc_halo_set(h);
    // one pass per kernel (rows) while the whole grid fits in one wave of blocks -- the
    // step is latency-bound there (64x64x36: 17 us rows vs 23 us streamed); streamed once
    // the rows form's 4x theta-halo recompute dominates (128x128x72: 57 us rows vs 41 us
    // streamed)
    const bool big = (size_t)h->X * h->Y * h->TH >= ST_MIN_CELLS;
    if (pc_rows_fit(h) && !big) return pc_rows_set(h);
    // large grids: the column form where it fits (128x128x72: 29.3 us per step vs 38.8 us
    // streamed, tools/pc_sweep.py), else the streamed form
    if (big && pc_cols_fit(h)) return pc_cols_set(h, 0);
    if (pc_stream_fit(h)) return pc_stream_set(h, def_bx, ST_DEF_WR, ST_DEF_WC, 0);
    // a filter table too large to stage in LDS: only the rows kernels read it in place
    RS_CHECK(pc_rows_fit(h), RS_ERR_ARG,
             "a table of %d path filters needs Y <= 128 (grid has Y = %d): the other step kernels stage at "
             "most %d filters",
             h->nf, h->Y, RT_NFMAX);
    return pc_rows_set(h);
}

}  // namespace

// ---------------------------------------------------------------------------
// extern "C" entry points
// ---------------------------------------------------------------------------
extern "C" {

int rs_pc_create(int X, int Y, int TH, const rs_pc_params* p, int device, rs_pc** out) {
    rs::clear_error();
    RS_CHECK(out, RS_ERR_ARG, "null output handle pointer");
    *out = nullptr;
    RS_CHECK(p, RS_ERR_ARG, "null parameters");
    RS_CHECK(X >= HALF && Y >= HALF && TH >= HALF, RS_ERR_ARG,
             "grid (%d, %d, %d): every dimension must be >= %d (3-cell wrap halo, convolution.py:52-81)",
             X, Y, TH, HALF);
    RS_CHECK((size_t)X * Y * TH < 0xFFFFFFFFull, RS_ERR_ARG, "grid too large for 32-bit cell index");
    RS_CHECK(p->precision == RS_PREC_F32 || p->precision == RS_PREC_F64, RS_ERR_ARG,
             "precision must be RS_PREC_F32 or RS_PREC_F64");
    RS_CHECK(p->nfilters >= 1 && p->xy_filters, RS_ERR_ARG, "empty path-integration filter table");
    RS_TRY(rs::use_device(device));

    // one failure exit: rs_pc_destroy takes a handle at any stage
    std::unique_ptr<rs_pc, int (*)(rs_pc*)> owner(new rs_pc(), rs_pc_destroy);
    rs_pc* const h = owner.get();
    h->X = X; h->Y = Y; h->TH = TH; h->prec = p->precision; h->device = device;
    h->n = (size_t)X * Y * TH;
    h->esz = p->precision == RS_PREC_F32 ? 4 : 8;
    h->nf = p->nfilters;
    fill_sep(h->kf, p);
    fill_sep(h->kd, p);
    h->ctlStride = rs::round_up(ctl_off_zf(h) + sizeof(double) * 8, 16);
    RS_TRY(pc_choose_form(h));
    h->nBmaxCap = h->nPart > 1024 ? h->nPart : 1024;

    // everything the handle allocates
    RS_TRY(h->stream.create());
    RS_TRY(h->dP.reserve(h->n * h->esz));
    RS_TRY(h->dQ.reserve(h->n * h->esz));
    RS_HIP(hipMemsetAsync(h->dP.get(), 0, h->n * h->esz, h->stream.get()));  // zeros(shape), :27
    // Q and the partials are rewritten in full by every excitation before a path
    // kernel reads them; zeroed anyway so that no launch can see a freed handle's data
    // (rs_pc_debug(RS_PC_DBG_POISON) + tests/test_posecell_gpu.py check the former)
    RS_HIP(hipMemsetAsync(h->dQ.get(), 0, h->n * h->esz, h->stream.get()));
    // (the halo form keeps two steps' partial sums: the one it reads, the one it writes)
    RS_TRY(h->dPart.reserve((size_t)h->nPart * 2));
    RS_HIP(hipMemsetAsync(h->dPart.get(), 0, sizeof(double) * h->nPart * 2, h->stream.get()));
    RS_TRY(h->dRec.reserve(2 * (size_t)h->nPart));
    // the volume-writing kernels' per-block flags (pc_halo_finish, pc_export2_kernel)
    RS_TRY(h->hFlag.reserve(HF_FLAGS, PC_FINE));
    std::memset(h->hFlag.get(), 0, sizeof(unsigned) * HF_FLAGS);
    if (h->form == PcForm::Halo) {
        RS_TRY(h->hRec.reserve(2 * (size_t)h->nPart, PC_FINE));
        RS_TRY(h->hKey.reserve(HF_FLAGS, PC_FINE));
    }
    RS_TRY(h->dBmax.reserve(h->esz * h->nBmaxCap));
    RS_TRY(h->dBidx.reserve((size_t)h->nBmaxCap));
    RS_TRY(h->dTmp.reserve(h->n));
    RS_TRY(h->dScalar.reserve(1));
    RS_TRY(h->dFilt.reserve(h->esz * FT * h->nf));
    if (h->prec == RS_PREC_F32) {
        std::vector<float> f(FT * (size_t)h->nf);
        for (size_t i = 0; i < f.size(); ++i) f[i] = (float)p->xy_filters[i];
        RS_HIP(hipMemcpy(h->dFilt.get(), f.data(), f.size() * sizeof(float), hipMemcpyHostToDevice));
    } else {
        RS_HIP(hipMemcpy(h->dFilt.get(), p->xy_filters, FT * (size_t)h->nf * sizeof(double),
                         hipMemcpyHostToDevice));
    }
    RS_TRY(h->ev0.create());
    RS_TRY(h->ev1.create());
    RS_TRY(pc_grow_steps(h, 16));
    RS_HIP(hipStreamSynchronize(h->stream.get()));
    *out = owner.release();
    return RS_OK;
}

int rs_pc_destroy(rs_pc* h) {
    if (!h) return RS_OK;
    (void)hipSetDevice(h->device);
    // the handle's last queued work: a fault or launch error the early-returning calls
    // left on the stream is reported here instead of being dropped
    const hipError_t se = rs::sync_streams({h->stream.get()});
    delete h;  // (the streams and events, then the buffers, go with their members)
    RS_CHECK(se == hipSuccess, RS_ERR_HIP, "work queued before rs_pc_destroy failed: %s", hipGetErrorString(se));
    return RS_OK;
}

int rs_pc_shape(const rs_pc* h, int* X, int* Y, int* TH) {
    RS_CHECK(h, RS_ERR_STATE, "null pose-cell handle");
    if (X) *X = h->X;
    if (Y) *Y = h->Y;
    if (TH) *TH = h->TH;
    return RS_OK;
}

int rs_pc_update(rs_pc* h, const int32_t* ox, const int32_t* oy, const int32_t* fidx,
                 const double* zf, int32_t out_xyz[3]) {
    rs::clear_error();
    return pc_run_impl(h, 1, ox, oy, fidx, zf, out_xyz);
}

int rs_pc_run(rs_pc* h, int n, const int32_t* ox, const int32_t* oy, const int32_t* fidx,
              const double* zf, int32_t* out_xyz) {
    rs::clear_error();
    return pc_run_impl(h, n, ox, oy, fidx, zf, out_xyz);
}

int rs_pc_excite(rs_pc* h) {
    rs::clear_error();
    RS_CHECK(h, RS_ERR_STATE, "null pose-cell handle");
    RS_HIP(hipSetDevice(h->device));
    RS_TRY(pc_halo_settle(h));  // (halo: a state a call left unnormalised)
    if (h->form == PcForm::Halo) {
        // the halo kernel's excitation-only instance: no shifts, Q of the own cells
        PcCtlHalo c{};
        c.uw = (short)HF_W;
        c.uh = (short)HF_W;
        RS_TRY(pc_launch_halo_step<true>(h, static_cast<const float*>(h->dP.get()), static_cast<float*>(h->dQ.get()),
                                         h->dPart.get(), 0, h->dPart.get(), nullptr, nullptr, c, nullptr));
    } else {
        RS_TRY(pc_by_prec(h, [&](auto t) {
            return pc_launch_step<decltype(t), PcCtlRing>(h, step_out(h, 0), nullptr, -1);
        }));
    }
    pc_by_prec(h, [&](auto t) {
        using T = decltype(t);
        hipLaunchKernelGGL((pc_scale_kernel<T>), dim3(64), dim3(NT), 0, h->stream.get(), static_cast<T*>(h->dQ.get()),
                           h->n, h->dPart.get(), h->nPart);
    });
    RS_HIP(hipGetLastError());
    // Q has P's layout in every form (the column form: both theta-fastest)
    RS_HIP(hipMemcpyAsync(h->dP.get(), h->dQ.get(), h->n * h->esz, hipMemcpyDeviceToDevice, h->stream.get()));
    RS_HIP(hipStreamSynchronize(h->stream.get()));
    return RS_OK;
}

int rs_pc_set_odometry_tables(rs_pc* h, double vtrans_scale, double vrot_scale,
                              const double* cos_a, const double* sin_a, int key_min,
                              int nkeys, const int32_t* key_rows, int zorig_min, int nz,
                              const double* zf_table) {
    rs::clear_error();
    RS_CHECK(h, RS_ERR_STATE, "null pose-cell handle");
    RS_CHECK(cos_a && sin_a && key_rows && zf_table, RS_ERR_ARG, "null table");
    RS_CHECK(nkeys > 0 && nz > 0, RS_ERR_ARG, "empty key or theta-filter table");
    RS_CHECK(vtrans_scale != 0.0 && vrot_scale != 0.0, RS_ERR_ARG, "zero odometry scale");
    for (int i = 0; i < nkeys; ++i)
        RS_CHECK(key_rows[i] >= 0 && key_rows[i] < h->nf, RS_ERR_ARG,
                 "key row %d outside the %d-filter table", key_rows[i], h->nf);
    OdoTables& o = h->odo;   // (the handle keeps its own copies)
    o.own.assign(cos_a, cos_a + h->TH);
    o.own.insert(o.own.end(), sin_a, sin_a + h->TH);
    o.own.insert(o.own.end(), zf_table, zf_table + (size_t)nz * FL);
    o.ownRows.assign(key_rows, key_rows + nkeys);
    fill_odo(o, h->TH, vtrans_scale, vrot_scale, o.own.data(), o.own.data() + h->TH, key_min, nkeys,
             o.ownRows.data(), zorig_min, nz, o.own.data() + 2 * (size_t)h->TH);
    h->odoReady = true;
    return RS_OK;
}

int rs_pc_odom_control(int TH, double vtrans_scale, double vrot_scale, const double* cos_a,
                       const double* sin_a, int key_min, int nkeys, const int32_t* key_rows,
                       int zorig_min, int nz, const double* zf_table, int n, const double* odom,
                       int32_t* ox, int32_t* oy, int32_t* fidx, double* zf, int32_t* status) {
    rs::clear_error();
    RS_CHECK(TH > 0 && n >= 0 && nkeys > 0 && nz > 0, RS_ERR_ARG, "bad table or batch size");
    RS_CHECK(cos_a && sin_a && key_rows && zf_table && (n == 0 || (odom && ox && oy && fidx && zf &&
             status)), RS_ERR_ARG, "null argument");
    OdoTables o;
    fill_odo(o, TH, vtrans_scale, vrot_scale, cos_a, sin_a, key_min, nkeys, key_rows, zorig_min, nz, zf_table);
    for (int s = 0; s < n; ++s)
        status[s] = pc_odom_control(&o, odom[2 * s], odom[2 * s + 1], ox + (size_t)TH * s,
                                    oy + (size_t)TH * s, fidx + (size_t)TH * s, zf + (size_t)FL * s);
    return RS_OK;
}

// One step from an odometry sample; xp: the volume after it into a pinned array; sums: the
// step's six peak sums (pc_run_impl).
static int pc_update_odom(rs_pc* h, double vtrans, double vrot, int32_t out_xyz[3], double* xp,
                          double* sums = nullptr) {
    rs::clear_error();
    RS_CHECK(h, RS_ERR_STATE, "null pose-cell handle");
    RS_CHECK(h->odoReady, RS_ERR_STATE, "rs_pc_set_odometry_tables has not been called");
    RS_CHECK(!sums || h->peakR > 0, RS_ERR_STATE, "rs_pc_set_peak_tables has not been called");
    h->cOx.resize(h->TH);
    h->cOy.resize(h->TH);
    h->cRows.resize(h->TH);
    h->cZf.resize(FL);
    const int st = pc_odom_control(&h->odo, vtrans, vrot, h->cOx.data(), h->cOy.data(),
                                   h->cRows.data(), h->cZf.data());
    if (st == RS_ERR_LUT_KEY) {
        // the reference raises inside path_integration, after steps 1-4 ran
        RS_TRY(rs_pc_excite(h));
        RS_CHECK(false, RS_ERR_LUT_KEY, "path-integration LUT key outside the table "
                 "(posecell_network.py:249)");
    }
    RS_CHECK(st == RS_OK, st, "odometry (%g, %g) outside the control tables", vtrans, vrot);
    return pc_run_impl(h, 1, h->cOx.data(), h->cOy.data(), h->cRows.data(), h->cZf.data(), out_xyz, xp, sums);
}

int rs_pc_update_odom(rs_pc* h, double vtrans, double vrot, int32_t out_xyz[3]) {
    return pc_update_odom(h, vtrans, vrot, out_xyz, nullptr);
}

int rs_pc_update_odom_read(rs_pc* h, double vtrans, double vrot, int32_t out_xyz[3], double* pinned) {
    rs::clear_error();
    RS_CHECK(h && pinned, RS_ERR_ARG, "null argument");
    RS_CHECK(reinterpret_cast<uintptr_t>(pinned) % 16 == 0, RS_ERR_ARG, "pinned buffer not 16-byte aligned");
    RS_HIP(hipSetDevice(h->device));
    double* xp = nullptr;   // the state export queued behind the step
    RS_HIP(hipHostGetDevicePointer(reinterpret_cast<void**>(&xp), pinned, 0));
    return pc_update_odom(h, vtrans, vrot, out_xyz, xp);
}

// A batch of steps from odometry samples; sums: six peak sums per step (pc_run_impl).
static int pc_run_odom(rs_pc* h, int n, const double* odom, int32_t* out_xyz, int* first_bad, double* sums,
                       const PcInj* inj = nullptr, int32_t* out_inj_xyz = nullptr) {
    rs::clear_error();
    RS_CHECK(h, RS_ERR_STATE, "null pose-cell handle");
    RS_CHECK(h->odoReady, RS_ERR_STATE, "rs_pc_set_odometry_tables has not been called");
    RS_CHECK(!sums || h->peakR > 0, RS_ERR_STATE, "rs_pc_set_peak_tables has not been called");
    RS_CHECK(n >= 0 && (odom || n == 0), RS_ERR_ARG, "bad odometry batch");
    if (inj) RS_TRY(pc_check_inj(h, n, *inj, out_inj_xyz));
    if (first_bad) *first_bad = -1;
    const size_t th = h->TH;
    h->cOx.resize(th * (n > 0 ? n : 1));
    h->cOy.resize(th * (n > 0 ? n : 1));
    h->cRows.resize(th * (n > 0 ? n : 1));
    h->cZf.resize((size_t)FL * (n > 0 ? n : 1));
    // The batch's control is formed before its first launch (the step kernels take it as
    // kernel arguments), so a long batch forms it on a few threads, each a contiguous range
    // of steps: 10,000 steps at 128x128x72 spent about 6 ms on one (0.6 us per step of the
    // 15 us step, added to the batch's wall time).  The first failing step decides, as in
    // order on one thread.
    int fail = n, fail_st = RS_OK;
    auto range = [&](int s0, int s1, int* fs, int* fst) {
        for (int s = s0; s < s1; ++s) {
            const int st = pc_odom_control(&h->odo, odom[2 * s], odom[2 * s + 1], h->cOx.data() + th * s,
                                           h->cOy.data() + th * s, h->cRows.data() + th * s,
                                           h->cZf.data() + (size_t)FL * s);
            if (st != RS_OK) {
                *fs = s;
                *fst = st;
                return;
            }
        }
    };
    const int nthr = n >= 1024 ? std::min(8, n / 512) : 1;
    if (nthr > 1) {
        std::vector<int> fs(nthr, n), fst(nthr, RS_OK);
        std::vector<std::thread> pool;
        const int per = (n + nthr - 1) / nthr;
        for (int t = 1; t < nthr; ++t) {
            try {
                pool.emplace_back(range, std::min(n, t * per), std::min(n, (t + 1) * per), &fs[t], &fst[t]);
            } catch (...) {   // no thread to be had: this one takes the range
                range(std::min(n, t * per), std::min(n, (t + 1) * per), &fs[t], &fst[t]);
            }
        }
        range(0, std::min(n, per), &fs[0], &fst[0]);
        for (auto& th_ : pool) th_.join();
        for (int t = 0; t < nthr; ++t)
            if (fs[t] < fail) {
                fail = fs[t];
                fail_st = fst[t];
            }
    } else {
        range(0, n, &fail, &fail_st);
    }
    int todo = n;
    if (fail < n) {
        if (fail_st == RS_ERR_LUT_KEY) todo = fail;
        else RS_CHECK(false, fail_st, "odometry of step %d outside the control tables", fail);
    }
    if (inj && inj->ni > 0)
        RS_TRY(pc_run_inj(h, todo, h->cOx.data(), h->cOy.data(), h->cRows.data(), h->cZf.data(), out_xyz, sums, *inj,
                          out_inj_xyz));
    else
        RS_TRY(pc_run_impl(h, todo, h->cOx.data(), h->cOy.data(), h->cRows.data(), h->cZf.data(),
                           out_xyz, nullptr, sums));
    if (todo < n) {
        RS_TRY(rs_pc_excite(h));
        if (first_bad) *first_bad = todo;
        RS_CHECK(false, RS_ERR_LUT_KEY, "path-integration LUT key outside the table at step %d "
                 "(posecell_network.py:249)", todo);
    }
    return RS_OK;
}

int rs_pc_run_odom(rs_pc* h, int n, const double* odom, int32_t* out_xyz, int* first_bad) {
    return pc_run_odom(h, n, odom, out_xyz, first_bad, nullptr);
}

int rs_pc_set_peak_tables(rs_pc* h, int r, const double* sc_x, const double* sc_y, const double* sc_th) {
    rs::clear_error();
    RS_CHECK(h, RS_ERR_STATE, "null pose-cell handle");
    RS_CHECK(sc_x && sc_y && sc_th, RS_ERR_ARG, "null table");
    RS_CHECK(r >= 1 && r <= rs::PC_PEAK_RMAX, RS_ERR_ARG, "peak radius %d outside 1 .. %d", r, rs::PC_PEAK_RMAX);
    RS_CHECK(rs::pc_peak_fits(h->X, h->Y, h->TH, r), RS_ERR_ARG,
             "grid (%d, %d, %d) does not hold a box of %d cells along every axis", h->X, h->Y, h->TH, 2 * r + 1);
    RS_HIP(hipSetDevice(h->device));
    const size_t nx = 2 * (size_t)h->X, ny = 2 * (size_t)h->Y, nth = 2 * (size_t)h->TH;
    std::vector<double> tab(sc_x, sc_x + nx);
    tab.insert(tab.end(), sc_y, sc_y + ny);
    tab.insert(tab.end(), sc_th, sc_th + nth);
    h->peakR = 0;
    RS_TRY(h->dPeakTab.reserve(tab.size()));
    // (ordered behind any peak launch still queued on the handle's stream)
    RS_HIP(hipMemcpyAsync(h->dPeakTab.get(), tab.data(), sizeof(double) * tab.size(), hipMemcpyHostToDevice, h->stream.get()));
    RS_HIP(hipStreamSynchronize(h->stream.get()));
    h->peakR = r;
    return RS_OK;
}

int rs_pc_get_peak(rs_pc* h, int32_t xyz[3], double sums[6]) {
    rs::clear_error();
    RS_CHECK(h && xyz && sums, RS_ERR_ARG, "null argument");
    RS_CHECK(h->peakR > 0, RS_ERR_STATE, "rs_pc_set_peak_tables has not been called");
    RS_HIP(hipSetDevice(h->device));
    RS_TRY(pc_halo_settle(h));  // (halo: a state a call left unnormalised)
    RS_TRY(pc_grow_peaks(h, 1));
    int nb = 0;
    RS_TRY(pc_by_prec(h, [&](auto t) { return pc_argmax_queue<decltype(t)>(h, &nb); }));
    RS_TRY(pc_launch_peak(h, h->dP.get(), nullptr, h->dBmax.get(), h->dBidx.get(), nb, 0));
    // the stream's completion, not a polled word: the sums are plain stores (pc_run_direct)
    RS_HIP(hipStreamSynchronize(h->stream.get()));
    decode_xyz(h, h->hRes.get()[0], xyz);
    std::memcpy(sums, h->hPeak.get(), sizeof(double) * 6);
    return RS_OK;
}

int rs_pc_update_odom_peak(rs_pc* h, double vtrans, double vrot, int32_t out_xyz[3], double sums[6]) {
    rs::clear_error();
    RS_CHECK(sums, RS_ERR_ARG, "null sums");
    return pc_update_odom(h, vtrans, vrot, out_xyz, nullptr, sums);
}

int rs_pc_run_odom_peaks(rs_pc* h, int n, const double* odom, int32_t* out_xyz, double* out_sums, int* first_bad) {
    rs::clear_error();
    RS_CHECK(out_sums || n <= 0, RS_ERR_ARG, "null sums");
    return pc_run_odom(h, n, odom, out_xyz, first_bad, out_sums);
}

int rs_pc_run_peaks(rs_pc* h, int n, const int32_t* ox, const int32_t* oy, const int32_t* fidx, const double* zf,
                    int32_t* out_xyz, double* out_sums) {
    rs::clear_error();
    RS_CHECK(out_sums || n <= 0, RS_ERR_ARG, "null sums");
    return pc_run_impl(h, n, ox, oy, fidx, zf, out_xyz, nullptr, out_sums);
}

int rs_pc_run_odom_inject(rs_pc* h, int n, const double* odom, int ni, const int32_t* inj_step,
                          const double* inj_energy, const int32_t* inj_loc, int32_t* out_xyz, int32_t* out_inj_xyz,
                          double* out_sums, int* first_bad) {
    const PcInj inj{ni, inj_step, inj_energy, inj_loc};
    return pc_run_odom(h, n, odom, out_xyz, first_bad, out_sums, &inj, out_inj_xyz);
}

int rs_pc_run_inject(rs_pc* h, int n, const int32_t* ox, const int32_t* oy, const int32_t* fidx, const double* zf,
                     int ni, const int32_t* inj_step, const double* inj_energy, const int32_t* inj_loc,
                     int32_t* out_xyz, int32_t* out_inj_xyz, double* out_sums) {
    rs::clear_error();
    RS_CHECK(h, RS_ERR_STATE, "null pose-cell handle");
    RS_CHECK(n >= 0, RS_ERR_ARG, "negative step count");
    RS_CHECK(!out_sums || h->peakR > 0, RS_ERR_STATE, "rs_pc_set_peak_tables has not been called");
    const PcInj inj{ni, inj_step, inj_energy, inj_loc};
    RS_TRY(pc_check_inj(h, n, inj, out_inj_xyz));
    if (ni == 0) return pc_run_impl(h, n, ox, oy, fidx, zf, out_xyz, nullptr, out_sums);
    return pc_run_inj(h, n, ox, oy, fidx, zf, out_xyz, out_sums, inj, out_inj_xyz);
}

int rs_pc_peak_host(int X, int Y, int TH, int r, const double* volume, const int32_t xyz[3], const double* sc_x,
                    const double* sc_y, const double* sc_th, double sums[6]) {
    rs::clear_error();
    RS_CHECK(volume && xyz && sums, RS_ERR_ARG, "null argument");
    RS_CHECK(sc_x && sc_y && sc_th, RS_ERR_ARG, "null table");
    RS_CHECK(r >= 1 && r <= rs::PC_PEAK_RMAX, RS_ERR_ARG, "peak radius %d outside 1 .. %d", r, rs::PC_PEAK_RMAX);
    RS_CHECK(X > 0 && Y > 0 && TH > 0 && rs::pc_peak_fits(X, Y, TH, r), RS_ERR_ARG,
             "grid (%d, %d, %d) does not hold a box of %d cells along every axis", X, Y, TH, 2 * r + 1);
    RS_CHECK(rs::pc_peak_host(X, Y, TH, r, volume, xyz, sc_x, sc_y, sc_th, sums), RS_ERR_ARG,
             "cell (%d, %d, %d) outside grid (%d, %d, %d)", xyz[0], xyz[1], xyz[2], X, Y, TH);
    return RS_OK;
}

int rs_pc_inject(rs_pc* h, double energy, int x, int y, int th) {
    rs::clear_error();
    RS_CHECK(h, RS_ERR_STATE, "null pose-cell handle");
    RS_CHECK(x >= 0 && x < h->X && y >= 0 && y < h->Y && th >= 0 && th < h->TH, RS_ERR_ARG,
             "inject location (%d, %d, %d) outside grid (%d, %d, %d)", x, y, th, h->X, h->Y, h->TH);
    RS_HIP(hipSetDevice(h->device));
    RS_TRY(pc_halo_settle(h));  // (halo: a state a call left unnormalised)
    // the column form keeps P theta-fastest (C order); the others layer-major
    const size_t idx = pc_thfast(h) ? ((size_t)x * h->Y + y) * h->TH + th : ((size_t)th * h->X + x) * h->Y + y;
    pc_by_prec(h, [&](auto t) {
        using T = decltype(t);
        hipLaunchKernelGGL((pc_inject_kernel<T>), dim3(1), dim3(64), 0, h->stream.get(), static_cast<T*>(h->dP.get()), idx,
                           energy);
    });
    RS_HIP(hipGetLastError());
    // no host sync: the add is ordered on the handle's stream before the next step,
    // read or argmax (template -> pose-cell feedback costs one queued launch)
    return RS_OK;
}

int rs_pc_get_max(rs_pc* h, int32_t out_xyz[3]) {
    rs::clear_error();
    RS_CHECK(h && out_xyz, RS_ERR_ARG, "null argument");
    RS_HIP(hipSetDevice(h->device));
    RS_TRY(pc_halo_settle(h));  // (halo: a state a call left unnormalised)
    return pc_by_prec(h, [&](auto t) { return pc_argmax_impl<decltype(t)>(h, out_xyz); });
}

// The float64 C-order volume into pinned host memory (dst: its device pointer) and the
// host back once it has landed: a pending halo state settled in the same pass
// (pc_halo_settle_read), else the export kernel; either way the writing kernel's
// blocks' flags are polled (pc_poll_flags) where allowed, else the stream synchronised.
int pc_read_volume(rs_pc* h, double* dst) {
    bool done = false;
    RS_TRY(pc_halo_settle_read(h, dst, &done));
    if (done) return RS_OK;
    int nb = 0;
    unsigned seq = 0u;
    RS_TRY(pc_launch_export(h, dst, true, &nb, &seq));
    if (!(seq != 0u && pc_poll_flags(h, nb, seq))) RS_HIP(hipStreamSynchronize(h->stream.get()));
    return RS_OK;
}

int rs_pc_read(rs_pc* h, double* host) {
    rs::clear_error();
    RS_CHECK(h && host, RS_ERR_ARG, "null argument");
    RS_HIP(hipSetDevice(h->device));
    // The export kernel writes the float64 C-order volume straight into pinned host
    // memory (one launch, no copy engine), then the host copies it into the caller's
    // array.
    RS_TRY(h->hRead.reserve(h->n, PC_FINE));
    RS_TRY(pc_read_volume(h, h->hRead.dev()));
    std::memcpy(host, h->hRead.get(), sizeof(double) * h->n);
    return RS_OK;
}

int rs_pc_read_pinned(rs_pc* h, double* pinned) {
    rs::clear_error();
    RS_CHECK(h && pinned, RS_ERR_ARG, "null argument");
    RS_CHECK(reinterpret_cast<uintptr_t>(pinned) % 16 == 0, RS_ERR_ARG, "pinned buffer not 16-byte aligned");
    RS_HIP(hipSetDevice(h->device));
    double* dst = nullptr;
    RS_HIP(hipHostGetDevicePointer(reinterpret_cast<void**>(&dst), pinned, 0));
    return pc_read_volume(h, dst);
}

int rs_pc_write(rs_pc* h, const double* host) {
    rs::clear_error();
    RS_CHECK(h && host, RS_ERR_ARG, "null argument");
    RS_HIP(hipSetDevice(h->device));
    h->haloPend = false;  // (halo: the whole state is replaced)
    h->haloCur = 0;
    RS_HIP(hipMemcpyAsync(h->dTmp.get(), host, sizeof(double) * h->n, hipMemcpyHostToDevice, h->stream.get()));
    pc_by_prec(h, [&](auto t) {
        using T = decltype(t);
        hipLaunchKernelGGL((pc_import_kernel<T>), dim3(256), dim3(NT), 0, h->stream.get(), h->dTmp.get(),
                           static_cast<T*>(h->dP.get()), h->X, h->Y, h->TH, (int)pc_thfast(h));
    });
    RS_HIP(hipGetLastError());
    RS_HIP(hipStreamSynchronize(h->stream.get()));
    return RS_OK;
}

int rs_pc_total(rs_pc* h, double* total) {
    rs::clear_error();
    RS_CHECK(h && total, RS_ERR_ARG, "null argument");
    RS_HIP(hipSetDevice(h->device));
    RS_TRY(pc_halo_settle(h));  // (halo: a state a call left unnormalised)
    pc_by_prec(h, [&](auto t) {
        using T = decltype(t);
        hipLaunchKernelGGL((pc_total_kernel<T>), dim3(1), dim3(NT), 0, h->stream.get(), static_cast<const T*>(h->dP.get()),
                           h->n, h->dScalar.get());
    });
    RS_HIP(hipGetLastError());
    RS_HIP(hipMemcpyAsync(total, h->dScalar.get(), sizeof(double), hipMemcpyDeviceToHost, h->stream.get()));
    RS_HIP(hipStreamSynchronize(h->stream.get()));
    return RS_OK;
}

int rs_pc_last_ms(rs_pc* h, double* ms) {
    RS_CHECK(h && ms, RS_ERR_ARG, "null argument");
    *ms = h->lastMs;
    return RS_OK;
}

int rs_pc_set_profiling(rs_pc* h, int enable) {
    RS_CHECK(h, RS_ERR_STATE, "null pose-cell handle");
    // 1: events around every launch too (kernel_ms); 2: around the whole call only
    h->profiling = enable != 0;
    h->profKernels = enable == 1;
    return RS_OK;
}

int rs_pc_kernel_ms(rs_pc* h, double ms[2]) {
    RS_CHECK(h && ms, RS_ERR_ARG, "null argument");
    ms[0] = h->kernelMs[0];
    ms[1] = h->kernelMs[1];
    return RS_OK;
}

const char* rs_pc_step_form(const rs_pc* h) {
    if (!h) return nullptr;
    switch (h->form) {
    case PcForm::Rows: return "rows";
    case PcForm::Stream: return "stream";
    case PcForm::Cols: return "cols";
    case PcForm::Halo: return "halo";
    }
    return nullptr;
}

int rs_pc_debug(rs_pc* h, int op) {
    rs::clear_error();
    RS_CHECK(h, RS_ERR_STATE, "null pose-cell handle");
    RS_HIP(hipSetDevice(h->device));
    RS_TRY(pc_halo_settle(h));  // (halo: a state a call left unnormalised)
    if (op == RS_PC_DBG_POISON) {
        // every buffer a step writes before it reads: all bits set (NaN volumes, the
        // largest possible argmax key in every slot of every step)
        RS_HIP(hipMemsetAsync(h->dQ.get(), 0xFF, h->n * h->esz, h->stream.get()));
        RS_HIP(hipMemsetAsync(h->dPart.get(), 0xFF, sizeof(double) * h->nPart * 2, h->stream.get()));
        RS_HIP(hipMemsetAsync(h->dRes.get(), 0xFF, sizeof(unsigned long long) * RES_SLOTS * h->resCap, h->stream.get()));
        RS_HIP(hipMemsetAsync(h->dBmax.get(), 0xFF, h->esz * h->nBmaxCap, h->stream.get()));
        RS_HIP(hipMemsetAsync(h->dBidx.get(), 0xFF, sizeof(unsigned) * h->nBmaxCap, h->stream.get()));
        if (h->dArgV.get()) RS_HIP(hipMemsetAsync(h->dArgV.get(), 0xFF, h->esz * (size_t)h->resCap * h->nPart, h->stream.get()));
        if (h->dArgI.get())
            RS_HIP(hipMemsetAsync(h->dArgI.get(), 0xFF, sizeof(unsigned) * (size_t)h->resCap * h->nPart, h->stream.get()));
        for (int s = 0; s < h->resCap; ++s) h->hRes.get()[s] = ~0ull;
        RS_HIP(hipStreamSynchronize(h->stream.get()));
        return RS_OK;
    }
    if (op == RS_PC_DBG_SKIP_EXPORT) {
        h->dbgSkipExport = true;
        return RS_OK;
    }
    if (op == RS_PC_DBG_HALO_SETTLE) {
        h->haloSettleAlways = true;
        return RS_OK;
    }

    RS_CHECK(false, RS_ERR_ARG, "unknown rs_pc_debug op %d", op);
}

int rs_pc_debug_value(rs_pc* h, int op, int64_t* value) {
    rs::clear_error();
    RS_CHECK(h && value, RS_ERR_ARG, "null argument");
    RS_CHECK(op == RS_PC_DBG_HALO_AMBIG, RS_ERR_ARG, "unknown rs_pc_debug_value op %d", op);
    *value = h->haloAmbig;
    return RS_OK;
}

}  // extern "C"
