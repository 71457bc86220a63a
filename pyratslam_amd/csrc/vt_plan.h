// What the view-template matcher's host side decides before it launches: which scan, how
// many blocks, which path through rs_vt_match_stream, how its host batches are grouped.
// Pure functions of integers and booleans, shared by view_templates.hip and by
// tests/vt_plan_main.cpp (built with the plain host compiler: no HIP include here).  The
// kernels' own constants (queries per staged batch, template blocks per thread block, the
// grid cap) come in as arguments.
#pragma once

#include <algorithm>
#include <cstdint>

namespace vt_plan {

// Templates of a library of global_count that live on `rank` of nranks (template g on rank g % nranks).
inline int64_t local_count_of(int rank, int nranks, int64_t global_count) {
    if (global_count <= rank) return 0;
    return (global_count - rank + nranks - 1) / nranks;
}

// Blocks per template block (nqc) for the plane scan.  A block's fixed cost
// (its template planes, 128 KiB, into VGPRs) is small next to its query batches,
// and the nqc blocks of a template block balance their batches dynamically, so
// finer splits fill the last round of resident blocks better; measured on
// MI355X (tools/scan_split.py, 1,024 queries): nqc = 32 is within 2% of the best
// split from 12.5k to 100k templates (100k: 18.6 ms at nqc = 1, the previous
// choice there, vs 15.0 ms), and small libraries gain from up to 4 rounds of
// blocks (1k: 128 -> 0.183 ms vs 0.199 ms at 32).  nqc >= 8 is a multiple of 8
// (the XCD query groups).  nqc_override > 0 (RS_VT_NQC, A/B) replaces the model.
inline int plane_split(int ntb, int nbatch, int slots, int nqc_override) {
    int nqc = nqc_override;
    if (nqc_override <= 0) {
        const int fill = (slots + ntb - 1) / ntb;  // blocks per template block for one round
        nqc = std::max(32, std::min(4 * fill, std::max(128, fill)));
    }
    nqc = std::min(nqc, std::max(1, nbatch));
    if (nqc >= 8) nqc &= ~7;
    return nqc;
}

// --- How the thread blocks of one template block share its query batches (the plane scan's
// kernel and tests/list_take_main.cpp run this one definition).
// The blocks serving a template block are numbered l = 0 .. nblk-1.  With nblk >= 8 (a
// multiple of 8) the batches are dealt to G = 8 groups (batch B belongs to group B % 8, one
// group per XCD) and block l serves group l & 7; otherwise G = 1.  Each group has its own
// counter.  Within a group, the k-th of its blocks (k = l >> 3, or l with G = 1) owns the
// group's batch k statically: it needs no atomic to learn its first batch.  The group's
// batches from nstat = nblk / G upwards are handed out by the counter: take t is batch
// nstat + t.  A block keeps taking until its first failed take (a batch index >= nbatch).
// Only blocks that own a static batch take, and only if the group has dynamic batches at
// all, so with ndyn > 0 exactly nact = nstat blocks end on one failed take each, the failed
// takes return ndyn .. ndyn + nact - 1, and the block that sees the largest is the
// counter's last user in the launch: it stores zero for the next launch.
#if defined(__HIPCC__)
#define VT_PLAN_HD __host__ __device__
#else
#define VT_PLAN_HD
#endif
struct Take {
    int nbatch;  // batches of this block's group
    int nstat;   // blocks per counter = batches owned statically, at most
    int sb;      // this block's static batch (it exists iff sb < nbatch)
    int ndyn;    // batches the counter hands out
    bool takes;  // this block touches the counter
    unsigned last;  // the failed take's value that marks the counter's last user
};
VT_PLAN_HD inline int take_groups(int nblk) { return nblk >= 8 ? 8 : 1; }
VT_PLAN_HD inline int take_group_of(int l, int nblk) { return nblk >= 8 ? (l & 7) : 0; }
// Which template block a thread block of the plane scan serves, and which of that template
// block's nqc blocks it is.  Template-block-major (the dense launch, pass B2): the nqc blocks
// of a template block are adjacent ids.  lfirst (pass B1): block l of every template block,
// then block l + 1 of every one, so the blocks that work (the first `use` of each) stand in
// front of the ones that leave at once.
struct BlockId {
    int tb, l;
};
VT_PLAN_HD inline BlockId block_id(unsigned bid, int ntb, int nqc, bool lfirst) {
    if (lfirst) {
        const unsigned l = bid / (unsigned)ntb;
        return {(int)(bid - l * (unsigned)ntb), (int)l};
    }
    const unsigned tb = bid / (unsigned)nqc;
    return {(int)tb, (int)(bid - tb * (unsigned)nqc)};
}
// Blocks that serve a list of nq entries in batches of nb, about `per` batches each, of the
// nqc the grid holds per template block (a multiple of 8 when nqc >= 8).
VT_PLAN_HD inline int list_use(int nq, int nb, int per, int nqc) {
    const int use = ((nq + nb - 1) / nb + per - 1) / per;
    if (nqc >= 8) {
        const int u8 = (use + 7) & ~7;
        return u8 < 8 ? 8 : (u8 > nqc ? nqc : u8);
    }
    return use < 1 ? 1 : (use > nqc ? nqc : use);
}
// Entries per batch (W) of a list pass, decided by each thread block from its list's length.
// A batch is walked by one thread block, its entries one after the other, so a short list in
// batches of 4 leaves most of the device idle: 63 entries are 16 working blocks per template
// block, 256 on a device that holds 512, each walking four queries in turn behind its
// prologue.  `fill` is the resident thread blocks divided by the template blocks (at least
// 1): the working blocks per template block that make one full resident round.  The widest W
// of {4, 2, 1} whose list_use reaches fill; 1 if none does.  Lists long enough for fill at 4
// (pass B2 at the headline, every all-miss list, any library with more template blocks than
// resident thread blocks) keep 4.  
VT_PLAN_HD inline int list_width(int entries, int per, int fill, int nqc) {
    if (list_use(entries, 4, per, nqc) >= fill) return 4;
    if (list_use(entries, 2, per, nqc) >= fill) return 2;
    return 1;
}
// The working blocks of a list whose batch the rule narrowed: no more than one resident round
// (fill, in whole groups of 8 like list_use).  list_use rounds up to eight blocks' worth, so
// lists a little longer than fill * w entries would otherwise put a few blocks into a second
// round, each behind a prologue of its own; the batches beyond the blocks go to the counters,
// where the blocks that finish first take them.
VT_PLAN_HD inline int list_round(int use, int fill, int nqc) {
    int cap = fill < 1 ? 1 : fill;
    if (nqc >= 8) cap = (cap + 7) & ~7;
    return use < cap ? use : cap;
}
// The ids of a block's static batch are read in the same trip as the list's length, so before
// W is known: every lane reads one candidate, lanes 0-3 the four entries of the batch of 4,
// lanes 4-5 the two of the batch of 2, lane 6 the one of the batch of 1 (lane 7 reads lane
// 6's again; every eight lanes alike).  spec_index: the entry lane reads for the block whose
// static batch is `batch` (sb * G + g), clamped into the slab of ld entries; spec_lane: the
// lane that holds entry 0 of width w's batch, entry e in lane spec_lane(w) + e.
VT_PLAN_HD inline int spec_width(int lane) { return (lane & 7) < 4 ? 4 : (lane & 7) < 6 ? 2 : 1; }
VT_PLAN_HD inline int spec_entry(int lane) { return (lane & 7) < 4 ? (lane & 7) : (lane & 7) < 6 ? (lane & 7) - 4 : 0; }
VT_PLAN_HD inline int spec_index(int batch, int lane, int ld) {
    const int i = batch * spec_width(lane) + spec_entry(lane);
    return i < ld - 1 ? i : ld - 1;
}
VT_PLAN_HD inline int spec_lane(int w) { return w == 4 ? 0 : w == 2 ? 4 : 6; }
// Batches per block of list pass B2 (list_use's per).  A block's prologue is one round trip
// for 128 KiB of template planes, paid per block, so fewer, longer blocks win while the
// template blocks are few and their blocks run side by side: 1,000 templates (16 template
// blocks; per 4 is 1,024 thread blocks there, two full rounds of the 512 resident) step in
// 0.354 ms with 4 against 0.371 with 3.  With more template blocks than resident thread
// blocks 3 measured faster (the cause is not established; the GPU is then full of other
// template blocks' work either way): 100,000 templates (1,563 template blocks) 6.59 ms per launch with 3, 7.51
// with 4; at 10,000 (157) the two are level.
inline int list_per(int ntb, int resident_blocks) { return ntb < resident_blocks ? 4 : 3; }
// Block l of the nblk that serve nq queries in batches of nb.
VT_PLAN_HD inline Take take_plan(int nq, int nb, int l, int nblk) {
    const int G = take_groups(nblk), g = take_group_of(l, nblk);
    Take t;
    t.nbatch = ((nq + nb - 1) / nb - g + G - 1) / G;
    t.nstat = nblk / G;
    t.sb = G == 8 ? (l >> 3) : l;
    t.ndyn = t.nbatch > t.nstat ? t.nbatch - t.nstat : 0;
    t.takes = t.ndyn > 0 && t.sb < t.nbatch;
    t.last = (unsigned)(t.ndyn + (t.nstat < t.nbatch ? t.nstat : t.nbatch) - 1);
    return t;
}
// The batch that take value t stands for (it exists iff it is < nbatch).
VT_PLAN_HD inline int take_batch(const Take& t, unsigned take) { return t.nstat + (int)take; }

// Frozen key scans of at least this many queries prune (RS_VT_PRUNE=1, the default).
constexpr int VT_PRUNE_MIN_Q = 512;
constexpr int64_t VT_PRUNE_MAX_TB = 65535;  // the list kernels' grid.y

// Whether a scan of nq queries against ntb template blocks from block tb0 takes the pruned
// path (forms: the view holds QS_J and compact planes; prune: 0 never, 1 the large scans,
// 2 "force").  Below VT_PRUNE_MIN_Q queries the call is one latency-bound launch and the
// prefilter, the list kernels and two scan passes cost more than they save; one template
// block has nothing to prune.
inline bool prunes(int H, bool cand, int64_t tb0, bool forms, int64_t ntb, int prune, int nq) {
    return H == 64 && !cand && tb0 == 0 && forms && ntb <= VT_PRUNE_MAX_TB &&
           (prune == 2 || (prune == 1 && nq >= VT_PRUNE_MIN_Q && ntb >= 2));
}

// --- The single list pass (RS_VT_PASSES).  passes: 1, the front kernel
// writes one list per template block on its verified score U0 and one list pass scans it;
// 2, the candidate block's pass (B1), then the lists on U(q) (B2).  No shape keeps two
// passes by rule today: the place for one is here.
inline int prune_passes(int passes_switch, int /*ntb*/, int /*nq*/) { return passes_switch == 2 ? 2 : 1; }
// The `fill` its list pass hands vt_plan::list_width: four resident rounds' worth of working
// blocks per template block, where passes B1 and B2 ask for one.  Measured at the headline
// (sixteen lists of about 1,005 entries, fill 32): in batches of 4 the pass is 64 working blocks
// per template block and takes 207 us, in batches of 2 (128 blocks) 171, of 1 181; lists that
// reach four rounds at 4 entries (every all-miss list) keep 4.  
#ifndef VT_SINGLE_ROUNDS
#define VT_SINGLE_ROUNDS 4
#endif
inline int single_pass_fill(int fill) { return std::min(65535, VT_SINGLE_ROUNDS * std::max(1, fill)); }
// Its list counters need no closing launch: they are doubled by call parity.  A pruned call
// appends to its own parity's counters, which the call before left at zero, and its first
// thread block zeroes the other parity's, the call before's, which nobody appends to during
// this call; the next call starts behind this one on the stream.  So the last call's counts
// stay readable until the next pruned call begins.  `used` is how many counters of a parity
// may be nonzero: what the next call has to zero.  A growth reallocates zeroed.
struct ParityCounters {
    int cap = 0;             // counters per parity
    int par = 0;             // the next pruned call's parity
    int used[2] = {0, 0};    // counters of each parity that may be nonzero
    int last = -1;           // the last pruned call's parity (-1: none yet)
};
struct ParityCall {
    size_t mine, other;      // offsets of this call's counters and of the ones it zeroes
    int nzero;               // how many of the others it zeroes
};
// Whether ntb counters per parity need a larger (zeroed) buffer, and its new capacity.
inline bool parity_grows(const ParityCounters& s, int ntb) { return ntb > s.cap; }
inline void parity_grown(ParityCounters& s, int ntb) {
    s.cap = std::max(ntb, 2 * s.cap);
    s.used[0] = s.used[1] = 0;
    s.last = -1;
}
inline ParityCall parity_begin(ParityCounters& s, int ntb) {
    const int p = s.par;
    const ParityCall c{(size_t)p * (size_t)s.cap, (size_t)(p ^ 1) * (size_t)s.cap, s.used[p ^ 1]};
    s.used[p ^ 1] = 0;
    s.used[p] = ntb;
    s.last = p;
    s.par = p ^ 1;
    return c;
}
// Where the last pruned call's counts are (valid while s.last >= 0).
inline size_t parity_last_offset(const ParityCounters& s) { return (size_t)s.last * (size_t)s.cap; }

// The prefilter's grid: x covers the template blocks, tb_per_block to a thread block; y the
// batches of q_per_batch queries, as many as keep the grid within `cap` thread blocks (at
// least one: the kernel strides over the rest).
struct Grid2 {
    int x, y;
};
inline Grid2 prefilter_grid(int ntb, int nq, int tb_per_block, int q_per_batch, int cap) {
    const int nqb = (nq + q_per_batch - 1) / q_per_batch, pfx = (ntb + tb_per_block - 1) / tb_per_block;
    return {pfx, std::min(nqb, std::max(1, cap / pfx))};
}

// Whether the prefilter and the verification run as one launch (vt_front_kernel: a thread
// block walks every template block for its query groups, tb_per_block at a time, then picks
// and verifies in its tail).  Yes when one thread block covers the library anyway: one
// chunk, and the grid is the prefilter's own.  Otherwise the two launches, the prefilter's
// grid with x > 1.  A wider rule, "or the query groups alone fill the resident thread
// blocks", measured slower where it applied (10,000 templates x 5,120 queries, ten chunks
// per group: 1.37 ms per step against 1.34): a thread block then loads
// its template planes once per group and chunk, where the prefilter loads them once for
// three groups.
inline bool front_fused(int ntb, int tb_per_block) { return ntb <= tb_per_block; }
// Its grid: x = 1, y the query groups within `cap` thread blocks; block y serves the groups
// y, y + grid.y, ... (the kernel strides), so every group is served exactly once.
inline Grid2 front_grid(int nq, int q_per_batch, int cap) {
    return {1, std::max(1, std::min((nq + q_per_batch - 1) / q_per_batch, cap))};
}

// Thread blocks of 256 of a key export of n keys (the kernel strides): a batch's keys, and
// the rows of rs_vt_match_stream.
constexpr int VT_EXPORT_BLOCKS = 64, VT_EXPORT_BLOCKS_STREAM = 256;
inline int export_grid(int64_t n, int max_blocks) { return (int)std::min<int64_t>((n + 255) / 256, max_blocks); }

// Batches of at most this many queries are read by the plane kernel straight from the
// pinned staging array (one launch in place of a host-to-device copy and the launch;
// the kernel leaves the raw bytes in dQraw for the template stores); RS_VT_ZC=0: always
// the copy.
constexpr int VT_ZC_MAX = 64;
inline bool stages_in_place(bool planar, int nq, bool zc_on) { return planar && nq <= VT_ZC_MAX && zc_on; }

// The host polls a call's keys in pinned memory instead of synchronising the stream
// (RS_VT_POLL=0: never), unless events time the scan or the keys are too many to spin on.
constexpr int VT_POLL_MAX = 4096;
inline bool polls_keys(bool poll_on, bool timed, int nq) { return poll_on && !timed && nq <= VT_POLL_MAX; }
// A plane scan whose keys the host polls exports them itself (its last block): one
// launch fewer per call.  Not when they are min-reduced over ranks first (fold_ok).
inline bool folds_keys(bool fold_ok, bool planar, int64_t local_count, bool poll_on, bool timing, int nq) {
    return fold_ok && planar && local_count > 0 && polls_keys(poll_on, timing, nq);
}

// rs_vt_match_stream's three ways through nb batches.
//   Fused: device-resident batches of the plane scan.  One launch builds every batch's
//     planes and ONE scan launch covers all nb * nq queries (the batches are independent
//     against a frozen library, and their keys are rows of one array), so the scan's fixed
//     costs -- each block's template planes into VGPRs, the last partial round of blocks --
//     are paid once per call instead of once per batch; a sharded handle then min-reduces
//     all rows in one collective.
//   HostGroups: host batches of the plane scan take the same path in groups (below).
//   PerBatch: every other handle, and one device-resident batch: a build and a scan per
//     batch, each row min-reduced on the collective stream.
enum class StreamPath { Fused, HostGroups, PerBatch };
inline StreamPath stream_path(bool on_device, bool planar, int nb) {
    if (!planar) return StreamPath::PerBatch;
    if (!on_device) return StreamPath::HostGroups;
    return nb > 1 ? StreamPath::Fused : StreamPath::PerBatch;
}

// Host batches in upload groups: a group is uploaded on the upload stream into one of two
// device buffers while the previous group's planes and scan run on the main stream (the
// upload of pageable memory holds the host, not the GPU), then its planes are built in one
// launch and scanned in one launch.  One batch per launch with its upload in line (the
// earlier form) ran at 0.52 of the HBM-resident rate.
// A first group of one batch (its upload is the only one not hidden behind a scan), then
// groups of about a third of the rest (2 .. VT_UP_GROUP batches: a scan launch of >= 2
// batches keeps the fused launch's efficiency).  10 batches of 1,024 queries from a
// pageable array: groups (1, 3, 3, 3) 1.674 ms per call against 1.745 for (2, 2, 2, 2, 2),
// 1.759 for threes, 1.762 for fives, 1.920 for ones, and 1.757 with the caller's array
// page-locked for the call (hipHostRegister): the uploads are not the bound
// (tools/stream_ab.py --host).
constexpr int VT_UP_GROUP = 16;  // host batches per upload group, at most
struct HostGroup {
    int b0, n;   // batches [b0, b0 + n); n == 0: past the last group
    int buf;     // which of the two upload buffers
    bool waits;  // the buffer's group before last must have had its planes built (evUsed)
};
struct HostGroups {
    int gb;      // batches per group (the capacity of an upload buffer)
    int first;   // batches of group 0
    int nb;
    HostGroup group(int g) const {
        const int b0 = g == 0 ? 0 : std::min(nb, first + (g - 1) * gb);
        return {b0, std::min(g == 0 ? first : gb, nb - b0), g & 1, g >= 2};
    }
};
inline HostGroups host_groups(int nb) {
    const int gb = std::min(nb, std::max(2, std::min(VT_UP_GROUP, (nb - 1) / 3)));
    return {gb, nb >= 4 ? 1 : gb, nb};
}

// --- True-SAD metric (RS_VT_METRIC_SAD; csrc/vt_sad.h).
constexpr int METRIC_WRAPPED = 0, METRIC_SAD = 1;   // RS_VT_METRIC_* of the ABI
inline bool metric_known(int metric) { return metric == METRIC_WRAPPED || metric == METRIC_SAD; }
// The fast form keeps a template column's H rows in registers and has an instance for the
// two shipped heights at the reference's max_offset; every other shape is generic.
inline bool sad_fast(int H, int max_offset) { return max_offset == 8 && (H == 64 || H == 32); }
inline const char* sad_form(int H, int max_offset) { return sad_fast(H, max_offset) ? "sad" : "sad-generic"; }
// Queries per group (accumulator sets per wave).  2: 107 VGPRs at H = 64, two 8-wave blocks
// a CU, so one block's LDS phase and barrier run beside the other's v_sad_u8 stream;
// 1,024 queries x 10,000 templates of 64 x 32 scan in 1.95 ms with 2 or 3, 2.16 with 4
// (135 VGPRs, one block a CU) and 2.14 with 8 (tools/vt_sad_ab.py).
constexpr int SAD_NQ = 2;
constexpr int SAD_NW = 8;   // waves per block, at most: one dword column each per pass
inline int sad_waves(int WD) { return std::min(WD, SAD_NW); }
// Blocks per template block (nqc) of the fast form: block j of a template block walks the
// query groups j, j + nqc, .. with its template columns resident.  The blocks are equal and
// 512 are resident (two a CU), so the grid wants many rounds of them, or its last round
// leaves CUs idle: enough blocks for about SAD_TARGET_BLOCKS in the grid.  But a block's
// prologue (its columns, 128 KiB at W = 32, into registers) is paid per block: no block
// walks fewer than SAD_MIN_GROUPS groups while the groups allow it.
constexpr int SAD_TARGET_BLOCKS = 4096, SAD_MIN_GROUPS = 8;
inline int sad_split(int ntb, int ngroups) {
    const int want = (SAD_TARGET_BLOCKS + ntb - 1) / ntb;
    return std::max(1, std::min(want, ngroups / SAD_MIN_GROUPS));
}

}  // namespace vt_plan
