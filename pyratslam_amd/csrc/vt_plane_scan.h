// The bit-plane scan kernel (vt_scan_plane_kernel): dense, matrix and list instances.
// Part of view_templates.hip, the one translation unit: not free-standing (it relies on the
// includes, the anonymous namespace and the headers that view_templates.hip includes before it).
#pragma once

// Query start rows [M-3, H-M-1] are split into PL_SPLIT ranges, one wave each
// per column group, so a wave keeps only the template units its rows meet
// (10 of 16 at H = 64): fewer VGPRs, four waves per SIMD.
constexpr int PL_SPLIT = 2;

template <int H, int HALF>
struct PlaneRange {
    static constexpr int M = FAST_M, NU = H / 4, S0 = M - 3, S1 = H - M - 1, NS = S1 - S0 + 1;
    static constexpr int NSH = (NS + PL_SPLIT - 1) / PL_SPLIT;
    static constexpr int SA = S0 + HALF * NSH;
    static constexpr int SB = (SA + NSH - 1) < S1 ? SA + NSH - 1 : S1;
    static constexpr int ja(int s) { return (s - (M - 1)) > 0 ? (s - (M - 1) + 3) / 4 : 0; }
    static constexpr int jb(int s) { return (s + (M - 1)) / 4 < NU - 1 ? (s + (M - 1)) / 4 : NU - 1; }
    static constexpr int JLO = ja(SA), JHI = jb(SB), NUH = JHI - JLO + 1;
};

// The walk over a wave's start rows [SA, SB] goes one residue class of S mod 4 at
// a time: a start row S meets offsets o = 4J - S only, so one class touches 3 or 4
// of the 2M-1 offsets ({-4,0,4}, {-5,-1,3,7}, {-6,-2,2,6}, {-7,-3,1,5} at M = 8)
// and only that many counters are live at once (ascending S kept all 2M-1 live for
// the whole query).  A class's counts are flushed into the LDS partial sums when
// the class ends, packed as u16 pairs taken within the class.  Offset index
// x = o + M - 1 belongs to class (M-1-x) mod 4, where it is counter x / 4.
constexpr int PL_NO = 2 * FAST_M - 1;
constexpr int PL_NA = (PL_NO + 3) / 4;   // counters of the largest class
constexpr int pl_class(int x) { return ((FAST_M - 1 - x) % 4 + 4) % 4; }
constexpr int pl_class_n(int rho) {      // offsets of class rho
    const int base = ((FAST_M - 1 - rho) % 4 + 4) % 4;
    return base < PL_NO ? (PL_NO - 1 - base) / 4 + 1 : 0;
}
constexpr int pl_class_slot(int rho) {   // first partial-count slot of class rho
    int s = 0;
    for (int r = 0; r < rho; ++r) s += (pl_class_n(r) + 1) / 2;
    return s;
}
constexpr int pl_slot(int x) { return pl_class_slot(pl_class(x)) + x / 8; }
constexpr int pl_half(int x) { return (x / 4) & 1; }

struct QRow {   // the 8 planes of one query unit
    uint32_t v[8];
};

template <int H, int HALF>
struct PlaneWalk {
    using R = PlaneRange<H, HALF>;
    static constexpr int NR = R::SB - R::SA + 1;
    static constexpr int first(int rho) { return R::SA + ((rho - R::SA) % 4 + 4) % 4; }
    static constexpr int rows(int rho) { return first(rho) <= R::SB ? (R::SB - first(rho)) / 4 + 1 : 0; }
    static constexpr int row(int i) {   // start row of step i
        for (int rho = 0; rho < 4; ++rho) {
            if (i < rows(rho)) return first(rho) + 4 * i;
            i -= rows(rho);
        }
        return -1;
    }
    static constexpr bool last(int i) { return i + 1 == NR || (row(i + 1) & 3) != (row(i) & 3); }
    static constexpr bool units_ok() {
        for (int s = R::SA; s <= R::SB; ++s) {
            const int nj = R::jb(s) - R::ja(s) + 1;
            if (nj < 1 || nj > PL_NA || R::ja(s) < R::JLO || R::jb(s) > R::JHI) return false;
        }
        return true;
    }
    static_assert(units_ok(), "units per query row");
    static_assert(rows(0) && rows(1) && rows(2) && rows(3), "every class has a row");
};

// One query start row S against the template units it meets (o = 4J - S within
// +-(M-1): 3 or 4 units).  The borrow chains of those units are interleaved
// plane by plane, so consecutive bitop3s are independent (a single chain would
// stall on every instruction).  All indices are compile-time.
template <int H, int HALF, int S>
__device__ __forceinline__ void plane_row(const uint32_t (&P)[PlaneRange<H, HALF>::NUH][8],
                                          const QRow& q, uint32_t (&a)[PL_NA]) {
    using R = PlaneRange<H, HALF>;
    constexpr int M = FAST_M, JA = R::ja(S), NJ = R::jb(S) - JA + 1;
    uint32_t b[NJ];
#pragma unroll
    for (int k = 0; k < 8; ++k)
#pragma unroll
        for (int j = 0; j < NJ; ++j)
            b[j] = __builtin_amdgcn_bitop3_b32(P[JA - R::JLO + j][k], q.v[k], k ? b[j] : 0u, 0x8E);
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        // v_bcnt's own accumulator (asm keeps the compiler from re-associating
        // the counts into half-rate v_add3_u32)
        uint32_t& c = a[(4 * (JA + j) - S + M - 1) / 4];
        asm("v_bcnt_u32_b32 %0, %1, %2" : "=v"(c) : "v"(b[j]), "v"(c));
    }
}

template <int H, int HALF, int S>
__device__ __forceinline__ QRow plane_read(const uint32_t* sq) {
    using R = PlaneRange<H, HALF>;
    const uint4 lo = *reinterpret_cast<const uint4*>(sq + (S - R::S0) * 8);
    const uint4 hi = *reinterpret_cast<const uint4*>(sq + (S - R::S0) * 8 + 4);
    return QRow{{lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w}};
}

// Query planes are staged per batch in LDS and read as wave-uniform
// ds_read_b128 broadcasts into VGPRs: on gfx950 a VALU instruction with an SGPR
// operand issues at about half the all-VGPR rate (tools/ubench_chain.hip:
// 0.23 vs 0.36-0.41 wave-instructions per SIMD-cycle), so the chains take both
// operands from VGPRs.  Step I of the walk: q holds its row's planes on entry and
// the next step's on return (after the last step, the first row of the next
// query, from sqn).  The next row's reads are issued ahead of this row's chains,
// in the registers the class order freed; the scheduling barrier keeps them from
// sinking back to their use (built with the max-ILP scheduler, _build.py, they end
// up a few planes into the row before, when that row's first planes are dead).
template <int H, int HALF, int I>
__device__ __forceinline__ void plane_walk(const uint32_t (&P)[PlaneRange<H, HALF>::NUH][8],
                                           const uint32_t* sq, const uint32_t* sqn, QRow& q,
                                           uint32_t (&a)[PL_NA], uint32_t (&part)[pl_class_slot(4)][64],
                                           int lane) {
    using WK = PlaneWalk<H, HALF>;
    constexpr int S = WK::row(I);
    constexpr bool wrap = I + 1 == WK::NR;
    const QRow qn = plane_read<H, HALF, WK::row(wrap ? 0 : I + 1)>(wrap ? sqn : sq);
    __builtin_amdgcn_sched_barrier(0);
    plane_row<H, HALF, S>(P, q, a);
    if constexpr (WK::last(I)) {
        constexpr int rho = S & 3, n = pl_class_n(rho);
#pragma unroll
        for (int k = 0; k < (n + 1) / 2; ++k)
            atomicAdd(&part[pl_class_slot(rho) + k][lane], a[2 * k] | (2 * k + 1 < n ? a[2 * k + 1] << 16 : 0u));
#pragma unroll
        for (int k = 0; k < PL_NA; ++k) a[k] = 0u;
    }
    q = qn;
    if constexpr (!wrap) plane_walk<H, HALF, I + 1>(P, sq, sqn, q, a, part, lane);
}


template <int H>
struct PlaneLds {
    static constexpr int M = FAST_M, NS = H - 2 * M + 3, NO = 2 * M - 1, NK = (NO + 1) / 2;
    static constexpr int QW = PL_CG * NS * 8;                 // query-plane dwords per query
    static constexpr int NW = PL_CG * PL_SPLIT;                // waves per block
    static constexpr int QP = (PL_NB * QW / 4 + 63) / 64 * 64;  // padded to whole 1 KiB wave-instructions
};

// The plane scan's LDS.  Double-buffered: batch i computes from its staged query
// planes and adds its partial counts into part[i&1] while batch i+1 is staged into
// the other plane buffer; one barrier per batch.  Each buffer is its own
// namespace-scope __shared__ variable and every access names one of them at
// compile time (pl_q<H, CUR>, pl_part<CUR>): hipcc waits for an LDS-DMA in flight
// before any LDS access it cannot prove disjoint from the DMA's variable, so
// only distinct, statically named variables let the next batch's DMA stay in
// flight through this batch's compute.
constexpr int PL_NK = PlaneLds<64>::NK;   // the same for every H (it depends on max_offset only)
static_assert(PlaneLds<32>::NK == PL_NK, "partial-count slots independent of H");
static_assert(pl_class_slot(4) == PL_NK, "the classes' u16 pairs fill the same slots");
// the staged query planes, sized per template height (a kernel allocates only the
// instances it names: the H = 32 scan, the ROS node's geometry, does not carry the
// H = 64 buffers)
template <int H>
__shared__ uint4 vt_pl_qa[PlaneLds<H>::QP];   // even batches
template <int H>
__shared__ uint4 vt_pl_qb[PlaneLds<H>::QP];   // odd batches
__shared__ uint32_t vt_pl_part0[PL_NB][PL_NK][64];  // u16 pairs of partial counts, summed by ds_add
__shared__ uint32_t vt_pl_part1[PL_NB][PL_NK][64];
__shared__ int vt_pl_bidx[3];             // batches taken ahead (ring)
alignas(16) __shared__ uint32_t vt_pl_ts[16][64];  // TS(o) of the block's 64 templates (LDS-DMA, 16 bytes a lane)
template <int H, int CUR>
__device__ __forceinline__ uint4* pl_q() {
    if constexpr (CUR == 0) return vt_pl_qa<H>;
    else return vt_pl_qb<H>;
}
template <int CUR>
__device__ __forceinline__ uint32_t (&pl_part())[PL_NB][PL_NK][64] {
    if constexpr (CUR == 0) return vt_pl_part0;
    else return vt_pl_part1;
}

template <int H, int HALF>
__device__ __forceinline__ void plane_load_units(const uint4* __restrict__ planes, int tb, int cg,
                                                 int lane, uint32_t (&P)[PlaneRange<H, HALF>::NUH][8]) {
    using R = PlaneRange<H, HALF>;
    const uint4* src = planes + ((size_t)(tb * PL_CG + cg) * (H / 4) + R::JLO) * 128 + lane;
#pragma unroll
    for (int j = 0; j < R::NUH; ++j) {
        const uint4 a = src[(2 * j) * 64], b = src[(2 * j + 1) * 64];
        P[j][0] = a.x; P[j][1] = a.y; P[j][2] = a.z; P[j][3] = a.w;
        P[j][4] = b.x; P[j][5] = b.y; P[j][6] = b.z; P[j][7] = b.w;
    }
}

// The work of one wave: column group cg, query start rows of range HALF.  One
// barrier per batch: before it, every wave stages its share of the next batch's
// planes and adds this batch's partial counts into LDS (ds_add; the per-half
// sums stay < 2^16, so the packed pairs never carry); after it, wave w < nb
// finishes query w of the batch and clears its partial slots for batch i+2.
// A block's first batch is its own (vt_plan::take_plan); the later ones are taken one
// ahead by thread 0, and a block stops taking after its first failed take, so every
// block that takes ends on exactly one failed take (counter rewind).
// One batch of plane_wave: compute from qcur (staged by the previous batch or the
// prologue) while this wave's share of the next batch goes global -> LDS into qnxt.
// CUR is the parity of the iteration (it & 1), so the plane buffers and the
// partial-count slots are compile-time: each LDS read names one __shared__
// variable and each DMA the other, and hipcc leaves the DMA in flight through the
// compute (a runtime choice of buffer made it wait vmcnt(0) before the first read).
// Returns false once the block has no batch left.
// LIST (pruned scan): the block's queries are the nq entries of its list ids[]: a
// batch is PL_NB consecutive entries, each DMA lane takes its source from its
// entry's query id, and the finish uses the id.  The ids of the batch being
// computed (qc) and of the one staged next (qnv, entry lane & 3) are carried from
// batch to batch: the ids of the batch after next are read right after the barrier.
// A list's batch is W = 4, 2 or 1 consecutive entries (vt_plan::list_width, decided by the
// block from the list's length); a batch of fewer than PL_NB fills the first W slots of the
// LDS buffers, and entries of (lane & 3) >= W in qnv and qc are read and never used.
// Single list pass (tbstar != nullptr): the finishing wave of entry (tb, q) with tbstar[q] == tb,
// the candidate block of an unsettled query, stores the block's minimum score, U(q), into
// ublk[q] (rs_vt_prune_stats counts the two-pass rule from it).
struct PlaneIds {
    int qc[PL_NB];  // query ids of the batch being computed (wave-uniform)
    int qnv;        // lane: query id of entry (lane & 3) of the batch staged next
    const int* tbstar = nullptr;
    uint32_t* ublk = nullptr;
    int tb = 0;     // the thread block's template block
};
// One take from the group's counter (thread 0): the batch it stands for, tk.nbatch when the
// block does not take; a failed take's value is kept for the rewind.
__device__ __forceinline__ int plane_take(unsigned* __restrict__ ctr, const vt_plan::Take& tk, unsigned& failed) {
    if (!tk.takes) return tk.nbatch;
    const unsigned t = atomicAdd(ctr, 1u);
    const int b = vt_plan::take_batch(tk, t);
    if (b >= tk.nbatch) failed = t;   // (>= ndyn >= 1: never mistaken for "no failed take")
    return b;
}
// Lanes' share of query batch `src` (ids qx[] with LIST, else consecutive from qn) -> LDS dst.
template <int H, bool LIST>
__device__ __forceinline__ void plane_stage(const uint4* __restrict__ qp4, int qn, int nbn, const int (&qx)[PL_NB],
                                            uint4* dst, int wave, int lane) {
    using LD = PlaneLds<H>;
    constexpr int NT = 64 * LD::NW;
    const int lim = nbn * LD::QW / 4;
    const uint4* src = qp4 + (size_t)qn * (LD::QW / 4);
#pragma unroll
    for (int k = 0; k < (LD::QP + NT - 1) / NT; ++k) {
        const int i0 = wave * 64 + k * NT;  // wave-uniform
        if (i0 < lim) {
            const uint4* from;
            if constexpr (LIST) {   // a 1 KiB piece may straddle two entries: per-lane source
                const int i = min(i0 + lane, lim - 1), e = i / (LD::QW / 4);
                const int id = e == 0 ? qx[0] : e == 1 ? qx[1] : e == 2 ? qx[2] : qx[3];
                from = qp4 + (size_t)id * (LD::QW / 4) + (i - e * (LD::QW / 4));
            } else {
                from = src + min(i0 + lane, lim - 1);
            }
            __builtin_amdgcn_global_load_lds((__attribute__((address_space(1))) const void*)from,
                                             (__attribute__((address_space(3))) void*)(dst + i0), 16, 0, 0);
        }
    }
}
// FIRST: the block's first batch.  The ids of the batch staged next were asked for only after
// the prologue's barrier (they depend on the take), so a list block issues that DMA after its
// first query's walk, when they have long arrived, not in front of the compute.
template <int H, int HALF, bool MATRIX, int CUR, bool LIST, bool FIRST = false>
__device__ __forceinline__ bool plane_batch(const uint32_t (&P)[PlaneRange<H, HALF>::NUH][8], int it,
                                            int& bi, const vt_plan::Take& tk, int64_t slot, int64_t count,
                                            const uint4* __restrict__ qp4, const uint32_t* __restrict__ qsum,
                                            int nq, unsigned* __restrict__ ctr, int G, int g, ScanOut out,
                                            int rank, int nranks, int wave, int cg, int lane,
                                            unsigned& failed, const int* __restrict__ ids, PlaneIds& pid,
                                            int w) {
    using R = PlaneRange<H, HALF>;
    using LD = PlaneLds<H>;
    constexpr int NO = LD::NO, NK = LD::NK, NS = LD::NS;
    constexpr bool DEFER = FIRST && LIST;
    const int W = LIST ? w : PL_NB;   // entries per batch (block-uniform; a list's own, PlaneList)
    const int nbatch = tk.nbatch;
    if (bi >= nbatch) return false;  // block-uniform
    const uint4* qcur = pl_q<H, CUR>();
    uint4* qnxt = pl_q<H, CUR ^ 1>();
    uint32_t(&part)[PL_NB][PL_NK][64] = pl_part<CUR>();
    const int tid = wave * 64 + lane;
    // batch ring: iteration it reads the next batch from slot (it+1) % 3 and thread
    // 0 writes the one after it into slot (it+2) % 3, last read two barriers ago
    const int r1 = (it + 1) % 3, r2 = (it + 2) % 3;
    const int bn = vt_pl_bidx[r1];
    const int qb = (bi * G + g) * W, nb = min(W, nq - qb);
    // The take comes first (its result is waited for); with no next batch there is
    // no further take: this block's failed take was bn.
    if (tid == 0)  // the batch after next
        vt_pl_bidx[r2] = bn < nbatch ? plane_take(ctr, tk, failed) : nbatch;
    // the next batch's planes go global -> LDS directly (global_load_lds, 1 KiB per
    // wave-instruction, lane-linear), in flight through this batch's compute
    int qnx[PL_NB] = {0, 0, 0, 0};  // LIST: the next batch's query ids
    auto stage_next = [&]() {
        if (bn < nbatch) {
            const int qn = (bn * G + g) * W, nbn = min(W, nq - qn);
            if constexpr (LIST) {
                static_assert(PL_NB == 4, "four ids per batch");
#pragma unroll
                for (int e = 0; e < PL_NB; ++e) qnx[e] = __builtin_amdgcn_readlane(pid.qnv, e);
            }
            plane_stage<H, LIST>(qp4, qn, nbn, qnx, qnxt, wave, lane);
        }
    };
    if constexpr (!DEFER) stage_next();
    const uint32_t* sq0 = reinterpret_cast<const uint32_t*>(qcur) + cg * NS * 8;
    QRow q = plane_read<H, HALF, PlaneWalk<H, HALF>::row(0)>(sq0);
    auto walk = [&](int b) {
        uint32_t a[PL_NA];
#pragma unroll
        for (int k = 0; k < PL_NA; ++k) a[k] = 0u;
        // (the last query of the batch reads its own first rows again)
        plane_walk<H, HALF, 0>(P, sq0 + b * (PL_CG * NS * 8), sq0 + min(b + 1, nb - 1) * (PL_CG * NS * 8), q, a,
                               part[b], lane);
    };
    if constexpr (DEFER) {
        walk(0);
        stage_next();
    }
#pragma unroll 1
    for (int b = DEFER ? 1 : 0; b < nb; ++b) walk(b);
    if constexpr (FIRST) VT_STAMP(4);
    // every wave's DMA into qnxt has landed before any wave passes the barrier and
    // reads it (explicit: nothing else guarantees this wait stays in front of it)
    __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0)
    __syncthreads();
    if (wave < nb) {  // wave w finishes query qb + w of the batch
        const int qi = !LIST ? qb + wave
                             : wave == 0 ? pid.qc[0] : wave == 1 ? pid.qc[1] : wave == 2 ? pid.qc[2] : pid.qc[3];
        uint32_t best = 0xFFFFFFFFu, t[NK];
#pragma unroll
        for (int k = 0; k < NK; ++k) {
            t[k] = part[wave][k][lane];
            part[wave][k][lane] = 0u;
        }
#pragma unroll
        for (int x = 0; x < NO; ++x)   // each count with its own TS(o)
            best = min(best, vt_pl_ts[x][lane] + 256u * (pl_half(x) ? t[pl_slot(x)] >> 16 : t[pl_slot(x)] & 0xFFFFu));
        if constexpr (LIST) {
            // emit_score's key, with the reduced one at hand for ublk
            const unsigned long long g = (unsigned long long)slot * nranks + rank;
            const unsigned long long key =
                wave_min_u64(slot < count ? (((unsigned long long)(best - qsum[qi]) << 32) | g) : NO_KEY);
            if (lane == 0) {
                atomicMin(out.best + qi, key);
                // (read behind the reduction: ahead of it the value costs the walk a VGPR)
                if (pid.tbstar && pid.tbstar[qi] == pid.tb) pid.ublk[qi] = (uint32_t)(key >> 32);
            }
        } else {
            emit_score<MATRIX>(out, slot, count, qi, nq, best - qsum[qi], rank, nranks, lane == 0);
        }
    }
    if constexpr (LIST) {
#pragma unroll
        for (int e = 0; e < PL_NB; ++e) pid.qc[e] = qnx[e];
        const int b2 = vt_pl_bidx[r2];   // thread 0 wrote it before the barrier
        pid.qnv = b2 < nbatch ? ids[min((b2 * G + g) * W + (lane & 3), nq - 1)] : 0;
    }
    bi = bn;
    return true;
}

// The block owns batch tk.sb of its group without asking (vt_plan::take_plan), so everything
// the first batch needs is asked for at once, in one global round trip: the take of the
// batch after it (thread 0, first: returns come back in order), the first batch's query
// planes and TS by LDS-DMA, the template planes into P; the partial-count slots are zeroed
// while they fly.  v0 (LIST): the lanes' candidates for the static batch's ids, read by the
// kernel together with the list's length (vt_plan::spec_index); w: the list's entries per batch.
template <int H, int HALF, bool MATRIX, bool LIST>
__device__ __forceinline__ void plane_wave(const uint4* __restrict__ planes, const uint32_t* __restrict__ tsum,
                                           int tb, int64_t count, const uint4* __restrict__ qp4,
                                           const uint32_t* __restrict__ qsum, int nq,
                                           unsigned* __restrict__ ctr, int G, int g, ScanOut out,
                                           int rank, int nranks, int wave, int cg, int lane,
                                           unsigned& failed, const int* __restrict__ ids,
                                           const vt_plan::Take& tk, int v0, int w, const int* tbstar,
                                           uint32_t* ublk) {
    using R = PlaneRange<H, HALF>;
    const int nbatch = tk.nbatch, tid = wave * 64 + lane;
    const int W = LIST ? w : PL_NB;   // entries per batch (block-uniform)
    int bi = tk.sb, b1 = nbatch;
    if (tid == 0) b1 = plane_take(ctr, tk, failed);
    for (int i = tid; i < PL_NB * PL_NK * 64; i += 64 * PL_CG * PL_SPLIT) {
        (&vt_pl_part0[0][0][0])[i] = 0u;
        (&vt_pl_part1[0][0][0])[i] = 0u;
    }
    PlaneIds pid{{0, 0, 0, 0}, 0, tbstar, ublk, tb};
    if constexpr (LIST) {
#pragma unroll
        for (int e = 0; e < PL_NB; ++e) pid.qc[e] = __builtin_amdgcn_readlane(v0, vt_plan::spec_lane(W) + e);
    }
    {
        const int qb = (bi * G + g) * W;
        plane_stage<H, LIST>(qp4, qb, min(W, nq - qb), pid.qc, vt_pl_qa<H>, wave, lane);
    }
    uint32_t P[R::NUH][8];
    plane_load_units<H, HALF>(planes, tb, cg, lane, P);
    static_assert(sizeof(vt_pl_ts) == 4 * 64 * 16, "TS: one 1 KiB DMA piece from each of four waves");
    if (wave < 4)
        __builtin_amdgcn_global_load_lds(
            (__attribute__((address_space(1))) const void*)(reinterpret_cast<const uint4*>(tsum) +
                                                            (size_t)tb * 256 + wave * 64 + lane),
            (__attribute__((address_space(3))) void*)(reinterpret_cast<uint4*>(&vt_pl_ts[0][0]) + wave * 64), 16, 0,
            0);
    if (tid == 0) {
        vt_pl_bidx[0] = bi;
        vt_pl_bidx[1] = b1;
    }
    VT_STAMP(1);
    // every wave's share of the first batch and of TS has landed before any wave passes the
    // barrier (and this wave's template planes with them: the walk needs them at once)
    __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0)
    VT_STAMP(3);
    __syncthreads();
    VT_STAMP(2);
    const int64_t slot = (int64_t)tb * 64 + lane;
    if constexpr (LIST) {   // the ids of the second batch: used after the first query's walk
        b1 = vt_pl_bidx[1];
        pid.qnv = b1 < nbatch ? ids[min((b1 * G + g) * W + (lane & 3), nq - 1)] : 0;
    }
    // unrolled by two: even iterations compute from qa and stage into qb, odd ones
    // the other way round (the prologue staged the first batch into qa)
    // The first batch is peeled off the loop: hipcc's wait analysis is exact for the
    // LDS accesses after a DMA issued in the same loop iteration but not across the
    // loop header's merge, so the loop body starts with an odd batch, whose compute
    // follows its own DMA issue, not the header.
    if (plane_batch<H, HALF, MATRIX, 0, LIST, true>(P, 0, bi, tk, slot, count, qp4, qsum, nq, ctr, G, g, out, rank,
                                                    nranks, wave, cg, lane, failed, ids, pid, W))
        for (int it = 1;; it += 2) {
            if (!plane_batch<H, HALF, MATRIX, 1, LIST>(P, it, bi, tk, slot, count, qp4, qsum, nq, ctr, G, g, out,
                                                       rank, nranks, wave, cg, lane, failed, ids, pid, W))
                break;
            if (!plane_batch<H, HALF, MATRIX, 0, LIST>(P, it + 1, bi, tk, slot, count, qp4, qsum, nq, ctr, G, g,
                                                       out, rank, nranks, wave, cg, lane, failed, ids, pid, W))
                break;
        }
    VT_STAMP(5);
}

// nqc blocks serve each template block; they take query batches of PL_NB from
// the template block's counter, so blocks that the SIMDs' oldest-first issue
// favours take more batches and no SIMD is left running a lone straggler.
// LIST (pruned scan, passes B1 and B2): template block tb scans only the queries of
// its list, pl.ids[tb * pl.ld ..] (pl.cnt[tb] entries, any order); nq is then the
// list's length.  A block whose list is empty, or whose static batch does not exist,
// leaves at once: before it asks for its template planes, and without a take.
// Batches per block of a list-driven pass (headline step, ms: 2 -> 0.525, 3 -> 0.515,
// 4 -> 0.527, 6 -> 0.567).
// Per launch (PlaneList::per): pass B1's lists hold only the queries the verification
// left unsettled, about 64 per template block at the headline shape: one batch per
// block there (VT_LIST_PER_B1; headline step, ms: 1 -> 0.467, 2 -> 0.473, 3 -> 0.493;
// DESIGN section 19).
// With the one-round-trip prologue (headline step, ms, per-process
// medians: B2 1 -> 0.360, 2 -> 0.361, 3 -> 0.371, 4 -> 0.354; B1 2 -> 0.386 beside 0.371),
// but 100,000 templates: 3 -> 6.59 ms per launch, 4 -> 7.51.  Pass B2 therefore takes
// vt_plan::list_per(template blocks, resident thread blocks): 4 or 3.  VT_LIST_PER, when
// defined (A/B builds), replaces the rule.
#ifndef VT_LIST_PER_B1
#define VT_LIST_PER_B1 1
#endif
// Entries per batch: each thread block takes vt_plan::list_width of its
// list's length, of per and of fill = resident thread blocks / template blocks, so a short
// list (pass B1: about 63 entries) is served by a full resident round of blocks in batches
// of 2 where batches of 4 occupy half of the device, and by no more blocks than that round
// (vt_plan::list_round); nb = 4, 2 or 1 replaces the rule (RS_VT_LIST_NB, or -DVT_LIST_NB=n
// for an A/B build).
// lfirst: the grid is sized for lists of every query, so of pass B1's 128 blocks per template
// block about 32 work and 96 leave on the list's length.  Numbered template block by template
// block, the leavers of one stand in the dispatch order ahead of the next one's workers, and
// once the workers fill most of the device they pass through the few slots left: the last
// template blocks' workers started late (pass B1 at 2 per batch: 26.6 us; with the blocks
// numbered l-major, every template block's l-th block side by side, 20.7).  Pass B2's lists
// fill their blocks, and its query planes are shared by the template blocks of an XCD group:
// it keeps the template-block-major order.
// per, nb and fill share the word that held per: the kernel's arguments, the hidden ones
// behind them included, keep their places, and the dense instances their code.
struct PlaneList {
    const int* ids = nullptr;
    const unsigned* cnt = nullptr;
    int ld = 0;
    uint32_t per : 8;
    uint32_t nb : 7;       // 0: by the rule
    uint32_t lfirst : 1;   // block ids run over the template blocks first (vt_plan::block_id): pass B1
    uint32_t fill : 16;
};
static_assert(sizeof(PlaneList) == 24, "the plane scan's kernel arguments keep their layout");
// The list instance's own argument: the single list pass's two buffers behind the dense
// instances' words (they keep PlaneList, and with it their arguments' places).
struct PlaneListU : PlaneList {
    const int* tbstar = nullptr;   // nullptr: passes B1 and B2
    uint32_t* ublk = nullptr;
};
template <bool LIST>
using PlaneListArg = std::conditional_t<LIST, PlaneListU, PlaneList>;
#ifdef VT_LIST_NB
static_assert(VT_LIST_NB == 1 || VT_LIST_NB == 2 || VT_LIST_NB == 4, "entries per batch: 1, 2 or 4");
#else
#define VT_LIST_NB 0
#endif

template <int H, bool MATRIX, bool LIST = false>
__global__ __launch_bounds__(64 * PL_CG * PL_SPLIT) __attribute__((amdgpu_waves_per_eu(4, 4)))
void vt_scan_plane_kernel(const uint4* __restrict__ planes, const uint32_t* __restrict__ tsum,
                          int ntb, int64_t count, const uint32_t* __restrict__ qp,
                          const uint32_t* __restrict__ qsum, int nq, int nqc,
                          unsigned* __restrict__ next_batch, ScanOut out, int rank, int nranks,
                          PlaneListArg<LIST> pl) {
    static_assert(PL_SPLIT == 2, "two row ranges");
    static_assert(!(LIST && MATRIX), "lists feed the key scan only");
    // The nqc blocks of a template block are adjacent block ids, so they are dispatched
    // together and split its query batches dynamically even when the grid runs in
    // several rounds.  XCD-aware: blocks b and b+8 share an XCD (and its L2); with
    // nqc >= 8 (a multiple of 8) the query batches are split into 8 groups by XCD, so
    // each L2 holds one group's planes
    VT_STAMP_BEGIN();
    // (pass B1 numbers its blocks the other way round, PlaneList::lfirst)
    const vt_plan::BlockId bid = vt_plan::block_id(blockIdx.x, ntb, nqc, LIST && pl.lfirst);
    const int tb = bid.tb;
    const int l = bid.l;   // this block among its template block's
    const int G = vt_plan::take_groups(nqc), g = vt_plan::take_group_of(l, nqc);
    unsigned* ctr = next_batch + (size_t)tb * 8 + g;
    const int lane = threadIdx.x & 63;
    const int* ids = nullptr;
    int v0 = 0;
    int W = PL_NB;   // entries per batch: a list's own (block-uniform), the dense launch's constant
    if constexpr (LIST) {
        // One round trip: the list's length and, before it is known, the ids of the batch
        // this block would own (the first `use` blocks own batches l >> 3 of group l & 7, or
        // l) at each width the length may choose, in distinct lanes (vt_plan::spec_index).
        // The speculative read stays inside the slab (ld entries); its value is used
        // only if the length says the entries exist.
        ids = pl.ids + (size_t)tb * pl.ld;
        v0 = ids[vt_plan::spec_index((G == 8 ? l >> 3 : l) * G + g, lane, pl.ld)];
        nq = (int)pl.cnt[tb];   // block-uniform
        if (nq == 0) return;
        W = pl.nb ? (int)pl.nb : vt_plan::list_width(nq, pl.per, pl.fill, nqc);
        // The grid is sized for a list of every query; a shorter list is served by
        // the first `use` of the template block's nqc blocks, about pl.per batches
        // each, so a block's fixed cost (its template planes, 128 KiB) is not paid per
        // batch.  The others leave before they ask for anything else.
        int use = vt_plan::list_use(nq, W, pl.per, nqc);
        if (!pl.nb && W < PL_NB) use = vt_plan::list_round(use, pl.fill, nqc);   // (the rule's own: vt_plan.h)
        if (l >= use) return;
        nqc = use;
    }
    // Which batches are this block's: its static one, and the counter's (vt_plan.h).  The
    // nqc / G blocks sharing a counter each end on exactly one failed take when the group
    // has more batches than blocks, and on none otherwise.
    const vt_plan::Take tk = vt_plan::take_plan(nq, W, l, nqc);
    VT_STAMP_KNOWN();
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int cg = wave % PL_CG, half = wave / PL_CG;
    unsigned failed = 0u;  // thread 0: the value of this block's one failed take
    const uint4* qp4 = reinterpret_cast<const uint4*>(qp);
    const int* tbstar = nullptr;
    uint32_t* ublk = nullptr;
    if constexpr (LIST) {
        tbstar = pl.tbstar;
        ublk = pl.ublk;
    }
    if (tk.sb >= tk.nbatch) {   // (block-uniform) no batch for this block: it leaves the counter alone
    } else if (half == 0)
        plane_wave<H, 0, MATRIX, LIST>(planes, tsum, tb, count, qp4, qsum, nq, ctr, G, g, out, rank, nranks,
                                       wave, cg, lane, failed, ids, tk, v0, W, tbstar, ublk);
    else
        plane_wave<H, 1, MATRIX, LIST>(planes, tsum, tb, count, qp4, qsum, nq, ctr, G, g, out, rank, nranks,
                                       wave, cg, lane, failed, ids, tk, v0, W, tbstar, ublk);
    // The block whose failed take returned tk.last is the counter's last user in this
    // launch: it rewinds the counter for the next launch (no memset).
    if (threadIdx.x == 0 && tk.takes && failed == tk.last) *ctr = 0u;
    if constexpr (!MATRIX) {
        if (out.host) {   // (kernel argument: uniform)
            // The key export folded into the scan (small calls, vt_scan_local_impl): the
            // keys are agent-scope atomics (performed at memory, never held in an L2), each
            // wave waits for its own (vmcnt(0)) before the block's counter add, the last
            // adder learns it from the add's return value and reads the keys with sc1
            // loads, then stores them into the pinned host words and resets them.
            // The model's agent-scope release before each block's counter add and acquire
            // in the last block frame the hand-off (a release fence after the block barrier
            // is cumulative over the waves' atomics; the acquire is one cache invalidate in
            // one block of the launch).
            __shared__ int s_last;
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __syncthreads();
            if (threadIdx.x == 0) {
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
                s_last = __hip_atomic_fetch_add(out.done, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) ==
                         gridDim.x - 1;
                if (s_last) __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
            }
            __syncthreads();
            if (s_last) {
                for (int i = threadIdx.x; i < nq; i += blockDim.x) {
                    const unsigned long long k =
                        __hip_atomic_load(out.best + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    __hip_atomic_store(out.best + i, ~0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    __hip_atomic_store(out.host + i, k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                }
                if (threadIdx.x == 0) __hip_atomic_store(out.done, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        }
    }
    VT_STAMP(6);
}
