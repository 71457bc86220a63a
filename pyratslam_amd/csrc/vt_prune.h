// The pruned plane scan (H = 64): prefilter, verification, the front kernel and the list
// passes; and vt_keys_export, which stays behind them (the compiler emits non-template
// kernels in order of definition, and it was the file's last).
// Part of view_templates.hip, the one translation unit: not free-standing (it relies on the
// includes, the anonymous namespace and the headers that view_templates.hip includes before it).
#pragma once

// --- Pruned plane scan (H = 64, keys): partial-distortion elimination.  Every term
// of a score is >= 0, so the sum over the byte pairs of PF_NU template units,
//   LB(t, q, o) = sum_J  TS_J(t) - QS_J(q, 4J - o) + 256 * B_J(t, q, o)
// (TS_J the unit's byte sum, QS_J the byte sum of the four query rows it meets at
// offset o, B_J their borrow count, all three over the unit's first PF_CGS column groups
// only), is an exact lower bound of score(t, q, o), and
// minLB[tb][q] = min over the block's templates and the offsets bounds every score of
// template block tb against q.  Pass B1 scans each query against its candidate block
// tb* = argmin_tb minLB (lowest on ties) only, which leaves an upper bound U(q) in
// best[]; pass B2 scans it against every other block with minLB <= U(q) -- "<=": a
// block that may hold an equal score at a lower index is scanned too.  A block left
// out has minLB > U(q) >= the minimum, so none of its scores is the minimum.
// With a single list pass (the default, RS_VT_PASSES) the verification
// lists on its own score U0 >= U(q) instead, tb* for an unsettled query and every other block
// with minLB <= U0: a superset of the two lists, scanned once, the same keys.
constexpr int PF_WAVES = 4;   // waves per thread block
// Template blocks per wave: every staged query plane is read once (an LDS broadcast)
// for all of them, which divides the LDS reads per VALU instruction: at one block per
// wave and a whole unit, 120 ds_read_b128 against 600 VALU per query, the reads set the
// pace (167 us against 135 us at the dense scan's VALU rate, headline shape).  A wave
// holds 64 plane VGPRs: two blocks of a whole unit, or four of half a unit (one
// ds_read_b128 per 18 VALU, the dense walk's ratio).  Two whole units of two blocks
// would not fit the VGPRs.
#ifndef VT_PF_TPW
#define VT_PF_TPW (VT_PF_UNITS == 1 ? 8 / (VT_PF_CGS) : 1)
#endif
constexpr int PF_TPW = VT_PF_TPW;
// Column groups per step of the walk: PF_TPW * PF_CPS independent borrow chains, four as
// the whole unit's two blocks had (two groups of four blocks at once: 117 VGPRs, and
// measured slower).
#ifndef VT_PF_CPS
#define VT_PF_CPS (VT_PF_TPW >= 4 ? 1 : 2)
#endif
constexpr int PF_CPS = VT_PF_CPS;
// Upper limit of the prefilter's thread blocks: beyond it a thread block takes several
// batches of PF_NB queries and loads its template planes once for them (2048 and 1024
// measured slower than 4096 at the headline shape).
#ifndef VT_PF_GRID_CAP
#define VT_PF_GRID_CAP 4096
#endif
constexpr int PF_NB = 4;      // queries staged per step
constexpr int PF_QW4 = PF_NU * PF_CGS * PL_NO * 2;   // staged uint4 per query
constexpr uint32_t PF_NONE = (1u << 26) - 1u;       // "no other template": above every score

// The walk adds TS once, after the minimum over the offsets: the staged sums are
// PF_BIAS - QS_J (PF_BIAS above every QS_J, so every partial bound stays non-negative) and
// a wave keeps tsb = sum_J TS_J - PF_NU * PF_BIAS per template.
constexpr uint32_t PF_BIAS = PF_CGS * 32 * 256;
static_assert(PF_NU * (PF_CGS * 32 * 256 + PF_BIAS) < (1u << 31), "the biased bounds do not wrap");

// The first PF_CGS column groups of the PF_NU units of template blocks tb0 .. tb0 + PF_TPW - 1
// (lane = template; a block past the library reads the last one and is not valid).
__device__ __forceinline__ void pf_load(const uint4* __restrict__ planes, int ntb, int64_t count, int tb0, int lane,
                                        uint32_t (&P)[PF_TPW][PF_NU][PF_CGS][8], uint32_t (&tsb)[PF_TPW],
                                        bool (&valid)[PF_TPW]) {
    constexpr int NU = 64 / 4;
#pragma unroll
    for (int t = 0; t < PF_TPW; ++t) {
        const int tbc = min(tb0 + t, ntb - 1);
        valid[t] = tb0 + t < ntb && (int64_t)(tb0 + t) * 64 + lane < count;
        tsb[t] = 0u - PF_NU * PF_BIAS;
#pragma unroll
        for (int u = 0; u < PF_NU; ++u) {
#pragma unroll
            for (int cg = 0; cg < PF_CGS; ++cg) {
                const uint4* src = planes + ((size_t)(tbc * PL_CG + cg) * NU + pf_unit(u)) * 128 + lane;
                const uint4 a = src[0], b = src[64];
                uint32_t(&p)[8] = P[t][u][cg];
                p[0] = a.x; p[1] = a.y; p[2] = a.z; p[3] = a.w;
                p[4] = b.x; p[5] = b.y; p[6] = b.z; p[7] = b.w;
#pragma unroll
                for (int k = 0; k < 8; ++k) tsb[t] += (uint32_t)__builtin_popcount(p[k]) << k;
            }
        }
    }
}

// Stage queries q0 .. q0 + nb - 1 for the walk (the whole thread block; barriers around it
// are the caller's).
__device__ __forceinline__ void pf_stage(const uint4* __restrict__ qc4, const uint32_t* __restrict__ qsj, int q0, int nb,
                                         uint4 (&s_q)[PF_NB][PF_NU][PF_CGS][PL_NO][2],
                                         uint32_t (&s_qs)[PF_NB][PF_NU][16]) {
    constexpr int M = FAST_M, S0 = M - 3;
    for (int i = threadIdx.x; i < nb * PF_QW4; i += blockDim.x) {
        const int qq = i / PF_QW4, r = i - qq * PF_QW4;
        const int u = r / (PF_CGS * PL_NO * 2), r2 = r - u * (PF_CGS * PL_NO * 2);
        const int cg = r2 / (PL_NO * 2), w = r2 - cg * (PL_NO * 2);
        // start rows 4J-(M-1) .. 4J+(M-1) of column group cg < PF_CGS, two uint4 each,
        // shifted out of the two aligned units around each
        (&s_q[0][0][0][0][0])[i] = qc_unit(qc4 + (size_t)(q0 + qq) * QC_Q4, cg,
                                           4 * pf_unit(u) - (M - 1) - S0 + (w >> 1), w & 1);
    }
    if ((int)threadIdx.x < nb * PF_NU * 16)
        (&s_qs[0][0][0])[threadIdx.x] = PF_BIAS - qsj[(size_t)q0 * PF_NU * 16 + threadIdx.x];
}

// One staged query against the wave's PF_TPW template blocks: v = (bound << 6) | lane of
// the block's minimum (the lowest lane on ties), w = min2, the minimum over the block's
// other valid templates (PF_NONE when it has no other).  Wave-uniform.
__device__ __forceinline__ void pf_walk(const uint32_t (&P)[PF_TPW][PF_NU][PF_CGS][8], const uint32_t (&tsb)[PF_TPW],
                                        const bool (&valid)[PF_TPW], const uint4 (&sq)[PF_NU][PF_CGS][PL_NO][2],
                                        const uint32_t (&sqs)[PF_NU][16], int lane, uint32_t (&v)[PF_TPW],
                                        uint32_t (&w)[PF_TPW]) {
    uint32_t m[PF_TPW];
#pragma unroll
    for (int t = 0; t < PF_TPW; ++t) m[t] = 0xFFFFFFFFu;
    // the planes of offset x, unit u, column groups cp .. cp + PF_CPS - 1
    auto read_q = [&](int x, int u, int cp, uint32_t(&q)[PF_CPS][8]) {
#pragma unroll
        for (int i = 0; i < PF_CPS; ++i) {
            const uint4 lo = sq[u][cp + i][PL_NO - 1 - x][0];
            const uint4 hi = sq[u][cp + i][PL_NO - 1 - x][1];
            q[i][0] = lo.x; q[i][1] = lo.y; q[i][2] = lo.z; q[i][3] = lo.w;
            q[i][4] = hi.x; q[i][5] = hi.y; q[i][6] = hi.z; q[i][7] = hi.w;
        }
    };
#pragma unroll
    for (int x = 0; x < PL_NO; ++x) {   // offset o = x - (M-1): start row 4J - o
        uint32_t lb[PF_TPW];
#pragma unroll
        for (int t = 0; t < PF_TPW; ++t) lb[t] = 0u;
#pragma unroll
        for (int u = 0; u < PF_NU; ++u) {
            uint32_t c[PF_TPW];
#pragma unroll
            for (int t = 0; t < PF_TPW; ++t) c[t] = 0u;
#pragma unroll
            for (int cp = 0; cp < PF_CGS; cp += PF_CPS) {
                uint32_t q[PF_CPS][8], b[PF_TPW][PF_CPS];
                read_q(x, u, cp, q);
#pragma unroll
                for (int k = 0; k < 8; ++k)
#pragma unroll
                    for (int t = 0; t < PF_TPW; ++t)
#pragma unroll
                        for (int i = 0; i < PF_CPS; ++i)
                            b[t][i] = __builtin_amdgcn_bitop3_b32(P[t][u][cp + i][k], q[i][k],
                                                                  k ? b[t][i] : 0u, 0x8E);
#pragma unroll
                for (int t = 0; t < PF_TPW; ++t)
#pragma unroll
                    for (int i = 0; i < PF_CPS; ++i)
                        asm("v_bcnt_u32_b32 %0, %1, %2" : "=v"(c[t]) : "v"(b[t][i]), "v"(c[t]));
                // (the max-ILP scheduler would pull the reads of many offsets ahead and
                // spill; the SIMD's other waves cover this wave's read latency)
                __builtin_amdgcn_sched_barrier(0);
            }
            const uint32_t qsb = sqs[u][x];   // PF_BIAS - QS_J
#pragma unroll
            for (int t = 0; t < PF_TPW; ++t) lb[t] += (c[t] << 8) + qsb;
        }
#pragma unroll
        for (int t = 0; t < PF_TPW; ++t) m[t] = min(m[t], lb[t]);
    }
    // All the reductions before the first store: behind a store's branch, a block's
    // running minimum is used in a later basic block only, its updates sink there,
    // and the 15 counts per block they wait for stay live (spills at four blocks).
#pragma unroll
    for (int t = 0; t < PF_TPW; ++t) {
        // value and lane in one reduction (a bound is below 2^26; the lowest lane on
        // ties), then the minimum over the valid templates other than that lane
        const uint32_t lbt = m[t] + tsb[t];   // >= 0 in all; the parts wrap mod 2^32
        v[t] = wave_min_u32_dpp(valid[t] ? (lbt << 6) | (uint32_t)lane : 0xFFFFFFFFu);
        w[t] = wave_min_u32_dpp(valid[t] && lane != (int)(v[t] & 63u) ? lbt : PF_NONE);
    }
}

// The single list pass: where the verification writes the lists itself.
// cnt == nullptr: two passes, the list kernels below write them.  cnt[tb] counts list[tb * nq ..],
// this call's parity of the counters; the call's first thread block zeroes the nzero counters
// of the other parity (vt_plan::parity_begin).  ublk[q] = U0 of a settled query (the list pass
// stores U(q) of the others): with minlb and tbstar, what rs_vt_prune_stats counts from.
struct FrontLists {
    unsigned* cnt = nullptr;
    int* list = nullptr;
    uint32_t* ublk = nullptr;
    unsigned* zero = nullptr;
    int nzero = 0;
};
__device__ __forceinline__ void front_zero(const FrontLists& fl) {
    if (blockIdx.x == 0 && blockIdx.y == 0)   // (block-uniform)
        for (int b = threadIdx.x; b < fl.nzero; b += blockDim.x) fl.zero[b] = 0u;
}

// minlb[tb * nq + q], and second[tb * nq + q] = (min2 << 6) | lane: the lane that holds
// the block's minimum (the lowest on ties) and min2, the minimum over the block's other
// valid templates (PF_NONE when it has no other).  The pick verifies that one template
// (vt_prune_verify_kernel).  Lane = template; the wave keeps the first PF_CGS column groups
// of the PF_NU units of its PF_TPW template blocks in VGPRs and reads the staged query
// planes as wave-uniform LDS broadcasts, PF_CPS column groups at a time (PF_CPS * PF_TPW
// independent borrow chains).
__global__ __launch_bounds__(64 * PF_WAVES) __attribute__((amdgpu_waves_per_eu(4)))
void vt_prefilter_kernel(const uint4* __restrict__ planes, int ntb,
                                                                    int64_t count,
                                                                    const uint4* __restrict__ qc4,
                                                                    const uint32_t* __restrict__ qsj, int nq,
                                                                    uint32_t* __restrict__ minlb,
                                                                    uint32_t* __restrict__ second, FrontLists fl) {
    front_zero(fl);
    static_assert(PF_CGS % PF_CPS == 0 && PF_CGS >= 1 && PF_CGS <= PL_CG, "whole steps of column groups, of the unit");
    static_assert(PF_NU * PF_CGS * 32 * 255 < (int)PF_NONE, "a bound and a lane fit one word");
    __shared__ uint4 s_q[PF_NB][PF_NU][PF_CGS][PL_NO][2];
    __shared__ uint32_t s_qs[PF_NB][PF_NU][16];
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const int tb0 = (blockIdx.x * PF_WAVES + wave) * PF_TPW;
    const bool live = tb0 < ntb;   // wave-uniform; a wave past the library still stages
    uint32_t P[PF_TPW][PF_NU][PF_CGS][8], tsb[PF_TPW];
    bool valid[PF_TPW];
    pf_load(planes, ntb, count, tb0, lane, P, tsb, valid);
    for (int q0 = blockIdx.y * PF_NB; q0 < nq; q0 += gridDim.y * PF_NB) {   // block-uniform
        const int nb = min(PF_NB, nq - q0);
        __syncthreads();   // the batch before has been read
        pf_stage(qc4, qsj, q0, nb, s_q, s_qs);
        __syncthreads();
        if (!live) continue;
#pragma unroll 1
        for (int qq = 0; qq < nb; ++qq) {
            uint32_t v[PF_TPW], w[PF_TPW];
            pf_walk(P, tsb, valid, s_q[qq], s_qs[qq], lane, v, w);
            if (lane == 0) {
#pragma unroll
                for (int t = 0; t < PF_TPW; ++t)
                    if (tb0 + t < ntb) {
                        // (a block of the library holds a valid template: v is a packed bound)
                        minlb[(size_t)(tb0 + t) * nq + q0 + qq] = v[t] >> 6;
                        second[(size_t)(tb0 + t) * nq + q0 + qq] = (w[t] << 6) | (v[t] & 63u);
                    }
            }
        }
    }
}

// Append q to a template block's list where `in`.  Atomics of the whole device on one
// counter run one after the other at memory (about 0.2 us each, measured: 160 waves'
// adds on each of 16 counters took 32 us), so a thread block of 1,024 queries adds
// once: ballots, a scan of the waves' counts in LDS, one atomic.  The order within a
// list does not matter, keys meet by atomicMin.
constexpr int VT_LIST_T = 1024;
__device__ __forceinline__ void list_append(bool in, int q, unsigned* __restrict__ cnt, int* __restrict__ list) {
    __shared__ unsigned s_w[VT_LIST_T / 64];
    __shared__ unsigned s_base;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long mask = __ballot(in);
    if (lane == 0) s_w[wave] = (unsigned)__popcll(mask);
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned t = 0u;
        for (int w = 0; w < VT_LIST_T / 64; ++w) {
            const unsigned c = s_w[w];
            s_w[w] = t;
            t += c;
        }
        s_base = t ? atomicAdd(cnt, t) : 0u;
    }
    __syncthreads();
    if (in) list[s_base + s_w[wave] + (unsigned)__popcll(mask & ((1ull << lane) - 1ull))] = q;
}

// List (a): the candidate block of every query, tb* = argmin_tb minLB[tb][q] ...
// (strict <: the lowest block on ties), and the verification of the one template the
// prefilter singled out in it, t^ = the lane of the block's minimum bound.  One wave per
// query.  U0 = the exact score of (t^, q), from the resident planes the scan reads:
// lane (x, cg) counts the borrows of offset x - (M-1) in column group cg over the
// template units j whose query start row 4j - o lies in [M-3, H-M-1] (the others meet
// zeroed rows only), the four column groups meet by shuffles, and
//   U0 = min_x TS(x) + 256 * B(x) - QS,
// the scan's own expression.  If min2 > U0, every other template of the block has
// score >= bound >= min2 > U0: the block's first argmin is t^ with score U0, the key
// the block scan would leave, and the query is settled: its key goes into best[] here
// and tbstar[q] = ~tb* keeps it off list1.  ">": a template whose bound equals U0 may
// hold an equal score at a lower index, so that query is block-scanned.
// The query's planes come from its compact units (vt_qplane_kernel): lane (x, cg) walks
// the aligned units upwards and shifts each pair by its own constant 8 * ((-o - 5) & 3).
// Once U0 is known the wave writes every start row of the query into qp4 if a scan pass
// will stage it: it is unsettled (list1), or another block's bound does not exceed U0
// (the rule of vt_prune_rest_kernel: list2).  Nothing else reads a query's full planes.
constexpr int VT_VQ4 = PlaneLds<64>::QW / 4;   // uint4 of a query's planes
constexpr int VT_VR = QC_NA + 7;               // staged unit rows: 3 never-counted, the units, the zero unit, 3 more
// One wave's verification of query q (the body above, shared by vt_prune_verify_kernel and
// the tail of vt_front_kernel, so the rule has one definition).  pick(pk, sec, m2) leaves
// each lane's share of the pick: its least key (minLB << 32) | tb, that block's `second`,
// and its lowest bound but one; the query's planes and QS are in flight through it.
// s_q, s_t: the wave's own VT_VQS and VT_VTS uint4 of LDS.  Between the staging stores and
// the reads of other lanes' entries: WAVE_LDS = false, a __syncthreads (every wave of the
// thread block must then call this); true, where s_q and s_t are no other wave's, the wave's
// own wait for its LDS writes, so a thread block's waves verify independently and a wave
// without a query does not call at all.
constexpr int VT_VQS = PL_CG * VT_VR * 2, VT_VTS = PL_CG * (64 / 4) * 2;
template <bool WAVE_LDS, class Pick>
__device__ __forceinline__ void vt_verify_query(int q, int lane, Pick&& pick, int nq,
                                                const uint4* __restrict__ planes,
                                                const uint32_t* __restrict__ tsum,
                                                const uint4* __restrict__ qc4, uint4* __restrict__ qp4,
                                                const uint32_t* __restrict__ qsum,
                                                unsigned long long* __restrict__ best, int rank, int nranks,
                                                int* __restrict__ tbstar, uint4* s_q, uint4* s_t,
                                                const uint32_t* minlb, int ntb, const FrontLists& fl) {
    constexpr int M = FAST_M, NU = 64 / 4, NS = PlaneLds<64>::NS, S0 = M - 3, S1 = 64 - M - 1;
    static_assert(PL_NO * PL_CG <= 64, "one lane per (offset, column group)");
    constexpr int QK = (QC_Q4 + 63) / 64;
    // s_q [cg][3 + aligned unit][2]: unit QC_NA is the zero unit; the rows before and after are
    // read (never counted) where a template unit meets no start row of the window
    // s_t [cg][unit][2]
    const int x = lane >> 2, cg = lane & 3, o = x - (M - 1);
    // what does not wait for the pick, in flight through it: the query's planes and QS
    uint4 qv[QK];
#pragma unroll
    for (int k = 0; k < QK; ++k) qv[k] = qc4[(size_t)q * QC_Q4 + min(lane + 64 * k, QC_Q4 - 1)];
    const uint32_t qs = qsum[q];
    // the pick: each lane's blocks with their `second`, so the winner's is at hand, and
    // the lane's lowest bound but one (for the lowest bound of the blocks other than tb*)
    unsigned long long pk = ~0ull;
    uint32_t sec = 0u, m2 = 0xFFFFFFFFu;
    pick(pk, sec, m2);
    // (keeps the plane reads above in front of the reduction: left alone they sink to
    // their LDS stores, one memory round trip each)
#pragma unroll
    for (int k = 0; k < QK; ++k) asm volatile("" : "+v"(qv[k].x), "+v"(qv[k].y), "+v"(qv[k].z), "+v"(qv[k].w));
    const unsigned long long mk = wave_min_u64(pk);
    const int tbs = (int)(unsigned)mk;
    uint32_t other = pk == mk ? m2 : (uint32_t)(pk >> 32);   // min over tb != tb* of minLB[tb][q]
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) other = min(other, (uint32_t)__shfl_xor((int)other, off));
    sec = (uint32_t)__shfl((int)sec, __ffsll((unsigned long long)__ballot(pk == mk)) - 1);   // (one lane holds block tbs)
    const int tl = (int)(sec & 63u);
    const uint32_t ts = x < PL_NO ? tsum[((size_t)tbs * 16 + x) * 64 + tl] : 0u;
    static_assert(PL_CG * NU * 2 == 128, "two template chunks per lane");
    const uint4 t0 = planes[((size_t)tbs * 128 + lane) * 64 + tl];
    const uint4 t1 = planes[((size_t)tbs * 128 + 64 + lane) * 64 + tl];
    s_t[lane] = t0;
    s_t[64 + lane] = t1;
#pragma unroll
    for (int k = 0; k < QK; ++k) {
        const int c = lane + 64 * k, g = c / (QC_NA * 2);
        if (c < QC_Q4) s_q[(g * VT_VR + 3) * 2 + (c - g * (QC_NA * 2))] = qv[k];
    }
    if (lane < 2 * PL_CG) s_q[((lane >> 1) * VT_VR + 3 + QC_NA) * 2 + (lane & 1)] = make_uint4(0u, 0u, 0u, 0u);
    if constexpr (WAVE_LDS) {
        // (the clobber keeps the compiler's LDS reads below behind the stores above; the
        // wave's LDS instructions complete in order)
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_wave_barrier();
    } else {
        __syncthreads();
    }
    uint32_t cnt = 0u;
    if (x < PL_NO) {
        // start row 4j - o = S0 + 4 (j + a) + r: the units a + j and a + j + 1, shifted by 8r
        const int a = (-o - S0) >> 2;   // (arithmetic: -3 .. 0)
        const uint32_t sh = 8u * (uint32_t)((-o - S0) & 3);
        const uint4* sq = s_q + (cg * VT_VR + 3 + a) * 2;
        uint4 la = sq[0], lc = sq[1];
        // (four units' reads in flight: unrolled fully, the max-ILP scheduler reads all
        // sixteen ahead into 176 VGPRs, two waves per SIMD.  Branch-free: a unit whose
        // start row lies outside the window reads rows nobody staged and counts nothing)
#pragma unroll 4
        for (int j = 0; j < NU; ++j) {
            const bool in = 4 * j - o >= S0 && 4 * j - o <= S1;
            const uint4 ta = s_t[(cg * NU + j) * 2], tc = s_t[(cg * NU + j) * 2 + 1];
            const uint4 ha = sq[(j + 1) * 2], hc = sq[(j + 1) * 2 + 1];
            const uint4 qa = qc_shift(la, ha, sh), qc = qc_shift(lc, hc, sh);
            la = ha;
            lc = hc;
            uint32_t b = __builtin_amdgcn_bitop3_b32(ta.x, qa.x, 0u, 0x8E);
            b = __builtin_amdgcn_bitop3_b32(ta.y, qa.y, b, 0x8E);
            b = __builtin_amdgcn_bitop3_b32(ta.z, qa.z, b, 0x8E);
            b = __builtin_amdgcn_bitop3_b32(ta.w, qa.w, b, 0x8E);
            b = __builtin_amdgcn_bitop3_b32(tc.x, qc.x, b, 0x8E);
            b = __builtin_amdgcn_bitop3_b32(tc.y, qc.y, b, 0x8E);
            b = __builtin_amdgcn_bitop3_b32(tc.z, qc.z, b, 0x8E);
            b = __builtin_amdgcn_bitop3_b32(tc.w, qc.w, b, 0x8E);
            cnt += in ? (uint32_t)__builtin_popcount(b) : 0u;
        }
    }
    cnt += __shfl_xor(cnt, 1);
    cnt += __shfl_xor(cnt, 2);
    uint32_t u0 = x < PL_NO ? ts + 256u * cnt : 0xFFFFFFFFu;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) u0 = min(u0, (uint32_t)__shfl_xor(u0, off));
    u0 -= qs;
    const bool settled = (sec >> 6) > u0;
    // single list pass: the bounds of the first 64 blocks, in flight through the expansion below
    const bool lists = fl.cnt && (!settled || other <= u0);   // (wave-uniform)
    uint32_t mlb0 = 0u;
    if (lists && lane < ntb) mlb0 = minlb[(size_t)lane * nq + q];
    if (!settled || other <= u0) {   // (wave-uniform) a scan pass stages this query
#pragma unroll
        for (int k = 0; k < (VT_VQ4 + 63) / 64; ++k) {
            const int i = lane + 64 * k, g = i / (NS * 2), r = i - g * (NS * 2), si = r >> 1;
            if (i < VT_VQ4) {
                const uint4* su = s_q + (g * VT_VR + 3 + (si >> 2)) * 2 + (r & 1);
                qp4[(size_t)q * VT_VQ4 + i] = qc_shift(su[0], su[2], 8u * (uint32_t)(si & 3));
            }
        }
    }
    if (lists) {   // single list pass: the lists, written here
        asm volatile("" : "+v"(mlb0));   // (mlb0 is needed here: its read does not sink into the loop)
        // tb* if the query is unsettled, and every other block whose bound does not exceed U0
        // (>= U(q): a superset of the two passes' lists, and keys meet by atomicMin).  Lane =
        // template block; the bounds are re-read (this wave's lanes hold no complete copy of
        // them past one chunk): the thread block's own stores, behind the chunk loop's last
        // barrier, or the prefilter launch's.  One atomic per listed (tb, q), none elsewhere.
        for (int tb = lane; tb < ntb; tb += 64) {
            const bool in = tb == tbs ? !settled : (tb < 64 ? mlb0 : minlb[(size_t)tb * nq + q]) <= u0;
            if (in) {
                const unsigned p = atomicAdd(fl.cnt + tb, 1u);
                if (p < (unsigned)nq) fl.list[(size_t)tb * nq + p] = q;   // (always: a query joins a list once)
            }
        }
    }
    if (lane == 0) {
        if (settled) {
            const unsigned long long g = ((unsigned long long)tbs * 64 + tl) * nranks + rank;
            atomicMin(best + q, ((unsigned long long)u0 << 32) | g);
            if (fl.cnt) fl.ublk[q] = u0;
        }
        tbstar[q] = settled ? ~tbs : tbs;
    }
}

__global__ __launch_bounds__(64) void vt_prune_verify_kernel(const uint32_t* __restrict__ minlb,
                                                             const uint32_t* __restrict__ second, int ntb, int nq,
                                                             const uint4* __restrict__ planes,
                                                             const uint32_t* __restrict__ tsum,
                                                             const uint4* __restrict__ qc4,
                                                             uint4* __restrict__ qp4,
                                                             const uint32_t* __restrict__ qsum,
                                                             unsigned long long* __restrict__ best, int rank,
                                                             int nranks, int* __restrict__ tbstar,
                                                             FrontLists fl) {
    __shared__ uint4 s_q[VT_VQS];
    __shared__ uint4 s_t[VT_VTS];
    const int q = blockIdx.x, lane = threadIdx.x;
    vt_verify_query<false>(q, lane, [&](unsigned long long& pk, uint32_t& sec, uint32_t& m2) {
        for (int tb = lane; tb < ntb; tb += 64) {
            const unsigned long long k = ((unsigned long long)minlb[(size_t)tb * nq + q] << 32) | (unsigned)tb;
            const uint32_t s2 = second[(size_t)tb * nq + q];
            const bool lt = k < pk;   // (selects: a branch would put the second read behind the first)
            m2 = min(m2, (uint32_t)((lt ? pk : k) >> 32));
            pk = lt ? k : pk;
            sec = lt ? s2 : sec;
        }
    }, nq, planes, tsum, qc4, qp4, qsum, best, rank, nranks, tbstar, s_q, s_t, minlb, ntb, fl);
}

// The front of a pruned call in one launch (vt_plan::front_fused): a thread block owns
// query groups of PF_NB queries (blockIdx.y, strided) and, for each, walks ALL template
// blocks in chunks of PF_WAVES * PF_TPW (wave w: blocks c0 + w * PF_TPW ...), writes
// minlb[] as the prefilter does (vt_prune_rest_kernel reads it) and leaves each
// (bound, second) of the chunk in LDS; after the chunk's barrier wave w folds the chunk
// into query w's pick, lane l the chunk's block l -- per lane the very update of the
// verify kernel's pick loop, only with the blocks dealt 16 to a chunk instead of 64 to a
// stride, and the wave-wide reductions that follow are associative.  Then wave w verifies
// query w (vt_verify_query) on its own: s_vq[w] and s_vt[w] are no other wave's, so the tail
// has no block barrier, no wave waits for the slowest one's template round trip, and a wave
// without a query (w >= nb, the last group) skips it.  second[] is not written.
// Barriers: every one is reached by all PF_WAVES waves -- the chunk loop's bounds are
// block-uniform and a wave without a template block skips the walk only (no barrier
// inside).  s_pick is double-buffered by chunk parity: with one barrier
// per chunk a wave is at most one chunk ahead of a wave still folding.
__global__ __launch_bounds__(64 * PF_WAVES) __attribute__((amdgpu_waves_per_eu(4)))
void vt_front_kernel(const uint4* __restrict__ planes, int ntb, int64_t count, const uint4* __restrict__ qc4,
                     const uint32_t* __restrict__ qsj, int nq, uint32_t* __restrict__ minlb,
                     const uint32_t* __restrict__ tsum, uint4* __restrict__ qp4,
                     const uint32_t* __restrict__ qsum, unsigned long long* __restrict__ best, int rank,
                     int nranks, int* __restrict__ tbstar, FrontLists fl) {
    front_zero(fl);
    constexpr int CH = PF_WAVES * PF_TPW;
    static_assert(PF_WAVES == PF_NB, "one wave per query of the group in the tail");
    static_assert(CH <= 64, "one lane per block of a chunk");
    __shared__ uint4 s_q[PF_NB][PF_NU][PF_CGS][PL_NO][2];
    __shared__ uint32_t s_qs[PF_NB][PF_NU][16];
    __shared__ uint2 s_pick[2][PF_NB][CH];   // (minlb, second) of the chunk's blocks
    __shared__ uint4 s_vq[PF_WAVES][VT_VQS];
    __shared__ uint4 s_vt[PF_WAVES][VT_VTS];
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    int par = 0;
    for (int q0 = blockIdx.y * PF_NB; q0 < nq; q0 += gridDim.y * PF_NB) {   // block-uniform
        const int nb = min(PF_NB, nq - q0);
        const int qw = min(wave, nb - 1);   // the query this wave picks for (and verifies, if wave < nb)
        __syncthreads();   // the group before has been read
        pf_stage(qc4, qsj, q0, nb, s_q, s_qs);
        __syncthreads();
        unsigned long long pk = ~0ull;
        uint32_t sec = 0u, m2 = 0xFFFFFFFFu;
        for (int c0 = 0; c0 < ntb; c0 += CH) {   // block-uniform
            const int tb0 = c0 + wave * PF_TPW;
            if (tb0 < ntb) {   // wave-uniform; no barrier inside
                // (loaded per chunk and dead in the tail: the verification has the VGPRs)
                uint32_t P[PF_TPW][PF_NU][PF_CGS][8], tsb[PF_TPW];
                bool valid[PF_TPW];
                pf_load(planes, ntb, count, tb0, lane, P, tsb, valid);
#pragma unroll 1
                for (int qq = 0; qq < nb; ++qq) {
                    uint32_t v[PF_TPW], w[PF_TPW];
                    pf_walk(P, tsb, valid, s_q[qq], s_qs[qq], lane, v, w);
                    if (lane == 0) {
#pragma unroll
                        for (int t = 0; t < PF_TPW; ++t)
                            if (tb0 + t < ntb) {
                                minlb[(size_t)(tb0 + t) * nq + q0 + qq] = v[t] >> 6;
                                s_pick[par][qq][wave * PF_TPW + t] = make_uint2(v[t] >> 6, (w[t] << 6) | (v[t] & 63u));
                            }
                    }
                }
            }
            __syncthreads();
            if (lane < CH && c0 + lane < ntb) {
                const uint2 e = s_pick[par][qw][lane];
                const unsigned long long k = ((unsigned long long)e.x << 32) | (unsigned)(c0 + lane);
                const bool lt = k < pk;
                m2 = min(m2, (uint32_t)((lt ? pk : k) >> 32));
                pk = lt ? k : pk;
                sec = lt ? e.y : sec;
            }
            par ^= 1;
        }
        // (the tail's lane arithmetic is loop-invariant: hoisted above the group loop it
        // would stay live through the walk, in scratch)
        int vl = lane;
        asm volatile("" : "+v"(vl));
        if (wave < nb)   // (wave-uniform; no barrier inside)
            vt_verify_query<true>(q0 + wave, vl, [&](unsigned long long& pk_, uint32_t& sec_, uint32_t& m2_) {
                pk_ = pk;
                sec_ = sec;
                m2_ = m2;
            }, nq, planes, tsum, qc4, qp4, qsum, best, rank, nranks, tbstar, s_vq[wave], s_vt[wave], minlb, ntb, fl);
    }
}

// ... and list1[tb] = the unsettled queries whose candidate block is tb (blockIdx.y =
// tb).  The thread blocks of tb = 0 also count the settled queries (one add each).
// The first thread block zeroes cnt2[]: the B2 pass of the call before has read it, this
// call's vt_prune_rest_kernel fills it, and rs_vt_prune_stats totals it in between.
__global__ __launch_bounds__(VT_LIST_T) void vt_prune_first_kernel(int nq, const int* __restrict__ tbstar,
                                                                   unsigned* __restrict__ cnt,
                                                                   int* __restrict__ list,
                                                                   unsigned* __restrict__ verified,
                                                                   unsigned* __restrict__ cnt2, int ntb) {
    const int q = blockIdx.x * VT_LIST_T + threadIdx.x, tb = blockIdx.y;
    const int ts = q < nq ? tbstar[q] : INT_MAX;
    if (blockIdx.x == 0 && tb == 0)
        for (int b = threadIdx.x; b < ntb; b += VT_LIST_T) cnt2[b] = 0u;
    if (tb == 0) {   // (block-uniform)
        const int n = __syncthreads_count(ts < 0);
        if (threadIdx.x == 0 && n) atomicAdd(verified, (unsigned)n);
    }
    list_append(ts == tb, q, cnt + tb, list + (size_t)tb * nq);
}

// List (b), after pass B1: q joins the list of every other block whose bound does not
// exceed U(q) = the score B1 left in best[q].
// The first thread block also closes list (a), which pass B1 has read: stat[0] = the
// queries pass B1 settled, by verification or by block scan, stat[2] = the verified ones
// alone (rs_vt_prune_stats; the pairs of B2 are the sum of cnt[], taken on the host), and
// cnt1[] and the verified count back to zero for the next call.
__global__ __launch_bounds__(VT_LIST_T) void vt_prune_rest_kernel(const uint32_t* __restrict__ minlb, int nq,
                                                                  const int* __restrict__ tbstar,
                                                                  const unsigned long long* __restrict__ best,
                                                                  unsigned* __restrict__ cnt,
                                                                  int* __restrict__ list,
                                                                  unsigned* __restrict__ cnt1,
                                                                  unsigned* __restrict__ verified, int ntb,
                                                                  unsigned long long* __restrict__ stat) {
    const int q = blockIdx.x * VT_LIST_T + threadIdx.x, tb = blockIdx.y;
    const int ts = q < nq ? tbstar[q] : 0;   // ~tb* where the verification settled the query
    const bool in = q < nq && tb != (ts < 0 ? ~ts : ts) && minlb[(size_t)tb * nq + q] <= (uint32_t)(best[q] >> 32);
    list_append(in, q, cnt + tb, list + (size_t)tb * nq);
    if (blockIdx.x == 0 && tb == 0) {   // (block-uniform)
        __shared__ unsigned long long s_sum;
        if (threadIdx.x == 0) s_sum = 0ull;
        __syncthreads();
        unsigned long long a = 0ull;
        for (int b = threadIdx.x; b < ntb; b += VT_LIST_T) {
            a += cnt1[b];
            cnt1[b] = 0u;
        }
        if (a) atomicAdd(&s_sum, a);
        __syncthreads();
        if (threadIdx.x == 0) {
            const unsigned v = *verified;
            *verified = 0u;
            stat[0] = s_sum + v;
            stat[2] = v;
        }
    }
}

// rs_vt_prune_stats after a single list pass: the two-pass rule's counts, from what the
// call left.  vt_prune_rest_kernel's predicate, counted instead of listed: acc[0] += the
// pairs (tb, q) with tb != tb* and minlb[tb][q] <= ublk[q] (ublk[q] = U(q): U0 of a settled
// query, the candidate block's minimum of the others), acc[1] += the settled marks in tbstar.
__global__ __launch_bounds__(256) void vt_prune_count_kernel(const uint32_t* __restrict__ minlb, int nq, int ntb,
                                                             const int* __restrict__ tbstar,
                                                             const uint32_t* __restrict__ ublk,
                                                             unsigned long long* __restrict__ acc) {
    __shared__ unsigned s_acc[2];
    if (threadIdx.x < 2) s_acc[threadIdx.x] = 0u;
    __syncthreads();
    const int q = blockIdx.x * 256 + threadIdx.x;
    if (q < nq) {
        const int ts = tbstar[q], tbs = ts < 0 ? ~ts : ts;
        const uint32_t u = ublk[q];
        unsigned n = 0u;
        for (int tb = 0; tb < ntb; ++tb) n += tb != tbs && minlb[(size_t)tb * nq + q] <= u;
        if (n) atomicAdd(&s_acc[0], n);
        if (ts < 0) atomicAdd(&s_acc[1], 1u);
    }
    __syncthreads();
    if (threadIdx.x < 2 && s_acc[threadIdx.x]) atomicAdd(acc + threadIdx.x, (unsigned long long)s_acc[threadIdx.x]);
}

// The batch's first-argmin keys -> the pinned host buffer (system-scope stores),
// and the device keys reset to UINT64_MAX for the next scan: one queued launch in
// place of a device-to-host blit copy and a memset before the next scan.
__global__ __launch_bounds__(256) void vt_keys_export(unsigned long long* __restrict__ keys, int n,
                                                      unsigned long long* host) {
    for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
        __hip_atomic_store(host + i, keys[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        keys[i] = ~0ull;
    }
}
