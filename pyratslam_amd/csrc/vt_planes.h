// The bit-plane layout of the wrapped metric: its constants, the template-plane store and
// the query-plane builds (full, compact, and one from the other).
// Part of view_templates.hip, the one translation unit: not free-standing (it relies on the
// includes, the anonymous namespace and the headers that view_templates.hip includes before it).
#pragma once

// ===========================================================================
// Bit-plane scan (default for W = 32, H in {32, 64}, max_offset 8).
//
// (T - Q) mod 256 = T - Q + 256 [T < Q], so a score is
//   score(o) = TS(o) - QS + 256 * B(o),
// TS(o) = the template's byte sum over rows [M+o, H-M+o) (stored with the
// template), QS = the query's byte sum over rows [M, H-M), and B(o) = the number
// of byte pairs with T < Q.  B is counted bit-sliced: a unit of 4 rows x 8
// columns (32 bytes) is stored as 8 bit planes (plane k, bit i = bit k of byte
// i), and [T < Q] for all 32 pairs of a unit is the borrow out of T - Q,
//   b = maj(~T_k, Q_k, b)  for k = 0..7   (one v_bitop3_b32 each, table 0x8E),
// followed by one v_bcnt_u32_b32 into the offset's counter: 9 VALU per
// 32 byte pairs, against 3 per 4 pairs for the byte-SWAR forms above.
//
// Template planes: uint4 chunk ((((tb*CG + cg)*NU + j)*2 + g)*64 + t) holds
// planes 4g..4g+3 of unit j (rows 4j..4j+3, columns 8cg..8cg+7) of slot
// tb*64 + t.  TS: tsum[(tb*16 + o+M-1)*64 + t].
// Query planes: for every start row s in [M-3, H-M-1] and column group cg, the
// unit of rows s..s+3 with rows outside [M, H-M) zeroed (a zero byte never
// borrows), qp[((q*CG + cg)*NS + s-(M-3))*8 + k]; qsum[q] = QS (raw bytes).
//
// A block is CG waves (one per column group) x 64 templates.  Wave cg keeps
// its NU units x 8 planes in VGPRs and streams query planes through SGPRs
// (wave-uniform scalar loads).  Template unit j meets query unit s at offset
// o = 4j - s.  The CG partial counts per (query, offset, template) meet in LDS.
// ===========================================================================
constexpr int PL_CG = 4;       // column groups of 8 bytes: W = 32

constexpr int PL_NB = 4;  // queries per LDS batch (staged planes; one reducing wave each)

// Pruned plane scan (H = 64): the prefilter bounds every score from below by its
// exact partial sum over PF_NU template units (4 rows x 32 columns each).  A unit J
// with 4J-(M-1) >= M and 4J+M+2 <= H-M-1 (J in [4, 11]) meets only query rows inside
// the window at every offset.  One unit (J = 7) or two (J = 5 and 10).
#ifndef VT_PF_UNITS
#define VT_PF_UNITS 1
#endif
constexpr int PF_NU = VT_PF_UNITS;
static_assert(PF_NU == 1 || PF_NU == 2, "one or two prefilter units");
__host__ __device__ constexpr int pf_unit(int u) { return PF_NU == 1 ? 7 : (u == 0 ? 5 : 10); }
static_assert(4 * pf_unit(0) - (FAST_M - 1) >= FAST_M && 4 * pf_unit(PF_NU - 1) + FAST_M + 2 <= 64 - FAST_M - 1,
              "the units' query rows lie inside the window at every offset");
// The bound is taken over column groups 0 .. PF_CGS-1 of a unit only (columns 0 .. 8*PF_CGS-1
// of its 4 rows): any subset of a score's byte pairs sums to a lower bound of it, and half
// a unit (64 pairs) still separates a hit's bound from every other template's by a wide
// margin.  4 = the whole unit.
#ifndef VT_PF_CGS
#define VT_PF_CGS 2
#endif
constexpr int PF_CGS = VT_PF_CGS;

// One block per stored template: planes + TS of raw template src[t] into slot dst[t].
__global__ __launch_bounds__(256) void vt_plane_store_kernel(const uint8_t* __restrict__ raw,
                                                             const int32_t* __restrict__ src,
                                                             const int64_t* __restrict__ dst,
                                                             int H, int M,
                                                             uint32_t* __restrict__ planes,
                                                             uint32_t* __restrict__ tsum) {
    constexpr int W = 8 * PL_CG;
    __shared__ uint32_t s_row[256];
    const uint8_t* T = raw + (size_t)src[blockIdx.x] * H * W;
    const int64_t slot = dst[blockIdx.x];
    const int64_t tb = slot >> 6, tl = slot & 63;
    const int NU = H / 4, wave = threadIdx.x >> 6, lane = threadIdx.x & 63, i = lane & 31;
    for (int u0 = 2 * wave; u0 < PL_CG * NU; u0 += 8) {
        const int u = u0 + (lane >> 5);
        const int cg = u / NU, j = u - cg * NU;
        const uint32_t byte = u < PL_CG * NU ? T[(size_t)(4 * j + (i >> 3)) * W + 8 * cg + (i & 7)] : 0u;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const unsigned long long m = __ballot((byte >> k) & 1u);
            if (i == k && u < PL_CG * NU)
                planes[((((tb * PL_CG + cg) * NU + j) * 2 + (k >> 2)) * 64 + tl) * 4 + (k & 3)] =
                    (uint32_t)(lane < 32 ? m : m >> 32);
        }
    }
    for (int r = threadIdx.x; r < H; r += blockDim.x) {
        uint32_t acc = 0;
        const uint32_t* row = reinterpret_cast<const uint32_t*>(T + (size_t)r * W);
#pragma unroll
        for (int d = 0; d < W / 4; ++d) acc = __builtin_amdgcn_sad_u8(row[d], 0u, acc);
        s_row[r] = acc;
    }
    __syncthreads();
    if (threadIdx.x < 16) {
        const int o = (int)threadIdx.x - (M - 1);
        uint32_t ts = 0;
        if (threadIdx.x < 2 * M - 1)
            for (int r = M + o; r < H - M + o; ++r) ts += s_row[r];
        tsum[(tb * 16 + threadIdx.x) * 64 + tl] = ts;
    }
}

// 8x8 bit-matrix transpose of 8 bytes held as (lo = bytes 0-3, hi = bytes 4-7):
// bit c of byte r  ->  bit r of byte c (three delta swaps, Hacker's Delight 7-3).
__device__ inline void transpose8x8(uint32_t& lo, uint32_t& hi) {
    uint32_t t;
    t = (lo ^ (lo >> 7)) & 0x00AA00AAu;   lo ^= t ^ (t << 7);
    t = (hi ^ (hi >> 7)) & 0x00AA00AAu;   hi ^= t ^ (t << 7);
    t = (lo ^ (lo >> 14)) & 0x0000CCCCu;  lo ^= t ^ (t << 14);
    t = (hi ^ (hi >> 14)) & 0x0000CCCCu;  hi ^= t ^ (t << 14);
    t = (lo ^ (hi << 4)) & 0xF0F0F0F0u;   lo ^= t;  hi ^= t >> 4;
}

// 4x4 byte transpose: out[k] byte q = byte k of in[q].
__device__ inline void transpose4x4_bytes(uint32_t a, uint32_t b, uint32_t c, uint32_t d,
                                          uint32_t (&o)[4]) {
    // pairs: (a,b) -> byte k of a, byte k of b interleaved; likewise (c,d)
    const uint32_t ab_lo = __builtin_amdgcn_perm(b, a, 0x05010400u);  // a0 b0 a1 b1
    const uint32_t ab_hi = __builtin_amdgcn_perm(b, a, 0x07030602u);  // a2 b2 a3 b3
    const uint32_t cd_lo = __builtin_amdgcn_perm(d, c, 0x05010400u);  // c0 d0 c1 d1
    const uint32_t cd_hi = __builtin_amdgcn_perm(d, c, 0x07030602u);  // c2 d2 c3 d3
    o[0] = __builtin_amdgcn_perm(cd_lo, ab_lo, 0x05040100u);          // a0 b0 c0 d0
    o[1] = __builtin_amdgcn_perm(cd_lo, ab_lo, 0x07060302u);          // a1 b1 c1 d1
    o[2] = __builtin_amdgcn_perm(cd_hi, ab_hi, 0x05040100u);
    o[3] = __builtin_amdgcn_perm(cd_hi, ab_hi, 0x07060302u);
}

// Compact query planes (H = 64): the units of the aligned start rows S0 + 4i, i < QC_NA
// (rows 5, 9, .., 53).  Bit b of a plane is pixel (S + b/8, b%8), so the unit of start
// row S + r, r in 0..3, is the low word of (unit(S + 4) : unit(S)) >> 8r, plane by plane;
// the unit past the last (start row 57: rows 57..60, all zeroed) is zero.
constexpr int QC_NA = (64 - 2 * FAST_M + 3 + 3) / 4;   // 13
constexpr int QC_Q4 = PL_CG * QC_NA * 2;                // uint4 per query
static_assert((FAST_M - 3) + 4 * QC_NA >= 64 - FAST_M, "the unit past the last aligned one is all zero");
__device__ __forceinline__ uint4 qc_shift(uint4 lo, uint4 hi, uint32_t sh) {
    return make_uint4(__builtin_amdgcn_alignbit(hi.x, lo.x, sh), __builtin_amdgcn_alignbit(hi.y, lo.y, sh),
                      __builtin_amdgcn_alignbit(hi.z, lo.z, sh), __builtin_amdgcn_alignbit(hi.w, lo.w, sh));
}
// chunk c (of two) of the unit of start row S0 + si, column group cg, from a query's
// compact planes in global memory
__device__ __forceinline__ uint4 qc_unit(const uint4* __restrict__ qcq, int cg, int si, int c) {
    const int ia = si >> 2;
    const uint4 lo = qcq[(cg * QC_NA + ia) * 2 + c];
    const uint4 hi = ia + 1 < QC_NA ? qcq[(cg * QC_NA + ia + 1) * 2 + c] : make_uint4(0u, 0u, 0u, 0u);
    return qc_shift(lo, hi, 8u * (uint32_t)(si & 3));
}

// Every start row of queries [0, nq) from their compact planes: for the consumers that
// read all queries' planes after a compact build (a matrix or dense scan).
__global__ __launch_bounds__(256) void vt_qexpand_kernel(const uint4* __restrict__ qc4, uint4* __restrict__ qp4) {
    constexpr int NS = 64 - 2 * FAST_M + 3;
    const uint4* qcq = qc4 + (size_t)blockIdx.x * QC_Q4;
    for (int i = threadIdx.x; i < PL_CG * NS * 2; i += blockDim.x) {
        const int cg = i / (NS * 2), r = i - cg * (NS * 2);
        qp4[(size_t)blockIdx.x * (PL_CG * NS * 2) + i] = qc_unit(qcq, cg, r >> 1, r & 1);
    }
}
// ... and the compact planes from the full ones (a pruned scan after a full build).
__global__ __launch_bounds__(128) void vt_qcompact_kernel(const uint4* __restrict__ qp4, uint4* __restrict__ qc4) {
    constexpr int NS = 64 - 2 * FAST_M + 3;
    const int i = threadIdx.x;
    if (i < QC_Q4) {
        const int cg = i / (QC_NA * 2), r = i - cg * (QC_NA * 2);
        qc4[(size_t)blockIdx.x * QC_Q4 + i] = qp4[(size_t)blockIdx.x * (PL_CG * NS * 2) + (cg * NS + 4 * (r >> 1)) * 2 + (r & 1)];
    }
}

// One block per query: query planes for every start row, and QS.  Phase 1: each
// thread bit-transposes one 8-byte row segment (row r, column group cg) so byte
// k holds bit k of its 8 pixels (rows outside [M, H-M) become zero), and adds
// the segment to QS.  Phase 2: each thread assembles one unit (4 rows from start
// row S0 + si, column group cg): plane k = byte k of its 4 segments, two 16-byte
// stores.  Bit b of plane k = bit k of pixel (row + b/8, col 8cg + b%8).
// With a prune buffer (qsj, H = 64): also QS_J(S), the byte sum of columns
// 0 .. 8*PF_CGS-1 of rows S..S+3 (the pairs the prefilter's bound covers), for
// the start rows S = 4J+7-x, x = 0..2M-2, that prefilter unit J meets
// (qsj[(query * PF_NU + u) * 16 + x]).
// Compact mode (qc, H = 64, ahead of a pruned scan): phase 2 assembles only the QC_NA
// aligned start rows S0 + 4i into qc[((q*CG + cg)*QC_NA + i)*8 + k] and leaves qp alone.
// Every other start row is a funnel shift of two aligned units (qc_shift); the pruned
// scan's kernels read these, and expand into qp the queries a scan pass will stage.
__global__ __launch_bounds__(256) void vt_qplane_kernel(const uint8_t* __restrict__ raw, int H,
                                                        int M, uint32_t* __restrict__ qp,
                                                        uint32_t* __restrict__ qsum,
                                                        uint8_t* __restrict__ raw_copy,
                                                        uint32_t* __restrict__ qsj,
                                                        uint32_t* __restrict__ qc) {
    constexpr int W = 8 * PL_CG;
    __shared__ uint32_t s_red[4];
    __shared__ uint2 s_t[64 * W / 8];   // transposed segments (H <= 64)
    __shared__ uint32_t s_rs[64];       // byte sums of the rows' first PF_CGS column groups (prune buffer only)
    if (threadIdx.x < 4) s_red[threadIdx.x] = 0u;   // (a block may be fewer than four waves)
    if (qsj) {   // (kernel argument: uniform)
        if (threadIdx.x < 64) s_rs[threadIdx.x] = 0u;
        __syncthreads();
    }
    // (compact: the aligned start rows only, NS of them at stride 4)
    const int NS = qc ? QC_NA : H - 2 * M + 3, S0 = M - 3, SS = qc ? 4 : 1;
    const uint8_t* Q = raw + (size_t)blockIdx.x * H * W;
    uint32_t* out = (qc ? qc : qp) + (size_t)blockIdx.x * PL_CG * NS * 8;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    uint32_t part = 0;
    for (int d = threadIdx.x; d < H * W / 8; d += blockDim.x) {
        uint2 v = reinterpret_cast<const uint2*>(Q)[d];
        // raw read in place from pinned host memory: its bytes also into the device copy
        if (raw_copy) reinterpret_cast<uint2*>(raw_copy + (size_t)blockIdx.x * H * W)[d] = v;
        const int r = d / (W / 8);
        const bool live = r >= M && r < H - M;
        if (live) part = __builtin_amdgcn_sad_u8(v.y, 0u, __builtin_amdgcn_sad_u8(v.x, 0u, part));
        // (d = row * PL_CG + column group: only the groups the prefilter's bound covers)
        if (qsj && d % PL_CG < PF_CGS)
            atomicAdd(&s_rs[r], __builtin_amdgcn_sad_u8(v.y, 0u, __builtin_amdgcn_sad_u8(v.x, 0u, 0u)));
        transpose8x8(v.x, v.y);
        s_t[d] = live ? v : make_uint2(0u, 0u);
    }
    __syncthreads();
    const int NU = PL_CG * NS;
    for (int u = threadIdx.x; u < NU; u += blockDim.x) {
        const int cg = u / NS, r0 = S0 + SS * (u - cg * NS);
        const uint2 q0 = s_t[(r0 + 0) * PL_CG + cg], q1 = s_t[(r0 + 1) * PL_CG + cg];
        const uint2 q2 = s_t[(r0 + 2) * PL_CG + cg], q3 = s_t[(r0 + 3) * PL_CG + cg];
        uint32_t lo[4], hi[4];
        transpose4x4_bytes(q0.x, q1.x, q2.x, q3.x, lo);
        transpose4x4_bytes(q0.y, q1.y, q2.y, q3.y, hi);
        uint4* o = reinterpret_cast<uint4*>(out + (size_t)u * 8);
        o[0] = make_uint4(lo[0], lo[1], lo[2], lo[3]);
        o[1] = make_uint4(hi[0], hi[1], hi[2], hi[3]);
    }
    if (qsj && threadIdx.x < PF_NU * 16) {
        const int u = threadIdx.x >> 4, x = threadIdx.x & 15;
        const int S = 4 * pf_unit(u) + M - 1 - min(x, 2 * M - 2);
        qsj[((size_t)blockIdx.x * PF_NU + u) * 16 + x] = s_rs[S] + s_rs[S + 1] + s_rs[S + 2] + s_rs[S + 3];
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) part += __shfl_xor(part, off);
    if (lane == 0) s_red[wave] = part;
    __syncthreads();
    if (threadIdx.x == 0) qsum[blockIdx.x] = s_red[0] + s_red[1] + s_red[2] + s_red[3];
}
