// The row-offset profile of matched (query, template) pairs (rs_vt_offset_profile, DESIGN
// section 30), included by view_templates.hip.  The rule is vt_offset_rule.h:
//
//   profile[i][k] = sum_{r=M..H-M-1, c} term(T_i[r + k - (M-1)][c], Q_i[r][c]),  k = 0 .. 2M-2
//   offset[i]     = (first k with profile[i][k] minimal) - (M - 1)
//
// for T_i = template index[i] of the library, read in the byte layout every handle keeps
// (chunk (tb, c, q, t) of view_templates.hip: rows 4q..4q+3 of dword column c of slot
// tb*64 + t, padding bytes zero), and Q_i = raw query i (H x W bytes, row-major).
//
// One wave per pair.  Its lanes stride over the (window row, dword column) items, column
// fastest, so a wave's query bytes are consecutive; the query dword is put together from byte
// reads (a raw row is not dword-aligned when W mod 4 != 0, and no address outside the query
// is formed; bytes past W stay zero like the library's).  A template dword is one 4-byte
// read of a chunk: the work is (H - 2M) * WD * (2M - 1) v_sad_u8 a pair, a few hundred
// cycles of arithmetic behind one round of memory latency, so nothing is staged in LDS.
//   FAST (max_offset 8): 2M - 1 = 15 accumulators in registers, a query dword read once;
//   generic (any max_offset): the offset loop outermost, one accumulator.
// Both sum across the wave by shuffles and write with plain vector stores, no atomics.
// index[i] == -1 (or, defensively, outside [0, count)): a row of UINT32_MAX and offset 0,
// no template read.
// (view_templates.hip includes vt_offset_rule.h at file scope, ahead of its own namespace.)
#pragma once

__device__ inline uint32_t vto_wave_sum(uint32_t v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

template <int METRIC, bool FAST>
__global__ __launch_bounds__(64) void vt_offset_profile_kernel(const uint4* __restrict__ lib, int64_t count,
                                                               int H, int W, int WD, int HQ, int M_,
                                                               const uint8_t* __restrict__ queries,
                                                               const int64_t* __restrict__ index,
                                                               uint32_t* __restrict__ profile,
                                                               int32_t* __restrict__ offset) {
    const int M = FAST ? FAST_M : M_;
    const int NO = 2 * M - 1;
    const int qi = blockIdx.x, lane = threadIdx.x;
    uint32_t* const prow = profile + (size_t)qi * NO;
    const int64_t g = index[qi];
    if (g < 0 || g >= count) {
        for (int k = lane; k < NO; k += 64) prow[k] = 0xFFFFFFFFu;
        if (lane == 0) offset[qi] = 0;
        return;
    }
    // dword (row s, dword column c) of slot g: tpl[((c * HQ + (s >> 2)) * 64) * 4 + (s & 3)];
    // s = r + o lies in [1, H - 2] for every window row r and offset o
    const uint32_t* const tpl =
        reinterpret_cast<const uint32_t*>(lib) + ((size_t)(g >> 6) * WD * HQ * 64 + (size_t)(g & 63)) * 4;
    const uint8_t* const q = queries + (size_t)qi * H * W;
    const int items = (H - 2 * M) * WD;
    uint32_t best = 0;
    int best_k = 0;
    if constexpr (FAST) {
        constexpr int NO8 = 2 * FAST_M - 1;
        uint32_t acc[NO8];
#pragma unroll
        for (int k = 0; k < NO8; ++k) acc[k] = 0u;
        for (int it = lane; it < items; it += 64) {
            const int rr = it / WD, c = it - rr * WD, r = FAST_M + rr;
            const uint32_t qd = rs::vto_row_dword(q + (size_t)r * W, W, c);
            const uint32_t* const col = tpl + (size_t)c * HQ * 256;
#pragma unroll
            for (int k = 0; k < NO8; ++k) {
                const int s = r + k - (FAST_M - 1);
                acc[k] = rs::vto_term<METRIC>(col[(size_t)(s >> 2) * 256 + (s & 3)], qd, acc[k]);
            }
        }
#pragma unroll
        for (int k = 0; k < NO8; ++k) {
            acc[k] = vto_wave_sum(acc[k]);
            rs::vto_pick(acc[k], k, best, best_k);
            if (lane == k) prow[k] = acc[k];
        }
    } else {
        for (int k = 0; k < NO; ++k) {
            uint32_t acc = 0u;
            for (int it = lane; it < items; it += 64) {
                const int rr = it / WD, c = it - rr * WD, r = M + rr;
                const int s = r + k - (M - 1);
                const uint32_t qd = rs::vto_row_dword(q + (size_t)r * W, W, c);
                acc = rs::vto_term<METRIC>(tpl[((size_t)c * HQ + (s >> 2)) * 256 + (s & 3)], qd, acc);
            }
            acc = vto_wave_sum(acc);
            rs::vto_pick(acc, k, best, best_k);
            if (lane == 0) prow[k] = acc;
        }
    }
    if (lane == 0) offset[qi] = best_k - (M - 1);
}
