// The byte-SWAR scans of the wrapped metric: the carry-count forms (max_offset 8) and the
// generic form (any H, max_offset).
// Part of view_templates.hip, the one translation unit: not free-standing (it relies on the
// includes, the anonymous namespace and the headers that view_templates.hip includes before it).
#pragma once

// --- carry-count forms.  v_sad_u8 issues at half rate on gfx950 (measured,
// tools/ubench_valu.hip), so the byte sum is taken apart exactly:
//   sum_b (a_b + c_b) mod 256 = bytesum(a) + bytesum(c) - 256 * #carries,
// with the carry out of byte b = majority(a_b7, c_b7, bit 7 of (a&0x7f + c&0x7f)_b):
// one v_bitop3 (table 0xE8; zero outside bit 7 since aH, cH are), counted by
// v_bcnt_u32_b32.  Per pair: v_add_u32 + v_bitop3_b32 + v_bcnt_u32_b32, all full
// rate.  bytesum(a) over each offset's row window is a sliding sum per column
// (query-independent), bytesum(c) is qsum[] from vt_qform_kernel.
__device__ inline uint32_t carry_pair(uint32_t aL, uint32_t aH, uint2 f, uint32_t cnt) {
    return __builtin_popcount(__builtin_amdgcn_bitop3_b32(aH, f.y, aL + f.x, 0xE8)) + cnt;
}

template <int H, int NQ, bool MATRIX>
__global__ __launch_bounds__(64) void vt_scan_carry_kernel(const uint4* __restrict__ lib, int ntb,
                                                           int64_t count, int WD,
                                                           const uint2* __restrict__ qf,
                                                           const uint32_t* __restrict__ qsum,
                                                           int nq, ScanOut out, int rank,
                                                           int nranks) {
    constexpr int M = FAST_M, HQ = (H + 3) / 4, NO = 2 * M - 1, R0 = M, R1 = H - M;
    // XCD-aware mapping (speed only): blocks b and b+8 are dealt to the same XCD, so
    // XCD x takes query groups qg = x (mod 8) against the whole library -- its L2
    // holds the library plus 1/8 of the query forms.
    const int j = blockIdx.x >> 3;
    const int tb = j % ntb;
    const int qg = (j / ntb) * 8 + (blockIdx.x & 7);
    if (qg * NQ >= nq) return;
    const int qbase = qg * NQ;
    const int lane = threadIdx.x;
    uint32_t cnt[NQ][NO];
    uint32_t A[NO];
#pragma unroll
    for (int o = 0; o < NO; ++o) {
        A[o] = 0u;
#pragma unroll
        for (int n = 0; n < NQ; ++n) cnt[n][o] = 0u;
    }
    for (int c = 0; c < WD; ++c) {
        const uint4* col = lib + ((size_t)(tb * WD + c) * HQ) * 64 + lane;
        uint32_t aL[4 * HQ], aH[4 * HQ], bs[4 * HQ];
#pragma unroll
        for (int q = 0; q < HQ; ++q) {
            const uint4 v = col[(size_t)q * 64];
            const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                aL[4 * q + k] = w[k] & 0x7F7F7F7Fu;
                aH[4 * q + k] = w[k] & 0x80808080u;
                bs[4 * q + k] = __builtin_amdgcn_sad_u8(w[k], 0u, 0u);
            }
        }
        uint32_t win = 0u;
#pragma unroll
        for (int s = R0 - (M - 1); s < R1 - (M - 1); ++s) win += bs[s];
        A[0] += win;
#pragma unroll
        for (int o = 1; o < NO; ++o) {
            win += bs[R1 - (M - 1) + o - 1] - bs[R0 - (M - 1) + o - 1];
            A[o] += win;
        }
#pragma unroll
        for (int r = R0; r < R1; ++r) {
#pragma unroll
            for (int n = 0; n < NQ; ++n) {
                const int qi = min(qbase + n, nq - 1);
                const uint2 f = qf[((size_t)qi * WD + c) * H + r];
#pragma unroll
                for (int o = 0; o < NO; ++o) {
                    const int s = r + o - (M - 1);
                    cnt[n][o] = carry_pair(aL[s], aH[s], f, cnt[n][o]);
                }
            }
        }
    }
    const int64_t slot = (int64_t)tb * 64 + lane;
#pragma unroll
    for (int n = 0; n < NQ; ++n) {
        const uint32_t qs = qsum[min(qbase + n, nq - 1)];
        uint32_t sc = 0xFFFFFFFFu;
#pragma unroll
        for (int o = 0; o < NO; ++o) sc = min(sc, A[o] + qs - 256u * cnt[n][o]);
        emit_score<MATRIX>(out, slot, count, qbase + n, nq, sc, rank, nranks, lane == 0);
    }
}

template <int H, int NQ>
__global__ __launch_bounds__(64) void vt_scan_carry_col_kernel(const uint4* __restrict__ lib,
                                                               int64_t count, int WD,
                                                               const uint2* __restrict__ qf,
                                                               const uint32_t* __restrict__ qsum,
                                                               int nq, ScanOut out, int rank,
                                                               int nranks) {
    constexpr int M = FAST_M, HQ = (H + 3) / 4, NO = 2 * M - 1, R0 = M, R1 = H - M;
    const int lane = threadIdx.x;
    const int t8 = lane >> 3, cl = lane & 7;
    const int64_t slot = (int64_t)blockIdx.x * 8 + t8;
    const int64_t tb = slot >> 6, tl = slot & 63;
    const int qbase = blockIdx.y * NQ;
    uint32_t val[NQ][NO];  // bytesum(a) - 256 * carries, mod 2^32, this lane's columns
#pragma unroll
    for (int n = 0; n < NQ; ++n)
#pragma unroll
        for (int o = 0; o < NO; ++o) val[n][o] = 0u;
    for (int c = cl; c < WD; c += 8) {
        const uint4* col = lib + ((size_t)(tb * WD + c) * HQ) * 64 + tl;
        uint32_t aL[4 * HQ], aH[4 * HQ], bs[4 * HQ];
#pragma unroll
        for (int q = 0; q < HQ; ++q) {
            const uint4 v = col[(size_t)q * 64];
            const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                aL[4 * q + k] = w[k] & 0x7F7F7F7Fu;
                aH[4 * q + k] = w[k] & 0x80808080u;
                bs[4 * q + k] = __builtin_amdgcn_sad_u8(w[k], 0u, 0u);
            }
        }
        uint32_t A[NO];
        uint32_t win = 0u;
#pragma unroll
        for (int s = R0 - (M - 1); s < R1 - (M - 1); ++s) win += bs[s];
        A[0] = win;
#pragma unroll
        for (int o = 1; o < NO; ++o) {
            win += bs[R1 - (M - 1) + o - 1] - bs[R0 - (M - 1) + o - 1];
            A[o] = win;
        }
#pragma unroll
        for (int n = 0; n < NQ; ++n) {
            uint32_t cnt[NO];
#pragma unroll
            for (int o = 0; o < NO; ++o) cnt[o] = 0u;
            const int qi = min(qbase + n, nq - 1);
#pragma unroll
            for (int r = R0; r < R1; ++r) {
                const uint2 f = qf[((size_t)qi * WD + c) * H + r];
#pragma unroll
                for (int o = 0; o < NO; ++o) cnt[o] = carry_pair(aL[r + o - (M - 1)], aH[r + o - (M - 1)], f, cnt[o]);
            }
#pragma unroll
            for (int o = 0; o < NO; ++o) val[n][o] += A[o] - 256u * cnt[o];
        }
    }
#pragma unroll
    for (int n = 0; n < NQ; ++n) {
        const uint32_t qs = qsum[min(qbase + n, nq - 1)];
        uint32_t sc = 0xFFFFFFFFu;
#pragma unroll
        for (int o = 0; o < NO; ++o) {
            uint32_t v = val[n][o];
            v += __shfl_xor(v, 1);
            v += __shfl_xor(v, 2);
            v += __shfl_xor(v, 4);
            sc = min(sc, v + qs);
        }
        const unsigned long long g = (unsigned long long)slot * nranks + rank;
        unsigned long long key =
            (slot < count && cl == 0) ? (((unsigned long long)sc << 32) | g) : NO_KEY;
        key = wave_min_u64(key);
        if (lane == 0 && qbase + n < nq) atomicMin(out.best + qbase + n, key);
    }
}

// --- generic form (any H, max_offset): one thread per (slot, query).
template <bool MATRIX>
__global__ __launch_bounds__(64) void vt_scan_generic_kernel(const uint4* __restrict__ lib, int ntb,
                                                             int64_t count, int H, int M, int WD,
                                                             const uint2* __restrict__ qf, int nq,
                                                             ScanOut out, int rank, int nranks) {
    const int HQ = (H + 3) / 4;
    const int tb = blockIdx.x % ntb;
    const int qi = blockIdx.x / ntb;
    const int lane = threadIdx.x;
    const uint32_t* base = reinterpret_cast<const uint32_t*>(lib);
    uint32_t best = 0xFFFFFFFFu;
    bool any = false;
    for (int o = -(M - 1); o <= M - 1; ++o) {
        uint32_t acc = 0;
        for (int r = M; r < H - M; ++r) {
            const int s = r + o;
            for (int c = 0; c < WD; ++c) {
                const size_t chunk = ((size_t)(tb * WD + c) * HQ + (s >> 2)) * 64 + lane;
                const uint32_t a = base[chunk * 4 + (s & 3)];
                acc = wrapped_pair(a & 0x7F7F7F7Fu, a & 0x80808080u,
                                   qf[((size_t)qi * WD + c) * H + r], acc);
            }
        }
        best = min(best, acc);
        any = true;
    }
    if (!any) best = 0;
    emit_score<MATRIX>(out, (int64_t)tb * 64 + lane, count, qi, nq, best, rank, nranks, lane == 0);
}
