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
#include <vector>

#include "rs_common.h"
#include "vt_offset_rule.h"
#include "vt_plan.h"

namespace {

constexpr int FAST_M = 8;  // ViewTemplate.max_offset (view_templates.py:14)
constexpr unsigned long long NO_KEY = ~0ull;

__device__ inline unsigned long long wave_min_u64(unsigned long long v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned long long o = __shfl_xor(v, off);
        v = o < v ? o : v;
    }
    return v;
}

__device__ inline uint32_t wrapped_pair(uint32_t aL, uint32_t aH, uint2 f, uint32_t acc) {
    return __builtin_amdgcn_sad_u8(__builtin_amdgcn_bitop3_b32(aL + f.x, aH, f.y, 0x96), 0u, acc);
}

// Scatter n raw (H x W) templates into library slots (layout above).
__global__ void vt_store_kernel(const uint8_t* __restrict__ raw, const int32_t* __restrict__ src,
                                const int64_t* __restrict__ dst, int n, uint4* __restrict__ lib,
                                int H, int W, int WD, int HQ) {
    const int64_t total = (int64_t)n * WD * HQ;
    for (int64_t idx = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; idx < total;
         idx += (int64_t)gridDim.x * blockDim.x) {
        const int t = (int)(idx / (WD * HQ));
        const int rem = (int)(idx - (int64_t)t * WD * HQ);
        const int c = rem / HQ, q = rem - c * HQ;
        const uint8_t* tpl = raw + (size_t)src[t] * H * W;
        uint32_t w[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int row = 4 * q + k;
            uint32_t d = 0;
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                const int col = 4 * c + b;
                const uint32_t byte = (row < H && col < W) ? tpl[(size_t)row * W + col] : 0u;
                d |= byte << (8 * b);
            }
            w[k] = d;
        }
        const int64_t slot = dst[t];
        const int64_t tb = slot >> 6, tl = slot & 63;
        lib[((tb * WD + c) * HQ + q) * 64 + tl] = make_uint4(w[0], w[1], w[2], w[3]);
    }
}

// On-device subsampling (view_templates.py:64, input[self.mask].reshape(shape)):
// query f = frame f gathered through the mask's pixel offsets, row-major.
__global__ __launch_bounds__(256) void vt_gather_kernel(const uint8_t* __restrict__ frames,
                                                        size_t frame_bytes,
                                                        const int32_t* __restrict__ pix, int npix,
                                                        uint8_t* __restrict__ out) {
    const uint8_t* f = frames + (size_t)blockIdx.x * frame_bytes;
    uint8_t* o = out + (size_t)blockIdx.x * npix;
    for (int i = threadIdx.x; i < npix; i += blockDim.x) o[i] = f[pix[i]];
}

// Query forms: qf[(n*WD + c)*H + r] = (cL, cH) of c = -Q[r][4c..4c+3] mod 256,
// and qsum[n] = sum over rows [M, H-M) of the bytes of c (carry-count scan).
// One block per query.
__global__ __launch_bounds__(256) void vt_qform_kernel(const uint8_t* __restrict__ raw, int H, int W,
                                                       int WD, int M, uint2* __restrict__ qf,
                                                       uint32_t* __restrict__ qsum) {
    __shared__ uint32_t s_red[4];
    const int qn = blockIdx.x;
    uint32_t part = 0;
    for (int idx = threadIdx.x; idx < WD * H; idx += blockDim.x) {
        const int c = idx / H, r = idx - c * H;
        uint32_t neg = 0;
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const int col = 4 * c + b;
            const uint32_t byte = col < W ? raw[((size_t)qn * H + r) * W + col] : 0u;
            neg |= ((256u - byte) & 0xFFu) << (8 * b);
        }
        qf[(size_t)qn * WD * H + idx] = make_uint2(neg & 0x7F7F7F7Fu, neg & 0x80808080u);
        if (r >= M && r < H - M) part = __builtin_amdgcn_sad_u8(neg, 0u, part);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) part += __shfl_xor(part, off);
    if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = part;
    __syncthreads();
    if (threadIdx.x == 0) qsum[qn] = s_red[0] + s_red[1] + s_red[2] + s_red[3];
}

// Output of a scan: either min-reduce packed keys per query (best[]) or
// write every (query, slot) score into a matrix.
struct ScanOut {
    unsigned long long* best;  // [nq] packed keys (MATRIX == false)
    uint32_t* mat;             // [nq][ld]          (MATRIX == true)
    int64_t ld;
    // plane scan, MATRIX == false: the block that finishes last hands the keys to the
    // host words and resets them (vt_keys_export folded in); done counts the blocks
    unsigned long long* host = nullptr;
    unsigned* done = nullptr;
};

template <bool MATRIX>
__device__ inline void emit_score(const ScanOut& out, int64_t slot, int64_t count, int qi, int nq,
                                  uint32_t score, int rank, int nranks, bool lane0_after_reduce) {
    if constexpr (MATRIX) {
        if (slot < count && qi < nq) out.mat[(size_t)qi * out.ld + slot] = score;
    } else {
        const unsigned long long g = (unsigned long long)slot * nranks + rank;
        unsigned long long key = slot < count ? (((unsigned long long)score << 32) | g) : NO_KEY;
        key = wave_min_u64(key);
        if (lane0_after_reduce && qi < nq) atomicMin(out.best + qi, key);
    }
}

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

static_assert(vt_plan::METRIC_WRAPPED == RS_VT_METRIC_WRAPPED && vt_plan::METRIC_SAD == RS_VT_METRIC_SAD,
              "vt_plan.h restates the ABI's metric codes");
#include "vt_sad.h"
static_assert(rs::VTO_METRIC_WRAPPED == RS_VT_METRIC_WRAPPED && rs::VTO_METRIC_SAD == RS_VT_METRIC_SAD,
              "vt_offset_rule.h restates the ABI's metric codes");
#include "vt_offset.h"

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

// Per-wave stamp hook, empty in the library: tools/vt_probe.hip defines it (realtime at
// the phase ends of every wave of the plane scan, hw ids) before it includes this file.
// VT_STAMP_BEGIN: kernel entry; VT_STAMP_KNOWN (slot 0): the list's length known and the
// block stays; then slots 1 the first take returned, 2 first
// batch staged (past the prologue's barrier), 3 this wave's template planes landed, 4 first
// batch computed, 5 last batch computed, 6 end.  Every site has `ids` in scope (the probe
// tells the launches apart by it).
#ifndef VT_STAMP
#define VT_STAMP_BEGIN() \
    do {                 \
    } while (0)
#define VT_STAMP_KNOWN() \
    do {                 \
    } while (0)
#define VT_STAMP(slot) \
    do {               \
    } while (0)
#endif
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
struct PlaneIds {
    int qc[PL_NB];  // query ids of the batch being computed (wave-uniform)
    int qnv;        // lane: query id of entry (lane & 3) of the batch staged next
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
        emit_score<MATRIX>(out, slot, count, qi, LIST ? qi + 1 : nq, best - qsum[qi], rank, nranks, lane == 0);
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
                                           const vt_plan::Take& tk, int v0, int w) {
    using R = PlaneRange<H, HALF>;
    const int nbatch = tk.nbatch, tid = wave * 64 + lane;
    const int W = LIST ? w : PL_NB;   // entries per batch (block-uniform)
    int bi = tk.sb, b1 = nbatch;
    if (tid == 0) b1 = plane_take(ctr, tk, failed);
    for (int i = tid; i < PL_NB * PL_NK * 64; i += 64 * PL_CG * PL_SPLIT) {
        (&vt_pl_part0[0][0][0])[i] = 0u;
        (&vt_pl_part1[0][0][0])[i] = 0u;
    }
    PlaneIds pid{{0, 0, 0, 0}, 0};
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
                          PlaneList pl) {
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
    if (tk.sb >= tk.nbatch) {   // (block-uniform) no batch for this block: it leaves the counter alone
    } else if (half == 0)
        plane_wave<H, 0, MATRIX, LIST>(planes, tsum, tb, count, qp4, qsum, nq, ctr, G, g, out, rank, nranks,
                                       wave, cg, lane, failed, ids, tk, v0, W);
    else
        plane_wave<H, 1, MATRIX, LIST>(planes, tsum, tb, count, qp4, qsum, nq, ctr, G, g, out, rank, nranks,
                                       wave, cg, lane, failed, ids, tk, v0, W);
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

// Wave-wide minimum as a wave-uniform value, without the LDS pipe (the prefilter's pace
// is set by its LDS reads, and a shuffle is a ds_bpermute): four DPP steps leave each
// row of 16 lanes its minimum (lanes ^1, ^2, then the row's other half-row and the
// other half mirrored), and the four rows meet through scalar registers.
__device__ __forceinline__ uint32_t wave_min_u32_dpp(uint32_t v) {
    v = min(v, (uint32_t)__builtin_amdgcn_update_dpp((int)v, (int)v, 0xB1, 0xF, 0xF, false));    // quad_perm [1,0,3,2]
    v = min(v, (uint32_t)__builtin_amdgcn_update_dpp((int)v, (int)v, 0x4E, 0xF, 0xF, false));    // quad_perm [2,3,0,1]
    v = min(v, (uint32_t)__builtin_amdgcn_update_dpp((int)v, (int)v, 0x141, 0xF, 0xF, false));   // row_half_mirror
    v = min(v, (uint32_t)__builtin_amdgcn_update_dpp((int)v, (int)v, 0x140, 0xF, 0xF, false));   // row_mirror
    return min(min((uint32_t)__builtin_amdgcn_readlane((int)v, 0), (uint32_t)__builtin_amdgcn_readlane((int)v, 16)),
               min((uint32_t)__builtin_amdgcn_readlane((int)v, 32), (uint32_t)__builtin_amdgcn_readlane((int)v, 48)));
}

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
                                                                    uint32_t* __restrict__ second) {
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
                                                int* __restrict__ tbstar, uint4* s_q, uint4* s_t) {
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
    if (lane == 0) {
        if (settled) {
            const unsigned long long g = ((unsigned long long)tbs * 64 + tl) * nranks + rank;
            atomicMin(best + q, ((unsigned long long)u0 << 32) | g);
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
                                                             int nranks, int* __restrict__ tbstar) {
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
    }, nq, planes, tsum, qc4, qp4, qsum, best, rank, nranks, tbstar, s_q, s_t);
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
                     int nranks, int* __restrict__ tbstar) {
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
            }, nq, planes, tsum, qc4, qp4, qsum, best, rank, nranks, tbstar, s_vq[wave], s_vt[wave]);
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

// ===========================================================================
// Float path of ViewTemplate.match (view_templates.py:16-28 with float arrays):
// no wrap, a true sum of |T - Q| per row offset in the arrays' own precision,
// summed in numpy's order -- np.sum of the contiguous (H-2M) x W difference is
// numpy's pairwise summation over the flattened n elements (blocks of <= 128
// with 8 strided accumulators, halves split at a multiple of 8), so the host
// lowers that recursion for this n into a postfix program of leaf sums and adds
// (int2 (start, len) = push the leaf's sum; (-1, 0) = pop two, push their sum)
// that every thread evaluates: the same additions in the same order, bit-exact.
// Then the first strict minimum over the offsets from +inf, as the reference's
// `if diff < mindiff` loop (an all-NaN pair stays +inf).
// ===========================================================================
template <typename T>
__device__ inline T sad_at(const T* __restrict__ a, const T* __restrict__ b, int W, int M, int o,
                           int i) {
    const int r = i / W, c = i - r * W;
    const T d = a[(size_t)(M + o + r) * W + c] - b[(size_t)(M + r) * W + c];
    if constexpr (sizeof(T) == 4) return fabsf(d);   // numpy's absolute is fabs
    else return fabs(d);
}

template <typename T>
__device__ T sad_leaf(const T* a, const T* b, int W, int M, int o, int s, int n) {
    if (n < 8) {
        T res = T(0);
        for (int i = 0; i < n; ++i) res += sad_at(a, b, W, M, o, s + i);
        return res;
    }
    T r[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) r[j] = sad_at(a, b, W, M, o, s + j);
    int i = 8;
    for (; i < n - (n % 8); i += 8)
#pragma unroll
        for (int j = 0; j < 8; ++j) r[j] += sad_at(a, b, W, M, o, s + i + j);
    T res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
    for (; i < n; ++i) res += sad_at(a, b, W, M, o, s + i);
    return res;
}

constexpr int SAD_STACK = 40;   // pairwise depth: log2(n / 128) + 2 <= 40 for any n < 2^31

// 4 (template, query) pairs per 64-thread block, 16 threads per pair (one per offset)
template <typename T>
__global__ __launch_bounds__(64) void vt_sad_float_kernel(const T* __restrict__ tpl, int64_t nt,
                                                          const T* __restrict__ qry, int nq, int H,
                                                          int W, int M,
                                                          const int2* __restrict__ prog, int nprog,
                                                          T* __restrict__ out) {
    __shared__ T s_d[4][16];
    const int sub = threadIdx.x >> 4, oi = threadIdx.x & 15, NO = 2 * M - 1;
    const int64_t pair = (int64_t)blockIdx.x * 4 + sub;
    const bool live = pair < nt * (int64_t)nq;
    const int64_t t = live ? pair % nt : 0, qi = live ? pair / nt : 0;
    T d = T(INFINITY);
    if (live && oi < NO) {
        const T* a = tpl + (size_t)t * H * W;
        const T* b = qry + (size_t)qi * H * W;
        const int o = oi - (M - 1);
        T st[SAD_STACK];
        int sp = 0;
        for (int k = 0; k < nprog; ++k) {
            const int2 op = prog[k];
            if (op.x >= 0) {
                st[sp++] = sad_leaf(a, b, W, M, o, op.x, op.y);
            } else {
                const T rhs = st[--sp];
                st[sp - 1] = st[sp - 1] + rhs;
            }
        }
        d = st[0];
    }
    if (oi < 16) s_d[sub][oi] = d;
    __syncthreads();
    if (live && oi == 0) {
        T best = T(INFINITY);
        for (int k = 0; k < NO; ++k)
            if (s_d[sub][k] < best) best = s_d[sub][k];
        out[(size_t)qi * nt + t] = best;
    }
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
// simply stays until all three have grown.
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
    hipStream_t stream = nullptr;
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
    hipStream_t cstream = nullptr;           // rs_vt_match_stream's collective stream
    hipEvent_t evScan = nullptr, evComm = nullptr;
    hipStream_t ustream = nullptr;           // rs_vt_match_stream: host batches' upload stream
    hipEvent_t evUp[2] = {nullptr, nullptr}, evUsed[2] = {nullptr, nullptr};
    rs::DevBuf<uint8_t> dUp[2];              // ... and its two raw-query group buffers
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
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
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
    RS_HIP(hipMemsetAsync(nb.get(), 0, bytes, h->stream));
    if (buf.get()) {
        if (keep > 0)
            RS_HIP(hipMemcpyAsync(nb.get(), buf.get(), (size_t)keep * bb, hipMemcpyDeviceToDevice, h->stream));
        RS_HIP(hipStreamSynchronize(h->stream));
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
        RS_HIP(hipStreamSynchronize(h->stream));
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

// RS_VT_ZC=0: no batch is read in place from the pinned staging array (vt_plan::stages_in_place).
bool vt_zc_env() { static const bool on = rs::env_on("RS_VT_ZC"); return on; }

// Upload nq raw queries and build their forms (the batch view) on the device.
int vt_stage_queries(rs_vt* h, int nq, const uint8_t* queries) {
    RS_TRY(vt_grow_queries(h, nq));
    RS_TRY(vt_qraw_idle(h));
    const QueryForms q = vt_batch_view(h);
    const size_t qb = (size_t)h->H * h->W * nq;
    // larger batches: HIP's own upload of the caller's (pageable) array, which returns
    // once the bytes are staged (per-batch PCIe-inclusive rate 4.04-4.12 against 3.44-3.54
    // G compares/s through our memcpy into pinned staging, round 5).  The call waits for
    // its keys, which the scan stores after the copy has run, so a pinned caller array is
    // no longer read when it returns.
    if (vt_plan::stages_in_place(h->planar, nq, vt_zc_env())) {
        std::memcpy(h->hQraw.get(), queries, qb);
        h->qrawBusy = true;
        uint32_t* const qc = vt_compact_for(h, q, nq);
        hipLaunchKernelGGL(vt_qplane_kernel, dim3(nq), dim3(qc ? VT_QC_THREADS : 256), 0, h->stream, h->hQraw.dev(), h->H,
                           h->M, q.qp, q.qsum, h->dQraw.get(), q.qsj, qc);
        RS_HIP(hipGetLastError());
        return RS_OK;
    }
    RS_HIP(hipMemcpyAsync(h->dQraw.get(), queries, qb, hipMemcpyHostToDevice, h->stream));
    return vt_build_forms(h, q, nq);
}

// Build the query forms of nq raw queries in device memory (default: dQraw) into the view q.
// The plane scan reads only the planes; the byte-SWAR forms serve the other scans.
int vt_build_forms(rs_vt* h, const QueryForms& q, int nq, const uint8_t* src) {
    if (h->metric == RS_VT_METRIC_SAD)
        hipLaunchKernelGGL(vt_qform_sad_kernel, dim3(nq), dim3(256), 0, h->stream, src, h->H, h->W, h->WD,
                           reinterpret_cast<uint32_t*>(h->dQf.get()));
    else if (!h->planar)
        hipLaunchKernelGGL(vt_qform_kernel, dim3(nq), dim3(256), 0, h->stream, src, h->H, h->W,
                           h->WD, h->M, h->dQf.get(), h->dQsum.get());
    else {
        uint32_t* const qc = vt_compact_for(h, q, nq);
        hipLaunchKernelGGL(vt_qplane_kernel, dim3(nq), dim3(qc ? VT_QC_THREADS : 256), 0, h->stream, src, h->H,
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
        RS_HIP(hipMemcpyAsync(h->dFrames.get(), h->hFrames.get(), fb, hipMemcpyHostToDevice, h->stream));
        src = h->dFrames.get();
    }
    hipLaunchKernelGGL(vt_gather_kernel, dim3(nf), dim3(256), 0, h->stream, src,
                       (size_t)h->frameBytes, h->dPix.get(), h->H * h->W, h->dQraw.get());
    RS_HIP(hipGetLastError());
    return vt_build_forms(h, vt_batch_view(h), nf);
}

// Store raw staged queries src[i] into slots dst[i] of the library (or, with
// `cand`, of the candidate buffer).
int vt_store(rs_vt* h, bool cand, const uint8_t* d_raw, int n) {
    if (n == 0) return RS_OK;
    uint4* lib = cand ? h->dCand.get() : h->dLib.get();
    RS_HIP(hipMemcpyAsync(h->dSrc.get(), h->hSrc.get(), sizeof(int32_t) * n, hipMemcpyHostToDevice, h->stream));
    RS_HIP(hipMemcpyAsync(h->dDst.get(), h->hDst.get(), sizeof(int64_t) * n, hipMemcpyHostToDevice, h->stream));
    h->stagingBusy = true;
    const int64_t total = (int64_t)n * h->WD * h->HQ;
    const int grid = (int)std::min<int64_t>((total + 255) / 256, 4096);
    hipLaunchKernelGGL(vt_store_kernel, dim3(grid), dim3(256), 0, h->stream, d_raw, h->dSrc.get(),
                       h->dDst.get(), n, lib, h->H, h->W, h->WD, h->HQ);
    if (h->planar)
        hipLaunchKernelGGL(vt_plane_store_kernel, dim3(n), dim3(256), 0, h->stream, d_raw, h->dSrc.get(),
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

// The only launch of vt_keys_export: n keys -> host (pinned, device address), reset behind it.
void vt_launch_keys_export(rs_vt* h, unsigned long long* keys, int n, unsigned long long* host, int max_blocks) {
    hipLaunchKernelGGL(vt_keys_export, dim3((unsigned)vt_plan::export_grid(n, max_blocks)), dim3(256), 0, h->stream,
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
void vt_launch_plane_scan(rs_vt* h, const PlaneScan& s, const ScanOut& out, const PlaneList& list) {
    hipLaunchKernelGGL((vt_scan_plane_kernel<H, MATRIX, LIST>), s.grid, dim3(64 * PL_CG * PL_SPLIT), 0, h->stream,
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
    if (ntb > h->listCntCap) {  // zero at first; the list kernels zero what they are about to fill
        const int cap = std::max(ntb, 2 * h->listCntCap);
        h->listCntCap = 0;
        RS_TRY(h->dListCnt.reserve(2 * (size_t)cap + 1));
        RS_HIP(hipMemsetAsync(h->dListCnt.get(), 0, sizeof(unsigned) * (2 * (size_t)cap + 1), h->stream));
        h->listCntCap = cap;
    }
    if (!h->dPruneStat.get()) {
        RS_TRY(h->dPruneStat.reserve(3));
        RS_HIP(hipMemsetAsync(h->dPruneStat.get(), 0, 3 * sizeof(unsigned long long), h->stream));
    }
    return RS_OK;
}

// Pruned scan of the frozen library (vt_prunes): prefilter, verification, then the scan of
// each query's candidate block (list 1, pass B1) and of the blocks its bound leaves (list 2,
// pass B2).
int vt_launch_pruned(rs_vt* h, const PlaneScan& s, const ScanOut& out) {
    const QueryForms& q = s.q;
    const int ntb = s.ntb, nq = s.nq;
    if (!h->qcValid) {   // the build before did not expect this scan to prune
        hipLaunchKernelGGL(vt_qcompact_kernel, dim3((unsigned)nq), dim3(128), 0, h->stream,
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
    if (h->front == 2 || (h->front == 1 && vt_plan::front_fused(ntb, PF_WAVES * PF_TPW))) {
        const vt_plan::Grid2 fg = vt_plan::front_grid(nq, PF_NB, VT_PF_GRID_CAP);
        hipLaunchKernelGGL(vt_front_kernel, dim3((unsigned)fg.x, (unsigned)fg.y), dim3(64 * PF_WAVES), 0, h->stream,
                           s.planes, ntb, s.count, reinterpret_cast<const uint4*>(q.qc), q.qsj, nq, h->dMinLB.get(),
                           s.ts, reinterpret_cast<uint4*>(q.qp), q.qsum, out.best, s.rank, s.nranks,
                           h->dTbStar.get());
    } else {
        const vt_plan::Grid2 pf = vt_plan::prefilter_grid(ntb, nq, PF_WAVES * PF_TPW, PF_NB, VT_PF_GRID_CAP);
        hipLaunchKernelGGL(vt_prefilter_kernel, dim3((unsigned)pf.x, (unsigned)pf.y), dim3(64 * PF_WAVES), 0,
                           h->stream, s.planes, ntb, s.count, reinterpret_cast<const uint4*>(q.qc), q.qsj, nq,
                           h->dMinLB.get(), h->dSecond.get());
        hipLaunchKernelGGL(vt_prune_verify_kernel, dim3((unsigned)nq), dim3(64), 0, h->stream, h->dMinLB.get(),
                           h->dSecond.get(), ntb, nq, s.planes, s.ts, reinterpret_cast<const uint4*>(q.qc),
                           reinterpret_cast<uint4*>(q.qp), q.qsum, out.best, s.rank, s.nranks, h->dTbStar.get());
    }
    const dim3 lgrid((unsigned)((nq + VT_LIST_T - 1) / VT_LIST_T), (unsigned)ntb);
    hipLaunchKernelGGL(vt_prune_first_kernel, lgrid, dim3(VT_LIST_T), 0, h->stream, nq, h->dTbStar.get(), cnt1,
                       list1, verified, cnt2, ntb);
    // the passes min into the same keys; the folded export (out.host) needs one
    // launch to be the last, so a pruned call exports with vt_keys_export
    ScanOut po = out;
    po.host = nullptr;
    po.done = nullptr;
    // working blocks per template block that make one resident round (vt_plan::list_width)
    const uint32_t fill = (uint32_t)std::min(65535, std::max(1, h->planeSlots / ntb));
    const uint32_t lnb = (uint32_t)h->listNb;
    vt_launch_plane_scan<64, false, true>(h, s, po,
                                          PlaneList{list1, cnt1, nq, (uint32_t)VT_LIST_PER_B1, lnb, 1u, fill});
    hipLaunchKernelGGL(vt_prune_rest_kernel, lgrid, dim3(VT_LIST_T), 0, h->stream, h->dMinLB.get(), nq,
                       h->dTbStar.get(), out.best, cnt2, list2, cnt1, verified, ntb, h->dPruneStat.get());
#ifdef VT_LIST_PER
    const int per2 = VT_LIST_PER;
#else
    const int per2 = vt_plan::list_per(ntb, h->planeSlots);
#endif
    vt_launch_plane_scan<64, false, true>(h, s, po, PlaneList{list2, cnt2, nq, (uint32_t)per2, lnb, 0u, fill});
    if (out.host) vt_launch_keys_export(h, out.best, nq, out.host, vt_plan::VT_EXPORT_BLOCKS);
    RS_HIP(hipGetLastError());
    h->prunePairs = (int64_t)pairs;
    h->prunePasses = 2;
    h->pruneNtb = ntb;
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
        RS_HIP(hipMemsetAsync(h->dCtr.get(), 0, sizeof(unsigned) * cap, h->stream));
    }
    RS_CHECK((int64_t)ntb * nqc < (1ll << 31), RS_ERR_ARG, "scan grid too large");
    const uint4* planes = reinterpret_cast<const uint4*>(
        reinterpret_cast<const uint8_t*>(cand ? h->dCandP.get() : h->dLibP.get()) + (size_t)tb0 * pblock_bytes(h));
    const uint32_t* ts = (cand ? h->dCandTs.get() : h->dLibTs.get()) + (size_t)tb0 * (TS_BLOCK_BYTES / 4);
    const PlaneScan s{dim3((unsigned)(ntb * nqc)), planes, ts, ntb, count, q, nq, nqc, rank, nranks};
    if constexpr (!MATRIX)
        if (vt_prunes(h, q, cand, tb0, count, nq)) return vt_launch_pruned(h, s, out);
    if (!h->qpFull) {   // a compact build, and a scan that reads every query's planes
        hipLaunchKernelGGL(vt_qexpand_kernel, dim3((unsigned)nq), dim3(256), 0, h->stream,
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
                               dim3(64 * vt_plan::sad_waves(h->WD)), 0, h->stream, lib, ntb, count, h->WD, qd, nq,
                               nqc, out, rank, nranks);
        });
    } else {
        hipLaunchKernelGGL((vt_scan_sad_generic_kernel<MATRIX>), dim3((unsigned)(ntb * nq)), dim3(64), 0, h->stream,
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
            hipLaunchKernelGGL((vt_scan_carry_col_kernel<decltype(H)::value, 1>), grid, dim3(64), 0, h->stream, lib,
                               count, h->WD, h->dQf.get(), h->dQsum.get(), nq, out, rank, nranks);
        });
    } else if (fast) {
        constexpr int NQ = 2;
        const int nqg = (nq + NQ - 1) / NQ;
        const dim3 grid((unsigned)(ntb * ((nqg + 7) / 8) * 8));
        vt_by_h(h, [&](auto H) {
            hipLaunchKernelGGL((vt_scan_carry_kernel<decltype(H)::value, NQ, MATRIX>), grid, dim3(64), 0, h->stream,
                               lib, ntb, count, h->WD, h->dQf.get(), h->dQsum.get(), nq, out, rank, nranks);
        });
    } else {
        hipLaunchKernelGGL((vt_scan_generic_kernel<MATRIX>), dim3((unsigned)(ntb * nq)), dim3(64),
                           0, h->stream, lib, ntb, count, h->H, h->M, h->WD, h->dQf.get(), nq, out, rank,
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
        RS_HIP(hipStreamSynchronize(h->stream));
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
    if (timed) RS_HIP(hipEventRecord(h->ev0, h->stream));
    RS_TRY(run());
    if (timed) RS_HIP(hipEventRecord(h->ev1, h->stream));
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
        RS_HIP(hipMemsetAsync(h->dBest.get(), 0xFF, sizeof(unsigned long long) * nq, h->stream));
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
            RS_HIP(hipMemsetAsync(h->dDone.get(), 0, sizeof(unsigned), h->stream));
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
                              h->stream));
        RS_HIP(hipStreamSynchronize(h->stream));
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
        RS_TRY(vt_allreduce_min(h, h->dBest.get(), (size_t)nq, h->stream));
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
        RS_HIP(hipStreamSynchronize(h->stream));
        h->stagingBusy = false;
    }
    // the keys are the call's last work: everything queued before them has run,
    // the readers of hQraw included (not the staging copies vt_store queues after them)
    h->qrawBusy = false;
    h->bestClean = h->bestPending;
    if (h->timedScan) RS_HIP(hipEventElapsedTime(&h->lastMs, h->ev0, h->ev1));
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
    RS_TRY(vt_build_forms(h, q, (int)total, queries));
    const ScanOut out{h->dStream.get(), nullptr, 0};
    RS_TRY(vt_timed_scan(h, h->timing, [&] {
        return vt_launch_scan<false>(h, q, false, lc, (int)total, out, h->rank, h->nranks);
    }));
    if (h->comm) RS_TRY(vt_allreduce_min(h, h->dStream.get(), total, h->stream));
    return RS_OK;
}

// Host batches in upload groups (vt_plan::host_groups), double-buffered on the upload
// stream; one collective.  Scans interleaved with upload waits have no single duration:
// timedScan stays false.
int vt_stream_host_groups(rs_vt* h, int nb, int nq, const uint8_t* queries, int64_t lc) {
    const size_t total = (size_t)nb * nq, qb = (size_t)h->H * h->W * nq;
    RS_TRY(vt_grow_stream_forms(h, total));
    const vt_plan::HostGroups plan = vt_plan::host_groups(nb);
    if (!h->ustream) {
        RS_HIP(hipStreamCreateWithFlags(&h->ustream, hipStreamNonBlocking));
        for (int i = 0; i < 2; ++i) {
            RS_HIP(hipEventCreateWithFlags(&h->evUp[i], hipEventDisableTiming));
            RS_HIP(hipEventCreateWithFlags(&h->evUsed[i], hipEventDisableTiming));
        }
    }
    if (qb * plan.gb > h->upCap) {
        RS_HIP(hipStreamSynchronize(h->ustream));
        h->upCap = 0;
        for (int i = 0; i < 2; ++i) RS_TRY(h->dUp[i].reserve(qb * plan.gb));
        h->upCap = qb * plan.gb;
    }
    for (int g = 0;; ++g) {
        const vt_plan::HostGroup grp = plan.group(g);
        if (grp.n == 0) break;
        const int bi = grp.buf;
        if (grp.waits) RS_HIP(hipStreamWaitEvent(h->ustream, h->evUsed[bi], 0));
        RS_HIP(hipMemcpyAsync(h->dUp[bi].get(), queries + qb * grp.b0, qb * grp.n, hipMemcpyHostToDevice, h->ustream));
        RS_HIP(hipEventRecord(h->evUp[bi], h->ustream));
        RS_HIP(hipStreamWaitEvent(h->stream, h->evUp[bi], 0));
        const QueryForms q = vt_stream_view(h, (size_t)grp.b0 * nq);
        RS_TRY(vt_build_forms(h, q, grp.n * nq, h->dUp[bi].get()));
        RS_HIP(hipEventRecord(h->evUsed[bi], h->stream));
        const ScanOut out{h->dStream.get() + (size_t)grp.b0 * nq, nullptr, 0};
        RS_TRY(vt_launch_scan<false>(h, q, false, lc, grp.n * nq, out, h->rank, h->nranks));
    }
    if (h->comm) RS_TRY(vt_allreduce_min(h, h->dStream.get(), total, h->stream));
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
            RS_HIP(hipMemcpyAsync(h->dQraw.get(), src, qb, hipMemcpyHostToDevice, h->stream));
            src = h->dQraw.get();
        }
        RS_TRY(vt_build_forms(h, vt_batch_view(h), nq, src));
        RS_TRY(vt_launch_scan<false>(h, vt_batch_view(h), false, lc, nq, out, h->rank, h->nranks));
        if (h->comm) {
            RS_HIP(hipEventRecord(h->evScan, h->stream));
            RS_HIP(hipStreamWaitEvent(h->cstream, h->evScan, 0));
            RS_TRY(vt_allreduce_min(h, keys, (size_t)nq, h->cstream));
        }
    }
    if (h->comm) {
        RS_HIP(hipEventRecord(h->evComm, h->cstream));
        RS_HIP(hipStreamWaitEvent(h->stream, h->evComm, 0));
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
    if (h->comm && !h->cstream) {
        RS_HIP(hipStreamCreateWithFlags(&h->cstream, hipStreamNonBlocking));
        RS_HIP(hipEventCreateWithFlags(&h->evScan, hipEventDisableTiming));
        RS_HIP(hipEventCreateWithFlags(&h->evComm, hipEventDisableTiming));
    }
    RS_HIP(hipSetDevice(h->device));
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
        RS_HIP(hipMemsetAsync(h->dStream.get(), 0xFF, sizeof(unsigned long long) * h->streamCap, h->stream));
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
    RS_HIP(hipStreamSynchronize(h->stream));
    h->streamClean = true;
    if (h->timedScan) RS_HIP(hipEventElapsedTime(&h->lastMs, h->ev0, h->ev1));
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
    int ndev = 0;
    RS_HIP(hipGetDeviceCount(&ndev));
    RS_CHECK(device >= 0 && device < ndev, RS_ERR_ARG, "device %d not in [0, %d)", device, ndev);
    RS_HIP(hipSetDevice(device));
    // one failure exit: rs_vt_destroy takes a handle at any stage (null streams and events)
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
        const char* e = std::getenv("RS_VT_PRUNE");
        if (!e || e[0] == 0 || std::strcmp(e, "1") == 0) h->prune = 1;
        else if (std::strcmp(e, "force") == 0) h->prune = 2;
        else RS_CHECK(std::strcmp(e, "0") == 0, RS_ERR_ARG, "RS_VT_PRUNE='%s': expected 0, 1 or force", e);
    }
    if (h->planar && h->H == 64) {
        // A/B switch: "0" keeps the prefilter and the verification two launches, "force"
        // fuses them for any shape (tests), "1" (or unset) follows vt_plan::front_fused
        const char* e = std::getenv("RS_VT_FRONT");
        if (!e || e[0] == 0 || std::strcmp(e, "1") == 0) h->front = 1;
        else if (std::strcmp(e, "force") == 0) h->front = 2;
        else {
            RS_CHECK(std::strcmp(e, "0") == 0, RS_ERR_ARG, "RS_VT_FRONT='%s': expected 0, 1 or force", e);
            h->front = 0;
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
    hipError_t e = hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipEventCreate(&h->ev0);
    if (e == hipSuccess) e = hipEventCreate(&h->ev1);
    RS_CHECK(e == hipSuccess, RS_ERR_HIP, "stream/event creation failed: %s", hipGetErrorString(e));
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
    hipError_t se = hipSuccess;
    for (hipStream_t st : {h->stream, h->cstream, h->ustream})
        if (st) {
            const hipError_t e = hipStreamSynchronize(st);
            if (se == hipSuccess) se = e;
        }
    if (h->comm) (void)ncclCommDestroy(h->comm);
    if (h->ev0) (void)hipEventDestroy(h->ev0);
    if (h->ev1) (void)hipEventDestroy(h->ev1);
    if (h->evScan) (void)hipEventDestroy(h->evScan);
    if (h->evComm) (void)hipEventDestroy(h->evComm);
    if (h->cstream) (void)hipStreamDestroy(h->cstream);
    for (int i = 0; i < 2; ++i) {
        if (h->evUp[i]) (void)hipEventDestroy(h->evUp[i]);
        if (h->evUsed[i]) (void)hipEventDestroy(h->evUsed[i]);
    }
    if (h->ustream) (void)hipStreamDestroy(h->ustream);
    if (h->stream) (void)hipStreamDestroy(h->stream);
    delete h;  // (the buffers go with their members)
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
    RS_HIP(hipMemcpyAsync(h->dQraw.get(), templates, qb,
                          attr.type == hipMemoryTypeDevice && direct_dma ? hipMemcpyDeviceToDevice
                                                                         : hipMemcpyHostToDevice,
                          h->stream));
    h->stagedQ = 0;  // the staging buffer now holds templates, not a query batch
    std::vector<std::pair<int, int64_t>> news;
    news.reserve(n);
    for (int i = 0; i < n; ++i) news.emplace_back(i, h->count + i);
    const int s = vt_append_staged(h, news);   // (its copies guarded by vt_staging_idle, not a sync)
    // (on the error path as well: the upload above is queued either way)
    if (direct_dma) {
        const hipError_t e = hipStreamSynchronize(h->stream);
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
                                  hipMemcpyDeviceToHost, h->stream));
    RS_HIP(hipStreamSynchronize(h->stream));
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
    RS_HIP(hipMemcpyAsync(h->dPix.get(), pixels, sizeof(int32_t) * npix, hipMemcpyHostToDevice, h->stream));
    RS_HIP(hipStreamSynchronize(h->stream));
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
                            sizeof(uint32_t) * nt, nq, hipMemcpyDeviceToHost, h->stream));
    RS_HIP(hipStreamSynchronize(h->stream));
    RS_HIP(hipEventElapsedTime(&h->lastMs, h->ev0, h->ev1));
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
    if (queries && rs::on_device(queries)) {
        src = queries;   // read in place
    } else if (queries) {
        RS_TRY(h->dOffQ.reserve(rs::grown<size_t>(h->dOffQ.capacity(), qb, 64 * (size_t)h->H * h->W)));
        RS_HIP(hipMemcpyAsync(h->dOffQ.get(), queries, qb, hipMemcpyHostToDevice, h->stream));
        src = h->dOffQ.get();
    }
    std::memcpy(h->hOffIdx.get(), index, sizeof(int64_t) * n);
    const bool sad = h->metric == RS_VT_METRIC_SAD, fast = h->M == FAST_M;
    auto launch = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, dim3(nq), dim3(64), 0, h->stream, h->dLib.get(), h->count, h->H, h->W,
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
    RS_HIP(hipStreamSynchronize(h->stream));
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

int rs_vt_prune_stats(rs_vt* h, int64_t out[4]) {
    rs::clear_error();
    RS_CHECK(h && out, RS_ERR_ARG, "null argument");
    out[0] = out[1] = out[2] = out[3] = 0;
    if (h->prunePasses == 0) return RS_OK;
    RS_HIP(hipSetDevice(h->device));
    // the pairs of B2: list2's counters, which stay until the next pruned launch's lists
    unsigned long long s0 = 0ull;
    std::vector<unsigned> c2((size_t)h->pruneNtb);
    RS_HIP(hipMemcpyAsync(&s0, h->dPruneStat.get(), sizeof(s0), hipMemcpyDeviceToHost, h->stream));
    RS_HIP(hipMemcpyAsync(c2.data(), h->dListCnt.get() + h->listCntCap, sizeof(unsigned) * c2.size(), hipMemcpyDeviceToHost,
                          h->stream));
    RS_HIP(hipStreamSynchronize(h->stream));
    out[0] = (int64_t)s0;
    for (const unsigned c : c2) out[1] += (int64_t)c;
    out[2] = h->prunePairs;
    out[3] = h->prunePasses;
    return RS_OK;
}

int rs_vt_prune_verified(rs_vt* h, int64_t* out) {
    rs::clear_error();
    RS_CHECK(h && out, RS_ERR_ARG, "null argument");
    *out = 0;
    if (h->prunePasses == 0) return RS_OK;
    RS_HIP(hipSetDevice(h->device));
    unsigned long long v = 0ull;
    RS_HIP(hipMemcpyAsync(&v, h->dPruneStat.get() + 2, sizeof(v), hipMemcpyDeviceToHost, h->stream));
    RS_HIP(hipStreamSynchronize(h->stream));
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

// host side of the float path: numpy's pairwise program for n elements
static void sad_program(int start, int n, std::vector<int2>& prog) {
    if (n <= 128) {
        prog.push_back(make_int2(start, n));
        return;
    }
    int n2 = n / 2;
    n2 -= n2 % 8;
    sad_program(start, n2, prog);
    sad_program(start + n2, n - n2, prog);
    prog.push_back(make_int2(-1, 0));
}

int rs_sad_scores(int device, int dtype, int H, int W, int max_offset, int64_t nt,
                  const void* templates, int nq, const void* queries, void* scores) {
    rs::clear_error();
    RS_CHECK(dtype == RS_DT_F32 || dtype == RS_DT_F64, RS_ERR_TYPE, "dtype %d is not F32/F64", dtype);
    RS_CHECK(H > 0 && W > 0 && max_offset >= 1 && max_offset <= 16 && H > 2 * max_offset,
             RS_ERR_ARG, "bad shape (%d, %d) for max_offset %d", H, W, max_offset);
    RS_CHECK((int64_t)H * W < (1ll << 31), RS_ERR_ARG, "template too large");
    RS_CHECK(nt >= 0 && nq >= 0, RS_ERR_ARG, "negative count");
    if (nt == 0 || nq == 0) return RS_OK;
    RS_CHECK(templates && queries && scores, RS_ERR_ARG, "null argument");
    int ndev = 0;
    RS_HIP(hipGetDeviceCount(&ndev));
    RS_CHECK(device >= 0 && device < ndev, RS_ERR_ARG, "device %d not in [0, %d)", device, ndev);
    RS_HIP(hipSetDevice(device));
    std::vector<int2> prog;
    sad_program(0, (H - 2 * max_offset) * W, prog);
    const size_t es = dtype == RS_DT_F32 ? 4 : 8;
    const size_t tb = (size_t)nt * H * W * es, qb = (size_t)nq * H * W * es, ob = (size_t)nt * nq * es;
    rs::DevBuf<void> bT, bQ, bO;
    rs::DevBuf<int2> bP;
    hipStream_t st = nullptr;
    int rc = RS_OK;
    auto run = [&]() -> int {
        RS_HIP(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
        RS_TRY(bT.reserve(tb));
        RS_TRY(bQ.reserve(qb));
        RS_TRY(bO.reserve(ob));
        RS_TRY(bP.reserve(prog.size()));
        void *const dT = bT.get(), *const dQ = bQ.get(), *const dO = bO.get();
        int2* const dP = bP.get();
        RS_HIP(hipMemcpyAsync(dT, templates, tb, hipMemcpyHostToDevice, st));
        RS_HIP(hipMemcpyAsync(dQ, queries, qb, hipMemcpyHostToDevice, st));
        RS_HIP(hipMemcpyAsync(dP, prog.data(), sizeof(int2) * prog.size(), hipMemcpyHostToDevice, st));
        const int64_t pairs = nt * (int64_t)nq;
        RS_CHECK((pairs + 3) / 4 < (1ll << 31), RS_ERR_ARG, "too many pairs");
        const dim3 grid((unsigned)((pairs + 3) / 4));
        if (dtype == RS_DT_F32)
            hipLaunchKernelGGL(vt_sad_float_kernel<float>, grid, dim3(64), 0, st,
                               static_cast<const float*>(dT), nt, static_cast<const float*>(dQ), nq,
                               H, W, max_offset, dP, (int)prog.size(),
                               static_cast<float*>(dO));
        else
            hipLaunchKernelGGL(vt_sad_float_kernel<double>, grid, dim3(64), 0, st,
                               static_cast<const double*>(dT), nt, static_cast<const double*>(dQ),
                               nq, H, W, max_offset, dP, (int)prog.size(),
                               static_cast<double*>(dO));
        RS_HIP(hipGetLastError());
        RS_HIP(hipMemcpyAsync(scores, dO, ob, hipMemcpyDeviceToHost, st));
        RS_HIP(hipStreamSynchronize(st));
        return RS_OK;
    };
    rc = run();
    if (st) (void)hipStreamDestroy(st);
    return rc;
}

}  // extern "C"
