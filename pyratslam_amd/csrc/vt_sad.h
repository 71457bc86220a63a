// True-SAD metric of the uint8 view-template matcher (RS_VT_METRIC_SAD), included by
// view_templates.hip behind vt_device.h (ScanOut / emit_score).
//
//   score(T, Q) = min_{o=-(M-1)..M-1} sum_{r=M..H-M-1, c} |T[r+o][c] - Q[r][c]|
// on the bytes as integers: ViewTemplate.match (view_templates.py:16-28) on the same
// arrays cast to float.  v_sad_u8 adds |a - b| of the four byte pairs of two dwords to an
// accumulator: one VALU instruction per template dword x query dword x offset.
//
// The library is read in the byte layout every handle keeps (chunk (tb, c, q, t) of
// view_templates.hip: rows 4q..4q+3 of dword column c of slot tb*64 + t; lane = template).
// Query form: qd[(n*WD + c)*H + r] = the dword Q[r][4c..4c+3] of query n, bytes past W
// zero (the library's padding bytes are zero too: such a pair adds |0 - 0|).
#pragma once

// One block per query.
__global__ __launch_bounds__(256) void vt_qform_sad_kernel(const uint8_t* __restrict__ raw, int H, int W,
                                                           int WD, uint32_t* __restrict__ qd) {
    const int qn = blockIdx.x;
    for (int idx = threadIdx.x; idx < WD * H; idx += blockDim.x) {
        const int c = idx / H, r = idx - c * H;
        uint32_t d = 0;
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const int col = 4 * c + b;
            const uint32_t byte = col < W ? raw[((size_t)qn * H + r) * W + col] : 0u;
            d |= byte << (8 * b);
        }
        qd[(size_t)qn * WD * H + idx] = d;
    }
}

// --- fast form (max_offset 8, H in {32, 64}, any W).
// A block is min(WD, SAD_NW) waves x 64 templates of template block tb.  Wave w takes the
// dword columns c = w, w + nw, ..: all H rows of one column in VGPRs (with WD <= SAD_NW the
// wave's one column stays there for every query the block walks), 2M-1 accumulators for
// each of SAD_NQ queries, the query dword Q[r][c] wave-uniform.  The waves' partial sums
// per (query, offset, template) meet in LDS as u32 (a sum reaches (H-16)*W*255) by
// ds_add_u32, in two buffers that alternate by query group: the wave that reduces a query
// zeroes its entries, which are next added to two groups (one barrier) later, so a group
// costs one barrier.  Block j of the nqc of a template block walks the groups j, j + nqc, ..
// (vt_plan::sad_split).  Queries past the last are clamped to it and never emitted.
constexpr int SAD_NQ = vt_plan::SAD_NQ, SAD_NW = vt_plan::SAD_NW;

template <int H, bool MATRIX>
__global__ __launch_bounds__(64 * SAD_NW) void vt_scan_sad_kernel(const uint4* __restrict__ lib, int ntb,
                                                                  int64_t count, int WD,
                                                                  const uint32_t* __restrict__ qd, int nq,
                                                                  int nqc, ScanOut out, int rank,
                                                                  int nranks) {
    constexpr int M = FAST_M, HQ = H / 4, NO = 2 * M - 1, R0 = M, R1 = H - M, NQ = SAD_NQ;
    constexpr int CH = 16, NCH = (R1 - R0) / CH;   // query rows a chunk, chunks a column
    static_assert((R1 - R0) % CH == 0, "whole chunks of query rows");
    __shared__ uint32_t s_sum[2][NQ][NO][64];
    const int tb = blockIdx.x % ntb, j = blockIdx.x / ntb;
    const int lane = threadIdx.x & 63, nw = blockDim.x >> 6;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    for (int i = threadIdx.x; i < 2 * NQ * NO * 64; i += blockDim.x) (&s_sum[0][0][0][0])[i] = 0u;
    __syncthreads();
    const int ngroups = (nq + NQ - 1) / NQ;
    const int64_t slot = (int64_t)tb * 64 + lane;
    uint32_t A[H];
    int held = -1;
    int buf = 0;
    for (int g = j; g < ngroups; g += nqc, buf ^= 1) {
        const int qbase = g * NQ;
        uint32_t acc[NQ][NO];
#pragma unroll
        for (int n = 0; n < NQ; ++n)
#pragma unroll
            for (int o = 0; o < NO; ++o) acc[n][o] = 0u;
        for (int c = wave; c < WD; c += nw) {
            if (c != held) {
                const uint4* col = lib + ((size_t)(tb * WD + c) * HQ) * 64 + lane;
#pragma unroll
                for (int q = 0; q < HQ; ++q) {
                    const uint4 v = col[(size_t)q * 64];
                    A[4 * q + 0] = v.x;
                    A[4 * q + 1] = v.y;
                    A[4 * q + 2] = v.z;
                    A[4 * q + 3] = v.w;
                }
                held = c;
            }
            const uint32_t* qrow[NQ];
#pragma unroll
            for (int n = 0; n < NQ; ++n) qrow[n] = qd + ((size_t)min(qbase + n, nq - 1) * WD + c) * H;
            // The query rows come in chunks of CH (one s_load_dwordx16 a query), the next chunk's
            // loads issued ahead of this chunk's v_sad_u8 and no further: left to itself the
            // scheduler hoists every chunk's loads to the top, runs out of SGPRs and spills them
            // through v_writelane / v_readlane, VALU slots of their own (7% of the instructions).
            uint32_t qv[2][NQ][CH];
#pragma unroll
            for (int n = 0; n < NQ; ++n)
#pragma unroll
                for (int i = 0; i < CH; ++i) qv[0][n][i] = qrow[n][R0 + i];
#pragma unroll
            for (int k = 0; k < NCH; ++k) {
                if (k + 1 < NCH) {
#pragma unroll
                    for (int n = 0; n < NQ; ++n)
#pragma unroll
                        for (int i = 0; i < CH; ++i) qv[(k + 1) & 1][n][i] = qrow[n][R0 + (k + 1) * CH + i];
                }
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int i = 0; i < CH; ++i) {
                    const int r = R0 + k * CH + i;
#pragma unroll
                    for (int n = 0; n < NQ; ++n)
#pragma unroll
                        for (int o = 0; o < NO; ++o)
                            acc[n][o] = __builtin_amdgcn_sad_u8(A[r + o - (M - 1)], qv[k & 1][n][i], acc[n][o]);
                }
                __builtin_amdgcn_sched_barrier(0);
            }
        }
#pragma unroll
        for (int n = 0; n < NQ; ++n)
#pragma unroll
            for (int o = 0; o < NO; ++o) atomicAdd(&s_sum[buf][n][o][lane], acc[n][o]);
        __syncthreads();
        for (int n = wave; n < NQ; n += nw) {
            uint32_t sc = 0xFFFFFFFFu;
#pragma unroll
            for (int o = 0; o < NO; ++o) {
                sc = min(sc, s_sum[buf][n][o][lane]);
                s_sum[buf][n][o][lane] = 0u;
            }
            emit_score<MATRIX>(out, slot, count, qbase + n, nq, sc, rank, nranks, lane == 0);
        }
    }
}

// --- generic form (any H, W, max_offset): one thread per (slot, query), the shape of
// vt_scan_generic_kernel.  An empty window (H = 2M) scores 0.
template <bool MATRIX>
__global__ __launch_bounds__(64) void vt_scan_sad_generic_kernel(const uint4* __restrict__ lib, int ntb,
                                                                 int64_t count, int H, int M, int WD,
                                                                 const uint32_t* __restrict__ qd, int nq,
                                                                 ScanOut out, int rank, int nranks) {
    const int HQ = (H + 3) / 4;
    const int tb = blockIdx.x % ntb;
    const int qi = blockIdx.x / ntb;
    const int lane = threadIdx.x;
    const uint32_t* base = reinterpret_cast<const uint32_t*>(lib);
    uint32_t best = 0xFFFFFFFFu;
    for (int o = -(M - 1); o <= M - 1; ++o) {
        uint32_t acc = 0;
        for (int r = M; r < H - M; ++r) {
            const int s = r + o;
            for (int c = 0; c < WD; ++c) {
                const size_t chunk = ((size_t)(tb * WD + c) * HQ + (s >> 2)) * 64 + lane;
                acc = __builtin_amdgcn_sad_u8(base[chunk * 4 + (s & 3)], qd[((size_t)qi * WD + c) * H + r], acc);
            }
        }
        best = min(best, acc);
    }
    emit_score<MATRIX>(out, (int64_t)tb * 64 + lane, count, qi, nq, best, rank, nranks, lane == 0);
}
