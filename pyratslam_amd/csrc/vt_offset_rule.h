// The row-offset profile of one (template, query) pair of the uint8 view-template matcher
// (DESIGN section 30), shared by the lanes of vt_offset_profile_kernel (vt_offset.h), by
// rs_vt_offset_profile_host and by tests/vt_offset_main.cpp.
//
//   profile[k] = sum_{r = M .. H-M-1, c} term(T[r + o][c], Q[r][c]),  o = k - (M - 1),
//   k = 0 .. 2M-2;  term = (T - Q) mod 256 (RS_VT_METRIC_WRAPPED) or |T - Q|
//   (RS_VT_METRIC_SAD), on the bytes as integers, summed as uint32 (rs_vt_create's bound
//   H * W * 255 < 2^32 - 1 keeps every entry below UINT32_MAX);
//   offset = o of the first k whose profile[k] is minimal: ViewTemplate.match's strict `<`
//   from -M+1 upwards (view_templates.py:19-27), which only keeps the value.
// An empty window (H == 2M) gives an all-zero profile and offset -(M - 1).
//
// The terms are per dword: four byte pairs at once, bytes past W zero on both sides
// (term(0, 0) = 0 under either metric).
#pragma once

#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#define VTO_HD __host__ __device__
#else
#define VTO_HD
#endif

namespace rs {

constexpr int VTO_METRIC_WRAPPED = 0, VTO_METRIC_SAD = 1;   // RS_VT_METRIC_* (ratslam_abi.h)

// acc + the sum of |a_b - b_b| over the four bytes b: v_sad_u8 on the device.
VTO_HD inline uint32_t vto_sad_u8(uint32_t a, uint32_t b, uint32_t acc) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_sad_u8(a, b, acc);
#else
    for (int i = 0; i < 4; ++i) {
        const uint32_t x = (a >> (8 * i)) & 0xFFu, y = (b >> (8 * i)) & 0xFFu;
        acc += x > y ? x - y : y - x;
    }
    return acc;
#endif
}

// The byte-wise difference (t_b - q_b) mod 256 of two dwords, carry-free: with bit 7 of
// every byte of t set and of q cleared no byte borrows from its neighbour, the low seven
// bits are then right, and bit 7 is t7 ^ q7 ^ borrow, where the subtraction left 1 ^ borrow.
VTO_HD inline uint32_t vto_bytes_sub(uint32_t t, uint32_t q) {
    constexpr uint32_t HI = 0x80808080u;
    return ((t | HI) - (q & ~HI)) ^ ((t ^ ~q) & HI);
}

// acc + the four terms of template dword t against query dword q.
VTO_HD inline uint32_t vto_term_sad(uint32_t t, uint32_t q, uint32_t acc) { return vto_sad_u8(t, q, acc); }
VTO_HD inline uint32_t vto_term_wrapped(uint32_t t, uint32_t q, uint32_t acc) {
    return vto_sad_u8(vto_bytes_sub(t, q), 0u, acc);
}
template <int METRIC>
VTO_HD inline uint32_t vto_term(uint32_t t, uint32_t q, uint32_t acc) {
    return METRIC == VTO_METRIC_SAD ? vto_term_sad(t, q, acc) : vto_term_wrapped(t, q, acc);
}

// The running first argmin: entry k of value v after the entries before it.
VTO_HD inline void vto_pick(uint32_t v, int k, uint32_t& best, int& best_k) {
    if (k == 0 || v < best) {
        best = v;
        best_k = k;
    }
}

// The offset of a whole profile of 2M - 1 entries.
VTO_HD inline int32_t vto_first_argmin(const uint32_t* profile, int M) {
    uint32_t best = 0;
    int best_k = 0;
    for (int k = 0; k < 2 * M - 1; ++k) vto_pick(profile[k], k, best, best_k);
    return best_k - (M - 1);
}

// The dword of bytes 4c .. 4c+3 of a raw row of W bytes, bytes past W zero.  Byte reads:
// a row of a raw image is not dword-aligned when W mod 4 != 0, and no address outside the
// row is formed.
VTO_HD inline uint32_t vto_row_dword(const uint8_t* row, int W, int c) {
    uint32_t d = 0;
    for (int b = 0; b < 4; ++b) {
        const int col = 4 * c + b;
        if (col < W) d |= (uint32_t)row[col] << (8 * b);
    }
    return d;
}

// The rule on the host: raw row-major H x W template and query, profile[2M - 1].
inline int32_t vto_profile_host(int metric, int H, int W, int M, const uint8_t* T, const uint8_t* Q,
                                uint32_t* profile) {
    const int WD = (W + 3) / 4;
    for (int k = 0; k < 2 * M - 1; ++k) {
        const int o = k - (M - 1);
        uint32_t acc = 0;
        for (int r = M; r < H - M; ++r)
            for (int c = 0; c < WD; ++c) {
                const uint32_t t = vto_row_dword(T + (size_t)(r + o) * W, W, c);
                const uint32_t q = vto_row_dword(Q + (size_t)r * W, W, c);
                acc = metric == VTO_METRIC_SAD ? vto_term_sad(t, q, acc) : vto_term_wrapped(t, q, acc);
            }
        profile[k] = acc;
    }
    return vto_first_argmin(profile, M);
}

}  // namespace rs
