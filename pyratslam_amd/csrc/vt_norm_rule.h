// Patch normalisation of a uint8 image, shared by vt_normalise_kernel
// (vt_norm.h), by rs_vt_normalise_host and by tests/vt_norm_main.cpp.
//
// For an H x W image p, radius R and gain G, at pixel (r, c):
//   window = rows max(0, r-R) .. min(H-1, r+R) x columns max(0, c-R) .. min(W-1, c+R)
//            (clamped to the image, never padded; a small image uses all of itself),
//   n = window pixels, S = sum p, S2 = sum p^2 over it,
//   D = n * S2 - S^2,  N = n * p[r][c] - S,  s = isqrt(D)   (n^2 x the variance; n x the
//   deviation from the mean; the floor square root, exact),
//   out = 128                                          if s == 0,
//         clamp(128 + sign(N) * ((G * |N| + s / 2) / s), 0, 255)   otherwise:
// the pixel in units of its neighbourhood's standard deviation, G levels per unit, rounded
// to nearest, around mid-grey.  A constant added to p changes neither N nor D; a positive
// factor scales both alike.
//
// Everything is an integer, so the device, the host and NumPy (normalise_u8) agree bit for
// bit.  Bounds, with 1 <= R <= 7 and 1 <= G <= 127: n <= 15^2 = 225; n * S2 <= 225^2 * 255^2
// = 3,291,890,625 < 2^32 and S^2 <= n * S2 (Cauchy-Schwarz), so D fits uint32 and is never
// negative; |N| <= 225 * 255 = 57,375 and G * |N| + s / 2 <= 127 * 57,375 + 32,767 < 2^23.
// Every intermediate fits uint32.
#pragma once

#include <cmath>
#include <cstddef>
#include <cstdint>
#include <vector>

#if defined(__HIPCC__)
#define VTN_HD __host__ __device__
#else
#define VTN_HD
#endif

namespace rs {

constexpr int VTN_MAX_RADIUS = 7, VTN_MAX_GAIN = 127;

// floor(sqrt(D)).  The float square root is only an estimate (a float holds 24 of D's 32
// bits); the integer steps end at s^2 <= D < (s + 1)^2, written as D - s^2 >= 2s + 1 so
// that nothing exceeds 32 bits at s = 65535.
VTN_HD inline uint32_t vtn_isqrt(uint32_t D) {
    uint32_t s = (uint32_t)sqrtf((float)D);
    if (s > 65535u) s = 65535u;
    while (s * s > D) --s;
    while (D - s * s >= 2u * s + 1u) ++s;
    return s;
}

// Rows (or columns) of the clamped window around index i of an axis of length L.
VTN_HD inline uint32_t vtn_extent(int i, int L, int R) {
    const int lo = i - R < 0 ? 0 : i - R, hi = i + R > L - 1 ? L - 1 : i + R;
    return (uint32_t)(hi - lo + 1);
}

// The output byte of a pixel p whose window holds n pixels of sum S and square sum S2.
VTN_HD inline uint8_t vtn_pixel(uint32_t n, uint32_t S, uint32_t S2, uint32_t p, uint32_t G) {
    const uint32_t s = vtn_isqrt(n * S2 - S * S);
    if (s == 0u) return 128u;
    const uint32_t np = n * p;
    const bool neg = np < S;
    const uint32_t q = (G * (neg ? S - np : np - S) + s / 2u) / s;
    if (neg) return (uint8_t)(q >= 128u ? 0u : 128u - q);
    return (uint8_t)(q >= 127u ? 255u : 128u + q);
}

// The rule on the host: row-major H x W bytes src -> dst (distinct).  Separable sums: the
// window's row sums of every pixel, then their column sums.
inline void vtn_normalise_host(int H, int W, int R, int G, const uint8_t* src, uint8_t* dst) {
    std::vector<uint32_t> rs((size_t)H * W), rs2((size_t)H * W);
    for (int r = 0; r < H; ++r)
        for (int c = 0; c < W; ++c) {
            uint32_t a = 0, b = 0;
            for (int k = (c - R < 0 ? 0 : c - R); k <= (c + R > W - 1 ? W - 1 : c + R); ++k) {
                const uint32_t v = src[(size_t)r * W + k];
                a += v;
                b += v * v;
            }
            rs[(size_t)r * W + c] = a;
            rs2[(size_t)r * W + c] = b;
        }
    for (int r = 0; r < H; ++r)
        for (int c = 0; c < W; ++c) {
            uint32_t S = 0, S2 = 0;
            for (int k = (r - R < 0 ? 0 : r - R); k <= (r + R > H - 1 ? H - 1 : r + R); ++k) {
                S += rs[(size_t)k * W + c];
                S2 += rs2[(size_t)k * W + c];
            }
            dst[(size_t)r * W + c] =
                vtn_pixel(vtn_extent(r, H, R) * vtn_extent(c, W, R), S, S2, src[(size_t)r * W + c], (uint32_t)G);
        }
}

}  // namespace rs
