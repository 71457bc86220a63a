// Patch normalisation of raw uint8 images on the device (rs_vt_set_normalise, DESIGN
// section 33), included by view_templates.hip.  The rule is vt_norm_rule.h.
//
// vt_normalise_kernel reads n raw H x W images from src and writes n normalised images to
// dst, a distinct buffer (never in place: a tile's halo is another tile's output).
//
// An image is cut into VTN_T x VTN_T output tiles; a block of 256 threads does one tile of
// one image, and the next image gridDim.y further on.  Three phases, a barrier between:
//   1. the tile and its halo of R pixels, (VTN_T + 2R)^2 bytes at most, go into LDS, each
//      source byte read once per tile, bytes outside the image as 0.  A zero adds nothing to
//      S or S2, and n is counted from the clamped window (vtn_extent), so the window is
//      clamped, not padded.  Byte reads: a raw row is not dword-aligned when W mod 4 != 0, and
//      no address outside the image is formed (the source may be pinned host memory);
//   2. row sums: for every staged row and output column the 2R + 1 bytes' sum and square sum
//      (uint32 each) into LDS;
//   3. column sums: an output pixel adds 2R + 1 row sums of its column, and the rule's
//      vtn_pixel gives the byte, stored with a byte store (32 consecutive bytes a row).
// Separable sums cost 2 (2R + 1) LDS reads of each kind a pixel where the direct window
// costs (2R + 1)^2: 30 against 225 at R = 7.  In phase 3 the lanes of a half-wave read
// consecutive dwords of one row of sums (bank = column, conflict-free); in phase 2 four lanes
// share each dword of staged bytes (a broadcast).  The LDS footprint is fixed by the tile:
// VTN_S * VTN_STRIDE bytes + 2 * VTN_S * VTN_T dwords = 13,984 bytes at any shape.
// No scratch, no atomics, no LDS-DMA.
// (view_templates.hip includes vt_norm_rule.h at file scope, ahead of its own namespace.)
#pragma once

constexpr int VTN_T = 32;                              // output tile side
constexpr int VTN_S = VTN_T + 2 * rs::VTN_MAX_RADIUS;  // staged rows / columns at most
constexpr int VTN_STRIDE = 48;                         // bytes a staged row (>= VTN_S, dwords)
constexpr int VTN_THREADS = 256;
static_assert(VTN_STRIDE >= VTN_S && VTN_STRIDE % 4 == 0, "a staged row holds the tile and both halos");

__global__ __launch_bounds__(VTN_THREADS) void vt_normalise_kernel(const uint8_t* __restrict__ src,
                                                                   uint8_t* __restrict__ dst, int n, int H, int W,
                                                                   int R, int G, int tiles_x) {
    __shared__ uint8_t raw[VTN_S * VTN_STRIDE];
    __shared__ uint32_t rowS[VTN_S * VTN_T], rowS2[VTN_S * VTN_T];
    const int tid = threadIdx.x;
    const int ty = (int)blockIdx.x / tiles_x, tx = (int)blockIdx.x - ty * tiles_x;
    const int r0 = ty * VTN_T, c0 = tx * VTN_T;
    const int th = min(VTN_T, H - r0), tw = min(VTN_T, W - c0);   // output rows / columns of this tile
    const int sh = th + 2 * R, sw = tw + 2 * R;                   // staged rows / columns (<= VTN_S)
    const size_t image = (size_t)H * W;
    for (int im = blockIdx.y; im < n; im += gridDim.y) {
        const uint8_t* const p = src + image * im;
        for (int i = tid; i < sh * sw; i += VTN_THREADS) {
            const int lr = i / sw, lc = i - lr * sw;
            const int gr = r0 - R + lr, gc = c0 - R + lc;
            uint8_t v = 0;
            if (gr >= 0 && gr < H && gc >= 0 && gc < W) v = p[(size_t)gr * W + gc];
            raw[lr * VTN_STRIDE + lc] = v;
        }
        __syncthreads();
        for (int i = tid; i < sh * VTN_T; i += VTN_THREADS) {
            const int lr = i / VTN_T, oc = i % VTN_T;
            if (oc >= tw) continue;
            uint32_t a = 0, b = 0;
            for (int k = 0; k <= 2 * R; ++k) {
                const uint32_t v = raw[lr * VTN_STRIDE + oc + k];
                a += v;
                b += v * v;
            }
            rowS[i] = a;
            rowS2[i] = b;
        }
        __syncthreads();
        uint8_t* const o = dst + image * im;
        for (int i = tid; i < th * VTN_T; i += VTN_THREADS) {
            const int orow = i / VTN_T, oc = i % VTN_T;
            if (oc >= tw) continue;
            uint32_t S = 0, S2 = 0;
            for (int k = 0; k <= 2 * R; ++k) {
                S += rowS[(orow + k) * VTN_T + oc];
                S2 += rowS2[(orow + k) * VTN_T + oc];
            }
            const int r = r0 + orow, c = c0 + oc;
            o[(size_t)r * W + c] = rs::vtn_pixel(rs::vtn_extent(r, H, R) * rs::vtn_extent(c, W, R), S, S2,
                                                 raw[(orow + R) * VTN_STRIDE + oc + R], (uint32_t)G);
        }
        __syncthreads();   // (the next image's phase 1 overwrites raw)
    }
}
