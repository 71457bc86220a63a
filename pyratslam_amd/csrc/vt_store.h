// Byte-layout library store, on-device subsampling and the byte-SWAR query forms.
// Part of view_templates.hip, the one translation unit: not free-standing (it relies on the
// includes, the anonymous namespace and the headers that view_templates.hip includes before it).
#pragma once

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
