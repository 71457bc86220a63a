// Scanline visual odometer on MI355X (gfx950).
//
// Replaces the module the reference's ROS node imports but does not ship:
// `from visual_odometer import SimpleVisualOdometer` (ros_simulate.py:5), constructed
// at :90, `delta = self.vis_odom.update(im)` per frame (:119-122), the deltas fed to
// update_posecells (:163-165).  The arithmetic is the scanline-profile odometer in
// exact integers (pyratslam_amd/visual_odometer.py is the NumPy restatement):
//
//   profile   prof[c] = sum_{y in [y0, y1)} frame[y][x0 + c]                   (uint32)
//   table     tab[s]  = sum_k |cur[k] - prev[k + s]|,  s in [-(S-1), S-1],     (uint32)
//             over the Wd - |s| values of k with both indices valid
//   select    first strict minimum of tab[s] / ((Wd - |s|) * R * 255) in float64,
//             candidates ordered 0, -1, +1, -2, +2, ...                        (host)
//
// Two regions per frame (`trans`, `rot`).  vo_profile_kernel is one streaming pass
// over the region's bytes; vo_shift_kernel is one block per (frame, region).  When
// the two regions are the same rectangle (the default) the frame is read once and
// the sums are stored to both profile slots; otherwise each region is a pass of its
// own and rows they share are read a second time (from L2 when the frame fits).
//
// Device layouts:  profiles [nf][Wd_trans + Wd_rot] uint32 (trans first),
//                  tables   [nf][2][2S - 1] uint32, tab index s + (S - 1).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstring>

#include "rs_common.h"

namespace {

constexpr int VO_THREADS = 256;
constexpr int VO_GROUPS = 64;         // 16-byte column groups per block (1 KiB of a row)
constexpr int VO_FLUSH = 256;         // rows per 16-bit partial sum: 256 * 255 < 2^16 (257 at most)
constexpr int VO_CHUNK_FRAMES = 256;  // host frames staged per chunk (visual_odometer.CHUNK_FRAMES)
constexpr int VO_LDS_WIDTH = 4096;    // widest profile pair vo_shift_kernel keeps in LDS

struct VoRegion {
    int y0, y1, x0, x1;
};

// Column sums of one region of each frame, 16-byte loads.  Needs the frame base and
// the pitch 16-byte aligned.  A block takes up to 64 aligned 16-column groups covering
// [x0, x1) (columns outside are dropped at the store) and all rows; thread t reads
// group t % gp of rows y0 + t / gp, + 256 / gp, ... (gp = groups rounded up to a power
// of two), so a wave's load is whole 16-byte pieces of consecutive rows.  Bytes are
// summed as 16-bit SWAR pairs, flushed to 32 bits every VO_FLUSH rows; the row lanes
// are reduced through LDS.
__global__ __launch_bounds__(VO_THREADS) void vo_profile_kernel(
    const uint8_t* __restrict__ frames, size_t frame_bytes, int pitch, VoRegion r0, VoRegion r1,
    int same, uint32_t* __restrict__ prof, int prof_stride) {
    __shared__ __attribute__((aligned(16))) uint32_t red[VO_THREADS * 16];
    const int reg = blockIdx.z;
    const VoRegion rg = reg ? r1 : r0;
    const int ax0 = rg.x0 & ~15;
    const int G = (rg.x1 - ax0 + 15) >> 4;
    const int g0 = blockIdx.y * VO_GROUPS;
    if (g0 >= G) return;  // (the other region is wider)
    const int ng = min(G - g0, VO_GROUPS);
    int lg = 0;
    while ((1 << lg) < ng) ++lg;
    const int gp = 1 << lg, rpi = VO_THREADS >> lg;
    const int tid = threadIdx.x;
    const int g = tid & (gp - 1), r = tid >> lg;
    const uint8_t* p = frames + (size_t)blockIdx.x * frame_bytes + ax0 + (size_t)(g0 + g) * 16;

    uint32_t s[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) s[i] = 0;
    if (g < ng) {
        int y = rg.y0 + r;
        while (y < rg.y1) {
            const int n = min(VO_FLUSH, (rg.y1 - y + rpi - 1) / rpi);
            uint32_t a[8];
#pragma unroll
            for (int i = 0; i < 8; ++i) a[i] = 0;
#pragma unroll 8
            for (int i = 0; i < n; ++i) {
                const uint4 v = *reinterpret_cast<const uint4*>(p + (size_t)(y + i * rpi) * pitch);
                a[0] += v.x & 0x00ff00ffu; a[1] += (v.x >> 8) & 0x00ff00ffu;
                a[2] += v.y & 0x00ff00ffu; a[3] += (v.y >> 8) & 0x00ff00ffu;
                a[4] += v.z & 0x00ff00ffu; a[5] += (v.z >> 8) & 0x00ff00ffu;
                a[6] += v.w & 0x00ff00ffu; a[7] += (v.w >> 8) & 0x00ff00ffu;
            }
            y += n * rpi;
#pragma unroll
            for (int j = 0; j < 4; ++j) {  // dword j, bytes 0 2 in a[2j], bytes 1 3 in a[2j+1]
                s[4 * j + 0] += a[2 * j] & 0xffffu;
                s[4 * j + 2] += a[2 * j] >> 16;
                s[4 * j + 1] += a[2 * j + 1] & 0xffffu;
                s[4 * j + 3] += a[2 * j + 1] >> 16;
            }
        }
    }
    // red[r][g * 16 + c], rows of gp * 16 columns: rpi * gp * 16 = 4096 words
    uint4* dst = reinterpret_cast<uint4*>(red + ((size_t)r * gp + g) * 16);
#pragma unroll
    for (int j = 0; j < 4; ++j) dst[j] = make_uint4(s[4 * j], s[4 * j + 1], s[4 * j + 2], s[4 * j + 3]);
    __syncthreads();
    const int ncol = ng * 16, row = gp * 16;
    uint32_t* out = prof + (size_t)blockIdx.x * prof_stride;
    const int off = reg ? (r0.x1 - r0.x0) : 0;
    for (int c = tid; c < ncol; c += VO_THREADS) {
        uint32_t t = 0;
        for (int k = 0; k < rpi; ++k) t += red[k * row + c];
        const int x = ax0 + g0 * 16 + c;
        if (x >= rg.x0 && x < rg.x1) {
            out[off + x - rg.x0] = t;
            if (same) out[(r0.x1 - r0.x0) + x - rg.x0] = t;
        }
    }
}

// The same sums byte by byte: any base, any pitch.  One thread per column.
__global__ __launch_bounds__(VO_THREADS) void vo_profile_bytes_kernel(
    const uint8_t* __restrict__ frames, size_t frame_bytes, int pitch, VoRegion r0, VoRegion r1,
    int same, uint32_t* __restrict__ prof, int prof_stride) {
    const int reg = blockIdx.z;
    const VoRegion rg = reg ? r1 : r0;
    const int c = blockIdx.y * VO_THREADS + threadIdx.x;
    if (c >= rg.x1 - rg.x0) return;
    const uint8_t* p = frames + (size_t)blockIdx.x * frame_bytes + rg.x0 + c;
    uint32_t t = 0;
    for (int y = rg.y0; y < rg.y1; ++y) t += p[(size_t)y * pitch];
    uint32_t* out = prof + (size_t)blockIdx.x * prof_stride;
    out[(reg ? (r0.x1 - r0.x0) : 0) + c] = t;
    if (same) out[(r0.x1 - r0.x0) + c] = t;
}

__device__ inline uint32_t wave_sum_u32(uint32_t v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

// Shift table of one (frame, region) per block: cur and prev profiles in LDS (profiles
// wider than VO_LDS_WIDTH are read in place), the 2S-1 shifts over the 4 waves, lanes
// striding over k, one wave reduction per shift.  prev = the frame before, or the
// handle's carried profile for frame 0; a frame with no predecessor gets a zero table.
template <bool LDS>
__global__ __launch_bounds__(VO_THREADS) void vo_shift_kernel(
    const uint32_t* __restrict__ prof, int prof_stride, const uint32_t* __restrict__ carry,
    int wd0, int wd1, int S, int same, uint32_t* __restrict__ tab) {
    extern __shared__ uint32_t sh[];
    const int f = blockIdx.x, reg = blockIdx.y, tid = threadIdx.x;
    const int wd = reg ? wd1 : wd0, off = reg ? wd0 : 0;
    const int nt = 2 * S - 1;
    uint32_t* out = tab + ((size_t)f * 2 + reg) * nt;
    uint32_t* out2 = same ? out + nt : nullptr;
    const uint32_t* cur = prof + (size_t)f * prof_stride + off;
    const uint32_t* prev = f > 0 ? cur - prof_stride : (carry ? carry + off : nullptr);
    if (!prev) {
        for (int j = tid; j < nt; j += VO_THREADS) {
            out[j] = 0;
            if (out2) out2[j] = 0;
        }
        return;
    }
    const uint32_t *c = cur, *p = prev;
    if (LDS) {
        for (int k = tid; k < wd; k += VO_THREADS) {
            sh[k] = cur[k];
            sh[wd + k] = prev[k];
        }
        __syncthreads();
        c = sh;
        p = sh + wd;
    }
    const int wave = tid >> 6, lane = tid & 63;
    for (int j = wave; j < nt; j += VO_THREADS / 64) {
        const int s = j - (S - 1);
        const int k0 = max(0, -s), k1 = min(wd, wd - s);
        uint32_t acc = 0;
        for (int k = k0 + lane; k < k1; k += 64) {
            const uint32_t a = c[k], b = p[k + s];
            acc += a > b ? a - b : b - a;
        }
        acc = wave_sum_u32(acc);
        if (lane == 0) {
            out[j] = acc;
            if (out2) out2[j] = acc;
        }
    }
}

// Selection rule (file header): candidates 0, -1, +1, -2, +2, ...; one correctly rounded
// float64 division each; strict <, so a tie keeps the smaller |s| and -s before +s.
void vo_select(int S, int wd, int rows, const uint32_t* tab, int* shift, double* mindiff) {
    double best = __builtin_inf();
    int sh = 0;
    for (int o = 0; o < S; ++o) {
        const double den = (double)((int64_t)(wd - o) * rows * 255);
        for (int sgn = -1; sgn <= 1; sgn += 2) {
            if (o == 0 && sgn > 0) break;
            const int s = sgn * o;
            const double v = (double)tab[s + S - 1] / den;
            if (v < best) {
                best = v;
                sh = s;
            }
        }
    }
    *shift = sh;
    *mindiff = best;
}

int vo_check_params(int im_h, int im_w, const rs_vo_params* p) {
    RS_CHECK(p, RS_ERR_ARG, "null odometer parameters");
    RS_CHECK(im_h > 0 && im_w > 0, RS_ERR_ARG, "bad frame shape (%d, %d)", im_h, im_w);
    RS_CHECK(p->max_shift >= 1 && p->max_shift <= 64, RS_ERR_ARG, "max_shift %d outside [1, 64]",
             p->max_shift);
    const int b[2][4] = {{p->trans_y0, p->trans_y1, p->trans_x0, p->trans_x1},
                         {p->rot_y0, p->rot_y1, p->rot_x0, p->rot_x1}};
    for (int r = 0; r < 2; ++r) {
        const char* name = r ? "rot" : "trans";
        RS_CHECK(b[r][0] >= 0 && b[r][0] < b[r][1] && b[r][1] <= im_h, RS_ERR_ARG,
                 "%s rows [%d, %d) empty or outside [0, %d)", name, b[r][0], b[r][1], im_h);
        RS_CHECK(b[r][2] >= 0 && b[r][2] < b[r][3] && b[r][3] <= im_w, RS_ERR_ARG,
                 "%s columns [%d, %d) empty or outside [0, %d)", name, b[r][2], b[r][3], im_w);
        const int64_t R = b[r][1] - b[r][0], wd = b[r][3] - b[r][2];
        RS_CHECK(wd >= p->max_shift, RS_ERR_ARG, "%s region is %lld columns wide, fewer than max_shift %d",
                 name, (long long)wd, p->max_shift);
        RS_CHECK(R * 255 * wd < (int64_t)1 << 32, RS_ERR_ARG,
                 "%s region: rows * 255 * columns = %lld does not fit 32 bits", name, (long long)(R * 255 * wd));
    }
    return RS_OK;
}

}  // namespace

// The buffers are rs::DevBuf / rs::PinnedBuf members (rs_common.h).  Group capacities, in
// frames: cap (dProf, dTab, hTab) and frameCap (dFrames, hFrames).  The stream and the events
// are rs::Stream / rs::Event owners.
struct rs_vo {
    int device = 0, H = 0, W = 0, S = 0;
    rs_vo_params p{};
    VoRegion reg[2]{};
    int wd[2]{}, rows[2]{};
    bool same = false;
    rs::DevBuf<uint8_t> dFrames;
    rs::PinnedBuf<uint8_t> hFrames;
    int frameCap = 0;
    rs::DevBuf<uint32_t> dProf, dTab, dCarry;
    rs::PinnedBuf<uint32_t> hTab;
    int cap = 0;
    bool hasCarry = false, timing = false, timed = false;
    float ms[2] = {0, 0};
    // the owners come after the buffers: members go in reverse order, streams and events first
    rs::Stream stream;
    rs::Event ev[3];
};

namespace {

int vo_grow(rs_vo* h, int n, bool staging) {
    const size_t ps = (size_t)h->wd[0] + h->wd[1], nt = 2 * (size_t)(2 * h->S - 1);
    if (n > h->cap) {
        const int cap = rs::grown(h->cap, n, 1);
        h->cap = 0;
        RS_TRY(h->dProf.reserve(ps * cap));
        RS_TRY(h->dTab.reserve(nt * cap));
        RS_TRY(h->hTab.reserve(nt * cap, hipHostMallocDefault));
        h->cap = cap;
    }
    if (staging && n > h->frameCap) {
        const int cap = rs::grown(h->frameCap, n, 1);
        const size_t fb = (size_t)h->H * h->W;
        h->frameCap = 0;
        RS_TRY(h->dFrames.reserve(fb * cap));
        RS_TRY(h->hFrames.reserve(fb * cap, hipHostMallocDefault));
        h->frameCap = cap;
    }
    return RS_OK;
}

// Queue the two kernels for n device frames at src (frame 0's predecessor: the carry).
int vo_launch(rs_vo* h, int n, const uint8_t* src, bool timed) {
    const size_t fb = (size_t)h->H * h->W;
    const int ps = h->wd[0] + h->wd[1], nreg = h->same ? 1 : 2;
    const bool vec = (reinterpret_cast<uintptr_t>(src) & 15) == 0 && h->W % 16 == 0;
    if (timed) RS_HIP(hipEventRecord(h->ev[0].get(), h->stream.get()));
    if (vec) {
        int tiles = 1;
        for (int r = 0; r < nreg; ++r) {
            const int G = (h->reg[r].x1 - (h->reg[r].x0 & ~15) + 15) / 16;
            tiles = std::max(tiles, (G + VO_GROUPS - 1) / VO_GROUPS);
        }
        hipLaunchKernelGGL(vo_profile_kernel, dim3(n, tiles, nreg), dim3(VO_THREADS), 0, h->stream.get(), src,
                           fb, h->W, h->reg[0], h->reg[1], (int)h->same, h->dProf.get(), ps);
    } else {
        const int wmax = std::max(h->wd[0], h->wd[1]);
        hipLaunchKernelGGL(vo_profile_bytes_kernel, dim3(n, (wmax + VO_THREADS - 1) / VO_THREADS, nreg),
                           dim3(VO_THREADS), 0, h->stream.get(), src, fb, h->W, h->reg[0], h->reg[1],
                           (int)h->same, h->dProf.get(), ps);
    }
    RS_HIP(hipGetLastError());
    if (timed) RS_HIP(hipEventRecord(h->ev[1].get(), h->stream.get()));
    const uint32_t* carry = h->hasCarry ? h->dCarry.get() : nullptr;
    const int wmax = std::max(h->wd[0], h->wd[1]);
    if (wmax <= VO_LDS_WIDTH)
        hipLaunchKernelGGL(vo_shift_kernel<true>, dim3(n, nreg), dim3(VO_THREADS),
                           sizeof(uint32_t) * 2 * wmax, h->stream.get(), h->dProf.get(), ps, carry, h->wd[0],
                           h->wd[1], h->S, (int)h->same, h->dTab.get());
    else
        hipLaunchKernelGGL(vo_shift_kernel<false>, dim3(n, nreg), dim3(VO_THREADS), 0, h->stream.get(),
                           h->dProf.get(), ps, carry, h->wd[0], h->wd[1], h->S, (int)h->same, h->dTab.get());
    RS_HIP(hipGetLastError());
    if (timed) RS_HIP(hipEventRecord(h->ev[2].get(), h->stream.get()));
    return RS_OK;
}

}  // namespace

extern "C" {

int rs_vo_select(int max_shift, int width, int rows, const uint32_t* table, int* shift,
                 double* mindiff) {
    rs::clear_error();
    RS_CHECK(table && shift && mindiff, RS_ERR_ARG, "null argument");
    RS_CHECK(max_shift >= 1 && max_shift <= 64, RS_ERR_ARG, "max_shift %d outside [1, 64]", max_shift);
    RS_CHECK(rows >= 1 && width >= max_shift && (int64_t)rows * 255 * width < (int64_t)1 << 32,
             RS_ERR_ARG, "bad region (%d rows, %d columns) for max_shift %d", rows, width, max_shift);
    vo_select(max_shift, width, rows, table, shift, mindiff);
    return RS_OK;
}

int rs_vo_create(int im_h, int im_w, const rs_vo_params* params, int device, rs_vo** out) {
    rs::clear_error();
    RS_CHECK(out, RS_ERR_ARG, "null output handle pointer");
    *out = nullptr;
    RS_TRY(vo_check_params(im_h, im_w, params));  // (before any device call: checked without a GPU)
    RS_TRY(rs::use_device(device));
    // one failure exit: rs_vo_destroy takes a handle at any stage
    std::unique_ptr<rs_vo, int (*)(rs_vo*)> owner(new rs_vo(), rs_vo_destroy);
    rs_vo* const h = owner.get();
    h->device = device; h->H = im_h; h->W = im_w; h->S = params->max_shift; h->p = *params;
    h->reg[0] = {params->trans_y0, params->trans_y1, params->trans_x0, params->trans_x1};
    h->reg[1] = {params->rot_y0, params->rot_y1, params->rot_x0, params->rot_x1};
    for (int r = 0; r < 2; ++r) {
        h->wd[r] = h->reg[r].x1 - h->reg[r].x0;
        h->rows[r] = h->reg[r].y1 - h->reg[r].y0;
    }
    h->same = std::memcmp(&h->reg[0], &h->reg[1], sizeof(VoRegion)) == 0;
    RS_TRY(h->stream.create());
    for (rs::Event& e : h->ev) RS_TRY(e.create());
    RS_TRY(h->dCarry.reserve((size_t)h->wd[0] + h->wd[1]));
    RS_TRY(vo_grow(h, 1, true));
    *out = owner.release();
    return RS_OK;
}

int rs_vo_destroy(rs_vo* h) {
    if (!h) return RS_OK;
    (void)hipSetDevice(h->device);
    // queued work that failed after a call returned is reported here, not dropped
    const hipError_t se = rs::sync_streams({h->stream.get()});
    delete h;  // (the streams and events, then the buffers, go with their members)
    RS_CHECK(se == hipSuccess, RS_ERR_HIP, "work queued before rs_vo_destroy failed: %s", hipGetErrorString(se));
    return RS_OK;
}

int rs_vo_reset(rs_vo* h) {
    rs::clear_error();
    RS_CHECK(h, RS_ERR_STATE, "null odometer handle");
    h->hasCarry = false;
    return RS_OK;
}

int rs_vo_run(rs_vo* h, int nf, const uint8_t* frames, double* deltas, uint32_t* tables,
              uint32_t* profiles) {
    rs::clear_error();
    RS_CHECK(h, RS_ERR_STATE, "null odometer handle");
    RS_CHECK(nf >= 0, RS_ERR_ARG, "negative frame count");
    if (nf == 0) return RS_OK;
    RS_CHECK(frames && deltas, RS_ERR_ARG, "null argument");
    RS_HIP(hipSetDevice(h->device));
    const bool on_device = rs::on_device(frames);
    // device-resident frames are read in place in one pass; host frames are staged
    // through the pinned buffer VO_CHUNK_FRAMES at a time
    const int chunk = on_device ? nf : std::min(nf, VO_CHUNK_FRAMES);
    RS_TRY(vo_grow(h, chunk, !on_device));
    const bool timed = h->timing && chunk == nf;
    h->timed = false;
    const size_t fb = (size_t)h->H * h->W, ps = (size_t)h->wd[0] + h->wd[1];
    const size_t nt = 2 * h->S - 1;
    for (int c0 = 0; c0 < nf; c0 += chunk) {
        const int n = std::min(chunk, nf - c0);
        const uint8_t* src = frames + fb * c0;
        if (!on_device) {
            std::memcpy(h->hFrames.get(), src, fb * n);
            RS_HIP(hipMemcpyAsync(h->dFrames.get(), h->hFrames.get(), fb * n, hipMemcpyHostToDevice, h->stream.get()));
            src = h->dFrames.get();
        }
        const bool first = !h->hasCarry;  // frame c0 has no predecessor
        RS_TRY(vo_launch(h, n, src, timed));
        RS_HIP(hipMemcpyAsync(h->dCarry.get(), h->dProf.get() + ps * (n - 1), sizeof(uint32_t) * ps,
                              hipMemcpyDeviceToDevice, h->stream.get()));
        h->hasCarry = true;
        RS_HIP(hipMemcpyAsync(h->hTab.get(), h->dTab.get(), sizeof(uint32_t) * 2 * nt * n, hipMemcpyDeviceToHost,
                              h->stream.get()));
        RS_HIP(hipStreamSynchronize(h->stream.get()));
        if (timed) {
            RS_HIP(hipEventElapsedTime(&h->ms[0], h->ev[0].get(), h->ev[1].get()));
            RS_HIP(hipEventElapsedTime(&h->ms[1], h->ev[1].get(), h->ev[2].get()));
            h->timed = true;
        }
        if (profiles)
            RS_HIP(hipMemcpy(profiles + ps * c0, h->dProf.get(), sizeof(uint32_t) * ps * n, hipMemcpyDeviceToHost));
        if (tables) std::memcpy(tables + 2 * nt * c0, h->hTab.get(), sizeof(uint32_t) * 2 * nt * n);
        for (int i = 0; i < n; ++i) {
            double* d = deltas + 2 * (size_t)(c0 + i);
            if (i == 0 && first) {
                d[0] = 0.0;
                d[1] = 0.0;
                continue;
            }
            const uint32_t* t = h->hTab.get() + 2 * nt * i;
            int st = 0, sr = 0;
            double bt = 0.0, br = 0.0;
            vo_select(h->S, h->wd[0], h->rows[0], t, &st, &bt);
            if (h->same) {  // one rectangle: the rot table is the trans table
                sr = st;
                br = bt;
            } else {
                vo_select(h->S, h->wd[1], h->rows[1], t + nt, &sr, &br);
            }
            (void)br;
            const double v = bt * h->p.vtrans_scale;
            d[0] = v > h->p.vtrans_max ? h->p.vtrans_max : v;
            d[1] = (double)sr * h->p.rad_per_column;
        }
    }
    return RS_OK;
}

int rs_vo_set_timing(rs_vo* h, int enable) {
    rs::clear_error();
    RS_CHECK(h, RS_ERR_STATE, "null odometer handle");
    h->timing = enable != 0;
    return RS_OK;
}

int rs_vo_last_ms(rs_vo* h, double ms[2]) {
    RS_CHECK(h && ms, RS_ERR_ARG, "null argument");
    ms[0] = h->timed ? h->ms[0] : -1.0;
    ms[1] = h->timed ? h->ms[1] : -1.0;
    return RS_OK;
}

}  // extern "C"
