// Pose-cell ensemble on MI355X (gfx950): B small networks, each stepped by one workgroup out
// of its compute unit's LDS.
//
// pce_run_kernel: one workgroup of 1,024 threads per member.  It loads the member's float32
// volume from HBM into LDS, runs the launch's n steps with workgroup barriers only, writes
// each step's first maximum and stores the volume back.  No workgroup waits on another one, so
// a member's result depends on its own state and control alone.  A step (the reference's
// update(), oracle/posecell.py):
//   excite   the wrapped 7x7x7 excitation in its rank-2 separable form, in place: a walk over
//            the x-planes (X - 3, X - 2, X - 1, 0, 1, .. X - 1) filters each plane along theta
//            into `temp` and along y into a ring of 7 plane pairs (ge, gi); output plane i is
//            written over input plane i once walk entries i .. i + 6 exist, with the member's
//            global inhibition applied and the total accumulated in float64
//   path     the per-layer shifted 7x7 filter of the normalised state (the division is one
//            multiplication of the filtered value), path_layers layers at a time into the
//            scratch that temp and ring have become, copied back layer by layer
//   theta    the 7-tap theta filter, a thread per (x, y) column with a sliding window in
//            registers, in place; the clamp and the first maximum in C order ride along
// The next step's control record is fetched from HBM at the head of a step and stored into
// LDS at its end.  Offsets and sizes come from pce_plan.h's PceFit, computed on the host.
//
// The kernel is a template on two flags; rs_pce_run launches <false, false>,
// which is the code above and nothing else.
//   INJ   a run's injections (rs_pce_run_inject): at the head of a step, and behind the last
//         step of a run's last launch, the workgroup walks its member's records of that
//         boundary; thread 0 resolves the cell and adds to the state in LDS
//   POSE  the sub-cell pose: behind a step's theta pass the box round the step's first maximum
//         is gathered from the state into the scratch that temp and ring are then, and the
//         stage functions of pc_peak_rule.h give the step's six sums
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "pc_peak_rule.h"
#include "pce_plan.h"
#include "rs_common.h"

namespace {

using rs::PCE_KEPT;
using rs::PCE_RING;
using rs::PCE_TAPS;
using rs::PCE_THREADS;
constexpr int PCE_WAVES = PCE_THREADS / 64;
constexpr int PCE_RUN = 4;            // cells along y per path task
constexpr int PCE_ARGMAX_THREADS = 256;

struct PceArgs {
    int X, Y, TH, TP, PS, N, L, nf;
    unsigned state_off, temp_off, ring_off, filt_off, ctl_off, red_off, rec_bytes, rec_oy, rec_fi;
    float ge[PCE_TAPS], gi[PCE_TAPS], ks;
};

__device__ __forceinline__ unsigned long long pce_key(float v, unsigned lin) {
    return ((unsigned long long)__float_as_uint(v) << 32) | (unsigned)~lin;
}

// The order of finite floats of either sign, -0 as +0, in front of ~lin: the largest key is the
// first maximum in C order (pce_key's order holds for values >= +0 only, what a step leaves)
__device__ __forceinline__ unsigned long long pce_ord_key(float v, unsigned lin) {
    const unsigned u = v == 0.f ? 0u : __float_as_uint(v);   // -0 == +0: the first of them
    const unsigned ord = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
    return ((unsigned long long)ord << 32) | (unsigned)~lin;
}

__device__ __forceinline__ unsigned long long pce_wave_max(unsigned long long k) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const unsigned long long o = __shfl_down(k, d, 64);
        k = o > k ? o : k;
    }
    return k;
}

__device__ __forceinline__ void pce_store_cell(int32_t* out, unsigned long long key, int Y, int TH) {
    const unsigned lin = ~(unsigned)key;
    out[0] = (int)(lin / (unsigned)(Y * TH));
    out[1] = (int)(lin / (unsigned)TH % (unsigned)Y);
    out[2] = (int)(lin % (unsigned)TH);
}

// The largest key of the block's `waves` waves, in every thread (red: a word per wave).
__device__ __forceinline__ unsigned long long pce_block_max(unsigned long long best, unsigned long long* red, int waves) {
    best = pce_wave_max(best);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = best;
    __syncthreads();
    unsigned long long k = red[0];
    for (int w = 1; w < waves; ++w) k = red[w] > k ? red[w] : k;
    return k;
}

// The six sums of the wrapped box round cell `lin` (pc_peak_rule.h), by the whole block: every
// thread calls it, the stages run on at most 49 threads each, three barriers apart.  sc: a
// scratch of pce_pose_scratch_bytes(r), in use until the caller's next barrier; cell(x, y, th)
// reads the state; tabs: the weights of x, y and theta, sin then cos of each.  Six plain
// 8-byte stores.
template <class Cell>
__device__ __forceinline__ void pce_peak_sums(double* sc, int r, int X, int Y, int TH, unsigned lin,
                                              const double* __restrict__ tabs, double* __restrict__ out, Cell cell) {
    const int tid = threadIdx.x, w = 2 * r + 1, w2 = w * w;
    if (lin >= (unsigned)(X * Y * TH)) lin = 0u;   // (never an address outside the state)
    double* const v = sc;
    double* const bR = v + w * w2;
    double* const bC = bR + w2;
    double* const mg = bC + w2;
    double* const tw = mg + 3 * w;
    const int pth = (int)(lin % (unsigned)TH);
    const unsigned xy = lin / (unsigned)TH;
    const int py = (int)(xy % (unsigned)Y), px = (int)(xy / (unsigned)Y);
    if (tid < 6 * w) {   // row q of the weights: axis q / 2, sin then cos
        const int q = tid / w, ax = q >> 1;
        const int nn = ax == 0 ? X : ax == 1 ? Y : TH, p = ax == 0 ? px : ax == 1 ? py : pth;
        tw[tid] = tabs[(ax == 0 ? 0 : ax == 1 ? 2 * X : 2 * (X + Y)) + (q & 1) * nn + rs::pc_peak_wrap(p, tid % w, r, nn)];
    }
    for (int e = tid; e < w * w2; e += (int)blockDim.x) {
        const int k = e % w, ij = e / w, j = ij % w, i = ij / w;
        v[e] = (double)cell(rs::pc_peak_wrap(px, i, r, X), rs::pc_peak_wrap(py, j, r, Y), rs::pc_peak_wrap(pth, k, r, TH));
    }
    __syncthreads();
    if (tid < w2) {
        bR[tid] = rs::pc_peak_R(v, w, tid / w, tid % w);
        bC[tid] = rs::pc_peak_C(v, w, tid / w, tid % w);
    }
    __syncthreads();
    if (tid < 3 * w) mg[tid] = rs::pc_peak_marginal(bR, bC, w, tid / w, tid % w);
    __syncthreads();
    if (tid < 6) out[tid] = rs::pc_peak_dot_w(mg + (tid >> 1) * w, tw + tid * w, w);
}

// What the INJ and POSE instantiations take besides the plain arguments (all zero for the plain one).
struct PceFb {
    const unsigned* inj_off;        // [B + 1]: member m's records are inj_rec[inj_off[m] .. inj_off[m + 1])
    const rs::PceInjRec* inj_rec;   // (pce_plan.h: pce_inj_group)
    unsigned* inj_cell;             // each record's resolved cell, as a C-order linear index
    const double* tabs;             // the pose weights (rs_pce_set_peak_tables)
    double* sums;                   // [(m * ntotal + s) * 6]
    int r;                          // the pose radius
    int last;                       // the run's last launch: the records of step ntotal follow its last step
};

template <bool INJ, bool POSE>
__global__ __launch_bounds__(PCE_THREADS) void pce_run_kernel(
    const PceArgs a, float* __restrict__ state, const float* __restrict__ ginh, const float* __restrict__ filt,
    const unsigned char* __restrict__ ctl, int n, int ntotal, int s0, int32_t* __restrict__ out, const PceFb fb) {
    extern __shared__ __align__(16) unsigned char pce_lds[];
    const int tid = threadIdx.x, m = blockIdx.x;
    const int X = a.X, Y = a.Y, TH = a.TH, TP = a.TP, PS = a.PS, XY = X * Y;
    float* const S = reinterpret_cast<float*>(pce_lds + a.state_off);
    float* const T = reinterpret_cast<float*>(pce_lds + a.temp_off);
    float* const R = reinterpret_cast<float*>(pce_lds + a.ring_off);
    float* const Fl = reinterpret_cast<float*>(pce_lds + a.filt_off);
    double* const redD = reinterpret_cast<double*>(pce_lds + a.red_off);
    unsigned long long* const redK = reinterpret_cast<unsigned long long*>(pce_lds + a.red_off + 128);
    const int rw = (int)(a.rec_bytes / 4);
    float* const gs = state + (size_t)m * a.N;
    const unsigned* const grec = reinterpret_cast<const unsigned*>(ctl + (size_t)m * n * a.rec_bytes);

    for (int c = tid; c < a.N; c += PCE_THREADS) {
        const int col = c / TH;
        S[col * TP + (c - col * TH)] = gs[c];
    }
    for (int i = tid; i < a.nf * PCE_TAPS * PCE_TAPS; i += PCE_THREADS) Fl[i] = filt[i];
    if ((!INJ || n > 0) && tid < rw) reinterpret_cast<unsigned*>(pce_lds + a.ctl_off)[tid] = grec[tid];
    const float g = ginh[m];
    __syncthreads();

    // ---- the member's injections of one boundary (INJ): uniform in the block ----
    unsigned cur = 0, end = 0;        // the records not yet applied
    bool fresh = false;               // `peak` is the state's first maximum: this launch's last step wrote it,
    unsigned long long peak = 0ull;   // and nothing was injected since (thread 0 holds the key)
    if constexpr (INJ) {
        cur = fb.inj_off[m], end = fb.inj_off[m + 1];
        while (cur < end && fb.inj_rec[cur].step < s0) ++cur;   // (applied by the launches before)
    }
    auto inject_at = [&](int step) {
        while (cur < end && fb.inj_rec[cur].step == step) {
            const rs::PceInjRec rc = fb.inj_rec[cur];
            unsigned long long k = peak;
            if (rc.kind == rs::PCE_INJ_PEAK && !fresh) {
                // the state may hold a negative cell or -0 (a launch's head, an injection of
                // this boundary): pce_argmax_kernel's order over the state in LDS
                __syncthreads();   // (thread 0 has read the last step's redK)
                unsigned long long best = 0ull;
                for (int c = tid; c < a.N; c += PCE_THREADS) {
                    const int col = c / TH;
                    const unsigned long long key = pce_ord_key(S[col * TP + (c - col * TH)], (unsigned)c);
                    best = key > best ? key : best;
                }
                k = pce_block_max(best, redK, PCE_WAVES);
            }
            if (tid == 0) {
                unsigned lin = rc.kind == rs::PCE_INJ_EXPLICIT ? rc.arg
                               : rc.kind == rs::PCE_INJ_SAME   ? fb.inj_cell[rc.arg]
                                                               : ~(unsigned)k;
                if (lin >= (unsigned)a.N) lin = 0u;   // (never an address outside the state)
                const unsigned col = lin / (unsigned)TH;
                S[col * TP + (lin - col * TH)] += rc.energy;
                fb.inj_cell[cur] = lin;
            }
            fresh = false;
            ++cur;
            __syncthreads();   // the next record's maximum, or the excitation, reads the state
        }
    };

    for (int s = 0; s < n; ++s) {
        if constexpr (INJ) inject_at(s0 + s);
        const unsigned char* const rec = pce_lds + a.ctl_off + (size_t)(s & 1) * a.rec_bytes;
        const bool fetch = tid < rw && s + 1 < n;
        unsigned next_word = 0;
        if (fetch) next_word = grec[(size_t)(s + 1) * rw + tid];

        // ---- excitation, inhibition, total ----
        double acc = 0.0;
        auto x_pass = [&](int i, int c) {   // output plane i, cell c of the plane
            float e = 0.f, q = 0.f;
#pragma unroll
            for (int t = 0; t < PCE_TAPS; ++t) {
                const int v = i + t;   // walk index
                const int slot = v > X + 2 ? PCE_RING + (v - X - 3) : v % PCE_RING;
                e += a.ge[t] * R[slot * 2 * PS + c];
                q += a.gi[t] * R[slot * 2 * PS + PS + c];
            }
            float val = a.ks * (e - q);
            val = val < g ? 0.f : val - g;
            const int y = c / TH;
            S[(i * Y + y) * TP + (c - y * TH)] = val;
            acc += (double)val;
        };
        for (int w = 0; w < X + 3; ++w) {
            const int p = w < 3 ? X - 3 + w : w - 3;
            for (int task = tid; task < 2 * PS; task += PCE_THREADS) {
                if (task < PS) {
                    const int y = task / TH, th = task - y * TH;
                    const float* row = S + (p * Y + y) * TP;
                    int k = th - 3;
                    k = k < 0 ? k + TH : k;
                    float e = 0.f, q = 0.f;
#pragma unroll
                    for (int t = 0; t < PCE_TAPS; ++t) {
                        const float v = row[k];
                        e += a.ge[t] * v;
                        q += a.gi[t] * v;
                        k = k + 1 == TH ? 0 : k + 1;
                    }
                    T[task] = e;
                    T[PS + task] = q;
                } else if (w >= PCE_RING) {
                    x_pass(w - PCE_RING, task - PS);
                }
            }
            __syncthreads();
            for (int c = tid; c < PS; c += PCE_THREADS) {
                const int y = c / TH, th = c - y * TH;
                int yy = y - 3;
                yy = yy < 0 ? yy + Y : yy;
                float e = 0.f, q = 0.f;
#pragma unroll
                for (int t = 0; t < PCE_TAPS; ++t) {
                    e += a.ge[t] * T[yy * TH + th];
                    q += a.gi[t] * T[PS + yy * TH + th];
                    yy = yy + 1 == Y ? 0 : yy + 1;
                }
                const int slot = w % PCE_RING;
                R[slot * 2 * PS + c] = e;
                R[slot * 2 * PS + PS + c] = q;
                if (w >= 3 && w < 3 + PCE_KEPT) {   // planes 0, 1, 2: also kept for the far end
                    R[(PCE_RING + w - 3) * 2 * PS + c] = e;
                    R[(PCE_RING + w - 3) * 2 * PS + PS + c] = q;
                }
            }
            __syncthreads();
        }
        for (int task = tid; task < 4 * PS; task += PCE_THREADS) {
            const int r = task / PS;
            x_pass(X - 4 + r, task - r * PS);
        }
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) acc += __shfl_down(acc, d, 64);
        if ((tid & 63) == 0) redD[tid >> 6] = acc;
        __syncthreads();
        double total = 0.0;
#pragma unroll
        for (int w = 0; w < PCE_WAVES; ++w) total += redD[w];
        const float scale = total != 0.0 ? (float)(1.0 / total) : 1.f;

        // ---- path filter, a group of layers at a time ----
        const unsigned short* const cox = reinterpret_cast<const unsigned short*>(rec + 32);
        const unsigned short* const coy = reinterpret_cast<const unsigned short*>(rec + a.rec_oy);
        const unsigned char* const cfi = rec + a.rec_fi;
        const int JR = (Y + PCE_RUN - 1) / PCE_RUN, tasks = X * JR;
        for (int g0 = 0; g0 < TH; g0 += a.L) {
            const int Lg = min(a.L, TH - g0);
            const int slot = tid / Lg, lk = tid - slot * Lg, nslots = PCE_THREADS / Lg;
            if (slot < nslots) {
                const int k = g0 + lk;
                const int ox = cox[k], oy = coy[k];
                const float* fk = Fl + (int)cfi[k] * (PCE_TAPS * PCE_TAPS);
                for (int task = slot; task < tasks; task += nslots) {
                    const int i = task / JR, j0 = (task - i * JR) * PCE_RUN;
                    int xi = i - 3 + ox;
                    xi = xi < 0 ? xi + X : (xi >= X ? xi - X : xi);
                    int yj0 = j0 - 3 + oy;
                    yj0 = yj0 < 0 ? yj0 + Y : (yj0 >= Y ? yj0 - Y : yj0);
                    float o[PCE_RUN] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 1
                    for (int dx = 0; dx < PCE_TAPS; ++dx) {
                        float v[PCE_RUN + PCE_TAPS - 1], tp[PCE_TAPS];   // (a filter row at a time: 49 taps do not fit the registers)
#pragma unroll
                        for (int dy = 0; dy < PCE_TAPS; ++dy) tp[dy] = fk[dx * PCE_TAPS + dy];
                        int yj = yj0;
#pragma unroll
                        for (int qy = 0; qy < PCE_RUN + PCE_TAPS - 1; ++qy) {
                            v[qy] = S[(xi * Y + yj) * TP + k];
                            yj = yj + 1 == Y ? 0 : yj + 1;
                        }
#pragma unroll
                        for (int dy = 0; dy < PCE_TAPS; ++dy)
#pragma unroll
                            for (int r = 0; r < PCE_RUN; ++r) o[r] += tp[dy] * v[r + dy];
                        xi = xi + 1 == X ? 0 : xi + 1;
                    }
#pragma unroll
                    for (int r = 0; r < PCE_RUN; ++r)
                        if (j0 + r < Y) {
                            const float val = scale * o[r];
                            T[lk * XY + i * Y + j0 + r] = val > 0.f ? val : 0.f;
                        }
                }
            }
            __syncthreads();
            for (int idx = tid; idx < Lg * XY; idx += PCE_THREADS) {
                const int l2 = idx / XY, col = idx - l2 * XY;
                S[col * TP + g0 + l2] = T[idx];
            }
            __syncthreads();
        }

        // ---- theta filter in place, clamp, first maximum ----
        float zf[PCE_TAPS];
#pragma unroll
        for (int t = 0; t < PCE_TAPS; ++t) zf[t] = reinterpret_cast<const float*>(rec)[t];
        unsigned long long best = 0ull;
        for (int col = tid; col < XY; col += PCE_THREADS) {
            float* const pc = S + col * TP;
            const float f0 = pc[0], f1 = pc[1], f2 = pc[2];
            float w0 = pc[TH - 3], w1 = pc[TH - 2], w2 = pc[TH - 1], w3 = f0, w4 = f1, w5 = f2, w6 = pc[3];
            for (int k = 0; k < TH; ++k) {
                float o = zf[0] * w0;
                o += zf[1] * w1;
                o += zf[2] * w2;
                o += zf[3] * w3;
                o += zf[4] * w4;
                o += zf[5] * w5;
                o += zf[6] * w6;
                o = o > 0.f ? o : 0.f;
                const int kn = k + 4;   // the original that enters the window next
                const float nv = kn < TH ? pc[kn] : (kn == TH ? f0 : (kn == TH + 1 ? f1 : f2));
                pc[k] = o;
                const unsigned long long key = pce_key(o, (unsigned)(col * TH + k));
                best = key > best ? key : best;
                w0 = w1, w1 = w2, w2 = w3, w3 = w4, w4 = w5, w5 = w6, w6 = nv;
            }
        }
        best = pce_wave_max(best);
        if ((tid & 63) == 0) redK[tid >> 6] = best;
        if (fetch) reinterpret_cast<unsigned*>(pce_lds + a.ctl_off + (size_t)((s + 1) & 1) * a.rec_bytes)[tid] = next_word;
        __syncthreads();
        unsigned long long k = 0ull;
        if (POSE || tid == 0) {   // (the pose: every thread decodes the cell)
            k = redK[0];
#pragma unroll
            for (int w = 1; w < PCE_WAVES; ++w) k = redK[w] > k ? redK[w] : k;
        }
        if (tid == 0) pce_store_cell(out + ((size_t)m * ntotal + s0 + s) * 3, k, Y, TH);
        if constexpr (INJ) peak = k, fresh = true;
        if constexpr (POSE) {
            // temp and ring are dead until the next excitation: the pose's scratch
            pce_peak_sums(reinterpret_cast<double*>(T), fb.r, X, Y, TH, ~(unsigned)k, fb.tabs,
                          fb.sums + ((size_t)m * ntotal + s0 + s) * 6,
                          [&](int cx, int cy, int ck) { return S[(cx * Y + cy) * TP + ck]; });
            __syncthreads();   // before the next excitation writes temp
        }
    }
    if constexpr (INJ) {
        if (fb.last) inject_at(ntotal);
    }
    __syncthreads();
    for (int c = tid; c < a.N; c += PCE_THREADS) {
        const int col = c / TH;
        gs[c] = S[col * TP + (c - col * TH)];
    }
}

// out[m] = the first maximum in C order of member m's stored volume
__global__ __launch_bounds__(PCE_ARGMAX_THREADS) void pce_argmax_kernel(const float* __restrict__ state, int N, int Y,
                                                                       int TH, int32_t* __restrict__ out) {
    __shared__ unsigned long long red[PCE_ARGMAX_THREADS / 64];
    const float* gs = state + (size_t)blockIdx.x * N;
    unsigned long long best = 0ull;
    for (int c = threadIdx.x; c < N; c += PCE_ARGMAX_THREADS) {
        // (a stored volume is finite; negative values, which a write or an injection can bring, order below +0)
        const unsigned long long key = pce_ord_key(gs[c], (unsigned)c);
        best = key > best ? key : best;
    }
    best = pce_wave_max(best);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = best;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long k = red[0];
        for (int w = 1; w < PCE_ARGMAX_THREADS / 64; ++w) k = red[w] > k ? red[w] : k;
        pce_store_cell(out + 3 * (size_t)blockIdx.x, k, Y, TH);
    }
}

// The stored state's first maximum and the six sums of the box round it: a block per member,
// pce_argmax_kernel's maximum, then the box from HBM (rs_pce_get_peak).
__global__ __launch_bounds__(PCE_ARGMAX_THREADS) void pce_peak_kernel(const float* __restrict__ state, int N, int X, int Y,
                                                                     int TH, int r, const double* __restrict__ tabs,
                                                                     int32_t* __restrict__ out, double* __restrict__ sums) {
    constexpr int W = rs::PC_PEAK_WMAX;
    __shared__ unsigned long long red[PCE_ARGMAX_THREADS / 64];
    __shared__ double sc[W * W * W + 2 * W * W + 9 * W];   // pce_pose_scratch_bytes(3)
    const float* gs = state + (size_t)blockIdx.x * N;
    unsigned long long best = 0ull;
    for (int c = threadIdx.x; c < N; c += PCE_ARGMAX_THREADS) {
        const unsigned long long key = pce_ord_key(gs[c], (unsigned)c);
        best = key > best ? key : best;
    }
    const unsigned long long k = pce_block_max(best, red, PCE_ARGMAX_THREADS / 64);
    if (threadIdx.x == 0) pce_store_cell(out + 3 * (size_t)blockIdx.x, k, Y, TH);
    pce_peak_sums(sc, r, X, Y, TH, ~(unsigned)k, tabs, sums + 6 * (size_t)blockIdx.x,
                  [&](int cx, int cy, int ck) { return gs[((size_t)cx * Y + cy) * TH + ck]; });
}

// state[m][lin] += e for member `member`, or for every member (member < 0)
__global__ void pce_inject_kernel(float* state, int B, int N, int member, int lin, float e) {
    const int m = blockIdx.x * blockDim.x + threadIdx.x;
    if (m < B && (member < 0 || m == member)) state[(size_t)m * N + lin] += e;
}

// The instantiation a run launches: the plain one unless it has injections or wants sums.
using PceRunKernel = void (*)(const PceArgs, float*, const float*, const float*, const unsigned char*, int, int, int,
                              int32_t*, const PceFb);
PceRunKernel pce_run_form(bool inj, bool pose) {
    return inj ? (pose ? pce_run_kernel<true, true> : pce_run_kernel<true, false>)
               : (pose ? pce_run_kernel<false, true> : pce_run_kernel<false, false>);
}

}  // namespace

// The buffers are rs::DevBuf / rs::PinnedBuf members, the stream and the events rs::Stream /
// rs::Event owners (rs_common.h).
struct rs_pce {
    int device = 0;
    int B = 0, X = 0, Y = 0, TH = 0;
    size_t N = 0;
    rs::PceFit fit;
    PceArgs args{};
    int nfilters = 0;
    int forced_chunk = 0;                  // RS_PCE_CHUNK, read at create
    rs::DevBuf<float> dState, dInhib, dFilt;
    rs::DevBuf<unsigned char> dCtl[2];     // a launch's records, two slots in turn
    rs::DevBuf<int32_t> dOut;
    rs::PinnedBuf<unsigned char> hCtl;     // a run's records, launch after launch
    rs::PinnedBuf<int32_t> hOut;
    rs::PinnedBuf<float> hState;           // staging of rs_pce_read / rs_pce_write
    // a run's injections: the offsets and the records (pce_inj_group) in one block, the resolved cells
    rs::DevBuf<unsigned char> dInj;
    rs::PinnedBuf<unsigned char> hInj;
    rs::DevBuf<unsigned> dInjCell;
    rs::PinnedBuf<unsigned> hInjCell;
    // the pose: the radius (0 before rs_pce_set_peak_tables), the weights, six sums per member and step
    int peak_r = 0;
    rs::DevBuf<double> dTabs, dSums;
    rs::PinnedBuf<double> hSums;
    bool timing = false, timed = false;
    // the owners come after the buffers: members go in reverse order, streams and events first
    rs::Stream stream;
    rs::Event ev[2];
};

extern "C" {

int rs_pce_fit(int X, int Y, int TH, size_t* lds_bytes) {
    rs::clear_error();
    const rs::PceFit f = rs::pce_fit(X, Y, TH);
    if (lds_bytes) *lds_bytes = f.total;
    RS_CHECK(X >= rs::PCE_MIN_DIM && Y >= rs::PCE_MIN_DIM && TH >= rs::PCE_MIN_DIM, RS_ERR_ARG,
             "grid (%d, %d, %d): every dimension of an ensemble member must be >= %d", X, Y, TH, rs::PCE_MIN_DIM);
    RS_CHECK(f.fits, RS_ERR_ARG,
             "grid (%d, %d, %d) needs %zu bytes of LDS per member, a compute unit has %zu", X, Y, TH, f.total,
             rs::PCE_LDS_BYTES);
    return RS_OK;
}

int rs_pce_create(int B, int X, int Y, int TH, const rs_pc_params* p, const double* global_inhibition, int device,
                  rs_pce** out) {
    rs::clear_error();
    RS_CHECK(out, RS_ERR_ARG, "null output handle pointer");
    *out = nullptr;
    RS_CHECK(p, RS_ERR_ARG, "null params");
    RS_CHECK(B >= 1, RS_ERR_ARG, "an ensemble of %d members", B);
    RS_CHECK(p->precision == RS_PREC_F32, RS_ERR_ARG, "the ensemble is float32 only (precision RS_PREC_F32)");
    RS_TRY(rs_pce_fit(X, Y, TH, nullptr));
    RS_CHECK(p->nfilters >= 1 && p->nfilters <= rs::PCE_MAX_FILTERS && p->xy_filters, RS_ERR_ARG,
             "path-integration filter table of %d filters: the ensemble stages 1 .. %d", p->nfilters,
             rs::PCE_MAX_FILTERS);
    const rs::PceFit fit = rs::pce_fit(X, Y, TH);
    const size_t N = (size_t)X * Y * TH;
    RS_CHECK((size_t)B * N < (1ull << 40) && (size_t)B < (1u << 24), RS_ERR_ARG, "an ensemble of %d members is too large", B);
    int forced = 0;
    if (const char* e = std::getenv("RS_PCE_CHUNK")) {
        if (*e) {
            char* end = nullptr;
            const long v = std::strtol(e, &end, 10);
            RS_CHECK(end && !*end && v >= 1 && v <= (1 << 20), RS_ERR_ARG, "RS_PCE_CHUNK=%s: expected 1 .. %d", e, 1 << 20);
            forced = (int)v;
        }
    }
    RS_TRY(rs::use_device(device));
    // one failure exit: rs_pce_destroy takes a handle at any stage
    std::unique_ptr<rs_pce, int (*)(rs_pce*)> owner(new rs_pce(), rs_pce_destroy);
    rs_pce* const h = owner.get();
    h->device = device;
    h->B = B, h->X = X, h->Y = Y, h->TH = TH, h->N = N;
    h->fit = fit;
    h->nfilters = p->nfilters;
    h->forced_chunk = forced;
    PceArgs& a = h->args;
    a.X = X, a.Y = Y, a.TH = TH, a.TP = fit.TP, a.PS = fit.PS, a.N = (int)N, a.L = fit.path_layers, a.nf = p->nfilters;
    a.state_off = (unsigned)fit.state_off, a.temp_off = (unsigned)fit.temp_off, a.ring_off = (unsigned)fit.ring_off;
    a.filt_off = (unsigned)fit.filt_off, a.ctl_off = (unsigned)fit.ctl_off, a.red_off = (unsigned)fit.red_off;
    a.rec_bytes = (unsigned)rs::pce_rec_bytes(TH);
    a.rec_oy = (unsigned)rs::pce_rec_oy(TH), a.rec_fi = (unsigned)rs::pce_rec_fi(TH);
    for (int t = 0; t < PCE_TAPS; ++t) a.ge[t] = (float)p->ge[t], a.gi[t] = (float)p->gi[t];
    a.ks = (float)p->k_scale;

    RS_TRY(h->stream.create());
    for (rs::Event& e : h->ev) RS_TRY(e.create());
    for (int v = 0; v < 4; ++v)
        RS_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(pce_run_form(v & 1, v & 2)),
                                   hipFuncAttributeMaxDynamicSharedMemorySize, (int)fit.total));
    const size_t nft = (size_t)p->nfilters * PCE_TAPS * PCE_TAPS;
    RS_TRY(h->dState.reserve((size_t)B * N, "ensemble volumes"));
    RS_TRY(h->dInhib.reserve(B, "ensemble inhibitions"));
    RS_TRY(h->dFilt.reserve(nft, "path filters"));
    RS_TRY(h->dOut.reserve(3 * (size_t)B, "ensemble peaks"));
    RS_TRY(h->hOut.reserve(3 * (size_t)B, hipHostMallocDefault, "ensemble peaks"));
    RS_TRY(h->hState.reserve(std::max((size_t)B, nft), hipHostMallocDefault, "ensemble staging"));
    float* st = h->hState.get();
    for (size_t i = 0; i < nft; ++i) st[i] = (float)p->xy_filters[i];
    RS_HIP(hipMemcpyAsync(h->dFilt.get(), st, sizeof(float) * nft, hipMemcpyHostToDevice, h->stream.get()));
    RS_HIP(hipStreamSynchronize(h->stream.get()));   // the staging is free again
    for (int m = 0; m < B; ++m) st[m] = (float)(global_inhibition ? global_inhibition[m] : p->global_inhibition);
    RS_HIP(hipMemcpyAsync(h->dInhib.get(), st, sizeof(float) * B, hipMemcpyHostToDevice, h->stream.get()));
    RS_HIP(hipMemsetAsync(h->dState.get(), 0, sizeof(float) * (size_t)B * N, h->stream.get()));
    RS_HIP(hipStreamSynchronize(h->stream.get()));
    *out = owner.release();
    return RS_OK;
}

int rs_pce_destroy(rs_pce* h) {
    if (!h) return RS_OK;
    (void)hipSetDevice(h->device);
    // queued work that failed after a call returned is reported here, not dropped
    const hipError_t se = rs::sync_streams({h->stream.get()});
    delete h;  // (the streams and events, then the buffers, go with their members)
    RS_CHECK(se == hipSuccess, RS_ERR_HIP, "work queued before rs_pce_destroy failed: %s", hipGetErrorString(se));
    return RS_OK;
}

int rs_pce_shape(const rs_pce* h, int* B, int* X, int* Y, int* TH) {
    rs::clear_error();
    RS_CHECK(h, RS_ERR_STATE, "null ensemble handle");
    if (B) *B = h->B;
    if (X) *X = h->X;
    if (Y) *Y = h->Y;
    if (TH) *TH = h->TH;
    return RS_OK;
}

int rs_pce_run(rs_pce* h, int n, const int32_t* ox, const int32_t* oy, const int32_t* fidx, const double* zf,
               int32_t* out_xyz) {
    return rs_pce_run_inject(h, n, ox, oy, fidx, zf, 0, nullptr, nullptr, nullptr, nullptr, out_xyz, nullptr, nullptr);
}

// rs_pce_run is this call without injections and sums: one path for both, which launches the
// plain instantiation then.
int rs_pce_run_inject(rs_pce* h, int n, const int32_t* ox, const int32_t* oy, const int32_t* fidx, const double* zf,
                      int ni, const int32_t* inj_member, const int32_t* inj_step, const double* inj_energy,
                      const int32_t* inj_loc, int32_t* out_xyz, int32_t* out_inj_xyz, double* out_sums) {
    rs::clear_error();
    RS_CHECK(h, RS_ERR_STATE, "null ensemble handle");
    RS_CHECK(n >= 0, RS_ERR_ARG, "negative step count");
    RS_CHECK(ni >= 0, RS_ERR_ARG, "negative injection count");
    h->timed = false;
    if (n == 0 && ni == 0) return RS_OK;
    RS_CHECK(n == 0 || (ox && oy && fidx && zf && out_xyz), RS_ERR_ARG, "null argument");
    RS_CHECK(ni == 0 || (inj_member && inj_step && inj_energy && inj_loc && out_inj_xyz), RS_ERR_ARG, "null argument");
    const int B = h->B, TH = h->TH;
    const size_t steps = (size_t)B * n;
    RS_CHECK(steps < (1ull << 31) / 4, RS_ERR_ARG, "%d members x %d steps: too many for one run", B, n);
    for (size_t i = 0; i < steps * TH; ++i)
        if (fidx[i] < 0 || fidx[i] >= h->nfilters) {
            rs::set_error("member %zu, step %zu: filter index %d outside the table of %d", i / TH / n, i / TH % n,
                          fidx[i], h->nfilters);
            return RS_ERR_ARG;
        }
    rs::PceInjBad why = rs::PCE_INJ_OK;
    const int bad = rs::pce_inj_first_bad(B, h->X, h->Y, TH, n, ni, inj_member, inj_step, inj_energy, inj_loc, &why);
    if (bad >= 0) {
        const int32_t* l = inj_loc + 3 * (size_t)bad;
        switch (why) {
        case rs::PCE_INJ_BAD_MEMBER: rs::set_error("injection %d: member %d outside [0, %d)", bad, inj_member[bad], B); break;
        case rs::PCE_INJ_BAD_STEP: rs::set_error("injection %d: step %d outside [0, %d]", bad, inj_step[bad], n); break;
        case rs::PCE_INJ_BAD_ORDER:
            rs::set_error("injection %d: step %d below an earlier injection's of member %d", bad, inj_step[bad], inj_member[bad]);
            break;
        case rs::PCE_INJ_BAD_SAME:
            rs::set_error("injection %d: same-as %d is no earlier injection of member %d", bad, l[1], inj_member[bad]);
            break;
        case rs::PCE_INJ_BAD_ENERGY: rs::set_error("injection %d: energy %g is not a finite float32", bad, inj_energy[bad]); break;
        default:
            rs::set_error("injection %d: cell (%d, %d, %d) outside grid (%d, %d, %d)", bad, l[0], l[1], l[2], h->X, h->Y, TH);
        }
        return RS_ERR_ARG;
    }
    const bool pose = out_sums && n > 0;
    RS_CHECK(!pose || h->peak_r > 0, RS_ERR_STATE, "sums asked for before rs_pce_set_peak_tables");
    RS_HIP(hipSetDevice(h->device));
    const size_t rb = rs::pce_rec_bytes(TH);
    const int K = std::max(1, std::min(n, rs::pce_chunk_len(B, TH, h->forced_chunk)));
    const int nchunks = rs::pce_chunk_count(n, K);
    const size_t inj_recs = rs::pce_align(sizeof(uint32_t) * ((size_t)B + 1));   // the records' place behind the offsets
    const size_t inj_bytes = ni ? inj_recs + sizeof(rs::PceInjRec) * (size_t)ni : 0;
    // (queued launches of an earlier call may still read the blocks a growth would free)
    if (steps * rb > h->hCtl.capacity() || (size_t)B * K * rb > h->dCtl[0].capacity() || 3 * steps > h->dOut.capacity() ||
        inj_bytes > h->dInj.capacity() || (size_t)ni > h->dInjCell.capacity() || (pose && 6 * steps > h->dSums.capacity()))
        RS_HIP(hipStreamSynchronize(h->stream.get()));
    RS_TRY(h->hCtl.reserve(steps * rb, hipHostMallocDefault, "ensemble control"));
    if (n > 0)
        for (auto& d : h->dCtl) RS_TRY(d.reserve((size_t)B * K * rb, "ensemble control"));
    RS_TRY(h->dOut.reserve(3 * steps, "ensemble peaks"));
    RS_TRY(h->hOut.reserve(3 * steps, hipHostMallocDefault, "ensemble peaks"));
    std::vector<int32_t> grouped((size_t)ni);
    PceFb fb{};
    if (ni > 0) {
        RS_TRY(h->dInj.reserve(inj_bytes, "ensemble injections"));
        RS_TRY(h->hInj.reserve(inj_bytes, hipHostMallocDefault, "ensemble injections"));
        RS_TRY(h->dInjCell.reserve(ni, "ensemble injection cells"));
        RS_TRY(h->hInjCell.reserve(ni, hipHostMallocDefault, "ensemble injection cells"));
        rs::pce_inj_group(B, h->Y, TH, ni, inj_member, inj_step, inj_energy, inj_loc,
                          reinterpret_cast<uint32_t*>(h->hInj.get()),
                          reinterpret_cast<rs::PceInjRec*>(h->hInj.get() + inj_recs), grouped.data());
        fb.inj_off = reinterpret_cast<const unsigned*>(h->dInj.get());
        fb.inj_rec = reinterpret_cast<const rs::PceInjRec*>(h->dInj.get() + inj_recs);
        fb.inj_cell = h->dInjCell.get();
    }
    if (pose) {
        RS_TRY(h->dSums.reserve(6 * steps, "ensemble sums"));
        RS_TRY(h->hSums.reserve(6 * steps, hipHostMallocDefault, "ensemble sums"));
        fb.tabs = h->dTabs.get();
        fb.sums = h->dSums.get();
        fb.r = h->peak_r;
    }
    const PceRunKernel kernel = pce_run_form(ni > 0, pose);
    // the records launch after launch, member-major inside a launch
    unsigned char* rec = h->hCtl.get();
    for (int c = 0; c < nchunks; ++c) {
        int first, count;
        rs::pce_chunk(n, K, c, &first, &count);
        for (int m = 0; m < B; ++m)
            for (int s = first; s < first + count; ++s, rec += rb) {
                const size_t i = (size_t)m * n + s;
                rs::pce_pack(h->X, h->Y, TH, ox + i * TH, oy + i * TH, fidx + i * TH, zf + i * PCE_TAPS, rec);
            }
    }
    if (ni > 0)
        RS_HIP(hipMemcpyAsync(h->dInj.get(), h->hInj.get(), inj_bytes, hipMemcpyHostToDevice, h->stream.get()));
    const bool timed = h->timing;
    if (timed) RS_HIP(hipEventRecord(h->ev[0].get(), h->stream.get()));
    size_t off = 0;
    for (int c = 0; c < nchunks; ++c) {
        int first, count;
        rs::pce_chunk(n, K, c, &first, &count);
        const size_t bytes = (size_t)B * count * rb;
        unsigned char* d = h->dCtl[c & 1].get();
        RS_HIP(hipMemcpyAsync(d, h->hCtl.get() + off, bytes, hipMemcpyHostToDevice, h->stream.get()));
        off += bytes;
        fb.last = c == nchunks - 1;
        hipLaunchKernelGGL(kernel, dim3(B), dim3(PCE_THREADS), h->fit.total, h->stream.get(), h->args, h->dState.get(),
                           h->dInhib.get(), h->dFilt.get(), d, count, n, first, h->dOut.get(), fb);
        RS_HIP(hipGetLastError());
    }
    if (n == 0) {   // the injections alone: a launch of no steps
        fb.last = 1;
        hipLaunchKernelGGL(kernel, dim3(B), dim3(PCE_THREADS), h->fit.total, h->stream.get(), h->args, h->dState.get(),
                           h->dInhib.get(), h->dFilt.get(), nullptr, 0, 0, 0, h->dOut.get(), fb);
        RS_HIP(hipGetLastError());
    }
    if (timed) {
        RS_HIP(hipEventRecord(h->ev[1].get(), h->stream.get()));
        h->timed = true;
    }
    if (n > 0)
        RS_HIP(hipMemcpyAsync(h->hOut.get(), h->dOut.get(), sizeof(int32_t) * 3 * steps, hipMemcpyDeviceToHost, h->stream.get()));
    if (ni > 0)
        RS_HIP(hipMemcpyAsync(h->hInjCell.get(), h->dInjCell.get(), sizeof(unsigned) * ni, hipMemcpyDeviceToHost, h->stream.get()));
    if (pose)
        RS_HIP(hipMemcpyAsync(h->hSums.get(), h->dSums.get(), sizeof(double) * 6 * steps, hipMemcpyDeviceToHost, h->stream.get()));
    RS_HIP(hipStreamSynchronize(h->stream.get()));
    if (n > 0) std::memcpy(out_xyz, h->hOut.get(), sizeof(int32_t) * 3 * steps);
    if (pose) std::memcpy(out_sums, h->hSums.get(), sizeof(double) * 6 * steps);
    for (int i = 0; i < ni; ++i) {
        const unsigned lin = h->hInjCell.get()[grouped[i]];
        out_inj_xyz[3 * (size_t)i] = (int32_t)(lin / (unsigned)(h->Y * TH));
        out_inj_xyz[3 * (size_t)i + 1] = (int32_t)(lin / (unsigned)TH % (unsigned)h->Y);
        out_inj_xyz[3 * (size_t)i + 2] = (int32_t)(lin % (unsigned)TH);
    }
    return RS_OK;
}

int rs_pce_set_peak_tables(rs_pce* h, int r, const double* sc_x, const double* sc_y, const double* sc_th) {
    rs::clear_error();
    RS_CHECK(h, RS_ERR_STATE, "null ensemble handle");
    RS_CHECK(sc_x && sc_y && sc_th, RS_ERR_ARG, "null argument");
    RS_CHECK(rs::pc_peak_fits(h->X, h->Y, h->TH, r), RS_ERR_ARG,
             "cells_to_avg %d: expected 1 .. %d and a box of 2r+1 cells that grid (%d, %d, %d) holds", r,
             rs::PC_PEAK_RMAX, h->X, h->Y, h->TH);
    RS_CHECK(rs::pce_pose_fits(h->fit, r), RS_ERR_ARG, "the pose scratch of radius %d does not fit the plan", r);
    RS_HIP(hipSetDevice(h->device));
    const size_t nx = 2 * (size_t)h->X, ny = 2 * (size_t)h->Y, nth = 2 * (size_t)h->TH;
    RS_HIP(hipStreamSynchronize(h->stream.get()));   // the staging is free, no queued launch reads the tables
    RS_TRY(h->dTabs.reserve(nx + ny + nth, "pose weights"));
    RS_TRY(h->hSums.reserve(std::max(nx + ny + nth, 6 * (size_t)h->B), hipHostMallocDefault, "ensemble sums"));
    RS_TRY(h->dSums.reserve(6 * (size_t)h->B, "ensemble sums"));
    double* st = h->hSums.get();
    std::memcpy(st, sc_x, sizeof(double) * nx);
    std::memcpy(st + nx, sc_y, sizeof(double) * ny);
    std::memcpy(st + nx + ny, sc_th, sizeof(double) * nth);
    RS_HIP(hipMemcpyAsync(h->dTabs.get(), st, sizeof(double) * (nx + ny + nth), hipMemcpyHostToDevice, h->stream.get()));
    RS_HIP(hipStreamSynchronize(h->stream.get()));
    h->peak_r = r;
    return RS_OK;
}

int rs_pce_get_peak(rs_pce* h, int32_t* out_xyz, double* out_sums) {
    rs::clear_error();
    RS_CHECK(h, RS_ERR_STATE, "null ensemble handle");
    RS_CHECK(out_xyz && out_sums, RS_ERR_ARG, "null argument");
    RS_CHECK(h->peak_r > 0, RS_ERR_STATE, "rs_pce_get_peak before rs_pce_set_peak_tables");
    RS_HIP(hipSetDevice(h->device));
    hipLaunchKernelGGL(pce_peak_kernel, dim3(h->B), dim3(PCE_ARGMAX_THREADS), 0, h->stream.get(), h->dState.get(),
                       (int)h->N, h->X, h->Y, h->TH, h->peak_r, h->dTabs.get(), h->dOut.get(), h->dSums.get());
    RS_HIP(hipGetLastError());
    RS_HIP(hipMemcpyAsync(h->hOut.get(), h->dOut.get(), sizeof(int32_t) * 3 * h->B, hipMemcpyDeviceToHost, h->stream.get()));
    RS_HIP(hipMemcpyAsync(h->hSums.get(), h->dSums.get(), sizeof(double) * 6 * h->B, hipMemcpyDeviceToHost, h->stream.get()));
    RS_HIP(hipStreamSynchronize(h->stream.get()));
    std::memcpy(out_xyz, h->hOut.get(), sizeof(int32_t) * 3 * h->B);
    std::memcpy(out_sums, h->hSums.get(), sizeof(double) * 6 * h->B);
    return RS_OK;
}

int rs_pce_inject(rs_pce* h, int member, double energy, int x, int y, int th) {
    rs::clear_error();
    RS_CHECK(h, RS_ERR_STATE, "null ensemble handle");
    RS_CHECK(member >= -1 && member < h->B, RS_ERR_ARG, "member %d outside [-1, %d)", member, h->B);
    RS_CHECK(x >= 0 && x < h->X && y >= 0 && y < h->Y && th >= 0 && th < h->TH, RS_ERR_ARG,
             "cell (%d, %d, %d) outside grid (%d, %d, %d)", x, y, th, h->X, h->Y, h->TH);
    RS_HIP(hipSetDevice(h->device));
    hipLaunchKernelGGL(pce_inject_kernel, dim3((h->B + 255) / 256), dim3(256), 0, h->stream.get(), h->dState.get(), h->B,
                       (int)h->N, member, (x * h->Y + y) * h->TH + th, (float)energy);
    RS_HIP(hipGetLastError());
    return RS_OK;
}

int rs_pce_get_max(rs_pce* h, int32_t* out_xyz) {
    rs::clear_error();
    RS_CHECK(h, RS_ERR_STATE, "null ensemble handle");
    RS_CHECK(out_xyz, RS_ERR_ARG, "null argument");
    RS_HIP(hipSetDevice(h->device));
    hipLaunchKernelGGL(pce_argmax_kernel, dim3(h->B), dim3(PCE_ARGMAX_THREADS), 0, h->stream.get(), h->dState.get(),
                       (int)h->N, h->Y, h->TH, h->dOut.get());
    RS_HIP(hipGetLastError());
    RS_HIP(hipMemcpyAsync(h->hOut.get(), h->dOut.get(), sizeof(int32_t) * 3 * h->B, hipMemcpyDeviceToHost, h->stream.get()));
    RS_HIP(hipStreamSynchronize(h->stream.get()));
    std::memcpy(out_xyz, h->hOut.get(), sizeof(int32_t) * 3 * h->B);
    return RS_OK;
}

int rs_pce_read(rs_pce* h, int first, int count, double* volumes) {
    rs::clear_error();
    RS_CHECK(h, RS_ERR_STATE, "null ensemble handle");
    RS_CHECK(first >= 0 && count >= 0 && first <= h->B && count <= h->B - first, RS_ERR_ARG,
             "members [%d, %d + %d) outside the %d of the ensemble", first, first, count, h->B);
    if (count == 0) return RS_OK;
    RS_CHECK(volumes, RS_ERR_ARG, "null argument");
    RS_HIP(hipSetDevice(h->device));
    const size_t cells = (size_t)count * h->N;
    if (cells > h->hState.capacity()) RS_HIP(hipStreamSynchronize(h->stream.get()));
    RS_TRY(h->hState.reserve(cells, hipHostMallocDefault, "ensemble staging"));
    RS_HIP(hipMemcpyAsync(h->hState.get(), h->dState.get() + (size_t)first * h->N, sizeof(float) * cells,
                          hipMemcpyDeviceToHost, h->stream.get()));
    RS_HIP(hipStreamSynchronize(h->stream.get()));
    const float* st = h->hState.get();
    for (size_t i = 0; i < cells; ++i) volumes[i] = (double)st[i];
    return RS_OK;
}

int rs_pce_write(rs_pce* h, int first, int count, const double* volumes) {
    rs::clear_error();
    RS_CHECK(h, RS_ERR_STATE, "null ensemble handle");
    RS_CHECK(first >= 0 && count >= 0 && first <= h->B && count <= h->B - first, RS_ERR_ARG,
             "members [%d, %d + %d) outside the %d of the ensemble", first, first, count, h->B);
    if (count == 0) return RS_OK;
    RS_CHECK(volumes, RS_ERR_ARG, "null argument");
    const size_t cells = (size_t)count * h->N;
    for (size_t i = 0; i < cells; ++i)
        if (!std::isfinite(volumes[i]) || !std::isfinite((float)volumes[i])) {
            rs::set_error("member %zu, cell %zu: %g is not a finite float32", first + i / h->N, i % h->N, volumes[i]);
            return RS_ERR_ARG;
        }
    RS_HIP(hipSetDevice(h->device));
    RS_HIP(hipStreamSynchronize(h->stream.get()));   // the staging is free, a growth frees nothing in use
    RS_TRY(h->hState.reserve(cells, hipHostMallocDefault, "ensemble staging"));
    float* st = h->hState.get();
    for (size_t i = 0; i < cells; ++i) st[i] = (float)volumes[i];
    RS_HIP(hipMemcpyAsync(h->dState.get() + (size_t)first * h->N, st, sizeof(float) * cells, hipMemcpyHostToDevice,
                          h->stream.get()));
    RS_HIP(hipStreamSynchronize(h->stream.get()));
    return RS_OK;
}

int rs_pce_set_timing(rs_pce* h, int enable) {
    rs::clear_error();
    RS_CHECK(h, RS_ERR_STATE, "null ensemble handle");
    h->timing = enable != 0;
    return RS_OK;
}

int rs_pce_last_ms(rs_pce* h, double* ms) {
    rs::clear_error();
    RS_CHECK(h && ms, RS_ERR_ARG, "null argument");
    *ms = -1.0;
    if (!h->timed) return RS_OK;
    float t = 0.f;
    RS_HIP(hipEventSynchronize(h->ev[1].get()));
    RS_HIP(hipEventElapsedTime(&t, h->ev[0].get(), h->ev[1].get()));
    *ms = t;
    return RS_OK;
}

}  // extern "C"
