// Pose-cell kernels on the stored state and on a step's result words, whatever the form:
// the key export, the argmax of (value, index) partials, export / import / inject /
// total, the packet's centroid and rs_pc_excite's scaling.
// Part of posecell.hip, the one translation unit: not free-standing (it relies on the
// includes and on the headers that posecell.hip includes before it).

namespace {

// Each step's RES_SLOTS packed argmax keys -> their max, stored straight into the
// pinned host buffer (system-scope stores): one queued launch in place of a
// device-to-host blit copy, which trailed the step by ~10 us (gap + copy kernel).
// One wave per step: each lane takes the max of RES_SLOTS / 64 slots, then DPP.
__global__ __launch_bounds__(64) void pc_res_export(const unsigned long long* __restrict__ res, int n,
                                                    unsigned long long* host) {
    for (int s = blockIdx.x; s < n; s += gridDim.x) {
        const unsigned long long m = pc_slots_max(res + (size_t)s * RES_SLOTS);
        if (threadIdx.x == 0) __hip_atomic_store(host + s, m, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}

// The halo form's key export for a call that leaves its state unnormalised: steps
// 0 .. n-2 as pc_res_export (each keyed by the next launch from the scaled state it
// loaded); step n-1 from the last launch's per-block records of U.  P = U * (1/t) with
// t > 0 (or P = U when t == 0, or U / t where 1/t is not finite) rounds monotonically,
// so P's first maximum is U's, unless some other cell's U lies within HF_NEAR of the
// maximum (it might round to the same P, and the earlier index would win): then the
// word is RES_AMBIG and the host settles the state exactly (pc_halo_finish).  NaN, 0
// and inf maxima are exact (their products are the same value for every such cell).
__global__ __launch_bounds__(64) void pc_halo_export(const unsigned long long* __restrict__ res, int n,
                                                     const unsigned long long* __restrict__ rec, int nrec,
                                                     unsigned long long* host) {
    const int lane = threadIdx.x;
    for (int s = blockIdx.x; s < n; s += gridDim.x) {
        unsigned long long m = 0ull;
        if (s < n - 1 || rec == nullptr) {
            m = pc_slots_max(res + (size_t)s * RES_SLOTS);
        } else {
            for (int b = lane; b < nrec; b += 64) m = max(m, rec[2 * b]);
            m = co_wave_max(m);
            const float gv = __uint_as_float((unsigned)(m >> 32)), thr = gv - gv * HF_NEAR;
            const bool exact = !(gv > 0.f) || gv == __builtin_inff() || gv != gv;   // 0 (all zero), inf, NaN
            bool amb = false;
            for (int b = lane; b < nrec; b += 64) {
                const unsigned long long kb = rec[2 * b];
                amb |= kb == m ? (rec[2 * b + 1] & ~REC_SET) > 1ull : __uint_as_float((unsigned)(kb >> 32)) >= thr;
            }
            amb = __ballot(amb) != 0ull;
            if (!exact && amb) m = RES_AMBIG;
        }
        if (lane == 0) __hip_atomic_store(host + s, m, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}

// Per-step argmax: block s reduces the nb (value, index) partials of step s (one block:
// pc_argmax_blocks' partials of the stored state, the key into res[0]).
template <typename T>
__global__ __launch_bounds__(NT) void pc_argmax_steps(const T* __restrict__ bmax,
                                                      const unsigned* __restrict__ bidx, int nb,
                                                      unsigned long long* __restrict__ res) {
    const size_t base = (size_t)blockIdx.x * nb;
    T bv = -std::numeric_limits<T>::infinity();
    unsigned bl = 0xFFFFFFFFu;
    for (int i = threadIdx.x; i < nb; i += NT) {
        const T v = bmax[base + i];
        const unsigned l = bidx[base + i];
        if (pc_better(v, l, bv, bl)) {
            bv = v;
            bl = l;
        }
    }
    const PcBest<T> best = pc_tree_best(bv, bl);
    if (threadIdx.x == 0) res[(size_t)blockIdx.x * RES_SLOTS] = 0xFFFFFFFFull - best.l;  // same decoding as the packed key
}

// Argmax of the stored state (get_pc_max outside update): per-block partials.
template <typename T>
__global__ __launch_bounds__(NT) void pc_argmax_blocks(const T* __restrict__ P, int X, int Y, int TH,
                                                       T* __restrict__ bmax,
                                                       unsigned* __restrict__ bidx, int thfast) {
    const size_t n = (size_t)X * Y * TH;
    T bv = -std::numeric_limits<T>::infinity();
    unsigned bl = 0xFFFFFFFFu;
    for (size_t e = blockIdx.x * (size_t)NT + threadIdx.x; e < n; e += (size_t)gridDim.x * NT) {
        const int k = (int)(e / ((size_t)X * Y));
        const int rem = (int)(e - (size_t)k * X * Y);
        const int i = rem / Y, j = rem - i * Y;
        const T v = P[e];
        const unsigned lin = thfast ? (unsigned)e : ((unsigned)i * Y + j) * TH + k;
        if (pc_better(v, lin, bv, bl)) {
            bv = v;
            bl = lin;
        }
    }
    const PcBest<T> best = pc_tree_best(bv, bl);
    if (threadIdx.x == 0) {
        bmax[blockIdx.x] = best.v;
        bidx[blockIdx.x] = best.l;
    }
}

// Element e of the C-order (x, y, th) volume -> its place in a layer-major volume
// (or itself in a theta-fastest one: the column form's P, which is C order).
__device__ inline size_t pc_layer_major(size_t e, int X, int Y, int TH) {
    const int k = (int)(e % TH);
    const size_t xy = e / TH;
    const int j = (int)(xy % Y), i = (int)(xy / Y);
    return ((size_t)k * X + i) * Y + j;
}

// The float64 C-order export with 16-byte stores (two consecutive cells per thread): a wave's
// stores are 1 KiB contiguous, the unit host writes over PCIe favour.  out is
// 16-byte aligned (rs_host_alloc / hipMalloc); an odd last cell goes alone.
// flag (host memory the host polls instead of the stream's completion, pc_poll_flags):
// every wave's volume stores acknowledged, the block's barrier, one lane's system-scope
// release, then the block's flag = seq -- the producer form of pc_halo_finish.
template <typename T>
__global__ void pc_export2_kernel(const T* __restrict__ P, double* __restrict__ out, int X, int Y,
                                  int TH, int thfast, unsigned* __restrict__ flag, unsigned seq) {
    typedef double d2 __attribute__((ext_vector_type(2)));
    const size_t n = (size_t)X * Y * TH, n2 = n / 2;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n2; i += (size_t)gridDim.x * blockDim.x) {
        const size_t e = 2 * i;
        d2 v;
        v.x = (double)P[thfast ? e : pc_layer_major(e, X, Y, TH)];
        v.y = (double)P[thfast ? e + 1 : pc_layer_major(e + 1, X, Y, TH)];
        *reinterpret_cast<d2*>(out + e) = v;
    }
    if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0)
        out[n - 1] = (double)P[thfast ? n - 1 : pc_layer_major(n - 1, X, Y, TH)];
    if (flag) {   // (kernel argument: uniform)
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        if (threadIdx.x == 0) {
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "");
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __hip_atomic_store(flag + blockIdx.x, seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        }
    }
}

template <typename T>
__global__ void pc_import_kernel(const double* __restrict__ in, T* __restrict__ P, int X, int Y,
                                 int TH, int thfast) {
    const size_t n = (size_t)X * Y * TH;
    for (size_t e = blockIdx.x * (size_t)blockDim.x + threadIdx.x; e < n;
         e += (size_t)gridDim.x * blockDim.x)
        P[thfast ? e : pc_layer_major(e, X, Y, TH)] = (T)in[e];
}


template <typename T>
__global__ void pc_inject_kernel(T* __restrict__ P, size_t idx, double energy) {
    if (threadIdx.x == 0) P[idx] = (T)((double)P[idx] + energy);
}

// An injection inside a batched run (rs_pc_run_odom_inject): one wave resolves the cell and
// adds, with pc_inject_kernel's arithmetic.  The cell, as a C-order linear index, comes from
//   PC_INJ_EXPLICIT  arg itself (the host checked it against the grid);
//   PC_INJ_KEY       the key words pc_peak_kernel reads, reduced the same way: a float32
//                    step's RES_SLOTS slot words (slot), else nb (value, index) block partials
//                    (a float64 step's, or pc_argmax_blocks' of the stored state);
//   PC_INJ_SAME      cells[arg], what an earlier injection of this call resolved to.
// The resolved index goes to cells[i] for later launches of the call, ordered behind this one
// on the stream, and to hcells[i] in pinned memory for the host (plain stores both: the host
// reads them only once it has synchronised the stream, as it does a peaks call's sums).  No address outside P
// is formed: a key no step wrote is clamped to cell 0 as pc_peak_kernel clamps it, and an
// explicit or same-as index that is no cell (PC_INJ_NONE: an injection that never ran) adds
// nothing and resolves to PC_INJ_NONE.
enum { PC_INJ_EXPLICIT = 0, PC_INJ_KEY = 1, PC_INJ_SAME = 2 };
constexpr unsigned PC_INJ_NONE = 0xFFFFFFFFu;

template <typename T>
__global__ __launch_bounds__(64) void pc_inject_run_kernel(T* __restrict__ P, int X, int Y, int TH, int thfast,
                                                           int src, unsigned arg,
                                                           const unsigned long long* __restrict__ slot,
                                                           const T* __restrict__ bmax,
                                                           const unsigned* __restrict__ bidx, int nb,
                                                           unsigned* cells, unsigned* __restrict__ hcells, int i,
                                                           double energy) {
    const int lane = threadIdx.x;
    const unsigned ncell = (unsigned)X * Y * TH;
    unsigned lin;
    if (src == PC_INJ_KEY) {   // (kernel arguments: uniform branches)
        if (slot) {
            lin = 0xFFFFFFFFu - (unsigned)(pc_slots_max(slot) & 0xFFFFFFFFull);
        } else {
            T bv = -std::numeric_limits<T>::infinity();
            unsigned bl = 0xFFFFFFFFu;
            for (int b = lane; b < nb; b += 64) {
                const T v = bmax[b];
                const unsigned l = bidx[b];
                if (pc_better(v, l, bv, bl)) {
                    bv = v;
                    bl = l;
                }
            }
            lin = pc_wave_best(bv, bl).l;
        }
        if (lin >= ncell) lin = 0u;
    } else if (src == PC_INJ_SAME) {
        lin = arg < (unsigned)i ? cells[arg] : PC_INJ_NONE;
    } else {
        lin = arg;
    }
    if (lane != 0) return;
    if (lin >= ncell) {
        cells[i] = PC_INJ_NONE;
        hcells[i] = PC_INJ_NONE;
        return;
    }
    const unsigned th = lin % (unsigned)TH, xy = lin / (unsigned)TH;
    const unsigned y = xy % (unsigned)Y, x = xy / (unsigned)Y;
    const size_t idx = thfast ? (size_t)lin : ((size_t)th * X + x) * Y + y;
    P[idx] = (T)((double)P[idx] + energy);
    cells[i] = lin;
    hcells[i] = lin;
}

template <typename T>
__global__ __launch_bounds__(NT) void pc_total_kernel(const T* __restrict__ P, size_t n,
                                                      double* __restrict__ out) {
    __shared__ double s_red[NT / 64];
    double s = 0.0;
    for (size_t e = threadIdx.x; e < n; e += NT) s += (double)P[e];
    s = block_sum(s, s_red);
    if (threadIdx.x == 0) *out = s;
}

// The activity packet's circular centroid round a step's first maximum (pc_peak_rule.h,
// DESIGN section 24): one wave per launch, queued where the step's state and its argmax key
// are both on the device.  The wave reduces the key itself -- a float32 step's RES_SLOTS
// slot words (slot), else nb (value, index) block partials (bmax, bidx: a float64 step's,
// or pc_argmax_blocks' of the stored state) -- decodes the cell as decode_xyz does, gathers
// the wrapped box of (2r+1)^3 cells from P (layer-major, or theta-fastest: thfast) into LDS
// as float64, and takes the rule's stages on at most 49 lanes each: R and C, the three
// marginals, the six dot products with the uploaded weights.  The rule fixes the order of
// every sum, so the bits do not depend on the lane mapping.  Six plain 8-byte stores.
template <typename T>
__global__ __launch_bounds__(64) void pc_peak_kernel(const T* __restrict__ P, int X, int Y, int TH, int thfast,
                                                     int r, const unsigned long long* __restrict__ slot,
                                                     const T* __restrict__ bmax, const unsigned* __restrict__ bidx,
                                                     int nb, const double* __restrict__ tabs,
                                                     double* __restrict__ out) {
    constexpr int W = rs::PC_PEAK_WMAX;
    __shared__ double s_v[W * W * W];
    __shared__ double s_R[W * W], s_C[W * W], s_m[3 * W], s_t[6 * W];
    const int lane = threadIdx.x, w = 2 * r + 1;
    unsigned lin;
    if (slot) {
        lin = 0xFFFFFFFFu - (unsigned)(pc_slots_max(slot) & 0xFFFFFFFFull);
    } else {
        T bv = -std::numeric_limits<T>::infinity();
        unsigned bl = 0xFFFFFFFFu;
        for (int i = lane; i < nb; i += 64) {
            const T v = bmax[i];
            const unsigned l = bidx[i];
            if (pc_better(v, l, bv, bl)) {
                bv = v;
                bl = l;
            }
        }
        bl = pc_wave_best(bv, bl).l;
        lin = bl;
    }
    if (lin >= (unsigned)X * Y * TH) lin = 0u;   // (a key no step wrote: never an address outside P)
    const int pth = (int)(lin % (unsigned)TH);
    const unsigned xy = lin / (unsigned)TH;
    const int py = (int)(xy % (unsigned)Y), px = (int)(xy / (unsigned)Y);
    // the six rows of weights the last stage multiplies by (row q: axis q / 2, sin then cos),
    // loaded with the box: one memory round trip behind the key, not one more behind the sums
    double tw = 0.0;
    if (lane < 6 * w) {
        const int q = lane / w, a = q >> 1;
        const int n = a == 0 ? X : a == 1 ? Y : TH, p = a == 0 ? px : a == 1 ? py : pth;
        tw = tabs[(a == 0 ? 0 : a == 1 ? 2 * X : 2 * (X + Y)) + (q & 1) * n + rs::pc_peak_wrap(p, lane % w, r, n)];
    }
    for (int e = lane; e < w * w * w; e += 64) {
        const int k = e % w, ij = e / w, j = ij % w, i = ij / w;
        const size_t cx = rs::pc_peak_wrap(px, i, r, X), cy = rs::pc_peak_wrap(py, j, r, Y),
                     ck = rs::pc_peak_wrap(pth, k, r, TH);
        s_v[e] = (double)P[thfast ? (cx * Y + cy) * TH + ck : (ck * X + cx) * Y + cy];
    }
    if (lane < 6 * w) s_t[lane] = tw;
    __syncthreads();
    if (lane < w * w) {
        s_R[lane] = rs::pc_peak_R(s_v, w, lane / w, lane % w);
        s_C[lane] = rs::pc_peak_C(s_v, w, lane / w, lane % w);
    }
    __syncthreads();
    if (lane < 3 * w) s_m[lane] = rs::pc_peak_marginal(s_R, s_C, w, lane / w, lane % w);
    __syncthreads();
    if (lane < 6) out[lane] = rs::pc_peak_dot_w(s_m + (lane >> 1) * w, s_t + lane * w, w);
}

// Scale the excited volume by 1/total in place (rs_pc_excite only).
template <typename T>
__global__ void pc_scale_kernel(T* __restrict__ P, size_t n, const double* __restrict__ part,
                                int npart) {
    __shared__ double s_red[NT / 64];
    double t = 0.0;
    for (int i = threadIdx.x; i < npart; i += NT) t += part[i];
    t = block_sum(t, s_red);
    if (t == 0.0) return;
    const PcNorm<T> nrm(t);
    for (size_t e = blockIdx.x * (size_t)NT + threadIdx.x; e < n; e += (size_t)gridDim.x * NT)
        P[e] = nrm(P[e]);
}

}  // namespace
