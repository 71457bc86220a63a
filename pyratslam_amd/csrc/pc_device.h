// Pose-cell device code that every kernel form uses: the block size and the result
// slots, the step's parameter and control types, the argmax order (first maximum in the
// reference's C order, a NaN above every number), the block and wave reductions, the
// write-through stores and the filter-table staging shared by the forms.
// Part of posecell.hip, the one translation unit: not free-standing (it relies on the
// includes and on the headers that posecell.hip includes before it).

namespace {

constexpr int NT = 256;            // threads per block (4 waves)
constexpr int FT = FL * FL;        // 49 taps of a 2-D filter

template <typename T>
struct SepKernel {
    T ge[FL];
    T gi[FL];
    T scale;
    T inhib;
};

// The normalisation P /= total (posecell_network.py:343-345).  float32: a product with
// the reciprocal of the total, rounded once from double (within an ulp of the division;
// one VALU op per value); where that reciprocal is not a finite float (a total below
// about 2.9e-39) each value is divided instead.  float64: the division, as the reference.
// A zero total leaves the volume as it is (:344).
template <typename T>
struct PcNorm;
template <>
struct PcNorm<float> {
    float r, t;
    bool div;
    __device__ PcNorm(float r_, float t_, bool div_) : r(r_), t(t_), div(div_) {}
    __device__ explicit PcNorm(double tot) {
        const float rf = (float)(tot != 0.0 ? 1.0 / tot : 1.0);
        // wave-uniform (every lane formed the same total): a scalar branch below, so the
        // division is never speculated into the common path
        div = __builtin_amdgcn_readfirstlane((int)!__builtin_isfinite(rf)) != 0;
        r = div ? 1.0f : rf;
        t = div ? (float)tot : 1.0f;
    }
    __device__ float operator()(float x) const {
        float y = x * r;
        if (div) {
            asm volatile("" ::: "memory");
            y = x / t;
        }
        return y;
    }
    template <int N>
    __device__ void operator()(float (&p)[N]) const {
        if (div) {
            asm volatile("" ::: "memory");
#pragma unroll
            for (int q = 0; q < N; ++q) p[q] = p[q] / t;
        } else {
#pragma unroll
            for (int q = 0; q < N; ++q) p[q] = p[q] * r;
        }
    }
};
template <>
struct PcNorm<double> {
    double t;
    __device__ explicit PcNorm(double tot) : t(tot != 0.0 ? tot : 1.0) {}
    __device__ double operator()(double x) const { return x / t; }
};

// Per-step control of the path-integration kernel: PcCtlInline (pc_ctl.h), or pointers
// into a device ring.
struct PcCtlRing {       // batched run(): one record per step, uploaded once per batch
    const int* ox;
    const int* oy;
    const int* f;
    const double* zf;
};

__device__ inline int ctl_ox(const PcCtlInline& c, int L) { return c.iox[L]; }
__device__ inline int ctl_oy(const PcCtlInline& c, int L) { return c.ioy[L]; }
__device__ inline int ctl_fi(const PcCtlInline& c, int L) { return c.ifi[L]; }
__device__ inline double ctl_zf(const PcCtlInline& c, int z) { return c.izf[z]; }
__device__ inline int ctl_ox(const PcCtlRing& c, int L) { return c.ox[L]; }
__device__ inline int ctl_oy(const PcCtlRing& c, int L) { return c.oy[L]; }
__device__ inline int ctl_fi(const PcCtlRing& c, int L) { return c.f[L]; }
__device__ inline double ctl_zf(const PcCtlRing& c, int z) { return c.zf[z]; }

// float32 argmax: one packed key per block, max-reduced into slot b % RES_SLOTS;
// pc_res_export takes each step's max.  256 slots: one block per slot on the
// column and rows grids (with 8 slots, 32 contending 64-bit atomics per address
// held each step's end back: 64x64x36 13.35 -> 12.32 us per batched step,
// 128x128x72 27.7 -> 26.8, tools/pc_ab.py).
constexpr int RES_SLOTS = 256;
// Step outputs are >= 0 or NaN (every step ends in a clamp), so the value bits order
// like the values (-0 taken as +0); every NaN is given one bit pattern above +inf, so
// that, as in numpy's argmax, a NaN beats every number and the first NaN wins.
__device__ inline unsigned long long argmax_key(float v, unsigned lin) {
    const unsigned bits = v != v ? 0x7FC00000u : v == 0.f ? 0u : __float_as_uint(v);  // -0 as +0
    return ((unsigned long long)bits << 32) | (0xFFFFFFFFu - lin);
}
// The clamps P[P < 0] = 0 (posecell_network.py:300,314): as the reference, a NaN stays
// a NaN (x > 0 ? x : 0 would zero it)
template <typename T>
__device__ inline T pc_clamp(T x) {
    return x < T(0) ? T(0) : x;
}
// The same order for (value, index) pairs (float64 steps, get_pc_max): a NaN beats every
// number, ties and NaNs among themselves go to the lower index; start from (-inf, ~0u).
template <typename T>
__device__ inline bool pc_better(T v, unsigned l, T bv, unsigned bl) {
    const bool vn = v != v, bn = bv != bv;
    return vn ? (!bn || l < bl) : (!bn && (v > bv || (v == bv && l < bl)));
}

// Phase-stamp hooks, empty in the library.  tools/pc_probe.hip defines them (a
// per-block s_memrealtime stamp) before it includes this file.
#ifndef PC_STAMP
#define PC_STAMP(kid, sid) \
    do {                   \
    } while (0)
#endif
#ifndef PC_STAMPW
#define PC_STAMPW(kid) \
    do {               \
    } while (0)
#endif

// A step's small result words (the normalisation partials, the argmax slots zeroed
// for the path kernel) stored write-through: an agent-scope relaxed atomic store is a
// plain store with sc1 on gfx950, so the line leaves the XCD's L2 at once and the
// kernel ends with nothing of these left dirty to write back at its boundary
// (tools/pc_ab.py, 5 rounds: 16.65 -> 16.49 us per 128x128x72 step, 11.41 -> 11.18 us
// per 64x64x36 step).
template <typename V>
__device__ inline void st_wt(V* p, V v) {
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Deterministic block sum of one double per thread (same value returned to all).
__device__ inline double block_sum(double v, double* s_red) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) s_red[w] = v;
    __syncthreads();
    double t = 0.0;
#pragma unroll
    for (int i = 0; i < NT / 64; ++i) t += s_red[i];
    __syncthreads();
    return t;
}

// path filter tables: staged in LDS by the stream, cols and halo forms
constexpr int RT_NFMAX = 8;  // filter tables up to this size are preloaded whole
constexpr int ST_FTP = 52;                // filter stride in LDS: 49 taps padded to 13 x 16 B

template <int NW>
__device__ inline double block_sum_w(double v, double* s_red) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = v;
    __syncthreads();
    double t = 0.0;
#pragma unroll
    for (int i = 0; i < NW; ++i) t += s_red[i];
    return t;
}

// Block barrier for LDS traffic only: waits for this wave's LDS operations, not
// for its global stores (a __syncthreads fence would drain those too).
__device__ inline void co_lds_barrier() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
}

// Wave-wide reductions by DPP row operations instead of ds_bpermute shuffles (six
// dependent LDS round trips each): within every 16-lane row by quad_perm xor 1,
// xor 2, row_half_mirror and row_mirror, then over the 4 rows by readlane.  Every
// lane computes the same additions on the same two operands at each step, so the
// result is identical in all lanes (wave-uniform) and deterministic.
template <int CTRL>
__device__ inline unsigned long long co_dpp64(unsigned long long v) {
    const int lo = __builtin_amdgcn_update_dpp(0, (int)(unsigned)v, CTRL, 0xF, 0xF, false);
    const int hi = __builtin_amdgcn_update_dpp(0, (int)(unsigned)(v >> 32), CTRL, 0xF, 0xF, false);
    return ((unsigned long long)(unsigned)hi << 32) | (unsigned)lo;
}
__device__ inline unsigned long long co_readlane64(unsigned long long v, int l) {
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)v, l);
    const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(v >> 32), l);
    return ((unsigned long long)hi << 32) | lo;
}
__device__ inline double co_wave_sum(double v) {
    v += __longlong_as_double((long long)co_dpp64<0xB1>((unsigned long long)__double_as_longlong(v)));
    v += __longlong_as_double((long long)co_dpp64<0x4E>((unsigned long long)__double_as_longlong(v)));
    v += __longlong_as_double((long long)co_dpp64<0x141>((unsigned long long)__double_as_longlong(v)));
    v += __longlong_as_double((long long)co_dpp64<0x140>((unsigned long long)__double_as_longlong(v)));
    const unsigned long long b = (unsigned long long)__double_as_longlong(v);
    return (__longlong_as_double((long long)co_readlane64(b, 0)) +
            __longlong_as_double((long long)co_readlane64(b, 16))) +
           (__longlong_as_double((long long)co_readlane64(b, 32)) +
            __longlong_as_double((long long)co_readlane64(b, 48)));
}
__device__ inline unsigned long long co_wave_max(unsigned long long v) {
    v = max(v, co_dpp64<0xB1>(v));
    v = max(v, co_dpp64<0x4E>(v));
    v = max(v, co_dpp64<0x141>(v));
    v = max(v, co_dpp64<0x140>(v));
    return max(max(co_readlane64(v, 0), co_readlane64(v, 16)),
               max(co_readlane64(v, 32), co_readlane64(v, 48)));
}

// The argmax reductions: pc_better's order for (value, index) pairs, the packed keys' for
// float32 steps (argmax_key: the same order, as unsigned integers).
// The wave's best pair: pairs are totally ordered, so every lane ends on the same pair.
template <typename T>
struct PcBest {
    T v;
    unsigned l;
};
template <typename T>
__device__ inline PcBest<T> pc_wave_best(T bv, unsigned bl) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const T ov = __shfl_xor(bv, off);
        const unsigned ol = __shfl_xor(bl, off);
        if (pc_better(ov, ol, bv, bl)) {
            bv = ov;
            bl = ol;
        }
    }
    return {bv, bl};
}
// The best pair of a block of NW waves, returned to thread 0: one LDS slot per wave
// (s_bv, s_bl) at the caller's wave index (rows holds it in a scalar register), the
// caller's barrier, thread 0 folds the slots.
template <int NW, typename T, typename BARRIER>
__device__ inline PcBest<T> pc_block_best(T bv_, unsigned bl_, T* s_bv, unsigned* s_bl, int wave, BARRIER barrier) {
    auto [bv, bl] = pc_wave_best(bv_, bl_);
    if ((threadIdx.x & 63) == 0) {
        s_bv[wave] = bv;
        s_bl[wave] = bl;
    }
    barrier();
    if (threadIdx.x == 0) {
        for (int w = 1; w < NW; ++w)
            if (pc_better(s_bv[w], s_bl[w], bv, bl)) {
                bv = s_bv[w];
                bl = s_bl[w];
            }
    }
    return {bv, bl};
}
// The largest packed key of block b (NW waves; wave: the caller's wave index) into the
// step's slot b % RES_SLOTS.
template <int NW>
__device__ inline void pc_block_key_max(unsigned long long bk, unsigned long long* __restrict__ res_slot, int b,
                                        int wave) {
    __shared__ unsigned long long s_bk[NW];
    bk = co_wave_max(bk);
    if ((threadIdx.x & 63) == 0) s_bk[wave] = bk;
    co_lds_barrier();
    if (threadIdx.x == 0) {
        for (int w = 1; w < NW; ++w) bk = max(bk, s_bk[w]);
        atomicMax(res_slot + (b & (RES_SLOTS - 1)), bk);
    }
}
// The best pair of a block of NT threads by an LDS tree, returned to thread 0.
template <typename T>
__device__ inline PcBest<T> pc_tree_best(T bv, unsigned bl) {
    __shared__ T s_bv[NT];
    __shared__ unsigned s_bl[NT];
    s_bv[threadIdx.x] = bv;
    s_bl[threadIdx.x] = bl;
    __syncthreads();
    for (int s = NT / 2; s > 0; s >>= 1) {
        if (threadIdx.x < s) {
            const T v = s_bv[threadIdx.x + s];
            const unsigned l = s_bl[threadIdx.x + s];
            if (pc_better(v, l, s_bv[threadIdx.x], s_bl[threadIdx.x])) {
                s_bv[threadIdx.x] = v;
                s_bl[threadIdx.x] = l;
            }
        }
        __syncthreads();
    }
    return {s_bv[0], s_bl[0]};
}
// The max of a step's RES_SLOTS slot words r on one wave (every lane gets it): each lane
// takes RES_SLOTS / 64 slots, then DPP.  (Keys are unsigned: 0 is below every key.)
__device__ inline unsigned long long pc_slots_max(const unsigned long long* __restrict__ r) {
    static_assert(RES_SLOTS % 64 == 0, "slots per lane");
    unsigned long long m = 0ull;
#pragma unroll
    for (int q = 0; q < RES_SLOTS / 64; ++q) m = max(m, r[(threadIdx.x & 63) + 64 * q]);
    return co_wave_max(m);
}

// XCD-aware tile numbering (pc_stream.h): dispatch is round-robin over the 8 XCDs, and XCD x
// takes a contiguous run of tiles
__device__ inline int st_tile(int b, int nb) {
    if ((nb & 7) != 0) return b;
    return (b & 7) * (nb >> 3) + (b >> 3);
}

// window coordinate a in [-n, 2n) -> [0, n)
__device__ inline int co_wrap(int a, int n) {
    a += a < 0 ? n : 0;
    return a - (a >= n ? n : 0);
}

// A 16-byte output vector at element offset e of a volume of nbytes bytes, stored
// write-through (sc1: the line leaves the XCD's L2 at once, so the kernel ends with
// nothing dirty to write back -- 128x128x72: 27.7 -> 24.3 us per batched step with
// the 16-byte theta-pass stores, tools/pc_ab.py; the excite -> path boundary gap
// 3.5 -> 2.1 us, tools/pc_probe.hip); volumes of 2 GiB or more: plain stores.
template <typename T, typename V>
__device__ inline void co_put(T* __restrict__ base, size_t e, V v, bool wt, int nbytes) {
    if (wt) {
        const __amdgpu_buffer_rsrc_t r = __builtin_amdgcn_make_buffer_rsrc(base, (short)0, nbytes, 0x00020000);
        if constexpr (sizeof(V) == 8) {
            typedef unsigned v2u __attribute__((ext_vector_type(2)));
            __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(v2u, v), r, (int)(e * sizeof(T)), 0, 16);
        } else {
            typedef unsigned v4u __attribute__((ext_vector_type(4)));
            __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(v4u, v), r, (int)(e * sizeof(T)), 0, 16);
        }
        return;
    }
    (void)wt;
    (void)nbytes;
    *reinterpret_cast<V*>(base + e) = v;
}

template <typename T>
struct CoVec;
// native vector types: their copies are vector loads/stores, not memcpys (a window
// array of HIP_vector_type kept live across a loop stayed in scratch)
typedef float co_f4 __attribute__((ext_vector_type(4)));
typedef double co_d2 __attribute__((ext_vector_type(2)));
template <>
struct CoVec<float> { using type = co_f4; };
template <>
struct CoVec<double> { using type = co_d2; };

// 49 filter taps from LDS (uniform address: broadcast reads, 16 B each for float)
template <typename T>
__device__ inline void st_filter(const T* __restrict__ src, T (&f)[FT]) {
    if constexpr (sizeof(T) == 4) {
        const float4* s4 = reinterpret_cast<const float4*>(src);
#pragma unroll
        for (int q = 0; q < ST_FTP / 4; ++q) {
            const float4 v = s4[q];
            if (4 * q + 0 < FT) f[4 * q + 0] = v.x;
            if (4 * q + 1 < FT) f[4 * q + 1] = v.y;
            if (4 * q + 2 < FT) f[4 * q + 2] = v.z;
            if (4 * q + 3 < FT) f[4 * q + 3] = v.w;
        }
    } else {
#pragma unroll
        for (int t = 0; t < FT; ++t) f[t] = src[t];
    }
}

}  // namespace
