// stream : pc_excite_stream + pc_path_stream, a block walks a chunk of layers behind a
//          prefetch ring; large grids outside the column form's limits
// Part of posecell.hip, the one translation unit: not free-standing (it relies on the
// includes and on the headers that posecell.hip includes before it).

namespace {

// ---------------------------------------------------------------------------
// Layer-streaming forms (large grids).  A block of WR x WC waves owns BXB = BX*WR
// rows x YT = 64*WC columns x KC layers of the output and walks its KC + 6
// input layers in order.  Per input layer only 2-D work is done (window load
// into double-buffered LDS, then the y and x passes or the 7x7 filter); the
// 7-tap theta pass runs on a 7-deep register ring of per-lane results, so the
// 2-D passes are evaluated (KC+6)/KC times per cell instead of the rows form's
// (BK+6)/BK = 4x.  Lane <-> column; each wave register-blocks BX rows.
// Window loads run ST_PF layers ahead of use (a 7-slot register ring, so the
// slot of every stage is a compile-time index of the 7-way unrolled layer loop).
// Every stage is straight-line: unconditional loads and LDS stores, and the
// outputs go to an LDS buffer written back after the loop, so the only
// vector-memory operations in the loop are the in-order window loads and the
// compiler's vmcnt wait at each stage covers just that stage's slot (a global
// store in flight makes it drain every prefetch).  The per-layer control
// (shifts, filter index) and the filter table are staged in LDS once per block.
// Tiles are numbered XCD-aware: dispatch is round-robin over the 8 XCDs, and
// XCD x takes a contiguous run of tiles, so neighbouring tiles' halo rows and
// layers meet in the same L2.
// ---------------------------------------------------------------------------
constexpr int ST_PF = 3;                  // window prefetch distance (layers)
// The streaming grids hold 1-2 blocks per CU, so occupancy buys nothing: let the
// scheduler spend registers on keeping LDS reads in flight (at the default
// occupancy target it serialises every ds_read behind an lgkmcnt(0)).
#define PC_ST_WAVES __attribute__((amdgpu_waves_per_eu(1, 2)))
constexpr int ST_MAXKC = 12;              // layers per block (outputs buffered in LDS)
constexpr int ST_MAXL = ST_MAXKC + 2 * 3 + ST_PF + 1;  // control entries staged in LDS
constexpr int ST_OUT_BYTES = 24 * 1024;   // LDS output buffer per block
// layers per block that fit the output buffer for a tile of bxb x yt cells of esz bytes
__host__ __device__ constexpr int st_maxkc(int esz, int bxb, int yt) {
    return ST_OUT_BYTES / (esz * bxb * yt) < ST_MAXKC ? ST_OUT_BYTES / (esz * bxb * yt) : ST_MAXKC;
}
constexpr int NPP_MAX_BLOCKS = 4 * 512 * 64;
constexpr size_t ST_MIN_CELLS = 512 * 1024;  // default form: streamed from this grid size
constexpr int ST_DEF_BX = 2, ST_DEF_WR = 8, ST_DEF_WC = 1;  // default streaming tile (float32)
static_assert(ST_PF >= 1 && ST_PF < FL, "prefetch ring has 7 slots");

struct StreamGrid {  // tiles along x, y and theta chunks; layers per chunk
    int gx, gy, gz, KC;
};


// Window loads.  Plain loads: hipcc counts them and places the waits.  (An
// earlier inline-asm form with hand-placed vmcnt waits is unsafe: hipcc treats an
// asm load's destination as written at the statement and may copy or reuse that
// register before the data lands.  It was the suspected cause of an illegal-address
// fault with two processes on one GPU; the plain form measures within 2%.)
template <typename T>
__device__ inline T st_load(const T* base, unsigned idx) {
    return base[idx];
}

// Excitation (posecell_network.py:336 -> convolution.py:228-246), inhibition
// (:339-340) and the normalisation partial sum (:343), streamed over layers.
template <typename T, int BX, int WR, int WC>
__global__ __launch_bounds__(64 * WR * WC) PC_ST_WAVES void pc_excite_stream(const T* __restrict__ P, T* __restrict__ Q,
                                                           double* __restrict__ part,
                                                           unsigned long long* __restrict__ res_slot,
                                                           int X, int Y, int TH, StreamGrid G,
                                                           SepKernel<T> k) {
    constexpr int NW = WR * WC, NT = 64 * NW, YT = 64 * WC, BXB = BX * WR;
    constexpr int HR = BXB + 2 * HALF, RW = YT + 2 * HALF, WN = HR * RW;
    constexpr int LPT = (WN + NT - 1) / NT;
    __shared__ T s_in[2][LPT * NT];  // padded: every thread stores every stage
    __shared__ T s_ye[2][HR * YT];
    __shared__ T s_yi[2][HR * YT];
    __shared__ T s_out[st_maxkc(sizeof(T), BXB, YT) * BXB * YT];
    __shared__ double s_red[NW];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int rg = wave % WR, col = (wave / WR) * 64 + lane;
    const int tile = st_tile(blockIdx.x, gridDim.x);
    const int bx = tile % G.gx, rest = tile / G.gx;
    const int i0 = bx * BXB, y0 = (rest % G.gy) * YT, k0 = (rest / G.gy) * G.KC;
    const int nL = min(G.KC, TH - k0) + 2 * HALF;
    const int gy = y0 + col;
    PC_STAMP(2, 0);
    if (res_slot != nullptr && blockIdx.x == 0)
        for (int i = tid; i < RES_SLOTS; i += blockDim.x) st_wt(&res_slot[i], 0ull);  // this step's path kernel max-reduces into them

    // window element e = (row r, col c) <-> P[L][(i0-3+r) % X][(y0-3+c) % Y]: the
    // in-layer offset is fixed over layers
    unsigned off[LPT];
#pragma unroll
    for (int u = 0; u < LPT; ++u) {
        const int e = min(tid + u * NT, WN - 1), r = e / RW, c = e - r * RW;
        off[u] = (unsigned)(rs::wrapi(i0 - HALF + r, X) * Y + rs::wrapi(y0 - HALF + c, Y));
    }
    const size_t lstride = (size_t)X * Y;
    T pre[FL][LPT];
#pragma unroll
    for (int d = 0; d < ST_PF; ++d) {
        const T* src = P + (size_t)rs::wrapi(k0 - HALF + d, TH) * lstride;
#pragma unroll
        for (int u = 0; u < LPT; ++u) pre[d][u] = st_load(src, off[u]);
    }

    T re[FL][BX], ri[FL][BX];
    double sum = 0.0;
    // software-pipelined over layers, one barrier per iteration: iteration it
    // stores window it+1, runs the y pass of layer it and the x / theta passes of
    // layer it-1 (its y pass landed before the previous barrier)
#pragma unroll
    for (int u = 0; u < LPT; ++u) s_in[0][tid + u * NT] = pre[0][u];
    {
        const T* src = P + (size_t)rs::wrapi(k0 - HALF + ST_PF, TH) * lstride;
#pragma unroll
        for (int u = 0; u < LPT; ++u) pre[ST_PF % FL][u] = st_load(src, off[u]);
    }
    __syncthreads();
    PC_STAMP(2, 1);
    for (int base = 0; base <= nL; base += FL) {
#pragma unroll
        for (int s = 0; s < FL; ++s) {
            const int it = base + s;
            if (it > nL) break;
            if (it < nL) {
                const int b = it & 1;
                // window it+1 (layers past the chunk are valid wrapped addresses: every
                // load is issued, so the counted waits stay in step)
#pragma unroll
                for (int u = 0; u < LPT; ++u) s_in[b ^ 1][tid + u * NT] = pre[(s + 1) % FL][u];
                {
                    const T* src = P + (size_t)rs::wrapi(k0 - HALF + it + 1 + ST_PF, TH) * lstride;
#pragma unroll
                    for (int u = 0; u < LPT; ++u) pre[(s + 1 + ST_PF) % FL][u] = st_load(src, off[u]);
                }
                // y pass of layer it: window rows rg, rg + WR, ... (both Gaussians share the loads)
                for (int r = rg; r < HR; r += WR) {
                    const T* rw = &s_in[b][r * RW + col];
                    T e = 0, g = 0;
#pragma unroll
                    for (int t = 0; t < FL; ++t) {
                        const T x = rw[t];
                        e += k.ge[t] * x;
                        g += k.gi[t] * x;
                    }
                    s_ye[b][r * YT + col] = e;
                    s_yi[b][r * YT + col] = g;
                }
            }
            if (it >= 1) {
                // x pass of layer it-1 (ring slot (s+6) % 7): this wave's BX rows,
                // register-blocked over the BX + 6 window rows
                const int b = (it - 1) & 1;
                T ye[BX + 2 * HALF], yi[BX + 2 * HALF];
#pragma unroll
                for (int a = 0; a < BX + 2 * HALF; ++a) {
                    ye[a] = s_ye[b][(rg * BX + a) * YT + col];
                    yi[a] = s_yi[b][(rg * BX + a) * YT + col];
                }
#pragma unroll
                for (int i = 0; i < BX; ++i) {
                    T e = 0, g = 0;
#pragma unroll
                    for (int t = 0; t < FL; ++t) {
                        e += k.ge[t] * ye[i + t];
                        g += k.gi[t] * yi[i + t];
                    }
                    re[(s + 6) % FL][i] = e;
                    ri[(s + 6) % FL][i] = g;
                }
                // theta pass for output layer o = it-7 over the ring (input o+t sits in
                // slot (s+t) % 7), relu(v - inhib), partial sum; the output waits in LDS
                if (it >= 2 * HALF + 1) {
                    const int o = it - 2 * HALF - 1;
#pragma unroll
                    for (int i = 0; i < BX; ++i) {
                        T e = 0, g = 0;
#pragma unroll
                        for (int t = 0; t < FL; ++t) {
                            e += k.ge[t] * re[(s + t) % FL][i];
                            g += k.gi[t] * ri[(s + t) % FL][i];
                        }
                        const T v = (e - g) * k.scale;
                        const T q = (v < k.inhib) ? T(0) : v - k.inhib;
                        s_out[(o * BXB + rg * BX + i) * YT + col] = q;
                        if (i0 + rg * BX + i < X && gy < Y) sum += (double)q;
                    }
                }
            }
            __syncthreads();
            if (it == 0) PC_STAMP(2, 2);
        }
    }
    PC_STAMP(2, 3);
    // write-back: each thread stores the cells it computed (its own LDS slots)
    for (int o = 0; o < nL - 2 * HALF; ++o)
#pragma unroll
        for (int i = 0; i < BX; ++i) {
            const int gi = i0 + rg * BX + i;
            if (gi < X && gy < Y)
                Q[((size_t)(k0 + o) * X + gi) * Y + gy] = s_out[(o * BXB + rg * BX + i) * YT + col];
        }
    sum = block_sum_w<NW>(sum, s_red);
    if (tid == 0) st_wt(&part[blockIdx.x], sum);
    PC_STAMP(2, 4);
}

// Path integration (posecell_network.py:252-314): per-layer shifted 7x7 filter
// (:273 -> convolution.py:320-340), clamp (:300), 7-tap theta filter (:310 ->
// convolution.py:344-359), clamp (:314), normalisation by the excitation total
// (:343-345, applied at the end), fused argmax (:317-319), streamed over layers.
template <typename T, int BX, int WR, int WC, typename CTL>
__global__ __launch_bounds__(64 * WR * WC) PC_ST_WAVES void pc_path_stream(
    const T* __restrict__ Q, T* __restrict__ P, const double* __restrict__ part, int npart,
    const T* __restrict__ filt, int nf, CTL ctl, unsigned long long* __restrict__ res_slot,
    T* __restrict__ bmax, unsigned* __restrict__ bidx, int X, int Y, int TH, StreamGrid G) {
    constexpr int NW = WR * WC, NT = 64 * NW, YT = 64 * WC, BXB = BX * WR;
    constexpr int HR = BXB + 2 * HALF, RW = YT + 2 * HALF, WN = HR * RW;
    constexpr int LPT = (WN + NT - 1) / NT;
    constexpr int NPP = 4;  // normalisation partials per thread (npart <= NPP * NT)
    __shared__ T s_win[2][LPT * NT];  // padded: every thread stores every stage
    __shared__ T s_out[st_maxkc(sizeof(T), BXB, YT) * BXB * YT];
    __shared__ __attribute__((aligned(16))) T s_ftab[RT_NFMAX * ST_FTP];
    __shared__ int s_ox[ST_MAXL], s_oy[ST_MAXL], s_fo[ST_MAXL];
    __shared__ double s_red[NW];
    __shared__ T s_bv[NW];
    __shared__ unsigned s_bl[NW];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int rg = wave % WR, col = (wave / WR) * 64 + lane;
    const int tile = st_tile(blockIdx.x, gridDim.x);
    const int bx = tile % G.gx, rest = tile / G.gx;
    const int i0 = bx * BXB, y0 = (rest % G.gy) * YT, k0 = (rest / G.gy) * G.KC;
    const int nL = min(G.KC, TH - k0) + 2 * HALF;
    const int gy = y0 + col;
    const size_t lstride = (size_t)X * Y;
    PC_STAMP(3, 0);

    // stage the block's control and the filter table; issue the normalisation
    // partials' loads (reduced after the first windows are in flight)
    if (tid < nL + ST_PF + 1) {  // + the prefetches issued past the chunk
        const int L = rs::wrapi(k0 - HALF + tid, TH);
        s_ox[tid] = rs::wrapi(ctl_ox(ctl, L), X);   // shifts may exceed the grid (vtrans large)
        s_oy[tid] = rs::wrapi(ctl_oy(ctl, L), Y);
        s_fo[tid] = ctl_fi(ctl, L) * ST_FTP;
    }
    for (int i = tid; i < nf * FT; i += NT) {
        const int fi = i / FT;
        s_ftab[fi * ST_FTP + (i - fi * FT)] = filt[i];
    }
    double pt[NPP];
#pragma unroll
    for (int u = 0; u < NPP; ++u) {
        const int i = tid + u * NT;
        pt[u] = part[min(i, npart - 1)];  // unconditional (a guarded load got its wait hoisted)
    }
    double pextra = 0.0;
    for (int i = tid + NPP * NT; i < npart; i += NT) pextra += part[i];
    T zf[FL];
#pragma unroll
    for (int z = 0; z < FL; ++z) zf[z] = (T)ctl_zf(ctl, z);
    __syncthreads();

    // window element e = (row r, col c) <-> Q[L][(i0-3+r+ox[L]) % X][(y0-3+c+oy[L]) % Y]
    // unshifted window coordinates, wrapped once: (a + o) % n == (a % n + o) % n with
    // o in [0, n), so a shifted coordinate needs one conditional subtraction
    int er[LPT], ec[LPT];
#pragma unroll
    for (int u = 0; u < LPT; ++u) {
        const int e = min(tid + u * NT, WN - 1), r = e / RW;
        er[u] = rs::wrapi(i0 - HALF + r, X);
        ec[u] = rs::wrapi(y0 - HALF + (e - r * RW), Y);
    }
    T pre[FL][LPT];
    auto load = [&](int it, T(&dst)[LPT]) {
        const int ox = s_ox[it], oy = s_oy[it];
        const T* src = Q + (size_t)rs::wrapi(k0 - HALF + it, TH) * lstride;
#pragma unroll
        for (int u = 0; u < LPT; ++u) {
            int gx = er[u] + ox, gc = ec[u] + oy;
            gx -= gx >= X ? X : 0;
            gc -= gc >= Y ? Y : 0;
            dst[u] = st_load(src, (unsigned)(gx * Y + gc));
        }
    };
#pragma unroll
    for (int d = 0; d < ST_PF; ++d) load(d, pre[d]);
    double tot = pextra;
#pragma unroll
    for (int u = 0; u < NPP; ++u) tot += tid + u * NT < npart ? pt[u] : 0.0;
    tot = block_sum_w<NW>(tot, s_red);
    const PcNorm<T> nrm(tot);

    T ring[FL][BX];
    T bv = -std::numeric_limits<T>::infinity();
    unsigned bl = 0xFFFFFFFFu;
    // software-pipelined: iteration it stores window it+1 while filtering window it;
    // one barrier per iteration
#pragma unroll
    for (int u = 0; u < LPT; ++u) s_win[0][tid + u * NT] = pre[0][u];
    load(ST_PF, pre[ST_PF % FL]);
    __syncthreads();
    PC_STAMP(3, 1);
    for (int base = 0; base < nL; base += FL) {
#pragma unroll
        for (int s = 0; s < FL; ++s) {
            const int it = base + s;
            if (it >= nL) break;
            const int b = it & 1;
            // window it+1 (every load is issued, past the chunk too, so the vmcnt
            // count always holds: see pc_excite_stream)
#pragma unroll
            for (int u = 0; u < LPT; ++u) s_win[b ^ 1][tid + u * NT] = pre[(s + 1) % FL][u];
            load(it + 1 + ST_PF, pre[(s + 1 + ST_PF) % FL]);
            if (it == 0) PC_STAMP(3, 2);
            T f[FT];
            st_filter<T>(s_ftab + s_fo[it], f);
            T acc[BX];
#pragma unroll
            for (int i = 0; i < BX; ++i) acc[i] = 0;
#pragma unroll
            for (int a = 0; a < BX + 2 * HALF; ++a) {
                T w[FL];
                const T* rw = &s_win[b][(rg * BX + a) * RW + col];
#pragma unroll
                for (int t = 0; t < FL; ++t) w[t] = rw[t];
#pragma unroll
                for (int i = 0; i < BX; ++i) {
                    const int x = a - i;
                    if (x < 0 || x >= FL) continue;
#pragma unroll
                    for (int t = 0; t < FL; ++t) acc[i] += w[t] * f[x * FL + t];
                }
            }
#pragma unroll
            for (int i = 0; i < BX; ++i) ring[s][i] = pc_clamp(acc[i]);
            if (it >= 2 * HALF) {
                const int o = it - 2 * HALF, gk = k0 + o;
#pragma unroll
                for (int i = 0; i < BX; ++i) {
                    T v = 0;
#pragma unroll
                    for (int z = 0; z < FL; ++z) v += ring[(s + 1 + z) % FL][i] * zf[z];
                    v = pc_clamp(v);
                    v = nrm(v);
                    s_out[(o * BXB + rg * BX + i) * YT + col] = v;
                    const int gi = i0 + rg * BX + i;
                    const unsigned lin = ((unsigned)gi * Y + gy) * TH + gk;
                    if (gi < X && gy < Y && pc_better(v, lin, bv, bl)) {
                        bv = v;
                        bl = lin;
                    }
                }
            }
            __syncthreads();
        }
    }
    PC_STAMP(3, 3);
    // write-back: each thread stores the cells it computed (its own LDS slots)
    for (int o = 0; o < nL - 2 * HALF; ++o)
#pragma unroll
        for (int i = 0; i < BX; ++i) {
            const int gi = i0 + rg * BX + i;
            if (gi < X && gy < Y)
                P[((size_t)(k0 + o) * X + gi) * Y + gy] = s_out[(o * BXB + rg * BX + i) * YT + col];
        }
    const PcBest<T> best = pc_block_best<NW>(bv, bl, s_bv, s_bl, wave, [] { __syncthreads(); });
    if (tid == 0) {
        if constexpr (sizeof(T) == 4) {
            atomicMax(res_slot + (blockIdx.x & (RES_SLOTS - 1)), argmax_key((float)best.v, best.l));
        } else {
            bmax[blockIdx.x] = best.v;
            bidx[blockIdx.x] = best.l;
        }
    }
    PC_STAMP(3, 4);
}

}  // namespace
