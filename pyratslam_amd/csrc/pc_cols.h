// cols   : pc_excite_cols + pc_path_cols, a block owns an 8 x 8 tile through all layers
//          (or a theta chunk); large grids
// Part of posecell.hip, the one translation unit: not free-standing (it relies on the
// includes and on the headers that posecell.hip includes before it).

namespace {

// ---------------------------------------------------------------------------
// Column forms (large grids).  A block of CO_NW waves owns a TX x TY tile of
// cells through ALL TH layers, so neither theta pass needs halo layers and no
// layer waits on another: the block loads its whole (TX+6) x (TY+6) x TH window
// at once (every load in flight together, one global round trip), then runs each
// pass over all layers in parallel with one barrier between passes.  The xy halo
// is re-read by neighbouring tiles ((TX+6)(TY+6) / (TX*TY) loads per cell) and
// the y pass runs over the TX+6 window rows; the theta passes are not repeated.
// The stream form's walk over KC+6 layers in sequence (one barrier and one LDS
// round trip chain per layer) is what bounds it at 128x128x72; here a block has
// four phases whatever TH is.  Tiles are numbered XCD-aware (st_tile).
// Window rows/cols wrap with one conditional add/subtract, so X >= TX+6 and
// Y >= TY+6 (checked on the host); TH <= co_thmax (the window in LDS).
// ---------------------------------------------------------------------------
// 12 waves per block (768 threads; 9, 10, 11, 13, 14, 16: 20.6, 20.3, 20.2, 20.5,
// 20.3, 20.2 us vs 19.8 per 128x128x72 step)
constexpr int CO_NW = 12;  // (the tile, CO_TX x CO_TY: pc_ctl.h)
// float64 whole-extent blocks: 8 waves (2 per SIMD), so the path kernel's 7x7 filter
// taps and its window loads fit the 256 VGPRs per wave without spilling
template <typename T>
__host__ __device__ constexpr int co_nw() { return sizeof(T) == 4 ? CO_NW : 8; }
// 7x7 filter tasks of the path kernel: 2 tasks per output column (4-row halves),
// 2 output columns per task, window rows scheduled 2 at a time
constexpr int CO_FSPLIT = 2, CO_FCOLS = 2, CO_FROWS = 2;
constexpr int CO_CH = 8;                        // layers per theta-pass task (scalar stream/rows helpers)
constexpr int CO_LDS = 150 * 1024;              // LDS budget of the excitation kernel
// Window rows are loaded as 16-byte vectors of VEC = 16 / sizeof(T) cells from a
// VEC-aligned start (Y % VEC == 0, so a vector never straddles the wrap): a row of
// HY cells starting d = start % VEC cells into its first vector takes
// ceil((HY + d) / VEC) vectors.  The excitation window starts at y0 - 3 with y0 a
// multiple of 8 (d = VEC - 3 % VEC); the path windows are shifted per layer (any d).
template <typename T>
__host__ __device__ constexpr int co_vec() { return 16 / (int)sizeof(T); }
template <typename T, bool SHIFTED>
__host__ __device__ constexpr int co_ncp() {  // vectors per window row
    return (CO_TY + 2 * HALF + (SHIFTED ? co_vec<T>() - 1 : (co_vec<T>() - HALF % co_vec<T>()) % co_vec<T>()) +
            co_vec<T>() - 1) / co_vec<T>();
}
// Layers of LDS window per block: the whole theta extent in one block per CU
// (co_thmax), or a theta chunk plus its 6 halo layers with two blocks per CU
// (co_thmax_chunk).  The excitation kernel's window + y-pass outputs set the size.
template <typename T>
__host__ __device__ constexpr int co_layer_bytes(bool padded) {
    return ((CO_TX + 2 * HALF) * (co_ncp<T, false>() + (padded ? 1 : 0)) * co_vec<T>() +
            2 * (CO_TX + 2 * HALF) * CO_TY) * (int)sizeof(T);
}
template <typename T>
__host__ __device__ constexpr int co_thmax() { return CO_LDS / co_layer_bytes<T>(true); }
constexpr int CO_LDS_CHUNK = 76 * 1024;   // two blocks per CU
constexpr int CO_NW_CHUNK = 8;            // 16 waves per CU: the path kernel's VGPRs allow 4 per SIMD
template <typename T>
__host__ __device__ constexpr int co_thmax_chunk() { return CO_LDS_CHUNK / co_layer_bytes<T>(false); }

// Layers of one column block: nl = nout + 2*halo window layers, local layer L
// holding global layer k0 - halo + L (wrapped); CHUNK: the block holds a theta
// chunk (halo 3), else the whole periodic extent (k0 = 0, nout = TH, halo 0).
template <bool CHUNK>
struct CoLayers {
    int k0, nout, nl;
    __device__ inline int global(int L, int TH) const { return CHUNK ? co_wrap(k0 - HALF + L, TH) : L; }
    // local layer of theta tap a (0..13) for the outputs of chunk j (8 per task)
    __device__ inline int tap(int j, int a, int TH) const {
        return CHUNK ? min(j * 8 + a, nl - 1) : co_wrap(j * 8 - HALF + a, TH);
    }
    // the same for chunks of cl output layers
    __device__ inline int tapc(int j, int a, int cl, int TH) const {
        return CHUNK ? min(j * cl + a, nl - 1) : co_wrap(j * cl - HALF + a, TH);
    }
};

template <bool CHUNK>
__device__ inline CoLayers<CHUNK> co_layers(int ch, int KC, int TH) {
    CoLayers<CHUNK> c;
    c.k0 = CHUNK ? ch * KC : 0;
    c.nout = CHUNK ? min(KC, TH - c.k0) : TH;
    c.nl = c.nout + (CHUNK ? 2 * HALF : 0);
    return c;
}

// Excitation (posecell_network.py:336 -> convolution.py:228-246), inhibition
// (:339-340) and the normalisation partial sum (:343) for one column tile.
// FIX_TH > 0: the instance for TH == FIX_TH (the x-pass output rows then have pitch
// TH + 64: a cell's row starts TH dwords modulo the 64 banks after the previous one, as
// if the rows were contiguous, so the theta pass's 16-byte reads of consecutive groups
// of consecutive cells are conflict-free)
template <typename T, int TX, int TY, int NW, int THM, bool CHUNK, int FIX_TH = 0>
__global__ __launch_bounds__(64 * NW) void pc_excite_cols(const T* __restrict__ P, int X, int Y, int TH,
                                                          int gx, int gy, int nblk, T* __restrict__ Q,
                                                          double* __restrict__ part,
                                                          unsigned long long* __restrict__ res_slot, int KC,
                                                          SepKernel<T> k) {
    constexpr int NT = 64 * NW, HX = TX + 2 * HALF, HY = TY + 2 * HALF;
    constexpr int VEC = co_vec<T>();
    static_assert(TY % VEC == 0, "row vectors");
    static_assert(FIX_TH == 0 || (FIX_TH == THM && !CHUNK && FIX_TH % 4 == 0), "fixed-extent instance");
    constexpr int SPO = 4, PP = FIX_TH ? FIX_TH + 64 : (THM + 12 + 3) / 4 * 4;
    __shared__ __attribute__((aligned(16))) T s_in[2 * TX * TY * PP];  // x-pass outputs (e, i)
    __shared__ __attribute__((aligned(16))) T s_ye[THM * HX * TY];  // [r][c][L]
    __shared__ __attribute__((aligned(16))) T s_yi[THM * HX * TY];
    __shared__ double s_red[NW];
    using V = typename CoVec<T>::type;
    const int tid = threadIdx.x;
    const int tile = st_tile(blockIdx.x, nblk), xy = tile % (gx * gy);
    const int x0 = (xy % gx) * TX, y0 = (xy / gx) * TY;
    const CoLayers<CHUNK> ly = co_layers<CHUNK>(tile / (gx * gy), KC, TH);
    // the fixed-extent instance's layer count is compile-time (no division per task)
    const int nlc = FIX_TH > 0 ? FIX_TH : ly.nl;
    if (res_slot != nullptr && blockIdx.x == 0)
        for (int i = tid; i < RES_SLOTS; i += blockDim.x) st_wt(&res_slot[i], 0ull);  // this step's path kernel max-reduces into them
    // the taps and constants in scalar registers for the whole kernel (float32): hipcc
    // otherwise reloads them from the kernel arguments after each barrier, a scalar
    // round trip at the head of the x and theta passes
    if constexpr (sizeof(T) == 4) {
#pragma unroll
        for (int q = 0; q < FL; ++q) asm volatile("" : "+s"(k.ge[q]), "+s"(k.gi[q]));
        asm volatile("" : "+s"(k.scale), "+s"(k.inhib));
    }
    PC_STAMP(5, 0);
    // y pass straight from the loads.  P is theta-fastest on this form (cell (x, y)
    // holds its TH layers contiguously), so task (r, L) = window row r of layer L
    // puts consecutive lanes on consecutive layers: each load instruction reads
    // consecutive words of one cell's theta column (whole 128-byte lines, where the
    // layer-major rows of 14 cells used a third of each line they touched).  Every
    // row of the block is in flight at once; the window never visits LDS; the y-pass
    // outputs go to LDS as [r][c][L].
    if constexpr (FIX_TH > 0) {
        // the fixed-extent instance: 16-byte loads of 4 consecutive layers of a cell
        // (a quarter of the load instructions), task (row r, layer group g): the row's
        // 14 window cells, 8 outputs x 4 layers, each output one 16-byte LDS store;
        // 14 x TH/4 tasks (252 at TH = 72: 4 waves).  (Half rows on 8 waves loaded 20
        // cells a row, 80 KiB a block through the load path instead of 56: 14.53 ->
        // 14.42 us per 128 x 128 x 72 step, tools/pc_ab.py, round 6)
        constexpr int NG = FIX_TH / 4, TH2 = TY, HW = TH2 + 2 * HALF;
        static_assert(HX * NG <= NT, "one task per thread");
        const int t = tid;
        if (t < HX * NG) {
            const int r = t / NG, h = 0, g = t - r * NG;
            const T* rowp = P + ((size_t)co_wrap(x0 - HALF + r, X) * Y) * FIX_TH + 4 * g;
            V w[HW];
#pragma unroll
            for (int c = 0; c < HW; ++c)
                w[c] = *reinterpret_cast<const V*>(rowp + (size_t)co_wrap(y0 - HALF + h * TH2 + c, Y) * FIX_TH);
#pragma unroll
            for (int c = 0; c < TH2; ++c) {
                V e = {0, 0, 0, 0}, gg = {0, 0, 0, 0};
#pragma unroll
                for (int q = 0; q < FL; ++q) {
                    e += k.ge[q] * w[c + q];
                    gg += k.gi[q] * w[c + q];
                }
                const int o = (r * TY + h * TH2 + c) * THM + 4 * g;
                *reinterpret_cast<V*>(s_ye + o) = e;
                *reinterpret_cast<V*>(s_yi + o) = gg;
            }
        }
    } else {
        constexpr int NR = (THM * HX + NT - 1) / NT;
        const int nrow = ly.nl * HX;
        T w[NR][HY];
#pragma unroll
        for (int u = 0; u < NR; ++u) {
            const int t = min(tid + u * NT, nrow - 1), r = t / ly.nl, L = t - r * ly.nl;
            const T* cell = P + ((size_t)co_wrap(x0 - HALF + r, X) * Y) * TH + ly.global(L, TH);
#pragma unroll
            for (int c = 0; c < HY; ++c) w[u][c] = cell[(size_t)co_wrap(y0 - HALF + c, Y) * TH];
        }
#pragma unroll
        for (int u = 0; u < NR; ++u) {
            const int t = tid + u * NT;
            if (t >= nrow) break;
            const int r = t / ly.nl, L = t - r * ly.nl;
#pragma unroll
            for (int c = 0; c < TY; ++c) {
                T e = 0, g = 0;
#pragma unroll
                for (int q = 0; q < FL; ++q) {
                    e += k.ge[q] * w[u][c + q];
                    g += k.gi[q] * w[u][c + q];
                }
                s_ye[(r * TY + c) * THM + L] = e;   // [r][c][L]: consecutive lanes, consecutive words
                s_yi[(r * TY + c) * THM + L] = g;
            }
        }
    }
    PC_STAMP(5, 1);
    co_lds_barrier();
    PC_STAMP(5, 2);
    // x pass: task (L, c) -> a column of TX outputs from HX y-pass rows, written as
    // [cell p][SPO + L] rows of pitch PP (16-byte aligned: the theta pass reads
    // them as vectors; consecutive lanes take consecutive layers, so the writes are
    // conflict-free).  The whole-extent form also writes each output's wrapped copy
    // (layers TH-4..TH-1 before SPO, 0..7 after SPO + TH), so every theta window is
    // one contiguous aligned run with no extra pass.
    T* s_xe = s_in;
    T* s_xi = s_in + TX * TY * PP;
    // one task: outputs i0 .. i0 + R - 1 of column c, layer L
    auto xtask = [&](int c, int L, int i0, auto r_c) __attribute__((always_inline)) {
        constexpr int R = decltype(r_c)::value;
        T ye[R + 2 * HALF], yi[R + 2 * HALF];
#pragma unroll
        for (int a = 0; a < R + 2 * HALF; ++a) {
            ye[a] = s_ye[((i0 + a) * TY + c) * THM + L];
            yi[a] = s_yi[((i0 + a) * TY + c) * THM + L];
        }
        // wrapped copies (TH >= 10, so at most one of each)
        const int Lw1 = !CHUNK && L < 8 ? nlc + L : INT_MIN, Lw2 = !CHUNK && L >= nlc - 4 ? L - nlc : INT_MIN;
#pragma unroll
        for (int i = 0; i < R; ++i) {
            T e = 0, g = 0;
#pragma unroll
            for (int q = 0; q < FL; ++q) {
                e += k.ge[q] * ye[i + q];
                g += k.gi[q] * yi[i + q];
            }
            const int r = ((i0 + i) * TY + c) * PP + SPO;
            s_xe[r + L] = e;
            s_xi[r + L] = g;
            if (Lw1 != INT_MIN) {
                s_xe[r + Lw1] = e;
                s_xi[r + Lw1] = g;
            }
            if (Lw2 != INT_MIN) {
                s_xe[r + Lw2] = e;
                s_xi[r + Lw2] = g;
            }
        }
    };
    if constexpr (FIX_TH == 72 && TX == 8 && TY == 8 && NW == 12) {
        // the 72-layer instance balances the four SIMDs (wave w runs on SIMD w % 4):
        // waves 0-7 take layers 0-63 (lane = layer) of column w, waves 8-11 layers 64-71
        // (64 + (lane & 7)) of column lane >> 3, two of the eight outputs each; 576 equal
        // tasks on 9 waves put three on SIMD 0
        const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
        if (wave < 8) xtask(wave, lane, 0, std::integral_constant<int, TX>{});
        else xtask(lane >> 3, 64 + (lane & 7), 2 * (wave - 8), std::integral_constant<int, 2>{});
    } else {
        for (int t = tid; t < nlc * TY; t += NT) {
            const int c = t / nlc, L = t - c * nlc;
            xtask(c, L, 0, std::integral_constant<int, TX>{});
        }
    }
    co_lds_barrier();
    PC_STAMP(5, 3);
    // theta pass: task (cell p, group j of VEC layers), consecutive lanes on
    // consecutive groups of one cell: the outputs of a group are one 16-byte
    // write-through store into Q, which is theta-fastest like P (the path kernel
    // then loads whole runs of each cell's layers)
    double sum = 0.0;
    {
        const int ng = FIX_TH > 0 ? FIX_TH / VEC : (ly.nout + VEC - 1) / VEC;
        const int nbytes = (int)min((size_t)X * Y * TH * sizeof(T), (size_t)INT_MAX);
        const bool wt = (size_t)X * Y * TH * sizeof(T) <= (size_t)INT_MAX;
        constexpr int ROFF = CHUNK ? 0 : 1, NRV = (ROFF + VEC + 2 * HALF + VEC - 1) / VEC;
#pragma unroll 1
        for (int t = tid; t < TX * TY * ng; t += NT) {
            const int p = t / ng, j = t - p * ng, i = p / TY;
            const int gi = x0 + i, gy = y0 + p - i * TY;
            // taps of output lo = j * VEC + o: local layers lo - 3 .. lo + 3 (whole
            // extent, from the aligned run starting at lo - 4) or lo .. lo + 6 (a chunk's
            // local layer lo + 3 is its output lo)
            const V* se = reinterpret_cast<const V*>(s_xe + p * PP + SPO + j * VEC - (CHUNK ? 0 : 4));
            const V* si = reinterpret_cast<const V*>(s_xi + p * PP + SPO + j * VEC - (CHUNK ? 0 : 4));
            T re[NRV * VEC], ri[NRV * VEC];
#pragma unroll
            for (int q = 0; q < NRV; ++q) {
                const V a = se[q], b = si[q];
#pragma unroll
                for (int c = 0; c < VEC; ++c) {
                    re[q * VEC + c] = a[c];
                    ri[q * VEC + c] = b[c];
                }
            }
            V qv;
#pragma unroll
            for (int o = 0; o < VEC; ++o) {
                T e = 0, g = 0;
#pragma unroll
                for (int z = 0; z < FL; ++z) {
                    e += k.ge[z] * re[ROFF + o + z];
                    g += k.gi[z] * ri[ROFF + o + z];
                }
                const T v = (e - g) * k.scale;
                qv[o] = (v < k.inhib) ? T(0) : v - k.inhib;
            }
            if (gi < X && gy < Y) {
                const int gk0 = ly.k0 + j * VEC, nv = min(VEC, ly.nout - j * VEC);
                const size_t e0 = ((size_t)gi * Y + gy) * TH + gk0;
                if (nv == VEC && e0 % VEC == 0) {
                    co_put(Q, e0, qv, wt, nbytes);
                } else {  // a ragged or unaligned group (TH or the chunk not a multiple of VEC)
#pragma unroll
                    for (int o = 0; o < VEC; ++o)
                        if (o < nv) Q[e0 + o] = qv[o];
                }
#pragma unroll
                for (int o = 0; o < VEC; ++o)
                    if (o < nv) sum += (double)qv[o];
            }
        }
    }
    sum = co_wave_sum(sum);
    if ((tid & 63) == 0) s_red[tid >> 6] = sum;
    co_lds_barrier();  // the Q stores drain meanwhile
    if (tid == 0) {
        double t = 0.0;
#pragma unroll
        for (int w = 0; w < NW; ++w) t += s_red[w];
        st_wt(&part[blockIdx.x], t);
    }
    PC_STAMP(5, 4);
}

// Path integration (posecell_network.py:252-314) for one column tile: per-layer
// shifted 7x7 filter (:273 -> convolution.py:320-340), clamp (:300), 7-tap theta
// filter (:310 -> convolution.py:344-359), clamp (:314), normalisation by the
// excitation total (:343-345, applied at the end), fused argmax (:317-319).
// Window buffer of the path kernel (bytes): the whole-extent form runs one block per
// CU, the theta-chunked form two.
constexpr int CO_WIN_BYTES = 128 * 1024, CO_WIN_BYTES_CHUNK = 56 * 1024;
// theta extent of the path kernel's LDS-DMA window instance (float32, whole extent,
// control as kernel arguments): BASELINE configs[3]'s 72 layers
constexpr int CO_DMA_TH = 72;

// wave min / max of an int by DPP row operations and readlanes (as co_wave_max)
template <bool MAX>
__device__ inline int co_wave_ext_i(int v) {
    auto op = [](int a, int b) { return MAX ? max(a, b) : min(a, b); };
    v = op(v, __builtin_amdgcn_update_dpp(v, v, 0xB1, 0xF, 0xF, false));
    v = op(v, __builtin_amdgcn_update_dpp(v, v, 0x4E, 0xF, 0xF, false));
    v = op(v, __builtin_amdgcn_update_dpp(v, v, 0x141, 0xF, 0xF, false));
    v = op(v, __builtin_amdgcn_update_dpp(v, v, 0x140, 0xF, 0xF, false));
    return op(op(__builtin_amdgcn_readlane(v, 0), __builtin_amdgcn_readlane(v, 16)),
              op(__builtin_amdgcn_readlane(v, 32), __builtin_amdgcn_readlane(v, 48)));
}

// DMA_TH > 0: the instance for TH == DMA_TH (float32, whole extent, control as kernel
// arguments).  Its window is an LDS image [u][v][layer] with no padding between a
// cell's layers, so each 16-byte piece of a cell's theta run in Q has a fixed place,
// and the pieces go global -> LDS by LDS-DMA (global_load_lds_dwordx4, lane-linear
// 1 KiB per wave-instruction): no register staging and no ds_write (the scalar
// stores into the odd-pitch image were 4-way bank conflicts), issued first thing from
// the host-formed union (PcCtlInline::umx..uwy), in flight together with the
// control's, the partials' and the filter table's loads: one round trip.
template <typename T, int TX, int TY, int NW, int THM, bool CHUNK, typename CTL, int DMA_TH = 0>
__global__ __launch_bounds__(64 * NW) void pc_path_cols(
    const T* __restrict__ Q, int X, int Y, int TH, int gx, int gy, int nblk, T* __restrict__ P,
    const double* __restrict__ part, int npart, const T* __restrict__ filt, int nf, CTL ctl,
    unsigned long long* __restrict__ res_slot, T* __restrict__ bmax, unsigned* __restrict__ bidx, int KC) {
    constexpr int NT = 64 * NW, VEC = co_vec<T>();
    constexpr bool DMA = DMA_TH > 0;
    // Q is theta-fastest, like P: the block loads the union of its layers' shifted
    // windows -- WX x WY cells, each cell's run of layers contiguous in Q -- into LDS
    // as [cell][layer] (every |shift| <= 3 at 128x128x72: 20 x 20 cells x 72 layers,
    // 115 KiB).  Consecutive lanes take consecutive layers: the loads read whole runs
    // of a cell's layers and the filter's LDS reads are conflict-free.  Shifts whose
    // union window does not fit take per-layer 14 x 14 windows instead.
    // (the DMA instance: windows of up to 20 x 20 cells, shifts spread over at most 6
    // cells, plus one wave-instruction of slack for the last pieces)
    constexpr int WBUF = DMA ? 20 * (TY + 2 * HALF + 6) * DMA_TH + 4 * 64
                             : (CHUNK ? CO_WIN_BYTES_CHUNK : CO_WIN_BYTES) / (int)sizeof(T);
    using V = typename CoVec<T>::type;
    __shared__ __attribute__((aligned(16))) T s_w[WBUF];
    // clamped 7x7 outputs [cell p][SPO + L], pitch PP (16-byte rows: the theta pass
    // reads VEC-aligned vectors); the whole-extent form also keeps wrapped copies of
    // the last 4 layers before SPO and of the first 8 after SPO + TH, so every theta
    // window is one contiguous aligned run
    // (the DMA instance: PP = TH + 64, so a cell's row starts TH dwords modulo the 64
    // banks after the previous one, as if the rows were contiguous: the theta pass's
    // 16-byte reads of consecutive groups of consecutive cells are conflict-free)
    constexpr int SPO = 4, PP = DMA ? DMA_TH + 64 : (THM + 12 + 3) / 4 * 4;
    __shared__ __attribute__((aligned(16))) T s_p[TX * TY * PP];
    __shared__ __attribute__((aligned(16))) T s_ftab[RT_NFMAX * ST_FTP];
    __shared__ int s_ox[THM], s_oy[THM], s_fo[THM];
    __shared__ T s_bv[NW];
    __shared__ unsigned s_bl[NW];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int tile = st_tile(blockIdx.x, nblk), xy = tile % (gx * gy);
    const int x0 = (xy % gx) * TX, y0 = (xy / gx) * TY;
    const CoLayers<CHUNK> ly = co_layers<CHUNK>(tile / (gx * gy), KC, TH);
    PC_STAMP(6, 0);
    // window strides are compile-time (the filter's LDS reads take immediate offsets):
    // WYP cells per window row, LPC layers per cell (odd: fewer bank conflicts between
    // lanes whose layers have different shifts; the DMA image: exactly TH), at most
    // WXP rows
    constexpr int WYP = TY + 2 * HALF + 6, LPC = DMA ? DMA_TH : (THM | 1), WXP = WBUF / (WYP * LPC);
    static_assert(WXP >= TX + 2 * HALF, "a per-layer window fits");
    bool dma = false;
    // the union's fields (DMA instance) in scalar registers for the whole kernel: hipcc
    // otherwise reloads them from the kernel arguments after the first barrier
    int cumx = 0, cumy = 0, cuwx = 0, cuwy = 0;
    if constexpr (DMA) {
        cumx = __builtin_amdgcn_readfirstlane((int)ctl.umx);
        cumy = __builtin_amdgcn_readfirstlane((int)ctl.umy);
        cuwx = __builtin_amdgcn_readfirstlane((int)ctl.uwx);
        cuwy = __builtin_amdgcn_readfirstlane((int)ctl.uwy);
        asm volatile("" : "+s"(cumx), "+s"(cumy), "+s"(cuwx), "+s"(cuwy));
    }
    if constexpr (DMA) {
        static_assert(sizeof(T) == 4 && !CHUNK && DMA_TH % 4 == 0 && DMA_TH <= THM, "DMA window form");
        constexpr int PPC = DMA_TH / 4;    // 16-byte pieces per cell
        static_assert(WXP * WYP * PPC + 63 <= WBUF / 4, "the last wave-instruction stays in the buffer");
        const int WX = cuwx, WY = cuwy;
        dma = TH == DMA_TH && WX <= WXP && WY <= WYP && WX <= X && WY <= Y;
        if (dma) {
            // piece p = (u * WYP + v) * PPC + l4 lands at s_w + 4p (the padding cells
            // v >= WY are not loaded); a thread's pieces advance by NT per instruction
            const int ux0 = co_wrap(x0 - HALF + cumx, X), uy0 = co_wrap(y0 - HALF + cumy, Y);
            const int npc = WX * WYP * PPC, wave_u = __builtin_amdgcn_readfirstlane(wave);
            constexpr int DC = NT / PPC, DL = NT % PPC, DU = DC / WYP, DV = DC % WYP;
            constexpr int NK = (WXP * WYP * PPC + NT - 1) / NT;
            const int p0 = wave_u * 64 + lane;
            int c = p0 / PPC, l4 = p0 - c * PPC, u = c / WYP, v = c - u * WYP;
#pragma unroll
            for (int k = 0; k < NK; ++k) {
                const int i0 = k * NT + wave_u * 64;  // wave-uniform
                if (i0 < npc) {
                    if (i0 + lane < npc && v < WY) {
                        int gr = ux0 + u, gc = uy0 + v;
                        gr -= gr >= X ? X : 0;
                        gc -= gc >= Y ? Y : 0;
                        __builtin_amdgcn_global_load_lds(
                            (__attribute__((address_space(1))) const void*)(Q + ((unsigned)gr * Y + gc) * DMA_TH + 4 * l4),
                            (__attribute__((address_space(3))) void*)(s_w + 4 * i0), 16, 0, 0);
                    }
                }
                l4 += DL;
                v += DV;
                u += DU;
                if (l4 >= PPC) {
                    l4 -= PPC;
                    ++v;
                }
                if (v >= WYP) {
                    v -= WYP;
                    ++u;
                }
            }
        }
    }
    // The control first (its loads are the ones the first barrier waits for; clamped
    // unconditional reads, in flight together), then the normalisation partials (a
    // guarded load had its wait hoisted to the kernel's start).  Every wave forms
    // the total itself: no block barrier between the window loads and their use.
    static_assert(THM <= NT, "one layer's control per thread");
    const int Lc = min(tid, ly.nl - 1), gLc = ly.global(Lc, TH);
    const int oxc = ctl_ox(ctl, gLc), oyc = ctl_oy(ctl, gLc), fic = ctl_fi(ctl, gLc);
    constexpr int NPL = 4;  // partials per lane loaded up front (npart <= 256 in one round)
    double pt[NPL];
#pragma unroll
    for (int u = 0; u < NPL; ++u) pt[u] = part[min(lane + 64 * u, npart - 1)];
    if (tid < ly.nl) {
        s_ox[tid] = co_centre(oxc, X);
        s_oy[tid] = co_centre(oyc, Y);
        s_fo[tid] = fic * ST_FTP;
    }
    constexpr int NFR = (RT_NFMAX * FT + NT - 1) / NT;
    T fr[NFR];
#pragma unroll
    for (int u = 0; u < NFR; ++u) fr[u] = tid + u * NT < nf * FT ? filt[tid + u * NT] : T(0);
    T zf[FL];
#pragma unroll
    for (int z = 0; z < FL; ++z) zf[z] = (T)ctl_zf(ctl, z);
    // the normalisation total (every wave forms it itself) and the filter table into
    // LDS before the first barrier, which waits for the control's loads anyway: the
    // window's loads then follow with nothing else to wait for
    // (the DMA instance forms it after the first barrier, in its last wave, which has no
    // filter task: the partials are the youngest loads of every wave, so forming the total
    // here waits for the whole window, and the DPP reduction and reciprocal sat between the
    // window's landing and the barrier)
    auto total = [&]() __attribute__((always_inline)) {
        double tot = 0.0;
#pragma unroll
        for (int u = 0; u < NPL; ++u) tot += lane + 64 * u < npart ? pt[u] : 0.0;
        for (int i = lane + 64 * NPL; i < npart; i += 64) tot += part[i];
        return co_wave_sum(tot);
    };
    // the normalisation (:343-345): PcNorm (float32: the product with the reciprocal)
    __shared__ float s_nrm[3];   // (the DMA instance: r, t, div of the total's PcNorm<float>)
    const PcNorm<T> nrm0(DMA ? 1.0 : total());
#pragma unroll
    for (int u = 0; u < NFR; ++u) {
        const int i = tid + u * NT, fi = i / FT;
        if (i < nf * FT) s_ftab[fi * ST_FTP + (i - fi * FT)] = fr[u];
    }
    // the DMA pieces have landed before any wave passes the barrier and reads them
    // (a wave's waitcnt covers its own LDS-DMA; the barrier, everyone's)
    if (DMA && dma) __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0)
    co_lds_barrier();
    PC_STAMP(6, 1);
    // the union window of the block's layers (every wave reduces the shifts itself;
    // the DMA form has it from the host)
    int mnx = INT_MAX, mxx = INT_MIN, mny = INT_MAX, mxy = INT_MIN;
    if (DMA && dma) {
        if constexpr (DMA) {
            mnx = cumx;
            mny = cumy;
            mxx = mnx + cuwx - (TX + 2 * HALF);
            mxy = mny + cuwy - (TY + 2 * HALF);
        }
    } else {
        for (int L = lane; L < ly.nl; L += 64) {
            mnx = min(mnx, s_ox[L]);
            mxx = max(mxx, s_ox[L]);
            mny = min(mny, s_oy[L]);
            mxy = max(mxy, s_oy[L]);
        }
        mnx = co_wave_ext_i<false>(mnx);
        mxx = co_wave_ext_i<true>(mxx);
        mny = co_wave_ext_i<false>(mny);
        mxy = co_wave_ext_i<true>(mxy);
    }
    const int WX = TX + 2 * HALF + mxx - mnx, WY = TY + 2 * HALF + mxy - mny;
    const bool uni = WX <= WXP && WY <= WYP && WX <= X && WY <= Y;
    const int ux0 = co_wrap(x0 - HALF + mnx, X), uy0 = co_wrap(y0 - HALF + mny, Y);

    constexpr int FS = CO_FSPLIT, TXH = TX / FS, CP = CO_FCOLS, NCG = TY / CP;
    static_assert(TX % FS == 0 && TY % CP == 0, "filter task shape");
    const int nl = DMA ? DMA_TH : ly.nl;   // (the DMA instance runs at TH == DMA_TH only: no division per task)
    if (DMA && dma) {
        // the window is in LDS already
    } else if (uni && !CHUNK && TH % VEC == 0) {
        // the common case: the union window (WX x WY cells) with 16-byte loads of VEC
        // consecutive layers of a cell, positions advanced incrementally (no
        // divisions per element); all of a thread's loads in flight together
        constexpr int NV = (WXP * WYP * LPC / VEC + NT - 1) / NT;
        // float64: two rounds of loads (all NV in flight spills the filter's registers)
        constexpr int NR = sizeof(T) == 4 ? 1 : 2, NVR = (NV + NR - 1) / NR;
        const int lcw = nl / VEC, nel = WX * WY * lcw;
        const int c = tid / lcw, dc = NT / lcw, dl = (NT - dc * lcw) * VEC;
        const int dcu = dc / WY, dcv = dc - dcu * WY;
        int cu = c / WY, cv = c - cu * WY, l = (tid - c * lcw) * VEC;   // load cursor
        int su = cu, sv = cv, sl = l;                                   // store cursor
        auto advance = [&](int& u_, int& v_, int& l_) __attribute__((always_inline)) {
            l_ += dl;
            v_ += dcv;
            u_ += dcu;
            if (l_ >= nl) {
                l_ -= nl;
                ++v_;
            }
            if (v_ >= WY) {
                v_ -= WY;
                ++u_;
            }
        };
#pragma unroll
        for (int r = 0; r < NR; ++r) {
            V w[NVR];
#pragma unroll
            for (int k = 0; k < NVR; ++k) {
                const int u = r * NVR + k;
                if (u < NV) {  // straight-line: a thread past the window re-reads element 0
                    int gr = ux0 + cu, gc = uy0 + cv;
                    gr -= gr >= X ? X : 0;
                    gc -= gc >= Y ? Y : 0;
                    const unsigned off = tid + u * NT < nel ? ((unsigned)gr * Y + gc) * TH + l
                                                            : ((unsigned)ux0 * Y + uy0) * TH;
                    w[k] = *reinterpret_cast<const V*>(Q + off);
                }
                advance(cu, cv, l);
            }
#pragma unroll
            for (int k = 0; k < NVR; ++k) {
                const int u = r * NVR + k;
                if (u < NV && tid + u * NT < nel) {
                    T* d = s_w + (su * WYP + sv) * LPC + sl;
#pragma unroll
                    for (int j = 0; j < VEC; ++j) d[j] = w[k][j];
                }
                advance(su, sv, sl);
            }
        }
    } else {
        // theta chunks (a window run may wrap around TH), ragged extents, and shifts
        // whose union window does not fit (each layer then takes its own 14 x 14
        // window): scalar elements, 8 loads in flight per thread
        const int wx = uni ? WX : TX + 2 * HALF, wy = uni ? WY : TY + 2 * HALF, nel = wx * wy * nl;
        for (int e0 = tid; e0 < nel; e0 += 8 * NT) {
            T w[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int e = e0 + u * NT;
                if (e < nel) {
                    const int c = e / nl, L = e - c * nl, cu = c / wy, cv = c - cu * wy;
                    const int bx = uni ? ux0 : co_wrap(x0 - HALF + s_ox[L], X);
                    const int by = uni ? uy0 : co_wrap(y0 - HALF + s_oy[L], Y);
                    w[u] = Q[((size_t)co_wrap(bx + cu, X) * Y + co_wrap(by + cv, Y)) * TH + ly.global(L, TH)];
                }
            }
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int e = e0 + u * NT;
                if (e < nel) {
                    const int c = e / nl, L = e - c * nl, cu = c / wy, cv = c - cu * wy;
                    s_w[(cu * WYP + cv) * LPC + L] = w[u];
                }
            }
        }
    }
    if (!(DMA && dma)) co_lds_barrier();
    PC_STAMP(6, 2);
    if constexpr (DMA) {
        static_assert(DMA_TH * NCG * FS <= 64 * (NW - 1), "the last wave has no filter task");
        if (wave == NW - 1) {
            const PcNorm<float> n1(total());
            if (lane == 0) {
                s_nrm[0] = n1.r;
                s_nrm[1] = n1.t;
                s_nrm[2] = n1.div ? 1.f : 0.f;
            }
        }
    }
    // 7x7 filter: task (layer, column group, row part) -> TX/FS rows x CP columns of
    // outputs from TX/FS + 6 window rows of CP + 6 cells (CP columns share each window
    // row's reads; reads of CO_FROWS rows at a time in flight: hoisting all of them
    // spills at 3 waves per SIMD).  Layer fastest over the lanes.
    // one task: R output rows from tile row x0r, CP columns from c0, of layer L
    auto ftask = [&](int L, int x0r, int c0, auto r_c) __attribute__((always_inline)) {
        constexpr int R = decltype(r_c)::value;
        T f[FT];
        st_filter<T>(s_ftab + s_fo[L], f);
        T acc[R][CP];
#pragma unroll
        for (int i = 0; i < R; ++i)
#pragma unroll
            for (int c = 0; c < CP; ++c) acc[i][c] = 0;
        const int dx = uni ? s_ox[L] - mnx : 0, dy = uni ? s_oy[L] - mny : 0;
        // the base index is opaque to the compiler, so each read keeps its compile-time
        // offset as an immediate (ds_read2_b32 pairs) instead of an address add each
        int wbase = ((x0r + dx) * WYP + c0 + dy) * LPC + L;
        asm volatile("" : "+v"(wbase));
        const T* win = s_w + wbase;
        // the window rows in a rotated order per wave group (waves w, w+4, w+8 share a
        // SIMD): the groups' LDS read bursts and FMA runs interleave instead of
        // running in lockstep behind the barrier
        auto rows = [&](auto rot_c) __attribute__((always_inline)) {
            constexpr int ROT = decltype(rot_c)::value, NRW = R + 2 * HALF;
#pragma unroll
            for (int aa = 0; aa < NRW; ++aa) {
                const int a = (aa + ROT) % NRW;
                T w[FL + CP - 1];
#pragma unroll
                for (int q = 0; q < FL + CP - 1; ++q) w[q] = win[(a * WYP + q) * LPC];
                if (aa % CO_FROWS == CO_FROWS - 1) __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int i = 0; i < R; ++i) {
                    const int x = a - i;
                    if (x < 0 || x >= FL) continue;
#pragma unroll
                    for (int c = 0; c < CP; ++c)
#pragma unroll
                        for (int q = 0; q < FL; ++q) acc[i][c] += w[c + q] * f[x * FL + q];
                }
            }
        };
        const int grp = __builtin_amdgcn_readfirstlane(tid >> 8);  // wave / 4
        if (grp == 0) rows(std::integral_constant<int, 0>{});
        else if (grp == 1) rows(std::integral_constant<int, 3>{});
        else rows(std::integral_constant<int, 6>{});
        // with the wrapped copies of the whole-extent form (layers TH-4..TH-1 also
        // before SPO, 0..7 also after SPO + TH; TH >= 10, so at most one of each)
        const int Lw1 = !CHUNK && L < 8 ? nl + L : INT_MIN, Lw2 = !CHUNK && L >= nl - 4 ? L - nl : INT_MIN;
#pragma unroll
        for (int i = 0; i < R; ++i)
#pragma unroll
            for (int c = 0; c < CP; ++c) {
                const T v = pc_clamp(acc[i][c]);
                T* sp = s_p + ((x0r + i) * TY + c0 + c) * PP + SPO;
                sp[L] = v;
                if (Lw1 != INT_MIN) sp[Lw1] = v;
                if (Lw2 != INT_MIN) sp[Lw2] = v;
            }
    };
    if constexpr (DMA) {
        // The DMA instance (72 layers, 8 x 8 tiles, 12 waves) balances the four SIMDs
        // (wave w runs on SIMD w % 4): waves 0-7 take layers 0-63 (lane = layer) in
        // 4-row x 2-column tasks, waves 8-11 layers 64-71 in 1-row x 2-column tasks
        // (layer 64 + (lane & 7), tile row lane >> 3).  Every SIMD issues 2 x 392 + 98
        // filter FMAs per lane, where 576 equal tasks on 9 waves put 3 x 392 on SIMD 0
        static_assert(TX == 8 && TY == 8 && CP == 2 && FS == 2 && NW == 12 && DMA_TH == 72, "DMA instance's task split");
        if (wave < 8) ftask(lane, (wave >> 2) * TXH, (wave & 3) * CP, std::integral_constant<int, TXH>{});
        else ftask(64 + (lane & 7), lane >> 3, (wave - 8) * CP, std::integral_constant<int, 1>{});
    } else {
        for (int t = tid; t < nl * NCG * FS; t += NT) {
            const int L = t % nl, rem = t / nl, hf = rem / NCG, c0 = (rem - hf * NCG) * CP;
            ftask(L, hf * TXH, c0, std::integral_constant<int, TXH>{});
        }
    }
    (void)VEC;
    co_lds_barrier();
    PC_STAMP(6, 3);
    PcNorm<T> nrm = nrm0;
    if constexpr (DMA)   // (div block-uniform: a scalar branch)
        nrm = PcNorm<T>(s_nrm[0], s_nrm[1], __builtin_amdgcn_readfirstlane((int)(s_nrm[2] != 0.f)) != 0);
    // theta pass, clamp, normalisation, argmax: task (cell p, chunk j).  float32:
    // the first maximum as the largest packed (value, ~index) key; float64: value
    // and index pairs
    T bv = -std::numeric_limits<T>::infinity();
    unsigned bl = 0xFFFFFFFFu;
    unsigned long long bk = 0ull;
    {
        // task (cell p, group j of VEC layers), consecutive lanes on consecutive groups
        // of one cell: P is theta-fastest on this form, so a group is one 16-byte
        // store and a wave's stores cover consecutive cells' theta columns
        using V = typename CoVec<T>::type;
        const int ng = DMA ? DMA_TH / VEC : (ly.nout + VEC - 1) / VEC;
        const int nbytes = (int)min((size_t)X * Y * TH * sizeof(T), (size_t)INT_MAX);
        const bool wt = (size_t)X * Y * TH * sizeof(T) <= (size_t)INT_MAX;
#pragma unroll 1
        for (int t = tid; t < TX * TY * ng; t += NT) {
            const int p = t / ng, j = t - p * ng, i = p / TY;
            const int gi = x0 + i, gy = y0 + p - i * TY;
            // taps of output lo = j * VEC + o: local layers lo - 3 .. lo + 3 (whole
            // extent, from the aligned run starting at lo - 4) or lo .. lo + 6 (a chunk's
            // local layer lo + 3 is its output lo)
            constexpr int ROFF = CHUNK ? 0 : 1, NRV = (ROFF + VEC + 2 * HALF + VEC - 1) / VEC;
            const V* sv = reinterpret_cast<const V*>(s_p + p * PP + SPO + j * VEC - (CHUNK ? 0 : 4));
            T rr[NRV * VEC];
#pragma unroll
            for (int q = 0; q < NRV; ++q) {
                const V x = sv[q];
#pragma unroll
                for (int c = 0; c < VEC; ++c) rr[q * VEC + c] = x[c];
            }
            const T* r = rr + ROFF;
            V v;
#pragma unroll
            for (int o = 0; o < VEC; ++o) {
                T x = 0;
#pragma unroll
                for (int z = 0; z < FL; ++z) x += r[o + z] * zf[z];
                x = pc_clamp(x);
                x = nrm(x);
                v[o] = x;
            }
            if (gi < X && gy < Y) {
                const int gk0 = ly.k0 + j * VEC, nv = min(VEC, ly.nout - j * VEC);
                const size_t e0 = ((size_t)gi * Y + gy) * TH + gk0;
                if (nv == VEC && e0 % VEC == 0) {
                    co_put(P, e0, v, wt, nbytes);
                } else {  // a ragged or unaligned group (TH or the chunk not a multiple of VEC)
#pragma unroll
                    for (int o = 0; o < VEC; ++o)
                        if (o < nv) P[e0 + o] = v[o];
                }
#pragma unroll
                for (int o = 0; o < VEC; ++o) {
                    if (o >= nv) break;
                    const unsigned lin = (unsigned)(e0 + o);
                    if constexpr (sizeof(T) == 4) {
                        bk = max(bk, argmax_key((float)v[o], lin));
                    } else if (pc_better(v[o], lin, bv, bl)) {
                        bv = v[o];
                        bl = lin;
                    }
                }
            }
        }
    }
    if constexpr (sizeof(T) == 4) {
        pc_block_key_max<NW>(bk, res_slot, blockIdx.x, wave);
    } else {
        const PcBest<T> best = pc_block_best<NW>(bv, bl, s_bv, s_bl, wave, co_lds_barrier);
        if (tid == 0) {
            bmax[blockIdx.x] = best.v;
            bidx[blockIdx.x] = best.l;
        }
    }
    PC_STAMP(6, 4);
}

}  // namespace
