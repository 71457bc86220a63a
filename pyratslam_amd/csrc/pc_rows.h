// rows   : pc_excite_rows + pc_path_rows, a block owns a few layers and rows over the
//          whole Y extent (Y <= 128); small grids, and any filter table too large for LDS
// Part of posecell.hip, the one translation unit: not free-standing (it relies on the
// includes and on the headers that posecell.hip includes before it).

namespace {

// ---------------------------------------------------------------------------
// Row-tiled forms (the fast path for Y <= 128).  A block (512 threads = 8
// waves) owns BK layers x BX rows x the whole Y extent; lanes own columns, so
// the periodic wrap in y is a 3-cell LDS halo and no hot loop divides.  The
// wrapped layer/row index of every halo row is computed once per block (one
// modulo per thread) into LDS; then every global load of a wave is issued
// unconditionally (column clamped) before the first use, so each phase costs
// one memory round trip.  One halo layer per wave for the stencil passes, which
// are register-blocked per column (a lane walks the x direction).
// ---------------------------------------------------------------------------
// Row-tile shape: BK layers x BX rows per block, BK + 6 = BK * BX waves (one
// window layer per wave in the y/x passes, one output row per wave in the theta
// pass).  6 x 2 (12 waves) keeps the 64x64x36 grid at 192 blocks, one per CU:
// 2 x 4 (8 waves) made 288 blocks, and the CUs that ran two of them set the
// kernels' span (path 8.7 -> 5.2 us, excitation 4.6 -> 3.8 us first block start
// to last block end; it also re-evaluates fewer halo rows and layers per output).
constexpr int RT_BX = 2, RT_BK = 6, RT_NW = RT_BK + 6, RT_NT = 64 * RT_NW;

template <typename T, int YP>
__global__ __launch_bounds__(RT_NT) void pc_excite_rows(const T* __restrict__ P, T* __restrict__ Q,
                                                         double* __restrict__ part,
                                                         unsigned long long* __restrict__ res_slot,
                                                         int X, int Y, int TH, SepKernel<T> k) {
    constexpr int BX = RT_BX, BK = RT_BK, HX = BX + 2 * HALF, HK = BK + 2 * HALF, NW = RT_NW;
    constexpr int RW = YP + 2 * HALF, JC = YP / 64, NR = HK * HX, RPW = NR / NW;
    static_assert(NR % NW == 0 && HK == NW && BK * BX == NW, "row tile / wave mapping");
    __shared__ T s_in[NR * RW];
    __shared__ T s_e[HK * BX * YP];
    __shared__ T s_i[HK * BX * YP];
    __shared__ int s_row[NR];
    __shared__ double s_red[NW];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int i0 = blockIdx.x * BX, k0 = blockIdx.y * BK;
    PC_STAMP(0, 0);
    if (res_slot != nullptr && blockIdx.x == 0 && blockIdx.y == 0)
        for (int i = tid; i < RES_SLOTS; i += blockDim.x) st_wt(&res_slot[i], 0ull);  // this step's path kernel max-reduces into them
    if (tid < NR) {
        const int kk = tid / HX, a = tid - kk * HX;
        s_row[tid] = rs::wrapi(k0 - HALF + kk, TH) * X + rs::wrapi(i0 - HALF + a, X);
    }
    co_lds_barrier();

    T v[RPW][JC];
#pragma unroll
    for (int q = 0; q < RPW; ++q) {
        const T* src = P + (size_t)s_row[wave + NW * q] * Y;
#pragma unroll
        for (int jc = 0; jc < JC; ++jc) v[q][jc] = src[min(lane + 64 * jc, Y - 1)];
    }
#pragma unroll
    for (int q = 0; q < RPW; ++q) {
        T* dst = s_in + (wave + NW * q) * RW;
#pragma unroll
        for (int jc = 0; jc < JC; ++jc) {
            const int c = lane + 64 * jc;
            if (c < Y) {
                dst[HALF + c] = v[q][jc];
                if (c < HALF) dst[HALF + Y + c] = v[q][jc];
                if (c >= Y - HALF) dst[c - (Y - HALF)] = v[q][jc];
            }
        }
    }
    co_lds_barrier();
    PC_STAMP(0, 1);

    // y pass (7 taps along the row) then x pass (7 rows) in registers; one layer per wave
    {
        const int kk = wave;
#pragma unroll
        for (int jc = 0; jc < JC; ++jc) {
            const int j = lane + 64 * jc;
            if (j >= Y) continue;
            T ey[HX], iy[HX];
#pragma unroll
            for (int a = 0; a < HX; ++a) {
                const T* rw = s_in + (kk * HX + a) * RW + j;
                T e = 0, g = 0;
#pragma unroll
                for (int t = 0; t < FL; ++t) {
                    const T x = rw[t];
                    e += k.ge[t] * x;
                    g += k.gi[t] * x;
                }
                ey[a] = e;
                iy[a] = g;
            }
#pragma unroll
            for (int i = 0; i < BX; ++i) {
                T e = 0, g = 0;
#pragma unroll
                for (int t = 0; t < FL; ++t) {
                    e += k.ge[t] * ey[i + t];
                    g += k.gi[t] * iy[i + t];
                }
                s_e[(kk * BX + i) * YP + j] = e;
                s_i[(kk * BX + i) * YP + j] = g;
            }
        }
    }
    co_lds_barrier();
    PC_STAMP(0, 2);

    // theta pass + relu(v - inhib) (posecell_network.py:339-340) + partial sum; one row per wave
    double sum = 0.0;
    {
        const int kq = wave / BX, i = wave - kq * BX;
        const int gk = k0 + kq, gi = i0 + i;
        if (gk < TH && gi < X) {
#pragma unroll
            for (int jc = 0; jc < JC; ++jc) {
                const int j = lane + 64 * jc;
                if (j >= Y) continue;
                T e = 0, g = 0;
#pragma unroll
                for (int t = 0; t < FL; ++t) {
                    e += k.ge[t] * s_e[((kq + t) * BX + i) * YP + j];
                    g += k.gi[t] * s_i[((kq + t) * BX + i) * YP + j];
                }
                const T val = (e - g) * k.scale;
                const T q = (val < k.inhib) ? T(0) : val - k.inhib;
                // write-through (sc1): nothing dirty left for the kernel's end to write back
                st_wt(&Q[((size_t)gk * X + gi) * Y + j], q);
                sum += (double)q;
            }
        }
    }
    sum = co_wave_sum(sum);
    if (lane == 0) s_red[wave] = sum;
    co_lds_barrier();  // the Q stores drain meanwhile
    if (tid == 0) {
        double t = 0.0;
#pragma unroll
        for (int w = 0; w < NW; ++w) t += s_red[w];
        st_wt(&part[blockIdx.y * gridDim.x + blockIdx.x], t);
    }
    PC_STAMP(0, 3);
}

template <typename T, int YP, typename CTL>
__global__ __launch_bounds__(RT_NT) void pc_path_rows(
    const T* __restrict__ Q, T* __restrict__ P, const double* __restrict__ part, int npart,
    const T* __restrict__ filt, int nf, CTL ctl, unsigned long long* __restrict__ res_slot,
    T* __restrict__ bmax, unsigned* __restrict__ bidx, int X, int Y, int TH) {
    constexpr int BX = RT_BX, BK = RT_BK, HX = BX + 2 * HALF, HK = BK + 2 * HALF, NW = RT_NW;
    constexpr int RW = YP + 2 * HALF, JC = YP / 64, NR = HK * HX, RPW = NR / NW;
    constexpr int NPP = 4;  // normalisation partials held per thread (npart <= NPP * RT_NT)
    static_assert(NR % NW == 0 && HK == NW && BK * BX == NW, "row tile / wave mapping");
    __shared__ T s_win[NR * RW];
    __shared__ T s_r[HK * BX * YP];
    __shared__ int s_row[NR];
    __shared__ int s_oy[HK], s_fi[HK];
    __shared__ double s_red[NW];
    __shared__ T s_bv[NW];
    __shared__ unsigned s_bl[NW];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    (void)nf;  // filter indices are validated on the host (pc_check_ctl)
    const int i0 = blockIdx.x * BX, k0 = blockIdx.y * BK;
    PC_STAMP(1, 0);

    // the block's control, and the row table straight from it (one barrier)
    if (tid < HK) {
        const int L = rs::wrapi(k0 - HALF + tid, TH);
        s_oy[tid] = rs::wrapi(ctl_oy(ctl, L), Y);
        s_fi[tid] = ctl_fi(ctl, L);
    }
    if (tid < NR) {
        const int kk = tid / HX, a = tid - kk * HX, L = rs::wrapi(k0 - HALF + kk, TH);
        // shifts may exceed the grid (vtrans large)
        s_row[tid] = L * X + rs::wrapi(i0 - HALF + a + rs::wrapi(ctl_ox(ctl, L), X), X);
    }
    co_lds_barrier();
    PC_STAMP(1, 1);
    PC_STAMP(1, 2);

    // shifted window rows: s_win[kk][a][HALF + d] = Q[L][(i0-3+a+ox) % X][(d + oy) % Y]
    T v[RPW][JC];
#pragma unroll
    for (int q = 0; q < RPW; ++q) {
        const T* src = Q + (size_t)s_row[wave + NW * q] * Y;
#pragma unroll
        for (int jc = 0; jc < JC; ++jc) v[q][jc] = src[min(lane + 64 * jc, Y - 1)];
    }
    // this wave's layer filter and the normalisation partials (reduced only at the
    // end), issued behind the window loads: a barrier waits for every load in
    // flight, so nothing global is loaded before the control barriers above
    T f[FT];
    {
        const T* fsrc = filt + (size_t)s_fi[wave] * FT;
#pragma unroll
        for (int t = 0; t < FT; ++t) f[t] = fsrc[t];
    }
    double pt[NPP];
#pragma unroll
    for (int u = 0; u < NPP; ++u) {
        const int i = tid + u * RT_NT;
        pt[u] = part[min(i, npart - 1)];  // unconditional (a guarded load got its wait hoisted)
    }
    double pextra = 0.0;  // npart beyond NPP * RT_NT (huge grids)
    for (int i = tid + NPP * RT_NT; i < npart; i += RT_NT) pextra += part[i];
#pragma unroll
    for (int q = 0; q < RPW; ++q) {
        const int row = wave + NW * q;
        const int oy = s_oy[row / HX];
        T* dst = s_win + row * RW;
#pragma unroll
        for (int jc = 0; jc < JC; ++jc) {
            const int c = lane + 64 * jc;
            if (c >= Y) continue;
            int d = c - oy;
            if (d < 0) d += Y;
            dst[HALF + d] = v[q][jc];
            if (d < HALF) dst[HALF + Y + d] = v[q][jc];
            if (d >= Y - HALF) dst[d - (Y - HALF)] = v[q][jc];
        }
    }
    co_lds_barrier();
    PC_STAMP(1, 3);

    // 7x7 per-layer correlation (:273-274), register-blocked over the BX rows, clamp (:300)
    {
        const int kk = wave;
#pragma unroll
        for (int jc = 0; jc < JC; ++jc) {
            const int j = lane + 64 * jc;
            if (j >= Y) continue;
            T acc[BX];
#pragma unroll
            for (int i = 0; i < BX; ++i) acc[i] = 0;
#pragma unroll
            for (int a = 0; a < HX; ++a) {
                T w[FL];
                const T* rw = s_win + (kk * HX + a) * RW + j;
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
            for (int i = 0; i < BX; ++i) s_r[(kk * BX + i) * YP + j] = pc_clamp(acc[i]);
        }
    }
    // normalisation total (its loads were issued at entry): per thread, then per
    // wave by DPP, then over the waves through LDS behind the barrier that also
    // publishes s_r
    double tot = pextra;
#pragma unroll
    for (int u = 0; u < NPP; ++u) tot += tid + u * RT_NT < npart ? pt[u] : 0.0;
    tot = co_wave_sum(tot);
    if (lane == 0) s_red[wave] = tot;
    co_lds_barrier();
    tot = 0.0;
#pragma unroll
    for (int w = 0; w < NW; ++w) tot += s_red[w];
    PC_STAMP(1, 4);

    // theta filter (:310), clamp (:314), normalise (:343-345), store, argmax (:317-319):
    // float32 as the largest packed (value, ~index) key, float64 as value/index pairs
    T bv = -std::numeric_limits<T>::infinity();
    unsigned bl = 0xFFFFFFFFu;
    unsigned long long bk = 0ull;
    {
        const PcNorm<T> nrm(tot);
        const int kq = wave / BX, i = wave - kq * BX;
        const int gk = k0 + kq, gi = i0 + i;
        if (gk < TH && gi < X) {
#pragma unroll
            for (int jc = 0; jc < JC; ++jc) {
                const int j = lane + 64 * jc;
                if (j >= Y) continue;
                T acc = 0;
#pragma unroll
                for (int z = 0; z < FL; ++z) acc += s_r[((kq + z) * BX + i) * YP + j] * (T)ctl_zf(ctl, z);
                T val = pc_clamp(acc);
                val = nrm(val);
                st_wt(&P[((size_t)gk * X + gi) * Y + j], val);
                const unsigned lin = ((unsigned)gi * Y + j) * TH + gk;
                if constexpr (sizeof(T) == 4) {
                    bk = max(bk, argmax_key((float)val, lin));
                } else if (pc_better(val, lin, bv, bl)) {
                    bv = val;
                    bl = lin;
                }
            }
        }
    }
    const int b = blockIdx.y * gridDim.x + blockIdx.x;
    if constexpr (sizeof(T) == 4) {
        pc_block_key_max<NW>(bk, res_slot, b, wave);
    } else {
        // block argmax -> one (value, index) partial per block (pc_argmax_steps reduces)
        const PcBest<T> best = pc_block_best<NW>(bv, bl, s_bv, s_bl, wave, co_lds_barrier);
        if (tid == 0) {
            bmax[b] = best.v;
            bidx[b] = best.l;
        }
    }
    PC_STAMP(1, 5);
}

}  // namespace
