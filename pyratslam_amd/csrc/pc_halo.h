// halo   : pc_step_halo, one launch per step: a block owns a 4 x 4 tile through all
//          layers and recomputes the excitation on its halo (float32, small grids)
// Part of posecell.hip, the one translation unit: not free-standing (it relies on the
// includes and on the headers that posecell.hip includes before it).

namespace {

// ---------------------------------------------------------------------------
// Halo form: ONE launch per step (float32; X, Y >= HF_W; TH == HF_TH).
//
// The reference's step (posecell_network.py:326-353) has one global dependency, the
// normalisation total (:343-345), and two local ones: the excitation's 3-cell halo
// (:336) and the path filter's shifted 7 x 7 window (:273).  The two-launch forms
// hand the excited volume Q from one kernel to the next through memory.  Here a
// block recomputes the excitation on its halo instead, so the only hand-off left is
// the one a kernel boundary gives for free: the state and its total.
//  * Between the launches of a batch the state is kept UNNORMALISED,
//    U = relu(conv_z(relu(conv_xy(Q)))), with the per-block partial sums of the
//    total t of Q (max(conv(Q/t), 0) = max(conv(Q), 0)/t for t > 0, which the
//    two-launch forms use too).  The next launch sums the partials and forms
//    P = U * (1/t) as it loads: the same product
//    the two-launch path kernels apply before their store, so P is the same.
//  * The argmax of a step (:317-319) is taken from those scaled values, exactly the
//    values of the state: by the next launch over its own tile, and for the last step
//    of a call by pc_halo_finish, which also stores the normalised state (between
//    calls the handle's state is normalised, as in every other form) and exports the
//    keys of all steps to the host (its last block, by an agent-scope counter).
//  * A block owns a 4 x 4 tile through all TH layers (256 blocks at 64 x 64).  Layer
//    j's path output needs Q on the 10 x 10 window shifted by the layer's (ox, oy),
//    and that Q needs P on the 16 x 16 window around it.  The excitation runs theta
//    pass first: the union of the step's shifted 16 x 16 windows goes global -> LDS
//    by LDS-DMA (each cell's theta column is contiguous, theta-fastest C order, so the
//    pieces are whole 1 KiB runs per wave-instruction); the theta pass reads it in
//    place, a lane per window cell through a run of layers (phase 2 below); then per
//    layer on its own window the y pass (16 x 10), the x pass (10 x 10) with the
//    inhibition, the 7 x 7 path filter and clamp, the theta filter and clamp, and the
//    write-through store.
//  * The partial sums cover, for layer j, the block's tile shifted by layer j's
//    shift (the centre of its Q window): those shifted tiles partition each layer as
//    the tiles do.
// ---------------------------------------------------------------------------
// (HF_T, the 4 x 4 tile, HF_W = 16, a layer's excitation window, HF_TH, HF_UMAX and HF_NEAR: pc_ctl.h)
constexpr int HF_Q = HF_T + 2 * HALF;         // 10: a layer's excited (Q) window
constexpr int HF_NW = 9, HF_NT = 64 * HF_NW;  // 576 threads: one task per (layer, window row) at TH = 36
// theta-pass windows, (e, i) pairs [j][rx][ry], row pitch 18 pairs: the y pass's 16-byte
// row reads (16 lanes on consecutive rows, 36 dwords apart) are conflict-free
constexpr int HF_WP = 18, HF_WJ = HF_W * HF_WP;
constexpr int HF_YC = HF_W + 4;               // y-pass outputs per Q column (16 rows, 16-byte aligned)
constexpr int HF_YL = HF_Q * HF_YC;           // ... per layer, [qc][rx]
constexpr int HF_QJ = HF_Q * HF_Q + 4;        // Q window per layer
constexpr int HF_EXP_MAX = 64;                // steps whose keys pc_halo_finish exports itself
// calls of at most this many steps poll their result words (pc_poll_words); longer ones
// wait in the stream synchronisation with the CPU idle (a 4,000-step run: 9.13 polled vs
// 9.02 us per step synchronised, tools/pc_ab.py, round 5)
constexpr int HF_POLL_MAX = 64;
constexpr int HF_FLAGS = 1024;   // pc_halo_finish blocks' flags in pinned host memory

typedef float hf_f2 __attribute__((ext_vector_type(2)));  // (excitatory, inhibitory) pairs: packed FMAs

// The normalisation total of a step from its per-block partials, formed by every wave
// itself in one fixed order (so every block gets the same bits): 4 per lane, then DPP.
// Split in two so a kernel can issue the loads first and sum them later, behind other
// loads already in flight (pc_step_halo).
__device__ inline void pc_partials_issue(const double* __restrict__ part, int npart, double (&pt)[4]) {
    const int lane = threadIdx.x & 63, np1 = npart > 0 ? npart - 1 : 0;
#pragma unroll
    for (int u = 0; u < 4; ++u) pt[u] = part[min(lane + 64 * u, np1)];  // unconditional
}
__device__ inline double pc_partials_sum(const double* __restrict__ part, int npart, const double (&pt)[4]) {
    const int lane = threadIdx.x & 63;
    double tot = 0.0;
#pragma unroll
    for (int u = 0; u < 4; ++u) tot += lane + 64 * u < npart ? pt[u] : 0.0;
    for (int i = lane + 256; i < npart; i += 64) tot += part[i];
    return co_wave_sum(tot);
}
__device__ inline double pc_partials_total(const double* __restrict__ part, int npart) {
    double pt[4];
    pc_partials_issue(part, npart, pt);
    return pc_partials_sum(part, npart, pt);
}
// (hf_pack and hf_magic, the host's forming of the preloaded arguments below: pc_ctl.h)

// EXC: excitation only (rs_pc_excite, the step the reference runs before a LUT
// KeyError): zero shifts, Q of the own cells stored into Uo (theta-fastest), partials.
// The first HF_PRELOAD arguments are everything the union image's LDS-DMA addresses
// need (the state, the grid, the block count, the union's origin and extent packed
// as 16-bit pairs): posecell.hip is built with -amdgpu-kernarg-preload-count, so they
// arrive in scalar registers with the wave and the image's loads issue without a
// kernel-argument round trip (two dependent ones before: the block count, then the
// union, 0.84 us from the block's start to the DMA issue at 64 x 64 x 36).
template <bool EXC, int TH>
__global__ __launch_bounds__(HF_NT) void pc_step_halo(
    const float* __restrict__ U, int xy, int gxnb, int ulo, int uext, unsigned mgx, unsigned muh,
    const double* __restrict__ part_in, int npart_in, float* __restrict__ Uo, double* __restrict__ part_out,
    unsigned long long* __restrict__ slot_prev, unsigned long long* __restrict__ slot_zero,
    const float* __restrict__ filt, int nf, PcCtlHalo ctl, SepKernel<float> k,
    unsigned long long* __restrict__ rec) {
    // TH: 36 (configs[1], the ROS node: the tuned phases below), or another even extent up
    // to HF_TH (18: configs[0]'s grid, 10: simulate.py's), whose theta columns are not
    // whole 16-byte pieces: the image then loads in 4-byte pieces, the theta pass runs a
    // thread per union cell (cell_pass below) and the theta filter in 2-layer groups
    static_assert(TH % 2 == 0 && TH >= FL + HALF && TH <= HF_TH, "an even theta extent, 10 .. HF_TH");
    constexpr bool V4 = TH % 4 == 0;
    constexpr int PW = V4 ? 4 : 1, NV = TH / PW;   // image pieces (PW floats each) per theta column
    constexpr int WBUF = HF_UMAX * TH + 64 * 4;   // union image [cell][layer] (+ a wave-instruction of slack)
    constexpr int YBUF = 2 * TH * HF_YL;
    constexpr int BBUF = WBUF > YBUF ? WBUF : YBUF;
    constexpr int PP = TH + 64;   // path outputs per cell: rows TH dwords apart modulo the 64 banks
    static_assert(HF_T * HF_T * PP <= BBUF && TH * HF_QJ <= 2 * TH * HF_WJ, "buffer reuse");
    // theta-pass (e, i) windows, then a dump slot per thread (a lane outside a layer's
    // window stores there: no branch); then Q
    __shared__ __attribute__((aligned(16))) float s_t[2 * (TH * HF_WJ + HF_NT)];
    __shared__ __attribute__((aligned(16))) float s_b[BBUF];  // union image; then y pass e | i; then path outputs
    __shared__ __attribute__((aligned(16))) float s_ftab[RT_NFMAX * ST_FTP];
    __shared__ int s_fo[TH];
    __shared__ double s_red[HF_NW];
    __shared__ unsigned long long s_rk[HF_NW];
    __shared__ int s_cnt[HF_NW];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int X = xy & 0xFFFF, Y = (int)((unsigned)xy >> 16), gx = gxnb & 0xFFFF, nblk = (int)((unsigned)gxnb >> 16);
    const int tile = st_tile(blockIdx.x, nblk);
    const int ty = (int)__umulhi((unsigned)tile, mgx);   // tile / gx (hf_magic)
    const int x0 = (tile - ty * gx) * HF_T, y0 = ty * HF_T;
    const int tw = min(HF_T, X - x0), tht = min(HF_T, Y - y0);
    const int cux = (short)(ulo & 0xFFFF), cuy = ulo >> 16;   // the union's origin (centred shifts)
    const int UW = uext & 0xFFFF, UH = uext >> 16, nu = UW * UH;
    const int ux0 = co_wrap(x0 - 2 * HALF + cux, X), uy0 = co_wrap(y0 - 2 * HALF + cuy, Y);
    const bool dma = nu <= HF_UMAX;
    PC_STAMP(7, 0);
    // the partial sums of the state entering the step, issued ahead of the union image so
    // they land first and the total is formed while the image is in flight
    double pt[4];
    pc_partials_issue(part_in, npart_in, pt);
    // 1. the union image, issued first: piece p = tid + HF_NT * r is piece p % NVU of union
    //    unit p / NVU (a unit: UC cells of one union row, units row-major, UH / UC per row),
    //    landing at s_b + PWU p.  TH % 4 == 0: a unit is a cell of TH / 4 16-byte pieces.
    //    Otherwise, when the host made the union's start column and width even (and Y is
    //    even: make_ctl_halo), a unit is a cell pair, 2 TH floats from an even cell, 16-byte
    //    aligned (TH / 2 16-byte pieces); else a cell of TH 4-byte pieces.
    auto issue = [&](auto pw_c, auto nvu_c, auto uc_c) __attribute__((always_inline)) {
        constexpr int PWU = decltype(pw_c)::value, NVU = decltype(nvu_c)::value, UC = decltype(uc_c)::value;
        constexpr int DC = HF_NT / NVU, DL = HF_NT % NVU, NR = (HF_UMAX / UC * NVU + HF_NT - 1) / HF_NT;
        // A lane walks its pieces with full-rate 32-bit arithmetic only (no 64-bit,
        // quarter-rate address math; measured neutral: the issue, about 0.95 us from the
        // block's start at 64 x 64 x 36, is not VALU-bound, r4 probe): the row's first cell rb =
        // gr * Y carried incrementally (the union row advances by dU or dU + 1 < X per
        // round and UW <= X, so one wrap suffices), a 32-bit byte offset from the state's
        // base (n * 4 <= INT_MAX, pc_halo_fit) by a 24-bit multiply (cells < 2^24).
        // Units per row: UH / UC, by the same high multiply (UC c / UH, c < 2^15)
        const int UHU = UH / UC, npc = nu / UC * NVU, XY = X * Y;
        const int dU = (int)__umulhi((unsigned)(UC * DC), muh), dV = DC - dU * UHU;
        int c = tid / NVU, l4 = tid - c * NVU, ui = (int)__umulhi((unsigned)(UC * c), muh), vi = c - ui * UHU;
        int rb = ux0 + ui;
        rb = (rb >= X ? rb - X : rb) * Y;
#pragma unroll
        for (int r = 0; r < NR; ++r) {
            const int i0 = r * HF_NT + wave * 64;  // wave-uniform
            if (i0 < npc) {
                if (i0 + lane < npc) {
                    int gc = uy0 + UC * vi;
                    gc -= gc >= Y ? Y : 0;
                    const unsigned boff = __umul24((unsigned)(rb + gc), (unsigned)(4 * TH)) + 4u * PWU * (unsigned)l4;
                    const auto gsrc = (__attribute__((address_space(1))) const void*)(reinterpret_cast<const char*>(U) + boff);
                    const auto ldst = (__attribute__((address_space(3))) void*)(s_b + PWU * i0);
                    if constexpr (PWU == 4) __builtin_amdgcn_global_load_lds(gsrc, ldst, 16, 0, 0);
                    else __builtin_amdgcn_global_load_lds(gsrc, ldst, 4, 0, 0);
                }
            }
            l4 += DL;
            vi += dV;
            rb += dU * Y;
            if (l4 >= NVU) {
                l4 -= NVU;
                ++vi;
            }
            if (vi >= UHU) {
                vi -= UHU;
                rb += Y;
            }
            rb -= rb >= XY ? XY : 0;
        }
    };
    using I1 = std::integral_constant<int, 1>;
    using I2 = std::integral_constant<int, 2>;
    using I4 = std::integral_constant<int, 4>;
    if (dma) {
        if constexpr (V4) {
            issue(I4{}, std::integral_constant<int, TH / 4>{}, I1{});
        } else {
            if (((cuy | UH | Y) & 1) == 0) issue(I4{}, std::integral_constant<int, TH / 2>{}, I2{});
            else issue(I1{}, std::integral_constant<int, TH>{}, I1{});
        }
    }
    PC_STAMP(10, 0);
    // the normalisation of the state entering the step, the filter table, the control
    // (lane L of every wave holds layer L's window start, read by readlane in phase 2)
    const int lsx = ctl.sx[lane < TH ? lane : 0], lsy = ctl.sy[lane < TH ? lane : 0];
    const float fr = tid < nf * FT ? filt[tid] : 0.f;
    static_assert(RT_NFMAX * FT <= HF_NT, "one filter tap per thread");
    if (tid < TH) s_fo[tid] = ctl.fo[tid] * ST_FTP;
    const PcNorm<float> nrm(pc_partials_sum(part_in, npart_in, pt));
    if (tid < nf * FT) s_ftab[(tid / FT) * ST_FTP + tid % FT] = fr;
    // the tap pairs and the wrap flag (kernel arguments beyond the preloaded ones) in
    // registers before the barrier: hipcc otherwise loads them after it, a scalar round
    // trip at the head of phase 2
    hf_f2 gei[FL];
#pragma unroll
    for (int t = 0; t < FL; ++t) {
        gei[t] = hf_f2{k.ge[t], k.gi[t]};
        asm volatile("" : "+s"(gei[t]));
    }
    int cwrap = ctl.wrap;
    asm volatile("" : "+s"(cwrap));
    // likewise the inhibition's constants (phase 4) and the theta filter (phase 6)
    float kscale = k.scale, kinhib = k.inhib, zf[FL];
    asm volatile("" : "+s"(kscale), "+s"(kinhib));
#pragma unroll
    for (int z = 0; z < FL; ++z) {
        zf[z] = ctl.zf[z];
        asm volatile("" : "+s"(zf[z]));
    }
    if (slot_zero != nullptr && blockIdx.x == 0)
        for (int i = tid; i < RES_SLOTS; i += HF_NT) st_wt(&slot_zero[i], 0ull);  // the next launch max-reduces into them
    if (dma) __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0): this wave's LDS-DMA pieces have landed
    PC_STAMP(10, 1);
    co_lds_barrier();
    PC_STAMP(7, 1);

    // 2. the theta pass of both Gaussians, as packed (e, i) FMAs, into the layers'
    //    windows [j][rx][ry] (row pitch HF_WP).
    hf_f2* s_tw = reinterpret_cast<hf_f2*>(s_t);
    unsigned long long bk = 0ull;
    const bool want_key = slot_prev != nullptr;
    PC_STAMP(11, 0);
    // a thread per union cell (theta extents other than HF_TH; at HF_TH a union larger
    // than the LDS-DMA image)
    auto cell_passes = [&]() __attribute__((always_inline)) {
        // a union spanning a whole period (the windows wrap inside it), or one larger
        // than the LDS-DMA image (columns from memory): thread c takes union cell c's
        // column, scales it, forms all TH theta-pass outputs in registers and stores
        // those of the windows holding the cell (a lane outside a window stores into its
        // own dump slot, a select rather than a branch, so the layers' FMA chains share
        // one basic block and interleave).  The own tile's keys: wave 8 when the union
        // is in LDS (below; HF_UMAX < 512, so wave 8 holds no union cell), else here.
        static_assert(HF_UMAX <= 8 * 64, "wave 8 takes no union cell");
        auto cell_pass = [&](int c, auto wrap_c) __attribute__((always_inline)) {
            constexpr bool WRAP = decltype(wrap_c)::value;
            const int ui = (int)__umulhi((unsigned)c, muh), vi = c - ui * UH;   // c / UH (hf_magic)
            const int cw = ui * HF_WP + vi, dump = TH * HF_WJ + tid;
            // (no wrap) lane L: layer L's window start as packed 16-bit (x, y), and the
            // byte offset of its window cell (0, 0) in layer 0's window image; the lane's
            // cell, packed and in bytes (pinned: one subtraction per layer each)
            const int lsp = (lsx << 16) + lsy, lso8 = 8 * (lsx * HF_WP + lsy - lane * HF_WJ);
            int uvp = (ui << 16) + vi, cw8 = 8 * cw;
            asm volatile("" : "+v"(uvp), "+v"(cw8));
            const int dump8 = 8 * dump;
            int gr = ux0 + ui, gc = uy0 + vi;
            gr -= gr >= X ? X : 0;
            gc -= gc >= Y ? Y : 0;
            float p[TH];
            // the column as 16-byte vectors (TH % 4 == 0) or 8-byte pairs (TH even: a
            // column starts 8-byte aligned)
            using CV = typename std::conditional<V4, co_f4, hf_f2>::type;
            constexpr int CW = V4 ? 4 : 2;
            auto rd = [&](const float* base) __attribute__((always_inline)) {
                const CV* src = reinterpret_cast<const CV*>(base);
#pragma unroll
                for (int v = 0; v < TH / CW; ++v) {
                    const CV x = src[v];
#pragma unroll
                    for (int w = 0; w < CW; ++w) p[CW * v + w] = x[w];
                }
            };
            if (dma) rd(s_b + c * TH);
            else rd(U + ((size_t)gr * Y + gc) * TH);
            nrm(p);
            if (want_key && !dma && (unsigned)(gr - x0) < (unsigned)tw && (unsigned)(gc - y0) < (unsigned)tht) {
                const unsigned lin0 = ((unsigned)gr * Y + gc) * TH;
#pragma unroll
                for (int q = 0; q < TH; ++q) bk = max(bk, argmax_key(p[q], lin0 + q));
            }
            auto store = [&](int j, hf_f2 eg) __attribute__((always_inline)) {
                if constexpr (WRAP) {
                    const int sxj = __builtin_amdgcn_readlane(lsx, j), syj = __builtin_amdgcn_readlane(lsy, j);
                    int rx = ui - sxj, ry = vi - syj;
                    rx += rx < 0 ? UW : 0;
                    ry += ry < 0 ? UH : 0;
                    const int a = j * HF_WJ + (int)__umul24((unsigned)rx, (unsigned)HF_WP) + ry;
                    s_tw[max((unsigned)rx, (unsigned)ry) < (unsigned)HF_W ? a : dump] = eg;
                } else {
                    // in the window: both 16-bit fields of the packed difference in [0, 16)
                    // (a negative y part borrows into bits 4-15 of the low field);
                    // |coordinates| < 2^15
                    static_assert(HF_W == 16, "the packed window test");
                    const int d = uvp - __builtin_amdgcn_readlane(lsp, j);
                    const int a8 = cw8 - __builtin_amdgcn_readlane(lso8, j);
                    *reinterpret_cast<hf_f2*>(reinterpret_cast<char*>(s_tw) + ((d & 0xFFF0FFF0) == 0 ? a8 : dump8)) = eg;
                }
            };
            // layers in pairs: two independent FMA chains interleaved
#pragma unroll
            for (int j = 0; j < TH; j += 2) {
                hf_f2 ea = {0.f, 0.f}, eb = {0.f, 0.f};
#pragma unroll
                for (int t = 0; t < FL; ++t) {
                    ea += gei[t] * p[(j + t + TH - HALF) % TH];
                    eb += gei[t] * p[(j + 1 + t + TH - HALF) % TH];
                }
                store(j, ea);
                store(j + 1, eb);
            }
        };
        if (cwrap) {
#pragma unroll 1
            for (int c = tid; c < nu; c += HF_NT) cell_pass(c, std::true_type{});
        } else {
#pragma unroll 1
            for (int c = tid; c < nu; c += HF_NT) cell_pass(c, std::false_type{});
        }
    };
    if constexpr (TH == HF_TH) {
      if (dma) {
        // the common case, read straight from the union image [cell][layer]: wave w < 8
        // takes window rows 4(w&3) .. +3 (a lane per window cell) through the layers
        // [18(w>>2), +18).  Layer j's window cell (rx, ry) is union cell (rx + sx_j,
        // ry + sy_j); its 7 theta taps are 7 consecutive floats of that cell's column,
        // held as 16-byte quads of the column in registers (conflict-free reads: lanes
        // 144 bytes apart).  While the shift stays the layer before's, a layer needs at
        // most one new quad, read PF layers ahead; a layer with a new shift (a
        // wave-uniform branch, a few per run) reloads the quads its taps and the next
        // PF layers' reach.  Each quad is scaled by 1/t as it arrives (the same products
        // as every other form's); every lane's store is one of a window's own cells.
        if (nrm.div) {   // 1/t not finite (t tiny): divide the image in place first
            for (int c = tid; c < nu; c += HF_NT) {
                co_f4* col = reinterpret_cast<co_f4*>(s_b + c * TH);
#pragma unroll
                for (int v = 0; v < NV; ++v) {
                    co_f4 x = col[v];
#pragma unroll
                    for (int w = 0; w < 4; ++w) x[w] = nrm(x[w]);
                    col[v] = x;
                }
            }
            co_lds_barrier();
        }
        if (wave < 8) {
            constexpr int JH = TH / 2, PF = 3;
            const int rx = 4 * (wave & 3) + (lane >> 4), ry = lane & 15;
            const int loff = (lsx * UH + lsy) * TH;   // lane L: layer L's window place in the union
            const int cbase = (rx * UH + ry) * TH;
            auto run = [&](auto hh, auto wc) __attribute__((always_inline)) {
                constexpr int J0 = decltype(hh)::value * JH;
                constexpr bool WRAP = decltype(wc)::value;
                // quads kq = 0 .. NQ-1 hold layers 4 (QB + kq) .. +3 (mod TH) of the current cell
                constexpr int QB = (J0 - HALF + 4 * TH) / 4 - TH, NQ = (J0 + JH - 1 + HALF - 4 * QB) / 4 + 1;
                co_f4 qd[NQ];
                hf_f2* dst = s_tw + J0 * HF_WJ + (rx * HF_WP + ry);
                // a union spanning a whole period (cwrap: 16 + the shifts' spread exceeds X
                // or Y, so the union is the period): window cell (rx, ry) of layer j is
                // union cell ((rx + sx_j) mod UW, (ry + sy_j) mod UH); else no wrap occurs
                auto colof = [&](int j) __attribute__((always_inline)) {
                    int ux = rx + __builtin_amdgcn_readlane(lsx, j), uy = ry + __builtin_amdgcn_readlane(lsy, j);
                    ux -= ux >= UW ? UW : 0;
                    uy -= uy >= UH ? UH : 0;
                    return s_b + (ux * UH + uy) * TH;
                };
                int prev = __builtin_amdgcn_readlane(loff, J0);
                const float* col = WRAP ? colof(J0) : s_b + cbase + prev;
                auto ld = [&](int kq) {
                    qd[kq] = *reinterpret_cast<const co_f4*>(col + ((4 * (QB + kq) + 4 * TH) % TH)) * nrm.r;
                };
                // quads holding layers lo .. hi (relative to 4 QB), clipped to the run
                auto ld_span = [&](int lo, int hi) __attribute__((always_inline)) {
#pragma unroll
                    for (int kq = 0; kq < NQ; ++kq)
                        if (4 * kq + 3 >= lo && 4 * kq <= hi) ld(kq);
                };
                ld_span(J0 - HALF - 4 * QB, J0 + HALF + PF - 4 * QB);
                auto tapv = [&](int e) { return qd[e / 4][e % 4]; };
                // layer jj's taps (first tap e0 relative to 4 QB) in the reference's order
                auto one = [&](int jj) __attribute__((always_inline)) {
                    const int e0 = J0 + jj - HALF - 4 * QB;
                    hf_f2 eg = {0.f, 0.f};
#pragma unroll
                    for (int t = 0; t < FL; ++t) eg += gei[t] * tapv(e0 + t);
                    dst[jj * HF_WJ] = eg;
                };
                // the new shift of layer jj, if any; else the quad its taps reach PF layers on
                auto enter = [&](int jj, int o) __attribute__((always_inline)) {
                    const int e0 = J0 + jj - HALF - 4 * QB;
                    if (o == prev) {
                        const int e = e0 + 2 * HALF + PF;
                        if (e % 4 == 0 && e / 4 < NQ) ld(e / 4);
                    } else {
                        prev = o;
                        col = WRAP ? colof(J0 + jj) : s_b + cbase + o;
                        ld_span(e0, e0 + 2 * HALF + PF);
                    }
                };
                // layers in pairs: two independent FMA chains interleaved, unless the
                // second layer of the pair takes a new shift (then one after the other,
                // the first before its quads are replaced)
                static_assert(JH % 2 == 0, "layer pairs");
#pragma unroll
                for (int jj = 0; jj < JH; jj += 2) {
                    if (jj > 0) enter(jj, __builtin_amdgcn_readlane(loff, J0 + jj));
                    const int o1 = __builtin_amdgcn_readlane(loff, J0 + jj + 1);
                    if (o1 == prev) {
                        enter(jj + 1, o1);
                        const int e0 = J0 + jj - HALF - 4 * QB;
                        hf_f2 ea = {0.f, 0.f}, eb = {0.f, 0.f};
#pragma unroll
                        for (int t = 0; t < FL; ++t) {
                            ea += gei[t] * tapv(e0 + t);
                            eb += gei[t] * tapv(e0 + 1 + t);
                        }
                        dst[jj * HF_WJ] = ea;
                        dst[(jj + 1) * HF_WJ] = eb;
                    } else {
                        one(jj);
                        enter(jj + 1, o1);
                        one(jj + 1);
                    }
                }
            };
            // (separate code for a wrapped union, so the common case keeps its registers)
            if (!cwrap) {
                if (wave < 4) run(std::integral_constant<int, 0>{}, std::false_type{});
                else run(std::integral_constant<int, 1>{}, std::false_type{});
            } else {
                if (wave < 4) run(std::integral_constant<int, 0>{}, std::true_type{});
                else run(std::integral_constant<int, 1>{}, std::true_type{});
            }
        } else if (want_key) {
            // wave 8: the argmax of the state entering the step over the own tile (lane:
            // cell lane & 15, quads lane >> 4 + 4 m)
            const int i = (lane & 15) >> 2, jc = lane & 3;
            int cu = co_wrap(2 * HALF - cux, X) + i, cv = co_wrap(2 * HALF - cuy, Y) + jc;
            cu -= cu >= X ? X : 0;
            cv -= cv >= Y ? Y : 0;
            if (i < tw && jc < tht && cu < UW && cv < UH) {
                const unsigned lin0 = ((unsigned)(x0 + i) * Y + (y0 + jc)) * TH;
                const co_f4* src = reinterpret_cast<const co_f4*>(s_b + (cu * UH + cv) * TH);
                for (int v = lane >> 4; v < NV; v += 4) {
                    const co_f4 x = src[v];
#pragma unroll
                    for (int w = 0; w < 4; ++w) bk = max(bk, argmax_key(x[w] * nrm.r, lin0 + 4 * v + w));  // (r = 1 once divided)
                }
            }
        }
      } else {
        cell_passes();
      }
    } else {
        cell_passes();
        if (dma && want_key && wave == 8) {
            // the own tile's keys from the image, off the cell-pass waves (lane: cell
            // lane & 15, layers lane >> 4 + 4 m), scaled as cell_pass scales
            const int i = (lane & 15) >> 2, jc = lane & 3;
            int cu = co_wrap(2 * HALF - cux, X) + i, cv = co_wrap(2 * HALF - cuy, Y) + jc;
            cu -= cu >= X ? X : 0;
            cv -= cv >= Y ? Y : 0;
            if (i < tw && jc < tht && cu < UW && cv < UH) {
                const unsigned lin0 = ((unsigned)(x0 + i) * Y + (y0 + jc)) * TH;
                const float* src = s_b + (cu * UH + cv) * TH;
                for (int q = lane >> 4; q < TH; q += 4) bk = max(bk, argmax_key(nrm(src[q]), lin0 + q));
            }
        }
    }
    PC_STAMP(11, 1);
    PC_STAMPW(12);
    if (want_key && tid < tw * tht) {
        // an own cell outside the union (a large uniform shift): its key from memory
        const int i = tid / tht, j = tid - i * tht;
        int cu = co_wrap(2 * HALF - cux, X) + i, cv = co_wrap(2 * HALF - cuy, Y) + j;
        cu -= cu >= X ? X : 0;
        cv -= cv >= Y ? Y : 0;
        if (cu >= UW || cv >= UH) {
            const unsigned lin0 = ((unsigned)(x0 + i) * Y + (y0 + j)) * TH;
            using CV = typename std::conditional<V4, co_f4, hf_f2>::type;
            constexpr int CW = V4 ? 4 : 2;
            const CV* src = reinterpret_cast<const CV*>(U + lin0);
#pragma unroll
            for (int v = 0; v < TH / CW; ++v) {
                const CV x = src[v];
#pragma unroll
                for (int w = 0; w < CW; ++w) bk = max(bk, argmax_key(nrm(x[w]), lin0 + CW * v + w));
            }
        }
    }
    co_lds_barrier();
    PC_STAMP(7, 2);

    // 3. y pass: task (layer j, window row rx) -> 10 outputs of each Gaussian, stored
    //    transposed, [j][qc][rx] (column pitch HF_YC), so that the x pass reads each
    //    column as four 16-byte vectors (conflict-free: lanes on consecutive columns are
    //    20 dwords apart, layers HF_YL apart)
    float* s_ye = s_b;
    float* s_yi = s_b + TH * HF_YL;
    // task (layer j, row rx, outputs QC0 .. QC0 + NQ - 1); the SIMDs are balanced (wave w
    // runs on SIMD w % 4): waves 0-7 take layers 0-31 whole, one wave per SIMD (8, 5, 6, 7)
    // a part of layers 32-35 (576 whole tasks on 9 waves put three on SIMD 0)
    auto ytask = [&](int j, int rx, auto qc0_c, auto nq_c) __attribute__((always_inline)) {
        constexpr int QC0 = decltype(qc0_c)::value, NQ = decltype(nq_c)::value;
        const co_f4* rw = reinterpret_cast<const co_f4*>(s_tw + j * HF_WJ + rx * HF_WP);
        hf_f2 w[HF_W];   // (e, i) of the row's 16 cells (those the outputs reach)
#pragma unroll
        for (int q = QC0 / 2; q <= (QC0 + NQ + 2 * HALF - 1) / 2; ++q) {
            const co_f4 a = rw[q];
            w[2 * q] = hf_f2{a.x, a.y};
            w[2 * q + 1] = hf_f2{a.z, a.w};
        }
        float* de = s_ye + j * HF_YL + rx;
        float* di = s_yi + j * HF_YL + rx;
#pragma unroll
        for (int qc = QC0; qc < QC0 + NQ; ++qc) {
            hf_f2 eg = {0.f, 0.f};
#pragma unroll
            for (int t2 = 0; t2 < FL; ++t2) eg += gei[t2] * w[qc + t2];
            de[qc * HF_YC] = eg.x;
            di[qc * HF_YC] = eg.y;
        }
    };
    static_assert(HF_W == 16 && HF_Q == 10 && HF_NW == 9, "phase 3's task split");
    if constexpr (TH == 18) {
        // waves 0-3 take layers 0-15 whole, one wave per SIMD; layers 16-17 go in 4-, 3-
        // and 3-output pieces to waves 5, 6, 7 (SIMDs 1-3): 288 whole tasks on 5 waves
        // put two on SIMD 0
        using I = std::integral_constant<int, 0>;
        if (wave < 4) ytask(tid >> 4, tid & 15, I{}, std::integral_constant<int, HF_Q>{});
        const int jr = 16 + ((lane >> 4) & 1), rr = lane & 15;
        if (lane < 32) {
            if (wave == 5) ytask(jr, rr, I{}, std::integral_constant<int, 4>{});
            else if (wave == 6) ytask(jr, rr, std::integral_constant<int, 4>{}, std::integral_constant<int, 3>{});
            else if (wave == 7) ytask(jr, rr, std::integral_constant<int, 7>{}, std::integral_constant<int, 3>{});
        }
    } else if constexpr (TH != 36) {
        for (int t = tid; t < TH * HF_W; t += HF_NT)
            ytask(t >> 4, t & 15, std::integral_constant<int, 0>{}, std::integral_constant<int, HF_Q>{});
    } else {
        using I = std::integral_constant<int, 0>;
        if (wave < 8) ytask(tid >> 4, tid & 15, I{}, std::integral_constant<int, HF_Q>{});
        const int jr = 32 + (lane >> 4), rr = lane & 15;
        if (wave == 8) ytask(jr, rr, I{}, std::integral_constant<int, 3>{});
        else if (wave == 5) ytask(jr, rr, std::integral_constant<int, 3>{}, std::integral_constant<int, 3>{});
        else if (wave == 6) ytask(jr, rr, std::integral_constant<int, 6>{}, std::integral_constant<int, 2>{});
        else if (wave == 7) ytask(jr, rr, std::integral_constant<int, 8>{}, std::integral_constant<int, 2>{});
    }
    co_lds_barrier();
    PC_STAMP(7, 3);

    // 4. x pass + inhibition (:339-340): task (layer j, Q column qc) -> 10 Q values;
    //    the partial sum over the layer's shifted own tile (Q rows/columns 3 .. 3+tw)
    float* s_q = s_t;
    double qs = 0.0;
    // task (layer j, Q column qc, Q rows 5H .. 5H + 4), H-uniform per wave; the SIMDs are
    // balanced: H = 0 on waves 0-5, H = 1 on waves 8, 6, 7, 1, 2, 3 (three 5-row tasks
    // per SIMD, where 360 10-row tasks on 6 waves put two on SIMDs 0 and 1)
    auto xtask = [&](int t, auto h_c) __attribute__((always_inline)) {
        constexpr int H = decltype(h_c)::value;
        if (t >= TH * HF_Q) return;
        const int j = t / HF_Q, qc = t - j * HF_Q;
        const co_f4* ce = reinterpret_cast<const co_f4*>(s_ye + j * HF_YL + qc * HF_YC) + H;
        const co_f4* ci = reinterpret_cast<const co_f4*>(s_yi + j * HF_YL + qc * HF_YC) + H;
        hf_f2 w[12];   // rows 4H .. 4H + 11
#pragma unroll
        for (int r4 = 0; r4 < 3; ++r4) {
            const co_f4 a = ce[r4], b = ci[r4];
#pragma unroll
            for (int u = 0; u < 4; ++u) w[4 * r4 + u] = hf_f2{a[u], b[u]};
        }
        const bool ocol = (unsigned)(qc - HALF) < (unsigned)tht;
#pragma unroll
        for (int o = 0; o < 5; ++o) {
            const int qa = 5 * H + o;
            hf_f2 eg = {0.f, 0.f};
#pragma unroll
            for (int a = 0; a < FL; ++a) eg += gei[a] * w[H + o + a];
            const float v = (eg.x - eg.y) * kscale;
            const float q = (v < kinhib) ? 0.f : v - kinhib;
            const bool own = ocol && (unsigned)(qa - HALF) < (unsigned)tw;
            if (own) qs += (double)q;
            if constexpr (EXC) {
                if (own) Uo[((size_t)(x0 + qa - HALF) * Y + (y0 + qc - HALF)) * TH + j] = q;
            } else {
                s_q[j * HF_QJ + qa * HF_Q + qc] = q;
            }
        }
    };
    if constexpr (TH != 36) {
        for (int t = tid; t < 2 * TH * HF_Q; t += HF_NT) {
            if (t < TH * HF_Q) xtask(t, std::integral_constant<int, 0>{});
            else xtask(t - TH * HF_Q, std::integral_constant<int, 1>{});
        }
    } else {
        static_assert(TH * HF_Q <= 6 * 64 && TH * HF_Q > 5 * 64, "phase 4's task split: 6 wave-tasks per half");
        if (wave < 6) xtask(wave * 64 + lane, std::integral_constant<int, 0>{});
        const int s1 = wave == 8 ? 0 : wave == 6 ? 1 : wave == 7 ? 2 : wave == 1 ? 3 : wave == 2 ? 4 : wave == 3 ? 5 : -1;
        if (s1 >= 0) xtask(s1 * 64 + lane, std::integral_constant<int, 1>{});
    }
    float* s_po = s_b;
    // rec (the last step of a call that leaves the state unnormalised, pc_run_halo):
    // the key of the block's largest output U and, below, how many of its outputs lie
    // within a relative 2^-20 of it (HF_NEAR): P = U * (1/t) rounds monotonically, so the
    // first maximum of P is the first maximum of U unless another cell lies that close
    unsigned long long rk = 0ull;
    co_f4 uv = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};   // (lanes past a 2-layer group's stay -inf)
    bool has_uv = false;
    // every thread's partial sum and key, past Q in s_t (free from here on): the last
    // wave, which has no task in phase 5, reduces them there -- lane l adds the values of
    // thread l of every wave in wave order, then one DPP reduction (a fixed order, so
    // every launch gives the same bits) -- and stores the block's partial sum and key, so
    // the block's tail is the theta filter and its store
    constexpr int QSW = (TH * HF_QJ + 1) / 2 * 2;   // (8-byte aligned)
    double* s_qsw = reinterpret_cast<double*>(s_t + QSW);
    unsigned long long* s_bkw = reinterpret_cast<unsigned long long*>(s_qsw + HF_NT);
    static_assert(QSW + 4 * HF_NT <= 2 * (TH * HF_WJ + HF_NT), "per-thread sums and keys in s_t");
    if constexpr (!EXC) {
        s_qsw[tid] = qs;
        s_bkw[tid] = bk;
        co_lds_barrier();
        PC_STAMP(7, 4);
        static_assert(TH * 8 <= (HF_NW - 1) * 64, "the last wave has no phase-5 task");
        if (wave == HF_NW - 1) {
            double v = 0.0;
            unsigned long long kb = 0ull;
#pragma unroll
            for (int w = 0; w < HF_NW; ++w) {
                v += s_qsw[w * 64 + lane];
                kb = max(kb, s_bkw[w * 64 + lane]);
            }
            const double bsum = co_wave_sum(v);
            if (want_key) kb = co_wave_max(kb);
            if (lane == 0) {
                st_wt(&part_out[blockIdx.x], bsum);
                if (want_key) atomicMax(slot_prev + (blockIdx.x & (RES_SLOTS - 1)), kb);
            }
        }
        // 5. 7 x 7 path filter (:273) + clamp (:300): task (layer j, tile column tb,
        //    row pair ap) -> 2 outputs from 8 x 7 Q values; into [cell][3 + j] rows with
        //    wrapped copies (layers TH-3.. before, 0..6 after), so every theta window
        //    below is one contiguous aligned run
        //    The SIMDs are balanced: waves 0-3 take layers 0-31 (2-row tasks), wave 5 layers
        //    32-35 as 1-row tasks (lane: layer 32 + (lane >> 4), row (lane >> 2) & 3, column
        //    lane & 3); 288 2-row tasks on waves 0-4 put two on SIMD 0, beside wave 8
        auto ptask = [&](int j, int tb, int a0, auto n_c) __attribute__((always_inline)) {
            constexpr int NO = decltype(n_c)::value;
            float f[FT];
            st_filter<float>(s_ftab + s_fo[j], f);
            float acc[NO];
#pragma unroll
            for (int h = 0; h < NO; ++h) acc[h] = 0.f;
            const float* qw = s_q + j * HF_QJ + a0 * HF_Q + tb;
#pragma unroll
            for (int r = 0; r < NO + 2 * HALF; ++r) {  // rows of the outputs: h .. h + 6
                float w[FL];
#pragma unroll
                for (int y = 0; y < FL; ++y) w[y] = qw[r * HF_Q + y];
#pragma unroll
                for (int h = 0; h < NO; ++h) {
                    if (r - h < 0 || r - h >= FL) continue;
#pragma unroll
                    for (int y = 0; y < FL; ++y) acc[h] += w[y] * f[(r - h) * FL + y];
                }
            }
#pragma unroll
            for (int h = 0; h < NO; ++h) {
                const float v = pc_clamp(acc[h]);
                float* sp = s_po + ((a0 + h) * HF_T + tb) * PP;
                sp[HALF + j] = v;
                if (j >= TH - HALF) sp[j - TH + HALF] = v;
                if (j < FL) sp[HALF + TH + j] = v;
            }
        };
        static_assert(HF_T == 4, "phase 5's task split");
        if constexpr (TH != 36) {
            for (int t = tid; t < TH * 8; t += HF_NT)
                ptask(t >> 3, t & 3, 2 * ((t >> 2) & 1), std::integral_constant<int, 2>{});
        } else {
            if (wave < 4) ptask(tid >> 3, tid & 3, 2 * ((tid >> 2) & 1), std::integral_constant<int, 2>{});
            else if (wave == 5) ptask(32 + (lane >> 4), lane & 3, (lane >> 2) & 3, std::integral_constant<int, 1>{});
        }
        co_lds_barrier();
        PC_STAMP(7, 5);
        // 6. theta filter (:310) + clamp (:314): task (cell, group of G layers) -> one
        //    write-through store of U (normalised by the next launch): G = 4 (16 bytes),
        //    or 2 (8 bytes) when TH is not a multiple of 4
        const int nbytes = (int)min((size_t)X * Y * TH * sizeof(float), (size_t)INT_MAX);
        const bool wt = (size_t)X * Y * TH * sizeof(float) <= (size_t)INT_MAX;
        constexpr int G = V4 ? 4 : 2, NGR = TH / G, NRD = (G + 2 * HALF + G - 1) / G;
        using GV = typename std::conditional<V4, co_f4, hf_f2>::type;
        static_assert(HF_T * HF_T * NGR <= HF_NT, "one theta-filter task per thread");
        if (tid < HF_T * HF_T * NGR) {
            const int t = tid;
            const int cell = t / NGR, g = t - cell * NGR, ta = cell >> 2, tb = cell & 3;
            if (ta < tw && tb < tht) {
            const GV* sv = reinterpret_cast<const GV*>(s_po + cell * PP + G * g);
            float r[NRD * G];
#pragma unroll
            for (int q = 0; q < NRD; ++q) {
                const GV x = sv[q];
#pragma unroll
                for (int w = 0; w < G; ++w) r[G * q + w] = x[w];
            }
            GV v;
#pragma unroll
            for (int o = 0; o < G; ++o) {
                float x = 0.f;
#pragma unroll
                for (int z = 0; z < FL; ++z) x += r[o + z] * zf[z];
                v[o] = pc_clamp(x);
            }
            const unsigned lin = ((unsigned)(x0 + ta) * Y + (y0 + tb)) * TH + G * g;
            co_put(Uo, lin, v, wt, nbytes);
            if (rec) {
#pragma unroll
                for (int o = 0; o < G; ++o) {
                    rk = max(rk, argmax_key(v[o], lin + o));
                    uv[o] = v[o];
                }
                has_uv = true;
            }
            }
        }
    }
    PC_STAMP(14, 0);
    if constexpr (EXC) {   // (the excitation-only instance: the block's partial sum at its end)
        qs = co_wave_sum(qs);
        if (lane == 0) s_red[wave] = qs;
        co_lds_barrier();
        if (tid == 0) {
            double bsum = 0.0;
#pragma unroll
            for (int w = 0; w < HF_NW; ++w) bsum += s_red[w];
            st_wt(&part_out[blockIdx.x], bsum);
        }
    }
    if (rec) {
        rk = co_wave_max(rk);
        if (lane == 0) s_rk[wave] = rk;
        co_lds_barrier();
    }
    PC_STAMP(14, 1);
    PC_STAMP(14, 2);
    if (rec) {
        // the block's record: its largest U's key and the count of its outputs within
        // HF_NEAR of that value (the maximum itself included)
        unsigned long long m = s_rk[0];
#pragma unroll
        for (int w = 1; w < HF_NW; ++w) m = max(m, s_rk[w]);
        const float mv = __uint_as_float((unsigned)(m >> 32)), thr = mv - mv * HF_NEAR;
        int c = 0;
#pragma unroll
        for (int o = 0; o < 4; ++o) c += __popcll(__ballot(has_uv && uv[o] >= thr));
        if (lane == 0) s_cnt[wave] = c;
        co_lds_barrier();
        if (tid == 0) {
            int cnt = 0;
#pragma unroll
            for (int w = 0; w < HF_NW; ++w) cnt += s_cnt[w];
            // one 16-byte store: the record may live in pinned host memory (a one-step
            // call, pc_run_halo, whose host polls it: fine-grained host memory, which the
            // store writes through).  The count word carries REC_SET, so that neither word
            // of a landed record is zero and the host waits for both.  (Two 8-byte
            // system-scope atomic stores instead: update() 20.2-22.2 us against
            // 16.8-18.9 us, tools/pc_ab.py --mode update, round 5.)
            typedef unsigned long long u2 __attribute__((ext_vector_type(2)));
            *reinterpret_cast<u2*>(rec + 2 * blockIdx.x) = u2{m, REC_SET | (unsigned long long)cnt};
        }
    }
    PC_STAMP(7, 6);
}

// The instances of pc_step_halo: HF_TH (configs[1], the ROS node) and the even extents
// of configs[0]'s grid (18) and simulate.py's (10); pc_halo_fit admits these.
inline bool hf_th_ok(int TH) { return TH == HF_TH || TH == 18 || TH == 10; }
template <bool EXC, typename... A>
void hf_launch(int TH, dim3 grid, hipStream_t st, A... a) {
    switch (TH) {
    case 18: hipLaunchKernelGGL((pc_step_halo<EXC, 18>), grid, dim3(HF_NT), 0, st, a...); break;
    case 10: hipLaunchKernelGGL((pc_step_halo<EXC, 10>), grid, dim3(HF_NT), 0, st, a...); break;
    default: hipLaunchKernelGGL((pc_step_halo<EXC, HF_TH>), grid, dim3(HF_NT), 0, st, a...); break;
    }
}

// The end of a halo-form call: the normalised state P = U * (1/t) of the last step
// (written back, so the handle's state is normalised between calls), its argmax key
// per block into the last step's slots, optionally the float64 C-order volume into a
// pinned host array (readback='eager'), and the keys of the call's nexp steps for the
// host (the export kernel of the other forms, folded in: one launch fewer per call):
// block 0 stores the words of steps 0 .. nexp-2, whose slots earlier launches of the
// call completed, and every block stores its own key of the last step into bkey[block],
// which the host max-reduces once it has waited for the launch.  No block reads what
// another block of this launch wrote, so the kernel needs no intra-launch hand-off (the
// round-5 form handed the last step's slots to the block that counted last through an
// agent-scope counter, outside the memory model's release/acquire).
__global__ __launch_bounds__(256) void pc_halo_finish(
    const float* U, float* P,  // may be one buffer: each element is read, then written, by one thread
    int n4, const double* __restrict__ part,
    int npart, unsigned long long* __restrict__ slot, const unsigned long long* __restrict__ res,
    int nexp, unsigned long long* __restrict__ host, unsigned long long* __restrict__ bkey,
    double* __restrict__ xp, int nbytes, unsigned* __restrict__ flag, unsigned seq) {
    __shared__ unsigned long long s_bk[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (nexp > 1 && blockIdx.x == 0) {
        // steps 0 .. nexp-2: each step's max of its RES_SLOTS slots (filled by the launches
        // before this one) straight into the pinned host words
        for (int s = wave; s < nexp - 1; s += 4) {
            const unsigned long long m = pc_slots_max(res + (size_t)s * RES_SLOTS);
            if (lane == 0) __hip_atomic_store(host + s, m, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        }
    }
    const PcNorm<float> nrm(pc_partials_total(part, npart));
    unsigned long long bk = 0ull;
    typedef double d2 __attribute__((ext_vector_type(2)));
    for (int i = blockIdx.x * 256 + tid; i < n4; i += gridDim.x * 256) {
        const co_f4 u = reinterpret_cast<const co_f4*>(U)[i];
        co_f4 p;
#pragma unroll
        for (int o = 0; o < 4; ++o) {
            p[o] = nrm(u[o]);
            bk = max(bk, argmax_key(p[o], 4u * (unsigned)i + o));
        }
        co_put(P, 4 * (size_t)i, p, true, nbytes);
        if (xp) {
            d2* d = reinterpret_cast<d2*>(xp + 4 * (size_t)i);
            d[0] = d2{(double)p[0], (double)p[1]};
            d[1] = d2{(double)p[2], (double)p[3]};
        }
    }
    bk = co_wave_max(bk);
    if (lane == 0) s_bk[wave] = bk;
    // flag (an eager readback the host polls for, pc_run_halo): every wave's volume
    // stores acknowledged before the block's barrier, then one lane's system-scope
    // release and the block's flag -- the producer form MI355X_MICROARCH.md gives
    // (stores, each wave's vmcnt(0), barrier, release, vmcnt(0), flag store)
    if (flag) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (tid == 0) {
        bk = max(max(s_bk[0], s_bk[1]), max(s_bk[2], s_bk[3]));
        if (slot) atomicMax(slot + (blockIdx.x & (RES_SLOTS - 1)), bk);
        if (bkey) __hip_atomic_store(bkey + blockIdx.x, bk, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        if (flag) {   // after the block's volume and its key
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "");
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __hip_atomic_store(flag + blockIdx.x, seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        }
    }
}

}  // namespace
