// The pose-cell step's control records as kernel arguments and the host rules that form and
// read them: pure functions of integers and small arrays, shared by posecell.hip (its host side; the kernels: pc_cols.h, pc_halo.h, pc_state.h) and by
// tests/pc_ctl_main.cpp (built with the plain host compiler: no HIP runtime call here).
// Everything sits in the unnamed namespace, as posecell.hip's kernels do: the control
// structs are kernel parameter types, and the kernels' names carry their namespace.
#pragma once

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdint>
#include <cstring>

#include "ratslam_abi.h"

#if defined(__HIPCC__)
#define PC_HD __host__ __device__
#else
#define PC_HD
#endif

namespace {

constexpr int FL = RS_FILTER_LEN;  // 7 taps
constexpr int HALF = FL / 2;       // 3

// Per-step control of the path-integration kernel: inline by value (one launch
// carries its step's shifts, filter rows and theta filter; no copy, no extra
// dependency) when TH <= CTL_INLINE_MAX, else pointers into a device ring.
constexpr int CTL_INLINE_MAX = 128;
struct PcCtlInline {     // single update(): the launch carries the control (~700 B kernarg)
    short iox[CTL_INLINE_MAX];
    short ioy[CTL_INLINE_MAX];
    unsigned char ifi[CTL_INLINE_MAX];
    double izf[FL];
    // the union of the step's per-layer shifted windows (column form, whole theta
    // extent: every block holds every layer, so it is the same for all blocks):
    // smallest centred shifts and the union's extent in cells, formed on the host
    // (make_ctl_inline) so the path kernel issues its window loads first thing
    short umx, umy, uwx, uwy;
};

// No step's packed key is ever 0: float32 keys are (value bits << 32 | ~lin) and
// float64 keys ~lin, with lin < X*Y*TH < 2^32 - 1 (rs_pc_create).  The host writes
// RES_NONE into each step's result word before the launch and refuses a result
// still holding it after the stream has synchronised.
constexpr unsigned long long RES_NONE = 0ull;
// A step's result word when its last-step records cannot settle the first maximum of the
// scaled state (a cell within HF_NEAR of the maximum): never a valid key (a key's low
// word is ~lin >= 2, lin < X*Y*TH < 2^32 - 1, rs_pc_create)
constexpr unsigned long long RES_AMBIG = 1ull;
constexpr unsigned long long REC_SET = 1ull << 63;   // a record's count word: REC_SET | count

constexpr int CO_TX = 8, CO_TY = 8;           // column form: a block's tile
constexpr int HF_T = 4;                       // tile: HF_T x HF_T cells through all layers
constexpr int HF_W = HF_T + 4 * HALF;         // 16: a layer's excitation window
constexpr int HF_TH = 36;                     // the theta extent instantiated (configs[1], the ROS node)
constexpr int HF_UMAX = 22 * 22;              // union cells staged by LDS-DMA (|shifts| spread <= 6)
constexpr float HF_NEAR = 0x1p-20f;           // relative margin of a possible rounding tie (pc_halo_export)

// One step's control of the halo form, a kernel argument (formed on the host by make_ctl_halo).
struct PcCtlHalo {
    short sx[HF_TH], sy[HF_TH];  // layer j's 16 x 16 window starts at union row sx[j], column sy[j]
    unsigned char fo[HF_TH];     // layer j's path filter (row of the filter table)
    float zf[FL];                // theta filter (posecell_network.py:308)
    short ux, uy;                // union origin = tile origin - 6 + the smallest centred shift
    short uw, uh;                // union extent in cells (at most X, Y)
    int wrap;                    // the union is a whole period in x or y (windows wrap inside it)
};

// signed shift in (-n/2, n/2] (control shifts may exceed the grid: vtrans large)
PC_HD inline int co_centre(int o, int n) {
    const int r = o % n;
    o = r < 0 ? r + n : r;
    return o > n / 2 ? o - n : o;
}

// two 16-bit fields in one kernel argument (pc_step_halo's preloaded union origin / extent)
inline int hf_pack(short lo, short hi) {
    return (int)((unsigned)(unsigned short)lo | ((unsigned)(unsigned short)hi << 16));
}
// q = n / d for n, d < 2^16, d >= 2, by one high multiply with m = hf_magic(d): the error
// of m / 2^32 against 1 / d is below 2^-32, so n * m / 2^32 stays below the next integer
// when n < 2^32 / d
inline unsigned hf_magic(int d) { return (unsigned)(0xFFFFFFFFull / (unsigned)d + 1ull); }

// The smallest and largest centred shift of a step's TH layers, in x and in y.
struct CtlRange {
    int mnx = INT_MAX, mxx = INT_MIN, mny = INT_MAX, mxy = INT_MIN;
};
inline CtlRange ctl_shift_range(int X, int Y, int TH, const int32_t* ox, const int32_t* oy) {
    CtlRange r;
    for (int k = 0; k < TH; ++k) {
        const int cx = co_centre(ox[k], X), cy = co_centre(oy[k], Y);
        r.mnx = std::min(r.mnx, cx);
        r.mxx = std::max(r.mxx, cx);
        r.mny = std::min(r.mny, cy);
        r.mxy = std::max(r.mxy, cy);
    }
    return r;
}

// Control of one step (ox, oy, fidx: its TH layers; zf: its FL taps) as a kernel argument
// (TH <= CTL_INLINE_MAX).
inline void make_ctl_inline(int X, int Y, int TH, const int32_t* ox, const int32_t* oy, const int32_t* fidx,
                            const double* zf, PcCtlInline* c) {
    for (int k = 0; k < TH; ++k) {
        c->iox[k] = (short)ox[k];
        c->ioy[k] = (short)oy[k];
        c->ifi[k] = (unsigned char)fidx[k];
    }
    for (int z = 0; z < FL; ++z) c->izf[z] = zf[z];
    const CtlRange r = ctl_shift_range(X, Y, TH, ox, oy);
    c->umx = (short)r.mnx;
    c->umy = (short)r.mny;
    c->uwx = (short)(CO_TX + 2 * HALF + r.mxx - r.mnx);
    c->uwy = (short)(CO_TY + 2 * HALF + r.mxy - r.mny);
}

// Control of one step for the halo form: the layers' centred shifts as window starts in
// the union of the step's shifted 16 x 16 windows (the same for every block), which the
// kernel loads first thing.
inline void make_ctl_halo(int X, int Y, int TH, const int32_t* ox, const int32_t* oy, const int32_t* fidx,
                          const double* zf, PcCtlHalo* c) {
    const CtlRange r = ctl_shift_range(X, Y, TH, ox, oy);
    const int uw = std::min(HF_W + r.mxx - r.mnx, X);
    int uy = r.mny, uh = std::min(HF_W + r.mxy - r.mny, Y);
    const bool wrap = HF_W + r.mxx - r.mnx > X || HF_W + r.mxy - r.mny > Y;
    // theta extents that are not whole 16-byte pieces (pc_step_halo loads the image in
    // 16-byte pieces of cell pairs then): an even start column and width, one column more
    // on either side where needed, when that stays a union the image holds
    if (TH % 4 != 0 && Y % 2 == 0 && !wrap) {
        const int py = uy - (uy & 1), ph = (uh + (uy & 1) + 1) & ~1;
        if (ph <= Y && uw * ph <= HF_UMAX) {
            uy = py;
            uh = ph;
        }
    }
    for (int k = 0; k < TH; ++k) {
        c->sx[k] = (short)(co_centre(ox[k], X) - r.mnx);
        c->sy[k] = (short)(co_centre(oy[k], Y) - uy);
        c->fo[k] = (unsigned char)fidx[k];
    }
    for (int z = 0; z < FL; ++z) c->zf[z] = (float)zf[z];
    c->ux = (short)r.mnx;
    c->uy = (short)uy;
    c->uw = (short)uw;
    c->uh = (short)uh;
    c->wrap = wrap;
}

// pc_halo_export's last-step rule on the host, over records in pinned host memory: the
// largest key, or RES_AMBIG when another cell may round to the same scaled value; RES_NONE
// when a block's record is missing (a record's key is never 0).
inline unsigned long long halo_key_from_records(const unsigned long long* rec, int nrec) {
    unsigned long long m = 0ull;
    for (int b = 0; b < nrec; ++b) {
        if (rec[2 * b] == 0ull || rec[2 * b + 1] == 0ull) return RES_NONE;
        m = std::max(m, rec[2 * b]);
    }
    auto val = [](unsigned long long k) {
        const unsigned u = (unsigned)(k >> 32);
        float f;
        std::memcpy(&f, &u, sizeof(f));
        return f;
    };
    const float gv = val(m), thr = gv - gv * HF_NEAR;
    if (!(gv > 0.f) || std::isinf(gv) || std::isnan(gv)) return m;   // 0, inf, NaN maxima are exact
    for (int b = 0; b < nrec; ++b) {
        const unsigned long long kb = rec[2 * b];
        if (kb == m ? (rec[2 * b + 1] & ~REC_SET) > 1ull : val(kb) >= thr) return RES_AMBIG;
    }
    return m;
}

// The rule of a run's injections (rs_pc_run_odom_inject): n steps, ni injections, step[ni]
// and loc[3 ni].  The index of the first injection that breaks it with the reason in *why,
// or -1: every step in [0, n] and not below the one before; a location that is a cell
// inside the grid, (RS_PC_INJ_AT_PEAK, ., .), or (RS_PC_INJ_SAME_AS, k, .) with 0 <= k < i.
// Reads step[0 .. ni) and loc[0 .. 3 ni) only.
enum PcInjBad { PC_INJ_OK = 0, PC_INJ_BAD_STEP, PC_INJ_BAD_ORDER, PC_INJ_BAD_SAME, PC_INJ_BAD_CELL };
inline int pc_inj_first_bad(int X, int Y, int TH, int n, int ni, const int32_t* step, const int32_t* loc,
                            PcInjBad* why) {
    for (int i = 0; i < ni; ++i) {
        const int32_t* l = loc + 3 * (size_t)i;
        PcInjBad bad = PC_INJ_OK;
        if (step[i] < 0 || step[i] > n) bad = PC_INJ_BAD_STEP;
        else if (i > 0 && step[i] < step[i - 1]) bad = PC_INJ_BAD_ORDER;
        else if (l[0] == RS_PC_INJ_AT_PEAK) bad = PC_INJ_OK;
        else if (l[0] == RS_PC_INJ_SAME_AS) bad = l[1] >= 0 && l[1] < i ? PC_INJ_OK : PC_INJ_BAD_SAME;
        else if (!(l[0] >= 0 && l[0] < X && l[1] >= 0 && l[1] < Y && l[2] >= 0 && l[2] < TH)) bad = PC_INJ_BAD_CELL;
        if (bad != PC_INJ_OK) {
            *why = bad;
            return i;
        }
    }
    *why = PC_INJ_OK;
    return -1;
}

}  // namespace
