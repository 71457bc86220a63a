// The pose-cell ensemble's host rules (DESIGN sections 35 and 36): the LDS plan of one member's
// workgroup, the compact control record of one step, the split of a run into launches, the
// rule and the device form of a run's injections and the pose stage's scratch.
// Pure functions of integers and small arrays, shared by pose_ensemble.hip (host side and
// kernel: the kernel takes its offsets from the same PceFit the host computed) and by
// tests/pce_plan_main.cpp (built with the plain host compiler: no HIP runtime call here).
//
// LDS plan of a member on an (X, Y, TH) grid, PS = Y * TH cells per x-plane, all float32:
//   red      256 B             the block reductions' per-wave words (16 doubles, 16 keys)
//   state    X * Y * TP        the volume, theta pitch TP = TH | 1 (odd: the theta pass walks
//                              columns, a lane per column, and an odd pitch spreads them over
//                              the banks; the path filter's lanes run along theta either way)
//   temp     2 * PS            one plane pair (ge, gi) after the theta taps
//   ring     10 * 2 * PS       7 plane pairs after the theta and y taps, in walk order, and
//                              the pairs of planes 0, 1, 2 kept for the wrap at the far end
//   filt     PCE_MAX_FILTERS * 49   the path filters
//   ctl      2 * record        this step's control and the next one's, fetched a step ahead
// temp and ring are contiguous: once the excitation is done they are the path filter's
// layer scratch, 22 * PS floats = path_layers layers of X * Y cells.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

#include "ratslam_abi.h"

namespace rs {

constexpr size_t PCE_LDS_BYTES = 160 * 1024;   // one compute unit's LDS
constexpr int PCE_THREADS = 1024;              // a member's workgroup
constexpr int PCE_MIN_DIM = 7;                 // one wrap per 7-tap window
constexpr int PCE_MAX_FILTERS = 16;            // path filters staged in LDS (the reference's table has 4)
constexpr int PCE_RING = 7, PCE_KEPT = 3;      // plane pairs of the x walk
constexpr int PCE_TAPS = 7;
// One launch's control records for all members stay within this many bytes: the device holds
// two such slots (a launch reads one while the next one's copy lands), 64 MiB in all, and a
// launch of 256 members of 36 layers still runs 585 steps, so the state's round trip through
// HBM (62 KiB per member and launch) stays below a thousandth of a launch.
constexpr size_t PCE_CTL_BUDGET = 32u << 20;

struct PceFit {
    int X = 0, Y = 0, TH = 0;
    int TP = 0;            // theta pitch of the state in LDS
    int PS = 0;            // cells of an x-plane
    int path_layers = 0;   // layers the scratch holds at once (at most TH)
    // byte offsets and sizes of the regions, in the order above
    size_t red_off = 0, red_bytes = 0;
    size_t state_off = 0, state_bytes = 0;
    size_t temp_off = 0, temp_bytes = 0;
    size_t ring_off = 0, ring_bytes = 0;
    size_t filt_off = 0, filt_bytes = 0;
    size_t ctl_off = 0, ctl_bytes = 0;
    size_t total = 0;
    bool fits = false;
};

inline size_t pce_align(size_t v) { return (v + 15) / 16 * 16; }

// One step's control record: zf[7] float32, 4 bytes unused, ox[TH] and oy[TH] uint16 (reduced
// shifts), fidx[TH] uint8; a multiple of 16 bytes.
inline size_t pce_rec_bytes(int TH) { return pce_align(32 + 5 * (size_t)TH); }
inline size_t pce_rec_ox(int) { return 32; }
inline size_t pce_rec_oy(int TH) { return 32 + 2 * (size_t)TH; }
inline size_t pce_rec_fi(int TH) { return 32 + 4 * (size_t)TH; }

// The plan for a shape.  `fits`: every dimension at least 7, below 2^15, the total within one
// compute unit's LDS, and room in the scratch for one layer at least.  The sizes are filled
// in either way (64-bit: no overflow for dimensions below 2^15).
inline PceFit pce_fit(int X, int Y, int TH) {
    PceFit f;
    f.X = X;
    f.Y = Y;
    f.TH = TH;
    if (X < 1 || Y < 1 || TH < 1 || X >= 32768 || Y >= 32768 || TH >= 32768) return f;
    f.TP = TH | 1;
    const size_t ps = (size_t)Y * TH;
    size_t o = 0;
    auto region = [&](size_t& off, size_t& bytes, size_t n) {
        off = o;
        bytes = n;
        o = pce_align(o + n);
    };
    region(f.red_off, f.red_bytes, 256);
    region(f.state_off, f.state_bytes, 4 * (size_t)X * Y * f.TP);
    region(f.temp_off, f.temp_bytes, 4 * 2 * ps);
    f.ring_off = f.temp_off + f.temp_bytes;   // contiguous with temp (the path scratch)
    f.ring_bytes = 4 * 2 * ps * (PCE_RING + PCE_KEPT);
    o = pce_align(f.ring_off + f.ring_bytes);
    region(f.filt_off, f.filt_bytes, 4 * (size_t)PCE_MAX_FILTERS * PCE_TAPS * PCE_TAPS);
    region(f.ctl_off, f.ctl_bytes, 2 * pce_rec_bytes(TH));
    f.total = o;
    const size_t layers = (f.temp_bytes + f.ring_bytes) / (4 * (size_t)X * Y);
    f.fits = X >= PCE_MIN_DIM && Y >= PCE_MIN_DIM && TH >= PCE_MIN_DIM && f.total <= PCE_LDS_BYTES && layers >= 1 &&
             ps < (1u << 24);
    if (f.fits) {
        f.PS = (int)ps;
        f.path_layers = (int)std::min<size_t>(layers, (size_t)TH);
    }
    return f;
}

// o mod n in [0, n) for any int o (n >= 1): the kernel never reduces a shift itself.
inline int pce_reduce_shift(int o, int n) {
    const int r = o % n;
    return r < 0 ? r + n : r;
}

// One step's control into its record (fidx in [0, 256), checked by the caller).
inline void pce_pack(int X, int Y, int TH, const int32_t* ox, const int32_t* oy, const int32_t* fidx,
                     const double* zf, unsigned char* rec) {
    float z[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int t = 0; t < PCE_TAPS; ++t) z[t] = (float)zf[t];
    std::memcpy(rec, z, 32);
    unsigned char* px = rec + pce_rec_ox(TH);
    unsigned char* py = rec + pce_rec_oy(TH);
    unsigned char* pf = rec + pce_rec_fi(TH);
    for (int k = 0; k < TH; ++k) {
        const uint16_t sx = (uint16_t)pce_reduce_shift(ox[k], X), sy = (uint16_t)pce_reduce_shift(oy[k], Y);
        std::memcpy(px + 2 * k, &sx, 2);
        std::memcpy(py + 2 * k, &sy, 2);
        pf[k] = (unsigned char)fidx[k];
    }
    const size_t used = pce_rec_fi(TH) + (size_t)TH;
    std::memset(rec + used, 0, pce_rec_bytes(TH) - used);
}

// A record read back: the reduced shifts, the filter rows and the taps as the kernel sees them.
inline void pce_unpack(int TH, const unsigned char* rec, int32_t* ox, int32_t* oy, int32_t* fidx, float* zf) {
    std::memcpy(zf, rec, sizeof(float) * PCE_TAPS);
    for (int k = 0; k < TH; ++k) {
        uint16_t sx, sy;
        std::memcpy(&sx, rec + pce_rec_ox(TH) + 2 * k, 2);
        std::memcpy(&sy, rec + pce_rec_oy(TH) + 2 * k, 2);
        ox[k] = sx;
        oy[k] = sy;
        fidx[k] = rec[pce_rec_fi(TH) + k];
    }
}

// Steps per launch for B members: `forced` (RS_PCE_CHUNK) when positive, else as many as keep
// one launch's records within PCE_CTL_BUDGET, one at least.
inline int pce_chunk_len(int B, int TH, int forced) {
    if (forced > 0) return forced;
    const size_t k = PCE_CTL_BUDGET / ((size_t)B * pce_rec_bytes(TH));
    return (int)std::min<size_t>(std::max<size_t>(k, 1), 1u << 20);
}
inline int pce_chunk_count(int n, int K) { return n <= 0 ? 0 : (n + K - 1) / K; }
// Launch c of a run of n steps cut by K: steps [*first, *first + *count).
inline void pce_chunk(int n, int K, int c, int* first, int* count) {
    *first = c * K;
    *count = std::min(K, n - c * K);
}

// ---- injections inside a run (rs_pce_run_inject) ----
// The rule of a run's injections: B members, n steps, ni injections (member[ni], step[ni],
// energy[ni], loc[3 ni]).  The index of the first injection that breaks it with the reason in
// *why, or -1.  It is pc_ctl.h's pc_inj_first_bad per member: a member in [0, B); a step in
// [0, n] and not below the step of the member's injection before it in list order (the order
// across members is free); a location that is a cell inside the grid, (RS_PC_INJ_AT_PEAK, ., .),
// or (RS_PC_INJ_SAME_AS, k, .) with 0 <= k < i and member[k] == member[i]; an energy that is
// a finite float32.  The reasons are tried in that order.  Reads [0, ni) of each array only.
enum PceInjBad {
    PCE_INJ_OK = 0,
    PCE_INJ_BAD_MEMBER,
    PCE_INJ_BAD_STEP,
    PCE_INJ_BAD_ORDER,
    PCE_INJ_BAD_SAME,
    PCE_INJ_BAD_CELL,
    PCE_INJ_BAD_ENERGY
};

// |e| rounds to a finite float32: below the midpoint of FLT_MAX and 2^128 (the tie goes to 2^128)
inline bool pce_finite_f32(double e) { return std::fabs(e) < 0x1.ffffffp127; }

inline int pce_inj_first_bad(int B, int X, int Y, int TH, int n, int ni, const int32_t* member, const int32_t* step,
                             const double* energy, const int32_t* loc, PceInjBad* why) {
    // by[0 .. ni): the injections ordered by member, list order inside a member, so that the
    // one before injection i of its member is its neighbour there
    std::vector<int> by((size_t)std::max(ni, 0)), before((size_t)std::max(ni, 0), -1);
    for (int i = 0; i < ni; ++i) by[i] = i;
    std::stable_sort(by.begin(), by.end(), [&](int a, int b) { return member[a] < member[b]; });
    for (int g = 1; g < ni; ++g)
        if (member[by[g]] == member[by[g - 1]]) before[by[g]] = by[g - 1];
    for (int i = 0; i < ni; ++i) {
        const int32_t* l = loc + 3 * (size_t)i;
        PceInjBad bad = PCE_INJ_OK;
        if (member[i] < 0 || member[i] >= B) bad = PCE_INJ_BAD_MEMBER;
        else if (step[i] < 0 || step[i] > n) bad = PCE_INJ_BAD_STEP;
        else if (before[i] >= 0 && step[i] < step[before[i]]) bad = PCE_INJ_BAD_ORDER;
        else if (l[0] == RS_PC_INJ_AT_PEAK) bad = PCE_INJ_OK;
        else if (l[0] == RS_PC_INJ_SAME_AS)
            bad = l[1] >= 0 && l[1] < i && member[l[1]] == member[i] ? PCE_INJ_OK : PCE_INJ_BAD_SAME;
        else if (!(l[0] >= 0 && l[0] < X && l[1] >= 0 && l[1] < Y && l[2] >= 0 && l[2] < TH)) bad = PCE_INJ_BAD_CELL;
        if (bad == PCE_INJ_OK && !pce_finite_f32(energy[i])) bad = PCE_INJ_BAD_ENERGY;
        if (bad != PCE_INJ_OK) {
            *why = bad;
            return i;
        }
    }
    *why = PCE_INJ_OK;
    return -1;
}

// An injection as the kernel reads it, 16 bytes: the step it stands in front of, the kind of
// its location, the cell's C-order linear index (explicit) or the grouped index of the
// injection it repeats (same-as), and the energy as the float32 that is added.
enum { PCE_INJ_EXPLICIT = 0, PCE_INJ_PEAK = 1, PCE_INJ_SAME = 2 };
struct PceInjRec {
    int32_t step;
    int32_t kind;
    uint32_t arg;
    float energy;
};
static_assert(sizeof(PceInjRec) == 16, "the device form of an injection");

// A list that pce_inj_first_bad accepts in its device form: member m's records are
// rec[off[m] .. off[m + 1]), in list order (off[B + 1], rec[ni]); grouped[i] is the place of
// the caller's injection i among them, which is also where the kernel leaves its resolved
// cell, and a same-as k has become grouped[k].
inline void pce_inj_group(int B, int Y, int TH, int ni, const int32_t* member, const int32_t* step,
                          const double* energy, const int32_t* loc, uint32_t* off, PceInjRec* rec, int32_t* grouped) {
    for (int m = 0; m <= B; ++m) off[m] = 0;
    for (int i = 0; i < ni; ++i) ++off[member[i] + 1];
    for (int m = 0; m < B; ++m) off[m + 1] += off[m];
    std::vector<uint32_t> next(off, off + B);
    for (int i = 0; i < ni; ++i) grouped[i] = (int32_t)next[member[i]]++;
    for (int i = 0; i < ni; ++i) {
        const int32_t* l = loc + 3 * (size_t)i;
        PceInjRec& r = rec[grouped[i]];
        r.step = step[i];
        r.energy = (float)energy[i];
        if (l[0] == RS_PC_INJ_AT_PEAK) r.kind = PCE_INJ_PEAK, r.arg = 0;
        else if (l[0] == RS_PC_INJ_SAME_AS) r.kind = PCE_INJ_SAME, r.arg = (uint32_t)grouped[l[1]];
        else r.kind = PCE_INJ_EXPLICIT, r.arg = ((uint32_t)l[0] * Y + l[1]) * TH + l[2];
    }
}

// ---- the sub-cell pose inside a run ----
// The pose stage's scratch for a radius r, w = 2r + 1, all float64: the box (w^3), R and C
// (w^2 each), the three marginals (3w) and the six rows of weights (6w); 4,032 bytes at r = 3.
// It lies at the head of temp + ring, which are dead between a step's theta pass and the next
// step's excitation: the pose adds no LDS region and pce_fit's total does not change.
inline size_t pce_pose_scratch_bytes(int r) {
    const size_t w = 2 * (size_t)r + 1;
    return 8 * (w * w * w + 2 * w * w + 3 * w + 6 * w);
}
// Whether a plan's scratch holds it (every shape pce_fit accepts does, at every radius whose
// box the grid holds: the smallest, 7 x 7 x 7, has 4,312 bytes there).
inline bool pce_pose_fits(const PceFit& f, int r) {
    return r >= 1 && r <= 3 && f.temp_off % 8 == 0 && pce_pose_scratch_bytes(r) <= f.temp_bytes + f.ring_bytes;
}

}  // namespace rs
