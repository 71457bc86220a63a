// The pose-cell packet's circular centroid: the six weighted sums of a
// wrapped box round a cell, shared by pc_peak_kernel (pc_state.h), by rs_pc_peak_host and
// by tests/pc_peak_main.cpp.  All float64, every operation correctly rounded and
// uncontracted (each function switches contraction off for itself: posecell.hip is not
// built with -ffp-contract=off); no sin / cos is evaluated here, the weights are tables.
//
//   grid (X, Y, TH), cell p = (px, py, pth), radius r in 1 .. 3, w = 2r + 1 <= min(X, Y, TH)
//   box      v[i][j][k] = cell ((px+i-r) mod X, (py+j-r) mod Y, (pth+k-r) mod TH), i, j, k in 0 .. 2r
//   every sum starts from +0.0 and adds left to right, ascending:
//   R[i][j]  = sum_k v[i][j][k]          C[i][k] = sum_j v[i][j][k]
//   sx[i]    = sum_j R[i][j]             sy[j]   = sum_i R[i][j]        sth[k] = sum_i C[i][k]
//   axis a with marginal s, centre p, size N, weights sin_a[N], cos_a[N]:
//   S_a      = sum_i fl(s[i] * sin_a[(p+i-r) mod N])      C_a the same with cos_a
//   sums     = (S_x, C_x, S_y, C_y, S_th, C_th)
//
// The pose is formed by the caller: atan2(S_a, C_a) * N / 2pi, modulo N.  The device sums
// belong to the stored state, which the halo form keeps unnormalised between steps: they may
// carry one positive factor common to all cells, so only atan2 of a pair is defined for
// callers.  Where the stored state equals what was written (after rs_pc_write, before any
// step) the sums are exactly the rule's.
//
// A box is held dense, v[(i * w + j) * w + k]; R as R[i * w + j], C as C[i * w + k].
#pragma once

#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#define PK_HD __host__ __device__
#else
#define PK_HD
#endif

namespace rs {

constexpr int PC_PEAK_RMAX = 3;                  // ratslam-python's PC_CELLS_TO_AVG
constexpr int PC_PEAK_WMAX = 2 * PC_PEAK_RMAX + 1;

// Every axis must hold the box without self-overlap.
PK_HD inline bool pc_peak_fits(int X, int Y, int TH, int r) {
    const int w = 2 * r + 1;
    return r >= 1 && r <= PC_PEAK_RMAX && w <= X && w <= Y && w <= TH;
}

// (p + o - r) mod n for p in [0, n), o in [0, 2r], 2r + 1 <= n: one wrap either way.
PK_HD inline int pc_peak_wrap(int p, int o, int r, int n) {
    const int c = p + o - r;
    return c < 0 ? c + n : c >= n ? c - n : c;
}

PK_HD inline double pc_peak_R(const double* v, int w, int i, int j) {
#pragma clang fp contract(off)
    double s = 0.0;
    for (int k = 0; k < w; ++k) s += v[(i * w + j) * w + k];
    return s;
}

PK_HD inline double pc_peak_C(const double* v, int w, int i, int k) {
#pragma clang fp contract(off)
    double s = 0.0;
    for (int j = 0; j < w; ++j) s += v[(i * w + j) * w + k];
    return s;
}

// Entry c of the marginal of axis a (0: sx from R, 1: sy from R, 2: sth from C).
PK_HD inline double pc_peak_marginal(const double* R, const double* C, int w, int a, int c) {
#pragma clang fp contract(off)
    double s = 0.0;
    if (a == 0)
        for (int j = 0; j < w; ++j) s += R[c * w + j];
    else if (a == 1)
        for (int i = 0; i < w; ++i) s += R[i * w + c];
    else
        for (int i = 0; i < w; ++i) s += C[i * w + c];
    return s;
}

// sum_i fl(s[i] * t[i]), t the w weights of the box's cells along the axis.
PK_HD inline double pc_peak_dot_w(const double* s, const double* t, int w) {
#pragma clang fp contract(off)
    double acc = 0.0;
    for (int i = 0; i < w; ++i) {
        const double q = s[i] * t[i];
        acc += q;
    }
    return acc;
}

// sum_i fl(s[i] * tab[(p+i-r) mod n]): S_a with the axis's sin table, C_a with its cos table.
PK_HD inline double pc_peak_dot(const double* s, int w, const double* tab, int p, int r, int n) {
    double t[PC_PEAK_WMAX];
    for (int i = 0; i < w; ++i) t[i] = tab[pc_peak_wrap(p, i, r, n)];
    return pc_peak_dot_w(s, t, w);
}

// The six sums of a gathered box, stage by stage as the kernel's lanes take them.  dims and p
// are (X, Y, TH) and the cell; sc[a] is axis a's sin weights, then its cos weights (2 * dims[a]).
PK_HD inline void pc_peak_box_sums(const double* v, int r, const int* dims, const int32_t* p,
                                   const double* const* sc, double* sums) {
    const int w = 2 * r + 1;
    double R[PC_PEAK_WMAX * PC_PEAK_WMAX], C[PC_PEAK_WMAX * PC_PEAK_WMAX], m[3 * PC_PEAK_WMAX];
    for (int a = 0; a < w; ++a)
        for (int b = 0; b < w; ++b) {
            R[a * w + b] = pc_peak_R(v, w, a, b);
            C[a * w + b] = pc_peak_C(v, w, a, b);
        }
    for (int a = 0; a < 3; ++a)
        for (int c = 0; c < w; ++c) m[a * w + c] = pc_peak_marginal(R, C, w, a, c);
    for (int a = 0; a < 3; ++a) {
        sums[2 * a] = pc_peak_dot(m + a * w, w, sc[a], p[a], r, dims[a]);
        sums[2 * a + 1] = pc_peak_dot(m + a * w, w, sc[a] + dims[a], p[a], r, dims[a]);
    }
}

// The rule on the host alone: the box gathered from a float64 C-order (X, Y, TH) volume.
// False when the grid does not hold the box (pc_peak_fits) or the cell lies outside the grid.
inline bool pc_peak_host(int X, int Y, int TH, int r, const double* volume, const int32_t* xyz,
                         const double* sc_x, const double* sc_y, const double* sc_th, double* sums) {
    if (!pc_peak_fits(X, Y, TH, r)) return false;
    if (xyz[0] < 0 || xyz[0] >= X || xyz[1] < 0 || xyz[1] >= Y || xyz[2] < 0 || xyz[2] >= TH) return false;
    const int w = 2 * r + 1;
    double v[PC_PEAK_WMAX * PC_PEAK_WMAX * PC_PEAK_WMAX];
    for (int i = 0; i < w; ++i)
        for (int j = 0; j < w; ++j)
            for (int k = 0; k < w; ++k) {
                const size_t cx = pc_peak_wrap(xyz[0], i, r, X), cy = pc_peak_wrap(xyz[1], j, r, Y),
                             ck = pc_peak_wrap(xyz[2], k, r, TH);
                v[(i * w + j) * w + k] = volume[(cx * Y + cy) * TH + ck];
            }
    const int dims[3] = {X, Y, TH};
    const double* const sc[3] = {sc_x, sc_y, sc_th};
    pc_peak_box_sums(v, r, dims, xyz, sc, sums);
    return true;
}

}  // namespace rs
