// The linked experience map's arithmetic and its incidence lists, shared
// by the kernels of experience_map.hip, by rs_em_relax_host and by tests/em_host_main.cpp.
// All float64, every operation correctly rounded and uncontracted (the file that includes
// this is built with -ffp-contract=off); cos / sin are the platform's.
//
//   wrap(a)        = a - 2pi * rint(a / 2pi)
//   link l = (a -> b, d, h, f), all relative to a:
//     ex = x_b - (x_a + d * cos(th_a + h)),  ey the same with sin,  df = wrap(th_b - (th_a + f))
//   sweep (damped Jacobi, reads the previous iterate only), experience i:
//     s = +0.0;  its links with i == a in ascending link id add (+ex, +ey, +df);
//     then its links with i == b in ascending link id add (-ex, -ey, -df)
//     w = c / deg_i;  x' = x + w * sx;  y' = y + w * sy;  th' = wrap(th + w * st)
//     deg_i == 0: the pose is copied unchanged
//
// Incidence lists (CSR): off[2n + 1], adj[2L]; adj[off[2i] .. off[2i+1]) are the links with
// a == i, adj[off[2i+1] .. off[2i+2]) those with b == i, both in ascending link id.
#pragma once

#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define EM_HD __host__ __device__
#else
#define EM_HD
#endif

namespace rs {

struct EmLink {
    int32_t a, b;
    double d, h, f;
};
static_assert(sizeof(EmLink) == 32, "EmLink is the 32-byte record of LinkedExperienceMap.links()");

constexpr double EM_TWO_PI = 6.283185307179586476925286766559;

EM_HD inline double em_wrap(double a) { return a - EM_TWO_PI * rint(a / EM_TWO_PI); }

// Pose of a new experience reached from `from` by the measurement (d, h, f): its residual
// on the link from -> new is zero.
EM_HD inline void em_place(const double* from, double d, double h, double f, double* out) {
    const double th = from[2];
    out[0] = from[0] + d * cos(th + h);
    out[1] = from[1] + d * sin(th + h);
    out[2] = em_wrap(th + f);
}

EM_HD inline void em_residual(const double* p, const EmLink& l, double& ex, double& ey, double& df) {
    const double* pa = p + 3 * (size_t)l.a;
    const double* pb = p + 3 * (size_t)l.b;
    const double tha = pa[2];
    ex = pb[0] - (pa[0] + l.d * cos(tha + l.h));
    ey = pb[1] - (pa[1] + l.d * sin(tha + l.h));
    df = em_wrap(pb[2] - (tha + l.f));
}

// One experience of one sweep: src is the previous iterate, dst the next (xyth, 3 per experience).
EM_HD inline void em_relax_one(int i, const double* src, double* dst, const int32_t* off,
                               const int32_t* adj, const EmLink* lk, double c) {
    const double x = src[3 * (size_t)i], y = src[3 * (size_t)i + 1], th = src[3 * (size_t)i + 2];
    const int b0 = off[2 * (size_t)i], b1 = off[2 * (size_t)i + 1], b2 = off[2 * (size_t)i + 2];
    if (b2 == b0) {
        dst[3 * (size_t)i] = x;
        dst[3 * (size_t)i + 1] = y;
        dst[3 * (size_t)i + 2] = th;
        return;
    }
    double sx = 0.0, sy = 0.0, st = 0.0, ex, ey, df;
    for (int k = b0; k < b1; ++k) {
        em_residual(src, lk[adj[k]], ex, ey, df);
        sx += ex;
        sy += ey;
        st += df;
    }
    for (int k = b1; k < b2; ++k) {
        em_residual(src, lk[adj[k]], ex, ey, df);
        sx -= ex;
        sy -= ey;
        st -= df;
    }
    const double w = c / (double)(b2 - b0);
    dst[3 * (size_t)i] = x + w * sx;
    dst[3 * (size_t)i + 1] = y + w * sy;
    dst[3 * (size_t)i + 2] = em_wrap(th + w * st);
}

// Build the incidence lists of nl links over n experiences into off[2n + 1] and adj[2 * nl]
// (a counting sort: two passes over the links, so each segment is in ascending link id).
// Every link's a and b must be in [0, n).
inline void em_build_incidence(int n, int nl, const EmLink* lk, int32_t* off, int32_t* adj) {
    for (int j = 0; j <= 2 * n; ++j) off[j] = 0;
    for (int l = 0; l < nl; ++l) {
        ++off[2 * lk[l].a + 1];
        ++off[2 * lk[l].b + 2];
    }
    for (int j = 0; j < 2 * n; ++j) off[j + 1] += off[j];
    // off[j] is now the start of segment j; fill with a moving cursor, then shift back
    for (int l = 0; l < nl; ++l) {
        adj[off[2 * lk[l].a]++] = l;
        adj[off[2 * lk[l].b + 1]++] = l;
    }
    for (int j = 2 * n; j > 0; --j) off[j] = off[j - 1];
    off[0] = 0;
}

}  // namespace rs
