// Stand-alone host test of pc_peak_rule.h: the six sums of the pose-cell packet's circular
// centroid (rs::pc_peak_host) against a restatement written straight from the rule's text,
// with boxes centred on every corner of the grid and on its centre, so that every wrap
// occurs.  The volume and the weight tables are exact-size heap blocks: a read one cell
// outside either is an AddressSanitizer report.  No GPU and no HIP header;
// tests/test_pc_peak.py builds it with -fsanitize=address,undefined -ffp-contract=off and
// runs it.  Exit status 0: every check held.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <memory>
#include <random>

#include "pc_peak_rule.h"

namespace {

long g_checks = 0, g_failed = 0;

#define CHECK(cond)                                                                  \
    do {                                                                             \
        ++g_checks;                                                                  \
        if (!(cond) && ++g_failed <= 20)                                             \
            std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond);          \
    } while (0)

// v mod n in [0, n) by stepping (the test's own arithmetic)
int mod_steps(int v, int n) {
    while (v < 0) v += n;
    while (v >= n) v -= n;
    return v;
}

bool same_bits(double a, double b) { return std::memcmp(&a, &b, sizeof a) == 0; }

// The rule, from its text: v[i][j][k], R, C, the three marginals, the six weighted sums.
void restate(const int* d, int r, const double* vol, const int* p, const double* const* sc, double* sums) {
    const int w = 2 * r + 1;
    double v[7][7][7], R[7][7], C[7][7], m[3][7];
    for (int i = 0; i < w; ++i)
        for (int j = 0; j < w; ++j)
            for (int k = 0; k < w; ++k)
                v[i][j][k] = vol[((size_t)mod_steps(p[0] + i - r, d[0]) * d[1] + mod_steps(p[1] + j - r, d[1])) * d[2] +
                                 mod_steps(p[2] + k - r, d[2])];
    for (int i = 0; i < w; ++i)
        for (int j = 0; j < w; ++j) {
            double s = 0.0;
            for (int k = 0; k < w; ++k) s = s + v[i][j][k];
            R[i][j] = s;
        }
    for (int i = 0; i < w; ++i)
        for (int k = 0; k < w; ++k) {
            double s = 0.0;
            for (int j = 0; j < w; ++j) s = s + v[i][j][k];
            C[i][k] = s;
        }
    for (int c = 0; c < w; ++c) {
        double sx = 0.0, sy = 0.0, sth = 0.0;
        for (int q = 0; q < w; ++q) {
            sx = sx + R[c][q];
            sy = sy + R[q][c];
            sth = sth + C[q][c];
        }
        m[0][c] = sx;
        m[1][c] = sy;
        m[2][c] = sth;
    }
    for (int a = 0; a < 3; ++a) {
        double S = 0.0, Cc = 0.0;
        for (int i = 0; i < w; ++i) {
            const int c = mod_steps(p[a] + i - r, d[a]);
            const double ts = m[a][i] * sc[a][c];
            const double tc = m[a][i] * sc[a][d[a] + c];
            S = S + ts;
            Cc = Cc + tc;
        }
        sums[2 * a] = S;
        sums[2 * a + 1] = Cc;
    }
}

void run_grid(int X, int Y, int TH, std::mt19937& rng) {
    const int d[3] = {X, Y, TH};
    const size_t n = (size_t)X * Y * TH;
    std::unique_ptr<double[]> vol(new double[n]);
    std::unique_ptr<double[]> tab[3];
    const double* sc[3];
    const double two_pi = 6.283185307179586476925286766559;
    for (int a = 0; a < 3; ++a) {
        tab[a].reset(new double[2 * (size_t)d[a]]);
        for (int c = 0; c < d[a]; ++c) {
            tab[a][c] = std::sin(two_pi * c / d[a]);
            tab[a][d[a] + c] = std::cos(two_pi * c / d[a]);
        }
        sc[a] = tab[a].get();
    }
    for (int kind = 0; kind < 2; ++kind) {
        std::uniform_real_distribution<double> u(0.0, 1.0);
        // random float64 values; then float32-representable ones with a few exact zeros
        for (size_t e = 0; e < n; ++e) vol[e] = kind == 0 ? u(rng) : (e % 5 == 0 ? 0.0 : (double)(float)u(rng));
        for (int r = 1; r <= rs::PC_PEAK_RMAX; ++r) {
            const bool fits = 2 * r + 1 <= X && 2 * r + 1 <= Y && 2 * r + 1 <= TH;
            CHECK(rs::pc_peak_fits(X, Y, TH, r) == fits);
            for (int corner = 0; corner < 9; ++corner) {
                const int32_t p[3] = {corner == 8 ? X / 2 : (corner & 1) ? X - 1 : 0,
                                      corner == 8 ? Y / 2 : (corner & 2) ? Y - 1 : 0,
                                      corner == 8 ? TH / 2 : (corner & 4) ? TH - 1 : 0};
                double got[6], want[6];
                const bool ok = rs::pc_peak_host(X, Y, TH, r, vol.get(), p, sc[0], sc[1], sc[2], got);
                CHECK(ok == fits);
                if (!ok || !fits) continue;
                const int pi[3] = {p[0], p[1], p[2]};
                restate(d, r, vol.get(), pi, sc, want);
                for (int q = 0; q < 6; ++q) CHECK(same_bits(got[q], want[q]));
            }
        }
    }
    // refusals: radii outside 1 .. 3, a cell outside the grid
    const int32_t in[3] = {0, 0, 0}, out[3] = {X, 0, 0}, neg[3] = {0, -1, 0};
    double s[6];
    CHECK(!rs::pc_peak_host(X, Y, TH, 0, vol.get(), in, sc[0], sc[1], sc[2], s));
    CHECK(!rs::pc_peak_host(X, Y, TH, 4, vol.get(), in, sc[0], sc[1], sc[2], s));
    CHECK(!rs::pc_peak_host(X, Y, TH, 1, vol.get(), out, sc[0], sc[1], sc[2], s));
    CHECK(!rs::pc_peak_host(X, Y, TH, 1, vol.get(), neg, sc[0], sc[1], sc[2], s));
}

}  // namespace

int main() {
    std::mt19937 rng(20240607u);
    run_grid(7, 7, 7, rng);      // the box is the whole grid at r = 3
    run_grid(9, 12, 8, rng);     // distinct extents: an axis mix-up reads outside a block
    run_grid(21, 21, 36, rng);
    run_grid(50, 50, 10, rng);
    run_grid(5, 21, 36, rng);    // r = 3 does not fit
    run_grid(3, 3, 3, rng);      // only r = 1 fits
    std::printf("pc_peak_rule: %ld checks, %ld failed\n", g_checks, g_failed);
    return g_failed == 0 ? 0 : 1;
}
