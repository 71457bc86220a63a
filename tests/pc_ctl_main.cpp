// Stand-alone host test of pc_ctl.h: the pose-cell control records formed on the host
// (make_ctl_halo's union window, make_ctl_inline's union extent) and the halo form's
// last-step record rule (halo_key_from_records), each against a brute-force restatement of
// what the kernels rely on.  No GPU and no HIP header; tests/test_pc_ctl.py builds it with
// -fsanitize=address,undefined and runs it.  Exit status 0: every check held.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <random>
#include <vector>

#include "pc_ctl.h"

namespace {

long g_checks = 0, g_failed = 0;
const char* g_case = "";

#define CHECK(cond)                                                                        \
    do {                                                                                   \
        ++g_checks;                                                                        \
        if (!(cond) && ++g_failed <= 20)                                                   \
            std::fprintf(stderr, "%s:%d: [%s] %s\n", __FILE__, __LINE__, g_case, #cond);   \
    } while (0)

// v mod n in [0, n), by stepping (the test's own arithmetic: no % on negatives)
int mod_steps(long v, int n) {
    v -= (v / n) * (long)n;   // |v| < n now, sign of the dividend
    while (v < 0) v += n;
    while (v >= n) v -= n;
    return (int)v;
}
// the representative of o (mod n) in (-n/2, n/2]
int centred(int o, int n) {
    for (int v = -n; v <= n; ++v)
        if (2 * v > -n && 2 * v <= n && mod_steps((long)o - v, n) == 0) return v;
    return INT_MIN;
}
bool fits16(int v) { return v >= -32768 && v <= 32767; }

struct Shifts {
    std::vector<int32_t> ox, oy, f;
    double zf[FL];
};

// One step's shifts of kind `kind` (cycled by the caller) on an X x Y x TH grid.
Shifts make_shifts(std::mt19937& rng, int kind, int X, int Y, int TH) {
    auto uni = [&](int lo, int hi) { return std::uniform_int_distribution<int>(lo, hi)(rng); };
    Shifts s;
    s.ox.resize(TH);
    s.oy.resize(TH);
    s.f.resize(TH);
    for (int z = 0; z < FL; ++z) s.zf[z] = std::uniform_real_distribution<double>(0.0, 1.0)(rng);
    // spreads (largest - smallest centred shift) per kind; -1: the whole period
    int spx = uni(0, 3), spy = uni(0, 3);
    int far = 0;
    switch (kind) {
    case 0: break;                                     // a small spread, the usual step
    case 1: far = 1; break;                            // shifts beyond the grid
    case 2: spx = spy = 0; break;                      // all equal
    case 3: spx = spy = 6; break;                      // the HF_UMAX edge: 22 x 22 cells
    case 4: spx = uni(0, 1) ? 7 : 6; spy = spx == 7 ? uni(6, 7) : 7; break;   // just past it
    case 5: spx = -1; break;                           // the union wraps in x
    case 6: spy = -1; break;                           // ... in y
    case 7: spx = spy = -1; break;                     // ... in both
    case 8: spx = uni(0, X - 1); spy = uni(0, Y - 1); break;   // any spread
    default: spx = uni(4, 8); spy = uni(4, 8); far = uni(0, 1); break;
    }
    auto axis = [&](std::vector<int32_t>& o, int n, int sp) {
        // centred shifts lie in (-n/2, n/2]: n of them, lo .. hi
        const int lo = n / 2 - n + 1, hi = n / 2;
        if (sp < 0 || sp > hi - lo) sp = hi - lo;
        const int base = uni(lo, hi - sp);
        for (int k = 0; k < TH; ++k) o[k] = base + uni(0, sp);
        if (TH >= 2) {   // both ends of the spread are taken
            const int a = uni(0, TH - 1), b = (a + 1 + uni(0, TH - 2)) % TH;
            o[a] = base;
            o[b] = base + sp;
        }
        // the same shifts modulo the period, some of them far outside the grid (int16 range)
        for (int k = 0; k < TH; ++k) {
            const int m = far ? uni(-32000 / n, 32000 / n - 1) : (uni(0, 7) == 0 ? uni(-1, 1) : 0);
            o[k] += m * n;
        }
    };
    axis(s.ox, X, spx);
    axis(s.oy, Y, spy);
    for (int k = 0; k < TH; ++k) s.f[k] = uni(0, 3);
    return s;
}

void check_grid(int X, int Y, int TH, int nsets, unsigned seed) {
    static char name[64];
    std::mt19937 rng(seed);
    for (int it = 0; it < nsets; ++it) {
        const int kind = it % 10;
        std::snprintf(name, sizeof(name), "%dx%dx%d set %d kind %d", X, Y, TH, it, kind);
        g_case = name;
        const Shifts s = make_shifts(rng, kind, X, Y, TH);
        // brute force: the centred shifts and their range
        std::vector<int> cx(TH), cy(TH);
        int mnx = INT_MAX, mxx = INT_MIN, mny = INT_MAX, mxy = INT_MIN;
        for (int k = 0; k < TH; ++k) {
            cx[k] = centred(s.ox[k], X);
            cy[k] = centred(s.oy[k], Y);
            CHECK(cx[k] != INT_MIN && cy[k] != INT_MIN);
            if (cx[k] < mnx) mnx = cx[k];
            if (cx[k] > mxx) mxx = cx[k];
            if (cy[k] < mny) mny = cy[k];
            if (cy[k] > mxy) mxy = cy[k];
        }
        const int ex = HF_W + mxx - mnx, ey = HF_W + mxy - mny;   // the unclamped union extents
        if (kind == 3) CHECK(ex * ey == HF_UMAX || X < 22 || Y < 22);
        if (kind == 5 || kind == 7) CHECK(ex > X);
        if (kind == 6 || kind == 7) CHECK(ey > Y);

        PcCtlHalo c;
        std::memset(&c, 0x5A, sizeof(c));
        make_ctl_halo(X, Y, TH, s.ox.data(), s.oy.data(), s.f.data(), s.zf, &c);
        const bool wrap = ex > X || ey > Y;
        CHECK((c.wrap != 0) == wrap);
        CHECK(c.wrap == 0 || c.wrap == 1);
        CHECK(c.uw >= 1 && c.uw <= X && c.uh >= 1 && c.uh <= Y);
        // the expected window: the smallest extents that hold every layer's 16 x 16 window,
        // clamped to the period; in y widened to an even start and width where pc_step_halo
        // loads cell pairs (TH % 4 != 0, even Y), if the widened union still fits
        int uy = mny, uh = ey < Y ? ey : Y;
        const int uw = ex < X ? ex : X;
        bool widened = false;
        if (TH % 4 != 0 && Y % 2 == 0 && !wrap) {
            int py = uy, ph;
            while (mod_steps(py, 2) != 0) --py;
            ph = uy + uh - py;
            while (mod_steps(ph, 2) != 0) ++ph;
            if (ph <= Y && uw * ph <= HF_UMAX) {
                uy = py;
                uh = ph;
                widened = true;
                CHECK(mod_steps(c.uy, 2) == 0 && mod_steps(c.uh, 2) == 0);
            }
        }
        CHECK(fits16(mnx) && fits16(uy) && fits16(uw) && fits16(uh));
        CHECK(c.ux == mnx && c.uy == uy && c.uw == uw && c.uh == uh);
        int smx = INT_MIN, smy = INT_MIN, snx = INT_MAX, sny = INT_MAX;
        for (int k = 0; k < TH; ++k) {
            CHECK(c.sx[k] >= 0 && c.sy[k] >= 0);
            CHECK(fits16(cx[k] - mnx) && fits16(cy[k] - uy));
            // the window start of layer k, from the union's origin, is its centred shift's
            CHECK(mod_steps((long)c.ux + c.sx[k], X) == mod_steps(cx[k], X));
            CHECK(mod_steps((long)c.uy + c.sy[k], Y) == mod_steps(cy[k], Y));
            CHECK(mod_steps((long)c.ux + c.sx[k], X) == mod_steps(s.ox[k], X));
            CHECK(mod_steps((long)c.uy + c.sy[k], Y) == mod_steps(s.oy[k], Y));
            CHECK(s.f[k] >= 0 && s.f[k] <= 255 && c.fo[k] == s.f[k]);
            if (!wrap) {   // every window inside [0, uw) x [0, uh)
                CHECK(c.sx[k] + HF_W <= c.uw);
                CHECK(c.sy[k] + HF_W <= c.uh);
            }
            if (c.sx[k] > smx) smx = c.sx[k];
            if (c.sy[k] > smy) smy = c.sy[k];
            if (c.sx[k] < snx) snx = c.sx[k];
            if (c.sy[k] < sny) sny = c.sy[k];
        }
        if (!wrap) {   // ... and no smaller extents do: a window at either edge
            CHECK(snx == 0 && smx + HF_W == c.uw);
            if (!widened) CHECK(sny == 0 && smy + HF_W == c.uh);
            else CHECK(sny <= 1 && c.uh - (smy + HF_W) <= 1);   // at most the one column on either side
        }
        for (int z = 0; z < FL; ++z) CHECK(c.zf[z] == (float)s.zf[z]);

        PcCtlInline ci;
        std::memset(&ci, 0x5A, sizeof(ci));
        make_ctl_inline(X, Y, TH, s.ox.data(), s.oy.data(), s.f.data(), s.zf, &ci);
        CHECK(fits16(CO_TX + 2 * HALF + mxx - mnx) && fits16(CO_TY + 2 * HALF + mxy - mny));
        CHECK(ci.umx == mnx && ci.umy == mny);
        CHECK(ci.uwx == CO_TX + 2 * HALF + mxx - mnx && ci.uwy == CO_TY + 2 * HALF + mxy - mny);
        for (int k = 0; k < TH; ++k) {
            CHECK(fits16(s.ox[k]) && fits16(s.oy[k]));
            CHECK(ci.iox[k] == s.ox[k] && ci.ioy[k] == s.oy[k] && ci.ifi[k] == s.f[k]);
        }
        for (int z = 0; z < FL; ++z) CHECK(ci.izf[z] == s.zf[z]);
    }
}

unsigned long long key_of(float v, unsigned lin) {
    unsigned bits;
    std::memcpy(&bits, &v, sizeof(bits));
    return ((unsigned long long)bits << 32) | (0xFFFFFFFFu - lin);
}

void check_records() {
    g_case = "records";
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    struct R { float v; unsigned lin; unsigned long long cnt; };
    auto run = [](const std::vector<R>& r) {
        std::vector<unsigned long long> rec;
        for (const R& e : r) {
            rec.push_back(key_of(e.v, e.lin));
            rec.push_back(REC_SET | e.cnt);
        }
        return halo_key_from_records(rec.data(), (int)r.size());
    };
    // a unique maximum, wherever its block is
    CHECK(run({{1.0f, 5, 1}, {0.5f, 9, 1}, {0.25f, 2, 3}}) == key_of(1.0f, 5));
    CHECK(run({{0.5f, 9, 1}, {0.25f, 2, 1}, {1.0f, 70000, 1}}) == key_of(1.0f, 70000));
    CHECK(run({{3.5f, 0, 1}}) == key_of(3.5f, 0));
    // a missing record: either word 0, in any block
    for (int b = 0; b < 3; ++b)
        for (int w = 0; w < 2; ++w) {
            std::vector<unsigned long long> rec = {key_of(1.0f, 5), REC_SET | 1, key_of(0.5f, 9), REC_SET | 1,
                                                   key_of(0.25f, 2), REC_SET | 1};
            rec[2 * b + w] = 0ull;
            CHECK(halo_key_from_records(rec.data(), 3) == RES_NONE);
        }
    // another block's value within HF_NEAR of the maximum, and just outside it (maxima that
    // are powers of two: g - g * HF_NEAR is exact)
    for (float g : {1.0f, 0.5f, 1024.0f, 0x1p-100f}) {
        const float thr = g - g * HF_NEAR, below = std::nextafter(thr, 0.0f);
        CHECK(thr < g && below < thr);
        CHECK(run({{g, 5, 1}, {thr, 9, 1}, {g / 4, 2, 1}}) == RES_AMBIG);
        CHECK(run({{thr, 9, 1}, {g / 4, 2, 1}, {g, 5, 1}}) == RES_AMBIG);
        CHECK(run({{g, 5, 1}, {std::nextafter(g, 0.0f), 9, 1}}) == RES_AMBIG);
        CHECK(run({{g, 5, 1}, {g, 9, 1}}) == RES_AMBIG);   // the same value in a later cell
        CHECK(run({{g, 5, 1}, {below, 9, 1}, {g / 4, 2, 1}}) == key_of(g, 5));
        CHECK(run({{below, 9, 7}, {g, 5, 1}}) == key_of(g, 5));   // (another block's count does not matter)
        // the maximal block's own count of near cells
        CHECK(run({{g, 5, 2}, {g / 2, 9, 1}}) == RES_AMBIG);
        CHECK(run({{g / 2, 9, 1}, {g, 5, 300}}) == RES_AMBIG);
        CHECK(run({{g, 5, 1}, {g / 2, 9, 1}}) == key_of(g, 5));
    }
    // maxima of 0, +inf and NaN are exact, whatever the counts and the other blocks hold
    CHECK(run({{0.0f, 5, 64}, {0.0f, 9, 64}}) == key_of(0.0f, 5));
    CHECK(run({{inf, 9, 2}, {inf, 12, 1}, {1.0f, 2, 1}}) == key_of(inf, 9));
    CHECK(run({{1.0f, 2, 1}, {nan, 12, 3}, {inf, 1, 1}}) == key_of(nan, 12));
}

}  // namespace

int main() {
    const int grids[6][3] = {{16, 16, 36}, {17, 30, 36}, {21, 21, 36}, {64, 64, 36}, {32, 32, 18}, {50, 50, 10}};
    for (int g = 0; g < 6; ++g) check_grid(grids[g][0], grids[g][1], grids[g][2], 400, 1234u + g);
    check_records();
    std::printf("pc_ctl: %ld checks, %ld failed\n", g_checks, g_failed);
    return g_failed == 0 ? 0 : 1;
}
