// Stand-alone host test of pc_ctl.h's pc_inj_first_bad: the rule of a run's injections
// (rs_pc_run_odom_inject) against a restatement that judges every injection on its own, over
// hand-made lists -- each refusal of the rule at the first, a middle and the last place -- and
// seeded random ones, on exact-size heap arrays so that a read past step[ni) or loc[3 ni)
// is a sanitizer report.  No GPU and no HIP header; tests/test_pc_inj.py builds it with
// -fsanitize=address,undefined and runs it.  Exit status 0: every check held.
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <random>
#include <vector>

#include "pc_ctl.h"

namespace {

long g_checks = 0, g_failed = 0;

#define CHECK(cond)                                                                  \
    do {                                                                             \
        ++g_checks;                                                                  \
        if (!(cond) && ++g_failed <= 20)                                             \
            std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond);          \
    } while (0)

struct Inj {
    int step, a, b, c;
};

// injection i on its own: what is wrong with it, in the order the rule names
PcInjBad judge(const std::vector<Inj>& v, size_t i, int X, int Y, int TH, int n) {
    const Inj& e = v[i];
    if (e.step < 0) return PC_INJ_BAD_STEP;
    if (e.step > n) return PC_INJ_BAD_STEP;
    if (i > 0 && v[i - 1].step > e.step) return PC_INJ_BAD_ORDER;
    if (e.a == -1) return PC_INJ_OK;                       // RS_PC_INJ_AT_PEAK
    if (e.a == -2) {                                       // RS_PC_INJ_SAME_AS
        for (size_t k = 0; k < i; ++k)
            if ((long)k == (long)e.b) return PC_INJ_OK;
        return PC_INJ_BAD_SAME;
    }
    const bool in = e.a >= 0 && e.a <= X - 1 && e.b >= 0 && e.b <= Y - 1 && e.c >= 0 && e.c <= TH - 1;
    return in ? PC_INJ_OK : PC_INJ_BAD_CELL;
}

void check_list(const std::vector<Inj>& v, int X, int Y, int TH, int n) {
    const int ni = (int)v.size();
    // exact-size heap blocks (none at all for an empty list)
    std::unique_ptr<int32_t[]> step(ni ? new int32_t[ni] : nullptr), loc(ni ? new int32_t[3 * (size_t)ni] : nullptr);
    for (int i = 0; i < ni; ++i) {
        step[i] = v[i].step;
        loc[3 * i] = v[i].a;
        loc[3 * i + 1] = v[i].b;
        loc[3 * i + 2] = v[i].c;
    }
    int want = -1;
    PcInjBad want_why = PC_INJ_OK;
    for (size_t i = 0; i < v.size() && want < 0; ++i) {
        want_why = judge(v, i, X, Y, TH, n);
        if (want_why != PC_INJ_OK) want = (int)i;
    }
    PcInjBad why = PC_INJ_BAD_CELL;
    const int got = pc_inj_first_bad(X, Y, TH, n, ni, step.get(), loc.get(), &why);
    CHECK(got == want);
    CHECK(why == want_why);
}

}  // namespace

int main() {
    static_assert(RS_PC_INJ_AT_PEAK == -1 && RS_PC_INJ_SAME_AS == -2, "the restatement's constants");
    const int X = 21, Y = 19, TH = 36, n = 12;
    const Inj ok0{0, 3, 4, 5}, peak5{5, -1, 0, 0}, same9{9, -2, 1, 0}, end{12, 20, 18, 35};
    // the empty list, n == 0, the valid table
    check_list({}, X, Y, TH, n);
    check_list({}, X, Y, TH, 0);
    check_list({{0, -1, 0, 0}, {0, -2, 0, 7}, {0, 0, 0, 0}}, X, Y, TH, 0);
    check_list({ok0, peak5, same9, end}, X, Y, TH, n);
    check_list({ok0, ok0, peak5, peak5, same9, end, end}, X, Y, TH, n);
    // every refusal at the first, a middle and the last place
    const std::vector<Inj> bad = {{-1, 1, 1, 1}, {13, 1, 1, 1}, {13, -1, 0, 0},                  // a step outside [0, n]
                                  {21, 0, 0, 0}, {5, -3, 0, 0}, {5, 0, 19, 0}, {5, 0, -1, 0},    // a cell outside the grid
                                  {5, 0, 0, 36}, {5, 0, 0, -1}, {5, 21, 0, 0},
                                  {5, -2, -1, 0}, {5, -2, 9, 0}, {5, -2, 2147483647, 0}};        // same-as no earlier one
    for (const Inj& b : bad) {
        check_list({b}, X, Y, TH, n);
        check_list({ok0, peak5, b, same9, end}, X, Y, TH, n);
        check_list({ok0, peak5, {5, 1, 2, 3}, b}, X, Y, TH, n);
    }
    check_list({{5, -2, 0, 0}}, X, Y, TH, n);                      // same-as itself
    check_list({ok0, {5, -2, 1, 0}}, X, Y, TH, n);
    check_list({ok0, {5, -2, 0, 0}}, X, Y, TH, n);                 // (valid)
    check_list({peak5, ok0}, X, Y, TH, n);                         // steps out of order
    check_list({ok0, same9, peak5, end}, X, Y, TH, n);
    check_list({ok0, end, {11, -1, 0, 0}}, X, Y, TH, n);
    // seeded lists: mostly valid entries, one kind of damage now and then
    std::mt19937 rng(20240531u);
    auto uni = [&](int lo, int hi) { return std::uniform_int_distribution<int>(lo, hi)(rng); };
    for (int t = 0; t < 4000; ++t) {
        const int gx = uni(7, 40), gy = uni(7, 40), gth = uni(7, 40), steps = uni(0, 20), ni = uni(0, 12);
        std::vector<Inj> v;
        int st = 0;
        for (int i = 0; i < ni; ++i) {
            st = std::min(steps, st + (uni(0, 2) == 0 ? uni(0, 3) : 0));
            Inj e{st, uni(0, gx - 1), uni(0, gy - 1), uni(0, gth - 1)};
            const int kind = uni(0, 3);
            if (kind == 0) e.a = -1;
            if (kind == 1 && i > 0) e.a = -2, e.b = uni(0, i - 1);
            switch (uni(0, 40)) {                                   // damage
            case 0: e.step = steps + uni(1, 3); break;
            case 1: e.step = -uni(1, 3); break;
            case 2: e.step = st - 1; break;                        // (below the one before, or -1)
            case 3: e.a = gx + uni(0, 2), e.b = 0; break;
            case 4: e.a = 0, e.b = gy + uni(0, 2); break;
            case 5: e.a = 0, e.b = 0, e.c = gth + uni(0, 2); break;
            case 6: e.a = -2, e.b = i + uni(0, 2); break;
            case 7: e.a = -2, e.b = -uni(1, 3); break;
            case 8: e.a = -uni(3, 9); break;
            default: break;
            }
            v.push_back(e);
        }
        check_list(v, gx, gy, gth, steps);
    }
    std::printf("pc_inj: %ld checks, %ld failed\n", g_checks, g_failed);
    return g_failed ? 1 : 0;
}
