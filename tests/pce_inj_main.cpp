// Stand-alone host test of pce_plan.h's rules for feedback inside an ensemble run (DESIGN
// section 36): pce_inj_first_bad against a restatement that judges every injection on its
// own -- each refusal at the first, a middle and the last place, and seeded random lists --,
// pce_inj_group against a restatement that collects each member's injections by scanning the
// list, and the pose scratch against temp + ring of the LDS plan.  Everything on exact-size
// heap arrays, so that a read or write past an array is a sanitizer report.  No GPU and no
// HIP header; tests/test_pce_inj.py builds it with -fsanitize=address,undefined and runs it.
// Exit status 0: every check held.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <memory>
#include <random>
#include <vector>

#include "pc_peak_rule.h"
#include "pce_plan.h"

namespace {

long g_checks = 0, g_failed = 0;

#define CHECK(cond)                                                                  \
    do {                                                                             \
        ++g_checks;                                                                  \
        if (!(cond) && ++g_failed <= 20)                                             \
            std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond);          \
    } while (0)

struct Inj {
    int member, step, a, b, c;
    double energy;
};

// injection i on its own: what is wrong with it, in the order the rule names
rs::PceInjBad judge(const std::vector<Inj>& v, size_t i, int B, int X, int Y, int TH, int n) {
    const Inj& e = v[i];
    if (e.member < 0 || e.member > B - 1) return rs::PCE_INJ_BAD_MEMBER;
    if (e.step < 0) return rs::PCE_INJ_BAD_STEP;
    if (e.step > n) return rs::PCE_INJ_BAD_STEP;
    for (size_t k = i; k-- > 0;)                              // the member's injection before this one
        if (v[k].member == e.member) {
            if (v[k].step > e.step) return rs::PCE_INJ_BAD_ORDER;
            break;
        }
    rs::PceInjBad where = rs::PCE_INJ_OK;
    if (e.a == -1) {                                          // RS_PC_INJ_AT_PEAK
    } else if (e.a == -2) {                                   // RS_PC_INJ_SAME_AS
        where = rs::PCE_INJ_BAD_SAME;
        for (size_t k = 0; k < i; ++k)
            if ((long)k == (long)e.b && v[k].member == e.member) where = rs::PCE_INJ_OK;
    } else if (!(e.a >= 0 && e.a <= X - 1 && e.b >= 0 && e.b <= Y - 1 && e.c >= 0 && e.c <= TH - 1)) {
        where = rs::PCE_INJ_BAD_CELL;
    }
    if (where != rs::PCE_INJ_OK) return where;
    const float f = (float)e.energy;                          // what the device adds
    return std::isfinite(e.energy) && std::isfinite(f) ? rs::PCE_INJ_OK : rs::PCE_INJ_BAD_ENERGY;
}

template <class T>
std::unique_ptr<T[]> exact(size_t n) {   // an exact-size heap block (none at all for no elements)
    return std::unique_ptr<T[]>(n ? new T[n] : nullptr);
}

void check_list(const std::vector<Inj>& v, int B, int X, int Y, int TH, int n) {
    const int ni = (int)v.size();
    auto member = exact<int32_t>(ni), step = exact<int32_t>(ni), loc = exact<int32_t>(3 * (size_t)ni);
    auto energy = exact<double>(ni);
    for (int i = 0; i < ni; ++i) {
        member[i] = v[i].member;
        step[i] = v[i].step;
        energy[i] = v[i].energy;
        loc[3 * i] = v[i].a;
        loc[3 * i + 1] = v[i].b;
        loc[3 * i + 2] = v[i].c;
    }
    int want = -1;
    rs::PceInjBad want_why = rs::PCE_INJ_OK;
    for (size_t i = 0; i < v.size() && want < 0; ++i) {
        want_why = judge(v, i, B, X, Y, TH, n);
        if (want_why != rs::PCE_INJ_OK) want = (int)i;
    }
    rs::PceInjBad why = rs::PCE_INJ_BAD_CELL;
    const int got = rs::pce_inj_first_bad(B, X, Y, TH, n, ni, member.get(), step.get(), energy.get(), loc.get(), &why);
    CHECK(got == want);
    CHECK(why == want_why);
    if (got >= 0) return;

    // the device form of a list the rule accepts
    auto off = exact<uint32_t>((size_t)B + 1);
    auto rec = exact<rs::PceInjRec>(ni);
    auto grouped = exact<int32_t>(ni);
    rs::pce_inj_group(B, Y, TH, ni, member.get(), step.get(), energy.get(), loc.get(), off.get(), rec.get(), grouped.get());
    CHECK(off[0] == 0 && off[B] == (uint32_t)ni);
    std::vector<int> back((size_t)ni, -1);   // grouped index -> the caller's
    for (int i = 0; i < ni; ++i) {
        CHECK(grouped[i] >= 0 && grouped[i] < ni);
        if (grouped[i] >= 0 && grouped[i] < ni) {
            CHECK(back[grouped[i]] == -1);   // a permutation
            back[grouped[i]] = i;
        }
    }
    size_t g = 0;
    for (int m = 0; m < B; ++m) {   // member m's records: its injections, in list order
        CHECK(off[m] == g);
        for (int i = 0; i < ni; ++i)
            if (v[i].member == m) {
                CHECK(grouped[i] == (int32_t)g);
                const rs::PceInjRec& r = rec[g];
                const float f = (float)v[i].energy;
                CHECK(r.step == v[i].step);
                CHECK(std::memcmp(&r.energy, &f, 4) == 0);
                if (v[i].a == -1) {
                    CHECK(r.kind == rs::PCE_INJ_PEAK);
                } else if (v[i].a == -2) {
                    CHECK(r.kind == rs::PCE_INJ_SAME);
                    CHECK(r.arg < g && r.arg >= off[m]);          // an earlier record of the same member
                    CHECK(r.arg < (uint32_t)ni && back[r.arg] == v[i].b);   // the remap and the map back are inverse
                } else {
                    CHECK(r.kind == rs::PCE_INJ_EXPLICIT);
                    CHECK(r.arg == (uint32_t)((v[i].a * Y + v[i].b) * TH + v[i].c));
                }
                ++g;
            }
        CHECK(off[m + 1] == g);
    }
}

void check_scratch() {
    CHECK(rs::pce_pose_scratch_bytes(3) == 4032);
    const int shapes[][3] = {{7, 7, 7}, {8, 8, 8}, {12, 9, 10}, {21, 21, 36}, {32, 32, 18}, {50, 50, 10}};
    for (const auto& s : shapes) {
        const rs::PceFit f = rs::pce_fit(s[0], s[1], s[2]);
        CHECK(f.fits);
        CHECK(f.ring_off == f.temp_off + f.temp_bytes && f.temp_off % 8 == 0);
        for (int r = 1; r <= 3; ++r) {
            if (!rs::pc_peak_fits(s[0], s[1], s[2], r)) continue;
            const size_t w = 2 * r + 1;
            const size_t doubles = w * w * w + w * w + w * w + 3 * w + 6 * w;   // box, R, C, marginals, weights
            CHECK(rs::pce_pose_scratch_bytes(r) == 8 * doubles);
            CHECK(8 * doubles <= f.temp_bytes + f.ring_bytes);
            CHECK(rs::pce_pose_fits(f, r));
        }
    }
    const rs::PceFit small = rs::pce_fit(7, 7, 7);
    CHECK(small.temp_bytes + small.ring_bytes == 4312);
    CHECK(rs::pc_peak_fits(7, 7, 7, 3) && rs::pce_pose_fits(small, 3));
    CHECK(!rs::pce_pose_fits(small, 0) && !rs::pce_pose_fits(small, 4));
    // every shape the plan accepts holds the scratch of every radius whose box it holds
    for (int X = 7; X <= 64; X += 3)
        for (int Y = 7; Y <= 64; Y += 5)
            for (int TH = 7; TH <= 72; TH += 4) {
                const rs::PceFit f = rs::pce_fit(X, Y, TH);
                if (!f.fits) continue;
                for (int r = 1; r <= 3; ++r)
                    if (rs::pc_peak_fits(X, Y, TH, r)) CHECK(rs::pce_pose_fits(f, r));
            }
}

}  // namespace

int main() {
    static_assert(RS_PC_INJ_AT_PEAK == -1 && RS_PC_INJ_SAME_AS == -2, "the restatement's constants");
    const int B = 5, X = 21, Y = 19, TH = 36, n = 12;
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    const Inj ok0{0, 0, 3, 4, 5, 0.1}, peak5{1, 5, -1, 0, 0, 0.02}, same9{1, 9, -2, 1, 0, -0.5}, end{4, 12, 20, 18, 35, 1.0};
    // the empty list, n == 0, valid tables (the order across members is free)
    check_list({}, B, X, Y, TH, n);
    check_list({}, B, X, Y, TH, 0);
    check_list({{2, 0, -1, 0, 0, 1.0}, {2, 0, -2, 0, 7, 1.0}, {0, 0, 0, 0, 0, 1.0}}, B, X, Y, TH, 0);
    check_list({ok0, peak5, same9, end}, B, X, Y, TH, n);
    check_list({end, peak5, ok0, {1, 9, -2, 1, 0, 2.0}, {0, 3, -2, 2, 0, 1.0}}, B, X, Y, TH, n);
    check_list({ok0, ok0, peak5, peak5, same9, end, end}, B, X, Y, TH, n);
    check_list({{3, 12, -1, 0, 0, 1.0}, {2, 0, -1, 0, 0, 1.0}, {3, 12, -2, 0, 0, 1.0}, {2, 4, -2, 1, 0, 1.0}}, B, X, Y, TH, n);
    // every refusal at the first, a middle and the last place
    const std::vector<Inj> bad = {
        {-1, 1, 1, 1, 1, 1.0}, {5, 1, 1, 1, 1, 1.0}, {2147483647, 1, -1, 0, 0, 1.0},                    // a member outside [0, B)
        {1, -1, 1, 1, 1, 1.0}, {1, 13, 1, 1, 1, 1.0}, {1, 13, -1, 0, 0, 1.0},                           // a step outside [0, n]
        {1, 5, 21, 0, 0, 1.0}, {1, 5, -3, 0, 0, 1.0}, {1, 5, 0, 19, 0, 1.0}, {1, 5, 0, -1, 0, 1.0},     // a cell outside the grid
        {1, 5, 0, 0, 36, 1.0}, {1, 5, 0, 0, -1, 1.0},
        {1, 5, -2, -1, 0, 1.0}, {1, 5, -2, 9, 0, 1.0}, {1, 5, -2, 2147483647, 0, 1.0},                  // same-as no earlier one
        {1, 5, -2, 0, 0, 1.0},                                                                         // same-as of another member
        {1, 5, 1, 1, 1, inf}, {1, 5, -1, 0, 0, -inf}, {1, 5, 1, 1, 1, nan}, {1, 5, 1, 1, 1, 3.5e38},    // not a finite float32
        {1, 5, 1, 1, 1, -1e300}};
    for (const Inj& b : bad) {
        check_list({b}, B, X, Y, TH, n);
        check_list({ok0, peak5, b, same9, end}, B, X, Y, TH, n);
        check_list({ok0, peak5, {1, 5, 1, 2, 3, 1.0}, b}, B, X, Y, TH, n);
    }
    check_list({{1, 5, 1, 1, 1, 3.4028234e38}}, B, X, Y, TH, n);             // (valid: rounds to float32's largest value)
    check_list({{1, 5, 1, 1, 1, 3.40282356e38}}, B, X, Y, TH, n);            // (valid: below the midpoint)
    check_list({{1, 5, 1, 1, 1, 3.40282357e38}}, B, X, Y, TH, n);            // (rounds to infinity)
    check_list({{1, 5, -2, 0, 0, 1.0}}, B, X, Y, TH, n);                     // same-as itself
    check_list({ok0, {1, 5, -2, 1, 0, 1.0}}, B, X, Y, TH, n);
    check_list({peak5, {1, 5, -2, 0, 0, 1.0}}, B, X, Y, TH, n);              // (valid)
    // steps out of order within a member; another member's steps do not count
    check_list({peak5, {1, 4, 0, 0, 0, 1.0}}, B, X, Y, TH, n);
    check_list({peak5, ok0, {1, 4, 0, 0, 0, 1.0}, end}, B, X, Y, TH, n);
    check_list({ok0, end, {1, 11, -1, 0, 0, 1.0}, {4, 11, -1, 0, 0, 1.0}}, B, X, Y, TH, n);
    check_list({{1, 9, 0, 0, 0, 1.0}, {2, 3, 0, 0, 0, 1.0}, {0, 0, 0, 0, 0, 1.0}, {2, 3, -1, 0, 0, 1.0}}, B, X, Y, TH, n);   // (valid)
    // seeded lists: mostly valid entries, one kind of damage now and then
    std::mt19937 rng(20240917u);
    auto uni = [&](int lo, int hi) { return std::uniform_int_distribution<int>(lo, hi)(rng); };
    for (int t = 0; t < 4000; ++t) {
        const int gb = uni(1, 6), gx = uni(7, 40), gy = uni(7, 40), gth = uni(7, 40), steps = uni(0, 20), ni = uni(0, 14);
        std::vector<Inj> v;
        std::vector<int> st(gb, 0);
        for (int i = 0; i < ni; ++i) {
            const int m = uni(0, gb - 1);
            st[m] = std::min(steps, st[m] + (uni(0, 2) == 0 ? uni(0, 3) : 0));
            Inj e{m, st[m], uni(0, gx - 1), uni(0, gy - 1), uni(0, gth - 1), uni(-8, 8) / 16.0};
            const int kind = uni(0, 3);
            if (kind == 0) e.a = -1;
            if (kind == 1 && i > 0) {   // an earlier injection, of the same member more often than not
                e.a = -2, e.b = uni(0, i - 1);
                for (int k = i - 1; k >= 0 && uni(0, 3) != 0; --k)
                    if (v[k].member == m) {
                        e.b = k;
                        break;
                    }
            }
            switch (uni(0, 48)) {                                   // damage
            case 0: e.step = steps + uni(1, 3); break;
            case 1: e.step = -uni(1, 3); break;
            case 2: e.step = st[m] - 1; break;                     // (below the member's one before, or -1)
            case 3: e.a = gx + uni(0, 2), e.b = 0; break;
            case 4: e.a = 0, e.b = gy + uni(0, 2); break;
            case 5: e.a = 0, e.b = 0, e.c = gth + uni(0, 2); break;
            case 6: e.a = -2, e.b = i + uni(0, 2); break;
            case 7: e.a = -2, e.b = -uni(1, 3); break;
            case 8: e.a = -uni(3, 9); break;
            case 9: e.member = gb + uni(0, 2); break;
            case 10: e.member = -uni(1, 3); break;
            case 11: e.energy = uni(0, 1) ? inf : nan; break;
            case 12: e.energy = uni(0, 1) ? 1e39 : -3.5e38; break;
            default: break;
            }
            v.push_back(e);
        }
        check_list(v, gb, gx, gy, gth, steps);
    }
    check_scratch();
    std::printf("pce_inj: %ld checks, %ld failed\n", g_checks, g_failed);
    return g_failed ? 1 : 0;
}
