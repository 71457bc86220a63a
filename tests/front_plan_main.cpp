// Stand-alone host test of the fused front's launch rule (csrc/vt_plan.h: front_fused,
// front_grid): for every library of 1..2,000 template blocks the rule is "fused" exactly
// when one thread block covers the library (the wider rule, "or the query groups fill the
// resident thread blocks", measured slower where it applied and was taken out: the rule no
// longer reads the query count); and for every query count 1..20,000 the grid it launches,
// walked as vt_front_kernel walks it (block y serves groups y, y + grid.y, ...), serves every
// query group exactly once within the cap.  No GPU and no HIP header;
// tests/test_front_plan.py builds it with -fsanitize=address,undefined and runs it.
// Exit status 0: every check held.
#include <cstdio>
#include <vector>

#include "vt_plan.h"

namespace {

long g_checks = 0, g_failed = 0;
const char* g_case = "";

#define CHECK(cond)                                                                        \
    do {                                                                                   \
        ++g_checks;                                                                        \
        if (!(cond) && ++g_failed <= 20)                                                   \
            std::fprintf(stderr, "%s:%d: [%s] %s\n", __FILE__, __LINE__, g_case, #cond);   \
    } while (0)

constexpr int TB_PER_BLOCK = 16, Q_PER_GROUP = 4, CAP = 4096;   // the kernel's constants
constexpr int NTB_MAX = 2000, NQ_MAX = 20000;

// Groups of a query count, counted (not divided).
int groups_counted(int nq, int per) {
    int g = 0;
    for (int q = 0; q < nq; q += per) ++g;
    return g;
}

void test_front_fused() {
    for (int ntb = 1; ntb <= NTB_MAX; ++ntb) {
        int chunks = 0;   // chunks of TB_PER_BLOCK template blocks, counted
        for (int tb = 0; tb < ntb; tb += TB_PER_BLOCK) ++chunks;
        CHECK(vt_plan::front_fused(ntb, TB_PER_BLOCK) == (chunks == 1));
    }
    for (int per : {1, 4, 64})
        for (int ntb = 1; ntb <= 200; ++ntb) CHECK(vt_plan::front_fused(ntb, per) == (ntb <= per));
}

void test_front_grid(int cap, int nq_step) {
    std::vector<int> served;
    for (int nq = 1; nq <= NQ_MAX; nq += nq_step) {
        const vt_plan::Grid2 g = vt_plan::front_grid(nq, Q_PER_GROUP, cap);
        const int groups = groups_counted(nq, Q_PER_GROUP);
        CHECK(g.x == 1 && g.y >= 1 && g.y <= cap && g.y <= groups);
        served.assign((size_t)groups, 0);
        bool in_range = true;
        for (int y = 0; y < g.y; ++y)
            for (int q0 = y * Q_PER_GROUP; q0 < nq; q0 += g.y * Q_PER_GROUP) {   // the kernel's loop
                in_range = in_range && q0 / Q_PER_GROUP < groups;
                if (q0 / Q_PER_GROUP < groups) ++served[(size_t)(q0 / Q_PER_GROUP)];
            }
        CHECK(in_range);
        bool once = true;
        for (int v : served) once = once && v == 1;
        CHECK(once);
    }
}

}  // namespace

int main() {
    g_case = "front_fused";
    test_front_fused();
    // the shapes DESIGN names: the headline, the sharded library, the stress templates, the tests' 17 blocks
    g_case = "named shapes";
    CHECK(vt_plan::front_fused(16, TB_PER_BLOCK));
    CHECK(!vt_plan::front_fused(1563, TB_PER_BLOCK));
    CHECK(!vt_plan::front_fused(157, TB_PER_BLOCK));
    CHECK(!vt_plan::front_fused(17, TB_PER_BLOCK));
    g_case = "front_grid, the kernel's cap";
    test_front_grid(CAP, 1);
    g_case = "front_grid, other caps";
    for (int cap : {1, 3, 64, 4999, 5000}) test_front_grid(cap, 53);
    g_case = "front_grid, two groups per block";
    CHECK(vt_plan::front_grid(16388, Q_PER_GROUP, CAP).y == CAP);
    CHECK(vt_plan::front_grid(16384, Q_PER_GROUP, CAP).y == CAP);
    CHECK(vt_plan::front_grid(16380, Q_PER_GROUP, CAP).y == CAP - 1);
    std::printf("front_plan: %ld checks, %ld failed\n", g_checks, g_failed);
    return g_failed ? 1 : 0;
}
