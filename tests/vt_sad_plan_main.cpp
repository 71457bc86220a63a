// Stand-alone host test of the true-SAD metric's rules in vt_plan.h (metric_known, sad_fast,
// sad_form, sad_waves, sad_split), each against a brute-force restatement: the fast form's
// grid is replayed block by block and every (template block, query group, dword column) must
// be served exactly once.  No GPU and no HIP header; tests/test_vt_sad.py builds it with
// -fsanitize=address,undefined and runs it.  Exit status 0: every check held.
#include <cstdio>
#include <cstring>
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

void test_metric_codes() {
    g_case = "metric_known";
    for (int m = -3; m <= 5; ++m) CHECK(vt_plan::metric_known(m) == (m == 0 || m == 1));
    CHECK(vt_plan::METRIC_WRAPPED == 0 && vt_plan::METRIC_SAD == 1);
}

void test_form() {
    g_case = "sad_fast / sad_form";
    for (int H = 1; H <= 130; ++H)
        for (int M = 1; M <= 16; ++M) {
            bool fast = false;   // the kernel's instances, listed
            if (M == 8 && H == 32) fast = true;
            if (M == 8 && H == 64) fast = true;
            CHECK(vt_plan::sad_fast(H, M) == fast);
            CHECK(std::strcmp(vt_plan::sad_form(H, M), fast ? "sad" : "sad-generic") == 0);
            // the fast form's window is never empty and H is whole chunks of 4 rows
            if (vt_plan::sad_fast(H, M)) CHECK(H > 2 * M && H % 4 == 0);
        }
}

// Replay the fast form's launch: ntb * nqc blocks of sad_waves(WD) waves; block (tb, j) walks
// the groups j, j + nqc, ..; wave w of it the columns w, w + nw, ...
void test_grid() {
    g_case = "sad_split / sad_waves";
    for (const int ntb : {1, 2, 3, 16, 157, 1024, 1025, 5000})
        for (const int nq : {1, 3, 4, 5, 9, 37, 256, 1024, 4099})
            for (const int WD : {1, 5, 8, 9, 12, 17}) {
                const int ngroups = (nq + vt_plan::SAD_NQ - 1) / vt_plan::SAD_NQ;
                const int nqc = vt_plan::sad_split(ntb, ngroups), nw = vt_plan::sad_waves(WD);
                CHECK(nqc >= 1 && nqc <= ngroups);
                CHECK(nw >= 1 && nw <= vt_plan::SAD_NW && nw <= WD && 64 * nw <= 1024);
                // the rule by brute force: the most blocks per template block that neither pass the
                // target with one to spare nor leave a block (the last has the fewest) short of groups
                int brute = 1;
                for (int n = 2; n <= ngroups; ++n) {
                    if ((long)ntb * (n - 1) >= vt_plan::SAD_TARGET_BLOCKS) break;
                    int fewest = 0;
                    for (int g = n - 1; g < ngroups; g += n) ++fewest;
                    if (fewest >= vt_plan::SAD_MIN_GROUPS) brute = n;
                }
                CHECK(nqc == brute);
                if (ntb > 16 && ntb != 157) continue;   // (the replay below is per template block: a few suffice)
                std::vector<int> served((size_t)ngroups * WD, 0);
                int maxq = -1;
                for (int j = 0; j < nqc; ++j)
                    for (int g = j; g < ngroups; g += nqc)
                        for (int w = 0; w < nw; ++w)
                            for (int c = w; c < WD; c += nw) {
                                ++served[(size_t)g * WD + c];
                                for (int n = 0; n < vt_plan::SAD_NQ; ++n) {   // the clamp of the tail queries
                                    const int qi = g * vt_plan::SAD_NQ + n < nq ? g * vt_plan::SAD_NQ + n : nq - 1;
                                    CHECK(qi >= 0 && qi < nq);
                                    maxq = qi > maxq ? qi : maxq;
                                }
                            }
                bool once = true;
                for (const int s : served) once = once && s == 1;
                CHECK(once);
                CHECK(maxq == nq - 1);
            }
}

}  // namespace

int main() {
    test_metric_codes();
    test_form();
    test_grid();
    std::printf("vt_sad_plan: %ld checks, %ld failed\n", g_checks, g_failed);
    return g_failed ? 1 : 0;
}
