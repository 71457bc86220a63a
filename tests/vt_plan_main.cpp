// Stand-alone host test of vt_plan.h: what the view-template matcher's host side decides
// before it launches (local counts, the plane scan's split, the prune predicate, the
// prefilter and export grids, the folded-keys decision, rs_vt_match_stream's path and its
// upload groups), each against an independent restatement -- by brute force where there is
// one -- of the rule as view_templates.hip wrote it out before the header existed.  No GPU
// and no HIP header; tests/test_vt_plan.py builds it with -fsanitize=address,undefined and
// runs it.  Exit status 0: every check held.
#include <cstdint>
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

int imin(int a, int b) { return a < b ? a : b; }
int imax(int a, int b) { return a > b ? a : b; }

// Template g lives on rank g % nranks: count them.
void test_local_count() {
    g_case = "local_count_of";
    for (int nranks = 1; nranks <= 8; ++nranks)
        for (int64_t count = 0; count <= 100; ++count) {
            int64_t sum = 0;
            for (int rank = 0; rank < nranks; ++rank) {
                int64_t mine = 0;
                for (int64_t g = 0; g < count; ++g) mine += g % nranks == rank;
                CHECK(vt_plan::local_count_of(rank, nranks, count) == mine);
                sum += vt_plan::local_count_of(rank, nranks, count);
            }
            CHECK(sum == count);
        }
}

// The split as the scan launch computed it, transcribed.
int split_transcribed(int ntb, int nbatch, int slots, bool set, int k) {
    int nqc;
    if (set) {
        nqc = imax(1, k);
    } else {
        const int fill = (slots + ntb - 1) / ntb;
        nqc = imax(32, imin(4 * fill, imax(128, fill)));
    }
    nqc = imin(nqc, imax(1, nbatch));
    if (nqc >= 8) nqc &= ~7;
    return nqc;
}

void test_plane_split() {
    g_case = "plane_split";
    for (const int ntb : {1, 2, 16, 196, 1563})
        for (const int nbatch : {1, 7, 8, 33, 256})
            for (const int slots : {256, 1024}) {
                const int nqc = vt_plan::plane_split(ntb, nbatch, slots, 0);
                CHECK(nqc >= 1 && nqc <= imax(1, nbatch));
                CHECK(nqc < 8 || nqc % 8 == 0);
                CHECK(nqc == split_transcribed(ntb, nbatch, slots, false, 0));
                for (const int k : {1, 2, 7, 8, 9, 31, 32, 100, 1000}) {
                    const int o = vt_plan::plane_split(ntb, nbatch, slots, k);
                    int want = imin(imax(1, k), imax(1, nbatch));
                    if (want >= 8) want -= want % 8;
                    CHECK(o == want);
                    CHECK(o == split_transcribed(ntb, nbatch, slots, true, k));
                }
            }
    CHECK(vt_plan::plane_split(16, 0, 1024, 0) == 1);   // no batch: still one block
    // spot values of the model: one round of 1,024 slots over 16 template blocks is 64
    // blocks each, and up to four rounds but no more than 128 blocks are taken; over
    // 1,563 template blocks a round is one block each, and the split stays at 32
    CHECK(vt_plan::plane_split(16, 256, 1024, 0) == 128);
    CHECK(vt_plan::plane_split(1563, 256, 1024, 0) == 32);
}

void test_prunes() {
    g_case = "prunes";
    CHECK(vt_plan::VT_PRUNE_MIN_Q == 512);
    for (const int H : {32, 64})
        for (const int cand : {0, 1})
            for (const int64_t tb0 : {0, 1})
                for (const int forms : {0, 1})
                    for (const int64_t ntb : {1, 2, 65535, 65536})
                        for (const int prune : {0, 1, 2})
                            for (const int nq : {511, 512}) {
                                // the truth table, condition by condition
                                bool want = true;
                                if (H != 64) want = false;
                                if (cand) want = false;
                                if (tb0 != 0) want = false;
                                if (!forms) want = false;
                                if (ntb > 65535) want = false;
                                if (prune == 0) want = false;
                                if (prune == 1 && (nq < 512 || ntb < 2)) want = false;
                                CHECK(vt_plan::prunes(H, cand != 0, tb0, forms != 0, ntb, prune, nq) == want);
                            }
}

void test_prefilter_grid() {
    g_case = "prefilter_grid";
    const int PF_NB = 4;   // queries per staged batch, as the kernel's loop steps
    for (const int tbpb : {4, 8, 16})
        for (const int cap : {1, 64, 1024, 4096})
            for (const int ntb : {1, 2, 15, 16, 17, 196, 1563, 65535})
                for (const int nq : {1, 3, 4, 5, 511, 512, 1024, 10240, 40000}) {
                    const vt_plan::Grid2 g = vt_plan::prefilter_grid(ntb, nq, tbpb, PF_NB, cap);
                    CHECK(g.x >= 1 && (int64_t)g.x * tbpb >= ntb && (int64_t)(g.x - 1) * tbpb < ntb);
                    CHECK(g.y >= 1);
                    CHECK((int64_t)g.x * g.y <= imax(cap, g.x));
                    CHECK(g.y <= (nq + PF_NB - 1) / PF_NB);   // no block without a batch
                    // the kernel's loop over block rows y: every query batch exactly once
                    std::vector<int> seen((size_t)(nq + PF_NB - 1) / PF_NB, 0);
                    for (int y = 0; y < g.y; ++y)
                        for (int q0 = y * PF_NB; q0 < nq; q0 += g.y * PF_NB) ++seen[(size_t)q0 / PF_NB];
                    bool once = true;
                    for (const int s : seen) once = once && s == 1;
                    CHECK(once);
                }
    // the shipped geometry at the headline shape: 16 template blocks a thread block, cap 4096
    const vt_plan::Grid2 h = vt_plan::prefilter_grid(157, 10240, 16, 4, 4096);
    CHECK(h.x == 10 && h.y == 409);
}

void test_export_grid() {
    g_case = "export_grid";
    CHECK(vt_plan::VT_EXPORT_BLOCKS == 64 && vt_plan::VT_EXPORT_BLOCKS_STREAM == 256);
    for (const int cap : {vt_plan::VT_EXPORT_BLOCKS, vt_plan::VT_EXPORT_BLOCKS_STREAM})
        for (const int64_t n : {(int64_t)1, (int64_t)255, (int64_t)256, (int64_t)257, (int64_t)16384, (int64_t)16385,
                                (int64_t)65536, (int64_t)65537, (int64_t)1 << 20, (int64_t)INT32_MAX}) {
            const int g = vt_plan::export_grid(n, cap);
            CHECK(g >= 1 && g <= cap);
            int64_t blocks = 0;   // blocks of 256 that cover n, counted
            while (blocks * 256 < n) ++blocks;
            CHECK(g == (blocks < cap ? blocks : cap));
        }
}

void test_small_rules() {
    g_case = "zero copy, poll, fold";
    CHECK(vt_plan::VT_ZC_MAX == 64 && vt_plan::VT_POLL_MAX == 4096);
    for (const int planar : {0, 1})
        for (const int on : {0, 1})
            for (const int nq : {1, 64, 65, 4096, 4097}) {
                CHECK(vt_plan::stages_in_place(planar, nq, on) == (planar && on && nq <= 64));
                for (const int timed : {0, 1}) {
                    CHECK(vt_plan::polls_keys(on, timed, nq) == (on && !timed && nq <= 4096));
                    for (const int fold_ok : {0, 1})
                        for (const int64_t lc : {0, 1})
                            CHECK(vt_plan::folds_keys(fold_ok, planar, lc, on, timed, nq) ==
                                  (fold_ok && planar && lc > 0 && on && !timed && nq <= 4096));
                }
            }
}

void test_stream_path() {
    g_case = "stream_path";
    using vt_plan::StreamPath;
    for (const int dev : {0, 1})
        for (const int planar : {0, 1})
            for (const int nb : {1, 2, 3, 40}) {
                // the two booleans the stream call tested before the enum
                const bool hostgroups = !dev && planar;
                const bool allplanes = (dev && planar && nb > 1) || hostgroups;
                const StreamPath want = hostgroups ? StreamPath::HostGroups
                                        : allplanes ? StreamPath::Fused
                                                    : StreamPath::PerBatch;
                CHECK(vt_plan::stream_path(dev, planar, nb) == want);
            }
}

void test_host_groups() {
    g_case = "host_groups";
    CHECK(vt_plan::VT_UP_GROUP == 16);
    for (int nb = 1; nb <= 200; ++nb) {
        const vt_plan::HostGroups plan = vt_plan::host_groups(nb);
        // gb = min(nb, max(2, min(16, (nb - 1) / 3))), by search: the largest value that
        // is at most nb and at most max(2, min(16, (nb - 1) / 3))
        int third = 0;
        while (3 * (third + 1) <= nb - 1) ++third;
        int gb = nb;
        for (int v = nb; v >= 1; --v)
            if (v <= imax(2, imin(16, third))) { gb = v; break; }
        CHECK(plan.gb == gb);
        CHECK(nb < 2 || (plan.gb >= 2 && plan.gb <= 16));
        CHECK((plan.first == 1) == (nb >= 4 || plan.gb == 1));
        CHECK(nb >= 4 ? plan.first == 1 : plan.first == plan.gb);
        // the groups as the upload loop walked them
        std::vector<int> sizes;
        for (int g = 0, b0 = 0, n = 0; b0 < nb; ++g, b0 += n) {
            n = imin(g == 0 ? (nb >= 4 ? 1 : gb) : gb, nb - b0);
            const vt_plan::HostGroup grp = plan.group(g);
            CHECK(grp.b0 == b0 && grp.n == n);   // contiguous, in order
            CHECK(grp.n >= 1 && grp.n <= plan.gb);   // (a group fits an upload buffer of gb batches)
            CHECK(grp.buf == g % 2);
            CHECK(grp.waits == (g >= 2));
            sizes.push_back(grp.n);
        }
        const int ng = (int)sizes.size();
        CHECK(plan.group(ng).n == 0 && plan.group(ng + 1).n == 0);   // past the last: empty
        int covered = 0;
        for (int g = 0; g < ng; ++g) {
            covered += sizes[(size_t)g];
            if (g > 0 && g < ng - 1) CHECK(sizes[(size_t)g] == gb);
        }
        CHECK(covered == nb);
    }
    auto sizes_of = [](int nb) {
        std::vector<int> s;
        const vt_plan::HostGroups plan = vt_plan::host_groups(nb);
        for (int g = 0; plan.group(g).n > 0; ++g) s.push_back(plan.group(g).n);
        return s;
    };
    CHECK((sizes_of(10) == std::vector<int>{1, 3, 3, 3}));
    CHECK((sizes_of(40) == std::vector<int>{1, 13, 13, 13}));
    CHECK((sizes_of(17) == std::vector<int>{1, 5, 5, 5, 1}));
    CHECK((sizes_of(1) == std::vector<int>{1}));
    CHECK((sizes_of(3) == std::vector<int>{2, 1}));
    CHECK((sizes_of(200) == std::vector<int>{1, 16, 16, 16, 16, 16, 16, 16, 16, 16, 16, 16, 16, 7}));
}

}  // namespace

int main() {
    test_local_count();
    test_plane_split();
    test_prunes();
    test_prefilter_grid();
    test_export_grid();
    test_small_rules();
    test_stream_path();
    test_host_groups();
    std::printf("%ld checks, %ld failed\n", g_checks, g_failed);
    return g_failed == 0 ? 0 : 1;
}
