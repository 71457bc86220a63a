// Stand-alone host test of pce_plan.h: the pose-cell ensemble's LDS plan, its control record
// and the split of a run into launches, each against the test's own restatement.  No GPU and
// no HIP header; tests/test_pce_plan.py builds it with -fsanitize=address,undefined and runs
// it.  Exit status 0: every check held.
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "pce_plan.h"

namespace {

long g_checks = 0, g_failed = 0;
const char* g_case = "";

#define CHECK(cond)                                                                        \
    do {                                                                                   \
        ++g_checks;                                                                        \
        if (!(cond) && ++g_failed <= 20)                                                   \
            std::fprintf(stderr, "%s:%d: [%s] %s\n", __FILE__, __LINE__, g_case, #cond);   \
    } while (0)

struct Region {
    size_t off, bytes;
};

void check_fit(int X, int Y, int TH, bool expect) {
    const rs::PceFit f = rs::pce_fit(X, Y, TH);
    CHECK(f.fits == expect);
    if (!f.fits) return;
    // temp and ring are one contiguous scratch; every region lies inside the total and
    // no two overlap
    const Region r[] = {{f.red_off, f.red_bytes},   {f.state_off, f.state_bytes}, {f.temp_off, f.temp_bytes},
                        {f.ring_off, f.ring_bytes}, {f.filt_off, f.filt_bytes},   {f.ctl_off, f.ctl_bytes}};
    const int nr = (int)(sizeof(r) / sizeof(r[0]));
    for (int i = 0; i < nr; ++i) {
        CHECK(r[i].bytes > 0);
        CHECK(r[i].off % 4 == 0);
        CHECK(r[i].off + r[i].bytes <= f.total);
        for (int j = i + 1; j < nr; ++j)
            CHECK(r[i].off + r[i].bytes <= r[j].off || r[j].off + r[j].bytes <= r[i].off);
    }
    CHECK(f.total <= rs::PCE_LDS_BYTES);
    CHECK(f.red_off % 8 == 0 && f.red_bytes >= 16 * 8 + 16 * 8);
    CHECK(f.ring_off == f.temp_off + f.temp_bytes);
    CHECK(f.TP >= TH && f.TP % 2 == 1);
    CHECK(f.PS == Y * TH);
    CHECK(f.state_bytes >= 4 * (size_t)X * Y * f.TP);
    CHECK(f.temp_bytes == 8 * (size_t)f.PS);
    CHECK(f.ring_bytes == 8 * (size_t)f.PS * 10);
    CHECK(f.ctl_bytes >= 2 * rs::pce_rec_bytes(TH));
    CHECK(f.filt_bytes >= 4u * rs::PCE_MAX_FILTERS * 49);
    // the path scratch holds path_layers layers
    CHECK(f.path_layers >= 1 && f.path_layers <= TH);
    CHECK(4 * (size_t)f.path_layers * X * Y <= f.temp_bytes + f.ring_bytes);
}

// v mod n in [0, n) by stepping (no % on negatives)
int mod_steps(long v, int n) {
    while (v < 0) v += n;
    while (v >= n) v -= n;
    return (int)v;
}

void check_records(std::mt19937& rng, int X, int Y, int TH) {
    auto uni = [&](int lo, int hi) { return std::uniform_int_distribution<int>(lo, hi)(rng); };
    const size_t rb = rs::pce_rec_bytes(TH);
    CHECK(rb % 16 == 0 && rb >= 32 + 5 * (size_t)TH);
    CHECK(rs::pce_rec_ox(TH) >= 28 && rs::pce_rec_oy(TH) >= rs::pce_rec_ox(TH) + 2 * (size_t)TH);
    CHECK(rs::pce_rec_fi(TH) >= rs::pce_rec_oy(TH) + 2 * (size_t)TH && rs::pce_rec_fi(TH) + TH <= rb);
    for (int rep = 0; rep < 50; ++rep) {
        std::vector<int32_t> ox(TH), oy(TH), fi(TH), rx(TH), ry(TH), rf(TH);
        double zf[7];
        float zr[7];
        for (int k = 0; k < TH; ++k) {
            ox[k] = uni(-3 * X, 3 * X);
            oy[k] = uni(-3 * Y, 3 * Y);
            fi[k] = uni(0, 255);
        }
        for (double& z : zf) z = std::uniform_real_distribution<double>(-1.0, 1.0)(rng);
        // exactly rb bytes, so that the sanitizer sees any write past the record
        std::vector<unsigned char> rec(rb, 0xAB);
        rs::pce_pack(X, Y, TH, ox.data(), oy.data(), fi.data(), zf, rec.data());
        rs::pce_unpack(TH, rec.data(), rx.data(), ry.data(), rf.data(), zr);
        for (int k = 0; k < TH; ++k) {
            CHECK(rx[k] == mod_steps(ox[k], X) && rx[k] == ((ox[k] % X) + X) % X);
            CHECK(ry[k] == mod_steps(oy[k], Y) && ry[k] == ((oy[k] % Y) + Y) % Y);
            CHECK(rf[k] == fi[k]);
        }
        for (int t = 0; t < 7; ++t) CHECK(zr[t] == (float)zf[t]);
    }
}

void check_chunks(int K) {
    const int ns[] = {0, 1, K - 1, K, K + 1, 3 * K + 2};
    for (int n : ns) {
        if (n < 0) continue;
        std::vector<int> seen((size_t)n, 0);
        const int nc = rs::pce_chunk_count(n, K);
        CHECK(nc == (n + K - 1) / K);
        int expect_first = 0;
        for (int c = 0; c < nc; ++c) {
            int first = -1, count = -1;
            rs::pce_chunk(n, K, c, &first, &count);
            CHECK(first == expect_first && count >= 1 && count <= K && first + count <= n);
            for (int s = first; s < first + count && s < n; ++s) ++seen[(size_t)s];
            expect_first = first + count;
        }
        CHECK(expect_first == n);
        for (int s = 0; s < n; ++s) CHECK(seen[(size_t)s] == 1);
    }
}

}  // namespace

int main() {
    g_case = "fit";
    const int fit_shapes[][3] = {{21, 21, 36}, {32, 32, 18}, {8, 8, 8}, {12, 9, 10}, {50, 50, 10}, {7, 7, 7}, {9, 30, 11}};
    for (const auto& s : fit_shapes) check_fit(s[0], s[1], s[2], true);
    const int no_shapes[][3] = {{64, 64, 36}, {6, 8, 8}, {8, 6, 8}, {8, 8, 6}, {0, 8, 8}, {-1, 8, 8}, {400, 7, 7}, {40000, 7, 7}};
    for (const auto& s : no_shapes) check_fit(s[0], s[1], s[2], false);
    // every shape of a sweep: the plan is consistent wherever it says it fits
    for (int X = 5; X <= 70; X += 5)
        for (int Y = 7; Y <= 70; Y += 9)
            for (int TH = 7; TH <= 48; TH += 7) {
                const rs::PceFit f = rs::pce_fit(X, Y, TH);
                check_fit(X, Y, TH, f.fits);
                if (X < 7) CHECK(!f.fits);
            }

    g_case = "shift";
    for (int n : {7, 8, 21, 32, 50})
        for (int o = -3 * n; o <= 3 * n; ++o) {
            const int r = rs::pce_reduce_shift(o, n);
            CHECK(r >= 0 && r < n && r == ((o % n) + n) % n && r == mod_steps(o, n));
        }
    CHECK(rs::pce_reduce_shift(INT32_MIN, 21) == mod_steps((long)INT32_MIN, 21));
    CHECK(rs::pce_reduce_shift(INT32_MAX, 21) == mod_steps((long)INT32_MAX, 21));

    g_case = "record";
    std::mt19937 rng(12345);
    check_records(rng, 21, 21, 36);
    check_records(rng, 32, 32, 18);
    check_records(rng, 8, 8, 8);
    check_records(rng, 12, 9, 10);
    check_records(rng, 50, 50, 10);
    check_records(rng, 9, 30, 11);

    g_case = "chunk";
    for (int K : {1, 2, 4, 7, 146, 585}) check_chunks(K);
    // the default length keeps a launch's records within the budget, one step at least
    for (int B : {1, 32, 256, 1024, 100000})
        for (int TH : {7, 10, 18, 36}) {
            const int K = rs::pce_chunk_len(B, TH, 0);
            CHECK(K >= 1);
            CHECK(K == 1 || (size_t)K * B * rs::pce_rec_bytes(TH) <= rs::PCE_CTL_BUDGET);
            CHECK((size_t)(K + 1) * B * rs::pce_rec_bytes(TH) > rs::PCE_CTL_BUDGET || K == (1 << 20));
            CHECK(rs::pce_chunk_len(B, TH, 4) == 4);
        }

    std::printf("pce_plan: %ld checks, %ld failed\n", g_checks, g_failed);
    return g_failed ? 1 : 0;
}
