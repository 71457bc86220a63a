// Stand-alone host test of the row-offset rule (csrc/vt_offset_rule.h): the per-dword terms,
// the first-argmin pick and vto_profile_host against a byte-by-byte restatement, on heap
// blocks of exactly H * W bytes, so that a read past a row that is not dword-aligned
// (W mod 4 != 0, the last row at the end of its block) is an AddressSanitizer report.  No GPU
// and no HIP header; tests/test_vt_offset.py builds it with -fsanitize=address,undefined and
// runs it.  Exit status 0: every check held.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "vt_offset_rule.h"

namespace {

long g_checks = 0, g_failed = 0;
const char* g_case = "";

#define CHECK(cond)                                                                        \
    do {                                                                                   \
        ++g_checks;                                                                        \
        if (!(cond) && ++g_failed <= 20)                                                   \
            std::fprintf(stderr, "%s:%d: [%s] %s\n", __FILE__, __LINE__, g_case, #cond);   \
    } while (0)

uint32_t g_rng = 12345u;
uint32_t rnd() {
    g_rng = g_rng * 1664525u + 1013904223u;
    return g_rng >> 8;
}

// an image in a heap block of exactly H * W bytes
std::unique_ptr<uint8_t[]> image(int H, int W, int kind) {
    std::unique_ptr<uint8_t[]> p(new uint8_t[(size_t)H * W]);
    for (int i = 0; i < H * W; ++i)
        p[i] = kind == 0 ? (uint8_t)rnd() : kind == 1 ? 0 : kind == 2 ? 255 : (rnd() & 1 ? 255 : 0);
    return p;
}

uint32_t byte_term(int metric, int t, int q) {
    return metric == rs::VTO_METRIC_SAD ? (uint32_t)std::abs(t - q) : (uint32_t)((t - q) & 255);
}

// the rule byte by byte
int brute(int metric, int H, int W, int M, const uint8_t* T, const uint8_t* Q, std::vector<uint32_t>& prof) {
    prof.assign((size_t)(2 * M - 1), 0u);
    int best_k = 0;
    for (int k = 0; k < 2 * M - 1; ++k) {
        const int o = k - (M - 1);
        uint64_t s = 0;
        for (int r = M; r < H - M; ++r)
            for (int c = 0; c < W; ++c) s += byte_term(metric, T[(size_t)(r + o) * W + c], Q[(size_t)r * W + c]);
        prof[(size_t)k] = (uint32_t)s;
        if (prof[(size_t)k] < prof[(size_t)best_k]) best_k = k;
    }
    return best_k - (M - 1);
}

void test_terms() {
    g_case = "dword terms";
    const uint32_t edge[] = {0u, 0xFFFFFFFFu, 0x80808080u, 0x7F7F7F7Fu, 0x01010101u, 0x00FF00FFu, 0xFF00FF00u,
                             0x807F0100u, 0x0001FF80u};
    std::vector<uint32_t> vals(edge, edge + sizeof(edge) / sizeof(edge[0]));
    for (int i = 0; i < 200; ++i) vals.push_back((rnd() << 8) ^ rnd());
    for (uint32_t t : vals)
        for (uint32_t q : vals) {
            uint32_t sad = 7u, wr = 11u, sub = 0u;
            for (int b = 0; b < 4; ++b) {
                const int tb = (t >> (8 * b)) & 255, qb = (q >> (8 * b)) & 255;
                sad += byte_term(rs::VTO_METRIC_SAD, tb, qb);
                wr += byte_term(rs::VTO_METRIC_WRAPPED, tb, qb);
                sub |= (uint32_t)((tb - qb) & 255) << (8 * b);
            }
            CHECK(rs::vto_bytes_sub(t, q) == sub);
            CHECK(rs::vto_term_sad(t, q, 7u) == sad);
            CHECK(rs::vto_term_wrapped(t, q, 11u) == wr);
            CHECK(rs::vto_term<rs::VTO_METRIC_SAD>(t, q, 7u) == sad);
            CHECK(rs::vto_term<rs::VTO_METRIC_WRAPPED>(t, q, 11u) == wr);
        }
    CHECK(rs::vto_term_sad(0u, 0u, 5u) == 5u && rs::vto_term_wrapped(0u, 0u, 5u) == 5u);   // padding adds nothing
}

void test_pick() {
    g_case = "first argmin";
    const uint32_t a[5] = {4, 2, 2, 9, 2};
    CHECK(rs::vto_first_argmin(a, 3) == 1 - 2);
    const uint32_t flat[15] = {0};
    CHECK(rs::vto_first_argmin(flat, 8) == -7);
    const uint32_t top[3] = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFEu};
    CHECK(rs::vto_first_argmin(top, 2) == 1);
    const uint32_t one[1] = {3};
    CHECK(rs::vto_first_argmin(one, 1) == 0);
}

void test_row_dword() {
    g_case = "row dword";
    for (int W = 1; W <= 9; ++W) {
        std::unique_ptr<uint8_t[]> row(new uint8_t[(size_t)W]);   // exactly one row
        for (int i = 0; i < W; ++i) row[i] = (uint8_t)(0x11 * (i + 1));
        for (int c = 0; c < (W + 3) / 4; ++c) {
            uint32_t want = 0;
            for (int b = 0; b < 4; ++b)
                if (4 * c + b < W) want |= (uint32_t)row[4 * c + b] << (8 * b);
            CHECK(rs::vto_row_dword(row.get(), W, c) == want);
        }
    }
}

void test_profiles() {
    const int shapes[][3] = {{64, 32, 8}, {32, 32, 8}, {64, 48, 8}, {24, 10, 8}, {16, 5, 8}, {10, 7, 3},
                             {18, 1, 8}, {7, 3, 1}, {20, 6, 10}};
    for (const auto& sh : shapes) {
        const int H = sh[0], W = sh[1], M = sh[2];
        static char name[64];
        std::snprintf(name, sizeof name, "profile %dx%d M=%d", H, W, M);
        g_case = name;
        for (int metric = 0; metric < 2; ++metric)
            for (int kind = 0; kind < 4; ++kind) {
                const auto T = image(H, W, kind);
                for (int qk = 0; qk < 4; ++qk) {
                    const auto Q = image(H, W, qk);
                    std::vector<uint32_t> want, got((size_t)(2 * M - 1), 0xDEADBEEFu);
                    const int wo = brute(metric, H, W, M, T.get(), Q.get(), want);
                    const int go = rs::vto_profile_host(metric, H, W, M, T.get(), Q.get(), got.data());
                    CHECK(go == wo);
                    CHECK(got == want);
                    if (H == 2 * M) CHECK(go == -(M - 1) && got == std::vector<uint32_t>((size_t)(2 * M - 1), 0u));
                }
                // the template rolled by every offset: an exact zero at it
                for (int o = -(M - 1); o <= M - 1 && kind == 0 && H > 2 * M; ++o) {
                    std::unique_ptr<uint8_t[]> Q(new uint8_t[(size_t)H * W]);
                    for (int r = 0; r < H; ++r)
                        std::memcpy(Q.get() + (size_t)r * W, T.get() + (size_t)(((r + o) % H + H) % H) * W, (size_t)W);
                    std::vector<uint32_t> got((size_t)(2 * M - 1));
                    const int go = rs::vto_profile_host(metric, H, W, M, T.get(), Q.get(), got.data());
                    CHECK(got[(size_t)(o + M - 1)] == 0u);
                    CHECK(go <= o);   // (an earlier offset can tie only with another exact zero)
                    CHECK(got[(size_t)(go + M - 1)] == 0u);
                }
            }
    }
}

}  // namespace

int main() {
    test_terms();
    test_pick();
    test_row_dword();
    test_profiles();
    std::printf("%ld checks, %ld failed\n", g_checks, g_failed);
    return g_failed ? 1 : 0;
}
