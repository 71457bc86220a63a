// Stand-alone host test of the patch-normalisation rule (csrc/vt_norm_rule.h): vtn_isqrt at
// and around every kind of boundary, vtn_pixel's clamps, and vtn_normalise_host against a
// direct per-pixel restatement in 64-bit integers, with source and destination in heap blocks
// of exactly H * W bytes, so that a read or write past an image whose rows are not
// dword-aligned (W mod 4 != 0) is an AddressSanitizer report.  No GPU and no HIP header;
// tests/test_vt_norm.py builds it with -fsanitize=address,undefined and runs it.  Exit status
// 0: every check held.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <memory>

#include "vt_norm_rule.h"

namespace {

long g_checks = 0, g_failed = 0;
const char* g_case = "";

#define CHECK(cond)                                                                        \
    do {                                                                                   \
        ++g_checks;                                                                        \
        if (!(cond) && ++g_failed <= 20)                                                   \
            std::fprintf(stderr, "%s:%d: [%s] %s\n", __FILE__, __LINE__, g_case, #cond);   \
    } while (0)

uint32_t g_rng = 2463534242u;
uint32_t rnd() {
    g_rng = g_rng * 1664525u + 1013904223u;
    return g_rng >> 8;
}

// an image in a heap block of exactly H * W bytes
std::unique_ptr<uint8_t[]> image(int H, int W, int kind) {
    std::unique_ptr<uint8_t[]> p(new uint8_t[(size_t)H * W]);
    for (int r = 0; r < H; ++r)
        for (int c = 0; c < W; ++c)
            p[(size_t)r * W + c] = kind == 0   ? (uint8_t)rnd()
                                   : kind == 1 ? 77
                                   : kind == 2 ? ((r + c) & 1 ? 255 : 0)
                                   : kind == 3 ? (c & 1 ? 255 : 0)
                                               : (uint8_t)(100 + rnd() % 3);
    return p;
}

uint64_t isqrt64(uint64_t d) {
    uint64_t s = 0;
    while ((s + 1) * (s + 1) <= d) ++s;
    return s;
}

// the rule at one pixel, the window walked directly, 64-bit signed integers
uint8_t brute(int H, int W, int R, int G, const uint8_t* p, int r, int c) {
    int64_t n = 0, S = 0, S2 = 0;
    for (int y = r - R; y <= r + R; ++y)
        for (int x = c - R; x <= c + R; ++x) {
            if (y < 0 || y >= H || x < 0 || x >= W) continue;
            const int64_t v = p[(size_t)y * W + x];
            ++n;
            S += v;
            S2 += v * v;
        }
    const int64_t D = n * S2 - S * S, N = n * p[(size_t)r * W + c] - S;
    // the header's root, accepted only where the defining inequality holds in 64 bits
    const int64_t s = (int64_t)rs::vtn_isqrt((uint32_t)D);
    CHECK(D >= 0 && s * s <= D && D < (s + 1) * (s + 1));
    if (s == 0) return 128;
    const int64_t q = (G * (N < 0 ? -N : N) + s / 2) / s;
    const int64_t o = N < 0 ? 128 - q : 128 + q;
    return (uint8_t)(o < 0 ? 0 : o > 255 ? 255 : o);
}

void test_isqrt() {
    g_case = "isqrt";
    for (uint32_t d = 0; d < 70000u; ++d) CHECK(rs::vtn_isqrt(d) == (uint32_t)isqrt64(d));
    for (uint32_t s = 1; s <= 65535u; s += (s < 300u ? 1u : 97u)) {   // around every square
        const uint32_t sq = s * s;
        CHECK(rs::vtn_isqrt(sq) == s);
        CHECK(rs::vtn_isqrt(sq - 1u) == s - 1u);
        if (s < 65535u) CHECK(rs::vtn_isqrt(sq + 2u * s) == s);   // (s + 1)^2 - 1
    }
    CHECK(rs::vtn_isqrt(65535u * 65535u) == 65535u);
    CHECK(rs::vtn_isqrt(0xFFFFFFFFu) == 65535u);    // the float estimate rounds to 65536 here
    CHECK(rs::vtn_isqrt(0xFFFE0000u) == 65534u);    // 65535^2 - 1
    CHECK(rs::vtn_isqrt(3291890625u) == 57375u);    // the largest n * S2: (225 * 255)^2
    for (int i = 0; i < 200000; ++i) {
        const uint32_t d = (rnd() << 8) ^ rnd();
        const uint64_t s = rs::vtn_isqrt(d);
        CHECK(s * s <= d && d < (s + 1) * (s + 1));
    }
}

void test_pixel() {
    g_case = "pixel";
    CHECK(rs::vtn_pixel(9, 9 * 50, 9 * 2500, 50, 32) == 128);            // D == 0
    CHECK(rs::vtn_pixel(2, 255, 65025, 255, 127) == 255);                // s = 255, q = 127: the clamp's edge
    CHECK(rs::vtn_pixel(2, 255, 65025, 0, 127) == 1);                    // 128 - 127
    CHECK(rs::vtn_pixel(225, 255, 65025, 255, 127) == 255);              // one bright pixel of 225: clamped
    CHECK(rs::vtn_pixel(225, 224 * 255, 224 * 65025, 0, 127) == 0);      // one dark pixel of 225: clamped
    CHECK(rs::vtn_extent(0, 10, 7) == 8 && rs::vtn_extent(9, 10, 7) == 8 && rs::vtn_extent(5, 7, 7) == 7);
    CHECK(rs::vtn_extent(20, 64, 3) == 7 && rs::vtn_extent(0, 1, 1) == 1);
}

void test_images() {
    static const int shapes[][2] = {{64, 32}, {24, 10}, {16, 5}, {10, 7}, {7, 10}, {33, 35}, {1, 9}, {9, 1}, {1, 1},
                                    {70, 13}};
    static const int radii[] = {1, 3, 7}, gains[] = {1, 32, 127};
    static char label[96];
    for (const auto& sh : shapes)
        for (const int R : radii)
            for (const int G : gains)
                for (int kind = 0; kind < 5; ++kind) {
                    const int H = sh[0], W = sh[1];
                    std::snprintf(label, sizeof label, "%dx%d R=%d G=%d kind %d", H, W, R, G, kind);
                    g_case = label;
                    const auto src = image(H, W, kind);
                    std::unique_ptr<uint8_t[]> dst(new uint8_t[(size_t)H * W]);
                    rs::vtn_normalise_host(H, W, R, G, src.get(), dst.get());
                    long bad = 0;
                    for (int r = 0; r < H; ++r)
                        for (int c = 0; c < W; ++c)
                            bad += dst[(size_t)r * W + c] != brute(H, W, R, G, src.get(), r, c);
                    CHECK(bad == 0);
                    if (kind == 1)
                        for (int i = 0; i < H * W; ++i) CHECK(dst[i] == 128);
                }
}

}  // namespace

int main() {
    test_isqrt();
    test_pixel();
    test_images();
    std::printf("vt_norm rule: %ld checks, %ld failed\n", g_checks, g_failed);
    return g_failed == 0 ? 0 : 1;
}
