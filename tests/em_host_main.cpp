// Stand-alone host test of the linked experience map's host side: rs::em_build_incidence
// (em_rule.h) and rs_em_relax_host (experience_map.hip), which runs the per-experience
// function the kernels run.  It makes no device call, so it needs no GPU;
// tests/test_linked_experience_map.py builds it together with experience_map.hip and
// rs_common.cpp, the host side with -fsanitize=address,undefined, and runs it.  Every array
// is a heap block of exactly the documented size, so a write or read past an end is the
// sanitizer's to report.  Exit status 0: every check held.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>

#include "em_rule.h"
#include "ratslam_abi.h"

namespace {

int g_checks = 0, g_failed = 0;

#define CHECK(cond)                                                        \
    do {                                                                   \
        ++g_checks;                                                        \
        if (!(cond)) {                                                     \
            ++g_failed;                                                    \
            std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); \
        }                                                                  \
    } while (0)

uint64_t g_rng = 0x9E3779B97F4A7C15ull;
uint32_t rnd() {
    g_rng ^= g_rng << 13;
    g_rng ^= g_rng >> 7;
    g_rng ^= g_rng << 17;
    return (uint32_t)(g_rng >> 32);
}
double uni(double lo, double hi) { return lo + (hi - lo) * (rnd() / 4294967296.0); }

struct Graph {
    int n = 0;
    std::vector<rs::EmLink> lk;
    std::vector<double> pose;
};

Graph random_graph(int n, int nl) {
    Graph g;
    g.n = n;
    for (int i = 0; i < n; ++i) {
        g.pose.push_back(uni(-3, 3));
        g.pose.push_back(uni(-3, 3));
        g.pose.push_back(uni(-7, 7));   // unwrapped headings too
    }
    for (int l = 0; l < nl && n > 1; ++l) {
        const int a = (int)(rnd() % n);
        int b = (int)(rnd() % n);
        if (b == a) b = (a + 1) % n;
        g.lk.push_back({a, b, uni(0, 2), uni(-4, 4), uni(-4, 4)});
    }
    return g;
}

// The lists of one graph: exact sizes, every segment complete and in ascending link id.
void check_incidence(const Graph& g) {
    const int n = g.n, nl = (int)g.lk.size();
    std::unique_ptr<int32_t[]> off(new int32_t[2 * (size_t)n + 1]), adj(new int32_t[2 * (size_t)nl + (nl ? 0 : 1)]);
    std::unique_ptr<rs::EmLink[]> lk(new rs::EmLink[nl ? nl : 1]);
    for (int l = 0; l < nl; ++l) lk[l] = g.lk[l];
    rs::em_build_incidence(n, nl, lk.get(), off.get(), adj.get());
    CHECK(off[0] == 0 && off[2 * n] == 2 * nl);
    for (int i = 0; i < n; ++i) {
        int want_a = 0, want_b = 0;
        for (int l = 0; l < nl; ++l) {
            want_a += lk[l].a == i;
            want_b += lk[l].b == i;
        }
        CHECK(off[2 * i + 1] - off[2 * i] == want_a);
        CHECK(off[2 * i + 2] - off[2 * i + 1] == want_b);
        for (int k = off[2 * i]; k < off[2 * i + 1]; ++k) {
            CHECK(adj[k] >= 0 && adj[k] < nl && lk[adj[k]].a == i);
            CHECK(k == off[2 * i] || adj[k - 1] < adj[k]);
        }
        for (int k = off[2 * i + 1]; k < off[2 * i + 2]; ++k) {
            CHECK(adj[k] >= 0 && adj[k] < nl && lk[adj[k]].b == i);
            CHECK(k == off[2 * i + 1] || adj[k - 1] < adj[k]);
        }
    }
}

// The sweep written directly over the link list (no incidence lists).
void naive_relax(const Graph& g, std::vector<double>& p, int loops, double c) {
    const int n = g.n;
    std::vector<double> q(p.size());
    for (int it = 0; it < loops; ++it) {
        for (int i = 0; i < n; ++i) {
            double s[3] = {0.0, 0.0, 0.0}, e[3];
            int deg = 0;
            for (int side = 0; side < 2; ++side)
                for (const rs::EmLink& l : g.lk) {
                    if ((side ? l.b : l.a) != i) continue;
                    rs::em_residual(p.data(), l, e[0], e[1], e[2]);
                    for (int k = 0; k < 3; ++k) s[k] = side ? s[k] - e[k] : s[k] + e[k];
                    ++deg;
                }
            for (int k = 0; k < 3; ++k) q[3 * i + k] = p[3 * i + k];
            if (!deg) continue;
            const double w = c / (double)deg;
            q[3 * i] = p[3 * i] + w * s[0];
            q[3 * i + 1] = p[3 * i + 1] + w * s[1];
            q[3 * i + 2] = rs::em_wrap(p[3 * i + 2] + w * s[2]);
        }
        p.swap(q);
    }
}

int relax_host(const Graph& g, double* xyth, int loops, double c) {
    const int nl = (int)g.lk.size();
    std::unique_ptr<int32_t[]> a(new int32_t[nl ? nl : 1]), b(new int32_t[nl ? nl : 1]);
    std::unique_ptr<double[]> d(new double[nl ? nl : 1]), h(new double[nl ? nl : 1]), f(new double[nl ? nl : 1]);
    for (int l = 0; l < nl; ++l) {
        a[l] = g.lk[l].a; b[l] = g.lk[l].b; d[l] = g.lk[l].d; h[l] = g.lk[l].h; f[l] = g.lk[l].f;
    }
    return rs_em_relax_host(g.n, nl, a.get(), b.get(), d.get(), h.get(), f.get(), xyth, loops, c);
}

void check_relax(const Graph& g, int loops) {
    std::vector<double> want = g.pose;
    naive_relax(g, want, loops, 0.5);
    std::unique_ptr<double[]> got(new double[g.pose.size() ? g.pose.size() : 1]);
    if (!g.pose.empty()) std::memcpy(got.get(), g.pose.data(), sizeof(double) * g.pose.size());
    CHECK(relax_host(g, got.get(), loops, 0.5) == RS_OK);
    CHECK(g.pose.empty() || std::memcmp(got.get(), want.data(), sizeof(double) * want.size()) == 0);
}

}  // namespace

int main() {
    const int shapes[][2] = {{0, 0}, {1, 0}, {2, 1}, {3, 7}, {17, 40}, {64, 0}, {301, 300}, {257, 1500}};
    for (const auto& s : shapes) {
        const Graph g = random_graph(s[0], s[1]);
        check_incidence(g);
        for (int loops : {0, 1, 2, 9}) check_relax(g, loops);
    }
    {   // a hub: every link at experience 0, alternating direction
        Graph g = random_graph(301, 0);
        for (int i = 1; i <= 300; ++i)
            g.lk.push_back({i % 2 ? 0 : i, i % 2 ? i : 0, uni(0, 2), uni(-4, 4), uni(-4, 4)});
        check_incidence(g);
        check_relax(g, 5);
    }
    {   // the wrap: -6.29 comes back as -6.29 + 2pi, not as +6.27
        CHECK(rs::em_wrap(-6.29) < 0.0 && rs::em_wrap(-6.29) > -0.01);
        CHECK(rs::em_wrap(0.5) == 0.5);
        CHECK(rs::em_wrap(rs::EM_TWO_PI) == 0.0);
    }
    {   // refusals: nothing is written
        Graph g = random_graph(4, 3);
        std::vector<double> p = g.pose;
        for (int bad = 0; bad < 3; ++bad) {
            Graph q = g;
            if (bad == 0) q.lk[1].a = 4;
            if (bad == 1) q.lk[2].b = -1;
            if (bad == 2) q.lk[0].b = q.lk[0].a;
            CHECK(relax_host(q, p.data(), 3, 0.5) == RS_ERR_ARG);
            CHECK(rs_last_error()[0] != 0);
            CHECK(p == g.pose);
        }
        CHECK(relax_host(g, p.data(), -1, 0.5) == RS_ERR_ARG);
        CHECK(rs_em_relax_host(2, 1, nullptr, nullptr, nullptr, nullptr, nullptr, p.data(), 1, 0.5) == RS_ERR_ARG);
        CHECK(rs_em_relax_host(2, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 1, 0.5) == RS_ERR_ARG);
        CHECK(rs_em_relax_host(0, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 1, 0.5) == RS_OK);
    }
    std::printf("em_host: %d checks, %d failed\n", g_checks, g_failed);
    return g_failed ? 1 : 0;
}
