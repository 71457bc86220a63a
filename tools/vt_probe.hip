// Diagnostic probe for the bit-plane template scan (not part of the library).
// Builds view_templates.hip with its VT_STAMP hook defined so every wave of vt_scan_plane_kernel
// stamps the ends of its phases (realtime 100 MHz; hw ids and shader clock at the first and
// last), then reports, per launch (dense, list pass B1, list pass B2), the kernel span, the
// median and p90 of every phase and of the block's whole life, waves per SIMD and the clock.
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -Iinclude -Ipyratslam_amd/csrc \
//         -mllvm -amdgpu-atomic-optimizer-strategy=None -mllvm -amdgpu-sched-strategy=max-ilp \
//         tools/vt_probe.hip pyratslam_amd/csrc/rs_common.cpp -lrccl -o tools/vt_probe
// usage: vt_probe [templates = 1000] [queries = 1024] [hit_frac = 0]
//   hit_frac > 0: that share of the queries are stored templates (exact hits), as the
//   headline mix (10240 queries, 0.9, RS_VT_PRUNE=1) has them.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <random>
#include <vector>

// the library's per-wave stamp hook (view_templates.hip leaves it empty).  A wave's record:
// [0..6] realtime at the slots, [7] realtime at kernel entry, [8] shader clock at slot 0,
// [9] shader clock at slot 6, [10] hw ids.  A launch's records lie in the region its list
// pointer names (0 dense, 1 pass B1, 2 pass B2: list 2 starts at vt_dbg_list2).
constexpr int VT_REC = 11;
constexpr size_t VT_REGION = 1 << 16;   // waves per region
__device__ unsigned long long* vt_dbg;
__device__ const int* vt_dbg_list2;
#define VT_STAMP_BEGIN() const unsigned long long vt_t_entry_ = __builtin_amdgcn_s_memrealtime()
#define VT_STAMP_KNOWN()                                                                   \
    do {                                                                                   \
        VT_STAMP(0);                                                                       \
        if ((threadIdx.x & 63) == 0) {                                                     \
            const size_t reg_ = ids == nullptr ? 0 : ids >= vt_dbg_list2 ? 2 : 1;          \
            const size_t w_ = (size_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); \
            if (w_ < VT_REGION) vt_dbg[(reg_ * VT_REGION + w_) * VT_REC + 7] = vt_t_entry_; \
        }                                                                                  \
    } while (0)
#define VT_STAMP(slot)                                                                     \
    do {                                                                                   \
        if ((threadIdx.x & 63) == 0) {                                                     \
            const size_t reg_ = ids == nullptr ? 0 : ids >= vt_dbg_list2 ? 2 : 1;          \
            const size_t w_ = (size_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); \
            if (w_ < VT_REGION) {                                                          \
                unsigned long long* d_ = vt_dbg + (reg_ * VT_REGION + w_) * VT_REC;        \
                d_[slot] = __builtin_amdgcn_s_memrealtime();                               \
                if ((slot) == 0) {                                                         \
                    unsigned hw_, xcc_;                                                    \
                    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw_));      \
                    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc_));    \
                    d_[8] = __builtin_amdgcn_s_memtime();                                  \
                    d_[10] = ((unsigned long long)xcc_ << 32) | hw_;                       \
                }                                                                          \
                if ((slot) == 6) d_[9] = __builtin_amdgcn_s_memtime();                     \
            }                                                                              \
        }                                                                                  \
    } while (0)
#ifdef VT_PROBE_SOURCE   // a stamped copy of another revision's view_templates.hip (A/B)
#include VT_PROBE_SOURCE
#else
#include "view_templates.hip"
#endif

static void pct(const char* name, std::vector<double>& v) {
    if (v.empty()) {
        printf("  %-34s (none)\n", name);
        return;
    }
    std::sort(v.begin(), v.end());
    printf("  %-34s median %7.2f  p90 %7.2f  max %7.2f  (n %zu)\n", name, v[v.size() / 2], v[v.size() * 9 / 10],
           v.back(), v.size());
}

int main(int argc, char** argv) {
    const int T = argc > 1 ? atoi(argv[1]) : 1000, Q = argc > 2 ? atoi(argv[2]) : 1024;
    const double hit = argc > 3 ? atof(argv[3]) : 0.0;
    const int H = 64, W = 32;
    rs_vt* h = nullptr;
    if (rs_vt_create(H, W, 8, 45000, T, 0, &h) != RS_OK) {
        fprintf(stderr, "create: %s\n", rs_last_error());
        return 1;
    }
    std::mt19937 rng(1);
    std::vector<uint8_t> lib((size_t)T * H * W), qs((size_t)Q * H * W);
    for (auto& b : lib) b = (uint8_t)rng();
    for (auto& b : qs) b = (uint8_t)rng();
    for (int q = 0; q < Q; ++q)   // hits: a stored template, unchanged
        if ((rng() & 0xFFFF) < hit * 65536.0)
            memcpy(&qs[(size_t)q * H * W], &lib[(size_t)(rng() % T) * H * W], (size_t)H * W);
    if (rs_vt_add(h, T, lib.data(), nullptr) != RS_OK) return 1;
    const size_t nrec = 3 * VT_REGION;
    unsigned long long* dbg;
    if (hipMalloc(&dbg, nrec * VT_REC * 8) != hipSuccess) return 1;
    hipMemset(dbg, 0, nrec * VT_REC * 8);
    hipMemcpyToSymbol(HIP_SYMBOL(vt_dbg), &dbg, sizeof(dbg));
    const int* none = reinterpret_cast<const int*>(~(uintptr_t)0);
    hipMemcpyToSymbol(HIP_SYMBOL(vt_dbg_list2), &none, sizeof(none));
    std::vector<uint64_t> sc(Q);
    std::vector<int64_t> ix(Q);
    std::vector<uint8_t> nw(Q);
    for (int rep = 0; rep < 5; ++rep) {
        if (rep == 4) {   // the stamps of the last repetition only; list 2 follows list 1's pairs
            hipDeviceSynchronize();
            hipMemset(dbg, 0, nrec * VT_REC * 8);
            if (h->dList.get()) {
                const int* l2 = h->dList.get() + (size_t)h->pruneNtb * Q;
                hipMemcpyToSymbol(HIP_SYMBOL(vt_dbg_list2), &l2, sizeof(l2));
            }
            hipDeviceSynchronize();
        }
        if (rs_vt_match_batch(h, Q, rep ? nullptr : qs.data(), RS_VT_FROZEN, sc.data(), ix.data(),
                              nw.data()) != RS_OK) {
            fprintf(stderr, "match: %s\n", rs_last_error());
            return 1;
        }
    }
    hipDeviceSynchronize();
    std::vector<unsigned long long> d(nrec * VT_REC);
    hipMemcpy(d.data(), dbg, d.size() * 8, hipMemcpyDeviceToHost);
    printf("templates %d  queries %d  hit_frac %.2f\n", T, Q, hit);
    static const char* region_name[3] = {"dense", "list pass B1", "list pass B2"};
    for (int reg = 0; reg < 3; ++reg) {
        const unsigned long long* base = &d[(size_t)reg * VT_REGION * VT_REC];
        unsigned long long t0 = ~0ull, t1 = 0;
        std::vector<double> life, clk, p_cnt, p_take, p_stage, p_planes, p_first, p_rest, p_end, pro;
        std::map<unsigned long long, std::vector<std::pair<unsigned long long, unsigned long long>>> simd;
        int nwaves = 0;
        for (size_t i = 0; i < VT_REGION; ++i) {
            const unsigned long long* e = base + i * VT_REC;
            if (!e[0] || !e[6]) continue;
            ++nwaves;
            t0 = std::min(t0, e[7]);
            t1 = std::max(t1, e[6]);
            const auto us = [](unsigned long long a, unsigned long long b) { return ((double)b - (double)a) * 0.01; };
            life.push_back(us(e[7], e[6]));
            clk.push_back((double)(e[9] - e[8]) / ((double)(e[6] - e[0]) * 10.0));  // GHz
            p_cnt.push_back(us(e[7], e[0]));
            if (e[2] && e[3]) {   // the block had a batch
                if ((i & 7) == 0 && e[1]) p_take.push_back(us(e[0], e[1]));   // wave 0 takes
                p_stage.push_back(us(e[0], e[2]));
                p_planes.push_back(us(e[0], e[3]));
                const unsigned long long ready = std::max(e[2], e[3]);
                pro.push_back(us(e[7], ready));
                if (e[4]) p_first.push_back(us(ready, e[4]));
                if (e[4] && e[5]) p_rest.push_back(us(e[4], e[5]));
                if (e[5]) p_end.push_back(us(e[5], e[6]));
            }
            const unsigned hw = (unsigned)e[10], xcc = (unsigned)(e[10] >> 32);
            const unsigned long long key = ((unsigned long long)xcc << 16) | ((hw >> 13) & 7) << 12 |
                                           ((hw >> 12) & 1) << 11 | ((hw >> 8) & 15) << 4 | ((hw >> 4) & 3);
            simd[key].push_back({e[7], e[6]});
        }
        if (!nwaves) continue;
        printf("[%s] waves %d  stamped span %.1f us\n", region_name[reg], nwaves, (t1 - t0) * 0.01);
        printf(" phases, us per wave:\n");
        pct("entry -> count known", p_cnt);
        pct("count known -> take returned (w0)", p_take);
        pct("count known -> first batch staged", p_stage);
        pct("count known -> planes landed", p_planes);
        pct("entry -> ready to compute", pro);
        pct("ready -> first batch computed", p_first);
        pct("first -> last batch computed", p_rest);
        pct("last batch computed -> end", p_end);
        pct("whole life (entry -> end)", life);
        std::sort(clk.begin(), clk.end());
        printf(" shader clock GHz (per wave): median %.2f\n", clk[clk.size() / 2]);
        std::map<int, int> hist;
        double busy = 0;
        for (auto& kv : simd) {
            hist[(int)kv.second.size()]++;
            for (auto& p : kv.second) busy += (double)(p.second - p.first);
        }
        printf(" SIMDs seen %zu; waves per SIMD histogram:", simd.size());
        for (auto& kv : hist) printf("  %d:%d", kv.first, kv.second);
        printf("\n avg concurrent waves per SIMD seen (over span) %.2f\n", busy / simd.size() / (double)(t1 - t0));
    }
    rs_vt_destroy(h);
    return 0;
}
