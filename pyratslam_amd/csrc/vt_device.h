// What several scan families of the uint8 view-template matcher share: the offset range of
// the fast forms, the packed-key reductions, the byte-SWAR pair, the output of a scan and the
// per-wave stamp hooks.
// Part of view_templates.hip, the one translation unit: not free-standing (it relies on the
// includes, the anonymous namespace and the headers that view_templates.hip includes before it).
#pragma once

constexpr int FAST_M = 8;  // ViewTemplate.max_offset (view_templates.py:14)
constexpr unsigned long long NO_KEY = ~0ull;

__device__ inline unsigned long long wave_min_u64(unsigned long long v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned long long o = __shfl_xor(v, off);
        v = o < v ? o : v;
    }
    return v;
}

__device__ inline uint32_t wrapped_pair(uint32_t aL, uint32_t aH, uint2 f, uint32_t acc) {
    return __builtin_amdgcn_sad_u8(__builtin_amdgcn_bitop3_b32(aL + f.x, aH, f.y, 0x96), 0u, acc);
}

// Output of a scan: either min-reduce packed keys per query (best[]) or
// write every (query, slot) score into a matrix.
struct ScanOut {
    unsigned long long* best;  // [nq] packed keys (MATRIX == false)
    uint32_t* mat;             // [nq][ld]          (MATRIX == true)
    int64_t ld;
    // plane scan, MATRIX == false: the block that finishes last hands the keys to the
    // host words and resets them (vt_keys_export folded in); done counts the blocks
    unsigned long long* host = nullptr;
    unsigned* done = nullptr;
};

template <bool MATRIX>
__device__ inline void emit_score(const ScanOut& out, int64_t slot, int64_t count, int qi, int nq,
                                  uint32_t score, int rank, int nranks, bool lane0_after_reduce) {
    if constexpr (MATRIX) {
        if (slot < count && qi < nq) out.mat[(size_t)qi * out.ld + slot] = score;
    } else {
        const unsigned long long g = (unsigned long long)slot * nranks + rank;
        unsigned long long key = slot < count ? (((unsigned long long)score << 32) | g) : NO_KEY;
        key = wave_min_u64(key);
        if (lane0_after_reduce && qi < nq) atomicMin(out.best + qi, key);
    }
}

// Per-wave stamp hook, empty in the library: tools/vt_probe.hip defines it (realtime at
// the phase ends of every wave of the plane scan, hw ids) before it includes view_templates.hip.
// VT_STAMP_BEGIN: kernel entry; VT_STAMP_KNOWN (slot 0): the list's length known and the
// block stays; then slots 1 the first take returned, 2 first
// batch staged (past the prologue's barrier), 3 this wave's template planes landed, 4 first
// batch computed, 5 last batch computed, 6 end.  Every site has `ids` in scope (the probe
// tells the launches apart by it).
#ifndef VT_STAMP
#define VT_STAMP_BEGIN() \
    do {                 \
    } while (0)
#define VT_STAMP_KNOWN() \
    do {                 \
    } while (0)
#define VT_STAMP(slot) \
    do {               \
    } while (0)
#endif

// Wave-wide minimum as a wave-uniform value, without the LDS pipe (the prefilter's pace
// is set by its LDS reads, and a shuffle is a ds_bpermute): four DPP steps leave each
// row of 16 lanes its minimum (lanes ^1, ^2, then the row's other half-row and the
// other half mirrored), and the four rows meet through scalar registers.
__device__ __forceinline__ uint32_t wave_min_u32_dpp(uint32_t v) {
    v = min(v, (uint32_t)__builtin_amdgcn_update_dpp((int)v, (int)v, 0xB1, 0xF, 0xF, false));    // quad_perm [1,0,3,2]
    v = min(v, (uint32_t)__builtin_amdgcn_update_dpp((int)v, (int)v, 0x4E, 0xF, 0xF, false));    // quad_perm [2,3,0,1]
    v = min(v, (uint32_t)__builtin_amdgcn_update_dpp((int)v, (int)v, 0x141, 0xF, 0xF, false));   // row_half_mirror
    v = min(v, (uint32_t)__builtin_amdgcn_update_dpp((int)v, (int)v, 0x140, 0xF, 0xF, false));   // row_mirror
    return min(min((uint32_t)__builtin_amdgcn_readlane((int)v, 0), (uint32_t)__builtin_amdgcn_readlane((int)v, 16)),
               min((uint32_t)__builtin_amdgcn_readlane((int)v, 32), (uint32_t)__builtin_amdgcn_readlane((int)v, 48)));
}
